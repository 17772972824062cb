"""State-dict keys / shapes of the reference model on the hot path (ViltContinualLearner with
Adaptered_ViltOutput in every layer: src/modeling/vilt.py:154-219,356-361; src/modeling/models/adapter.py:22-58;
HF ViltModel with ViltConfig defaults = dandelin/vilt-b32-mlm) and a random initialiser of that architecture
(there is no network for checkpoints: benchmarks use random-init weights of the real shapes)."""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

ENC = "vilt_encoder.vilt."

# Label counts of the reference's task table (src/configs/task_configs_fed.py, 'num_labels'): every CLOVE / domain task answers
# over 100 labels, `vqa` (VQAv2) over 3129.  A task name the table does not hold gets DEFAULT_NUM_LABELS.
DEFAULT_NUM_LABELS = 100
TASK_NUM_LABELS = {
    **{t: 100 for t in ("art", "abstract", "vizwiz", "toronto", "gqa")},
    **{f"clove_scene_{c}": 100 for c in "abcdef"},
    **{f"clove_function_{c}": 100 for c in "abcde"},
    "vqa": 3129,
}


def task_num_labels(task: str) -> int:
    return TASK_NUM_LABELS.get(task, DEFAULT_NUM_LABELS)


def param_shapes(layers: int = 12, tasks: Sequence[str] = ("art",), hidden: int = 768, inter: int = 3072,
                 patch: int = 32, grid: int = 12, max_text: int = 40, vocab: int = 30522, num_labels: int = 100,
                 bottleneck: int = 48, optimizer_mode: str = "dat") -> Dict[str, Tuple[int, ...]]:
    """optimizer_mode "dat": adapter_{0,1,2} in every layer; "adapter": the single `adapter` (main.py:114-118); "bias" / "norm":
    the plain backbone, no adapter (these modes add no parameters)."""
    H, I, r = hidden, inter, bottleneck
    stems = {"dat": ("adapter_0_", "adapter_1_", "adapter_2_"), "adapter": ("adapter_",), "bias": (), "norm": ()}[optimizer_mode]
    s: Dict[str, Tuple[int, ...]] = {}
    e = ENC + "embeddings."
    s[e + "cls_token"] = (1, 1, H)
    s[e + "position_embeddings"] = (1, grid * grid + 1, H)
    s[e + "text_embeddings.word_embeddings.weight"] = (vocab, H)
    s[e + "text_embeddings.position_embeddings.weight"] = (max_text, H)
    s[e + "text_embeddings.token_type_embeddings.weight"] = (2, H)
    s[e + "text_embeddings.LayerNorm.weight"] = (H,)
    s[e + "text_embeddings.LayerNorm.bias"] = (H,)
    s[e + "patch_embeddings.projection.weight"] = (H, 3, patch, patch)
    s[e + "patch_embeddings.projection.bias"] = (H,)
    s[e + "token_type_embeddings.weight"] = (3, H)
    for i in range(layers):
        L = ENC + f"encoder.layer.{i}."
        for n in ("query", "key", "value"):
            s[L + f"attention.attention.{n}.weight"] = (H, H)
            s[L + f"attention.attention.{n}.bias"] = (H,)
        s[L + "attention.output.dense.weight"] = (H, H)
        s[L + "attention.output.dense.bias"] = (H,)
        s[L + "intermediate.dense.weight"] = (I, H)
        s[L + "intermediate.dense.bias"] = (I,)
        # Adaptered_ViltOutput keeps the HF ViltOutput as `.layer`; without an adapter (bias / norm) the HF keys stay as they are
        out = "output.layer.dense." if stems else "output.dense."
        s[L + out + "weight"] = (H, I)
        s[L + out + "bias"] = (H,)
        for stem in stems:
            A = L + f"output.adapter.{stem}"
            s[A + "down.weight"] = (r, H)
            s[A + "down.bias"] = (r,)
            s[A + "up.weight"] = (H, r)
            s[A + "up.bias"] = (H,)
        for ln in ("layernorm_before", "layernorm_after"):
            s[L + ln + ".weight"] = (H,)
            s[L + ln + ".bias"] = (H,)
    s[ENC + "layernorm.weight"] = (H,)
    s[ENC + "layernorm.bias"] = (H,)
    s[ENC + "pooler.dense.weight"] = (H, H)
    s[ENC + "pooler.dense.bias"] = (H,)
    for t in tasks:
        s[f"task_layer.{t}.clf_fc0.weight"] = (2 * H, H)
        s[f"task_layer.{t}.clf_fc0.bias"] = (2 * H,)
        s[f"task_layer.{t}.clf_norm0.weight"] = (2 * H,)
        s[f"task_layer.{t}.clf_norm0.bias"] = (2 * H,)
        s[f"task_layer.{t}.clf_fc1.weight"] = (num_labels, 2 * H)
        s[f"task_layer.{t}.clf_fc1.bias"] = (num_labels,)
    return s


def random_init(layers: int = 12, tasks: Sequence[str] = ("art",), seed: int = 0, device="cpu",
                std: float = 0.02, bias_std: float = 0.02, optimizer_mode: str = "dat",
                num_labels: int = 100) -> Dict[str, torch.Tensor]:
    """BERT-style init (adapter.py:5-14: N(0, 0.02) weights, LayerNorm 1/0) -- biases get a small N(0, bias_std)
    instead of exact zeros so that every bias path of the kernels is exercised.  optimizer_mode "adapter": the single adapter
    per layer, with init_bert_weights' own zero biases."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out = {}
    for k, shp in param_shapes(layers, tasks, num_labels=num_labels, optimizer_mode=optimizer_mode).items():
        is_ln = ("LayerNorm" in k) or ("layernorm" in k) or ("clf_norm0" in k)
        if optimizer_mode == "adapter" and ".adapter.adapter_" in k and k.endswith("bias"):
            out[k] = torch.zeros(shp, device=device)
        elif is_ln and k.endswith("weight"):
            out[k] = 1.0 + bias_std * torch.randn(shp, generator=g, device=device)
        elif k.endswith("bias"):
            out[k] = bias_std * torch.randn(shp, generator=g, device=device)
        else:
            out[k] = std * torch.randn(shp, generator=g, device=device)
    return out


def client_label_prior(client: int, num_labels: int = 100, alpha: float = 0.5, seed: int = 1234) -> torch.Tensor:
    """Heterogeneous clients: client k draws its answers from its own Dirichlet(alpha = 0.5) prior over
    the labels -- a few answers dominate each client, differently per client, so the clients' gradients disagree the way
    non-IID VQA domains do (the reference's clients are different datasets: vqa_utils.py:21-31,62-67 build the targets)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed + 7919 * int(client))
    p = torch._standard_gamma(torch.full((num_labels,), float(alpha)), generator=g)
    p = p.clamp_min(1e-12)
    return p / p.sum()


def synthetic_batch(B: int, res: int, seed: int, device="cpu", text_len: int = 40, num_labels: int = 100,
                    label_prior: torch.Tensor = None):
    """Synthetic VQA batch in the reference's schema (HF ViLT encodings + target_scores):
    N(0,1) pixels, [CLS] 38 random ids [SEP], 1-3 labels per row with scores in {0.3, 0.6, 0.9, 1.0}; labels uniform, or
    drawn without replacement from `label_prior` (client_label_prior: the heterogeneous clients of config 3)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    px = torch.randn(B, 3, res, res, generator=g)
    ids = torch.randint(1000, 30000, (B, text_len), generator=g)
    ids[:, 0], ids[:, -1] = 101, 102
    target = torch.zeros(B, num_labels)
    scores = torch.tensor([0.3, 0.6, 0.9, 1.0])
    for b in range(B):
        n = int(torch.randint(1, 4, (1,), generator=g))
        if label_prior is None:
            labs = torch.randperm(num_labels, generator=g)[:n]
        else:
            labs = torch.multinomial(label_prior, n, replacement=False, generator=g)
        target[b, labs] = scores[torch.randint(0, 4, (n,), generator=g)]
    batch = {"pixel_values": px, "pixel_mask": torch.ones(B, res, res, dtype=torch.long), "input_ids": ids,
             "attention_mask": torch.ones(B, text_len, dtype=torch.long),
             "token_type_ids": torch.zeros(B, text_len, dtype=torch.long), "target_scores": target}
    return {k: v.to(device) for k, v in batch.items()}
