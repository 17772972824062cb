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


PROMPT_LEN = 5      # main.py:214


def prompt_tensor_init(key: str, shape, generator, device="cpu") -> torch.Tensor:
    """torch's defaults for the modules of a prompt MLP: Embedding N(0, 1); Linear weight and bias U(+-1 / sqrt(fan_in))."""
    if key.endswith("0.weight"):
        return torch.randn(shape, generator=generator, device=device)
    if len(shape) == 2:
        fan_in = shape[1]
    else:      # a bias: Linear 1 maps H -> H / 4 (its bias has H / 4 elements), Linear 3 maps H / 4 -> H
        fan_in = shape[0] * 4 if key.endswith("1.bias") else shape[0] // 4
    bound = 1.0 / fan_in ** 0.5
    return (2.0 * torch.rand(shape, generator=generator, device=device) - 1.0) * bound


def prompt_init(seed: int = 0, hidden: int = 768, device="cpu") -> Dict[str, torch.Tensor]:
    """The ten prompt tensors (vis first, state-dict order) drawn by prompt_tensor_init from one generator seeded with `seed`."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    shapes = param_shapes(0, (), hidden=hidden, optimizer_mode="prompt")
    return {k: prompt_tensor_init(k, s, g, device) for k, s in shapes.items() if ".prompt_embedding_" in k}


def task_num_labels(task: str) -> int:
    return TASK_NUM_LABELS.get(task, DEFAULT_NUM_LABELS)


def param_shapes(layers: int = 12, tasks: Sequence[str] = ("art",), hidden: int = 768, inter: int = 3072,
                 patch: int = 32, grid: int = 12, max_text: int = 40, vocab: int = 30522, num_labels: int = 100,
                 bottleneck: int = 48, optimizer_mode: str = "dat") -> Dict[str, Tuple[int, ...]]:
    """optimizer_mode "dat": adapter_{0,1,2} in every layer; "adapter": the single `adapter` (main.py:114-118); "bias" / "norm":
    the plain backbone, no adapter (these modes add no parameters); "prompt": the plain backbone with the reference's two prompt
    modules behind the embeddings' own tensors (main.py:214-229), identical shapes for vis and text."""
    H, I, r = hidden, inter, bottleneck
    stems = {"dat": ("adapter_0_", "adapter_1_", "adapter_2_"), "adapter": ("adapter_",), "bias": (), "norm": (),
             "prompt": ()}[optimizer_mode]
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
    if optimizer_mode == "prompt":      # Sequential(Embedding(5, H), Linear(H, H / 4), Tanh(), Linear(H / 4, H)), vis first
        for which in ("vis", "text"):
            p = e + f"prompt_embedding_{which}."
            s[p + "0.weight"], s[p + "1.weight"], s[p + "1.bias"] = (PROMPT_LEN, H), (H // 4, H), (H // 4,)
            s[p + "3.weight"], s[p + "3.bias"] = (H, H // 4), (H,)
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
    per layer, with init_bert_weights' own zero biases.  optimizer_mode "prompt": the prompt modules get torch's own defaults
    (prompt_tensor_init)."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out = {}
    for k, shp in param_shapes(layers, tasks, num_labels=num_labels, optimizer_mode=optimizer_mode).items():
        is_ln = ("LayerNorm" in k) or ("layernorm" in k) or ("clf_norm0" in k)
        if ".prompt_embedding_" in k:
            out[k] = prompt_tensor_init(k, shp, g, device)
        elif optimizer_mode == "adapter" and ".adapter.adapter_" in k and k.endswith("bias"):
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


# ----------------------------------------------------------------------------------------------------------------------
# mixed frames: portrait, landscape and square images in one pixel frame, and the patch-slot layout of their sequences
# ----------------------------------------------------------------------------------------------------------------------
def pad_to_valid(batch: Dict[str, torch.Tensor], valid_hw: Sequence[Tuple[int, int]], text_lens: Sequence[int] = None):
    """What the HF ViLT processor yields for images of different sizes in one frame: sample b keeps the top-left
    valid_hw[b] = (h, w) pixels (multiples of the patch size), the rest is zero with pixel_mask = 0; with text_lens the
    questions are padded ([PAD] = 0, attention_mask = 0) behind text_lens[b] tokens.  Returns a new batch."""
    out = {k: v.clone() for k, v in batch.items()}
    for i, (h, w) in enumerate(valid_hw):
        out["pixel_mask"][i] = 0
        out["pixel_mask"][i, :h, :w] = 1
        out["pixel_values"][i] *= out["pixel_mask"][i][None].to(out["pixel_values"].dtype)
    if text_lens is not None:
        for i, n in enumerate(text_lens):
            out["attention_mask"][i, n:] = 0
            out["input_ids"][i, n:] = 0
    return out


def extend_frame(batch: Dict[str, torch.Tensor], frame: Tuple[int, int]):
    """The same batch in a larger pixel frame: pixel_values and pixel_mask zero-extended to frame = (H, W)."""
    out = dict(batch)
    px, pm = batch["pixel_values"], batch["pixel_mask"]
    n, _, h, w = px.shape
    if frame[0] < h or frame[1] < w:
        raise ValueError(f"frame {frame} is smaller than the batch's {h}x{w}")
    out["pixel_values"] = px.new_zeros(n, 3, frame[0], frame[1])
    out["pixel_values"][:, :, :h, :w] = px
    out["pixel_mask"] = pm.new_zeros(n, frame[0], frame[1])
    out["pixel_mask"][:, :h, :w] = pm
    return out


def orientation_sizes(frame: Tuple[int, int], patch: int = 32):
    """The valid rectangles --synthetic_orientations draws from, inside frame = (H, W): the ViLT size rule's landscape (shorter
    edge 0.6 of the longer), portrait and square, each as large as the frame allows, and a small landscape; multiples of the
    patch size."""
    H, W = frame

    def fit(h, w):
        return max(patch, min(H, h) // patch * patch), max(patch, min(W, w) // patch * patch)
    long_ = max(H, W)
    short = int(long_ * 0.6)
    sizes = [fit(short, long_), fit(long_, short), fit(min(H, W) * 3 // 4, min(H, W) * 3 // 4), fit(short // 2, long_ * 3 // 4)]
    return sizes


def synthetic_mixed_batch(B: int, frame, seed: int, device="cpu", text_len: int = 40, num_labels: int = 100,
                          label_prior: torch.Tensor = None, sizes: Sequence[Tuple[int, int]] = None):
    """synthetic_batch in a frame = (H, W) (an int: square) whose samples draw their valid rectangle from `sizes` (default:
    orientation_sizes(frame)) with a generator seeded by `seed`: zero-padded pixels and the pixel_mask that says so."""
    frame = (frame, frame) if isinstance(frame, int) else tuple(frame)
    sizes = list(sizes) if sizes is not None else orientation_sizes(frame)
    side = max(frame)
    b = synthetic_batch(B, side, seed, "cpu", text_len, num_labels, label_prior)
    b["pixel_values"] = b["pixel_values"][:, :, :frame[0], :frame[1]].contiguous()
    b["pixel_mask"] = b["pixel_mask"][:, :frame[0], :frame[1]].contiguous()
    g = torch.Generator(device="cpu")
    g.manual_seed(seed + 0x5EED)
    pick = torch.randint(0, len(sizes), (B,), generator=g).tolist()
    b = pad_to_valid(b, [sizes[i] for i in pick])
    return {k: v.to(device) for k, v in b.items()}


def patch_slot_plan(patch_mask: torch.Tensor, max_patches: int):
    """The patch-slot layout (include/feddat_hip.h, "PATCH SLOTS") restated on the host.  patch_mask: [B, gh, gw], the pixel
    mask at the patch origins.  Sample b's valid rectangle is vh x vw = the valid patch rows of patch column 0 times the valid
    patch columns of patch row 0; slot j < min(vh * vw, max_patches) holds grid cell (j / vw, j % vw), as the flat index
    (j / vw) * gw + j % vw; the slots behind are empty (-1).
    Returns (cells int64 [B, max_patches], counts int64 [B] = vh * vw, overflow bool [B] = counts > max_patches)."""
    pm = torch.as_tensor(patch_mask).cpu() != 0
    B, gh, gw = pm.shape
    if not 1 <= max_patches <= gh * gw:
        raise ValueError(f"max_patches must lie in 1 .. {gh * gw}, got {max_patches}")
    vh, vw = pm[:, :, 0].sum(1), pm[:, 0, :].sum(1)
    counts = (vh * vw).to(torch.int64)
    cells = torch.full((B, max_patches), -1, dtype=torch.int64)
    for b in range(B):
        n, w = min(int(counts[b]), max_patches), int(vw[b])
        if n:
            j = torch.arange(n)
            cells[b, :n] = (j // w) * gw + j % w
    return cells, counts, counts > max_patches
