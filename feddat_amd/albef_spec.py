"""State-dict keys / shapes of the reference's ALBEF dual-adapter model (ALBEFContinualLearner.albef_model.albef:
VisionTransformer with an Adapter per block, src/modeling/models/vit.py:79-110; BertModel / BertLMHeadModel whose BertOutput
holds an Adapter, src/modeling/models/xbert.py:429-445; built by src/modeling/models/albef_model.py:13-43) and a random
initialiser of that architecture (no network for ALBEF.pth / bert-base-uncased here: benchmarks use random-init weights of the
real shapes).  The LM-head decoder weight is the decoder's word-embedding matrix (tied), so it has no entry of its own."""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

PRE = "albef_model.albef."
# the adapters every module carries, per optimizer_mode: what follows "<module>.adapter." in a key, up to "down" / "up"
ADAPTER_STEMS = {"dat": ("adapter_0_", "adapter_1_", "adapter_2_"), "adapter": ("adapter_",)}


def param_shapes(vit_depth: int = 12, enc_layers: int = 12, fusion_layer: int = 6, dec_layers: int = 6, image: int = 384,
                 patch: int = 16, hidden: int = 768, inter: int = 3072, vocab: int = 30522, max_pos: int = 512,
                 bottleneck: int = 48, optimizer_mode: str = "dat") -> Dict[str, Tuple[int, ...]]:
    """optimizer_mode "dat": three adapters per module (adapter_{0,1,2}_{down,up}); "adapter": the single-adapter FedAvg build
    (adapter_config names = ["adapter"], main.py:114-118), one adapter_down / adapter_up pair per module.  Backbone and LM head
    are the same."""
    if optimizer_mode not in ("dat", "adapter"):
        raise ValueError(f"ALBEF is built for optimizer_mode 'dat' or 'adapter', got {optimizer_mode!r}")
    H, I, r = hidden, inter, bottleneck
    s: Dict[str, Tuple[int, ...]] = {}
    stems = ADAPTER_STEMS[optimizer_mode]

    def adapters(base):
        for stem in stems:
            s[f"{base}{stem}down.weight"] = (r, H)
            s[f"{base}{stem}down.bias"] = (r,)
            s[f"{base}{stem}up.weight"] = (H, r)
            s[f"{base}{stem}up.bias"] = (H,)

    v = PRE + "visual_encoder."
    s[v + "cls_token"] = (1, 1, H)
    s[v + "pos_embed"] = (1, (image // patch) ** 2 + 1, H)
    s[v + "patch_embed.proj.weight"] = (H, 3, patch, patch)
    s[v + "patch_embed.proj.bias"] = (H,)
    for i in range(vit_depth):
        b = f"{v}blocks.{i}."
        for n, shp in (("norm1.weight", (H,)), ("norm1.bias", (H,)), ("attn.qkv.weight", (3 * H, H)), ("attn.qkv.bias", (3 * H,)),
                       ("attn.proj.weight", (H, H)), ("attn.proj.bias", (H,)), ("norm2.weight", (H,)), ("norm2.bias", (H,)),
                       ("mlp.fc1.weight", (I, H)), ("mlp.fc1.bias", (I,)), ("mlp.fc2.weight", (H, I)), ("mlp.fc2.bias", (H,))):
            s[b + n] = shp
        adapters(b + "adapter.")
    s[v + "norm.weight"] = (H,)
    s[v + "norm.bias"] = (H,)
    for tower, layers, fusion in ((PRE + "text_encoder.", enc_layers, fusion_layer), (PRE + "text_decoder.bert.", dec_layers, 0)):
        e = tower + "embeddings."
        s[e + "word_embeddings.weight"] = (vocab, H)
        s[e + "position_embeddings.weight"] = (max_pos, H)
        s[e + "token_type_embeddings.weight"] = (2, H)
        s[e + "LayerNorm.weight"] = (H,)
        s[e + "LayerNorm.bias"] = (H,)
        for i in range(layers):
            Lp = f"{tower}encoder.layer.{i}."
            for blk in (("attention",) + (("crossattention",) if i >= fusion else ())):
                for n in ("query", "key", "value"):
                    s[f"{Lp}{blk}.self.{n}.weight"] = (H, H)
                    s[f"{Lp}{blk}.self.{n}.bias"] = (H,)
                s[f"{Lp}{blk}.output.dense.weight"] = (H, H)
                s[f"{Lp}{blk}.output.dense.bias"] = (H,)
                s[f"{Lp}{blk}.output.LayerNorm.weight"] = (H,)
                s[f"{Lp}{blk}.output.LayerNorm.bias"] = (H,)
            s[Lp + "intermediate.dense.weight"] = (I, H)
            s[Lp + "intermediate.dense.bias"] = (I,)
            s[Lp + "output.dense.weight"] = (H, I)
            s[Lp + "output.dense.bias"] = (H,)
            s[Lp + "output.LayerNorm.weight"] = (H,)
            s[Lp + "output.LayerNorm.bias"] = (H,)
            adapters(Lp + "output.adapter.")
    c = PRE + "text_decoder.cls.predictions."
    s[c + "bias"] = (vocab,)
    s[c + "transform.dense.weight"] = (H, H)
    s[c + "transform.dense.bias"] = (H,)
    s[c + "transform.LayerNorm.weight"] = (H,)
    s[c + "transform.LayerNorm.bias"] = (H,)
    return s


def random_init(seed: int = 0, device="cpu", std: float = 0.02, bias_std: float = 0.02, **dims) -> Dict[str, torch.Tensor]:
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out = {}
    for k, shp in param_shapes(**dims).items():
        is_ln = ("LayerNorm" in k) or (".norm" in k)
        if is_ln and k.endswith("weight"):
            out[k] = 1.0 + bias_std * torch.randn(shp, generator=g, device=device)
        elif k.endswith("bias"):
            out[k] = bias_std * torch.randn(shp, generator=g, device=device)
        else:
            out[k] = std * torch.randn(shp, generator=g, device=device)
    return out


def synthetic_batch(B: int, seed: int, image: int = 384, q_len: int = 25, a_len: int = 4, k: Sequence[int] = None,
                    vocab: int = 30522, device="cpu"):
    """N(0,1) images, questions of q_len tokens ([CLS] ... [SEP]), one (or k[b]) answers per
    question of a_len tokens ([CLS] a b [SEP]), weights 1 -- the reference's batch after tokenisation (albef.py:52-60)."""
    g = torch.Generator().manual_seed(seed)
    k = list(k) if k is not None else [1] * B
    n = sum(k)
    q = torch.randint(1000, min(30000, vocab), (B, q_len), generator=g)
    q[:, 0], q[:, -1] = 101, 102
    a = torch.randint(1000, min(30000, vocab), (n, a_len), generator=g)
    a[:, 0], a[:, -1] = 101, 102
    batch = {"image": torch.randn(B, 3, image, image, generator=g), "question_ids": q,
             "question_mask": torch.ones(B, q_len, dtype=torch.long), "answer_ids": a,
             "answer_mask": torch.ones(n, a_len, dtype=torch.long), "weights": torch.ones(n)}
    out = {kk: v.to(device) for kk, v in batch.items()}
    out["k"] = k
    return out


def synthetic_raw_images(n: int, seed: int, image: int = 384):
    """n decoded RGB images as the image datasets hand them out, before any transform: uint8 [H, W, 3] numpy arrays of mixed
    sizes and orientations, scaled with the engine's image size (at 384: 480 x 640 and 427 x 640 landscape, 640 x 427 portrait, a
    384 x 384 square and a 240 x 320 thumbnail that is up-scaled).  Deterministic in (n, seed, image)."""
    g = torch.Generator().manual_seed(seed)
    shapes = [(480, 640), (640, 427), (384, 384), (427, 640), (240, 320)]
    out = []
    for i in range(n):
        h, w = shapes[int(torch.randint(0, len(shapes), (1,), generator=g))]
        h, w = max(1, h * image // 384), max(1, w * image // 384)
        out.append(torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).numpy())
    return out


def synthetic_answer_list(M: int, a_len: int = 4, vocab: int = 30522, seed: int = 0):
    """A stand-in for the task's tokenised answer list (albef.py:62-64): -> (ids [M, a_len], mask [M, a_len]) int64.  Entry i is
    [CLS] t ... [SEP]; the first tokens t are distinct (rank_answer shortlists by the first token's probability, so two entries with
    the same one would tie), and every third entry is one token shorter, [CLS] ... [SEP] [PAD] with mask 0 on the padding.
    Deterministic in (M, a_len, vocab, seed)."""
    lo, hi = 1000, min(30000, vocab)
    if M < 1 or a_len < 3 or M > hi - lo:
        raise ValueError(f"synthetic_answer_list: need 1 <= M <= {hi - lo} distinct first tokens and a_len >= 3, got M={M}, a_len={a_len}")
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(lo, hi, (M, a_len), generator=g)
    ids[:, 1] = torch.randperm(hi - lo, generator=g)[:M] + lo
    ids[:, 0], ids[:, -1] = 101, 102
    mask = torch.ones(M, a_len, dtype=torch.long)
    if a_len > 3:
        ids[2::3, -2], ids[2::3, -1] = 102, 0
        mask[2::3, -1] = 0
    return ids, mask


def synthetic_eval_loader(Q: int, batch_size: int, seed: int, answer_ids, answer_mask, k: int, image: int = 384, q_len: int = 25,
                          vocab: int = 30522, device="cpu"):
    """Q evaluation questions in batches of batch_size, the LAST ONE SHORT when Q is no multiple (the reference's eval loader keeps
    it: vqa_dataset_crossvqa.py:580-603).  Each batch is what ALBEFContinualLearner.forward(train=False) takes -- image, question_ids /
    question_mask, the answer list (answer_list_ids / answer_list_mask, shared by all batches), k -- plus gts: per question 1-3
    indices into the answer list, the ground truth AlbefTaskTrainer.eval_one_loader scores against (task_trainer.py:188-196)."""
    g = torch.Generator().manual_seed(seed)
    M = answer_ids.shape[0]
    answer_ids, answer_mask = answer_ids.to(device), answer_mask.to(device)
    loader = []
    for first in range(0, Q, batch_size):
        n = min(batch_size, Q - first)
        q = torch.randint(1000, min(30000, vocab), (n, q_len), generator=g)
        q[:, 0], q[:, -1] = 101, 102
        img = torch.randn(n, 3, image, image, generator=g)
        gts = [torch.randperm(M, generator=g)[:min(M, 1 + int(torch.randint(0, 3, (1,), generator=g)))].tolist() for _ in range(n)]
        loader.append({"image": img.to(device), "question_ids": q.to(device),
                       "question_mask": torch.ones(n, q_len, dtype=torch.long, device=device), "answer_list_ids": answer_ids,
                       "answer_list_mask": answer_mask, "k": k, "gts": gts})
    return loader
