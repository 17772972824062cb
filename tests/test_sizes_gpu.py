"""Parity at the sizes the bench lines are quoted on (VERDICT r02 "sizes the goldens do not reach").

  * test_b64_12_layers_two_steps_vs_oracle       configs[4]'s batch (B = 64: M = 23 680 rows, other tile plans / XCD grids
                                                 than B = 32), bf16 path, against the fp32 oracle: losses + update parity.
  * test_fp8_b64_12_layers_vs_oracle             configs[4] itself: fp8 backbone products, 12 layers, B = 64, against the
                                                 ORACLE (not the bf16 engine) with the tolerances stated in the docstring.
  * test_albef_full_size_b8_four_steps_vs_oracle configs[3]'s real architecture at B = 8 for 4 train_steps.
  * test_gemm_production_shapes_per_element      K1 on the five shapes that carry the step's FLOPs, all epilogues, checked
                                                 PER ELEMENT (|out - ref| <= atol + rtol |ref|): the max/max figure of
                                                 test_gemm_epilogues is blind to errors confined to small outputs.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import albef_oracle as A
from oracle import feddat_oracle as O
from tests.golden_util import assert_update_parity

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(b):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import engine
    return engine


def _names(P):
    return O.trainable_names(P, "art", 0) + [n for n in O.trainable_names(P, "art", 1) if "adapter_1" in n]


def test_b64_12_layers_two_steps_vs_oracle(engine):
    B, res = 64, 384
    d = O.ViltDims(layers=12)
    P = O.make_params(d, ["art"], bias_std=0.02)
    P0 = {k: v.clone() for k, v in P.items()}
    eng = engine.ViltDatEngine(P, ["art"], DEV, batch=B, res=res, layers=12)
    client = O.DatClient(P, d, "art", lr=1e-4, steps_per_epoch=2)       # lambda = 0, 1/3, 2/3, 1 over the two batches
    eng.begin_local_update("art", steps_per_epoch=2)
    torch.set_num_threads(min(torch.get_num_threads(), 64))
    for s in range(2):
        b = O.synthetic_batch(B, res, 6464 + s)
        ref = float(client.train_step(b)[0])
        out = eng.train_step(_dev(b), use_graph=(s == 1))
        torch.cuda.synchronize()
        assert abs(float(out[0]) - ref) < 2e-3 * abs(ref) + 2e-3, (s, float(out[0]), ref)
        assert abs(float(out[2]) - client.last_L0) < 2e-3 * abs(client.last_L0) + 2e-3
        assert abs(float(eng.loss_buf["p1"][2]) - client.last_L1) < 2e-3 * abs(client.last_L1) + 2e-3
    worst = assert_update_parity(_names(P), eng.state_dict(), P, P0, 1e-3, 0.1, "B=64")
    print("B=64 12-layer bf16, 2 steps: worst (max |ddW|, mean ratio)", worst)


def test_fp8_b64_12_layers_vs_oracle(engine):
    """configs[4] at its own size against the fp32 ORACLE.  Stated tolerances of the fp8 path (e4m3 operands, 3 mantissa
    bits, for the forward QKV / FFN1 / FFN2 products and the dX products FFN2^T / FFN1^T / attention-output^T of all 12 layers;
    everything else as the bf16 path):
        logits          max |diff| < 0.12              (measured 0.108; four-product form 0.069; bf16 path at this size: < 3e-2)
        losses          within 1.5 % per step          (bf16: 0.2 %)
        adapter / head  per tensor, on the UPDATE dW:  max |ddW| < 1e-3 (measured 3.9e-4: the north-star bound on the
        update          weights still holds over two steps), mean |ddW| <= 0.2 mean |dW_ref| (measured 0.119; four-product
                        form 0.086; bf16 path 0.011 on the same batches), cosine(dW, dW_ref) > 0.9 (measured 0.926; 0.954)
    i.e. the direction of every update is the reference's, its element-wise noise is ~10x the bf16 path's.  Six of the eight
    frozen products per layer run on the fp8 MFMA here (QKV, FFN1, FFN2 forward; FFN2^T, FFN1^T, attention-output^T backward);
    `fp8_ffn_chain=False` gives the four-product form of the start of round 3."""
    B, res = 64, 384
    d = O.ViltDims(layers=12)
    P = O.make_params(d, ["art"], bias_std=0.02)
    P0 = {k: v.clone() for k, v in P.items()}
    eng = engine.ViltDatEngine(P, ["art"], DEV, batch=B, res=res, layers=12, fp8=True)
    torch.set_num_threads(min(torch.get_num_threads(), 64))
    b0 = O.synthetic_batch(B, res, 6400)
    with torch.no_grad():
        _, rl = O.vilt_forward(P, d, b0, "gating", "art")
    _, l8 = eng.forward(_dev(b0), "gating", "art")
    dl = float((l8.cpu() - rl).abs().max())
    print(f"fp8 B=64 12 layers: logits max diff vs oracle {dl:.4f}")
    assert dl < 0.12
    client = O.DatClient(P, d, "art", lr=1e-4, steps_per_epoch=2)
    eng.begin_local_update("art", steps_per_epoch=2)
    for s in range(2):
        b = O.synthetic_batch(B, res, 6464 + s)
        ref = float(client.train_step(b)[0])
        out = eng.train_step(_dev(b), use_graph=(s == 1))
        torch.cuda.synchronize()
        assert abs(float(out[0]) - ref) < 1.5e-2 * abs(ref), (s, float(out[0]), ref)
    sd = eng.state_dict()
    worst_max, worst_ratio, worst_cos = 0.0, 0.0, 1.0
    for n in _names(P):
        d_ref, d_got = (P[n] - P0[n]).flatten(), (sd[n].cpu() - P0[n]).flatten()
        if float(d_ref.abs().max()) == 0:
            continue
        err = (d_got - d_ref).abs()
        ratio = float(err.mean() / d_ref.abs().mean())
        cos = float(torch.dot(d_got, d_ref) / (d_got.norm() * d_ref.norm()))
        worst_max, worst_ratio, worst_cos = max(worst_max, float(err.max())), max(worst_ratio, ratio), min(worst_cos, cos)
        assert float(err.max()) < 1e-3 and ratio < 0.2 and cos > 0.9, (n, float(err.max()), ratio, cos)
    print(f"fp8 B=64 12 layers, 2 steps vs oracle: worst max |ddW| {worst_max:.2e}, mean ratio {worst_ratio:.3f}, "
          f"cosine {worst_cos:.3f}")


def _albef_full_size_vs_oracle(B, steps, seed0, graph_from, max_bound=1e-3, ratio_bound=0.15, what="", operands="bf16"):
    """configs[3]'s real architecture: `steps` train_steps of an AlbefDatEngine at batch B next to the oracle stepping the same
    batches (the round's own schedule: steps_per_epoch = steps); losses every step, updates of every trainable tensor at the end."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import albef_engine
    d = A.AlbefDims()
    P = A.make_params(d)
    P0 = {k: v.clone() for k, v in P.items()}
    eng = albef_engine.AlbefDatEngine(P, DEV, batch=B, n_answers=B, operands=operands)
    client = A.AlbefDatClient(P, d, lr=1e-4, steps_per_epoch=steps)
    eng.begin_local_update(steps_per_epoch=steps)
    torch.set_num_threads(min(torch.get_num_threads(), 64))
    for s in range(steps):
        b = A.synthetic_batch(B, d, seed0 + s)
        ref = float(client.train_step(b))
        out = eng.train_step(_dev(b), use_graph=(s >= graph_from))
        torch.cuda.synchronize()
        assert abs(float(out[0]) - ref) < 3e-3 * ref, (s, float(out[0]), ref)
        assert abs(float(out[2]) - client.last_L0) < 3e-3 * abs(client.last_L0)
    sd = eng.state_dict()
    worst_max, worst_ratio, moved = 0.0, 0.0, 0.0
    for k in A.trainable_names(P, 0) + A.trainable_names(P, 1):
        d_ref, d_got = P[k] - P0[k], sd[k].cpu() - P0[k]
        err, move = (d_got - d_ref).abs(), float(d_ref.abs().mean())
        assert float(err.max()) < max_bound, (k, float(err.max()))
        assert float(err.mean()) <= ratio_bound * move, (k, float(err.mean()), move)
        worst_max, worst_ratio = max(worst_max, float(err.max())), max(worst_ratio, float(err.mean()) / move)
        moved = max(moved, float(d_ref.abs().max()))
    print(f"ALBEF full size {what}B={B}, {steps} steps: worst max |ddW| {worst_max:.2e}, worst mean ratio {worst_ratio:.3f}, "
          f"the reference path moves the weights by up to {moved:.2e}")
    return worst_max, worst_ratio, moved


@pytest.mark.parametrize("operands", ["bf16", "f16"])
def test_albef_full_size_b8_four_steps_vs_oracle(operands):
    """(both operand formats; fp16 = the fp16 library + 2^14 loss scale through feddat_lm_loss_fwd_bwd's grad_scale.)  ViT-B/16 (577 tokens) + BERT-base 12 + 6 layers + 30 522-way head at B = 8 (4 616-row image GEMMs: the large-M tile
    plans, not the few-row kernel a B = 2 test exercises), 4 train_steps (eager, then hipGraph replay)."""
    mx, ratio, _ = _albef_full_size_vs_oracle(8, 4, 880, graph_from=2, operands=operands, what=f"({operands} operands) ")
    if operands == "f16":
        assert ratio < 0.03, ratio


def test_albef_bench_size_b32_two_steps_vs_oracle():
    """The size `bench.py --workload albef` runs (B = 32 per client: 18 464-row image products on the 160- / 224-row tile plans,
    800-row text and 128-row answer streams): two train_steps, eager then hipGraph replay, against the oracle."""
    _albef_full_size_vs_oracle(32, 2, 4300, graph_from=1, what="(the bench's size) ")


def test_albef_full_size_round_of_20_steps_vs_oracle():
    """A 20-step round of the full-size model (B = 4; schedule of a 20-batch loader: 30 warm-up ticks = 15 batches, the last
    5 batches at the peak lr): north_star's bound on every adapter tensor of the 30 modules after the round."""
    _, _, moved = _albef_full_size_vs_oracle(4, 20, 6100, graph_from=1, ratio_bound=0.12, what="round, ")
    assert moved > 5e-4


@pytest.mark.parametrize("seed0", [7700, 8800])
@pytest.mark.parametrize("operands", ["f16", "bf16"])
def test_albef_full_size_round_of_40_steps_vs_reference_golden(golden_dir, operands, seed0):
    """Round 6 (G11b): the REFERENCE's own 40-step round of the full-size ALBEF (ALBEFContinualLearner + TaskTrainer.train_step,
    albef_model.py:69-145, task_trainer.py:280-330; ViT-B/16 at 384, BERT-base 12 + 6 layers, vocab 30522; B = 4, 25-token
    questions, one 4-token answer each; num_epochs = 15: 600 scheduler ticks, 60 warm-up ticks, the last 10 batches at the
    peak lr; oracle/make_albef_golden.py --only-g11b -> tests/golden/g11b_albef_full_round40.npz) replayed on AlbefDatEngine as
    one hipGraph per step: north_star's 1e-3 on the reference's samples of all 240 adapter_0 / adapter_1 tensors after 20 and
    40 steps, plus bulk statistics and the loss trajectory.  Both operand formats.  seed0 = 8800: a second, independent round of the
    reference (other batches; --only-g11b --seed0 8800 -> g11b_albef_full_round40_seed8800.npz)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import albef_engine
    from tests.golden_util import load
    import os as _os
    name = "g11b_albef_full_round40" + ("" if seed0 == 7700 else f"_seed{seed0}") + ".npz"
    if not _os.path.exists(_os.path.join(golden_dir, name)):
        pytest.skip("fixture not generated")
    g = load(golden_dir, name)
    steps, B = int(g["steps"]), int(g["batch"])
    assert (steps, B) == (40, 4)
    d = A.AlbefDims()
    P = A.make_params(d)
    P0 = {k: v.clone() for k, v in P.items()}
    eng = albef_engine.AlbefDatEngine(P, DEV, batch=B, n_answers=B, operands=operands)
    eng.begin_local_update(steps_per_epoch=steps, num_epochs=15)
    keys = [k.split("::", 2)[2] for k in g if k.startswith("s40::dsamp::")]
    assert len(keys) == 240
    losses = []
    for s in range(steps):
        out = eng.train_step(_dev(A.synthetic_batch(B, d, seed0 + s)), use_graph=True)
        losses.append(float(out[0]))
        if s + 1 not in (20, 40):
            continue
        n, sd = s + 1, eng.state_dict()
        worst = dict(max=0.0, ratio=0.0, norm=0.0, moved=0.0, over=0)
        for k in keys:
            dw = (sd[k].cpu() - P0[k]).flatten()
            ref = torch.from_numpy(g[f"s{n}::dsamp::{k}"])
            err = (dw[torch.linspace(0, dw.numel() - 1, min(1024, dw.numel())).long()] - ref).abs()
            worst["max"] = max(worst["max"], float(err.max()))
            worst["ratio"] = max(worst["ratio"], float(err.mean()) / max(float(ref.abs().mean()), 1e-12))
            worst["norm"] = max(worst["norm"], abs(float(dw.norm()) - float(g[f"s{n}::dnorm::{k}"])) / float(g[f"s{n}::dnorm::{k}"]))
            worst["moved"] = max(worst["moved"], float(g[f"s{n}::dmax::{k}"]))
            worst["over"] += int((err > 1e-3).sum())
        print(f"ALBEF full size, {operands}, seed0 {seed0}, {n} steps vs the reference's round: max |ddW| {worst['max']:.2e}, mean ratio "
              f"{worst['ratio']:.4f}, norm {worst['norm']:.4f}, samples > 1e-3: {worst['over']}, the reference moves the adapters by up "
              f"to {worst['moved']:.2e}")
        assert worst["moved"] > (3e-4 if n == 20 else 1.5e-3)
        assert worst["max"] < 1e-3 and worst["over"] == 0, (operands, n, worst)
        assert worst["ratio"] < (0.05 if operands == "f16" else 0.12) and worst["norm"] < (0.02 if operands == "f16" else 0.05), (operands, n, worst)
    rel = np.abs(np.array(losses) - g["losses"]) / np.maximum(np.abs(g["losses"]), 1.0)
    print("ALBEF full-size round: loss trajectory worst rel diff", float(rel.max()))
    assert rel.max() < 1e-2


PROD = [(11840, 2304, 768), (11840, 768, 768), (11840, 3072, 768), (11840, 768, 3072), (11840, 768, 2304)]


@pytest.mark.parametrize("M,N,K", PROD)
def test_gemm_production_shapes_per_element(M, N, K):
    """Reference = fp64 product of the (exactly representable) bf16 operands.  bf16 outputs: half an ulp of bf16 is 2^-9
    relative, the fp32 accumulation over K <= 3072 adds ~1e-6 relative to sqrt(K)-sized sums -> rtol 2^-8, atol 2e-4 (the
    packed-polynomial GELU's own max error is 5e-5; GELU' is within 3.2e-4 absolute, which the product turns into an extra
    4e-4 |x| for that epilogue).  fp32 outputs: rtol 2e-5, atol 2e-4."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import lib as L
    L.load()
    g = torch.Generator(device="cpu").manual_seed(M + 3 * N + 7 * K)
    Ah = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    Bh = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    resid = torch.randn(M, N, generator=g).to(DEV)
    aux = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)
    ref = (Ah.double() @ Bh.double().t())

    def check(out, want, rtol, atol, what, extra=None):
        e = (out.double() - want).abs()
        bound = atol + rtol * want.abs()
        if extra is not None:
            bound = bound + extra
        bad = e > bound
        assert not bool(bad.any()), (what, M, N, K, int(bad.sum()), float((e - bound).max()))

    o16 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    u16 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    o32 = torch.empty(M, N, device=DEV)
    RT16, AT = 2.0 ** -8, 2e-4
    L.gemm_bf16_nt(Ah, Bh, L.EPI_BF16, bias=bias, out_bf16=o16)
    check(o16, ref + bias.double(), RT16, AT, "bf16")
    L.gemm_bf16_nt(Ah, Bh, L.EPI_RESID_F32, bias=bias, resid=resid, out_f32=o32)
    check(o32, ref + bias.double() + resid.double(), 2e-5, AT, "resid_f32")
    L.gemm_bf16_nt(Ah, Bh, L.EPI_GELU, bias=bias, out_bf16=o16, out2_bf16=u16)
    check(u16, ref + bias.double(), RT16, AT, "gelu.u")
    check(o16, F.gelu(ref + bias.double()), RT16, AT, "gelu.f")
    L.gemm_bf16_nt(Ah, Bh, L.EPI_MUL_DGELU, aux=aux, out_bf16=o16)
    a64 = aux.double().requires_grad_(True)
    F.gelu(a64).sum().backward()
    # the packed-polynomial GELU' is within 3.2e-4 ABSOLUTE of the exact derivative: that error is multiplied by |x|
    check(o16, ref * a64.grad, RT16, AT, "mul_dgelu", extra=4e-4 * ref.abs())
    L.gemm_bf16_nt(Ah, Bh, L.EPI_F32, bias=bias, out_f32=o32)
    check(o32, ref + bias.double(), 2e-5, AT, "f32")
    torch.cuda.synchronize()


GELU_CODE_SHAPES = [(11840, 3072, 768, False), (5920, 3072, 768, False), (1030, 192, 64, False), (11840, 3072, 768, True)]


@pytest.mark.parametrize("M,N,K,fp8", GELU_CODE_SHAPES)
def test_gemm_gelu_code_epilogues(M, N, K, fp8):
    """FEDDAT_EPI_GELU_G8 / FEDDAT_EPI_MUL_G8 (8-bit gelu' codes in place of the bf16 u).  Against the fp64 product:
      codes   within 1 of round((gelu'(u) - LO) / STEP) everywhere, equal on > 97 % (the packed-polynomial gelu' is within
              3.2e-4 = 0.064 steps of the exact derivative, so only values near a rounding boundary may differ);
      gelu    the bf16 output as in the plain GELU epilogue;
      . code  out = (A B^T) * (LO + STEP * code) per element to bf16 rounding -- i.e. exact in the code it was given;
      end to end: (A B^T) * decode(encode(gelu'(u))) differs from (A B^T) * gelu'(u) by at most STEP / 2 + 3.2e-4 relative to
              |A B^T| -- the stated 2.5e-3 bound of the header."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import lib as L
    L.load()
    g = torch.Generator(device="cpu").manual_seed(5 * M + N + K)
    Af = torch.randn(M, K, generator=g)
    Bf = torch.randn(N, K, generator=g) * (1.5 / K ** 0.5)
    bias = torch.randn(N, generator=g).to(DEV)
    if fp8:
        A8, B8 = torch.empty(M, K, dtype=torch.uint8, device=DEV), torch.empty(N, K, dtype=torch.uint8, device=DEV)
        sa, sb = torch.empty(M, device=DEV), torch.empty(N, device=DEV)
        L.quant_rows_fp8(Af.to(DEV), A8, sa)
        L.quant_rows_fp8(Bf.to(DEV), B8, sb)
        Ad = A8.view(torch.float8_e4m3fn).double() * sa.double()[:, None]
        Bd = B8.view(torch.float8_e4m3fn).double() * sb.double()[:, None]
    else:
        Ah, Bh = Af.to(torch.bfloat16).to(DEV), Bf.to(torch.bfloat16).to(DEV)
        Ad, Bd = Ah.double(), Bh.double()
    ref = Ad @ Bd.t()
    u = (ref + bias.double()).requires_grad_(True)
    F.gelu(u).sum().backward()
    gp = u.grad
    f16 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    code = torch.empty(M, N, dtype=torch.uint8, device=DEV)
    if fp8:
        L.gemm_fp8_nt(A8, sa, B8, sb, L.EPI_GELU_G8, bias=bias, out_bf16=f16, out2_bf16=code)
    else:
        L.gemm_bf16_nt(Ah, Bh, L.EPI_GELU_G8, bias=bias, out_bf16=f16, out2_bf16=code)
    want = torch.round((gp - L.G8_LO) / L.G8_STEP)
    dc = (code.double() - want).abs()
    assert float(dc.max()) <= 1, float(dc.max())
    assert float((dc == 0).double().mean()) > 0.97
    fg = F.gelu(u.detach())
    assert bool(((f16.double() - fg).abs() <= 2e-4 + 2.0 ** -8 * fg.abs()).all())
    dec = L.G8_LO + L.G8_STEP * code.double()
    assert float((dec - gp).abs().max()) <= L.G8_STEP / 2 + 4e-4
    # . code on a fresh product (the FFN2^T shape is the transpose role: same kernel, aux = codes)
    o16 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    if fp8:
        L.gemm_fp8_nt(A8, sa, B8, sb, L.EPI_MUL_G8, aux=code, out_bf16=o16)
    else:
        L.gemm_bf16_nt(Ah, Bh, L.EPI_MUL_G8, aux=code, out_bf16=o16)
    w = ref * dec
    assert bool(((o16.double() - w).abs() <= 2e-4 + 2.0 ** -8 * w.abs()).all())
    if fp8:
        # the e4m3-output forms (configs[4]'s FFN chain).  e4m3: 3 mantissa bits -> half an ulp = 2^-4 relative; below
        # 2^-6 x scale the grid is uniform with step 2^-9 x scale
        f8 = torch.empty(M, N, dtype=torch.uint8, device=DEV)
        code2 = torch.empty_like(code)
        L.gemm_fp8_nt(A8, sa, B8, sb, L.EPI_GELU_G8_F8, bias=bias, out_bf16=f8, out2_bf16=code2)
        assert torch.equal(code2, code)
        fdec = f8.view(torch.float8_e4m3fn).double() * L.F8_ACT_SCALE
        fsat = fg.clamp(-448 * L.F8_ACT_SCALE, 448 * L.F8_ACT_SCALE)
        assert bool(((fdec - fsat).abs() <= 2.0 ** -4 * fsat.abs() + 2.0 ** -10 * L.F8_ACT_SCALE + 2e-4).all())   # + the packed GELU's own 5e-5
        d8 = torch.empty(M, N, dtype=torch.uint8, device=DEV)
        L.gemm_fp8_nt(A8, sa, B8, sb, L.EPI_MUL_G8_F8, aux=code, out_bf16=d8)
        rs = (L.F8_GRAD_HEADROOM * sa.double())[:, None]                       # the row scale the output carries
        ddec = d8.view(torch.float8_e4m3fn).double() * rs
        assert float((w.abs() / rs).max()) < 448                              # no saturation on this input
        assert bool(((ddec - w).abs() <= 2.0 ** -4 * w.abs() + 2.0 ** -10 * rs + 2e-4).all())      # 2e-4: fp32 accumulation, as above
        # fp8 product with fp32 output + residual
        resid = torch.randn(M, N, generator=g).to(DEV)
        o32 = torch.empty(M, N, device=DEV)
        L.gemm_fp8_nt_f32(A8, sa, B8, sb, bias=bias, resid=resid, out_f32=o32)
        want32 = ref + bias.double() + resid.double()
        assert bool(((o32.double() - want32).abs() <= 2e-4 + 2e-5 * want32.abs()).all())
        L.gemm_fp8_nt_f32(A8, sa, B8, sb, out_f32=o32)
        assert bool(((o32.double() - ref).abs() <= 2e-4 + 2e-5 * ref.abs()).all())
    torch.cuda.synchronize()


def test_gemm_gelu_code_epilogues_need_the_persistent_kernel():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import lib as L
    L.load()
    A = torch.zeros(512, 64, dtype=torch.bfloat16, device=DEV)
    B = torch.zeros(192, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(L.FeddatHipError):
        L.gemm_bf16_nt(A, B, L.EPI_GELU_G8, out_bf16=torch.empty(512, 192, dtype=torch.bfloat16, device=DEV),
                       out2_bf16=torch.empty(512, 192, dtype=torch.uint8, device=DEV))
