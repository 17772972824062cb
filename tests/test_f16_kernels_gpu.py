"""The fp16-operand build (libfeddat_hip_f16.so, the default of both engines) kernel by kernel against float64.

That library is compiled from the same sources as the bf16 one with `bf16` = IEEE half (csrc/common.hip.h), so every kernel
that touches the 16-bit type is a different binary there: 2^-11 rounding instead of 2^-8, a range of 65504 instead of 3.4e38,
and a backward that sees gradients multiplied by the loss scale.  tests/test_f16_gpu.py covers the plain GEMM epilogues, the
ViLT attention, layernorm_fwd and the adapter; this module covers the rest of the default path.

  A. op-level parity at the shapes of the bf16 build's own tests (their shape lists are imported, so the two builds cannot drift
     apart), against a float64 restatement on the same fp16-rounded operands.  Every tolerance is at most 1/4 of the bf16 test's
     (a kernel that quietly rounds through bf16 in this build fails) and is stated in the test's docstring with the worst value
     measured on the MI355X.  16-bit copies of an fp32 result are checked BIT-EQUAL to torch's round-to-nearest-even
     .to(torch.float16) of the kernel's own fp32 result or of the fp32 reference.
  B. the loss-scaled range of the backward kernels with 16-bit outputs:
       headroom  the incoming gradient times a power of two s that puts the largest EXACT output in [2^12, 2^13) (or, where
                 the 16-bit incoming gradient would leave fp16's range first, the largest s that keeps it below 2^15): every output
                 finite and equal to s x the unscaled exact result within the kernel's tolerance of A -- a 16-bit intermediate
                 held well above the outputs (attention's dS is converted before its 1/8 score scale) would overflow first;
       overflow  s such that the largest exact output lies in [2^17, 2^18): every element whose exact value exceeds 2^16 (fp16's
                 round-to-nearest-even overflow threshold is 65520) comes out +-inf or NaN, never a finite clamped value, and
                 such a gradient fed through adapter_wgrad_reduce_checked raises the overflow flag the dynamic scaler reads.
  C. direct tests, in both operand builds, of the entry points that had none: layernorm_bwd_dx_sparse, adapter_pack_strided,
     image_embed_assemble_masked, gather_rows, segment_sum_rows, axpby3 and their argument refusals."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import albef_oracle as A
from tests.test_dropout_gpu import ATTN2_DROPOUT_SHAPES, DROPOUT_SHAPES
from tests.test_ops_gpu import ATTN2_SHAPES, ATTN_CLS_SHAPES, ATTN_SHAPES, LAYERNORM_SHAPES, SKINNY_SHAPES
from tests.test_sizes_gpu import GELU_CODE_SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMTS = ("bf16", "f16")
F16_MAX_FINITE = 65504.0
INF_FROM = 2.0 ** 16          # exact values at or above this round to inf under round-to-nearest-even (threshold 65520)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import lib
    lib.load()
    with lib.operands("f16"):
        lib.load()
    return lib


def h(x):
    return x.to(torch.float16)


def rel64(got, want):
    """max |got - want| / max |want| with both in float64."""
    return float((got.double() - want.double()).abs().max() / (want.double().abs().max() + 1e-300))


def _pow2_for(m, top):
    """The power of two s with s * m in [2^top, 2^(top + 1))."""
    return 2.0 ** (top - math.floor(math.log2(m)))


def _flag(L, g16):
    """Feed the rows of a 16-bit gradient (as the fp32 dy of one adapter-wgrad segment) through adapter_wgrad_partial and
    adapter_wgrad_reduce_checked; returns the segment's overflow flag."""
    H, R = 768, 48
    flat = g16.float().flatten()
    bad = (~torch.isfinite(flat)).nonzero()
    start = (int(bad[0]) // H) * H if bad.numel() else 0
    T = 64
    dy = torch.zeros(T * H, device=DEV)
    piece = flat[start:start + T * H]
    dy[:piece.numel()] = piece
    dy = dy.view(T, H)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(T, H, generator=gen).to(DEV)
    z, dz = torch.rand(T, R, generator=gen).to(DEV) + 0.5, torch.randn(T, R, generator=gen).to(DEV)
    n = R * H + R + H * R + H
    stride = L.adapter_wgrad_workspace_elems(1)
    part = torch.empty(stride, device=DEV)
    grad = torch.empty(n, device=DEV)
    ptrs = torch.tensor([grad.data_ptr()], dtype=torch.int64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    with L.operands("f16"):
        L.adapter_wgrad_partial(L.make_wgrad_segs([dict(x=x, dy=dy, z=z, dz=dz, grad=grad, rows=T, scale=1.0)]), part)
        L.adapter_wgrad_reduce_checked(ptrs, 1, 1, part, stride, flags)
    torch.cuda.synchronize()
    return int(flags[0])


def _check_overflowed(L, outs, exact, what):
    """B (overflow): every element whose exact value is >= 2^16 is non-finite, there is at least one, and the checked reduce
    flags the tensor that holds one."""
    n_big = 0
    for o, e in zip(outs, exact):
        big = e.abs() >= INF_FROM * 1.01          # 1 %: the kernel's own error may not carry an exact 65536 below 65520
        n_big += int(big.sum())
        assert not bool(torch.isfinite(o.float()[big]).any()), (what, "a finite value where the exact one overflows fp16")
        if bool(big.any()):
            assert _flag(L, o) == 1, (what, "overflow not flagged")
    assert n_big > 0, (what, "the overflow scale did not reach 2^16")


# ====================================================================================== A. op-level parity
def _attn2_data(B, Sq, Skv, heads, masked, v_scale=1.0):
    g = torch.Generator().manual_seed(Sq * 1000 + Skv)
    H = heads * 64
    q = h(torch.randn(B * Sq, H, generator=g)).to(DEV)
    kv = torch.randn(B * Skv, 2 * H, generator=g)
    kv[:, H:] *= v_scale
    kv = h(kv).to(DEV)
    do = h(torch.randn(B * Sq, H, generator=g)).to(DEV)
    km = None
    if masked:
        km = torch.ones(B, Skv, dtype=torch.uint8)
        for b in range(B):
            km[b, max(1, Skv - 1 - 2 * b):] = 0
        km = km.to(DEV)
    return q, kv, do, km


def _attn2_ref64(q, kv, do, km, B, Sq, Skv, heads, causal, keep=None, p=0.0):
    """float64 attention on the fp16 operands: ctx, lse and the exact dQ, dK, dV for the incoming gradient do."""
    H = heads * 64
    qr = q.double().view(B, Sq, heads, 64).transpose(1, 2).requires_grad_(True)
    kr = kv[:, :H].double().reshape(B, Skv, heads, 64).transpose(1, 2).requires_grad_(True)
    vr = kv[:, H:].double().reshape(B, Skv, heads, 64).transpose(1, 2).requires_grad_(True)
    sc = qr @ kr.transpose(-1, -2) / 8.0
    if km is not None:
        sc = sc + (1.0 - km.double())[:, None, None, :] * -10000.0
    if causal:
        sc = sc + torch.triu(torch.full((Sq, Skv), -10000.0, dtype=torch.float64, device=DEV), diagonal=1)
    pr = sc.softmax(-1)
    if keep is not None:
        pr = pr * (keep.double() / (1.0 - p))
    ctx = (pr @ vr).transpose(1, 2).reshape(B * Sq, H)
    ctx.backward(do.double())
    grads = (qr.grad.transpose(1, 2).reshape(B * Sq, H), kr.grad.transpose(1, 2).reshape(B * Skv, H),
             vr.grad.transpose(1, 2).reshape(B * Skv, H))
    return ctx.detach(), torch.logsumexp(sc, -1).detach(), grads


def _attn2_run(L, q, kv, do, km, B, Sq, Skv, heads, causal, drop=None):
    H = heads * 64
    k, v = kv[:, :H], kv[:, H:]
    ctx = torch.zeros(B * Sq, H, dtype=torch.float16, device=DEV)
    lse = torch.zeros(B, heads, Sq, device=DEV)
    dq = torch.zeros_like(q)
    dkv = torch.zeros_like(kv)
    ws = torch.empty(B, heads, Sq, device=DEV)
    with L.operands("f16"):
        L.attn2_fwd(q, k, v, ctx, lse, B, Sq, Skv, heads, key_mask=km, causal=causal, drop=drop)
        L.attn2_bwd(q, k, v, ctx, lse, do, ws, dq, dkv[:, :H], dkv[:, H:], B, Sq, Skv, heads, key_mask=km, causal=causal,
                    drop=drop)
    torch.cuda.synchronize()
    return ctx, lse, (dq, dkv[:, :H], dkv[:, H:])


@pytest.mark.parametrize("B,Sq,Skv,heads,causal,masked", ATTN2_SHAPES)
def test_attn2_fwd_bwd_fp16(L, B, Sq, Skv, heads, causal, masked):
    """attn2 (the ALBEF attention) at test_ops_gpu's 12 shapes.  Tolerances (bf16 build: 2e-2 / 2e-3 / 2e-2): ctx max abs error
    3e-3, lse 1e-5, max error / max |exact| of dQ 1.1e-3, dK and dV 1.5e-3.  Measured worst over these and the dropout shapes:
    ctx 1.5e-3, lse 1.0e-6, dQ 8.3e-4, dK 9.7e-4, dV 6.0e-4.  The dQ bound is what catches a dS rounded through bf16 before
    the dQ / dK products (measured 1.4e-3 ... 2.9e-3 on dQ with that mutation)."""
    q, kv, do, km = _attn2_data(B, Sq, Skv, heads, masked)
    cref, lref, gref = _attn2_ref64(q, kv, do, km, B, Sq, Skv, heads, causal)
    ctx, lse, grads = _attn2_run(L, q, kv, do, km, B, Sq, Skv, heads, causal)
    e_ctx, e_lse = float((ctx.double() - cref).abs().max()), float((lse.double() - lref).abs().max())
    e_g = [rel64(a, r) for a, r in zip(grads, gref)]
    print(f"attn2 fp16 {(B, Sq, Skv, heads, causal, masked)}: ctx {e_ctx:.2e} lse {e_lse:.2e} dQ/dK/dV",
          " ".join(f"{e:.2e}" for e in e_g))
    assert e_ctx < 3e-3 and e_lse < 1e-5
    for e, name, tol in zip(e_g, ("dQ", "dK", "dV"), (1.1e-3, 1.5e-3, 1.5e-3)):
        assert e < tol, (name, e)


@pytest.mark.parametrize("B,Sq,Skv,heads,causal,masked", ATTN2_DROPOUT_SHAPES)
def test_attn2_dropout_fwd_bwd_fp16(L, B, Sq, Skv, heads, causal, masked):
    """attn2 with dropped probabilities at test_dropout_gpu's shapes, with test_attn2_fwd_bwd_fp16's tolerances (bf16 build:
    2e-2 / 2e-2)."""
    p, step = 0.1, 3
    k0, k1 = L.dropout_keys(5, 1, 9)
    drop = (p, k0, k1, torch.tensor([step, 0], dtype=torch.int32, device=DEV))
    q, kv, do, km = _attn2_data(B, Sq, Skv, heads, masked)
    keep = A.dropout_keep(B * heads * Sq * Skv, p, k0, k1, step).view(B, heads, Sq, Skv).to(DEV)
    cref, lref, gref = _attn2_ref64(q, kv, do, km, B, Sq, Skv, heads, causal, keep=keep, p=p)
    ctx, lse, grads = _attn2_run(L, q, kv, do, km, B, Sq, Skv, heads, causal, drop=drop)
    e_ctx, e_lse = float((ctx.double() - cref).abs().max()), float((lse.double() - lref).abs().max())
    e_g = [rel64(a, r) for a, r in zip(grads, gref)]
    print(f"attn2+dropout fp16 {(B, Sq, Skv, heads, causal, masked)}: ctx {e_ctx:.2e} lse {e_lse:.2e} dQ/dK/dV",
          " ".join(f"{e:.2e}" for e in e_g))
    assert e_ctx < 3e-3 and e_lse < 1e-5
    for e, name, tol in zip(e_g, ("dQ", "dK", "dV"), (1.1e-3, 1.5e-3, 1.5e-3)):
        assert e < tol, (name, e)


def _cls_data(B, S, heads, masked):
    g = torch.Generator().manual_seed(B * S + heads)
    H = heads * 64
    qkv = h(torch.randn(B * S, 3 * H, generator=g) * 0.7).to(DEV)
    km = None
    if masked:
        km = (torch.rand(B, S, generator=g) > 0.3).to(torch.uint8)
        km[:, 0] = 1
        km = km.to(DEV)
    d0 = torch.randn(B, H, generator=g).to(DEV)
    return qkv, km, d0


def _cls_ref64(qkv, km, ctx0, d0, B, S, heads):
    """float64 token-0 attention backward; D uses the stored 16-bit context row, as the kernel does."""
    q4 = qkv.double().view(B, S, 3, heads, 64)
    q0, K, V = q4[:, 0, 0], q4[:, :, 1], q4[:, :, 2]
    sc = torch.einsum("bhd,bshd->bhs", q0, K) / 8.0
    if km is not None:
        sc = sc.masked_fill(km[:, None, :] == 0, float("-inf"))
    p = torch.softmax(sc, -1)
    g0 = d0.double().view(B, heads, 64)
    Dv = (g0 * ctx0.double()).sum(-1, keepdim=True)
    dS = p * (torch.einsum("bhd,bshd->bhs", g0, V) - Dv)
    dV = torch.einsum("bhs,bhd->bshd", p, g0)
    dK = torch.einsum("bhs,bhd->bshd", dS, q0) / 8.0
    dQ0 = torch.einsum("bhs,bshd->bhd", dS, K) / 8.0
    return torch.einsum("bhs,bshd->bhd", p, V), torch.logsumexp(sc, -1), (dQ0, dK, dV)


def _cls_run(L, qkv, km, d0, B, S, heads):
    H = heads * 64
    ctx = torch.zeros(B * S, H, dtype=torch.float16, device=DEV)
    lse = torch.zeros(B, heads, S, device=DEV)
    dqkv = torch.full((B * S, 3 * H), float("nan"), dtype=torch.float16, device=DEV)
    with L.operands("f16"):
        L.attn_cls_fwd(qkv, ctx, lse, B, S, heads, key_mask=km)
        L.attn_cls_bwd(qkv, ctx, lse, d0, dqkv, B, S, heads, key_mask=km)
    torch.cuda.synchronize()
    got = dqkv.view(B, S, 3, heads, 64)
    return ctx, lse, (got[:, 0, 0], got[:, :, 1], got[:, :, 2]), got


@pytest.mark.parametrize("B,S,heads,masked", ATTN_CLS_SHAPES)
def test_attn_cls_fwd_bwd_fp16(L, B, S, heads, masked):
    """attn_cls_fwd / attn_cls_bwd (the top ViLT layer's token-0 attention) at test_ops_gpu's shapes (S = 185, 90, 281, 7).
    Tolerances (bf16 build: 1.5e-2 abs, 1e-4, 1e-2 x max + 1e-4): ctx0 max abs error 3.75e-3, lse 2.5e-5, dQ0 / dK / dV max abs
    error 2.5e-3 x max |exact| + 2.5e-5.  Rows 1.. of the dQ block stay zero.  Measured: printed per shape."""
    qkv, km, d0 = _cls_data(B, S, heads, masked)
    ctx, lse, got, full = _cls_run(L, qkv, km, d0, B, S, heads)
    ctx0 = ctx.view(B, S, heads, 64)[:, 0]
    o0, l0, ref = _cls_ref64(qkv, km, ctx0, d0, B, S, heads)
    e_ctx, e_lse = float((ctx0.double() - o0).abs().max()), float((lse[:, :, 0].double() - l0).abs().max())
    errs = [float((a.double() - r).abs().max()) / (float(r.abs().max()) + 1e-6) for a, r in zip(got, ref)]
    print(f"attn_cls fp16 {(B, S, heads, masked)}: ctx0 {e_ctx:.2e} lse {e_lse:.2e} dQ0/dK/dV (rel. to max)",
          " ".join(f"{e:.2e}" for e in errs))
    assert e_ctx < 3.75e-3 and e_lse < 2.5e-5
    assert not torch.isnan(full.float()).any() and not full[:, 1:, 0].any()
    for a, r, name in zip(got, ref, ("dQ0", "dK", "dV")):
        assert float((a.double() - r).abs().max()) < 2.5e-3 * (float(r.abs().max()) + 1e-6) + 2.5e-5, name


@pytest.mark.parametrize("rows,H", LAYERNORM_SHAPES)
def test_layernorm_backwards_fp16(L, rows, H):
    """layernorm_bwd_dx with fp32 and 16-bit dy, fp32 and 16-bit outputs, with and without dres; layernorm_bwd_full (rows <= 1024).
    Against float64 autograd on the same (fp16-rounded where the kernel reads 16 bits) operands.  Tolerances (bf16 build: 5e-5
    abs, rel 1e-2, 1e-4 x max(1, max)): fp32 outputs max abs error 1.25e-5; 16-bit outputs bit-equal to the fp32 output's RNE
    .to(float16) and max error / max 2.5e-3; dgamma / dbeta 2.5e-5 x max(1, max |exact|).  Measured: printed per shape."""
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, H, generator=g) * 2 + 0.3).to(DEV)
    gamma = (1 + 0.1 * torch.randn(H, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(H, generator=g)).to(DEV)
    eps = 1e-12 if H == 768 else 1e-5
    stats = torch.empty(rows, 2, device=DEV)
    dy = torch.randn(rows, H, generator=g).to(DEV)
    dres = torch.randn(rows, H, generator=g).to(DEV)
    dy16 = h(dy)
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)

    def ref(d):
        xr.grad = gr.grad = br.grad = None
        F.layer_norm(xr, (H,), gr, br, eps).backward(d.double())
        return xr.grad.clone()

    out = torch.empty(rows, H, device=DEV)
    o16 = torch.empty(rows, H, dtype=torch.float16, device=DEV)
    errs = []
    with L.operands("f16"):
        L.layernorm_fwd(x, gamma, beta, eps, rows, H, y_f32=torch.empty(rows, H, device=DEV), stats=stats)
        for dyk, dr in (("f32", dres), ("f32", None), ("f16", dres), ("f16", None)):
            kw = dict(dy_f32=dy) if dyk == "f32" else dict(dy_bf16=dy16)
            L.layernorm_bwd_dx(x, stats, gamma, rows, H, dres=dr, out_f32=out, out_bf16=o16, **kw)
            torch.cuda.synchronize()
            want = ref(dy if dyk == "f32" else dy16.float()) + (dr.double() if dr is not None else 0.0)
            e32, e16 = float((out.double() - want).abs().max()), rel64(o16, want)
            errs.append((dyk, dr is not None, e32, e16))
            assert e32 < 1.25e-5, (dyk, e32)
            assert torch.equal(o16, h(out)), dyk
            assert e16 < 2.5e-3, (dyk, e16)
        if rows <= 1024:
            dx, dg, db = torch.empty(rows, H, device=DEV), torch.empty(H, device=DEV), torch.empty(H, device=DEV)
            L.layernorm_bwd_full(dy, x, stats, gamma, rows, H, dx, dg, db)
            torch.cuda.synchronize()
            want = ref(dy)
            e_dx = float((dx.double() - want).abs().max())
            e_dg = float((dg.double() - gr.grad).abs().max()) / max(1.0, float(gr.grad.abs().max()))
            e_db = float((db.double() - br.grad).abs().max()) / max(1.0, float(br.grad.abs().max()))
            errs.append(("full", e_dx, e_dg, e_db))
            assert e_dx < 1.25e-5 and e_dg < 2.5e-5 and e_db < 2.5e-5
    print(f"layernorm bwd fp16 ({rows}, {H}):", errs)


def test_gelu_fwd_bwd_fp16_build(L):
    """gelu_fwd / gelu_bwd (fp32 in and out) in the fp16 build: BIT-IDENTICAL to the bf16 build's (no 16-bit stage), and against
    float64 within 5e-7 / 2.5e-6 x max(1, |exact|) (bf16 build's test: 1e-6 / 1e-5 absolute against fp32 torch; fp32's own
    rounding keeps the forward from a quarter of it: measured 2.6e-7 / 5.1e-7)."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(100003, generator=g).to(DEV)
    dy = torch.randn(100003, generator=g).to(DEV)
    y = {f: torch.empty_like(x) for f in FMTS}
    dx = {f: torch.empty_like(x) for f in FMTS}
    for f in FMTS:
        with L.operands(f):
            L.gelu_fwd(x, y[f])
            L.gelu_bwd(x, dy, dx[f])
    torch.cuda.synchronize()
    assert torch.equal(y["f16"], y["bf16"]) and torch.equal(dx["f16"], dx["bf16"])
    xr = x.double().requires_grad_(True)
    yr = F.gelu(xr)
    yr.backward(dy.double())
    e_y = float(((y["f16"].double() - yr).abs() / yr.detach().abs().clamp(min=1)).max())
    e_dx = float(((dx["f16"].double() - xr.grad).abs() / xr.grad.abs().clamp(min=1)).max())
    print(f"gelu fp16 build: fwd {e_y:.2e} bwd {e_dx:.2e} (error / max(1, |exact|)); absolute "
          f"{float((y['f16'].double() - yr).abs().max()):.2e} / {float((dx['f16'].double() - xr.grad).abs().max()):.2e}")
    assert e_y < 5e-7 and e_dx < 2.5e-6


def _adapter_params(L, fmt, seed):
    gen = torch.Generator().manual_seed(seed)
    dt = L.OPERAND_DTYPE[fmt]
    par = []
    for a in range(3):
        wd = (torch.randn(48, 768, generator=gen) * 0.05).to(DEV)
        wu = (torch.randn(768, 48, generator=gen) * 0.05).to(DEV)
        w = [torch.empty(48, 768, dtype=dt, device=DEV), torch.empty(768, 48, dtype=dt, device=DEV),
             torch.empty(768, 48, dtype=dt, device=DEV), torch.empty(48, 768, dtype=dt, device=DEV)]
        with L.operands(fmt):
            L.adapter_pack(wd, wu, *w)
        par.append(dict(wd=w[0], wdT=w[1], wu=w[2], wuT=w[3], bd=(torch.randn(48, generator=gen) * 0.1).to(DEV),
                        bu=(torch.randn(768, generator=gen) * 0.1).to(DEV)))
    return par


def _adapter_segs(L, par, T):
    hT = 16 * 31 + 5
    return L.make_segs([dict(row_begin=0, row_end=hT, train_slot=0, adapters=[dict(par[0], scale=0.5), dict(par[2], scale=0.5)]),
                        dict(row_begin=hT, row_end=T, train_slot=0, adapters=[dict(par[1], scale=1.0)])])


def test_adapter_fwd_ln_fp16(L):
    """adapter_fwd_ln = adapter_fwd + layernorm_fwd of its output, in the fp16 build, T = 1007 (ragged tail).  The adapter output
    is bit-identical to adapter_fwd's; stats within 2.5e-5 relative (bf16 build: 1e-4); y within one fp16 ulp (2^-10 relative,
    bf16 build: 2^-7) + 2.5e-6 of the separate launches, and both y against the float64 LayerNorm of the adapter output within
    2.5e-3 of max |y| (layernorm_fwd's bf16 bound: 1e-2).  Measured: printed."""
    par = _adapter_params(L, "f16", 21)
    T = 1000 + 7
    x = torch.randn(T, 768, generator=torch.Generator().manual_seed(11)).to(DEV)
    segs = _adapter_segs(L, par, T)
    gg = torch.Generator().manual_seed(12)
    gamma, beta = torch.randn(768, generator=gg).to(DEV), torch.randn(768, generator=gg).to(DEV)
    out_a, out_b = torch.zeros_like(x), torch.zeros_like(x)
    y_a = torch.zeros(T, 768, dtype=torch.float16, device=DEV)
    y_b = torch.zeros_like(y_a)
    st_a, st_b = torch.zeros(T, 2, device=DEV), torch.zeros(T, 2, device=DEV)
    with L.operands("f16"):
        L.adapter_fwd(x, out_a, segs, T)
        L.layernorm_fwd(out_a, gamma, beta, 1e-12, T, 768, y_bf16=y_a, stats=st_a)
        L.adapter_fwd_ln(x, out_b, segs, T, gamma, beta, 1e-12, y_b, st_b)
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b)
    e_st = float((st_a - st_b).abs().max() / st_a.abs().max())
    d = (y_a.double() - y_b.double()).abs()
    e_ulp = float((d / torch.maximum(y_a.double().abs(), y_b.double().abs()).clamp(min=1e-3)).max())
    ref = F.layer_norm(out_a.double(), (768,), gamma.double(), beta.double(), 1e-12)
    e_a, e_b = rel64(y_a, ref), rel64(y_b, ref)
    print(f"adapter_fwd_ln fp16: stats {e_st:.2e}, y fused vs separate (rel, per element) {e_ulp:.2e}, "
          f"vs fp64 {e_a:.2e} / {e_b:.2e}")
    assert e_st < 2.5e-5
    assert bool((d <= torch.maximum(y_a.double().abs(), y_b.double().abs()) * 2 ** -10 + 2.5e-6).all())
    assert e_a < 2.5e-3 and e_b < 2.5e-3


@pytest.mark.parametrize("M,N,K", [s[:3] for s in GELU_CODE_SHAPES if not s[3]])
def test_gemm_gelu_code_epilogues_fp16(L, M, N, K):
    """EPI_GELU_G8 / EPI_MUL_G8 in the fp16 build at test_sizes_gpu's bf16-operand shapes, under that test's code criteria:
    codes within 1 of round((gelu'(u) - LO) / STEP) everywhere and equal on > 97 %; decoded code within STEP / 2 + 4e-4 of
    gelu'(u).  Against the float64 product of the fp16 operands, per element: (A B^T) . decode(code) within 5e-5 + 2^-10 |exact|
    (bf16 build: 2e-4 + 2^-8 |exact|; measured excess over 2^-10 |exact| <= 1.0e-6); the gelu output within 1.5e-4 + 2^-10
    |exact|: its relative term, where a 16-bit rounding shows, is a quarter of the bf16 build's, its absolute term is the
    epilogue polynomial's own error (measured 1.13e-4 over 2^-10 |exact| at all three shapes), which no operand format removes."""
    g = torch.Generator(device="cpu").manual_seed(5 * M + N + K)
    Af = torch.randn(M, K, generator=g)
    Bf = torch.randn(N, K, generator=g) * (1.5 / K ** 0.5)
    bias = torch.randn(N, generator=g).to(DEV)
    Ah, Bh = h(Af).to(DEV), h(Bf).to(DEV)
    ref = Ah.double() @ Bh.double().t()
    u = (ref + bias.double()).requires_grad_(True)
    F.gelu(u).sum().backward()
    gp = u.grad
    f16 = torch.empty(M, N, dtype=torch.float16, device=DEV)
    code = torch.empty(M, N, dtype=torch.uint8, device=DEV)
    o16 = torch.empty(M, N, dtype=torch.float16, device=DEV)
    with L.operands("f16"):
        L.gemm_bf16_nt(Ah, Bh, L.EPI_GELU_G8, bias=bias, out_bf16=f16, out2_bf16=code)
        L.gemm_bf16_nt(Ah, Bh, L.EPI_MUL_G8, aux=code, out_bf16=o16)
    torch.cuda.synchronize()
    dc = (code.double() - torch.round((gp - L.G8_LO) / L.G8_STEP)).abs()
    fg = F.gelu(u.detach())
    dec = L.G8_LO + L.G8_STEP * code.double()
    w = ref * dec
    e_f = float(((f16.double() - fg).abs() - 2.0 ** -10 * fg.abs()).max())
    e_m = float(((o16.double() - w).abs() - 2.0 ** -10 * w.abs()).max())
    print(f"gelu-code fp16 {(M, N, K)}: codes max diff {float(dc.max())}, equal {float((dc == 0).double().mean()):.4f}; "
          f"gelu excess over 2^-10|x| {e_f:.2e}, mul excess {e_m:.2e}")
    assert float(dc.max()) <= 1 and float((dc == 0).double().mean()) > 0.97
    assert float((dec - gp).abs().max()) <= L.G8_STEP / 2 + 4e-4
    assert bool(((f16.double() - fg).abs() <= 1.5e-4 + 2.0 ** -10 * fg.abs()).all())
    assert bool(((o16.double() - w).abs() <= 5e-5 + 2.0 ** -10 * w.abs()).all())


@pytest.mark.parametrize("M,N,K", SKINNY_SHAPES + [(1, 768, 3072)])
def test_gemm_skinny_all_epilogues_fp16(L, M, N, K):
    """The split-K skinny GEMM (M <= 64) in the fp16 build, every epilogue, strided A and residual as the engine passes them, at
    test_ops_gpu's shapes plus M = 1.  Against the float64 product of the fp16 operands.  Tolerances (bf16 build: 2e-2 x max
    |AB^T| for 16-bit outputs, 1e-3 x max + 1e-4 for fp32): 16-bit outputs 5e-3 x max |AB^T|, fp32 outputs 2.5e-4 x max +
    2.5e-5.  Measured: printed per shape."""
    torch.manual_seed(M + N)
    A_ = h(torch.randn(M, 3, K, device=DEV))[:, 0]
    Bw = h(torch.randn(N, K, device=DEV) * 0.03)
    bias = torch.randn(N, device=DEV)
    resid = torch.randn(M, 2, N, device=DEV)[:, 1]
    aux = h(torch.randn(M, N, device=DEV))
    ref = A_.double() @ Bw.double().t()
    rmax = float(ref.abs().max())
    b64 = bias.double()
    u = aux.double().requires_grad_(True)
    F.gelu(u).sum().backward()
    o16, o2 = torch.zeros(M, N, dtype=torch.float16, device=DEV), torch.zeros(M, N, dtype=torch.float16, device=DEV)
    o32 = torch.zeros(M, N, device=DEV)
    errs = {}
    with L.operands("f16"):
        ws = torch.empty(L.gemm_skinny_workspace_elems(M, N, K), device=DEV)
        L.gemm_bf16_nt(A_, Bw, L.EPI_BF16, bias=bias, out_bf16=o16, skinny_workspace=ws)
        errs["bf16"] = float((o16.double() - (ref + b64)).abs().max())
        L.gemm_bf16_nt(A_, Bw, L.EPI_RESID_F32, bias=bias, resid=resid, out_f32=o32, skinny_workspace=ws)
        errs["resid_f32"] = float((o32.double() - (ref + b64 + resid.double())).abs().max())
        L.gemm_bf16_nt(A_, Bw, L.EPI_GELU, bias=bias, out_bf16=o16, out2_bf16=o2, skinny_workspace=ws)
        errs["gelu.u"] = float((o2.double() - (ref + b64)).abs().max())
        errs["gelu"] = float((o16.double() - F.gelu(ref + b64)).abs().max())
        L.gemm_bf16_nt(A_, Bw, L.EPI_MUL_DGELU, aux=aux, out_bf16=o16, skinny_workspace=ws)
        errs["mul_dgelu"] = float((o16.double() - ref * u.grad).abs().max())
        L.gemm_bf16_nt(A_, Bw, L.EPI_F32, out_f32=o32, skinny_workspace=ws)
        errs["f32"] = float((o32.double() - ref).abs().max())
    torch.cuda.synchronize()
    print(f"skinny fp16 {(M, N, K)}: max |AB^T| {rmax:.3f}, errors / max |AB^T|:",
          {k: f"{v / rmax:.2e}" for k, v in errs.items()})
    for k in ("bf16", "gelu.u", "gelu", "mul_dgelu"):
        assert errs[k] < 5e-3 * rmax, k
    for k in ("resid_f32", "f32"):
        assert errs[k] < 2.5e-4 * rmax + 2.5e-5, k


def test_conversions_are_round_to_nearest_even_fp16(L):
    """cvt_f32_bf16 / transpose_f32_bf16 / scatter_cls_rows / im2col_patches in the fp16 build: the 16-bit output is BIT-EQUAL to
    torch's .to(torch.float16) of the fp32 input -- including ties, values past 65504 (inf), fp16 subnormals and signed zeros."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(70 * 130, generator=g) * torch.exp2(torch.randint(-30, 18, (70 * 130,), generator=g).float())
    edge = torch.tensor([65504.0, 65519.0, 65520.0, 70000.0, -1e6, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -14,
                         1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -0.0, 0.0, float("inf"), -float("inf")])
    x[:edge.numel()] = edge
    x = x.to(DEV)
    o = torch.empty(70 * 130, dtype=torch.float16, device=DEV)
    ot = torch.empty(130, 70, dtype=torch.float16, device=DEV)
    with L.operands("f16"):
        L.cvt_f32_bf16(x, o)
        L.transpose_f32_bf16(x.view(70, 130), ot, 70, 130)
        w = torch.randn(768, 3072, generator=g).to(DEV)
        wt = torch.empty(3072, 768, dtype=torch.float16, device=DEV)
        L.transpose_f32_bf16(w, wt, 768, 3072)
        rows = (torch.randn(3, 768, generator=g) * 300).to(DEV)
        o32 = torch.full((15, 768), float("nan"), device=DEV)
        o16 = torch.full((15, 768), float("nan"), dtype=torch.float16, device=DEV)
        L.scatter_cls_rows(rows, o32, o16, 3, 5, 768)
        B, Hi, Wi, P = 2, 96, 64, 32
        pix = (torch.randn(B, 3, Hi, Wi, generator=g) * 3).to(DEV)
        patches = torch.empty(B * (Hi // P) * (Wi // P), 3 * P * P, dtype=torch.float16, device=DEV)
        L.im2col_patches(pix, patches, B, 3, Hi, Wi, P)
    torch.cuda.synchronize()
    assert torch.equal(o.view(torch.int16), h(x).view(torch.int16))           # int16 view: -0 / +0 and inf compared by bits
    assert torch.equal(ot.view(torch.int16), h(x.view(70, 130)).t().contiguous().view(torch.int16))
    assert torch.equal(wt, h(w).t().contiguous())
    exp = torch.zeros(3, 5, 768, device=DEV)
    exp[:, 0] = rows
    assert torch.equal(o32, exp.reshape(15, 768)) and torch.equal(o16, h(o32))
    ref = pix.unfold(2, P, P).unfold(3, P, P).permute(0, 2, 3, 1, 4, 5).reshape(B * (Hi // P) * (Wi // P), 3 * P * P)
    assert torch.equal(patches, h(ref))


@pytest.mark.parametrize("n,p,step", DROPOUT_SHAPES)
def test_dropout_fp16_output(L, n, p, step):
    """feddat_dropout in the fp16 build at test_dropout_gpu's shapes: the oracle's mask; the 16-bit output BIT-EQUAL to the fp32
    reference's RNE .to(float16) (with and without the fused residual), and the fp16 input form exact."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 40
    res = torch.randn(n, generator=g) * 40
    k0, k1 = L.dropout_keys(77, 2, 41)
    ctr = torch.tensor([step, 0], dtype=torch.int32, device=DEV)
    keep = A.dropout_keep(n, p, k0, k1, step)
    scale = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32))
    want = x * (keep.float() * scale)
    out = torch.empty(n, device=DEV)
    o16 = torch.empty(n, dtype=torch.float16, device=DEV)
    with L.operands("f16"):
        L.dropout(x.to(DEV), (p, k0, k1, ctr), out_f32=out, out_bf16=o16)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want) and torch.equal(o16.cpu(), h(want))
        L.dropout(x.to(DEV), (p, k0, k1, ctr), resid=res.to(DEV), out_f32=out, out_bf16=o16)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want + res) and torch.equal(o16.cpu(), h(want + res))
        L.dropout(h(x).to(DEV), (p, k0, k1, None), out_f32=out, out_bf16=o16)
        torch.cuda.synchronize()
    want0 = h(x).float() * (A.dropout_keep(n, p, k0, k1, 0).float() * scale)
    assert torch.equal(out.cpu(), want0) and torch.equal(o16.cpu(), h(want0))


# ====================================================================================== B. loss-scaled range
def _headroom_scale(m, g16):
    """The headroom power of two for exact outputs of max m, unless the 16-bit incoming gradient g16 would leave fp16's range
    first: then the largest power of two that keeps max |g16| s below 2^15."""
    s = _pow2_for(m, 12)
    return min(s, 2.0 ** (14 - math.floor(math.log2(float(g16.abs().max()))))) if g16 is not None else s


def _scaled(t16, s):
    """t16 (fp16) times the power of two s: exact as long as it stays below 65504."""
    r = t16.double() * s
    assert float(r.abs().max()) <= F16_MAX_FINITE, "the scaled incoming gradient must itself be representable"
    return h(r.float())


def _headroom_check(L, outs, exact, s, tol, what):
    errs = []
    for o, e in zip(outs, exact):
        assert bool(torch.isfinite(o.float()).all()), (what, "non-finite output in the headroom range")
        errs.append(rel64(o.double() / s, e))
        assert _flag(L, o) == 0, what
    print(f"headroom {what}: s = 2^{int(math.log2(s))}, max |exact scaled output| "
          f"{max(float(e.abs().max()) for e in exact) * s:.0f}, errors", " ".join(f"{x:.2e}" for x in errs))
    for x in errs:
        assert x < tol, (what, x)


@pytest.mark.parametrize("B,Sq,Skv,heads,causal,masked", ATTN2_SHAPES)
def test_attn2_bwd_loss_scaled_range(L, B, Sq, Skv, heads, causal, masked):
    """B (headroom) for attn2_bwd at every attn2 shape: dQ, dK, dV finite and s x exact within test_attn2_fwd_bwd_fp16's 5e-3."""
    q, kv, do, km = _attn2_data(B, Sq, Skv, heads, masked)
    _, _, gref = _attn2_ref64(q, kv, do, km, B, Sq, Skv, heads, causal)
    s = _headroom_scale(max(float(r.abs().max()) for r in gref), do)
    _, _, grads = _attn2_run(L, q, kv, _scaled(do, s), km, B, Sq, Skv, heads, causal)
    _headroom_check(L, grads, gref, s, 5e-3, f"attn2_bwd {(B, Sq, Skv, heads, causal, masked)}")


@pytest.mark.parametrize("B,Sq,Skv,heads,causal,masked", ATTN2_DROPOUT_SHAPES)
def test_attn2_bwd_dropout_loss_scaled_range(L, B, Sq, Skv, heads, causal, masked):
    """B (headroom) for attn2_bwd with dropout at the dropout shapes, tolerance 5e-3."""
    p, step = 0.1, 3
    k0, k1 = L.dropout_keys(5, 1, 9)
    drop = (p, k0, k1, torch.tensor([step, 0], dtype=torch.int32, device=DEV))
    q, kv, do, km = _attn2_data(B, Sq, Skv, heads, masked)
    keep = A.dropout_keep(B * heads * Sq * Skv, p, k0, k1, step).view(B, heads, Sq, Skv).to(DEV)
    _, _, gref = _attn2_ref64(q, kv, do, km, B, Sq, Skv, heads, causal, keep=keep, p=p)
    s = _headroom_scale(max(float(r.abs().max()) for r in gref), do)
    _, _, grads = _attn2_run(L, q, kv, _scaled(do, s), km, B, Sq, Skv, heads, causal, drop=drop)
    _headroom_check(L, grads, gref, s, 5e-3, f"attn2_bwd+dropout {(B, Sq, Skv, heads, causal, masked)}")


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("B,Sq,Skv,heads,causal,masked", [(3, 25, 25, 12, False, True), (2, 200, 130, 3, False, False)])
def test_attn2_bwd_overflow_is_not_hidden(L, B, Sq, Skv, heads, causal, masked, dropout):
    """B (overflow) for attn2_bwd: V x 32 makes dQ / dK exceed the incoming gradient, so an fp16 dO can drive them past 2^16."""
    q, kv, do, km = _attn2_data(B, Sq, Skv, heads, masked, v_scale=32.0)
    drop, keep, p = None, None, 0.1
    if dropout:
        k0, k1 = L.dropout_keys(5, 1, 9)
        drop = (p, k0, k1, torch.tensor([3, 0], dtype=torch.int32, device=DEV))
        keep = A.dropout_keep(B * heads * Sq * Skv, p, k0, k1, 3).view(B, heads, Sq, Skv).to(DEV)
    _, _, gref = _attn2_ref64(q, kv, do, km, B, Sq, Skv, heads, causal, keep=keep, p=p)
    s = _pow2_for(max(float(r.abs().max()) for r in gref), 17)
    _, _, grads = _attn2_run(L, q, kv, _scaled(do, s), km, B, Sq, Skv, heads, causal, drop=drop)
    _check_overflowed(L, grads, [r * s for r in gref], f"attn2_bwd {(B, Sq, Skv, dropout)}")


def _attn_data(B, S, heads, masked, v_scale=1.0):
    g = torch.Generator().manual_seed(S)
    H = heads * 64
    qkv = torch.randn(B * S, 3 * H, generator=g)
    qkv[:, 2 * H:] *= v_scale
    qkv = h(qkv).to(DEV)
    mask = None
    if masked:
        mask = torch.ones(B, S, dtype=torch.uint8)
        for b in range(B):
            mask[b, 20 + 3 * b: 20 + 3 * b + 7] = 0
        mask = mask.to(DEV)
    dctx = h(torch.randn(B * S, H, generator=g)).to(DEV)
    return qkv, mask, dctx


def _attn_ref64(qkv, mask, dctx, B, S, heads):
    H = heads * 64
    qr = qkv.double().requires_grad_(True)
    q, k, v = (qr[:, i * H:(i + 1) * H].reshape(B, S, heads, 64).transpose(1, 2) for i in range(3))
    sc = q @ k.transpose(-1, -2) / 8.0
    if mask is not None:
        sc = sc.masked_fill(~mask[:, None, None, :].bool(), float("-inf"))
    ctx = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B * S, H)
    ctx.backward(dctx.double())
    return [qr.grad[:, i * H:(i + 1) * H] for i in range(3)]


def _attn_bwd_run(L, qkv, mask, dctx, B, S, heads):
    H = heads * 64
    ctx = torch.empty(B * S, H, dtype=torch.float16, device=DEV)
    lse = torch.empty(B, heads, S, device=DEV)
    dqkv = torch.full((B * S, 3 * H), float("nan"), dtype=torch.float16, device=DEV)
    with L.operands("f16"):
        L.attn_fwd(qkv, ctx, lse, B, S, heads, key_mask=mask)
        L.attn_bwd(qkv, ctx, lse, dctx, dqkv, B, S, heads, key_mask=mask)
    torch.cuda.synchronize()
    return [dqkv[:, i * H:(i + 1) * H] for i in range(3)]


@pytest.mark.parametrize("B,S,heads,masked", ATTN_SHAPES)
def test_attn_bwd_loss_scaled_range(L, B, S, heads, masked):
    """B (headroom) for the ViLT attention backward at test_ops_gpu's shapes: tolerance 6e-3 (test_f16_gpu's fp16 bound for the
    same kernel, 1/5 of the bf16 build's 3e-2)."""
    qkv, mask, dctx = _attn_data(B, S, heads, masked)
    ref = _attn_ref64(qkv, mask, dctx, B, S, heads)
    s = _headroom_scale(max(float(r.abs().max()) for r in ref), dctx)
    got = _attn_bwd_run(L, qkv, mask, _scaled(dctx, s), B, S, heads)
    _headroom_check(L, got, ref, s, 6e-3, f"attn_bwd {(B, S, heads, masked)}")


@pytest.mark.parametrize("B,S,heads,masked", [(2, 185, 12, False), (3, 90, 12, True)])
def test_attn_bwd_overflow_is_not_hidden(L, B, S, heads, masked):
    """B (overflow) for the ViLT attention backward (V x 32, as for attn2)."""
    qkv, mask, dctx = _attn_data(B, S, heads, masked, v_scale=32.0)
    ref = _attn_ref64(qkv, mask, dctx, B, S, heads)
    s = _pow2_for(max(float(r.abs().max()) for r in ref), 17)
    got = _attn_bwd_run(L, qkv, mask, _scaled(dctx, s), B, S, heads)
    _check_overflowed(L, got, [r * s for r in ref], f"attn_bwd {(B, S, heads, masked)}")


@pytest.mark.parametrize("B,S,heads,masked", ATTN_CLS_SHAPES)
def test_attn_cls_bwd_loss_scaled_range(L, B, S, heads, masked):
    """B for attn_cls_bwd (fp32 incoming gradient, 16-bit dqkv): headroom within 2.5e-3 of max (test_attn_cls_fwd_bwd_fp16's
    bound), and overflow."""
    qkv, km, d0 = _cls_data(B, S, heads, masked)
    ctx, _, _, _ = _cls_run(L, qkv, km, d0, B, S, heads)
    _, _, ref = _cls_ref64(qkv, km, ctx.view(B, S, heads, 64)[:, 0], d0, B, S, heads)
    m = max(float(r.abs().max()) for r in ref)
    s = _pow2_for(m, 12)
    _, _, got, _ = _cls_run(L, qkv, km, d0 * s, B, S, heads)
    _headroom_check(L, got, ref, s, 2.5e-3, f"attn_cls_bwd {(B, S, heads, masked)}")
    s = _pow2_for(m, 17)
    _, _, got, _ = _cls_run(L, qkv, km, d0 * s, B, S, heads)
    _check_overflowed(L, [t.contiguous() for t in got], [r * s for r in ref], f"attn_cls_bwd {(B, S, heads, masked)}")


@pytest.mark.parametrize("rows,H", LAYERNORM_SHAPES)
def test_layernorm_bwd_dx_loss_scaled_range(L, rows, H):
    """B for layernorm_bwd_dx's 16-bit output: headroom with fp32 and 16-bit dy (tolerance 2.5e-3, as in A), overflow with
    fp32 dy."""
    g = torch.Generator().manual_seed(rows + 1)
    x = (torch.randn(rows, H, generator=g) * 2 + 0.3).to(DEV)
    gamma = (1 + 0.1 * torch.randn(H, generator=g)).to(DEV)
    eps = 1e-12 if H == 768 else 1e-5
    dy16 = h(torch.randn(rows, H, generator=g)).to(DEV)
    xr = x.double().requires_grad_(True)
    F.layer_norm(xr, (H,), gamma.double(), None, eps).backward(dy16.double())
    ref = xr.grad
    stats = torch.empty(rows, 2, device=DEV)
    o16 = torch.empty(rows, H, dtype=torch.float16, device=DEV)
    s12, s17 = _headroom_scale(float(ref.abs().max()), dy16), _pow2_for(float(ref.abs().max()), 17)
    with L.operands("f16"):
        L.layernorm_fwd(x, gamma, torch.zeros_like(gamma), eps, rows, H, y_f32=torch.empty(rows, H, device=DEV), stats=stats)
        L.layernorm_bwd_dx(x, stats, gamma, rows, H, dy_bf16=_scaled(dy16, s12), out_bf16=o16)
        torch.cuda.synchronize()
        _headroom_check(L, [o16.clone()], [ref], s12, 2.5e-3, f"layernorm_bwd_dx dy16 {(rows, H)}")
        L.layernorm_bwd_dx(x, stats, gamma, rows, H, dy_f32=dy16.float() * s12, out_bf16=o16)
        torch.cuda.synchronize()
        _headroom_check(L, [o16.clone()], [ref], s12, 2.5e-3, f"layernorm_bwd_dx dy32 {(rows, H)}")
        L.layernorm_bwd_dx(x, stats, gamma, rows, H, dy_f32=dy16.float() * s17, out_bf16=o16)
        torch.cuda.synchronize()
    _check_overflowed(L, [o16], [ref * s17], f"layernorm_bwd_dx {(rows, H)}")


def test_adapter_bwd_dx16_loss_scaled_range(L):
    """B for adapter_bwd's 16-bit dx copy (fp32 dy): headroom -- dx16 / s against the fp32 dx of the unscaled call within 1.5e-3
    of max (test_f16_gpu's bound for dx16 vs dx) -- and overflow against s x that fp32 dx."""
    par = _adapter_params(L, "f16", 31)
    T = 1007
    gen = torch.Generator().manual_seed(32)
    x = torch.randn(T, 768, generator=gen).to(DEV)
    dy = torch.randn(T, 768, generator=gen).to(DEV)
    segs = _adapter_segs(L, par, T)
    dx = torch.zeros(T, 768, device=DEV)
    dx16 = torch.zeros(T, 768, dtype=torch.float16, device=DEV)
    with L.operands("f16"):
        L.adapter_bwd(x, dy, dx, segs, T, dx_bf16=dx16)
        torch.cuda.synchronize()
        ref = dx.double().clone()
        s = _pow2_for(float(ref.abs().max()), 12)
        L.adapter_bwd(x, dy * s, dx, segs, T, dx_bf16=dx16)
        torch.cuda.synchronize()
        _headroom_check(L, [dx16.clone()], [ref], s, 1.5e-3, "adapter_bwd dx16")
        s = _pow2_for(float(ref.abs().max()), 17)
        L.adapter_bwd(x, dy * s, dx, segs, T, dx_bf16=dx16)
        torch.cuda.synchronize()
    _check_overflowed(L, [dx16], [ref * s], "adapter_bwd dx16")


def test_gelu_bwd_loss_scaled_range(L):
    """gelu_bwd is fp32 in and out in both builds: a power-of-two scale of dy leaves BIT-EXACTLY at 2^12 and at 2^17 (no 16-bit
    stage anywhere that could clamp or overflow)."""
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(4096, generator=g) * 2).to(DEV)
    dy = torch.randn(4096, generator=g).to(DEV)
    d1, d2 = torch.empty_like(x), torch.empty_like(x)
    with L.operands("f16"):
        L.gelu_bwd(x, dy, d1)
        for e in (12, 17):
            s = _pow2_for(float(d1.abs().max()), e)
            L.gelu_bwd(x, dy * s, d2)
            torch.cuda.synchronize()
            assert torch.equal(d2, d1 * s), e


def test_gemm_mul_g8_loss_scaled_range(L):
    """B for EPI_MUL_G8 (the FFN backward's gelu'-code product, 16-bit output) at (5920, 3072, 768): headroom with the gradient
    operand A scaled (out / s within 5e-5 + 2^-10 |exact| per element, as in A), overflow with A and B scaled (each stays below
    65504)."""
    M, N, K = 5920, 3072, 768
    g = torch.Generator().manual_seed(9)
    A_ = h(torch.randn(M, K, generator=g)).to(DEV)
    Bh = h(torch.randn(N, K, generator=g) * (1.5 / K ** 0.5)).to(DEV)
    code = torch.randint(0, 256, (M, N), generator=g, dtype=torch.uint8).to(DEV)
    w = (A_.double() @ Bh.double().t()) * (L.G8_LO + L.G8_STEP * code.double())
    o16 = torch.empty(M, N, dtype=torch.float16, device=DEV)
    s = _pow2_for(float(w.abs().max()), 12)
    with L.operands("f16"):
        L.gemm_bf16_nt(_scaled(A_, s), Bh, L.EPI_MUL_G8, aux=code, out_bf16=o16)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o16.float()).all())
        got = o16.double() / s
        excess = float(((got - w).abs() - 2.0 ** -10 * w.abs()).max())
        print(f"headroom EPI_MUL_G8: s = 2^{int(math.log2(s))}, max |exact| {float(w.abs().max()) * s:.0f}, "
              f"excess of out / s over 2^-10|exact| {excess:.2e}")
        assert bool(((got - w).abs() <= 5e-5 + 2.0 ** -10 * w.abs()).all())
        sa = 2.0 ** (14 - math.floor(math.log2(float(A_.abs().max()))))
        sb = _pow2_for(float(w.abs().max()) * sa, 17)
        L.gemm_bf16_nt(_scaled(A_, sa), _scaled(Bh, sb), L.EPI_MUL_G8, aux=code, out_bf16=o16)
        torch.cuda.synchronize()
    _check_overflowed(L, [o16], [w * (sa * sb)], "EPI_MUL_G8")


# ====================================================================================== C. entry points without a direct test
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("E", [1, 7, 185, 281])
def test_layernorm_bwd_dx_sparse_is_the_dense_kernel_on_zero_expanded_dres(L, fmt, E):
    """feddat_layernorm_bwd_dx_sparse (the top ViLT layer's LayerNorm backward) = feddat_layernorm_bwd_dx given the zero-expanded
    dense dres, bit for bit: both dy forms, both outputs, strides > H on every operand, B = 1, 3, 32 samples of E rows.  Output
    padding columns (fp32 output; the 16-bit output has ld = H) stay untouched.  The C ABI refuses dres_every <= 0 and a NULL
    dres; the Python wrapper sends dres_every = 0 to the dense kernel."""
    H = 768
    dt = L.OPERAND_DTYPE[fmt]
    for B in (1, 3, 32):
        rows = B * E
        g = torch.Generator().manual_seed(E * 100 + B)
        xs, dys, drs, os_ = H + 64, 2 * H, H + 4, H + 32
        x = (torch.randn(rows, xs, generator=g) * 2 + 0.3).to(DEV)
        gamma = (1 + 0.1 * torch.randn(H, generator=g)).to(DEV)
        stats = torch.empty(rows, 2, device=DEV)
        dy32 = torch.randn(rows, dys, generator=g).to(DEV)
        dy16 = dy32.to(dt)
        dres_c = torch.randn(B, drs, generator=g).to(DEV)
        dres_d = torch.zeros(rows, drs, device=DEV)
        dres_d[::E] = dres_c
        with L.operands(fmt):
            L.layernorm_fwd(x, gamma, torch.zeros_like(gamma), 1e-12, rows, H, x_stride=xs, y_f32=torch.empty(rows, H, device=DEV),
                            stats=stats)
            for dyk in ("f32", "16"):
                kw = dict(dy_f32=dy32) if dyk == "f32" else dict(dy_bf16=dy16)
                outs = []
                for every, dres in ((0, dres_d), (E, dres_c)):
                    o32 = torch.full((rows, os_), -7.0, device=DEV)
                    o16 = torch.full((rows * H + 64,), -7.0, dtype=dt, device=DEV)
                    L.layernorm_bwd_dx(x, stats, gamma, rows, H, dy_stride=dys, x_stride=xs, dres=dres, dres_stride=drs,
                                       out_f32=o32, out_stride=os_, out_bf16=o16, dres_every=every, **kw)
                    outs.append((o32, o16))
                torch.cuda.synchronize()
                (a32, a16), (b32, b16) = outs
                assert torch.equal(a32, b32) and torch.equal(a16, b16), (B, dyk)
                assert bool((b32[:, H:] == -7.0).all()) and bool((b16[rows * H:] == -7.0).all())
                assert torch.equal(b16[:rows * H].view(rows, H), b32[:, :H].to(dt))
            lib = L.load()
            for every, dres in ((-1, dres_c), (0, dres_c), (E, None)):
                rc = lib.feddat_layernorm_bwd_dx_sparse(None, C.c_void_p(dy32.data_ptr()), dys, C.c_void_p(x.data_ptr()), xs,
                                                        C.c_void_p(stats.data_ptr()), C.c_void_p(gamma.data_ptr()),
                                                        None if dres is None else C.c_void_p(dres.data_ptr()), drs, every,
                                                        rows, H, C.c_void_p(o32.data_ptr()), os_, None,
                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
                assert rc == 1, (every, dres is None, rc)          # FEDDAT_EINVAL


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("n", [1, 3])
def test_adapter_pack_strided_is_adapter_pack_per_module(L, fmt, n):
    """feddat_adapter_pack_strided (all modules of one adapter after an optimizer step, both engines) = feddat_adapter_pack per
    module, bit for bit, with strides that leave gaps between the modules' fp32 masters and between their 16-bit copies; the
    sentinel in the gaps stays untouched."""
    r, H = 48, 768
    rH = r * H
    dt = L.OPERAND_DTYPE[fmt]
    g = torch.Generator().manual_seed(40 + n)
    off_u, stride32 = rH + 48, 2 * rH + 1024
    stride16 = 4 * rH + 256
    flat32 = (torch.randn(n * stride32, generator=g) * 0.05).to(DEV)
    buf = torch.full((n * stride16,), -7.0, dtype=dt, device=DEV)
    with L.operands(fmt):
        L.adapter_pack_strided(flat32, flat32[off_u:], stride32, buf, buf[rH:], buf[2 * rH:], buf[3 * rH:], stride16, n)
        for l in range(n):
            wd = flat32[l * stride32: l * stride32 + rH].view(r, H)
            wu = flat32[l * stride32 + off_u: l * stride32 + off_u + rH].view(H, r)
            w = [torch.empty(rH, dtype=dt, device=DEV) for _ in range(4)]
            L.adapter_pack(wd, wu, *w)
            torch.cuda.synchronize()
            for c in range(4):
                assert torch.equal(buf[l * stride16 + c * rH: l * stride16 + (c + 1) * rH], w[c]), (l, c)
            assert bool((buf[l * stride16 + 4 * rH: (l + 1) * stride16] == -7.0).all()), l


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("nrep", [1, 2])
@pytest.mark.parametrize("with_attention_mask", [False, True])
def test_image_embed_assemble_masked_is_the_three_launches(L, fmt, nrep, with_attention_mask):
    """feddat_image_embed_assemble_masked (the ViLT engine's image embedding tail) = vilt_key_mask + pos_embed_resize_masked +
    image_embed_assemble, bit for bit, for padded images of a different valid patch rectangle per sample."""
    B, Lt, gh, gw, g0, H = 4, 40, 12, 12, 12, 768
    np_ = gh * gw
    S = Lt + 1 + np_
    gen = torch.Generator().manual_seed(50 + nrep)
    proj = torch.randn(B * np_, H, generator=gen).to(DEV)
    cls, pos0, mod1 = (torch.randn(H, generator=gen).to(DEV) for _ in range(3))
    pos_grid = torch.randn(g0, g0, H, generator=gen).to(DEV)
    pm = torch.zeros(B, gh, gw, dtype=torch.int64)
    for b, (vh, vw) in enumerate([(12, 12), (8, 12), (12, 7), (1, 2)]):
        pm[b, :vh, :vw] = 1
    pm = pm.to(DEV)
    am = None
    if with_attention_mask:
        am = torch.ones(B, Lt, dtype=torch.int64)
        for b, n in enumerate([40, 31, 12, 1]):
            am[b, n:] = 0
        am = am.to(DEV)
    h0 = torch.randn(B, S, H, generator=gen).to(DEV)
    h_a, h_b = h0.clone(), h0.clone()
    km_a = torch.full((nrep * B, S), 7, dtype=torch.uint8, device=DEV)
    km_b = km_a.clone()
    pos_img = torch.empty(B, np_, H, device=DEV)
    with L.operands(fmt):
        L.vilt_key_mask(am, pm, km_a, B, Lt, gh, gw, 1, nrep=nrep)
        L.pos_embed_resize_masked(pos_grid, pm, pos_img, g0, B, gh, gw, 1, H)
        L.image_embed_assemble(proj, cls, pos0, pos_img, mod1, h_a, B, Lt, np_, S, H, pos_batch_stride=np_ * H)
        L.image_embed_assemble_masked(proj, cls, pos0, pos_grid, pm, am, mod1, h_b, km_b, B, Lt, gh, gw, g0, H, nrep=nrep)
    torch.cuda.synchronize()
    assert torch.equal(h_a, h_b)
    assert torch.equal(km_a, km_b)
    assert torch.equal(h_b[:, :Lt], h0[:, :Lt])                    # the text rows are not the image tail's
    assert bool((km_b[:, Lt + 1:].reshape(nrep, B, np_).float().sum(-1)[0].cpu() == torch.tensor([144., 96., 84., 2.])).all())


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("Lq", [1, 25])
def test_gather_rows(L, fmt, Lq):
    """feddat_gather_rows (one question's states per answer, ALBEF): dst[r] = src[idx[r]], a zero row for idx < 0, duplicates
    allowed, width = Lq x 768; the fp32 output exact and the 16-bit one bit-equal to its RNE conversion."""
    dt = L.OPERAND_DTYPE[fmt]
    width = Lq * 768
    gen = torch.Generator().manual_seed(60 + Lq)
    src = (torch.randn(5, width, generator=gen) * 1e3).to(DEV)
    idx = torch.tensor([3, 3, -1, 0, 4, 4, 4, -1, 1], dtype=torch.int32, device=DEV)
    want = torch.where((idx >= 0)[:, None], src[idx.clamp(min=0).long()], torch.zeros((), device=DEV))
    d32 = torch.full((9, width), float("nan"), device=DEV)
    d16 = torch.full((9, width), float("nan"), dtype=dt, device=DEV)
    d16b = torch.full((9, width), float("nan"), dtype=dt, device=DEV)
    with L.operands(fmt):
        L.gather_rows(src, idx, dst_f32=d32, dst_bf16=d16)
        L.gather_rows(src, idx, dst_bf16=d16b)
    torch.cuda.synchronize()
    assert torch.equal(d32, want)
    assert torch.equal(d16, want.to(dt)) and torch.equal(d16b, d16)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("accumulate", [False, True])
def test_segment_sum_rows_is_the_sequential_fp32_sum(L, fmt, accumulate):
    """feddat_segment_sum_rows (gather_rows' adjoint): bit-equal to a sequential fp32 sum in index order (the order the kernel
    documents), empty and one-row segments, accumulate 0 / 1, width not a multiple of 1024."""
    width = 772
    offs = [0, 0, 1, 4, 4, 9, 10]                # segments of 0, 1, 3, 0, 5, 1 rows
    gen = torch.Generator().manual_seed(70)
    src = (torch.randn(10, width, generator=gen) * torch.exp2(torch.randint(-8, 8, (10, 1), generator=gen).float())).to(DEV)
    dst0 = torch.randn(len(offs) - 1, width, generator=gen).to(DEV)
    dst = dst0.clone()
    with L.operands(fmt):
        L.segment_sum_rows(src, torch.tensor(offs, dtype=torch.int32, device=DEV), dst, accumulate=accumulate)
    torch.cuda.synchronize()
    for s in range(len(offs) - 1):
        acc = dst0[s].clone() if accumulate else torch.zeros(width, device=DEV)
        for j in range(offs[s], offs[s + 1]):
            acc = acc + src[j]
        assert torch.equal(dst[s], acc), s


@pytest.mark.parametrize("fmt", FMTS)
def test_axpby3_every_operand_combination(L, fmt):
    """feddat_axpby3: out = alpha a + beta b + gamma c for every NULL combination of b / c, negative coefficients, n = 4004 (not a
    multiple of 1024).  fp32 output within 2 ulp of the float64 sum's terms (the compiler may contract into FMAs; a alone is the
    exact fp32 product); 16-bit output bit-equal to the fp32 output's RNE conversion."""
    dt = L.OPERAND_DTYPE[fmt]
    n = 4004
    gen = torch.Generator().manual_seed(80)
    a, b, c = ((torch.randn(n, generator=gen) * 300).to(DEV) for _ in range(3))
    alpha, beta, gamma = -0.75, 1.25, -3.0
    for bb, cc in ((None, None), (b, None), (None, c), (b, c)):
        o32 = torch.full((n + 4,), float("nan"), device=DEV)
        o16 = torch.full((n + 4,), float("nan"), dtype=dt, device=DEV)
        with L.operands(fmt):
            L.axpby3(a, alpha, bb, beta, cc, gamma, out_f32=o32[:n], out_bf16=o16[:n])
        torch.cuda.synchronize()
        ref = a.double() * alpha
        mag = ref.abs()
        if bb is not None:
            ref, mag = ref + bb.double() * beta, mag + (bb.double() * beta).abs()
        if cc is not None:
            ref, mag = ref + cc.double() * gamma, mag + (cc.double() * gamma).abs()
        if bb is None and cc is None:
            assert torch.equal(o32[:n], a * alpha)
        assert bool(((o32[:n].double() - ref).abs() <= 2.0 ** -22 * mag).all()), (bb is None, cc is None)
        assert torch.equal(o16[:n], o32[:n].to(dt))
        assert bool(torch.isnan(o32[n:]).all()) and bool(torch.isnan(o16[n:].float()).all())


@pytest.mark.parametrize("fmt", FMTS)
def test_elementwise_refusals(L, fmt):
    """n % 4 != 0 (axpby3, dropout) and width % 4 != 0 (gather_rows, segment_sum_rows) are refused with FeddatHipError."""
    x = torch.zeros(4 * 30, device=DEV)
    with L.operands(fmt):
        with pytest.raises(L.FeddatHipError):
            L.axpby3(x[:118], 1.0, out_f32=torch.empty(118, device=DEV))
        with pytest.raises(L.FeddatHipError):
            L.dropout(x[:118], (0.1, 1, 2, None), out_f32=torch.empty(118, device=DEV))
        src = torch.zeros(4, 30, device=DEV)
        with pytest.raises(L.FeddatHipError):
            L.gather_rows(src, torch.zeros(2, dtype=torch.int32, device=DEV), dst_f32=torch.empty(2, 30, device=DEV))
        with pytest.raises(L.FeddatHipError):
            L.segment_sum_rows(src, torch.tensor([0, 4], dtype=torch.int32, device=DEV), torch.empty(1, 30, device=DEV))
