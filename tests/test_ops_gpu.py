"""Op-level parity of the HIP kernels (through the C ABI / ctypes) against the CPU oracle, the golden
fixtures captured from the reference, and plain fp32 PyTorch restatements of the same op.

Tolerances: the kernels compute in bf16 with fp32 accumulation (north_star: bf16 MFMA); references are fp32 on
bf16-rounded inputs where the kernel rounds its inputs, so the stated tolerances cover output rounding
(bf16 eps = 2^-8 relative) and accumulation-order differences only."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import feddat_oracle as O
from tests.golden_util import load

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import lib
    lib.load()
    return lib


def bf(x):
    return x.to(torch.bfloat16)


def rel_err(a, b):
    return float((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-12))


# ------------------------------------------------------------------ hardware semantics
def test_probe_tr16_layout(L):
    x = torch.arange(64 * 64, dtype=torch.float32, device=DEV).reshape(64, 64)
    x = bf(x % 251 + (x // 64) * 0.0)  # small exact integers
    x = bf(torch.arange(64 * 64, device=DEV).reshape(64, 64).float() % 509)
    out = torch.zeros(64, 8, dtype=torch.bfloat16, device=DEV)
    L.probe_tr16(x, out)
    torch.cuda.synchronize()
    exp = torch.zeros(64, 8, dtype=torch.bfloat16, device=DEV)
    for lane in range(64):
        g, i = lane >> 4, lane & 15
        for j in range(4):
            exp[lane, j] = x[4 * g + j, 16 + i]
            exp[lane, 4 + j] = x[16 + 4 * g + j, 16 + i]
    assert torch.equal(out, exp), (out[:20], exp[:20])


# ------------------------------------------------------------------ K1 GEMM
@pytest.mark.parametrize("M,N,K", [(300, 256, 192), (128, 128, 64),       # M < 1024: the small-tile ring kernel (64 x 64 tiles)
                                   (800, 768, 3072), (800, 3072, 768),    # ... ALBEF text-stream shapes; the second on 64 x 128 tiles
                                   (100, 192, 128), (96, 30592, 768),     # ... N % 128 != 0; the LM-head product
                                   (1200, 256, 192), (1030, 640, 64),     # M >= 1024, N % 192 != 0: the 128 x 128 kernel
                                   (5920, 768, 3072), (11840, 2304, 768),
                                   (11840, 3072, 768),    # ViLT's only production shape on the 256 x 192 (WM = 4) tiles (test_gemm_route_cpu.py)
                                   (11849, 3072, 768)])   # the same plan with a ragged last M tile
def test_gemm_epilogues(L, M, N, K):
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A = bf(torch.randn(M, K, generator=g)).to(DEV)
    B = bf(torch.randn(N, K, generator=g) * 0.05).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    resid = torch.randn(M, N, generator=g).to(DEV)
    aux = bf(torch.randn(M, N, generator=g)).to(DEV)
    ref = A.float() @ B.float().t()
    tol = 1.5e-2

    o16 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    L.gemm_bf16_nt(A, B, L.EPI_BF16, bias=bias, out_bf16=o16)
    assert rel_err(o16, ref + bias) < tol

    o32 = torch.empty(M, N, device=DEV)
    L.gemm_bf16_nt(A, B, L.EPI_RESID_F32, bias=bias, resid=resid, out_f32=o32)
    assert rel_err(o32, ref + bias + resid) < 2e-3

    u16 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    L.gemm_bf16_nt(A, B, L.EPI_GELU, bias=bias, out_bf16=o16, out2_bf16=u16)
    assert rel_err(u16, ref + bias) < tol
    assert rel_err(o16, F.gelu(ref + bias)) < tol

    L.gemm_bf16_nt(A, B, L.EPI_MUL_DGELU, aux=aux, out_bf16=o16)
    a32 = aux.float().requires_grad_(True)
    F.gelu(a32).sum().backward()
    assert rel_err(o16, ref * a32.grad) < tol

    L.gemm_bf16_nt(A, B, L.EPI_F32, bias=bias, out_f32=o32)
    assert rel_err(o32, ref + bias) < 2e-3
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,N,K", [(11849, 3072, 768), (5920, 2304, 768), (11840, 768, 3072), (1030, 192, 64), (18464, 768, 768), (18464, 2304, 768),
                                   (5920, 768, 3072), (4608, 768, 3072), (5920, 768, 768)])      # the last three: one partial round of tiles (160-row plan)
def test_gemm_kernel_variants_bit_identical(L, M, N, K):
    """The two persistent kernels (v2: two wave groups per SIMD; v3: one wave per SIMD, inline-asm MFMAs with AGPR
    accumulators) and the tile heights of each (192 / 256 rows; v3 also 160 rows where they fill the rounds of the 256 CUs
    better -- 5920 x 2304 and ALBEF's 18464 x 768 here; flag 1 << 27 switches them off) accumulate in the same order and
    share the epilogues: every epilogue's output must be bit-identical across them (the production dispatch mixes them per
    launch)."""
    g = torch.Generator(device="cpu").manual_seed(M + N)
    A = bf(torch.randn(M, K, generator=g)).to(DEV)
    B = bf(torch.randn(N, K, generator=g) * 0.05).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    resid = torch.randn(M, N, generator=g).to(DEV)
    aux = bf(torch.randn(M, N, generator=g)).to(DEV)

    def run(flags):
        L.set_debug_flags(flags)
        try:
            o0 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            o2, u2, o3 = torch.zeros_like(o0), torch.zeros_like(o0), torch.zeros_like(o0)
            o1, o4 = torch.zeros(M, N, device=DEV), torch.zeros(M, N, device=DEV)
            L.gemm_bf16_nt(A, B, L.EPI_BF16, bias=bias, out_bf16=o0)
            L.gemm_bf16_nt(A, B, L.EPI_RESID_F32, bias=bias, resid=resid, out_f32=o1)
            L.gemm_bf16_nt(A, B, L.EPI_GELU, bias=bias, out_bf16=o2, out2_bf16=u2)
            L.gemm_bf16_nt(A, B, L.EPI_MUL_DGELU, aux=aux, out_bf16=o3)
            L.gemm_bf16_nt(A, B, L.EPI_F32, bias=bias, out_f32=o4)
            torch.cuda.synchronize()
        finally:
            L.set_debug_flags(0)
        return [o0, o1, o2, u2, o3, o4]
    ref = run(1 | 32)                      # v2, 192-row tiles
    assert rel_err(ref[0], A.float() @ B.float().t() + bias) < 1.5e-2
    # v2 256-row, v3 192 / 256 / best-fit rows, no 160-row tiles, production, and (round 6) the DUAL form: two independent
    # 128 x 192 workgroups per CU (3 = flags 1 | 2 together: every persistent launch; 3 | 64: those with >= 2 rounds of the doubled grid)
    for flags in (1 | 64, 2 | 32, 2 | 64, 2, 1 << 27, 0, 3, 3 | 64):
        for a_, b_ in zip(ref, run(flags)):
            assert torch.equal(a_, b_), flags


@pytest.mark.parametrize("M,N,K", [(11840, 3072, 768), (2051, 384, 192)])
def test_gemm_dual_form_code_epilogues_bit_identical(L, M, N, K):
    """The 8-bit gelu' code epilogues (FFN1: GELU + codes; FFN2^T: . code) on the DUAL form of the persistent kernel against the
    two-group kernel they run on in production; the runtime must grant the design's two workgroups per CU."""
    assert L.gemm_dual_blocks_per_cu() == 2
    g = torch.Generator(device="cpu").manual_seed(M + N + 1)
    A = bf(torch.randn(M, K, generator=g)).to(DEV)
    B = bf(torch.randn(N, K, generator=g) * 0.05).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    codes = torch.randint(0, 256, (M, N), generator=g, dtype=torch.uint8).to(DEV)

    def run(flags):
        L.set_debug_flags(flags)
        try:
            o, c, o2 = (torch.zeros(M, N, dtype=torch.bfloat16, device=DEV), torch.zeros(M, N, dtype=torch.uint8, device=DEV),
                        torch.zeros(M, N, dtype=torch.bfloat16, device=DEV))
            L.gemm_bf16_nt(A, B, L.EPI_GELU_G8, bias=bias, out_bf16=o, out2_bf16=c)
            L.gemm_bf16_nt(A, B, L.EPI_MUL_G8, aux=codes, out_bf16=o2)
            torch.cuda.synchronize()
        finally:
            L.set_debug_flags(0)
        return o, c, o2
    for a_, b_ in zip(run(0), run(3)):
        assert torch.equal(a_, b_)


def test_gemm_rejects_bad_shapes(L):
    A = torch.zeros(8, 60, dtype=torch.bfloat16, device=DEV)
    B = torch.zeros(100, 60, dtype=torch.bfloat16, device=DEV)
    o = torch.zeros(8, 100, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(L.FeddatHipError):
        L.gemm_bf16_nt(A, B, L.EPI_BF16, out_bf16=o)


# ------------------------------------------------------------------ K3 LayerNorm
LAYERNORM_SHAPES = [(37, 768), (5920, 768), (64, 1536)]


@pytest.mark.parametrize("rows,H", LAYERNORM_SHAPES)
def test_layernorm_fwd_bwd(L, rows, H):
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, H, generator=g) * 2 + 0.3).to(DEV)
    gamma = (1 + 0.1 * torch.randn(H, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(H, generator=g)).to(DEV)
    y32 = torch.empty(rows, H, device=DEV)
    y16 = torch.empty(rows, H, dtype=torch.bfloat16, device=DEV)
    stats = torch.empty(rows, 2, device=DEV)
    eps = 1e-12 if H == 768 else 1e-5
    L.layernorm_fwd(x, gamma, beta, eps, rows, H, y_bf16=y16, y_f32=y32, stats=stats)
    ref = F.layer_norm(x, (H,), gamma, beta, eps)
    assert (y32 - ref).abs().max() < 2e-5
    assert rel_err(y16, ref) < 1e-2
    # dX-only backward with residual add
    dy = torch.randn(rows, H, generator=g).to(DEV)
    dres = torch.randn(rows, H, generator=g).to(DEV)
    xr = x.clone().requires_grad_(True)
    F.layer_norm(xr, (H,), gamma, beta, eps).backward(dy)
    out = torch.empty(rows, H, device=DEV)
    L.layernorm_bwd_dx(x, stats, gamma, rows, H, dy_f32=dy, dres=dres, out_f32=out)
    assert (out - (xr.grad + dres)).abs().max() < 5e-5
    dy16 = bf(dy)
    o16 = torch.empty(rows, H, dtype=torch.bfloat16, device=DEV)
    L.layernorm_bwd_dx(x, stats, gamma, rows, H, dy_bf16=dy16, out_f32=out, out_bf16=o16)
    xr.grad = None
    F.layer_norm(xr, (H,), gamma, beta, eps).backward(dy16.float())
    assert (out - xr.grad).abs().max() < 5e-5
    assert rel_err(o16, xr.grad) < 1e-2
    if rows <= 1024:
        gr = gamma.clone().requires_grad_(True)
        br = beta.clone().requires_grad_(True)
        xr.grad = None
        F.layer_norm(xr, (H,), gr, br, eps).backward(dy)
        dx = torch.empty(rows, H, device=DEV)
        dg = torch.empty(H, device=DEV)
        db = torch.empty(H, device=DEV)
        L.layernorm_bwd_full(dy, x, stats, gamma, rows, H, dx, dg, db)
        assert (dx - xr.grad).abs().max() < 5e-5
        assert (dg - gr.grad).abs().max() < 1e-4 * max(1.0, float(gr.grad.abs().max()))
        assert (db - br.grad).abs().max() < 1e-4 * max(1.0, float(br.grad.abs().max()))


# ------------------------------------------------------------------ K4 adapter
def _pack(L, wd, wu):
    r, H = wd.shape
    w = [torch.empty(r, H, dtype=torch.bfloat16, device=DEV), torch.empty(H, r, dtype=torch.bfloat16, device=DEV),
         torch.empty(H, r, dtype=torch.bfloat16, device=DEV), torch.empty(r, H, dtype=torch.bfloat16, device=DEV)]
    L.adapter_pack(wd, wu, *w)
    return w


def _golden_adapter(L, golden_dir):
    g = load(golden_dir, "g1_adapter.npz")
    par = {}
    for a in range(3):
        wd = torch.from_numpy(g[f"p.adapter_{a}_down.weight"]).to(DEV)
        wu = torch.from_numpy(g[f"p.adapter_{a}_up.weight"]).to(DEV)
        wd16, wdT16, wu16, wuT16 = _pack(L, wd, wu)
        par[a] = dict(wd=wd16, wdT=wdT16, wu=wu16, wuT=wuT16, wd32=wd, wu32=wu,
                      bd=torch.from_numpy(g[f"p.adapter_{a}_down.bias"]).to(DEV),
                      bu=torch.from_numpy(g[f"p.adapter_{a}_up.bias"]).to(DEV))
    return g, par


def test_adapter_pack(L, golden_dir):
    """Fragment-major operand copies (documented in feddat_hip.h / adapter.hip): every wave load is one contiguous burst."""
    g, par = _golden_adapter(L, golden_dir)
    r, c = torch.meshgrid(torch.arange(48), torch.arange(768), indexing="ij")
    pc = (c // 32) * 32 + ((c % 16) // 4) * 8 + ((c % 32) // 16) * 4 + c % 4
    q, gg, j = pc // 32, (pc % 32) // 8, pc % 8
    down_idx = ((((r // 16) * 24 + q) * 64 + gg * 16 + r % 16) * 8 + j).reshape(-1).to(DEV)
    ct, i16, seg, g4, e = c // 16, c % 16, r // 16, (r % 16) // 4, r % 4
    lane = g4 * 16 + i16
    up_idx = torch.where(seg < 2, (ct * 64 + lane) * 8 + seg * 4 + e, 48 * 64 * 8 + (ct * 64 + lane) * 4 + e).reshape(-1).to(DEV)
    wd, wu = bf(par[0]["wd32"]), bf(par[0]["wu32"])          # [48,768], [768,48]
    assert torch.equal(par[0]["wd"].reshape(-1)[down_idx], wd.reshape(-1))
    assert torch.equal(par[0]["wdT"].reshape(-1)[up_idx], wd.reshape(-1))
    assert torch.equal(par[0]["wuT"].reshape(-1)[down_idx], wu.t().contiguous().reshape(-1))
    assert torch.equal(par[0]["wu"].reshape(-1)[up_idx], wu.t().contiguous().reshape(-1))


def test_adapter_fwd_bwd_vs_reference_golden(L, golden_dir):
    """G1: outputs and gradients of the reference's own Adapter module (adapter.py:124-163)."""
    g, par = _golden_adapter(L, golden_dir)
    x = torch.from_numpy(g["x"]).reshape(-1, 768).to(DEV)
    dy = torch.from_numpy(g["dy"]).reshape(-1, 768).to(DEV)
    T = x.shape[0]
    # one launch, two segments: rows [0,T/2) gated (adapter_0 + adapter_2), rows [T/2,T) single adapter_1
    h = T // 2
    segs = L.make_segs([
        dict(row_begin=0, row_end=h, train_slot=0,
             adapters=[dict(par[0], scale=0.5), dict(par[2], scale=0.5)]),
        dict(row_begin=h, row_end=T, train_slot=0, adapters=[dict(par[1], scale=1.0)]),
    ])
    out = torch.zeros_like(x)
    L.adapter_fwd(x, out, segs, T)
    yg = torch.from_numpy(g["gating.y"]).reshape(-1, 768).to(DEV)
    ys = torch.from_numpy(g["adapter_1.y"]).reshape(-1, 768).to(DEV)
    # the adapter delta here is O(1) (golden weights have std 0.05): bf16 operands (2^-8 relative) on a 768- and a
    # 48-term contraction -> abs error <~ 1e-2 on the delta; the fp32 residual path is exact
    assert (out[:h] - yg[:h]).abs().max() < 1.2e-2
    assert (out[h:] - ys[h:]).abs().max() < 1.2e-2

    dx = torch.zeros_like(x)
    dx16 = torch.zeros(T, 768, dtype=torch.bfloat16, device=DEV)
    z = torch.zeros(T, 48, device=DEV)
    dz = torch.zeros(T, 48, device=DEV)
    L.adapter_bwd(x, dy, dx, segs, T, dx_bf16=dx16, z_out=z, dz_out=dz)
    dxg = torch.from_numpy(g["gating.dx"]).reshape(-1, 768).to(DEV)
    dxs = torch.from_numpy(g["adapter_1.dx"]).reshape(-1, 768).to(DEV)
    # |dx - dy| ~ 1 with bf16 operands -> ~1e-3 typical error.  A bottleneck unit whose pre-activation lies within
    # bf16 noise of 0 may flip its ReLU mask relative to the fp32 reference; one flip moves that token's whole dx row
    # by up to |g| * |Wd| ~ 0.3.  Rows with such a fragile unit (|pre-activation| < 0.008 in fp32) are bounded
    # loosely, all other rows tightly.
    for a_, b_, rows_, ads_ in ((dx[:h], dxg[:h], x[:h], (0, 2)), (dx[h:], dxs[h:], x[h:], (1,))):
        pre = torch.cat([F.linear(rows_, par[a]["wd32"], par[a]["bd"]) for a in ads_], 1)
        fragile = pre.abs().min(1).values < 0.008
        d_ = (a_ - b_).abs().max(1).values
        assert int((~fragile).sum()) > len(d_) // 4
        assert float(d_[~fragile].max()) < 2e-2
        assert float(d_.max()) < 0.6
    assert rel_err(dx16, dx) < 1e-2
    # weight gradients from (z, dz) with the exact-fp32 MFMA GEMM; compare with an fp32 restatement on the SAME
    # rows (the golden weight grads cover all T rows, ours half of them per mode)
    for (lo, hi, a, sc, x_, dy_) in ((0, h, 0, 0.5, x[:h], dy[:h]), (h, T, 1, 1.0, x[h:], dy[h:])):
        wd32, wu32, bd, bu = par[a]["wd32"], par[a]["wu32"], par[a]["bd"], par[a]["bu"]
        zz = F.relu(F.linear(x_, wd32, bd))
        gg = (dy_ @ wu32) * sc
        dzz = gg * (zz > 0)
        n = hi - lo
        dWu = torch.empty(768, 48, device=DEV)
        dbu = torch.empty(768, device=DEV)
        L.sgemm_f32(dy[lo:], 1, 768, z[lo:], 48, 1, 768, 48, n, dWu, alpha=sc, colsum=dbu)
        dWd = torch.empty(48, 768, device=DEV)
        dbd = torch.empty(48, device=DEV)
        L.sgemm_f32(dz[lo:], 1, 48, x[lo:], 768, 1, 48, 768, n, dWd, colsum=dbd)
        # z / dz exported by the kernel: compared where the ReLU mask cannot flip under bf16 noise
        pre = F.linear(x_, wd32, bd)
        solid = pre.abs() > 0.008
        assert (z[lo:hi] - zz)[solid].abs().max() < 1e-2 * float(zz.abs().max())
        assert (dz[lo:hi] - dzz)[solid].abs().max() < 2e-2 * float(dzz.abs().max())
        assert float(solid.float().mean()) > 0.98
        # weight gradients: exact-fp32 products of the exported z / dz (so the reference uses the same z / dz)
        ref_dWu = dy_.t() @ (z[lo:hi] * sc)
        ref_dWd = dz[lo:hi].t() @ x_
        assert rel_err(dWu, ref_dWu) < 1e-5
        assert rel_err(dWd, ref_dWd) < 1e-5
        assert rel_err(dbu, dy_.sum(0) * sc) < 1e-5
        assert rel_err(dbd, dz[lo:hi].sum(0)) < 1e-5
        # (not compared with the all-fp32 gradients: with 64 tokens one flipped ReLU mask moves dW_down by ~20 %;
        #  end-to-end gradient quality is covered by tests/test_engine_gpu.py against the reference's weights)
        # the dedicated weight-gradient kernel (what the engine uses) must agree with the generic fp32 GEMM
        grad = torch.full((48 * 768 + 48 + 768 * 48 + 768,), float("nan"), device=DEV)
        part = torch.empty(L.adapter_wgrad_workspace_elems(1), device=DEV)
        L.adapter_wgrad(L.make_wgrad_segs([dict(x=x[lo:], dy=dy[lo:], z=z[lo:], dz=dz[lo:], grad=grad, rows=n,
                                                scale=sc)]), part)
        o = 48 * 768
        assert (grad[:o].view(48, 768) - dWd).abs().max() < 1e-4 * float(dWd.abs().max())
        assert (grad[o:o + 48] - dbd).abs().max() < 1e-4 * float(dbd.abs().max())
        assert (grad[o + 48:o + 48 + o].view(768, 48) - dWu).abs().max() < 1e-4 * float(dWu.abs().max())
        assert (grad[o + 48 + o:] - dbu).abs().max() < 1e-4 * float(dbu.abs().max())


def test_adapter_full_size_and_ragged_rows(L):
    """T = 5920 x 2 rows (configs[1]) and a segment length that is not a multiple of 16."""
    g = torch.Generator().manual_seed(3)
    T = 5920 * 2 + 7
    x = torch.randn(T, 768, generator=g).to(DEV)
    ads = []
    for a in range(3):
        wd = (torch.randn(48, 768, generator=g) * 0.03).to(DEV)
        wu = (torch.randn(768, 48, generator=g) * 0.03).to(DEV)
        wd16, wdT16, wu16, wuT16 = _pack(L, wd, wu)
        ads.append(dict(wd=wd16, wdT=wdT16, wu=wu16, wuT=wuT16, wd32=wd, wu32=wu,
                        bd=(torch.randn(48, generator=g) * 0.02).to(DEV),
                        bu=(torch.randn(768, generator=g) * 0.02).to(DEV)))
    h = 5920 + 7
    segs = L.make_segs([
        dict(row_begin=0, row_end=h, adapters=[dict(ads[0], scale=0.5), dict(ads[2], scale=0.5)]),
        dict(row_begin=h, row_end=T, adapters=[dict(ads[1], scale=1.0)]),
    ])
    out = torch.full_like(x, float("nan"))
    L.adapter_fwd(x, out, segs, T)

    def ref_ad(xx, a):
        wd, wu = bf(a["wd32"]).float(), bf(a["wu32"]).float()
        z = F.relu(bf(xx).float() @ wd.t() + a["bd"])
        return bf(z).float() @ wu.t() + a["bu"]
    ref0 = x[:h] + 0.5 * ref_ad(x[:h], ads[0]) + 0.5 * ref_ad(x[:h], ads[2])
    ref1 = x[h:] + ref_ad(x[h:], ads[1])
    assert (out[:h] - ref0).abs().max() < 2e-3
    assert (out[h:] - ref1).abs().max() < 2e-3
    # weight gradients at full size (T = 5920 + 7 and 5920 rows) against fp64
    dy = torch.randn(T, 768, generator=g).to(DEV)
    dx = torch.empty_like(x)
    z = torch.empty(T, 48, device=DEV)
    dz = torch.empty(T, 48, device=DEV)
    segs_b = L.make_segs([
        dict(row_begin=0, row_end=h, train_slot=0, adapters=[dict(ads[0], scale=0.5), dict(ads[2], scale=0.5)]),
        dict(row_begin=h, row_end=T, train_slot=0, adapters=[dict(ads[1], scale=1.0)]),
    ])
    L.adapter_bwd(x, dy, dx, segs_b, T, z_out=z, dz_out=dz)
    # the engine's path: the forward saves z = relu(Wd x + bd) of every slot, the backward takes it back and does not read
    # x -- same arithmetic in the same order, so every output is bit-identical with the recompute path
    zs = torch.full((T, 2, 48), float("nan"), device=DEV)
    out2 = torch.empty_like(x)
    L.adapter_fwd(x, out2, segs_b, T, z_save=zs)
    assert torch.equal(out2, out)
    dx2, z2, dz2 = torch.empty_like(x), torch.empty(T, 48, device=DEV), torch.empty(T, 48, device=DEV)
    dx16a = torch.empty(T, 768, dtype=torch.bfloat16, device=DEV)
    L.adapter_bwd(None, dy, dx2, segs_b, T, dx_bf16=dx16a, z_out=z2, dz_out=dz2, z_saved=zs)
    assert torch.equal(dx2, dx) and torch.equal(z2, z) and torch.equal(dz2, dz)
    assert torch.equal(zs[:h, 0], z[:h]) and torch.equal(zs[h:, 0], z[h:]) and not torch.isnan(zs[:h, 1]).any()
    assert torch.equal(dx16a, dx2.to(torch.bfloat16))
    # configs[4]: the same backward with dx also as e4m3 rows + per-row scale (quantised in the kernel): identical fp32
    # outputs, scale = row amax / 448, codes = round-to-nearest e4m3 of dx / scale (ragged tails included)
    dx3, z3, dz3 = torch.empty_like(x), torch.empty(T, 48, device=DEV), torch.empty(T, 48, device=DEV)
    d8 = torch.zeros(T, 768, dtype=torch.uint8, device=DEV)
    dsc = torch.zeros(T, device=DEV)
    L.adapter_bwd_fp8(dy, dx3, d8, dsc, segs_b, T, z_saved=zs, z_out=z3, dz_out=dz3)
    assert torch.equal(dx3, dx) and torch.equal(z3, z) and torch.equal(dz3, dz)
    amax = dx.abs().amax(1)
    assert torch.allclose(dsc, amax / 448.0, rtol=1e-6)
    deq = d8.view(torch.float8_e4m3fn).float() * dsc[:, None]
    assert bool(((deq - dx).abs() <= amax[:, None] * (2.0 ** -4) + 1e-12).all())
    assert float((d8.view(torch.float8_e4m3fn).float() == (dx / dsc[:, None]).to(torch.float8_e4m3fn).float()).float().mean()) > 0.99
    with pytest.raises(L.FeddatHipError):
        L.adapter_bwd(None, dy, dx2, segs_b, T)
    n = 48 * 768 + 48 + 768 * 48 + 768
    grads = torch.full((2, n), float("nan"), device=DEV)
    part = torch.empty(L.adapter_wgrad_workspace_elems(2), device=DEV)
    L.adapter_wgrad(L.make_wgrad_segs([
        dict(x=x, dy=dy, z=z, dz=dz, grad=grads[0], rows=h, scale=0.5),
        dict(x=x[h:], dy=dy[h:], z=z[h:], dz=dz[h:], grad=grads[1], rows=T - h, scale=1.0)]), part)
    o = 48 * 768
    for k, (lo, hi, sc) in enumerate(((0, h, 0.5), (h, T, 1.0))):
        xd, dyd, zd, dzd = (t[lo:hi].double() for t in (x, dy, z, dz))
        ref = torch.cat([(dzd.t() @ xd).flatten(), dzd.sum(0), (sc * dyd.t() @ zd).flatten(), sc * dyd.sum(0)])
        err = (grads[k].double() - ref).abs().max() / ref.abs().max()
        assert float(err) < 1e-5, (k, float(err))
    # the per-layer form: partial sums now, ONE batched reduction later (two "layers" = two launches): bit-identical
    ws = L.adapter_wgrad_workspace_elems(2)
    parts = torch.empty(2 * ws, device=DEV)
    g2 = torch.full((2, 2, n), float("nan"), device=DEV)        # [launch, segment, tensor block]
    for l in range(2):
        L.adapter_wgrad_partial(L.make_wgrad_segs([
            dict(x=x, dy=dy, z=z, dz=dz, grad=g2[l, 0], rows=h, scale=0.5),
            dict(x=x[h:], dy=dy[h:], z=z[h:], dz=dz[h:], grad=g2[l, 1], rows=T - h, scale=1.0)]), parts[l * ws:(l + 1) * ws])
    ptrs = torch.tensor([g2[l, k].data_ptr() for l in range(2) for k in range(2)], dtype=torch.int64, device=DEV)
    L.adapter_wgrad_reduce(ptrs, 2, 2, parts, ws)
    assert torch.equal(g2[0], grads) and torch.equal(g2[1], grads)


@pytest.mark.parametrize("rows", [(16, 16), (5, 9), (64, 64), (800, 128), (33, 1)])
def test_adapter_few_tiles_per_block(L, rows):
    """Launches with FEWER tiles than CUs (grid = tiles: every block has exactly one 16-token tile and nothing behind the
    weight loads in the memory pipe -- the top-layer adapter on 2B rows, the ALBEF text / answer towers): the prologue must
    wait for the tile itself, not for a count of younger requests that are not there (round-3 ADVICE: vmcnt(54) with only 42
    weight loads behind tile 0).  Forward (+ fused LayerNorm), z-path backward, both segment kinds (one adapter / gated),
    repeated with a second stream hammering HBM so that tile 0 is late; every repeat must be bit-identical and match fp32."""
    g = torch.Generator().manual_seed(rows[0] * 131 + rows[1])
    n0, n1 = rows
    T = n0 + n1
    ads = []
    for a in range(3):
        wd = (torch.randn(48, 768, generator=g) * 0.03).to(DEV)
        wu = (torch.randn(768, 48, generator=g) * 0.03).to(DEV)
        wd16, wdT16, wu16, wuT16 = _pack(L, wd, wu)
        ads.append(dict(wd=wd16, wdT=wdT16, wu=wu16, wuT=wuT16, wd32=wd, wu32=wu,
                        bd=(torch.randn(48, generator=g) * 0.02).to(DEV), bu=(torch.randn(768, generator=g) * 0.02).to(DEV)))
    x = torch.randn(T, 768, generator=g).to(DEV)
    dy = torch.randn(T, 768, generator=g).to(DEV)
    gam, bet = (1 + 0.1 * torch.randn(768, generator=g)).to(DEV), (0.1 * torch.randn(768, generator=g)).to(DEV)
    segs = L.make_segs([
        dict(row_begin=0, row_end=n0, train_slot=0, adapters=[dict(ads[0], scale=0.5), dict(ads[2], scale=0.5)]),
        dict(row_begin=n0, row_end=T, train_slot=0, adapters=[dict(ads[1], scale=1.0)]),
    ])

    def ref_ad(xx, a):
        z = F.relu(bf(xx).float() @ bf(a["wd32"]).float().t() + a["bd"])
        return bf(z).float() @ bf(a["wu32"]).float().t() + a["bu"]
    ref = torch.cat([x[:n0] + 0.5 * ref_ad(x[:n0], ads[0]) + 0.5 * ref_ad(x[:n0], ads[2]), x[n0:] + ref_ad(x[n0:], ads[1])])
    big = torch.empty(64 << 20, device=DEV)
    side = torch.cuda.Stream()
    first = None
    for rep in range(12):
        out = torch.full_like(x, float("nan"))
        y16 = torch.empty(T, 768, dtype=torch.bfloat16, device=DEV)
        st = torch.empty(T, 2, device=DEV)
        zs = torch.full((T, 2, 48), float("nan"), device=DEV)
        dx = torch.full_like(x, float("nan"))
        z, dz = torch.empty(T, 48, device=DEV), torch.empty(T, 48, device=DEV)
        if rep % 2:
            with torch.cuda.stream(side):        # contention: tile 0's DMA lands late
                big.add_(1.0)
        L.adapter_fwd_ln(x, out, segs, T, gam, bet, 1e-12, y16, st, z_save=zs)
        L.adapter_bwd(None, dy, dx, segs, T, z_out=z, dz_out=dz, z_saved=zs)
        torch.cuda.synchronize()
        got = (out.clone(), y16.clone(), zs[:, 0].clone(), dx.clone(), dz.clone())
        if first is None:
            first = got
            assert (out - ref).abs().max() < 2e-3
            assert (y16.float() - F.layer_norm(out, (768,), gam, bet, 1e-12)).abs().max() < 3e-2
            assert not torch.isnan(dx).any() and not torch.isnan(dz).any()
        else:
            for a, b in zip(first, got):
                assert torch.equal(a, b), rep
    # the recompute-from-x backward agrees with the z path (same arithmetic)
    dx2, z2, dz2 = torch.empty_like(x), torch.empty(T, 48, device=DEV), torch.empty(T, 48, device=DEV)
    L.adapter_bwd(x, dy, dx2, segs, T, z_out=z2, dz_out=dz2)
    assert torch.equal(dx2, first[3]) and torch.equal(dz2, first[4])


def test_vqa_score_accumulate(L):
    """feddat_vqa_score_accumulate == sum_b target[b, argmax logits[b]] (first maximal index), accumulated over batches."""
    g = torch.Generator().manual_seed(5)
    acc = torch.zeros(2, device=DEV)
    want, seen = 0.0, 0
    for B, C in ((32, 100), (7, 100), (1, 3129), (64, 100)):
        lg = torch.randn(B, C, generator=g)
        lg[0, 5] = lg[0, 50] = 9.0            # a tie: the first index wins
        tg = torch.rand(B, C, generator=g)
        L.vqa_score_accumulate(lg.to(DEV), tg.to(DEV), acc)
        want += float(tg.gather(1, lg.argmax(1, keepdim=True)).double().sum())
        seen += B
    got = acc.tolist()
    assert got[1] == seen and abs(got[0] - want) < 1e-4 * want


# ------------------------------------------------------------------ exact fp32 small GEMM
@pytest.mark.parametrize("I,J,K,ksplit", [(64, 1536, 768, 1), (100, 48, 5921, 16), (17, 5, 3, 2)])
def test_sgemm_f32(L, I, J, K, ksplit):
    g = torch.Generator().manual_seed(I * J)
    A = torch.randn(I, K, generator=g).to(DEV)
    Bm = torch.randn(K, J, generator=g).to(DEV)
    bias = torch.randn(J, generator=g).to(DEV)
    out = torch.empty(ksplit, I, J, device=DEV)
    cs = torch.empty(ksplit, I, device=DEV)
    L.sgemm_f32(A, K, 1, Bm, J, 1, I, J, K, out, ksplit=ksplit, alpha=0.5, bias_j=bias,
                out_split_stride=I * J, colsum=cs)
    res = torch.empty(I, J, device=DEV)
    L.reduce_partials(out, I * J, ksplit, I * J, res)
    ref = 0.5 * (A.double() @ Bm.double()) + bias.double()
    assert (res.double() - ref).abs().max() < 2e-5 * math.sqrt(K) * 4
    assert (cs.sum(0).double() - 0.5 * A.double().sum(1)).abs().max() < 1e-4 * math.sqrt(K)
    # transposed access patterns: D = A^T-view
    At = A.t().contiguous()  # [K, I]
    out2 = torch.empty(I, J, device=DEV)
    L.sgemm_f32(At, 1, I, Bm, J, 1, I, J, K, out2)
    assert (out2.double() - A.double() @ Bm.double()).abs().max() < 2e-5 * math.sqrt(K) * 4


ATTN_CLS_SHAPES = [(64, 185, 12, False), (3, 90, 12, True), (2, 281, 4, True), (1, 7, 1, False)]


@pytest.mark.parametrize("B,S,heads,masked", ATTN_CLS_SHAPES)
def test_attention_token0_only_vs_dense_and_fp32(L, B, S, heads, masked):
    """feddat_attn_cls_fwd / _bwd (the last layer: one query per (sample, head)) against fp32 attention restricted to query 0,
    and against the dense kernels fed a dctx that is zero off token 0."""
    g = torch.Generator().manual_seed(B * S + heads)
    H = heads * 64
    qkv = bf(torch.randn(B * S, 3 * H, generator=g) * 0.7).to(DEV)
    km = None
    if masked:
        km = (torch.rand(B, S, generator=g) > 0.3).to(torch.uint8)
        km[:, 0] = 1
        km = km.to(DEV)
    ctx = torch.zeros(B * S, H, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(B, heads, S, device=DEV)
    L.attn_cls_fwd(qkv, ctx, lse, B, S, heads, key_mask=km)
    q4 = qkv.float().view(B, S, 3, heads, 64)
    q0, K, V = q4[:, 0, 0], q4[:, :, 1], q4[:, :, 2]                          # [B, h, 64], [B, S, h, 64]
    sc = torch.einsum("bhd,bshd->bhs", q0, K) / 8.0
    if masked:
        sc = sc.masked_fill(km[:, None, :] == 0, float("-inf"))
    p = torch.softmax(sc, -1)
    o0 = torch.einsum("bhs,bshd->bhd", p, V)
    got0 = ctx.view(B, S, heads, 64)[:, 0].float()
    assert (got0 - o0).abs().max() < 1.5e-2
    assert (lse[:, :, 0] - torch.logsumexp(sc, -1)).abs().max() < 1e-4
    assert not ctx.view(B, S, H)[:, 1:].any()                                  # only the token-0 rows are written
    # dense forward agrees on the token-0 rows
    ctx_d, lse_d = torch.empty_like(ctx), torch.empty_like(lse)
    L.attn_fwd(qkv, ctx_d, lse_d, B, S, heads, key_mask=km)
    assert (ctx_d.view(B, S, H)[:, 0].float() - ctx.view(B, S, H)[:, 0].float()).abs().max() < 2e-2
    # backward
    d0 = torch.randn(B, H, generator=g).to(DEV)
    dqkv = torch.full((B * S, 3 * H), float("nan"), dtype=torch.bfloat16, device=DEV)
    L.attn_cls_bwd(qkv, ctx, lse, d0, dqkv, B, S, heads, key_mask=km)
    g0 = d0.view(B, heads, 64)
    o_used = got0                                                             # D uses the stored (bf16) context row
    Dv = (g0 * o_used).sum(-1, keepdim=True)
    dP = torch.einsum("bhd,bshd->bhs", g0, V)
    dS = p * (dP - Dv)
    dV = torch.einsum("bhs,bhd->bshd", p, g0)
    dK = torch.einsum("bhs,bhd->bshd", dS, q0) / 8.0
    dQ0 = torch.einsum("bhs,bshd->bhd", dS, K) / 8.0
    got = dqkv.float().view(B, S, 3, heads, 64)
    assert not torch.isnan(got).any()
    scale = lambda t: float(t.abs().max()) + 1e-6
    assert (got[:, :, 2] - dV).abs().max() < 1e-2 * scale(dV) + 1e-4
    assert (got[:, :, 1] - dK).abs().max() < 1e-2 * scale(dK) + 1e-4
    assert (got[:, 0, 0] - dQ0).abs().max() < 1e-2 * scale(dQ0) + 1e-4
    assert not got[:, 1:, 0].any()
    if S <= 192:       # the dense fused backward on the scattered gradient
        dctx = torch.zeros(B * S, H, dtype=torch.bfloat16, device=DEV)
        dctx.view(B, S, H)[:, 0] = d0.to(torch.bfloat16)
        dq_d = torch.empty_like(dqkv)
        L.attn_bwd(qkv, ctx_d, lse_d, dctx, dq_d, B, S, heads, key_mask=km)
        assert (dq_d.float() - dqkv.float()).abs().max() < 3e-2 * scale(dqkv.float()) + 1e-3


# ------------------------------------------------------------------ fused step tail (csrc/head_tail.hip)
def test_head_gemm_prologues_epilogues_and_two_jobs(L):
    """feddat_head_gemm against fp64: plain / bias, LayerNorm prologue on strided rows (+ stats), tanh epilogue, tanh'
    prologue, gelu' epilogue, the batch-contraction mode with its column sum, ragged sizes, and two jobs in one launch."""
    g = torch.Generator().manual_seed(17)
    H, nb, S = 768, 64, 5
    hl = torch.randn(nb, S * H, generator=g).to(DEV)                    # token-0 rows at stride S * H
    gam, bet = (1 + 0.1 * torch.randn(H, generator=g)).to(DEV), (0.1 * torch.randn(H, generator=g)).to(DEV)
    W = (torch.randn(H, H, generator=g) * 0.05).to(DEV)
    bias = torch.randn(H, generator=g).to(DEV)
    pooled, st = torch.empty(nb, H, device=DEV), torch.empty(nb, 2, device=DEV)
    L.head_gemm(L.ht_job(hl, S * H, 1, W, 1, H, nb, H, H, pooled, bias_j=bias, pro=L.HT_PRO_LN, pro_a=gam, pro_b=bet,
                         pro_eps=1e-12, stats_out=st, epi=L.HT_EPI_TANH))
    x = hl[:, :H].double()
    ln = F.layer_norm(x, (H,), gam.double(), bet.double(), 1e-12)
    ref = torch.tanh(ln @ W.double().t() + bias.double())
    assert (pooled.double() - ref).abs().max() < 2e-5
    assert (st[:, 0].double() - x.mean(1)).abs().max() < 1e-6
    assert (st[:, 1].double() - 1 / torch.sqrt(x.var(1, unbiased=False) + 1e-12)).abs().max() < 1e-4
    # backward through the pooler: (dpooled * (1 - pooled^2)) W
    dp = torch.randn(nb, H, generator=g).to(DEV)
    dcls = torch.empty(nb, H, device=DEV)
    L.head_gemm(L.ht_job(dp, H, 1, W, H, 1, nb, H, H, dcls, pro=L.HT_PRO_TANH_BWD, pro_a=pooled))
    assert (dcls.double() - (dp.double() * (1 - pooled.double() ** 2)) @ W.double()).abs().max() < 2e-5
    # two jobs in one launch, the head backward's first pair: dW_fc1 = dl^T g0 (+ db) | dn0 = (dl W1) * gelu'(n0); ragged B, C
    for B, C, H2 in ((32, 100, 1536), (7, 37, 200)):
        dl = torch.randn(B, C, generator=g).to(DEV)
        g0, n0 = torch.randn(B, H2, generator=g).to(DEV), torch.randn(B, H2, generator=g).to(DEV)
        W1 = (torch.randn(C, H2, generator=g) * 0.05).to(DEV)
        dW, db = torch.full((C, H2), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
        dn0 = torch.full((B, H2), float("nan"), device=DEV)
        L.head_gemm(L.ht_job(dl, 1, C, g0, H2, 1, C, H2, B, dW, mode=1, colsum=db),
                    L.ht_job(dl, C, 1, W1, H2, 1, B, H2, C, dn0, epi=L.HT_EPI_MUL_DGELU, aux=n0, ld_aux=H2))
        n0d = n0.double()
        gp = 0.5 * (1 + torch.erf(n0d / math.sqrt(2))) + n0d * torch.exp(-0.5 * n0d ** 2) / math.sqrt(2 * math.pi)
        assert (dW.double() - dl.double().t() @ g0.double()).abs().max() < 2e-5
        assert (db.double() - dl.double().sum(0)).abs().max() < 2e-5
        assert (dn0.double() - (dl.double() @ W1.double()) * gp).abs().max() < 2e-5
    with pytest.raises(L.FeddatHipError):
        L.head_gemm(L.ht_job(dp, H, 1, W, H, 1, nb, H, H, dcls, pro=L.HT_PRO_LN))        # LN without gamma / beta


def test_head_layernorm_gelu_and_full_backward(L):
    g = torch.Generator().manual_seed(19)
    for rows, H in ((64, 1536), (5, 100)):
        x = torch.randn(rows, H, generator=g)
        gam, bet = 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
        dy = torch.randn(rows, H, generator=g)
        y, st, ge = torch.empty(rows, H, device=DEV), torch.empty(rows, 2, device=DEV), torch.empty(rows, H, device=DEV)
        L.head_ln_gelu(x.to(DEV), gam.to(DEV), bet.to(DEV), 1e-5, y, st, ge)
        xd = x.double().requires_grad_(True)
        gd, bd = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
        yr = F.layer_norm(xd, (H,), gd, bd, 1e-5)
        assert (y.cpu().double() - yr).abs().max() < 2e-6 and (ge.cpu().double() - F.gelu(yr)).abs().max() < 2e-6
        yr.backward(dy.double())
        dx, dg, db = torch.empty(rows, H, device=DEV), torch.empty(H, device=DEV), torch.empty(H, device=DEV)
        L.head_ln_bwd_full(dy.to(DEV), x.to(DEV), st, gam.to(DEV), dx, dg, db)
        assert (dx.cpu().double() - xd.grad).abs().max() < 1e-5
        assert (dg.cpu().double() - gd.grad).abs().max() < 1e-5 and (db.cpu().double() - bd.grad).abs().max() < 1e-5
        # ... and it is the two-launch form (feddat_layernorm_bwd_full) bit for bit on the affine gradients
        dx2, dg2, db2 = torch.empty_like(dx), torch.empty_like(dg), torch.empty_like(db)
        L.layernorm_bwd_full(dy.to(DEV), x.to(DEV), st, gam.to(DEV), rows, H, dx2, dg2, db2)
        assert torch.equal(dg, dg2) and torch.equal(db, db2) and (dx - dx2).abs().max() < 1e-6


def test_loss_single_launch_and_adamw_multi_match_the_separate_launches(L, golden_dir):
    g = load(golden_dir, "g2_loss.npz")
    lg, te, ta = (torch.from_numpy(g[k]).to(DEV) for k in ("logits", "teacher", "target"))
    gen = torch.Generator().manual_seed(2)
    for lgs, tes, tas in ((lg, te, ta), tuple(torch.randn(32, 100, generator=gen).to(DEV) for _ in range(3)),
                          tuple(torch.randn(70, 33, generator=gen).to(DEV) for _ in range(3))):
        B = lgs.shape[0]
        dl1, dl2 = torch.empty_like(lgs), torch.empty_like(lgs)
        sc1, sc2 = torch.zeros(4 + 2 * B, device=DEV), torch.zeros(4, device=DEV)
        L.dat_loss_fwd_bwd(lgs, tes, tas, dl1, sc1)
        L.dat_loss_fwd_bwd_single(lgs, tes, tas, dl2, sc2)
        # (same formulas; hipcc contracts the two bodies' multiply-adds differently: last-bit differences)
        assert (dl1 - dl2).abs().max() < 1e-8 and (sc1[:3] - sc2[:3]).abs().max() < 1e-5 * sc1[:3].abs().max()
    # three groups in one launch, the middle one reading its counters one ahead == separate launches with a tick between
    sizes = (48 * 768 + 48, 1536 * 4, 768 * 48 + 768)
    def mk():
        gg = torch.Generator().manual_seed(9)
        out = []
        for n in sizes:
            p, gr = (torch.randn(n, generator=gg) * 0.05).to(DEV), torch.randn(n, generator=gg).to(DEV)
            m, v = (torch.randn(n, generator=gg) * 0.01).to(DEV), (torch.rand(n, generator=gg) * 0.01).to(DEV)
            seg_off = torch.tensor([0, n // 2, n], dtype=torch.int64, device=DEV)
            seg_wd = torch.tensor([0.01, 0.0], device=DEV)
            out.append([p, gr, m, v, seg_off, seg_wd])
        return out
    A, Bg = mk(), mk()
    states = [torch.tensor(s, dtype=torch.int32, device=DEV) for s in ([6, 3], [6, 6], [7, 3])]
    states_b = [s.clone() for s in states]
    L.adamw_multi([L.adamw_group(*A[0], states[0]), L.adamw_group(*A[1], states[1], 1, 1), L.adamw_group(*A[2], states[2])],
                  1e-4, 5, 60, 0.9, 0.98, 1e-8)
    L.step_tick_multi(states, [2, 2, 2], [1, 2, 1])
    L.step_tick(states_b[1], 1, 1)
    for k in range(3):
        L.adamw_flat(Bg[k][0], Bg[k][1], Bg[k][2], Bg[k][3], Bg[k][4], Bg[k][5], states_b[k], 1e-4, 5, 60, 0.9, 0.98, 1e-8)
    L.step_tick(states_b[0], 2, 1)
    L.step_tick(states_b[1], 1, 1)
    L.step_tick(states_b[2], 2, 1)
    torch.cuda.synchronize()
    for k in range(3):
        for a, b in zip(A[k][:4], Bg[k][:4]):
            assert torch.equal(a, b), k
        assert torch.equal(states[k], states_b[k])
    assert float((A[0][0] - mk()[0][0]).abs().max()) > 0


# ------------------------------------------------------------------ K5 loss
def test_loss_vs_reference_golden(L, golden_dir):
    g = load(golden_dir, "g2_loss.npz")
    lg = torch.from_numpy(g["logits"]).to(DEV)
    te = torch.from_numpy(g["teacher"]).to(DEV)
    ta = torch.from_numpy(g["target"]).to(DEV)
    dl = torch.empty_like(lg)
    sc = torch.empty(4 + 2 * lg.shape[0], device=DEV)
    L.dat_loss_fwd_bwd(lg, te, ta, dl, sc)
    assert abs(float(sc[0]) - float(g["bce"])) < 1e-4
    assert abs(float(sc[1]) - float(g["kl"])) < 1e-5
    assert abs(float(sc[2]) - float(g["L"])) < 1e-4
    assert (dl.cpu() - torch.from_numpy(g["dlogits"])).abs().max() < 1e-6


# ------------------------------------------------------------------ K6 AdamW + schedule
@pytest.mark.parametrize("shapes", [[(48, 768), (48,), (1536,), (768,)],        # quad-aligned tensors (the engine's layouts)
                                    [(47, 3), (7,), (1530,), (10,)]])           # tensor boundaries inside quads, n % 4 == 0
def test_adamw_flat_vs_oracle(L, shapes):
    g = torch.Generator().manual_seed(5)
    names = ["w.weight", "w.bias", "clf_norm0.weight", "x.LayerNorm.weight"]
    P = {n: torch.randn(s, generator=g) * 0.05 for n, s in zip(names, shapes)}
    offs = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
    flat = torch.cat([P[n].flatten() for n in names]).to(DEV)
    m = torch.zeros_like(flat)
    v = torch.zeros_like(flat)
    seg_off = torch.tensor(offs, dtype=torch.int64, device=DEV)
    seg_wd = torch.tensor([0.0 if O.is_no_decay(n) else 0.01 for n in names], device=DEV)
    state = torch.zeros(2, dtype=torch.int32, device=DEV)
    opt = O.AdamWState(names, 1e-4)
    warm, total = 3, 40
    for t in range(6):
        grads = {n: torch.randn(s, generator=g) * (10.0 ** -t) for n, s in zip(names, shapes)}
        gflat = torch.cat([grads[n].flatten() for n in names]).to(DEV)
        L.adamw_flat(flat, gflat, m, v, seg_off, seg_wd, state, 1e-4, warm, total)
        L.step_tick(state, 1, 1)
        opt.step(P, grads, 1e-4 * O.poly_lr_lambda(t, warm, total))
    ref = torch.cat([P[n].flatten() for n in names])
    assert (flat.cpu() - ref).abs().max() < 2e-7
    assert state.tolist() == [6, 6]


# ------------------------------------------------------------------ K2 attention
def _attn_ref(qkv, B, S, heads, mask=None):
    H = heads * 64
    q, k, v = (qkv[:, i * H:(i + 1) * H].float().reshape(B, S, heads, 64).transpose(1, 2) for i in range(3))
    sc = q @ k.transpose(-1, -2) / 8.0
    if mask is not None:
        sc = sc.masked_fill(~mask[:, None, None, :].bool(), float("-inf"))
    p = torch.softmax(sc, -1)
    ctx = (p @ v).transpose(1, 2).reshape(B * S, H)
    return ctx, torch.logsumexp(sc, -1)


ATTN_SHAPES = [(2, 185, 12, False), (3, 90, 12, True), (1, 33, 2, True), (64, 185, 12, False), (2, 281, 12, True),
               (1, 320, 3, False)]


@pytest.mark.parametrize("B,S,heads,masked", ATTN_SHAPES)
def test_attention_fwd_bwd(L, B, S, heads, masked):
    g = torch.Generator().manual_seed(S)
    H = heads * 64
    qkv = bf(torch.randn(B * S, 3 * H, generator=g)).to(DEV)
    mask = None
    if masked:
        mask = torch.ones(B, S, dtype=torch.uint8)
        for b in range(B):
            mask[b, 20 + 3 * b: 20 + 3 * b + 7] = 0
        mask = mask.to(DEV)
    ctx = torch.empty(B * S, H, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B, heads, S, device=DEV)
    L.attn_fwd(qkv, ctx, lse, B, S, heads, key_mask=mask)
    qr = qkv.float().requires_grad_(True)
    cref, lref = _attn_ref(qr, B, S, heads, mask)
    assert rel_err(ctx, cref) < 1.5e-2
    assert (lse - lref).abs().max() < 2e-3
    dctx = bf(torch.randn(B * S, H, generator=g)).to(DEV)
    cref.backward(dctx.float())
    dqkv = torch.full((B * S, 3 * H), float("nan"), dtype=torch.bfloat16, device=DEV)
    L.attn_bwd(qkv, ctx, lse, dctx, dqkv, B, S, heads, key_mask=mask)
    for part, name in enumerate("QKV"):
        a = dqkv[:, part * H:(part + 1) * H]
        r = qr.grad[:, part * H:(part + 1) * H]
        assert torch.isfinite(a.float()).all(), name
        assert rel_err(a, r) < 3e-2, (name, rel_err(a, r))


# ------------------------------------------------------------------ K8 embeddings
@pytest.mark.parametrize("res", [224, 384])
def test_embeddings_vs_oracle(L, res):
    d = O.ViltDims(layers=1)
    P = O.make_params(d, ["art"], bias_std=0.02)
    batch = O.synthetic_batch(3, res, 99)
    ref = O.vilt_embed(P, d, batch)            # [B,S,H] fp32, CPU oracle
    B, S, H = ref.shape
    e = O.ENC + "embeddings."
    dev = {k: v.to(DEV) for k, v in P.items() if k.startswith(e)}
    h = torch.full((B, S, H), float("nan"), device=DEV)
    tok = dev[e + "token_type_embeddings.weight"]
    L.text_embed(batch["input_ids"].to(DEV), batch["token_type_ids"].to(DEV),
                 dev[e + "text_embeddings.word_embeddings.weight"],
                 dev[e + "text_embeddings.position_embeddings.weight"],
                 dev[e + "text_embeddings.token_type_embeddings.weight"],
                 dev[e + "text_embeddings.LayerNorm.weight"], dev[e + "text_embeddings.LayerNorm.bias"], d.ln_eps,
                 tok[0].contiguous(), h, B, 40, S, H)
    gsz = res // 32
    npatch = gsz * gsz
    patches = torch.empty(B * npatch, 3072, dtype=torch.bfloat16, device=DEV)
    L.im2col_patches(batch["pixel_values"].to(DEV), patches, B, 3, res, res, 32)
    ref_patches = F.unfold(batch["pixel_values"], 32, stride=32).transpose(1, 2).reshape(B * npatch, 3072)
    assert torch.equal(patches.cpu(), bf(ref_patches))
    wp = bf(dev[e + "patch_embeddings.projection.weight"].reshape(768, 3072))
    proj = torch.empty(B * npatch, 768, device=DEV)
    L.gemm_bf16_nt(patches, wp, L.EPI_F32, bias=dev[e + "patch_embeddings.projection.bias"], out_f32=proj)
    pos = dev[e + "position_embeddings"][0]
    pos_img = torch.empty(npatch, 768, device=DEV)
    L.pos_embed_resize(pos[1:].contiguous(), pos_img, 12, gsz, gsz, 768)
    ref_pos = O.interp_pos_embed(P, d, gsz, gsz)[0]
    assert (pos_img.cpu() - ref_pos).abs().max() < 1e-6
    L.image_embed_assemble(proj, dev[e + "cls_token"].reshape(768), pos[0].contiguous(), pos_img,
                           tok[1].contiguous(), h, B, 40, npatch, S, H)
    torch.cuda.synchronize()
    assert (h[:, :41].cpu() - ref[:, :41]).abs().max() < 2e-5          # text rows + CLS: fp32 exact path
    assert (h[:, 41:].cpu() - ref[:, 41:]).abs().max() < 2e-2          # bf16 patch projection (K = 3072)


# ------------------------------------------------------------------ misc
def test_misc_elementwise_and_fedavg(L, golden_dir):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1000, generator=g).to(DEV)
    y = x.clone()
    L.tanh_fwd(y)
    assert (y - torch.tanh(x)).abs().max() < 1e-6
    dy = torch.randn(1000, generator=g).to(DEV)
    dx = torch.empty_like(x)
    L.tanh_bwd(y, dy, dx)
    assert (dx - dy * (1 - torch.tanh(x) ** 2)).abs().max() < 1e-5
    L.gelu_fwd(x, y)
    assert (y - F.gelu(x)).abs().max() < 1e-6
    xr = x.clone().requires_grad_(True)
    F.gelu(xr).backward(dy)
    L.gelu_bwd(x, dy, dx)
    assert (dx - xr.grad).abs().max() < 1e-5
    w = torch.randn(70, 130, generator=g).to(DEV)
    o = torch.empty(130, 70, dtype=torch.bfloat16, device=DEV)
    L.transpose_f32_bf16(w, o, 70, 130)
    assert torch.equal(o, bf(w).t().contiguous())
    o2 = torch.empty(70 * 130, dtype=torch.bfloat16, device=DEV)
    L.cvt_f32_bf16(w, o2)
    assert torch.equal(o2, bf(w).flatten())
    rows = torch.randn(3, 768, generator=g).to(DEV)
    o32 = torch.full((3 * 5, 768), float("nan"), device=DEV)
    o16 = torch.full((3 * 5, 768), float("nan"), dtype=torch.bfloat16, device=DEV)
    L.scatter_cls_rows(rows, o32, o16, 3, 5, 768)
    exp = torch.zeros(3, 5, 768, device=DEV)
    exp[:, 0] = rows
    assert torch.equal(o32, exp.reshape(15, 768)) and torch.equal(o16, bf(exp.reshape(15, 768)))
    # FedAvg accumulate: bit-exact with the reference's get_average_net (main.py:50-65) golden
    gd = load(golden_dir, "g5_fedavg.npz")
    keys = [k[4:] for k in gd if k.startswith("avg.")]
    nums = list(gd["nums"])
    for k in keys[:4]:
        acc = torch.empty(gd["avg." + k].shape, device=DEV)
        for i in range(5):
            L.fedavg_accumulate(acc, torch.from_numpy(gd[f"c{i}.{k}"]).to(DEV), nums[i], sum(nums), i == 0)
        assert torch.equal(acc.cpu(), torch.from_numpy(gd["avg." + k])), k


def test_padded_image_masks_and_position_grids(L):
    """feddat_vilt_key_mask / feddat_pos_embed_resize_masked vs the oracle's restatement of HF visual_embed."""
    d = O.ViltDims(layers=1)
    P = O.make_params(d, ["art"], bias_std=0.02)
    b = O.pad_batch(O.synthetic_batch(4, 384, 5), [(384, 384), (256, 384), (384, 224), (32, 64)], [40, 31, 40, 1])
    B, Lt, S = 4, 40, 40 + 1 + 144
    km = torch.zeros(2 * B, S, dtype=torch.uint8, device=DEV)
    L.vilt_key_mask(b["attention_mask"].to(DEV), b["pixel_mask"].to(DEV), km, B, Lt, 384, 384, 32, nrep=2)
    want = O.key_mask(b, 145, d)
    assert torch.equal(km[:B].bool().cpu(), want) and torch.equal(km[B:].bool().cpu(), want)
    km1 = torch.zeros(B, S, dtype=torch.uint8, device=DEV)
    L.vilt_key_mask(None, None, km1, B, Lt, 384, 384, 32)
    assert bool(km1.all())
    pos = P[O.ENC + "embeddings.position_embeddings"][0, 1:].contiguous().to(DEV)
    out = torch.empty(B, 144, 768, device=DEV)
    L.pos_embed_resize_masked(pos, b["pixel_mask"].to(DEV), out, 12, B, 384, 384, 32, 768)
    for i, (h, w) in enumerate([(12, 12), (8, 12), (12, 7), (1, 2)]):
        ref = torch.nn.functional.pad(O.interp_pos_embed(P, d, h, w).transpose(1, 2).reshape(1, 768, h, w),
                                      (0, 12 - w, 0, 12 - h)).flatten(2).transpose(1, 2)[0]
        assert (out[i].cpu() - ref).abs().max() < 2e-6, i


def test_adapter_fwd_with_fused_layernorm(L, golden_dir):
    """feddat_adapter_fwd_ln = feddat_adapter_fwd followed by feddat_layernorm_fwd on its output (incl. a ragged tail)."""
    g, par = _golden_adapter(L, golden_dir)
    T = 1000 + 7
    x = torch.randn(T, 768, generator=torch.Generator().manual_seed(11)).to(DEV)
    h = 16 * 31 + 5
    segs = L.make_segs([dict(row_begin=0, row_end=h, adapters=[dict(par[0], scale=0.5), dict(par[2], scale=0.5)]),
                        dict(row_begin=h, row_end=T, adapters=[dict(par[1], scale=1.0)])])
    gg = torch.Generator().manual_seed(12)
    gamma, beta = torch.randn(768, generator=gg).to(DEV), torch.randn(768, generator=gg).to(DEV)
    out_a, out_b = torch.zeros_like(x), torch.zeros_like(x)
    y_a = torch.zeros(T, 768, dtype=torch.bfloat16, device=DEV)
    y_b = torch.zeros_like(y_a)
    st_a, st_b = torch.zeros(T, 2, device=DEV), torch.zeros(T, 2, device=DEV)
    L.adapter_fwd(x, out_a, segs, T)
    L.layernorm_fwd(out_a, gamma, beta, 1e-12, T, 768, y_bf16=y_a, stats=st_a)
    L.adapter_fwd_ln(x, out_b, segs, T, gamma, beta, 1e-12, y_b, st_b)
    assert torch.equal(out_a, out_b)
    assert (st_a - st_b).abs().max() < 1e-4 * st_a.abs().max()
    # at most one bf16 ulp (the fused kernel combines per-wave (mean, M2) pairs, the stand-alone one sums all 768 columns in
    # two passes: mean / rstd agree to ~1e-7 relative), or 1e-5 absolute where (x - mean) rstd gamma + beta cancels to ~0
    dy_ = (y_a.float() - y_b.float()).abs()
    assert bool((dy_ <= torch.maximum(y_a.float().abs(), y_b.float().abs()) * 2 ** -7 + 1e-5).all())
    assert ((y_a.float() - y_b.float()).abs() > 0).float().mean() < 0.02


SKINNY_SHAPES = [(64, 768, 3072), (64, 3072, 768), (8, 768, 768), (37, 768, 3072)]


@pytest.mark.parametrize("M,N,K", SKINNY_SHAPES)
def test_gemm_skinny_all_epilogues(L, M, N, K):
    """Split-K skinny GEMM (top layer, 2B token-0 rows) against the same fp32 restatement as the big kernel, with a
    strided A operand and residual as the engine passes them."""
    torch.manual_seed(M + N)
    Abig = torch.randn(M, 3, K, device=DEV).to(torch.bfloat16)
    A = Abig[:, 0]                                   # row stride 3K
    Bw = (torch.randn(N, K, device=DEV) * 0.03).to(torch.bfloat16)
    bias = torch.randn(N, device=DEV)
    resid_big = torch.randn(M, 2, N, device=DEV)
    resid = resid_big[:, 1]
    aux = torch.randn(M, N, device=DEV).to(torch.bfloat16)
    ws = torch.empty(L.gemm_skinny_workspace_elems(M, N, K), device=DEV)
    ref = A.float() @ Bw.float().t()
    o16 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    o2 = torch.zeros_like(o16)
    o32 = torch.zeros(M, N, device=DEV)
    tol = 2e-2 * ref.abs().max().item()
    L.gemm_bf16_nt(A, Bw, L.EPI_BF16, bias=bias, out_bf16=o16, skinny_workspace=ws)
    assert (o16.float() - (ref + bias)).abs().max() < tol
    L.gemm_bf16_nt(A, Bw, L.EPI_RESID_F32, bias=bias, resid=resid, out_f32=o32, skinny_workspace=ws)
    assert (o32 - (ref + bias + resid)).abs().max() < 1e-3 * ref.abs().max().item() + 1e-4
    L.gemm_bf16_nt(A, Bw, L.EPI_GELU, bias=bias, out_bf16=o16, out2_bf16=o2, skinny_workspace=ws)
    assert (o2.float() - (ref + bias)).abs().max() < tol
    assert (o16.float() - F.gelu(ref + bias)).abs().max() < tol
    L.gemm_bf16_nt(A, Bw, L.EPI_MUL_DGELU, aux=aux, out_bf16=o16, skinny_workspace=ws)
    u = aux.float().requires_grad_(True)
    F.gelu(u).sum().backward()
    assert (o16.float() - ref * u.grad).abs().max() < tol
    L.gemm_bf16_nt(A, Bw, L.EPI_F32, out_f32=o32, skinny_workspace=ws)
    assert (o32 - ref).abs().max() < 1e-3 * ref.abs().max().item() + 1e-4
    # the one-launch form (K split over the waves of a block) against the split-K + epilogue pair it replaced (debug flag 128)
    o32b = torch.zeros(M, N, device=DEV)
    L.set_debug_flags(128)
    try:
        L.gemm_bf16_nt(A, Bw, L.EPI_RESID_F32, bias=bias, resid=resid, out_f32=o32b, skinny_workspace=ws)
    finally:
        L.set_debug_flags(0)
    L.gemm_bf16_nt(A, Bw, L.EPI_RESID_F32, bias=bias, resid=resid, out_f32=o32, skinny_workspace=ws)
    assert (o32 - o32b).abs().max() < 2e-5 * ref.abs().max().item() + 1e-5


@pytest.mark.parametrize("M,N,K,epi", [(11840, 3072, 768, 2), (11840, 768, 3072, 1), (5920, 2304, 768, 0)])
def test_gemm_race_screen_bit_identical_repeats(L, M, N, K, epi):
    """The persistent ping-pong GEMM orders its LDS stages by barrier slots only; a missed ordering shows up as rare
    wrong tiles.  The kernel is deterministic, so 60 repeats of a multi-round launch must be bit-identical."""
    torch.manual_seed(1)
    A = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    Bw = (torch.randn(N, K, device=DEV) * 0.02).to(torch.bfloat16)
    bias, resid = torch.randn(N, device=DEV), torch.randn(M, N, device=DEV)
    o16 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    o2, o32 = torch.empty_like(o16), torch.empty(M, N, device=DEV)
    kw = {0: dict(bias=bias, out_bf16=o16), 1: dict(bias=bias, resid=resid, out_f32=o32),
          2: dict(bias=bias, out_bf16=o16, out2_bf16=o2)}[epi]
    out = o32 if epi == 1 else o16
    L.gemm_bf16_nt(A, Bw, epi, **kw)
    first = out.clone()
    for _ in range(60):
        out.zero_()
        L.gemm_bf16_nt(A, Bw, epi, **kw)
        assert torch.equal(out, first)


# ------------------------------------------------------------------ contexts / RCCL-direct collective
def test_two_contexts_in_one_process_and_threads(L):
    """Two feddat_ctx handles (a one-GPU box: both on device 0) and launches from two host threads: the per-device caches
    are keyed by device and mutex-guarded, nothing is first-caller-wins."""
    import threading
    c0, c1 = L.Context(0), L.Context(0)
    assert c0.info() == c1.info() and c0.info()[1] >= 64
    A = bf(torch.randn(1200, 768, device=DEV))
    Bw = bf(torch.randn(768, 768, device=DEV) * 0.05)
    ref = A.float() @ Bw.float().t()
    outs, errs = [None, None], []

    def work(i):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                o = torch.empty(1200, 768, dtype=torch.bfloat16, device=DEV)
                for _ in range(20):
                    L.gemm_bf16_nt(A, Bw, L.EPI_BF16, out_bf16=o)
                s.synchronize()
                outs[i] = o
        except Exception as e:      # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    assert torch.equal(outs[0], outs[1]) and rel_err(outs[0], ref) < 1.5e-2
    c0.close()
    c1.close()


def test_fedavg_allreduce_through_the_c_abi_single_rank(L):
    """feddat_comm_* + feddat_fedavg_allreduce with a 1-rank RCCL communicator (all a one-GPU box can hold): run-time RCCL
    binding, pre-scale in the reference's op order, all-reduce, write-back."""
    comm = L.RcclComm(1, 0, lambda ident: ident)
    g = torch.Generator().manual_seed(5)
    flat = torch.randn(894528, generator=g).to(DEV)
    # the reference's CPU arithmetic (main.py:62): (x * num) / total with a true fp32 division (torch's GPU scalar division
    # multiplies by the reciprocal instead, so it is not the yardstick)
    want = torch.from_numpy((flat.cpu().numpy() * np.float32(3.0)) / np.float32(7.0)).to(DEV)
    scratch = torch.empty_like(flat)
    comm.fedavg_allreduce(flat, scratch, 3.0, 7.0)
    torch.cuda.synchronize()
    assert torch.equal(flat, want)
    comm.close()


# ------------------------------------------------------------------ K2b general attention (ALBEF path)
ATTN2_SHAPES = [
    (2, 577, 577, 12, False, False),     # ViT-B/16 at 384 x 384
    (3, 25, 577, 12, False, False),      # text -> image cross-attention
    (3, 25, 25, 12, False, True),        # text self-attention with padded questions
    (5, 7, 7, 12, True, True),           # decoder: causal + padded answers
    (5, 7, 25, 12, False, True),         # decoder -> question cross-attention
    (1, 130, 200, 2, True, False),       # causal across chunk boundaries
    (2, 300, 130, 2, True, True),        # 128-row blocks, ragged last block, causal + mask, Sq > Skv
    (2, 64, 65, 3, False, True),         # Sq on the 64-row kernel, Skv just over it
    # the mask-free instantiations (no key mask, not causal) and their short last chunks
    (2, 200, 130, 3, False, False),      # last key chunk of 2 (a quarter / half chunk), last query chunk of 8
    (2, 128, 192, 2, False, False),      # whole chunks only: nothing is ever masked
    (2, 100, 100, 2, False, False),      # last chunk of 36 keys: forward on the masking kernel, backward mask-free
    (1, 70, 90, 2, False, False),        # last chunks of 26 keys / 6 queries
]


@pytest.mark.parametrize("B,Sq,Skv,heads,causal,masked", ATTN2_SHAPES)
def test_attn2_fwd_bwd_vs_fp32_reference(L, B, Sq, Skv, heads, causal, masked):
    g = torch.Generator().manual_seed(Sq * 1000 + Skv)
    H = heads * 64
    q = bf(torch.randn(B * Sq, H, generator=g)).to(DEV)
    kv = bf(torch.randn(B * Skv, 2 * H, generator=g)).to(DEV)       # [K | V] fused, as a cross-attention K/V GEMM leaves it
    k, v = kv[:, :H], kv[:, H:]
    do = bf(torch.randn(B * Sq, H, generator=g)).to(DEV)
    km = None
    if masked:
        km = torch.ones(B, Skv, dtype=torch.uint8)
        for b in range(B):
            km[b, max(1, Skv - 1 - 2 * b):] = 0
        km = km.to(DEV)
    ctx = torch.zeros(B * Sq, H, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(B, heads, Sq, device=DEV)
    L.attn2_fwd(q, k, v, ctx, lse, B, Sq, Skv, heads, key_mask=km, causal=causal)
    # fp32 restatement on the same bf16-rounded operands
    qr = q.float().view(B, Sq, heads, 64).transpose(1, 2).requires_grad_(True)
    kr = k.float().reshape(B, Skv, heads, 64).transpose(1, 2).requires_grad_(True)
    vr = v.float().reshape(B, Skv, heads, 64).transpose(1, 2).requires_grad_(True)
    sc = qr @ kr.transpose(-1, -2) / 8.0
    if km is not None:
        sc = sc + (1.0 - km.float())[:, None, None, :] * -10000.0      # the reference's additive mask
    if causal:
        sc = sc + torch.triu(torch.full((Sq, Skv), -10000.0, device=DEV), diagonal=1)
    pr = sc.softmax(-1)
    ref = (pr @ vr).transpose(1, 2).reshape(B * Sq, H)
    assert (ctx.float() - ref).abs().max() < 2e-2
    assert (lse - torch.logsumexp(sc, -1)).abs().max() < 2e-3
    ref.backward(do.float())
    dq = torch.zeros_like(q)
    dkv = torch.zeros_like(kv)
    ws = torch.empty(B, heads, Sq, device=DEV)
    L.attn2_bwd(q, k, v, ctx, lse, do, ws, dq, dkv[:, :H], dkv[:, H:], B, Sq, Skv, heads, key_mask=km, causal=causal)
    for got, want in ((dq, qr.grad.transpose(1, 2).reshape(B * Sq, H)),
                      (dkv[:, :H], kr.grad.transpose(1, 2).reshape(B * Skv, H)),
                      (dkv[:, H:], vr.grad.transpose(1, 2).reshape(B * Skv, H))):
        assert rel_err(got, want) < 2e-2, rel_err(got, want)


# ------------------------------------------------------------------ configs[4]: fp8 (e4m3) frozen linears
def _fp8_deq(y8, scale):
    return y8.view(torch.float8_e4m3fn).float() * scale[:, None]


@pytest.mark.parametrize("rows,cols", [(2304, 768), (37, 3072)])
def test_quant_rows_fp8(L, rows, cols):
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, cols, generator=g) * torch.rand(rows, 1, generator=g) * 3).to(DEV)
    x[3] = 0.0                                                     # an all-zero row must not divide by zero
    y8 = torch.empty(rows, cols, dtype=torch.uint8, device=DEV)
    sc = torch.empty(rows, device=DEV)
    L.quant_rows_fp8(x, y8, sc)
    amax = x.abs().amax(1)
    assert torch.allclose(sc, torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)), rtol=1e-6)
    ref8 = (x / sc[:, None]).to(torch.float8_e4m3fn)               # torch's own round-to-nearest-even e4m3 conversion
    assert torch.equal(y8.view(torch.float8_e4m3fn).float(), ref8.float())
    assert (_fp8_deq(y8, sc) - x).abs().max() <= (amax.max() / 448.0) * 16 + 1e-6     # half an ulp at the top binade


def test_layernorm_fwd_fp8(L):
    rows, H = 500, 768
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(rows, H, generator=g) * 2).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(H, generator=g)).to(DEV), (0.1 * torch.randn(H, generator=g)).to(DEV)
    y8 = torch.empty(rows, H, dtype=torch.uint8, device=DEV)
    sc = torch.empty(rows, device=DEV)
    y16 = torch.empty(rows, H, dtype=torch.bfloat16, device=DEV)
    st = torch.empty(rows, 2, device=DEV)
    L.layernorm_fwd_fp8(x, gamma, beta, 1e-12, rows, H, y8, sc, y_bf16=y16, stats=st)
    ref = F.layer_norm(x, (H,), gamma, beta, 1e-12)
    assert rel_err(y16, ref) < 1e-2
    assert torch.allclose(sc, ref.abs().amax(1) / 448.0, rtol=1e-4)
    assert torch.equal(y8.view(torch.float8_e4m3fn).float(), (ref / sc[:, None]).to(torch.float8_e4m3fn).float()) or \
        (_fp8_deq(y8, sc) - ref).abs().max() < 0.07 * ref.abs().max()


def test_layernorm_bwd_dx_fp8(L):
    """The LayerNorm backward that also leaves its result as e4m3 rows + per-row scale: fp32 / bf16 outputs identical to the
    plain entry point, the fp8 copy = torch's round-to-nearest e4m3 of out / (amax / 448)."""
    rows, H = 1003, 768
    g = torch.Generator().manual_seed(5)
    x = torch.randn(rows, H, generator=g).to(DEV)
    dy = (torch.randn(rows, H, generator=g) * 1e-4).to(torch.bfloat16).to(DEV)
    dres = (torch.randn(rows, H, generator=g) * 1e-4).to(DEV)
    gamma = (1 + 0.1 * torch.randn(H, generator=g)).to(DEV)
    st = torch.empty(rows, 2, device=DEV)
    y = torch.empty(rows, H, dtype=torch.bfloat16, device=DEV)
    L.layernorm_fwd(x, gamma, torch.zeros(H, device=DEV), 1e-12, rows, H, y_bf16=y, stats=st)
    o_a, o_b = torch.empty(rows, H, device=DEV), torch.empty(rows, H, device=DEV)
    L.layernorm_bwd_dx(x, st, gamma, rows, H, dy_bf16=dy, dres=dres, out_f32=o_a)
    o8 = torch.empty(rows, H, dtype=torch.uint8, device=DEV)
    sc = torch.empty(rows, device=DEV)
    L.layernorm_bwd_dx_fp8(x, st, gamma, rows, H, o8, sc, dy_bf16=dy, dres=dres, out_f32=o_b)
    assert torch.equal(o_a, o_b)
    amax = o_a.abs().amax(1)
    assert torch.allclose(sc, amax / 448.0, rtol=1e-6)
    # the kernel multiplies by 1 / scale, torch divides: codes may differ by one step at a rounding tie -> compare dequantised
    deq = o8.view(torch.float8_e4m3fn).float() * sc[:, None]
    assert bool(((deq - o_a).abs() <= amax[:, None] * (2.0 ** -4) + 1e-12).all())          # half a step of e4m3's 3-bit mantissa
    same = (o8.view(torch.float8_e4m3fn).float() == (o_a / sc[:, None]).to(torch.float8_e4m3fn).float()).float().mean()
    assert float(same) > 0.99


@pytest.mark.parametrize("M,N,K,epi", [(11840, 2304, 768, 0), (11840, 3072, 768, 2), (5920, 3072, 768, 2), (1200, 192, 256, 0),
                                       (11840, 3072, 768, 3), (11849, 768, 768, 0), (1200, 384, 128, 3)])
def test_gemm_fp8_vs_fp32_on_the_dequantised_operands(L, M, N, K, epi):
    """The kernel's own arithmetic: e4m3 x e4m3 products are exact in fp32, so against an fp32 product of the dequantised
    operands only the accumulation order and the bf16 output rounding differ."""
    g = torch.Generator().manual_seed(M + N)
    A = torch.randn(M, K, generator=g).to(DEV)
    W = (torch.randn(N, K, generator=g) * 0.05).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    A8, sa = torch.empty(M, K, dtype=torch.uint8, device=DEV), torch.empty(M, device=DEV)
    W8, sw = torch.empty(N, K, dtype=torch.uint8, device=DEV), torch.empty(N, device=DEV)
    L.quant_rows_fp8(A, A8, sa)
    L.quant_rows_fp8(W, W8, sw)
    ref = _fp8_deq(A8, sa) @ _fp8_deq(W8, sw).t() + bias
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    if epi == 0:
        L.gemm_fp8_nt(A8, sa, W8, sw, L.EPI_BF16, bias=bias, out_bf16=out)
        assert rel_err(out, ref) < 1e-2
    elif epi == 3:      # the dX product of FFN2: (dY W2) . gelu'(u), A8 = e4m3 gradient rows, no bias
        aux = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)
        L.gemm_fp8_nt(A8, sa, W8, sw, L.EPI_MUL_DGELU, aux=aux, out_bf16=out)
        a32 = aux.float().requires_grad_(True)
        F.gelu(a32).sum().backward()
        assert rel_err(out, (ref - bias) * a32.grad) < 1e-2
    else:
        u = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        L.gemm_fp8_nt(A8, sa, W8, sw, L.EPI_GELU, bias=bias, out_bf16=out, out2_bf16=u)
        assert rel_err(u, ref) < 1e-2 and rel_err(out, F.gelu(ref)) < 1e-2
    # and how far fp8 operands are from the fp32 product itself (the precision cost of configs[4], reported not bounded tightly)
    full = A @ W.t() + bias
    print(f"fp8 ({M},{N},{K}): rel err vs fp32 operands {rel_err(ref, full):.4f}")
    assert rel_err(ref, full) < 0.08


def _mx_quant(x):
    """Host-side (torch) MX quantiser: one E8M0 scale per (row, 32 consecutive columns), 2^ceil(log2(amax / 448)); e4m3 codes by
    torch's own round-to-nearest-even conversion.  -> (codes uint8 [M, K], scale bytes uint8 [M, K / 32], dequantised fp32)."""
    M, K = x.shape
    xb = x.view(M, K // 32, 32)
    amax = xb.abs().amax(-1)
    e = torch.ceil(torch.log2(amax.clamp_min(2.0 ** -120) / 448.0)).clamp(-127, 127)
    scale = torch.exp2(e)
    q = (xb / scale[..., None]).to(torch.float8_e4m3fn)
    deq = (q.float() * scale[..., None]).view(M, K)
    return q.view(M, K).view(torch.uint8).contiguous(), (e + 127).to(torch.uint8).contiguous(), deq


@pytest.mark.parametrize("M,N,K", [(11840, 768, 2304), (23680, 768, 2304), (1200, 192, 128), (11849, 768, 768), (5920, 2304, 768)])
def test_gemm_fp8_mx_block_scaled_A(L, M, N, K):
    """feddat_gemm_fp8mx_nt: A with true MX block scales (E8M0 per (row, 32 k)) applied by the block-scaled MFMA itself.  Rows whose
    32-blocks differ in magnitude by many binades (what per-row scaling cannot represent) against the fp32 product of the
    dequantised operands: only accumulation order + the bf16 output rounding differ."""
    g = torch.Generator().manual_seed(M + K)
    mag = torch.exp2(torch.randint(-12, 4, (M, K // 32, 1), generator=g).float())          # block magnitudes over 16 binades
    A = (torch.randn(M, K // 32, 32, generator=g) * mag).view(M, K).to(DEV)
    A[5, 64:96] = 0.0                                                                       # an all-zero block
    W = (torch.randn(N, K, generator=g) * 0.05).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV) * 0.01
    A8, amx, Adeq = _mx_quant(A)
    assert (Adeq - A).abs().max() <= float(A.abs().max()) / 8 and float((Adeq - A).abs().mean() / A.abs().mean()) < 0.04
    W8, sw = torch.empty(N, K, dtype=torch.uint8, device=DEV), torch.empty(N, device=DEV)
    L.quant_rows_fp8(W, W8, sw)
    ref = Adeq @ _fp8_deq(W8, sw).t() + bias
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    L.gemm_fp8mx_nt(A8, amx, W8, sw, bias=bias, out_bf16=out)
    assert torch.isfinite(out.float()).all()
    err = (out.float() - ref).abs()
    tol = 8e-3 * ref.abs() + 2e-3 * float(ref.abs().mean())            # bf16 output rounding + accumulation order
    assert bool((err <= tol).all()), (float(err.max()), float(ref.abs().max()), int((err > tol).sum()))


@pytest.mark.parametrize("B,S,heads,masked", [(4, 185, 12, False), (3, 90, 12, True), (64, 185, 12, False)])
def test_attention_bwd_mx_fp8_output(L, B, S, heads, masked):
    """feddat_attn_bwd_fp8mx: the same backward as feddat_attn_bwd with dq | dk | dv written as e4m3 + one E8M0 scale per (row, 32
    columns).  Dequantised it must equal the 16-bit dqkv of the plain kernel up to the e4m3 rounding of each value (3 mantissa
    bits: 1/16 relative, half a subnormal step of its block at the bottom); every scale is the smallest power of two that
    brings its block's maximum under 448."""
    g = torch.Generator().manual_seed(S + B)
    H = heads * 64
    qkv = bf(torch.randn(B * S, 3 * H, generator=g)).to(DEV)
    mask = None
    if masked:
        mask = torch.ones(B, S, dtype=torch.uint8)
        for b in range(B):
            mask[b, 20 + 3 * b: 20 + 3 * b + 7] = 0
        mask = mask.to(DEV)
    ctx = torch.empty(B * S, H, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B, heads, S, device=DEV)
    L.attn_fwd(qkv, ctx, lse, B, S, heads, key_mask=mask)
    dctx = bf(torch.randn(B * S, H, generator=g) * 1e-3).to(DEV)
    ref = torch.empty(B * S, 3 * H, dtype=torch.bfloat16, device=DEV)
    L.attn_bwd(qkv, ctx, lse, dctx, ref, B, S, heads, key_mask=mask)
    dq8 = torch.full((B * S, 3 * H), 0x7F, dtype=torch.uint8, device=DEV)
    sc = torch.zeros(B * S, 3 * H // 32, dtype=torch.uint8, device=DEV)
    L.attn_bwd_fp8mx(qkv, ctx, lse, dctx, dq8, sc, B, S, heads, key_mask=mask)
    scale = torch.exp2(sc.float() - 127.0)
    deq = (dq8.view(torch.float8_e4m3fn).float().view(B * S, -1, 32) * scale[..., None]).view(B * S, 3 * H)
    r32 = ref.float()
    amax = r32.view(B * S, -1, 32).abs().amax(-1)
    assert torch.isfinite(deq).all()
    tol = r32.abs() / 16 + (amax * 1e-5)[..., None].expand(-1, -1, 32).reshape(B * S, 3 * H) + 1e-30
    assert bool(((deq - r32).abs() <= tol).all()), float(((deq - r32).abs() / tol).max())
    nz = amax > 0
    assert bool((scale[nz] * 448.0 >= amax[nz] * 0.999).all()) and bool((scale[nz] * 448.0 < amax[nz] * 2.001).all())
    # ... and it is the operand feddat_gemm_fp8mx_nt takes: QKV^T of the quantised gradient against the 16-bit product
    W = (torch.randn(768, 3 * H, generator=g) * 0.05).to(DEV)
    if B * S >= 1024 and 3 * H % 128 == 0:
        W8, sw = torch.empty(768, 3 * H, dtype=torch.uint8, device=DEV), torch.empty(768, device=DEV)
        L.quant_rows_fp8(W, W8, sw)
        out = torch.empty(B * S, 768, dtype=torch.bfloat16, device=DEV)
        L.gemm_fp8mx_nt(dq8, sc, W8, sw, out_bf16=out)
        full = r32 @ W.t()
        assert rel_err(out, deq @ _fp8_deq(W8, sw).t()) < 1e-2
        print(f"QKV^T on MX e4m3 dqkv vs the 16-bit operands: rel err {rel_err(out, full):.4f}")
        assert rel_err(out, full) < 0.08


@pytest.mark.parametrize("R,V,ldl,with_teacher", [(96, 30522, 30592, True), (7, 1001, 1024, True), (5, 3072, 3072, False)])
def test_lm_loss_fwd_bwd_vs_torch(L, R, V, ldl, with_teacher):
    """feddat_lm_loss_fwd_bwd against autograd on the reference's formula (albef_model.py:142-143: per-row weighted CE with
    ignore_index -100; task_trainer.py:506-516: T^2 * KL(softmax(t / T) || softmax(l / T)), batchmean folded into kl_scale;
    L = (ce + kl) / 2): V not a multiple of 4 (the vocabulary's own 30 522), padded row stride, labels -100, per-row KL
    factors.  Loss terms 1e-5 relative; dlogits (stored in bf16) 2^-8 relative + 1e-9."""
    g = torch.Generator().manual_seed(R + V)
    lg = torch.zeros(R, ldl)
    lg[:, :V] = torch.randn(R, V, generator=g) * 3
    tc = torch.zeros(R, ldl)
    tc[:, :V] = torch.randn(R, V, generator=g) * 3
    labels = torch.randint(0, V, (R,), generator=g)
    labels[::3] = -100
    labels[1] = V - 1                                   # a label in the scalar tail columns
    rw = torch.rand(R, generator=g) + 0.1
    rk = torch.ones(R)
    rk[2] = 0.0
    rk[3] = 1.5
    T, ks = 3.0, 9.0 / R
    l32 = lg[:, :V].clone().requires_grad_(True)
    logp = F.log_softmax(l32, -1)
    ce_rows = torch.where(labels >= 0, -logp.gather(1, labels.clamp(min=0)[:, None])[:, 0] * rw, torch.zeros(R))
    ce = ce_rows.sum()
    if with_teacher:
        q = F.softmax(tc[:, :V] / T, -1)
        kl_rows = (q * (torch.log(q) - F.log_softmax(l32 / T, -1))).sum(-1) * rk
        kl = ks * kl_rows.sum()
    else:
        kl = torch.zeros(())
    (0.5 * (ce + kl)).backward()
    dl = torch.full((R, ldl), 7.0, dtype=torch.bfloat16, device=DEV)
    sc = torch.zeros(4 + 2 * R, device=DEV)
    L.lm_loss_fwd_bwd(lg.to(DEV), tc.to(DEV) if with_teacher else None, labels.to(DEV), rw.to(DEV), V, T,
                      ks if with_teacher else 0.0, dl, sc, row_kl=rk.to(DEV))
    sc = sc.cpu()
    assert abs(float(sc[0]) - float(ce)) <= 1e-5 * abs(float(ce)) + 1e-6
    assert abs(float(sc[1]) - float(kl)) <= 2e-5 * abs(float(kl)) + 1e-6
    assert abs(float(sc[2]) - 0.5 * float(ce + kl)) <= 2e-5 * abs(float(ce + kl)) + 1e-6
    got = dl.float().cpu()
    assert torch.equal(got[:, V:], torch.zeros(R, ldl - V))
    err = (got[:, :V] - l32.grad).abs()
    assert bool((err <= 2.0 ** -8 * l32.grad.abs() + 1e-9).all()), float(err.max())
