"""The vector-gradient kernels (csrc/vector_grad.hip) element by element against float64, in both operand builds.

Inputs are drawn in the format the kernel reads (16-bit operands of the build, or fp32), so every term of every sum is known
exactly and the float64 restatement differs from the kernel by the kernel's own fp32 roundings only.

Bound, per column, derived (u = 2^-24; round-to-nearest fp32 adds, |fl(a + b) - (a + b)| <= u |a + b|, and every partial sum is
bounded by sum|terms|):
  a column of `rows` terms is added up as  8 sequential adds per row lane (rows r, r + 8, ... of a 64-row slab; the first one
  adds to 0 and is exact), 7 adds over the 8 row lanes in LDS, ceil(slabs / 4) sequential adds per slab chain (first exact) and
  2 adds to join the four chains, slabs = ceil(rows / 64):
      D(rows) = 7 + 7 + (ceil(slabs / 4) - 1) + 2  roundings on any path   ->   |err| <= D u sum|terms|   (to first order; the
      second-order terms are below D^2 u^2, covered by the factor 1 + 2^-10)
  (D = 39 at 5 920 rows, 62 at 11 840: far below the naive rows * 2^-24 * sum|terms| of a sequential sum.)
  LayerNorm dgamma: each term dy * ((x - mean) * rstd) carries up to 3 more roundings (subtract, two products; fewer where
  the compiler contracts into an fma): D + 3.  The reduce kernel's unscale factor is a power of two (exact).
Each case prints its worst measured ratio to the bound (run with -s)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMTS = ("bf16", "f16")
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
U32 = 2.0 ** -24
SLAB = 64


def depth(rows):
    slabs = -(-rows // SLAB)
    return 7 + 7 + (-(-slabs // 4) - 1) + 2


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import lib
    lib.load()
    with lib.operands("f16"):
        lib.load()
    return lib


def _matrix(rows, N, stride, dtype, seed, scale=1.0):
    """[rows, N] view (row stride `stride`) of values exactly representable in `dtype`, magnitudes over several binades; the
    padding columns hold a sentinel that would wreck any sum that touched them."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(rows, stride, generator=g) * torch.exp2(torch.randint(-6, 3, (rows, 1), generator=g).float()) * scale
    base[:, N:] = 3.0e4
    buf = base.to(dtype).to(DEV)
    return buf[:, :N]


def _reduce(L, parts, grads, unscale=1.0, unscale_dev=None, flag=None, flags=0):
    jobs = [(p, p.numel() // g.numel(), g, flags) for p, g in zip(parts, grads)]
    table, n, max_n = L.make_vgrad_jobs(jobs, DEV)
    L.vector_grad_reduce(table, n, max_n, unscale, unscale_dev, flag)
    torch.cuda.synchronize()
    return table


CASES = [(5920, 768, 0, False), (5920, 2304, 0, False), (5920, 3072, 0, False), (11840, 768, 0, False), (11840, 2304, 0, False),
         (11840, 3072, 0, False), (5917, 768, 0, False), (5920, 768, 64, False), (5920, 768, 0, True), (1000, 3072, 8, True),
         (32, 768, 185 * 768 - 768, False), (7, 2304, 0, False)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("f32_in", [False, True])
@pytest.mark.parametrize("rows,N,pad,masked", CASES)
def test_colsum_against_float64(L, fmt, f32_in, rows, N, pad, masked):
    with L.operands(fmt):
        x = _matrix(rows, N, N + pad, torch.float32 if f32_in else DT[fmt], rows + N + pad)
        mask = None
        if masked:
            mask = (torch.rand(rows, generator=torch.Generator().manual_seed(rows)) < 0.6).to(torch.uint8).to(DEV)
        elems = L.vector_grad_workspace_elems(rows, N)
        assert elems == -(-rows // SLAB) * N
        part = torch.full((elems,), float("nan"), device=DEV)
        slabs = L.colsum_partial(x, part, row_mask=mask)
        grad = torch.full((N + 8,), -31.0, device=DEV)
        _reduce(L, [part], [grad[:N]])
        part2 = torch.full((elems,), float("nan"), device=DEV)
        L.colsum_partial(x, part2, row_mask=mask)
        grad2 = torch.full((N,), -31.0, device=DEV)
        _reduce(L, [part2], [grad2])
    assert slabs == -(-rows // SLAB)
    assert torch.equal(part, part2) and torch.equal(grad[:N], grad2), "two launches differ"
    assert bool((grad[N:] == -31.0).all()), "wrote past the vector"
    xd = x.double()
    if masked:
        xd = xd * mask.double()[:, None]
    ref, mag = xd.sum(0), xd.abs().sum(0)
    bound = depth(rows) * U32 * mag * (1 + 2.0 ** -10)
    err = (grad[:N].double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"colsum {fmt} {'f32' if f32_in else '16b'} rows {rows} N {N} pad {pad} masked {masked}: worst err / bound {ratio:.3f}"
          f" (D = {depth(rows)})")
    assert bool((err <= bound).all()), ratio


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("f32_dy", [False, True])
@pytest.mark.parametrize("rows,N,xpad", [(5920, 768, 0), (11840, 768, 0), (5920, 2304, 0), (5920, 3072, 0), (5917, 768, 0),
                                         (5920, 768, 32), (32, 768, 0)])
def test_ln_param_grads_against_float64(L, fmt, f32_dy, rows, N, xpad):
    with L.operands(fmt):
        dy = _matrix(rows, N, N + (8 if xpad else 0), torch.float32 if f32_dy else DT[fmt], 3 * rows + N, scale=0.01)
        x = _matrix(rows, N, N + xpad, torch.float32, 5 * rows + N)
        g = torch.Generator().manual_seed(rows)
        stats = torch.stack([0.1 * torch.randn(rows, generator=g), 0.5 + torch.rand(rows, generator=g)], 1).contiguous().to(DEV)
        elems = L.vector_grad_workspace_elems(rows, N)
        outs = []
        for _ in range(2):
            pb, pg = torch.full((elems,), float("nan"), device=DEV), torch.full((elems,), float("nan"), device=DEV)
            L.ln_param_grad_partial(dy, x, stats, pb, pg)
            grads = torch.full((2, N), -31.0, device=DEV)
            _reduce(L, [pb, pg], [grads[0], grads[1]])
            outs.append((pb, pg, grads))
        # beta alone (optimizer_mode bias): x and stats are not read, and the result is the column sum, bit for bit
        pb1 = torch.full((elems,), float("nan"), device=DEV)
        L.ln_param_grad_partial(dy, None, None, pb1, None)
        pc = torch.full((elems,), float("nan"), device=DEV)
        L.colsum_partial(dy, pc)
        torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])), "two launches differ"
    assert torch.equal(pb1, pc) and torch.equal(pb1, outs[0][0])
    dbeta, dgamma = outs[0][2][0].double(), outs[0][2][1].double()
    dyd = dy.double()
    xh = (x.double() - stats[:, 0:1].double()) * stats[:, 1:2].double()
    for name, got, terms, extra in (("dbeta", dbeta, dyd, 0), ("dgamma", dgamma, dyd * xh, 3)):
        ref, mag = terms.sum(0), terms.abs().sum(0)
        bound = (depth(rows) + extra) * U32 * mag * (1 + 2.0 ** -10)
        err = (got - ref).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        print(f"ln {name} {fmt} dy {'f32' if f32_dy else '16b'} rows {rows} N {N} xpad {xpad}: worst err / bound {ratio:.3f}")
        assert bool((err <= bound).all()), (name, ratio)


@pytest.mark.parametrize("fmt", FMTS)
def test_reduce_unscales_by_the_device_scale_and_flags_non_finite(L, fmt):
    with L.operands(fmt):
        N, slabs = 768, 93
        g = torch.Generator().manual_seed(7)
        pa, pb = torch.randn(slabs * N, generator=g).to(DEV), torch.randn(5 * 3072, generator=g).to(DEV)
        ga, gb, gc = torch.zeros(N, device=DEV), torch.zeros(3072, device=DEV), torch.zeros(N, device=DEV)
        inv = torch.tensor([2.0 ** -14], device=DEV)
        flag = torch.zeros(2, dtype=torch.int32, device=DEV)
        jobs = [(pa, slabs, ga, 0), (pb, 5, gb, 0), (pa, slabs, gc, L.VGRAD_UNSCALED)]
        table, n, max_n = L.make_vgrad_jobs(jobs, DEV)
        L.vector_grad_reduce(table, n, max_n, 1.0, inv, flag[0:1])
        torch.cuda.synchronize()
        assert flag.tolist() == [0, 0]
        ra = pa.view(slabs, N).double().sum(0)
        assert float((gc.double() - ra).abs().max()) <= depth(slabs * 64) * U32 * float(pa.view(slabs, N).abs().sum(0).max())
        assert torch.equal(ga, gc * 2.0 ** -14)                   # a power of two: exact, and taken from the device
        assert float((gb.double() - pb.view(5, 3072).double().sum(0) * 2.0 ** -14).abs().max()) < 1e-9
        inv.fill_(0.5)                                            # the device value is read at run time, not at table-build time
        L.vector_grad_reduce(table, n, max_n, 1.0, inv, flag[0:1])
        torch.cuda.synchronize()
        assert torch.equal(ga, gc * 0.5) and flag.tolist() == [0, 0]
        L.vector_grad_reduce(table, n, max_n, 0.25, None, None)   # static scale: the host factor alone, no flag
        torch.cuda.synchronize()
        assert torch.equal(ga, gc * 0.25)
        for bad in (float("inf"), float("nan")):
            flag.zero_()
            keep = float(pb[3 * 3072 + 17])
            pb[3 * 3072 + 17] = bad
            L.vector_grad_reduce(table, n, max_n, 1.0, inv, flag[0:1])
            torch.cuda.synchronize()
            assert flag.tolist() == [1, 0] and not math.isfinite(float(gb[17]))
            pb[3 * 3072 + 17] = keep
        L.vector_grad_reduce(table, n, max_n, 1.0, inv, flag[0:1])  # the flag is OR-ed into, never cleared here
        torch.cuda.synchronize()
        assert flag.tolist() == [1, 0] and bool(torch.isfinite(gb).all())
        # a finite sum that overflows only through the unscale factor is an overflow too
        flag.zero_()
        inv.fill_(2.0 ** 127)
        L.vector_grad_reduce(table, n, max_n, 1.0, inv, flag[0:1])
        torch.cuda.synchronize()
        assert flag.tolist() == [1, 0] and bool(torch.isfinite(gc).all())


def test_wrapper_refuses_the_other_builds_operands(L):
    with L.operands("bf16"):
        with pytest.raises(L.FeddatHipError):
            L.colsum_partial(torch.zeros(64, 768, dtype=torch.float16, device=DEV), torch.zeros(768, device=DEV))
    with L.operands("f16"):
        with pytest.raises(L.FeddatHipError):      # N % 8 != 0 -> EINVAL
            L.colsum_partial(torch.zeros(64, 772, dtype=torch.float16, device=DEV), torch.zeros(772, device=DEV))
