"""The two-wave-group adapter kernels (csrc/adapter.hip: adapter_fwd_g2_kernel / adapter_bwd_g2_kernel) against the four-wave
kernels they replace (debug flag 2048 selects those): bit-identical on every output, in both operand builds.

The new kernels split the four-wave kernels' work over two groups of four waves (gated segment: by adapter; single-adapter
segment: by r-tile and column tile) and promise the same operations in the same order for every element, fused multiply-adds
included.  Each case runs both forms in one process on the same inputs into NaN-filled buffers that carry padding rows in front
of and behind the segments, and compares the bit patterns of the WHOLE buffers: a differing element, a missing store and a store
outside the kernel's rows all show up.  What the values should be is test_adapter_kernels_gpu.py's subject (float64 bounds).

Shapes: segments of 1, 15, 16, 17, 33 and 48 rows (one row, a ragged tile, one full tile, a full and a ragged tile, two full and
one ragged, three full) as gated + single two-segment descriptors -- which with n rows per segment is also the 2B token-0 form of
the top layer at B = n --, in the first-layer form (the second segment reads the first one's x rows, x_row_delta = -n), and as
single-segment descriptors of each kind.  These grids have one tile per block; the step's own shape (2 x 185 x 32 rows: 740 tiles
on one block per compute unit, i.e. two to three tiles per block with a ragged last round, both tile buffers and the prefetch of
tile t + 2 in use) is run once per build on top.
Forward: with and without the fused LayerNorm, with and without z_save.  Backward (from the saved z): dx = None (layer 0), dx with
and without its 16-bit copy, train_slot -1, 0 and (gated) 1."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMTS = ("bf16", "f16")
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
H, RB = 768, 48
PAD = 3                      # NaN rows in front of and behind the segments
FOUR_WAVE = 1 << 11          # feddat_set_debug_flags: the four-wave weight-stationary kernels
LN_EPS = 1e-12
GATED = ((0, 0.5), (2, 0.5))
AD1 = ((1, 1.0),)
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import lib
    lib.load()
    with lib.operands("f16"):
        lib.load()
    return lib


@pytest.fixture(scope="module")
def params(L):
    """Three adapters per build (adapter_0, adapter_1, adapter_2 of one layer), packed by the build's own adapter_pack."""
    out = {}
    for fmt in FMTS:
        gen = torch.Generator().manual_seed(23)
        par = []
        for _ in range(3):
            wd = (torch.randn(RB, H, generator=gen) * 0.05).to(DEV)
            wu = (torch.randn(H, RB, generator=gen) * 0.05).to(DEV)
            w = [torch.empty(RB, H, dtype=DT[fmt], device=DEV), torch.empty(H, RB, dtype=DT[fmt], device=DEV),
                 torch.empty(H, RB, dtype=DT[fmt], device=DEV), torch.empty(RB, H, dtype=DT[fmt], device=DEV)]
            with L.operands(fmt):
                L.adapter_pack(wd, wu, *w)
            par.append(dict(wd=w[0], wdT=w[1], wu=w[2], wuT=w[3], bd=(torch.randn(RB, generator=gen) * 0.1).to(DEV),
                            bu=(torch.randn(H, generator=gen) * 0.1).to(DEV)))
        out[fmt] = par
    torch.cuda.synchronize()
    return out


def _forms(n):
    """(name, segments) with rows counted from PAD; a segment is (row_begin, row_end, adapters, x_row_delta)."""
    a, b, c = PAD, PAD + n, PAD + 2 * n
    return [("gated+single", [(a, b, GATED, 0), (b, c, AD1, 0)]),        # inner layers; the 2B token-0 rows at B = n
            ("first-layer", [(a, b, GATED, 0), (b, c, AD1, -n)]),
            ("gated", [(a, b, GATED, 0)]),
            ("single", [(a, b, AD1, 0)])]


SMALL = [(f"{n}rows-{name}", segs) for n in (1, 15, 16, 17, 33, 48) for name, segs in _forms(n)]
STEP = [(f"step-{name}", segs) for name, segs in _forms(185 * 32)[:2]]
CASES = SMALL + STEP


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b, what):
    if not torch.equal(_bits(a), _bits(b)):
        bad = (_bits(a) != _bits(b)).nonzero()
        first = [(tuple(i.tolist()), float(a[tuple(i)]), float(b[tuple(i)])) for i in bad[:6]]
        raise AssertionError((what, "two-group kernel != four-wave kernel", len(bad), "elements differ; (index, new, old):", first))


def _segs(L, par, segs, train):
    """train: train_slot per segment."""
    return L.make_segs([dict(row_begin=rb, row_end=re, train_slot=ts, x_row_delta=xd,
                             adapters=[dict(par[i], scale=sc) for i, sc in ads])
                        for (rb, re, ads, xd), ts in zip(segs, train)])


def _both(L, fn):
    """fn() under the four-wave kernels and under the default (two-group) kernels; fn returns its freshly NaN-filled outputs."""
    L.set_debug_flags(FOUR_WAVE)
    try:
        ref = fn()
        torch.cuda.synchronize()
    finally:
        L.set_debug_flags(0)
    got = fn()
    torch.cuda.synchronize()
    return ref, got


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("fmt", FMTS)
def test_two_groups_bit_identical_with_four_waves(L, params, fmt, case):
    name, segs = case
    par = params[fmt]
    T = max(re for _, re, _, _ in segs) + PAD
    inside = torch.zeros(T, dtype=torch.bool, device=DEV)
    for rb, re, _, _ in segs:
        inside[rb:re] = True
    gen = torch.Generator(device=DEV).manual_seed(sum(map(ord, name)))
    x = torch.randn(T, H, generator=gen, device=DEV)
    dy = torch.randn(T, H, generator=gen, device=DEV)
    gamma = 1 + 0.1 * torch.randn(H, generator=gen, device=DEV)
    beta = 0.1 * torch.randn(H, generator=gen, device=DEV)

    def nan(*shape, dtype=torch.float32):
        return torch.full(shape, NAN, dtype=dtype, device=DEV)

    def untouched_outside(o, what):
        for k, t in o.items():
            assert bool(torch.isnan(t[~inside].float()).all()), (what, k, "a store outside the segments")

    with L.operands(fmt):
        fseg = _segs(L, par, segs, [-1] * len(segs))
        zsave = None
        # ---- forward: with / without z_save, with / without the fused LayerNorm
        for with_z in (True, False):
            def fwd():
                o = dict(out=nan(T, H))
                if with_z:
                    o["z"] = nan(T, 2, RB)
                L.adapter_fwd(x, o["out"], fseg, T, z_save=o.get("z"))
                return o

            def fwd_ln():
                o = dict(out=nan(T, H), y16=nan(T, H, dtype=DT[fmt]), st=nan(T, 2))
                if with_z:
                    o["z"] = nan(T, 2, RB)
                L.adapter_fwd_ln(x, o["out"], fseg, T, gamma, beta, LN_EPS, o["y16"], o["st"], z_save=o.get("z"))
                return o

            for tag, fn in (("fwd", fwd), ("fwd_ln", fwd_ln)):
                ref, got = _both(L, fn)
                what = f"{fmt} {name} {tag} z_save={with_z}"
                for k in ref:
                    _same(got[k], ref[k], (what, k))
                untouched_outside(got, what)
                assert not bool(torch.isnan(got["out"][inside]).any()), (what, "a row of the segments was not stored")
                if with_z:
                    zsave = ref["z"]
        # ---- backward from the saved z: dx = None / dx / dx + 16-bit copy; train_slot -1, 0 and (gated) 1
        trains = [[-1] * len(segs), [0] * len(segs)]
        if len(segs[0][2]) == 2:
            trains.append([1] + [0] * (len(segs) - 1))
        for train in trains:
            bseg = _segs(L, par, segs, train)
            for form in ("nodx", "dx", "dx+16"):
                if form == "nodx" and max(train) < 0:
                    continue              # nothing to write: the ABI refuses dx = None without z_out

                def bwd():
                    o = dict(z=nan(T, RB), dz=nan(T, RB))
                    if form != "nodx":
                        o["dx"] = nan(T, H)
                    if form == "dx+16":
                        o["dx16"] = nan(T, H, dtype=DT[fmt])
                    L.adapter_bwd(None, dy, o.get("dx"), bseg, T, dx_bf16=o.get("dx16"), z_out=o["z"], dz_out=o["dz"],
                                  z_saved=zsave)
                    return o

                ref, got = _both(L, bwd)
                what = f"{fmt} {name} bwd {form} train_slot={train}"
                for k in ref:
                    _same(got[k], ref[k], (what, k))
                untouched_outside(got, what)
                if "dx" in got:
                    assert not bool(torch.isnan(got["dx"][inside]).any()), (what, "a row of the segments was not stored")
