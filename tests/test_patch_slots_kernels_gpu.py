"""The two patch-slot kernels (include/feddat_hip.h, "PATCH SLOTS") one by one, at the smallest shapes at which they can go wrong:
a 96 x 160 frame (3 x 5 cells), P = 32, B = 3, Lt = 3, H = 64, a 12 x 12 position table, key masks written once and twice, both
operand builds.

feddat_image_embed_assemble_slots against feddat_image_embed_assemble_masked, BIT for bit: the grid kernel is given the same
projection rows scattered to the grid cells that vilt_spec.patch_slot_plan maps the slots to; every valid slot row, the CLS rows
and the key masks must be equal, empty slots finite with key mask 0.  feddat_im2col_patches_slots against feddat_im2col_patches'
rows at the mapped cells.  Every output buffer sits between guard regions that must come back untouched, the overflow case (a
full 3 x 5 sample in 6 slots) included."""
import pytest
import torch

from feddat_amd import vilt_spec

pytestmark = pytest.mark.gpu
DEV = "cuda"
GH, GW, P, B, LT, H, G0 = 3, 5, 32, 3, 3, 64, 12
GUARD = 64
# (max_patches, valid rectangle vh x vw per sample)
CASES = {"full_1x1_column": (15, [(3, 5), (1, 1), (3, 1)]),
         "row_2x3_full": (15, [(1, 5), (2, 3), (3, 5)]),
         "count_equals_slots": (6, [(2, 3), (1, 5), (1, 1)]),
         "overflow": (6, [(3, 5), (2, 3), (3, 1)])}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def L():
    from feddat_amd import lib
    lib.load()
    return lib


def _patch_mask(rects, hole=False):
    pm = torch.zeros(B, GH, GW, dtype=torch.int64)
    for b, (vh, vw) in enumerate(rects):
        pm[b, :vh, :vw] = 1
        if hole and vh >= 2 and vw >= 3:      # a masked patch INSIDE the rectangle (column 0 and row 0 stay whole)
            pm[b, 1, 2] = 0
    return pm


def _guarded(shape, dtype, fill):
    """A tensor of `shape` in the middle of a buffer whose first and last GUARD elements hold `fill`."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf, fill):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool((g == fill).all())


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("nrep", [1, 2])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_assemble_slots_is_the_grid_kernel_at_the_mapped_cells(L, fmt, nrep, case):
    mp, rects = CASES[case]
    pm = _patch_mask(rects, hole=True)
    cells, counts, over = vilt_spec.patch_slot_plan(pm, mp)
    assert bool(over.any()) == (case == "overflow")
    gen = torch.Generator().manual_seed(17)
    proj_slots = torch.randn(B * mp, H, generator=gen)
    proj_grid = torch.randn(B * GH * GW, H, generator=gen)
    for b in range(B):
        for j in range(mp):
            if cells[b, j] >= 0:
                proj_grid[b * GH * GW + int(cells[b, j])] = proj_slots[b * mp + j]
    cls, pos0, mod1 = (torch.randn(H, generator=gen).to(DEV) for _ in range(3))
    pos_grid = torch.randn(G0 * G0, H, generator=gen).to(DEV)
    am = torch.ones(B, LT, dtype=torch.int64)
    am[1, 2:] = 0
    pm_d, am_d = pm.to(DEV), am.to(DEV)
    S, Sg = LT + 1 + mp, LT + 1 + GH * GW
    with L.operands(fmt):
        h_g = torch.full((B, Sg, H), -7.0, device=DEV)
        km_g = torch.full((nrep * B, Sg), 9, dtype=torch.uint8, device=DEV)
        L.image_embed_assemble_masked(proj_grid.to(DEV), cls, pos0, pos_grid, pm_d, am_d, mod1, h_g, km_g, B, LT, GH, GW, G0, H,
                                      nrep=nrep)
        hbuf, h_s = _guarded((B, S, H), torch.float32, -7.0)
        kbuf, km_s = _guarded((nrep * B, S), torch.uint8, 9)
        fbuf, flag = _guarded((1,), torch.int32, 0)
        L.image_embed_assemble_slots(proj_slots.to(DEV), cls, pos0, pos_grid, pm_d, am_d, mod1, h_s, km_s, flag, B, LT, GH, GW,
                                     mp, G0, H, nrep=nrep)
        torch.cuda.synchronize()
    assert _guards_intact(hbuf, -7.0) and _guards_intact(kbuf, 9) and _guards_intact(fbuf, 0)
    assert int(flag.item()) == int(case == "overflow")
    h_s, h_g, km_s, km_g = h_s.cpu(), h_g.cpu(), km_s.cpu(), km_g.cpu()
    assert bool((h_s[:, :LT] == -7.0).all())                                   # the text rows belong to feddat_text_embed
    assert torch.equal(h_s[:, LT], h_g[:, LT])                                 # CLS rows
    assert torch.equal(km_s[:, :LT + 1], km_g[:, :LT + 1]) and bool((km_s[:, LT] == 1).all())
    checked = 0
    for b in range(B):
        for j in range(mp):
            c = int(cells[b, j])
            row = h_s[b, LT + 1 + j]
            if c >= 0:
                assert torch.equal(row, h_g[b, LT + 1 + c]), (b, j, c)
                for r in range(nrep):
                    assert km_s[b + r * B, LT + 1 + j] == km_g[b + r * B, LT + 1 + c] == pm[b].flatten()[c], (b, j, r)
                checked += 1
            else:
                # an empty slot: projection + modality, no position value, masked as a key
                assert bool(torch.isfinite(row).all()) and torch.equal(row, (proj_slots[b * mp + j] + 0.0) + mod1.cpu())
                assert all(km_s[b + r * B, LT + 1 + j] == 0 for r in range(nrep))
    assert checked == int(counts.clamp(max=mp).sum())
    if case == "row_2x3_full":      # the hole inside sample 2's rectangle is a masked key in its slot (cell 1 * 5 + 2, slot 7)
        assert km_s[2, LT + 1 + 7] == 0 and km_s[2, LT + 1 + 6] == 1
    if case == "overflow":          # the full sample keeps its first 6 cells: row 0 and the first cell of row 1
        assert cells[0].tolist() == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("n", [3, 2])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_gather_slots_is_im2col_at_the_mapped_cells(L, fmt, n, case):
    mp, rects = CASES[case]
    pm = _patch_mask(rects)
    if n < B:
        pm[n:] = pm[:B - n]      # the replicas of a short batch carry their source's mask (feddat_vilt_pad_batch)
    cells, _, _ = vilt_spec.patch_slot_plan(pm, mp)
    px = torch.randn(n, 3, GH * P, GW * P, generator=torch.Generator().manual_seed(23)).to(DEV)
    K = 3 * P * P
    with L.operands(fmt):
        dt = L.OPERAND_DTYPE[fmt]
        ref = torch.empty(n * GH * GW, K, dtype=dt, device=DEV)
        L.im2col_patches(px, ref, n, 3, GH * P, GW * P, P)
        buf, out = _guarded((B * mp, K), dt, 3.0)
        L.im2col_patches_slots(px, pm.to(DEV), out, n, B, 3, GH * P, GW * P, P, mp)
        torch.cuda.synchronize()
    assert _guards_intact(buf, 3.0)
    out, ref = out.cpu().view(torch.int16), ref.cpu().view(torch.int16)
    for b in range(B):
        for j in range(mp):
            c = int(cells[b, j])
            if c >= 0:
                assert torch.equal(out[b * mp + j], ref[(b % n) * GH * GW + c]), (b, j, c)
            else:
                assert not out[b * mp + j].any(), (b, j)
    if n == 2:
        assert torch.equal(out[2 * mp:3 * mp], out[:mp])
