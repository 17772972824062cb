"""The streaming kernels of the step -- LayerNorm forward / backward, the adapter weight-gradient reduction, the multi-group
AdamW, and the embedding / packing kernels (im2col, text_embed, image_embed_assemble_masked, adapter_pack_strided) -- BIT for bit
against what the parent's kernels produced, and against float64 / a torch construction.

tests/golden/stream_kernels.json holds sha256 digests of every output of every case below, written by
tools/make_stream_golden.py from the libraries of the commit BEFORE the kernels were restructured (one wave per row LayerNorm,
element-per-thread reduction, per-thread segment search in AdamW).  The inputs are seeded; a digest of the inputs is stored too,
so a generator that draws other numbers is reported as that and not as a kernel difference.  A digest is compared for equality:
zero differing bits, no case exempt.  What the digests cannot say -- that the numbers are RIGHT -- is checked next to them:
LayerNorm against float64 under the bounds of tests/test_ops_gpu.py (bf16 build) / tests/test_f16_kernels_gpu.py (fp16 build), the
reduction against the fp32 sum ((0 + P_0) + P_1) + ... done on the CPU (IEEE addition: exactly reproducible, so this one is bitwise
too), AdamW against a float64 AdamW under tests/test_lossscale_gpu.py's 2e-7.

LayerNorm rows (H = 768): 1, 4 (one block of the one-row kernel), 5, 9, 4 * grid + 3 and 12 * grid + 3, where grid is the persistent
kernels' block count on this device (LN_WALK_BLOCKS_PER_CU blocks per CU, read from layernorm.hip) and 4 * grid its wave count: at
4 * grid + 3 every wave has one row and three waves a second (one trip round the loop, a ragged last pass); at 12 * grid + 3 every
wave walks three rows and three waves a fourth, so the loop's back-edge (prefetch, copy, prefetch, copy) is taken at least twice
in every wave.  H = 1536 (the one-row kernels) with 5 rows.  x is always the token-0 view (x_stride = 5 H).

Embedding group (the smallest frames: B = 2, 64 x 96 pixels = 2 x 3 patches, 3 text tokens, 2 adapter layers): im2col against
unfold + .to(operand dtype); text_embed against float64 and the parent's digest (its LayerNorm sums have the kernel's own order);
image_embed_assemble_masked against its three separate launches, bit for bit, and the parent's digest (bilinear blend);
adapter_pack_strided against the parent's digest and, as a permutation, against the sorted .to(operand dtype) of its sources."""
import hashlib
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMTS = ("bf16", "f16")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_kernels.json")
with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "feddat_amd", "csrc", "layernorm.hip")) as _f:
    LN_WALK_BLOCKS_PER_CU = int(re.search(r"constexpr int LN_WALK_BLOCKS_PER_CU = (\d+);", _f.read()).group(1))
H_, R_, NBLK = 768, 48, 10           # adapter_wgrad.hip
RH = R_ * H_
PSTRIDE, GN = RH + R_ + H_, 2 * RH + R_ + H_


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
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


def digest(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()[:32]


def ln_grid():
    return LN_WALK_BLOCKS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count


def ln_shapes():
    return [(1, 768), (4, 768), (5, 768), (9, 768), (4 * ln_grid() + 3, 768), (5, 1536), (12 * ln_grid() + 3, 768)]


def _check(got, want, key, what):
    assert key in want, f"{key}: no such case in the fixture (regenerate it with tools/make_stream_golden.py on the parent commit)"
    assert got["inputs"] == want[key]["inputs"], f"{key}: the seeded INPUTS differ from the fixture's (another generator?)"
    bad = [k for k in want[key] if got.get(k) != want[key][k]]
    assert not bad and set(got) == set(want[key]), f"{key}: {what} differ from the replaced kernels' in {bad}"


# ------------------------------------------------------------------------------------------ LayerNorm
E_SPARSE = 5


def ln_case(L, fmt, rows, H, check=True):
    """Every output of every forward / backward form on one seeded input -> {name: digest}; float64 bounds asserted on the way."""
    op = L.OPERAND_DTYPE[fmt]
    g = torch.Generator().manual_seed(1000 + rows + H)
    xfull = (torch.randn(rows, 5 * H, generator=g) * 2 + 0.3).to(DEV)
    x = xfull[:, :H]                                        # the token-0 view: row stride 5 H
    gamma = (1 + 0.1 * torch.randn(H, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(H, generator=g)).to(DEV)
    dy = torch.randn(rows, H, generator=g).to(DEV)
    dres = torch.randn(rows, H, generator=g).to(DEV)
    nsp = (rows + E_SPARSE - 1) // E_SPARSE
    dres_c = torch.randn(nsp, H, generator=g).to(DEV)       # compact: row r / E of it belongs to rows r = 0, E, 2 E, ...
    dy16 = dy.to(op)
    eps = 1e-12 if H == 768 else 1e-5
    out = {"inputs": digest(torch.cat([xfull.flatten(), gamma, beta, dy.flatten(), dres.flatten(), dres_c.flatten()]))}
    tol16 = 1e-2 if fmt == "bf16" else 2.5e-3
    tol32_bwd = 5e-5 if fmt == "bf16" else 1.25e-5
    with L.operands(fmt):
        # forward: y16 + stats, y32 + stats
        y16, y32 = torch.zeros(rows, H, dtype=op, device=DEV), torch.zeros(rows, H, device=DEV)
        st_a, st_b = torch.zeros(rows, 2, device=DEV), torch.zeros(rows, 2, device=DEV)
        L.layernorm_fwd(x, gamma, beta, eps, rows, H, x_stride=5 * H, y_bf16=y16, stats=st_a)
        L.layernorm_fwd(x, gamma, beta, eps, rows, H, x_stride=5 * H, y_f32=y32, stats=st_b)
        torch.cuda.synchronize()
        out.update({"fwd.y16": digest(y16), "fwd.st16": digest(st_a), "fwd.y32": digest(y32), "fwd.st32": digest(st_b)})
        xr = x.double().requires_grad_(True)
        ref = F.layer_norm(xr, (H,), gamma.double(), beta.double(), eps)
        if check:
            e32 = float((y32.double() - ref).abs().max())
            e16 = float((y16.double() - ref).abs().max() / ref.abs().max())
            print(f"ln fwd {fmt} ({rows}, {H}): y32 max abs err {e32:.2e}, y16 max err / max {e16:.2e}")
            assert e32 < 2e-5 and e16 < tol16
            assert torch.equal(st_a, st_b) and torch.equal(y16, y32.to(op))
            mean, var = x.double().mean(1), x.double().var(1, unbiased=False)
            assert float((st_a[:, 0].double() - mean).abs().max()) < 1e-5
            assert float((st_a[:, 1].double() * (var + eps).sqrt() - 1).abs().max()) < 1e-5
        # backward: (16-bit dy -> out32), (16-bit dy -> out32 + out16), (fp32 dy -> out32)  x  (no dres, dres, compact dres)
        for dk, dyk, with16 in (("d16", dict(dy_bf16=dy16), False), ("d16o16", dict(dy_bf16=dy16), True),
                                ("d32", dict(dy_f32=dy), False)):
            (gx,) = torch.autograd.grad(ref, xr, (dy16 if "dy_bf16" in dyk else dy).double(), retain_graph=True)
            for rk, rkw in (("none", {}), ("dres", dict(dres=dres)), ("sparse", dict(dres=dres_c, dres_every=E_SPARSE))):
                o32 = torch.zeros(rows, H, device=DEV)
                o16 = torch.zeros(rows, H, dtype=op, device=DEV) if with16 else None
                L.layernorm_bwd_dx(x, st_a, gamma, rows, H, x_stride=5 * H, out_f32=o32, out_bf16=o16, **dyk, **rkw)
                torch.cuda.synchronize()
                out[f"bwd.{dk}.{rk}.o32"] = digest(o32)
                if with16:
                    out[f"bwd.{dk}.{rk}.o16"] = digest(o16)
                if check:
                    want = gx.clone()
                    if rk == "dres":
                        want += dres.double()
                    elif rk == "sparse":
                        want[::E_SPARSE] += dres_c.double()
                    e32 = float((o32.double() - want).abs().max())
                    assert e32 < tol32_bwd, (dk, rk, e32)
                    if with16:
                        assert torch.equal(o16, o32.to(op)), (dk, rk)
                        assert float((o16.double() - want).abs().max() / want.abs().max()) < tol16, (dk, rk)
        # the fp8 forms (5 rows): fixture only (their accuracy: tests/test_ops_gpu.py)
        if rows == 5 and H == 768:
            xc = x.contiguous()
            y8, sc = torch.zeros(rows, H, dtype=torch.uint8, device=DEV), torch.zeros(rows, device=DEV)
            y16b, st8 = torch.zeros(rows, H, dtype=op, device=DEV), torch.zeros(rows, 2, device=DEV)
            L.layernorm_fwd_fp8(x, gamma, beta, eps, rows, H, y8, sc, y_bf16=y16b, stats=st8, x_stride=5 * H)
            o8, osc, o32 = torch.zeros(rows, H, dtype=torch.uint8, device=DEV), torch.zeros(rows, device=DEV), torch.zeros(rows, H, device=DEV)
            L.layernorm_bwd_dx_fp8(xc, st_a, gamma, rows, H, o8, osc, dy_bf16=dy16, dres=dres, out_f32=o32)
            torch.cuda.synchronize()
            out.update({"fp8.fwd.y8": digest(y8), "fp8.fwd.scale": digest(sc), "fp8.fwd.y16": digest(y16b), "fp8.fwd.st": digest(st8),
                        "fp8.bwd.o8": digest(o8), "fp8.bwd.scale": digest(osc), "fp8.bwd.o32": digest(o32)})
            if check:
                assert torch.equal(y16b, y16) and torch.equal(st8, st_a)
                # the one-row kernel (the fp8 entry's) and the persistent one, against each other
                assert out["fp8.bwd.o32"] == out["bwd.d16.dres.o32"]
    return out


def ln_key(fmt, rows, H):
    return f"ln.{fmt}.{rows}x{H}"


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("which", range(7))
def test_layernorm_is_bit_identical_and_right(L, golden, fmt, which):
    rows, H = ln_shapes()[which]
    _check(ln_case(L, fmt, rows, H), golden, ln_key(fmt, rows, H), "LayerNorm outputs")


# ------------------------------------------------------------------------------------------ weight-gradient reduction
def reduce_case(L, nseg, poison=None):
    """n = 2 launches' partials -> gradients by both entry points.  poison: None | "gradient" | "byproduct"."""
    n = 2
    stride = L.adapter_wgrad_workspace_elems(nseg)
    assert stride == nseg * 2 * NBLK * PSTRIDE
    g = torch.Generator().manual_seed(70 + nseg)
    part = torch.randn(n * stride, generator=g) * 0.01
    P = part.view(n, nseg, 2, NBLK, PSTRIDE)
    if poison == "gradient":
        P[1, nseg - 1, 1, 7, 5 * H_ + 11] = float("inf")           # up problem, unit 5, column 11 -> wu[11][5]
    elif poison == "byproduct":
        P[:, :, 0, 3, RH + R_:] = float("inf")                      # down problem's column sums of x
        P[:, :, 1, 6, RH:RH + R_] = float("-inf")                   # up problem's column sums of z
    s32 = torch.zeros(n, nseg, 2, PSTRIDE)
    for b in range(NBLK):
        s32 = s32 + P[:, :, :, b]                                   # ((0 + P_0) + P_1) + ...: fp32, the kernel's order
    d, u = s32[:, :, 0], s32[:, :, 1]
    wu = u[..., :RH].reshape(n, nseg, R_, H_).transpose(-1, -2).reshape(n, nseg, RH)
    want = torch.cat([d[..., :RH + R_], wu, u[..., RH + R_:]], -1)
    dpart = part.to(DEV)
    outs = {}
    for name in ("plain", "checked"):
        grads = torch.full((n, nseg, GN), float("nan"), device=DEV)
        ptrs = torch.tensor([grads[l, s].data_ptr() for l in range(n) for s in range(nseg)], dtype=torch.int64, device=DEV)
        flags = torch.zeros(2, dtype=torch.int32, device=DEV)
        if name == "plain":
            L.adapter_wgrad_reduce(ptrs, n, nseg, dpart, stride)
        else:
            L.adapter_wgrad_reduce_checked(ptrs, n, nseg, dpart, stride, flags)
        torch.cuda.synchronize()
        outs[name] = (grads.cpu(), flags.tolist())
    return want, outs


@pytest.mark.parametrize("nseg", [1, 2])
@pytest.mark.parametrize("poison", [None, "gradient", "byproduct"])
def test_wgrad_reduce_is_the_sequential_fp32_sum(L, nseg, poison):
    want, outs = reduce_case(L, nseg, poison)
    for name, (got, flags) in outs.items():
        diff = int((got.view(torch.int32) != want.view(torch.int32)).sum())
        assert diff == 0, (name, nseg, poison, diff)
        if name == "checked":
            expect = [0, 0]
            if poison == "gradient":
                expect[nseg - 1] = 1
            assert flags == expect, (nseg, poison, flags)
    if poison == "gradient":
        assert int((~torch.isfinite(want)).sum()) == 1 and not bool(torch.isfinite(want[1, nseg - 1, RH + R_ + 11 * R_ + 5]))
    else:
        assert bool(torch.isfinite(want).all())


# ------------------------------------------------------------------------------------------ AdamW
ADAM_SIZES = (20, 1036, 5164)          # whole quads (the entry point's n % 4 == 0), no multiple of 256 or of a 1024-element block
ADAM_SEGS = ([0, 7], [0, 3, 514, 1030], [0, 1025, 1026, 4099])        # boundaries inside quads; the weight decays alternate
LR, WARM, TOTAL, B1, B2, EPS = 1e-4, 3, 40, 0.9, 0.98, 1e-8
ADAM_TICKS = ((1, 0), (5, 6))          # (schedule index, Adam steps done): in warm-up at t = 1; past it at t = 7
# (name, bak_mode, skip flag, restore flag, skip slot: 0 = skip_if[0] alone, 1 = skip_if (a zero flag, the flag): the second slot decides)
# bak_mode 2 with both flags set: the restore wins (the head under the dynamic loss scale: skip_if = (flag B,), restore_if = flag A)
ADAM_MODES = (("plain", 0, 0, 0, 0), ("skip", 0, 1, 0, 0), ("bak", 1, 0, 0, 0), ("bak+skip", 1, 1, 0, 0), ("keep", 2, 0, 0, 0),
              ("restore", 2, 0, 1, 0), ("keep+skip", 2, 1, 0, 0), ("restore+skip", 2, 1, 1, 0), ("skip2nd", 0, 1, 0, 1),
              ("plain2nd", 0, 0, 0, 1), ("bak+skip2nd", 1, 1, 0, 1))


def _adam_inputs(sizes, segs, seed):
    g = torch.Generator().manual_seed(seed)
    data = []
    for n, off in zip(sizes, segs):
        p, gr = torch.randn(n, generator=g) * 0.05, torch.randn(n, generator=g) * 10.0 ** -(n % 3)
        m, v = torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 1e-4
        bak = torch.randn(3 * n, generator=g)
        wd = torch.tensor([0.01 if s % 2 == 0 else 0.0 for s in range(len(off))])
        data.append(dict(p=p, g=gr, m=m, v=v, bak=bak, off=torch.tensor(list(off) + [n], dtype=torch.int64), wd=wd))
    return data


def _adam_f64(d, sched_t, t):
    lam = sched_t / max(1, WARM) if sched_t < WARM else 0.0 if sched_t > TOTAL else 1.0 - (sched_t - WARM) / (TOTAL - WARM)
    f32 = lambda c: float(torch.tensor(c, dtype=torch.float32))         # the kernel's arguments are fp32: 1 - 0.98f is 2e-6 off 0.02
    lr, B1, B2, EPS = f32(LR) * lam, f32(globals()["B1"]), f32(globals()["B2"]), f32(globals()["EPS"])
    n = d["p"].numel()
    wd = torch.zeros(n, dtype=torch.float64)
    for s in range(d["wd"].numel()):
        wd[int(d["off"][s]):int(d["off"][s + 1])] = float(d["wd"][s])
    p, g, m, v = (d[k].double() for k in ("p", "g", "m", "v"))
    p = p * (1 - lr * wd)
    m = m + (g - m) * (1 - B1)
    v = v * B2 + (1 - B2) * g * g
    p = p - lr / (1 - B1 ** t) * (m / (v.sqrt() / (1 - B2 ** t) ** 0.5 + EPS))
    return p, m, v


def adam_case(L, sizes, segs, seed, mode, tick, check=True):
    name, bak_mode, skip, restore, slot = mode
    sched_t, done = tick
    data = _adam_inputs(sizes, segs, seed)
    out = {"inputs": digest(torch.cat([torch.cat([d[k].float() for k in ("p", "g", "m", "v", "bak", "wd")]) for d in data]))}
    f_skip = torch.tensor([skip], dtype=torch.int32, device=DEV)
    f_restore = torch.tensor([restore], dtype=torch.int32, device=DEV)
    f_zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    groups, bufs = [], []
    for d in data:
        b = {k: d[k].clone().to(DEV) for k in ("p", "g", "m", "v", "bak", "off", "wd")}
        state = torch.tensor([sched_t, done], dtype=torch.int32, device=DEV)
        kw = dict(skip_if=(f_zero, f_skip) if slot else (f_skip,))
        if bak_mode:
            kw.update(bak=b["bak"], bak_mode=bak_mode)
        if bak_mode == 2:
            kw.update(restore_if=f_restore)
        groups.append(L.adamw_group(b["p"], b["g"], b["m"], b["v"], b["off"], b["wd"], state, **kw))
        bufs.append(b)
    L.adamw_multi(groups, LR, WARM, TOTAL, B1, B2, EPS)
    torch.cuda.synchronize()
    for k, (d, b) in enumerate(zip(data, bufs)):
        for f in ("p", "m", "v", "bak"):
            out[f"g{k}.{f}"] = digest(b[f])
        if not check:
            continue
        n = d["p"].numel()
        got = {f: b[f].cpu() for f in ("p", "m", "v", "bak")}
        if restore:
            want = dict(p=d["bak"][:n], m=d["bak"][n:2 * n], v=d["bak"][2 * n:])
        elif skip:
            want = dict(p=d["p"], m=d["m"], v=d["v"])
        else:
            p64, m64, v64 = _adam_f64(d, sched_t, done + 1)
            assert float((got["p"].double() - p64).abs().max()) < 2e-7, (name, tick, k)
            # m: three fp32 roundings of values below 0.5; v: four roundings, relative to v (fp32: 2^-24 each)
            assert float((got["m"].double() - m64).abs().max()) < 1e-7
            assert bool(((got["v"].double() - v64).abs() <= 4 * 2.0 ** -24 * v64.abs() + 1e-12).all())
            assert not torch.equal(got["p"], d["p"])
            want = {}
        for f, w in want.items():
            assert torch.equal(got[f], w), (name, tick, k, f)
        want_bak = torch.cat([d["p"], d["m"], d["v"]]) if bak_mode == 1 else d["bak"]
        assert torch.equal(got["bak"], want_bak), (name, tick, k)
    return out


def adam_key(tag, mode, tick):
    return f"adamw.{tag}.{mode[0]}.t{tick[1] + 1}"


@pytest.mark.parametrize("tick", ADAM_TICKS)
@pytest.mark.parametrize("mode", ADAM_MODES, ids=[m[0] for m in ADAM_MODES])
def test_adamw_multi_is_bit_identical_and_right(L, golden, mode, tick):
    _check(adam_case(L, ADAM_SIZES, ADAM_SEGS, 11, mode, tick), golden, adam_key("three", mode, tick), "AdamW results")


MANY = 1100           # more segments than the kernel keeps in LDS (1024): the table is searched in global memory
MANY_SIZES = (4 * MANY + 8,)
MANY_SEGS = ([0] + [4 * s + 1 for s in range(1, MANY)],)


@pytest.mark.parametrize("tick", ADAM_TICKS)
def test_adamw_multi_with_a_segment_table_beyond_lds(L, golden, tick):
    mode = ADAM_MODES[2]
    _check(adam_case(L, MANY_SIZES, MANY_SEGS, 12, mode, tick), golden, adam_key("many", mode, tick), "AdamW results")


# ------------------------------------------------------------------------------------------ im2col / embed / pack
def embed_case(L, fmt, check=True):
    op = L.OPERAND_DTYPE[fmt]
    B, Hi, Wi, P, Lt, H, g0 = 2, 64, 96, 32, 3, 768, 12
    gh, gw = Hi // P, Wi // P
    np_ = gh * gw
    S = Lt + 1 + np_
    g = torch.Generator().manual_seed(90)
    px = torch.randn(B, 3, Hi, Wi, generator=g)
    V = 50
    ids, tts = torch.randint(0, V, (B, Lt), generator=g), torch.randint(0, 2, (B, Lt), generator=g)
    word, pos, typ = torch.randn(V, H, generator=g), torch.randn(40, H, generator=g), torch.randn(2, H, generator=g)
    ln_g, ln_b, mod0, mod1 = (torch.randn(H, generator=g) for _ in range(4))
    proj = torch.randn(B * np_, H, generator=g)
    cls, pos0 = torch.randn(H, generator=g), torch.randn(H, generator=g)
    pos_grid = torch.randn(g0, g0, H, generator=g)
    pm = torch.zeros(B, gh, gw, dtype=torch.int64)
    pm[0], pm[1, :1, :2] = 1, 1                              # sample 1: a 1 x 2 valid patch rectangle
    am = torch.ones(B, Lt, dtype=torch.int64)
    am[1, 2:] = 0
    r, rH, n = R_, RH, 2
    off_u, stride32, stride16 = rH + 48, 2 * rH + 1024, 4 * rH + 256
    flat32 = torch.randn(n * stride32, generator=g) * 0.05
    out = {"inputs": digest(torch.cat([t.flatten().float() for t in (px, ids, tts, word, pos, typ, ln_g, ln_b, mod0, mod1, proj, cls,
                                                                    pos0, pos_grid, flat32)]))}
    d = lambda t: t.to(DEV)
    with L.operands(fmt):
        patches = torch.zeros(B * np_, 3 * P * P, dtype=op, device=DEV)
        L.im2col_patches(d(px), patches, B, 3, Hi, Wi, P)
        h = torch.full((B, S, H), 3.0, device=DEV)
        L.text_embed(d(ids), d(tts), d(word), d(pos), d(typ), d(ln_g), d(ln_b), 1e-12, d(mod0), h, B, Lt, S, H)
        h_text = h.clone()
        km = torch.full((B, S), 7, dtype=torch.uint8, device=DEV)
        L.image_embed_assemble_masked(d(proj), d(cls), d(pos0), d(pos_grid), d(pm), d(am), d(mod1), h, km, B, Lt, gh, gw, g0, H)
        buf = torch.full((n * stride16,), -7.0, dtype=op, device=DEV)
        f32 = d(flat32)
        L.adapter_pack_strided(f32, f32[off_u:], stride32, buf, buf[rH:], buf[2 * rH:], buf[3 * rH:], stride16, n)
        torch.cuda.synchronize()
        out.update({"im2col": digest(patches), "text_embed.h": digest(h_text), "image.h": digest(h), "image.key_mask": digest(km),
                    "pack": digest(buf)})
        if not check:
            return out
        ref = F.unfold(px, P, stride=P).transpose(1, 2).reshape(B * np_, 3 * P * P).to(op)
        assert torch.equal(patches.cpu(), ref)
        e = (word[ids] + typ[tts] + pos[:Lt]).double()
        want = F.layer_norm(e, (H,), ln_g.double(), ln_b.double(), 1e-12) + mod0.double()
        assert float((h_text[:, :Lt].cpu().double() - want).abs().max()) < 2e-5            # tests/test_ops_gpu.py's bound
        assert bool((h_text[:, Lt:] == 3.0).all()) and torch.equal(h[:, :Lt], h_text[:, :Lt])
        # the image tail = its three separate launches
        h3, km3 = h_text.clone(), torch.full((B, S), 7, dtype=torch.uint8, device=DEV)
        pos_img = torch.empty(B, np_, H, device=DEV)
        L.vilt_key_mask(d(am), d(pm), km3, B, Lt, gh, gw, 1)
        L.pos_embed_resize_masked(d(pos_grid), d(pm), pos_img, g0, B, gh, gw, 1, H)
        L.image_embed_assemble(d(proj), d(cls), d(pos0), pos_img, d(mod1), h3, B, Lt, np_, S, H, pos_batch_stride=np_ * H)
        torch.cuda.synchronize()
        assert torch.equal(h, h3) and torch.equal(km, km3)
        assert torch.equal(h[:, Lt].cpu(), ((cls + pos0) + mod1).expand(B, H))                # the CLS row, in the kernel's order
        assert km[:, Lt + 1:].long().sum(1).tolist() == [np_, 2] and km[:, :Lt].long().sum(1).tolist() == [3, 2]
        # pack: four permuted 16-bit copies per module, the gaps untouched
        for l in range(n):
            wd = flat32[l * stride32: l * stride32 + rH].to(op).float().sort().values
            wu = flat32[l * stride32 + off_u: l * stride32 + off_u + rH].to(op).float().sort().values
            for c, src in enumerate((wd, wd, wu, wu)):
                got = buf[l * stride16 + c * rH: l * stride16 + (c + 1) * rH].cpu().float().sort().values
                assert torch.equal(got, src), (l, c)
            assert bool((buf[l * stride16 + 4 * rH: (l + 1) * stride16] == -7.0).all()), l
    return out


@pytest.mark.parametrize("fmt", FMTS)
def test_im2col_embed_pack_are_bit_identical_and_right(L, golden, fmt):
    _check(embed_case(L, fmt), golden, f"embed.{fmt}", "im2col / embed / pack outputs")


def all_digests(L):
    """Every fixture entry (tools/make_stream_golden.py, run on the commit whose kernels are the reference)."""
    out = {}
    for fmt in FMTS:
        out[f"embed.{fmt}"] = embed_case(L, fmt, check=False)
        for rows, H in ln_shapes():
            out[ln_key(fmt, rows, H)] = ln_case(L, fmt, rows, H, check=False)
    for tick in ADAM_TICKS:
        for mode in ADAM_MODES:
            out[adam_key("three", mode, tick)] = adam_case(L, ADAM_SIZES, ADAM_SEGS, 11, mode, tick, check=False)
        out[adam_key("many", ADAM_MODES[2], tick)] = adam_case(L, MANY_SIZES, MANY_SEGS, 12, ADAM_MODES[2], tick, check=False)
    return out
