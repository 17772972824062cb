"""The fused dual adapter (csrc/adapter.hip, csrc/adapter_wgrad.hip) element by element against float64, in both operand builds.

Every adapter gradient of the round passes through feddat_adapter_bwd's z / dz, and every lower layer's gradient through its dx.
This module restates the kernels in float64 on the operands the kernels round, at the descriptors the engines build and at the
edges of the segment ABI, and bounds every element.

Restatement (_seg_ref): the 16-bit roundings sit where adapter.hip puts them -- x to 16 bits for the down-projection (cvt8), z to 16
bits for the up-projection (pad8 / cvt8), dy to 16 bits for g = Wu^T dy and dz = scale g (z > 0) to 16 bits for the Wd^T dz
product (backward steps 3-5); the weights are the packed operands w32.to(OPERAND_DTYPE); the residual, the biases, the exported
z / dz and dx stay fp32.  The reference keeps z and dz UNROUNDED (fp64) and the bound carries their 16-bit rounding.

Bounds, per element, derived (u32 = 2^-24; u16 = 2^-8 bf16, 2^-11 fp16; eta16 = half the smallest subnormal step, 2^-25 fp16):
  |got - ref| <= c * u32 * sum|terms| + u16 * sum|propagated rounded terms| (+ the propagated bounds of the inputs)
  C_DN = 80   K = 768 products (down-projection, Wu^T dy): 16-bit x 16-bit products are exact in fp32; a wave chains 6 MFMAs
              (each at most log2(32) + 1 = 6 roundings deep), 3 K-split adds, 1 bias add = 40 roundings, doubled for an adder
              that truncates (2^-23 per step).
  C_UP = 32   K = 48 products (up-projection, Wd^T dz): 2 chained MFMAs (12), bias add and one residual add per adapter (3),
              doubled.
  C_LN = 128  fused LayerNorm statistics: 48 sequential adds per lane, 2 shuffles, the 4-wave combine, rsqrt: < 64, doubled.
  C_W(n)      adapter_wgrad over n tokens: the split-bf16 products carry 2^-17 relative; per wave ceil(tps / 32) rounds of 4 chained
              MFMAs (24 roundings) plus tps sequential column-sum adds, the 4-wave LDS sum (3), the 10-block reduce (10), the scale
              (1) and 2 shuffles, doubled.
ReLU masks: the kernel's z must lie within C_DN u32 sum|terms| of relu(pre64), so its mask (z > 0) can differ from the fp64 mask
only where |pre64| <= (C_DN / 4) 2^-22 sum|terms|; such units are counted and must be rare.  dz and dx are restated with the
KERNEL's mask, so every element gets the strict bound.  The fp16 build's bounds are shown to fail on a restatement that rounds z,
dy or dz through bf16 instead.

Segment layouts: empty segments, segments that start after row 0 with gaps between them, positive and negative x_row_delta and
train_slot 1 / -1 are SUPPORTED by the ABI (prep_launch accepts them; every row outside every segment is left untouched and is
checked for that with a sentinel).  A train_slot outside [-1, n_adapters) is refused.

Each case prints its worst measured ratio to the bound (run with -s)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMTS = ("bf16", "f16")
H, RB = 768, 48
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
ETA16 = {"bf16": 2.0 ** -134, "f16": 2.0 ** -25}
U32 = 2.0 ** -24
C_DN, C_UP, C_LN = 80, 32, 128
FLIP_MULT = C_DN / 4              # the mask-flip band in units of 2^-22 sum|terms|
SENT = -31.0                      # sentinel of every output buffer (exact in all formats)
LN_EPS = 1e-12                    # the engines' layernorm eps
F16_INF_FROM = 65520.0            # fp16 round-to-nearest-even overflows at and above this


def C_W(n):
    tps = -(-n // 40)
    tps = (tps + 7) // 8 * 8
    return 2 * (24 * -(-tps // 32) + tps + 16)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import lib
    lib.load()
    with lib.operands("f16"):
        lib.load()
    return lib


def _r16(t, fmt):
    """float64 value of the 16-bit round-to-nearest-even of fp32 t (the kernels' cvt of an fp32 value)."""
    return t.float().to(DT[fmt]).double()


def _params(L, fmt, seed, wstd=0.05):
    """Three adapters (adapter_0, adapter_1, adapter_2 of one layer): fp32 masters, the build's packed operands and the float64
    values of those operands."""
    gen = torch.Generator().manual_seed(seed)
    par = []
    for _ in range(3):
        wd = (torch.randn(RB, H, generator=gen) * wstd).to(DEV)
        wu = (torch.randn(H, RB, generator=gen) * wstd).to(DEV)
        bd = (torch.randn(RB, generator=gen) * 0.1).to(DEV)
        bu = (torch.randn(H, generator=gen) * 0.1).to(DEV)
        dt = DT[fmt]
        w = [torch.empty(RB, H, dtype=dt, device=DEV), torch.empty(H, RB, dtype=dt, device=DEV),
             torch.empty(H, RB, dtype=dt, device=DEV), torch.empty(RB, H, dtype=dt, device=DEV)]
        with L.operands(fmt):
            L.adapter_pack(wd, wu, *w)
        par.append(dict(wd=w[0], wdT=w[1], wu=w[2], wuT=w[3], bd=bd, bu=bu,
                        wd64=wd.to(dt).double(), wu64=wu.to(dt).double(), bd64=bd.double(), bu64=bu.double()))
    return par


def _seg(rb, re, ads, ts=0, xd=0):
    """ads: (adapter index, scale) per slot."""
    return dict(rb=rb, re=re, ads=tuple(ads), ts=ts, xd=xd)


GATED = ((0, 0.5), (2, 0.5))
AD1 = ((1, 1.0),)


def _vilt(R, first=False):
    """ViltDatEngine._segs (engine.py): rows [0,R) gated adapter_0 + adapter_2 at 0.5, rows [R,2R) adapter_1 at 1.0; layer 0
    (first=True): the second segment reads the same R input rows (x_row_delta = -R).  Also _top_segs with R = B."""
    return [_seg(0, R, GATED), _seg(R, 2 * R, AD1, xd=-R if first else 0)]


def _cases():
    c = []
    for B in (32, 64, 7):            # configs[1]; B = 64: several rounds of the persistent grid; B = 7: boundary mid-tile
        R = 185 * B
        c.append((f"vilt_inner_B{B}", 2 * R, _vilt(R)))
        c.append((f"vilt_layer0_B{B}", 2 * R, _vilt(R, first=True)))
    for B in (32, 7):                # ViltDatEngine._top_segs: the 2B token-0 rows (B = 7: fewer tiles than CUs)
        c.append((f"vilt_top_B{B}", 2 * B, _vilt(B)))
    for rows in (185 * 32, 32):      # ViltAdapterEngine._segs / _top_segs (adapter_engine.py): one segment, one adapter
        c.append((f"adapter_mode_{rows}", rows, [_seg(0, rows, ((0, 1.0),))]))
    for rows in (32 * 577, 32 * 25, 32 * 25 + 1):     # AlbefBackbone._segs (albef_backbone.py): image rows, question rows, odd
        h = rows // 2
        c.append((f"albef_both_{rows}", rows, [_seg(0, h, GATED), _seg(h, rows, AD1)]))
        c.append((f"albef_gating_{rows}", rows, [_seg(0, rows, GATED)]))
        c.append((f"albef_adapter_1_{rows}", rows, [_seg(0, rows, AD1)]))
    # edges of the segment ABI
    c.append(("T1", 1, [_seg(0, 1, GATED)]))
    c.append(("T1_empty_seg1", 1, [_seg(0, 1, AD1), _seg(1, 1, GATED)]))
    c.append(("rows_1_15", 16, [_seg(0, 1, GATED), _seg(1, 16, AD1)]))
    c.append(("rows_16_17", 33, [_seg(0, 16, AD1), _seg(16, 33, GATED)]))
    c.append(("t0_much_smaller", 16 + 11840, [_seg(0, 16, GATED), _seg(16, 16 + 11840, AD1)]))
    c.append(("t0_much_larger", 11840 + 17, [_seg(0, 11840, GATED), _seg(11840, 11840 + 17, AD1)]))
    c.append(("empty_seg0", 300, [_seg(0, 0, GATED), _seg(0, 300, AD1)]))
    c.append(("empty_seg1", 300, [_seg(0, 300, GATED), _seg(300, 300, AD1)]))
    c.append(("gaps_and_positive_delta", 320, [_seg(5, 40, GATED, xd=200), _seg(77, 300, AD1)]))
    c.append(("train_slot_1_and_none", 200, [_seg(0, 100, GATED, ts=1), _seg(100, 200, AD1, ts=-1)]))
    return c


CASES = _cases()


def _csegs(L, segs, par, bwd):
    """The C descriptor; the forward's carries train_slot -1, as every engine's does."""
    return L.make_segs([dict(row_begin=s["rb"], row_end=s["re"], train_slot=s["ts"] if bwd else -1, x_row_delta=s["xd"],
                             adapters=[dict(par[a], scale=sc) for a, sc in s["ads"]]) for s in segs])


def _data(T, segs, seed, dy_scale=1.0):
    """x and dy of T rows; every x row no segment reads and every dy row outside the segments is NaN (a stray read poisons
    an output that is checked)."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(T, H, generator=gen, device=DEV)
    dy = torch.randn(T, H, generator=gen, device=DEV) * dy_scale
    xread = torch.zeros(T, dtype=torch.bool, device=DEV)
    inside = torch.zeros(T, dtype=torch.bool, device=DEV)
    for s in segs:
        xread[s["rb"] + s["xd"]:s["re"] + s["xd"]] = True
        inside[s["rb"]:s["re"]] = True
    x[~xread] = float("nan")
    dy[~inside] = float("nan")
    return x, dy, inside


class _Ratios:
    def __init__(self):
        self.r = {}

    def check(self, key, err, bound, what):
        """err <= bound element-wise; records the worst ratio."""
        if err.numel() == 0:
            return
        ratio = err / bound.clamp_min(1e-300)
        worst = float(ratio.max())
        assert not bool(torch.isnan(err).any()), (what, key, "NaN")
        self.r[key] = max(self.r.get(key, 0.0), worst)
        assert worst <= 1.0, (what, key, worst)

    def note(self, key, v):
        self.r[key] = max(self.r.get(key, 0.0), v)

    def line(self):
        return " ".join(f"{k} {v:.3g}" for k, v in sorted(self.r.items()))


def _seg_ref(fmt, s, par, x, dy, zk):
    """float64 restatement of one segment on the operands the kernels round.  zk: the forward's z_save rows of the segment
    (the kernel's own ReLU masks).  Returns the per-slot and per-segment references with their bounds."""
    u, eta = U16[fmt], ETA16[fmt]
    rb, re, xd = s["rb"], s["re"], s["xd"]
    xs = x[rb + xd:re + xd].double()
    X = _r16(xs, fmt)
    dys = dy[rb:re].double()
    DY = _r16(dys, fmt)
    out = xs.clone()
    outA, outB = xs.abs(), torch.zeros_like(xs)
    dx = dys.clone()
    dxA, dxB = dys.abs(), torch.zeros_like(dys)
    alt = dict(out=xs.clone(), dx=dys.clone())         # z resp. dz rounded through bf16
    slots = []
    for k, (a, sc) in enumerate(s["ads"]):
        p = par[a]
        wd, wu = p["wd64"], p["wu64"]                  # [RB, H], [H, RB]
        pre = X @ wd.t() + p["bd64"]
        apre = X.abs() @ wd.abs().t() + p["bd64"].abs()          # sum|terms| of the pre-activation
        ez = C_DN * U32 * apre
        z64 = pre.clamp_min(0.0)
        out += sc * (z64 @ wu.t() + p["bu64"])
        outA += sc * (z64 @ wu.abs().t() + p["bu64"].abs())
        outB += sc * ((u * z64 + eta * (z64 > 0) + ez) @ wu.abs().t())
        alt["out"] += sc * (_r16(z64, "bf16") @ wu.t() + p["bu64"])
        mk = (zk[:, k] > 0).double()
        g = DY @ wu
        dz = sc * g * mk
        edz = C_DN * U32 * sc * (DY.abs() @ wu.abs()) * mk
        dz_alt = sc * (_r16(dys, "bf16") @ wu) * mk     # dy rounded through bf16
        dx += dz @ wd
        dxA += dz.abs() @ wd.abs()
        dxB += (u * dz.abs() + (eta + edz) * mk) @ wd.abs()
        alt["dx"] += _r16(dz, "bf16") @ wd
        slots.append(dict(pre=pre, apre=apre, ez=ez, z=z64, dz=dz, edz=edz, dz_alt=dz_alt, mk=mk.bool(), sc=sc))
    return dict(xs=xs, dys=dys, slots=slots, out=out, bout=C_UP * U32 * outA + outB, dx=dx, bdx=C_UP * U32 * dxA + dxB, alt=alt)


def _ln_ref(o64, bout, gamma, beta, fmt):
    """float64 LayerNorm of the float64 adapter output and bounds for the fused kernel's stats and 16-bit y: the kernel
    normalises its own out (within bout of o64) in fp32."""
    g, b = gamma.double(), beta.double()
    mu = o64.mean(1)
    var = o64.var(1, unbiased=False)
    sig = var.sqrt()
    rs = 1.0 / (var + LN_EPS).sqrt()
    e_mu = C_LN * U32 * o64.abs().mean(1) + bout.mean(1)
    d = bout + e_mu[:, None]                              # |(o_k - mu_k) - (o64 - mu64)|
    q = (d.pow(2).mean(1)).sqrt() / sig
    e_rs = rs * (C_LN * U32 + q + q * q)
    c = o64 - mu[:, None]
    y = c * rs[:, None] * g + b
    e_y = g.abs() * (d * rs[:, None] + c.abs() * e_rs[:, None]) + 8 * U32 * ((c * rs[:, None] * g).abs() + b.abs())
    return mu, rs, y, e_mu, e_rs, e_y + U16[fmt] * (y.abs() + e_y) + ETA16[fmt]




NGRAD = RB * H + RB + H * RB + H        # one layer's flat adapter gradient [wd | bd | wu | bu]


def _wgrads(L, fmt, segs, x, dy, z, dz, flags=None):
    """adapter_wgrad_partial + adapter_wgrad_reduce (or _reduce_checked with `flags`) over the train-slot segments, from the
    backward's exported z / dz; x rows offset by x_row_delta as in ViltDatEngine._wgrad_segs.  Returns [nseg, NGRAD]."""
    tr = [s for s in segs if s["ts"] >= 0 and s["re"] > s["rb"]]
    if not tr:
        return tr, None
    grads = torch.full((len(tr), NGRAD), float("nan"), device=DEV)
    with L.operands(fmt):
        ws = L.make_wgrad_segs([dict(x=x[s["rb"] + s["xd"]:], dy=dy[s["rb"]:], z=z[s["rb"]:], dz=dz[s["rb"]:], grad=grads[i],
                                     rows=s["re"] - s["rb"], scale=s["ads"][s["ts"]][1]) for i, s in enumerate(tr)])
        stride = L.adapter_wgrad_workspace_elems(len(tr))
        part = torch.empty(stride, device=DEV)
        L.adapter_wgrad_partial(ws, part)
        ptrs = torch.tensor([g.data_ptr() for g in grads], dtype=torch.int64, device=DEV)
        if flags is None:
            L.adapter_wgrad_reduce(ptrs, 1, len(tr), part, stride)
        else:
            L.adapter_wgrad_reduce_checked(ptrs, 1, len(tr), part, stride, flags)
    torch.cuda.synchronize()
    return tr, grads


def _run(L, fmt, T, segs, par, x, dy, *, with_ln=True, seed=0):
    """Every entry point of the family on one case, into sentinel-filled buffers."""
    dt = DT[fmt]
    o = {}

    def buf(*shape, dtype=torch.float32):
        return torch.full(shape, SENT, dtype=dtype, device=DEV)
    with L.operands(fmt):
        cf, cb = _csegs(L, segs, par, False), _csegs(L, segs, par, True)
        o["out"], o["zsave"] = buf(T, H), buf(T, 2, RB)
        L.adapter_fwd(x, o["out"], cf, T, z_save=o["zsave"])
        if with_ln:
            gen = torch.Generator().manual_seed(seed + 7)
            o["gamma"] = (1 + 0.1 * torch.randn(H, generator=gen)).to(DEV)
            o["beta"] = (0.1 * torch.randn(H, generator=gen)).to(DEV)
            o["out_ln"], o["zsave_ln"], o["y16"], o["st"] = buf(T, H), buf(T, 2, RB), buf(T, H, dtype=dt), buf(T, 2)
            L.adapter_fwd_ln(x, o["out_ln"], cf, T, o["gamma"], o["beta"], LN_EPS, o["y16"], o["st"], z_save=o["zsave_ln"])
        for path in ("bwd_z", "bwd_x"):        # from the saved z (x is not read) / recomputing z from x
            xx, zz = (None, o["zsave"]) if path == "bwd_z" else (x, None)
            r = dict(dx=buf(T, H), dx16=buf(T, H, dtype=dt), z=buf(T, RB), dz=buf(T, RB), z_nodx=buf(T, RB), dz_nodx=buf(T, RB))
            L.adapter_bwd(xx, dy, r["dx"], cb, T, dx_bf16=r["dx16"], z_out=r["z"], dz_out=r["dz"], z_saved=zz)
            L.adapter_bwd(xx, dy, None, cb, T, z_out=r["z_nodx"], dz_out=r["dz_nodx"], z_saved=zz)   # layer 0's call
            o[path] = r
        if fmt == "bf16":                      # configs[4]: the same backward with an e4m3 copy of dx
            r = dict(dx=buf(T, H), z=buf(T, RB), dz=buf(T, RB))
            d8, dsc = torch.zeros(T, H, dtype=torch.uint8, device=DEV), torch.zeros(T, device=DEV)
            L.adapter_bwd_fp8(dy, r["dx"], d8, dsc, cb, T, z_saved=o["zsave"], z_out=r["z"], dz_out=r["dz"])
            o["fp8"] = r
    torch.cuda.synchronize()
    o["tr"], o["grads"] = _wgrads(L, fmt, segs, x, dy, o["bwd_z"]["z"], o["bwd_z"]["dz"])
    return o


def _check(L, fmt, T, segs, par, x, dy, inside, o, what, *, sens=True):
    """Section 1 + 2 checks of one run; returns the ratio record."""
    dt = DT[fmt]
    R = _Ratios()
    out = lambda t: t[~inside]                                    # noqa: E731
    # ---- stores stay inside the segments
    for name, t in (("out", o["out"]), ("zsave", o["zsave"]), ("out_ln", o.get("out_ln")), ("y16", o.get("y16")),
                    ("stats", o.get("st")), ("zsave_ln", o.get("zsave_ln"))):
        if t is not None:
            assert bool((out(t).float() == SENT).all()), (what, name, "store outside the segments")
    for path in ("bwd_z", "bwd_x", "fp8"):
        for name, t in o.get(path, {}).items():
            assert bool((out(t).float() == SENT).all()), (what, path, name, "store outside the segments")
    n_units = n_band = n_flip = 0
    refs = []
    for s in segs:
        rb, re = s["rb"], s["re"]
        if re == rb:
            continue
        zk = o["zsave"][rb:re].double()
        ref = _seg_ref(fmt, s, par, x, dy, zk)
        refs.append((s, ref))
        na = len(s["ads"])
        if na == 1:        # slot 1 of a single-adapter segment stays untouched
            assert bool((o["zsave"][rb:re, 1] == SENT).all()), (what, "z_save slot 1 written")
        assert torch.equal(o["out_ln"][rb:re], o["out"][rb:re]), (what, "adapter_fwd_ln out != adapter_fwd out")
        assert torch.equal(o["zsave_ln"][rb:re], o["zsave"][rb:re]), (what, "adapter_fwd_ln z_save != adapter_fwd z_save")
        # ---- forward: z per slot, then out
        for k, sl in enumerate(ref["slots"]):
            R.check("z", (zk[:, k] - sl["z"]).abs(), sl["ez"], what)
            band = sl["pre"].abs() <= FLIP_MULT * 2.0 ** -22 * sl["apre"]
            flip = sl["mk"] != (sl["pre"] > 0)
            assert not bool((flip & ~band).any()), (what, "ReLU mask differs outside the noise band")
            n_units += band.numel()
            n_band += int(band.sum())
            n_flip += int(flip.sum())
        R.check("out", (o["out"][rb:re].double() - ref["out"]).abs(), ref["bout"], what)
        # ---- fused LayerNorm: stats and the 16-bit y against the fp64 LayerNorm of the fp64 out
        mu, rs, y, e_mu, e_rs, e_y = _ln_ref(ref["out"], ref["bout"], o["gamma"], o["beta"], fmt)
        R.check("ln_mean", (o["st"][rb:re, 0].double() - mu).abs(), e_mu, what)
        R.check("ln_rstd", (o["st"][rb:re, 1].double() - rs).abs(), e_rs, what)
        R.check("ln_y16", (o["y16"][rb:re].double() - y).abs(), e_y, what)
        # ---- backward, both paths (and the fp8 form: bit-identical)
        ts = s["ts"]
        for path in ("bwd_z", "bwd_x"):
            r = o[path]
            R.check("dx", (r["dx"][rb:re].double() - ref["dx"]).abs(), ref["bdx"], f"{what} {path}")
            assert torch.equal(r["dx16"][rb:re], r["dx"][rb:re].to(dt)), (what, path, "dx16 != RNE(dx)")
            if ts >= 0:
                sl = ref["slots"][ts]
                # the exported z is the forward's saved z (recomputed with the same arithmetic on the x path)
                assert torch.equal(r["z"][rb:re], o["zsave"][rb:re, ts]), (what, path, "z_out != the forward's z")
                R.check("dz", (r["dz"][rb:re].double() - sl["dz"]).abs(), sl["edz"], f"{what} {path}")
            else:
                for name in ("z", "dz", "z_nodx", "dz_nodx"):
                    assert bool((r[name][rb:re] == SENT).all()), (what, path, name, "z / dz of a train_slot -1 segment written")
            assert torch.equal(r["z_nodx"][rb:re], r["z"][rb:re]) and torch.equal(r["dz_nodx"][rb:re], r["dz"][rb:re]), \
                (what, path, "dx = None changes z / dz")
        for name in ("dx", "dx16", "z", "dz"):
            assert torch.equal(o["bwd_x"][name][rb:re], o["bwd_z"][name][rb:re]), (what, name, "x path != z_saved path")
        if "fp8" in o:
            for name in ("dx", "z", "dz"):
                assert torch.equal(o["fp8"][name][rb:re], o["bwd_z"][name][rb:re]), (what, name, "adapter_bwd_fp8 != adapter_bwd")
        # ---- the bf16-rounding sensitivity of the fp16 bounds (z, dy and dz each rounded through bf16 instead)
        if fmt == "f16" and sens and re - rb >= 16:
            R.note("sens_out", float(((ref["alt"]["out"] - ref["out"]).abs() / ref["bout"]).max()))
            R.note("sens_dx", float(((ref["alt"]["dx"] - ref["dx"]).abs() / ref["bdx"]).max()))
            R.note("sens_dz", max(float(((sl["dz_alt"] - sl["dz"]).abs() / sl["edz"].clamp_min(1e-300)).max())
                                  for sl in ref["slots"]))
    if fmt == "f16" and sens and any(s["re"] - s["rb"] >= 16 for s in segs):
        for k in ("sens_out", "sens_dx", "sens_dz"):
            assert R.r[k] > 1.0, (what, k, R.r[k], "the fp16 bound does not see a bf16 rounding")
    # the noise band is rare, flips rarer
    assert n_band <= max(8, n_units >> 12), (what, n_band, n_units)
    R.note("mask_band", n_band)
    R.note("mask_flips", n_flip)
    # ---- weight gradients against the fp64 chain dz64^T x, sum dz64, s dy64^T z64, s sum dy
    if o["grads"] is not None:
        byseg = {id(s): ref for s, ref in refs}
        for i, s in enumerate(o["tr"]):
            ref = byseg[id(s)]
            sl, sc = ref["slots"][s["ts"]], s["ads"][s["ts"]][1]
            n = s["re"] - s["rb"]
            cw = C_W(n) * U32 + 2.0 ** -17
            xs, dys = ref["xs"], ref["dys"]
            zk = o["bwd_z"]["z"][s["rb"]:s["re"]].double()
            dzk = o["bwd_z"]["dz"][s["rb"]:s["re"]].double()
            g = o["grads"][i].double()
            a0, a1, a2 = RB * H, RB * H + RB, RB * H + RB + H * RB
            R.check("wgrad_wd", (g[:a0].view(RB, H) - sl["dz"].t() @ xs).abs(),
                    cw * dzk.abs().t() @ xs.abs() + sl["edz"].t() @ xs.abs(), what)
            R.check("wgrad_bd", (g[a0:a1] - sl["dz"].sum(0)).abs(), cw * dzk.abs().sum(0) + sl["edz"].sum(0), what)
            R.check("wgrad_wu", (g[a1:a2].view(H, RB) - sc * dys.t() @ sl["z"]).abs(),
                    cw * sc * dys.abs().t() @ zk.abs() + sc * dys.abs().t() @ sl["ez"], what)
            R.check("wgrad_bu", (g[a2:] - sc * dys.sum(0)).abs(), cw * sc * dys.abs().sum(0) + 1e-300, what)
    return R


@pytest.fixture(scope="module")
def params(L):
    return {fmt: _params(L, fmt, 11) for fmt in FMTS}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("fmt", FMTS)
def test_adapter_family_vs_fp64(L, params, fmt, case):
    """Sections 1 + 2: forward (+ fused LayerNorm), both backward paths (+ dx = None, + the fp8 form), weight gradients, the
    stores outside the segments, at the engines' descriptors and the ABI's edges."""
    name, T, segs = case
    par = params[fmt]
    seed = sum(map(ord, name))
    x, dy, inside = _data(T, segs, seed)
    o = _run(L, fmt, T, segs, par, x, dy, seed=seed)
    R = _check(L, fmt, T, segs, par, x, dy, inside, o, f"{fmt} {name}")
    print(f"\n[adapter {fmt} {name}] worst ratio to bound: {R.line()}")


# ====================================================================================== 3. the loss-scaled range
HR = 7 * 185          # ViLT inner layer at B = 7 (boundary mid-tile)


def _exact_dx_max(fmt, segs, par, x, dy, zsave):
    return max(float(_seg_ref(fmt, s, par, x, dy, zsave[s["rb"]:s["re"]].double())["dx"].abs().max()) for s in segs)


@pytest.mark.parametrize("fmt", FMTS)
def test_adapter_bwd_loss_scale_headroom(L, params, fmt):
    """dy x 2^k with the largest exact |dx| in [2^12, 2^13).  bf16 build: dx, dx16, z, dz and the weight gradients are 2^k x the
    unscaled call's bit for bit (z unchanged).  fp16 build: every output finite and within the bounds of section 1."""
    par, segs, T = params[fmt], _vilt(HR), 2 * HR
    x, dy, inside = _data(T, segs, 91)
    o1 = _run(L, fmt, T, segs, par, x, dy, seed=91)
    s = 2.0 ** (12 - math.floor(math.log2(_exact_dx_max(fmt, segs, par, x, dy, o1["zsave"]))))
    o2 = _run(L, fmt, T, segs, par, x, dy * s, seed=91)
    for path in ("bwd_z", "bwd_x"):
        a, b = o1[path], o2[path]
        assert bool(torch.isfinite(b["dx"][inside]).all() and torch.isfinite(b["dz"][inside]).all())
        if fmt == "bf16":
            assert torch.equal(b["dx"][inside], a["dx"][inside] * s), path
            assert torch.equal(b["dx16"][inside], (a["dx16"][inside].float() * s).to(torch.bfloat16)), path
            assert torch.equal(b["dz"][inside], a["dz"][inside] * s), path
            assert torch.equal(b["z"][inside], a["z"][inside]), path
    if fmt == "bf16":
        assert torch.equal(o2["grads"], o1["grads"] * s)
    else:
        assert bool(torch.isfinite(o2["grads"]).all())
        R = _check(L, fmt, T, segs, par, x, dy * s, inside, o2, f"{fmt} headroom 2^{int(math.log2(s))}", sens=False)
        print(f"\n[adapter {fmt} loss scale 2^{int(math.log2(s))}] worst ratio to bound: {R.line()}")


def test_adapter_bwd_fp16_overflow_is_nonfinite(L, params):
    """fp16 build, ViLT inner layer, segment 1's dy x 2^k with max |2^k dy| in [2^16, 2^17) (some tokens overflow, most do not),
    plus rows crafted so that 2^k dy stays at 4096 while one active unit's dz exceeds 2^17.  For every token with an element above 2^16 (of 2^k dy, or of dz at
    an active unit) and an active unit, dx is non-finite in every column and the 16-bit overflow never comes out as a finite
    clamped value; dz (fp32) is non-finite at the active units where 2^k dy overflowed and finite, unclamped (> 65504) where
    only dz did.  Segment 0 (unscaled) is bit-identical with the unscaled call, and adapter_wgrad_reduce_checked flags
    segment 1 and only segment 1."""
    fmt, par, segs, T = "f16", params["f16"], _vilt(HR), 2 * HR
    x, dy, inside = _data(T, segs, 97)
    o1 = _run(L, fmt, T, segs, par, x, dy, seed=97)
    zs1 = o1["zsave"][HR:, 0]
    s = 2.0 ** (16 - math.floor(math.log2(float(dy[HR:].abs().max()))))
    wu1 = par[1]["wu64"]
    crafted = torch.arange(HR + 3, T, 97, device=DEV)
    r0 = zs1[crafted - HR].argmax(1)
    assert bool((zs1[crafted - HR].gather(1, r0[:, None]) > 0).all())
    dys = dy.clone()
    dys[crafted] = (2.0 ** 12 / s) * torch.sign(wu1[:, r0].t()).float()
    dys[HR:] *= s
    o2 = _run(L, fmt, T, segs, par, x, dys, seed=97)
    act = zs1 > 0                                                    # [HR, RB] active units of segment 1
    dy_ovf = (dys[HR:].abs() >= F16_INF_FROM).any(1)
    dz_exact = _r16(torch.where(dys[HR:].abs() >= F16_INF_FROM, 0.0, dys[HR:]), fmt) @ wu1
    dz_ovf = ((dz_exact.abs() >= 2.0 ** 16 * 1.01) & act).any(1) & ~dy_ovf
    hot = (dy_ovf | dz_ovf) & act.any(1)
    cold = ~(dys[HR:].abs() >= 65504.0).any(1) & ~((dz_exact.abs() >= 65504.0 / 1.01) & act).any(1)
    assert int(dy_ovf.sum()) > 0 and int(cold.sum()) > 0 and bool(dz_ovf[crafted - HR].all())
    for path in ("bwd_z", "bwd_x"):
        r = o2[path]
        dx1, dz1 = r["dx"][HR:], r["dz"][HR:]
        assert not bool(torch.isfinite(dx1[hot]).any()), (path, "a finite dx where a 16-bit operand overflowed")
        assert not bool(torch.isfinite(dz1[dy_ovf[:, None] & act]).any()), (path, "a finite dz where 2^k dy overflowed")
        d = dz1[crafted - HR].gather(1, r0[:, None])
        assert bool(torch.isfinite(d).all() and (d.abs() > 65504.0).all()), (path, "the fp32 dz of a crafted row is clamped")
        assert bool(torch.isfinite(dx1[cold]).all()), path
        for name in ("dx", "dx16", "z", "dz"):
            assert torch.equal(r[name][:HR], o1[path][name][:HR]), (path, name, "segment 0 changed")
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    _wgrads(L, fmt, segs, x, dys, o2["bwd_z"]["z"], o2["bwd_z"]["dz"], flags=flags)
    assert flags.tolist() == [0, 1]
    print(f"\n[adapter f16 overflow 2^{int(math.log2(s))}] hot tokens {int(hot.sum())} of {HR} "
          f"(2^k dy overflow {int(dy_ovf.sum())}, dz only {int(dz_ovf.sum())}), finite-range tokens {int(cold.sum())}")


# ====================================================================================== 4. refusals
@pytest.mark.parametrize("fmt", FMTS)
def test_adapter_refusals(L, params, fmt):
    """Descriptors and argument combinations the ABI does not define raise FeddatHipError and write nothing."""
    par, T = params[fmt], 64
    dt = DT[fmt]
    x, dy, _ = _data(T, _vilt(32), 5)
    out, dx, dx16 = (torch.full((T, H), SENT, device=DEV), torch.full((T, H), SENT, device=DEV),
                     torch.full((T, H), SENT, dtype=dt, device=DEV))
    zs, z, dz = torch.full((T, 2, RB), SENT, device=DEV), torch.full((T, RB), SENT, device=DEV), torch.full((T, RB), SENT, device=DEV)

    def segs_of(desc, ads=None):
        return L.make_segs([dict(row_begin=s["rb"], row_end=s["re"], train_slot=s["ts"], x_row_delta=s["xd"],
                                 adapters=ads if ads is not None else [dict(par[a], scale=sc) for a, sc in s["ads"]])
                            for s in desc])

    def refused(fn):
        with L.operands(fmt):
            with pytest.raises(L.FeddatHipError):
                fn()
        torch.cuda.synchronize()
        for t in (out, dx, dx16, zs, z, dz):
            assert bool((t.float() == SENT).all()), "a refused call wrote"

    def fwd(c):
        return lambda: L.adapter_fwd(x, out, c, T, z_save=zs)

    def bwd(c):
        return lambda: L.adapter_bwd(x, dy, dx, c, T, dx_bf16=dx16, z_out=z, dz_out=dz)

    good = _vilt(32)
    three = segs_of(good + [_seg(0, 0, AD1)])
    n0 = segs_of([_seg(0, 32, AD1)], ads=[])
    n3 = segs_of([_seg(0, 32, GATED)])
    n3[0].n_adapters = 3
    for c in (segs_of([]), three, n0, n3,
              segs_of([_seg(0, 32, GATED), _seg(32, T + 1, AD1)]),                # row_end > T
              segs_of([_seg(0, 32, GATED, xd=-1), _seg(32, T, AD1)]),             # x rows before row 0
              segs_of([_seg(0, 32, GATED), _seg(32, T, AD1, xd=1)])):             # x rows past T
        refused(fwd(c))
        refused(bwd(c))
    no_t = [dict(par[1], scale=1.0, wdT=None)], [dict(par[1], scale=1.0, wuT=None)]
    for ads in no_t:                                  # the forward does not need the transposed copies, the backward does
        c = segs_of([_seg(0, T, AD1)], ads=ads)
        refused(bwd(c))
    for ts, ads in ((1, AD1), (2, GATED), (-2, GATED)):      # train_slot outside [-1, n_adapters)
        refused(bwd(segs_of([_seg(0, T, ads, ts=ts)])))
    c = segs_of(good)
    refused(lambda: L.adapter_bwd(x, dy, dx, c, T, z_out=z))                       # z_out without dz_out
    refused(lambda: L.adapter_bwd(x, dy, dx, c, T, dz_out=dz))                     # dz_out without z_out
    d8, dsc = torch.zeros(T, H, dtype=torch.uint8, device=DEV), torch.zeros(T, device=DEV)
    refused(lambda: L.adapter_bwd_fp8(dy, dx, d8, dsc, c, T, z_saved=None))        # dx_fp8 without z_saved
