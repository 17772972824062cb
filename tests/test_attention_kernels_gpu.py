"""The attention kernels (csrc/attention.hip, attention_cls.hip, attention2.hip) element by element against float64, in both
operand builds.

Restatement, rounding sites, the per-element bounds and the derivation of their fp32 constants: tests/attention_ref.py (whose
bounds tests/test_attention_bounds_cpu.py shows to hold for an emulation of the roundings and to reject an fp16 build that rounds
P / dS through bf16).  Every forward is compared with the float64 softmax(q k^T / 8 + mask) v of the 16-bit operands it is handed;
every backward is tested AS A FUNCTION OF ITS OWN INPUTS: it is handed the float64 forward's ctx rounded to 16 bits and lse
rounded to fp32, and the restatement uses those, so no forward error is budgeted.  No element is excluded from a comparison.

Inputs (attention_ref.make_heads / key_mask, seeded): unit randn; 'peaked' (scores with a standard deviation of 6: a few keys
dominate each row, most probabilities are subnormal or zero in fp16); 'top' (dctx zero outside token 0, what the top layer sees).
Masks: none, random with key 0 kept, only key 0, the last 16-key tile, the last 32-key slab, a different pattern per sample.

Which case launches which instantiation
  attn_fwd_kernel<NKS>, attn_bwd_kernel<NKS> (both roles), NKS = 1..10: test_vilt_edges at S = 32 NKS - 31, - 16, - 15, 32 NKS
      (and S = 1); the two-role backward is the default above S = 192 and is selected by debug flag 2 below.
  attn_bwd_fused_kernel<NKS>, NKS = 1..6: the same test at S <= 192, grid = one block per pair (few pairs);
      test_vilt_persistent_pairs: grid = n_cu with n_cu - 1, n_cu, n_cu + 1 and 2 n_cu + 3 pairs (ragged last round), against the
      one-block-per-pair launch (debug bit 23) and the two-role kernel; test_vilt_production: 768 and 168 pairs at 12 heads.
  attn_bwd_fused_kernel<NKS, true> (fp8 MX output): test_vilt_fp8mx_relation (NKS 1, 2, 6; the persistent grid at 2 n_cu + 3).
  attn_cls_fwd / attn_cls_bwd: on the data of every test_vilt_edges and test_vilt_production case.
  attn2_fwd_kernel / attn2_bwd_dq_kernel / attn2_bwd_dkv_kernel <QT = 1 | 2, CAUSAL, DROP, MASK>: test_attn2 (QT = 2 on a side
      longer than 64 rows; the mask-free forms where there is no mask, causal or dropout; the short last chunk at 65, 129, 577).

What the paths of attn_bwd give (asserted; common.hip.h and DESIGN.md say the same):
  persistent grid == one block per pair (bit 23), bit for bit: the same kernel, only the walk over the pairs differs;
  fused kernel vs two-role kernel (flag 2): see TWO_ROLE_* below and the docstring of _paths_agree.

Undefined corners, pinned (include/feddat_hip.h states them): any non-zero mask byte attends (bit-identical with 1); a sample
whose keys are all masked is outside the contract of the ViLT kernels (NaN) and of every backward, does not disturb the other
samples of its launch, and attn2_fwd gives it ctx = 0, lse = -inf.

Worst error / bound measured on the MI355X (n_cu = 256; run with -s to see every case's figures), per kernel family and build:
                                         ctx    lse     dQ     dK     dV
  attn_fwd / attn_bwd, edges     bf16   0.74  0.006   0.84   0.96   0.98
                                 f16    0.55  0.006   0.57   0.84   1.00 (0.997: S = 1, where P = 1 and dV = RNE(dO) exactly)
  production shapes              bf16   0.77  0.005   0.80   0.97   0.98
                                 f16    0.47  0.005   0.58   0.84   1.00 (0.997)
  persistent pairs               bf16   0.75  0.005   0.85   0.86   0.89
                                 f16    0.52  0.005   0.68   0.62   0.64
  attn_cls_fwd / attn_cls_bwd    bf16   0.98  0.016   0.97   0.99   0.99
                                 f16    0.87  0.016   0.88   1.00   1.00 (0.999: outputs that are one rounding of an exact value)
  attn2_fwd / attn2_bwd          bf16   0.86  0.013   0.87   0.95   0.98
                                 f16    0.81  0.012   0.72   1.00   1.00 (0.997)
(the one-block-per-pair and two-role launches give the same figures to two digits).  These were measured with C_CLS = 64 and
C_ATTN2(n) = 64 + 28 n; the derivation in attention_ref.py was then completed by the |lse| term of the backward's exponent
(C_CLS = 128, C_ATTN2(n) = 184 + 28 n), which can only lower them.  The CPU module's fp16 emulation with P / dS rounded through
bf16 exceeds the same bounds 1.5 ... 3.2 times on every one of ctx, dV, dK, dQ.
Run time on the same machine: this module 10.9 s with 18 cases per S in test_vilt_edges (since reduced to 6), against
test_adapter_kernels_gpu.py 3.3 s + test_f16_kernels_gpu.py 5.0 s."""
import math

import pytest
import torch

from tests import attention_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMTS = A.FMTS
DT = A.DT
SENT = -31.0          # sentinel of every output buffer (exact in all formats)
G = 3                 # guard rows before and after every output
BIT23 = 1 << 23       # one attention-backward block per (sample, head)
TWO_ROLE = 2          # the two-role backward at S <= 192
# fused vs two-role backward: dK | dV come from the same arithmetic in the same order; dQ is recomputed by role 1 from scores in the
# transposed orientation and a D = sum_d dO O summed in another order (16 products per lane + 2 shuffles against 8 + 3)
TWO_ROLE_DKV_BITEQ = True
TWO_ROLE_DQ_BITEQ = False


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
def n_cu(L):
    c = L.Context(0)
    try:
        return c.info()[1]
    finally:
        c.close()


def _guarded(rows, cols, dtype):
    """A [rows, cols] view with G sentinel rows before and after it."""
    full = torch.full((rows + 2 * G, cols), SENT, dtype=dtype, device=DEV)
    return full, full[G:G + rows]


def _guards_intact(full, rows, what):
    assert bool((full[:G].float() == SENT).all()) and bool((full[G + rows:].float() == SENT).all()), (what, "wrote outside its rows")


def _heads(t, B, S, heads):
    """[B S, heads 64] -> float64 [B, heads, S, 64]"""
    return t.view(B, S, heads, 64).permute(0, 2, 1, 3).double()


def _rows(t, B, S, heads):
    return t.permute(0, 2, 1, 3).reshape(B * S, heads * 64)


def _split(dqkv, B, S, heads):
    """[B S, 3 H] -> float64 [3, B, heads, S, 64]"""
    return dqkv.view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4).double()


class ViltCase:
    """One (shape, family, mask) of the ViLT family: operands, float64 references and bounds (computed in sample chunks)."""

    def __init__(self, fmt, B, S, heads, family, mask_kind, seed):
        self.fmt, self.B, self.S, self.heads, self.H = fmt, B, S, heads, heads * 64
        self.what = f"{fmt} B{B} S{S} h{heads} {family} {mask_kind}"
        dt = DT[fmt]
        q, k, v, do = A.make_heads(fmt, (B, heads), S, S, family, seed, DEV)
        self.mask = A.key_mask(mask_kind, B, S, seed + 1, DEV)
        self.qkv = torch.cat([_rows(t, B, S, heads) for t in (q, k, v)], 1).to(dt).contiguous()
        self.dctx = _rows(do, B, S, heads).to(dt).contiguous()
        gen = torch.Generator(device=DEV).manual_seed(seed + 2)
        self.dctx0 = torch.randn(B, self.H, generator=gen, device=DEV)                 # fp32, attn_cls_bwd's operand
        do0 = self.dctx0.view(B, heads, 1, 64).double()
        nb = max(1, (1 << 25) // (heads * S * S))
        acc = {}

        def put(name, t):
            acc.setdefault(name, []).append(t)
        for b0 in range(0, B, nb):
            sl = slice(b0, min(B, b0 + nb))
            q_, k_, v_, do_ = q[sl], k[sl], v[sl], do[sl]
            allow = torch.ones(1, 1, 1, S, dtype=torch.bool, device=DEV) if self.mask is None else self.mask[sl].bool()[:, None, None, :]
            fr = A.fwd_ref(q_, k_, v_, allow)
            assert float(fr["lse"].abs().max()) <= A.LSE_MAX, (self.what, "inputs outside the range the bound is derived for")
            b_ctx, b_lse = A.fwd_bound(fr, v_, fmt, A.C_VILT)
            ctx16, lse32 = A.r16(fr["ctx"], fmt), A.r32(fr["lse"])
            br = A.bwd_ref(q_, k_, v_, allow, None, ctx16, lse32, do_)
            bq, bk, bv = A.bwd_bound(br, q_, k_, do_, fmt, A.C_VILT)
            for name, t in (("ctx", fr["ctx"]), ("lse", fr["lse"]), ("b_ctx", b_ctx), ("b_lse", b_lse), ("ctx16", ctx16), ("lse32", lse32),
                            ("dQ", br["dQ"]), ("dK", br["dK"]), ("dV", br["dV"]), ("b_dQ", bq), ("b_dK", bk), ("b_dV", bv)):
                put(name, t)
            del fr, br
            # token 0 only (attention_cls.hip): fp32 VALU, P and dS are not rounded
            q0 = q_[:, :, :1]
            f0 = A.fwd_ref(q0, k_, v_, allow)
            c_ctx, c_lse = A.fwd_bound(f0, v_, fmt, A.C_CLS, round_p=False)
            c16, l32 = A.r16(f0["ctx"], fmt), A.r32(f0["lse"])
            b0r = A.bwd_ref(q0, k_, v_, allow, None, c16, l32, do0[sl])
            cq, ck, cv = A.bwd_bound(b0r, q0, k_, do0[sl], fmt, A.C_CLS, round_p=False)
            for name, t in (("c_ctx", f0["ctx"]), ("c_lse", f0["lse"]), ("cb_ctx", c_ctx), ("cb_lse", c_lse), ("c_ctx16", c16),
                            ("c_lse32", l32), ("c_dQ", b0r["dQ"]), ("c_dK", b0r["dK"]), ("c_dV", b0r["dV"]), ("cb_dQ", cq),
                            ("cb_dK", ck), ("cb_dV", cv)):
                put(name, t)
            del f0, b0r
        self.ref = {name: torch.cat(ts, 0) for name, ts in acc.items()}
        r = self.ref
        self.ctx_in = _rows(r["ctx16"], B, S, heads).to(dt).contiguous()               # the backward's given ctx / lse
        self.lse_in = r["lse32"].float().contiguous()
        del q, k, v, do

    # ---- launches (inside `with L.operands(fmt)`), each into guarded sentinel-filled buffers
    def fwd(self, L, qkv=None, mask="same", sl=None):
        B, S, heads, H = (self.B if sl is None else 1), self.S, self.heads, self.H
        qkv = self.qkv if qkv is None else qkv
        mask = self.mask if isinstance(mask, str) else mask
        if sl is not None:
            qkv, mask = qkv[sl * S:(sl + 1) * S], (None if mask is None else mask[sl:sl + 1].contiguous())
        cf, ctx = _guarded(B * S, H, DT[self.fmt])
        lf, lse = _guarded(B * heads, S, torch.float32)
        L.attn_fwd(qkv, ctx, lse.view(B, heads, S), B, S, heads, key_mask=mask)
        torch.cuda.synchronize()
        _guards_intact(cf, B * S, (self.what, "attn_fwd ctx"))
        _guards_intact(lf, B * heads, (self.what, "attn_fwd lse"))
        return ctx, lse.view(B, heads, S)

    def bwd(self, L, qkv=None, mask="same", sl=None, dctx=None, fn=None):
        B, S, heads, H = (self.B if sl is None else 1), self.S, self.heads, self.H
        qkv = self.qkv if qkv is None else qkv
        mask = self.mask if isinstance(mask, str) else mask
        dctx = self.dctx if dctx is None else dctx
        ctx, lse = self.ctx_in, self.lse_in
        if sl is not None:
            rs = slice(sl * S, (sl + 1) * S)
            qkv, dctx, ctx, lse = qkv[rs], dctx[rs], ctx[rs], lse[sl:sl + 1].contiguous()
            mask = None if mask is None else mask[sl:sl + 1].contiguous()
        df, dqkv = _guarded(B * S, 3 * H, DT[self.fmt])
        L.attn_bwd(qkv, ctx, lse, dctx, dqkv, B, S, heads, key_mask=mask)
        torch.cuda.synchronize()
        _guards_intact(df, B * S, (self.what, "attn_bwd dqkv"))
        return dqkv

    def masked_rows_zero(self, dqkv, what):
        if self.mask is None:
            return
        dead = (self.mask == 0).view(-1)
        assert bool((dqkv[dead][:, self.H:].float() == 0).all()), (what, "dK / dV rows of masked keys are not zero")

    def check_fwd(self, L, R):
        ctx, lse = self.fwd(L)
        r = self.ref
        R.check("ctx", _heads(ctx, self.B, self.S, self.heads), r["ctx"], r["b_ctx"], self.what)
        R.check("lse", lse.double(), r["lse"], r["b_lse"], self.what)
        return ctx, lse

    def check_bwd(self, L, R, tag):
        dqkv = self.bwd(L)
        got, r = _split(dqkv, self.B, self.S, self.heads), self.ref
        for i, n in enumerate(("dQ", "dK", "dV")):
            R.check(f"{n}{tag}", got[i], r[n], r["b_" + n], (self.what, tag))
        self.masked_rows_zero(dqkv, (self.what, tag))
        return dqkv

    def cls(self, L, qkv=None, mask="same"):
        """attn_cls_fwd and attn_cls_bwd; the backward's ctx and lse are NaN outside the rows the kernels may read."""
        B, S, heads, H, dt = self.B, self.S, self.heads, self.H, DT[self.fmt]
        qkv = self.qkv if qkv is None else qkv
        mask = self.mask if isinstance(mask, str) else mask
        r = self.ref
        cf, ctx = _guarded(B * S, H, dt)
        lse = torch.full((B, heads, S), SENT, device=DEV)
        L.attn_cls_fwd(qkv, ctx, lse, B, S, heads, key_mask=mask)
        ctx_in = torch.full((B * S, H), float("nan"), dtype=dt, device=DEV)
        ctx_in[::S] = _rows(r["c_ctx16"], B, 1, heads).to(dt)
        lse_in = torch.full((B, heads, S), float("nan"), device=DEV)
        lse_in[:, :, 0] = r["c_lse32"][:, :, 0].float()
        df, dqkv = _guarded(B * S, 3 * H, dt)
        L.attn_cls_bwd(qkv, ctx_in, lse_in, self.dctx0, dqkv, B, S, heads, key_mask=mask)
        torch.cuda.synchronize()
        _guards_intact(cf, B * S, (self.what, "attn_cls_fwd ctx"))
        _guards_intact(df, B * S, (self.what, "attn_cls_bwd dqkv"))
        return ctx, lse, dqkv

    def check_cls(self, L, R):
        B, S, heads, H = self.B, self.S, self.heads, self.H
        ctx, lse, dqkv = self.cls(L)
        r = self.ref
        other = torch.ones(B * S, dtype=torch.bool, device=DEV)
        other[::S] = False
        assert bool((ctx[other].float() == SENT).all()), (self.what, "attn_cls_fwd wrote a ctx row other than token 0")
        assert bool((lse[:, :, 1:] == SENT).all()), (self.what, "attn_cls_fwd wrote an lse entry other than token 0")
        R.check("cls_ctx", _heads(ctx[::S], B, 1, heads), r["c_ctx"], r["cb_ctx"], self.what)
        R.check("cls_lse", lse[:, :, :1].double(), r["c_lse"], r["cb_lse"], self.what)
        got = _split(dqkv, B, S, heads)
        R.check("cls_dQ", got[0][:, :, :1], r["c_dQ"], r["cb_dQ"], self.what)
        assert bool((got[0][:, :, 1:] == 0).all()), (self.what, "attn_cls_bwd: dQ rows other than token 0 are not zero")
        R.check("cls_dK", got[1], r["c_dK"], r["cb_dK"], self.what)
        R.check("cls_dV", got[2], r["c_dV"], r["cb_dV"], self.what)
        self.masked_rows_zero(dqkv, (self.what, "cls"))


def _with_flags(L, flags, fn):
    """fn() with the debug flag word of the CURRENTLY BOUND library set to `flags`, restored afterwards."""
    L.set_debug_flags(flags)
    try:
        return fn()
    finally:
        L.set_debug_flags(0)


def _paths_agree(c, outs, R):
    """outs: {flags: dqkv}.  Persistent grid and one block per pair are the same kernel: bit equality.  The two-role kernel's role 0
    repeats the fused kernel's phase A operation for operation (dK | dV: bit equality); its role 1 recomputes dQ from scores in the
    transposed orientation and its own sum for D (no equality claimed; both are held to the per-element bound)."""
    H = c.H
    if BIT23 in outs:
        assert torch.equal(outs[BIT23], outs[0]), (c.what, "one block per pair != the default launch")
    if TWO_ROLE in outs:
        a, b = outs[TWO_ROLE], outs[0]
        same_kv, same_q = torch.equal(a[:, H:], b[:, H:]), torch.equal(a[:, :H], b[:, :H])
        R.note("two_role_dKV_differs", 0.0 if same_kv else 1.0)
        R.note("two_role_dQ_differs", 0.0 if same_q else 1.0)
        if TWO_ROLE_DKV_BITEQ:
            assert same_kv, (c.what, "two-role dK | dV != fused dK | dV")
        if TWO_ROLE_DQ_BITEQ:
            assert same_q, (c.what, "two-role dQ != fused dQ")


def _paths(S):
    return (0, BIT23, TWO_ROLE) if S <= 192 else (0,)


def _invariants(L, c, ctx, lse, dqkv):
    """Exact properties on one masked case (default paths): two runs, masked K / V rows replaced, a sample launched alone."""
    B, S, heads, H, dt = c.B, c.S, c.heads, c.H, DT[c.fmt]
    ctx2, lse2 = c.fwd(L)
    assert torch.equal(ctx2, ctx) and torch.equal(lse2, lse), (c.what, "two forward runs differ")
    assert torch.equal(c.bwd(L), dqkv), (c.what, "two backward runs differ")
    cls0 = c.cls(L)
    dead = (c.mask == 0).view(-1)
    live = ~dead
    if bool(dead.any()):
        gen = torch.Generator(device=DEV).manual_seed(S)
        alt = c.qkv.clone()
        alt[dead, H:] = (2.0 * torch.randn(int(dead.sum()), 2 * H, generator=gen, device=DEV)).to(dt)
        ctx3, lse3 = c.fwd(L, qkv=alt)
        assert torch.equal(ctx3, ctx) and torch.equal(lse3, lse), (c.what, "the K / V rows of masked keys reach ctx / lse")
        d3 = c.bwd(L, qkv=alt)
        assert torch.equal(d3[:, :H], dqkv[:, :H]) and torch.equal(d3[live], dqkv[live]), (c.what, "the K / V rows of masked keys reach a gradient")
        c.masked_rows_zero(d3, (c.what, "replaced masked rows"))
        cls3 = c.cls(L, qkv=alt)
        assert torch.equal(cls3[0], cls0[0]) and torch.equal(cls3[1], cls0[1]), (c.what, "cls: masked K / V rows reach ctx / lse")
        assert torch.equal(cls3[2][:, :H], cls0[2][:, :H]) and torch.equal(cls3[2][live], cls0[2][live]), (c.what, "cls: masked rows reach a gradient")
    b = B - 1
    ctx1, lse1 = c.fwd(L, sl=b)
    assert torch.equal(ctx1, ctx[b * S:(b + 1) * S]) and torch.equal(lse1[0], lse[b]), (c.what, "a sample alone != inside the batch (fwd)")
    assert torch.equal(c.bwd(L, sl=b), dqkv[b * S:(b + 1) * S]), (c.what, "a sample alone != inside the batch (bwd)")


def _run_vilt(L, cases, paths, R, invariants_on=None):
    fmt = cases[0].fmt
    with L.operands(fmt):
        fw = {}
        for c in cases:
            fw[id(c)] = c.check_fwd(L, R)
            c.check_cls(L, R)
        outs = {id(c): {} for c in cases}
        for flags in paths:
            tag = {0: "", BIT23: "/pair", TWO_ROLE: "/2role"}[flags]

            def go():
                for c in cases:
                    outs[id(c)][flags] = c.check_bwd(L, R, tag)
            _with_flags(L, flags, go)
        for c in cases:
            _paths_agree(c, outs[id(c)], R)
        if invariants_on is not None:
            c = invariants_on
            _invariants(L, c, *fw[id(c)], outs[id(c)][0])


EDGE_S = [32 * n + d for n in range(1, 11) for d in (-31, -16, -15, 0)]          # starts at S = 1


@pytest.mark.parametrize("S", EDGE_S)
@pytest.mark.parametrize("fmt", FMTS)
def test_vilt_edges(L, fmt, S):
    """Every NKS of attn_fwd / attn_bwd (both backward kernels at S <= 192) on its tile edges: every mask pattern, the input family
    rotating with the pattern and with S (each family under two patterns per S, every combination within any three consecutive
    S), the token-0 kernels on the same data, and the exact invariants on the mask-per-sample case."""
    heads = 1 + S % 3
    cases = []
    for i, mask in enumerate(A.MASKS):
        cases.append(ViltCase(fmt, 5 if mask == "per_sample" else 2, S, heads, A.FAMILIES[(i + EDGE_S.index(S)) % 3], mask, 1000 * S + i))
    R = A.Ratios()
    _run_vilt(L, cases, _paths(S), R, invariants_on=cases[A.MASKS.index("per_sample")])
    print(f"\n[attention {fmt} S={S} heads={heads}] worst error / bound: {R.line()}")


@pytest.mark.parametrize("S", (90, 185, 281))
@pytest.mark.parametrize("B", (64, 14))
@pytest.mark.parametrize("fmt", FMTS)
def test_vilt_production(L, fmt, B, S):
    """The production shapes at 12 heads: 2 B = 64 (768 pairs: three full rounds of the persistent backward) and 14 samples."""
    combos = [("randn", "random"), ("top", "tile16"), ("peaked", "slab32")]
    if B == 14:
        combos += [("peaked", "per_sample"), ("randn", "none"), ("top", "only0")]
    R = A.Ratios()
    for i, (family, mask) in enumerate(combos):
        c = ViltCase(fmt, B, S, 12, family, mask, 77 * S + B + i)
        _run_vilt(L, [c], _paths(S), R)
        del c
    print(f"\n[attention {fmt} B={B} S={S} heads=12] worst error / bound: {R.line()}")


@pytest.mark.parametrize("fmt", FMTS)
def test_vilt_persistent_pairs(L, n_cu, fmt):
    """The fused backward's persistent walk with a ragged last round: n_cu - 1 (one block per pair), n_cu, n_cu + 1 and 2 n_cu + 3
    pairs (heads = 1), against the one-block-per-pair launch and the two-role kernel."""
    R = A.Ratios()
    for i, (n, S) in enumerate(((n_cu - 1, 185), (n_cu, 185), (n_cu + 1, 185), (2 * n_cu + 3, 185), (2 * n_cu + 3, 33), (n_cu + 1, 100))):
        c = ViltCase(fmt, n, S, 1, ("randn", "peaked")[i % 2], "per_sample", 31 * n + S)
        _run_vilt(L, [c], _paths(S), R)
        del c
    print(f"\n[attention {fmt} persistent pairs, n_cu = {n_cu}] worst error / bound: {R.line()}")


def _mx_relation(L, c, what):
    """test_ops_gpu.test_attention_bwd_mx_fp8_output's relation between attn_bwd_fp8mx and attn_bwd, on case c."""
    B, S, heads, H = c.B, c.S, c.heads, c.H
    ref = c.bwd(L)
    dq8 = torch.full((B * S, 3 * H), 0x7F, dtype=torch.uint8, device=DEV)
    sc = torch.zeros(B * S, 3 * H // 32, dtype=torch.uint8, device=DEV)
    L.attn_bwd_fp8mx(c.qkv, c.ctx_in, c.lse_in, c.dctx, dq8, sc, B, S, heads, key_mask=c.mask)
    torch.cuda.synchronize()
    scale = torch.exp2(sc.float() - 127.0)
    deq = (dq8.view(torch.float8_e4m3fn).float().view(B * S, -1, 32) * scale[..., None]).view(B * S, 3 * H)
    r32 = ref.float()
    amax = r32.view(B * S, -1, 32).abs().amax(-1)
    assert torch.isfinite(deq).all(), what
    tol = r32.abs() / 16 + (amax * 1e-5)[..., None].expand(-1, -1, 32).reshape(B * S, 3 * H) + 1e-30
    assert bool(((deq - r32).abs() <= tol).all()), (what, float(((deq - r32).abs() / tol).max()))
    nz = amax > 0
    assert bool((scale[nz] * 448.0 >= amax[nz] * 0.999).all()) and bool((scale[nz] * 448.0 < amax[nz] * 2.001).all()), what


@pytest.mark.parametrize("fmt", FMTS)
def test_vilt_fp8mx_relation(L, n_cu, fmt):
    """attn_bwd_fp8mx keeps its relation to attn_bwd at the new mask patterns, at S = 1, 32, 33 and 192, on a ragged persistent
    grid, and refuses S = 193."""
    with L.operands(fmt):
        for S in (1, 32, 33, 192):
            for i, mask in enumerate(A.MASKS):
                c = ViltCase(fmt, 5 if mask == "per_sample" else 2, S, 2, ("randn", "peaked", "top")[i % 3], mask, 500 * S + i)
                _mx_relation(L, c, c.what)
        c = ViltCase(fmt, 2 * n_cu + 3, 33, 1, "randn", "per_sample", 9)
        _mx_relation(L, c, c.what)
        c = ViltCase(fmt, 2, 193, 1, "randn", "none", 10)
        dq8 = torch.zeros(2 * 193, 3 * 64, dtype=torch.uint8, device=DEV)
        sc = torch.zeros(2 * 193, 6, dtype=torch.uint8, device=DEV)
        with pytest.raises(L.FeddatHipError):
            L.attn_bwd_fp8mx(c.qkv, c.ctx_in, c.lse_in, c.dctx, dq8, sc, 2, 193, 1)
        torch.cuda.synchronize()
        assert not bool(dq8.any()) and not bool(sc.any()), "a refused call wrote"


@pytest.mark.parametrize("fmt", FMTS)
def test_vilt_mask_bytes_and_all_masked_sample(L, fmt):
    """Pinned corners of the key mask (include/feddat_hip.h): every non-zero byte attends, bit-identically with 1; a sample whose
    keys are all masked is outside the contract and leaves the other samples of the launch untouched."""
    S, heads = 100, 2
    c = ViltCase(fmt, 3, S, heads, "randn", "random", 5)
    odd = c.mask.clone()
    odd[c.mask != 0] = torch.tensor([2, 255, 128, 1, 7], dtype=torch.uint8, device=DEV).repeat(S)[:int((c.mask != 0).sum())]
    gone = c.mask.clone()
    gone[1] = 0
    S_ = slice(0, S), slice(2 * S, 3 * S)
    with L.operands(fmt):
        ctx, lse = c.fwd(L)
        dqkv = c.bwd(L)
        cls = c.cls(L)
        ctx2, lse2 = c.fwd(L, mask=odd)
        assert torch.equal(ctx2, ctx) and torch.equal(lse2, lse) and torch.equal(c.bwd(L, mask=odd), dqkv)
        assert all(torch.equal(a, b) for a, b in zip(c.cls(L, mask=odd), cls))
        ctx3, lse3 = c.fwd(L, mask=gone)
        d3 = c.bwd(L, mask=gone)
        cls3 = c.cls(L, mask=gone)
        for rows in S_:
            assert torch.equal(ctx3[rows], ctx[rows]) and torch.equal(d3[rows], dqkv[rows])
            assert torch.equal(cls3[0][rows], cls[0][rows]) and torch.equal(cls3[2][rows], cls[2][rows])
        for b in (0, 2):
            assert torch.equal(lse3[b], lse[b]) and torch.equal(cls3[1][b], cls[1][b])


# ====================================================================================================== attention2.hip
class Attn2Case:
    """One launch geometry of the general attention: separate operands, optional key mask / causal / dropout, and either plain
    contiguous operands or the engine's layout: rows_per_sample larger than S with NaN rows between the samples (sentinel rows in
    the outputs) and K | V (dK | dV) as column halves of one wider tensor."""

    def __init__(self, L, fmt, B, Sq, Skv, heads, family, seed, mask=None, causal=False, pdrop=0.0, wide=False):
        self.fmt, self.B, self.Sq, self.Skv, self.heads, self.H = fmt, B, Sq, Skv, heads, heads * 64
        self.causal, self.wide = causal, wide
        self.what = f"{fmt} B{B} {Sq}x{Skv} h{heads} {family} mask={mask} causal={causal} p={pdrop} wide={wide}"
        H, dt = self.H, DT[fmt]
        q, k, v, do = A.make_heads(fmt, (B, heads), Sq, Skv, family, seed, DEV)
        self.qr, self.kr = (Sq + 2, Skv + 3) if wide else (Sq, Skv)
        if mask == "chunk64":                      # the whole last 64-row chunk masked (key 0 kept)
            m = torch.ones(B, Skv, dtype=torch.uint8)
            m[:, 64 * ((Skv - 1) // 64):] = 0
            m[:, 0] = 1
            self.mask = m.to(DEV)
        else:
            self.mask = A.key_mask(mask or "none", B, Skv, seed + 1, DEV)
        allow = torch.ones(B, 1, Sq, Skv, dtype=torch.bool, device=DEV)
        if self.mask is not None:
            allow = allow & self.mask.bool()[:, None, None, :]
        if causal:
            allow = allow & A.causal_allow(Sq, Skv, DEV)
        assert bool(allow.any(-1).all()), "every query needs a key"
        self.drop, mk = None, None
        if pdrop:
            from oracle.albef_oracle import dropout_keep
            k0, k1 = 0x1234567 + seed, 0x89ABCDE
            keep = dropout_keep(B * heads * Sq * Skv, pdrop, k0, k1, 0).view(B, heads, Sq, Skv).to(DEV)
            scale = float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(pdrop)))          # fp32, as the kernel's
            mk = keep.double() * scale
            self.drop = (pdrop, k0, k1, None)
        c32 = A.C_ATTN2(max(Sq, Skv))
        fr = A.fwd_ref(q, k, v, allow, mk)
        assert float(fr["lse"].abs().max()) <= A.LSE_MAX
        b_ctx, b_lse = A.fwd_bound(fr, v, fmt, c32)
        ctx16, lse32 = A.r16(fr["ctx"], fmt), A.r32(fr["lse"])
        br = A.bwd_ref(q, k, v, allow, mk, ctx16, lse32, do)
        bq, bk, bv = A.bwd_bound(br, q, k, do, fmt, c32)
        self.ref = dict(ctx=fr["ctx"], lse=fr["lse"], b_ctx=b_ctx, b_lse=b_lse, dQ=br["dQ"], dK=br["dK"], dV=br["dV"], b_dQ=bq,
                        b_dK=bk, b_dV=bv)
        self.lse_in = lse32.float().contiguous()
        # operands in their layouts
        self.q = self._place(q, self.qr, Sq, 3 * H if wide else H, 0, float("nan"))
        kv = None
        if wide:
            kv = torch.full((B * self.kr, 2 * H), float("nan"), dtype=dt, device=DEV)
        self.k = self._place(k, self.kr, Skv, 2 * H, 0, float("nan"), into=kv)
        self.v = self._place(v, self.kr, Skv, 2 * H, H, float("nan"), into=kv)
        self.do = self._place(do, self.qr, Sq, H + 64 if wide else H, 0, float("nan"))
        self.ctx_in = self._place(ctx16, self.qr, Sq, H + 128 if wide else H, 0, float("nan"))

    def _place(self, t, rps, S, width, col, fill, into=None):
        """[B, heads, S, 64] -> a [B rps, H] view (column offset col of a [B rps, width] tensor when wide)."""
        B, H, dt = self.B, self.H, DT[self.fmt]
        if not self.wide:
            return _rows(t, B, S, self.heads).to(dt).contiguous()
        full = into if into is not None else torch.full((B * rps, width), fill, dtype=dt, device=DEV)
        full.view(B, rps, -1)[:, :S, col:col + H] = t.permute(0, 2, 1, 3).reshape(B, S, H).to(dt)
        return full[:, col:col + H]

    def _out(self, B, rps, width, col):
        full = torch.full((B * rps + 2 * G, width), SENT, dtype=DT[self.fmt], device=DEV)
        return full, full[G:G + B * rps, col:col + self.H]

    def _unplace(self, B, full, views, rps, S, what):
        """The S live rows of every sample of each view as float64 [B, heads, S, 64]; the rest of the allocation still holds SENT."""
        H = self.H
        probe = full.clone()
        out = []
        for view in views:
            c0 = view.storage_offset() % full.shape[1]
            probe[G:G + B * rps].view(B, rps, -1)[:, :S, c0:c0 + H] = SENT
            out.append(view.reshape(B, rps, H)[:, :S].reshape(B, S, self.heads, 64).permute(0, 2, 1, 3).double())
        assert bool((probe.float() == SENT).all()), (self.what, what, "wrote outside its rows / columns")
        return out

    def dead_rows(self):
        """bool over the rows of k / v: the masked keys (never the NaN rows between the samples)."""
        d = torch.zeros(self.B, self.kr, dtype=torch.bool, device=DEV)
        d[:, :self.Skv] = self.mask == 0
        return d.view(-1)

    def run(self, L, k=None, v=None, mask="same", sl=None):
        """Forward, and the backward on the given ctx / lse.  sl = b: sample b launched alone (forms without dropout only: the
        dropout mask is indexed by the sample)."""
        Sq, Skv, heads, H = self.Sq, self.Skv, self.heads, self.H
        q, k, v = self.q, (self.k if k is None else k), (self.v if v is None else v)
        mask = self.mask if isinstance(mask, str) else mask
        ctx_in, lse_in, do, B = self.ctx_in, self.lse_in, self.do, self.B
        if sl is not None:
            assert self.drop is None
            rq, rk = slice(sl * self.qr, (sl + 1) * self.qr), slice(sl * self.kr, (sl + 1) * self.kr)
            q, k, v, ctx_in, do, lse_in, B = q[rq], k[rk], v[rk], ctx_in[rq], do[rq], lse_in[sl:sl + 1].contiguous(), 1
            mask = None if mask is None else mask[sl:sl + 1].contiguous()
        kw = dict(key_mask=mask, causal=self.causal, q_rows=self.qr, kv_rows=self.kr, drop=self.drop)
        wq, wk = (H + 64, 2 * H) if self.wide else (H, H)
        cf, ctx = self._out(B, self.qr, wq, 0)
        lf, lse = _guarded(B * heads, Sq, torch.float32)
        L.attn2_fwd(q, k, v, ctx, lse.view(B, heads, Sq), B, Sq, Skv, heads, **kw)
        qf, dq = self._out(B, self.qr, wq, 64 if self.wide else 0)
        kf, dk = self._out(B, self.kr, wk, 0)
        if self.wide:                              # dK | dV as the column halves of one tensor, as the engine has them
            vf, dv = kf, kf[G:G + B * self.kr, H:]
        else:
            vf, dv = self._out(B, self.kr, wk, 0)
        dsum = torch.full((B, heads, Sq), float("nan"), device=DEV)
        L.attn2_bwd(q, k, v, ctx_in, lse_in, do, dsum, dq, dk, dv, B, Sq, Skv, heads, **kw)
        torch.cuda.synchronize()
        _guards_intact(lf, B * heads, (self.what, "attn2_fwd lse"))
        o = dict(ctx=self._unplace(B, cf, [ctx], self.qr, Sq, "ctx")[0], lse=lse.view(B, heads, Sq).double(),
                 dQ=self._unplace(B, qf, [dq], self.qr, Sq, "dq")[0])
        if self.wide:
            o["dK"], o["dV"] = self._unplace(B, kf, [dk, dv], self.kr, Skv, "dk | dv")
        else:
            o["dK"] = self._unplace(B, kf, [dk], self.kr, Skv, "dk")[0]
            o["dV"] = self._unplace(B, vf, [dv], self.kr, Skv, "dv")[0]
        return o

    def check(self, L, R):
        o, r = self.run(L), self.ref
        for n in ("ctx", "lse", "dQ", "dK", "dV"):
            R.check(n, o[n], r[n], r["b_" + n], self.what)
        if self.mask is not None:
            dead = (self.mask == 0)[:, None, :, None].expand_as(o["dK"])
            assert bool((o["dK"][dead] == 0).all()) and bool((o["dV"][dead] == 0).all()), (self.what, "dK / dV rows of masked keys are not zero")
        return o


ATTN2_SHAPES = [(1, 1), (1, 129), (63, 64), (64, 63), (64, 65), (65, 64), (127, 128), (128, 127), (128, 129), (129, 128), (129, 1),
                (65, 127), (127, 65), (577, 577), (25, 577), (7, 25)]
ATTN2_VARIANTS = [dict(), dict(mask="random"), dict(mask="chunk64"), dict(causal=True), dict(pdrop=0.1),
                  dict(mask="per_sample", causal=True, pdrop=0.1)]


@pytest.mark.parametrize("Sq,Skv", ATTN2_SHAPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_attn2(L, fmt, Sq, Skv):
    """attn2_fwd / attn2_bwd and their dropout forms at the block edges of both sides and the ALBEF shapes: every variant in the
    plain layout and in the engine's (rows_per_sample > S, strided K | V and outputs), B heads blocks not a multiple of 8; plus the
    exact invariants on the masked variant."""
    R = A.Ratios()
    with L.operands(fmt):
        for i, var in enumerate(ATTN2_VARIANTS):
            B, heads = (3, 2) if max(Sq, Skv) > 200 else (5, 3)
            c = Attn2Case(L, fmt, B, Sq, Skv, heads, A.FAMILIES[i % 3], 100 * Sq + Skv + i, wide=bool((i + Sq) % 2), **var)
            o = c.check(L, R)
            if var.get("mask") == "random":
                o2 = c.run(L)
                assert all(torch.equal(o[n], o2[n]) for n in o), (c.what, "two runs differ")
                dead = c.dead_rows()
                if bool(dead.any()):
                    gen = torch.Generator(device=DEV).manual_seed(Sq)
                    k2, v2 = c.k.clone(), c.v.clone()
                    k2[dead] = (2.0 * torch.randn(int(dead.sum()), c.H, generator=gen, device=DEV)).to(DT[fmt])
                    v2[dead] = (2.0 * torch.randn(int(dead.sum()), c.H, generator=gen, device=DEV)).to(DT[fmt])
                    o3 = c.run(L, k=k2, v=v2)
                    assert all(torch.equal(o[n], o3[n]) for n in o), (c.what, "the K / V rows of masked keys reach a result")
                odd = c.mask.clone()
                odd[c.mask != 0] = 200
                o4 = c.run(L, mask=odd)
                assert all(torch.equal(o[n], o4[n]) for n in o), (c.what, "a non-zero mask byte other than 1 changes a result")
            if not var.get("pdrop"):
                b = B - 1
                o1 = c.run(L, sl=b)
                assert all(torch.equal(o[n][b], o1[n][0]) for n in o), (c.what, "a sample alone != inside the batch")
            del c
    print(f"\n[attn2 {fmt} {Sq}x{Skv}] worst error / bound: {R.line()}")


@pytest.mark.parametrize("fmt", FMTS)
def test_attn2_all_masked_sample_forward(L, fmt):
    """A sample whose keys are all masked: attn2_fwd gives it ctx = 0 and lse = -inf (stated in include/feddat_hip.h; its backward
    is outside the contract) and the other samples are untouched."""
    c = Attn2Case(L, fmt, 3, 40, 70, 2, "randn", 3, mask="random")
    gone = c.mask.clone()
    gone[1] = 0
    H, dt = c.H, DT[fmt]
    with L.operands(fmt):
        outs = []
        for m in (c.mask, gone):
            ctx = torch.full((3 * 40, H), SENT, dtype=dt, device=DEV)
            lse = torch.full((3, 2, 40), SENT, device=DEV)
            L.attn2_fwd(c.q, c.k, c.v, ctx, lse, 3, 40, 70, 2, key_mask=m)
            torch.cuda.synchronize()
            outs.append((ctx, lse))
    (ctx, lse), (ctx2, lse2) = outs
    assert bool((ctx2[40:80].float() == 0).all()) and bool((lse2[1] == -math.inf).all())
    for b in (0, 2):
        assert torch.equal(ctx2[40 * b:40 * b + 40], ctx[40 * b:40 * b + 40]) and torch.equal(lse2[b], lse[b])
