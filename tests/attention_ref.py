"""float64 restatement of the attention kernels (csrc/attention.hip, attention_cls.hip, attention2.hip), the per-element error
bounds of their roundings, and a float64 EMULATION of those roundings.  Shared by tests/test_attention_bounds_cpu.py (which
shows that the bounds hold for the emulation and reject an fp16 build that rounds P / dS through bf16) and
tests/test_attention_kernels_gpu.py (which holds the real kernels to the same bounds).  Nothing here runs a kernel.

All tensors are float64 with leading batch dimensions: q [..., Sq, 64], k / v [..., Skv, 64], allow bool [..., Sq, Skv] (key
mask, causal and any combination; every query row must allow at least one key), mk None or float64 [..., Sq, Skv] = the dropout
factor keep / (1 - p) on the probabilities (attention2.hip's _dropout forms).  Scores are q . k / 8 (head_dim 64).

Rounding sites, as the code has them (U, ETA = unit roundoff and half the smallest subnormal step of the build's 16-bit format):
  forward   scores, running / row maximum, exp2, row sum l: fp32.  Only the P operand of the P V product is rounded to 16 bits
            (cvt8), in its UNNORMALISED form p = exp2(s - m) (after the dropout factor where there is one); l sums the
            unrounded p; ctx = (P V) / l is rounded to 16 bits on the way out; lse is fp32.  attention2.hip rounds p relative
            to a LAZY running maximum m (p <= 2^8) and rescales the partial ctx by alpha <= 1 in fp32: the absolute error
            ETA of a subnormal p is divided by an l taken relative to an m that is at most the true maximum, so
            ETA colsum|V| / l (l relative to the true maximum) still covers it.
  backward  a function of (q, k, v, ctx, lse, dctx): P = valid * exp2(s log2e - lse log2e), D = sum_d dO O, dP = dO V^T
            (x the dropout factor), dS = P (dP - D) in fp32; P (x the dropout factor) and dS are rounded to 16 bits before
            the dV = P^T dO, dK = dS^T Q, dQ = dS K products; the 1/8 is applied in fp32 after them (exact); outputs are
            rounded to 16 bits.
  token 0   (attention_cls.hip) fp32 VALU throughout: no 16-bit rounding of P or dS (U_p = ETA_p = 0), only of the outputs.

The fp32 constant (relative error c u32 (1 + |q|.|k| / 8) on each probability and, through sum|terms|, on each product):
  MFMA chains are counted as in test_adapter_kernels_gpu.py: one 16x16x32 MFMA is at most log2(32) + 1 = 6 roundings deep, and
  the count is doubled for an adder that truncates.  VALU operations round to nearest (one u32 each).
  part proportional to |q|.|k| / 8 (the score): 2 chained MFMAs (24), the log2e / 8 factor and its constant (2), the
     subtraction of the maximum or of lse log2e, |s - m| <= 2 |q|.|k| / 8 (2)                                        = 28
  part proportional to 1, dense ViLT kernels: exp2 (4, see Builtins), the row sum of up to 80 sequential adds and 2 shuffles
     (82; its relative error sits on the denominator, the factor 2 in b_ctx adds numerator and denominator), 1 / l and the
     multiplication (3), the P V / P^T dO / dS^T Q / dS K chain of up to NKS = 10 MFMAs (120)                  <= 4 + 82 + 3 + 120 = 209
  The backward kernels form exp2(s log2e - fl(lse log2e)): the rounded product, the constant and the rounded difference put
  2.5 u32 |lse| on the exponent, a term proportional to |lse| and not to |q|.|k| / 8.  The harness asserts |lse| <= LSE_MAX = 40
  on its INPUTS (the peaked family reaches about 30) and the constants carry 3 LSE_MAX = 120:
  C_VILT = 256 >= 130 + 120 (backward: exp2 4 + dP, D and the products 6 + the chain 120) covers every S <= 320 in both directions.
  attention2.hip streams n = ceil(S_streamed / 64) chunks: per chunk 2 chained MFMAs per accumulator (24), a rescale (exp2 and
  a multiplication, 3) and one add to l: C_ATTN2(n) = 184 + 28 n (184 = the score part 28 + exp2 4 + the final 1 / l 3 + products
  6 + 120 for lse, rounded up).
  token-0 kernels (VALU, round to nearest): 8 sequential FMAs + 3 shuffles per dot product and __expf's own rounded x log2e
  product (measured below: 0.75 |x| u32, |x| <= 2 |q|.|k| / 8 in the forward) make a score part of 11 + 2 + 3 = 16; a block
  reduction (6 + 3), at most 10 sequential adds per lane + 3 shuffles + 3 for the V / dQ sums, one division, __expf (3): < 40 in the
  forward; the backward's __expf(s - lse) adds 1.5 |lse| u32 <= 60: < 100.  C_CLS = 128.
  Builtins: v_exp_f32 / v_log_f32 are documented at 1 ulp = 2 u32.  Measured on the MI355X against float64, 2^22 arguments each
  (BUILTIN_MEASURED, in u32): __builtin_amdgcn_exp2f over [-100, 9] (the kernels' arguments: <= 0 in the dense forward, <= 8 with
  attention2's lazy maximum, about 0 +- |lse| in the backward): 1.40, budgeted 4 (> 2 x 1.40); __logf over [1, 2^17] (l <= 320
  resp. 577 x 2^8): 3.02 max(1, |log l|) absolute, i.e. <= 2 x 3.02 x 12 = 73 u32 on an lse, within c u32 (1 + ...) for every c
  here; __expf over [-87, 0] (normal results): 64.6 at x = -86.6 = 0.75 |x|, the rounded x log2e product, counted above.
lse (fp32 in both builds): |lse - ref| <= c u32 (1 + max_j |q|.|k_j| / 8 + |ref|).
fp32 itself flushes below 2^-126: F32_TINY joins every absolute term (it only matters for bf16, whose ETA is 2^-134)."""
import math

import torch

U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
ETA16 = {"bf16": 2.0 ** -134, "f16": 2.0 ** -25}
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
U32 = 2.0 ** -24
F32_TINY = 2.0 ** -126
C_VILT, C_CLS = 256, 128
LSE_MAX = 40.0
FMTS = ("bf16", "f16")
# worst relative error in units of u32 = 2^-24 measured on the MI355X (gfx950) against float64, 2^22 arguments each
BUILTIN_MEASURED = {"exp2f[-100,9]": 1.402, "logf_abs[1,2^17]": 3.022, "expf[-87,0]": 64.561}


def C_ATTN2(s_streamed):
    return 184 + 28 * -(-int(s_streamed) // 64)


def r16(t, fmt):
    """float64 value of the 16-bit round-to-nearest-even of t (through fp32, as the kernels' cvt of an fp32 value)."""
    return t.float().to(DT[fmt]).double()


def r32(t):
    return t.float().double()


def causal_allow(Sq, Skv, device="cpu"):
    """key j <= query i (attention2.hip's causal form: no offset between the two sides)."""
    return torch.arange(Skv, device=device)[None, :] <= torch.arange(Sq, device=device)[:, None]


# ------------------------------------------------------------------------------------------------ restatement
def fwd_ref(q, k, v, allow, mk=None):
    s = (q @ k.transpose(-1, -2)) / 8
    allow = allow.expand(s.shape)
    s = s.masked_fill(~allow, -math.inf)
    mx = s.amax(-1, keepdim=True)
    e = torch.exp(s - mx)
    l = e.sum(-1, keepdim=True)
    P = e / l
    Pd = P if mk is None else P * mk
    asc = (q.abs() @ k.abs().transpose(-1, -2)) / 8
    return dict(P=P, Pd=Pd, l=l, ctx=Pd @ v, lse=(mx + torch.log(l)).squeeze(-1), asc=asc, allow=allow,
                live=allow if mk is None else allow & (mk > 0))


def fwd_bound(ref, v, fmt, c32, round_p=True):
    """(b_ctx, b_lse) per element."""
    U, ETA = U16[fmt], ETA16[fmt] + F32_TINY
    av = v.abs()
    rel = c32 * U32 * (1 + ref["asc"])
    b = 2 * ((ref["Pd"] * rel) @ av) + U * ref["ctx"].abs() + ETA
    if round_p:
        b = b + U * (ref["Pd"] @ av) + ETA * (ref["live"].double() @ av) / ref["l"]
    amax = ref["asc"].masked_fill(~ref["allow"], 0.0).amax(-1)
    return b, c32 * U32 * (1 + amax + ref["lse"].abs())


def bwd_ref(q, k, v, allow, mk, ctx_given, lse_given, do):
    s = (q @ k.transpose(-1, -2)) / 8
    allow = allow.expand(s.shape)
    Pb = torch.where(allow, torch.exp(s - lse_given.unsqueeze(-1)), torch.zeros((), dtype=s.dtype, device=s.device))
    D = (do * ctx_given).sum(-1, keepdim=True)
    dP = do @ v.transpose(-1, -2)
    adP = do.abs() @ v.abs().transpose(-1, -2)
    if mk is not None:
        dP, adP = dP * mk, adP * mk
    dS = Pb * (dP - D)
    Pd = Pb if mk is None else Pb * mk
    asc = (q.abs() @ k.abs().transpose(-1, -2)) / 8
    return dict(Pb=Pb, Pd=Pd, dS=dS, D=D, asc=asc, allow=allow, live=allow if mk is None else allow & (mk > 0),
                adS=Pb * (adP + (do.abs() * ctx_given.abs()).sum(-1, keepdim=True)),
                dV=Pd.transpose(-1, -2) @ do, dK=(dS.transpose(-1, -2) @ q) / 8, dQ=(dS @ k) / 8)


def bwd_bound(ref, q, k, do, fmt, c32, round_p=True):
    """(b_dQ, b_dK, b_dV) per element; the issue's formulae, with every term of a disallowed (query, key) pair zero: the kernels
    multiply those probabilities by an exact 0."""
    U, ETA = U16[fmt], ETA16[fmt] + F32_TINY
    Up, ETAp = (U, ETA) if round_p else (0.0, F32_TINY)
    rel = c32 * U32 * (1 + ref["asc"])
    dS, Pd = ref["dS"], ref["Pd"]
    e_dS = (Up * dS.abs() + ETAp + c32 * U32 * ref["adS"] + dS.abs() * rel) * ref["allow"]
    e_P = (Up * Pd + ETAp + Pd * rel) * ref["live"]
    b_dV = e_P.transpose(-1, -2) @ do.abs() + U * ref["dV"].abs() + ETA
    b_dK = (e_dS.transpose(-1, -2) @ q.abs()) / 8 + U * ref["dK"].abs() + ETA
    b_dQ = (e_dS @ k.abs()) / 8 + U * ref["dQ"].abs() + ETA
    return b_dQ, b_dK, b_dV


# ------------------------------------------------------------------------------------------------ emulation of the roundings
def fwd_emul(q, k, v, allow, mk, fmt, pfmt=None):
    """The forward with the kernels' 16-bit roundings and exact fp32 steps; pfmt: the format P is rounded through (default: fmt)."""
    pfmt = pfmt or fmt
    s = (q @ k.transpose(-1, -2)) / 8
    s = s.masked_fill(~allow.expand(s.shape), -math.inf)
    mx = s.amax(-1, keepdim=True)
    e = torch.exp(s - mx)
    l = e.sum(-1, keepdim=True)
    p = e if mk is None else e * mk
    return r16((r16(p, pfmt) @ v) / l, fmt), r32((mx + torch.log(l)).squeeze(-1))


def bwd_emul(q, k, v, allow, mk, ctx_given, lse_given, do, fmt, pfmt=None):
    pfmt = pfmt or fmt
    ref = bwd_ref(q, k, v, allow, mk, ctx_given, lse_given, do)
    P16, dS16 = r16(ref["Pd"], pfmt), r16(ref["dS"], pfmt)
    return (r16((dS16 @ k) / 8, fmt), r16((dS16.transpose(-1, -2) @ q) / 8, fmt), r16(P16.transpose(-1, -2) @ do, fmt))


# ------------------------------------------------------------------------------------------------ inputs
FAMILIES = ("randn", "peaked", "top")
PEAK = math.sqrt(6.0)          # q, k ~ N(0, 6): the scores q . k / 8 have a standard deviation of 6


def make_heads(fmt, lead, Sq, Skv, family, seed, device="cpu"):
    """q [*lead, Sq, 64], k, v [*lead, Skv, 64], do [*lead, Sq, 64]: float64 values of 16-bit operands.  'peaked': a few keys
    dominate each row and most probabilities are subnormal or zero in fp16; 'top': dctx zero outside query 0."""
    gen = torch.Generator(device=device).manual_seed(seed)

    def rn(*shape):
        return torch.randn(*lead, *shape, generator=gen, device=device)
    q, k, v, do = rn(Sq, 64), rn(Skv, 64), rn(Skv, 64), rn(Sq, 64)
    if family == "peaked":
        q, k = q * PEAK, k * PEAK
    if family == "top":
        do[..., 1:, :] = 0.0
    return tuple(r16(t, fmt) for t in (q, k, v, do))


MASKS = ("none", "random", "only0", "tile16", "slab32", "per_sample")


def key_mask(kind, B, S, seed, device="cpu"):
    """uint8 [B, S] (1 = attend) or None.  Key 0 is always attended.  'tile16' / 'slab32': the last 16-key tile / 32-key slab of
    the kernels' tiling (keys from 16 ((S - 1) // 16) resp. 32 ((S - 1) // 32) on) is masked, what a padded image does;
    'per_sample': sample b takes pattern b mod 5 of the others."""
    if kind == "none":
        return None
    gen = torch.Generator().manual_seed(seed)
    m = torch.ones(B, S, dtype=torch.uint8)
    for b in range(B):
        kd = ("none", "random", "only0", "tile16", "slab32")[b % 5] if kind == "per_sample" else kind
        if kd == "random":
            m[b] = (torch.rand(S, generator=gen) < 0.6).to(torch.uint8)
        elif kd == "only0":
            m[b] = 0
        elif kd == "tile16":
            m[b, 16 * ((S - 1) // 16):] = 0
        elif kd == "slab32":
            m[b, 32 * ((S - 1) // 32):] = 0
    m[:, 0] = 1
    return m.to(device)


class Ratios:
    """Worst error / bound per output."""

    def __init__(self):
        self.r = {}

    def check(self, key, got, ref, bound, what):
        err = (got - ref).abs()
        assert not bool(torch.isnan(err).any()), (what, key, "NaN")
        worst = float((err / bound).max()) if err.numel() else 0.0
        self.r[key] = max(self.r.get(key, 0.0), worst)
        assert worst <= 1.0, (what, key, "error / bound", worst)

    def note(self, key, v):
        self.r[key] = max(self.r.get(key, 0.0), float(v))

    def merge(self, other):
        for k, v in other.r.items():
            self.note(k, v)

    def line(self):
        return " ".join(f"{k} {v:.3g}" for k, v in sorted(self.r.items()))
