"""Cases, float64 reference and derived error bounds for feddat_head_gemm (feddat_amd/csrc/head_tail.hip: ht_gemm_kernel), shared
by tests/test_head_gemm_kernels_gpu.py (runs them) and tests/test_head_gemm_plan_cpu.py (pins the path each one takes).  Plain
torch on the CPU; nothing here touches a device.

A case is a Spec: sizes, the LAYOUT of each operand (which is what selects the load path: an operand contiguous along k, with
K % 4 == 0, a row stride % 4 == 0 and a 16-byte-aligned base is fetched with 16-byte loads, every other one with dword loads),
prologue / epilogue and the optional outputs.  `want` is the (avec, bvec, jt) the case is there to exercise; the GPU test asserts
it against feddat_head_gemm_plan before it launches.

The bound (all in float64, u = 2^-24, the unit roundoff of fp32)
----------------------------------------------------------------
With a' = pro(A) computed in float64 from the same fp32 inputs, lin = alpha sum_k a'[i,k] b[k,j] + bias[j] and
S = sum_k mag(a')[i,k] |b[k,j]|:

    |lin_kernel - lin| <= 2 (D + c) u |alpha| S + u |bias[j]| + (LayerNorm only) the statistics' term below.

D is the number of fp32 additions one product a' b can pass through, in the order include/feddat_hip.h documents:
  mode 0: the wave that owns a 16-deep k-chunk feeds it to four v_mfma_f32_16x16x4_f32 (each adds its four-k sum onto the
          accumulator: 1 addition per instruction at the accumulator, and the four-term sum inside it: 3), a wave owns
          ceil(ceil(K / 16) / 8) chunks, and the eight waves' accumulators are then added in wave order (7):
          D = 4 ceil(ceil(K / 16) / 8) + 3 + 7;
  mode 1: one wave runs the whole K: ceil(K / 4) instructions and the in-instruction sum: D = ceil(K / 4) + 3.
c counts the roundings outside the sum: alpha * acc (1; alpha * *alpha_dev is exact for the powers of two it holds), + bias (1,
relative to the result, hence also the u |bias| term), and the prologue's roundings of a' itself, C_PRO below.  The factor 2 is
headroom for the MFMA unit's internal rounding of its four-term sum, which the hardware guides do not specify (an exact four-term
sum rounded once would need no headroom; four sequentially rounded additions are what D already counts).
mag(a') is |a'| without a prologue and an upper bound of it built from the terms that are rounded where there is one:
  LayerNorm: a' = (x - m) r g + b: three roundings relative to |(x - m) r g| and one relative to |a'| <= |(x - m) r g| + |b|:
             mag = |(x - m) r g| + |b|, C_PRO = 4;
  tanh':     a' = a (1 - y^2): y^2 (1), 1 - y^2 (1, relative to at most 1 + y^2), the product (1): mag = |a| (1 + y^2), C_PRO = 3.

LayerNorm statistics (ht_body: a lane adds the 4 values of each of its ceil(K / 256) 16-byte chunks, six butterfly levels add the
64 lanes, one division): every x passes through at most d_sum = 4 ceil(K / 256) + 6 additions, so
    |m_kernel - m| <= dm = (d_sum + 1) u mean|x|                                                     (mean|x| = sum|x| / K).
The variance is the two-pass one about the kernel's own mean m~: sum (x - m~)^2 / K = var + (m~ - m)^2 exactly, each (x - m~)
rounded once (relative u), squared (2 u + u), summed (d_sum), divided (1), + eps (1); rsqrtf within 2 ulp:
    |r_kernel / r - 1| <= er = (3 + d_sum + 2) u / 2 + 2 u + (dm r)^2 / 2.
A one-pass variance (E x^2 - m^2) of x + 1000 is wrong by about 10^6 u / var, i.e. several per cent of r: far outside er.
Through a' these move lin by at most  |alpha| r dm |sum_k g[k] b[k,j]|  (the SAME shift of every x - m in the row, so it enters
through the signed sum)  +  |alpha| er sum_k |(x - m) r g[k]| |b[k,j]|.

Epilogues, on top of the bound L of lin:
  TANH:       |tanh'| <= 1 - tanh^2(max(|lin| - L, 0)) on the interval (mean value theorem), tanhf within 2 ulp + the interval's
              own rounding: L (1 - tanh^2(...)) + 3 u |tanh(lin)|;
  MUL_DGELU:  out = lin g'(aux): |g'| L + |lin| dg + u |out|, where dg = 1.1e-6 bounds the kernel's gelu'(aux) (common.hip.h:
              erf by Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7, evaluated in at most 20 fp32 roundings of quantities <= 1.5:
              20 * 1.5 u = 1.8e-6, both halved by the factor 1/2 of gelu', plus 4 roundings of aux phi(aux) <= 0.25).
colsum[i] = alpha sum_k a'[i,k] is summed on the VALU in the same split: at most D_cs = (mode 0: 4 ceil(ceil(K / 16) / 8) + 2 + 7,
mode 1: 4 ceil(K / 16) + 2) additions: (D_cs + 1 + C_PRO) u |alpha| sum_k mag(a') + the statistics' term with b = 1.
"""
import dataclasses
import math
import zlib
from typing import Optional, Tuple

import torch

U = 2.0 ** -24
PRO_NONE, PRO_LN, PRO_TANH_BWD = 0, 1, 2
EPI_NONE, EPI_TANH, EPI_MUL_DGELU = 0, 1, 2
C_PRO = {PRO_NONE: 0, PRO_LN: 4, PRO_TANH_BWD: 3}
DG = 1.1e-6
BASE = 0x7F0000000000          # made-up device addresses for the CPU plan test: 256-byte aligned, 1 GiB apart


@dataclasses.dataclass(frozen=True)
class Spec:
    name: str
    I: int
    J: int
    K: int
    want: Tuple[int, int, int]            # (avec, bvec, jt) the case is there to exercise
    mode: int = 0
    a_lay: str = "k"                      # "k": A[i, k] at i * (K + sa_pad) + k;  "i": at k * (I + sa_pad) + i
    b_lay: str = "k"                      # "k": B[k, j] at j * (K + sb_pad) + k;  "j": at k * (J + sb_pad) + j
    sa_pad: int = 0
    sb_pad: int = 0
    a_off: int = 0                        # floats between the (256-byte aligned) allocation and the operand's base
    b_off: int = 0
    y_off: int = 0
    pro: int = PRO_NONE
    epi: int = EPI_NONE
    bias: bool = False
    alpha: float = 1.0
    alpha_dev: Optional[float] = None
    colsum: bool = False
    stats: bool = False
    ldo_pad: int = 0
    aux_pad: int = 0
    eps: float = 1e-12
    x_shift: float = 0.0                  # LayerNorm input x + x_shift
    bias_span: float = 0.0                # bias = linspace(-span, span): pre-activations out to +- span
    aux_span: float = 0.0                 # aux = linspace(-span, span) shuffled
    data: Optional[str] = None            # draw the operands of this other case (same logical values, another layout)
    rows: Optional[int] = None            # ... and keep its first `rows` rows only

    @property
    def path(self):
        return self.want + (self.mode, self.pro, self.epi)


def geometry(s: Spec) -> dict:
    """Element strides and allocation sizes of the operands (what the layouts mean)."""
    if s.a_lay == "k":
        sa_i, sa_k, a_elems = s.K + s.sa_pad, 1, s.I * (s.K + s.sa_pad)
    else:
        sa_i, sa_k, a_elems = 1, s.I + s.sa_pad, s.K * (s.I + s.sa_pad)
    if s.b_lay == "k":
        sb_k, sb_j, b_elems = 1, s.K + s.sb_pad, s.J * (s.K + s.sb_pad)
    else:
        sb_k, sb_j, b_elems = s.J + s.sb_pad, 1, s.K * (s.J + s.sb_pad)
    return dict(sa_i=sa_i, sa_k=sa_k, a_elems=a_elems, sb_k=sb_k, sb_j=sb_j, b_elems=b_elems, ldo=s.J + s.ldo_pad,
                ld_aux=s.J + s.aux_pad)


def fill_job(lib, s: Spec, ptr: dict):
    """The feddat_ht_job of a case; ptr maps A, B, out, bias_j, colsum, pro_a, pro_b, stats_out, aux, alpha_dev to addresses of
    the (aligned) allocations -- the operand offsets of the Spec are added here."""
    g = geometry(s)
    j = lib.HtJob()
    j.A, j.sa_i, j.sa_k = ptr["A"] + 4 * s.a_off, g["sa_i"], g["sa_k"]
    j.B, j.sb_k, j.sb_j = ptr["B"] + 4 * s.b_off, g["sb_k"], g["sb_j"]
    j.I, j.J, j.K, j.mode, j.alpha = s.I, s.J, s.K, s.mode, s.alpha
    j.out, j.ldo = ptr["out"], g["ldo"]
    j.bias_j = ptr["bias_j"] if s.bias else None
    j.colsum = ptr["colsum"] if s.colsum else None
    j.pro, j.pro_eps = s.pro, (s.eps if s.pro == PRO_LN else 0.0)
    j.pro_a = ptr["pro_a"] + 4 * s.y_off if s.pro != PRO_NONE else None
    j.pro_b = ptr["pro_b"] if s.pro == PRO_LN else None
    j.stats_out = ptr["stats_out"] if s.stats else None
    j.epi = s.epi
    j.aux, j.ld_aux = (ptr["aux"], g["ld_aux"]) if s.epi == EPI_MUL_DGELU else (None, 0)
    j.alpha_dev = ptr["alpha_dev"] if s.alpha_dev is not None else None
    return j


FAKE_PTRS = {n: BASE + (k << 30) for k, n in enumerate(("A", "B", "out", "bias_j", "colsum", "pro_a", "pro_b", "stats_out", "aux",
                                                        "alpha_dev"))}


def fake_job(lib, s: Spec):
    """The job of a case at made-up addresses (feddat_head_gemm_plan dereferences nothing)."""
    return fill_job(lib, s, FAKE_PTRS)


# ------------------------------------------------------------------------------------------------ the cases
def _load_paths():
    """a. the four (avec, bvec) combinations at mode 0 / jt 1 (48 x 1000: 3 x 16 = 48 tiles), mode 0 / jt 4 (49 x 1000: 4 x 16 =
    64 tiles, ragged both ways) and mode 1, chosen by layout.  K = 20: K % 16 != 0 and seven of the eight waves get no chunk;
    K = 388 = 384 + 4: one full three-deep round for all eight waves and one more chunk.  Dword paths also at K = 3 and at
    K = 37 with BOTH operands contiguous along k (the K % 4 != 0 reason for dword loads)."""
    out = []
    for cfg, I, mode, jt in (("m0jt1", 48, 0, 1), ("m0jt4", 49, 0, 4), ("m1", 49, 1, 4)):
        for av, bv in ((1, 1), (1, 0), (0, 1), (0, 0)):
            for K in ((20, 388) if av or bv else (3, 20, 37, 388)):
                lay = ("k", "k") if K == 37 else ("k" if av else "i", "k" if bv else "j")
                out.append(Spec(f"a_{cfg}_a{av}b{bv}_k{K}", I, 1000, K, (av, bv, jt), mode=mode, a_lay=lay[0], b_lay=lay[1]))
    return out


def _fallbacks():
    """b. the data of an (avec, bvec) = (1, 1) case through a copy whose A or B base is one float off 16-byte alignment: the plan
    flips that operand to dword loads, and the result is bit-identical (the k order does not depend on the load width).  Also a
    row stride with sa_i % 4 != 0 / sb_j % 4 != 0, and tanh' with only pro_a misaligned (section e)."""
    out = []
    for cfg, jt in (("m0jt1", 1), ("m0jt4", 4), ("m1", 4)):
        base = f"a_{cfg}_a1b1_k388"
        I, mode = (48 if cfg == "m0jt1" else 49), (1 if cfg == "m1" else 0)
        out.append(Spec(f"b_{cfg}_Aoff", I, 1000, 388, (0, 1, jt), mode=mode, a_off=1, data=base))
        out.append(Spec(f"b_{cfg}_Boff", I, 1000, 388, (1, 0, jt), mode=mode, b_off=1, data=base))
    out.append(Spec("b_m0jt4_Astride", 49, 1000, 388, (0, 1, 4), sa_pad=1, data="a_m0jt4_a1b1_k388"))
    out.append(Spec("b_m0jt4_Bstride", 49, 1000, 388, (1, 0, 4), sb_pad=2, data="a_m0jt4_a1b1_k388"))
    return out


FALLBACK_PAIRS = [(f"a_{c}_a1b1_k388", f"b_{c}_{w}") for c in ("m0jt1", "m0jt4", "m1") for w in ("Aoff", "Boff")] + \
                 [("a_m0jt4_a1b1_k388", "b_m0jt4_Astride"), ("a_m0jt4_a1b1_k388", "b_m0jt4_Bstride")]

# c. rows 0..15 of the jt == 4 case as their own job: 1 x 16 = 16 tiles, so jt == 1; bit-identical to those rows of the full run
JT_IDENTITY = [(f"a_m0jt4_a{av}b{bv}_k388", f"c_rows16_a{av}b{bv}") for av, bv in ((1, 1), (0, 0))]


def _jt_identity():
    return [Spec(f"c_rows16_a{av}b{bv}", 16, 1000, 388, (av, bv, 1), a_lay="k" if av else "i", b_lay="k" if bv else "j",
                 data=f"a_m0jt4_a{av}b{bv}_k388", rows=16) for av, bv in ((1, 1), (0, 0))]


def _layernorm():
    """d. K in {4, 772, 2048} (2048 = 8 x 64 x 4, the register-resident limit), rows strided like the token-0 rows (sa_i > K),
    I in {1, 17, 64} (ragged I: the rows >= I of a tile have no statistics), B on both load paths, jt 1 and 4, both modes (mode 1
    at J = 1000: two column blocks per row tile compute the statistics, only jb == 0 writes them), stats_out written and omitted,
    colsum, and x + 1000.  The shifted input is at K = 4: the kernel's mean of a row near 1000 is off by up to dm ~ 10^-3 (fp32 can do
    no better), every a' of the row moves with it, and at K = 772 that term of the bound is as large as one k-slice of the
    product -- the bound would no longer notice a missing slice (the CPU self-check).  The one-pass variance it is there to catch
    is wrong at any K.  Mode 1 runs the LayerNorm at K = 4 and 772 only: its D grows with K / 4, and at K = 2048 the bound is
    again wider than a slice."""
    LN = dict(pro=PRO_LN, bias=True)
    return [
        Spec("d_k772_i64_bv_jt4_stats", 64, 1000, 772, (1, 1, 4), sa_pad=2 * 772 + 4, stats=True, colsum=True, **LN),
        Spec("d_k2048_i17_bd_jt1", 17, 100, 2048, (1, 0, 1), sa_pad=8, b_lay="j", colsum=True, **LN),
        Spec("d_k4_i1_bv_jt1_stats", 1, 40, 4, (1, 1, 1), sa_pad=12, stats=True, colsum=True, **LN),
        Spec("d_k4_i17_bd_jt4_stats", 17, 2000, 4, (1, 0, 4), sa_pad=4, b_lay="j", stats=True, **LN),
        Spec("d_k772_i17_bv_m1_stats", 17, 1000, 772, (1, 1, 4), mode=1, sa_pad=772, stats=True, colsum=True, **LN),
        Spec("d_k4_i64_bd_m1", 64, 200, 4, (1, 0, 4), mode=1, sa_pad=4, b_lay="j", colsum=True, **LN),
        Spec("d_k2048_i1_bv_jt1_stats", 1, 100, 2048, (1, 1, 1), stats=True, eps=1e-5, **LN),
        Spec("d_k4_i17_shift1000", 17, 100, 4, (1, 1, 1), sa_pad=8, stats=True, colsum=True, x_shift=1000.0, **LN),
        Spec("d_k4_i17_shift1000_m1", 17, 100, 4, (1, 0, 4), mode=1, sa_pad=4, b_lay="j", stats=True, colsum=True, x_shift=1000.0,
             **LN),
    ]


def _tanh_bwd():
    """e. the tanh' prologue on the vector and the dword path, both modes, with colsum, alpha = 0.37 and *alpha_dev = 2^-3 / 2^5; and
    the fallback of a misaligned pro_a (A itself aligned)."""
    T = dict(pro=PRO_TANH_BWD, colsum=True, alpha=0.37)
    return [
        Spec("e_vec_m0jt4", 49, 1000, 388, (1, 0, 4), b_lay="j", alpha_dev=2.0 ** -3, **T),
        Spec("e_vec_m0jt1", 48, 100, 20, (1, 1, 1), alpha_dev=2.0 ** 5, **T),
        Spec("e_dw_m0jt1", 48, 100, 37, (0, 0, 1), a_lay="i", b_lay="j", alpha_dev=2.0 ** 5, **T),
        Spec("e_dw_m0jt4", 49, 1000, 20, (0, 1, 4), a_lay="i", alpha_dev=2.0 ** -3, **T),
        Spec("e_vec_m1", 49, 200, 20, (1, 0, 4), mode=1, b_lay="j", alpha_dev=2.0 ** -3, **T),
        Spec("e_dw_m1", 49, 200, 37, (0, 0, 4), mode=1, a_lay="i", b_lay="j", alpha_dev=2.0 ** 5, **T),
        Spec("e_yoff_m0jt4", 49, 1000, 388, (0, 0, 4), b_lay="j", y_off=1, alpha_dev=2.0 ** -3, data="e_vec_m0jt4", **T),
        Spec("e_yoff_m1", 49, 200, 20, (0, 0, 4), mode=1, b_lay="j", y_off=1, alpha_dev=2.0 ** -3, data="e_vec_m1", **T),
    ]


def _epilogues():
    """f. TANH with a bias that takes the pre-activations out to +-12; MUL_DGELU with ld_aux > J and aux out to +-6; ldo > J on both;
    alpha not a power of two next to the bias (which must not be scaled); each at jt 1 and 4, and in mode 1."""
    return [
        Spec("f_tanh_jt1", 17, 100, 100, (1, 1, 1), epi=EPI_TANH, bias=True, bias_span=12.0, ldo_pad=7, alpha=0.37),
        Spec("f_tanh_jt4", 49, 1000, 20, (0, 0, 4), a_lay="i", b_lay="j", epi=EPI_TANH, bias=True, bias_span=12.0, ldo_pad=24,
             alpha=1.7),
        Spec("f_tanh_m1", 20, 130, 12, (1, 1, 4), mode=1, epi=EPI_TANH, bias=True, bias_span=3.0, ldo_pad=2, alpha=0.37),
        Spec("f_dgelu_jt1", 17, 100, 37, (0, 0, 1), a_lay="i", b_lay="j", epi=EPI_MUL_DGELU, bias=True, aux_span=6.0, aux_pad=5,
             ldo_pad=3, alpha=1.7),
        Spec("f_dgelu_jt4", 64, 1000, 100, (1, 0, 4), b_lay="j", epi=EPI_MUL_DGELU, bias=True, aux_span=6.0, aux_pad=8, ldo_pad=8,
             alpha=0.37),
        Spec("f_dgelu_m1", 20, 130, 12, (0, 1, 4), mode=1, a_lay="i", epi=EPI_MUL_DGELU, aux_span=6.0, aux_pad=1, ldo_pad=5),
        Spec("f_bias_alpha_jt1", 23, 50, 20, (1, 1, 1), bias=True, alpha=0.37, ldo_pad=1),
    ]


def _colsum_mode0():
    """g. colsum in mode 0 over several column blocks (only jb == 0 may write) with ragged I, at both jt; and with ONE column
    block (J = 16), where no other block could write the same sums in its place."""
    return [
        Spec("g_cs_one_block", 23, 16, 37, (0, 0, 1), a_lay="i", b_lay="j", colsum=True),
        Spec("g_cs_jt1", 23, 200, 388, (1, 1, 1), colsum=True),
        Spec("g_cs_jt1_dw", 23, 200, 37, (0, 0, 1), a_lay="i", b_lay="j", colsum=True, alpha=0.37),
        Spec("g_cs_jt4", 49, 1000, 20, (1, 0, 4), b_lay="j", colsum=True),
    ]


def _step_products(B=64, H=768, C=100):
    """j. the products of a train step at B = 64, H = 768, C = 100, as the engines call them (the L.ht_job sites of
    vilt_backbone.py and engine.py / vector_engine.py): the pooler (token-0 rows at stride 5 H here: the stride only has to exceed
    K), fc0, fc1, the two backward pairs, and d(pooler input)."""
    return [
        Spec("j_pool", B, H, H, (1, 1, 1), sa_pad=4 * H, pro=PRO_LN, bias=True, stats=True, epi=EPI_TANH),
        Spec("j_fc0", B, 2 * H, H, (1, 1, 4), bias=True),
        Spec("j_fc1", B, C, 2 * H, (1, 1, 1), bias=True),
        Spec("j_dW_fc1", C, 2 * H, B, (0, 0, 4), mode=1, a_lay="i", b_lay="j", colsum=True),
        Spec("j_dn0", B, 2 * H, C, (1, 0, 4), b_lay="j", epi=EPI_MUL_DGELU, aux_span=4.0),
        Spec("j_dW_fc0", 2 * H, H, B, (0, 0, 4), mode=1, a_lay="i", b_lay="j", colsum=True),
        Spec("j_dpooled", B, H, 2 * H, (1, 0, 1), b_lay="j"),
        Spec("j_dcls", B, H, H, (1, 0, 1), b_lay="j", pro=PRO_TANH_BWD, alpha=1.0, alpha_dev=2.0 ** 7),
    ]


def _refusal_bases():
    """i. the good jobs the refusals are made from by changing ONE field (so the change alone is what is refused)."""
    return [
        Spec("i_plain", 17, 40, 20, (1, 1, 1), bias=True, colsum=True),
        Spec("i_ln", 17, 40, 20, (1, 1, 1), sa_pad=4, pro=PRO_LN, stats=True, colsum=True),
        Spec("i_tb", 17, 40, 20, (1, 1, 1), pro=PRO_TANH_BWD),
        Spec("i_dg", 17, 40, 20, (1, 1, 1), epi=EPI_MUL_DGELU, aux_span=2.0, aux_pad=2),
    ]


def _set(**kw):
    def f(j):
        for k, v in kw.items():
            setattr(j, k, v)
    return f


def _bump(field):                 # that pointer 4 bytes further: off 16-byte alignment
    def f(j):
        setattr(j, field, getattr(j, field) + 4)
    return f


# (name, the good job's case, the one change that must be refused)
REFUSALS = [
    ("I_0", "i_plain", _set(I=0)), ("J_0", "i_plain", _set(J=0)), ("K_0", "i_plain", _set(K=0)),
    ("I_negative", "i_plain", _set(I=-16)),
    ("A_null", "i_plain", _set(A=None)), ("B_null", "i_plain", _set(B=None)), ("out_null", "i_plain", _set(out=None)),
    ("ldo_lt_J", "i_plain", _set(ldo=39)), ("mode_2", "i_plain", _set(mode=2)), ("mode_negative", "i_plain", _set(mode=-1)),
    ("pro_3", "i_plain", _set(pro=3)), ("pro_negative", "i_plain", _set(pro=-1)),
    ("epi_3", "i_plain", _set(epi=3)), ("epi_negative", "i_plain", _set(epi=-1)),
    ("ln_K_mod_4", "i_ln", _set(K=18)), ("ln_K_gt_2048", "i_ln", _set(K=2052)), ("ln_sa_k_2", "i_ln", _set(sa_k=2)),
    ("ln_sa_i_mod_4", "i_ln", _set(sa_i=26)), ("ln_eps_0", "i_ln", _set(pro_eps=0.0)), ("ln_eps_negative", "i_ln", _set(pro_eps=-1e-5)),
    ("ln_A_misaligned", "i_ln", _bump("A")), ("ln_gamma_misaligned", "i_ln", _bump("pro_a")),
    ("ln_beta_misaligned", "i_ln", _bump("pro_b")), ("ln_gamma_null", "i_ln", _set(pro_a=None)),
    ("ln_beta_null", "i_ln", _set(pro_b=None)),
    ("tanh_bwd_y_null", "i_tb", _set(pro_a=None)),
    ("dgelu_aux_null", "i_dg", _set(aux=None)), ("dgelu_ld_aux_lt_J", "i_dg", _set(ld_aux=39)),
]

CASES = (_load_paths() + _fallbacks() + _jt_identity() + _layernorm() + _tanh_bwd() + _epilogues() + _colsum_mode0() +
         _step_products() + _refusal_bases())
CASE = {s.name: s for s in CASES}
assert len(CASE) == len(CASES)

# h. two jobs in one launch: pairs that instantiate different templates, run in both orders; each output bit-identical to the job alone
TWO_JOB_PAIRS = [
    ("d_k772_i17_bv_m1_stats", "a_m0jt1_a0b0_k37"),        # LN (mode 1, vector) | no prologue (mode 0, dword, jt 1)
    ("a_m1_a1b0_k20", "a_m0jt4_a0b1_k388"),                # mode 1 | mode 0, other load paths
    ("a_m0jt4_a1b1_k388", "f_tanh_jt1"),                   # jt 4 | jt 1 (with an epilogue)
    ("d_k2048_i17_bd_jt1", "e_dw_m0jt4"),                  # LN jt 1 | tanh' jt 4
    ("j_dW_fc1", "j_dn0"), ("j_dW_fc0", "j_dpooled"),      # the step's own pairs
]


# k. an infinite B element: the k slots past K (and the chunks past the last one) fetch a clamped, VALID element of B -- element 0 of
# the column on the 16-byte path, element K - 1 on the dword path -- and drop it by a select on BOTH operands; 0 * inf would turn
# the column's +-inf into NaN.  Cases whose K leaves such slots, on each load path of B and in both modes.
INF_B_CASES = ["a_m0jt1_a1b1_k20", "a_m0jt4_a0b1_k20", "a_m0jt4_a0b0_k37", "a_m0jt1_a1b0_k20", "a_m1_a1b1_k20", "a_m1_a0b0_k37"]
INF_B_COLS = (5, 998)            # B[0, 5] = +inf, B[K - 1, 998] = -inf


# ------------------------------------------------------------------------------------------------ operands
def operands(s: Spec) -> dict:
    """fp32 CPU operands of a case in LOGICAL shape (A [I, K], B [K, J], ...): A ~ N(0, 1), B ~ 0.05 N(0, 1).  With operands of
    this kind the float32 restatement uses a small part of the bound and a missing k-slice leaves it (the CPU self-check)."""
    if s.data is not None:
        o = dict(operands(CASE[s.data]))
        if s.rows is not None:
            for n in ("A", "y", "aux"):
                if o.get(n) is not None:
                    o[n] = o[n][:s.rows].contiguous()
        return o
    g = torch.Generator().manual_seed(zlib.crc32(s.name.encode()))
    o = {"A": torch.randn(s.I, s.K, generator=g) + s.x_shift, "B": 0.05 * torch.randn(s.K, s.J, generator=g)}
    o["y"] = torch.tanh(0.5 * torch.randn(s.I, s.K, generator=g)) if s.pro == PRO_TANH_BWD else None
    o["gamma"] = 1 + 0.1 * torch.randn(s.K, generator=g) if s.pro == PRO_LN else None
    o["beta"] = 0.1 * torch.randn(s.K, generator=g) if s.pro == PRO_LN else None
    if s.bias:
        o["bias"] = torch.linspace(-s.bias_span, s.bias_span, s.J) if s.bias_span else torch.randn(s.J, generator=g)
    else:
        o["bias"] = None
    if s.epi == EPI_MUL_DGELU:
        flat = torch.linspace(-s.aux_span, s.aux_span, s.I * s.J)
        o["aux"] = flat[torch.randperm(s.I * s.J, generator=g)].reshape(s.I, s.J).contiguous()
    else:
        o["aux"] = None
    return o


def alpha_of(s: Spec) -> float:
    """The fp32 factor the kernel multiplies by: float(alpha) * *alpha_dev (exact: alpha_dev holds a power of two)."""
    a = float(torch.tensor(s.alpha, dtype=torch.float32))
    return a * (s.alpha_dev if s.alpha_dev is not None else 1.0)


def depth(s: Spec) -> int:
    nchunk = -(-s.K // 16)
    return 4 * (-(-nchunk // 8)) + 3 + 7 if s.mode == 0 else -(-s.K // 4) + 3


def depth_colsum(s: Spec) -> int:
    nchunk = -(-s.K // 16)
    return 4 * (-(-nchunk // 8)) + 2 + 7 if s.mode == 0 else 4 * nchunk + 2


def _gelu_grad(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def reference(s: Spec, o: dict, drop_k: Optional[int] = None) -> dict:
    """float64 restatement of the header's formula and the bounds of the module docstring.  drop_k: leave that k out of the
    product (the CPU self-check's wrong answer); the bounds are those of the full product."""
    A, Bm = o["A"].double(), o["B"].double()
    alpha = alpha_of(s)
    r = {}
    shift = None                                                   # LayerNorm: (statistics' term per unit of b, per row)
    if s.pro == PRO_LN:
        g, b = o["gamma"].double(), o["beta"].double()
        m = A.mean(1, keepdim=True)
        var = ((A - m) ** 2).mean(1, keepdim=True)
        rs = 1 / torch.sqrt(var + float(torch.tensor(s.eps, dtype=torch.float32)))
        xh = (A - m) * rs * g
        ap, mag = xh + b, xh.abs() + b.abs()
        d_sum = 4 * (-(-s.K // 256)) + 6
        dm = (d_sum + 1) * U * A.abs().mean(1, keepdim=True)
        er = (3 + d_sum + 2) * U / 2 + 2 * U + (dm * rs) ** 2 / 2
        r.update(stats=torch.cat([m, rs], 1), mean_bound=dm[:, 0], rstd_rel_bound=er[:, 0])
        shift = (rs * dm, g, er, xh.abs())
    elif s.pro == PRO_TANH_BWD:
        y = o["y"].double()
        ap, mag = A * (1 - y * y), A.abs() * (1 + y * y)
    else:
        ap, mag = A, A.abs()
    c = 2 + C_PRO[s.pro]
    keep = torch.ones(s.K, dtype=torch.bool)
    if drop_k is not None:
        keep[drop_k] = False
    lin = alpha * (ap[:, keep] @ Bm[keep])
    L = 2 * (depth(s) + c) * U * abs(alpha) * (mag @ Bm.abs())
    cs = alpha * ap[:, keep].sum(1)
    CS = (depth_colsum(s) + 1 + C_PRO[s.pro]) * U * abs(alpha) * mag.sum(1)
    if shift is not None:
        rdm, g, er, axh = shift
        L = L + abs(alpha) * (rdm * (g @ Bm).abs()[None, :] + er * (axh @ Bm.abs()))
        CS = CS + abs(alpha) * (rdm[:, 0] * g.sum().abs() + er[:, 0] * axh.sum(1))
    if o["bias"] is not None:
        lin = lin + o["bias"].double()
        L = L + U * o["bias"].double().abs()
    r.update(lin=lin, lin_bound=L, colsum=cs, colsum_bound=CS)
    if s.epi == EPI_TANH:
        out = torch.tanh(lin)
        B_ = L * (1 - torch.tanh((lin.abs() - L).clamp_min(0)) ** 2) + 3 * U * out.abs()
    elif s.epi == EPI_MUL_DGELU:
        gp = _gelu_grad(o["aux"].double())
        out = lin * gp
        B_ = gp.abs() * L + lin.abs() * DG + U * out.abs()
    else:
        out, B_ = lin, L
    r.update(out=out, out_bound=B_)
    return r


def restate_f32(s: Spec, o: dict) -> dict:
    """The same formula in fp32 with torch's own summation order (the CPU self-check's right answer): lin, colsum, stats."""
    A, Bm = o["A"], o["B"]
    alpha = torch.tensor(alpha_of(s), dtype=torch.float32)
    r = {}
    if s.pro == PRO_LN:
        m = A.mean(1, keepdim=True)
        rs = torch.rsqrt(((A - m) ** 2).mean(1, keepdim=True) + torch.tensor(s.eps, dtype=torch.float32))
        ap = (A - m) * rs * o["gamma"] + o["beta"]
        r["stats"] = torch.cat([m, rs], 1)
    elif s.pro == PRO_TANH_BWD:
        ap = A * (1 - o["y"] * o["y"])
    else:
        ap = A
    lin = alpha * (ap @ Bm)
    if o["bias"] is not None:
        lin = lin + o["bias"]
    r.update(lin=lin, colsum=alpha * ap.sum(1))
    return r
