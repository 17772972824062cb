"""The per-element attention bounds of tests/attention_ref.py must hold and must bite (no GPU needed).

A float64 emulation that applies exactly the kernels' 16-bit roundings (P resp. dS before the products, every output; fp32 steps
exact) stays within the bounds for every input family, mask pattern and shape class the GPU module uses, in both operand formats;
and the fp16 bounds reject -- error / bound > 1 on each of ctx, dV, dK and dQ -- the same emulation with P and dS rounded through
bf16, the mutation that a max-norm tolerance of 6e-3 does not see."""
import pytest
import torch

from tests import attention_ref as A

SHAPES = [(1, 1), (17, 17), (33, 33), (185, 185), (7, 25), (65, 129), (129, 64)]


def _case(fmt, Sq, Skv, family, mask, seed, causal=False, pdrop=0.0):
    lead = (3, 2)
    q, k, v, do = A.make_heads(fmt, lead, Sq, Skv, family, seed)
    allow = torch.ones(3, 1, Sq, Skv, dtype=torch.bool)
    km = A.key_mask(mask, 3, Skv, seed + 1)
    if km is not None:
        allow = allow & km.bool()[:, None, None, :]
    if causal:
        allow = allow & A.causal_allow(Sq, Skv)
    mk = None
    if pdrop:
        gen = torch.Generator().manual_seed(seed + 2)
        mk = (torch.rand(3, 2, Sq, Skv, generator=gen) >= pdrop).double() / (1.0 - pdrop)
    return q, k, v, do, allow, mk


def _ratios(fmt, case, c32, pfmt=None):
    q, k, v, do, allow, mk = case
    ref = A.fwd_ref(q, k, v, allow, mk)
    b_ctx, b_lse = A.fwd_bound(ref, v, fmt, c32)
    ctx, lse = A.fwd_emul(q, k, v, allow, mk, fmt, pfmt)
    ctx16, lse32 = A.r16(ref["ctx"], fmt), A.r32(ref["lse"])
    bref = A.bwd_ref(q, k, v, allow, mk, ctx16, lse32, do)
    bq, bk, bv = A.bwd_bound(bref, q, k, do, fmt, c32)
    dq, dk, dv = A.bwd_emul(q, k, v, allow, mk, ctx16, lse32, do, fmt, pfmt)
    assert float(ref["lse"].abs().max()) <= A.LSE_MAX
    return {"ctx": float(((ctx - ref["ctx"]).abs() / b_ctx).max()), "lse": float(((lse - ref["lse"]).abs() / b_lse).max()),
            "dQ": float(((dq - bref["dQ"]).abs() / bq).max()), "dK": float(((dk - bref["dK"]).abs() / bk).max()),
            "dV": float(((dv - bref["dV"]).abs() / bv).max())}


@pytest.mark.parametrize("fmt", A.FMTS)
@pytest.mark.parametrize("Sq,Skv", SHAPES)
def test_emulated_roundings_stay_within_the_bounds(fmt, Sq, Skv):
    worst = {}
    for family in A.FAMILIES:
        for mask in A.MASKS:
            variants = [dict()] if Sq == Skv else [dict(), dict(causal=True), dict(pdrop=0.1), dict(causal=True, pdrop=0.1)]
            for var in variants:
                c32 = A.C_VILT if Sq == Skv else A.C_ATTN2(max(Sq, Skv))
                r = _ratios(fmt, _case(fmt, Sq, Skv, family, mask, 100 * Sq + Skv, **var), c32)
                for key, val in r.items():
                    assert val <= 1.0, (fmt, Sq, Skv, family, mask, var, key, val)
                    worst[key] = max(worst.get(key, 0.0), val)
    print(f"\n[bounds {fmt} {Sq}x{Skv}] worst emulated error / bound: " + " ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("family", ("randn", "peaked"))
@pytest.mark.parametrize("mask", ("none", "random"))
@pytest.mark.parametrize("S", (33, 185))
def test_fp16_bounds_reject_bf16_rounding_of_p_and_ds(S, mask, family):
    case = _case("f16", S, S, family, mask, 7 * S)
    good = _ratios("f16", case, A.C_VILT)
    bad = _ratios("f16", case, A.C_VILT, pfmt="bf16")
    print(f"\n[bounds f16 S={S} {family} {mask}] fp16 roundings " + " ".join(f"{k} {v:.3g}" for k, v in sorted(good.items()))
          + " | P, dS through bf16 " + " ".join(f"{k} {v:.3g}" for k, v in sorted(bad.items())))
    for key in ("ctx", "dV", "dK", "dQ"):
        assert good[key] <= 1.0, (key, good[key])
        assert bad[key] > 1.0, (key, bad[key], "the fp16 bound does not see a bf16 rounding of P / dS")
