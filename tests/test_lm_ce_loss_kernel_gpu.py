"""feddat_lm_ce_loss_fwd_bwd (include/feddat_hip_albef.h), the LM loss without a teacher, in both operand builds: bit for bit the
teacher-less call of feddat_lm_loss_fwd_bwd_dyn with twice the grad_scale (the kernel is that kernel's second instantiation), its
own finish (L in scalars[0] and [2], 0 in [1]), float64 element by element, the overflow flag, and the argument checks.

Tolerances against float64.  Loss and row terms: 1e-5 relative (+ 1e-6), the bound tests/test_ops_gpu.py holds the general kernel
to.  dlogits is stored in the operand format: half an ulp of it is 2^-9 (bf16) / 2^-12 (fp16) relative; the fp32 softmax ahead of
the rounding (__expf, the 1024-lane sum) adds a few 1e-6; the bound is one ulp, 2^-8 / 2^-11, plus an absolute term -- 1e-9 for
bf16 (fp32's exponent range), 2^-24 for fp16 (the spacing of its subnormals, where a softmax tail of 1e-8 lands)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 5, 8, 8), (7, 30522, 30592, 30592), (96, 3072, 3072, 3072), (5, 4099, 4224, 4224)]
REL = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
ABS = {"bf16": 1e-9, "f16": 2.0 ** -24}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import lib
    return lib


def _case(R, V, ldl, seed=0):
    g = torch.Generator().manual_seed(1000 * R + V + seed)
    lg = torch.zeros(R, ldl)
    lg[:, :V] = torch.randn(R, V, generator=g) * 3
    labels = torch.randint(0, V, (R,), generator=g)
    labels[::3] = -100
    labels[R - 1] = V - 1                                   # the last column (the scalar tail when V % 4 != 0)
    if R > 1:
        labels[1] = 0
    rw = torch.rand(R, generator=g) + 0.1
    return lg, labels, rw


def _reference(lg, labels, rw, V, scale):
    """float64: (L, row terms w_r ce_r, scale * dL/dlogits)."""
    l64 = lg[:, :V].double().clone().requires_grad_(True)
    logp = F.log_softmax(l64, -1)
    rows = torch.where(labels >= 0, -logp.gather(1, labels.clamp(min=0)[:, None])[:, 0] * rw.double(), torch.zeros(len(rw), dtype=torch.float64))
    rows.sum().backward()
    return rows.sum().detach(), rows.detach(), scale * l64.grad


@pytest.mark.parametrize("operands", ["f16", "bf16"])
@pytest.mark.parametrize("R,V,ldl,ldd", SHAPES)
@pytest.mark.parametrize("form", ["static", "dynamic"])
def test_ce_loss_equals_the_teacherless_general_call_and_float64(L, operands, R, V, ldl, ldd, form):
    """static: grad_scale 4, no device scale, no flag.  dynamic: grad_scale 1, the device scale 2^10, the flag given."""
    lg, labels, rw = _case(R, V, ldl)
    dt = L.OPERAND_DTYPE[operands]
    gs, gdev = (4.0, None) if form == "static" else (1.0, torch.tensor([1024.0], device=DEV))
    flag = None if form == "static" else torch.zeros(1, dtype=torch.int32, device=DEV)
    flag_old = torch.zeros(1, dtype=torch.int32, device=DEV)
    d_lg, d_lab, d_rw = lg.to(DEV), labels.to(DEV), rw.to(DEV)
    dl, dl_old = (torch.full((R, ldd), 7.0, dtype=dt, device=DEV) for _ in range(2))
    sc, sc_old, sc_nod = (torch.full((4 + 2 * R,), -3.0, device=DEV) for _ in range(3))
    with L.operands(operands):
        L.lm_ce_loss_fwd_bwd(d_lg, d_lab, d_rw, V, dl, sc, grad_scale=gs, grad_scale_dev=gdev, nonfinite=flag)
        L.lm_ce_loss_fwd_bwd(d_lg, d_lab, d_rw, V, None, sc_nod, grad_scale=gs, grad_scale_dev=gdev, nonfinite=flag)   # dlogits = NULL
        # the general entry point without a teacher: it computes 0.5 * grad_scale * dL/dlogits, so twice the scale
        L.lm_loss_fwd_bwd(d_lg, None, d_lab, d_rw, V, 3.0, 0.0, dl_old, sc_old, grad_scale=2 * gs, grad_scale_dev=gdev,
                          nonfinite=flag_old)
    torch.cuda.synchronize()
    # ---- bit equality with the old entry point: dlogits, L and every row term
    assert torch.equal(dl.view(torch.int16), dl_old.view(torch.int16))
    assert torch.equal(sc[0], sc_old[0]) and torch.equal(sc[4:], sc_old[4:])
    assert torch.equal(sc, sc_nod)
    # ---- its own finish
    assert float(sc[2]) == float(sc[0]) and float(sc[1]) == 0.0 and float(sc_old[2]) == 0.5 * float(sc_old[0])
    assert float(sc[5::2].abs().max()) == 0.0
    assert float(sc[3]) == -3.0                       # scalars[3] is not the kernel's
    if flag is not None:
        assert int(flag) == 0
    # ---- padding columns and float64
    got = dl.float().cpu()
    assert torch.equal(got[:, V:], torch.zeros(R, ldd - V))
    scale = gs * (1024.0 if gdev is not None else 1.0)
    Lref, rows, gref = _reference(lg, labels, rw, V, scale)
    assert abs(float(sc[0]) - float(Lref)) <= 1e-5 * abs(float(Lref)) + 1e-6
    assert bool(((sc[4::2].cpu().double() - rows).abs() <= 1e-5 * rows.abs() + 1e-6).all())
    err = (got[:, :V].double() - gref).abs()
    tol = REL[operands] * gref.abs() + ABS[operands] * (scale if operands == "bf16" else 1.0)      # (fp32's floor moves with the scale)
    assert bool((err <= tol).all()), (float(err.max()), float((err / tol).max()))


@pytest.mark.parametrize("operands", ["f16", "bf16"])
def test_inf_in_the_logits_sets_the_flag(L, operands):
    R, V, ldl = 5, 4099, 4224
    lg, labels, rw = _case(R, V, ldl)
    labels[1] = 17
    lg[1, 17] = float("inf")              # ce of row 1 = inf - inf
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    sc = torch.zeros(4 + 2 * R, device=DEV)
    dl = torch.zeros(R, ldl, dtype=L.OPERAND_DTYPE[operands], device=DEV)
    with L.operands(operands):
        L.lm_ce_loss_fwd_bwd(lg.to(DEV), labels.to(DEV), rw.to(DEV), V, dl, sc, nonfinite=flag)
    torch.cuda.synchronize()
    assert int(flag) == 1 and not bool(torch.isfinite(sc[0]))
    flag.zero_()
    lg[1, 17] = 0.5
    with L.operands(operands):
        L.lm_ce_loss_fwd_bwd(lg.to(DEV), labels.to(DEV), rw.to(DEV), V, dl, sc, nonfinite=flag)
    torch.cuda.synchronize()
    assert int(flag) == 0 and bool(torch.isfinite(sc[0]))


@pytest.mark.parametrize("operands", ["f16", "bf16"])
def test_every_refused_call_writes_nothing(L, operands):
    """The argument checks of feddat_lm_loss_fwd_bwd_dyn: FEDDAT_EINVAL, and neither dlogits, scalars nor the flag is touched."""
    R, V, ldl = 5, 4099, 4224
    lg, labels, rw = _case(R, V, ldl)
    d_lg, d_lab, d_rw = lg.to(DEV), labels.to(DEV), rw.to(DEV)
    dl = torch.full((R, ldl), 7.0, dtype=L.OPERAND_DTYPE[operands], device=DEV)
    sc = torch.full((4 + 2 * R,), -3.0, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    ok = dict(logits=p(d_lg), ldl=ldl, labels=p(d_lab), rw=p(d_rw), R=R, V=V, gs=1.0, gdev=None, flag=p(flag), dl=p(dl), ldd=ldl,
              sc=p(sc))
    bad = [dict(logits=None), dict(labels=None), dict(rw=None), dict(sc=None), dict(R=0), dict(V=0), dict(ldl=V - 3), dict(gs=0.0),
           dict(gs=-1.0), dict(ldd=V - 3), dict(ldl=ldl + 2), dict(ldd=ldl + 2), dict(logits=C.c_void_p(d_lg.data_ptr() + 4)),
           dict(dl=C.c_void_p(dl.data_ptr() + 2))]
    with L.operands(operands):
        fn = L._ext("feddat_lm_ce_loss_fwd_bwd")
        for kw in bad:
            a = dict(ok, **kw)
            rc = fn(a["logits"], a["ldl"], a["labels"], a["rw"], a["R"], a["V"], a["gs"], a["gdev"], a["flag"], a["dl"], a["ldd"],
                    a["sc"], None)
            assert rc == 1, kw                  # FEDDAT_EINVAL
        with pytest.raises(L.FeddatHipError):
            L._ext("feddat_lm_loss_fwd_bwd_dyn")            # _ext serves the extension header only
    torch.cuda.synchronize()
    assert bool((dl == 7.0).all()) and bool((sc == -3.0).all()) and int(flag) == 0
