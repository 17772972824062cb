"""feddat_dat_loss_fwd_bwd_wide (csrc/head_tail.hip), the DAT loss at any width, element by element against a float64 evaluation
of the same formulas on the same fp32 inputs, in both operand builds (the kernel is fp32 in both).

Bounds, derived (u = 2^-24: one round-to-nearest fp32 operation, |fl(a op b) - (a op b)| <= u |a op b|; expf, logf and log1pf of
the HIP device library are within 1 ulp = 2 u relative; a sum of N non-negative terms added along any tree of depth D is within
D u of its exact value, relatively, to first order; T = 3, A = max(|x|, |t|) / T over the rows the call reads):

  row reductions: a lane adds its ceil(C / 256) elements in column order (the first add, to 0, is exact -- counted anyway), then
  6 wave_sum levels, then 3 adds over the four waves:            D_C = ceil(C / 256) + 9
  batch reduction: ceil(n / 64) adds per lane, 6 wave_sum levels:  D_n = ceil(n / 64) + 6

  log-probabilities, logp = x / T - (mx + log(sum exp(x / T - mx))):
      x * fl(1 / T): 2 u A.  exp argument a - mx: its rounding u * 2 A plus the two products' 4 u A.  Each exponential: 2 u + that.
      The sum: + D_C u.  So sum_exp is within (2 + 8 A + D_C) u relatively; logf of it: that, + 2 u log C for the result's ulp.
      mx + log(...): u (A + log C).  a - lsx: its own product 2 u A and the rounding u (2 A + log C).
      E_lp = u (13 A + 2 + D_C + 4 log C)                                   absolute, for logp and logq alike
  p = exp(logp) <= 1: |dp| <= E_lp + 2 u, same for q.  sigmoid = 1 / (1 + exp(-x)) <= 1: 4 u.
  dlogits = gs ((sig - y) + T (p - q)), gs = fl(0.5 / n):
      sig - y: 4 u + u.   T (p - q): T (2 (E_lp + 2 u) + 2 u).   the outer add and the two products: 3 (1 + T) u.
      |d dlogits| <= gs ((5 + 6 T + 3 (1 + T)) u + 2 T E_lp) = gs (35 u + 6 E_lp)  at T = 3
  BCE element f = max(x, 0) - x y + log1p(exp(-|x|)) >= 0:  u |x| (the product), 2 u + 1.4 u (log1p: argument and result),
      two adds 2 u (|x| + 0.7):  e_f <= u (3 |x| + 5).   scalars[0] = sum f / n:
      |d scalars[0]| <= (sum_elements e_f + (D_C + D_n + 1) u sum f) / n
  KL element k = q (logq - logp), d = logq - logp:  |dk| <= q (2 E_lp + u |d|) + (E_lp + 2 u) q |d| + u |k|, and sum_j q_j = 1:
      |d scalars[1]| <= T^2 / n (sum_rows (2 E_lp + (E_lp + 4 u) sum_j q_j |d_j|) + (D_C + D_n + 3) u sum |k|)
  scalars[2] = 0.5 (scalars[0] + scalars[1]): half the sum of the two bounds + u |scalars[2]|.
  Second-order terms are covered by the factor 1 + 2^-10.

feddat_dat_loss_fwd_bwd_checked adds two elements per lane and 6 wave levels per row (a shallower tree) with the same
element arithmetic, so the same expressions bound it; the two kernels agree within the sum of their bounds, 2 x the above.

Measured worst |error| / bound over all cases of this file (MI355X, the two builds give the same bits): dlogits 0.017,
scalars[0] 0.059, scalars[1] 0.064, scalars[2] 0.064; wide vs checked (against 2 x the bound) dlogits 0.0027, scalars 0.0033.
Every case prints its own ratios (run with -s)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMTS = ("bf16", "f16")
U = 2.0 ** -24
T = 3.0
REG_LIMIT = 4096      # columns up to which a row's operands stay in registers (WIDE_REG_C, csrc/head_tail.hip)
SHAPES = [(1, 129), (5, 255), (4, 256), (4, 257), (3, 1), (65, 1000), (32, 3129), (2, REG_LIMIT + 1)]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import lib
    lib.load()
    with lib.operands("f16"):
        lib.load()
    return lib


_INPUTS = {}


def inputs(B, C):
    """fp32 (logits, teacher, target) on the host, once per shape: logits / teacher N(0, 2), 1-3 labels per row with scores
    in {0.3, 0.6, 0.9, 1.0} (the synthetic batches' targets)."""
    if (B, C) not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * B + C)
        x = torch.randn(B, C, generator=g) * 2
        t = torch.randn(B, C, generator=g) * 2
        y = torch.zeros(B, C)
        scores = torch.tensor([0.3, 0.6, 0.9, 1.0])
        for b in range(B):
            k = min(C, int(torch.randint(1, 4, (1,), generator=g)))
            y[b, torch.randperm(C, generator=g)[:k]] = scores[torch.randint(0, 4, (k,), generator=g)]
        _INPUTS[(B, C)] = (x, t, y)
    return _INPUTS[(B, C)]


_REF = {}


def reference(B, C, n):
    """float64 evaluation on rows [0, n) and the derived bounds: (dlogits [n, C], scalars [3], bound_dl, bound_scalars [3])."""
    if (B, C, n) in _REF:
        return _REF[(B, C, n)]
    x, t, y = (v[:n].double() for v in inputs(B, C))
    logp = torch.log_softmax(x / T, 1)
    logq = torch.log_softmax(t / T, 1)
    p, q = logp.exp(), logq.exp()
    f = x.clamp_min(0) - x * y + torch.log1p(torch.exp(-x.abs()))
    k = q * (logq - logp)
    dl = 0.5 / n * ((torch.sigmoid(x) - y) + T * (p - q))
    bce, kl = float(f.sum()) / n, float(k.sum()) / n * T * T
    sc = torch.tensor([bce, kl, 0.5 * (bce + kl)], dtype=torch.float64)
    A = max(float(x.abs().max()), float(t.abs().max())) / T
    d_c, d_n = math.ceil(C / 256) + 9, math.ceil(n / 64) + 6
    e_lp = U * (13 * A + 2 + d_c + 4 * math.log(C))
    slack = 1 + 2.0 ** -10
    b_dl = 0.5 / n * (35 * U + 6 * e_lp) * slack
    b0 = (float((U * (3 * x.abs() + 5)).sum()) + (d_c + d_n + 1) * U * float(f.sum())) / n * slack
    qd = float((q * (logq - logp).abs()).sum())
    b1 = T * T / n * (2 * e_lp * n + (e_lp + 4 * U) * qd + (d_c + d_n + 3) * U * float(k.abs().sum())) * slack
    b2 = (0.5 * (b0 + b1) + U * abs(float(sc[2]))) * slack
    _REF[(B, C, n)] = (dl, sc, b_dl, torch.tensor([b0, b1, b2], dtype=torch.float64))
    return _REF[(B, C, n)]


def run(L, x, t, y, B, C, n, flag=None, dl=None):
    dl = torch.full((B, C), 7.0, device=DEV) if dl is None else dl
    sc = torch.full((4,), -5.0, device=DEV)
    ws = torch.full((L.dat_loss_wide_workspace_elems(B),), float("nan"), device=DEV)
    L.dat_loss_fwd_bwd_wide(x, t, y, dl, sc, ws, n=n, nonfinite=flag, temp=T)
    torch.cuda.synchronize()
    return dl, sc


def rows_of(B):
    return sorted({B, 1, max(B - 1, 1)})


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("with_flag", [False, True])
@pytest.mark.parametrize("B,C", SHAPES)
def test_wide_loss_against_float64(L, fmt, with_flag, B, C):
    x, t, y = (v.to(DEV) for v in inputs(B, C))
    with L.operands(fmt):
        assert L.dat_loss_wide_workspace_elems(B) == 2 * B
        for n in rows_of(B):
            flag = torch.zeros(1, dtype=torch.int32, device=DEV) if with_flag else None
            dl_ref, sc_ref, b_dl, b_sc = reference(B, C, n)
            # rows >= n of the inputs hold NaN: never read
            xs, ts, ys = (v.clone() for v in (x, t, y))
            for v in (xs, ts, ys):
                v[n:] = float("nan")
            dl, sc = run(L, xs, ts, ys, B, C, n, flag)      # dlogits starts as 7.0 everywhere: "a previous call's non-zeros"
            dl2, sc2 = run(L, xs, ts, ys, B, C, n, flag)
            assert torch.equal(dl, dl2) and torch.equal(sc[:3], sc2[:3]), "two calls differ"
            assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(sc[:3]).all())
            assert float(sc[3]) == -5.0, "wrote past scalars[2]"
            assert torch.equal(dl[n:], torch.zeros_like(dl[n:])), "rows [n, B) are not exactly 0.0f"
            if flag is not None:
                assert int(flag) == 0
            e_dl = float((dl[:n].double().cpu() - dl_ref).abs().max())
            e_sc = (sc[:3].double().cpu() - sc_ref).abs()
            print(f"{fmt} ({B}, {C}) n={n} flag={with_flag}: dlogits {e_dl:.3e} / {b_dl:.3e} = {e_dl / b_dl:.4f}; scalars "
                  + ", ".join(f"{float(e):.3e} / {float(b):.3e} = {float(e / b):.4f}" for e, b in zip(e_sc, b_sc)))
            assert e_dl <= b_dl, (n, e_dl, b_dl)
            assert bool((e_sc <= b_sc).all()), (n, e_sc.tolist(), b_sc.tolist())


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,C", SHAPES)
def test_flag_follows_the_valid_rows_and_is_only_set(L, fmt, B, C):
    x, t, y = (v.to(DEV) for v in inputs(B, C))
    with L.operands(fmt):
        for n in rows_of(B):
            yi = y.clone()
            # an inf target in the last valid row ((65, 1000) at n = 65: row 64, the second stride of the finish launch's lane 0)
            yi[n - 1, C // 2] = float("inf")
            flag = torch.zeros(1, dtype=torch.int32, device=DEV)
            _, sc = run(L, x, t, yi, B, C, n, flag)
            assert int(flag) == 1 and not bool(torch.isfinite(sc[0]))
            run(L, x, t, y, B, C, n, flag)          # a clean call leaves the flag as it was
            assert int(flag) == 1
            run(L, x, t, yi, B, C, n, None)         # no flag pointer: nothing to write, no fault
            if n < B:                               # the same inf in a row that is not part of the batch
                yo = y.clone()
                yo[n, C // 2] = float("inf")
                flag.zero_()
                _, sc = run(L, x, t, yo, B, C, n, flag)
                assert int(flag) == 0 and bool(torch.isfinite(sc[:3]).all())


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,C", SHAPES)
def test_twenty_calls_in_one_graph_give_the_eager_bits(L, fmt, B, C):
    x, t, y = (v.to(DEV) for v in inputs(B, C))
    with L.operands(fmt):
        for n in rows_of(B):
            _graph_case(L, x, t, y, B, C, n)


def _graph_case(L, x, t, y, B, C, n):
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    dl_e, sc_e = run(L, x, t, y, B, C, n, flag)
    dl = torch.full((B, C), 7.0, device=DEV)
    sc = torch.full((4,), -5.0, device=DEV)
    ws = torch.empty(L.dat_loss_wide_workspace_elems(B), device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        L.dat_loss_fwd_bwd_wide(x, t, y, dl, sc, ws, n=n, nonfinite=flag, temp=T)      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(20):
            L.dat_loss_fwd_bwd_wide(x, t, y, dl, sc, ws, n=n, nonfinite=flag, temp=T)
    for _ in range(2):
        dl.fill_(7.0)
        sc.fill_(-5.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dl, dl_e) and torch.equal(sc[:3], sc_e[:3]) and int(flag) == 0, (B, C, n)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("C", [100, 128])
def test_agrees_with_the_checked_kernel_where_both_apply(L, fmt, C):
    B = 32
    x, t, y = (v.to(DEV) for v in inputs(B, C))
    with L.operands(fmt):
        dl_w, sc_w = run(L, x, t, y, B, C, B)
        dl_c = torch.empty(B, C, device=DEV)
        sc_c = torch.empty(4, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        L.dat_loss_fwd_bwd_checked(x, t, y, dl_c, sc_c, flag, temp=T)
        torch.cuda.synchronize()
    _, _, b_dl, b_sc = reference(B, C, B)
    e_dl = float((dl_w.double() - dl_c.double()).abs().max())
    e_sc = (sc_w[:3].double() - sc_c[:3].double()).abs().cpu()
    print(f"{fmt} C={C}: wide vs checked dlogits {e_dl:.3e} / {2 * b_dl:.3e}; scalars {e_sc.tolist()} / {(2 * b_sc).tolist()}")
    assert e_dl <= 2 * b_dl and bool((e_sc <= 2 * b_sc).all())
