"""feddat_head_gemm (feddat_amd/csrc/head_tail.hip: ht_gemm_kernel) over its whole dispatch matrix, element by element against
float64, and the head's two LayerNorm launches at the edges of their register-resident rows.

The kernel specialises into 2 x 2 x 2 load / tile templates x 2 modes x 3 prologues x 3 epilogues, chosen on the host from strides,
K % 4, pointer alignment and a tile count.  Every case here (tests/head_gemm_ref.py: CASES) first ASKS feddat_head_gemm_plan which
path its job takes and asserts the one it is there for, so a case cannot silently move to another path; then it fills every output
with NaN (with the ldo gap and a guard behind each buffer), launches, and holds every element against the float64 restatement
of the header's formula under the bound derived in tests/head_gemm_ref.py -- derived from the summation order and the number
formats, not from what the kernel gives.  Nothing outside [I, J], [I] and [I, 2] may have changed, nothing inside may still be
NaN.  The padding of every strided INPUT is NaN as well: a load that strays off its row poisons the output.

test_bound_notices_a_missing_slice_cpu checks the bound against the reference alone, without a GPU: a float32 restatement in
another summation order lies inside it, and a product with one k-slice left out lies outside it on at least 90 % of the outputs."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import head_gemm_ref as R

gpu = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
GUARD = 64
FMTS = ("bf16", "f16")          # the two operand builds of the library: head_tail.hip is exact fp32 in both, both must pass
NAMES = [s.name for s in R.CASES]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import lib
    lib.load()
    with lib.operands("f16"):
        lib.load()
    return lib


_REF = {}          # case name -> (operands, float64 reference): computed once, shared by every test, never written to


def ref_of(name):
    if name not in _REF:
        s = R.CASE[name]
        o = R.operands(s)
        _REF[name] = (o, R.reference(s, o))
    return _REF[name]


# ------------------------------------------------------------------------------------------------ device side
def _strided(logical, inner, pad, off):
    """`logical` [rows, inner] as rows of stride inner + pad behind `off` floats, everything else NaN (CPU, then to the device)."""
    rows = logical.shape[0]
    flat = torch.full((off + rows * (inner + pad),), NAN)
    flat[off:].view(rows, inner + pad)[:, :inner] = logical
    return flat.to(DEV)


class Bufs:
    """The device buffers of one case and its job."""

    def __init__(self, L, s, o):
        g = R.geometry(s)
        self.s, self.g = s, g
        lay_a = (lambda t, off: _strided(t, s.K, s.sa_pad, off)) if s.a_lay == "k" else (lambda t, off: _strided(t.t(), s.I, s.sa_pad, off))
        self.A = lay_a(o["A"], s.a_off)
        self.B = _strided(o["B"].t(), s.K, s.sb_pad, s.b_off) if s.b_lay == "k" else _strided(o["B"], s.J, s.sb_pad, s.b_off)
        self.y = lay_a(o["y"], s.y_off) if s.pro == R.PRO_TANH_BWD else None
        self.gamma = o["gamma"].to(DEV) if s.pro == R.PRO_LN else None
        self.beta = o["beta"].to(DEV) if s.pro == R.PRO_LN else None
        self.bias = o["bias"].to(DEV) if s.bias else None
        self.aux = _strided(o["aux"], s.J, s.aux_pad, 0) if s.epi == R.EPI_MUL_DGELU else None
        self.alpha_dev = torch.tensor([s.alpha_dev], device=DEV) if s.alpha_dev is not None else None
        self.out = torch.full((s.I * g["ldo"] + GUARD,), NAN, device=DEV)
        self.colsum = torch.full((s.I + GUARD,), NAN, device=DEV)
        self.stats = torch.full((2 * s.I + GUARD,), NAN, device=DEV)
        p = lambda t: t.data_ptr() if t is not None else 0
        pro_a = self.gamma if s.pro == R.PRO_LN else self.y
        self.job = R.fill_job(L, s, dict(A=p(self.A), B=p(self.B), out=p(self.out), bias_j=p(self.bias), colsum=p(self.colsum),
                                         pro_a=p(pro_a), pro_b=p(self.beta), stats_out=p(self.stats), aux=p(self.aux),
                                         alpha_dev=p(self.alpha_dev)))

    def untouched(self):
        return bool(torch.isnan(self.out).all() and torch.isnan(self.colsum).all() and torch.isnan(self.stats).all())

    def results(self):
        """What the launch wrote, after checking that it wrote nowhere else: (out [I, J], colsum [I] | None, stats [I, 2] | None)."""
        s, ldo = self.s, self.g["ldo"]
        o2 = self.out[:s.I * ldo].view(s.I, ldo)
        assert torch.isnan(self.out[s.I * ldo:]).all(), f"{s.name}: wrote behind out"
        assert torch.isnan(o2[:, s.J:]).all(), f"{s.name}: wrote into the ldo gap"
        assert not torch.isnan(o2[:, :s.J]).any(), f"{s.name}: out has unwritten (or poisoned) elements"
        cs = st = None
        if s.colsum:
            assert torch.isnan(self.colsum[s.I:]).all() and not torch.isnan(self.colsum[:s.I]).any(), f"{s.name}: colsum extent"
            cs = self.colsum[:s.I].clone()
        else:
            assert torch.isnan(self.colsum).all(), f"{s.name}: colsum written without being asked for"
        if s.stats:
            assert torch.isnan(self.stats[2 * s.I:]).all() and not torch.isnan(self.stats[:2 * s.I]).any(), f"{s.name}: stats extent"
            st = self.stats[:2 * s.I].view(s.I, 2).clone()
        else:
            assert torch.isnan(self.stats).all(), f"{s.name}: stats written without being asked for"
        return o2[:, :s.J].clone(), cs, st


def assert_plan(L, s, job):
    """The case runs on the path it is there for -- asked of the library before anything is launched."""
    p = L.head_gemm_plan(job)
    assert (p["avec"], p["bvec"], p["jt"]) == s.want, (s.name, p)
    return s.path


_RUN = {}          # (fmt, case name) -> results() of the case launched alone


def run_alone(L, fmt, name):
    if (fmt, name) not in _RUN:
        s = R.CASE[name]
        with L.operands(fmt):
            b = Bufs(L, s, ref_of(name)[0])
            assert_plan(L, s, b.job)
            L.head_gemm(b.job)
            torch.cuda.synchronize()
        _RUN[(fmt, name)] = b.results()
    return _RUN[(fmt, name)]


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ a, d, e, f, g, j: every case
@gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fmt", FMTS)
def test_case_against_float64(L, fmt, name):
    s = R.CASE[name]
    _, ref = ref_of(name)
    out, cs, st = run_alone(L, fmt, name)
    err = (out.cpu().double() - ref["out"]).abs()
    msg = f"{name} [{fmt}] path {s.path}: out uses {float((err / ref['out_bound']).max()):.3f} of its bound"
    ok = bool((err <= ref["out_bound"]).all())
    if cs is not None:
        e = (cs.cpu().double() - ref["colsum"]).abs()
        msg += f", colsum {float((e / ref['colsum_bound']).max()):.3f}"
        ok = ok and bool((e <= ref["colsum_bound"]).all())
    if st is not None:
        st = st.cpu().double()
        em = (st[:, 0] - ref["stats"][:, 0]).abs()
        er = (st[:, 1] / ref["stats"][:, 1] - 1).abs()
        msg += f", mean {float((em / ref['mean_bound']).max()):.3f}, rstd {float((er / ref['rstd_rel_bound']).max()):.3f}"
        ok = ok and bool((em <= ref["mean_bound"]).all()) and bool((er <= ref["rstd_rel_bound"]).all())
    print(msg)
    assert ok, msg


# ------------------------------------------------------------------------------------------------ b, c: bit identities
@gpu
@pytest.mark.parametrize("aligned,fallback", R.FALLBACK_PAIRS)
@pytest.mark.parametrize("fmt", FMTS)
def test_dword_fallback_is_bit_identical(L, fmt, aligned, fallback):
    """The same values through a copy whose base is one float off 16-byte alignment (or whose row stride is not a multiple of 4):
    the plan flips that operand to dword loads (asserted in run_alone), the k order is the same, so are the bits."""
    assert R.CASE[aligned].want != R.CASE[fallback].want
    assert _same(run_alone(L, fmt, aligned), run_alone(L, fmt, fallback))


@gpu
@pytest.mark.parametrize("full,rows16", R.JT_IDENTITY)
@pytest.mark.parametrize("fmt", FMTS)
def test_one_and_four_tiles_per_wave_are_bit_identical(L, fmt, full, rows16):
    """Rows 0..15 of the jt == 4 case as their own job run at jt == 1: the same k order per element, the same bits."""
    assert R.CASE[full].want[2] == 4 and R.CASE[rows16].want[2] == 1
    assert torch.equal(run_alone(L, fmt, full)[0][:16], run_alone(L, fmt, rows16)[0])


@gpu
@pytest.mark.parametrize("name", R.INF_B_CASES)
@pytest.mark.parametrize("fmt", FMTS)
def test_infinite_b_element_stays_infinite_in_its_column(L, fmt, name):
    """B[0, j0] = +inf and B[K - 1, j1] = -inf: columns j0 / j1 of the product are +-inf with the sign of alpha a[i, 0] / -alpha
    a[i, K - 1] -- not NaN, which is what 0 * inf from a k slot past K would make of them -- and every other column keeps its bits."""
    s = R.CASE[name]
    o = dict(ref_of(name)[0])
    j0, j1 = R.INF_B_COLS
    o["B"] = o["B"].clone()
    o["B"][0, j0], o["B"][s.K - 1, j1] = float("inf"), float("-inf")
    clean = run_alone(L, fmt, name)[0]
    with L.operands(fmt):
        b = Bufs(L, s, o)
        assert_plan(L, s, b.job)
        L.head_gemm(b.job)
        torch.cuda.synchronize()
    out = b.results()[0]
    inf = torch.full((s.I,), float("inf"), device=DEV)
    assert torch.equal(out[:, j0], torch.copysign(inf, o["A"][:, 0].to(DEV) * s.alpha))
    assert torch.equal(out[:, j1], torch.copysign(inf, -o["A"][:, s.K - 1].to(DEV) * s.alpha))
    keep = torch.ones(s.J, dtype=torch.bool, device=DEV)
    keep[[j0, j1]] = False
    assert torch.equal(out[:, keep], clean[:, keep])


# ------------------------------------------------------------------------------------------------ h: two jobs per launch
@gpu
@pytest.mark.parametrize("first,second", R.TWO_JOB_PAIRS + [(b, a) for a, b in R.TWO_JOB_PAIRS])
@pytest.mark.parametrize("fmt", FMTS)
def test_two_jobs_in_one_launch_equal_each_alone(L, fmt, first, second):
    alone = [run_alone(L, fmt, n) for n in (first, second)]
    with L.operands(fmt):
        bufs = [Bufs(L, R.CASE[n], ref_of(n)[0]) for n in (first, second)]
        assert R.CASE[first].path != R.CASE[second].path
        for b in bufs:
            assert_plan(L, b.s, b.job)
        L.head_gemm(bufs[0].job, bufs[1].job)
        torch.cuda.synchronize()
    for b, a in zip(bufs, alone):
        assert _same(b.results(), a), b.s.name


# ------------------------------------------------------------------------------------------------ i: refusals
@gpu
@pytest.mark.parametrize("name", [r[0] for r in R.REFUSALS])
@pytest.mark.parametrize("fmt", FMTS)
def test_refusal(L, fmt, name):
    """One field of a good job changed: FeddatHipError from the host, nothing launched, the NaN-filled outputs untouched -- alone,
    and as the second job behind a good first one (whose outputs stay untouched too)."""
    _, base, change = next(r for r in R.REFUSALS if r[0] == name)
    s = R.CASE[base]
    with L.operands(fmt):
        bad, good = Bufs(L, s, ref_of(base)[0]), Bufs(L, s, ref_of(base)[0])
        L.head_gemm_plan(bad.job)                          # good before the change
        change(bad.job)
        with pytest.raises(L.FeddatHipError, match="EINVAL"):
            L.head_gemm_plan(bad.job)
        with pytest.raises(L.FeddatHipError, match="EINVAL"):
            L.head_gemm(bad.job)
        with pytest.raises(L.FeddatHipError, match="EINVAL"):
            L.head_gemm(good.job, bad.job)
        torch.cuda.synchronize()
    assert bad.untouched() and good.untouched()


@gpu
@pytest.mark.parametrize("njobs", [0, 3])
@pytest.mark.parametrize("fmt", FMTS)
def test_refusal_njobs(L, fmt, njobs):
    with L.operands(fmt):
        bufs = [Bufs(L, R.CASE["i_plain"], ref_of("i_plain")[0]) for _ in range(njobs)]
        with pytest.raises(L.FeddatHipError, match="EINVAL"):
            L.head_gemm(*[b.job for b in bufs])
        torch.cuda.synchronize()
    assert all(b.untouched() for b in bufs)


# ------------------------------------------------------------------------------------------------ the bound itself, on the CPU
@pytest.mark.parametrize("name", NAMES)
def test_bound_notices_a_missing_slice_cpu(name):
    """The bound held against the reference alone: (1) the fp32 restatement of the same formula in torch's summation order lies
    inside it -- lin, colsum, and the LayerNorm statistics; (2) the float64 product with one k-slice left out lies outside it on at
    least 90 % of the outputs.  Both are about lin = alpha sum a' b + bias, the part the bound is derived for; the epilogues map it
    on monotonically (a saturated tanh hides a slice from any bound)."""
    s = R.CASE[name]
    o, ref = ref_of(name)
    f = R.restate_f32(s, o)
    assert ((f["lin"].double() - ref["lin"]).abs() <= ref["lin_bound"]).all()
    assert ((f["colsum"].double() - ref["colsum"]).abs() <= ref["colsum_bound"]).all()
    if s.pro == R.PRO_LN:
        assert ((f["stats"][:, 0].double() - ref["stats"][:, 0]).abs() <= ref["mean_bound"]).all()
        assert ((f["stats"][:, 1].double() / ref["stats"][:, 1] - 1).abs() <= ref["rstd_rel_bound"]).all()
    wrong = R.reference(s, o, drop_k=s.K // 2)
    caught = ((wrong["lin"] - ref["lin"]).abs() > ref["lin_bound"]).double().mean()
    assert caught >= 0.9, float(caught)


# ------------------------------------------------------------------------------------------------ the head's LayerNorm launches
def _ln_depth(H):
    return 4 * (-(-H // 256)) + 6          # additions an element passes through: its lane's chunks, then six butterfly levels


def _ln_inputs(rows, H, shift, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, H, generator=g) + shift
    gam, bet = 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    return x, gam, bet, torch.randn(rows, H, generator=g)


def _guarded(*shape):
    n = math.prod(shape)
    flat = torch.full((n + GUARD,), NAN, device=DEV)
    return flat, flat[:n].view(*shape)


def _written(flat, view, what):
    assert torch.isnan(flat[view.numel():]).all(), f"{what}: wrote behind the buffer"
    assert not torch.isnan(view).any(), f"{what}: unwritten elements"
    return view.cpu().double()


@gpu
@pytest.mark.parametrize("rows,H,shift", [(1, 4, 0.0), (5, 4, 0.0), (4096, 4, 0.0), (1, 260, 0.0), (5, 260, 0.0), (1, 2048, 0.0),
                                          (5, 2048, 0.0), (5, 4, 1000.0), (5, 260, 1000.0), (5, 2048, 1000.0)])
@pytest.mark.parametrize("fmt", FMTS)
def test_head_layernorm_launches_at_their_edges(L, fmt, rows, H, shift):
    """feddat_head_ln_gelu and feddat_head_ln_bwd_full at H in {4, 260, 2048} (2048 = the 8 x 64 x 4 register-resident row) and
    rows in {1, 5, 4096} (4096 = the backward's limit; at H = 4 only), with x and x + 1000, into NaN-filled guarded outputs.

    Bounds (u = 2^-24, d = 4 ceil(H / 256) + 6 the additions a row element passes through; the statistics as in head_gemm_ref.py):
      mean:  (d + 1) u mean|x| = dm;   rstd, relative:  (3 + d + 2) u / 2 + 2 u + (dm r)^2 / 2 = er;
      y = (x - m) r g + b:  4 u (|xh g| + |b|)  [its four roundings]  + r dm |g|  [the mean's error]  + er |xh g|  [rstd's];
      gelu_out = gelu_f(y_kernel): gelu' <= 1.13, and gelu_f itself is 0.5 y (1 + erf): the erf of common.hip.h within 1.5e-7 +
             20 * 1.5 u = 1.95e-6 (head_gemm_ref.py), two more roundings: 1.13 y_bound + 0.5 |y| 1.95e-6 + 2 u |gelu(y)|.
    The backward is held against ITS formula in float64 FROM THE SAME fp32 statistics it is handed (they are its inputs; their own
    error is bounded above), with gd = dy g, xh = (x - mean) rstd, m1 = mean gd, m2 = mean gd xh:
      m1: gd (1) + sum (d) + division (1): (d + 2) u mean|gd| = e1;   m2: gd (1), xh (2), product (1), sum, division:
          (d + 5) u mean|gd xh| = e2;
      dx = r (gd - m1 - xh m2): r (3 u |gd| + e1 + 2 u |m1| + |xh| e2 + 5 u |xh m2|) + u |dx|
          [gd's rounding and the two subtractions relative to it, m1's error and the subtractions relative to it, m2's error, xh's
          two roundings + the product + the subtractions relative to xh m2, the final product];
      dgamma[c] = sum_r dy xh in four row-interleaved partial sums added pairwise: ceil(rows / 4) + 2 additions, xh (2), product (1):
          (ceil(rows / 4) + 5) u sum_r |dy xh|;   dbeta[c]: (ceil(rows / 4) + 2) u sum_r |dy|."""
    U = R.U
    x, gam, bet, dy = _ln_inputs(rows, H, shift, 100 * H + rows)
    eps = 1e-5
    with L.operands(fmt):
        (yf, y), (sf, st), (gf, ge) = _guarded(rows, H), _guarded(rows, 2), _guarded(rows, H)
        L.head_ln_gelu(x.to(DEV), gam.to(DEV), bet.to(DEV), eps, y, st, ge)
        (dxf, dx), (dgf, dg), (dbf, db) = _guarded(rows, H), _guarded(H), _guarded(H)
        L.head_ln_bwd_full(dy.to(DEV), x.to(DEV), st, gam.to(DEV), dx, dg, db)
        torch.cuda.synchronize()
    xd, g64, b64, d = x.double(), gam.double(), bet.double(), _ln_depth(H)
    m = xd.mean(1, keepdim=True)
    r = 1 / torch.sqrt(((xd - m) ** 2).mean(1, keepdim=True) + float(torch.tensor(eps, dtype=torch.float32)))
    dm = (d + 1) * U * xd.abs().mean(1, keepdim=True)
    er = (3 + d + 2) * U / 2 + 2 * U + (dm * r) ** 2 / 2
    st64 = _written(sf, st, "stats")
    use = {"mean": ((st64[:, :1] - m).abs() / dm).max(), "rstd": ((st64[:, 1:] / r - 1).abs() / er).max()}
    xh = (xd - m) * r * g64
    y_ref, y_bound = xh + b64, 4 * U * (xh.abs() + b64.abs()) + r * dm * g64.abs() + er * xh.abs()
    use["y"] = ((_written(yf, y, "y") - y_ref).abs() / y_bound).max()
    ge_bound = 1.13 * y_bound + 0.5 * y_ref.abs() * 1.95e-6 + 2 * U * F.gelu(y_ref).abs()
    use["gelu"] = ((_written(gf, ge, "gelu_out") - F.gelu(y_ref)).abs() / ge_bound).max()
    # the backward, from the statistics it was handed
    mk, rk, dyd = st64[:, :1], st64[:, 1:], dy.double()
    gd, xk = dyd * g64, (xd - mk) * rk
    m1, m2 = gd.mean(1, keepdim=True), (gd * xk).mean(1, keepdim=True)
    e1, e2 = (d + 2) * U * gd.abs().mean(1, keepdim=True), (d + 5) * U * (gd * xk).abs().mean(1, keepdim=True)
    dx_ref = rk * (gd - m1 - xk * m2)
    dx_bound = rk * (3 * U * gd.abs() + e1 + 2 * U * m1.abs() + xk.abs() * e2 + 5 * U * (xk * m2).abs()) + U * dx_ref.abs()
    use["dx"] = ((_written(dxf, dx, "dx") - dx_ref).abs() / dx_bound).max()
    q = -(-rows // 4)
    use["dgamma"] = ((_written(dgf, dg, "dgamma") - (dyd * xk).sum(0)).abs() / ((q + 5) * U * (dyd * xk).abs().sum(0))).max()
    use["dbeta"] = ((_written(dbf, db, "dbeta") - dyd.sum(0)).abs() / ((q + 2) * U * dyd.abs().sum(0))).max()
    msg = f"rows {rows} H {H} shift {shift} [{fmt}]: part of each bound used: " + ", ".join(f"{k} {float(v):.3f}" for k, v in use.items())
    print(msg)
    assert all(float(v) <= 1.0 for v in use.values()), msg


@gpu
@pytest.mark.parametrize("what", ["H_mod_4", "H_gt_2048", "bwd_rows_gt_4096", "eps_0", "eps_negative"])
@pytest.mark.parametrize("fmt", FMTS)
def test_head_layernorm_refusals(L, fmt, what):
    rows, H, eps = {"H_mod_4": (5, 6, 1e-5), "H_gt_2048": (5, 2052, 1e-5), "bwd_rows_gt_4096": (4097, 4, 1e-5), "eps_0": (5, 8, 0.0),
                    "eps_negative": (5, 8, -1e-5)}[what]
    x, gam, bet, dy = (t.to(DEV) for t in _ln_inputs(rows, H, 0.0, 7))
    outs = [_guarded(rows, H), _guarded(rows, 2), _guarded(rows, H), _guarded(rows, H), _guarded(H), _guarded(H)]
    (_, y), (_, st), (_, ge), (_, dx), (_, dg), (_, db) = outs
    with L.operands(fmt):
        if what != "bwd_rows_gt_4096":
            with pytest.raises(L.FeddatHipError, match="EINVAL"):
                L.head_ln_gelu(x, gam, bet, eps, y, st, ge)
        if not what.startswith("eps"):
            stats = torch.zeros(rows, 2, device=DEV)
            with pytest.raises(L.FeddatHipError, match="EINVAL"):
                L.head_ln_bwd_full(dy, x, stats, gam, dx, dg, db)
        torch.cuda.synchronize()
    assert all(torch.isnan(flat).all() for flat, _ in outs)


# ------------------------------------------------------------------------------------------------ what the cases cover
def test_cases_cover_the_dispatch_matrix():
    """The (avec, bvec, jt, mode, pro, epi) tuples the cases assert (through the same assert_plan, at made-up addresses: the plan
    reads no memory): all twelve load / tile / mode paths, each prologue on a vector path -- tanh' also on a dword path -- in both
    modes, each epilogue at both jt."""
    from feddat_amd import lib
    paths = {assert_plan(lib, s, R.fake_job(lib, s)) for s in R.CASES}
    plain = {p[:4] for p in paths if p[4:] == (R.PRO_NONE, R.EPI_NONE)}
    assert plain >= {(a, b, jt, mode) for a in (0, 1) for b in (0, 1) for jt, mode in ((1, 0), (4, 0), (4, 1))}
    for mode in (0, 1):
        assert any(p[0] == 1 and p[3] == mode and p[4] == R.PRO_LN for p in paths)
        assert any(p[0] == 1 and p[3] == mode and p[4] == R.PRO_TANH_BWD for p in paths)
        assert any(p[0] == 0 and p[3] == mode and p[4] == R.PRO_TANH_BWD for p in paths)
    for epi in (R.EPI_TANH, R.EPI_MUL_DGELU):
        assert {p[2] for p in paths if p[5] == epi} == {1, 4}
    assert {p[2] for p in paths if p[4] == R.PRO_LN and p[3] == 0} == {1, 4}
