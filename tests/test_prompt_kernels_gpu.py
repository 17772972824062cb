"""The prompt-tuning entry points one by one against float64 restatements in torch (csrc/prompt.hip: feddat_prompt_frame_assemble,
feddat_prompt_grad_gather; lib.prompt_mlp_fwd / prompt_mlp_bwd: the MLP's products as feddat_head_gemm jobs), in both operand
builds (everything here is fp32; the two libraries must agree with the restatement alike).

Bounds are derived, not measured.  An fp32 dot product of length K, whatever its summation order, is within
K * 2^-24 * sum_i |a_i| |b_i| of the exact value (u = 2^-24, first order in u); the sum is evaluated in float64.  An output behind
the tanh (t; P, which reads t) or behind its derivative (dz = dt * (1 - t^2) and what reads it: dW1, db1, dE) gets twice that: tanh
is 1-Lipschitz and its fp32 evaluation, the 1 - t^2 factor and the product with it add a few u on top of the dot product's K u.
Every product is checked against the float64 value of the operands it actually read (the entry point's own t resp. dt buffers for
its second stage), so each bound is the bound of ONE product.  The gather sums 2 B terms per element: 2 B * 2^-24 * sum |terms|.
"""
import pytest
import torch

from feddat_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
H, D, NP = 768, 192, 5
SHAPES = [(40, 49), (3, 1)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def _mlp_weights(seed):
    g = _gen(seed)
    E = torch.randn(NP, H, generator=g)
    W1 = (2 * torch.rand(D, H, generator=g) - 1) * H ** -0.5
    b1 = (2 * torch.rand(D, generator=g) - 1) * H ** -0.5
    W2 = (2 * torch.rand(H, D, generator=g) - 1) * D ** -0.5
    b2 = (2 * torch.rand(H, generator=g) - 1) * D ** -0.5
    return [t.to(DEV) for t in (E, W1, b1, W2, b2)]


def _within(got, ref64, bound64, what):
    err = (got.double() - ref64).abs()
    ratio = float((err / bound64.clamp_min(1e-300)).max())
    print(f"   {what}: max err {float(err.max()):.3e}, worst err / bound {ratio:.3f}")
    assert bool((err <= bound64).all()), (what, float(err.max()), ratio)


# ------------------------------------------------------------------------------------------------------- MLP forward / backward
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_mlp_forward_vs_float64(fmt):
    E, W1, b1, W2, b2 = _mlp_weights(1)
    t, P = torch.full((NP, D), 7.0, device=DEV), torch.full((NP, H), 7.0, device=DEV)
    with L.operands(fmt):
        L.prompt_mlp_fwd(E, W1, b1, W2, b2, t, P)
    torch.cuda.synchronize()
    Ed, W1d, W2d = E.double(), W1.double(), W2.double()
    z = Ed @ W1d.T + b1.double()
    _within(t, torch.tanh(z), 2 * H * U * (Ed.abs() @ W1d.abs().T + b1.double().abs()), "t = tanh(E W1^T + b1)")
    td = t.double()      # the operand the second product read
    _within(P, td @ W2d.T + b2.double(), 2 * D * U * (td.abs() @ W2d.abs().T + b2.double().abs()), "P = t W2^T + b2")
    # and the chain as a whole agrees with float64 to fp32 accuracy
    ref = torch.tanh(z) @ W2d.T + b2.double()
    assert float((P.double() - ref).abs().max()) < 1e-4


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_mlp_backward_vs_float64(fmt):
    E, W1, b1, W2, b2 = _mlp_weights(2)
    g = _gen(3)
    G = (torch.randn(NP, H, generator=g) * 1e-3).to(DEV)
    # t as the forward leaves it for these weights (pre-activations of standard deviation ~0.6, |t| < 0.97)
    t = torch.tanh(E.double() @ W1.double().T + b1.double()).float()
    # the outputs are slices of one flat buffer, as the engine's gradient group holds them, with canaries between and around
    sizes = [NP * H, D * H, D, H * D, H]
    flat = torch.full((sum(sizes) + 4 * (len(sizes) + 1),), 3.25, device=DEV)
    outs, o = [], 4
    for n in sizes:
        outs.append(flat[o:o + n])
        o += n + 4
    dE, dW1, db1, dW2, db2 = outs[0].view(NP, H), outs[1].view(D, H), outs[2], outs[3].view(H, D), outs[4]
    dt = torch.zeros(NP, D, device=DEV)
    with L.operands(fmt):
        L.prompt_mlp_bwd(G, t, E, W1, W2, dt, dE, dW1, db1, dW2, db2)
    torch.cuda.synchronize()
    Gd, td, Ed, W1d, W2d = (x.double() for x in (G, t, E, W1, W2))
    _within(dW2, Gd.T @ td, NP * U * (Gd.abs().T @ td.abs()), "dW2 = G^T t")
    _within(db2, Gd.sum(0), NP * U * Gd.abs().sum(0), "db2 = sum_j G")
    _within(dt, Gd @ W2d, H * U * (Gd.abs() @ W2d.abs()), "dt = G W2")
    dz = dt.double() * (1 - td * td)      # from the dt the second stage read
    _within(dW1, dz.T @ Ed, 2 * NP * U * (dz.abs().T @ Ed.abs()), "dW1 = dz^T E")
    _within(db1, dz.sum(0), 2 * NP * U * dz.abs().sum(0), "db1 = sum_j dz")
    _within(dE, dz @ W1d, 2 * D * U * (dz.abs() @ W1d.abs()), "dE = dz W1")
    # canaries: nothing outside the five slices was written
    keep = torch.ones_like(flat, dtype=torch.bool)
    o = 4
    for n in sizes:
        keep[o:o + n] = False
        o += n + 4
    assert bool((flat[keep] == 3.25).all())
    # the whole chain against autograd in float64
    Ea, W1a, b1a, W2a, b2a = (x.double().requires_grad_() for x in (E, W1, b1, W2, b2))
    ta = torch.tanh(Ea @ W1a.T + b1a)
    ((ta @ W2a.T + b2a) * Gd).sum().backward()
    for got, ref, name in ((dE, Ea.grad, "dE"), (dW1, W1a.grad, "dW1"), (db1, b1a.grad, "db1"), (dW2, W2a.grad, "dW2"),
                           (db2, b2a.grad, "db2")):
        scale = float(ref.abs().max())
        assert float((got.double() - ref).abs().max()) < 1e-5 * scale, name


# ------------------------------------------------------------------------------------------------------- frame assemble
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("nrep", [1, 2])
@pytest.mark.parametrize("Lt,Np", SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_frame_assemble_is_bit_exact_and_stays_inside(B, Lt, Np, nrep, fmt):
    g = _gen(10 * B + Lt)
    S0, S = Lt + 1 + Np, Lt + Np + 11
    h_in = torch.randn(B, S0, H, generator=g).to(DEV)
    km_in = (torch.rand(B, S0, generator=g) < 0.7).to(torch.uint8).to(DEV)
    P, mod0, mod1 = (torch.randn(n, generator=g).to(DEV) for n in ((NP, H), (H,), (H,)))
    pad = 2 * H      # canary floats / bytes before and after each output
    hbuf = torch.full((pad + B * S * H + pad,), -123.5, device=DEV)
    mbuf = torch.full((pad + nrep * B * S + pad,), 77, dtype=torch.uint8, device=DEV)
    h_out, km_out = hbuf[pad:pad + B * S * H], mbuf[pad:pad + nrep * B * S]
    with L.operands(fmt):
        L.prompt_frame_assemble(h_in, km_in, P, mod0, mod1, h_out, km_out, B, Lt, Np, H, nrep=nrep)
    torch.cuda.synchronize()
    got, gm = h_out.view(B, S, H), km_out.view(nrep, B, S)
    rows = L.prompt_row_map(Lt, Np)
    assert len(rows) == S
    want = torch.empty(B, S, H, device=DEV)
    wm = torch.empty(B, S, dtype=torch.uint8, device=DEV)
    for s, r in enumerate(rows):
        if r[0] == "src":
            want[:, s], wm[:, s] = h_in[:, r[1]], km_in[:, r[1]]
        else:
            want[:, s], wm[:, s] = P[r[1]] + (mod0, mod1)[r[2]], 1      # one fp32 add
    assert torch.equal(got, want)
    for rep in range(nrep):
        assert torch.equal(gm[rep], wm)
    assert bool((hbuf[:pad] == -123.5).all()) and bool((hbuf[-pad:] == -123.5).all())
    assert bool((mbuf[:pad] == 77).all()) and bool((mbuf[-pad:] == 77).all())
    # no key mask asked for: the frame alone, nothing else
    hbuf.fill_(-123.5)
    with L.operands(fmt):
        L.prompt_frame_assemble(h_in, None, P, mod0, mod1, h_out, None, B, Lt, Np, H)
    torch.cuda.synchronize()
    assert torch.equal(h_out.view(B, S, H), want) and bool((hbuf[:pad] == -123.5).all()) and bool((hbuf[-pad:] == -123.5).all())


# ------------------------------------------------------------------------------------------------------- gradient gather
def _gather_ref(dh, Lt, us):
    d = dh.double()
    terms = torch.stack([d[:, 1:6], d[:, Lt + 6:Lt + 11]], 1)      # [B, 2, 5, H]
    return terms.sum((0, 1)) * us, terms.abs().sum((0, 1)) * us


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("Lt,Np", SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_grad_gather_vs_float64(B, Lt, Np, fmt):
    g = _gen(100 * B + Lt)
    S = Lt + Np + 11
    dh = torch.randn(B, S, H, generator=g).to(DEV)
    inv = torch.tensor([2.0 ** -14], device=DEV)
    one = torch.tensor([1.0], device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    buf = torch.full((8 + NP * H + 8,), 9.5, device=DEV)
    G = buf[8:8 + NP * H]
    # the two factors: host scalar x device scalar, each 1 or 2^-14
    for us_host, us_dev, us in ((1.0, None, 1.0), (2.0 ** -14, None, 2.0 ** -14), (1.0, inv, 2.0 ** -14), (1.0, one, 1.0),
                                (2.0 ** -14, inv, 2.0 ** -28)):
        with L.operands(fmt):
            L.prompt_grad_gather(dh, B, S, Lt, H, G, us_host, us_dev, flag)
        torch.cuda.synchronize()
        ref, mag = _gather_ref(dh, Lt, us)
        _within(G.view(NP, H), ref, 2 * B * U * mag, f"gather x {us:g}")
        first = G.clone()
        with L.operands(fmt):
            L.prompt_grad_gather(dh, B, S, Lt, H, G, us_host, us_dev, flag)
        torch.cuda.synchronize()
        assert torch.equal(first, G)      # two runs, the same bits
    assert int(flag) == 0 and bool((buf[:8] == 9.5).all()) and bool((buf[-8:] == 9.5).all())
    # the summation order is the documented one: b ascending, text row before image row
    acc = torch.zeros(NP, H, device=DEV)
    for b in range(B):
        acc = acc + dh[b, 1:6]
        acc = acc + dh[b, Lt + 6:Lt + 11]
    with L.operands(fmt):
        L.prompt_grad_gather(dh, B, S, Lt, H, G)
    torch.cuda.synchronize()
    assert torch.equal(G.view(NP, H), acc)


@pytest.mark.parametrize("Lt,Np", SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_grad_gather_flags_only_what_it_reads(B, Lt, Np):
    g = _gen(7)
    S = Lt + Np + 11
    dh = torch.randn(B, S, H, generator=g).to(DEV)
    G = torch.zeros(NP, H, device=DEV)
    prompt_rows = set(range(1, 6)) | set(range(Lt + 6, Lt + 11))
    # an inf in EVERY non-prompt row: not read, so no flag and a finite, unchanged result
    L.prompt_grad_gather(dh, B, S, Lt, H, G)
    clean = G.clone()
    bad = dh.clone()
    for s in range(S):
        if s not in prompt_rows:
            bad[:, s, ::7] = float("inf")
            bad[:, s, 1::7] = float("nan")
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.prompt_grad_gather(bad, B, S, Lt, H, G, 1.0, None, flag)
    torch.cuda.synchronize()
    assert int(flag) == 0 and torch.equal(G, clean)
    # an inf / NaN in one prompt row, text side or image side, last sample: the flag goes up (and is never cleared here)
    for s, v in ((3, float("inf")), (Lt + 10, float("nan")), (Lt + 6, float("-inf"))):
        bad = dh.clone()
        bad[B - 1, s, H - 1] = v
        flag.zero_()
        L.prompt_grad_gather(bad, B, S, Lt, H, G, 1.0, None, flag)
        torch.cuda.synchronize()
        assert int(flag) == 1, (s, v)
        L.prompt_grad_gather(dh, B, S, Lt, H, G, 1.0, None, flag)
        torch.cuda.synchronize()
        assert int(flag) == 1 and torch.equal(G, clean)
    # without a flag pointer the kernel just writes
    L.prompt_grad_gather(bad, B, S, Lt, H, G)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(G).all())
