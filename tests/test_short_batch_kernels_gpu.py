"""The three entry points a short last batch adds (include/feddat_hip.h: feddat_vilt_pad_batch, feddat_dat_loss_fwd_bwd_rows,
feddat_bce_loss_fwd_bwd_rows), in both operand builds.  Everything here is an exact statement: copies and untouched bytes are
torch.equal, the valid rows of the _rows losses carry the bits of the existing kernels on the n-row views, the tail rows are 0.0."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPERANDS = ("f16", "bf16")
PATCH_ELEMS = 3 * 32 * 32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(shape, dtype, g):
    """Random bit patterns (NaN payloads included: a copy must move bits, not values)."""
    if dtype in (torch.float16, torch.bfloat16):
        return torch.randint(-32768, 32767, shape, generator=g, dtype=torch.int16).view(dtype)
    if dtype == torch.int64:
        return torch.randint(-2 ** 62, 2 ** 62, shape, generator=g, dtype=torch.int64)
    return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int32).view(torch.float32)


def _same(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _pad_buffers(B, n_patches, Lt, C, dtype, seed):
    """Every input of a step for B samples plus ONE sentinel sample behind each: {name: [B + 1, per-sample elements]}."""
    g = torch.Generator().manual_seed(seed)
    return {"patches": _bits((B + 1, n_patches * PATCH_ELEMS), dtype, g).to(DEV),
            "input_ids": _bits((B + 1, Lt), torch.int64, g).to(DEV),
            "token_type_ids": _bits((B + 1, Lt), torch.int64, g).to(DEV),
            "attention_mask": _bits((B + 1, Lt), torch.int64, g).to(DEV),
            "patch_mask": _bits((B + 1, n_patches), torch.int64, g).to(DEV),
            "target": _bits((B + 1, C), torch.float32, g).to(DEV)}


def _call_pad(L, buf, n, B, n_patches):
    inp = {k: v[:B] for k, v in buf.items() if k != "patches"}
    return L.vilt_pad_batch_rc(buf["patches"][:B].view(B * n_patches, PATCH_ELEMS), inp, n, B)


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("n_patches,Lt,C", [(49, 40, 100), (240, 16, 6)])
@pytest.mark.parametrize("n,B", [(1, 2), (3, 4), (2, 5), (4, 4)])
def test_pad_batch_replicates_the_valid_samples(operands, n_patches, Lt, C, n, B):
    """(49, 40, 100): patch_mask samples of 392 bytes, so every odd sample is 8-byte aligned only; (240, 16, 6): target samples of
    24 bytes.  Both take the 4-byte path next to the 16-byte one of the patch matrix and the text inputs."""
    from feddat_amd import lib as L
    buf = _pad_buffers(B, n_patches, Lt, C, L.OPERAND_DTYPE[operands], 100 * n + B)
    before = {k: v.clone() for k, v in buf.items()}
    with L.operands(operands):
        assert _call_pad(L, buf, n, B, n_patches) == 0
    torch.cuda.synchronize()
    for k, v in buf.items():
        for j in range(n, B):
            assert _same(v[j], before[k][j % n]), (k, j)
        assert _same(v[:n], before[k][:n]), k
        assert _same(v[B], before[k][B]), (k, "sentinel")


@pytest.mark.parametrize("operands", OPERANDS)
def test_pad_batch_refuses_a_row_count_outside_the_frame(operands):
    from feddat_amd import lib as L
    B, n_patches = 4, 49
    buf = _pad_buffers(B, n_patches, 40, 100, L.OPERAND_DTYPE[operands], 7)
    before = {k: v.clone() for k, v in buf.items()}
    with L.operands(operands):
        for n in (0, B + 1, -3):
            assert _call_pad(L, buf, n, B, n_patches) == 1      # FEDDAT_EINVAL
        with pytest.raises(L.FeddatHipError):
            L.vilt_pad_batch(buf["patches"][:B].view(B * n_patches, PATCH_ELEMS), {k: v[:B] for k, v in buf.items()}, 0, B)
    torch.cuda.synchronize()
    assert all(_same(v, before[k]) for k, v in buf.items())


LOSS_CASES = [(1, 2, 100), (3, 4, 100), (3, 4, 6), (31, 32, 100), (4, 4, 100)]


def _loss_inputs(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    lg = (torch.randn(B, C, generator=g) * 2).to(DEV)
    te = (torch.randn(B, C, generator=g) * 2).to(DEV)
    ta = ((torch.rand(B, C, generator=g) < 0.05).float() * torch.rand(B, C, generator=g)).to(DEV)
    return lg, te, ta


def _flag():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("n,B,C", LOSS_CASES)
def test_dat_loss_rows(operands, n, B, C):
    from feddat_amd import lib as L
    lg, te, ta = _loss_inputs(B, C, 1000 * n + B + C)
    with L.operands(operands):
        dl_ref, sc_ref, f_ref = torch.empty(n, C, device=DEV), torch.zeros(4, device=DEV), _flag()
        L.dat_loss_fwd_bwd_checked(lg[:n], te[:n], ta[:n], dl_ref, sc_ref, f_ref)

        def run(lg, te, ta, flag=True):
            dl, sc, f = torch.full((B, C), float("nan"), device=DEV), torch.zeros(4, device=DEV), _flag()
            L.dat_loss_fwd_bwd_rows(lg, te, ta, dl, sc, n, f if flag else None)
            torch.cuda.synchronize()
            return dl, sc, int(f[0])
        dl, sc, f = run(lg, te, ta)
        assert torch.equal(dl[:n], dl_ref) and torch.equal(sc[:3], sc_ref[:3]) and f == 0 == int(f_ref[0])
        assert torch.equal(dl[n:], torch.zeros(B - n, C, device=DEV))
        assert bool(torch.isfinite(sc[:3]).all())
        dl2, sc2, _ = run(lg, te, ta, flag=False)      # nonfinite = NULL: the static-scale / unfused-tail configurations
        assert torch.equal(dl2, dl) and torch.equal(sc2[:3], sc[:3])
        if n < B:      # rows >= n are never read: inf / NaN there change nothing, and the flag follows the valid rows only
            lg2, te2, ta2 = lg.clone(), te.clone(), ta.clone()
            lg2[n:, ::3], lg2[n:, 1::3] = float("inf"), float("nan")
            te2[n:], ta2[n:] = float("nan"), float("inf")
            dl3, sc3, f3 = run(lg2, te2, ta2)
            assert f3 == 0 and bool(torch.isfinite(sc3[:3]).all())
            assert torch.equal(dl3, dl) and torch.equal(sc3[:3], sc[:3])
        lg4 = lg.clone()
        lg4[n - 1, C // 2] = float("inf")
        assert run(lg4, te, ta)[2] == 1


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("n,B,C", LOSS_CASES)
def test_bce_loss_rows(operands, n, B, C):
    from feddat_amd import lib as L
    lg, _, ta = _loss_inputs(B, C, 2000 * n + B + C)
    with L.operands(operands):
        dl_ref, sc_ref, f_ref = torch.empty(n, C, device=DEV), torch.zeros(4, device=DEV), _flag()
        L.bce_loss_fwd_bwd(lg[:n], ta[:n], dl_ref, sc_ref, f_ref)

        def run(lg, ta, flag=True):
            dl, sc, f = torch.full((B, C), float("nan"), device=DEV), torch.zeros(4, device=DEV), _flag()
            L.bce_loss_fwd_bwd_rows(lg, ta, dl, sc, n, f if flag else None)
            torch.cuda.synchronize()
            return dl, sc, int(f[0])
        dl, sc, f = run(lg, ta)
        assert torch.equal(dl[:n], dl_ref) and torch.equal(sc[:1], sc_ref[:1]) and f == 0 == int(f_ref[0])
        assert torch.equal(dl[n:], torch.zeros(B - n, C, device=DEV))
        assert bool(torch.isfinite(sc[:1]).all())
        dl2, sc2, _ = run(lg, ta, flag=False)
        assert torch.equal(dl2, dl) and torch.equal(sc2[:1], sc[:1])
        if n < B:
            lg2, ta2 = lg.clone(), ta.clone()
            lg2[n:, ::2], lg2[n:, 1::2] = float("inf"), float("nan")
            ta2[n:] = float("nan")
            dl3, sc3, f3 = run(lg2, ta2)
            assert f3 == 0 and bool(torch.isfinite(sc3[:1]).all())
            assert torch.equal(dl3, dl) and torch.equal(sc3[:1], sc[:1])
        lg4 = lg.clone()
        lg4[n - 1, C // 2] = float("inf")
        assert run(lg4, ta)[2] == 1


def test_rows_losses_refuse_a_row_count_outside_the_frame():
    from feddat_amd import lib as L
    lg, te, ta = _loss_inputs(4, 100, 5)
    dl, sc = torch.zeros(4, 100, device=DEV), torch.zeros(4, device=DEV)
    for n in (0, 5):
        with pytest.raises((L.FeddatHipError, AssertionError)):
            L.dat_loss_fwd_bwd_rows(lg, te, ta, dl, sc, n)
        with pytest.raises((L.FeddatHipError, AssertionError)):
            L.bce_loss_fwd_bwd_rows(lg, ta, dl, sc, n)
    torch.cuda.synchronize()
    assert not bool(dl.any()) and not bool(sc.any())
