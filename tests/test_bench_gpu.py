"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, written so that two runs (or two builds) of the
benchmark can be compared output for output.  Same arguments -> same inputs -> the same bits; and the files hold the state of
the LAST timed step, not of anything bench.py runs after the timed region.  And what a plain run leaves to `--full`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, RES, STEPS, WARMUP = 4, 224, 3, 2


def _run(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--batch", str(B), "--res", str(RES), *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def _bench(out_dir):
    return _run("--no-roofline", "--no-cpu-baseline", "--dump-outputs", str(out_dir))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


@pytest.mark.timeout(900)
def test_dump_outputs_repeat_bit_for_bit_and_hold_the_last_timed_step(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    line = _bench(tmp_path / "a")
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["ms_per_step"] > 0
    a = _load(tmp_path / "a")
    assert line["dump_outputs"]["arrays"] == len(a) and sum(v.nbytes for v in a.values()) <= 64 << 20
    assert all(v.dtype == np.float32 for v in a.values())
    _bench(tmp_path / "b")
    b = _load(tmp_path / "b")
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k

    # the same W + K steps on the engine, set up as bench.py sets up its default line
    from feddat_amd import engine, vilt_spec
    dev = torch.device("cuda", 0)
    params = vilt_spec.random_init(12, ["client0"], seed=0, device="cpu")
    eng = engine.ViltDatEngine(params, ["client0"], dev, batch=B, res=RES, layers=12, operands="f16")
    batches = [vilt_spec.synthetic_batch(B, RES, 1234 + i, device=dev) for i in range(4)]
    eng.begin_local_update("client0", steps_per_epoch=max(STEPS + WARMUP, 40))
    for i in list(range(WARMUP)) + list(range(STEPS)):
        loss = eng.train_step(batches[i % 4], use_graph=True)
    torch.cuda.synchronize()
    # loss_0, KL, L_0; the buffer's tail is scratch of the loss kernels and is not part of the dump
    assert a["loss"].shape == (3,), a["loss"]
    assert np.allclose(a["loss"], loss[:3].float().cpu().numpy(), rtol=1e-6, atol=0), (a["loss"], loss)
    sd = eng.state_dict()
    assert {"state." + k for k in sd} | {"loss"} == set(a)
    init = {k: params[k].float().numpy() for k in sd}
    moved = 0
    for k, v in sd.items():
        got = v.float().cpu().numpy()
        assert np.abs(a["state." + k] - got).max() <= 1e-6, k
        moved += int(not np.array_equal(a["state." + k], init[k]))
    assert moved > 0


AUX = ("other_operand_format", "roofline", "cpu_baseline")


@pytest.mark.timeout(900)
def test_plain_line_is_the_headline_and_full_adds_the_auxiliary_figures():
    """A plain run prints the headline figures only; --full adds the other operand format, the in-step roofline and the CPU
    baseline, each measured, not an error record."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    plain = _run()
    assert not set(AUX) & set(plain), sorted(plain)
    full = _run("--full")
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert full[k] == plain[k], k
    assert full["value"] > 0 and full["ms_per_step"] > 0
    for k in AUX:
        assert k in full and "error" not in full[k], (k, full.get(k))
    assert full["other_operand_format"]["operands"] == "bf16" and full["other_operand_format"]["ms_per_step"] > 0
    assert full["roofline"]["achieved"] > 0 and full["cpu_baseline"]["value"] > 0
