"""Host-side pieces of optimizer_mode 'adapter' (no GPU): the name sets per mode, the shapes / init of the single adapter, the
reference's scheduler behaviour under overflow (tests/golden/ga3), a federation checkpoint round trip, and the C ABI
additions (declared, exported, bound)."""
import os
import re

import numpy as np
import pytest
import torch

from feddat_amd import lib as L
from feddat_amd.modes import mode_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("feddat_bce_loss_fwd_bwd", "feddat_single_step_finish")


def _keys(mode, layers=2, tasks=("art", "gqa")):
    from feddat_amd import vilt_spec
    return list(vilt_spec.param_shapes(layers, tasks, optimizer_mode=mode))


def test_name_sets_per_mode():
    keys = _keys("adapter", layers=12, tasks=("art",))
    s = mode_names(keys, "adapter")
    ad = [k for k in keys if ".output.adapter.adapter_" in k]
    assert len(ad) == 48 and all(re.search(r"adapter\.adapter_(down|up)\.(weight|bias)$", k) for k in ad)
    assert s["communicated"] == ad
    assert s["personal"] == [k for k in keys if k.startswith("task_layer.")]
    assert s["trainable"] == ad + s["personal"]
    shapes = __import__("feddat_amd.vilt_spec", fromlist=["x"]).param_shapes(12, ("art",), optimizer_mode="adapter")
    assert sum(int(np.prod(shapes[k])) for k in s["communicated"]) == 894528
    d = mode_names(_keys("dat", layers=12, tasks=("art",)), "dat")
    assert all("adapter_1" in k for k in d["communicated"]) and len(d["communicated"]) == 48
    assert not any("adapter_1" in k for k in d["personal"]) and any("adapter_2" in k for k in d["personal"])
    assert not any("adapter_2" in k for k in d["trainable"])
    with pytest.raises(L.FeddatHipError):
        mode_names(keys, "lora")


def test_reference_key_lists(golden_dir):
    """The fixtures' key lists are the reference model's: the communicated set of ga4 is every 'adapter' key of a 2-layer
    model, its personal set the heads."""
    g = np.load(os.path.join(golden_dir, "ga4_round_2clients.npz"))
    server = sorted(k[len("r0.server.dall::"):] for k in g.files if k.startswith("r0.server.dall::"))
    assert server == sorted(mode_names(_keys("adapter", tasks=("art", "abstract")), "adapter")["communicated"])
    heads = [k.split("::")[-1][len("r0.art."):] for k in g.files if k.split("::")[-1].startswith("r0.art.")]
    assert sorted(set(heads)) == sorted(k for k in mode_names(_keys("adapter", tasks=("art", "abstract")), "adapter")["personal"]
                                        if k.startswith("task_layer.art."))


def test_random_init_adapter_mode():
    from feddat_amd import vilt_spec
    P = vilt_spec.random_init(2, ("art",), seed=3, optimizer_mode="adapter")
    k = vilt_spec.ENC + "encoder.layer.1.output.adapter.adapter_"
    assert P[k + "down.weight"].shape == (48, 768) and P[k + "up.weight"].shape == (768, 48)
    assert torch.count_nonzero(P[k + "down.bias"]) == 0 and torch.count_nonzero(P[k + "up.bias"]) == 0
    assert 0.015 < float(P[k + "down.weight"].std()) < 0.025
    assert not any("adapter_0" in n or "adapter_2" in n for n in P)
    # the dat initialisation is unchanged by the mode switch
    a = vilt_spec.random_init(2, ("art",), seed=3)
    b = vilt_spec.random_init(2, ("art",), seed=3, optimizer_mode="dat")
    assert a.keys() == b.keys() and all(torch.equal(a[n], b[n]) for n in a)


def test_ga3_scheduler_moves_once_per_applied_batch(golden_dir):
    g = np.load(os.path.join(golden_dir, "ga3_scaler_skip.npz"))
    over = set(g["overflow_steps"].tolist())
    t, scale, want_t, want_scale = 0, 65536.0, [], []
    for s in range(len(g["losses"])):
        if s in over:
            scale *= 0.5
        else:
            t += 1
        want_t.append(t)
        want_scale.append(scale)
    assert g["sched_t"].tolist() == want_t and g["scale"].tolist() == want_scale


def test_federation_checkpoint_round_trip(tmp_path):
    from feddat_amd import checkpoint, vilt_spec
    P = vilt_spec.random_init(2, ("art", "gqa"), seed=5, optimizer_mode="adapter")
    names = mode_names(list(P), "adapter")
    comm = {k: P[k] for k in names["communicated"]}
    pers = {t: {k: P[k] + 1.0 for k in names["personal"]} for t in ("art", "gqa")}
    checkpoint.save_federation(str(tmp_path), {}, pers, 3, write_server=False)
    checkpoint.save_federation(str(tmp_path), comm, {}, 3, server_flags={0: True})
    c2, p2, last, flags = checkpoint.load_federation(str(tmp_path), ["art", "gqa"])
    assert last == 3 and flags == {0: True}
    assert c2.keys() == comm.keys() and all(torch.equal(c2[k], comm[k]) for k in comm)
    for t in pers:
        assert p2[t].keys() == pers[t].keys() and all(torch.equal(p2[t][k], pers[t][k]) for k in pers[t])


def test_new_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "feddat_hip.h")).read()
    from feddat_amd import build
    import ctypes
    lib = ctypes.CDLL(build.build())
    for n in NEW_SYMBOLS:
        assert re.search(rf"^int {n}\(", src, flags=re.M), n
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n), n
    assert lib.feddat_abi_version() == 8
    assert callable(L.bce_loss_fwd_bwd) and callable(L.single_step_finish)


def test_adapter_mode_ops_need_a_device():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(L.FeddatHipError):
        L.bce_loss_fwd_bwd(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(4))


def test_main_refuses_albef_adapter_and_other_modes():
    from feddat_amd import train
    with pytest.raises(L.FeddatHipError, match="ALBEF supports only"):
        train.main(["--encoder_name", "albef_no_distill", "--optimizer_mode", "adapter"])
    with pytest.raises(L.FeddatHipError):
        train.main(["--optimizer_mode", "lora"])


def test_allreduce_average_tells_the_engine_through_comm_written(tmp_path, monkeypatch):
    """fedavg.allreduce_average on an engine whose averaged adapter is slot 0 (ViltAdapterEngine.COMM_ADAPTER): after the write-back
    it calls the engine's comm_written() once, whose default rebuilds the operand copies of slot COMM_ADAPTER -- never slot 1.
    One-rank gloo group, the HIP pre-scale replaced by test_fedavg_gloo's host stand-in (same operation order)."""
    import torch.distributed as dist
    from feddat_amd import fedavg
    from feddat_amd.local_update import LocalUpdateEngine

    class Stub(LocalUpdateEngine):
        COMM_ADAPTER = 0

        def __init__(self):
            self.flat = torch.randn(4096, generator=torch.Generator().manual_seed(3))
            self.written, self.repacked = 0, []

        def comm_flat(self):
            return self.flat

        def comm_written(self):
            self.written += 1
            super().comm_written()

        def repack_adapter(self, a):
            self.repacked.append(a)

    monkeypatch.setattr(fedavg.L, "fedavg_accumulate", lambda acc, x, num, total, first: acc.copy_(x * num / total))
    eng = Stub()
    sent = eng.flat.clone()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/rendezvous", rank=0, world_size=1)
    try:
        out = fedavg.allreduce_average(eng, 1)
    finally:
        dist.destroy_process_group()
    assert out is eng.flat and torch.equal(eng.flat, sent)
    assert eng.written == 1
    assert eng.repacked == [0]
