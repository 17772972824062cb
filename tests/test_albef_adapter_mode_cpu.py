"""ALBEF optimizer_mode 'adapter' (the single-adapter FedAvg baseline), the parts that need no device: key sets and shapes,
the trainable / communicated / personal / decayed name lists against the reference's own objects
(tests/golden/gb1_albef_adapter_small.npz, tools/make_albef_adapter_golden.py), the checkpoint loader, the engine's class layout,
and what train.main still refuses."""
import os

import numpy as np
import pytest
import torch

from feddat_amd import albef_spec, modes, weights
from feddat_amd import lib as L
from feddat_amd.local_update import _no_decay

SMALL = dict(vit_depth=2, enc_layers=3, fusion_layer=1, dec_layers=2, image=64, vocab=3072, max_pos=64)
CLS = "albef_model.albef.text_decoder.cls.predictions."
# state-dict keys of the reference's module that are no tensors of their own: buffers and the tied aliases of the LM head
ALIASES = ("position_ids", CLS + "decoder.weight", CLS + "decoder.bias")


@pytest.fixture(scope="module")
def gb1(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "gb1_albef_adapter_small.npz")))


def test_param_shapes_are_the_reference_modules(gb1):
    shapes = albef_spec.param_shapes(optimizer_mode="adapter", **SMALL)
    ref = {k: tuple(int(x) for x in dims.split(",")) for k, dims in zip(gb1["shapes.keys"].tolist(), gb1["shapes.dims"].tolist())
           if not any(a in k for a in ALIASES)}
    assert list(shapes) == list(ref)                   # the same keys in the same (state-dict) order
    assert shapes == ref
    ad = [k for k in shapes if "adapter" in k]
    assert len(ad) == 28 == 4 * 7 and all(".adapter.adapter_down." in k or ".adapter.adapter_up." in k for k in ad)
    assert albef_spec.ADAPTER_STEMS["adapter"] == ("adapter_",)
    # full size: the payload is as large as DAT's adapter_1
    full = albef_spec.param_shapes(optimizer_mode="adapter")
    assert sum(int(np.prod(s)) for k, s in full.items() if "adapter" in k) == 2236320
    with pytest.raises(ValueError):
        albef_spec.param_shapes(optimizer_mode="bias")


def test_dat_shapes_are_unchanged():
    dat = albef_spec.param_shapes(**SMALL)
    assert dat == albef_spec.param_shapes(optimizer_mode="dat", **SMALL)
    one = albef_spec.param_shapes(optimizer_mode="adapter", **SMALL)
    assert [k for k in dat if "adapter" not in k] == [k for k in one if "adapter" not in k]
    assert len([k for k in dat if "adapter" in k]) == 3 * 28
    keys = list(dat)
    got = modes.mode_names(keys, "dat")
    assert got == modes.mode_names(keys, "dat", albef=True)
    assert all("adapter_1" in k for k in got["communicated"]) and len(got["communicated"]) == 28
    assert [k for k in got["trainable"] if ".cls." in k] == [k for k in keys if ".cls." in k]
    r = albef_spec.random_init(seed=1, optimizer_mode="adapter", **SMALL)
    assert list(r) == list(one) and all(tuple(r[k].shape) == one[k] for k in one)


def test_mode_names_equal_the_reference_lists(gb1):
    keys = list(albef_spec.param_shapes(optimizer_mode="adapter", **SMALL))
    got = modes.mode_names(keys, "adapter", albef=True)
    drop = lambda names: [n for n in names if not any(a in n for a in ALIASES)]      # noqa: E731
    assert got["trainable"] == gb1["head.names.trainable"].tolist()
    assert got["communicated"] == gb1["head.names.communicated"].tolist() and len(got["communicated"]) == 28
    assert got["personal"] == drop(gb1["head.names.personal"].tolist()) and len(got["personal"]) == 5
    assert [n for n in got["trainable"] if not _no_decay(n)] == gb1["head.names.decayed"].tolist()
    # the head is never part of the payload; without albef=True the lists are the ViLT ones ('.cls.' is no head there)
    assert not set(got["communicated"]) & set(got["personal"])
    vilt = modes.mode_names(keys, "adapter")
    assert vilt["communicated"] == got["communicated"] and vilt["personal"] == [] and vilt["trainable"] == got["communicated"]
    # the fixture's frozen-head run: the reference's modules with the '.cls.' flags cleared
    assert gb1["nohead.names.trainable"].tolist() == got["communicated"]


def test_load_albef_pretrained_builds_the_single_adapter(tmp_path):
    """On the synthetic ALBEF.pth of tests/ckpt_util.py (what tests/test_weights.py loads in dat mode)."""
    from tests import ckpt_util
    from tests.test_weights import ALBEF_DIMS as dims
    path = ckpt_util.write_albef_checkpoint(str(tmp_path / "ALBEF.pth"), vit_depth=dims["vit_depth"], enc_layers=dims["enc_layers"],
                                            pre_image=48, vocab=dims["vocab"], max_pos=dims["max_pos"])
    shapes = albef_spec.param_shapes(optimizer_mode="adapter", **dims)
    P = weights.load_albef_pretrained(path, seed=0, optimizer_mode="adapter", **dims)
    assert sorted(P) == sorted(shapes) and all(tuple(P[k].shape) == shapes[k] for k in shapes)
    ad = [k for k in P if "adapter" in k]
    assert len(ad) == 4 * (dims["vit_depth"] + dims["enc_layers"] + dims["dec_layers"])
    assert all(float(P[k].abs().max()) == 0.0 for k in ad if k.endswith("bias"))
    assert all(float(P[k].abs().max()) > 0.0 for k in ad if k.endswith("weight"))
    D = weights.load_albef_pretrained(path, seed=0, **dims)
    assert sorted(D) == sorted(albef_spec.param_shapes(**dims))
    assert all(torch.equal(D[k], P[k]) for k in P if "adapter" not in k)


def test_engine_layout():
    from feddat_amd import albef_adapter_engine, albef_backbone, albef_engine
    E = albef_adapter_engine.AlbefAdapterEngine
    assert issubclass(E, albef_engine.AlbefDatEngine)
    assert E.ADAPTER_STEMS == ("adapter_",) == albef_spec.ADAPTER_STEMS["adapter"] and E.COMM_ADAPTER == 0
    assert E.ACT_SETS == ("adapter",) and E.FROZEN_ADAPTERS == ()
    B = albef_backbone.AlbefBackbone
    assert B.ADAPTER_STEMS == albef_spec.ADAPTER_STEMS["dat"] and B.ACT_SETS == ("gating", "adapter_1") and B.FROZEN_ADAPTERS == (2,)
    assert E._mode_segments("adapter", 9) == [(0, 9, [(0, 1.0)])]
    for mode in ("gating", "adapter_0", "adapter_1", "both"):
        with pytest.raises(L.FeddatHipError):
            E._mode_segments(mode, 9)
    # the backward is the DAT engine's own, not a copy
    for name in ("_bert_bwd", "_vit_bwd", "_towers_bwd", "_lm_head_bwd", "_wgrad", "_wgrad_reduce", "train_step"):
        assert getattr(E, name) is getattr(albef_engine.AlbefDatEngine, name), name
    with pytest.raises(L.FeddatHipError, match="stack"):
        E({}, "cpu", batch=2, n_answers=2, stack_text=True)


def test_main_still_refuses_the_combination():
    from feddat_amd import train
    with pytest.raises(L.FeddatHipError, match="ALBEF supports only"):
        train.main(["--encoder_name", "albef_no_distill", "--optimizer_mode", "adapter"])
