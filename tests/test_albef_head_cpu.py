"""Host-side pieces of the trainable ALBEF LM head (no GPU): the name rules against the reference's own lists
(tests/golden/gh1_albef_head_small.npz: prepare_model's statements executed on the reference model, tools/make_albef_head_golden.py),
the head group's layout and weight decay, train.main's option, and the new entry point feddat_lm_head_refresh -- declared,
exported, bound in both builds, and checking its arguments."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from feddat_amd import lib as L
from feddat_amd.albef_engine import LM_HEAD, lm_head_group_spec
from feddat_amd.local_update import FlatGroup
from feddat_amd.modes import mode_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
HEAD = [LM_HEAD + n for n in ("bias", "transform.dense.weight", "transform.dense.bias", "transform.LayerNorm.weight",
                              "transform.LayerNorm.bias")]
ALIASES = [LM_HEAD + "decoder.weight", LM_HEAD + "decoder.bias"]        # tied: state_dict keys, not parameters of their own


@pytest.fixture(scope="module")
def names(golden_dir):
    g = np.load(os.path.join(golden_dir, "gh1_albef_head_small.npz"))
    return {k: [str(n) for n in g["names." + k]] for k in ("trainable", "communicated", "personal", "decayed")}


def test_mode_names_reproduce_the_references_lists(names):
    """mode_names(keys, "dat") on the fixture's key list (every key any of the reference's lists names) gives the reference's
    trainable and personal lists minus the two tied aliases, and its communicated list unchanged: the adapter_1 keys alone."""
    keys = list(dict.fromkeys(names["personal"] + names["trainable"] + names["communicated"]))
    assert all(a in names["personal"] for a in ALIASES) and not any(a in names["trainable"] for a in ALIASES)
    own = [k for k in keys if k not in ALIASES]
    got = mode_names(own, "dat")
    assert sorted(got["trainable"]) == sorted(names["trainable"])
    assert sorted(got["personal"]) == sorted(n for n in names["personal"] if n not in ALIASES)
    assert got["communicated"] == [k for k in own if k in names["communicated"]] and len(got["communicated"]) == len(names["communicated"])
    assert all("adapter_1" in k for k in got["communicated"]) and len(got["communicated"]) == 4 * (2 + 3 + 2)
    assert sorted(k for k in got["trainable"] if ".cls." in k) == sorted(HEAD)
    assert sorted(k for k in got["personal"] if ".cls." in k) == sorted(HEAD)
    # full depth: 30 adapter modules x 4 tensors communicated, with or without the head's keys
    from feddat_amd import albef_spec
    full = mode_names(list(albef_spec.param_shapes()), "dat")
    assert len(full["communicated"]) == 120 and sorted(k for k in full["personal"] if ".cls." in k) == sorted(HEAD)


def test_group_layout_and_weight_decay(names):
    """The head's flat group: the five `.cls.` tensors of the reference's trainable list, 622 650 floats at V = 30 522; the decayed
    ones are exactly those in create_optimizer's first group (transform.dense.weight); the vocabulary bias comes last and the
    buffers reach the padded vocabulary behind it."""
    for vocab in (3072, 30522):
        spec, pad = lm_head_group_spec(vocab)
        grp = FlatGroup(spec, "cpu", with_opt=True, pad=pad)
        assert sorted(grp.names) == sorted(n for n in names["trainable"] if ".cls." in n) == sorted(HEAD)
        assert grp.numel == 768 * 768 + 3 * 768 + vocab and (vocab != 30522 or grp.numel == 622650)
        decayed = [n for n, wd in zip(grp.names, grp.seg_wd.tolist()) if wd != 0.0]
        assert decayed == [n for n in names["decayed"] if ".cls." in n] == [LM_HEAD + "transform.dense.weight"]
        Vp = (vocab + 127) // 128 * 128
        ob = grp.offsets[LM_HEAD + "bias"]
        assert grp.names[-1] == LM_HEAD + "bias" and grp.names[0] == LM_HEAD + "transform.dense.weight" and grp.offsets[grp.names[0]] == 0
        assert ob % 4 == 0 and all(t.numel() >= ob + Vp and t.numel() % 4 == 0 for t in (grp.p, grp.g, grp.m, grp.v))
        assert grp.seg_off.tolist()[-1] == grp.numel and tuple(grp.view(LM_HEAD + "bias").shape) == (vocab,)
    assert FlatGroup(spec, "cpu", with_opt=True).p.numel() == (622650 + 3) // 4 * 4       # without the argument: as before


def test_train_main_refuses_the_option_for_vilt():
    from feddat_amd import train
    with pytest.raises(L.FeddatHipError, match="--albef_train_lm_head is an ALBEF option"):      # before any device is touched
        train.main(["--encoder_name", "vilt", "--albef_train_lm_head"])
    assert train.build_parser().parse_args([]).albef_train_lm_head is False


@pytest.mark.parametrize("f16", [False, True])
def test_lm_head_refresh_declared_exported_bound_and_checked(f16):
    """Every refusal happens in the argument checks: the pointers are never dereferenced and no kernel is launched."""
    from feddat_amd import build
    src = open(os.path.join(ROOT, "include", "feddat_hip.h")).read()
    lib = ctypes.CDLL(build.build(f16=f16))
    n = "feddat_lm_head_refresh"
    assert re.search(rf"^int {n}\(", src, flags=re.M)
    assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n)
    fn = getattr(lib, n)
    fn.argtypes, fn.restype = L._SIGS[n], ctypes.c_int
    assert lib.feddat_abi_version() == 8 == L.ABI_VERSION
    X = 0x1000          # 16-byte aligned, never dereferenced
    ok = dict(w=X, bias=X + 4, H=768, V=30522, Vp=30592, w16=X, wT16=X + 8, bpad=X)

    def call(**kw):
        a = dict(ok, **kw)
        return fn(a["w"], a["bias"], a["H"], a["V"], a["Vp"], a["w16"], a["wT16"], a["bpad"], None)
    for p in ("w", "bias", "w16", "wT16", "bpad"):
        assert call(**{p: None}) == EINVAL, p
    for bad in (dict(w=X + 4), dict(w=X + 8), dict(bpad=X + 4), dict(bias=X + 2), dict(w16=X + 4), dict(wT16=X + 2),      # alignment
                dict(H=0), dict(H=-768), dict(H=760), dict(H=8224), dict(V=0), dict(V=-1), dict(Vp=30521), dict(Vp=30594),
                dict(V=1 << 30, Vp=1 << 30)):
        assert call(**bad) == EINVAL, bad


def test_wrapper_needs_a_device():
    """CPU tensors are refused before the library is touched: there is no host path."""
    w, b = torch.zeros(768, 768), torch.zeros(3072)
    with pytest.raises(L.FeddatHipError):
        L.lm_head_refresh(w, b, torch.zeros(768, 768, dtype=torch.bfloat16), torch.zeros(768, 768, dtype=torch.bfloat16), torch.zeros(3072))
