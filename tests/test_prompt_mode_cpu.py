"""optimizer_mode 'prompt' without a GPU: the name sets against what the reference's own objects say (gp1, written by
tools/make_prompt_golden.py from prepare_model's statements and create_optimizer), the payload size, the row map of the prompted
frame, the C ABI of the two new kernels (declared in include/feddat_hip_prompt.h = exported = bound; argument checks) and what the engine refuses."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from feddat_amd import lib as L
from feddat_amd import vilt_spec
from feddat_amd.modes import MODES, averaged_names, mode_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("feddat_prompt_frame_assemble", "feddat_prompt_grad_gather")
EINVAL = 1
TASKS = ["art", "gqa"]


@pytest.fixture(scope="module")
def gp1(golden_dir):
    return np.load(os.path.join(golden_dir, "gp1_vilt2_prompt.npz"))


def test_name_sets_equal_the_references(gp1):
    from feddat_amd.modes import PROMPT_MODE
    assert PROMPT_MODE == "prompt" and MODES == ("dat", "adapter", "bias", "norm")
    keys = list(vilt_spec.param_shapes(2, TASKS, optimizer_mode="prompt"))
    got = mode_names(keys, "prompt")
    for k in ("trainable", "communicated", "personal"):
        assert got[k] == gp1["names." + k].tolist(), k
    assert len(got["communicated"]) == 10 and not any("clf" in k for k in got["communicated"])
    assert averaged_names(keys, "prompt") == got["communicated"]
    assert got["personal"] == [k for k in keys if k.startswith("task_layer.")]
    # vis first, the reference's state-dict order
    assert [k.split("prompt_embedding_")[1] for k in got["communicated"]] == \
        [f"{w}.{n}" for w in ("vis", "text") for n in ("0.weight", "1.weight", "1.bias", "3.weight", "3.bias")]


def test_payload_is_599424_floats_and_the_group_decays_the_weights(gp1):
    from feddat_amd.local_update import FlatGroup
    from feddat_amd.prompt_engine import prompt_names
    shapes = vilt_spec.param_shapes(2, TASKS, optimizer_mode="prompt")
    comm = mode_names(list(shapes), "prompt")["communicated"]
    assert sum(int(np.prod(shapes[k])) for k in comm) == 599424
    ns = prompt_names("vis") + prompt_names("text")
    assert [n for n, _ in ns] == comm and all(tuple(s) == tuple(shapes[n]) for n, s in ns)
    grp = FlatGroup(prompt_names("text"), "cpu", True)
    assert grp.numel == 299712 and grp.p.numel() == 299712      # no quad padding: vis | text lie back to back
    decayed = set(gp1["names.decayed"].tolist())
    assert [n for n, w in zip(grp.names, grp.seg_wd.tolist()) if w == 1.0] == [n for n in grp.names if n in decayed]
    assert [n.rsplit("prompt_embedding_text.", 1)[1] for n, w in zip(grp.names, grp.seg_wd.tolist()) if w == 1.0] == \
        ["0.weight", "1.weight", "3.weight"]


def test_random_init_and_pretrained_fill_know_the_prompt_tensors():
    P = vilt_spec.random_init(2, TASKS, seed=3, optimizer_mode="prompt")
    shapes = vilt_spec.param_shapes(2, TASKS, optimizer_mode="prompt")
    assert P.keys() == shapes.keys() and all(tuple(P[k].shape) == tuple(shapes[k]) for k in P)
    e = vilt_spec.ENC + "embeddings.prompt_embedding_"
    assert not torch.equal(P[e + "vis.1.weight"], P[e + "text.1.weight"])
    assert float(P[e + "text.1.weight"].abs().max()) <= 768 ** -0.5 and float(P[e + "text.3.bias"].abs().max()) <= 192 ** -0.5
    assert 2.0 < float(P[e + "text.0.weight"].abs().max()) < 6.0      # N(0, 1)
    Q = vilt_spec.random_init(2, TASKS, seed=3, optimizer_mode="prompt")
    assert all(torch.equal(P[k], Q[k]) for k in P)
    # the plain backbone under the prompt: bias mode's keys plus the ten
    assert [k for k in shapes if "prompt" not in k] == list(vilt_spec.param_shapes(2, TASKS, optimizer_mode="bias"))
    from feddat_amd.weights import init_trainable
    fresh = init_trainable({k: s for k, s in shapes.items() if "prompt" in k or k.startswith("task_layer.")}, seed=1)
    assert sorted(fresh) == sorted(k for k in shapes if "prompt" in k or k.startswith("task_layer."))


@pytest.mark.parametrize("Lt,Np", [(40, 49), (40, 144), (3, 1)])
def test_row_map_of_the_prompted_frame(Lt, Np):
    rows = L.prompt_row_map(Lt, Np)
    S = Lt + Np + 11
    assert len(rows) == S
    assert rows[0] == ("src", 0)                                                  # text token 0: what the pooler reads
    assert rows[1:6] == [("prompt", j, 0) for j in range(5)]                      # P[j] + type0
    assert rows[6:Lt + 5] == [("src", r) for r in range(1, Lt)]                   # text tokens 1 .. Lt - 1
    assert rows[Lt + 5] == ("src", Lt)                                            # image CLS
    assert rows[Lt + 6:Lt + 11] == [("prompt", j, 1) for j in range(5)]           # P[j] + type1
    assert rows[Lt + 11:] == [("src", r) for r in range(Lt + 1, Lt + 1 + Np)]     # patches
    assert sorted(r[1] for r in rows if r[0] == "src") == list(range(Lt + 1 + Np))
    with pytest.raises(L.FeddatHipError):
        L.prompt_row_map(0, Np)


def test_frame_shape_of_the_reference(gp1):
    assert gp1["frame.shape"].tolist() == [4, 100, 768] and len(L.prompt_row_map(40, 49)) == 100


@pytest.mark.parametrize("f16", [False, True])
def test_new_symbols_declared_exported_bound_and_checked(f16):
    from feddat_amd import build
    src = open(os.path.join(ROOT, "include", "feddat_hip_prompt.h")).read()
    lib = ctypes.CDLL(build.build(f16=f16))
    # the extension header's declarations = the binding's own table = what both libraries export
    assert sorted(re.findall(r"^(?:int|long) (feddat_[a-z0-9_]+)\(", src, flags=re.M)) == sorted(NEW_SYMBOLS) == \
        sorted(L.PROMPT_SYMBOLS)
    assert '#include "feddat_hip.h"' in src
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n not in L.EXPORTED_SYMBOLS, n
    assert lib.feddat_abi_version() == 8
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    asm = lib.feddat_prompt_frame_assemble
    asm.argtypes, asm.restype = L._PROMPT_SIGS["feddat_prompt_frame_assemble"], i32
    X, Y, M = 0x1000, 0x200000, 0x3000          # never dereferenced: every call below is refused by the argument checks
    ok = dict(h_in=X, km_in=M, P=X, m0=X, m1=X, h_out=Y, km_out=M, B=2, Lt=40, Np=49, H=768, nrep=1)

    def call(**kw):
        a = dict(ok, **kw)
        return asm(a["h_in"], a["km_in"], a["P"], a["m0"], a["m1"], a["h_out"], a["km_out"], a["B"], a["Lt"], a["Np"], a["H"],
                   a["nrep"], None)
    for bad in (dict(h_in=None), dict(P=None), dict(m0=None), dict(m1=None), dict(h_out=None), dict(B=0), dict(Lt=0), dict(Np=0),
                dict(H=770), dict(km_in=None), dict(nrep=0), dict(h_out=X), dict(h_in=X + 4), dict(P=X + 8)):
        assert call(**bad) == EINVAL, bad
    ga = lib.feddat_prompt_grad_gather
    ga.argtypes, ga.restype = L._PROMPT_SIGS["feddat_prompt_grad_gather"], i32
    with L.operands("f16" if f16 else "bf16"):      # the binding's loader types them too
        assert L.load().feddat_prompt_grad_gather.argtypes == L._PROMPT_SIGS["feddat_prompt_grad_gather"]
    assert [vp, i32, i32, i32, i32, f32, vp, vp, vp, vp] == L._PROMPT_SIGS["feddat_prompt_grad_gather"]
    assert ga(None, 2, 100, 40, 768, 1.0, None, Y, None, None) == EINVAL      # no gradient
    assert ga(X, 2, 100, 40, 768, 1.0, None, None, None, None) == EINVAL      # no output
    assert ga(X, 0, 100, 40, 768, 1.0, None, Y, None, None) == EINVAL
    assert ga(X, 2, 51, 40, 768, 1.0, None, Y, None, None) == EINVAL          # S too short for the image-side prompt rows
    assert ga(X, 2, 100, 40, 770, 1.0, None, Y, None, None) == EINVAL
    assert ga(X + 4, 2, 100, 40, 768, 1.0, None, Y, None, None) == EINVAL     # not 16-byte aligned


def test_prompt_ops_need_a_device():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(L.FeddatHipError):
        L.prompt_grad_gather(torch.zeros(2 * 100 * 768), 2, 100, 40, 768, torch.zeros(5, 768))
    with pytest.raises(L.FeddatHipError):
        L.prompt_frame_assemble(torch.zeros(2 * 90 * 768), None, torch.zeros(5, 768), torch.zeros(768), torch.zeros(768),
                                torch.zeros(2 * 100 * 768), None, 2, 40, 49, 768)


def test_engine_refuses_fp8_patch_slots_and_other_modes():
    from feddat_amd.prompt_engine import ViltPromptEngine
    with pytest.raises(L.FeddatHipError, match="16-bit operands only"):
        ViltPromptEngine({}, ["art"], "cpu", 2, 224, fp8=True)
    with pytest.raises(L.FeddatHipError, match="max_patches"):
        ViltPromptEngine({}, ["art"], "cpu", 2, 224, max_patches=40)
    for mode in ("bias", "lora", "dat"):
        with pytest.raises(L.FeddatHipError, match="runs optimizer_mode 'prompt'"):
            ViltPromptEngine({}, ["art"], "cpu", 2, 224, mode=mode)


def test_other_modes_are_still_unknown_and_main_keeps_its_four():
    keys = list(vilt_spec.param_shapes(2, TASKS, optimizer_mode="prompt"))
    for mode in ("lora", "full", "none"):
        with pytest.raises(L.FeddatHipError):
            mode_names(keys, mode)
    from feddat_amd import train
    with pytest.raises(L.FeddatHipError, match="dat, adapter, bias or norm"):
        train.main(["--optimizer_mode", "prompt"])


def test_prompt_engine_is_a_backbone_with_ten_extra_tokens():
    from feddat_amd.prompt_engine import ViltPromptEngine
    from feddat_amd.vilt_backbone import MAX_SEQ, ViltBackbone
    import inspect
    assert issubclass(ViltPromptEngine, ViltBackbone) and ViltPromptEngine.EXTRA_TOKENS == 10
    sig = inspect.signature(ViltBackbone.__init__)
    assert sig.parameters["extra_tokens"].default == 0
    assert 40 + 1 + 144 + 10 <= MAX_SEQ
