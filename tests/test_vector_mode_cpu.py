"""optimizer_mode 'bias' / 'norm' without a GPU: the name sets against what the reference's own objects say (gv3, written by
tools/make_vector_golden.py from prepare_model's statements, create_optimizer and the personal-parameter shuttle), the C ABI
of the vector-gradient kernels (declared = exported = bound; argument checks), and what train.main accepts."""
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
NEW_SYMBOLS = ("feddat_vector_grad_workspace_elems", "feddat_colsum_partial", "feddat_ln_param_grad_partial",
               "feddat_vector_grad_reduce")
EINVAL = 1


@pytest.fixture(scope="module")
def gv3(golden_dir):
    return np.load(os.path.join(golden_dir, "gv3_round_2clients_vector.npz"))


@pytest.mark.parametrize("mode", ["bias", "norm"])
@pytest.mark.parametrize("tag,layers", [("names", 2), ("names12", 12)])
def test_name_sets_equal_the_references(gv3, mode, tag, layers):
    keys = list(vilt_spec.param_shapes(layers, ["art", "abstract"], optimizer_mode=mode))
    got = mode_names(keys, mode)
    for k in ("trainable", "communicated", "personal"):
        assert got[k] == gv3[f"{mode}.{tag}.{k}"].tolist(), k
    # case-sensitive substring: the text LayerNorm (capital N) is no 'norm' parameter, the head's clf_norm0 is one
    ln = vilt_spec.ENC + "embeddings.text_embeddings.LayerNorm."
    assert (ln + "bias" in got["trainable"]) == (mode == "bias") and ln + "weight" not in got["trainable"]
    # the head's own matches are communicated AND personal; get_average_net skips them ('clf'), so nothing of a head is averaged
    both = sorted(set(got["communicated"]) & set(got["personal"]))
    want = {"bias": ("clf_fc0.bias", "clf_norm0.bias", "clf_fc1.bias"), "norm": ("clf_norm0.weight", "clf_norm0.bias")}[mode]
    assert both == sorted(f"task_layer.{t}.{n}" for t in ("art", "abstract") for n in want)
    avg = averaged_names(keys, mode)
    assert avg == [k for k in got["communicated"] if k not in both] and not any("task_layer" in k for k in avg)
    n_backbone = sum(int(np.prod(vilt_spec.param_shapes(layers, (), optimizer_mode=mode)[k])) for k in avg)
    if layers == 12:
        assert n_backbone == {"bias": 104448, "norm": 38400}[mode]


@pytest.mark.parametrize("mode", ["bias", "norm"])
def test_group_layout_and_weight_decay(gv3, mode):
    """The engine's flat group holds exactly the reference's trainable backbone tensors, q | k | v adjacent, and decays what
    create_optimizer's first parameter group holds: the gammas of norm mode (layernorm_*.weight is no 'LayerNorm.weight'), no
    bias."""
    from feddat_amd.local_update import FlatGroup
    from feddat_amd.vector_engine import vector_names
    ns = vector_names(mode, 12)
    ref_train = [k for k in gv3[f"{mode}.names12.trainable"].tolist() if not k.startswith("task_layer.")]
    assert [n for n, _ in ns] == ref_train
    shapes = vilt_spec.param_shapes(12, (), optimizer_mode=mode)
    assert all(tuple(s) == tuple(shapes[n]) for n, s in ns)
    grp = FlatGroup(ns, "cpu", True)
    decayed = set(gv3[f"{mode}.names12.decayed"].tolist())
    assert [n for n, w in zip(grp.names, grp.seg_wd.tolist()) if w == 1.0] == [n for n in grp.names if n in decayed]
    assert (sum(grp.seg_wd.tolist()) > 0) == (mode == "norm")
    if mode == "bias":
        for i in range(12):
            q = vilt_spec.ENC + f"encoder.layer.{i}.attention.attention.query.bias"
            assert grp.offsets[q.replace("query", "key")] == grp.offsets[q] + 768
            assert grp.offsets[q.replace("query", "value")] == grp.offsets[q] + 1536


def test_plain_backbone_keys_and_init():
    """bias / norm add no parameters and no Adaptered_ViltOutput: the FFN's second product keeps its HF key."""
    a, d = vilt_spec.param_shapes(2, ("art",), optimizer_mode="bias"), vilt_spec.param_shapes(2, ("art",))
    assert a == vilt_spec.param_shapes(2, ("art",), optimizer_mode="norm")
    assert not any("adapter" in k for k in a)
    assert sorted(re.sub(r"(layer\.\d+\.output\.)dense", r"\1layer.dense", k) for k in a) == sorted(k for k in d if "adapter" not in k)
    P = vilt_spec.random_init(2, ("art",), seed=3, optimizer_mode="bias")
    assert P.keys() == a.keys() and float(P[vilt_spec.ENC + "encoder.layer.1.output.dense.bias"].abs().max()) > 0
    assert MODES == ("dat", "adapter", "bias", "norm")


@pytest.mark.parametrize("f16", [False, True])
def test_new_symbols_declared_exported_bound_and_checked(f16):
    from feddat_amd import build
    src = open(os.path.join(ROOT, "include", "feddat_hip.h")).read()
    lib = ctypes.CDLL(build.build(f16=f16))
    for n in NEW_SYMBOLS:
        assert re.search(rf"^(?:int|long) {n}\(", src, flags=re.M), n
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n), n
    assert lib.feddat_abi_version() == 8
    assert ctypes.sizeof(L.VgradJob) == 32 and "int reserved;" in src
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    ws = lib.feddat_vector_grad_workspace_elems
    ws.argtypes, ws.restype = [i32, i32], i64
    assert ws(5920, 768) == 93 * 768 and ws(64, 8) == 8 and ws(65, 8) == 16 and ws(0, 768) == 0
    cs = lib.feddat_colsum_partial
    cs.argtypes, cs.restype = [vp, vp, i64, vp, i32, i32, vp, i64, vp], i32
    X, Pp = 0x1000, 0x2000          # never dereferenced: every call below is refused by the argument checks
    assert cs(None, None, 768, None, 64, 768, Pp, 768, None) == EINVAL           # no input
    assert cs(X, X, 768, None, 64, 768, Pp, 768, None) == EINVAL                 # both inputs
    assert cs(X, None, 772, None, 64, 772, Pp, 772, None) == EINVAL              # N % 8 != 0
    assert cs(X, None, 760, None, 64, 768, Pp, 768, None) == EINVAL              # row stride < N
    assert cs(X, None, 768, None, 65, 768, Pp, 768, None) == EINVAL              # partial buffer one slab short
    assert cs(X, None, 768, None, 64, 768, None, 768, None) == EINVAL            # no output
    ln = lib.feddat_ln_param_grad_partial
    ln.argtypes, ln.restype = [vp, vp, i64, vp, i64, vp, i32, i32, vp, vp, i64, vp], i32
    assert ln(None, None, 768, X, 768, X, 64, 768, Pp, Pp, 768, None) == EINVAL  # NULL dy
    assert ln(X, None, 768, None, 768, X, 64, 768, Pp, Pp, 768, None) == EINVAL  # dgamma asked for without x
    assert ln(X, None, 768, X, 768, X, 64, 768, Pp, None, 768, None) == EINVAL   # no dbeta output
    assert ln(X, None, 768, X, 768, X, 129, 768, Pp, Pp, 2 * 768, None) == EINVAL
    rd = lib.feddat_vector_grad_reduce
    rd.argtypes, rd.restype = [vp, i32, i32, f32, vp, vp, vp], i32
    assert rd(None, 1, 768, 1.0, None, None, None) == EINVAL and rd(X, 0, 768, 1.0, None, None, None) == EINVAL
    assert rd(X, 1, 0, 1.0, None, None, None) == EINVAL


def test_vector_ops_need_a_device():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(L.FeddatHipError):
        L.colsum_partial(torch.zeros(64, 768), torch.zeros(768))


def test_main_accepts_the_four_modes_and_refuses_the_rest():
    from feddat_amd import train
    for mode in ("bias", "norm"):
        with pytest.raises(L.FeddatHipError, match="ALBEF supports only"):
            train.main(["--encoder_name", "albef_no_distill", "--optimizer_mode", mode])
    for mode in ("lora", "prompt", "full", "none", "freeze_encoder"):
        with pytest.raises(L.FeddatHipError, match="dat, adapter, bias or norm"):
            train.main(["--optimizer_mode", mode])


def test_engine_refuses_fp8_and_unknown_modes():
    from feddat_amd.vector_engine import ViltVectorEngine
    with pytest.raises(L.FeddatHipError, match="16-bit operands only"):
        ViltVectorEngine({}, ["art"], "cpu", 2, 224, mode="bias", fp8=True)
    with pytest.raises(L.FeddatHipError):
        ViltVectorEngine({}, ["art"], "cpu", 2, 224, mode="lora")


def test_vector_engine_is_a_backbone_and_not_a_dat_engine():
    from feddat_amd.engine import ViltDatEngine
    from feddat_amd.vector_engine import ViltVectorEngine
    from feddat_amd.vilt_backbone import ViltBackbone
    assert issubclass(ViltVectorEngine, ViltBackbone) and issubclass(ViltDatEngine, ViltBackbone)
    assert not issubclass(ViltVectorEngine, ViltDatEngine)
