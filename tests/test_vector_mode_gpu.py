"""optimizer_mode 'bias' / 'norm' on the MI355X: vector_engine.ViltVectorEngine against the reference's fixtures tests/golden/gv*
(written by tools/make_vector_golden.py) and train.main in those modes.

Tolerances: pooled / logits 3e-2, losses 2e-3 relative (test_adapter_mode_gpu.py's for ga1: the same forward minus the
adapter); updates by ga1's rule (every element < 1e-3, mean error <= REL_MEAN of the mean update).

Gradients (gv1): the project has no gradient tolerance to take over, so the fixture carries one.  Next to the fp32 gradient
g of every trainable tensor it stores g16, the gradient of the same reference modules under torch.autocast("cpu", bfloat16);
e16 = max|g16 - g| / max|g| is what a 16-bit implementation of this step costs by the reference's own account.  The bf16 build
must stay within 2 x e16 per tensor (two 16-bit implementations that round at different sites and sum in different orders),
the f16 build within the same absolute bound.

key.bias: its gradient is exactly zero in exact arithmetic (softmax is shift-invariant), so both implementations hold
rounding noise there and element-wise parity is meaningless (tests print it).  It is covered by (a) the ratio
max|g key.bias| / max|g query.bias| of the same layer: ours must stay below KEY_RATIO_MULT x the same ratio of the reference's
bf16-autocast run, and (b) function parity of the trained model (gv2's held-out logits).  In gv1's update rule the key.bias
tensors keep the < 1e-3 bound and are excused, BY NAME, from the mean-error criterion only (Adam normalises the noise into
steps of up to lr in a direction that depends on summation order)."""
import lzma
import re

import numpy as np
import pytest
import torch

from oracle import feddat_oracle as O
from tests.golden_util import assert_update_parity, golden_tensor, load, sampled_update_parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL_MEAN = 0.1
MODES = ("bias", "norm")
# measured (gv1, 2 layers, B = 4, 224, both cases, per layer): max|g key.bias| / max|g query.bias| is 1.6e-7 .. 4.8e-7 in the
# fp32 reference, 1.5e-3 .. 2.4e-3 in its bf16-autocast run, 3.3e-3 .. 5.7e-3 in our bf16 step (1.6 .. 3.2 x the reference's
# 16-bit ratio of the same layer: autocast keeps softmax and LayerNorm in fp32, our step also rounds probabilities, dctx and
# dqkv to 16 bits) and 3.5e-4 .. 7.2e-4 in our f16 step (0.24 .. 0.30 x).  The multiple: a noise floor within 4 x the
# reference's own 16-bit one, three orders of magnitude below 1 (= a key.bias gradient as large as a real one)
KEY_RATIO_MULT = 4.0
GV1_VALID = [(224, 224), (160, 224), (224, 128), (96, 192)]
GV1_TEXT = [40, 31, 40, 12]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def plain_params(layers, tasks, bias_std=0.02):
    """The fixtures' weights: the name-seeded fill of the dat fixtures on the plain backbone's keys (no adapter; FFN2 under its
    HF key output.dense)."""
    out = {}
    for k, shp in O.param_shapes(O.ViltDims(layers=layers), tasks).items():
        if ".adapter." not in k:
            out[k.replace(".output.layer.dense.", ".output.dense.")] = O.seeded_value(k, shp, 0.02, bias_std)
    return out


def unpack_codes(g, prefix):
    codes = np.frombuffer(lzma.decompress(g[prefix + "lzma"].tobytes()), np.int8)
    step = float(g[prefix + "step"])
    out, o = {}, 0
    for k, n in zip(g[prefix + "names"].tolist(), g[prefix + "sizes"].tolist()):
        out[k] = torch.from_numpy(codes[o:o + n].astype(np.float32)) * step
        o += n
    assert o == codes.size
    return out, step


def _dev(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _engine(P, tasks, B, res, layers, mode, **kw):
    from feddat_amd.vector_engine import ViltVectorEngine
    return ViltVectorEngine(P, tasks, DEV, batch=B, res=res, layers=layers, mode=mode, **kw)


def _batches(case, n, seed0=2000):
    bs = [O.synthetic_batch(4, 224, seed0 + s) for s in range(n)]
    return [O.pad_batch(b, GV1_VALID, GV1_TEXT) for b in bs] if case == "padded" else bs


def _is_key_bias(k):
    return k.endswith("attention.attention.key.bias")


# ------------------------------------------------------------------------------------------------------- gv1: forward, gradients
@pytest.mark.parametrize("case", ["plain", "padded"])
@pytest.mark.parametrize("operands", ["bf16", "f16"])
@pytest.mark.parametrize("mode", MODES)
def test_gradient_of_every_trainable_tensor(golden_dir, mode, operands, case):
    g = load(golden_dir, f"gv1_vilt2_{mode}.npz")
    pre = f"{mode}.{case}."
    P = plain_params(2, ["art"])
    eng = _engine(P, ["art"], 4, 224, 2, mode, operands=operands, dynamic_loss_scale=False)
    batch = _batches(case, 1)[0]
    pooled, logits = eng.forward(_dev(batch), "art")
    dp = float((pooled.cpu() - torch.from_numpy(g[pre + "fwd.pooled"])).abs().max())
    dl = float((logits.cpu() - torch.from_numpy(g[pre + "fwd.logits"])).abs().max())
    eng.begin_local_update("art", steps_per_epoch=4)
    loss = float(eng.train_step(_dev(batch), use_graph=False)[0])
    ref_loss = float(g[pre + "loss"])
    print(f"gv1 {mode} {operands} {case}: |pooled| {dp:.2e} |logits| {dl:.2e} loss {loss:.5f} (ref {ref_loss:.5f})")
    assert dp < 3e-2 and dl < 3e-2
    assert abs(loss - ref_loss) < 2e-3 * abs(ref_loss) + 2e-3
    torch.cuda.synchronize()
    grads = {n: eng.vec.view(n, eng.vec.g).cpu() for n in eng.vec.names}
    hp = eng.head["art"]
    grads.update({n: hp.view(n, hp.g).cpu() for n in hp.names})
    names = [k[len(pre) + 3:] for k in g if k.startswith(pre + "g::") and "task_layer." not in k]
    assert sorted(names) == sorted(n for n in grads if not n.startswith("task_layer."))
    worst, fails = {}, []
    for n in names:
        ref, ref16, got = torch.from_numpy(g[pre + "g::" + n]), torch.from_numpy(g[pre + "g16::" + n]), grads[n]
        gmax = float(ref.abs().max())
        e16 = float((ref16 - ref).abs().max()) / gmax
        err = float((got - ref).abs().max()) / gmax
        kind = re.sub(r"layer\.\d+\.", "layer.*.", n)
        w = worst.setdefault(kind, [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], e16), max(w[1], err), max(w[2], err / e16)
        if _is_key_bias(n):
            q = n.replace("key.bias", "query.bias")
            r16 = float(ref16.abs().max()) / float(torch.from_numpy(g[pre + "g16::" + q]).abs().max())
            r32 = gmax / float(torch.from_numpy(g[pre + "g::" + q]).abs().max())
            ours = float(got.abs().max()) / float(grads[q].abs().max())
            print(f"   {n}: max|g key| / max|g query|  fp32 ref {r32:.2e}  bf16-autocast ref {r16:.2e}  ours {ours:.2e}")
            if not ours < KEY_RATIO_MULT * r16:
                fails.append((n, "key / query ratio", ours, "reference bf16", r16))
            continue
        if not err <= 2 * e16:
            fails.append((n, "err / max|g|", err, "e16", e16))
    # the head's gradients: whole tensors or put()'s strided samples, the same rule
    for n in hp.names:
        flat = grads[n].flatten()
        if pre + "g::" + n in g:
            ref, ref16 = torch.from_numpy(g[pre + "g::" + n]).flatten(), torch.from_numpy(g[pre + "g16::" + n]).flatten()
        else:
            idx = torch.linspace(0, flat.numel() - 1, 2048).long()
            flat, ref, ref16 = flat[idx], torch.from_numpy(g["samp::" + pre + "g::" + n]), torch.from_numpy(g["samp::" + pre + "g16::" + n])
        gmax = float(ref.abs().max())
        e16, err = float((ref16 - ref).abs().max()) / gmax, float((flat - ref).abs().max()) / gmax
        worst[n] = [e16, err, err / e16]
        if not err <= 2 * e16:
            fails.append((n, "err / max|g|", err, "e16", e16))
    for kind, (e16, err, ratio) in worst.items():
        print(f"   {kind}: e16 {e16:.3e}  ours {err:.3e}  bound {2 * e16:.3e}  worst ours / e16 {ratio:.2f}")
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------- gv1: four steps
@pytest.mark.parametrize("case", ["plain", "padded"])
@pytest.mark.parametrize("operands,use_graph", [("f16", False), ("f16", True), ("bf16", True)])
@pytest.mark.parametrize("mode", MODES)
def test_two_layer_engine_vs_reference(golden_dir, mode, operands, use_graph, case):
    g = load(golden_dir, f"gv1_vilt2_{mode}.npz")
    pre = f"{mode}.{case}."
    P = plain_params(2, ["art", "gqa"])
    P0 = {k: v.clone() for k, v in P.items()}
    eng = _engine(P, ["art", "gqa"], 4, 224, 2, mode, operands=operands)
    batches = _batches(case, 4)
    eng.begin_local_update("art", steps_per_epoch=4)
    if use_graph:
        eng.set_batch(_dev(O.synthetic_batch(4, 224, 1)))
        eng.ensure_captured()
    for s in range(4):
        out = eng.train_step(_dev(batches[s]), use_graph=use_graph)
        ref = float(g[pre + "losses"][s])
        assert abs(float(out[0]) - ref) < 2e-3 * abs(ref) + 2e-3, (s, float(out[0]), ref)
        assert eng.vec.state.tolist() == [s + 1, s + 1] == eng.head["art"].state.tolist()
        if s + 1 in (1, 4):
            sd = eng.state_dict()
            p = pre + f"after{s + 1}."
            vecs = [k[len(p) + 3:] for k in g if k.startswith(p + "d::")]
            assert sorted(vecs) == sorted(eng.vec.names)
            ref = {k: P0[k] + torch.from_numpy(g[p + "d::" + k]) for k in vecs}
            strict = [k for k in vecs if not _is_key_bias(k)]
            w = assert_update_parity(strict, sd, ref, P0, 1e-3, REL_MEAN, p)
            for k in vecs:
                if _is_key_bias(k):      # rounding noise normalised by Adam: the bound on every element stays, the mean rule does not apply
                    e = float((sd[k].cpu() - ref[k]).abs().max())
                    print(f"   {p}{k}: |dW - dW_ref| max {e:.2e}, reference moved {float((ref[k] - P0[k]).abs().max()):.2e}")
                    assert e < 1e-3, (k, e)
            whole = [k[len(p):] for k in g if k.startswith(p) and "::" not in k]
            w2 = assert_update_parity(whole, sd, {k: golden_tensor(g, p + k).reshape(P0[k].shape) for k in whole}, P0, 1e-3,
                                      REL_MEAN, p)
            w3 = sampled_update_parity(g, p, sd, P0, 2048, 1e-3, REL_MEAN)
            assert len(whole) >= 4
            print(f"gv1 {mode} {operands} graph {use_graph} {case} after {s + 1}: worst max {max(w[0], w2[0], w3[0]):.2e} "
                  f"worst mean ratio {max(w[1], w2[1], w3[1]):.3f}")
    assert eng.scaler_state()["skipped_substeps"] == 0
    sd = eng.state_dict()
    assert all(torch.equal(sd[k].cpu(), P0[k]) for k in sd if k.startswith("task_layer.gqa."))
    from feddat_amd.modes import mode_names
    assert sorted(sd) == sorted(mode_names(list(P0), mode)["trainable"])
    assert eng.comm_flat().numel() == {"bias": 2 * 8448 + 4 * 768, "norm": 2 * 4 * 768 + 2 * 768}[mode]
    # the kernels read the updated vectors in place: the frozen-weight entries are views into the group
    ln1b = "vilt_encoder.vilt.encoder.layer.0.layernorm_before.bias"
    assert eng.layers[0]["ln1b"].data_ptr() == eng.vec.view(ln1b).data_ptr() and torch.equal(eng.layers[0]["ln1b"], sd[ln1b])


def test_graph_replay_is_bit_identical_to_eager_and_to_itself():
    for mode in MODES:
        outs = []
        for use_graph in (False, True, True):
            eng = _engine(plain_params(2, ["art"]), ["art"], 4, 224, 2, mode)
            eng.begin_local_update("art", steps_per_epoch=3)
            for s in range(3):
                eng.train_step(_dev(O.synthetic_batch(4, 224, 700 + s)), use_graph=use_graph)
            torch.cuda.synchronize()
            outs.append({k: v.clone() for k, v in eng.state_dict().items()})
        for k in outs[0]:
            assert torch.equal(outs[0][k], outs[1][k]) and torch.equal(outs[1][k], outs[2][k]), (mode, k)


def test_fp8_is_refused():
    from feddat_amd import lib as L
    with pytest.raises(L.FeddatHipError):
        _engine(plain_params(2, ["art"]), ["art"], 2, 224, 2, "bias", fp8=True)


# ------------------------------------------------------------------------------------------------------- skipped step
@pytest.mark.parametrize("mode", MODES)
def test_injected_overflow_skips_the_step_and_halves_the_scale(mode):
    """GradScaler semantics, as ga3 checks for the adapter mode: a step whose overflow flag is set leaves parameters, Adam
    moments and the schedule untouched, halves the scale and clears the flag; the next step applies."""
    eng = _engine(plain_params(2, ["art"]), ["art"], 4, 224, 2, mode)
    s0 = eng.loss_scale
    eng.begin_local_update("art", steps_per_epoch=4)
    hp = eng.head["art"]
    eng.train_step(_dev(O.synthetic_batch(4, 224, 1500)), use_graph=True)
    eng.train_step(_dev(O.synthetic_batch(4, 224, 1501)), use_graph=True)
    torch.cuda.synchronize()
    keep = [t.clone() for grp in (eng.vec, hp) for t in (grp.p, grp.m, grp.v, grp.state)]
    eng.ovf_flags[0] = 1
    eng.train_step(_dev(O.synthetic_batch(4, 224, 1502)), use_graph=True)
    torch.cuda.synchronize()
    now = [t for grp in (eng.vec, hp) for t in (grp.p, grp.m, grp.v, grp.state)]
    assert all(torch.equal(a, b) for a, b in zip(keep, now))
    st = eng.scaler_state()
    assert st["scale"] == s0 / 2 and st["skipped_substeps"] == 1 and int(eng.ovf_flags[0]) == 0
    assert eng.vec.state.tolist() == [2, 2] == hp.state.tolist()
    eng.train_step(_dev(O.synthetic_batch(4, 224, 1503)), use_graph=True)
    torch.cuda.synchronize()
    assert eng.vec.state.tolist() == [3, 3] and not torch.equal(keep[0], eng.vec.p)
    # a non-finite partial sum raises the flag through the reduce kernel itself
    eng2 = _engine(plain_params(2, ["art"]), ["art"], 4, 224, 2, mode)
    eng2.begin_local_update("art", steps_per_epoch=4)
    eng2.train_step(_dev(O.synthetic_batch(4, 224, 1500)), use_graph=False)
    p_before = eng2.vec.p.clone()
    eng2.scaler_f.copy_(torch.tensor([2.0 ** 30, 2.0 ** -30]))      # a scale at which the 16-bit gradient operands overflow
    eng2.train_step(_dev(O.synthetic_batch(4, 224, 1501)), use_graph=False)
    torch.cuda.synchronize()
    assert torch.equal(p_before, eng2.vec.p) and eng2.scaler_state()["scale"] == 2.0 ** 29
    assert bool(torch.isfinite(eng2.vec.p).all())


# ------------------------------------------------------------------------------------------------------- 80-step round vs gv2
def _round80(golden_dir, mode, operands):
    g = load(golden_dir, f"gv2_round80_b32_{mode}.npz")
    P = plain_params(12, ["art"])
    P0 = {k: v.clone() for k, v in P.items()}
    eng = _engine(P, ["art"], 32, 384, 12, mode, operands=operands)
    eng.begin_local_update("art", steps_per_epoch=80)
    ref_moves = (float(g["max_abs_d_key_bias"]), float(g["max_abs_d_query_bias"]))
    worst, worst_key = {}, {}
    for s in range(80):
        eng.train_step(_dev(O.synthetic_batch(32, 384, 8000 + s)), use_graph=True)
        n = s + 1
        if n in (20, 40, 60, 80):
            ref, step = unpack_codes(g, f"s{n}::dq::")
            sd = eng.state_dict()
            assert sorted(ref) == sorted(k for k in sd)
            w = wk = 0.0
            for k in ref:
                e = float(((sd[k].detach().cpu() - P0[k]).flatten() - ref[k]).abs().max())
                if _is_key_bias(k):
                    wk = max(wk, e)
                w = max(w, e)
            worst[n], worst_key[n] = w, wk
    held = O.synthetic_batch(32, 384, int(g["heldout.seed"]))
    pooled, logits = eng.forward(_dev(held), "art")
    dl = float((logits.cpu() - torch.from_numpy(g["heldout.logits"])).abs().max())
    dp = float((pooled.cpu() - torch.from_numpy(g["heldout.pooled"])).abs().max())
    print(f"gv2 {mode} {operands}: worst |dW - dW_ref| over EVERY element (key.bias included) per snapshot {worst}; key.bias alone "
          f"{worst_key}; reference to within {step / 2}; fp32 reference moved key.bias by {ref_moves[0]:.2e}, query.bias by "
          f"{ref_moves[1]:.2e}; held-out |logits| {dl:.2e} |pooled| {dp:.2e}; scaler {eng.scaler_state()}")
    return worst, step, dl, dp


@pytest.mark.parametrize("mode", MODES)
def test_round80_b32_every_element_under_1e3(golden_dir, mode):
    """12 layers, B = 32, 384 x 384, 80 steps (ga2's protocol and batches), default (f16) engine through the hipGraph: every
    element of every trainable tensor's update within 1e-3 of the reference at 20 / 40 / 60 / 80 steps (held to 1e-3 - q, q the
    fixture's quantisation half-step), and the trained model's logits on a held-out batch at ga1's logit tolerance.  The fp32
    reference moves key.bias by at most 1.2e-5 in the round (query.bias: 2.5e-3): it stays put there, so the key.bias elements
    stay in this test."""
    worst, step, dl, dp = _round80(golden_dir, mode, "f16")
    assert all(v < 1e-3 - step / 2 for v in worst.values()), worst
    assert dl < 3e-2 and dp < 3e-2


@pytest.mark.parametrize("mode", MODES)
def test_round80_b32_bf16_operands_reported(golden_dir, mode):
    """The bf16 build on the same round: printed, and held to function parity only (test_round_b32_gpu.py's treatment of
    the bf16 operands)."""
    worst, step, dl, dp = _round80(golden_dir, mode, "bf16")
    assert dl < 3e-2 and dp < 3e-2


# ------------------------------------------------------------------------------------------------------- train.main vs gv3
def _gv3_args(mode):
    return ["--optimizer_mode", mode, "--ordered_cl_tasks", "art,abstract", "--num_layers", "2", "--image_size", "224",
            "--batch_size", "4", "--synthetic_steps", "3,2", "--seed", "42"]


@pytest.mark.parametrize("mode", MODES)
def test_main_vs_reference_federation(golden_dir, tmp_path, mode):
    from feddat_amd import train, vilt_spec
    from feddat_amd.modes import averaged_names
    g = load(golden_dir, "gv3_round_2clients_vector.npz")
    P0 = vilt_spec.random_init(2, ["art", "abstract"], seed=42, optimizer_mode=mode)
    a = train.main(_gv3_args(mode) + ["--comm_rounds", "2", "--save_every", "1", "--output_dir", str(tmp_path / "a")])
    sd = a.state_dict()
    assert a.comm_state_dict_names == g[f"{mode}.names.communicated"].tolist()
    avg = averaged_names(list(sd), mode)
    ref = {k: P0[k] + torch.from_numpy(g[f"{mode}.r1.server.d::" + k]) for k in avg}
    strict = [k for k in avg if not _is_key_bias(k)]
    w = assert_update_parity(strict, sd, ref, P0, 1e-3, REL_MEAN, f"gv3 {mode} server")
    for k in avg:
        if _is_key_bias(k):
            assert float((sd[k].cpu() - ref[k]).abs().max()) < 1e-3, k
    # the heads' own communicated keys never move on the reference's server (get_average_net skips 'clf')
    for k in a.comm_state_dict_names:
        if k not in avg:
            assert float(np.abs(g[f"{mode}.r1.server.d::" + k]).max()) == 0.0, k
    from safetensors.torch import load_file
    for t in ("art", "abstract"):
        pa = load_file(str(tmp_path / "a" / f"personal_{t}.safetensors"))
        assert all(k.startswith("task_layer.") for k in pa)
        names = [k for k in pa if k.startswith(f"task_layer.{t}.")]
        whole = [k for k in names if f"{mode}.r1.{t}." + k in g]
        assert_update_parity(whole, pa, {k: golden_tensor(g, f"{mode}.r1.{t}." + k).reshape(P0[k].shape) for k in whole}, P0,
                             1e-3, REL_MEAN, f"gv3 {mode} {t}")
        sampled_update_parity(g, f"{mode}.r1.{t}.", pa, P0, 2048, 1e-3, REL_MEAN)
    print(f"gv3 {mode}: server worst max {w[0]:.2e} worst mean ratio {w[1]:.3f}")


# ------------------------------------------------------------------------------------------------------- two ranks
@pytest.mark.parametrize("mode", MODES)
def test_two_ranks_through_train_main_match_single_process(tmp_path, mode):
    """test_multirank_gpu.py's protocol: two ranks share cuda:0 and exchange the vector group over gloo; the averaged tensors
    (two addends per element) and every client's personal tensors equal the single-process run bit for bit."""
    import os
    import socket
    import subprocess
    import sys
    from safetensors.torch import load_file
    from feddat_amd import train, vilt_spec
    from feddat_amd.modes import averaged_names
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--optimizer_mode", mode, "--num_layers", "2", "--image_size", "224", "--batch_size", "2", "--synthetic_steps",
              "3,2", "--comm_rounds", "2", "--save_every", "1", "--synthetic_label_alpha", "0.5", "--ordered_cl_tasks", "art,gqa"]
    single = train.main(common + ["--output_dir", str(tmp_path / "single")])
    sd1 = {k: v.cpu().clone() for k, v in single.state_dict().items()}
    env = dict(os.environ)
    env.update(FEDDAT_FORCE_DEVICE="0", FEDDAT_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=root)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = tmp_path / "two"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", "feddat_amd.train"] + common + ["--output_dir", str(out)]
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    srv = load_file(str(out / "server_adapter.safetensors"))
    avg = averaged_names(list(sd1), mode)
    assert sorted(srv) == sorted(single.comm_state_dict_names) and len(avg) == {"bias": 20, "norm": 10}[mode]
    P0 = vilt_spec.random_init(2, ["art", "gqa"], seed=42, optimizer_mode=mode)      # (train.main's default seed)
    for k in avg:
        assert torch.equal(srv[k], sd1[k]), (k, float((srv[k] - sd1[k]).abs().max()))
    assert max(float((srv[k] - P0[k]).abs().max()) for k in avg) > 0
    for t in ("art", "gqa"):
        a = load_file(str(tmp_path / "single" / f"personal_{t}.safetensors"))
        b = load_file(str(out / f"personal_{t}.safetensors"))
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a), t
