"""The ctypes binding is derived from the C headers (feddat_amd/cheader.py): the reader against signatures spelled by hand,
the struct layouts against the host compiler, every call site's arity against the declarations, lib.py's numeric constants
against the #defines.  No GPU, no library call."""
import ast
import ctypes as C
import glob
import os
import subprocess

from feddat_amd import cheader as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i32, i64, f32, u32 = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_uint
STRUCTS = {"AdapterSeg": "feddat_adapter_seg", "WgradSeg": "feddat_wgrad_seg", "ViltLayerWeights": "feddat_vilt_layer_weights",
           "ViltLayerActs": "feddat_vilt_layer_acts", "ViltLayerGrads": "feddat_vilt_layer_grads", "VgradJob": "feddat_vgrad_job",
           "HtJob": "feddat_ht_job", "AdamwGroup": "feddat_adamw_group", "GemmRoute": "feddat_gemm_route_t",
           "HtPlan": "feddat_ht_plan"}


def test_signatures_spelled_by_hand():
    from feddat_amd import lib as L
    P = C.POINTER
    want = {
        # long strides, float, unsigned
        "feddat_attn2_fwd_dropout": [vp, i64, vp, i64, vp, i64, vp, i32, vp, i64, vp, i32, i32, i32, i64, i64, i32, f32, u32, u32,
                                     vp, vp],
        # four struct pointers (and the opaque feddat_ctx*, uint8_t*)
        "feddat_vilt_layer_bwd": [vp, P(L.ViltLayerWeights), P(L.ViltLayerActs), P(L.ViltLayerGrads), i32, i32, i32, vp,
                                  P(L.AdapterSeg), i32, P(L.WgradSeg), i32, vp, i64, i32, vp],
        # jobs_dev: a struct pointer that is a device address
        "feddat_vector_grad_reduce": [vp, i32, i32, f32, vp, vp, vp],
        # float* const*
        "feddat_adapter_wgrad_reduce": [vp, i32, i32, vp, i64, vp],
        # feddat_ctx**
        "feddat_ctx_create": [i32, vp],
        # void** out-parameter
        "feddat_comm_create_timeout": [vp, i32, i32, i32, vp],
        # const char*, const long*
        "feddat_wordpiece_table_build": [vp, vp, i32, vp, i64],
        "feddat_layernorm_bwd_dx_fp8": [vp, vp, i64, vp, i64, vp, vp, vp, i64, i32, i32, vp, i64, vp, vp, vp, vp],
        "feddat_head_gemm_plan": [P(L.HtJob), P(L.HtPlan)],
        "feddat_abi_version": [],
    }
    for name, sig in want.items():
        assert L._SIGS[name] == sig, name
        assert [t for t, _ in H.MAIN.functions[name][1]] == sig, name
    assert L._PROMPT_SIGS["feddat_prompt_grad_gather"] == [vp, i32, i32, i32, i32, f32, vp, vp, vp, vp]
    assert [n for _, n in H.PROMPT.functions["feddat_prompt_grad_gather"][1]] == \
        ["dh0", "B", "S", "Lt", "H", "unscale", "unscale_dev", "G", "nonfinite", "stream"]
    # the aliases are the objects the derived lists hold
    assert (L.vp, L.i32, L.i64, L.f32, L.u32) == (vp, i32, i64, f32, u32)
    assert all(t in (vp, i32, i64, f32, u32) or issubclass(t._type_, C.Structure)
               for sigs in (L._SIGS, L._PROMPT_SIGS) for sig in sigs.values() for t in sig)
    assert H.MAIN.functions["feddat_gemm_skinny_workspace_elems"][0] is i64
    assert H.MAIN.functions["feddat_gemm_route"][0] is i32 and H.PROMPT.functions["feddat_prompt_grad_gather"][0] is i32
    assert len(H.MAIN.functions) == 115 == len(L.EXPORTED_SYMBOLS) and L.EXPORTED_SYMBOLS == tuple(H.MAIN.functions)
    assert len(H.PROMPT.functions) == 2 and L.PROMPT_SYMBOLS == tuple(H.PROMPT.functions)
    assert sorted(H.MAIN.structs) == sorted(STRUCTS.values()) and not H.PROMPT.structs
    for py, c in STRUCTS.items():
        assert getattr(L, py) is H.MAIN.types[c] and getattr(L, py)._fields_ == H.MAIN.structs[c], py
    # fixed arrays and pointer fields, by hand
    assert H.MAIN.structs["feddat_adapter_seg"][5:8] == [("reserved", i32), ("scale", f32 * 2), ("wd", vp * 2)]
    assert H.MAIN.structs["feddat_adamw_group"][4:6] == [("n", i64), ("seg_off", vp)]
    assert dict(H.MAIN.structs["feddat_adamw_group"])["skip_if"] is vp * 2
    # the loader gives every function the header's return type
    bound = L.load()
    for hdr in (H.MAIN, H.PROMPT):
        for name, (restype, params) in hdr.functions.items():
            fn = getattr(bound, name)
            assert fn.restype is restype and list(fn.argtypes) == [t for t, _ in params], name


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof and every offsetof, from the host compiler on the header itself (it needs no HIP: it typedefs hipStream_t)."""
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "feddat_hip.h"', "int main() {"]
    for name, fields in H.MAIN.structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in fields]
    lines.append("}")
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["g++", "-I", H.INCLUDE, str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    want = {}
    for name, cls in H.MAIN.types.items():
        want[name] = str(C.sizeof(cls))
        want.update({f"{name}.{f}": str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert len(H.MAIN.types) == 10 and got == want


def test_every_call_site_passes_the_declared_arguments():
    """ctypes refuses too few arguments at run time and never too many: every `<x>.feddat_*(...)` call in the package, tools/ and
    bench.py names a declared function and passes exactly its parameters, positionally."""
    declared = {n: len(p) for hdr in (H.MAIN, H.PROMPT) for n, (_, p) in hdr.functions.items()}
    files = sorted(glob.glob(os.path.join(ROOT, "feddat_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")))
    sites = 0
    for path in files + [os.path.join(ROOT, "bench.py")]:
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("feddat_"):
                where = f"{os.path.relpath(path, ROOT)}:{node.lineno} {node.func.attr}"
                assert node.func.attr in declared, where
                assert not node.keywords and not any(isinstance(a, ast.Starred) for a in node.args), where
                assert len(node.args) == declared[node.func.attr], where
                sites += 1
    assert sites >= 117


def test_constants_equal_the_defines():
    from feddat_amd import lib as L
    defines = {**H.MAIN.defines, **H.PROMPT.defines}
    checked = set()
    for name, value in defines.items():
        if hasattr(L, name):
            mine = getattr(L, name)
            assert type(mine) is type(value) and float(mine) == float(value), name
            checked.add(name)
    named = [n for n in defines if n.startswith(("EPI_", "GEMM_", "HT_", "FILTER_", "F8_", "G8_", "OPERANDS_"))]
    assert len(named) == 9 + 8 + 6 + 2 + 2 + 2 + 2
    assert checked >= set(named) | {"VGRAD_UNSCALED", "ABI_VERSION"}
    assert L.ABI_VERSION == defines["ABI_VERSION"] == 8
    assert defines["G8_LO"] == -0.135 and defines["F8_ACT_SCALE"] == 0.125 and defines["ADAMW_MAX_GROUPS"] == 4
