"""The third C ABI header, include/feddat_hip_albef.h, gets the checks tests/test_binding_cpu.py gives the other two: the parsed
signature against one spelled by hand, the bound argtypes / restype, and every `_ext("...")(...)` call site against the
declaration.  No GPU, no library call."""
import ast
import ctypes as C
import glob
import os
import re

import pytest

from feddat_amd import cheader as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_long, C.c_float


def test_signature_spelled_by_hand():
    from feddat_amd import lib as L
    assert list(H.ALBEF.functions) == ["feddat_lm_ce_loss_fwd_bwd"] and L.ALBEF_SYMBOLS == tuple(H.ALBEF.functions)
    restype, params = H.ALBEF.functions["feddat_lm_ce_loss_fwd_bwd"]
    assert restype is i32
    assert [t for t, _ in params] == [vp, i64, vp, vp, i32, i32, f32, vp, vp, vp, i64, vp, vp] == L._ALBEF_SIGS["feddat_lm_ce_loss_fwd_bwd"]
    assert [n for _, n in params] == ["logits", "ldl", "labels", "row_weight", "R", "V", "grad_scale", "grad_scale_dev", "nonfinite",
                                      "dlogits_bf16", "ldd", "scalars", "stream"]
    # an extension header: it includes the main one, adds no struct and no define, and shares no name with the other two
    src = open(H.ALBEF.path).read()
    assert '#include "feddat_hip.h"' in src and not H.ALBEF.structs and not H.ALBEF.defines
    assert not set(H.ALBEF.functions) & (set(H.MAIN.functions) | set(H.PROMPT.functions))
    assert sorted(re.findall(H.DECLARATION, src, flags=re.M)) == sorted(L.ALBEF_SYMBOLS)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_both_libraries_export_and_bind_it(fmt):
    from feddat_amd import lib as L
    with L.operands(fmt):
        bound = L.load()
        for name, (restype, params) in H.ALBEF.functions.items():
            fn = getattr(bound, name)
            assert fn.restype is restype and list(fn.argtypes) == [t for t, _ in params], name
            assert L._ext(name) is fn
        with pytest.raises(L.FeddatHipError):
            L._ext("feddat_axpby3")                 # a function of the main header is not served by name
        # refused by its argument checks (no pointer is dereferenced): FEDDAT_EINVAL
        assert L._ext("feddat_lm_ce_loss_fwd_bwd")(None, 8, None, None, 1, 5, 1.0, None, None, None, 8, None, None) == 1
        assert bound.feddat_abi_version() == 8


def test_every_ext_call_site_passes_the_declared_arguments():
    """Every `_ext("<name>")(...)` call in the package, tools/ and bench.py names a function of the header with a string literal
    and passes exactly its parameters, positionally; nothing calls the header's functions as attributes of the library."""
    declared = {n: len(p) for n, (_, p) in H.ALBEF.functions.items()}
    files = sorted(glob.glob(os.path.join(ROOT, "feddat_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")))
    sites, called, lookups, trees = 0, set(), [], []
    for path in files + [os.path.join(ROOT, "bench.py")]:
        trees.append(ast.parse(open(path).read(), path))          # (kept alive: the nodes' ids are compared below)
        for node in ast.walk(trees[-1]):
            where = f"{os.path.relpath(path, ROOT)}:{getattr(node, 'lineno', 0)}"
            if isinstance(node, ast.Attribute):
                assert node.attr not in declared, where
            if not isinstance(node, ast.Call):
                continue
            inner = node.func
            if isinstance(inner, ast.Call) and (getattr(inner.func, "id", None) == "_ext" or getattr(inner.func, "attr", None) == "_ext"):
                assert len(inner.args) == 1 and isinstance(inner.args[0], ast.Constant) and not inner.keywords, where
                name = inner.args[0].value
                assert name in declared, f"{where} {name}"
                assert not node.keywords and not any(isinstance(a, ast.Starred) for a in node.args), where
                assert len(node.args) == declared[name], f"{where} {name}"
                sites += 1
                called.add(id(inner))
            elif getattr(inner, "id", None) == "_ext" or getattr(inner, "attr", None) == "_ext":
                lookups.append((id(node), where))
    # an _ext(...) whose result is not called on the spot would escape the arity check
    assert all(i in called for i, _ in lookups), [w for i, w in lookups if i not in called]
    assert sites >= 1
