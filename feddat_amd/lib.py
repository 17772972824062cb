"""ctypes binding of libfeddat_hip.so (include/feddat_hip.h and its extension headers include/feddat_hip_prompt.h and
include/feddat_hip_albef.h).

The HIP library is THE product path: if it cannot be loaded this module raises -- there is no eager /
PyTorch / CPU fallback anywhere in feddat_amd.  torch is used only as plumbing: device allocations
(tensor.data_ptr()), the current HIP stream, and torch.distributed for the one RCCL all-reduce per round.

The headers are the one statement of the C ABI: every entry point's argument and return types and the fields of the ten
structs are read from them at import (feddat_amd/cheader.py), nothing of that is restated here.  A new entry point is declared
in its header and gets its wrapper below.  The numeric constants are literals here (tests/test_binding_cpu.py holds them to
the headers' #defines).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import threading
from typing import Optional, Sequence

import torch  # imported first on purpose: libfeddat_hip.so must bind to the HIP runtime torch already loaded

from . import cheader as _H

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libfeddat_hip.so")
# the same sources and C ABI with IEEE-half operands (include/feddat_hip.h, Conventions): bound by operands("f16")
LIB_PATH_F16 = os.path.join(_PKG, "libfeddat_hip_f16.so")
OPERANDS_BF16, OPERANDS_FP16 = 0, 1      # feddat_operand_format()
OPERAND_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}

EPI_BF16, EPI_RESID_F32, EPI_GELU, EPI_MUL_DGELU, EPI_F32, EPI_GELU_G8, EPI_MUL_G8, EPI_GELU_G8_F8, EPI_MUL_G8_F8 = range(9)
F8_ACT_SCALE, F8_GRAD_HEADROOM = 0.125, 4.0      # FEDDAT_F8_ACT_SCALE / FEDDAT_F8_GRAD_HEADROOM
G8_LO, G8_STEP = -0.135, 0.005        # FEDDAT_G8_LO / FEDDAT_G8_STEP: gelu' ~ G8_LO + G8_STEP * code
GEMM_OP16, GEMM_FP8, GEMM_FP8MX = range(3)                               # feddat_gemm_route: operand kind
GEMM_V1, GEMM_MID, GEMM_V2, GEMM_V3, GEMM_DUAL = range(5)                # ... and kernel family (FEDDAT_GEMM_*)
FILTER_BILINEAR, FILTER_BICUBIC = 2, 3      # FEDDAT_FILTER_*: Pillow's Image.BILINEAR / Image.BICUBIC

ABI_VERSION = 8
vp, i32, i64, f32, u32 = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_uint

# the structs of include/feddat_hip.h: their _fields_ are the header's, read by cheader
AdapterSeg = _H.MAIN.types["feddat_adapter_seg"]
WgradSeg = _H.MAIN.types["feddat_wgrad_seg"]
ViltLayerWeights = _H.MAIN.types["feddat_vilt_layer_weights"]
ViltLayerActs = _H.MAIN.types["feddat_vilt_layer_acts"]
ViltLayerGrads = _H.MAIN.types["feddat_vilt_layer_grads"]
VgradJob = _H.MAIN.types["feddat_vgrad_job"]
HtJob = _H.MAIN.types["feddat_ht_job"]
AdamwGroup = _H.MAIN.types["feddat_adamw_group"]
GemmRoute = _H.MAIN.types["feddat_gemm_route_t"]
HtPlan = _H.MAIN.types["feddat_ht_plan"]

VGRAD_UNSCALED = 1
HT_PRO_NONE, HT_PRO_LN, HT_PRO_TANH_BWD = 0, 1, 2
HT_EPI_NONE, HT_EPI_TANH, HT_EPI_MUL_DGELU = 0, 1, 2


def _fill(struct, **tensors):
    """ctypes struct of device pointers from tensors (None -> NULL); keeps the tensors alive on the struct."""
    s = struct()
    s._keep = tensors
    for k, t in tensors.items():
        setattr(s, k, (t.data_ptr() if isinstance(t, torch.Tensor) else t) if t is not None else None)
    return s


# every entry point's argument types as its header declares them (cheader's type rules), in declaration order
_SIGS = {name: [t for t, _ in params] for name, (_, params) in _H.MAIN.functions.items()}
EXPORTED_SYMBOLS = tuple(_SIGS)
# the extension header include/feddat_hip_prompt.h (csrc/prompt.hip): the same libraries
_PROMPT_SIGS = {name: [t for t, _ in params] for name, (_, params) in _H.PROMPT.functions.items()}
PROMPT_SYMBOLS = tuple(_PROMPT_SIGS)
# the extension header include/feddat_hip_albef.h (csrc/albef_misc.hip): the same libraries.  Its functions are called by name
# through _ext (below), not as attributes of the loaded library
_ALBEF_SIGS = {name: [t for t, _ in params] for name, (_, params) in _H.ALBEF.functions.items()}
ALBEF_SYMBOLS = tuple(_ALBEF_SIGS)


class FeddatHipError(RuntimeError):
    pass


_lib = None            # the bf16-operand library (the default binding)
_lib_f16 = None        # the fp16-operand library
_tls = threading.local()


def _open(path: str, want_format: int) -> C.CDLL:
    if not os.path.exists(path):
        raise FeddatHipError(
            f"{path} not found: the HIP library is the only implementation of this path "
            "(no CPU/PyTorch fallback). Build it with `python __graft_entry__.py` or `python -m feddat_amd.build`.")
    lib = C.CDLL(path)
    for header, sigs in ((_H.MAIN, _SIGS), (_H.PROMPT, _PROMPT_SIGS), (_H.ALBEF, _ALBEF_SIGS)):
        for name, args in sigs.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, header.functions[name][0]
    if lib.feddat_abi_version() != ABI_VERSION:
        raise FeddatHipError(f"{os.path.basename(path)} ABI version mismatch")
    if lib.feddat_operand_format() != want_format:
        raise FeddatHipError(f"{os.path.basename(path)} was built for another operand format")
    return lib


def load() -> C.CDLL:
    """The library the calling thread is bound to: libfeddat_hip.so (bf16 operands) unless inside `with operands("f16")`.
    Raises loudly if it is missing (build with `python -m feddat_amd.build`)."""
    global _lib, _lib_f16
    if getattr(_tls, "fmt", "bf16") == "f16":
        if _lib_f16 is None:
            _lib_f16 = _open(LIB_PATH_F16, OPERANDS_FP16)
        return _lib_f16
    if _lib is None:
        _lib = _open(LIB_PATH, OPERANDS_BF16)
    return _lib


@contextlib.contextmanager
def operands(fmt: str):
    """Bind this thread's calls to the library built for the 16-bit operand format `fmt` ("bf16" | "f16") for the duration of
    the block.  Both libraries export the same C ABI; buffers the header calls "bf16" hold OPERAND_DTYPE[fmt] values.  An
    engine makes all its calls (and creates its feddat_ctx) inside the block of ITS format, so engines of both formats can
    live in one process."""
    if fmt not in OPERAND_DTYPE:
        raise FeddatHipError(f"unknown operand format {fmt!r} (bf16 | f16)")
    prev = getattr(_tls, "fmt", "bf16")
    _tls.fmt = fmt
    try:
        yield
    finally:
        _tls.fmt = prev


def current_operands() -> str:
    return getattr(_tls, "fmt", "bf16")


def use_ablation_build():
    """tools/ only, and only before the first load(): bind libfeddat_hip_ablate.so (`python -m feddat_amd.build --ablate`), the
    -DFEDDAT_ABLATE build that contains the timing-only probes (wrong results).  Nothing in feddat_amd/, bench.py or tests/
    calls this; the production library rejects those flags (feddat_set_debug_flags -> EINVAL)."""
    global LIB_PATH
    if _lib is not None:
        raise FeddatHipError("use_ablation_build() must be called before the library is loaded")
    LIB_PATH = os.path.join(_PKG, "libfeddat_hip_ablate.so")


def set_debug_flags(flags: int):
    """Kernel-selection switches (bit-identical results, except dQ of the two-role attention backward that flag 2 selects at
    S <= 192: equally accurate, not bit-identical; its dK | dV are): 1 / 2 GEMMs on the two-group / one-wave-per-SIMD kernel, 32 / 64
    force 192- / 256-row tiles, 128 no small-tile kernel, 256 K = 32 fp8 MFMA, bit 23 one attention-backward block per pair,
    bits 28..31 cap the persistent GEMM grid, 1 | 2 together the dual form of the persistent GEMM (what they do to a given
    GEMM launch: gemm_route), bit 11 (2048) the four-wave weight-stationary adapter kernels instead of the two-wave-group
    ones.  The timing-only ablations (8 skip epilogue, 4 / 16, 512, bits 8..22, 24..26) exist in the ablation build only
    (use_ablation_build); there bit 11 is also part of the GEMM block cap (bits 8..19), which only GEMM launches read."""
    _chk(load().feddat_set_debug_flags(int(flags)), "feddat_set_debug_flags")


class Context:
    """feddat_ctx: explicit per-device handle (sets every kernel's launch attributes on that device at creation)."""

    def __init__(self, device: int):
        self._h = vp()
        self._lib = load()          # a handle belongs to the library (operand format) it was made by
        _chk(self._lib.feddat_ctx_create(int(device), C.byref(self._h)), "feddat_ctx_create")

    def info(self):
        d, cu = i32(), i32()
        _chk(self._lib.feddat_ctx_device(self._h, C.byref(d), C.byref(cu)), "feddat_ctx_device")
        return d.value, cu.value

    def close(self):
        if self._h:
            self._lib.feddat_ctx_destroy(self._h)
            self._h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gemm_dual_blocks_per_cu() -> int:
    """Workgroups per CU the runtime grants the dual form of the persistent GEMM (diagnostics)."""
    n = C.c_int(0)
    _chk(load().feddat_gemm_dual_blocks_per_cu(C.byref(n)), "feddat_gemm_dual_blocks_per_cu")
    return n.value


def gemm_route(M: int, N: int, K: int, epi: int, *, n_cu: int, kind: int = GEMM_OP16, flags: int = 0) -> dict:
    """The route gemm_bf16_nt (kind GEMM_OP16), gemm_fp8_nt / _f32 (GEMM_FP8) or gemm_fp8mx_nt (GEMM_FP8MX) gives this product on
    a device of n_cu compute units under the selection flags `flags`: kernel family (GEMM_V1 .. GEMM_DUAL), tile rows, launch
    geometry and tiling (feddat_gemm_route).  Host only: needs no device.  Raises where the entry point rejects the shape."""
    r = GemmRoute()
    _chk(load().feddat_gemm_route(M, N, K, epi, kind, n_cu, flags, C.byref(r)), "feddat_gemm_route")
    return {n: getattr(r, n) for n, _ in GemmRoute._fields_}


def rccl_available() -> bool:
    """True when the library could bind RCCL in this process (feddat_comm_info without a communicator: version only)."""
    v = C.c_int(0)
    return load().feddat_comm_info(None, C.byref(v), None, None) == 0      # (ELAUNCH when RCCL could not be bound; the version
    #                                                                          symbol itself is optional: diagnostics only)


class RcclComm:
    """ncclComm_t made through the C ABI (feddat_comm_*): rank 0 draws the unique id, `exchange(id_bytes) -> id_bytes`
    ships it to the other ranks over any host channel (torch.distributed object broadcast, a TCPStore, MPI, a file)."""

    def __init__(self, world: int, rank: int, exchange, timeout_s: float = 120.0):
        """timeout_s: watchdog on the collective ncclCommInitRank (feddat_comm_create_timeout): a peer that died or could not
        load RCCL makes this raise after timeout_s instead of hanging; 0 = wait forever."""
        buf = C.create_string_buffer(128)
        self._lib = load()
        rc0 = self._lib.feddat_comm_unique_id(buf) if rank == 0 else 0
        # rank 0 ships its return code with the id, so that a failure there (RCCL not loadable) raises on EVERY rank instead of
        # leaving the others waiting in the exchange
        msg = exchange(bytes([0 if rc0 == 0 else 1]) + bytes(buf.raw))
        if msg[0] != 0:
            raise FeddatHipError("feddat_comm_unique_id failed on rank 0 (is librccl loadable?)")
        ident = msg[1:]
        self._h = vp()
        _chk(self._lib.feddat_comm_create_timeout(C.c_char_p(ident), world, rank, int(timeout_s * 1000), C.byref(self._h)),
             "feddat_comm_create_timeout")
        self.world, self.rank = world, rank

    def fedavg_allreduce(self, flat, scratch, num: float, total: float):
        _dev(flat, scratch)
        _chk(self._lib.feddat_fedavg_allreduce(self._h, _p(flat), _p(scratch), flat.numel(), float(num), float(total),
                                            _stream()), "feddat_fedavg_allreduce")

    def info(self):
        """{'rccl_version': ncclGetVersion code, 'ranks': ranks of the communicator, 'rank': this rank} from the library."""
        v, n, r = C.c_int(0), C.c_int(0), C.c_int(0)
        _chk(self._lib.feddat_comm_info(self._h, C.byref(v), C.byref(n), C.byref(r)), "feddat_comm_info")
        return {"rccl_version": v.value, "ranks": n.value, "rank": r.value}

    def close(self):
        if self._h:
            self._lib.feddat_comm_destroy(self._h)
            self._h = vp()


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(rc: int, what: str):
    if rc != 0:
        raise FeddatHipError(f"{what} failed with code {rc} ({ {1: 'EINVAL', 2: 'ELAUNCH', 3: 'ETIMEOUT'}.get(rc, '?') })")


def _ext(name: str):
    """The bound function `name` of the extension header include/feddat_hip_albef.h, from the calling thread's library."""
    if name not in _ALBEF_SIGS:
        raise FeddatHipError(f"{name} is not declared in include/feddat_hip_albef.h")
    return getattr(load(), name)


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise FeddatHipError("feddat_amd ops need device (HIP) tensors; there is no CPU path")


# ---------------------------------------------------------------------------------------------------
# thin typed wrappers (tensors in, tensors out; no arithmetic happens on the Python side)
# ---------------------------------------------------------------------------------------------------
def gemm_skinny_workspace_elems(M: int, N: int, K: int) -> int:
    return int(load().feddat_gemm_skinny_workspace_elems(M, N, K))


def gemm_bf16_nt(A, B, epi, *, bias=None, resid=None, aux=None, out_f32=None, out_bf16=None, out2_bf16=None,
                 M=None, skinny_workspace=None):
    """C[M,N] = A[M,K] @ B[N,K]^T (+ epilogue).  A, B bf16 2-D (row stride taken from the tensors).
    With M <= 64 and a fp32 `skinny_workspace` the split-K skinny kernel pair is used."""
    _dev(A, B)
    M = A.shape[0] if M is None else M
    K = A.shape[1]
    N = B.shape[0]

    def ld(t):
        return 0 if t is None else t.stride(0)
    if skinny_workspace is not None and M <= 64:
        _dev(skinny_workspace)
        rc = load().feddat_gemm_bf16_nt_skinny(_p(A), A.stride(0), _p(B), B.stride(0), M, N, K, epi, _p(bias),
                                               _p(resid), ld(resid), _p(aux), ld(aux), _p(out_f32), ld(out_f32),
                                               _p(out_bf16), ld(out_bf16), _p(out2_bf16), ld(out2_bf16),
                                               _p(skinny_workspace), skinny_workspace.numel(), _stream())
        _chk(rc, "feddat_gemm_bf16_nt_skinny")
        return
    rc = load().feddat_gemm_bf16_nt(_p(A), A.stride(0), _p(B), B.stride(0), M, N, K, epi, _p(bias), _p(resid),
                                    ld(resid), _p(aux), ld(aux), _p(out_f32), ld(out_f32), _p(out_bf16),
                                    ld(out_bf16), _p(out2_bf16), ld(out2_bf16), _stream())
    _chk(rc, "feddat_gemm_bf16_nt")


def gemm_fp8_nt(A8, a_scale, B8, b_scale, epi, *, bias=None, aux=None, out_bf16=None, out2_bf16=None):
    """C = (A8 @ B8^T) * a_scale[:, None] * b_scale[None, :] (+ bias; epilogue EPI_BF16, EPI_GELU or EPI_MUL_DGELU with aux);
    A8 / B8: e4m3 bytes as uint8 / float8 tensors [M,K] / [N,K]."""
    _dev(A8, B8, a_scale, b_scale, out_bf16, aux)
    M, K = A8.shape
    N = B8.shape[0]
    _chk(load().feddat_gemm_fp8_nt(_p(A8), A8.stride(0), _p(a_scale), _p(B8), B8.stride(0), _p(b_scale), M, N, K, epi,
                                   _p(bias), _p(aux), 0 if aux is None else aux.stride(0), _p(out_bf16), out_bf16.stride(0),
                                   _p(out2_bf16),
                                   0 if out2_bf16 is None else out2_bf16.stride(0), _stream()), "feddat_gemm_fp8_nt")


def gemm_fp8mx_nt(A8, a_mx, B8, b_scale, *, bias=None, out_bf16=None):
    """out = (A . B^T) * b_scale[None, :] + bias with A = A8 (e4m3) * 2^(a_mx - 127) per (row, 32-column block): a_mx uint8
    [M, K / 32] E8M0 block scales applied by the MFMA itself (feddat_gemm_fp8mx_nt)."""
    _dev(A8, a_mx, B8, b_scale, out_bf16)
    M, K = A8.shape
    N = B8.shape[0]
    _chk(load().feddat_gemm_fp8mx_nt(_p(A8), A8.stride(0), _p(a_mx), a_mx.stride(0), _p(B8), B8.stride(0), _p(b_scale), M, N, K,
                                     _p(bias), _p(out_bf16), out_bf16.stride(0), _stream()), "feddat_gemm_fp8mx_nt")


def gemm_fp8_nt_f32(A8, a_scale, B8, b_scale, *, bias=None, resid=None, out_f32=None):
    """out_f32 = (A8 @ B8^T) * a_scale[:, None] * b_scale[None, :] + bias (+ resid)."""
    _dev(A8, B8, a_scale, b_scale, out_f32, resid, bias)
    M, K = A8.shape
    N = B8.shape[0]
    _chk(load().feddat_gemm_fp8_nt_f32(_p(A8), A8.stride(0), _p(a_scale), _p(B8), B8.stride(0), _p(b_scale), M, N, K, _p(bias),
                                       _p(resid), 0 if resid is None else resid.stride(0), _p(out_f32), out_f32.stride(0),
                                       _stream()), "feddat_gemm_fp8_nt_f32")


def quant_rows_fp8(x, y8, scale):
    _dev(x, y8, scale)
    _chk(load().feddat_quant_rows_fp8(_p(x), x.stride(0), x.shape[0], x.shape[1], _p(y8), _p(scale), _stream()),
         "feddat_quant_rows_fp8")


def layernorm_fwd_fp8(x, gamma, beta, eps, rows, H, y_fp8, y_scale, *, y_bf16=None, stats=None, x_stride=None):
    _dev(x, y_fp8, y_scale)
    _chk(load().feddat_layernorm_fwd_fp8(_p(x), H if x_stride is None else x_stride, _p(gamma), _p(beta), eps, rows, H,
                                         _p(y_fp8), _p(y_scale), _p(y_bf16), _p(stats), _stream()), "feddat_layernorm_fwd_fp8")


def attn_fwd(qkv, ctx, lse, B, S, heads, key_mask=None):
    _dev(qkv, ctx)
    _chk(load().feddat_attn_fwd(_p(qkv), _p(key_mask), _p(ctx), _p(lse), B, S, heads, _stream()), "feddat_attn_fwd")


def attn_bwd(qkv, ctx, lse, dctx, dqkv, B, S, heads, key_mask=None):
    _dev(qkv, ctx, dctx, dqkv)
    _chk(load().feddat_attn_bwd(_p(qkv), _p(key_mask), _p(ctx), _p(lse), _p(dctx), _p(dqkv), B, S, heads, _stream()),
         "feddat_attn_bwd")


def attn_bwd_fp8mx(qkv, ctx, lse, dctx, dq8, dq_scale, B, S, heads, key_mask=None):
    """attn_bwd with dq | dk | dv as MX-scaled e4m3: dq8 uint8 [B S, 3 H], dq_scale uint8 [B S, 3 H / 32] (E8M0 per 32 columns)."""
    _dev(qkv, ctx, dctx, dq8, dq_scale)
    _chk(load().feddat_attn_bwd_fp8mx(_p(qkv), _p(key_mask), _p(ctx), _p(lse), _p(dctx), _p(dq8), _p(dq_scale), B, S, heads,
                                      _stream()), "feddat_attn_bwd_fp8mx")


def attn_cls_fwd(qkv, ctx, lse, B, S, heads, key_mask=None):
    """Attention for token 0 of every sample only (the last layer): writes ctx rows b*S and lse[b, h, 0]."""
    _dev(qkv, ctx)
    _chk(load().feddat_attn_cls_fwd(_p(qkv), _p(key_mask), _p(ctx), _p(lse), B, S, heads, _stream()), "feddat_attn_cls_fwd")


def attn_cls_bwd(qkv, ctx, lse, dctx0, dqkv, B, S, heads, key_mask=None):
    """dctx0: fp32 [B, H] gradient of the token-0 context rows -> the complete dqkv."""
    _dev(qkv, ctx, dctx0, dqkv)
    assert dctx0.dtype == torch.float32 and dctx0.is_contiguous()
    _chk(load().feddat_attn_cls_bwd(_p(qkv), _p(key_mask), _p(ctx), _p(lse), _p(dctx0), _p(dqkv), B, S, heads, _stream()),
         "feddat_attn_cls_bwd")


def attn2_fwd(q, k, v, ctx, lse, B, Sq, Skv, heads, *, key_mask=None, causal=False, q_rows=None, kv_rows=None, drop=None):
    """General attention: q [B*q_rows, >=heads*64] / k, v [B*kv_rows, ...] bf16 2-D views (row strides from the tensors).
    drop = (p, key0, key1, step_counter) applies dropout to the attention probabilities (xbert.py:333)."""
    _dev(q, k, v, ctx)
    if drop is not None and drop[0] > 0:
        _chk(load().feddat_attn2_fwd_dropout(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(key_mask),
                                             int(causal), _p(ctx), ctx.stride(0), _p(lse), B, Sq, Skv,
                                             Sq if q_rows is None else q_rows, Skv if kv_rows is None else kv_rows, heads,
                                             drop[0], drop[1], drop[2], _p(drop[3]), _stream()), "feddat_attn2_fwd_dropout")
        return
    _chk(load().feddat_attn2_fwd(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(key_mask), int(causal),
                                 _p(ctx), ctx.stride(0), _p(lse), B, Sq, Skv, Sq if q_rows is None else q_rows,
                                 Skv if kv_rows is None else kv_rows, heads, _stream()), "feddat_attn2_fwd")


def attn2_bwd(q, k, v, ctx, lse, dctx, dsum_ws, dq, dk, dv, B, Sq, Skv, heads, *, key_mask=None, causal=False,
              q_rows=None, kv_rows=None, drop=None):
    _dev(q, k, v, ctx, dctx, dq, dk, dv)
    if drop is not None and drop[0] > 0:
        _chk(load().feddat_attn2_bwd_dropout(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(key_mask),
                                             int(causal), _p(ctx), ctx.stride(0), _p(lse), _p(dctx), dctx.stride(0),
                                             _p(dsum_ws), _p(dq), dq.stride(0), _p(dk), dk.stride(0), _p(dv), dv.stride(0), B, Sq,
                                             Skv, Sq if q_rows is None else q_rows, Skv if kv_rows is None else kv_rows, heads,
                                             drop[0], drop[1], drop[2], _p(drop[3]), _stream()), "feddat_attn2_bwd_dropout")
        return
    _chk(load().feddat_attn2_bwd(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(key_mask), int(causal),
                                 _p(ctx), ctx.stride(0), _p(lse), _p(dctx), dctx.stride(0), _p(dsum_ws), _p(dq),
                                 dq.stride(0), _p(dk), dk.stride(0), _p(dv), dv.stride(0), B, Sq, Skv,
                                 Sq if q_rows is None else q_rows, Skv if kv_rows is None else kv_rows, heads, _stream()),
         "feddat_attn2_bwd")


def layernorm_fwd(x, gamma, beta, eps, rows, H, *, x_stride=None, y_bf16=None, y_f32=None, stats=None):
    _dev(x)
    _chk(load().feddat_layernorm_fwd(_p(x), H if x_stride is None else x_stride, _p(gamma), _p(beta), eps, rows, H,
                                     _p(y_bf16), _p(y_f32), _p(stats), _stream()), "feddat_layernorm_fwd")


def layernorm_bwd_dx(x, stats, gamma, rows, H, *, dy_bf16=None, dy_f32=None, dy_stride=None, x_stride=None,
                     dres=None, dres_stride=None, out_f32=None, out_stride=None, out_bf16=None, dres_every=0):
    """dres_every = E > 0: dres is compact, its row r / E belongs to output row r for r % E == 0 (feddat_layernorm_bwd_dx_sparse)."""
    _dev(x)
    if dres_every:
        _dev(dres)
        _chk(load().feddat_layernorm_bwd_dx_sparse(_p(dy_bf16), _p(dy_f32), H if dy_stride is None else dy_stride, _p(x),
                                                   H if x_stride is None else x_stride, _p(stats), _p(gamma), _p(dres),
                                                   H if dres_stride is None else dres_stride, int(dres_every), rows, H,
                                                   _p(out_f32), H if out_stride is None else out_stride, _p(out_bf16), _stream()),
             "feddat_layernorm_bwd_dx_sparse")
        return
    _chk(load().feddat_layernorm_bwd_dx(_p(dy_bf16), _p(dy_f32), H if dy_stride is None else dy_stride, _p(x),
                                        H if x_stride is None else x_stride, _p(stats), _p(gamma), _p(dres),
                                        H if dres_stride is None else dres_stride, rows, H, _p(out_f32),
                                        H if out_stride is None else out_stride, _p(out_bf16), _stream()),
         "feddat_layernorm_bwd_dx")


def layernorm_bwd_dx_fp8(x, stats, gamma, rows, H, out_fp8, out_scale, *, dy_bf16=None, dy_f32=None, dres=None, out_f32=None,
                         out_bf16=None):
    """layernorm_bwd_dx whose result also leaves as e4m3 rows + per-row scale (the A operand of an fp8 dX product)."""
    _dev(x, out_fp8, out_scale)
    _chk(load().feddat_layernorm_bwd_dx_fp8(_p(dy_bf16), _p(dy_f32), H, _p(x), H, _p(stats), _p(gamma), _p(dres), H, rows, H,
                                            _p(out_f32), H, _p(out_bf16), _p(out_fp8), _p(out_scale), _stream()),
         "feddat_layernorm_bwd_dx_fp8")


def layernorm_bwd_full(dy, x, stats, gamma, rows, H, dx, dgamma, dbeta):
    _dev(dy, x)
    _chk(load().feddat_layernorm_bwd_full(_p(dy), _p(x), _p(stats), _p(gamma), rows, H, _p(dx), _p(dgamma),
                                          _p(dbeta), _stream()), "feddat_layernorm_bwd_full")


def make_segs(segs: Sequence[dict]):
    arr = (AdapterSeg * len(segs))()
    for s, d in zip(arr, segs):
        s.row_begin, s.row_end = d["row_begin"], d["row_end"]
        ads = d["adapters"]  # list of dicts with wd, wdT, wu, wuT (bf16), bd, bu (fp32), scale
        s.n_adapters = len(ads)
        s.train_slot = d.get("train_slot", -1)
        s.x_row_delta = d.get("x_row_delta", 0)
        for a, ad in enumerate(ads):
            s.scale[a] = ad["scale"]
            s.wd[a] = ad["wd"].data_ptr()
            s.wu[a] = ad["wu"].data_ptr()
            s.wdT[a] = ad["wdT"].data_ptr() if ad.get("wdT") is not None else None
            s.wuT[a] = ad["wuT"].data_ptr() if ad.get("wuT") is not None else None
            s.bd[a] = ad["bd"].data_ptr()
            s.bu[a] = ad["bu"].data_ptr()
    return arr


def adapter_fwd(x, out, segs_arr, T, H=768, r=48, z_save=None):
    """z_save: optional fp32 [T, 2, r] receiving relu(W_down x + b_down) per adapter slot (for adapter_bwd's z_saved)."""
    _dev(x, out, z_save)
    _chk(load().feddat_adapter_fwd(_p(x), _p(out), T, H, r, segs_arr, len(segs_arr), _p(z_save), _stream()),
         "feddat_adapter_fwd")


def adapter_fwd_ln(x, out, segs_arr, T, gamma, beta, eps, y_bf16, stats=None, H=768, r=48, z_save=None):
    """adapter_fwd + the next layer's LayerNorm of the output rows (bf16 y, [T,2] stats)."""
    _dev(x, out, y_bf16, z_save)
    _chk(load().feddat_adapter_fwd_ln(_p(x), _p(out), T, H, r, segs_arr, len(segs_arr), _p(gamma), _p(beta), eps,
                                      _p(y_bf16), _p(stats), _p(z_save), _stream()), "feddat_adapter_fwd_ln")


def adapter_bwd(x, dy, dx, segs_arr, T, *, dx_bf16=None, z_out=None, dz_out=None, z_saved=None, H=768, r=48):
    """x may be None when z_saved (the forward's z_save) is given: the backward then does not read x at all."""
    _dev(x, dy, dx, z_saved)
    if x is None and z_saved is None:
        raise FeddatHipError("adapter_bwd needs x or z_saved")
    _chk(load().feddat_adapter_bwd(_p(x), _p(z_saved), _p(dy), _p(dx), _p(dx_bf16), _p(z_out), _p(dz_out), T, H, r,
                                   segs_arr, len(segs_arr), _stream()), "feddat_adapter_bwd")


def adapter_bwd_fp8(dy, dx, dx_fp8, dx_scale, segs_arr, T, *, z_saved, z_out=None, dz_out=None, H=768, r=48):
    """adapter_bwd (saved-z form) whose dx also leaves as e4m3 rows + per-row scale."""
    _dev(dy, dx, dx_fp8, dx_scale, z_saved)
    _chk(load().feddat_adapter_bwd_fp8(_p(z_saved), _p(dy), _p(dx), _p(dx_fp8), _p(dx_scale), _p(z_out), _p(dz_out), T, H, r,
                                       segs_arr, len(segs_arr), _stream()), "feddat_adapter_bwd_fp8")


def make_wgrad_segs(segs: Sequence[dict]):
    arr = (WgradSeg * len(segs))()
    for s, d in zip(arr, segs):
        s.x, s.dy, s.z, s.dz, s.grad = (d[k].data_ptr() for k in ("x", "dy", "z", "dz", "grad"))
        s.rows, s.scale, s.grad_unscale = d["rows"], d["scale"], d.get("grad_unscale", 1.0)
        t = d.get("grad_unscale_dev")          # device float: 1 / the dynamic loss scale (ABI 8)
        s.grad_unscale_dev = t.data_ptr() if t is not None else None
    arr._keep = [d.get("grad_unscale_dev") for d in segs]
    return arr


def adapter_wgrad_workspace_elems(nseg: int) -> int:
    return int(load().feddat_adapter_wgrad_workspace_elems(nseg))


def adapter_wgrad_partial(segs_arr, partials, H=768, r=48):
    _dev(partials)
    _chk(load().feddat_adapter_wgrad_partial(segs_arr, len(segs_arr), _p(partials), partials.numel(), H, r, _stream()),
         "feddat_adapter_wgrad_partial")


def adapter_wgrad_reduce(grads_dev, n, nseg, partials, stride):
    """grads_dev: int64 device tensor [n * nseg] of gradient-buffer addresses; launch l's partials at partials[l * stride:]."""
    _dev(grads_dev, partials)
    _chk(load().feddat_adapter_wgrad_reduce(_p(grads_dev), n, nseg, _p(partials), stride, _stream()),
         "feddat_adapter_wgrad_reduce")


def adapter_wgrad_reduce_checked(grads_dev, n, nseg, partials, stride, nonfinite):
    """feddat_adapter_wgrad_reduce + GradScaler's inf check: nonfinite (int32 device tensor, >= nseg elements) is OR-ed per segment."""
    _dev(grads_dev, partials, nonfinite)
    assert nonfinite.dtype == torch.int32 and nonfinite.numel() >= nseg
    _chk(load().feddat_adapter_wgrad_reduce_checked(_p(grads_dev), n, nseg, _p(partials), stride, _p(nonfinite), _stream()),
         "feddat_adapter_wgrad_reduce_checked")


def adapter_wgrad(segs_arr, partials, H=768, r=48):
    _dev(partials)
    _chk(load().feddat_adapter_wgrad(segs_arr, len(segs_arr), _p(partials), partials.numel(), H, r, _stream()),
         "feddat_adapter_wgrad")


def adapter_pack_strided(wd, wu, stride32, wd16, wdT16, wu16, wuT16, stride16, n, H=768, r=48):
    _dev(wd, wu, wd16)
    _chk(load().feddat_adapter_pack_strided(_p(wd), _p(wu), stride32, _p(wd16), _p(wdT16), _p(wu16), _p(wuT16), stride16,
                                            n, H, r, _stream()), "feddat_adapter_pack_strided")


def adapter_pack(wd, wu, wd16, wdT16, wu16, wuT16, H=768, r=48):
    _dev(wd, wu)
    _chk(load().feddat_adapter_pack(_p(wd), _p(wu), _p(wd16), _p(wdT16), _p(wu16), _p(wuT16), H, r, _stream()),
         "feddat_adapter_pack")


def vilt_layer_fwd(ctx: "Context", W, A, nb, S, heads, segs_arr, *, key_mask=None, ln1_done=False, next_ln_g=None,
                   next_ln_b=None):
    """One ViltLayer + Adaptered_ViltOutput forward as ONE C-ABI call (W / A: ViltLayerWeights / ViltLayerActs structs)."""
    _chk(load().feddat_vilt_layer_fwd(ctx._h, C.byref(W), C.byref(A), nb, S, heads, _p(key_mask), int(ln1_done), segs_arr,
                                      len(segs_arr), _p(next_ln_g), _p(next_ln_b), _stream()), "feddat_vilt_layer_fwd")


def vilt_layer_bwd(ctx: "Context", W, A, G, nb, S, heads, segs_arr, wsegs_arr, partials, *, key_mask=None,
                   wgrad_reduce_now=True):
    _chk(load().feddat_vilt_layer_bwd(ctx._h, C.byref(W), C.byref(A), C.byref(G), nb, S, heads, _p(key_mask), segs_arr,
                                      len(segs_arr), wsegs_arr, 0 if wsegs_arr is None else len(wsegs_arr), _p(partials),
                                      0 if partials is None else partials.numel(), int(wgrad_reduce_now), _stream()),
         "feddat_vilt_layer_bwd")


def sgemm_f32(A, sa_i, sa_k, B, sb_k, sb_j, I, J, K, out, *, ldo=None, ksplit=1, alpha=1.0, bias_j=None,
              out_split_stride=0, colsum=None, colsum_split_stride=None):
    _dev(A, B, out)
    _chk(load().feddat_sgemm_f32(_p(A), sa_i, sa_k, _p(B), sb_k, sb_j, I, J, K, ksplit, alpha, _p(bias_j), _p(out),
                                 J if ldo is None else ldo, out_split_stride, _p(colsum),
                                 I if colsum_split_stride is None else colsum_split_stride, _stream()),
         "feddat_sgemm_f32")


def reduce_partials(inp, stride, nsplit, n, out):
    _dev(inp, out)
    _chk(load().feddat_reduce_partials(_p(inp), stride, nsplit, n, _p(out), _stream()), "feddat_reduce_partials")


def dat_loss_fwd_bwd(logits, teacher, target, dlogits, scalars, temp=3.0):
    _dev(logits, teacher, target)
    B, Cn = logits.shape
    assert scalars.numel() >= 4 + 2 * B
    _chk(load().feddat_dat_loss_fwd_bwd(_p(logits), _p(teacher), _p(target), B, Cn, temp, _p(dlogits), _p(scalars),
                                        _stream()), "feddat_dat_loss_fwd_bwd")


def ht_job(A, sa_i, sa_k, B, sb_k, sb_j, I, J, K, out, ldo=None, mode=0, alpha=1.0, bias_j=None, colsum=None, pro=HT_PRO_NONE,
           pro_a=None, pro_b=None, pro_eps=0.0, stats_out=None, epi=HT_EPI_NONE, aux=None, ld_aux=0, alpha_dev=None) -> HtJob:
    """One product of feddat_head_gemm (include/feddat_hip.h: feddat_ht_job); keeps its tensors alive."""
    _dev(A, B, out)
    j = HtJob()
    j._keep = (A, B, out, bias_j, colsum, pro_a, pro_b, stats_out, aux, alpha_dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    j.A, j.sa_i, j.sa_k, j.B, j.sb_k, j.sb_j = ptr(A), sa_i, sa_k, ptr(B), sb_k, sb_j
    j.I, j.J, j.K, j.mode, j.alpha = I, J, K, mode, alpha
    j.bias_j, j.out, j.ldo, j.colsum = ptr(bias_j), ptr(out), (J if ldo is None else ldo), ptr(colsum)
    j.pro, j.pro_a, j.pro_b, j.pro_eps, j.stats_out = pro, ptr(pro_a), ptr(pro_b), pro_eps, ptr(stats_out)
    j.epi, j.aux, j.ld_aux, j.alpha_dev = epi, ptr(aux), ld_aux, ptr(alpha_dev)
    return j


def head_gemm(*jobs: HtJob):
    """One launch for one or two independent small fp32 products (feddat_head_gemm)."""
    arr = (HtJob * len(jobs))(*jobs)
    arr._keep = jobs
    _chk(load().feddat_head_gemm(arr, len(jobs), _stream()), "feddat_head_gemm")


def head_gemm_plan(job: HtJob) -> dict:
    """The path and grid feddat_head_gemm gives this job: avec / bvec (16-byte or dword loads of A / B), jt (16-column tiles per
    wave), itiles, jblocks, blocks (feddat_head_gemm_plan).  Host only: needs no device and reads only the job's sizes, strides
    and pointer values, so the job may hold made-up addresses.  Raises where head_gemm rejects the job."""
    p = HtPlan()
    _chk(load().feddat_head_gemm_plan(C.byref(job), C.byref(p)), "feddat_head_gemm_plan")
    return {n: getattr(p, n) for n, _ in HtPlan._fields_}


def head_ln_gelu(x, gamma, beta, eps, y, stats, gelu_out):
    _dev(x, y, stats, gelu_out)
    _chk(load().feddat_head_ln_gelu(_p(x), _p(gamma), _p(beta), eps, x.shape[0], x.shape[1], _p(y), _p(stats), _p(gelu_out),
                                    _stream()), "feddat_head_ln_gelu")


def head_ln_bwd_full(dy, x, stats, gamma, dx, dgamma, dbeta):
    _dev(dy, x, stats, dx)
    _chk(load().feddat_head_ln_bwd_full(_p(dy), _p(x), _p(stats), _p(gamma), x.shape[0], x.shape[1], _p(dx), _p(dgamma),
                                        _p(dbeta), _stream()), "feddat_head_ln_bwd_full")


def dat_loss_fwd_bwd_single(logits, teacher, target, dlogits, scalars, temp=3.0):
    _dev(logits, teacher, target)
    B, Cn = logits.shape
    assert scalars.numel() >= 4
    _chk(load().feddat_dat_loss_fwd_bwd_single(_p(logits), _p(teacher), _p(target), B, Cn, temp, _p(dlogits), _p(scalars),
                                               _stream()), "feddat_dat_loss_fwd_bwd_single")


def dat_loss_fwd_bwd_checked(logits, teacher, target, dlogits, scalars, nonfinite, temp=3.0):
    """dat_loss_fwd_bwd_single that also ORs 1 into nonfinite[0] (int32 device tensor) when the loss is inf / NaN."""
    _dev(logits, teacher, target, nonfinite)
    B, Cn = logits.shape
    assert scalars.numel() >= 4 and nonfinite.dtype == torch.int32
    _chk(load().feddat_dat_loss_fwd_bwd_checked(_p(logits), _p(teacher), _p(target), B, Cn, temp, _p(dlogits), _p(scalars),
                                                _p(nonfinite), _stream()), "feddat_dat_loss_fwd_bwd_checked")


def dat_step_finish(head_state, ad1_state, ad0_state, flags, scaler_f, scaler_i, growth=2.0, backoff=0.5, growth_interval=2000):
    """End of a dat train_step under the dynamic loss scale (include/feddat_hip.h: feddat_dat_step_finish)."""
    _dev(head_state, ad1_state, ad0_state, flags, scaler_f, scaler_i)
    _chk(load().feddat_dat_step_finish(_p(head_state), _p(ad1_state), _p(ad0_state), _p(flags), _p(scaler_f), _p(scaler_i),
                                       growth, backoff, growth_interval, _stream()), "feddat_dat_step_finish")


def bce_loss_fwd_bwd(logits, target, dlogits, scalars, nonfinite=None):
    """scalars[0] = BCEWithLogits_mean(logits, target) * C, dlogits = (sigmoid(logits) - target) / B; nonfinite (int32 device
    tensor, optional) gets 1 OR-ed in when the loss is inf / NaN (include/feddat_hip.h: feddat_bce_loss_fwd_bwd)."""
    _dev(logits, target, dlogits, scalars)
    B, Cn = logits.shape
    assert scalars.numel() >= 1 and (nonfinite is None or nonfinite.dtype == torch.int32)
    _chk(load().feddat_bce_loss_fwd_bwd(_p(logits), _p(target), B, Cn, _p(dlogits), _p(scalars),
                                        _p(nonfinite), _stream()), "feddat_bce_loss_fwd_bwd")


def dat_loss_fwd_bwd_rows(logits, teacher, target, dlogits, scalars, n, nonfinite=None, temp=3.0):
    """The DAT loss of rows [0, n) of a B-row frame (n <= B = dlogits.shape[0]): dlogits[:n] and scalars[:3] as
    dat_loss_fwd_bwd_checked gives on the [:n] views, dlogits[n:] = 0 (include/feddat_hip.h: feddat_dat_loss_fwd_bwd_rows)."""
    _dev(logits, teacher, target, dlogits, scalars, nonfinite)
    B, Cn = dlogits.shape
    assert scalars.numel() >= 4 and (nonfinite is None or nonfinite.dtype == torch.int32)
    assert logits.shape[0] >= n and teacher.shape[0] >= n and target.shape[0] >= n and logits.shape[1] == Cn
    _chk(load().feddat_dat_loss_fwd_bwd_rows(_p(logits), _p(teacher), _p(target), int(n), B, Cn, temp, _p(dlogits), _p(scalars),
                                             _p(nonfinite), _stream()), "feddat_dat_loss_fwd_bwd_rows")


def dat_loss_wide_workspace_elems(B: int) -> int:
    """Floats of the row-term workspace dat_loss_fwd_bwd_wide needs for a B-row frame (2 B)."""
    return int(load().feddat_dat_loss_wide_workspace_elems(int(B)))


def dat_loss_fwd_bwd_wide(logits, teacher, target, dlogits, scalars, workspace, n=None, nonfinite=None, temp=3.0):
    """The DAT loss at any width (include/feddat_hip.h: feddat_dat_loss_fwd_bwd_wide): rows [0, n) of the B-row frame
    (B = dlogits.shape[0]; n = None: all of them), dlogits[n:] = 0; nonfinite (int32 device tensor, optional) gets 1 OR-ed in
    when the loss is inf / NaN; workspace: fp32 device tensor of at least dat_loss_wide_workspace_elems(B) elements."""
    _dev(logits, teacher, target, dlogits, scalars, workspace, nonfinite)
    B, Cn = dlogits.shape
    n = B if n is None else int(n)
    assert scalars.numel() >= 4 and (nonfinite is None or nonfinite.dtype == torch.int32)
    assert workspace.dtype == torch.float32 and workspace.is_contiguous()
    for t in (logits, teacher, target, dlogits):      # the kernel indexes all four as [b * C + j]
        assert t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and t.shape[1] == Cn and t.shape[0] >= n
    assert scalars.dtype == torch.float32 and scalars.is_contiguous() and 1 <= n <= B
    _chk(load().feddat_dat_loss_fwd_bwd_wide(_p(logits), _p(teacher), _p(target), n, B, Cn, temp, _p(dlogits), _p(scalars),
                                             _p(nonfinite), _p(workspace), workspace.numel(), _stream()),
         "feddat_dat_loss_fwd_bwd_wide")


def bce_loss_fwd_bwd_rows(logits, target, dlogits, scalars, n, nonfinite=None):
    """bce_loss_fwd_bwd of rows [0, n) of a B-row frame (n <= B = dlogits.shape[0]); dlogits[n:] = 0
    (include/feddat_hip.h: feddat_bce_loss_fwd_bwd_rows)."""
    _dev(logits, target, dlogits, scalars, nonfinite)
    B, Cn = dlogits.shape
    assert scalars.numel() >= 1 and (nonfinite is None or nonfinite.dtype == torch.int32)
    assert logits.shape[0] >= n and target.shape[0] >= n and logits.shape[1] == Cn
    _chk(load().feddat_bce_loss_fwd_bwd_rows(_p(logits), _p(target), int(n), B, Cn, _p(dlogits), _p(scalars), _p(nonfinite),
                                             _stream()), "feddat_bce_loss_fwd_bwd_rows")


# ---- gradients of per-column vectors (optimizer_mode bias / norm; include/feddat_hip.h, csrc/vector_grad.hip)
def vector_grad_workspace_elems(rows: int, N: int) -> int:
    """Floats of one partial buffer for `rows` rows of N columns (slabs * N)."""
    return int(load().feddat_vector_grad_workspace_elems(int(rows), int(N)))


def _rows_of(t, what):
    """(16-bit pointer, fp32 pointer, row stride) of a [rows, N] matrix whose rows are contiguous."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise FeddatHipError(f"{what} must be a [rows, N] matrix with contiguous rows")
    if t.dtype == torch.float32:
        return None, _p(t), t.stride(0)
    if t.dtype != OPERAND_DTYPE[current_operands()]:
        raise FeddatHipError(f"{what} must be fp32 or the bound library's operand format, got {t.dtype}")
    return _p(t), None, t.stride(0)


def colsum_partial(x, partials, row_mask=None):
    """partials[s] = sum of the rows of slab s of x [rows, N] (16-bit operands or fp32; row stride = x.stride(0)); row_mask:
    optional uint8 [rows], rows with 0 are left out.  Returns the number of slabs written."""
    _dev(x, partials, row_mask)
    p16, p32, ld = _rows_of(x, "x")
    rows, N = x.shape
    assert partials.dtype == torch.float32 and partials.is_contiguous()
    assert row_mask is None or (row_mask.dtype == torch.uint8 and row_mask.numel() == rows and row_mask.is_contiguous())
    _chk(load().feddat_colsum_partial(p16, p32, ld, _p(row_mask), rows, N, _p(partials), partials.numel(), _stream()),
         "feddat_colsum_partial")
    return vector_grad_workspace_elems(rows, N) // N


def ln_param_grad_partial(dy, x, stats, dbeta_partials, dgamma_partials=None):
    """One pass over the rows of a LayerNorm: dbeta_partials[s] = sum dy, dgamma_partials[s] = sum dy * xhat (None: beta
    alone, x and stats are not read).  dy 16-bit operands or fp32, x fp32, stats the saved {mean, rstd} rows."""
    _dev(dy, x, stats, dbeta_partials, dgamma_partials)
    p16, p32, ld = _rows_of(dy, "dy")
    rows, N = dy.shape
    n = dbeta_partials.numel()
    assert dbeta_partials.dtype == torch.float32 and dbeta_partials.is_contiguous()
    xs = 0
    if dgamma_partials is not None:
        assert dgamma_partials.dtype == torch.float32 and dgamma_partials.is_contiguous() and dgamma_partials.numel() >= n
        assert x.dtype == torch.float32 and x.stride(1) == 1 and x.shape[0] >= rows and stats.dtype == torch.float32
        assert stats.is_contiguous() and stats.numel() >= 2 * rows
        xs = x.stride(0)
    _chk(load().feddat_ln_param_grad_partial(p16, p32, ld, _p(x), xs, _p(stats), rows, N, _p(dgamma_partials),
                                             _p(dbeta_partials), n, _stream()), "feddat_ln_param_grad_partial")
    return vector_grad_workspace_elems(rows, N) // N


def make_vgrad_jobs(jobs, device):
    """Device-resident feddat_vgrad_job table from [(partials, slabs, grad[, flags])] (grad: the N-float slice of a flat
    gradient buffer the job writes; flags: VGRAD_UNSCALED).  Returns (table, njobs, max_n); the caller keeps the tensors alive."""
    arr = (VgradJob * len(jobs))()
    for j, (part, slabs, grad, *fl) in zip(arr, jobs):
        j.flags = fl[0] if fl else 0
        _dev(part, grad)
        assert part.dtype == torch.float32 and grad.dtype == torch.float32 and grad.is_contiguous()
        assert part.numel() >= slabs * grad.numel()
        j.partials, j.grad, j.slabs, j.n = part.data_ptr(), grad.data_ptr(), int(slabs), grad.numel()
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    return table, len(jobs), max(job[2].numel() for job in jobs)


def vector_grad_reduce(table, njobs, max_n, unscale=1.0, unscale_dev=None, nonfinite=None):
    """Fold every job's partials into its gradient slice, times unscale * unscale_dev[0]; nonfinite (int32 device tensor,
    optional) gets 1 OR-ed in on an inf / NaN (include/feddat_hip.h: feddat_vector_grad_reduce)."""
    _dev(table, unscale_dev, nonfinite)
    assert nonfinite is None or nonfinite.dtype == torch.int32
    _chk(load().feddat_vector_grad_reduce(_p(table), njobs, max_n, unscale, _p(unscale_dev), _p(nonfinite), _stream()),
         "feddat_vector_grad_reduce")


# ---- prompt tuning (optimizer_mode prompt; include/feddat_hip_prompt.h, csrc/prompt.hip)
PROMPT_ROWS = 5      # rows per insertion point: the reference's prompt_tokens = arange(5)


def prompt_row_map(Lt: int, Np: int):
    """Pure host function: the source of every row of the prompted frame of S = Lt + 1 + Np + 10 rows, as
    feddat_prompt_frame_assemble lays it out: ("src", r) = row r of the unprompted [text(Lt) | CLS | patches(Np)] frame,
    ("prompt", j, m) = P[j] + modality[m]."""
    n = PROMPT_ROWS
    if Lt < 1 or Np < 1:
        raise FeddatHipError(f"a prompted frame needs at least one text token and one patch, got Lt = {Lt}, Np = {Np}")
    rows = [("src", 0)] + [("prompt", j, 0) for j in range(n)] + [("src", r) for r in range(1, Lt + 1)]
    rows += [("prompt", j, 1) for j in range(n)] + [("src", r) for r in range(Lt + 1, Lt + 1 + Np)]
    return rows


def prompt_frame_assemble(h_in, key_mask_in, P, mod0, mod1, h_out, key_mask_out, B, Lt, Np, H, nrep=1):
    """h_in fp32 [B, Lt + 1 + Np, H] + the five prompt rows P [5, H] -> h_out fp32 [B, Lt + 1 + Np + 10, H] and, when
    key_mask_out (uint8 [nrep * B, S]) is given, its key mask from key_mask_in (uint8, row stride Lt + 1 + Np)."""
    _dev(h_in, key_mask_in, P, mod0, mod1, h_out, key_mask_out)
    S0 = Lt + 1 + Np
    assert h_in.dtype == h_out.dtype == P.dtype == torch.float32 and h_in.is_contiguous() and h_out.is_contiguous()
    assert h_in.numel() >= B * S0 * H and h_out.numel() >= B * (S0 + 2 * PROMPT_ROWS) * H and P.numel() >= PROMPT_ROWS * H
    assert P.is_contiguous() and mod0.numel() >= H and mod1.numel() >= H
    if key_mask_out is not None:
        assert key_mask_in.dtype == key_mask_out.dtype == torch.uint8 and key_mask_in.is_contiguous()
        assert key_mask_out.is_contiguous() and key_mask_in.numel() >= B * S0
        assert key_mask_out.numel() >= nrep * B * (S0 + 2 * PROMPT_ROWS)
    _chk(load().feddat_prompt_frame_assemble(_p(h_in), _p(key_mask_in), _p(P), _p(mod0), _p(mod1), _p(h_out), _p(key_mask_out),
                                             B, Lt, Np, H, nrep, _stream()), "feddat_prompt_frame_assemble")


def prompt_grad_gather(dh0, B, S, Lt, H, G, unscale=1.0, unscale_dev=None, nonfinite=None):
    """G [5, H] = sum over the samples of the ten prompt rows' gradient in dh0 fp32 [B, S, H] (text row, then image row, b
    ascending), times unscale * unscale_dev[0]; nonfinite (int32 device tensor, optional) gets 1 OR-ed in on an inf / NaN."""
    _dev(dh0, G, unscale_dev, nonfinite)
    assert dh0.dtype == G.dtype == torch.float32 and dh0.is_contiguous() and G.is_contiguous()
    assert dh0.numel() >= B * S * H and G.numel() >= PROMPT_ROWS * H
    assert nonfinite is None or nonfinite.dtype == torch.int32
    _chk(load().feddat_prompt_grad_gather(_p(dh0), B, S, Lt, H, unscale, _p(unscale_dev), _p(G), _p(nonfinite), _stream()),
         "feddat_prompt_grad_gather")


def prompt_mlp_fwd(E, W1, b1, W2, b2, t, P):
    """The reference's prompt MLP on its five tokens, two dependent feddat_head_gemm launches: t = tanh(E W1^T + b1) [5, D]
    (kept for the backward), P = t W2^T + b2 [5, H].  E [5, H], W1 [D, H], W2 [H, D]."""
    n, H = E.shape
    D = W1.shape[0]
    head_gemm(ht_job(E, H, 1, W1, 1, H, n, D, H, t, bias_j=b1, epi=HT_EPI_TANH))
    head_gemm(ht_job(t, D, 1, W2, 1, D, n, H, D, P, bias_j=b2))


def prompt_mlp_bwd(G, t, E, W1, W2, dt, dE, dW1, db1, dW2, db2):
    """Backward of prompt_mlp_fwd from G = dL/dP [5, H], two feddat_head_gemm launches of two independent products each:
    {dW2 = G^T t with db2 = column sums of G; dt = G W2}, then with dz = dt * (1 - t^2) formed in the operand prologue
    {dW1 = dz^T E with db1 = column sums of dz; dE = dz W1}.  The outputs may be slices of a flat gradient buffer."""
    n, H = E.shape
    D = W1.shape[0]
    head_gemm(ht_job(G, 1, H, t, D, 1, H, D, n, dW2, mode=1, colsum=db2),
              ht_job(G, H, 1, W2, D, 1, n, D, H, dt))
    head_gemm(ht_job(dt, 1, D, E, H, 1, D, H, n, dW1, mode=1, colsum=db1, pro=HT_PRO_TANH_BWD, pro_a=t),
              ht_job(dt, D, 1, W1, H, 1, n, H, D, dE, pro=HT_PRO_TANH_BWD, pro_a=t))


def single_step_finish(states, flag, scaler_f, scaler_i, growth=2.0, backoff=0.5, growth_interval=2000):
    """End of a single-adapter train_step under the dynamic loss scale (include/feddat_hip.h: feddat_single_step_finish)."""
    n = len(states)
    _dev(*states, flag, scaler_f, scaler_i)
    sp = (vp * n)(*[s.data_ptr() for s in states])
    _chk(load().feddat_single_step_finish(sp, n, _p(flag), _p(scaler_f), _p(scaler_i), growth, backoff, growth_interval,
                                          _stream()), "feddat_single_step_finish")


def adamw_group(p, g, m, v, seg_off, seg_wd, state, d_sched=0, d_adam=0, skip_if=(), bak=None, bak_mode=0,
                restore_if=None) -> AdamwGroup:
    """skip_if: up to two int32 device tensors (the update is skipped when either is non-zero); bak / bak_mode / restore_if: the
    save (1) / conditional restore (2) of p | m | v around an update that may have to be undone (feddat_adamw_group, ABI 8)."""
    _dev(p, g, m, v, seg_off, seg_wd, state)
    G = AdamwGroup()
    G._keep = (p, g, m, v, seg_off, seg_wd, state, tuple(skip_if), bak, restore_if)
    for k, t in enumerate(skip_if):
        G.skip_if[k] = t.data_ptr()
    if bak is not None:
        assert bak.numel() >= 3 * p.numel() and bak_mode in (1, 2)
        G.bak, G.bak_mode = bak.data_ptr(), bak_mode
    if restore_if is not None:
        G.restore_if = restore_if.data_ptr()
    G.p, G.g, G.m, G.v, G.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
    G.seg_off, G.seg_wd, G.nseg, G.state, G.d_sched, G.d_adam = (seg_off.data_ptr(), seg_wd.data_ptr(), seg_wd.numel(),
                                                                   state.data_ptr(), d_sched, d_adam)
    return G


def adamw_multi(groups, lr, warmup, total, beta1, beta2, eps):
    arr = (AdamwGroup * len(groups))(*groups)
    arr._keep = groups
    _chk(load().feddat_adamw_multi(arr, len(groups), lr, warmup, total, beta1, beta2, eps, _stream()), "feddat_adamw_multi")


def step_tick_multi(states, d_sched, d_adam):
    n = len(states)
    _dev(*states)
    sp = (vp * n)(*[s.data_ptr() for s in states])
    _chk(load().feddat_step_tick_multi(sp, (i32 * n)(*d_sched), (i32 * n)(*d_adam), n, _stream()), "feddat_step_tick_multi")


def vqa_score_accumulate(logits, target, acc):
    """acc[0] += sum_b target[b, argmax logits[b]], acc[1] += B (device; train_vqa_crossvqa.py:241-257)."""
    _dev(logits, target, acc)
    assert logits.shape == target.shape and logits.is_contiguous() and target.is_contiguous() and acc.numel() >= 2
    _chk(load().feddat_vqa_score_accumulate(_p(logits), _p(target), logits.shape[0], logits.shape[1], _p(acc), _stream()),
         "feddat_vqa_score_accumulate")


def lm_loss_fwd_bwd(logits, teacher, labels, row_weight, V, temp, kl_scale, dlogits_bf16, scalars, row_kl=None, grad_scale=1.0,
                    grad_scale_dev=None, nonfinite=None):
    """grad_scale_dev / nonfinite (device float / int32 tensors): the dynamic loss scale and its overflow flag (ABI 8)."""
    _dev(logits, teacher, labels, row_weight, dlogits_bf16, scalars, row_kl, grad_scale_dev, nonfinite)
    R = logits.shape[0]
    assert scalars.numel() >= 4 + 2 * R and labels.dtype == torch.int64
    if grad_scale_dev is not None or nonfinite is not None:
        _chk(load().feddat_lm_loss_fwd_bwd_dyn(_p(logits), _p(teacher), logits.stride(0), _p(labels), _p(row_weight), _p(row_kl), R, V,
                                               temp, kl_scale, float(grad_scale), _p(grad_scale_dev), _p(nonfinite), _p(dlogits_bf16),
                                               0 if dlogits_bf16 is None else dlogits_bf16.stride(0), _p(scalars), _stream()),
             "feddat_lm_loss_fwd_bwd_dyn")
        return
    _chk(load().feddat_lm_loss_fwd_bwd(_p(logits), _p(teacher), logits.stride(0), _p(labels), _p(row_weight), _p(row_kl), R, V, temp,
                                       kl_scale, float(grad_scale), _p(dlogits_bf16), 0 if dlogits_bf16 is None else dlogits_bf16.stride(0),
                                       _p(scalars), _stream()), "feddat_lm_loss_fwd_bwd")


def lm_ce_loss_fwd_bwd(logits, labels, row_weight, V, dlogits_bf16, scalars, grad_scale=1.0, grad_scale_dev=None, nonfinite=None):
    """L = sum_r row_weight[r] ce_r, the LM loss without a teacher (include/feddat_hip_albef.h): scalars[0] = scalars[2] = L,
    dlogits = grad_scale * (*grad_scale_dev) * dL/dlogits in the operand format."""
    _dev(logits, labels, row_weight, dlogits_bf16, scalars, grad_scale_dev, nonfinite)
    R = logits.shape[0]
    assert scalars.numel() >= 4 + 2 * R and labels.dtype == torch.int64 and labels.numel() >= R and row_weight.numel() >= R
    assert dlogits_bf16 is None or dlogits_bf16.shape[0] >= R
    _chk(_ext("feddat_lm_ce_loss_fwd_bwd")(_p(logits), logits.stride(0), _p(labels), _p(row_weight), R, V, float(grad_scale),
                                           _p(grad_scale_dev), _p(nonfinite), _p(dlogits_bf16),
                                           0 if dlogits_bf16 is None else dlogits_bf16.stride(0), _p(scalars), _stream()),
         "feddat_lm_ce_loss_fwd_bwd")


def vilt_stage_inputs(input_ids, token_type_ids, attention_mask, target, pixel_mask, dst: dict, B, Lt, n_labels, Hi, Wi, P):
    """The step's small inputs -> the engine's static buffers (dst: input_ids, token_type_ids, attention_mask, target,
    patch_mask) in one launch.  All sources on the device, int64 / fp32, contiguous."""
    _dev(input_ids, token_type_ids, attention_mask, target, pixel_mask)
    _chk(load().feddat_vilt_stage_inputs(_p(input_ids), _p(token_type_ids), _p(attention_mask), _p(target), _p(pixel_mask),
                                         _p(dst["input_ids"]), _p(dst["token_type_ids"]), _p(dst["attention_mask"]),
                                         _p(dst["target"]), _p(dst["patch_mask"]), B, Lt, n_labels, Hi, Wi, P, _stream()),
         "feddat_vilt_stage_inputs")


def vilt_pad_batch_rc(patches, inp: dict, n: int, B: int) -> int:
    """feddat_vilt_pad_batch on an engine's static inputs (patches: 16-bit [B * np, 3 P P]; inp: input_ids, token_type_ids,
    attention_mask, patch_mask, target): samples [n, B) become copies of samples j mod n.  Returns the C return code."""
    _dev(patches, *(inp[k] for k in ("input_ids", "token_type_ids", "attention_mask", "patch_mask", "target")))
    assert patches.element_size() == 2 and patches.is_contiguous() and patches.shape[0] % B == 0
    assert inp["target"].dtype == torch.float32 and all(
        inp[k].dtype == torch.int64 and inp[k].is_contiguous() for k in ("input_ids", "token_type_ids", "attention_mask",
                                                                         "patch_mask"))
    n_patches = patches.shape[0] // B
    assert inp["patch_mask"][:B].numel() == B * n_patches
    return int(load().feddat_vilt_pad_batch(_p(patches), _p(inp["input_ids"]), _p(inp["token_type_ids"]),
                                            _p(inp["attention_mask"]), _p(inp["patch_mask"]), _p(inp["target"]), int(n), int(B),
                                            n_patches, patches.shape[1], inp["input_ids"].shape[1], inp["target"].shape[1],
                                            _stream()))


def vilt_pad_batch(patches, inp: dict, n: int, B: int):
    _chk(vilt_pad_batch_rc(patches, inp, n, B), "feddat_vilt_pad_batch")


def softmax_gather_rows(logits, rows, row_stride, V, ids, out):
    """out[r, j] = softmax(logits.flatten()[r * row_stride : r * row_stride + V])[ids[j]]; ids int64 (any 1-D stride)."""
    _dev(logits, ids, out)
    assert logits.dtype == torch.float32 and ids.dtype == torch.int64 and out.dtype == torch.float32 and out.is_contiguous()
    n = ids.shape[0]
    assert out.shape == (rows, n)
    _chk(load().feddat_softmax_gather_rows(_p(logits), row_stride, rows, V, _p(ids), ids.stride(0), n, _p(out), _stream()),
         "feddat_softmax_gather_rows")


def topk_rows(vals, k, *, minus=None, log_first=False, softmax=False):
    """-> (values [rows, k] fp32, indices [rows, k] int64), descending; ties: lower index first."""
    _dev(vals, minus)
    rows, n = vals.shape
    assert vals.dtype == torch.float32 and vals.stride(1) == 1 and (minus is None or (minus.is_contiguous() and minus.shape == vals.shape))
    ov = torch.empty(rows, k, dtype=torch.float32, device=vals.device)
    oi = torch.empty(rows, k, dtype=torch.int64, device=vals.device)
    _chk(load().feddat_topk_rows(_p(vals), vals.stride(0), _p(minus), rows, n, k, (1 if log_first else 0) | (2 if softmax else 0),
                                 _p(ov), _p(oi), _stream()), "feddat_topk_rows")
    return ov, oi


def albef_pad_questions(image, question_ids, question_mask, nq: int):
    """feddat_albef_pad_questions on an ALBEF engine's static inputs (image fp32 [B, 3, R, R]; question_ids / question_mask int64
    [B, Lq]): samples [nq, B) become copies of samples j mod nq."""
    _dev(image, question_ids, question_mask)
    B, Lq = question_ids.shape
    assert image.dtype == torch.float32 and image.is_contiguous() and image.shape[0] == B
    assert all(t.dtype == torch.int64 and t.is_contiguous() and tuple(t.shape) == (B, Lq) for t in (question_ids, question_mask))
    _chk(load().feddat_albef_pad_questions(_p(image), _p(question_ids), _p(question_mask), int(nq), B, image[0].numel(), Lq,
                                           _stream()), "feddat_albef_pad_questions")


def rank_slab_gather(topk_ids, list_ids, list_mask, answer_ids, answer_mask, answer_mask8, labels, row_w, B: int, slab: int,
                     pad_id: int):
    """feddat_rank_slab_gather: slab `slab` of the shortlist topk_ids [nq, k] (device int64) -> the [N, La] answer frame, its
    labels and per-row weights."""
    _dev(topk_ids, list_ids, list_mask, answer_ids, answer_mask, answer_mask8, labels, row_w)
    (nq, k), (M, la), (N, La) = topk_ids.shape, list_ids.shape, answer_ids.shape
    assert all(t.dtype == torch.int64 and t.is_contiguous() for t in (topk_ids, list_ids, list_mask, answer_ids, answer_mask, labels))
    assert tuple(list_mask.shape) == (M, la) and tuple(answer_mask.shape) == (N, La)
    assert answer_mask8 is None or (answer_mask8.dtype == torch.uint8 and answer_mask8.is_contiguous() and tuple(answer_mask8.shape) == (N, La))
    assert labels.numel() == N * (La - 1) and row_w.dtype == torch.float32 and row_w.is_contiguous() and row_w.numel() == N * (La - 1)
    _chk(load().feddat_rank_slab_gather(_p(topk_ids), _p(list_ids), _p(list_mask), _p(answer_ids), _p(answer_mask), _p(answer_mask8),
                                        _p(labels), _p(row_w), nq, k, M, la, int(B), N, La, int(slab), int(pad_id), _stream()),
         "feddat_rank_slab_gather")


def rank_slab_loss(scalars, answer_loss, nq: int, k: int, B: int, N: int, La: int, slab: int):
    """feddat_rank_slab_loss: answer_loss[slab * N + i] = the sum of candidate i's La - 1 CE terms in `scalars` (what
    lm_loss_fwd_bwd wrote for the slab's logits)."""
    _dev(scalars, answer_loss)
    assert scalars.dtype == torch.float32 and scalars.is_contiguous() and scalars.numel() >= 4 + 2 * N * (La - 1)
    assert answer_loss.dtype == torch.float32 and answer_loss.is_contiguous() and answer_loss.numel() == nq * k
    _chk(load().feddat_rank_slab_loss(_p(scalars), _p(answer_loss), int(nq), int(k), int(B), int(N), int(La), int(slab), _stream()),
         "feddat_rank_slab_loss")


def lm_head_refresh(w, bias, w16, wT16, bias_pad):
    """feddat_lm_head_refresh: the trainable LM head's fp32 master tensors (w = transform.dense.weight [H, H], bias =
    predictions.bias [V], views of a flat group) -> the step's operands in one launch: w16 / wT16 [H, H] in the bound library's
    operand format (the bits of cvt_f32_bf16 / transpose_f32_bf16) and bias_pad [Vp] = bias followed by zeros."""
    _dev(w, bias, w16, wT16, bias_pad)
    H = w.shape[0]
    fmt = OPERAND_DTYPE[current_operands()]
    if not (w.dim() == 2 and w.shape[1] == H and w.dtype == torch.float32 and w.is_contiguous() and bias.dim() == 1
            and bias.dtype == torch.float32 and bias.is_contiguous() and bias_pad.dtype == torch.float32
            and bias_pad.is_contiguous() and bias_pad.dim() == 1 and bias_pad.numel() >= bias.numel()):
        raise FeddatHipError("lm_head_refresh: w fp32 [H, H], bias fp32 [V], bias_pad fp32 [Vp >= V], all contiguous")
    for t in (w16, wT16):
        if not (t.dtype == fmt and tuple(t.shape) == (H, H) and t.is_contiguous()):
            raise FeddatHipError(f"lm_head_refresh: w16 / wT16 must be contiguous [{H}, {H}] tensors of {fmt}")
    _chk(load().feddat_lm_head_refresh(_p(w), _p(bias), H, bias.numel(), bias_pad.numel(), _p(w16), _p(wT16), _p(bias_pad),
                                       _stream()), "feddat_lm_head_refresh")


def dropout(x, drop, *, resid=None, out_f32=None, out_bf16=None):
    """out = mask(idx) x / (1 - p) (+ resid); x fp32 or bf16; drop = (p, key0, key1, step_counter)."""
    _dev(x, resid, out_f32, out_bf16)
    x32, x16 = (x, None) if x.dtype == torch.float32 else (None, x)
    _chk(load().feddat_dropout(_p(x32), _p(x16), _p(resid), _p(out_f32), _p(out_bf16), x.numel(), drop[0], drop[1], drop[2],
                               _p(drop[3]), _stream()), "feddat_dropout")


def dropout_keys(seed: int, pass_id: int, site: int):
    """(key0, key1) of one dropout site: splitmix64 of (seed, pass, site) split in two 32-bit halves (include/feddat_hip.h)."""
    M = (1 << 64) - 1
    z = (seed * 0x9E3779B97F4A7C15 + pass_id * 0xBF58476D1CE4E5B9 + site * 0x94D049BB133111EB + 0x2545F4914F6CDD1D) & M
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M
    z ^= z >> 31
    return z & 0xFFFFFFFF, z >> 32


def axpby3(a, alpha, b=None, beta=0.0, c=None, gamma=0.0, *, out_f32=None, out_bf16=None):
    _dev(a, b, c, out_f32, out_bf16)
    _chk(load().feddat_axpby3(_p(a), alpha, _p(b), beta, _p(c), gamma, _p(out_f32), _p(out_bf16), a.numel(), _stream()),
         "feddat_axpby3")


def gather_rows(src, idx, dst_f32=None, dst_bf16=None):
    _dev(src, idx, dst_f32, dst_bf16)
    assert idx.dtype == torch.int32
    _chk(load().feddat_gather_rows(_p(src), _p(idx), _p(dst_f32), _p(dst_bf16), idx.numel(), src.shape[-1], _stream()),
         "feddat_gather_rows")


def segment_sum_rows(src, seg_offsets, dst, accumulate=False):
    _dev(src, seg_offsets, dst)
    assert seg_offsets.dtype == torch.int32
    _chk(load().feddat_segment_sum_rows(_p(src), _p(seg_offsets), _p(dst), seg_offsets.numel() - 1, src.shape[-1],
                                        int(accumulate), _stream()), "feddat_segment_sum_rows")


def adamw_flat(p, g, m, v, seg_off, seg_wd, state, base_lr, warmup, total, beta1=0.9, beta2=0.98, eps=1e-8):
    _dev(p, g, m, v)
    _chk(load().feddat_adamw_flat(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(seg_off), _p(seg_wd), seg_wd.numel(),
                                  _p(state), base_lr, warmup, total, beta1, beta2, eps, _stream()),
         "feddat_adamw_flat")


def step_tick(state, d_sched, d_adam):
    _chk(load().feddat_step_tick(_p(state), d_sched, d_adam, _stream()), "feddat_step_tick")


def text_embed(ids, tts, word, pos, typ, ln_g, ln_b, eps, mod0, h, B, Lt, S, H):
    _dev(ids, h)
    _chk(load().feddat_text_embed(_p(ids), _p(tts), _p(word), _p(pos), _p(typ), _p(ln_g), _p(ln_b), eps, _p(mod0),
                                  _p(h), B, Lt, S, H, _stream()), "feddat_text_embed")


def _host_i32(a, n=None):
    import numpy as np
    a = np.ascontiguousarray(a, dtype=np.int32)
    if a.ndim != 1 or (n is not None and a.shape[0] != n):
        raise FeddatHipError("image sizes are host int arrays of one entry per image")
    return a


def _host_i64(a, n):
    import numpy as np
    a = np.ascontiguousarray(a, dtype=np.int64)
    if a.ndim != 1 or a.shape[0] != n:
        raise FeddatHipError("image offsets are host int64 arrays of one entry per image")
    return a


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _image_workspace(workspace, need: int, device, what: str):
    if need < 0:
        raise FeddatHipError(f"{what} rejected the image sizes")
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    _dev(workspace)
    return workspace


def image_resample_u8(images, offsets, heights, widths, out_h, out_w, out, out_offsets, filter=FILTER_BILINEAR, workspace=None):
    """feddat_image_resample_u8: image i, packed uint8 [h][w][3] at byte offsets[i] of the device buffer `images`, is resampled with
    Pillow's bilinear / bicubic (FILTER_*) to [out_h][out_w][3] at byte out_offsets[i] of the device buffer `out` (which may be
    `images` itself where no result overlaps a source).  Sizes and offsets are host arrays.  Every image must lie inside its
    buffer: checked here, the kernels trust the offsets.  -> the workspace used (hand it back in to reuse it)."""
    _dev(images, out)
    if images.dtype != torch.uint8 or out.dtype != torch.uint8 or not images.is_contiguous() or not out.is_contiguous():
        raise FeddatHipError("image_resample_u8 takes contiguous uint8 device buffers")
    h = _host_i32(heights)
    n = h.shape[0]
    w, oh, ow = _host_i32(widths, n), _host_i32(out_h, n), _host_i32(out_w, n)
    so, do = _host_i64(offsets, n), _host_i64(out_offsets, n)
    if n < 1 or min(h.min(), w.min(), oh.min(), ow.min()) < 1 or so.min() < 0 or do.min() < 0:
        raise FeddatHipError("image_resample_u8: sizes must be >= 1 and offsets >= 0")
    if int((so + h.astype("int64") * w * 3).max()) > images.numel() or int((do + oh.astype("int64") * ow * 3).max()) > out.numel():
        raise FeddatHipError("image_resample_u8: an image reaches past the end of its buffer")
    need = int(load().feddat_image_resample_workspace_bytes(_hp(h), _hp(w), _hp(oh), _hp(ow), n, int(filter)))
    workspace = _image_workspace(workspace, need, images.device, "feddat_image_resample_workspace_bytes")
    _chk(load().feddat_image_resample_u8(_p(images), _hp(so), _hp(h), _hp(w), _hp(oh), _hp(ow), _hp(do), n, int(filter), _p(out),
                                         _p(workspace), workspace.numel(), _stream()), "feddat_image_resample_u8")
    return workspace


def albef_image_preprocess(images, offsets, heights, widths, out, mean, std, workspace=None):
    """feddat_albef_image_preprocess: n packed uint8 images (as image_resample_u8) -> out fp32 [n, 3, R, R] (contiguous; may be
    a slice of a larger buffer): bicubic to R x R, x / 255, (x - mean) / std in float32.  -> the workspace used."""
    import numpy as np
    _dev(images, out)
    if images.dtype != torch.uint8 or not images.is_contiguous():
        raise FeddatHipError("albef_image_preprocess takes a contiguous uint8 device buffer")
    h = _host_i32(heights)
    n = h.shape[0]
    w, so = _host_i32(widths, n), _host_i64(offsets, n)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 4 or out.shape[0] != n or out.shape[1] != 3 \
            or out.shape[2] != out.shape[3]:
        raise FeddatHipError(f"albef_image_preprocess writes a contiguous fp32 [n, 3, R, R] tensor of n = {n} images, got "
                             f"{tuple(out.shape)} {out.dtype}")
    if n < 1 or min(h.min(), w.min()) < 1 or so.min() < 0 or int((so + h.astype("int64") * w * 3).max()) > images.numel():
        raise FeddatHipError("albef_image_preprocess: an image is empty or reaches past the end of its buffer")
    R = int(out.shape[2])
    m, s = np.ascontiguousarray(mean, dtype=np.float32), np.ascontiguousarray(std, dtype=np.float32)
    if m.shape != (3,) or s.shape != (3,):
        raise FeddatHipError("mean and std hold one value per RGB channel")
    need = int(load().feddat_albef_image_workspace_bytes(_hp(h), _hp(w), n, R))
    workspace = _image_workspace(workspace, need, images.device, "feddat_albef_image_workspace_bytes")
    _chk(load().feddat_albef_image_preprocess(_p(images), _hp(so), _hp(h), _hp(w), n, R, _hp(m), _hp(s), _p(out), _p(workspace),
                                              workspace.numel(), _stream()), "feddat_albef_image_preprocess")
    return workspace


def image_embed_assemble_masked(proj, cls, pos0, pos_grid, patch_mask, attention_mask, mod1, h, key_mask, B, Lt, gh, gw, g, H,
                                nrep=1):
    """image_embed_assemble + pos_embed_resize_masked + vilt_key_mask in one launch (patch_mask: int64 [B, gh, gw])."""
    _dev(proj, h, patch_mask)
    _chk(load().feddat_image_embed_assemble_masked(_p(proj), _p(cls), _p(pos0), _p(pos_grid), _p(patch_mask),
                                                   _p(attention_mask), _p(mod1), _p(h), _p(key_mask), B, Lt, gh, gw, g, H, nrep,
                                                   _stream()), "feddat_image_embed_assemble_masked")


def im2col_patches(pixels, patches, B, Cc, Hi, Wi, P):
    _dev(pixels, patches)
    _chk(load().feddat_im2col_patches(_p(pixels), _p(patches), B, Cc, Hi, Wi, P, _stream()), "feddat_im2col_patches")


def im2col_patches_slots(pixels, patch_mask, patches, n, B, Cc, Hi, Wi, P, max_patches):
    """Patch slots: pixels fp32 [n, Cc, Hi, Wi] -> patches 16-bit [B * max_patches, Cc P P], slot j of sample b = cell
    (j / vw, j % vw) of its valid rectangle (patch_mask: int64 [B, Hi/P, Wi/P]), read from sample b mod n; empty slots zero."""
    _dev(pixels, patch_mask, patches)
    if patch_mask.dtype != torch.int64 or pixels.dtype != torch.float32:
        raise FeddatHipError("im2col_patches_slots takes fp32 pixels and an int64 patch mask")
    _chk(load().feddat_im2col_patches_slots(_p(pixels), _p(patch_mask), _p(patches), n, B, Cc, Hi, Wi, P, max_patches,
                                            _stream()), "feddat_im2col_patches_slots")


def image_embed_assemble_slots(proj, cls, pos0, pos_grid, patch_mask, attention_mask, mod1, h, key_mask, overflow, B, Lt, gh, gw,
                               max_patches, g, H, nrep=1):
    """image_embed_assemble_masked on patch slots (proj: [B * max_patches, H]; h: [B, Lt + 1 + max_patches, H]); overflow:
    int32 [1], set to 1 when a sample has more valid patches than slots."""
    _dev(proj, h, patch_mask)
    if patch_mask.dtype != torch.int64 or (overflow is not None and overflow.dtype != torch.int32):
        raise FeddatHipError("image_embed_assemble_slots takes an int64 patch mask and an int32 overflow flag")
    _chk(load().feddat_image_embed_assemble_slots(_p(proj), _p(cls), _p(pos0), _p(pos_grid), _p(patch_mask), _p(attention_mask),
                                                  _p(mod1), _p(h), _p(key_mask), _p(overflow), B, Lt, gh, gw, max_patches, g, H,
                                                  nrep, _stream()), "feddat_image_embed_assemble_slots")


def image_embed_assemble(proj, cls, pos0, pos_img, mod1, h, B, Lt, npatch, S, H, pos_batch_stride=0):
    _dev(proj, h)
    _chk(load().feddat_image_embed_assemble(_p(proj), _p(cls), _p(pos0), _p(pos_img), pos_batch_stride, _p(mod1), _p(h),
                                            B, Lt, npatch, S, H, _stream()), "feddat_image_embed_assemble")


def pos_embed_resize_masked(grid, pixel_mask, out, g, B, Hi, Wi, P, H):
    _dev(grid, pixel_mask, out)
    if pixel_mask.dtype != torch.int64:
        raise FeddatHipError("pixel_mask must be int64 (HF processor output)")
    _chk(load().feddat_pos_embed_resize_masked(_p(grid), _p(pixel_mask), _p(out), g, B, Hi, Wi, P, H, _stream()),
         "feddat_pos_embed_resize_masked")


def vilt_key_mask(attention_mask, pixel_mask, key_mask, B, Lt, Hi, Wi, P, nrep=1):
    _dev(key_mask)
    for m in (attention_mask, pixel_mask):
        if m is not None and (m.dtype != torch.int64 or not m.is_cuda):
            raise FeddatHipError("masks must be int64 device tensors (HF processor output)")
    _chk(load().feddat_vilt_key_mask(_p(attention_mask), _p(pixel_mask), _p(key_mask), B, Lt, Hi, Wi, P, nrep,
                                     _stream()), "feddat_vilt_key_mask")


def pos_embed_resize(grid, out, g, gh, gw, H):
    _dev(grid, out)
    _chk(load().feddat_pos_embed_resize(_p(grid), _p(out), g, gh, gw, H, _stream()), "feddat_pos_embed_resize")


def cvt_f32_bf16(x, out):
    _dev(x, out)
    _chk(load().feddat_cvt_f32_bf16(_p(x), _p(out), x.numel(), _stream()), "feddat_cvt_f32_bf16")


def transpose_f32_bf16(x, out, R, Cc):
    _dev(x, out)
    _chk(load().feddat_transpose_f32_bf16(_p(x), _p(out), R, Cc, _stream()), "feddat_transpose_f32_bf16")


def tanh_fwd(x):
    _dev(x)
    _chk(load().feddat_tanh_fwd(_p(x), x.numel(), _stream()), "feddat_tanh_fwd")


def tanh_bwd(y, dy, dx):
    _dev(y, dy, dx)
    _chk(load().feddat_tanh_bwd(_p(y), _p(dy), _p(dx), y.numel(), _stream()), "feddat_tanh_bwd")


def gelu_fwd(x, y):
    _dev(x, y)
    _chk(load().feddat_gelu_fwd(_p(x), _p(y), x.numel(), _stream()), "feddat_gelu_fwd")


def gelu_bwd(x, dy, dx):
    _dev(x, dy, dx)
    _chk(load().feddat_gelu_bwd(_p(x), _p(dy), _p(dx), x.numel(), _stream()), "feddat_gelu_bwd")


def scatter_cls_rows(rows, out_f32, out_bf16, B, S, H):
    _dev(rows)
    _chk(load().feddat_scatter_cls_rows(_p(rows), _p(out_f32), _p(out_bf16), B, S, H, _stream()),
         "feddat_scatter_cls_rows")


def fedavg_accumulate(acc, x, num, total, first):
    _dev(acc, x)
    _chk(load().feddat_fedavg_accumulate(_p(acc), _p(x), acc.numel(), float(num), float(total), int(first),
                                         _stream()), "feddat_fedavg_accumulate")


def probe_tr16(inp, out):
    _dev(inp, out)
    _chk(load().feddat_probe_tr16(_p(inp), _p(out), _stream()), "feddat_probe_tr16")
