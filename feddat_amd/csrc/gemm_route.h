// Routing of the K1 GEMM entry points (gemm_bf16.hip): which kernel family, tile height, XCD split, grid and LDS size a launch
// gets.  Plain C++ without HIP and without globals -- a pure function of its arguments (the entry points pass the device's CU
// count and the selection flags in), so it can be called and pinned on a machine without a GPU: feddat_gemm_route,
// tests/test_gemm_route_cpu.py.  Every family and tile height accumulates in the same order (bit-identical results), so a
// routing mistake only costs time; that test is what reports it.
#pragma once
#include <stddef.h>

#include "../../include/feddat_hip.h"

typedef feddat_gemm_route_t GemmRoute;

// Dynamic LDS bytes of a family at a tile height (gemm_bf16.hip asserts them against its V2Cfg / V3Cfg): the persistent kernels
// hold two stages of (rows + 192) 128-byte k-tile rows and 5 KiB of epilogue staging per wave (8 waves: two-group kernel, 4: one
// wave per SIMD; the dual form stages inside the k-tile stage it has just consumed: 80 KiB, two workgroups fill a CU's 160 KiB)
constexpr int fd_gemm_lds(int family, int rows) {
    return family == FEDDAT_GEMM_V1    ? 4 * 128 * 128
           : family == FEDDAT_GEMM_MID ? 4 * 64 * 128
                                       : 2 * (rows + 192) * 128 + (family == FEDDAT_GEMM_V2 ? 8 : family == FEDDAT_GEMM_V3 ? 4 : 0) * 5120;
}

// Balanced M tiles of <= `rows` rows for N / 192 tile columns, and the XCD-aware tile order: the XCDs are split over N as well
// (nx = 2: 4 M groups of equal size x 2 N halves) when B (N x K elements of `esize` bytes) would not stay in a 4 MiB L2 and the
// launch takes more than one round of tiles.  Returns the rounds of the persistent grid.
inline int fd_gemm_plan(int M, int N, int K, int esize, int n_cu, int rows, GemmRoute& o) {
    const int tiles_n = N / 192;
    int nmt = (M + rows - 1) / rows;
    o.nx = 1;
    if ((size_t)N * K * esize > (3u << 20) && tiles_n % 2 == 0 && nmt * tiles_n > n_cu) {
        o.nx = 2;
        nmt = (nmt + 3) & ~3;
    }
    o.rows = rows;
    o.bm = (M + nmt - 1) / nmt;
    o.tiles_m = o.nx == 1 ? (M + o.bm - 1) / o.bm : nmt;
    o.tm_per = o.tiles_m / (8 / o.nx);
    o.tn_per = tiles_n / o.nx;
    return (o.tiles_m * tiles_n + n_cu - 1) / n_cu;
}

// the planned route `r` on a persistent family: one workgroup per tile up to `blocks` resident workgroups
inline int fd_gemm_route_persistent(GemmRoute& r, int family, int N, int blocks, int extra_lds = 0) {
    const int total = r.tiles_m * (N / 192);
    r.family = family;
    r.threads = family == FEDDAT_GEMM_V2 ? 512 : 256;
    r.lds_bytes = fd_gemm_lds(family, r.rows) + extra_lds;
    r.grid = total < blocks ? total : blocks;
    return FEDDAT_OK;
}

// M, N, K in elements of the caller's operand type; kind: FEDDAT_GEMM_OP16 / _FP8 / _FP8MX; flags: the kernel-selection bits
// of feddat_set_debug_flags.  FEDDAT_EINVAL for a shape or epilogue no kernel takes.
inline int fd_gemm_route(int M, int N, int K, int epi, int kind, int n_cu, int flags, GemmRoute& r) {
    r = GemmRoute{};
    if (M <= 0 || N <= 0 || K <= 0 || n_cu <= 0) return FEDDAT_EINVAL;
    if (kind != FEDDAT_GEMM_OP16) {
        // fp8 operands: the two-group persistent kernel only; . gelu'(bf16 u) and the dequantising + residual epilogue stay on
        // 192-row tiles (their 256-row instantiations spill); MX: + the scale stages
        const bool mx = kind == FEDDAT_GEMM_FP8MX;
        if ((kind != FEDDAT_GEMM_FP8 && !mx) || M < 1024 || N % 192 || K % 128 || epi < 0 || epi > FEDDAT_EPI_MUL_G8_F8 ||
            (mx && epi != FEDDAT_EPI_BF16))
            return FEDDAT_EINVAL;
        GemmRoute r4 = r;
        const int rounds3 = fd_gemm_plan(M, N, K, 1, n_cu, 192, r), rounds4 = fd_gemm_plan(M, N, K, 1, n_cu, 256, r4);
        if (rounds4 * 12 < rounds3 * 10 && epi != FEDDAT_EPI_MUL_DGELU && epi != FEDDAT_EPI_RESID_F32) r = r4;
        return fd_gemm_route_persistent(r, FEDDAT_GEMM_V2, N, n_cu, mx ? 2 * 256 * (r.rows / 64) : 0);
    }
    if (epi < 0 || epi > FEDDAT_EPI_MUL_G8 || K % 64) return FEDDAT_EINVAL;
    const bool g8 = epi == FEDDAT_EPI_GELU_G8 || epi == FEDDAT_EPI_MUL_G8;      // persistent kernels only
    // Medium M (ALBEF's stacked text streams: 2 x 800 rows): the persistent kernels would put 1600 x 768 on 9 x 4 = 36 tiles, i.e.
    // 36 of the 256 CUs; the small-tile kernel fills the chip with 64 x 64 tiles (same k order: bit-identical results).  Taken
    // when a launch has fewer 192-row tiles than 0.6 x the CUs (all of them, whatever bits 28..31 say); not for the gelu' code
    // epilogues; flag 1 (everything on the two-group persistent kernel) keeps the old routing (A/B: tools/albef_stack_ab.py);
    // flag 128 = "no small-tile kernel": such launches stay persistent instead of falling through to the 128 x 128 kernel,
    // which needs N % 128 == 0 -- N = 192 x odd would lose its tail columns there
    const bool big = N % 192 == 0 && M >= 1024;
    const bool small_grid = big && M < 4096 && !g8 && !(flags & (1 | 128)) && ((M + 191) / 192) * (N / 192) * 10 < n_cu * 6;
    if (!big || small_grid) {
        const bool v1_ok = N % 128 == 0;
        const int tiles1 = ((M + 127) / 128) * (N / 128);
        if (g8) return FEDDAT_EINVAL;
        // few rows and too few 128 x 128 tiles to fill the chip: the latency-oriented small-tile kernel
        const bool mid = (M < 1024 || small_grid) && N % 64 == 0 && (!v1_ok || tiles1 < 150) && !(flags & 128);
        if (!mid && !v1_ok) return FEDDAT_EINVAL;      // the 128 x 128 kernel has no column tail
        r.family = mid ? FEDDAT_GEMM_MID : FEDDAT_GEMM_V1;
        r.rows = mid ? 64 : 128;
        r.threads = 256;
        r.lds_bytes = fd_gemm_lds(r.family, r.rows);
        r.grid = mid ? ((M + 63) / 64) * (N / 64) : tiles1;
        return FEDDAT_OK;
    }
    // tools/overlap_probe.py: bits 28..31 of the flags cap the persistent grid at 16 x value workgroups, so that a launch on a
    // side stream leaves compute units to the kernels of the main stream
    if (const int cap16 = (flags >> 28) & 0xf) n_cu = n_cu < cap16 * 16 ? n_cu : cap16 * 16;
    r.dbg = flags;
    // The DUAL form (flags 1 | 2 together: every persistent launch; 1 | 2 | 64: only launches of at least two full rounds of the
    // doubled grid, e.g. N = 3072 at M = 11 840: 96 x 16 tiles = 3.0 rounds of 512): two independent 128-row workgroups per CU.
    // Measured, not the default: profiles/r06_gemm_dual_ab.txt, DESIGN.md section 7e.
    if ((flags & 3) == 3) {
        if (K / 64 >= 3) {      // (its self-contained tiles need a first, a penultimate and a last k-tile)
            fd_gemm_plan(M, N, K, 2, 2 * n_cu, 128, r);
            if (!(flags & 64) || r.tiles_m * (N / 192) >= 4 * n_cu) return fd_gemm_route_persistent(r, FEDDAT_GEMM_DUAL, N, 2 * n_cu);
        }
        flags &= ~3;      // not taken: the production routing below
        r.dbg = flags;
    }
    if (g8 && (flags & (2 | 512))) return FEDDAT_EINVAL;      // the code epilogues exist on the two-group (and the dual) kernel only
    GemmRoute r4 = r, r5 = r, r7 = r;
    const int rounds3 = fd_gemm_plan(M, N, K, 2, n_cu, 192, r), rounds4 = fd_gemm_plan(M, N, K, 2, n_cu, 256, r4);
    const int rounds5 = fd_gemm_plan(M, N, K, 2, n_cu, 160, r5), rounds7 = fd_gemm_plan(M, N, K, 2, n_cu, 224, r7);
    // a 256-row tile costs about 1.2x a 192-row tile (48 vs 36 MFMAs per k-tile and wave, L phase 20 vs 18 reads); the 256-row
    // instantiation of . gelu'(bf16 u) spills (180 B of scratch per lane and tile); flags 32 / 64 force 192 / 256 rows
    const bool rows256 = (flags & 64) || (!(flags & 32) && epi != FEDDAT_EPI_MUL_DGELU && rounds4 * 12 < rounds3 * 10);
    // v3 (one wave per SIMD) has the faster k-loop (1.1-1.28 PF/s against 0.96-1.15) but only four waves to run an epilogue: it
    // takes every launch except the heavy epilogues (GELU with two outputs; . gelu'(aux) with its cold aux operand; the codes) --
    // in isolation v3 is level or ahead on those too (84 against 98 us for . gelu'), in the step, with nothing cache-warm, it
    // is behind (86 / 89 us against 82 / 81: tools/step_breakdown.py --detail); flag 1 keeps everything on v2, flag 2 forces v3
    const bool v3_pick = epi != FEDDAT_EPI_GELU && epi != FEDDAT_EPI_MUL_DGELU && !g8;
    if (!((flags & 2) || v3_pick) || (flags & 1)) {
        if (rows256) r = r4;
        return fd_gemm_route_persistent(r, FEDDAT_GEMM_V2, N, n_cu);
    }
    // 160-row tiles (~0.87 of a 192-row tile's time) where they fill the rounds better: 18 464 rows x N = 768 (ALBEF's ViT) = 388
    // tiles of 192 rows = 1.52 rounds of the 256 CUs, paid as 2; 464 tiles of 160 rows = 1.81 rounds, paid as 2 x 0.87.
    // configs[1]'s 11 840 rows (64 x 185) keep their exact rounds of 192-row tiles.  224-row tiles (~1.1 of a 192-row tile's time)
    // likewise: 18 464 rows x N = 2304 = 4 rounds of either 256- or 224-row tiles.  Flags 32, 64 and bit 27 switch both off.
    const int cost68 = rows256 ? rounds4 * 120 : rounds3 * 100;
    const bool odd_ok = !(flags & (32 | 64 | (1 << 27)));
    const bool rows160 = odd_ok && rounds5 * 87 < cost68 && rounds5 * 87 <= rounds7 * 110;
    const bool rows224 = odd_ok && !rows160 && rounds7 * 110 < cost68;
    if (rows160 || rows224 || rows256) r = rows160 ? r5 : rows224 ? r7 : r4;
    return fd_gemm_route_persistent(r, FEDDAT_GEMM_V3, N, n_cu);
}
