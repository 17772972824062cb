// K3: LayerNorm forward / dX-only backward (frozen affine) / full backward (trainable affine).
// One 64-lane wave per row, the row lives in registers (H <= 2048), float4 I/O.  HBM-bound.
#include "common.hip.h"

namespace {

// MAXC = float4 chunks per lane (H <= 256 * MAXC); instantiated for 3 (H=768), 6 (H=1536), 8 (H<=2048)

template <int MAXC>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, long x_stride,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float eps, int rows, int H, bf16* __restrict__ y16,
                                                     float* __restrict__ y32, float* __restrict__ stats,
                                                     unsigned char* __restrict__ y8 = nullptr,
                                                     float* __restrict__ y8_scale = nullptr) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int nc = H >> 2;
    const float* xr = x + (size_t)row * x_stride;
    f32x4 v[MAXC];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int i = lane + c * 64;
        if (i < nc) {
            v[c] = *reinterpret_cast<const f32x4*>(xr + i * 4);
            s += v[c][0] + v[c][1] + v[c][2] + v[c][3];
        }
    }
    const float mean = wave_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int i = lane + c * 64;
        if (i < nc) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[c][e] - mean;
                q += d * d;
            }
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)H + eps);
    if (stats && lane == 0) {
        stats[2 * row] = mean;
        stats[2 * row + 1] = rstd;
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int i = lane + c * 64;
        if (i < nc) {
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + i * 4);
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(beta + i * 4);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (v[c][e] - mean) * rstd * g4[e] + b4[e];
            if (y16) *reinterpret_cast<bf16x4*>(y16 + (size_t)row * H + i * 4) = cvt4(o);
            if (y32) *reinterpret_cast<f32x4*>(y32 + (size_t)row * H + i * 4) = o;
            v[c] = o;
        }
    }
    if (!y8) return;
    // fp8 (e4m3) copy with a per-row scale: y8 = round(y / s), s = max|y| / 448 (the fp8 GEMM multiplies s back in)
    float amax = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (lane + c * 64 < nc)
#pragma unroll
            for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fabsf(v[c][e]));
    amax = wave_max(amax);
    const float sc = amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f;
    const float inv = 1.0f / sc;
    if (lane == 0) y8_scale[row] = sc;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int i = lane + c * 64;
        if (i < nc) {
            int pk = __builtin_amdgcn_cvt_pk_fp8_f32(v[c][0] * inv, v[c][1] * inv, 0, false);
            pk = __builtin_amdgcn_cvt_pk_fp8_f32(v[c][2] * inv, v[c][3] * inv, pk, true);
            *reinterpret_cast<int*>(y8 + (size_t)row * H + i * 4) = pk;
        }
    }
}

template <int MAXC>
__global__ __launch_bounds__(256) void ln_bwd_dx_kernel(const bf16* __restrict__ dy16, const float* __restrict__ dy32,
                                                        long dy_stride, const float* __restrict__ x, long x_stride,
                                                        const float* __restrict__ stats,
                                                        const float* __restrict__ gamma, const float* __restrict__ dres,
                                                        long dres_stride, int rows, int H, float* __restrict__ out32,
                                                        long out_stride, bf16* __restrict__ out16,
                                                        unsigned char* __restrict__ out8 = nullptr,
                                                        float* __restrict__ out8_scale = nullptr, const int dres_every = 0) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int nc = H >> 2;
    const float mean = stats[2 * row], rstd = stats[2 * row + 1];
    f32x4 xh[MAXC], gg[MAXC];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int i = lane + c * 64;
        if (i < nc) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (size_t)row * x_stride + i * 4);
            f32x4 d;
            if (dy16) {
                const bf16x4 t = *reinterpret_cast<const bf16x4*>(dy16 + (size_t)row * dy_stride + i * 4);
                d = f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
            } else {
                d = *reinterpret_cast<const f32x4*>(dy32 + (size_t)row * dy_stride + i * 4);
            }
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + i * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xh[c][e] = (xv[e] - mean) * rstd;
                gg[c][e] = d[e] * g4[e];
                s1 += gg[c][e];
                s2 += gg[c][e] * xh[c][e];
            }
        }
    }
    const float m1 = wave_sum(s1) / (float)H;
    const float m2 = wave_sum(s2) / (float)H;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int i = lane + c * 64;
        if (i < nc) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = rstd * (gg[c][e] - m1 - xh[c][e] * m2);
            // dres_every = E > 0: the residual gradient is non-zero on rows 0, E, 2 E, ... only and comes COMPACT (row r / E of
            // dres): the top layer's, whose gradient lives on token 0 of every sample (wave-uniform condition)
            if (dres && (dres_every == 0 || row % dres_every == 0)) {
                const size_t rr = dres_every ? (size_t)(row / dres_every) : (size_t)row;
                const f32x4 r4 = *reinterpret_cast<const f32x4*>(dres + rr * dres_stride + i * 4);
                o = o + r4;
            }
            if (out32) *reinterpret_cast<f32x4*>(out32 + (size_t)row * out_stride + i * 4) = o;
            if (out16) *reinterpret_cast<bf16x4*>(out16 + (size_t)row * H + i * 4) = cvt4(o);
            gg[c] = o;
        }
    }
    if (!out8) return;
    // e4m3 copy with a per-row scale (configs[4]: the A operand of the fp8 dX product that follows), as in ln_fwd_kernel
    float amax = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (lane + c * 64 < nc)
#pragma unroll
            for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fabsf(gg[c][e]));
    amax = wave_max(amax);
    const float sc = amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f;
    const float inv = 1.0f / sc;
    if (lane == 0) out8_scale[row] = sc;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int i = lane + c * 64;
        if (i < nc) {
            int pk = __builtin_amdgcn_cvt_pk_fp8_f32(gg[c][0] * inv, gg[c][1] * inv, 0, false);
            pk = __builtin_amdgcn_cvt_pk_fp8_f32(gg[c][2] * inv, gg[c][3] * inv, pk, true);
            *reinterpret_cast<int*>(out8 + (size_t)row * H + i * 4) = pk;
        }
    }
}

// PERSISTENT forms of the two kernels above for H = 256 MAXC exactly and no fp8 copy (H = 768: every LayerNorm of the fp16 / bf16
// step).  The grid is LN_WALK_BLOCKS_PER_CU blocks per CU; wave w of W walks rows w, w + W, w + 2 W, ... and asks for EVERY operand
// of its next row (x; dy, dres and the statistics in the backward) before the first reduction of the current one, so a row costs
// one memory latency instead of two (the one-row kernels fetch dres / gamma / beta after their reductions) and none once the
// walk is under way; gamma / beta are read once per wave.  A row is still one wave's, lane l on chunks l, l + 64, l + 128, summed
// in the same order (c, then e) through the same wave_sum sequence: per row the arithmetic is the one-row kernel's, operation
// for operation, and so are the bits.  The last pass prefetches its own row again (a cache hit), which keeps the loop free of
// branches around loads.
constexpr int LN_WALK_BLOCKS_PER_CU = 2;

template <int MAXC>
__global__ __launch_bounds__(256) void ln_fwd_walk_kernel(const float* __restrict__ x, long x_stride,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float eps, int rows, bf16* __restrict__ y16,
                                                          float* __restrict__ y32, float* __restrict__ stats) {
    constexpr int H = 256 * MAXC;
    const int lane = threadIdx.x & 63;
    const int nwaves = gridDim.x * 4;
    int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= rows) return;
    f32x4 g4[MAXC], b4[MAXC], va[MAXC], vb[MAXC];
    auto load = [&](f32x4(&v)[MAXC], int r) {
#pragma unroll
        for (int c = 0; c < MAXC; ++c) v[c] = *reinterpret_cast<const f32x4*>(x + (size_t)r * x_stride + (lane + c * 64) * 4);
    };
    auto finish = [&](const f32x4(&v)[MAXC], int r) {
        // the fused multiply-adds are spelled out (see ln_bwd_dx_walk_kernel): as in ln_fwd_kernel<3>'s binary, the centred
        // moment is multiply + add and the output ((v - mean) rstd) g + b one fma
#pragma clang fp contract(off)
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) s += v[c][0] + v[c][1] + v[c][2] + v[c][3];
        const float mean = wave_sum(s) / (float)H;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[c][e] - mean;
                q += d * d;
            }
        const float rstd = rsqrtf(wave_sum(q) / (float)H + eps);
        if (stats && lane == 0) {
            stats[2 * r] = mean;
            stats[2 * r + 1] = rstd;
        }
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int i = lane + c * 64;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = __builtin_fmaf((v[c][e] - mean) * rstd, g4[c][e], b4[c][e]);
            if (y16) *reinterpret_cast<bf16x4*>(y16 + (size_t)r * H + i * 4) = cvt4(o);
            if (y32) *reinterpret_cast<f32x4*>(y32 + (size_t)r * H + i * 4) = o;
        }
    };
    load(va, row);
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        g4[c] = *reinterpret_cast<const f32x4*>(gamma + (lane + c * 64) * 4);
        b4[c] = *reinterpret_cast<const f32x4*>(beta + (lane + c * 64) * 4);
    }
    for (;;) {
        const int next = row + nwaves;
        load(vb, next < rows ? next : row);
        finish(va, row);
        if (next >= rows) return;
        row = next;
        __builtin_amdgcn_sched_barrier(0);      // the copy waits for the prefetch: it stays behind this row's stores
#pragma unroll
        for (int c = 0; c < MAXC; ++c) va[c] = vb[c];
    }
}

// one row's operands of the backward.  DY16: dy in the operand format (else fp32).  DRES: 0 none, 1 a row of dres per row,
// 2 compact (dres_every = E > 0: row r / E of dres belongs to rows r = 0, E, 2 E, ... and no other row has one; the top layer's)
template <int MAXC, bool DY16, int DRES>
struct LnBwdRow {
    f32x4 x[MAXC], r[MAXC], d32[MAXC];
    bf16x4 d16[MAXC];
    float mean, rstd;
    bool add_r;
    __device__ __forceinline__ void load(const int row, const int lane, const void* dy, long dy_stride, const float* x_,
                                         long x_stride, const float* stats, const float* dres, long dres_stride,
                                         int dres_every) {
        mean = stats[2 * row];
        rstd = stats[2 * row + 1];
        add_r = DRES == 1 || (DRES == 2 && row % dres_every == 0);      // wave-uniform
        const size_t rr = DRES == 2 ? (size_t)(row / dres_every) : (size_t)row;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int i = lane + c * 64;
            x[c] = *reinterpret_cast<const f32x4*>(x_ + (size_t)row * x_stride + i * 4);
            if (DY16) d16[c] = *reinterpret_cast<const bf16x4*>((const bf16*)dy + (size_t)row * dy_stride + i * 4);
            else d32[c] = *reinterpret_cast<const f32x4*>((const float*)dy + (size_t)row * dy_stride + i * 4);
            if (DRES) r[c] = *reinterpret_cast<const f32x4*>(dres + rr * dres_stride + i * 4);    // compact: a cache hit if unused
        }
    }
};

template <int MAXC, bool DY16, int DRES>
__global__ __launch_bounds__(256) void ln_bwd_dx_walk_kernel(const void* __restrict__ dy, long dy_stride,
                                                             const float* __restrict__ x, long x_stride,
                                                             const float* __restrict__ stats, const float* __restrict__ gamma,
                                                             const float* __restrict__ dres, long dres_stride, int rows,
                                                             float* __restrict__ out32, long out_stride,
                                                             bf16* __restrict__ out16, const int dres_every) {
    static_assert(MAXC == 3, "finish() spells out ln_bwd_dx_kernel<3>'s fused multiply-adds");
    constexpr int H = 256 * MAXC;
    const int lane = threadIdx.x & 63;
    const int nwaves = gridDim.x * 4;
    int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= rows) return;
    f32x4 g4[MAXC];
    LnBwdRow<MAXC, DY16, DRES> ra, rb;
    auto load = [&](LnBwdRow<MAXC, DY16, DRES>& R, int r) {
        R.load(r, lane, dy, dy_stride, x, x_stride, stats, dres, dres_stride, dres_every);
    };
    auto finish = [&](const LnBwdRow<MAXC, DY16, DRES>& R, int r) {
        // Which multiply-adds are fused is spelled out: left to the compiler it changes with the code around an expression (it
        // did here: this loop body came out with other fusions than ln_bwd_dx_kernel's), and the result must not.  The choices
        // below are those of ln_bwd_dx_kernel<3> as hipcc builds it, in both operand formats: s2 unfused; the output's
        // - xhat m2 fused into (g - m1), EXCEPT in the last two elements of the third chunk.
#pragma clang fp contract(off)
        const float mean = R.mean, rstd = R.rstd;
        f32x4 xh[MAXC], gg[MAXC];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            f32x4 d;
            if (DY16) d = f32x4{(float)R.d16[c][0], (float)R.d16[c][1], (float)R.d16[c][2], (float)R.d16[c][3]};
            else d = R.d32[c];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xh[c][e] = (R.x[c][e] - mean) * rstd;
                gg[c][e] = d[e] * g4[c][e];
                s1 += gg[c][e];
                s2 += gg[c][e] * xh[c][e];
            }
        }
        const float m1 = wave_sum(s1) / (float)H;
        const float m2 = wave_sum(s2) / (float)H;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int i = lane + c * 64;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = gg[c][e] - m1;
                o[e] = rstd * (c == 2 && e >= 2 ? t - xh[c][e] * m2 : __builtin_fmaf(-xh[c][e], m2, t));
            }
            if (DRES && R.add_r) o = o + R.r[c];
            if (out32) *reinterpret_cast<f32x4*>(out32 + (size_t)r * out_stride + i * 4) = o;
            if (out16) *reinterpret_cast<bf16x4*>(out16 + (size_t)r * H + i * 4) = cvt4(o);
        }
    };
    load(ra, row);
#pragma unroll
    for (int c = 0; c < MAXC; ++c) g4[c] = *reinterpret_cast<const f32x4*>(gamma + (lane + c * 64) * 4);
    for (;;) {
        const int next = row + nwaves;
        load(rb, next < rows ? next : row);
        finish(ra, row);
        if (next >= rows) return;
        row = next;
        __builtin_amdgcn_sched_barrier(0);      // the copy waits for the prefetch: it stays behind this row's stores
        ra = rb;
    }
}

// trainable-affine backward for the task head's clf_norm0 (rows <= 1024): one block per 64 columns,
// lanes over columns for dgamma/dbeta; dx by the wave-per-row kernel above with fp32 dy.
__global__ __launch_bounds__(256) void ln_bwd_affine_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ stats, int rows, int H,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ float sg[4][64], sb[4][64];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63);
    const int part = threadIdx.x >> 6;
    float ag = 0.f, ab = 0.f;
    if (col < H) {
        for (int r = part; r < rows; r += 4) {
            const float d = dy[(size_t)r * H + col];
            const float xh = (x[(size_t)r * H + col] - stats[2 * r]) * stats[2 * r + 1];
            ag += d * xh;
            ab += d;
        }
    }
    sg[part][threadIdx.x & 63] = ag;
    sb[part][threadIdx.x & 63] = ab;
    __syncthreads();
    if (part == 0 && col < H) {
        const int l = threadIdx.x;
        dgamma[col] = (sg[0][l] + sg[1][l]) + (sg[2][l] + sg[3][l]);
        dbeta[col] = (sb[0][l] + sb[1][l]) + (sb[2][l] + sb[3][l]);
    }
}

}  // namespace

// grid of the persistent H = 768 kernels: one wave per row up to LN_WALK_BLOCKS_PER_CU blocks of 4 waves per CU
static int ln_walk_grid(int rows, int* grid) {
    int n_cu = 0;
    if (fd_device_cus(&n_cu) != FEDDAT_OK) return FEDDAT_ELAUNCH;
    const int need = (rows + 3) / 4, cap = n_cu * LN_WALK_BLOCKS_PER_CU;
    *grid = need < cap ? need : cap;
    return FEDDAT_OK;
}

static int ln_bwd_dx_walk(const void* dy_bf16, const float* dy_f32, long dy_stride, const float* x, long x_stride,
                          const float* stats, const float* gamma, const float* dres, long dres_stride, int dres_every, int rows,
                          float* out_f32, long out_stride, void* out_bf16, hipStream_t stream) {
    int grid;
    if (ln_walk_grid(rows, &grid) != FEDDAT_OK) return FEDDAT_ELAUNCH;
    const void* dy = dy_bf16 ? dy_bf16 : (const void*)dy_f32;
#define LN_WALK(DY16, DRES)                                                                                              \
    hipLaunchKernelGGL((ln_bwd_dx_walk_kernel<3, DY16, DRES>), dim3(grid), dim3(256), 0, stream, dy, dy_stride, x, x_stride, \
                       stats, gamma, dres, dres_stride, rows, out_f32, out_stride, (bf16*)out_bf16, dres_every)
    const int mode = !dres ? 0 : dres_every ? 2 : 1;
    if (dy_bf16) {
        if (mode == 0) LN_WALK(true, 0); else if (mode == 1) LN_WALK(true, 1); else LN_WALK(true, 2);
    } else {
        if (mode == 0) LN_WALK(false, 0); else if (mode == 1) LN_WALK(false, 1); else LN_WALK(false, 2);
    }
#undef LN_WALK
    FD_LAUNCH_RET();
}

extern "C" int feddat_layernorm_fwd(const float* x, long x_stride, const float* gamma, const float* beta, float eps,
                                    int rows, int H, void* y_bf16, float* y_f32, float* stats, hipStream_t stream) {
    FD_CHECK_ARG(x && gamma && beta && rows > 0 && H > 0 && H % 4 == 0 && H <= 2048 && x_stride % 4 == 0);
    FD_CHECK_ARG(y_bf16 || y_f32);
#define LN_FWD(MC)                                                                                              \
    hipLaunchKernelGGL(ln_fwd_kernel<MC>, dim3((rows + 3) / 4), dim3(256), 0, stream, x, x_stride, gamma, beta, eps, \
                       rows, H, (bf16*)y_bf16, y_f32, stats)
    if (H == 768) {
        int grid;
        if (ln_walk_grid(rows, &grid) != FEDDAT_OK) return FEDDAT_ELAUNCH;
        hipLaunchKernelGGL(ln_fwd_walk_kernel<3>, dim3(grid), dim3(256), 0, stream, x, x_stride, gamma, beta, eps, rows,
                           (bf16*)y_bf16, y_f32, stats);
    } else if (H <= 768) LN_FWD(3); else if (H <= 1536) LN_FWD(6); else LN_FWD(8);
#undef LN_FWD
    FD_LAUNCH_RET();
}

extern "C" int feddat_layernorm_fwd_fp8(const float* x, long x_stride, const float* gamma, const float* beta, float eps,
                                        int rows, int H, void* y_fp8, float* y_scale, void* y_bf16, float* stats,
                                        hipStream_t stream) {
    FD_CHECK_ARG(x && gamma && beta && rows > 0 && H > 0 && H % 4 == 0 && H <= 2048 && x_stride % 4 == 0);
    FD_CHECK_ARG(y_fp8 && y_scale);
#define LN_FWD8(MC)                                                                                              \
    hipLaunchKernelGGL(ln_fwd_kernel<MC>, dim3((rows + 3) / 4), dim3(256), 0, stream, x, x_stride, gamma, beta, eps, \
                       rows, H, (bf16*)y_bf16, (float*)nullptr, stats, (unsigned char*)y_fp8, y_scale)
    if (H <= 768) LN_FWD8(3); else if (H <= 1536) LN_FWD8(6); else LN_FWD8(8);
#undef LN_FWD8
    FD_LAUNCH_RET();
}

// x fp32 [rows, cols] (row stride ld) -> e4m3 [rows, cols] + per-row scale (amax / 448): frozen weights (per output
// channel) at load time, or any activation
namespace {
__global__ __launch_bounds__(256) void quant_rows_fp8_kernel(const float* __restrict__ x, long ld, int cols,
                                                             unsigned char* __restrict__ y, float* __restrict__ scale) {
    __shared__ float red[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* xr = x + (size_t)row * ld;
    float amax = 0.f;
    for (int c = tid * 4; c < cols; c += 1024) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + c);
        amax = fmaxf(fmaxf(amax, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
    }
    amax = wave_max(amax);
    if ((tid & 63) == 0) red[tid >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float sc = amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f;
    const float inv = 1.0f / sc;
    if (tid == 0) scale[row] = sc;
    for (int c = tid * 4; c < cols; c += 1024) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + c);
        int pk = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv, v[1] * inv, 0, false);
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv, v[3] * inv, pk, true);
        *reinterpret_cast<int*>(y + (size_t)row * cols + c) = pk;
    }
}
}  // namespace

extern "C" int feddat_quant_rows_fp8(const float* x, long ld, int rows, int cols, void* y_fp8, float* scale,
                                     hipStream_t stream) {
    FD_CHECK_ARG(x && y_fp8 && scale && rows > 0 && cols > 0 && cols % 4 == 0 && ld % 4 == 0 && ld >= cols);
    hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3(rows), dim3(256), 0, stream, x, ld, cols, (unsigned char*)y_fp8, scale);
    FD_LAUNCH_RET();
}

extern "C" int feddat_layernorm_bwd_dx(const void* dy_bf16, const float* dy_f32, long dy_stride, const float* x,
                                       long x_stride, const float* stats, const float* gamma, const float* dres,
                                       long dres_stride, int rows, int H, float* out_f32, long out_stride,
                                       void* out_bf16, hipStream_t stream) {
    FD_CHECK_ARG((dy_bf16 != nullptr) != (dy_f32 != nullptr));
    FD_CHECK_ARG(x && stats && gamma && rows > 0 && H > 0 && H % 4 == 0 && H <= 2048);
    FD_CHECK_ARG(dy_stride % 4 == 0 && x_stride % 4 == 0 && (!dres || dres_stride % 4 == 0));
    FD_CHECK_ARG((out_f32 && out_stride % 4 == 0) || out_bf16);
#define LN_BWD(MC)                                                                                                \
    hipLaunchKernelGGL(ln_bwd_dx_kernel<MC>, dim3((rows + 3) / 4), dim3(256), 0, stream, (const bf16*)dy_bf16, dy_f32, \
                       dy_stride, x, x_stride, stats, gamma, dres, dres_stride, rows, H, out_f32, out_stride,          \
                       (bf16*)out_bf16)
    if (H == 768)
        return ln_bwd_dx_walk(dy_bf16, dy_f32, dy_stride, x, x_stride, stats, gamma, dres, dres_stride, 0, rows, out_f32,
                              out_stride, out_bf16, stream);
    if (H <= 768) LN_BWD(3); else if (H <= 1536) LN_BWD(6); else LN_BWD(8);
#undef LN_BWD
    FD_LAUNCH_RET();
}

extern "C" int feddat_layernorm_bwd_dx_sparse(const void* dy_bf16, const float* dy_f32, long dy_stride, const float* x,
                                              long x_stride, const float* stats, const float* gamma, const float* dres,
                                              long dres_stride, int dres_every, int rows, int H, float* out_f32,
                                              long out_stride, void* out_bf16, hipStream_t stream) {
    FD_CHECK_ARG((dy_bf16 != nullptr) != (dy_f32 != nullptr));
    FD_CHECK_ARG(x && stats && gamma && dres && dres_every > 0 && rows > 0 && H > 0 && H % 4 == 0 && H <= 2048);
    FD_CHECK_ARG(dy_stride % 4 == 0 && x_stride % 4 == 0 && dres_stride % 4 == 0);
    FD_CHECK_ARG((out_f32 && out_stride % 4 == 0) || out_bf16);
#define LN_BWDS(MC)                                                                                               \
    hipLaunchKernelGGL(ln_bwd_dx_kernel<MC>, dim3((rows + 3) / 4), dim3(256), 0, stream, (const bf16*)dy_bf16, dy_f32, \
                       dy_stride, x, x_stride, stats, gamma, dres, dres_stride, rows, H, out_f32, out_stride,          \
                       (bf16*)out_bf16, (unsigned char*)nullptr, (float*)nullptr, dres_every)
    if (H == 768)
        return ln_bwd_dx_walk(dy_bf16, dy_f32, dy_stride, x, x_stride, stats, gamma, dres, dres_stride, dres_every, rows,
                              out_f32, out_stride, out_bf16, stream);
    if (H <= 768) LN_BWDS(3); else if (H <= 1536) LN_BWDS(6); else LN_BWDS(8);
#undef LN_BWDS
    FD_LAUNCH_RET();
}

extern "C" int feddat_layernorm_bwd_dx_fp8(const void* dy_bf16, const float* dy_f32, long dy_stride, const float* x,
                                           long x_stride, const float* stats, const float* gamma, const float* dres,
                                           long dres_stride, int rows, int H, float* out_f32, long out_stride,
                                           void* out_bf16, void* out_fp8, float* out_scale, hipStream_t stream) {
    FD_CHECK_ARG((dy_bf16 != nullptr) != (dy_f32 != nullptr));
    FD_CHECK_ARG(x && stats && gamma && rows > 0 && H > 0 && H % 4 == 0 && H <= 2048 && out_fp8 && out_scale);
    FD_CHECK_ARG(dy_stride % 4 == 0 && x_stride % 4 == 0 && (!dres || dres_stride % 4 == 0) && (!out_f32 || out_stride % 4 == 0));
#define LN_BWD8(MC)                                                                                               \
    hipLaunchKernelGGL(ln_bwd_dx_kernel<MC>, dim3((rows + 3) / 4), dim3(256), 0, stream, (const bf16*)dy_bf16, dy_f32, \
                       dy_stride, x, x_stride, stats, gamma, dres, dres_stride, rows, H, out_f32, out_stride,          \
                       (bf16*)out_bf16, (unsigned char*)out_fp8, out_scale)
    if (H <= 768) LN_BWD8(3); else if (H <= 1536) LN_BWD8(6); else LN_BWD8(8);
#undef LN_BWD8
    FD_LAUNCH_RET();
}

extern "C" int feddat_layernorm_bwd_full(const float* dy, const float* x, const float* stats, const float* gamma,
                                         int rows, int H, float* dx, float* dgamma, float* dbeta,
                                         hipStream_t stream) {
    FD_CHECK_ARG(dy && x && stats && gamma && dx && dgamma && dbeta && rows > 0 && rows <= 1024);
    FD_CHECK_ARG(H > 0 && H % 4 == 0 && H <= 2048);
    hipLaunchKernelGGL(ln_bwd_affine_kernel, dim3((H + 63) / 64), dim3(256), 0, stream, dy, x, stats, rows, H, dgamma,
                       dbeta);
    return feddat_layernorm_bwd_dx(nullptr, dy, (long)H, x, (long)H, stats, gamma, nullptr, 0L, rows, H, dx, (long)H,
                                   nullptr, stream);
}
