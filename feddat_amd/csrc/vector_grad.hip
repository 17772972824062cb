// Gradients of per-column vectors over a long row dimension (optimizer_mode bias / norm): a linear layer's bias
// (column sums of the gradient at its output) and a LayerNorm's gamma / beta (sum_r dy * xhat, sum_r dy), over
// R = B * S rows and N = 768 .. 3072 columns.  HBM-bound streaming reductions, no LDS traffic on the row loop:
//
//   partial kernels   grid (ceil(N / 256), slabs): a block owns 256 columns x one slab of VG_SLAB_ROWS = 64 rows.  Its 256
//                     threads are 32 column lanes (8 columns = one 16-byte load of 16-bit operands, two of fp32) x 8 row
//                     lanes; a wave reads two rows x 512 contiguous bytes per load, every thread issues its 8 rows' loads
//                     back to back and accumulates in fp32 registers.  The 8 row lanes meet in LDS once per block, in a
//                     fixed order, and the block writes one fp32 row of `partials` [slabs, N].  At R = 5920, N = 768 that is
//                     3 x 93 = 279 blocks (all 256 CUs), at N = 3072 1116; the partials are 1 / 32 of the bytes read (16-bit).
//   reduce kernel     ONE launch per step for every vector of the step: job j (a device-resident table) folds its
//                     [slabs, N] partials into N floats of the flat gradient, times 1 / (loss scale), and ORs GradScaler's
//                     inf check into a device flag (the role feddat_adapter_wgrad_reduce_checked plays for the adapters).
//
// Summation order is a function of (rows, N) alone -- rows of a slab: row lane j takes rows j, j + 8, ... in order; row lanes
// 0..7 in order; slabs in four interleaved chains (s mod 4) joined as (c0 + c1) + (c2 + c3) -- and there are no floating-point
// atomics: two launches on the same inputs give the same bits.
#include "common.hip.h"

namespace {

constexpr int VG_SLAB_ROWS = 64;     // rows per slab (8 per row lane)
constexpr int VG_COLS = 256;         // columns per block (32 column lanes x 8)
constexpr int VG_RL = 8;             // row lanes per block

__device__ __forceinline__ void vg_load8(const bf16* p, float (&v)[8]) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
}
__device__ __forceinline__ void vg_load8(const float* p, float (&v)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = a[e];
        v[4 + e] = b[e];
    }
}

// T = element type of dy (bf16 = the build's operand type, or float).  LN: also sum_r dy * (x - mean) * rstd.
template <typename T, bool LN>
__global__ __launch_bounds__(256) void vg_partial_kernel(const T* __restrict__ dy, long dy_stride,
                                                         const unsigned char* __restrict__ row_mask,
                                                         const float* __restrict__ x, long x_stride,
                                                         const float* __restrict__ stats, int rows, int N,
                                                         float* __restrict__ sum_part, float* __restrict__ dot_part) {
    __shared__ float red[LN ? 2 : 1][VG_RL][VG_COLS];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int col = blockIdx.x * VG_COLS + cl * 8;
    const int r0 = blockIdx.y * VG_SLAB_ROWS;
    const int r1 = min(rows, r0 + VG_SLAB_ROWS);
    float as[8], ad[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) as[e] = ad[e] = 0.f;
    if (col < N) {
#pragma unroll
        for (int k = 0; k < VG_SLAB_ROWS / VG_RL; ++k) {
            const int r = r0 + rl + k * VG_RL;
            if (r < r1 && (!row_mask || row_mask[r])) {
                float d[8];
                vg_load8(dy + (size_t)r * dy_stride + col, d);
                if (LN) {
                    float xv[8];
                    vg_load8(x + (size_t)r * x_stride + col, xv);
                    const float mean = stats[2 * r], rstd = stats[2 * r + 1];
#pragma unroll
                    for (int e = 0; e < 8; ++e) ad[e] += d[e] * ((xv[e] - mean) * rstd);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) as[e] += d[e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        red[0][rl][cl * 8 + e] = as[e];
        if (LN) red[LN ? 1 : 0][rl][cl * 8 + e] = ad[e];
    }
    __syncthreads();
    // thread t folds column t of the block's 256 over the 8 row lanes, in order
    const int c = blockIdx.x * VG_COLS + threadIdx.x;
    if (c >= N) return;
    float s = red[0][0][threadIdx.x];
#pragma unroll
    for (int j = 1; j < VG_RL; ++j) s += red[0][j][threadIdx.x];
    sum_part[(size_t)blockIdx.y * N + c] = s;
    if (LN && dot_part) {
        float g = red[LN ? 1 : 0][0][threadIdx.x];
#pragma unroll
        for (int j = 1; j < VG_RL; ++j) g += red[LN ? 1 : 0][j][threadIdx.x];
        dot_part[(size_t)blockIdx.y * N + c] = g;
    }
}

__global__ __launch_bounds__(256) void vg_reduce_kernel(const feddat_vgrad_job* __restrict__ jobs, float unscale,
                                                        const float* __restrict__ unscale_dev, int* __restrict__ nonfinite) {
    const feddat_vgrad_job J = jobs[blockIdx.y];
    const int c = blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (c < J.n) {
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        int s = 0;
        for (; s + 4 <= J.slabs; s += 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] += J.partials[(size_t)(s + k) * J.n + c];
        }
        for (int k = 0; s + k < J.slabs; ++k) a[k] += J.partials[(size_t)(s + k) * J.n + c];
        // FEDDAT_VGRAD_UNSCALED: a gradient formed above the point where the loss scale enters the backward (pooler bias)
        const float us = (J.flags & FEDDAT_VGRAD_UNSCALED) ? 1.f : unscale_dev ? unscale * *unscale_dev : unscale;
        const float g = ((a[0] + a[1]) + (a[2] + a[3])) * us;
        J.grad[c] = g;
        bad = fd_nonfinite(g);
    }
    if (nonfinite && __ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(nonfinite, 1);
}

inline int vg_slabs(int rows) { return (rows + VG_SLAB_ROWS - 1) / VG_SLAB_ROWS; }

}  // namespace

extern "C" long feddat_vector_grad_workspace_elems(int rows, int N) {
    if (rows <= 0 || N <= 0) return 0;
    return (long)vg_slabs(rows) * N;
}

extern "C" int feddat_colsum_partial(const void* x_bf16, const float* x_f32, long x_stride, const unsigned char* row_mask,
                                     int rows, int N, float* partials, long partials_elems, hipStream_t stream) {
    FD_CHECK_ARG((x_bf16 != nullptr) != (x_f32 != nullptr));
    FD_CHECK_ARG(partials && rows > 0 && N > 0 && N % 8 == 0 && x_stride >= N && x_stride % 8 == 0);
    FD_CHECK_ARG(partials_elems >= feddat_vector_grad_workspace_elems(rows, N));
    const dim3 grid((N + VG_COLS - 1) / VG_COLS, vg_slabs(rows));
    if (x_bf16)
        hipLaunchKernelGGL((vg_partial_kernel<bf16, false>), grid, dim3(256), 0, stream, (const bf16*)x_bf16, x_stride,
                           row_mask, (const float*)nullptr, 0L, (const float*)nullptr, rows, N, partials, (float*)nullptr);
    else
        hipLaunchKernelGGL((vg_partial_kernel<float, false>), grid, dim3(256), 0, stream, x_f32, x_stride, row_mask,
                           (const float*)nullptr, 0L, (const float*)nullptr, rows, N, partials, (float*)nullptr);
    FD_LAUNCH_RET();
}

extern "C" int feddat_ln_param_grad_partial(const void* dy_bf16, const float* dy_f32, long dy_stride, const float* x,
                                            long x_stride, const float* stats, int rows, int N, float* dgamma_partials,
                                            float* dbeta_partials, long partials_elems, hipStream_t stream) {
    FD_CHECK_ARG((dy_bf16 != nullptr) != (dy_f32 != nullptr));
    FD_CHECK_ARG(dbeta_partials && rows > 0 && N > 0 && N % 8 == 0 && dy_stride >= N && dy_stride % 8 == 0);
    FD_CHECK_ARG(partials_elems >= feddat_vector_grad_workspace_elems(rows, N));
    if (!dgamma_partials)      // beta alone (optimizer_mode bias): a plain column sum of dy, x is not read
        return feddat_colsum_partial(dy_bf16, dy_f32, dy_stride, nullptr, rows, N, dbeta_partials, partials_elems, stream);
    FD_CHECK_ARG(x && stats && x_stride >= N && x_stride % 4 == 0);
    const dim3 grid((N + VG_COLS - 1) / VG_COLS, vg_slabs(rows));
    if (dy_bf16)
        hipLaunchKernelGGL((vg_partial_kernel<bf16, true>), grid, dim3(256), 0, stream, (const bf16*)dy_bf16, dy_stride,
                           (const unsigned char*)nullptr, x, x_stride, stats, rows, N, dbeta_partials, dgamma_partials);
    else
        hipLaunchKernelGGL((vg_partial_kernel<float, true>), grid, dim3(256), 0, stream, dy_f32, dy_stride,
                           (const unsigned char*)nullptr, x, x_stride, stats, rows, N, dbeta_partials, dgamma_partials);
    FD_LAUNCH_RET();
}

extern "C" int feddat_vector_grad_reduce(const feddat_vgrad_job* jobs_dev, int njobs, int max_n, float unscale,
                                         const float* unscale_dev, int* nonfinite, hipStream_t stream) {
    FD_CHECK_ARG(jobs_dev && njobs > 0 && njobs <= 65535 && max_n > 0);
    hipLaunchKernelGGL(vg_reduce_kernel, dim3((max_n + 255) / 256, njobs), dim3(256), 0, stream, jobs_dev,
                       unscale == 0.f ? 1.f : unscale, unscale_dev, nonfinite);
    FD_LAUNCH_RET();
}
