// The serial tail of a DAT train_step: ViltModel.layernorm + ViltPooler on the token-0 rows, the task head
// (src/modeling/vilt.py:202-209: fc0 -> LayerNorm(1536, eps 1e-5) -> GELU -> fc1) forward and backward for the P0 / P1 / P2
// passes, the DAT loss, and the AdamW / scheduler bookkeeping (src/train/visionlanguage_tasks/task_trainer.py:280-330,
// 477-504).  All exact fp32, ~0.2 GFLOP in total: the cost is LAUNCHES (round 3: 48 kernels of 2-10 us behind each other, a
// fifth of the step's graph nodes), so this file fuses what used to be separate kernels:
//   * ht_gemm_kernel: the strided exact-fp32 MFMA product of sgemm_f32.hip with the K range split over the 8 waves of a
//     block (no split-K partials in HBM, no reduce launch), an optional A-side prologue (LayerNorm of the rows with the
//     statistics computed in the block; multiply by 1 - y^2 = tanh'), an optional epilogue (bias, tanh, multiply by
//     gelu'(aux)), the column sum that gives a weight-gradient job its bias gradient, and up to TWO independent products
//     per launch (e.g. dW_fc1 = dl^T g0 next to dn0 = (dl W_fc1) * gelu'(n0));
//   * ht_ln_gelu_kernel, ht_ln_bwd_full_kernel: the head's LayerNorm + GELU, and its full backward (dx, dgamma, dbeta) in one
//     launch each; dat_loss_single_kernel: loss + dlogits + the batch reduction in one block;
//   * adamw_multi_kernel / step_tick_multi_kernel: the step's last three AdamW launches as one, their four counter ticks
//     as one (an AdamW launch can read its schedule / step counters at an offset, so the head's second update does not
//     need a tick between the two).
#include "common.hip.h"

namespace {

constexpr int HT_JT = 4;       // 16-column tiles per wave sharing one A operand (block tile: 16 rows x 64 columns)
constexpr int HT_NW = 8;       // waves per block
constexpr int HT_U = 3;        // 16-deep k-chunks whose loads are in flight together per wave

struct HtJob {
    const float* A; long sa_i, sa_k;
    const float* B; long sb_k, sb_j;
    int I, J, K;
    int mode;                  // 0: the block's waves split K (summed through LDS in wave order); 1: the waves take
                               //    consecutive j-groups, each over the whole K (short contractions: K = batch)
    float alpha;
    const float* alpha_dev;    // optional device factor on alpha (the dynamic loss scale)
    const float* bias_j;
    float* out; long ldo;
    float* colsum;             // colsum[i] = alpha * sum_k A'[i][k]  (A' = A after the prologue)
    int pro;                   // FEDDAT_HT_PRO_*
    const float* pro_a;        // LN: gamma [K]           TANH_BWD: y, indexed like A
    const float* pro_b;        // LN: beta [K]
    float pro_eps;
    float* stats_out;          // LN: [I, 2] = {mean, rstd} (optional)
    int epi;                   // FEDDAT_HT_EPI_*
    const float* aux; long ld_aux;
    int itiles, jblocks;       // grid decomposition of this job
    int avec, bvec;            // operand contiguous along k and 16-byte aligned: float4 loads
    int jt;                    // 16-column tiles per wave (1 or HT_JT)
};
struct HtLaunch {
    HtJob job[2];
    int blocks0;               // blocks [0, blocks0) run job 0, the rest job 1
};

// Main loop of one wave: k runs in chunks of 16; inside a chunk, MFMA step e (0..3) gives lane group g the index
// k = chunk + 4 g + e -- for BOTH operands, which is all the instruction needs (its four k slots are summed).  An operand
// that is contiguous along k is therefore fetched as ONE 16-byte load per lane and chunk (AV / BV; a product whose B is
// [J, K] row-major used to issue 16 separate 64-byte segments per dword load and was bound by the CU's address path, not by
// bytes: 44 us for the 64 x 1536 x 768 fc0 product); the other layout (contiguous along i / j) keeps dword loads, which
// are 64-byte runs per lane group there.
template <bool AV, bool BV, int JT>
__device__ __forceinline__ void ht_mainloop(const HtJob& p, const float* ap, const float* yp, const float* const (&bp)[JT],
                                            const bool iv, const bool (&jv)[JT], const int g, const float mean,
                                            const float rstd, const int c_first, const int c_step, f32x4 (&acc)[JT],
                                            float& asum) {
    const int nchunk = (p.K + 15) >> 4;
    for (int c0 = c_first; c0 < nchunk; c0 += c_step * HT_U) {
        f32x4 a[HT_U], y[HT_U], ga[HT_U], be[HT_U], b[HT_U][JT];
#pragma unroll
        for (int u = 0; u < HT_U; ++u) {
            const int k0 = (c0 + c_step * u) * 16 + 4 * g;           // this lane's four k of the chunk: k0 .. k0 + 3
            const bool in = k0 < p.K;                                // (K % 4 == 0 where a vector load is used)
            const int kc = in ? k0 : 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ke = min(k0 + e, p.K - 1);
                if (!AV) a[u][e] = ap[(size_t)ke * p.sa_k];
                if (!AV && p.pro == FEDDAT_HT_PRO_TANH_BWD) y[u][e] = yp[(size_t)ke * p.sa_k];
            }
            if (AV) {
                a[u] = *reinterpret_cast<const f32x4*>(ap + kc);
                if (p.pro == FEDDAT_HT_PRO_TANH_BWD) y[u] = *reinterpret_cast<const f32x4*>(yp + kc);
            }
            if (p.pro == FEDDAT_HT_PRO_LN) {                         // (LN implies AV: checked on the host)
                ga[u] = *reinterpret_cast<const f32x4*>(p.pro_a + kc);
                be[u] = *reinterpret_cast<const f32x4*>(p.pro_b + kc);
            }
#pragma unroll
            for (int t = 0; t < JT; ++t) {
                if (BV) {
                    b[u][t] = *reinterpret_cast<const f32x4*>(bp[t] + kc);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) b[u][t][e] = bp[t][(size_t)min(k0 + e, p.K - 1) * p.sb_k];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < HT_U; ++u) {
            const int k0 = (c0 + c_step * u) * 16 + 4 * g;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool kv = (k0 + e) < p.K && (c0 + c_step * u) < nchunk;
                float av = a[u][e];
                if (p.pro == FEDDAT_HT_PRO_LN) av = (av - mean) * rstd * ga[u][e] + be[u][e];
                if (p.pro == FEDDAT_HT_PRO_TANH_BWD) av = av * (1.f - y[u][e] * y[u][e]);
                av = (iv && kv) ? av : 0.f;
                asum += av;
#pragma unroll
                for (int t = 0; t < JT; ++t) acc[t] = mfma16x4_f32(av, (jv[t] && kv) ? b[u][t][e] : 0.f, acc[t]);
            }
        }
    }
}

// JT = 16-column tiles per wave: 4 (64 columns per block) for the products with enough tiles to fill the chip, 1 for the
// few-tile ones (fc1: 64 x 100; d(pooled): 32 x 768 -- their time is one wave's chain of dependent load batches, so more,
// narrower blocks win).
template <int JT>
__device__ __forceinline__ void ht_body(const HtJob& p, const int wid, float* ht_smem) {
    float (*red)[64][HT_JT * 4 + 4] = reinterpret_cast<float (*)[64][HT_JT * 4 + 4]>(ht_smem);     // [HT_NW - 1]
    float (*srow)[2] = reinterpret_cast<float (*)[2]>(ht_smem + (HT_NW - 1) * 64 * (HT_JT * 4 + 4));     // [16]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int itile = wid / p.jblocks, jb = wid - itile * p.jblocks;
    const int i16 = lane & 15, g = lane >> 4;
    const int i = itile * 16 + i16;
    const bool iv = i < p.I;
    const float* ap = p.A + (size_t)(iv ? i : 0) * p.sa_i;
    const float* yp = p.pro == FEDDAT_HT_PRO_TANH_BWD ? p.pro_a + (size_t)(iv ? i : 0) * p.sa_i : nullptr;

    // LayerNorm prologue: wave w computes the statistics of rows 16 itile + w, + w + HT_NW
    float mean = 0.f, rstd = 0.f;
    if (p.pro == FEDDAT_HT_PRO_LN) {
        for (int rl = wave; rl < 16; rl += HT_NW) {
            const int r = itile * 16 + rl;
            if (r >= p.I) continue;
            // (sa_k == 1, K % 4 == 0, K <= 2048: checked on the host) the row sits in registers: one pass of loads
            const float* xr = p.A + (size_t)r * p.sa_i;
            const int nc = p.K >> 2;
            f32x4 v[8];
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int q4 = lane + c * 64;
                if (q4 < nc) {
                    v[c] = *reinterpret_cast<const f32x4*>(xr + q4 * 4);
                    s += v[c][0] + v[c][1] + v[c][2] + v[c][3];
                }
            }
            const float m = wave_sum(s) / (float)p.K;
            float q = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (lane + c * 64 < nc)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float d = v[c][e] - m;
                        q += d * d;
                    }
            const float rs = rsqrtf(wave_sum(q) / (float)p.K + p.pro_eps);
            if (lane == 0) {
                srow[rl][0] = m;
                srow[rl][1] = rs;
                if (p.stats_out && jb == 0) {
                    p.stats_out[2 * r] = m;
                    p.stats_out[2 * r + 1] = rs;
                }
            }
        }
        __syncthreads();
        mean = srow[i16][0];
        rstd = srow[i16][1];
    }

    const int jgrp = p.mode == 0 ? jb : jb * HT_NW + wave;
    int j[JT];
    bool jv[JT];
    const float* bp[JT];
#pragma unroll
    for (int t = 0; t < JT; ++t) {
        j[t] = (jgrp * JT + t) * 16 + i16;
        jv[t] = j[t] < p.J;
        bp[t] = p.B + (size_t)(jv[t] ? j[t] : 0) * p.sb_j;
    }
    f32x4 acc[JT];
#pragma unroll
    for (int t = 0; t < JT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float asum = 0.f;
    const int c_first = p.mode == 0 ? wave : 0, c_step = p.mode == 0 ? HT_NW : 1;
    if (p.avec && p.bvec) ht_mainloop<true, true, JT>(p, ap, yp, bp, iv, jv, g, mean, rstd, c_first, c_step, acc, asum);
    else if (p.avec) ht_mainloop<true, false, JT>(p, ap, yp, bp, iv, jv, g, mean, rstd, c_first, c_step, acc, asum);
    else if (p.bvec) ht_mainloop<false, true, JT>(p, ap, yp, bp, iv, jv, g, mean, rstd, c_first, c_step, acc, asum);
    else ht_mainloop<false, false, JT>(p, ap, yp, bp, iv, jv, g, mean, rstd, c_first, c_step, acc, asum);
    asum += __shfl_xor(asum, 16, 64);
    asum += __shfl_xor(asum, 32, 64);
    if (p.mode == 0) {
        if (wave > 0) {
            float* dst = red[wave - 1][lane];
#pragma unroll
            for (int t = 0; t < JT; ++t) *reinterpret_cast<f32x4*>(dst + 4 * t) = acc[t];
            dst[JT * 4] = asum;
        }
        __syncthreads();
        if (wave != 0) return;
#pragma unroll 1
        for (int w = 0; w < HT_NW - 1; ++w) {
            const float* src = red[w][lane];
#pragma unroll
            for (int t = 0; t < JT; ++t) acc[t] = acc[t] + *reinterpret_cast<const f32x4*>(src + 4 * t);
            asum += src[JT * 4];
        }
    }
    const float alpha = p.alpha_dev ? p.alpha * *p.alpha_dev : p.alpha;      // (a power of two: the product is exact)
#pragma unroll
    for (int t = 0; t < JT; ++t) {
        if (!jv[t]) continue;
        const float bj = p.bias_j ? p.bias_j[j[t]] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int io = itile * 16 + 4 * g + e;
            if (io >= p.I) continue;
            float v = alpha * acc[t][e] + bj;
            if (p.epi == FEDDAT_HT_EPI_TANH) v = tanhf(v);
            if (p.epi == FEDDAT_HT_EPI_MUL_DGELU) v *= gelu_grad_f(p.aux[(size_t)io * p.ld_aux + j[t]]);
            p.out[(size_t)io * p.ldo + j[t]] = v;
        }
    }
    if (p.colsum && jgrp == 0 && g == 0 && iv) p.colsum[i] = alpha * asum;
}

__global__ __launch_bounds__(HT_NW * 64) void ht_gemm_kernel(const HtLaunch L) {
    extern __shared__ __attribute__((aligned(16))) float ht_smem[];
    const bool second = (int)blockIdx.x >= L.blocks0;
    const HtJob& p = L.job[second ? 1 : 0];
    const int wid = second ? blockIdx.x - L.blocks0 : blockIdx.x;
    if (p.jt == 1) ht_body<1>(p, wid, ht_smem);
    else ht_body<HT_JT>(p, wid, ht_smem);
}

// y = LayerNorm(x) (fp32, stats), g = gelu(y): one wave per row, H <= 2048
__global__ __launch_bounds__(256) void ht_ln_gelu_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps, int rows, int H,
                                                         float* __restrict__ y, float* __restrict__ stats,
                                                         float* __restrict__ gl) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int nc = H >> 2;
    const float* xr = x + (size_t)row * H;
    f32x4 v[8];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int i = lane + c * 64;
        if (i < nc) {
            v[c] = *reinterpret_cast<const f32x4*>(xr + i * 4);
            s += v[c][0] + v[c][1] + v[c][2] + v[c][3];
        }
    }
    const float mean = wave_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (lane + c * 64 < nc)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[c][e] - mean;
                q += d * d;
            }
    const float rstd = rsqrtf(wave_sum(q) / (float)H + eps);
    if (lane == 0) {
        stats[2 * row] = mean;
        stats[2 * row + 1] = rstd;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int i = lane + c * 64;
        if (i < nc) {
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + i * 4);
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(beta + i * 4);
            f32x4 o, ge;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[e] = (v[c][e] - mean) * rstd * g4[e] + b4[e];
                ge[e] = gelu_f(o[e]);
            }
            *reinterpret_cast<f32x4*>(y + (size_t)row * H + i * 4) = o;
            *reinterpret_cast<f32x4*>(gl + (size_t)row * H + i * 4) = ge;
        }
    }
}

// Full LayerNorm backward (trainable affine) in one launch: blocks [0, ceil(rows / 4)) give dx (one wave per row),
// the rest give dgamma / dbeta (64 columns per block, four row-interleaved partial sums, fixed order).
__global__ __launch_bounds__(256) void ht_ln_bwd_full_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                             const float* __restrict__ stats,
                                                             const float* __restrict__ gamma, int rows, int H,
                                                             float* __restrict__ dx, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta) {
    __shared__ float sg[4][64], sb[4][64];
    const int row_blocks = (rows + 3) / 4;
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
    if ((int)blockIdx.x < row_blocks) {
        const int row = blockIdx.x * 4 + part;
        if (row >= rows) return;
        const int nc = H >> 2;
        const float mean = stats[2 * row], rstd = stats[2 * row + 1];
        f32x4 gd[8], xh[8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int i = lane + c * 64;
            if (i < nc) {
                const f32x4 d4 = *reinterpret_cast<const f32x4*>(dy + (size_t)row * H + i * 4);
                const f32x4 x4 = *reinterpret_cast<const f32x4*>(x + (size_t)row * H + i * 4);
                const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + i * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    gd[c][e] = d4[e] * g4[e];
                    xh[c][e] = (x4[e] - mean) * rstd;
                    s1 += gd[c][e];
                    s2 += gd[c][e] * xh[c][e];
                }
            }
        }
        const float m1 = wave_sum(s1) / (float)H, m2 = wave_sum(s2) / (float)H;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int i = lane + c * 64;
            if (i < nc) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = rstd * (gd[c][e] - m1 - xh[c][e] * m2);
                *reinterpret_cast<f32x4*>(dx + (size_t)row * H + i * 4) = o;
            }
        }
        return;
    }
    const int col = ((int)blockIdx.x - row_blocks) * 64 + lane;
    float ag = 0.f, ab = 0.f;
    if (col < H) {
        for (int r = part; r < rows; r += 4) {
            const float d = dy[(size_t)r * H + col];
            ag += d * ((x[(size_t)r * H + col] - stats[2 * r]) * stats[2 * r + 1]);
            ab += d;
        }
    }
    sg[part][lane] = ag;
    sb[part][lane] = ab;
    __syncthreads();
    if (part == 0 && col < H) {
        dgamma[col] = (sg[0][lane] + sg[1][lane]) + (sg[2][lane] + sg[3][lane]);
        dbeta[col] = (sb[0][lane] + sb[1][lane]) + (sb[2][lane] + sb[3][lane]);
    }
}

// DAT loss (task_trainer.py:299-301, 506-516) in ONE launch: wave w takes rows w, w + 16, ...; the batch sums run over
// the row terms in LDS in the order of the two-kernel form (feddat_dat_loss_fwd_bwd), so both give the same bits.
__device__ __forceinline__ void dat_loss_single_body(const float* __restrict__ logits, const float* __restrict__ teacher,
                                                     const float* __restrict__ target, int B, int C, float temp,
                                                     float* __restrict__ dlogits, float* __restrict__ scalars,
                                                     int* __restrict__ nonfinite) {
    extern __shared__ float terms[];       // [2 B]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float it = 1.0f / temp;
    // C <= 128 (the VQA heads: 100 labels): two elements per lane, the rows of a wave are loaded up front (RPW at a time) so
    // that their three passes run from registers -- the launch is a chain of dependent reductions, not bytes
    constexpr int RPW = 4;
    for (int b0 = wave; b0 < B; b0 += 16 * RPW) {
        float xv[RPW][2], tv[RPW][2], yv[RPW][2];
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int b = b0 + 16 * r;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = lane + 64 * h;
                const bool ok = b < B && j < C;
                xv[r][h] = ok ? logits[(size_t)b * C + j] : 0.f;
                tv[r][h] = ok ? teacher[(size_t)b * C + j] : 0.f;
                yv[r][h] = ok ? target[(size_t)b * C + j] : 0.f;
            }
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int b = b0 + 16 * r;
            if (b >= B) break;
            const bool v0 = lane < C, v1 = lane + 64 < C;
            float mx = fmaxf(v0 ? xv[r][0] * it : -INFINITY, v1 ? xv[r][1] * it : -INFINITY);
            float mt = fmaxf(v0 ? tv[r][0] * it : -INFINITY, v1 ? tv[r][1] * it : -INFINITY);
            mx = wave_max(mx);
            mt = wave_max(mt);
            float sx = (v0 ? expf(xv[r][0] * it - mx) : 0.f) + (v1 ? expf(xv[r][1] * it - mx) : 0.f);
            float st = (v0 ? expf(tv[r][0] * it - mt) : 0.f) + (v1 ? expf(tv[r][1] * it - mt) : 0.f);
            sx = wave_sum(sx);
            st = wave_sum(st);
            const float lsx = mx + logf(sx), lst = mt + logf(st);
            float bce = 0.f, kl = 0.f;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (!(h ? v1 : v0)) continue;
                const float x = xv[r][h];
                bce += fmaxf(x, 0.f) - x * yv[r][h] + log1pf(expf(-fabsf(x)));
                const float logp = x * it - lsx;
                const float logq = tv[r][h] * it - lst;
                const float q = expf(logq);
                kl += q * (logq - logp);
                const float sig = 1.0f / (1.0f + expf(-x));
                dlogits[(size_t)b * C + lane + 64 * h] = 0.5f / (float)B * ((sig - yv[r][h]) + temp * (expf(logp) - q));
            }
            bce = wave_sum(bce);
            kl = wave_sum(kl);
            if (lane == 0) {
                terms[2 * b] = bce;
                terms[2 * b + 1] = kl;
            }
        }
    }
    __syncthreads();
    if (wave != 0) return;
    float bce = 0.f, kl = 0.f;
    for (int b = lane; b < B; b += 64) {
        bce += terms[2 * b];
        kl += terms[2 * b + 1];
    }
    bce = wave_sum(bce);
    kl = wave_sum(kl);
    if (lane == 0) {
        const float l_bce = bce / (float)B;
        const float l_kl = kl / (float)B * temp * temp;
        scalars[0] = l_bce;
        scalars[1] = l_kl;
        scalars[2] = 0.5f * (l_bce + l_kl);
        // GradScaler's inf check, at its source: a non-finite loss means non-finite gradients in every parameter it reaches
        if (nonfinite && fd_nonfinite(l_bce + l_kl)) atomicOr(nonfinite, 1);
    }
}

__global__ __launch_bounds__(1024) void dat_loss_single_kernel(const float* __restrict__ logits,
                                                               const float* __restrict__ teacher,
                                                               const float* __restrict__ target, int B, int C, float temp,
                                                               float* __restrict__ dlogits, float* __restrict__ scalars,
                                                               int* __restrict__ nonfinite) {
    dat_loss_single_body(logits, teacher, target, B, C, temp, dlogits, scalars, nonfinite);
}

// A short batch in the static B-sample frame: rows [n, B) of dlogits become 0.0f (they hold the previous step's gradient
// otherwise) and the loss runs on the n valid rows alone -- the same body with B = n, so rows [0, n) and the scalars carry the
// bits of the full kernel on the n-row views and rows >= n of logits / teacher / target are never read.
__device__ __forceinline__ void loss_zero_tail_rows(float* __restrict__ dlogits, int n, int B, int C) {
    const size_t end = (size_t)B * C;
    for (size_t i = (size_t)n * C + threadIdx.x; i < end; i += blockDim.x) dlogits[i] = 0.0f;
}

__global__ __launch_bounds__(1024) void dat_loss_rows_kernel(const float* __restrict__ logits,
                                                             const float* __restrict__ teacher,
                                                             const float* __restrict__ target, int n, int B, int C, float temp,
                                                             float* __restrict__ dlogits, float* __restrict__ scalars,
                                                             int* __restrict__ nonfinite) {
    loss_zero_tail_rows(dlogits, n, B, C);
    dat_loss_single_body(logits, teacher, target, n, C, temp, dlogits, scalars, nonfinite);
}

// DAT loss at ANY width (the reference's `vqa` task: num_labels = 3129, task_configs_fed.py; same formulas and outputs as
// dat_loss_single_body): one workgroup of 256 threads per row of the B-row frame, thread t takes columns t, t + 256, ...
// Rows [0, n) are the batch; a workgroup of a row in [n, B) writes its dlogits row as 0.0f and reads nothing.  Up to
// WIDE_REG_C = 256 * WIDE_NPT = 4096 columns the row's three operands are loaded once and stay in registers over the three
// passes (maxima; sums of exponentials; terms and dlogits): 3 * 16 = 48 operand VGPRs per lane, nothing spills; wider rows
// re-read their operands in every pass.  Every load is a dword (a row of 3129 floats starts 16-byte aligned only every fourth
// row); consecutive lanes read consecutive floats.  Reductions in a fixed order, no float atomics: wave_max / wave_sum, then the
// row's waves 0..3 in that order through LDS.  The row's two terms go to workspace[2 b], workspace[2 b + 1]; the batch sums
// are dat_loss_wide_finish_kernel, a second launch.
constexpr int WIDE_T = 256;
constexpr int WIDE_NPT = 16;
constexpr int WIDE_REG_C = WIDE_T * WIDE_NPT;

__device__ __forceinline__ void wide_row_max2(float& a, float& b, float (*part)[4]) {
    a = wave_max(a);
    b = wave_max(b);
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = a;
        part[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = fmaxf(fmaxf(fmaxf(part[0][0], part[0][1]), part[0][2]), part[0][3]);
    b = fmaxf(fmaxf(fmaxf(part[1][0], part[1][1]), part[1][2]), part[1][3]);
}

__device__ __forceinline__ void wide_row_sum2(float& a, float& b, float (*part)[4]) {
    a = wave_sum(a);
    b = wave_sum(b);
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = a;
        part[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
    b = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
}

// one element's BCE and KL terms and its dlogits (the arithmetic of dat_loss_single_body, element by element)
__device__ __forceinline__ float wide_elem(float x, float t, float y, float it, float temp, float lsx, float lst, float gs,
                                           float& bce, float& kl) {
    bce += fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
    const float logp = x * it - lsx;
    const float logq = t * it - lst;
    const float q = expf(logq);
    kl += q * (logq - logp);
    const float sig = 1.0f / (1.0f + expf(-x));
    return gs * ((sig - y) + temp * (expf(logp) - q));
}

template <bool REG>
__global__ __launch_bounds__(WIDE_T) void dat_loss_wide_kernel(const float* __restrict__ logits,
                                                               const float* __restrict__ teacher,
                                                               const float* __restrict__ target, int n, int C, float temp,
                                                               float* __restrict__ dlogits, float* __restrict__ row_terms) {
    __shared__ float part[3][2][4];       // one slot per pass: one barrier per pass
    const int b = blockIdx.x, tid = threadIdx.x;
    float* __restrict__ dl = dlogits + (size_t)b * C;
    if (b >= n) {       // a replica row of a short batch: zero gradient, its inputs are never read
        for (int j = tid; j < C; j += WIDE_T) dl[j] = 0.0f;
        return;
    }
    const float* __restrict__ x = logits + (size_t)b * C;
    const float* __restrict__ t = teacher + (size_t)b * C;
    const float* __restrict__ y = target + (size_t)b * C;
    const float it = 1.0f / temp, gs = 0.5f / (float)n;
    float mx = -INFINITY, mt = -INFINITY, sx = 0.f, st = 0.f, bce = 0.f, kl = 0.f;
    if (REG) {
        float xv[WIDE_NPT], tv[WIDE_NPT], yv[WIDE_NPT];
#pragma unroll
        for (int k = 0; k < WIDE_NPT; ++k) {
            const int j = tid + WIDE_T * k;
            const bool ok = j < C;
            xv[k] = ok ? x[j] : 0.f;
            tv[k] = ok ? t[j] : 0.f;
            yv[k] = ok ? y[j] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < WIDE_NPT; ++k) {
            if (tid + WIDE_T * k < C) {
                mx = fmaxf(mx, xv[k] * it);
                mt = fmaxf(mt, tv[k] * it);
            }
        }
        wide_row_max2(mx, mt, part[0]);
#pragma unroll
        for (int k = 0; k < WIDE_NPT; ++k) {
            if (tid + WIDE_T * k < C) {
                sx += expf(xv[k] * it - mx);
                st += expf(tv[k] * it - mt);
            }
        }
        wide_row_sum2(sx, st, part[1]);
        const float lsx = mx + logf(sx), lst = mt + logf(st);
#pragma unroll
        for (int k = 0; k < WIDE_NPT; ++k) {
            const int j = tid + WIDE_T * k;
            if (j < C) dl[j] = wide_elem(xv[k], tv[k], yv[k], it, temp, lsx, lst, gs, bce, kl);
        }
    } else {
        for (int j = tid; j < C; j += WIDE_T) {
            mx = fmaxf(mx, x[j] * it);
            mt = fmaxf(mt, t[j] * it);
        }
        wide_row_max2(mx, mt, part[0]);
        for (int j = tid; j < C; j += WIDE_T) {
            sx += expf(x[j] * it - mx);
            st += expf(t[j] * it - mt);
        }
        wide_row_sum2(sx, st, part[1]);
        const float lsx = mx + logf(sx), lst = mt + logf(st);
        for (int j = tid; j < C; j += WIDE_T) dl[j] = wide_elem(x[j], t[j], y[j], it, temp, lsx, lst, gs, bce, kl);
    }
    wide_row_sum2(bce, kl, part[2]);
    if (tid == 0) {
        row_terms[2 * b] = bce;
        row_terms[2 * b + 1] = kl;
    }
}

// The batch sums of the wide loss, one wave, in the order of dat_loss_finish (loss_optim.hip): lane b % 64 adds its rows in row
// order, then wave_sum; + GradScaler's inf check of the loss.  A launch of its own on purpose: the hand-off from the row
// workgroups is the kernel boundary, not a fence and a ticket across XCDs.
__global__ __launch_bounds__(64) void dat_loss_wide_finish_kernel(const float* __restrict__ row_terms, int n, float temp,
                                                                  float* __restrict__ scalars, int* __restrict__ nonfinite) {
    float bce = 0.f, kl = 0.f;
    for (int b = threadIdx.x; b < n; b += 64) {
        bce += row_terms[2 * b];
        kl += row_terms[2 * b + 1];
    }
    bce = wave_sum(bce);
    kl = wave_sum(kl);
    if (threadIdx.x == 0) {
        const float l_bce = bce / (float)n;
        const float l_kl = kl / (float)n * temp * temp;
        scalars[0] = l_bce;
        scalars[1] = l_kl;
        scalars[2] = 0.5f * (l_bce + l_kl);
        if (nonfinite && fd_nonfinite(l_bce + l_kl)) atomicOr(nonfinite, 1);
    }
}

// Single-adapter step loss (optimizer_mode adapter; task_trainer.py:433-441): L = BCEWithLogits_mean(logits, target) * C and
// dL/dlogits = (sigmoid(x) - t) / B in ONE launch.  Any C: lane j of a wave takes columns j, j + 64, ...; for C <= 128 a row's
// terms are added in dat_loss_single_kernel's order and its batch sum is the same, so scalars[0] carries the same bits as
// that kernel's BCE half.  Fixed-order reductions, no float atomics.
__device__ __forceinline__ void bce_loss_body(const float* __restrict__ logits, const float* __restrict__ target, int B, int C,
                                              float* __restrict__ dlogits, float* __restrict__ scalars,
                                              int* __restrict__ nonfinite) {
    extern __shared__ float terms[];       // [B]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_b = 1.0f / (float)B;
    for (int b = wave; b < B; b += 16) {
        float bce = 0.f;
        for (int j = lane; j < C; j += 64) {
            const float x = logits[(size_t)b * C + j];
            const float y = target[(size_t)b * C + j];
            bce += fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
            const float sig = 1.0f / (1.0f + expf(-x));
            dlogits[(size_t)b * C + j] = (sig - y) * inv_b;
        }
        bce = wave_sum(bce);
        if (lane == 0) terms[b] = bce;
    }
    __syncthreads();
    if (wave != 0) return;
    float bce = 0.f;
    for (int b = lane; b < B; b += 64) bce += terms[b];
    bce = wave_sum(bce);
    if (lane == 0) {
        const float l_bce = bce / (float)B;
        scalars[0] = l_bce;
        if (nonfinite && fd_nonfinite(l_bce)) atomicOr(nonfinite, 1);
    }
}

__global__ __launch_bounds__(1024) void bce_loss_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                        int B, int C, float* __restrict__ dlogits,
                                                        float* __restrict__ scalars, int* __restrict__ nonfinite) {
    bce_loss_body(logits, target, B, C, dlogits, scalars, nonfinite);
}

__global__ __launch_bounds__(1024) void bce_loss_rows_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                             int n, int B, int C, float* __restrict__ dlogits,
                                                             float* __restrict__ scalars, int* __restrict__ nonfinite) {
    loss_zero_tail_rows(dlogits, n, B, C);
    bce_loss_body(logits, target, n, C, dlogits, scalars, nonfinite);
}

__device__ __forceinline__ float ht_poly_lambda(int t, int warmup, int total) {     // = poly_lambda of loss_optim.hip
    if (t < warmup) return (float)t / (float)max(1, warmup);
    if (t > total) return 0.f;
    return 1.0f - (float)(t - warmup) / (float)(total - warmup);
}

struct AdamwMulti {
    feddat_adamw_group grp[FEDDAT_ADAMW_MAX_GROUPS];
    int block_end[FEDDAT_ADAMW_MAX_GROUPS];      // group k owns blocks [block_end[k-1], block_end[k])
    int ngroups;
    float base_lr, beta1, beta2, eps;
    int warmup, total;
};

// the weight decays of elements i .. i + 3 from the segment table (off / wdv: in LDS, or in global memory for a table too long for it)
__device__ __forceinline__ void adamw_quad_wd(const long* off, const float* wdv, const int nseg, const long i, float (&wd)[4]) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) wd[e] = wdv[lo];
    if (lo + 1 < nseg && off[lo + 1] < i + 4) {
        for (int e = 1; e < 4; ++e) {
            int s2 = lo;
            while (s2 + 1 < nseg && off[s2 + 1] <= i + e) ++s2;
            wd[e] = wdv[s2];
        }
    }
}

// adamw_flat_kernel<4>'s arithmetic (loss_optim.hip; bit-identical per element) for up to three parameter groups in one
// launch; a group reads its schedule index / Adam step count at (state[0] + d_sched, state[1] + d_adam).
// The stream (g, p, m, v: 16 of the 28 bytes a parameter moves) is asked for FIRST: the flags, the counters and the segment table
// are a chain of dependent reads that used to stand in front of it.  The loads are harmless on a skipped or restored block.
// The block then takes its group's segment table into LDS once (every lane searched it in global memory: ~log2(nseg) dependent
// round trips) and thread 0 evaluates the two bias corrections for the block -- the same powf calls on the same arguments.
constexpr int ADAMW_SEG_LDS = 1024;      // a longer table is searched in global memory as before
__global__ __launch_bounds__(256) void adamw_multi_kernel(const AdamwMulti a) {
    __shared__ long s_off[ADAMW_SEG_LDS];
    __shared__ float s_wd[ADAMW_SEG_LDS];
    __shared__ float s_bc[2];
    int k = 0;
    while (k + 1 < a.ngroups && (int)blockIdx.x >= a.block_end[k]) ++k;
    const feddat_adamw_group& G = a.grp[k];
    const int blk = (int)blockIdx.x - (k ? a.block_end[k - 1] : 0);
    const long i = ((long)blk * 256 + threadIdx.x) * 4;
    const bool live = i < G.n;
    f32x4 gi = {0.f, 0.f, 0.f, 0.f}, pi = gi, mi = gi, vi = gi;
    if (live) {
        gi = *reinterpret_cast<const f32x4*>(G.g + i);
        pi = *reinterpret_cast<const f32x4*>(G.p + i);
        mi = *reinterpret_cast<const f32x4*>(G.m + i);
        vi = *reinterpret_cast<const f32x4*>(G.v + i);
    }
    // dynamic loss scale (ABI 8): restore / skip decisions are block-uniform device flags (head_tail.hip)
    if (G.bak_mode == 2 && G.restore_if && *G.restore_if) {
        if (live) {
            *reinterpret_cast<f32x4*>(G.p + i) = *reinterpret_cast<const f32x4*>(G.bak + i);
            *reinterpret_cast<f32x4*>(G.m + i) = *reinterpret_cast<const f32x4*>(G.bak + G.n + i);
            *reinterpret_cast<f32x4*>(G.v + i) = *reinterpret_cast<const f32x4*>(G.bak + 2 * G.n + i);
        }
        return;
    }
    const bool skip = (G.skip_if[0] && *G.skip_if[0]) || (G.skip_if[1] && *G.skip_if[1]);
    if (skip && G.bak_mode != 1) return;
    const int sched_t = G.state[0] + G.d_sched;
    const int t = G.state[1] + G.d_adam + 1;
    const float lr = a.base_lr * ht_poly_lambda(sched_t, a.warmup, a.total);
    const bool table_in_lds = G.nseg <= ADAMW_SEG_LDS;
    if (table_in_lds)
        for (int s = threadIdx.x; s < G.nseg; s += 256) {
            s_off[s] = G.seg_off[s];
            s_wd[s] = G.seg_wd[s];
        }
    if (threadIdx.x == 0) {
        s_bc[0] = 1.0f - powf(a.beta1, (float)t);
        s_bc[1] = 1.0f - powf(a.beta2, (float)t);
    }
    __syncthreads();
    if (!live) return;
    float wd[4];
    if (table_in_lds) adamw_quad_wd(s_off, s_wd, G.nseg, i, wd);
    else adamw_quad_wd(G.seg_off, G.seg_wd, G.nseg, i, wd);
    const float bc1 = s_bc[0], bc2 = s_bc[1];
    if (G.bak_mode == 1) {
        *reinterpret_cast<f32x4*>(G.bak + i) = pi;
        *reinterpret_cast<f32x4*>(G.bak + G.n + i) = mi;
        *reinterpret_cast<f32x4*>(G.bak + 2 * G.n + i) = vi;
        if (skip) return;
    }
    // adamw_flat_kernel's expressions (loss_optim.hip):
    //     p *= 1 - lr wd;   m += (g - m)(1 - beta1);   v = v beta2 + (1 - beta2) g g;   p -= (lr / bc1)(m / (sqrt v / sqrt bc2 + eps))
    // with the multiply-adds hipcc fused in this kernel spelled out.  Left to the compiler the fusions change with the code around
    // the expressions (they did when the loads moved in front of the table search: half of the v updates came out unfused), and
    // the trained weights with them.
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma clang fp contract(off)
        const float keep = __builtin_fmaf(-lr, wd[e], 1.0f);
        mi[e] = __builtin_fmaf(gi[e] - mi[e], 1.0f - a.beta1, mi[e]);
        vi[e] = __builtin_fmaf(vi[e], a.beta2, (1.0f - a.beta2) * gi[e] * gi[e]);
        const float denom = sqrtf(vi[e]) / sqrtf(bc2) + a.eps;
        pi[e] = __builtin_fmaf(pi[e], keep, -((lr / bc1) * (mi[e] / denom)));
    }
    *reinterpret_cast<f32x4*>(G.p + i) = pi;
    *reinterpret_cast<f32x4*>(G.m + i) = mi;
    *reinterpret_cast<f32x4*>(G.v + i) = vi;
}

struct TickMulti {
    int* state[FEDDAT_ADAMW_MAX_GROUPS];
    int d_sched[FEDDAT_ADAMW_MAX_GROUPS], d_adam[FEDDAT_ADAMW_MAX_GROUPS];
    int n;
};
__global__ void step_tick_multi_kernel(const TickMulti t) {
    const int k = threadIdx.x;
    if (blockIdx.x == 0 && k < t.n) {
        t.state[k][0] += t.d_sched[k];
        t.state[k][1] += t.d_adam[k];
    }
}

// End of one dat train_step under a dynamic loss scale: counter ticks by what was applied, GradScaler.update(), flags cleared
// (semantics: include/feddat_hip.h, feddat_dat_step_finish).
__global__ void dat_step_finish_kernel(int* head_state, int* ad1_state, int* ad0_state, int* flags, float* scaler_f,
                                       int* scaler_i, float growth, float backoff, int growth_interval) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int fB = flags[0], fA = flags[1];
    const int applied = fA ? 0 : fB ? 1 : 2;
    head_state[0] += applied;
    head_state[1] += applied;
    ad1_state[0] += applied;
    ad1_state[1] += applied >= 1 ? 1 : 0;
    ad0_state[0] += applied;
    ad0_state[1] += applied == 2 ? 1 : 0;
    if (applied < 2) {
        scaler_i[1] += 2 - applied;
        scaler_i[2] += 1;
    }
    // GradScaler.update() once per backward, in the reference's order: sub-step A, then B
    float scale = scaler_f[0];
    int tracker = scaler_i[0];
    for (const int found_inf : {fA, fB}) {
        if (found_inf) {
            scale = fmaxf(scale * backoff, 6.103515625e-05f);
            tracker = 0;
        } else if (++tracker >= growth_interval) {
            scale = fminf(scale * growth, 1073741824.0f);
            tracker = 0;
        }
    }
    scaler_f[0] = scale;
    scaler_f[1] = 1.0f / scale;
    scaler_i[0] = tracker;
    flags[0] = 0;
    flags[1] = 0;
}

// End of one single-adapter train_step under a dynamic loss scale: every counter moves by what was applied (one optimizer step
// and one scheduler tick per batch), GradScaler.update() for one backward, flag cleared (include/feddat_hip.h).
struct SingleFinish {
    int* state[FEDDAT_ADAMW_MAX_GROUPS];
    int n;
};
__global__ void single_step_finish_kernel(const SingleFinish s, int* flag, float* scaler_f, int* scaler_i, float growth,
                                          float backoff, int growth_interval) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int applied = *flag ? 0 : 1;
    for (int k = 0; k < s.n; ++k) {
        s.state[k][0] += applied;
        s.state[k][1] += applied;
    }
    float scale = scaler_f[0];
    int tracker = scaler_i[0];
    if (!applied) {
        scale = fmaxf(scale * backoff, 6.103515625e-05f);
        tracker = 0;
        scaler_i[1] += 1;
        scaler_i[2] += 1;
    } else {
        tracker += 1;
        if (tracker >= growth_interval) {
            scale = fminf(scale * growth, 1073741824.0f);
            tracker = 0;
        }
    }
    scaler_f[0] = scale;
    scaler_f[1] = 1.0f / scale;
    scaler_i[0] = tracker;
    *flag = 0;
}

// Every decision feddat_head_gemm takes about one job, and every reason it refuses one: host arithmetic on the job's sizes,
// strides and pointer VALUES only (nothing is dereferenced, no device is touched), exported as feddat_head_gemm_plan and
// pinned on the CPU by tests/test_head_gemm_plan_cpu.py.  ht_fill below is its only other caller.
int ht_plan(const feddat_ht_job& s, feddat_ht_plan& p) {
    if (!(s.A && s.B && s.out && s.I > 0 && s.J > 0 && s.K > 0 && s.ldo >= s.J && (s.mode == 0 || s.mode == 1)))
        return FEDDAT_EINVAL;
    if (s.pro == FEDDAT_HT_PRO_LN && !(s.pro_a && s.pro_b && s.pro_eps > 0.f && s.sa_k == 1 && s.K % 4 == 0 && s.K <= 2048 &&
                                       s.sa_i % 4 == 0 && ((uintptr_t)s.A & 15) == 0))
        return FEDDAT_EINVAL;
    if (s.pro == FEDDAT_HT_PRO_TANH_BWD && !s.pro_a) return FEDDAT_EINVAL;
    if (s.epi == FEDDAT_HT_EPI_MUL_DGELU && !(s.aux && s.ld_aux >= s.J)) return FEDDAT_EINVAL;
    if (s.pro < 0 || s.pro > FEDDAT_HT_PRO_TANH_BWD || s.epi < 0 || s.epi > FEDDAT_HT_EPI_MUL_DGELU) return FEDDAT_EINVAL;
    p.avec = s.sa_k == 1 && s.K % 4 == 0 && s.sa_i % 4 == 0 && ((uintptr_t)s.A & 15) == 0 &&
             (s.pro != FEDDAT_HT_PRO_TANH_BWD || ((uintptr_t)s.pro_a & 15) == 0);
    p.bvec = s.sb_k == 1 && s.K % 4 == 0 && s.sb_j % 4 == 0 && ((uintptr_t)s.B & 15) == 0;
    if (s.pro == FEDDAT_HT_PRO_LN && !(p.avec && (((uintptr_t)s.pro_a | (uintptr_t)s.pro_b) & 15) == 0)) return FEDDAT_EINVAL;
    p.itiles = (s.I + 15) / 16;
    int jgroups = (s.J + 16 * HT_JT - 1) / (16 * HT_JT);
    p.jt = HT_JT;
    if (s.mode == 0 && p.itiles * jgroups < 64) {      // too few 16 x 64 tiles: 16 x 16 tiles, four times the blocks
        p.jt = 1;
        jgroups = (s.J + 15) / 16;
    }
    p.jblocks = s.mode == 0 ? jgroups : (jgroups + HT_NW - 1) / HT_NW;
    p.blocks = p.itiles * p.jblocks;
    return FEDDAT_OK;
}

int ht_fill(HtJob& j, const feddat_ht_job& s) {
    feddat_ht_plan p;
    const int rc = ht_plan(s, p);
    if (rc != FEDDAT_OK) return rc;
    j.A = s.A; j.sa_i = s.sa_i; j.sa_k = s.sa_k; j.B = s.B; j.sb_k = s.sb_k; j.sb_j = s.sb_j;
    j.I = s.I; j.J = s.J; j.K = s.K; j.mode = s.mode; j.alpha = s.alpha; j.alpha_dev = s.alpha_dev; j.bias_j = s.bias_j; j.out = s.out; j.ldo = s.ldo;
    j.colsum = s.colsum; j.pro = s.pro; j.pro_a = s.pro_a; j.pro_b = s.pro_b; j.pro_eps = s.pro_eps;
    j.stats_out = s.stats_out; j.epi = s.epi; j.aux = s.aux; j.ld_aux = s.ld_aux;
    j.avec = p.avec; j.bvec = p.bvec; j.jt = p.jt; j.itiles = p.itiles; j.jblocks = p.jblocks;
    return FEDDAT_OK;
}

}  // namespace

extern "C" int feddat_head_gemm(const feddat_ht_job* jobs, int njobs, hipStream_t stream) {
    FD_CHECK_ARG(jobs && (njobs == 1 || njobs == 2));
    HtLaunch L{};
    int total = 0;
    for (int k = 0; k < njobs; ++k) {
        const int rc = ht_fill(L.job[k], jobs[k]);
        if (rc != FEDDAT_OK) return rc;
        const int nb = L.job[k].itiles * L.job[k].jblocks;
        if (k == 0) L.blocks0 = nb;
        total += nb;
    }
    constexpr int lds = ((HT_NW - 1) * 64 * (HT_JT * 4 + 4) + 32) * (int)sizeof(float);
    if (fd_set_max_lds((const void*)ht_gemm_kernel, lds) != FEDDAT_OK) return FEDDAT_ELAUNCH;
    hipLaunchKernelGGL(ht_gemm_kernel, dim3(total), dim3(HT_NW * 64), lds, stream, L);
    FD_LAUNCH_RET();
}

extern "C" int feddat_head_gemm_plan(const feddat_ht_job* job, feddat_ht_plan* out) {
    FD_CHECK_ARG(job && out);
    return ht_plan(*job, *out);
}

extern "C" int feddat_head_ln_gelu(const float* x, const float* gamma, const float* beta, float eps, int rows, int H,
                                   float* y, float* stats, float* gelu_out, hipStream_t stream) {
    FD_CHECK_ARG(x && gamma && beta && y && stats && gelu_out && rows > 0 && H > 0 && H % 4 == 0 && H <= 2048 && eps > 0.f);
    hipLaunchKernelGGL(ht_ln_gelu_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, x, gamma, beta, eps, rows, H, y, stats,
                       gelu_out);
    FD_LAUNCH_RET();
}

extern "C" int feddat_head_ln_bwd_full(const float* dy, const float* x, const float* stats, const float* gamma, int rows,
                                       int H, float* dx, float* dgamma, float* dbeta, hipStream_t stream) {
    FD_CHECK_ARG(dy && x && stats && gamma && dx && dgamma && dbeta && rows > 0 && rows <= 4096 && H > 0 && H % 4 == 0 &&
                 H <= 2048);
    hipLaunchKernelGGL(ht_ln_bwd_full_kernel, dim3((rows + 3) / 4 + (H + 63) / 64), dim3(256), 0, stream, dy, x, stats, gamma,
                       rows, H, dx, dgamma, dbeta);
    FD_LAUNCH_RET();
}

extern "C" int feddat_dat_loss_fwd_bwd_single(const float* logits, const float* teacher, const float* target, int B, int C,
                                              float temp, float* dlogits, float* scalars, hipStream_t stream) {
    FD_CHECK_ARG(logits && teacher && target && dlogits && scalars && B > 0 && B <= 4096 && C > 0 && C <= 128 && temp > 0.f);
    hipLaunchKernelGGL(dat_loss_single_kernel, dim3(1), dim3(1024), 2 * B * sizeof(float), stream, logits, teacher, target, B,
                       C, temp, dlogits, scalars, (int*)nullptr);
    FD_LAUNCH_RET();
}

extern "C" int feddat_dat_loss_fwd_bwd_checked(const float* logits, const float* teacher, const float* target, int B, int C,
                                               float temp, float* dlogits, float* scalars, int* nonfinite, hipStream_t stream) {
    FD_CHECK_ARG(logits && teacher && target && dlogits && scalars && B > 0 && B <= 4096 && C > 0 && C <= 128 && temp > 0.f);
    hipLaunchKernelGGL(dat_loss_single_kernel, dim3(1), dim3(1024), 2 * B * sizeof(float), stream, logits, teacher, target, B,
                       C, temp, dlogits, scalars, nonfinite);
    FD_LAUNCH_RET();
}

extern "C" int feddat_dat_loss_fwd_bwd_rows(const float* logits, const float* teacher, const float* target, int n, int B, int C,
                                            float temp, float* dlogits, float* scalars, int* nonfinite, hipStream_t stream) {
    FD_CHECK_ARG(logits && teacher && target && dlogits && scalars && n > 0 && n <= B && B <= 4096 && C > 0 && C <= 128 &&
                 temp > 0.f);
    hipLaunchKernelGGL(dat_loss_rows_kernel, dim3(1), dim3(1024), 2 * n * sizeof(float), stream, logits, teacher, target, n, B,
                       C, temp, dlogits, scalars, nonfinite);
    FD_LAUNCH_RET();
}

extern "C" long feddat_dat_loss_wide_workspace_elems(int B) { return B > 0 ? 2L * B : 0L; }

extern "C" int feddat_dat_loss_fwd_bwd_wide(const float* logits, const float* teacher, const float* target, int n, int B, int C,
                                            float temp, float* dlogits, float* scalars, int* nonfinite, float* workspace,
                                            long workspace_elems, hipStream_t stream) {
    FD_CHECK_ARG(logits && teacher && target && dlogits && scalars && workspace && n > 0 && n <= B && B <= 4096 && C > 0 &&
                 temp > 0.f && workspace_elems >= feddat_dat_loss_wide_workspace_elems(B));
    if (C <= WIDE_REG_C)
        hipLaunchKernelGGL(dat_loss_wide_kernel<true>, dim3(B), dim3(WIDE_T), 0, stream, logits, teacher, target, n, C, temp,
                           dlogits, workspace);
    else
        hipLaunchKernelGGL(dat_loss_wide_kernel<false>, dim3(B), dim3(WIDE_T), 0, stream, logits, teacher, target, n, C, temp,
                           dlogits, workspace);
    hipLaunchKernelGGL(dat_loss_wide_finish_kernel, dim3(1), dim3(64), 0, stream, workspace, n, temp, scalars, nonfinite);
    FD_LAUNCH_RET();
}

extern "C" int feddat_dat_step_finish(int* head_state, int* ad1_state, int* ad0_state, int* flags, float* scaler_f,
                                      int* scaler_i, float growth, float backoff, int growth_interval, hipStream_t stream) {
    FD_CHECK_ARG(head_state && ad1_state && ad0_state && flags && scaler_f && scaler_i && growth >= 1.0f && backoff > 0.f &&
                 backoff <= 1.0f && growth_interval > 0);
    hipLaunchKernelGGL(dat_step_finish_kernel, dim3(1), dim3(64), 0, stream, head_state, ad1_state, ad0_state, flags, scaler_f,
                       scaler_i, growth, backoff, growth_interval);
    FD_LAUNCH_RET();
}

extern "C" int feddat_adamw_multi(const feddat_adamw_group* groups, int ngroups, float base_lr, int warmup, int total,
                                  float beta1, float beta2, float eps, hipStream_t stream) {
    FD_CHECK_ARG(groups && ngroups >= 1 && ngroups <= FEDDAT_ADAMW_MAX_GROUPS && total > warmup);
    AdamwMulti a{};
    int blocks = 0;
    for (int k = 0; k < ngroups; ++k) {
        const feddat_adamw_group& G = groups[k];
        FD_CHECK_ARG(G.p && G.g && G.m && G.v && G.n > 0 && G.n % 4 == 0 && G.seg_off && G.seg_wd && G.nseg > 0 && G.state);
        FD_CHECK_ARG((((uintptr_t)G.p | (uintptr_t)G.g | (uintptr_t)G.m | (uintptr_t)G.v) & 15) == 0);
        FD_CHECK_ARG(G.bak_mode >= 0 && G.bak_mode <= 2 && (G.bak_mode == 0 || (G.bak && ((uintptr_t)G.bak & 15) == 0)) &&
                     (G.bak_mode != 2 || G.restore_if));
        a.grp[k] = G;
        blocks += (int)((G.n / 4 + 255) / 256);
        a.block_end[k] = blocks;
    }
    a.ngroups = ngroups;
    a.base_lr = base_lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.warmup = warmup; a.total = total;
    hipLaunchKernelGGL(adamw_multi_kernel, dim3(blocks), dim3(256), 0, stream, a);
    FD_LAUNCH_RET();
}

extern "C" int feddat_step_tick_multi(int* const* states, const int* d_sched, const int* d_adam, int n, hipStream_t stream) {
    FD_CHECK_ARG(states && d_sched && d_adam && n >= 1 && n <= FEDDAT_ADAMW_MAX_GROUPS);
    TickMulti t{};
    for (int k = 0; k < n; ++k) {
        FD_CHECK_ARG(states[k]);
        t.state[k] = states[k];
        t.d_sched[k] = d_sched[k];
        t.d_adam[k] = d_adam[k];
    }
    t.n = n;
    hipLaunchKernelGGL(step_tick_multi_kernel, dim3(1), dim3(64), 0, stream, t);
    FD_LAUNCH_RET();
}

extern "C" int feddat_bce_loss_fwd_bwd(const float* logits, const float* target, int B, int C, float* dlogits, float* scalars,
                                       int* nonfinite, hipStream_t stream) {
    FD_CHECK_ARG(logits && target && dlogits && scalars && B > 0 && B <= 4096 && C > 0);
    hipLaunchKernelGGL(bce_loss_kernel, dim3(1), dim3(1024), B * sizeof(float), stream, logits, target, B, C, dlogits, scalars,
                       nonfinite);
    FD_LAUNCH_RET();
}

extern "C" int feddat_bce_loss_fwd_bwd_rows(const float* logits, const float* target, int n, int B, int C, float* dlogits,
                                            float* scalars, int* nonfinite, hipStream_t stream) {
    FD_CHECK_ARG(logits && target && dlogits && scalars && n > 0 && n <= B && B <= 4096 && C > 0);
    hipLaunchKernelGGL(bce_loss_rows_kernel, dim3(1), dim3(1024), n * sizeof(float), stream, logits, target, n, B, C, dlogits,
                       scalars, nonfinite);
    FD_LAUNCH_RET();
}

extern "C" int feddat_single_step_finish(int* const* states, int n, int* flag, float* scaler_f, int* scaler_i, float growth,
                                         float backoff, int growth_interval, hipStream_t stream) {
    FD_CHECK_ARG(states && n >= 1 && n <= FEDDAT_ADAMW_MAX_GROUPS && flag && scaler_f && scaler_i && growth >= 1.0f &&
                 backoff > 0.f && backoff <= 1.0f && growth_interval > 0);
    SingleFinish s{};
    for (int k = 0; k < n; ++k) {
        FD_CHECK_ARG(states[k]);
        s.state[k] = states[k];
    }
    s.n = n;
    hipLaunchKernelGGL(single_step_finish_kernel, dim3(1), dim3(64), 0, stream, s, flag, scaler_f, scaler_i, growth, backoff,
                       growth_interval);
    FD_LAUNCH_RET();
}
