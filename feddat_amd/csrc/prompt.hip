// Prompt tuning (optimizer_mode prompt): the two row movers around the frozen ViLT backbone.  The reference inserts the five rows
// P = prompt_embedding_text(arange(5)) behind row 0 of the text embeddings AND behind row 0 (the CLS row) of the image embeddings;
// the token-type embeddings are added afterwards, to the prompt rows too.  With Lt text tokens and Np patch positions the
// unprompted frame has S0 = Lt + 1 + Np rows per sample, the prompted one S = S0 + 10:
//
//   row s of the prompted frame      content
//   0                                source row 0                 (text token 0: what the pooler reads)
//   1 .. 5                           P[s - 1] + modality[0]
//   6 .. Lt + 4                      source row s - 5             (text tokens 1 .. Lt - 1)
//   Lt + 5                           source row Lt                (image CLS)
//   Lt + 6 .. Lt + 10                P[s - Lt - 6] + modality[1]
//   Lt + 11 .. S - 1                 source row s - 10            (patches)
//
//   assemble   one wave per output row (4 rows per block): the wave computes its source row ONCE (wave-uniform, no per-element
//              row arithmetic), then moves the row with 16-byte loads and stores, H / 4 float4 over 64 lanes; lane 0 writes the
//              row's key-mask byte(s).  One pass: every output element is written exactly once, nothing else is touched.
//   gather     G[j, :] = sum_b (dh0[b, 1 + j, :] + dh0[b, Lt + 6 + j, :]): one thread per float4 of G, b ascending, text row before
//              image row, fp32 registers, no atomics on floats -- equal inputs give equal bits.  Reads the 10 B prompt rows only.
//              The sum leaves times unscale * (*unscale_dev) (the two-factor form of feddat_vector_grad_reduce) and an inf / NaN
//              ORs 1 into the overflow flag (an integer atomic).
//
// Both are graph-capturable: no host reads, no allocation.
#include "common.hip.h"
#include "../../include/feddat_hip_prompt.h"

namespace {

constexpr int PR_NP = 5;            // prompt rows per insertion point (the reference's prompt_tokens = arange(5))
constexpr int PR_ROWS_PER_BLOCK = 4;

// Source of row s of the prompted frame: >= 0 a row of the unprompted frame; < 0: prompt row -(v + 1) (0..4 text side: modality 0,
// 5..9 image side: modality 1).
__device__ __forceinline__ int pr_source_row(int s, int Lt) {
    if (s == 0) return 0;
    if (s <= PR_NP) return -s;                                     // prompt j = s - 1, text side
    if (s <= Lt + PR_NP) return s - PR_NP;                         // text tokens 1 .. Lt - 1 and the image CLS (source row Lt)
    if (s <= Lt + 2 * PR_NP) return -(s - Lt - PR_NP - 1 + PR_NP) - 1;      // prompt j = s - Lt - 6, image side
    return s - 2 * PR_NP;
}

__global__ __launch_bounds__(64 * PR_ROWS_PER_BLOCK) void prompt_assemble_kernel(
    const float* __restrict__ h_in, const unsigned char* __restrict__ mask_in, const float* __restrict__ P,
    const float* __restrict__ mod0, const float* __restrict__ mod1, float* __restrict__ h_out,
    unsigned char* __restrict__ mask_out, int B, int Lt, int S0, int H, int nrep) {
    const int S = S0 + 2 * PR_NP;
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * PR_ROWS_PER_BLOCK + (threadIdx.x >> 6);      // wave-uniform
    if (row >= (long)B * S) return;
    const int b = (int)(row / S), s = (int)(row - (long)b * S);
    const int src = pr_source_row(s, Lt);
    f32x4* __restrict__ out = reinterpret_cast<f32x4*>(h_out + row * H);
    const int nq = H >> 2;
    unsigned char m = 1;
    if (src >= 0) {
        const f32x4* __restrict__ in = reinterpret_cast<const f32x4*>(h_in + ((long)b * S0 + src) * H);
        for (int q = lane; q < nq; q += 64) out[q] = in[q];
        if (mask_out && lane == 0) m = mask_in[(long)b * S0 + src];
    } else {
        const int pj = -src - 1;
        const f32x4* __restrict__ p = reinterpret_cast<const f32x4*>(P + (long)(pj % PR_NP) * H);
        const f32x4* __restrict__ md = reinterpret_cast<const f32x4*>(pj < PR_NP ? mod0 : mod1);
        for (int q = lane; q < nq; q += 64) out[q] = p[q] + md[q];
    }
    if (mask_out && lane == 0)
        for (int rep = 0; rep < nrep; ++rep) mask_out[((long)rep * B + b) * S + s] = m;
}

__global__ __launch_bounds__(64) void prompt_gather_kernel(const float* __restrict__ dh0, int B, int S, int Lt, int H,
                                                           float unscale, const float* __restrict__ unscale_dev,
                                                           float* __restrict__ G, int* __restrict__ nonfinite) {
    const int nq = H >> 2;
    const int t = blockIdx.x * 64 + threadIdx.x;
    bool bad = false;
    if (t < PR_NP * nq) {
        const int j = t / nq, q = t - j * nq;
        const f32x4* __restrict__ text = reinterpret_cast<const f32x4*>(dh0 + (long)(1 + j) * H) + q;
        const f32x4* __restrict__ img = reinterpret_cast<const f32x4*>(dh0 + (long)(Lt + PR_NP + 1 + j) * H) + q;
        const long sq = (long)S * nq;      // float4 per sample
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        int b = 0;
        for (; b + 4 <= B; b += 4) {      // eight loads in flight, summed in the fixed order b ascending, text before image
            f32x4 a[4], c[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a[k] = text[(b + k) * sq];
                c[k] = img[(b + k) * sq];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc += a[k];
                acc += c[k];
            }
        }
        for (; b < B; ++b) {
            acc += text[b * sq];
            acc += img[b * sq];
        }
        const float us = unscale_dev ? unscale * *unscale_dev : unscale;
        acc *= us;
        reinterpret_cast<f32x4*>(G)[t] = acc;
        bad = fd_nonfinite(acc[0]) || fd_nonfinite(acc[1]) || fd_nonfinite(acc[2]) || fd_nonfinite(acc[3]);
    }
    if (nonfinite && __ballot(bad) != 0 && threadIdx.x == 0) atomicOr(nonfinite, 1);
}

inline bool pr_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int feddat_prompt_frame_assemble(const float* h_in, const uint8_t* key_mask_in, const float* P, const float* modality0,
                                            const float* modality1, float* h_out, uint8_t* key_mask_out, int B, int Lt, int Np,
                                            int H, int nrep, hipStream_t stream) {
    FD_CHECK_ARG(h_in && P && modality0 && modality1 && h_out && B > 0 && Lt > 0 && Np > 0 && H > 0 && H % 4 == 0);
    FD_CHECK_ARG((key_mask_out == nullptr) || (key_mask_in != nullptr && nrep >= 1));
    FD_CHECK_ARG(h_in != h_out && pr_aligned16(h_in) && pr_aligned16(P) && pr_aligned16(modality0) && pr_aligned16(modality1) &&
                 pr_aligned16(h_out));
    const int S0 = Lt + 1 + Np;
    const long rows = (long)B * (S0 + 2 * PR_NP);
    const long blocks = (rows + PR_ROWS_PER_BLOCK - 1) / PR_ROWS_PER_BLOCK;
    FD_CHECK_ARG(blocks <= 0x7fffffffL);
    hipLaunchKernelGGL(prompt_assemble_kernel, dim3((unsigned)blocks), dim3(64 * PR_ROWS_PER_BLOCK), 0, stream, h_in,
                       key_mask_in, P, modality0, modality1, h_out, key_mask_out, B, Lt, S0, H, nrep);
    FD_LAUNCH_RET();
}

extern "C" int feddat_prompt_grad_gather(const float* dh0, int B, int S, int Lt, int H, float unscale, const float* unscale_dev,
                                         float* G, int* nonfinite, hipStream_t stream) {
    FD_CHECK_ARG(dh0 && G && B > 0 && Lt > 0 && S >= Lt + 2 * PR_NP + 2 && H > 0 && H % 4 == 0);
    FD_CHECK_ARG(pr_aligned16(dh0) && pr_aligned16(G));
    const int threads = PR_NP * (H / 4);
    hipLaunchKernelGGL(prompt_gather_kernel, dim3((threads + 63) / 64), dim3(64), 0, stream, dh0, B, S, Lt, H,
                       unscale == 0.f ? 1.f : unscale, unscale_dev, G, nonfinite);
    FD_LAUNCH_RET();
}
