/* libfeddat_hip.so -- the prompt-tuning entry points of the C ABI (gfx950 only), an extension header of include/feddat_hip.h.
 *
 * The same library, the same ABI version and the same conventions as feddat_hip.h (device pointers, asynchronous launches on
 * `stream`, FEDDAT_OK / FEDDAT_EINVAL / FEDDAT_ELAUNCH); both operand builds export these symbols.  They are declared here and
 * bound by their own table in feddat_amd/lib.py (PROMPT_SYMBOLS), beside the 115 entry points of feddat_hip.h.
 */
#ifndef FEDDAT_HIP_PROMPT_H
#define FEDDAT_HIP_PROMPT_H

#include "feddat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Prompt tuning (optimizer_mode prompt), csrc/prompt.hip.  The reference inserts the five rows
 * P = prompt_embedding_text(arange(5)) behind row 0 of the text embeddings and behind row 0 (CLS) of the image embeddings, then
 * adds the token-type embeddings.  The unprompted frame has S0 = Lt + 1 + Np rows per sample, the prompted one S = S0 + 10:
 * row 0 = source row 0; rows 1..5 = P[j] + modality0; rows 6..Lt+4 = source rows 1..Lt-1; row Lt+5 = source row Lt (CLS);
 * rows Lt+6..Lt+10 = P[j] + modality1; rows Lt+11..S-1 = source rows Lt+1..S0-1.  All fp32, no float atomics, no host reads.
 * feddat_prompt_frame_assemble: h_in [B, S0, H] (complete embeddings: positions, text LayerNorm, token types) -> h_out
 *   [B, S, H]; source rows are copied bit for bit, prompt rows are one fp32 add.  key_mask_out (uint8 [nrep * B, S], optional):
 *   the bytes of key_mask_in (uint8, row stride S0, its first B rows) at the source rows, 1 at the prompt rows, written nrep times
 *   (rows b + rep * B).  H % 4 == 0, 16-byte aligned fp32 pointers, h_in != h_out.
 * feddat_prompt_grad_gather: G[j, :] = (sum over b ascending of dh0[b, 1 + j, :] then dh0[b, Lt + 6 + j, :]) * unscale *
 *   (*unscale_dev when given: 1 / the dynamic loss scale), j < 5; dh0 fp32 [B, S, H], G fp32 [5, H].  Reads those 10 B rows only.
 *   *nonfinite (DEVICE int, may be NULL) is OR-ed with 1 when a written value is inf / NaN.  unscale 0 = 1.  S >= Lt + 12. */
int feddat_prompt_frame_assemble(const float* h_in, const uint8_t* key_mask_in, const float* P, const float* modality0,
                                 const float* modality1, float* h_out, uint8_t* key_mask_out, int B, int Lt, int Np, int H,
                                 int nrep, hipStream_t stream);
int feddat_prompt_grad_gather(const float* dh0, int B, int S, int Lt, int H, float unscale, const float* unscale_dev, float* G,
                              int* nonfinite, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDDAT_HIP_PROMPT_H */
