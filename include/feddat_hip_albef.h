/* libfeddat_hip.so -- the ALBEF single-adapter (FedAvg baseline) entry point of the C ABI (gfx950 only), an extension header of
 * include/feddat_hip.h.
 *
 * The same library, the same ABI version and the same conventions as feddat_hip.h (device pointers, asynchronous launches on
 * `stream`, FEDDAT_OK / FEDDAT_EINVAL / FEDDAT_ELAUNCH); both operand builds export this symbol.  It is declared here and
 * bound by its own table in feddat_amd/lib.py (ALBEF_SYMBOLS), beside the 115 entry points of feddat_hip.h and the two of
 * feddat_hip_prompt.h: additive within ABI 8.
 */
#ifndef FEDDAT_HIP_ALBEF_H
#define FEDDAT_HIP_ALBEF_H

#include "feddat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The LM loss without a teacher (optimizer_mode adapter on ALBEF: the non-dat branch of the reference's train_step returns
 * ALBEF.forward's weighted LM loss alone, no KL and no factor 1/2), csrc/albef_misc.hip.  The kernel is
 * feddat_lm_loss_fwd_bwd_dyn's, instantiated without its teacher loads.
 *   L = sum_r row_weight[r] * ce_r,   ce_r = logsumexp(logits[r, :V]) - logits[r, labels[r]]   (0 where labels[r] < 0)
 *   scalars (4 + 2 R floats): [0] = [2] = L, [1] = 0, scalars[4 + 2 r] = row_weight[r] * ce_r, scalars[5 + 2 r] = 0
 *   dlogits (16-bit operand format, row stride ldd, may be NULL) = grad_scale * (*grad_scale_dev when given) * dL/dlogits,
 *   zeros in the columns [V, ldd)
 *   *nonfinite (DEVICE int, may be NULL) is OR-ed with 1 when L is inf / NaN.
 * Bit for bit the dlogits, scalars[0] and row terms of feddat_lm_loss_fwd_bwd_dyn(teacher = NULL, kl_scale = 0, twice the
 * grad_scale).  Argument checks as there: logits 16-byte aligned, ldl % 4 == 0, ldl >= V, dlogits 8-byte aligned, ldd % 4 == 0,
 * ldd >= V, grad_scale > 0; FEDDAT_EINVAL writes nothing. */
int feddat_lm_ce_loss_fwd_bwd(const float* logits, long ldl, const long* labels, const float* row_weight, int R, int V,
                              float grad_scale, const float* grad_scale_dev, int* nonfinite, void* dlogits_bf16, long ldd,
                              float* scalars, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDDAT_HIP_ALBEF_H */
