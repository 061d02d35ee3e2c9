/* psgd_kron_quad_x3_hip.h -- C ABI of the QUAD Kronecker update with its products on the bf16 matrix cores at fp32 grade
 * ("bf16 x 3"), psgd_kron_quad_x3.hip, in libpsgd_hip.so.
 *
 * The definition, the operands, the state (Ql, Qr symmetric fp32, L = [Ll, Lr]) and every convention are those of
 * psgd_kron_quad_hip.h; the three entry points below take the arguments of their namesakes there, return the same error codes
 * from the same checks (null, shape and aliasing checks and the workspace check return before any HIP call), and need a workspace
 * of the same size and layout.  State written by one route is read by the other: a run may switch between them at any step.
 * An update is 6 launches, an apply 4; the host reads nothing; no atomics, every partial has one writer and every fold a fixed
 * order: repeated calls are bit-identical.  The stored Q is exactly symmetric.  Any M, N >= 1; no alignment demand beyond 4 bytes,
 * and a call on a skewed base produces the bits of the aligned one.
 *
 * What differs is the arithmetic of the PRODUCTS (W = Ql G, A = W Qr, Tl, Tr, T Q, P1 T and the four of the apply).  Every fp32
 * operand element is split exactly into three bf16 terms x = h + m + l (truncating, 8 + 8 + 8 significant bits) on the way into
 * LDS, and a product is accumulated in fp32 as  m m' + h l' + l h' + h m' + m h' + h h'  on v_mfma_f32_16x16x32_bf16: six
 * matrix instructions at 16 times the rate of the fp32 one.  The dropped terms m l' + l m' + l l' are at most 2^-21 of |a| |b|
 * per term, against the 2^-24 of one fp32 rounding: the results stay inside the bars of the fp32 route (README, "Parity"), within
 * a factor of 8 of its error or 2^-21, whichever is larger.  Products of operands with at most 8 significant bits are exact.
 * Everything else (the fp64 Lipschitz bound, the step formulas, the symmetrisation) is the fp32 route's code.
 *
 * Non-finite values.  Update: a NaN or Inf anywhere in G makes both factors and both L entirely NaN, as on the fp32 route.
 * Apply: the SET of non-finite output elements is the one the definition gives, but the split turns an Inf operand into
 * h = Inf, m = NaN, so an element the definition makes +Inf or -Inf may be NaN here. */
#ifndef PSGD_KRON_QUAD_X3_HIP_H
#define PSGD_KRON_QUAD_X3_HIP_H

#include <stdint.h>
#include "psgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t psgd_kron_quad_x3_workspace_bytes(int M, int N);   /* PSGD_ERR_BAD_ARG for M < 1 or N < 1 */
int psgd_kron_quad_x3_apply_f32(const float *Ql, const float *Qr, const float *G, float *out, int M, int N, void *ws,
                                int64_t ws_bytes, void *stream);
int psgd_kron_quad_x3_update_f32(float *Ql, float *Qr, float *L, const float *G, int M, int N, float step, float decay, void *ws,
                                 int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PSGD_KRON_QUAD_X3_HIP_H */
