/* psgd_kron_quad_nd_hip.h -- C ABI of the QUAD Kronecker update on ORDER-3 tensors with THREE symmetric factors,
 * psgd_kron_qnd.hip, in libpsgd_hip.so.
 *
 * The quadratic-form update of the PyTorch line of PSGD takes one factor per tensor mode; psgd_kron_quad_hip.h restates it for
 * matrices, this header for tensors of order 3.  A conv kernel [Cout, Cin, kh, kw] is the tensor [Cout, Cin, kh kw]: factors
 * Cout^2, Cin^2 and (kh kw)^2 instead of the Cout^2 and (Cin kh kw)^2 of the folded matrix.
 *
 * G is a contiguous fp32 tensor [A, B, C], A, B, C >= 1.  Qa (A x A), Qb (B x B), Qc (C x C) are SYMMETRIC fp32 factors,
 * P = (Qa Qa) (x) (Qb Qb) (x) (Qc Qc).  L = [La, Lb, Lc] are three fp32 scalars on the device, 0 at the start.  xk is the mode-k
 * product (Y = X xk Q: Y_(k) = Q X_(k)), X_(k) the mode-k unfolding: n_k rows, A B C / n_k columns.
 *
 *   apply    out = G x1 Qa^2 x2 Qb^2 x3 Qc^2            six mode products, each factor applied twice back to back
 *   update   X   = G x1 Qa x2 Qb x3 Qc                   in this order
 *            per mode k:  T_k = X_(k) X_(k)',  t2_k = A B C / n_k
 *            then, per side (T, t2, Q, L), exactly the rule of psgd_kron_quad_hip.h:
 *              s = max|T| (NaN propagates);  bound = 0 when s == 0, else with j = first index of the largest column sum of
 *              squares of T/s:  x = (T/s)[:, j], y = (T/s) x, z = (T/s)(y / |y|_2), bound = s |z|_2   (fp64 sums, fixed order)
 *              ell = bound + t2
 *              L  <- max(decay L + (1 - decay) ell, ell)
 *              c   = step / (2 L)
 *              P1  = Q  - c (T Q  - t2 Q)
 *              P2  = P1 - c (P1 T - t2 P1)
 *              Q  <- (P2 + P2') / 2
 *            Everything on the right-hand sides is the OLD state; Qa, Qb, Qc and L are rewritten IN PLACE.
 *
 * With A = 1 and Qa = [[1]] this is the two-factor update on the matrix [B, C], bit for bit: Qb, Qc, Lb, Lc come out as
 * psgd_kron_quad_update_f32 leaves Ql, Qr, Ll, Lr (the same tile bodies, the same K order in every sum).
 *
 * The order of the apply's modes is a function of the shape alone: ascending extent, the lower mode number first among equal
 * extents; the two products of a mode are adjacent.  (Every mode product costs 2 A B C n_k flops wherever it stands; the order
 * fixes the rounding, and with A = 1 it is the order of psgd_kron_quad_apply_f32.)  The sums that form T_k run over the other two
 * modes in ascending address order: for the middle mode, a outer and c inner.
 *
 * Properties as in psgd_kron_quad_hip.h.  G = 0: every factor grows by (1 + c t2)^2.  A NaN or Inf anywhere in G makes all three
 * factors and all of L NaN.  The stored factors are exactly symmetric: Q[i,j] and Q[j,i] are one value written twice.
 *
 * The conventions are those of psgd_hip.h (its error codes; null and shape checks return before any HIP call; nothing allocates
 * or synchronises; no atomics, every output element has one writer and every reduction a fixed order: repeated calls are
 * bit-identical).  Any A, B, C >= 1 with A B C < 2^31; no alignment demand beyond 4 bytes.  out identical to a factor or to G is
 * PSGD_ERR_BAD_ARG, and so are two identical factors and G or L identical to a factor (or to each other) in the update.  The
 * workspace (>= psgd_kron_qnd_workspace_bytes(A, B, C), 256-byte aligned, needs no initialisation) holds two tensors of G's size
 * and the per-side matrices; PSGD_ERR_WORKSPACE when missing, short or misaligned.  The host reads nothing back.  An update is 7
 * launches (3 products, Gram, Lipschitz, P1, symmetrised P2), an apply 6. */
#ifndef PSGD_KRON_QUAD_ND_HIP_H
#define PSGD_KRON_QUAD_ND_HIP_H

#include <stdint.h>
#include "psgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t psgd_kron_qnd_workspace_bytes(int A, int B, int C);   /* PSGD_ERR_BAD_ARG for an extent < 1 or A B C >= 2^31 */
int psgd_kron_qnd_apply_f32(const float *Qa, const float *Qb, const float *Qc, const float *G, float *out, int A, int B, int C,
                            void *ws, int64_t ws_bytes, void *stream);
int psgd_kron_qnd_update_f32(float *Qa, float *Qb, float *Qc, float *L, const float *G, int A, int B, int C, float step, float decay,
                             void *ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PSGD_KRON_QUAD_ND_HIP_H */
