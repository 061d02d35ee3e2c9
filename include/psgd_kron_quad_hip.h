/* psgd_kron_quad_hip.h -- C ABI of the inverse-free Kronecker whitening update (QUAD), psgd_kron_quad.hip, in libpsgd_hip.so.
 *
 * G is an M x N fp32 gradient, Ql (M x M) and Qr (N x N) are SYMMETRIC fp32 factors, P = (Ql Ql) (x) (Qr Qr).  L = [Ll, Lr] are
 * two fp32 scalars on the device, 0 at the start: the running Lipschitz estimates that bound the step.  The reference has no code
 * for this update; it is the quadratic-form update of the PyTorch line of PSGD, restated here in full:
 *
 *   apply    out = Ql (Ql G Qr) Qr
 *   update   A  = Ql G Qr
 *            Tl = A A',  t2l = N          Tr = A' A,  t2r = M          (t2 = numel(G) / side length)
 *            per side (T, t2, Q, L):
 *              s = max|T|                                   (the maximum propagates NaN)
 *              if s == 0:  bound = 0
 *              else:  j = first index of the largest column sum of squares of T/s
 *                     x = (T/s)[:, j];  y = (T/s) x;  z = (T/s) (y / |y|_2);  bound = s |z|_2     (fp64 sums, fixed order)
 *              ell = bound + t2
 *              L  <- max(decay L + (1 - decay) ell, ell)
 *              c   = step / (2 L)
 *              P1  = Q  - c (T Q  - t2 Q)
 *              P2  = P1 - c (P1 T - t2 P1)
 *              Q  <- (P2 + P2') / 2
 *            Everything on the right-hand sides is the OLD state; Ql, Qr and L are rewritten IN PLACE.
 *
 * Properties.  The fixed point is E[Ql G Qr Qr G' Ql] = N I and its mirror E[Qr G' Ql Ql G Qr] = M I on the right: the Kronecker
 * whitening condition; for G = Cl^(1/2) Z Cr^(1/2) it is reached by P = Cl^-1 (x) Cr^-1, the inverse of the
 * gradient's Kronecker covariance.  No solve, no inverse, no probe: products and norms only.  With G = 0 every T is 0, ell = t2, and the
 * factors GROW by (1 + c t2)^2 -- that is the method: "zero in gives zero out" holds for the apply, not for this update.  A NaN
 * or Inf anywhere in G makes both factors and both L entirely NaN.  The stored Q is exactly symmetric: Q[i,j] and Q[j,i] are one
 * value written twice.
 *
 * The conventions are those of psgd_hip.h (its error codes; null and shape checks return before any HIP call; nothing allocates
 * or synchronises; no atomics, every reduction has a fixed order: repeated calls are bit-identical).  Any M, N >= 1; no
 * alignment demand beyond 4 bytes (16-byte loads are used where a tile allows them, dword loads otherwise; partial tiles are
 * handled in the kernels).  out identical to Ql, Qr or G is PSGD_ERR_BAD_ARG, and so are Ql == Qr and G or L identical to a
 * factor in the update.  The workspace (>= psgd_kron_quad_workspace_bytes(M, N), 256-byte aligned, needs no initialisation) holds
 * the intermediate products; PSGD_ERR_WORKSPACE when missing, short or misaligned.  The host reads nothing back: L and c travel
 * through device memory.  An update is 6 launches, an apply 4. */
#ifndef PSGD_KRON_QUAD_HIP_H
#define PSGD_KRON_QUAD_HIP_H

#include <stdint.h>
#include "psgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PSGD_KRON_QUAD_TILE  64   /* edge of the output tile one workgroup owns */

int64_t psgd_kron_quad_workspace_bytes(int M, int N);   /* PSGD_ERR_BAD_ARG for M < 1 or N < 1 */
int psgd_kron_quad_apply_f32(const float *Ql, const float *Qr, const float *G, float *out, int M, int N, void *ws, int64_t ws_bytes,
                             void *stream);
int psgd_kron_quad_update_f32(float *Ql, float *Qr, float *L, const float *G, int M, int N, float step, float decay, void *ws,
                              int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PSGD_KRON_QUAD_HIP_H */
