/* psgd_kron_quad_diag_hip.h -- C ABI of the QUAD Kronecker update with ONE DIAGONAL side, psgd_kron_qdiag.hip, in libpsgd_hip.so.
 *
 * include/psgd_kron_quad_hip.h is the update on two full symmetric factors.  Here one factor is a vector: a layer such as an
 * embedding table (131 072 x 1024) cannot hold a dense factor on its long side, so that side is diag(q).
 *
 * G is an M x N fp32 gradient.  One factor is a SYMMETRIC fp32 matrix Q (n x n, n = M or N), the other a vector q of length D
 * (the other extent) that stands for diag(q).  diag_side says which: 0 = the left factor is the vector (Ql = ql[M], Qr = Qr[N, N]),
 * 1 = the right one is (Ql = Ql[M, M], Qr = qr[N]).  L = [Ll, Lr] are two fp32 scalars on the device, 0 at the start, as in the
 * parent.  The left-diagonal case in full; the right-diagonal case is its mirror, rows and columns exchanged (A = (Ql G) diag(qr),
 * tr[j] = sum_i A[i,j]^2 with t2r = M, Tl = A A' with t2l = N, out = (Ql (Ql G)) diag(qr o qr)):
 *
 *   P        = diag(ql)^2 (x) (Qr Qr)
 *   apply    out = diag(ql o ql) ((G Qr) Qr)                      (ql o ql formed once in fp32)
 *   update   A   = diag(ql) (G Qr)
 *            tl[i] = sum_j A[i,j]^2           t2l = N              (fp64 sum in a fixed order, stored as fp32)
 *            Tr  = A' A                       t2r = M
 *      diagonal side:  ell = max_i tl[i] + t2l                     (the maximum propagates NaN)
 *                      Ll <- max(decay Ll + (1 - decay) ell, ell);  c = step / (2 Ll)
 *                      gain_i = 1 - c (tl[i] - t2l);   ql[i] <- ql[i] gain_i gain_i
 *      dense side:     exactly the parent's per-side rule on (Tr, t2r, Qr, Lr)
 *                      (s, j, bound, ell, L, c, P1, P2, Q <- (P2 + P2') / 2)
 *      Everything on the right-hand sides is the OLD state; q, Q and L are rewritten IN PLACE.
 *
 * Properties.  This is the parent's rule with T restricted to its diagonal: P2 = q gain^2 is exact, and the Lipschitz bound of a
 * diagonal matrix is its largest entry, so a diagonal side of length 1 coincides with the parent's 1 x 1 dense side.  With G = 0
 * the diagonal grows by (1 + c t2)^2, like the dense factor.  A NaN in G makes the dense factor, both L and every q NaN; an Inf in
 * row i of G (left-diagonal case) makes tl[i] and Ll +Inf, c = 0, and so leaves q finite except q[i] = NaN, while the dense
 * factor and its L are NaN.  The stored Q is exactly symmetric.
 *
 * The conventions are the parent's (the error codes of psgd_hip.h; null, shape, diag_side and aliasing checks return
 * PSGD_ERR_BAD_ARG before any HIP call; nothing allocates or synchronises; no atomics, every reduction has a fixed order: repeated
 * calls are bit-identical).  Any M, N >= 1; no alignment demand beyond 4 bytes; addresses are 64-bit.  out identical to Ql, Qr
 * or G is PSGD_ERR_BAD_ARG, and so are Ql == Qr and G or L identical to a factor in the update.  The workspace (>=
 * psgd_kron_qdiag_workspace_bytes(M, N, diag_side), 256-byte aligned, needs no initialisation) holds the intermediate products;
 * PSGD_ERR_WORKSPACE when missing, short or misaligned.  The host reads nothing back.  An update is at most 7 launches, an apply 2.
 *
 * The Gram matrix of the dense side sums over the LONG extent D, so it is split along K: S slices per upper tile, S a pure function
 * of (D, n) with fixed constants -- no device query, the bits do not depend on the board:
 *   S0 = max(1, min(ceil(PSGD_KRON_QDIAG_SLICE_TARGET / upper tiles), ceil(D / PSGD_KRON_QDIAG_SLICE_MIN_K)))
 *   steps = ceil(D / 16);  per = ceil(steps / S0);  S = ceil(steps / per)
 * Slice s sums the K range [16 per s, min(D, 16 per (s + 1))): every slice but the last has the same length, a multiple of the K
 * step, and no slice is empty.  psgd_kron_qdiag_slices returns S. */
#ifndef PSGD_KRON_QUAD_DIAG_HIP_H
#define PSGD_KRON_QUAD_DIAG_HIP_H

#include <stdint.h>
#include "psgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PSGD_KRON_QDIAG_SLICE_TARGET  1024  /* workgroups the split-K Gram aims for */
#define PSGD_KRON_QDIAG_SLICE_MIN_K   256   /* ... with no slice meant to be shorter than this */

int64_t psgd_kron_qdiag_workspace_bytes(int M, int N, int diag_side);   /* 0 = left factor diagonal, 1 = right */
int     psgd_kron_qdiag_slices(int M, int N, int diag_side);            /* S of the split-K Gram */
int psgd_kron_qdiag_apply_f32 (const float *Ql, const float *Qr, const float *G, float *out, int M, int N, int diag_side,
                               void *ws, int64_t ws_bytes, void *stream);
int psgd_kron_qdiag_update_f32(float *Ql, float *Qr, float *L, const float *G, int M, int N, int diag_side,
                               float step, float decay, void *ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PSGD_KRON_QUAD_DIAG_HIP_H */
