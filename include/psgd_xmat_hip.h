/* psgd_xmat_hip.h -- C ABI of the X-shaped (and diagonal) preconditioner, psgd_xmat.hip, in libpsgd_hip.so.
 *
 * Q = diag(a) + adiag(b), P = Q'Q, the state two fp32 vectors of length N.  With j = N-1-i the mirror index, every pair
 * (i, j) is an independent 2 x 2 block [[a_i, b_i], [b_j, a_j]]; for odd N the middle element m = (N-1)/2 is its own mirror,
 * b[m] is 0 by contract and nablaB[m] is taken as 0.
 *
 *   apply    w = a*g + b*flip(g),  out_i = a_i w_i + b_j w_j
 *   update   A = a*h + b*flip(h),  B_i = (a_j v_i - b_j v_j) / (a_i a_j - b_i b_j),
 *            nablaA = A*A - B*B,  nablaB = A*flip(A) - B*flip(B),  mu = step / (max(max|nablaA|, max|nablaB|) + tiny),
 *            a_i <- a_i - mu (nablaA_i a_i + nablaB_i b_j),  b_i <- b_i - mu (nablaA_i b_i + nablaB_i a_j)   (old a, b on the right)
 *
 * The conventions are those of psgd_hip.h (its error codes; null and shape checks return before any HIP call; nothing allocates
 * or synchronises; every reduction has a fixed order, no atomics: repeated calls are bit-identical).  The maximum propagates
 * NaN.  The update rewrites a and b IN PLACE.
 *
 * b == NULL selects the DIAGONAL preconditioner: b is taken as 0 everywhere and stays 0 (nablaB taken as 0), nothing is read
 * or written through b; the state is a alone.  Every other pointer is required (PSGD_ERR_BAD_ARG), N >= 1.
 * out identical to any input of the same call is PSGD_ERR_BAD_ARG.
 * All pointers 16-byte aligned and N % 4 == 0: 16-byte loads and stores on both streams; anything else: dword accesses, any
 * 4-byte alignment.  The workspace (>= psgd_xmat_workspace_bytes(N), 256-byte aligned, needs no initialisation) carries the
 * partial maxima between the two launches of an update; PSGD_ERR_WORKSPACE when missing, short or misaligned.
 * psgd_xmat_update_apply_f32 gives the bits of psgd_xmat_update_f32 followed by psgd_xmat_apply_f32. */
#ifndef PSGD_XMAT_HIP_H
#define PSGD_XMAT_HIP_H

#include <stdint.h>
#include "psgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PSGD_XMAT_TILE_ELEMS  2048   /* elements (1024 pairs) one workgroup owns per trip of its grid-stride loop */
#define PSGD_XMAT_MAX_GRID    2048   /* workgroups of the reading sweep == partial maxima in the workspace        */

int64_t psgd_xmat_workspace_bytes(int64_t N);   /* PSGD_ERR_BAD_ARG for N <= 0 */
int psgd_xmat_apply_f32(const float *a, const float *b, const float *g, float *out, int64_t N, void *stream);
int psgd_xmat_update_f32(float *a, float *b, const float *v, const float *h, int64_t N, float step, float tiny,
                         void *ws, int64_t ws_bytes, void *stream);
int psgd_xmat_update_apply_f32(float *a, float *b, const float *v, const float *h, const float *g, float *out, int64_t N,
                               float step, float tiny, void *ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PSGD_XMAT_HIP_H */
