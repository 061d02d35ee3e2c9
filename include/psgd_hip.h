/*
 * psgd_hip.h -- C ABI of the MI355X (gfx950) PSGD preconditioner engine.
 *
 * This is the drop-in boundary for the hot path of the reference module
 * preconditioned_stochastic_gradient_descent.py ("psgd.py" below).  The
 * reference has no FFI of its own (it is pure Python on TensorFlow), so each
 * entry point cites the reference *function* (file:line) whose arithmetic it
 * replaces.  The Python module of the same name in this repository binds these
 * symbols through ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - Every data pointer is a DEVICE pointer (HBM) unless marked [host].
 *   - Matrices are row-major fp32.  U, V are [N, r] contiguous (leading
 *     dimension r), vectors are [N] (the reference's [N,1] columns).
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on
 *     it and performs no host synchronisation and no allocation.
 *   - Return value: PSGD_OK (0) or a negative PSGD_ERR_* code.  Nothing is
 *     written when an argument check fails.
 *   - `ws` is a caller-owned device workspace of at least
 *     psgd_uvd_workspace_bytes(N, r) bytes, 256-byte aligned.  Its contents
 *     carry the small reduced vectors between the stages of one call.
 *
 * Multi-GPU (row-sharded flat parameter vector, one process per GPU): call the
 * *_sweepK stage functions on the local shard and all-reduce the region that
 * psgd_uvd_ws_region() reports between stages (SUM on the fp64 sums, MAX on
 * the fp32 max buffer); pass sums_reduced=1 to the following stage.
 */
#ifndef PSGD_HIP_H
#define PSGD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* History: 1 = round 1; 2 = round 2 (psgd_uvd_fused_s1_f32 removed, SUMS region of stage 13 holds 4r entries,
 * workspace layout changed); 3 = round 3 (entry points added, bf16 apply workspace carries a hand-off route word);
 * 4 = round 4 (Kron dense (x) dense workspaces of small layers carry the scratch of the fused strip kernels);
 * 5 = round 4, late (the *_ld row-stride forms of the wide-rank building blocks and psgd_kron_dd_apply_direct_f32 added; Kron tuning
 * keys retired / renumbered -- bf16 key 4 now selects the stream-K gradient launches, not the DMA position; the workspace of
 * psgd_kron_dd_update_bf16 gained the stream-K partial tiles (up to 128 MiB more for M, N multiples of 256) and padded W1 / W2
 * row strides: always size it with psgd_kron_dd_update_workspace_bytes_bf16);
 * 6 = round 5 (psgd_uvd_apply_cols_f32 added: precond_grad_UVd_math on a matrix g; psgd_uvd_gram_wide_f32 and the psgd_uvd_wide_*
 * entry points of ranks 33 .. 64 added (building blocks, update, fused update -> apply); the sparse-LU entry points take ranks up to PSGD_SPLU_MAX_RANK = 64 and their workspace
 * regions have that capacity -- offsets from psgd_splu_ws_region changed; the fused strip kernels of small Kron layers and their
 * tuning key 21 removed: Kron workspaces of small layers shrink back by that scratch);
 * 7 = round 6 (psgd_kron_bf16_handoff_counter_offset added; bf16 tuning key 7: XCD patch of the fused pair; no layout change);
 *     later, additive: psgd_kron_dd_route_flags and the PSGD_KRON_ROUTE_* bits; the dense preconditioner's
 *     psgd_dense_workspace_bytes, psgd_dense_update_f32 and psgd_dense_apply_f32 (new symbols only: the version stays 7);
 *     the psgd_uvd_*_bf16 entry points of a bf16-stored UVd state (new symbols only);
 *     psgd_uvd_pack_f32, psgd_uvd_sumsq_f32 and psgd_uvd_param_update_multi, the tail of UVd.step (new symbols only: still 7).
 *     the stage forms of the bf16-state UVd calls, psgd_uvd_bf16_ws_region and psgd_uvd_bf16_fold_gathered_f64 (new symbols only: still 7).
 *     psgd_uvd_bf16_narrow_f32, the fp32 -> stored bf16 narrowing of a checkpoint load (new symbol only: still 7).
 *     psgd_splu_bf16_workspace_bytes, psgd_splu_apply_bf16 and psgd_splu_update_bf16, the sparse-LU preconditioner on a bf16-stored
 *     state (new symbols only, no existing layout changes: still 7).
 *     psgd_uvd_pack_blend_f32 and psgd_uvd_param_update_multi_wd, momentum and decoupled weight decay in the tail of UVd.step
 *     (new symbols only: still 7).
 *     psgd_uvd_pack_check_f32 and psgd_uvd_check_multi, the non-finite guard of UVd.step (new symbols only: still 7).
 *     psgd_multi_sumsq_f32, psgd_multi_param_update_f32 and psgd_multi_diff_scale_f32, the step tail on lists of tensors of
 *     class Kron (new symbols only: still 7).
 *     psgd_multi_blend_f32, psgd_multi_scale_check_f32 and psgd_multi_param_update_wd_f32: momentum, the non-finite guard with the
 *     loss scale, and decoupled weight decay of class Kron (additive, new symbols only: still 7).
 *     psgd_multi_widen_check and psgd_multi_param_update_t: bfloat16 / float16 parameters of class Kron (additive, new symbols
 *     only: still 7).
 *     psgd_multi_vec_update_f32 and psgd_multi_vec_apply_f32: the vector layers of class Kron(any_rank=True) (additive, new symbols
 *     only: still 7).
 *     psgd_multi_narrow_bf16, psgd_multi_sumsq_mixed and psgd_multi_param_update_mixed: the bf16-operand layers of class
 *     Kron(operands="bfloat16") (additive, new symbols only: still 7).
 *     psgd_uvd_param_update_multi_sr, psgd_multi_param_update_sr and psgd_multi_param_update_mixed_sr: stochastic rounding of the
 *     bf16 parameter update of class UVd and class Kron (additive, new symbols only: still 7).
 *     psgd_multi_randn_f32: the counter-based probe vectors of class Kron(preconditioner_fit="whitening") (additive, a new symbol
 *     only: still 7).
 * psgd_tf_amd/_lib.py refuses a library whose psgd_abi_version() differs from the one it was written for. */
#define PSGD_ABI_VERSION 7

#define PSGD_OK                 0
#define PSGD_ERR_BAD_ARG       (-1)   /* null pointer, N <= 0, r <= 0 ...            */
#define PSGD_ERR_RANK          (-2)   /* rank r outside the entry point's range      */
#define PSGD_ERR_WORKSPACE     (-3)   /* workspace missing, too small or misaligned  */
#define PSGD_ERR_ALIGN         (-4)   /* a matrix pointer is not 16-byte aligned     */
#define PSGD_ERR_LAUNCH        (-5)   /* HIP reported a launch error                 */
#define PSGD_ERR_SHAPE         (-6)   /* Kron: shapes inconsistent / unsupported     */

#define PSGD_UVD_MAX_RANK 32
#define PSGD_SPLU_MAX_RANK 64   /* the sparse-LU entry points (round 5: the tail kernels are instantiated for 1 .. 64) */

/* workspace regions that the multi-GPU driver exchanges between stages.  Two equivalent protocols:
 *  (a) all-gather + fold (what psgd_tf_amd/sharded.py does): all-gather every rank's PSGD_WS_SEND_F64 region of the
 *      stage into a [world][count] fp64 buffer and call psgd_*_fold_gathered_f64, which folds the copies in rank
 *      order (SUM or MAX per entry).  One collective per exchange point, and the reduced values are bit-identical on
 *      every rank whatever algorithm the collective library picks.
 *  (b) all-reduce in place: SUM on the PSGD_WS_SUMS_F64 region and MAX on the PSGD_WS_MAX_F32 region of the stage. */
#define PSGD_WS_SUMS_F64   0   /* double[len]: SUM over ranks  */
#define PSGD_WS_MAX_F32    1   /* float[len]:  MAX over ranks  */
#define PSGD_WS_SEND_F64   2   /* double[len]: this rank's contribution, to be all-gathered and folded */

int         psgd_abi_version(void);
const char *psgd_error_string(int code);

/* ------------------------------------------------------------------ UVd ---
 * Q = (I + U V') diag(d), preconditioner P = Q'Q  (psgd.py:527-627).        */

/* Bytes of device workspace needed for a shard of N rows at rank r
 * (includes the N-float temporary for nablaD, psgd.py:581). <0 on error.   */
int64_t psgd_uvd_workspace_bytes(int64_t N, int r);

/* Byte offset (into ws) and element count of a region to all-reduce.
 * `which` = PSGD_WS_SUMS_F64 / PSGD_WS_MAX_F32; `stage` selects what the next
 * stage consumes: apply: 1 (after sweep1: r sums), 2 (after sweep2: r sums);
 * update: 10 (balance maxima: 2 floats), 11 (after sweep1: Gram sums),
 * 12 (after sweep2: 1 float max), 13 (after the fused sweep2: the 4r sums [pU | pV | qU | qV]).
 * Returns 0 or an error code.                                                */
int psgd_uvd_ws_region(int which, int stage, int64_t N, int r,
                       int64_t *offset_bytes, int64_t *count);
/* Protocol (a): PSGD_WS_SEND_F64 regions exist for stages 1, 2, 11 (sums), 10 (2 maxima), 12 (1 maximum) and
 * 13 ([pU | pV | qU | qV | max]: the 4r sums and the maximum of the fused sweep 2 in ONE region, so the fused step
 * needs two exchanges: 11, 13).  `gathered` = the all-gathered regions, [world][count] doubles in rank order (device).   */
int psgd_uvd_fold_gathered_f64(int stage, const double *gathered, int world, int64_t N, int r,
                               void *ws, int64_t ws_bytes, void *stream);

/* precond_grad_UVd_math(U, V, d, g)   psgd.py:619-627 (IpUVtmatvec :540-544)
 *   out = d .* (I + V U') (I + U V') (d .* g)
 * Three streaming sweeps (the second reduction depends on the first); V is read twice and
 * U once:
 *   sweep1: s1 = V'(d.*g)                          reads V,d,g
 *   sweep2: g1 = d.*g + U s1 -> out;  s2 = U'g1    reads U,d,g   writes out (= g1)
 *   sweep3: out = d.*(g1 + V s2)  in place         reads V,d,out writes out
 * `out` must not alias any input; between sweep2 and sweep3 it holds g1.          */
int psgd_uvd_apply_f32(const float *U, const float *V, const float *d,
                       const float *g, float *out, int64_t N, int r,
                       void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_apply_sweep1_f32(const float *V, const float *d, const float *g,
                              int64_t N, int r, void *ws, int64_t ws_bytes,
                              void *stream);
int psgd_uvd_apply_sweep2_f32(const float *U, const float *d, const float *g,
                              float *out, int64_t N, int r, int sums_reduced,
                              void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_apply_sweep3_f32(const float *V, const float *d, float *out,
                              int64_t N, int r, int sums_reduced,
                              void *ws, int64_t ws_bytes, void *stream);

/* update_precond_UVd_math_(U, V, d, v, h, step, tiny)   psgd.py:554-617
 * Mutates U or V (branch update_U, psgd.py:588) and d in place.
 *   balance  : the branch of psgd.py:562-567 (rescale U/rho, rho*V)
 *   update_U : 1 -> psgd.py:589-601, 0 -> psgd.py:603-615
 * Stages: [balance_max, balance_scale]  sweep1 (Gram of [U V t w])
 *         sweep2 (r x r solves, row-local update of U or V, nablaD, max)
 *         sweep3 (d <- d - mu d nablaD).                                    */
int psgd_uvd_update_f32(float *U, float *V, float *d, const float *v,
                        const float *h, int64_t N, int r, float step,
                        float tiny, int balance, int update_U,
                        void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_balance_max_f32(const float *U, const float *V, int64_t N, int r,
                             void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_balance_scale_f32(float *U, float *V, int64_t N, int r,
                               void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_update_sweep1_f32(const float *U, const float *V, const float *d,
                               const float *v, const float *h, int64_t N,
                               int r, void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_update_sweep2_f32(float *U, float *V, const float *d,
                               const float *v, const float *h, int64_t N,
                               int r, float step, float tiny, int update_U,
                               void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_update_sweep3_f32(float *d, int64_t N, int r, float step,
                               float tiny, void *ws, int64_t ws_bytes,
                               void *stream);

/* Fused update -> apply (the UVd.step call pattern, psgd.py:732 -> :748): THREE sweeps for both calls.
 * Same U, V, d as psgd_uvd_update_f32; `out` = precond_grad_UVd_math on the updated state.  Update sweep 2 also
 * reduces the four r-vectors [Unew | Vnew]' [d.*g, d.*g.*nablaD] (on the matrix core).  With dnew = d - mu_d d.*nablaD
 * (psgd.py:584) both reductions of the apply follow from them and from the Gram of sweep 1:
 *     s1' = Vnew'(dnew.*g) = pV - mu_d qV,      s2' = Unew'(dnew.*g + Unew s1') = pU - mu_d qU + (Unew'Unew) s1'
 * (Unew'Unew = U'U plus a rank-2 correction known from the r x r algebra), so the d update and the whole apply are
 * ONE last sweep: out = dnew .* (dnew.*g + Unew s1' + Vnew s2').  628 -> 612 bytes per parameter at r = 20 and 9 -> 6 launches.
 * Multi-GPU stages: [balance] -> update_sweep1 -> X(11) -> update_sweep2_fused -> X(13: 4r sums | max) ->
 * fused_post -> fused_final: two exchanges per step. */
int psgd_uvd_update_apply_f32(float *U, float *V, float *d, const float *v, const float *h,
                              const float *g, float *out, int64_t N, int r, float step, float tiny,
                              int balance, int update_U, void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_update_sweep2_fused_f32(float *U, float *V, const float *d, const float *v,
                                     const float *h, const float *g, int64_t N, int r, float step,
                                     float tiny, int update_U, void *ws, int64_t ws_bytes,
                                     void *stream);
int psgd_uvd_fused_post_f32(int64_t N, int r, float step, float tiny, int update_U, void *ws,
                            int64_t ws_bytes, void *stream);
int psgd_uvd_fused_final_f32(const float *U, const float *V, float *d, const float *g, float *out,
                             int64_t N, int r, float step, float tiny, void *ws, int64_t ws_bytes,
                             void *stream);

/* IpUVtmatvec(U, V, x)   psgd.py:540-544:  out = x + U (V' x), x is [N].   */
int psgd_uvd_ipuvt_matvec_f32(const float *U, const float *V, const float *x,
                              float *out, int64_t N, int r,
                              void *ws, int64_t ws_bytes, void *stream);

/* IpUVtmatvec with a matrix x (psgd.py:542 "matrices or column vectors"): k columns, given as HOST arrays of k device
 * pointers to contiguous [N] vectors (xs in, outs out; outs[j] may not alias any input).  One sweep of V and one of U
 * per group of four columns.                                                                                       */
int psgd_uvd_ipuvt_matvec_cols_f32(const float *U, const float *V, const float *const *xs,
                                   float *const *outs, int k, int64_t N, int r,
                                   void *ws, int64_t ws_bytes, void *stream);

/* precond_grad_UVd_math(U, V, d, g) with a MATRIX g (psgd.py:619-627; docstring :623 "either matrices or column vectors": d
 * broadcasts over the columns, psgd.py:625-626): k columns as HOST arrays of k device pointers to contiguous [N] vectors (gs in,
 * outs out; outs[j] may be gs[j], otherwise no aliasing).  Per group of four columns: S1 = V'(d.*G), G1 = d.*G + U S1 with
 * S2 = U'G1 from the same sweep, out = d.*(G1 + V S2) -- three sweeps (V, U, V) per FOUR columns.                      */
int psgd_uvd_apply_cols_f32(const float *U, const float *V, const float *d, const float *const *gs,
                            float *const *outs, int k, int64_t N, int r,
                            void *ws, int64_t ws_bytes, void *stream);

/* The Gram of update_precond_UVd_math_ (psgd.py:569-615: every inner product of the columns of W = [U | V | d .* h | v ./ d]) for
 * ranks PSGD_UVD_MAX_RANK < r <= 2 PSGD_UVD_MAX_RANK in ONE sweep over U and V (round 5; the chunked wide-rank path needed three):
 * G [2r + 2][2r + 2], fp64, row-major, symmetric.  U, V contiguous [N, r] (16-byte aligned when r % 4 == 0); scratch:
 * psgd_uvd_gram_wide_scratch_bytes(N, r) bytes, 256-byte aligned, contents need not survive.                                      */
int64_t psgd_uvd_gram_wide_scratch_bytes(int64_t N, int r);
int psgd_uvd_gram_wide_f32(const float *U, const float *V, const float *d, const float *v, const float *h,
                           int64_t N, int r, double *G, void *scratch, int64_t scratch_bytes, void *stream);

/* Ranks PSGD_UVD_MAX_RANK < r <= 2 PSGD_UVD_MAX_RANK on the whole contiguous [N, r] matrices (round 5; 16-byte aligned): the three
 * sweeps of precond_grad_UVd_math on k columns (k = 1: the column-vector call), and the four-column building blocks of the update's
 * row-local part -- S = M'[x_0 ..] (fp64 [k][r]), out_j = x_j + M S_j (S fp32 [k][r]), M <- M - (a c1' - b c2') (c = [c1 | c2] fp32).
 * scratch: psgd_uvd_wide_scratch_bytes(N, r) bytes, 256-byte aligned, contents need not survive.  (Ranks above 64, and strided
 * views, stay on the column-chunk blocks below.)                                                                                     */
int64_t psgd_uvd_wide_scratch_bytes(int64_t N, int r);
int psgd_uvd_wide_apply_cols_f32(const float *U, const float *V, const float *d, const float *const *gs, float *const *outs,
                                 int k, int64_t N, int r, void *scratch, int64_t scratch_bytes, void *stream);
int psgd_uvd_wide_colsums_f32(const float *M, const float *const *xs, int k, double *S, int64_t N, int r,
                              void *scratch, int64_t scratch_bytes, void *stream);
int psgd_uvd_wide_axpy_cols_f32(const float *M, const float *const *xs, float *const *outs, int k, const float *S,
                                int64_t N, int r, void *stream);
int psgd_uvd_wide_rank2_update_f32(float *M, const float *a, const float *b, const float *c, int64_t N, int r, void *stream);

/* update_precond_UVd_math_ (psgd.py:554-617 without the balancing of :562-567, which stays with the caller) for
 * PSGD_UVD_MAX_RANK < r <= 2 PSGD_UVD_MAX_RANK on one GPU, in place on U or V (update_U) and d: the Gram of
 * psgd_uvd_gram_wide_f32, the r x r algebra in one workgroup (fp64, partial pivoting), one sweep that reads U and V and
 * writes the updated factor and nablaD, and the update of d -- 5r + 10 floats per row, the traffic of the specialised ranks.
 * U, V contiguous [N, r], 16-byte aligned, d 16-byte aligned; scratch: psgd_uvd_wide_update_scratch_bytes(N, r) bytes
 * (about 4 N), 256-byte aligned, contents need not survive.                                                              */
int64_t psgd_uvd_wide_update_scratch_bytes(int64_t N, int r);
/* ... followed by precond_grad_UVd_math on the updated state (the UVd.step pattern, psgd.py:732 -> :748; what
 * psgd_uvd_update_apply_f32 is for r <= 32): sweep 2 also reduces [Unew | Vnew]' [d.*g, d.*g.*nablaD], one small kernel turns those
 * sums and the Gram into the two r-vectors of the apply, one last sweep updates d and writes out -- U and V are read three times.
 * g, out: [N], out must not alias g.  Same results as the two calls within rounding (tests: 2e-5).                              */
int64_t psgd_uvd_wide_update_apply_scratch_bytes(int64_t N, int r);
int psgd_uvd_wide_update_apply_f32(float *U, float *V, float *d, const float *v, const float *h, const float *g, float *out,
                                   int64_t N, int r, float step, float tiny, int update_U,
                                   void *scratch, int64_t scratch_bytes, void *stream);
int psgd_uvd_wide_update_f32(float *U, float *V, float *d, const float *v, const float *h, int64_t N, int r,
                             float step, float tiny, int update_U, void *scratch, int64_t scratch_bytes, void *stream);

/* Building blocks of the wide-rank path.  The sweep kernels are instantiated for ranks 1..PSGD_UVD_MAX_RANK; a
 * preconditioner of larger rank (the reference has no limit, psgd.py:663) is handled one level up
 * (psgd_tf_amd/uvd_wide.py) on column chunks of U and V -- each chunk a contiguous [N, rc] matrix, rc <= 32 -- with the
 * Gram sweep (psgd_uvd_update_sweep1_f32 on pairs of chunks) and these three calls.  xs / outs: HOST arrays of k device
 * pointers to contiguous [N] vectors; S, c: DEVICE arrays.
 *   colsums:    S[j][0..r) = M' x_j                (fp64)
 *   axpy_cols:  out_j = x_j + M S_j                (S fp32 [k][r]; out_j may be x_j itself)
 *   rank2:      M <- M - (a c1' - b c2')           (c = [c1 | c2] fp32; psgd.py:600-601 / :614-615 with mu folded in)  */
int psgd_uvd_colsums_f32(const float *M, const float *const *xs, int k, double *S, int64_t N, int r,
                         void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_axpy_cols_f32(const float *M, const float *const *xs, float *const *outs, int k,
                           const float *S, int64_t N, int r, void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_rank2_update_f32(float *M, const float *a, const float *b, const float *c, int64_t N, int r,
                              void *ws, int64_t ws_bytes, void *stream);

/* The same building blocks on a strided VIEW (round 4): M (U, V) is an [N, r] column block of a wider row-major matrix, element
 * (row, c) at M[row * ld + c], ld >= r in floats -- psgd_tf_amd/uvd_wide.py and splu_wide.py pass column views of U, V, L2
 * instead of copies of them (SURVEY 8b's `ldU, ldV`).  ld and the byte address of the view must be multiples of the rank's access
 * width (r % 4 == 0: 16 bytes, r % 2 == 0: 8, odd r: 4), else PSGD_ERR_ALIGN (the callers then copy that chunk).  ld == r is the
 * contiguous call.  psgd_uvd_update_sweep1_ld_f32 is the Gram sweep (stage 11) of a pair of such views. */
int psgd_uvd_colsums_ld_f32(const float *M, int64_t ld, const float *const *xs, int k, double *S, int64_t N, int r,
                            void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_axpy_cols_ld_f32(const float *M, int64_t ld, const float *const *xs, float *const *outs, int k,
                              const float *S, int64_t N, int r, void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_rank2_update_ld_f32(float *M, int64_t ld, const float *a, const float *b, const float *c, int64_t N, int r,
                                 void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_update_sweep1_ld_f32(const float *U, int64_t ldU, const float *V, int64_t ldV, const float *d,
                                  const float *v, const float *h, int64_t N, int r, void *ws, int64_t ws_bytes,
                                  void *stream);

/* ------------------------------------------------------ UVd, bf16 state ---
 * The same preconditioner with U, V ([N, r]) and d ([N]) STORED as bf16 (psgd.py:671, :688-690: the state in the
 * parameters' type); v, h, g and out are fp32 and all arithmetic is fp32 / fp64 -- only the HBM image of the state is
 * narrow (psgd_uvd_bf16.hip).  1 <= r <= PSGD_UVD_MAX_RANK (PSGD_ERR_RANK above), any N >= 1.  U, V, d must be 16-byte
 * aligned (PSGD_ERR_ALIGN).  The workspace (psgd_uvd_bf16_workspace_bytes, 256-byte aligned, about 16 MiB + 4 N) has a
 * layout of its own and needs no initialisation.  Results are bit-identical from call to call.
 *   rounding 0: round to nearest even.
 *   rounding 1: stochastic -- a finite fp32 value with bits b is stored as (b + u) >> 16, u uniform in [0, 2^16) from a
 *               counter hash of (seed, tensor, flat element index): the result depends on the seed and the element only.
 *               NaN and Inf are stored as they are.  Applies to every state tensor the call writes.
 *   any other value: PSGD_ERR_BAD_ARG.
 * balance = 1 (psgd.py:562-567) rewrites both factors; the rescaling happens in registers, so every stored element is
 * rounded once.  psgd_uvd_update_apply_bf16 = the update followed by precond_grad_UVd_math ON THE STORED (rounded) STATE:
 * five sweeps (the d update rides on the apply's first sweep); out must not alias g, v or h.                          */
int64_t psgd_uvd_bf16_workspace_bytes(int64_t N, int r);
/* The 64-bit key of the stochastic-rounding stream of one state tensor (0 = U, 1 = V, 2 = d) under `seed`; host only.  The
 * seed is hashed before the tensor id enters, so related seeds (seed + c, ...) never alias one tensor's stream to another's. */
uint64_t psgd_uvd_bf16_rounding_key(uint64_t seed, int tensor);
int psgd_uvd_apply_bf16(const void *U, const void *V, const void *d, const float *g, float *out,
                        int64_t N, int r, void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_update_bf16(void *U, void *V, void *d, const float *v, const float *h, int64_t N, int r,
                         float step, float tiny, int balance, int update_U,
                         int rounding, uint64_t seed, void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_update_apply_bf16(void *U, void *V, void *d, const float *v, const float *h, const float *g, float *out,
                               int64_t N, int r, float step, float tiny, int balance, int update_U,
                               int rounding, uint64_t seed, void *ws, int64_t ws_bytes, void *stream);
/* fp32 values into the stored form (loading an fp32 checkpoint into a bf16 state): dst[i] = the bf16 code of src[i], i < count,
 * narrowed exactly as the calls above narrow what they write (rounding 0 / 1; NaN and Inf stored as they are).  tensor: 0 = U,
 * 1 = V, 2 = d -- the stream is that of psgd_uvd_bf16_rounding_key(seed, tensor).  index0: the flat GLOBAL element index of
 * src[0], (row0 + first row) * r for a factor and row0 + first row for d, so the codes depend on neither the chunks a caller
 * copies in nor the row split.  Streaming: no workspace, no atomics, no synchronisation; src needs 4-byte and dst 2-byte
 * alignment only (PSGD_ERR_ALIGN), 16-byte stores and loads from any such addresses.  count = 0 is a no-op (PSGD_OK); null
 * pointers, count < 0, index0 < 0, tensor outside 0 .. 2 and rounding outside 0 .. 1 return PSGD_ERR_BAD_ARG before any HIP call. */
int psgd_uvd_bf16_narrow_f32(const float *src, void *dst, int64_t count, int64_t index0, int tensor, int rounding,
                             uint64_t seed, void *stream);

/* Stage forms of the three calls above for a ROW-SHARDED bf16 state (one process per GPU; every rank passes its rows, N = its
 * row count).  Same conventions: bf16 U, V, d (16-byte aligned), fp32 v, h, g, out, the workspace of
 * psgd_uvd_bf16_workspace_bytes(N, r), rounding and seed as above; argument checks return before any HIP call.  Every stage
 * leaves this rank's contribution to the following exchange as fp64 in the send region psgd_uvd_bf16_ws_region reports
 * (`which` must be PSGD_WS_SEND_F64: protocol (a), all-gather + fold, is the only one; stages 10, 11, 12, 1, 2 as in the fp32
 * family).  psgd_uvd_bf16_fold_gathered_f64 folds the gathered copies ([world][count] doubles, rank order) in rank order --
 * sums in fp64, maxima with the NaN-propagating maximum -- and leaves the workspace exactly as the next kernel of the one-call
 * sequence expects it.  The fold is not optional: with world = 1 it is what publishes the values.
 *   stage 10: 2 maxima (max|U|, max|V|)        11: the folded Gram, the 16 ceil((2r + 6) / 16) rows of the fp64 [.][80] matrix
 *         12: 1 maximum (max|nablaD|)               in use (at most 80 x 80 = 50 KB, never the block partials)
 *          1: r sums V'(d .* g)                2: r sums U'g1
 * Sequences (X = exchange):
 *   apply:   apply_sweep1 -> X(1) -> apply_sweep2 -> X(2) -> apply_sweep3                                       2 exchanges
 *   update:  [balance_max -> X(10)] update_gram -> X(11) -> update_rewrite -> X(12) -> update_d                 2 (+1)
 *   fused:   [balance_max -> X(10)] update_gram -> X(11) -> update_rewrite -> X(12) -> apply_sweep1_d -> X(1)
 *            -> apply_sweep2 -> X(2) -> apply_sweep3                                                            4 (+1)
 * The fused step needs FOUR exchanges where the fp32 family needs two: that family derives the apply's reductions from sums
 * over the unrounded d and factor, and here the apply must see the STORED (rounded) state, which exists only after the
 * rewrite and the d update.  Exchanges must not be merged by algebra on the unrounded state.
 * row0: the global index of this rank's first row.  The stochastic-rounding index of element (row, c) of U / V is
 * (row0 + row) * r + c and of d it is row0 + row, so no two ranks share random numbers and the stored codes do not depend on
 * the split (up to the fp64 fold order of the sums).  The one-call functions are row0 = 0.
 * balance (update_rewrite) must be what the call decided for balance_max: 1 rescales and rewrites both factors.          */
int psgd_uvd_bf16_ws_region(int which, int stage, int64_t N, int r, int64_t *offset_bytes, int64_t *count);
int psgd_uvd_bf16_fold_gathered_f64(int stage, const double *gathered, int world, int64_t N, int r,
                                    void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_balance_max_bf16(const void *U, const void *V, int64_t N, int r, void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_update_gram_bf16(const void *U, const void *V, const void *d, const float *v, const float *h,
                              int64_t N, int r, void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_update_rewrite_bf16(void *U, void *V, const void *d, const float *v, const float *h, int64_t N, int r,
                                 float step, float tiny, int balance, int update_U, int rounding, uint64_t seed,
                                 int64_t row0, void *ws, int64_t ws_bytes, void *stream);
/* d <- d - mu_d d nablaD on its own (the plain update) ... */
int psgd_uvd_update_d_bf16(void *d, int64_t N, int r, float step, float tiny, int rounding, uint64_t seed,
                           int64_t row0, void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_apply_sweep1_bf16(const void *V, const void *d, const float *g, int64_t N, int r,
                               void *ws, int64_t ws_bytes, void *stream);
/* ... or riding on the apply's first sweep (the fused step) */
int psgd_uvd_apply_sweep1_d_bf16(const void *V, void *d, const float *g, int64_t N, int r, float step, float tiny,
                                 int rounding, uint64_t seed, int64_t row0, void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_apply_sweep2_bf16(const void *U, const void *d, const float *g, float *out, int64_t N, int r,
                               void *ws, int64_t ws_bytes, void *stream);
int psgd_uvd_apply_sweep3_bf16(const void *V, const void *d, float *out, int64_t N, int r,
                               void *ws, int64_t ws_bytes, void *stream);

/* ------------------------------------------------- UVd, tail of the step ---
 * What class UVd does around the preconditioner call (psgd.py:729-730, :747, :750-762), for any number k of parameter tensors
 * in a fixed number of launches (psgd_uvd_tail.hip).  All k tensors of one call have one dtype (PSGD_DTYPE_*).
 *
 * Two DEVICE tables describe the work:
 *   segments: k entries {uint64_t ptr; int64_t start; int64_t count} -- a tensor's device pointer (aligned to its element), its
 *             start offset in the flat vector and its element count (0 allowed);
 *   chunks:   nchunks entries {int64_t seg; int64_t off} -- elements [off, min(off + PSGD_UVD_TAIL_CHUNK, count)) of segment seg.
 *             Built by the caller from the sizes alone: for every segment in order, off = 0, CHUNK, 2 CHUNK, ... while off < count,
 *             so every flat element belongs to exactly one chunk and no chunk crosses a segment.  Entries that do not fit the
 *             segment table (seg outside [0, k), off outside [0, count)) are skipped.
 * Null pointers, k < 0, nchunks < 0 and an unknown dtype return PSGD_ERR_BAD_ARG before any HIP call; nchunks == 0 is a no-op.  */
#define PSGD_DTYPE_F32   0
#define PSGD_DTYPE_BF16  1
#define PSGD_DTYPE_F16   2
#define PSGD_UVD_TAIL_CHUNK      4096   /* elements per chunk */
#define PSGD_UVD_SUMSQ_WS_BYTES  8192   /* workspace of psgd_uvd_sumsq_f32 (8-byte aligned, needs no initialisation) */

/* out[start + i] = fl32(float(tensor[i]) * scale) for every segment: torch.cat([...]).float() * scale (psgd.py:729-730, :747;
 * scale = 1 / delta_param_scale on the finite-difference branch, :734-736).  out: flat fp32, 4-byte aligned.                     */
int psgd_uvd_pack_f32(const void *segs, int k, const void *chunks, int64_t nchunks, int dtype, float scale, float *out,
                      void *stream);

/* The same pack BLENDED into out (the momentum buffer of class UVd): x = fl32(float(tensor[i]) * scale), then
 *     out[start + i] = fl32(fl32(beta * out[start + i]) + fl32(omb * x)),
 * every operation rounded on its own.  beta and omb are separate arguments: the caller passes omb = float(1) - beta, rounded once
 * on the host.  beta == 0 does NOT read out: out[start + i] = fl32(omb * x), whatever out held (with omb == 1 the bits of
 * psgd_uvd_pack_f32).  Same tables, dtypes and argument checks as psgd_uvd_pack_f32.                                             */
int psgd_uvd_pack_blend_f32(const void *segs, int k, const void *chunks, int64_t nchunks, int dtype, float scale, float beta,
                            float omb, float *out, void *stream);

/* The guarded step of class UVd (nonfinite="skip").  psgd_uvd_pack_check_f32 writes exactly the bits of psgd_uvd_pack_f32 and, when
 * any value it WRITES, fl32(float(tensor[i]) * scale), is not finite (+-Inf or NaN: a finite input that overflows under scale
 * counts), stores stamp to *flag.  psgd_uvd_check_multi applies the same predicate to the same tables, reading every element once
 * in its own type, and writes nothing but the flag (for the gradients of a momentum step: psgd_uvd_pack_blend_f32 overwrites the
 * buffer it blends into, so they are judged before the blend).
 * flag: one 4-byte aligned device word.  Every writer stores the same value with an ordinary store: no atomics, no reduction.  The
 * word is never zeroed: the caller passes a stamp it has not used on this word before (1, 2, ... 2^31 - 1, then 1 again) and reads
 * "bad" as *flag == stamp after the launch has completed.  flag == NULL or stamp <= 0: PSGD_ERR_BAD_ARG before any HIP call. */
int psgd_uvd_pack_check_f32(const void *segs, int k, const void *chunks, int64_t nchunks, int dtype, float scale, float *out,
                            int32_t *flag, int32_t stamp, void *stream);
int psgd_uvd_check_multi(const void *segs, int k, const void *chunks, int64_t nchunks, int dtype, float scale, int32_t *flag,
                         int32_t stamp, void *stream);

/* out[0] = sum_i fl32(x[i] * x[i]), summed in fp64 in a fixed order (the square of the clip norm of psgd.py:753): two launches,
 * no floating-point atomics, the same bits on every call.  N >= 0; x 4-byte aligned.                                             */
int psgd_uvd_sumsq_f32(const float *x, int64_t N, double *out, void *ws, int64_t ws_bytes, void *stream);

/* psgd.py:757-762 for all parameters in ONE launch, T = the parameters' type, every operation rounded to nearest even on its own:
 *     delta = T(fl32(lr_eff * pre_grad[start + i]));   vs_segs given: delta = T(delta + v[i]);   p[i] = T(p[i] - delta)
 * lr_eff = lr when sumsq is NULL; otherwise lr_eff = fl32(lr * min(max_norm / (sqrt(*sumsq) + tiny), 1)) (:753-754), evaluated in
 * fp64 on the device from the double psgd_uvd_sumsq_f32 left (all-reduced first when the vector is sharded): no host read.
 * pre_grad == NULL (vs_segs required, sumsq must be NULL): p[i] = T(p[i] + v[i]), the perturbation of :723.
 * vs_segs: the segment table of the vs tensors (same sizes and dtype as the parameters), or NULL.                              */
int psgd_uvd_param_update_multi(const void *param_segs, const void *vs_segs, int k, const void *chunks, int64_t nchunks, int dtype,
                                const float *pre_grad, float lr, const double *sumsq, float max_norm, float tiny, void *stream);

/* psgd_uvd_param_update_multi with decoupled weight decay, in the parameters' type: with c = fl32(lr_eff * wd),
 *     delta = T(fl32(lr_eff * pre_grad[start + i]));   vs_segs given: delta = T(delta + v[i]);
 *     wd != 0: delta = T(delta + T(fl32(c * float(p[i]))));   p[i] = T(p[i] - delta).
 * wd == 0 takes no extra rounding step: the bits of psgd_uvd_param_update_multi (which forwards here).  pre_grad == NULL with
 * wd != 0 is PSGD_ERR_BAD_ARG.                                                                                                  */
int psgd_uvd_param_update_multi_wd(const void *param_segs, const void *vs_segs, int k, const void *chunks, int64_t nchunks, int dtype,
                                   const float *pre_grad, float lr, const double *sumsq, float max_norm, float tiny, float wd,
                                   void *stream);

/* ------------------------------------------------- step tail on lists of tensors ---
 * What an optimizer does around per-layer preconditioner calls (class Kron: mnist_with_lenet5.py:54-56 and the finite-difference
 * route of psgd.py:716-727, :734-736, :761) when NO operand is a flat vector: every operand is a list of k fp32 tensors with its own
 * segment table (psgd_multi_tail.hip).  Tables as above; `start` is not read.  All tables of one call describe tensors of the same
 * element counts and share one chunk table; a chunk never runs past the shortest of its segments.  The _f32 entry points take fp32
 * lists only; psgd_multi_widen_check and psgd_multi_param_update_t (below) take a PSGD_DTYPE_* code for the lists that hold parameters
 * of another type, and psgd_multi_narrow_bf16, psgd_multi_sumsq_mixed and psgd_multi_param_update_mixed (further below) serve the
 * layers whose preconditioner runs on bf16 operands.
 * Null tables, k < 0 and nchunks < 0 return PSGD_ERR_BAD_ARG before any HIP call; nchunks == 0 is a no-op (nothing is written).   */
#define PSGD_MULTI_SUMSQ_WS_BYTES  8192   /* workspace of psgd_multi_sumsq_f32 (8-byte aligned, needs no initialisation) */

/* out[0] = sum over every element of every tensor of fl32(x * x), summed in fp64: one partial per workgroup over a fixed set of
 * chunks, lanes -> waves -> workgroup folded in a fixed order, then a one-workgroup fold of the partials: two launches, no atomics,
 * the same bits on every call.  out: 8-byte aligned.  Only the first PSGD_MULTI_SUMSQ_WS_BYTES bytes of ws are touched; a missing,
 * short or misaligned workspace is PSGD_ERR_WORKSPACE (ws == NULL: PSGD_ERR_BAD_ARG).                                            */
int psgd_multi_sumsq_f32(const void *segs, int k, const void *chunks, int64_t nchunks, double *out, void *ws, int64_t ws_bytes,
                         void *stream);

/* For every element of every parameter, in ONE launch, every operation rounded to nearest even on its own:
 *     delta = fl32(lr_eff * g[i]);   vs_segs given: delta = fl32(delta + v[i]);   p[i] = fl32(p[i] - delta)
 * lr_eff = lr when sumsq is NULL; otherwise lr_eff = fl32(lr * min(max_norm / (sqrt(*sumsq) + tiny), 1)), evaluated in fp64 on the
 * device from the double psgd_multi_sumsq_f32 left: no host read; a NaN *sumsq makes lr_eff NaN.
 * grad_segs == NULL (vs_segs required, sumsq must be NULL): p[i] = fl32(p[i] + v[i]), the perturbation of psgd.py:723.          */
int psgd_multi_param_update_f32(const void *param_segs, const void *grad_segs, const void *vs_segs, int k, const void *chunks,
                                int64_t nchunks, float lr, const double *sumsq, float max_norm, float tiny, void *stream);

/* h[i] = fl32(fl32(a[i] - b[i]) * s) and, when v_segs and x_segs are given (both or neither), x[i] = fl32(v[i] * s): the
 * finite-difference dG = (g' - g) / delta and dX = v / delta of psgd.py:727, :734-736 with s = 1 / delta, in ONE launch.         */
int psgd_multi_diff_scale_f32(const void *a_segs, const void *b_segs, const void *h_segs, const void *v_segs, const void *x_segs,
                              int k, const void *chunks, int64_t nchunks, float s, void *stream);

/* Momentum of class Kron: m[i] = fl32(fl32(beta * m[i]) + fl32(omb * g[i])) for every element of every tensor, in ONE launch, every
 * operation rounded on its own.  beta and omb are separate arguments: the caller passes omb = float(1) - beta, rounded once on the
 * host (the convention of psgd_uvd_pack_blend_f32).  beta == 0 does NOT read m: m[i] = fl32(omb * g[i]), whatever m held.          */
int psgd_multi_blend_f32(const void *m_segs, const void *g_segs, int k, const void *chunks, int64_t nchunks, float beta, float omb,
                         void *stream);

/* The guarded step of class Kron: one to three lists (segs1 and segs2 may be NULL; their scales are then not read) in ONE launch.
 * For every element of list j, y = fl32(x * scale_j); where scale_j != 1, y is stored back in place (a list with scale_j == 1 is
 * only read).  flag != NULL: when any y is +-Inf or NaN (a finite input that overflows under its scale counts), stamp is stored to
 * *flag -- the flag contract of psgd_uvd_pack_check_f32: one 4-byte aligned device word that is never zeroed, every writer stores
 * the same value with an ordinary store, no atomics, "bad" is *flag == stamp after the launch has completed.  flag != NULL with
 * stamp <= 0 is PSGD_ERR_BAD_ARG.  flag == NULL is a pure rescale (stamp is ignored); all scales of the given lists equal to 1 is
 * then PSGD_ERR_BAD_ARG: there is nothing to do.                                                                                  */
int psgd_multi_scale_check_f32(const void *segs0, const void *segs1, const void *segs2, float scale0, float scale1, float scale2,
                               int k, const void *chunks, int64_t nchunks, int32_t *flag, int32_t stamp, void *stream);

/* psgd_multi_param_update_f32 with decoupled weight decay: with c = fl32(lr_eff * wd),
 *     delta = fl32(lr_eff * g[i]);   vs_segs given: delta = fl32(delta + v[i]);
 *     wd != 0: delta = fl32(delta + fl32(c * p[i]));   p[i] = fl32(p[i] - delta).
 * wd == 0 takes no extra rounding step: the bits of psgd_multi_param_update_f32 (which forwards here).  grad_segs == NULL with
 * wd != 0 is PSGD_ERR_BAD_ARG.                                                                                                  */
int psgd_multi_param_update_wd_f32(const void *param_segs, const void *grad_segs, const void *vs_segs, int k, const void *chunks,
                                   int64_t nchunks, float lr, const double *sumsq, float max_norm, float tiny, float wd,
                                   void *stream);

/* Parameters of type T = bfloat16 or float16 (dtype = PSGD_DTYPE_BF16 / PSGD_DTYPE_F16) in class Kron: factors, momentum buffers and
 * everything the preconditioner reads stay fp32, so once per step the T lists of the step are widened, in ONE launch:
 *     dst_j[i] = fl32(float(src_j[i]) * scale_j)          for one to three (src_j, dst_j) pairs of lists,
 * src_j tensors of type T (aligned to their element), dst_j fp32 tensors of the same element counts.  An absent list passes NULL
 * for BOTH of its tables (list 0 is required); a source without a destination, or the reverse, is PSGD_ERR_BAD_ARG.
 * flag != NULL: when any value WRITTEN is +-Inf or NaN (a finite input that overflows under its scale counts, and so does an fp16
 * +-Inf), stamp is stored to *flag -- the flag contract of psgd_multi_scale_check_f32: one 4-byte aligned device word that is never
 * zeroed, every writer stores the same value with an ordinary store, no atomics, "bad" is *flag == stamp after the launch has
 * completed.  flag != NULL with stamp <= 0 is PSGD_ERR_BAD_ARG.  flag == NULL only widens (stamp is ignored).
 * dtype == PSGD_DTYPE_F32 is PSGD_ERR_BAD_ARG: fp32 lists are scaled and judged in place by psgd_multi_scale_check_f32.            */
int psgd_multi_widen_check(const void *src0, const void *src1, const void *src2, const void *dst0, const void *dst1, const void *dst2,
                           float scale0, float scale1, float scale2, int k, const void *chunks, int64_t nchunks, int dtype,
                           int32_t *flag, int32_t stamp, void *stream);

/* psgd_multi_param_update_wd_f32 on parameters and vs of type T with fp32 gradients, every operation rounded to nearest even on its
 * own (the chain of psgd_uvd_param_update_multi_wd): with c = fl32(lr_eff * wd),
 *     delta = T(fl32(lr_eff * g[i]));   vs_segs given: delta = T(delta + v[i]);
 *     wd != 0: delta = T(delta + T(fl32(c * float(p[i]))));   p[i] = T(p[i] - delta).
 * grad_segs == NULL (vs_segs required, sumsq NULL, wd == 0): p[i] = T(p[i] + v[i]).  lr_eff, sumsq, max_norm, tiny and the rejected
 * combinations are those of psgd_multi_param_update_wd_f32; wd == 0 takes no extra rounding step.  dtype == PSGD_DTYPE_F32 forwards
 * to psgd_multi_param_update_wd_f32 (every operand fp32); an unknown dtype is PSGD_ERR_BAD_ARG.                                   */
int psgd_multi_param_update_t(const void *param_segs, const void *grad_segs, const void *vs_segs, int k, const void *chunks,
                              int64_t nchunks, int dtype, float lr, const double *sumsq, float max_norm, float tiny, float wd,
                              void *stream);

/* Vector layers of class Kron.  A rank-1 parameter of length n is the reference's layer of shape [1, n] in the (dense, scaling)
 * format: Ql is 1 x 1, qr is [1, n] (psgd.py:276-322).  All k vectors of a model in ONE launch each.  Four segment tables of k
 * entries (the Seg of the step-tail kernels; `start` is not read): ql_segs names k tensors of one fp32 element, the other three k
 * fp32 tensors of n_i >= 2 elements each.  One workgroup of 256 threads owns one vector (workgroup b takes vectors b, b + grid, ...
 * under the grid cap of the step-tail kernels), so a vector's result depends on its own length and values only: not on k, not on
 * its place in the list, not on where its tensors start.  min_count is the smallest n_i as the caller knows it: the tables live
 * on the device and are not read on the host.  A null table, k < 1 or min_count < 2 is PSGD_ERR_BAD_ARG before any HIP call;
 * whatever the caller says, a segment of fewer than 2 elements moves nothing.  Nothing allocates or synchronises.
 *
 * Update, in place, fp32 in the reference's order (psgd.py:288-307 with M = 1):
 *     rho = sqrt(ql / max(qr));   ql' = ql / rho;   qr' = rho * qr;
 *     A = (ql' * dG) * qr';   Bt = (dX / ql') * (1 / qr');   grad1 = sum(A A) - sum(Bt Bt);   grad2 = A A - Bt Bt;
 *     ql = ql' - (step1 * grad1) * ql',  step1 = step / (|grad1| + tiny);
 *     qr = qr' - (step2 * grad2) * qr',  step2 = step / (max|grad2| + tiny).
 * The two sums add the fp32 squares in fp64, per lane and then lanes -> waves -> workgroup in a fixed order (no atomics: the same
 * bits on every call), and grad1 is their fp64 difference rounded once; the maxima propagate NaN as tf.reduce_max does.  A vector
 * of a million elements is correct and slow (one workgroup): long vectors are not what this is for.                              */
int psgd_multi_vec_update_f32(const void *ql_segs, const void *qr_segs, const void *dx_segs, const void *dg_segs, int k,
                              int64_t min_count, float step, float tiny, void *stream);

/* out[i] = fl32(fl32(fl32(ql * ql) * g[i]) * fl32(qr[i] * qr[i])) for every vector: precond_grad_kron on the [1, n] layer, the M < N
 * branch of psgd.py:318-319 and :322.  out_segs may name the tensors of g_segs (in place).                                          */
int psgd_multi_vec_apply_f32(const void *ql_segs, const void *qr_segs, const void *g_segs, const void *out_segs, int k,
                             int64_t min_count, void *stream);

/* bf16-operand layers of class Kron(operands="bfloat16"): large (dense, dense) layers take dX, dG and the gradient as bf16 tensors
 * (psgd_kron_dd_update_bf16, psgd_kron_dd_apply_bf16) and return a bf16 preconditioned gradient; everything else stays fp32.
 *
 * psgd_multi_narrow_bf16 is psgd_multi_widen_check in the other direction, without a flag: in ONE launch
 *     dst_j[i] = bf16(src_j[i])          for one to three (src_j, dst_j) pairs of lists,
 * src_j fp32 tensors, dst_j bf16 tensors of the same element counts, each aligned to its element only.  Round to nearest even,
 * the bits of torch's .to(torch.bfloat16): NaN -> the quiet NaN 0x7FC0, a finite value beyond the bf16 range -> +-Inf, subnormals
 * kept.  An absent list passes NULL for BOTH of its tables (list 0 is required); a source without a destination, or the reverse,
 * is PSGD_ERR_BAD_ARG.  Nothing is judged: the guard of a step has seen the fp32 values.                                          */
int psgd_multi_narrow_bf16(const void *src0, const void *src1, const void *src2, const void *dst0, const void *dst1, const void *dst2,
                           int k, const void *chunks, int64_t nchunks, void *stream);

/* MIXED lists: a list whose tensors are fp32 or bf16, tensor by tensor.  The `start` field of a segment, which no entry point of
 * this section reads otherwise, holds that segment's PSGD_DTYPE_F32 or PSGD_DTYPE_BF16; its pointer is aligned to its element and
 * its count is in elements.  The table lives on the device, so the host cannot judge the codes: a segment with any other code is
 * skipped (it adds nothing to the sum, and its parameters are not touched).
 *
 * psgd_multi_sumsq_mixed: psgd_multi_sumsq_f32 on a mixed list, sum of fl32(float(x) * float(x)) in fp64: the same partial / fold
 * structure, workspace (PSGD_MULTI_SUMSQ_WS_BYTES), argument checks and fixed order.  Two bit contracts: with every segment fp32
 * the result has the bits of psgd_multi_sumsq_f32 on the same tensors; a bf16 segment is summed in the order in which
 * psgd_multi_sumsq_f32 sums a 16-byte aligned fp32 tensor holding the widened values (what psgd_multi_widen_check with scale 1
 * writes into a fresh buffer), wherever the bf16 tensor itself starts.                                                            */
int psgd_multi_sumsq_mixed(const void *segs, int k, const void *chunks, int64_t nchunks, double *out, void *ws, int64_t ws_bytes,
                           void *stream);

/* psgd_multi_param_update_t with a mixed list as the gradients: parameters and vs of type T = dtype (PSGD_DTYPE_F32, _BF16 or
 * _F16; for F32 the chain is that of psgd_multi_param_update_wd_f32), gradient segment i fp32 or bf16 as grad_segs[i].start says,
 * read as float(g): delta = T(fl32(lr_eff * float(g[i]))), and everything after it as in psgd_multi_param_update_t.  With every
 * segment fp32 the bits are those of psgd_multi_param_update_t; with bf16 segments those of widening them exactly first.
 * grad_segs == NULL is PSGD_ERR_BAD_ARG (the perturbation p + v has no gradient and keeps psgd_multi_param_update_t), and so is
 * an unknown dtype; lr_eff, sumsq, max_norm, tiny and wd as in psgd_multi_param_update_wd_f32.                                    */
int psgd_multi_param_update_mixed(const void *param_segs, const void *grad_segs, const void *vs_segs, int k, const void *chunks,
                                  int64_t nchunks, int dtype, float lr, const double *sumsq, float max_norm, float tiny, float wd,
                                  void *stream);

/* ------------------------------------------------- bf16 parameters written with stochastic rounding ---
 * param_rounding="stochastic" of class UVd and class Kron.  A bf16 parameter under round to nearest ignores every update below half
 * its spacing; these three entry points form the update ONCE in fp32 and narrow it ONCE, stochastically.  With w = float(p[i]) and
 * c = fl32(lr_eff * wd), every operation rounded to fp32 on its own:
 *     d = fl32(lr_eff * float(g[i]));   vs_segs given: d = fl32(d + float(v[i]));   wd != 0: d = fl32(d + fl32(c * w));
 *     x = fl32(w - d);   p[i] = SR(x).
 * SR(x) is the stochastic narrowing of the bf16-stored states, (bits(x) + u) >> 16 with u the top 16 bits of their counter hash of
 * (key, idx), where key is the rounding stream of (seed, tensor id 16 = "parameters") and idx = index0 + start + i, start being
 * the `start` field of the PARAMETER segment (which the psgd_multi_* entry points above never read): the element's index in the
 * optimizer's flat parameter order.  The stored bits therefore do not depend on the grid, the chunk table, where a tensor starts
 * or how a flat vector is split over ranks (index0 = the rank's first row).  A NaN x is stored as 0x7FC0; +-Inf stays +-Inf; an x
 * that is exactly a bf16 value is never changed; a finite x beyond the largest finite bf16 value may carry into +-Inf -- its upper
 * neighbour, so the correct stochastic outcome.  lr_eff, sumsq, max_norm and tiny are evaluated exactly as in the siblings (a NaN
 * *sumsq makes every parameter NaN).  Same tables, launch shape and accesses as the siblings; one hash per written element.
 * dtype must be PSGD_DTYPE_BF16 (float16 needs its own narrowing for its subnormal range) and index0 >= 0: anything else is
 * PSGD_ERR_BAD_ARG, and so is a missing gradient -- the perturbation p + v and its undo round to nearest and keep the siblings.
 * Other argument checks as in the siblings.  Nothing allocates or synchronises.
 *
 * psgd_uvd_param_update_multi_sr: psgd_uvd_param_update_multi_wd (flat fp32 pre_grad, g[i] = pre_grad[start + i]).
 * psgd_multi_param_update_sr: psgd_multi_param_update_t (a list of fp32 gradients).
 * psgd_multi_param_update_mixed_sr: psgd_multi_param_update_mixed (gradient segment i fp32 or bf16 as grad_segs[i].start says).   */
int psgd_uvd_param_update_multi_sr(const void *param_segs, const void *vs_segs, int k, const void *chunks, int64_t nchunks, int dtype,
                                   const float *pre_grad, float lr, const double *sumsq, float max_norm, float tiny, float wd,
                                   uint64_t seed, int64_t index0, void *stream);
int psgd_multi_param_update_sr(const void *param_segs, const void *grad_segs, const void *vs_segs, int k, const void *chunks,
                               int64_t nchunks, int dtype, float lr, const double *sumsq, float max_norm, float tiny, float wd,
                               uint64_t seed, int64_t index0, void *stream);
int psgd_multi_param_update_mixed_sr(const void *param_segs, const void *grad_segs, const void *vs_segs, int k, const void *chunks,
                                     int64_t nchunks, int dtype, float lr, const double *sumsq, float max_norm, float tiny, float wd,
                                     uint64_t seed, int64_t index0, void *stream);

/* The probe vectors of class Kron(preconditioner_fit="whitening"): k contiguous fp32 tensors filled with standard normal draws in
 * ONE launch (psgd_multi_tail.hip).  Element i of segment s gets fl32(scale * z_g), g = index0 + out_segs[s].start + i: the
 * element's index in the concatenation of the list (this entry point reads `start`, as the stochastic updates above do), and z_g
 * depends on (seed, g) alone -- not on how the list is cut into tensors, where they start, the chunk table or the grid.
 * Stream: K = the key of (seed, tensor id 17 = "probe vectors") built as for the rounding streams; pair j = g >> 1 takes one 64-bit
 * hash h = mix64(K + 0x9E3779B97F4A7C15 * (j + 1)) (mix64: the splitmix64 finaliser); u1 = ((h >> 32) + 1) * 2^-32 in (0, 1],
 * r = sqrt(-2 ln u1) <= 6.67, theta = 2 pi (h & 0xFFFFFFFF) 2^-32; even g takes r cos theta, odd g takes r sin theta.  fp32
 * arithmetic with the full-precision logf / log1pf / sqrtf / sincospif (within a few fp32 ulps of the float64 evaluation,
 * counter_randn in Python).  Every value written is finite for a scale of ordinary size: no Inf and no NaN whatever the seed.
 * Argument checks before any HIP call: null tables, k < 1, nchunks < 0, index0 < 0 or a scale that is not finite are
 * PSGD_ERR_BAD_ARG.  nchunks == 0 is PSGD_OK and writes nothing.  Nothing allocates or synchronises. */
int psgd_multi_randn_f32(const void *out_segs, int k, const void *chunks, int64_t nchunks, uint64_t seed, int64_t index0, float scale,
                         void *stream);

/* Tuning knobs for experiments (not part of the stable ABI).
 * key 0: streaming policy (0 = automatic: non-temporal when U,V exceed the Infinity Cache,
 *        1 = never non-temporal, 2 = always non-temporal).
 * key 1: cap on blocks per CU for the sweeps (0 = occupancy query).
 * key 2: r x r algebra of the update: 0 (default) one-row-per-lane register kernel, 1 = block-cooperative reference.
 * key 3: short sweeps: tiles a wave should stream at least (default 8; grids shrink to that, never below one block per CU). */
int psgd_set_tuning(int key, int value);

/* Live kernel timing for bench.py (measurement aid, not part of the reference's surface).
 * While enabled, every sweep-kernel launch is bracketed by HIP events recorded on the launch
 * stream.  psgd_prof_collect() waits for the recorded events of `slot`, returns the summed
 * kernel time and the launch count since the last collect, and clears the slot.
 * It is the only call here that synchronises with the device.                            */
#define PSGD_PROF_APPLY_S1   0
#define PSGD_PROF_APPLY_S2   1
#define PSGD_PROF_APPLY_S3   2
#define PSGD_PROF_UPDATE_S1  3
#define PSGD_PROF_UPDATE_S2  4
#define PSGD_PROF_UPDATE_S3  5
int psgd_prof_enable(int on);
int psgd_prof_collect(int slot, double *total_ms, int *count);

/* ------------------------------------------------------------ sparse LU ---
 * P = Q'Q, Q = L U, L = [L1 0; L2 diag(l3)], U = [U1 U2; 0 diag(u3)]  (psgd.py:396-404).
 * Layout is the reference's: L12 = [L1; L2] is [N, r] row-major (L1 lower triangular), U12 = [U1, U2]
 * is [r, N] row-major (U1 upper triangular), l3 and u3 are [N - r].  1 <= r <= PSGD_SPLU_MAX_RANK
 * (64 since round 5: ranks above 32 take 64-row tiles, one workgroup per CU, and about 0.6 of the rate of the ranks below),
 * N >= r.  L12 (and L12_new) must be 16-byte aligned; vectors need 4-byte alignment only.
 *
 * psgd_splu_apply_f32  replaces precond_grad_splu(L12, l3, U12, u3, grads)   psgd.py:483-524
 *   g, out: the concatenated gradient / preconditioned gradient, [N] (the list <-> flat vector plumbing of
 *   :495-497,:518-522 stays on the host side).  out must not alias g.
 * psgd_splu_update_f32 replaces update_precond_splu(L12, l3, U12, u3, dxs, dgs, step)   psgd.py:396-480
 *   dx, dg: the concatenated perturbations [N].  Pure like the reference: the new factors go to the *_new
 *   buffers (which may alias the inputs for an in-place update).  tiny = psgd.py:22 `_tiny`.          */
int64_t psgd_splu_workspace_bytes(int64_t N, int r);
int psgd_splu_apply_f32(const float *L12, const float *l3, const float *U12, const float *u3, const float *g,
                        float *out, int64_t N, int r, void *ws, int64_t ws_bytes, void *stream);
int psgd_splu_update_f32(const float *L12, const float *l3, const float *U12, const float *u3, const float *dx,
                         const float *dg, float *L12_new, float *l3_new, float *U12_new, float *u3_new, int64_t N,
                         int r, float step, float tiny, void *ws, int64_t ws_bytes, void *stream);

/* Stage forms of the two calls above, for tail rows sharded over several GPUs (one process per GPU): every rank passes
 * its local tensors -- L12 = [L1; its rows of L2] ([r + n_local, r]), U12 = [U1, its columns of U2], its slices of
 * l3 / u3, and flat vectors [the r corner entries (replicated); its slice of the tail] -- with N = r + n_local, and
 * all-reduces the workspace region psgd_splu_ws_region(which, stage) reports after stage `stage`:
 *   which 0 (fp64, SUM): stage 1: r sums (U2 x2); stage 2: 2r sums (apply uses the first r); stage 3: r sums (update)
 *   which 1 (fp32, MAX): stage 3: 4 maxima (update)
 * Every rank then redoes the r x r corner algebra on identical inputs and gets identical corner results.
 * psgd_splu_stage1_f32 serves both paths (x = the flat gradient for the apply, dg for the update).
 * has_tail (update stage 4): the GLOBAL problem has tail rows (N_global > r).                                       */
int psgd_splu_ws_region(int which, int stage, int64_t N, int r, int64_t *offset_bytes, int64_t *count);
/* all-gather + fold form (protocol (a) above): PSGD_WS_SEND_F64 regions for stage 1 (r sums), 2 (2r sums) and
 * 3 ([r sums | 4 maxima] in one region: three exchanges per update, two per apply).                                */
int psgd_splu_fold_gathered_f64(int stage, const double *gathered, int world, int64_t N, int r, void *ws,
                                int64_t ws_bytes, void *stream);
int psgd_splu_stage1_f32(const float *U12, const float *x, int64_t N, int r, void *ws, int64_t ws_bytes, void *stream);
int psgd_splu_apply_stage2_f32(const float *L12, const float *l3, const float *U12, const float *u3, const float *g,
                               float *out, int64_t N, int r, void *ws, int64_t ws_bytes, void *stream);
int psgd_splu_apply_stage3_f32(const float *L12, const float *l3, const float *U12, const float *u3, float *out,
                               int64_t N, int r, void *ws, int64_t ws_bytes, void *stream);
int psgd_splu_update_stage2_f32(const float *L12, const float *l3, const float *U12, const float *u3, const float *dx,
                                const float *dg, int64_t N, int r, void *ws, int64_t ws_bytes, void *stream);
int psgd_splu_update_stage3_f32(const float *L12, const float *l3, const float *U12, const float *u3, const float *dx,
                                const float *dg, int64_t N, int r, void *ws, int64_t ws_bytes, void *stream);
int psgd_splu_update_stage4_f32(const float *L12, const float *l3, const float *U12, const float *u3, const float *dx,
                                const float *dg, float *L12_new, float *l3_new, float *U12_new, float *u3_new, int64_t N,
                                int r, float step, float tiny, int has_tail, void *ws, int64_t ws_bytes, void *stream);

/* ------------------------------------------------- sparse LU, bf16 state ---
 * The same preconditioner with L12 ([N, r]), U12 ([r, N]), l3 and u3 ([N - r]) STORED as bf16 (psgd_splu_bf16.hip); dx, dg, g
 * and out stay fp32.  Elements are widened when loaded and narrowed once when written; all arithmetic is fp64.
 * 1 <= r <= PSGD_UVD_MAX_RANK (PSGD_ERR_RANK above), N >= r (N == r: no tail, l3 / u3 may be null).  The four state pointers
 * (inputs and outputs) must be 16-byte aligned (PSGD_ERR_ALIGN).  The workspace (psgd_splu_bf16_workspace_bytes, 256-byte
 * aligned, about 0.6 MiB whatever N) has a layout of its own.  Argument checks return before any HIP call.
 * psgd_splu_update_bf16 is pure: the new factors go to the *_new buffers, which must not overlap the inputs or one another
 * (PSGD_ERR_BAD_ARG).  The balance of psgd.py:411-417 rescales every element, so every element of the state is re-rounded
 * by every update.  rounding: 0 = round to nearest even, 1 = stochastic, the stream keyed by (seed, tensor, flat element
 * index) as in the bf16 UVd state, with tensor ids 8, 9, 10, 11 for L12, l3, U12, u3
 * (psgd_uvd_bf16_rounding_key(seed, id) is the key of a stream).  NaN and Inf are stored as they are.                    */
int64_t psgd_splu_bf16_workspace_bytes(int64_t N, int r);
int psgd_splu_apply_bf16(const void *L12, const void *l3, const void *U12, const void *u3, const float *g, float *out,
                         int64_t N, int r, void *ws, int64_t ws_bytes, void *stream);
int psgd_splu_update_bf16(const void *L12, const void *l3, const void *U12, const void *u3, const float *dx,
                          const float *dg, void *L12_new, void *l3_new, void *U12_new, void *u3_new, int64_t N, int r,
                          float step, float tiny, int rounding, uint64_t seed, void *ws, int64_t ws_bytes, void *stream);

/* ----------------------------------------------------------------- Kron ---
 * P = kron(Qr'Qr, Ql'Ql) with dense upper-triangular Ql [M,M], Qr [N,N]
 * (psgd.py:156-192).  G, dX, dG are [M,N] row-major.                       */

int64_t psgd_kron_dd_workspace_bytes(int M, int N);

/* Experiment knobs (not stable ABI; defaults in brackets).  Settled A/B keys were frozen into constants in round 4 (5, 8, 10, 13-15,
 * 17, 19, 20).  Keys 1, 4, 12, 16 change what prepared state in a workspace means: prepare again after changing them.
 *  0 fp32 GEMM tile: [0] auto, 1 = 64, 2 = 128, 3 = 32        1 [1] 128-tile products as fp32-accurate bf16 x 3 GEMMs, 0 = exact fp32 MFMA
 *  2 solve strips: [0] register-resident, 1 = LDS-resident      3 32-tile products: [1] k_gemm_small (ring of 4 K tiles), 0 = generic body
 *  4 [1] large products on operands split ONCE into planes (k_split3 / k_gemm_p3), 0 = split inside every GEMM tile
 *  6 [1] K split of the tail of the gradient grid (large fp32 update, M = N), 0 = whole tiles
 *  7 bits [3]: 1 = batched small update shares launches between product and solve stages; 2 = single small updates as a batch of one
 *  9 [1] large updates fork the products of psgd.py:173 onto a side stream (events only: capturable), 0 = one stream
 * 11 [1] M, N >= 2048: the solves of :174 as products with explicit inverses of diagonal blocks, 0 = substitution strips
 * 12 plane format: [2] f16 x 2 (x 2^e = h + 2^-11 M) in the large apply and update, 1 = apply only, 0 = bf16 x 3 everywhere
 * 16 [1] chained products write fp32 + max|C| and a split launch makes exact-scale planes, 0 = epilogue planes at a bound scale
 * 23 [1] 512-blocks of an inverse from one strip launch (k_tri_inv512), 0 = k_tri_inv128 + doubling levels 128, 256
 * 24 [2048] block size h of the blocked solves on inverses of diagonal h-blocks, 0 = whole inverses, one product per solve;
 *    a value that would make more than 4 block columns per side (ceil(max(M, N) / h) > 4) is replaced by 2048 for that call
 * 25 [-1] stream order of the inverse route: by shape (both inversions first from 4096^2 on), 0 / 1 = products / inversions first
 * 27 [1] the factor updates (:179) of the large update walk their tiles in 4 x 4 patches per XCD (from 32 x 32 tiles on), 0 = whole tile rows
 * 28 [1] chained f16 x 2 plane products write their planes from the epilogue at TILE scales (each 128 x 128 tile at its own maximum; the
 *    consumer's K loop shifts its accumulators when the scale changes), 0 = fp32 out + max|C| + a split launch (one scale per matrix)
 * 29 [1] large fp32 update with both inversions first: dX's planes on the side stream ahead of Ql's inversion, 0 = on the caller's stream
 * 30 [-1] (round 6) large fp32 update: 1 = the products of psgd.py:173 on a third stream from the fork point on (beside both inversions),
 *      0 = behind Ql's inversion on the side stream, -1 = 1 when both factors reach 4096
 * 31 [1] (round 6) large fp32 update on the tile-scale inverse route: the prologue is rho + ONE sweep (balanced upper tiles in fp32, both
 *      plane forms of both factors at tile scales, the inverted 32-blocks) and dX's / dG's planes are one sweep each at tile scales;
 *      0 = the round-5 prologue (two sweeps, one scale per factor; max|dX|, max|dG| launches ahead of their splits)
 * 32 [1] (round 6, shapes below key 30's rule) dX's and dG's planes on the third stream, Ql's inversion from the fork point on
 * 33 [1] (round 6) M != N: every tile of the smaller factor's gradient is split along its K (the longer side) into chunks as long as the
 *      other gradient's tiles; 0 = whole tiles
 * 34 [1] (round 6) products of the blocked solves with at most 256 output tiles and >= 64 K steps: two workgroups per tile; 0 = one */
int psgd_kron_set_tuning(int key, int value);

/* _precond_grad_dense_dense(Ql, Qr, Grad)  psgd.py:182-192.
 * Association order follows the reference: M < N uses ((Ql'Ql) G) Qr' Qr,
 * otherwise Ql' (Ql (G (Qr'Qr))).  Ql, Qr are upper-triangular by the reference's
 * invariant (psgd.py:175-179); entries below the diagonal are not read.     */
int psgd_kron_dd_apply_f32(const float *Ql, const float *Qr, const float *G,
                           float *out, int M, int N, void *ws,
                           int64_t ws_bytes, void *stream);
/* The same call in two halves: what depends on the factors only (their Grams, kept in ws) and what depends on the
 * gradient.  psgd_kron_dd_apply_f32 == prepare + apply_prepared; a caller that applies unchanged factors to several
 * gradients prepares once.  For M, N <= 512 (every launch latency-bound) BOTH Grams are prepared and the gradient half
 * is two products, (Ql'Ql) G (Qr'Qr) -- the reference's association on one side, re-associated on the other.        */
int psgd_kron_dd_prepare_f32(const float *Ql, const float *Qr, int M, int N, void *ws,
                             int64_t ws_bytes, void *stream);
int psgd_kron_dd_apply_prepared_f32(const float *Ql, const float *Qr, const float *G, float *out,
                                    int M, int N, void *ws, int64_t ws_bytes, void *stream);
/* The apply for factors that are NEW on every call (the reference's pattern: an apply right after an update): no Gram, nothing
 * prepared -- out = Ql' (Ql ((G Qr') Qr)) as four chained triangular products where the f16 x 2 plane products apply (large
 * layers: 4096^2 1.01 -> 0.93 ms); the same as psgd_kron_dd_apply_f32 elsewhere.  Leaves no prepared state in ws:
 * psgd_kron_dd_apply_prepared_f32 needs psgd_kron_dd_prepare_f32 (or psgd_kron_dd_apply_f32) for these factors first.  */
int psgd_kron_dd_apply_direct_f32(const float *Ql, const float *Qr, const float *G, float *out, int M, int N, void *ws,
                                  int64_t ws_bytes, void *stream);
/* 1 when the call above is a path of its own for this shape under the current tuning, 0 when it is psgd_kron_dd_apply_f32 */
int psgd_kron_dd_apply_direct_distinct(int M, int N);

/* The routes the Kron dense (x) dense calls take for an M x N layer under the current tuning keys (psgd_kron_set_tuning,
 * psgd_kron_bf16_set_tuning), as a mask of the bits below; PSGD_ERR_SHAPE for M <= 0 or N <= 0.  Host only, no HIP call.
 * Each bit is the predicate the launch code branches on, so a test can pin the shapes on either side of every threshold. */
#define PSGD_KRON_ROUTE_SMALL          (1 << 0)   /* psgd_kron_dd_update_f32 runs as a batch of one (small layers)            */
#define PSGD_KRON_ROUTE_PLANES_APPLY   (1 << 1)   /* the fp32 apply's products on operand planes                              */
#define PSGD_KRON_ROUTE_PLANES_UPDATE  (1 << 2)   /* the fp32 update's products on operand planes                             */
#define PSGD_KRON_ROUTE_INV_SOLVES     (1 << 3)   /* the fp32 update's solves through explicit inverses of diagonal blocks    */
#define PSGD_KRON_ROUTE_INV_FIRST      (1 << 4)   /* ... with both inversions ahead of the products of psgd.py:173            */
#define PSGD_KRON_ROUTE_BG_FRONT       (1 << 5)   /* ... and those products on a third stream from the fork point on          */
#define PSGD_KRON_ROUTE_FACTOR_TS      (1 << 6)   /* ... with the fused prologue: the factors' planes at tile scales         */
#define PSGD_KRON_ROUTE_GRAD_RECT      (1 << 7)   /* M != N: the smaller gradient's tiles split along their long K           */
#define PSGD_KRON_ROUTE_APPLY_DIRECT   (1 << 8)   /* psgd_kron_dd_apply_direct_f32 is a path of its own                       */
#define PSGD_KRON_ROUTE_BF16_INV       (1 << 9)   /* psgd_kron_dd_update_bf16's fp32 solves through explicit inverses        */
#define PSGD_KRON_ROUTE_RECT_CHUNKS_SHIFT 12      /* bits 12-15: the K chunks per tile of PSGD_KRON_ROUTE_GRAD_RECT           */
#define PSGD_KRON_ROUTE_RECT_CHUNKS_MASK  (15 << PSGD_KRON_ROUTE_RECT_CHUNKS_SHIFT)
int psgd_kron_dd_route_flags(int M, int N);

/* _update_precond_dense_dense(Ql, Qr, dX, dG, step)  psgd.py:156-179.
 * Pure: Ql, Qr are read, the new factors are written to QlOut, QrOut.      */
int psgd_kron_dd_update_f32(const float *Ql, const float *Qr, const float *dX,
                            const float *dG, float *QlOut, float *QrOut,
                            int M, int N, float step, float tiny, void *ws,
                            int64_t ws_bytes, void *stream);

/* Batched forms for networks of small layers (LeNet5: mnist_with_lenet5.py:12-16, where every
 * GEMM is launch-bound): the same stage of every layer runs in ONE launch.  Arrays are HOST
 * arrays of `count` device pointers / sizes; `ws` holds the per-layer workspaces back to back
 * (psgd_kron_dd_workspace_bytes_batched).  Results are identical to the per-layer calls.
 * The batched update requires M, N <= 512 for every layer (PSGD_ERR_SHAPE otherwise).       */
int64_t psgd_kron_dd_workspace_bytes_batched(const int *M, const int *N, int count);
int psgd_kron_dd_apply_batched_f32(const float *const *Ql, const float *const *Qr,
                                   const float *const *G, float *const *out,
                                   const int *M, const int *N, int count,
                                   void *ws, int64_t ws_bytes, void *stream);
int psgd_kron_dd_prepare_batched_f32(const float *const *Ql, const float *const *Qr, const int *M,
                                     const int *N, int count, void *ws, int64_t ws_bytes, void *stream);
int psgd_kron_dd_apply_prepared_batched_f32(const float *const *Ql, const float *const *Qr,
                                            const float *const *G, float *const *out,
                                            const int *M, const int *N, int count,
                                            void *ws, int64_t ws_bytes, void *stream);
int psgd_kron_dd_update_batched_f32(const float *const *Ql, const float *const *Qr,
                                    const float *const *dX, const float *const *dG,
                                    float *const *QlOut, float *const *QrOut,
                                    const int *M, const int *N, int count,
                                    float step, float tiny,
                                    void *ws, int64_t ws_bytes, void *stream);

/* Sparse Kronecker factors (psgd.py:198-391), canonical orientations; the dispatcher's mirrored
 * formats (psgd.py:86,102,104 / :128,144,146) call these on transposed views.
 *   fmt 0 "ds": (dense, scaling)          Ql [M,M], qr [N]          psgd.py:276-322
 *   fmt 1 "nd": (normalization, dense)    ql [2,M], Qr [N,N]        psgd.py:198-270
 *   fmt 2 "ns": (normalization, scaling)  ql [2,M], qr [N]          psgd.py:328-391
 * dX, dG, G are strided views: element (m,n) at p[m*rs + n*cs] (dX and dG share strides).
 * Factor outputs and `out` are contiguous ([M,M] / [2,M] / [N] / [N,N] / [M,N]).  Pure: inputs
 * are never written.                                                                        */
int64_t psgd_kron_sparse_workspace_bytes(int fmt, int M, int N);
int psgd_kron_ds_update_f32(const float *Ql, const float *qr, const float *dX, const float *dG,
                            int64_t xrs, int64_t xcs, float *QlOut, float *qrOut, int M, int N,
                            float step, float tiny, void *ws, int64_t ws_bytes, void *stream);
int psgd_kron_ds_apply_f32(const float *Ql, const float *qr, const float *G, int64_t grs,
                           int64_t gcs, float *out, int M, int N, void *ws, int64_t ws_bytes,
                           void *stream);
int psgd_kron_nd_update_f32(const float *ql, const float *Qr, const float *dX, const float *dG,
                            int64_t xrs, int64_t xcs, float *qlOut, float *QrOut, int M, int N,
                            float step, float tiny, void *ws, int64_t ws_bytes, void *stream);
int psgd_kron_nd_apply_f32(const float *ql, const float *Qr, const float *G, int64_t grs,
                           int64_t gcs, float *out, int M, int N, void *ws, int64_t ws_bytes,
                           void *stream);
int psgd_kron_ns_update_f32(const float *ql, const float *qr, const float *dX, const float *dG,
                            int64_t xrs, int64_t xcs, float *qlOut, float *qrOut, int M, int N,
                            float step, float tiny, void *ws, int64_t ws_bytes, void *stream);
int psgd_kron_ns_apply_f32(const float *ql, const float *qr, const float *G, int64_t grs,
                           int64_t gcs, float *out, int M, int N, void *ws, int64_t ws_bytes,
                           void *stream);

/* bf16-operand variant of _precond_grad_dense_dense (psgd.py:182-192) for Transformer-scale
 * matrices (BASELINE config 5).  Outside the reference's contract (its Kron API is pinned to
 * fp32, psgd.py:113-115): Ql, Qr are the fp32 master factors (rounded to bf16 per call), G and
 * out are bf16 [M,N]; every product runs on the bf16 matrix cores with fp32 accumulation and
 * bf16 intermediates, in the reference's association order.  M and N must be multiples of 8.
 * Upper-triangular Ql, Qr are assumed (entries below the diagonal are not read).            */
int64_t psgd_kron_dd_workspace_bytes_bf16(int M, int N);
/* Experiment knob (not stable ABI). key 0: bf16 GEMM variant: 0 auto (256^2 8-phase kernel for large dense
 * products, fused triangular pair when every 256^2 tile gets its own CU, 128^2 register-staged otherwise);
 * 1 128^2 register-staged everywhere; 2 128^2 LDS-DMA ring; 3 256^2 for every product; 4 auto without the fused pair.
 * key 1: 1 (default) two fused triangular pairs, (G Qr') Qr then Ql' (Ql .), where legal (M, N multiples of 256 and at
 *        least 16 tiles of 256^2; the Python side pads the apply to such shapes when that costs <= 20 %); 0 keep the Gram-first chain.
 * key 2: log2 of the hand-off poll bound of the fused pair (default 22 ~ 0.5 s; tests set 0 to provoke time-outs).
 * key 3: bf16-operand update: 1 (default) the trailing products of its two triangular solves keep the three leading
 *        terms of the bf16 x 3 split (h h' + h m' + m h': 2^-16 relative per product, below the bf16 rounding of the
 *        operands); 0 = all six terms.
 * key 4: bf16-operand update, the two gradient products (psgd.py:175-176): 1 (default) on the 256^2 8-phase loop as whole-tile
 *        rounds + a stream-K tail finished by a second launch (M = N multiples of 256 with at least one tile per CU: 4096^2
 *        502 -> 262 us); 0 = the 128^2 one-tile-per-workgroup kernel for every shape; 2 / 3 = the stream-K launches for every
 *        shape the kernel can take, with / without whole-tile rounds (tests).
 * key 5: bf16-operand update, the factor updates (:179): 1 (default) tiles in 4 x 4 patches per XCD, 0 = whole tile rows.
 * key 7: fused triangular pair of the apply: tile rows of the patch an XCD works on (4: 4 x 8 tiles per XCD at 4096^2, 12 operand panels per
 *        K step and L2 instead of 18); 0 = whole tile columns per XCD (rounds 1-5); -1 (default) = 8 from 32 tile rows on, 0 below (the
 *        only shapes where it was measured to gain).  Results are bitwise the same. */
int psgd_kron_bf16_set_tuning(int key, int value);
int psgd_kron_dd_apply_bf16(const float *Ql, const float *Qr, const void *G_bf16,
                            void *out_bf16, int M, int N, void *ws,
                            int64_t ws_bytes, void *stream);
/* The same call in two halves.  The bf16 copies of the factors (plain and transposed, kept in ws) change only when
 * the factors do -- after update_precond_kron -- so a caller that applies the same factors to several gradients
 * prepares once: psgd_kron_dd_apply_bf16 == psgd_kron_bf16_prepare_factors + psgd_kron_dd_apply_bf16_prepared.      */
int psgd_kron_bf16_prepare_factors(const float *Ql, const float *Qr, int M, int N, void *ws,
                                   int64_t ws_bytes, void *stream);
int psgd_kron_dd_apply_bf16_prepared(const void *G_bf16, void *out_bf16, int M, int N, void *ws,
                                     int64_t ws_bytes, void *stream);
/* bf16-operand variant of _update_precond_dense_dense (psgd.py:156-180), the update-side companion of the entry
 * point above (same contract: outside the reference's fp32-only API, M and N multiples of 8, upper-triangular fp32
 * master factors in, fp32 updated factors out; dX, dG are bf16 [M,N]).  fp32 throughout: the balance (:166-170), the
 * two triangular solves of :174, the max-norms and step sizes of :177-178 and the subtraction Q - step*grad*Q.  bf16
 * operands with fp32 accumulation: A = Ql dG Qr' (:173), the Grams of :175-176 and grad * Q (:179-180).            */
int64_t psgd_kron_dd_update_workspace_bytes_bf16(int M, int N);
int psgd_kron_dd_update_bf16(const float *Ql, const float *Qr, const void *dX_bf16, const void *dG_bf16,
                             float *QlOut, float *QrOut, int M, int N, float step, float tiny,
                             void *ws, int64_t ws_bytes, void *stream);
/* The fused triangular pairs of the bf16 apply hand tiles between workgroups inside one launch.  Their schedule
 * assumes every workgroup of the launch resident (checked against the CU count -- which cannot see other streams or
 * processes on the GPU); their RESULT does not: a consumer that has waited for a tile for its whole bound (~0.5 s)
 * produces that tile itself (same instructions, same inputs: the same bytes its owner would write), publishes it and
 * redoes its own accumulation from the start, so every call returns the undisturbed bits whatever the residency.  The
 * workspace counts such recoveries: psgd_kron_bf16_handoff_timeouts (synchronises: call it at a point where the host
 * waits anyway) returns how many happened on this workspace since it was created or reset -- a diagnostic (a device
 * that is persistently shared wastes up to the bound per recovery; psgd_kron_bf16_set_tuning(0, 4) selects the kernels
 * without in-launch hand-offs).  A fresh workspace must be reset once before its first use (the word lives in
 * caller-owned memory).                                                                                              */
int psgd_kron_bf16_handoff_timeouts(const void *ws, int M, int N);
int psgd_kron_bf16_handoff_reset(void *ws, int M, int N, void *stream);
/* Byte offset of that 32-bit recovery counter inside a workspace of shape (M, N) (round 6): a caller that wants to WATCH it without
 * synchronising copies the word to pinned host memory asynchronously now and then (psgd_tf_amd/kron.py does, and switches to the
 * hand-off-free kernels by itself after three recoveries).  < 0 on a bad shape.                                                     */
int64_t psgd_kron_bf16_handoff_counter_offset(int M, int N);

/* ---------------------------------------------------------------- dense ---
 * One dense N x N preconditioner factor Q, P = Q'Q (psgd.py:26-63).  Q is row-major [N, N]; dx, dg, g are the
 * concatenated columns [N].  Q is used as a full matrix in the products; the triangular solve of :39 reads its upper
 * triangle only.  The update never forms G = triu(a a' - b b') nor an N^3 product: (G Q)[i,j] = a_i A[i,j] - b_i B[i,j]
 * with A, B the suffix sums sum_{k>=i} a_k Q[k,j], sum_{k>=i} b_k Q[k,j] down each column.  Results are bit-identical
 * from call to call.  The workspace (>= psgd_dense_workspace_bytes(N), 256-byte aligned) serves both calls.         */
int64_t psgd_dense_workspace_bytes(int64_t N);   /* PSGD_ERR_BAD_ARG for N <= 0 */
/* update_precond_dense (psgd.py:26-42): a = Q dg, Q' b = dx, mu = step / (max_{i<=j} |a_i a_j - b_i b_j| + tiny),
 * Qout = Q - mu G Q.  Pure: Qout == Q is PSGD_ERR_BAD_ARG.                                                   */
int psgd_dense_update_f32(const float *Q, const float *dx, const float *dg, float *Qout, int64_t N,
                          float step, float tiny, void *ws, int64_t ws_bytes, void *stream);
/* precond_grad_dense (psgd.py:55): out = Q' (Q g) */
int psgd_dense_apply_f32(const float *Q, const float *g, float *out, int64_t N, void *ws, int64_t ws_bytes,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PSGD_HIP_H */
