/* psgd_kron_quad_nd_list_hip.h -- C ABI of the GROUPED QUAD Kronecker update and apply on ORDER-3 tensors,
 * psgd_kron_qtlist.hip, in libpsgd_hip.so.
 *
 * include/psgd_kron_quad_nd_hip.h is the update on one tensor layer [A, B, C] with three symmetric factors: seven launches, six
 * for the apply, each grid one layer's tiles.  Here a LIST of k such layers goes through the same stages in at most eight launches
 * per GROUP of layers (six for the apply), every launch a grid over the work of all the layers of the group -- what
 * psgd_kron_quad_list_hip.h does for matrix layers -- and the Gram of a SHORT side (few output tiles, a long sum) is split along K
 * into S slices whose raw accumulators are folded in fp64 in slice order.  The math is that of psgd_kron_quad_nd_hip.h; the tile
 * code, the K-step order inside a slice, the fp64 fold orders and the load routes are the per-layer ones.  A layer all of whose
 * sides have S = 1 gets, bit for bit, what psgd_kron_qnd_update_f32 gives on that layer alone; the apply always has the bits of
 * psgd_kron_qnd_apply_f32; a split side differs from the per-layer T by the rounding of its sum alone (S fp32 partial sums added
 * in fp64 and rounded once, instead of one fp32 chain).  Results never depend on the list, its order or the cap.
 *
 * Slice rule: a function of the side's shape and of gram_slice_k alone.  For a side of extent n with b(n) = ceil(n /
 * PSGD_KRON_QUAD_TILE) tile rows, u = b(n) (b(n) + 1) / 2 upper tiles and Gram length K (the product of the other two extents):
 *   steps_total = ceil(K / 16)                                   (16: the K step of the product core)
 *   S    = min(ceil(steps_total 16 / gram_slice_k), max(1, PSGD_KRON_QTL_CUS / u))
 *   per  = ceil(steps_total / S)                                 K steps per slice; the last slice has the rest
 *   S    = ceil(steps_total / per)                               so that no slice is empty
 * Slice i sums k in [16 i per, min(K, 16 (i + 1) per)).  For the middle mode (K = A C, a outer and c inner) a slice bound may
 * fall anywhere, also inside a slab.  gram_slice_k must be a positive multiple of 16.
 *
 * Descriptor table (device memory, k records of psgd_kron_qtl_layer, list order).  A record holds the layer's operands, its shape
 * and ws_off[]: the byte offsets, from the base of the workspace block, of the layer's carve (PSGD_KRON_QTL_WS_* below, each a
 * multiple of 256): the regions of the per-layer workspace in the per-layer order, then one partial buffer per side, of
 * S u 16 KiB when the side is split and empty otherwise.  A partial is the accumulator fragment of one (tile, slice) as the
 * product core leaves it: for q = 0 .. 3 (acc[q >> 1][q & 1]) thread t's four floats at byte (q 256 + t) 16, so that every one of
 * a wave's four 16-byte stores covers one contiguous KiB; partial (tile u, slice i) is number u S + i of its side.  The kernels
 * derive every operand view from the record; a workgroup reads no record but its own layer's.  update reads Qa, Qb, Qc, L, G (out
 * is ignored) and rewrites Qa, Qb, Qc, L in place; apply reads Qa, Qb, Qc, G and writes out (L is ignored).  The table is the
 * caller's: a null or aliased operand INSIDE a record is the caller's to refuse (psgd_tf_amd/kron_quad_nd_list.py does).  Within a
 * list no written operand may overlap any other operand of any layer.
 *
 * Groups: as in psgd_kron_quad_list_hip.h.  The list is cut, in list order, into consecutive groups whose summed carves stay at or
 * under max_group_bytes; a layer over the cap alone is a group of one; the groups run one after another on the same block, whose
 * size psgd_kron_qtl_workspace_bytes gives (the largest group's sum).
 *
 * Plan (psgd_kron_qtl_plan, host only, no HIP call; a function of the shapes, the cap and gram_slice_k alone).  It writes
 *   group_start[0 .. groups]                 layer index at which each group begins, group_start[groups] = k; returns `groups`
 *   plan[PSGD_KRON_QTL_PLAN_INTS(k)]         per stage class s: order[s][k], then prefix[s][k + 1]
 *   ws_off[k][PSGD_KRON_QTL_WS_REGIONS]      the carve of every layer, to be copied into the records
 *   slices[k][3]                             S of the three sides of every layer
 * order[s] holds, group by group, the layers sorted by the K of the stage, longest first, ties in list order; prefix[s][i] is the
 * number of workgroups of the positions before i.  Workgroup b of the launch of group g serves the position i with
 * prefix[s][i] <= b + prefix[s][group_start[g]] < prefix[s][i + 1], found by a bisection that is uniform over the workgroup (a
 * position without workgroups -- FOLD only -- is never found).  With n = (A, B, C), K_s = A B C / n_s, b_s = b(n_s),
 * u_s = u(n_s), S_s the slice count, and m(i) the mode at place i of the apply's order (ascending extent, the lower mode first):
 *
 *   stage class     serves                               K of the sort             workgroups of a layer
 *   MODE_A          update launch 1 (x1 Qa)              A                         b(A) b(B C)
 *   MODE_B          update launch 2 (x2 Qb, all slabs)   B                         A b(B) b(C)
 *   MODE_C          update launch 3 (x3 Qc)              C                         b(A B) b(C)
 *   APPLY_0 .. _2   apply launches 2i + 1, 2i + 2        n_m(i)                    those of MODE_m(i)
 *   GRAM            update launch 4                      max_s 16 per_s (<= K_s)   sum_s u_s S_s
 *   FOLD            update launch 5                      max_s S_s                 sum over the sides with S_s > 1 of u_s
 *   UPPER           update launch 8 (symmetrised P2)     max(A, B, C)              u_a + u_b + u_c
 *   FULL            update launch 7 (P1)                 max(A, B, C)              b_a^2 + b_b^2 + b_c^2
 *   (Lipschitz)     update launch 6, the order of UPPER  -                         3 (of 1024 threads; workgroup b: position b / 3)
 *
 * Inside a layer the workgroups of GRAM, FOLD, UPPER and FULL run side a, then b, then c; a GRAM workgroup of a side is
 * (tile, slice) number tile S + slice.  A side with S = 1 is finished in launch 4 (product over its whole K and the Gram
 * epilogue, as the per-layer kernel); a split side stores partials there and is finished by launch 5, one workgroup per upper
 * tile: every thread adds its fragment over the S partials in slice order in fp64, rounds once to fp32 and runs the same epilogue
 * (T stored and mirrored, the per-tile max|T|, the column sum-of-squares partials).  Launch 5 is not issued for a group without a
 * split side.  Launch i of a layer's apply runs that layer's own mode m(i / 2), so one launch mixes modes across layers; reads and
 * writes follow the per-layer ping-pong G -> X[0] -> X[1] -> ... -> out.
 *
 * The entry points take the plan twice: plan_dev, the device copy the kernels read, and plan_host / group_start, what the planner
 * wrote.  Checks before any HIP call: PSGD_ERR_BAD_ARG for a null table, plan or shape array, k < 1, an extent < 1 or
 * A B C >= 2^31, gram_slice_k that is not a positive multiple of 16, group_start that is not 0 < ... < k, or a plan whose order or
 * prefix cannot belong to these shapes; PSGD_ERR_WORKSPACE for a workspace that is null, not 256-byte aligned or shorter than the
 * largest group.  Nothing allocates or synchronises, the host reads nothing back, no atomics: every output element and every
 * partial has one writer and every fold a fixed order, so repeated calls are bit-identical. */
#ifndef PSGD_KRON_QUAD_ND_LIST_HIP_H
#define PSGD_KRON_QUAD_ND_LIST_HIP_H

#include <stdint.h>
#include "psgd_kron_quad_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* regions of a layer's carve; side s in 0 .. 2 (a, b, c) */
#define PSGD_KRON_QTL_WS_X         0   /* + i, i in 0 .. 1: A B C fp32 */
#define PSGD_KRON_QTL_WS_T         2   /* + 5 s: n x n fp32 */
#define PSGD_KRON_QTL_WS_P1        3   /* + 5 s: n x n fp32 */
#define PSGD_KRON_QTL_WS_TMAX      4   /* + 5 s: b(n) b(n) fp32 */
#define PSGD_KRON_QTL_WS_PART      5   /* + 5 s: b(n) n fp64 */
#define PSGD_KRON_QTL_WS_VEC       6   /* + 5 s: 2 n fp64 */
#define PSGD_KRON_QTL_WS_COEF      17  /* 3 fp32 */
#define PSGD_KRON_QTL_WS_SLICES    18  /* + s: S u partials of 16 KiB when S > 1, else empty */
#define PSGD_KRON_QTL_WS_REGIONS   21

#define PSGD_KRON_QTL_STAGE_MODE_A   0
#define PSGD_KRON_QTL_STAGE_MODE_B   1
#define PSGD_KRON_QTL_STAGE_MODE_C   2
#define PSGD_KRON_QTL_STAGE_APPLY_0  3
#define PSGD_KRON_QTL_STAGE_APPLY_1  4
#define PSGD_KRON_QTL_STAGE_APPLY_2  5
#define PSGD_KRON_QTL_STAGE_GRAM     6
#define PSGD_KRON_QTL_STAGE_FOLD     7
#define PSGD_KRON_QTL_STAGE_UPPER    8
#define PSGD_KRON_QTL_STAGE_FULL     9
#define PSGD_KRON_QTL_STAGES         10
#define PSGD_KRON_QTL_PLAN_INTS(k)   (PSGD_KRON_QTL_STAGES * (2 * (k) + 1))

#define PSGD_KRON_QTL_CUS                  256              /* compute units the slice rule fills */
#define PSGD_KRON_QTL_DEFAULT_GROUP_BYTES  (1024ll << 20)
#define PSGD_KRON_QTL_DEFAULT_SLICE_K      2048

typedef struct psgd_kron_qtl_layer {        /* 232 bytes, no padding */
  float *Qa, *Qb, *Qc, *L;
  const float *G;
  float *out;
  int32_t A, B, C, reserved;                /* reserved = 0 */
  int64_t ws_off[PSGD_KRON_QTL_WS_REGIONS];
} psgd_kron_qtl_layer;

/* bytes of the workspace block: the largest group's sum; PSGD_ERR_BAD_ARG for null arrays, k < 1, a bad shape or gram_slice_k */
int64_t psgd_kron_qtl_workspace_bytes(const int *A, const int *B, const int *C, int k, int64_t max_group_bytes, int gram_slice_k);
/* the number of groups (>= 1), or PSGD_ERR_BAD_ARG (as above; also when a launch would pass 2^31 - 1 workgroups) */
int psgd_kron_qtl_plan(const int *A, const int *B, const int *C, int k, int64_t max_group_bytes, int gram_slice_k,
                       int32_t *group_start, int32_t *plan, int64_t *ws_off, int32_t *slices);
int psgd_kron_qtl_update_f32(const psgd_kron_qtl_layer *table, const int32_t *plan_dev, const int32_t *plan_host,
                             const int32_t *group_start, int groups, const int *A, const int *B, const int *C, int k,
                             int gram_slice_k, float step, float decay, void *ws, int64_t ws_bytes, void *stream);
int psgd_kron_qtl_apply_f32(const psgd_kron_qtl_layer *table, const int32_t *plan_dev, const int32_t *plan_host,
                            const int32_t *group_start, int groups, const int *A, const int *B, const int *C, int k,
                            int gram_slice_k, void *ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PSGD_KRON_QUAD_ND_LIST_HIP_H */
