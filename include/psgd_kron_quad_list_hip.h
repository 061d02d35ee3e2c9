/* psgd_kron_quad_list_hip.h -- C ABI of the GROUPED QUAD Kronecker update and apply, psgd_kron_qlist.hip, in libpsgd_hip.so.
 *
 * include/psgd_kron_quad_hip.h is the update on one layer: six launches, four for the apply, each grid one layer's tiles.  Here a
 * LIST of k layers (both factors dense and symmetric) goes through the same stages in six launches per GROUP of layers (four for
 * the apply), every launch a grid over the tiles of all the layers of the group.  The math, the tile code, the K-step order, the
 * fp64 fold orders and the load routes are the per-layer ones: for every layer the result is, bit for bit, what
 * psgd_kron_quad_update_f32 / psgd_kron_quad_apply_f32 give on that layer alone, whatever the list, its order and the cap.
 *
 * Descriptor table (device memory, k records of psgd_kron_qlist_layer, list order).  A record holds the layer's operands, its
 * shape and ws_off[]: the byte offsets, from the base of the workspace block, of the layer's carve -- the regions of the per-layer
 * workspace in the per-layer order (PSGD_KRON_QLIST_WS_* below), each a multiple of 256.  The kernels derive every operand view of
 * every stage from the record; a workgroup reads no record but its own layer's.  update reads Ql, Qr, L, G (out is ignored) and
 * rewrites Ql, Qr, L in place; apply reads Ql, Qr, G and writes out (L is ignored).  The table is the caller's: the entry points
 * cannot look into it, so a null or aliased operand INSIDE a record is the caller's to refuse (psgd_tf_amd/kron_quad_list.py
 * does).  Within a list no written operand may overlap any other operand of any layer.
 *
 * Groups.  A grouped launch needs the workspace of every layer of the group alive at once, so the list is cut, in list order, into
 * consecutive groups whose summed per-layer workspace stays at or under max_group_bytes; a layer that exceeds the cap alone is a
 * group of one.  The groups run one after another on the SAME workspace block: psgd_kron_qlist_workspace_bytes is the largest
 * group's sum, and ws_off[] counts from the block's base, the first layer of every group at 0.
 *
 * Plan (psgd_kron_qlist_plan, host only, no HIP call; a function of the shapes and the cap alone).  It writes
 *   group_start[0 .. groups]   layer index at which each group begins, group_start[groups] = k; returns `groups`
 *   plan[PSGD_KRON_QLIST_PLAN_INTS(k)]   per stage class s (PSGD_KRON_QLIST_STAGE_*): order[s][k], then prefix[s][k + 1]
 *   ws_off[k][PSGD_KRON_QLIST_WS_REGIONS]   the carve of every layer, to be copied into the records
 * order[s] holds, group by group (positions group_start[g] .. group_start[g + 1] - 1), the layers of the group sorted by the K
 * of the stage, longest first, ties in list order: the tail of a grid is made of short tiles.  prefix[s][i] is the number of
 * workgroups of the positions before i (cumulative over the whole list): the launch of group g has
 * prefix[s][group_start[g + 1]] - prefix[s][group_start[g]] workgroups, and workgroup b serves the position i of the group with
 * prefix[s][i] <= b + prefix[s][group_start[g]] < prefix[s][i + 1], found by a binary search that is uniform over the workgroup.
 * With b(n) = ceil(n / PSGD_KRON_QUAD_TILE) and u(n) = b(n) (b(n) + 1) / 2:
 *
 *   stage class   serves                          K of the sort    workgroups of a layer
 *   PROD_M        update launch 1 (W = Ql G)      M                b(M) b(N)
 *   PROD_N        update launch 2 (A = W Qr)      N                b(M) b(N)
 *   PROD_MIN      apply launches 1, 2             min(M, N)        b(M) b(N)
 *   PROD_MAX      apply launches 3, 4             max(M, N)        b(M) b(N)
 *   UPPER         Gram and symmetrised P2         max(M, N)        u(M) + u(N)
 *   FULL          P1                              max(M, N)        b(M)^2 + b(N)^2
 *   (Lipschitz)   the order of UPPER              -                2 (of 1024 threads; no prefix: workgroup b is position b / 2)
 *
 * Launch s of a layer's apply is a left product (Ql .) or a right one (. Qr) by the layer's own M <= N rule -- the shorter side's
 * two products first, as psgd_kron_quad_apply_f32 does -- so one launch holds left products of some layers and right products of
 * others.  The load route (16-byte, or dword with bounds) is chosen per layer and per step from the layer's own base, stride and
 * extents, as in the per-layer kernels.
 *
 * The entry points take the plan twice: plan_dev, the device copy the kernels read, and plan_host / group_start, what the planner
 * wrote, from which the host takes the grids.  They must be the same plan for the same M[], N[].  Checks before any HIP call:
 * PSGD_ERR_BAD_ARG for a null table, plan or shape array, k < 1, M or N < 1, group_start that is not 0 < ... < k, or a plan whose
 * order or prefix cannot belong to these shapes; PSGD_ERR_WORKSPACE for a workspace that is null, not 256-byte aligned or shorter
 * than the largest group.  Nothing allocates or synchronises, the host reads nothing back, no atomics: every output tile has one
 * writer and every fold a fixed order, so repeated calls are bit-identical.  An update is 6 launches per group, an apply 4. */
#ifndef PSGD_KRON_QUAD_LIST_HIP_H
#define PSGD_KRON_QUAD_LIST_HIP_H

#include <stdint.h>
#include "psgd_kron_quad_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* regions of a layer's carve, in the order of the per-layer workspace; side 1 (right) follows side 0 (left) */
#define PSGD_KRON_QLIST_WS_W        0   /* M x N fp32 */
#define PSGD_KRON_QLIST_WS_A        1   /* M x N fp32 */
#define PSGD_KRON_QLIST_WS_T        2   /* + 5 side: n x n fp32 */
#define PSGD_KRON_QLIST_WS_P1       3   /* + 5 side: n x n fp32 */
#define PSGD_KRON_QLIST_WS_TMAX     4   /* + 5 side: b(n) b(n) fp32 */
#define PSGD_KRON_QLIST_WS_PART     5   /* + 5 side: b(n) n fp64 */
#define PSGD_KRON_QLIST_WS_VEC      6   /* + 5 side: 2 n fp64 */
#define PSGD_KRON_QLIST_WS_COEF     12  /* 2 fp32 */
#define PSGD_KRON_QLIST_WS_REGIONS  13

#define PSGD_KRON_QLIST_STAGE_PROD_M    0
#define PSGD_KRON_QLIST_STAGE_PROD_N    1
#define PSGD_KRON_QLIST_STAGE_PROD_MIN  2
#define PSGD_KRON_QLIST_STAGE_PROD_MAX  3
#define PSGD_KRON_QLIST_STAGE_UPPER     4
#define PSGD_KRON_QLIST_STAGE_FULL      5
#define PSGD_KRON_QLIST_STAGES          6
#define PSGD_KRON_QLIST_PLAN_INTS(k)    (PSGD_KRON_QLIST_STAGES * (2 * (k) + 1))

#define PSGD_KRON_QLIST_DEFAULT_GROUP_BYTES  (1024ll << 20)

typedef struct psgd_kron_qlist_layer {      /* 152 bytes, no padding */
  float *Ql, *Qr, *L;
  const float *G;
  float *out;
  int32_t M, N;
  int64_t ws_off[PSGD_KRON_QLIST_WS_REGIONS];
} psgd_kron_qlist_layer;

/* bytes of the workspace block: the largest group's sum; PSGD_ERR_BAD_ARG for null arrays, k < 1, M or N < 1 */
int64_t psgd_kron_qlist_workspace_bytes(const int *M, const int *N, int k, int64_t max_group_bytes);
/* the number of groups (>= 1), or PSGD_ERR_BAD_ARG (as above; also when a launch would pass 2^31 - 1 workgroups) */
int psgd_kron_qlist_plan(const int *M, const int *N, int k, int64_t max_group_bytes, int32_t *group_start, int32_t *plan,
                         int64_t *ws_off);
int psgd_kron_qlist_update_f32(const psgd_kron_qlist_layer *table, const int32_t *plan_dev, const int32_t *plan_host,
                               const int32_t *group_start, int groups, const int *M, const int *N, int k, float step, float decay,
                               void *ws, int64_t ws_bytes, void *stream);
int psgd_kron_qlist_apply_f32(const psgd_kron_qlist_layer *table, const int32_t *plan_dev, const int32_t *plan_host,
                              const int32_t *group_start, int groups, const int *M, const int *N, int k, void *ws, int64_t ws_bytes,
                              void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PSGD_KRON_QUAD_LIST_HIP_H */
