// psgd_kron_qlist.hip -- the QUAD Kronecker update and apply on a LIST of (dense, dense) layers, gfx950: the stages of
// psgd_kron_quad.hip with one launch per stage for a whole GROUP of layers.  include/psgd_kron_quad_list_hip.h has the contract.
//
// Why.  A 256 x 256 layer is 16 product workgroups on a 256-CU device and its Lipschitz launch is two: the per-layer route is
// bound by launches and empty CUs, not by arithmetic.  Here the grid of a stage is the concatenation of the layers' tile grids.
//
// How a workgroup finds its work.  The kernels take no per-layer argument.  A launch gets the device plan (per stage class an
// order[] of layers and a prefix[] of workgroup counts over that order) and the range of positions [lo, hi) of its group.
// Workgroup b looks for the position i with prefix[i] <= b + prefix[lo] < prefix[i + 1] by bisection -- blockIdx and kernel
// arguments only, so the search, the layer and the tile number are uniform and are pinned to scalar registers -- and then
// reads ONE record of the descriptor table, its layer's: pointers, M, N and the byte offsets of the layer's workspace carve.
// From these it builds the Opnd / GramSide / LipSide / StepSide views the per-layer host code builds, and runs the per-layer tile
// body of kron_quad_core.h: same tile code, same K steps, same fp64 folds, same choice between 16-byte and dword loads (made
// per step from the layer's own base, stride and extents), hence the same bits.
//
// Order.  Within a group the layers of a stage are laid out longest K first (the planner below), so the last workgroups the
// dispatcher hands out are the short ones.  Every output tile has one writer and every fold its fixed order: nothing depends on it.
//
// Update = 6 launches per group (W = Ql G | A = W Qr | Gram of both sides | Lipschitz, two workgroups per layer | P1 | P2
// symmetrised), apply = 4 (launch s of a layer is a left or a right product by its own M <= N rule).  No atomics.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "kron_quad_core.h"
#include "psgd_kron_quad_list_hip.h"

namespace psgdq {

typedef psgd_kron_qlist_layer Layer;
static_assert(sizeof(Layer) == 152, "the host layer writes the table as rows of 19 int64");

// --------------------------------------------------------------------------------------------------------------- the map
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// where workgroup blockIdx.x of a launch over the positions [lo, hi) works: the layer and the workgroup's number inside it
struct Where {
  int layer, local;
};
__device__ __forceinline__ Where locate(const int32_t* __restrict__ order, const int32_t* __restrict__ prefix, int lo, int hi) {
  const int b = (int)blockIdx.x + prefix[lo];
  while (hi - lo > 1) {                                 // prefix[lo] <= b < prefix[hi]; every layer has >= 1 workgroup
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= b) lo = mid; else hi = mid;
  }
  return Where{uni(order[lo]), uni(b - prefix[lo])};
}

// a region of the layer's carve
template <class T>
__device__ __forceinline__ T* region(char* ws, const Layer& d, int r) {
  return reinterpret_cast<T*>(ws + d.ws_off[r]);
}
__device__ __forceinline__ GramSide gram_side(char* ws, const Layer& d, int side) {
  const int M = d.M, N = d.N, n = side ? N : M, r = 5 * side;
  const float* A = region<float>(ws, d, PSGD_KRON_QLIST_WS_A);
  return GramSide{side ? Opnd{A, 1, N, N} : Opnd{A, N, 1, M}, n, side ? M : N, (n + kTile - 1) / kTile,
                  region<float>(ws, d, PSGD_KRON_QLIST_WS_T + r), region<float>(ws, d, PSGD_KRON_QLIST_WS_TMAX + r),
                  region<double>(ws, d, PSGD_KRON_QLIST_WS_PART + r)};
}
__device__ __forceinline__ StepSide step_side(char* ws, const Layer& d, int side) {
  const int n = side ? d.N : d.M, r = 5 * side;
  return StepSide{n, (n + kTile - 1) / kTile, region<float>(ws, d, PSGD_KRON_QLIST_WS_T + r), side ? d.Qr : d.Ql,
                  region<float>(ws, d, PSGD_KRON_QLIST_WS_P1 + r), (float)(side ? d.M : d.N)};
}
__device__ __forceinline__ int upper_of(int n) {
  const int nb = (n + kTile - 1) / kTile;
  return nb * (nb + 1) / 2;
}

// --------------------------------------------------------------------------------------------------------------- kernels
// what a product launch computes for every layer: source -> destination, and which factor multiplies
enum ProductMode { kApply0 = 0, kApply1, kApply2, kApply3, kUpdateW, kUpdateA };

// one tile of C = Ql X (left) or C = X Qr (right) of the workgroup's layer
__global__ __launch_bounds__(kT) void k_list_product(const Layer* __restrict__ table, char* __restrict__ ws,
                                                     const int32_t* __restrict__ order, const int32_t* __restrict__ prefix, int lo,
                                                     int hi, int mode) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const Where w = locate(order, prefix, lo, hi);
  const Layer& d = table[w.layer];
  const int M = d.M, N = d.N;
  float* W = region<float>(ws, d, PSGD_KRON_QLIST_WS_W);
  float* A = region<float>(ws, d, PSGD_KRON_QLIST_WS_A);
  // G -> W -> A -> W -> out; the shorter side's factor multiplies in the first two launches of the apply
  const float* X = (mode == kApply0 || mode == kUpdateW) ? d.G : (mode == kApply2) ? A : W;
  float* C = (mode == kApply0 || mode == kApply2 || mode == kUpdateW) ? W : (mode == kApply3) ? d.out : A;
  const bool left = mode == kUpdateW || (mode <= kApply3 && ((mode < kApply2) == (M <= N)));
  const Opnd a = left ? Opnd{d.Ql, M, 1, M} : Opnd{X, N, 1, M};
  const Opnd b = left ? Opnd{X, 1, N, N} : Opnd{d.Qr, 1, N, N};
  const int tiles_n = (N + kTile - 1) / kTile;
  const int m0 = (w.local / tiles_n) * kTile, n0 = (w.local % tiles_n) * kTile;
  f32x4 acc[2][2];
  product(a, b, left ? M : N, m0, n0, lds, acc);
  each_elem([&](int i, int j, int e, int r, int c) {
    if (m0 + r < M && n0 + c < N) C[(long)(m0 + r) * N + (n0 + c)] = acc[i][j][e];
  });
}

// Tl and Tr of the workgroup's layer: its upper tiles of the left side, then those of the right
__global__ __launch_bounds__(kT) void k_list_gram(const Layer* __restrict__ table, char* __restrict__ ws,
                                                  const int32_t* __restrict__ order, const int32_t* __restrict__ prefix, int lo, int hi) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  __shared__ float red[kT / 64];
  const Where w = locate(order, prefix, lo, hi);
  const Layer& d = table[w.layer];
  const int upper_l = upper_of(d.M);
  const bool right = w.local >= upper_l;
  const GramSide s = gram_side(ws, d, right);
  int ti, tj;
  upper_tile(right ? w.local - upper_l : w.local, s.nb, ti, tj);
  f32x4 acc[2][2];
  product(s.o, s.o, s.K, ti * kTile, tj * kTile, lds, acc);
  gram_epilogue(s, ti, tj, acc, lds, red);
}

// two workgroups per layer, position blockIdx.x / 2 of the group: L (in place) and c of the left side, of the right side
__global__ __launch_bounds__(kLipT) void k_list_lipschitz(const Layer* __restrict__ table, char* __restrict__ ws,
                                                          const int32_t* __restrict__ order, int lo, float step, float decay) {
  __shared__ double red[kLipT];
  __shared__ int redi[kLipT];
  __shared__ float redf[kLipT / 64];
  const Layer& d = table[uni(order[lo + (int)(blockIdx.x >> 1)])];
  const int side = blockIdx.x & 1, n = side ? d.N : d.M, r = 5 * side;
  const LipSide s{n, (n + kTile - 1) / kTile, region<float>(ws, d, PSGD_KRON_QLIST_WS_T + r),
                  region<float>(ws, d, PSGD_KRON_QLIST_WS_TMAX + r), region<double>(ws, d, PSGD_KRON_QLIST_WS_PART + r),
                  region<double>(ws, d, PSGD_KRON_QLIST_WS_VEC + r), (double)(side ? d.M : d.N)};
  lipschitz_dense(s, d.L + side, region<float>(ws, d, PSGD_KRON_QLIST_WS_COEF) + side, step, decay, red, redi, redf);
}

// P1 = Q - c (T Q - t2 Q): every tile of the left side of the workgroup's layer, then every tile of the right
__global__ __launch_bounds__(kT) void k_list_p1(const Layer* __restrict__ table, char* __restrict__ ws,
                                                const int32_t* __restrict__ order, const int32_t* __restrict__ prefix, int lo, int hi) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const Where w = locate(order, prefix, lo, hi);
  const Layer& d = table[w.layer];
  const int nbl = (d.M + kTile - 1) / kTile, tiles_l = nbl * nbl;
  const bool right = w.local >= tiles_l;
  p1_tile(step_side(ws, d, right), right ? w.local - tiles_l : w.local, region<float>(ws, d, PSGD_KRON_QLIST_WS_COEF)[right ? 1 : 0],
          lds);
}

// Q <- (P2 + P2') / 2 over the upper tiles of the left side of the workgroup's layer, then of the right
__global__ __launch_bounds__(kT) void k_list_p2_sym(const Layer* __restrict__ table, char* __restrict__ ws,
                                                    const int32_t* __restrict__ order, const int32_t* __restrict__ prefix, int lo,
                                                    int hi) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const Where w = locate(order, prefix, lo, hi);
  const Layer& d = table[w.layer];
  const int upper_l = upper_of(d.M);
  const bool right = w.local >= upper_l;
  p2_sym_tiles(step_side(ws, d, right), right ? w.local - upper_l : w.local,
               region<float>(ws, d, PSGD_KRON_QLIST_WS_COEF)[right ? 1 : 0], lds);
}

// --------------------------------------------------------------------------------------------------------------- the host
// the carve of one layer from byte `base` on: the regions of the per-layer workspace, in its order.  Returns the bytes taken.
static int64_t carve_layer(int M, int N, int64_t base, int64_t* off) {
  int64_t at = base, scratch[PSGD_KRON_QLIST_WS_REGIONS];
  if (!off) off = scratch;
  auto take = [&](int r, int64_t bytes) {
    off[r] = at;
    at += up256(bytes);
  };
  const int64_t mn = (int64_t)M * N, dim[2] = {M, N};
  take(PSGD_KRON_QLIST_WS_W, mn * 4);
  take(PSGD_KRON_QLIST_WS_A, mn * 4);
  for (int s = 0; s < 2; ++s) {
    const int64_t n = dim[s], nb = tiles_of((int)n);
    take(PSGD_KRON_QLIST_WS_T + 5 * s, n * n * 4);
    take(PSGD_KRON_QLIST_WS_P1 + 5 * s, n * n * 4);
    take(PSGD_KRON_QLIST_WS_TMAX + 5 * s, nb * nb * 4);
    take(PSGD_KRON_QLIST_WS_PART + 5 * s, nb * n * 8);
    take(PSGD_KRON_QLIST_WS_VEC + 5 * s, 2 * n * 8);
  }
  take(PSGD_KRON_QLIST_WS_COEF, 2 * 4);
  return at - base;
}

static bool shapes_ok(const int* M, const int* N, int k) {
  if (!M || !N || k < 1) return false;
  for (int i = 0; i < k; ++i)
    if (M[i] < 1 || N[i] < 1) return false;
  return true;
}

// the end (exclusive) of the group that begins at layer g0, and its bytes
static int group_end(const int* M, const int* N, int k, int64_t cap, int g0, int64_t* bytes) {
  int64_t sum = carve_layer(M[g0], N[g0], 0, nullptr);
  int g1 = g0 + 1;
  for (; g1 < k; ++g1) {
    const int64_t b = carve_layer(M[g1], N[g1], 0, nullptr);
    if (sum + b > cap) break;
    sum += b;
  }
  *bytes = sum;
  return g1;
}

static int sort_key(int stage, int M, int N) {
  switch (stage) {
    case PSGD_KRON_QLIST_STAGE_PROD_M: return M;
    case PSGD_KRON_QLIST_STAGE_PROD_N: return N;
    case PSGD_KRON_QLIST_STAGE_PROD_MIN: return std::min(M, N);
    default: return std::max(M, N);
  }
}
static int64_t stage_count(int stage, int M, int N) {
  const int64_t bm = tiles_of(M), bn = tiles_of(N);
  if (stage == PSGD_KRON_QLIST_STAGE_UPPER) return bm * (bm + 1) / 2 + bn * (bn + 1) / 2;
  if (stage == PSGD_KRON_QLIST_STAGE_FULL) return bm * bm + bn * bn;
  return bm * bn;
}
static const int32_t* plan_order(const int32_t* plan, int k, int stage) { return plan + (int64_t)stage * (2 * k + 1); }
static const int32_t* plan_prefix(const int32_t* plan, int k, int stage) { return plan_order(plan, k, stage) + k; }

// what the entry points check before any HIP call
static int check_call(const void* table, const int32_t* plan_dev, const int32_t* plan, const int32_t* gs, int groups, const int* M,
                      const int* N, int k, const void* ws, int64_t ws_bytes) {
  if (!table || !plan_dev || !plan || !gs || !shapes_ok(M, N, k) || groups < 1 || groups > k || gs[0] != 0 || gs[groups] != k)
    return PSGD_ERR_BAD_ARG;
  int64_t need = 0;
  for (int g = 0; g < groups; ++g) {
    if (gs[g + 1] <= gs[g] || gs[g + 1] > k) return PSGD_ERR_BAD_ARG;
    int64_t sum = 0;
    for (int i = gs[g]; i < gs[g + 1]; ++i) sum += carve_layer(M[i], N[i], 0, nullptr);
    need = std::max(need, sum);
    for (int s = 0; s < PSGD_KRON_QLIST_STAGES; ++s) {   // every position a layer of this group, with that layer's workgroups
      const int32_t *order = plan_order(plan, k, s), *prefix = plan_prefix(plan, k, s);
      for (int i = gs[g]; i < gs[g + 1]; ++i) {
        const int l = order[i];
        if (l < gs[g] || l >= gs[g + 1] || (int64_t)prefix[i + 1] - prefix[i] != stage_count(s, M[l], N[l])) return PSGD_ERR_BAD_ARG;
      }
    }
  }
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) || ws_bytes < need) return PSGD_ERR_WORKSPACE;
  return PSGD_OK;
}

struct Launch {
  const Layer* table;
  char* ws;
  const int32_t *plan_dev, *plan;
  int k, lo, hi;
  hipStream_t st;
  unsigned grid(int stage) const { return (unsigned)(plan_prefix(plan, k, stage)[hi] - plan_prefix(plan, k, stage)[lo]); }
  void product(int stage, int mode) const {
    hipLaunchKernelGGL(k_list_product, dim3(grid(stage)), dim3(kT), 0, st, table, ws, plan_order(plan_dev, k, stage),
                       plan_prefix(plan_dev, k, stage), lo, hi, mode);
  }
};

}  // namespace psgdq

using namespace psgdq;

extern "C" {

int64_t psgd_kron_qlist_workspace_bytes(const int* M, const int* N, int k, int64_t max_group_bytes) {
  if (!shapes_ok(M, N, k)) return PSGD_ERR_BAD_ARG;
  int64_t need = 0, bytes;
  for (int g0 = 0; g0 < k;) {
    g0 = group_end(M, N, k, max_group_bytes, g0, &bytes);
    need = std::max(need, bytes);
  }
  return need;
}

int psgd_kron_qlist_plan(const int* M, const int* N, int k, int64_t max_group_bytes, int32_t* group_start, int32_t* plan,
                         int64_t* ws_off) {
  if (!shapes_ok(M, N, k) || !group_start || !plan || !ws_off) return PSGD_ERR_BAD_ARG;
  int groups = 0;
  for (int g0 = 0; g0 < k;) {
    int64_t bytes;
    const int g1 = group_end(M, N, k, max_group_bytes, g0, &bytes);
    group_start[groups++] = g0;
    int64_t base = 0;
    for (int i = g0; i < g1; ++i) base += carve_layer(M[i], N[i], base, ws_off + (int64_t)i * PSGD_KRON_QLIST_WS_REGIONS);
    for (int s = 0; s < PSGD_KRON_QLIST_STAGES; ++s) {
      int32_t* order = const_cast<int32_t*>(plan_order(plan, k, s));
      for (int i = g0; i < g1; ++i) order[i] = i;
      std::stable_sort(order + g0, order + g1, [&](int a, int b) { return sort_key(s, M[a], N[a]) > sort_key(s, M[b], N[b]); });
    }
    g0 = g1;
  }
  group_start[groups] = k;
  for (int s = 0; s < PSGD_KRON_QLIST_STAGES; ++s) {
    const int32_t* order = plan_order(plan, k, s);
    int32_t* prefix = const_cast<int32_t*>(plan_prefix(plan, k, s));
    int64_t sum = 0;
    for (int i = 0; i < k; ++i) {
      prefix[i] = (int32_t)sum;
      sum += stage_count(s, M[order[i]], N[order[i]]);
      if (sum > INT32_MAX) return PSGD_ERR_BAD_ARG;
    }
    prefix[k] = (int32_t)sum;
  }
  return groups;
}

int psgd_kron_qlist_apply_f32(const psgd_kron_qlist_layer* table, const int32_t* plan_dev, const int32_t* plan_host,
                              const int32_t* group_start, int groups, const int* M, const int* N, int k, void* ws, int64_t ws_bytes,
                              void* stream) {
  if (const int rc = check_call(table, plan_dev, plan_host, group_start, groups, M, N, k, ws, ws_bytes)) return rc;
  for (int g = 0; g < groups; ++g) {
    const Launch l{table, static_cast<char*>(ws), plan_dev, plan_host, k, group_start[g], group_start[g + 1],
                   static_cast<hipStream_t>(stream)};
    l.product(PSGD_KRON_QLIST_STAGE_PROD_MIN, kApply0);
    l.product(PSGD_KRON_QLIST_STAGE_PROD_MIN, kApply1);
    l.product(PSGD_KRON_QLIST_STAGE_PROD_MAX, kApply2);
    l.product(PSGD_KRON_QLIST_STAGE_PROD_MAX, kApply3);
  }
  return launched();
}

int psgd_kron_qlist_update_f32(const psgd_kron_qlist_layer* table, const int32_t* plan_dev, const int32_t* plan_host,
                               const int32_t* group_start, int groups, const int* M, const int* N, int k, float step, float decay,
                               void* ws, int64_t ws_bytes, void* stream) {
  if (const int rc = check_call(table, plan_dev, plan_host, group_start, groups, M, N, k, ws, ws_bytes)) return rc;
  const int U = PSGD_KRON_QLIST_STAGE_UPPER, F = PSGD_KRON_QLIST_STAGE_FULL;
  for (int g = 0; g < groups; ++g) {
    const Launch l{table, static_cast<char*>(ws), plan_dev, plan_host, k, group_start[g], group_start[g + 1],
                   static_cast<hipStream_t>(stream)};
    l.product(PSGD_KRON_QLIST_STAGE_PROD_M, kUpdateW);
    l.product(PSGD_KRON_QLIST_STAGE_PROD_N, kUpdateA);
    hipLaunchKernelGGL(k_list_gram, dim3(l.grid(U)), dim3(kT), 0, l.st, table, l.ws, plan_order(plan_dev, k, U),
                       plan_prefix(plan_dev, k, U), l.lo, l.hi);
    hipLaunchKernelGGL(k_list_lipschitz, dim3(2u * (unsigned)(l.hi - l.lo)), dim3(kLipT), 0, l.st, table, l.ws,
                       plan_order(plan_dev, k, U), l.lo, step, decay);
    hipLaunchKernelGGL(k_list_p1, dim3(l.grid(F)), dim3(kT), 0, l.st, table, l.ws, plan_order(plan_dev, k, F),
                       plan_prefix(plan_dev, k, F), l.lo, l.hi);
    hipLaunchKernelGGL(k_list_p2_sym, dim3(l.grid(U)), dim3(kT), 0, l.st, table, l.ws, plan_order(plan_dev, k, U),
                       plan_prefix(plan_dev, k, U), l.lo, l.hi);
  }
  return launched();
}

}  // extern "C"
