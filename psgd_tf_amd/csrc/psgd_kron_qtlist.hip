// psgd_kron_qtlist.hip -- the QUAD Kronecker update and apply on a LIST of ORDER-3 tensor layers [A, B, C] with three symmetric
// factors each, gfx950: the stages of psgd_kron_qnd.hip with one launch per stage for a whole GROUP of layers, and a Gram that is
// split along K where a side has few tiles and a long sum.  include/psgd_kron_quad_nd_list_hip.h has the contract.
//
// Why.  A conv kernel 64 x 64 x 9 is one tile per side: its per-layer update is seven launches of one to nine workgroups on a
// 256-CU device, and a network has twenty to fifty such layers.  Here the grid of a stage is the concatenation of the layers'
// grids, found as in psgd_kron_qlist.hip: a launch gets the device plan (per stage class an order[] of layers and a prefix[] of
// workgroup counts) and the positions [lo, hi) of its group; a workgroup bisects the prefix -- blockIdx and kernel arguments only,
// so layer and local number are uniform and live in scalar registers -- reads ONE record of the descriptor table, builds the
// Opnd / SegOpnd / GramSide / LipSide / StepSide views psgd_kron_qnd.hip builds on the host, and runs the per-layer tile body.
//
// Split Gram.  T_c of 512 x 512 x 9 is ONE 64 x 64 tile over K = 262 144: one workgroup walking 16 384 K steps while the device
// idles.  The Gram grid here is over (layer, side, upper tile, SLICE): a side with S > 1 (the slice rule of the header: a function
// of the side's shape and gram_slice_k alone) runs the product core over its slice [k0, k1) only -- the operand views advanced to
// k0, a multiple of the K step; the segmented operand of the middle mode takes k0 as an offset into its (a, c) pair index, so a
// slice may begin inside a slab -- and stores the raw accumulator fragment: four 16-byte stores per thread, fragment-major, no
// bounds logic (rows and columns past n are exact zeros).  The fold launch has one workgroup per split (layer, side, tile): each
// thread adds its 16 elements over the S partials in slice order in fp64, rounds once, and runs gram_epilogue() as if it had
// formed the tile itself.  A side with S = 1 is finished in the Gram launch, by the code of k_gram3: the per-layer bits.
//
// Update = 8 launches per group (3 mode products | Gram slices | fold | Lipschitz, three workgroups per layer | P1 | P2
// symmetrised; the fold is skipped when no side of the group is split), apply = 6 (launch i of a layer is its own mode
// order[i / 2]).  No atomics; every output element and every partial has one writer, every fold a fixed order.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "kron_quad_core.h"
#include "kron_quad_seg.h"
#include "psgd_kron_quad_nd_list_hip.h"

namespace psgdqt {
using namespace psgdq;

typedef psgd_kron_qtl_layer Layer;
static_assert(sizeof(Layer) == 232, "the host layer writes the table as rows of 29 int64");
constexpr int kFrag = 4 * kT;                // f32x4 per partial: one 64 x 64 accumulator tile, 16 KiB

// ------------------------------------------------------------------------------------------- shape rules, host and device
__host__ __device__ inline int tiles(int n) { return (n + kTile - 1) / kTile; }
__host__ __device__ inline int upper_of(int n) { return tiles(n) * (tiles(n) + 1) / 2; }
__host__ __device__ inline int side_n(int A, int B, int C, int s) { return s == 0 ? A : s == 1 ? B : C; }
__host__ __device__ inline int side_K(int A, int B, int C, int s) { return s == 0 ? B * C : s == 1 ? A * C : A * B; }

// the mode at place `at` of the apply: ascending extent, the lower mode first among equals (the stable sort of
// psgd_kron_qnd_apply_f32, as ranks)
__host__ __device__ inline int mode_at(int A, int B, int C, int at) {
  const int ra = (B < A) + (C < A), rb = (A <= B) + (C < B);
  return ra == at ? 0 : rb == at ? 1 : 2;
}

// the slice rule: S slices of `per` K steps (the last one has the rest)
struct Slices {
  int S, per;
};
__host__ __device__ inline Slices slices_of(int n, int K, int gsk) {
  const int steps = (K + kGK - 1) / kGK, u = upper_of(n);
  const long want = ((long)steps * kGK + gsk - 1) / gsk;
  const long room = u >= PSGD_KRON_QTL_CUS ? 1 : PSGD_KRON_QTL_CUS / u;
  const int S = (int)(want < room ? want : room);
  const int per = (steps + S - 1) / S;
  return Slices{(steps + per - 1) / per, per};
}

// --------------------------------------------------------------------------------------------------------------- the map
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// where workgroup blockIdx.x of a launch over the positions [lo, hi) works: the layer and the workgroup's number inside it
struct Where {
  int layer, local;
};
__device__ __forceinline__ Where locate(const int32_t* __restrict__ order, const int32_t* __restrict__ prefix, int lo, int hi) {
  const int b = (int)blockIdx.x + prefix[lo];
  while (hi - lo > 1) {                                 // prefix[lo] <= b < prefix[hi]: ends on a position with workgroups
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= b) lo = mid; else hi = mid;
  }
  return Where{uni(order[lo]), uni(b - prefix[lo])};
}

template <class T>
__device__ __forceinline__ T* region(char* ws, const Layer& d, int r) {
  return reinterpret_cast<T*>(ws + d.ws_off[r]);
}

// the views of side s of a layer, as psgd_kron_qnd_update_f32 builds them (the Gram operand of side 1 is `mid`: see k_tl_gram)
__device__ __forceinline__ GramSide gram_side(char* ws, const Layer& d, int s) {
  const int A = d.A, B = d.B, C = d.C, n = side_n(A, B, C, s), r = 5 * s;
  const float* X = region<float>(ws, d, PSGD_KRON_QTL_WS_X);
  const Opnd o = s == 0 ? Opnd{X, (long)B * C, 1, A} : s == 1 ? Opnd{nullptr, 0, 0, 0} : Opnd{X, 1, C, C};
  return GramSide{o, n, side_K(A, B, C, s), tiles(n), region<float>(ws, d, PSGD_KRON_QTL_WS_T + r),
                  region<float>(ws, d, PSGD_KRON_QTL_WS_TMAX + r), region<double>(ws, d, PSGD_KRON_QTL_WS_PART + r)};
}
__device__ __forceinline__ StepSide step_side(char* ws, const Layer& d, int s) {
  const int n = side_n(d.A, d.B, d.C, s), r = 5 * s;
  return StepSide{n, tiles(n), region<float>(ws, d, PSGD_KRON_QTL_WS_T + r), s == 0 ? d.Qa : s == 1 ? d.Qb : d.Qc,
                  region<float>(ws, d, PSGD_KRON_QTL_WS_P1 + r), (float)side_K(d.A, d.B, d.C, s)};
}

// a layer's workgroups of a stage run side a, then b, then c: which side `local` falls into (it becomes the number inside that
// side), the sides having c0, c1 and the rest
__device__ __forceinline__ int side_of(int& local, int c0, int c1) {
  if (local < c0) return 0;
  local -= c0;
  if (local < c1) return 1;
  local -= c1;
  return 2;
}

// the segmented operand seen from k0 on: step k of a slice is step k0 + k of the whole sum
struct SegSlice {
  SegOpnd o;
  int k0;
};
__device__ __forceinline__ void g2r(const SegSlice& s, int x0, int k, int K, float (&r)[4]) { g2r(s.o, x0, s.k0 + k, s.k0 + K, r); }
__device__ __forceinline__ void r2s(const SegSlice& s, const float (&r)[4], float* S) { r2s(s.o, r, S); }

// --------------------------------------------------------------------------------------------------------------- kernels
// one tile of one mode product of the workgroup's layer.  launch 0 .. 2: the update's X = G x1 Qa x2 Qb x3 Qc through X[0],
// X[1], X[0]; launch 3 + i: product i of the apply, mode mode_at(i / 2), G -> X[0] -> X[1] -> ... -> out.  The views are those
// of mode_product() of psgd_kron_qnd.hip, the tile decode that of k_mode.
__global__ __launch_bounds__(kT) void k_tl_mode(const Layer* __restrict__ table, char* __restrict__ ws, const int32_t* __restrict__ order,
                                                const int32_t* __restrict__ prefix, int lo, int hi, int launch) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const Where w = locate(order, prefix, lo, hi);
  const Layer& d = table[w.layer];
  const int A = d.A, B = d.B, C = d.C, AB = A * B, BC = B * C;
  float* X[2] = {region<float>(ws, d, PSGD_KRON_QTL_WS_X), region<float>(ws, d, PSGD_KRON_QTL_WS_X + 1)};
  const int i = launch - 3;
  const int mode = launch < 3 ? launch : mode_at(A, B, C, i >> 1);
  const float* src = launch < 3 ? (launch == 0 ? d.G : launch == 1 ? X[0] : X[1]) : (i == 0 ? d.G : ((i - 1) & 1) ? X[1] : X[0]);
  float* dst = launch < 3 ? (launch == 1 ? X[1] : X[0]) : (i == 5 ? d.out : (i & 1) ? X[1] : X[0]);
  const float* Q = mode == 0 ? d.Qa : mode == 1 ? d.Qb : d.Qc;
  Opnd a, b;
  int K, M, N;
  if (mode == 0) {                                      // [A, BC] view: Qa from the left
    a = Opnd{Q, A, 1, A}, b = Opnd{src, 1, BC, BC}, K = A, M = A, N = BC;
  } else if (mode == 1) {                               // per slab [B, C]: Qb from the left
    a = Opnd{Q, B, 1, B}, b = Opnd{src, 1, C, C}, K = B, M = B, N = C;
  } else {                                              // [AB, C] view: Qc from the right
    a = Opnd{src, C, 1, AB}, b = Opnd{Q, 1, C, C}, K = C, M = AB, N = C;
  }
  const int tiles_n = tiles(N), tiles_slab = tiles(M) * tiles_n;
  const int slab = w.local / tiles_slab, tile = w.local - slab * tiles_slab;      // (modes 1 and 3: one slab)
  const int m0 = (tile / tiles_n) * kTile, n0 = (tile % tiles_n) * kTile;
  b.p += slab * (long)BC;
  float* Cs = dst + slab * (long)BC;
  f32x4 acc[2][2];
  product(a, b, K, m0, n0, lds, acc);
  each_elem([&](int i_, int j, int e, int r, int c) {
    if (m0 + r < M && n0 + c < N) Cs[(long)(m0 + r) * N + (n0 + c)] = acc[i_][j][e];
  });
}

// the Gram slices of the workgroup's layer: (side, upper tile, slice).  S = 1: the whole sum and the epilogue, as k_gram3.
// S > 1: the slice's sum, its raw fragment to partial number tile S + slice of the side.
__global__ __launch_bounds__(kT) void k_tl_gram(const Layer* __restrict__ table, char* __restrict__ ws, const int32_t* __restrict__ order,
                                                const int32_t* __restrict__ prefix, int lo, int hi, int gsk) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  __shared__ float red[kT / 64];
  const Where w = locate(order, prefix, lo, hi);
  const Layer& d = table[w.layer];
  const int A = d.A, B = d.B, C = d.C;
  int local = w.local;
  const int side = side_of(local, upper_of(A) * slices_of(A, B * C, gsk).S, upper_of(B) * slices_of(B, A * C, gsk).S);
  const GramSide s = gram_side(ws, d, side);
  const Slices sl = slices_of(s.n, s.K, gsk);
  const int u = local / sl.S, slice = local - u * sl.S;
  int ti, tj;
  upper_tile(u, s.nb, ti, tj);
  const SegOpnd mid{region<float>(ws, d, PSGD_KRON_QTL_WS_X), (long)B * C, C, B};
  f32x4 acc[2][2];
  if (sl.S == 1) {
    if (side == 1)
      product_of(mid, mid, s.K, ti * kTile, tj * kTile, lds, acc);
    else
      product(s.o, s.o, s.K, ti * kTile, tj * kTile, lds, acc);
    gram_epilogue(s, ti, tj, acc, lds, red);
    return;
  }
  const int k0 = slice * sl.per * kGK, len = min(s.K - k0, sl.per * kGK);
  if (side == 1) {
    const SegSlice m{mid, k0};
    product_of(m, m, len, ti * kTile, tj * kTile, lds, acc);
  } else {
    Opnd o = s.o;
    o.p += (long)k0 * o.ks;                             // k0 * ks is a multiple of 16 floats: the load route does not change
    product(o, o, len, ti * kTile, tj * kTile, lds, acc);
  }
  f32x4* P = region<f32x4>(ws, d, PSGD_KRON_QTL_WS_SLICES + side) + (long)local * kFrag + threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) P[q * kT] = acc[q >> 1][q & 1];
}

// one workgroup per split (side, upper tile) of the workgroup's layer: the S partials added in slice order in fp64, rounded once,
// then the Gram epilogue
__global__ __launch_bounds__(kT) void k_tl_fold(const Layer* __restrict__ table, char* __restrict__ ws, const int32_t* __restrict__ order,
                                                const int32_t* __restrict__ prefix, int lo, int hi, int gsk) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  __shared__ float red[kT / 64];
  const Where w = locate(order, prefix, lo, hi);
  const Layer& d = table[w.layer];
  const int A = d.A, B = d.B, C = d.C;
  int local = w.local;
  const int side = side_of(local, slices_of(A, B * C, gsk).S > 1 ? upper_of(A) : 0, slices_of(B, A * C, gsk).S > 1 ? upper_of(B) : 0);
  const GramSide s = gram_side(ws, d, side);
  const int S = slices_of(s.n, s.K, gsk).S;
  int ti, tj;
  upper_tile(local, s.nb, ti, tj);
  const f32x4* P = region<f32x4>(ws, d, PSGD_KRON_QTL_WS_SLICES + side) + (long)local * S * kFrag + threadIdx.x;
  f32x4 acc[2][2];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < S; ++i) {
      const f32x4 v = P[(long)i * kFrag + q * kT];
#pragma unroll
      for (int e = 0; e < 4; ++e) sum[e] += (double)v[e];
    }
    acc[q >> 1][q & 1] = f32x4{(float)sum[0], (float)sum[1], (float)sum[2], (float)sum[3]};
  }
  gram_epilogue(s, ti, tj, acc, lds, red);
}

// three workgroups per layer, position blockIdx.x / 3 of the group: L (in place) and c of side blockIdx.x % 3
__global__ __launch_bounds__(kLipT) void k_tl_lipschitz(const Layer* __restrict__ table, char* __restrict__ ws,
                                                        const int32_t* __restrict__ order, int lo, float step, float decay) {
  __shared__ double red[kLipT];
  __shared__ int redi[kLipT];
  __shared__ float redf[kLipT / 64];
  const Layer& d = table[uni(order[lo + (int)(blockIdx.x / 3)])];
  const int side = blockIdx.x % 3, n = side_n(d.A, d.B, d.C, side), r = 5 * side;
  const LipSide s{n, tiles(n), region<float>(ws, d, PSGD_KRON_QTL_WS_T + r), region<float>(ws, d, PSGD_KRON_QTL_WS_TMAX + r),
                  region<double>(ws, d, PSGD_KRON_QTL_WS_PART + r), region<double>(ws, d, PSGD_KRON_QTL_WS_VEC + r),
                  (double)side_K(d.A, d.B, d.C, side)};
  lipschitz_dense(s, d.L + side, region<float>(ws, d, PSGD_KRON_QTL_WS_COEF) + side, step, decay, red, redi, redf);
}

// P1 = Q - c (T Q - t2 Q): every tile of the three sides of the workgroup's layer
__global__ __launch_bounds__(kT) void k_tl_p1(const Layer* __restrict__ table, char* __restrict__ ws, const int32_t* __restrict__ order,
                                              const int32_t* __restrict__ prefix, int lo, int hi) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const Where w = locate(order, prefix, lo, hi);
  const Layer& d = table[w.layer];
  int local = w.local;
  const int side = side_of(local, tiles(d.A) * tiles(d.A), tiles(d.B) * tiles(d.B));
  p1_tile(step_side(ws, d, side), local, region<float>(ws, d, PSGD_KRON_QTL_WS_COEF)[side], lds);
}

// Q <- (P2 + P2') / 2 over the upper tiles of the three sides of the workgroup's layer: the body of k_p2_sym3
__global__ __launch_bounds__(kT) void k_tl_p2_sym(const Layer* __restrict__ table, char* __restrict__ ws,
                                                  const int32_t* __restrict__ order, const int32_t* __restrict__ prefix, int lo, int hi) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const Where w = locate(order, prefix, lo, hi);
  const Layer& d = table[w.layer];
  int local = w.local;
  const int side = side_of(local, upper_of(d.A), upper_of(d.B));
  const StepSide s = step_side(ws, d, side);
  const float c1 = region<float>(ws, d, PSGD_KRON_QTL_WS_COEF)[side];
  int ti, tj;
  upper_tile(local, s.nb, ti, tj);
  const int m0 = ti * kTile, n0 = tj * kTile;
  f32x4 up[2][2];
  p2_tile(s, c1, m0, n0, lds, up);
  if (ti == tj) {
    p2_sym_store(s, m0, n0, true, up, up, lds);
  } else {
    f32x4 lo_[2][2];
    p2_tile(s, c1, n0, m0, lds, lo_);
    p2_sym_store(s, m0, n0, false, up, lo_, lds);
  }
}

// --------------------------------------------------------------------------------------------------------------- the host
struct Shapes {
  const int *A, *B, *C;
  int k, gsk;
  bool ok() const {
    if (!A || !B || !C || k < 1 || gsk < kGK || gsk % kGK) return false;
    for (int i = 0; i < k; ++i)
      if (A[i] < 1 || B[i] < 1 || C[i] < 1 || (int64_t)A[i] * B[i] * C[i] > INT32_MAX) return false;
    return true;
  }
  Slices slices(int i, int s) const { return slices_of(side_n(A[i], B[i], C[i], s), side_K(A[i], B[i], C[i], s), gsk); }

  // the carve of layer i from byte `base` on: the regions of the per-layer workspace in its order, then the partials
  int64_t carve(int i, int64_t base, int64_t* off) const {
    int64_t at = base, scratch[PSGD_KRON_QTL_WS_REGIONS];
    if (!off) off = scratch;
    auto take = [&](int r, int64_t bytes) {
      off[r] = at;
      at += up256(bytes);
    };
    const int64_t numel = (int64_t)A[i] * B[i] * C[i];
    take(PSGD_KRON_QTL_WS_X, numel * 4);
    take(PSGD_KRON_QTL_WS_X + 1, numel * 4);
    for (int s = 0; s < 3; ++s) {
      const int64_t n = side_n(A[i], B[i], C[i], s), nb = tiles((int)n);
      take(PSGD_KRON_QTL_WS_T + 5 * s, n * n * 4);
      take(PSGD_KRON_QTL_WS_P1 + 5 * s, n * n * 4);
      take(PSGD_KRON_QTL_WS_TMAX + 5 * s, nb * nb * 4);
      take(PSGD_KRON_QTL_WS_PART + 5 * s, nb * n * 8);
      take(PSGD_KRON_QTL_WS_VEC + 5 * s, 2 * n * 8);
    }
    take(PSGD_KRON_QTL_WS_COEF, 3 * 4);
    for (int s = 0; s < 3; ++s) {
      const int S = slices(i, s).S;
      take(PSGD_KRON_QTL_WS_SLICES + s, S > 1 ? (int64_t)S * upper_of(side_n(A[i], B[i], C[i], s)) * kFrag * 16 : 0);
    }
    return at - base;
  }

  // the end (exclusive) of the group that begins at layer g0, and its bytes
  int group_end(int64_t cap, int g0, int64_t* bytes) const {
    int64_t sum = carve(g0, 0, nullptr);
    int g1 = g0 + 1;
    for (; g1 < k; ++g1) {
      const int64_t b = carve(g1, 0, nullptr);
      if (sum + b > cap) break;
      sum += b;
    }
    *bytes = sum;
    return g1;
  }

  int64_t mode_count(int i, int mode) const {
    const int64_t a = A[i], b = B[i], c = C[i];
    if (mode == 0) return (int64_t)tiles((int)a) * tiles((int)(b * c));
    if (mode == 1) return a * tiles((int)b) * tiles((int)c);
    return (int64_t)tiles((int)(a * b)) * tiles((int)c);
  }
  int64_t count(int stage, int i) const {
    const int a = A[i], b = B[i], c = C[i];
    int64_t sum = 0;
    switch (stage) {
      case PSGD_KRON_QTL_STAGE_MODE_A:
      case PSGD_KRON_QTL_STAGE_MODE_B:
      case PSGD_KRON_QTL_STAGE_MODE_C: return mode_count(i, stage);
      case PSGD_KRON_QTL_STAGE_APPLY_0:
      case PSGD_KRON_QTL_STAGE_APPLY_1:
      case PSGD_KRON_QTL_STAGE_APPLY_2: return mode_count(i, mode_at(a, b, c, stage - PSGD_KRON_QTL_STAGE_APPLY_0));
      case PSGD_KRON_QTL_STAGE_GRAM:
        for (int s = 0; s < 3; ++s) sum += (int64_t)upper_of(side_n(a, b, c, s)) * slices(i, s).S;
        return sum;
      case PSGD_KRON_QTL_STAGE_FOLD:
        for (int s = 0; s < 3; ++s) sum += slices(i, s).S > 1 ? upper_of(side_n(a, b, c, s)) : 0;
        return sum;
      case PSGD_KRON_QTL_STAGE_UPPER: return upper_of(a) + upper_of(b) + upper_of(c);
      default: return (int64_t)tiles(a) * tiles(a) + (int64_t)tiles(b) * tiles(b) + (int64_t)tiles(c) * tiles(c);
    }
  }
  int sort_key(int stage, int i) const {
    const int a = A[i], b = B[i], c = C[i];
    int key = 0;
    switch (stage) {
      case PSGD_KRON_QTL_STAGE_MODE_A:
      case PSGD_KRON_QTL_STAGE_MODE_B:
      case PSGD_KRON_QTL_STAGE_MODE_C: return side_n(a, b, c, stage);
      case PSGD_KRON_QTL_STAGE_APPLY_0:
      case PSGD_KRON_QTL_STAGE_APPLY_1:
      case PSGD_KRON_QTL_STAGE_APPLY_2: return side_n(a, b, c, mode_at(a, b, c, stage - PSGD_KRON_QTL_STAGE_APPLY_0));
      case PSGD_KRON_QTL_STAGE_GRAM:
        for (int s = 0; s < 3; ++s) key = std::max(key, std::min(side_K(a, b, c, s), slices(i, s).per * kGK));
        return key;
      case PSGD_KRON_QTL_STAGE_FOLD:
        for (int s = 0; s < 3; ++s) key = std::max(key, slices(i, s).S);
        return key;
      default: return std::max(a, std::max(b, c));
    }
  }
};

static const int32_t* plan_order(const int32_t* plan, int k, int stage) { return plan + (int64_t)stage * (2 * k + 1); }
static const int32_t* plan_prefix(const int32_t* plan, int k, int stage) { return plan_order(plan, k, stage) + k; }

// what the entry points check before any HIP call
static int check_call(const void* table, const int32_t* plan_dev, const int32_t* plan, const int32_t* gs, int groups, const Shapes& sh,
                      const void* ws, int64_t ws_bytes) {
  const int k = sh.k;
  if (!table || !plan_dev || !plan || !gs || !sh.ok() || groups < 1 || groups > k || gs[0] != 0 || gs[groups] != k) return PSGD_ERR_BAD_ARG;
  int64_t need = 0;
  for (int g = 0; g < groups; ++g) {
    if (gs[g + 1] <= gs[g] || gs[g + 1] > k) return PSGD_ERR_BAD_ARG;
    int64_t sum = 0;
    for (int i = gs[g]; i < gs[g + 1]; ++i) sum += sh.carve(i, 0, nullptr);
    need = std::max(need, sum);
    for (int s = 0; s < PSGD_KRON_QTL_STAGES; ++s) {     // every position a layer of this group, with that layer's workgroups
      const int32_t *order = plan_order(plan, k, s), *prefix = plan_prefix(plan, k, s);
      for (int i = gs[g]; i < gs[g + 1]; ++i) {
        const int l = order[i];
        if (l < gs[g] || l >= gs[g + 1] || (int64_t)prefix[i + 1] - prefix[i] != sh.count(s, l)) return PSGD_ERR_BAD_ARG;
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
  const int32_t* order(int stage) const { return plan_order(plan_dev, k, stage); }
  const int32_t* prefix(int stage) const { return plan_prefix(plan_dev, k, stage); }
  void mode(int stage, int launch) const {
    hipLaunchKernelGGL(k_tl_mode, dim3(grid(stage)), dim3(kT), 0, st, table, ws, order(stage), prefix(stage), lo, hi, launch);
  }
};

}  // namespace psgdqt

using namespace psgdqt;

extern "C" {

int64_t psgd_kron_qtl_workspace_bytes(const int* A, const int* B, const int* C, int k, int64_t max_group_bytes, int gram_slice_k) {
  const Shapes sh{A, B, C, k, gram_slice_k};
  if (!sh.ok()) return PSGD_ERR_BAD_ARG;
  int64_t need = 0, bytes;
  for (int g0 = 0; g0 < k;) {
    g0 = sh.group_end(max_group_bytes, g0, &bytes);
    need = std::max(need, bytes);
  }
  return need;
}

int psgd_kron_qtl_plan(const int* A, const int* B, const int* C, int k, int64_t max_group_bytes, int gram_slice_k, int32_t* group_start,
                       int32_t* plan, int64_t* ws_off, int32_t* slices) {
  const Shapes sh{A, B, C, k, gram_slice_k};
  if (!sh.ok() || !group_start || !plan || !ws_off || !slices) return PSGD_ERR_BAD_ARG;
  int groups = 0;
  for (int g0 = 0; g0 < k;) {
    int64_t bytes;
    const int g1 = sh.group_end(max_group_bytes, g0, &bytes);
    group_start[groups++] = g0;
    int64_t base = 0;
    for (int i = g0; i < g1; ++i) base += sh.carve(i, base, ws_off + (int64_t)i * PSGD_KRON_QTL_WS_REGIONS);
    for (int s = 0; s < PSGD_KRON_QTL_STAGES; ++s) {
      int32_t* order = const_cast<int32_t*>(plan_order(plan, k, s));
      for (int i = g0; i < g1; ++i) order[i] = i;
      std::stable_sort(order + g0, order + g1, [&](int a, int b) { return sh.sort_key(s, a) > sh.sort_key(s, b); });
    }
    g0 = g1;
  }
  group_start[groups] = k;
  for (int i = 0; i < k; ++i)
    for (int s = 0; s < 3; ++s) slices[3 * i + s] = sh.slices(i, s).S;
  for (int s = 0; s < PSGD_KRON_QTL_STAGES; ++s) {
    const int32_t* order = plan_order(plan, k, s);
    int32_t* prefix = const_cast<int32_t*>(plan_prefix(plan, k, s));
    int64_t sum = 0;
    for (int i = 0; i < k; ++i) {
      prefix[i] = (int32_t)sum;
      sum += sh.count(s, order[i]);
      if (sum > INT32_MAX) return PSGD_ERR_BAD_ARG;
    }
    prefix[k] = (int32_t)sum;
  }
  return groups;
}

int psgd_kron_qtl_apply_f32(const psgd_kron_qtl_layer* table, const int32_t* plan_dev, const int32_t* plan_host,
                            const int32_t* group_start, int groups, const int* A, const int* B, const int* C, int k, int gram_slice_k,
                            void* ws, int64_t ws_bytes, void* stream) {
  const Shapes sh{A, B, C, k, gram_slice_k};
  if (const int rc = check_call(table, plan_dev, plan_host, group_start, groups, sh, ws, ws_bytes)) return rc;
  for (int g = 0; g < groups; ++g) {
    const Launch l{table, static_cast<char*>(ws), plan_dev, plan_host, k, group_start[g], group_start[g + 1],
                   static_cast<hipStream_t>(stream)};
    for (int i = 0; i < 6; ++i) l.mode(PSGD_KRON_QTL_STAGE_APPLY_0 + i / 2, 3 + i);
  }
  return launched();
}

int psgd_kron_qtl_update_f32(const psgd_kron_qtl_layer* table, const int32_t* plan_dev, const int32_t* plan_host,
                             const int32_t* group_start, int groups, const int* A, const int* B, const int* C, int k, int gram_slice_k,
                             float step, float decay, void* ws, int64_t ws_bytes, void* stream) {
  const Shapes sh{A, B, C, k, gram_slice_k};
  if (const int rc = check_call(table, plan_dev, plan_host, group_start, groups, sh, ws, ws_bytes)) return rc;
  const int G = PSGD_KRON_QTL_STAGE_GRAM, D = PSGD_KRON_QTL_STAGE_FOLD, U = PSGD_KRON_QTL_STAGE_UPPER, F = PSGD_KRON_QTL_STAGE_FULL;
  for (int g = 0; g < groups; ++g) {
    const Launch l{table, static_cast<char*>(ws), plan_dev, plan_host, k, group_start[g], group_start[g + 1],
                   static_cast<hipStream_t>(stream)};
    for (int m = 0; m < 3; ++m) l.mode(PSGD_KRON_QTL_STAGE_MODE_A + m, m);
    hipLaunchKernelGGL(k_tl_gram, dim3(l.grid(G)), dim3(kT), 0, l.st, table, l.ws, l.order(G), l.prefix(G), l.lo, l.hi, gram_slice_k);
    if (l.grid(D))                                      // (no split side in this group: nothing to fold)
      hipLaunchKernelGGL(k_tl_fold, dim3(l.grid(D)), dim3(kT), 0, l.st, table, l.ws, l.order(D), l.prefix(D), l.lo, l.hi, gram_slice_k);
    hipLaunchKernelGGL(k_tl_lipschitz, dim3(3u * (unsigned)(l.hi - l.lo)), dim3(kLipT), 0, l.st, table, l.ws, l.order(U), l.lo, step,
                       decay);
    hipLaunchKernelGGL(k_tl_p1, dim3(l.grid(F)), dim3(kT), 0, l.st, table, l.ws, l.order(F), l.prefix(F), l.lo, l.hi);
    hipLaunchKernelGGL(k_tl_p2_sym, dim3(l.grid(U)), dim3(kT), 0, l.st, table, l.ws, l.order(U), l.prefix(U), l.lo, l.hi);
  }
  return launched();
}

}  // extern "C"
