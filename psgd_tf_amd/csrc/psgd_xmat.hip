// psgd_xmat.hip -- the X-shaped preconditioner Q = diag(a) + adiag(b) (and, with b absent, the diagonal one) on gfx950.
//
// The math is in include/psgd_xmat_hip.h.  With j = N-1-i every pair (i, j) is an independent 2 x 2 block; the only global
// quantity of the update is max(max|nablaA|, max|nablaB|).
//
// Ownership.  A thread owns whole PAIRS: kE front elements and their kE mirrors from the back.  It reads a, b, v, h (and g) for
// both ends and writes both ends, so the in-place rewrite of a and b needs no ordering between workgroups, and the mirrored
// operand of every formula is already in a register.  P = ceil(N / 2) pairs; for odd N the last one is the middle element, whose
// mirror is itself: it is computed as a pair with both ends equal, nablaB forced to 0, and stored once.  A workgroup owns
// kT * kE = 1024 pairs (2048 elements) per trip of a grid-stride loop.
//
// Two routes, chosen per call on the host:
//   VEC    every pointer 16-byte aligned and N % 4 == 0 (then the back stream N-4-i0 is 16-byte aligned too).  A thread's kE = 4
//          front elements are one 16-byte load, its mirrors one 16-byte load reversed in registers; stores likewise.  Only quads
//          whose four pairs are all two-element pairs (i0 + 4 <= floor(N / 2)) go this way, so no vector store ever covers an
//          element another thread owns; the one quad where the front and back runs meet (and the quads past it, which own nothing)
//          takes the dword path below with its per-element masks.
//   dword  anything else (N % 4 != 0 or a base skewed by 4, 8 or 12 bytes).  Pair e of a thread is tile * 1024 + e * 256 + tid:
//          consecutive lanes read consecutive dwords on both streams, the back one descending, so every access is fully coalesced
//          whatever the alignment.  (The alternative, aligned 16-byte loads plus a rotate through a neighbour lane's registers,
//          was not built: the dword route already moves whole cache lines per wave instruction.)
//
// Update = two launches.  k_nabla_max forms nablaA, nablaB per pair and reduces the NaN-propagating maximum (nanmax.h: a maximum
// of bit patterns, exact in any order) to one partial per workgroup.  k_rewrite folds those partials itself -- every workgroup
// the same <= 2048 floats in the same order, 8 KiB out of L2 -- so there is no finalize launch, no cooperative launch and no
// grid-wide wait; it then RECOMPUTES the pair quantities (16 B per parameter of reads, against 16 B of traffic plus a buffer for
// a stored nabla) and rewrites a and b.  With APPLY it also reads g and forms out from the NEW a, b still in registers: the
// fused update -> apply (48 B per parameter instead of 40 + 16).  The separate apply is the same kernel without UPD.  All
// arithmetic is written with explicit fmaf / __f*_rn so that no context-dependent contraction can make the fused call differ
// from update-then-apply: they are bit-identical.
//
// Launch shape, decided by measurement at N = 100M (profiles/xmat_timing.txt): the reading sweep runs up to kReadGrid = 2048
// workgroups (8 per CU), the writing sweeps kWriteGrid = 1024 (4 per CU, the project's rule for streams that are written: 8 per
// CU measured 1 % slower on the fused call and 4 % on the update); g and out, touched once, go non-temporal from kNtMinN elements
// on (without: fused 2.6 % and apply 3.5 % slower; below that size the operands sit in the Infinity Cache and a later kernel
// finds them there).  Both differences are small, from single A/B runs.  The 16-byte route runs the writing sweep at the
// project's in-place rewrite rate; the dword route reaches about three quarters of it.  Indices are 64-bit throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "psgd_xmat_hip.h"
#include "nanmax.h"
using psgd::amaxf;

#ifndef PSGD_XMAT_WRITE_GRID
#define PSGD_XMAT_WRITE_GRID 1024
#endif
#ifndef PSGD_XMAT_NT_MIN_N
#define PSGD_XMAT_NT_MIN_N (int64_t(16) << 20)
#endif

namespace psgdx {

constexpr int kT = 256;                        // threads per workgroup
constexpr int kE = 4;                          // pairs per thread per trip
constexpr int64_t kTilePairs = (int64_t)kT * kE;
static_assert(2 * kTilePairs == PSGD_XMAT_TILE_ELEMS, "header and kernel disagree on the tile");
constexpr int kReadGrid = PSGD_XMAT_MAX_GRID;
constexpr int kWriteGrid = PSGD_XMAT_WRITE_GRID;
static_assert(kWriteGrid <= kReadGrid, "the writing sweeps never run more workgroups than the reading one");
constexpr int64_t kNtMinN = PSGD_XMAT_NT_MIN_N;

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ f32x4 ld4(const float* p) {
  const f32x4* q = reinterpret_cast<const f32x4*>(p);
  if constexpr (NT) return __builtin_nontemporal_load(q); else return *q;
}
template <bool NT>
__device__ __forceinline__ void st4(float* p, f32x4 v) {
  f32x4* q = reinterpret_cast<f32x4*>(p);
  if constexpr (NT) __builtin_nontemporal_store(v, q); else *q = v;
}
template <bool NT>
__device__ __forceinline__ float ld1(const float* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p); else return *p;
}
template <bool NT>
__device__ __forceinline__ void st1(float* p, float v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p); else *p = v;
}

__device__ __forceinline__ float wave_amax(float v) {
  for (int o = 32; o > 0; o >>= 1) v = amaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// the workgroup's maximum, in every thread
__device__ __forceinline__ float block_amax(float m) {
  __shared__ float red[kT / 64];
  m = wave_amax(m);
  __syncthreads();                                      // (red may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  return amaxf(amaxf(red[0], red[1]), amaxf(red[2], red[3]));
}

// ---------------------------------------------------------------------------------------------------- the pair arithmetic
// out_i = a_i w_i + b_j w_j with w = a*g + b*flip(g), both ends of the pair
__device__ __forceinline__ void pair_apply(float ai, float aj, float bi, float bj, float gi, float gj, float& oi, float& oj) {
  const float wi = fmaf(ai, gi, __fmul_rn(bi, gj));
  const float wj = fmaf(aj, gj, __fmul_rn(bj, gi));
  oi = fmaf(ai, wi, __fmul_rn(bj, wj));
  oj = fmaf(aj, wj, __fmul_rn(bi, wi));
}
// nablaA at both ends and the pair's nablaB (0 for the middle element)
__device__ __forceinline__ void pair_nabla(float ai, float aj, float bi, float bj, float vi, float vj, float hi, float hj, bool mid,
                                           float& nAi, float& nAj, float& nB) {
  const float Ai = fmaf(ai, hi, __fmul_rn(bi, hj));
  const float Aj = fmaf(aj, hj, __fmul_rn(bj, hi));
  const float det = fmaf(ai, aj, -__fmul_rn(bi, bj));
  const float Bi = __fdiv_rn(fmaf(aj, vi, -__fmul_rn(bj, vj)), det);
  const float Bj = __fdiv_rn(fmaf(ai, vj, -__fmul_rn(bi, vi)), det);
  nAi = fmaf(Ai, Ai, -__fmul_rn(Bi, Bi));
  nAj = fmaf(Aj, Aj, -__fmul_rn(Bj, Bj));
  nB = mid ? 0.f : fmaf(Ai, Aj, -__fmul_rn(Bi, Bj));
}
// x - mu (nA x + nB y): nA = nB = 0 gives x - mu 0 = x, bit for bit
__device__ __forceinline__ float stepped(float x, float y, float nA, float nB, float mu) {
  return __fsub_rn(x, __fmul_rn(mu, fmaf(nA, x, __fmul_rn(nB, y))));
}

// ------------------------------------------------------------------------------------------------- who owns what, and I/O
struct Own {
  int64_t i0;            // VEC: the first front element of the quad
  int64_t i[kE];         // the front element of pair e
  bool on[kE], mid[kE];  // the pair exists; it is the middle element (its own mirror)
  bool vec;              // all four are two-element pairs of one aligned quad: 16-byte accesses, no masks
};
template <bool VEC>
__device__ __forceinline__ Own own_of(int64_t tile, int64_t N) {
  const int64_t H = N / 2, P = N - H;                   // two-element pairs; pairs including the middle element of an odd N
  Own o;
  o.i0 = (tile * kT + threadIdx.x) * kE;
  o.vec = VEC && o.i0 + kE <= H;
#pragma unroll
  for (int e = 0; e < kE; ++e) {
    o.i[e] = VEC ? o.i0 + e : tile * kTilePairs + (int64_t)e * kT + threadIdx.x;
    o.on[e] = o.i[e] < P;
    o.mid[e] = o.on[e] && o.i[e] >= H;
  }
  return o;
}

// one stream's values for the thread's pairs: f[e] the front element i_e, r[e] its mirror N-1-i_e
struct Run {
  float f[kE], r[kE];
};
__device__ __forceinline__ Run zeros() {
  Run x;
#pragma unroll
  for (int e = 0; e < kE; ++e) x.f[e] = x.r[e] = 0.f;
  return x;
}
template <bool NT>
__device__ __forceinline__ Run load_run(const float* p, const Own& o, int64_t N) {
  Run x;
  if (o.vec) {                                          // [i0, i0+4) and [N-4-i0, N-i0): inside [0, N/2) and [N/2, N)
    const f32x4 f = ld4<NT>(p + o.i0), r = ld4<NT>(p + (N - kE - o.i0));
#pragma unroll
    for (int e = 0; e < kE; ++e) {
      x.f[e] = f[e];
      x.r[e] = r[kE - 1 - e];                           // the back run, reversed in registers
    }
  } else {
#pragma unroll
    for (int e = 0; e < kE; ++e) {                      // i < P <= N and N-1-i >= N-P >= 0
      x.f[e] = o.on[e] ? ld1<NT>(p + o.i[e]) : 0.f;
      x.r[e] = !o.on[e] ? 0.f : o.mid[e] ? x.f[e] : ld1<NT>(p + (N - 1 - o.i[e]));
    }
  }
  return x;
}
template <bool NT>
__device__ __forceinline__ void store_run(float* p, const Own& o, int64_t N, const Run& x) {
  if (o.vec) {
    f32x4 f, r;
#pragma unroll
    for (int e = 0; e < kE; ++e) {
      f[e] = x.f[e];
      r[kE - 1 - e] = x.r[e];
    }
    st4<NT>(p + o.i0, f);
    st4<NT>(p + (N - kE - o.i0), r);
  } else {
#pragma unroll
    for (int e = 0; e < kE; ++e) {                      // owned elements only; the middle element once
      if (o.on[e]) st1<NT>(p + o.i[e], x.f[e]);
      if (o.on[e] && !o.mid[e]) st1<NT>(p + (N - 1 - o.i[e]), x.r[e]);
    }
  }
}

__device__ __forceinline__ int64_t tiles_of(int64_t N) { return (N - N / 2 + kTilePairs - 1) / kTilePairs; }

// ------------------------------------------------------------------------------------------------------------- the sweeps
// update, launch 1: partial[blockIdx.x] = this workgroup's max(|nablaA|, |nablaB|) over the pairs it owns
template <bool VEC, bool DIAG>
__global__ __launch_bounds__(kT) void k_nabla_max(const float* __restrict__ a, const float* __restrict__ b,
                                                  const float* __restrict__ v, const float* __restrict__ h,
                                                  float* __restrict__ partial, int64_t N) {
  float m = 0.f;
  const int64_t tiles = tiles_of(N);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const Own o = own_of<VEC>(tile, N);
    const Run A = load_run<false>(a, o, N), B = DIAG ? zeros() : load_run<false>(b, o, N);
    const Run V = load_run<false>(v, o, N), Hh = load_run<false>(h, o, N);
#pragma unroll
    for (int e = 0; e < kE; ++e) {
      if (o.vec || o.on[e]) {
        float nAi, nAj, nB;
        pair_nabla(A.f[e], A.r[e], B.f[e], B.r[e], V.f[e], V.r[e], Hh.f[e], Hh.r[e], !o.vec && o.mid[e], nAi, nAj, nB);
        if (DIAG) nB = 0.f;
        m = amaxf(m, amaxf(amaxf(fabsf(nAi), fabsf(nAj)), fabsf(nB)));
      }
    }
  }
  m = block_amax(m);
  if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// update launch 2 (UPD), the apply (APPLY), or both in one pass: the fused update -> apply
template <bool VEC, bool DIAG, bool UPD, bool APPLY, bool NT>
__global__ __launch_bounds__(kT) void k_rewrite(float* a, float* b, const float* __restrict__ v, const float* __restrict__ h,
                                                const float* __restrict__ g, float* __restrict__ out,
                                                const float* __restrict__ partial, int nparts, int64_t N, float step, float tiny) {
  float mu = 0.f;
  if constexpr (UPD) {                                  // every workgroup folds the same partials in the same order
    float m = 0.f;
    for (int k = threadIdx.x; k < nparts; k += kT) m = amaxf(m, partial[k]);
    mu = __fdiv_rn(step, __fadd_rn(block_amax(m), tiny));
  }
  const int64_t tiles = tiles_of(N);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const Own o = own_of<VEC>(tile, N);
    Run A = load_run<false>(a, o, N), B = DIAG ? zeros() : load_run<false>(b, o, N);
    Run G;
    if constexpr (APPLY) G = load_run<NT>(g, o, N);     // issued ahead of the update's arithmetic
    if constexpr (UPD) {
      const Run V = load_run<false>(v, o, N), Hh = load_run<false>(h, o, N);
#pragma unroll
      for (int e = 0; e < kE; ++e) {
        if (o.vec || o.on[e]) {
          float nAi, nAj, nB;
          pair_nabla(A.f[e], A.r[e], B.f[e], B.r[e], V.f[e], V.r[e], Hh.f[e], Hh.r[e], !o.vec && o.mid[e], nAi, nAj, nB);
          if (DIAG) nB = 0.f;
          const float ai = A.f[e], aj = A.r[e], bi = B.f[e], bj = B.r[e];       // old a, b on the right
          A.f[e] = stepped(ai, bj, nAi, nB, mu);
          A.r[e] = stepped(aj, bi, nAj, nB, mu);
          if (!DIAG) {
            B.f[e] = stepped(bi, aj, nAi, nB, mu);
            B.r[e] = stepped(bj, ai, nAj, nB, mu);
          }
        }
      }
      store_run<false>(a, o, N, A);
      if (!DIAG) store_run<false>(b, o, N, B);
    }
    if constexpr (APPLY) {
      Run O;
#pragma unroll
      for (int e = 0; e < kE; ++e) pair_apply(A.f[e], A.r[e], B.f[e], B.r[e], G.f[e], G.r[e], O.f[e], O.r[e]);
      store_run<NT>(out, o, N, O);
    }
  }
}

// --------------------------------------------------------------------------------------------------------------- the host
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static int launched() { return hipGetLastError() == hipSuccess ? PSGD_OK : PSGD_ERR_LAUNCH; }
static unsigned grid_of(int64_t N, int cap) {
  const int64_t tiles = (N - N / 2 + kTilePairs - 1) / kTilePairs;
  return (unsigned)(tiles < cap ? tiles : cap);
}
static int ws_check(const void* ws, int64_t ws_bytes) {
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) || ws_bytes < (int64_t)kReadGrid * (int64_t)sizeof(float)) return PSGD_ERR_WORKSPACE;
  return PSGD_OK;
}

// f(VEC, DIAG, NT) with the three flags as compile-time constants
template <class F>
static void with_flags(bool vec, bool diag, bool nt, F&& f) {
  auto d2 = [&](auto V, auto D) {
    if (nt) f(V, D, std::true_type{}); else f(V, D, std::false_type{});
  };
  auto d1 = [&](auto V) {
    if (diag) d2(V, std::true_type{}); else d2(V, std::false_type{});
  };
  if (vec) d1(std::true_type{}); else d1(std::false_type{});
}

// update (g == out == nullptr), apply (v == h == nullptr, nothing of the state is written) or the fused call
static int run(float* a, float* b, const float* v, const float* h, const float* g, float* out, int64_t N, float step, float tiny,
               void* ws, hipStream_t st) {
  const bool upd = v != nullptr, app = g != nullptr, diag = b == nullptr;
  bool vec = N % 4 == 0 && aligned16(a) && aligned16(b);
  if (upd) vec = vec && aligned16(v) && aligned16(h);
  if (app) vec = vec && aligned16(g) && aligned16(out);
  const bool nt = app && N >= kNtMinN;
  float* partial = static_cast<float*>(ws);
  const unsigned g1 = grid_of(N, kReadGrid), g2 = grid_of(N, kWriteGrid);
  with_flags(vec, diag, nt, [&](auto V, auto D, auto T) {
    constexpr bool kV = decltype(V)::value, kD = decltype(D)::value, kN = decltype(T)::value;
    if (upd) hipLaunchKernelGGL((k_nabla_max<kV, kD>), dim3(g1), dim3(kT), 0, st, a, b, v, h, partial, N);
    if (upd && app)
      hipLaunchKernelGGL((k_rewrite<kV, kD, true, true, kN>), dim3(g2), dim3(kT), 0, st, a, b, v, h, g, out, partial, (int)g1, N, step, tiny);
    else if (upd)
      hipLaunchKernelGGL((k_rewrite<kV, kD, true, false, false>), dim3(g2), dim3(kT), 0, st, a, b, v, h, g, out, partial, (int)g1, N, step, tiny);
    else
      hipLaunchKernelGGL((k_rewrite<kV, kD, false, true, kN>), dim3(g2), dim3(kT), 0, st, a, b, v, h, g, out, partial, 0, N, step, tiny);
  });
  return launched();
}

}  // namespace psgdx

using namespace psgdx;

extern "C" {

int64_t psgd_xmat_workspace_bytes(int64_t N) {
  if (N <= 0) return PSGD_ERR_BAD_ARG;
  return (int64_t)kReadGrid * (int64_t)sizeof(float);
}

int psgd_xmat_apply_f32(const float* a, const float* b, const float* g, float* out, int64_t N, void* stream) {
  if (!a || !g || !out || N <= 0 || out == a || out == b || out == g) return PSGD_ERR_BAD_ARG;
  return run(const_cast<float*>(a), const_cast<float*>(b), nullptr, nullptr, g, out, N, 0.f, 0.f, nullptr,
             static_cast<hipStream_t>(stream));
}

int psgd_xmat_update_f32(float* a, float* b, const float* v, const float* h, int64_t N, float step, float tiny, void* ws,
                         int64_t ws_bytes, void* stream) {
  if (!a || !v || !h || N <= 0 || a == b || v == a || v == b || h == a || h == b) return PSGD_ERR_BAD_ARG;
  if (ws_check(ws, ws_bytes)) return PSGD_ERR_WORKSPACE;
  return run(a, b, v, h, nullptr, nullptr, N, step, tiny, ws, static_cast<hipStream_t>(stream));
}

int psgd_xmat_update_apply_f32(float* a, float* b, const float* v, const float* h, const float* g, float* out, int64_t N,
                               float step, float tiny, void* ws, int64_t ws_bytes, void* stream) {
  if (!a || !v || !h || !g || !out || N <= 0 || a == b || v == a || v == b || h == a || h == b || g == a || g == b)
    return PSGD_ERR_BAD_ARG;
  if (out == a || out == b || out == v || out == h || out == g) return PSGD_ERR_BAD_ARG;
  if (ws_check(ws, ws_bytes)) return PSGD_ERR_WORKSPACE;
  return run(a, b, v, h, g, out, N, step, tiny, ws, static_cast<hipStream_t>(stream));
}

}  // extern "C"
