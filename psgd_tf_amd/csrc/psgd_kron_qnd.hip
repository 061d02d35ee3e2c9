// psgd_kron_qnd.hip -- the QUAD Kronecker update and its apply on ORDER-3 tensors [A, B, C] with three symmetric factors, gfx950.
//
// The math is in include/psgd_kron_quad_nd_hip.h.  The product core, the Gram epilogue, the Lipschitz body and the P1 / symmetrised
// P2 stages are the inline bodies of kron_quad_core.h, unchanged: a side of this update IS a side of the matrix update once its
// T exists.  New here are the mode products, the Gram over the middle mode, and the grids over three sides.
//
// Mode products.  X is row-major [A, B, C].  Mode 1 is product() on the [A, BC] view (Qa from the left), mode 3 product() on
// the [AB, C] view (Qc from the right); neither moves a byte.  Mode 2 is Y[a] = Qb X[a] for every slab a: ONE launch of
// A ceil(B/64) ceil(C/64) workgroups, each of which decodes (slab, tile row, tile column) from blockIdx and builds its Opnd
// views on the slab's base X + a BC.  One kernel, k_mode, serves the three: modes 1 and 3 are its one-slab case.
//
// Gram over the middle mode.  T_b[b, b'] = sum_{a, c} X[a, b, c] X[a, b', c]: the summed index is the PAIR (a, c), at address
// a BC + c, which no (xs, ks) pair of an Opnd expresses, and a transposed copy of X would cost 8 A B C bytes of traffic and
// 4 A B C bytes of workspace more.  SegOpnd (kron_quad_seg.h) is the operand with a SEGMENTED K: k -> (k / C) BC + (k % C), K = A C, a outer and
// c inner, so the order of the sum is that of the addresses.  Its fetch is the k-contiguous half of g2r(): thread t owns x = t & 63 and four consecutive k
// from (t >> 6) 4; one integer division per thread and step gives (a, c) of the first, the other three follow by increment and
// wrap.  When C % 4 == 0 and the base is 16-byte aligned, four consecutive k that start at a multiple of 4 lie in one segment
// at a 16-byte aligned address: one 16-byte load, as for a plain operand.  Otherwise four dword loads from checked addresses --
// and these may straddle a slab boundary, as a whole K step of 16 may: C = 9 packs 16 k into every step (1.8 segments), it
// does not pad each slab to 16.  The LDS image, the MFMA loop (product_of() of the core: product() with the fetch as a type)
// and gram_epilogue() are those of every other Gram here.  T_a uses the plain view (x stride BC, k contiguous, K = BC), T_c
// the plain view (x contiguous, k stride C, K = AB).
//
// Update = 7 launches, the host reads nothing:
//   1-3  X = G x1 Qa x2 Qb x3 Qc through two workspace tensors                 2 A B C (A + B + C) flops
//   4    T_a, T_b, T_c in ONE grid over the upper tiles of the three            A B C (A + B + C)
//   5    three workgroups: s, j, the two fp64 matvecs, L in place, c           4 (A^2 + B^2 + C^2)
//   6    P1 of the three sides in one grid over all their tiles                2 (A^3 + B^3 + C^3)
//   7    P2 and Q <- (P2 + P2') / 2 of the three sides, upper tiles            2 (A^3 + B^3 + C^3)
// Apply = 6 mode products, the modes in ascending extent (ties: the lower mode first), each factor twice back to back.
//
// Determinism: no atomics; every output element and every partial has one writer, every fold a fixed order.
#include <hip/hip_runtime.h>
#include "kron_quad_core.h"
#include "kron_quad_seg.h"
#include "psgd_kron_quad_nd_hip.h"

namespace psgdqn {
using namespace psgdq;

// --------------------------------------------------------------------------------------------------------------- kernels
// one mode product: per slab s (blockIdx / tiles_slab), C_s (M x N, row-major) = a b_s', C_s and b_s at s * stride floats from
// the bases.  Modes 1 and 3 are one slab; mode 2 has A slabs of stride B C.
__global__ __launch_bounds__(kT) void k_mode(Opnd a, Opnd b, int K, float* __restrict__ C, int M, int N, int tiles_n, int tiles_slab,
                                             long stride) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const int slab = blockIdx.x / tiles_slab, tile = blockIdx.x - slab * tiles_slab;
  const int m0 = (tile / tiles_n) * kTile, n0 = (tile % tiles_n) * kTile;
  b.p += slab * stride;
  C += slab * stride;
  f32x4 acc[2][2];
  product(a, b, K, m0, n0, lds, acc);
  each_elem([&](int i, int j, int e, int r, int c) {
    if (m0 + r < M && n0 + c < N) C[(long)(m0 + r) * N + (n0 + c)] = acc[i][j][e];
  });
}

// which of three sides a workgroup belongs to, and its number inside that side: the grid is [0, e0) [e0, e1) [e1, total)
struct Split3 {
  int e0, e1;
  __device__ __forceinline__ int side(int b) const { return b < e0 ? 0 : b < e1 ? 1 : 2; }
  __device__ __forceinline__ int local(int b) const { return b < e0 ? b : b < e1 ? b - e0 : b - e1; }
};
template <class S>
__device__ __forceinline__ const S& pick(int side, const S& a, const S& b, const S& c) {
  return side == 0 ? a : side == 1 ? b : c;
}

// T_a, T_b, T_c: upper tiles only, mirrored on write; per-tile max|T| and column sum-of-squares partials.  The middle side sums
// over (a, c) through the segmented operand.
__global__ __launch_bounds__(kT) void k_gram3(GramSide sa, GramSide sb, GramSide sc, SegOpnd mid, Split3 sp) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  __shared__ float red[kT / 64];
  const int side = sp.side(blockIdx.x);
  const GramSide& s = pick(side, sa, sb, sc);
  int ti, tj;
  upper_tile(sp.local(blockIdx.x), s.nb, ti, tj);
  f32x4 acc[2][2];
  if (side == 1)
    product_of(mid, mid, s.K, ti * kTile, tj * kTile, lds, acc);
  else
    product(s.o, s.o, s.K, ti * kTile, tj * kTile, lds, acc);
  gram_epilogue(s, ti, tj, acc, lds, red);
}

// one workgroup per side: s, j, the two matvecs, L (in place) and c = step / (2 L) to coef[side]
__global__ __launch_bounds__(kLipT) void k_lip3(LipSide sa, LipSide sb, LipSide sc, float* L, float* coef, float step, float decay) {
  __shared__ double red[kLipT];
  __shared__ int redi[kLipT];
  __shared__ float redf[kLipT / 64];
  lipschitz_dense(pick((int)blockIdx.x, sa, sb, sc), L + blockIdx.x, coef + blockIdx.x, step, decay, red, redi, redf);
}

// P1 = Q - c (T Q - t2 Q), every tile of the three sides
__global__ __launch_bounds__(kT) void k_p1_3(StepSide sa, StepSide sb, StepSide sc, const float* __restrict__ coef, Split3 sp) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const int side = sp.side(blockIdx.x);
  p1_tile(pick(side, sa, sb, sc), sp.local(blockIdx.x), coef[side], lds);
}

// Q <- (P2 + P2') / 2, the three sides in one grid over their upper tiles.  The pieces of p2_sym_tiles() with the diagonal case
// branched around the second product: the same arithmetic, and no accumulator parked in scratch between the two products
// (a diagonal tile does not read `lo`, so `up` stands in for it)
__global__ __launch_bounds__(kT) void k_p2_sym3(StepSide sa, StepSide sb, StepSide sc, const float* __restrict__ coef, Split3 sp) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const int side = sp.side(blockIdx.x);
  const StepSide& s = pick(side, sa, sb, sc);
  const float c1 = coef[side];
  int ti, tj;
  upper_tile(sp.local(blockIdx.x), s.nb, ti, tj);
  const int m0 = ti * kTile, n0 = tj * kTile;
  f32x4 up[2][2];
  p2_tile(s, c1, m0, n0, lds, up);
  if (ti == tj) {
    p2_sym_store(s, m0, n0, true, up, up, lds);
  } else {
    f32x4 lo[2][2];
    p2_tile(s, c1, n0, m0, lds, lo);
    p2_sym_store(s, m0, n0, false, up, lo, lds);
  }
}

// --------------------------------------------------------------------------------------------------------------- the host
struct Ws {
  float *X[2], *T[3], *P1[3], *tmax[3], *coef;
  double *part[3], *vec[3];
  int64_t bytes;
};
static Ws carve(void* base, int A, int B, int C) {
  Ws w;
  char* p = static_cast<char*>(base);
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* q = p + off;
    off += up256(bytes);
    return q;
  };
  const int64_t numel = (int64_t)A * B * C, dim[3] = {A, B, C};
  for (int i = 0; i < 2; ++i) w.X[i] = reinterpret_cast<float*>(take(numel * 4));
  for (int s = 0; s < 3; ++s) {
    const int64_t n = dim[s], nb = tiles_of((int)n);
    w.T[s] = reinterpret_cast<float*>(take(n * n * 4));
    w.P1[s] = reinterpret_cast<float*>(take(n * n * 4));
    w.tmax[s] = reinterpret_cast<float*>(take(nb * nb * 4));
    w.part[s] = reinterpret_cast<double*>(take(nb * n * 8));
    w.vec[s] = reinterpret_cast<double*>(take(2 * n * 8));
  }
  w.coef = reinterpret_cast<float*>(take(3 * 4));
  w.bytes = off;
  return w;
}
static bool shape_ok(int A, int B, int C) { return A >= 1 && B >= 1 && C >= 1 && (int64_t)A * B * C <= INT32_MAX; }
static int ws_check(const void* ws, int64_t ws_bytes, int A, int B, int C) {
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) || ws_bytes < carve(nullptr, A, B, C).bytes) return PSGD_ERR_WORKSPACE;
  return PSGD_OK;
}

// dst = src x_mode Q, src and dst distinct tensors [A, B, C]
static void mode_product(int mode, const float* Q, const float* src, float* dst, int A, int B, int C, hipStream_t st) {
  const int AB = A * B, BC = B * C;
  Opnd a, b;
  int K, M, N, slabs = 1;
  if (mode == 0) {                                      // [A, BC] view: Qa from the left
    a = Opnd{Q, A, 1, A}, b = Opnd{src, 1, BC, BC}, K = A, M = A, N = BC;
  } else if (mode == 1) {                               // per slab [B, C]: Qb from the left
    a = Opnd{Q, B, 1, B}, b = Opnd{src, 1, C, C}, K = B, M = B, N = C, slabs = A;
  } else {                                              // [AB, C] view: Qc from the right
    a = Opnd{src, C, 1, AB}, b = Opnd{Q, 1, C, C}, K = C, M = AB, N = C;
  }
  const int tn = tiles_of(N), per = tiles_of(M) * tn;
  // (one slab: the slab offset is 0 whatever the stride; mode 3 keeps src in `a`, which k_mode never offsets)
  hipLaunchKernelGGL(k_mode, dim3((unsigned)((int64_t)slabs * per)), dim3(kT), 0, st, a, b, K, dst, M, N, tn, per, (long)BC);
}

}  // namespace psgdqn

using namespace psgdqn;

extern "C" {

int64_t psgd_kron_qnd_workspace_bytes(int A, int B, int C) {
  if (!shape_ok(A, B, C)) return PSGD_ERR_BAD_ARG;
  return carve(nullptr, A, B, C).bytes;
}

int psgd_kron_qnd_apply_f32(const float* Qa, const float* Qb, const float* Qc, const float* G, float* out, int A, int B, int C,
                            void* ws, int64_t ws_bytes, void* stream) {
  if (!Qa || !Qb || !Qc || !G || !out || !shape_ok(A, B, C) || out == Qa || out == Qb || out == Qc || out == G) return PSGD_ERR_BAD_ARG;
  if (ws_check(ws, ws_bytes, A, B, C)) return PSGD_ERR_WORKSPACE;
  const Ws w = carve(ws, A, B, C);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* Q[3] = {Qa, Qb, Qc};
  const int dim[3] = {A, B, C};
  int order[3] = {0, 1, 2};                             // ascending extent, stable: a function of the shape alone
  for (int i = 1; i < 3; ++i)
    for (int j = i; j > 0 && dim[order[j]] < dim[order[j - 1]]; --j) {
      const int tmp = order[j];
      order[j] = order[j - 1];
      order[j - 1] = tmp;
    }
  const float* src = G;
  for (int i = 0; i < 6; ++i) {
    float* dst = i == 5 ? out : w.X[i & 1];
    mode_product(order[i / 2], Q[order[i / 2]], src, dst, A, B, C, st);
    src = dst;
  }
  return launched();
}

int psgd_kron_qnd_update_f32(float* Qa, float* Qb, float* Qc, float* L, const float* G, int A, int B, int C, float step, float decay,
                             void* ws, int64_t ws_bytes, void* stream) {
  if (!Qa || !Qb || !Qc || !L || !G || !shape_ok(A, B, C) || Qa == Qb || Qa == Qc || Qb == Qc || G == Qa || G == Qb || G == Qc ||
      L == Qa || L == Qb || L == Qc || L == G)
    return PSGD_ERR_BAD_ARG;
  if (ws_check(ws, ws_bytes, A, B, C)) return PSGD_ERR_WORKSPACE;
  const Ws w = carve(ws, A, B, C);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int AB = A * B, BC = B * C, AC = A * C;
  const int nba = tiles_of(A), nbb = tiles_of(B), nbc = tiles_of(C);
  const int ua = nba * (nba + 1) / 2, ub = nbb * (nbb + 1) / 2, uc = nbc * (nbc + 1) / 2;

  mode_product(0, Qa, G, w.X[0], A, B, C, st);
  mode_product(1, Qb, w.X[0], w.X[1], A, B, C, st);
  mode_product(2, Qc, w.X[1], w.X[0], A, B, C, st);
  const float* X = w.X[0];

  const GramSide ga{Opnd{X, BC, 1, A}, A, BC, nba, w.T[0], w.tmax[0], w.part[0]};
  const GramSide gb{Opnd{nullptr, 0, 0, 0}, B, AC, nbb, w.T[1], w.tmax[1], w.part[1]};   // (its operand is `mid`)
  const GramSide gc{Opnd{X, 1, C, C}, C, AB, nbc, w.T[2], w.tmax[2], w.part[2]};
  const SegOpnd mid{X, (long)BC, C, B};
  hipLaunchKernelGGL(k_gram3, dim3((unsigned)(ua + ub + uc)), dim3(kT), 0, st, ga, gb, gc, mid, Split3{ua, ua + ub});

  const LipSide la{A, nba, w.T[0], w.tmax[0], w.part[0], w.vec[0], (double)BC};
  const LipSide lb{B, nbb, w.T[1], w.tmax[1], w.part[1], w.vec[1], (double)AC};
  const LipSide lc{C, nbc, w.T[2], w.tmax[2], w.part[2], w.vec[2], (double)AB};
  hipLaunchKernelGGL(k_lip3, dim3(3), dim3(kLipT), 0, st, la, lb, lc, L, w.coef, step, decay);

  const StepSide pa{A, nba, w.T[0], Qa, w.P1[0], (float)BC};
  const StepSide pb{B, nbb, w.T[1], Qb, w.P1[1], (float)AC};
  const StepSide pc{C, nbc, w.T[2], Qc, w.P1[2], (float)AB};
  const int ta = nba * nba, tb = nbb * nbb;
  hipLaunchKernelGGL(k_p1_3, dim3((unsigned)(ta + tb + nbc * nbc)), dim3(kT), 0, st, pa, pb, pc, w.coef, Split3{ta, ta + tb});
  hipLaunchKernelGGL(k_p2_sym3, dim3((unsigned)(ua + ub + uc)), dim3(kT), 0, st, pa, pb, pc, w.coef, Split3{ua, ua + ub});
  return launched();
}

}  // extern "C"
