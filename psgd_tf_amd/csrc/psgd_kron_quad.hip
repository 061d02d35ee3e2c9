// psgd_kron_quad.hip -- the inverse-free Kronecker whitening update (QUAD) and its apply on FULL symmetric factors, gfx950.
//
// The math is in include/psgd_kron_quad_hip.h.  Nothing here is shared with the triangular Kronecker kernels: those never read
// below the diagonal, and every product here has a full operand on both sides.  The product core (product(): one 64 x 64 tile of
// C = op(A) op(B) on v_mfma_f32_16x16x4_f32 through double-buffered LDS) and the bodies of the per-side stages are in
// kron_quad_core.h, which psgd_kron_qdiag.hip (one factor diagonal) includes too.
//
// Update = 6 launches, the host reads nothing:
//   1  W  = Ql G                                                             2 M M N flops
//   2  A  = W Qr                                                             2 M N N
//   3  Tl = A A', Tr = A' A in ONE grid over the upper tiles of both; a tile goes through LDS, is stored and (off the diagonal)
//      mirrored with coalesced rows, and leaves max|tile| and fp64 column sums of squares (row sums for the mirror) as
//      partials, so T is not read again for them                             M M N + M N N
//   4  one workgroup per side: folds the partials (s, j), runs the two fp64 matvecs on T (read by columns: T is stored
//      exactly symmetric), writes the new L in place and c to the workspace   4 (M M + N N)
//   5  P1 = Q - c (T Q - t2 Q), both sides in one grid                        2 (M^3 + N^3)
//   6  P2 = P1 - c (P1 T - t2 P1) and Q <- (P2 + P2') / 2, both sides in one grid over the upper tiles: one workgroup forms
//      tile (i, j) AND tile (j, i), transposes the second through LDS, averages, and writes both -- Q[i,j] and Q[j,i] are one
//      value written twice; Q is read only by launch 5 and written only here   2 (M^3 + N^3)
// Apply = 4 chained products through two M x N workspace buffers, the shorter side's two products first.
//
// Determinism: no atomics; every partial has exactly one writer and every fold a fixed order.
#include <hip/hip_runtime.h>
#include "kron_quad_core.h"

namespace psgdq {

// --------------------------------------------------------------------------------------------------------------- kernels
// C (M x N, row-major) = a b', one workgroup per tile
__global__ __launch_bounds__(kT) void k_product(Opnd a, Opnd b, int K, float* __restrict__ C, int M, int N, int tiles_n) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const int m0 = (blockIdx.x / tiles_n) * kTile, n0 = (blockIdx.x % tiles_n) * kTile;
  f32x4 acc[2][2];
  product(a, b, K, m0, n0, lds, acc);
  each_elem([&](int i, int j, int e, int r, int c) {
    if (m0 + r < M && n0 + c < N) C[(long)(m0 + r) * N + (n0 + c)] = acc[i][j][e];
  });
}

// Tl and Tr, upper tiles only, mirrored on write; per-tile max|T| and column sum-of-squares partials
__global__ __launch_bounds__(kT) void k_gram(GramSide sl, GramSide sr, int upper_l) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  __shared__ float red[kT / 64];
  const bool right = (int)blockIdx.x >= upper_l;
  const GramSide& s = right ? sr : sl;
  int ti, tj;
  upper_tile(right ? blockIdx.x - upper_l : blockIdx.x, s.nb, ti, tj);
  f32x4 acc[2][2];
  product(s.o, s.o, s.K, ti * kTile, tj * kTile, lds, acc);
  gram_epilogue(s, ti, tj, acc, lds, red);
}

// one workgroup per side: s, j, the two matvecs, L (in place) and c = step / (2 L) to coef[side]
__global__ __launch_bounds__(kLipT) void k_lipschitz(LipSide sl, LipSide sr, float* L, float* coef, float step, float decay) {
  __shared__ double red[kLipT];
  __shared__ int redi[kLipT];
  __shared__ float redf[kLipT / 64];
  lipschitz_dense(blockIdx.x ? sr : sl, L + blockIdx.x, coef + blockIdx.x, step, decay, red, redi, redf);
}

// P1 = Q - c (T Q - t2 Q), every tile of both sides
__global__ __launch_bounds__(kT) void k_p1(StepSide sl, StepSide sr, const float* __restrict__ coef, int tiles_l) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const bool right = (int)blockIdx.x >= tiles_l;
  p1_tile(right ? sr : sl, right ? blockIdx.x - tiles_l : blockIdx.x, coef[right ? 1 : 0], lds);
}

// Q <- (P2 + P2') / 2, both sides in one grid over the upper tiles
__global__ __launch_bounds__(kT) void k_p2_sym(StepSide sl, StepSide sr, const float* __restrict__ coef, int upper_l) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const bool right = (int)blockIdx.x >= upper_l;
  p2_sym_tiles(right ? sr : sl, right ? blockIdx.x - upper_l : blockIdx.x, coef[right ? 1 : 0], lds);
}

// --------------------------------------------------------------------------------------------------------------- the host
struct Ws {
  float *W, *A, *T[2], *P1[2], *tmax[2], *coef;
  double *part[2], *vec[2];
  int64_t bytes;
};
static Ws carve(void* base, int M, int N) {
  Ws w;
  char* p = static_cast<char*>(base);
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* q = p + off;
    off += up256(bytes);
    return q;
  };
  const int64_t mn = (int64_t)M * N, dim[2] = {M, N};
  w.W = reinterpret_cast<float*>(take(mn * 4));
  w.A = reinterpret_cast<float*>(take(mn * 4));
  for (int s = 0; s < 2; ++s) {
    const int64_t n = dim[s], nb = tiles_of((int)n);
    w.T[s] = reinterpret_cast<float*>(take(n * n * 4));
    w.P1[s] = reinterpret_cast<float*>(take(n * n * 4));
    w.tmax[s] = reinterpret_cast<float*>(take(nb * nb * 4));
    w.part[s] = reinterpret_cast<double*>(take(nb * n * 8));
    w.vec[s] = reinterpret_cast<double*>(take(2 * n * 8));
  }
  w.coef = reinterpret_cast<float*>(take(2 * 4));
  w.bytes = off;
  return w;
}
static int ws_check(const void* ws, int64_t ws_bytes, int M, int N) {
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) || ws_bytes < carve(nullptr, M, N).bytes) return PSGD_ERR_WORKSPACE;
  return PSGD_OK;
}

// C (M x N) = a b' with the operands as (x, k) views
static void launch_product(Opnd a, Opnd b, int K, float* C, int M, int N, hipStream_t st) {
  const int tn = tiles_of(N);
  hipLaunchKernelGGL(k_product, dim3((unsigned)(tiles_of(M) * tn)), dim3(kT), 0, st, a, b, K, C, M, N, tn);
}
// C = Q X (Q is M x M, X is M x N) and C = X Q (Q is N x N)
static void left_product(const float* Q, const float* X, float* C, int M, int N, hipStream_t st) {
  launch_product(Opnd{Q, M, 1, M}, Opnd{X, 1, N, N}, M, C, M, N, st);
}
static void right_product(const float* X, const float* Q, float* C, int M, int N, hipStream_t st) {
  launch_product(Opnd{X, N, 1, M}, Opnd{Q, 1, N, N}, N, C, M, N, st);
}

}  // namespace psgdq

using namespace psgdq;

extern "C" {

int64_t psgd_kron_quad_workspace_bytes(int M, int N) {
  if (M < 1 || N < 1) return PSGD_ERR_BAD_ARG;
  return carve(nullptr, M, N).bytes;
}

int psgd_kron_quad_apply_f32(const float* Ql, const float* Qr, const float* G, float* out, int M, int N, void* ws, int64_t ws_bytes,
                             void* stream) {
  if (!Ql || !Qr || !G || !out || M < 1 || N < 1 || out == Ql || out == Qr || out == G) return PSGD_ERR_BAD_ARG;
  if (ws_check(ws, ws_bytes, M, N)) return PSGD_ERR_WORKSPACE;
  const Ws w = carve(ws, M, N);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (M <= N) {
    left_product(Ql, G, w.W, M, N, st);
    left_product(Ql, w.W, w.A, M, N, st);
    right_product(w.A, Qr, w.W, M, N, st);
    right_product(w.W, Qr, out, M, N, st);
  } else {
    right_product(G, Qr, w.W, M, N, st);
    right_product(w.W, Qr, w.A, M, N, st);
    left_product(Ql, w.A, w.W, M, N, st);
    left_product(Ql, w.W, out, M, N, st);
  }
  return launched();
}

int psgd_kron_quad_update_f32(float* Ql, float* Qr, float* L, const float* G, int M, int N, float step, float decay, void* ws,
                              int64_t ws_bytes, void* stream) {
  if (!Ql || !Qr || !L || !G || M < 1 || N < 1 || Ql == Qr || G == Ql || G == Qr || L == Ql || L == Qr || L == G)
    return PSGD_ERR_BAD_ARG;
  if (ws_check(ws, ws_bytes, M, N)) return PSGD_ERR_WORKSPACE;
  const Ws w = carve(ws, M, N);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nbl = tiles_of(M), nbr = tiles_of(N);
  const int ul = nbl * (nbl + 1) / 2, ur = nbr * (nbr + 1) / 2;

  left_product(Ql, G, w.W, M, N, st);
  right_product(w.W, Qr, w.A, M, N, st);

  const GramSide gl{Opnd{w.A, N, 1, M}, M, N, nbl, w.T[0], w.tmax[0], w.part[0]};
  const GramSide gr{Opnd{w.A, 1, N, N}, N, M, nbr, w.T[1], w.tmax[1], w.part[1]};
  hipLaunchKernelGGL(k_gram, dim3((unsigned)(ul + ur)), dim3(kT), 0, st, gl, gr, ul);

  const LipSide ll{M, nbl, w.T[0], w.tmax[0], w.part[0], w.vec[0], (double)N};
  const LipSide lr{N, nbr, w.T[1], w.tmax[1], w.part[1], w.vec[1], (double)M};
  hipLaunchKernelGGL(k_lipschitz, dim3(2), dim3(kLipT), 0, st, ll, lr, L, w.coef, step, decay);

  const StepSide pl{M, nbl, w.T[0], Ql, w.P1[0], (float)N};
  const StepSide pr{N, nbr, w.T[1], Qr, w.P1[1], (float)M};
  hipLaunchKernelGGL(k_p1, dim3((unsigned)(nbl * nbl + nbr * nbr)), dim3(kT), 0, st, pl, pr, w.coef, nbl * nbl);
  hipLaunchKernelGGL(k_p2_sym, dim3((unsigned)(ul + ur)), dim3(kT), 0, st, pl, pr, w.coef, ul);
  return launched();
}

}  // extern "C"