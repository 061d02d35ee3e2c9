// psgd_kron_quad_x3.hip -- the QUAD update and its apply (include/psgd_kron_quad_hip.h) with every product on the bf16 matrix
// cores at fp32 grade: the "bf16 x 3" core of kron_quad_x3_core.h on 128 x 128 macro tiles.  C ABI: psgd_kron_quad_x3_hip.h.
//
// The math, the workspace layout and the launch structure are those of psgd_kron_quad.hip: 6 launches per update, 4 per apply,
// the host reads nothing.  What differs is the product core and the grid: a workgroup owns a macro tile, i.e. 2 x 2 of the
// 64-tiles, and runs the 64-tile epilogues of kron_quad_core.h once per sub-tile, so tmax, the fp64 column-sumsq partials
// part[nb][n] and the Lipschitz launch (lipschitz_dense, the same code) keep their 64-tile indexing:
//   1  W  = Ql G                                  every macro tile
//   2  A  = W Qr
//   3  Tl = A A', Tr = A' A in ONE grid over the upper MACRO tiles of both.  Off the diagonal all four sub-tiles are upper
//      64-tiles; in a diagonal macro tile the sub-tile (1, 0) is the mirror of (0, 1), which stores it: it is skipped, and every
//      element of T, tmax and part keeps one writer
//   4  the Lipschitz launch of the fp32 route
//   5  P1 = Q - c (T Q - t2 Q), every macro tile of both sides in one grid
//   6  P2 and Q <- (P2 + P2') / 2, both sides in one grid over the upper macro tiles: one workgroup forms the macro tile (I, J)
//      AND (J, I) (on the diagonal: once), and pairs sub-tile (si, sj) of the first with (sj, si) of the second through LDS --
//      Q[i,j] and Q[j,i] are one value written twice
// Determinism: no atomics; every partial has exactly one writer and every fold a fixed order.
#include <hip/hip_runtime.h>
#include "kron_quad_x3_core.h"
#include "psgd_kron_quad_x3_hip.h"

namespace psgdq {

// f(si, sj) for the sub-tiles of the macro tile (m0, n0) that reach into an m x n matrix, a barrier between two of them (the
// 64-tile epilogues end without one)
template <class F>
__device__ __forceinline__ void each_sub(int m0, int n0, int m, int n, F&& f) {
#pragma unroll
  for (int si = 0; si < 2; ++si)
#pragma unroll
    for (int sj = 0; sj < 2; ++sj)
      if (m0 + si * kTile < m && n0 + sj * kTile < n) {   // uniform
        f(si, sj);
        __syncthreads();
      }
}

// --------------------------------------------------------------------------------------------------------------- kernels
// C (M x N, row-major) = a b', one workgroup per macro tile
__global__ __launch_bounds__(kT) void k_x3_product(Opnd a, Opnd b, int K, float* __restrict__ C, int M, int N, int tiles_n) {
  __shared__ __attribute__((aligned(16))) X3Lds L;
  const int m0 = (blockIdx.x / tiles_n) * kMac, n0 = (blockIdx.x % tiles_n) * kMac;
  f32x4 acc[2][2][2][2];
  product_x3(a, b, K, m0, n0, L, acc);
#pragma unroll
  for (int si = 0; si < 2; ++si)
#pragma unroll
    for (int sj = 0; sj < 2; ++sj) {
      const int r0 = m0 + si * kTile, c0 = n0 + sj * kTile;
      each_elem([&](int i, int j, int e, int r, int c) {
        if (r0 + r < M && c0 + c < N) C[(long)(r0 + r) * N + (c0 + c)] = acc[si][sj][i][j][e];
      });
    }
}

// Tl and Tr, upper macro tiles only
__global__ __launch_bounds__(kT) void k_x3_gram(GramSide sl, GramSide sr, int upper_l) {
  __shared__ __attribute__((aligned(16))) X3Lds L;
  __shared__ float red[kT / 64];
  const bool right = (int)blockIdx.x >= upper_l;
  const GramSide& s = right ? sr : sl;
  int I, J;
  upper_tile(right ? blockIdx.x - upper_l : blockIdx.x, macro_tiles_of(s.n), I, J);
  f32x4 acc[2][2][2][2];
  product_x3(s.o, s.o, s.K, I * kMac, J * kMac, L, acc);
  float* lds = reinterpret_cast<float*>(&L);
  each_sub(I * kMac, J * kMac, s.n, s.n, [&](int si, int sj) {
    if (I != J || si <= sj) gram_epilogue(s, 2 * I + si, 2 * J + sj, acc[si][sj], lds, red);
  });
}

__global__ __launch_bounds__(kLipT) void k_x3_lipschitz(LipSide sl, LipSide sr, float* L, float* coef, float step, float decay) {
  __shared__ double red[kLipT];
  __shared__ int redi[kLipT];
  __shared__ float redf[kLipT / 64];
  lipschitz_dense(blockIdx.x ? sr : sl, L + blockIdx.x, coef + blockIdx.x, step, decay, red, redi, redf);
}

// P1 = Q - c (T Q - t2 Q), every macro tile of both sides
__global__ __launch_bounds__(kT) void k_x3_p1(StepSide sl, StepSide sr, const float* __restrict__ coef, int tiles_l) {
  __shared__ __attribute__((aligned(16))) X3Lds L;
  const bool right = (int)blockIdx.x >= tiles_l;
  const StepSide& s = right ? sr : sl;
  const int b = right ? blockIdx.x - tiles_l : blockIdx.x, nm = macro_tiles_of(s.n), n = s.n;
  const int m0 = (b / nm) * kMac, n0 = (b % nm) * kMac;
  const float c1 = coef[right ? 1 : 0];
  f32x4 acc[2][2][2][2];
  product_x3(Opnd{s.T, n, 1, n}, Opnd{s.Q, 1, n, n}, n, m0, n0, L, acc);
#pragma unroll
  for (int si = 0; si < 2; ++si)
#pragma unroll
    for (int sj = 0; sj < 2; ++sj) p1_store(s, c1, m0 + si * kTile, n0 + sj * kTile, acc[si][sj]);
}

// the macro tile (m0, n0) of P2 = P1 - c (P1 T - t2 P1), zero outside the matrix
__device__ __forceinline__ void p2_macro(const StepSide& s, float c1, int m0, int n0, X3Lds& L, f32x4 (&acc)[2][2][2][2]) {
  const int n = s.n;
  product_x3(Opnd{s.P1, n, 1, n}, Opnd{s.T, 1, n, n}, n, m0, n0, L, acc);
#pragma unroll
  for (int si = 0; si < 2; ++si)
#pragma unroll
    for (int sj = 0; sj < 2; ++sj) p2_finish(s, c1, m0 + si * kTile, n0 + sj * kTile, acc[si][sj]);
}

// Q <- (P2 + P2') / 2, both sides in one grid over the upper macro tiles
__global__ __launch_bounds__(kT) void k_x3_p2_sym(StepSide sl, StepSide sr, const float* __restrict__ coef, int upper_l) {
  __shared__ __attribute__((aligned(16))) X3Lds L;
  const bool right = (int)blockIdx.x >= upper_l;
  const StepSide& s = right ? sr : sl;
  const float c1 = coef[right ? 1 : 0];
  int I, J;
  upper_tile(right ? blockIdx.x - upper_l : blockIdx.x, macro_tiles_of(s.n), I, J);
  const int m0 = I * kMac, n0 = J * kMac;
  f32x4 up[2][2][2][2], lo[2][2][2][2];
  p2_macro(s, c1, m0, n0, L, up);
  float* lds = reinterpret_cast<float*>(&L);
  if (I != J) {
    p2_macro(s, c1, n0, m0, L, lo);
    each_sub(m0, n0, s.n, s.n, [&](int si, int sj) {
      p2_sym_store(s, m0 + si * kTile, n0 + sj * kTile, false, up[si][sj], lo[sj][si], lds);
    });
  } else {                                              // the macro tile is its own mirror; (1, 0) is written by (0, 1)
    each_sub(m0, n0, s.n, s.n, [&](int si, int sj) {
      if (si == sj) p2_sym_store(s, m0 + si * kTile, n0 + sj * kTile, true, up[si][sj], up[si][sj], lds);
      else if (si < sj) p2_sym_store(s, m0 + si * kTile, n0 + sj * kTile, false, up[si][sj], up[sj][si], lds);
    });
  }
}

// --------------------------------------------------------------------------------------------------------------- the host
// the workspace of psgd_kron_quad.hip, region for region
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

static void launch_product(Opnd a, Opnd b, int K, float* C, int M, int N, hipStream_t st) {
  const int tn = macro_tiles_of(N);
  hipLaunchKernelGGL(k_x3_product, dim3((unsigned)(macro_tiles_of(M) * tn)), dim3(kT), 0, st, a, b, K, C, M, N, tn);
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

int64_t psgd_kron_quad_x3_workspace_bytes(int M, int N) {
  if (M < 1 || N < 1) return PSGD_ERR_BAD_ARG;
  return carve(nullptr, M, N).bytes;
}

int psgd_kron_quad_x3_apply_f32(const float* Ql, const float* Qr, const float* G, float* out, int M, int N, void* ws,
                                int64_t ws_bytes, void* stream) {
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

int psgd_kron_quad_x3_update_f32(float* Ql, float* Qr, float* L, const float* G, int M, int N, float step, float decay, void* ws,
                                 int64_t ws_bytes, void* stream) {
  if (!Ql || !Qr || !L || !G || M < 1 || N < 1 || Ql == Qr || G == Ql || G == Qr || L == Ql || L == Qr || L == G)
    return PSGD_ERR_BAD_ARG;
  if (ws_check(ws, ws_bytes, M, N)) return PSGD_ERR_WORKSPACE;
  const Ws w = carve(ws, M, N);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nbl = tiles_of(M), nbr = tiles_of(N), nml = macro_tiles_of(M), nmr = macro_tiles_of(N);
  const int ul = nml * (nml + 1) / 2, ur = nmr * (nmr + 1) / 2;

  left_product(Ql, G, w.W, M, N, st);
  right_product(w.W, Qr, w.A, M, N, st);

  const GramSide gl{Opnd{w.A, N, 1, M}, M, N, nbl, w.T[0], w.tmax[0], w.part[0]};
  const GramSide gr{Opnd{w.A, 1, N, N}, N, M, nbr, w.T[1], w.tmax[1], w.part[1]};
  hipLaunchKernelGGL(k_x3_gram, dim3((unsigned)(ul + ur)), dim3(kT), 0, st, gl, gr, ul);

  const LipSide ll{M, nbl, w.T[0], w.tmax[0], w.part[0], w.vec[0], (double)N};
  const LipSide lr{N, nbr, w.T[1], w.tmax[1], w.part[1], w.vec[1], (double)M};
  hipLaunchKernelGGL(k_x3_lipschitz, dim3(2), dim3(kLipT), 0, st, ll, lr, L, w.coef, step, decay);

  const StepSide pl{M, nbl, w.T[0], Ql, w.P1[0], (float)N};
  const StepSide pr{N, nbr, w.T[1], Qr, w.P1[1], (float)M};
  hipLaunchKernelGGL(k_x3_p1, dim3((unsigned)(nml * nml + nmr * nmr)), dim3(kT), 0, st, pl, pr, w.coef, nml * nml);
  hipLaunchKernelGGL(k_x3_p2_sym, dim3((unsigned)(ul + ur)), dim3(kT), 0, st, pl, pr, w.coef, ul);
  return launched();
}

}  // extern "C"
