// psgd_kron_qdiag.hip -- the QUAD Kronecker update and its apply with ONE DIAGONAL side (embedding-scale layers), gfx950.
//
// The math is in include/psgd_kron_quad_diag_hip.h.  One factor is diag(q), q of length D (the long extent); the other is a full
// symmetric Q, n x n.  The product core and the stages of the dense side are those of kron_quad_core.h; one kernel set serves
// both orientations through the strided operand views, the vector applied along rows or along columns in the epilogue.
//
// Update = 6 launches, the host reads nothing:
//   1  k_sprod   A = diag(q) (G Q) or (Q G) diag(q), one 64 x 64 tile per workgroup; the epilogue scales, writes A, parks the
//                tile in LDS and leaves one fp64 sum of squares per tile row (column) -- over the tile's columns (rows) INSIDE
//                the matrix only, so an Inf in one row cannot turn a neighbour's sum into NaN through the zero padding --
//                in part[tile index along n][D]                                                  2 D n n flops
//   2  k_gram_split   T = A'A (A A') over the long extent: (upper tiles of T) x S workgroups, slice s of psgd_kron_qdiag_slices
//                sums its own K range and writes its 64 x 64 fp32 partial in the accumulator layout (16-byte stores, coalesced);
//                with S = 1 the workgroup finishes the tile itself through the parent's epilogue   D n n
//   3  k_fold    one workgroup per upper tile adds the S partials in slice order in fp64, rounds once and runs the parent's Gram
//                epilogue (tile and mirror, max|T|, fp64 column sums of squares); further workgroups of the same grid fold
//                part over the tiles of n into t[D] (fp64, rounded once) and leave one NaN-propagating maximum per 256 entries
//   4  k_lip     two workgroups: the parent's Lipschitz body on the dense side; the fold of the block maxima, L and c on the
//                diagonal side
//   5  k_p1      P1 = Q - c (T Q - t2 Q) on the dense side; further workgroups rewrite q <- q gain^2       2 n^3
//   6  k_p2      P2 and Q <- (P2 + P2') / 2 on the dense side                                             2 n^3
// Apply = 2 launches of k_sprod: W = G Q (no scale), out = diag(q o q) (W Q).
//
// A goes through HBM (4 D n bytes written, read once per tile row of T by launch 2): the Gram of launch 2 needs a whole row of A
// (all n columns) per output tile pair, launch 1 produces A by 64-column tiles, and holding n columns of a 64-row slab in LDS
// would cap n at 512; the round trip is 2 x 4 D n bytes against 3 D n^2 flops, under 1 % of the update's time at n = 1024.
//
// Determinism: no atomics; every partial has exactly one writer and every fold a fixed order; S depends on (D, n) alone.
#include <hip/hip_runtime.h>
#include "psgd_kron_quad_diag_hip.h"
#include "kron_quad_core.h"

#ifndef PSGD_QDIAG_SLICE_TARGET            /* build experiments only (tools/kron_quad_diag_timing.py's A/B) */
#define PSGD_QDIAG_SLICE_TARGET PSGD_KRON_QDIAG_SLICE_TARGET
#endif

namespace psgdqd {
using namespace psgdq;

constexpr int kTileElems = kTile * kTile;

// --------------------------------------------------------------------------------------------------------------- kernels
struct Scale {
  const float* q;   // the vector; null: C = a b' as it is
  int rows;         // 1: q[m] scales row m of C; 0: q[n] scales column n
  int square;       // scale by q o q (formed once in fp32)
  double* part;     // null, or [tiles along the other extent][D]: sums of squares of the scaled tile rows (columns)
  long D;
};

// C (M x N, row-major) = scale o (a b'), one workgroup per tile
__global__ __launch_bounds__(kT) void k_sprod(Opnd a, Opnd b, int K, float* __restrict__ C, int M, int N, int tiles_n, Scale sc) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  __shared__ float qs[kTile];
  const int t = threadIdx.x;
  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
  const int m0 = tm * kTile, n0 = tn * kTile;
  if (sc.q && t < kTile) {                              // (product() enters with a barrier: qs is whole before the epilogue)
    const int at = (sc.rows ? m0 : n0) + t;
    const float v = at < (sc.rows ? M : N) ? sc.q[at] : 0.f;
    qs[t] = sc.square ? v * v : v;
  }
  f32x4 acc[2][2];
  product(a, b, K, m0, n0, lds, acc);
  each_elem([&](int i, int j, int e, int r, int c) {
    const float v = sc.q ? acc[i][j][e] * qs[sc.rows ? r : c] : acc[i][j][e];
    if (m0 + r < M && n0 + c < N) C[(long)(m0 + r) * N + (n0 + c)] = v;
    if (sc.part) lds[r * kSP + c] = v;
  });
  if (!sc.part) return;
  __syncthreads();
  if (t < kTile) {
    const int rows_in = min(kTile, M - m0), cols_in = min(kTile, N - n0);
    double q = 0.0;
    if (sc.rows) {                                      // row t over the tile's columns inside the matrix
      if (t < rows_in) {
        for (int c = 0; c < cols_in; ++c) {
          const double v = lds[t * kSP + c];
          q += v * v;
        }
        sc.part[(long)tn * sc.D + (m0 + t)] = q;
      }
    } else if (t < cols_in) {                           // column t over the tile's rows inside the matrix
      for (int r = 0; r < rows_in; ++r) {
        const double v = lds[r * kSP + t];
        q += v * v;
      }
      sc.part[(long)tm * sc.D + (n0 + t)] = q;
    }
  }
}

struct Split {
  int S, per;      // slices per upper tile; K steps of kGK per slice (the last slice takes what is left)
  float* gpart;    // [upper tiles][S][kTile * kTile] in the accumulator layout: element e of acc[i][j] of thread t at
};                 // ((i 2 + j) kT + t) 4 + e

// slice blockIdx.x % S of upper tile blockIdx.x / S of T
__global__ __launch_bounds__(kT) void k_gram_split(GramSide s, Split sp) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  __shared__ float red[kT / 64];
  const int u = blockIdx.x / sp.S, sl = blockIdx.x % sp.S;
  int ti, tj;
  upper_tile(u, s.nb, ti, tj);
  const int k0 = sl * sp.per * kGK, k1 = min(s.K, k0 + sp.per * kGK);
  Opnd o = s.o;                                         // (k0 is a multiple of kGK: the 16-byte route of g2r() stays aligned)
  o.p += (long)k0 * o.ks;
  f32x4 acc[2][2];
  product(o, o, k1 - k0, ti * kTile, tj * kTile, lds, acc);
  if (sp.S == 1) {
    gram_epilogue(s, ti, tj, acc, lds, red);
    return;
  }
  float* g = sp.gpart + (long)blockIdx.x * kTileElems;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) *reinterpret_cast<f32x4*>(g + ((i * 2 + j) * kT + threadIdx.x) * 4) = acc[i][j];
}

struct TFold {
  const double* part;   // [nbn][D]
  int nbn;
  long D;
  float* t;             // [D]
  float* tmaxd;         // [ceil(D / kT)]
};

// workgroups [0, upper): the S partials of an upper tile, then the Gram epilogue; the others: kT entries of t each
__global__ __launch_bounds__(kT) void k_fold(GramSide s, Split sp, int upper, TFold f) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  __shared__ float red[kT / 64];
  const int t = threadIdx.x;
  if ((int)blockIdx.x < upper) {
    int ti, tj;
    upper_tile(blockIdx.x, s.nb, ti, tj);
    double sum[2][2][4] = {};
    for (int sl = 0; sl < sp.S; ++sl) {
      const float* g = sp.gpart + ((long)blockIdx.x * sp.S + sl) * kTileElems;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(g + ((i * 2 + j) * kT + t) * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) sum[i][j][e] += (double)v[e];
        }
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][j][e] = (float)sum[i][j][e];
    gram_epilogue(s, ti, tj, acc, lds, red);
    return;
  }
  const int b = blockIdx.x - upper;
  const long at = (long)b * kT + t;
  float v = 0.f;                                        // (sums of squares: non-negative or NaN, what amaxf() orders)
  if (at < f.D) {
    double a = 0.0;
    for (int tb = 0; tb < f.nbn; ++tb) a += f.part[(long)tb * f.D + at];
    v = (float)a;
    f.t[at] = v;
  }
  for (int o = 32; o > 0; o >>= 1) v = amaxf(v, __shfl_xor(v, o, 64));
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  if (t == 0) f.tmaxd[b] = amaxf(amaxf(red[0], red[1]), amaxf(red[2], red[3]));
}

// workgroup 0: the dense side (L, c to coef[0]); workgroup 1: ell = max t + t2 of the diagonal side, its L, c to coef[1]
__global__ __launch_bounds__(kLipT) void k_lip(LipSide dense, float* L_dense, float* L_diag, float* coef, const float* tmaxd,
                                               int nblk, double t2_diag, float step, float decay) {
  __shared__ double red[kLipT];
  __shared__ int redi[kLipT];
  __shared__ float redf[kLipT / 64];
  if (blockIdx.x == 0) {
    lipschitz_dense(dense, L_dense, coef, step, decay, red, redi, redf);
    return;
  }
  const int t = threadIdx.x;
  float m = 0.f;
  for (int idx = t; idx < nblk; idx += kLipT) m = amaxf(m, tmaxd[idx]);
  for (int o = 32; o > 0; o >>= 1) m = amaxf(m, __shfl_xor(m, o, 64));
  if ((t & 63) == 0) redf[t >> 6] = m;
  __syncthreads();
  if (t == 0) {
    m = 0.f;
    for (int k = 0; k < kLipT / 64; ++k) m = amaxf(m, redf[k]);
    lipschitz_write((double)m + t2_diag, L_diag, coef + 1, step, decay);
  }
}

struct QStep {
  float* q;
  const float* t;
  float t2;
  long D;
};

// workgroups [0, tiles): P1 of the dense side; the others: q <- q gain^2, kT entries each
__global__ __launch_bounds__(kT) void k_p1(StepSide s, const float* __restrict__ coef, int tiles, QStep d) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  if ((int)blockIdx.x < tiles) {
    p1_tile(s, blockIdx.x, coef[0], lds);
    return;
  }
  const long at = (long)(blockIdx.x - tiles) * kT + threadIdx.x;
  if (at < d.D) {
    const float gain = 1.f - coef[1] * (d.t[at] - d.t2);
    d.q[at] = d.q[at] * gain * gain;
  }
}

__global__ __launch_bounds__(kT) void k_p2(StepSide s, const float* __restrict__ coef) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  p2_sym_tiles(s, blockIdx.x, coef[0], lds);
}

// --------------------------------------------------------------------------------------------------------------- the host
struct Dims {
  int D, n;        // the diagonal side's length, the dense side's
  int nb, upper;   // tiles per edge of T, upper tiles
  int S, per;      // the split of the Gram
  int nblk;        // workgroups that fold t
};
static Dims dims_of(int M, int N, int diag_side) {
  Dims d;
  d.D = diag_side ? N : M;
  d.n = diag_side ? M : N;
  d.nb = tiles_of(d.n);
  d.upper = d.nb * (d.nb + 1) / 2;
  int S0 = (PSGD_QDIAG_SLICE_TARGET + d.upper - 1) / d.upper;
  const int by_k = (d.D + PSGD_KRON_QDIAG_SLICE_MIN_K - 1) / PSGD_KRON_QDIAG_SLICE_MIN_K;
  if (S0 > by_k) S0 = by_k;
  if (S0 < 1) S0 = 1;
  const int steps = (d.D + kGK - 1) / kGK;
  d.per = (steps + S0 - 1) / S0;
  d.S = (steps + d.per - 1) / d.per;
  d.nblk = (d.D + kT - 1) / kT;
  return d;
}

struct Ws {
  float *A, *T, *P1, *tmax, *t, *tmaxd, *gpart, *coef;
  double *part, *vec, *partd;
  int64_t bytes;
};
static Ws carve(void* base, int M, int N, const Dims& d) {
  Ws w;
  char* p = static_cast<char*>(base);
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* q = p + off;
    off += up256(bytes);
    return q;
  };
  const int64_t n = d.n, D = d.D, nb = d.nb;
  w.A = reinterpret_cast<float*>(take((int64_t)M * N * 4));
  w.T = reinterpret_cast<float*>(take(n * n * 4));
  w.P1 = reinterpret_cast<float*>(take(n * n * 4));
  w.tmax = reinterpret_cast<float*>(take(nb * nb * 4));
  w.part = reinterpret_cast<double*>(take(nb * n * 8));
  w.vec = reinterpret_cast<double*>(take(2 * n * 8));
  w.partd = reinterpret_cast<double*>(take(nb * D * 8));
  w.t = reinterpret_cast<float*>(take(D * 4));
  w.tmaxd = reinterpret_cast<float*>(take((int64_t)d.nblk * 4));
  w.gpart = reinterpret_cast<float*>(take(d.S > 1 ? (int64_t)d.upper * d.S * kTileElems * 4 : 0));
  w.coef = reinterpret_cast<float*>(take(2 * 4));
  w.bytes = off;
  return w;
}
static int ws_check(const void* ws, int64_t ws_bytes, int M, int N, const Dims& d) {
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) || ws_bytes < carve(nullptr, M, N, d).bytes) return PSGD_ERR_WORKSPACE;
  return PSGD_OK;
}

// C = scale o (X Q) for diag_side 0 (Q is N x N, the vector runs along the rows), C = scale o (Q X) for 1 (Q is M x M, columns)
static void launch_sprod(const float* Q, const float* X, float* C, int M, int N, int diag_side, const float* q, int square,
                         double* part, hipStream_t st) {
  const int tn = tiles_of(N);
  const Opnd a = diag_side ? Opnd{Q, M, 1, M} : Opnd{X, N, 1, M};
  const Opnd b = diag_side ? Opnd{X, 1, N, N} : Opnd{Q, 1, N, N};
  const Scale sc{q, diag_side ? 0 : 1, square, part, diag_side ? N : M};
  hipLaunchKernelGGL(k_sprod, dim3((unsigned)(tiles_of(M) * tn)), dim3(kT), 0, st, a, b, diag_side ? M : N, C, M, N, tn, sc);
}

}  // namespace psgdqd

using namespace psgdqd;

extern "C" {

int64_t psgd_kron_qdiag_workspace_bytes(int M, int N, int diag_side) {
  if (M < 1 || N < 1 || (diag_side != 0 && diag_side != 1)) return PSGD_ERR_BAD_ARG;
  return carve(nullptr, M, N, dims_of(M, N, diag_side)).bytes;
}

int psgd_kron_qdiag_slices(int M, int N, int diag_side) {
  if (M < 1 || N < 1 || (diag_side != 0 && diag_side != 1)) return PSGD_ERR_BAD_ARG;
  return dims_of(M, N, diag_side).S;
}

int psgd_kron_qdiag_apply_f32(const float* Ql, const float* Qr, const float* G, float* out, int M, int N, int diag_side, void* ws,
                              int64_t ws_bytes, void* stream) {
  if (!Ql || !Qr || !G || !out || M < 1 || N < 1 || (diag_side != 0 && diag_side != 1) || out == Ql || out == Qr || out == G)
    return PSGD_ERR_BAD_ARG;
  const Dims d = dims_of(M, N, diag_side);
  if (ws_check(ws, ws_bytes, M, N, d)) return PSGD_ERR_WORKSPACE;
  const Ws w = carve(ws, M, N, d);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* q = diag_side ? Qr : Ql;
  const float* Q = diag_side ? Ql : Qr;
  launch_sprod(Q, G, w.A, M, N, diag_side, nullptr, 0, nullptr, st);
  launch_sprod(Q, w.A, out, M, N, diag_side, q, 1, nullptr, st);
  return launched();
}

int psgd_kron_qdiag_update_f32(float* Ql, float* Qr, float* L, const float* G, int M, int N, int diag_side, float step, float decay,
                               void* ws, int64_t ws_bytes, void* stream) {
  if (!Ql || !Qr || !L || !G || M < 1 || N < 1 || (diag_side != 0 && diag_side != 1) || Ql == Qr || G == Ql || G == Qr || L == Ql ||
      L == Qr || L == G)
    return PSGD_ERR_BAD_ARG;
  const Dims d = dims_of(M, N, diag_side);
  if (ws_check(ws, ws_bytes, M, N, d)) return PSGD_ERR_WORKSPACE;
  const Ws w = carve(ws, M, N, d);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* q = diag_side ? Qr : Ql;
  float* Q = diag_side ? Ql : Qr;

  launch_sprod(Q, G, w.A, M, N, diag_side, q, 0, w.partd, st);

  const Opnd view = diag_side ? Opnd{w.A, N, 1, M} : Opnd{w.A, 1, N, N};   // (x, k) = (dense index, long index) of A
  const GramSide gs{view, d.n, d.D, d.nb, w.T, w.tmax, w.part};
  const Split sp{d.S, d.per, w.gpart};
  hipLaunchKernelGGL(k_gram_split, dim3((unsigned)(d.upper * d.S)), dim3(kT), 0, st, gs, sp);
  const int fold_tiles = d.S > 1 ? d.upper : 0;
  const TFold tf{w.partd, d.nb, d.D, w.t, w.tmaxd};
  hipLaunchKernelGGL(k_fold, dim3((unsigned)(fold_tiles + d.nblk)), dim3(kT), 0, st, gs, sp, fold_tiles, tf);

  const LipSide ls{d.n, d.nb, w.T, w.tmax, w.part, w.vec, (double)d.D};
  hipLaunchKernelGGL(k_lip, dim3(2), dim3(kLipT), 0, st, ls, L + (1 - diag_side), L + diag_side, w.coef, w.tmaxd, d.nblk,
                     (double)d.n, step, decay);

  const StepSide ps{d.n, d.nb, w.T, Q, w.P1, (float)d.D};
  const QStep qs{q, w.t, (float)d.n, d.D};
  hipLaunchKernelGGL(k_p1, dim3((unsigned)(d.nb * d.nb + d.nblk)), dim3(kT), 0, st, ps, w.coef, d.nb * d.nb, qs);
  hipLaunchKernelGGL(k_p2, dim3((unsigned)d.upper), dim3(kT), 0, st, ps, w.coef);
  return launched();
}

}  // extern "C"
