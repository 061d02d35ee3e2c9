// kron_quad_core.h -- what psgd_kron_quad.hip (both factors dense) and psgd_kron_qdiag.hip (one factor diagonal) share: the fp32
// MFMA product core and the per-side stages of the QUAD update on a dense symmetric factor (the Gram epilogue, the Lipschitz
// bound, P1 and the symmetrised P2).  Device code only, all of it inline: each unit wraps the bodies in kernels of its own.
//
// Product core.  product() forms one kTile x kTile (64 x 64) tile of C = op(A) op(B) for a workgroup of four waves, each wave a
// 32 x 32 quarter as 2 x 2 v_mfma_f32_16x16x4_f32 tiles: exact fp32 fma chains, so a chain of four products keeps fp32 accuracy.
// An operand is a strided view Opnd{p, xs, ks, X}: element (x, k) -- x the output index, k the summed one -- is p[x xs + k ks],
// which covers A, A', B and B' with one code path.  K runs in steps of kGK = 16 through double-buffered LDS (global -> registers
// for step t+1 is issued before the MFMAs of step t, registers -> LDS after them: one barrier per step).  The LDS image of an
// operand step is [k][x] with a pitch of 80 floats: an MFMA operand read takes k = lane >> 4, x = lane & 15, four runs of 16
// consecutive banks 16 apart, conflict-free for the 64 lanes; the x-contiguous fill writes 16-byte rows, the k-contiguous fill
// writes 64 consecutive floats of one k per wave instruction.  Global loads are 16 bytes (four x or four k, whichever is
// contiguous) when the base is 16-byte aligned, the other stride is a multiple of 4 and the step lies inside the operand; any
// other step (a partial tile, a ragged K tail, a skewed base, an odd leading dimension) takes dword loads with per-element
// bounds, zero-filled.  Nothing is ever read or written outside [0, X) x [0, K).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "psgd_kron_quad_hip.h"
#include "nanmax.h"

namespace psgdq {
using psgd::amaxf;

constexpr int kTile = PSGD_KRON_QUAD_TILE;   // output tile edge
constexpr int kT = 256;                      // threads per product workgroup: 2 x 2 waves of 32 x 32
constexpr int kGK = 16;                      // K step
constexpr int kPitch = kTile + 16;           // LDS row pitch of an operand step [kGK][kTile]
constexpr int kSP = kTile + 1;               // pitch of a whole tile parked in LDS (transposed reads conflict-free)
constexpr int kLdsFloats = 4 * kGK * kPitch; // A and B, two buffers each
static_assert(kTile == 64 && kT == 256 && kGK == 16, "the thread <-> element maps below are written for these");
static_assert(kTile * kSP <= kLdsFloats, "a parked tile reuses the operand buffers");
constexpr int kLipT = 1024;                  // threads of the per-side Lipschitz kernel

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Opnd {
  const float* p;
  long xs, ks;   // element (x, k) = p[x xs + k ks]; one of the two is 1 (both when a dimension is 1)
  int X;         // extent in x
};

// ------------------------------------------------------------------------------------------------------- the product core
// this thread's four elements of the step [x0, x0 + kTile) x [k0, k0 + kGK) of an operand, zero outside [0, X) x [0, K)
__device__ __forceinline__ void g2r(const Opnd& o, int x0, int k0, int K, float (&r)[4]) {
  const int t = threadIdx.x;
  const bool inside = x0 + kTile <= o.X && k0 + kGK <= K && (reinterpret_cast<uintptr_t>(o.p) & 15) == 0;
  if (o.xs == 1) {                                     // x contiguous: k = t >> 4, four x from (t & 15) * 4
    const int k = k0 + (t >> 4), x = x0 + (t & 15) * 4;
    if (inside && (o.ks & 3) == 0) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(o.p + (long)k * o.ks + x);
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = v[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = (k < K && x + e < o.X) ? o.p[(long)k * o.ks + (x + e)] : 0.f;
    }
  } else {                                             // k contiguous: x = t & 63, four k from (t >> 6) * 4
    const int x = x0 + (t & 63), k = k0 + (t >> 6) * 4;
    if (inside && o.ks == 1 && (o.xs & 3) == 0) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(o.p + (long)x * o.xs + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = v[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = (x < o.X && k + e < K) ? o.p[(long)x * o.xs + (long)(k + e) * o.ks] : 0.f;
    }
  }
}
// ... into the LDS image S[kGK][kPitch] of the step
__device__ __forceinline__ void r2s(const Opnd& o, const float (&r)[4], float* S) {
  const int t = threadIdx.x;
  if (o.xs == 1) {
    *reinterpret_cast<f32x4*>(S + (t >> 4) * kPitch + (t & 15) * 4) = f32x4{r[0], r[1], r[2], r[3]};
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) S[((t >> 6) * 4 + e) * kPitch + (t & 63)] = r[e];
  }
}

// acc = the tile (m0, n0) of sum_k a(m, k) b(n, k).  Enters with a barrier (the LDS may still be read by the caller's previous
// stage) and leaves after one: the LDS is free on return.  Element e of acc[i][j] is row wm 32 + i 16 + (lane >> 4) 4 + e,
// column wn 32 + j 16 + (lane & 15) of the tile.
__device__ __forceinline__ void product(const Opnd& a, const Opnd& b, int K, int m0, int n0, float* lds, f32x4 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1;
  float* LA = lds;
  float* LB = lds + 2 * kGK * kPitch;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nk = (K + kGK - 1) / kGK;
  float ra[4], rb[4];
  g2r(a, m0, 0, K, ra);
  g2r(b, n0, 0, K, rb);
  __syncthreads();
  r2s(a, ra, LA);
  r2s(b, rb, LB);
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    const bool more = t + 1 < nk;
    if (more) {
      g2r(a, m0, (t + 1) * kGK, K, ra);
      g2r(b, n0, (t + 1) * kGK, K, rb);
    }
    const float* A = LA + buf * kGK * kPitch;
    const float* B = LB + buf * kGK * kPitch;
#pragma unroll
    for (int kk = 0; kk < kGK / 4; ++kk) {
      const int kr = kk * 4 + (lane >> 4);
      float av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) av[i] = A[kr * kPitch + wm * 32 + i * 16 + (lane & 15)];
#pragma unroll
      for (int j = 0; j < 2; ++j) bv[j] = B[kr * kPitch + wn * 32 + j * 16 + (lane & 15)];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      r2s(a, ra, LA + (buf ^ 1) * kGK * kPitch);
      r2s(b, rb, LB + (buf ^ 1) * kGK * kPitch);
    }
    __syncthreads();
  }
}

// product() for operands of any two types that bring their own g2r() / r2s() overloads (found by argument type at the point of
// instantiation): the same schedule, the same MFMA loop, the same K order.  With two Opnd it is product() itself; a unit with an
// addressing that Opnd cannot express (psgd_kron_qnd.hip: a K index made of two tensor modes) defines the operand and its two
// fetch halves and calls this.
template <class OA, class OB>
__device__ __forceinline__ void product_of(const OA& a, const OB& b, int K, int m0, int n0, float* lds, f32x4 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1;
  float* LA = lds;
  float* LB = lds + 2 * kGK * kPitch;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nk = (K + kGK - 1) / kGK;
  float ra[4], rb[4];
  g2r(a, m0, 0, K, ra);
  g2r(b, n0, 0, K, rb);
  __syncthreads();
  r2s(a, ra, LA);
  r2s(b, rb, LB);
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    const bool more = t + 1 < nk;
    if (more) {
      g2r(a, m0, (t + 1) * kGK, K, ra);
      g2r(b, n0, (t + 1) * kGK, K, rb);
    }
    const float* A = LA + buf * kGK * kPitch;
    const float* B = LB + buf * kGK * kPitch;
#pragma unroll
    for (int kk = 0; kk < kGK / 4; ++kk) {
      const int kr = kk * 4 + (lane >> 4);
      float av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) av[i] = A[kr * kPitch + wm * 32 + i * 16 + (lane & 15)];
#pragma unroll
      for (int j = 0; j < 2; ++j) bv[j] = B[kr * kPitch + wn * 32 + j * 16 + (lane & 15)];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      r2s(a, ra, LA + (buf ^ 1) * kGK * kPitch);
      r2s(b, rb, LB + (buf ^ 1) * kGK * kPitch);
    }
    __syncthreads();
  }
}

// f(i, j, e, r, c) over this thread's 16 elements, (r, c) inside the tile
template <class F>
__device__ __forceinline__ void each_elem(F&& f) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) f(i, j, e, wm * 32 + i * 16 + (lane >> 4) * 4 + e, wn * 32 + j * 16 + (lane & 15));
}

// the tile parked in S (pitch kSP) to rows [r0, r0 + kTile) x columns [c0, c0 + kTile) of the n x n matrix C, in coalesced rows;
// mirror: S' to the tile (c0, r0) instead.  sym: element (r, c) is taken from the upper triangle of S (a diagonal tile).
__device__ __forceinline__ void store_tile(float* C, int n, int r0, int c0, const float* S, bool mirror, bool sym) {
  for (int idx = threadIdx.x; idx < kTile * kTile; idx += kT) {
    const int hi = idx >> 6, lo = idx & 63;            // lo runs along the stored row
    const int r = mirror ? lo : hi, c = mirror ? hi : lo;
    if (r0 + r < n && c0 + c < n) {
      const float v = sym ? S[min(r, c) * kSP + max(r, c)] : S[r * kSP + c];
      if (mirror) C[(long)(c0 + c) * n + (r0 + r)] = v; else C[(long)(r0 + r) * n + (c0 + c)] = v;
    }
  }
}

// upper tile number u of an nb x nb tile grid, row-major over ti <= tj
__device__ __forceinline__ void upper_tile(int u, int nb, int& ti, int& tj) {
  ti = 0;
  while (u >= nb - ti) {
    u -= nb - ti;
    ++ti;
  }
  tj = ti + u;
}

// ------------------------------------------------------------------------------------- the stages of one dense symmetric side
struct GramSide {
  Opnd o;          // (x, k) view of A whose Gram matrix this side is
  int n, K, nb;    // T is n x n, the sum runs over K, nb = tiles per edge
  float* T;
  float* tmax;     // [nb * nb], entry ti * nb + tj for ti <= tj
  double* part;    // [nb][n]: part[rb][c] = sum of squares of column c of T over the rows of tile row rb
};

// the finished upper tile (ti, tj) of T in acc: through LDS (free on entry) it is stored and, off the diagonal, mirrored (a
// diagonal tile symmetrised from its upper triangle), and leaves max|tile| and the fp64 column sums of squares (row sums for the
// mirror) as partials.  red: kT / 64 floats of LDS.
__device__ __forceinline__ void gram_epilogue(const GramSide& s, int ti, int tj, const f32x4 (&acc)[2][2], float* lds, float* red) {
  const int m0 = ti * kTile, n0 = tj * kTile;
  const bool diag = ti == tj;
  float mx = 0.f;                                       // rows and columns past n are exact zeros
  each_elem([&](int i, int j, int e, int r, int c) {
    lds[r * kSP + c] = acc[i][j][e];
    mx = amaxf(mx, fabsf(acc[i][j][e]));
  });
  for (int o = 32; o > 0; o >>= 1) mx = amaxf(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  store_tile(s.T, s.n, m0, n0, lds, false, diag);
  if (!diag) store_tile(s.T, s.n, m0, n0, lds, true, false);
  const int t = threadIdx.x;
  if (t == 0) s.tmax[ti * s.nb + tj] = amaxf(amaxf(red[0], red[1]), amaxf(red[2], red[3]));
  if (t < kTile) {                                      // column t of the tile: rows of tile row ti
    if (n0 + t < s.n) {
      double q = 0.0;
      for (int r = 0; r < kTile; ++r) {
        const double v = diag ? lds[min(r, t) * kSP + max(r, t)] : lds[r * kSP + t];
        q += v * v;
      }
      s.part[(long)ti * s.n + (n0 + t)] = q;
    }
  } else if (t < 2 * kTile && !diag) {                  // row t - 64 of the tile = a column of the mirror tile, tile row tj
    const int r = t - kTile;
    if (m0 + r < s.n) {
      double q = 0.0;
      for (int c = 0; c < kTile; ++c) {
        const double v = lds[r * kSP + c];
        q += v * v;
      }
      s.part[(long)tj * s.n + (m0 + r)] = q;
    }
  }
}

struct LipSide {
  int n, nb;
  const float* T;
  const float* tmax;
  const double* part;
  double* vec;     // [2 n]: x then y
  double t2;
};

__device__ __forceinline__ double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int h = kLipT / 2; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// L <- max(decay L + (1 - decay) ell, ell) in place and c = step / (2 L) to *coef, by one thread
__device__ __forceinline__ void lipschitz_write(double ell, float* L, float* coef, float step, float decay) {
  const double d = (double)decay;
  const double Ln = psgd::nmax(d * (double)*L + (1.0 - d) * ell, ell);
  *L = (float)Ln;
  *coef = (float)((double)step / (2.0 * Ln));
}

// one workgroup of kLipT threads: s, j, the two matvecs of a dense side, its L (in place) and its c.  red: kLipT doubles, redi:
// kLipT ints, redf: kLipT / 64 floats of LDS.
__device__ __forceinline__ void lipschitz_dense(const LipSide& s, float* L, float* coef, float step, float decay, double* red,
                                                int* redi, float* redf) {
  const int t = threadIdx.x, n = s.n;
  float m = 0.f;
  for (int idx = t; idx < s.nb * s.nb; idx += kLipT)
    if (idx % s.nb >= idx / s.nb) m = amaxf(m, s.tmax[idx]);
  for (int o = 32; o > 0; o >>= 1) m = amaxf(m, __shfl_xor(m, o, 64));
  if ((t & 63) == 0) redf[t >> 6] = m;
  __syncthreads();
  m = 0.f;
  for (int k = 0; k < kLipT / 64; ++k) m = amaxf(m, redf[k]);
  double bound = 0.0;
  if (m != 0.f) {                                       // uniform; NaN takes this arm and comes out as NaN
    double best = -1.0;
    int bj = 0x7fffffff;
    for (int c = t; c < n; c += kLipT) {
      double q = 0.0;
      for (int rb = 0; rb < s.nb; ++rb) q += s.part[(long)rb * n + c];
      if (q > best) {
        best = q;
        bj = c;
      }
    }
    red[t] = best;
    redi[t] = bj;
    __syncthreads();
    for (int h = kLipT / 2; h > 0; h >>= 1) {
      if (t < h && (red[t + h] > red[t] || (red[t + h] == red[t] && redi[t + h] < redi[t]))) {
        red[t] = red[t + h];
        redi[t] = redi[t + h];
      }
      __syncthreads();
    }
    const int j = redi[0] < n ? redi[0] : 0;            // (every sum NaN: any column gives the NaN the result must be)
    __syncthreads();
    const double sd = (double)m, inv = 1.0 / sd;
    double* x = s.vec;
    double* y = s.vec + n;
    for (int i = t; i < n; i += kLipT) x[i] = (double)s.T[(long)j * n + i] * inv;
    __syncthreads();
    double ss = 0.0;
    for (int i = t; i < n; i += kLipT) {
      double a = 0.0;
      for (int k = 0; k < n; ++k) a += ((double)s.T[(long)k * n + i] * inv) * x[k];
      y[i] = a;
      ss += a * a;
    }
    const double ny = sqrt(block_sum(ss, red));
    for (int i = t; i < n; i += kLipT) y[i] = y[i] / ny;
    __syncthreads();
    ss = 0.0;
    for (int i = t; i < n; i += kLipT) {
      double a = 0.0;
      for (int k = 0; k < n; ++k) a += ((double)s.T[(long)k * n + i] * inv) * y[k];
      ss += a * a;
    }
    bound = sd * sqrt(block_sum(ss, red));
  }
  if (t == 0) lipschitz_write(bound + s.t2, L, coef, step, decay);
}

struct StepSide {
  int n, nb;
  const float* T;
  float* Q;        // read by p1_tile, rewritten by p2_sym_tiles
  float* P1;
  float t2;
};

// acc = the tile (m0, n0) of T Q: the tile of P1 = Q - c (T Q - t2 Q) is stored
__device__ __forceinline__ void p1_store(const StepSide& s, float c1, int m0, int n0, const f32x4 (&acc)[2][2]) {
  const int n = s.n;
  each_elem([&](int i, int j, int e, int r, int c) {
    if (m0 + r < n && n0 + c < n) {
      const long at = (long)(m0 + r) * n + (n0 + c);
      const float q = s.Q[at];
      s.P1[at] = q - c1 * (acc[i][j][e] - s.t2 * q);
    }
  });
}

// tile b (row-major over nb x nb) of P1 = Q - c (T Q - t2 Q)
__device__ __forceinline__ void p1_tile(const StepSide& s, int b, float c1, float* lds) {
  const int n = s.n;
  const int m0 = (b / s.nb) * kTile, n0 = (b % s.nb) * kTile;
  f32x4 acc[2][2];
  product(Opnd{s.T, n, 1, n}, Opnd{s.Q, 1, n, n}, n, m0, n0, lds, acc);
  p1_store(s, c1, m0, n0, acc);
}

// acc = the tile (m0, n0) of P1 T on entry, of P2 = P1 - c (P1 T - t2 P1) on return, zero outside the matrix
__device__ __forceinline__ void p2_finish(const StepSide& s, float c1, int m0, int n0, f32x4 (&acc)[2][2]) {
  const int n = s.n;
  each_elem([&](int i, int j, int e, int r, int c) {
    float v = 0.f;
    if (m0 + r < n && n0 + c < n) {
      const float p = s.P1[(long)(m0 + r) * n + (n0 + c)];
      v = p - c1 * (acc[i][j][e] - s.t2 * p);
    }
    acc[i][j][e] = v;
  });
}

// the tile (m0, n0) of P2
__device__ __forceinline__ void p2_tile(const StepSide& s, float c1, int m0, int n0, float* lds, f32x4 (&acc)[2][2]) {
  product(Opnd{s.P1, s.n, 1, s.n}, Opnd{s.T, 1, s.n, s.n}, s.n, m0, n0, lds, acc);
  p2_finish(s, c1, m0, n0, acc);
}

// up = the tile (m0, n0) of P2, lo = the tile (n0, m0) (diag: not read): (up + lo') / 2, the transpose through LDS (free on
// entry), is written to the tile (m0, n0) of Q and, off the diagonal, transposed to (n0, m0).  Ends without a barrier.
__device__ __forceinline__ void p2_sym_store(const StepSide& s, int m0, int n0, bool diag, f32x4 (&up)[2][2], const f32x4 (&lo)[2][2],
                                             float* lds) {
  if (!diag) {
    each_elem([&](int i, int j, int e, int r, int c) { lds[r * kSP + c] = lo[i][j][e]; });   // local (r, c) of tile (tj, ti)
  } else {
    each_elem([&](int i, int j, int e, int r, int c) { lds[r * kSP + c] = up[i][j][e]; });
  }
  __syncthreads();
  each_elem([&](int i, int j, int e, int r, int c) { up[i][j][e] = 0.5f * (up[i][j][e] + lds[c * kSP + r]); });
  __syncthreads();
  each_elem([&](int i, int j, int e, int r, int c) { lds[r * kSP + c] = up[i][j][e]; });
  __syncthreads();
  store_tile(s.Q, s.n, m0, n0, lds, false, false);      // (a diagonal tile is symmetric already: a + b == b + a)
  if (!diag) store_tile(s.Q, s.n, m0, n0, lds, true, false);
}

// Q <- (P2 + P2') / 2 on upper tile u: P2 is formed on (ti, tj) AND on (tj, ti), the second transposed through LDS, the two
// averaged, and both tiles of Q written -- Q[i,j] and Q[j,i] are one value written twice
__device__ __forceinline__ void p2_sym_tiles(const StepSide& s, int u, float c1, float* lds) {
  int ti, tj;
  upper_tile(u, s.nb, ti, tj);
  const int m0 = ti * kTile, n0 = tj * kTile;
  const bool diag = ti == tj;
  f32x4 up[2][2], lo[2][2];
  p2_tile(s, c1, m0, n0, lds, up);
  if (!diag) p2_tile(s, c1, n0, m0, lds, lo);
  p2_sym_store(s, m0, n0, diag, up, lo, lds);
}

// --------------------------------------------------------------------------------------------------------------- the host
static inline int64_t up256(int64_t b) { return (b + 255) & ~int64_t(255); }
static inline int tiles_of(int n) { return (n + kTile - 1) / kTile; }
static inline int launched() { return hipGetLastError() == hipSuccess ? PSGD_OK : PSGD_ERR_LAUNCH; }

}  // namespace psgdq
