// psgd_splu_bf16.hip -- the sparse-LU preconditioner (psgd.py:396-524) on a state whose HBM image is bf16.
//
//   Q = L U,  L = [L1 0; L2 diag(l3)],  U = [U1 U2; 0 diag(u3)]
//
// L12 = [L1; L2] ([N, r] row-major), U12 = [U1, U2] ([r, N] row-major), l3 and u3 ([N - r]) are stored as bf16; dx, dg, g and
// the preconditioned gradient are fp32.  Elements are widened when they are loaded and narrowed exactly once, when an output
// element is written.  One kernel family for ranks 1 .. 32 with the rank as a run-time value:
//
//   * A tile is TR consecutive rows n of L12 and the same TR columns n of every row of U12 (Geo of bf16_state.h); thread t of
//     a block owns row / column row0 + t.  L12 is copied with load_tile / store_tile of bf16_state.h; a row of U12 is a span
//     of N codes that starts at any 2-byte offset, so its tile segment is covered with the 16-byte chunks of the ALIGNED flat
//     buffer: loads read whole chunks (only codes of the buffer), stores write whole chunks inside the segment and single
//     codes at its two ragged ends -- a neighbouring tile's codes are never touched.
//   * The rows n < r are the r x r heads L1 and U1: the sweeps skip them, a one-wave kernel reads them into fp64 and does
//     the r x r algebra (four triangular solves, both grad1 blocks, both max_abs_grad, the new heads) between the sweeps.
//   * Arithmetic: the row-local expressions, the block partials, the r x r algebra and every fold are fp64 -- the row-local
//     part too, which the fp32 family (splu_kernels.h) does in fp32: a value that is rounded to bf16 is then the nearest code
//     of the exact result except in ties of the fp64 arithmetic itself.  The fp64 result goes to fp32 with round-to-odd
//     (to_f32_odd), so the one narrowing that follows rounds the fp64 value correctly.
//   * The balance of :411-417 comes FIRST, as in the reference: a pre-pass takes max l3 / max u3 over the stored codes, the
//     one-wave kernel k_rho adds the head diagonals; every later kernel works on L12 / rho, l3 / rho, rho U12, rho u3.  Every
//     element of the state is therefore rescaled and re-rounded by every update.
//   * Reductions have a fixed order (tile -> thread partition -> block -> fold over blocks in block order); no float
//     atomics.  Grids are sized by the LDS footprint on a fixed CU count: results do not depend on the device.
//   * Maxima follow the reference as the fp64 oracle transcribes it: reduce_max over an array propagates NaN, and the
//     scalars are then combined in the order written (max_l = max(head, tail); max_abs_grad = max(grad1, grad2, grad3)).
//
//   apply   a1: U2 g2 | a2: Qg2 (parked in out), L2' Qg2 | a3: out2                       reads (2r + 2) * 2 + 12 B / row
//   update  s0: max l3, u3 | s1: U2 dg2 | s2: L2'Qg2, L2'iQtx2 | s3: U2 iPx2, maxima | s4: the new factors
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "bf16_state.h"
#include "nanmax.h"
#include "psgd_hip.h"

namespace {

using namespace psgd::bf16s;
using psgd::nmax;

constexpr int kMaxR = PSGD_UVD_MAX_RANK;
constexpr int kMaxBlocks = 1024;   // cap of every sweep grid
constexpr int kCUs = 256;          // grids are a property of the kernel family, not of the device
constexpr int kLDU = kT + 1;       // LDS stride (floats) of one U12 row of a tile: odd, so r-strided reads spread over the banks
constexpr int kCPR = kT / 8 + 1;   // 16-byte chunks that cover a tile segment of a U12 row at any phase
constexpr int kPartStride = 2 * kMaxR;
constexpr unsigned kIdL12 = 8, kIdl3 = 9, kIdU12 = 10, kIdu3 = 11;   // rounding-stream tensor ids (UVd: 0, 1, 2)

// workspace header, in doubles
enum { kUg1 = 0, kQg1 = 32, kIUtx1 = 64, kIQtx1 = 96, kLtQg1 = 128, kPg1 = 160, kILiQtx1 = 192, kCa = 224, kCb = 256,
       kCc = 288, kCe = 320, kScal = 352 /* rho, 1/rho, sL, sU */, kHdrDoubles = 384 };
constexpr int64_t kOffHdr = 0;
constexpr int64_t kOffHeads = kHdrDoubles * 8;                          // float[2][32 * 32]: the new L1, U1 (round-to-odd fp32)
constexpr int64_t kOffPart = kOffHeads + 2 * kMaxR * kMaxR * 4;         // double[kMaxBlocks][64]: block partial sums
constexpr int64_t kOffPmax = kOffPart + (int64_t)kMaxBlocks * kPartStride * 8;   // double[kMaxBlocks][6]: block maxima
constexpr int64_t kWsBytes = (kOffPmax + (int64_t)kMaxBlocks * 6 * 8 + 255) & ~(int64_t)255;

struct Ws { double* hdr; float* heads; double* part; double* pmax; };

enum Stage { kDot = 0, kA2 = 1, kA3 = 2, kU2 = 3, kU3 = 4, kU4 = 5 };

// fp64 -> fp32 with round-to-odd: truncated towards zero, the last bit set when the conversion is inexact.  Rounding that
// fp32 value to bf16 (16 bits fewer) gives the correctly rounded bf16 code of the fp64 value.  NaN and Inf pass.
__device__ __forceinline__ float to_f32_odd(double x) {
  const float f = (float)x;
  if (f != f) return f;
  const double d = (double)f;
  if (d == x) return f;
  unsigned b = __float_as_uint(f);
  if (fabs(d) > fabs(x)) b -= 1u;
  return __uint_as_float(b | 1u);
}

// maximum as the oracle's scalar max(cur, x): x replaces cur only when it compares greater
__device__ __forceinline__ double pymax(double cur, double x) { return (x > cur) ? x : cur; }

__device__ __forceinline__ double wave_nmax(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = nmax(v, __shfl_xor(v, o));
  return v;
}

// tile segment [row0, row0 + rows) of the r rows of U12 ([r, N] bf16) -> Us[k * kLDU + t], fp32
__device__ __forceinline__ void load_cols(const u16* __restrict__ U, float* Us, int r, long N, long row0, int rows) {
  const long total = (long)r * N;
  for (int idx = threadIdx.x; idx < r * kCPR; idx += kT) {
    const int k = idx / kCPR, j = idx - k * kCPR;
    const long s0 = (long)k * N + row0;
    const long a0 = (s0 & ~7L) + 8L * j;
    if (a0 >= s0 + rows) continue;
    float* dst = Us + k * kLDU;
    if (a0 + 8 <= total) {
      const u32x4 raw = *reinterpret_cast<const u32x4*>(U + a0);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const long col = a0 + e - s0;
        const unsigned bits = (e & 1) ? (raw[e >> 1] & 0xffff0000u) : (raw[e >> 1] << 16);
        if (col >= 0 && col < rows) dst[col] = __uint_as_float(bits);
      }
    } else {
      for (int e = 0; e < 8; ++e) {
        const long col = a0 + e - s0;
        if (a0 + e < total && col >= 0 && col < rows) dst[col] = widen(U[a0 + e]);
      }
    }
  }
}

// Us (fp32 values that are exact bf16) -> the same segment of the output U12
__device__ __forceinline__ void store_cols(u16* __restrict__ U, const float* Us, int r, long N, long row0, int rows) {
  for (int idx = threadIdx.x; idx < r * kCPR; idx += kT) {
    const int k = idx / kCPR, j = idx - k * kCPR;
    const long s0 = (long)k * N + row0;
    const long a0 = (s0 & ~7L) + 8L * j;
    if (a0 >= s0 + rows) continue;
    const float* src = Us + k * kLDU;
    const long c0 = a0 - s0;
    if (c0 >= 0 && c0 + 8 <= rows) {       // the chunk lies inside the segment (and so inside the buffer)
      u32x4 raw;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        raw[q] = (__float_as_uint(src[c0 + 2 * q]) >> 16) | (__float_as_uint(src[c0 + 2 * q + 1]) & 0xffff0000u);
      *reinterpret_cast<u32x4*>(U + a0) = raw;
    } else {
      for (int e = 0; e < 8; ++e) {
        const long col = c0 + e;
        if (col >= 0 && col < rows) U[s0 + col] = (u16)(__float_as_uint(src[col]) >> 16);
      }
    }
  }
}

// ------------------------------------------------------------------ s0: max l3, max u3 over the stored codes (:411-412)
__global__ __launch_bounds__(kT) void k_tailmax(const u16* __restrict__ l3, const u16* __restrict__ u3, long n2,
                                                double* pmax) {
  __shared__ double red[2][4];
  double ml = -INFINITY, mu = -INFINITY;
  const long nch = (n2 + 7) / 8;
  for (long c = (long)blockIdx.x * kT + threadIdx.x; c < nch; c += (long)gridDim.x * kT) {
    const long e0 = 8 * c;
    if (e0 + 8 <= n2) {
      const u32x4 a = *reinterpret_cast<const u32x4*>(l3 + e0), b = *reinterpret_cast<const u32x4*>(u3 + e0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        ml = nmax(ml, (double)widen(a[q] & 0xffffu)); ml = nmax(ml, (double)widen(a[q] >> 16));
        mu = nmax(mu, (double)widen(b[q] & 0xffffu)); mu = nmax(mu, (double)widen(b[q] >> 16));
      }
    } else {
      for (long e = e0; e < n2; ++e) {
        ml = nmax(ml, (double)widen(l3[e]));
        mu = nmax(mu, (double)widen(u3[e]));
      }
    }
  }
  ml = wave_nmax(ml);
  mu = wave_nmax(mu);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = ml; red[1][threadIdx.x >> 6] = mu; }
  __syncthreads();
  if (threadIdx.x == 0) {
    pmax[2 * blockIdx.x] = nmax(nmax(red[0][0], red[0][1]), nmax(red[0][2], red[0][3]));
    pmax[2 * blockIdx.x + 1] = nmax(nmax(red[1][0], red[1][1]), nmax(red[1][2], red[1][3]));
  }
}

// rho = sqrt(max_l / max_u) (:411-413); nblk = 0: no tail (reduce_max of an empty tensor is -inf); balance = 0 (apply): 1
__global__ __launch_bounds__(64) void k_rho(const u16* __restrict__ L12, const u16* __restrict__ U12, long N, int r,
                                            const double* pmax, int nblk, int balance, double* hdr) {
  const int t = threadIdx.x;
  double rho = 1.0;
  if (balance) {
    double dl = -INFINITY, du = -INFINITY;
    if (t < r) { dl = (double)widen(L12[(long)t * r + t]); du = (double)widen(U12[(long)t * N + t]); }
    dl = wave_nmax(dl);
    du = wave_nmax(du);
    double ml = -INFINITY, mu = -INFINITY;
    for (int b = t; b < nblk; b += 64) { ml = nmax(ml, pmax[2 * b]); mu = nmax(mu, pmax[2 * b + 1]); }
    ml = wave_nmax(ml);
    mu = wave_nmax(mu);
    rho = sqrt(pymax(dl, ml) / pymax(du, mu));
  }
  if (t == 0) { hdr[kScal] = rho; hdr[kScal + 1] = 1.0 / rho; }
}

// ------------------------------------------------------------------ r x r heads (fp64, one wave)
struct Corner {
  double L1[kMaxR][kMaxR + 1];
  double U1[kMaxR][kMaxR + 1];
  double v[8][kMaxR];
};

// the balanced heads L1 / rho and rho U1
__device__ __forceinline__ void corner_load(Corner& c, const u16* L12, const u16* U12, long N, int r, const double* hdr) {
  const double rho = hdr[kScal], irho = hdr[kScal + 1];
  for (int e = threadIdx.x; e < r * r; e += 64) {
    const int i = e / r, j = e - i * r;
    c.L1[i][j] = (double)widen(L12[(long)i * r + j]) * irho;
    c.U1[i][j] = rho * (double)widen(U12[(long)i * N + j]);
  }
  __syncthreads();
}

// y = M x (trans = false) or M' x; y must not alias x
__device__ __forceinline__ void corner_matvec(const double (*M)[kMaxR + 1], bool trans, const double* x, double* y, int r) {
  const int i = threadIdx.x;
  if (i < r) {
    double s = 0.0;
    for (int j = 0; j < r; ++j) s += (trans ? M[j][i] : M[i][j]) * x[j];
    y[i] = s;
  }
  __syncthreads();
}

// in place: b <- T^-1 b, T = M or M'; `lower` says which triangle of M is used (the other one is ignored)
__device__ __forceinline__ void corner_trisolve(const double (*M)[kMaxR + 1], bool lower, bool trans, double* b, int r) {
  const bool fwd = (lower != trans);
  const int j = threadIdx.x;
  for (int step = 0; step < r; ++step) {
    const int p = fwd ? step : r - 1 - step;
    if (j == p) b[p] = b[p] / M[p][p];
    __syncthreads();
    const bool rem = fwd ? (j > p && j < r) : (j < p);
    if (rem) b[j] -= (trans ? M[p][j] : M[j][p]) * b[p];
    __syncthreads();
  }
}

// sum over the blocks, in block order, of column `col` of the block partials
__device__ __forceinline__ double fold_part(const double* part, int nblk, int col) {
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(long)b * kPartStride + col];
  return s;
}

// after a1 / s1: Ug1 = U1 x1 + U2 x2 (:430 / :506), Qg1 = L1 Ug1 (:433 / :509); update: iUtx1 = U1^-T dx1 (:436)
__global__ __launch_bounds__(64) void k_corner1(const u16* L12, const u16* U12, long N, int r, const float* x /* g or dg */,
                                                const float* dx /* null for the apply */, const double* part, int nblk,
                                                double* hdr) {
  __shared__ Corner c;
  corner_load(c, L12, U12, N, r, hdr);
  const int t = threadIdx.x;
  if (t < r) c.v[0][t] = (double)x[t];
  __syncthreads();
  corner_matvec(c.U1, false, c.v[0], c.v[1], r);
  if (t < r) {
    c.v[1][t] += fold_part(part, nblk, t);
    hdr[kUg1 + t] = c.v[1][t];
  }
  __syncthreads();
  corner_matvec(c.L1, false, c.v[1], c.v[2], r);
  if (t < r) hdr[kQg1 + t] = c.v[2][t];
  if (dx) {
    if (t < r) c.v[3][t] = (double)dx[t];
    __syncthreads();
    corner_trisolve(c.U1, /*lower=*/false, /*trans=*/true, c.v[3], r);
    if (t < r) hdr[kIUtx1 + t] = c.v[3][t];
  }
}

// apply, after a2: LtQg1 = L1' Qg1 + L2' Qg2 (:512); out1 = U1' LtQg1 (:515)
__global__ __launch_bounds__(64) void k_corner_apply2(const u16* L12, const u16* U12, long N, int r, const double* part,
                                                      int nblk, double* hdr, float* out) {
  __shared__ Corner c;
  corner_load(c, L12, U12, N, r, hdr);
  const int t = threadIdx.x;
  if (t < r) c.v[0][t] = hdr[kQg1 + t];
  __syncthreads();
  corner_matvec(c.L1, true, c.v[0], c.v[1], r);
  if (t < r) {
    c.v[1][t] += fold_part(part, nblk, t);
    hdr[kLtQg1 + t] = c.v[1][t];
  }
  __syncthreads();
  corner_matvec(c.U1, true, c.v[1], c.v[2], r);
  if (t < r) out[t] = (float)c.v[2][t];
}

// update, after s2: iQtx1 (:440), LtQg1 (:442), Pg1 (:445), iLiQtx1 (:448)
__global__ __launch_bounds__(64) void k_corner_upd2(const u16* L12, const u16* U12, long N, int r, const double* part,
                                                    int nblk, double* hdr) {
  __shared__ Corner c;
  corner_load(c, L12, U12, N, r, hdr);
  const int t = threadIdx.x;
  if (t < r) {
    c.v[0][t] = hdr[kIUtx1 + t] - fold_part(part, nblk, r + t);   // iUtx1 - L2' iQtx2
    c.v[1][t] = hdr[kQg1 + t];
    c.v[5][t] = fold_part(part, nblk, t);                         // L2' Qg2
  }
  __syncthreads();
  corner_trisolve(c.L1, /*lower=*/true, /*trans=*/true, c.v[0], r);   // iQtx1
  corner_matvec(c.L1, true, c.v[1], c.v[2], r);                      // L1' Qg1
  if (t < r) c.v[2][t] += c.v[5][t];                                  // LtQg1
  __syncthreads();
  corner_matvec(c.U1, true, c.v[2], c.v[3], r);                      // Pg1
  if (t < r) c.v[4][t] = c.v[0][t];
  __syncthreads();
  corner_trisolve(c.L1, /*lower=*/true, /*trans=*/false, c.v[4], r);  // iLiQtx1
  if (t < r) {
    hdr[kIQtx1 + t] = c.v[0][t];
    hdr[kLtQg1 + t] = c.v[2][t];
    hdr[kPg1 + t] = c.v[3][t];
    hdr[kILiQtx1 + t] = c.v[4][t];
  }
}

// update, after s3: iPx1 (:452); both grad1 blocks, both step sizes, the new heads (:455-463, :468-476) as round-to-odd
// fp32 for s4 to narrow; the r-vectors a = L1' Qg1, b = L1' iQtx1, c = U1 Pg1, e = U1 dx1 of the tail rows' update
__global__ __launch_bounds__(64) void k_corner_upd3(const u16* L12, const u16* U12, long N, int r, const float* dx,
                                                    const float* dg, float step, float tiny, const double* part,
                                                    const double* pmax, int nblk, double* hdr, float* heads) {
  __shared__ Corner c;
  __shared__ double G[kMaxR][kMaxR + 1];
  corner_load(c, L12, U12, N, r, hdr);
  const int t = threadIdx.x;
  // v0 = iPx1, v1 = Qg1, v2 = iQtx1, v3 = Pg1, v4 = dx1, v5 = dg1
  if (t < r) {
    c.v[0][t] = hdr[kILiQtx1 + t] - fold_part(part, nblk, t);
    c.v[1][t] = hdr[kQg1 + t];
    c.v[2][t] = hdr[kIQtx1 + t];
    c.v[3][t] = hdr[kPg1 + t];
    c.v[4][t] = (double)dx[t];
    c.v[5][t] = (double)dg[t];
  }
  __syncthreads();
  corner_trisolve(c.U1, /*lower=*/false, /*trans=*/false, c.v[0], r);
  // block maxima of the tail: |grad2|, |grad3| of L, then of U (0 without a tail, as the maximum of an empty array)
  double mx[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = t; b < nblk; b += 64)
#pragma unroll
    for (int q = 0; q < 4; ++q) mx[q] = nmax(mx[q], pmax[(long)b * 6 + q]);
#pragma unroll
  for (int q = 0; q < 4; ++q) mx[q] = wave_nmax(mx[q]);

  // ---- L: grad1 = tril(Qg1 Qg1' - iQtx1 iQtx1'), step0, newL1 = L1 - (step0 grad1) L1
  double m = 0.0;
  for (int e = t; e < r * r; e += 64) {
    const int i = e / r, j = e - i * r;
    const double g = (j <= i) ? c.v[1][i] * c.v[1][j] - c.v[2][i] * c.v[2][j] : 0.0;
    G[i][j] = g;
    m = nmax(m, fabs(g));
  }
  m = pymax(pymax(wave_nmax(m), mx[0]), mx[1]);
  const double sL = (double)step / (m + (double)tiny);
  __syncthreads();
  for (int e = t; e < r * r; e += 64) {
    const int i = e / r, j = e - i * r;
    double s = 0.0;
    for (int k = 0; k < r; ++k) s += (sL * G[i][k]) * c.L1[k][j];
    heads[i * kMaxR + j] = to_f32_odd(c.L1[i][j] - s);
  }
  if (t < r) {
    double a = 0.0, b = 0.0;
    for (int k = 0; k < r; ++k) {
      a += c.L1[k][t] * c.v[1][k];
      b += c.L1[k][t] * c.v[2][k];
    }
    hdr[kCa + t] = a;
    hdr[kCb + t] = b;
  }
  __syncthreads();

  // ---- U: grad1 = triu(Pg1 dg1' - dx1 iPx1'), step0, newU1 = U1 - U1 (step0 grad1)
  m = 0.0;
  for (int e = t; e < r * r; e += 64) {
    const int i = e / r, j = e - i * r;
    const double g = (j >= i) ? c.v[3][i] * c.v[5][j] - c.v[4][i] * c.v[0][j] : 0.0;
    G[i][j] = g;
    m = nmax(m, fabs(g));
  }
  m = pymax(pymax(wave_nmax(m), mx[2]), mx[3]);
  const double sU = (double)step / (m + (double)tiny);
  __syncthreads();
  for (int e = t; e < r * r; e += 64) {
    const int i = e / r, j = e - i * r;
    double s = 0.0;
    for (int k = 0; k < r; ++k) s += c.U1[i][k] * (sU * G[k][j]);
    heads[kMaxR * kMaxR + i * kMaxR + j] = to_f32_odd(c.U1[i][j] - s);
  }
  if (t < r) {
    double cc = 0.0, ee = 0.0;
    for (int k = 0; k < r; ++k) {
      cc += c.U1[t][k] * c.v[3][k];
      ee += c.U1[t][k] * c.v[4][k];
    }
    hdr[kCc + t] = cc;
    hdr[kCe + t] = ee;
  }
  if (t == 0) { hdr[kScal + 2] = sL; hdr[kScal + 3] = sU; }
}

// ------------------------------------------------------------------ the sweeps over the N - r tail rows
// dynamic LDS: double red[2][kT] | double X[2][kT] | float A[TR * rp] (the L12 tile) | float Us[r * kLDU] (the U12 tile)
constexpr size_t kLdsDoubles = 4 * kT;
size_t sweep_lds(const Geo& g) { return kLdsDoubles * 8 + ((size_t)kT * g.rp + (size_t)g.r * kLDU) * 4; }
constexpr size_t kSweepLdsMax = kLdsDoubles * 8 + ((size_t)kT * (kMaxR | 1) + (size_t)kMaxR * kLDU) * 4;

struct SweepArgs {
  const u16 *L12, *l3, *U12, *u3;   // the state
  const float *x, *dx;              // kDot: the vector of the product; kA2: g; update sweeps: x = dg, dx
  float* out;                       // apply: the preconditioned gradient (kA2 parks Qg2 in it)
  u16 *L12o, *l3o, *U12o, *u3o;     // kU4
  long N;
  const double* hdr;
  const float* heads;
  double *part, *pmax;
  int mode;
  SrKey keyL, keyl, keyU, keyu;
};

template <int STAGE>
__global__ __launch_bounds__(kT) void k_sweep(SweepArgs a, Geo g) {
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  double* red = lds_d;
  double* X0 = lds_d + 2 * kT;
  double* X1 = X0 + kT;
  float* A = reinterpret_cast<float*>(lds_d + kLdsDoubles);
  float* Us = A + kT * g.rp;
  constexpr bool kNeedL = STAGE == kA2 || STAGE == kU2 || STAGE == kU3 || STAGE == kU4;
  constexpr bool kNeedU = STAGE != kA2;
  constexpr bool kSumL = STAGE == kA2 || STAGE == kU2;
  constexpr bool kSumU = STAGE == kDot || STAGE == kU3;
  constexpr bool kUpdate = STAGE >= kU2;
  const int r = g.r, t = threadIdx.x;
  const long N = a.N;
  const Slots sl = make_slots(g);
  const double* h = a.hdr;
  const double rho = h[kScal], irho = h[kScal + 1];
  const double sL = (STAGE == kU4) ? h[kScal + 2] : 0.0, sU = (STAGE == kU4) ? h[kScal + 3] : 0.0;
  // thread (c, p) of the column sums: column c of the tile, rows p, p + P, ...
  const int P = kT / r;
  const int sc = t % r, sp = t / r;
  double acc0 = 0.0, acc1 = 0.0;
  double mL2 = 0.0, mL3 = 0.0, mU2 = 0.0, mU3 = 0.0;

  const long ntiles = (N + g.TR - 1) / g.TR;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long row0 = tile * g.TR;
    const int rows = (int)((N - row0 < g.TR) ? (N - row0) : g.TR);
    const int t_lo = (row0 < r) ? (int)(r - row0) : 0;       // the head rows (tile 0 only) are not tail rows
    if (kNeedL) load_tile(a.L12, A, g, sl, row0, rows, 1.0f);
    if (kNeedU) load_cols(a.U12, Us, r, N, row0, rows);
    __syncthreads();
    const bool tail = t >= t_lo && t < rows;
    if (tail) {
      const long n = row0 + t, i = n - r;
      float* a_ = A + t * g.rp;
      float* u_ = Us + t;
      if (STAGE == kDot) {
        X0[t] = (double)a.x[n];
      } else {
        const double l = (double)widen(a.l3[i]) * irho, u = rho * (double)widen(a.u3[i]);
        if (STAGE == kA2) {
          double q = 0.0;
          for (int c = 0; c < r; ++c) q += ((double)a_[c] * irho) * h[kUg1 + c];
          q += l * (u * (double)a.x[n]);                                          // :507, :510
          a.out[n] = (float)q;
          X0[t] = q;
        } else if (STAGE == kA3) {
          double o = 0.0;
          for (int k = 0; k < r; ++k) o += (rho * (double)u_[k * kLDU]) * h[kLtQg1 + k];
          a.out[n] = (float)(o + u * (l * (double)a.out[n]));                      // :513, :516
        } else {
          const double gg = (double)a.x[n], xx = (double)a.dx[n];
          double q = 0.0, du = 0.0;
          for (int c = 0; c < r; ++c) q += ((double)a_[c] * irho) * h[kUg1 + c];
          q += l * (u * gg);                                                      // Qg2    :431, :434
          for (int k = 0; k < r; ++k) du += (rho * (double)u_[k * kLDU]) * h[kIUtx1 + k];
          const double iq = ((xx - du) / u) / l;                                  // iQtx2  :437, :439
          if (STAGE == kU2) {
            X0[t] = q;
            X1[t] = iq;
          } else {
            double pg = 0.0, dl = 0.0;
            for (int k = 0; k < r; ++k) pg += (rho * (double)u_[k * kLDU]) * h[kLtQg1 + k];
            pg += u * (l * q);                                                    // Pg2    :443, :446
            for (int c = 0; c < r; ++c) dl += ((double)a_[c] * irho) * h[kILiQtx1 + c];
            const double ipx = ((iq - dl) / l) / u;                               // iPx2   :449, :451
            const double g3L = q * q - iq * iq, g3U = pg * gg - xx * ipx;         // grad3  :458, :471
            if (STAGE == kU3) {
              X0[t] = ipx;
              mL3 = nmax(mL3, fabs(g3L));
              mU3 = nmax(mU3, fabs(g3U));
              for (int k = 0; k < r; ++k) {                                       // grad2  :457, :470
                mL2 = nmax(mL2, fabs(q * h[kQg1 + k] - iq * h[kIQtx1 + k]));
                mU2 = nmax(mU2, fabs(h[kPg1 + k] * gg - (double)a.dx[k] * ipx));
              }
            } else {   // kU4: :464-465, :477-478
              const double gl3 = sL * g3L, gu3 = sU * g3U;
              const double sq = sL * q, siq = sL * iq, sg = sU * gg, sp_ = sU * ipx;
              const unsigned long long eL = (unsigned long long)n * (unsigned)r;
              for (int c = 0; c < r; ++c) {
                const double lk = (double)a_[c] * irho;
                const double v = lk - (sq * h[kCa + c] - siq * h[kCb + c]) - gl3 * lk;
                a_[c] = widen(narrow(to_f32_odd(v), a.mode, a.keyL, eL + c));
              }
              for (int k = 0; k < r; ++k) {
                const double uk = rho * (double)u_[k * kLDU];
                const double v = uk - (h[kCc + k] * sg - h[kCe + k] * sp_) - gu3 * uk;
                u_[k * kLDU] = widen(narrow(to_f32_odd(v), a.mode, a.keyU, (unsigned long long)k * N + n));
              }
              a.l3o[i] = (u16)narrow(to_f32_odd(l - gl3 * l), a.mode, a.keyl, (unsigned long long)i);
              a.u3o[i] = (u16)narrow(to_f32_odd(u - gu3 * u), a.mode, a.keyu, (unsigned long long)i);
            }
          }
        }
      }
    } else if (STAGE == kU4 && t < rows) {
      // a head row of tile 0: row t of the new L1 and column t of the new U1, computed by k_corner_upd3
      for (int c = 0; c < r; ++c)
        A[t * g.rp + c] = widen(narrow(a.heads[t * kMaxR + c], a.mode, a.keyL, (unsigned long long)t * r + c));
      for (int k = 0; k < r; ++k)
        Us[k * kLDU + t] =
            widen(narrow(a.heads[kMaxR * kMaxR + k * kMaxR + t], a.mode, a.keyU, (unsigned long long)k * N + t));
    }
    __syncthreads();
    if (kSumL && sp < P) {
      const double s = kUpdate ? irho : 1.0;
      for (int tt = t_lo + sp; tt < rows; tt += P) {
        const double x = (double)A[tt * g.rp + sc] * s;
        acc0 += x * X0[tt];
        if (STAGE == kU2) acc1 += x * X1[tt];
      }
    }
    if (kSumU && sp < P) {
      for (int tt = t_lo + sp; tt < rows; tt += P) acc0 += (rho * (double)Us[sc * kLDU + tt]) * X0[tt];
    }
    if (STAGE == kU4) {
      store_tile(a.L12o, A, g, sl, row0, rows);
      store_cols(a.U12o, Us, r, N, row0, rows);
    }
    __syncthreads();
  }
  if (kSumL || kSumU) {
    if (sp < P) { red[t] = acc0; red[kT + t] = acc1; }     // t = sp * r + sc
    __syncthreads();
    if (t < r) {
      double s0 = 0.0, s1 = 0.0;
      for (int p = 0; p < P; ++p) { s0 += red[p * r + t]; s1 += red[kT + p * r + t]; }
      a.part[(long)blockIdx.x * kPartStride + t] = s0;
      if (STAGE == kU2) a.part[(long)blockIdx.x * kPartStride + r + t] = s1;
    }
  }
  if (STAGE == kU3) {
    double mx[4] = {wave_nmax(mL2), wave_nmax(mL3), wave_nmax(mU2), wave_nmax(mU3)};
    __syncthreads();
    if ((t & 63) == 0)
#pragma unroll
      for (int q = 0; q < 4; ++q) red[q * 4 + (t >> 6)] = mx[q];
    __syncthreads();
    if (t < 4) a.pmax[(long)blockIdx.x * 6 + t] = nmax(nmax(red[t * 4], red[t * 4 + 1]), nmax(red[t * 4 + 2], red[t * 4 + 3]));
  }
}

// ------------------------------------------------------------------ host side
bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

bool overlaps(const void* p, int64_t pb, const void* q, int64_t qb) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return pb > 0 && qb > 0 && a < b + (uintptr_t)qb && b < a + (uintptr_t)pb;
}

int check_common(int64_t N, int r) {
  if (r <= 0) return PSGD_ERR_BAD_ARG;
  if (r > kMaxR) return PSGD_ERR_RANK;
  if (N < r) return PSGD_ERR_BAD_ARG;
  return PSGD_OK;
}

int carve(void* ws, int64_t ws_bytes, Ws& o) {
  if (!ws || ws_bytes < kWsBytes || misaligned(ws, 256)) return PSGD_ERR_WORKSPACE;
  char* b = static_cast<char*>(ws);
  o.hdr = reinterpret_cast<double*>(b + kOffHdr);
  o.heads = reinterpret_cast<float*>(b + kOffHeads);
  o.part = reinterpret_cast<double*>(b + kOffPart);
  o.pmax = reinterpret_cast<double*>(b + kOffPmax);
  return PSGD_OK;
}

int launch_ok() { return hipGetLastError() == hipSuccess ? PSGD_OK : PSGD_ERR_LAUNCH; }

// one block per tile up to the number of blocks a fixed machine of kCUs CUs holds at this LDS footprint
int grid_for(int64_t N, const Geo& g, size_t lds_bytes) {
  int per_cu = (int)((160 * 1024) / (lds_bytes + 512));
  if (per_cu > 4) per_cu = 4;
  if (per_cu < 1) per_cu = 1;
  int64_t blocks = (int64_t)kCUs * per_cu;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  const int64_t ntiles = (N + g.TR - 1) / g.TR;
  return (int)(ntiles < blocks ? ntiles : blocks);
}

template <int STAGE>
int run_sweep(const SweepArgs& a, const Geo& g, int grid, hipStream_t st) {
  if (int rc = set_lds<k_sweep<STAGE>>(kSweepLdsMax)) return rc;
  hipLaunchKernelGGL(k_sweep<STAGE>, dim3(grid), dim3(kT), sweep_lds(g), st, a, g);
  return launch_ok();
}

// the state pointers: all four 16-byte aligned; l3 / u3 may be null when there is no tail (N == r)
int check_state(const void* L12, const void* l3, const void* U12, const void* u3, int64_t N, int r) {
  if (!L12 || !U12) return PSGD_ERR_BAD_ARG;
  if (N > r && (!l3 || !u3)) return PSGD_ERR_BAD_ARG;
  if (misaligned(L12, 16) || misaligned(U12, 16) || misaligned(l3, 16) || misaligned(u3, 16)) return PSGD_ERR_ALIGN;
  return PSGD_OK;
}

int check_apply(const void* L12, const void* l3, const void* U12, const void* u3, const float* g, float* out, int64_t N,
                int r) {
  if (int rc = check_common(N, r)) return rc;
  if (!g || !out || out == g) return PSGD_ERR_BAD_ARG;
  if (int rc = check_state(L12, l3, U12, u3, N, r)) return rc;
  if (misaligned(g, 4) || misaligned(out, 4)) return PSGD_ERR_ALIGN;
  return PSGD_OK;
}

int check_update(const void* L12, const void* l3, const void* U12, const void* u3, const float* dx, const float* dg,
                 const void* L12o, const void* l3o, const void* U12o, const void* u3o, int64_t N, int r, int rounding) {
  if (int rc = check_common(N, r)) return rc;
  if (!dx || !dg) return PSGD_ERR_BAD_ARG;
  if (rounding != 0 && rounding != 1) return PSGD_ERR_BAD_ARG;
  if (int rc = check_state(L12, l3, U12, u3, N, r)) return rc;
  if (int rc = check_state(L12o, l3o, U12o, u3o, N, r)) return rc;
  if (misaligned(dx, 4) || misaligned(dg, 4)) return PSGD_ERR_ALIGN;
  // the update is pure: an output that overlaps an input (or another output) is refused
  const int64_t big = 2 * N * r, small = 2 * (N - r);
  const void* p[8] = {L12, U12, l3, u3, L12o, U12o, l3o, u3o};
  const int64_t nb[8] = {big, big, small, small, big, big, small, small};
  for (int i = 4; i < 8; ++i)
    for (int j = 0; j < i; ++j)
      if (overlaps(p[i], nb[i], p[j], nb[j])) return PSGD_ERR_BAD_ARG;
  return PSGD_OK;
}

}  // namespace

extern "C" {

int64_t psgd_splu_bf16_workspace_bytes(int64_t N, int r) {
  if (int rc = check_common(N, r)) return rc;
  return kWsBytes;
}

int psgd_splu_apply_bf16(const void* L12, const void* l3, const void* U12, const void* u3, const float* g, float* out,
                         int64_t N, int r, void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = check_apply(L12, l3, U12, u3, g, out, N, r)) return rc;
  Ws w;
  if (int rc = carve(ws, ws_bytes, w)) return rc;
  const Geo geo = make_geo(r);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = grid_for(N, geo, sweep_lds(geo));
  const u16 *Lq = static_cast<const u16*>(L12), *Uq = static_cast<const u16*>(U12);
  SweepArgs a{};
  a.L12 = Lq; a.l3 = static_cast<const u16*>(l3); a.U12 = Uq; a.u3 = static_cast<const u16*>(u3);
  a.x = g; a.out = out; a.N = (long)N; a.hdr = w.hdr; a.heads = w.heads; a.part = w.part; a.pmax = w.pmax;
  hipLaunchKernelGGL(k_rho, dim3(1), dim3(64), 0, st, Lq, Uq, (long)N, r, w.pmax, 0, 0, w.hdr);
  if (int rc = run_sweep<kDot>(a, geo, grid, st)) return rc;
  hipLaunchKernelGGL(k_corner1, dim3(1), dim3(64), 0, st, Lq, Uq, (long)N, r, g, (const float*)nullptr, w.part, grid, w.hdr);
  if (int rc = run_sweep<kA2>(a, geo, grid, st)) return rc;
  hipLaunchKernelGGL(k_corner_apply2, dim3(1), dim3(64), 0, st, Lq, Uq, (long)N, r, w.part, grid, w.hdr, out);
  return run_sweep<kA3>(a, geo, grid, st);
}

int psgd_splu_update_bf16(const void* L12, const void* l3, const void* U12, const void* u3, const float* dx, const float* dg,
                          void* L12_new, void* l3_new, void* U12_new, void* u3_new, int64_t N, int r, float step, float tiny,
                          int rounding, uint64_t seed, void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = check_update(L12, l3, U12, u3, dx, dg, L12_new, l3_new, U12_new, u3_new, N, r, rounding)) return rc;
  Ws w;
  if (int rc = carve(ws, ws_bytes, w)) return rc;
  const Geo geo = make_geo(r);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = grid_for(N, geo, sweep_lds(geo));
  const u16 *Lq = static_cast<const u16*>(L12), *Uq = static_cast<const u16*>(U12);
  const u16 *lq = static_cast<const u16*>(l3), *uq = static_cast<const u16*>(u3);
  SweepArgs a{};
  a.L12 = Lq; a.l3 = lq; a.U12 = Uq; a.u3 = uq;
  a.x = dg; a.dx = dx; a.N = (long)N; a.hdr = w.hdr; a.heads = w.heads; a.part = w.part; a.pmax = w.pmax;
  a.L12o = static_cast<u16*>(L12_new); a.l3o = static_cast<u16*>(l3_new);
  a.U12o = static_cast<u16*>(U12_new); a.u3o = static_cast<u16*>(u3_new);
  a.mode = rounding;
  a.keyL = make_key(seed, kIdL12); a.keyl = make_key(seed, kIdl3); a.keyU = make_key(seed, kIdU12); a.keyu = make_key(seed, kIdu3);
  const int64_t n2 = N - r;
  int mgrid = 0;
  if (n2 > 0) {
    const int64_t want = ((n2 + 7) / 8 + kT - 1) / kT;
    mgrid = (int)(want < kMaxBlocks ? want : kMaxBlocks);
    hipLaunchKernelGGL(k_tailmax, dim3(mgrid), dim3(kT), 0, st, lq, uq, (long)n2, w.pmax);
  }
  hipLaunchKernelGGL(k_rho, dim3(1), dim3(64), 0, st, Lq, Uq, (long)N, r, w.pmax, mgrid, 1, w.hdr);
  if (int rc = run_sweep<kDot>(a, geo, grid, st)) return rc;
  hipLaunchKernelGGL(k_corner1, dim3(1), dim3(64), 0, st, Lq, Uq, (long)N, r, dg, dx, w.part, grid, w.hdr);
  if (int rc = run_sweep<kU2>(a, geo, grid, st)) return rc;
  hipLaunchKernelGGL(k_corner_upd2, dim3(1), dim3(64), 0, st, Lq, Uq, (long)N, r, w.part, grid, w.hdr);
  if (int rc = run_sweep<kU3>(a, geo, grid, st)) return rc;
  hipLaunchKernelGGL(k_corner_upd3, dim3(1), dim3(64), 0, st, Lq, Uq, (long)N, r, dx, dg, step, tiny, w.part, w.pmax, grid,
                     w.hdr, w.heads);
  return run_sweep<kU4>(a, geo, grid, st);
}

}  // extern "C"
