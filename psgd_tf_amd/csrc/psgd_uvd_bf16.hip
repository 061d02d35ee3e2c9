// psgd_uvd_bf16.hip -- the UVd preconditioner (psgd.py:527-627) on a state whose HBM image is bf16.
//
// U, V ([N, r] row-major) and d ([N]) are stored as bf16; v, h, g and the output are fp32.  All arithmetic is fp32 (fp64
// for the block partial sums, the r x r algebra and every fold): a tile is widened on its way into LDS and narrowed once
// when it is written back.  One kernel family for ranks 1 .. 32 with the rank as a run-time value:
//
//   * A tile is a contiguous span of TR rows (TR * r is a multiple of 8), copied with 16-byte loads (8 bf16) whatever the
//     rank: a row is 2 r bytes, so no load is ever issued per row.  The S = r * m active threads of a block each own chunk
//     t, t + S, ... of the span; 8 S elements are a whole number of rows, so the column of each of a thread's 8 slots and
//     its row offset never change and the LDS address of a slot is one add (no division in the loop).
//   * In LDS a tile is fp32 with an odd row stride (r | 1): one thread per row reads its row without bank conflicts, the
//     r-vectors of the call come through the scalar cache.
//   * Column sums (the Gram of [U | V | t | w], V'x, U'x) run on v_mfma_f32_16x16x32_bf16.  U and V are exact bf16 values:
//     one pass; the derived fp32 columns are split into three bf16 pieces (x = h + m + l exactly).
//   * Reductions have a fixed order (tile -> wave -> block -> fold over blocks); no float atomics.  Grids are sized by the
//     LDS footprint on a fixed CU count, so results do not depend on the device either.
//   * Narrowing: round to nearest even, or stochastic: (bits + u) >> 16 with u from a counter hash of (seed, tensor, flat
//     element index) -- independent of grid, tile order and wave.
//
// The stored state is what the apply must see, so the fused update -> apply does NOT use the algebraic short cut of the
// fp32 path (its reductions are linear in the unrounded d and factor): it is the update's sweeps followed by the apply's,
// with the d update folded into the apply's first sweep -- five sweeps, about (8r + 4) * 2 + 52 bytes per parameter.
//
// Row-sharded state (one process per GPU, psgd_tf_amd/sharded.py): every sweep already ends in a small fold kernel, so the
// staged entry points stop there, leave this rank's contribution as fp64 in a send region of the workspace
// (psgd_uvd_bf16_ws_region) and psgd_uvd_bf16_fold_gathered_f64 folds the all-gathered copies in rank order into exactly
// what the next kernel of the one-call sequence reads.  Exchanges per call -- one more on the balance branch (stage 10):
//     apply 2 (stages 1, 2)      update 2 (11, 12)      fused update -> apply 4 (11, 12, 1, 2)
// Four, not the two of the fp32 family: its short cut derives the apply's reductions from sums over the UNROUNDED d and
// factor, and here the apply must see the stored codes.  The stochastic-rounding stream of a shard is keyed by the GLOBAL
// element index (row0 + row), so ranks never round their rows with the same random numbers and the stored state does not
// depend on how the rows are split.
//
// psgd_uvd_bf16_narrow_f32 (k_narrow_f32) brings fp32 values into this stored form with the same narrow() and the same
// global-index stream: what loading an fp32 checkpoint into a bf16 state runs, chunk by chunk, with no workspace.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16_state.h"
#include "nanmax.h"
#include "psgd_hip.h"

namespace {

using psgd::amaxf;
using namespace psgd::bf16s;   // widen / narrow / keys / split3 / tile copies: bf16_state.h (shared with psgd_splu_bf16.hip)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxBlocks = 2048;   // cap of every sweep grid (sized by LDS, at most 6 blocks on each of 256 CUs)
constexpr int kGramBlocks = 512;   // the Gram sweep: two blocks per CU (its fp64 block partials are 30 KB each)
constexpr int kCUs = 256;          // grids are a property of the kernel family, not of the device: results do not depend on it
constexpr int kMaxR = 32;
constexpr int kGS = 80;            // row stride of the folded Gram (2r + 6 <= 70 columns)
constexpr int kPairs = 15;         // block pairs bi <= bj of 5 column blocks

// workspace layout (bytes)
constexpr int64_t kOffHdr = 0;                                    // float[1024]
constexpr int64_t kOffG = 4096;                                   // double[80 * 80]
constexpr int64_t kOffMax = kOffG + kGS * kGS * 8;                // float[2 * kMaxBlocks]
constexpr int64_t kOffVec = kOffMax + 2 * kMaxBlocks * 4;         // double[kMaxBlocks * 32]
constexpr int64_t kOffGram = kOffVec + kMaxBlocks * 32 * 8;       // double[kGramBlocks * kPairs * 256]
constexpr int64_t kOffNabla = kOffGram + (int64_t)kGramBlocks * kPairs * 256 * 8;   // float[N]
// fp64 send regions of the staged entry points, in the unused tail of the header (floats 320 .. 1023 are free)
constexpr int64_t kOffSend10 = 2048;   // double[2]: max|U|, max|V|
constexpr int64_t kOffSend12 = 2064;   // double[1]: max|nablaD|
constexpr int64_t kOffSend1 = 2304;    // double[32]: V'(d .* g)
constexpr int64_t kOffSend2 = 2560;    // double[32]: U'g1
// header floats
constexpr int kHScaleU = 0, kHScaleV = 1, kHMuD = 2, kHCo = 8, kHS1 = 256, kHS2 = 288;
// coefficient r-vectors inside the header (32 floats each, from kHCo)
constexpr int kCoAl = 0, kCoBe = 32, kCoGa = 64, kCoDe = 96, kCoC1 = 128, kCoC2 = 160, kCoMu = 192;

// MFMA fragment: rows row0 .. row0 + 7 of one column (stride apart), zero outside the tile / the matrix
__device__ __forceinline__ bf16x8 gather8(const float* col, int stride, bool valid, int row0, int rows) {
  u32x4 p;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r0 = row0 + 2 * q;
    const unsigned x0 = (valid && r0 < rows) ? __float_as_uint(col[r0 * stride]) : 0u;
    const unsigned x1 = (valid && r0 + 1 < rows) ? __float_as_uint(col[(r0 + 1) * stride]) : 0u;
    p[q] = (x0 >> 16) | (x1 & 0xffff0000u);
  }
  return __builtin_bit_cast(bf16x8, p);
}

__device__ __forceinline__ float block_amax(float x, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = amaxf(x, __shfl_xor(x, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  return amaxf(amaxf(red[0], red[1]), amaxf(red[2], red[3]));
}

// ------------------------------------------------------------------ balance (psgd.py:562-567)
__global__ __launch_bounds__(kT) void k_bmax(const u16* __restrict__ U, const u16* __restrict__ V, long total,
                                              float* maxpart) {
  __shared__ float red[4];
  float mu = 0.f, mv = 0.f;
  const long nch = (total + 7) / 8;
  for (long c = (long)blockIdx.x * kT + threadIdx.x; c < nch; c += (long)gridDim.x * kT) {
    const long e0 = 8 * c;
    if (e0 + 8 <= total) {
      const u32x4 a = *reinterpret_cast<const u32x4*>(U + e0), b = *reinterpret_cast<const u32x4*>(V + e0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        mu = amaxf(mu, fabsf(widen(a[q] & 0xffffu))); mu = amaxf(mu, fabsf(widen(a[q] >> 16)));
        mv = amaxf(mv, fabsf(widen(b[q] & 0xffffu))); mv = amaxf(mv, fabsf(widen(b[q] >> 16)));
      }
    } else {
      for (long e = e0; e < total; ++e) {
        mu = amaxf(mu, fabsf(widen(U[e])));
        mv = amaxf(mv, fabsf(widen(V[e])));
      }
    }
  }
  mu = block_amax(mu, red);
  mv = block_amax(mv, red);
  if (threadIdx.x == 0) { maxpart[2 * blockIdx.x] = mu; maxpart[2 * blockIdx.x + 1] = mv; }
}

// scales of the call: U <- U * su, V <- V * sv (1, 1 without the balance branch)
__global__ void k_scales(const float* maxpart, int nblk, int balance, float* hdr) {
  if (threadIdx.x != 0) return;
  float su = 1.f, sv = 1.f;
  if (balance) {
    float mu = 0.f, mv = 0.f;
    for (int b = 0; b < nblk; ++b) { mu = amaxf(mu, maxpart[2 * b]); mv = amaxf(mv, maxpart[2 * b + 1]); }
    const float rho = sqrtf(mu / mv);
    su = 1.0f / rho;
    sv = rho;
  }
  hdr[kHScaleU] = su;
  hdr[kHScaleV] = sv;
}

// ------------------------------------------------------------------ update sweep 1: Gram of [U | V | t3 | w3]
// NB = column blocks of 16 in use (2r + 6 columns): the accumulators of unused block pairs do not exist
template <int NB>
__global__ __launch_bounds__(kT, 2) void k_gram(const u16* __restrict__ U, const u16* __restrict__ V,
                                                 const u16* __restrict__ d, const float* __restrict__ v,
                                                 const float* __restrict__ h, long N, Geo g, double* part) {
  constexpr int nb = NB;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* A = lds;
  float* B = A + kT * g.rp;
  float* X = B + kT * g.rp;   // [kT][7]: t (3 pieces), w (3 pieces)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const Slots sl = make_slots(g);

  const float* cbase[5];
  int cstride[5];
  bool cvalid[5];
#pragma unroll
  for (int b = 0; b < 5; ++b) {
    const int col = 16 * b + (lane & 15);
    cvalid[b] = true;
    if (col < g.r) { cbase[b] = A + col; cstride[b] = g.rp; }
    else if (col < 2 * g.r) { cbase[b] = B + (col - g.r); cstride[b] = g.rp; }
    else if (col < 2 * g.r + 6) { cbase[b] = X + (col - 2 * g.r); cstride[b] = 7; }
    else { cbase[b] = A; cstride[b] = 0; cvalid[b] = false; }
  }

  // fp32 MFMA chains are at most kFlushTiles tiles long (<= 64 slabs of 32 rows per wave); then the waves park their
  // accumulators in LDS (the tile is free at that point) and the block adds them, wave 0 .. 3 in order, into its fp64 partial in
  // the workspace (<= 30 KB, L2-resident) -- the same for every rank.  Pairs are stored compactly: only those with bj < nb.
  constexpr int kFlushTiles = 32;
  constexpr int kUsed = NB * (NB + 1) / 2;
  f32x4 acc[kPairs];
#pragma unroll
  for (int p = 0; p < kPairs; ++p) acc[p] = f32x4{0.f, 0.f, 0.f, 0.f};
  double* out = part + (long)blockIdx.x * kPairs * 256;
  bool first = true;
  auto flush = [&]() {   // called by the whole block, after a barrier
    float* S = lds + w * (kUsed * 256) + lane * 4;
    int p = 0, pc = 0;
#pragma unroll
    for (int bi = 0; bi < 5; ++bi)
#pragma unroll
      for (int bj = bi; bj < 5; ++bj) {
        if (bj < nb) {
          *reinterpret_cast<f32x4*>(S + pc * 256) = acc[p];
          acc[p] = f32x4{0.f, 0.f, 0.f, 0.f};
          ++pc;
        }
        ++p;
      }
    __syncthreads();
#pragma unroll 1
    for (int i = threadIdx.x; i < kUsed * 256; i += kT) {
      double s = first ? 0.0 : out[i];
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) s += (double)lds[ww * (kUsed * 256) + i];
      out[i] = s;
    }
    __syncthreads();
    first = false;
  };
  int tiles_done = 0;

  const long ntiles = (N + g.TR - 1) / g.TR;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long row0 = tile * g.TR;
    const int rows = (int)((N - row0 < g.TR) ? (N - row0) : g.TR);
    load_tile(U, A, g, sl, row0, rows, 1.0f);
    load_tile(V, B, g, sl, row0, rows, 1.0f);
    if ((int)threadIdx.x < rows) {
      const long row = row0 + threadIdx.x;
      const float dd = widen(d[row]);
      const float t = dd * h[row], ww = v[row] / dd;
      float* x = X + threadIdx.x * 7;
      split3(t, x[0], x[1], x[2]);
      split3(ww, x[3], x[4], x[5]);
    }
    __syncthreads();
    const int nslab = (rows + 31) >> 5;
    for (int s = w; s < nslab; s += 4) {
      const int r0 = 32 * s + 8 * (lane >> 4);
      bf16x8 f[5];
#pragma unroll
      for (int b = 0; b < 5; ++b)
        if (b < nb) f[b] = gather8(cbase[b], cstride[b], cvalid[b], r0, rows);
        else f[b] = f[0];
      int p = 0;
#pragma unroll
      for (int bi = 0; bi < 5; ++bi)
#pragma unroll
        for (int bj = bi; bj < 5; ++bj) {
          if (bj < nb) acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[bi], f[bj], acc[p], 0, 0, 0);
          ++p;
        }
    }
    __syncthreads();
    if (++tiles_done == kFlushTiles) {
      flush();
      tiles_done = 0;
    }
  }
  flush();
}

// fold the block partials in block order into the symmetric [kGS][kGS] Gram
__global__ __launch_bounds__(kT) void k_gram_fold(const double* part, int nblk, int nb, double* G) {
  const int q = blockIdx.x;   // pair index
  int bi = 0, bj = 0, p = 0, pc = 0, qc = 0;
  for (int a = 0; a < 5; ++a)
    for (int b = a; b < 5; ++b) {
      if (p == q) { bi = a; bj = b; qc = pc; }
      if (b < nb) ++pc;     // the Gram sweep stores the pairs in use compactly
      ++p;
    }
  if (bj >= nb) return;
  const int x = threadIdx.x;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[((long)b * kPairs + qc) * 256 + x];
  const int l = x >> 2, e = x & 3;
  const int i = 16 * bi + 4 * (l >> 4) + e, j = 16 * bj + (l & 15);
  G[i * kGS + j] = s;
  if (bi != bj) G[j * kGS + i] = s;
}

// the r x r algebra of psgd.py:569-615 in fp64, one wave; writes the fp32 r-vectors the rewrite sweep needs
__global__ __launch_bounds__(64) void k_small(const double* __restrict__ G, int r, float step, float tiny, int update_U,
                                               float* hdr) {
  __shared__ double Mx[kMaxR][2 * kMaxR + 1];
  __shared__ double al[kMaxR], be[kMaxR], ga[kMaxR], de[kMaxR], Ut[kMaxR], Vt[kMaxR], Uw[kMaxR], Vw[kMaxR], Vb[kMaxR],
      e1[kMaxR], pv[kMaxR], t1[kMaxR], t2[kMaxR];
  const int i = threadIdx.x;
  const double su = (double)hdr[kHScaleU], sv = (double)hdr[kHScaleV];
  auto UU = [&](int a, int b) { return G[a * kGS + b] * su * su; };
  auto VV = [&](int a, int b) { return G[(r + a) * kGS + r + b] * sv * sv; };
  auto VU = [&](int a, int b) { return G[(r + a) * kGS + b] * su * sv; };   // (V'U)[a][b]
  const int ct = 2 * r, cw = 2 * r + 3;
  if (i < r) {
    double a = 0, b = 0, c = 0, e = 0;
    for (int p = 0; p < 3; ++p) {
      a += G[i * kGS + ct + p];
      b += G[(r + i) * kGS + ct + p];
      c += G[i * kGS + cw + p];
      e += G[(r + i) * kGS + cw + p];
    }
    Ut[i] = su * a; Vt[i] = sv * b; Uw[i] = su * c; Vw[i] = sv * e;
    al[i] = sv * b;
    for (int j = 0; j < r; ++j) {
      Mx[i][j] = (i == j ? 1.0 : 0.0) + VU(i, j);
      Mx[i][r + j] = (i == j ? 1.0 : 0.0);
    }
  }
  double tt = 0, ww = 0, tw = 0;
  for (int p = 0; p < 3; ++p)
    for (int q = 0; q < 3; ++q) {
      tt += G[(ct + p) * kGS + ct + q];
      ww += G[(cw + p) * kGS + cw + q];
      tw += G[(ct + p) * kGS + cw + q];
    }
  __syncthreads();
  // Gauss-Jordan with partial pivoting on [I + V'U | I]
  for (int k = 0; k < r; ++k) {
    int piv = k;
    double best = fabs(Mx[k][k]);
    for (int a = k + 1; a < r; ++a) {
      const double x = fabs(Mx[a][k]);
      if (x > best) { best = x; piv = a; }
    }
    __syncthreads();
    if (piv != k && i < 2 * r) {
      const double x = Mx[k][i];
      Mx[k][i] = Mx[piv][i];
      Mx[piv][i] = x;
    }
    __syncthreads();
    const double inv = 1.0 / Mx[k][k];
    const double f = (i < r) ? Mx[i][k] : 0.0;
    __syncthreads();
    if (i < 2 * r) Mx[k][i] *= inv;
    __syncthreads();
    if (i < r && i != k)
      for (int j = 0; j < 2 * r; ++j) Mx[i][j] -= f * Mx[k][j];
    __syncthreads();
  }
  if (i < r) {
    double s = Ut[i], g2 = 0;
    for (int j = 0; j < r; ++j) { s += UU(i, j) * al[j]; g2 += Mx[j][r + i] * Uw[j]; }
    be[i] = s;
    ga[i] = g2;
  }
  __syncthreads();
  if (i < r) {
    double s = Vw[i], e = 0;
    for (int j = 0; j < r; ++j) { s -= VV(i, j) * ga[j]; e += VU(j, i) * ga[j]; }
    Vb[i] = s;
    e1[i] = e;
  }
  __syncthreads();
  if (i < r) {
    double s = 0;
    for (int j = 0; j < r; ++j) s += Mx[i][r + j] * Vb[j];
    de[i] = s;
  }
  double aa = tt, bb = ww, ab = tw;
  for (int j = 0; j < r; ++j) {
    aa += 2.0 * al[j] * Ut[j] + al[j] * (be[j] - Ut[j]);
    bb += -2.0 * ga[j] * Vw[j] + ga[j] * (Vw[j] - Vb[j]);
    ab += -ga[j] * Vt[j] + al[j] * Uw[j] - al[j] * e1[j];
  }
  float* co = hdr + kHCo;
  if (update_U) {
    // p = V'a, q = V'b; U <- U - mu (a p'M - b q'M), M = I + V'U  (psgd.py:589-601)
    if (i < r) {
      double s = Vt[i];
      for (int j = 0; j < r; ++j) s += VU(i, j) * al[j];
      pv[i] = s;
    }
    __syncthreads();
    if (i < r) {
      double a = 0, b = 0;
      for (int j = 0; j < r; ++j) { a += VV(i, j) * pv[j]; b += VV(i, j) * Vb[j]; }
      t1[i] = a; t2[i] = b;
    }
    __syncthreads();
    double pp = 0, qq = 0, pq = 0;
    for (int j = 0; j < r; ++j) { pp += pv[j] * t1[j]; qq += Vb[j] * t2[j]; pq += pv[j] * t2[j]; }
    const double mu = (double)step / (sqrt(fabs(aa * pp + bb * qq - 2.0 * ab * pq)) + (double)tiny);
    if (i < r) {
      double c1 = pv[i], c2 = Vb[i];
      for (int j = 0; j < r; ++j) { c1 += pv[j] * VU(j, i); c2 += Vb[j] * VU(j, i); }
      co[kCoC1 + i] = (float)(mu * c1);
      co[kCoC2 + i] = (float)(mu * c2);
    }
    if (i == 0) co[kCoMu] = (float)mu;
  } else {
    // beta = U'a, eps = U'b; V <- V - mu ((a + V beta) beta' - (b + V eps) eps')  (psgd.py:603-615)
    if (i < r) pv[i] = Uw[i] - e1[i];
    __syncthreads();
    if (i < r) {
      double a = 0, b = 0;
      for (int j = 0; j < r; ++j) { a += UU(i, j) * be[j]; b += UU(i, j) * pv[j]; }
      t1[i] = a; t2[i] = b;
    }
    __syncthreads();
    double b2 = 0, e2 = 0, bx = 0;
    for (int j = 0; j < r; ++j) { b2 += be[j] * t1[j]; e2 += pv[j] * t2[j]; bx += be[j] * t2[j]; }
    const double mu = (double)step / (sqrt(fabs(b2 * aa + e2 * bb - 2.0 * bx * ab)) + (double)tiny);
    if (i < r) {
      co[kCoC1 + i] = (float)be[i];
      co[kCoC2 + i] = (float)pv[i];
    }
    if (i == 0) co[kCoMu] = (float)mu;
  }
  if (i < r) {
    co[kCoAl + i] = (float)al[i];
    co[kCoBe + i] = (float)be[i];
    co[kCoGa + i] = (float)ga[i];
    co[kCoDe + i] = (float)de[i];
  }
}

// ------------------------------------------------------------------ update sweep 2: nablaD, its maximum, the factor rewrite
__global__ __launch_bounds__(kT, 2) void k_rewrite(u16* __restrict__ U, u16* __restrict__ V, const u16* __restrict__ d,
                                                    const float* __restrict__ v, const float* __restrict__ h, long N, Geo g,
                                                    const float* __restrict__ hdr, int update_U, int write_both, int mode,
                                                    SrKey keyU, SrKey keyV, long grow0, float* __restrict__ nabla,
                                                    float* maxpart) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float red[4];
  float* A = lds;
  float* B = A + kT * g.rp;
  const Slots sl = make_slots(g);
  const float su = hdr[kHScaleU], sv = hdr[kHScaleV];
  const float* co = hdr + kHCo;
  const float mu = co[kCoMu];
  const int r = g.r;
  float lmax = 0.f;
  const long ntiles = (N + g.TR - 1) / g.TR;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long row0 = tile * g.TR;
    const int rows = (int)((N - row0 < g.TR) ? (N - row0) : g.TR);
    load_tile(U, A, g, sl, row0, rows, su);
    load_tile(V, B, g, sl, row0, rows, sv);
    __syncthreads();
    if ((int)threadIdx.x < rows) {
      const long row = row0 + threadIdx.x;
      float* a_ = A + threadIdx.x * g.rp;
      float* b_ = B + threadIdx.x * g.rp;
      const float dd = widen(d[row]), hh = h[row], vv = v[row];
      const float t = dd * hh, w = vv / dd;
      float ua = 0.f, ud = 0.f, vbe = 0.f, vg = 0.f, ve = 0.f;
#pragma unroll 4
      for (int k = 0; k < r; ++k) {
        const float x = a_[k], y = b_[k];
        ua = fmaf(x, co[kCoAl + k], ua);
        ud = fmaf(x, co[kCoDe + k], ud);
        vbe = fmaf(y, co[kCoBe + k], vbe);
        vg = fmaf(y, co[kCoGa + k], vg);
        ve = fmaf(y, co[kCoC2 + k], ve);   // V eps (update_V only)
      }
      const float a = t + ua, b = w - vg;                    // Qh, invQtv (psgd.py:569, :577)
      const float Ph = dd * (a + vbe);                       // :570
      const float invPv = (b - ud) / dd;                     // :578-579
      const float nab = Ph * hh - vv * invPv;                // :581
      nabla[row] = nab;
      lmax = amaxf(lmax, fabsf(nab));
      const unsigned long long e0 = (unsigned long long)(grow0 + row) * (unsigned)r;   // grow0: first row of a shard
      if (update_U) {
#pragma unroll 4
        for (int k = 0; k < r; ++k) {
          const float x = a_[k] - (a * co[kCoC1 + k] - b * co[kCoC2 + k]);
          a_[k] = widen(narrow(x, mode, keyU, e0 + k));
        }
        if (write_both)
          for (int k = 0; k < r; ++k) b_[k] = widen(narrow(b_[k], mode, keyV, e0 + k));
      } else {
        const float fa = mu * (a + vbe), fb = mu * (b + ve);
#pragma unroll 4
        for (int k = 0; k < r; ++k) {
          const float x = b_[k] - (fa * co[kCoC1 + k] - fb * co[kCoC2 + k]);
          b_[k] = widen(narrow(x, mode, keyV, e0 + k));
        }
        if (write_both)
          for (int k = 0; k < r; ++k) a_[k] = widen(narrow(a_[k], mode, keyU, e0 + k));
      }
    }
    __syncthreads();
    if (update_U || write_both) store_tile(U, A, g, sl, row0, rows);
    if (!update_U || write_both) store_tile(V, B, g, sl, row0, rows);
    __syncthreads();
  }
  lmax = block_amax(lmax, red);
  if (threadIdx.x == 0) maxpart[blockIdx.x] = lmax;
}

// mu_d = step / (max |nablaD| + tiny)   (psgd.py:582)
__device__ __forceinline__ float wave_fold_max(const float* maxpart, int nblk) {
  float m = 0.f;
  for (int b = threadIdx.x; b < nblk; b += 64) m = amaxf(m, maxpart[b]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = amaxf(m, __shfl_xor(m, o));
  return m;
}

__global__ __launch_bounds__(64) void k_mu_d(const float* maxpart, int nblk, float step, float tiny, float* hdr) {
  const float m = wave_fold_max(maxpart, nblk);
  if (threadIdx.x == 0) hdr[kHMuD] = step / (m + tiny);
}

// staged form: this rank's max |nablaD|, as the double it is sent as
__global__ __launch_bounds__(64) void k_max_fold(const float* maxpart, int nblk, double* send) {
  const float m = wave_fold_max(maxpart, nblk);
  if (threadIdx.x == 0) send[0] = (double)m;
}

// staged form of the fold inside k_scales (the same order): this rank's max|U|, max|V|
__global__ void k_bmax_fold(const float* maxpart, int nblk, double* send) {
  if (threadIdx.x != 0) return;
  float mu = 0.f, mv = 0.f;
  for (int b = 0; b < nblk; ++b) { mu = amaxf(mu, maxpart[2 * b]); mv = amaxf(mv, maxpart[2 * b + 1]); }
  send[0] = (double)mu;
  send[1] = (double)mv;
}

// Exchange, second half: `gathered` = the send regions of all ranks, [world][count] doubles in rank order.  Every rank
// folds them in that order (is_max: NaN-propagating maximum, else +), so all ranks hold the same bits.  dst: the fp64
// region itself; fdst (optional): the fp32 words the next kernel reads.  ncols > 0: dst is the [.][kGS] Gram and only its
// first ncols columns are in use (the rest is never written by k_gram_fold and never read by k_small).
__global__ void k_fold_gathered_b(const double* __restrict__ gathered, int world, int count, int is_max, int ncols,
                                  double* __restrict__ dst, float* __restrict__ fdst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  if (ncols > 0 && i % kGS >= ncols) return;
  double a = gathered[i];
  if (is_max) {
    for (int k = 1; k < world; ++k) a = psgd::nmax(a, gathered[(long)k * count + i]);
  } else {
    for (int k = 1; k < world; ++k) a += gathered[(long)k * count + i];
  }
  dst[i] = a;
  if (fdst) fdst[i] = (float)a;
}

// d <- d - mu_d d nablaD   (psgd.py:584), on its own (the update without the apply)
__global__ __launch_bounds__(kT) void k_d_update(u16* __restrict__ d, const float* __restrict__ nabla, long N,
                                                  const float* __restrict__ hdr, int mode, SrKey keyD, long grow0) {
  const float mu = hdr[kHMuD];
  for (long i = (long)blockIdx.x * kT + threadIdx.x; i < N; i += (long)gridDim.x * kT) {
    const float dd = widen(d[i]);
    d[i] = (u16)narrow(dd - mu * dd * nabla[i], mode, keyD, (unsigned long long)(grow0 + i));
  }
}

// ------------------------------------------------------------------ fp32 -> stored bf16 (loading an fp32 checkpoint)
// dst[i] = narrow(src[i]) for i < count, the rounding index of element i being idx0 + i (its flat GLOBAL index in the tensor the
// key belongs to: the codes depend on neither how the caller chunks the copy nor the row split).  HBM-bound streaming, the shape
// of psgd_uvd_tail.hip: a scalar head brings dst to a 16-byte boundary, the body stores 16 bytes (8 codes) per lane from two
// 16-byte loads, a scalar tail finishes.  src is read through a vector type whose declared alignment is the element's, so an
// odd idx0 or an src that starts at any fp32 element still takes wide loads.
typedef float f32x4_e __attribute__((ext_vector_type(4), aligned(4)));       // 16 bytes from any fp32 element
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

__global__ __launch_bounds__(kT) void k_narrow_f32(const float* __restrict__ src, u16* __restrict__ dst, long count, int mode,
                                                   SrKey key, unsigned long long idx0) {
  long head = (long)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) / 2u);
  if (head > count) head = count;
  const long nvec = (count - head) / 8;
  const long tid = (long)blockIdx.x * kT + threadIdx.x;
  const long nthr = (long)gridDim.x * kT;
  if (tid < head) dst[tid] = (u16)narrow(src[tid], mode, key, idx0 + (unsigned long long)tid);
#pragma unroll 2
  for (long q = tid; q < nvec; q += nthr) {
    const long i = head + q * 8;
    const f32x4_e a = *reinterpret_cast<const f32x4_e*>(src + i);
    const f32x4_e b = *reinterpret_cast<const f32x4_e*>(src + i + 4);
    const unsigned long long e0 = idx0 + (unsigned long long)i;
    u16x8 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = (u16)narrow(a[e], mode, key, e0 + e);
      v[e + 4] = (u16)narrow(b[e], mode, key, e0 + 4 + e);
    }
    *reinterpret_cast<u16x8*>(dst + i) = v;
  }
  const long i = head + nvec * 8 + tid;
  if (i < count) dst[i] = (u16)narrow(src[i], mode, key, idx0 + (unsigned long long)i);
}

// ------------------------------------------------------------------ the three sweeps of the apply (psgd.py:619-627)
// MODE 0: s1 = M'(d .* g)                                   (M = V)
// MODE 1: the same after d <- d - mu_d d nablaD (written)   (M = V; the fused call)
// MODE 2: g1 = d .* g + M s1 -> out, s2 = M' g1             (M = U)
// MODE 3: out = d .* (out + M s2)                           (M = V)
template <int MODE>
__global__ __launch_bounds__(kT, 2) void k_apply(const u16* __restrict__ M, u16* d, const float* __restrict__ g, float* out,
                                                  long N, Geo geo, const float* __restrict__ hdr,
                                                  const float* __restrict__ nabla, int mode, SrKey keyD, long grow0,
                                                  double* vecpart) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* A = lds;
  float* X = A + kT * geo.rp;   // [kT][4]: three pieces of the reduced column
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const Slots sl = make_slots(geo);
  const int r = geo.r;
  const float* sv = hdr + (MODE == 2 ? kHS1 : kHS2);
  const float mu_d = (MODE == 1) ? hdr[kHMuD] : 0.f;

  const float* cbase[3];
  int cstride[3];
  bool cvalid[3];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int col = 16 * b + (lane & 15);
    cbase[b] = A + col; cstride[b] = geo.rp; cvalid[b] = col < r;
  }
  cbase[2] = X + (lane & 15); cstride[2] = 4; cvalid[2] = (lane & 15) < 3;
  const int nbA = (r + 15) >> 4;

  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  double acc64[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  int since = 0;

  const long ntiles = (N + geo.TR - 1) / geo.TR;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long row0 = tile * geo.TR;
    const int rows = (int)((N - row0 < geo.TR) ? (N - row0) : geo.TR);
    load_tile(M, A, geo, sl, row0, rows, 1.0f);
    if (MODE >= 2) __syncthreads();
    if ((int)threadIdx.x < rows) {
      const long row = row0 + threadIdx.x;
      float dd = widen(d[row]);
      float x;
      if (MODE == 1) {
        const unsigned code = narrow(dd - mu_d * dd * nabla[row], mode, keyD, (unsigned long long)(grow0 + row));
        d[row] = (u16)code;
        dd = widen(code);
      }
      if (MODE <= 1) {
        x = dd * g[row];
      } else {
        const float* a_ = A + threadIdx.x * geo.rp;
        float s = 0.f;
#pragma unroll 4
        for (int k = 0; k < r; ++k) s = fmaf(a_[k], sv[k], s);
        if (MODE == 2) {
          x = dd * g[row] + s;
          out[row] = x;
        } else {
          out[row] = dd * (out[row] + s);
        }
      }
      if (MODE != 3) {
        float* xx = X + threadIdx.x * 4;
        split3(x, xx[0], xx[1], xx[2]);
      }
    }
    __syncthreads();
    if (MODE != 3) {
      const int nslab = (rows + 31) >> 5;
      for (int s = w; s < nslab; s += 4) {
        const int r0 = 32 * s + 8 * (lane >> 4);
        const bf16x8 fb = gather8(cbase[2], cstride[2], cvalid[2], r0, rows);
#pragma unroll
        for (int b = 0; b < 2; ++b)
          if (b < nbA) {
            const bf16x8 fa = gather8(cbase[b], cstride[b], cvalid[b], r0, rows);
            acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[b], 0, 0, 0);
          }
        if (++since == 8) {
#pragma unroll
          for (int b = 0; b < 2; ++b) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc64[b][e] += (double)acc[b][e];
            acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
          since = 0;
        }
      }
      __syncthreads();
    }
  }
  if (MODE != 3) {
    // D[i][j]: lane holds j = lane % 16 (piece, < 3), i = 4 (lane / 16) + e (column of M within its block)
    double* Sc = reinterpret_cast<double*>(lds);   // [4 waves][32 columns][3 pieces]
    if ((lane & 15) < 3) {
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          Sc[(w * 32 + 16 * b + 4 * (lane >> 4) + e) * 3 + (lane & 15)] = acc64[b][e] + (double)acc[b][e];
    }
    __syncthreads();
    if ((int)threadIdx.x < r) {
      double s = 0.0;
      for (int ww = 0; ww < 4; ++ww)
        for (int p = 0; p < 3; ++p) s += Sc[(ww * 32 + threadIdx.x) * 3 + p];
      vecpart[(long)blockIdx.x * 32 + threadIdx.x] = s;
    }
  }
}

// eight interleaved partial folds per column, then their sum: a fixed order.  dst64 (staged form): the sums stay fp64,
// this rank's contribution to the exchange; the fold over ranks then writes the fp32 words of dst.
__global__ __launch_bounds__(kT) void k_vec_fold(const double* vecpart, int nblk, int r, float* dst, double* dst64) {
  __shared__ double sh[8][32];
  const int i = threadIdx.x & 31, part = threadIdx.x >> 5;
  double s = 0.0;
  if (i < r)
    for (int b = part; b < nblk; b += 8) s += vecpart[(long)b * 32 + i];
  sh[part][i] = s;
  __syncthreads();
  if ((int)threadIdx.x < r) {
    double t = 0.0;
    for (int p = 0; p < 8; ++p) t += sh[p][threadIdx.x];
    if (dst64) dst64[threadIdx.x] = t;
    else dst[threadIdx.x] = (float)t;
  }
}

// ------------------------------------------------------------------ host side
struct Ws {
  float* hdr; double* G; float* maxpart; double* vecpart; double* grampart; float* nabla;
};

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

int64_t ws_bytes_for(int64_t N) { return (kOffNabla + 4 * N + 255) & ~(int64_t)255; }

int carve(void* ws, int64_t ws_bytes, int64_t N, Ws& o) {
  if (!ws || ws_bytes < ws_bytes_for(N) || misaligned(ws, 256)) return PSGD_ERR_WORKSPACE;
  char* b = static_cast<char*>(ws);
  o.hdr = reinterpret_cast<float*>(b + kOffHdr);
  o.G = reinterpret_cast<double*>(b + kOffG);
  o.maxpart = reinterpret_cast<float*>(b + kOffMax);
  o.vecpart = reinterpret_cast<double*>(b + kOffVec);
  o.grampart = reinterpret_cast<double*>(b + kOffGram);
  o.nabla = reinterpret_cast<float*>(b + kOffNabla);
  return PSGD_OK;
}

int check_common(int64_t N, int r) {
  if (N <= 0 || r <= 0) return PSGD_ERR_BAD_ARG;
  if (r > kMaxR) return PSGD_ERR_RANK;
  return PSGD_OK;
}

// one block per tile up to the number of blocks the CUs hold at this LDS footprint
int grid_for(int64_t N, const Geo& g, size_t lds_bytes, int cap) {
  int per_cu = (int)((160 * 1024) / (lds_bytes + 512));
  if (per_cu > 6) per_cu = 6;
  if (per_cu < 1) per_cu = 1;
  int64_t blocks = (int64_t)kCUs * per_cu;
  if (blocks > cap) blocks = cap;
  const int64_t ntiles = (N + g.TR - 1) / g.TR;
  return (int)(ntiles < blocks ? ntiles : blocks);
}

constexpr int kMaxRp = kMaxR | 1;
constexpr size_t kGramLdsMax = (size_t)kT * (2 * kMaxRp + 7) * 4;
constexpr size_t kRewriteLdsMax = (size_t)kT * 2 * kMaxRp * 4;

int launch_ok() { return hipGetLastError() == hipSuccess ? PSGD_OK : PSGD_ERR_LAUNCH; }

// send: nullptr = the one-call form (the sums go straight to the header as fp32); otherwise the staged form, which leaves
// them as fp64 in `send` for the exchange
template <int MODE>
int run_apply_sweep(const u16* M, u16* d, const float* g, float* out, int64_t N, const Geo& geo, const Ws& w, int mode,
                    SrKey keyD, int64_t row0, double* send, hipStream_t st) {
  const size_t lds = (size_t)kT * (geo.rp + 4) * 4 < 4 * 32 * 3 * 8 ? 4 * 32 * 3 * 8 : (size_t)kT * (geo.rp + 4) * 4;
  const int grid = grid_for(N, geo, lds, kMaxBlocks);
  hipLaunchKernelGGL(k_apply<MODE>, dim3(grid), dim3(kT), lds, st, M, d, g, out, (long)N, geo, w.hdr, w.nabla, mode, keyD,
                     (long)row0, w.vecpart);
  if (MODE != 3)
    hipLaunchKernelGGL(k_vec_fold, dim3(1), dim3(kT), 0, st, w.vecpart, grid, geo.r, w.hdr + (MODE == 2 ? kHS2 : kHS1), send);
  return launch_ok();
}

// block maxima of |U|, |V| (the balance branch); returns the number of blocks
int run_bmax(const u16* U, const u16* V, int64_t N, int r, const Ws& w, hipStream_t st) {
  const int64_t nch = (N * r + 7) / 8;
  const int64_t want = (nch + kT - 1) / kT;
  const int bgrid = (int)(want < kMaxBlocks ? want : kMaxBlocks);
  hipLaunchKernelGGL(k_bmax, dim3(bgrid), dim3(kT), 0, st, U, V, (long)(N * r), w.maxpart);
  return bgrid;
}

// Gram sweep and the fold of its block partials
int run_gram(const u16* U, const u16* V, const u16* d, const float* v, const float* h, int64_t N, const Geo& geo, const Ws& w,
             hipStream_t st) {
  const int r = geo.r;
  const int nb = (2 * r + 6 + 15) / 16;
  const size_t lds = (size_t)kT * (2 * geo.rp + 7) * 4;
  const int ggrid = grid_for(N, geo, lds, kGramBlocks);
  switch (nb) {
#define PSGD_GRAM_CASE(NB)                                                                                            \
  case NB:                                                                                                            \
    if (int rc = set_lds<k_gram<NB>>(kGramLdsMax)) return rc;                                                                 \
    hipLaunchKernelGGL(k_gram<NB>, dim3(ggrid), dim3(kT), lds, st, U, V, d, v, h, (long)N, geo, w.grampart);           \
    break;
    PSGD_GRAM_CASE(1) PSGD_GRAM_CASE(2) PSGD_GRAM_CASE(3) PSGD_GRAM_CASE(4) PSGD_GRAM_CASE(5)
#undef PSGD_GRAM_CASE
    default: return PSGD_ERR_RANK;
  }
  hipLaunchKernelGGL(k_gram_fold, dim3(kPairs), dim3(kT), 0, st, w.grampart, ggrid, nb, w.G);
  return PSGD_OK;
}

// r x r algebra and the rewrite sweep; *grid_out = the number of block maxima of |nablaD| it leaves
int run_rewrite(u16* U, u16* V, const u16* d, const float* v, const float* h, int64_t N, const Geo& geo, float step,
                float tiny, int balance, int update_U, int mode, uint64_t seed, int64_t row0, const Ws& w, hipStream_t st,
                int* grid_out) {
  hipLaunchKernelGGL(k_small, dim3(1), dim3(64), 0, st, w.G, geo.r, step, tiny, update_U, w.hdr);
  const size_t lds2 = (size_t)kT * 2 * geo.rp * 4;
  const int grid = grid_for(N, geo, lds2, kMaxBlocks);
  if (int rc = set_lds<k_rewrite>(kRewriteLdsMax)) return rc;
  hipLaunchKernelGGL(k_rewrite, dim3(grid), dim3(kT), lds2, st, U, V, d, v, h, (long)N, geo, w.hdr, update_U, balance, mode,
                     make_key(seed, 0), make_key(seed, 1), (long)row0, w.nabla, w.maxpart);
  *grid_out = grid;
  return PSGD_OK;
}

// update without its d sweep: [balance maxima] scales, Gram, fold, r x r algebra, rewrite, mu_d
int run_update_front(u16* U, u16* V, const u16* d, const float* v, const float* h, int64_t N, const Geo& geo, float step,
                     float tiny, int balance, int update_U, int mode, uint64_t seed, const Ws& w, hipStream_t st) {
  const int bgrid = balance ? run_bmax(U, V, N, geo.r, w, st) : 1;
  hipLaunchKernelGGL(k_scales, dim3(1), dim3(64), 0, st, w.maxpart, bgrid, balance, w.hdr);
  if (int rc = run_gram(U, V, d, v, h, N, geo, w, st)) return rc;
  int grid = 0;
  if (int rc = run_rewrite(U, V, d, v, h, N, geo, step, tiny, balance, update_U, mode, seed, 0, w, st, &grid)) return rc;
  hipLaunchKernelGGL(k_mu_d, dim3(1), dim3(64), 0, st, w.maxpart, grid, step, tiny, w.hdr);
  return launch_ok();
}

void run_d_update(u16* d, int64_t N, int mode, uint64_t seed, int64_t row0, const Ws& w, hipStream_t st) {
  const int64_t want = (N + kT - 1) / kT;
  const int grid = (int)(want < 2048 ? want : 2048);
  hipLaunchKernelGGL(k_d_update, dim3(grid), dim3(kT), 0, st, d, w.nabla, (long)N, w.hdr, mode, make_key(seed, 2), (long)row0);
}

double* send_ptr(void* ws, int64_t off) { return reinterpret_cast<double*>(static_cast<char*>(ws) + off); }

// offset (bytes) and count (doubles) of the send region of `stage`; false for an unknown stage
bool send_region(int stage, int r, int64_t* off, int64_t* count) {
  switch (stage) {
    case 1: *off = kOffSend1; *count = r; return true;
    case 2: *off = kOffSend2; *count = r; return true;
    case 10: *off = kOffSend10; *count = 2; return true;
    case 11: *off = kOffG; *count = (int64_t)16 * ((2 * r + 6 + 15) / 16) * kGS; return true;   // the rows of G in use
    case 12: *off = kOffSend12; *count = 1; return true;
    default: return false;
  }
}

}  // namespace

extern "C" {

uint64_t psgd_uvd_bf16_rounding_key(uint64_t seed, int tensor) { return key64(seed, (unsigned)tensor); }

int64_t psgd_uvd_bf16_workspace_bytes(int64_t N, int r) {
  if (int rc = check_common(N, r)) return rc;
  return ws_bytes_for(N);
}

int psgd_uvd_bf16_narrow_f32(const float* src, void* dst, int64_t count, int64_t index0, int tensor, int rounding, uint64_t seed,
                             void* stream) {
  if (!src || !dst || count < 0 || index0 < 0) return PSGD_ERR_BAD_ARG;
  if (tensor < 0 || tensor > 2 || (rounding != 0 && rounding != 1)) return PSGD_ERR_BAD_ARG;
  if (misaligned(src, 4) || misaligned(dst, 2)) return PSGD_ERR_ALIGN;
  if (count == 0) return PSGD_OK;
  // two 8-element groups per thread before the grid-stride loop takes over
  int64_t blocks = (count / 8 + 2 * kT - 1) / (2 * kT);
  if (blocks < 1) blocks = 1;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  hipLaunchKernelGGL(k_narrow_f32, dim3((unsigned)blocks), dim3(kT), 0, static_cast<hipStream_t>(stream), src, static_cast<u16*>(dst),
                     (long)count, rounding, make_key(seed, (unsigned)tensor), (unsigned long long)index0);
  return launch_ok();
}

static int check_apply(const void* U, const void* V, const void* d, const float* g, float* out, int64_t N, int r) {
  if (!U || !V || !d || !g || !out) return PSGD_ERR_BAD_ARG;
  if (int rc = check_common(N, r)) return rc;
  if (out == g) return PSGD_ERR_BAD_ARG;
  if (misaligned(U, 16) || misaligned(V, 16) || misaligned(d, 16) || misaligned(g, 4) || misaligned(out, 4))
    return PSGD_ERR_ALIGN;
  return PSGD_OK;
}

int psgd_uvd_apply_bf16(const void* U, const void* V, const void* d, const float* g, float* out, int64_t N, int r, void* ws,
                        int64_t ws_bytes, void* stream) {
  if (int rc = check_apply(U, V, d, g, out, N, r)) return rc;
  Ws w;
  if (int rc = carve(ws, ws_bytes, N, w)) return rc;
  const Geo geo = make_geo(r);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const SrKey k0{0, 0};
  u16* dd = const_cast<u16*>(static_cast<const u16*>(d));   // MODE 0, 2, 3 only read d
  if (int rc = run_apply_sweep<0>(static_cast<const u16*>(V), dd, g, out, N, geo, w, 0, k0, 0, nullptr, st)) return rc;
  if (int rc = run_apply_sweep<2>(static_cast<const u16*>(U), dd, g, out, N, geo, w, 0, k0, 0, nullptr, st)) return rc;
  return run_apply_sweep<3>(static_cast<const u16*>(V), dd, g, out, N, geo, w, 0, k0, 0, nullptr, st);
}

static int check_update(const void* U, const void* V, const void* d, const float* v, const float* h, int64_t N, int r,
                        int rounding) {
  if (!U || !V || !d || !v || !h) return PSGD_ERR_BAD_ARG;
  if (int rc = check_common(N, r)) return rc;
  if (rounding != 0 && rounding != 1) return PSGD_ERR_BAD_ARG;
  if (U == V) return PSGD_ERR_BAD_ARG;
  if (misaligned(U, 16) || misaligned(V, 16) || misaligned(d, 16) || misaligned(v, 4) || misaligned(h, 4))
    return PSGD_ERR_ALIGN;
  return PSGD_OK;
}

int psgd_uvd_update_bf16(void* U, void* V, void* d, const float* v, const float* h, int64_t N, int r, float step, float tiny,
                         int balance, int update_U, int rounding, uint64_t seed, void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = check_update(U, V, d, v, h, N, r, rounding)) return rc;
  Ws w;
  if (int rc = carve(ws, ws_bytes, N, w)) return rc;
  const Geo geo = make_geo(r);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = run_update_front(static_cast<u16*>(U), static_cast<u16*>(V), static_cast<const u16*>(d), v, h, N, geo, step,
                                tiny, balance != 0, update_U != 0, rounding, seed, w, st))
    return rc;
  run_d_update(static_cast<u16*>(d), N, rounding, seed, 0, w, st);
  return launch_ok();
}

int psgd_uvd_update_apply_bf16(void* U, void* V, void* d, const float* v, const float* h, const float* g, float* out,
                               int64_t N, int r, float step, float tiny, int balance, int update_U, int rounding,
                               uint64_t seed, void* ws, int64_t ws_bytes, void* stream) {
  if (!g || !out) return PSGD_ERR_BAD_ARG;
  if (int rc = check_update(U, V, d, v, h, N, r, rounding)) return rc;
  if (out == g || out == v || out == h) return PSGD_ERR_BAD_ARG;
  if (misaligned(g, 4) || misaligned(out, 4)) return PSGD_ERR_ALIGN;
  Ws w;
  if (int rc = carve(ws, ws_bytes, N, w)) return rc;
  const Geo geo = make_geo(r);
  hipStream_t st = static_cast<hipStream_t>(stream);
  u16 *Uq = static_cast<u16*>(U), *Vq = static_cast<u16*>(V), *dq = static_cast<u16*>(d);
  if (int rc = run_update_front(Uq, Vq, dq, v, h, N, geo, step, tiny, balance != 0, update_U != 0, rounding, seed, w, st))
    return rc;
  const SrKey kd = make_key(seed, 2);
  if (int rc = run_apply_sweep<1>(Vq, dq, g, out, N, geo, w, rounding, kd, 0, nullptr, st)) return rc;
  if (int rc = run_apply_sweep<2>(Uq, dq, g, out, N, geo, w, rounding, kd, 0, nullptr, st)) return rc;
  return run_apply_sweep<3>(Vq, dq, g, out, N, geo, w, rounding, kd, 0, nullptr, st);
}

// ------------------------------------------------------------------ staged forms (row-sharded state)
int psgd_uvd_bf16_ws_region(int which, int stage, int64_t N, int r, int64_t* offset_bytes, int64_t* count) {
  if (!offset_bytes || !count) return PSGD_ERR_BAD_ARG;
  if (int rc = check_common(N, r)) return rc;
  if (which != PSGD_WS_SEND_F64) return PSGD_ERR_BAD_ARG;
  return send_region(stage, r, offset_bytes, count) ? PSGD_OK : PSGD_ERR_BAD_ARG;
}

int psgd_uvd_bf16_fold_gathered_f64(int stage, const double* gathered, int world, int64_t N, int r, void* ws,
                                    int64_t ws_bytes, void* stream) {
  if (!gathered || world < 1 || misaligned(gathered, 8)) return PSGD_ERR_BAD_ARG;
  if (int rc = check_common(N, r)) return rc;
  int64_t off = 0, count = 0;
  if (!send_region(stage, r, &off, &count)) return PSGD_ERR_BAD_ARG;
  Ws w;
  if (int rc = carve(ws, ws_bytes, N, w)) return rc;
  float* fdst = nullptr;
  int is_max = 0, ncols = 0;
  if (stage == 1) fdst = w.hdr + kHS1;
  else if (stage == 2) fdst = w.hdr + kHS2;
  else if (stage == 11) ncols = 16 * ((2 * r + 6 + 15) / 16);
  else { is_max = 1; fdst = w.maxpart; }   // 10: what k_scales folds (one "block"); 12: what k_mu_d folds
  hipLaunchKernelGGL(k_fold_gathered_b, dim3(((int)count + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                     gathered, world, (int)count, is_max, ncols, send_ptr(ws, off), fdst);
  return launch_ok();
}

int psgd_uvd_balance_max_bf16(const void* U, const void* V, int64_t N, int r, void* ws, int64_t ws_bytes, void* stream) {
  if (!U || !V) return PSGD_ERR_BAD_ARG;
  if (int rc = check_common(N, r)) return rc;
  if (misaligned(U, 16) || misaligned(V, 16)) return PSGD_ERR_ALIGN;
  Ws w;
  if (int rc = carve(ws, ws_bytes, N, w)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int bgrid = run_bmax(static_cast<const u16*>(U), static_cast<const u16*>(V), N, r, w, st);
  hipLaunchKernelGGL(k_bmax_fold, dim3(1), dim3(64), 0, st, w.maxpart, bgrid, send_ptr(ws, kOffSend10));
  return launch_ok();
}

int psgd_uvd_update_gram_bf16(const void* U, const void* V, const void* d, const float* v, const float* h, int64_t N, int r,
                              void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = check_update(U, V, d, v, h, N, r, 0)) return rc;
  Ws w;
  if (int rc = carve(ws, ws_bytes, N, w)) return rc;
  if (int rc = run_gram(static_cast<const u16*>(U), static_cast<const u16*>(V), static_cast<const u16*>(d), v, h, N,
                        make_geo(r), w, static_cast<hipStream_t>(stream)))
    return rc;
  return launch_ok();
}

int psgd_uvd_update_rewrite_bf16(void* U, void* V, const void* d, const float* v, const float* h, int64_t N, int r,
                                 float step, float tiny, int balance, int update_U, int rounding, uint64_t seed,
                                 int64_t row0, void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = check_update(U, V, d, v, h, N, r, rounding)) return rc;
  if (row0 < 0) return PSGD_ERR_BAD_ARG;
  Ws w;
  if (int rc = carve(ws, ws_bytes, N, w)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // after the fold of stage 10 the maxima of the whole problem are the one "block" of the scales kernel
  hipLaunchKernelGGL(k_scales, dim3(1), dim3(64), 0, st, w.maxpart, 1, balance != 0, w.hdr);
  int grid = 0;
  if (int rc = run_rewrite(static_cast<u16*>(U), static_cast<u16*>(V), static_cast<const u16*>(d), v, h, N, make_geo(r), step,
                           tiny, balance != 0, update_U != 0, rounding, seed, row0, w, st, &grid))
    return rc;
  hipLaunchKernelGGL(k_max_fold, dim3(1), dim3(64), 0, st, w.maxpart, grid, send_ptr(ws, kOffSend12));
  return launch_ok();
}

static int check_d(const void* d, int64_t N, int r, int rounding, int64_t row0) {
  if (!d) return PSGD_ERR_BAD_ARG;
  if (int rc = check_common(N, r)) return rc;
  if ((rounding != 0 && rounding != 1) || row0 < 0) return PSGD_ERR_BAD_ARG;
  if (misaligned(d, 16)) return PSGD_ERR_ALIGN;
  return PSGD_OK;
}

int psgd_uvd_update_d_bf16(void* d, int64_t N, int r, float step, float tiny, int rounding, uint64_t seed, int64_t row0,
                           void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = check_d(d, N, r, rounding, row0)) return rc;
  Ws w;
  if (int rc = carve(ws, ws_bytes, N, w)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_mu_d, dim3(1), dim3(64), 0, st, w.maxpart, 1, step, tiny, w.hdr);
  run_d_update(static_cast<u16*>(d), N, rounding, seed, row0, w, st);
  return launch_ok();
}

int psgd_uvd_apply_sweep1_bf16(const void* V, const void* d, const float* g, int64_t N, int r, void* ws, int64_t ws_bytes,
                               void* stream) {
  if (!V || !d || !g) return PSGD_ERR_BAD_ARG;
  if (int rc = check_common(N, r)) return rc;
  if (misaligned(V, 16) || misaligned(d, 16) || misaligned(g, 4)) return PSGD_ERR_ALIGN;
  Ws w;
  if (int rc = carve(ws, ws_bytes, N, w)) return rc;
  u16* dd = const_cast<u16*>(static_cast<const u16*>(d));   // MODE 0 only reads d
  return run_apply_sweep<0>(static_cast<const u16*>(V), dd, g, nullptr, N, make_geo(r), w, 0, SrKey{0, 0}, 0,
                            send_ptr(ws, kOffSend1), static_cast<hipStream_t>(stream));
}

int psgd_uvd_apply_sweep1_d_bf16(const void* V, void* d, const float* g, int64_t N, int r, float step, float tiny,
                                 int rounding, uint64_t seed, int64_t row0, void* ws, int64_t ws_bytes, void* stream) {
  if (!V || !g) return PSGD_ERR_BAD_ARG;
  if (int rc = check_d(d, N, r, rounding, row0)) return rc;
  if (misaligned(V, 16) || misaligned(g, 4)) return PSGD_ERR_ALIGN;
  Ws w;
  if (int rc = carve(ws, ws_bytes, N, w)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_mu_d, dim3(1), dim3(64), 0, st, w.maxpart, 1, step, tiny, w.hdr);
  return run_apply_sweep<1>(static_cast<const u16*>(V), static_cast<u16*>(d), g, nullptr, N, make_geo(r), w, rounding,
                            make_key(seed, 2), row0, send_ptr(ws, kOffSend1), st);
}

int psgd_uvd_apply_sweep2_bf16(const void* U, const void* d, const float* g, float* out, int64_t N, int r, void* ws,
                               int64_t ws_bytes, void* stream) {
  if (int rc = check_apply(U, U, d, g, out, N, r)) return rc;
  Ws w;
  if (int rc = carve(ws, ws_bytes, N, w)) return rc;
  u16* dd = const_cast<u16*>(static_cast<const u16*>(d));
  return run_apply_sweep<2>(static_cast<const u16*>(U), dd, g, out, N, make_geo(r), w, 0, SrKey{0, 0}, 0,
                            send_ptr(ws, kOffSend2), static_cast<hipStream_t>(stream));
}

int psgd_uvd_apply_sweep3_bf16(const void* V, const void* d, float* out, int64_t N, int r, void* ws, int64_t ws_bytes,
                               void* stream) {
  if (!V || !d || !out) return PSGD_ERR_BAD_ARG;
  if (int rc = check_common(N, r)) return rc;
  if (misaligned(V, 16) || misaligned(d, 16) || misaligned(out, 4)) return PSGD_ERR_ALIGN;
  Ws w;
  if (int rc = carve(ws, ws_bytes, N, w)) return rc;
  u16* dd = const_cast<u16*>(static_cast<const u16*>(d));
  return run_apply_sweep<3>(static_cast<const u16*>(V), dd, nullptr, out, N, make_geo(r), w, 0, SrKey{0, 0}, 0, nullptr,
                            static_cast<hipStream_t>(stream));
}

}  // extern "C"
