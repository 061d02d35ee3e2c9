// kron_quad_x3_core.h -- the second product core of the QUAD kernels: fp32-grade products of FULL operands on the bf16 matrix
// cores ("bf16 x 3"), for psgd_kron_quad_x3.hip.  Device code only, all of it inline.
//
// Arithmetic.  Every fp32 operand element is split exactly into three bf16 terms x = h + m + l (truncating: h = the top 16 bits,
// r = x - h, m = the top 16 bits of r, l = r - m; 8 + 8 + 8 significant bits), on the way into LDS: there is no conversion launch
// and no bf16 copy in HBM.  A product is accumulated in fp32 as six v_mfma_f32_16x16x32_bf16 terms per K step, smallest first:
// m m' + h l' + l h' + h m' + m h' + h h'.  The dropped terms m l' + l m' + l l' are at most 2^-21 of |a||b|.  An operand whose
// elements have at most 8 significant bits is its own h plane (m = l = 0), and h h' is then the exact product.
//
// Tile.  product_x3() forms one 128 x 128 macro tile for a workgroup of four waves, K step 32.  Wave (wm, wn) owns the 32 x 32
// quarter (wm, wn) of EACH of the four 64 x 64 sub-tiles: acc[si][sj][i][j], 16 f32x4.  acc[si][sj] is therefore, for the four
// waves together, exactly the accumulator layout product() of kron_quad_core.h documents for the 64-tile (si, sj) of the macro
// tile, and the 64-tile epilogues of that header (gram_epilogue, store_tile, p1_store, p2_finish, p2_sym_store, each_elem) run
// on it once per sub-tile, unchanged.  Per K step a wave reads 8 row groups x 3 planes = 24 ds_read_b128 for 96 MFMAs (the
// 64 x 64 tile would read 12 for 24: operand-bandwidth-bound at this matrix rate).
//
// LDS image.  [A|B][plane][row * 4 + (chunk ^ x3_swz(row))]: 128 rows of 32 k as bf16 (64 bytes = four 16-byte chunks), three
// planes per operand, 48 KiB, ONE buffer: the next K step waits in registers (16 floats per operand and thread) while the MFMAs
// of this one run, and is split and committed between two barriers.  The chunk swizzle (0 - (row >> 2)) & 3 is conflict-free
// for the lane groups ds_read_b128 is really served in (see psgd_kron.hip, lds_swz: the same map).  Whatever the layout of the
// view in memory, a thread ends up with 16 consecutive k of ONE row, so both layouts end as k-contiguous rows in LDS by two
// 16-byte stores per plane:
//   X3_KVEC  k contiguous (ks == 1), base 16-byte aligned, xs a multiple of 4: row = tid / 2, k half = tid % 2, four 16-byte loads;
//   X3_XROW  x contiguous (xs == 1), any base and ks: row = tid % 128, k half = tid / 128, sixteen dword loads, each coalesced
//            across the wave (lane -> row).  16-byte loads along x would leave a lane with four rows x four k, i.e. 2-byte
//            scattered LDS stores or a transpose through LDS; the lane -> row map transposes in registers for nothing;
//   X3_EDGE  anything else (a skewed base, an odd leading dimension) and the ragged K tail: the first map with dword loads from
//            CLAMPED addresses; what lies outside [0, X) x [0, K) is zeroed when the step is committed to LDS.
// The fast modes serve partial tiles in x too: the lane's row is clamped to the operand's last one (a duplicate load) and zeroed
// at the commit.  Nothing is ever read or written outside [0, X) x [0, K).  The fetch is straight-line code and never USES a
// loaded value, and the mode pair is chosen once per product, outside the K loop: the loads of step t + 1 are issued ahead of
// the MFMAs of step t, and a use -- or a branch between load variants -- would put a memory latency in front of the matrix work.
// The value of an element in LDS does not depend on the mode, and every mode pair runs the same K steps in the same order on the
// same MFMA sequence: a skewed or odd-strided call produces the bits of the aligned one.
#pragma once
#include "kron_quad_core.h"

namespace psgdq {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kMac = 2 * kTile;              // macro tile edge
constexpr int kXK = 32;                      // K step
static_assert(kMac == 128 && kT == 256, "the thread <-> element maps below are written for these");

struct X3Lds {
  u32x4 P[2][3][kMac * 4];                   // [A|B][plane][row * 4 + (chunk ^ x3_swz(row))], a chunk = 8 consecutive k as bf16
};
static_assert(sizeof(X3Lds) == 48 * 1024 && sizeof(X3Lds) >= sizeof(float) * kLdsFloats, "a parked 64-tile reuses the planes");

__device__ __forceinline__ int x3_swz(int row) { return (0 - (row >> 2)) & 3; }

// two fp32 values -> three packed bf16 pairs (plane h, m, l; low half = x0): 4 VALU ops per element, one v_perm_b32 per pair
// and plane
__device__ __forceinline__ void x3_split_pair(float x0, float x1, unsigned (&pk)[3]) {
  const unsigned top = 0xFFFF0000u;
  const float h0 = __uint_as_float(__float_as_uint(x0) & top), h1 = __uint_as_float(__float_as_uint(x1) & top);
  const float r0 = x0 - h0, r1 = x1 - h1;
  const float m0 = __uint_as_float(__float_as_uint(r0) & top), m1 = __uint_as_float(__float_as_uint(r1) & top);
  const float s0 = r0 - m0, s1 = r1 - m1;
  pk[0] = __builtin_amdgcn_perm(__float_as_uint(x1), __float_as_uint(x0), 0x07060302u);   // (x0 >> 16) | (x1 & top)
  pk[1] = __builtin_amdgcn_perm(__float_as_uint(r1), __float_as_uint(r0), 0x07060302u);
  pk[2] = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302u);
}

enum { X3_EDGE = 0, X3_KVEC = 1, X3_XROW = 2 };

__device__ __forceinline__ int x3_mode(const Opnd& o) {
  if (o.xs == 1) return X3_XROW;
  if (o.ks == 1 && (o.xs & 3) == 0 && (reinterpret_cast<uintptr_t>(o.p) & 15) == 0) return X3_KVEC;
  return X3_EDGE;
}

// the per-lane byte offset of a fast mode, the same for every K step (the base is uniform and advances with k); x0 < X
template <int MODE>
__device__ __forceinline__ unsigned x3_lane_offset(const Opnd& o, int x0) {
  const int tid = threadIdx.x, last = o.X - 1 - x0;
  if (MODE == X3_XROW) return 4u * ((unsigned)(tid >> 7) * 16u * (unsigned)o.ks + (unsigned)min(tid & 127, last));
  if (MODE == X3_KVEC) return 4u * ((unsigned)min(tid >> 1, last) * (unsigned)o.xs + (unsigned)(tid & 1) * 16u);
  return 0u;
}

// this thread's 16 consecutive k of one row of the step [x0, x0 + 128) x [k0, k0 + 32); the fast modes need k0 + 32 <= K
template <int MODE>
__device__ __forceinline__ void x3_g2r(const Opnd& o, int x0, int k0, int K, unsigned voff, float (&r)[16]) {
  const int tid = threadIdx.x;
  if (MODE == X3_XROW) {
    const char* sb = reinterpret_cast<const char*>(o.p + (long)k0 * o.ks + x0);
#pragma unroll
    for (int u = 0; u < 16; ++u) r[u] = *reinterpret_cast<const float*>(sb + (long)u * o.ks * 4 + voff);
  } else if (MODE == X3_KVEC) {
    const char* sb = reinterpret_cast<const char*>(o.p + (long)x0 * o.xs + k0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(sb + 16 * q + voff);
#pragma unroll
      for (int e = 0; e < 4; ++e) r[4 * q + e] = v[e];
    }
  } else {
    const long xo = (long)min(x0 + (tid >> 1), o.X - 1) * o.xs;
#pragma unroll
    for (int u = 0; u < 16; ++u) r[u] = o.p[xo + (long)min(k0 + (tid & 1) * 16 + u, K - 1) * o.ks];
  }
}

// ... split and committed to the three planes P of the operand, zero outside [0, X) x [0, K)
template <int MODE>
__device__ __forceinline__ void x3_r2s(const Opnd& o, int x0, int k0, int K, const float (&r)[16], u32x4 (*P)[kMac * 4]) {
  const int tid = threadIdx.x;
  const int xr = MODE == X3_XROW ? (tid & 127) : (tid >> 1);
  const int kb = MODE == X3_XROW ? (tid >> 7) * 16 : (tid & 1) * 16;
  const bool xin = x0 + xr < o.X;
  unsigned pk[3][8];
#pragma unroll
  for (int u = 0; u < 16; u += 2) {
    float v0, v1;
    if (MODE == X3_EDGE) {
      v0 = (xin && k0 + kb + u < K) ? r[u] : 0.0f;
      v1 = (xin && k0 + kb + u + 1 < K) ? r[u + 1] : 0.0f;
    } else {
      v0 = xin ? r[u] : 0.0f;
      v1 = xin ? r[u + 1] : 0.0f;
    }
    unsigned q[3];
    x3_split_pair(v0, v1, q);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) pk[pl][u >> 1] = q[pl];
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = (kb >> 3) + h;
    const int sl = xr * 4 + (c ^ x3_swz(xr));
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) P[pl][sl] = u32x4{pk[pl][4 * h], pk[pl][4 * h + 1], pk[pl][4 * h + 2], pk[pl][4 * h + 3]};
  }
}

// n K steps [k0 + 32 t, + 32) accumulated into acc.  Enters and leaves with the LDS buffer free.
template <int MA, int MB>
__device__ __forceinline__ void x3_pass(const Opnd& a, const Opnd& b, int m0, int n0, int k0, int K, int n, X3Lds& L,
                                        f32x4 (&acc)[2][2][2][2]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1, c = lane >> 4;
  float ra[16], rb[16];
  const unsigned va = x3_lane_offset<MA>(a, m0), vb = x3_lane_offset<MB>(b, n0);
  x3_g2r<MA>(a, m0, k0, K, va, ra);
  x3_g2r<MB>(b, n0, k0, K, vb, rb);
  x3_r2s<MA>(a, m0, k0, K, ra, L.P[0]);
  x3_r2s<MB>(b, n0, k0, K, rb, L.P[1]);
  __syncthreads();
  for (int t = 0; t < n; ++t) {
    const int kn = k0 + min(t + 1, n - 1) * kXK;       // the last step re-reads its own tile: no branch round the loads
    x3_g2r<MA>(a, m0, kn, K, va, ra);
    x3_g2r<MB>(b, n0, kn, K, vb, rb);
    __builtin_amdgcn_sched_barrier(0);                 // the loads are issued here, ahead of the matrix work
    bf16x8 fa[2][2][3], fb[2][2][3];                   // [sub-tile][16-row group][plane]
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int ar = s * kTile + wm * 32 + i * 16 + (lane & 15), br = s * kTile + wn * 32 + i * 16 + (lane & 15);
        const int sa = ar * 4 + (c ^ x3_swz(ar)), sb = br * 4 + (c ^ x3_swz(br));
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
          fa[s][i][pl] = __builtin_bit_cast(bf16x8, L.P[0][pl][sa]);
          fb[s][i][pl] = __builtin_bit_cast(bf16x8, L.P[1][pl][sb]);
        }
      }
#pragma unroll
    for (int si = 0; si < 2; ++si)
#pragma unroll
      for (int sj = 0; sj < 2; ++sj)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            f32x4 v = acc[si][sj][i][j];
            v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[si][i][1], fb[sj][j][1], v, 0, 0, 0);   // m m'
            v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[si][i][0], fb[sj][j][2], v, 0, 0, 0);   // h l'
            v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[si][i][2], fb[sj][j][0], v, 0, 0, 0);   // l h'
            v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[si][i][0], fb[sj][j][1], v, 0, 0, 0);   // h m'
            v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[si][i][1], fb[sj][j][0], v, 0, 0, 0);   // m h'
            v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[si][i][0], fb[sj][j][0], v, 0, 0, 0);   // h h'
            acc[si][sj][i][j] = v;
          }
    __builtin_amdgcn_sched_barrier(0);                 // ... and nothing that uses them is hoisted into it
    __syncthreads();                                   // every wave is done reading this K step
    if (t + 1 < n) {
      x3_r2s<MA>(a, m0, kn, K, ra, L.P[0]);
      x3_r2s<MB>(b, n0, kn, K, rb, L.P[1]);
    }
    __syncthreads();
  }
}

// acc = the macro tile (m0, n0) of sum_k a(m, k) b(n, k), m0 < a.X, n0 < b.X.  Enters with a barrier and leaves after one: the
// LDS is free on return.  Element e of acc[si][sj][i][j] is row si 64 + wm 32 + i 16 + (lane >> 4) 4 + e, column sj 64 + wn 32 +
// j 16 + (lane & 15) of the macro tile.  The whole K steps run in the pair's fast mode, the ragged tail (and every step of a
// pair without one) in X3_EDGE.
__device__ __forceinline__ void product_x3(const Opnd& a, const Opnd& b, int K, int m0, int n0, X3Lds& L, f32x4 (&acc)[2][2][2][2]) {
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[s >> 1][s & 1][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  const int ntot = (K + kXK - 1) / kXK, nfull = K / kXK;
  const int ma = x3_mode(a), mb = x3_mode(b);
  int e0 = 0;
  if (nfull > 0) {
    if (ma == X3_KVEC && mb == X3_XROW) {
      x3_pass<X3_KVEC, X3_XROW>(a, b, m0, n0, 0, K, nfull, L, acc);
      e0 = nfull;
    } else if (ma == X3_KVEC && mb == X3_KVEC) {
      x3_pass<X3_KVEC, X3_KVEC>(a, b, m0, n0, 0, K, nfull, L, acc);
      e0 = nfull;
    } else if (ma == X3_XROW && mb == X3_XROW) {
      x3_pass<X3_XROW, X3_XROW>(a, b, m0, n0, 0, K, nfull, L, acc);
      e0 = nfull;
    }
  }
  if (ntot > e0) x3_pass<X3_EDGE, X3_EDGE>(a, b, m0, n0, e0 * kXK, K, ntot - e0, L, acc);
}

__host__ __device__ static inline int macro_tiles_of(int n) { return (n + kMac - 1) / kMac; }

}  // namespace psgdq
