// kron_quad_seg.h -- SegOpnd, the operand with a SEGMENTED K, shared by psgd_kron_qnd.hip (one order-3 layer) and
// psgd_kron_qtlist.hip (a list of them): the Gram over the middle mode of a row-major tensor [A, B, C] sums over the PAIR (a, c),
// k -> (k / C) BC + (k % C), K = A C.  psgd_kron_qnd.hip says why and how the fetch works; product_of() of kron_quad_core.h finds
// the two fetch halves below by argument type.  Device code only.
#pragma once
#include "kron_quad_core.h"

namespace psgdq {

// an operand whose summed index runs over two tensor modes: element (x, k) = p[(k / C) BC + x C + (k % C)], x in [0, X)
struct SegOpnd {
  const float* p;
  long BC;
  int C, X;
};

// this thread's four elements of the step [x0, x0 + kTile) x [k0, k0 + kGK), zero outside [0, X) x [0, K): x = t & 63, four k
// from (t >> 6) * 4, as the k-contiguous half of g2r(const Opnd&)
__device__ __forceinline__ void g2r(const SegOpnd& o, int x0, int k0, int K, float (&r)[4]) {
  const int t = threadIdx.x;
  const int x = x0 + (t & 63), k = k0 + (t >> 6) * 4;
  int a = k / o.C, c = k - a * o.C;
  const bool wide = x0 + kTile <= o.X && k0 + kGK <= K && (o.C & 3) == 0 && (reinterpret_cast<uintptr_t>(o.p) & 15) == 0;
  if (wide) {                                           // k % 4 == 0 and C % 4 == 0: one segment, a 16-byte aligned address
    const f32x4 v = *reinterpret_cast<const f32x4*>(o.p + (long)a * o.BC + (long)x * o.C + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = v[e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      r[e] = (x < o.X && k + e < K) ? o.p[(long)a * o.BC + (long)x * o.C + c] : 0.f;
      if (++c == o.C) {                                 // the next k opens the next slab
        c = 0;
        ++a;
      }
    }
  }
}
__device__ __forceinline__ void r2s(const SegOpnd&, const float (&r)[4], float* S) {
  const int t = threadIdx.x;
#pragma unroll
  for (int e = 0; e < 4; ++e) S[((t >> 6) * 4 + e) * kPitch + (t & 63)] = r[e];
}

}  // namespace psgdq
