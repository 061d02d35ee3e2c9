// psgd_multi_tail.hip -- the tail of a step on LISTS of fp32 tensors (class Kron: mnist_with_lenet5.py:54-56 and the finite-difference
// route of psgd.py:716-727, :734-736) on gfx950, whatever the number of tensors; the parameter update itself (psgd_multi_param_update_*)
// is psgd_param_update.hip.
//
//   psgd_multi_sumsq_f32         sum of fl32(x x) over every element of every tensor -> one device double       (the clip norm's square)
//   psgd_multi_diff_scale_f32    h <- fl32(fl32(a - b) s),  and x <- fl32(v s) when given
//   psgd_multi_blend_f32         m <- fl32(fl32(beta m) + fl32(omb g));  beta == 0 does not read m                (momentum of class Kron)
//   psgd_multi_scale_check_f32   one to three lists: x <- fl32(x s_j) where s_j != 1, and a stamp stored to a flag word when a
//                                product is not finite                                                              (guarded step)
// and, for parameters of type T = bf16 / fp16 (everything else of the step stays fp32):
//   psgd_multi_widen_check       one to three lists of T tensors -> as many lists of fp32 tensors, dst <- fl32(float(src) s_j), with the
//                                flag of psgd_multi_scale_check_f32 on the written values
// and, for the VECTOR LAYERS of class Kron (a rank-1 parameter of length n is the [1, n] layer of the (dense, scaling) format:
// Ql is 1 x 1, qr is [1, n]; psgd.py:276-322), all k of them in one launch each:
//   psgd_multi_vec_update_f32    the factor update of psgd.py:276-307 on every (ql, qr), in place
//   psgd_multi_vec_apply_f32     out <- fl32(fl32(fl32(ql ql) g) fl32(qr qr)), the M < N branch of psgd.py:318-319, :322
// and, for the layers of class Kron(operands="bfloat16") that run on the bf16-operand Kron kernels (psgd_kron_bf16.hip):
//   psgd_multi_narrow_bf16       one to three lists of fp32 tensors -> as many lists of bf16 tensors, round to nearest even
//   psgd_multi_sumsq_mixed       psgd_multi_sumsq_f32 on a list whose tensors are fp32 or bf16, tensor by tensor
// and, for the probe vectors of class Kron(preconditioner_fit="whitening") (this one reads `start` of its table):
//   psgd_multi_randn_f32         out <- fl32(scale z), z standard normal, a counter-based draw keyed by (seed, flat element index)
//
// The tables are those of tail_common.h: a SEGMENT is one tensor {pointer, start, count}, a CHUNK one piece of at most
// PSGD_UVD_TAIL_CHUNK consecutive elements of one segment {segment index, offset}.  Here EVERY operand is a list: each has its own
// segment table, all tables of a call describe tensors of the same sizes, one chunk table serves them all, and `start` is not read.
// A chunk never runs past the shortest of its segments, whatever the tables say.
//
// HBM-bound streaming as in k_uvd_pack: inside a chunk the first stored operand is brought to a 16-byte boundary by a scalar head,
// the body moves 4 fp32 per lane and access, a scalar tail finishes; the other operands go through vector types whose declared
// alignment is the element's, so tensors that start at any float still take wide accesses.
//
// The sum of squares rounds each product to fp32, accumulates in fp64 per lane, folds lanes -> waves -> workgroup in a fixed order
// into one fp64 partial per workgroup; workgroup b takes chunks b, b + nb, b + 2 nb, ... with nb a function of nchunks alone, and a
// second one-workgroup launch folds the partials in index order: no atomics, the same bits on every call.
//
// No entry point allocates or synchronises; argument checks return before any HIP call.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "psgd_hip.h"
#include "tail_common.h"
#include "bf16_state.h"
#include "nanmax.h"

// The roundings are the contract (bit-equal to the torch expressions they replace): no product may be fused into a following sum.
#pragma clang fp contract(off)

namespace psgdm {

// the tables, the launch shape, F32 / BF16 / F16 (the PSGD_DTYPE_* codes) with their conversions and 16-byte accesses: tail_common.h
using namespace psgdtt;

constexpr int kSumsqBlocks = 1024;         // partials of the sum of squares: PSGD_MULTI_SUMSQ_WS_BYTES / 8
static_assert(kSumsqBlocks * 8 == PSGD_MULTI_SUMSQ_WS_BYTES, "workspace constant of the header");

// One chunk of a call: its element count (0: nothing to do) and the element pointers of up to five operands.
template <int kOps>
struct Piece {
  float* p[kOps];
  int n;
};

// tabs[j] == nullptr: operand j is absent (its pointer stays null and its length does not count)
template <int kOps>
__device__ __forceinline__ Piece<kOps> piece_of(const Seg* const (&tabs)[kOps], const Chunk ch, int k) {
  Piece<kOps> r;
  r.n = 0;
#pragma unroll
  for (int j = 0; j < kOps; ++j) r.p[j] = nullptr;
  if ((uint64_t)ch.seg >= (uint64_t)k || ch.off < 0) return r;      // a table that does not belong to these segments moves nothing
  int64_t left = kChunk;
#pragma unroll
  for (int j = 0; j < kOps; ++j) {
    if (!tabs[j]) continue;
    const Seg s = tabs[j][ch.seg];
    const int64_t l = s.count - ch.off;
    left = l < left ? l : left;
    r.p[j] = reinterpret_cast<float*>(s.ptr) + ch.off;
  }
  r.n = left > 0 ? (int)left : 0;
  return r;
}

// ------------------------------------------------------------------------------------------------------------- sum of squares
__global__ __launch_bounds__(kT) void k_multi_sumsq_partial(const Seg* __restrict__ segs, const Chunk* __restrict__ chunks,
                                                            int64_t nchunks, int k, double* __restrict__ partial) {
  __shared__ double lds[kT / 64];
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Seg* const tabs[1] = {segs};
    const Piece<1> pc = piece_of<1>(tabs, chunks[c], k);
    const int n = pc.n;
    if (n <= 0) continue;
    acc = sumsq_piece_f32(acc, pc.p[0], n, t);
  }
  const double s = block_sum(acc, lds);
  if (t == 0) partial[blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------------------- difference and scale
// h = fl32(fl32(a - b) s); kX: x = fl32(v s).  The 16-byte body is aligned on h; x is stored through the element-aligned type.
template <bool kX>
__global__ __launch_bounds__(kT) void k_multi_diff_scale(const Seg* __restrict__ asegs, const Seg* __restrict__ bsegs,
                                                         const Seg* __restrict__ hsegs, const Seg* __restrict__ vsegs,
                                                         const Seg* __restrict__ xsegs, const Chunk* __restrict__ chunks,
                                                         int64_t nchunks, int k, float s) {
  const int t = threadIdx.x;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Seg* const tabs[5] = {asegs, bsegs, hsegs, kX ? vsegs : nullptr, kX ? xsegs : nullptr};
    const Piece<5> pc = piece_of<5>(tabs, chunks[c], k);
    const int n = pc.n;
    if (n <= 0) continue;
    const float* a = pc.p[0];
    const float* b = pc.p[1];
    float* h = pc.p[2];
    const float* v = pc.p[3];
    float* x = pc.p[4];
    const int head = head_of<4>(h, n);
    const int nvec = (n - head) / 4;
    if (t < head) {
      const float d = a[t] - b[t];
      h[t] = d * s;
      if constexpr (kX) x[t] = v[t] * s;
    }
#pragma unroll 2
    for (int q = t; q < nvec; q += kT) {
      const int i = head + q * 4;
      const f32x4_u aa = *reinterpret_cast<const f32x4_u*>(a + i);
      const f32x4_u bb = *reinterpret_cast<const f32x4_u*>(b + i);
      f32x4 hh;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = aa[e] - bb[e];
        hh[e] = d * s;
      }
      *reinterpret_cast<f32x4*>(h + i) = hh;
      if constexpr (kX) {
        const f32x4_u vv = *reinterpret_cast<const f32x4_u*>(v + i);
        f32x4_u xx;
#pragma unroll
        for (int e = 0; e < 4; ++e) xx[e] = vv[e] * s;
        *reinterpret_cast<f32x4_u*>(x + i) = xx;
      }
    }
    const int i = head + nvec * 4 + t;
    if (i < n) {
      const float d = a[i] - b[i];
      h[i] = d * s;
      if constexpr (kX) x[i] = v[i] * s;
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------------- blend
// m = fl32(fl32(beta m) + fl32(omb g)); !kRead (beta == 0): m = fl32(omb g), m is not read.  The 16-byte body is aligned on m.
template <bool kRead>
__device__ __forceinline__ float blend_one(float m, float g, float beta, float omb) {
  const float b = omb * g;
  if constexpr (!kRead) {
    return b;
  } else {
    const float a = beta * m;
    return a + b;
  }
}

template <bool kRead>
__global__ __launch_bounds__(kT) void k_multi_blend(const Seg* __restrict__ msegs, const Seg* __restrict__ gsegs,
                                                    const Chunk* __restrict__ chunks, int64_t nchunks, int k, float beta, float omb) {
  const int t = threadIdx.x;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Seg* const tabs[2] = {msegs, gsegs};
    const Piece<2> pc = piece_of<2>(tabs, chunks[c], k);
    const int n = pc.n;
    if (n <= 0) continue;
    float* m = pc.p[0];
    const float* g = pc.p[1];
    const int head = head_of<4>(m, n);
    const int nvec = (n - head) / 4;
    if (t < head) m[t] = blend_one<kRead>(kRead ? m[t] : 0.f, g[t], beta, omb);
#pragma unroll 2
    for (int q = t; q < nvec; q += kT) {
      const int i = head + q * 4;
      f32x4 mm = {0.f, 0.f, 0.f, 0.f};
      if constexpr (kRead) mm = *reinterpret_cast<const f32x4*>(m + i);
      const f32x4_u gg = *reinterpret_cast<const f32x4_u*>(g + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) mm[e] = blend_one<kRead>(mm[e], gg[e], beta, omb);
      *reinterpret_cast<f32x4*>(m + i) = mm;
    }
    const int i = head + nvec * 4 + t;
    if (i < n) m[i] = blend_one<kRead>(kRead ? m[i] : 0.f, g[i], beta, omb);
  }
}

// ------------------------------------------------------------------------------------------------------------- scale and check
// one list inside one chunk: y = fl32(x s), stored in place where s != 1 (a list with s == 1 is only read); returns whether a y of
// this lane is not finite.  Every list is its own stored operand: head, body and tail are laid on its own 16-byte boundaries.
__device__ __forceinline__ bool scale_check_list(float* x, int n, float s, int t) {
  const bool store = s != 1.f;
  bool bad = false;
  const int head = head_of<4>(x, n);
  const int nvec = (n - head) / 4;
  if (t < head) {
    const float y = x[t] * s;
    bad |= not_finite(y);
    if (store) x[t] = y;
  }
#pragma unroll 2
  for (int q = t; q < nvec; q += kT) {
    const int i = head + q * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(x + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = v[e] * s;
      bad |= not_finite(v[e]);
    }
    if (store) *reinterpret_cast<f32x4*>(x + i) = v;
  }
  const int i = head + nvec * 4 + t;
  if (i < n) {
    const float y = x[i] * s;
    bad |= not_finite(y);
    if (store) x[i] = y;
  }
  return bad;
}

// A lane that formed a non-finite product stores `stamp` to *flag when it is done -- an ordinary store of one value by every
// writer, from a vector lane under a per-lane predicate: no atomic, no reduction, and nobody zeroes the word (the contract of
// psgd_uvd_pack_check_f32).  flag == nullptr: a pure rescale.
__global__ __launch_bounds__(kT) void k_multi_scale_check(const Seg* __restrict__ segs0, const Seg* __restrict__ segs1,
                                                          const Seg* __restrict__ segs2, float s0, float s1, float s2,
                                                          const Chunk* __restrict__ chunks, int64_t nchunks, int k,
                                                          int32_t* flag, int32_t stamp) {
  const int t = threadIdx.x;
  bool bad = false;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Seg* const tabs[3] = {segs0, segs1, segs2};
    const Piece<3> pc = piece_of<3>(tabs, chunks[c], k);
    const int n = pc.n;
    if (n <= 0) continue;
    bad |= scale_check_list(pc.p[0], n, s0, t);
    if (segs1) bad |= scale_check_list(pc.p[1], n, s1, t);
    if (segs2) bad |= scale_check_list(pc.p[2], n, s2, t);
  }
  if (flag != nullptr && bad) *reinterpret_cast<volatile int32_t*>(flag) = stamp;
}

// ------------------------------------------------------------------------------------- half-precision parameters: widen and check
// one list inside one chunk: dst = fl32(float(src) s), src of type T (bf16 / fp16), dst fp32; returns whether a value this lane
// wrote is not finite.  The stored side is dst: head, body (4 floats = 16 bytes per lane and access, 8 bytes of src through the
// element-aligned type) and tail are laid on its 16-byte boundaries.
template <class T>
__device__ __forceinline__ bool widen_list(const uint16_t* src, float* dst, int n, float s, int t) {
  bool bad = false;
  const int head = head_of<4>(dst, n);
  const int nvec = (n - head) / 4;
  if (t < head) {
    const float y = T::widen(src[t]) * s;
    bad |= not_finite(y);
    dst[t] = y;
  }
#pragma unroll 2
  for (int q = t; q < nvec; q += kT) {
    const int i = head + q * 4;
    const u16x4_u v = *reinterpret_cast<const u16x4_u*>(src + i);
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      y[e] = T::widen(v[e]) * s;
      bad |= not_finite(y[e]);
    }
    *reinterpret_cast<f32x4*>(dst + i) = y;
  }
  const int i = head + nvec * 4 + t;
  if (i < n) {
    const float y = T::widen(src[i]) * s;
    bad |= not_finite(y);
    dst[i] = y;
  }
  return bad;
}

// One to three (source, destination) pairs of lists in one launch; the flag is that of k_multi_scale_check.  A chunk never runs
// past the shortest of its segments, sources and destinations alike.
template <class T>
__global__ __launch_bounds__(kT) void k_multi_widen_check(const Seg* __restrict__ src0, const Seg* __restrict__ src1,
                                                          const Seg* __restrict__ src2, const Seg* __restrict__ dst0,
                                                          const Seg* __restrict__ dst1, const Seg* __restrict__ dst2, float s0,
                                                          float s1, float s2, const Chunk* __restrict__ chunks, int64_t nchunks,
                                                          int k, int32_t* flag, int32_t stamp) {
  const int t = threadIdx.x;
  bool bad = false;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    if ((uint64_t)ch.seg >= (uint64_t)k || ch.off < 0) continue;     // a table that does not belong to these segments moves nothing
    const Seg* const srcs[3] = {src0, src1, src2};
    const Seg* const dsts[3] = {dst0, dst1, dst2};
    const float scales[3] = {s0, s1, s2};
    const uint16_t* sp[3] = {nullptr, nullptr, nullptr};
    float* dp[3] = {nullptr, nullptr, nullptr};
    int64_t left = kChunk;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (!srcs[j]) continue;
      const Seg a = srcs[j][ch.seg];
      const Seg b = dsts[j][ch.seg];
      const int64_t l = (a.count < b.count ? a.count : b.count) - ch.off;
      left = l < left ? l : left;
      sp[j] = reinterpret_cast<const uint16_t*>(a.ptr) + ch.off;
      dp[j] = reinterpret_cast<float*>(b.ptr) + ch.off;
    }
    if (left <= 0) continue;
    const int n = (int)left;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (srcs[j]) bad |= widen_list<T>(sp[j], dp[j], n, scales[j], t);
  }
  if (flag != nullptr && bad) *reinterpret_cast<volatile int32_t*>(flag) = stamp;
}

// ---------------------------------------------------------------------------------------------------------------- vector layers
// A vector of length n is the reference's layer of shape [1, n] in the (dense, scaling) format: Ql = [[ql]], qr = [1, n].  One
// workgroup owns one vector (workgroup b takes vectors b, b + grid, ...): what a vector gets depends on its own n and values only,
// never on k, on its place in the list or on where its tensors start.  Segments of the tables: ql has one element, the others n; a
// vector shorter than 2 (or a table whose counts disagree below 2) moves nothing.
//
// Update (psgd.py:276-307 with M = 1), fp32 in the reference's order, three phases between two workgroup barriers; the vector is
// read again from cache in every phase, so any n works (a vector of a million elements is correct and slow: one workgroup):
//   1. m = max(qr);  rho = sqrt(ql / m);  ql' = ql / rho;  qr' = rho qr                                              (:288-292)
//   2. A = (ql' dG) qr';  Bt = (dX / ql') (1 / qr');  sum A^2, sum Bt^2 (fp64 sums of the fp32 squares);  max |A^2 - Bt^2|
//   3. grad1 = sum A^2 - sum Bt^2;  ql <- ql' - (step1 grad1) ql';  qr <- qr' - (step2 grad2) qr'                   (:301-307)
//      step1 = step / (|grad1| + tiny),  step2 = step / (max |grad2| + tiny)
// Lane t takes the elements 4 (t + 256 j) .. + 3 and the last n mod 4 go to lanes 0 .. 2, whatever the alignment (every access is
// through the element-aligned vector type), each lane accumulates its squares in fp64 in index order, and the lanes are folded
// lanes -> waves -> workgroup in a fixed order: no atomics, the same bits on every call.  The maxima propagate NaN (nanmax.h).
struct VecFold {
  float m1[kT / 64];        // phase 1: max(qr)
  double sa[kT / 64];       // phase 2: sum A^2, sum Bt^2, max |grad2|
  double sb[kT / 64];
  float m2[kT / 64];
};

// every lane runs `one(i)` for its single elements and `four(i)` for its groups of four consecutive ones
template <class F1, class F4>
__device__ __forceinline__ void vec_sweep(int n, int head, int t, F1 one, F4 four) {
  const int nvec = (n - head) / 4;
  if (t < head) one(t);
#pragma unroll 2
  for (int q = t; q < nvec; q += kT) four(head + 4 * q);
  const int i = head + nvec * 4 + t;
  if (i < n) one(i);
}

__device__ __forceinline__ float wave_nmax(float v) {
  for (int o = 32; o > 0; o >>= 1) v = psgd::nmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// A^2, Bt^2 of one element as the reference forms them
__device__ __forceinline__ void vec_squares(float qlp, float rho, float qr, float dx, float dg, float& qrp, float& a2, float& b2) {
  qrp = rho * qr;
  const float a = (qlp * dg) * qrp;
  const float inv = 1.0f / qrp;
  const float bt = (dx / qlp) * inv;
  a2 = a * a;
  b2 = bt * bt;
}

__global__ __launch_bounds__(kT) void k_multi_vec_update(const Seg* __restrict__ qlsegs, const Seg* __restrict__ qrsegs,
                                                         const Seg* __restrict__ dxsegs, const Seg* __restrict__ dgsegs, int k,
                                                         float step, float tiny) {
  __shared__ VecFold lds;
  const int t = threadIdx.x;
  const int w = t >> 6;
  for (int s = blockIdx.x; s < k; s += gridDim.x) {
    const Seg sl = qlsegs[s], sr = qrsegs[s], sx = dxsegs[s], sg = dgsegs[s];
    int64_t cnt = sr.count < sx.count ? sr.count : sx.count;
    cnt = sg.count < cnt ? sg.count : cnt;
    if (sl.count < 1 || cnt < 2 || cnt > 0x7fffffff) continue;      // (the same for every lane of the workgroup)
    const int n = (int)cnt;
    float* qlptr = reinterpret_cast<float*>(sl.ptr);
    float* qr = reinterpret_cast<float*>(sr.ptr);
    const float* dX = reinterpret_cast<const float*>(sx.ptr);
    const float* dG = reinterpret_cast<const float*>(sg.ptr);
    const float ql = qlptr[0];
    // ---- phase 1: max(qr)
    float m = __uint_as_float(0xff800000u);                         // -inf
    vec_sweep(n, 0, t, [&](int i) { m = psgd::nmaxf(m, qr[i]); },
              [&](int i) {
                const f32x4_u v = *reinterpret_cast<const f32x4_u*>(qr + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) m = psgd::nmaxf(m, v[e]);
              });
    m = wave_nmax(m);
    if ((t & 63) == 0) lds.m1[w] = m;
    __syncthreads();
    m = lds.m1[0];
#pragma unroll
    for (int j = 1; j < kT / 64; ++j) m = psgd::nmaxf(m, lds.m1[j]);
    const float rho = sqrtf(ql / m);                                // :288-290
    const float qlp = ql / rho;                                     // :291
    // ---- phase 2: the two sums and max |grad2|
    double sa = 0.0, sb = 0.0;
    float mx = 0.f;
    vec_sweep(n, 0, t,
              [&](int i) {
                float qrp, a2, b2;
                vec_squares(qlp, rho, qr[i], dX[i], dG[i], qrp, a2, b2);
                sa += (double)a2;
                sb += (double)b2;
                mx = psgd::amaxf(mx, fabsf(a2 - b2));
              },
              [&](int i) {
                const f32x4_u vr = *reinterpret_cast<const f32x4_u*>(qr + i);
                const f32x4_u vx = *reinterpret_cast<const f32x4_u*>(dX + i);
                const f32x4_u vg = *reinterpret_cast<const f32x4_u*>(dG + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  float qrp, a2, b2;
                  vec_squares(qlp, rho, vr[e], vx[e], vg[e], qrp, a2, b2);
                  sa += (double)a2;
                  sb += (double)b2;
                  mx = psgd::amaxf(mx, fabsf(a2 - b2));
                }
              });
    sa = wave_sum(sa);
    sb = wave_sum(sb);
    for (int o = 32; o > 0; o >>= 1) mx = psgd::amaxf(mx, __shfl_xor(mx, o, 64));
    if ((t & 63) == 0) {
      lds.sa[w] = sa;
      lds.sb[w] = sb;
      lds.m2[w] = mx;
    }
    __syncthreads();
    sa = lds.sa[0];
    sb = lds.sb[0];
    mx = lds.m2[0];
#pragma unroll
    for (int j = 1; j < kT / 64; ++j) {
      sa += lds.sa[j];
      sb += lds.sb[j];
      mx = psgd::amaxf(mx, lds.m2[j]);
    }
    // ---- phase 3: the new factors                                  (:301-307)
    const float grad1 = (float)(sa - sb);
    const float step1 = step / (fabsf(grad1) + tiny);
    const float step2 = step / (mx + tiny);
    vec_sweep(n, 0, t,
              [&](int i) {
                float qrp, a2, b2;
                vec_squares(qlp, rho, qr[i], dX[i], dG[i], qrp, a2, b2);
                const float g2 = a2 - b2;
                qr[i] = qrp - (step2 * g2) * qrp;
              },
              [&](int i) {
                f32x4_u vr = *reinterpret_cast<const f32x4_u*>(qr + i);
                const f32x4_u vx = *reinterpret_cast<const f32x4_u*>(dX + i);
                const f32x4_u vg = *reinterpret_cast<const f32x4_u*>(dG + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  float qrp, a2, b2;
                  vec_squares(qlp, rho, vr[e], vx[e], vg[e], qrp, a2, b2);
                  const float g2 = a2 - b2;
                  vr[e] = qrp - (step2 * g2) * qrp;
                }
                *reinterpret_cast<f32x4_u*>(qr + i) = vr;
              });
    // every lane read ql before the first barrier; lds.m1 is next written after this vector's second barrier, lds.sa / sb / m2
    // after the next vector's first one: two barriers per vector are enough
    if (t == 0) qlptr[0] = qlp - (step1 * grad1) * qlp;
  }
}

// out = fl32(fl32(fl32(ql ql) g) fl32(qr qr)).  Streaming: a scalar head to the 16-byte boundary of out, 4 floats per lane and access,
// a scalar tail; g and qr through the element-aligned type.  out may be g: every element is read and written by one lane.
__global__ __launch_bounds__(kT) void k_multi_vec_apply(const Seg* __restrict__ qlsegs, const Seg* __restrict__ qrsegs,
                                                        const Seg* __restrict__ gsegs, const Seg* __restrict__ osegs, int k) {
  const int t = threadIdx.x;
  for (int s = blockIdx.x; s < k; s += gridDim.x) {
    const Seg sl = qlsegs[s], sr = qrsegs[s], sg = gsegs[s], so = osegs[s];
    int64_t cnt = sr.count < sg.count ? sr.count : sg.count;
    cnt = so.count < cnt ? so.count : cnt;
    if (sl.count < 1 || cnt < 2 || cnt > 0x7fffffff) continue;
    const int n = (int)cnt;
    const float* qr = reinterpret_cast<const float*>(sr.ptr);
    const float* g = reinterpret_cast<const float*>(sg.ptr);
    float* out = reinterpret_cast<float*>(so.ptr);
    const float ql = reinterpret_cast<const float*>(sl.ptr)[0];
    const float ql2 = ql * ql;
    vec_sweep(n, head_of<4>(out, n), t,
              [&](int i) {
                const float r = qr[i];
                out[i] = (ql2 * g[i]) * (r * r);
              },
              [&](int i) {
                const f32x4_u vr = *reinterpret_cast<const f32x4_u*>(qr + i);
                const f32x4_u vg = *reinterpret_cast<const f32x4_u*>(g + i);
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (ql2 * vg[e]) * (vr[e] * vr[e]);
                *reinterpret_cast<f32x4*>(out + i) = o;
              });
  }
}

// ------------------------------------------------------------------------------ bf16 operands of class Kron: narrow, mixed lists
// one list inside one chunk: dst = bf16(src), round to nearest even (BF16::narrow: NaN -> quiet NaN, a finite value beyond the bf16
// range -> +-Inf).  The stored side is dst: a scalar head to its 16-byte boundary, a body of 8 elements per lane and access (two
// 16-byte reads of src through the element-aligned type, one 16-byte store), a scalar tail.
__device__ __forceinline__ void narrow_list(const float* src, uint16_t* dst, int n, int t) {
  const int head = head_of<2>(dst, n);
  const int nvec = (n - head) / 8;
  if (t < head) dst[t] = BF16::narrow(src[t]);
#pragma unroll 2
  for (int q = t; q < nvec; q += kT) {
    const int i = head + q * 8;
    u16x8 y;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const f32x4_u w = *reinterpret_cast<const f32x4_u*>(src + i + 4 * b);
#pragma unroll
      for (int e = 0; e < 4; ++e) y[4 * b + e] = BF16::narrow(w[e]);
    }
    *reinterpret_cast<u16x8*>(dst + i) = y;
  }
  const int i = head + nvec * 8 + t;
  if (i < n) dst[i] = BF16::narrow(src[i]);
}

// One to three (source, destination) pairs of lists in one launch: k_multi_widen_check in the other direction, without a flag.
__global__ __launch_bounds__(kT) void k_multi_narrow_bf16(const Seg* __restrict__ src0, const Seg* __restrict__ src1,
                                                          const Seg* __restrict__ src2, const Seg* __restrict__ dst0,
                                                          const Seg* __restrict__ dst1, const Seg* __restrict__ dst2,
                                                          const Chunk* __restrict__ chunks, int64_t nchunks, int k) {
  const int t = threadIdx.x;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    if ((uint64_t)ch.seg >= (uint64_t)k || ch.off < 0) continue;     // a table that does not belong to these segments moves nothing
    const Seg* const srcs[3] = {src0, src1, src2};
    const Seg* const dsts[3] = {dst0, dst1, dst2};
    const float* sp[3] = {nullptr, nullptr, nullptr};
    uint16_t* dp[3] = {nullptr, nullptr, nullptr};
    int64_t left = kChunk;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (!srcs[j]) continue;
      const Seg a = srcs[j][ch.seg];
      const Seg b = dsts[j][ch.seg];
      const int64_t l = (a.count < b.count ? a.count : b.count) - ch.off;
      left = l < left ? l : left;
      sp[j] = reinterpret_cast<const float*>(a.ptr) + ch.off;
      dp[j] = reinterpret_cast<uint16_t*>(b.ptr) + ch.off;
    }
    if (left <= 0) continue;
    const int n = (int)left;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (srcs[j]) narrow_list(sp[j], dp[j], n, t);
  }
}

// The MIXED lists: every segment of the gradient list is fp32 or bf16, and its `start` field -- which no list kernel reads --
// holds its PSGD_DTYPE_* code.  A segment with any other code moves nothing: the tables live on the device and the host cannot
// judge them.  (The update that takes such a list: GradMixed of psgd_param_update.hip.)

// k_multi_sumsq_partial on a mixed list.  An fp32 segment is summed exactly as there (the same lanes take the same elements in the
// same order: the same bits).  A bf16 segment is summed as that kernel sums a 16-BYTE ALIGNED fp32 tensor of the widened values --
// no head, lane t takes the groups of four at 4 (t + 256 j), then the tail -- wherever the bf16 tensor starts: 8 bytes per lane
// and access through the element-aligned type.
__global__ __launch_bounds__(kT) void k_multi_sumsq_partial_mixed(const Seg* __restrict__ segs, const Chunk* __restrict__ chunks,
                                                                  int64_t nchunks, int k, double* __restrict__ partial) {
  __shared__ double lds[kT / 64];
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    if ((uint64_t)ch.seg >= (uint64_t)k || ch.off < 0) continue;
    const Seg s = segs[ch.seg];
    int64_t left = s.count - ch.off;
    left = left < kChunk ? left : kChunk;
    if (left <= 0) continue;
    const int n = (int)left;
    if (s.start == PSGD_DTYPE_F32) {
      acc = sumsq_piece_f32(acc, reinterpret_cast<const float*>(s.ptr) + ch.off, n, t);
    } else if (s.start == PSGD_DTYPE_BF16) {
      const uint16_t* x = reinterpret_cast<const uint16_t*>(s.ptr) + ch.off;
      const int nvec = n / 4;
#pragma unroll 2
      for (int g = t; g < nvec; g += kT) {
        const u16x4_u v = *reinterpret_cast<const u16x4_u*>(x + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float w = BF16::widen(v[e]);
          acc += (double)(w * w);
        }
      }
      const int i = nvec * 4 + t;
      if (i < n) {
        const float w = BF16::widen(x[i]);
        acc += (double)(w * w);
      }
    }
  }
  const double s = block_sum(acc, lds);
  if (t == 0) partial[blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------- probe vectors: counter-based normals
// psgd_multi_randn_f32: element i of the concatenation of the list (i = index0 + the segment's `start` + the offset inside it) gets
// fl32(scale * z_i), z_i a function of (seed, i) alone.  Stream: K = key64(seed, tensor id 17) (bf16_state.h); pair j = i >> 1 takes
// ONE 64-bit hash h = mix64(K + 0x9E3779B97F4A7C15 (j + 1)) -- the splitmix64 sequence started at K -- and Box-Muller on its words:
//   hi = h >> 32:   u1 = (hi + 1) 2^-32, in (0, 1];   r = sqrt(-2 ln u1), in [0, 6.67]
//   lo = h & M32:   theta = 2 pi lo 2^-32
//   z_{2j} = fl32(r cos theta),   z_{2j+1} = fl32(r sin theta)         (parity of the GLOBAL index: a segment that starts on an odd
//                                                                       index starts with the sine half of a pair)
// Evaluated in fp32 with the full-precision logf / log1pf / sqrtf / sincospif, arranged so that no input rounding is amplified:
// for u1 <= 1/2, ln u1 = logf(fl32(hi + 1) 2^-32) (a relative error of 2^-24 in u1 moves r by less than 1e-7); for u1 > 1/2,
// ln u1 = log1pf(-w) with w = 1 - u1 = fl32(2^32 - 1 - hi) 2^-32 <= 1/2, which keeps r's RELATIVE accuracy down to r = 0 (logf of
// a u1 rounded to 24 bits would not: near u1 = 1 it loses r altogether); theta enters as sincospif(x), x = int32(lo) 2^-31 in
// [-1, 1), the same angle modulo 2 pi with |x| small where fl32(lo) would round.  FINITE BY CONSTRUCTION: u1 > 0, so ln u1 >= -32 ln 2
// and r <= 6.67; u1 <= 1, so the radicand is >= 0 (never NaN); sin and cos are in [-1, 1]: no Inf and no NaN whatever the seed --
// with a finite scale of ordinary size class Kron's guard does not judge these vectors, and relies on this.
// The value of an element does not depend on the lane, the chunk, the grid, where a tensor starts or how the list is cut: every
// path below calls the one randn_pair.  A lane that owns both halves of a pair hashes once.  Accesses: a scalar head to the 16-byte
// boundary of the segment's piece, 4 floats per lane and store, a scalar tail.  The kernel only writes.
__device__ __forceinline__ void randn_pair(uint64_t K, uint64_t j, float& zc, float& zs) {
  const uint64_t h = psgd::bf16s::mix64(K + 0x9E3779B97F4A7C15ull * (j + 1ull));
  const uint32_t hi = (uint32_t)(h >> 32), lo = (uint32_t)h;
  float nl;                                                              // -ln u1 >= 0
  if (hi < 0x80000000u)
    nl = -logf((float)(hi + 1u) * 0x1p-32f);
  else
    nl = -log1pf(-((float)(~hi) * 0x1p-32f));
  const float r = sqrtf(2.0f * nl);
  float s, c;
  sincospif((float)(int32_t)lo * 0x1p-31f, &s, &c);
  zc = r * c;
  zs = r * s;
}

__device__ __forceinline__ float randn_one(uint64_t K, uint64_t i, float scale) {
  float zc, zs;
  randn_pair(K, i >> 1, zc, zs);
  return scale * ((i & 1ull) ? zs : zc);
}

__global__ __launch_bounds__(kT) void k_multi_randn(const Seg* __restrict__ segs, const Chunk* __restrict__ chunks, int64_t nchunks,
                                                    int k, uint64_t K, unsigned long long index0, float scale) {
  const int t = threadIdx.x;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    if ((uint64_t)ch.seg >= (uint64_t)k || ch.off < 0) continue;     // a table that does not belong to these segments moves nothing
    const Seg sg = segs[ch.seg];
    int64_t left = sg.count - ch.off;
    left = left < kChunk ? left : kChunk;
    if (left <= 0) continue;
    const int n = (int)left;
    float* out = reinterpret_cast<float*>(sg.ptr) + ch.off;
    const uint64_t i0 = index0 + (uint64_t)(sg.start + ch.off);
    const int head = head_of<4>(out, n);
    const int nvec = (n - head) / 4;
    if (t < head) out[t] = randn_one(K, i0 + (unsigned)t, scale);
    const bool odd = ((i0 + (unsigned)head) & 1ull) != 0;              // the same for every group of four of this piece
#pragma unroll 2
    for (int q = t; q < nvec; q += kT) {
      const int i = head + q * 4;
      const uint64_t j = (i0 + (unsigned)i) >> 1;
      float c0, s0, c1, s1;
      randn_pair(K, j, c0, s0);
      randn_pair(K, j + 1, c1, s1);
      f32x4 v;
      if (!odd) {                       // two whole pairs
        v[0] = c0; v[1] = s0; v[2] = c1; v[3] = s1;
      } else {                          // the sine half of pair j, pair j + 1, the cosine half of pair j + 2
        float c2, s2;
        randn_pair(K, j + 2, c2, s2);
        v[0] = s0; v[1] = c1; v[2] = s1; v[3] = c2;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = scale * v[e];
      *reinterpret_cast<f32x4*>(out + i) = v;
    }
    const int i = head + nvec * 4 + t;
    if (i < n) out[i] = randn_one(K, i0 + (unsigned)i, scale);
  }
}

}  // namespace psgdm

using namespace psgdm;

extern "C" {

int psgd_multi_sumsq_f32(const void* segs, int k, const void* chunks, int64_t nchunks, double* out, void* ws, int64_t ws_bytes,
                         void* stream) {
  if (!segs || !chunks || !out || ((uintptr_t)out & 7) || !ws || k < 0 || nchunks < 0) return PSGD_ERR_BAD_ARG;
  if (ws_bytes < PSGD_MULTI_SUMSQ_WS_BYTES || ((uintptr_t)ws & 7)) return PSGD_ERR_WORKSPACE;
  if (nchunks == 0) return PSGD_OK;                                           // out is NOT written: the sum of nothing is the caller's
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)(nchunks < kSumsqBlocks ? nchunks : kSumsqBlocks);      // a function of nchunks alone: the partition never changes
  hipLaunchKernelGGL(k_multi_sumsq_partial, dim3(nb), dim3(kT), 0, st, (const Seg*)segs, (const Chunk*)chunks, nchunks, k,
                     (double*)ws);
  hipLaunchKernelGGL(k_sumsq_fold, dim3(1), dim3(kT), 0, st, (const double*)ws, nb, out);
  return launched();
}

int psgd_multi_blend_f32(const void* m_segs, const void* g_segs, int k, const void* chunks, int64_t nchunks, float beta, float omb,
                         void* stream) {
  if (!m_segs || !g_segs || !chunks || k < 0 || nchunks < 0) return PSGD_ERR_BAD_ARG;
  if (nchunks == 0) return PSGD_OK;
  hipStream_t st = (hipStream_t)stream;
  const Chunk* ch = (const Chunk*)chunks;
  const int grid = grid_for(nchunks);
  if (beta == 0.f)
    hipLaunchKernelGGL(k_multi_blend<false>, dim3(grid), dim3(kT), 0, st, (const Seg*)m_segs, (const Seg*)g_segs, ch, nchunks, k,
                       beta, omb);
  else
    hipLaunchKernelGGL(k_multi_blend<true>, dim3(grid), dim3(kT), 0, st, (const Seg*)m_segs, (const Seg*)g_segs, ch, nchunks, k,
                       beta, omb);
  return launched();
}

int psgd_multi_scale_check_f32(const void* segs0, const void* segs1, const void* segs2, float scale0, float scale1, float scale2,
                               int k, const void* chunks, int64_t nchunks, int32_t* flag, int32_t stamp, void* stream) {
  if (!segs0 || !chunks || k < 0 || nchunks < 0) return PSGD_ERR_BAD_ARG;
  if (flag) {
    if (stamp <= 0 || ((uintptr_t)flag & 3)) return PSGD_ERR_BAD_ARG;
  } else if (scale0 == 1.f && (!segs1 || scale1 == 1.f) && (!segs2 || scale2 == 1.f)) {
    return PSGD_ERR_BAD_ARG;                                                 // nothing to check and nothing to scale
  }
  if (nchunks == 0) return PSGD_OK;
  hipLaunchKernelGGL(k_multi_scale_check, dim3(grid_for(nchunks)), dim3(kT), 0, (hipStream_t)stream, (const Seg*)segs0,
                     (const Seg*)segs1, (const Seg*)segs2, scale0, scale1, scale2, (const Chunk*)chunks, nchunks, k, flag, stamp);
  return launched();
}

int psgd_multi_diff_scale_f32(const void* a_segs, const void* b_segs, const void* h_segs, const void* v_segs, const void* x_segs,
                              int k, const void* chunks, int64_t nchunks, float s, void* stream) {
  if (!a_segs || !b_segs || !h_segs || !chunks || k < 0 || nchunks < 0) return PSGD_ERR_BAD_ARG;
  if ((v_segs == nullptr) != (x_segs == nullptr)) return PSGD_ERR_BAD_ARG;   // v and x go together
  if (nchunks == 0) return PSGD_OK;
  hipStream_t st = (hipStream_t)stream;
  const Chunk* ch = (const Chunk*)chunks;
  const int grid = grid_for(nchunks);
  if (x_segs)
    hipLaunchKernelGGL(k_multi_diff_scale<true>, dim3(grid), dim3(kT), 0, st, (const Seg*)a_segs, (const Seg*)b_segs,
                       (const Seg*)h_segs, (const Seg*)v_segs, (const Seg*)x_segs, ch, nchunks, k, s);
  else
    hipLaunchKernelGGL(k_multi_diff_scale<false>, dim3(grid), dim3(kT), 0, st, (const Seg*)a_segs, (const Seg*)b_segs,
                       (const Seg*)h_segs, (const Seg*)v_segs, (const Seg*)x_segs, ch, nchunks, k, s);
  return launched();
}

int psgd_multi_widen_check(const void* src0, const void* src1, const void* src2, const void* dst0, const void* dst1, const void* dst2,
                           float scale0, float scale1, float scale2, int k, const void* chunks, int64_t nchunks, int dtype,
                           int32_t* flag, int32_t stamp, void* stream) {
  if (!src0 || !dst0 || !chunks || k < 0 || nchunks < 0) return PSGD_ERR_BAD_ARG;
  if ((src1 == nullptr) != (dst1 == nullptr) || (src2 == nullptr) != (dst2 == nullptr)) return PSGD_ERR_BAD_ARG;
  if (dtype != PSGD_DTYPE_BF16 && dtype != PSGD_DTYPE_F16) return PSGD_ERR_BAD_ARG;      // fp32 lists: psgd_multi_scale_check_f32
  if (flag && (stamp <= 0 || ((uintptr_t)flag & 3))) return PSGD_ERR_BAD_ARG;
  if (nchunks == 0) return PSGD_OK;
  hipStream_t st = (hipStream_t)stream;
  const int grid = grid_for(nchunks);
  if (dtype == PSGD_DTYPE_BF16)
    hipLaunchKernelGGL(k_multi_widen_check<BF16>, dim3(grid), dim3(kT), 0, st, (const Seg*)src0, (const Seg*)src1, (const Seg*)src2,
                       (const Seg*)dst0, (const Seg*)dst1, (const Seg*)dst2, scale0, scale1, scale2, (const Chunk*)chunks, nchunks, k,
                       flag, stamp);
  else
    hipLaunchKernelGGL(k_multi_widen_check<F16>, dim3(grid), dim3(kT), 0, st, (const Seg*)src0, (const Seg*)src1, (const Seg*)src2,
                       (const Seg*)dst0, (const Seg*)dst1, (const Seg*)dst2, scale0, scale1, scale2, (const Chunk*)chunks, nchunks, k,
                       flag, stamp);
  return launched();
}

int psgd_multi_vec_update_f32(const void* ql_segs, const void* qr_segs, const void* dx_segs, const void* dg_segs, int k,
                              int64_t min_count, float step, float tiny, void* stream) {
  if (!ql_segs || !qr_segs || !dx_segs || !dg_segs || k < 1 || min_count < 2) return PSGD_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_multi_vec_update, dim3(grid_for(k)), dim3(kT), 0, (hipStream_t)stream, (const Seg*)ql_segs,
                     (const Seg*)qr_segs, (const Seg*)dx_segs, (const Seg*)dg_segs, k, step, tiny);
  return launched();
}

int psgd_multi_vec_apply_f32(const void* ql_segs, const void* qr_segs, const void* g_segs, const void* out_segs, int k,
                             int64_t min_count, void* stream) {
  if (!ql_segs || !qr_segs || !g_segs || !out_segs || k < 1 || min_count < 2) return PSGD_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_multi_vec_apply, dim3(grid_for(k)), dim3(kT), 0, (hipStream_t)stream, (const Seg*)ql_segs,
                     (const Seg*)qr_segs, (const Seg*)g_segs, (const Seg*)out_segs, k);
  return launched();
}

int psgd_multi_narrow_bf16(const void* src0, const void* src1, const void* src2, const void* dst0, const void* dst1, const void* dst2,
                           int k, const void* chunks, int64_t nchunks, void* stream) {
  if (!src0 || !dst0 || !chunks || k < 0 || nchunks < 0) return PSGD_ERR_BAD_ARG;
  if ((src1 == nullptr) != (dst1 == nullptr) || (src2 == nullptr) != (dst2 == nullptr)) return PSGD_ERR_BAD_ARG;
  if (nchunks == 0) return PSGD_OK;
  hipLaunchKernelGGL(k_multi_narrow_bf16, dim3(grid_for(nchunks)), dim3(kT), 0, (hipStream_t)stream, (const Seg*)src0,
                     (const Seg*)src1, (const Seg*)src2, (const Seg*)dst0, (const Seg*)dst1, (const Seg*)dst2, (const Chunk*)chunks,
                     nchunks, k);
  return launched();
}

int psgd_multi_sumsq_mixed(const void* segs, int k, const void* chunks, int64_t nchunks, double* out, void* ws, int64_t ws_bytes,
                           void* stream) {
  if (!segs || !chunks || !out || ((uintptr_t)out & 7) || !ws || k < 0 || nchunks < 0) return PSGD_ERR_BAD_ARG;
  if (ws_bytes < PSGD_MULTI_SUMSQ_WS_BYTES || ((uintptr_t)ws & 7)) return PSGD_ERR_WORKSPACE;
  if (nchunks == 0) return PSGD_OK;                                           // out is NOT written, as in psgd_multi_sumsq_f32
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)(nchunks < kSumsqBlocks ? nchunks : kSumsqBlocks);      // the partition of psgd_multi_sumsq_f32
  hipLaunchKernelGGL(k_multi_sumsq_partial_mixed, dim3(nb), dim3(kT), 0, st, (const Seg*)segs, (const Chunk*)chunks, nchunks, k,
                     (double*)ws);
  hipLaunchKernelGGL(k_sumsq_fold, dim3(1), dim3(kT), 0, st, (const double*)ws, nb, out);
  return launched();
}

int psgd_multi_randn_f32(const void* out_segs, int k, const void* chunks, int64_t nchunks, uint64_t seed, int64_t index0, float scale,
                         void* stream) {
  if (!out_segs || !chunks || k < 1 || nchunks < 0 || index0 < 0) return PSGD_ERR_BAD_ARG;
  if ((__builtin_bit_cast(uint32_t, scale) & 0x7F800000u) == 0x7F800000u) return PSGD_ERR_BAD_ARG;      // +-Inf, NaN
  if (nchunks == 0) return PSGD_OK;
  const uint64_t K = psgd::bf16s::key64(seed, 17u);                          // tensor id 17: the probe vectors (bf16_state.h)
  hipLaunchKernelGGL(k_multi_randn, dim3(grid_for(nchunks)), dim3(kT), 0, (hipStream_t)stream, (const Seg*)out_segs,
                     (const Chunk*)chunks, nchunks, k, K, (unsigned long long)index0, scale);
  return launched();
}

}  // extern "C"
