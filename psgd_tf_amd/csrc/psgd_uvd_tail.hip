// psgd_uvd_tail.hip -- the tail of UVd.step (psgd.py:729-730, :747, :750-762) on gfx950, whatever the number of parameter tensors.
//
//   psgd_uvd_pack_f32            k tensors of one dtype (fp32 / bf16 / fp16) -> one flat fp32 vector, times a scale      (:729-736, :747)
//   psgd_uvd_pack_blend_f32      the same pack blended into the flat vector: out <- fl32(fl32(beta out) + fl32(omb x))  (momentum of class UVd)
//   psgd_uvd_pack_check_f32      the plain pack, and a stamp stored to a flag word when a written value is not finite     (guarded step)
//   psgd_uvd_check_multi         the same predicate on the same tables; writes the flag alone (the gradients before a blend)
//   psgd_uvd_sumsq_f32           sum x^2 of a flat fp32 vector -> one device double (the clip norm's square)              (:753)
//   psgd_uvd_param_update_multi  p <- T(p - [T(T(fl32(lr_eff pre_grad)) + v)])  for every element of every parameter      (:757-762)
//   psgd_uvd_param_update_multi_wd  ... with decoupled weight decay: delta <- T(delta + T(fl32(fl32(lr_eff wd) p)))
//   psgd_uvd_param_update_multi_sr  bf16 parameters, the update formed once in fp32 and narrowed once, stochastically
//
// The work of pack and update is described by two device tables.  A SEGMENT is one tensor: {pointer, start offset in the flat vector,
// element count}.  A CHUNK is one piece of at most kChunk consecutive elements of one segment: {segment index, offset inside it}; the
// host builds the chunk table once from the sizes, every flat element belongs to exactly one chunk, and a workgroup takes whole chunks
// (grid-stride): nothing searches.  One launch serves any k.
//
// HBM-bound streaming: inside a chunk the stored side (the flat vector for pack, the parameters for the update) is brought to a
// 16-byte boundary by a scalar head, the body moves 16 bytes of the narrowest type per lane and access (4 fp32 or 8 half-precision
// elements), a scalar tail finishes.  The other streams of the body are read through vector types whose declared alignment is the
// element's, so tensors that start at any element (offset views, odd sizes in front of them) still take wide loads.
//
// The sum of squares rounds each product to fp32 (as the torch expression it replaces does), accumulates in fp64 per lane, folds
// lanes -> waves -> workgroup in a fixed order into one fp64 partial per workgroup, and a second one-workgroup launch folds the
// partials in index order: no floating-point atomics, the same bits on every call.
//
// No entry point allocates or synchronises; argument checks return before any HIP call.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "psgd_hip.h"
#include "tail_types.h"
#include "bf16_state.h"

// The roundings of this file are its contract (bit-equal to the torch expressions it replaces): no product may be fused into a
// following sum.  hipcc contracts by default, and the header's __fmul_rn / __fadd_rn are compiled under that default: plain
// operators under this pragma are what stays unfused (checked in the ISA: no v_fma / v_fmac / v_pk_fma on fp32).
#pragma clang fp contract(off)

namespace psgdt {

constexpr int kT = 256;                    // threads per workgroup
constexpr int kChunk = PSGD_UVD_TAIL_CHUNK;
constexpr int kMaxGrid = 2048;             // 8 workgroups per CU; the rest is grid-stride
constexpr int kSumsqBlocks = 1024;         // partials of the sum of squares: PSGD_UVD_SUMSQ_WS_BYTES / 8
static_assert(kSumsqBlocks * 8 == PSGD_UVD_SUMSQ_WS_BYTES, "workspace constant of the header");

struct Seg {
  uint64_t ptr;
  int64_t start, count;
};
struct Chunk {
  int64_t seg, off;
};

// F32 / BF16 / F16 (the dtype codes of the C ABI), their conversions and the 16-byte accesses: tail_types.h
using namespace psgdtt;

// elements in front of the first 16-byte boundary at or after p (elements of `bytes` bytes), at most n
__device__ __forceinline__ int head_of(const void* p, int bytes, int n) {
  const int h = (int)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / bytes;
  return h < n ? h : n;
}

// ------------------------------------------------------------------------------------------------------------------------- pack
// kBlend (psgd_uvd_pack_blend_f32): x = fl32(widen(t) * scale) as in the plain pack, then out = fl32(fl32(beta * out) + fl32(omb * x)),
// every operation rounded on its own.  kBlend && !kRead (beta == 0): out = fl32(omb * x), the flat vector is NOT read -- whatever
// it held (NaN of a fresh allocation included) is gone after the first step.
template <bool kBlend, bool kRead>
__device__ __forceinline__ float pack_one(float x, float old, float scale, float beta, float omb) {
  x = x * scale;
  if constexpr (!kBlend) return x;
  const float nx = omb * x;
  if constexpr (!kRead) return nx;
  const float bo = beta * old;
  return bo + nx;
}

// The non-finite predicate of the guarded step, on a value as it is WRITTEN: exponent all ones (+-Inf, NaN).
__device__ __forceinline__ bool not_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u; }

// kCheck (psgd_uvd_pack_check_f32): the plain pack, and a lane that wrote a non-finite value stores `stamp` to *flag when it is
// done -- an ordinary store of one value by every writer: no atomic, no reduction, and nobody zeroes the word (the host passes a
// stamp it has not used before and reads "bad" as *flag == stamp once the launch has completed).
template <class T, bool kBlend = false, bool kRead = false, bool kCheck = false>
__global__ __launch_bounds__(kT) void k_uvd_pack(const Seg* __restrict__ segs, const Chunk* __restrict__ chunks, int64_t nchunks,
                                                 int k, float scale, float beta, float omb, float* __restrict__ out,
                                                 int32_t* __restrict__ flag, int32_t stamp) {
  using raw = typename T::raw;
  constexpr int E = T::E;
  const int t = threadIdx.x;
  bool bad = false;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    if ((uint64_t)ch.seg >= (uint64_t)k) continue;              // a table that does not belong to these segments moves nothing
    const Seg s = segs[ch.seg];
    const int64_t left = s.count - ch.off;
    if (ch.off < 0 || left <= 0) continue;
    const int n = (int)(left < kChunk ? left : kChunk);
    const raw* src = reinterpret_cast<const raw*>(s.ptr) + ch.off;
    float* dst = out + s.start + ch.off;
    const int head = head_of(dst, 4, n);
    const int nvec = (n - head) / E;
    if (t < head) {
      const float y = pack_one<kBlend, kRead>(T::widen(src[t]), kRead ? dst[t] : 0.f, scale, beta, omb);
      if constexpr (kCheck) bad |= not_finite(y);
      dst[t] = y;
    }
#pragma unroll 2
    for (int g = t; g < nvec; g += kT) {
      const int i = head + g * E;
      float x[E], o[E];
      load_any<T>(src + i, x);
      if constexpr (kRead) {
#pragma unroll
        for (int q = 0; q < E / 4; ++q) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(dst + i + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) o[4 * q + e] = v[e];
        }
      }
#pragma unroll
      for (int e = 0; e < E; ++e) x[e] = pack_one<kBlend, kRead>(x[e], kRead ? o[e] : 0.f, scale, beta, omb);
      if constexpr (kCheck) {
#pragma unroll
        for (int e = 0; e < E; ++e) bad |= not_finite(x[e]);
      }
#pragma unroll
      for (int q = 0; q < E / 4; ++q) {
        f32x4 v = {x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]};
        *reinterpret_cast<f32x4*>(dst + i + 4 * q) = v;
      }
    }
    const int i = head + nvec * E + t;
    if (i < n) {
      const float y = pack_one<kBlend, kRead>(T::widen(src[i]), kRead ? dst[i] : 0.f, scale, beta, omb);
      if constexpr (kCheck) bad |= not_finite(y);
      dst[i] = y;
    }
  }
  if constexpr (kCheck) {
    if (bad) *flag = stamp;
  }
}

// psgd_uvd_check_multi: the predicate of the checked pack on the same tables, and nothing written but the flag.  Every element is
// read once in its own type; the 16-byte body is aligned on the SOURCE (there is no stored side), head and tail are scalar.
template <class T>
__global__ __launch_bounds__(kT) void k_uvd_check(const Seg* __restrict__ segs, const Chunk* __restrict__ chunks, int64_t nchunks, int k,
                                                  float scale, int32_t* __restrict__ flag, int32_t stamp) {
  using raw = typename T::raw;
  constexpr int E = T::E;
  const int t = threadIdx.x;
  bool bad = false;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    if ((uint64_t)ch.seg >= (uint64_t)k) continue;
    const Seg s = segs[ch.seg];
    const int64_t left = s.count - ch.off;
    if (ch.off < 0 || left <= 0) continue;
    const int n = (int)(left < kChunk ? left : kChunk);
    const raw* src = reinterpret_cast<const raw*>(s.ptr) + ch.off;
    const int head = head_of(src, (int)sizeof(raw), n);
    const int nvec = (n - head) / E;
    if (t < head) bad |= not_finite(T::widen(src[t]) * scale);
#pragma unroll 2
    for (int g = t; g < nvec; g += kT) {
      float x[E];
      load_16<T>(src + head + g * E, x);
#pragma unroll
      for (int e = 0; e < E; ++e) bad |= not_finite(x[e] * scale);
    }
    const int i = head + nvec * E + t;
    if (i < n) bad |= not_finite(T::widen(src[i]) * scale);
  }
  if (bad) *flag = stamp;
}

// ------------------------------------------------------------------------------------------------------------- sum of squares
__device__ __forceinline__ double block_sum(double v, double* lds) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[w] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kT / 64; ++k) s += lds[k];
  return s;
}

__global__ __launch_bounds__(kT) void k_uvd_sumsq_partial(const float* __restrict__ x, int64_t N, double* __restrict__ partial) {
  __shared__ double lds[kT / 64];
  const int64_t nvec = N / 4;
  double acc = 0.0;
#pragma unroll 4
  for (int64_t g = (int64_t)blockIdx.x * kT + threadIdx.x; g < nvec; g += (int64_t)gridDim.x * kT) {
    const f32x4_u v = *reinterpret_cast<const f32x4_u*>(x + 4 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc += (double)(v[e] * v[e]);
  }
  if (blockIdx.x == 0) {
    const int64_t i = 4 * nvec + threadIdx.x;
    if (i < N) acc += (double)(x[i] * x[i]);
  }
  const double s = block_sum(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(kT) void k_uvd_sumsq_fold(const double* __restrict__ partial, int n, double* __restrict__ out) {
  __shared__ double lds[kT / 64];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += kT) acc += partial[i];
  const double s = block_sum(acc, lds);
  if (threadIdx.x == 0) out[0] = s;
}

// ------------------------------------------------------------------------------------------------------------ parameter update
// psgd.py:757-762 with the roundings of the torch expressions:  delta = T(fl32(lr_eff * pre_grad));  [delta = T(delta + v)];
// p = T(p - delta).  No contraction: every product, sum and difference is rounded on its own.
// kOpaque (the scalar head and tail of a chunk): the product reaches the narrowing as a rounded fp32 value in a register.  Left to
// itself hipcc selects v_fma_mixlo_f16 lr_eff, g, 0 for the float16 narrow(lr_eff * g) there, and the +0 addend turns a -0 product
// into +0: a parameter -0 then stays -0 where the torch tail gives -0 - (-0) = +0.  (The 16-byte body converts with v_cvt_pk_f16_f32.)
// kWd (decoupled weight decay, psgd_uvd_param_update_multi_wd with wd != 0): after v, delta = T(delta + T(fl32(c * p))) with
// c = fl32(lr_eff * wd).  Its product is opaque where the first one is, for the same reason (the sign of a -0 term); in the 16-byte
// body an asm statement would also keep the loop from being unrolled (checked in the ISA: no v_fma_mix* in any instantiation).
template <class T, bool kPre, bool kVs, bool kWd, bool kOpaque = false>
__device__ __forceinline__ float update_one(float p, float g, float v, float lr_eff, float c) {
  if constexpr (!kPre) {
    return p + v;                                     // p.add_(v) of the finite-difference branch (:723)
  } else {
    float prod = lr_eff * g;
    if constexpr (kOpaque) asm("" : "+v"(prod));
    float delta = T::widen(T::narrow(prod));
    if constexpr (kVs) delta = T::widen(T::narrow(delta + v));
    if constexpr (kWd) {
      float dec = c * p;
      if constexpr (kOpaque) asm("" : "+v"(dec));
      delta = T::widen(T::narrow(delta + T::widen(T::narrow(dec))));
    }
    return p - delta;
  }
}

template <class T, bool kPre, bool kVs, bool kWd = false>
__global__ __launch_bounds__(kT) void k_uvd_param_update(const Seg* __restrict__ psegs, const Seg* __restrict__ vsegs,
                                                         const Chunk* __restrict__ chunks, int64_t nchunks, int k,
                                                         const float* __restrict__ pre_grad, float lr, const double* __restrict__ sumsq,
                                                         float max_norm, float tiny, float wd) {
  using raw = typename T::raw;
  constexpr int E = T::E;
  const int t = threadIdx.x;
  float lr_eff = lr;
  if (kPre && sumsq) {        // psgd.py:753-754, one rounding: lr_eff = fl32(lr * min(max_norm / (sqrt(sumsq) + tiny), 1))
    // the minimum propagates NaN as tf.minimum and torch.clamp do: a NaN norm makes lr_eff, and with it every parameter, NaN
    // (ratio < 1.0 alone is false for a NaN and would take the full unclipped step)
    const double ratio = (double)max_norm / (sqrt(sumsq[0]) + (double)tiny);
    lr_eff = (float)((double)lr * (ratio != ratio ? ratio : (ratio < 1.0 ? ratio : 1.0)));
  }
  const float dc = kWd ? lr_eff * wd : 0.f;      // fl32(lr_eff * wd): one rounding, the same whether lr_eff was clipped or not
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    if ((uint64_t)ch.seg >= (uint64_t)k) continue;
    const Seg s = psegs[ch.seg];
    const int64_t left = s.count - ch.off;
    if (ch.off < 0 || left <= 0) continue;
    const int n = (int)(left < kChunk ? left : kChunk);
    raw* p = reinterpret_cast<raw*>(s.ptr) + ch.off;
    const float* g = kPre ? pre_grad + s.start + ch.off : nullptr;
    const raw* v = kVs ? reinterpret_cast<const raw*>(vsegs[ch.seg].ptr) + ch.off : nullptr;
    const int head = head_of(p, (int)sizeof(raw), n);
    const int nvec = (n - head) / E;
    if (t < head)
      p[t] = T::narrow(update_one<T, kPre, kVs, kWd, true>(T::widen(p[t]), kPre ? g[t] : 0.f, kVs ? T::widen(v[t]) : 0.f, lr_eff, dc));
#pragma unroll 2
    for (int q = t; q < nvec; q += kT) {
      const int i = head + q * E;
      float x[E], gg[E], vv[E];
      load_16<T>(p + i, x);
      if constexpr (kPre) {
#pragma unroll
        for (int b = 0; b < E / 4; ++b) {
          const f32x4_u w = *reinterpret_cast<const f32x4_u*>(g + i + 4 * b);
#pragma unroll
          for (int e = 0; e < 4; ++e) gg[4 * b + e] = w[e];
        }
      }
      if constexpr (kVs) load_any<T>(v + i, vv);
#pragma unroll
      for (int e = 0; e < E; ++e) x[e] = update_one<T, kPre, kVs, kWd>(x[e], kPre ? gg[e] : 0.f, kVs ? vv[e] : 0.f, lr_eff, dc);
      store_16<T>(p + i, x);
    }
    const int i = head + nvec * E + t;
    if (i < n)
      p[i] = T::narrow(update_one<T, kPre, kVs, kWd, true>(T::widen(p[i]), kPre ? g[i] : 0.f, kVs ? T::widen(v[i]) : 0.f, lr_eff, dc));
  }
}

// ------------------------------------------------------------------------------ parameter update, stochastic rounding (bf16)
// psgd_uvd_param_update_multi_sr: the update of k_uvd_param_update formed ONCE in fp32 and narrowed ONCE, stochastically.  With
// w = float(p):  d = fl32(lr_eff * g);  kVs: d = fl32(d + float(v));  kWd: d = fl32(d + fl32(c * w)), c = fl32(lr_eff * wd);
// x = fl32(w - d);  p = narrow_param(x, key, idx)  (bf16_state.h: (bits(x) + u) >> 16, u the top 16 bits of the counter hash of
// (key, idx); NaN -> 0x7FC0).  idx = index0 + the segment's start + the offset inside it: the element's place in the optimizer's
// flat parameter order, so what is stored depends on neither the grid, the chunks nor where a tensor starts.  No contraction.
template <bool kVs, bool kWd>
__device__ __forceinline__ float update_one_sr(float w, float g, float v, float lr_eff, float c) {
  float d = lr_eff * g;
  if constexpr (kVs) d = d + v;
  if constexpr (kWd) {
    const float dec = c * w;
    d = d + dec;
  }
  return w - d;
}

// The launch shape, the chunk loop and the accesses of k_uvd_param_update<BF16, true, ., .>: a scalar head to the 16-byte boundary
// of p, a body of 8 elements (16 bytes of p, two 16-byte reads of g) per lane and access, a scalar tail; one hash per element.
template <bool kVs, bool kWd>
__global__ __launch_bounds__(kT) void k_uvd_param_update_sr(const Seg* __restrict__ psegs, const Seg* __restrict__ vsegs,
                                                            const Chunk* __restrict__ chunks, int64_t nchunks, int k,
                                                            const float* __restrict__ pre_grad, float lr,
                                                            const double* __restrict__ sumsq, float max_norm, float tiny, float wd,
                                                            psgd::bf16s::SrKey key, unsigned long long index0) {
  using T = BF16;
  constexpr int E = 8;
  const int t = threadIdx.x;
  float lr_eff = lr;
  if (sumsq) {                // as k_uvd_param_update: fp64, one rounding, a NaN norm propagates
    const double ratio = (double)max_norm / (sqrt(sumsq[0]) + (double)tiny);
    lr_eff = (float)((double)lr * (ratio != ratio ? ratio : (ratio < 1.0 ? ratio : 1.0)));
  }
  const float dc = kWd ? lr_eff * wd : 0.f;      // c = fl32(lr_eff * wd)
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    if ((uint64_t)ch.seg >= (uint64_t)k) continue;
    const Seg s = psegs[ch.seg];
    const int64_t left = s.count - ch.off;
    if (ch.off < 0 || left <= 0) continue;
    const int n = (int)(left < kChunk ? left : kChunk);
    uint16_t* p = reinterpret_cast<uint16_t*>(s.ptr) + ch.off;
    const float* g = pre_grad + s.start + ch.off;
    const uint16_t* v = kVs ? reinterpret_cast<const uint16_t*>(vsegs[ch.seg].ptr) + ch.off : nullptr;
    const unsigned long long idx0 = index0 + (unsigned long long)(s.start + ch.off);
    const int head = head_of(p, 2, n);
    const int nvec = (n - head) / E;
    if (t < head)
      p[t] = (uint16_t)psgd::bf16s::narrow_param(
          update_one_sr<kVs, kWd>(T::widen(p[t]), g[t], kVs ? T::widen(v[t]) : 0.f, lr_eff, dc), key, idx0 + t);
#pragma unroll 2
    for (int q = t; q < nvec; q += kT) {
      const int i = head + q * E;
      float x[E], gg[E], vv[E];
      load_16<T>(p + i, x);
#pragma unroll
      for (int b = 0; b < E / 4; ++b) {
        const f32x4_u w = *reinterpret_cast<const f32x4_u*>(g + i + 4 * b);
#pragma unroll
        for (int e = 0; e < 4; ++e) gg[4 * b + e] = w[e];
      }
      if constexpr (kVs) load_any<T>(v + i, vv);
      u16x8 y;
#pragma unroll
      for (int e = 0; e < E; ++e)
        y[e] = (uint16_t)psgd::bf16s::narrow_param(update_one_sr<kVs, kWd>(x[e], gg[e], kVs ? vv[e] : 0.f, lr_eff, dc), key,
                                                   idx0 + (unsigned)(i + e));
      *reinterpret_cast<u16x8*>(p + i) = y;
    }
    const int i = head + nvec * E + t;
    if (i < n)
      p[i] = (uint16_t)psgd::bf16s::narrow_param(
          update_one_sr<kVs, kWd>(T::widen(p[i]), g[i], kVs ? T::widen(v[i]) : 0.f, lr_eff, dc), key, idx0 + (unsigned)i);
  }
}

static int grid_for(int64_t nchunks) { return (int)(nchunks < kMaxGrid ? nchunks : kMaxGrid); }
static bool bad_dtype(int dtype) { return dtype < PSGD_DTYPE_F32 || dtype > PSGD_DTYPE_F16; }
static int launched() { return hipGetLastError() == hipSuccess ? PSGD_OK : PSGD_ERR_LAUNCH; }

template <class T, bool kPre, bool kVs, bool kWd, class... A>
static void launch_update_as(int grid, hipStream_t st, A... a) {
  hipLaunchKernelGGL((k_uvd_param_update<T, kPre, kVs, kWd>), dim3(grid), dim3(kT), 0, st, a...);
}

template <class T>
static void launch_update(bool pre, bool vs, int grid, hipStream_t st, const Seg* ps, const Seg* vsg, const Chunk* ch, int64_t nchunks,
                          int k, const float* pre_grad, float lr, const double* sumsq, float max_norm, float tiny, float wd) {
  const bool dec = wd != 0.f;                         // wd == 0 runs the kernels without the decay term: no extra rounding step
  if (!pre)
    launch_update_as<T, false, true, false>(grid, st, ps, vsg, ch, nchunks, k, pre_grad, lr, sumsq, max_norm, tiny, wd);
  else if (vs && dec)
    launch_update_as<T, true, true, true>(grid, st, ps, vsg, ch, nchunks, k, pre_grad, lr, sumsq, max_norm, tiny, wd);
  else if (vs)
    launch_update_as<T, true, true, false>(grid, st, ps, vsg, ch, nchunks, k, pre_grad, lr, sumsq, max_norm, tiny, wd);
  else if (dec)
    launch_update_as<T, true, false, true>(grid, st, ps, vsg, ch, nchunks, k, pre_grad, lr, sumsq, max_norm, tiny, wd);
  else
    launch_update_as<T, true, false, false>(grid, st, ps, vsg, ch, nchunks, k, pre_grad, lr, sumsq, max_norm, tiny, wd);
}

template <class T>
static void launch_pack(int mode, int grid, hipStream_t st, const Seg* sg, const Chunk* ch, int64_t nchunks, int k, float scale,
                        float beta, float omb, float* out, int32_t* flag, int32_t stamp) {
  if (mode == 0)
    hipLaunchKernelGGL((k_uvd_pack<T, false, false>), dim3(grid), dim3(kT), 0, st, sg, ch, nchunks, k, scale, beta, omb, out, flag,
                       stamp);
  else if (mode == 1)
    hipLaunchKernelGGL((k_uvd_pack<T, true, false>), dim3(grid), dim3(kT), 0, st, sg, ch, nchunks, k, scale, beta, omb, out, flag,
                       stamp);
  else if (mode == 2)
    hipLaunchKernelGGL((k_uvd_pack<T, true, true>), dim3(grid), dim3(kT), 0, st, sg, ch, nchunks, k, scale, beta, omb, out, flag,
                       stamp);
  else
    hipLaunchKernelGGL((k_uvd_pack<T, false, false, true>), dim3(grid), dim3(kT), 0, st, sg, ch, nchunks, k, scale, beta, omb, out,
                       flag, stamp);
}

// mode 0: the plain pack; 1: blend with beta == 0 (out is not read); 2: blend; 3: the plain pack with the non-finite check
static int pack_entry(int mode, const void* segs, int k, const void* chunks, int64_t nchunks, int dtype, float scale, float beta,
                      float omb, float* out, void* stream, int32_t* flag = nullptr, int32_t stamp = 0) {
  if (!segs || !chunks || !out || k < 0 || nchunks < 0 || bad_dtype(dtype)) return PSGD_ERR_BAD_ARG;
  if (mode == 3 && (!flag || stamp <= 0)) return PSGD_ERR_BAD_ARG;
  if (nchunks == 0) return PSGD_OK;
  hipStream_t st = (hipStream_t)stream;
  const Seg* sg = (const Seg*)segs;
  const Chunk* ch = (const Chunk*)chunks;
  const int grid = grid_for(nchunks);
  if (dtype == PSGD_DTYPE_F32)
    launch_pack<F32>(mode, grid, st, sg, ch, nchunks, k, scale, beta, omb, out, flag, stamp);
  else if (dtype == PSGD_DTYPE_BF16)
    launch_pack<BF16>(mode, grid, st, sg, ch, nchunks, k, scale, beta, omb, out, flag, stamp);
  else
    launch_pack<F16>(mode, grid, st, sg, ch, nchunks, k, scale, beta, omb, out, flag, stamp);
  return launched();
}

}  // namespace psgdt

using namespace psgdt;

extern "C" {

int psgd_uvd_pack_f32(const void* segs, int k, const void* chunks, int64_t nchunks, int dtype, float scale, float* out,
                      void* stream) {
  return pack_entry(0, segs, k, chunks, nchunks, dtype, scale, 0.f, 1.f, out, stream);
}

int psgd_uvd_pack_blend_f32(const void* segs, int k, const void* chunks, int64_t nchunks, int dtype, float scale, float beta,
                            float omb, float* out, void* stream) {
  return pack_entry(beta == 0.f ? 1 : 2, segs, k, chunks, nchunks, dtype, scale, beta, omb, out, stream);
}

int psgd_uvd_pack_check_f32(const void* segs, int k, const void* chunks, int64_t nchunks, int dtype, float scale, float* out,
                            int32_t* flag, int32_t stamp, void* stream) {
  return pack_entry(3, segs, k, chunks, nchunks, dtype, scale, 0.f, 1.f, out, stream, flag, stamp);
}

int psgd_uvd_check_multi(const void* segs, int k, const void* chunks, int64_t nchunks, int dtype, float scale, int32_t* flag,
                         int32_t stamp, void* stream) {
  if (!segs || !chunks || !flag || stamp <= 0 || k < 0 || nchunks < 0 || bad_dtype(dtype)) return PSGD_ERR_BAD_ARG;
  if (nchunks == 0) return PSGD_OK;
  hipStream_t st = (hipStream_t)stream;
  const Seg* sg = (const Seg*)segs;
  const Chunk* ch = (const Chunk*)chunks;
  const int grid = grid_for(nchunks);
  if (dtype == PSGD_DTYPE_F32)
    hipLaunchKernelGGL(k_uvd_check<F32>, dim3(grid), dim3(kT), 0, st, sg, ch, nchunks, k, scale, flag, stamp);
  else if (dtype == PSGD_DTYPE_BF16)
    hipLaunchKernelGGL(k_uvd_check<BF16>, dim3(grid), dim3(kT), 0, st, sg, ch, nchunks, k, scale, flag, stamp);
  else
    hipLaunchKernelGGL(k_uvd_check<F16>, dim3(grid), dim3(kT), 0, st, sg, ch, nchunks, k, scale, flag, stamp);
  return launched();
}

int psgd_uvd_sumsq_f32(const float* x, int64_t N, double* out, void* ws, int64_t ws_bytes, void* stream) {
  if (!x || !out || !ws || N < 0) return PSGD_ERR_BAD_ARG;
  if (ws_bytes < PSGD_UVD_SUMSQ_WS_BYTES || ((uintptr_t)ws & 7)) return PSGD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t tiles = (N + kChunk - 1) / kChunk;
  const int nb = (int)(tiles < kSumsqBlocks ? tiles : kSumsqBlocks);        // a function of N alone: the partition never changes
  if (nb > 0) hipLaunchKernelGGL(k_uvd_sumsq_partial, dim3(nb), dim3(kT), 0, st, x, N, (double*)ws);
  hipLaunchKernelGGL(k_uvd_sumsq_fold, dim3(1), dim3(kT), 0, st, (const double*)ws, nb, out);
  return launched();
}

int psgd_uvd_param_update_multi_wd(const void* param_segs, const void* vs_segs, int k, const void* chunks, int64_t nchunks, int dtype,
                                   const float* pre_grad, float lr, const double* sumsq, float max_norm, float tiny, float wd,
                                   void* stream) {
  if (!param_segs || !chunks || k < 0 || nchunks < 0 || bad_dtype(dtype)) return PSGD_ERR_BAD_ARG;
  if (!pre_grad && (!vs_segs || sumsq)) return PSGD_ERR_BAD_ARG;            // nothing to do, or a clip norm without a gradient
  if (!pre_grad && wd != 0.f) return PSGD_ERR_BAD_ARG;                      // the perturbation of :723 decays nothing
  if (nchunks == 0) return PSGD_OK;
  hipStream_t st = (hipStream_t)stream;
  const Seg* ps = (const Seg*)param_segs;
  const Seg* vsg = (const Seg*)vs_segs;
  const Chunk* ch = (const Chunk*)chunks;
  const int grid = grid_for(nchunks);
  const bool pre = pre_grad != nullptr, vs = vs_segs != nullptr;
  if (dtype == PSGD_DTYPE_F32)
    launch_update<F32>(pre, vs, grid, st, ps, vsg, ch, nchunks, k, pre_grad, lr, sumsq, max_norm, tiny, wd);
  else if (dtype == PSGD_DTYPE_BF16)
    launch_update<BF16>(pre, vs, grid, st, ps, vsg, ch, nchunks, k, pre_grad, lr, sumsq, max_norm, tiny, wd);
  else
    launch_update<F16>(pre, vs, grid, st, ps, vsg, ch, nchunks, k, pre_grad, lr, sumsq, max_norm, tiny, wd);
  return launched();
}

int psgd_uvd_param_update_multi_sr(const void* param_segs, const void* vs_segs, int k, const void* chunks, int64_t nchunks, int dtype,
                                   const float* pre_grad, float lr, const double* sumsq, float max_norm, float tiny, float wd,
                                   uint64_t seed, int64_t index0, void* stream) {
  if (!param_segs || !chunks || k < 0 || nchunks < 0 || dtype != PSGD_DTYPE_BF16 || index0 < 0) return PSGD_ERR_BAD_ARG;
  if (!pre_grad) return PSGD_ERR_BAD_ARG;                                   // the perturbation of :723 and its undo round to nearest
  if (nchunks == 0) return PSGD_OK;
  hipStream_t st = (hipStream_t)stream;
  const Seg* ps = (const Seg*)param_segs;
  const Seg* vsg = (const Seg*)vs_segs;
  const Chunk* ch = (const Chunk*)chunks;
  const int grid = grid_for(nchunks);
  const psgd::bf16s::SrKey key = psgd::bf16s::make_key(seed, 16u);          // tensor id 16: the parameters (bf16_state.h)
  const unsigned long long i0 = (unsigned long long)index0;
#define PSGD_UVD_UPDATE_SR(VS, WD)                                                                                              \
  hipLaunchKernelGGL((k_uvd_param_update_sr<VS, WD>), dim3(grid), dim3(kT), 0, st, ps, vsg, ch, nchunks, k, pre_grad, lr, sumsq, \
                     max_norm, tiny, wd, key, i0)
  if (wd != 0.f) {                           // (a NaN wd decays too: it propagates)
    if (vsg)
      PSGD_UVD_UPDATE_SR(true, true);
    else
      PSGD_UVD_UPDATE_SR(false, true);
  } else if (vsg)
    PSGD_UVD_UPDATE_SR(true, false);
  else
    PSGD_UVD_UPDATE_SR(false, false);
#undef PSGD_UVD_UPDATE_SR
  return launched();
}

int psgd_uvd_param_update_multi(const void* param_segs, const void* vs_segs, int k, const void* chunks, int64_t nchunks, int dtype,
                                const float* pre_grad, float lr, const double* sumsq, float max_norm, float tiny, void* stream) {
  return psgd_uvd_param_update_multi_wd(param_segs, vs_segs, k, chunks, nchunks, dtype, pre_grad, lr, sumsq, max_norm, tiny, 0.f,
                                        stream);
}

}  // extern "C"
