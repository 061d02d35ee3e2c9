// psgd_uvd_tail.hip -- the tail of UVd.step (psgd.py:729-730, :747, :753) on gfx950, whatever the number of parameter tensors; the
// parameter update itself (:757-762) is psgd_param_update.hip.
//
//   psgd_uvd_pack_f32            k tensors of one dtype (fp32 / bf16 / fp16) -> one flat fp32 vector, times a scale      (:729-736, :747)
//   psgd_uvd_pack_blend_f32      the same pack blended into the flat vector: out <- fl32(fl32(beta out) + fl32(omb x))  (momentum of class UVd)
//   psgd_uvd_pack_check_f32      the plain pack, and a stamp stored to a flag word when a written value is not finite     (guarded step)
//   psgd_uvd_check_multi         the same predicate on the same tables; writes the flag alone (the gradients before a blend)
//   psgd_uvd_sumsq_f32           sum x^2 of a flat fp32 vector -> one device double (the clip norm's square)              (:753)
//
// The work of pack is described by two device tables (tail_common.h).  A SEGMENT is one tensor: {pointer, start offset in the flat
// vector, element count}.  A CHUNK is one piece of at most kChunk consecutive elements of one segment: {segment index, offset inside
// it}; the host builds the chunk table once from the sizes, every flat element belongs to exactly one chunk, and a workgroup takes
// whole chunks (grid-stride): nothing searches.  One launch serves any k.
//
// HBM-bound streaming: inside a chunk the stored side (the flat vector) is brought to a 16-byte boundary by a scalar head, the body
// moves 16 bytes of the narrowest type per lane and access (4 fp32 or 8 half-precision elements), a scalar tail finishes.  The
// source is read through vector types whose declared alignment is the element's, so tensors that start at any element (offset
// views, odd sizes in front of them) still take wide loads.
//
// The sum of squares rounds each product to fp32 (as the torch expression it replaces does), accumulates in fp64 per lane, folds
// lanes -> waves -> workgroup in a fixed order into one fp64 partial per workgroup, and a second one-workgroup launch folds the
// partials in index order: no floating-point atomics, the same bits on every call.
//
// No entry point allocates or synchronises; argument checks return before any HIP call.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "psgd_hip.h"
#include "tail_common.h"

// The roundings of this file are its contract (bit-equal to the torch expressions it replaces): no product may be fused into a
// following sum.  hipcc contracts by default, and the header's __fmul_rn / __fadd_rn are compiled under that default: plain
// operators under this pragma are what stays unfused (checked in the ISA: no v_fma / v_fmac / v_pk_fma on fp32).
#pragma clang fp contract(off)

namespace psgdt {

// the tables, the launch shape, F32 / BF16 / F16 (the dtype codes of the C ABI) with their 16-byte accesses: tail_common.h
using namespace psgdtt;

constexpr int kSumsqBlocks = 1024;         // partials of the sum of squares: PSGD_UVD_SUMSQ_WS_BYTES / 8
static_assert(kSumsqBlocks * 8 == PSGD_UVD_SUMSQ_WS_BYTES, "workspace constant of the header");

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
    const int head = head_of<4>(dst, n);
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
    const int head = head_of<(int)sizeof(raw)>(src, n);
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
  hipLaunchKernelGGL(k_sumsq_fold, dim3(1), dim3(kT), 0, st, (const double*)ws, nb, out);
  return launched();
}

}  // extern "C"
