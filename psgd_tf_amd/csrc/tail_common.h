// tail_common.h -- what the step-tail units (psgd_uvd_tail.hip, psgd_multi_tail.hip, psgd_param_update.hip) share beside the element
// types of tail_types.h: the two device tables and the launch shape, the non-finite predicate, the clip prologue of the parameter
// update, and the pieces of the sums of squares that do not depend on how a sum is partitioned.  One copy of each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "psgd_hip.h"
#include "tail_types.h"

// The roundings of the tail kernels are their contract: no product may be fused into a following sum.  The pragma covers the
// arithmetic of this header; every unit repeats it for its own.
#pragma clang fp contract(off)

namespace psgdtt {

constexpr int kT = 256;                    // threads per workgroup
constexpr int kChunk = PSGD_UVD_TAIL_CHUNK;
constexpr int kMaxGrid = 2048;             // 8 workgroups per CU; the rest is grid-stride

// A SEGMENT is one tensor; a CHUNK is one piece of at most kChunk consecutive elements of one segment.
struct Seg {
  uint64_t ptr;
  int64_t start, count;
};
struct Chunk {
  int64_t seg, off;
};

static int grid_for(int64_t nchunks) { return (int)(nchunks < kMaxGrid ? nchunks : kMaxGrid); }
static int launched() { return hipGetLastError() == hipSuccess ? PSGD_OK : PSGD_ERR_LAUNCH; }
static bool bad_dtype(int dtype) { return dtype < PSGD_DTYPE_F32 || dtype > PSGD_DTYPE_F16; }

// elements of `bytes` bytes in front of the first 16-byte boundary at or after p, at most n
template <int bytes>
__device__ __forceinline__ int head_of(const void* p, int n) {
  const int h = (int)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / bytes;
  return h < n ? h : n;
}

// The non-finite predicate of the guarded step, on a value as it is written: exponent all ones (+-Inf, NaN).
__device__ __forceinline__ bool not_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u; }

// psgd.py:753-754 in fp64 with one rounding: lr_eff = fl32(lr * min(max_norm / (sqrt(sumsq) + tiny), 1)); no norm, no clip.  The
// minimum propagates NaN as tf.minimum and torch.clamp do: a NaN norm makes lr_eff, and with it every parameter, NaN (ratio < 1.0
// alone is false for a NaN and would take the full unclipped step).
__device__ __forceinline__ float clipped_lr(float lr, const double* sumsq, float max_norm, float tiny) {
  if (!sumsq) return lr;
  const double ratio = (double)max_norm / (sqrt(sumsq[0]) + (double)tiny);
  return (float)((double)lr * (ratio != ratio ? ratio : (ratio < 1.0 ? ratio : 1.0)));
}

// ------------------------------------------------------------------------------------------------------------- sum of squares
// lanes -> waves -> workgroup in a fixed order
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

// acc + the squares of lane t's elements of one piece of a list of fp32 tensors, each product rounded to fp32: a scalar head to the
// 16-byte boundary, groups of four at head + 4 (t + 256 j), a scalar tail
__device__ __forceinline__ double sumsq_piece_f32(double acc, const float* x, int n, int t) {
  const int head = head_of<4>(x, n);
  const int nvec = (n - head) / 4;
  if (t < head) acc += (double)(x[t] * x[t]);
#pragma unroll 2
  for (int g = t; g < nvec; g += kT) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + head + 4 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc += (double)(v[e] * v[e]);
  }
  const int i = head + nvec * 4 + t;
  if (i < n) acc += (double)(x[i] * x[i]);
  return acc;
}

// the partials of the workgroups in index order -> one double (static: each unit that launches it has its own)
static __global__ __launch_bounds__(kT) void k_sumsq_fold(const double* __restrict__ partial, int n, double* __restrict__ out) {
  __shared__ double lds[kT / 64];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += kT) acc += partial[i];
  const double s = block_sum(acc, lds);
  if (threadIdx.x == 0) out[0] = s;
}

}  // namespace psgdtt
