// bf16_state.h -- what the kernel families of a bf16-STORED preconditioner state share (psgd_uvd_bf16.hip, psgd_splu_bf16.hip):
// the widening and the one narrowing of an element (round to nearest even or stochastic, a counter hash keyed by seed,
// tensor id and flat element index), the rounding-stream keys, the exact three-piece bf16 split of an fp32 value, and the
// tile copies of an [N, r] row-major bf16 matrix with 16-byte loads and stores whatever the rank.
// Tensor ids of the rounding streams: 0, 1, 2 = U, V, d of UVd; 8, 9, 10, 11 = L12, l3, U12, u3 of the sparse-LU state;
// 16 = the bf16 PARAMETERS of class UVd / class Kron (param_rounding="stochastic": narrow_param below, the step-tail kernels);
// 17 = the PROBE VECTORS of class Kron(preconditioner_fit="whitening"): not a rounding stream but the standard normal draws of
// psgd_multi_randn_f32 (psgd_multi_tail.hip), keyed the same way -- key64(seed, 17) and the element's flat index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "psgd_hip.h"

namespace psgd {
namespace bf16s {

typedef unsigned short u16;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kT = 256;            // threads per block (4 waves)
struct Geo {
  int r, rp, S, RI, IT, TR;   // rank, LDS row stride, active loader threads, rows per loader pass, passes, rows per tile
};

inline Geo make_geo(int r) {
  Geo g;
  g.r = r;
  g.rp = r | 1;
  int m = kT / r;
  if (m > 32) m = 32;
  g.S = r * m;
  g.RI = 8 * m;
  g.IT = kT / g.RI;
  g.TR = g.IT * g.RI;
  return g;
}

struct SrKey { unsigned a, b; };

__host__ __device__ inline uint64_t mix64(uint64_t z) {   // the splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// key of one tensor's rounding stream: the seed is hashed BEFORE the tensor id enters and the sum is hashed again, so no
// arithmetic relation between seeds (seed + c, seed ^ c, ...) maps one tensor's stream onto another's
inline uint64_t key64(uint64_t seed, unsigned tensor) {
  return mix64(mix64(seed + 0x9E3779B97F4A7C15ull) ^ (0xD1B54A32D192ED03ull * (uint64_t)(tensor + 1)));
}

inline SrKey make_key(uint64_t seed, unsigned tensor) {
  const uint64_t z = key64(seed, tensor);
  return SrKey{(unsigned)z, (unsigned)(z >> 32)};
}

__device__ __forceinline__ float widen(unsigned bits16) { return __uint_as_float(bits16 << 16); }

// fp32 -> bf16 code.  mode 0: round to nearest even; mode 1: stochastic, (bits + u) >> 16, u a hash of (key, idx).
// NaN and Inf are stored as they are (a NaN keeps a mantissa bit).
__device__ __forceinline__ unsigned narrow(float x, int mode, SrKey key, unsigned long long idx) {
  const unsigned b = __float_as_uint(x);
  if ((b & 0x7f800000u) == 0x7f800000u) return (b >> 16) | ((b & 0xffffu) ? 0x40u : 0u);
  unsigned add;
  if (mode == 0) {
    add = 0x7fffu + ((b >> 16) & 1u);
  } else {
    unsigned z = (unsigned)idx * 0x9E3779B1u + key.a + (unsigned)(idx >> 32) * 0x85EBCA77u;
    z ^= z >> 16; z *= 0x7feb352du;
    z ^= key.b;
    z ^= z >> 15; z *= 0x846ca68bu;
    z ^= z >> 16;
    add = z >> 16;
  }
  return (b + add) >> 16;
}

// fp32 -> bf16 code of a PARAMETER written by the stochastic step-tail kernels (tensor id 16): the mode-1 narrowing above on the
// element's index in the optimizer's flat parameter order, except that a NaN becomes the quiet NaN 0x7FC0 (what
// psgdtt::BF16::narrow and torch store).  +-Inf stays +-Inf.  A value that is exactly a bf16 code is never changed (its low 16 bits
// are 0 and the addend is below 2^16).  A finite x beyond the largest finite bf16 value (low 16 bits f of 0x7F7Fffff's neighbourhood)
// carries into +-Inf with probability f / 2^16: that IS the stochastic outcome -- the two neighbours of such an x are the largest
// finite bf16 value and Inf -- and round to nearest does the same from the midpoint on.
__device__ __forceinline__ unsigned narrow_param(float x, SrKey key, unsigned long long idx) {
  if (x != x) return 0x7FC0u;
  return narrow(x, 1, key, idx);
}

// x = h + m + l, each an exact bf16 value kept as fp32
// (a NaN becomes the canonical quiet NaN first: its top 16 bits alone must still be a NaN in the MFMA operand)
__device__ __forceinline__ void split3(float x, float& h, float& m, float& l) {
  if (x != x) x = __uint_as_float(0x7fc00000u);
  h = __uint_as_float(__float_as_uint(x) & 0xffff0000u);
  const float r1 = x - h;
  m = __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
  l = r1 - m;
}

// per-thread loader state: LDS offset of each of the 8 slots of this thread's chunk (row offset * rp + column)
struct Slots { int off[8]; };

__device__ __forceinline__ Slots make_slots(const Geo& g) {
  Slots s;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int e = 8 * (int)threadIdx.x + j;
    const int row = e / g.r;
    s.off[j] = row * g.rp + (e - row * g.r);
  }
  return s;
}

// global bf16 span -> LDS fp32 tile (times scale).  rows = valid rows of the tile.
__device__ __forceinline__ void load_tile(const u16* __restrict__ M, float* L, const Geo& g, const Slots& s, long row0,
                                          int rows, float scale) {
  if ((int)threadIdx.x >= g.S) return;
  const int telems = rows * g.r;
  const u16* base = M + row0 * g.r;
  for (int it = 0; it < g.IT; ++it) {
    const int e0 = 8 * ((int)threadIdx.x + it * g.S);
    if (e0 >= telems) break;
    u32x4 raw;
    if (e0 + 8 <= telems) {
      raw = *reinterpret_cast<const u32x4*>(base + e0);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned lo = (e0 + 2 * q < telems) ? base[e0 + 2 * q] : 0u;
        const unsigned hi = (e0 + 2 * q + 1 < telems) ? base[e0 + 2 * q + 1] : 0u;
        raw[q] = lo | (hi << 16);
      }
    }
    float* Lb = L + it * g.RI * g.rp;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned bits = (j & 1) ? (raw[j >> 1] & 0xffff0000u) : (raw[j >> 1] << 16);
      Lb[s.off[j]] = __uint_as_float(bits) * scale;
    }
  }
}

// LDS tile (fp32 values that are exact bf16) -> global bf16 span
__device__ __forceinline__ void store_tile(u16* __restrict__ M, const float* L, const Geo& g, const Slots& s, long row0,
                                           int rows) {
  if ((int)threadIdx.x >= g.S) return;
  const int telems = rows * g.r;
  u16* base = M + row0 * g.r;
  for (int it = 0; it < g.IT; ++it) {
    const int e0 = 8 * ((int)threadIdx.x + it * g.S);
    if (e0 >= telems) break;
    const float* Lb = L + it * g.RI * g.rp;
    unsigned c[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = __float_as_uint(Lb[s.off[j]]) >> 16;
    if (e0 + 8 <= telems) {
      u32x4 raw;
#pragma unroll
      for (int q = 0; q < 4; ++q) raw[q] = c[2 * q] | (c[2 * q + 1] << 16);
      *reinterpret_cast<u32x4*>(base + e0) = raw;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (e0 + j < telems) base[e0 + j] = (u16)c[j];
    }
  }
}

// dynamic LDS above the default limit: the attribute is set ONCE per kernel and device, to what the kernel needs at the
// largest rank (no runtime call on later launches, none inside a stream capture after the first call)
template <auto Kernel>
int set_lds(size_t max_bytes) {
  static std::atomic<uint64_t> done{0};
  if (max_bytes <= 48 * 1024) return PSGD_OK;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return PSGD_ERR_LAUNCH;
  const uint64_t bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return PSGD_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_bytes) !=
      hipSuccess)
    return PSGD_ERR_LAUNCH;
  done.fetch_or(bit, std::memory_order_release);
  return PSGD_OK;
}

}  // namespace bf16s
}  // namespace psgd
