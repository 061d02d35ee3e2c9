// tail_types.h -- the element types of the step-tail kernels (psgd_uvd_tail.hip, psgd_multi_tail.hip, psgd_param_update.hip): fp32 / bf16 / fp16 as the
// PSGD_DTYPE_* codes of the C ABI name them, their conversions to and from float, and 16-byte vector accesses on them.  The
// conversions are the ones the tests of psgd_uvd_tail.hip pin bit for bit against torch (fp16 subnormals, NaN -> quiet NaN);
// every unit takes them from here so that there is one copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace psgdtt {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));       // 16 bytes from any fp32 element
typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));
typedef uint16_t u16x8_u __attribute__((ext_vector_type(8), aligned(2)));    // 16 bytes from any 16-bit element
typedef uint16_t u16x4_u __attribute__((ext_vector_type(4), aligned(2)));    // 8 bytes from any 16-bit element

// dtype codes of the C ABI
struct F32 {
  using raw = float;
  using vec = f32x4;               // 16 bytes of raw
  static constexpr int E = 4;
  static __device__ __forceinline__ float widen(float x) { return x; }
  static __device__ __forceinline__ float narrow(float x) { return x; }
};
struct BF16 {
  using raw = uint16_t;
  using vec = u16x8;
  static constexpr int E = 8;
  static __device__ __forceinline__ float widen(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }
  static __device__ __forceinline__ uint16_t narrow(float x) {          // round to nearest even, NaN -> quiet NaN
    const uint32_t u = __float_as_uint(x);
    if (x != x) return 0x7FC0;
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
  }
};
struct F16 {
  using raw = uint16_t;
  using vec = u16x8;
  static constexpr int E = 8;
  static __device__ __forceinline__ float widen(uint16_t b) {
    union { uint16_t u; _Float16 h; } c;
    c.u = b;
    return (float)c.h;
  }
  static __device__ __forceinline__ uint16_t narrow(float x) {          // v_cvt_f16_f32: round to nearest even
    union { uint16_t u; _Float16 h; } c;
    c.h = (_Float16)x;
    return c.u;
  }
};

// E consecutive elements of type T from an address aligned to the element only
template <class T>
__device__ __forceinline__ void load_any(const typename T::raw* p, float (&x)[T::E]) {
  if constexpr (T::E == 4) {
    const f32x4_u v = *reinterpret_cast<const f32x4_u*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = v[e];
  } else {
    const u16x8_u v = *reinterpret_cast<const u16x8_u*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = T::widen(v[e]);
  }
}
// ... from / to a 16-byte aligned address
template <class T>
__device__ __forceinline__ void load_16(const typename T::raw* p, float (&x)[T::E]) {
  if constexpr (T::E == 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = v[e];
  } else {
    const u16x8 v = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = T::widen(v[e]);
  }
}
template <class T>
__device__ __forceinline__ void store_16(typename T::raw* p, const float (&x)[T::E]) {
  if constexpr (T::E == 4) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = x[e];
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
    u16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = T::narrow(x[e]);
    *reinterpret_cast<u16x8*>(p) = v;
  }
}

}  // namespace psgdtt
