// psgd_param_update.hip -- the parameter update of a step, p <- p - delta(g, v, p) for every element of every parameter tensor
// (psgd.py:757-762; the perturbation p <- p + v of :723 when there is no gradient), on gfx950: ONE kernel template behind
//
//   psgd_uvd_param_update_multi[_wd]   the gradient is the flat fp32 vector of class UVd; parameters and vs fp32 / bf16 / fp16
//   psgd_uvd_param_update_multi_sr     ... bf16 parameters, the update formed once in fp32 and narrowed once, stochastically
//   psgd_multi_param_update[_wd]_f32   the gradients are a list of fp32 tensors (class Kron); parameters and vs fp32
//   psgd_multi_param_update_t          ... parameters and vs fp32 / bf16 / fp16
//   psgd_multi_param_update_mixed      ... every gradient tensor fp32 or bf16 (the layers on the bf16-operand Kron kernels)
//   psgd_multi_param_update_sr         the list forms with bf16 parameters and stochastic rounding
//   psgd_multi_param_update_mixed_sr
//
// The tables are those of tail_common.h: a segment table per operand, one chunk table for all, a workgroup takes whole chunks
// (grid-stride).  A chunk never runs past the shortest of its segments (parameters, the gradient list, vs), whatever the tables say.
// HBM-bound streaming: inside a chunk p is brought to a 16-byte boundary by a scalar head, the body moves 16 bytes of p per lane and
// access (4 fp32 or 8 half-precision elements), a scalar tail finishes; g and v go through vector types whose declared alignment is
// the element's, so tensors that start at any element still take wide loads.
//
// No entry point allocates or synchronises; argument checks return before any HIP call.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "psgd_hip.h"
#include "tail_common.h"
#include "bf16_state.h"

// The roundings of this file are its contract (bit-equal to the torch expressions it replaces): no product may be fused into a
// following sum.  hipcc contracts by default, and the header's __fmul_rn / __fadd_rn are compiled under that default: plain
// operators under this pragma are what stays unfused (checked in the ISA: no v_fma / v_fmac / v_pk_fma on fp32, no v_fma_mix*).
#pragma clang fp contract(off)

namespace psgdu {

using namespace psgdtt;
using psgd::bf16s::SrKey;

// ------------------------------------------------------------------------------------------------------------ gradient sources
// bind(): the gradient of one chunk of parameter segment ps; shrinks `left` to what the source holds; false: the chunk moves
// nothing.  at(i) is element i as a float, load(i, gg) E consecutive ones from an address aligned to the element only.
struct GradF32 {
  const float* g = nullptr;
  static constexpr bool kOpaqueBody = false;
  __device__ __forceinline__ float at(int i) const { return g[i]; }
  template <int E>
  __device__ __forceinline__ void load(int i, float (&gg)[E]) const {
#pragma unroll
    for (int b = 0; b < E / 4; ++b) {
      const f32x4_u w = *reinterpret_cast<const f32x4_u*>(g + i + 4 * b);
#pragma unroll
      for (int e = 0; e < 4; ++e) gg[4 * b + e] = w[e];
    }
  }
};
// the flat fp32 vector of class UVd, indexed by the parameter segment's `start`
struct GradFlat : GradF32 {
  __device__ __forceinline__ bool bind(const float* flat, const Seg*, const Chunk ch, const Seg ps, int64_t&) {
    g = flat + ps.start + ch.off;
    return true;
  }
};
// a list of fp32 tensors
struct GradList : GradF32 {
  __device__ __forceinline__ bool bind(const float*, const Seg* gsegs, const Chunk ch, const Seg, int64_t& left) {
    const Seg gs = gsegs[ch.seg];
    const int64_t l = gs.count - ch.off;
    left = l < left ? l : left;
    g = reinterpret_cast<const float*>(gs.ptr) + ch.off;
    return true;
  }
};
// a MIXED list: every segment is fp32 or bf16, and its `start` field holds its PSGD_DTYPE_* code.  A segment with any other code
// moves nothing: the tables live on the device and the host cannot judge them.
struct GradMixed {
  const void* g = nullptr;
  bool bf = false;
  static constexpr bool kOpaqueBody = true;
  __device__ __forceinline__ bool bind(const float*, const Seg* gsegs, const Chunk ch, const Seg, int64_t& left) {
    const Seg gs = gsegs[ch.seg];
    if (gs.start != PSGD_DTYPE_F32 && gs.start != PSGD_DTYPE_BF16) return false;
    bf = gs.start == PSGD_DTYPE_BF16;
    const int64_t l = gs.count - ch.off;
    left = l < left ? l : left;
    g = reinterpret_cast<const char*>(gs.ptr) + ch.off * (bf ? 2 : 4);
    return true;
  }
  __device__ __forceinline__ float at(int i) const {
    return bf ? BF16::widen(reinterpret_cast<const uint16_t*>(g)[i]) : reinterpret_cast<const float*>(g)[i];
  }
  template <int E>
  __device__ __forceinline__ void load(int i, float (&gg)[E]) const {
    if (!bf) {
      GradF32{reinterpret_cast<const float*>(g)}.load(i, gg);
    } else if constexpr (E == 8) {
      load_any<BF16>(reinterpret_cast<const uint16_t*>(g) + i, gg);
    } else {
      const u16x4_u w = *reinterpret_cast<const u16x4_u*>(reinterpret_cast<const uint16_t*>(g) + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) gg[e] = BF16::widen(w[e]);
    }
  }
};

// -------------------------------------------------------------------------------------------------------------------- rounding
// one(): the stored element from w = float(p), float(g), float(v), lr_eff and c = fl32(lr_eff * wd).  No contraction: every
// product, sum and difference is rounded on its own.
//
// Nearest<T>: psgd.py:757-762 with the roundings of the torch expressions on tensors of type T:  delta = T(fl32(lr_eff * g));
// kVs: delta = T(delta + v);  kWd (decoupled weight decay, wd != 0): delta = T(delta + T(fl32(c * p)));  p = T(p - delta).  For
// T = F32 every T(.) is the identity.  !kPre: p = T(p + v), p.add_(v) of the finite-difference branch (:723).
// kOpaque: the products reach their narrowing as rounded fp32 values in a register.  Left to itself hipcc selects
// v_fma_mixlo_f16 lr_eff, g, 0 for the float16 narrow(lr_eff * g) of a scalar access, and the +0 addend turns a -0 product into +0:
// a parameter -0 then stays -0 where the torch tail gives -0 - (-0) = +0.  The decay product is opaque where the first one is, for
// the same reason (the sign of a -0 term).  Set on the scalar head and tail of a chunk; the 16-byte body converts with
// v_cvt_pk_f16_f32 and an asm statement there would also keep the loop from being unrolled, so the body is opaque only for the
// mixed lists (GradMixed::kOpaqueBody), whose body would take v_fma_mix* too.  Checked in the ISA: no v_fma_mix* in any instantiation.
template <class T>
struct Nearest {
  template <bool kPre, bool kVs, bool kWd, bool kOpaque>
  static __device__ __forceinline__ typename T::raw one(float p, float g, float v, float lr_eff, float c, SrKey, unsigned long long) {
    if constexpr (!kPre) {
      return T::narrow(p + v);
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
      return T::narrow(p - delta);
    }
  }
};

// Stochastic (bf16 parameters): the update formed ONCE in fp32 and narrowed ONCE.  d = fl32(lr_eff * g);  kVs: d = fl32(d + v);
// kWd: d = fl32(d + fl32(c * w));  x = fl32(w - d);  p = narrow_param(x, key, idx)  (bf16_state.h: (bits(x) + u) >> 16, u the top
// 16 bits of the counter hash of (key, idx); NaN -> 0x7FC0).  idx = index0 + the PARAMETER segment's start + the offset inside it:
// the element's place in the optimizer's flat parameter order, so what is stored depends on neither the grid, the chunks nor where
// a tensor starts.  One hash per element.
struct Stochastic {
  template <bool kPre, bool kVs, bool kWd, bool kOpaque>
  static __device__ __forceinline__ uint16_t one(float w, float g, float v, float lr_eff, float c, SrKey key, unsigned long long idx) {
    static_assert(kPre, "the perturbation p + v and its undo round to nearest");
    float d = lr_eff * g;
    if constexpr (kVs) d = d + v;
    if constexpr (kWd) {
      const float dec = c * w;
      d = d + dec;
    }
    return (uint16_t)psgd::bf16s::narrow_param(w - d, key, idx);
  }
};

// ------------------------------------------------------------------------------------------------------------------ the kernel
// T: the type of p and v (tail_types.h);  G: where the gradient comes from (`flat` or `gsegs`, the other is not read);  R: the
// rounding (key and index0 are read by Stochastic alone);  kPre / kVs / kWd: which terms there are -- wd == 0 runs without the
// decay term and takes no extra rounding step.
template <class T, class G, class R, bool kPre, bool kVs, bool kWd>
__global__ __launch_bounds__(kT) void k_param_update(const Seg* __restrict__ psegs, const float* __restrict__ flat,
                                                     const Seg* __restrict__ gsegs, const Seg* __restrict__ vsegs,
                                                     const Chunk* __restrict__ chunks, int64_t nchunks, int k, float lr,
                                                     const double* __restrict__ sumsq, float max_norm, float tiny, float wd, SrKey key,
                                                     unsigned long long index0) {
  using raw = typename T::raw;
  constexpr int E = T::E;
  const int t = threadIdx.x;
  const float lr_eff = kPre ? clipped_lr(lr, sumsq, max_norm, tiny) : lr;
  const float dc = kWd ? lr_eff * wd : 0.f;      // c = fl32(lr_eff * wd): one rounding, the same whether lr_eff was clipped or not
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    if ((uint64_t)ch.seg >= (uint64_t)k || ch.off < 0) continue;     // a table that does not belong to these segments moves nothing
    const Seg ps = psegs[ch.seg];
    int64_t left = ps.count - ch.off;
    left = left < kChunk ? left : kChunk;
    raw* p = reinterpret_cast<raw*>(ps.ptr) + ch.off;
    G g;
    if constexpr (kPre) {
      if (!g.bind(flat, gsegs, ch, ps, left)) continue;
    }
    const raw* v = nullptr;
    if constexpr (kVs) {
      const Seg vsg = vsegs[ch.seg];
      const int64_t l = vsg.count - ch.off;
      left = l < left ? l : left;
      v = reinterpret_cast<const raw*>(vsg.ptr) + ch.off;
    }
    if (left <= 0) continue;
    const int n = (int)left;
    const unsigned long long idx0 = index0 + (unsigned long long)(ps.start + ch.off);
    const int head = head_of<(int)sizeof(raw)>(p, n);
    const int nvec = (n - head) / E;
    if (t < head)
      p[t] = R::template one<kPre, kVs, kWd, true>(T::widen(p[t]), kPre ? g.at(t) : 0.f, kVs ? T::widen(v[t]) : 0.f, lr_eff, dc, key,
                                                   idx0 + (unsigned)t);
#pragma unroll 2
    for (int q = t; q < nvec; q += kT) {
      const int i = head + q * E;
      float x[E], gg[E], vv[E];
      load_16<T>(p + i, x);
      if constexpr (kPre) g.load(i, gg);
      if constexpr (kVs) load_any<T>(v + i, vv);
      typename T::vec y;
#pragma unroll
      for (int e = 0; e < E; ++e)
        y[e] = R::template one<kPre, kVs, kWd, G::kOpaqueBody>(x[e], kPre ? gg[e] : 0.f, kVs ? vv[e] : 0.f, lr_eff, dc, key,
                                                               idx0 + (unsigned)(i + e));
      *reinterpret_cast<typename T::vec*>(p + i) = y;
    }
    const int i = head + nvec * E + t;
    if (i < n)
      p[i] = R::template one<kPre, kVs, kWd, true>(T::widen(p[i]), kPre ? g.at(i) : 0.f, kVs ? T::widen(v[i]) : 0.f, lr_eff, dc, key,
                                                   idx0 + (unsigned)i);
  }
}

// ---------------------------------------------------------------------------------------------------------------- the launcher
struct Args {
  const void *psegs, *flat, *gsegs, *vsegs, *chunks;
  int64_t nchunks;
  int k;
  float lr;
  const double* sumsq;
  float max_norm, tiny, wd;
  void* stream;
  uint64_t seed = 0;
  int64_t index0 = 0;
};

template <class T, class G, class R, bool kPre, bool kVs, bool kWd>
static void launch_as(const Args& a) {
  const SrKey key = psgd::bf16s::make_key(a.seed, 16u);                       // tensor id 16: the parameters (bf16_state.h)
  hipLaunchKernelGGL((k_param_update<T, G, R, kPre, kVs, kWd>), dim3(grid_for(a.nchunks)), dim3(kT), 0, (hipStream_t)a.stream,
                     (const Seg*)a.psegs, (const float*)a.flat, (const Seg*)a.gsegs, (const Seg*)a.vsegs, (const Chunk*)a.chunks,
                     a.nchunks, a.k, a.lr, a.sumsq, a.max_norm, a.tiny, a.wd, key, (unsigned long long)a.index0);
}

// (gradient?, vs?, wd != 0) -> the form.  kPerturb: whether this family has the form without a gradient, p + v.
template <class T, class G, class R, bool kPerturb>
static int launch_update(const Args& a) {
  const bool pre = a.flat || a.gsegs, vs = a.vsegs != nullptr;
  const bool dec = a.wd != 0.f;              // wd == 0 runs without the decay term; a NaN wd decays too: it propagates
  if (!pre) {
    if constexpr (kPerturb) launch_as<T, G, R, false, true, false>(a);
  } else if (vs && dec)
    launch_as<T, G, R, true, true, true>(a);
  else if (vs)
    launch_as<T, G, R, true, true, false>(a);
  else if (dec)
    launch_as<T, G, R, true, false, true>(a);
  else
    launch_as<T, G, R, true, false, false>(a);
  return launched();
}

template <class G, bool kPerturb>
static int launch_nearest(int dtype, const Args& a) {
  if (dtype == PSGD_DTYPE_F32) return launch_update<F32, G, Nearest<F32>, kPerturb>(a);
  if (dtype == PSGD_DTYPE_BF16) return launch_update<BF16, G, Nearest<BF16>, kPerturb>(a);
  return launch_update<F16, G, Nearest<F16>, kPerturb>(a);
}

// the two stochastic list entry points: a gradient list is required, bf16 parameters only, index0 >= 0
template <class G>
static int update_sr_entry(const void* param_segs, const void* grad_segs, const void* vs_segs, int k, const void* chunks,
                           int64_t nchunks, int dtype, float lr, const double* sumsq, float max_norm, float tiny, float wd,
                           uint64_t seed, int64_t index0, void* stream) {
  if (dtype != PSGD_DTYPE_BF16 || index0 < 0) return PSGD_ERR_BAD_ARG;
  if (!param_segs || !grad_segs || !chunks || k < 0 || nchunks < 0) return PSGD_ERR_BAD_ARG;
  if (nchunks == 0) return PSGD_OK;
  return launch_update<BF16, G, Stochastic, false>(
      {param_segs, nullptr, grad_segs, vs_segs, chunks, nchunks, k, lr, sumsq, max_norm, tiny, wd, stream, seed, index0});
}

}  // namespace psgdu

using namespace psgdu;

extern "C" {

// The flat entry points bound a chunk by the parameter segment AND the vs segment (the rule of every list kernel): with a vs table
// whose counts are shorter than the parameters' they stop at the shorter count, where they used to trust the vs table.
int psgd_uvd_param_update_multi_wd(const void* param_segs, const void* vs_segs, int k, const void* chunks, int64_t nchunks, int dtype,
                                   const float* pre_grad, float lr, const double* sumsq, float max_norm, float tiny, float wd,
                                   void* stream) {
  if (!param_segs || !chunks || k < 0 || nchunks < 0 || bad_dtype(dtype)) return PSGD_ERR_BAD_ARG;
  if (!pre_grad && (!vs_segs || sumsq)) return PSGD_ERR_BAD_ARG;            // nothing to do, or a clip norm without a gradient
  if (!pre_grad && wd != 0.f) return PSGD_ERR_BAD_ARG;                      // the perturbation of :723 decays nothing
  if (nchunks == 0) return PSGD_OK;
  return launch_nearest<GradFlat, true>(
      dtype, {param_segs, pre_grad, nullptr, vs_segs, chunks, nchunks, k, lr, sumsq, max_norm, tiny, wd, stream});
}

int psgd_uvd_param_update_multi(const void* param_segs, const void* vs_segs, int k, const void* chunks, int64_t nchunks, int dtype,
                                const float* pre_grad, float lr, const double* sumsq, float max_norm, float tiny, void* stream) {
  return psgd_uvd_param_update_multi_wd(param_segs, vs_segs, k, chunks, nchunks, dtype, pre_grad, lr, sumsq, max_norm, tiny, 0.f,
                                        stream);
}

int psgd_uvd_param_update_multi_sr(const void* param_segs, const void* vs_segs, int k, const void* chunks, int64_t nchunks, int dtype,
                                   const float* pre_grad, float lr, const double* sumsq, float max_norm, float tiny, float wd,
                                   uint64_t seed, int64_t index0, void* stream) {
  if (!param_segs || !chunks || k < 0 || nchunks < 0 || dtype != PSGD_DTYPE_BF16 || index0 < 0) return PSGD_ERR_BAD_ARG;
  if (!pre_grad) return PSGD_ERR_BAD_ARG;                                   // the perturbation of :723 and its undo round to nearest
  if (nchunks == 0) return PSGD_OK;
  return launch_update<BF16, GradFlat, Stochastic, false>(
      {param_segs, pre_grad, nullptr, vs_segs, chunks, nchunks, k, lr, sumsq, max_norm, tiny, wd, stream, seed, index0});
}

int psgd_multi_param_update_wd_f32(const void* param_segs, const void* grad_segs, const void* vs_segs, int k, const void* chunks,
                                   int64_t nchunks, float lr, const double* sumsq, float max_norm, float tiny, float wd,
                                   void* stream) {
  if (!param_segs || !chunks || k < 0 || nchunks < 0) return PSGD_ERR_BAD_ARG;
  if (!grad_segs && (!vs_segs || sumsq)) return PSGD_ERR_BAD_ARG;            // nothing to do, or a clip norm without a gradient
  if (!grad_segs && wd != 0.f) return PSGD_ERR_BAD_ARG;                      // the perturbation p + v takes no decay
  if (nchunks == 0) return PSGD_OK;
  return launch_update<F32, GradList, Nearest<F32>, true>(
      {param_segs, nullptr, grad_segs, vs_segs, chunks, nchunks, k, lr, sumsq, max_norm, tiny, wd, stream});
}

int psgd_multi_param_update_f32(const void* param_segs, const void* grad_segs, const void* vs_segs, int k, const void* chunks,
                                int64_t nchunks, float lr, const double* sumsq, float max_norm, float tiny, void* stream) {
  return psgd_multi_param_update_wd_f32(param_segs, grad_segs, vs_segs, k, chunks, nchunks, lr, sumsq, max_norm, tiny, 0.f, stream);
}

int psgd_multi_param_update_t(const void* param_segs, const void* grad_segs, const void* vs_segs, int k, const void* chunks,
                              int64_t nchunks, int dtype, float lr, const double* sumsq, float max_norm, float tiny, float wd,
                              void* stream) {
  if (bad_dtype(dtype)) return PSGD_ERR_BAD_ARG;
  if (dtype == PSGD_DTYPE_F32)                // every operand fp32: the same kernels, the same bits
    return psgd_multi_param_update_wd_f32(param_segs, grad_segs, vs_segs, k, chunks, nchunks, lr, sumsq, max_norm, tiny, wd, stream);
  if (!param_segs || !chunks || k < 0 || nchunks < 0) return PSGD_ERR_BAD_ARG;
  if (!grad_segs && (!vs_segs || sumsq)) return PSGD_ERR_BAD_ARG;            // nothing to do, or a clip norm without a gradient
  if (!grad_segs && wd != 0.f) return PSGD_ERR_BAD_ARG;                      // the perturbation p + v takes no decay
  if (nchunks == 0) return PSGD_OK;
  return launch_nearest<GradList, true>(
      dtype, {param_segs, nullptr, grad_segs, vs_segs, chunks, nchunks, k, lr, sumsq, max_norm, tiny, wd, stream});
}

int psgd_multi_param_update_mixed(const void* param_segs, const void* grad_segs, const void* vs_segs, int k, const void* chunks,
                                  int64_t nchunks, int dtype, float lr, const double* sumsq, float max_norm, float tiny, float wd,
                                  void* stream) {
  if (bad_dtype(dtype)) return PSGD_ERR_BAD_ARG;
  if (!param_segs || !grad_segs || !chunks || k < 0 || nchunks < 0) return PSGD_ERR_BAD_ARG;   // (p + v keeps its entry points)
  if (nchunks == 0) return PSGD_OK;
  return launch_nearest<GradMixed, false>(
      dtype, {param_segs, nullptr, grad_segs, vs_segs, chunks, nchunks, k, lr, sumsq, max_norm, tiny, wd, stream});
}

int psgd_multi_param_update_sr(const void* param_segs, const void* grad_segs, const void* vs_segs, int k, const void* chunks,
                               int64_t nchunks, int dtype, float lr, const double* sumsq, float max_norm, float tiny, float wd,
                               uint64_t seed, int64_t index0, void* stream) {
  return update_sr_entry<GradList>(param_segs, grad_segs, vs_segs, k, chunks, nchunks, dtype, lr, sumsq, max_norm, tiny, wd, seed,
                                   index0, stream);
}

int psgd_multi_param_update_mixed_sr(const void* param_segs, const void* grad_segs, const void* vs_segs, int k, const void* chunks,
                                     int64_t nchunks, int dtype, float lr, const double* sumsq, float max_norm, float tiny, float wd,
                                     uint64_t seed, int64_t index0, void* stream) {
  return update_sr_entry<GradMixed>(param_segs, grad_segs, vs_segs, k, chunks, nchunks, dtype, lr, sumsq, max_norm, tiny, wd, seed,
                                    index0, stream);
}

}  // extern "C"
