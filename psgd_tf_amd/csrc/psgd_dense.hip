// psgd_dense.hip -- dense preconditioner (psgd.py:26-63) on gfx950.
//
//   update (:34-42):  a = Q dg (full Q), Q' b = dx (upper triangle of Q only), G = triu(a a' - b b'),
//                     mu = step / (max|G| + tiny), Q_new = Q - mu G Q
//   apply  (:55):     Q' (Q g)
//
// G is never formed.  (G Q)[i,j] = a_i A[i,j] - b_i B[i,j] with A[i,j] = sum_{k>=i} a_k Q[k,j] and B likewise with b: suffix
// sums down each column of diag(a) Q and diag(b) Q.  The identity holds for any Q, so a Q with a non-zero lower triangle gets the
// reference's full products, and an upper-triangular Q stays upper-triangular (its lower suffix sums are exact zeros).
//
// Kernels of the update (N > kSmallN), in launch order:
//   k_gemv_rows     a = Q dg, one wave per row; also copies dx into the solve's right-hand side r
//   k_diag_inv      inverses Z[K] of the upper triangles of all 64 x 64 diagonal blocks, one wave each, in one launch
//   k_solve_step    one launch per 64-row block K of Q' b = dx: one wave forms b_K = Z[K]' r_K (the other waves load their rows
//                   of Q meanwhile), every workgroup then subtracts that block's contribution Q[K, c]' b_K from r[c] for its 64
//                   columns c right of it
//   k_sweep_a       per 64-row tile t and column j: PA[t][j] = sum_{k in t} a_k Q[k,j], PB likewise, and the tile's share of
//                   max_{i<=j} |fl(a_i a_j) - fl(b_i b_j)| (the pair max, O(N) bytes, fused into this sweep)
//   k_carry         PA, PB -> exclusive suffix over tiles (in place); workgroup 0 folds the pair maxima into mu
//   k_sweep_b       bottom-up within each tile from its carry: Q_new[k,j] = Q[k,j] - mu (a_k A[k,j] - b_k B[k,j])
// The apply is k_gemv_rows (y = Q g), k_sweep_a on y alone (column partials per tile) and k_fold (fixed-order sum over tiles).
// N <= kSmallN runs each call as one workgroup in one launch (k_small_update / k_small_apply): the 2x2 of hello_psgd.
//
// Every reduction has a fixed order and there are no atomics: repeated calls are bit-identical.  Indices into Q are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "psgd_hip.h"
#include "nanmax.h"
using psgd::amaxf;

namespace psgdd {

constexpr int kT = 256;       // threads per workgroup of the sweeps
constexpr int kB = 64;        // diagonal block of the solve == row tile of the sweeps
constexpr int kSmallN = 64;   // one-workgroup route up to here (the substitution wave holds a whole column per lane)

__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_amax(float v) {
  for (int o = 32; o > 0; o >>= 1) v = amaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float bcast(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
// |fl(a_i a_j) - fl(b_i b_j)|: the reference's matmul-then-subtract (psgd.py:40), no contraction into an fma
__device__ __forceinline__ float pair_abs(float ai, float aj, float bi, float bj) {
  return fabsf(__fsub_rn(__fmul_rn(ai, aj), __fmul_rn(bi, bj)));
}

template <int V>
__device__ __forceinline__ void load_v(const float* p, float (&q)[V]) {
  if constexpr (V == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
  } else {
    q[0] = p[0];
  }
}
template <int V>
__device__ __forceinline__ void store_v(float* p, const float (&q)[V]) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(q[0], q[1], q[2], q[3]);
  } else {
    p[0] = q[0];
  }
}

// Forward substitution Q[k0:k0+nb, k0:k0+nb]' x = r in ONE wave (call from all 64 lanes of a wave): lane j holds column j of the
// block (rows i <= j only: the upper triangle), r_j and the reciprocal of its diagonal entry; returns x_j (0 on lanes j >= nb).
// The dependent chain per row is one multiply, one v_readlane and one fma: x_i = r_i * (1 / Q_ii) (within 1.5 ulp of r_i / Q_ii).
__device__ __forceinline__ float diag_solve(const float* __restrict__ Q, int64_t N, int64_t k0, int nb, float rj) {
  const int j = threadIdx.x & 63;
  float q[kB];
#pragma unroll
  for (int i = 0; i < kB; ++i) q[i] = (i <= j && j < nb) ? Q[(k0 + i) * N + k0 + j] : 0.f;
  const float inv = j < nb ? 1.f / Q[(k0 + j) * N + k0 + j] : 0.f;
  float xj = 0.f;
#pragma unroll
  for (int i = 0; i < kB; ++i) {
    if (i < nb) {
      const float xi = bcast(rj * inv, i);
      if (j == i) xj = xi;
      if (j > i) rj = fmaf(-q[i], xi, rj);
    }
  }
  return xj;
}

// y = Q x, one wave per row; dst[row] = src[row] alongside when dst is set (the solve's right-hand side)
template <int V>
__global__ __launch_bounds__(kT) void k_gemv_rows(const float* __restrict__ Q, const float* __restrict__ x, float* __restrict__ y,
                                                  int64_t N, const float* __restrict__ src, float* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* q = Q + row * N;
  float s = 0.f;
#pragma unroll 4
  for (int64_t k = (int64_t)lane * V; k < N; k += 64 * V) {
    float v[V];
    load_v<V>(q + k, v);
#pragma unroll
    for (int e = 0; e < V; ++e) s = fmaf(v[e], x[k + e], s);
  }
  s = wave_sum(s);
  if (lane == 0) {
    y[row] = s;
    if (dst) dst[row] = src[row];
  }
}

// Z[K] = inverse of the upper triangle of the diagonal block K of Q (64 x 64, identity-padded past N), one wave per block: lane c
// back-substitutes column c of Z on its own (no cross-lane chain), the block's rows broadcast from LDS.  Z[K][i][c], row-major.
__global__ __launch_bounds__(64) void k_diag_inv(const float* __restrict__ Q, float* __restrict__ Z, int64_t N) {
  __shared__ float U[kB][kB + 1];
  const int64_t k0 = (int64_t)blockIdx.x * kB;
  const int nb = (int)(N - k0 < kB ? N - k0 : kB), c = threadIdx.x;
  for (int i = 0; i < kB; ++i) U[i][c] = (i <= c && c < nb) ? Q[(k0 + i) * N + k0 + c] : (i == c ? 1.f : 0.f);
  __syncthreads();
  float z[kB];
#pragma unroll
  for (int i = kB - 1; i >= 0; --i) {
    float s = (i == c) ? 1.f : 0.f;
#pragma unroll
    for (int k = i + 1; k < kB; ++k) s = fmaf(-U[i][k], z[k], s);
    z[i] = s / U[i][i];
  }
  float* zk = Z + (int64_t)blockIdx.x * kB * kB;
#pragma unroll
  for (int i = 0; i < kB; ++i) zk[i * kB + c] = z[i];
}

// Block K (rows k0 .. k0+63) of Q' b = r: b_K = Z[K]' r_K (one wave, 64 independent products: no substitution chain), then
// r[c] -= sum_i Q[k0+i, c] b_i for the 64 columns c = k0 + 64 + 64 blockIdx.x + lane, the 64 rows split over the four waves and
// folded in a fixed order.
__global__ __launch_bounds__(kT) void k_solve_step(const float* __restrict__ Q, const float* __restrict__ Z, float* __restrict__ r,
                                                   float* __restrict__ b, int64_t N, int64_t k0) {
  constexpr int kRows = kB / (kT / 64);                 // rows of the block per wave in the trailing update
  __shared__ float sb[kB];
  __shared__ float part[kT / 64][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nb = (int)(N - k0 < kB ? N - k0 : kB);
  const int64_t c = k0 + kB + (int64_t)blockIdx.x * 64 + lane;
  const bool live = c < N;                              // then N > k0 + kB: nb == kB
  const int i0 = w * kRows;
  float qc[kRows];                                      // loaded ahead of the block product: their latency hides behind it
#pragma unroll
  for (int i = 0; i < kRows; ++i) qc[i] = live ? Q[(k0 + i0 + i) * N + c] : 0.f;
  if (w == 0) {
    const float* zk = Z + (k0 / kB) * kB * kB;
    float zc[kB];
#pragma unroll
    for (int i = 0; i < kB; ++i) zc[i] = zk[i * kB + lane];
    const float rv = lane < nb ? r[k0 + lane] : 0.f;
    float xj = 0.f;
#pragma unroll
    for (int i = 0; i < kB; ++i) xj = fmaf(zc[i], bcast(rv, i), xj);
    sb[lane] = xj;
    if (blockIdx.x == 0 && lane < nb) b[k0 + lane] = xj;
  }
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kRows; ++i) s = fmaf(qc[i], sb[i0 + i], s);
  part[w][lane] = s;
  __syncthreads();
  if (w == 0 && live) r[c] -= (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

// Column partials of one 64-row tile (blockIdx.y) over kT * V columns (blockIdx.x).  UPD: of a and b, plus the tile's pair max
// over the (k, j) with k in the tile, j in the columns, k <= j -> pm[tile * gridDim.x + blockIdx.x].  Else: of a alone.
template <int V, bool UPD>
__global__ __launch_bounds__(kT) void k_sweep_a(const float* __restrict__ Q, const float* __restrict__ a,
                                                const float* __restrict__ b, float* __restrict__ PA, float* __restrict__ PB,
                                                float* __restrict__ pm, int64_t N) {
  const int64_t t = blockIdx.y, k0 = t * kB, k1 = (k0 + kB < N) ? k0 + kB : N;
  const int64_t j0 = ((int64_t)blockIdx.x * kT + threadIdx.x) * V;
  float m = 0.f;
  if (j0 < N) {
    float sa[V], sb[V], aj[V], bj[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      sa[e] = sb[e] = 0.f;
      aj[e] = UPD ? a[j0 + e] : 0.f;
      bj[e] = UPD ? b[j0 + e] : 0.f;
    }
#pragma unroll 8
    for (int64_t k = k0; k < k1; ++k) {
      float q[V];
      load_v<V>(Q + k * N + j0, q);
      const float ak = a[k];
      const float bk = UPD ? b[k] : 0.f;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        sa[e] = fmaf(ak, q[e], sa[e]);
        if (UPD) {
          sb[e] = fmaf(bk, q[e], sb[e]);
          if (k <= j0 + e) m = amaxf(m, pair_abs(ak, aj[e], bk, bj[e]));
        }
      }
    }
    store_v<V>(PA + t * N + j0, sa);
    if (UPD) store_v<V>(PB + t * N + j0, sb);
  }
  if (UPD) {
    __shared__ float red[kT / 64];
    m = wave_amax(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) pm[t * gridDim.x + blockIdx.x] = amaxf(amaxf(red[0], red[1]), amaxf(red[2], red[3]));
  }
}

// PA, PB [T][N] -> their exclusive suffix sums over tiles, in place; workgroup 0 also folds the pair maxima into
// mu = step / (max + tiny) (psgd.py:41; a NaN anywhere makes mu NaN: nanmax.h)
__global__ __launch_bounds__(64) void k_carry(float* __restrict__ PA, float* __restrict__ PB, const float* __restrict__ pm, int npm,
                                              float* __restrict__ mu, int64_t N, int64_t T, float step, float tiny) {
  const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (j < N) {
    float ra = 0.f, rb = 0.f;
#pragma unroll 8
    for (int64_t t = T - 1; t >= 0; --t) {
      const float pa = PA[t * N + j], pb = PB[t * N + j];
      PA[t * N + j] = ra;
      PB[t * N + j] = rb;
      ra += pa;
      rb += pb;
    }
  }
  if (blockIdx.x == 0) {
    float m = 0.f;
    for (int i = threadIdx.x; i < npm; i += 64) m = amaxf(m, pm[i]);
    m = wave_amax(m);
    if (threadIdx.x == 0) mu[0] = __fdiv_rn(step, __fadd_rn(m, tiny));
  }
}

// Q_new[k, j] = Q[k, j] - mu (a_k A[k, j] - b_k B[k, j]), walking the tile bottom-up from the carries CA, CB of the tiles below
template <int V>
__global__ __launch_bounds__(kT) void k_sweep_b(const float* __restrict__ Q, const float* __restrict__ a, const float* __restrict__ b,
                                                const float* __restrict__ CA, const float* __restrict__ CB,
                                                const float* __restrict__ mu_p, float* __restrict__ Qout, int64_t N) {
  const int64_t t = blockIdx.y, k0 = t * kB, k1 = (k0 + kB < N) ? k0 + kB : N;
  const int64_t j0 = ((int64_t)blockIdx.x * kT + threadIdx.x) * V;
  if (j0 >= N) return;
  const float mu = mu_p[0];
  float sa[V], sb[V];
  load_v<V>(CA + t * N + j0, sa);
  load_v<V>(CB + t * N + j0, sb);
#pragma unroll 8
  for (int64_t k = k1 - 1; k >= k0; --k) {
    float q[V], o[V];
    load_v<V>(Q + k * N + j0, q);
    const float ak = a[k], bk = b[k];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      sa[e] = fmaf(ak, q[e], sa[e]);
      sb[e] = fmaf(bk, q[e], sb[e]);
      o[e] = q[e] - mu * (ak * sa[e] - bk * sb[e]);
    }
    store_v<V>(Qout + k * N + j0, o);
  }
}

// out[j] = sum_t P[t][j], t ascending
__global__ __launch_bounds__(64) void k_fold(const float* __restrict__ P, float* __restrict__ out, int64_t N, int64_t T) {
  const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (j >= N) return;
  float s = 0.f;
#pragma unroll 8
  for (int64_t t = 0; t < T; ++t) s += P[t * N + j];
  out[j] = s;
}

// N <= kSmallN: the whole update in one workgroup
__global__ __launch_bounds__(kT) void k_small_update(const float* __restrict__ Q, const float* __restrict__ dx,
                                                     const float* __restrict__ dg, float* __restrict__ Qout, int N, float step,
                                                     float tiny) {
  __shared__ float sa[64], sb[64], red[kT / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (w == 0) {
    float s = 0.f;
    if (lane < N)
      for (int k = 0; k < N; ++k) s = fmaf(Q[(int64_t)lane * N + k], dg[k], s);
    sa[lane] = s;
    sb[lane] = diag_solve(Q, N, 0, N, lane < N ? dx[lane] : 0.f);
  }
  __syncthreads();
  float m = 0.f;
  for (int p = tid; p < 64 * 64; p += kT) {
    const int i = p >> 6, j = p & 63;
    if (i <= j && j < N) m = amaxf(m, pair_abs(sa[i], sa[j], sb[i], sb[j]));
  }
  m = wave_amax(m);
  if (lane == 0) red[w] = m;
  __syncthreads();
  const float mu = __fdiv_rn(step, __fadd_rn(amaxf(amaxf(red[0], red[1]), amaxf(red[2], red[3])), tiny));
  if (tid < N) {
    float A = 0.f, B = 0.f;
    for (int k = N - 1; k >= 0; --k) {
      const float q = Q[(int64_t)k * N + tid];
      A = fmaf(sa[k], q, A);
      B = fmaf(sb[k], q, B);
      Qout[(int64_t)k * N + tid] = q - mu * (sa[k] * A - sb[k] * B);
    }
  }
}

__global__ __launch_bounds__(kT) void k_small_apply(const float* __restrict__ Q, const float* __restrict__ g,
                                                    float* __restrict__ out, int N) {
  __shared__ float y[64];
  const int tid = threadIdx.x;
  if (tid < 64) {
    float s = 0.f;
    if (tid < N)
      for (int k = 0; k < N; ++k) s = fmaf(Q[(int64_t)tid * N + k], g[k], s);
    y[tid] = s;
  }
  __syncthreads();
  if (tid < N) {
    float s = 0.f;
    for (int i = 0; i < N; ++i) s = fmaf(Q[(int64_t)i * N + tid], y[i], s);
    out[tid] = s;
  }
}

// workspace: a, b, r [N], mu, pair maxima [T][ceil(N / kT)], PA, PB [T][N], inverses of the diagonal blocks Z [T][64][64]; every
// region 256-byte aligned
struct DenseWs {
  float *a, *b, *r, *mu, *pm, *PA, *PB, *Z;
  int64_t T, bytes;
};
static DenseWs dense_layout(void* base, int64_t N) {
  DenseWs w;
  w.T = (N + kB - 1) / kB;
  int64_t off = 0;
  auto take = [&](int64_t n) {
    float* p = base ? static_cast<float*>(base) + off : nullptr;
    off += (n + 63) / 64 * 64;
    return p;
  };
  w.a = take(N);
  w.b = take(N);
  w.r = take(N);
  w.mu = take(1);
  w.pm = take(w.T * ((N + kT - 1) / kT));
  w.PA = take(w.T * N);
  w.PB = take(w.T * N);
  w.Z = take(w.T * kB * kB);
  w.bytes = off * (int64_t)sizeof(float);
  return w;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int ws_check(const void* ws, int64_t ws_bytes, int64_t N) {
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) || ws_bytes < dense_layout(nullptr, N).bytes) return PSGD_ERR_WORKSPACE;
  return PSGD_OK;
}

static int launched() { return hipGetLastError() == hipSuccess ? PSGD_OK : PSGD_ERR_LAUNCH; }

template <int V>
static int update_large(const float* Q, const float* dx, const float* dg, float* Qout, int64_t N, float step, float tiny,
                        const DenseWs& w, hipStream_t st) {
  const dim3 sweep((unsigned)((N + (int64_t)kT * V - 1) / ((int64_t)kT * V)), (unsigned)w.T);
  hipLaunchKernelGGL(k_gemv_rows<V>, dim3((unsigned)((N + kT / 64 - 1) / (kT / 64))), dim3(kT), 0, st, Q, dg, w.a, N, dx, w.r);
  hipLaunchKernelGGL(k_diag_inv, dim3((unsigned)w.T), dim3(64), 0, st, Q, w.Z, N);
  for (int64_t K = 0; K < w.T; ++K) {
    const int64_t right = N - (K + 1) * kB;
    const unsigned grid = right > 0 ? (unsigned)((right + 63) / 64) : 1u;
    hipLaunchKernelGGL(k_solve_step, dim3(grid), dim3(kT), 0, st, Q, w.Z, w.r, w.b, N, K * kB);
  }
  hipLaunchKernelGGL((k_sweep_a<V, true>), sweep, dim3(kT), 0, st, Q, w.a, w.b, w.PA, w.PB, w.pm, N);
  hipLaunchKernelGGL(k_carry, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, w.PA, w.PB, w.pm, (int)(sweep.x * sweep.y), w.mu, N,
                     w.T, step, tiny);
  hipLaunchKernelGGL(k_sweep_b<V>, sweep, dim3(kT), 0, st, Q, w.a, w.b, w.PA, w.PB, w.mu, Qout, N);
  return launched();
}

template <int V>
static int apply_large(const float* Q, const float* g, float* out, int64_t N, const DenseWs& w, hipStream_t st) {
  const dim3 sweep((unsigned)((N + (int64_t)kT * V - 1) / ((int64_t)kT * V)), (unsigned)w.T);
  hipLaunchKernelGGL(k_gemv_rows<V>, dim3((unsigned)((N + kT / 64 - 1) / (kT / 64))), dim3(kT), 0, st, Q, g, w.a, N, nullptr, nullptr);
  hipLaunchKernelGGL((k_sweep_a<V, false>), sweep, dim3(kT), 0, st, Q, w.a, nullptr, w.PA, nullptr, nullptr, N);
  hipLaunchKernelGGL(k_fold, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, w.PA, out, N, w.T);
  return launched();
}

}  // namespace psgdd

using namespace psgdd;

extern "C" {

int64_t psgd_dense_workspace_bytes(int64_t N) {
  if (N <= 0) return PSGD_ERR_BAD_ARG;
  return dense_layout(nullptr, N).bytes;
}

int psgd_dense_update_f32(const float* Q, const float* dx, const float* dg, float* Qout, int64_t N, float step, float tiny,
                          void* ws, int64_t ws_bytes, void* stream) {
  if (!Q || !dx || !dg || !Qout || N <= 0 || Qout == Q) return PSGD_ERR_BAD_ARG;
  if (ws_check(ws, ws_bytes, N)) return PSGD_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (N <= kSmallN) {
    hipLaunchKernelGGL(k_small_update, dim3(1), dim3(kT), 0, st, Q, dx, dg, Qout, (int)N, step, tiny);
    return launched();
  }
  const DenseWs w = dense_layout(ws, N);
  if (N % 4 == 0 && aligned16(Q) && aligned16(Qout)) return update_large<4>(Q, dx, dg, Qout, N, step, tiny, w, st);
  return update_large<1>(Q, dx, dg, Qout, N, step, tiny, w, st);
}

int psgd_dense_apply_f32(const float* Q, const float* g, float* out, int64_t N, void* ws, int64_t ws_bytes, void* stream) {
  if (!Q || !g || !out || N <= 0) return PSGD_ERR_BAD_ARG;
  if (ws_check(ws, ws_bytes, N)) return PSGD_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (N <= kSmallN) {
    hipLaunchKernelGGL(k_small_apply, dim3(1), dim3(kT), 0, st, Q, g, out, (int)N);
    return launched();
  }
  const DenseWs w = dense_layout(ws, N);
  if (N % 4 == 0 && aligned16(Q)) return apply_large<4>(Q, g, out, N, w, st);
  return apply_large<1>(Q, g, out, N, w, st);
}

}  // extern "C"
