// Fused hard-label softmax cross-entropy with label smoothing, optional
// mixup (two labels + per-row weight) and the rank of the true class.
//
// forward, per row i (w = lam_i, or 1 without mixup):
//   lse_i  = logsumexp_j s_ij
//   loss_i = lse_i - (1-eps)*(w*s[i,a_i] + (1-w)*s[i,b_i]) - (eps/C)*sum_j s_ij
//   rank_i = #{j : s_ij > s_ia} + #{j < a_i : s_ij == s_ia}
// backward:
//   ds_ij  = (exp(s_ij - lse_i) - q_ij) * gout / B
//   q_ij   = (1-eps)*(w*[j==a_i] + (1-w)*[j==b_i]) + eps/C
//
// The reference trainer's calc_loss (example/collective/resnet50/
// train_with_fleet.py: label_smooth + softmax_with_cross_entropy, mixed
// by lam) and its acc_top1/acc_top5 in ONE read of the logits. One
// 256-thread workgroup per row like kd_loss.hip, but a single pass:
// every lane keeps a running (max, sum exp) pair, the pairs are merged
// per wave with the common.h shuffles and across the 4 waves by one LDS
// round. No atomics: results are bit-reproducible. gout is read from
// DEVICE memory so forward+backward capture into a hipGraph (the KD
// wrapper's float(gout) is a host sync).
//
// Labels outside [0, C) are never dereferenced: such a label contributes
// no target term to loss or gradient (the eps/C smoothing term stays)
// and, for y_a, reports rank = C (never top-k correct).
#include "common.h"
#include "launchers.h"

namespace {

constexpr int kThreads = 256;
constexpr float kNegBig = -1e30f;  // finite "-inf": exp(kNegBig - m) == 0

template <typename T>
struct VecOf;
template <>
struct VecOf<float> { static constexpr int N = 4; };
template <>
struct VecOf<__hip_bfloat16> { static constexpr int N = 8; };

template <typename T>
__device__ __forceinline__ float ld1(const T* p);
template <>
__device__ __forceinline__ float ld1<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float ld1<__hip_bfloat16>(const __hip_bfloat16* p) {
  return __bfloat162float(*p);
}
template <typename T>
__device__ __forceinline__ void st1(T* p, float v);
template <>
__device__ __forceinline__ void st1<float>(float* p, float v) { *p = v; }
template <>
__device__ __forceinline__ void st1<__hip_bfloat16>(__hip_bfloat16* p, float v) {
  *p = __float2bfloat16(v);
}

// 16-byte vector load/store of VecOf<T>::N elements. Vector path only:
// the launcher guarantees 16-B aligned rows, and assume_aligned keeps
// LLVM from splitting the access (it infers align 2 from bf16 pointer
// arithmetic — see the alignment note in docs/kernels.md).
__device__ __forceinline__ void ldv(const float* p, float* o) {
  const float4 r = *reinterpret_cast<const float4*>(__builtin_assume_aligned(p, 16));
  o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
}
__device__ __forceinline__ void ldv(const __hip_bfloat16* p, float* o) {
  const uint4 r = *reinterpret_cast<const uint4*>(__builtin_assume_aligned(p, 16));
  const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[2 * i] = __uint_as_float(w[i] << 16);
    o[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ void stv(float* p, const float* v) {
  *reinterpret_cast<float4*>(__builtin_assume_aligned(p, 16)) =
      make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void stv(__hip_bfloat16* p, const float* v) {
  unsigned w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned lo = __hip_bfloat16_raw(__float2bfloat16(v[2 * i])).x;
    const unsigned hi = __hip_bfloat16_raw(__float2bfloat16(v[2 * i + 1])).x;
    w[i] = lo | (hi << 16);
  }
  *reinterpret_cast<uint4*>(__builtin_assume_aligned(p, 16)) =
      make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ int wave_reduce_sum_i32(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// running per-lane state of the single pass
struct RowAcc {
  float m = kNegBig;  // running max
  float e = 0.f;      // sum exp(x - m)
  float t = 0.f;      // plain sum (smoothing term)
  int r = 0;          // rank contribution

  __device__ __forceinline__ void add(float x, int j, float sa, int a) {
    if (x > m) {
      e = e * __expf(m - x) + 1.f;
      m = x;
    } else {
      e += __expf(x - m);
    }
    t += x;
    r += (x > sa) || (x == sa && j < a);
  }
};

template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void softmax_ce_fwd_kernel(
    const T* __restrict__ s, const long long* __restrict__ ya,
    const long long* __restrict__ yb, const float* __restrict__ lam,
    float* __restrict__ loss_row, float* __restrict__ lse_out,
    int* __restrict__ rank_out, const float eps, const int C) {
  __shared__ float lds_m[4], lds_e[4], lds_t[4];
  __shared__ int lds_r[4];
  const int row = blockIdx.x;
  const T* srow = s + (long long)row * C;

  // true-class logits first (the rank needs s_ia during the pass);
  // out-of-range labels are not dereferenced
  const long long a = ya[row];
  const bool a_ok = a >= 0 && a < C;
  const float sa = a_ok ? ld1(srow + a) : 0.f;
  const int ai = a_ok ? (int)a : 0;

  RowAcc acc;
  if (VEC) {
    constexpr int N = VecOf<T>::N;
    const int nvec = C / N;  // exact: C*sizeof(T) % 16 == 0 on this path
    for (int v = threadIdx.x; v < nvec; v += kThreads) {
      float x[N];
      ldv(srow + v * N, x);
#pragma unroll
      for (int i = 0; i < N; ++i) acc.add(x[i], v * N + i, sa, ai);
    }
  } else {
    for (int j = threadIdx.x; j < C; j += kThreads)
      acc.add(ld1(srow + j), j, sa, ai);
  }

  // merge the (max, sum) pairs: per wave, then the 4 waves through LDS
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float wm = __shfl(wave_reduce_max(acc.m), 0, 64);
  const float we = wave_reduce_sum(acc.e * __expf(acc.m - wm));
  const float wt = wave_reduce_sum(acc.t);
  const int wr = wave_reduce_sum_i32(acc.r);
  if (lane == 0) {
    lds_m[wid] = wm;
    lds_e[wid] = we;
    lds_t[wid] = wt;
    lds_r[wid] = wr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float M = fmaxf(fmaxf(lds_m[0], lds_m[1]), fmaxf(lds_m[2], lds_m[3]));
    float E = 0.f, S = 0.f;
    int R = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      E += lds_e[w] * __expf(lds_m[w] - M);
      S += lds_t[w];
      R += lds_r[w];
    }
    const float lse = M + __logf(E);
    float tgt = a_ok ? sa : 0.f;
    if (yb != nullptr) {
      const float w = lam[row];
      const long long b = yb[row];
      const float sb = (b >= 0 && b < C) ? ld1(srow + b) : 0.f;
      tgt = w * tgt + (1.f - w) * sb;
    }
    loss_row[row] = lse - (1.f - eps) * tgt - (eps / (float)C) * S;
    lse_out[row] = lse;
    rank_out[row] = a_ok ? R : C;
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void softmax_ce_bwd_kernel(
    const T* __restrict__ s, const float* __restrict__ lse,
    const long long* __restrict__ ya, const long long* __restrict__ yb,
    const float* __restrict__ lam, const float* __restrict__ gout,
    T* __restrict__ ds, const float eps, const float inv_B, const int C) {
  const int row = blockIdx.x;
  const T* srow = s + (long long)row * C;
  T* drow = ds + (long long)row * C;
  const float g = gout[0] * inv_B;
  const float l = lse[row];
  const float q0 = eps / (float)C;
  // out-of-range labels match no column (j >= 0 always)
  const long long a64 = ya[row];
  const int a = (a64 >= 0 && a64 < C) ? (int)a64 : -1;
  int b = -1;
  float qa = 1.f - eps, qb = 0.f;
  if (yb != nullptr) {
    const float w = lam[row];
    const long long b64 = yb[row];
    b = (b64 >= 0 && b64 < C) ? (int)b64 : -1;
    qa = (1.f - eps) * w;
    qb = (1.f - eps) * (1.f - w);
  }
  if (VEC) {
    constexpr int N = VecOf<T>::N;
    const int nvec = C / N;
    for (int v = threadIdx.x; v < nvec; v += kThreads) {
      float x[N];
      ldv(srow + v * N, x);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int j = v * N + i;
        const float q = q0 + (j == a ? qa : 0.f) + (j == b ? qb : 0.f);
        x[i] = (__expf(x[i] - l) - q) * g;
      }
      stv(drow + v * N, x);
    }
  } else {
    for (int j = threadIdx.x; j < C; j += kThreads) {
      const float q = q0 + (j == a ? qa : 0.f) + (j == b ? qb : 0.f);
      st1(drow + j, (__expf(ld1(srow + j) - l) - q) * g);
    }
  }
}

// 16 bytes per lane needs every row 16-B aligned: the base pointer and
// the row pitch C*sizeof(T). An odd-C bf16 matrix fails the second.
template <typename T>
bool vec_ok(const void* s, const void* ds, int C) {
  return ((size_t)C * sizeof(T)) % 16 == 0 && ((uintptr_t)s % 16) == 0 &&
         ((uintptr_t)ds % 16) == 0;
}

template <typename T>
void launch_fwd(const void* s, const long long* ya, const long long* yb,
                const float* lam, float* loss_row, float* lse, int* rank,
                float eps, int B, int C, hipStream_t stream) {
  if (vec_ok<T>(s, nullptr, C))
    hipLaunchKernelGGL((softmax_ce_fwd_kernel<T, true>), dim3(B), dim3(kThreads),
                       0, stream, (const T*)s, ya, yb, lam, loss_row, lse, rank,
                       eps, C);
  else
    hipLaunchKernelGGL((softmax_ce_fwd_kernel<T, false>), dim3(B), dim3(kThreads),
                       0, stream, (const T*)s, ya, yb, lam, loss_row, lse, rank,
                       eps, C);
}

template <typename T>
void launch_bwd(const void* s, const float* lse, const long long* ya,
                const long long* yb, const float* lam, const float* gout,
                void* ds, float eps, float inv_B, int B, int C,
                hipStream_t stream) {
  if (vec_ok<T>(s, ds, C))
    hipLaunchKernelGGL((softmax_ce_bwd_kernel<T, true>), dim3(B), dim3(kThreads),
                       0, stream, (const T*)s, lse, ya, yb, lam, gout, (T*)ds,
                       eps, inv_B, C);
  else
    hipLaunchKernelGGL((softmax_ce_bwd_kernel<T, false>), dim3(B), dim3(kThreads),
                       0, stream, (const T*)s, lse, ya, yb, lam, gout, (T*)ds,
                       eps, inv_B, C);
}

}  // namespace

extern "C" void launch_softmax_ce_fwd(const void* s, int is_bf16,
                                      const long long* ya, const long long* yb,
                                      const float* lam, float* loss_row,
                                      float* lse, int* rank, float eps, int B,
                                      int C, hipStream_t stream) {
  if (B <= 0) return;
  if (is_bf16)
    launch_fwd<__hip_bfloat16>(s, ya, yb, lam, loss_row, lse, rank, eps, B, C, stream);
  else
    launch_fwd<float>(s, ya, yb, lam, loss_row, lse, rank, eps, B, C, stream);
}

extern "C" void launch_softmax_ce_bwd(const void* s, int is_bf16,
                                      const float* lse, const long long* ya,
                                      const long long* yb, const float* lam,
                                      const float* gout, void* ds, float eps,
                                      float inv_B, int B, int C,
                                      hipStream_t stream) {
  if (B <= 0) return;
  if (is_bf16)
    launch_bwd<__hip_bfloat16>(s, lse, ya, yb, lam, gout, ds, eps, inv_B, B, C, stream);
  else
    launch_bwd<float>(s, lse, ya, yb, lam, gout, ds, eps, inv_B, B, C, stream);
}
