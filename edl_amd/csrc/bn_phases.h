// Per-octet and per-channel pieces of the BatchNorm kernels, one copy each:
// bnrelu.hip (row-split, three launches a pass), bn_finalize.hip and
// bn_wide.hip (channel-slab, one launch a pass) all build on them.
#pragma once
#include <type_traits>

#include "common.h"

using bf16 = __hip_bfloat16;

struct F8 {
  float v[8];
};

__device__ __forceinline__ F8 load8(const bf16* p) {
  // 16-byte vector load of 8 bf16. assume_aligned is LOAD-BEARING: from
  // bf16 pointer arithmetic LLVM infers align 2 and lowers the uint4
  // load as ushort+dwordx2+dword+ushort pieces (4 VMEM ops, seen in the
  // .s of the r2 reduce loop — the BN kernels ran 5x off roofline).
  const uint4 raw = *reinterpret_cast<const uint4*>(
      __builtin_assume_aligned(p, 16));
  F8 o;
  const ushort* u = reinterpret_cast<const ushort*>(&raw);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    union { unsigned u32; float f; } c;
    c.u32 = ((unsigned)u[i]) << 16;
    o.v[i] = c.f;
  }
  return o;
}

__device__ __forceinline__ void store8(bf16* p, const F8& x) {
  uint4 raw;
  ushort* u = reinterpret_cast<ushort*>(&raw);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    u[i] = (ushort)(__hip_bfloat16_raw(__float2bfloat16(x.v[i])).x);
  }
  *reinterpret_cast<uint4*>(__builtin_assume_aligned(p, 16)) = raw;
}

// dy_eff: keep g[k] where bit k of the fwd apply's mask byte is set.
__device__ __forceinline__ void relu_select(F8& g, const unsigned mb) {
#pragma unroll
  for (int k = 0; k < 8; ++k) g.v[k] = (mb >> k) & 1 ? g.v[k] : 0.0f;
}

// One octet of the fwd apply: v = relu?(v*scale + shift [+ res]). Returns
// the ReLU mask byte (bit k = channel c0+k positive), 0 without RELU.
// `res` points at this octet's residual and is read only with ADD.
template <bool RELU, bool ADD>
__device__ __forceinline__ unsigned char apply_octet(
    F8& v, const bf16* res, const float* __restrict__ scale,
    const float* __restrict__ shift, const int c0) {
#pragma unroll
  for (int k = 0; k < 8; ++k) v.v[k] = fmaf(v.v[k], scale[c0 + k], shift[c0 + k]);
  if (ADD) {
    F8 rv = load8(res);
#pragma unroll
    for (int k = 0; k < 8; ++k) v.v[k] += rv.v[k];
  }
  unsigned char mb = 0;
  if (RELU) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (v.v[k] > 0.0f) mb |= (1u << k);
      v.v[k] = fmaxf(v.v[k], 0.0f);
    }
  }
  return mb;
}

// One octet of dx = scale * (dy_eff - s1/M - xhat * s2/M) (TRAINING), or
// scale * dy_eff with frozen stats. g is dy_eff: loaded and masked by the
// caller, each kernel with its own load helper.
template <bool TRAINING>
__device__ __forceinline__ F8 dx_octet(
    const F8& g, const F8& xv, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ sums, const float inv_m, const int c0,
    const int C) {
  F8 o;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = c0 + k;
    const float is = invstd[c];
    if (TRAINING) {
      const float xhat = (xv.v[k] - mean[c]) * is;
      o.v[k] = gamma[c] * is *
               (g.v[k] - sums[c] * inv_m - xhat * sums[C + c] * inv_m);
    } else {
      o.v[k] = gamma[c] * is * g.v[k];
    }
  }
  return o;
}

// Channel c of the training forward finalize, from its sum and sum of
// squares over M rows: batch statistics for backward, the affine pair the
// apply pass uses, and the momentum update of the running estimates
// (rm/rv: their values as loaded; running_mean null: no update). Every
// output is indexed by c; the slab kernels pass slab-relative pointers.
// T is the type the statistics are formed in. float is bn_finalize_kernel's
// arithmetic, whose var carries the roundings of 1/M, mean^2 and the fma
// (about 1.5 ulp at an M that is no power of two). bn_wide.hip, with one
// finalize of W channels per block, takes double: mean and the unbiased
// variance then round once, to fp32, from sums that are fp32 as before.
template <typename T = float>
__device__ __forceinline__ void bn_channel_finalize(
    const float ssum, const float qsum, const float g, const float bt,
    const float rm, const float rv, const long long M, const float momentum,
    const float eps, const int c, float* __restrict__ mean_out,
    float* __restrict__ invstd_out, float* __restrict__ scale_out,
    float* __restrict__ shift_out, float* __restrict__ running_mean,
    float* __restrict__ running_var) {
  const T inv_m = (T)1 / (T)M;
  const T mean_t = ssum * inv_m;
  const T d = qsum * inv_m - mean_t * mean_t;
  const T var = std::is_same<T, float>::value ? (T)fmaxf((float)d, 0.0f)
                                              : (T)fmax((double)d, 0.0);
  const float mean = (float)mean_t;
  const float invstd = rsqrtf((float)(var + eps));
  mean_out[c] = mean;
  invstd_out[c] = invstd;
  scale_out[c] = g * invstd;
  shift_out[c] = bt - g * invstd * mean;
  if (running_mean != nullptr) {
    // unbiased variance for the running estimate (torch semantics)
    const T ub = (M > 1) ? var * (T)M / (T)(M - 1) : var;
    running_mean[c] = fmaf(momentum, mean - rm, rm);
    running_var[c] = fmaf(momentum, (float)ub - rv, rv);
  }
}

// Runtime bools -> template arguments: calls f with one std::true_type or
// std::false_type per bool, e.g.
//   dispatch_bools([&](auto R, auto A) { kernel<decltype(R)::value, ...> },
//                  relu, add);
template <class F>
static void dispatch_bools(F&& f) {
  f();
}

template <class F, class... Bools>
static void dispatch_bools(F&& f, const bool b, const Bools... rest) {
  if (b)
    dispatch_bools([&](auto... t) { f(std::true_type{}, t...); }, rest...);
  else
    dispatch_bools([&](auto... t) { f(std::false_type{}, t...); }, rest...);
}
