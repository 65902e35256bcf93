// Global gradient norm over the flat fp32 buckets, and the device-side clip
// state the update kernels (fused_sgd.hip, fused_adam.hip) read.
//
// Gradients live as views into flat per-bucket buffers
// (edl_amd/train/bucketed_ddp.py) and the 1/world average is folded into
// the update kernel, so the true gradient is never materialised: clipping
// by global norm (torch.nn.utils.clip_grad_norm_) has to be two small
// kernels in front of the update, with nothing on the host in between — a
// whole step replays as one hipGraph.
//
//   grad_sumsq_f32      per-block partial sums of squares of up to
//                       kGradNormMaxSegs buffers in ONE launch
//                       (blockIdx.y = buffer, blockIdx.x = row)
//   grad_clip_finalize  one block: sums the rows in a fixed order, writes
//                       state = [coef, norm, skip, nskipped]
//
// Every element is squared and accumulated in DOUBLE — per lane, through the
// wave fold, the LDS fold across waves and the stored partial: no overflow
// below 1e154 and an arithmetic error (~n * 2^-53) far under the one
// rounding of the result to fp32. Memory-bound all the same: one read of
// 4 B per element, float4 loads (guide Guideline 13), grid-stride, scalar
// tail for n % 4.
//
// EVERY block of a buffer's rows stores its row, a block without elements
// stores 0.0: the partial buffer needs no fill launch (torch.empty) and a
// graph replay never sees a stale row — the bn_apply_pad halo idiom. No
// atomics anywhere: the row a block writes and the order rows are summed
// in depend on the launch geometry alone, so the result is bitwise
// reproducible (guide Guideline 12, last paragraph).
#include "common.h"
#include "launchers.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;

// block sum in a fixed order: lanes by shuffle, then wave 0..3 in sequence;
// valid in thread 0
__device__ __forceinline__ double block_reduce_sum_f64(double v, double* s_w) {
  v = wave_reduce_sum_f64(v);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) s_w[wave] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kWaves; ++w) t += s_w[w];
  }
  return t;
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void grad_sumsq_f32(
    const GradNormSegs segs, double* __restrict__ partial) {
  __shared__ double s_w[kWaves];
  const int b = blockIdx.y;
  const int rows = segs.rows[b];
  const int row = blockIdx.x;
  if (row >= rows) return;  // the grid is sized for the largest buffer
  const long long n = segs.n[b];
  const float* g =
      static_cast<const float*>(__builtin_assume_aligned(segs.ptr[b], 16));
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const long long n4 = n >> 2;
  const long long stride = (long long)rows * kBlock;
  const long long first = (long long)row * kBlock + threadIdx.x;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
  for (long long i = first; i < n4; i += stride) {
    const float4 x = g4[i];
    sq_acc(a0, x.x);
    sq_acc(a1, x.y);
    sq_acc(a2, x.z);
    sq_acc(a3, x.w);
  }
  // tail (n % 4)
  for (long long j = (n4 << 2) + first; j < n; j += stride) sq_acc(a0, g[j]);
  const double t = block_reduce_sum_f64((a0 + a1) + (a2 + a3), s_w);
  if (threadIdx.x == 0) partial[segs.row_off[b] + row] = t;
}

// state = [coef, norm, skip, nskipped] (fp32). norm = grad_scale * sqrt(sum)
// in double, rounded once; coef = clamp(max_norm / (norm + 1e-6), max=1) in
// fp32 exactly as torch.nn.utils.clip_grad_norm_ forms it, a NaN quotient
// staying NaN (torch.clamp propagates it; fminf would not).
extern "C" __global__ __launch_bounds__(256) void grad_clip_finalize(
    const double* __restrict__ partial, const int rows_total,
    const double grad_scale, const float max_norm, const int skip_nonfinite,
    float* __restrict__ state) {
  __shared__ double s_w[kWaves];
  // thread t adds rows t, t+256, ... in that order; unrolled so 8 loads are
  // in flight at a time (the adds keep their sequence)
  double acc = 0.0;
#pragma unroll 8
  for (int r = threadIdx.x; r < rows_total; r += kBlock) acc += partial[r];
  const double sum = block_reduce_sum_f64(acc, s_w);
  if (threadIdx.x != 0) return;
  const float norm = (float)(grad_scale * sqrt(sum));
  const float q = max_norm / (norm + 1e-6f);
  float coef = q > 1.0f ? 1.0f : q;
  float skip = 0.0f;
  if (skip_nonfinite != 0 && !isfinite(norm)) {
    skip = 1.0f;
    coef = 0.0f;
    state[3] += 1.0f;
  }
  state[0] = coef;
  state[1] = norm;
  state[2] = skip;
}

extern "C" int grad_norm_rows(long long n) {
  const long long want = ((n + 3) / 4 + kBlock - 1) / kBlock;
  if (want < 1) return 1;  // an empty buffer still owns one row (0.0)
  return (int)(want < kGradNormRowCap ? want : kGradNormRowCap);
}

extern "C" void launch_grad_sumsq_f32(const GradNormSegs* segs,
                                      double* partial, hipStream_t stream) {
  int max_rows = 0;
  for (int k = 0; k < segs->nseg; ++k)
    max_rows = segs->rows[k] > max_rows ? segs->rows[k] : max_rows;
  if (segs->nseg <= 0 || max_rows <= 0) return;
  hipLaunchKernelGGL(grad_sumsq_f32, dim3(max_rows, segs->nseg), dim3(kBlock),
                     0, stream, *segs, partial);
}

extern "C" void launch_grad_clip_finalize(const double* partial,
                                          int rows_total, double grad_scale,
                                          float max_norm, int skip_nonfinite,
                                          float* state, hipStream_t stream) {
  hipLaunchKernelGGL(grad_clip_finalize, dim3(1), dim3(kBlock), 0, stream,
                     partial, rows_total, grad_scale, max_norm,
                     skip_nonfinite, state);
}
