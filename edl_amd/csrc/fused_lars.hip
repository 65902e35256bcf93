// Fused LARS (layer-wise adaptive rate scaling, Paddle's lars_momentum) over
// the flat parameter buckets (fp32).
//
// With s the gradient scale the update kernels form (grad_scale times the
// clip coefficient), for every parameter tensor k with decay wd_k:
//
//   pn = sqrt(sum p^2)        gn = s * sqrt(sum g^2)          (over tensor k)
//   trust = coeff * pn / (gn + wd_k*pn + eps)   if wd_k, pn, gn > 0, else 1
//   v = mu*v + (lr*trust) * (s*g + wd_k*p)      (velocity holds the LR)
//   p -= v
//
// Excluded tensors (biases, norm scale/shift) have wd_k = 0: plain lr, no
// decay. Three kernels, all on the caller's stream, nothing on the host in
// between (a whole step replays as one hipGraph):
//
//   lars_sumsq_f32   one block per row of a device CHUNK TABLE built once
//                    (ops/lars.py): {bucket, start, len}, len <= kLarsChunk,
//                    never across a tensor boundary. Up to kLarsMaxBufs
//                    buckets per launch, so the launch count does not grow
//                    with the number of tensors. Each block stores its two
//                    double partials {sum p^2, sum g^2} unconditionally: no
//                    atomics, no fill launch, no stale slot on a graph
//                    replay (the grad_norm.hip idiom, and its fold order).
//   lars_trust_f32   one WAVE per tensor adds the tensor's chunk partials in
//                    ascending chunk order and writes trust[k] (1.0 for a
//                    tensor without chunks) on every launch.
//   fused_lars_f32   one launch per bucket, shaped like fused_adam_f32:
//                    seg_end / seg_wd / lr*trust tables in LDS, looked up
//                    per ELEMENT (a float4 may straddle a boundary, a
//                    segment may be shorter than a vector).
//
// Memory-bound: 2 reads per element for the norms, 3 reads + 2 writes for
// the update, float4 throughout (guide Guideline 13). Tensors sit at
// arbitrary offsets in a bucket (no padding), so a chunk starts at any
// offset mod 4: the reduction peels to 16-byte alignment, runs float4, and
// ends with a scalar tail.
//
// Every table value is clamped before it is used as an index or an extent:
// a malformed table gives wrong numbers, never an access outside the
// buffers (the bindings check the tables once; under stream capture they
// cannot).
#include "flat_update.h"
#include "launchers.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kTrustRounds = kLarsTrustPreload / kWave;
static_assert(kLarsTrustPreload % kWave == 0, "whole 64-chunk rounds");

// lane l's value in every lane, l wave-uniform: two v_readlane_b32 through
// SGPRs, where a __shfl is a ds_bpermute round trip in every step of a
// dependent add chain.
__device__ __forceinline__ double readlane_f64(const double v, const int l) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ long long clampll(long long x, long long lo,
                                             long long hi) {
  return x < lo ? lo : (x > hi ? hi : x);
}

// d = s*g + wd*p; v = mu*v + llr*d; p -= v  (llr = lr * trust)
__device__ __forceinline__ void lars_elem(const float s, const float mu,
                                          const float wd, const float llr,
                                          const float g, float& p, float& v) {
  const float d = fmaf(s, g, wd * p);
  v = fmaf(mu, v, llr * d);
  p -= v;
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void lars_sumsq_f32(
    const LarsBufs bufs, const int4* __restrict__ chunks, const int chunk_base,
    double* __restrict__ partial) {
  __shared__ double s_p[kWaves], s_g[kWaves];
  const int c = chunk_base + blockIdx.x;
  const int4 e = chunks[c];  // {bucket, start, len, 0}
  const int b = (int)clampll(e.x - bufs.first, 0, bufs.nbuf - 1);
  const long long n = bufs.n[b];
  const long long start = clampll(e.y, 0, n);
  const int len = (int)clampll(e.z, 0, n - start);
  const float* p = bufs.p[b] + start;
  const float* g = bufs.g[b] + start;
  double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
  double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0;
  // the bucket bases are 16-byte aligned: peel (4 - start % 4) % 4 elements
  int head = (int)((4 - (start & 3)) & 3);
  head = head < len ? head : len;
  if ((int)threadIdx.x < head) {
    sq_acc(p0, p[threadIdx.x]);
    sq_acc(g0, g[threadIdx.x]);
  }
  const float4* p4 = reinterpret_cast<const float4*>(p + head);
  const float4* g4 = reinterpret_cast<const float4*>(g + head);
  const int n4 = (len - head) >> 2;
#pragma unroll 4
  for (int i = threadIdx.x; i < n4; i += kBlock) {
    const float4 x = p4[i], y = g4[i];
    sq_acc(p0, x.x); sq_acc(p1, x.y); sq_acc(p2, x.z); sq_acc(p3, x.w);
    sq_acc(g0, y.x); sq_acc(g1, y.y); sq_acc(g2, y.z); sq_acc(g3, y.w);
  }
  // tail: fewer than 4 elements
  const int j = head + (n4 << 2) + (int)threadIdx.x;
  if (j < len) {
    sq_acc(p0, p[j]);
    sq_acc(g0, g[j]);
  }
  // block sums in a fixed order: lanes by shuffle, then wave 0..3
  const double wp = wave_reduce_sum_f64((p0 + p1) + (p2 + p3));
  const double wg = wave_reduce_sum_f64((g0 + g1) + (g2 + g3));
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) {
    s_p[wave] = wp;
    s_g[wave] = wg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tp = 0.0, tg = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      tp += s_p[w];
      tg += s_g[w];
    }
    partial[2 * (long long)c] = tp;
    partial[2 * (long long)c + 1] = tg;
  }
}

// One wave per tensor. The lanes load 64 chunk partials at a time, then
// every lane adds them in ascending chunk order (a lane past the end holds
// +0.0, which leaves a sum of squares unchanged): the order depends on the
// chunk table alone. trust in double, rounded to fp32 once.
extern "C" __global__ __launch_bounds__(256) void lars_trust_f32(
    const double* __restrict__ partial, const int2* __restrict__ tensor_chunks,
    const int ntensors, const int nchunks_total, const double coeff,
    const double wd, const double eps, const float grad_scale,
    const float* __restrict__ clip, float* __restrict__ trust) {
  const int lane = threadIdx.x & (kWave - 1);
  const int k = blockIdx.x * kWaves + threadIdx.x / kWave;
  if (k >= ntensors) return;  // wave-uniform
  const int2 tc = tensor_chunks[k];  // {first chunk, chunk count}
  const int first = (int)clampll(tc.x, 0, nchunks_total);
  const int cnt = (int)clampll(tc.y, 0, nchunks_total - first);
  const double2* part2 = reinterpret_cast<const double2*>(partial);
  double sp = 0.0, sg = 0.0;
  // kTrustRounds * 64 partials are in flight before the first add: one
  // load latency per 512 chunks instead of one per 64 (a tensor of 2.36M
  // elements owns 288)
  for (int base = 0; base < cnt; base += kTrustRounds * kWave) {
    double2 x[kTrustRounds];
#pragma unroll
    for (int r = 0; r < kTrustRounds; ++r) {
      const int i = base + r * kWave + lane;
      x[r] = make_double2(0.0, 0.0);
      if (i < cnt) x[r] = part2[first + i];
    }
#pragma unroll
    for (int r = 0; r < kTrustRounds; ++r) {
      const int left = cnt - base - r * kWave;  // wave-uniform
      const int m = left < kWave ? left : kWave;
      for (int l = 0; l < m; ++l) {
        sp += readlane_f64(x[r].x, l);
        sg += readlane_f64(x[r].y, l);
      }
    }
  }
  if (lane != 0) return;
  // the fp32 product the update kernel forms
  const float s = clip_scale(grad_scale, clip);
  const double pn = sqrt(sp);
  const double gn = (double)s * sqrt(sg);
  double t = 1.0;
  if (wd > 0.0 && pn > 0.0 && gn > 0.0) t = coeff * pn / (gn + wd * pn + eps);
  trust[k] = (float)t;
}

extern "C" __global__ void fused_lars_f32(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ v,
    const float* __restrict__ lr_dev, const float lr_host, const float mu,
    const float scale, const long long n, const int* __restrict__ seg_end,
    const float* __restrict__ seg_wd, const int* __restrict__ seg_tensor,
    const int nseg, const float* __restrict__ trust, const int ntensors,
    const float* __restrict__ clip) {
  if (clip_skipped(clip)) return;
  extern __shared__ int s_tab[];  // [nseg] ends, [nseg] decays, [nseg] lr*trust
  int* s_end = s_tab;
  float* s_wd = reinterpret_cast<float*>(s_tab + nseg);
  float* s_lr = reinterpret_cast<float*>(s_tab + 2 * nseg);
  // lr meets the trust ratio HERE, not on the host
  const float lr = load_lr(lr_dev, lr_host);
  for (int k = threadIdx.x; k < nseg; k += blockDim.x) {
    s_end[k] = seg_end[k];
    s_wd[k] = seg_wd[k];
    int t = seg_tensor[k];
    t = t < 0 ? 0 : (t >= ntensors ? ntensors - 1 : t);
    s_lr[k] = lr * trust[t];
  }
  __syncthreads();
  const float s = clip_scale(scale, clip);

  const long long n4 = n >> 2;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* v4 = reinterpret_cast<float4*>(v);
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  int cur = 0;  // segment cursor of find_seg4
  for (; i < n4; i += stride) {
    const float4 pg = g4[i];
    float4 pp = p4[i], pv = v4[i];
    // the binding holds n < 2^31
    const Seg4 q = find_seg4(s_end, cur, nseg, (int)(i << 2));
    lars_elem(s, mu, s_wd[q.q0], s_lr[q.q0], pg.x, pp.x, pv.x);
    lars_elem(s, mu, s_wd[q.q1], s_lr[q.q1], pg.y, pp.y, pv.y);
    lars_elem(s, mu, s_wd[q.q2], s_lr[q.q2], pg.z, pp.z, pv.z);
    lars_elem(s, mu, s_wd[q.q3], s_lr[q.q3], pg.w, pp.w, pv.w);
    v4[i] = pv;
    p4[i] = pp;
  }
  // tail (n % 4)
  for (long long j = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x;
       j < n; j += stride) {
    const int q = find_seg(s_end, 0, nseg, (int)j);
    float pj = p[j], vj = v[j];
    lars_elem(s, mu, s_wd[q], s_lr[q], g[j], pj, vj);
    v[j] = vj;
    p[j] = pj;
  }
}

extern "C" void launch_lars_sumsq_f32(const LarsBufs* bufs, const int* chunks,
                                      int chunk_base, int nchunks,
                                      double* partial, hipStream_t stream) {
  if (nchunks <= 0 || bufs->nbuf <= 0) return;
  hipLaunchKernelGGL(lars_sumsq_f32, dim3(nchunks), dim3(kBlock), 0, stream,
                     *bufs, reinterpret_cast<const int4*>(chunks), chunk_base,
                     partial);
}

extern "C" void launch_lars_trust_f32(const double* partial,
                                      const int* tensor_chunks, int ntensors,
                                      int nchunks_total, double coeff,
                                      double wd, double eps, float grad_scale,
                                      const float* clip, float* trust,
                                      hipStream_t stream) {
  if (ntensors <= 0) return;
  const int grid = (ntensors + kWaves - 1) / kWaves;
  hipLaunchKernelGGL(lars_trust_f32, dim3(grid), dim3(kBlock), 0, stream,
                     partial, reinterpret_cast<const int2*>(tensor_chunks),
                     ntensors, nchunks_total, coeff, wd, eps, grad_scale, clip,
                     trust);
}

extern "C" void launch_fused_lars_f32(
    float* p, const float* g, float* v, const float* lr_dev, float lr,
    float mu, float scale, long long n, const int* seg_end,
    const float* seg_wd, const int* seg_tensor, int nseg, const float* trust,
    int ntensors, const float* clip, hipStream_t stream) {
  const int block = 256;
  const int grid = elementwise_grid((n + 3) / 4, block);
  const size_t lds = (size_t)nseg * (2 * sizeof(int) + sizeof(float));
  hipLaunchKernelGGL(fused_lars_f32, dim3(grid), dim3(block), lds, stream, p,
                     g, v, lr_dev, lr, mu, scale, n, seg_end, seg_wd,
                     seg_tensor, nseg, trust, ntensors, clip);
}
