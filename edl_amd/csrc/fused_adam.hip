// Fused Adam / AdamW over a flat parameter bucket (fp32).
//
// One launch updates an entire bucket in place: p, m (exp_avg), v
// (exp_avg_sq), read-only g — the same flat buffers fused_sgd.hip walks
// (edl_amd/train/bucketed_ddp.py), with the data-parallel gradient average
// and the fp16 loss-scale inverse folded in as `scale`. Replaces the
// reference's per-parameter Paddle Adam ops (example/ctr/ctr/train.py:234,
// example/distill/nlp/model.py:35-51).
//
//   g' = scale*g            (+ wd*p in L2 mode)
//   p *= 1 - lr*wd          (decoupled mode, before the update)
//   m  = b1*m + (1-b1)*g'
//   v  = b2*v + (1-b2)*g'^2
//   p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps),   bc_i = 1 - b_i^t
//
// Memory-bound: 4 reads + 3 writes of 4 B per element; float4-vectorized
// (16 B/lane, guide Guideline 13), grid-stride, scalar tail for n % 4.
//
// Everything that changes between steps is read from device memory: lr
// (lr_dev, host fallback when null) and the step count t (step_dev, int32).
// The bias corrections are computed HERE from t: a captured hipGraph
// replays with its capture-time host arguments, so host-computed
// corrections would freeze at the capture step.
//
// omb1/omb2 = 1-b1, 1-b2 and ln_b1/ln_b2 = ln b1, ln b2 arrive computed in
// double on the host: 1.0f - 0.999f is off by ~6e-5 relative (it would
// poison v), and bc = -expm1f(t*ln b) does not cancel at small t the way
// 1 - powf(b, t) does.
//
// Per-segment weight decay (biases / norm scales excluded from decay) stays
// one launch: seg_end[nseg] (cumulative element ends, last == n) and
// seg_wd[nseg] are copied to LDS once per block (8 B per segment, at most
// kAdamMaxSegments) and looked up per element (flat_update.h). nseg == 0
// (null tables) = uniform wd, no LDS, no lookup.
#include "flat_update.h"
#include "launchers.h"

namespace {

struct AdamCoef {
  float lr, b1, b2, omb1, omb2, eps, scale, step_size, sqrt_bc2;
  bool decoupled;
};

__device__ __forceinline__ void adam_elem(const AdamCoef& c, const float wd,
                                          const float g, float& p, float& m,
                                          float& v) {
  float gs = c.scale * g;
  if (c.decoupled)
    p *= 1.0f - c.lr * wd;
  else
    gs = fmaf(wd, p, gs);
  m = fmaf(c.b1, m, c.omb1 * gs);
  v = fmaf(c.b2, v, (c.omb2 * gs) * gs);
  const float denom = sqrtf(v) / c.sqrt_bc2 + c.eps;
  p = fmaf(-c.step_size, m / denom, p);
}

}  // namespace

extern "C" __global__ void fused_adam_f32(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, const int* __restrict__ step_dev,
    const float* __restrict__ lr_dev, const float lr_host, const float b1,
    const float b2, const float omb1, const float omb2, const float ln_b1,
    const float ln_b2, const float eps, const float wd, const float scale,
    const int decoupled, const long long n, const int* __restrict__ seg_end,
    const float* __restrict__ seg_wd, const int nseg,
    const float* __restrict__ clip) {
  if (clip_skipped(clip)) return;
  extern __shared__ int s_tab[];  // [nseg] ends, then [nseg] decays
  int* s_end = s_tab;
  float* s_wd = reinterpret_cast<float*>(s_tab + nseg);
  if (nseg > 0) {
    for (int k = threadIdx.x; k < nseg; k += blockDim.x) {
      s_end[k] = seg_end[k];
      s_wd[k] = seg_wd[k];
    }
    __syncthreads();
  }

  // one broadcast load each, L2-resident
  AdamCoef c;
  c.lr = load_lr(lr_dev, lr_host);
  const int t = *step_dev;
  const float tf = (float)(t > 1 ? t : 1);
  c.b1 = b1; c.b2 = b2; c.omb1 = omb1; c.omb2 = omb2;
  c.eps = eps; c.scale = clip_scale(scale, clip);
  c.decoupled = decoupled != 0;
  c.step_size = c.lr / -expm1f(tf * ln_b1);
  c.sqrt_bc2 = sqrtf(-expm1f(tf * ln_b2));

  const long long n4 = n >> 2;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  int cur = 0;  // segment cursor of find_seg4
  for (; i < n4; i += stride) {
    float4 pg = g4[i], pp = p4[i], pm = m4[i], pv = v4[i];
    float w0 = wd, w1 = wd, w2 = wd, w3 = wd;
    if (nseg > 0) {
      // the binding holds n < 2^31 here
      const Seg4 q = find_seg4(s_end, cur, nseg, (int)(i << 2));
      w0 = s_wd[q.q0];
      w1 = s_wd[q.q1];
      w2 = s_wd[q.q2];
      w3 = s_wd[q.q3];
    }
    adam_elem(c, w0, pg.x, pp.x, pm.x, pv.x);
    adam_elem(c, w1, pg.y, pp.y, pm.y, pv.y);
    adam_elem(c, w2, pg.z, pp.z, pm.z, pv.z);
    adam_elem(c, w3, pg.w, pp.w, pm.w, pv.w);
    m4[i] = pm;
    v4[i] = pv;
    p4[i] = pp;
  }
  // tail (n % 4)
  for (long long j = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x;
       j < n; j += stride) {
    float w = wd;
    if (nseg > 0) w = s_wd[find_seg(s_end, 0, nseg, (int)j)];
    float pj = p[j], mj = m[j], vj = v[j];
    adam_elem(c, w, g[j], pj, mj, vj);
    m[j] = mj;
    v[j] = vj;
    p[j] = pj;
  }
}

extern "C" void launch_fused_adam_f32(
    float* p, const float* g, float* m, float* v, const int* step_dev,
    const float* lr_dev, float lr, float b1, float b2, float omb1, float omb2,
    float ln_b1, float ln_b2, float eps, float wd, float scale, int decoupled,
    long long n, const int* seg_end, const float* seg_wd, int nseg,
    const float* clip, hipStream_t stream) {
  const int block = 256;
  const int grid = elementwise_grid((n + 3) / 4, block);
  const size_t lds = (size_t)nseg * (sizeof(int) + sizeof(float));
  hipLaunchKernelGGL(fused_adam_f32, dim3(grid), dim3(block), lds, stream, p,
                     g, m, v, step_dev, lr_dev, lr, b1, b2, omb1, omb2, ln_b1,
                     ln_b2, eps, wd, scale, decoupled, n, seg_end, seg_wd,
                     nseg, clip);
}
