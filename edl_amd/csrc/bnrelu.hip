// Fused BatchNorm(+residual Add)+ReLU, NHWC bf16, training fwd + bwd.
//
// Replaces the reference's fuse_bn_act_ops / cudnn_batchnorm_spatial_persistent
// knobs (reference train_with_fleet.py:374, train_pretrain.sh:20) — and, on
// MI355X, torch-autocast's fp32 BatchNorm path, which pays TWO full-tensor
// casts (bf16->fp32->bf16: the SubTensorOpWithCast* kernels = ~13% of step
// time in rocprof) plus 5 MIOpen kernels per BN. Here: bf16 reads with fp32
// math, 3 lean kernels fwd / 3 bwd, ReLU and the bottleneck's residual add
// folded in, dgamma/dbeta written straight into fp32 grad bucket views.
//
// Layout: x is NHWC [M rows, C channels], C % 8 == 0; the training kernels
// additionally need C a power of two <= 2048 (all ResNet/ResNeXt widths;
// see row_partition). Each thread owns 8 consecutive channels (one
// ushort4x2 = 16 B load, guide G13); a block's 256 threads cover 2048
// channels' worth of a row-group; blocks grid-stride over rows, fold
// per-channel fp32 partials in LDS and store one partial row per block.
#include <type_traits>

#include "common.h"
#include "launchers.h"

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

// load8 whose 16-byte load stays ONE dwordx4: where the consumer masks
// single elements (the ReLU select in the dx kernels) LLVM narrows the
// vector load back into ushort/dwordx2/dword/ushort pieces despite the
// alignment (seen in the .s of bn_bwd_dx_kernel<RELU>); the empty asm
// makes the four dwords opaque so the load cannot be split.
__device__ __forceinline__ F8 load8_whole(const bf16* p) {
  uint4 raw = *reinterpret_cast<const uint4*>(__builtin_assume_aligned(p, 16));
  asm volatile("" : "+v"(raw.x), "+v"(raw.y), "+v"(raw.z), "+v"(raw.w));
  F8 o;
  const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o.v[2 * i] = __uint_as_float(w[i] << 16);
    o.v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
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

// ---------------- shared phases ----------------
// Each piece below is the single copy of a step that several kernels run.
// Those that stride by the block size take it as `nthr`: the kernels read
// blockDim.x and pass it down, because read inside a device function it
// misses the compiler's uniform-work-group fold (a vector load and a
// select per kernel instead of one scalar load).

// dy_eff: keep g[k] where bit k of the fwd apply's mask byte is set.
__device__ __forceinline__ void relu_select(F8& g, const unsigned mb) {
#pragma unroll
  for (int k = 0; k < 8; ++k) g.v[k] = (mb >> k) & 1 ? g.v[k] : 0.0f;
}

// Flat octet index over [rows, C/8] -> (channel octet, row). Every model
// width is pow2: % and / as mask and shift (the generic 64-bit divmod
// lowers to a ~100-instruction sequence per octet).
struct OctSplit {
  int c8, m8;  // octets per row; c8 - 1, the pow2 mask
  bool p2;
  int c8l;     // log2(c8) when p2
  __device__ __forceinline__ explicit OctSplit(const int C) {
    c8 = C >> 3;
    m8 = c8 - 1;
    p2 = (c8 & m8) == 0;
    c8l = 31 - __clz((unsigned)c8);
  }
  __device__ __forceinline__ int oct(const long long i) const {
    return p2 ? (int)(i & m8) : (int)(i % c8);
  }
  __device__ __forceinline__ long long row(const long long i) const {
    return p2 ? (i >> c8l) : (i / c8);
  }
};

// 16-byte zero store: one halo octet of a padded buffer.
__device__ __forceinline__ void zero8(bf16* p) {
  *reinterpret_cast<uint4*>(__builtin_assume_aligned(p, 16)) =
      uint4{0, 0, 0, 0};
}

// Row partition of the per-channel reductions: thread -> (channel octet,
// first row); the whole grid strides the tensor by rstride rows.
// PRECONDITION: C/8 divides the 256-thread block, i.e. C is a power of two
// in 8..2048 — only then does the octet taken from threadIdx agree with
// the row taken from the global thread id, and every (row, octet) pair is
// visited exactly once. check_bn_inputs (module.cpp) enforces it and
// BNReLU2d._use_fused routes other widths to the torch fallback.
struct RowPart {
  long long row0, rstride;
  int lane_c, c0;  // channel octet and its first channel
};

__device__ __forceinline__ RowPart row_partition(const int C,
                                                 const unsigned nthr) {
  const int tpr = C >> 3;  // threads per row (each owns 8 channels)
  const int tid = blockIdx.x * nthr + threadIdx.x;
  RowPart p;
  p.row0 = tid / tpr;
  p.rstride = ((long long)gridDim.x * nthr) / tpr;
  p.lane_c = (int)(threadIdx.x % tpr);
  p.c0 = p.lane_c * 8;
  return p;
}

// Block fold, two-stage and free of global atomics (single-stage atomics
// measured 17-40 us/dispatch fixed cost: same-word serialization at ~88
// adds/us for small C, grid x 2C traffic for large C): fold_begin zeroes
// the block's LDS row before the row loop; fold_end LDS-reduces every
// thread's two 8-channel accumulators and STORES the block's [2C] row of
// partial[grid][2C]. The finalize kernels reduce over blocks.
__device__ __forceinline__ void fold_begin(float* lsum, const int C,
                                           const unsigned nthr) {
  for (int i = threadIdx.x; i < 2 * C; i += nthr) lsum[i] = 0.0f;
  __syncthreads();
}

__device__ __forceinline__ void fold_end(float* lsum, const float (&a)[8],
                                         const float (&b)[8], const int c0,
                                         const int C, const unsigned nthr,
                                         float* __restrict__ partial) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    atomicAdd(&lsum[c0 + i], a[i]);
    atomicAdd(&lsum[C + c0 + i], b[i]);
  }
  __syncthreads();
  float* out = partial + (long long)blockIdx.x * 2 * C;
  for (int i = threadIdx.x; i < 2 * C; i += nthr) out[i] = lsum[i];
}

// ---------------- forward ----------------

// K1: per-channel sum and sum-of-squares PARTIALS (training stats).
__global__ void bn_stats_kernel(
    const bf16* __restrict__ x, float* __restrict__ partial,  // [grid, 2C]
    const long long M, const int C) {
  __shared__ float lsum[2 * 2048];
  const RowPart p = row_partition(C, blockDim.x);
  const long long rstride = p.rstride;
  const int c0 = p.c0;
  fold_begin(lsum, C, blockDim.x);

  float s[8] = {0}, q[8] = {0};
  long long r = p.row0;
  // 4 independent row streams: the grid is capped (finalize reads the
  // partials serially), so per-thread in-flight bytes must cover HBM
  // latency — 1 stream measured ~1.2 TB/s, latency-bound
  for (; r + 3 * rstride < M; r += 4 * rstride) {
    F8 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = load8(x + (r + u * rstride) * C + c0);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        s[i] += v[u].v[i];
        q[i] = fmaf(v[u].v[i], v[u].v[i], q[i]);
      }
    }
  }
  for (; r < M; r += rstride) {
    F8 v = load8(x + r * C + c0);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      s[i] += v.v[i];
      q[i] = fmaf(v.v[i], v.v[i], q[i]);
    }
  }
  fold_end(lsum, s, q, c0, C, blockDim.x, partial);
}

// K2: strip-parallel fwd finalize — reduce the partials over blocks,
// finalize mean/invstd/scale/shift, update the running stats. 256 threads
// = 64 channels x 4 strips over the block range (one thread per channel
// ran a single wave at C=64, serially reading every partial:
// latency-bound).
extern "C" __global__ void bn_finalize_kernel(
    float* __restrict__ partial, const int nblocks, const int zero_src,
    const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ mean_out,
    float* __restrict__ invstd_out, float* __restrict__ scale_out,
    float* __restrict__ shift_out, float* __restrict__ running_mean,
    float* __restrict__ running_var, const float momentum, const float eps,
    const long long M, const int C) {
  __shared__ float accs[4][64];
  __shared__ float accq[4][64];
  const int lane = threadIdx.x & 63;
  const int strip = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const long long st = 2 * C;
  float sa[4] = {0}, qa[4] = {0};
  if (c < C) {
    int b = strip;
    for (; b + 12 < nblocks; b += 16) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long i0 = (long long)(b + 4 * u) * st + c;
        sa[u] += partial[i0];
        qa[u] += partial[i0 + C];
        if (zero_src) { partial[i0] = 0.0f; partial[i0 + C] = 0.0f; }
      }
    }
    for (; b < nblocks; b += 4) {
      const long long i0 = (long long)b * st + c;
      sa[0] += partial[i0];
      qa[0] += partial[i0 + C];
      if (zero_src) { partial[i0] = 0.0f; partial[i0 + C] = 0.0f; }
    }
  }
  accs[strip][lane] = (sa[0] + sa[1]) + (sa[2] + sa[3]);
  accq[strip][lane] = (qa[0] + qa[1]) + (qa[2] + qa[3]);
  __syncthreads();
  if (strip != 0 || c >= C) return;
  const float s = (accs[0][lane] + accs[1][lane]) +
                  (accs[2][lane] + accs[3][lane]);
  const float q = (accq[0][lane] + accq[1][lane]) +
                  (accq[2][lane] + accq[3][lane]);
  const float inv_m = 1.0f / (float)M;
  const float mean = s * inv_m;
  const float var = fmaxf(q * inv_m - mean * mean, 0.0f);
  const float invstd = rsqrtf(var + eps);
  mean_out[c] = mean;
  invstd_out[c] = invstd;
  const float g = gamma[c];
  scale_out[c] = g * invstd;
  shift_out[c] = beta[c] - g * invstd * mean;
  if (running_mean != nullptr) {
    // unbiased variance for the running estimate (torch semantics)
    const float ub = (M > 1) ? var * (float)M / (float)(M - 1) : var;
    running_mean[c] = fmaf(momentum, mean - running_mean[c], running_mean[c]);
    running_var[c] = fmaf(momentum, ub - running_var[c], running_var[c]);
  }
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

// K3: y = relu?(x*scale + shift [+ res]); NHWC vectorized by channel octets.
// MASK (with RELU only): also emit a 1-bit-per-channel ReLU mask (one byte
// per octet) so the backward kernels never re-read y (16x fewer bytes on
// that stream).
template <bool RELU, bool ADD, bool MASK>
__global__ void bn_apply_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ res,
    bf16* __restrict__ y, unsigned char* __restrict__ mask,
    const float* __restrict__ scale,
    const float* __restrict__ shift, const long long M, const int C) {
  static_assert(RELU || !MASK, "the mask is the ReLU mask");
  const OctSplit os(C);
  const long long total = M * os.c8;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int c0 = os.oct(i) * 8;
    const long long eoff = os.row(i) * C + c0;
    F8 v = load8(x + eoff);
    const unsigned char mb = apply_octet<RELU, ADD>(
        v, ADD ? res + eoff : nullptr, scale, shift, c0);
    if (MASK) mask[i] = mb;
    store8(y + eoff, v);
  }
}

// Padded-layout addressing shared by the *_pad kernels below: flat octet
// index j over [N, Hp, Wp, C/8] -> destination pixel `pix` and, for
// interior pixels, the unpadded row. pix < 2^31 (host-checked), so the
// Wp/Hp splits are 32-bit unsigned divides.
struct PadIdx {
  int oct;
  unsigned pix;
  long long row;  // unpadded NHWC row, or -1 on the halo
};

__device__ __forceinline__ PadIdx pad_index(const long long j,
                                            const OctSplit& os, const int H,
                                            const int W) {
  PadIdx o;
  o.oct = os.oct(j);
  o.pix = (unsigned)os.row(j);
  const unsigned Wp = (unsigned)W + 2u, Hp = (unsigned)H + 2u;
  const unsigned t = o.pix / Wp;
  const unsigned w = o.pix - t * Wp - 1u;  // wraps to huge on the halo
  const unsigned n = t / Hp;
  const unsigned h = t - n * Hp - 1u;
  o.row = (h < (unsigned)H && w < (unsigned)W)
              ? ((long long)n * H + h) * W + w
              : -1;
  return o;
}

// K3p: bn_apply (ReLU + mask, no residual) that writes y straight into the
// zero-halo padded layout [N, H+2, W+2, C] the implicit-GEMM 3x3 kernels
// read — the following conv skips its pad_nhwc pass. Iterates the PADDED
// index space: interior octets get the normal value and mask byte (mask
// stays indexed by the unpadded octet), halo octets get zeros. The halo is
// rewritten on every launch, so uninitialised storage and hipGraph replay
// are both safe.
__global__ void bn_apply_pad_kernel(
    const bf16* __restrict__ x, bf16* __restrict__ yp,
    unsigned char* __restrict__ mask, const float* __restrict__ scale,
    const float* __restrict__ shift, const int Nimg, const int H, const int W,
    const int C) {
  const OctSplit os(C);
  const long long total = (long long)Nimg * (H + 2) * (W + 2) * os.c8;
  long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (; j < total; j += stride) {
    const PadIdx p = pad_index(j, os, H, W);
    const int c0 = p.oct * 8;
    bf16* dst = yp + (long long)p.pix * C + c0;
    if (p.row < 0) {
      zero8(dst);
      continue;
    }
    F8 v = load8(x + p.row * C + c0);
    mask[p.row * os.c8 + p.oct] =
        apply_octet<true, false>(v, nullptr, scale, shift, c0);
    store8(dst, v);
  }
}

// ---------------- backward ----------------

// Row loop of the backward reduce: this thread's s1 += dy_eff and
// s2 += dy_eff * xhat over its rows of the partition, where dy_eff applies
// the fused ReLU mask (bitmask from the fwd apply). 4 row streams x 3
// tensors = up to 12 outstanding 16-B loads per thread for latency hiding
// at the capped grids, then a one-row tail.
template <bool RELU>
__device__ __forceinline__ void bwd_reduce_rows(
    const bf16* __restrict__ dy, const unsigned char* __restrict__ mask,
    const bf16* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const RowPart& p, const long long M,
    const int C, float (&s1)[8], float (&s2)[8]) {
  const int c8 = C >> 3;
  const long long rstride = p.rstride;
  const int lane_c = p.lane_c, c0 = p.c0;
  float mu[8], is[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    mu[i] = mean[c0 + i];
    is[i] = invstd[c0 + i];
  }
  long long r = p.row0;
  for (; r + 3 * rstride < M; r += 4 * rstride) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const long long r0 = r + 2 * u * rstride, r1 = r + (2 * u + 1) * rstride;
      const long long e0 = r0 * C + c0, e1 = r1 * C + c0;
      F8 g0 = load8(dy + e0), g1 = load8(dy + e1);
      F8 x0 = load8(x + e0), x1 = load8(x + e1);
      if (RELU) {
        const unsigned m0 = mask[r0 * c8 + lane_c];
        const unsigned m1 = mask[r1 * c8 + lane_c];
        relu_select(g0, m0);
        relu_select(g1, m1);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        s1[i] += g0.v[i] + g1.v[i];
        s2[i] = fmaf(g0.v[i], (x0.v[i] - mu[i]) * is[i],
                     fmaf(g1.v[i], (x1.v[i] - mu[i]) * is[i], s2[i]));
      }
    }
  }
  for (; r < M; r += rstride) {
    const long long eoff = r * C + c0;
    F8 g = load8(dy + eoff);
    F8 xv = load8(x + eoff);
    if (RELU) relu_select(g, mask[r * c8 + lane_c]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      s1[i] += g.v[i];
      s2[i] = fmaf(g.v[i], (xv.v[i] - mu[i]) * is[i], s2[i]);
    }
  }
}

// B1: per-channel PARTIALS of s1 = sum(dy_eff), s2 = sum(dy_eff * xhat).
template <bool RELU>
__global__ void bn_bwd_reduce_kernel(
    const bf16* __restrict__ dy, const unsigned char* __restrict__ mask,
    const bf16* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, float* __restrict__ partial,  // [grid, 2C]
    const long long M, const int C) {
  __shared__ float lsum[2 * 2048];
  const RowPart p = row_partition(C, blockDim.x);
  fold_begin(lsum, C, blockDim.x);
  float s1[8] = {0}, s2[8] = {0};
  bwd_reduce_rows<RELU>(dy, mask, x, mean, invstd, p, M, C, s1, s2);
  fold_end(lsum, s1, s2, p.c0, C, blockDim.x, partial);
}

// B1b: strip-parallel reduction of the bwd partials over blocks ->
// sums[2C] (= [dbeta; dgamma]). 256 threads = 64 channel indices x 4
// strips over the block range (one thread per index ran only 2C threads
// total: HALF A WAVE at C=64 doing the whole latency-bound serial partial
// read).
// db_acc/dg_acc: optional direct-grad targets (the param's bucket-view
// gradient) — accumulating here removes the per-param AccumulateGrad
// add kernels at world 1 (~106 tiny launches/step across ResNet50's
// BN layers). Single writer per channel, so a plain += suffices.
extern "C" __global__ void bn_bwd_finalize_kernel(
    const float* __restrict__ partial, const int nblocks,
    float* __restrict__ sums, const int C, float* __restrict__ db_acc,
    float* __restrict__ dg_acc) {
  __shared__ float acc[4][64];
  const int lane = threadIdx.x & 63;
  const int strip = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  const long long st = 2 * C;
  float sa[8] = {0};
  if (i < 2 * C) {
    int b = strip;
    for (; b + 28 < nblocks; b += 32) {
#pragma unroll
      for (int u = 0; u < 8; ++u)
        sa[u] += partial[(long long)(b + 4 * u) * st + i];
    }
    for (; b < nblocks; b += 4) sa[0] += partial[(long long)b * st + i];
  }
  acc[strip][lane] = ((sa[0] + sa[1]) + (sa[2] + sa[3])) +
                     ((sa[4] + sa[5]) + (sa[6] + sa[7]));
  __syncthreads();
  if (strip == 0 && i < 2 * C) {
    const float v = (acc[0][lane] + acc[1][lane]) +
                    (acc[2][lane] + acc[3][lane]);
    sums[i] = v;
    if (i < C) {
      if (db_acc) db_acc[i] += v;
    } else if (dg_acc) {
      dg_acc[i - C] += v;
    }
  }
}

// (no separate dgamma/dbeta kernel: the bwd-reduce workspace IS [dbeta; dgamma]
// — sums[0:C] = s1 = dbeta, sums[C:2C] = s2 = dgamma; Python returns views.)

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

// B3: dx (+ dres) as its own launch.
template <bool RELU, bool ADD, bool TRAINING>
__global__ void bn_bwd_dx_kernel(
    const bf16* __restrict__ dy, const unsigned char* __restrict__ mask,
    const bf16* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ sums, bf16* __restrict__ dx,
    bf16* __restrict__ dres, const long long M, const int C) {
  const OctSplit os(C);
  const long long total = M * os.c8;
  const float inv_m = 1.0f / (float)M;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int c0 = os.oct(i) * 8;
    const long long eoff = os.row(i) * C + c0;
    F8 g = load8(dy + eoff);
    if (RELU) relu_select(g, mask[i]);
    if (ADD) store8(dres + eoff, g);
    const F8 xv = load8(x + eoff);
    store8(dx + eoff, dx_octet<TRAINING>(g, xv, mean, invstd, gamma, sums,
                                         inv_m, c0, C));
  }
}

// B3p: bn_bwd_dx (training, no residual) storing dx into the zero-halo
// padded layout [N, H+2, W+2, C]: the producing conv's dgrad and wgrad
// read it in place of a pad_nhwc copy. Same per-element math as
// bn_bwd_dx_kernel; halo written on every launch (see bn_apply_pad_kernel).
template <bool RELU>
__global__ void bn_bwd_dx_pad_kernel(
    const bf16* __restrict__ dy, const unsigned char* __restrict__ mask,
    const bf16* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ sums, bf16* __restrict__ dxp, const int Nimg,
    const int H, const int W, const int C) {
  const OctSplit os(C);
  const long long total = (long long)Nimg * (H + 2) * (W + 2) * os.c8;
  const float inv_m = 1.0f / (float)((long long)Nimg * H * W);
  long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (; j < total; j += stride) {
    const PadIdx p = pad_index(j, os, H, W);
    const int c0 = p.oct * 8;
    bf16* dst = dxp + (long long)p.pix * C + c0;
    if (p.row < 0) {
      zero8(dst);
      continue;
    }
    const long long eoff = p.row * C + c0;
    F8 g = load8_whole(dy + eoff);
    if (RELU) relu_select(g, mask[p.row * os.c8 + p.oct]);
    const F8 xv = load8(x + eoff);
    store8(dst, dx_octet<true>(g, xv, mean, invstd, gamma, sums, inv_m, c0, C));
  }
}

// B-fused: reduce + finalize + dx in ONE launch (EDL_BN_BWD_FUSED).
// The three-kernel backward pays two launch/drain boundaries per BN layer
// (53 layers in resnet50_vd). Here the grid rendezvouses in device memory:
// every block writes its partial row and bumps an arrival counter; the
// first F blocks wait for full arrival, then finalize a channel SLICE each
// (parallel finalize — a single finalizer block measured 45+ us on 512
// partial rows) and bump a done counter; everyone spins RELAXED (an
// acquire per poll invalidates L2 every iteration — measured as an ~85 us
// rendezvous storm) with ONE acquire fence on exit. grid <= 512 with
// __launch_bounds__(256, 2) guarantees co-residency on 256 CUs (the spin
// cannot deadlock); all spins are iteration-bounded regardless. ws = a
// persistent int[4] {arrive, done, depart, pad}: the last block OUT
// resets it, so hipGraph replays and back-to-back layers need no host
// zeroing.
template <bool RELU, bool ADD>
__global__ __launch_bounds__(256, 2) void bn_bwd_fused_kernel(
    const bf16* __restrict__ dy, const unsigned char* __restrict__ mask,
    const bf16* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    float* __restrict__ partial, float* __restrict__ sums,
    float* __restrict__ db_acc, float* __restrict__ dg_acc,
    bf16* __restrict__ dx, bf16* __restrict__ dres, int* __restrict__ ws,
    const int nfin, const long long M, const int C) {
  // ---- phase 1: per-block channel reduction (bn_bwd_reduce) ----
  {
    __shared__ float lsum[2 * 2048];
    const RowPart p = row_partition(C, blockDim.x);
    fold_begin(lsum, C, blockDim.x);
    float s1[8] = {0}, s2[8] = {0};
    bwd_reduce_rows<RELU>(dy, mask, x, mean, invstd, p, M, C, s1, s2);
    fold_end(lsum, s1, s2, p.c0, C, blockDim.x, partial);
  }

  // ---- rendezvous ----
  __threadfence();
  if (threadIdx.x == 0)
    __hip_atomic_fetch_add(&ws[0], 1, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_AGENT);
  const int g = gridDim.x;
  if ((int)blockIdx.x < nfin) {
    // finalizer: wait for all partials, then reduce a channel slice
    if (threadIdx.x == 0) {
      for (long long it = 0; it < 50000000LL; ++it) {
        if (__hip_atomic_load(&ws[0], __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) == g)
          break;
        __builtin_amdgcn_s_sleep(2);
      }
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const long long st = 2 * C;
    const int i0 = blockIdx.x * 2 * C / nfin;
    const int i1 = (blockIdx.x + 1) * 2 * C / nfin;
    for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
      float sa[4] = {0, 0, 0, 0};
      int b = 0;
      for (; b + 4 <= g; b += 4)
#pragma unroll
        for (int u = 0; u < 4; ++u)
          sa[u] += partial[(long long)(b + u) * st + i];
      for (; b < g; ++b) sa[0] += partial[(long long)b * st + i];
      const float v = (sa[0] + sa[1]) + (sa[2] + sa[3]);
      sums[i] = v;
      if (i < C) {
        if (db_acc) db_acc[i] += v;
      } else if (dg_acc) {
        dg_acc[i - C] += v;
      }
    }
    __syncthreads();
    __threadfence();
    if (threadIdx.x == 0)
      __hip_atomic_fetch_add(&ws[1], 1, __ATOMIC_RELEASE,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
  // everyone: wait for all slices, one acquire fence on exit
  if (threadIdx.x == 0) {
    for (long long it = 0; it < 50000000LL; ++it) {
      if (__hip_atomic_load(&ws[1], __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_AGENT) == nfin)
        break;
      __builtin_amdgcn_s_sleep(2);
    }
    const int depart = __hip_atomic_fetch_add(&ws[2], 1, __ATOMIC_ACQ_REL,
                                              __HIP_MEMORY_SCOPE_AGENT);
    if (depart == g - 1) {  // everyone passed both waits: reset
      __hip_atomic_store(&ws[0], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&ws[1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&ws[2], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

  // ---- phase 2: dx (+dres), training form (bn_bwd_dx) ----
  const OctSplit os(C);
  const long long total = M * os.c8;
  const float inv_m = 1.0f / (float)M;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int c0 = os.oct(i) * 8;
    const long long eoff = os.row(i) * C + c0;
    F8 g2 = load8(dy + eoff);
    if (RELU) relu_select(g2, mask[i]);
    if (ADD) store8(dres + eoff, g2);
    const F8 xv = load8(x + eoff);
    store8(dx + eoff,
           dx_octet<true>(g2, xv, mean, invstd, gamma, sums, inv_m, c0, C));
  }
}

// ---------------- launchers ----------------

static long long env_ll(const char* name, long long dflt) {
  const char* e = getenv(name);
  return e ? atoll(e) : dflt;
}

static int bn_grid_common(long long M, int C, long long cap_env) {
  const int c8 = C >> 3;
  long long rows_per_block = 256 / c8 > 0 ? 256 / c8 : 1;
  long long want = (M + rows_per_block - 1) / rows_per_block;
  long long cap = 131072 / (2 * (long long)C);
  if (cap > cap_env) cap = cap_env;
  if (cap < 8) cap = 8;
  long long g = want < cap ? want : cap;
  return (int)(g > 0 ? g : 1);
}

extern "C" int bn_stats_grid(long long M, int C) {
  // cover the tensor with enough blocks for bandwidth, but keep the
  // partial buffer (grid x 2C fp32) around <= 1 MiB.
  // cap bounds the finalize kernels' serial partial-read loop (they were
  // latency-bound at ~12-14 us with 512-block partials; ~5 us at 192).
  // EDL_BN_GRID_CAP overrides for A/B (192 = measured best tradeoff).
  return bn_grid_common(M, C, env_ll("EDL_BN_GRID_CAP", 192));
}

extern "C" int bn_bwd_grid(long long M, int C) {
  // the BWD reduce grid is decoupled from the fwd one: with the
  // strip-parallel finalize the partial-read cost no longer binds the
  // grid, so the reduce can run wider for bandwidth.
  return bn_grid_common(M, C,
                        env_ll("EDL_BN_BWD_GRID_CAP",
                               env_ll("EDL_BN_GRID_CAP", 192)));
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

extern "C" void launch_bn_stats(const void* x, float* partial, int grid,
                                long long M, int C, hipStream_t s) {
  hipLaunchKernelGGL(bn_stats_kernel, dim3(grid), dim3(256), 0, s,
                     (const bf16*)x, partial, M, C);
}

extern "C" void launch_bn_finalize(float* partial, int nblocks, int zero_src,
                                   const float* gamma,
                                   const float* beta, float* mean, float* invstd,
                                   float* scale, float* shift, float* rmean,
                                   float* rvar, float momentum, float eps,
                                   long long M, int C, hipStream_t s) {
  // zero_src: store 0 back after each read — returns a pooled pre_part
  // buffer to the pool clean, killing the per-step FillFunctor launches
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 63) / 64), dim3(256), 0, s,
                     partial, nblocks, zero_src, gamma, beta, mean, invstd,
                     scale, shift, rmean, rvar, momentum, eps, M, C);
}

extern "C" void launch_bn_bwd_finalize(const float* partial, int nblocks,
                                       float* sums, int C, float* db_acc,
                                       float* dg_acc, hipStream_t s) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((2 * C + 63) / 64),
                     dim3(256), 0, s, partial, nblocks, sums, C, db_acc,
                     dg_acc);
}

extern "C" void launch_bn_apply(const void* x, const void* res, void* y,
                                unsigned char* mask,
                                const float* scale, const float* shift,
                                long long M, int C, bool relu, bool add,
                                hipStream_t s) {
  const long long total = M * (C >> 3);
  const int grid = elementwise_grid(total, 256);
  dispatch_bools(
      [&](auto R, auto A, auto Mk) {
        constexpr bool RELU = decltype(R)::value, ADD = decltype(A)::value;
        // the mask is the ReLU mask: no <RELU=false, MASK=true> variants
        constexpr bool MASK = RELU && decltype(Mk)::value;
        hipLaunchKernelGGL((bn_apply_kernel<RELU, ADD, MASK>), dim3(grid),
                           dim3(256), 0, s, (const bf16*)x,
                           ADD ? (const bf16*)res : nullptr, (bf16*)y,
                           MASK ? mask : nullptr, scale, shift, M, C);
      },
      relu, add, mask != nullptr);
}

extern "C" void launch_bn_bwd_reduce(const void* dy, const unsigned char* mask,
                                     const void* x,
                                     const float* mean, const float* invstd,
                                     float* partial, int grid, long long M, int C,
                                     bool relu, hipStream_t s) {
  dispatch_bools(
      [&](auto R) {
        constexpr bool RELU = decltype(R)::value;
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<RELU>), dim3(grid), dim3(256),
                           0, s, (const bf16*)dy, RELU ? mask : nullptr,
                           (const bf16*)x, mean, invstd, partial, M, C);
      },
      relu);
}

extern "C" void launch_bn_bwd_dx(const void* dy, const unsigned char* mask,
                                 const void* x,
                                 const float* mean, const float* invstd,
                                 const float* gamma, const float* sums, void* dx,
                                 void* dres, long long M, int C, bool relu,
                                 bool add, bool training, hipStream_t s) {
  const long long total = M * (C >> 3);
  const int grid = elementwise_grid(total, 256);
  dispatch_bools(
      [&](auto R, auto A, auto T) {
        hipLaunchKernelGGL((bn_bwd_dx_kernel<decltype(R)::value,
                                             decltype(A)::value,
                                             decltype(T)::value>),
                           dim3(grid), dim3(256), 0, s, (const bf16*)dy, mask,
                           (const bf16*)x, mean, invstd, gamma, sums,
                           (bf16*)dx, (bf16*)dres, M, C);
      },
      relu, add, training);
}

extern "C" void launch_bn_apply_pad(const void* x, void* yp,
                                    unsigned char* mask, const float* scale,
                                    const float* shift, int Nimg, int H, int W,
                                    int C, hipStream_t s) {
  const long long total = (long long)Nimg * (H + 2) * (W + 2) * (C >> 3);
  const int grid = elementwise_grid(total, 256);
  hipLaunchKernelGGL(bn_apply_pad_kernel, dim3(grid), dim3(256), 0, s,
                     (const bf16*)x, (bf16*)yp, mask, scale, shift, Nimg, H, W,
                     C);
}

extern "C" void launch_bn_bwd_dx_pad(const void* dy, const unsigned char* mask,
                                     const void* x, const float* mean,
                                     const float* invstd, const float* gamma,
                                     const float* sums, void* dxp, int Nimg,
                                     int H, int W, int C, bool relu,
                                     hipStream_t s) {
  const long long total = (long long)Nimg * (H + 2) * (W + 2) * (C >> 3);
  const int grid = elementwise_grid(total, 256);
  dispatch_bools(
      [&](auto R) {
        constexpr bool RELU = decltype(R)::value;
        hipLaunchKernelGGL((bn_bwd_dx_pad_kernel<RELU>), dim3(grid), dim3(256),
                           0, s, (const bf16*)dy, RELU ? mask : nullptr,
                           (const bf16*)x, mean, invstd, gamma, sums,
                           (bf16*)dxp, Nimg, H, W, C);
      },
      relu);
}

extern "C" void launch_bn_bwd_fused(const void* dy, const unsigned char* mask,
                                    const void* x, const float* mean,
                                    const float* invstd, const float* gamma,
                                    float* partial, float* sums, float* db_acc,
                                    float* dg_acc, void* dx, void* dres,
                                    int* ws, int grid, int nfin, long long M,
                                    int C, bool relu, bool add, hipStream_t s) {
  dispatch_bools(
      [&](auto R, auto A) {
        constexpr bool RELU = decltype(R)::value;
        hipLaunchKernelGGL((bn_bwd_fused_kernel<RELU, decltype(A)::value>),
                           dim3(grid), dim3(256), 0, s, (const bf16*)dy,
                           RELU ? mask : nullptr, (const bf16*)x, mean, invstd,
                           gamma, partial, sums, db_acc, dg_acc, (bf16*)dx,
                           (bf16*)dres, ws, nfin, M, C);
      },
      relu, add);
}
