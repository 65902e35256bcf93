// The classifier head on CDNA4: global average pool + FC, forward and
// backward, bf16 with fp32 accumulation on v_mfma_f32_16x16x32_bf16.
//
//   x [N, HW, C] (channels_last rows), W [K, C] (K classes), bias fp32 [K]
//   fwd:  pooled[n,c] = bf16(sum_hw x / HW)          head_pool_kernel
//         logits[n,k] = bf16(pooled . W[k] + bias)   head_fc_kernel
//   bwd:  dx[n,hw,c]  = bf16((dl . W[:,c]) / HW)     head_dx_kernel
//         dW[k,c] (+)= sum_n dl[n,k] pooled[n,c]     head_dw_kernel
//         db[k]   (+)= sum_n dl[n,k]                 (same launch)
//
// None of the GEMM kernels fits: the batch is 16-32 rows against their
// 128/256-row M tiles, K = 1000 is no multiple of 64, and the dW reduction
// is 32 long where gemm_tn expects ~1e5. All three products here are
// SKINNY (one dimension is the batch), so the work split follows the one
// large operand, W or dW (4 MB / 8 MB at 1000 x 2048), which every kernel
// touches exactly once:
//
//   * head_fc: a block owns 16 classes, its 4 waves take the 32-channel
//     k-steps round robin (the KW idea of gemm_tn) and fold their partials
//     through LDS in wave order. Both MFMA operands are k-contiguous in
//     memory (pooled [n][c], W [k][c]), so a lane's 8-element fragment IS
//     one 16-byte global load: W goes HBM -> VGPR once, with no LDS image
//     to build and no barrier in the k loop. pooled (128 KB at N = 32)
//     comes from L2. Class and row tails: clamped loads, guarded stores
//     (rows and columns of the product are independent).
//   * head_dx: the reduction runs over the classes and W is read in its
//     native [K, C] layout, so the B fragment (8 consecutive k at one c) is
//     a column walk. A block owns 32 channels; each wave stages its own
//     [32 k x 32 c] slab of W (16-byte loads, next slab's loads in flight
//     over the MFMAs) and reads fragments with 8 ds_read_u16. Slab rows are
//     padded to 17 dwords: the four k-groups of a fragment read sit 8 rows
//     apart, 8*17 = 136 = 8 (mod 32) dwords, i.e. on the four disjoint
//     8-bank sets; an XOR slot swizzle cannot do that on a 16-dword row,
//     where rows of equal parity share their 16 banks. The class tail is
//     ZERO-FILLED on both operands (a clamped duplicate would be added into
//     the sum). The block rounds its [rows x 32] result once and
//     broadcast-stores it over the HW pixels with 16-byte stores.
//   * head_dw: output-bound (8 MB of fp32 against a 32-long reduction). A
//     block owns a [64 classes x 64 channels] tile; both operands are
//     staged TRANSPOSED ([col][n], 16-byte rows padded to 80 B) so a
//     fragment is one ds_read_b128, batch rows past N zero-filled up to the
//     MFMA k step. Channels ride the MFMA row index, so a lane's 4
//     accumulators are 4 consecutive channels: one float4 store (or load +
//     add + store in accumulate mode). The blocks of channel tile 0 also
//     sum their 64 columns of dl into db.
//
// Every output element has exactly one owner and every sum a fixed order:
// no atomics, run-to-run bit-identical.
#include "common.h"
#include "launchers.h"

using bf16 = __hip_bfloat16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

__device__ __forceinline__ float bits_f32(unsigned short u) {
  return __uint_as_float(((unsigned)u) << 16);
}
__device__ __forceinline__ unsigned short f32_bits(float f) {
  return (unsigned short)__hip_bfloat16_raw(__float2bfloat16(f)).x;
}

constexpr int kPoolOct = 32;    // channel octets per pool block
constexpr int kPoolSlices = 8;  // hw slices per pool block
constexpr int kRowsPass = 64;   // batch rows per pass of fc / dx (4 tiles)
constexpr int kDxCh = 32;       // channels per dx block
constexpr int kDxRow = 34;      // slab row stride, bf16 elements (17 dwords)
constexpr int kDwPad = 40;      // transposed-tile row stride (32 n + 8)

}  // namespace

// grid (ceil(C/256), N), 256 threads = 32 octets x 8 hw slices. Slice s sums
// pixels s, s+8, ... in order; the 8 slice sums fold in slice order.
extern "C" __global__ __launch_bounds__(256) void head_pool_kernel(
    const bf16* __restrict__ x, bf16* __restrict__ pooled, const int HW,
    const int C) {
  __shared__ float part[kPoolSlices][kPoolOct * 8];
  const int o = threadIdx.x & (kPoolOct - 1);
  const int s = threadIdx.x / kPoolOct;
  const int n = blockIdx.y;
  const int oct = blockIdx.x * kPoolOct + o;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (oct * 8 < C) {
    const bf16* src = x + (long long)n * HW * C + oct * 8;
    for (int hw = s; hw < HW; hw += kPoolSlices) {
      const uint4 raw = *reinterpret_cast<const uint4*>(
          __builtin_assume_aligned(src + (long long)hw * C, 16));
      const unsigned short* u = reinterpret_cast<const unsigned short*>(&raw);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += bits_f32(u[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) part[s][o * 8 + k] = acc[k];
  __syncthreads();
  // thread t owns channel t of the block's 256: consecutive 2-byte stores
  const int c = blockIdx.x * (kPoolOct * 8) + threadIdx.x;
  if (c < C) {
    float v = part[0][threadIdx.x];
#pragma unroll
    for (int i = 1; i < kPoolSlices; ++i) v += part[i][threadIdx.x];
    reinterpret_cast<unsigned short*>(pooled)[(long long)n * C + c] =
        f32_bits(v / (float)HW);
  }
}

// grid ceil(K/16), 256 threads. logits [N, K] = pooled [N, C] . W [K, C]^T
extern "C" __global__ __launch_bounds__(256) void head_fc_kernel(
    const bf16* __restrict__ pooled, const bf16* __restrict__ W,
    const float* __restrict__ bias, bf16* __restrict__ logits, const int N,
    const int C, const int K) {
  __shared__ f32x4 fold[4][4][64];  // [wave][row tile][lane]
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l15 = lane & 15, kg = lane >> 4;
  const int k0 = blockIdx.x * 16;
  const int nsteps = C >> 5;
  const bf16* wp = W + (long long)min(k0 + l15, K - 1) * C + kg * 8;
  const int cls = k0 + l15;
  const float bv = (bias != nullptr && cls < K) ? bias[cls] : 0.f;

  for (int r0 = 0; r0 < N; r0 += kRowsPass) {
    const bf16* ap[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
      ap[rt] = pooled + (long long)min(r0 + rt * 16 + l15, N - 1) * C + kg * 8;
    f32x4 acc[4] = {};
    for (int st = wave; st < nsteps; st += 4) {
      const bf16x8 b = *(const bf16x8*)(wp + st * 32);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        if (r0 + rt * 16 < N) {
          const bf16x8 a = *(const bf16x8*)(ap[rt] + st * 32);
          acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[rt], 0,
                                                            0, 0);
        }
    }
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) fold[wave][rt][lane] = acc[rt];
    __syncthreads();
    // wave w finishes row tile w: partials in wave order, bias, one rounding
    const int rb = r0 + wave * 16;
    if (rb < N && cls < K) {
      f32x4 v = fold[0][wave][lane];
#pragma unroll
      for (int w = 1; w < 4; ++w) v += fold[w][wave][lane];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = rb + kg * 4 + j;
        if (row < N)
          reinterpret_cast<unsigned short*>(logits)[(long long)row * K + cls] =
              f32_bits(v[j] + bv);
      }
    }
    __syncthreads();
  }
}

// grid C/32, 256 threads. dx [N, HW, C] = bcast_hw(bf16((dl [N, K] . W) / HW))
extern "C" __global__ __launch_bounds__(256) void head_dx_kernel(
    const bf16* __restrict__ dl, const bf16* __restrict__ W,
    bf16* __restrict__ dx, const int N, const int C, const int K,
    const int HW) {
  __shared__ __attribute__((aligned(16))) unsigned short slab[2][4][32 * kDxRow];
  __shared__ f32x4 fold[4][8][64];  // [wave][row tile * 2 + col tile][lane]
  __shared__ __attribute__((aligned(16))) unsigned short obuf[kRowsPass][kDxCh];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l15 = lane & 15, kg = lane >> 4;
  const int c0 = blockIdx.x * kDxCh;
  const int nsteps = (K + 31) >> 5;
  const int iters = (nsteps + 3) >> 2;  // uniform over the waves
  const bool k8 = (K & 7) == 0;         // dl rows 16-byte aligned
  const unsigned short* dlu = reinterpret_cast<const unsigned short*>(dl);

  // the wave's slab of k-step ks: 32 class rows x 4 channel octets, two
  // 16-byte loads per lane; rows past K are zero
  auto load_slab = [&](int ks, uint4 (&r)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = lane + i * 64;
      const int k = ks * 32 + (idx >> 2);
      r[i] = make_uint4(0u, 0u, 0u, 0u);
      if (k < K)
        r[i] = *reinterpret_cast<const uint4*>(__builtin_assume_aligned(
            W + (long long)k * C + c0 + (idx & 3) * 8, 16));
    }
  };
  auto store_slab = [&](int buf, const uint4 (&r)[2]) {
    unsigned* d = reinterpret_cast<unsigned*>(slab[buf][wave]);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = lane + i * 64;
      unsigned* p = d + (idx >> 2) * (kDxRow / 2) + (idx & 3) * 4;
      p[0] = r[i].x; p[1] = r[i].y; p[2] = r[i].z; p[3] = r[i].w;
    }
  };

  for (int r0 = 0; r0 < N; r0 += kRowsPass) {
    int arow[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) arow[rt] = min(r0 + rt * 16 + l15, N - 1);
    f32x4 acc[4][2] = {};
    uint4 stg[2];
    load_slab(wave, stg);
    for (int it = 0; it < iters; ++it) {
      const int ks = it * 4 + wave;
      const int buf = it & 1;
      store_slab(buf, stg);
      if (it + 1 < iters) load_slab(ks + 4, stg);
      __syncthreads();
      if (ks < nsteps) {
        const int kc = ks * 32 + kg * 8;
        bf16x8 b[2];
        const unsigned short* sl = slab[buf][wave];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int j = 0; j < 8; ++j)
            b[ct][j] = __builtin_bit_cast(
                __bf16, sl[(kg * 8 + j) * kDxRow + ct * 16 + l15]);
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
          if (r0 + rt * 16 < N) {
            bf16x8 a = {};
            const long long base = (long long)arow[rt] * K + kc;
            if (k8) {
              if (kc < K) a = *(const bf16x8*)(dl + base);
            } else {
#pragma unroll
              for (int j = 0; j < 8; ++j)
                if (kc + j < K) a[j] = __builtin_bit_cast(__bf16, dlu[base + j]);
            }
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
              acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a, b[ct], acc[rt][ct], 0, 0, 0);
          }
      }
    }
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) fold[wave][rt * 2 + ct][lane] = acc[rt][ct];
    __syncthreads();
    // 8 tiles x 64 lanes of float4: two per thread, partials in wave order
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int p = threadIdx.x + i * 256;
      const int tile = p >> 6, ln = p & 63;
      f32x4 v = fold[0][tile][ln];
#pragma unroll
      for (int w = 1; w < 4; ++w) v += fold[w][tile][ln];
      const int row = (tile >> 1) * 16 + (ln >> 4) * 4;
      const int ch = (tile & 1) * 16 + (ln & 15);
#pragma unroll
      for (int j = 0; j < 4; ++j) obuf[row + j][ch] = f32_bits(v[j] / (float)HW);
    }
    __syncthreads();
    // rows r0 .. r0+nv-1 are consecutive images: pixel p of the pass is
    // global pixel r0*HW + p; 4 x 16 bytes per pixel
    const int nv = min(kRowsPass, N - r0);
    const int total = nv * HW * 4;
    bf16* dst = dx + (long long)r0 * HW * C + c0;
    for (int idx = threadIdx.x; idx < total; idx += 256) {
      const int q = idx & 3, p = idx >> 2;
      const uint4 v = *reinterpret_cast<const uint4*>(&obuf[p / HW][q * 8]);
      *reinterpret_cast<uint4*>(
          __builtin_assume_aligned(dst + (long long)p * C + q * 8, 16)) = v;
    }
    __syncthreads();
  }
}

// grid (ceil(K/64), C/64), 256 threads. dW [K, C] fp32, db [K] fp32 (or null)
extern "C" __global__ __launch_bounds__(256) void head_dw_kernel(
    const bf16* __restrict__ dl, const bf16* __restrict__ pooled,
    float* __restrict__ dW, float* __restrict__ db, const int N, const int C,
    const int K, const int acc_w, const int acc_b) {
  __shared__ __attribute__((aligned(16))) unsigned short tp[64][kDwPad];
  __shared__ __attribute__((aligned(16))) unsigned short td[64][kDwPad];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l15 = lane & 15, kg = lane >> 4;
  const int k0 = blockIdx.x * 64;
  const int c0 = blockIdx.y * 64;
  const unsigned short* dlu = reinterpret_cast<const unsigned short*>(dl);
  const bool do_db = db != nullptr && blockIdx.y == 0 && threadIdx.x < 64;

  f32x4 acc[4] = {};
  float dbv = 0.f;
  for (int nb = 0; nb < N; nb += 32) {
    {  // pooled [32 n x 64 c]: one 16-byte load per thread, stored [c][n]
      const int n = threadIdx.x >> 3, oq = threadIdx.x & 7;
      uint4 raw = make_uint4(0u, 0u, 0u, 0u);
      if (nb + n < N)
        raw = *reinterpret_cast<const uint4*>(__builtin_assume_aligned(
            pooled + (long long)(nb + n) * C + c0 + oq * 8, 16));
      const unsigned short* u = reinterpret_cast<const unsigned short*>(&raw);
#pragma unroll
      for (int i = 0; i < 8; ++i) tp[oq * 8 + i][n] = u[i];
    }
    // dl [32 n x 64 k]: rows of dl have no alignment (any K), 2-byte loads
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = threadIdx.x + i * 256;
      const int n = e >> 6, kk = e & 63;
      unsigned short v = 0;
      if (nb + n < N && k0 + kk < K) v = dlu[(long long)(nb + n) * K + k0 + kk];
      td[kk][n] = v;
    }
    __syncthreads();
    const bf16x8 b = *reinterpret_cast<const bf16x8*>(&td[wave * 16 + l15][kg * 8]);
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(&tp[rt * 16 + l15][kg * 8]);
      acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[rt], 0, 0, 0);
    }
    if (do_db) {
#pragma unroll 8
      for (int n = 0; n < 32; ++n) dbv += bits_f32(td[threadIdx.x][n]);
    }
    __syncthreads();
  }
  const int cls = k0 + wave * 16 + l15;
  if (cls < K) {
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      float* p = dW + (long long)cls * C + c0 + rt * 16 + kg * 4;
      f32x4 v = acc[rt];
      if (acc_w) v += *reinterpret_cast<const f32x4*>(p);
      *reinterpret_cast<f32x4*>(p) = v;
    }
  }
  if (do_db && k0 + (int)threadIdx.x < K) {
    float* p = db + k0 + threadIdx.x;
    *p = acc_b ? *p + dbv : dbv;
  }
}

extern "C" void launch_head_fwd(const void* x, const void* w,
                                const float* bias, void* pooled, void* logits,
                                int N, int HW, int C, int K, hipStream_t s) {
  hipLaunchKernelGGL(head_pool_kernel,
                     dim3((C + kPoolOct * 8 - 1) / (kPoolOct * 8), N),
                     dim3(256), 0, s, (const bf16*)x, (bf16*)pooled, HW, C);
  hipLaunchKernelGGL(head_fc_kernel, dim3((K + 15) / 16), dim3(256), 0, s,
                     (const bf16*)pooled, (const bf16*)w, bias, (bf16*)logits,
                     N, C, K);
}

extern "C" void launch_head_dx(const void* dl, const void* w, void* dx, int N,
                               int HW, int C, int K, hipStream_t s) {
  hipLaunchKernelGGL(head_dx_kernel, dim3(C / kDxCh), dim3(256), 0, s,
                     (const bf16*)dl, (const bf16*)w, (bf16*)dx, N, C, K, HW);
}

extern "C" void launch_head_dw(const void* dl, const void* pooled, float* dw,
                               float* db, int N, int C, int K, int acc_w,
                               int acc_b, hipStream_t s) {
  hipLaunchKernelGGL(head_dw_kernel, dim3((K + 63) / 64, C / 64), dim3(256), 0,
                     s, (const bf16*)dl, (const bf16*)pooled, dw, db, N, C, K,
                     acc_w, acc_b);
}
