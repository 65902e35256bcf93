// Training BatchNorm(+ReLU) for the widths bnrelu.hip cannot take: NHWC
// bf16 [M, C] with C > 2048, C % 64 == 0 (the 4096-wide stage-4 BNs of
// ResNeXt101_32x16d). One launch per pass.
//
// bnrelu.hip splits ROWS over the grid, so every block holds 2C floats of
// partial sums and a second launch reduces over blocks: at C = 4096 and the
// short tensors wide BNs see (M = 49*B or 196*B rows) the partial buffer
// is as large as the activation. Here the split is over CHANNELS: block b
// owns the slab [b*W, (b+1)*W) for every row. Per-channel sums are complete
// inside the block, so there is no partial buffer, no finalize launch, no
// global atomic and nothing shared between blocks; statistics, finalize and
// apply (backward: reduce, dgamma/dbeta and dx) run back to back in one
// kernel with two block barriers in between.
//
// Thread t of the 1024 owns octet t % (W/8) of row t / (W/8) of every
// sweep of RPS = 1024 / (W/8) rows: W/8 neighbouring lanes read one
// contiguous 2W-byte run of a row with 16-byte loads (W = 64: a 128-byte
// line), and 4 sweeps (backward: 2) are in flight per thread for the reason
// given at bn_stats_kernel — there is at most one block per CU's worth of
// slabs (C/W <= 256 for every model width), so in-flight bytes per thread
// are what covers the HBM latency.
//
// RESIDENT: pass 1 also stores what it loaded to a dynamic-LDS image of the
// slab, and pass 2 reads that instead of global memory. The image is the
// dense [M, W] bf16 slab in 16-byte slots, slot = row * (W/8) + octet. With
// the thread tiling above that is slot = sweep * 1024 + t: a wave's 64
// lanes write (ds_write_b128) and later read (ds_read_b128) 64 CONSECUTIVE
// 16-byte slots, 1 KiB contiguous, which the LDS serves at full rate: in
// each 16-lane group of a b128 access the lanes cover 64 consecutive banks
// once. No padding or swizzle is needed because pass 2 keeps pass 1's
// thread tiling; each thread reads back its own slots.
//
// The block fold is fixed-order: a xor butterfly over the lanes of a wave
// that share an octet, one LDS row per wave, then 4 chains over the 16
// waves. Identical inputs give identical bits on every launch and replay.
#include "bn_phases.h"
#include "launchers.h"

constexpr int kWideThreads = 1024;
constexpr int kWideWaves = kWideThreads / kWave;
// Dynamic-LDS budget of the resident image(s). With the 8.5 KiB of static
// fold storage a block stays under the CU's 160 KiB; an image of up to
// half the budget leaves room for a second block on the CU.
constexpr int kWideLdsBudget = 144 * 1024;
static_assert(kWideWaves % 4 == 0, "slab_sum folds the waves in 4 chains");

extern __shared__ __attribute__((aligned(16))) char smem[];

__device__ __forceinline__ uint4 load_raw8(const bf16* p) {
  return *reinterpret_cast<const uint4*>(__builtin_assume_aligned(p, 16));
}

__device__ __forceinline__ F8 unpack8(const uint4 raw) {
  F8 o;
  const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o.v[2 * i] = __uint_as_float(w[i] << 16);
    o.v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
  return o;
}

// Inverse of unpack8 for values that ARE bf16 (a masked dy): no rounding.
__device__ __forceinline__ uint4 pack8_exact(const F8& v) {
  unsigned w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    w[i] = (__float_as_uint(v.v[2 * i]) >> 16) |
           (__float_as_uint(v.v[2 * i + 1]) & 0xffff0000u);
  return uint4{w[0], w[1], w[2], w[3]};
}

// This thread's rows of the slab: rl, rl + RPS, ... < M, UN sweeps at a
// time (f(integral_constant<UN>, r) covers r + u*RPS, u < UN), then singly.
// Forward keeps 4 rows in flight; backward 2 rows of dy, x and the mask:
// 4 there spill the 128 VGPRs a 1024-thread block may use.
template <int RPS, int UN, class F>
__device__ __forceinline__ void sweep_rows(const int rl, const int M, F&& f) {
  int r = rl;
  for (; r + (UN - 1) * RPS < M; r += UN * RPS)
    f(std::integral_constant<int, UN>{}, r);
  for (; r < M; r += RPS) f(std::integral_constant<int, 1>{}, r);
}

// Block fold of every thread's two octet accumulators: afterwards
// red[0][w][c] / red[1][w][c] hold wave w's sums of a / b for slab channel
// c, visible to the whole block.
template <int W>
__device__ __forceinline__ void slab_fold(float (&a)[8], float (&b)[8],
                                          float (&red)[2][kWideWaves][W],
                                          const int oct) {
  constexpr int OPR = W / 8;
#pragma unroll
  for (int off = OPR; off < kWave; off <<= 1) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      a[i] += __shfl_xor(a[i], off, kWave);
      b[i] += __shfl_xor(b[i], off, kWave);
    }
  }
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  if (lane < OPR) {  // lane == oct here
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      red[0][wave][oct * 8 + i] = a[i];
      red[1][wave][oct * 8 + i] = b[i];
    }
  }
  __syncthreads();
}

template <int W>
__device__ __forceinline__ float slab_sum(const float (&r)[kWideWaves][W],
                                          const int c) {
  float ch[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int w = 0; w < kWideWaves; w += 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) ch[j] += r[w + j][c];
  }
  return (ch[0] + ch[1]) + (ch[2] + ch[3]);
}

// ---------------- forward ----------------

template <int W, bool RELU, bool RESIDENT>
__global__ __launch_bounds__(kWideThreads) void bn_wide_fwd_kernel(
    const bf16* __restrict__ x, bf16* __restrict__ y,
    unsigned char* __restrict__ mask, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ mean_out,
    float* __restrict__ invstd_out, float* __restrict__ running_mean,
    float* __restrict__ running_var, const float momentum, const float eps,
    const int M, const int C) {
  constexpr int OPR = W / 8, RPS = kWideThreads / OPR;
  __shared__ float red[2][kWideWaves][W];
  __shared__ float par[2][W];  // scale, shift
  uint4* img = reinterpret_cast<uint4*>(smem);  // [M][OPR], RESIDENT only
  const int tid = threadIdx.x;
  const int oct = tid % OPR, rl = tid / OPR;
  const int cb = blockIdx.x * W;  // the slab's first channel
  const int c0 = cb + oct * 8;
  const int c8 = C >> 3;

  // finalize operands of the W finalizer threads, out ahead of pass 1
  const bool fin = tid < W;
  float g = 0.0f, bt = 0.0f, rm = 0.0f, rv = 0.0f;
  if (fin) {
    g = gamma[cb + tid];
    bt = beta[cb + tid];
    if (running_mean != nullptr) {
      rm = running_mean[cb + tid];
      rv = running_var[cb + tid];
    }
  }

  // ---- pass 1: sum and sum of squares (+ the LDS image) ----
  float s[8] = {0}, q[8] = {0};
  sweep_rows<RPS, 4>(rl, M, [&](auto U, const int r) {
    constexpr int N = decltype(U)::value;
    uint4 raw[N];
#pragma unroll
    for (int u = 0; u < N; ++u)
      raw[u] = load_raw8(x + (long long)(r + u * RPS) * C + c0);
#pragma unroll
    for (int u = 0; u < N; ++u) {
      if (RESIDENT) img[(r + u * RPS) * OPR + oct] = raw[u];
      const F8 v = unpack8(raw[u]);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        s[i] += v.v[i];
        q[i] = fmaf(v.v[i], v.v[i], q[i]);
      }
    }
  });
  slab_fold<W>(s, q, red, oct);

  // ---- finalize the slab's W channels ----
  if (fin) {
    bn_channel_finalize<double>(
        slab_sum<W>(red[0], tid), slab_sum<W>(red[1], tid), g, bt, rm, rv, M,
        momentum, eps, tid, mean_out + cb, invstd_out + cb, par[0], par[1],
        running_mean != nullptr ? running_mean + cb : nullptr,
        running_var + cb);
  }
  __syncthreads();

  // ---- pass 2: apply ----
  float sc[8], sh[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sc[i] = par[0][oct * 8 + i];
    sh[i] = par[1][oct * 8 + i];
  }
  sweep_rows<RPS, 4>(rl, M, [&](auto U, const int r) {
    constexpr int N = decltype(U)::value;
    uint4 raw[N];
#pragma unroll
    for (int u = 0; u < N; ++u) {
      const int ru = r + u * RPS;
      raw[u] = RESIDENT ? img[ru * OPR + oct]
                        : load_raw8(x + (long long)ru * C + c0);
    }
#pragma unroll
    for (int u = 0; u < N; ++u) {
      const long long ru = r + u * RPS;
      F8 v = unpack8(raw[u]);
      const unsigned char mb =
          apply_octet<RELU, false>(v, nullptr, sc, sh, 0);
      store8(y + ru * C + c0, v);
      if (RELU) mask[ru * c8 + (c0 >> 3)] = mb;
    }
  });
}

// ---------------- backward ----------------

template <int W, bool RELU, bool RESIDENT>
__global__ __launch_bounds__(kWideThreads) void bn_wide_bwd_kernel(
    const bf16* __restrict__ dy, const unsigned char* __restrict__ mask,
    const bf16* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    float* __restrict__ sums,  // [dbeta; dgamma], fp32 [2, C]
    float* __restrict__ db_acc, float* __restrict__ dg_acc,
    bf16* __restrict__ dx, const int M, const int C) {
  constexpr int OPR = W / 8, RPS = kWideThreads / OPR;
  __shared__ float red[2][kWideWaves][W];
  __shared__ float par[2][W];  // s1 = sum dy_eff, s2 = sum dy_eff * xhat
  // RESIDENT only: dy_eff [M][OPR], then x [M][OPR]
  uint4* img_g = reinterpret_cast<uint4*>(smem);
  uint4* img_x = img_g + M * OPR;
  const int tid = threadIdx.x;
  const int oct = tid % OPR, rl = tid / OPR;
  const int cb = blockIdx.x * W;
  const int c0 = cb + oct * 8;
  const int c8 = C >> 3;

  float mu[8], is[8], gm[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    mu[i] = mean[c0 + i];
    is[i] = invstd[c0 + i];
    gm[i] = gamma[c0 + i];
  }

  // one row segment: dy_eff and x as floats, from global
  auto load_rows = [&](auto U, const int r, F8 (&gv)[decltype(U)::value],
                       F8 (&xv)[decltype(U)::value]) {
    constexpr int N = decltype(U)::value;
    uint4 rg[N], rx[N];
    unsigned mb[N];
#pragma unroll
    for (int u = 0; u < N; ++u) {
      const long long ru = r + u * RPS;
      rg[u] = load_raw8(dy + ru * C + c0);
      rx[u] = load_raw8(x + ru * C + c0);
      if (RELU) mb[u] = mask[ru * c8 + (c0 >> 3)];
    }
#pragma unroll
    for (int u = 0; u < N; ++u) {
      gv[u] = unpack8(rg[u]);
      if (RELU) relu_select(gv[u], mb[u]);
      xv[u] = unpack8(rx[u]);
    }
  };

  // ---- pass 1: s1, s2 (+ the LDS images) ----
  float s1[8] = {0}, s2[8] = {0};
  sweep_rows<RPS, 2>(rl, M, [&](auto U, const int r) {
    constexpr int N = decltype(U)::value;
    F8 gv[N], xv[N];
    load_rows(U, r, gv, xv);
#pragma unroll
    for (int u = 0; u < N; ++u) {
      if (RESIDENT) {
        img_g[(r + u * RPS) * OPR + oct] = pack8_exact(gv[u]);
        img_x[(r + u * RPS) * OPR + oct] = pack8_exact(xv[u]);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        s1[i] += gv[u].v[i];
        s2[i] = fmaf(gv[u].v[i], (xv[u].v[i] - mu[i]) * is[i], s2[i]);
      }
    }
  });
  slab_fold<W>(s1, s2, red, oct);

  // ---- dbeta, dgamma: the block is the only writer of its channels ----
  if (tid < W) {
    const float b = slab_sum<W>(red[0], tid), gsum = slab_sum<W>(red[1], tid);
    par[0][tid] = b;
    par[1][tid] = gsum;
    sums[cb + tid] = b;
    sums[C + cb + tid] = gsum;
    if (db_acc != nullptr) db_acc[cb + tid] += b;
    if (dg_acc != nullptr) dg_acc[cb + tid] += gsum;
  }
  __syncthreads();

  // ---- pass 2: dx ----
  float sm[16];  // dx_octet's sums[c] / sums[C + c] with c0 = 0, C = 8
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sm[i] = par[0][oct * 8 + i];
    sm[8 + i] = par[1][oct * 8 + i];
  }
  const float inv_m = 1.0f / (float)M;
  sweep_rows<RPS, 2>(rl, M, [&](auto U, const int r) {
    constexpr int N = decltype(U)::value;
    F8 gv[N], xv[N];
    if (RESIDENT) {
#pragma unroll
      for (int u = 0; u < N; ++u) {
        gv[u] = unpack8(img_g[(r + u * RPS) * OPR + oct]);
        xv[u] = unpack8(img_x[(r + u * RPS) * OPR + oct]);
      }
    } else {
      load_rows(U, r, gv, xv);
    }
#pragma unroll
    for (int u = 0; u < N; ++u)
      store8(dx + (long long)(r + u * RPS) * C + c0,
             dx_octet<true>(gv[u], xv[u], mu, is, gm, sm, inv_m, 0, 8));
  });
}

// ---------------- launchers ----------------

// EDL_BN_WIDE_W = 32 | 64 forces the slab width, EDL_BN_WIDE_RESIDENT = 0
// the streaming variant: the A/B columns of tools/bn_wide_bench.py. Read
// per call so one process can time every column.
//
// The picks, measured at C = 4096 (docs/kernels.md, "bn_wide.hip"): W = 32
// (C/32 blocks, twice the CUs busy) wins every backward by more than the
// spread; in forward the two widths differ by less than the order of the
// columns in the timing loop does, so W = 32 serves both passes.
static int wide_resident_cap(const int W, const int backward) {
  const char* e = getenv("EDL_BN_WIDE_RESIDENT");
  if (e && atoi(e) == 0) return 0;
  return kWideLdsBudget / (W * 2 * (backward ? 2 : 1));
}

static int wide_pick_w() {
  const char* e = getenv("EDL_BN_WIDE_W");
  return e && atoi(e) == 64 ? 64 : 32;
}

extern "C" int bn_wide_resident_rows(int C, int backward) {
  (void)C;  // the cap is the same at every width
  return wide_resident_cap(wide_pick_w(), backward);
}

// A launch may ask for more than the 64 KiB default of dynamic LDS only
// after the kernel was told so, once per instantiation.
template <auto Kernel>
static void wide_allow_lds() {
  static const hipError_t e = hipFuncSetAttribute(
      reinterpret_cast<const void*>(Kernel),
      hipFuncAttributeMaxDynamicSharedMemorySize, kWideLdsBudget);
  (void)e;
}

extern "C" void launch_bn_wide_fwd(const void* x, void* y, unsigned char* mask,
                                   const float* gamma, const float* beta,
                                   float* mean, float* invstd, float* rmean,
                                   float* rvar, float momentum, float eps,
                                   int M, int C, bool relu, hipStream_t s) {
  const int W = wide_pick_w();
  const bool resident = M <= wide_resident_cap(W, 0);
  const size_t lds = resident ? (size_t)M * W * 2 : 0;
  dispatch_bools(
      [&](auto W64, auto R, auto Res) {
        constexpr int Wc = decltype(W64)::value ? 64 : 32;
        constexpr auto kern = bn_wide_fwd_kernel<Wc, decltype(R)::value,
                                                 decltype(Res)::value>;
        if (decltype(Res)::value) wide_allow_lds<kern>();
        hipLaunchKernelGGL(kern, dim3(C / Wc), dim3(kWideThreads), lds, s,
                           (const bf16*)x, (bf16*)y, mask, gamma, beta, mean,
                           invstd, rmean, rvar, momentum, eps, M, C);
      },
      W == 64, relu, resident);
}

extern "C" void launch_bn_wide_bwd(const void* dy, const unsigned char* mask,
                                   const void* x, const float* mean,
                                   const float* invstd, const float* gamma,
                                   float* sums, float* db_acc, float* dg_acc,
                                   void* dx, int M, int C, bool relu,
                                   hipStream_t s) {
  const int W = wide_pick_w();
  const bool resident = M <= wide_resident_cap(W, 1);
  const size_t lds = resident ? (size_t)M * W * 4 : 0;
  dispatch_bools(
      [&](auto W64, auto R, auto Res) {
        constexpr int Wc = decltype(W64)::value ? 64 : 32;
        constexpr auto kern = bn_wide_bwd_kernel<Wc, decltype(R)::value,
                                                 decltype(Res)::value>;
        if (decltype(Res)::value) wide_allow_lds<kern>();
        hipLaunchKernelGGL(kern, dim3(C / Wc), dim3(kWideThreads), lds, s,
                           (const bf16*)dy, mask, (const bf16*)x, mean, invstd,
                           gamma, sums, db_acc, dg_acc, (bf16*)dx, M, C);
      },
      W == 64, relu, resident);
}
