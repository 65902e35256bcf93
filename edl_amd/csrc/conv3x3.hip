// Implicit-GEMM 3x3 convolution (stride 1 or 2, same-pad) on PADDED NHWC
// bf16 input — the ResNet bottleneck 3x3s (MIOpen's igemm ran them at a
// few % of MFMA peak).
//
//   y[M, Cout] = sum_{s=(dy,dx)} A_s[M, Cin] @ B_s[Cout, Cin]^T
//
// where A_s row m reads xp[n, h*stride+dy, w*stride+dx, :] of the padded
// image xp [N, Hp, Wp, Cin] (halo pre-zeroed by pad_nhwc — no border
// predicates in the hot loop), and B = W3 [Cout, 9*Cin] (s-major repacked
// weights) is EXACTLY the gemm_bt B operand with K = 9*Cin.
//
// Same engine as gemm_bt: 4 waves, 64x64 per wave, BK=64,
// global_load_lds 16B staging (XOR source+read swizzle), double-buffered
// LDS, mfma_f32_16x16x32_bf16. The only delta: each thread PRECOMPUTES
// the padded-row byte address for the A rows it stages (fixed across the
// K loop); the k-tile adds shift_off[s] + 128*cb.
#include "common.h"
#include "launchers.h"

using bf16 = __hip_bfloat16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

extern __shared__ __attribute__((aligned(16))) char smem[];

// zero-halo pad: xp[n, h+1, w+1, c] = x[n, h, w, c]; halo = 0.
extern "C" __global__ void pad_nhwc_kernel(
    const bf16* __restrict__ x, bf16* __restrict__ xp, const int HW_in,
    const int H, const int W, const int Hp, const int Wp, const int C) {
  const int c8 = C >> 3;
  const long long total = (long long)gridDim.y * Hp * Wp * c8;  // per image n
  // grid: x = flat over Hp*Wp*c8 (strided), y = image index
  const int n = blockIdx.y;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long img_elems = (long long)Hp * Wp * c8;
  for (; i < img_elems; i += stride) {
    const int oct = (int)(i % c8);
    const long long pix = i / c8;
    const int wp = (int)(pix % Wp);
    const int hp = (int)(pix / Wp);
    bf16* dst = xp + ((long long)n * Hp * Wp + pix) * C + oct * 8;
    const int h = hp - 1, w = wp - 1;
    if (h >= 0 && h < H && w >= 0 && w < W) {
      const bf16* src = x + (((long long)n * H + h) * W + w) * C + oct * 8;
      *reinterpret_cast<uint4*>(__builtin_assume_aligned(dst, 16)) =
          *reinterpret_cast<const uint4*>(__builtin_assume_aligned(src, 16));
    } else {
      *reinterpret_cast<uint4*>(__builtin_assume_aligned(dst, 16)) = uint4{0, 0, 0, 0};
    }
  }
  (void)HW_in;
  (void)total;
}

// GROUPED: grouped conv (ResNeXt 32x16d shapes, 16-128 in/out channels
// per group). `gw` is the GEMM group width — the contiguous input-channel
// window each 64-wide n-tile consumes, at channel base (n0/gw)*gw:
//   cpg >= 64: gw = cpg. A 64-wide n-tile's groups share exactly their
//     own input channels -> the dense engine runs with ZERO wasted MFMA
//     (stage 3/4 of ResNeXt101_32x16d, ~80% of its grouped FLOPs).
//   cpg 16/32: gw = 64 with a block-diagonal zero-padded weight repack
//     (4x/2x MFMA on zeros, still ~MFMA rate vs MIOpen's grouped path).
// SPLITK (grid.y > 1, non-grouped): the deep-K small-M shapes (ResNet
// stage 3/4: 52-98 tiles on a 256-CU chip, K up to 4608) slice the
// K-range over grid.y and atomically fold fp32 partials into C_part
// (zeroed by the caller; cast to bf16 afterwards) — measured 56 us/call
// at 52 blocks before, CU-starved.
// BN_PART: per-channel sum/sumsq partials of the (bf16-rounded) OUTPUT,
// one row per m-tile ([tiles_m, 2N]: sums then sumsq) — the following
// BatchNorm skips its stats kernel entirely (a full activation re-read,
// measured ~0.53 ms/step). Folded in the epilogue via LDS atomics into
// the dead staging buffers; disjoint column ranges per block, so the
// partial rows need no zero-init and no global atomics.
// AFF (0 = off, 1 = affine, 2 = affine + relu; never with split-K or
// BN_PART): the eval-mode BN(+ReLU) of the following layer folded into the
// epilogue on the bf16-ROUNDED accumulator, bit for bit this kernel followed
// by bnrelu.hip's bn_apply_kernel:
//   C = bf16(relu?(fmaf(float(bf16(acc)), scale[n], shift[n])))
// scale/shift (fp32 [N]) are loaded into registers ahead of the K loop.
template <int BM, int BN, int WAVES_M, int WAVES_N, bool GROUPED = false,
          int AFF = 0>
__global__ __launch_bounds__(256, 2) void conv3x3_kernel(
    const bf16* __restrict__ XP, const bf16* __restrict__ B,
    bf16* __restrict__ C_out, const int M, const int N, const int Cin,
    const int HW_out, const int W_out, const int Hp, const int Wp,
    const int stride_hw, const int gw = 0,
    float* __restrict__ C_part = nullptr,
    float* __restrict__ bn_part = nullptr,
    const float* __restrict__ bn_scale = nullptr,
    const float* __restrict__ bn_shift = nullptr) {
  constexpr int BK = 64;
  constexpr int A_BYTES = BM * BK * 2;
  constexpr int B_BYTES = BN * BK * 2;
  const int Cin_k = GROUPED ? gw : Cin;  // channels entering the gemm K
  const int K = 9 * Cin_k;               // gemm K
  const int cb_per_s = Cin_k >> 6;       // 64-wide channel blocks per shift
  char* lds = smem;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  const int tiles_n = N / BN;
  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int m0 = (bid / tiles_n) * BM;
  const int n0 = (bid % tiles_n) * BN;
  const int wm = (wave / WAVES_N) * 64;
  const int wn = (wave % WAVES_N) * 64;

  // ---- per-thread A-row address table (fixed across the K loop) ----
  constexpr int A_CHUNKS = A_BYTES / 1024;
  constexpr int B_CHUNKS = B_BYTES / 1024;
  long long arow[A_CHUNKS / 4];
#pragma unroll
  for (int i = 0; i < A_CHUNKS / 4; ++i) {
    const int ch = wave * (A_CHUNKS / 4) + i;
    const int r = ch * 8 + (lane >> 3);
    long long m = m0 + r;
    if (m >= M) m = M - 1;  // clamped dup row; C-write guarded
    const int n_img = (int)(m / HW_out);
    const int rem = (int)(m % HW_out);
    const int h = rem / W_out;
    const int w = rem % W_out;
    arow[i] = (((long long)n_img * Hp + h * stride_hw) * Wp + w * stride_hw) *
              Cin;  // element offset of (dy=0, dx=0)
  }
  int shift_elems[9];
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    shift_elems[s] = ((s / 3) * Wp + (s % 3)) * Cin;
  }

  const int a_ch_base = GROUPED ? (n0 / gw) * gw : 0;  // group channel base
  auto stage = [&](int buf, int kt) {
    const int s = kt / cb_per_s;
    const int cb = kt % cb_per_s;
    char* abase = lds + buf * (A_BYTES + B_BYTES);
    char* bbase = abase + A_BYTES;
#pragma unroll
    for (int i = 0; i < A_CHUNKS / 4; ++i) {
      const int ch = wave * (A_CHUNKS / 4) + i;
      const int r = ch * 8 + (lane >> 3);
      const int gslot = (lane & 7) ^ (r & 7);
      const bf16* src = XP + arow[i] + shift_elems[s] + a_ch_base + cb * 64 +
                        gslot * 8;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)(abase + ch * 1024), 16, 0, 0);
    }
    const long long k0 = (long long)kt * BK;
#pragma unroll
    for (int i = 0; i < B_CHUNKS / 4; ++i) {
      const int ch = wave * (B_CHUNKS / 4) + i;
      const int r = ch * 8 + (lane >> 3);
      const int gslot = (lane & 7) ^ (r & 7);
      const bf16* src = B + (long long)(n0 + r) * K + k0 + gslot * 8;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)(bbase + ch * 1024), 16, 0, 0);
    }
  };

  auto read_a = [&](int buf, int mf, int kk) -> bf16x8 {
    const char* abase = lds + buf * (A_BYTES + B_BYTES);
    const int r = wm + mf * 16 + (lane & 15);
    const int c = kk * 4 + (lane >> 4);
    return *(const __attribute__((address_space(3))) bf16x8*)(
        (const __attribute__((address_space(3))) char*)(abase) + r * 128 +
        ((c ^ (r & 7)) << 4));
  };
  auto read_b = [&](int buf, int nf, int kk) -> bf16x8 {
    const char* bbase = lds + buf * (A_BYTES + B_BYTES) + A_BYTES;
    const int r = wn + nf * 16 + (lane & 15);
    const int c = kk * 4 + (lane >> 4);
    return *(const __attribute__((address_space(3))) bf16x8*)(
        (const __attribute__((address_space(3))) char*)(bbase) + r * 128 +
        ((c ^ (r & 7)) << 4));
  };

  f32x4 acc[4][4] = {};
  const int KT = K / BK;
  int kt0 = 0, kt1 = KT;
  if (!GROUPED && gridDim.y > 1) {
    const int per = (KT + gridDim.y - 1) / gridDim.y;
    kt0 = blockIdx.y * per;
    kt1 = kt0 + per < KT ? kt0 + per : KT;
    if (kt0 >= kt1) return;
  }
  stage(kt0 & 1, kt0);
  // AFF: the lane's 4 + 4 scale/shift values (columns n0 + wn + nf*16 +
  // (lane & 15)), issued here so the epilogue waits on nothing
  float aff_sc[4], aff_sh[4];
  if constexpr (AFF != 0) {
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      aff_sc[nf] = bn_scale[n0 + wn + nf * 16 + (lane & 15)];
      aff_sh[nf] = bn_shift[n0 + wn + nf * 16 + (lane & 15)];
    }
  }
  __syncthreads();
  for (int kt = kt0; kt < kt1; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < kt1) stage(cur ^ 1, kt + 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 a[4], b[4];
#pragma unroll
      for (int mf = 0; mf < 4; ++mf) a[mf] = read_a(cur, mf, kk);
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) b[nf] = read_b(cur, nf, kk);
#pragma unroll
      for (int mf = 0; mf < 4; ++mf)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
          acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[mf], b[nf], acc[mf][nf], 0, 0, 0);
    }
    __syncthreads();
  }

  const int cn = lane & 15;
  const int r4 = (lane >> 4) * 4;
  if constexpr (AFF != 0) {
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int m = m0 + wm + mf * 16 + r4 + reg;
        if (m < M) {
          bf16* crow = C_out + (long long)m * N + n0 + wn + cn;
#pragma unroll
          for (int nf = 0; nf < 4; ++nf) {
            const bf16 yb = __float2bfloat16(acc[mf][nf][reg]);
            float v = fmaf(__bfloat162float(yb), aff_sc[nf], aff_sh[nf]);
            if constexpr (AFF == 2) v = fmaxf(v, 0.0f);
            crow[nf * 16] = __float2bfloat16(v);
          }
        }
      }
    }
    return;
  }
  // local per-column stats accumulators (summed into LDS afterwards)
  float ls[4] = {0, 0, 0, 0}, lq[4] = {0, 0, 0, 0};
#pragma unroll
  for (int mf = 0; mf < 4; ++mf) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int m = m0 + wm + mf * 16 + r4 + reg;
      if (m < M) {
        if (!GROUPED && C_part != nullptr) {
          float* prow = C_part + (long long)m * N + n0 + wn + cn;
#pragma unroll
          for (int nf = 0; nf < 4; ++nf)
            atomicAdd(&prow[nf * 16], acc[mf][nf][reg]);
        } else {
          bf16* crow = C_out + (long long)m * N + n0 + wn + cn;
#pragma unroll
          for (int nf = 0; nf < 4; ++nf) {
            const bf16 yb = __float2bfloat16(acc[mf][nf][reg]);
            crow[nf * 16] = yb;
            if (bn_part != nullptr) {
              // stats must see the bf16-ROUNDED value BN will read
              const float yv = __bfloat162float(yb);
              ls[nf] += yv;
              lq[nf] = fmaf(yv, yv, lq[nf]);
            }
          }
        }
      }
    }
  }

  if (bn_part != nullptr) {
    // the staging buffers are dead past the last k-loop barrier
    float* bsum = (float*)smem;
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * BN; i += blockDim.x) bsum[i] = 0.0f;
    __syncthreads();
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      // fold the 4 lanes sharing column cn (lane, +16, +32, +48): ONE
      // LDS atomic per address per wave instead of a 4-way serialized
      // same-address conflict
      ls[nf] += __shfl_down(ls[nf], 32);
      ls[nf] += __shfl_down(ls[nf], 16);
      lq[nf] += __shfl_down(lq[nf], 32);
      lq[nf] += __shfl_down(lq[nf], 16);
    }
    if (lane < 16) {
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) {
        atomicAdd(&bsum[wn + nf * 16 + cn], ls[nf]);
        atomicAdd(&bsum[BN + wn + nf * 16 + cn], lq[nf]);
      }
    }
    __syncthreads();
    // fold into <= kStatsPartRowCap partial rows (finalize latency/traffic
    // cap): rows beyond the cap atomically add into row mtile %% cap
    // (buffer pre-zeroed by the caller in that case)
    const int tiles_m = gridDim.x / (N / BN);
    const int cap = tiles_m < kStatsPartRowCap ? tiles_m : kStatsPartRowCap;
    const int mtile = (bid / (N / BN)) % cap;
    float* dst = bn_part + (long long)mtile * 2 * N + n0;
    if (tiles_m > cap) {
      for (int i = threadIdx.x; i < BN; i += blockDim.x) {
        atomicAdd(&dst[i], bsum[i]);
        atomicAdd(&dst[N + i], bsum[BN + i]);
      }
    } else {
      for (int i = threadIdx.x; i < BN; i += blockDim.x) {
        dst[i] = bsum[i];
        dst[N + i] = bsum[BN + i];
      }
    }
  }
}

// ---- small-channel 3x3 conv (the ResNet-vd deep stem: 3->32->32->64 at
// 112-224px) ----
//
// The dense kernel needs C % 64; the stem has Cin in {3(padded 16), 32}
// and Cout in {32, 64}. Here a 64-wide K-step spans TPK = 64/CPT taps of
// CPT channels each (taps padded to TAPS_PAD with zero weights, A re-reads
// tap 0 there), and the gemm N is padded to 64 with zero B rows + a
// guarded store against Cout_real. Replaces MIOpen's stem fwd/dgrad
// (igemm/naive find-phase — VERDICT r1 #4).
template <int CPT>
__global__ __launch_bounds__(256, 2) void conv3x3_small_kernel(
    const bf16* __restrict__ XP, const bf16* __restrict__ B,
    bf16* __restrict__ C_out, const int M, const int Cout_real,
    const int HW_out, const int W_out, const int Hp, const int Wp,
    const int stride_hw, float* __restrict__ bn_part = nullptr) {
  constexpr int BM = 256, BN = 64;
  constexpr int TPK = 64 / CPT;                    // taps per 64-K step
  constexpr int TAPS_PAD = CPT == 16 ? 12 : (CPT == 32 ? 10 : 9);
  constexpr int K = TAPS_PAD * CPT;
  constexpr int KT = K / 64;
  constexpr int A_BYTES = BM * 64 * 2;
  constexpr int B_BYTES = BN * 64 * 2;
  char* lds = smem;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int m0 = bid * BM;      // single 64-wide n-tile
  const int wm = wave * 64;

  constexpr int A_CHUNKS = A_BYTES / 1024;
  constexpr int B_CHUNKS = B_BYTES / 1024;
  long long arow[A_CHUNKS / 4];
#pragma unroll
  for (int i = 0; i < A_CHUNKS / 4; ++i) {
    const int ch = wave * (A_CHUNKS / 4) + i;
    const int r = ch * 8 + (lane >> 3);
    long long m = m0 + r;
    if (m >= M) m = M - 1;
    const int n_img = (int)(m / HW_out);
    const int rem = (int)(m % HW_out);
    const int h = rem / W_out;
    const int w = rem % W_out;
    arow[i] = (((long long)n_img * Hp + h * stride_hw) * Wp +
               w * stride_hw) * CPT;
  }
  int shift_elems[TAPS_PAD];
#pragma unroll
  for (int s = 0; s < TAPS_PAD; ++s) {
    const int t = s < 9 ? s : 0;  // padded taps re-read tap 0 (B zeros)
    shift_elems[s] = ((t / 3) * Wp + (t % 3)) * CPT;
  }

  auto stage = [&](int buf, int kt) {
    char* abase = lds + buf * (A_BYTES + B_BYTES);
    char* bbase = abase + A_BYTES;
#pragma unroll
    for (int i = 0; i < A_CHUNKS / 4; ++i) {
      const int ch = wave * (A_CHUNKS / 4) + i;
      const int r = ch * 8 + (lane >> 3);
      const int gslot = (lane & 7) ^ (r & 7);
      const int tap = kt * TPK + gslot / (CPT / 8);
      const int coff = (gslot % (CPT / 8)) * 8;
      const bf16* src = XP + arow[i] + shift_elems[tap] + coff;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)(abase + ch * 1024), 16, 0, 0);
    }
    const long long k0 = (long long)kt * 64;
#pragma unroll
    for (int i = 0; i < B_CHUNKS / 4; ++i) {
      const int ch = wave * (B_CHUNKS / 4) + i;
      const int r = ch * 8 + (lane >> 3);
      const int gslot = (lane & 7) ^ (r & 7);
      const bf16* src = B + (long long)r * K + k0 + gslot * 8;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)(bbase + ch * 1024), 16, 0, 0);
    }
  };

  auto read_a = [&](int buf, int mf, int kk) -> bf16x8 {
    const char* abase = lds + buf * (A_BYTES + B_BYTES);
    const int r = wm + mf * 16 + (lane & 15);
    const int c = kk * 4 + (lane >> 4);
    return *(const __attribute__((address_space(3))) bf16x8*)(
        (const __attribute__((address_space(3))) char*)(abase) + r * 128 +
        ((c ^ (r & 7)) << 4));
  };
  auto read_b = [&](int buf, int nf, int kk) -> bf16x8 {
    const char* bbase = lds + buf * (A_BYTES + B_BYTES) + A_BYTES;
    const int r = nf * 16 + (lane & 15);
    const int c = kk * 4 + (lane >> 4);
    return *(const __attribute__((address_space(3))) bf16x8*)(
        (const __attribute__((address_space(3))) char*)(bbase) + r * 128 +
        ((c ^ (r & 7)) << 4));
  };

  f32x4 acc[4][4] = {};
  stage(0, 0);
  __syncthreads();
  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < KT) stage(cur ^ 1, kt + 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 a[4], b[4];
#pragma unroll
      for (int mf = 0; mf < 4; ++mf) a[mf] = read_a(cur, mf, kk);
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) b[nf] = read_b(cur, nf, kk);
#pragma unroll
      for (int mf = 0; mf < 4; ++mf)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
          acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[mf], b[nf], acc[mf][nf], 0, 0, 0);
    }
    __syncthreads();
  }

  const int cn = lane & 15;
  const int r4 = (lane >> 4) * 4;
  float ls[4] = {0, 0, 0, 0}, lq[4] = {0, 0, 0, 0};
#pragma unroll
  for (int mf = 0; mf < 4; ++mf) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int m = m0 + wm + mf * 16 + r4 + reg;
      if (m < M) {
        bf16* crow = C_out + (long long)m * Cout_real + cn;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
          if (nf * 16 + cn < Cout_real) {
            const bf16 yb = __float2bfloat16(acc[mf][nf][reg]);
            crow[nf * 16] = yb;
            if (bn_part != nullptr) {
              const float yv = __bfloat162float(yb);
              ls[nf] += yv;
              lq[nf] = fmaf(yv, yv, lq[nf]);
            }
          }
      }
    }
  }

  if (bn_part != nullptr) {  // see conv3x3_kernel BN_PART comment
    float* bsum = (float*)smem;
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * BN; i += blockDim.x) bsum[i] = 0.0f;
    __syncthreads();
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      // fold the 4 lanes sharing column cn (lane, +16, +32, +48): ONE
      // LDS atomic per address per wave instead of a 4-way serialized
      // same-address conflict
      ls[nf] += __shfl_down(ls[nf], 32);
      ls[nf] += __shfl_down(ls[nf], 16);
      lq[nf] += __shfl_down(lq[nf], 32);
      lq[nf] += __shfl_down(lq[nf], 16);
    }
    if (lane < 16) {
#pragma unroll
      for (int nf = 0; nf < 4; ++nf)
        if (nf * 16 + cn < Cout_real) {
          atomicAdd(&bsum[nf * 16 + cn], ls[nf]);
          atomicAdd(&bsum[BN + nf * 16 + cn], lq[nf]);
        }
    }
    __syncthreads();
    const int cap = (int)gridDim.x < kStatsPartRowCap ? (int)gridDim.x
                                                      : kStatsPartRowCap;
    float* dst = bn_part + (long long)(bid % cap) * 2 * Cout_real;
    if ((int)gridDim.x > cap) {
      for (int i = threadIdx.x; i < Cout_real; i += blockDim.x) {
        atomicAdd(&dst[i], bsum[i]);
        atomicAdd(&dst[Cout_real + i], bsum[BN + i]);
      }
    } else {
      for (int i = threadIdx.x; i < Cout_real; i += blockDim.x) {
        dst[i] = bsum[i];
        dst[Cout_real + i] = bsum[BN + i];
      }
    }
  }
}

// zero-halo + CHANNEL pad for the 3-channel stem input: xp[n,h+1,w+1,c] =
// x[n,h,w,c] for c < Creal else 0 (xp has Cpad channels).
extern "C" __global__ void pad_nhwc_cpad_kernel(
    const bf16* __restrict__ x, bf16* __restrict__ xp, const int H,
    const int W, const int Hp, const int Wp, const int Creal,
    const int Cpad) {
  const int n = blockIdx.y;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long img_px = (long long)Hp * Wp;
  for (; i < img_px; i += stride) {
    const int wp = (int)(i % Wp);
    const int hp = (int)(i / Wp);
    bf16* dst = xp + ((long long)n * img_px + i) * Cpad;
    const int h = hp - 1, w = wp - 1;
    const bool in = h >= 0 && h < H && w >= 0 && w < W;
    const bf16* src = x + (((long long)n * H + h) * W + w) * Creal;
    // build the padded row in registers, store 16 B octets (the scalar
    // per-channel store loop measured ~0.7 TB/s)
    for (int o = 0; o < Cpad; o += 8) {
      uint4 raw = {0, 0, 0, 0};
      ushort* u = reinterpret_cast<ushort*>(&raw);
      if (in) {
#pragma unroll 8
        for (int k = 0; k < 8; ++k) {
          const int c = o + k;
          if (c < Creal)
            u[k] = __hip_bfloat16_raw(src[c]).x;
        }
      }
      *reinterpret_cast<uint4*>(__builtin_assume_aligned(dst + o, 16)) = raw;
    }
  }
}

extern "C" void launch_pad_nhwc_cpad(const void* x, void* xp, int Nimg, int H,
                                     int W, int Hp, int Wp, int Creal,
                                     int Cpad, hipStream_t s) {
  const long long per_img = (long long)Hp * Wp;
  int gx = (int)((per_img + 255) / 256);
  if (gx > 512) gx = 512;
  hipLaunchKernelGGL(pad_nhwc_cpad_kernel, dim3(gx, Nimg), dim3(256), 0, s,
                     (const bf16*)x, (bf16*)xp, H, W, Hp, Wp, Creal, Cpad);
}

// rows per block of conv3x3_small_kernel (its BM); the grid is one block
// per m-tile, which is also the stats-partial row count before the cap
constexpr int kSmallBM = 256;

extern "C" int conv3x3_small_tiles_m(int M) {
  return (M + kSmallBM - 1) / kSmallBM;
}

extern "C" void launch_conv3x3_small(const void* xp, const void* w3s, void* y,
                                     int M, int Cout_real, int cpt, int HW_out,
                                     int W_out, int Hp, int Wp, int stride,
                                     float* bn_part, hipStream_t s) {
  constexpr int BM = kSmallBM;
  const int grid = conv3x3_small_tiles_m(M);
  const int lds_bytes = 2 * (BM * 64 * 2 + 64 * 64 * 2);
#define SCASE(CPT)                                                          \
  hipLaunchKernelGGL((conv3x3_small_kernel<CPT>), dim3(grid), dim3(256),    \
                     lds_bytes, s, (const bf16*)xp, (const bf16*)w3s,       \
                     (bf16*)y, M, Cout_real, HW_out, W_out, Hp, Wp, stride, \
                     bn_part)
  if (cpt == 16) SCASE(16);
  else if (cpt == 32) SCASE(32);
  else SCASE(64);
#undef SCASE
}

// ---- stride-2 3x3 same-pad DGRAD via parity decomposition ----
//
// dx[n,h,w,:] of parity class p=(h&1,w&1) receives only taps with
// dy≡(h+1)&1, dxx≡(w+1)&1 — classes have 1/2/2/4 taps — so each class is
// an implicit GEMM over K = T*Cout against the zero-padded dY:
//   dx[m, ci] = sum_t sum_co dYp[arow(m) + shift_t, co] * W[co, ci, tap_t]
// Exact work (no zero-stuffed transposed-conv upsampling; MIOpen's
// igemm_bwd path replaced — VERDICT r1 #4). Weights come repacked as
// wcat [Cin, 9*Cout], classes' tap slabs contiguous (conv.py
// _repack_w3_s2dgrad), col_base selecting the class.
template <int BM, int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(256, 2) void conv3x3s2_dgrad_kernel(
    const bf16* __restrict__ DYP, const bf16* __restrict__ B,
    bf16* __restrict__ DX, const int M, const int N, const int Cout,
    const int Wc, const int HWc, const int Hop, const int Wop, const int H,
    const int W, const int ph, const int pw, const int T, const int col_base,
    const int sh0, const int sh1, const int sh2, const int sh3) {
  constexpr int BK = 64;
  constexpr int A_BYTES = BM * BK * 2;
  constexpr int B_BYTES = BN * BK * 2;
  const int K = T * Cout;       // this class's gemm K
  const int Krow = 9 * Cout;    // B row stride (all classes)
  const int cb_per_t = Cout >> 6;
  char* lds = smem;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  const int tiles_n = N / BN;
  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int m0 = (bid / tiles_n) * BM;
  const int n0 = (bid % tiles_n) * BN;
  const int wm = (wave / WAVES_N) * 64;
  const int wn = (wave % WAVES_N) * 64;

  constexpr int A_CHUNKS = A_BYTES / 1024;
  constexpr int B_CHUNKS = B_BYTES / 1024;
  long long arow[A_CHUNKS / 4];
#pragma unroll
  for (int i = 0; i < A_CHUNKS / 4; ++i) {
    const int ch = wave * (A_CHUNKS / 4) + i;
    const int r = ch * 8 + (lane >> 3);
    long long m = m0 + r;
    if (m >= M) m = M - 1;  // clamped dup row; C-write guarded
    const int n_img = (int)(m / HWc);
    const int rem = (int)(m % HWc);
    const int i_r = rem / Wc;
    const int j_c = rem % Wc;
    arow[i] = (((long long)n_img * Hop + i_r) * Wop + j_c) * Cout;
  }
  const int shift_elems[4] = {sh0, sh1, sh2, sh3};

  auto stage = [&](int buf, int kt) {
    const int s = kt / cb_per_t;
    const int cb = kt % cb_per_t;
    char* abase = lds + buf * (A_BYTES + B_BYTES);
    char* bbase = abase + A_BYTES;
#pragma unroll
    for (int i = 0; i < A_CHUNKS / 4; ++i) {
      const int ch = wave * (A_CHUNKS / 4) + i;
      const int r = ch * 8 + (lane >> 3);
      const int gslot = (lane & 7) ^ (r & 7);
      const bf16* src = DYP + arow[i] + shift_elems[s] + cb * 64 + gslot * 8;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)(abase + ch * 1024), 16, 0, 0);
    }
    const int k0 = col_base + kt * BK;
#pragma unroll
    for (int i = 0; i < B_CHUNKS / 4; ++i) {
      const int ch = wave * (B_CHUNKS / 4) + i;
      const int r = ch * 8 + (lane >> 3);
      const int gslot = (lane & 7) ^ (r & 7);
      const bf16* src = B + (long long)(n0 + r) * Krow + k0 + gslot * 8;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)(bbase + ch * 1024), 16, 0, 0);
    }
  };

  auto read_a = [&](int buf, int mf, int kk) -> bf16x8 {
    const char* abase = lds + buf * (A_BYTES + B_BYTES);
    const int r = wm + mf * 16 + (lane & 15);
    const int c = kk * 4 + (lane >> 4);
    return *(const __attribute__((address_space(3))) bf16x8*)(
        (const __attribute__((address_space(3))) char*)(abase) + r * 128 +
        ((c ^ (r & 7)) << 4));
  };
  auto read_b = [&](int buf, int nf, int kk) -> bf16x8 {
    const char* bbase = lds + buf * (A_BYTES + B_BYTES) + A_BYTES;
    const int r = wn + nf * 16 + (lane & 15);
    const int c = kk * 4 + (lane >> 4);
    return *(const __attribute__((address_space(3))) bf16x8*)(
        (const __attribute__((address_space(3))) char*)(bbase) + r * 128 +
        ((c ^ (r & 7)) << 4));
  };

  f32x4 acc[4][4] = {};
  const int KT = K / BK;
  stage(0, 0);
  __syncthreads();
  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < KT) stage(cur ^ 1, kt + 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 a[4], b[4];
#pragma unroll
      for (int mf = 0; mf < 4; ++mf) a[mf] = read_a(cur, mf, kk);
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) b[nf] = read_b(cur, nf, kk);
#pragma unroll
      for (int mf = 0; mf < 4; ++mf)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
          acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[mf], b[nf], acc[mf][nf], 0, 0, 0);
    }
    __syncthreads();
  }

  const int cn = lane & 15;
  const int r4 = (lane >> 4) * 4;
#pragma unroll
  for (int mf = 0; mf < 4; ++mf) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int m = m0 + wm + mf * 16 + r4 + reg;
      if (m < M) {
        const int n_img = m / HWc;
        const int rem = m % HWc;
        const int h = 2 * (rem / Wc) + ph;
        const int w = 2 * (rem % Wc) + pw;
        bf16* crow = DX + (((long long)n_img * H + h) * W + w) * N + n0 + wn + cn;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
          crow[nf * 16] = __float2bfloat16(acc[mf][nf][reg]);
      }
    }
  }
}

extern "C" void launch_conv3x3s2_dgrad(const void* dyp, const void* wcat,
                                       void* dx, int Nimg, int H, int W,
                                       int Cin, int Cout, int Hop, int Wop,
                                       hipStream_t s) {
  // classes (ph,pw) with tap lists per the conv.py repack ordering
  const int col_base[4] = {0, Cout, 3 * Cout, 5 * Cout};
  const int dys[2][2] = {{1, 1}, {0, 2}};   // dys[ph][...]; ph=0 -> {1}
  const int ndy[2] = {1, 2};
  for (int ph = 0; ph < 2; ++ph) {
    for (int pw = 0; pw < 2; ++pw) {
      const int cls = ph * 2 + pw;
      const int Hc = (H - ph + 1) / 2, Wc = (W - pw + 1) / 2;
      const int M = Nimg * Hc * Wc;
      if (M <= 0) continue;
      int shifts[4] = {0, 0, 0, 0};
      int t = 0;
      for (int a = 0; a < ndy[ph]; ++a)
        for (int b = 0; b < ndy[pw]; ++b) {
          const int dy = dys[ph][a], dxx = dys[pw][b];
          const int r = (ph + 3 - dy) / 2, c = (pw + 3 - dxx) / 2;
          shifts[t++] = (r * Wop + c) * Cout;
        }
      const int T = t;
      if (Cin % 128 == 0) {
        constexpr int BM = 128, BN = 128;
        const int grid = ((M + BM - 1) / BM) * (Cin / BN);
        const int lds_bytes = 2 * (BM * 64 * 2 + BN * 64 * 2);
        hipLaunchKernelGGL((conv3x3s2_dgrad_kernel<BM, BN, 2, 2>), dim3(grid),
                           dim3(256), lds_bytes, s, (const bf16*)dyp,
                           (const bf16*)wcat, (bf16*)dx, M, Cin, Cout, Wc,
                           Hc * Wc, Hop, Wop, H, W, ph, pw, T, col_base[cls],
                           shifts[0], shifts[1], shifts[2], shifts[3]);
      } else {
        constexpr int BM = 256, BN = 64;
        const int grid = ((M + BM - 1) / BM) * (Cin / BN);
        const int lds_bytes = 2 * (BM * 64 * 2 + BN * 64 * 2);
        hipLaunchKernelGGL((conv3x3s2_dgrad_kernel<BM, BN, 4, 1>), dim3(grid),
                           dim3(256), lds_bytes, s, (const bf16*)dyp,
                           (const bf16*)wcat, (bf16*)dx, M, Cin, Cout, Wc,
                           Hc * Wc, Hop, Wop, H, W, ph, pw, T, col_base[cls],
                           shifts[0], shifts[1], shifts[2], shifts[3]);
      }
    }
  }
}

extern "C" void launch_pad_nhwc(const void* x, void* xp, int Nimg, int H, int W,
                                int Hp, int Wp, int C, hipStream_t s) {
  const long long per_img = (long long)Hp * Wp * (C >> 3);
  int gx = (int)((per_img + 255) / 256);
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(pad_nhwc_kernel, dim3(gx, Nimg), dim3(256), 0, s,
                     (const bf16*)x, (bf16*)xp, H * W, H, W, Hp, Wp, C);
}

extern "C" void launch_conv3x3_grouped(const void* xp, const void* w3g, void* y,
                                       int M, int Cout, int Cin, int HW_out,
                                       int W_out, int Hp, int Wp, int stride,
                                       int gw, hipStream_t s) {
  // BN = 64; w3g is [Cout, 9*gw] (gw = gemm group width: cpg when >= 64,
  // else 64 with a block-diagonal repack)
  constexpr int BM = 256, BN = 64;
  const int grid = ((M + BM - 1) / BM) * (Cout / BN);
  const int lds_bytes = 2 * (BM * 64 * 2 + BN * 64 * 2);
  hipLaunchKernelGGL((conv3x3_kernel<BM, BN, 4, 1, true>), dim3(grid),
                     dim3(256), lds_bytes, s, (const bf16*)xp, (const bf16*)w3g,
                     (bf16*)y, M, Cout, Cin, HW_out, W_out, Hp, Wp, stride, gw);
}

// launch_conv3x3_grouped with the eval BN(+ReLU) apply in the epilogue:
// y = bf16(relu?(fma(float(bf16(conv)), scale[c], shift[c]))), scale/shift
// fp32 [Cout]
extern "C" void launch_conv3x3_grouped_bn(const void* xp, const void* w3g,
                                          void* y, int M, int Cout, int Cin,
                                          int HW_out, int W_out, int Hp,
                                          int Wp, int stride, int gw,
                                          const float* scale,
                                          const float* shift, bool relu,
                                          hipStream_t s) {
  constexpr int BM = 256, BN = 64;
  const int grid = ((M + BM - 1) / BM) * (Cout / BN);
  const int lds_bytes = 2 * (BM * 64 * 2 + BN * 64 * 2);
  if (relu)
    hipLaunchKernelGGL((conv3x3_kernel<BM, BN, 4, 1, true, 2>), dim3(grid),
                       dim3(256), lds_bytes, s, (const bf16*)xp,
                       (const bf16*)w3g, (bf16*)y, M, Cout, Cin, HW_out, W_out,
                       Hp, Wp, stride, gw, nullptr, nullptr, scale, shift);
  else
    hipLaunchKernelGGL((conv3x3_kernel<BM, BN, 4, 1, true, 1>), dim3(grid),
                       dim3(256), lds_bytes, s, (const bf16*)xp,
                       (const bf16*)w3g, (bf16*)y, M, Cout, Cin, HW_out, W_out,
                       Hp, Wp, stride, gw, nullptr, nullptr, scale, shift);
}

extern "C" int conv3x3_pick_splitk(int M, int Cout, int Cin) {
  // split only CU-starved deep-K launches (stage 3/4 at bs32: 52-98
  // tiles, K 2304-4608); aim for ~384-512 total blocks
  const int bm = Cout % 128 == 0 ? 128 : 256;
  const int bn = bm == 128 ? 128 : 64;
  const int tiles = ((M + bm - 1) / bm) * (Cout / bn);
  const int KT = 9 * Cin / 64;
  if (tiles >= 224 || KT < 8) return 1;
  int sk = 384 / tiles;
  if (sk > KT / 4) sk = KT / 4;  // keep >= 4 k-steps per slice
  return sk < 1 ? 1 : sk;
}

extern "C" int conv3x3_tiles_m(int M, int Cout) {
  const int bm = Cout % 128 == 0 ? 128 : 256;
  return (M + bm - 1) / bm;
}

extern "C" void launch_conv3x3(const void* xp, const void* w3, void* y, int M,
                               int Cout, int Cin, int HW_out, int W_out, int Hp,
                               int Wp, int stride, float* cpart, int splitk,
                               float* bn_part, hipStream_t s) {
  if (splitk < 1) splitk = 1;
  if (cpart == nullptr) splitk = 1;
  if (splitk > 1) bn_part = nullptr;  // stats need the final values
  if (Cout % 128 == 0) {
    constexpr int BM = 128, BN = 128;
    const int grid = ((M + BM - 1) / BM) * (Cout / BN);
    const int lds_bytes = 2 * (BM * 64 * 2 + BN * 64 * 2);
    hipLaunchKernelGGL((conv3x3_kernel<BM, BN, 2, 2>), dim3(grid, splitk),
                       dim3(256), lds_bytes, s, (const bf16*)xp,
                       (const bf16*)w3, (bf16*)y, M, Cout, Cin, HW_out, W_out,
                       Hp, Wp, stride, 0, splitk > 1 ? cpart : nullptr,
                       bn_part);
  } else {
    constexpr int BM = 256, BN = 64;
    const int grid = ((M + BM - 1) / BM) * (Cout / BN);
    const int lds_bytes = 2 * (BM * 64 * 2 + BN * 64 * 2);
    hipLaunchKernelGGL((conv3x3_kernel<BM, BN, 4, 1>), dim3(grid, splitk),
                       dim3(256), lds_bytes, s, (const bf16*)xp,
                       (const bf16*)w3, (bf16*)y, M, Cout, Cin, HW_out, W_out,
                       Hp, Wp, stride, 0, splitk > 1 ? cpart : nullptr,
                       bn_part);
  }
}

// launch_conv3x3's non-split route with the eval BN(+ReLU) apply in the
// epilogue (see conv3x3_kernel AFF); the caller sends split-K shapes through
// launch_conv3x3 + cast + launch_bn_apply instead. scale/shift fp32 [Cout]
extern "C" void launch_conv3x3_bn(const void* xp, const void* w3, void* y,
                                  int M, int Cout, int Cin, int HW_out,
                                  int W_out, int Hp, int Wp, int stride,
                                  const float* scale, const float* shift,
                                  bool relu, hipStream_t s) {
#define CBN_CASE(BM, BN, WM, WN, AFF)                                         \
  hipLaunchKernelGGL((conv3x3_kernel<BM, BN, WM, WN, false, AFF>),            \
                     dim3(((M + BM - 1) / BM) * (Cout / BN)), dim3(256),      \
                     2 * (BM * 64 * 2 + BN * 64 * 2), s, (const bf16*)xp,     \
                     (const bf16*)w3, (bf16*)y, M, Cout, Cin, HW_out, W_out,  \
                     Hp, Wp, stride, 0, nullptr, nullptr, scale, shift)
  if (Cout % 128 == 0) {
    if (relu) CBN_CASE(128, 128, 2, 2, 2);
    else CBN_CASE(128, 128, 2, 2, 1);
  } else {
    if (relu) CBN_CASE(256, 64, 4, 1, 2);
    else CBN_CASE(256, 64, 4, 1, 1);
  }
#undef CBN_CASE
}
