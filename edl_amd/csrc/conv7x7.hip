// 7x7 stride-2 pad-3 stem convolution, Cin <= 4 -> 64 channels (the ResNeXt
// teacher's conv1), as an implicit GEMM on NHWC bf16 with the eval-mode
// BN(+ReLU) apply in the epilogue. Forward only: the input is the image.
//
//   y[M, 64] = A[M, 224] @ W7[64, 224]^T,   M = N*Ho*Wo,   K = 7 rows x 32
//
// The input is first written into xp [N, Hp, Wp, 4] (pad_stem7_kernel:
// channels padded to 4, zero halo, interior at (3, 3), Hp = 2*Ho + 5,
// Wp = 2*Wo + 6). A pixel is then 8 bytes and a 16-byte SLOT is two pixels.
// With stride 2, output pixel (oy, ox) and filter row ky read the 8 pixels
// 2*ox .. 2*ox+7 of padded row 2*oy + ky: the 64 contiguous bytes that
// start at slot ox. That is one k-step of v_mfma_f32_16x16x32_bf16 (8 kx
// slots x 4 channels; kx = 7 and the channels >= Cin carry zero weights:
// 147 real products of 224), and the A fragment of a lane (row = lane & 15,
// k-group g = lane >> 4) is the single aligned slot ox + g. No im2col image
// exists anywhere: a block copies the input patch of its output tile into
// LDS linearly, and every fragment is one ds_read_b128 from it.
//
// Work split. One tile = 16 x 16 output pixels of one image, 256 threads,
// 4 waves. An M-fragment is 16 consecutive ox of ONE output row; wave w owns
// rows 4w .. 4w+3: 4 M-fragments x 4 N-fragments = 16 f32x4 accumulators,
// 7 k-steps, 112 MFMAs per tile and wave. Blocks are persistent: the grid is
// capped (launch_conv7x7s2) and each block walks tiles t = b, b + grid, ...
// in xcd_swizzle order, so W7 is staged once per block, not once per tile.
//
// LDS images (dynamic, 52224 B):
//   W7   64 rows x 29 slots (28 data + 1 pad)            29696 B
//   patch, double buffered: 37 rows x 19 slots (+1)    2 x 11264 B
// Both are filled with global_load_lds, 16 B per lane, which writes lane l
// of a chunk at chunk base + 16*l: the DESTINATION is linear, so each lane
// derives its source from its destination slot (row = q / stride,
// col = q % stride); the W7 pad column and the one slot past the patch
// re-read a neighbour and are never read back.
// Bank argument (a ds_read_b128 is served in groups of lanes that are
// consecutive within one 16-lane quarter; LDS words repeat every 256 B):
//   B: the 16 lanes of a quarter read the same slot column of 16
//      consecutive rows. Unpadded rows are 28 slots = 448 B apart, i.e.
//      192 B mod 256: rows r and r+4 collide, 4-way. With 29 slots the row
//      offsets are 29*r mod 16 = 13*r mod 16 slots, a permutation of 0..15
//      (13 is odd): 16 distinct 16-byte columns, conflict-free.
//   A: the 16 lanes of a quarter read 16 CONSECUTIVE slots of one patch row
//      (slot ox_l + g): 256 contiguous bytes, conflict-free whatever the
//      row stride. The 19-slot stride never enters a fragment, because a
//      fragment never straddles rows. The four quarters overlap in 13 of
//      their slots and are served one after another.
// The next tile's patch is in flight under the current tile's MFMAs; one
// __syncthreads per tile both publishes it and retires the buffer just read.
//
// Tails. Tiles overhang Ho and Wo; the patch copy clamps the SOURCE row and
// slot to the last valid one, the products are computed and the stores are
// guarded on oy < Ho && ox < Wo. Every read of a stored output is in range
// unclamped: row 2*oy + ky <= 2*(Ho-1) + 6 = Hp - 1 and slot
// ox + g <= Wo + 2 = Wp/2 - 1. The image index is part of the tile index.
//
// AFF (0 = off, 1 = affine, 2 = affine + ReLU), exactly conv3x3_kernel's:
//   y = bf16(relu?(fmaf(float(bf16(acc)), scale[c], shift[c])))
// The accumulator is rounded first, so the result is the plain kernel
// followed by bnrelu.hip's bn_apply_kernel bit for bit.
#include "common.h"
#include "launchers.h"

using bf16 = __hip_bfloat16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

extern __shared__ __attribute__((aligned(16))) char smem[];

namespace {

constexpr int kTile = 16;                        // output tile edge
constexpr int kPatchRows = 2 * kTile + 5;        // 37
constexpr int kPatchSlots = kTile + 3;           // 19
constexpr int kPatchN = kPatchRows * kPatchSlots;         // 703 slots
constexpr int kPatchChunks = (kPatchN + 63) / 64;         // 11 x 1 KB
constexpr int kPatchBytes = kPatchChunks * 1024;
constexpr int kWSlots = 28;                      // 224 bf16 = 28 slots
constexpr int kWStride = 29;                     // + 1 pad slot per row
constexpr int kWChunks = 64 * kWStride / 64;     // 29 x 1 KB, exact
constexpr int kWBytes = kWChunks * 1024;
constexpr int kLdsBytes = kWBytes + 2 * kPatchBytes;
// persistent grid: 256 CUs x 2 resident blocks (LDS: 2 x 51 KB of 160 KB)
constexpr int kMaxBlocks = 256 * 2;

__device__ __forceinline__ void load16_to_lds(const char* src, char* dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)src,
      (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

__device__ __forceinline__ bf16x8 lds_read16(const char* p) {
  return *(const __attribute__((address_space(3))) bf16x8*)(
      (const __attribute__((address_space(3))) char*)p);
}

}  // namespace

// x [N, H, W, Cin] -> xp [N, Hp, Sp slots of 2 pixels x 4 channels] with a
// zero border of `halo` pixels above and to the left (3 here, 1 for the 3x3
// stem wgrad, conv3x3_small_wgrad.hip). One
// thread builds one slot in registers and stores it whole (16 B; see the
// note in pad_nhwc_cpad_kernel on per-channel store loops). Halo, channels
// >= Cin and the extra row / column of an odd H / W are zeros written here
// on every launch: there is no fill launch to replay.
extern "C" __global__ void pad_stem7_kernel(
    const bf16* __restrict__ x, bf16* __restrict__ xp, const int H,
    const int W, const int Hp, const int Sp, const int Cin, const int halo,
    const long long total) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int s = (int)(i % Sp);
    const long long rest = i / Sp;
    const int hp = (int)(rest % Hp);
    const long long n = rest / Hp;
    const int h = hp - halo;
    uint4 raw = {0, 0, 0, 0};
    ushort* u = reinterpret_cast<ushort*>(&raw);
    if (h >= 0 && h < H) {
#pragma unroll
      for (int px = 0; px < 2; ++px) {
        const int w = 2 * s + px - halo;
        if (w >= 0 && w < W) {
          const bf16* src = x + ((n * H + h) * W + w) * Cin;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (c < Cin) u[px * 4 + c] = __hip_bfloat16_raw(src[c]).x;
        }
      }
    }
    *reinterpret_cast<uint4*>(__builtin_assume_aligned(xp + i * 8, 16)) = raw;
  }
}

template <int AFF>
__global__ __launch_bounds__(256, 2) void conv7x7s2_kernel(
    const bf16* __restrict__ XP, const bf16* __restrict__ W7,
    bf16* __restrict__ Y, const int Ho, const int Wo, const int Hp,
    const int Sp, const int tiles_x, const int tiles_y, const int tiles,
    const float* __restrict__ bn_scale, const float* __restrict__ bn_shift) {
  char* lds = smem;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l15 = lane & 15;
  const int g = lane >> 4;
  const int tiles_img = tiles_x * tiles_y;

  // the (row, slot) of the patch each of this lane's chunks fills: fixed
  // across tiles. Slot 703 (the last lane of chunk 10) re-reads slot 702.
  int prow[3], pslot[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    int p = (wave + 4 * i) * 64 + lane;
    if (p > kPatchN - 1) p = kPatchN - 1;
    prow[i] = p / kPatchSlots;
    pslot[i] = p % kPatchSlots;
  }

  auto stage_patch = [&](int buf, int t) {
    const int tile = xcd_swizzle(t, tiles);
    const int n = tile / tiles_img;
    const int rem = tile % tiles_img;
    const int oy0 = (rem / tiles_x) * kTile;
    const int ox0 = (rem % tiles_x) * kTile;
    char* pbase = lds + kWBytes + buf * kPatchBytes;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int ch = wave + 4 * i;  // wave-uniform
      if (ch < kPatchChunks) {
        int r = 2 * oy0 + prow[i];
        if (r > Hp - 1) r = Hp - 1;  // overhang: clamped source, unstored
        int s = ox0 + pslot[i];
        if (s > Sp - 1) s = Sp - 1;
        const char* src = (const char*)XP +
                          (((long long)n * Hp + r) * Sp + s) * 16;
        load16_to_lds(src, pbase + ch * 1024);
      }
    }
  };

  // W7 -> LDS rows of 29 slots, once per block
#pragma unroll
  for (int i = 0; i < (kWChunks + 3) / 4; ++i) {
    const int ch = wave + 4 * i;  // wave-uniform
    if (ch < kWChunks) {
      const int q = ch * 64 + lane;
      const int row = q / kWStride;
      int col = q % kWStride;
      if (col > kWSlots - 1) col = kWSlots - 1;  // pad slot: never read
      load16_to_lds((const char*)W7 + (row * kWSlots + col) * 16,
                    lds + ch * 1024);
    }
  }
  stage_patch(0, blockIdx.x);

  // AFF: the lane's 4 + 4 scale/shift values (channels nf*16 + (lane & 15)),
  // loaded once, ahead of the tile loop
  float aff_sc[4], aff_sh[4];
  if constexpr (AFF != 0) {
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      aff_sc[nf] = bn_scale[nf * 16 + l15];
      aff_sh[nf] = bn_shift[nf * 16 + l15];
    }
  }
  __syncthreads();

  int buf = 0;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    if (t + (int)gridDim.x < tiles) stage_patch(buf ^ 1, t + gridDim.x);

    const int tile = xcd_swizzle(t, tiles);
    const int n = tile / tiles_img;
    const int rem = tile % tiles_img;
    const int oy0 = (rem / tiles_x) * kTile;
    const int ox0 = (rem % tiles_x) * kTile;

    const char* wb = lds + (l15 * kWStride + g) * 16;
    const char* pb = lds + kWBytes + buf * kPatchBytes +
                     (8 * wave * kPatchSlots + l15 + g) * 16;
    f32x4 acc[4][4] = {};
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) {
      bf16x8 a[4], b[4];
#pragma unroll
      for (int nf = 0; nf < 4; ++nf)
        b[nf] = lds_read16(wb + (nf * 16 * kWStride + ky * 4) * 16);
#pragma unroll
      for (int mf = 0; mf < 4; ++mf)
        a[mf] = lds_read16(pb + (2 * mf + ky) * kPatchSlots * 16);
#pragma unroll
      for (int mf = 0; mf < 4; ++mf)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
          acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[mf], b[nf], acc[mf][nf], 0, 0, 0);
    }

    // C/D map: col = lane & 15 -> channel, row = (lane >> 4)*4 + reg -> ox
    const int r4 = g * 4;
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) {
      const int oy = oy0 + 4 * wave + mf;
      if (oy < Ho) {
        bf16* yrow = Y + ((long long)n * Ho + oy) * Wo * 64 + l15;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int ox = ox0 + r4 + reg;
          if (ox < Wo) {
            bf16* c = yrow + (long long)ox * 64;
#pragma unroll
            for (int nf = 0; nf < 4; ++nf) {
              const bf16 yb = __float2bfloat16(acc[mf][nf][reg]);
              if constexpr (AFF == 0) {
                c[nf * 16] = yb;
              } else {
                float v = fmaf(__bfloat162float(yb), aff_sc[nf], aff_sh[nf]);
                if constexpr (AFF == 2) v = fmaxf(v, 0.0f);
                c[nf * 16] = __float2bfloat16(v);
              }
            }
          }
        }
      }
    }
    // the next patch has landed; nobody reads this one any more
    __syncthreads();
    buf ^= 1;
  }
}

extern "C" void launch_pad_c4(const void* x, void* xp, int Nimg, int H, int W,
                              int Cin, int halo, int Hp, int Sp,
                              hipStream_t s) {
  const long long total = (long long)Nimg * Hp * Sp;
  hipLaunchKernelGGL(pad_stem7_kernel, dim3(elementwise_grid(total, 256)),
                     dim3(256), 0, s, (const bf16*)x, (bf16*)xp, H, W, Hp, Sp,
                     Cin, halo, total);
}

extern "C" void launch_pad_stem7(const void* x, void* xp, int Nimg, int H,
                                 int W, int Cin, hipStream_t s) {
  const int Hp = 2 * ((H - 1) / 2 + 1) + 5;
  const int Sp = (W - 1) / 2 + 1 + 3;  // Wp / 2
  launch_pad_c4(x, xp, Nimg, H, W, Cin, 3, Hp, Sp, s);
}

extern "C" int conv7x7s2_tiles(int Nimg, int H, int W) {
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  return Nimg * ((Ho + kTile - 1) / kTile) * ((Wo + kTile - 1) / kTile);
}

// The grid: every block gets the same number of tiles (+-1). With `rounds`
// = ceil(tiles / cap) passes needed anyway, ceil(tiles / rounds) blocks
// finish together instead of a full grid whose first blocks run one more.
extern "C" int conv7x7s2_grid(int tiles, int max_blocks) {
  const int cap = max_blocks > 0 && max_blocks < kMaxBlocks ? max_blocks
                                                            : kMaxBlocks;
  const int rounds = (tiles + cap - 1) / cap;
  return (tiles + rounds - 1) / rounds;
}

template <int AFF>
static void conv7x7s2_run(const void* xp, const void* w7, void* y, int Nimg,
                          int H, int W, const float* scale,
                          const float* shift, int max_blocks, hipStream_t s) {
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int tiles_x = (Wo + kTile - 1) / kTile;
  const int tiles_y = (Ho + kTile - 1) / kTile;
  const int tiles = conv7x7s2_tiles(Nimg, H, W);
  if (tiles == 0) return;
  hipLaunchKernelGGL((conv7x7s2_kernel<AFF>),
                     dim3(conv7x7s2_grid(tiles, max_blocks)), dim3(256),
                     kLdsBytes, s, (const bf16*)xp, (const bf16*)w7, (bf16*)y,
                     Ho, Wo, 2 * Ho + 5, Wo + 3, tiles_x, tiles_y, tiles,
                     scale, shift);
}

extern "C" void launch_conv7x7s2(const void* xp, const void* w7, void* y,
                                 int Nimg, int H, int W, int max_blocks,
                                 hipStream_t s) {
  conv7x7s2_run<0>(xp, w7, y, Nimg, H, W, nullptr, nullptr, max_blocks, s);
}

extern "C" void launch_conv7x7s2_bn(const void* xp, const void* w7, void* y,
                                    int Nimg, int H, int W,
                                    const float* scale, const float* shift,
                                    bool relu, int max_blocks,
                                    hipStream_t s) {
  if (relu)
    conv7x7s2_run<2>(xp, w7, y, Nimg, H, W, scale, shift, max_blocks, s);
  else
    conv7x7s2_run<1>(xp, w7, y, Nimg, H, W, scale, shift, max_blocks, s);
}
