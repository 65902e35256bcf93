// Weight gradient of the 7x7 stride-2 pad-3 stem conv (conv7x7.hip), Cin <= 4
// -> 64 channels, on the forward's padded input xp [N, Hp, Wp, 4]:
//
//   dW7[co, ky, kxs, c] = sum_{n,oy,ox} dy[n,oy,ox,co] * xp[n, 2oy+ky, 2ox+kxs, c]
//
// a GEMM with a 64 x 224 output (224 = 7 ky x 8 kxs x 4 c, the layout of
// conv.py _repack_w7) whose reduction runs over every output pixel. Both
// operands are k-major in memory (a pixel is the slow index of dy and of xp),
// so every MFMA fragment is a TRANSPOSED read; the kx = 7 slot and the
// channels >= Cin are computed and dropped by the fold.
//
// Work split. One tile = 16 x 16 output pixels of one image, 256 threads, the
// forward's tiles, patch (37 rows x 19 slots) and persistent walk (tiles
// t = b, b + grid, ... in xcd_swizzle order). A block keeps the WHOLE 64 x 224
// result in registers across its tiles: wave w owns co rows 32*(w>>1) ..
// +31 (two 16-row M tiles) and the 7 column tiles (ky, kxs half w&1), i.e.
// 2 x 7 f32x4 accumulators per lane. (One wave per 16 co rows and all 14
// column tiles has the same accumulators but re-reads every B fragment in all
// four waves.) A tile is 8 k-steps of
// 32 pixels = two output rows x 16 ox; MFMA k-group g = lane >> 4 is row
// g >> 1, ox half g & 1, and its 8 k values are ox 8(g&1) .. +7. The B
// fragment of (ks, ky) is patch row 4ks + ky, so three of the seven of a
// k-step are the previous step's ky + 4 and stay in registers. Per tile and
// wave: 112 MFMAs, 32 + 70 ds_read_b64_tr_b16.
//
// Fragments. ds_read_b64_tr_b16 works on 16 lanes: lanes 4e .. 4e+3 supply
// the 16 values of row e (8 bytes each, any address), and lane i receives
// element i of rows 0..3. One read is therefore 4 k values (pixels) x 16 rows
// or columns, and a bf16x8 operand is two reads (r = 0, 1: ox + 4r):
//   A (dY^T, row = co):  lane 4e+q reads co 4q..4q+3 of pixel
//      p = 32ks + 8g + 4r + e of the slab: 8 bytes of its 128-byte row.
//   B (patch, column = (kxs, c)): lane 4e+q reads ALL FOUR channels of patch
//      pixel 2*ox + 4h + q in row 2*oy + ky: a padded pixel is exactly one
//      aligned 8-byte row, so the stride-2 gather costs nothing.
// Both use the same (g, r, e) -> pixel map, which is all the MFMA needs of k.
//
// LDS images (dynamic, 2 x 44032 B, double buffered, global_load_lds 16 B per
// lane with the linear destination of the forward: a lane derives its source
// from its destination unit):
//   patch  37 rows x 19 slots (+1), 11264 B, linear, exactly the forward's.
//   slab   256 pixels x 64 co of dY, 32768 B; pixel p's row of 128 B holds
//          its four 32-byte granules (16 co each) at granule ^ f(p),
//          f(p) = ((p >> 1) & 1) | (((p >> 3) & 1) << 1).
// Bank argument (64 banks x 4 B: LDS words repeat every 256 B; a
// ds_read_b64 moves 512 B and is served as lanes 0..31, then 32..63):
//   A: the 32 lanes of a half read pixels 8g + 4r + e for g in {2a, 2a+1},
//      e = 0..3, each lane 8 bytes at q*8 inside ONE granule. Unswizzled,
//      pixel rows are 128 B apart: the eight pixels fall on two 128-byte
//      phases and the same 32 bytes of each, 4-way. With the swizzle the
//      phase is p & 1 = e & 1 and the granule is mt ^ (e >> 1 | (g & 1) << 1):
//      (e & 1, e >> 1, g & 1) are eight distinct (phase, granule) pairs, 8 x
//      32 = 256 distinct bytes, conflict-free.
//   B: a half has g in {2a, 2a+1}: ONE patch row (row depends on g >> 1) and
//      pixels 16(g&1) + 8r + 4h + 2e + q. For one g that is 10 distinct
//      consecutive pixels, 80 B (lanes that share a pixel read the same
//      words: a broadcast); the two g are 128 B apart: [0, 80) and
//      [128, 208), conflict-free whatever the 304-byte row stride. The other
//      half sits two rows (608 B = 96 mod 256) further and would collide
//      with this one 2-way; it is a pass of its own.
//
// Tails. Tiles overhang Ho and Wo. A clamped duplicate of a dY row would be
// ADDED into the sum, so the slab stages pixels with oy >= Ho or ox >= Wo as
// zeros: the lanes of a chunk that are in range issue the global_load_lds,
// the others write 16 zero bytes to the same linear destination. The patch
// stays clamped as in the forward (finite * 0).
//
// Partials. No atomics: block b dumps its accumulators as row b of part
// [grid, 64*224] fp32, accumulator a = (wave*14 + m*7 + ky) at floats
// (a*64 + lane)*4 .. +3 (1 KB per wave and store, coalesced). Every row is
// written on every launch: no fill launch, graph-replay safe.
// conv7x7s2_wgrad_fold_kernel adds the rows in a fixed order (bit-identical
// from run to run), decodes the dump and writes dW [64, Cin, 7, 7].
#include "common.h"
#include "launchers.h"

using bf16 = __hip_bfloat16;
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

extern __shared__ __attribute__((aligned(16))) char smem[];

namespace {

constexpr int kTile = 16;
constexpr int kPatchRows = 2 * kTile + 5;                 // 37
constexpr int kPatchSlots = kTile + 3;                    // 19
constexpr int kPatchN = kPatchRows * kPatchSlots;         // 703 slots
constexpr int kPatchChunks = (kPatchN + 63) / 64;         // 11 x 1 KB
constexpr int kPatchBytes = kPatchChunks * 1024;
constexpr int kPatchRowBytes = kPatchSlots * 16;          // 304
constexpr int kSlabChunks = kTile * kTile * 128 / 1024;   // 32 x 1 KB
constexpr int kSlabBytes = kSlabChunks * 1024;
constexpr int kBufBytes = kPatchBytes + kSlabBytes;
constexpr int kLdsBytes = 2 * kBufBytes;                  // 88064: 1 block/CU
constexpr int kPartRow = 64 * 224;                        // floats per block
// default cap of the persistent grid: one block per CU, all the LDS allows.
// Measured (docs/kernels.md, wgrad per-shape table): caps of 64 / 128 / 192
// are slower at batch 16 and 32; the partial rows cost less than the idle CUs.
constexpr int kWgradDefaultBlocks = 256;
constexpr int kFoldCols = 16;   // f32x4 columns per fold block
constexpr int kFoldRows = 16;   // row groups per fold block

using lds_char = __attribute__((address_space(3))) char;

__device__ __forceinline__ void load16_to_lds(const char* src, char* dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)src,
      (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

// one bf16x8 operand: two transposed reads, the second `step` bytes on
__device__ __forceinline__ bf16x8 tr_read8(const lds_char* p, int step) {
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4*)p);
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4*)(p + step));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

}  // namespace

__global__ __launch_bounds__(256, 1) void conv7x7s2_wgrad_kernel(
    const bf16* __restrict__ XP, const bf16* __restrict__ DY,
    float* __restrict__ part, const int Ho, const int Wo, const int Hp,
    const int Sp, const int tiles_x, const int tiles_y, const int tiles) {
  char* lds = smem;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane >> 4;
  const int e = (lane >> 2) & 3;
  const int q = lane & 3;
  const int tiles_img = tiles_x * tiles_y;

  // patch: the (row, slot) each of this lane's chunks fills, as the forward
  int prow[3], pslot[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    int p = (wave + 4 * i) * 64 + lane;
    if (p > kPatchN - 1) p = kPatchN - 1;
    prow[i] = p / kPatchSlots;
    pslot[i] = p % kPatchSlots;
  }
  // slab: chunk ch = wave + 4i holds pixels 8ch .. 8ch+7, lane l the 16-byte
  // unit l & 7 of pixel p = 8ch + (l >> 3): tile row ch >> 1 = (wave >> 1) +
  // 2i, tile column 8(wave & 1) + (l >> 3), fixed across i. The unit holds
  // SOURCE unit (granule ^ f(p)), f(p) = (l >> 4 & 1) | (wave & 1) << 1.
  const int stx = 8 * (wave & 1) + (lane >> 3);
  const int sf = ((lane >> 4) & 1) | ((wave & 1) << 1);
  const int ssrc = stx * 128 + (((((lane & 7) >> 1) ^ sf) << 1) | (lane & 1)) * 16;

  auto stage = [&](int buf, int t) {
    const int tile = xcd_swizzle(t, tiles);
    const int n = tile / tiles_img;
    const int rem = tile % tiles_img;
    const int oy0 = (rem / tiles_x) * kTile;
    const int ox0 = (rem % tiles_x) * kTile;
    char* pbase = lds + buf * kBufBytes;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int ch = wave + 4 * i;  // wave-uniform
      if (ch < kPatchChunks) {
        int r = 2 * oy0 + prow[i];
        if (r > Hp - 1) r = Hp - 1;  // overhang: clamped, times a zero of dY
        int s = ox0 + pslot[i];
        if (s > Sp - 1) s = Sp - 1;
        const char* src = (const char*)XP +
                          (((long long)n * Hp + r) * Sp + s) * 16;
        load16_to_lds(src, pbase + ch * 1024);
      }
    }
    char* sbase = pbase + kPatchBytes;
    const bool xin = ox0 + stx < Wo;
#pragma unroll
    for (int i = 0; i < kSlabChunks / 4; ++i) {
      const int ch = wave + 4 * i;  // wave-uniform
      const int oy = oy0 + (wave >> 1) + 2 * i;
      char* dst = sbase + ch * 1024;
      if (xin && oy < Ho) {
        const char* src = (const char*)DY +
                          (((long long)n * Ho + oy) * Wo + ox0) * 128 + ssrc;
        load16_to_lds(src, dst);
      } else {
        *(__attribute__((address_space(3))) f32x4*)((lds_char*)dst +
                                                    lane * 16) = f32x4{};
      }
    }
  };

  stage(0, blockIdx.x);

  // fragment bases of this lane (bytes inside one buffer)
  const int mh = wave >> 1, h = wave & 1;
  const int af = (e >> 1) | ((g & 1) << 1);
  unsigned a_off[2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
    a_off[m] = kPatchBytes + (8 * g + e) * 128 + (((2 * mh + m) ^ af) << 5) +
               q * 8;
  const unsigned b_off = 2 * (g >> 1) * kPatchRowBytes +
                         (16 * (g & 1) + 2 * e + 4 * h + q) * 8;

  f32x4 acc[2][7] = {};
  __syncthreads();

  int buf = 0;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    if (t + (int)gridDim.x < tiles) stage(buf ^ 1, t + gridDim.x);

    const lds_char* base = (const lds_char*)lds + buf * kBufBytes;
    // B fragment (ks, ky) is patch row 4ks + ky (+ the lane's 2(g >> 1)):
    // (ks + 1, ky) is (ks, ky + 4) for ky < 3, so a k-step reads only the 4
    // new rows (35 fragments per tile, not 56), and it reads them, with the
    // next A pair, ahead of the current k-step's MFMAs.
    bf16x8 a[2], b[7];
#pragma unroll
    for (int m = 0; m < 2; ++m) a[m] = tr_read8(base + a_off[m], 512);
#pragma unroll
    for (int ky = 0; ky < 7; ++ky)
      b[ky] = tr_read8(base + b_off + ky * kPatchRowBytes, 64);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      bf16x8 an[2], bn[4];
      if (ks < 7) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
          an[m] = tr_read8(base + a_off[m] + (ks + 1) * 4096, 512);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          bn[j] = tr_read8(
              base + b_off + (4 * ks + 7 + j) * kPatchRowBytes, 64);
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int ky = 0; ky < 7; ++ky)
          acc[m][ky] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[m], b[ky], acc[m][ky], 0, 0, 0);
      if (ks < 7) {
#pragma unroll
        for (int m = 0; m < 2; ++m) a[m] = an[m];
#pragma unroll
        for (int j = 0; j < 3; ++j) b[j] = b[j + 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[3 + j] = bn[j];
      }
    }
    // the next tile has landed; nobody reads this buffer any more
    __syncthreads();
    buf ^= 1;
  }

  f32x4* prow4 = reinterpret_cast<f32x4*>(
      part + (long long)blockIdx.x * kPartRow) + wave * 14 * 64 + lane;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) prow4[(m * 7 + ky) * 64] = acc[m][ky];
}

// part [rows, 64*224] -> dW [64, Cin, 7, 7]. A block takes kFoldCols f32x4
// columns of the dump; row group rg adds rows rg, rg + 16, ... in order, then
// thread (0, col) adds the 16 group sums in order: one fixed tree, the same
// bits every run. f32x4 v of the dump is lane v & 63 of accumulator v >> 6:
// D map col = lane & 15 -> (kxs, c), row = (lane >> 4)*4 + reg -> co.
__global__ __launch_bounds__(256) void conv7x7s2_wgrad_fold_kernel(
    const float* __restrict__ part, float* __restrict__ dW, const int rows,
    const int Cin) {
  __shared__ f32x4 red[kFoldRows][kFoldCols];
  const int cl = threadIdx.x % kFoldCols;
  const int rg = threadIdx.x / kFoldCols;
  const int v = blockIdx.x * kFoldCols + cl;  // < 64*224/4, exact grid
  const int lane = v & 63, a = v >> 6;
  const int wave = a / 14, m = (a % 14) / 7, ky = a % 7;
  const int kxs = 4 * (wave & 1) + ((lane & 15) >> 2), c = lane & 3;
  const bool keep = kxs < 7 && c < Cin;
  f32x4 s = {};
  if (keep) {
    const f32x4* src = reinterpret_cast<const f32x4*>(part) + v;
    for (int r = rg; r < rows; r += kFoldRows)
      s += src[(long long)r * (kPartRow / 4)];
  }
  red[rg][cl] = s;
  __syncthreads();
  if (rg == 0 && keep) {
#pragma unroll
    for (int r = 1; r < kFoldRows; ++r) s += red[r][cl];
    const int co = 16 * (2 * (wave >> 1) + m) + 4 * (lane >> 4);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      dW[(((co + reg) * Cin + c) * 7 + ky) * 7 + kxs] = s[reg];
  }
}

extern "C" int conv7x7s2_wgrad_grid(int tiles, int max_blocks) {
  const int cap = max_blocks > 0 && max_blocks < kWgradDefaultBlocks
                      ? max_blocks
                      : kWgradDefaultBlocks;
  const int rounds = (tiles + cap - 1) / cap;
  return rounds == 0 ? 0 : (tiles + rounds - 1) / rounds;
}

extern "C" void launch_conv7x7s2_wgrad(const void* xp, const void* dy,
                                       float* part, float* dw, int Nimg,
                                       int H, int W, int Cin, int max_blocks,
                                       hipStream_t s) {
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int tiles_x = (Wo + kTile - 1) / kTile;
  const int tiles_y = (Ho + kTile - 1) / kTile;
  const int tiles = Nimg * tiles_x * tiles_y;
  const int grid = conv7x7s2_wgrad_grid(tiles, max_blocks);
  if (grid > 0)
    hipLaunchKernelGGL(conv7x7s2_wgrad_kernel, dim3(grid), dim3(256),
                       kLdsBytes, s, (const bf16*)xp, (const bf16*)dy, part,
                       Ho, Wo, 2 * Ho + 5, Wo + 3, tiles_x, tiles_y, tiles);
  // rows == 0 (an empty batch): the fold writes zeros
  hipLaunchKernelGGL(conv7x7s2_wgrad_fold_kernel,
                     dim3(kPartRow / 4 / kFoldCols), dim3(256), 0, s, part,
                     dw, grid, Cin);
}
