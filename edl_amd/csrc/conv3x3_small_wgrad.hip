// Weight gradient of the small-channel 3x3 pad-1 stem convs (conv3x3.hip
// conv3x3_small), on a zero-halo padded input xp:
//
//   dW[co, ky, kx, c] = sum_{n,oy,ox} dy[n,oy,ox,co] * xp[n, s*oy+ky, s*ox+kx, c]
//
// fp32 accumulation, fp32 result [Cout, Cin, 3, 3]. Two classes, no others:
//   narrow  Cin <= 4, stride 2, Cout 32 | 64: xp [N, 2Ho+1, 2Wo+2, 4] (the
//           pad_stem7_kernel layout with a halo of 1: a pixel is one aligned
//           8-byte row). Output Cout x 48 columns: column tile ky = 4 kx
//           slots x 4 channels; the kx = 3 slot and the channels >= Cin are
//           computed and dropped by the fold.
//   wide    Cin = 32, stride 1, Cout 32 | 64: xp [N, H+2, W+2, 32]
//           (pad_nhwc). Output Cout x 288 columns: column tile (tap, channel
//           half) = 16 channels of one tap, 18 tiles.
// Both operands are k-major in memory (a pixel is the slow index of dy and of
// xp), so every MFMA (v_mfma_f32_16x16x32_bf16, k = 32 output pixels)
// fragment is a pair of TRANSPOSED reads (ds_read_b64_tr_b16).
//
// Work split. One tile = 16 x 16 output pixels of one image, 256 threads,
// persistent walk (tiles t = b, b + grid, ... in xcd_swizzle order); a block
// keeps the WHOLE dW in MFMA accumulators across its tiles. A tile is 8
// k-steps of 32 pixels = two output rows x 16 ox; k-group g = lane >> 4 is
// row g >> 1, ox half g & 1, its 8 k values are ox 8(g&1) .. +7.
//   wide:   wave w owns co half w >> 1 (Cout/32 M tiles) and channel half
//           w & 1 of all 9 taps: Cout/32 x 9 f32x4 accumulators per lane, and
//           every A and B fragment is read by two waves, not four. B fragment
//           (ks, ky, kx) covers patch rows 2ks + ky (+ g >> 1), so (ks+1, 0,
//           kx) IS (ks, 2, kx) and stays in registers: 6 new fragments per
//           k-step, not 9. Per tile and wave (Cout 64): 144 MFMAs, 32 + 102
//           ds_read_b64_tr_b16.
//   narrow: only Cout/16 x 3 accumulator tiles, so the waves split the
//           k-steps instead (wave w takes ks = w and w + 4, all M tiles, all
//           three ky): no fragment is read twice at all. The four waves'
//           sums meet in LDS once per block, after the last tile, and are
//           added in the fixed order wave 0, 1, 2, 3.
//
// Fragments. ds_read_b64_tr_b16 works on 16 lanes: lanes 4e .. 4e+3 supply
// the 16 values of row e (8 bytes each, any address), and lane i receives
// element i of rows 0..3. A bf16x8 operand is two reads (r = 0, 1: ox + 4r):
//   A (dY^T, row = co): lane 4e+q reads co 4q..4q+3 of M tile mt of slab
//      pixel p = 32ks + 8g + 4r + e: 8 bytes of its Cout*2-byte row.
//   B narrow (column = (kx slot, c)): lane 4e+q reads ALL FOUR channels of
//      patch pixel 2*ox + q in row 2*oy + ky: the stride-2 gather is free.
//   B wide (column = channel 16*half + i): lane 4e+q reads channels
//      16*half + 4q .. +3 of patch pixel (oy + ky, ox + kx).
// A and B use the same (g, r, e) -> pixel map, which is all the MFMA needs.
//
// LDS images (dynamic, double buffered, global_load_lds 16 B per lane with a
// linear destination: a lane derives its source from its destination unit):
//   slab   256 pixels x Cout of dY in its native [M, Cout] rows, 16 | 32 KB.
//          Pixel p's 32-byte granules (16 co each) sit at granule ^ f(p):
//          Cout 64 (128-byte rows): f = ((p >> 1) & 1) | (((p >> 3) & 1) << 1),
//          Cout 32 (64-byte rows):  f = (p >> 3) & 1.
//   patch  narrow: 33 rows x 17 slots of 2 pixels, 9216 B, linear.
//          wide: 18 x 18 pixels x 64 B, 21504 B; the two 32-byte granules
//          (channel halves) of patch column pc sit at granule ^ ((pc >> 3) & 1).
//   Buffers: narrow 25600 | 41984 B, wide 37888 | 54272 B, twice: one block
//   per CU by LDS for all but narrow Cout 32.
// Bank argument (64 banks x 4 B: LDS words repeat every 256 B; a
// ds_read_b64 moves 512 B and is served as lanes 0..31, then 32..63; a half
// has g in {2a, 2a+1}, e = 0..3, q = 0..3):
//   A, Cout 64: as conv7x7_wgrad.hip: the eight pixels 8g + 4r + e fall on
//      phase e & 1 of 256 B and granule mt ^ (e >> 1 | (g & 1) << 1): eight
//      distinct (phase, granule) pairs x 32 B = 256 distinct bytes.
//   A, Cout 32: pixel rows are 64 B: e picks one of four 64-byte phases, the
//      two g are 512 B = 0 (mod 256) apart and would collide 2-way; with the
//      swizzle they read granules mt and mt ^ 1 of the same phase:
//      (e, g & 1, q) -> 32 distinct 8-byte words, conflict-free.
//   B narrow: as conv7x7_wgrad.hip: ONE patch row per half (the row depends
//      on g >> 1), pixels 16(g&1) + 8r + 2e + q: 10 consecutive pixels (80 B,
//      shared pixels are broadcasts) per g, the two g 128 B apart: [0, 80)
//      and [128, 208), conflict-free whatever the 272-byte row stride.
//   B wide: ONE patch row per half, columns pc = 8(g&1) + 4r + e + kx, 64 B
//      apart, each lane 8 bytes inside one 32-byte granule. The four e are
//      four consecutive columns = four distinct 64-byte phases; the two g are
//      8 columns = 512 B = 0 (mod 256) apart: unswizzled, the same 32 bytes
//      twice, 2-way. Columns pc and pc + 8 always differ in (pc >> 3) & 1
//      (pc <= 17), so with the swizzle they hold the wanted half in OPPOSITE
//      granules of the same phase: 4 phases x 2 granules x 32 B = 256
//      distinct bytes, for every kx and r. A swizzle and not a pad: 32 B of
//      pad per 8 pixels moves column 17 onto column 6's words when a half
//      straddles the pad (kx = 2, r = 1); the swizzle has no such seam and
//      keeps the patch a whole number of 1 KB chunks. Its price: the swizzle
//      bit depends on kx and r per lane, so a lane keeps six column offsets.
//
// Tails. Tiles overhang Ho and Wo. A clamped duplicate of a dY row would be
// ADDED into the sum, so the slab stages pixels with oy >= Ho or ox >= Wo as
// zeros: the lanes of a chunk that are in range issue the global_load_lds,
// the others write 16 zero bytes to the same linear destination. The patch
// is not clamped per row: an overhanging patch unit runs on into the next
// row or image of xp (finite values that only ever meet those zeros: a patch
// row > s*Ho or column past the padded row feeds no pixel with oy < Ho,
// ox < Wo), and one min() keeps it inside the buffer.
//
// Partials. No atomics: block b dumps its accumulators as row b of part
// [grid, Cout*48 | Cout*288] fp32, accumulator a at floats (a*64 + lane)*4
// .. +3 (1 KB per wave and store, coalesced); wide a = wave*(Cout/32)*9 +
// m*9 + tap, narrow a = mt*3 + ky. Every row is written on every launch: no
// fill launch, graph-replay safe. conv3x3s_wgrad_fold_kernel adds the rows
// in a fixed order (bit-identical from run to run), decodes the dump, drops
// the pad slot and pad channels and writes dW [Cout, Cin, 3, 3].
#include "common.h"
#include "launchers.h"

using bf16 = __hip_bfloat16;
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

extern __shared__ __attribute__((aligned(16))) char smem[];

namespace {

constexpr int kTile = 16;
// narrow patch: 33 rows x 17 slots of 16 B (2 pixels x 4 channels)
constexpr int kNRows = 2 * kTile + 1;
constexpr int kNSlots = kTile + 1;
constexpr int kNUnits = kNRows * kNSlots;                  // 561
constexpr int kNChunks = (kNUnits + 63) / 64;              // 9 x 1 KB
constexpr int kNPatchBytes = kNChunks * 1024;
constexpr int kNRowBytes = kNSlots * 16;                   // 272
// wide patch: 18 x 18 pixels of 64 B = 4 units of 16 B
constexpr int kWSide = kTile + 2;
constexpr int kWUnits = kWSide * kWSide * 4;               // 1296
constexpr int kWChunks = (kWUnits + 63) / 64;              // 21 x 1 KB
constexpr int kWPatchBytes = kWChunks * 1024;
constexpr int kWRowBytes = kWSide * 64;                    // 1152
// default cap of the persistent grid: one block per CU
constexpr int kWgradDefaultBlocks = 256;
constexpr int kFoldCols = 16;   // f32x4 columns per fold block
constexpr int kFoldRows = 16;   // row groups per fold block

using lds_char = __attribute__((address_space(3))) char;

__device__ __forceinline__ void load16_to_lds(const char* src, char* dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)src,
      (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

// one bf16x8 operand: two transposed reads
__device__ __forceinline__ bf16x8 tr_read8(const lds_char* p0,
                                           const lds_char* p1) {
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4*)p0);
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4*)p1);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// The dY slab of one tile: 256 pixels x COUT in 1 KB chunks, chunk ch =
// wave + 4i. Lane l fills the 16-byte unit l % kUnits of tile pixel
// p = kPix*ch + l / kUnits (tile row p >> 4, column p & 15); the swizzle f
// depends on the column alone, so a lane's column, f and source unit are the
// same for all its chunks.
template <int COUT>
struct Slab {
  static constexpr int kPixB = COUT * 2;          // bytes per pixel row
  static constexpr int kUnits = kPixB / 16;       // 4 | 8
  static constexpr int kPix = 64 / kUnits;        // pixels per chunk 16 | 8
  static constexpr int kChunks = 256 / kPix;      // 16 | 32
  static constexpr int kBytes = kChunks * 1024;
  static constexpr int kRowStep = 4 * kPix / 16;  // tile rows between chunks

  static __device__ __forceinline__ int f(int col) {
    return COUT == 64 ? (((col >> 1) & 1) | (((col >> 3) & 1) << 1))
                      : ((col >> 3) & 1);
  }

  int col, row0, ssrc;
  __device__ __forceinline__ Slab(int wave, int lane) {
    const int p0 = kPix * wave + lane / kUnits;
    col = p0 & 15;
    row0 = p0 >> 4;
    const int u = lane % kUnits;
    ssrc = col * kPixB + (((((u >> 1) ^ f(col)) << 1) | (u & 1)) << 4);
  }

  // overhanging pixels are staged as ZEROS (a clamped row would be added)
  __device__ __forceinline__ void stage(char* sbase, const bf16* DY, int n,
                                        int oy0, int ox0, int Ho, int Wo,
                                        int wave, int lane) const {
    const bool xin = ox0 + col < Wo;
#pragma unroll
    for (int i = 0; i < kChunks / 4; ++i) {
      const int oy = oy0 + row0 + kRowStep * i;
      char* dst = sbase + (wave + 4 * i) * 1024;  // wave-uniform
      if (xin && oy < Ho) {
        const char* src = (const char*)DY +
                          (((long long)n * Ho + oy) * Wo + ox0) * kPixB + ssrc;
        load16_to_lds(src, dst);
      } else {
        *(__attribute__((address_space(3))) f32x4*)((lds_char*)dst +
                                                    lane * 16) = f32x4{};
      }
    }
  }

  // byte offset of this lane's A fragment of M tile mt at k-step 0, r = 0;
  // r is + 4*kPixB, a k-step + 32*kPixB
  static __device__ __forceinline__ unsigned a_off(int mt, int g, int e,
                                                   int q) {
    const int af = COUT == 64 ? ((e >> 1) | ((g & 1) << 1)) : (g & 1);
    return (8 * g + e) * kPixB + ((mt ^ af) << 5) + q * 8;
  }
};

}  // namespace

// ---- narrow: Cin <= 4, stride 2 -------------------------------------------
template <int COUT>
__global__ __launch_bounds__(256, 1) void conv3x3s_wgrad_narrow_kernel(
    const bf16* __restrict__ XP, const bf16* __restrict__ DY,
    float* __restrict__ part, const int Ho, const int Wo, const int Hp,
    const int Sp, const long long xp_last, const int tiles_x,
    const int tiles_y, const int tiles) {
  using S = Slab<COUT>;
  constexpr int kMT = COUT / 16;             // M tiles, all in every wave
  constexpr int kNA = kMT * 3;               // accumulators per lane
  constexpr int kBufBytes = kNPatchBytes + S::kBytes;
  char* lds = smem;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane >> 4;
  const int e = (lane >> 2) & 3;
  const int q = lane & 3;
  const int tiles_img = tiles_x * tiles_y;

  // patch: byte offset of each of this lane's units from the tile's origin
  int prel[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    int p = (wave + 4 * i) * 64 + lane;
    if (p > kNUnits - 1) p = kNUnits - 1;
    prel[i] = ((p / kNSlots) * Sp + p % kNSlots) * 16;
  }
  const S slab(wave, lane);

  auto stage = [&](int buf, int t) {
    const int tile = xcd_swizzle(t, tiles);
    const int n = tile / tiles_img;
    const int rem = tile % tiles_img;
    const int oy0 = (rem / tiles_x) * kTile;
    const int ox0 = (rem % tiles_x) * kTile;
    char* pbase = lds + buf * kBufBytes;
    const long long origin =
        (((long long)n * Hp + 2 * oy0) * Sp + ox0) * 16;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int ch = wave + 4 * i;  // wave-uniform
      if (ch < kNChunks) {
        long long off = origin + prel[i];
        if (off > xp_last) off = xp_last;  // overhang: times a zero of dY
        load16_to_lds((const char*)XP + off, pbase + ch * 1024);
      }
    }
    slab.stage(pbase + kNPatchBytes, DY, n, oy0, ox0, Ho, Wo, wave, lane);
  };

  stage(0, blockIdx.x);

  // fragment bases of this lane at its first k-step ks = wave (bytes inside
  // one buffer); its second k-step wave + 4 is 4 k-steps = 16 patch rows on
  unsigned a_off[kMT];
#pragma unroll
  for (int m = 0; m < kMT; ++m)
    a_off[m] = kNPatchBytes + wave * 32 * S::kPixB + S::a_off(m, g, e, q);
  const unsigned b_off = (4 * wave + 2 * (g >> 1)) * kNRowBytes +
                         (16 * (g & 1) + 2 * e + q) * 8;

  f32x4 acc[kMT][3] = {};
  __syncthreads();

  int buf = 0;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    if (t + (int)gridDim.x < tiles) stage(buf ^ 1, t + gridDim.x);

    const lds_char* base = (const lds_char*)lds + buf * kBufBytes;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      bf16x8 a[kMT], b[3];
#pragma unroll
      for (int m = 0; m < kMT; ++m) {
        const lds_char* p = base + a_off[m] + j * 128 * S::kPixB;
        a[m] = tr_read8(p, p + 4 * S::kPixB);
      }
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const lds_char* p = base + b_off + (16 * j + ky) * kNRowBytes;
        b[ky] = tr_read8(p, p + 64);
      }
#pragma unroll
      for (int m = 0; m < kMT; ++m)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
          acc[m][ky] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[m], b[ky], acc[m][ky], 0, 0, 0);
    }
    // the next tile has landed; nobody reads this buffer any more
    __syncthreads();
    buf ^= 1;
  }

  // the four waves hold sums over different k-steps: meet in LDS (both
  // buffers are free after the last barrier), add in wave order
  __attribute__((address_space(3))) f32x4* red =
      (__attribute__((address_space(3))) f32x4*)(lds_char*)lds;
#pragma unroll
  for (int m = 0; m < kMT; ++m)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
      red[(wave * kNA + m * 3 + ky) * 64 + lane] = acc[m][ky];
  __syncthreads();
  f32x4* prow4 =
      reinterpret_cast<f32x4*>(part + (long long)blockIdx.x * (kNA * 256));
#pragma unroll
  for (int a = wave; a < kNA; a += 4) {
    f32x4 s = red[a * 64 + lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) s += red[(w * kNA + a) * 64 + lane];
    prow4[a * 64 + lane] = s;
  }
}

// ---- wide: Cin = 32, stride 1 ---------------------------------------------
template <int COUT>
__global__ __launch_bounds__(256, 1) void conv3x3s_wgrad_wide_kernel(
    const bf16* __restrict__ XP, const bf16* __restrict__ DY,
    float* __restrict__ part, const int Ho, const int Wo, const int Hp,
    const int Wp, const long long xp_last, const int tiles_x,
    const int tiles_y, const int tiles) {
  using S = Slab<COUT>;
  constexpr int kMT = COUT / 32;             // M tiles per wave
  constexpr int kBufBytes = kWPatchBytes + S::kBytes;
  char* lds = smem;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane >> 4;
  const int e = (lane >> 2) & 3;
  const int q = lane & 3;
  const int tiles_img = tiles_x * tiles_y;

  // patch: unit U = 64*ch + lane is 16-byte unit U & 3 of patch pixel U >> 2
  // and holds SOURCE unit with the granule bit ^ ((column >> 3) & 1)
  int prel[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    int U = (wave + 4 * i) * 64 + lane;
    if (U > kWUnits - 1) U = kWUnits - 1;
    const int pp = U >> 2, u = U & 3;
    const int pr = pp / kWSide, pc = pp % kWSide;
    const int su = ((((u >> 1) ^ (pc >> 3)) & 1) << 1) | (u & 1);
    prel[i] = (pr * Wp + pc) * 64 + su * 16;
  }
  const S slab(wave, lane);

  auto stage = [&](int buf, int t) {
    const int tile = xcd_swizzle(t, tiles);
    const int n = tile / tiles_img;
    const int rem = tile % tiles_img;
    const int oy0 = (rem / tiles_x) * kTile;
    const int ox0 = (rem % tiles_x) * kTile;
    char* pbase = lds + buf * kBufBytes;
    const long long origin = (((long long)n * Hp + oy0) * Wp + ox0) * 64;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int ch = wave + 4 * i;  // wave-uniform
      if (ch < kWChunks) {
        long long off = origin + prel[i];
        if (off > xp_last) off = xp_last;  // overhang: times a zero of dY
        load16_to_lds((const char*)XP + off, pbase + ch * 1024);
      }
    }
    slab.stage(pbase + kWPatchBytes, DY, n, oy0, ox0, Ho, Wo, wave, lane);
  };

  stage(0, blockIdx.x);

  // fragment bases of this lane (bytes inside one buffer)
  const int mh = wave >> 1, hf = wave & 1;
  unsigned a_off[kMT];
#pragma unroll
  for (int m = 0; m < kMT; ++m)
    a_off[m] = kWPatchBytes + S::a_off(kMT * mh + m, g, e, q);
  // B: patch row (g >> 1) (+ 2ks + ky), column 8(g&1) + 4r + e + kx; the
  // granule swizzle follows the column, so one offset per (kx, r)
  unsigned b_off[3][2];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx)
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int pc = 8 * (g & 1) + 4 * r + e + kx;
      b_off[kx][r] = (g >> 1) * kWRowBytes + pc * 64 +
                     (((hf ^ (pc >> 3)) & 1) << 5) + q * 8;
    }

  f32x4 acc[kMT][9] = {};
  __syncthreads();

  int buf = 0;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    if (t + (int)gridDim.x < tiles) stage(buf ^ 1, t + gridDim.x);

    const lds_char* base = (const lds_char*)lds + buf * kBufBytes;
    // B fragment (ks, ky, kx) is patch rows 2ks + ky: (ks + 1, 0, kx) is
    // (ks, 2, kx), so a k-step reads only the rows ky = 1, 2 anew
    bf16x8 a[kMT], b[3][3];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
#pragma unroll
      for (int m = 0; m < kMT; ++m) {
        const lds_char* p = base + a_off[m] + ks * 32 * S::kPixB;
        a[m] = tr_read8(p, p + 4 * S::kPixB);
      }
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          if (ky == 0 && ks > 0) {
            b[0][kx] = b[2][kx];
          } else {
            const int row = (2 * ks + ky) * kWRowBytes;
            b[ky][kx] = tr_read8(base + b_off[kx][0] + row,
                                 base + b_off[kx][1] + row);
          }
        }
#pragma unroll
      for (int m = 0; m < kMT; ++m)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
          acc[m][tap] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[m], b[tap / 3][tap % 3], acc[m][tap], 0, 0, 0);
    }
    // the next tile has landed; nobody reads this buffer any more
    __syncthreads();
    buf ^= 1;
  }

  f32x4* prow4 = reinterpret_cast<f32x4*>(
      part + (long long)blockIdx.x * (COUT * 288)) + wave * kMT * 9 * 64 +
      lane;
#pragma unroll
  for (int m = 0; m < kMT; ++m)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) prow4[(m * 9 + tap) * 64] = acc[m][tap];
}

// part [rows, Cout*48 | Cout*288] -> dW [Cout, Cin, 3, 3]. A block takes
// kFoldCols f32x4 columns of the dump; row group rg adds rows rg, rg + 16,
// ... in order, then thread (0, col) adds the 16 group sums in order: one
// fixed tree, the same bits every run. f32x4 v of the dump is lane v & 63 of
// accumulator v >> 6: D map col = lane & 15, row = (lane >> 4)*4 + reg -> co.
__global__ __launch_bounds__(256) void conv3x3s_wgrad_fold_kernel(
    const float* __restrict__ part, float* __restrict__ dW, const int rows,
    const int Cin, const int Cout, const int wide) {
  __shared__ f32x4 red[kFoldRows][kFoldCols];
  const int cl = threadIdx.x % kFoldCols;
  const int rg = threadIdx.x / kFoldCols;
  const int row4 = Cout * (wide ? 72 : 12);   // f32x4 per partial row
  const int v = blockIdx.x * kFoldCols + cl;  // < row4, exact grid
  const int lane = v & 63, a = v >> 6;
  int mt, ky, kx, c;
  if (wide) {
    const int mtw = Cout / 32, wave = a / (mtw * 9), tap = a % 9;
    mt = mtw * (wave >> 1) + (a % (mtw * 9)) / 9;
    ky = tap / 3;
    kx = tap % 3;
    c = 16 * (wave & 1) + (lane & 15);
  } else {
    mt = a / 3;
    ky = a % 3;
    kx = (lane & 15) >> 2;
    c = lane & 3;
  }
  const bool keep = kx < 3 && c < Cin;
  f32x4 s = {};
  if (keep) {
    const f32x4* src = reinterpret_cast<const f32x4*>(part) + v;
    for (int r = rg; r < rows; r += kFoldRows) s += src[(long long)r * row4];
  }
  red[rg][cl] = s;
  __syncthreads();
  if (rg == 0 && keep) {
#pragma unroll
    for (int r = 1; r < kFoldRows; ++r) s += red[r][cl];
    const int co = 16 * mt + 4 * (lane >> 4);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      dW[(((co + reg) * Cin + c) * 3 + ky) * 3 + kx] = s[reg];
  }
}

extern "C" int conv3x3_small_wgrad_tiles(int Nimg, int Ho, int Wo) {
  return Nimg * ((Ho + kTile - 1) / kTile) * ((Wo + kTile - 1) / kTile);
}

// every block gets the same number of tiles (+-1), as conv7x7s2_wgrad_grid
extern "C" int conv3x3_small_wgrad_grid(int tiles, int max_blocks) {
  const int cap = max_blocks > 0 && max_blocks < kWgradDefaultBlocks
                      ? max_blocks
                      : kWgradDefaultBlocks;
  const int rounds = (tiles + cap - 1) / cap;
  return rounds == 0 ? 0 : (tiles + rounds - 1) / rounds;
}

extern "C" void launch_conv3x3_small_wgrad(const void* xp, const void* dy,
                                           float* part, float* dw, int Nimg,
                                           int Ho, int Wo, int Cin, int Cout,
                                           int stride, int max_blocks,
                                           hipStream_t s) {
  const bool wide = stride == 1;
  const int tiles_x = (Wo + kTile - 1) / kTile;
  const int tiles_y = (Ho + kTile - 1) / kTile;
  const int tiles = Nimg * tiles_x * tiles_y;
  const int grid = conv3x3_small_wgrad_grid(tiles, max_blocks);
  // rows of xp and 16-byte units (narrow) or pixels (wide) per row
  const int Hp = wide ? Ho + 2 : 2 * Ho + 1;
  const int Rp = wide ? Wo + 2 : Wo + 1;
  const long long xp_last =
      (long long)Nimg * Hp * Rp * (wide ? 64 : 16) - 16;
  const int slab = Cout * 512;  // 256 pixels x Cout bf16
  const bf16* X = (const bf16*)xp;
  const bf16* D = (const bf16*)dy;
  if (grid > 0) {
    if (wide) {
      const int lds = 2 * (kWPatchBytes + slab);
      if (Cout == 64)
        hipLaunchKernelGGL(conv3x3s_wgrad_wide_kernel<64>, dim3(grid),
                           dim3(256), lds, s, X, D, part, Ho, Wo, Hp, Rp,
                           xp_last, tiles_x, tiles_y, tiles);
      else
        hipLaunchKernelGGL(conv3x3s_wgrad_wide_kernel<32>, dim3(grid),
                           dim3(256), lds, s, X, D, part, Ho, Wo, Hp, Rp,
                           xp_last, tiles_x, tiles_y, tiles);
    } else {
      const int lds = 2 * (kNPatchBytes + slab);
      if (Cout == 64)
        hipLaunchKernelGGL(conv3x3s_wgrad_narrow_kernel<64>, dim3(grid),
                           dim3(256), lds, s, X, D, part, Ho, Wo, Hp, Rp,
                           xp_last, tiles_x, tiles_y, tiles);
      else
        hipLaunchKernelGGL(conv3x3s_wgrad_narrow_kernel<32>, dim3(grid),
                           dim3(256), lds, s, X, D, part, Ho, Wo, Hp, Rp,
                           xp_last, tiles_x, tiles_y, tiles);
    }
  }
  // rows == 0 (an empty batch): the fold writes zeros
  hipLaunchKernelGGL(conv3x3s_wgrad_fold_kernel,
                     dim3(Cout * (wide ? 72 : 12) / kFoldCols), dim3(256), 0,
                     s, part, dw, grid, Cin, Cout, wide ? 1 : 0);
}
