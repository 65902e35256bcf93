// Image input stage: crop + bilinear resize + mirror + mean/std normalize of
// a batch of decoded uint8 RGB images, in one launch, written as the
// channels-last bf16 (or fp32) batch the stem convolution reads (reference
// example/collective/resnet50/dali.py: RandomResizedCrop + CropMirrorNormalize;
// utils/img_tool.py: random_crop + cv2.resize INTER_LINEAR + flip + normalize).
//
// Sources sit back to back in one byte buffer at arbitrary offsets, each with
// its own size; one table row per image (launchers.h: kImagePrepFields) names
// the source and the window to resample. For output (oy, ox) of image b:
//
//   ox' = flip ? S-1-ox : ox
//   sx  = max(x0, min(x0 + (ox'+0.5)*(cw/S) - 0.5, x0+cw-1))     (y alike)
//   xa  = floor(sx), xb = min(xa+1, W-1), fx = sx - xa
//   v   = lerp(lerp(aa, ab, fx), lerp(ba, bb, fx), fy)            per channel
//   out = v * 1/(255*std[c]) - mean[c]/std[c]
//
// Shape: a thread owns kImagePrepRun consecutive output pixels of a row
// (12 values: 24 B of bf16 as three 8-byte stores, 48 B of fp32 as three
// 16-byte stores, guide Guideline 13) and walks kImagePrepRows rows with the
// column taps (xa, xb, fx) kept in registers. Neighbouring threads own
// neighbouring runs of the same rows, so a wave writes whole output rows.
// Write-dominated: 6 B (bf16) out per pixel against at most 12 B of byte
// taps that neighbours share through the caches. No LDS, no atomics.
//
// No table content can take an access out of bounds: tap coordinates are
// clamped into the image the row names, and the byte index of every tap into
// the packed buffer. The output index depends on B and S alone.
#include "common.h"
#include "launchers.h"

namespace {

constexpr int kRun = kImagePrepRun;
constexpr int kRows = kImagePrepRows;
constexpr int kBlock = 256;
// extents beyond this only come from a broken table; the clamp keeps the
// index arithmetic inside 64 bits
constexpr int kMaxExtent = 1 << 24;

struct Norm3 {
  float k[3];  // 1 / (255 * std)
  float b[3];  // mean / std
};

__device__ __forceinline__ unsigned bf16_bits_rn(const float f) {
  const unsigned u = __float_as_uint(f);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;  // finite inputs only
}

// source coordinate of output index o' (already mirrored) along one axis:
// -> tap a (clamped into [0, n-1]), tap b, weight of b
__device__ __forceinline__ void axis_taps(const int o, const float org,
                                          const float ext, const float step,
                                          const int n, int& a, int& b,
                                          float& f) {
  float s = fmaf((float)o + 0.5f, step, org) - 0.5f;
  s = fmaxf(org, fminf(s, org + ext - 1.0f));
  // a valid table leaves s in [0, n-1] already; fmaxf/fminf also drop a NaN
  s = fminf(fmaxf(s, 0.0f), (float)(n - 1));
  const float fl = floorf(s);
  a = min(max((int)fl, 0), n - 1);
  b = min(a + 1, n - 1);
  f = s - fl;
}

__device__ __forceinline__ float lerp(const float a, const float b,
                                      const float t) {
  return fmaf(t, b - a, a);
}

template <bool BF16>
__global__ __launch_bounds__(kBlock) void image_prep_kernel(
    const unsigned char* __restrict__ packed, const long long nbytes,
    const int* __restrict__ table, void* __restrict__ out, const int S,
    const int blocks_per_image, const Norm3 nrm) {
  const int b = blockIdx.x / blocks_per_image;
  const int ncg = (S + kRun - 1) / kRun;
  const int nrg = (S + kRows - 1) / kRows;
  const int item =
      (blockIdx.x - b * blocks_per_image) * kBlock + (int)threadIdx.x;
  if (item >= ncg * nrg) return;
  const int ox0 = (item % ncg) * kRun;
  const int oy0 = (item / ncg) * kRows;

  const int4 ti = reinterpret_cast<const int4*>(table)[2 * b];
  const float4 tf = reinterpret_cast<const float4*>(table)[2 * b + 1];
  const long long offset = ti.x;
  const int H = min(max(ti.y, 1), kMaxExtent);
  const int W = min(max(ti.z, 1), kMaxExtent);
  const bool flip = ti.w != 0;
  const float x0 = tf.x, y0 = tf.y, cw = tf.z, ch = tf.w;
  const float stepx = cw / (float)S, stepy = ch / (float)S;

  // column taps, once for all the rows of this thread (byte offsets in a row)
  int xa[kRun], xb[kRun];
  float fx[kRun];
#pragma unroll
  for (int j = 0; j < kRun; ++j) {
    const int ox = min(ox0 + j, S - 1);  // a lane past the row repeats S-1
    int a, bb;
    axis_taps(flip ? S - 1 - ox : ox, x0, cw, stepx, W, a, bb, fx[j]);
    xa[j] = 3 * a;
    xb[j] = 3 * bb;
  }
  const bool full = ox0 + kRun <= S;
  const long long last = nbytes - 3;  // last byte index a pixel may start at

  for (int r = 0; r < kRows; ++r) {
    const int oy = oy0 + r;
    if (oy >= S) break;
    int ya, yb;
    float fy;
    axis_taps(oy, y0, ch, stepy, H, ya, yb, fy);
    const long long rowa = offset + (long long)ya * W * 3;
    const long long rowb = offset + (long long)yb * W * 3;
    float v[3 * kRun];
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
      // a pixel is 3 bytes: clamping its first byte to nbytes-3 keeps all
      // three at or below nbytes-1
      const unsigned char* paa =
          packed + max(0LL, min(rowa + xa[j], last));
      const unsigned char* pab =
          packed + max(0LL, min(rowa + xb[j], last));
      const unsigned char* pba =
          packed + max(0LL, min(rowb + xa[j], last));
      const unsigned char* pbb =
          packed + max(0LL, min(rowb + xb[j], last));
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float top = lerp((float)paa[c], (float)pab[c], fx[j]);
        const float bot = lerp((float)pba[c], (float)pbb[c], fx[j]);
        v[3 * j + c] = fmaf(lerp(top, bot, fy), nrm.k[c], -nrm.b[c]);
      }
    }
    const long long e = (((long long)b * S + oy) * S + ox0) * 3;
    if (BF16) {
      unsigned short* o = reinterpret_cast<unsigned short*>(out) + e;
      if (full && (reinterpret_cast<uintptr_t>(o) & 7) == 0) {
        uint2* o2 = reinterpret_cast<uint2*>(o);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          uint2 w;
          w.x = bf16_bits_rn(v[4 * q]) | (bf16_bits_rn(v[4 * q + 1]) << 16);
          w.y = bf16_bits_rn(v[4 * q + 2]) | (bf16_bits_rn(v[4 * q + 3]) << 16);
          o2[q] = w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < kRun; ++j)
          if (ox0 + j < S) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
              o[3 * j + c] = (unsigned short)bf16_bits_rn(v[3 * j + c]);
          }
      }
    } else {
      float* o = reinterpret_cast<float*>(out) + e;
      if (full && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
        float4* o4 = reinterpret_cast<float4*>(o);
#pragma unroll
        for (int q = 0; q < 3; ++q)
          o4[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2],
                              v[4 * q + 3]);
      } else {
#pragma unroll
        for (int j = 0; j < kRun; ++j)
          if (ox0 + j < S) {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[3 * j + c] = v[3 * j + c];
          }
      }
    }
  }
}

}  // namespace

extern "C" int image_prep_blocks_per_image(int S) {
  const long long items =
      (long long)((S + kRun - 1) / kRun) * ((S + kRows - 1) / kRows);
  return (int)((items + kBlock - 1) / kBlock);
}

extern "C" void launch_image_prep(const unsigned char* packed,
                                  long long nbytes, const int* table, void* out,
                                  int B, int S, int out_bf16, const float* k3,
                                  const float* b3, hipStream_t stream) {
  Norm3 nrm;
  for (int c = 0; c < 3; ++c) {
    nrm.k[c] = k3[c];
    nrm.b[c] = b3[c];
  }
  const int bpi = image_prep_blocks_per_image(S);
  const dim3 grid((unsigned)((long long)B * bpi)), block(kBlock);
  if (out_bf16)
    hipLaunchKernelGGL(image_prep_kernel<true>, grid, block, 0, stream, packed,
                       nbytes, table, out, S, bpi, nrm);
  else
    hipLaunchKernelGGL(image_prep_kernel<false>, grid, block, 0, stream, packed,
                       nbytes, table, out, S, bpi, nrm);
}
