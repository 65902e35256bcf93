// BN forward finalize: reduce the [nblocks, 2C] statistics partials over
// rows, then mean / invstd / scale / shift and the running-stat update.
//
// The kernel moves a few hundred KB at most and is pure latency: what a
// call costs is the number of DEPENDENT memory round trips a thread makes
// (other XCDs wrote the partial rows one launch earlier, so every first
// touch misses L2). The previous cut, 64 channels x 4 strips walking 4 rows
// per iteration with a full vmcnt drain in between, made 12 of them at 192
// rows plus two for the parameters: 8.0-8.7 us/call against 4.7 for the
// short partials. Here a 1024-thread block owns kFinCols consecutive
// channels and splits the rows over kFinStrips strips; a thread issues
// every load of a batch (up to kFinRowsMax rows: kStatsPartRowCap rows are
// ONE batch) before it waits for the first, then the zero-after-read
// stores, then the adds, and the parameter loads go out ahead of all of
// it. Strips fold through LDS in a fixed order: no atomics, identical
// partials give identical bits on every launch and graph replay.
//
// Built without packed-fp32 VALU ops (build_hip.py): the folds are plain
// v_add_f32 chains, which is also what the generated code is read against
// in docs/kernels.md.
#include "bn_phases.h"
#include "launchers.h"

constexpr int kFinThreads = 1024;
constexpr int kFinCols = 64;  // a wave reads one 256-byte run of a row
constexpr int kFinStrips = kFinThreads / kFinCols;
constexpr int kFinRowsMax = kStatsPartRowCap / kFinStrips;  // 12
constexpr int kFinRowsMid = 4;
static_assert(kFinCols >= 16 && kStatsPartRowCap % kFinStrips == 0 &&
                  kFinStrips % 4 == 0 && kFinRowsMid < kFinRowsMax,
              "finalize geometry");

// One batch: rows row0 + kFinStrips * u, u < U, columns c (sum) and C + c
// (sum of squares). A row past the end is read from the last valid row
// instead (a load that is always in bounds keeps the batch branch-free)
// and contributes 0; only rows this thread owns are zeroed, each once.
template <int U>
__device__ __forceinline__ void fin_batch(float* __restrict__ partial,
                                          const int row0, const int nblocks,
                                          const int c, const int C,
                                          const bool zero, float& s,
                                          float& q) {
  float vs[U], vq[U];
  long long at[U];
  bool ok[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int row = row0 + kFinStrips * u;
    ok[u] = row < nblocks;
    at[u] = (long long)(ok[u] ? row : nblocks - 1) * (2 * C) + c;
    vs[u] = partial[at[u]];
    vq[u] = partial[at[u] + C];
  }
  if (zero) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (ok[u]) {
        partial[at[u]] = 0.0f;
        partial[at[u] + C] = 0.0f;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    s += ok[u] ? vs[u] : 0.0f;
    q += ok[u] ? vq[u] : 0.0f;
  }
}

// Fixed-order fold of one channel's kFinStrips strip sums (4 chains).
__device__ __forceinline__ float fin_fold(
    const float (&a)[kFinStrips][kFinCols], const int lane) {
  float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int s = 0; s < kFinStrips; s += 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] += a[s + j][lane];
  }
  return (c[0] + c[1]) + (c[2] + c[3]);
}

extern "C" __global__ __launch_bounds__(kFinThreads) void bn_finalize_kernel(
    float* __restrict__ partial, const int nblocks, const int zero_src,
    const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ mean_out,
    float* __restrict__ invstd_out, float* __restrict__ scale_out,
    float* __restrict__ shift_out, float* __restrict__ running_mean,
    float* __restrict__ running_var, const float momentum, const float eps,
    const long long M, const int C) {
  __shared__ float accs[kFinStrips][kFinCols];
  __shared__ float accq[kFinStrips][kFinCols];
  const int lane = threadIdx.x % kFinCols;
  const int strip = threadIdx.x / kFinCols;
  const int c = blockIdx.x * kFinCols + lane;
  const bool fin = strip == 0 && c < C;
  float g = 0.0f, bt = 0.0f, rm = 0.0f, rv = 0.0f;
  if (fin) {
    g = gamma[c];
    bt = beta[c];
    if (running_mean != nullptr) {
      rm = running_mean[c];
      rv = running_var[c];
    }
  }
  float s = 0.0f, q = 0.0f;
  if (c < C) {
    // one batch up to kStatsPartRowCap rows, sized down for the short
    // partials of the late stages; a longer pre_part loops over batches
    const bool zero = zero_src != 0;
    int base = 0;
    while (base < nblocks) {
      const int rem = nblocks - base;
      if (rem > kFinRowsMid * kFinStrips) {
        fin_batch<kFinRowsMax>(partial, base + strip, nblocks, c, C, zero, s,
                               q);
        base += kFinRowsMax * kFinStrips;
      } else if (rem > kFinStrips) {
        fin_batch<kFinRowsMid>(partial, base + strip, nblocks, c, C, zero, s,
                               q);
        base += kFinRowsMid * kFinStrips;
      } else {
        fin_batch<1>(partial, base + strip, nblocks, c, C, zero, s, q);
        base += kFinStrips;
      }
    }
  }
  accs[strip][lane] = s;
  accq[strip][lane] = q;
  __syncthreads();
  if (!fin) return;
  const float ssum = fin_fold(accs, lane);
  const float qsum = fin_fold(accq, lane);
  bn_channel_finalize(ssum, qsum, g, bt, rm, rv, M, momentum, eps, c, mean_out,
                      invstd_out, scale_out, shift_out, running_mean,
                      running_var);
}

extern "C" void launch_bn_finalize(float* partial, int nblocks, int zero_src,
                                   const float* gamma,
                                   const float* beta, float* mean, float* invstd,
                                   float* scale, float* shift, float* rmean,
                                   float* rvar, float momentum, float eps,
                                   long long M, int C, hipStream_t s) {
  // zero_src: store 0 back after each read — returns a pooled pre_part
  // buffer to the pool clean, killing the per-step FillFunctor launches
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + kFinCols - 1) / kFinCols),
                     dim3(kFinThreads), 0, s, partial, nblocks, zero_src,
                     gamma, beta, mean, invstd, scale, shift, rmean, rvar,
                     momentum, eps, M, C);
}
