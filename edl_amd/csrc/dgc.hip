// DGC (deep gradient compression) with momentum correction: top-k
// compress / decode over one flat fp32 gradient bucket.
//
//   dgc_accumulate   u = mu*u + (g + wd*p); v += u         (5-6 streams)
//                    + radix-select pass 0 (histogram of the top 11 bits)
//   dgc_hist         radix-select passes 1, 2 (10 bits each; 1 stream)
//   dgc_pick         one block: fix a digit / the final threshold
//   dgc_compact      (index, value) pairs of the selected; v = u = 0 there
//   dgc_scatter_add  out[idx] += val for ONE rank's payload (decode)
//
// Selection rule (edl_amd/ops/dgc.py holds the torch twin): a_i = the bit
// pattern of |v_i| (31 bits, so inf/nan sort highest), P = the k-th
// largest a_i; select a >= P when count(a >= P) <= k, else a > P; never
// a == 0. Both cases collapse to one threshold T (a >= T), and the count
// nsel <= k is known once the last digit is fixed, so the compaction can
// fill the slots [nsel, k) with -1 while the selected land in [0, nsel).
//
// Workspace (uint32, zeroed ONCE by the caller): 2048 histogram bins, then
// the state words below. dgc_pick re-zeroes the histogram after reading
// it and its last pass resets the cursor, so a step needs no fill launch.
// One workspace serves one stream at a time.
#include "common.h"
#include "launchers.h"

namespace {

constexpr int kBins0 = 2048;  // pass 0: bits 30..20
constexpr int kBins = 1024;   // passes 1, 2: bits 19..10, 9..0
constexpr int kBlock = 256;
// The streaming kernels run 1024-thread blocks, at most 512 of them: the
// same 2048*256 threads as elementwise_grid's cap, but a quarter of the
// blocks, because what each BLOCK does once (the histogram flush, the
// compaction's cursor claim) is a global atomic on shared words, and those
// atomics, not the stream, set the time at 2048 blocks.
constexpr int kStream = 1024;
constexpr int kStreamBlocks = 512;

enum { ST_PREFIX = 0, ST_KREM = 1, ST_THRESH = 2, ST_NSEL = 3, ST_CURSOR = 4 };

__device__ __forceinline__ unsigned abs_bits(float x) {
  return __float_as_uint(x) & 0x7fffffffu;
}

__device__ __forceinline__ float4 ld4(const float* p) {
  return *reinterpret_cast<const float4*>(__builtin_assume_aligned(p, 16));
}

__device__ __forceinline__ void st4(float* p, float4 x) {
  *reinterpret_cast<float4*>(__builtin_assume_aligned(p, 16)) = x;
}

template <bool HAS_P>
__device__ __forceinline__ float acc1(float g, float& u, float v, float p,
                                      float mu, float wd) {
  const float t = HAS_P ? g + wd * p : g;
  u = mu * u + t;
  return v + u;
}

// R copies of the block histogram, chosen by lane & (R-1) and interleaved
// (bin*R + copy) so the copies of one bin sit in neighbouring LDS banks:
// gradient magnitudes share a handful of exponents, so most lanes of a
// wave hit the same few bins.
template <bool HAS_P, int R>
__global__ __launch_bounds__(kStream) void dgc_accumulate_kernel(
    const float* __restrict__ g, float* __restrict__ u, float* __restrict__ v,
    const float* __restrict__ p, const float mu, const float wd,
    const long long n, const int vec, unsigned* __restrict__ hist) {
  __shared__ unsigned lh[kBins0 * R];
  for (int b = threadIdx.x; b < kBins0 * R; b += blockDim.x) lh[b] = 0;
  __syncthreads();
  const unsigned copy = threadIdx.x & (R - 1);
  const long long n4 = vec ? (n >> 2) : 0;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = t0; i < n4; i += stride) {
    const float4 pg = ld4(g + 4 * i);
    float4 pu = ld4(u + 4 * i), pv = ld4(v + 4 * i);
    float4 pp = {0.0f, 0.0f, 0.0f, 0.0f};
    if (HAS_P) pp = ld4(p + 4 * i);
    pv.x = acc1<HAS_P>(pg.x, pu.x, pv.x, pp.x, mu, wd);
    pv.y = acc1<HAS_P>(pg.y, pu.y, pv.y, pp.y, mu, wd);
    pv.z = acc1<HAS_P>(pg.z, pu.z, pv.z, pp.z, mu, wd);
    pv.w = acc1<HAS_P>(pg.w, pu.w, pv.w, pp.w, mu, wd);
    st4(u + 4 * i, pu);
    st4(v + 4 * i, pv);
    atomicAdd(&lh[(abs_bits(pv.x) >> 20) * R + copy], 1u);
    atomicAdd(&lh[(abs_bits(pv.y) >> 20) * R + copy], 1u);
    atomicAdd(&lh[(abs_bits(pv.z) >> 20) * R + copy], 1u);
    atomicAdd(&lh[(abs_bits(pv.w) >> 20) * R + copy], 1u);
  }
  // tail (n % 4), or everything when a pointer is not 16-B aligned
  for (long long j = (n4 << 2) + t0; j < n; j += stride) {
    float uu = u[j];
    const float vv = acc1<HAS_P>(g[j], uu, v[j], HAS_P ? p[j] : 0.0f, mu, wd);
    u[j] = uu;
    v[j] = vv;
    atomicAdd(&lh[(abs_bits(vv) >> 20) * R + copy], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kBins0; b += blockDim.x) {
    unsigned c = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) c += lh[b * R + r];
    if (c) atomicAdd(&hist[b], c);
  }
}

// passes 1, 2: the next 10-bit digit of the elements whose higher bits
// equal the prefix fixed so far
__global__ __launch_bounds__(kStream) void dgc_hist_kernel(
    const float* __restrict__ v, const long long n, const int vec,
    const int shift_hi, const int shift_lo, unsigned* __restrict__ hist,
    const unsigned* __restrict__ state) {
  __shared__ unsigned lh[kBins];
  for (int b = threadIdx.x; b < kBins; b += blockDim.x) lh[b] = 0;
  __syncthreads();
  const unsigned prefix = state[ST_PREFIX];
  const long long n4 = vec ? (n >> 2) : 0;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = t0; i < n4; i += stride) {
    const float4 x = ld4(v + 4 * i);
    const unsigned a0 = abs_bits(x.x), a1 = abs_bits(x.y);
    const unsigned a2 = abs_bits(x.z), a3 = abs_bits(x.w);
    if ((a0 >> shift_hi) == prefix) atomicAdd(&lh[(a0 >> shift_lo) & 1023u], 1u);
    if ((a1 >> shift_hi) == prefix) atomicAdd(&lh[(a1 >> shift_lo) & 1023u], 1u);
    if ((a2 >> shift_hi) == prefix) atomicAdd(&lh[(a2 >> shift_lo) & 1023u], 1u);
    if ((a3 >> shift_hi) == prefix) atomicAdd(&lh[(a3 >> shift_lo) & 1023u], 1u);
  }
  for (long long j = (n4 << 2) + t0; j < n; j += stride) {
    const unsigned a = abs_bits(v[j]);
    if ((a >> shift_hi) == prefix) atomicAdd(&lh[(a >> shift_lo) & 1023u], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kBins; b += blockDim.x) {
    const unsigned c = lh[b];
    if (c) atomicAdd(&hist[b], c);
  }
}

// One block. Thread t owns the `per` bins [t*per, (t+1)*per); a suffix
// scan over the thread sums finds the thread, then the bin, that holds
// the krem-th largest element of the current prefix.
__global__ __launch_bounds__(kBlock) void dgc_pick_kernel(
    unsigned* __restrict__ hist, unsigned* __restrict__ state, const int nbins,
    const int pass, const unsigned k) {
  __shared__ unsigned scan[kBlock];
  const int t = threadIdx.x;
  const int per = nbins / kBlock;  // 8 (pass 0) or 4
  unsigned c[8];
  unsigned s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    c[j] = j < per ? hist[t * per + j] : 0u;
    s += c[j];
  }
  const unsigned krem = pass == 0 ? k : state[ST_KREM];
  const unsigned prefix = pass == 0 ? 0u : state[ST_PREFIX];
  scan[t] = s;
  __syncthreads();
  for (int off = 1; off < kBlock; off <<= 1) {
    const unsigned add = t + off < kBlock ? scan[t + off] : 0u;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  const unsigned incl = scan[t];   // elements in this thread's bins and above
  unsigned above = incl - s;       // elements in the bins above this thread's
  if (above < krem && krem <= incl) {  // true for exactly one thread
    int dsel = -1;
    unsigned csel = 0;
#pragma unroll
    for (int j = 7; j >= 0; --j) {
      if (j < per && dsel < 0) {
        if (above + c[j] >= krem) {
          dsel = j;
          csel = c[j];
        } else {
          above += c[j];
        }
      }
    }
    const unsigned digit = (unsigned)(t * per + dsel);
    const unsigned newk = krem - above;  // 1 <= newk <= csel
    const unsigned np = pass == 0 ? digit : ((prefix << 10) | digit);
    state[ST_PREFIX] = np;
    state[ST_KREM] = newk;
    if (pass == 2) {
      // np = P, csel = count(a == P), k - newk = count(a > P)
      const unsigned gt = k - newk;
      const bool inclusive = csel <= newk;  // count(a >= P) <= k
      unsigned thresh = inclusive ? np : np + 1u;
      unsigned nsel = inclusive ? gt + csel : gt;
      if (thresh == 0u) {  // P == 0: zeros are never sent
        thresh = 1u;
        nsel = gt;
      }
      state[ST_THRESH] = thresh;
      state[ST_NSEL] = nsel;
      state[ST_CURSOR] = 0u;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (j < per) hist[t * per + j] = 0u;
}

// Compaction stages the selected in LDS and claims payload slots with ONE
// cursor atomic per block per flush. A returning atomic on one word
// serialises chip-wide (about 11 ns each on MI355X), so a claim per wave,
// i.e. nearly one per selected element at 0.1% density, costs more than
// the whole stream.
constexpr int kStage = 6144;              // staged (idx, bits) pairs
constexpr int kStageLimit = kStage - 4 * kStream;  // flush above this

struct Stage {
  int idx[kStage];
  unsigned bits[kStage];
  unsigned count, base;
};

// block-uniform: every thread of the block calls it the same number of times
__device__ __forceinline__ void stage_flush(Stage& st, const unsigned limit,
                                            const unsigned k,
                                            float* __restrict__ v,
                                            float* __restrict__ u,
                                            int* __restrict__ payload,
                                            unsigned* __restrict__ cursor) {
  __syncthreads();  // this iteration's staged pairs are in
  const unsigned cnt = st.count;
  __syncthreads();  // everyone has read it before anyone stages more
  if (cnt <= limit) return;
  if (threadIdx.x == 0) {
    st.base = atomicAdd(cursor, cnt);
    st.count = 0;
  }
  __syncthreads();
  const unsigned base = st.base;
  for (unsigned e = threadIdx.x; e < cnt; e += blockDim.x) {
    const unsigned slot = base + e;
    if (slot < k) {  // always true by the selection rule; keeps a bug in bounds
      const int idx = st.idx[e];
      payload[slot] = idx;
      payload[(size_t)k + slot] = (int)st.bits[e];
      v[idx] = 0.0f;
      u[idx] = 0.0f;
    }
  }
  __syncthreads();  // the pairs are out before the stage is reused
}

// one LDS atomic per wave: the offset is broadcast from lane 0 and each
// lane adds the popcount of the ballot below it
__device__ __forceinline__ unsigned wave_claim(unsigned* count, int total,
                                               int lane) {
  unsigned off = 0;
  if (lane == 0) off = atomicAdd(count, (unsigned)total);
  return __shfl(off, 0, 64);
}

__device__ __forceinline__ void stage_put(Stage& st, unsigned e, long long idx,
                                          float x) {
  st.idx[e] = (int)idx;
  st.bits[e] = __float_as_uint(x);
}

__global__ __launch_bounds__(kStream) void dgc_compact_kernel(
    float* __restrict__ v, float* __restrict__ u, const long long n,
    const int vec, int* __restrict__ payload, const unsigned k,
    unsigned* __restrict__ state) {
  __shared__ Stage st;
  if (threadIdx.x == 0) st.count = 0;
  const unsigned thresh = state[ST_THRESH];
  const unsigned nsel = state[ST_NSEL];
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long b0 = (long long)blockIdx.x * blockDim.x;
  // inert slots: index -1, bits 0. The selected claim [0, nsel) only.
  for (long long j = (long long)nsel + b0 + threadIdx.x; j < (long long)k;
       j += stride) {
    payload[j] = -1;
    payload[(size_t)k + j] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  const unsigned long long below = (1ull << lane) - 1ull;
  const long long n4 = vec ? (n >> 2) : 0;
  // block-uniform trip counts, so every lane reaches the ballots and syncs
  for (long long b = b0; b < n4; b += stride) {
    const long long i = b + threadIdx.x;
    const bool in = i < n4;
    float4 x = {0.0f, 0.0f, 0.0f, 0.0f};
    if (in) x = ld4(v + 4 * i);
    const bool s0 = in && abs_bits(x.x) >= thresh;
    const bool s1 = in && abs_bits(x.y) >= thresh;
    const bool s2 = in && abs_bits(x.z) >= thresh;
    const bool s3 = in && abs_bits(x.w) >= thresh;
    const unsigned long long m0 = __ballot(s0), m1 = __ballot(s1);
    const unsigned long long m2 = __ballot(s2), m3 = __ballot(s3);
    const int c0 = __popcll(m0), c1 = __popcll(m1), c2 = __popcll(m2);
    const int total = c0 + c1 + c2 + __popcll(m3);
    if (total) {  // wave-uniform
      const unsigned off = wave_claim(&st.count, total, lane);
      if (s0) stage_put(st, off + __popcll(m0 & below), 4 * i, x.x);
      if (s1) stage_put(st, off + c0 + __popcll(m1 & below), 4 * i + 1, x.y);
      if (s2) stage_put(st, off + c0 + c1 + __popcll(m2 & below), 4 * i + 2,
                        x.z);
      if (s3) stage_put(st, off + c0 + c1 + c2 + __popcll(m3 & below),
                        4 * i + 3, x.w);
    }
    stage_flush(st, kStageLimit, k, v, u, payload, &state[ST_CURSOR]);
  }
  for (long long b = (n4 << 2) + b0; b < n; b += stride) {
    const long long j = b + threadIdx.x;
    const float x = j < n ? v[j] : 0.0f;
    const bool s = j < n && abs_bits(x) >= thresh;
    const unsigned long long ms = __ballot(s);
    const int total = __popcll(ms);
    if (total) {
      const unsigned off = wave_claim(&st.count, total, lane);
      if (s) stage_put(st, off + __popcll(ms & below), j, x);
    }
    stage_flush(st, kStageLimit, k, v, u, payload, &state[ST_CURSOR]);
  }
  stage_flush(st, 0u, k, v, u, payload, &state[ST_CURSOR]);
}

// indices are unique within one rank's payload: plain read-add-write
__global__ __launch_bounds__(kBlock) void dgc_scatter_add_kernel(
    float* __restrict__ out, const long long n, const int* __restrict__ payload,
    const long long k) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long j = (long long)blockIdx.x * kBlock + threadIdx.x; j < k;
       j += stride) {
    const int idx = payload[j];
    if (idx >= 0 && idx < n) out[idx] += __int_as_float(payload[k + j]);
  }
}

inline int stream_grid(long long work) {
  const long long want = (work + kStream - 1) / kStream;
  return (int)(want < kStreamBlocks ? want : kStreamBlocks);
}

inline int aligned16(const void* a, const void* b, const void* c,
                     const void* d) {
  const uintptr_t m = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d;
  return (m & 15u) == 0;
}

}  // namespace

extern "C" int dgc_workspace_words() { return kBins0 + 8; }

// ws: the zero-initialised workspace. hist_copies: 1 or 4 (LDS replication
// of the pass-0 histogram).
extern "C" void launch_dgc_accumulate(const float* g, float* u, float* v,
                                      const float* p, float mu, float wd,
                                      long long n, unsigned* ws,
                                      int hist_copies, hipStream_t stream) {
  const int vec = aligned16(g, u, v, p);
  const int grid = stream_grid(vec ? (n + 3) / 4 : n);
#define EDL_DGC_ACC(HASP, R)                                                 \
  hipLaunchKernelGGL((dgc_accumulate_kernel<HASP, R>), dim3(grid),          \
                     dim3(kStream), 0, stream, g, u, v, p, mu, wd, n, vec, ws)
  if (p) {
    if (hist_copies == 4) EDL_DGC_ACC(true, 4); else EDL_DGC_ACC(true, 1);
  } else {
    if (hist_copies == 4) EDL_DGC_ACC(false, 4); else EDL_DGC_ACC(false, 1);
  }
#undef EDL_DGC_ACC
}

extern "C" void launch_dgc_hist(const float* v, long long n, unsigned* ws,
                                int pass, hipStream_t stream) {
  const int vec = aligned16(v, nullptr, nullptr, nullptr);
  const int grid = stream_grid(vec ? (n + 3) / 4 : n);
  hipLaunchKernelGGL(dgc_hist_kernel, dim3(grid), dim3(kStream), 0, stream, v,
                     n, vec, pass == 1 ? 20 : 10, pass == 1 ? 10 : 0, ws,
                     ws + kBins0);
}

extern "C" void launch_dgc_pick(unsigned* ws, int pass, unsigned k,
                                hipStream_t stream) {
  hipLaunchKernelGGL(dgc_pick_kernel, dim3(1), dim3(kBlock), 0, stream, ws,
                     ws + kBins0, pass == 0 ? kBins0 : kBins, pass, k);
}

extern "C" void launch_dgc_compact(float* v, float* u, long long n,
                                   int* payload, unsigned k, unsigned* ws,
                                   hipStream_t stream) {
  const int vec = aligned16(v, nullptr, nullptr, nullptr);
  const int grid = stream_grid(vec ? (n + 3) / 4 : n);
  hipLaunchKernelGGL(dgc_compact_kernel, dim3(grid), dim3(kStream), 0, stream,
                     v, u, n, vec, payload, k, ws + kBins0);
}

extern "C" void launch_dgc_scatter_add(float* out, long long n,
                                       const int* payload, long long k,
                                       hipStream_t stream) {
  const int grid = elementwise_grid(k, kBlock);
  hipLaunchKernelGGL(dgc_scatter_add_kernel, dim3(grid), dim3(kBlock), 0,
                     stream, out, n, payload, k);
}
