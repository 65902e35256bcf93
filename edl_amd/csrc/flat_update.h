// What the flat-bucket update kernels (fused_sgd.hip, fused_adam.hip,
// fused_lars.hip) share. Device-only.
#pragma once
#include "common.h"

// clip = [coef, norm, skip, nskipped] of grad_norm.hip, or null. A skipped
// step leaves the kernel before any store or barrier (uniform: every thread
// reads the same word); otherwise the clip coefficient folds into the
// gradient scale as an fp32 product (coef == 1.0f is bitwise the null path).
__device__ __forceinline__ bool clip_skipped(const float* clip) {
  return clip && clip[2] != 0.0f;
}

__device__ __forceinline__ float clip_scale(const float scale,
                                            const float* clip) {
  return clip ? scale * clip[0] : scale;
}

// lr comes from a device scalar when provided so a hipGraph-captured step
// picks up LR-schedule changes on replay (the host scalar would be frozen
// at capture time); one broadcast load, L2-resident.
__device__ __forceinline__ float load_lr(const float* lr_dev,
                                         const float lr_host) {
  return lr_dev ? *lr_dev : lr_host;
}

// ---- the per-bucket segment table, copied to LDS by the kernel ----
// s_end[nseg] holds cumulative element ends (last == n). Every index
// returned is clamped to nseg-1, so a malformed table mis-assigns segments
// but never reads outside the LDS copy.

// first segment s in [lo, nseg) with s_end[s] > e (nseg-1 if none)
__device__ __forceinline__ int find_seg(const int* s_end, int lo,
                                        const int nseg, const int e) {
  int hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s_end[mid] > e) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// segment of element e, walking forward from s (e >= the start of s)
__device__ __forceinline__ int next_seg(const int* s_end, int s,
                                        const int nseg, const int e) {
  while (s + 1 < nseg && e >= s_end[s]) ++s;
  return s;
}

// The segments of the elements e..e+3 of one float4, looked up per ELEMENT:
// a float4 may straddle a boundary and a segment may be shorter than a
// vector. s is the caller's cursor: segments only grow along a thread's
// grid-stride walk, so the search for e starts from the last answer.
struct Seg4 {
  int q0, q1, q2, q3;
};

__device__ __forceinline__ Seg4 find_seg4(const int* s_end, int& s,
                                          const int nseg, const int e) {
  Seg4 q;
  q.q0 = s = find_seg(s_end, s, nseg, e);
  q.q1 = next_seg(s_end, q.q0, nseg, e + 1);
  q.q2 = next_seg(s_end, q.q1, nseg, e + 2);
  q.q3 = next_seg(s_end, q.q2, nseg, e + 3);
  return q;
}
