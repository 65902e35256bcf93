// The launcher ABI of the edl_amd kernel layer: every extern "C" host entry
// point the .hip translation units define, declared exactly once.
//
// module.cpp (plain C++) includes this to call them; every .hip file
// includes it too, so a definition that drifts from its declaration is a
// compile error ("conflicting types") instead of a link that succeeds and
// passes garbage. Host-only: nothing here but the HIP runtime API header
// (for hipStream_t) and constants both sides must agree on.
#pragma once
#include <hip/hip_runtime_api.h>

// Row cap of the BN-stats partial buffers the fused conv/GEMM epilogues
// write (gemm_bt.hip, conv3x3.hip dense + small): tiles beyond the cap fold
// atomically into row tile % cap, so the host allocates min(tiles_m, cap)
// rows. NOT the BN kernels' own reduce grid (EDL_BN_GRID_CAP, bnrelu.hip),
// which merely defaults to the same number.
constexpr int kStatsPartRowCap = 192;

extern "C" {

// ---- fused_sgd.hip ----
// (clip: the fp32[4] state grad_clip_finalize writes, or null)
void launch_fused_sgd_f32(float* p, const float* g, float* m, float lr,
                          float mu, float wd, float scale, long long n,
                          const float* lr_dev, const float* clip,
                          hipStream_t stream);

// ---- fused_adam.hip ---- (step_dev BEFORE lr_dev; omb = 1-b and ln_b in
// double on the host; seg tables device pointers, null with nseg == 0)
constexpr int kAdamMaxSegments = 1024;  // LDS table: 8 B per segment
void launch_fused_adam_f32(float* p, const float* g, float* m, float* v,
                           const int* step_dev, const float* lr_dev, float lr,
                           float b1, float b2, float omb1, float omb2,
                           float ln_b1, float ln_b2, float eps, float wd,
                           float scale, int decoupled, long long n,
                           const int* seg_end, const float* seg_wd, int nseg,
                           const float* clip, hipStream_t stream);

// ---- grad_norm.hip ---- (sum of squares of up to kGradNormMaxSegs flat
// fp32 buffers per launch into double partial rows, then one block that
// turns the rows into state = [coef, norm, skip, nskipped])
constexpr int kGradNormMaxSegs = 16;
// Rows (blocks of 256 threads) one buffer gets at most; grad_norm_rows(n)
// is the count for n elements (>= 1: an empty buffer writes one 0.0 row).
// Measured on MI355X (tools/clip_bench.py, docs/kernels.md): the reduction
// runs within 5% of its best anywhere from 256 to 8192 rows in total, best
// at 512 for one buffer, while the finalize block pays ~1 us per 4096 rows;
// 512 keeps a single bucket at its best and 16 buckets at 8192 rows.
constexpr int kGradNormRowCap = 512;
constexpr int kGradClipStateLen = 4;
struct GradNormSegs {  // passed to the kernel by value
  const float* ptr[kGradNormMaxSegs];
  long long n[kGradNormMaxSegs];
  int row_off[kGradNormMaxSegs];  // first partial row of the buffer
  int rows[kGradNormMaxSegs];     // == grad_norm_rows(n)
  int nseg;
};
int grad_norm_rows(long long n);
void launch_grad_sumsq_f32(const GradNormSegs* segs, double* partial,
                           hipStream_t stream);
void launch_grad_clip_finalize(const double* partial, int rows_total,
                               double grad_scale, float max_norm,
                               int skip_nonfinite, float* state,
                               hipStream_t stream);

// ---- fused_lars.hip ---- (per-tensor sums of squares of p and g over up to
// kLarsMaxBufs buckets per launch, one block per row of the device chunk
// table; one launch that turns them into trust[tensor]; then the update,
// one launch per bucket)
constexpr int kLarsMaxBufs = 16;
// Elements one block of lars_sumsq_f32 reduces: a chunk never crosses a
// tensor boundary, so a tensor of n elements owns ceil(n / kLarsChunk)
// chunks. 8 float4 per lane and array; the largest ResNet50_vd tensor
// (2.36M elements) owns 288 chunks, which one wave of lars_trust_f32 sums.
constexpr int kLarsChunk = 8192;
constexpr int kLarsChunkFields = 4;  // int32 {bucket, start, len, 0} per chunk
// Chunk partials one wave of lars_trust_f32 loads before it starts adding;
// a tensor with more chunks takes another pass of the same loop.
constexpr int kLarsTrustPreload = 512;
struct LarsBufs {  // passed to the kernel by value
  const float* p[kLarsMaxBufs];
  const float* g[kLarsMaxBufs];
  long long n[kLarsMaxBufs];
  int first;  // bucket index of slot 0 (the chunk table counts all buckets)
  int nbuf;
};
// partial: double [2 * chunks] = {sum p^2, sum g^2} per chunk; the launch
// writes chunks [chunk_base, chunk_base + nchunks)
void launch_lars_sumsq_f32(const LarsBufs* bufs, const int* chunks,
                           int chunk_base, int nchunks, double* partial,
                           hipStream_t stream);
// tensor_chunks: int32 {first chunk, chunk count} per tensor
void launch_lars_trust_f32(const double* partial, const int* tensor_chunks,
                           int ntensors, int nchunks_total, double coeff,
                           double wd, double eps, float grad_scale,
                           const float* clip, float* trust,
                           hipStream_t stream);
// segment tables as fused_adam's (at most kAdamMaxSegments), plus
// seg_tensor: the slot of `trust` a segment reads
void launch_fused_lars_f32(float* p, const float* g, float* v,
                           const float* lr_dev, float lr, float mu,
                           float scale, long long n, const int* seg_end,
                           const float* seg_wd, const int* seg_tensor,
                           int nseg, const float* trust, int ntensors,
                           const float* clip, hipStream_t stream);

// ---- kd_loss.hip ----
void launch_kd_ce_fwd_f32(const float* s, const float* t, float* lpr, int B,
                          int C, hipStream_t stream);
void launch_kd_ce_bwd_f32(const float* s, const float* t, float* ds,
                          float gob, int B, int C, hipStream_t stream);
void launch_kd_ce_fwd_bf16(const void* s, const void* t, float* lpr, int B,
                           int C, hipStream_t stream);
void launch_kd_ce_bwd_bf16(const void* s, const void* t, void* ds, float gob,
                           int B, int C, hipStream_t stream);

// ---- softmax_ce.hip ---- (bwd: lse comes BEFORE the labels; eps, inv_B)
void launch_softmax_ce_fwd(const void* s, int is_bf16, const long long* ya,
                           const long long* yb, const float* lam,
                           float* loss_row, float* lse, int* rank, float eps,
                           int B, int C, hipStream_t stream);
void launch_softmax_ce_bwd(const void* s, int is_bf16, const float* lse,
                           const long long* ya, const long long* yb,
                           const float* lam, const float* gout, void* ds,
                           float eps, float inv_B, int B, int C,
                           hipStream_t stream);

// ---- bnrelu.hip ---- (M is long long, C int; the accumulators go
// db_acc THEN dg_acc; the *_pad launchers take Nimg, H, W, C as ints)
int bn_stats_grid(long long M, int C);
int bn_bwd_grid(long long M, int C);
void launch_bn_stats(const void* x, float* partial, int grid, long long M,
                     int C, hipStream_t s);
void launch_bn_finalize(float* partial, int nblocks, int zero_src,
                        const float* gamma, const float* beta, float* mean,
                        float* invstd, float* scale, float* shift,
                        float* rmean, float* rvar, float momentum, float eps,
                        long long M, int C, hipStream_t s);
void launch_bn_apply(const void* x, const void* res, void* y,
                     unsigned char* mask, const float* scale,
                     const float* shift, long long M, int C, bool relu,
                     bool add, hipStream_t s);
void launch_bn_apply_pad(const void* x, void* yp, unsigned char* mask,
                         const float* scale, const float* shift, int Nimg,
                         int H, int W, int C, hipStream_t s);
void launch_bn_bwd_reduce(const void* dy, const unsigned char* mask,
                          const void* x, const float* mean,
                          const float* invstd, float* partial, int grid,
                          long long M, int C, bool relu, hipStream_t s);
void launch_bn_bwd_finalize(const float* partial, int nblocks, float* sums,
                            int C, float* db_acc, float* dg_acc,
                            hipStream_t s);
void launch_bn_bwd_dx(const void* dy, const unsigned char* mask,
                      const void* x, const float* mean, const float* invstd,
                      const float* gamma, const float* sums, void* dx,
                      void* dres, long long M, int C, bool relu, bool add,
                      bool training, hipStream_t s);
void launch_bn_bwd_dx_pad(const void* dy, const unsigned char* mask,
                          const void* x, const float* mean,
                          const float* invstd, const float* gamma,
                          const float* sums, void* dxp, int Nimg, int H,
                          int W, int C, bool relu, hipStream_t s);
void launch_bn_bwd_fused(const void* dy, const unsigned char* mask,
                         const void* x, const float* mean,
                         const float* invstd, const float* gamma,
                         float* partial, float* sums, float* db_acc,
                         float* dg_acc, void* dx, void* dres, int* ws,
                         int grid, int nfin, long long M, int C, bool relu,
                         bool add, hipStream_t s);

// ---- gemm_bt.hip ---- (M, N, K: C[M,N] = A[M,K] @ B[N,K]^T)
int gemm_bt_tiles_m(int M, int N);
void launch_gemm_bt(const void* A, const void* B, void* C, int M, int N,
                    int K, float* bn_part, hipStream_t s);
// C = bf16(float(bf16(A @ B^T)) + float(R)), R bf16 [M, N] laid out like C
void launch_gemm_bt_add(const void* A, const void* B, const void* R, void* C,
                        int M, int N, int K, hipStream_t s);
// C = bf16(relu?(fma(float(bf16(A @ B^T)), scale[n], shift[n]) [+ R])): the
// eval BN(+Add)+ReLU apply in the epilogue. R (bf16 [M, N] like C, or null)
// comes BEFORE C as in launch_gemm_bt_add; scale, shift fp32 [N] after K
void launch_gemm_bt_bn(const void* A, const void* B, const void* R, void* C,
                       int M, int N, int K, const float* scale,
                       const float* shift, bool relu, hipStream_t s);
void launch_gemm_bt_splitk(const void* A, const void* B, float* Cf32, int M,
                           int N, int K, int splitk, hipStream_t s);

// ---- conv3x3.hip ---- (dense/grouped take Cout BEFORE Cin, the s2 dgrad
// Cin before Cout; HW_out, W_out, Hp, Wp, stride always in that order)
int conv3x3_tiles_m(int M, int Cout);
int conv3x3_small_tiles_m(int M);
int conv3x3_pick_splitk(int M, int Cout, int Cin);
void launch_pad_nhwc(const void* x, void* xp, int Nimg, int H, int W, int Hp,
                     int Wp, int C, hipStream_t s);
void launch_pad_nhwc_cpad(const void* x, void* xp, int Nimg, int H, int W,
                          int Hp, int Wp, int Creal, int Cpad,
                          hipStream_t s);
void launch_conv3x3(const void* xp, const void* w3, void* y, int M, int Cout,
                    int Cin, int HW_out, int W_out, int Hp, int Wp,
                    int stride, float* cpart, int splitk, float* bn_part,
                    hipStream_t s);
void launch_conv3x3_grouped(const void* xp, const void* w3g, void* y, int M,
                            int Cout, int Cin, int HW_out, int W_out, int Hp,
                            int Wp, int stride, int gw, hipStream_t s);
// the _bn twins: the eval BN(+ReLU) apply in the epilogue, non-split only;
// scale, shift (fp32 [Cout]) and relu follow the geometry (and gw)
void launch_conv3x3_bn(const void* xp, const void* w3, void* y, int M,
                       int Cout, int Cin, int HW_out, int W_out, int Hp,
                       int Wp, int stride, const float* scale,
                       const float* shift, bool relu, hipStream_t s);
void launch_conv3x3_grouped_bn(const void* xp, const void* w3g, void* y,
                               int M, int Cout, int Cin, int HW_out,
                               int W_out, int Hp, int Wp, int stride, int gw,
                               const float* scale, const float* shift,
                               bool relu, hipStream_t s);
void launch_conv3x3_small(const void* xp, const void* w3s, void* y, int M,
                          int Cout_real, int cpt, int HW_out, int W_out,
                          int Hp, int Wp, int stride, float* bn_part,
                          hipStream_t s);
void launch_conv3x3s2_dgrad(const void* dyp, const void* wcat, void* dx,
                            int Nimg, int H, int W, int Cin, int Cout,
                            int Hop, int Wop, hipStream_t s);

// ---- gemm_tn.hip ---- (3x3: Cout, Cin, M, then Ho, Wo, Hp, Wp; the small
// launcher puts CinP BEFORE stride, the others end stride, splitk, perm)
void launch_gemm_tn_splitk(const void* A, const void* B, float* C, int N1,
                           int N2, int K, int splitk, hipStream_t s);
void launch_gemm_tn3x3_splitk(const void* dy, const void* xpad, float* C,
                              int Cout, int Cin, int M, int Ho, int Wo,
                              int Hp, int Wp, int stride, int splitk,
                              int perm, hipStream_t s);
void launch_gemm_tn3x3_splitk_apad(const void* dyp, const void* xpad,
                                   float* C, int Cout, int Cin, int M, int Ho,
                                   int Wo, int Hp, int Wp, int stride,
                                   int splitk, int perm, hipStream_t s);
void launch_gemm_tn3x3_small(const void* dy, const void* xpad, float* C,
                             int N1v, int N2v, int M, int Ho, int Wo, int Hp,
                             int Wp, int CinP, int stride, int splitk,
                             hipStream_t s);

// ---- transpose.hip ---- (shift9: M, C, Mp first, then the conv geometry)
void launch_transpose_pad(const void* in, void* out, int M, int C, int Mp,
                          hipStream_t s);
void launch_shift9_transpose(const void* xp, void* out, int M, int C, int Mp,
                             int HW_out, int W_out, int Hp, int Wp,
                             int stride, hipStream_t s);
void launch_repack_dgrad_w3(const void* in, void* out, int Co, int Ci,
                            int mode, hipStream_t s);
void launch_cast_bf16_zero(float* src, void* dst, long long n, hipStream_t s);

// ---- maxpool.hip ---- (input extent H, W before output extent Ho, Wo)
void launch_maxpool3x3s2_fwd(const void* x, void* y, unsigned char* idx,
                             int N, int H, int W, int Ho, int Wo, int C,
                             hipStream_t s);
void launch_maxpool3x3s2_bwd(const void* dy, const unsigned char* idx,
                             void* dx, int N, int H, int W, int Ho, int Wo,
                             int C, hipStream_t s);

// ---- avgpool.hip ---- (as maxpool: H, W, Ho, Wo, C)
void launch_avgpool2x2_fwd(const void* x, void* y, int N, int H, int W,
                           int Ho, int Wo, int C, hipStream_t s);
void launch_avgpool2x2_bwd(const void* dy, void* dx, int N, int H, int W,
                           int Ho, int Wo, int C, hipStream_t s);

// ---- dgc.hip ---- (n is long long; compact's k is unsigned, scatter's
// long long)
int dgc_workspace_words();
void launch_dgc_accumulate(const float* g, float* u, float* v,
                           const float* p, float mu, float wd, long long n,
                           unsigned* ws, int hist_copies, hipStream_t stream);
void launch_dgc_hist(const float* v, long long n, unsigned* ws, int pass,
                     hipStream_t stream);
void launch_dgc_pick(unsigned* ws, int pass, unsigned k, hipStream_t stream);
void launch_dgc_compact(float* v, float* u, long long n, int* payload,
                        unsigned k, unsigned* ws, hipStream_t stream);
void launch_dgc_scatter_add(float* out, long long n, const int* payload,
                            long long k, hipStream_t stream);

// ---- image_prep.hip ---- (crop + bilinear resize + mirror + normalize of B
// decoded uint8 RGB images into one channels-last batch [B, S, S, 3])
// packed: the sources (HWC, 3 bytes per pixel, rows dense) back to back at
// any byte offsets, nbytes in all (3 <= nbytes < 2^31). table: one row of
// kImagePrepFields int32 per image, 16-byte aligned:
//   [0] byte offset of the source in packed   [1] H   [2] W   [3] flip (0/1)
//   [4..7] the fp32 BITS of x0, y0, cw, ch: the source window in pixel
//          units, fractional allowed, cw, ch > 0
// The kernel clamps every tap into the image and every byte index into
// packed, whatever the table holds; the caller still checks the host copy
// (ops/image_prep.py). k3 = 1/(255*std), b3 = mean/std: host fp32[3], read
// before the launcher returns.
constexpr int kImagePrepFields = 8;
constexpr int kImagePrepRun = 4;   // consecutive output pixels per thread
constexpr int kImagePrepRows = 4;  // output rows a thread walks
int image_prep_blocks_per_image(int S);
void launch_image_prep(const unsigned char* packed, long long nbytes,
                       const int* table, void* out, int B, int S,
                       int out_bf16, const float* k3, const float* b3,
                       hipStream_t stream);

}  // extern "C"
