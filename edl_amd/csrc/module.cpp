// Python bindings for the edl_amd CDNA4 kernel layer (edl_amd._C).
// Compiled by hipcc directly (no hipify, no CUDA path) — see build_hip.py.
#include <iterator>
#include <mutex>
#include <unordered_map>
#include <unordered_set>
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <c10/util/FunctionRef.h>
#include <hip/hip_runtime.h>

#include "launchers.h"  // every launcher of the .hip translation units

namespace {

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// ---- checks and arithmetic the bindings share ----------------------------

// x must be a 4-D channels_last bf16 GPU tensor; cmod > 0 additionally
// requires C % cmod == 0 (sites that check no modulus pass none)
void check_nhwc_bf16(const torch::Tensor& x, const char* who, int cmod = 0) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 &&
                  x.scalar_type() == torch::kBFloat16 &&
                  x.is_contiguous(torch::MemoryFormat::ChannelsLast),
              who, ": 4-D channels_last bf16 GPU tensor required");
  TORCH_CHECK(cmod <= 0 || x.size(1) % cmod == 0, who, ": C % ", cmod);
}

// output extent of a 3x3 pad-1 conv (or ceil-mode stride-2 pool)
int out_extent(int64_t in, int64_t stride) {
  return (int)((in - 1) / stride + 1);
}

// split-K pick: total blocks ~ 2x CUs, at most `upper` k-slices
int64_t auto_splitk(int tiles, int64_t upper) {
  const int64_t sk = std::max<int64_t>(1, 512 / std::max(1, tiles));
  return std::min(sk, upper);
}

// a [M, K] and b [N, K]: 2-D bf16 GPU operands of a bt GEMM, K, N % 64
void check_bt_operands(const torch::Tensor& a, const torch::Tensor& b,
                       const char* who) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.dim() == 2 && b.dim() == 2 &&
                  a.size(1) == b.size(1),
              who, ": [M,K] x [N,K] GPU tensors required");
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 &&
                  b.scalar_type() == torch::kBFloat16,
              who, ": bf16 only");
  TORCH_CHECK(a.size(1) % 64 == 0 && b.size(0) % 64 == 0, who,
              ": K,N % 64 == 0");
}

// n-tiles of the TN kernels along one output dim (n % 64 == 0)
int tn_tiles(int n) { return n / (n % 128 == 0 ? 128 : 64); }

// wgrad target: the caller's fp32 buffer of rows*cols elements to
// ACCUMULATE into (direct-grad mode: the param's bucket-view gradient,
// pre-zeroed by reducer.zero_grad — no fresh zeros tensor, no
// AccumulateGrad add afterwards), else fresh zeros [rows, cols]
torch::Tensor out_or_zeros(const c10::optional<torch::Tensor>& out,
                           int64_t rows, int64_t cols,
                           torch::TensorOptions opts, const char* msg) {
  if (!out.has_value())
    return torch::zeros({rows, cols}, opts.dtype(torch::kFloat32));
  TORCH_CHECK(out->is_contiguous() &&
                  out->scalar_type() == torch::kFloat32 &&
                  out->numel() == rows * cols,
              msg);
  return *out;
}

// optional fp32 [C] accumulator (direct-grad mode) -> pointer or null
float* acc_ptr(const c10::optional<torch::Tensor>& acc, int64_t C,
               const char* msg) {
  if (!acc.has_value()) return nullptr;
  TORCH_CHECK(acc->numel() == C && acc->is_contiguous() &&
                  acc->scalar_type() == torch::kFloat32,
              msg);
  return acc->data_ptr<float>();
}

// pad_hw = (H, W) of the [M, C] rows' images -> (N, H, W) of the zero-halo
// padded buffer [N, H+2, W+2, C]
struct PadNHW {
  int64_t n = 0, h = 0, w = 0;
};

PadNHW parse_pad_hw(const std::vector<int64_t>& pad_hw, long long M,
                    const char* who) {
  TORCH_CHECK(pad_hw.size() == 2, who, ": pad_hw = (H, W)");
  PadNHW p;
  p.h = pad_hw[0];
  p.w = pad_hw[1];
  TORCH_CHECK(p.h >= 1 && p.w >= 1 && M >= 1 && M % (p.h * p.w) == 0, who,
              ": pad_hw does not divide the rows of x");
  p.n = M / (p.h * p.w);
  TORCH_CHECK(p.n * (p.h + 2) * (p.w + 2) < (1LL << 31), who,
              ": padded pixel count must stay below 2^31");
  return p;
}

// ---- DGC top-k compress / decode (dgc.hip) -------------------------------
void dgc_check_flat(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                  t.dim() == 1 && t.is_contiguous(),
              "dgc: ", name, " must be a flat contiguous fp32 GPU tensor");
  TORCH_CHECK(t.numel() >= 1 && t.numel() < (1LL << 31),
              "dgc: 1 <= n < 2^31 required for ", name);
}

unsigned* dgc_ws_ptr(const torch::Tensor& ws, const torch::Tensor& like) {
  TORCH_CHECK(ws.is_cuda() && ws.device() == like.device() &&
                  ws.scalar_type() == torch::kInt32 && ws.is_contiguous() &&
                  ws.numel() == dgc_workspace_words(),
              "dgc: workspace must be the int32 GPU tensor of "
              "dgc_workspace_words() zeros");
  return reinterpret_cast<unsigned*>(ws.data_ptr<int>());
}

void dgc_check_k(int64_t k, const torch::Tensor& v) {
  TORCH_CHECK(k >= 1 && k <= v.numel(), "dgc: 1 <= k <= n required");
}

int* dgc_payload_ptr(const torch::Tensor& payload, int64_t k,
                     const torch::Tensor& like) {
  TORCH_CHECK(payload.is_cuda() && payload.device() == like.device() &&
                  payload.scalar_type() == torch::kInt32 &&
                  payload.is_contiguous() && payload.dim() == 2 &&
                  payload.size(0) == 2 && payload.size(1) == k,
              "dgc: payload must be a contiguous int32 [2, k] GPU tensor");
  return payload.data_ptr<int>();
}

void dgc_accumulate(torch::Tensor g, torch::Tensor u, torch::Tensor v,
                    c10::optional<torch::Tensor> p, double mu, double wd,
                    torch::Tensor ws, int64_t hist_copies) {
  // u = mu*u + (g + wd*p); v += u; histogram of the top 11 bits of |v|
  dgc_check_flat(g, "g");
  dgc_check_flat(u, "u");
  dgc_check_flat(v, "v");
  TORCH_CHECK(g.numel() == u.numel() && g.numel() == v.numel() &&
                  g.device() == u.device() && g.device() == v.device(),
              "dgc: g, u, v must match in size and device");
  const float* pp = nullptr;
  if (p.has_value()) {
    dgc_check_flat(*p, "p");
    TORCH_CHECK(p->numel() == g.numel() && p->device() == g.device(),
                "dgc: p must match g");
    pp = p->data_ptr<float>();
  }
  TORCH_CHECK(hist_copies == 1 || hist_copies == 4, "dgc: hist_copies 1 or 4");
  launch_dgc_accumulate(g.data_ptr<float>(), u.data_ptr<float>(),
                        v.data_ptr<float>(), pp, (float)mu, (float)wd,
                        (long long)g.numel(), dgc_ws_ptr(ws, g),
                        (int)hist_copies, cur_stream());
}

void dgc_hist(torch::Tensor v, torch::Tensor ws, int64_t pass) {
  dgc_check_flat(v, "v");
  TORCH_CHECK(pass == 1 || pass == 2, "dgc_hist: pass 1 or 2");
  launch_dgc_hist(v.data_ptr<float>(), (long long)v.numel(),
                  dgc_ws_ptr(ws, v), (int)pass, cur_stream());
}

void dgc_pick(torch::Tensor v, torch::Tensor ws, int64_t pass, int64_t k) {
  dgc_check_flat(v, "v");
  dgc_check_k(k, v);
  TORCH_CHECK(pass >= 0 && pass <= 2, "dgc_pick: pass 0..2");
  launch_dgc_pick(dgc_ws_ptr(ws, v), (int)pass, (unsigned)k, cur_stream());
}

void dgc_compact(torch::Tensor v, torch::Tensor u, torch::Tensor payload,
                 torch::Tensor ws) {
  dgc_check_flat(v, "v");
  dgc_check_flat(u, "u");
  TORCH_CHECK(u.numel() == v.numel() && u.device() == v.device(),
              "dgc: u must match v");
  const int64_t k = payload.dim() == 2 ? payload.size(1) : -1;
  dgc_check_k(k, v);
  launch_dgc_compact(v.data_ptr<float>(), u.data_ptr<float>(),
                     (long long)v.numel(), dgc_payload_ptr(payload, k, v),
                     (unsigned)k, dgc_ws_ptr(ws, v), cur_stream());
}

void dgc_select(torch::Tensor v, torch::Tensor u, torch::Tensor payload,
                torch::Tensor ws) {
  // everything after dgc_accumulate: pick 0, (hist, pick) x 2, compact
  const int64_t k = payload.dim() == 2 ? payload.size(1) : -1;
  dgc_pick(v, ws, 0, k);
  dgc_hist(v, ws, 1);
  dgc_pick(v, ws, 1, k);
  dgc_hist(v, ws, 2);
  dgc_pick(v, ws, 2, k);
  dgc_compact(v, u, payload, ws);
}

void dgc_scatter_add(torch::Tensor out, torch::Tensor payload) {
  // out[idx] += val for one rank's payload; idx < 0 (empty slot) is skipped
  dgc_check_flat(out, "out");
  const int64_t k = payload.dim() == 2 ? payload.size(1) : -1;
  TORCH_CHECK(k >= 1, "dgc: payload must be int32 [2, k]");
  launch_dgc_scatter_add(out.data_ptr<float>(), (long long)out.numel(),
                         dgc_payload_ptr(payload, k, out), (long long)k,
                         cur_stream());
}

// optional fp32[4] clip state [coef, norm, skip, nskipped] on `like`'s
// device (grad_norm.hip writes it, the update kernels read it) -> pointer
// or null
float* clip_state_ptr(const c10::optional<torch::Tensor>& st,
                      const torch::Tensor& like, const char* who) {
  if (!st.has_value()) return nullptr;
  TORCH_CHECK(st->is_cuda() && st->device() == like.device() &&
                  st->scalar_type() == torch::kFloat32 &&
                  st->is_contiguous() && st->numel() == kGradClipStateLen,
              who, ": clip_state must be a contiguous fp32[",
              kGradClipStateLen, "] tensor on the buffers' device");
  return st->data_ptr<float>();
}

// ---- flat-bucket update kernels (fused_sgd/adam/lars.hip): shared checks --

// p, g and the state buffers of one bucket: GPU, fp32, contiguous, equal
// numel, one device, 16-byte aligned (the kernels walk them as float4)
// -> numel
long long check_flat_f32(const char* who,
                         std::initializer_list<const torch::Tensor*> ts) {
  const torch::Tensor& p = **ts.begin();
  for (const torch::Tensor* t : ts)
    TORCH_CHECK(t->is_cuda(), who, ": GPU tensors required");
  for (const torch::Tensor* t : ts)
    TORCH_CHECK(t->scalar_type() == torch::kFloat32, who, ": fp32 only");
  for (const torch::Tensor* t : ts)
    TORCH_CHECK(t->is_contiguous(), who,
                ": contiguous flat buffers required");
  for (const torch::Tensor* t : ts)
    TORCH_CHECK(t->numel() == p.numel(), who, ": size mismatch");
  for (const torch::Tensor* t : ts)
    TORCH_CHECK(t->device() == p.device(), who,
                ": the flat buffers must share a device");
  for (const torch::Tensor* t : ts)
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, who,
                ": the flat buffers must be 16-byte aligned (float4)");
  return (long long)p.numel();
}

// optional fp32 LR scalar on `like`'s device -> pointer or null
const float* lr_dev_ptr(const c10::optional<torch::Tensor>& lr_dev,
                        const torch::Tensor& like, const char* who) {
  if (!lr_dev.has_value()) return nullptr;
  TORCH_CHECK(lr_dev->is_cuda() && lr_dev->device() == like.device() &&
                  lr_dev->scalar_type() == torch::kFloat32 &&
                  lr_dev->numel() == 1,
              who, ": lr_dev must be a fp32 GPU scalar");
  return lr_dev->data_ptr<float>();
}

// A table that lives on the device costs a D2H sync to check: a table
// TENSOR is checked on its first eager launch and again whenever its
// version counter or `key` (the extent it was checked against) changes.
// The record holds a weak reference to the tensor (which pins the tensor's
// header, never its storage), so a record cannot pass for a new tensor that
// lands on the same address, and the kind of check that passed, so a tensor
// checked as one table cannot pass for another. A launch under stream
// capture cannot sync and skips the check: the optimizers check the host
// lists they build their tables from, and the kernels clamp every table
// value, so even an unchecked table cannot read out of bounds.
enum class TableKind { kSegEnd, kSegTensor, kLarsChunks, kLarsTensorChunks };

struct TableSeen {
  c10::weak_intrusive_ptr<c10::TensorImpl> impl;
  uint32_t version;
  long long key;
  TableKind kind;
};

void check_device_table(
    const torch::Tensor& table, TableKind kind, long long key,
    const char* who, c10::function_ref<void(const int*, int64_t)> check) {
  static std::mutex mu;
  static std::unordered_map<const c10::TensorImpl*, TableSeen> seen;
  std::lock_guard<std::mutex> lock(mu);
  const c10::TensorImpl* id = table.unsafeGetTensorImpl();
  const uint32_t version = table._version();
  auto it = seen.find(id);
  // a live weak reference pins the TensorImpl's address: same id, same
  // tensor
  if (it != seen.end() && !it->second.impl.expired() &&
      it->second.version == version && it->second.key == key &&
      it->second.kind == kind)
    return;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  TORCH_CHECK(hipStreamIsCapturing(cur_stream(), &cap) == hipSuccess, who,
              ": hipStreamIsCapturing failed");
  if (cap != hipStreamCaptureStatusNone) return;
  auto host = table.cpu();
  check(host.data_ptr<int>(), host.numel());
  for (auto e = seen.begin(); e != seen.end();)  // drop dead tensors' records
    e = e->second.impl.expired() ? seen.erase(e) : std::next(e);
  seen.insert_or_assign(
      id, TableSeen{c10::weak_intrusive_ptr<c10::TensorImpl>(
                        table.getIntrusivePtr()),
                    version, key, kind});
}

// The per-bucket segment table of fused_adam / fused_lars over a bucket of
// n elements: seg_end (int32, cumulative ends, last == n) and seg_wd (fp32)
// come together or not at all, seg_tensor (int32) only with them -> the
// number of segments, 0 without a table
int check_seg_table(const char* who, const torch::Tensor& p, long long n,
                    const torch::Tensor* seg_end, const torch::Tensor* seg_wd,
                    const torch::Tensor* seg_tensor = nullptr) {
  TORCH_CHECK((seg_end != nullptr) == (seg_wd != nullptr), who,
              ": seg_end and seg_wd come together");
  if (seg_end == nullptr) return 0;
  for (const torch::Tensor* t : {seg_end, seg_wd, seg_tensor})
    TORCH_CHECK(t == nullptr ||
                    (t->is_cuda() && t->device() == p.device() &&
                     t->is_contiguous() && t->dim() == 1 &&
                     t->scalar_type() ==
                         (t == seg_wd ? torch::kFloat32 : torch::kInt32)),
                who, ": seg_end, seg_tensor int32 / seg_wd fp32 flat GPU "
                     "tensors on the buffers' device");
  const int64_t nseg = seg_end->numel();
  TORCH_CHECK(seg_wd->numel() == nseg &&
                  (seg_tensor == nullptr || seg_tensor->numel() == nseg),
              who, ": seg_end, seg_wd, seg_tensor differ in length");
  TORCH_CHECK(nseg >= 1 && nseg <= kAdamMaxSegments, who,
              ": 1 <= segments <= ", kAdamMaxSegments, " per bucket (got ",
              nseg, ")");
  TORCH_CHECK(n < (1LL << 31), who, ": a segment table needs numel < 2^31");
  check_device_table(*seg_end, TableKind::kSegEnd, n, who,
                     [&](const int* e, int64_t cnt) {
    int prev = 0;
    for (int64_t k = 0; k < cnt; ++k) {
      TORCH_CHECK(e[k] >= prev, who, ": seg_end must not decrease");
      prev = e[k];
    }
    TORCH_CHECK(prev == n, who, ": last seg_end (", prev,
                ") must equal numel (", n, ")");
  });
  return (int)nseg;
}

void fused_sgd(torch::Tensor p, torch::Tensor g, torch::Tensor m, double lr,
               double momentum, double weight_decay, double grad_scale,
               c10::optional<torch::Tensor> lr_dev,
               c10::optional<torch::Tensor> clip_state) {
  const long long n = check_flat_f32("fused_sgd", {&p, &g, &m});
  launch_fused_sgd_f32(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                       (float)lr, (float)momentum, (float)weight_decay,
                       (float)grad_scale, n, lr_dev_ptr(lr_dev, p, "fused_sgd"),
                       clip_state_ptr(clip_state, p, "fused_sgd"),
                       cur_stream());
}

// ---- fused Adam / AdamW (fused_adam.hip) ---------------------------------

void fused_adam(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                torch::Tensor v, torch::Tensor step_dev, double lr,
                double beta1, double beta2, double eps, double weight_decay,
                double grad_scale, bool decoupled,
                c10::optional<torch::Tensor> lr_dev,
                c10::optional<torch::Tensor> seg_end,
                c10::optional<torch::Tensor> seg_wd,
                c10::optional<torch::Tensor> clip_state) {
  const long long n = check_flat_f32("fused_adam", {&p, &g, &m, &v});
  TORCH_CHECK(step_dev.is_cuda() && step_dev.device() == p.device() &&
                  step_dev.scalar_type() == torch::kInt32 &&
                  step_dev.numel() == 1,
              "fused_adam: step_dev must be an int32 GPU scalar");
  TORCH_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
              "fused_adam: betas must lie in [0, 1)");
  const float* lrp = lr_dev_ptr(lr_dev, p, "fused_adam");
  const int nseg = check_seg_table(
      "fused_adam", p, n, seg_end.has_value() ? &*seg_end : nullptr,
      seg_wd.has_value() ? &*seg_wd : nullptr);
  const int* endp = nseg ? seg_end->data_ptr<int>() : nullptr;
  const float* wdp = nseg ? seg_wd->data_ptr<float>() : nullptr;
  const float* clipp = clip_state_ptr(clip_state, p, "fused_adam");
  if (n == 0) return;
  // 1-b and ln b in double: the float forms lose ~6e-5 relative on 1-b2
  launch_fused_adam_f32(
      p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
      v.data_ptr<float>(), step_dev.data_ptr<int>(), lrp, (float)lr,
      (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
      (float)std::log(beta1), (float)std::log(beta2), (float)eps,
      (float)weight_decay, (float)grad_scale, decoupled ? 1 : 0, n, endp, wdp,
      nseg, clipp, cur_stream());
}

// ---- global gradient norm / clip state (grad_norm.hip) --------------------

// -> partial rows of the buffers, in order (what grad_sumsq writes)
int64_t grad_norm_rows_total(const std::vector<torch::Tensor>& bufs) {
  int64_t total = 0;
  for (const auto& b : bufs) total += grad_norm_rows((long long)b.numel());
  return total;
}

// partial[row] = sum of squares (double) of a slice of one buffer; every row
// of [0, rows_total) is written. More than kGradNormMaxSegs buffers take
// further launches of the same kernel. -> rows_total
int64_t grad_sumsq(std::vector<torch::Tensor> bufs, torch::Tensor partial) {
  const int64_t rows_total = grad_norm_rows_total(bufs);
  TORCH_CHECK(partial.is_cuda() && partial.scalar_type() == torch::kFloat64 &&
                  partial.is_contiguous() && partial.numel() >= rows_total,
              "grad_sumsq: partial must be a contiguous fp64 GPU tensor of "
              "at least ", rows_total, " rows (grad_norm_rows per buffer)");
  for (const auto& b : bufs) {
    TORCH_CHECK(b.is_cuda(), "grad_sumsq: GPU tensors required");
    TORCH_CHECK(b.scalar_type() == torch::kFloat32, "grad_sumsq: fp32 only");
    TORCH_CHECK(b.is_contiguous(),
                "grad_sumsq: contiguous flat buffers required");
    TORCH_CHECK(b.device() == partial.device(),
                "grad_sumsq: buffers and partial must share a device");
    TORCH_CHECK(b.numel() >= 0, "grad_sumsq: n >= 0");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(b.data_ptr()) % 16 == 0,
                "grad_sumsq: buffers must be 16-byte aligned (float4)");
  }
  auto s = cur_stream();
  int row = 0;
  for (size_t base = 0; base < bufs.size(); base += kGradNormMaxSegs) {
    GradNormSegs segs = {};
    const size_t cnt = std::min<size_t>(kGradNormMaxSegs, bufs.size() - base);
    segs.nseg = (int)cnt;
    for (size_t k = 0; k < cnt; ++k) {
      const auto& b = bufs[base + k];
      segs.ptr[k] = b.numel() ? b.data_ptr<float>() : nullptr;
      segs.n[k] = (long long)b.numel();
      segs.rows[k] = grad_norm_rows(segs.n[k]);
      segs.row_off[k] = row;
      row += segs.rows[k];
    }
    launch_grad_sumsq_f32(&segs, partial.data_ptr<double>(), s);
  }
  return rows_total;
}

// state = [coef, norm, skip, nskipped] from partial[0 .. rows_total)
void grad_clip_finalize(torch::Tensor partial, int64_t rows_total,
                        torch::Tensor state, double grad_scale,
                        double max_norm, bool skip_nonfinite) {
  TORCH_CHECK(partial.is_cuda() && partial.scalar_type() == torch::kFloat64 &&
                  partial.is_contiguous(),
              "grad_clip_finalize: partial must be a contiguous fp64 GPU "
              "tensor");
  TORCH_CHECK(rows_total >= 0 && rows_total <= partial.numel() &&
                  rows_total < (1LL << 31),
              "grad_clip_finalize: 0 <= rows_total <= partial.numel()");
  TORCH_CHECK(state.is_cuda() && state.device() == partial.device() &&
                  state.scalar_type() == torch::kFloat32 &&
                  state.is_contiguous() &&
                  state.numel() == kGradClipStateLen,
              "grad_clip_finalize: state must be a contiguous fp32[",
              kGradClipStateLen, "] tensor on partial's device");
  TORCH_CHECK(max_norm >= 0.0, "grad_clip_finalize: max_norm >= 0 (inf = "
                               "norm only)");
  launch_grad_clip_finalize(partial.data_ptr<double>(), (int)rows_total,
                            grad_scale, (float)max_norm,
                            skip_nonfinite ? 1 : 0, state.data_ptr<float>(),
                            cur_stream());
}

// ---- fused LARS (fused_lars.hip) ------------------------------------------

void lars_check_int_table(const torch::Tensor& t, const torch::Tensor& like,
                          const char* who, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() &&
                  t.scalar_type() == torch::kInt32 && t.is_contiguous() &&
                  reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              who, ": ", what,
              " must be a contiguous, 16-byte aligned int32 tensor on the "
              "buffers' device");
}

// partial[2c], partial[2c+1] = sums of squares (double) of p and g over
// chunk c of `chunks` (int32 [nchunks, 4] = {bucket, start, len, 0}, sorted
// by bucket; bucket_chunk_off[b] = first chunk of bucket b, one more entry
// than buckets). Every chunk's pair is written. More than kLarsMaxBufs
// buckets take further launches of the same kernel. -> nchunks
int64_t lars_sumsq(std::vector<torch::Tensor> ps, std::vector<torch::Tensor> gs,
                   torch::Tensor chunks,
                   std::vector<int64_t> bucket_chunk_off,
                   torch::Tensor partial) {
  const size_t nb = ps.size();
  TORCH_CHECK(gs.size() == nb && bucket_chunk_off.size() == nb + 1,
              "lars_sumsq: one g and one chunk offset per p, plus the end");
  TORCH_CHECK(partial.is_cuda() && partial.scalar_type() == torch::kFloat64 &&
                  partial.is_contiguous() &&
                  reinterpret_cast<uintptr_t>(partial.data_ptr()) % 16 == 0,
              "lars_sumsq: partial must be a contiguous, 16-byte aligned "
              "fp64 GPU tensor");
  lars_check_int_table(chunks, partial, "lars_sumsq", "chunks");
  TORCH_CHECK(chunks.dim() == 2 && chunks.size(1) == kLarsChunkFields,
              "lars_sumsq: chunks must be int32 [nchunks, ",
              kLarsChunkFields, "]");
  const int64_t nchunks = chunks.size(0);
  TORCH_CHECK(nchunks < (1LL << 30) && partial.numel() >= 2 * nchunks,
              "lars_sumsq: partial needs 2 slots per chunk (", 2 * nchunks,
              ")");
  TORCH_CHECK(bucket_chunk_off[0] == 0 && bucket_chunk_off[nb] == nchunks,
              "lars_sumsq: bucket_chunk_off must run from 0 to nchunks");
  long long total = 0;
  for (size_t b = 0; b < nb; ++b) {
    TORCH_CHECK(bucket_chunk_off[b] <= bucket_chunk_off[b + 1],
                "lars_sumsq: bucket_chunk_off must not decrease");
    for (const torch::Tensor* t : {&ps[b], &gs[b]}) {
      TORCH_CHECK(t->is_cuda() && t->device() == partial.device(),
                  "lars_sumsq: buffers and partial must share a GPU");
      TORCH_CHECK(t->scalar_type() == torch::kFloat32, "lars_sumsq: fp32 only");
      TORCH_CHECK(t->is_contiguous(),
                  "lars_sumsq: contiguous flat buffers required");
      TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                  "lars_sumsq: buffers must be 16-byte aligned (float4)");
    }
    TORCH_CHECK(ps[b].numel() == gs[b].numel() &&
                    ps[b].numel() < (1LL << 31),
                "lars_sumsq: p and g of a bucket must agree, numel < 2^31");
    total += (long long)ps[b].numel();
  }
  check_device_table(chunks, TableKind::kLarsChunks, total, "lars_sumsq",
                     [&](const int* e, int64_t) {
    int prev = 0;
    for (int64_t c = 0; c < nchunks; ++c, e += kLarsChunkFields) {
      TORCH_CHECK(e[0] >= prev && e[0] < (int64_t)nb &&
                      c >= bucket_chunk_off[e[0]] &&
                      c < bucket_chunk_off[e[0] + 1],
                  "lars_sumsq: chunk ", c, " names bucket ", e[0],
                  " outside its bucket_chunk_off range");
      prev = e[0];
      TORCH_CHECK(e[1] >= 0 && e[2] >= 0 && e[2] <= kLarsChunk &&
                      (int64_t)e[1] + e[2] <= ps[e[0]].numel(),
                  "lars_sumsq: chunk ", c, " [", e[1], ", +", e[2],
                  ") leaves its bucket or exceeds ", kLarsChunk, " elements");
    }
  });
  auto s = cur_stream();
  for (size_t base = 0; base < nb; base += kLarsMaxBufs) {
    LarsBufs bufs = {};
    const size_t cnt = std::min<size_t>(kLarsMaxBufs, nb - base);
    bufs.first = (int)base;
    bufs.nbuf = (int)cnt;
    for (size_t k = 0; k < cnt; ++k) {
      const auto& p = ps[base + k];
      bufs.p[k] = p.numel() ? p.data_ptr<float>() : nullptr;
      bufs.g[k] = p.numel() ? gs[base + k].data_ptr<float>() : nullptr;
      bufs.n[k] = (long long)p.numel();
    }
    const int64_t lo = bucket_chunk_off[base], hi = bucket_chunk_off[base + cnt];
    launch_lars_sumsq_f32(&bufs, chunks.data_ptr<int>(), (int)lo,
                          (int)(hi - lo), partial.data_ptr<double>(), s);
  }
  return nchunks;
}

// trust[k] = coeff*pn/(gn + wd*pn + eps) from the chunk partials of tensor k
// (tensor_chunks: int32 [ntensors, 2] = {first chunk, count}); 1.0 for a
// tensor without chunks or with pn, gn or wd not > 0. Every slot is written.
void lars_trust(torch::Tensor partial, int64_t nchunks,
                torch::Tensor tensor_chunks, torch::Tensor trust,
                double lars_coeff, double lars_weight_decay, double epsilon,
                double grad_scale, c10::optional<torch::Tensor> clip_state) {
  TORCH_CHECK(partial.is_cuda() && partial.scalar_type() == torch::kFloat64 &&
                  partial.is_contiguous() &&
                  reinterpret_cast<uintptr_t>(partial.data_ptr()) % 16 == 0,
              "lars_trust: partial must be a contiguous, 16-byte aligned "
              "fp64 GPU tensor");
  TORCH_CHECK(nchunks >= 0 && nchunks < (1LL << 30) &&
                  2 * nchunks <= partial.numel(),
              "lars_trust: 0 <= 2 * nchunks <= partial.numel()");
  lars_check_int_table(tensor_chunks, partial, "lars_trust", "tensor_chunks");
  TORCH_CHECK(tensor_chunks.dim() == 2 && tensor_chunks.size(1) == 2 &&
                  tensor_chunks.size(0) >= 1 &&
                  tensor_chunks.size(0) < (1LL << 30),
              "lars_trust: tensor_chunks must be int32 [ntensors >= 1, 2]");
  const int64_t nt = tensor_chunks.size(0);
  TORCH_CHECK(trust.is_cuda() && trust.device() == partial.device() &&
                  trust.scalar_type() == torch::kFloat32 &&
                  trust.is_contiguous() && trust.numel() >= nt,
              "lars_trust: trust must be a contiguous fp32 tensor of at "
              "least ntensors slots on partial's device");
  TORCH_CHECK(lars_coeff >= 0.0 && lars_weight_decay >= 0.0 && epsilon >= 0.0,
              "lars_trust: lars_coeff, lars_weight_decay, epsilon >= 0");
  check_device_table(tensor_chunks, TableKind::kLarsTensorChunks, nchunks,
                     "lars_trust", [&](const int* e, int64_t) {
    for (int64_t k = 0; k < nt; ++k, e += 2)
      TORCH_CHECK(e[0] >= 0 && e[1] >= 0 && (int64_t)e[0] + e[1] <= nchunks,
                  "lars_trust: tensor ", k, " owns chunks [", e[0], ", +",
                  e[1], ") of ", nchunks);
  });
  launch_lars_trust_f32(partial.data_ptr<double>(),
                        tensor_chunks.data_ptr<int>(), (int)nt, (int)nchunks,
                        lars_coeff, lars_weight_decay, epsilon,
                        (float)grad_scale,
                        clip_state_ptr(clip_state, partial, "lars_trust"),
                        trust.data_ptr<float>(), cur_stream());
}

void fused_lars(torch::Tensor p, torch::Tensor g, torch::Tensor v, double lr,
                double momentum, double grad_scale, torch::Tensor seg_end,
                torch::Tensor seg_wd, torch::Tensor seg_tensor,
                torch::Tensor trust, c10::optional<torch::Tensor> lr_dev,
                c10::optional<torch::Tensor> clip_state) {
  const long long n = check_flat_f32("fused_lars", {&p, &g, &v});
  const float* lrp = lr_dev_ptr(lr_dev, p, "fused_lars");
  // 16-byte aligned int tables, as fused_lars (not fused_adam) asks
  lars_check_int_table(seg_end, p, "fused_lars", "seg_end");
  lars_check_int_table(seg_tensor, p, "fused_lars", "seg_tensor");
  const int nseg =
      check_seg_table("fused_lars", p, n, &seg_end, &seg_wd, &seg_tensor);
  TORCH_CHECK(trust.is_cuda() && trust.device() == p.device() &&
                  trust.scalar_type() == torch::kFloat32 &&
                  trust.is_contiguous() && trust.numel() >= 1 &&
                  trust.numel() < (1LL << 31),
              "fused_lars: trust must be a non-empty contiguous fp32 tensor "
              "on the buffers' device");
  check_device_table(seg_tensor, TableKind::kSegTensor, trust.numel(),
                     "fused_lars", [&](const int* e, int64_t cnt) {
    for (int64_t k = 0; k < cnt; ++k)
      TORCH_CHECK(e[k] >= 0 && e[k] < trust.numel(),
                  "fused_lars: seg_tensor[", k, "] = ", e[k],
                  " is no slot of trust (", trust.numel(), ")");
  });
  const float* clipp = clip_state_ptr(clip_state, p, "fused_lars");
  if (n == 0) return;
  launch_fused_lars_f32(p.data_ptr<float>(), g.data_ptr<float>(),
                        v.data_ptr<float>(), lrp, (float)lr, (float)momentum,
                        (float)grad_scale, n, seg_end.data_ptr<int>(),
                        seg_wd.data_ptr<float>(), seg_tensor.data_ptr<int>(),
                        nseg, trust.data_ptr<float>(),
                        (int)trust.numel(), clipp, cur_stream());
}

torch::Tensor kd_ce_forward(torch::Tensor s, torch::Tensor t) {
  TORCH_CHECK(s.is_cuda() && t.is_cuda(), "kd_ce: GPU tensors required");
  TORCH_CHECK(s.dim() == 2 && t.sizes() == s.sizes(), "kd_ce: [B,C] logits expected");
  TORCH_CHECK(s.scalar_type() == t.scalar_type(), "kd_ce: dtype mismatch");
  auto sc = s.contiguous();
  auto tc = t.contiguous();
  const int B = (int)s.size(0), C = (int)s.size(1);
  auto lpr = torch::empty({B}, s.options().dtype(torch::kFloat32));
  if (s.scalar_type() == torch::kFloat32) {
    launch_kd_ce_fwd_f32(sc.data_ptr<float>(), tc.data_ptr<float>(),
                         lpr.data_ptr<float>(), B, C, cur_stream());
  } else if (s.scalar_type() == torch::kBFloat16) {
    launch_kd_ce_fwd_bf16(sc.data_ptr(), tc.data_ptr(), lpr.data_ptr<float>(), B, C,
                          cur_stream());
  } else {
    TORCH_CHECK(false, "kd_ce: fp32/bf16 only");
  }
  return lpr;
}

torch::Tensor kd_ce_backward(torch::Tensor s, torch::Tensor t, double gout_over_B) {
  auto sc = s.contiguous();
  auto tc = t.contiguous();
  const int B = (int)s.size(0), C = (int)s.size(1);
  auto ds = torch::empty_like(sc);
  if (s.scalar_type() == torch::kFloat32) {
    launch_kd_ce_bwd_f32(sc.data_ptr<float>(), tc.data_ptr<float>(), ds.data_ptr<float>(),
                         (float)gout_over_B, B, C, cur_stream());
  } else if (s.scalar_type() == torch::kBFloat16) {
    launch_kd_ce_bwd_bf16(sc.data_ptr(), tc.data_ptr(), ds.data_ptr(),
                          (float)gout_over_B, B, C, cur_stream());
  } else {
    TORCH_CHECK(false, "kd_ce: fp32/bf16 only");
  }
  return ds;
}

// shared argument checks of softmax_ce_forward/backward; returns the
// (y_b, lam) device pointers, both null without mixup
std::pair<const long long*, const float*> check_softmax_ce_inputs(
    const torch::Tensor& s, const torch::Tensor& ya,
    const c10::optional<torch::Tensor>& yb,
    const c10::optional<torch::Tensor>& lam) {
  TORCH_CHECK(s.is_cuda() && ya.device() == s.device(),
              "softmax_ce: logits and labels on one GPU required");
  TORCH_CHECK(s.dim() == 2 && s.size(0) >= 1 && s.size(1) >= 1,
              "softmax_ce: [B,C] logits expected");
  TORCH_CHECK(s.scalar_type() == torch::kFloat32 ||
                  s.scalar_type() == torch::kBFloat16,
              "softmax_ce: fp32/bf16 only");
  TORCH_CHECK(s.is_contiguous(), "softmax_ce: contiguous logits required");
  TORCH_CHECK(s.numel() < (1LL << 31), "softmax_ce: B*C < 2^31");
  const int64_t B = s.size(0);
  TORCH_CHECK(ya.scalar_type() == torch::kInt64 && ya.dim() == 1 &&
                  ya.numel() == B && ya.is_contiguous(),
              "softmax_ce: labels must be contiguous int64 [B]");
  TORCH_CHECK(yb.has_value() == lam.has_value(),
              "softmax_ce: labels_b and lam go together");
  if (!yb.has_value()) return {nullptr, nullptr};
  TORCH_CHECK(yb->is_cuda() && yb->scalar_type() == torch::kInt64 &&
                  yb->dim() == 1 && yb->numel() == B && yb->is_contiguous(),
              "softmax_ce: labels_b must be contiguous int64 [B] on the GPU");
  TORCH_CHECK(lam->is_cuda() && lam->scalar_type() == torch::kFloat32 &&
                  lam->dim() == 1 && lam->numel() == B && lam->is_contiguous(),
              "softmax_ce: lam must be contiguous fp32 [B] on the GPU");
  return {(const long long*)yb->data_ptr<int64_t>(), lam->data_ptr<float>()};
}

std::vector<torch::Tensor> softmax_ce_forward(torch::Tensor s, torch::Tensor ya,
                                              c10::optional<torch::Tensor> yb,
                                              c10::optional<torch::Tensor> lam,
                                              double eps) {
  // -> (loss_row f32 [B], lse f32 [B], rank i32 [B]); see softmax_ce.hip
  auto mix = check_softmax_ce_inputs(s, ya, yb, lam);
  const int B = (int)s.size(0), C = (int)s.size(1);
  auto opts = s.options().dtype(torch::kFloat32);
  auto loss_row = torch::empty({B}, opts);
  auto lse = torch::empty({B}, opts);
  auto rank = torch::empty({B}, s.options().dtype(torch::kInt32));
  launch_softmax_ce_fwd(s.data_ptr(), s.scalar_type() == torch::kBFloat16,
                        (const long long*)ya.data_ptr<int64_t>(), mix.first,
                        mix.second, loss_row.data_ptr<float>(),
                        lse.data_ptr<float>(), rank.data_ptr<int>(), (float)eps,
                        B, C, cur_stream());
  return {loss_row, lse, rank};
}

torch::Tensor softmax_ce_backward(torch::Tensor s, torch::Tensor lse,
                                  torch::Tensor ya,
                                  c10::optional<torch::Tensor> yb,
                                  c10::optional<torch::Tensor> lam, double eps,
                                  torch::Tensor gout, double inv_B) {
  // gout: DEVICE fp32 scalar (no host read, so the call is graph-capturable)
  auto mix = check_softmax_ce_inputs(s, ya, yb, lam);
  const int B = (int)s.size(0), C = (int)s.size(1);
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == torch::kFloat32 &&
                  lse.numel() == B && lse.is_contiguous(),
              "softmax_ce: lse must be contiguous fp32 [B] on the GPU");
  TORCH_CHECK(gout.is_cuda() && gout.scalar_type() == torch::kFloat32 &&
                  gout.numel() == 1,
              "softmax_ce: gout must be a fp32 GPU scalar");
  auto ds = torch::empty_like(s);
  launch_softmax_ce_bwd(s.data_ptr(), s.scalar_type() == torch::kBFloat16,
                        lse.data_ptr<float>(),
                        (const long long*)ya.data_ptr<int64_t>(), mix.first,
                        mix.second, gout.data_ptr<float>(), ds.data_ptr(),
                        (float)eps, (float)inv_B, B, C, cur_stream());
  return ds;
}

static std::unordered_set<const void*>& pooled_ptr_set() {
  static std::unordered_set<const void*> ptrs;
  return ptrs;
}

static torch::Tensor part_pool_get(int rows, int64_t cols,
                                   torch::TensorOptions opts) {
  // Capped BN-stats partial buffers are accumulated with atomics, so they
  // must start zeroed. Pool them per (device, shape): zeroed ONCE here,
  // and bn_finalize(zero_src=1) stores zeros back after reading, so reuse
  // needs no per-step fill launch. If a producer's partials are ever
  // dropped unconsumed, the Python side zeroes them (bnrelu.forward).
  static std::unordered_map<int64_t, torch::Tensor> pool;
  const int64_t key = ((int64_t)opts.device().index() << 48) |
                      ((int64_t)rows << 28) | cols;
  auto it = pool.find(key);
  if (it != pool.end()) return it->second;
  auto t = torch::zeros({rows, cols}, opts);
  pool.emplace(key, t);
  pooled_ptr_set().insert(t.data_ptr());
  return t;
}

// fp32 [min(tiles_m, cap), cols] stats-partial buffer for a fused epilogue:
// capped (atomically folded) partials come from the pre-zeroed pool, the
// rest are written once per row and can be transient
torch::Tensor stats_part_buf(int tiles_m, int64_t cols,
                             torch::TensorOptions opts) {
  opts = opts.dtype(torch::kFloat32);
  const int rows = std::min(tiles_m, kStatsPartRowCap);
  return tiles_m > rows ? part_pool_get(rows, cols, opts)
                        : torch::empty({rows, cols}, opts);
}

// x: NHWC bf16 viewed as [M, C] contiguous (channels_last 4-D collapses to
// this). gamma/beta/running stats: fp32 [C].
void check_bn_inputs_eval(const torch::Tensor& x, int64_t C) {
  // eval apply is elementwise — no channel cap (ResNeXt101_32x16d
  // stage-4 BNs are 4096-wide)
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16,
              "bn: bf16 GPU tensor required");
  TORCH_CHECK(C % 8 == 0, "bn: C % 8 == 0 required, got ", C);
}

void check_bn_inputs(const torch::Tensor& x, int64_t C) {
  check_bn_inputs_eval(x, C);
  // the training stats/reduce kernels stage 2*C fp32 in LDS
  TORCH_CHECK(C <= 2048, "bn: C <= 2048 supported");
  // and partition rows by C/8 threads of a 256-thread block (bnrelu.hip
  // row_partition): exact only when C/8 divides 256
  TORCH_CHECK((C & (C - 1)) == 0,
              "bn: training needs a power-of-two C (8..2048): the stats and "
              "reduce kernels split each 256-thread block into C/8-thread "
              "rows; got ", C);
}

std::vector<torch::Tensor> bn_fwd_train(torch::Tensor x, torch::Tensor gamma,
                                        torch::Tensor beta, torch::Tensor rmean,
                                        torch::Tensor rvar, double momentum,
                                        double eps,
                                        c10::optional<torch::Tensor> res,
                                        bool relu,
                                        c10::optional<torch::Tensor> pre_part,
                                        c10::optional<std::vector<int64_t>> pad_hw) {
  // x: [M, C] contiguous view of an NHWC tensor (Python side reshapes).
  // pad_hw = (H, W): y is returned as the zero-halo padded buffer
  // [N, H+2, W+2, C] the 3x3 implicit-GEMM kernels read (relu, no res).
  const int64_t C = gamma.numel();
  TORCH_CHECK(x.dim() == 2 && x.size(1) == C && x.is_contiguous(),
              "bn: x must be a contiguous [M, C] view");
  check_bn_inputs(x, C);
  const long long M = x.numel() / C;
  PadNHW pad;  // pad.n == 0: plain [M, C] output
  if (pad_hw.has_value()) {
    TORCH_CHECK(relu && !res.has_value(),
                "bn: pad_hw needs relu and no residual");
    pad = parse_pad_hw(*pad_hw, M, "bn");
  }
  auto opts = gamma.options().dtype(torch::kFloat32);
  const int grid = bn_stats_grid(M, (int)C);
  auto partial = torch::empty({grid, 2 * C}, opts);
  auto mean = torch::empty({C}, opts);
  auto invstd = torch::empty({C}, opts);
  auto scale = torch::empty({C}, opts);
  auto shift = torch::empty({C}, opts);
  auto y = pad.n ? torch::empty({pad.n, pad.h + 2, pad.w + 2, C}, x.options())
                 : torch::empty_like(x);
  // 1-bit/channel ReLU mask for the backward (one byte per channel octet)
  auto msk = relu ? torch::empty({M, C / 8}, x.options().dtype(torch::kUInt8))
                  : torch::empty({0}, x.options().dtype(torch::kUInt8));
  auto s = cur_stream();
  int fin_grid = grid;
  if (pre_part.has_value()) {
    // stats already folded into the producing conv's epilogue
    // ([tiles_m, 2C] fp32, conv3x3.hip BN_PART) — skip the stats kernel
    // (a full activation re-read)
    TORCH_CHECK(pre_part->is_contiguous() &&
                    pre_part->scalar_type() == torch::kFloat32 &&
                    pre_part->dim() == 2 && pre_part->size(1) == 2 * C,
                "bn: pre_part [tiles, 2C] fp32");
    partial = *pre_part;
    fin_grid = (int)pre_part->size(0);
  } else {
    launch_bn_stats(x.data_ptr(), partial.data_ptr<float>(), grid, M, (int)C,
                    s);
  }
  // zero-after-read ONLY for pooled buffers (capped partials): transient
  // uncapped partials are discarded, zeroing them is pure write waste
  const int zero_src =
      pre_part.has_value() &&
      pooled_ptr_set().count((const void*)partial.data_ptr());
  launch_bn_finalize(partial.data_ptr<float>(), fin_grid,
                     zero_src, gamma.data_ptr<float>(),
                     beta.data_ptr<float>(), mean.data_ptr<float>(),
                     invstd.data_ptr<float>(), scale.data_ptr<float>(),
                     shift.data_ptr<float>(),
                     rmean.defined() ? rmean.data_ptr<float>() : nullptr,
                     rvar.defined() ? rvar.data_ptr<float>() : nullptr,
                     (float)momentum, (float)eps, M, (int)C, s);
  if (pad.n) {
    launch_bn_apply_pad(x.data_ptr(), y.data_ptr(),
                        (unsigned char*)msk.data_ptr(),
                        scale.data_ptr<float>(), shift.data_ptr<float>(),
                        (int)pad.n, (int)pad.h, (int)pad.w, (int)C, s);
  } else {
    launch_bn_apply(x.data_ptr(), res.has_value() ? res->data_ptr() : nullptr,
                    y.data_ptr(),
                    relu ? (unsigned char*)msk.data_ptr() : nullptr,
                    scale.data_ptr<float>(), shift.data_ptr<float>(), M,
                    (int)C, relu, res.has_value(), s);
  }
  return {y, mean, invstd, msk};
}

torch::Tensor bn_fwd_eval(torch::Tensor x, torch::Tensor scale, torch::Tensor shift,
                          c10::optional<torch::Tensor> res, bool relu) {
  const int64_t C = scale.numel();
  check_bn_inputs_eval(x, C);
  const long long M = x.numel() / C;
  auto y = torch::empty_like(x);
  launch_bn_apply(x.data_ptr(), res.has_value() ? res->data_ptr() : nullptr,
                  y.data_ptr(), nullptr,
                  scale.data_ptr<float>(), shift.data_ptr<float>(),
                  M, (int)C, relu, res.has_value(), cur_stream());
  return y;
}

std::vector<torch::Tensor> bn_bwd(torch::Tensor dy, c10::optional<torch::Tensor> msk,
                                  torch::Tensor x,
                                  torch::Tensor mean, torch::Tensor invstd,
                                  torch::Tensor gamma, bool relu, bool add,
                                  bool training,
                                  c10::optional<torch::Tensor> dgamma_acc,
                                  c10::optional<torch::Tensor> dbeta_acc,
                                  c10::optional<std::vector<int64_t>> pad_hw) {
  // pad_hw = (H, W): dx comes back as the zero-halo padded buffer
  // [N, H+2, W+2, C] (training, no residual, three-kernel route only; the
  // single-launch EDL_BN_BWD_FUSED route returns the plain [M, C] dx and
  // the caller tells the two apart by dx.dim()).
  const int64_t C = gamma.numel();
  check_bn_inputs(x, C);
  const long long M = x.numel() / C;
  auto opts = gamma.options().dtype(torch::kFloat32);
  const int grid = bn_bwd_grid(M, (int)C);
  auto sums = torch::empty({2, C}, opts);
  // read per call (not static) so tests can A/B via os.environ
  const char* fenv = getenv("EDL_BN_BWD_FUSED");
  const bool fused_bwd = fenv ? atoi(fenv) != 0 : false;
  PadNHW pad;  // pad.n == 0: plain [M, C] dx
  if (pad_hw.has_value() && !(fused_bwd && training)) {
    TORCH_CHECK(training && !add, "bn_bwd: pad_hw needs training, no residual");
    pad = parse_pad_hw(*pad_hw, M, "bn_bwd");
  }
  auto dx = pad.n ? torch::empty({pad.n, pad.h + 2, pad.w + 2, C}, x.options())
                  : torch::empty_like(x);
  auto dres = add ? torch::empty_like(x) : torch::Tensor();
  auto s = cur_stream();
  auto dyc = dy.is_contiguous() ? dy : dy.contiguous();
  TORCH_CHECK(!relu || (msk.has_value() && msk->numel() == M * (C / 8)),
              "bn_bwd: relu path needs the fwd mask");
  const unsigned char* mp =
      relu ? (const unsigned char*)msk->data_ptr() : nullptr;
  // direct-grad mode: accumulate dgamma/dbeta straight into the params'
  // bucket-view gradients (skips the per-param AccumulateGrad kernels)
  float* dg_acc = acc_ptr(dgamma_acc, C, "bn_bwd: dgamma_acc fp32 [C]");
  float* db_acc = acc_ptr(dbeta_acc, C, "bn_bwd: dbeta_acc fp32 [C]");
  if (fused_bwd && training) {
    // one launch: reduce + last-block finalize + dx (grid-wide flag sync);
    // ws = persistent per-device {arrive, flag, depart} ints, self-resetting
    static std::unordered_map<int, torch::Tensor> ws_pool;
    const int dev = (int)x.device().index();
    auto wit = ws_pool.find(dev);
    if (wit == ws_pool.end())
      wit = ws_pool.emplace(dev, torch::zeros({4},
          x.options().dtype(torch::kInt32))).first;
    // grid: big enough for the dx phase to saturate HBM (the reduce-grid
    // cap of 192 starved phase 2 by 3-7x in the v1 cut), bounded at 512 =
    // the co-residency guarantee of __launch_bounds__(256, 2) on 256 CUs
    // (the rendezvous spins cannot deadlock)
    const long long total8 = M * (C / 8);
    int fgrid = (int)((total8 + 1023) / 1024);
    if (fgrid < grid) fgrid = grid;
    if (fgrid > 512) fgrid = 512;
    // parallel finalize: slice 2C across up to 8 blocks, >=256 ch each
    int nfin = (int)(2 * C) / 256;
    if (nfin < 1) nfin = 1;
    if (nfin > 8) nfin = 8;
    auto fpartial = torch::empty({fgrid, 2 * C}, opts);
    launch_bn_bwd_fused(dyc.data_ptr(), mp, x.data_ptr(),
                        mean.data_ptr<float>(), invstd.data_ptr<float>(),
                        gamma.data_ptr<float>(), fpartial.data_ptr<float>(),
                        sums.data_ptr<float>(), db_acc, dg_acc, dx.data_ptr(),
                        add ? dres.data_ptr() : nullptr,
                        wit->second.data_ptr<int>(), fgrid, nfin, M, (int)C,
                        relu, add, s);
    return {dx, sums[1], sums[0], dres};
  }
  auto partial = torch::empty({grid, 2 * C}, opts);
  launch_bn_bwd_reduce(dyc.data_ptr(), mp, x.data_ptr(),
                       mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       partial.data_ptr<float>(), grid, M, (int)C, relu, s);
  launch_bn_bwd_finalize(partial.data_ptr<float>(), grid, sums.data_ptr<float>(),
                         (int)C, db_acc, dg_acc, s);
  if (pad.n) {
    launch_bn_bwd_dx_pad(dyc.data_ptr(), mp, x.data_ptr(),
                         mean.data_ptr<float>(), invstd.data_ptr<float>(),
                         gamma.data_ptr<float>(), sums.data_ptr<float>(),
                         dx.data_ptr(), (int)pad.n, (int)pad.h, (int)pad.w,
                         (int)C, relu, s);
  } else {
    launch_bn_bwd_dx(dyc.data_ptr(), mp, x.data_ptr(), mean.data_ptr<float>(),
                     invstd.data_ptr<float>(), gamma.data_ptr<float>(),
                     sums.data_ptr<float>(), dx.data_ptr(),
                     add ? dres.data_ptr() : nullptr, M, (int)C, relu, add,
                     training, s);
  }
  // dbeta = sums[0], dgamma = sums[1] (views of the reduce workspace)
  return {dx, sums[1], sums[0], dres};
}

// C[M, N] = A[M, K] @ B[N, K]^T, bf16 row-major -> {C} or, with_stats,
// {C, BN stats partials [tiles_m, 2N] of the bf16-rounded output} (the
// following BN skips its stats kernel)
std::vector<torch::Tensor> gemm_bt_impl(const torch::Tensor& a,
                                        const torch::Tensor& b,
                                        bool with_stats) {
  check_bt_operands(a, b, "gemm_bt");
  auto ac = a.contiguous();
  auto bc = b.contiguous();
  const int M = (int)a.size(0), K = (int)a.size(1), N = (int)b.size(0);
  auto c = torch::empty({M, N}, a.options());
  torch::Tensor part;
  if (with_stats)
    part = stats_part_buf(gemm_bt_tiles_m(M, N), 2 * N, a.options());
  launch_gemm_bt(ac.data_ptr(), bc.data_ptr(), c.data_ptr(), M, N, K,
                 with_stats ? part.data_ptr<float>() : nullptr, cur_stream());
  return {c, part};  // part undefined without stats
}

torch::Tensor gemm_bt(torch::Tensor a, torch::Tensor b) {
  return gemm_bt_impl(a, b, false)[0];
}

std::vector<torch::Tensor> gemm_bt_stats(torch::Tensor a, torch::Tensor b) {
  return gemm_bt_impl(a, b, true);
}

// C = bf16(float(bf16(A @ B^T)) + float(R)): gemm_bt followed by a bf16 add,
// bit for bit, in one kernel (the 1x1 dgrad + residual-gradient sum). r is
// read in place and never written; no stats epilogue with it.
torch::Tensor gemm_bt_add(torch::Tensor a, torch::Tensor b, torch::Tensor r) {
  check_bt_operands(a, b, "gemm_bt_add");
  const int M = (int)a.size(0), K = (int)a.size(1), N = (int)b.size(0);
  TORCH_CHECK(r.scalar_type() == torch::kBFloat16, "gemm_bt_add: r bf16 only");
  TORCH_CHECK(r.is_cuda() && r.device() == a.device(),
              "gemm_bt_add: r on another device than a");
  TORCH_CHECK(r.dim() == 2 && r.size(0) == M && r.size(1) == N,
              "gemm_bt_add: r shape [M, N] required");
  TORCH_CHECK(r.is_contiguous(), "gemm_bt_add: r not contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(r.data_ptr()) % 16 == 0,
              "gemm_bt_add: r base not 16-byte aligned");
  auto ac = a.contiguous();
  auto bc = b.contiguous();
  auto c = torch::empty({M, N}, a.options());
  launch_gemm_bt_add(ac.data_ptr(), bc.data_ptr(), r.data_ptr(), c.data_ptr(),
                     M, N, K, cur_stream());
  return c;
}

// the eval-BN epilogue operands: scale, shift fp32 [N], dense, on like's
// device
void check_bn_affine(const torch::Tensor& scale, const torch::Tensor& shift,
                     int64_t N, const torch::Tensor& like, const char* who) {
  TORCH_CHECK(scale.scalar_type() == torch::kFloat32 &&
                  shift.scalar_type() == torch::kFloat32,
              who, ": scale/shift fp32 only");
  TORCH_CHECK(scale.is_cuda() && shift.is_cuda() &&
                  scale.device() == like.device() &&
                  shift.device() == like.device(),
              who, ": scale/shift on another device than the input");
  TORCH_CHECK(scale.dim() == 1 && shift.dim() == 1 && scale.size(0) == N &&
                  shift.size(0) == N,
              who, ": scale/shift shape [N] required, N = ", N);
  TORCH_CHECK(scale.is_contiguous() && shift.is_contiguous(), who,
              ": scale/shift not contiguous");
}

// y = bf16(relu?(fma(float(bf16(A @ B^T)), scale[n], shift[n]) [+ res])):
// gemm_bt followed by bn_fwd_eval, bit for bit, in one kernel (conv1x1 ->
// eval BN(+Add)+ReLU). res is read in place and never written.
torch::Tensor gemm_bt_bn(torch::Tensor a, torch::Tensor b, torch::Tensor scale,
                         torch::Tensor shift, bool relu,
                         c10::optional<torch::Tensor> res) {
  check_bt_operands(a, b, "gemm_bt_bn");
  const int M = (int)a.size(0), K = (int)a.size(1), N = (int)b.size(0);
  check_bn_affine(scale, shift, N, a, "gemm_bt_bn");
  if (res.has_value()) {
    const torch::Tensor& r = *res;
    TORCH_CHECK(r.scalar_type() == torch::kBFloat16,
                "gemm_bt_bn: res bf16 only");
    TORCH_CHECK(r.is_cuda() && r.device() == a.device(),
                "gemm_bt_bn: res on another device than a");
    TORCH_CHECK(r.dim() == 2 && r.size(0) == M && r.size(1) == N,
                "gemm_bt_bn: res shape [M, N] required");
    TORCH_CHECK(r.is_contiguous(), "gemm_bt_bn: res not contiguous");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(r.data_ptr()) % 16 == 0,
                "gemm_bt_bn: res base not 16-byte aligned");
  }
  auto ac = a.contiguous();
  auto bc = b.contiguous();
  auto c = torch::empty({M, N}, a.options());
  launch_gemm_bt_bn(ac.data_ptr(), bc.data_ptr(),
                    res.has_value() ? res->data_ptr() : nullptr, c.data_ptr(),
                    M, N, K, scale.data_ptr<float>(), shift.data_ptr<float>(),
                    relu, cur_stream());
  return c;
}

// flat zero-halo padded copy of x [N, C, H, W] channels_last bf16, widened
// to cpad >= C channels: N * (H+2) * (W+2) * cpad elements
torch::Tensor pad_nhwc_flat(const torch::Tensor& x, int cpad, hipStream_t s) {
  const int Nimg = (int)x.size(0), C = (int)x.size(1);
  const int H = (int)x.size(2), W = (int)x.size(3);
  const int Hp = H + 2, Wp = W + 2;
  auto xp = torch::empty({(long long)Nimg * Hp * Wp * cpad}, x.options());
  if (C == cpad) {
    launch_pad_nhwc(x.data_ptr(), xp.data_ptr(), Nimg, H, W, Hp, Wp, C, s);
  } else {
    launch_pad_nhwc_cpad(x.data_ptr(), xp.data_ptr(), Nimg, H, W, Hp, Wp, C,
                         cpad, s);
  }
  return xp;
}

// scale/shift given: the eval BN(+ReLU) apply rides in the kernel epilogue
torch::Tensor conv3x3_grouped_impl(const torch::Tensor& x,
                                   const torch::Tensor& w3g, int64_t stride,
                                   const torch::Tensor* scale,
                                   const torch::Tensor* shift, bool relu) {
  // grouped 3x3: w3g [Cout, 9*gw] where gw = the gemm group width —
  // channels-per-group when >= 64 (exact, zero wasted MFMA), else 64
  // with a block-diagonal zero-padded repack (conv.py _repack_w3_grouped)
  check_nhwc_bf16(x, "conv3x3g");
  const int Nimg = (int)x.size(0), Cin = (int)x.size(1);
  const int H = (int)x.size(2), W = (int)x.size(3);
  const int Cout = (int)w3g.size(0);
  TORCH_CHECK(w3g.size(1) % 9 == 0 && w3g.is_contiguous(), "conv3x3g: w3g");
  const int gw = (int)(w3g.size(1) / 9);
  TORCH_CHECK(gw % 64 == 0 && Cin % gw == 0, "conv3x3g: gw % 64, Cin % gw");
  TORCH_CHECK(Cin % 64 == 0 && Cout % 64 == 0 && Cin == Cout,
              "conv3x3g: C % 64, equal in/out");
  if (scale != nullptr)
    check_bn_affine(*scale, *shift, Cout, x, "conv3x3g_bn");
  const int Hout = out_extent(H, stride), Wout = out_extent(W, stride);
  const long long M = (long long)Nimg * Hout * Wout;
  auto s = cur_stream();
  auto xp = pad_nhwc_flat(x, Cin, s);
  auto y = torch::empty({M, Cout}, x.options());
  if (scale != nullptr)
    launch_conv3x3_grouped_bn(xp.data_ptr(), w3g.data_ptr(), y.data_ptr(),
                              (int)M, Cout, Cin, Hout * Wout, Wout, H + 2,
                              W + 2, (int)stride, gw, scale->data_ptr<float>(),
                              shift->data_ptr<float>(), relu, s);
  else
    launch_conv3x3_grouped(xp.data_ptr(), w3g.data_ptr(), y.data_ptr(),
                           (int)M, Cout, Cin, Hout * Wout, Wout, H + 2, W + 2,
                           (int)stride, gw, s);
  return y;
}

torch::Tensor conv3x3_grouped_fwd(torch::Tensor x, torch::Tensor w3g,
                                  int64_t stride) {
  return conv3x3_grouped_impl(x, w3g, stride, nullptr, nullptr, false);
}

torch::Tensor conv3x3_grouped_fwd_bn(torch::Tensor x, torch::Tensor w3g,
                                     int64_t stride, torch::Tensor scale,
                                     torch::Tensor shift, bool relu) {
  return conv3x3_grouped_impl(x, w3g, stride, &scale, &shift, relu);
}

// stem conv (small channels): x [N, Cin, H, W] channels_last bf16 with
// Cin <= cpt (cpt in {16,32,64}); w3s [64, TAPS_PAD*cpt] zero-padded
// repack (conv.py _repack_w3_small). Returns {y2d [M, cout_real]} or,
// with_stats, {y2d, BN stats partials [tiles_m, 2*cout_real]}.
std::vector<torch::Tensor> conv3x3_small_impl(const torch::Tensor& x,
                                              const torch::Tensor& w3s,
                                              int64_t cout_real, int64_t cpt,
                                              int64_t stride,
                                              bool with_stats) {
  check_nhwc_bf16(x, "conv3x3s");
  TORCH_CHECK(stride == 1 || stride == 2, "conv3x3s: stride 1 or 2");
  TORCH_CHECK(cpt == 16 || cpt == 32 || cpt == 64, "conv3x3s: cpt 16/32/64");
  const int Nimg = (int)x.size(0), Cin = (int)x.size(1);
  const int H = (int)x.size(2), W = (int)x.size(3);
  TORCH_CHECK(Cin <= cpt, "conv3x3s: Cin <= cpt");
  const int taps_pad = cpt == 16 ? 12 : (cpt == 32 ? 10 : 9);
  TORCH_CHECK(w3s.is_contiguous() && w3s.size(0) == 64 &&
                  w3s.size(1) == taps_pad * cpt,
              "conv3x3s: w3s [64, taps_pad*cpt]");
  TORCH_CHECK(cout_real >= 1 && cout_real <= 64, "conv3x3s: cout <= 64");
  const int Hout = out_extent(H, stride), Wout = out_extent(W, stride);
  const long long M = (long long)Nimg * Hout * Wout;
  auto s = cur_stream();
  auto xp = pad_nhwc_flat(x, (int)cpt, s);
  auto y = torch::empty({M, cout_real}, x.options());
  torch::Tensor bpart;
  if (with_stats)
    bpart = stats_part_buf(conv3x3_small_tiles_m((int)M), 2 * cout_real,
                           x.options());
  launch_conv3x3_small(xp.data_ptr(), w3s.data_ptr(), y.data_ptr(), (int)M,
                       (int)cout_real, (int)cpt, Hout * Wout, Wout, H + 2,
                       W + 2, (int)stride,
                       with_stats ? bpart.data_ptr<float>() : nullptr, s);
  return {y, bpart};  // bpart undefined without stats
}

torch::Tensor conv3x3_small_fwd(torch::Tensor x, torch::Tensor w3s,
                                int64_t cout_real, int64_t cpt,
                                int64_t stride) {
  return conv3x3_small_impl(x, w3s, cout_real, cpt, stride, false)[0];
}

std::vector<torch::Tensor> conv3x3_small_fwd_stats(torch::Tensor x,
                                                   torch::Tensor w3s,
                                                   int64_t cout_real,
                                                   int64_t cpt,
                                                   int64_t stride) {
  return conv3x3_small_impl(x, w3s, cout_real, cpt, stride, true);
}

// ---- zero-halo padded NHWC buffers -------------------------------------
// The 3x3 implicit-GEMM kernels read xp [N, H+2, W+2, C] with a zero
// halo. The *_padded entry points take such a buffer (from pad_nhwc below,
// or written directly by bn_fwd_train / bn_bwd with pad_hw) so a tensor is
// padded once per step instead of once per consumer; the unsuffixed entry
// points pad and forward to them.

// x: 4-D channels_last bf16 -> xp [N, H+2, W+2, C]
torch::Tensor pad_nhwc(torch::Tensor x) {
  check_nhwc_bf16(x, "pad_nhwc", 8);
  const int Nimg = (int)x.size(0), C = (int)x.size(1);
  const int H = (int)x.size(2), W = (int)x.size(3);
  auto xp = torch::empty({Nimg, H + 2, W + 2, C}, x.options());
  launch_pad_nhwc(x.data_ptr(), xp.data_ptr(), Nimg, H, W, H + 2, W + 2, C,
                  cur_stream());
  return xp;
}

void check_padded(const torch::Tensor& xp, int64_t H, int64_t W,
                  const char* who) {
  TORCH_CHECK(xp.is_cuda() && xp.dim() == 4 &&
                  xp.scalar_type() == torch::kBFloat16 && xp.is_contiguous(),
              who, ": xp must be a contiguous [N, H+2, W+2, C] bf16 buffer");
  TORCH_CHECK(H >= 1 && W >= 1 && xp.size(1) == H + 2 && xp.size(2) == W + 2,
              who, ": xp is not the padded layout of an H x W image");
}

torch::Tensor conv3x3s2_dgrad_padded(torch::Tensor dyp, torch::Tensor wcat,
                                     int64_t H, int64_t W) {
  // stride-2 3x3 same-pad dgrad (parity decomposition, conv3x3.hip).
  // dyp: zero-halo padded dY [N, Ho+2, Wo+2, Cout]; wcat: [Cin, 9*Cout]
  // (conv.py _repack_w3_s2dgrad). Returns dx2d [N*H*W, Cin] bf16.
  const int64_t Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  check_padded(dyp, Ho, Wo, "s2dgrad");
  const int Nimg = (int)dyp.size(0), Cout = (int)dyp.size(3);
  const int Cin = (int)(wcat.size(0));
  TORCH_CHECK(wcat.is_contiguous() && wcat.size(1) == 9 * Cout,
              "s2dgrad: wcat [Cin, 9*Cout]");
  TORCH_CHECK(Cin % 64 == 0 && Cout % 64 == 0, "s2dgrad: C % 64");
  auto dx = torch::empty({(long long)Nimg * H * W, Cin}, dyp.options());
  launch_conv3x3s2_dgrad(dyp.data_ptr(), wcat.data_ptr(), dx.data_ptr(), Nimg,
                         (int)H, (int)W, Cin, Cout, (int)Ho + 2, (int)Wo + 2,
                         cur_stream());
  return dx;
}

torch::Tensor conv3x3s2_dgrad(torch::Tensor dy, torch::Tensor wcat,
                              int64_t H, int64_t W) {
  // dy: [N, Cout, Ho, Wo] channels_last bf16 (pads, then the call above)
  check_nhwc_bf16(dy, "s2dgrad dy", 64);
  TORCH_CHECK((H + 1) / 2 == dy.size(2) && (W + 1) / 2 == dy.size(3),
              "s2dgrad: shape");
  return conv3x3s2_dgrad_padded(pad_nhwc(dy), wcat, H, W);
}

torch::Tensor repack_dgrad_w3(torch::Tensor w_smaj, int64_t ci,
                              int64_t mode) {
  // w_smaj: [Co, 9*Ci] bf16 contiguous (the channels-last mirror's
  // s-major view) -> [Ci, 9*Co]: mode 0 = rotated stride-1 dgrad
  // weights, mode 1 = the stride-2 parity-class wcat. One kernel
  // instead of flip + permute-copy + cast per conv per step.
  TORCH_CHECK(w_smaj.is_cuda() && w_smaj.scalar_type() == torch::kBFloat16 &&
                  w_smaj.is_contiguous() && w_smaj.dim() == 2 &&
                  w_smaj.size(1) == 9 * ci,
              "repack_dgrad_w3: [Co, 9*Ci] bf16");
  const int Co = (int)w_smaj.size(0);
  TORCH_CHECK(Co % 64 == 0 && ci % 64 == 0, "repack_dgrad_w3: C % 64");
  auto out = torch::empty({ci, (long long)9 * Co}, w_smaj.options());
  launch_repack_dgrad_w3(w_smaj.data_ptr(), out.data_ptr(), Co, (int)ci,
                         (int)mode, cur_stream());
  return out;
}

std::vector<torch::Tensor> maxpool3x3s2_fwd(torch::Tensor x) {
  check_nhwc_bf16(x, "maxpool3x3s2", 8);
  const int N = (int)x.size(0), C = (int)x.size(1);
  const int H = (int)x.size(2), W = (int)x.size(3);
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  auto y = torch::empty({N, C, Ho, Wo},
                        x.options().memory_format(torch::MemoryFormat::ChannelsLast));
  auto idx = torch::empty({(long long)N * Ho * Wo * C},
                          x.options().dtype(torch::kUInt8));
  launch_maxpool3x3s2_fwd(x.data_ptr(), y.data_ptr(),
                          idx.data_ptr<unsigned char>(), N, H, W, Ho, Wo, C,
                          cur_stream());
  return {y, idx};
}

torch::Tensor maxpool3x3s2_bwd(torch::Tensor dy, torch::Tensor idx,
                               int64_t H, int64_t W) {
  check_nhwc_bf16(dy, "maxpool3x3s2_bwd");  // idx is taken on trust
  const int N = (int)dy.size(0), C = (int)dy.size(1);
  const int Ho = (int)dy.size(2), Wo = (int)dy.size(3);
  auto dx = torch::empty({N, C, (long long)H, (long long)W},
                         dy.options().memory_format(torch::MemoryFormat::ChannelsLast));
  launch_maxpool3x3s2_bwd(dy.data_ptr(), idx.data_ptr<unsigned char>(),
                          dx.data_ptr(), N, (int)H, (int)W, Ho, Wo, C,
                          cur_stream());
  return dx;
}

torch::Tensor avgpool2x2_fwd(torch::Tensor x) {
  // x: 4-D channels_last bf16; 2x2 stride-2 ceil_mode pool
  check_nhwc_bf16(x, "avgpool2x2", 8);
  const int N = (int)x.size(0), C = (int)x.size(1);
  const int H = (int)x.size(2), W = (int)x.size(3);
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  auto y = torch::empty({N, C, Ho, Wo},
                        x.options().memory_format(torch::MemoryFormat::ChannelsLast));
  launch_avgpool2x2_fwd(x.data_ptr(), y.data_ptr(), N, H, W, Ho, Wo, C,
                        cur_stream());
  return y;
}

torch::Tensor avgpool2x2_bwd(torch::Tensor dy, int64_t H, int64_t W) {
  const int N = (int)dy.size(0), C = (int)dy.size(1);
  const int Ho = (int)dy.size(2), Wo = (int)dy.size(3);
  auto dyc = dy.contiguous(torch::MemoryFormat::ChannelsLast);
  auto dx = torch::empty({N, C, H, W},
                         dy.options().memory_format(torch::MemoryFormat::ChannelsLast));
  launch_avgpool2x2_bwd(dyc.data_ptr(), dx.data_ptr(), N, (int)H, (int)W, Ho,
                        Wo, C, cur_stream());
  return dx;
}

torch::Tensor conv3x3_wgrad_operand_padded(torch::Tensor xp, int64_t H,
                                           int64_t W, int64_t stride) {
  // xp: zero-halo padded conv input [N, H+2, W+2, Cin] -> [9*Cin, Mp]
  // shifted transpose.
  check_padded(xp, H, W, "wgrad_operand");
  TORCH_CHECK(stride == 1 || stride == 2, "wgrad_operand: stride 1 or 2");
  const int Nimg = (int)xp.size(0), Cin = (int)xp.size(3);
  const int Hp = (int)H + 2, Wp = (int)W + 2;
  const int Hout = out_extent(H, stride), Wout = out_extent(W, stride);
  const int M = Nimg * Hout * Wout;
  const int Mp = (M + 63) / 64 * 64;
  auto out = torch::empty({(long long)9 * Cin, Mp}, xp.options());
  launch_shift9_transpose(xp.data_ptr(), out.data_ptr(), M, Cin, Mp,
                          Hout * Wout, Wout, Hp, Wp, (int)stride,
                          cur_stream());
  return out;
}

torch::Tensor conv3x3_wgrad_operand(torch::Tensor x, int64_t stride) {
  // x: 4-D channels_last bf16 input of the conv (pads, then the call above)
  auto xp = pad_nhwc(x);
  return conv3x3_wgrad_operand_padded(xp, x.size(2), x.size(3), stride);
}

torch::Tensor gemm_bt_splitk(torch::Tensor a, torch::Tensor b, int64_t splitk) {
  // fp32 C[M,N] = A[M,K] @ B[N,K]^T with grid.y k-slices (atomic combine).
  check_bt_operands(a, b, "gemm_bt_splitk");
  auto ac = a.contiguous();
  auto bc = b.contiguous();
  const int M = (int)a.size(0), K = (int)a.size(1), N = (int)b.size(0);
  if (splitk <= 0) {
    // pick splitk so total blocks ~ 2x CUs, bounded by k-tiles
    const int tiles = ((M + 127) / 128) * ((N + 63) / 64);
    splitk = auto_splitk(tiles, K / 64);
  }
  auto c = torch::zeros({M, N}, a.options().dtype(torch::kFloat32));
  launch_gemm_bt_splitk(ac.data_ptr(), bc.data_ptr(), c.data_ptr<float>(), M, N,
                        K, (int)splitk, cur_stream());
  return c;
}

torch::Tensor gemm_tn_splitk(torch::Tensor a, torch::Tensor b, int64_t splitk,
                             c10::optional<torch::Tensor> out) {
  // fp32 C[N1,N2] = A[K,N1]^T @ B[K,N2] — conv wgrad WITHOUT the
  // transpose_pad materializations (operands in native activation layout)
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.dim() == 2 && b.dim() == 2 &&
                  a.size(0) == b.size(0),
              "gemm_tn_splitk: [K,N1] x [K,N2] GPU");
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 &&
                  b.scalar_type() == torch::kBFloat16,
              "gemm_tn_splitk: bf16 only");
  auto ac = a.contiguous();
  auto bc = b.contiguous();
  const int K = (int)a.size(0), N1 = (int)a.size(1), N2 = (int)b.size(1);
  TORCH_CHECK(N1 % 64 == 0 && N2 % 64 == 0, "gemm_tn_splitk: N1,N2 % 64");
  const int nchunks = (K + 63) / 64;
  if (splitk <= 0) splitk = auto_splitk(tn_tiles(N1) * tn_tiles(N2), nchunks);
  splitk = std::min<int64_t>(splitk, nchunks);
  auto c = out_or_zeros(out, N1, N2, a.options(),
                        "gemm_tn_splitk: out fp32 contiguous [N1,N2]");
  launch_gemm_tn_splitk(ac.data_ptr(), bc.data_ptr(), c.data_ptr<float>(), N1,
                        N2, K, (int)splitk, cur_stream());
  return c;
}

torch::Tensor gemm_tn3x3_splitk_padded(torch::Tensor dy, torch::Tensor xp,
                                       int64_t H64, int64_t W64,
                                       int64_t stride, int64_t splitk,
                                       c10::optional<torch::Tensor> out) {
  // conv3x3 wgrad, fully direct: fp32 dW3[Cout, 9*Cin] = dY^T @
  // gather3x3(xp) — no transpose_pad / shift9 materializations.
  // xp: zero-halo padded conv input [N, H+2, W+2, Cin] bf16.
  // dy: [M, Cout] bf16 (NHWC-flattened dY), or dY in its own zero-halo
  // padded layout [N, Ho+2, Wo+2, Cout] (4-D, as the BN backward writes
  // it), read through the kernel's A-operand row map.
  check_padded(xp, H64, W64, "gemm_tn3x3");
  TORCH_CHECK(stride == 1 || stride == 2, "gemm_tn3x3: stride 1 or 2");
  const bool dy_padded = dy.dim() == 4;
  TORCH_CHECK(dy.is_cuda() && (dy.dim() == 2 || dy_padded) &&
                  dy.scalar_type() == torch::kBFloat16,
              "gemm_tn3x3: dy [M,Cout] or padded [N,Ho+2,Wo+2,Cout] bf16");
  const int Nimg = (int)xp.size(0), Cin = (int)xp.size(3);
  const int H = (int)H64, W = (int)W64;
  const int Hp = H + 2, Wp = W + 2;
  const int Ho = out_extent(H, stride), Wo = out_extent(W, stride);
  const int M = Nimg * Ho * Wo;
  const int Cout = (int)dy.size(dy_padded ? 3 : 1);
  if (dy_padded) {
    check_padded(dy, Ho, Wo, "gemm_tn3x3 dy");
    TORCH_CHECK(dy.size(0) == Nimg, "gemm_tn3x3: dy batch != xp batch");
  } else {
    TORCH_CHECK((int)dy.size(0) == M, "gemm_tn3x3: dy2d rows != N*Ho*Wo");
  }
  TORCH_CHECK(Cin % 64 == 0 && Cout % 64 == 0, "gemm_tn3x3: C % 64");
  auto dyc = dy.contiguous();
  auto s = cur_stream();
  const int nchunks = (M + 63) / 64;
  if (splitk <= 0)
    splitk = auto_splitk(tn_tiles(Cout) * 9 * tn_tiles(Cin), nchunks);
  splitk = std::min<int64_t>(splitk, nchunks);
  auto c = out_or_zeros(out, Cout, 9 * Cin, xp.options(),
                        "gemm_tn3x3_splitk: out fp32 contiguous");
  // A 2-D [Cout, 9*Cin] target (channels-last bucket storage, or the fresh
  // zeros) takes the kernel's NATIVE s-major epilogue — coalesced; a
  // [Cout, Cin, 3, 3] one takes the perm remap (stride-9 scatter, kept
  // for the standard layout).
  const int perm = (c.dim() == 2 && c.size(1) == 9 * Cin) ? 0 : Cin;
  if (dy_padded)
    launch_gemm_tn3x3_splitk_apad(dyc.data_ptr(), xp.data_ptr(),
                                  c.data_ptr<float>(), Cout, Cin, M, Ho, Wo,
                                  Hp, Wp, (int)stride, (int)splitk, perm, s);
  else
    launch_gemm_tn3x3_splitk(dyc.data_ptr(), xp.data_ptr(),
                             c.data_ptr<float>(), Cout, Cin, M, Ho, Wo, Hp, Wp,
                             (int)stride, (int)splitk, perm, s);
  return c;
}

torch::Tensor gemm_tn3x3_splitk(torch::Tensor dy2d, torch::Tensor x,
                                int64_t stride, int64_t splitk,
                                c10::optional<torch::Tensor> out) {
  // dy2d: [M, Cout] bf16; x: 4-D channels_last bf16 (pads, then the call
  // above)
  TORCH_CHECK(dy2d.dim() == 2, "gemm_tn3x3: dy2d [M,Cout] bf16");
  auto xp = pad_nhwc(x);
  return gemm_tn3x3_splitk_padded(dy2d, xp, x.size(2), x.size(3), stride,
                                  splitk, out);
}

torch::Tensor transpose_pad(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 &&
                  x.scalar_type() == torch::kBFloat16 && x.is_contiguous(),
              "transpose_pad: contiguous 2-D bf16 GPU tensor");
  const int M = (int)x.size(0), C = (int)x.size(1);
  TORCH_CHECK(C % 8 == 0, "transpose_pad: C % 8");
  const int Mp = (M + 63) / 64 * 64;
  auto y = torch::empty({C, Mp}, x.options());
  launch_transpose_pad(x.data_ptr(), y.data_ptr(), M, C, Mp, cur_stream());
  return y;
}

// geometry shared by the padded-input 3x3 forward entry points
struct Conv3x3Geom {
  int Cin, Cout, Hp, Wp, Hout, Wout;
  long long M;
};

Conv3x3Geom conv3x3_geom(const torch::Tensor& xp, const torch::Tensor& w3,
                         int64_t stride, int64_t H, int64_t W) {
  check_padded(xp, H, W, "conv3x3");
  TORCH_CHECK(stride == 1 || stride == 2, "conv3x3: stride 1 or 2");
  Conv3x3Geom g;
  g.Cin = (int)xp.size(3);
  g.Cout = (int)w3.size(0);
  TORCH_CHECK(w3.size(1) == 9 * g.Cin && w3.is_contiguous(),
              "conv3x3: w3 shape");
  TORCH_CHECK(g.Cin % 64 == 0 && g.Cout % 64 == 0, "conv3x3: C % 64");
  g.Hp = (int)H + 2;
  g.Wp = (int)W + 2;
  g.Hout = out_extent(H, stride);
  g.Wout = out_extent(W, stride);
  g.M = (long long)xp.size(0) * g.Hout * g.Wout;
  return g;
}

// xp: zero-halo padded input [N, H+2, W+2, Cin] bf16; w3: [Cout, 9*Cin].
// Returns {y2d [M, Cout]} or, with_stats, {y2d, BN stats partials of the
// output [tiles_m, 2*Cout]}. Split-K shapes can't fold stats (sumsq is
// nonlinear over partial sums) — the second return is then an undefined
// tensor (Python None).
std::vector<torch::Tensor> conv3x3_fwd_impl(const torch::Tensor& xp,
                                            const torch::Tensor& w3,
                                            int64_t stride, int64_t H,
                                            int64_t W, bool with_stats) {
  const Conv3x3Geom g = conv3x3_geom(xp, w3, stride, H, W);
  const int M = (int)g.M;
  auto s = cur_stream();
  const int splitk = conv3x3_pick_splitk(M, g.Cout, g.Cin);
  torch::Tensor y, bpart;
  if (splitk > 1) {
    // CU-starved deep-K shape: fp32 split-K partials + cast
    // pooled pre-zeroed fold target; cast_bf16_zero returns it clean
    auto part =
        part_pool_get(M, g.Cout, xp.options().dtype(torch::kFloat32));
    launch_conv3x3(xp.data_ptr(), w3.data_ptr(), nullptr, M, g.Cout, g.Cin,
                   g.Hout * g.Wout, g.Wout, g.Hp, g.Wp, (int)stride,
                   part.data_ptr<float>(), splitk, nullptr, s);
    y = torch::empty({g.M, g.Cout}, xp.options());
    launch_cast_bf16_zero(part.data_ptr<float>(), y.data_ptr(),
                          g.M * g.Cout, s);
  } else {
    y = torch::empty({g.M, g.Cout}, xp.options());
    if (with_stats)
      bpart = stats_part_buf(conv3x3_tiles_m(M, g.Cout), 2 * g.Cout,
                             xp.options());
    launch_conv3x3(xp.data_ptr(), w3.data_ptr(), y.data_ptr(), M, g.Cout,
                   g.Cin, g.Hout * g.Wout, g.Wout, g.Hp, g.Wp, (int)stride,
                   nullptr, 1, with_stats ? bpart.data_ptr<float>() : nullptr,
                   s);
  }
  return {y, bpart};  // bpart undefined without stats
}

torch::Tensor conv3x3_fwd_padded(torch::Tensor xp, torch::Tensor w3,
                                 int64_t stride, int64_t H, int64_t W) {
  return conv3x3_fwd_impl(xp, w3, stride, H, W, false)[0];
}

std::vector<torch::Tensor> conv3x3_fwd_stats_padded(torch::Tensor xp,
                                                    torch::Tensor w3,
                                                    int64_t stride, int64_t H,
                                                    int64_t W) {
  return conv3x3_fwd_impl(xp, w3, stride, H, W, true);
}

// conv3x3_fwd_padded followed by bn_fwd_eval (no residual), bit for bit.
// Non-split shapes run the fused epilogue; split-K shapes run the split-K
// launch and the cast as above, then the BN apply kernel on the result, so
// the caller never has to know the pick.
torch::Tensor conv3x3_fwd_bn_padded(torch::Tensor xp, torch::Tensor w3,
                                    int64_t stride, int64_t H, int64_t W,
                                    torch::Tensor scale, torch::Tensor shift,
                                    bool relu) {
  const Conv3x3Geom g = conv3x3_geom(xp, w3, stride, H, W);
  check_bn_affine(scale, shift, g.Cout, xp, "conv3x3_bn");
  const int M = (int)g.M;
  auto s = cur_stream();
  if (conv3x3_pick_splitk(M, g.Cout, g.Cin) > 1) {
    auto y0 = conv3x3_fwd_impl(xp, w3, stride, H, W, false)[0];
    auto y = torch::empty_like(y0);
    launch_bn_apply(y0.data_ptr(), nullptr, y.data_ptr(), nullptr,
                    scale.data_ptr<float>(), shift.data_ptr<float>(), g.M,
                    g.Cout, relu, false, s);
    return y;
  }
  auto y = torch::empty({g.M, g.Cout}, xp.options());
  launch_conv3x3_bn(xp.data_ptr(), w3.data_ptr(), y.data_ptr(), M, g.Cout,
                    g.Cin, g.Hout * g.Wout, g.Wout, g.Hp, g.Wp, (int)stride,
                    scale.data_ptr<float>(), shift.data_ptr<float>(), relu, s);
  return y;
}

// the unpadded twins: x 4-D channels_last bf16 [N, C, H, W], padded here
torch::Tensor conv3x3_fwd(torch::Tensor x, torch::Tensor w3, int64_t stride) {
  check_nhwc_bf16(x, "conv3x3", 64);
  return conv3x3_fwd_padded(pad_nhwc(x), w3, stride, x.size(2), x.size(3));
}

std::vector<torch::Tensor> conv3x3_fwd_stats(torch::Tensor x, torch::Tensor w3,
                                             int64_t stride) {
  check_nhwc_bf16(x, "conv3x3", 64);
  return conv3x3_fwd_stats_padded(pad_nhwc(x), w3, stride, x.size(2),
                                  x.size(3));
}

torch::Tensor gemm_tn3x3_small(torch::Tensor dy2d, torch::Tensor x,
                               int64_t stride, int64_t splitk) {
  // Deep-stem conv wgrad, fully in-repo (closes VERDICT r1 #4's last
  // MIOpen rows): fp32 dW[64, N2v] = dY^T @ gather3x3(cpad(x)) via the
  // G3S small-Cin gather (gemm_tn.hip). dy2d: [M, 64] bf16 with the real
  // Cout columns first (caller zero-pads); x: 4-D channels_last bf16,
  // Cin <= 64. Returns [64, N2v]; caller slices [:Cout, :9*CinP] and
  // re-lays to [Cout, Cin, 3, 3].
  check_nhwc_bf16(x, "tn3x3s");
  TORCH_CHECK(stride == 1 || stride == 2, "tn3x3s: stride 1 or 2");
  const int Nimg = (int)x.size(0), Cin = (int)x.size(1);
  const int H = (int)x.size(2), W = (int)x.size(3);
  TORCH_CHECK(Cin >= 1 && Cin <= 64, "tn3x3s: Cin <= 64");
  const int Hout = out_extent(H, stride), Wout = out_extent(W, stride);
  const long long M = (long long)Nimg * Hout * Wout;
  TORCH_CHECK(dy2d.is_cuda() && dy2d.is_contiguous() && dy2d.dim() == 2 &&
                  dy2d.scalar_type() == torch::kBFloat16 &&
                  dy2d.size(0) == M && dy2d.size(1) == 64,
              "tn3x3s: dy2d [M, 64] bf16");
  int CinP = 8;
  while (CinP < Cin) CinP <<= 1;
  const int N2 = 9 * CinP;
  const int N2v = (N2 + 63) / 64 * 64;
  auto s = cur_stream();
  auto xp = pad_nhwc_flat(x, CinP, s);
  if (splitk <= 0) {
    const int nch = (int)((M + 63) / 64);
    splitk = auto_splitk(N2v / 64, std::max(1, nch));
  }
  auto c = torch::zeros({64, N2v}, x.options().dtype(torch::kFloat32));
  launch_gemm_tn3x3_small(dy2d.data_ptr(), xp.data_ptr(), c.data_ptr<float>(),
                          64, N2v, (int)M, Hout, Wout, H + 2, W + 2, CinP,
                          (int)stride, (int)splitk, s);
  return c;
}

// ---- image input stage (image_prep.hip) -----------------------------------

// packed: flat uint8 sources; table: int32 [B, kImagePrepFields] (layout in
// launchers.h) -> channels-last [B, 3, S, S] bf16 or fp32, into `out` when
// given. The table's CONTENT is checked on its host copy by the caller
// (ops/image_prep.py); the kernel clamps every index regardless.
torch::Tensor crop_resize_normalize(torch::Tensor packed, torch::Tensor table,
                                    int64_t out_size, std::vector<double> mean,
                                    std::vector<double> stdv, bool out_bf16,
                                    c10::optional<torch::Tensor> out) {
  const char* who = "crop_resize_normalize";
  TORCH_CHECK(packed.is_cuda() && table.is_cuda() &&
                  packed.device() == table.device(),
              who, ": packed and table must sit on one GPU");
  TORCH_CHECK(packed.scalar_type() == torch::kUInt8 && packed.dim() == 1 &&
                  packed.is_contiguous(),
              who, ": packed must be a flat contiguous uint8 tensor");
  TORCH_CHECK(packed.numel() >= 3 && packed.numel() < (1LL << 31), who,
              ": 3 <= packed.numel() < 2^31");
  TORCH_CHECK(table.scalar_type() == torch::kInt32 && table.dim() == 2 &&
                  table.size(1) == kImagePrepFields && table.is_contiguous() &&
                  reinterpret_cast<uintptr_t>(table.data_ptr()) % 16 == 0,
              who, ": table must be a contiguous, 16-byte aligned int32 [B, ",
              kImagePrepFields, "] tensor");
  const int64_t B = table.size(0), S = out_size;
  TORCH_CHECK(B >= 1, who, ": B >= 1");
  TORCH_CHECK(S >= 1 && S <= 16384, who, ": 1 <= out_size <= 16384");
  TORCH_CHECK(B * image_prep_blocks_per_image((int)S) < (1LL << 31), who,
              ": batch too large for one launch");
  TORCH_CHECK(mean.size() == 3 && stdv.size() == 3, who,
              ": mean and std have 3 entries");
  float k3[3], b3[3];
  for (int c = 0; c < 3; ++c) {
    TORCH_CHECK(stdv[c] > 0.0, who, ": std > 0");
    k3[c] = (float)(1.0 / (255.0 * stdv[c]));
    b3[c] = (float)(mean[c] / stdv[c]);
  }
  const auto dtype = out_bf16 ? torch::kBFloat16 : torch::kFloat32;
  torch::Tensor y;
  if (out.has_value()) {
    y = *out;
    TORCH_CHECK(y.is_cuda() && y.device() == packed.device() &&
                    y.scalar_type() == dtype && y.dim() == 4 &&
                    y.size(0) == B && y.size(1) == 3 && y.size(2) == S &&
                    y.size(3) == S && y.permute({0, 2, 3, 1}).is_contiguous(),
                who, ": out must be a channels-last [B, 3, S, S] tensor of "
                     "the output dtype on packed's device");
  } else {
    y = torch::empty({B, 3, S, S}, packed.options().dtype(dtype).memory_format(
                                       torch::MemoryFormat::ChannelsLast));
  }
  launch_image_prep(packed.data_ptr<uint8_t>(), (long long)packed.numel(),
                    table.data_ptr<int>(), y.data_ptr(), (int)B, (int)S,
                    out_bf16 ? 1 : 0, k3, b3, cur_stream());
  return y;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("crop_resize_normalize", &crop_resize_normalize,
        "crop + bilinear resize + mirror + mean/std normalize of packed uint8 "
        "RGB sources -> channels-last [B, 3, S, S] (table: int32 [B, 8] = "
        "{offset, H, W, flip, bits of x0, y0, cw, ch})",
        py::arg("packed"), py::arg("table"), py::arg("out_size"),
        py::arg("mean"), py::arg("std"), py::arg("out_bf16"),
        py::arg("out") = py::none());
  m.attr("IMAGE_PREP_FIELDS") = kImagePrepFields;
  m.def("fused_sgd", &fused_sgd,
        "fused flat momentum-SGD update (p,g,m flat fp32; folds grad_scale)",
        py::arg("p"), py::arg("g"), py::arg("m"), py::arg("lr"),
        py::arg("momentum"), py::arg("weight_decay"), py::arg("grad_scale"),
        py::arg("lr_dev") = py::none(), py::arg("clip_state") = py::none());
  m.def("grad_norm_rows", [](int64_t n) { return grad_norm_rows(n); },
        "partial rows grad_sumsq writes for a buffer of n elements",
        py::arg("n"));
  m.def("grad_sumsq", &grad_sumsq,
        "per-block double sums of squares of flat fp32 buffers into "
        "partial (every row written; 16 buffers per launch) -> rows_total",
        py::arg("buffers"), py::arg("partial"));
  m.def("grad_clip_finalize", &grad_clip_finalize,
        "partial rows -> state [coef, norm, skip, nskipped]: norm = "
        "grad_scale*sqrt(sum), coef = min(1, max_norm/(norm+1e-6))",
        py::arg("partial"), py::arg("rows_total"), py::arg("state"),
        py::arg("grad_scale"), py::arg("max_norm"),
        py::arg("skip_nonfinite") = false);
  m.attr("GRAD_NORM_MAX_SEGS") = kGradNormMaxSegs;
  m.attr("GRAD_NORM_ROW_CAP") = kGradNormRowCap;
  m.def("fused_adam", &fused_adam,
        "fused flat Adam/AdamW update (p,g,m,v flat fp32; step count and lr "
        "read from device scalars; optional per-segment decay table of at "
        "most 1024 segments); does not advance step_dev",
        py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"),
        py::arg("step_dev"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("weight_decay"),
        py::arg("grad_scale"), py::arg("decoupled"),
        py::arg("lr_dev") = py::none(), py::arg("seg_end") = py::none(),
        py::arg("seg_wd") = py::none(), py::arg("clip_state") = py::none());
  m.attr("ADAM_MAX_SEGMENTS") = kAdamMaxSegments;
  m.def("lars_sumsq", &lars_sumsq,
        "LARS: double sums of squares of p and g per row of the chunk table "
        "(int32 [nchunks, 4] = {bucket, start, len, 0}) into partial "
        "[2 * nchunks]; every pair written; 16 buckets per launch "
        "-> nchunks",
        py::arg("ps"), py::arg("gs"), py::arg("chunks"),
        py::arg("bucket_chunk_off"), py::arg("partial"));
  m.def("lars_trust", &lars_trust,
        "LARS: chunk partials -> trust[k] = coeff*pn/(gn + wd*pn + eps) per "
        "tensor (1.0 without chunks or with pn, gn or wd not > 0), "
        "gn = grad_scale * clip coef * sqrt(sum g^2)",
        py::arg("partial"), py::arg("nchunks"), py::arg("tensor_chunks"),
        py::arg("trust"), py::arg("lars_coeff"),
        py::arg("lars_weight_decay"), py::arg("epsilon"),
        py::arg("grad_scale"), py::arg("clip_state") = py::none());
  m.def("fused_lars", &fused_lars,
        "fused flat LARS momentum update (p,g,v flat fp32): v = mu*v + "
        "lr*trust[seg_tensor]*(scale*g + seg_wd*p); p -= v; at most 1024 "
        "segments; lr read from the device scalar when given",
        py::arg("p"), py::arg("g"), py::arg("v"), py::arg("lr"),
        py::arg("momentum"), py::arg("grad_scale"), py::arg("seg_end"),
        py::arg("seg_wd"), py::arg("seg_tensor"), py::arg("trust"),
        py::arg("lr_dev") = py::none(), py::arg("clip_state") = py::none());
  m.attr("LARS_CHUNK") = kLarsChunk;
  m.attr("LARS_MAX_BUFS") = kLarsMaxBufs;
  m.attr("LARS_TRUST_PRELOAD") = kLarsTrustPreload;
  m.def("dgc_workspace_words", &dgc_workspace_words,
        "int32 words of the (zero-initialised) DGC select workspace");
  m.def("dgc_accumulate", &dgc_accumulate,
        "DGC: u = mu*u + (g + wd*p); v += u; radix-select pass 0 histogram",
        py::arg("g"), py::arg("u"), py::arg("v"), py::arg("p"), py::arg("mu"),
        py::arg("wd"), py::arg("ws"), py::arg("hist_copies") = 4);
  m.def("dgc_hist", &dgc_hist, "DGC radix-select histogram pass 1 or 2",
        py::arg("v"), py::arg("ws"), py::arg("pass_"));
  m.def("dgc_pick", &dgc_pick, "DGC radix-select: fix one digit (pass 0..2)",
        py::arg("v"), py::arg("ws"), py::arg("pass_"), py::arg("k"));
  m.def("dgc_compact", &dgc_compact,
        "DGC: write the selected (idx, bits) into payload [2,k]; zero v, u",
        py::arg("v"), py::arg("u"), py::arg("payload"), py::arg("ws"));
  m.def("dgc_select", &dgc_select,
        "DGC: pick 0, (hist, pick) x 2 and compact, after dgc_accumulate",
        py::arg("v"), py::arg("u"), py::arg("payload"), py::arg("ws"));
  m.def("dgc_scatter_add", &dgc_scatter_add,
        "DGC decode: out[idx] += val for one rank's payload",
        py::arg("out"), py::arg("payload"));
  m.def("kd_ce_forward", &kd_ce_forward, "KD soft-label CE forward -> per-row loss");
  m.def("kd_ce_backward", &kd_ce_backward, "KD soft-label CE backward -> dlogits");
  m.def("softmax_ce_forward", &softmax_ce_forward,
        "hard-label CE (label smoothing, optional mixup) fwd -> "
        "(loss_row, lse, rank)",
        py::arg("s"), py::arg("labels"), py::arg("labels_b") = py::none(),
        py::arg("lam") = py::none(), py::arg("eps") = 0.0);
  m.def("softmax_ce_backward", &softmax_ce_backward,
        "hard-label CE bwd -> dlogits (gout is a device scalar)",
        py::arg("s"), py::arg("lse"), py::arg("labels"), py::arg("labels_b"),
        py::arg("lam"), py::arg("eps"), py::arg("gout"), py::arg("inv_B"));
  m.def("bn_fwd_train", &bn_fwd_train,
        "fused NHWC bf16 BN(+add)+ReLU train fwd -> (y, mean, invstd, mask)",
        py::arg("x"), py::arg("gamma"), py::arg("beta"), py::arg("rmean"),
        py::arg("rvar"), py::arg("momentum"), py::arg("eps"), py::arg("res"),
        py::arg("relu"), py::arg("pre_part") = py::none(),
        py::arg("pad_hw") = py::none());
  m.def("bn_fwd_eval", &bn_fwd_eval, "fused NHWC bf16 BN(+add)+ReLU eval fwd");
  m.def("bn_bwd", &bn_bwd,
        "fused BN(+add)+ReLU bwd -> (dx, dgamma, dbeta, dres?)",
        py::arg("dy"), py::arg("msk"), py::arg("x"), py::arg("mean"),
        py::arg("invstd"), py::arg("gamma"), py::arg("relu"), py::arg("add"),
        py::arg("training"), py::arg("dgamma_acc") = py::none(),
        py::arg("dbeta_acc") = py::none(), py::arg("pad_hw") = py::none());
  m.def("pad_nhwc", &pad_nhwc,
        "channels_last bf16 [N,C,H,W] -> zero-halo padded [N,H+2,W+2,C]");
  m.def("conv3x3_fwd_padded", &conv3x3_fwd_padded,
        "conv3x3_fwd on an already padded xp [N,H+2,W+2,Cin]", py::arg("xp"),
        py::arg("w3"), py::arg("stride"), py::arg("H"), py::arg("W"));
  m.def("conv3x3_fwd_stats_padded", &conv3x3_fwd_stats_padded,
        "conv3x3_fwd_stats on an already padded xp", py::arg("xp"),
        py::arg("w3"), py::arg("stride"), py::arg("H"), py::arg("W"));
  m.def("conv3x3s2_dgrad_padded", &conv3x3s2_dgrad_padded,
        "conv3x3s2_dgrad on an already padded dy [N,Ho+2,Wo+2,Cout]",
        py::arg("dyp"), py::arg("wcat"), py::arg("H"), py::arg("W"));
  m.def("gemm_tn3x3_splitk_padded", &gemm_tn3x3_splitk_padded,
        "gemm_tn3x3_splitk on padded xp; dy [M,Cout] or padded 4-D",
        py::arg("dy"), py::arg("xp"), py::arg("H"), py::arg("W"),
        py::arg("stride"), py::arg("splitk") = 0, py::arg("out") = py::none());
  m.def("conv3x3_wgrad_operand_padded", &conv3x3_wgrad_operand_padded,
        "conv3x3_wgrad_operand on an already padded xp", py::arg("xp"),
        py::arg("H"), py::arg("W"), py::arg("stride"));
  m.def("gemm_bt", &gemm_bt, "bf16 MFMA GEMM: C[M,N] = A[M,K] @ B[N,K]^T");
  m.def("conv3x3_fwd", &conv3x3_fwd,
        "implicit-GEMM 3x3 same-pad conv (stride 1/2) -> y2d [M, Cout]");
  m.def("conv3x3_fwd_stats", &conv3x3_fwd_stats,
        "conv3x3_fwd + BN stats partials -> (y2d, part-or-None)");
  m.def("gemm_bt_stats", &gemm_bt_stats,
        "gemm_bt + BN stats partials -> (C, part)");
  m.def("gemm_bt_add", &gemm_bt_add,
        "gemm_bt with a bf16 [M,N] addend: bf16(float(bf16(A@B^T)) + R)",
        py::arg("a"), py::arg("b"), py::arg("r"));
  m.def("gemm_bt_bn", &gemm_bt_bn, py::arg("a"), py::arg("b"),
        py::arg("scale"), py::arg("shift"), py::arg("relu"),
        py::arg("res") = py::none(),
        "gemm_bt + eval BN(+Add)+ReLU apply in one kernel, bit-equal to "
        "bn_fwd_eval(gemm_bt(a, b), scale, shift, res, relu)");
  m.def("conv3x3_fwd_bn_padded", &conv3x3_fwd_bn_padded,
        "conv3x3_fwd_padded + eval BN(+ReLU) apply: (xp, w3, stride, H, W, "
        "scale, shift, relu) -> y2d; fused epilogue on non-split shapes");
  m.def("conv3x3_grouped_fwd_bn", &conv3x3_grouped_fwd_bn,
        "conv3x3_grouped_fwd + eval BN(+ReLU) apply in the epilogue: (x, "
        "w3g, stride, scale, shift, relu) -> y2d");
  m.def("transpose_pad", &transpose_pad,
        "bf16 [M,C] -> [C, ceil64(M)] transpose with zero pad");
  m.def("gemm_bt_splitk", &gemm_bt_splitk,
        "split-K bt GEMM -> fp32 C (wgrad shapes)", py::arg("a"), py::arg("b"),
        py::arg("splitk") = 0);
  m.def("gemm_tn3x3_splitk", &gemm_tn3x3_splitk,
        "direct conv3x3 wgrad: fp32 dW3[Cout,9Cin] = dY^T @ gather3x3(pad(x))",
        py::arg("dy2d"), py::arg("x"), py::arg("stride"), py::arg("splitk") = 0,
        py::arg("out") = py::none());
  m.def("gemm_tn3x3_small", &gemm_tn3x3_small, py::arg("dy2d"),
        py::arg("x"), py::arg("stride"), py::arg("splitk") = 0,
        "stem wgrad: dY^T @ gather3x3(cpad(x)) -> fp32 [64, N2v] (G3S)");
  m.def("gemm_tn_splitk", &gemm_tn_splitk,
        "split-K TN GEMM: fp32 C[N1,N2] = A[K,N1]^T @ B[K,N2] (direct wgrad)",
        py::arg("a"), py::arg("b"), py::arg("splitk") = 0,
        py::arg("out") = py::none());
  m.def("conv3x3_wgrad_operand", &conv3x3_wgrad_operand,
        "padded shifted transpose of conv3x3 input -> [9*Cin, Mp]");
  m.def("avgpool2x2_fwd", &avgpool2x2_fwd, "2x2/s2 ceil avg pool (NHWC bf16)");
  m.def("conv3x3_grouped_fwd", &conv3x3_grouped_fwd,
        "grouped (16ch/group) 3x3 conv fwd -> y2d [M, Cout]");
  m.def("conv3x3s2_dgrad", &conv3x3s2_dgrad,
        "stride-2 3x3 same-pad dgrad (parity implicit GEMM) -> dx2d [N*H*W, Cin]");
  m.def("conv3x3_small_fwd", &conv3x3_small_fwd,
        "small-channel 3x3 conv (deep stem) -> y2d [M, cout_real]");
  m.def("conv3x3_small_fwd_stats", &conv3x3_small_fwd_stats,
        "stem conv + BN stats partials -> (y2d, part)");
  m.def("repack_dgrad_w3", &repack_dgrad_w3,
        "dgrad weight repack [Co,9Ci]->[Ci,9Co] (mode 0 rot / 1 s2 order)");
  m.def("maxpool3x3s2_fwd", &maxpool3x3s2_fwd,
        "3x3/s2/p1 max pool NHWC bf16 -> (y, tap idx)");
  m.def("maxpool3x3s2_bwd", &maxpool3x3s2_bwd,
        "3x3/s2/p1 max pool backward (bounded gather via tap idx)");
  m.def("avgpool2x2_bwd", &avgpool2x2_bwd, "2x2/s2 ceil avg pool backward");
  m.attr("_arch") = "gfx950";
}
