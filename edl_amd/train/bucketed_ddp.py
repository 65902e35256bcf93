"""Gradient-bucketed data parallelism over RCCL/xGMI — our own DDP.

Replaces Paddle Fleet's fuse_all_reduce_ops + sync NCCL all-reduce
(reference train_with_fleet.py:371, train_pretrain.sh:17
FLAGS_sync_nccl_allreduce=1) with an MI355X-first design:

  * parameter gradients ARE views into flat per-dtype bucket buffers
    (no flatten/unflatten copies at all — the "fusion kernel" is free);
  * buckets fill in reverse parameter order (backward order), and each
    bucket's all-reduce is issued asynchronously the moment its last
    gradient lands (post-accumulate-grad hooks), overlapping communication
    with the rest of backward;
  * bucket size is tunable per topology: on one node each GPU has 7 xGMI
    p2p links (~153 GB/s each); ring all-reduce is per-link bound, so RCCL
    splits traffic over many channels — buckets must be large enough to
    keep all channels busy but small enough to start overlapping early.
    Default 25 MiB; re-tuned on every elastic resize via rebuild()
    (BASELINE north star: "re-bucketing gradients for 7 xGMI links per GPU
    on every membership change").

Gradient averaging (the 1/world factor) is NOT applied here; the fused
SGD kernel folds it into its update (grad_scale), saving one pass over
all gradients per step.
"""
import os

import torch
import torch.distributed as dist


def _view_like(flat_slice, p):
    """View a flat bucket slice with the param's LOGICAL shape.

    Plain params: a contiguous view. Params flagged `_edl_phys_shape` /
    `_edl_phys_perm` (the engine marks conv3x3 weights channels-last:
    phys [Cout, 3, 3, Cin], perm (0, 3, 1, 2)) get the physical layout
    in the bucket and a permuted logical view — the per-step s-major w3
    repack then becomes a zero-cost reshape of the bf16 mirror, and the
    3x3 wgrad's s-major epilogue writes the grad bucket COALESCED
    (round-1's measured-negative stride-9 scatter disappears)."""
    phys = getattr(p, "_edl_phys_shape", None)
    if phys is None:
        return flat_slice.view_as(p)
    return flat_slice.view(*phys).permute(*p._edl_phys_perm)


class _Bucket:
    __slots__ = ("params", "buffer", "ready", "work", "grads", "param_flat")

    def __init__(self, params, buffer, grads, param_flat=None):
        self.params = params
        self.buffer = buffer
        self.grads = grads  # per-param views into buffer
        self.param_flat = param_flat  # flat param data (flatten_params=True)
        self.ready = 0
        self.work = None


class BucketedAllReducer:
    def __init__(self, params, bucket_cap_mb=25, process_group=None, async_reduce=True,
                 flatten_params=True):
        """flatten_params=True additionally re-homes each parameter's DATA
        into a flat per-bucket buffer matching the gradient layout — the
        fused SGD then updates one contiguous array per bucket (one kernel)
        instead of one launch per parameter tensor."""
        self._pg = process_group
        self._async = async_reduce and dist.is_initialized() and dist.get_world_size() > 1
        self._enabled = dist.is_initialized() and dist.get_world_size() > 1
        self._flatten_params = flatten_params
        params = [p for p in params if p.requires_grad]
        self._params = params
        self._hooks = []
        self._buckets = []
        self._param_bucket = {}
        self._build(params, bucket_cap_mb)
        self._mark_direct_grads()
        if self._enabled:
            for p in params:
                h = p.register_post_accumulate_grad_hook(self._on_grad)
                self._hooks.append(h)

    # ---- construction ----
    def _build(self, params, cap_mb):
        cap = int(cap_mb * 1024 * 1024)
        groups = []  # list of (dtype, [params])
        cur, cur_bytes, cur_dtype = [], 0, None
        # reverse order: grads become ready roughly back-to-front
        for p in reversed(params):
            nbytes = p.numel() * p.element_size()
            if cur and (p.dtype != cur_dtype or cur_bytes + nbytes > cap):
                groups.append((cur_dtype, cur))
                cur, cur_bytes = [], 0
            cur.append(p)
            cur_bytes += nbytes
            cur_dtype = p.dtype
        if cur:
            groups.append((cur_dtype, cur))

        for dtype, ps in groups:
            total = sum(p.numel() for p in ps)
            buf = torch.zeros(total, dtype=dtype, device=ps[0].device)
            pflat = None
            if self._flatten_params:
                pflat = torch.empty(total, dtype=dtype, device=ps[0].device)
            grads = []
            off = 0
            for p in ps:
                g = _view_like(buf[off:off + p.numel()], p)
                p.grad = g
                grads.append(g)
                if pflat is not None:
                    with torch.no_grad():
                        pv = _view_like(pflat[off:off + p.numel()], p)
                        pv.copy_(p.data)
                        p.data = pv
                off += p.numel()
            b = _Bucket(ps, buf, grads, pflat)
            self._buckets.append(b)
            for p in ps:
                self._param_bucket[id(p)] = b

    def rebuild(self, bucket_cap_mb):
        """Re-bucket (e.g. after an elastic resize changed the optimal
        chunk size). Gradients are re-viewed into fresh buffers. The state
        of an attached flat-bucket optimizer (FusedSGD, FusedAdam,
        FusedLARS) is snapshotted per-param through its state dict and
        restored into the new bucket layout, and on_rebuild callbacks (e.g. the
        engine's bf16-mirror rebuild) fire afterwards — without this the
        optimizer would keep updating the DEAD flat buffers and training
        would silently stop progressing."""
        opt = getattr(self, "_attached_opt", None)
        opt_sd = opt.state_dict() if opt is not None else None
        for h in self._hooks:
            h.remove()
        self._hooks = []
        self._buckets = []
        self._param_bucket = {}
        self._build(self._params, bucket_cap_mb)
        self._mark_direct_grads()
        if self._enabled:
            for p in self._params:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._on_grad))
        if opt is not None:
            opt.drop_buckets()  # re-materialize against the new flats
            if opt_sd is not None:
                opt.load_state_dict(opt_sd)
        for cb in getattr(self, "_on_rebuild", ()):
            cb()

    def register_rebuild_callback(self, cb):
        if not hasattr(self, "_on_rebuild"):
            self._on_rebuild = []
        self._on_rebuild.append(cb)

    def _mark_direct_grads(self):
        """World 1 (no collectives, no readiness hooks needed): flag every
        param so the custom HIP backward ops accumulate straight into the
        bucket-view .grad and return None — this removes one
        AccumulateGrad add kernel per parameter per step (~150 small
        launches / ~0.7 ms on ResNet50_vd) plus the fresh zeros the wgrad
        kernels otherwise allocate. At world > 1 the flag stays off: the
        overlap machinery needs the post-accumulate hooks to fire."""
        direct = (not self._enabled
                  and os.environ.get("EDL_DIRECT_GRAD", "1") != "0")
        for p in self._params:
            p._edl_direct_grad = direct

    # ---- per-step protocol ----
    def zero_grad(self):
        for b in self._buckets:
            b.buffer.zero_()
            b.ready = 0
            b.work = None

    def _on_grad(self, p):
        b = self._param_bucket[id(p)]
        b.ready += 1
        if b.ready == len(b.params):
            if self._async:
                b.work = dist.all_reduce(b.buffer, group=self._pg, async_op=True)

    def finalize(self):
        """Wait for (or issue) all bucket reductions. Call after backward,
        before the optimizer step."""
        if not self._enabled:
            return
        for b in self._buckets:
            if b.work is not None:
                b.work.wait()
            else:
                # sync mode, or a bucket whose params saw no gradient this
                # step (its buffer is zeros — still must participate)
                dist.all_reduce(b.buffer, group=self._pg)
            b.work = None
            b.ready = 0

    # ---- utilities ----
    @property
    def grad_scale(self):
        """Factor the optimizer must multiply grads by (the DP average)."""
        return 1.0 / dist.get_world_size() if self._enabled else 1.0

    def bucket_sizes_mb(self):
        return [b.buffer.numel() * b.buffer.element_size() / 2**20 for b in self._buckets]

    def broadcast_params(self, src=0):
        """Initial parameter sync (reference: fleet broadcast of epoch-0
        params, SURVEY.md §2.4 collective table)."""
        if not self._enabled:
            return
        with torch.no_grad():
            for b in self._buckets:
                if b.param_flat is not None:
                    dist.broadcast(b.param_flat, src=src, group=self._pg)
                else:
                    for p in b.params:
                        dist.broadcast(p.data, src=src, group=self._pg)
