"""DGC — deep gradient compression (optional sparse all-reduce path).

Parity: the reference exposes Paddle's DGCMomentumOptimizer
(train_with_fleet.py:98,106-111: rampup_begin_step, momentum correction)
as an optional strategy. This is the standard DGC scheme (Lin et al.,
public algorithm) on our bucket layout:

  * per bucket, keep local ERROR FEEDBACK: residual += grad
  * pick the top-k% of |residual|; zero them out of the residual
  * exchange (indices, values) with all_gather; every rank scatter-adds
    all ranks' sparse contributions into the bucket buffer (÷ world)
  * before rampup_begin_step, fall back to dense all-reduce

Enabled via DistributedStrategy(use_dgc=True) -> TrainerEngine(dgc=...) or
directly: reducer = BucketedAllReducer(..., async_reduce=False);
dgc = DGCCompressor(reducer, ...); dgc.step() replaces reducer.finalize().
"""
import torch
import torch.distributed as dist


class DGCCompressor:
    def __init__(self, reducer, compress_ratio=0.01, rampup_begin_step=0,
                 process_group=None):
        self._reducer = reducer
        self.compress_ratio = compress_ratio
        self.rampup_begin_step = rampup_begin_step
        self._pg = process_group
        self._step = 0
        self._residuals = [torch.zeros_like(b.buffer)
                           for b in reducer._buckets]
        # DGC exchanges instead of the reducer's own async all-reduce
        reducer._async = False

    @property
    def enabled(self):
        return dist.is_initialized() and dist.get_world_size() > 1

    @torch.no_grad()
    def step(self):
        """Call instead of reducer.finalize() after backward."""
        self._step += 1
        if not self.enabled:
            return
        if self._step <= self.rampup_begin_step:
            self._reducer.finalize()
            return
        world = dist.get_world_size()
        for b, res in zip(self._reducer._buckets, self._residuals):
            res.add_(b.buffer)  # error feedback accumulates the raw grad
            n = res.numel()
            k = max(1, int(n * self.compress_ratio))
            _, idx = torch.topk(res.abs(), k, sorted=False)
            vals = res[idx].clone()
            res[idx] = 0  # transmitted mass leaves the residual

            # exchange sparse (idx, vals) with all ranks
            idx_list = [torch.empty_like(idx) for _ in range(world)]
            val_list = [torch.empty_like(vals) for _ in range(world)]
            dist.all_gather(idx_list, idx, group=self._pg)
            dist.all_gather(val_list, vals, group=self._pg)

            b.buffer.zero_()
            for i, v in zip(idx_list, val_list):
                b.buffer.scatter_add_(0, i, v)
            # NOTE: the reducer's grad_scale (1/world) is applied by the
            # optimizer, matching the dense path's averaging.


class DGCMomentum:
    """DGC with momentum correction, momentum factor masking and a
    sparsity warm-up (Lin et al., "Deep Gradient Compression"; the
    algorithm behind Paddle's DGCMomentumOptimizer that the reference's
    `--use_dgc` selects). DGCCompressor above accumulates the RAW
    gradient and lets the optimizer's global momentum multiply each late,
    large sparse update; here momentum is applied locally, before
    compression.

    `s` = the 1-based global step (the engine passes global_step + 1, so
    a resumed run lands in the right phase). Per bucket, on every rank:

      s <= rampup_begin_step   dense phase: reducer.finalize() and the
                               normal optimizer step with its own momentum
      s >  rampup_begin_step   with g the local bucket gradient, p the
                               bucket's flat params:
          u = mu*u + (g + wd*p)          momentum correction
          v = v + u
          i = min(len(sparsity)-1,
                  (s - rampup_begin_step - 1) * len(sparsity) // rampup_step)
          k = max(1, int(n * (1 - sparsity[i])))
          payload = top-k of |v| (rule: ops/dgc.py) as (index, v[index])
          v[sel] = 0; u[sel] = 0         the second is the momentum masking
          all-gather the payloads: ONE collective per bucket on a packed
          int32 [2, k] buffer, no counts, nothing read back on the host
          bucket.buffer = sum of the payloads, added in rank order 0..W-1
          (bit-identical on every rank at any world size)
      then plain SGD on that sum: the optimizer steps with
      opt_overrides() = momentum 0, weight decay 0 (both already live in
      u); grad_scale (1/world) stays as it is.

    u and v are fp32, bucket-sized, rank-local, and start at ZERO on the
    first DGC step, as Paddle's do: the dense phase's momentum is lost
    once, at the switch. They are NOT checkpointed (matching the
    reference), so they restart at zero after a stop-resume. On
    reducer.rebuild() they follow their parameters into the new bucket
    layout.

    At world 1 the same steps run without the collective. The reducer's
    asynchronous all-reduce is switched off (the buckets must hold LOCAL
    gradients when step() runs), in the dense phase too.

    Not built: Paddle's local_grad_clip_norm; Paddle's 16384-element
    dense exemption (our unit is the bucket and every bucket is
    compressed); hipGraph capture of multi-rank steps (k and the phase
    are host-side schedule state, so the engine does not capture a step
    that runs this class). An fp16 loss scaler is refused by the engine:
    a changing loss scale corrupts the accumulated v.
    """

    def __init__(self, reducer, optimizer, momentum, weight_decay,
                 rampup_begin_step=0, rampup_step=1, sparsity=(0.999,),
                 process_group=None):
        sparsity = tuple(float(x) for x in sparsity)
        if not sparsity or any(not 0.0 <= x < 1.0 for x in sparsity):
            raise ValueError("dgc: sparsity entries must lie in [0, 1)")
        if rampup_step < 1 or rampup_begin_step < 0:
            raise ValueError("dgc: rampup_step >= 1, rampup_begin_step >= 0")
        self._reducer = reducer
        self._opt = optimizer
        self.momentum = float(momentum)
        self.weight_decay = float(weight_decay)
        self.rampup_begin_step = int(rampup_begin_step)
        self.rampup_step = int(rampup_step)
        self.sparsity = sparsity
        self._pg = process_group
        self._step = 0
        self.compressed = False  # did the last step() run the DGC phase?
        self._state = None  # per bucket: {"u", "v", "params", "offsets"}
        reducer._async = False
        reducer.register_rebuild_callback(self._on_rebuild)

    # ---- schedule ----
    def in_dgc_phase(self, s):
        return s > self.rampup_begin_step

    def sparsity_index(self, s):
        m = len(self.sparsity)
        return min(m - 1, (s - self.rampup_begin_step - 1) * m
                   // self.rampup_step)

    def k_for(self, n, s):
        return max(1, int(n * (1 - self.sparsity[self.sparsity_index(s)])))

    def opt_overrides(self):
        """Keyword overrides for FusedSGD.step() after the last step()."""
        if self.compressed:
            return {"momentum": 0.0, "weight_decay": 0.0}
        return {}

    # ---- state ----
    @staticmethod
    def _layout(bucket):
        offsets, off = [], 0
        for p in bucket.params:
            offsets.append((off, p.numel()))
            off += p.numel()
        return offsets

    def _materialize(self):
        if self._state is None:
            self._state = []
            for b in self._reducer._buckets:
                if b.buffer.dtype != torch.float32:
                    raise RuntimeError("dgc: fp32 gradient buckets required")
                if b.param_flat is None and self.weight_decay != 0.0:
                    raise RuntimeError(
                        "dgc: weight decay needs flatten_params=True buckets")
                self._state.append({
                    "u": torch.zeros_like(b.buffer),
                    "v": torch.zeros_like(b.buffer),
                    "params": list(b.params), "offsets": self._layout(b)})
        return self._state

    def _on_rebuild(self):
        """The reducer re-bucketed: carry each parameter's slice of u, v
        from the old flats (which this object owns) into the new layout."""
        old = self._state
        if old is None:
            return
        where = {}
        for st in old:
            for p, (off, n) in zip(st["params"], st["offsets"]):
                where[id(p)] = (st, off, n)
        self._state = None
        for st in self._materialize():
            for p, (off, n) in zip(st["params"], st["offsets"]):
                src = where.get(id(p))
                if src is None:
                    continue
                ost, ooff, _ = src
                st["u"][off:off + n].copy_(ost["u"][ooff:ooff + n])
                st["v"][off:off + n].copy_(ost["v"][ooff:ooff + n])

    # ---- the step ----
    @torch.no_grad()
    def step(self, global_step=None):
        """Call instead of reducer.finalize() after backward.
        -> True when the DGC phase ran (step the optimizer with
        opt_overrides())."""
        from ..ops.dgc import dgc_compress, dgc_decode

        self._step = self._step + 1 if global_step is None else int(global_step)
        s = self._step
        if not self.in_dgc_phase(s):
            self._reducer.finalize()
            self.compressed = False
            return False
        multi = dist.is_initialized() and dist.get_world_size(self._pg) > 1
        world = dist.get_world_size(self._pg) if multi else 1
        for b, st in zip(self._reducer._buckets, self._materialize()):
            n = b.buffer.numel()
            k = self.k_for(n, s)
            p = b.param_flat if self.weight_decay != 0.0 else None
            if not multi:
                payload = dgc_compress(b.buffer, st["u"], st["v"], p,
                                       self.momentum, self.weight_decay, k)
                dgc_decode(b.buffer, [payload])
                continue
            packed = torch.empty(world, 2, k, dtype=torch.int32,
                                 device=b.buffer.device)
            mine = dgc_compress(b.buffer, st["u"], st["v"], p, self.momentum,
                                self.weight_decay, k)
            slots = list(packed.unbind(0))
            dist.all_gather(slots, mine, group=self._pg)
            dgc_decode(b.buffer, slots)
            b.work = None
            b.ready = 0
        self.compressed = True
        return True
