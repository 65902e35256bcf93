"""FusedLARS — layer-wise adaptive rate scaling over the reducer's flat
buckets (Paddle's lars_momentum op / DistributedStrategy.lars).

The engine rescales the learning rate linearly with the elastic world; LARS
is the large-batch remedy for what one global LR does to individual layers.
With s = grad_scale (times the clip coefficient when a clip state is given,
an fp32 product), for each parameter tensor k with decay wd_k
(lars_weight_decay, or 0 when the tensor is excluded):

    pn = sqrt(sum p^2)        gn = s * sqrt(sum g^2)
    trust = lars_coeff * pn / (gn + wd_k*pn + epsilon)  if wd_k, pn, gn > 0
          = 1                                           otherwise
    v = momentum*v + (lr*trust) * (s*g + wd_k*p)        p -= v

The velocity holds the learning rate, as in Paddle (and unlike
torch.optim.SGD's momentum_buffer: the state dict calls it `velocity` so
FusedSGD cannot load it by mistake). Excluded tensors (`exclude`: None |
predicate param -> bool | iterable of params) are plain momentum at lr with
no decay.

It cannot be bolted on from outside for the reasons ops/clip.py gives:
gradients are views into flat buckets, the 1/world average is folded into
the update, and a step replays as one hipGraph. So on a GPU a step is
edl_amd._C.lars_sumsq (per-tensor double sums of squares of p and g over a
device chunk table, one launch per 16 buckets), lars_trust (one launch)
and fused_lars (one launch per bucket), all on the current stream with
nothing on the host in between; lr is read from a device scalar. Buckets on
a GPU ALWAYS take the kernels (a missing extension raises); CPU buckets run
the same rule in torch with double sums per tensor.

The tables (chunks, per-tensor chunk ranges, per-bucket segments) are built
once per bucket layout and rebuilt after reducer.rebuild(). A non-excluded
tensor is always its own segment, adjacent excluded tensors coalesce; the
update kernel takes at most LARS_MAX_SEGMENTS (1024) segments per bucket."""
import torch

from . import ext
from ..train.bucketed_ddp import _view_like

LARS_MAX_SEGMENTS = 1024  # == _C.ADAM_MAX_SEGMENTS (csrc/launchers.h)


class FusedLARS:
    handles_grad_scale = True

    def __init__(self, params, lr, momentum=0.9, lars_coeff=0.001,
                 lars_weight_decay=0.0005, epsilon=0.0, exclude=None,
                 grad_scale=1.0, reducer=None):
        if min(lr, momentum, lars_coeff, lars_weight_decay, epsilon) < 0.0:
            raise ValueError("FusedLARS: lr, momentum, lars_coeff, "
                             "lars_weight_decay, epsilon must be >= 0")
        # state-dict and trust indices follow the order given
        self._all_params = list(params)
        self._index = {id(p): i for i, p in enumerate(self._all_params)}
        if exclude is None:
            ex = []
        elif callable(exclude):
            ex = [i for i, p in enumerate(self._all_params) if exclude(p)]
        else:
            ids = {id(p) for p in exclude}
            ex = [i for i, p in enumerate(self._all_params) if id(p) in ids]
        self._exclude = set(ex)
        self.defaults = dict(lr=float(lr), momentum=float(momentum),
                             lars_coeff=float(lars_coeff),
                             lars_weight_decay=float(lars_weight_decay),
                             epsilon=float(epsilon), exclude=sorted(ex))
        self.param_groups = [dict(
            self.defaults,
            params=[p for p in self._all_params if p.requires_grad])]
        self.grad_scale = grad_scale
        self._reducer = reducer
        self._buckets = None
        self._lr_dev = None  # LR device scalar on GPU (see FusedSGD)
        self._trust = None   # fp32 [len(params)], survives a rebuild
        self._tables = None  # GPU: chunks, tensor_chunks, partial, ...
        if reducer is not None:
            self.attach(reducer)

    def attach(self, reducer):
        self._reducer = reducer
        self._buckets = None
        reducer._attached_opt = self  # rebuild() snapshots/restores v
        return self

    def set_lr(self, lr):
        """Set the learning rate (updates the device scalar when present)."""
        for g in self.param_groups:
            g["lr"] = float(lr)
        if self._lr_dev is not None:
            self._lr_dev.fill_(float(lr))

    def _param_wd(self, p):
        wd = self.param_groups[0]["lars_weight_decay"]
        return 0.0 if self._index.get(id(p)) in self._exclude else wd

    def _build_tables(self):
        """Per bucket the segment lists [end, wd, param index]; on a GPU
        also the device tables of the three kernels."""
        on_gpu = bool(self._buckets) and self._buckets[0]["p"].is_cuda
        chunk = int(ext().LARS_CHUNK) if on_gpu else 0
        chunks = []        # [bucket, start, len, 0], sorted by bucket
        bucket_off = [0]   # first chunk of each bucket, then the end
        tensor_chunks = [[0, 0] for _ in self._all_params]
        for bi, bk in enumerate(self._buckets):
            segs = []
            for (off, n), p in zip(bk["offsets"], bk["params"]):
                wd, idx = self._param_wd(p), self._index[id(p)]
                if wd == 0.0 and segs and segs[-1][1] == 0.0:
                    segs[-1][0] = off + n  # adjacent excluded: one segment
                else:
                    segs.append([off + n, wd, idx])
                if on_gpu and wd != 0.0:  # excluded tensors get no chunks
                    tensor_chunks[idx][0] = len(chunks)
                    for s in range(off, off + n, chunk):
                        chunks.append([bi, s, min(chunk, off + n - s), 0])
                    tensor_chunks[idx][1] = len(chunks) - tensor_chunks[idx][0]
            bucket_off.append(len(chunks))
            bk["segs"] = segs
            if not on_gpu:
                continue
            # checked HERE, on the host lists: the bindings can only check a
            # device table with a D2H sync, which they cannot afford under
            # graph capture
            if len(segs) > LARS_MAX_SEGMENTS:
                raise RuntimeError(
                    "FusedLARS: a bucket needs %d segments; the kernel's "
                    "table holds %d per bucket (use a smaller bucket cap)"
                    % (len(segs), LARS_MAX_SEGMENTS))
            ends = [s[0] for s in segs]
            if (ends != sorted(ends) or ends[-1] != bk["p"].numel()
                    or bk["p"].numel() >= 2 ** 31):
                raise RuntimeError("FusedLARS: malformed segment table")
            dev = bk["p"].device
            bk["seg_end"] = torch.tensor(ends, dtype=torch.int32, device=dev)
            bk["seg_wd"] = torch.tensor([s[1] for s in segs],
                                        dtype=torch.float32, device=dev)
            bk["seg_tensor"] = torch.tensor([s[2] for s in segs],
                                            dtype=torch.int32, device=dev)
        self._tables = None
        if on_gpu:
            dev = self._buckets[0]["p"].device
            self._tables = {
                "chunks": torch.tensor(chunks, dtype=torch.int32,
                                       device=dev).view(-1, 4),
                "bucket_off": bucket_off,
                "tensor_chunks": torch.tensor(tensor_chunks, dtype=torch.int32,
                                              device=dev).view(-1, 2),
                # every live slot is written on every launch: no fill
                "partial": torch.empty(max(2 * len(chunks), 2),
                                       dtype=torch.float64, device=dev),
                "ps": [bk["p"] for bk in self._buckets],
                "gs": [bk["g"] for bk in self._buckets],
            }

    def _materialize(self):
        if self._buckets is not None:
            return self._buckets
        r = self._reducer
        if r is None:
            raise RuntimeError("FusedLARS needs a BucketedAllReducer (call attach())")
        out = []
        for b in r._buckets:
            if b.param_flat is None:
                raise RuntimeError("FusedLARS requires flatten_params=True buckets")
            if b.param_flat.is_cuda and b.param_flat.dtype != torch.float32:
                raise RuntimeError("FusedLARS needs fp32 buckets on a GPU")
            offsets = []
            off = 0
            for p in b.params:
                offsets.append((off, p.numel()))
                off += p.numel()
            out.append({"p": b.param_flat, "g": b.buffer,
                        "v": torch.zeros_like(b.param_flat),
                        "params": b.params, "offsets": offsets})
        self._buckets = out
        self._build_tables()
        if out:
            dev = out[0]["p"].device
            if self._trust is None or self._trust.device != dev:
                self._trust = torch.ones(max(len(self._all_params), 1),
                                         dtype=torch.float32, device=dev)
            if dev.type == "cuda" and self._lr_dev is None:
                self._lr_dev = torch.full(
                    (1,), self.param_groups[0]["lr"], dtype=torch.float32,
                    device=dev)
        return out

    @torch.no_grad()
    def step(self, clip_state=None):
        """clip_state: the [coef, norm, skip, nskipped] tensor of
        ops/clip.py GradClipper.run() — the gradient scale is multiplied
        by coef (in the gradient norm too); skip != 0 leaves p and v
        untouched."""
        from .conv import bump_weight_epoch

        bump_weight_epoch()  # invalidate per-step weight-derived caches
        buckets = self._materialize()
        if not buckets:
            return
        g0 = self.param_groups[0]
        lr, mu = g0["lr"], g0["momentum"]
        coeff, wd, eps = g0["lars_coeff"], g0["lars_weight_decay"], g0["epsilon"]
        if buckets[0]["p"].is_cuda:
            C = ext()  # a missing kernel is an error
            t = self._tables
            nchunks = C.lars_sumsq(t["ps"], t["gs"], t["chunks"],
                                   t["bucket_off"], t["partial"])
            C.lars_trust(t["partial"], nchunks, t["tensor_chunks"],
                         self._trust, coeff, wd, eps, self.grad_scale,
                         clip_state)
            for bk in buckets:
                C.fused_lars(bk["p"], bk["g"], bk["v"], lr, mu,
                             self.grad_scale, bk["seg_end"], bk["seg_wd"],
                             bk["seg_tensor"], self._trust, self._lr_dev,
                             clip_state)
            return
        # CPU (tests / gloo): the same rule in torch, double sums per tensor
        s = torch.tensor(self.grad_scale, dtype=torch.float32)
        if clip_state is not None:
            if bool(clip_state[2] != 0):
                return  # skipped step: p, v untouched
            s = s * clip_state[0]  # fp32 product, as the kernel forms it
        lr32 = torch.tensor(lr, dtype=torch.float32)
        for bk in buckets:
            for (off, n), p in zip(bk["offsets"], bk["params"]):
                pv, gv, vv = (bk[k][off:off + n] for k in "pgv")
                pwd = self._param_wd(p)
                trust = torch.ones((), dtype=torch.float32)
                if pwd > 0.0:
                    pn = pv.double().pow(2).sum().sqrt()
                    gn = s.double() * gv.double().pow(2).sum().sqrt()
                    if bool(pn > 0) and bool(gn > 0):
                        trust = (coeff * pn / (gn + pwd * pn + eps)).float()
                self._trust[self._index[id(p)]] = trust
                d = gv * s.to(gv.dtype)
                if pwd != 0.0:
                    d = d.add(pv, alpha=pwd)
                vv.mul_(mu).add_(d * (lr32 * trust).to(d.dtype))
                pv.sub_(vv)

    def zero_grad(self, set_to_none=False):
        if self._reducer is not None:
            self._reducer.zero_grad()

    def state_buffers(self):
        """Every tensor that must agree across ranks: the velocities (the
        engine broadcasts them from rank 0)."""
        return [bk["v"] for bk in self._materialize()]

    def trust_ratios(self):
        """The trust ratios of the last step: fp32 device tensor, one entry
        per param in the order given (1.0 for excluded ones), overwritten
        by every step; no host sync."""
        self._materialize()
        return self._trust[:len(self._all_params)]

    # ---- state dict: per-param `velocity`, indexed in the order given ----
    def state_dict(self):
        state = {}
        for bk in self._materialize():
            for (off, n), p in zip(bk["offsets"], bk["params"]):
                state[self._index[id(p)]] = {
                    "velocity": _view_like(bk["v"][off:off + n], p).clone()}
        state = {k: state[k] for k in sorted(state)}
        groups = [{k: v for k, v in self.param_groups[0].items() if k != "params"}]
        groups[0]["exclude"] = sorted(self._exclude)
        groups[0]["params"] = list(range(len(self._all_params)))
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        """The velocities, lr, momentum, lars_coeff, lars_weight_decay and
        epsilon are taken from `sd`. The excluded set is this optimizer's
        construction-time choice: a state dict that records another one is
        refused with a ValueError before anything is loaded."""
        src = sd["param_groups"][0] if sd.get("param_groups") else {}
        if "exclude" in src and sorted(src["exclude"]) != sorted(self._exclude):
            raise ValueError(
                "FusedLARS: state dict excludes params %s from LARS, this "
                "optimizer %s" % (sorted(src["exclude"]), sorted(self._exclude)))
        state = sd.get("state", {})
        for bk in self._materialize():
            for (off, n), p in zip(bk["offsets"], bk["params"]):
                idx = self._index[id(p)]
                ent = state.get(idx, state.get(str(idx)))
                if ent and ent.get("velocity") is not None:
                    _view_like(bk["v"][off:off + n], p).copy_(
                        ent["velocity"].to(bk["v"].device))
        g0 = self.param_groups[0]
        changed = False
        for k in ("lr", "momentum", "lars_coeff", "lars_weight_decay", "epsilon"):
            if k in src:
                changed |= k == "lars_weight_decay" and float(src[k]) != g0[k]
                g0[k] = float(src[k])
        if self._lr_dev is not None:
            self._lr_dev.fill_(g0["lr"])
        if changed:
            self._build_tables()  # seg_wd holds the decay
