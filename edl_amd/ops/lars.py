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
nothing on the host in between; lr is read from a device scalar. CPU
buckets run the same rule in torch with double sums per tensor.

The tables (chunks, per-tensor chunk ranges, per-bucket segments) are built
once per bucket layout and rebuilt after reducer.rebuild(). A non-excluded
tensor is always its own segment, adjacent excluded tensors coalesce; the
update kernel takes at most MAX_SEGMENTS (1024) segments per bucket."""
import torch

from . import ext
from .flat_optimizer import MAX_SEGMENTS, FlatBucketOptimizer

LARS_MAX_SEGMENTS = MAX_SEGMENTS


class FusedLARS(FlatBucketOptimizer):
    _name = "FusedLARS"
    _state_names = ("v",)
    _state_keys = {"velocity": "v"}
    _hyper_keys = ("lr", "momentum", "lars_coeff", "lars_weight_decay",
                   "epsilon")
    _decay_key = "lars_weight_decay"
    _select_key = "exclude"

    def __init__(self, params, lr, momentum=0.9, lars_coeff=0.001,
                 lars_weight_decay=0.0005, epsilon=0.0, exclude=None,
                 grad_scale=1.0, reducer=None):
        if min(lr, momentum, lars_coeff, lars_weight_decay, epsilon) < 0.0:
            raise ValueError("FusedLARS: lr, momentum, lars_coeff, "
                             "lars_weight_decay, epsilon must be >= 0")
        self._trust = None   # fp32 [len(params)], survives a rebuild
        self._tables = None  # GPU: chunks, tensor_chunks, partial, ...
        super().__init__(
            params,
            dict(lr=float(lr), momentum=float(momentum),
                 lars_coeff=float(lars_coeff),
                 lars_weight_decay=float(lars_weight_decay),
                 epsilon=float(epsilon)),
            select=exclude, grad_scale=grad_scale, reducer=reducer)

    def _build_tables(self):
        """Per bucket the segment lists [end, wd, param index]; on a GPU
        also the device tables of the three kernels."""
        on_gpu = bool(self._buckets) and self._buckets[0]["p"].is_cuda
        chunk = int(ext().LARS_CHUNK) if on_gpu else 0
        chunks = []        # [bucket, start, len, 0], sorted by bucket
        bucket_off = [0]   # first chunk of each bucket, then the end
        tensor_chunks = [[0, 0] for _ in self._all_params]
        for bi, bk in enumerate(self._buckets):
            # a non-excluded tensor is its own segment, adjacent excluded
            # ones coalesce
            self._build_segments(
                bk, merge=lambda prev, wd: prev == 0.0 and wd == 0.0,
                always_table=True, with_tensor=True)
            for (off, n), p in zip(bk["offsets"], bk["params"]):
                if on_gpu and self._param_wd(p) != 0.0:
                    # excluded tensors get no chunks
                    idx = self._index[id(p)]
                    tensor_chunks[idx][0] = len(chunks)
                    for s in range(off, off + n, chunk):
                        chunks.append([bi, s, min(chunk, off + n - s), 0])
                    tensor_chunks[idx][1] = len(chunks) - tensor_chunks[idx][0]
            bucket_off.append(len(chunks))
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

    def _on_materialize(self, buckets):
        for bk in buckets:
            if bk["p"].is_cuda and bk["p"].dtype != torch.float32:
                raise RuntimeError("FusedLARS needs fp32 buckets on a GPU")
        self._build_tables()
        if buckets:
            dev = buckets[0]["p"].device
            if self._trust is None or self._trust.device != dev:
                self._trust = torch.ones(max(len(self._all_params), 1),
                                         dtype=torch.float32, device=dev)

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
        s = self._cpu_scale(clip_state)
        if s is None:
            return  # skipped step: p, v untouched
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

    def trust_ratios(self):
        """The trust ratios of the last step: fp32 device tensor, one entry
        per param in the order given (1.0 for excluded ones), overwritten
        by every step; no host sync."""
        self._materialize()
        return self._trust[:len(self._all_params)]

    # state dict: per-param `velocity`, indexed in the order given
    def _on_load(self, entries, changed):
        if changed and "lars_weight_decay" in changed:
            self._build_tables()  # seg_wd holds the decay
