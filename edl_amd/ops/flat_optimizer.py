"""FlatBucketOptimizer — what FusedSGD, FusedAdam and FusedLARS share.

BucketedAllReducer re-homes params and grads into flat per-bucket buffers,
so an optimizer here is one update over (p, g, state...) per bucket with the
DP gradient average folded in as grad_scale. This base owns everything that
does not depend on the update rule: the reducer attachment, the LR device
scalar, the walk over the reducer's buckets that builds the per-bucket
dicts, the per-bucket decay segment tables, the CPU handling of a clip
state, and the per-param state dict (so checkpoints survive re-bucketing
across elastic resizes). A subclass names its state buffers and state-dict
keys, builds its own tables in _on_materialize() and writes step().

Buckets on a GPU ALWAYS take the HIP kernels: FusedAdam and FusedLARS raise
there without the built extension (ops.ext()) — a missing kernel is an
error in this project, not a slower path taken quietly. FusedSGD alone
keeps a `_use_ext` switch and runs its torch math on a GPU without the
extension (bring-up)."""
import torch

from ..train.bucketed_ddp import _view_like

MAX_SEGMENTS = 1024  # == _C.ADAM_MAX_SEGMENTS (csrc/launchers.h)


class FlatBucketOptimizer:
    handles_grad_scale = True

    _name = "FlatBucketOptimizer"  # class name used in messages
    _state_names = ()     # zero state buffers per bucket dict, e.g. ("m", "v")
    _state_keys = {}      # state-dict key -> state buffer name
    _hyper_keys = ()      # hyper-parameters load_state_dict() takes
    _bucket_order = False  # state dict indexed in bucket order (FusedSGD)
    _decay_key = "weight_decay"  # the param group's decay
    _select_key = None    # param-group key of the selection set
    _table_kind = "segment"
    _cap_message = ("a bucket needs %d segments; the kernel's table holds %d "
                    "per bucket (use a smaller bucket cap)")

    def __init__(self, params, defaults, select=None, grad_scale=1.0,
                 reducer=None):
        # state-dict (and trust) indices follow the order given, as
        # torch.optim does
        self._all_params = list(params)
        self._index = {id(p): i for i, p in enumerate(self._all_params)}
        # params exempt from decay (no_decay / exclude):
        # None | predicate param -> bool | iterable of params
        if select is None:
            picked = []
        elif callable(select):
            picked = [i for i, p in enumerate(self._all_params) if select(p)]
        else:
            ids = {id(p) for p in select}
            picked = [i for i, p in enumerate(self._all_params) if id(p) in ids]
        self._selected = set(picked)
        self.defaults = dict(defaults)
        if self._select_key is not None:
            self.defaults[self._select_key] = sorted(picked)
        self.param_groups = [dict(
            self.defaults,
            params=[p for p in self._all_params if p.requires_grad])]
        self.grad_scale = grad_scale
        self._reducer = reducer
        self._buckets = None  # list of per-bucket dicts, see _materialize()
        self._use_ext = True
        # LR lives in a device scalar on GPU: the update kernel reads it at
        # run time, so a hipGraph-captured step tracks set_lr() on replay
        # instead of freezing the capture-time value (warmup/decay schedules
        # keep working under graph capture).
        self._lr_dev = None
        if reducer is not None:
            self.attach(reducer)

    def attach(self, reducer):
        self._reducer = reducer
        self._buckets = None
        reducer._attached_opt = self  # rebuild() snapshots/restores the state
        return self

    def drop_buckets(self):
        """The reducer re-bucketed: re-materialize against the new flats."""
        self._buckets = None

    def set_lr(self, lr):
        """Set the learning rate (updates the device scalar when present)."""
        for g in self.param_groups:
            g["lr"] = float(lr)
        if self._lr_dev is not None:
            self._lr_dev.fill_(float(lr))

    def zero_grad(self, set_to_none=False):
        if self._reducer is not None:
            self._reducer.zero_grad()

    def _materialize(self):
        """-> one dict per bucket: p, g (the reducer's flats), one zero
        buffer per _state_names, params, offsets [(start, numel)], and
        whatever _on_materialize() adds (segs, seg_end, seg_wd, ...)."""
        if self._buckets is not None:
            return self._buckets
        r = self._reducer
        if r is None:
            raise RuntimeError(
                "%s needs a BucketedAllReducer (call attach())" % self._name)
        out = []
        for b in r._buckets:
            if b.param_flat is None:
                raise RuntimeError(
                    "%s requires flatten_params=True buckets" % self._name)
            offsets = []
            off = 0
            for p in b.params:
                offsets.append((off, p.numel()))
                off += p.numel()
            bk = {"p": b.param_flat, "g": b.buffer, "params": b.params,
                  "offsets": offsets}
            for name in self._state_names:
                bk[name] = torch.zeros_like(b.param_flat)
            out.append(bk)
        if self._bucket_order:
            self._index = {id(p): i for i, p in enumerate(
                p for bk in out for p in bk["params"])}
        self._buckets = out
        try:
            self._on_materialize(out)
        except Exception:
            self._buckets = None  # half-built tables never step
            raise
        if out:
            dev = out[0]["p"].device
            if dev.type == "cuda" and self._use_ext and self._lr_dev is None:
                self._lr_dev = torch.full(
                    (1,), self.param_groups[0]["lr"], dtype=torch.float32,
                    device=dev)
        return out

    def _on_materialize(self, buckets):
        """Subclass hook: tables and extra device state for new buckets."""

    # ---- decay segments ----
    def _param_wd(self, p):
        wd = self.param_groups[0][self._decay_key]
        return 0.0 if self._index.get(id(p)) in self._selected else wd

    def _build_segments(self, bk, merge, always_table=False,
                        with_tensor=False):
        """bk["segs"] = [end, wd(, param index)] per segment: adjacent
        params coalesce where merge(previous wd, wd). On a GPU, when there
        is more than one segment (or always_table), also the kernel's
        device tables bk["seg_end"], bk["seg_wd"](, bk["seg_tensor"])."""
        segs = []
        for (off, n), p in zip(bk["offsets"], bk["params"]):
            wd = self._param_wd(p)
            if segs and merge(segs[-1][1], wd):
                segs[-1][0] = off + n
            elif with_tensor:
                segs.append([off + n, wd, self._index[id(p)]])
            else:
                segs.append([off + n, wd])
        bk["segs"] = segs
        bk["seg_end"] = bk["seg_wd"] = bk["seg_tensor"] = None
        if not (bk["p"].is_cuda and (always_table or len(segs) > 1)):
            return
        if len(segs) > MAX_SEGMENTS:
            raise RuntimeError("%s: " % self._name + self._cap_message
                               % (len(segs), MAX_SEGMENTS))
        # checked HERE, on the host lists: the bindings can only check a
        # device table with a D2H sync, which they cannot afford under
        # graph capture
        ends = [s[0] for s in segs]
        if (ends != sorted(ends) or ends[-1] != bk["p"].numel()
                or bk["p"].numel() >= 2 ** 31):
            raise RuntimeError("%s: malformed %s table"
                               % (self._name, self._table_kind))
        dev = bk["p"].device
        bk["seg_end"] = torch.tensor(ends, dtype=torch.int32, device=dev)
        bk["seg_wd"] = torch.tensor([s[1] for s in segs],
                                    dtype=torch.float32, device=dev)
        if with_tensor:
            bk["seg_tensor"] = torch.tensor([s[2] for s in segs],
                                            dtype=torch.int32, device=dev)

    # ---- CPU twins of the kernels' clip prelude ----
    def _cpu_scale(self, clip_state):
        """The gradient scale as the kernels form it, an fp32 product of
        grad_scale and the clip coefficient; None for a skipped step."""
        s = torch.tensor(self.grad_scale, dtype=torch.float32)
        if clip_state is not None:
            if bool(clip_state[2] != 0):
                return None
            s = s * clip_state[0]
        return s

    def _cpu_grad(self, bk, clip_state):
        """The bucket's scaled gradient (bk["g"] itself when the scale is
        1); None for a skipped step."""
        if clip_state is None:
            g = bk["g"]
            return g if self.grad_scale == 1.0 else g.mul(self.grad_scale)
        s = self._cpu_scale(clip_state)
        return None if s is None else bk["g"].mul(s)

    # ---- state ----
    def state_buffers(self):
        """Every tensor that must agree across ranks (the engine broadcasts
        them from rank 0): the state buffers of every bucket."""
        return [bk[name] for bk in self._materialize()
                for name in self._state_names]

    def _state_entry(self):
        """Subclass hook: tensors every param's state-dict entry carries
        beside the buffers (each entry gets its own copy)."""
        return {}

    def state_dict(self):
        state = {}
        extra = self._state_entry()  # once: it may read the device back
        for bk in self._materialize():
            for (off, n), p in zip(bk["offsets"], bk["params"]):
                ent = {k: v.clone() for k, v in extra.items()}
                for key, name in self._state_keys.items():
                    ent[key] = _view_like(bk[name][off:off + n], p).clone()
                state[self._index[id(p)]] = ent
        state = {k: state[k] for k in sorted(state)}
        groups = [{k: v for k, v in self.param_groups[0].items() if k != "params"}]
        if self._select_key is not None:
            groups[0][self._select_key] = sorted(self._selected)
        groups[0]["params"] = list(range(
            len(state) if self._bucket_order else len(self._all_params)))
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        """The state buffers and _hyper_keys are taken from `sd`. The
        selection set (no_decay / exclude) is this optimizer's
        construction-time choice: a state dict that records another one is
        refused with a ValueError before anything is loaded, rather than
        silently changing what weight decay means mid-run."""
        src = sd["param_groups"][0] if sd.get("param_groups") else None
        key = self._select_key
        if (src and key in src
                and sorted(src[key]) != sorted(self._selected)):
            raise ValueError(
                "%s: state dict records %s=%s, this optimizer %s" % (
                    self._name, key, sorted(src[key]), sorted(self._selected)))
        state = sd.get("state", {})
        found = []
        for bk in self._materialize():
            for (off, n), p in zip(bk["offsets"], bk["params"]):
                idx = self._index[id(p)]
                ent = state.get(idx, state.get(str(idx)))
                if not ent:
                    continue
                found.append(ent)
                for key, name in self._state_keys.items():
                    if ent.get(key) is not None:
                        _view_like(bk[name][off:off + n], p).copy_(
                            ent[key].to(bk[name].device))
        changed = None  # the hyper-parameters that moved, None: none given
        if src is not None:
            g0 = self.param_groups[0]
            changed = set()
            for k in self._hyper_keys:
                if k in src:
                    v = src[k]
                    v = (tuple(float(x) for x in v)
                         if isinstance(v, (tuple, list)) else float(v))
                    if v != g0[k]:
                        changed.add(k)
                    g0[k] = v
            if self._lr_dev is not None:
                self._lr_dev.fill_(float(g0["lr"]))
        self._on_load(found, changed)

    def _on_load(self, entries, changed):
        """Subclass hook after load_state_dict(): the state entries that
        were found, the hyper-parameter keys that changed (None when the
        state dict carried no param groups)."""
