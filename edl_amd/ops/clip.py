"""GradClipper — global-norm gradient clipping over the reducer's flat
buckets, with nothing on the host between the reduction and the update.

torch.nn.utils.clip_grad_norm_ cannot be used from outside: the gradients
live as views into flat buckets, the 1/world average is folded into the
update kernels (the true gradient is never materialised), and a whole step
replays as one hipGraph, where no host code, `.item()` or data-dependent
branch runs. So the clip is a 4-float DEVICE state

    state = [coef, norm, skip, nskipped]
      norm = grad_scale * sqrt(sum of squares over all buckets)
      coef = min(1, max_norm / (norm + 1e-6))     (clip_grad_norm_'s rule)
      skip = 1 when skip_nonfinite is on and norm is inf/nan (then coef = 0
             and nskipped counts one more), else 0

that two HIP launches write (edl_amd._C.grad_sumsq over all buckets, then
grad_clip_finalize) and FusedSGD.step / FusedAdam.step take as
`clip_state=`: their kernels multiply the gradient scale by coef, or leave
p, m, v untouched on skip. The sum runs in double and uses no atomics, so
every rank computes the same bits from the same all-reduced buckets and no
extra collective is needed.

max_norm=None is the norm-only mode (coef stays 1): `norm` is still
reported and skip_nonfinite still guards the step. Buckets on a GPU ALWAYS
take the kernels (a missing extension raises); CPU buckets (tests, gloo)
run the same rule in torch with a double sum."""
import math

import torch

from . import ext

COEF, NORM, SKIP, NSKIPPED = 0, 1, 2, 3


class GradClipper:
    def __init__(self, reducer, max_norm=None, skip_nonfinite=False):
        max_norm = math.inf if max_norm is None else float(max_norm)
        if not max_norm >= 0.0:
            raise ValueError("GradClipper: max_norm must be >= 0 or None")
        self.max_norm = max_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        self._reducer = reducer
        self._bufs = None
        self._partial = None
        self._rows = 0
        # survives a rebuild: nskipped keeps counting
        self.state = None
        reducer.register_rebuild_callback(self._rebuilt)

    def _rebuilt(self):
        self._bufs = None  # the buckets were re-made: look at the new flats
        self._partial = None

    def _materialize(self):
        if self._bufs is not None:
            return self._bufs
        bufs = [b.buffer for b in self._reducer._buckets]
        for b in bufs:
            if b.dtype != torch.float32:
                raise RuntimeError("GradClipper needs fp32 gradient buckets")
        dev = bufs[0].device if bufs else torch.device("cpu")
        if self.state is None or self.state.device != dev:
            self.state = torch.zeros(4, dtype=torch.float32, device=dev)
        if dev.type == "cuda":
            C = ext()  # a missing kernel is an error
            self._rows = sum(C.grad_norm_rows(b.numel()) for b in bufs)
            # every row is written on every launch: no fill needed
            self._partial = torch.empty(max(self._rows, 1),
                                        dtype=torch.float64, device=dev)
        self._bufs = bufs
        return bufs

    @torch.no_grad()
    def run(self, grad_scale=1.0):
        """Reduce the buckets as they stand (after reducer.finalize()) and
        write the state; grad_scale is what the optimizer will multiply
        the gradients by (1/world, times 1/loss-scale under fp16).
        -> the state tensor, for opt.step(clip_state=...)."""
        bufs = self._materialize()
        st = self.state
        if st.is_cuda:
            C = ext()
            rows = C.grad_sumsq(bufs, self._partial)
            C.grad_clip_finalize(self._partial, rows, st, float(grad_scale),
                                 self.max_norm, self.skip_nonfinite)
            return st
        total = torch.zeros((), dtype=torch.float64)
        for b in bufs:
            total += b.double().pow(2).sum()
        norm = (total.sqrt() * float(grad_scale)).float()
        q = self.max_norm / (norm + 1e-6)
        # torch.clamp(max=1) semantics: a NaN quotient stays NaN
        coef = torch.where(q > 1.0, torch.ones_like(q), q)
        skip = torch.zeros_like(norm)
        if self.skip_nonfinite:
            skip = (~torch.isfinite(norm)).float()
            coef = torch.where(skip != 0, torch.zeros_like(coef), coef)
            st[NSKIPPED] += skip
        st[COEF] = coef
        st[NORM] = norm
        st[SKIP] = skip
        return st

    @property
    def norm(self):
        """The last global gradient norm: a [1] view of the state (device
        tensor, overwritten by every run; no host sync)."""
        self._materialize()
        return self.state[NORM:NORM + 1]

    @property
    def skipped(self):
        """Steps skipped so far for a non-finite norm: a [1] fp32 view."""
        self._materialize()
        return self.state[NSKIPPED:NSKIPPED + 1]
