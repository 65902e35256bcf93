"""Mixup (reference example/collective/resnet50: --use_mixup/--mixup_alpha,
utils/reader.py create_mixup_reader): each batch is blended with a
permutation of itself, and the loss is the lam-weighted CE of both label
sets (ops.functional.softmax_cross_entropy with labels_b/lam).

Plain torch ops on the loader's device: at 32x3x224x224 the blend is a
~19 MB elementwise pass, not worth a kernel."""
import torch


class MixupLoader:
    """Wraps anything with .next() -> (x, y); .next() yields
    (x_mixed, y_a, y_b, lam):

        lam     ~ Beta(alpha, alpha), ONE draw per batch
        perm    = seeded permutation of the batch
        x_mixed = lam * x + (1 - lam) * x[perm]
        y_a, y_b = y, y[perm]
        lam     -> [B] fp32 tensor on x's device (the loss kernel's
                   per-row weight)

    The draws come from a private seeded CPU generator, so a run is
    reproducible per seed whatever the device. x keeps its memory format
    (channels_last stays channels_last)."""

    def __init__(self, loader, alpha=0.2, seed=0):
        if alpha <= 0:
            raise ValueError("mixup alpha must be > 0, got %r" % (alpha,))
        self.loader = loader
        self.alpha = float(alpha)
        self._gen = torch.Generator().manual_seed(seed)

    def _draw_lam(self):
        # Beta(a, a) = Ga / (Ga + Gb) from two Gamma(a, 1) draws
        # (torch.distributions cannot take a generator)
        a = torch.full((2,), self.alpha, dtype=torch.float64)
        g = torch._standard_gamma(a, generator=self._gen)
        tot = float(g.sum())
        return float(g[0]) / tot if tot > 0 else 0.5

    def next(self):
        x, y = self.loader.next()
        B = x.shape[0]
        lam = self._draw_lam()
        perm = torch.randperm(B, generator=self._gen).to(x.device)
        if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last):
            # gather through the NHWC view: index_select returns a dense
            # tensor in the layout it is GIVEN, so the partner batch (and
            # the blend) stay channels_last with no re-layout copy
            xp = x.permute(0, 2, 3, 1).index_select(0, perm).permute(0, 3, 1, 2)
        else:
            xp = x.index_select(0, perm)
        x_mixed = torch.lerp(xp, x, lam)
        lam_t = torch.full((B,), lam, dtype=torch.float32, device=x.device)
        return x_mixed, y, y.index_select(0, perm), lam_t
