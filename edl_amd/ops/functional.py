"""Autograd wrappers over the HIP kernels + torch reference fallbacks."""
import torch

from . import available, ext


class _KDSoftCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student_logits, teacher_logits):
        ctx.save_for_backward(student_logits, teacher_logits)
        lpr = ext().kd_ce_forward(student_logits, teacher_logits)
        return lpr.mean()

    @staticmethod
    def backward(ctx, gout):
        s, t = ctx.saved_tensors
        gob = float(gout) / s.shape[0] if gout.dim() == 0 else None
        if gob is None:
            gob = gout.item() / s.shape[0]
        ds = ext().kd_ce_backward(s, t, gob)
        return ds, None


class _SoftmaxCE(torch.autograd.Function):
    """Hard-label CE on csrc/softmax_ce.hip -> (mean loss, rank). Unlike
    _KDSoftCE the backward hands gout to the kernel as a DEVICE scalar:
    no host sync, so forward+backward capture into a hipGraph."""

    @staticmethod
    def forward(ctx, logits, labels, labels_b, lam, eps):
        s = logits.contiguous()
        loss_row, lse, rank = ext().softmax_ce_forward(s, labels, labels_b,
                                                       lam, eps)
        ctx.save_for_backward(s, lse, labels, labels_b, lam)
        ctx.eps = eps
        ctx.mark_non_differentiable(rank)
        return loss_row.mean(), rank

    @staticmethod
    def backward(ctx, gout, _grank):
        s, lse, labels, labels_b, lam = ctx.saved_tensors
        ds = ext().softmax_ce_backward(s, lse, labels, labels_b, lam, ctx.eps,
                                       gout.float(), 1.0 / s.shape[0])
        return ds, None, None, None, None


def _softmax_ce_reference(logits, labels, eps, labels_b, lam):
    """Torch reference of csrc/softmax_ce.hip (CPU tests, fp16): same
    formulas, same tie rule (ties go to the lower index), same
    out-of-range-label rule (no target term, rank = C)."""
    s = logits.float()
    C = s.shape[1]

    def pick(y):
        ok = (y >= 0) & (y < C)
        return s.gather(1, y.clamp(0, C - 1)[:, None])[:, 0] * ok, ok

    sa, a_ok = pick(labels)
    tgt = sa
    if labels_b is not None:
        tgt = lam * sa + (1.0 - lam) * pick(labels_b)[0]
    loss_row = (torch.logsumexp(s, dim=1) - (1.0 - eps) * tgt
                - (eps / C) * s.sum(1))
    with torch.no_grad():
        sd, col = s.detach(), torch.arange(C, device=s.device)
        rank = ((sd > sa.detach()[:, None])
                | ((sd == sa.detach()[:, None]) & (col < labels[:, None]))).sum(1)
        rank = torch.where(a_ok, rank, torch.full_like(rank, C)).to(torch.int32)
    return loss_row.mean(), rank


def softmax_cross_entropy(logits, labels, label_smoothing=0.0, labels_b=None,
                          lam=None, return_rank=False):
    """Mean hard-label cross-entropy of [B,C] logits with label smoothing
    and optional mixup — the reference trainer's calc_loss
    (example/collective/resnet50/train_with_fleet.py): per row
    lam*CE(labels) + (1-lam)*CE(labels_b) on eps-smoothed one-hots.
    `lam` is a python float or a [B] tensor; labels_b and lam go together.

    return_rank=True also returns rank[B] (int32): how many classes score
    above the true class `labels`, ties counted for the lower index —
    top-k correct is rank < k. A label outside [0,C) contributes no
    target term and reports rank = C."""
    if (labels_b is None) != (lam is None):
        raise ValueError("labels_b and lam must be given together")
    B = logits.shape[0]
    labels = labels.long().contiguous()
    if labels_b is not None:
        labels_b = labels_b.long().contiguous()
        if not torch.is_tensor(lam):
            lam = torch.full((B,), float(lam), device=logits.device)
        lam = lam.detach().to(device=logits.device, dtype=torch.float32)
        lam = lam.expand(B).contiguous()
    eps = float(label_smoothing)
    if (logits.is_cuda and available()
            and logits.dtype in (torch.float32, torch.bfloat16)):
        loss, rank = _SoftmaxCE.apply(logits, labels, labels_b, lam, eps)
    else:
        loss, rank = _softmax_ce_reference(logits, labels, eps, labels_b, lam)
    return (loss, rank) if return_rank else loss


def kd_soft_cross_entropy(student_logits, teacher_logits):
    """mean_i CE(softmax(teacher_i), student_i) — the KD loss of the
    reference distill example (soft_label cross_entropy,
    example/distill/resnet/train_with_fleet.py:254-259)."""
    if student_logits.is_cuda and available():
        t = teacher_logits.detach()
        if t.dtype != student_logits.dtype:
            t = t.to(student_logits.dtype)
        return _KDSoftCE.apply(student_logits, t)
    # torch reference (CPU tests / numerics baseline)
    logp = torch.log_softmax(student_logits.float(), dim=1)
    soft = torch.softmax(teacher_logits.detach().float(), dim=1)
    return -(soft * logp).sum(1).mean()
