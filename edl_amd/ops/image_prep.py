"""crop_resize_normalize — the image input stage as one op: crop, bilinear
resize, mirror and mean/std normalize of a batch of decoded uint8 RGB images
(reference example/collective/resnet50/dali.py; utils/img_tool.py
random_crop + cv2.resize INTER_LINEAR + flip + normalize).

    packed  flat uint8: B images (HWC, 3 bytes per pixel, rows dense) back
            to back at any byte offsets; sizes differ per image
    table   int32 [B, 8], one row per image (make_table builds it):
              [0] byte offset   [1] H   [2] W   [3] flip (0/1)
              [4..7] the fp32 bits of x0, y0, cw, ch: the source window in
                     pixel units, fractional allowed, cw, ch > 0
    ->      [B, 3, S, S], channels-last, bf16 or fp32

For output (oy, ox) of image b, all in fp32:

    ox' = S-1-ox if flip else ox
    sx  = max(x0, min(x0 + (ox'+0.5)*(cw/S) - 0.5, x0+cw-1))
    xa  = floor(sx), xb = min(xa+1, W-1), fx = sx - xa
    (y alike from oy, y0, ch; never flipped)
    v   = the 4 taps lerped horizontally, then vertically
    out = v * (1/(255*std[c])) - mean[c]/std[c]      (round-to-nearest bf16)

For an integer window this is F.interpolate(crop, (S, S), mode="bilinear",
align_corners=False, antialias=False), then flip, then normalize.

A GPU `packed` ALWAYS takes the HIP kernel (csrc/image_prep.hip; a missing
extension raises); a CPU `packed` runs the torch twin below, which is the
statement of the contract. The table is checked on the host before anything
is launched: pass the HOST table (pinned for an asynchronous upload) and the
op uploads it; a device table is accepted too, at the price of a copy back.
"""
import numpy as np
import torch

from . import ext

FIELDS = 8
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def make_table(rows):
    """rows of (offset, H, W, flip, x0, y0, cw, ch) -> int32 [B, 8] CPU
    tensor, the floats bit-cast."""
    t = np.empty((len(rows), FIELDS), dtype=np.int32)
    fill_table(t, rows)
    return torch.from_numpy(t)


def fill_table(arr, rows):
    """Write rows into the int32 numpy view `arr` [len(rows), 8]."""
    a = np.asarray(rows, dtype=np.float64).reshape(len(rows), FIELDS)
    arr[:, :4] = a[:, :4].astype(np.int64)
    arr[:, 4:] = a[:, 4:].astype(np.float32).view(np.int32)


def validate_table(table, nbytes):
    """Raise ValueError unless every row of the host table names a source
    inside `nbytes` of packed and a window inside that source."""
    if (table.dtype != torch.int32 or table.dim() != 2
            or table.shape[1] != FIELDS or table.shape[0] < 1):
        raise ValueError("image table must be int32 [B >= 1, %d], got %s %s"
                         % (FIELDS, table.dtype, tuple(table.shape)))
    t = table.detach().cpu().contiguous().numpy()
    ints = t[:, :4].astype(np.int64)
    win = np.ascontiguousarray(t[:, 4:]).view(np.float32).astype(np.float64)
    off, H, W, flip = ints.T
    x0, y0, cw, ch = win.T
    with np.errstate(invalid="ignore"):
        checks = (
            ((H >= 1) & (W >= 1), "H, W >= 1"),
            ((off >= 0) & (off + 3 * H * W <= nbytes),
             "offset + 3*H*W <= packed.numel() (%d)" % nbytes),
            ((flip == 0) | (flip == 1), "flip is 0 or 1"),
            (np.isfinite(win).all(axis=1), "a finite window"),
            ((cw > 0) & (ch > 0), "cw, ch > 0"),
            ((x0 >= 0) & (y0 >= 0) & (x0 + cw <= W) & (y0 + ch <= H),
             "the window inside the image"),
        )
    for ok, what in checks:
        if not ok.all():
            b = int(np.argmin(ok))
            raise ValueError(
                "image table row %d violates %s: offset=%d H=%d W=%d flip=%d "
                "window x0=%g y0=%g cw=%g ch=%g"
                % (b, what, off[b], H[b], W[b], flip[b], x0[b], y0[b], cw[b],
                   ch[b]))


def _norm_consts(mean, std):
    if len(mean) != 3 or len(std) != 3 or min(std) <= 0:
        raise ValueError("mean and std need 3 entries, std > 0")
    k = [float(np.float32(1.0 / (255.0 * s))) for s in std]
    b = [float(np.float32(m / s)) for m, s in zip(mean, std)]
    return k, b


def _axis_taps(o, org, ext_, S, n):
    """fp32 taps along one axis for output indices o (already mirrored)."""
    step = ext_ / torch.tensor(float(S), dtype=torch.float32,
                               device=ext_.device)
    s = org + (o + 0.5) * step - 0.5
    s = torch.maximum(org, torch.minimum(s, org + ext_ - 1.0))
    fl = torch.floor(s)
    a = fl.to(torch.int64).clamp_(0, n - 1)
    return a, (a + 1).clamp_(max=n - 1), s - fl


def crop_resize_normalize_torch(packed, table, out_size, mean=IMAGENET_MEAN,
                                std=IMAGENET_STD, out_dtype=torch.float32):
    """The torch twin: the formula above, in fp32, image by image."""
    S = int(out_size)
    k, bias = _norm_consts(mean, std)
    dev = packed.device
    k = torch.tensor(k, dtype=torch.float32, device=dev)
    bias = torch.tensor(bias, dtype=torch.float32, device=dev)
    t = table.cpu()
    win = t[:, 4:].contiguous().view(torch.float32)
    out = torch.empty((t.shape[0], S, S, 3), dtype=torch.float32, device=dev)
    o = torch.arange(S, dtype=torch.float32, device=dev)
    for b in range(t.shape[0]):
        off, H, W, flip = (int(v) for v in t[b, :4])
        x0, y0, cw, ch = win[b].to(dev)
        img = packed[off:off + 3 * H * W].view(H, W, 3).to(torch.float32)
        xa, xb, fx = _axis_taps((S - 1) - o if flip else o, x0, cw, S, W)
        ya, yb, fy = _axis_taps(o, y0, ch, S, H)
        fx = fx.view(1, S, 1)
        fy = fy.view(S, 1, 1)
        ra, rb = img[ya], img[yb]
        top = ra[:, xa] + fx * (ra[:, xb] - ra[:, xa])
        bot = rb[:, xa] + fx * (rb[:, xb] - rb[:, xa])
        out[b] = (top + fy * (bot - top)) * k - bias
    return out.to(out_dtype).permute(0, 3, 1, 2)


def crop_resize_normalize(packed, table, out_size, mean=IMAGENET_MEAN,
                          std=IMAGENET_STD, out_dtype=torch.bfloat16,
                          out=None):
    """-> [B, 3, S, S] channels-last `out_dtype` (bf16 or fp32) on packed's
    device, launched on the current stream with no host sync when `table` is
    a host tensor. `out` (GPU only): a channels-last tensor to write into."""
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("out_dtype must be torch.bfloat16 or torch.float32")
    if packed.dtype != torch.uint8 or packed.dim() != 1:
        raise ValueError("packed must be a flat uint8 tensor")
    if table.is_cuda and not packed.is_cuda:
        raise ValueError("a CPU packed buffer cannot take a GPU table")
    if int(out_size) < 1:
        raise ValueError("out_size >= 1")
    validate_table(table, packed.numel())
    if not packed.is_cuda:
        if out is not None:
            raise ValueError("out= is for the GPU path")
        return crop_resize_normalize_torch(packed, table, out_size, mean, std,
                                           out_dtype)
    C = ext()  # a missing kernel is an error
    dev_table = table.contiguous().to(packed.device, non_blocking=True)
    return C.crop_resize_normalize(
        packed, dev_table, int(out_size), [float(m) for m in mean],
        [float(s) for s in std], out_dtype == torch.bfloat16, out)
