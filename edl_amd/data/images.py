"""Image files -> device batches: the last hop of the input pipeline
(reference example/collective/resnet50/dali.py, and its CPU twin
utils/img_tool.py + utils/reader.py).

Records are `relpath label` lines (the reference's train_list.txt format and
what the elastic data plane delivers). Per record the host decodes the file
(PIL, in a thread pool), draws the augmentation window, and copies ONLY the
window's bounding rectangle, as uint8, into a pinned staging buffer; one
upload and one kernel (ops.image_prep.crop_resize_normalize) then resample,
mirror and normalize the whole batch into the channels-last tensor the stem
reads. Train: random-area/aspect crop + coin-flip mirror (img_tool.py
random_crop). Eval: resize-short then centre-crop, folded into one resample.
"""
import hashlib
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ..ops.image_prep import (FIELDS, IMAGENET_MEAN, IMAGENET_STD,
                              crop_resize_normalize, fill_table)


def draw_train_window(H, W, gen, lower_scale=0.08, lower_ratio=3.0 / 4.0,
                      upper_ratio=4.0 / 3.0):
    """The reference's random_crop window for an H x W image, plus the
    mirror coin -> (x0, y0, cw, ch, flip), all integers.

    aspect = sqrt(U(lower_ratio, upper_ratio)); the area fraction is drawn
    from U(min(lower_scale, bound), min(1, bound)) with `bound` the largest
    fraction at which a window of that aspect still fits; w, h are truncated
    to integers (and kept >= 1), the corner is uniform over what is left.
    All draws come from `gen` (a torch.Generator)."""
    u = torch.rand(5, generator=gen, dtype=torch.float64).tolist()
    aspect = math.sqrt(lower_ratio + (upper_ratio - lower_ratio) * u[0])
    w, h = aspect, 1.0 / aspect
    bound = min((float(W) / H) / (w * w), (float(H) / W) / (h * h))
    scale_max = min(1.0, bound)
    scale_min = min(lower_scale, bound)
    area = H * W * (scale_min + (scale_max - scale_min) * u[1])
    side = math.sqrt(area)
    cw = min(max(int(side * w), 1), W)
    ch = min(max(int(side * h), 1), H)
    y0 = min(int(u[2] * (H - ch + 1)), H - ch)
    x0 = min(int(u[3] * (W - cw + 1)), W - cw)
    return x0, y0, cw, ch, int(u[4] < 0.5)


def eval_window(H, W, crop=224, resize_short=256):
    """≈ the reference's validation pipe (resize the short side to
    `resize_short`, centre-crop `crop`) as ONE source window: a centred
    square of side crop/resize_short * min(H, W), fractional, no mirror
    -> (x0, y0, cw, ch, 0). Only ≈: the reference rounds the resized extent
    to whole pixels before it crops."""
    side = float(crop) / float(resize_short) * min(H, W)
    return (W - side) / 2.0, (H - side) / 2.0, side, side, 0


def parse_record(rec):
    """`relpath label` -> (relpath, int label); the path may hold spaces."""
    path, _, label = rec.strip().rpartition(" ")
    if not path or not label.lstrip("-").isdigit():
        raise ValueError("image record must be `relpath label`, got %r" % rec)
    return path.strip(), int(label)


def record_seed(seed, epoch, rec):
    """The generator seed of a record's augmentation draw: a function of
    (seed, epoch, md5(record)) alone, so a record yields the same pixels
    whichever rank or world size draws it."""
    h = hashlib.md5(rec.encode("utf-8", "replace")).hexdigest()
    d = hashlib.md5(("%d:%d:%s" % (seed, epoch, h)).encode()).digest()
    return int.from_bytes(d[:8], "little") & ((1 << 63) - 1)


class _Slot:
    """One staging buffer of the ring: uint8 bytes + the table, pinned on a
    GPU loader, and the event after which the host may overwrite them."""

    def __init__(self, batch_size, pin):
        self.pin = pin
        self.table = self._alloc(batch_size * FIELDS * 4).view(torch.int32) \
            .view(batch_size, FIELDS)
        self.bytes = self._alloc(1 << 16)
        self.event = None

    def _alloc(self, n):
        return torch.empty(n, dtype=torch.uint8, pin_memory=self.pin)

    def reserve(self, n):
        if self.bytes.numel() < n:  # grow with headroom: sizes vary per batch
            self.bytes = self._alloc(n + n // 4)
        return self.bytes


class ImageRecordLoader:
    """TrainerEngine loader (.next() -> (images, labels), .steps()) over
    image files; MixupLoader and TrainerEngine.train_epoch / evaluate take it
    unchanged. Like RecordImageSet it cycles its records for as long as
    next() is called.

    Batch i+1 is decoded by the pool, packed, uploaded and resampled on a
    side stream while step i computes; next() hands a batch over with
    wait_stream / record_stream as SyntheticImageNet does. On a CPU device
    the same code runs through the op's torch twin, without streams."""

    def __init__(self, records, image_root, batch_size, device, out_size=224,
                 train=True, seed=0, epoch=0, out_dtype=None, num_workers=8,
                 depth=2, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 lower_scale=0.08, lower_ratio=3.0 / 4.0,
                 upper_ratio=4.0 / 3.0, resize_short=None):
        if not records:
            raise ValueError("ImageRecordLoader: no records")
        self.records = list(records)
        self.image_root = image_root
        self.batch_size = int(batch_size)
        self.device = torch.device(device)
        self.out_size = int(out_size)
        self.train = bool(train)
        self.seed, self.epoch = int(seed), int(epoch)
        cuda = self.device.type == "cuda"
        if out_dtype is None:
            out_dtype = torch.bfloat16 if cuda else torch.float32
        self.out_dtype = out_dtype
        self.mean, self.std = tuple(mean), tuple(std)
        self.crop_args = (lower_scale, lower_ratio, upper_ratio)
        # eval: the reference's 224-of-256 centre crop, scaled to out_size
        self.resize_short = (self.out_size * 256.0 / 224.0
                             if resize_short is None else float(resize_short))
        if self.resize_short < self.out_size:
            raise ValueError("resize_short (%g) must be >= out_size (%d)"
                             % (self.resize_short, self.out_size))
        self._pool = ThreadPoolExecutor(max(1, int(num_workers)),
                                        thread_name_prefix="edl-img")
        self._slots = [_Slot(self.batch_size, cuda)
                       for _ in range(max(1, int(depth)))]
        self._stream = torch.cuda.Stream(self.device) if cuda else None
        self._cursor = 0   # next record to submit for decoding
        self._batch = 0    # batches packed so far (picks the ring slot)
        self._decoding = []
        self._next = None
        for _ in self._slots:
            self._submit()
        self._prefetch()

    def steps(self):
        return len(self.records) // self.batch_size

    def close(self):
        self._pool.shutdown(wait=False, cancel_futures=True)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    # -- host side ---------------------------------------------------------
    def _load(self, rec):
        """-> (crop uint8 [h, w, 3], x0, y0, cw, ch, flip, label) with the
        window rebased to the crop: the window's integer bounding rectangle
        plus the one extra tap column and row, clipped to the image."""
        try:
            from PIL import Image

            path, label = parse_record(rec)
            with Image.open(os.path.join(self.image_root, path)) as im:
                img = np.asarray(im.convert("RGB"), dtype=np.uint8)
        except Exception as e:  # noqa: BLE001
            raise RuntimeError("cannot decode image record %r: %s: %s"
                               % (rec, type(e).__name__, e)) from e
        H, W = img.shape[:2]
        if self.train:
            gen = torch.Generator().manual_seed(
                record_seed(self.seed, self.epoch, rec))
            x0, y0, cw, ch, flip = draw_train_window(H, W, gen,
                                                     *self.crop_args)
        else:
            x0, y0, cw, ch, flip = eval_window(H, W, self.out_size,
                                               self.resize_short)
        xl, yl = int(math.floor(x0)), int(math.floor(y0))
        xh = min(W, int(math.ceil(x0 + cw)) + 1)
        yh = min(H, int(math.ceil(y0 + ch)) + 1)
        crop = np.ascontiguousarray(img[yl:yh, xl:xh])
        return crop, x0 - xl, y0 - yl, cw, ch, flip, label

    def _submit(self):
        futs = []
        for _ in range(self.batch_size):
            rec = self.records[self._cursor % len(self.records)]
            self._cursor += 1
            futs.append(self._pool.submit(self._load, rec))
        self._decoding.append(futs)

    def _pack(self, items, slot):
        """Crops back to back into the slot's bytes, rows into its table
        -> (packed view, table, labels)."""
        total = sum(it[0].size for it in items)
        buf = slot.reserve(total)
        flat = buf.numpy()
        rows, off = [], 0
        for crop, x0, y0, cw, ch, flip, _ in items:
            n = crop.size
            flat[off:off + n] = crop.reshape(-1)
            rows.append((off, crop.shape[0], crop.shape[1], flip,
                         x0, y0, cw, ch))
            off += n
        fill_table(slot.table.numpy(), rows)
        labels = torch.tensor([it[6] for it in items], dtype=torch.long)
        return buf[:total], slot.table, labels

    # -- device side -------------------------------------------------------
    def _prefetch(self):
        items = [f.result() for f in self._decoding.pop(0)]
        self._submit()
        slot = self._slots[self._batch % len(self._slots)]
        self._batch += 1
        if slot.event is not None:
            slot.event.synchronize()  # its last upload has left the buffer
        packed, table, labels = self._pack(items, slot)
        if self._stream is None:
            x = crop_resize_normalize(packed, table, self.out_size, self.mean,
                                      self.std, self.out_dtype)
            self._next = (x, labels)
            return
        with torch.cuda.stream(self._stream):
            dev = packed.to(self.device, non_blocking=True)
            x = crop_resize_normalize(dev, table, self.out_size, self.mean,
                                      self.std, self.out_dtype)
            y = labels.pin_memory().to(self.device, non_blocking=True)
            slot.event = torch.cuda.Event()
            slot.event.record(self._stream)
        self._next = (x, y)

    def next(self):
        """-> (images, labels) on the device; prepares the following batch."""
        if self._stream is not None:
            torch.cuda.current_stream().wait_stream(self._stream)
        batch = self._next
        if self._stream is not None:
            # the tensors are consumed on the compute stream
            batch[0].record_stream(torch.cuda.current_stream())
            batch[1].record_stream(torch.cuda.current_stream())
        self._prefetch()
        return batch
