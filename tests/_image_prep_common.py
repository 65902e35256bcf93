"""What the image-input tests share: the float64 statement of the
crop_resize_normalize contract (the oracle; never the code under test), one
batch that holds every edge case at once, and a set of PNG files."""
import numpy as np
import torch

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)

# fp32 bound, normalised units: torch's own fp32 bilinear sits 8.7e-4 pixel
# units from the float64 formula on sources <= 70 px, 1.5e-5 after the
# 1/(255*0.224) scaling; 1e-4 leaves ~6x for another valid fp32 order.
TOL_F32 = 1e-4


def tol_bf16(oracle):
    """round-to-nearest is 2^-9 relative; doubled for double rounding at
    ties, plus the fp32 bound."""
    return 2.0 ** -8 * np.abs(oracle) + 1e-4


def oracle_f64(packed, rows, S, mean=MEAN, std=STD):
    """packed: uint8 numpy; rows: (offset, H, W, flip, x0, y0, cw, ch) with
    the window as the table holds it (fp32 values) -> float64 [B, 3, S, S]."""
    out = np.empty((len(rows), 3, S, S), dtype=np.float64)
    k = 1.0 / (255.0 * np.asarray(std, dtype=np.float64))
    bias = np.asarray(mean, dtype=np.float64) / np.asarray(std, np.float64)

    def taps(o, org, ext, n):
        s = org + (o + 0.5) * (ext / S) - 0.5
        s = np.maximum(org, np.minimum(s, org + ext - 1.0))
        a = np.floor(s).astype(np.int64)
        return a, np.minimum(a + 1, n - 1), s - a

    o = np.arange(S, dtype=np.float64)
    for b, (off, H, W, flip, x0, y0, cw, ch) in enumerate(rows):
        x0, y0, cw, ch = (float(np.float32(v)) for v in (x0, y0, cw, ch))
        img = packed[off:off + 3 * H * W].reshape(H, W, 3).astype(np.float64)
        xa, xb, fx = taps((S - 1) - o if flip else o, x0, cw, W)
        ya, yb, fy = taps(o, y0, ch, H)
        fx = fx[None, :, None]
        fy = fy[:, None, None]
        top = img[ya][:, xa] + fx * (img[ya][:, xb] - img[ya][:, xa])
        bot = img[yb][:, xa] + fx * (img[yb][:, xb] - img[yb][:, xa])
        v = top + fy * (bot - top)
        out[b] = (v * k - bias).transpose(2, 0, 1)
    return out


def edge_batch(seed=0):
    """-> (packed uint8 numpy, rows): 9 sources with odd extents at byte
    offsets of every alignment, holding at once an upscale (5x7 window), a
    downscale (61x47), windows touching each image edge, the full image, a
    1x1 window and a 1x1 image, fractional eval-style windows, flip on and
    off."""
    rng = np.random.RandomState(seed)
    # (H, W), gap of junk bytes before the source, flip, (x0, y0, cw, ch)
    spec = [
        ((23, 37), 1, 0, (0, 0, 37, 23)),            # full image
        ((23, 37), 0, 1, (4, 9, 5, 7)),              # upscale, flipped
        ((50, 64), 2, 0, (2, 1, 61, 47)),            # downscale
        ((1, 1), 0, 1, (0, 0, 1, 1)),                # 1x1 image
        ((5, 64), 3, 0, (63, 4, 1, 1)),              # 1x1 window, corner
        ((5, 64), 0, 1, (0, 0, 10, 5)),              # left + top + bottom
        ((64, 5), 1, 0, (2, 30, 3, 34)),             # right + bottom edge
        ((41, 29), 2, 1, (1.8125, 7.8125, 25.375, 25.375)),   # eval-style
        ((33, 47), 0, 0, (7.21875, 0.21875, 32.5625, 32.5625)),
    ]
    chunks, rows, off = [], [], 0
    for (H, W), gap, flip, win in spec:
        chunks.append(rng.randint(0, 256, gap).astype(np.uint8))
        off += gap
        chunks.append(rng.randint(0, 256, 3 * H * W).astype(np.uint8))
        rows.append((off, H, W, flip) + tuple(win))
        off += 3 * H * W
    packed = np.concatenate(chunks)
    assert {r[0] % 4 for r in rows} == {0, 1, 2, 3}
    return packed, rows


PNG_SIZES = [(37, 23), (64, 48), (1, 1), (5, 64), (64, 5), (50, 50),
             (33, 47), (80, 61), (24, 24), (41, 29)]  # (H, W)


def write_pngs(root, seed=0):
    """10 PNGs of different sizes under root -> `relpath label` records."""
    from PIL import Image

    rng = np.random.RandomState(seed)
    records = []
    for i, (H, W) in enumerate(PNG_SIZES):
        # smooth ramps plus noise: resampling errors show, and the mirror
        # and the crop position change the picture
        yy, xx = np.mgrid[0:H, 0:W]
        img = np.stack([(xx * 255) // max(W - 1, 1),
                        (yy * 255) // max(H - 1, 1),
                        rng.randint(0, 256, (H, W))], axis=2).astype(np.uint8)
        name = "img%d.png" % i
        Image.fromarray(img, "RGB").save(str(root / name))
        records.append("%s %d" % (name, (7 * i) % 10))
    return records


def to_np64(t):
    return t.detach().to(torch.float64).cpu().numpy()
