"""The image input stage on the CPU: the torch twin of
crop_resize_normalize against the float64 contract, the window draws, and
ImageRecordLoader end to end (through the trainer too)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _image_prep_common import (MEAN, STD, TOL_F32, edge_batch, oracle_f64,
                                to_np64, write_pngs)

from edl_amd.data.images import (ImageRecordLoader, draw_train_window,
                                 eval_window)
from edl_amd.data.mixup import MixupLoader
from edl_amd.ops.image_prep import (crop_resize_normalize, make_table,
                                    validate_table)


@pytest.fixture(scope="module")
def edge():
    packed, rows = edge_batch()
    refs = {S: oracle_f64(packed, rows, S) for S in (1, 7, 20, 32)}
    return packed, rows, refs


@pytest.mark.parametrize("S", [1, 7, 20, 32])
def test_twin_matches_float64_formula(edge, S):
    packed, rows, refs = edge
    out = crop_resize_normalize(torch.from_numpy(packed), make_table(rows), S,
                                MEAN, STD, torch.float32)
    assert out.shape == (len(rows), 3, S, S) and out.dtype == torch.float32
    assert out.is_contiguous(memory_format=torch.channels_last)
    err = np.abs(to_np64(out) - refs[S]).max()
    print("S=%d twin vs float64 formula: %.3g" % (S, err))
    assert err <= TOL_F32


def test_twin_bf16_is_rounded_fp32(edge):
    packed, rows, _ = edge
    p, t = torch.from_numpy(packed), make_table(rows)
    f = crop_resize_normalize(p, t, 20, MEAN, STD, torch.float32)
    h = crop_resize_normalize(p, t, 20, MEAN, STD, torch.bfloat16)
    assert h.dtype == torch.bfloat16 and torch.equal(h, f.to(torch.bfloat16))


def test_twin_matches_interpolate_on_integer_windows(edge):
    """Integer windows: the contract is F.interpolate(bilinear, no
    antialias) + flip + normalize. Bound: the twin's fp32 bound against the
    formula plus torch's own distance from it (8.7e-4 pixel units measured
    on such shapes, 1.5e-5 normalised)."""
    packed, rows, _ = edge
    rows = [r for r in rows if all(float(v).is_integer() for v in r[4:])]
    assert len(rows) >= 6
    S = 20
    out = crop_resize_normalize(torch.from_numpy(packed), make_table(rows), S,
                                MEAN, STD, torch.float32)
    mean = torch.tensor(MEAN).view(3, 1, 1)
    std = torch.tensor(STD).view(3, 1, 1)
    worst = 0.0
    for b, (off, H, W, flip, x0, y0, cw, ch) in enumerate(rows):
        img = torch.from_numpy(packed[off:off + 3 * H * W].reshape(H, W, 3))
        crop = img[y0:y0 + ch, x0:x0 + cw].permute(2, 0, 1).float()[None]
        ref = F.interpolate(crop, (S, S), mode="bilinear",
                            align_corners=False, antialias=False)[0]
        if flip:
            ref = ref.flip(2)
        ref = (ref / 255.0 - mean) / std
        worst = max(worst, float((out[b] - ref).abs().max()))
    print("twin vs F.interpolate: %.3g" % worst)
    assert worst <= TOL_F32 + 1.5e-5


@pytest.mark.parametrize("bad, what", [
    (dict(off=10 ** 6), "offset"),
    (dict(H=0), "H, W"),
    (dict(x0=30.0, cw=10.0), "window"),
    (dict(cw=0.0), "cw, ch"),
])
def test_validate_table_rejects(bad, what):
    row = dict(off=0, H=23, W=37, flip=0, x0=0.0, y0=0.0, cw=37.0, ch=23.0)
    validate_table(make_table([tuple(row.values())]), 3 * 23 * 37)
    row.update(bad)
    with pytest.raises(ValueError, match=what):
        validate_table(make_table([tuple(row.values())]), 3 * 23 * 37)


SIZES = [(1, 1), (3, 200), (200, 3), (375, 500), (500, 375), (64, 64),
         (37, 23)]


def test_draw_train_window_2000_draws():
    gen = torch.Generator().manual_seed(7)
    ls, lr, ur = 0.08, 3.0 / 4.0, 4.0 / 3.0
    flips = 0
    for n in range(2000):
        H, W = SIZES[n % len(SIZES)]
        x0, y0, cw, ch, flip = draw_train_window(H, W, gen, ls, lr, ur)
        assert all(isinstance(v, int) for v in (x0, y0, cw, ch, flip))
        assert cw >= 1 and ch >= 1 and x0 >= 0 and y0 >= 0
        assert x0 + cw <= W and y0 + ch <= H
        flips += flip
        # the fit bound is (W/H)/aspect^2 or its inverse; it stays above
        # lower_scale for every aspect when min(W/H, H/W) * lower_ratio does
        if min(W / H, H / W) * lr >= ls and min(H, W) > 1:
            # w, h were truncated: the real extents lie in [cw, cw+1) x
            # [ch, ch+1)
            assert cw * ch <= H * W
            assert (cw + 1) * (ch + 1) >= ls * H * W
            assert cw / (ch + 1) <= ur and (cw + 1) / ch >= lr
    assert 800 < flips < 1200


def test_draw_train_window_is_seeded():
    a = [draw_train_window(375, 500, torch.Generator().manual_seed(3))
         for _ in range(2)]
    b = draw_train_window(375, 500, torch.Generator().manual_seed(4))
    assert a[0] == a[1] and a[0] != b


@pytest.mark.parametrize("H, W", [(375, 500), (500, 375), (64, 64), (1, 1)])
def test_eval_window(H, W):
    x0, y0, cw, ch, flip = eval_window(H, W, crop=224, resize_short=256)
    assert flip == 0 and cw == ch == 224.0 / 256.0 * min(H, W)
    assert x0 + cw / 2 == pytest.approx(W / 2)
    assert y0 + ch / 2 == pytest.approx(H / 2)
    assert x0 >= 0 and y0 >= 0 and x0 + cw <= W and y0 + ch <= H
    side = eval_window(H, W, crop=32, resize_short=40)[2]
    assert side == 0.8 * min(H, W)


# ---- the loader -------------------------------------------------------------

CPU = torch.device("cpu")


def drain(loader, n):
    xs, ys = zip(*(loader.next() for _ in range(n)))
    loader.close()
    return torch.cat(xs), torch.cat(ys)


@pytest.fixture(scope="module")
def pngs(tmp_path_factory):
    root = tmp_path_factory.mktemp("pngs")
    return root, write_pngs(root)


def test_loader_shapes_and_labels(pngs):
    root, records = pngs
    ld = ImageRecordLoader(records, str(root), 4, CPU, out_size=20, seed=1)
    assert ld.steps() == 2
    x, y = ld.next()
    assert x.shape == (4, 3, 20, 20) and x.dtype == torch.float32
    assert x.is_contiguous(memory_format=torch.channels_last)
    assert y.dtype == torch.long and y.tolist() == [0, 7, 4, 1]
    x2, y2 = ld.next()
    assert y2.tolist() == [8, 5, 2, 9]
    assert torch.isfinite(x).all() and not torch.equal(x, x2)
    # the stream cycles: batch 3 starts at record 8 and wraps to record 0
    assert ld.next()[1].tolist() == [6, 3, 0, 7]
    ld.close()


def test_loader_eval_matches_formula_on_the_full_files(pngs):
    """Packing only the window's rectangle moves no tap: the eval batch
    equals the float64 formula applied to the WHOLE decoded files."""
    from PIL import Image

    root, records = pngs
    S = 20
    ld = ImageRecordLoader(records, str(root), 10, CPU, out_size=S,
                           train=False)
    x, _ = ld.next()
    ld.close()
    chunks, rows, off = [], [], 0
    for rec in records:
        img = np.asarray(Image.open(str(root / rec.split()[0])).convert("RGB"))
        H, W = img.shape[:2]
        x0, y0, cw, ch, flip = eval_window(H, W, S, S * 256.0 / 224.0)
        rows.append((off, H, W, flip, x0, y0, cw, ch))
        chunks.append(img.reshape(-1))
        off += img.size
    ref = oracle_f64(np.concatenate(chunks), rows, S)
    # + the window's fp32 rounding before and after the rebase (2^-24 * 80
    # px = 5e-6 px, times a slope of at most 255/px, normalised)
    assert np.abs(to_np64(x) - ref).max() <= TOL_F32 + 5e-6 / 0.224


def test_loader_record_pixels_do_not_depend_on_sharding(pngs):
    root, records = pngs
    kw = dict(out_size=20, seed=5, epoch=2)
    whole, yw = drain(ImageRecordLoader(records, str(root), 5, CPU, **kw), 2)
    for r in (0, 1):
        part, yp = drain(
            ImageRecordLoader(records[r::2], str(root), 5, CPU, **kw), 1)
        assert torch.equal(part, whole[r::2]) and torch.equal(yp, yw[r::2])


def test_loader_epoch_and_seed(pngs):
    root, records = pngs

    def batch(train, seed, epoch):
        return drain(ImageRecordLoader(records, str(root), 10, CPU,
                                       out_size=20, train=train, seed=seed,
                                       epoch=epoch), 1)[0]

    assert torch.equal(batch(True, 1, 0), batch(True, 1, 0))
    assert not torch.equal(batch(True, 1, 0), batch(True, 1, 1))
    assert not torch.equal(batch(True, 1, 0), batch(True, 2, 0))
    assert torch.equal(batch(False, 1, 0), batch(False, 2, 3))


def test_loader_unreadable_file_names_the_record(pngs, tmp_path):
    root, records = pngs
    (tmp_path / "broken.png").write_bytes(b"not a png at all")
    (tmp_path / "img0.png").write_bytes((root / "img0.png").read_bytes())
    recs = ["img0.png 1", "broken.png 3", "missing.png 4"]
    with pytest.raises(RuntimeError, match=r"broken\.png 3"):
        ImageRecordLoader(recs[:2], str(tmp_path), 2, CPU, out_size=8).next()
    with pytest.raises(RuntimeError, match=r"missing\.png 4"):
        ImageRecordLoader(recs[::2], str(tmp_path), 2, CPU, out_size=8).next()


def test_loader_under_mixup(pngs):
    root, records = pngs
    ld = ImageRecordLoader(records, str(root), 4, CPU, out_size=20)
    x, ya, yb, lam = MixupLoader(ld, 0.2, seed=0).next()
    ld.close()
    assert x.shape == (4, 3, 20, 20) and lam.shape == (4,)
    assert x.is_contiguous(memory_format=torch.channels_last)
    assert ya.tolist() == [0, 7, 4, 1] and sorted(yb.tolist()) == [0, 1, 4, 7]


def test_trainer_end_to_end_from_image_files(pngs, tmp_path):
    """train_resnet from --train_list / --image_root / --val_list on the
    CPU: one epoch of 2 steps plus an eval pass."""
    import os
    import subprocess
    import sys

    root, records = pngs
    (tmp_path / "train_list.txt").write_text("\n".join(records) + "\n")
    (tmp_path / "val_list.txt").write_text("\n".join(records[:4]) + "\n")
    argv = [
        "--model", "resnet18_vd", "--batch_size", "4", "--num_epochs", "1",
        "--steps_per_epoch", "2", "--image_hw", "32", "--use_hip_ops", "0",
        "--dtype", "fp32", "--eval_steps", "1",
        "--train_list", str(tmp_path / "train_list.txt"),
        "--val_list", str(tmp_path / "val_list.txt"),
        "--image_root", str(root), "--decode_workers", "2",
        "--checkpoint", str(tmp_path / "ck"),
    ]
    # a process of its own, with no GPU in sight: main() picks the device
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; from edl_amd.train import train_resnet; "
            "sys.exit(train_resnet.main(sys.argv[1:]))")
    out = subprocess.run(
        [sys.executable, "-c", code] + argv, cwd=repo, capture_output=True,
        text=True, timeout=240,
        env=dict(os.environ, CUDA_VISIBLE_DEVICES="", PYTHONPATH=repo))
    assert out.returncode == 0, out.stdout + out.stderr
    log = out.stdout + out.stderr
    assert "epoch 0 done" in log and "epoch 0 eval" in log
    assert (tmp_path / "ck" / "checkpoint.0").is_dir()


def test_data_plane_records_decode_from_image_root(coord_server, pngs,
                                                   tmp_path):
    """--data_dir + --image_root at world 2 under the launcher: the elastic
    data plane delivers the `relpath label` lines, ImageRecordLoader turns
    them into pixels."""
    import re

    from test_train_scripts import run_edlrun

    root, records = pngs
    data = tmp_path / "data"
    data.mkdir()
    for i in range(2):
        (data / ("part%d.txt" % i)).write_text(
            "\n".join(records[i::2] * 2) + "\n")
    run_edlrun(
        coord_server, tmp_path,
        ["-m", "edl_amd.train.train_resnet", "--model", "resnet18_vd",
         "--num_epochs", "1", "--batch_size", "2", "--image_hw", "32",
         "--steps_per_epoch", "2", "--data_dir", str(data),
         "--image_root", str(root), "--decode_workers", "2",
         "--use_hip_ops", "0", "--dtype", "fp32",
         "--checkpoint", str(tmp_path / "ck")],
        timeout=240,
    )
    assert (tmp_path / "ck" / "checkpoint.0").is_dir()
    logs = "".join((tmp_path / ("agent%d.log" % i)).read_text()
                   for i in (0, 1))
    counts = [int(m) for m in re.findall(r"rank \d+: (\d+) records", logs)]
    assert len(counts) == 2 and sum(counts) == 20, counts
    assert "epoch 0 done" in logs
