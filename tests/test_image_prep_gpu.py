"""The image input stage on the GPU: csrc/image_prep.hip against the float64
statement of the contract (never against the code under test), and
ImageRecordLoader on the device."""
import numpy as np
import pytest
import torch

from _image_prep_common import (MEAN, STD, TOL_F32, edge_batch, oracle_f64,
                                to_np64, tol_bf16, write_pngs)

pytestmark = pytest.mark.gpu

SIZES = (1, 7, 20, 32)


def op(*a, **k):
    from edl_amd.ops.image_prep import crop_resize_normalize

    return crop_resize_normalize(*a, **k)


@pytest.fixture(scope="module")
def edge():
    """One batch with every edge case, its host table, and the float64
    oracle per output size: computed once, never changed."""
    from edl_amd.ops.image_prep import make_table

    packed, rows = edge_batch()
    refs = {S: oracle_f64(packed, rows, S) for S in SIZES}
    return torch.from_numpy(packed).cuda(), make_table(rows), refs


@pytest.mark.parametrize("S", SIZES)
def test_fp32_matches_float64_formula(edge, S):
    packed, table, refs = edge
    out = op(packed, table, S, MEAN, STD, torch.float32)
    assert out.shape == (table.shape[0], 3, S, S)
    assert out.dtype == torch.float32 and out.is_cuda
    assert out.permute(0, 2, 3, 1).is_contiguous()
    err = np.abs(to_np64(out) - refs[S])
    print("S=%d fp32 max err %.3g" % (S, err.max()))
    assert err.max() <= TOL_F32


@pytest.mark.parametrize("S", SIZES)
def test_bf16_matches_float64_formula(edge, S):
    packed, table, refs = edge
    out = op(packed, table, S, MEAN, STD, torch.bfloat16)
    assert out.dtype == torch.bfloat16
    assert out.permute(0, 2, 3, 1).is_contiguous()
    err = np.abs(to_np64(out) - refs[S])
    print("S=%d bf16 max err/tol %.3g" % (S, (err / tol_bf16(refs[S])).max()))
    assert (err <= tol_bf16(refs[S])).all()


@pytest.mark.parametrize("S", SIZES)
def test_bf16_is_the_rounded_fp32(edge, S):
    packed, table, _ = edge
    f = op(packed, table, S, MEAN, STD, torch.float32)
    h = op(packed, table, S, MEAN, STD, torch.bfloat16)
    assert torch.equal(h, f.to(torch.bfloat16))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("S, lead", [(7, 5), (20, 8), (32, 3)])
def test_guard_bytes_stay_untouched(edge, S, lead, dtype):
    """The output as a view inside a sentinel-filled allocation, at element
    offsets that break and that keep the vector stores' alignment."""
    packed, table, _ = edge
    B = table.shape[0]
    n = B * S * S * 3
    tail = 64
    ref = op(packed, table, S, MEAN, STD, dtype)
    raw = torch.full((lead + n + tail,), -77.0, dtype=dtype, device="cuda")
    view = raw[lead:lead + n].view(B, S, S, 3).permute(0, 3, 1, 2)
    got = op(packed, table, S, MEAN, STD, dtype, out=view)
    assert got.data_ptr() == view.data_ptr()
    assert torch.equal(view, ref)
    assert (raw[:lead] == -77.0).all() and (raw[lead + n:] == -77.0).all()


def test_side_stream_gives_the_same_bits(edge):
    packed, table, _ = edge
    want = op(packed, table, 20, MEAN, STD, torch.bfloat16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = op(packed, table, 20, MEAN, STD, torch.bfloat16)
    torch.cuda.current_stream().wait_stream(side)
    got.record_stream(torch.cuda.current_stream())
    assert torch.equal(got, want)


def test_bad_tables_are_rejected_before_any_launch(edge):
    """Asserted as exceptions only: a bad table is never launched."""
    from edl_amd.ops import ext
    from edl_amd.ops.image_prep import make_table

    packed, table, _ = edge
    n = packed.numel()
    good = (0, 23, 37, 0, 0.0, 0.0, 37.0, 23.0)

    def bad(**kw):
        row = dict(zip(("off", "H", "W", "flip", "x0", "y0", "cw", "ch"),
                       good))
        row.update(kw)
        return make_table([tuple(row.values())])

    for t, what in ((bad(off=n - 10), "offset"), (bad(H=0), "H, W"),
                    (bad(x0=30.0, cw=10.0), "window"),
                    (bad(y0=-1.0), "window")):
        with pytest.raises(ValueError, match=what):
            op(packed, t, 8, MEAN, STD, torch.float32)
    with pytest.raises(ValueError, match="CPU packed"):
        op(packed.cpu(), table.cuda(), 8, MEAN, STD, torch.float32)
    # the binding's own checks, under the Python wrapper
    C = ext()
    dev_table = table.cuda()
    args = (8, list(MEAN), list(STD), False)
    with pytest.raises(RuntimeError, match="one GPU"):
        C.crop_resize_normalize(packed.cpu(), dev_table, *args)
    with pytest.raises(RuntimeError, match="uint8"):
        C.crop_resize_normalize(packed.float(), dev_table, *args)
    with pytest.raises(RuntimeError, match="int32"):
        C.crop_resize_normalize(packed, dev_table[:, :4].contiguous(), *args)
    with pytest.raises(RuntimeError, match="B >= 1"):
        C.crop_resize_normalize(packed, dev_table[:0], *args)
    with pytest.raises(RuntimeError, match="out_size"):
        C.crop_resize_normalize(packed, dev_table, 0, list(MEAN), list(STD),
                                False)
    with pytest.raises(RuntimeError, match="channels-last"):
        C.crop_resize_normalize(
            packed, dev_table, *args,
            out=torch.empty(dev_table.shape[0], 3, 8, 8, device="cuda"))


# ---- the loader on the device -----------------------------------------------

@pytest.fixture(scope="module")
def pngs(tmp_path_factory):
    root = tmp_path_factory.mktemp("pngs")
    return root, write_pngs(root)


def test_loader_on_the_gpu_matches_the_cpu_loader(pngs):
    """Channels-last bf16 batches within the bf16 bound of the CPU loader's
    fp32 output for the same seed; three consecutive next() calls (the
    prefetch ring wraps at depth 2) return distinct, correct batches."""
    from edl_amd.data.images import ImageRecordLoader

    root, records = pngs
    kw = dict(out_size=20, seed=3, epoch=1, num_workers=4)
    cpu = ImageRecordLoader(records, str(root), 4, torch.device("cpu"),
                            out_dtype=torch.float32, **kw)
    gpu = ImageRecordLoader(records, str(root), 4, torch.device("cuda"), **kw)
    assert gpu.steps() == 2
    seen = []
    for _ in range(3):
        xc, yc = cpu.next()
        xg, yg = gpu.next()
        assert xg.is_cuda and xg.dtype == torch.bfloat16
        assert xg.shape == (4, 3, 20, 20)
        assert xg.permute(0, 2, 3, 1).is_contiguous()
        assert yg.is_cuda and torch.equal(yg.cpu(), yc)
        ref = to_np64(xc)
        assert (np.abs(to_np64(xg) - ref) <= tol_bf16(ref)).all()
        seen.append(xg.float().cpu())
    cpu.close()
    gpu.close()
    assert not torch.equal(seen[0], seen[1])
    assert not torch.equal(seen[1], seen[2])
    assert not torch.equal(seen[0], seen[2])
