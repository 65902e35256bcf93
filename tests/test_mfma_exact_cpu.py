"""CPU self-test of the integer-exact helper (tests/_mfma_exact_common.py):
its fp64 references agree with torch's own, and check_exact can fail."""
import pytest
import torch
import torch.nn.functional as F

import _mfma_exact_common as X


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("groups", [1, 2])
def test_conv_reference_equals_conv2d_fp64(stride, groups):
    gen = torch.Generator().manual_seed(7)
    x = X.ints((2, 8, 7, 9), X.PM12, gen)        # odd H and W
    w = X.ints((6, 8 // groups, 3, 3), X.ASYM3, gen)
    ref = X.exact_ref_conv(x, w, stride, groups)
    want = F.conv2d(x.double(), w.double(), stride=stride, padding=1,
                    groups=groups)
    assert ref.dtype == torch.float64 and torch.equal(ref, want)
    X.check_budget(ref, 9 * 8 // groups, x, w, bf16_out=True)
    # the kernels' row layout: row (n, oy, ox), column channel
    r = X.rows(ref)
    ho, wo = want.shape[2:]
    assert torch.equal(r[1 * ho * wo + 2 * wo + 1], want[1, :, 2, 1])


def test_check_exact_rejects_one_element_off_by_one():
    gen = torch.Generator().manual_seed(8)
    a = X.ints((37, 64), X.PM12, gen)
    b = X.ints((16, 64), X.ASYM3, gen)
    ref = X.exact_ref_bt(a, b)
    X.check_budget(ref, 64, a, b, bf16_out=True)
    for dtype in (torch.float32, torch.bfloat16):
        good = ref.to(dtype)
        X.check_exact(good, ref, "good")
        bad = good.clone()
        bad[36, 5] += 1
        with pytest.raises(AssertionError, match=r"1 of 592 .*\(36, 5\)"):
            X.check_exact(bad, ref, "bad")
    assert torch.equal(X.exact_ref_tn(a.t(), b.t()), ref)


def test_budget_conditions_can_fail():
    gen = torch.Generator().manual_seed(9)
    # K * 3 * 3 >= 2^24: the accumulation budget
    a = X.ints((2, 64), X.ASYM3, gen)
    with pytest.raises(AssertionError, match="budget"):
        X.check_budget(X.exact_ref_bt(a, a), 1 << 21, a, a, bf16_out=False)
    # |ref| mostly above 256: the bf16 share
    a = torch.full((4, 512), 2.0).to(torch.bfloat16)
    with pytest.raises(AssertionError, match="share"):
        X.check_budget(X.exact_ref_bt(a, a), 512, a, a, bf16_out=True)
    # per-channel sum y^2 >= 2^24: the stats budget
    with pytest.raises(AssertionError, match="budget"):
        X.ref_stats(torch.full((5000, 2), 64.0, dtype=torch.float64))
