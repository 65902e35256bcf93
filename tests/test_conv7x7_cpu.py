"""The host side of the 7x7 stem route, without a GPU: the weight repack
against its definition, the predicate that picks the route, and the model's
state-dict layout."""
import pytest
import torch

from edl_amd.ops.conv import Conv2dFast, _repack_w7


@pytest.mark.parametrize("cin", [1, 3, 4])
def test_repack_w7_is_its_definition(cin):
    g = torch.Generator().manual_seed(cin)
    w = torch.randn(64, cin, 7, 7, generator=g)
    w7 = _repack_w7(w)
    assert w7.dtype == torch.bfloat16 and w7.shape == (64, 224)
    assert w7.is_contiguous()
    v = w7.view(64, 7, 8, 4)
    wb = w.to(torch.bfloat16)
    for ky in range(7):
        for kx in range(7):
            for c in range(cin):
                assert torch.equal(v[:, ky, kx, c], wb[:, c, ky, kx])
    assert bool((v[:, :, 7, :] == 0).all())      # the kx = 7 slot
    assert bool((v[:, :, :, cin:] == 0).all())   # channels >= Cin
    assert int((v != 0).sum()) == 64 * 49 * cin  # randn: nothing else is 0


def test_is_stem7x7():
    def conv(cin=3, cout=64, k=7, **kw):
        kw = {"stride": 2, "padding": 3, "bias": False, **kw}
        return Conv2dFast(cin, cout, k, **kw)

    assert conv()._is_stem7x7()  # the teacher's conv1
    assert conv(cin=1)._is_stem7x7() and conv(cin=4)._is_stem7x7()
    for other in (conv(stride=1), conv(padding=2), conv(bias=True),
                  conv(cout=32), conv(cin=8), conv(cin=4, groups=2),
                  conv(dilation=2), conv(k=3, padding=1)):
        assert not other._is_stem7x7(), other


def test_resnext_state_dict_keys_unchanged():
    from edl_amd.models.resnext_wsl import ResNeXtWSL

    with torch.device("meta"):
        m = ResNeXtWSL((1, 1, 1, 1), groups=4, base_width=16, num_classes=4)
    keys = list(m.state_dict().keys())
    assert keys[:6] == ["conv1.weight", "bn1.weight", "bn1.bias",
                        "bn1.running_mean", "bn1.running_var",
                        "bn1.num_batches_tracked"]
    assert {k.split(".")[0] for k in keys} == {"conv1", "bn1", "stages", "fc"}
    assert tuple(m.conv1.weight.shape) == (64, 3, 7, 7)
