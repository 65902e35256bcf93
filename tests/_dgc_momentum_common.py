"""Inputs and an independent (sort-based) statement of the DGC selection
rule, shared by test_dgc_momentum_cpu.py, test_dgc_momentum_gpu.py and
their workers."""
import torch

MU, WD = 0.5, 0.25


def exact_inputs(n, seed=0):
    """g, u, v, p on which u = mu*u + (g + wd*p), v += u is EXACT in fp32
    for mu=0.5, wd=0.25: integers/16 (u: /8), so every product and partial
    sum is a multiple of 1/64 far below 2^24/64 and FMA contraction cannot
    move a value. Many ties in |v|. Draw order: g, u, v, p."""
    gen = torch.Generator().manual_seed(seed)

    def draw(div):
        return torch.randint(-1024, 1025, (n,), generator=gen).float() / div

    g = draw(16)
    u = draw(8)
    v = draw(16)
    p = draw(16)
    return g, u, v, p


def abs_bits_ref(v):
    return (v.contiguous().view(torch.int32) & 0x7FFFFFFF).to(torch.int64)


def ref_select(v, k):
    """The rule, by a full sort: -> sorted int64 indices of the selected."""
    a = abs_bits_ref(v)
    P = torch.sort(a, descending=True).values[k - 1]
    ge = a >= P
    mask = ge if int(ge.sum()) <= k else a > P
    mask = mask & (a > 0)
    return mask.nonzero().view(-1)


def sort_payload(payload):
    """Slot order is unspecified: sort by index (stable, so the -1 slots,
    whose bits are all 0, compare equal too)."""
    order = torch.sort(payload[0], stable=True).indices
    return payload[:, order]


def payload_indices(payload):
    idx = payload[0]
    return torch.sort(idx[idx >= 0].to(torch.int64)).values
