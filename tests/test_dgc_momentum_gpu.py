"""DGC momentum correction on the GPU: the HIP compress / decode kernels
(csrc/dgc.hip) against the torch path (edl_amd/ops/dgc.py, run on the
CPU), and DGCMomentum at world 2 on one GPU."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from _dgc_momentum_common import (MU, WD, exact_inputs, payload_indices,
                                  sort_payload)
from edl_amd.ops.dgc import dgc_compress, dgc_decode

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 3, 257, 1021, 70_001, 2_100_003]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ks(n):
    return sorted({1, n // 1000 or 1, n // 100 or 1, n})


_REF = {}


def _reference(n, k, with_p=True):
    """Torch path on the CPU, computed once per case and never modified."""
    key = (n, k, with_p)
    if key not in _REF:
        g, u, v, p = exact_inputs(n)
        pl = dgc_compress(g, u, v, p if with_p else None, MU, WD, k)
        _REF[key] = (u, v, sort_payload(pl))
    return _REF[key]


def _offset_by_one(t):
    """A CUDA copy of t that starts 4 bytes past a 16-B boundary."""
    buf = torch.empty(t.numel() + 5, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + t.numel()]
    out.copy_(t)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_compress_bit_exact(n):
    for k in _ks(n):
        g, u, v, p = (t.cuda() for t in exact_inputs(n))
        pl = dgc_compress(g, u, v, p, MU, WD, k)
        ru, rv, rpl = _reference(n, k)
        assert pl.shape == (2, k) and pl.dtype == torch.int32
        assert torch.equal(u.cpu(), ru), (n, k)
        assert torch.equal(v.cpu(), rv), (n, k)
        assert torch.equal(sort_payload(pl.cpu()), rpl), (n, k)


@pytest.mark.parametrize("with_p", [True, False])
def test_compress_bit_exact_unaligned(with_p):
    """g, u, v one element past a 16-B boundary: the scalar path."""
    n, k = 70_001, 683  # a tie crosses the boundary at this k
    g, u, v, p = exact_inputs(n)
    g, u, v = _offset_by_one(g), _offset_by_one(u), _offset_by_one(v)
    assert g.data_ptr() % 16 == 4 and v.data_ptr() % 16 == 4
    pl = dgc_compress(g, u, v, p.cuda() if with_p else None, MU, WD, k)
    ru, rv, rpl = _reference(n, k, with_p)
    assert torch.equal(u.cpu(), ru) and torch.equal(v.cpu(), rv)
    assert torch.equal(sort_payload(pl.cpu()), rpl)
    if with_p:
        assert payload_indices(pl.cpu()).numel() == 682


def test_workspace_is_left_clean():
    """Back-to-back calls with different n and k share one workspace."""
    for n, k in ((70_001, 700), (1021, 1021), (70_001, 1), (257, 2)):
        g, u, v, p = (t.cuda() for t in exact_inputs(n))
        pl = dgc_compress(g, u, v, p, MU, WD, k)
        ru, rv, rpl = _reference(n, k)
        assert torch.equal(v.cpu(), rv) and torch.equal(u.cpu(), ru)
        assert torch.equal(sort_payload(pl.cpu()), rpl)


def test_maximum_contention():
    """All of |v| equal: one histogram bin, one n-way tie."""
    n = 70_001
    for k, nsel in ((70, 0), (n, n)):
        g = torch.full((n,), 1.25, device="cuda")
        g[::2] = -1.25
        want_v = g.clone()
        u = torch.zeros(n, device="cuda")
        v = torch.zeros(n, device="cuda")
        pl = dgc_compress(g, u, v, None, 0.5, 0.0, k).cpu()
        assert int((pl[0] >= 0).sum()) == nsel
        if nsel == 0:
            assert torch.equal(pl[1], torch.zeros(k, dtype=torch.int32))
            assert torch.equal(v, want_v) and torch.equal(u, want_v)
        else:
            assert torch.equal(payload_indices(pl), torch.arange(n))
            assert torch.equal(sort_payload(pl)[1].view(torch.float32),
                               want_v.cpu())
            assert not bool(v.ne(0).any() or u.ne(0).any())


@pytest.mark.parametrize("n,k", [(2_100_003, 2100), (70_001, 70), (1021, 10)])
def test_random_data(n, k):
    """randn data: u, v against fp64 within 4 * 2^-24 * (|mu u| + |g| +
    |wd p| + |v|) (at most three roundings, each relative to a partial sum
    no larger than that total, one unit of margin); selection by property."""
    mu, wd = 0.9, 1e-4
    gen = torch.Generator().manual_seed(0)
    g, u, v, p = (torch.randn(n, generator=gen) for _ in range(4))
    u64 = mu * u.double() + (g.double() + wd * p.double())
    v64 = v.double() + u64
    bound = 4 * 2.0 ** -24 * ((mu * u).abs() + g.abs() + (wd * p).abs()
                              + v.abs()).double()
    gd, ud, vd, pd = (t.cuda() for t in (g, u, v, p))
    pl = dgc_compress(gd, ud, vd, pd, mu, wd, k).cpu()
    ua, va = ud.cpu(), vd.cpu()
    idx = payload_indices(pl)
    assert idx.numel() == k and idx.unique().numel() == k
    sent = torch.zeros(n, dtype=torch.bool)
    sent[idx] = True
    # zero exactly at the payload indices (randn: no exact zeros elsewhere)
    assert torch.equal(va == 0, sent) and torch.equal(ua == 0, sent)
    vals = sort_payload(pl)[1].view(torch.float32)
    u_err = (ua.double() - u64).abs()[~sent]
    v_err = (va.double() - v64).abs()[~sent]
    p_err = (vals.double() - v64[idx]).abs()
    print("n=%d max u_err/bound %.3f v_err/bound %.3f payload_err/bound %.3f"
          % (n, float((u_err / bound[~sent]).max()),
             float((v_err / bound[~sent]).max()),
             float((p_err / bound[idx]).max())))
    assert bool((u_err <= bound[~sent]).all())
    assert bool((v_err <= bound[~sent]).all())
    assert bool((p_err <= bound[idx]).all())
    assert float(vals.abs().min()) >= float(va.abs().max())


def test_non_finite_values_are_sent():
    n = 70_001
    g, u, v, p = (t.cuda() for t in exact_inputs(n))
    g[12_345] = float("inf")
    g[54_321] = float("nan")
    pl = dgc_compress(g, u, v, p, MU, WD, 70).cpu()
    idx = payload_indices(pl).tolist()
    assert 12_345 in idx and 54_321 in idx and len(idx) <= 70
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(u).all())


def test_decode_rank_order():
    """Overlapping indices and -1 slots: bit-equal to sequential
    index_add_ in rank order, and idempotent."""
    n = 1021
    gen = torch.Generator().manual_seed(3)

    def pl(k, scale):
        idx = torch.randperm(n, generator=gen)[:k].to(torch.int32)
        idx[::5] = -1
        vals = torch.randn(k, generator=gen) * scale
        return torch.stack([idx, vals.view(torch.int32)])

    pls = [pl(700, 1e6), pl(700, 1.0), pl(700, 1e-3)]
    want = torch.zeros(n)
    for q in pls:
        keep = q[0] >= 0
        want.index_add_(0, q[0][keep].long(), q[1][keep].view(torch.float32))
    assert torch.equal(dgc_decode(torch.ones(n), pls), want)  # the torch path
    out = torch.full((n,), 3.0, device="cuda")
    dev = [q.cuda() for q in pls]
    dgc_decode(out, dev)
    assert torch.equal(out.cpu(), want)
    dgc_decode(out, dev)
    assert torch.equal(out.cpu(), want)
    # another order is another sum somewhere: the order is what is tested
    rev = dgc_decode(torch.empty(n), pls[::-1])
    assert not torch.equal(rev, want)


def test_two_ranks_one_gpu():
    script = os.path.join(REPO, "tests", "_dgc_momentum_cuda_worker.py")
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29549", script],
        env=env, cwd=REPO, capture_output=True, text=True, timeout=240)
    sys.stderr.write(r.stdout[-2000:] + r.stderr[-1500:])
    assert r.returncode == 0
    oks = [json.loads(m) for m in
           re.findall(r'\{"dgc_momentum_cuda".*?\}', r.stdout)]
    assert len(oks) == 2 and all(v["ok"] for v in oks), oks
    assert all(v["buckets"] == 2 for v in oks)
