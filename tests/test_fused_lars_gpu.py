"""GPU tests of the LARS kernels (csrc/fused_lars.hip) and of FusedLARS on
them: the raw bindings against the plain per-tensor LARS of _lars_common
under its tolerance rule, ragged layouts, launch geometry, buffer bounds,
determinism, the clip state, hipGraph capture and the engine with
optimizer="lars".

Every test here requires an MI355X."""
import json
import os
import subprocess
import sys

import pytest
import torch

import _adam_common as A
import _lars_common as L

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from edl_amd import ops
else:
    ops = None

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 8
SENTINEL = -7.0  # no live slot can hold it: sums of squares and trust >= 0
H = L.HYPER


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    # loud check: the HIP extension must be present on a GPU box
    assert ops.available(), "edl_amd._C missing on a GPU box"


def _tables(buckets):
    """The device tables of the three kernels for `buckets`, a list of
    layouts (tensors numbered across the buckets in order), built here
    independently of FusedLARS."""
    dev, chunk = "cuda", ops.ext().LARS_CHUNK
    chunks, boff, tchunks, segs, t = [], [0], [], [], 0
    for bi, layout in enumerate(buckets):
        seg = []
        for s, e, ex in L.spans(layout):
            if ex and seg and seg[-1][1] == 0.0:
                seg[-1][0] = e  # adjacent excluded tensors coalesce
            else:
                seg.append([e, 0.0 if ex else H["lars_weight_decay"], t])
            first = len(chunks)
            if not ex:
                for c in range(s, e, chunk):
                    chunks.append([bi, c, min(chunk, e - c), 0])
            tchunks.append([first, len(chunks) - first])
            t += 1
        boff.append(len(chunks))
        segs.append(tuple(
            torch.tensor([x[k] for x in seg], dtype=dt, device=dev)
            for k, dt in ((0, torch.int32), (1, torch.float32),
                          (2, torch.int32))))
    return {
        "chunks": torch.tensor(chunks, dtype=torch.int32,
                               device=dev).view(-1, 4),
        "boff": boff, "nchunks": len(chunks), "nt": t, "segs": segs,
        "tchunks": torch.tensor(tchunks, dtype=torch.int32,
                                device=dev).view(-1, 2),
    }


def _raw_run(buckets, p0, grads, clip=None, grad_scale=L.GRAD_SCALE):
    """One launch sequence per gradient on guard-padded, sentinel-filled
    buffers. -> (per-step (p, v, trust) on CPU, the raw buffers)."""
    dev, ext = "cuda", ops.ext()
    tb = _tables(buckets)
    sizes = [sum(ln for ln, _ in b) for b in buckets]
    alloc = [(n + GUARD + 3) // 4 * 4 + 4 for n in sizes]
    raw = {k: [torch.full((a,), s, device=dev) for a in alloc]
           for k, s in (("p", 7.0), ("g", 5.0), ("v", 3.0))}
    ps, gs, vs = ([b[:n] for b, n in zip(raw[k], sizes)] for k in "pgv")
    off = 0
    for p, v, n in zip(ps, vs, sizes):
        p.copy_(p0[off:off + n].float())
        v.zero_()
        off += n
    raw["partial"] = torch.full((2 * tb["nchunks"] + GUARD,), SENTINEL,
                                dtype=torch.float64, device=dev)
    raw["trust"] = torch.full((tb["nt"] + GUARD,), SENTINEL, device=dev)
    lr_dev = torch.full((1,), H["lr"], device=dev)
    if clip is not None:
        clip = torch.tensor(clip, dtype=torch.float32, device=dev)
    out = []
    for gt in grads:
        off = 0
        for g, n in zip(gs, sizes):
            g.copy_(gt[off:off + n].float())
            off += n
        n_done = ext.lars_sumsq(ps, gs, tb["chunks"], tb["boff"],
                                raw["partial"])
        assert n_done == tb["nchunks"]
        ext.lars_trust(raw["partial"], tb["nchunks"], tb["tchunks"],
                       raw["trust"], H["lars_coeff"], H["lars_weight_decay"],
                       H["epsilon"], grad_scale, clip)
        for p, g, v, (s_end, s_wd, s_t) in zip(ps, gs, vs, tb["segs"]):
            # host lr deliberately wrong: the device scalar must win
            ext.fused_lars(p, g, v, 123.0, H["momentum"], grad_scale, s_end,
                           s_wd, s_t, raw["trust"], lr_dev, clip)
        out.append((torch.cat(ps).cpu(), torch.cat(vs).cpu(),
                    raw["trust"][:tb["nt"]].cpu()))
    torch.cuda.synchronize()
    raw["sizes"], raw["nchunks"], raw["nt"] = sizes, tb["nchunks"], tb["nt"]
    return out, raw


def _case(buckets, offset=0, steps=L.STEPS):
    flat = [t for b in buckets for t in b]
    return L.case_reference(flat, offset, steps)


def _single_sizes():
    return [1, 3, 4, 5, 1027, "chunk+1", A.N_REF, "preload+1"]


@pytest.mark.parametrize("n", _single_sizes())
def test_single_tensor_matches_truth(n):
    """One non-excluded tensor; each n is held to K times torch-fp32's own
    error on the same n elements. chunk+1: a second chunk of one element.
    N_REF: 129 chunks, three 64-chunk rounds of the trust kernel.
    preload+1: one chunk more than its wave loads per pass (4.2M elements,
    the smallest tensor that takes a second pass)."""
    if n == "chunk+1":
        n = ops.ext().LARS_CHUNK + 1
    elif n == "preload+1":
        n = ops.ext().LARS_CHUNK * ops.ext().LARS_TRUST_PRELOAD + 1
    buckets = [[(n, False)]]
    p0, grads, truth, ref = _case(buckets)
    got, raw = _raw_run(buckets, p0, grads)
    assert raw["nchunks"] == -(-n // ops.ext().LARS_CHUNK)
    L.check(L.run_errors(got, truth), ref, "gpu single n=%d" % n)


@pytest.mark.parametrize("offset,excluded", [(0, None), (55, {2, 3, 7, 8})])
def test_ragged_bucket_matches_truth(offset, excluded):
    """Tensor starts at all four offsets mod 4, tensors shorter than a
    float4, a float4 over three tensors. offset 0: every 4th excluded, zero
    params in the first tensors (pn == 0). offset 55: adjacent excluded
    tensors, and the first tensor is one element with a zero gradient
    (gn == 0)."""
    buckets = [L.ragged_layout(excluded)]
    p0, grads, truth, ref = _case(buckets, offset)
    got, _ = _raw_run(buckets, p0, grads)
    tr = got[0][2]
    print("trust:", tr.tolist())
    assert float(tr[0]) == 1.0 and float(tr[3]) == 1.0
    assert float(tr[4]) != 1.0 and float(tr[9]) != 1.0
    L.check(L.run_errors(got, truth), ref,
            "gpu ragged offset=%d" % offset)


def _many_buckets(nb):
    return [[(3 + b, False), (2, b % 2 == 0), (1 + b % 5, False)]
            for b in range(nb)]


def test_two_buckets_in_one_launch():
    buckets = [L.ragged_layout(), [(1027, False), (5, True), (3, False)]]
    p0, grads, truth, ref = _case(buckets)
    got, _ = _raw_run(buckets, p0, grads)
    L.check(L.run_errors(got, truth), ref, "gpu two buckets")


def test_more_buckets_than_one_launch_takes():
    nb = 2 * ops.ext().LARS_MAX_BUFS + 1
    buckets = _many_buckets(nb)
    p0, grads, truth, ref = _case(buckets, offset=40)
    got, _ = _raw_run(buckets, p0, grads)
    L.check(L.run_errors(got, truth), ref, "gpu %d buckets" % nb)


def test_every_live_slot_written_no_guard_touched():
    nb = ops.ext().LARS_MAX_BUFS + 1
    buckets = [L.ragged_layout()] + _many_buckets(nb)
    p0, grads, _, _ = _case(buckets)
    got, raw = _raw_run(buckets, p0, grads[:1])
    live, tail = (raw["partial"][:2 * raw["nchunks"]].cpu(),
                  raw["partial"][2 * raw["nchunks"]:].cpu())
    assert live.numel() and bool((live >= 0).all())
    assert tail.numel() == GUARD and bool((tail == SENTINEL).all())
    live, tail = raw["trust"][:raw["nt"]].cpu(), raw["trust"][raw["nt"]:].cpu()
    assert bool((live > 0).all())
    assert tail.numel() == GUARD and bool((tail == SENTINEL).all())
    for k, sentinel in (("p", 7.0), ("g", 5.0), ("v", 3.0)):
        for b, n in zip(raw[k], raw["sizes"]):
            t = b[n:].cpu()
            assert t.numel() >= GUARD
            assert torch.equal(t, torch.full_like(t, sentinel))
    assert bool(got[-1][1].ne(0).any())  # the live part really updated


def test_two_runs_are_bitwise_equal():
    buckets = [L.ragged_layout(), [(ops.ext().LARS_CHUNK * 3 + 5, False)]]
    p0, grads, _, _ = _case(buckets)
    a, _ = _raw_run(buckets, p0, grads[:3])
    b, _ = _raw_run(buckets, p0, grads[:3])
    for x, y in zip(a[-1], b[-1]):
        assert torch.equal(x, y)


def test_skip_leaves_p_and_v_untouched_with_nan_gradients():
    buckets = [L.ragged_layout()]
    p0, grads, _, _ = _case(buckets)
    bad = grads[0].clone()
    bad[5] = float("nan")
    bad[2000] = float("inf")
    got, _ = _raw_run(buckets, p0, [bad], clip=[0.0, float("nan"), 1.0, 1.0])
    assert torch.equal(got[0][0], p0.float())
    assert torch.equal(got[0][1], torch.zeros_like(got[0][1]))


def test_coef_one_is_bitwise_the_null_clip_path():
    buckets = [L.ragged_layout()]
    p0, grads, _, _ = _case(buckets)
    a, _ = _raw_run(buckets, p0, grads[:2], clip=[1.0, 3.0, 0.0, 0.0])
    b, _ = _raw_run(buckets, p0, grads[:2])
    for x, y in zip(a[-1], b[-1]):
        assert torch.equal(x, y)
    # and a coefficient scales the gradient, in its norm too: 0.5 on
    # grad_scale 0.25 is bitwise grad_scale 0.125 (exact powers of two)
    c, _ = _raw_run(buckets, p0, grads[:2], clip=[0.5, 3.0, 0.0, 0.0],
                    grad_scale=0.25)
    for x, y in zip(b[-1], c[-1]):
        assert torch.equal(x, y)


def test_bindings_reject_bad_arguments():
    ext, dev = ops.ext(), "cuda"
    p, g, v = (torch.zeros(16, device=dev) for _ in range(3))
    part = torch.zeros(8, dtype=torch.float64, device=dev)
    trust = torch.ones(2, device=dev)

    def i32(x, cols=None):
        t = torch.tensor(x, dtype=torch.int32, device=dev)
        return t if cols is None else t.view(-1, cols)

    ok = i32([[0, 0, 16, 0]], 4)
    with pytest.raises(RuntimeError, match="16-byte"):
        ext.lars_sumsq([torch.zeros(17, device=dev)[1:]], [g], ok, [0, 1], part)
    with pytest.raises(RuntimeError, match="must agree"):
        ext.lars_sumsq([p], [g[:8]], ok, [0, 1], part)
    with pytest.raises(RuntimeError, match="leaves its bucket"):
        ext.lars_sumsq([p], [g], i32([[0, 8, 16, 0]], 4), [0, 1], part)
    with pytest.raises(RuntimeError, match="outside its bucket"):
        ext.lars_sumsq([p], [g], i32([[1, 0, 16, 0]], 4), [0, 1], part)
    with pytest.raises(RuntimeError, match="2 slots per chunk"):
        ext.lars_sumsq([p], [g], ok, [0, 1], part[:1])
    with pytest.raises(RuntimeError, match="owns chunks"):
        ext.lars_trust(part, 1, i32([[0, 2], [0, 0]], 2), trust, 0.02, 5e-4,
                       0.0, 1.0)
    seg = (i32([4, 16]), torch.zeros(2, device=dev), i32([0, 1]))
    with pytest.raises(RuntimeError, match="last seg_end"):
        ext.fused_lars(p, g, v, 0.1, 0.9, 1.0, i32([4, 12]), seg[1], seg[2],
                       trust)
    with pytest.raises(RuntimeError, match="no slot of trust"):
        ext.fused_lars(p, g, v, 0.1, 0.9, 1.0, seg[0], seg[1], i32([0, 2]),
                       trust)
    with pytest.raises(RuntimeError, match="segments <= 1024"):
        ext.fused_lars(p, g, v, 0.1, 0.9, 1.0, i32(list(range(1, 1026))),
                       torch.zeros(1025, device=dev), i32([0] * 1025), trust)
    torch.cuda.synchronize()
    assert not bool(p.ne(0).any()) and not bool(part.ne(0).any())


def test_too_many_segments_raise_at_materialize_time():
    layout = [(1, False)] * (ops.ext().ADAM_MAX_SEGMENTS + 1)
    p0 = torch.ones(len(layout), dtype=torch.float64)
    params = L.make_params(layout, p0, "cuda")
    _, opt = L.make_opt(params, layout)
    with pytest.raises(RuntimeError, match="segments"):
        opt._materialize()
    torch.cuda.synchronize()
    assert all(float(p.detach()) == 1.0 for p in params[:3] + params[-3:])


def test_fused_lars_over_a_reducer_matches_truth():
    """FusedLARS builds its own tables over several small buckets (filled
    in reverse parameter order); trust_ratios() is in the order given."""
    layout = L.ragged_layout()
    p0, grads, truth, ref = L.case_reference(layout)
    params = L.make_params(layout, p0, "cuda")
    r, opt = L.make_opt(params, layout, cap_mb=0.004)
    assert len(r._buckets) > 2
    got = L.run_opt(params, layout, opt, grads)
    L.check(L.run_errors(got, truth), ref, "gpu FusedLARS 3+ buckets")
    assert opt.trust_ratios().is_cuda


def _run_child(name, timeout):
    """Run a GPU script in a FRESH process with its own time limit (capture
    after unrelated GPU activity in the same process can crash the runtime,
    and a crash must not take the suite down). The exit status is checked
    before anything is read. -> the child's RESULT dict."""
    env = dict(os.environ)
    env["EDL_REPO"] = REPO
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "tests", name)],
        capture_output=True, text=True, timeout=timeout, cwd=REPO, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    assert lines, out.stdout[-3000:] + out.stderr[-3000:]
    return json.loads(lines[-1][len("RESULT "):])


def test_graph_capture_subprocess():
    """One captured FusedLARS step replayed 3 times with new gradients, a
    new LR before the third: held to the rule against 3 eager reference
    steps; the trust ratios follow the new gradients on replay."""
    res = _run_child("_lars_capture_gpu_child.py", timeout=240)
    print("capture child:", res)
    L.check(res["errs"], res["ref"], "gpu captured")
    assert res["v_after_capture"] == 0.0, res  # a capture runs nothing
    assert res["trust_changed"] == [True, True], res
    assert res["lr_gap"] > 1e-4, res  # the old LR would be far outside


def test_engine_lars_trains_captured_subprocess():
    """The engine's whole lars step (clip_grad_norm, HIP ops) under the
    default capture policy: the loss on a fixed batch falls over 8 steps.
    The batch is 8x3x64x64, as in test_fused_adam_gpu."""
    res = _run_child("_lars_engine_gpu_child.py", timeout=480)
    print("engine child:", res)
    assert res["captured"], res
    assert res["opt"] == "FusedLARS", res
    assert all(l == l and abs(l) != float("inf") for l in res["losses"]), res
    assert res["losses"][-1] < res["losses"][0], res
    assert res["global_step"] == 8, res
    assert res["trust_excluded_all_one"] and res["trust_moved"], res
    assert res["grad_norm"] > 0.0 and res["skipped"] == 0.0, res
