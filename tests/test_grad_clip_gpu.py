"""GPU tests of the gradient-norm kernels (csrc/grad_norm.hip), of the clip
state the update kernels read (fused_sgd.hip, fused_adam.hip), and of
GradClipper / the engine on them.

The norm bound. Every element is squared and summed in double (error about
n * 2^-53 relative, 1e-10 at the largest n here) and the result is rounded
to fp32 once (2^-24): against the fp64 norm on the CPU the relative error
must stay within 2^-23, one fp32 ulp, a factor 2 of slack. Measured on
MI355X: at most 3.4e-8 (0.29 ulp, at n = 3) over every case of this file;
each case prints its figure (CLIP_NORM lines under `pytest -s`).

Every test here requires an MI355X."""
import json
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import _adam_common as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from edl_amd import ops
else:
    ops = None

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2.0 ** -23
GUARD = 8
SENTINEL = -7.0
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    # loud check: the HIP extension must be present on a GPU box
    assert ops.available(), "edl_amd._C missing on a GPU box"


def _grad(n, offset=0):
    """_adam_common's first-step gradient (1e-6..1e2, every 7th zero)."""
    return C.make_inputs(n, offset)[1][0].float()


def _norm(bufs, grad_scale=C.GRAD_SCALE, max_norm=INF, skip=False,
          state=None, fill=SENTINEL):
    """Both raw bindings over `bufs` (GPU tensors) -> (state on CPU, the
    partial buffer, rows_total). The partial buffer is GUARD rows longer
    than needed and pre-filled, rows included: every row must be written."""
    ext = ops.ext()
    rows = sum(ext.grad_norm_rows(b.numel()) for b in bufs)
    partial = torch.full((rows + GUARD,), fill, dtype=torch.float64,
                         device="cuda")
    if state is None:
        state = torch.zeros(4, device="cuda")
    got_rows = ext.grad_sumsq(bufs, partial)
    assert got_rows == rows
    ext.grad_clip_finalize(partial, rows, state, grad_scale, max_norm, skip)
    torch.cuda.synchronize()
    return state.cpu(), partial, rows


def _check_norm(state, ref, what):
    got = float(state[1])
    rel = abs(got - ref) / ref
    print("CLIP_NORM %s: got %.9e fp64 %.9e rel %.3e (%.2f ulp)"
          % (what, got, ref, rel, rel / 2.0 ** -23))
    assert math.isfinite(got)
    assert rel <= BOUND, (what, got, ref, rel)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, C.N_REF])
def test_norm_matches_fp64(n):
    g = _grad(n)
    state, partial, rows = _norm([g.cuda()])
    _check_norm(state, C.GRAD_SCALE * float(g.double().norm()), "n=%d" % n)
    assert float(state[0]) == 1.0 and float(state[2]) == 0.0  # norm only
    tail = partial[rows:].cpu()
    assert torch.equal(tail, torch.full_like(tail, SENTINEL))
    assert rows == ops.ext().grad_norm_rows(n) == min(
        ops.ext().GRAD_NORM_ROW_CAP, max(1, -(-((n + 3) // 4) // 256)))


def test_norm_over_three_buffers():
    sizes, off, gs = [5, 1027, 4097], 0, []
    for n in sizes:
        gs.append(_grad(n, off))
        off += n
    state, partial, rows = _norm([g.cuda() for g in gs])
    _check_norm(state,
                C.GRAD_SCALE * float(torch.cat(gs).double().norm()),
                "three buffers")
    assert rows == 1 + 2 + 5
    assert bool((partial[:rows] >= 0).all())  # no sentinel left in a row


def test_empty_buffer_writes_a_zero_row():
    g = _grad(1027)
    state, partial, rows = _norm(
        [torch.empty(0, device="cuda"), g.cuda()])
    assert rows == 3 and float(partial[0]) == 0.0
    _check_norm(state, C.GRAD_SCALE * float(g.double().norm()), "empty+1027")
    state, _, rows = _norm([])
    assert rows == 0 and float(state[1]) == 0.0 and float(state[0]) == 1.0


@pytest.mark.parametrize("n", [5, 1027])
def test_bounds_guard_elements_not_read(n):
    g = _grad(n)
    buf = torch.full((n + GUARD,), 1e30, device="cuda")
    buf[:n].copy_(g)
    state, partial, rows = _norm([buf[:n]])
    _check_norm(state, C.GRAD_SCALE * float(g.double().norm()),
                "guarded n=%d" % n)
    tail = partial[rows:].cpu()
    assert tail.numel() == GUARD
    assert torch.equal(tail, torch.full_like(tail, SENTINEL))


def test_no_overflow_where_fp32_squares_would():
    g = _grad(1027)
    g[500] = 1e25
    assert math.isinf(float((g * g).sum()))  # what fp32 squares give
    state, _, _ = _norm([g.cuda()])
    _check_norm(state, C.GRAD_SCALE * float(g.double().norm()), "1e25")


def test_index_past_2_to_31():
    n = (1 << 31) + 5
    ones = torch.ones(n, device="cuda")
    state, _, rows = _norm([ones])
    del ones
    assert rows == ops.ext().GRAD_NORM_ROW_CAP
    _check_norm(state, C.GRAD_SCALE * math.sqrt(n), "n=2^31+5")


def test_two_runs_are_bit_equal():
    g = _grad(C.N_REF).cuda()
    # other garbage in the partial rows each time: all of them are written
    a, pa, rows = _norm([g], max_norm=1.0, fill=SENTINEL)
    b, pb, _ = _norm([g], max_norm=1.0, fill=float("nan"))
    assert torch.equal(a, b)
    assert torch.equal(pa[:rows], pb[:rows])
    assert float(a[0]) < 1.0  # clipped: coef is part of what is compared


def test_seventeen_buffers_take_two_launches():
    assert ops.ext().GRAD_NORM_MAX_SEGS == 16
    gs, off = [], 0
    for k in range(17):
        n = 3 + 61 * k
        gs.append(_grad(n, off))
        off += n
    state, partial, rows = _norm([g.cuda() for g in gs])
    _check_norm(state, C.GRAD_SCALE * float(torch.cat(gs).double().norm()),
                "17 buffers")
    assert rows == 17
    # row k is buffer k's own sum of squares, the 17th included
    want = torch.stack([g.double().pow(2).sum() for g in gs])
    assert torch.allclose(partial[:rows].cpu(), want, rtol=1e-12, atol=0)


def test_finalize_rule():
    """coef, skip and the skip count, on a norm known exactly: 16 ones,
    grad_scale 0.125 -> norm 0.5."""
    ones = torch.ones(16, device="cuda")
    st, _, _ = _norm([ones], max_norm=0.25)
    assert float(st[1]) == 0.5
    want = torch.tensor(0.25) / (torch.tensor(0.5) + 1e-6)  # torch, fp32
    assert float(st[0]) == float(want) and float(st[2]) == 0.0
    st, _, _ = _norm([ones], max_norm=2.0)
    assert float(st[0]) == 1.0
    bad = ones.clone()
    bad[3] = INF
    # no skip: torch's formula, max_norm / inf = 0 and inf / inf = nan
    st, _, _ = _norm([bad], max_norm=2.0)
    assert float(st[0]) == 0.0 and math.isinf(float(st[1]))
    st, _, _ = _norm([bad])
    assert math.isnan(float(st[0])) and float(st[2]) == 0.0
    bad[5] = float("nan")
    st, _, _ = _norm([bad], max_norm=2.0)
    assert math.isnan(float(st[0])) and math.isnan(float(st[1]))
    # skip: counted in the state it is given, cleared by a finite launch
    state = torch.tensor([9.0, 9.0, 9.0, 2.0], device="cuda")
    st, _, _ = _norm([bad], max_norm=2.0, skip=True, state=state)
    assert st.tolist()[0] == 0.0 and st.tolist()[2:] == [1.0, 3.0]
    st, _, _ = _norm([ones], max_norm=2.0, skip=True, state=state)
    assert st.tolist() == [1.0, 0.5, 0.0, 3.0]


def test_binding_rejects_bad_arguments():
    ext = ops.ext()
    g = torch.zeros(64, device="cuda")
    partial = torch.zeros(4, dtype=torch.float64, device="cuda")
    state = torch.zeros(4, device="cuda")
    with pytest.raises(RuntimeError, match="16-byte"):
        ext.grad_sumsq([torch.zeros(65, device="cuda")[1:]], partial)
    with pytest.raises(RuntimeError, match="fp32 only"):
        ext.grad_sumsq([g.double()], partial)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.grad_sumsq([torch.zeros(128, device="cuda")[::2]], partial)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        ext.grad_sumsq([g.cpu()], partial)
    with pytest.raises(RuntimeError, match="at least"):
        ext.grad_sumsq([g] * 5, partial)
    with pytest.raises(RuntimeError, match="fp64"):
        ext.grad_sumsq([g], partial.float())
    with pytest.raises(RuntimeError, match="rows_total"):
        ext.grad_clip_finalize(partial, 5, state, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="state must be"):
        ext.grad_clip_finalize(partial, 1, torch.zeros(3, device="cuda"),
                               1.0, 1.0)
    with pytest.raises(RuntimeError, match="max_norm"):
        ext.grad_clip_finalize(partial, 1, state, 1.0, -1.0)
    p, m, v = (torch.zeros(64, device="cuda") for _ in range(3))
    step = torch.ones(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="clip_state"):
        ext.fused_sgd(p, g, m, 0.1, 0.9, 0.0, 1.0, None, state[:3])
    with pytest.raises(RuntimeError, match="clip_state"):
        ext.fused_adam(p, g, m, v, step, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0,
                       False, None, None, None, state.double())
    torch.cuda.synchronize()
    assert not bool(p.ne(0).any())  # nothing launched


# ---- the update kernels read the state -----------------------------------

N_UPD = 1027  # 256 float4 + a 3-element tail


def _sgd(n, grads, clip, grad_scale=C.GRAD_SCALE):
    p0, _ = C.make_inputs(n)
    p = p0.float().cuda()
    m = torch.zeros(n, device="cuda")
    g = torch.empty(n, device="cuda")
    lr_dev = torch.full((1,), 1e-3, device="cuda")
    for gt in grads:
        g.copy_(gt.float())
        ops.ext().fused_sgd(p, g, m, 123.0, 0.9, 1e-2, grad_scale, lr_dev,
                            clip)
    torch.cuda.synchronize()
    return p.cpu(), m.cpu()


def _adam(n, grads, clip, mode="decoupled", grad_scale=C.GRAD_SCALE):
    """-> per-step (p, m, v) on CPU; the counter advances as FusedAdam.step
    does, by 1 - skip."""
    p0, _ = C.make_inputs(n)
    p = p0.float().cuda()
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    g = torch.empty(n, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    lr_dev = torch.full((1,), C.HYPER["lr"], device="cuda")
    out = []
    for gt in grads:
        g.copy_(gt.float())
        step.add_(1 if clip is None else int(1 - float(clip[2])))
        ops.ext().fused_adam(p, g, m, v, step, 123.0, *C.HYPER["betas"],
                             C.HYPER["eps"], C.WD[mode], grad_scale,
                             mode == "decoupled", lr_dev, None, None, clip)
        out.append((p.cpu(), m.cpu(), v.cpu()))
    torch.cuda.synchronize()
    return out


def _state(coef, skip):
    return torch.tensor([coef, 123.0, skip, 9.0], device="cuda")


def test_coef_one_is_bitwise_the_null_argument():
    _, grads = C.make_inputs(N_UPD)
    for a, b in zip(_sgd(N_UPD, grads, _state(1.0, 0.0)),
                    _sgd(N_UPD, grads, None)):
        assert torch.equal(a, b)
    a = _adam(N_UPD, grads, _state(1.0, 0.0))
    b = _adam(N_UPD, grads, None)
    for x, y in zip(a[-1], b[-1]):
        assert torch.equal(x, y)
    assert bool(a[-1][2].ne(0).any())


def test_skip_leaves_everything_unchanged():
    p0, grads = C.make_inputs(N_UPD)
    # a NaN coef: nothing of it may reach p, m or v
    skip = _state(float("nan"), 1.0)
    p, m = _sgd(N_UPD, grads[:2], skip)
    assert torch.equal(p, p0.float()) and not bool(m.ne(0).any())
    p, m, v = _adam(N_UPD, grads[:2], skip)[-1]
    assert torch.equal(p, p0.float())
    assert not bool(m.ne(0).any()) and not bool(v.ne(0).any())


@pytest.mark.parametrize("coef", [0.25, 0.3])
def test_coef_folds_into_the_gradient_scale(coef):
    """The kernel's scale is fl32(grad_scale * coef): bit-equal to passing
    that product as grad_scale (exact for 0.25, rounded once for 0.3)."""
    _, grads = C.make_inputs(N_UPD)
    c32 = torch.tensor(coef, dtype=torch.float32)
    folded = float(c32 * torch.tensor(C.GRAD_SCALE, dtype=torch.float32))
    if coef == 0.25:
        assert folded == C.GRAD_SCALE * 0.25
    for a, b in zip(_sgd(N_UPD, grads, _state(coef, 0.0)),
                    _sgd(N_UPD, grads, None, grad_scale=folded)):
        assert torch.equal(a, b)
    for x, y in zip(_adam(N_UPD, grads, _state(coef, 0.0))[-1],
                    _adam(N_UPD, grads, None, grad_scale=folded)[-1]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("mode", ["l2", "decoupled"])
def test_general_coef_matches_fp64_torch(mode):
    """coef = 0.3: six steps against torch on gradients scaled by the same
    fp32 coefficient, under _adam_common's K-rule."""
    c32 = float(torch.tensor(0.3, dtype=torch.float32))
    p0, grads = C.make_inputs(N_UPD)
    scaled = [g * c32 for g in grads]
    truth = C.torch_run(p0, scaled, mode, torch.float64)
    ref = C.run_errors(C.torch_run(p0, scaled, mode, torch.float32), truth)
    got = _adam(N_UPD, grads, _state(0.3, 0.0), mode)
    C.check(C.run_errors(got, truth), ref, "gpu coef 0.3 " + mode)


# ---- GradClipper and the engine ------------------------------------------

def test_engine_update_norm_is_lr_times_clipped_norm():
    """resnet18_vd, momentum 0, decay 0, eager: after one step
    ||dp|| = lr * min(norm, max_norm), with max_norm far below and far
    above the norm; last_grad_norm is the fp64 norm of the buckets. lr = 1
    keeps the update far above the rounding of p itself (about 3e-6 in
    norm over 11M params)."""
    from edl_amd.train.engine import TrainerEngine

    gen = torch.Generator().manual_seed(0)
    x = torch.randn(8, 3, 64, 64, generator=gen).cuda().contiguous(
        memory_format=torch.channels_last)
    y = torch.randint(0, 10, (8,), generator=gen).cuda()
    for max_norm, below in ((0.05, True), (1e4, False)):
        eng = TrainerEngine(
            model="resnet18_vd", per_device_batch=8, num_classes=10,
            base_lr=1.0, momentum=0.0, weight_decay=0.0, use_hip_ops=True,
            graph_capture=False, checkpoint_dir=None,
            clip_grad_norm=max_norm).setup()
        before = [b.param_flat.double() for b in eng.reducer._buckets]
        eng.train_step(x, y)
        torch.cuda.synchronize()
        norm = float(eng.last_grad_norm)
        ref = float(torch.linalg.vector_norm(torch.cat(
            [b.buffer.double() for b in eng.reducer._buckets])))
        dp = float(torch.linalg.vector_norm(torch.cat(
            [b.param_flat.double() - p0
             for b, p0 in zip(eng.reducer._buckets, before)])))
        want = 1.0 * min(norm, max_norm)
        print("CLIP_ENGINE max_norm %g: norm %.6e fp64 %.6e dp %.6e want %.6e"
              % (max_norm, norm, ref, dp, want))
        assert abs(norm - ref) <= BOUND * ref
        assert (norm > 10 * max_norm) if below else (norm < max_norm / 10)
        assert abs(dp - want) <= 1e-3 * want
        assert float(eng.skipped_steps) == 0.0
        assert eng.last_grad_norm.is_cuda and eng.skipped_steps.is_cuda


def _run_child(name, timeout):
    """Run a GPU script in a FRESH process (capture after unrelated GPU
    activity in the same process can crash the runtime, and a crash must
    not take the suite down). -> the child's RESULT dict."""
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
    """reduce + finalize + FusedAdamW.step captured once, replayed on a
    gradient below the bound, one above it, one holding an inf (skipped)
    and one below again: equals the three applied eager torch steps."""
    res = _run_child("_clip_capture_gpu_child.py", timeout=240)
    print("capture child:", res)
    assert res["step_after_capture"] == 0, res
    assert res["coef_lt_1"] == [False, True, False, False], res
    assert res["skip"] == [0.0, 0.0, 1.0, 0.0], res
    assert res["skipped_step_unchanged"], res
    assert res["step"] == 3 and res["nskipped"] == 1.0, res
    C.check(res["errs"], res["ref"], "gpu captured clip")


def test_two_ranks_one_gpu():
    """2 ranks share cuda:0 (gloo collectives: RCCL refuses a duplicate
    device), different data per rank: params and last_grad_norm end
    bit-equal across the ranks."""
    script = os.path.join(REPO, "tests", "_clip_cuda_worker.py")
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    env["EDL_FORCE_BACKEND"] = "gloo"
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29559", script],
        env=env, cwd=REPO, capture_output=True, text=True, timeout=240)
    sys.stderr.write(r.stdout[-2000:] + r.stderr[-1500:])
    assert r.returncode == 0
    oks = [json.loads(m) for m in re.findall(r'\{"clip_cuda".*?\}', r.stdout)]
    assert len(oks) == 2 and all(v["ok"] for v in oks), oks
    assert all(v["clipped"] >= 1 for v in oks), oks
