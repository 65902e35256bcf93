"""GPU tests of the fused Adam kernel (csrc/fused_adam.hip) and of FusedAdam
on it: numerics against torch.optim.Adam / AdamW on CPU under the tolerance
rule of _adam_common, the per-segment decay table, bounds, hipGraph
capture, and the engine with optimizer="adamw".

Every test here requires an MI355X."""
import json
import os
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
SEG_LENS = [1, 2, 3, 5, 4, 7, 1, 64, 1029]  # boundaries off float4 multiples
GUARD = 8


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    # loud check: the HIP extension must be present on a GPU box
    assert ops.available(), "edl_amd._C missing on a GPU box"


def _launch_steps(p0, grads, mode, wd, table=None, n_alloc=None):
    """Six launches of the raw binding on the first n elements of n_alloc
    element buffers, the device counter advanced before each (as
    FusedAdam.step does). -> (per-step (p, m, v) on CPU, final buffers)."""
    n = p0.numel()
    n_alloc = n_alloc or n
    dev = "cuda"
    bufs = [torch.full((n_alloc,), s, device=dev) for s in (7.0, 5.0, 3.0)]
    p, m, v = (b[:n] for b in bufs)
    p.copy_(p0.float())
    m.zero_()
    v.zero_()
    g = torch.empty(n, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    lr_dev = torch.full((1,), C.HYPER["lr"], device=dev)
    seg = (None, None)
    if table is not None:
        seg = (torch.tensor(table[0], dtype=torch.int32, device=dev),
               torch.tensor(table[1], dtype=torch.float32, device=dev))
    out = []
    for gt in grads:
        g.copy_(gt.float())
        step.add_(1)
        # host lr deliberately wrong: the device scalar must win
        ops.ext().fused_adam(p, g, m, v, step, 123.0, *C.HYPER["betas"],
                             C.HYPER["eps"], wd, C.GRAD_SCALE,
                             mode == "decoupled", lr_dev, *seg)
        out.append((p.cpu(), m.cpu(), v.cpu()))
    torch.cuda.synchronize()
    return out, bufs


@pytest.mark.parametrize("mode", ["l2", "decoupled"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, C.N_REF])
def test_kernel_matches_torch(n, mode):
    """Six steps driven by the device counter; each n is held to K times
    torch-fp32's own error on the same n elements."""
    truth, ref = C.case_reference(n, mode)
    p0, grads = C.make_inputs(n)
    got, _ = _launch_steps(p0, grads, mode, C.WD[mode])
    C.check(C.run_errors(got, truth), ref, "gpu n=%d %s" % (n, mode))


def _seg_table(wd_values):
    ends, wds, off = [], [], 0
    for k, ln in enumerate(SEG_LENS):
        off += ln
        ends.append(off)
        wds.append(wd_values[k % len(wd_values)])
    return ends, wds


def test_segment_table_matches_param_groups():
    """Decay alternates 0 / 1e-2 over segments shorter than a float4 and
    across float4 boundaries; the reference is torch AdamW with one param
    per segment in two param groups (the rule, literally, on these 1116
    elements)."""
    ends, wds = _seg_table([0.0, 1e-2])
    n = ends[-1]
    groups = [(e - ln, e, w) for e, ln, w in zip(ends, SEG_LENS, wds)]
    p0, grads = C.make_inputs(n)
    truth = C.torch_run(p0, grads, "decoupled", torch.float64, groups)
    ref = C.run_errors(
        C.torch_run(p0, grads, "decoupled", torch.float32, groups), truth)
    got, _ = _launch_steps(p0, grads, "decoupled", 0.5, (ends, wds))
    C.check(C.run_errors(got, truth), ref, "gpu segments")
    # the table matters: uniform decay would miss the rule
    uni, _ = _launch_steps(p0, grads, "decoupled", 1e-2)
    assert C.rel_err(uni[-1][0], truth[-1][0]) > C.K * ref["p"]


@pytest.mark.parametrize("mode", ["l2", "decoupled"])
def test_all_equal_table_is_bitwise_the_null_table(mode):
    ends, wds = _seg_table([1e-2])
    p0, grads = C.make_inputs(ends[-1])
    # the uniform wd argument is ignored when a table is given
    a, _ = _launch_steps(p0, grads, mode, 0.75, (ends, wds))
    b, _ = _launch_steps(p0, grads, mode, 1e-2)
    for x, y in zip(a[-1], b[-1]):
        assert torch.equal(x, y)
    assert bool(a[-1][1].ne(0).any())


@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("n", [5, 1027])
def test_bounds_guard_elements_untouched(n, with_table):
    table = None
    if with_table:
        cut = [1, 3, n - 1, n] if n == 5 else [1, 6, 513, 1026, n]
        table = (cut, [1e-2 * (k % 2) for k in range(len(cut))])
    p0, grads = C.make_inputs(n)
    n_alloc = (n + GUARD + 3) // 4 * 4 + 4
    got, bufs = _launch_steps(p0, grads, "decoupled", 1e-2, table, n_alloc)
    for b, sentinel in zip(bufs, (7.0, 5.0, 3.0)):
        tail = b[n:].cpu()
        assert tail.numel() >= GUARD
        assert torch.equal(tail, torch.full_like(tail, sentinel))
    assert bool(got[-1][2].ne(0).any())  # the first n really updated


def test_binding_rejects_bad_arguments():
    ext = ops.ext()
    dev = "cuda"
    p, g, m, v = (torch.zeros(16, device=dev) for _ in range(4))
    step = torch.ones(1, dtype=torch.int32, device=dev)
    args = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, False)

    def table(ends):
        return (None, torch.tensor(ends, dtype=torch.int32, device=dev),
                torch.zeros(len(ends), device=dev))

    with pytest.raises(RuntimeError, match="16-byte"):
        ext.fused_adam(torch.zeros(17, device=dev)[1:], g, m, v, step, *args)
    with pytest.raises(RuntimeError, match="size mismatch"):
        ext.fused_adam(p, g[:8], m, v, step, *args)
    with pytest.raises(RuntimeError, match="int32"):
        ext.fused_adam(p, g, m, v, step.float(), *args)
    with pytest.raises(RuntimeError, match="last seg_end"):
        ext.fused_adam(p, g, m, v, step, *args, *table([4, 12]))
    with pytest.raises(RuntimeError, match="differ in length"):
        ext.fused_adam(p, g, m, v, step, *args, None,
                       torch.tensor([16], dtype=torch.int32, device=dev),
                       torch.zeros(2, device=dev))
    with pytest.raises(RuntimeError, match="segments <= 1024"):
        ext.fused_adam(p, g, m, v, step, *args,
                       *table(list(range(1, 1026))))
    assert ext.ADAM_MAX_SEGMENTS == 1024
    torch.cuda.synchronize()
    assert not bool(p.ne(0).any())  # nothing launched


def test_table_is_rechecked_when_it_changes():
    """A table that passed once is checked again after an in-place write
    (version counter) and so is a NEW tensor, wherever it is allocated."""
    ext = ops.ext()
    dev = "cuda"
    p, g, m, v = (torch.zeros(16, device=dev) for _ in range(4))
    step = torch.ones(1, dtype=torch.int32, device=dev)
    args = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, False, None)
    wd = torch.zeros(2, device=dev)
    ends = torch.tensor([4, 16], dtype=torch.int32, device=dev)
    ext.fused_adam(p, g, m, v, step, *args, ends, wd)
    ext.fused_adam(p, g, m, v, step, *args, ends, wd)
    ends[1] = 12
    with pytest.raises(RuntimeError, match="last seg_end"):
        ext.fused_adam(p, g, m, v, step, *args, ends, wd)
    del ends
    for _ in range(3):  # the allocator may hand the freed block out again
        bad = torch.tensor([4, 12], dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError, match="last seg_end"):
            ext.fused_adam(p, g, m, v, step, *args, bad, wd)
        del bad
    dec = torch.tensor([8, 4], dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="must not decrease"):
        ext.fused_adam(p, g, m, v, step, *args, dec, wd)


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
    """One captured FusedAdamW step (decay table included) replayed 3
    times equals 3 eager torch AdamW steps: t advanced on replay, the LR
    change before the third replay took effect, state_dict() says 3."""
    res = _run_child("_adam_capture_gpu_child.py", timeout=240)
    print("capture child:", res)
    assert res["has_table"], res
    assert res["step_after_capture"] == 0, res
    assert res["step"] == 3 and res["sd_step"] == 3.0, res
    C.check(res["errs"], res["ref"], "gpu captured")
    assert res["lr_gap"] > 1e-4, res  # the old LR would be far outside


def test_engine_adamw_trains_captured_subprocess():
    """The engine's whole adamw step under the default capture policy:
    the loss on a fixed batch falls over 8 steps (it would stay flat if the
    bf16 mirrors or the weight epoch were not refreshed) and the optimizer
    counted all 8 — eager, warm-up and replayed ones. The batch is
    8x3x64x64, the size test_fused_sgd_trains_resnet_gpu runs. 2x3x32x32
    would leave the last two stages M = 8 and M = 2 rows for the MFMA GEMM,
    3x3 and wgrad kernels; no binding rejects that, but no test of this
    suite has ever run them below M = 32 (this batch's last stage), and
    the bounds of a dozen kernels at such M are not something this test is
    the place to find out."""
    res = _run_child("_adam_engine_gpu_child.py", timeout=480)
    print("engine child:", res)
    assert res["captured"], res
    assert res["opt"] == "FusedAdam" and res["tables"] >= 1, res
    assert all(l == l and abs(l) != float("inf") for l in res["losses"]), res
    assert res["losses"][-1] < res["losses"][0], res
    assert res["global_step"] == 8 and res["opt_step"] == 8, res
