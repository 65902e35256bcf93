"""bench.py driver-contract test on CPU (gloo, world 2): the exact
invocation shape the driver uses for SCALE runs, minus the GPUs."""
import json
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_plain(extra):
    # the CPU path everywhere (fp32, bit-reproducible): hide any GPU
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "1", "--model", "resnet18_vd",
         "--batch_size", "2"] + extra,
        env=env, cwd=REPO, capture_output=True, text=True, timeout=240,
    )
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly ONE JSON result line"
    return json.loads(lines[0])


DUMP_NAMES = ["bn_var", "loss"]


def _state_arrays(eng, loss):
    """The dump's contract, written out independently of bench.py."""
    import numpy as np

    return {
        "loss": np.array([loss.item()]),
        "bn_var": np.concatenate(
            [b.numpy().ravel() for n, b in eng.model.named_buffers()
             if n.endswith("running_var")]),
    }


def test_bench_dump_outputs_match_independent_run(tmp_path, monkeypatch):
    """--dump-outputs against a reference that shares no code with it: the
    same seeded engine and loader stepped in this process. The dump must
    equal the state after warmup + steps, and differ from the state one
    step earlier and from the state before the timed steps, so a dump of
    stale, constant or warmup values cannot pass. Two runs with the same
    arguments agree bit for bit on the CPU path, and --full keeps the line.

    Tolerance: both sides are the same fp32 CPU code on the same inputs;
    only the summation order of threaded reductions may differ: ~1e-6
    relative, times the ~1e2 that the untrained 18-layer net can amplify
    -> rtol 1e-4."""
    import numpy as np
    import torch

    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    ja = _run_plain(["--dump-outputs", a])
    jb = _run_plain(["--dump-outputs", b, "--full"])
    for j in (ja, jb):
        assert j["metric"] == "img/s" and j["unit"] == "img/s"
        assert j["steps"] == 2 and j["ms_per_step"] > 0
        assert j["higher_is_better"] is True and j["dtype"] == "fp32"
    assert sorted(os.listdir(a)) == [n + ".npy" for n in DUMP_NAMES]
    assert sum(os.path.getsize(os.path.join(a, f))
               for f in os.listdir(a)) <= 64 * 2**20
    dump = {}
    for name in DUMP_NAMES:
        dump[name] = np.load(os.path.join(a, name + ".npy"))
        assert dump[name].dtype == np.float32 and dump[name].ndim == 1
        assert np.isfinite(dump[name]).all()
        assert np.array_equal(dump[name],
                              np.load(os.path.join(b, name + ".npy"))), name

    # the reference: bench.py's documented protocol (one batch for the
    # capture attempt, W warmup steps, K timed steps), _run_plain's arguments
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from edl_amd.data.synthetic import SyntheticImageNet
    from edl_amd.train.engine import TrainerEngine

    eng = TrainerEngine(model="resnet18_vd", per_device_batch=2, base_lr=0.1,
                        dtype="fp32", channels_last=False, checkpoint_dir=None,
                        use_hip_ops=False).setup()
    eng.model.train()
    eng.set_lr(eng.scaled_lr(0))
    loader = SyntheticImageNet(2, eng.device, channels_last=False, seed=1234)
    loader.next()
    states = []
    for _ in range(1 + 2):
        x, y = loader.next()
        states.append(_state_arrays(eng, eng.train_step(x, y)))
    before_timed, one_short, want = states

    for name in DUMP_NAMES:
        assert dump[name].shape == want[name].shape, name
        assert np.allclose(dump[name], want[name], rtol=1e-4, atol=1e-7), (
            name, np.abs(dump[name] - want[name]).max())
        for other in (before_timed, one_short):
            rel = (np.linalg.norm(dump[name] - other[name])
                   / np.linalg.norm(want[name]))
            assert rel > 1e-3, (name, rel)  # >> the 1e-4 it matches `want` to


def test_bench_dump_sampling_is_fixed(tmp_path, monkeypatch):
    """Arrays above DUMP_MAX_ELEMS are cut by ONE documented index sample:
    sorted default_rng(0).choice(n, DUMP_MAX_ELEMS, replace=False)."""
    import numpy as np
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.syspath_prepend(REPO)
    import bench
    from edl_amd.train.engine import TrainerEngine

    eng = TrainerEngine(model="resnet18_vd", per_device_batch=2, num_classes=10,
                        dtype="fp32", channels_last=False, checkpoint_dir=None,
                        use_hip_ops=False).setup()
    x = torch.randn(2, 3, 64, 64)
    loss = eng.train_step(x, torch.tensor([1, 2]))
    full = _state_arrays(eng, loss)
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    bench.dump_outputs(str(tmp_path), eng, loss)
    for name in ("bn_var",):
        n = full[name].size
        assert n > 1000
        idx = np.sort(np.random.default_rng(0).choice(n, size=1000, replace=False))
        got = np.load(str(tmp_path / (name + ".npy")))
        assert got.shape == (1000,)
        assert np.allclose(got, full[name][idx], rtol=1e-6, atol=0), name
    assert np.load(str(tmp_path / "loss.npy")).shape == (1,)  # below the cap


def test_bench_world2_gloo_json_contract():
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    # this is the CPU/gloo form of the contract: on a box that does have a
    # GPU both ranks would land on cuda:0 and RCCL refuses duplicate devices
    env["HIP_VISIBLE_DEVICES"] = env["CUDA_VISIBLE_DEVICES"] = ""
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29541", os.path.join(REPO, "bench.py"),
         "--gpus", "2", "--steps", "2", "--warmup", "1",
         "--model", "resnet18_vd", "--batch_size", "2"],
        env=env, cwd=REPO, capture_output=True, text=True, timeout=420,
    )
    sys.stderr.write(r.stdout[-2000:] + r.stderr[-1500:])
    assert r.returncode == 0
    # torchrun can interleave rank output without newlines
    matches = re.findall(r'\{"metric".*?\}\}', r.stdout)
    assert len(matches) == 1, "exactly ONE rank prints the JSON line"
    j = json.loads(matches[0])
    assert j["metric"] == "img/s" and j["value"] > 0
    assert j["n_gpus"] == 2 and j["steps"] == 2 and j["warmup"] == 1
    assert j["scaling"] == "weak" and j["higher_is_better"] is True
    assert j["config"]["global_batch"] == 4  # 2/rank x 2 (whole-job)
    assert j["config"]["parallelism"] == "dp2"
    assert "ms_per_step" in j and "vs_baseline" in j
