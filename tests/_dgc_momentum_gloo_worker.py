"""Worker for test_dgc_momentum_cpu.test_engine_two_rank_gloo_matches_plain_sgd:
2 gloo ranks on CPU drive TrainerEngine with DGC momentum correction at
sparsity 0.0 and compare against torch.optim.SGD(momentum=0,
weight_decay=wd) on the rank-averaged gradients."""
import copy
import os
import sys

import torch
import torch.distributed as dist
import torch.nn.functional as F

sys.path.insert(0, os.environ.get("EDL_REPO") or os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))

from edl_amd.train.dgc import DGCMomentum  # noqa: E402
from edl_amd.train.engine import TrainerEngine  # noqa: E402


def main():
    lr, wd = 0.05, 1e-2
    eng = TrainerEngine(
        model="mnist_mlp", per_device_batch=8, num_classes=10, base_lr=lr,
        momentum=0.9, weight_decay=wd, label_smoothing=0.0, dtype="fp32",
        channels_last=False, checkpoint_dir=None, use_hip_ops=False,
        dgc=True, dgc_momentum_correction=True, dgc_sparsity=(0.0,),
        dgc_rampup=0).setup()
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2 and isinstance(eng.dgc, DGCMomentum)
    ref = copy.deepcopy(eng.model)  # after the rank-0 broadcast
    opt = torch.optim.SGD(ref.parameters(), lr=lr, momentum=0.0,
                          weight_decay=wd)
    gen = torch.Generator().manual_seed(100 + rank)  # per-rank data
    for step in range(3):
        x = torch.randn(8, 1, 28, 28, generator=gen)
        y = torch.randint(0, 10, (8,), generator=gen)
        eng.train_step(x, y)
        assert eng.dgc.compressed
        opt.zero_grad()
        F.cross_entropy(ref(x), y).backward()
        for p in ref.parameters():
            dist.all_reduce(p.grad)
            p.grad.div_(world)
        opt.step()
        for (name, p), q in zip(eng.model.named_parameters(),
                                ref.parameters()):
            assert torch.allclose(p, q, rtol=1e-5), (
                step, name, float((p - q).abs().max()))
        # everything non-zero was sent: nothing is held back
        for st in eng.dgc._state:
            assert not bool(st["u"].ne(0).any() or st["v"].ne(0).any())
    # the plain-SGD trajectory really moved
    assert eng.global_step == 3
    dist.barrier()
    dist.destroy_process_group()
    print("DGC_GLOO_OK rank %d" % rank, flush=True)


if __name__ == "__main__":
    main()
