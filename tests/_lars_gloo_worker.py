"""Worker for test_fused_lars_cpu.test_two_rank_gloo_identical_bits: two gloo
ranks on CPU resume TrainerEngine(optimizer="lars") from DIFFERENT local
checkpoints (argv[1]/rank<r>). After setup() both must hold rank 0's
velocities; after 3 steps on per-rank data the params, the velocities and
the trust ratios must agree bit for bit."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.environ.get("EDL_REPO") or os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))

from edl_amd.models import build_model  # noqa: E402
from edl_amd.ops.lars import FusedLARS  # noqa: E402
from edl_amd.train.bucketed_ddp import BucketedAllReducer  # noqa: E402
from edl_amd.train.checkpoint import CheckpointManager  # noqa: E402
from edl_amd.train.engine import TrainerEngine  # noqa: E402


def write_local_checkpoint(path, rank):
    """A checkpoint only this rank has: 2 + rank LARS steps on its own
    random gradients."""
    torch.manual_seed(500 + rank)
    model = build_model("mnist_mlp", num_classes=10)
    r = BucketedAllReducer(model.parameters(), bucket_cap_mb=25)
    opt = FusedLARS(model.parameters(), lr=0.1, lars_coeff=0.02, reducer=r,
                    exclude=lambda p: p.ndim <= 1)  # as no_decay_1d
    for _ in range(2 + rank):
        for p in model.parameters():
            p.grad.copy_(torch.randn_like(p))
        opt.step()
    CheckpointManager(path, use_pinned=False).save(
        model.state_dict(), {"epoch_no": 0, "global_step": 2 + rank},
        optimizer_state=opt.state_dict(), blocking=True)


def same_on_all_ranks(t, world):
    got = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(got, t.contiguous())
    return all(torch.equal(got[0], x) for x in got[1:])


def main():
    rank = int(os.environ["RANK"])
    ckpt = os.path.join(sys.argv[1], "rank%d" % rank)
    write_local_checkpoint(ckpt, rank)
    eng = TrainerEngine(
        model="mnist_mlp", per_device_batch=8, num_classes=10, base_lr=0.1,
        weight_decay=5e-4, label_smoothing=0.0, dtype="fp32",
        channels_last=False, checkpoint_dir=ckpt, use_hip_ops=False,
        optimizer="lars", lars_coeff=0.02, no_decay_1d=True,
        clip_grad_norm=1.0).setup()
    world = dist.get_world_size()
    assert world == 2
    bufs = eng.opt.state_buffers()
    assert len(bufs) == len(eng.reducer._buckets)
    for t in bufs:
        assert same_on_all_ranks(t, world)
    assert any(bool(t.ne(0).any()) for t in bufs)  # really resumed
    gen = torch.Generator().manual_seed(100 + rank)  # per-rank data
    for _ in range(3):
        x = torch.randn(8, 1, 28, 28, generator=gen)
        y = torch.randint(0, 10, (8,), generator=gen)
        eng.train_step(x, y)
    for p in eng.model.parameters():
        assert same_on_all_ranks(p.detach(), world)
    for t in eng.opt.state_buffers() + [eng.last_trust_ratios]:
        assert same_on_all_ranks(t, world)
    assert bool(eng.last_trust_ratios.ne(1).any())
    dist.barrier()
    dist.destroy_process_group()
    print("LARS_GLOO_OK rank %d" % rank, flush=True)


if __name__ == "__main__":
    main()
