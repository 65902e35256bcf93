"""Worker for test_grad_clip_cpu.test_two_rank_gloo_clips_the_averaged_
gradient: two gloo ranks on CPU put DIFFERENT gradients into their buckets
(rank 1's has the sign of every odd element flipped, so the average keeps
the even elements and cancels the odd ones, exactly), all-reduce, clip with
GradClipper and step FusedAdamW with grad_scale = 1/2. Both ranks must end
bit-equal, in params and in the norm, and match (rule of _adam_common)
one process that clips the averaged gradient with clip_grad_norm_."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.environ.get("EDL_REPO") or os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _adam_common as C  # noqa: E402
import _clip_common as CC  # noqa: E402


def rank_sign(n, rank):
    s = torch.ones(n, dtype=torch.float64)
    if rank == 1:
        s[1::2] = -1.0
    return s


def same_on_all_ranks(t, world):
    got = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(got, t.contiguous())
    return all(torch.equal(got[0], x) for x in got[1:])


def main():
    rank = int(os.environ["RANK"])
    dist.init_process_group("gloo")
    world = dist.get_world_size()
    assert world == 2
    m, grads = CC.model()
    n = grads[0].numel()
    # what the ranks' average is, over GRAD_SCALE (exact: x + x and x - x)
    avg = [g * (rank_sign(n, 0) + rank_sign(n, 1)) / 2 for g in grads]
    max_norm = CC.max_norm_for(avg)
    clipped = CC.clipped_steps(avg, max_norm)
    assert any(clipped) and not all(clipped)
    r, opt, clipper = CC.make_fused(m, "adamw", max_norm, grad_scale=0.5)
    assert r.grad_scale == 0.5  # the DP average the optimizer folds in
    got = []
    for g in grads:
        r.zero_grad()
        CC.set_grads(m, g * rank_sign(n, rank) * C.GRAD_SCALE)
        r.finalize()
        st = clipper.run(opt.grad_scale)
        opt.step(clip_state=st)
        got.append(CC.fused_state(m, opt, "adamw"))
        assert same_on_all_ranks(st[:3].clone(), world)
    for x in got[-1]:
        assert same_on_all_ranks(x, world)
    truth = CC.torch_run("adamw", torch.float64, avg, max_norm)
    ref = C.run_errors(CC.torch_run("adamw", torch.float32, avg, max_norm),
                       truth)
    C.check(C.run_errors(got, truth), ref, "gloo rank %d" % rank)
    dist.barrier()
    dist.destroy_process_group()
    print("CLIP_GLOO_OK rank %d" % rank, flush=True)


if __name__ == "__main__":
    main()
