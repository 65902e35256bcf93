"""Worker for test_dgc_momentum_gpu.test_two_ranks_one_gpu: 2 gloo ranks
sharing cuda:0 run DGCMomentum (HIP compress / decode) for 4 steps on
exact-arithmetic gradients written straight into the bucket buffers. The
decoded buckets must be bit-equal across the ranks and bit-equal to a
torch-path simulation of BOTH ranks, which every rank builds locally on
the CPU from the known seeds."""
import json
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _dgc_momentum_common import MU, WD, exact_inputs  # noqa: E402
from edl_amd.ops.dgc import dgc_compress, dgc_decode  # noqa: E402
from edl_amd.train.bucketed_ddp import BucketedAllReducer  # noqa: E402
from edl_amd.train.dgc import DGCMomentum  # noqa: E402

STEPS, BEGIN, RAMP, SPARSITY = 4, 1, 2, (0.75, 0.9375)


def grad_for(n, step, rank, bucket):
    return exact_inputs(n, seed=1000 + 100 * step + 10 * rank + bucket)[0]


def main():
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(7)
    model = torch.nn.Sequential(
        torch.nn.Linear(257, 129), torch.nn.ReLU(), torch.nn.Linear(129, 7)
    ).cuda()
    reducer = BucketedAllReducer(model.parameters(), bucket_cap_mb=0.05)
    sizes = [b.buffer.numel() for b in reducer._buckets]
    # exact-arithmetic params (integers/16), the same on both ranks
    for i, b in enumerate(reducer._buckets):
        b.param_flat.copy_(exact_inputs(sizes[i], seed=500 + i)[3])
    dgc = DGCMomentum(reducer, None, MU, WD, rampup_begin_step=BEGIN,
                      rampup_step=RAMP, sparsity=SPARSITY)

    # torch-path simulation of both ranks (CPU)
    sim_p = [b.param_flat.cpu() for b in reducer._buckets]
    sim_u = [[torch.zeros(n) for n in sizes] for _ in range(world)]
    sim_v = [[torch.zeros(n) for n in sizes] for _ in range(world)]

    ok, detail = True, ""
    for s in range(1, STEPS + 1):
        for i, b in enumerate(reducer._buckets):
            b.buffer.copy_(grad_for(sizes[i], s, rank, i))
        compressed = dgc.step(global_step=s)
        if compressed != (s > BEGIN):
            ok, detail = False, "phase wrong at step %d" % s
        for i, b in enumerate(reducer._buckets):
            n = sizes[i]
            if s <= BEGIN:
                want = sum(grad_for(n, s, r, i) for r in range(world))
            else:
                k = dgc.k_for(n, s)
                pls = [dgc_compress(grad_for(n, s, r, i), sim_u[r][i],
                                    sim_v[r][i], sim_p[i], MU, WD, k)
                       for r in range(world)]
                want = dgc_decode(torch.empty(n), pls)
            got = b.buffer.cpu()
            if not torch.equal(got, want):
                ok = False
                detail = "step %d bucket %d differs from the simulation" % (s, i)
            gathered = [torch.empty_like(got) for _ in range(world)]
            dist.all_gather(gathered, got)
            if not all(torch.equal(t, gathered[0]) for t in gathered):
                ok, detail = False, "step %d bucket %d differs across ranks" % (s, i)
    # the ramp was walked: 0.75 at s=2, 0.9375 from s=3
    ks = [dgc.k_for(1000, s) for s in (2, 3, 4)]
    if ks != [250, 62, 62]:
        ok, detail = False, "schedule %r" % (ks,)
    for i in range(len(sizes)):
        if not (torch.equal(dgc._state[i]["u"].cpu(), sim_u[rank][i])
                and torch.equal(dgc._state[i]["v"].cpu(), sim_v[rank][i])):
            ok, detail = False, "u/v of bucket %d differ from the simulation" % i
    dist.barrier()
    dist.destroy_process_group()
    print(json.dumps({"dgc_momentum_cuda": True, "rank": rank, "ok": ok,
                      "buckets": len(sizes), "detail": detail}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
