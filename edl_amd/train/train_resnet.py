"""Flagship collective trainer — the `train_with_fleet.py` equivalent.

Spawned by the edlrun launcher (one process per GPU); reads the env
contract (TrainerEnv), builds the RCCL world, trains ResNet50_vd (or any
model in the zoo) on synthetic ImageNet-shaped data, or on image files
(--image_root with --train_list or --data_dir: data/images.py), with elastic
stop-resume: per-epoch (and optional per-N-steps) checkpoints, LR rescaled
by the linear-scaling rule on every world change, train status reported to
the coordination store so the generator can veto near-end scaling.

CLI parity subset of reference example/collective/resnet50/train_with_fleet.py.
"""
import argparse
import os
import sys
import time

import torch

from ..cluster.status import TrainStatus, save_train_status
from ..coord.client import CoordClient
from ..data.mixup import MixupLoader
from ..data.synthetic import SyntheticImageNet
from ..utils.log import get_logger
from . import dist as edist
from .engine import TrainerEngine
from .env import TrainerEnv

log = get_logger("edl.train")


def parse_args(argv=None):
    p = argparse.ArgumentParser("edl_amd resnet trainer")
    p.add_argument("--model", default="resnet50_vd")
    p.add_argument("--batch_size", type=int, default=32, help="per-GPU batch")
    p.add_argument("--num_epochs", type=int, default=2)
    p.add_argument("--steps_per_epoch", type=int, default=100)
    p.add_argument("--lr", type=float, default=0.1)
    p.add_argument("--momentum", type=float, default=0.9)
    p.add_argument("--weight_decay", type=float, default=1e-4)
    p.add_argument("--checkpoint", default=None, help="checkpoint dir (resume + save)")
    p.add_argument("--checkpoint_steps", type=int, default=0,
                   help="also checkpoint every N steps (0 = per-epoch only)")
    p.add_argument("--data_dir", default=None,
                   help="txt record files: train through the elastic "
                        "data plane (leader-balanced Reader) instead of "
                        "the synthetic loader; records deterministically "
                        "seed synthetic images, or with --image_root name "
                        "the image files to decode")
    p.add_argument("--image_hw", type=int, default=224)
    p.add_argument("--use_hip_ops", type=int, default=1)
    p.add_argument("--graph_capture", type=int, default=None)
    p.add_argument("--bucket_mb", type=int, default=25)
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--profile", action="store_true")
    # reference train_with_fleet.py: --use_label_smoothing /
    # --label_smoothing_epsilon, --use_mixup / --mixup_alpha, and the
    # per-epoch test_prog pass (loss / acc_top1 / acc_top5)
    p.add_argument("--label_smoothing", type=float, default=0.1)
    p.add_argument("--use_mixup", type=int, default=0)
    p.add_argument("--mixup_alpha", type=float, default=0.2)
    p.add_argument("--fused_ce", type=int, default=0,
                   help="hard-label loss on the fused softmax-CE kernel")
    p.add_argument("--eval_steps", type=int, default=0,
                   help="validation batches after each epoch (0 = no eval)")
    # reference train_with_fleet.py --use_dgc / --rampup_begin_step
    # (DGCMomentumOptimizer): DGC with momentum correction
    p.add_argument("--use_dgc", type=int, default=0)
    p.add_argument("--rampup_begin_step", type=int, default=0,
                   help="dense all-reduce up to and including this step")
    p.add_argument("--rampup_step", type=int, default=1,
                   help="steps over which --dgc_sparsity is walked")
    p.add_argument("--dgc_sparsity", default="0.999",
                   help="comma list, e.g. 0.75,0.9375,0.984375,0.996,0.999")
    # reference train_with_fleet.py:196-200 `adam` strategy (constant LR);
    # adamw = decoupled decay
    p.add_argument("--optimizer", default="momentum",
                   choices=["momentum", "adam", "adamw", "lars"])
    p.add_argument("--beta1", type=float, default=0.9)
    p.add_argument("--beta2", type=float, default=0.999)
    p.add_argument("--epsilon", type=float, default=1e-8)
    p.add_argument("--no_decay_1d", type=int, default=0,
                   help="adam/adamw: no weight decay on biases and BN "
                        "scale/shift (params with ndim <= 1); lars: those "
                        "take the plain LR")
    # lars: Paddle's lars_momentum; --weight_decay is the LARS decay and the
    # LR follows the momentum schedule
    p.add_argument("--lars_coeff", type=float, default=0.001)
    p.add_argument("--lars_eps", type=float, default=0.0)
    p.add_argument("--clip_grad_norm", type=float, default=None,
                   help="clip the global gradient norm to this value "
                        "(device-side, capture-safe; not with --use_dgc)")
    p.add_argument("--skip_nonfinite", type=int, default=0,
                   help="skip the update of a step whose gradient norm is "
                        "inf/nan")
    # image files (reference train_with_fleet.py --data_dir + dali.py /
    # utils/reader.py): `relpath label` records decoded from --image_root
    p.add_argument("--image_root", default=None,
                   help="directory the records' image paths are relative "
                        "to: with --data_dir the data-plane records are "
                        "decoded from it, else --train_list names them")
    p.add_argument("--train_list", default=None,
                   help="file of `relpath label` lines (with --image_root, "
                        "without --data_dir), sharded records[rank::world]")
    p.add_argument("--val_list", default=None,
                   help="file of `relpath label` lines for --eval_steps")
    p.add_argument("--lower_scale", type=float, default=0.08)
    p.add_argument("--lower_ratio", type=float, default=3.0 / 4.0)
    p.add_argument("--upper_ratio", type=float, default=4.0 / 3.0)
    p.add_argument("--resize_short", type=float, default=None,
                   help="eval: short side before the centre crop "
                        "(default image_hw * 256/224)")
    p.add_argument("--input_dtype", default="auto",
                   choices=["auto", "fp32", "bf16"],
                   help="dtype of the image batches from --image_root; auto "
                        "= bf16 when the engine runs bf16 on a GPU")
    p.add_argument("--decode_workers", type=int, default=8)
    return p.parse_args(argv)


def read_list(path):
    with open(path) as f:
        return [ln.strip() for ln in f if ln.strip()]


def main(argv=None):
    args = parse_args(argv)
    tenv = TrainerEnv()
    ckpt_dir = args.checkpoint or tenv.checkpoint_dir

    engine = TrainerEngine(
        model=args.model,
        per_device_batch=args.batch_size,
        base_lr=args.lr,
        momentum=args.momentum,
        weight_decay=args.weight_decay,
        dtype=args.dtype if torch.cuda.is_available() else "fp32",
        channels_last=torch.cuda.is_available(),
        bucket_mb=args.bucket_mb,
        checkpoint_dir=ckpt_dir,
        use_hip_ops=bool(args.use_hip_ops) and torch.cuda.is_available(),
        graph_capture=None if args.graph_capture is None else bool(args.graph_capture),
        label_smoothing=args.label_smoothing,
        fused_ce=bool(args.fused_ce),
        dgc=bool(args.use_dgc),
        dgc_momentum_correction=bool(args.use_dgc),
        dgc_rampup=args.rampup_begin_step,
        dgc_rampup_step=args.rampup_step,
        dgc_sparsity=[float(x) for x in args.dgc_sparsity.split(",") if x],
        optimizer=args.optimizer,
        betas=(args.beta1, args.beta2),
        eps=args.epsilon,
        no_decay_1d=bool(args.no_decay_1d),
        clip_grad_norm=args.clip_grad_norm,
        skip_nonfinite=bool(args.skip_nonfinite),
        lars_coeff=args.lars_coeff,
        lars_eps=args.lars_eps,
    ).setup(tenv)

    # status reporting back to the control plane (reference TrainStatus flow,
    # utils/train_status.py; generator reads it to veto near-end scale-out)
    store = None
    if tenv.store_endpoints:
        try:
            store = CoordClient(tenv.store_endpoints, tenv.job_id)
        except Exception as e:  # noqa: BLE001
            log.warning("no coordination store (%s); status reporting off", e)
    pod_id = os.environ.get("EDL_POD_ID", "pod")

    def report(status):
        if store is not None and tenv.is_rank0:
            try:
                save_train_status(store, pod_id, status)
            except Exception:  # noqa: BLE001
                pass

    report(TrainStatus.RUNNING)
    shape = (3, args.image_hw, args.image_hw)
    cl = engine.channels_last and engine.device.type == "cuda"
    if (args.train_list or args.val_list) and not args.image_root:
        raise SystemExit("--train_list / --val_list need --image_root")
    if args.image_root and not (args.data_dir or args.train_list):
        raise SystemExit("--image_root needs --data_dir or --train_list")
    if args.train_list and args.data_dir:
        raise SystemExit("--train_list and --data_dir exclude each other")

    def image_loader(records, train, epoch=0):
        from ..data.images import ImageRecordLoader

        bf16 = (args.input_dtype == "bf16" or
                (args.input_dtype == "auto" and engine.device.type == "cuda"
                 and engine.dtype == torch.bfloat16))
        return ImageRecordLoader(
            records, args.image_root, args.batch_size, engine.device,
            out_size=args.image_hw, train=train, seed=1234, epoch=epoch,
            out_dtype=torch.bfloat16 if bf16 else torch.float32,
            num_workers=args.decode_workers, lower_scale=args.lower_scale,
            lower_ratio=args.lower_ratio, upper_ratio=args.upper_ratio,
            resize_short=args.resize_short)

    train_records = None
    if args.train_list:
        rank, world = engine.env.global_rank, engine.world_size
        train_records = read_list(args.train_list)[rank::world]
    loader = None
    if not args.data_dir and train_records is None:
        loader = SyntheticImageNet(
            args.batch_size, engine.device, image_shape=shape,
            channels_last=cl, seed=1234 + engine.env.global_rank,
        )

    eval_loader = None
    if args.eval_steps > 0 and args.val_list:
        rank, world = engine.env.global_rank, engine.world_size
        eval_loader = image_loader(read_list(args.val_list)[rank::world],
                                   train=False)
    elif args.eval_steps > 0:
        # held-out synthetic batches: a seed of their own
        eval_loader = SyntheticImageNet(
            args.batch_size, engine.device, image_shape=shape,
            channels_last=cl, seed=987654 + engine.env.global_rank,
        )

    def agree_steps(steps):
        """Ranks can hold slightly unequal record counts, so all ranks
        agree on the MIN step count before training (collectives must
        stay matched across the world)."""
        import torch.distributed as dist

        if dist.is_initialized():
            t = torch.tensor([steps], dtype=torch.long,
                             device=engine.device
                             if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            steps = int(t.item())
        if args.steps_per_epoch:
            steps = min(steps, args.steps_per_epoch)
        return steps

    def plane_epoch_loader(epoch):
        """Elastic data plane: leader-balanced record slices -> loader."""
        from ..data.plane import RecordImageSet, fetch_epoch_records

        recs = fetch_epoch_records(tenv, args.data_dir, args.batch_size)
        if args.image_root:
            # no full batch: report 0 steps (below) rather than build a loader
            ds = (image_loader(recs, True, epoch)
                  if len(recs) >= args.batch_size else None)
        else:
            ds = RecordImageSet(recs, args.batch_size, engine.device,
                                image_shape=shape, channels_last=cl)
        return ds, agree_steps(ds.steps() if ds is not None else 0)

    def on_step(epoch, it):
        if args.checkpoint_steps and (engine.global_step % args.checkpoint_steps == 0):
            engine.save_checkpoint(
                epoch, extra={"mid_epoch": True, "step_in_epoch": it + 1})

    t_start = time.monotonic()
    for epoch in range(engine.start_epoch, args.num_epochs):
        if epoch == args.num_epochs - 1:
            report(TrainStatus.NEARTHEEND)
        if args.data_dir:
            ep_loader, ep_steps = plane_epoch_loader(epoch)
            if ep_steps == 0:
                log.warning("epoch %d: no full batch from the data plane", epoch)
                continue
        elif train_records is not None:
            ep_loader = image_loader(train_records, True, epoch)
            ep_steps = agree_steps(ep_loader.steps())
        else:
            ep_loader, ep_steps = loader, args.steps_per_epoch
        if args.use_mixup:
            ep_loader = MixupLoader(
                ep_loader, args.mixup_alpha,
                seed=4321 + 1000 * epoch + engine.env.global_rank)
        stats = engine.train_epoch(
            epoch, ep_loader, ep_steps, on_step=on_step,
            start_step=engine.start_step if epoch == engine.start_epoch else 0)
        if engine.env.is_rank0:
            log.info("epoch %d done: %.1f img/s (world=%d, global_batch=%d)",
                     epoch, stats["img_per_s"], engine.world_size, engine.global_batch)
        if args.eval_steps > 0:
            ev = engine.evaluate(eval_loader, args.eval_steps)
            if engine.env.is_rank0:
                log.info("epoch %d eval: loss=%.4f acc1=%.4f acc5=%.4f "
                         "(%d samples)", epoch, ev["loss"], ev["acc1"],
                         ev["acc5"], ev["samples"])
        engine.save_checkpoint(epoch)
    if engine.ckpt is not None:
        engine.ckpt.wait()
    report(TrainStatus.SUCCEED)
    edist.barrier(engine.device)
    if engine.env.is_rank0:
        log.info("training done in %.1fs", time.monotonic() - t_start)
    edist.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
