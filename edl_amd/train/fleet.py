"""paddle_edl-compatible training API facade.

The reference's user scripts drive Paddle Fleet
(train_with_fleet.py:367-381: fleet.init(role), DistributedStrategy,
fleet.distributed_optimizer(...).minimize, fleet.save/load_check_point with
TrainStatus). This module keeps those NAMES working on top of the MI355X
engine so a paddle_edl user can port a script mechanically:

    from edl_amd.train import fleet
    fleet.init()
    engine = fleet.distributed_engine(model, lr=0.1)   # torch-native core
    ts = fleet.load_check_point(engine, path)
    for epoch in range(ts.next(), epochs): ...
    fleet.save_check_point(engine, TrainStatus(epoch), path)
"""
from dataclasses import dataclass, field

import torch

from . import dist as edist
from .checkpoint import CheckpointManager
from .env import TrainerEnv


@dataclass
class DistributedStrategy:
    """Knob parity with the reference's strategy/flags:
    values are recorded; the engine applies the equivalents."""

    nccl_comm_num: int = 1                   # RCCL communicators
    use_hierarchical_allreduce: bool = False  # moot intra-node over xGMI
    fuse_all_reduce_ops: bool = True          # always on: flat bucket views
    fuse_all_reduce_ops_mb: int = 25          # bucket size
    use_amp: bool = True                      # bf16 autocast
    use_dgc: bool = False                     # optional sparse allreduce
    # Paddle's keys: rampup_begin_step, rampup_step, sparsity (a list).
    # Non-empty (with use_dgc) = DGC with momentum correction.
    dgc_configs: dict = field(default_factory=dict)
    use_recompute: bool = False
    # global-norm gradient clipping (Paddle: GradientClipByGlobalNorm);
    # None = off. Refused together with use_dgc.
    clip_grad_norm: float = None
    # LARS (Paddle: strategy.lars + lars_configs). Paddle's keys:
    # lars_coeff, lars_weight_decay, epsilon, exclude_from_weight_decay (a
    # list of parameter-name substrings). Refused together with use_dgc.
    lars: bool = False
    lars_configs: dict = field(default_factory=dict)
    extra: dict = field(default_factory=dict)


class TrainStatus:
    """Epoch cursor (reference doc/fault_tolerance.md:55-62)."""

    def __init__(self, epoch_no=-1):
        self.epoch_no = epoch_no

    def next(self):
        return self.epoch_no + 1

    def __eq__(self, o):
        return isinstance(o, TrainStatus) and o.epoch_no == self.epoch_no


_state = {"env": None, "device": None}


def init(role=None, strategy=None):
    """fleet.init: join the RCCL/gloo world from the launcher env."""
    env, device = edist.init_from_env()
    _state["env"], _state["device"] = env, device
    return env


def worker_index():
    return (_state["env"] or TrainerEnv()).global_rank


def worker_num():
    return (_state["env"] or TrainerEnv()).world_size


def is_first_worker():
    return worker_index() == 0


def distributed_engine(model_name="resnet50_vd", strategy=None, **kwargs):
    """Build the TrainerEngine (our fleet.distributed_optimizer analog)."""
    from .engine import TrainerEngine

    strategy = strategy or DistributedStrategy()
    kwargs.setdefault("bucket_mb", strategy.fuse_all_reduce_ops_mb)
    kwargs.setdefault("dtype", "bf16" if strategy.use_amp and
                      torch.cuda.is_available() else "fp32")
    kwargs.setdefault("dgc", strategy.use_dgc)
    if strategy.use_dgc and strategy.dgc_configs:
        cfg = dict(strategy.dgc_configs)
        unknown = set(cfg) - {"rampup_begin_step", "rampup_step", "sparsity"}
        if unknown:
            raise ValueError("dgc_configs: unknown keys %s" % sorted(unknown))
        kwargs.setdefault("dgc_momentum_correction", True)
        kwargs.setdefault("dgc_rampup", cfg.get("rampup_begin_step", 0))
        kwargs.setdefault("dgc_rampup_step", cfg.get("rampup_step", 1))
        kwargs.setdefault("dgc_sparsity", cfg.get("sparsity", [0.999]))
    if strategy.lars:
        cfg = dict(strategy.lars_configs)
        unknown = set(cfg) - {"lars_coeff", "lars_weight_decay", "epsilon",
                              "exclude_from_weight_decay"}
        if unknown:
            raise ValueError("lars_configs: unknown keys %s" % sorted(unknown))
        kwargs.setdefault("optimizer", "lars")
        kwargs.setdefault("lars_coeff", cfg.get("lars_coeff", 0.001))
        kwargs.setdefault("weight_decay", cfg.get("lars_weight_decay", 0.0005))
        kwargs.setdefault("lars_eps", cfg.get("epsilon", 0.0))
        kwargs.setdefault("lars_exclude",
                          list(cfg.get("exclude_from_weight_decay", ())))
    kwargs.setdefault("recompute", strategy.use_recompute)
    kwargs.setdefault("clip_grad_norm", strategy.clip_grad_norm)
    eng = TrainerEngine(model=model_name, **kwargs)
    eng.setup(_state["env"])
    return eng


def save_check_point(engine, train_status, path, fs=None):
    """Rank-0 versioned checkpoint (reference train_with_fleet.py:562-570)."""
    if engine.env is not None and not engine.env.is_rank0:
        return None
    cm = engine.ckpt if (engine.ckpt and engine.ckpt.path == path) else \
        CheckpointManager(path)
    return cm.save(engine.model.state_dict(),
                   {"epoch_no": train_status.epoch_no,
                    "global_step": engine.global_step},
                   optimizer_state=engine.opt.state_dict())


def load_check_point(engine, path, fs=None, trainer_id=None):
    """-> TrainStatus or None (reference train_with_fleet.py:427-431)."""
    cm = CheckpointManager(path)
    got = cm.load()
    if got is None:
        return None
    model_state, opt_state, ts = got
    engine.model.load_state_dict(model_state)
    if opt_state is not None:
        try:
            engine.opt.load_state_dict(opt_state)
        except (KeyError, ValueError):
            pass
    engine.global_step = int(ts.get("global_step", 0))
    return TrainStatus(int(ts.get("epoch_no", -1)))
