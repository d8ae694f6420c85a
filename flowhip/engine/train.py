"""Training driver: DDP over RCCL/xGMI, one process per GPU.

Behavioral parity with the reference `train.py:167-262` (optimizer/scheduler
recipes, grad clip 1.0, gamma-weighted sequence loss, VAL_FREQ=5000
checkpoint + validation cadence, freeze_bn after chairs) re-architected for
torch.distributed:

- launch with torchrun (one rank per GPU); --batch_size is the GLOBAL batch
  and is sharded across ranks (reference DataParallel semantics);
- gradients all-reduce through DDP/RCCL during backward (single 64MB bucket
  — see engine.distributed); loss/metrics are computed per-rank on local
  shards, mathematically equal to the reference's gathered-mean for mean
  losses with drop_last shards;
- rank 0 owns logging/checkpointing/validation;
- full train-state checkpoints (model/opt/sched/step/rng) enable true
  resume, which the reference lacks.
"""

import copy
import os

import numpy as np
import torch

if torch.cuda.is_available() and os.environ.get("FLOWHIP_MIOPEN_FIND", "0") == "1":
    # MIOpen benchmark/find mode, off by default: the A/B measured no
    # steady-state difference (bench10: 30.80 vs 30.74 pairs/s), and with
    # one process per GPU the concurrent find's user-db file locking only
    # adds warmup wall time and trace noise
    torch.backends.cudnn.benchmark = True
import torch.optim as optim

from .. import ops
from ..data.datasets import fetch_dataloader
from ..models import build_model
from ..utils.amp import NoOpGradScaler
from . import checkpoints, distributed
from . import evaluate as evaluate_mod
from .logger import Logger

VAL_FREQ = 5000


def count_parameters(model):
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def fetch_optimizer(args, model):
    """AdamW/Adam + OneCycleLR/StepLR (reference train.py:83-99)."""
    params = [p for p in model.parameters() if p.requires_grad]
    if args.optimizer.lower() == "adamw":
        optimizer = optim.AdamW(params, lr=args.lr, weight_decay=args.wdecay,
                                eps=args.epsilon)
    elif args.optimizer.lower() == "adam":
        optimizer = optim.Adam(params, lr=args.lr, weight_decay=args.wdecay,
                               eps=args.epsilon)
    else:
        raise NotImplementedError(f"{args.optimizer} optimizer is not implemented!")

    if args.scheduler.lower() == "cyclic":
        scheduler = optim.lr_scheduler.OneCycleLR(
            optimizer, args.lr, args.num_steps + 100,
            pct_start=0.05, cycle_momentum=False, anneal_strategy="linear")
    elif args.scheduler.lower() == "step":
        scheduler = optim.lr_scheduler.StepLR(
            optimizer, step_size=args.scheduler_step, gamma=0.5)
    else:
        raise NotImplementedError(f"{args.scheduler} scheduler is not implemented!")
    return optimizer, scheduler


def _make_profiler(out_dir):
    """Rank-0 in-loop torch.profiler: wait 1 / warmup 2 /
    active 3 steps, then a chrome trace + a self-time op table land in
    `out_dir`. One cycle only — profiling stays out of steady-state steps."""
    os.makedirs(out_dir, exist_ok=True)

    def _on_ready(prof):
        prof.export_chrome_trace(os.path.join(out_dir, "train_trace.json"))
        table = prof.key_averages().table(
            sort_by="self_cuda_time_total" if torch.cuda.is_available()
            else "self_cpu_time_total", row_limit=50)
        with open(os.path.join(out_dir, "train_ops.txt"), "w") as f:
            f.write(table)

    activities = [torch.profiler.ProfilerActivity.CPU]
    if torch.cuda.is_available():
        activities.append(torch.profiler.ProfilerActivity.CUDA)
    return torch.profiler.profile(
        activities=activities,
        schedule=torch.profiler.schedule(wait=1, warmup=2, active=3, repeat=1),
        on_trace_ready=_on_ready)


def apply_deterministic(args):
    """--deterministic: turn on the HIP kernels' deterministic mode, and
    have torch name (warn_only) every op of its own that has no
    deterministic implementation, e.g. --small's bilinear upflow8 backward."""
    if getattr(args, "deterministic", False):
        ops.set_deterministic(True)
        torch.use_deterministic_algorithms(True, warn_only=True)


def train(args):
    apply_deterministic(args)
    rank, world_size, device = distributed.init_distributed()

    torch.manual_seed(args.seed)
    np.random.seed(args.seed)

    model = build_model(args).to(device)
    model.train()
    if args.stage != "chairs":
        model.freeze_bn()

    if args.restore_ckpt is not None:
        checkpoints.load_weights(model, args.restore_ckpt, strict=False)

    ddp_model = distributed.wrap_ddp(model, device)

    assert args.batch_size % world_size == 0, \
        f"global batch {args.batch_size} must divide world size {world_size}"
    per_rank = args.batch_size // world_size

    loader_args = copy.copy(args)
    loader_args.batch_size = per_rank
    train_loader = fetch_dataloader(loader_args, distributed=world_size > 1,
                                    rank=rank, world_size=world_size)

    optimizer, scheduler = fetch_optimizer(args, model)
    scaler = NoOpGradScaler()  # bf16 autocast: no loss scaling needed

    total_steps = 0
    if getattr(args, "resume_full", None):
        total_steps = checkpoints.load_train_state(
            args.resume_full, model, optimizer, scheduler)

    logger = None
    if distributed.is_main():
        logger = Logger(scheduler, args)
        num_params = count_parameters(model)
        print("Parameter Count: %d" % num_params)
        logger.txt_file.write("Parameter Count: %d\n" % num_params)

    profiler = None
    if getattr(args, "profile_dir", None) and distributed.is_main():
        profiler = _make_profiler(args.profile_dir)
        profiler.__enter__()

    should_keep_training = True
    epoch = 0
    while should_keep_training:
        if world_size > 1 and train_loader.sampler is not None and \
                hasattr(train_loader.sampler, "set_epoch"):
            train_loader.sampler.set_epoch(epoch)
        epoch += 1

        for data_blob in train_loader:
            optimizer.zero_grad(set_to_none=True)
            image1, image2, flow, valid = [
                x.to(device, non_blocking=True) for x in data_blob]

            if args.add_noise:
                stdv = np.random.uniform(0.0, 5.0)
                image1 = (image1 + stdv * torch.randn_like(image1)).clamp(0.0, 255.0)
                image2 = (image2 + stdv * torch.randn_like(image2)).clamp(0.0, 255.0)

            flow_predictions = ddp_model(image1, image2, iters=args.iters)

            loss, metrics = ops.sequence_loss(flow_predictions, flow, valid,
                                              args.gamma)
            scaler.scale(loss).backward()

            scaler.unscale_(optimizer)
            torch.nn.utils.clip_grad_norm_(model.parameters(), args.clip)

            scaler.step(optimizer)
            scheduler.step()
            scaler.update()

            if profiler is not None:
                profiler.step()

            if logger is not None:
                logger.push(metrics, n_imgs=args.batch_size)

            if total_steps % VAL_FREQ == VAL_FREQ - 1:
                _validate_and_save(args, model, optimizer, scheduler,
                                   total_steps, logger)
                model.train()
                if args.stage != "chairs":
                    model.freeze_bn()

            total_steps += 1
            if total_steps > args.num_steps:
                should_keep_training = False
                break

    if profiler is not None:
        profiler.__exit__(None, None, None)

    if distributed.is_main():
        logger.close()
        PATH = "checkpoints/%s/final_model.pth" % args.name
        checkpoints.save_weights(model, PATH)
    else:
        PATH = None
    distributed.barrier()
    return PATH


def _validate_and_save(args, model, optimizer, scheduler, total_steps, logger):
    """Rank-0 checkpoint + validation; other ranks wait at the barrier."""
    if distributed.is_main():
        PATH = "checkpoints/%s/%d_%s.pth" % (args.name, total_steps + 1, args.name)
        checkpoints.save_weights(model, PATH)
        checkpoints.save_train_state(
            "checkpoints/%s/train_state.pth" % args.name,
            model, optimizer, scheduler, total_steps)

        results = {}
        for val_dataset in args.validation:
            if val_dataset == "chairs":
                iters = 12 if args.model == "raft_nc_sep" else 24
                results.update(evaluate_mod.validate_chairs(model, iters))
            elif val_dataset == "sintel":
                results.update(evaluate_mod.validate_sintel(model))
            elif val_dataset == "kitti":
                results.update(evaluate_mod.validate_kitti(model))
            elif val_dataset == "synthetic":
                results.update(evaluate_mod.validate_synthetic(model, args.iters))
        if logger is not None and results:
            logger.write_dict(results)
    distributed.barrier()
