"""Minimal trainer with the slice of pytorch_lightning.Trainer's behaviour the reference relies on
(reference train.py:160-180,244): one process per GPU, bf16 compute (the kernels' native flow), gradient-norm clipping
at `gradient_clip_val`, per-step LR scheduler, EMA inside training_step, periodic checkpoints with the
Lightning checkpoint keys (`state_dict`, `hyper_parameters`, `global_step`)."""
from __future__ import annotations

import datetime
import os
import sys
import time
from typing import Any, Dict, Iterable, Optional

import torch
import torch.distributed as dist

from .ddp import FlatGradAllReducer


def heartbeat(msg: str) -> None:
    """One line per rank on stderr at every stage of a multi-rank start (rendezvous, broadcast, first collective): when an N-rank
    launch stalls, the last line of each rank says where.  WJ_HEARTBEAT=0 silences it."""
    if os.environ.get("WJ_HEARTBEAT", "1") != "0" and "RANK" in os.environ:
        print(f"[rank {os.environ.get('RANK')}/{os.environ.get('WORLD_SIZE')} pid {os.getpid()} +{time.perf_counter() - _T0:.1f}s] {msg}",
              file=sys.stderr, flush=True)


_T0 = time.perf_counter()


def init_distributed() -> tuple:
    """(rank, local device index, world).  RCCL ("nccl" backend on ROCm) when launched by torch.distributed.run.

    WJ_DIST_BACKEND=gloo is a development aid: RCCL refuses two ranks on one device, gloo does not, so a 1-GPU box can run the
    N-rank launch end to end (ranks then share the visible GPUs round-robin; the compute path is unchanged)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    launched = "RANK" in os.environ and "WORLD_SIZE" in os.environ      # started by torch.distributed.run (any world size)
    backend = os.environ.get("WJ_DIST_BACKEND", "nccl")
    if backend != "nccl":
        local %= max(torch.cuda.device_count(), 1)
    if launched and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        torch.cuda.set_device(local)
        # a collective that does not complete inside the bound aborts the process (non-zero exit) instead of hanging the launch:
        # WJ_DIST_TIMEOUT_S, default 300 s (the first RCCL collective builds its rings / loads kernels: tens of seconds at most)
        timeout = datetime.timedelta(seconds=float(os.environ.get("WJ_DIST_TIMEOUT_S", "300")))
        os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "1")
        heartbeat(f"rendezvous at {os.environ['MASTER_ADDR']}:{os.environ['MASTER_PORT']} (backend {backend}, device {local})")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local), timeout=timeout)
        else:
            if os.environ["MASTER_ADDR"] in ("127.0.0.1", "localhost"):
                # gloo binds to the interface the HOSTNAME resolves to; container hostnames often do not resolve (or do after a resolver
                # time-out): a one-node run stays on the loopback interface
                os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
            dist.init_process_group(backend=backend, rank=rank, world_size=world, timeout=timeout)
        heartbeat("process group up")
    elif torch.cuda.is_available():
        torch.cuda.set_device(local)
    return rank, local, world


DP_PERSIST_CUS = 28     # resident persistent-GEMM workgroups per XCD in a data-parallel run: 4 CUs per XCD (32 in all) stay free


def init_persist_cus(world: int) -> int:
    """A persistent GEMM workgroup owns its CU (the whole register file, 150 KB of LDS): while one is resident on every CU an RCCL
    channel kernel cannot start.  With more than one rank the persistent kernels therefore leave DP_PERSIST_CUS..32 CUs per XCD to the
    gradient all-reduce that runs beside the backward (WJ_PERSIST_CUS set by the user wins).  Returns the value in effect."""
    from . import ops
    if world > 1 and "WJ_PERSIST_CUS" not in os.environ:
        ops.gemm_set_persist_cus(DP_PERSIST_CUS)
    return ops.gemm_set_persist_cus(0)


def check_accumulate(k) -> int:
    """accumulate_grad_batches as an integer >= 1; anything else (0, a float, a string, a bool) is a ValueError."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"accumulate_grad_batches must be an integer >= 1, not {k!r}")
    return k


def saved_accumulate(checkpoint: Dict[str, Any]) -> int:
    """k of the run that wrote `checkpoint`: the key is written only when k > 1, so a checkpoint without it (every k = 1 run, every
    checkpoint from before accumulation, the reference's) reads 1."""
    return int(checkpoint.get("accumulate_grad_batches", 1))


def refuse_unsupported_accumulation(model, k: int) -> None:
    """k > 1 on a module whose backward exposes no section hooks (the Denoiser stage: its own engine, whose backward_pair clears the
    gradient buffer unconditionally) is refused on the host, before any GPU work -- never trained as a silent k = 1."""
    if k > 1 and not hasattr(model, "_grads_ready_hook"):
        raise NotImplementedError(f"accumulate_grad_batches={k} with {type(model).__name__}: gradient accumulation covers the JEPA stage "
                                  "only; the Denoiser stage's backward clears the gradient buffer, so it would train on the last "
                                  "micro-batch alone.  Run it with accumulate_grad_batches=1")


class StepRunner:
    """One optimisation step in the reference's order.

    accumulate_grad_batches = k > 1 (Lightning's automatic optimisation): every call of step() still takes one loader batch -- one
    micro-batch: on_after_batch_transfer, training_step (with the teacher's EMA), (loss / k).backward() ADDED into the flat gradient
    buffer.  Only the k-th call of a window waits for the all-reduces, clips, updates, steps the scheduler and counts a global step;
    the ones before it issue no collective (their backward runs without the section hooks: DDP's no_sync).  `closed` says whether
    the last call closed its window, `window_loss()` is the mean loss of the last closed window, flush() closes an open one."""

    def __init__(self, model, gradient_clip_val: float = 5.0, enc_chunk: int = 3, accumulate_grad_batches: int = 1):
        self.model = model
        self.k = check_accumulate(accumulate_grad_batches)
        refuse_unsupported_accumulation(model, self.k)
        model._ensure_engine()
        self.reducer = FlatGradAllReducer(model, enc_chunk=enc_chunk)
        self.reducer.broadcast_parameters()
        if self.reducer.active:
            torch.cuda.synchronize()
            heartbeat("parameters broadcast from rank 0")
        init_persist_cus(dist.get_world_size() if dist.is_initialized() else 1)
        self._first_step_done = False
        self.sectioned = hasattr(model, "_grads_ready_hook")      # JEPA: bucketed all-reduces launched from the backward's hooks
        self._hook = None
        if self.sectioned:
            self._hook = self.reducer.hook if (self.reducer.active or self.reducer.emulate) else None
            model._grads_ready_hook = self._hook
        oc = model.configure_optimizers()
        self.optimizer = oc["optimizer"]
        self.scheduler = oc["lr_scheduler"]["scheduler"]
        self.optimizer.max_grad_norm = float(gradient_clip_val or 0.0)
        if self.sectioned and hasattr(self.optimizer, "overlap_next_forward"):
            # (JEPA only: its engine's forward knows where to wait.)  This loop reads parameters only through the engine / state_dict, which wait
            self.optimizer.overlap_next_forward = True
            self.optimizer.fuse_zero_grad = True        # (this loop never reads p.grad behind step())
        self.closed = True              # the last call of step() closed its window (k = 1: every call does)
        self.micro = 0                  # micro-batches gathered in the open window
        self._sum = self._mean = None   # running sum of the open window's detached losses / mean of the last closed one (device scalars)
        # the model reads k where Lightning keeps it: its trainer's attribute (training_step: dropout counter, monitored forward)
        from .jepa import accumulate_window
        seen = accumulate_window(model)
        if seen != self.k:
            if self.k > 1 and getattr(model.trainer, "accumulate_grad_batches", None) is None:
                model.trainer.accumulate_grad_batches = self.k          # (a model without a Trainer: its stand-in carries it)
            else:
                raise ValueError(f"the model's trainer has accumulate_grad_batches={seen}, this StepRunner {self.k}")
        if self.k > 1:
            model.accumulate_grads = True               # backward adds; the update (fuse_zero_grad) or zero_grad() clears

    def step(self, raw_batch, batch_idx: int) -> Dict[str, Any]:
        if self.k > 1:
            return self._micro_step(raw_batch, batch_idx)
        m = self.model
        batch = m.on_after_batch_transfer(raw_batch, 0)     # crops + normalise + bf16 on the device
        out = m.training_step(batch, batch_idx)             # forward + EMA of the teacher
        out["loss"].backward()                              # engine backward; buckets all-reduce as they complete
        if not self.sectioned:
            self.reducer.reduce_all()
        self._update()
        return out

    def _update(self) -> None:
        m = self.model
        self.reducer.wait()
        self.optimizer.step()                               # fused global-norm clip + AdamW over the flat buffers
        self.scheduler.step()
        m.global_step += 1
        if not self._first_step_done:
            self._first_step_done = True
            if self.reducer.active:
                torch.cuda.synchronize()
                heartbeat("first optimisation step (all gradient buckets reduced) done")

    def _micro_step(self, raw_batch, batch_idx: int) -> Dict[str, Any]:
        m, k, i = self.model, self.k, self.micro
        if int(batch_idx) % k != i:
            raise ValueError(f"batch_idx {batch_idx} is micro-batch {int(batch_idx) % k} of a window of {k}, but the open window holds {i}: "
                             "pass batch_idx = global_step * accumulate_grad_batches + micro-batch index")
        if i == 0:
            self.optimizer.zero_grad()                      # (nothing is launched behind an update that cleared the buffer itself)
        closing = i == k - 1
        batch = m.on_after_batch_transfer(raw_batch, 0)
        out = m.training_step(batch, batch_idx)             # forward + EMA of the teacher, per micro-batch as under pl.Trainer
        m._grads_ready_hook = self._hook if closing else None       # all-reduces start from the closing backward only, over the sum
        try:
            (out["loss"] / k).backward()
        finally:
            m._grads_ready_hook = self._hook
        loss = out["loss"].detach().float()
        self._sum = loss.clone() if i == 0 else self._sum + loss
        self.micro, self.closed = i + 1, False
        if closing:
            self._close()
        return out

    def _close(self) -> None:
        self._mean = self._sum / self.micro
        self._update()
        self.micro, self.closed, self._sum = 0, True, None

    def flush(self) -> bool:
        """Close an open window (the loader ended inside it): the update runs on what has been gathered, every part scaled 1 / k as it
        was (Lightning's last-batch rule).  No backward is left to carry the bucketed all-reduces: one over the whole buffer.  True if
        there was a window to close."""
        if self.k == 1 or self.micro == 0:
            return False
        self.reducer.reduce_all()
        self._close()
        return True

    def window_loss(self) -> Optional[torch.Tensor]:
        """Mean of the micro-batch losses of the last closed window (device scalar, no host sync); None before the first."""
        return self._mean


class CollapseError(RuntimeError):
    """A collapse monitor fell below its threshold (Trainer(min_pred_var=..., min_target_var=...))."""


class Trainer:
    def __init__(self, accelerator: str = "gpu", max_steps: int = 375000, max_epochs: int = -1, precision: str = "bf16-mixed",
                 devices: int = 1, gradient_clip_val: float = 5.0, gradient_clip_algorithm: str = "norm", strategy: str = "auto",
                 log_every_n_steps: int = 50, default_root_dir: Optional[str] = None, checkpoint_every_n_steps: int = 25000,
                 deterministic: bool = False, min_pred_var: float = 0.0, min_target_var: float = 0.0, accumulate_grad_batches: int = 1,
                 **unused):
        if accelerator not in ("gpu", "cuda", "auto"):
            raise ValueError("wavjepa_amd trains on MI355X GPUs only (accelerator='gpu'); there is no CPU path")
        if precision not in ("bf16-mixed", "bf16"):
            raise ValueError("the HIP path computes in bf16 with fp32 master weights (precision='bf16-mixed')")
        if gradient_clip_algorithm != "norm":
            raise ValueError("only norm clipping is implemented")
        # k loader batches (micro-batches) per optimiser step, Lightning's name and semantics (StepRunner); max_steps, log_every_n_steps,
        # checkpoint_every_n_steps and the schedules all count optimiser steps.  The model reads it here (training_step).
        self.accumulate_grad_batches = check_accumulate(accumulate_grad_batches)
        self.max_steps = int(max_steps)
        self.devices = int(devices)
        self.gradient_clip_val = gradient_clip_val
        self.log_every_n_steps = log_every_n_steps
        self.root = default_root_dir
        self.ckpt_every = checkpoint_every_n_steps
        # True: the engine's deterministic mode (bit-reproducible gradients and updates on one build and GPU model; the WJ_DETERMINISTIC
        # environment variable switches it on as well).  One GPU: the order of a multi-GPU gradient reduction is RCCL's.
        self.deterministic = bool(deterministic)
        # Collapse thresholds (data2vec 2.0: 0.01 / 0.1; 0 = no check) on the statistics of a monitored step (model.monitor_every):
        # checked at log steps, the one place this loop synchronises.
        self.min_pred_var, self.min_target_var = float(min_pred_var), float(min_target_var)
        self.rank, self.local_rank, self.world = init_distributed()
        self.logged: Dict[str, Any] = {}

    def log_dict(self, data: Dict[str, Any], **kw) -> None:
        self.logged = data          # kept on the device: no per-step host sync / scalar all-reduce

    def check_collapse(self, step: int, pred_var: float, target_var: float) -> None:
        """Raise CollapseError when a statistic of the monitored step `step` lies below its threshold."""
        for name, value, floor in (("pred_var", pred_var, self.min_pred_var), ("target_var", target_var, self.min_target_var)):
            if floor > 0.0 and not value >= floor:          # (a NaN statistic is a collapse too)
                raise CollapseError(f"{name} = {value:.6g} is below min_{name} = {floor:.6g} at step {step}: the run has collapsed "
                                    f"(pred_var {pred_var:.6g}, target_var {target_var:.6g})")

    def _monitor_values(self, model, seen) -> tuple:
        """(step, pred_var, target_var) of the last monitored step as host floats.  One rank: the step's own scalars.  Several: every
        rank's row count and per-column moments are gathered and merged (merge_moments), so all ranks hold the statistic of the
        global batch and raise together."""
        step, pv, tv = seen
        if not (dist.is_initialized() and self.world > 1):
            return step, float(pv), float(tv)
        from .ops import merge_moments
        eng = model._engine
        mine = torch.cat([eng.moments[2:3].double(), eng.moments_col.reshape(-1)])
        every = [torch.empty_like(mine) for _ in range(self.world)]
        dist.all_gather(every, mine)
        host = torch.stack(every).cpu().numpy()
        D = (host.shape[1] - 1) // 4
        stat = [merge_moments([(h[0], h[1 + 2 * q * D:1 + (2 * q + 1) * D], h[1 + (2 * q + 1) * D:1 + (2 * q + 2) * D]) for h in host])
                for q in (0, 1)]
        return step, stat[0], stat[1]

    def save_checkpoint(self, model, runner: StepRunner, path: str, versioned: bool = False) -> None:
        """`versioned`: never overwrite (Lightning's enable_version_counter): last.ckpt, last-v1.ckpt, ... -- the run directory is
        the reference's run-identity directory, where an earlier run's (or a reference run's) last.ckpt may already sit."""
        if self.rank != 0:
            return
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        if versioned and os.path.exists(path):
            stem, ext = os.path.splitext(path)
            v = 1
            while os.path.exists(f"{stem}-v{v}{ext}"):
                v += 1
            path = f"{stem}-v{v}{ext}"
        ck = {"state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
              "hyper_parameters": dict(model.hparams), "global_step": model.global_step,
              "optimizer": runner.optimizer.state_dict(), "lr_scheduler": runner.scheduler.state_dict()}
        if self.accumulate_grad_batches > 1:      # (k = 1: exactly the keys a checkpoint always had)
            ck["accumulate_grad_batches"] = self.accumulate_grad_batches
        torch.save(ck, path)

    def _after_step(self, model, runner: StepRunner, out, seen, t0: float, ckpt_path) -> tuple:
        """What fit() does behind an optimiser step: log, monitor, checkpoint -> (seen, t0).  `out`: the step's (the closing
        micro-batch's) outputs, None behind a flushed window; the logged loss is the window's mean at k > 1."""
        gs = model.global_step
        if out is not None and "pred_var" in out:
            seen = (gs - 1, out["pred_var"].detach(), out["target_var"].detach())
        mon = None
        if self.log_every_n_steps and gs % self.log_every_n_steps == 0:
            lt = (out["loss"].detach().float() if runner.k == 1 else runner.window_loss()).clone()
            if dist.is_initialized() and self.world > 1:
                dist.all_reduce(lt, op=dist.ReduceOp.AVG)   # the reference logs with sync_dist=True (jepa.py:328): the rank mean
            if seen is not None:
                mon, seen = self._monitor_values(model, seen), None
        if self.log_every_n_steps and gs % self.log_every_n_steps == 0 and self.rank == 0:
            loss = float(lt)                      # the only host sync, every n steps
            dt = time.time() - t0
            ema = f"  ema {model._get_ema_decay():.6f}" if hasattr(model, "_get_ema_decay") else ""
            var = f"  pred_var {mon[1]:.5f}  target_var {mon[2]:.5f} (step {mon[0]})" if mon is not None else ""
            kept = getattr(model, "last_kept", None)          # LayerDrop: layers of the student / the predictor that ran in the last forward
            if kept is not None:
                var += f"  kept {len(kept['enc'])}/{len(kept['dec'])}"
            print(f"step {gs}  loss {loss:.5f}  lr {runner.scheduler.get_last_lr()[0]:.3e}{ema}{var}  "
                  f"{dt / self.log_every_n_steps * 1000:.1f} ms/step", flush=True)
            t0 = time.time()
        if mon is not None:
            self.check_collapse(*mon)
        if self.root and self.ckpt_every and gs % self.ckpt_every == 0:
            self.save_checkpoint(model, runner, os.path.join(self.root, f"step={gs}.ckpt"), versioned=ckpt_path is None)
        return seen, t0

    def fit(self, model, datamodule=None, train_dataloaders: Optional[Iterable] = None, ckpt_path: Optional[str] = None):
        k = self.accumulate_grad_batches
        refuse_unsupported_accumulation(model, k)           # (the Denoiser stage: on the host, before any GPU work)
        dev = torch.device("cuda", self.local_rank)
        model.to(dev)
        model.trainer = self
        model.train()
        runner = StepRunner(model, self.gradient_clip_val) if k == 1 else StepRunner(model, self.gradient_clip_val, accumulate_grad_batches=k)
        if self.deterministic:
            model._ensure_engine().deterministic = True       # before the first step
        if ckpt_path:
            ck = torch.load(ckpt_path, map_location="cpu", weights_only=False)
            model.load_state_dict(ck["state_dict"])
            model.global_step = int(ck.get("global_step", 0))
            saved_k = saved_accumulate(ck)
            if saved_k != k and self.rank == 0:
                print(f"resuming a run saved with accumulate_grad_batches={saved_k} at accumulate_grad_batches={k}: the dropout mask "
                      "sequence (a function of global_step * k + micro-batch) differs from the saved run's", flush=True)
            # dropout masks are a function of (dropout_seed, global_step): a resumed run continues the saved run's mask sequence
            seed = (ck.get("hyper_parameters") or {}).get("dropout_seed")
            if seed is not None and hasattr(model, "dropout_seed"):
                model.dropout_seed = int(seed)
            if "optimizer" in ck:
                runner.optimizer.load_state_dict(ck["optimizer"])
            if "lr_scheduler" in ck:
                runner.scheduler.load_state_dict(ck["lr_scheduler"])
        loader = train_dataloaders if train_dataloaders is not None else datamodule.train_dataloader()
        t0 = time.time()
        batches = 0
        seen = None         # (step, pred_var, target_var) of the last monitored step since the last log step, still on the device
        for batch in loader:
            if model.global_step >= self.max_steps:
                break
            # one loader batch is one micro-batch of a window of k (k = 1: batch_idx = global_step, every call closes its window)
            out = runner.step(batch, model.global_step * k + runner.micro)
            batches += 1
            if runner.closed:           # logging, monitors and checkpoints: at optimiser steps only
                seen, t0 = self._after_step(model, runner, out, seen, t0, ckpt_path)
        if runner.flush():              # the loader ended inside a window: the update runs on what was gathered
            self._after_step(model, runner, None, seen, t0, ckpt_path)
        if self.root:
            self.save_checkpoint(model, runner, os.path.join(self.root, "last.ckpt"), versioned=ckpt_path is None)
        eng = getattr(model, "_engine", None)
        if eng is not None and hasattr(eng, "wait_optimizer"):
            # the last step's update of the transformer stacks may still run on the side stream (overlap_next_forward): whatever the caller
            # does with the model next (export, .cpu(), a submodule's state_dict) is ordered behind it on the compute stream -- no host sync
            eng.wait_optimizer()
        if self.rank == 0 and self.log_every_n_steps:
            micro = f" ({batches} micro-batches, accumulate_grad_batches={k})" if k > 1 else ""
            print(f"done: {model.global_step} steps{micro}, peak HBM {torch.cuda.max_memory_allocated(dev) / 2**30:.1f} GiB allocated, "
                  f"{torch.cuda.max_memory_reserved(dev) / 2**30:.1f} GiB reserved", flush=True)
        return runner
