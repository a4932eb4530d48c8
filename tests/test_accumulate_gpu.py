"""Gradient accumulation (accumulate_grad_batches = k) through the engine, the autograd bridge, StepRunner, Trainer and the launcher
(GPU only).

A small deep model -- 3 student layers of width 128 (so the student's weight-gradient group of 2 is crossed), 3 predictor layers of width
64 -- on 2 to 4 clips of 2.01 s with the golden AudioSet masks, in deterministic mode unless a test says otherwise.  Every test prints
its figures before it asserts."""
import importlib.util
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import jepa_oracle as J
from tests import accumulate_reference as A
from tests import launch
from tests.test_conv_layernorm_gpu import build_ln
from tests.test_jepa_gpu import SMALL_SPEC, build, dev, group_of, masks, oracle_kw, rel
from tests.test_prenorm_gpu import build_pre, clips
from tests.test_recompute_gpu import bits, differing

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACC = dict(conv_spec=SMALL_SPEC, d_enc=128, h_enc=2, l_enc=3, d_dec=64, h_dec=2, l_dec=3, top_k=2)
BUILDERS = dict(post=build, pre=build_pre, layer_norm=build_ln)


def fresh(form="post", deterministic=True, **kw):
    m, P = BUILDERS[form](ACC, **kw)
    m._ensure_engine().deterministic = deterministic
    m.trainer.max_steps = 20
    return m, P


def window(golden_dir, k):
    """k micro-batches with different clips and different mask rows; the second has 3 clips between two of 4 (the arena is rebuilt
    inside the window)."""
    ctx, tgt, vis = masks(golden_dir, 8)
    out = []
    for j in range(k):
        n = 3 if j == 1 else 4
        sl = slice(2 * j, 2 * j + n)
        out.append((clips(n, seed=500 + j), ctx[sl], tgt[sl], vis[sl]))
    return out


def accumulate(m, batches, k):
    """the ordinary torch loop under accumulate_grads: zero_grad(), k times (loss / k).backward() -> (gradient buffer, losses)"""
    m.accumulate_grads = True
    opt = getattr(m, "_test_opt", None) or m.configure_optimizers()["optimizer"]
    m._test_opt = opt
    opt.zero_grad()
    losses = []
    for b in batches:
        out = m(*b)
        (out["loss"] / k).backward()
        losses.append(out["loss"].detach().float().reshape(1).clone())
    torch.cuda.synchronize()
    return m._flat.g32.clone(), torch.cat(losses)


def group_errors(m, got, want):
    num, den = {}, {}
    for name, sl in m._flat.by_name.items():
        a, b = got[sl.offset:sl.offset + sl.numel].double(), want[sl.offset:sl.offset + sl.numel].double()
        g = group_of(name)
        num[g] = num.get(g, 0.0) + float((a - b).pow(2).sum())
        den[g] = den.get(g, 0.0) + float(b.pow(2).sum())
    return {g: (num[g] / (den[g] + 1e-300)) ** 0.5 for g in num if den[g] > 0}


def prepared(m):
    """StepRunner.step on ready crops: the crop step of on_after_batch_transfer draws random offsets and shuffles the rows"""
    m.on_after_batch_transfer = lambda batch, dataloader_idx=0: batch
    return m


def runner(m, k=None, **kw):
    from wavjepa_amd.trainer import StepRunner
    prepared(m)
    run = StepRunner(m, 5.0, **kw) if k is None else StepRunner(m, 5.0, accumulate_grad_batches=k, **kw)
    return run


def state_bits(m):
    m._engine.wait_optimizer()
    torch.cuda.synchronize()
    f = m._flat
    return dict(parameters=bits(f.p32), teacher=bits(f.t32), adam_m=bits(f.adam_m), adam_v=bits(f.adam_v))


# ------------------------------------------------------------------------------------------------------------ 1. accumulation sums
@pytest.mark.parametrize("form,k", [("post", 3), ("pre", 2), ("layer_norm", 2)])
def test_accumulated_gradient_is_the_sum_of_the_single_backwards(golden_dir, form, k):
    batches = window(golden_dir, k)
    m, _ = fresh(form)
    got, losses = accumulate(m, batches, k)
    # reference: single backwards of a fresh identical model at the same scale 1 / k (the scale enters dpreds before its bf16 rounding),
    # summed in fp64
    ref, _ = fresh(form)
    assert ref.accumulate_grads is False
    total, singles = torch.zeros_like(got, dtype=torch.float64), []
    for b in batches:
        out = ref(*b)
        (out["loss"] / k).backward()
        torch.cuda.synchronize()
        singles.append(ref._flat.g32.clone())
        total += singles[-1].double()
    errs = group_errors(m, got, total)
    print(form, "k =", k, "accumulated against the fp64 sum of single backwards, relative L2 per group:", errs,
          "losses", losses.tolist(), flush=True)
    assert {"encoder", "decoder", "extract_audio", "mask_token", "feature_norms"} <= set(errs)
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    for g, e in errs.items():
        assert e <= 1e-5, (g, e)
    # every parameter's gradient took part: none of them is the last micro-batch's alone
    last = group_errors(m, got, singles[-1].double())
    print(form, "distance of the accumulated gradient from the last micro-batch's:", last, flush=True)
    assert all(e > 1e-2 for e in last.values()), last
    # without the flag the same loop leaves the last micro-batch's gradient: the behaviour that must not change (and zero_grad() the no-op)
    again = ref.configure_optimizers()["optimizer"]
    again.zero_grad()
    assert bool(torch.equal(bits(ref._flat.g32), bits(singles[-1])))
    assert float(singles[-1].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ 2. halves equal the whole
def test_two_halves_equal_the_whole_batch(golden_dir):
    ctx, tgt, vis = masks(golden_dir, 2)
    audio = clips(4, seed=520)
    halves = [(audio[:2], ctx, tgt, vis), (audio[2:], ctx, tgt, vis)]
    whole = (audio, torch.cat([ctx, ctx]), torch.cat([tgt, tgt]), torch.cat([vis, vis]))
    m, _ = fresh()
    got, losses = accumulate(m, halves, 2)
    ref, _ = fresh()
    out = ref(*whole)
    out["loss"].backward()
    torch.cuda.synchronize()
    want, l_whole, l_mean = ref._flat.g32, float(out["loss"].detach()), float(losses.double().mean())
    errs = {name: rel(got[s.offset:s.offset + s.numel], want[s.offset:s.offset + s.numel]) for name, s in m._flat.by_name.items()}
    worst = max(errs, key=errs.get)
    print("mean of the halves' losses / the whole's:", l_mean, l_whole, "worst parameter:", worst, errs[worst], flush=True)
    assert abs(l_mean - l_whole) <= 1e-5 * abs(l_whole), (l_mean, l_whole)
    for name, e in errs.items():
        assert e <= 2e-3, (name, e)


# ------------------------------------------------------------------------------------------------------------ 3. reproducible
def test_window_is_bit_reproducible(golden_dir):
    batches = window(golden_dir, 3)
    runs = []
    for _ in range(2):
        m, _ = fresh(warmup_steps=2)
        g, losses = accumulate(m, batches, 3)
        m._test_opt.max_grad_norm = 5.0
        m._test_opt.step()
        runs.append(dict(g32=bits(g), losses=bits(losses), **state_bits(m)))
    for name in runs[0]:
        print(name, "bit-equal:", bool(torch.equal(runs[0][name], runs[1][name])), flush=True)
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), name
    assert int(runs[0]["adam_m"].ne(0).sum()) > 0


# ------------------------------------------------------------------------------------------------------------ 4. trajectory
def test_training_trajectory_at_k_2_vs_reference(golden_dir):
    """Four optimiser steps at k = 2 through StepRunner against tests/accumulate_reference.py in the oracle's bf16 mode, with the
    constants of test_training_trajectory_vs_oracle."""
    m, P = fresh(warmup_steps=3)
    P = {k: v.detach().clone() for k, v in P.items()}
    m.hparams["ema_decay"], m.hparams["ema_end_decay"], m.ema_end_step = 0.9, 0.99, 10
    run = runner(m, 2)
    ctx, tgt, vis = masks(golden_dir, 6)
    state, worst, open_window = {}, 0.0, []
    for i in range(8):
        sl = slice(2 * (i % 3), 2 * (i % 3) + 2)
        audio = clips(2, seed=100 + i % 3)
        out = run.step((audio, ctx[sl], tgt[sl], vis[sl]), i)
        open_window.append(((audio, ctx[sl].to(dev()), tgt[sl].to(dev()), vis[sl].to(dev())), float(out["loss"].detach())))
        assert run.closed == (i % 2 == 1) and m.global_step == (i + 1) // 2
        if not run.closed:
            continue
        step = i // 2
        r = A.train_window(P, state, step, [b for b, _ in open_window], mode="bf16", warmup=3, total_steps=20, ema=(0.9, 0.99, 10),
                           **oracle_kw(ACC))
        gn = float(run.optimizer.grad_norm())
        mean = float(run.window_loss())
        print("step", step, "losses hip / reference:", [l for _, l in open_window], r["losses"], "grad norm:", gn, r["grad_norm"], flush=True)
        for (_, lo), lr_ in zip(open_window, r["losses"]):
            worst = max(worst, abs(lo - lr_) / abs(lr_))
        assert abs(gn - r["grad_norm"]) < 3e-2 * r["grad_norm"], (step, gn, r["grad_norm"])
        assert abs(mean - sum(l for _, l in open_window) / 2) <= 1e-6 * abs(mean)
        open_window = []
    print("worst relative loss deviation over 8 micro-batches:", worst, flush=True)
    assert worst < 2e-3
    assert m.global_step == 4 and run.optimizer._t == 4 and run.scheduler.last_epoch == 4 and run.micro == 0 and not run.flush()
    sd = m.state_dict()
    for k in ("encoder.layers.1.linear1.weight", "teacher_encoder.layers.1.linear1.weight", "extract_audio.cnn.2.0.weight"):
        print(k, rel(sd[k], P[k]), flush=True)
        assert rel(sd[k], P[k]) < 2e-3, k


# ------------------------------------------------------------------------------------------------------------ 5. k = 1 is the parent
def launch_trace():
    spec = importlib.util.spec_from_file_location("wj_launch_trace", os.path.join(ROOT, "tools", "launch_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_k_1_issues_and_computes_what_it_always_did(golden_dir):
    LT = launch_trace()
    ctx, tgt, vis = masks(golden_dir, 4)
    batches = [(clips(4, seed=700 + i), ctx, tgt, vis) for i in range(3)]
    ends, traces = [], []
    for explicit in (False, True):
        m, _ = fresh(warmup_steps=2)
        run = runner(m, 1 if explicit else None)
        assert run.k == 1 and m.accumulate_grads is False and not hasattr(m.trainer, "accumulate_grad_batches")
        run.step(batches[0], 0)
        with LT.Trace(m._engine) as tr:
            run.step(batches[1], 1)
        run.step(batches[2], 2)
        assert run.closed and run.micro == 0 and m.global_step == 3
        ends.append(state_bits(m))
        traces.append(tr.lines)
    print("events of a traced k = 1 step:", len(traces[0]), len(traces[1]), flush=True)
    assert traces[0] == traces[1] and len(traces[0]) > 50
    for name in ends[0]:
        assert torch.equal(ends[0][name], ends[1][name]), name


def test_fused_zero_grad_clears_behind_the_closing_update_only(golden_dir):
    ctx, tgt, vis = masks(golden_dir, 4)
    m, _ = fresh(warmup_steps=2)
    run = runner(m, 2)
    assert run.optimizer.fuse_zero_grad and m.accumulate_grads is True and m.trainer.accumulate_grad_batches == 2
    seen = []
    for i in range(4):
        run.step((clips(4, seed=710 + i), ctx, tgt, vis), i)
        m._engine.wait_optimizer()
        torch.cuda.synchronize()
        seen.append((run.closed, float(m._flat.g32.abs().max()), bool(m._flat.g_clean), m.global_step))
    print("(closed, max |g32|, g_clean, global_step) behind each micro-batch:", seen, flush=True)
    assert [s[0] for s in seen] == [False, True, False, True] and [s[3] for s in seen] == [0, 1, 1, 2]
    assert seen[0][1] > 0 and seen[2][1] > 0 and seen[1][1] == 0.0 and seen[3][1] == 0.0
    assert [s[2] for s in seen] == [False, True, False, True]
    with pytest.raises(ValueError, match="batch_idx"):
        run.step((clips(4, seed=710), ctx, tgt, vis), 1)        # the window is closed: micro-batch 1 of 2 does not open one


# ------------------------------------------------------------------------------------------------------------ 6. the loader ends inside a window
def test_loader_that_ends_inside_a_window(golden_dir):
    from wavjepa_amd.trainer import Trainer
    ctx, tgt, vis = masks(golden_dir, 4)
    batches = [(clips(4, seed=720 + i), ctx, tgt, vis) for i in range(5)]
    # (a) Trainer.fit over a loader of five batches
    ma, _ = fresh(warmup_steps=2)
    prepared(ma)
    ra = Trainer(max_steps=20, accumulate_grad_batches=2, log_every_n_steps=0, deterministic=True).fit(ma, train_dataloaders=iter(batches))
    # (b) by hand: two windows through the runner, then the fifth batch as the ordinary torch loop writes it, scaled 1 / 2
    mb, _ = fresh(warmup_steps=2)
    rb = runner(mb, 2)
    for i in range(4):
        rb.step(batches[i], i)
    assert mb.global_step == 2 and rb.closed
    rb.optimizer.zero_grad()
    out = mb.training_step(batches[4], 4)
    (out["loss"] / 2).backward()
    rb.optimizer.step()
    rb.scheduler.step()
    mb.global_step += 1
    print("global_step / optimiser steps / scheduler steps after five batches at k = 2:", ma.global_step, ra.optimizer._t,
          ra.scheduler.last_epoch, flush=True)
    assert ma.global_step == 3 and ra.optimizer._t == 3 and ra.scheduler.last_epoch == 3 and ra.micro == 0 and ra.closed
    a, b = state_bits(ma), state_bits(mb)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    # the part kept its scale 1 / 2: the last update's gradient norm is half of what the batch gives at scale 1 from the same state
    mc, _ = fresh(warmup_steps=2)
    rc = runner(mc, 2)
    for i in range(4):
        rc.step(batches[i], i)
    out = mc.training_step(batches[4], 4)
    mc.accumulate_grads = False
    out["loss"].backward()
    torch.cuda.synchronize()
    full = float(mc._flat.g32.double().norm())
    half = float(ra.optimizer.grad_norm())
    print("gradient norm of the flushed window / of the same batch at scale 1:", half, full, flush=True)
    assert abs(half - full / 2) <= 1e-5 * full


# ------------------------------------------------------------------------------------------------------------ 7. options ride along
def test_recomputation_at_k_2_is_bit_equal(golden_dir):
    batches = window(golden_dir, 2)
    on, _ = fresh(use_gradient_checkpointing=True)
    off, _ = fresh()
    assert on._engine.recompute and not off._engine.recompute
    g_on, l_on = accumulate(on, batches, 2)
    g_off, l_off = accumulate(off, batches, 2)
    bad = differing(on, g_on, g_off)
    print("recompute on / off at k = 2: gradient tensors that differ:", bad[:8], len(bad), flush=True)
    assert torch.equal(bits(l_on), bits(l_off)) and not bad and torch.equal(bits(g_on), bits(g_off)) and float(g_off.abs().max()) > 0


def drop_model(seed=7):
    from tests.test_dropout_gpu import build_drop
    m, _ = build_drop(0.1, 0.1, seed=seed, warmup_steps=2)
    m._ensure_engine().deterministic = True
    m.trainer.max_steps = 20
    return m


def test_dropout_micro_batches_draw_different_masks(golden_dir):
    ctx, tgt, vis = masks(golden_dir, 4)
    batch = (clips(4, seed=730), ctx, tgt, vis)
    m = drop_model()
    m.hparams["ema_decay"] = m.hparams["ema_end_decay"] = 1.0          # the teacher stands still: the same data gives the same targets
    run = runner(m, 2)
    calls, losses = [], []
    for i in range(4):
        out = run.step(batch, i)
        calls.append(m._engine.drop_call)
        losses.append(int(bits(out["loss"].detach().float().reshape(1))))
    print("drop_call of the micro-batches of two steps:", calls, "loss bits:", losses, flush=True)
    assert calls == [0, 1, 2, 3]
    assert losses[0] != losses[1] and losses[2] != losses[3]             # the same data and parameters, other masks
    m.dropout_call = 7                                                   # an explicit counter wins: one mask set for both
    pair = []
    for i in range(4, 6):
        out = run.step(batch, i)
        assert m._engine.drop_call == 7
        pair.append(int(bits(out["loss"].detach().float().reshape(1))))
    print("loss bits with dropout_call = 7:", pair, flush=True)
    assert pair[0] == pair[1]


def test_dropout_checkpoint_resume_at_k_2_is_bit_equal(tmp_path):
    from wavjepa_amd.data import SyntheticAudioSource
    from wavjepa_amd.masking import TimeInverseBlockMasker
    from wavjepa_amd.trainer import Trainer

    def source():
        return SyntheticAudioSource(TimeInverseBlockMasker(4, 0.65, 10, 0.25, 10, 0.1), batch_size=2, samples_per_audio=2, n_tokens=200,
                                    seconds=3.0, seed=11, n_mask_sets=4, device=dev())
    mask_sets = source().mask_sets

    def loader(skip):
        src = source()
        src.mask_sets = mask_sets
        for i in range(8):
            b = src.next_batch()
            torch.manual_seed(1000 + i)        # the crop offsets of on_after_batch_transfer come from the global generator
            if i >= skip:
                yield b

    def run(seed, root, ckpt=None, skip=0):
        m = drop_model(seed)
        tr = Trainer(max_steps=4, default_root_dir=str(root), checkpoint_every_n_steps=2, log_every_n_steps=0, deterministic=True,
                     accumulate_grad_batches=2)
        return m, tr.fit(m, train_dataloaders=loader(skip), ckpt_path=ckpt)
    ma, ra = run(7, tmp_path / "a")
    ck = tmp_path / "a" / "step=2.ckpt"
    saved = torch.load(ck, map_location="cpu", weights_only=False)
    assert saved["global_step"] == 2 and saved["accumulate_grad_batches"] == 2 and saved["optimizer"]["step"] == 2
    mb, rb = run(8, tmp_path / "b", ckpt=str(ck), skip=4)
    assert ma.global_step == mb.global_step == 4 and ra.optimizer._t == rb.optimizer._t == 4
    a, b = state_bits(ma), state_bits(mb)
    for name in a:
        print(name, "bit-equal after the resume:", bool(torch.equal(a[name], b[name])), flush=True)
    for name in a:
        assert torch.equal(a[name], b[name]), name


# ------------------------------------------------------------------------------------------------------------ 8. monitor
def test_only_the_closing_micro_batch_is_monitored(golden_dir):
    ctx, tgt, vis = masks(golden_dir, 4)
    m, _ = fresh(warmup_steps=2)
    m.monitor_every = 1
    run = runner(m, 2)
    has = []
    for i in range(4):
        out = run.step((clips(4, seed=740 + i), ctx, tgt, vis), i)
        has.append(("pred_var" in out, "target_var" in out))
        if has[-1][0]:
            assert float(out["pred_var"]) > 0 and float(out["target_var"]) > 0
    print("pred_var / target_var in the micro-batches' outputs:", has, flush=True)
    assert has == [(False, False), (True, True), (False, False), (True, True)]


# ------------------------------------------------------------------------------------------------------------ 9. memory
def peak_of(k, batches):
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    m, _ = fresh(warmup_steps=2)
    run = runner(m, k)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for i, b in enumerate(batches):
        run.step(b, i)
    m._engine.wait_optimizer()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    # the mask plan of one micro-batch, every tensor in whole 512-byte blocks of the caching allocator
    plan = sum(-(-t.numel() * t.element_size() // 512) * 512 for t in vars(m._engine.plan).values() if torch.is_tensor(t))
    return peak, plan


def test_window_peaks_at_the_micro_batch_size(golden_dir):
    ctx, tgt, vis = masks(golden_dir, 6)
    audio = clips(6, seed=750)
    micro = [(audio[2 * j:2 * j + 2], ctx[2 * j:2 * j + 2], tgt[2 * j:2 * j + 2], vis[2 * j:2 * j + 2]) for j in range(3)]
    p_window, plan = peak_of(3, micro)
    p_single, _ = peak_of(1, micro[:1])
    p_whole, _ = peak_of(1, [(audio, ctx, tgt, vis)])
    # what a window keeps beyond one step, from the shapes: per micro-batch the scaled loss, its upstream gradient, the detached loss and
    # the running sum -- fp32 scalars, each one 512-byte block of the caching allocator -- plus the window's mean; and the mask plan of
    # the previous micro-batch, which the engine holds until the next forward has built its own
    scalars, plans = (4 * 3 + 1) * 512, plan
    print("peak bytes: window of 3 x 2 clips", p_window, "one step of 2 clips", p_single, "one step of 6 clips", p_whole,
          "allowance: scalars", scalars, "mask plan", plans, flush=True)
    assert p_single <= p_window <= p_single + scalars + plans
    assert p_window < p_whole


# ------------------------------------------------------------------------------------------------------------ 10. two ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, golden_dir, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), GLOO_SOCKET_IFNAME="lo")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path[:0] = [os.path.dirname(here), here, os.path.join(here, "golden")]
        from tests import test_accumulate_gpu as T
        from wavjepa_amd.ddp import section_ranges

        def model(shift):
            m, _ = T.fresh(warmup_steps=2)
            if shift:
                with torch.no_grad():
                    for p in m.parameters():
                        p.add_(0.01)
            m.hparams["ema_decay"], m.hparams["ema_end_decay"], m.ema_end_step = 0.9, 0.99, 10
            return m
        m = model(rank == 1)
        run = T.runner(m, 2)
        assert run.reducer.active and run.sectioned and m._grads_ready_hook is not None
        flat = m._flat
        fx = dict(np.load(os.path.join(golden_dir, "masks.npz")))

        def batch(i):          # ranks and micro-batches see different clips and masks
            lo = 2 * ((2 * i + rank) % 3)
            return (T.clips(2, seed=300 + 2 * i + rank),) + tuple(torch.from_numpy(fx[k][lo:lo + 2]) for k in ("as_ctx", "as_tgt", "as_vis"))
        # this rank's LOCAL accumulated gradient of the first window, on an un-hooked replica of the broadcast state
        twin = model(False)
        twin._ensure_engine().deterministic = True
        twin._flat.p32.copy_(flat.p32)
        twin._flat.t32.copy_(flat.t32)
        twin._student_bf16_fresh = twin._teacher_bf16_fresh = False
        twin.accumulate_grads = True
        twin.configure_optimizers()["optimizer"].zero_grad()
        for i in range(2):
            out = twin.training_step(batch(i), i)
            (out["loss"] / 2).backward()
        torch.cuda.synchronize()
        local = twin._flat.g32.clone()
        both = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(both, local)
        want = sum(both) / world
        # the hooked model: count the collectives every call of step() launches; look at the buffer in front of the first update
        launched, per_call, reduced = [0], [], []
        real_hook, real_update = run._hook, run._update

        def hook(tag):
            before = len(run.reducer.handles)
            real_hook(tag)
            launched[0] += len(run.reducer.handles) - before
        run._hook = hook

        def update():
            run.reducer.wait()
            torch.cuda.synchronize()
            reduced.append(flat.g32.clone())
            real_update()
        run._update = update
        for i in range(6):
            before = launched[0]
            out = run.step(batch(i), i)
            per_call.append(launched[0] - before)
        m._engine.wait_optimizer()
        torch.cuda.synchronize()
        buckets = sum(len(v) for v in section_ranges(flat, m.encoder.num_layers, run.reducer.enc_chunk).values())
        dev_grad = float((reduced[0] - want).norm() / (want.norm() + 1e-30))
        not_local = float((reduced[0] - local).norm() / (local.norm() + 1e-30))
        sums = torch.stack([flat.p32.double().sum(), flat.p32.double().abs().sum(), flat.t32.double().sum()]).cpu()
        allsums = [torch.empty_like(sums) for _ in range(world)]
        dist.all_gather(allsums, sums)
        q.put((rank, per_call, buckets, dev_grad, not_local, [s.tolist() for s in allsums], m.global_step, float(out["loss"].detach())))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_reduce_once_per_optimiser_step(golden_dir):
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, golden_dir, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=560) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, per_call, buckets, dev_grad, not_local, allsums, gs, loss in res:
        print("rank", rank, "collectives per call of step():", per_call, "buckets:", buckets, "averaged against the mean of the local "
              "accumulated gradients:", dev_grad, "against the local one:", not_local, flush=True)
        assert buckets >= 3 and per_call == [0, buckets] * 3
        assert dev_grad < 1e-6, dev_grad
        assert not_local > 1e-2
        assert allsums[0] == allsums[1], f"replicas diverged after three optimiser steps: {allsums}"
        assert gs == 3 and np.isfinite(loss)


# ------------------------------------------------------------------------------------------------------------ 11. the launcher
@pytest.mark.parametrize("k", [2, None])
def test_launcher_accumulates(tmp_path, k):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "trainer.size=tiny", "trainer.batch_size=1", "data.samples_per_audio=4",
           "trainer.steps=3", "trainer.warmup_steps=2", "trainer.log_every_n_steps=1", f"save_dir={tmp_path}"]
    if k is not None:
        cmd.append(f"trainer.accumulate_grad_batches={k}")
    rc, out, err = launch.run(cmd, cwd=ROOT, timeout=300)
    assert rc == 0, (out[-1500:], err[-4000:])
    losses = [float(v) for v in re.findall(r"step \d+\s+loss (\S+)", out)]
    print("losses:", losses, [ln for ln in out.splitlines() if ln.startswith(("done", "Effective"))], flush=True)
    assert len(losses) == 3 and all(np.isfinite(losses)) and len(set(losses)) == 3, out[-1500:]
    found = list(tmp_path.rglob("last.ckpt"))
    assert len(found) == 1
    ck = torch.load(found[0], map_location="cpu", weights_only=False)
    assert ck["global_step"] == 3 and ck["optimizer"]["step"] == 3
    assert all(bool(torch.isfinite(v.float()).all()) for v in ck["state_dict"].values())
    if k is None:
        assert set(ck) == {"state_dict", "hyper_parameters", "global_step", "optimizer", "lr_scheduler"}
        assert "Effective Batch Size is: 4" in out and "micro-batches" not in out
    else:
        assert ck["accumulate_grad_batches"] == 2 and "accumulate_grad_batches" not in ck["hyper_parameters"]
        assert "Effective Batch Size is: 8" in out and "done: 3 steps (6 micro-batches, accumulate_grad_batches=2)" in out, out[-1500:]
