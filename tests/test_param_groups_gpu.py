"""Parameter groups through the training step (GPU only): JEPA(weight_decay_exclude="1d", layer_lr_decay=0.75) on the small model of
tests/test_jepa_gpu.py, 4 clips of 2.01 s with the golden AudioSet masks, deterministic mode, the cosine schedule with warmup_steps=2.

Every optimiser step that is checked is held element by element to tests/param_groups_reference.grouped_step (optimizer_reference's
fp64 step and bound, per group), driven by the engine's own gradient, moments and sum of squares and by that step's per-group lr and
weight decay.  Every test prints its figures before it asserts."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import launch
from tests import norm_reference as nr
from tests import param_groups_reference as pgr
from tests.test_accumulate_gpu import launch_trace, prepared, runner, state_bits
from tests.test_jepa_gpu import SMALL, build, dev, masks
from tests.test_prenorm_gpu import clips
from tests.test_recompute_gpu import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPED = dict(weight_decay_exclude="1d", layer_lr_decay=0.75, warmup_steps=2)
LR, WD, DECAY = 4e-4, 0.04, 0.75             # tests.test_jepa_gpu.build's lr and weight decay


def fresh(seed=7, **kw):
    m, _ = build(SMALL, seed=seed, **dict(GROUPED, **kw))
    m._ensure_engine().deterministic = True
    m.trainer.max_steps = 20
    return m


def batches(golden_dir, n, seed=800):
    ctx, tgt, vis = masks(golden_dir, 4)
    return [(clips(4, seed=seed + i), ctx, tgt, vis) for i in range(n)]


def lambda_of(step, warmup=2, total=20):
    import math
    if step < warmup:
        return float(step) / float(max(1, warmup))
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * (float(step - warmup) / float(max(1, total - warmup))))))


def expected_groups(m):
    """(initial lr, weight decay) per group of the small model: ids 0 .. L + 1, each decayed then not"""
    L = m.encoder.num_layers
    return [(LR * DECAY ** (L + 1 - i), wd) for i in range(L + 2) for wd in (WD, 0.0)]


_ELEM = {}


def element_map(m, opt):
    key = tuple(sorted(opt._assignment.items()))
    if key not in _ELEM:
        _ELEM[key] = pgr.element_groups(m._flat.slots, opt._assignment, m._flat.n)
    return _ELEM[key]


def snapshot(m):
    m._engine.wait_optimizer()
    torch.cuda.synchronize()
    f = m._flat
    f.ensure_adam_state()
    return {k: t.detach().cpu().clone() for k, t in (("p", f.p32), ("g", f.g32), ("m", f.adam_m), ("v", f.adam_v))}


def held_step(m, opt, lrs, wds, what, zero_grad=False):
    """opt.step() between two snapshots, every element of p, m, v, the bf16 shadow and g held to the reference with the given pairs"""
    before = snapshot(m)
    opt.step()
    after = snapshot(m)
    after["p_bf16"] = m._flat.p16.detach().cpu().clone()
    ss = opt._sumsq.detach().cpu()
    Fc = pgr.common_fields(opt._t, 1.0, max_norm=opt.max_grad_norm)
    ref = pgr.grouped_step(before["p"], before["g"], before["m"], before["v"], ss if opt.max_grad_norm > 0 else None, Fc, lrs, wds,
                           element_map(m, opt), zero_grad=zero_grad)
    worst = {k: nr.worst(after[k], *ref[k]) for k in ("p", "m", "v", "p_bf16", "g")}
    print(what, "step", opt._t, "lr", [f"{x:.3e}" for x in lrs], "wd", wds, "norm", float(ss.sqrt()), "worst error / bound:", worst, flush=True)
    for k, w in worst.items():
        assert w <= 1.0, f"{what} step {opt._t}: {k} error / bound = {w:.3g} {nr.where_worst(after[k], *ref[k])}"
    assert torch.equal(after["p_bf16"], after["p"].to(torch.bfloat16))
    return before, after, ref


def slot_range(m, name):
    s = m._flat.by_name[name]
    return slice(s.offset, s.offset + s.numel)


# ------------------------------------------------------------------------------------------------------------ 1. four steps
def test_four_steps_against_the_reference(golden_dir):
    m = fresh()
    assert m.hparams["weight_decay_exclude"] == "1d" and m.hparams["layer_lr_decay"] == 0.75
    oc = m.configure_optimizers()
    opt, sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
    opt.max_grad_norm = 5.0
    want = expected_groups(m)
    assert [(g["initial_lr"], g["weight_decay"]) for g in opt.param_groups] == want and len(want) == 8
    flat = m._flat
    one_d, two_d = "encoder.layers.0.norm1.weight", "encoder.layers.0.linear1.weight"
    assert opt.param_groups[opt._assignment[one_d]]["weight_decay"] == 0.0 and opt.param_groups[opt._assignment[two_d]]["weight_decay"] == WD
    for i, b in enumerate(batches(golden_dir, 4)):
        out = m(*b)
        out["loss"].backward()
        lrs, wds = [x * lambda_of(i) for x, _ in want], [w for _, w in want]
        assert [g["lr"] for g in opt.param_groups] == lrs, i
        if i == 2:
            # a parameter without gradient and without history moves by its decay factor alone: the "1d" one not at all, the matrix by
            # 1 - lr * wd of ITS group
            flat.ensure_adam_state()
            for name in (one_d, two_d, "mask_token"):
                for t in (flat.g32, flat.adam_m, flat.adam_v):
                    t[slot_range(m, name)] = 0.0
        before, after, _ = held_step(m, opt, lrs, wds, "four steps")
        assert torch.equal(after["g"], before["g"])                                # (fuse_zero_grad is off in this loop)
        if i == 0:
            assert torch.equal(bits(after["p"]), bits(before["p"])), "lr 0 at the first step of the warm-up: nothing may move"
        if i == 2:
            for name in (one_d, "mask_token"):
                assert torch.equal(bits(after["p"][slot_range(m, name)]), bits(before["p"][slot_range(m, name)])), f"{name} carries a decay factor"
            a, b0 = after["p"][slot_range(m, two_d)].double(), before["p"][slot_range(m, two_d)].double()
            k = opt._assignment[two_d]
            moved = float(((a - b0).abs() / b0.abs().clamp_min(1e-30)).median())
            print("median relative move of the matrix without gradient:", moved, "lr * wd of its group:", lrs[k] * WD, flush=True)
            assert abs(moved - lrs[k] * WD) < 0.25 * lrs[k] * WD and lrs[k] * WD > 1e-6
        sched.step()
        m.global_step += 1
    # the groups really differ: the last step moved the front-end (lr * 0.75^3) less than the predictor, relative to Adam's unit step
    assert len({round(x, 12) for x in lrs}) == 4


# ------------------------------------------------------------------------------------------------------------ 2. the training loop's forms
def test_overlap_and_fused_clear_are_bit_equal_to_the_plain_update(golden_dir):
    LT = launch_trace()
    bs = batches(golden_dir, 4, seed=820)
    ends, counts = [], []
    for on in (True, False):
        m = fresh()
        run = runner(m)
        assert run.optimizer.overlap_next_forward and run.optimizer.fuse_zero_grad and run.optimizer._assignment is not None
        if not on:
            run.optimizer.overlap_next_forward = run.optimizer.fuse_zero_grad = False
        for i, b in enumerate(bs):
            if i == 2:
                with LT.Trace(m._engine) as tr:
                    run.step(b, i)
                counts.append([ln.split()[0] for ln in tr.lines if " wj_adamw_groups_step " in ln])
                assert not [ln for ln in tr.lines if " wj_adamw_step " in ln]
            else:
                run.step(b, i)
        st = state_bits(m)
        st["g_max"] = float(m._flat.g32.abs().max())
        ends.append(st)
    front, rest = m._flat.front_and_rest_ranges()
    print("grouped launches of one step (streams), overlap on / off:", counts, "front / rest ranges:", len(front), len(rest),
          "max |g32| behind the last step, fused clear on / off:", ends[0]["g_max"], ends[1]["g_max"], flush=True)
    assert counts[1] == ["main"]
    if m._engine.use_side:
        assert counts[0] == ["main"] * len(front) + ["side"] * len(rest) and len(counts[0]) >= 3
    assert ends[0]["g_max"] == 0.0 and ends[1]["g_max"] > 0.0
    for name in ("parameters", "teacher", "adam_m", "adam_v"):
        assert torch.equal(ends[0][name], ends[1][name]), name


# ------------------------------------------------------------------------------------------------------------ 3. a user's schedule
def test_a_weight_decay_schedule_written_between_steps_is_used(golden_dir):
    m = fresh()
    oc = m.configure_optimizers()
    opt, sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
    opt.max_grad_norm = 5.0
    want = expected_groups(m)
    for i, b in enumerate(batches(golden_dir, 4, seed=840)):
        wds = [0.04 + 0.12 * i + 0.01 * k for k in range(len(want))]           # (also on the groups that started without decay)
        for g, w in zip(opt.param_groups, wds):
            g["weight_decay"] = w
        out = m(*b)
        out["loss"].backward()
        held_step(m, opt, [x * lambda_of(i) for x, _ in want], wds, "wd schedule")
        sched.step()
        m.global_step += 1
    # the bound tells the schedule from a constant: the last step with the first step's decays is rejected
    before = snapshot(m)
    stale = pgr.grouped_step(before["p"], before["g"], before["m"], before["v"], opt._sumsq.cpu(), pgr.common_fields(opt._t + 1, 1.0, max_norm=5.0),
                             [g["lr"] for g in opt.param_groups], [0.04 + 0.01 * k for k in range(len(want))], element_map(m, opt))
    opt.step()
    after = snapshot(m)
    assert nr.worst(after["p"], *stale["p"]) > 1.0


# ------------------------------------------------------------------------------------------------------------ 4. accumulation
def test_accumulated_gradient_feeds_the_grouped_update(golden_dir):
    bs = batches(golden_dir, 4, seed=860)
    twin = fresh()                                                                # the ordinary torch loop: zero_grad, 2 x (loss / 2).backward()
    prepared(twin).accumulate_grads = True
    twin.configure_optimizers()["optimizer"].zero_grad()
    for i, b in enumerate(bs[:2]):
        (twin.training_step(b, i)["loss"] / 2).backward()
    torch.cuda.synchronize()
    g_window = twin._flat.g32.clone()
    m = fresh()
    run = runner(m, 2)
    opt = run.optimizer
    assert opt._assignment is not None and opt.fuse_zero_grad and m.accumulate_grads
    want = expected_groups(m)
    seen = []
    real = opt.step

    def step():
        i = opt._t
        opt.step = real
        try:
            before, after, _ = held_step(m, opt, [x * lambda_of(i) for x, _ in want], [w for _, w in want], "accumulate k=2", zero_grad=True)
        finally:
            opt.step = step
        seen.append(before["g"])
        assert float(after["g"].abs().max()) == 0.0
    opt.step = step
    for i, b in enumerate(bs):
        run.step(b, i)
    assert len(seen) == 2 and m.global_step == 2
    print("accumulated buffer in front of the first update against the torch loop's: bit-equal",
          bool(torch.equal(bits(seen[0]), bits(g_window.cpu()))), flush=True)
    assert torch.equal(bits(seen[0]), bits(g_window.cpu()))


# ------------------------------------------------------------------------------------------------------------ 5. checkpoint resume
def test_checkpoint_resume_is_bit_equal_and_keeps_the_group_lrs(tmp_path):
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
        for i in range(4):
            b = src.next_batch()
            torch.manual_seed(1000 + i)        # the crop offsets of on_after_batch_transfer come from the global generator
            if i >= skip:
                yield b

    def run(seed, root, ckpt=None, skip=0):
        m, _ = build(SMALL, seed=seed, **GROUPED)
        tr = Trainer(max_steps=4, default_root_dir=str(root), checkpoint_every_n_steps=2, log_every_n_steps=0, deterministic=True)
        return m, tr.fit(m, train_dataloaders=loader(skip), ckpt_path=ckpt)
    ma, ra = run(7, tmp_path / "a")
    ck = tmp_path / "a" / "step=2.ckpt"
    saved = torch.load(ck, map_location="cpu", weights_only=False)
    want = expected_groups(ma)
    # (Trainer(max_steps=4): the cosine runs over 4 steps)
    lam = lambda_of(2, total=4)
    print("group lrs in the checkpoint:", saved["optimizer"]["group_lr"], "hyper-parameters:",
          {k: saved["hyper_parameters"][k] for k in ("weight_decay_exclude", "layer_lr_decay")}, flush=True)
    assert saved["global_step"] == 2 and saved["optimizer"]["step"] == 2
    assert saved["optimizer"]["group_lr"] == [x * lam for x, _ in want] and saved["optimizer"]["group_weight_decay"] == [w for _, w in want]
    assert len(set(saved["optimizer"]["group_lr"])) == 4
    assert saved["hyper_parameters"]["weight_decay_exclude"] == "1d" and saved["hyper_parameters"]["layer_lr_decay"] == 0.75
    mb, rb = run(8, tmp_path / "b", ckpt=str(ck), skip=2)
    assert ma.global_step == mb.global_step == 4 and ra.optimizer._t == rb.optimizer._t == 4
    assert [g["lr"] for g in ra.optimizer.param_groups] == [g["lr"] for g in rb.optimizer.param_groups]
    a, b = state_bits(ma), state_bits(mb)
    for name in a:
        print(name, "bit-equal after the resume:", bool(torch.equal(a[name], b[name])), flush=True)
    for name in a:
        assert torch.equal(a[name], b[name]), name


# ------------------------------------------------------------------------------------------------------------ 6. the default model
def test_default_model_issues_the_single_group_launches(golden_dir):
    """A model without the keywords, and one that passes their defaults, issue the same events: wj_adamw_step with the one lr and weight
    decay, on the ranges it always took, and no grouped launch.  (The hashes of tools/launch_trace.py --summary against the parent
    tree's are in PARITY.md: they need both trees.)"""
    LT = launch_trace()
    bs = batches(golden_dir, 3, seed=880)
    traces = []
    for kw in ({}, dict(weight_decay_exclude=None, layer_lr_decay=1.0)):
        m, _ = build(SMALL, warmup_steps=2, **kw)
        m._ensure_engine().deterministic = True
        m.trainer.max_steps = 20
        assert not {"weight_decay_exclude", "layer_lr_decay"} & set(m.hparams)
        run = runner(m)
        assert run.optimizer._assignment is None and len(run.optimizer.param_groups) == 1
        run.step(bs[0], 0)
        with LT.Trace(m._engine) as tr:
            run.step(bs[1], 1)
        run.step(bs[2], 2)
        traces.append((tr.lines, state_bits(m)))
    lines = traces[0][0]
    adam = [ln for ln in lines if " wj_adamw_step " in ln]
    front, rest = m._flat.front_and_rest_ranges()
    print("events of a traced default step:", len(lines), "wj_adamw_step launches:", len(adam), flush=True)
    assert not [ln for ln in lines if "wj_adamw_groups_step" in ln]
    assert len(adam) == (len(front) + len(rest) if m._engine.use_side else 1)
    assert all(f"lr={nr.f32eps(LR * lambda_of(1))!r} " in ln and f"weight_decay={nr.f32eps(WD)!r} " in ln for ln in adam), adam[0]
    assert traces[0][0] == traces[1][0] and len(lines) > 50
    for name in traces[0][1]:
        assert torch.equal(traces[0][1][name], traces[1][1][name]), name


# ------------------------------------------------------------------------------------------------------------ 7. two ranks
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
        from tests import test_param_groups_gpu as T
        m = T.fresh()
        if rank == 1:                              # the broadcast from rank 0 must undo this
            with torch.no_grad():
                for p in m.parameters():
                    p.add_(0.01)
        run = T.runner(m)
        assert run.reducer.active and run.optimizer._assignment is not None and len(run.optimizer.param_groups) == 8
        fx = dict(np.load(os.path.join(golden_dir, "masks.npz")))
        for i in range(2):                         # the ranks see different clips and masks
            lo = 2 * ((i + rank) % 3)
            run.step((T.clips(2, seed=900 + 2 * i + rank),) + tuple(torch.from_numpy(fx[k][lo:lo + 2]) for k in ("as_ctx", "as_tgt", "as_vis")), i)
        m._engine.wait_optimizer()
        torch.cuda.synchronize()
        flat = m._flat
        sums = torch.stack([flat.p32.double().sum(), flat.p32.double().abs().sum(), flat.t32.double().sum(), flat.adam_m.double().abs().sum(),
                            flat.adam_v.double().sum()]).cpu()
        allsums = [torch.empty_like(sums) for _ in range(world)]
        dist.all_gather(allsums, sums)
        q.put((rank, [s.tolist() for s in allsums], m.global_step, [g["lr"] for g in run.optimizer.param_groups]))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_stay_identical_with_groups(golden_dir):
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
    for rank, allsums, gs, lrs in res:
        print("rank", rank, "sums of p, |p|, teacher, |m|, v on both ranks:", allsums, "group lrs:", lrs, flush=True)
        assert allsums[0] == allsums[1], f"replicas diverged after two optimiser steps: {allsums}"
        assert gs == 2 and all(np.isfinite(allsums[0])) and len(set(lrs)) == 4


# ------------------------------------------------------------------------------------------------------------ 8. the launcher
@pytest.mark.parametrize("exclude", ["1d", None])
def test_launcher_takes_the_key(tmp_path, exclude):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "trainer.size=tiny", "trainer.batch_size=1", "data.samples_per_audio=4",
           "trainer.steps=3", "trainer.warmup_steps=2", "trainer.log_every_n_steps=1", f"save_dir={tmp_path}"]
    if exclude is not None:
        cmd.append(f"+optimizer.weight_decay_exclude={exclude}")
    rc, out, err = launch.run(cmd, cwd=ROOT, timeout=300)
    assert rc == 0, (out[-1500:], err[-4000:])
    losses = [float(v) for v in re.findall(r"step \d+\s+loss (\S+)", out)]
    print("losses:", losses, flush=True)
    assert len(losses) == 3 and all(np.isfinite(losses)), out[-1500:]
    found = list(tmp_path.rglob("last.ckpt"))
    assert len(found) == 1
    ck = torch.load(found[0], map_location="cpu", weights_only=False)
    assert ck["global_step"] == 3 and ck["optimizer"]["step"] == 3
    assert all(bool(torch.isfinite(v.float()).all()) for v in ck["state_dict"].values())
    if exclude is None:
        assert not {"weight_decay_exclude", "layer_lr_decay"} & set(ck["hyper_parameters"])
        assert set(ck["optimizer"]) == {"step", "lr", "m", "v"}
    else:
        assert ck["hyper_parameters"]["weight_decay_exclude"] == "1d" and "layer_lr_decay" not in ck["hyper_parameters"]
        assert ck["optimizer"]["group_weight_decay"] == [ck["hyper_parameters"]["adam_weight_decay"], 0.0] and len(ck["optimizer"]["group_lr"]) == 2
