"""The masked-loss family on the GPU: wj_masked_loss held per element against the fp64 reference and bounds of
tests/loss_reference.py, a training step with each objective against the oracle (its loss replaced by torch's), deterministic mode and
the train.py launcher.

Kernel cases: the shapes of test_masked_mse -- one active lane, 1.5, 3 and 3.9 passes of the 256-column loop -- with two planted
elements per case (p == y exactly; |p - y| == beta exactly), every kind x beta of loss_reference.GRID.  End to end: the yardstick forms
of tests/parity_yardstick.py with the project's constants, d(HIP, fp32) against d(oracle-bf16, fp32) on the same draw.

With WJ_MASKED_LOSS_REPORT=<path> the module appends the per-group yardstick table of every end-to-end case (and, for L1, the sign
flips of both bf16 pipelines against the fp32 oracle) to that file.
"""
import os
import re
import sys

import pytest
import torch

import synth
from oracle import jepa_oracle as J
from tests import launch
from tests import loss_reference as lr
from tests import norm_reference as nr
from tests import parity_yardstick as Y
from tests.test_jepa_gpu import SMALL, build, dev, group_of, masks, oracle_kw, rel

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 1, 4), (2, 3, 37, 384), (3, 4, 50, 768), (2, 2, 33, 1000)]


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    return o


def report(line):
    print(line)
    path = os.environ.get("WJ_MASKED_LOSS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def to_dev(t):
    return None if t is None else t.to(dev())


def G(M, D=None, dtype=torch.float32):
    return nr.guarded_like(M, D, dtype, dev())


# ------------------------------------------------------------------------------------------------------------ kernel
def run_loss(ops, c, B, G_, T, D, kind, beta, tag, aligned=True, gscale=1.0, gscale_dev=None, rows=None, with_dpreds=True, entry="loss"):
    """two launches of wj_masked_loss (entry="mse": of wj_masked_mse) into guarded outputs: every output within its fp64 bound, guard
    rows untouched, the workspace inside its own rows, identical bits from both launches.  Returns the outputs on the CPU and the
    reference."""
    n = B * G_ * T
    preds = c["preds"] if rows is None else (c["preds"][rows.long()] if rows.numel() else c["preds"][:1])
    R = n if rows is None else int(rows.numel())
    mbuf = torch.ones(n + 32, dtype=torch.uint8, device=dev())          # bytes around the mask are not targets of this call
    off = 0 if aligned else 1
    mbuf[off:off + n] = to_dev(c["tgt"])
    assert mbuf.data_ptr() % 16 == 0
    gp = None if gscale_dev is None else torch.tensor([gscale_dev], device=dev())
    ref = lr.masked_loss(preds, c["targets"], c["tgt"], B, G_, T, D, kind, beta, gscale, gscale_dev, rows)
    what = f"masked_loss {kind} beta={beta} {B, G_, T, D} {tag}"
    outs = []
    for rep in range(2):
        loss, ws = G(2), G(2 + n)
        dp = G(max(R, 1), D, torch.bfloat16)
        kw = dict(B=B, G=G_, T=T, D=D, dpreds=dp.view if with_dpreds else None, gscale=gscale, gscale_ptr=gp,
                  rows=None if rows is None else to_dev(rows if rows.numel() else torch.zeros(1, dtype=torch.int32)),
                  n_rows=R if rows is not None else 0)
        if entry == "mse":
            ops.masked_mse(to_dev(preds), to_dev(c["targets"]), mbuf.data_ptr() + off, loss.view, ws.view, **kw)
        else:
            ops.masked_loss(to_dev(preds), to_dev(c["targets"]), mbuf.data_ptr() + off, loss.view, ws.view, kind=kind, beta=beta, **kw)
        ws.check("workspace " + what)
        got = {"loss": loss.check("loss " + what).cpu()}
        if with_dpreds and R > 0:
            got["dpreds"] = dp.check("dpreds " + what).cpu()
        else:
            assert bool(torch.isnan(dp.check("dpreds").float()).all()), f"{what}: dpreds written though not asked for"
        outs.append(got)
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), f"{what}: {k} differs between two launches"
    got = outs[0]
    ratios = {k: nr.check(got[k], *ref[k], what=f"{what} {k}") for k in got}
    print(what, "error / bound:", {k: round(v, 3) for k, v in ratios.items()})
    assert float(got["loss"][1]) == float(ref["loss"][0][1]), f"{what}: count"
    if "dpreds" in got:
        assert bool((got["dpreds"][ref["_on"][0] == 0].float() == 0).all()), f"{what}: dpreds non-zero on a row that is not a target"
    return got, ref


@pytest.mark.parametrize("kind,beta", lr.GRID)
@pytest.mark.parametrize("B,G_,T,D", CASES)
def test_masked_loss_kernel(ops, B, G_, T, D, kind, beta):
    n = B * G_ * T
    c = lr.plant(nr.mse_inputs(B, G_, T, D, 700), B, G_, T, D, beta)
    cnt, share = lr.quadratic_share(c, B, G_, T, D, beta)
    if cnt >= 1000:      # a condition of the case: both branches of smooth-L1 / Huber are populated
        assert 0.1 <= share <= 0.9, (cnt, share)
    got, ref = run_loss(ops, c, B, G_, T, D, kind, beta, "aligned+tail")            # n % 16 != 0 in every case: vector path and tail
    assert n % 16 != 0
    una, _ = run_loss(ops, c, B, G_, T, D, kind, beta, "unaligned", aligned=False)
    assert torch.equal(una["loss"], got["loss"]) and torch.equal(una["dpreds"], got["dpreds"])
    z, _ = run_loss(ops, lr.plant(nr.mse_inputs(B, G_, T, D, 701, "zeros"), B, G_, T, D, beta), B, G_, T, D, kind, beta, "all-zero mask")
    assert z["loss"].tolist() == [0.0, 0.0] and bool((z["dpreds"].float() == 0).all())
    o, _ = run_loss(ops, lr.plant(nr.mse_inputs(B, G_, T, D, 702, "ones"), B, G_, T, D, beta), B, G_, T, D, kind, beta, "all-ones mask")
    assert float(o["loss"][1]) == n
    run_loss(ops, c, B, G_, T, D, kind, beta, "gscale", gscale=0.5, gscale_dev=3.0)
    on = c["tgt"] != 0
    keep = on | (torch.arange(n) % 3 == 0)          # ragged: the targets and every third of the other rows, in dense order
    rows = torch.nonzero(keep).squeeze(1).to(torch.int32)
    rg, _ = run_loss(ops, c, B, G_, T, D, kind, beta, "ragged", rows=rows)
    assert float(rg["loss"][1]) == float(got["loss"][1]) and torch.equal(rg["dpreds"], got["dpreds"][rows.long()])
    run_loss(ops, c, B, G_, T, D, kind, beta, "ragged, no dpreds", rows=rows, with_dpreds=False)
    e, _ = run_loss(ops, c, B, G_, T, D, kind, beta, "ragged, n_rows=0", rows=torch.zeros(0, dtype=torch.int32))
    assert e["loss"].tolist() == [0.0, float(on.sum())]
    if kind == "mse":       # the same instantiation behind both entries
        m, _ = run_loss(ops, c, B, G_, T, D, kind, beta, "wj_masked_mse", entry="mse")
        assert torch.equal(m["loss"].view(torch.int32), got["loss"].view(torch.int32)), "kind MSE differs from wj_masked_mse: loss"
        assert torch.equal(m["dpreds"].view(torch.int16), got["dpreds"].view(torch.int16)), "kind MSE differs from wj_masked_mse: dpreds"
        mr, _ = run_loss(ops, c, B, G_, T, D, kind, beta, "wj_masked_mse ragged", rows=rows, entry="mse")
        assert torch.equal(mr["loss"].view(torch.int32), rg["loss"].view(torch.int32))
        assert torch.equal(mr["dpreds"].view(torch.int16), rg["dpreds"].view(torch.int16))
    if kind in ("mse", "l1"):       # beta is ignored by these kinds, whatever it holds
        ig, _ = run_loss(ops, c, B, G_, T, D, kind, -1.0, "beta ignored")
        assert torch.equal(ig["loss"], got["loss"]) and torch.equal(ig["dpreds"], got["dpreds"])
    # sensitivity, on the kernel's own (accepted) output
    assert nr.rejected(nr.mutate_count(got["loss"]), *ref["loss"]), "count off by one accepted"
    for label, k, m in lr.mutations(got, c, B, G_, T, D, kind, beta):
        assert nr.rejected(m, *ref[k]), f"{kind} beta={beta}: mutation '{label}' of {k} accepted"
    r, _, _ = c["planted"]
    if bool(on[r]):
        assert float(got["dpreds"][r, 0]) == 0.0, "dpreds at p == y"


# ------------------------------------------------------------------------------------------------------------ end to end
def clips(n, seed=3):
    return torch.from_numpy(synth.synth_audio(n, 1, 32159, seed=seed)).to(torch.bfloat16).to(dev())


def sign_flips(out, ref32, seen):
    """target elements whose sign(pred - target) differs from the fp32 oracle's: (flipped, elements)"""
    B, T, D = ref32["targets"].shape
    def s(o):
        p = o["preds"].float().view(B, -1, T, D)
        return torch.sign(p - o["targets"].float()[:, None]).view(-1, T, D)[seen]
    a, b = s(out), s(ref32)
    return int((a != b).sum()), int(a.numel())


E2E = [("l1", 1.0, True, True), ("l1", 1.0, False, True), ("smooth_l1", 1.0, True, True), ("smooth_l1", 1.0, False, True),
       ("smooth_l1", 1.0, True, False), ("smooth_l1", 0.25, True, True), ("huber", 1.0, True, True)]


@pytest.mark.parametrize("kind,beta,ragged,trim", E2E)
def test_loss_kinds_forward_backward_parity(golden_dir, monkeypatch, kind, beta, ragged, trim):
    """test_prenorm_forward_backward_parity's form for each objective: SMALL, 4 clips, golden AudioSet masks; the oracle's masked_mse
    is the reference's masked_loss with torch's loss.  Loss, activations and parameter-gradient groups in the yardstick forms.

    Measured on the oracle alone (CPU, this draw): d(oracle-bf16, fp32) per group is 0.004 - 0.006 under smooth-L1 and Huber, as under
    MSE, and 0.0076 - 0.009 under L1, where a sign flip on an element whose |d| is below the bf16 rounding of the prediction is a
    discrete event both pipelines meet."""
    monkeypatch.setattr(J, "masked_mse", lr.oracle_masked_loss(kind, beta))
    m, P = build(SMALL, loss_fn=lr.torch_loss_module(kind, beta))
    eng = m._ensure_engine()
    assert (eng.cfg.loss_kind, eng.cfg.loss_beta) == (kind, beta)
    eng.ragged, eng.trim_tail = ragged, trim
    ctx, tgt, vis = masks(golden_dir, 4)
    audio = clips(4)
    out = m(audio, ctx, tgt, vis)
    assert eng.ragged_step == ragged and (eng.tail is not None) == (ragged and trim)
    names = J.trainable_names(P)
    for k in names:
        P[k].requires_grad_(True)
    dm = [t.to(dev()) for t in (ctx, tgt, vis)]
    ref = J.jepa_forward(P, audio, *dm, mode="bf16", **oracle_kw(SMALL))
    ref32 = J.jepa_forward({k: v.detach() for k, v in P.items()}, audio.float(), *dm, mode="fp32", **oracle_kw(SMALL))
    tseen = tgt.reshape(-1, vis.shape[-1]).to(dev())
    tag = f"{kind} beta={beta} {'ragged' if ragged else 'dense'}{'' if trim else ' untrimmed'}"
    for k in ("local_features", "contextual_features", "targets", "preds"):
        sel = (lambda x: x[tseen]) if k == "preds" else (lambda x: x)       # preds are compared where every step form computes them
        d_hip, d_orc, pair = (rel(sel(out[k]).float(), sel(ref32[k]).float()), rel(sel(ref[k]).float(), sel(ref32[k]).float()),
                              rel(sel(out[k]).float(), sel(ref[k]).float()))
        print(tag, k, "d_hip, d_orc, pair:", d_hip, d_orc, pair)
        assert d_hip < Y.ACT_FACTOR * d_orc + Y.ACT_EPS, (k, d_hip, d_orc)
        assert pair < Y.PAIR_FACTOR * d_orc + Y.ACT_EPS, (k, pair, d_orc)
    lo, lr_, l32 = float(out["loss"].detach()), float(ref["loss"].detach()), float(ref32["loss"])
    print(tag, "loss hip/oracle-bf16/oracle-fp32:", lo, lr_, l32)
    assert abs(lo - lr_) < 1e-3 * abs(lr_), (lo, lr_)
    assert abs(lo - l32) < 2e-2 * abs(l32), (lo, l32)
    out["loss"].backward()
    ref["loss"].backward()
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    gbf = {k: P[k].grad for k in names}
    assert set(names) <= set(got)
    _, g32 = Y.oracle_fp32_grads(J, P, audio, *dm, names, **oracle_kw(SMALL))
    table = Y.grad_yardstick(got, gbf, g32, names, group_of)
    report(f"# {tag}: loss hip {lo:.6f} oracle-bf16 {lr_:.6f} oracle-fp32 {l32:.6f}")
    for g, r in table.items():
        report(f"{tag:34s} {g:28s} d_hip {r['d_hip']:.5f}  d_orc {r['d_orc']:.5f}  pair {r['pair']:.5f}  ratio {r['ratio']:.3f}")
    if kind == "l1":
        fh, n_el = sign_flips(out, ref32, tseen)
        fo, _ = sign_flips(ref, ref32, tseen)
        report(f"{tag:34s} sign(pred - target) against the fp32 oracle on {n_el} target elements: HIP {fh} flipped, oracle-bf16 {fo} flipped")
    Y.assert_grad_yardstick(table)


def test_mse_models_launch_masked_mse_and_the_other_kinds_masked_loss(golden_dir, monkeypatch):
    """the default step is what it was: an MSE model (loss_fn None or nn.MSELoss) never reaches wj_masked_loss; every other kind goes
    through it in the forward and in the backward, and never through wj_masked_mse"""
    from wavjepa_amd import ops
    calls = []
    for name in ("masked_mse", "masked_loss"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _fn=fn, _n=name, **k: (calls.append((_n, k.get("dpreds") is not None)), _fn(*a, **k))[1])
    ctx, tgt, vis = masks(golden_dir, 4)
    audio = clips(4)
    for loss_fn, entry in ((None, "masked_mse"), (torch.nn.MSELoss(reduction="none"), "masked_mse"),
                           (torch.nn.L1Loss(reduction="none"), "masked_loss"), (torch.nn.HuberLoss(reduction="none", delta=0.5), "masked_loss")):
        calls.clear()
        m, _ = build(SMALL, loss_fn=loss_fn)
        m(audio, ctx, tgt, vis)["loss"].backward()
        torch.cuda.synchronize()
        assert calls == [(entry, False), (entry, True)], (type(loss_fn).__name__, calls)


def test_smooth_l1_deterministic_mode_repeats_bit_for_bit(golden_dir):
    """two fresh models, one step each with smooth-L1 and engine.deterministic: loss and every gradient bit for bit"""
    ctx, tgt, vis = masks(golden_dir, 4)
    audio = clips(4, seed=700)
    runs = []
    for _ in range(2):
        m, _ = build(SMALL, loss_fn=lr.torch_loss_module("smooth_l1", 1.0))
        m._ensure_engine().deterministic = True
        out = m(audio, ctx, tgt, vis)
        out["loss"].backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
        runs.append((out["loss"].detach().float().reshape(1).clone(), grads))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert set(runs[0][1]) == set(runs[1][1]) and len(runs[0][1]) > 20
    for k, g in runs[0][1].items():
        assert torch.equal(g.view(torch.int32), runs[1][1][k].view(torch.int32)), k


def test_launcher_trains_with_the_configured_loss(tmp_path):
    """`train.py trainer.size=tiny trainer.loss=smooth_l1 trainer.loss_beta=0.5 trainer.steps=3` in a child process: finite losses, the
    checkpoint's hyper-parameters carry the objective; a trainer.loss=mse run's carry neither key."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hp = {}
    for name, extra in (("smooth_l1", ["trainer.loss=smooth_l1", "trainer.loss_beta=0.5"]), ("mse", ["trainer.loss=mse"])):
        save = tmp_path / name
        cmd = [sys.executable, os.path.join(root, "train.py"), "trainer.size=tiny", "trainer.batch_size=1", "data.samples_per_audio=4",
               "trainer.steps=3", "trainer.warmup_steps=2", "trainer.log_every_n_steps=1", f"save_dir={save}"] + extra
        rc, out, err = launch.run(cmd, cwd=root, timeout=300)
        assert rc == 0, (out[-1500:], err[-4000:])
        losses = [float(v) for v in re.findall(r"step \d+\s+loss (\S+)", out)]
        assert len(losses) == 3 and all(v == v and abs(v) < float("inf") for v in losses), out[-1500:]
        found = list(save.rglob("last.ckpt"))
        assert len(found) == 1
        ck = torch.load(found[0], map_location="cpu", weights_only=False)
        assert ck["global_step"] == 3 and all(bool(torch.isfinite(v.float()).all()) for v in ck["state_dict"].values())
        hp[name] = ck["hyper_parameters"]
    assert hp["smooth_l1"].get("loss") == "smooth_l1" and hp["smooth_l1"].get("loss_beta") == 0.5
    assert "loss" not in hp["mse"] and "loss_beta" not in hp["mse"]
    assert set(hp["smooth_l1"]) == set(hp["mse"]) | {"loss", "loss_beta"}
