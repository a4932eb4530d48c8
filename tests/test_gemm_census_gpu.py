"""Every GEMM call of the benchmarked training step, replayed against an fp64 reference (tests/gemm_reference.py).

Census: for each workload of bench.WORKLOADS one training step runs through StepRunner at the benchmark's clips per GPU, with
ops.gemm / ops.gemm_mxfp8 / ops.wgrad_grouped wrapped to record the fields of every call (the gather lists copied to the host) before
calling through.  The calls are deduplicated on their full signature; the model is freed; then every class is replayed on fresh
seeded operands placed at the recorded page offsets, with guard bands:
  * as recorded (the library's choice), and at persist_cus 28 (the data-parallel setting);
  * forced to every variant (schedule 0-6), the persistent ones also at persist_cus 28;
each launch on NaN-filled outputs, every element inside the region within its per-element fp64 bound, every byte outside unchanged.
Outputs written without atomics must keep the header's promises: variants 0-3 and 5 bit-identical, 4 and 6 bit-identical (also at
28 workgroups per XCD), 4 against 3 last-place differences on < 2e-3 of the elements.  Every class then proves the checker sensitive at
its own shape: each mutation of gemm_reference applied to the real output must be rejected.  A call form without a reference fails
the test with its fields.  WJ_GEMM_CENSUS_REPORT=<path>: the per-class report is also written there (profiles/gemm_census.txt)."""
import ctypes
import gc
import json
import os
import time

import numpy as np
import pytest
import torch

from tests import gemm_reference as gr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIPS = {"2s-bf16": 256, "4s-bf16": 256, "4s-fp8": 256, "2s-nat": 256}     # bench.py's default --clips-per-gpu
VARIANTS = tuple(range(7))
REPORT = []


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    return o


def dev():
    return torch.device("cuda:0")


_HIP = []


def _d2h_int32(ptr, n: int) -> np.ndarray:
    """n int32 entries of a device list (a tensor or a raw pointer of the engine's arena), after a device synchronise"""
    torch.cuda.synchronize()
    if isinstance(ptr, torch.Tensor):
        return ptr.view(-1)[:n].to(torch.int32).cpu().numpy().copy()
    if not _HIP:
        lib = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
        lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _HIP.append(lib)
    out = np.empty(n, dtype=np.int32)
    rc = _HIP[0].hipMemcpy(out.ctypes.data, ctypes.c_void_p(int(ptr)), n * 4, 2)      # hipMemcpyDeviceToHost
    assert rc == 0, f"hipMemcpy failed ({rc})"
    return out


def census(ops, monkeypatch, workload: str, clips: int):
    """[(kind, fields or [fields per problem])] of every GEMM call of one training step of `workload` at `clips` clips per GPU."""
    import bench
    from tests.test_jepa_gpu import PinnedRng
    from wavjepa_amd.data import NatSceneSource, SyntheticAudioSource
    from wavjepa_amd.masking import TimeInverseBlockMasker
    from wavjepa_amd.trainer import StepRunner
    seconds, fp8, nat = bench.WORKLOADS[workload]
    model = bench.build_model(dev(), seed=42, seconds=seconds, nat=nat)
    model._ensure_engine().fp8 = fp8
    model.trainer.max_steps = 375000
    # as bench.main() builds them (masker: configs/masker/AudioSet.yaml; one mask set instead of 64 cycled ones)
    masker = TimeInverseBlockMasker(4, 0.65, 10, 0.25, 10, 0.1, channel_based_masking=nat, channel_major=nat)
    with PinnedRng(4242):
        src = (NatSceneSource if nat else SyntheticAudioSource)(masker, batch_size=clips // 8, samples_per_audio=8,
                                                                n_tokens=model.total_patches, seed=42, n_mask_sets=1, device=dev())
    torch.manual_seed(42)
    torch.cuda.manual_seed(42)
    runner = StepRunner(model, gradient_clip_val=5.0)
    calls = []
    real_gemm, real_fp8, real_wgrad = ops.gemm, ops.gemm_mxfp8, ops.wgrad_grouped

    def gemm(A, B, C, **kw):
        full = dict(kw, A=A, B=B, C=C)
        rm = kw.get("rowmap")
        host = None if rm is None else _d2h_int32(rm, kw["K"] + 256 if kw.get("a_trans") else kw["M"])
        f = gr.call_fields(full, host)
        f["schedule"] = ops._GEMM_SCHEDULE if kw.get("schedule") is None else int(kw["schedule"])      # as the binding resolves them
        f["persist_cus"] = ops._PERSIST_CUS if kw.get("persist_cus") is None else int(kw["persist_cus"])
        calls.append(("gemm", f))
        return real_gemm(A, B, C, **kw)

    def gemm_mxfp8(A8, B8, scale_a, scale_b, C, **kw):
        calls.append(("gemm_mxfp8", gr.call_fields(dict(kw, A8=A8, B8=B8, scale_a=scale_a, scale_b=scale_b, C=C), entry="gemm_mxfp8")))
        return real_fp8(A8, B8, scale_a, scale_b, C, **kw)

    def wgrad_grouped(problems, stream=None):
        calls.append(("wgrad", [gr.wgrad_fields(*p) for p in problems]))
        return real_wgrad(problems, stream=stream)

    with monkeypatch.context() as mp:
        mp.setattr(ops, "gemm", gemm)
        mp.setattr(ops, "gemm_mxfp8", gemm_mxfp8)
        mp.setattr(ops, "wgrad_grouped", wgrad_grouped)
        out = runner.step(src.next_batch(), 0)
        torch.cuda.synchronize()
    assert bool(torch.isfinite(torch.as_tensor(float(out["loss"].detach())))), "the census step's loss is not finite"
    del model, runner, src, out
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return calls


def classes(calls):
    seen = {}
    for kind, f in calls:
        key = (kind, tuple(gr.signature(x) for x in f)) if kind == "wgrad" else (kind, gr.signature(f))
        if key not in seen:
            seen[key] = [kind, f, 0]
        seen[key][2] += 1
    return list(seen.values())


def _quantize(ops):
    def q(x):
        M, N = x.shape
        xq = x.contiguous()
        qb = torch.empty(M, N, dtype=torch.uint8, device=dev())
        sc = torch.zeros(ops.fp8_scale_dwords(M, N), dtype=torch.int32, device=dev())
        ops.quantize_mxfp8(xq, qb, sc, M=M, K=N, ldx=N, ldq=N, ld_scale=M)
        return qb, sc[:(N // 128) * M].view(N // 128, M)
    return q


def _bits(t):
    return gr._ibits(t)


def _ulp_relation(o, exp, a, b, name):
    """variant 4 against 3: last-place differences on < 2e-3 of the region (test_gemm_persistent_schedule's figure)"""
    x, y = o.region(name, a), o.region(name, b)
    d = (x.float() - y.float()).abs()
    frac = float((d > 0).float().mean())
    ok = frac < 2e-3 and bool((d <= 2.0 ** -6 * torch.maximum(x.float().abs(), y.float().abs()) + 4e-3).all())
    return ok, frac


def replay_gemm(ops, f, seed, fails):
    o = gr.Operands(f, dev(), seed=seed)
    q = None
    atomic = f["epilogue"] == "ATOMIC_F32"
    exp, snap = None, None
    rec = f["schedule"]
    runs = [("recorded", rec, f["persist_cus"], f["workspace"]), ("recorded@28", rec, 28, f["workspace"])]
    runs += [(f"v{v}", v, 32, False) for v in VARIANTS] + [("v4@28", 4, 28, False), ("v6@28", 6, 28, False)]
    kept, worst, ran, recorded = {}, 0.0, [], None
    for name, sched, cus, ws in runs:
        o.reset_outputs()
        if exp is None:
            snap = o.snapshot()
            exp = gr.reference(o, snap)
        wsb = None
        if ws:
            nb = ops.workspace_bytes("wj_gemm_bf16", M=f["M"], N=f["N"], K=f["K"], epilogue=gr.EPI[f["epilogue"]], split_k=f["split_k"])
            wsb = torch.zeros(max(nb, 256), dtype=torch.uint8, device=dev())
        ops.gemm(**o.kwargs(), schedule=sched, persist_cus=cus, workspace=wsb)
        torch.cuda.synchronize()
        bad, w = gr.check(o, exp, snap, quantize=q)
        worst = max(worst, w)
        ran.append(name)
        fails += [f"{name}: {b}" for b in bad]
        outs = {n: o.b[n].t.clone() for n in exp.ref}
        if name == "recorded":
            recorded = {n: o.b[n].t.clone() for n in snap}
        if atomic:
            continue
        rep = {"recorded@28": "recorded", "v1": "v0", "v2": "v0", "v3": "v0", "v5": "v0", "v6": "v4", "v4@28": "v4", "v6@28": "v4"}.get(name)
        if rep is None:
            kept[name] = outs
        else:
            for n in exp.ref:
                if not torch.equal(_bits(outs[n]), _bits(kept[rep][n])):
                    fails.append(f"{name} not bit-identical to {rep} ({n}: {int((_bits(o.region(n, outs[n])) != _bits(o.region(n, kept[rep][n]))).sum())} elements)")
        if name == "v4":
            for n in exp.ref:
                ok, frac = _ulp_relation(o, exp, outs[n], kept["v0"][n], n)
                if not ok:
                    fails.append(f"v4 against v3 ({n}): {frac:.2e} of the elements differ, or by more than the last place")
    split = f["split_k"] if atomic else 1
    for what, mutated in gr.mutations(o, exp, recorded, split):
        if not gr.check(o, exp, snap, mutated)[0]:
            fails.append(f"mutation '{what}' was not rejected")
    del o, exp, kept, recorded
    return ran, worst


def replay_fp8(ops, f, seed, fails):
    o = gr.Operands(f, dev(), seed=seed)
    q = _quantize(ops)
    o.reset_outputs()
    snap = o.snapshot()
    exp = gr.reference(o, snap)
    ops.gemm_mxfp8(**o.kwargs())
    torch.cuda.synchronize()
    ran, worst, q_source = ["recorded"], 0.0, None
    if f["q_out"] and not f["C"]:           # q_out alone: the same call with C given must write the same bytes, = quantize(C)
        g = dict(f, C=True)
        o2 = gr.Operands(g, dev(), seed=seed)
        o2.reset_outputs()
        snap2 = o2.snapshot()
        exp2 = gr.reference(o2, snap2)
        ops.gemm_mxfp8(**o2.kwargs())
        torch.cuda.synchronize()
        bad, worst = gr.check(o2, exp2, snap2, quantize=q)
        fails += [f"with C: {b}" for b in bad]
        q_source = o2.region("C")
        for n in ("q_out", "q_scales"):
            if not torch.equal(o.b[n].t[o.b[n].p:o.b[n].p + o.b[n].hi], o2.b[n].t[o2.b[n].p:o2.b[n].p + o2.b[n].hi]):
                fails.append(f"{n} differs between the call with and without C")
        ran.append("with C")
        for what, mutated in gr.mutations(o2, exp2, {n: o2.b[n].t.clone() for n in snap2}):
            if not gr.check(o2, exp2, snap2, mutated)[0]:
                fails.append(f"mutation '{what}' was not rejected")
    bad, w = gr.check(o, exp, snap, quantize=q, q_source=q_source)
    fails += [f"recorded: {b}" for b in bad]
    worst = max(worst, w)
    for what, mutated in gr.mutations(o, exp, {n: o.b[n].t.clone() for n in snap}):
        if not gr.check(o, exp, snap, mutated)[0]:
            fails.append(f"mutation '{what}' was not rejected")
    return ran, worst


def replay_wgrad(ops, fs, seed, fails):
    os_ = [gr.Operands(f, dev(), seed=seed + i) for i, f in enumerate(fs)]
    snaps, exps = [], []
    for o in os_:
        o.reset_outputs()
        snaps.append(o.snapshot())
        exps.append(gr.reference(o, snaps[-1]))
    ops.wgrad_grouped([(o.b["A"].ptr, o.b["B"].ptr, o.b["C"].ptr, o.f["M"], o.f["N"], o.f["K"]) for o in os_])
    torch.cuda.synchronize()
    worst = 0.0
    for i, (o, e, s) in enumerate(zip(os_, exps, snaps)):
        bad, w = gr.check(o, e, s)
        worst = max(worst, w)
        fails += [f"problem {i}: {b}" for b in bad]
        for what, mutated in gr.mutations(o, e, {n: o.b[n].t.clone() for n in s}, 2):
            if not gr.check(o, e, s, mutated)[0]:
                fails.append(f"problem {i}: mutation '{what}' was not rejected")
    return ["grouped"], worst


def _class_key(lay, epi, M, N, K):
    """(layout, epilogue, N, K); for the weight gradients K is the token count, which moves with the masks: (layout, epilogue, M, N)"""
    return (lay, epi, M, N) if epi == "ATOMIC_F32" else (lay, epi, N, K)


def _profile_classes():
    """class keys of every class in the committed rocprof census of the headline step"""
    d = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_gemm_shapes.json")))
    out = set()
    for k in d:
        if not k.startswith("gemm_kernel<"):
            continue
        head, rest = k[len("gemm_kernel<"):].split(">", 1)
        lay, epi = head.split(",")
        kv = dict(x.split("=") for x in rest.split() if "=" in x)
        out.add(_class_key(lay, epi, int(kv["M"]), int(kv["N"]), int(kv["K"])))
    return out


@pytest.mark.parametrize("workload", sorted(CLIPS))
def test_gemm_census_replays_within_the_fp64_bound(ops, monkeypatch, workload):
    t0 = time.perf_counter()
    sched0, cus0 = ops._GEMM_SCHEDULE, ops._PERSIST_CUS
    clips = CLIPS[workload]
    calls = census(ops, monkeypatch, workload, clips)
    t_census = time.perf_counter() - t0
    cls = classes(calls)
    gate = [f"{kind}: {gr.unsupported(x)}: {x}" for kind, f, _ in cls for x in (f if kind == "wgrad" else [f]) if gr.unsupported(x)]
    assert not gate, "call forms the reference helper does not cover:\n" + "\n".join(gate)
    if workload == "2s-bf16":
        have = {_class_key("NT"[f["a_trans"]] + "NT"[f["b_trans"]], f["epilogue"], f["M"], f["N"], f["K"]) for kind, f, _ in cls if kind == "gemm"}
        missing = _profile_classes() - have
        assert not missing, f"classes of profiles/r06_bench_gemm_shapes.json the census did not see: {sorted(missing)}"
        assert any(kind == "wgrad" for kind, _, _ in cls), "no grouped weight gradient in the census"
    failing, lines = [], []
    for i, (kind, f, count) in enumerate(cls):
        fails = []
        seed = 1000 + i
        if kind == "gemm":
            ran, worst = replay_gemm(ops, f, seed, fails)
            desc = gr.describe(f) + (f" schedule={f['schedule']} persist_cus={f['persist_cus']}")
        elif kind == "gemm_mxfp8":
            ran, worst = replay_fp8(ops, f, seed, fails)
            desc = gr.describe(f)
        else:
            ran, worst = replay_wgrad(ops, f, seed, fails)
            desc = "wgrad_grouped [" + "; ".join(f"M={x['M']} N={x['N']} K={x['K']}" for x in f) + "]"
        gc.collect()
        torch.cuda.empty_cache()
        line = f"{workload} x{count} {desc} | ran {','.join(ran)} | max err/bound {worst:.3f}" + (" | FAIL" if fails else "")
        lines.append(line)
        print(line, flush=True)
        if fails:
            failing.append(line + "\n    " + "\n    ".join(fails[:8]))
    elapsed = time.perf_counter() - t0
    summary = f"{workload}: {clips} clips per GPU, {len(calls)} calls, {len(cls)} classes; census {t_census:.1f} s, total {elapsed:.1f} s"
    print(summary, flush=True)
    REPORT.extend([summary] + lines)
    path = os.environ.get("WJ_GEMM_CENSUS_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write("\n".join([summary] + lines) + "\n")
    assert (ops._GEMM_SCHEDULE, ops._PERSIST_CUS) == (sched0, cus0), "the binding's GEMM defaults changed"
    assert not failing, f"{len(failing)} of {len(cls)} classes failed:\n" + "\n".join(failing)
