#!/usr/bin/env python3
"""What does the group lookup cost the AdamW pass?  wj_adamw_groups_step (libwavjepa_hip_optim.so) against wj_adamw_step of ANOTHER
build of libwavjepa_hip.so -- the parent commit's, given with --parent-lib -- over the base model's flat buffers (p, g, m, v fp32 and the
bf16 shadow: 1.7 GB, far beyond the Infinity Cache, so every launch streams from HBM), with the fused clear and the fused clip on.

Variants: the parent's pass; 2 groups alternating per slot as `weight_decay_exclude="1d"` lays them out on the base model (weights and
their biases / norm scales alternate through the flat layout); 52 groups, slot j in group j % 52.  Forms: the full grid (workgroups 0)
and the side-stream form of FusedAdamW.overlap_next_forward (256 workgroups).  One process; a block times `--reps` launches of every
variant in turn (device events around each launch), `--blocks` blocks; the figure of a variant is the median of its block medians.
Acceptance (per form): grouped median <= parent median x (1 + 0.005 + s), s = (max - min) / median of the parent's own block medians.

  python tools/optim_groups_bench.py --parent-lib /path/to/parent/libwavjepa_hip.so
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wavjepa_amd import _abi, ops  # noqa: E402
from wavjepa_amd.params import ALIGN, _layout  # noqa: E402

HYPER = dict(beta1=0.9, beta2=0.98, eps=1e-6, max_norm=5.0)
STEP = 1000


def base_layout():
    """slots and flat size of the base model as the launcher builds it (host only: no device buffer is made for it)"""
    import train
    from wavjepa_amd.config import load_config
    from wavjepa_amd.optim import param_groups, resolve_groups
    m, _ = train.build_model(load_config(os.path.join(ROOT, "configs"), ["trainer.size=base"]))
    slots, n = _layout([(k, p) for k, p in m.named_parameters() if p.requires_grad])
    groups = param_groups(m, weight_decay_exclude="1d", lr=4e-4, weight_decay=0.04)
    _, assignment = resolve_groups(m, groups, dict(lr=4e-4, weight_decay=0.04, betas=(0.9, 0.98), eps=1e-6))
    return slots, n, assignment


def byte_map(slots, n, group_of, dev):
    host = torch.empty(n // ALIGN, dtype=torch.uint8)
    for j, s in enumerate(slots):
        host[s.offset // ALIGN:(s.offset + s.numel + ALIGN - 1) // ALIGN] = group_of(j, s)
    return host.to(dev)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", required=True, help="libwavjepa_hip.so of the commit to compare against")
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
    parent.wj_adamw_step.restype, parent.wj_adamw_step.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]
    if parent.wj_abi_version() != _abi.DEFINES["WJ_ABI_VERSION"]:
        raise SystemExit(f"{a.parent_lib}: ABI {parent.wj_abi_version()}, this tree declares {_abi.DEFINES['WJ_ABI_VERSION']}")
    slots, n, assignment = base_layout()
    flips = sum(assignment[x.name] != assignment[y.name] for x, y in zip(slots, slots[1:]))
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=g)
    grad0 = torch.randn(n, device=dev, generator=g) * 1e-2
    grad = grad0.clone()
    m, v = grad0 * 0.1, grad0 * grad0
    p16 = torch.empty(n, dtype=torch.bfloat16, device=dev)
    sumsq = (grad0.double() ** 2).sum().float().reshape(1)
    maps = {"2 groups": (byte_map(slots, n, lambda j, s: assignment[s.name], dev), [4e-4, 4e-4], [0.04, 0.0]),
            "52 groups": (byte_map(slots, n, lambda j, s: j % 52, dev), [4e-4 * 0.98 ** k for k in range(52)], [0.04 * (k % 2) for k in range(52)])}
    stream = torch.cuda.current_stream().cuda_stream
    S = _abi.STRUCTS["wj_adamw_args"]
    common = dict(step=STEP, sumsq=sumsq, p_bf16=p16, zero_grad=True, **HYPER)

    def parent_launch(wg):
        args = S(p=p.data_ptr(), g=grad.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), p_bf16=p16.data_ptr(), sumsq=sumsq.data_ptr(), n=n, lr=4e-4,
                 beta1=HYPER["beta1"], beta2=HYPER["beta2"], eps=HYPER["eps"], weight_decay=0.04, bc1=1.0 - HYPER["beta1"] ** STEP,
                 bc2=1.0 - HYPER["beta2"] ** STEP, max_norm=HYPER["max_norm"], grad_scale=1.0, workgroups=wg, zero_grad=1)
        rc = parent.wj_adamw_step(ctypes.byref(args), stream)
        if rc != 0:
            raise SystemExit(f"the parent's wj_adamw_step returned {rc}")

    def grouped_launch(name, wg):
        gmap, lr, wd = maps[name]
        ops.adamw_groups_step(p, grad, m, v, n, lr=lr, weight_decay=wd, group_map=gmap, first=0, workgroups=wg, **common)

    variants = [("parent wj_adamw_step", parent_launch)] + [(f"wj_adamw_groups_step, {k}", lambda wg, k=k: grouped_launch(k, wg)) for k in maps]
    forms = [("full grid", 0), ("256 workgroups", 256)]
    print(f"base model: n = {n} elements in {len(slots)} slots ({n * 4 / 1e6:.0f} MB per fp32 buffer; the 2-group map changes group at {flips} of "
          f"{len(slots) - 1} slot boundaries); {a.blocks} blocks x {a.reps} launches per variant and form", flush=True)
    for form, wg in forms:                       # warm every launch the timed window uses
        for _, launch in variants:
            launch(wg)
    torch.cuda.synchronize()
    meds = {(label, form): [] for label, _ in variants for form, _ in forms}
    for _ in range(a.blocks):
        for form, wg in forms:
            for label, launch in variants:
                times = []
                for _ in range(a.reps):
                    grad.copy_(grad0)            # (every launch clears the gradient it read: refill outside the timed bracket)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    launch(wg)
                    e1.record()
                    times.append((e0, e1))
                torch.cuda.synchronize()
                meds[(label, form)].append(statistics.median(x.elapsed_time(y) * 1e3 for x, y in times))
    mb = n * 34 / 1e6                            # 28 B of p, g, m, v traffic, 2 B of shadow, 4 B of fused clear per element
    ok = True
    for form, _ in forms:
        base = meds[(variants[0][0], form)]
        pm = statistics.median(base)
        spread = (max(base) - min(base)) / pm
        print(f"{form:15s} {variants[0][0]:32s} median {pm:8.1f} us  ({mb / pm:5.2f} TB/s)  block medians {min(base):.1f} .. {max(base):.1f} us, "
              f"spread {100 * spread:.2f} %")
        for label, _ in variants[1:]:
            gm = statistics.median(meds[(label, form)])
            limit = pm * (1 + 0.005 + spread)
            good = gm <= limit
            ok &= good
            print(f"{form:15s} {label:32s} median {gm:8.1f} us  ({mb / gm:5.2f} TB/s)  {100 * (gm / pm - 1):+.2f} % of the parent, limit "
                  f"{limit:.1f} us: {'within' if good else 'MISSED'}")
    assert bool(torch.isfinite(p).all())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
