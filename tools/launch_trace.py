#!/usr/bin/env python3
"""What does the HOST issue for one step?  One line per host-side event, in issue order, for a list of small cases (each on a freshly
built model): every library launch with the scalar fields of its argument struct and every pointer field replaced by the ordinal of that
value's first appearance in the case (addresses differ from process to process, the order in which buffers are first touched does not);
the members of the array-carrying entries (wj_wgrad_grouped, wj_colsum_f32_group, ...) the same way; every event record / wait.  Each
line names the stream it went to (main / side / upload / other).  A case ends with `== <case>: <events> events, sha256 <hash>`; the
WJ_DETERMINISTIC=1 cases add the sha256 of the loss bytes and of flat.g32 after the backward, the stand-alone extractor forwards that
of their tokens.

Two trees issue the same step exactly when these hashes agree: run this file unchanged in both (it uses only what `ops._run` and the
array-carrying wrappers end in -- `_abi.call` -- and the `build` / `build_pre` / `build_ln` / `masks` / `clips` helpers of the GPU tests) and diff the
outputs.  `--summary` prints the `==` lines only; a substring argument selects cases."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path[:0] = [ROOT, GOLDEN]
import synth  # noqa: E402
from tests import test_denoiser_gpu as TD  # noqa: E402
from tests.test_conv_layernorm_gpu import build_ln  # noqa: E402
from tests.test_jepa_gpu import BASE, SMALL, PinnedRng, build, dev  # noqa: E402
from tests.test_prenorm_gpu import build_pre, clips, masks  # noqa: E402
from wavjepa_amd import _abi, engine as E  # noqa: E402


class Trace:
    """Hooks `_abi.call` and the event calls of torch.cuda while active; `lines` is the case's trace."""

    def __init__(self, eng):
        self.lines, self.ptrs, self.events, self.keep = [], {}, {}, []
        self.streams = {torch.cuda.current_stream(dev()).cuda_stream: "main", eng.side.cuda_stream: "side"}
        self.eng = eng

    def stream(self, s) -> str:
        h = s if isinstance(s, int) else (torch.cuda.current_stream() if s is None else s).cuda_stream
        if h not in self.streams:
            up = {u.cuda_stream for u in E._UPLOAD_STREAMS.values()}
            self.streams[h] = "upload" if h in up else "other"
        return self.streams[h]

    def ptr(self, v) -> str:
        return "0" if not v else "p%d" % self.ptrs.setdefault(int(v), len(self.ptrs) + 1)

    def event(self, ev) -> str:
        if id(ev) not in self.events:
            self.events[id(ev)] = len(self.events) + 1
            self.keep.append(ev)                       # (a collected event's id may come back for a new one)
        return "e%d" % self.events[id(ev)]

    def field(self, name, ctype, v, n) -> str:
        if issubclass(ctype, ctypes.Array):            # array-carrying entries: the first `n` members
            one = self.ptr if ctype._type_ is ctypes.c_void_p else repr
            return "%s=[%s]" % (name, ",".join(one(x) for x in list(v)[:n]))
        return "%s=%s" % (name, self.ptr(v) if ctype is ctypes.c_void_p else repr(v))

    def launch(self, fn, a, stream) -> None:
        n = getattr(a, "n", None)
        self.lines.append("%s %s %s" % (self.stream(int(stream or 0)), fn,
                                        " ".join(self.field(k, t, getattr(a, k), n) for k, t in a._fields_)))

    def __enter__(self):
        self.saved = (_abi.call, torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream)
        call, record, wait_event, wait_stream = self.saved
        tr = self

        def traced_call(fn, a, stream, lab=False):
            tr.launch(fn, a, stream)
            return call(fn, a, stream, lab=lab)

        def traced_record(ev, stream=None):
            tr.lines.append("%s record %s" % (tr.stream(stream), tr.event(ev)))
            return record(ev) if stream is None else record(ev, stream)

        def traced_wait_event(s, ev):
            tr.lines.append("%s wait_event %s" % (tr.stream(s), tr.event(ev)))
            return wait_event(s, ev)

        def traced_wait_stream(s, other):
            tr.lines.append("%s wait_stream %s" % (tr.stream(s), tr.stream(other)))
            return wait_stream(s, other)
        _abi.call, torch.cuda.Event.record = traced_call, traced_record
        torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream = traced_wait_event, traced_wait_stream
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        _abi.call, torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream = self.saved


def sha(t) -> str:
    t = t.detach().contiguous()
    return hashlib.sha256((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().tobytes()).hexdigest()


def two_channel_batch():
    """3 two-channel clips of 16000 samples (198 tokens) with channel-based masks: test_conv_layernorm_channel_extractor's."""
    from wavjepa_amd.masking import TimeInverseBlockMasker
    with PinnedRng(4100):
        ctx, tgt, vis = TimeInverseBlockMasker(4, 0.65, 10, 0.25, 10, 0.1, channel_based_masking=True, channel_major=True)(
            batch_size=3, n_times=198, in_channels=2)
    return torch.from_numpy(synth.synth_audio(3, 2, 16000, seed=31)).to(torch.bfloat16).to(dev()), ctx, tgt, vis


def build_case(layout, cfg, conv_bias=None, channels=None, **kw):
    """conv_bias None: mode "default", else mode "layer_norm" with / without conv bias; channels "own" / "shared": two-channel extractor."""
    if channels is not None:
        kw.update(seconds=1.0, tokens=198, in_channels=2, channel_stacks=channels)
    builder = build if layout == "post" else (lambda c, **k: build_pre(c, layout, **k))
    return builder(cfg, **kw) if conv_bias is None else build_ln(cfg, conv_bias, builder=builder, **kw)


def jepa_step(layout, cfg=SMALL, ragged=True, env=None, infer=False, fp8=False, conv_bias=None, channels=None):
    """One case: a fresh model (built, engine and side stream included, before the trace starts), then one training step or inference."""
    def run():
        kw = {}
        if fp8:                                         # the configuration of test_fp8_forward_path_base_model_400_tokens_vs_bf16_path
            kw = dict(seconds=4.01, tokens=400)
            fx = dict(np.load(os.path.join(GOLDEN, "masks.npz")))
            ctx, tgt, vis = (torch.from_numpy(fx[k][:2]) for k in ("as400_ctx", "as400_tgt", "as400_vis"))
            audio = torch.from_numpy(synth.synth_audio(2, 1, 64160, seed=41)).to(torch.bfloat16).to(dev())
        elif infer:
            audio = torch.from_numpy(synth.synth_audio(3, 1, 32159, seed=9)).to(dev())
            pad = torch.zeros(3, 200, dtype=torch.bool)
            pad[1, 150:] = True
        elif channels is not None:
            audio, ctx, tgt, vis = two_channel_batch()
        else:
            ctx, tgt, vis = masks(GOLDEN, 4)
            audio = clips(4)
        m, _ = build_case(layout, cfg, conv_bias, channels, **kw)
        eng = m._ensure_engine()
        eng.ragged, eng.fp8 = ragged, fp8
        extra = []
        with Trace(eng) as tr:
            if infer:
                for mask in (pad.to(dev()), None):
                    m.get_audio_representation(audio, mask)
            else:
                out = m(audio, ctx, tgt, vis)
                out["loss"].backward()
                assert eng.ragged_step == ragged
        if eng.deterministic and not infer:
            extra = ["loss sha256 " + sha(out["loss"]), "g32 sha256 " + sha(m._flat.g32)]
        return tr.lines, extra
    return run, env or {}


def denoiser_step():
    def run():
        den, _, _ = TD.build()
        clean = torch.from_numpy(synth.synth_audio(3, 1, 32159, seed=41)).to(torch.bfloat16).to(dev())
        noise = torch.from_numpy(synth.synth_audio(3, 1, 32159, seed=42)).to(dev())
        generated = (clean.float() + 0.5 * noise).to(torch.bfloat16)
        den.teacher._ensure_engine()
        with Trace(den._ensure_engine()) as tr:
            den(generated, clean)["loss"].backward()
        return tr.lines, []
    return run, {}


def standalone_forward(conv_bias=None, channels=None):
    """The extractor's own forward, m.extract_audio(audio), outside the engine; adds the sha256 of the tokens."""
    def run():
        audio = clips(3) if channels is None else two_channel_batch()[0]
        m, _ = build_case("post", SMALL, conv_bias, channels)
        with Trace(m._ensure_engine()) as tr:
            tok = m.extract_audio(audio)
        return tr.lines, ["tokens sha256 " + sha(tok)]
    return run, {}


CASES = {}
for lay in ("post", "both"):
    CASES[f"{lay} ragged"] = jepa_step(lay)
    CASES[f"{lay} dense"] = jepa_step(lay, ragged=False)
for lay in ("dec", "enc"):
    CASES[f"{lay} ragged"] = jepa_step(lay)
for lay in ("post", "both"):
    for switch in ("WJ_TRIM_TAIL=0", "WJ_SIDE_STREAM=0", "WJ_DEFER_FOLDS=0", "WJ_DETERMINISTIC=1"):
        CASES[f"{lay} {switch}"] = jepa_step(lay, env=dict([switch.split("=")]))
    for top_k in (1, 8):
        CASES[f"{lay} top_k={top_k}"] = jepa_step(lay, cfg=dict(SMALL, top_k=top_k))
    CASES[f"{lay} inference"] = jepa_step(lay, infer=True)
# the conv front-end: mode "layer_norm", the conv switches, the two-channel extractor, the stand-alone forward
for bias in (True, False):
    CASES[f"layer_norm ragged bias={bias}"] = jepa_step("post", conv_bias=bias)
    CASES[f"layer_norm dense bias={bias}"] = jepa_step("post", ragged=False, conv_bias=bias)
for switch in ("WJ_DETERMINISTIC=1", "WJ_SIDE_STREAM=0"):
    CASES[f"layer_norm {switch}"] = jepa_step("post", env=dict([switch.split("=")]), conv_bias=True)
for switch in ("WJ_SPARSE_CONV=0", "WJ_CONV_WGRAD_SIDE=0"):
    CASES[f"post {switch}"] = jepa_step("post", env=dict([switch.split("=")]))
    CASES[f"layer_norm {switch}"] = jepa_step("post", env=dict([switch.split("=")]), conv_bias=True)
for switch in ("WJ_FUSE_CONV_GELU_BWD=0", "WJ_FUSE_ADD_POS=0"):
    CASES[f"post {switch}"] = jepa_step("post", env=dict([switch.split("=")]))
for mode, bias in (("default", None), ("layer_norm", True)):
    for stacks in ("own", "shared"):
        CASES[f"{mode} two-channel {stacks}"] = jepa_step("post", conv_bias=bias, channels=stacks)
        CASES[f"{mode} stand-alone two-channel {stacks}"] = standalone_forward(bias, stacks)
    CASES[f"{mode} stand-alone mono"] = standalone_forward(bias)
CASES["layer_norm two-channel own WJ_DETERMINISTIC=1"] = jepa_step("post", env={"WJ_DETERMINISTIC": "1"}, conv_bias=True, channels="own")
CASES["post fp8"] = jepa_step("post", cfg=BASE, fp8=True)
CASES["denoiser"] = denoiser_step()


def main() -> None:
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    summary = "--summary" in sys.argv
    for name, (run, env) in CASES.items():
        if args and not any(a in name for a in args):
            continue
        os.environ.update(env)
        try:
            lines, extra = run()
        finally:
            for k in env:
                del os.environ[k]
        if not summary:
            for ln in lines:
                print(f"{name}: {ln}")
        print(f"== {name}: {len(lines)} events, sha256 {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}"
              + "".join("; " + e for e in extra), flush=True)


if __name__ == "__main__":
    main()
