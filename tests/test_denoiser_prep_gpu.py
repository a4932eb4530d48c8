"""wj_noise_prepare on the GPU, through the C ABI, against the float64 reference of tests/noise_prep_reference.py (bound 2e-6 of the
RMS, derived there); the host side (DenoiserDevicePrep, WebAudioDataModuleDenoiser(device_prep=True)), the denoiser's batch hook
on a device-prepared batch, and denoise.py end to end.

Measured on an MI355X (max |y - reference| / rms): see PARITY.md row f4."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_prep_reference as RA  # noqa: E402
import noise_prep_reference as R  # noqa: E402
from wavjepa_amd import audio_prep, ops  # noqa: E402

pytestmark = pytest.mark.gpu
T, F, GUARD = R.T_SMALL, R.F_SMALL, 4096
SR, OUT_LEN, FADE = 32000, 320000, 6400
SENTINEL = 12345.0


def _call(cases, *, out_len=T, fade_len=F, out=None, B=None, rows=None, lead=0):
    """cases: [(name, clip, cut_start, place_start)] -> the [B][out_len] rows the entry wrote (NaN where it did not), and the
    buffer.  Output and workspace sit between guard bands that must come back unchanged.  `lead`: floats in front of the first
    clip in the flat buffer (moves every clip's alignment)."""
    dev = torch.device("cuda")
    B = len(cases) if B is None else B
    rows = list(range(len(cases))) if rows is None else rows
    lengths, offsets = np.zeros(B, np.int32), np.zeros(B, np.int64)
    cuts, places = np.zeros(B, np.int32), np.zeros(B, np.int32)
    flat, pos = [np.full(lead, 7.0, np.float32)], lead
    for (_, x, cut, place), row in zip(cases, rows):
        lengths[row], offsets[row], cuts[row], places[row] = len(x), pos, cut, place
        flat.append(np.asarray(x, np.float32))
        pos += len(x)
    noise = torch.from_numpy(np.concatenate(flat + [np.full(1, 7.0, np.float32)])).to(dev)
    dims = dict(B=B, max_len=int(lengths.max()), out_len=out_len, fade_len=fade_len)
    need = ops.workspace_bytes("wj_noise_prepare", n_clips=len(rows), **dims)
    ws = torch.full((GUARD + need // 4 + GUARD,), SENTINEL, device=dev)
    if out is None:
        out = torch.full((GUARD + B * out_len + GUARD,), float("nan"), device=dev)
        out[:GUARD], out[-GUARD:] = SENTINEL, SENTINEL
    ops.noise_prepare(noise, out[GUARD:], ws[GUARD:], offsets=offsets, lengths=lengths, cut_start=cuts, place_start=places,
                      clips=np.asarray(rows, np.int32), noise_elems=pos, workspace_bytes=need, **dims)
    torch.cuda.synchronize()
    for t in (out, ws):
        assert bool((t[:GUARD] == SENTINEL).all()) and bool((t[-GUARD:] == SENTINEL).all()), "guard band overwritten"
    return out[GUARD:-GUARD].view(B, out_len).cpu().numpy(), out


def test_every_edge_case_in_one_ragged_batch_against_the_reference():
    cases = R.edge_cases()
    y, _ = _call(cases)
    worst = 0.0
    for b, (name, x, cut, place) in enumerate(cases):
        ref = R.reference(x, F, T, cut, place)
        d = R.distance(np.nan_to_num(y[b]), ref)
        worst = max(worst, d)
        print(f"{name}: {d:.2e} of the RMS")
        assert R.problems(y[b], ref) == [], name
    print(f"MAX edge cases: {worst:.2e}")
    assert cases[-1][0] == "silent" and np.isfinite(y[-1]).all() and not y[-1].any(), "a silent clip gives zeros, no NaN"


def test_unlisted_rows_single_calls_and_a_second_launch():
    cases = R.edge_cases()
    B = len(cases) + 1
    rows = [b for b in range(B) if b != 3]                               # row 3 belongs to no clip
    together, buf = _call(cases, B=B, rows=rows)
    assert np.isnan(together[3]).all(), "a row no call lists was written"
    again, _ = _call(cases, B=B, rows=rows)
    keep = np.asarray(rows)
    assert np.array_equal(together[keep].view(np.uint32), again[keep].view(np.uint32)), "second launch differs"
    for lead in (0, 1, 2, 3):                                            # a call of its own, at every alignment of the source
        for case, row in zip(cases, rows):
            alone, _ = _call([case], lead=lead)
            assert np.array_equal(alone[0].view(np.uint32), together[row].view(np.uint32)), (case[0], lead)
    # the same row filled by two calls into one output
    half, buf2 = _call(cases[:5], B=B, rows=rows[:5])
    both, _ = _call(cases[5:], B=B, rows=rows[5:], out=buf2)
    assert np.array_equal(both[keep].view(np.uint32), together[keep].view(np.uint32)) and np.isnan(both[3]).all()


def test_real_size_rows():
    """10 s rows at 32 kHz, 0.2 s fades: one clip shorter (placed), one longer (cut) -- several workgroups per clip in both passes."""
    cases = [("200000 placed", R.noise_clip(200000, 21), 0, 119999), ("700000 cut", R.noise_clip(700000, 22, loud=(0, 100000)), 123457, 0)]
    y, _ = _call(cases, out_len=OUT_LEN, fade_len=FADE)
    for b, (name, x, cut, place) in enumerate(cases):
        ref = R.reference(x, FADE, OUT_LEN, cut, place)
        print(f"{name}: {R.distance(np.nan_to_num(y[b]), ref):.2e} of the RMS")
        assert R.problems(y[b], ref) == [], name


# ------------------------------------------------------------------------------------------------------------ module and hook
@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    return R.make_denoiser_shards(str(tmp_path_factory.mktemp("denoiser_shards")))


def _stream(shards, n, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g = R.denoiser_module(shards, **kw)._batches(0, 1)
        return [next(g) for _ in range(n)]


def test_device_prepared_batches_match_the_default_mode(shards):
    plain, raw = _stream(shards, 3), _stream(shards, 3, device_prep=True)
    prep = audio_prep.DenoiserDevicePrep(SR, 10, "cuda")
    outs = []
    for (audio, srir, noise, length, start, nrirs, snr), rb in zip(plain, raw):
        got = prep.prepare(rb)
        outs.append(got[0])
        assert len(got) == 7 and all(isinstance(t, torch.Tensor) and t.is_cuda for t in got)
        a, s, nz, ln, st, nr, sn = got
        assert a.shape == (3, OUT_LEN) and nz.shape == (3, OUT_LEN) and a.dtype == nz.dtype == torch.float32
        assert torch.equal(ln.cpu(), length) and torch.equal(st.cpu(), start) and torch.equal(sn.cpu(), snr)
        assert torch.equal(s.cpu(), srir) and torch.equal(nr.cpu(), nrirs)
        a, nz = a.cpu().numpy(), nz.cpu().numpy()
        for b in range(3):
            ref = RA.same_table_reference(rb.clean.clip(b).numpy(), int(rb.clean.bits[b]), int(rb.clean.rates[b]), SR, OUT_LEN)
            assert RA.problems(a[b], ref) == []
            nref = R.reference(rb.noise_clip(b).numpy(), FADE, OUT_LEN, int(rb.cut_start[b]), int(rb.place_start[b]))
            assert R.problems(nz[b], nref) == []
            assert R.problems(noise[b].numpy(), nref) == []            # the default mode's row: same draws
    assert outs[0].data_ptr() == outs[2].data_ptr() != outs[1].data_ptr()      # two alternating buffers


@pytest.mark.parametrize("with_noise,with_rir", [(True, True), (False, True), (False, False)])
def test_batch_hook_on_a_device_prepared_batch_equals_the_plain_tuple(shards, with_noise, with_rir):
    """Denoiser.on_after_batch_transfer on what DenoiserDevicePrep hands out, and on a plain CPU tuple rebuilt from the same prepared
    tensors: bit-identical (generated, clean) -- field order, dtypes, views and stream ordering of the new plumbing.  (Noise without
    RIRs is not a case of the hook in either mode: add_noise takes the [B, C, T] source a RIR convolution makes.)"""
    from wavjepa_amd.denoiser import Denoiser
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    torch.manual_seed(0)
    den = Denoiser(ConvFeatureExtractor(conv_layers_spec=[(64, 10, 5)] + [(64, 3, 2)] * 4 + [(64, 2, 2)], in_channels=1),
                   TransformerLayerCFG.create(d_model=128, nhead=2), TransformerEncoderCFG.create(num_layers=2), nr_samples_per_audio=2).to("cuda")
    raw = _stream(shards, 2, device_prep=True, with_noise=with_noise, with_rir=with_rir)
    loader = audio_prep.DevicePrepLoader(raw, audio_prep.DenoiserDevicePrep(SR, 10, "cuda"))
    for k, batch in enumerate(loader):
        plain = tuple(t.cpu().clone() if isinstance(t, torch.Tensor) else t for t in batch)
        for t, on in ((batch[1], with_rir), (batch[2], with_noise), (batch[5], with_noise and with_rir), (batch[6], with_noise)):
            assert isinstance(t, torch.Tensor) if on else t == [None] * 3
        torch.manual_seed(100 + k)
        gen, clean = den.on_after_batch_transfer(batch, 0)
        torch.manual_seed(100 + k)
        gen2, clean2 = den.on_after_batch_transfer(plain, 0)
        assert gen.shape == clean.shape == (3 * 2, 1, den.target_length) and gen.dtype == clean.dtype == torch.bfloat16
        assert torch.equal(gen, gen2) and torch.equal(clean, clean2)
        assert bool(torch.isfinite(gen.float()).all()) and (with_noise or with_rir) == (not torch.equal(gen, clean))


def test_denoise_py_runs_with_device_prep(tmp_path):
    """The twin of test_denoiser_gpu.py::test_denoise_py_runs_end_to_end with data.device_prep=true: worker processes ship raw
    batches, both clips are prepared on the GPU, three optimisation steps with finite losses."""
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.jepa import JEPA
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    sh = R.make_denoiser_shards(str(tmp_path), rates=(32000, 44100, 16000, 32000))
    torch.manual_seed(0)
    tea = JEPA(feature_extractor=ConvFeatureExtractor(conv_layers_spec=[(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)], in_channels=1),
               transformer_encoder_cfg=TransformerEncoderCFG.create(), transformer_encoder_layers_cfg=TransformerLayerCFG.create(),
               transformer_decoder_cfg=TransformerEncoderCFG.create(), transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=384),
               process_audio_seconds=2.01)
    sd = {k.replace("encoder.", "encoder._orig_mod.", 1) if k.startswith("encoder.") else k: v for k, v in tea.state_dict().items()}
    ckpt = tmp_path / "teacher.ckpt"
    torch.save({"state_dict": sd, "hyper_parameters": {}, "global_step": 375000}, ckpt)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "denoise.py"), f"data.data_dir={sh['audio']}", f"data.rir_dir={sh['rir']}",
           f"data.noise_dir={sh['noise']}", f"trainer.teacher_ckpt_weights={ckpt}", "data.device_prep=true", "trainer.batch_size=2",
           "trainer.steps=3", "trainer.log_every_n_steps=1", f"save_dir={tmp_path / 'runs'}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    losses = [float(ln.split("loss")[1].split()[0]) for ln in r.stdout.splitlines() if ln.startswith("step ")]
    assert len(losses) >= 3 and all(np.isfinite(losses)), r.stdout[-1500:]
    assert 0.0 < losses[0] < 1.5, losses                  # the student starts from the teacher: only the scene's distance remains
    saved = [p for p in (tmp_path / "runs").rglob("last.ckpt")]
    assert saved and "state_dict" in torch.load(saved[0], weights_only=False)
