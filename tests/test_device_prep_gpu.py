"""wj_audio_prepare on the GPU, through the C ABI, against the float64 references of tests/audio_prep_reference.py; the host side
(DevicePrep, prepare_waveforms, WebAudioDataModule(device_prep=True)) and train.py end to end.

Measured on an MI355X (max |y - same-table ref| / rms over all lengths and both bit depths): see PARITY.md row f3."""
import io
import os
import subprocess
import sys
import tarfile
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_prep_reference as R  # noqa: E402
from wavjepa_amd import audio_prep, ops  # noqa: E402

pytestmark = pytest.mark.gpu
SR, OUT_LEN, GUARD = 16000, 160000, 4096
RATES = [44100, 22050, 11025, 48000, 32000, 24000, 8000, 16000]
SENTINEL = 12345.0


def _call(clips, rate, *, kind=0, out=None, B=None, rows=None, skip_normalize=False, check_guards=True):
    """clips: [(samples 1-D numpy, bits)] of ONE file rate -> the [B][OUT_LEN] rows the entry wrote (NaN where it did not).  Output
    and workspace sit between guard bands that must come back unchanged."""
    dev = torch.device("cuda")
    dtype = {0: np.int16, 1: np.int32, 2: np.float32}[kind]
    B = len(clips) if B is None else B
    rows = list(range(len(clips))) if rows is None else rows
    lengths, offsets, bits = np.zeros(B, np.int32), np.zeros(B, np.int64), np.full(B, 16, np.int32)
    flat, pos = [], 0
    for (x, b), row in zip(clips, rows):
        lengths[row], offsets[row], bits[row] = len(x), pos, b
        flat.append(np.asarray(x).astype(dtype))
        pos += len(x)
    pcm = torch.from_numpy(np.concatenate(flat + [np.zeros(1, dtype)])).to(dev)
    orig, new, width, taps = audio_prep.rate_pair(rate, SR) if rate != SR else (1, 1, 0, 1)
    table = None
    if rate != SR:
        table = torch.from_numpy(R.product_table(rate, SR)[0].astype(np.float32)).to(dev)
        assert table.shape == (new, taps)
    max_len = int(lengths.max())
    dims = dict(B=B, pcm_kind=kind, max_len=max_len, orig=orig, nw=new, width=width, taps=taps, out_len=OUT_LEN)
    need = ops.workspace_bytes("wj_audio_prepare", n_clips=len(rows), table=0 if table is None else 1, **dims)
    ws = torch.full((GUARD + need // 4 + GUARD,), SENTINEL, device=dev)
    if out is None:
        out = torch.full((GUARD + B * OUT_LEN + GUARD,), float("nan"), device=dev)
        out[:GUARD], out[-GUARD:] = SENTINEL, SENTINEL
    ops.audio_prepare(pcm, table, out[GUARD:], ws[GUARD:], offsets=offsets, lengths=lengths, bits=None if kind == 2 else bits,
                      clips=np.asarray(rows, np.int32), pcm_elems=pos, workspace_bytes=need, skip_normalize=skip_normalize, **dims)
    torch.cuda.synchronize()
    if check_guards:
        for t in (out, ws):
            assert bool((t[:GUARD] == SENTINEL).all()) and bool((t[-GUARD:] == SENTINEL).all()), "guard band overwritten"
    return out[GUARD:-GUARD].view(B, OUT_LEN).cpu().numpy(), out


def _lengths(rate):
    taps = audio_prep.rate_pair(rate, SR)[3] if rate != SR else 1
    out = []
    for n in (1, taps - 1, taps, taps + 1, int(0.7 * rate), 10 * rate, int(11.3 * rate)):
        if n >= 1 and n not in out:
            out.append(n)
    return out


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("rate", RATES)
def test_prepare_against_both_references(rate, bits):
    """Every length of one rate in ONE ragged batch (+ a silent clip).  Bounds: same-table reference 1e-5 of the RMS (y and the
    un-scaled r); oracle: d(GPU) <= 1.1 d(CPU product path) + 1e-5, both in units of the RMS."""
    clips = [(R.noise_pcm(n, bits, seed=rate + i, loud_tail=n // 10 if n > 10 * rate else 0)[:, 0], bits) for i, n in enumerate(_lengths(rate))]
    clips.append((np.zeros(int(0.3 * rate), np.int64), bits))
    kind = 0 if bits <= 16 else 1
    y, _ = _call(clips, rate, kind=kind)
    r, _ = _call(clips, rate, kind=kind, skip_normalize=True)
    assert np.isfinite(y).all() and np.isfinite(r).all()
    worst = 0.0
    for b, (x, _) in enumerate(clips[:-1]):
        ref = R.same_table_reference(x, bits, rate, SR, OUT_LEN)
        d = R.distance(y[b], ref)
        worst = max(worst, d)
        print(f"rate {rate} bits {bits} n {len(x)}: same-table y {d:.2e} r {R.distance(r[b], ref, 'r'):.2e}", end="")
        assert R.problems(y[b], ref, r[b]) == [], (rate, bits, len(x))
        if ref["n_valid"] < OUT_LEN:
            assert abs(R.level_db(y[b], ref["n_valid"]) + 14.0) < 0.05
        orc = R.oracle_reference(x, bits, rate, SR, OUT_LEN)
        d_gpu, d_cpu = R.distance(y[b], orc), R.distance(R.cpu_product_path(x, bits, rate, SR, OUT_LEN), orc)
        print(f"   oracle: gpu {d_gpu:.2e} cpu {d_cpu:.2e}")
        assert orc["n_valid"] == ref["n_valid"] and d_gpu <= 1.1 * d_cpu + R.REL_BOUND, (rate, bits, len(x), d_gpu, d_cpu)
    print(f"MAX rate {rate} bits {bits}: {worst:.2e}")
    assert not y[-1].any() and not r[-1].any(), "a silent clip gives zeros"


def test_mixed_rates_equal_single_calls_and_repeat_bit_for_bit():
    clips = [(R.noise_pcm(int((0.4 + 0.05 * i) * rate), 16, seed=100 + i)[:, 0], 16) for i, rate in enumerate(RATES)]
    B = len(RATES)
    mixed = None
    for i, rate in enumerate(RATES):                     # one batch, one call per rate into the same output
        y, mixed = _call([clips[i]], rate, out=mixed, B=B, rows=[i], check_guards=i == B - 1)
    again = None
    for i, rate in enumerate(RATES):
        y2, again = _call([clips[i]], rate, out=again, B=B, rows=[i])
    assert np.isfinite(y).all() and np.array_equal(y.view(np.uint32), y2.view(np.uint32)), "second launch differs"
    for i, rate in enumerate(RATES):
        single, _ = _call([clips[i]], rate)
        assert np.array_equal(single[0].view(np.uint32), y[i].view(np.uint32)), f"row {i} ({rate} Hz) depends on its batch"
    # and several clips of one rate in one call against one call each
    rate = 44100
    three = [(R.noise_pcm(n, 16, seed=n)[:, 0], 16) for n in (30000, 441, 61234)]
    together, _ = _call(three, rate)
    for i in range(3):
        alone, _ = _call([three[i]], rate)
        assert np.array_equal(alone[0].view(np.uint32), together[i].view(np.uint32))


@pytest.mark.parametrize("rate", [32000, 48000, 8000])
def test_resampled_signal_equals_wj_resample_fir_bit_for_bit(rate):
    """Same float input, same table, same tap order (one fmaf chain over k ascending): r before the gain is wj_resample_fir's output."""
    from wavjepa_amd.resample import KAISER_BEST, resample_waveform
    x = np.random.default_rng(rate).uniform(-0.5, 0.5, int(0.9 * rate) + 3).astype(np.float32)
    want = resample_waveform(torch.from_numpy(x).cuda()[None], rate, SR, resampling_method="sinc_interp_kaiser", **KAISER_BEST)[0].cpu().numpy()
    r, _ = _call([(x, 0)], rate, kind=2, skip_normalize=True)
    assert np.array_equal(r[0, :want.shape[0]], want) and not r[0, want.shape[0]:].any()


def test_device_prep_and_prepare_waveforms():
    """The host side: grouping by rate, int16 / int32 / float clips, the two alternating output buffers."""
    batches = []
    for k in range(3):
        items = []
        for i, rate in enumerate((44100, 32000, 16000, 44100)):
            bits = 24 if (i + k) % 2 else 16
            items.append((R.noise_pcm(int(rate * (0.3 + 0.1 * i)), bits, seed=10 * k + i)[:, 0], rate, bits))
        batches.append(items)
    prep = audio_prep.DevicePrep(SR, 10, "cuda")
    outs = []
    for items in batches:
        raw = audio_prep.RawAudioBatch.collate([(x.astype(np.int32 if b > 16 else np.int16), rate, b, audio_prep.PCM, None, None, None)
                                                for x, rate, b in items])
        audio = prep.prepare(raw)[0]
        assert audio.shape == (4, 1, OUT_LEN) and audio.is_cuda and audio.dtype == torch.float32
        outs.append(audio)
    assert outs[0].data_ptr() == outs[2].data_ptr() != outs[1].data_ptr()
    torch.cuda.synchronize()
    for k in (1, 2):                                     # the two live buffers
        for b, (x, rate, bits) in enumerate(batches[k]):
            assert R.problems(outs[k][b, 0].cpu().numpy(), R.same_table_reference(x, bits, rate, SR, OUT_LEN)) == []
    x, rate, bits = batches[0][0]
    f = (x.astype(np.float64) * 2.0 ** -(bits - 1)).astype(np.float32)
    y = audio_prep.prepare_waveforms([(torch.from_numpy(x.astype(np.int16)), rate), (torch.from_numpy(f), rate),
                                      (torch.from_numpy(x.astype(np.int32)), rate, 16)])
    ref = R.same_table_reference(x, bits, rate, SR, OUT_LEN)
    assert y.shape == (3, 1, OUT_LEN)
    for b in range(3):
        assert R.problems(y[b, 0].cpu().numpy(), ref) == []
    assert torch.equal(y[0], y[2])


def test_worker_prepared_clips_are_copied_bit_for_bit():
    """A clip the worker prepared itself (longer than RAW_MAX_SECONDS) travels as its float32 row: the device copies it, beside PCM
    clips of the same batch."""
    long_pcm = R.noise_pcm(int(32000 * 10.6), 16, seed=1, loud_tail=9000)[:, 0]
    row = R.cpu_product_path(long_pcm, 16, 32000, SR, OUT_LEN)
    short = R.noise_pcm(20000, 16, seed=2)[:, 0]
    raw = audio_prep.RawAudioBatch.collate([(short.astype(np.int16), 44100, 16, audio_prep.PCM, None, None, None),
                                            (row, SR, 32, audio_prep.PREPARED, None, None, None),
                                            (short.astype(np.int16), SR, 16, audio_prep.PCM, None, None, None)])
    audio = audio_prep.DevicePrep(SR, 10, "cuda").prepare(raw)[0].cpu().numpy()
    assert np.array_equal(audio[1, 0].view(np.uint32), row.view(np.uint32))
    assert R.problems(audio[0, 0], R.same_table_reference(short, 16, 44100, SR, OUT_LEN)) == []
    assert R.problems(audio[2, 0], R.same_table_reference(short, 16, SR, SR, OUT_LEN)) == []


def _write_shard(path, n_clips, rates, seconds=1.2):
    import flac_encoder as E
    with tarfile.open(path, "w") as tf:
        for i in range(n_clips):
            rate = rates[i % len(rates)]
            n = int(rate * (seconds + 0.1 * i))
            rng = np.random.default_rng(i)
            pcm = np.round(6000 * np.sin(2 * np.pi * (200 + 40 * i) * np.arange(n) / rate) + 500 * rng.standard_normal(n)).astype(np.int64)[:, None]
            data = E.encode(pcm, rate, 16, blocksize=4096, subframes=dict(kind="fixed", order=2, porder=2))
            ti = tarfile.TarInfo(f"clip{i:03d}.flac")
            ti.size = len(data)
            tf.addfile(ti, io.BytesIO(data))


def test_data_module_batches_match_the_default_mode(tmp_path):
    from wavjepa_amd.data import pinned_mask_draws
    from wavjepa_amd.data_modules import WebAudioDataModule
    from wavjepa_amd.masking import TimeInverseBlockMasker
    _write_shard(tmp_path / "shard-000.tar", 6, (44100, 32000, 16000, 22050))

    class DM(WebAudioDataModule):
        SHUFFLE = 4

    def stream(**kw):
        dm = DM(TimeInverseBlockMasker(4, 0.65, 10, 0.25, 10, 0.1), str(tmp_path), None, batch_size=4, nr_samples_per_audio=2,
                nr_time_points=200, sr=SR, seed=3, **kw)
        with pinned_mask_draws(5):
            g = dm._batches(0, 1)
            return [next(g) for _ in range(3)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain, raw = stream(), stream(device_prep=True)
    prep = audio_prep.DevicePrep(SR, 10, "cuda")
    for (audio, ctx, tgt, vis), rb in zip(plain, raw):
        got, c2, t2, v2 = prep.prepare(rb)
        assert torch.equal(ctx, c2) and torch.equal(tgt, t2) and torch.equal(vis, v2)
        got = got.cpu().numpy()
        for b in range(4):
            ref = R.same_table_reference(rb.clip(b).numpy(), int(rb.bits[b]), int(rb.rates[b]), SR, OUT_LEN)
            assert R.problems(got[b, 0], ref) == []
            d_cpu = R.distance(audio[b, 0].numpy(), ref)
            assert np.abs(got[b, 0] - audio[b, 0].numpy()).max() <= (R.REL_BOUND + d_cpu) * ref["rms"]


def test_train_py_runs_with_device_prep(tmp_path):
    """train.py on FLAC shards that include 44.1 kHz clips, workers shipping raw PCM, preparation on the GPU: three steps."""
    shard = tmp_path / "shard-000.tar"
    _write_shard(shard, 6, (44100, 32000, 16000), seconds=2.4)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "train.py"), "data=audioset", f"data.data_dirs={shard}", "data.device_prep=true",
           "trainer.batch_size=2", "trainer.steps=3", "trainer.log_every_n_steps=1", f"save_dir={tmp_path / 'runs'}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    losses = [float(ln.split("loss")[1].split()[0]) for ln in r.stdout.splitlines() if ln.startswith("step ")]
    assert len(losses) >= 3 and all(np.isfinite(losses)) and len(set(losses)) > 1, r.stdout[-1500:]
    assert len(list((tmp_path / "runs" / "saved_models_jepa_new_masking").rglob("last.ckpt"))) == 1
