"""Device-side audio preparation, the parts that need no GPU: the float64 reference helper held to account (it agrees with the
loader's CPU path and rejects mutated candidates), the raw mode of WebAudioDataModule on temporary shards, the argument checks
and workspace query of wj_audio_prepare, and the absence of a CPU fallback."""
import ctypes
import io
import os
import sys
import tarfile
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_prep_reference as R  # noqa: E402
import flac_encoder as E  # noqa: E402
from wavjepa_amd import _abi, audio_prep, ops  # noqa: E402
from wavjepa_amd.data import pinned_mask_draws  # noqa: E402
from wavjepa_amd.data_modules import WebAudioDataModule  # noqa: E402
from wavjepa_amd.masking import TimeInverseBlockMasker  # noqa: E402

SR = 16000


# ------------------------------------------------------------------------------------------------------------ the reference helper
@pytest.mark.parametrize("rate", [44100, 22050, 11025, 48000, 32000, 24000, 8000, 16000])
def test_reference_agrees_with_the_cpu_product_path(rate):
    """same-table reference: the CPU path (float32 matrix product with the same table) within the kernel's own bound; oracle
    reference: within the float32 table's reach -- 1.2e-4 of the RMS was the largest measured (11.025 kHz), <= 2.3e-6 for the pairs
    with one to three phases."""
    out_len = SR                                   # "10 s" shrunk to 1 s: same code, CPU-sized
    pcm = R.noise_pcm(int(rate * 0.7), 16, seed=rate)[:, 0]
    cpu = R.cpu_product_path(pcm, 16, rate, SR, out_len)
    same, orc = R.same_table_reference(pcm, 16, rate, SR, out_len), R.oracle_reference(pcm, 16, rate, SR, out_len)
    d_same, d_orc = R.distance(cpu, same), R.distance(cpu, orc)
    print(f"rate {rate}: cpu vs same-table {d_same:.2e}, cpu vs oracle {d_orc:.2e}")
    assert same["n_valid"] == orc["n_valid"] == -(-SR * pcm.shape[0] // rate)
    assert R.problems(cpu, same) == []
    assert d_orc < (3e-4 if rate in (44100, 22050, 11025) else 1e-5)
    assert abs(R.level_db(same["y"], same["n_valid"]) + 14.0) < 1e-9


def test_reference_rejects_mutated_candidates():
    rate, out_len, bits = 44100, SR, 16
    n = int(rate * 1.13)                                                    # "11.3 s" against a 1 s window, loud tail
    stereo = R.noise_pcm(n, bits, seed=5, channels=2, loud_tail=int(rate * 0.1))
    pcm = stereo[:, 0]
    ref = R.same_table_reference(pcm, bits, rate, SR, out_len)
    assert R.problems(ref["y"].astype(np.float32), ref, ref["r"].astype(np.float32)) == []
    short = R.same_table_reference(pcm[:int(rate * 0.5)], bits, rate, SR, out_len)      # a clip with padding
    assert R.problems(short["y"].astype(np.float32), short) == []

    head = R.same_table_reference(pcm, bits, rate, SR, out_len, rms_over="head")
    assert R.problems(head["y"], ref, head["r"]), "RMS over the first window only"
    ch1 = R.same_table_reference(stereo[:, 1], bits, rate, SR, out_len)
    assert R.problems(ch1["y"], ref, ch1["r"]), "channel 1"
    half = R.same_table_reference(pcm, bits, rate, SR, out_len, scale_bits=bits)
    assert R.problems(half["y"], ref) == [] and R.problems(half["y"], ref, half["r"]), "scale 2^-bits (the gain hides it in y: r shows it)"
    pad = short["y"].copy()
    pad[-1] = 1e-30
    assert R.problems(pad, short) == ["padding is not exactly 0.0"]
    assert R.problems(np.roll(ref["y"], 1), ref) and R.problems(np.roll(short["y"], 1), short), "shifted by one sample"
    swapped = R.same_table_reference(pcm, bits, rate, SR, out_len, swap_phase=7)
    assert R.problems(swapped["y"], ref, swapped["r"]), "phase 7 computed with the row of phase 8"
    nan = ref["y"].copy()
    nan[3] = np.nan
    assert "not finite" in R.problems(nan, ref)


# ------------------------------------------------------------------------------------------------------------ raw mode of the data module
def make_shard(path, clips):
    with tarfile.open(path, "w") as tf:
        for key, data in clips:
            ti = tarfile.TarInfo(f"{key}.flac")
            ti.size = len(data)
            tf.addfile(ti, io.BytesIO(data))


@pytest.fixture()
def shards(tmp_path):
    """-> (directory, {key: (pcm [n, ch], rate, bits)}): rates 16 / 22.05 / 32 / 44.1 kHz, mono and stereo, 16 and 24 bits, a silent
    clip, a truncated member, one clip longer than RAW_MAX_SECONDS (of the test's subclass: 2 s)."""
    spec = [("c00", 16000, 1, 16, 0.6), ("c01", 22050, 2, 16, 0.7), ("c02", 32000, 1, 24, 0.8), ("c03", 44100, 2, 24, 0.9),
            ("c04", 44100, 1, 16, 0.5), ("c05", 32000, 2, 16, 1.1), ("long", 32000, 1, 16, 2.5)]
    clips, truth = [], {}
    for i, (key, rate, ch, bits, sec) in enumerate(spec):
        pcm = R.noise_pcm(int(rate * sec), bits, seed=i, channels=ch) // 4
        truth[key] = (pcm, rate, bits)
        clips.append((key, E.encode(pcm, rate, bits, blocksize=4096, stereo="mid_side" if ch == 2 else "independent",
                                    subframes=dict(kind="fixed", order=1, porder=2))))
    truth["silent"] = (np.zeros((8000, 1), np.int64), 16000, 16)
    clips.append(("silent", E.encode(truth["silent"][0], 16000, 16, subframes=dict(kind="constant"))))
    clips.append(("broken", clips[0][1][:300]))
    make_shard(tmp_path / "shard-000.tar", clips[:5])
    make_shard(tmp_path / "shard-001.tar", clips[5:])
    return tmp_path, truth


class DM(WebAudioDataModule):
    SHUFFLE, NUM_WORKERS, PREFETCH_FACTOR, RAW_MAX_SECONDS = 4, 2, 1, 2


def _dm(path, **kw):
    masker = TimeInverseBlockMasker(4, 0.65, 10, 0.25, 10, 0.1)
    dm = DM(masker, str(path), None, batch_size=3, nr_samples_per_audio=2, nr_time_points=200, sr=SR, seed=7, **kw)
    dm.setup("fit")
    return dm


def _identify(clip: np.ndarray, rate: int, truth):
    for key, (pcm, r, bits) in truth.items():
        if r == rate and pcm.shape[0] == clip.shape[0] and np.array_equal(pcm[:, 0], clip):
            return key, bits
    return None, None


def test_device_prep_is_off_by_default_and_returns_a_plain_dataloader(shards):
    from torch.utils.data import DataLoader
    path, _ = shards
    dm = _dm(path)
    assert dm.device_prep is False and type(dm.train_dataloader()) is DataLoader
    on = _dm(path, device_prep=True).train_dataloader()
    assert isinstance(on, audio_prep.DevicePrepLoader) and type(on.loader) is DataLoader


def test_raw_mode_ships_channel_0_pcm_and_the_same_masks(shards, monkeypatch):
    path, truth = shards
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pinned_mask_draws(11):
            g = _dm(path)._batches(0, 1)
            plain = [next(g) for _ in range(5)]
        # raw mode: the resampler may run for the over-long clip only
        M = sys.modules["wavjepa_amd.data_modules.WebAudioDataModule"]
        real, tripped = M.resample_waveform_cpu, []

        def guarded(wav, orig, new, **kw):
            tripped.append(int(wav.shape[-1]))
            return real(wav, orig, new, **kw)
        monkeypatch.setattr(M, "resample_waveform_cpu", guarded)
        with pinned_mask_draws(11):
            g = _dm(path, device_prep=True)._batches(0, 1)
            raw = [next(g) for _ in range(5)]
    seen = set()
    for (audio, ctx, tgt, vis), rb in zip(plain, raw):
        assert isinstance(rb, audio_prep.RawAudioBatch) and len(rb) == 3
        assert torch.equal(ctx, rb.ctx) and torch.equal(tgt, rb.tgt) and torch.equal(vis, rb.vis)
        for b in range(3):
            rate, clip = int(rb.rates[b]), rb.clip(b).numpy()
            if int(rb.prepared[b]):
                # the over-long clip: prepared by the worker, bit-identical to the default mode's row
                assert rate == SR and clip.dtype == np.float32 and np.array_equal(clip, audio[b, 0].numpy())
                seen.add("long")
                continue
            key, bits = _identify(clip, rate, truth)
            assert key is not None and key != "long" and int(rb.bits[b]) == bits, (b, rate, clip.shape)
            assert clip.dtype == (np.int32 if rb.pcm.dtype == torch.int32 else np.int16)
            seen.add(key)
            # same clip order as the default mode: its row is this clip prepared on the CPU
            want = R.cpu_product_path(truth[key][0][:, 0], bits, rate, SR, 10 * SR)
            assert np.array_equal(want, audio[b, 0].numpy()), key
        wide = any(int(rb.bits[b]) > 16 and not int(rb.prepared[b]) for b in range(3))
        assert rb.pcm.dtype == (torch.int32 if wide else torch.int16)
    assert {"long", "silent"} <= seen and len(seen) >= 6, seen
    assert tripped and set(tripped) == {truth["long"][0].shape[0]}, tripped


def test_raw_batches_travel_through_worker_processes(shards):
    path, truth = shards
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        it = iter(_dm(path, device_prep=True).train_dataloader().loader)        # the DataLoader itself: two worker processes
        batches = [next(it) for _ in range(4)]
        del it
    for rb in batches:
        assert isinstance(rb, audio_prep.RawAudioBatch) and len(rb) == 3 and rb.ctx.shape == (3, 2, 200)
        for b in range(3):
            if not int(rb.prepared[b]):
                assert _identify(rb.clip(b).numpy(), int(rb.rates[b]), truth)[0] is not None
    assert hasattr(batches[0], "pin_memory")


# ------------------------------------------------------------------------------------------------------------ C ABI without a GPU
def _args(**over):
    a = _abi.STRUCTS["wj_audio_prepare_args"]()
    keep = dict(offsets=np.zeros(2, np.int64), lengths=np.array([100, 50], np.int32), bits=np.array([16, 16], np.int32),
                clips=np.array([0, 1], np.int32))
    keep["offsets"][1] = 100
    fields = dict(pcm=0x1000, table=0x2000, out=0x3000, workspace=0x4000, pcm_elems=150, workspace_bytes=1 << 20, B=2, n_clips=2,
                  pcm_kind=0, max_len=100, orig=2, nw=1, width=136, taps=274, out_len=1000, skip_normalize=0)
    for k, v in over.items():
        if k in keep:
            keep[k] = v
        else:
            fields[k] = v
    for k, v in keep.items():
        setattr(a, k, 0 if v is None else v.ctypes.data)
    for k, v in fields.items():
        setattr(a, k, v)
    return a, keep


def test_wj_audio_prepare_argument_errors_and_workspace_query():
    lib = _abi.load()
    assert "wj_audio_prepare" in _abi.FUNCTIONS and lib.wj_struct_size(b"wj_audio_prepare_args") == ctypes.sizeof(_abi.STRUCTS["wj_audio_prepare_args"])
    assert _abi.DEFINES["WJ_ABI_VERSION"] == 17

    def rc(**over):
        a, keep = _args(**over)
        return lib.wj_audio_prepare(ctypes.byref(a), None)
    assert lib.wj_audio_prepare(None, None) == -1
    for bad in (dict(pcm=0), dict(out=0), dict(workspace=0), dict(offsets=None), dict(lengths=None), dict(bits=None), dict(clips=None),
                dict(B=0), dict(n_clips=0), dict(out_len=0), dict(taps=273), dict(width=-1), dict(orig=0), dict(nw=0), dict(pcm_kind=3),
                dict(clips=np.array([0, 2], np.int32)), dict(clips=np.array([-1, 1], np.int32)),
                dict(bits=np.array([16, 7], np.int32)), dict(bits=np.array([33, 16], np.int32)), dict(bits=np.array([24, 16], np.int32)),
                dict(lengths=np.array([101, 50], np.int32)), dict(pcm_elems=149), dict(workspace_bytes=4),
                dict(table=0)):                                   # no table needs orig == nw
        assert rc(**bad) == -1, bad
    # beyond the table limits: unsupported, not an argument error
    assert rc(nw=1025) == -3
    assert rc(orig=4000, width=100, taps=4200) == -3
    # the workspace query: grows with the longest clip and the clip count, -1 for dimensions the entry refuses
    small = ops.workspace_bytes("wj_audio_prepare", table=1, n_clips=2, B=2, max_len=100, orig=2, nw=1, width=136, taps=274, out_len=1000)
    big = ops.workspace_bytes("wj_audio_prepare", table=1, n_clips=32, B=32, max_len=441000, orig=441, nw=160, width=187, taps=815, out_len=160000)
    assert 0 < small < big < 1 << 20 and big % 4 == 0
    a, _ = _args(taps=273)
    assert lib.wj_workspace_bytes(b"wj_audio_prepare", ctypes.byref(a)) == -1
    assert audio_prep.rate_pair(44100, 16000) == (441, 160, 187, 815) and audio_prep.device_supports(44100, 16000)
    assert not audio_prep.device_supports(44101, 16000)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the no-GPU behaviour")
def test_no_cpu_fallback():
    rb = audio_prep.RawAudioBatch.collate([(np.zeros(100, np.int16), 32000, 16, audio_prep.PCM, None, None, None)])
    with pytest.raises((_abi.WavJepaHipError, RuntimeError)):
        audio_prep.DevicePrep(SR).prepare(rb)
    with pytest.raises((_abi.WavJepaHipError, RuntimeError)):
        audio_prep.prepare_waveforms([(torch.zeros(100, dtype=torch.int16), 32000)])
