"""Device-side preparation of the denoiser stage, the parts that need no GPU: the float64 reference helper held to account (the
loader's CPU path passes it, mutated candidates do not), the argument checks and workspace query of wj_noise_prepare, the raw mode
of WebAudioDataModuleDenoiser on temporary shards (same draws as the default mode for one seed), and the absence of a CPU fallback."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_prep_reference as RA  # noqa: E402
import noise_prep_reference as R  # noqa: E402
from wavjepa_amd import _abi, audio_prep, ops  # noqa: E402

T, F = R.T_SMALL, R.F_SMALL


# ------------------------------------------------------------------------------------------------------------ the reference helper
def test_cpu_plain_path_passes_the_reference_on_every_edge_case():
    worst = 0.0
    for name, x, cut, place in R.edge_cases():
        ref = R.reference(x, F, T, cut, place)
        y = R.cpu_plain_path(x, F, T, cut, place)
        d = R.distance(y, ref)
        worst = max(worst, d)
        print(f"{name}: cpu float32 path vs float64 reference {d:.2e} of the RMS")
        assert y.dtype == np.float32 and R.problems(y, ref) == [], name
        assert ref["m"] == min(len(x), T) and ref["p"] == (0 if len(x) > T else place)
    print(f"largest: {worst:.2e} (the bound is {R.REL_BOUND:g})")
    silent = R.edge_cases()[-1]
    assert not R.cpu_plain_path(silent[1], F, T, silent[2], silent[3]).any()


def test_reference_rejects_mutated_candidates():
    cases = {name: (x, cut, place) for name, x, cut, place in R.edge_cases()}
    x, cut, place = cases["n=3T last legal cut, loud head"]
    ref = R.reference(x, F, T, cut, place)
    assert R.problems(ref["y"].astype(np.float32), ref) == []
    assert R.problems(R.reference(x, F, T, cut, place, rms_over="window")["y"], ref), "RMS over the cut window only"
    x, cut, place = cases["n=2F"]
    ref = R.reference(x, F, T, cut, place)
    assert R.problems(R.reference(x, F, T, cut, place, ramp_points=F + 1)["y"], ref), "ramps of F + 1 points"
    assert R.problems(R.reference(x, F, T, cut, place, shift=1)["y"], ref), "placed one sample late"
    assert R.problems(R.reference(x, F, T, cut, place + 1)["y"], ref), "placement draw off by one"
    pad = ref["y"].copy()
    pad[place - 1] = 1e-30
    assert R.problems(pad, ref) == ["not exactly 0.0 outside the clip"]
    pad = ref["y"].copy()
    pad[-1] = -1e-30
    assert R.problems(pad, ref) == ["not exactly 0.0 outside the clip"]
    x, cut, place = cases["n=T+1 cut 0"]
    ref = R.reference(x, F, T, cut, place)
    assert R.problems(R.reference(x, F, T, cut, place, fade_in_on_cut=True)["y"], ref), "fade-in on a cut clip"
    nan = ref["y"].copy()
    nan[3] = np.nan
    assert "not finite" in R.problems(nan, ref)
    assert R.problems(ref["y"][:-1], ref)[0].startswith("shape")


# ------------------------------------------------------------------------------------------------------------ C ABI without a GPU
def _args(**over):
    a = _abi.STRUCTS["wj_noise_prepare_args"]()
    keep = dict(offsets=np.array([0, 8000], np.int64), lengths=np.array([8000, 3000], np.int32), cut_start=np.array([100, 0], np.int32),
                place_start=np.array([0, 50], np.int32), clips=np.array([0, 1], np.int32))
    fields = dict(noise=0x1000, out=0x3000, workspace=0x4000, noise_elems=11000, workspace_bytes=1 << 20, B=2, n_clips=2, max_len=8000,
                  out_len=T, fade_len=F)
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


def test_wj_noise_prepare_is_declared_and_reports_argument_errors_before_any_launch():
    lib = _abi.load()
    assert "wj_noise_prepare" in _abi.FUNCTIONS
    assert lib.wj_struct_size(b"wj_noise_prepare_args") == ctypes.sizeof(_abi.STRUCTS["wj_noise_prepare_args"])
    assert _abi.DEFINES["WJ_ABI_VERSION"] == 17 and lib.wj_abi_version() == 17

    def rc(**over):
        a, keep = _args(**over)
        return lib.wj_noise_prepare(ctypes.byref(a), None)
    i32 = lambda *v: np.array(v, np.int32)       # noqa: E731
    assert lib.wj_noise_prepare(None, None) == -1
    for bad in (dict(noise=0), dict(out=0), dict(workspace=0), dict(offsets=None), dict(lengths=None), dict(cut_start=None),
                dict(place_start=None), dict(clips=None), dict(B=0), dict(n_clips=0), dict(out_len=0), dict(fade_len=0), dict(max_len=0),
                dict(noise_elems=10999),                                        # clip 1 ends outside the buffer
                dict(offsets=np.array([-1, 8000], np.int64)),
                dict(lengths=i32(8000, F - 1)),                                 # n < F
                dict(lengths=i32(8001, 3000)),                                  # n > max_len
                dict(out_len=F - 1),                                            # T < F
                dict(fade_len=T + 1),
                dict(cut_start=i32(8000 - T, 0)), dict(cut_start=i32(-1, 0)),   # s in [0, n - T)
                dict(place_start=i32(0, T - 3000 + 1)), dict(place_start=i32(0, -1)),    # p in [0, T - n]
                dict(clips=i32(0, 2)), dict(clips=i32(-1, 1)),
                dict(workspace_bytes=4)):
        assert rc(**bad) == -1, bad
    # the draws that do not apply to a clip are not read: a cut position on the short clip, a placement on the long one
    a, _ = _args(cut_start=i32(100, -5), place_start=i32(99999, 50), clips=i32(0, 2))
    assert lib.wj_noise_prepare(ctypes.byref(a), None) == -1                    # (still refused: the clip index)


def test_wj_noise_prepare_workspace_query():
    q = lambda **d: ops.workspace_bytes("wj_noise_prepare", **d)               # noqa: E731
    small = q(B=2, n_clips=2, max_len=8000, out_len=T, fade_len=F)
    more_clips = q(B=128, n_clips=128, max_len=8000, out_len=T, fade_len=F)
    longer = q(B=2, n_clips=2, max_len=700000, out_len=320000, fade_len=6400)
    full = q(B=128, n_clips=128, max_len=700000, out_len=320000, fade_len=6400)
    assert 0 < small < more_clips and small < longer < full < 1 << 20 and full % 4 == 0
    lib = _abi.load()
    for bad in (dict(fade_len=T + 1), dict(max_len=F - 1), dict(n_clips=0), dict(fade_len=0)):
        a, _ = _args(**bad)
        assert lib.wj_workspace_bytes(b"wj_noise_prepare", ctypes.byref(a)) == -1, bad


# ------------------------------------------------------------------------------------------------------------ raw mode of the data module
SR, OUT_LEN, FADE = 32000, 320000, 6400


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    return R.make_denoiser_shards(str(tmp_path_factory.mktemp("denoiser_shards")))


def _stream(shards, n, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g = R.denoiser_module(shards, **kw)._batches(0, 1)
        return [next(g) for _ in range(n)]


@pytest.mark.parametrize("with_noise,with_rir", [(True, True), (True, False), (False, True), (False, False)])
def test_raw_mode_makes_the_same_draws_and_ships_the_clips_as_they_are(shards, with_noise, with_rir):
    plain = _stream(shards, 3, with_noise=with_noise, with_rir=with_rir)
    raw = _stream(shards, 3, with_noise=with_noise, with_rir=with_rir, device_prep=True)
    seen_long = seen_short = 0
    for (audio, srir, noise, length, start, nrirs, snr), rb in zip(plain, raw):
        assert isinstance(rb, audio_prep.RawDenoiserBatch) and len(rb) == 3 and rb.out_len == OUT_LEN
        assert isinstance(rb.clean, audio_prep.RawAudioBatch) and rb.clean.ctx is None and rb.clean.tgt is None and rb.clean.vis is None
        assert rb.has_noise is with_noise
        # integers, SNR and RIRs are the default mode's
        assert torch.equal(rb.noise_length, length) and rb.noise_length.dtype == length.dtype
        assert torch.equal(rb.noise_start_idx, start) and rb.noise_start_idx.dtype == start.dtype
        for mine, theirs, on in ((rb.snr, snr, with_noise), (rb.source_rir, srir, with_rir), (rb.noise_rirs, nrirs, with_noise and with_rir)):
            if on:
                assert isinstance(mine, torch.Tensor) and mine.dtype == theirs.dtype and torch.equal(mine, theirs)
            else:
                assert mine == [None] * 3 and theirs == [None] * 3
        if not with_noise:
            assert noise == [None] * 3 and int(rb.noise_lengths.sum()) == 0 and rb.noise.numel() == 1
        for b in range(3):
            # the clean clip: the decoder's channel-0 PCM, in the default mode's order
            clip, rate = rb.clean.clip(b).numpy(), int(rb.clean.rates[b])
            key = [k for k, (pcm, r, _) in shards["pcm"].items() if r == rate and pcm.shape[0] == clip.shape[0] and np.array_equal(pcm[:, 0], clip)]
            assert len(key) == 1 and int(rb.clean.prepared[b]) == audio_prep.PCM and int(rb.clean.bits[b]) == 16
            assert np.array_equal(RA.cpu_product_path(clip, 16, rate, SR, OUT_LEN), audio[b].numpy()), key
            if not with_noise:
                continue
            # the noise clip: the .npy member itself; the default mode's row is this clip under the draws the raw batch carries
            x = rb.noise_clip(b).numpy()
            assert x.dtype == np.float32 and any(np.array_equal(x, n) for n in shards["noises"]) and int(rb.noise_offsets[b]) % 4 == 0
            cut, place = int(rb.cut_start[b]), int(rb.place_start[b])
            seen_long += len(x) > OUT_LEN
            seen_short += len(x) < OUT_LEN
            assert (0 <= cut < len(x) - OUT_LEN and place == 0) if len(x) > OUT_LEN else (cut == 0 and 0 <= place <= OUT_LEN - len(x))
            assert R.problems(noise[b].numpy(), R.reference(x, FADE, OUT_LEN, cut, place)) == []
    if with_noise:
        assert seen_long and seen_short


def test_a_noise_clip_shorter_than_the_fade_is_skipped_in_both_modes(tmp_path):
    sh = R.make_denoiser_shards(str(tmp_path))
    R._shard(sh["noise"], [("short.npy", R._npy(np.ones(FADE - 1, np.float32))), ("ok.npy", R._npy(sh["noises"][0]))])
    for mode in (False, True):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            g = R.denoiser_module(sh, with_rir=False, device_prep=mode)._batches(0, 1)
            batches = [next(g) for _ in range(2)]
        assert any("skipped" in str(x.message) for x in w), mode
        lengths = torch.cat([b.noise_lengths if mode else b[3] for b in batches])
        assert set(lengths.tolist()) == {len(sh["noises"][0])}


def test_device_prep_is_off_by_default_and_returns_a_plain_dataloader(shards):
    from torch.utils.data import DataLoader
    dm = R.denoiser_module(shards)
    assert dm.device_prep is False and type(dm.train_dataloader()) is DataLoader
    batch = _stream(shards, 1)[0]
    assert isinstance(batch, tuple) and len(batch) == 7 and batch[0].shape == (3, OUT_LEN) and batch[2].shape == (3, OUT_LEN)
    on = R.denoiser_module(shards, device_prep=True, prep_device="cuda:0")
    assert on.device_prep is True
    loader = on.train_dataloader()
    assert isinstance(loader, audio_prep.DevicePrepLoader) and type(loader.loader) is DataLoader
    assert isinstance(loader.prep, audio_prep.DenoiserDevicePrep) and loader.prep.out_len == OUT_LEN and loader.prep.fade_len == FADE


def test_raw_denoiser_batches_travel_through_worker_processes(shards):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        it = iter(R.denoiser_module(shards, device_prep=True).train_dataloader().loader)       # the DataLoader itself: two worker processes
        batches = [next(it) for _ in range(3)]
        del it
    for rb in batches:
        assert isinstance(rb, audio_prep.RawDenoiserBatch) and len(rb) == 3 and rb.snr.shape == (3,) and rb.noise_rirs.shape == (3, 2, 2, 600)
        assert all(any(np.array_equal(rb.noise_clip(b).numpy(), n) for n in shards["noises"]) for b in range(3))
    assert hasattr(batches[0], "pin_memory")


@pytest.mark.skipif(torch.cuda.is_available(), reason="the no-GPU behaviour")
def test_no_cpu_fallback(shards):
    rb = _stream(shards, 1, device_prep=True)[0]
    with pytest.raises((_abi.WavJepaHipError, RuntimeError)):
        audio_prep.DenoiserDevicePrep(SR, 10).prepare(rb)
    with pytest.raises((_abi.WavJepaHipError, RuntimeError)):
        next(iter(audio_prep.DevicePrepLoader([rb], audio_prep.DenoiserDevicePrep(SR, 10))))
