"""The denoiser's engine is the encoder base plus its own loss: its arena holds none of the predictor, teacher or JEPA-loss buffers,
and its backward ring has the student's stack only.  A JEPA engine holds all of them.  Smallest shapes of the suite (d = 128,
2 heads, 2 layers, 3 clips of 32159 samples).

The file's name sorts behind the other GPU files on purpose.  Every engine takes six streams from torch's round-robin pool of 32 for
its side-stream probe, and the upload stream comes from the same pool: three more engines in front of a test that compares the stream
labels of two traced models (test_param_groups_gpu.py) moved one of its models onto the upload stream's handle."""
import pytest
import torch

import synth
from tests import test_denoiser_gpu as TD
from tests.test_jepa_gpu import SMALL, build, dev, masks
from tests.test_prenorm_gpu import clips

pytestmark = pytest.mark.gpu
JEPA_ONLY = ("preds", "targets", "dpreds", "cf", "d_cf", "dec_in", "tail_o", "tea_keep", "mse_ws")


def test_denoiser_engine_holds_the_encoder_arena_only():
    from wavjepa_amd.encoder_engine import EncoderEngine
    from wavjepa_amd.engine import JepaEngine
    den, _, _ = TD.build()
    clean = torch.from_numpy(synth.synth_audio(3, 1, 32159, seed=41)).to(torch.bfloat16).to(dev())
    noise = torch.from_numpy(synth.synth_audio(3, 1, 32159, seed=42)).to(dev())
    generated = (clean.float() + 0.5 * noise).to(torch.bfloat16)
    eng = den._ensure_engine()
    den.teacher._ensure_engine()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    den(generated, clean)["loss"].backward()
    torch.cuda.synchronize()
    print("denoiser step: torch.cuda.max_memory_allocated() =", torch.cuda.max_memory_allocated(), flush=True)
    assert isinstance(eng, EncoderEngine) and not isinstance(eng, JepaEngine)
    assert [n for n in JEPA_ONLY if hasattr(eng, n)] == []
    assert set(eng.bw) == {"enc"}
    assert bool(torch.isfinite(eng.dn_loss).all()) and bool(torch.isfinite(den._flat.g32).all())


def test_jepa_engine_holds_the_predictor_teacher_and_loss_buffers(golden_dir):
    m, _ = build(SMALL)
    m(clips(4), *masks(golden_dir, 4))["loss"].backward()
    eng = m._engine
    assert [n for n in JEPA_ONLY if not hasattr(eng, n)] == []
    assert set(eng.bw) == {"enc", "dec"}
