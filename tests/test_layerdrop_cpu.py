"""LayerDrop on the host: the keep draw (wavjepa_amd/layerdrop.py) against the test helper's restatement of the dropout generator,
the module surface (constructor keywords, hyper-parameters, layerdrop_keep, the launcher's keys, refusals) and the oracle helper
(tests/layerdrop_reference.py).  The engine's walkers are checked on the GPU (tests/test_layerdrop_gpu.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import jepa_oracle as J
from tests import dropout_reference as R
from tests import layerdrop_reference as LR
from tests.test_dropout_cpu import SPEC, _jepa
from tests.test_oracle_golden import TINY, load, params_from
from wavjepa_amd import layerdrop as LD

SEED = (0x5DEECE66D << 20) ^ 20240607          # a seed with a non-zero high word


# ---------------------------------------------------------------------------------------------------------------- the draw
def test_draw_is_a_pure_function_of_seed_call_stack_layer_and_bit_equal_to_the_reference_generator():
    assert LD.SITE_LAYER == 5 and LD.STACK == R.STACK
    for seed in (0, 7, SEED, (1 << 64) - 1):
        for call in (0, 3, (1 << 32) - 1):
            for stack in (0, 1):
                got = LD.layer_draws(seed, call, stack, range(24))
                again = LD.layer_draws(seed, call, stack, range(24))
                want = [int(R.philox4x32_10(0, 0, 5 | i << 8 | stack << 16, call, seed & 0xFFFFFFFF, seed >> 32)[0]) & 0xFFFF for i in range(24)]
                assert got.tolist() == again.tolist() == want == [LR.draw(seed, call, stack, i) for i in range(24)]
    # the product's own restatement of the generator, word for word
    for ctr, key in (((0, 0, 0, 0), (0, 0)), ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))):
        assert [int(w) for w in LD.philox4x32_10(*ctr, *key)] == [int(w) for w in R.philox4x32_10(*ctr, *key)]
    base = LD.layer_draws(SEED, 3, 0, range(24))
    for other in (LD.layer_draws(SEED + 1, 3, 0, range(24)), LD.layer_draws(SEED ^ (1 << 40), 3, 0, range(24)),
                  LD.layer_draws(SEED, 4, 0, range(24)), LD.layer_draws(SEED, 3, 1, range(24))):
        assert int((base != other).sum()) >= 22
    assert len(set(base.tolist())) >= 23                                   # ... and on the layer
    assert LD.kept_layers(SEED, 3, "enc", 24, 0.2) == LR.kept_set(SEED, 3, "enc", 24, 0.2)
    assert LD.kept_layers(SEED, 3, "dec", 12, 0.5) == LR.kept_set(SEED, 3, "dec", 12, 0.5)


def test_site_5_differs_from_the_kernels_sites():
    five = LD.layer_draws(SEED, 9, 0, range(24))
    for site in (1, 2, 3, 4):
        other = LD.layer_draws(SEED, 9, 0, range(24), site=site)
        want = [int(R.group_draws(SEED, 9, R.stream_id(0, i, site), np.zeros(1, np.uint64))[0, 0]) for i in range(24)]
        assert other.tolist() == want                                      # (draw 0 of element group 0 of the kernels' site)
        assert int((five != other).sum()) >= 22


def test_draw_is_independent_of_the_rank(monkeypatch):
    """The element masks' key mixes the data-parallel rank in (JEPA._dropout_key); the kept layers come from dropout_seed itself."""
    torch.manual_seed(1234)
    m = _jepa(encoder_layerdrop=0.5, decoder_layerdrop=0.5)
    import torch.distributed as dist
    sets, keys = [], []
    for rank in (0, 1, 5):
        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dist, "get_rank", lambda r=rank: r)
        sets.append([m._layerdrop_kept(c) for c in range(16)])
        keys.append(m._dropout_key())
    assert len(set(keys)) == 3 and sets[0] == sets[1] == sets[2]
    assert sets[0] == [dict(enc=LR.kept_set(1234, c, "enc", 2, 0.5), dec=LR.kept_set(1234, c, "dec", 2, 0.5)) for c in range(16)]
    assert len({tuple(s["enc"]) for s in sets[0]}) > 1


@pytest.mark.parametrize("p", [0.05, 0.2, 0.5])
def test_keep_rate(p):
    thr = LD.threshold(p)
    assert thr == round(p * 65536)
    kept = sum(len(LD.kept_layers(SEED, call, "enc", 20, p)) for call in range(1000))       # 20 000 (call, layer) pairs
    rate, want = kept / 20000, 1 - thr / 65536
    sigma = np.sqrt(want * (1 - want) / 20000)
    print("p", p, "keep rate", rate, "expected", want, "sigma", sigma)
    assert abs(rate - want) < 5 * sigma


def test_rate_0_keeps_everything_without_a_generator_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the generator was evaluated")
    monkeypatch.setattr(LD, "philox4x32_10", boom)
    assert LD.kept_layers(SEED, 3, "enc", 7, 0.0) == list(range(7)) and LD.kept_layers(SEED, 3, "dec", 5, 0) == list(range(5))
    m = _jepa()
    assert m._layerdrop_kept(3) is None
    m = _jepa(encoder_layerdrop=0.3)
    m.layerdrop_keep = dict(enc=[1])
    assert m._layerdrop_kept(3) == dict(enc=[1])                           # an explicit value wins over the draw: nothing is drawn
    with pytest.raises(AssertionError):
        LD.kept_layers(SEED, 3, "enc", 7, 0.1)
    assert LD.threshold(0.0) == 0 and LD.threshold(0.99999999) == 65535


# ---------------------------------------------------------------------------------------------------------------- module surface
def test_constructor_and_hyper_parameters():
    from tests.test_recompute_cpu import DEFAULT_HPARAMS, plain_path
    torch.manual_seed(77)
    off = _jepa()
    assert off.encoder_layerdrop == 0.0 and off.decoder_layerdrop == 0.0 and off.layerdrop_keep is None and off.last_kept is None
    assert not {"encoder_layerdrop", "decoder_layerdrop", "dropout_seed"} & set(off.hparams)
    if plain_path():
        assert set(off.hparams) == DEFAULT_HPARAMS
    torch.manual_seed(77)
    enc = _jepa(encoder_layerdrop=0.05)
    assert enc.encoder_layerdrop == 0.05 and enc.decoder_layerdrop == 0.0
    assert set(enc.hparams) - set(off.hparams) == {"encoder_layerdrop", "dropout_seed"}
    assert enc.hparams["encoder_layerdrop"] == 0.05 and enc.hparams["dropout_seed"] == 77 == enc.dropout_seed
    both = _jepa(encoder_layerdrop=0.2, decoder_layerdrop=0.1)
    assert set(both.hparams) - set(off.hparams) == {"encoder_layerdrop", "decoder_layerdrop", "dropout_seed"}
    with_drop = _jepa(0.1, 0.0, decoder_layerdrop=0.1)
    assert {"dropout_encoder", "dropout_decoder", "dropout_seed", "decoder_layerdrop"} <= set(with_drop.hparams)
    both.dropout_seed = 5
    assert both.hparams["dropout_seed"] == 5
    assert list(both.state_dict()) == list(off.state_dict())
    for bad in (-0.1, 1.0, 1.5, "x", None, True):
        with pytest.raises(ValueError, match=r"encoder_layerdrop.*\[0, 1\)"):
            _jepa(encoder_layerdrop=bad)
        with pytest.raises(ValueError, match=r"decoder_layerdrop.*\[0, 1\)"):
            _jepa(decoder_layerdrop=bad)


def test_layerdrop_keep_is_validated():
    m = _jepa()                                                            # 2 + 2 layers
    m.layerdrop_keep = dict(enc=[0, 1], dec=[])
    assert m.layerdrop_keep == dict(enc=[0, 1], dec=[]) and m._layerdrop_kept(0) == dict(enc=[0, 1], dec=[])
    m.layerdrop_keep = dict(dec=(1,))
    assert m.layerdrop_keep == dict(dec=[1])
    m.layerdrop_keep = None
    assert m.layerdrop_keep is None and m._layerdrop_kept(0) is None
    for bad in (dict(enc=[1, 0]), dict(enc=[0, 0]), dict(enc=[2]), dict(dec=[-1]), dict(tea=[0]), dict(enc=[0.5]), dict(enc=3), [0, 1],
                dict(enc=[True])):
        with pytest.raises(ValueError, match="layerdrop_keep"):
            m.layerdrop_keep = bad
    assert m.layerdrop_keep is None


def test_launcher_reads_the_two_keys():
    import train
    from wavjepa_amd.config import load_config
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")
    off, _ = train.build_model(load_config(root, ["trainer.size=tiny"]))
    on, _ = train.build_model(load_config(root, ["trainer.size=tiny", "trainer.encoder_layerdrop=0.5"]))
    both, _ = train.build_model(load_config(root, ["trainer.size=tiny", "trainer.encoder_layerdrop=0.05", "+trainer.decoder_layerdrop=0.1"]))
    assert off.encoder_layerdrop == 0.0 and off.decoder_layerdrop == 0.0 and not {"encoder_layerdrop", "decoder_layerdrop"} & set(off.hparams)
    assert on.encoder_layerdrop == 0.5 and on.decoder_layerdrop == 0.0
    assert set(on.hparams) - set(off.hparams) == {"encoder_layerdrop", "dropout_seed"}
    assert both.encoder_layerdrop == 0.05 and both.decoder_layerdrop == 0.1
    with pytest.raises(RuntimeError, match=r"encoder_layerdrop.*\[0, 1\)"):
        train.build_model(load_config(root, ["trainer.size=tiny", "trainer.encoder_layerdrop=1.0"]))


def test_engine_refuses_fp8_with_layerdrop_and_checks_its_config():
    """The check that lives in the engine, on a stand-in that has only what it reads (the engine itself needs a GPU)."""
    from wavjepa_amd.engine import EngineConfig, JepaEngine
    fields = {f.name: f.default for f in EngineConfig.__dataclass_fields__.values()}
    assert fields["layerdrop_enc"] == 0.0 and fields["layerdrop_dec"] == 0.0
    kw = dict(conv_spec=SPEC, in_channels=1, n_samples=32159, d_enc=64, h_enc=2, l_enc=2, d_dec=64, h_dec=2, l_dec=2, top_k=2)

    class Stub:
        fp8, recompute = True, False
    for rates in (dict(layerdrop_enc=0.1), dict(layerdrop_dec=0.2)):
        s = Stub()
        s.cfg = EngineConfig(**kw, **rates)
        with pytest.raises(RuntimeError, match=r"(?s)fp8.*layerdrop"):
            JepaEngine._check_fp8(s)
        s.fp8 = False
        JepaEngine._check_fp8(s)
    s = Stub()
    s.cfg = EngineConfig(**kw)
    JepaEngine._check_fp8(s)                                               # (fp8 alone is still taken)


# ---------------------------------------------------------------------------------------------------------------- the oracle helper
def _tiny(golden_dir):
    fx = load(golden_dir, "tiny_model.npz")
    return params_from(fx), tuple(torch.from_numpy(fx[k]) for k in ("audio", "ctx", "tgt", "vis"))


def test_helper_with_every_layer_listed_is_the_oracle(golden_dir, monkeypatch):
    P, batch = _tiny(golden_dir)
    n = dict(enc=J.n_layers(P, "encoder"), dec=J.n_layers(P, "decoder"))
    want = J.jepa_forward(P, *batch, mode="fp32", **TINY)
    want_bf = J.jepa_forward(P, *batch, mode="bf16", **TINY)
    for kept in (dict(enc=list(range(n["enc"])), dec=list(range(n["dec"]))), dict(enc=list(range(n["enc"]))), {}):
        LR.install(monkeypatch, kept)
        assert J.encoder_stack is not LR._ENCODER_STACK
        got, got_bf = J.jepa_forward(P, *batch, mode="fp32", **TINY), J.jepa_forward(P, *batch, mode="bf16", **TINY)
        monkeypatch.undo()
        for k in ("local_features", "contextual_features", "preds", "targets", "loss"):
            assert torch.equal(got[k], want[k]) and torch.equal(got_bf[k], want_bf[k]), k


def test_helper_skips_the_listed_layers_only(golden_dir, monkeypatch):
    P, batch = _tiny(golden_dir)
    n = dict(enc=J.n_layers(P, "encoder"), dec=J.n_layers(P, "decoder"))
    assert n["enc"] >= 2 and n["dec"] >= 2
    names = J.trainable_names(P)
    full = J.jepa_forward(P, *batch, mode="fp32", **TINY)
    kept = dict(enc=[n["enc"] - 1], dec=[0])
    LR.install(monkeypatch, kept)
    for k in names:
        P[k].requires_grad_(True)
    out = J.jepa_forward(P, *batch, mode="fp32", **TINY)
    out["loss"].backward()
    skipped = LR.skipped_names(P, kept)
    assert skipped and all(P[k].grad is None for k in skipped)
    assert all(P[k].grad is not None for k in names if k not in skipped)
    assert float(P[f"encoder.layers.{n['enc'] - 1}.linear1.weight"].grad.abs().max()) > 0
    assert torch.equal(out["targets"], full["targets"])                    # the teacher never drops
    assert not torch.equal(out["contextual_features"], full["contextual_features"]) and float(out["loss"].detach()) != float(full["loss"])
    # the student is its last layer and its final norm
    with torch.no_grad():
        lf = J.local_features(P, batch[0], TINY["spec"], "fp32")
        x = J.post_norm_layer(P, f"encoder.layers.{n['enc'] - 1}.", lf, TINY["enc_heads"], batch[1], "fp32")
        x = J._ln(x, P["encoder.norm.weight"], P["encoder.norm.bias"], 1e-5)
        cf = J._lin(x[~batch[1]], P["encoder_to_decoder_mapper.weight"], P["encoder_to_decoder_mapper.bias"], "fp32")
    assert torch.equal(cf, out["contextual_features"].detach())
    # an empty stack is its final norm over its input
    kept.update(enc=[], dec=[])
    with torch.no_grad():
        x = torch.randn(2, 9, P["decoder.norm.weight"].numel(), generator=torch.Generator().manual_seed(1))
        assert torch.equal(J.encoder_stack(P, "decoder", x, TINY["dec_heads"], None, "fp32"),
                           J._ln(x, P["decoder.norm.weight"], P["decoder.norm.bias"], 1e-5))
        y = J.encoder_stack(P, "teacher_encoder", lf, TINY["enc_heads"], None, "fp32", final_norm=False)
    assert torch.equal(y, LR._ENCODER_STACK(P, "teacher_encoder", lf, TINY["enc_heads"], None, "fp32", final_norm=False))


def test_trajectory_helper_at_k_1_with_every_layer_is_the_oracles_train_step(golden_dir, monkeypatch):
    P, batch = _tiny(golden_dir)
    Pa, Pb = ({k: v.clone() for k, v in P.items()} for _ in range(2))
    n = dict(enc=list(range(J.n_layers(P, "encoder"))), dec=list(range(J.n_layers(P, "decoder"))))
    sa, sb, kept = {}, {}, {}
    for step in range(2):
        a = J.train_step(Pa, sa, step, batch, mode="fp32", warmup=2, total_steps=10, **TINY)
        LR.install(monkeypatch, kept)
        b = LR.train_window(Pb, sb, step, [batch], [n], kept, mode="fp32", warmup=2, total_steps=10, **TINY)
        monkeypatch.undo()
        assert a["loss"] == b["loss"] and a["grad_norm"] == b["grad_norm"]
    assert all(torch.equal(Pa[k], Pb[k]) for k in Pa)
    # a skipped layer has gradient zero, not None: the update still reaches it (weight decay, the decaying first moment)
    LR.install(monkeypatch, kept)
    w = "encoder.layers.0.linear1.weight"
    before, m_before = Pb[w].clone(), sb[w]["m"].clone()
    LR.train_window(Pb, sb, 2, [batch], [dict(enc=n["enc"][1:])], kept, mode="fp32", warmup=2, total_steps=10, **TINY)
    assert not torch.equal(Pb[w], before) and torch.equal(sb[w]["m"], m_before * 0.9)
