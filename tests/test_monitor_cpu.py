"""Collapse monitor, host side: the reference against torch, the emulation of wj_masked_moments against the bound, the mutations the
bound must reject, merge_moments, the C ABI of libwavjepa_hip_monitor.so, and the module / trainer / launcher surface.  None of this
needs a GPU (tests/test_monitor_ops_gpu.py and tests/test_monitor_gpu.py run the kernel and the step)."""
from __future__ import annotations

import ctypes
import inspect
import os
import types

import numpy as np
import pytest
import torch

from tests import moments_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows():
    from wavjepa_amd import ops
    return ops.MOMENTS_ROWS


@pytest.fixture(scope="module")
def cases():
    return mr.kernel_cases(_rows())


# ---------------------------------------------------------------------------------------------------------------- reference
@pytest.mark.parametrize("form", mr.FORMS)
def test_reference_equals_torch_on_rows_gathered_by_hand(form):
    case = mr.make_case(3, 4, 50, 768, seed=14)
    B, G, T, D = (case[k] for k in "BGTD")
    dense_preds, targets, tgt = case["preds"].view(B * G, T, D), case["targets"].view(B, T, D), case["tgt"].view(B, G, T)
    inv = {int(d): r for r, d in enumerate(mr.row_list(case, form))}          # dense position -> row of the form's preds
    held = mr.packed_preds(case, form)
    P, Y = [], []
    for b in range(B):
        for g in range(G):
            for t in range(T):
                if tgt[b, g, t] == 1:
                    r = inv[(b * G + g) * T + t]
                    assert torch.equal(held[r], dense_preds[b * G + g, t])
                    P.append(held[r])
                    Y.append(targets[b, t])
    ref = mr.reference(case, form)
    assert ref["n"] == len(P) == int(tgt.sum()) and len({id(y) for y in Y}) <= len(Y)
    for rows, key in ((P, "pred_var"), (Y, "target_var")):
        y = torch.stack(rows).double()
        assert abs(ref[key] - float(torch.sqrt(y.var(0) + 1e-6).mean())) <= 1e-13 * ref[key], key
    multi = (tgt.sum(1) > 1).sum()
    assert int(multi) > 0, "the case must hold tokens that are targets in two groups"


def test_degenerate_counts_give_variance_zero():
    one = mr.reference(mr.make_case(1, 1, 1, 8, seed=1), "dense")
    assert one["n"] == 1 and one["pred_var"] == one["target_var"] == np.sqrt(1e-6)
    two = mr.reference(mr.make_case(1, 1, 2, 8, seed=2), "trimmed")
    assert two["n"] == 2 and two["var"][0][mr.COL_CONST] == 0.0 and two["var"][0][4] > 0


# ---------------------------------------------------------------------------------------------------------------- emulation
def test_emulation_stays_inside_the_bound_on_every_kernel_case(cases):
    """Prints the yardstick distances and the bounds PARITY.md records."""
    for name, case in cases:
        for form in mr.FORMS:
            bnd = mr.bounds(case, form)
            got = mr.emulate(case, form, _rows())
            err = [np.abs(got["var"][q] - bnd["ref"]["var"][q]) for q in (0, 1)]
            print(f"{name} {form}: n {bnd['ref']['n']}  yardstick max col dist preds {bnd['dist_col'][0].max():.3e} targets {bnd['dist_col'][1].max():.3e}"
                  f"  stat dist {bnd['dist_stat'][0]:.3e} {bnd['dist_stat'][1]:.3e}  bound stat {bnd['bound_stat'][0]:.3e} {bnd['bound_stat'][1]:.3e}"
                  f"  emulation max err/bound {max((err[0] / bnd['bound_col'][0]).max(), (err[1] / bnd['bound_col'][1]).max()):.3e}"
                  f"  stat err {abs(got['pred_var'] - bnd['ref']['pred_var']):.3e} {abs(got['target_var'] - bnd['ref']['target_var']):.3e}")
            assert mr.violations(got, case, form, bnd) == [], (name, form)


@pytest.mark.parametrize("mutation", mr.MUTATIONS)
def test_every_mutation_is_rejected_by_the_same_check(mutation):
    case = mr.make_case(3, 4, 50, 768, seed=14)
    form = "ragged"                                            # the one form in which every mutation changes something
    bad = mr.violations(mr.emulate(case, form, _rows(), mutation=mutation), case, form)
    print(mutation, bad)
    assert bad, mutation
    assert mr.violations(mr.emulate(case, form, _rows()), case, form) == []


def test_mutations_change_the_row_set_only_where_they_should():
    case = mr.make_case(3, 4, 50, 768, seed=14)
    n = {f: mr.reference(case, f)["n"] for f in mr.FORMS}
    assert n["dense"] == n["ragged"] == n["trimmed"]
    assert mr.gather(case, "ragged", "nontarget_rows")[0].shape[0] == len(case["dec_rows"]) > n["ragged"]
    assert mr.gather(case, "trimmed", "nontarget_rows")[0].shape[0] == n["trimmed"]
    assert mr.gather(case, "ragged", "no_multiplicity")[0].shape[0] < n["ragged"]


# ------------------------------------------------------------------------------------------------------------ merge_moments
def test_merge_moments_of_a_split_equals_the_unsplit_statistic():
    from wavjepa_amd.ops import merge_moments
    case = mr.make_case(3, 4, 50, 768, seed=14)
    ref = mr.reference(case, "trimmed")
    P, Y = mr.gather(case, "trimmed")
    for X, want in ((P.numpy(), ref["pred_var"]), (Y.numpy(), ref["target_var"])):
        for cuts in ([0, len(X)], [0, 1, len(X)], [0, 100, 100, 333, len(X)], [0, len(X) // 2, len(X)]):
            parts = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                part = X[a:b]
                mean = part.mean(0) if len(part) else np.zeros(X.shape[1])
                parts.append((len(part), mean, ((part - mean) ** 2).sum(0) if len(part) else np.zeros(X.shape[1])))
            got = merge_moments(parts)
            assert abs(got - want) <= 1e-12 * want, (cuts, got, want)
    const = np.full((5, 8), 2.5)
    assert merge_moments([(2, const[:2].mean(0), np.zeros(8)), (3, const[2:].mean(0), np.zeros(8))]) == np.sqrt(1e-6)
    assert merge_moments([(1, np.ones(8), np.zeros(8))]) == np.sqrt(1e-6)          # fewer than two rows: variance 0
    with pytest.raises(ValueError):
        merge_moments([])


# -------------------------------------------------------------------------------------------------------------------- C ABI
def test_abi_of_the_monitor_entry():
    """The entry lives in a library and a header of its own: what libwavjepa_hip.so exports and declares has not moved."""
    import subprocess
    from wavjepa_amd import _abi, ops
    rel, lib = _abi.load(), _abi.load("monitor")
    assert _abi.DEFINES["WJ_ABI_VERSION"] == 17 == rel.wj_abi_version()
    assert "wj_masked_moments" not in _abi.FUNCTIONS and "wj_masked_moments" not in _abi.ENTRY_ARGS and not hasattr(rel, "wj_masked_moments")
    assert _abi.LIBRARIES["monitor"].entry_args == {"wj_masked_moments": "wj_moments_args"}
    S = _abi.LIBRARIES["monitor"].struct_types["wj_moments_args"]
    assert ctypes.sizeof(S) == 7 * 8 + 5 * 4 + 4 == lib.wj_monitor_struct_size(b"wj_moments_args")
    assert [n for n, _ in S._fields_] == ["preds", "targets", "tgt", "rows", "out", "col", "workspace", "B", "G", "T", "D", "n_rows"]
    assert lib.wj_monitor_struct_size(b"wj_mse_args") == -1 and lib.wj_monitor_struct_size(None) == -1
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIBRARIES["monitor"].path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert exported == set(_abi.LIBRARIES["monitor"].functions) == {"wj_masked_moments", "wj_monitor_struct_size", "wj_monitor_workspace_bytes"}
    assert ops.MOMENTS_ROWS == _abi.LIBRARIES["monitor"].defines["WJ_MOMENTS_ROWS"] > 0 and ops._ENTRY_STRUCT["wj_masked_moments"] is S
    # the scratch: a count per row group, then [2][2][D padded to the column slab] doubles per row group, for the longest row list
    R, Dc = ops.MOMENTS_ROWS, ops.MOMENTS_COLS
    for dims, rows, D in ((dict(B=3, G=4, T=50, D=768), 600, 768), (dict(B=1, G=1, T=1, D=8), 1, 8), (dict(B=1, G=1, T=R + 1, D=1000), R + 1, 1000),
                          (dict(B=1, G=1, T=1, D=16, n_rows=3 * R), 3 * R, 16)):
        groups, Dp = -(-rows // R), -(-D // Dc) * Dc
        assert ops.workspace_bytes("wj_masked_moments", **dims) == 8 * (groups + 4 * groups * Dp), dims
    assert int(lib.wj_monitor_workspace_bytes(b"wj_masked_moments", ctypes.byref(S()))) == 0
    assert int(lib.wj_monitor_workspace_bytes(b"wj_masked_moments", ctypes.byref(S(B=-1)))) == -1
    assert int(lib.wj_monitor_workspace_bytes(b"wj_masked_loss", ctypes.byref(S()))) == -1
    assert int(lib.wj_monitor_workspace_bytes(None, None)) == -1


def test_monitor_entry_rejects_bad_arguments_without_a_gpu():
    from wavjepa_amd import _abi, ops
    lib = _abi.load("monitor")
    S = _abi.LIBRARIES["monitor"].struct_types["wj_moments_args"]
    ptr = 4096                                                  # never dereferenced: every call below is refused on the host
    good = dict(preds=ptr, targets=ptr, tgt=ptr, out=ptr, workspace=ptr, B=2, G=2, T=8, D=64)
    call = lambda **kw: int(lib.wj_masked_moments(ctypes.byref(S(**dict(good, **kw))), None))
    assert int(lib.wj_masked_moments(None, None)) == -1
    for name in ("preds", "targets", "tgt", "out", "workspace"):
        assert call(**{name: 0}) == -1, name
    for name in ("B", "G", "T", "D"):
        for v in (0, -3):
            assert call(**{name: v}) == -1, (name, v)
    assert call(rows=ptr, n_rows=-1) == -1
    for D in (4, 12, 60, 770):
        assert call(D=D) == -3, D                               # D % 8: unsupported
    assert call(preds=ptr + 8) == -1 and call(targets=ptr + 4) == -1 and call(workspace=ptr + 4) == -1 and call(col=ptr + 4) == -1
    assert call(rows=ptr, n_rows=ops.MOMENTS_ROWS * ops.MOMENTS_MAX_GROUPS + 1) == -3      # more row groups than pass 2 holds factors for
    with pytest.raises(_abi.WavJepaHipError):
        ops.masked_moments(ptr, ptr, ptr, ptr, ptr, B=1, G=1, T=1, D=12, stream=0)


# ------------------------------------------------------------------------------------------------------------ module surface
def small_model(**kw):
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.jepa import JEPA
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    ext = ConvFeatureExtractor(conv_layers_spec=[(64, 10, 5)] + [(64, 3, 2)] * 4 + [(64, 2, 2)], in_channels=1)
    return JEPA(feature_extractor=ext, transformer_encoder_cfg=TransformerEncoderCFG.create(num_layers=1),
                transformer_encoder_layers_cfg=TransformerLayerCFG.create(d_model=128, nhead=2),
                transformer_decoder_cfg=TransformerEncoderCFG.create(num_layers=1),
                transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=64, nhead=2), average_top_k_layers=1,
                process_audio_seconds=2.01, nr_samples_per_audio=2, **kw)


def test_default_model_is_what_it_was():
    """monitor_every is an attribute, default 0: no constructor argument, no hyper-parameter; a step that is not monitored logs the two
    keys it always logged, a monitored one adds train/pred_var and train/target_var."""
    from wavjepa_amd.engine import JepaEngine
    from wavjepa_amd.jepa import JEPA
    m = small_model()
    assert m.monitor_every == 0 and "monitor_every" not in m.hparams
    ctor = set(inspect.signature(JEPA.__init__).parameters)
    assert not {p for p in ctor if "monitor" in p or "var" in p} and set(m.hparams) <= ctor
    assert inspect.signature(JepaEngine.forward).parameters["monitor"].default is False
    logged = {}
    m.log_dict = lambda data, **kw: logged.update(data)
    m._step_teacher = lambda: None
    m.forward = lambda *a: dict(loss=torch.tensor(1.0))
    out = m.training_step((None, None, None, None), 0)
    assert set(logged) == {"train/loss", "ema"} and set(out) == {"loss"}
    m.forward = lambda *a: dict(loss=torch.tensor(1.0), pred_var=torch.tensor(0.5), target_var=torch.tensor(0.9))
    m.training_step((None, None, None, None), 0)
    assert set(logged) == {"train/loss", "ema", "train/pred_var", "train/target_var"} and float(logged["train/pred_var"]) == 0.5


def test_launcher_reads_the_three_keys():
    import train
    from wavjepa_amd.config import load_config
    root = os.path.join(ROOT, "configs")
    cfg = lambda *over: load_config(root, ["trainer.size=tiny", *over])
    assert train.monitor_settings(cfg()) == (0, 0.0, 0.0)
    assert train.monitor_settings(cfg("trainer.monitor_every=7")) == (7, 0.0, 0.0)
    assert train.monitor_settings(cfg("trainer.monitor_every=7", "trainer.min_pred_var=0.01", "trainer.min_target_var=0.1")) == (7, 0.01, 0.1)
    # a threshold without monitor_every: the steps the trainer logs
    assert train.monitor_settings(cfg("trainer.min_target_var=0.1", "trainer.log_every_n_steps=20")) == (20, 0.0, 0.1)
    assert train.monitor_settings(cfg("trainer.min_pred_var=0.01"))[0] == int(cfg().trainer.get("log_every_n_steps", 50))
    off, _ = train.build_model(cfg())
    on, _ = train.build_model(cfg("trainer.monitor_every=3"))
    assert off.monitor_every == 0 and on.monitor_every == 3 and set(on.hparams) == set(off.hparams)
    src = inspect.getsource(train)
    for key in ("monitor_every", "min_pred_var", "min_target_var"):
        assert f'cfg.trainer.get("{key}", 0' in src, key


# ------------------------------------------------------------------------------------------------------------------ trainer
def test_trainer_thresholds_raise_collapse_error():
    from wavjepa_amd.trainer import CollapseError, Trainer
    assert issubclass(CollapseError, RuntimeError)
    sig = inspect.signature(Trainer.__init__).parameters
    assert sig["min_pred_var"].default == 0.0 and sig["min_target_var"].default == 0.0
    stub = types.SimpleNamespace(min_pred_var=0.01, min_target_var=0.1, world=1)
    check = lambda *a: Trainer.check_collapse(stub, *a)
    check(40, 0.5, 0.9)
    check(40, 0.01, 0.1)                                       # at the threshold: not below it
    with pytest.raises(CollapseError) as e:
        check(40, 0.001, 0.9)
    msg = str(e.value)
    assert "pred_var" in msg and "0.001" in msg and "0.01" in msg and "step 40" in msg
    with pytest.raises(CollapseError) as e:
        check(120, 0.5, 0.05)
    msg = str(e.value)
    assert "target_var" in msg and "0.05" in msg and "0.1" in msg and "step 120" in msg
    with pytest.raises(CollapseError):
        check(1, float("nan"), 0.9)
    off = types.SimpleNamespace(min_pred_var=0.0, min_target_var=0.0, world=1)
    Trainer.check_collapse(off, 1, 1e-3, 1e-3)                 # thresholds 0: no check
    # one rank: the step's own device scalars, read at the log step
    assert Trainer._monitor_values(stub, None, (7, torch.tensor(0.25), torch.tensor(0.75))) == (7, 0.25, 0.75)
