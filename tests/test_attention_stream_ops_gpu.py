"""Single launches of the block-streamed attention entries (wj_attn_stream_fwd / wj_attn_stream_bwd) against the fp64 reference and
per-element bound of tests/attention_reference.py, unchanged (tests/test_attention_stream_cpu.py shows why it applies): NaN-filled
outputs inside guard bands, bytes outside every output region unchanged, two launches bit-identical, defer_fold 1 and 0.

K_B = 128 keys per streamed block.  Shapes: B = 3, H = 2, hd 32 and 64; T at every edge of the block and of the 64-query chunk, the
whole-image limit (416 / 417), a last block of one key (385, 513) and the largest T; whole key blocks masked at the start, in the
middle and at the end of a sequence; a fully masked sequence; ragged lengths across block edges with empty sequences."""
import numpy as np
import pytest
import torch

from tests import attention_reference as ar
from tests.test_attention_census_gpu import replay

pytestmark = pytest.mark.gpu

K_B = 128
B, H = 3, 2
T_EDGES = (1, 17, 127, 128, 129, 256, 416, 417, 385, 513, 1024)
ALL_REGIMES_AT = (417, 513)


def dev():
    return torch.device("cuda:0")


class _StreamOps:
    """ops with attn_fwd / attn_bwd bound to the streamed entries: what tests/test_attention_census_gpu.py's replay() launches"""

    def __init__(self, ops, deterministic=False):
        self._ops, self._det = ops, deterministic

    def attn_fwd(self, **kw):
        self._ops.attn_stream_fwd(**kw)

    def attn_bwd(self, **kw):
        self._ops.attn_stream_bwd(deterministic=self._det, **kw)


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    return o


@pytest.fixture(scope="module")
def sops(ops):
    return _StreamOps(ops)


def _run(sops, f, regimes, what):
    fails = []
    for regime in regimes:
        _, _, _, per = replay(sops, f, regime, fails)
        print(f"{what} {ar.describe(f)} {regime}: worst err/bound " + " ".join(f"{k}={v:.3f}" for k, v in per.items()), flush=True)
    assert not fails, "\n".join(fails)


def _regimes(T, form="none"):
    if T not in ALL_REGIMES_AT:
        return ("flat", "planted")
    return ar.REGIMES


def random_mask(rows, T, seed, p=0.4):
    m = np.random.default_rng(seed).random((rows, T)) < p
    m[:, 0] = False
    return m


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("T", T_EDGES)
def test_lengths_at_every_edge_dense(sops, T, hd):
    _run(sops, ar.fields(B, T, H, hd), _regimes(T), "dense")


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("T", (127, 129, 417, 513, 1024))
def test_lengths_at_every_edge_key_mask(sops, T, hd):
    _run(sops, ar.fields(B, T, H, hd, "mask", mask=random_mask(B, T, T + hd)), _regimes(T), "key mask")


def block_mask(rows, T, seed, which, full_row=None):
    m = np.random.default_rng(seed).random((rows, T)) < 0.3
    nblk = (T + K_B - 1) // K_B
    kb = {"first": 0, "middle": nblk // 2, "last": nblk - 1}[which]
    m[:, kb * K_B:(kb + 1) * K_B] = True
    m[:, K_B if kb == 0 else 0] = False               # every row keeps a key outside the masked block
    if full_row is not None:
        m[full_row] = True
    return m


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("mask_group", [1, 3])
@pytest.mark.parametrize("which", ["first", "middle", "last"])
def test_whole_key_blocks_masked(sops, which, mask_group, hd):
    """513 tokens = four full blocks and one key: "last" masks exactly that key's block, "first" leaves the running maximum at -inf
    through the whole first block, "middle" puts a dead block between live ones."""
    T = 513
    rows = (B + mask_group - 1) // mask_group
    f = ar.fields(B, T, H, hd, "mask", mask=block_mask(rows, T, 11 + hd, which), mask_group=mask_group)
    _run(sops, f, ("flat", "planted", "extreme"), f"{which} block masked")


@pytest.mark.parametrize("hd", [32, 64])
def test_fully_masked_sequence(ops, sops, hd):
    T = 417
    f = ar.fields(B, T, H, hd, "mask", mask=block_mask(B, T, 5, "middle", full_row=1))
    fails = []
    o, ex_f, ex_b, per = replay(sops, f, "flat", fails)
    print(f"fully masked sequence hd={hd}: worst err/bound", per, flush=True)
    assert not fails, "\n".join(fails)
    rows = slice(T, 2 * T)
    assert bool(ex_f.dead[rows].all()) and not bool(ex_f.dead[:T].any())
    assert float(o.view("out")[rows].float().abs().max()) == 0.0
    assert bool((o.lse_rows()[rows] == float("inf")).all())
    assert float(o.view("dqkv")[rows].float().abs().max()) == 0.0          # dq = 0, and its keys are all masked: dk = dv = 0
    assert float(o.view("dbias_ws")[1].abs().max()) == 0.0                  # nothing taken from it into dbias


def _off(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


@pytest.mark.parametrize("hd", [32, 64])
def test_ragged_lengths_across_block_edges(sops, hd):
    lens = [0, 1, K_B, K_B + 1, 417, 600]
    for order in (lens, lens[::-1]):
        f = ar.fields(len(order), 600, H, hd, "ragged", seq_off=_off(order))
        _run(sops, f, ar.REGIMES if order is lens else ("flat", "planted"), "ragged")


@pytest.mark.parametrize("form", ["none", "mask", "ragged"])
@pytest.mark.parametrize("hd", [32, 64])
def test_old_and_new_kernels_on_the_same_operands(ops, sops, form, hd):
    """T = 400 is in the range of both families: each sits inside the fp64 bound on the same operands (no bit-equality is asked)."""
    T = 400
    f = {"none": ar.fields(B, T, H, hd), "mask": ar.fields(B, T, H, hd, "mask", mask=random_mask(B, T, 3)),
         "ragged": ar.fields(B, T, H, hd, "ragged", seq_off=_off([400, 257, 129]))}[form]
    for regime in ("flat", "planted"):
        fails, pers = [], {}
        for name, which in (("whole-image", ops), ("streamed", sops)):
            _, _, _, pers[name] = replay(which, f, regime, fails)
            fails = [f"{name}: {x}" for x in fails]
            assert not fails, "\n".join(fails)
        print(f"old against new, {ar.describe(f)} {regime}: " + "; ".join(
            f"{n}: " + " ".join(f"{k}={v:.3f}" for k, v in p.items()) for n, p in pers.items()), flush=True)


@pytest.mark.parametrize("form", ["mask", "ragged"])
def test_deterministic_mode_is_bit_reproducible(ops, form):
    """deterministic = 1: dqkv, dbias_ws and dbias bit-identical over three launches, and inside the bound."""
    T, hd = 513, 64
    f = (ar.fields(B, T, H, hd, "mask", mask=random_mask(B, T, 9)) if form == "mask" else
         ar.fields(B, T, H, hd, "ragged", seq_off=_off([513, 0, 130])))
    det = _StreamOps(ops, deterministic=True)
    o = ar.Operands(f, dev(), seed=1, regime="flat")
    snap_f = o.snapshot("fwd")
    det.attn_fwd(**o.fwd_kwargs())
    torch.cuda.synchronize()
    ex_f = ar.reference_fwd(o)
    bad, _ = ar.check(o, ex_f, snap_f, "fwd")
    assert not bad, "\n".join(bad)
    ex_b = ar.reference_bwd(o, ex_f)
    snap_b = o.snapshot("bwd")
    kept = []
    for _ in range(3):
        o.reset_outputs("bwd")
        det.attn_bwd(**o.bwd_kwargs(False))
        torch.cuda.synchronize()
        bad, _ = ar.check(o, ex_b, snap_b, "bwd", folded=True)
        assert not bad, "\n".join(bad)
        kept.append({n: o.b[n].t.clone() for n in snap_b})
    for other in kept[1:]:
        for n in ("dqkv", "dbias_ws", "dbias"):
            assert torch.equal(ar._ibits(kept[0][n]), ar._ibits(other[n])), n


def test_stream_entries_refuse_what_they_do_not_run(ops):
    from wavjepa_amd import _abi
    o = ar.Operands(ar.fields(1, 32, 2, 16), dev())
    with pytest.raises(_abi.WavJepaHipError, match="unsupported"):
        ops.attn_stream_fwd(**o.fwd_kwargs())
    kw = o.fwd_kwargs()
    kw.update(T=1025, hd=32)
    with pytest.raises(_abi.WavJepaHipError, match="invalid argument"):
        ops.attn_stream_fwd(**kw)
