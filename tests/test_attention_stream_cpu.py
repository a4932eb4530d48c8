"""The block-streamed attention entries (wj_attn_stream_fwd / wj_attn_stream_bwd, csrc/attention_stream.hip) on the host: argument
handling (every error is answered before a launch), the workspace query, the engine's choice of entry, and -- the evidence that
tests/attention_reference.py's bound applies to them unchanged -- an emulation of the kernels' arithmetic, block by block.

The emulation follows the kernels: keys in blocks of K_B = 128; pass 1 keeps, per LANE GROUP (key k of a 16-key tile belongs to group
(k % 16) // 4), a running maximum and a running sum that is rescaled by exp2((m_old - m_new) scale log2 e) once per block, merges the
four groups at the end; pass 2 forms P = exp2(s scale log2 e - m scale log2 e) * (1 / sum), rounds it to bf16 and accumulates P V block
after block in fp32; out is rounded to bf16 and lse = m scale + log(sum).  The backward recomputes p from the stored lse in the exp2
domain with the key mask inside the exponent, rounds dS and P to bf16, and accumulates dq over key blocks and dk / dv over query blocks
in fp32.  The only difference from the whole-image kernels is fp32 summation order and the fp32 rescale of the running sum -- both
below the T u32 terms the bound already carries -- so the emulation must pass attention_reference.check at the module's KAPPA, and
the GPU tests use the helper as it is.  Worst err / bound of the emulation over all cases: see PARITY.md."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import attention_reference as ar

DEV = torch.device("cpu")
K_B = 128


# ------------------------------------------------------------------------------------------------------------ arguments
def _fwd_args(_abi, **kw):
    a = _abi.STRUCTS["wj_attn_fwd_args"]()
    a.qkv = a.out = 16
    a.B, a.T, a.H, a.hd, a.mask_group = 1, 500, 2, 64, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _bwd_args(_abi, **kw):
    a = _abi.STRUCTS["wj_attn_bwd_args"]()
    a.qkv = a.out = a.dout = a.lse = a.dqkv = 16
    a.B, a.T, a.H, a.hd, a.mask_group = 1, 500, 2, 64, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_stream_entries_answer_bad_arguments_before_any_launch():
    from wavjepa_amd import _abi
    lib = _abi.load()
    assert lib.wj_abi_version() == 17
    for fn, mk, ptrs in ((lib.wj_attn_stream_fwd, _fwd_args, ("qkv", "out")),
                         (lib.wj_attn_stream_bwd, _bwd_args, ("qkv", "out", "dout", "lse", "dqkv"))):
        assert fn(None, None) == -1
        for p in ptrs:
            assert fn(ctypes.byref(mk(_abi, **{p: None})), None) == -1, p
        assert fn(ctypes.byref(mk(_abi, T=0)), None) == -1
        assert fn(ctypes.byref(mk(_abi, T=1025)), None) == -1
        assert fn(ctypes.byref(mk(_abi, mask_group=0)), None) == -1
        assert fn(ctypes.byref(mk(_abi, B=0)), None) == -1
        assert fn(ctypes.byref(mk(_abi, H=0)), None) == -1
        assert fn(ctypes.byref(mk(_abi, key_mask=16, seq_off=16)), None) == -1       # the ragged form takes no key mask
        assert fn(ctypes.byref(mk(_abi, hd=16)), None) == -3
        assert fn(ctypes.byref(mk(_abi, hd=48)), None) == -3
        assert fn(ctypes.byref(mk(_abi, hd=16, T=200)), None) == -3                  # 16-wide heads stay with the whole-image kernels
    assert lib.wj_attn_stream_bwd(ctypes.byref(_bwd_args(_abi, dbias=16)), None) == -1   # dbias without dbias_ws
    # the whole-image entries keep their limit and their answer
    assert lib.wj_attn_fwd(ctypes.byref(_fwd_args(_abi, T=500)), None) == -1
    assert lib.wj_attn_bwd(ctypes.byref(_bwd_args(_abi, T=500)), None) == -1


def test_stream_workspace_query():
    from wavjepa_amd import ops
    assert ops.workspace_bytes("wj_attn_stream_bwd", B=7, T=499, H=12, hd=64) == 7 * 3 * 12 * 64 * 4      # one row per sequence
    assert ops.workspace_bytes("wj_attn_stream_bwd", B=7, T=1000, H=12, hd=64) == ops.workspace_bytes("wj_attn_bwd", B=7, T=400, H=12, hd=64)
    from wavjepa_amd import _abi
    assert _abi.workspace_bytes("wj_attn_stream_fwd", _abi.STRUCTS["wj_attn_fwd_args"]()) == 0


def test_dispatch_picks_the_entries_by_the_length_of_the_call():
    from wavjepa_amd import ops
    assert ops.attn_entries(416) == ("wj_attn_fwd", "wj_attn_bwd")
    assert ops.attn_entries(417) == ("wj_attn_stream_fwd", "wj_attn_stream_bwd")
    assert ops.attn_entries(1) == ("wj_attn_fwd", "wj_attn_bwd")
    assert ops.attn_entries(1024) == ("wj_attn_stream_fwd", "wj_attn_stream_bwd")
    with pytest.raises(NotImplementedError):
        ops.attn_entries(1025)
    for name in ops.attn_entries(417):
        assert callable(getattr(ops, name[3:]))


def test_ten_second_model_constructs_on_the_host():
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.jepa import JEPA
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    spec = [(64, 10, 5)] + [(64, 3, 2)] * 4 + [(64, 2, 2)] * 2
    m = JEPA(feature_extractor=ConvFeatureExtractor(conv_layers_spec=spec, in_channels=1),
             transformer_encoder_cfg=TransformerEncoderCFG.create(num_layers=1),
             transformer_encoder_layers_cfg=TransformerLayerCFG.create(d_model=128, nhead=2),
             transformer_decoder_cfg=TransformerEncoderCFG.create(num_layers=1),
             transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=64, nhead=2),
             process_audio_seconds=10.0)
    assert m.total_patches == 499 and m.target_length == 160000
    assert tuple(m.pos_encoding_encoder.shape[-2:]) == (499, 128)


# ------------------------------------------------------------------------------------------------------------ emulation
def emulate_stream_fwd(o):
    f, ix = o.f, o.ix
    H, hd = f["H"], f["hd"]
    scale = np.float32(1.0 / math.sqrt(hd))
    scale2 = np.float32(scale * np.float32(ar.LOG2E))
    out, lse = o.view("out"), o.lse_rows().clone()
    ninf = float("-inf")
    for b in range(f["B"]):
        L, r0 = int(ix.len[b]), int(ix.row0[b])
        if L == 0:
            continue
        x = o.view("qkv")[r0:r0 + L].float().reshape(L, 3, H, hd)
        kv = ix.kval[b, :L]
        nblk = (L + K_B - 1) // K_B
        group = (torch.arange(L) % 16) // 4
        for h in range(H):
            q, k, v = x[:, 0, h], x[:, 1, h], x[:, 2, h]
            s = q @ k.t() + torch.where(kv, 0.0, ninf)[None, :]
            # ---- pass 1: per lane group, running maximum and rescaled running sum over the key blocks
            m_run = torch.full((4, L), ninf)
            l_run = torch.zeros(4, L)
            for kb in range(nblk):
                blk = slice(kb * K_B, min(L, (kb + 1) * K_B))
                for g in range(4):
                    sg = s[:, blk][:, group[blk] == g]
                    bm = torch.maximum(m_run[g], sg.amax(1)) if sg.shape[1] else m_run[g]
                    m2 = torch.where(torch.isinf(bm), torch.zeros_like(bm), bm) * scale2
                    l_run[g] = l_run[g] * torch.exp2(m_run[g] * scale2 - m2) + torch.exp2(sg * scale2 - m2[:, None]).sum(1)
                    m_run[g] = bm
            mx = m_run.amax(0)
            ms = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
            sm = (l_run * torch.exp2(m_run * scale2 - (ms * scale2)[None, :])).sum(0)
            inv = torch.where(sm > 0, 1.0 / sm, torch.zeros_like(sm))
            # ---- pass 2: normalised P in bf16, P V accumulated block after block
            acc = torch.zeros(L, hd)
            for kb in range(nblk):
                blk = slice(kb * K_B, min(L, (kb + 1) * K_B))
                P = (torch.exp2(s[:, blk] * scale2 - (ms * scale2)[:, None]) * inv[:, None]).to(torch.bfloat16).float()
                acc = acc + P @ v[blk]
            out[r0:r0 + L, h * hd:(h + 1) * hd] = acc.to(torch.bfloat16)
            lse[r0:r0 + L, h] = torch.where(sm > 0, ms * scale + torch.log(sm), torch.full_like(sm, float("inf")))
    if f["lse"]:
        o.set_lse_rows(lse, o.b["lse"].t)
    return lse


def emulate_stream_bwd(o, lse):
    f, ix = o.f, o.ix
    H, hd, D = f["H"], f["hd"], o.D
    scale = np.float32(1.0 / math.sqrt(hd))
    scale2 = np.float32(scale * np.float32(ar.LOG2E))
    log2e = np.float32(ar.LOG2E)
    dqkv, ws = o.view("dqkv"), o.view("dbias_ws")
    ninf = float("-inf")
    for b in range(f["B"]):
        L, r0 = int(ix.len[b]), int(ix.row0[b])
        if f["dbias"]:
            ws[b] = 0.0
        if L == 0:
            continue
        x = o.view("qkv")[r0:r0 + L].float().reshape(L, 3, H, hd)
        kvalid = torch.where(ix.kval[b, :L], 0.0, ninf)
        nblk = (L + K_B - 1) // K_B
        for h in range(H):
            c = slice(h * hd, (h + 1) * hd)
            q, k, v = x[:, 0, h], x[:, 1, h], x[:, 2, h]
            dO, O = o.view("dout")[r0:r0 + L, c].float(), o.view("out")[r0:r0 + L, c].float()
            l2 = lse[r0:r0 + L, h] * log2e
            delta = (dO * O).sum(1, keepdim=True)
            p = torch.exp2((q @ k.t()) * scale2 + (kvalid[None, :] - l2[:, None]))
            ds = (p * (dO @ v.t() - delta) * scale).to(torch.bfloat16).float()
            pb = p.to(torch.bfloat16).float()
            dq, dk, dv = torch.zeros(L, hd), torch.zeros(L, hd), torch.zeros(L, hd)
            for kb in range(nblk):                       # phase A: key blocks; phase B: query blocks
                blk = slice(kb * K_B, min(L, (kb + 1) * K_B))
                dq = dq + ds[:, blk] @ k[blk]
                dk = dk + ds[blk].t() @ q[blk]
                dv = dv + pb[blk].t() @ dO[blk]
            for j, val in enumerate((dq, dk, dv)):
                val = val.to(torch.bfloat16)
                dqkv[r0:r0 + L, j * D + h * hd:j * D + (h + 1) * hd] = val
                if f["dbias"]:
                    ws[b, j * D + h * hd:j * D + (h + 1) * hd] = val.float().sum(0)
    if f["dbias"] and not f["defer_fold"]:
        o.view("dbias").add_(ws.sum(0))


def run_case(f, regime, seed=0):
    o = ar.Operands(f, DEV, seed=seed, regime=regime)
    snap_f, snap_b = o.snapshot("fwd"), o.snapshot("bwd")
    lse = emulate_stream_fwd(o)
    ex_f = ar.reference_fwd(o)
    emulate_stream_bwd(o, lse)
    ex_b = ar.reference_bwd(o, ex_f)
    return o, ex_f, ex_b, snap_f, snap_b


def block_mask(rows, T, seed, which):
    """random 40 % key mask with one whole 128-key block masked: "first", "middle", "last" (every row keeps keys elsewhere)"""
    g = np.random.default_rng(seed)
    m = g.random((rows, T)) < 0.4
    nblk = (T + K_B - 1) // K_B
    kb = {"first": 0, "middle": nblk // 2, "last": nblk - 1}[which]
    m[:, kb * K_B:(kb + 1) * K_B] = True
    keep = K_B if kb == 0 else 0                       # a key that stays attended, outside the masked block
    m[:, keep] = False
    return m


def _off(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def ragged_lengths(T):
    """two sequences: one of the full length, one that ends one key into a block (and is no multiple of 16: the extreme regime's
    odd sequence needs padding keys)"""
    return [T, min(T - 1, ((T // 2) // K_B) * K_B + 1)]


def cases_for(T):
    return {"none": ar.fields(2, T, 2, 64),
            "mask": ar.fields(2, T, 2, 32, "mask", mask=block_mask(2, T, T, "middle")),
            "ragged": ar.fields(2, T, 2, 64, "ragged", seq_off=_off(ragged_lengths(T)))}


T_VALUES = (417, 512, 513, 1000)
# the extreme regime of the reference helper needs a sequence of odd index whose length is no multiple of 16 (padding keys of score 0
# above a very negative lse); at T = 512 the dense forms have none and Operands refuses to build the regime -- the ragged form covers it
GRID = [(T, form, r) for T in T_VALUES for form in ("none", "mask", "ragged") for r in ar.REGIMES
        if not (r == "extreme" and T % 16 == 0 and form != "ragged")]
WORST = {}


@pytest.mark.parametrize("T,form,regime", GRID, ids=[f"T{T}-{fo}-{r}" for T, fo, r in GRID])
def test_stream_emulation_is_within_the_unchanged_bound(T, form, regime):
    o, ex_f, ex_b, snap_f, snap_b = run_case(cases_for(T)[form], regime)
    bad_f, w_f = ar.check(o, ex_f, snap_f, "fwd")
    per = dict(ar.LAST)
    bad_b, w_b = ar.check(o, ex_b, snap_b, "bwd")
    per.update(ar.LAST)
    WORST[(T, form, regime)] = max(w_f, w_b)
    print(f"stream emulation T={T} {form} {regime}: worst err/bound " + " ".join(f"{k}={v:.3f}" for k, v in per.items())
          + f"   (largest so far {max(WORST.values()):.3f})")
    assert not bad_f and not bad_b, "\n".join(bad_f + bad_b)
    assert max(w_f, w_b) < 0.5, (w_f, w_b)       # the margin the whole-image emulation is held to (tests/test_attention_reference_cpu.py)


@pytest.mark.parametrize("regime", ("flat", "planted"))
@pytest.mark.parametrize("form", ("none", "mask", "ragged"))
def test_mutations_stay_rejected_at_513_tokens(form, regime):
    o, ex_f, ex_b, snap_f, snap_b = run_case(cases_for(513)[form], regime)
    outs_f = {n: o.b[n].t.clone() for n in snap_f}
    outs_b = {n: o.b[n].t.clone() for n in snap_b}
    names, missed = [], []
    for what, phase, mutated in ar.mutations(o, outs_f, outs_b):
        names.append(what)
        bad, _ = ar.check(o, ex_f if phase == "fwd" else ex_b, snap_f if phase == "fwd" else snap_b, phase, mutated)
        if not bad:
            missed.append(what)
    assert len(names) >= 14, names
    assert not missed, f"not rejected: {missed}"
