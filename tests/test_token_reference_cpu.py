"""The token-plumbing reference helper (tests/token_reference.py) on the host.

  * its backward agrees with torch float64 autograd through the forward it belongs to, and its exact forward with a plain fp32 add;
  * an fp32 numpy emulation of the backward in the kernel's order (a token's groups four at a time, a wave's rows in order,
    (w0 + w1) + (w2 + w3), the workgroups ascending and shuffled) stays below MARGIN of every bound;
  * every mutation is rejected on the emulation's output;
  * every field of the five argument structs is handled by the reference or named in its exclusion list.
"""
import collections
import random

import numpy as np
import torch

from tests import norm_reference as nr
from tests import token_reference as tr
from wavjepa_amd import _abi

MARGIN = 0.8
# every D at one (M, G), every G at D in {260, 768}, every M at D = 384
SHAPES = [(67, D, 4) for D in tr.WIDTHS] + [(67, D, G) for D in (260, 768) for G in tr.GROUPS] + [(M, 384, 5) for M in tr.ROWS]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def case(M, D, G, pattern, ragged, kind, seed):
    B, T = tr.split_rows(M)
    inv, n_ctx = tr.make_inv(pattern, M, seed)
    rows, rowmap = tr.make_ragged(inv, B, T, G, seed + 1) if ragged else (None, None)
    n_in = B * G * T if rows is None else int(rows.numel())
    d_in = tr.make_d_in(kind, n_in, D, seed + 2, rowmap, B, T, G)
    return B, T, inv, n_ctx, rows, rowmap, d_in


def test_references_agree_with_torch_float64_and_a_plain_fp32_add():
    M, D, G = 34, 12, 3
    for ragged in (False, True):
        B, T, inv, n_ctx, rows, rowmap, d_in = case(M, D, G, "mixed", ragged, "randn", 1)
        gen = torch.Generator().manual_seed(2)
        feats = torch.randn(n_ctx, D, generator=gen, dtype=torch.float64, requires_grad=True)
        mtok = torch.randn(D, generator=gen, dtype=torch.float64, requires_grad=True)
        pos = torch.randn(T, D, generator=gen, dtype=torch.float64)
        on = inv >= 0
        tok = mtok[None].expand(M, D).clone()
        tok[on] = feats[inv[on].long()]
        out = (tok.reshape(B, T, D) + pos)[:, None].expand(B, G, T, D).reshape(B * G * T, D)
        if ragged:
            out = out[rows.long()]
        (out * d_in.double()).sum().backward()
        ref = tr.scatter_fill_bwd(d_in, inv, rowmap, B, T, G, n_ctx)
        assert float((ref["dtok"][0][on][torch.argsort(inv[on])] - feats.grad).abs().max()) < 1e-12
        assert float((ref["d_mask_token"][0] - mtok.grad).abs().max()) < 1e-12
        assert float((ref["partials"][0].sum(0) - mtok.grad).abs().max()) < 1e-12
        assert torch.equal(ref["d_ctx_feats"][0], nr.bf16(feats.grad))
        if ragged:       # token 0: a context row no group sees
            assert int(inv[0]) == 0 and float(ref["d_ctx_feats"][0][0].abs().max()) == 0 and float(ref["d_ctx_feats"][1][0].abs().max()) == 0
        # forward: the mask token rounded first, one fp32 add, bf16 of the f32 output
        f16, mt32, p32 = feats.detach().to(torch.bfloat16), 0.02 * mtok.detach().float(), pos.float()
        fw = tr.scatter_fill(f16, inv, mt32, p32, B, T, G, rows)
        tok32 = mt32.to(torch.bfloat16).float()[None].expand(M, D).clone()
        tok32[on] = f16.float()[inv[on].long()]
        want = (tok32.reshape(B, T, D) + p32)[:, None].expand(B, G, T, D).reshape(B * G * T, D)
        want = want[rows.long()] if ragged else want
        assert torch.equal(fw["out_f32"][0].float(), want) and torch.equal(fw["out_bf16"][0].float(), want.to(torch.bfloat16).float())
    x = torch.randn(7, 8).to(torch.bfloat16)
    pos = torch.randn(3, 8)
    ap = tr.add_pos(x, pos, 3)
    assert torch.equal(ap["y_f32"][0].float(), x.float() + pos[torch.arange(7) % 3])
    inv = torch.tensor([2, -1, 0, -1, 1], dtype=torch.int32)
    src = torch.randn(3, 4)
    um = tr.unmask(src, inv, 5, False)[0].float()
    assert torch.equal(um[0], src[2]) and torch.equal(um[2], src[0]) and float(um[1].abs().max()) == 0 and float(um[3].abs().max()) == 0
    assert torch.equal(tr.unmask(src, None, 3, True)[0].float(), src.to(torch.bfloat16).float())
    assert torch.equal(tr.gather(src, torch.tensor([2, 0]))[0].float(), src[[2, 0]])


def test_backward_emulation_stays_below_the_margin_and_mutations_are_rejected():
    w = collections.defaultdict(float)
    rng = random.Random(3)
    n_mut = 0
    labels = set()
    for i, (M, D, G) in enumerate(SHAPES):
        for pattern in tr.PATTERNS:
            for ragged in (False, True):
                for kind in ("randn", "cancel"):
                    B, T, inv, n_ctx, rows, rowmap, d_in = case(M, D, G, pattern, ragged, kind, 10 + i)
                    ref = tr.scatter_fill_bwd(d_in, inv, rowmap, B, T, G, n_ctx)
                    nwg = ref["partials"][0].shape[0]
                    order = list(range(nwg))
                    rng.shuffle(order)
                    for o in (None, order):
                        got = tr.emulate_bwd(d_in, inv, rowmap, B, T, G, o)
                        for k in ("dtok", "d_ctx_feats", "partials", "d_mask_token"):
                            w[k + " " + kind] = max(w[k + " " + kind], nr.worst(t(got[k]), *ref[k]))
                    if pattern in ("mixed", "blocks"):
                        got = {k: t(v) for k, v in tr.emulate_bwd(d_in, inv, rowmap, B, T, G).items()}
                        for label, k, m in tr.bwd_mutations(got, d_in, inv, rowmap, B, T, G):
                            assert nr.rejected(m, *ref[k]), f"M={M} D={D} G={G} {pattern} ragged={ragged} {kind}: {label} ({k}) accepted"
                            n_mut += 1
                            labels.add(label)
                        trunc = tr.truncated(ref["dtok"][0][inv >= 0].float())
                        pair = (ref["d_ctx_feats"][0][inv[inv >= 0].long()], ref["d_ctx_feats"][1][inv[inv >= 0].long()])
                        if trunc.numel() and not (ragged and M == 1):
                            assert nr.rejected(trunc, *pair), f"M={M} D={D} G={G} {pattern} {kind}: truncated d_ctx_feats accepted"
    print()
    for k, v in w.items():
        print(f"emulation / bound  {k:22s} {v:.3f}")
    over = {k: v for k, v in w.items() if not v < MARGIN}
    assert not over, f"emulation above {MARGIN} of the bound: {over}"
    assert labels >= {"a group left out", "a group counted twice", "-1 in rowmap read as row 0", "the last row dropped",
                      "a masked row's sum routed to d_ctx_feats row 0", "chunk at column 256 stale", "chunk at column 512 stale"}, labels
    assert n_mut > 1000


def test_forward_mutations_change_the_exact_outputs():
    M, D, G = 67, 516, 3
    B, T = tr.split_rows(M)
    inv, n_ctx = tr.make_inv("mixed", M, 5)
    gen = torch.Generator().manual_seed(6)
    feats = torch.randn(n_ctx, D, generator=gen).to(torch.bfloat16)
    mtok, pos = 0.02 * torch.randn(D, generator=gen), torch.randn(T, D, generator=gen)
    ref = tr.scatter_fill(feats, inv, mtok, pos, B, T, G)
    for k in ("out_f32", "out_bf16"):
        assert nr.rejected(tr.scatter_fill(feats, inv, mtok, pos, B, T, G, shift=1)[k][0], *ref[k]), "pos[t + 1] accepted"
        assert nr.rejected(tr.scatter_fill(feats, inv, mtok, pos, B, T, G, round_token=False)[k][0], *ref[k]), "unrounded mask token accepted"
        for c in tr.stale_columns(D):
            assert nr.rejected(tr.mutate_chunk(ref[k][0], M * G - 1, c), *ref[k])
    assert nr.rejected(tr.truncated(ref["out_f32"][0].float()), *ref["out_bf16"]), "truncated bf16 accepted"
    x = torch.randn(M, D, generator=gen).to(torch.bfloat16)
    ap = tr.add_pos(x, pos, T)
    assert nr.rejected(tr.add_pos(x, pos, T, shift=1)["y_f32"][0], *ap["y_f32"]) and nr.rejected(tr.truncated(ap["y_f32"][0].float()), *ap["y_bf16"])


def test_every_field_of_the_argument_structs_is_handled_or_excluded():
    assert set(tr.HANDLED) == {"wj_add_pos_args", "wj_gather_args", "wj_scatter_fill_args", "wj_scatter_fill_bwd_args", "wj_unmask_rows_args"}
    for name, handled in tr.HANDLED.items():
        fields = {f for f, _ in _abi._STRUCT_FIELDS[name]}
        excluded = set(tr.EXCLUDED.get(name, {}))
        assert not (handled & excluded), name
        assert fields - handled - excluded == set(), f"{name}: fields without a reference or an exclusion: {sorted(fields - handled - excluded)}"
        assert (handled | excluded) - fields == set(), f"{name}: listed but not in the header: {sorted((handled | excluded) - fields)}"
