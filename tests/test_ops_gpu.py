"""Op-level parity of every C-ABI entry point against plain fp32 PyTorch math on the same inputs (GPU only).

Tolerances are stated per test: bf16 outputs are compared at bf16 resolution (2^-8 relative) on top of the fp32
reference; pure copies (gather) must be bit-exact.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    return o


def dev():
    return torch.device("cuda:0")


def rnd(*shape, scale=1.0, dtype=torch.float32, seed=None):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed if seed is not None else (hash(shape) & 0xFFFF))
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev())


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


# ------------------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("M,N,K", [(300, 192, 136), (1024, 768, 768), (128, 128, 64), (50, 64, 32)])
def test_gemm_nt_bias(ops, M, N, K):
    A = rnd(M, K, dtype=torch.bfloat16, seed=1)
    W = rnd(N, K, scale=0.1, dtype=torch.bfloat16, seed=2)
    bias = rnd(N, seed=3)
    C = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    ops.gemm(A, W, C, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias)
    ref = A.float() @ W.float().t() + bias
    assert relerr(C.float(), ref) < 4e-3
    assert maxerr(C.float(), ref) < 0.05 * float(ref.abs().max())


def test_gemm_nt_asymmetric_identity(ops):
    """A = I against an asymmetric B catches a transposed C write (guide: always check with asymmetric data)."""
    n = 128
    A = torch.eye(n, dtype=torch.bfloat16, device=dev())
    W = (torch.arange(n * n, device=dev()).reshape(n, n) % 251).to(torch.bfloat16)
    C = torch.empty(n, n, dtype=torch.bfloat16, device=dev())
    ops.gemm(A, W, C, M=n, N=n, K=n, lda=n, ldb=n, ldc=n)
    assert torch.equal(C.float(), W.float().t())


def test_gemm_bias_gelu2(ops):
    M, N, K = 260, 256, 128
    A = rnd(M, K, dtype=torch.bfloat16, seed=4)
    W = rnd(N, K, scale=0.2, dtype=torch.bfloat16, seed=5)
    bias = rnd(N, seed=6)
    H = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    G = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    ops.gemm(A, W, H, C2=G, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias, epilogue=ops.EPI_BIAS_GELU2)
    h = (A.float() @ W.float().t() + bias).to(torch.bfloat16).float()     # the pre-activation is a bf16 tensor
    hr = h.clone().requires_grad_(True)
    F.gelu(hr).sum().backward()
    assert relerr(G.float(), F.gelu(h)) < 6e-3                            # C2 = gelu(h)
    assert relerr(H.float(), hr.grad) < 6e-3                              # C  = gelu'(h), what the backward needs of h
    # elementwise: the fast erf (A&S 7.1.26, v_rcp) stays within one bf16 ulp of torch's erf-GELU
    assert maxerr(G.float(), F.gelu(h)) <= 2.0 ** -8 * float(F.gelu(h).abs().max())
    G1 = torch.empty_like(G)                                              # single-output form (teacher / inference)
    ops.gemm(A, W, G1, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias, epilogue=ops.EPI_BIAS_GELU)
    assert torch.equal(G1, G)


@pytest.mark.parametrize("M,N,K,epi", [
    (8192, 2048, 256, "BF16"),          # 256 tiles: one per resident workgroup, nothing pulled
    (16500, 1152, 128, "BF16"),         # M and N edges (shifted tiles), two K tiles per output tile, 325 tiles
    (20000, 1024, 384, "BIAS_GELU2"),   # two outputs, tiles pulled from the per-XCD counters
    (20000, 768, 256, "BIAS_GELU"),
    (16080, 512, 1024, "CONV_GELU"),    # 40 segments of 402 rows, 400 valid
    (16384, 2304, 256, "BIAS_GELU"),    # 64 panels x 9 items: every XCD owns whole panels (the shapes WJ_PERSIST_WBLOCK re-orders)
    (8192, 3072, 128, "BF16"),          # 32 panels x 12 items
])
def test_gemm_persistent_schedule(ops, M, N, K, epi):
    """The persistent eight-phase kernel (csrc/gemm_persist.hip, variant 4) through the C ABI: fp32 torch reference at bf16 resolution;
    against variant 3 only last-place differences (it starts its accumulators from the bias); NaN-filled outputs, launched five
    times: a tile the scheduler skipped would stay NaN, a race would differ between launches."""
    e = getattr(ops, "EPI_" + epi)
    A = rnd(M, K, dtype=torch.bfloat16, seed=11)
    W = rnd(N, K, scale=0.08, dtype=torch.bfloat16, seed=12)
    bias = rnd(N, seed=13)
    kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, epilogue=e)
    if epi == "CONV_GELU":
        kw.update(seg_rows=402, seg_valid=400)
    else:
        kw["bias"] = bias
    two = epi in ("BIAS_GELU2", "CONV_GELU")

    def run(variant):
        C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
        C2 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev()) if two else None
        prev = ops.gemm_set_variant(variant)
        try:
            ops.gemm(A, W, C, **(dict(kw, C2=C2) if two else kw))
            torch.cuda.synchronize()
        finally:
            ops.gemm_set_variant(prev)
        return C, C2

    C4, C24 = run(4)
    assert not bool(torch.isnan(C4.float()).any()) and (C24 is None or not bool(torch.isnan(C24.float()).any()))
    for _ in range(4):
        Cr, C2r = run(4)
        assert torch.equal(Cr.view(torch.int16), C4.view(torch.int16))
        assert C24 is None or torch.equal(C2r.view(torch.int16), C24.view(torch.int16))
    C3, C23 = run(3)
    for x, y in ((C3, C4),) + (((C23, C24),) if two else ()):
        d = (x.float() - y.float()).abs()
        assert float((d > 0).float().mean()) < 2e-3                       # measured: <= 0.05 % of the elements
        assert bool((d <= 2.0 ** -6 * torch.maximum(x.float().abs(), y.float().abs()) + 4e-3).all())
    h = A.float() @ W.float().t() + (0 if epi == "CONV_GELU" else bias)
    if epi == "BF16":
        assert relerr(C4.float(), h) < 4e-3
    else:
        hb = h.to(torch.bfloat16).float()
        g = F.gelu(hb)
        if epi == "BIAS_GELU":
            assert relerr(C4.float(), g) < 6e-3
        elif epi == "BIAS_GELU2":
            hr = hb.clone().requires_grad_(True)
            F.gelu(hr).sum().backward()
            assert relerr(C24.float(), g) < 6e-3 and relerr(C4.float(), hr.grad) < 6e-3
        else:
            valid = ((torch.arange(M, device=dev()) % 402) < 400).float()[:, None]
            assert relerr(C4.float(), hb * valid) < 4e-3 and relerr(C24.float(), g * valid) < 6e-3


@pytest.mark.parametrize("M,N,K", [(9945, 768, 3072),       # the ragged student's linear2 / linear1-dgrad: 117 tiles -> 234 workgroups
                                   (9945, 768, 2304),       # in_proj dgrad (18 K tiles per half)
                                   (8500, 1024, 1536),      # 34 x 4 = 136 tiles: too many for one round -> stays unsplit (same bits)
                                   (2200, 1024, 1536),      # 36 tiles, M edge inside the last panel
                                   (16384, 512, 1536)])     # 128 tiles: the largest split problem (every XCD: 16 + 16 workgroups)
def test_gemm_k_split_pairs(ops, M, N, K):
    """K-split pairs of the eight-phase schedule (wj_gemm_args.workspace): two workgroups per output tile, half of K each, fp32 partial
    sums exchanged through the scratch.  Through the C ABI on NaN-filled outputs: against the fp32 reference at bf16 resolution; against
    the unsplit launch only last-place differences (fp32 sums of two halves instead of one chain); five launches bit-identical (a flag
    left set, a partial read before it was posted or a tile half nobody finished would show); the scratch's flags are back at zero."""
    A = rnd(M, K, dtype=torch.bfloat16, seed=21)
    W = rnd(N, K, scale=0.05, dtype=torch.bfloat16, seed=22)
    bias = rnd(N, seed=23)
    kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias)
    need = ops.workspace_bytes("wj_gemm_bf16", M=M, N=N, K=K, lda=K, ldb=K, ldc=N, epilogue=ops.EPI_BF16)
    tiles = -(-M // 256) * (N // 256)
    assert (need > 0) == (32 < tiles <= 128)
    ws = torch.zeros(max(need, 256), dtype=torch.uint8, device=dev())

    def run(workspace):
        C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
        ops.gemm(A, W, C, workspace=workspace, **kw)
        torch.cuda.synchronize()
        return C

    C0 = run(None)
    C1 = run(ws)
    assert not bool(torch.isnan(C1.float()).any())
    for _ in range(4):
        assert torch.equal(run(ws).view(torch.int16), C1.view(torch.int16))
    assert int(ws[:tiles * 8].view(torch.int32).abs().sum()) == 0          # every flag consumed
    h = A.float() @ W.float().t() + bias
    assert relerr(C1.float(), h) < 4e-3
    d = (C0.float() - C1.float()).abs()
    if need == 0:
        assert torch.equal(C0.view(torch.int16), C1.view(torch.int16))
    else:
        assert float((d > 0).float().mean()) < 2e-2
        assert bool((d <= 2.0 ** -6 * torch.maximum(C0.float().abs(), C1.float().abs()) + 4e-3).all())
    if need:
        # a second product through the same scratch, alternating with the first: a partial sum read from a stale cache line (the
        # partner's workgroup runs on another CU, usually another XCD = another L2) would carry the OTHER product's values
        A2 = rnd(M, K, dtype=torch.bfloat16, seed=24)
        h2 = A2.float() @ W.float().t() + bias
        C2 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
        for it in range(6):
            ops.gemm(A2, W, C2, workspace=ws, **kw)
            ops.gemm(A, W, C0, workspace=ws, **kw)           # back to back, no host synchronisation in between
        torch.cuda.synchronize()
        assert relerr(C2.float(), h2) < 4e-3 and torch.equal(C0.view(torch.int16), C1.view(torch.int16))
        C0 = run(None)
    # a scratch that is too small is ignored (one workgroup per tile), not overrun
    if need:
        small = torch.zeros(need // 2, dtype=torch.uint8, device=dev())
        assert torch.equal(run(small).view(torch.int16), C0.view(torch.int16)) and int(small.view(torch.int32).abs().sum()) == 0


@pytest.mark.parametrize("M,N,K,cus", [(33100, 384, 384, 32),      # a full + a half-width item per 256-row panel, shifted M edge
                                        (33100, 640, 256, 32),      # two full tiles + a half-width item
                                        (40000, 384, 1152, 28),     # fewer resident workgroups per XCD (the data-parallel default)
                                        (20000, 1152, 128, 5)])     # ... far fewer: every workgroup pulls many items
def test_gemm_persistent_half_width_items_and_fewer_workgroups(ops, M, N, K, cus):
    """N % 256 == 128: the last work item of a row panel is 128 columns wide (no duplicated columns).  Through the C ABI on NaN-filled
    outputs: bit-identical to the one-tile eight-phase kernel up to the bias-first last-place differences, bit-identical to itself
    across launches and across the number of resident workgroups per XCD (wj_gemm_set_persist_cus)."""
    A = rnd(M, K, dtype=torch.bfloat16, seed=21)
    W = rnd(N, K, scale=0.08, dtype=torch.bfloat16, seed=22)
    bias = rnd(N, seed=23)
    kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias)

    def run(variant, n_cus):
        C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
        prev_v, prev_c = ops.gemm_set_variant(variant), ops.gemm_set_persist_cus(n_cus)
        try:
            ops.gemm(A, W, C, **kw)
            torch.cuda.synchronize()
        finally:
            ops.gemm_set_variant(prev_v)
            ops.gemm_set_persist_cus(prev_c)
        return C

    C4 = run(4, cus)
    assert not bool(torch.isnan(C4.float()).any())
    for n_cus in (cus, 32, 17):
        assert torch.equal(run(4, n_cus).view(torch.int16), C4.view(torch.int16)), n_cus
    C3 = run(3, 32)
    d = (C3.float() - C4.float()).abs()
    assert float((d > 0).float().mean()) < 2e-3 and bool((d <= 2.0 ** -6 * torch.maximum(C3.float().abs(), C4.float().abs()) + 1e-4).all())
    assert relerr(C4.float(), A.float() @ W.float().t() + bias) < 4e-3
    assert ops.gemm_set_persist_cus(0) == 32                 # the process default is untouched


@pytest.mark.parametrize("M,K,cus,with_bias", [(33100, 384, 32, True),      # 259 panels, the last one shifted inwards; 6 K tiles
                                                (40000, 1152, 28, True),     # fewer resident workgroups per XCD (the data-parallel default)
                                                (87421, 1536, 32, False),    # the predictor's linear2 / linear1-dgrad at full size
                                                (5003, 256, 32, True),       # fewer panels (40) than workgroups; the shortest K (4 K tiles)
                                                (128, 768, 32, False),       # one panel
                                                (20001, 384, 5, True)])      # every workgroup walks many panels
def test_gemm_row_panel_schedule_for_thin_outputs(ops, M, K, cus, with_bias):
    """Variant 5 (csrc/gemm_panel.hip): N = 384 as full-row work items of 128 rows x 384 columns, A staged four K tiles ahead by waves of its
    own (the predictor's out_proj / linear2 / dgrads into d = 384; autograd of reference jepa.py:129-131,422-440).  On NaN-filled outputs:
    against fp32 torch math, BIT-IDENTICAL to the one-tile eight-phase kernel (same k order, bias added last), to itself across launches
    and across the number of resident workgroups per XCD."""
    N = 384
    A = rnd(M, K, dtype=torch.bfloat16, seed=61)
    W = rnd(N, K, scale=0.08, dtype=torch.bfloat16, seed=62)
    bias = rnd(N, seed=63) if with_bias else None
    kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias)

    def run(variant, n_cus=None):
        C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
        ops.gemm(A, W, C, schedule=variant, persist_cus=n_cus, **kw)
        torch.cuda.synchronize()
        return C

    C5 = run(5, cus)
    assert not bool(torch.isnan(C5.float()).any())
    ref = A.float() @ W.float().t() + (bias if with_bias else 0.0)
    assert relerr(C5.float(), ref) < 4e-3
    C3 = run(3)
    assert torch.equal(C5.view(torch.int16), C3.view(torch.int16))
    for n_cus in (cus, 32, 17):
        assert torch.equal(run(5, n_cus).view(torch.int16), C5.view(torch.int16)), n_cus
    # the automatic choice takes it where the rows fill the chip, and keeps the other schedules elsewhere
    Ca = run(-1)
    assert relerr(Ca.float(), ref) < 4e-3
    # strided operands (a column block of a wider activation, output into a column block of a wider buffer)
    if M <= 40000:
        Abig = rnd(M, K + 128, dtype=torch.bfloat16, seed=64)
        Cbig = torch.full((M, N + 256), float("nan"), dtype=torch.bfloat16, device=dev())
        ops.gemm(Abig, W, Cbig, M=M, N=N, K=K, lda=K + 128, ldb=K, ldc=N + 256, bias=bias, schedule=5)
        torch.cuda.synchronize()
        want = Abig[:, :K].float() @ W.float().t() + (bias if with_bias else 0.0)
        assert relerr(Cbig[:, :N].float(), want) < 4e-3 and bool(torch.isnan(Cbig[:, N:].float()).all())


@pytest.mark.parametrize("M,N,K,epi,cus", [(51200, 3072, 768, "gelu", None),     # the teacher's linear1
                                            (86317, 1536, 384, "gelu2", None),     # the predictor's linear1 (ragged rows: a shifted last panel)
                                            (9907, 3072, 768, "gelu2", 28),        # the student's linear1; 28 resident workgroups per XCD
                                            (16640, 1024, 256, "gelu2", None),     # four K tiles: every K tile of an item carries a block
                                            (102912, 512, 1536, "conv", None),     # a sparse conv layer (402-row segments, 400 valid)
                                            (33000, 512, 1024, "conv", 5),         # few resident workgroups: long item queues
                                            (65664, 256, 512, "gelu", None)])      # one item per panel
def test_gemm_deferred_epilogue_schedule(ops, M, N, K, epi, cus):
    """Variant 6 (csrc/gemm_pde.hip): 128 x 256 work items whose GELU epilogue is deferred -- the finished tile is parked as packed bf16 and
    taken through GELU / the stores in four blocks inside the next item's K loop (reference jepa.py:129-131 + the transformer MLPs; conv
    layers of extractors/audio_feature_extractor.py:54-138).  On NaN-filled outputs: against fp32 torch math, and BIT-IDENTICAL to the
    persistent 256 x 256 kernel (same k order, accumulators started from the bias, same GELU code), to itself across launches and across the
    number of resident workgroups."""
    A = rnd(M, K, dtype=torch.bfloat16, seed=81)
    W = rnd(N, K, scale=0.06, dtype=torch.bfloat16, seed=82)
    bias = rnd(N, seed=83)
    code = {"gelu": ops.EPI_BIAS_GELU, "gelu2": ops.EPI_BIAS_GELU2, "conv": ops.EPI_CONV_GELU}[epi]
    kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, epilogue=code)
    if epi == "conv":
        kw.update(seg_rows=402, seg_valid=400)
    else:
        kw["bias"] = bias

    def run(variant, n_cus=None):
        C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
        C2 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev()) if epi != "gelu" else None
        ops.gemm(A, W, C, C2=C2, schedule=variant, persist_cus=n_cus, **kw)
        torch.cuda.synchronize()
        return C, C2

    C6, C6b = run(6, cus)
    h = (A.float() @ W.float().t() + (bias if epi != "conv" else 0.0)).to(torch.bfloat16).float()
    if epi == "conv":
        valid = (torch.arange(M, device=dev()) % 402 < 400).float()[:, None]
        assert relerr(C6.float(), h * valid) < 4e-3                                        # C = pre-activation, C2 = GELU, rows outside the segments 0
        assert relerr(C6b.float(), F.gelu(h) * valid) < 6e-3
        assert float(C6.float()[401::402].abs().max()) == 0.0 and float(C6b.float()[400::402].abs().max()) == 0.0
    elif epi == "gelu2":
        gp = 0.5 * (1 + torch.erf(h / math.sqrt(2))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2 * math.pi)
        assert relerr(C6.float(), gp) < 6e-3                                               # C = gelu'(h), C2 = gelu(h)
        assert relerr(C6b.float(), F.gelu(h)) < 6e-3
    else:
        assert relerr(C6.float(), F.gelu(h)) < 6e-3
    C4, C4b = run(4)
    assert torch.equal(C6.view(torch.int16), C4.view(torch.int16))
    assert C6b is None or torch.equal(C6b.view(torch.int16), C4b.view(torch.int16))
    for n_cus in (cus, 32, 11):
        Cx, Cxb = run(6, n_cus)
        assert torch.equal(Cx.view(torch.int16), C6.view(torch.int16)), n_cus
        assert C6b is None or torch.equal(Cxb.view(torch.int16), C6b.view(torch.int16)), n_cus


def test_gemm_deferred_epilogue_repeated_launches_beside_another_stream(ops):
    """60 launches of the deferred-epilogue kernel on two streams at once (each workgroup then finds its CU shared or late and pulls fewer
    items), into NaN-filled outputs: every launch gives the first one's bits.  A wait that counted one store too many or too few shows as
    stale operand tiles in a few items."""
    M, N, K = 86317, 1536, 384
    A = rnd(M, K, dtype=torch.bfloat16, seed=84)
    W = rnd(N, K, scale=0.06, dtype=torch.bfloat16, seed=85)
    bias = rnd(N, seed=86)
    kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, epilogue=ops.EPI_BIAS_GELU2, bias=bias, schedule=6)
    ref, ref2 = (torch.empty(M, N, dtype=torch.bfloat16, device=dev()) for _ in range(2))
    ops.gemm(A, W, ref, C2=ref2, **kw)
    torch.cuda.synchronize()
    outs = [(torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev()), torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev()))
            for _ in range(4)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for rep in range(15):
        for j, st in enumerate(streams):
            with torch.cuda.stream(st):
                for q in range(2):
                    ops.gemm(A, W, outs[2 * j + q][0], C2=outs[2 * j + q][1], **kw)
        torch.cuda.synchronize()
        for o, o2 in outs:
            assert torch.equal(o.view(torch.int16), ref.view(torch.int16)) and torch.equal(o2.view(torch.int16), ref2.view(torch.int16)), rep
            o.fill_(float("nan")); o2.fill_(float("nan"))


def test_gemm_row_panel_repeated_launches_are_bit_identical(ops):
    """60 launches of the row-panel kernel into NaN-filled outputs (two streams alternating): every one gives the first one's bits."""
    M, N, K = 87000, 384, 1152
    A = rnd(M, K, dtype=torch.bfloat16, seed=65)
    W = rnd(N, K, scale=0.08, dtype=torch.bfloat16, seed=66)
    outs = [torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev()) for _ in range(4)]
    ref = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    ops.gemm(A, W, ref, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, schedule=5)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for rep in range(60):
        with torch.cuda.stream(streams[rep & 1]):
            outs[rep & 3].fill_(float("nan"))
            ops.gemm(A, W, outs[rep & 3], M=M, N=N, K=K, lda=K, ldb=K, ldc=N, schedule=5)
        if rep % 4 == 3:
            torch.cuda.synchronize()
            for o in outs:
                assert torch.equal(o.view(torch.int16), ref.view(torch.int16)), rep


@pytest.mark.parametrize("M,N,K", [(33001, 1536, 384), (20000, 640, 256), (9907, 3072, 768)])
def test_gemm_persistent_mul_gelu_grad_with_column_sums(ops, M, N, K):
    """The backward through linear2 + GELU as a row-form GEMM against W^T on the persistent kernel (reference: autograd of
    nn.TransformerEncoderLayer's `linear2(activation(linear1(x)))`, types/wavjepa_configs.py:28-47): C = bf16(bf16(acc) * gelu'(h)), and
    the column sums of C (linear1's bias gradient) ADDED to what the buffer holds.  Bit-identical to the one-tile schedule; the sums
    against float64 sums of the stored values; rows that a shifted M-edge tile shares with its neighbour are counted once."""
    dY = rnd(M, K, dtype=torch.bfloat16, seed=31)
    Wt = rnd(N, K, scale=0.08, dtype=torch.bfloat16, seed=32)       # W^T: [N][K], K contiguous
    gp = (torch.rand(M, N, device=dev(), generator=torch.Generator(device=dev()).manual_seed(33)) * 1.2 - 0.1).to(torch.bfloat16)
    kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, epilogue=ops.EPI_MUL_GELU_GRAD, aux=gp)
    out = {}
    for v in (3, 4):
        C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
        cs = torch.full((N,), 0.5, device=dev())
        prev = ops.gemm_set_variant(v)
        try:
            ops.gemm(dY, Wt, C, colsum=cs, **kw)
            torch.cuda.synchronize()
        finally:
            ops.gemm_set_variant(prev)
        out[v] = (C, cs)
    assert torch.equal(out[3][0].view(torch.int16), out[4][0].view(torch.int16))
    C = out[4][0].float()
    want = 0.5 + C.sum(0, dtype=torch.float64)
    scale = C.abs().sum(0, dtype=torch.float64) + 1e-6
    for v in (3, 4):
        assert float(((out[v][1].double() - want).abs() / scale).max()) < 2e-5, v
    assert relerr(C, (dY.float() @ Wt.float().t()).to(torch.bfloat16).float() * gp.float()) < 6e-3


def test_transpose_bf16_batched(ops):
    """wj_transpose_bf16: several matrices of one flat buffer transposed in place of their own offsets in a second one (the W^T shadows
    of the row-form dgrads)."""
    shapes = [(384, 1152), (1536, 384), (64, 64), (768, 3072)]
    offs, rows, tiles, total = [], [], 0, 0
    for r, c in shapes:
        offs.append(total)
        rows.append((total, r, c, tiles))
        tiles += (r // 64) * (c // 64)
        total += r * c + 8                                   # slots are padded to 8 elements in the flat layout
    src = rnd(total, dtype=torch.bfloat16, seed=41)
    dst = torch.full((total,), float("nan"), dtype=torch.bfloat16, device=dev())
    table = torch.tensor(rows, dtype=torch.int64, device=dev())
    ops.transpose_bf16(src, dst, table, len(rows), tiles)
    for (r, c), o in zip(shapes, offs):
        assert torch.equal(dst[o:o + r * c].view(c, r), src[o:o + r * c].view(r, c).t())


@pytest.mark.parametrize("M,N,K", [(300, 136, 192), (512, 768, 3072)])
def test_gemm_dgrad_layout(ops, M, N, K):
    """dX[M, N] = dY[M, K] @ W[K, N]  (b_trans: W stored [K][N], N contiguous)."""
    dY = rnd(M, K, dtype=torch.bfloat16, seed=7)
    W = rnd(K, N, scale=0.1, dtype=torch.bfloat16, seed=8)
    C = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    ops.gemm(dY, W, C, M=M, N=N, K=K, lda=K, ldb=N, ldc=N, b_trans=1)
    ref = dY.float() @ W.float()
    assert relerr(C.float(), ref) < 4e-3
    # fp32 output + addend
    add = rnd(M, N, seed=9)
    C32 = torch.empty(M, N, dtype=torch.float32, device=dev())
    ops.gemm(dY, W, C32, M=M, N=N, K=K, lda=K, ldb=N, ldc=N, b_trans=1, epilogue=ops.EPI_ADD_F32, aux=add)
    assert relerr(C32, ref + add) < 1e-3
    # gelu-grad epilogue (+ fused column sums = bias gradient of the producing Linear)
    Hpre = rnd(M, N, dtype=torch.bfloat16, seed=10)
    Cg = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    cs = torch.ones(N, device=dev())
    ops.gemm(dY, W, Cg, M=M, N=N, K=K, lda=K, ldb=N, ldc=N, b_trans=1, epilogue=ops.EPI_MUL_GELU_GRAD, aux=Hpre, colsum=cs)
    assert relerr(cs, 1 + Cg.float().sum(0)) < 1e-4
    cs2 = torch.zeros(N, device=dev())
    ops.gemm(dY, W, C, M=M, N=N, K=K, lda=K, ldb=N, ldc=N, b_trans=1, colsum=cs2)
    assert relerr(cs2, C.float().sum(0)) < 1e-4
    assert relerr(Cg.float(), ref.to(torch.bfloat16).float() * Hpre.float()) < 6e-3    # aux = saved gelu'(h)


@pytest.mark.parametrize("Mtok,Nout,Kin,split", [(1000, 192, 136, 1), (4096, 256, 384, 4), (800, 64, 64, 3)])
def test_gemm_wgrad_layout(ops, Mtok, Nout, Kin, split):
    """dW[Nout, Kin] += dY[Mtok, Nout]^T @ X[Mtok, Kin]  (both operands stored with the contraction as rows)."""
    dY = rnd(Mtok, Nout, dtype=torch.bfloat16, seed=11)
    X = rnd(Mtok, Kin, dtype=torch.bfloat16, seed=12)
    dW = torch.ones(Nout, Kin, dtype=torch.float32, device=dev())
    ops.gemm(dY, X, dW, M=Nout, N=Kin, K=Mtok, lda=Nout, ldb=Kin, ldc=Kin, a_trans=1, b_trans=1,
             epilogue=ops.EPI_ATOMIC_F32, split_k=split, alpha=0.5)
    ref = 1.0 + 0.5 * (dY.float().t() @ X.float())
    assert relerr(dW, ref) < 1e-3


@pytest.mark.parametrize("dims,K", [([(384, 128), (128, 128), (512, 128), (128, 512)], 1000), ([(192, 64), (64, 64), (256, 64), (64, 256)] * 2, 777),
                                    ([(2304, 768), (768, 768)], 2500),
                                    # a predictor layer (every shape has a 384: half-full row tiles of the 256 x 128 schedule) and a 72-row tail
                                    ([(1152, 384), (384, 384), (1536, 384), (384, 1536), (328, 256)], 9000),
                                    # exactly a predictor layer: every problem a multiple of 384 x 128 -> the 384 x 128 tile (36 full tiles,
                                    # split-K 7; K with a tail that is not a multiple of the 32-deep K tile), and two layers' worth in one group
                                    ([(1152, 384), (384, 384), (1536, 384), (384, 1536)], 21001),
                                    ([(1152, 384), (384, 384), (1536, 384), (384, 1536)] * 2, 5000)])
def test_wgrad_grouped(ops, dims, K):
    """Several dW = dY^T X problems in one launch (one split-K factor for the group) == the individual fp32 products, accumulated
    on top of what the gradient buffers already hold."""
    probs, refs = [], []
    for i, (n_out, k_in) in enumerate(dims):
        dy = rnd(K, n_out, dtype=torch.bfloat16, seed=300 + i)
        x = rnd(K, k_in, dtype=torch.bfloat16, seed=400 + i)
        gw = rnd(n_out, k_in, seed=500 + i)
        refs.append(gw.clone() + dy.float().t() @ x.float())
        probs.append((dy, x, gw, n_out, k_in, K))
    ops.wgrad_grouped(probs)
    for (dy, x, gw, *_), ref in zip(probs, refs):
        assert relerr(gw, ref) < 2e-5


def test_gemm_gather_forms(ops):
    """Sparse conv backward GEMMs: logical rows / logical k taken from a row list == the dense GEMM on compacted copies."""
    g = torch.Generator().manual_seed(20)
    C, k, s_ = 512, 3, 2
    rows_out, rows_in = 3000, 6016                                # layer rows (all clips), previous layer rows
    sel = torch.sort(torch.randperm(rows_out - 4, generator=g)[:700] + 2).values.to(torch.int32).to(dev())
    n = int(sel.numel())
    # --- dgrad (row gather): C[rowmap[m]] = A[rowmap[m] .. +U rows] @ W, U = 2 taps spanning consecutive rows
    U = 2
    dpre = rnd(rows_out + 8, C, dtype=torch.bfloat16, seed=21)
    wd = rnd(U * C, C, scale=0.05, dtype=torch.bfloat16, seed=22)
    out = torch.zeros(rows_in + 16, C, dtype=torch.bfloat16, device=dev())
    a_ptr = dpre.data_ptr() + (2 - (U - 1)) * C * 2                # logical row g starts at storage row 2 + g - (U-1)
    ops.gemm(a_ptr, wd, out.data_ptr(), M=n, N=C, K=U * C, lda=C, ldb=C, ldc=s_ * C, b_trans=1, rowmap=sel)
    A = torch.cat([dpre[1 + sel.long()], dpre[2 + sel.long()]], 1).float()           # rows g-1, g of the logical matrix
    want = (A @ wd.float()).to(torch.bfloat16)
    got = out.view(-1)[: (rows_in // s_) * s_ * C].view(-1, s_ * C)[sel.long(), :C]
    assert relerr(got.float(), want.float()) < 4e-3
    mask = torch.ones(out.shape[0] * C // (s_ * C), dtype=torch.bool, device=dev())
    mask[sel.long()] = False
    assert float(out.view(-1)[: mask.numel() * s_ * C].view(-1, s_ * C)[mask].abs().max()) == 0.0   # nothing else written
    # --- the same dgrad with GELU' of the layer below fused into its epilogue: exactly the bits of the plain form followed by
    #     wj_gelu_bwd_bf16 over the rows it wrote (and nothing else written)
    pre = rnd(rows_in + 16, C, scale=1.5, dtype=torch.bfloat16, seed=25)
    out2 = torch.zeros(rows_in + 16, C, dtype=torch.bfloat16, device=dev())
    ops.gemm(a_ptr, wd, out2.data_ptr(), M=n, N=C, K=U * C, lda=C, ldb=C, ldc=s_ * C, b_trans=1, rowmap=sel,
             epilogue=ops.EPI_MUL_GELU_GRAD_Z, aux=pre.data_ptr())
    ref2 = torch.zeros_like(out)
    ops.gelu_bwd_bf16(out, pre, ref2, out.numel())
    view = lambda t: t.view(-1)[: (rows_in // s_) * s_ * C].view(-1, s_ * C)
    assert torch.equal(view(out2)[sel.long(), :C].view(torch.int16), view(ref2)[sel.long(), :C].view(torch.int16))
    full = out2.view(-1)[: mask.numel() * s_ * C].view(-1, s_ * C)
    assert float(full[mask].abs().max()) == 0.0 and float(full[:, C:].abs().max()) == 0.0
    # --- wgrad (k gather): dW[o][kk*C + c] = sum_{g in list} dY[g][o] * X[s*g + kk][c]
    dy = rnd(rows_out, C, dtype=torch.bfloat16, seed=23)
    x = rnd(rows_in + 16, C, scale=0.3, dtype=torch.bfloat16, seed=24)
    dw = torch.zeros(C, k * C, device=dev())
    lst = torch.cat([sel, torch.zeros(256, dtype=torch.int32, device=dev())])
    ops.gemm(dy, x, dw, M=C, N=k * C, K=n, lda=C, ldb=s_ * C, ldc=k * C, a_trans=1, b_trans=1, epilogue=ops.EPI_ATOMIC_F32,
             split_k=ops.pick_split_k(C, k * C, n), rowmap=lst)
    X = torch.cat([x[s_ * sel.long() + kk] for kk in range(k)], 1).float()
    want = dy[sel.long()].float().t() @ X
    assert relerr(dw, want) < 2e-3
    from wavjepa_amd._abi import WavJepaHipError
    with pytest.raises(WavJepaHipError):                          # no gather form for the forward layout
        ops.gemm(dy, x, out, M=64, N=C, K=C, lda=C, ldb=C, ldc=C, rowmap=sel)


def test_gelu_bwd_rows_and_zero_rows(ops):
    R, C = 500, 512
    dpost = rnd(R, C, dtype=torch.bfloat16, seed=25)
    pre = rnd(R, C, dtype=torch.bfloat16, seed=26)
    dense = torch.empty_like(dpost)
    ops.gelu_bwd_bf16(dpost, pre, dense, R * C)
    rows = torch.tensor([0, 3, 4, 77, 499], dtype=torch.int32, device=dev())
    got = torch.full_like(dpost, 7.0)
    dp = dpost.clone()
    ops.gelu_bwd_bf16(dp, pre, got, 0, rows=rows, n_rows=5, row_elems=C, clear_dpost=True)
    assert torch.equal(got[rows.long()], dense[rows.long()])
    keep = torch.ones(R, dtype=torch.bool, device=dev()); keep[rows.long()] = False
    assert bool((got[keep] == 7.0).all()) and torch.equal(dp[keep], dpost[keep]) and float(dp[rows.long()].abs().max()) == 0.0
    ops.zero_rows(got, rows, n_rows=5, row_bytes=C * 2)
    assert float(got[rows.long()].abs().max()) == 0.0 and bool((got[keep] == 7.0).all())


def test_gemm_conv_overlapping_rows(ops):
    """Conv1d(k=3, s=2) over a channels-last [rows][C] activation = GEMM with lda = 2C, K = 3C (implicit im2col),
    with the CONV_GELU epilogue zeroing the padded rows of every clip."""
    C, N, P_out, L_out = 64, 3, 21, 20
    P_in = 2 * P_out
    x = torch.zeros(N * P_in + 8, C, dtype=torch.bfloat16, device=dev())
    x[: N * P_in] = rnd(N * P_in, C, dtype=torch.bfloat16, seed=13)
    w = rnd(C, C, 3, scale=0.1, seed=14)                       # [o][c][k] reference layout
    wp = torch.empty(C, 3 * C, dtype=torch.bfloat16, device=dev())
    ops.conv_weight_layout(w, wp, C_out=C, C_in=C, k=3, mode=0)
    assert torch.equal(wp.float(), w.permute(0, 2, 1).reshape(C, 3 * C).to(torch.bfloat16).float())
    pre = torch.empty(N * P_out, C, dtype=torch.bfloat16, device=dev())
    post = torch.empty_like(pre)
    ops.gemm(x, wp, pre, C2=post, M=N * P_out, N=C, K=3 * C, lda=2 * C, ldb=3 * C, ldc=C, epilogue=ops.EPI_CONV_GELU,
             seg_rows=P_out, seg_valid=L_out)
    xin = x[: N * P_in].float().reshape(N, P_in, C).transpose(1, 2)           # [N][C][P_in]
    ref = F.conv1d(xin, w.to(torch.bfloat16).float(), stride=2)               # [N][C][P_in//2 - 1 ...]
    ref = ref.transpose(1, 2)[:, :L_out]
    got = pre.float().reshape(N, P_out, C)
    assert relerr(got[:, :L_out], ref) < 4e-3
    assert float(got[:, L_out:].abs().max()) == 0.0
    gp = post.float().reshape(N, P_out, C)
    assert relerr(gp[:, :L_out], F.gelu(got[:, :L_out])) < 4e-3
    assert float(gp[:, L_out:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ LayerNorm
# the last four: both grids of the backward (one pass per wave up to 16 384 row slots, four passes and a capped grid beyond) on either
# side of the switch, for the one-row-per-wave (D = 768) and the two-rows-per-wave (D = 384) forms
@pytest.mark.parametrize("M,D", [(37, 768), (64, 384), (67, 384), (10, 32), (9, 512), (5, 1024), (11, 128),
                                 (16384, 768), (16391, 768), (32768, 384), (60003, 384)])
def test_layernorm_fwd_bwd(ops, M, D):
    x = rnd(M, D, seed=20)
    r = rnd(M, D, dtype=torch.bfloat16, seed=21)
    gamma = 1 + 0.1 * rnd(D, seed=22)
    beta = 0.1 * rnd(D, seed=23)
    y = torch.empty(M, D, device=dev())
    yb = torch.empty(M, D, dtype=torch.bfloat16, device=dev())
    mean = torch.empty(M, device=dev())
    rstd = torch.empty(M, device=dev())
    ops.layernorm_fwd(x, gamma, beta, M=M, D=D, eps=1e-6, r=r, y_f32=y, y_bf16=yb, mean=mean, rstd=rstd)
    xr = x.clone().requires_grad_(True)
    rr = r.float().requires_grad_(True)
    g2 = gamma.clone().requires_grad_(True)
    b2 = beta.clone().requires_grad_(True)
    ref = F.layer_norm(xr + rr, (D,), g2, b2, 1e-6)
    assert relerr(y, ref) < 1e-5
    assert torch.equal(yb, y.to(torch.bfloat16))
    dy = rnd(M, D, seed=24)
    ref.backward(dy)
    ds = torch.empty(M, D, device=dev())
    dsb = torch.empty(M, D, dtype=torch.bfloat16, device=dev())
    dgamma = torch.zeros(D, device=dev())
    dbeta = torch.zeros(D, device=dev())
    dbias = torch.zeros(D, device=dev())
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, M=M, D=D, r=r, ds_f32=ds, ds_bf16=dsb, dgamma=dgamma, dbeta=dbeta, dbias=dbias)
    # two-stage variant (workspace partials + fold kernel) must agree with the atomic variant
    dg2, db2, dbi2 = torch.zeros(D, device=dev()), torch.zeros(D, device=dev()), torch.zeros(D, device=dev())
    wsp = torch.empty(1536 * 3 * D, device=dev())
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, M=M, D=D, r=r, ds_f32=ds, ds_bf16=dsb, dgamma=dg2, dbeta=db2, dbias=dbi2, workspace=wsp)
    assert relerr(dg2, dgamma) < 1e-5 and relerr(db2, dbeta) < 1e-5 and relerr(dbi2, dbias) < 1e-5
    assert ops.ln_bwd_partial_rows(M, D) <= 1536                     # what the workspace above is sized for
    assert relerr(ds, xr.grad) < 2e-5
    assert relerr(dgamma, g2.grad) < (2e-5 if M < 1000 else 2e-4)     # fp32 column sums over up to 60 k rows against torch's
    assert relerr(dbeta, b2.grad) < (2e-5 if M < 1000 else 2e-4)
    assert torch.equal(dsb, ds.to(torch.bfloat16))
    assert relerr(dbias, dsb.float().sum(0)) < (1e-5 if M < 1000 else 2e-4)


@pytest.mark.parametrize("M,D,wgs", [(61, 64, 4), (1000, 128, 256), (5003, 384, 256), (5003, 768, 256), (3001, 768, 16), (515, 1024, 8), (700, 512, 256)])
def test_layernorm_fwd_lean_form_on_a_capped_grid(ops, M, D, wgs):
    """wj_ln_fwd_args.workgroups: the lean (<= 48 VGPR) kernel on at most `wgs` workgroups -- the form that shares a CU with a persistent
    GEMM of another stream.  Against fp32 torch math, and bit for bit what the full-grid kernel writes (same arithmetic in the same order)."""
    x = rnd(M, D, seed=120)
    r = rnd(M, D, dtype=torch.bfloat16, seed=121)
    gamma = 1 + 0.1 * rnd(D, seed=122)
    beta = 0.1 * rnd(D, seed=123)
    outs = []
    for cap in (0, wgs):
        y = torch.full((M, D), float("nan"), device=dev())
        yb = torch.full((M, D), float("nan"), dtype=torch.bfloat16, device=dev())
        mean = torch.full((M,), float("nan"), device=dev())
        rstd = torch.full((M,), float("nan"), device=dev())
        ops.layernorm_fwd(x, gamma, beta, M=M, D=D, eps=1e-6, r=r, y_f32=y, y_bf16=yb, mean=mean, rstd=rstd, workgroups=cap)
        outs.append((y, yb, mean, rstd))
    ref = F.layer_norm(x + r.float(), (D,), gamma, beta, 1e-6)
    assert relerr(outs[1][0], ref) < 1e-5
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    # bf16 input, no residual, bf16 output only (the final norms)
    xb = rnd(M, D, dtype=torch.bfloat16, seed=124)
    y0 = torch.empty(M, D, dtype=torch.bfloat16, device=dev())
    y1 = torch.full((M, D), float("nan"), dtype=torch.bfloat16, device=dev())
    ops.layernorm_fwd(xb, gamma, beta, M=M, D=D, eps=1e-5, y_bf16=y0, x_is_bf16=True)
    ops.layernorm_fwd(xb, gamma, beta, M=M, D=D, eps=1e-5, y_bf16=y1, x_is_bf16=True, workgroups=wgs)
    assert torch.equal(y0, y1)


def test_layernorm_bf16_input_with_row_remap(ops):
    """feature_norms reads the conv tokens from the padded [N][P][C] buffer (P = T + 1)."""
    N, T, P, D = 3, 10, 11, 64
    buf = rnd(N * P, D, dtype=torch.bfloat16, seed=25)
    gamma = 1 + 0.1 * rnd(D, seed=26)
    beta = 0.1 * rnd(D, seed=27)
    yb = torch.empty(N * T, D, dtype=torch.bfloat16, device=dev())
    mean = torch.empty(N * T, device=dev())
    rstd = torch.empty(N * T, device=dev())
    ops.layernorm_fwd(buf, gamma, beta, M=N * T, D=D, eps=1e-5, y_bf16=yb, mean=mean, rstd=rstd, x_is_bf16=True, in_seg=P, in_valid=T)
    xin = buf.float().reshape(N, P, D)[:, :T].reshape(N * T, D)
    ref = F.layer_norm(xin, (D,), gamma, beta, 1e-5)
    assert relerr(yb.float(), ref) < 4e-3
    dy = rnd(N * T, D, seed=28)
    dxb = torch.zeros(N * P, D, dtype=torch.bfloat16, device=dev())
    dg = torch.zeros(D, device=dev())
    db = torch.zeros(D, device=dev())
    ops.layernorm_bwd(dy, buf, gamma, mean, rstd, M=N * T, D=D, ds_bf16=dxb, dgamma=dg, dbeta=db, x_is_bf16=True, in_seg=P,
                      in_valid=T, out_seg=P, out_valid=T)
    xr = xin.clone().requires_grad_(True)
    F.layer_norm(xr, (D,), gamma, beta, 1e-5).backward(dy)
    got = dxb.float().reshape(N, P, D)
    assert relerr(got[:, :T].reshape(N * T, D), xr.grad) < 4e-3
    assert float(got[:, T:].abs().max()) == 0.0


@pytest.mark.parametrize("dy2_is_bf16", [False, True])
@pytest.mark.parametrize("M,D", [(67, 384),     # two rows per wave, odd M: a dead second row slot
                                 (37, 768),     # one row per wave
                                 (9, 1024)])    # the widest instance, fewer rows than a workgroup
def test_layernorm_bwd_second_gradient_operand(ops, M, D, dy2_is_bf16):
    """wj_ln_bwd_args.dy2 (f32, or bf16 with dy2_is_bf16): the backward of LN(x + r) driven with dy + dy2, atomic and workspace forms.
    Bounds: those of test_layernorm_fwd_bwd for M < 1000."""
    x = rnd(M, D, seed=130)
    r = rnd(M, D, dtype=torch.bfloat16, seed=131)
    gamma = 1 + 0.1 * rnd(D, seed=132)
    beta = 0.1 * rnd(D, seed=133)
    dy = rnd(M, D, seed=134)
    dy2 = rnd(M, D, dtype=torch.bfloat16 if dy2_is_bf16 else torch.float32, seed=135)
    mean = torch.empty(M, device=dev())
    rstd = torch.empty(M, device=dev())
    ops.layernorm_fwd(x, gamma, beta, M=M, D=D, eps=1e-6, r=r, mean=mean, rstd=rstd)
    xr = x.clone().requires_grad_(True)
    g2 = gamma.clone().requires_grad_(True)
    b2 = beta.clone().requires_grad_(True)
    F.layer_norm(xr + r.float(), (D,), g2, b2, 1e-6).backward(dy + dy2.float())
    outs = []
    for with_ws in (False, True):
        ds = torch.empty(M, D, device=dev())
        dsb = torch.empty(M, D, dtype=torch.bfloat16, device=dev())
        dgamma, dbeta, dbias = (torch.zeros(D, device=dev()) for _ in range(3))
        wsp = torch.empty(ops.ln_bwd_partial_rows(M, D) * 3 * D, device=dev()) if with_ws else None
        ops.layernorm_bwd(dy, x, gamma, mean, rstd, M=M, D=D, r=r, dy2=dy2, dy2_is_bf16=dy2_is_bf16, ds_f32=ds, ds_bf16=dsb,
                          dgamma=dgamma, dbeta=dbeta, dbias=dbias, workspace=wsp)
        assert relerr(ds, xr.grad) < 2e-5
        assert relerr(dgamma, g2.grad) < 2e-5
        assert relerr(dbeta, b2.grad) < 2e-5
        assert torch.equal(dsb, ds.to(torch.bfloat16))
        assert relerr(dbias, dsb.float().sum(0)) < 1e-5
        outs.append((dgamma, dbeta, dbias))
    for atomic, folded in zip(*outs):
        assert relerr(folded, atomic) < 1e-5


def test_layernorm_channel_major_row_remap(ops):
    """in_chan / chan = S > 1: token m = (n*S + c)*T + t lives at row (c*N + n)*P + t of the channel-major padded conv buffer."""
    N, S, T, P, D = 3, 2, 10, 11, 64
    M = N * S * T
    buf = rnd(S * N * P, D, dtype=torch.bfloat16, seed=140)
    gamma = 1 + 0.1 * rnd(D, seed=141)
    beta = 0.1 * rnd(D, seed=142)
    yb = torch.empty(M, D, dtype=torch.bfloat16, device=dev())
    mean = torch.empty(M, device=dev())
    rstd = torch.empty(M, device=dev())
    ops.layernorm_fwd(buf, gamma, beta, M=M, D=D, eps=1e-5, y_bf16=yb, mean=mean, rstd=rstd, x_is_bf16=True, in_seg=P, in_valid=T, in_chan=S)
    # [c][n][p][d] -> tokens in (n, c, t) order
    xin = buf.float().reshape(S, N, P, D)[:, :, :T].permute(1, 0, 2, 3).reshape(M, D)
    ref = F.layer_norm(xin, (D,), gamma, beta, 1e-5)
    assert relerr(yb.float(), ref) < 4e-3
    dy = rnd(M, D, seed=143)
    dxb = torch.zeros(S * N * P, D, dtype=torch.bfloat16, device=dev())
    dg = torch.zeros(D, device=dev())
    db = torch.zeros(D, device=dev())
    ops.layernorm_bwd(dy, buf, gamma, mean, rstd, M=M, D=D, ds_bf16=dxb, dgamma=dg, dbeta=db, x_is_bf16=True, in_seg=P, in_valid=T,
                      out_seg=P, out_valid=T, chan=S)
    xr = xin.clone().requires_grad_(True)
    F.layer_norm(xr, (D,), gamma, beta, 1e-5).backward(dy)
    got = dxb.float().reshape(S, N, P, D)
    assert relerr(got[:, :, :T].permute(1, 0, 2, 3).reshape(M, D), xr.grad) < 4e-3
    assert float(got[:, :, T:].abs().max()) == 0.0


def test_colsum(ops):
    M, N = 1003, 192
    x = rnd(M, N, dtype=torch.bfloat16, seed=29)
    out = torch.ones(N, device=dev())
    ops.colsum_bf16(x, out, M=M, N=N, ldx=N)
    assert relerr(out, 1 + x.float().sum(0)) < 1e-5


# ------------------------------------------------------------------------------------------------------------ attention
def ref_attention(qkv, H, mask):
    B, T, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    q, k, v = qkv.view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    lse = torch.logsumexp(s, -1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B, T, D), lse


@pytest.mark.parametrize("B,T,H,hd", [(3, 200, 12, 64), (4, 200, 12, 32), (2, 49, 4, 64), (2, 24, 2, 32), (1, 224, 2, 64),
                                      (2, 400, 12, 64), (2, 400, 12, 32), (1, 416, 2, 64), (2, 225, 2, 32),
                                      (2, 129, 4, 32), (2, 150, 4, 32), (2, 192, 2, 32), (2, 193, 2, 32), (2, 150, 2, 64),
                                      # 16-wide heads (BASELINE config 1's predictor: 4 x 16): the 32-wide geometry, upper half zeros
                                      (3, 200, 4, 16), (2, 49, 4, 16), (2, 128, 2, 16), (2, 150, 4, 16), (1, 224, 6, 16)])
def test_attention_fwd_bwd(ops, B, T, H, hd):
    D = H * hd
    qkv = rnd(B, T, 3 * D, dtype=torch.bfloat16, seed=30)
    g = torch.Generator().manual_seed(31)
    mask = (torch.rand(B, T, generator=g) < 0.6)
    mask[:, 0] = False
    mask = mask.to(dev())
    mask_u8 = mask.to(torch.uint8).contiguous()
    out = torch.full((B, T, D), float("nan"), dtype=torch.bfloat16, device=dev())
    lse = torch.empty(B, H, T, device=dev())
    ops.attn_fwd(qkv, out, B=B, T=T, H=H, hd=hd, key_mask=mask_u8, lse=lse)
    x = qkv.float().requires_grad_(True)
    ref, ref_lse = ref_attention(x, H, mask)
    assert relerr(out.float(), ref) < 8e-3
    assert maxerr(lse, ref_lse) < 2e-3
    dout = rnd(B, T, D, dtype=torch.bfloat16, seed=32)
    ref.backward(dout.float())
    dqkv = torch.empty_like(qkv)
    dbias = torch.ones(3 * D, device=dev())
    ws = torch.empty(B, 3 * D, device=dev())
    ops.attn_bwd(qkv, out, dout, lse, dqkv, B=B, T=T, H=H, hd=hd, key_mask=mask_u8, dbias=dbias, dbias_ws=ws)
    got = dqkv.float()
    assert relerr(dbias, 1 + got.sum((0, 1))) < 1e-4             # fused in_proj_bias gradient = column sums of dqkv
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        assert relerr(got[..., sl], x.grad[..., sl]) < 1.5e-2, name
    # masked keys receive no gradient through k / v
    assert float(got[..., D:][mask].abs().max()) == 0.0


def test_attention_no_mask(ops):
    B, T, H, hd = 2, 200, 12, 64
    D = H * hd
    qkv = rnd(B, T, 3 * D, dtype=torch.bfloat16, seed=33)
    out = torch.empty(B, T, D, dtype=torch.bfloat16, device=dev())
    ops.attn_fwd(qkv, out, B=B, T=T, H=H, hd=hd)
    ref, _ = ref_attention(qkv.float(), H, None)
    assert relerr(out.float(), ref) < 8e-3


@pytest.mark.parametrize("B,T,H,hd", [(5, 200, 12, 64), (8, 200, 12, 32), (3, 40, 2, 32), (6, 200, 4, 16), (3, 40, 4, 16)])
def test_attention_ragged_matches_key_masked(ops, B, T, H, hd):
    """Ragged form (packed visible rows, every key attended) == the dense key-masked form on the visible rows, and both
    == plain softmax attention over each sequence's visible tokens."""
    D = H * hd
    qkv = rnd(B, T, 3 * D, dtype=torch.bfloat16, seed=34)
    g = torch.Generator().manual_seed(35)
    mask = (torch.rand(B, T, generator=g) < torch.linspace(0.3, 0.9, B)[:, None])
    mask[:, 3] = False
    mask[0] = True
    mask[0, 7] = False                                          # a one-token sequence
    mask = mask.to(dev())
    vis = ~mask
    lens = vis.sum(1)
    off = torch.zeros(B + 1, dtype=torch.int32, device=dev())
    off[1:] = torch.cumsum(lens, 0).to(torch.int32)
    n = int(off[-1])
    Tmax = int(lens.max())
    pk = qkv[vis].contiguous()                                  # [n, 3D] packed in (b, t) order
    out_r = torch.empty(n, D, dtype=torch.bfloat16, device=dev())
    lse_r = torch.empty(n, H, device=dev())
    ops.attn_fwd(pk, out_r, B=B, T=Tmax, H=H, hd=hd, seq_off=off, lse=lse_r)
    out_d = torch.empty(B, T, D, dtype=torch.bfloat16, device=dev())
    lse_d = torch.empty(B, H, T, device=dev())
    ops.attn_fwd(qkv, out_d, B=B, T=T, H=H, hd=hd, key_mask=mask.to(torch.uint8).contiguous(), lse=lse_d)
    x = qkv.float().requires_grad_(True)
    ref, ref_lse = ref_attention(x, H, mask)
    assert relerr(out_r.float(), ref[vis]) < 8e-3
    assert relerr(out_r.float(), out_d[vis].float()) < 8e-3
    assert maxerr(lse_r, ref_lse.permute(0, 2, 1)[vis]) < 2e-3
    dout = torch.zeros(B, T, D, dtype=torch.bfloat16, device=dev())
    dout[vis] = rnd(n, D, dtype=torch.bfloat16, seed=36)        # invisible query rows get no gradient (zero loss weight)
    ref.backward(dout.float())
    dq_r = torch.empty_like(pk)
    dbias = torch.zeros(3 * D, device=dev())
    ws = torch.empty(B, 3 * D, device=dev())
    ops.attn_bwd(pk, out_r, dout[vis].contiguous(), lse_r, dq_r, B=B, T=Tmax, H=H, hd=hd, seq_off=off, dbias=dbias, dbias_ws=ws)
    want = x.grad[vis]
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        assert relerr(dq_r.float()[..., sl], want[..., sl]) < 1.5e-2, name
    assert relerr(dbias, dq_r.float().sum(0)) < 1e-4
    # invisible rows of the dense formulation indeed carry no gradient: the ragged form loses nothing
    assert float(x.grad[mask][..., D:].abs().max()) == 0.0
    from wavjepa_amd._abi import WavJepaHipError
    with pytest.raises(WavJepaHipError):                        # ragged form and key mask are mutually exclusive
        ops.attn_fwd(pk, out_r, B=B, T=Tmax, H=H, hd=hd, seq_off=off, key_mask=mask.to(torch.uint8).contiguous())


def test_attention_ragged_with_empty_sequence(ops):
    """A sequence of length 0 in the packed form (no visible token) is skipped; its neighbours are unaffected."""
    H, hd = 2, 32
    D = H * hd
    lens = torch.tensor([5, 0, 17, 0, 1])
    B = int(lens.numel())
    off = torch.zeros(B + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(lens, 0).to(torch.int32)
    n = int(off[-1])
    pk = rnd(n, 3 * D, dtype=torch.bfloat16, seed=37)
    out = torch.zeros(n, D, dtype=torch.bfloat16, device=dev())
    lse = torch.zeros(n, H, device=dev())
    ops.attn_fwd(pk, out, B=B, T=int(lens.max()), H=H, hd=hd, seq_off=off.to(dev()), lse=lse)
    dout = rnd(n, D, dtype=torch.bfloat16, seed=38)
    dq = torch.zeros_like(pk)
    dbias = torch.zeros(3 * D, device=dev())
    ws = torch.zeros(B, 3 * D, device=dev())
    ops.attn_bwd(pk, out, dout, lse, dq, B=B, T=int(lens.max()), H=H, hd=hd, seq_off=off.to(dev()), dbias=dbias, dbias_ws=ws)
    x = pk.float().requires_grad_(True)
    refs = []
    for b in range(B):
        lo, hi = int(off[b]), int(off[b + 1])
        if hi > lo:
            r, _ = ref_attention(x[lo:hi][None], H, None)
            refs.append(r[0])
    ref = torch.cat(refs, 0)
    assert relerr(out.float(), ref) < 8e-3
    ref.backward(dout.float())
    assert relerr(dq.float(), x.grad) < 1.5e-2
    assert relerr(dbias, dq.float().sum(0)) < 1e-4
    assert bool(torch.isfinite(dq.float()).all()) and float(ws[1].abs().max()) == 0.0 and float(ws[3].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ MX fp8
def _dequant(q, scales, M, K, ld_scale):
    """e4m3 bytes [M][K] + block scales [K/128][ld_scale] dwords -> fp32 [M][K]."""
    x = q.view(torch.float8_e4m3fn).float()
    sc = scales[:(K // 128) * ld_scale].view(K // 128, ld_scale)[:, :M]                       # [kt][row] dwords (int32)
    b = torch.stack([(sc >> (8 * j)) & 0xFF for j in range(4)], dim=-1)                          # [kt][row][4]
    e = b.permute(1, 0, 2).reshape(M, K // 32).float() - 127.0                                   # [row][block]
    return x * torch.exp2(e).repeat_interleave(32, dim=1)


@pytest.mark.parametrize("M,K", [(300, 256), (1000, 768), (64, 3072)])
def test_quantize_mxfp8(ops, M, K):
    """Block scale = ceil(log2(amax / 448)) per 32 consecutive elements, elements RNE to e4m3: checked against the same rule in
    torch (bit-exact bytes and scales), and the relative error of the round trip (<= 2^-4 per element, ~3 % rms)."""
    x = (rnd(M, K, seed=90) * torch.exp2(torch.randint(-6, 6, (M, K // 32), generator=torch.Generator().manual_seed(1)).float())
         .repeat_interleave(32, dim=1).to(dev())).to(torch.bfloat16)
    x[3, 64:96] = 0                                                                               # an all-zero block
    q = torch.full((M, K), 0x7F, dtype=torch.uint8, device=dev())
    sc = torch.zeros(ops.fp8_scale_dwords(M + 5, K), dtype=torch.int32, device=dev())
    ops.quantize_mxfp8(x, q, sc, M=M, K=K, ldx=K, ldq=K, ld_scale=M + 5)
    xf = x.float().view(M, K // 32, 32)
    amax = xf.abs().amax(-1)
    s = torch.where(amax > 0, torch.ceil(torch.log2(amax / 448.0)), torch.zeros_like(amax))
    want_q = (xf * torch.exp2(-s)[..., None]).reshape(M, K).to(torch.float8_e4m3fn).view(torch.uint8)
    got_s = _dequant(torch.full_like(q, 0x38), sc, M, K, M + 5)                                   # 0x38 = 1.0: the scale alone
    assert torch.equal(got_s.view(M, K // 32, 32)[..., 0], torch.exp2(s))
    assert torch.equal(q, want_q)
    back = _dequant(q, sc, M, K, M + 5)
    assert float((back - x.float()).abs().max() / x.float().abs().max()) < 0.07 and relerr(back, x.float()) < 4e-2


@pytest.mark.parametrize("M,N,K,epi", [(300, 256, 256, "bf16"), (1000, 768, 768, "bf16"), (513, 3072, 768, "gelu2"), (700, 384, 1536, "gelu"),
                                       (4100, 2304, 768, "bf16")])
def test_gemm_mxfp8(ops, M, N, K, epi):
    """MX fp8 GEMM against fp32 torch math on the DEQUANTISED operands (the kernel's own inputs: errors are fp32 summation order +
    the bf16 output rounding), and against the unquantised product (the format's error, ~4 % per operand element averaging down
    over K)."""
    x = rnd(M, K, dtype=torch.bfloat16, seed=91)
    w = rnd(N, K, dtype=torch.bfloat16, scale=0.05, seed=92)
    bias = rnd(N, seed=93)
    qx, qw = torch.empty(M, K, dtype=torch.uint8, device=dev()), torch.empty(N, K, dtype=torch.uint8, device=dev())
    sx = torch.zeros(ops.fp8_scale_dwords(M, K), dtype=torch.int32, device=dev())
    sw = torch.zeros(ops.fp8_scale_dwords(N, K), dtype=torch.int32, device=dev())
    ops.quantize_mxfp8(x, qx, sx, M=M, K=K, ldx=K, ldq=K, ld_scale=M)
    ops.quantize_mxfp8(w, qw, sw, M=N, K=K, ldx=K, ldq=K, ld_scale=N)
    C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
    C2 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
    e = {"bf16": ops.EPI_BF16, "gelu2": ops.EPI_BIAS_GELU2, "gelu": ops.EPI_BIAS_GELU}[epi]
    ops.gemm_mxfp8(qx, qw, sx, sw, C, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ld_scale_a=M, ld_scale_b=N, epilogue=e, bias=bias,
                   C2=C2 if epi == "gelu2" else None)
    h = (_dequant(qx, sx, M, K, M) @ _dequant(qw, sw, N, K, N).t() + bias).to(torch.bfloat16).float()
    exact = x.float() @ w.float().t() + bias
    if epi == "bf16":
        assert relerr(C.float(), h) < 3e-3
        assert relerr(C.float(), exact) < 5e-2
    elif epi == "gelu":
        assert relerr(C.float(), F.gelu(h)) < 4e-3
    else:
        hp = h.clone().requires_grad_(True)
        F.gelu(hp).sum().backward()
        assert relerr(C2.float(), F.gelu(h)) < 4e-3 and relerr(C.float(), hp.grad) < 4e-3


def test_fp8_outputs_fused_into_layernorm_and_gelu_epilogue(ops):
    """Config 5 producers: LayerNorm and the linear1 GELU epilogue emit their output directly in the MX fp8 operand format; both
    must be BIT-identical to wj_quantize_mxfp8 applied to the bf16 output they also write (bytes and block scales)."""
    M, D = 333, 768
    x, r = rnd(M, D, seed=95) * 3 + 0.5, rnd(M, D, dtype=torch.bfloat16, seed=96)
    g, b = 1 + 0.1 * rnd(D, seed=97), 0.1 * rnd(D, seed=98)
    yb = torch.empty(M, D, dtype=torch.bfloat16, device=dev())
    q = torch.zeros(M, D, dtype=torch.uint8, device=dev())
    sc = torch.zeros(ops.fp8_scale_dwords(M, D), dtype=torch.int32, device=dev())
    ops.layernorm_fwd(x, g, b, M=M, D=D, eps=1e-6, r=r, y_bf16=yb, y_fp8=q, y_fp8_scales=sc, ld_fp8_scale=M)
    q2, sc2 = torch.zeros_like(q), torch.zeros_like(sc)
    ops.quantize_mxfp8(yb, q2, sc2, M=M, K=D, ldx=D, ldq=D, ld_scale=M)
    assert torch.equal(q, q2) and torch.equal(sc[:(D // 128) * M], sc2[:(D // 128) * M])
    # GELU epilogue of the MX fp8 GEMM (teacher form: fp8 only; training form: bf16 gelu + gelu' + fp8)
    M, N, K = 700, 1024, 768
    a, w, bias = rnd(M, K, dtype=torch.bfloat16, seed=99), rnd(N, K, dtype=torch.bfloat16, scale=0.05, seed=100), rnd(N, seed=101)
    qa, qw = torch.empty(M, K, dtype=torch.uint8, device=dev()), torch.empty(N, K, dtype=torch.uint8, device=dev())
    sa = torch.zeros(ops.fp8_scale_dwords(M, K), dtype=torch.int32, device=dev())
    sw = torch.zeros(ops.fp8_scale_dwords(N, K), dtype=torch.int32, device=dev())
    ops.quantize_mxfp8(a, qa, sa, M=M, K=K, ldx=K, ldq=K, ld_scale=M)
    ops.quantize_mxfp8(w, qw, sw, M=N, K=K, ldx=K, ldq=K, ld_scale=N)
    kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ld_scale_a=M, ld_scale_b=N, bias=bias)
    gl, gp = torch.empty(M, N, dtype=torch.bfloat16, device=dev()), torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    qg = torch.zeros(M, N, dtype=torch.uint8, device=dev())
    sg = torch.zeros(ops.fp8_scale_dwords(M, N), dtype=torch.int32, device=dev())
    ops.gemm_mxfp8(qa, qw, sa, sw, gp, C2=gl, epilogue=ops.EPI_BIAS_GELU2, q_out=qg, q_scales=sg, ld_q_scale=M, **kw)
    qr, sr = torch.zeros_like(qg), torch.zeros_like(sg)
    ops.quantize_mxfp8(gl, qr, sr, M=M, K=N, ldx=N, ldq=N, ld_scale=M)
    assert torch.equal(qg, qr) and torch.equal(sg[:(N // 128) * M], sr[:(N // 128) * M])
    gl2, gp2 = torch.empty_like(gl), torch.empty_like(gp)
    ops.gemm_mxfp8(qa, qw, sa, sw, gp2, C2=gl2, epilogue=ops.EPI_BIAS_GELU2, **kw)
    assert torch.equal(gl, gl2) and torch.equal(gp, gp2)                       # the bf16 outputs do not change
    qt, st = torch.zeros_like(qg), torch.zeros_like(sg)
    ops.gemm_mxfp8(qa, qw, sa, sw, None, epilogue=ops.EPI_BIAS_GELU, q_out=qt, q_scales=st, ld_q_scale=M, **kw)      # no bf16 output at all
    assert torch.equal(qt, qg) and torch.equal(st[:(N // 128) * M], sg[:(N // 128) * M])


# ------------------------------------------------------------------------------------------------------------ conv0
def test_conv0_statistics_of_high_pass_filters_on_a_smooth_signal(ops):
    """The GroupNorm statistics of conv layer 0 are formed from the clip's patch Gram matrix (w^T X2 w, csrc/conv0.hip).  A difference
    filter on a smooth signal makes that a difference of terms 1e4-1e6 times its size: the Gram path runs in double precision, and its
    mean / rstd must still match the statistics of the reference's bf16-rounded conv output (torch, fp64 sums) -- as must the
    activations that are normalised with them."""
    N, C_in, L, C, k, s = 2, 1, 32159, 64, 10, 5
    L_out = (L - k) // s + 1
    P = L_out + 2
    t = torch.arange(L, dtype=torch.float64)
    sig = torch.stack([torch.sin(2 * math.pi * t / 900.0) + 0.5 * torch.sin(2 * math.pi * t / 210.0 + 1.0),
                       torch.cos(2 * math.pi * t / 1500.0) * (1 + 0.3 * torch.sin(2 * math.pi * t / 5000.0))])
    sig = sig + 1e-3 * torch.randn(N, L, generator=torch.Generator().manual_seed(70), dtype=torch.float64)
    sig = (sig - sig.mean(-1, keepdim=True)) / sig.std(-1, keepdim=True)             # per-crop normalisation, as the data path does
    audio = sig.to(torch.float32).to(torch.bfloat16).view(N, C_in, L).to(dev())
    w = rnd(C, C_in, k, scale=math.sqrt(2.0 / k), seed=71)
    w[0] = 0; w[0, 0, 4] = 1.0; w[0, 0, 5] = -1.0                                   # first difference
    w[1] = 0; w[1, 0, 3] = 1.0; w[1, 0, 4] = -2.0; w[1, 0, 5] = 1.0                 # second difference
    w[2] = 0; w[2, 0, :4] = torch.tensor([1.0, -3.0, 3.0, -1.0], device=dev())      # third difference
    wb = w.to(torch.bfloat16)
    gamma, beta = torch.ones(C, device=dev()), torch.zeros(C, device=dev())
    act = torch.empty(N, P, C, dtype=torch.bfloat16, device=dev())
    stats = torch.empty(2, N, C, device=dev())
    dims = dict(N=N, C_in=C_in, C=C, k=k, L_out=L_out)
    ws = torch.full((ops.workspace_bytes("wj_conv0_gn_gelu_fwd", **dims) // 4,), float("nan"), device=dev())
    yx = torch.empty(N, C, C_in * k, device=dev())
    x1 = torch.empty(N, C_in * k, device=dev())
    ops.conv0_fwd(audio, wb, gamma, beta, act, stats[0], stats[1], ws, N=N, C_in=C_in, L=L, C=C, k=k, stride=s, L_out=L_out, P=P, yx=yx, x1=x1)
    y = F.conv1d(audio.float(), wb.float(), stride=s).to(torch.bfloat16).double()  # what the reference's GroupNorm sees
    mean_ref = y.mean(-1)
    rstd_ref = (y.var(-1, unbiased=False) + 1e-5).rsqrt()
    ystd = y.std(-1)
    # the difference filters' outputs are 1e-2 .. 1e-4 of the signal: that is where an fp32 Gram would lose the variance
    assert float(ystd[:, :3].max()) < 0.1                # (the bf16 signal's own rounding noise included)
    assert float(((stats[0].double() - mean_ref).abs() / ystd).max()) < 2e-3
    assert float(((stats[1].double() - rstd_ref).abs() / rstd_ref).max()) < 2e-3
    ref = F.gelu(F.group_norm(y.float(), C, gamma, beta, 1e-5)).transpose(1, 2)
    assert relerr(act.float()[:, :L_out], ref) < 5e-3
    for c in range(3):                                                              # the small-output channels on their own
        assert relerr(act.float()[:, :L_out, c], ref[..., c]) < 8e-3, c


def test_conv0_reference_rounding_point_statistics_path(tmp_path):
    """WJ_CONV0_STATS=mfma (read once per process: a child process): the GroupNorm statistics from a pass over the bf16-ROUNDED conv output,
    i.e. at the reference's own rounding point (extractors/audio_feature_extractor.py:90-96 under autocast) -- kept alive beside the default
    patch-Gram form, and held much closer to the rounded tensor's statistics than the Gram form's averaged-rounding-noise distance."""
    import subprocess
    import sys
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import math, sys, torch
        import torch.nn.functional as F
        sys.path.insert(0, %r)
        from wavjepa_amd import ops
        dev = torch.device("cuda:0")
        g = torch.Generator(device=dev).manual_seed(5)
        N, C_in, L, C, k, s = 2, 1, 32159, 512, 10, 5
        L_out = (L - k) // s + 1
        P = L_out + 2
        audio = torch.randn(N, C_in, L, device=dev, generator=g).to(torch.bfloat16)
        wb = (torch.randn(C, C_in, k, device=dev, generator=g) * math.sqrt(2.0 / (C_in * k))).to(torch.bfloat16)
        gamma = 1 + 0.1 * torch.randn(C, device=dev, generator=g)
        beta = 0.1 * torch.randn(C, device=dev, generator=g)
        act = torch.empty(N, P, C, dtype=torch.bfloat16, device=dev)
        stats = torch.empty(2, N, C, device=dev)
        ws = torch.empty(ops.workspace_bytes("wj_conv0_gn_gelu_fwd", N=N, C_in=C_in, C=C, k=k, L_out=L_out) // 4, device=dev)
        ops.conv0_fwd(audio, wb, gamma, beta, act, stats[0], stats[1], ws, N=N, C_in=C_in, L=L, C=C, k=k, stride=s, L_out=L_out, P=P)
        y = F.conv1d(audio.float(), wb.float(), stride=s).to(torch.bfloat16).float()        # the tensor the reference's GroupNorm sees
        mean_err = float((stats[0] - y.mean(-1)).abs().max() / y.std())
        rstd_ref = (y.var(-1, unbiased=False) + 1e-5).rsqrt()
        rstd_err = float(((stats[1] - rstd_ref) / rstd_ref).abs().max())
        z = F.gelu(F.group_norm(y, C, gamma, beta, 1e-5)).transpose(1, 2)
        act_err = float((act.float()[:, :L_out] - z).norm() / z.norm())
        print("RESULT", mean_err, rstd_err, act_err)
    """ % root)
    out = {}
    for mode in ("mfma", "gram"):
        env = dict(os.environ, WJ_CONV0_STATS=mode)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out[mode] = [float(v) for v in [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1].split()[1:]]
    print("conv0 statistics (mean err / sigma, rstd rel err, activation rel err):", out)
    assert out["mfma"][0] < 2e-6 and out["mfma"][1] < 5e-6, out          # sums of the rounded values themselves, fp32 accumulation
    # the default: the unrounded conv output's sums (PARITY.md).  Measured on this draw: mean 9.0e-5 sigma, rstd 1.25e-4 (the maximum over
    # the 2 x 512 channels; the rounding-point form above: 8.6e-7 / 8.7e-7)
    assert out["gram"][0] < 3e-4 and out["gram"][1] < 3e-4, out
    assert out["mfma"][2] < 5e-3 and out["gram"][2] < 5e-3


@pytest.mark.parametrize("N,C_in,L,C", [(2, 1, 32159, 512), (3, 1, 4000, 32), (2, 2, 4000, 64), (2, 2, 4100, 128), (3, 1, 2571, 256)])
def test_conv0_fwd_bwd(ops, N, C_in, L, C):
    k, s = 10, 5
    L_out = (L - k) // s + 1
    P = L_out + 2
    audio = rnd(N, C_in, L, dtype=torch.bfloat16, seed=40)
    w = rnd(C, C_in, k, scale=math.sqrt(2.0 / (C_in * k)), seed=41)
    wb = w.to(torch.bfloat16)
    gamma = 1 + 0.1 * rnd(C, seed=42)
    beta = 0.1 * rnd(C, seed=43)
    act = torch.empty(N, P, C, dtype=torch.bfloat16, device=dev())
    stats = torch.empty(2, N, C, device=dev())
    dims = dict(N=N, C_in=C_in, C=C, k=k, L_out=L_out)
    ws = torch.full((ops.workspace_bytes("wj_conv0_gn_gelu_fwd", **dims) // 4,), float("nan"), device=dev())   # scratch needs no zeroing
    yx = torch.empty(N, C, C_in * k, device=dev())
    x1 = torch.empty(N, C_in * k, device=dev())
    ops.conv0_fwd(audio, wb, gamma, beta, act, stats[0], stats[1], ws, N=N, C_in=C_in, L=L, C=C, k=k, stride=s, L_out=L_out, P=P,
                  yx=yx, x1=x1)
    # no float atomics in the statistics: a second run reproduces every bit (activations, statistics, the sums kept for the backward)
    act_b, stats_b, yx_b, x1_b = torch.empty_like(act), torch.empty_like(stats), torch.empty_like(yx), torch.empty_like(x1)
    ops.conv0_fwd(audio, wb, gamma, beta, act_b, stats_b[0], stats_b[1], torch.full_like(ws, 7.0), N=N, C_in=C_in, L=L, C=C, k=k, stride=s,
                  L_out=L_out, P=P, yx=yx_b, x1=x1_b)
    assert torch.equal(act, act_b) and torch.equal(stats, stats_b) and torch.equal(yx, yx_b) and torch.equal(x1, x1_b)
    wr = wb.float().requires_grad_(True)
    gr = gamma.clone().requires_grad_(True)
    br = beta.clone().requires_grad_(True)
    y = F.conv1d(audio.float(), wr, stride=s).to(torch.bfloat16).float()
    y_ste = F.conv1d(audio.float(), wr, stride=s)
    y = y_ste + (y - y_ste).detach()                      # value of the bf16-rounded conv, gradient of the exact one
    z = F.gelu(F.group_norm(y, C, gr, br, 1e-5))
    ref = z.transpose(1, 2)
    got = act.float()
    assert relerr(got[:, :L_out], ref) < 5e-3
    assert float(got[:, L_out:].abs().max()) == 0.0
    # the statistics come from the clip's patch Gram matrix (sums of the UNROUNDED conv output, in double precision: csrc/conv0.hip); the
    # reference's GroupNorm sees the bf16-rounded tensor.  The difference is the averaged rounding noise of L_out values (per value: up
    # to half a bf16 step, rms ~1.8e-3 |y|): ~2e-5 of the channel's standard deviation at 6430 time steps, the largest of the N C means a
    # few times that; rstd a few 1e-5 relative
    noise = 1.8e-3 * float(y.detach().std()) / math.sqrt(L_out)
    assert maxerr(stats[0], y.mean(-1)) < 8 * noise, (maxerr(stats[0], y.mean(-1)), noise)
    rstd_ref = (y.detach().var(-1, unbiased=False) + 1e-5).rsqrt()
    assert relerr(stats[1], rstd_ref) < (6e-5 if L_out > 4000 else 3e-4), relerr(stats[1], rstd_ref)
    dact = torch.zeros(N, P, C, dtype=torch.bfloat16, device=dev())
    dact[:, :L_out] = rnd(N, L_out, C, dtype=torch.bfloat16, seed=44)
    ref.backward(dact[:, :L_out].float())
    dw = torch.zeros(C, C_in, k, device=dev())
    dg = torch.zeros(C, device=dev())
    db = torch.zeros(C, device=dev())
    ws2 = torch.full((ops.workspace_bytes("wj_conv0_gn_gelu_bwd", max_rows=0, **dims) // 4,), float("nan"), device=dev())
    ops.conv0_bwd(audio, wb, gamma, beta, stats[0], stats[1], dact, dw, dg, db, ws2, yx=yx, x1=x1, N=N, C_in=C_in, L=L, C=C, k=k,
                  stride=s, L_out=L_out, P=P)
    assert relerr(dg, gr.grad) < 5e-3
    assert relerr(db, br.grad) < 5e-3
    assert relerr(dw, wr.grad) < 1e-2
    # forward sums kept for the backward: patches x_{t,q} = audio[ci][s t + kk], q = ci*k + kk
    patches = audio.float().unfold(2, k, s).permute(0, 2, 1, 3).reshape(N, L_out, C_in * k)
    assert relerr(x1, patches.sum(1)) < 1e-4 or maxerr(x1, patches.sum(1)) < 1e-2
    assert relerr(yx, torch.einsum("nct,ntq->ncq", y.detach(), patches)) < 1e-3
    # listed-rows form: the output gradient is zero outside a few runs of rows (the student's context) and only those
    # rows are read -- GroupNorm still spreads the gradient over the whole time axis through the forward sums
    g = torch.Generator().manual_seed(45)
    live = torch.zeros(N, L_out, dtype=torch.bool)
    for n in range(N):
        for st in torch.randint(0, L_out - 40, (5,), generator=g).tolist():
            live[n, st:st + 37] = True
    live[N - 1] = False
    live[N - 1, 5] = True                                          # a clip with a single live row
    dact2 = torch.zeros_like(dact)
    dact2[:, :L_out][live.to(dev())] = dact[:, :L_out][live.to(dev())]
    rows = torch.nonzero(torch.cat([live, torch.zeros(N, P - L_out, dtype=torch.bool)], 1).reshape(-1)).squeeze(1).to(torch.int32)
    off = torch.zeros(N + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(live.sum(1), 0).to(torch.int32)
    for t in (wr, gr, br):
        t.grad = None
    y = F.conv1d(audio.float(), wr, stride=s).to(torch.bfloat16).float()
    y_ste = F.conv1d(audio.float(), wr, stride=s)
    F.gelu(F.group_norm(y_ste + (y - y_ste).detach(), C, gr, br, 1e-5)).transpose(1, 2).backward(dact2[:, :L_out].float())
    dw2, dg2, db2 = torch.zeros_like(dw), torch.zeros_like(dg), torch.zeros_like(db)
    poison = dact2.clone()
    poison[:, :L_out][~live.to(dev())] = 1e4                       # rows outside the list must never be read
    ops.conv0_bwd(audio, wb, gamma, beta, stats[0], stats[1], poison, dw2, dg2, db2, ws2, yx=yx, x1=x1, N=N, C_in=C_in, L=L, C=C,
                  k=k, stride=s, L_out=L_out, P=P, rows=rows.to(dev()), row_off=off.to(dev()), max_rows=int(live.sum(1).max()))
    assert relerr(dg2, gr.grad) < 5e-3 and relerr(db2, br.grad) < 5e-3
    assert relerr(dw2, wr.grad) < 1e-2
    dw3, dg3, db3 = torch.zeros_like(dw), torch.zeros_like(dg), torch.zeros_like(db)       # bit-reproducible as well
    ops.conv0_bwd(audio, wb, gamma, beta, stats[0], stats[1], poison, dw3, dg3, db3, torch.full_like(ws2, 3.0), yx=yx, x1=x1, N=N, C_in=C_in,
                  L=L, C=C, k=k, stride=s, L_out=L_out, P=P, rows=rows.to(dev()), row_off=off.to(dev()), max_rows=int(live.sum(1).max()))
    assert torch.equal(dw2, dw3) and torch.equal(dg2, dg3) and torch.equal(db2, db3)


def test_gelu_bwd_and_conv_weight_layouts(ops):
    n = 8 * 1000
    d = rnd(n, dtype=torch.bfloat16, seed=50)
    p = rnd(n, dtype=torch.bfloat16, seed=51)
    o = torch.empty_like(d)
    ops.gelu_bwd_bf16(d, p, o, n)
    pr = p.float().requires_grad_(True)
    F.gelu(pr).backward(d.float())
    assert relerr(o.float(), pr.grad) < 4e-3
    Co, Ci, k, s = 16, 8, 3, 2
    w = rnd(Co, Ci, k, seed=52)
    for rho, U in ((0, 2), (1, 1)):
        wd = torch.empty(U * Co, Ci, dtype=torch.bfloat16, device=dev())
        ops.conv_weight_layout(w, wd, C_out=Co, C_in=Ci, k=k, mode=1, stride=s, rho=rho, U=U)
        ref = torch.cat([w[:, :, rho + s * (U - 1 - v)] for v in range(U)], 0)
        assert torch.equal(wd.float(), ref.to(torch.bfloat16).float())
    dwp = rnd(Co, k * Ci, seed=53)
    dw = torch.ones(Co, Ci, k, device=dev())
    ops.conv_weight_layout(dwp, dw, C_out=Co, C_in=Ci, k=k, mode=2)
    assert torch.equal(dw, 1 + dwp.reshape(Co, k, Ci).permute(0, 2, 1))


# ------------------------------------------------------------------------------------------------------------ tokens
def test_token_plumbing(ops):
    B, T, D, G = 3, 20, 64, 4
    x = rnd(B * T, D, dtype=torch.bfloat16, seed=60)
    pos = rnd(T, D, seed=61)
    y = torch.empty(B * T, D, device=dev())
    yb = torch.empty(B * T, D, dtype=torch.bfloat16, device=dev())
    ops.add_pos(x, pos, M=B * T, T=T, D=D, y_f32=y, y_bf16=yb)
    ref = x.float().reshape(B, T, D) + pos
    assert torch.equal(y.reshape(B, T, D), ref) and torch.equal(yb, y.to(torch.bfloat16))

    g = torch.Generator().manual_seed(62)
    ctx_mask = (torch.rand(B, T, generator=g) < 0.7).to(dev())
    keep = torch.nonzero(~ctx_mask.reshape(-1)).squeeze(1).to(torch.int32)
    n = int(keep.numel())
    enc = rnd(B * T, D, seed=63)
    out = torch.empty(n, D, device=dev())
    ops.mask_gather_rows(enc, keep, out, n_rows=n, D=D, elem_bytes=4)
    assert torch.equal(out, enc.reshape(B, T, D)[~ctx_mask])                 # bit-exact copy

    inv = torch.full((B * T,), -1, dtype=torch.int32, device=dev())
    inv[keep.long()] = torch.arange(n, dtype=torch.int32, device=dev())
    feats = rnd(n, D, dtype=torch.bfloat16, seed=64)
    mtok = 0.02 * rnd(D, seed=65)
    o32 = torch.empty(B * G, T, D, device=dev())
    o16 = torch.empty(B * G, T, D, dtype=torch.bfloat16, device=dev())
    ops.mask_scatter_fill_pos(feats, inv, mtok, pos, B=B, T=T, D=D, G=G, out_f32=o32, out_bf16=o16)
    tgt = mtok.to(torch.bfloat16).expand(B, T, D).clone()
    tgt[~ctx_mask] = feats
    ref = (tgt.float() + pos)[:, None].expand(B, G, T, D).reshape(B * G, T, D)
    assert torch.equal(o32, ref) and torch.equal(o16, ref.to(torch.bfloat16))

    d_in = rnd(B * G, T, D, seed=66)
    dfe = torch.zeros(n, D, dtype=torch.bfloat16, device=dev())
    dmt = torch.zeros(D, device=dev())
    ops.mask_scatter_fill_pos_bwd(d_in, inv, dfe, dmt, B=B, T=T, D=D, G=G)
    dsum = d_in.reshape(B, G, T, D).sum(1)
    assert relerr(dfe.float(), dsum[~ctx_mask]) < 4e-3
    assert relerr(dmt, dsum[ctx_mask].sum(0)) < 1e-5
    # the mask-token gradient as partial rows (no atomics) + a column-sum fold: the same bf16 rows, the same sums, bit-identical reruns
    nrows = ops.scatter_fill_bwd_partial_rows(B, T)
    assert ops.workspace_bytes("wj_mask_scatter_fill_pos_bwd", B=B, T=T, D=D, G=G) == nrows * D * 4
    outs = []
    for _ in range(2):
        part = torch.full((nrows, D), float("nan"), device=dev())
        dfe2 = torch.zeros(n, D, dtype=torch.bfloat16, device=dev())
        dmt2 = torch.zeros(D, device=dev())
        ops.mask_scatter_fill_pos_bwd(d_in, inv, dfe2, dmt2, B=B, T=T, D=D, G=G, partials=part)
        assert float(dmt2.abs().max()) == 0.0 and torch.equal(dfe2, dfe)
        ops.colsum_f32_group([(part, D, nrows, D, dmt2, None, None, D)])
        outs.append(dmt2)
    assert relerr(outs[0], dsum[ctx_mask].sum(0)) < 1e-5 and torch.equal(outs[0], outs[1])

    back = torch.empty(B * T, D, device=dev())
    ops.unmask_rows_f32(feats, inv, back, M=B * T, D=D)
    ref = torch.zeros(B, T, D, device=dev())
    ref[~ctx_mask] = feats.float()
    assert torch.equal(back.reshape(B, T, D), ref)
    # dtype variants + identity
    f32src = rnd(n, D, seed=67)
    back16 = torch.empty(B * T, D, dtype=torch.bfloat16, device=dev())
    ops.unmask_rows_f32(f32src, inv, back16, M=B * T, D=D, src_is_f32=True, dst_is_bf16=True)
    ref = torch.zeros(B, T, D, device=dev())
    ref[~ctx_mask] = f32src
    assert torch.equal(back16.reshape(B, T, D), ref.to(torch.bfloat16))
    wide = torch.empty(n, D, device=dev())
    ops.unmask_rows_f32(feats, None, wide, M=n, D=D)
    assert torch.equal(wide, feats.float())

    # ragged predictor input / its backward: only the visible rows of every (clip, group), packed
    tmask = (torch.rand(B, G, T, generator=g) < 0.3).to(dev()) & ctx_mask[:, None]
    vis = (~ctx_mask)[:, None] | tmask                                      # context or this group's targets
    rows = torch.nonzero(vis.reshape(-1)).squeeze(1).to(torch.int32)
    nd = int(rows.numel())
    r32 = torch.empty(nd, D, device=dev())
    r16 = torch.empty(nd, D, dtype=torch.bfloat16, device=dev())
    ops.mask_scatter_fill_pos(feats, inv, mtok, pos, B=B, T=T, D=D, G=G, out_f32=r32, out_bf16=r16, rows=rows, n_rows=nd)
    assert torch.equal(r32, o32.reshape(-1, D)[rows.long()]) and torch.equal(r16, o16.reshape(-1, D)[rows.long()])
    rowmap = torch.full((B * G * T,), -1, dtype=torch.int32, device=dev())
    rowmap[rows.long()] = torch.arange(nd, dtype=torch.int32, device=dev())
    d_pk = rnd(nd, D, seed=68)
    d_dense = torch.zeros(B * G * T, D, device=dev())
    d_dense[rows.long()] = d_pk
    dfe2 = torch.zeros(n, D, dtype=torch.bfloat16, device=dev())
    dmt2 = torch.zeros(D, device=dev())
    ops.mask_scatter_fill_pos_bwd(d_pk, inv, dfe2, dmt2, B=B, T=T, D=D, G=G, rowmap=rowmap)
    dsum = d_dense.reshape(B, G, T, D).sum(1)
    assert relerr(dfe2.float(), dsum[~ctx_mask]) < 4e-3
    assert relerr(dmt2, dsum[ctx_mask].sum(0)) < 1e-5


# ------------------------------------------------------------------------------------------------------------ targets / loss
def test_instnorm_and_mse(ops):
    B, T, D, G, K = 3, 200, 768, 4, 3
    layers = [rnd(B, T, D, seed=70 + i) * (1 + i) + i for i in range(K)]
    tg = torch.empty(B, T, D, device=dev())
    for i, x in enumerate(layers):
        ops.instnorm_accumulate(x, tg, B=B, TD=T * D, accumulate=i > 0, scale=1.0 / K)
    ref = torch.stack([F.instance_norm(x.transpose(1, 2)[None])[0].transpose(1, 2) for x in layers]).mean(0)
    assert relerr(tg, ref) < 1e-5
    # one-pass form: the layer outputs come out of LayerNorm together with their per-sample (sum, sum of squares)
    g = 1 + 0.1 * rnd(D, seed=77)
    b = 0.1 * rnd(D, seed=78)
    stats = torch.full((K, B, ops.GROUP_STATS_SPLIT, 2), float("nan"), device=dev())   # written, not accumulated: no zeroing
    outs = []
    for i, x in enumerate(layers):
        y = torch.empty(B * T, D, device=dev())
        ops.layernorm_fwd(x.reshape(B * T, D), g, b, M=B * T, D=D, eps=1e-6, y_f32=y, group_stats=stats[i], group_rows=T)
        outs.append(y)
        yr = F.layer_norm(x, (D,), g, b, 1e-6)
        got = stats[i].sum(1)
        assert relerr(got[:, 0], yr.sum((1, 2))) < 1e-4 or maxerr(got[:, 0], yr.sum((1, 2))) < 0.5
        assert relerr(got[:, 1], (yr * yr).sum((1, 2))) < 1e-5
        again = torch.empty_like(stats[i])
        ops.layernorm_fwd(x.reshape(B * T, D), g, b, M=B * T, D=D, eps=1e-6, y_f32=y, group_stats=again, group_rows=T)
        assert torch.equal(again, stats[i])                                             # bit-reproducible
    tg2 = torch.empty(B, T, D, device=dev())
    ops.instnorm_mean(outs, stats, tg2, B=B, TD=T * D)
    ref2 = torch.stack([F.instance_norm(F.layer_norm(x, (D,), g, b, 1e-6).transpose(1, 2)[None])[0].transpose(1, 2) for x in layers]).mean(0)
    assert relerr(tg2, ref2) < 2e-5

    preds = rnd(B * G, T, D, dtype=torch.bfloat16, seed=75)
    g = torch.Generator().manual_seed(76)
    tmask = (torch.rand(B, G, T, generator=g) < 0.25).to(dev())
    loss = torch.zeros(2, device=dev())
    ws = torch.empty(2 + B * G * T, device=dev())
    dp = torch.empty_like(preds)
    ops.masked_mse(preds, tg, tmask.to(torch.uint8), loss, ws, B=B, G=G, T=T, D=D, dpreds=dp, gscale=1.0)
    pr = preds.float().requires_grad_(True)
    err = ((pr.view(B, G, T, D) - tg[:, None]) ** 2).mean(-1) * tmask
    ref_loss = err.sum() / (tmask.sum() + 1e-8)
    ref_loss.backward()
    assert abs(float(loss[0]) - float(ref_loss)) < 1e-5 * float(ref_loss)
    assert float(loss[1]) == float(tmask.sum())
    assert relerr(dp.float(), pr.grad) < 4e-3
    # ragged form: preds hold only listed rows (targets + some extra non-target rows)
    seen = tmask | (torch.rand(B, G, T, generator=g) < 0.2).to(dev())
    rows = torch.nonzero(seen.reshape(-1)).squeeze(1).to(torch.int32)
    nd = int(rows.numel())
    pk = preds.reshape(-1, D)[rows.long()].contiguous()
    loss2 = torch.zeros(2, device=dev())
    dp2 = torch.empty_like(pk)
    ops.masked_mse(pk, tg, tmask.to(torch.uint8), loss2, ws, B=B, G=G, T=T, D=D, dpreds=dp2, gscale=1.0, rows=rows, n_rows=nd)
    assert abs(float(loss2[0]) - float(loss[0])) < 1e-6 * float(loss[0]) and float(loss2[1]) == float(loss[1])
    assert torch.equal(dp2, dp.reshape(-1, D)[rows.long()])


# ------------------------------------------------------------------------------------------------------------ optimiser side
def test_ema_adamw_sumsq_cast(ops):
    n = 4 * 100003
    s = rnd(n, seed=80)
    t = rnd(n, seed=81)
    tb = torch.empty(n, dtype=torch.bfloat16, device=dev())
    ref_t = t * 0.999 + (1 - 0.999) * s
    ops.ema_update(s, t, n, 0.999, teacher_bf16=tb)
    assert relerr(t, ref_t) < 1e-6 and torch.equal(tb, t.to(torch.bfloat16))

    g = rnd(n, scale=0.01, seed=82)
    out = torch.zeros(1, device=dev())
    ws = torch.empty(1024, device=dev())
    ops.grad_sumsq(g, out, ws, n)
    assert abs(float(out) - float(g.double().pow(2).sum())) < 1e-5 * float(out)

    p = rnd(n, seed=83)
    pref = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([pref], lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.04)
    m = torch.zeros(n, device=dev())
    v = torch.zeros(n, device=dev())
    pb = torch.empty(n, dtype=torch.bfloat16, device=dev())
    for step in (1, 2, 3):
        gstep = g * step
        pref.grad = gstep.clone()
        total = torch.nn.utils.clip_grad_norm_([pref], 0.5)
        opt.step()
        ops.grad_sumsq(gstep, out, ws, n)
        ops.adamw_step(p, gstep, m, v, n, lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-6, weight_decay=0.04, step=step,
                       max_norm=0.5, sumsq=out, p_bf16=pb)
        assert float(total) > 0.5          # clipping is active in this test
    assert relerr(p, pref.detach()) < 1e-5
    assert torch.equal(pb, p.to(torch.bfloat16))

    c = torch.empty(n + 3, dtype=torch.bfloat16, device=dev())
    src = rnd(n + 3, seed=84)
    ops.cast_f32_to_bf16(src, c, n + 3)
    assert torch.equal(c, src.to(torch.bfloat16))


def test_adamw_fused_zero_grad_and_sumsq_by_sections(ops):
    """ABI 16: wj_adamw_args.zero_grad clears the gradient behind the read (same update, g == 0 afterwards, also on a capped grid);
    wj_sumsq_args.accumulate / .workgroups give the squared norm section by section -- the sum of the sections' sums."""
    n = 4 * 250001
    g = rnd(n, scale=0.02, seed=182)
    out = torch.zeros(1, device=dev())
    ws = torch.empty(1024, device=dev())
    ops.grad_sumsq(g, out, ws, n)
    whole = float(out)
    cuts = [0, 4 * 1000, 4 * 77777, 4 * 200000, n]
    acc = torch.full((1,), 123.0, device=dev())                     # (overwritten by the first, non-accumulating section)
    for k, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        ops.grad_sumsq(g.data_ptr() + 4 * lo, acc, ws, hi - lo, accumulate=k > 0, workgroups=0 if k % 2 else 37)
    assert abs(float(acc) - whole) < 2e-6 * whole and abs(whole - float(g.double().pow(2).sum())) < 1e-5 * whole
    kw = dict(lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-6, weight_decay=0.04, step=1, max_norm=0.5, sumsq=out)
    res = []
    for zg, wgs in ((False, 0), (True, 0), (True, 64)):
        p = rnd(n, seed=183)
        gg = g.clone()
        m, v = torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
        pb = torch.empty(n, dtype=torch.bfloat16, device=dev())
        ops.adamw_step(p, gg, m, v, n, p_bf16=pb, zero_grad=zg, workgroups=wgs, **kw)
        torch.cuda.synchronize()
        res.append((p, m, v, pb))
        assert (float(gg.abs().max()) == 0.0) == zg
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)


def test_crop_normalize(ops, golden_dir):
    import os
    fx = dict(np.load(os.path.join(golden_dir, "crops.npz")))
    src = torch.from_numpy(fx["src"]).to(dev())
    starts = torch.from_numpy(fx["starts"]).to(torch.int32).to(dev())
    perm = torch.from_numpy(fx["perm"])
    B, S = starts.shape
    L = int(fx["target_length"])
    perm_inv = torch.empty_like(perm)
    perm_inv[perm] = torch.arange(perm.numel())
    out = torch.empty(B * S, 1, L, dtype=torch.bfloat16, device=dev())
    ops.crop_normalize_bf16(src, starts, out, B=B, S=S, C=1, L_full=src.shape[-1], length=L, perm_inv=perm_inv.to(torch.int32).to(dev()))
    want = torch.from_numpy(fx["out_bits"]).view(torch.bfloat16).to(dev())     # the REFERENCE's output bits
    diff = (out.float() - want.float()).abs()
    assert float(diff.max()) <= 2 ** -6 and float((diff > 0).float().mean()) < 2e-3


def test_rccl_bucket_allreduce_family_one_rank_world():
    """wj_rccl_unique_id -> _init -> _launch (average / sum, on a side stream) -> _wait -> _finalize through the C ABI on a world of one
    (the box has one GPU and RCCL takes one rank per device): reduced values equal the inputs bit for bit, the consuming stream is
    ordered behind the bucket stream, and a second init without finalize is refused.  In a child process: a communicator is
    per-process state."""
    import os
    import sys
    from tests import launch
    code = r'''
import torch
from wavjepa_amd import ops, _abi
dev = torch.device("cuda", 0)
uid = ops.rccl_unique_id()
assert len(uid) == 128 and any(uid)
ops.rccl_bucket_allreduce_init(uid, 0, 1)
try:
    ops.rccl_bucket_allreduce_init(uid, 0, 1)
    raise SystemExit("second init must be refused")
except _abi.WavJepaHipError:
    pass
g = torch.Generator(device="cpu").manual_seed(5)
x = torch.randn(3_000_000, generator=g).to(dev)
want = x.clone()
side = torch.cuda.Stream()
big = torch.randn(4096, 4096, device=dev)
for _ in range(20):
    big = big @ big * 1e-2                     # keep the compute stream busy: the bucket must wait for the producer below
x.mul_(2.0)
side.wait_stream(torch.cuda.current_stream())
ops.rccl_bucket_allreduce_launch(x.data_ptr(), x.numel(), average=True, stream=side.cuda_stream)
ops.rccl_bucket_allreduce_launch(x[1024:2048].data_ptr(), 1024, average=False, stream=side.cuda_stream)
ops.rccl_bucket_allreduce_wait(side.cuda_stream)
y = x * 0.5                                    # current stream: ordered behind both buckets
torch.cuda.synchronize()
assert torch.equal(y, want), float((y - want).abs().max())
ops.rccl_bucket_allreduce_finalize()
try:
    ops.rccl_bucket_allreduce_launch(x.data_ptr(), 16)
    raise SystemExit("launch after finalize must be refused")
except _abi.WavJepaHipError:
    pass
print("RCCL_FAMILY_OK")
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rc, out, err = launch.run([sys.executable, "-c", code], cwd=root, timeout=240)
    assert rc == 0 and "RCCL_FAMILY_OK" in out, (out[-2000:], err[-4000:])


@pytest.mark.parametrize("variant", [0, 3, 4])
def test_gelu_epilogue_on_every_bf16_input(ops, variant):
    """nn.GELU() on a bf16 tensor has 65 536 possible inputs: push every one of them through the BIAS_GELU2 epilogue (h = bf16(0 + bias),
    A = 0) of each GEMM schedule and hold gelu(h) and gelu'(h) to the correctly rounded float64 values -- within one bf16 ulp wherever the
    result is not deep in the negative tail (there: to 2e-7 |h| absolute, the A-S 7.1.26 erf's own error), and exactly h / 1 / -0 / 0 where
    the function has saturated.  (reference: wavjepa/types/wavjepa_configs.py:37 activation = nn.GELU())"""
    bits = torch.arange(65536, dtype=torch.int32)
    vals = (bits << 16).view(torch.float32)
    ok = torch.isfinite(vals) & (vals.abs() >= 2.0 ** -126)                   # normal, finite inputs (denormals are flushed on the way)
    N, M, K = 65536, 256, 128
    bias = torch.where(ok, vals, torch.zeros_like(vals)).to(dev())
    A = torch.zeros(M, K, dtype=torch.bfloat16, device=dev())
    W = rnd(N, K, scale=0.05, dtype=torch.bfloat16, seed=70)
    gp = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
    gl = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
    prev = ops.gemm_set_variant(variant)
    try:
        ops.gemm(A, W, gp, C2=gl, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, epilogue=ops.EPI_BIAS_GELU2, bias=bias)
        torch.cuda.synchronize()
    finally:
        ops.gemm_set_variant(prev)
    assert torch.equal(gl[0].view(torch.int16), gl[M - 1].view(torch.int16)) and torch.equal(gp[0].view(torch.int16), gp[137].view(torch.int16))
    h = vals.double()
    cdf = 0.5 * torch.erfc(-h / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)
    want = {"gelu": h * cdf, "gelu'": cdf + h * pdf}
    got = {"gelu": gl[0].cpu(), "gelu'": gp[0].cpu()}

    def ordinal(t):                                                           # bf16 bits -> integers ordered like the values
        b = t.view(torch.int16).to(torch.int32) & 0xFFFF
        return torch.where(b >= 0x8000, 0x8000 - b, b)

    for name in want:
        w = want[name].float().to(torch.bfloat16)
        ulp = (ordinal(got[name]) - ordinal(w)).abs()
        near = (got[name].double() - want[name]).abs() <= 2e-7 * h.abs().clamp(min=1.0)
        bad = ok & (ulp > 1) & ~near
        assert not bool(bad.any()), (name, variant, vals[bad][:8].tolist(), got[name][bad][:8].tolist(), w[bad][:8].tolist())
        frac = float(((ulp > 0) & ok).float().sum() / ok.float().sum())
        assert frac < 0.02, (name, variant, frac)                               # exactly rounded on > 98 % of the inputs
        print(name, "variant", variant, "inputs off by one ulp or in the tail:", int(((ulp > 0) & ok).sum()), "of", int(ok.sum()))
    big = ok & (vals >= 8.0)
    assert torch.equal(got["gelu"][big].view(torch.int16), vals[big].to(torch.bfloat16).view(torch.int16))      # gelu(h) = h
    assert bool((got["gelu'"][big].float() == 1.0).all())


def test_gelu_backward_kernel_on_every_bf16_input(ops):
    """The conv stack's GELU backward (dpre = dpost * gelu'(pre), pre a bf16 tensor) on all 65 536 bf16 values of `pre` with dpost = 1 and
    dpost = -0.75: within one bf16 ulp of the correctly rounded float64 product (or inside the erf approximation's 2e-7 |h| in the tail)."""
    bits = torch.arange(65536, dtype=torch.int32)
    vals = (bits << 16).view(torch.float32)
    ok = torch.isfinite(vals) & (vals.abs() >= 2.0 ** -126)
    pre = torch.where(ok, vals, torch.zeros_like(vals)).to(torch.bfloat16).to(dev())
    h = vals.double()
    gp = 0.5 * torch.erfc(-h / math.sqrt(2.0)) + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)

    def ordinal(t):
        b = t.view(torch.int16).to(torch.int32) & 0xFFFF
        return torch.where(b >= 0x8000, 0x8000 - b, b)

    for scale in (1.0, -0.75):
        dpost = torch.full((65536,), scale, dtype=torch.bfloat16, device=dev())
        out = torch.full((65536,), float("nan"), dtype=torch.bfloat16, device=dev())
        ops.gelu_bwd_bf16(dpost, pre, out, 65536)
        want = gp * scale
        got = out.cpu()
        ulp = (ordinal(got) - ordinal(want.float().to(torch.bfloat16))).abs()
        near = (got.double() - want).abs() <= 2e-7 * h.abs().clamp(min=1.0)
        bad = ok & (ulp > 1) & ~near
        assert not bool(bad.any()), (scale, vals[bad][:8].tolist(), got[bad][:8].tolist(), want[bad][:8].tolist())
        assert float(((ulp > 0) & ok).float().sum() / ok.float().sum()) < 0.02


def test_collective_footprint_measurement_aid(ops):
    """bench.py --emulate-allreduce: the stand-in for an all-reduce's on-GPU footprint rereads and rewrites the bucket in place -- the
    values must come back unchanged (ragged size, few / many workgroups), and a paced launch lasts at least its pace."""
    n = 3_000_003 * 4
    x = rnd(n, seed=90)
    ref = x.clone()
    for wgs, passes in ((32, 2), (1, 1), (256, 3)):
        ops.collective_footprint(x, n * 4 - (n * 4) % 16, workgroups=wgs, passes=passes)
        torch.cuda.synchronize()
        assert torch.equal(x, ref)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ops.collective_footprint(x, n * 4 - (n * 4) % 16, workgroups=32, passes=2, min_ticks=200_000)     # 2 ms of the 100 MHz clock
    e1.record()
    torch.cuda.synchronize()
    assert torch.equal(x, ref) and 1.9 < e0.elapsed_time(e1) < 4.0
    with pytest.raises(Exception):
        ops.collective_footprint(x, 24, workgroups=32)                       # not a multiple of 16 bytes


@pytest.mark.timeout(60)
def test_pair_and_persistent_gemms_finish_beside_a_long_lived_cu_holding_kernel(ops):
    """The RCCL-channel shape on one GPU: ONE launch of 32 resident workgroups (wj_collective_footprint, the laboratory library's rehearsal
    kernel, paced to last ~2 s) holds its CUs for the whole test, the way a collective's channel kernels do while they wait for a peer GPU.
    Beside it, on two other streams: the K-split PAIR kernel (two workgroups per tile that spin on each other's flags -- forward progress
    needs both roles resident; 234 workgroups for 256 CUs of which 32 are taken) and the persistent GEMM at 28 workgroups per XCD (the
    data-parallel default, wj_gemm_args.persist_cus).  Everything must finish inside the time-out with the bits of the undisturbed run."""
    M, N, K = 9945, 768, 3072                        # the ragged student's linear2: 39 x 3 = 117 tiles -> K-split pairs
    A = rnd(M, K, dtype=torch.bfloat16, seed=71)
    W = rnd(N, K, scale=0.03, dtype=torch.bfloat16, seed=72)
    need = ops.workspace_bytes("wj_gemm_bf16", M=M, N=N, K=K, lda=K, ldb=K, ldc=N, epilogue=ops.EPI_BF16)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=dev())
    Mp, Np, Kp = 51200, 768, 768                     # the teacher's out_proj: 600 items on the persistent kernel
    Ap = rnd(Mp, Kp, dtype=torch.bfloat16, seed=73)
    Wp = rnd(Np, Kp, scale=0.05, dtype=torch.bfloat16, seed=74)

    def run_pair(out):
        ops.gemm(A, W, out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, workspace=ws, schedule=3)

    def run_persist(out):
        ops.gemm(Ap, Wp, out, M=Mp, N=Np, K=Kp, lda=Kp, ldb=Kp, ldc=Np, schedule=4, persist_cus=28)

    ref_pair = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    ref_pers = torch.empty(Mp, Np, dtype=torch.bfloat16, device=dev())
    run_pair(ref_pair)
    run_persist(ref_pers)
    torch.cuda.synchronize()
    assert relerr(ref_pair.float(), A.float() @ W.float().t()) < 4e-3 and relerr(ref_pers.float(), Ap.float() @ Wp.float().t()) < 4e-3
    hold = rnd(16 * 1024 * 1024, seed=75)            # 64 MB bucket, rewritten in place (values unchanged)
    hold_ref = hold.clone()
    s_hold = torch.cuda.Stream()

    ops.spin(100, stream=s_hold.cuda_stream)          # load the code object before timing
    ticks = 30_000

    def single_ms() -> float:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s_hold)
        ops.spin(ticks, stream=s_hold.cuda_stream)
        e1.record(s_hold)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def pair_ms(cand) -> float:
        """HIP deals streams onto a few hardware queues; two streams on one queue serialise (wavjepa_amd.engine._pick_side_stream).  Two
        busy-wait waves (~0.3 ms each), started together: concurrent streams take one wait, serialised ones two (measured with 16
        candidates: 1.05-1.35 beside, 2.2-2.5 on the holder's queue -- every fourth stream of torch's pool)."""
        best = 1e9
        for _ in range(3):
            e0, e1, go, done = (torch.cuda.Event(enable_timing=True) for _ in range(4))
            go.record(s_hold)
            cand.wait_event(go)
            e0.record(s_hold)
            ops.spin(ticks, stream=s_hold.cuda_stream)
            ops.spin(ticks, stream=cand.cuda_stream)
            done.record(cand)
            s_hold.wait_event(done)
            e1.record(s_hold)
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1))
        return best

    single = min(single_ms() for _ in range(3))
    if single < 0.25:                                 # s_memtime ticks at the shader clock here (measured: 30 000 ticks = 16 us): stretch the
        ticks = int(ticks * 0.3 / max(single, 1e-3))  # wait to ~0.3 ms, where the cross-stream event hops (~15 us) no longer blur the ratio
        single = min(single_ms() for _ in range(3))
    pool = [torch.cuda.Stream() for _ in range(12)]
    ratios = [round(pair_ms(c) / single, 2) for c in pool]
    print("stream probe: single", round(single, 3), "ms; pair / single per candidate", ratios)
    beside = [c for c, r in zip(pool, ratios) if r < 1.5]
    assert len(beside) >= 2, ("no two streams that run beside the holder's stream", single, ratios)
    s_pair, s_pers = beside[0], beside[1]
    # the NaN fills run on the default stream, which may share the holder's hardware queue: they must be done before the holder starts,
    # or they land ~2 s later on top of the GEMMs' results
    outs_pair = [torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev()) for _ in range(4)]
    outs_pers = [torch.full((Mp, Np), float("nan"), dtype=torch.bfloat16, device=dev()) for _ in range(4)]
    torch.cuda.synchronize()
    done_hold = torch.cuda.Event()
    with torch.cuda.stream(s_hold):
        ops.collective_footprint(hold, hold.numel() * 4, workgroups=32, passes=8, min_ticks=200_000_000)    # ~2 s of the 100 MHz clock
        done_hold.record(s_hold)
    import time
    time.sleep(0.05)                                  # the holder is resident before the GEMMs are queued
    for rep in range(24):
        with torch.cuda.stream(s_pair):
            run_pair(outs_pair[rep % 4])
        with torch.cuda.stream(s_pers):
            run_persist(outs_pers[rep % 4])
    s_pair.synchronize()
    s_pers.synchronize()
    assert not done_hold.query(), "the CU-holding launch ended before the GEMMs did: nothing was tested"
    for o in outs_pair:
        assert torch.equal(o.view(torch.int16), ref_pair.view(torch.int16))
    for o in outs_pers:
        assert torch.equal(o.view(torch.int16), ref_pers.view(torch.int16))
    torch.cuda.synchronize()
    assert torch.equal(hold, hold_ref)
    assert int(ws[:4096].view(torch.int32).abs().sum()) == 0          # the pair flags are back at zero


def test_gemm_persistent_counter_slots_are_recycled(ops):
    """The persistent kernel keys its tile counters by stream (64 sets).  A host that keeps creating streams used to drop to the one-tile
    schedule from the 65th stream on; idle streams' sets are now handed on (least recently used first).  80 streams, two launches each
    into NaN-filled outputs: every result must equal the first stream's bits (a counter set shared by two live launches, or one that
    was not back at zero, would skip or repeat tiles)."""
    M, N, K = 8192, 2048, 256
    A = rnd(M, K, dtype=torch.bfloat16, seed=31)
    W = rnd(N, K, scale=0.08, dtype=torch.bfloat16, seed=32)
    prev = ops.gemm_set_variant(4)
    try:
        ref = None
        streams = [torch.cuda.Stream() for _ in range(80)]
        outs = []
        for st in streams:
            C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                ops.gemm(A, W, C, M=M, N=N, K=K, lda=K, ldb=K, ldc=N)
                ops.gemm(A, W, C, M=M, N=N, K=K, lda=K, ldb=K, ldc=N)
            outs.append(C)
            if len(outs) % 16 == 0:
                torch.cuda.synchronize()             # earlier streams are idle: their counter sets may change hands
        torch.cuda.synchronize()
        ref = outs[0]
        assert not bool(torch.isnan(ref.float()).any()) and relerr(ref.float(), A.float() @ W.float().t()) < 4e-3
        for C in outs[1:]:
            assert torch.equal(C.view(torch.int16), ref.view(torch.int16))
        # streams handed back explicitly (wj_gemm_release_stream, before they are destroyed): their counter sets serve the next newcomers
        for st in streams[-8:]:
            st.synchronize()
            ops.gemm_release_stream(st.cuda_stream)
        fresh = [torch.cuda.Stream() for _ in range(8)]
        for st in fresh:
            C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                ops.gemm(A, W, C, M=M, N=N, K=K, lda=K, ldb=K, ldc=N)
            st.synchronize()
            assert torch.equal(C.view(torch.int16), ref.view(torch.int16))
    finally:
        ops.gemm_set_variant(prev)


@pytest.mark.parametrize("M,N,K,T", [(5000, 768, 512, 200), (2100, 256, 128, 99), (777, 512, 64, 50)])
def test_gemm_add_pos_epilogue_equals_gemm_then_add_pos(ops, M, N, K, T):
    """WJ_EPI_BF16_ADD_POS (the post-extraction mapper with the position add of jepa.py:394-396 in its epilogue, SURVEY K8 + K9) gives
    exactly the bits of the two-launch form: bf16 mapper output, then wj_add_pos."""
    A = rnd(M, K, dtype=torch.bfloat16, seed=41)
    W = rnd(N, K, scale=0.06, dtype=torch.bfloat16, seed=42)
    bias = rnd(N, seed=43)
    pos = rnd(T, N, seed=44)
    mid = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    ops.gemm(A, W, mid, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias)
    y32 = torch.empty(M, N, device=dev())
    y16 = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    ops.add_pos(mid, pos, M=M, T=T, D=N, y_f32=y32, y_bf16=y16)
    f32 = torch.full((M, N), float("nan"), device=dev())
    f16 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
    ops.gemm(A, W, f16, C2=f32, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias, epilogue=ops.EPI_BF16_ADD_POS, aux=pos, seg_rows=T)
    torch.cuda.synchronize()
    # (the two-launch form may run the persistent schedule, whose bias-first accumulation differs in the last place on <= 0.05 % of the
    # bf16 mapper outputs: compared against the one-tile schedule the fused epilogue shares)
    prev = ops.gemm_set_variant(3)
    try:
        ops.gemm(A, W, mid, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias)
    finally:
        ops.gemm_set_variant(prev)
    ops.add_pos(mid, pos, M=M, T=T, D=N, y_f32=y32, y_bf16=y16)
    torch.cuda.synchronize()
    assert torch.equal(f32, y32) and torch.equal(f16.view(torch.int16), y16.view(torch.int16))
    ref = (A.float() @ W.float().t() + bias).to(torch.bfloat16).float() + pos.repeat((M + T - 1) // T, 1)[:M]
    assert relerr(f32, ref) < 4e-3
    with pytest.raises(Exception):
        ops.gemm(A, W, f16, C2=f32, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, epilogue=ops.EPI_BF16_ADD_POS)      # no position table
