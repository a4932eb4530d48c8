"""Deterministic mode, host side: the workspace queries of the store-and-sum forms, their argument checks (answered before any
launch, so they run without a GPU), the struct mirrors and the documented switch."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kps(K, split):
    return ((K + split - 1) // split + 63) // 64 * 64


def _split(K, want):
    """K slices of a split-K launch as the header states them: 64-deep multiples, none empty"""
    want = max(1, want)
    return -(-K // _kps(K, want))


def _group(shapes, K, deterministic=1):
    from wavjepa_amd import _abi
    a = _abi.STRUCTS["wj_wgrad_group_args"]()
    for i, (m, n) in enumerate(shapes):
        a.A[i] = a.B[i] = a.C[i] = 256
        a.M[i], a.N[i], a.K[i] = m, n, K if isinstance(K, int) else K[i]
        a.lda[i], a.ldb[i], a.ldc[i] = m, n, n
    a.n = len(shapes)
    a.deterministic = deterministic
    return a


def _group_split(shapes, K, bm, bn, slots):
    """launch_grouped's rule: one factor for the group (tiles x split ~ the chip, rounded to nearest), K slices >= 1024 deep"""
    tiles = sum(-(-m // bm) * -(-n // bn) for m, n in shapes)
    out = []
    for i, _ in enumerate(shapes):
        k = K if isinstance(K, int) else K[i]
        s = max(1, (slots + tiles // 2) // tiles)
        s = min(s, -(-k // 1024))
        out.append(_split(k, s))
    return out


def test_new_fields_are_mirrored_and_zero_means_the_default_path():
    from wavjepa_amd import _abi
    lib = _abi.load()
    assert _abi.DEFINES["WJ_ABI_VERSION"] == 17 == lib.wj_abi_version()
    for name in ("wj_gemm_args", "wj_wgrad_group_args", "wj_colsum_args", "wj_colsum_group_args", "wj_attn_bwd_args"):
        cls = _abi.STRUCTS[name]
        fields = [f[0] for f in cls._fields_]
        assert "deterministic" in fields, name
        assert fields.index("deterministic") == len(fields) - 1, f"{name}: new fields go at the end"
        assert lib.wj_struct_size(name.encode()) == ctypes.sizeof(cls), name
        assert cls().deterministic == 0
    for name in ("wj_wgrad_group_args", "wj_colsum_args"):
        fields = [f[0] for f in _abi.STRUCTS[name]._fields_]
        assert fields[-3:] == ["workspace", "workspace_bytes", "deterministic"], name
    # a zero-initialised struct asks for no deterministic scratch
    assert _abi.workspace_bytes("wj_wgrad_grouped", _group([(384, 1536)], 84000, deterministic=0)) == 0
    c = _abi.STRUCTS["wj_colsum_args"]()
    c.M, c.N = 84000, 1152
    assert _abi.workspace_bytes("wj_colsum_bf16", c) == 0


def test_workspace_bytes_of_the_deterministic_weight_gradients():
    """need = split x M x ldc x 4 with the split the launch uses"""
    from wavjepa_amd import _abi, ops
    # the predictor's group: d = 384, 84 k token rows -> the 384 x 128 tile, 256 slots
    shapes = [(384, 1536), (1536, 384), (384, 384), (1152, 384)]
    K = 84000
    splits = _group_split(shapes, K, 384, 128, 256)
    assert splits[0] > 1
    want = sum(s * m * n * 4 for s, (m, n) in zip(splits, shapes))
    assert _abi.workspace_bytes("wj_wgrad_grouped", _group(shapes, K)) == want
    assert ops.wgrad_grouped_workspace_bytes([(0, 0, 0, m, n, K) for m, n in shapes]) == want
    # problems of one group with different token counts (the last predictor layer): each problem its own slices
    Ks = [46547, 46547, 46547, 87071]
    splits = _group_split(shapes, Ks, 384, 128, 256)
    assert _abi.workspace_bytes("wj_wgrad_grouped", _group(shapes, Ks)) == sum(s * m * n * 4 for s, (m, n) in zip(splits, shapes))
    # two student layers: 216 tiles of 256 x 256 for 256 slots -> split 1, the existing epilogue has one adder per element: need 0
    student = [(768, 3072), (3072, 768), (768, 768), (2304, 768)] * 2
    assert _group_split(student, 10131, 256, 256, 256) == [1] * 8
    assert _abi.workspace_bytes("wj_wgrad_grouped", _group(student, 10131)) == 0
    # one student layer: 108 tiles -> split 2
    one = student[:4]
    splits = _group_split(one, 10131, 256, 256, 256)
    assert splits == [2] * 4
    assert _abi.workspace_bytes("wj_wgrad_grouped", _group(one, 10131)) == sum(2 * m * n * 4 for m, n in one)
    # ungrouped: a mapper weight gradient and the sparse conv gather form (ldc > N stays the slab's row stride)
    for M, N, K, ldc, want_split in ((768, 384, 46547, 384, 46), (512, 1536, 44010, 1536, 21), (512, 1024, 10131, 1024, 10), (512, 1024, 10131, 1088, 10)):
        sk = ops.pick_split_k(M, N, K)
        assert _split(K, sk) == want_split
        got = ops.workspace_bytes("wj_gemm_bf16", M=M, N=N, K=K, ldc=ldc, a_trans=1, b_trans=1, epilogue=ops.EPI_ATOMIC_F32, split_k=sk,
                                  deterministic=1)
        assert got == want_split * M * ldc * 4
    # one slice: no slabs
    assert ops.workspace_bytes("wj_gemm_bf16", M=768, N=384, K=900, ldc=384, a_trans=1, b_trans=1, epilogue=ops.EPI_ATOMIC_F32, split_k=1,
                               deterministic=1) == 0
    # the bf16 column sums: one partial row of N floats per row range
    n = ops.workspace_bytes("wj_colsum_bf16", M=84000, N=1152, deterministic=1)
    assert n > 0 and n % (1152 * 4) == 0 and n // (1152 * 4) <= 2048 // (1152 // 64)


def test_deterministic_forms_reject_a_missing_or_short_workspace_without_a_gpu():
    """WJ_ERR_ARG (-1), never a fall-back to atomics; answered before any launch"""
    from wavjepa_amd import _abi, ops
    lib = _abi.load()
    a = _abi.STRUCTS["wj_gemm_args"]()
    a.A = a.B = a.C = 256
    a.M, a.N, a.K, a.lda, a.ldb, a.ldc = 768, 384, 46547, 768, 384, 384
    a.a_trans = a.b_trans = 1
    a.epilogue, a.split_k, a.alpha, a.deterministic = ops.EPI_ATOMIC_F32, 46, 1.0, 1
    need = _abi.workspace_bytes("wj_gemm_bf16", a)
    assert need == 46 * 768 * 384 * 4
    assert lib.wj_gemm_bf16(ctypes.byref(a), None) == -1             # no workspace
    a.workspace, a.workspace_bytes = 4096, need - 4
    assert lib.wj_gemm_bf16(ctypes.byref(a), None) == -1             # short
    a.workspace, a.workspace_bytes = 4100, need
    assert lib.wj_gemm_bf16(ctypes.byref(a), None) == -1             # not 16-byte aligned
    a.workspace, a.a_trans = 4096, 0
    a.lda = 46552
    assert lib.wj_gemm_bf16(ctypes.byref(a), None) in (-1, -3)       # row-form split-K: no deterministic form
    b = _abi.STRUCTS["wj_gemm_args"]()                               # the fused column sums are atomics: refused
    b.A = b.B = b.C = 256
    b.colsum = 256
    b.M, b.N, b.K, b.lda, b.ldb, b.ldc, b.deterministic = 256, 256, 256, 256, 256, 256, 1
    assert lib.wj_gemm_bf16(ctypes.byref(b), None) == -1
    g = _group([(384, 1536), (1536, 384), (384, 384), (1152, 384)], 84000)
    need = _abi.workspace_bytes("wj_wgrad_grouped", g)
    assert lib.wj_wgrad_grouped(ctypes.byref(g), None) == -1
    g.workspace, g.workspace_bytes = 4096, need - 4
    assert lib.wj_wgrad_grouped(ctypes.byref(g), None) == -1
    c = _abi.STRUCTS["wj_colsum_args"]()
    c.x = c.out = 256
    c.M, c.N, c.ldx, c.deterministic = 84000, 1152, 1152, 1
    assert lib.wj_colsum_bf16(ctypes.byref(c), None) == -1
    c.workspace, c.workspace_bytes = 4096, _abi.workspace_bytes("wj_colsum_bf16", c) - 4
    assert lib.wj_colsum_bf16(ctypes.byref(c), None) == -1


def test_switch_is_read_by_the_engine_and_documented():
    src = open(os.path.join(ROOT, "wavjepa_amd", "encoder_engine.py")).read()       # (the base of both step engines reads the switches)
    assert 'environ.get("WJ_DETERMINISTIC", "0")' in src
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [ln for ln in doc.splitlines() if ln.startswith("|") and "`WJ_DETERMINISTIC`" in ln]
    assert row, "WJ_DETERMINISTIC is missing from INTEGRATION.md's switch table"
    # the library itself reads no environment for the mode: it travels in the argument structs
    for name in os.listdir(os.path.join(ROOT, "wavjepa_amd", "csrc")):
        assert "WJ_DETERMINISTIC" not in open(os.path.join(ROOT, "wavjepa_amd", "csrc", name), errors="replace").read(), name


def test_trainer_configs_carry_the_switch_off():
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "configs", "trainer", "*.yaml")))
    assert files
    for p in files:
        assert any(ln.split("#")[0].strip() == "deterministic: false" for ln in open(p)), p
