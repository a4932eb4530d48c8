"""Forced schedules of the one-tile GEMM kernels (csrc/gemm.hip) at the smallest shapes at which their K loops can go wrong, single
launches held to the fp64 bound of tests/gemm_reference.py (every element of the output region within its per-element bound, every
byte outside it unchanged: `Operands` / `reference` / `check` as the census uses them).

  * schedule 1..4 (variants 0-3), row-form operands: M = 300 (a clamped last row tile), N = 256 / 384, K = 128 (two 64-deep tiles:
    prologue and drain only), 256 (the first steady-state pair), 384; BF16 with bias and BIAS_GELU2;
  * schedule 1..3 (variants 0-2), K tails: also the col-form layouts (0,1) and (1,1); K = 40 (a tail through the zero page, fewer tiles
    than ring stages), 96 (full tiles, still fewer than the ring), 136 (a tail behind full tiles);
  * split-K: (1,1) ATOMIC_F32, split_k = 3, K = 800;
  * grouped weight gradients, one launch per tile form (256 x 256, 256 x 128, 384 x 128), K = 200.
A variant that cannot run a shape falls back by the documented rule (include/wavjepa_hip.h); the result is checked all the same.
One reference per shape serves every schedule of it."""
import pytest
import torch

from tests import gemm_reference as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    return o


def dev():
    return torch.device("cuda:0")


def fields(M, N, K, a_trans=0, b_trans=0, epilogue="BF16", bias=True, split_k=1):
    """One ops.gemm call as gemm_reference describes it; ldc leaves 8 columns between the rows of C (they must stay untouched)"""
    return dict(entry="gemm", unknown=(), M=M, N=N, K=K, lda=M if a_trans else K, ldb=N if b_trans else K, ldc=N + 8,
                a_trans=a_trans, b_trans=b_trans, epilogue=epilogue, bias=bias, C=True, C2=epilogue == "BIAS_GELU2", aux=False,
                colsum=False, split_k=split_k, seg_rows=0, seg_valid=0, alpha=1.0, rowmap=None, workspace=False, schedule=None,
                persist_cus=None, align=())


def run_schedules(ops, f, schedules, seed):
    o = gr.Operands(f, dev(), seed=seed)
    o.reset_outputs()
    snap = o.snapshot()
    exp = gr.reference(o, snap)
    fails = []
    for sched in schedules:
        o.reset_outputs()
        ops.gemm(**o.kwargs(), schedule=sched)
        torch.cuda.synchronize()
        bad, worst = gr.check(o, exp, snap)
        print(f"{gr.describe(f)} schedule={sched}: worst |got - ref| / bound = {worst:.3f}")
        fails += [f"schedule {sched}: {b}" for b in bad]
    assert not fails, gr.describe(f) + "\n" + "\n".join(fails)


@pytest.mark.parametrize("epilogue", ["BF16", "BIAS_GELU2"])
@pytest.mark.parametrize("K", [128, 256, 384])
@pytest.mark.parametrize("N", [256, 384])
def test_row_form_schedules_1_to_4(ops, N, K, epilogue):
    run_schedules(ops, fields(300, N, K, epilogue=epilogue), (1, 2, 3, 4), seed=N + K)


@pytest.mark.parametrize("K", [40, 96, 136])
@pytest.mark.parametrize("N", [256, 384])
@pytest.mark.parametrize("layout", [(0, 0), (0, 1), (1, 1)])
def test_k_tails_schedules_1_to_3(ops, layout, N, K):
    at, bt = layout
    M = 296 if at else 300            # col-form A: M % 8 == 0 (wj_gemm_bf16's argument rule)
    run_schedules(ops, fields(M, N, K, a_trans=at, b_trans=bt), (1, 2, 3), seed=7 * N + K + at + 2 * bt)


def test_split_k_atomic(ops):
    run_schedules(ops, fields(296, 256, 800, a_trans=1, b_trans=1, epilogue="ATOMIC_F32", bias=False, split_k=3), (None,), seed=800)


# (n_out, k_in): N % 256 == 0 -> 256 x 256 tiles; n_out % 384 == 0 and k_in % 128 == 0 -> 384 x 128; otherwise 256 x 128
@pytest.mark.parametrize("n_out,k_in", [(320, 256), (320, 384), (384, 384)], ids=["256x256", "256x128", "384x128"])
def test_grouped_wgrad_tile_forms(ops, n_out, k_in):
    f = gr.wgrad_fields(None, None, None, n_out, k_in, 200)
    o = gr.Operands(f, dev(), seed=n_out + k_in)
    o.reset_outputs()
    snap = o.snapshot()
    exp = gr.reference(o, snap)
    ops.wgrad_grouped([(o.b["A"].ptr, o.b["B"].ptr, o.b["C"].ptr, n_out, k_in, 200)])
    torch.cuda.synchronize()
    bad, worst = gr.check(o, exp, snap)
    print(f"{gr.describe(f)}: worst |got - ref| / bound = {worst:.3f}")
    assert not bad, gr.describe(f) + "\n" + "\n".join(bad)
