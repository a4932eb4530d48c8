"""What a build of the library answers to its callers' questions, as text to diff between two builds:

    python tools/abi_dump.py wavjepa_amd/lib/libwavjepa_hip.so > a.txt

prints the exported wj_ symbols (nm -D), wj_struct_size of every struct of the headers, and wj_workspace_bytes over a fixed grid of
VALID argument sets: what the CPU tests query, what the engine queries at the benchmark configuration (256 clips of 2 s, encoder 768 /
12 heads, predictor 384, 4 target groups of 200 steps), and for every rule its smallest and its largest supported shape, with the
deterministic and listed-row forms where it has them.  Refused dimensions are the business of tests/test_host_cpu.py.
Needs no GPU; the struct layouts come from the headers of the tree this file is in."""
import ctypes
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (the library binds to the HIP runtime torch ships)
from wavjepa_amd import _abi  # noqa: E402

STRUCTS = {**_abi.STRUCTS, **_abi.LAB_STRUCTS}
EPI = _abi.ENUMS
BIG = 1 << 30


def grid():
    """[(entry, struct, {field: value})]"""
    g = []

    def q(fn, struct, **dims):
        g.append((fn, struct, dims))
    # ---- LayerNorm backward (any M): smallest, the tests' widths, the widest the kernels take
    for D in (4, 64, 128, 256, 384, 512, 768, 1024, 2048):
        q("wj_layernorm_bwd", "wj_ln_bwd_args", D=D, M=1)
        q("wj_layernorm_pre_bwd", "wj_ln_pre_bwd_args", D=D, M=51200)
    # ---- attention backward, both families: one row per sequence
    for B, H, hd in ((1, 1, 16), (1, 1, 32), (1024, 12, 32), (256, 12, 64), (1024, 12, 64), (65536, 16, 64)):
        for fn in ("wj_attn_bwd", "wj_attn_stream_bwd"):
            q(fn, "wj_attn_bwd_args", B=B, H=H, hd=hd, T=200, mask_group=1)
    # ---- conv layer 0 (GroupNorm): the chunk count follows the clip count; dense and listed-row backward
    for N in (1, 2, 3, 8, 64, 200, 256, 500, 1024, 2000):
        for C_in in (1, 2):
            for C in (16, 32, 48, 64, 80, 512, 576):
                for L_out in (1, 31, 32, 33, 255, 256, 257, 513, 1500, 2100, 2177, 6430, 20000):
                    q("wj_conv0_gn_gelu_fwd", "wj_conv0_fwd_args", N=N, C_in=C_in, C=C, k=10, L_out=L_out)
    for N in (1, 64, 256, 2000):
        for C_in in (1, 2):
            for L_out, max_rows in ((1, 0), (256, 0), (257, 0), (6430, 0), (6430, 1), (6430, 1300), (6430, 6430), (32000, 0)):
                for C in (4, 64, 512):
                    q("wj_conv0_gn_gelu_bwd", "wj_conv0_bwd_args", N=N, C_in=C_in, C=C, k=10, L_out=L_out, max_rows=max_rows)
    # ---- conv stack in layer-norm mode
    for rows, C in ((0, 64), (1, 64), (120, 64), (5000, 512), (823168, 512), (3, 128), (77, 256), (1 << 30, 512)):
        q("wj_conv_ln_gelu_bwd", "wj_conv_ln_bwd_args", M=rows, C=C)
        q("wj_conv_ln_gelu_bwd", "wj_conv_ln_bwd_args", M=1 << 30, C=C, rows=1, n_rows=rows)       # the listed-row form
    for N in (1, 3, 256, 2000):
        for C_in, C, L_out in ((1, 64, 1), (1, 64, 162), (1, 512, 6430), (2, 512, 6431), (2, 512, 32000)):
            for max_rows in (0, 1, 40, 512, 513, L_out):
                q("wj_conv0_ln_gelu_bwd", "wj_conv0_ln_bwd_args", N=N, C_in=C_in, C=C, k=10, L_out=L_out, max_rows=max_rows)
    # ---- token scatter backward, losses, gradient norm
    for B, T, D, G in ((1, 1, 4, 1), (256, 200, 384, 4), (256, 200, 768, 4), (64, 400, 384, 4), (1024, 1024, 1024, 15)):
        q("wj_mask_scatter_fill_pos_bwd", "wj_scatter_fill_bwd_args", B=B, T=T, D=D, G=G)
        q("wj_masked_mse", "wj_mse_args", B=B, G=G, T=T, D=D)
        for kind in range(4):
            q("wj_masked_loss", "wj_loss_args", B=B, G=G, T=T, D=D, kind=kind, beta=1.0, rows=kind & 1, n_rows=17 * (kind & 1))
    for n in (4, 1 << 20, 1 << 33):
        q("wj_grad_sumsq", "wj_sumsq_args", n=n)
        q("wj_grad_sumsq", "wj_sumsq_args", n=n, workgroups=64)
    # ---- GEMM: the K-split pair rule on the tests' grid, the engine's scratch, the deterministic slabs
    for M in (8, 900, 4000, 8300, 9945, 12000, 16384, 32768, 33000, 51200):
        for N in (256, 384, 512, 768, 1024):
            for K in (256, 768, 1280, 1536, 2304, 3072):
                q("wj_gemm_bf16", "wj_gemm_args", M=M, N=N, K=K, lda=K, ldb=K, ldc=N, epilogue=EPI["WJ_EPI_BF16"])
    gemm = dict(M=9945, N=768, K=3072, lda=3072, ldb=3072, ldc=768)
    q("wj_gemm_bf16", "wj_gemm_args", epilogue=EPI["WJ_EPI_ADD_F32"], **gemm)
    q("wj_gemm_bf16", "wj_gemm_args", epilogue=EPI["WJ_EPI_BF16"], b_trans=1, **gemm)
    q("wj_gemm_bf16", "wj_gemm_args", M=256 * 64, N=512, K=2048, lda=2048, ldb=2048, ldc=512, epilogue=EPI["WJ_EPI_BF16"])
    det_shapes = [(768, 384), (384, 768), (768, 512), (512, 1536), (512, 1024), (8, 8), (3072, 768)]
    for m, n in det_shapes:
        for K in (8, 10240, 51200, BIG):
            bn = 256 if n % 256 == 0 else 128                       # ops.pick_split_k
            tiles = ((m + 255) // 256) * ((n + bn - 1) // bn)
            split = max(1, min(max(1, ((256 if bn == 256 else 512) + tiles // 2) // max(1, tiles)), (K + 1023) // 1024))
            for rowmap in (0, 1):
                q("wj_gemm_bf16", "wj_gemm_args", M=m, N=n, K=K, ldc=n, a_trans=1, b_trans=1, epilogue=EPI["WJ_EPI_ATOMIC_F32"],
                  split_k=split, deterministic=1, rowmap=rowmap)
    for M in (1, 8, 10240, 51200, BIG):
        for N in (8, 384, 768, 1536, 3072):
            q("wj_colsum_bf16", "wj_colsum_args", M=M, N=N, deterministic=1)
            q("wj_colsum_bf16", "wj_colsum_args", M=M, N=N)
    # ---- scene augmentation, denoiser stage, audio preparation
    for B, C, T, L, fft in ((2, 1, 1, 1, 1024), (1, 3, 511, 513, 1024), (2, 2, 512, 512, 1024), (1, 1, 1537, 2049, 1024),
                            (2, 1, 5000, 9000, 1024), (1, 2, 9000, 4097, 0), (1, 1, 100, 30000, 0), (8, 2, 320000, 48000, 0)):
        q("wj_rir_convolve", "wj_rir_conv_args", B=B, C=C, T=T, L=L, fft_size=fft)
        q("wj_snr_mix", "wj_snr_mix_args", B=B, C=C, T=T)
    for G in (1, 2, 8):
        q("wj_mse_groups", "wj_mse_groups_args", G=G, n=1)
        q("wj_mse_groups", "wj_mse_groups_args", G=G, n=1 << 28)
    q("wj_audio_prepare", "wj_audio_prepare_args", table=1, n_clips=2, B=2, max_len=100, orig=2, nw=1, width=136, taps=274, out_len=1000)
    q("wj_audio_prepare", "wj_audio_prepare_args", table=1, n_clips=32, B=32, max_len=441000, orig=441, nw=160, width=187, taps=815, out_len=160000)
    q("wj_audio_prepare", "wj_audio_prepare_args", table=1, n_clips=3, B=4, max_len=48000, orig=3, nw=1, width=20, taps=43, out_len=16000)
    q("wj_audio_prepare", "wj_audio_prepare_args", table=1, n_clips=3, B=4, max_len=48000, orig=2, nw=3, width=20, taps=42, out_len=72000)
    q("wj_audio_prepare", "wj_audio_prepare_args", table=0, n_clips=1, B=1, max_len=0, orig=1, nw=1, out_len=1)
    q("wj_audio_prepare", "wj_audio_prepare_args", table=0, n_clips=64, B=64, max_len=160000, orig=1, nw=1, out_len=160000, pcm_kind=2)
    for B, n_clips, max_len, out_len, fade in ((2, 2, 8000, 5000, 640), (128, 128, 8000, 5000, 640), (1, 1, 1, 1, 1), (64, 17, 960000, 320000, 3200)):
        q("wj_noise_prepare", "wj_noise_prepare_args", B=B, n_clips=n_clips, max_len=max_len, out_len=out_len, fade_len=fade)
    return g


def wgrad_groups():
    """the engine's deterministic grouped weight gradients (JepaEngine._det_ws_bytes) and the plain form"""
    out = []
    for d, group in ((768, 2), (384, 1), (128, 2), (64, 1)):
        layer = [(d, 4 * d), (4 * d, d), (d, d), (3 * d, d)]
        for n in range(1, group + 1):
            for K in (8, 10240, 51200, BIG):
                for det in (0, 1):
                    out.append(([(m, k, K) for m, k in layer * n], det))
    return out


def main(path: str) -> None:
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = sorted(ln.split()[-1] for ln in nm.splitlines() if " T wj_" in ln)
    for sym in exported:
        print("export", sym)
    lib = ctypes.CDLL(path)
    lib.wj_struct_size.argtypes, lib.wj_struct_size.restype = [ctypes.c_char_p], ctypes.c_int
    lib.wj_workspace_bytes.argtypes, lib.wj_workspace_bytes.restype = [ctypes.c_char_p, ctypes.c_void_p], ctypes.c_int64
    print("abi_version", lib.wj_abi_version())
    for name in sorted(STRUCTS):
        print("sizeof", name, lib.wj_struct_size(name.encode()))
    for fn, struct, dims in grid():
        n = lib.wj_workspace_bytes(fn.encode(), ctypes.byref(STRUCTS[struct](**dims)))
        print("ws", fn, " ".join(f"{k}={v}" for k, v in dims.items()), "->", n)
    for problems, det in wgrad_groups():
        a = STRUCTS["wj_wgrad_group_args"](n=len(problems), deterministic=det)
        for i, (m, n_, k) in enumerate(problems):
            a.M[i], a.N[i], a.K[i], a.lda[i], a.ldb[i], a.ldc[i] = m, n_, k, m, n_, n_
        print("ws wj_wgrad_grouped", f"det={det}", problems, "->", lib.wj_workspace_bytes(b"wj_wgrad_grouped", ctypes.byref(a)))
    for fn, struct in sorted(_abi.ENTRY_ARGS.items()):                # entries without scratch answer 0 whatever the arguments
        if fn in exported and fn not in {g[0] for g in grid()} | {"wj_wgrad_grouped"}:
            print("ws", fn, "(zeroed) ->", lib.wj_workspace_bytes(fn.encode(), ctypes.byref(STRUCTS[struct]())))


if __name__ == "__main__":
    main(sys.argv[1])
