"""Build libwavjepa_hip.so (gfx950) in-tree with hipcc.  No torch dependency: plain HIP + a C ABI."""
from __future__ import annotations

import glob
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
SOURCES = ["gemm.hip", "gemm_persist.hip", "gemm_pde.hip", "gemm_panel.hip", "norm.hip", "attention.hip", "attention_stream.hip", "conv0.hip", "conv_ln.hip", "misc.hip", "abi.hip", "fp8.hip", "scene.hip", "denoise.hip", "audio_prep.hip", "noise_prep.hip", "rccl_bucket.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wno-unused-value"]


class Library(NamedTuple):
    file: str          # under wavjepa_amd/lib
    sources: list      # under wavjepa_amd/csrc
    flags: list        # behind FLAGS
    objdir: str        # under wavjepa_amd/lib

    @property
    def path(self) -> str:
        return os.path.join(LIBDIR, self.file)


# Every shared library of the package, in build order (the keys are wavjepa_amd._abi.LIBRARIES' too).  A side library exports what its
# header declares and nothing else: -fvisibility=hidden keeps the release entries that its shared sources also define inside it.
LIBRARIES = {
    # compute + query entries, production-safe switches only (include/wavjepa_hip.h)
    "release": Library("libwavjepa_hip.so", SOURCES, [], "obj"),
    # the dropout forms of the LayerNorm and streamed-attention kernels, from the SAME sources, and wj_dropout_rows (include/wavjepa_hip_dropout.h)
    "dropout": Library("libwavjepa_hip_dropout.so", ["dropout.hip", "norm.hip", "attention_stream.hip"], ["-DWJ_DROPOUT_LIB", "-fvisibility=hidden"], "obj_dropout"),
    # wj_masked_moments, the collapse monitor (include/wavjepa_hip_monitor.h)
    "monitor": Library("libwavjepa_hip_monitor.so", ["monitor.hip"], ["-fvisibility=hidden"], "obj_monitor"),
    # wj_gemm_bf16_act, linear1's forward GEMM with the activation chosen per call, from the SAME GEMM sources: the one-tile and the
    # persistent kernels, the activation a template argument there (include/wavjepa_hip_act.h)
    "act": Library("libwavjepa_hip_act.so", ["gemm.hip", "gemm_persist.hip"], ["-DWJ_ACT_LIB", "-fvisibility=hidden"], "obj_act"),
    # wj_adamw_groups_step, the AdamW pass with parameter groups (include/wavjepa_hip_optim.h)
    "optim": Library("libwavjepa_hip_optim.so", ["optim.hip"], ["-fvisibility=hidden"], "obj_optim"),
    # the release sources with -DWJ_LAB: the extra entries of include/wavjepa_hip_lab.h and every A/B / diagnostic environment switch
    "lab": Library("libwavjepa_hip_lab.so", SOURCES, ["-DWJ_LAB"], "obj_lab"),
}


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the HIP toolchain (ROCm) is required to build libwavjepa_hip.so")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(name: str = "release", force: bool = False, verbose: bool = True) -> str:
    """Compile and link one library of LIBRARIES; with the release library, libwavjepa_io.so too."""
    library = LIBRARIES[name]
    hipcc = _hipcc()
    objdir = os.path.join(LIBDIR, library.objdir)
    os.makedirs(objdir, exist_ok=True)
    inc = os.path.join(os.path.dirname(HERE), "include")
    headers = glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(inc, "*.h"))
    flags, lib, sources = FLAGS + library.flags, library.path, library.sources
    jobs = []
    for src in sources:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        if force or _stale(o, [s] + headers):
            jobs.append((s, o))

    def compile_one(job):
        s, o = job
        cmd = [hipcc] + flags + ["-c", s, "-o", o]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {s}:\n{r.stderr}")
        return s

    if jobs:
        with ThreadPoolExecutor(max_workers=min(4, len(jobs))) as ex:
            for s in ex.map(compile_one, jobs):
                if verbose:
                    print(f"[wavjepa_amd.build] compiled {os.path.basename(s)}", file=sys.stderr)
    objs = [os.path.join(objdir, s.replace(".hip", ".o")) for s in sources]
    if force or jobs or _stale(lib, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr}")
        if verbose:
            print(f"[wavjepa_amd.build] linked {lib}", file=sys.stderr)
    if name == "release":
        build_io(force=force, verbose=verbose)
    return lib


def build_all(force: bool = False, verbose: bool = True) -> None:
    """Every library (what __graft_entry__.build() and the test suite need)."""
    for name in LIBRARIES:
        build(name, force=force, verbose=verbose)


IO_LIB = os.path.join(LIBDIR, "libwavjepa_io.so")
IO_SOURCES = ["flac_decode.cpp"]


def build_io(force: bool = False, verbose: bool = True) -> str:
    """Host-side library of the data path (FLAC decoder): plain C++ with a C ABI, built with g++ (no GPU code)."""
    os.makedirs(LIBDIR, exist_ok=True)
    srcs = [os.path.join(CSRC, s) for s in IO_SOURCES]
    if force or _stale(IO_LIB, srcs):
        cxx = shutil.which("g++") or shutil.which("c++")
        if cxx is None:
            raise RuntimeError("g++ not found: needed for libwavjepa_io.so")
        r = subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", IO_LIB] + srcs, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"g++ failed for libwavjepa_io.so:\n{r.stderr}")
        if verbose:
            print(f"[wavjepa_amd.build] built {IO_LIB}", file=sys.stderr)
    return IO_LIB


if __name__ == "__main__":
    if "--release-only" in sys.argv:
        build(force="--force" in sys.argv)
    else:
        build_all(force="--force" in sys.argv)
