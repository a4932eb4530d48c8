"""ctypes binding of libwavjepa_hip.so.

The argument structs are generated from `include/wavjepa_hip.h` itself (a tiny parser for its plain-C struct
syntax), so the Python mirror cannot drift from the header; sizes are cross-checked against the library's own
`wj_struct_size`.  There is NO fallback: if the shared library is missing or a symbol is absent, importing the
product path fails loudly.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import Dict, List, Tuple

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "wavjepa_hip.h")
LAB_HEADER = os.path.join(os.path.dirname(HERE), "include", "wavjepa_hip_lab.h")
DROPOUT_HEADER = os.path.join(os.path.dirname(HERE), "include", "wavjepa_hip_dropout.h")
LIB_PATH = os.environ.get("WAVJEPA_HIP_LIB") or os.path.join(HERE, "lib", "libwavjepa_hip.so")   # override: A/B and ablation builds
# the laboratory build of the same sources (-DWJ_LAB): extra diagnostic entries + every A/B switch; loaded only by load_lab()
LAB_LIB_PATH = os.environ.get("WAVJEPA_HIP_LAB_LIB") or os.path.join(HERE, "lib", "libwavjepa_hip_lab.so")
# the dropout forms of the LayerNorm / streamed-attention kernels and wj_dropout_rows (include/wavjepa_hip_dropout.h); loaded by load_dropout()
DROPOUT_LIB_PATH = os.path.join(HERE, "lib", "libwavjepa_hip_dropout.so")

_SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "int": ctypes.c_int,
            "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}


class WavJepaHipError(RuntimeError):
    pass


def _strip_comments(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


class Header:
    """What the binding needs of one header: {struct: [(field, ctype)]}, {function: (restype, [argtypes])} in declaration order,
    {stream entry `int f(const S*, void* stream)`: S}, {enum constant: value} and the integer `#define WJ_x value` constants."""

    def __init__(self, path: str, known: "Header" = None):
        """known: the header this one includes (its structs may be embedded by value)"""
        text = _strip_comments(open(path).read())
        self.defines = {k: int(v, 0) for k, v in re.findall(r"^\s*#\s*define\s+(WJ_\w+)\s+(-?(?:0x[0-9a-fA-F]+|\d+))\s*$", text, flags=re.M)}
        self.structs: Dict[str, List[Tuple[str, object]]] = {}
        self.struct_types: Dict[str, type] = {}      # the ctypes classes, in declaration order: a later struct may embed an earlier one by value
        earlier = dict(known.struct_types) if known is not None else {}
        for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
            fields: List[Tuple[str, object]] = []
            for decl in body.split(";"):
                decl = decl.strip()
                if not decl:
                    continue
                is_ptr = "*" in decl
                toks = decl.replace("*", " * ").split()
                toks = [t for t in toks if t != "const"]
                base = toks[0]
                names = "".join(toks[1:]).replace("*", "").split(",")
                for n in names:
                    n = n.strip()
                    if not n:
                        continue
                    ctype = ctypes.c_void_p if is_ptr else ({**earlier, **self.struct_types}[base] if base in earlier or base in self.struct_types else _SCALARS[base])
                    arr = re.match(r"(\w+)\[(\w+)\]$", n)          # fixed-size array member: name[N] (N a number or a #define)
                    if arr:
                        n, dim = arr.group(1), arr.group(2)
                        ctype = ctype * (int(dim) if dim.isdigit() else self.defines[dim])
                    fields.append((n, ctype))
            self.structs[name] = fields
            self.struct_types[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
        self.functions: Dict[str, Tuple[object, list]] = {}
        self.entry_args: Dict[str, str] = {}
        for ret, name, params in re.findall(r"\b(int|int64_t)\s+(wj_\w+)\s*\(([^)]*)\)\s*;", text):
            params = [" ".join(p.replace("*", " * ").split()) for p in params.split(",") if p.strip() != "void"]
            self.functions[name] = (_SCALARS[ret], [_param_ctype(p) for p in params])
            entry = re.fullmatch(r"const (wj_\w+) \*", params[0]) if len(params) == 2 and params[1] == "void * stream" else None
            if entry:
                self.entry_args[name] = entry.group(1)
        self.enums: Dict[str, int] = {}
        for body in re.findall(r"enum\s*\{(.*?)\}\s*;", text, flags=re.S):
            val = -1
            for item in filter(None, map(str.strip, body.split(","))):
                k, _, v = item.partition("=")
                val = int(v.strip(), 0) if v else val + 1
                self.enums[k.strip()] = val


def _param_ctype(param: str):
    """ctypes type of one prototype parameter: `const char*` is a string, any other pointer an address, the rest a scalar."""
    if "*" in param:
        return ctypes.c_char_p if param.startswith("const char *") else ctypes.c_void_p
    return _SCALARS[param.split()[0]]


_HEADER, _LAB = Header(HEADER), Header(LAB_HEADER)
_STRUCT_FIELDS, ENUMS, DEFINES = _HEADER.structs, _HEADER.enums, _HEADER.defines
FUNCTIONS, LAB_FUNCTIONS = list(_HEADER.functions), list(_LAB.functions)
_PROTOTYPES = {**_HEADER.functions, **_LAB.functions}            # name -> (restype, argtypes)
ENTRY_ARGS = {**_HEADER.entry_args, **_LAB.entry_args}           # stream entry -> its argument struct


STRUCTS, LAB_STRUCTS = _HEADER.struct_types, _LAB.struct_types
# libwavjepa_hip_dropout.so: a header, a function list and an entry map of its own -- what describes libwavjepa_hip.so above is unchanged
_DROP = Header(DROPOUT_HEADER, known=_HEADER)
DROPOUT_STRUCTS, DROPOUT_FUNCTIONS, DROPOUT_ENTRY_ARGS = _DROP.struct_types, list(_DROP.functions), dict(_DROP.entry_args)

# libwavjepa_hip_monitor.so (wj_masked_moments, the collapse monitor): likewise a header, a function list and an entry map of its own
MONITOR_HEADER = os.path.join(os.path.dirname(HERE), "include", "wavjepa_hip_monitor.h")
MONITOR_LIB_PATH = os.path.join(HERE, "lib", "libwavjepa_hip_monitor.so")
_MON = Header(MONITOR_HEADER, known=_HEADER)
MONITOR_STRUCTS, MONITOR_FUNCTIONS, MONITOR_ENTRY_ARGS, MONITOR_DEFINES = _MON.struct_types, list(_MON.functions), dict(_MON.entry_args), _MON.defines

# libwavjepa_hip_act.so (wj_gemm_bf16_act: linear1's forward GEMM with the activation chosen per call): likewise
ACT_HEADER = os.path.join(os.path.dirname(HERE), "include", "wavjepa_hip_act.h")
ACT_LIB_PATH = os.path.join(HERE, "lib", "libwavjepa_hip_act.so")
_ACT = Header(ACT_HEADER, known=_HEADER)
ACT_STRUCTS, ACT_FUNCTIONS, ACT_ENTRY_ARGS, ACT_ENUMS = _ACT.struct_types, list(_ACT.functions), dict(_ACT.entry_args), _ACT.enums

# libwavjepa_hip_optim.so (wj_adamw_groups_step: the AdamW pass with parameter groups): likewise
OPTIM_HEADER = os.path.join(os.path.dirname(HERE), "include", "wavjepa_hip_optim.h")
OPTIM_LIB_PATH = os.path.join(HERE, "lib", "libwavjepa_hip_optim.so")
_OPT = Header(OPTIM_HEADER, known=_HEADER)
OPTIM_STRUCTS, OPTIM_FUNCTIONS, OPTIM_ENTRY_ARGS, OPTIM_DEFINES = _OPT.struct_types, list(_OPT.functions), dict(_OPT.entry_args), _OPT.defines

_lib = None
_lab_lib = None
_dropout_lib = None
_monitor_lib = None
_act_lib = None
_optim_lib = None


def optim_loaded() -> bool:
    """True once libwavjepa_hip_optim.so is in the process (an optimiser with one parameter group never loads it)."""
    return _optim_lib is not None


def load_optim():
    """libwavjepa_hip_optim.so (once), its struct sizes cross-checked against its own wj_optim_struct_size.  Loaded behind the release
    library, as load_dropout() does."""
    global _optim_lib
    if _optim_lib is None:
        load()
        if not os.path.exists(OPTIM_LIB_PATH):
            raise WavJepaHipError(f"{OPTIM_LIB_PATH} is missing: run `python -m wavjepa_amd.build` (or __graft_entry__.build())")
        lib = ctypes.CDLL(OPTIM_LIB_PATH)
        for fn in OPTIM_FUNCTIONS:
            if not hasattr(lib, fn):
                raise WavJepaHipError(f"{OPTIM_LIB_PATH} does not export {fn} (declared in include/wavjepa_hip_optim.h); rebuild it")
            f = getattr(lib, fn)
            f.restype, f.argtypes = _OPT.functions[fn]
        for name, cls in OPTIM_STRUCTS.items():
            want = lib.wj_optim_struct_size(name.encode())
            if want != ctypes.sizeof(cls):
                raise WavJepaHipError(f"struct {name}: header mirror is {ctypes.sizeof(cls)} bytes, library says {want}")
        _optim_lib = lib
    return _optim_lib


def act_loaded() -> bool:
    """True once libwavjepa_hip_act.so is in the process (a model whose stacks all run GELU never loads it)."""
    return _act_lib is not None


def load_act():
    """libwavjepa_hip_act.so (once), its struct sizes cross-checked against its own wj_act_struct_size.  Loaded behind the release
    library, as load_dropout() does."""
    global _act_lib
    if _act_lib is None:
        load()
        if not os.path.exists(ACT_LIB_PATH):
            raise WavJepaHipError(f"{ACT_LIB_PATH} is missing: run `python -m wavjepa_amd.build` (or __graft_entry__.build())")
        lib = ctypes.CDLL(ACT_LIB_PATH)
        for fn in ACT_FUNCTIONS:
            if not hasattr(lib, fn):
                raise WavJepaHipError(f"{ACT_LIB_PATH} does not export {fn} (declared in include/wavjepa_hip_act.h); rebuild it")
            f = getattr(lib, fn)
            f.restype, f.argtypes = _ACT.functions[fn]
        for name, cls in ACT_STRUCTS.items():
            want = lib.wj_act_struct_size(name.encode())
            if want != ctypes.sizeof(cls):
                raise WavJepaHipError(f"struct {name}: header mirror is {ctypes.sizeof(cls)} bytes, library says {want}")
        _act_lib = lib
    return _act_lib


def load_monitor():
    """libwavjepa_hip_monitor.so (once), its struct sizes cross-checked against its own wj_monitor_struct_size.  Loaded behind the release
    library, as load_dropout() does."""
    global _monitor_lib
    if _monitor_lib is None:
        load()
        if not os.path.exists(MONITOR_LIB_PATH):
            raise WavJepaHipError(f"{MONITOR_LIB_PATH} is missing: run `python -m wavjepa_amd.build` (or __graft_entry__.build())")
        lib = ctypes.CDLL(MONITOR_LIB_PATH)
        for fn in MONITOR_FUNCTIONS:
            if not hasattr(lib, fn):
                raise WavJepaHipError(f"{MONITOR_LIB_PATH} does not export {fn} (declared in include/wavjepa_hip_monitor.h); rebuild it")
            f = getattr(lib, fn)
            f.restype, f.argtypes = _MON.functions[fn]
        for name, cls in MONITOR_STRUCTS.items():
            want = lib.wj_monitor_struct_size(name.encode())
            if want != ctypes.sizeof(cls):
                raise WavJepaHipError(f"struct {name}: header mirror is {ctypes.sizeof(cls)} bytes, library says {want}")
        _monitor_lib = lib
    return _monitor_lib


def load_dropout():
    """libwavjepa_hip_dropout.so (once), its struct sizes cross-checked against its own wj_dropout_struct_size.  Loaded behind the release
    library, so that both bind to the HIP runtime torch brought."""
    global _dropout_lib
    if _dropout_lib is None:
        load()
        if not os.path.exists(DROPOUT_LIB_PATH):
            raise WavJepaHipError(f"{DROPOUT_LIB_PATH} is missing: run `python -m wavjepa_amd.build` (or __graft_entry__.build())")
        lib = ctypes.CDLL(DROPOUT_LIB_PATH)
        for fn in DROPOUT_FUNCTIONS:
            if not hasattr(lib, fn):
                raise WavJepaHipError(f"{DROPOUT_LIB_PATH} does not export {fn} (declared in include/wavjepa_hip_dropout.h); rebuild it")
            f = getattr(lib, fn)
            f.restype, f.argtypes = _DROP.functions[fn]
        for name, cls in DROPOUT_STRUCTS.items():
            want = lib.wj_dropout_struct_size(name.encode())
            if want != ctypes.sizeof(cls):
                raise WavJepaHipError(f"struct {name}: header mirror is {ctypes.sizeof(cls)} bytes, library says {want}")
        _dropout_lib = lib
    return _dropout_lib


def lib_path() -> str:
    return LIB_PATH


def load_lab():
    """The laboratory library (include/wavjepa_hip_lab.h): the release entries plus the diagnostic ones.  Used by tools/, the all-reduce
    rehearsal (bench.py --emulate-allreduce) and the tests that dissect a kernel; never by the training / inference path."""
    global _lab_lib
    if _lab_lib is None:
        _lab_lib = _load(LAB_LIB_PATH, FUNCTIONS + LAB_FUNCTIONS, {**STRUCTS, **LAB_STRUCTS})
    return _lab_lib


def load():
    """Load the library (once).  Raises WavJepaHipError when it is not built."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH, FUNCTIONS, STRUCTS)
    return _lib


def _load(LIB_PATH: str, FUNCTIONS, STRUCTS):
    if not os.path.exists(LIB_PATH):
        raise WavJepaHipError(
            f"{LIB_PATH} is missing: the HIP extension is not built. Run `python -m wavjepa_amd.build` "
            "(or __graft_entry__.build()). wavjepa_amd has no CPU/PyTorch fallback by design.")
    # PyTorch-ROCm ships its own libamdhip64; the library must bind to THAT runtime (the one that owns the tensors and streams
    # it is handed), so torch is loaded first and the dynamic linker resolves our libamdhip64 dependency to the copy already
    # in the process.  Loaded the other way round there are two HIP runtimes and the first launch fails with "no ROCm-capable
    # device is detected".
    import torch  # noqa: F401
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise WavJepaHipError(f"cannot load {LIB_PATH}: {e}") from e
    for fn in FUNCTIONS:
        if not hasattr(lib, fn):
            raise WavJepaHipError(f"{LIB_PATH} does not export {fn} (declared in include/wavjepa_hip.h); rebuild it")
        f = getattr(lib, fn)
        f.restype, f.argtypes = _PROTOTYPES[fn]
    if lib.wj_abi_version() != DEFINES["WJ_ABI_VERSION"]:
        raise WavJepaHipError(f"{LIB_PATH} reports ABI version {lib.wj_abi_version()}, include/wavjepa_hip.h declares "
                              f"{DEFINES['WJ_ABI_VERSION']}: stale library, rebuild it (python -m wavjepa_amd.build)")
    for name, cls in STRUCTS.items():
        want = lib.wj_struct_size(name.encode())
        if want != ctypes.sizeof(cls):
            raise WavJepaHipError(f"struct {name}: header mirror is {ctypes.sizeof(cls)} bytes, library says {want}")
    return lib


def workspace_bytes(fn_name: str, args_struct) -> int:
    """Scratch bytes the call `fn_name(args_struct)` needs (pointers in the struct are ignored)."""
    if fn_name in DROPOUT_ENTRY_ARGS:
        n = int(load_dropout().wj_dropout_workspace_bytes(fn_name.encode(), ctypes.byref(args_struct)))
    elif fn_name in MONITOR_ENTRY_ARGS:
        n = int(load_monitor().wj_monitor_workspace_bytes(fn_name.encode(), ctypes.byref(args_struct)))
    elif fn_name in ACT_ENTRY_ARGS:
        n = int(load_act().wj_act_workspace_bytes(fn_name.encode(), ctypes.byref(args_struct)))
    elif fn_name in OPTIM_ENTRY_ARGS:
        n = int(load_optim().wj_optim_workspace_bytes(fn_name.encode(), ctypes.byref(args_struct)))
    else:
        n = int(load().wj_workspace_bytes(fn_name.encode(), ctypes.byref(args_struct)))
    if n < 0:
        raise WavJepaHipError(f"wj_workspace_bytes: unknown entry point {fn_name}")
    return n


_ERR = {-1: "invalid argument", -2: "kernel launch failed", -3: "unsupported configuration"}


def call(fn_name: str, args_struct, stream: int, lab: bool = False) -> None:
    if fn_name in ACT_ENTRY_ARGS:
        lib = load_act()
    elif fn_name in OPTIM_ENTRY_ARGS:
        lib = load_optim()
    else:
        lib = load_dropout() if fn_name in DROPOUT_ENTRY_ARGS else (load_monitor() if fn_name in MONITOR_ENTRY_ARGS else (load_lab() if lab else load()))
    rc = getattr(lib, fn_name)(ctypes.byref(args_struct), stream)
    if rc != 0:
        raise WavJepaHipError(f"{fn_name} failed: {_ERR.get(rc, rc)}")
