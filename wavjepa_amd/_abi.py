"""ctypes binding of libwavjepa_hip.so and of the libraries beside it (LIBRARIES: one row each).

The argument structs are generated from the headers under `include/` themselves (a tiny parser for their plain-C struct
syntax), so the Python mirror cannot drift from a header; sizes are cross-checked against each library's own
struct-size query.  There is NO fallback: if a shared library is missing or a symbol is absent, the first use of the
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
LIB_PATH = os.environ.get("WAVJEPA_HIP_LIB") or os.path.join(HERE, "lib", "libwavjepa_hip.so")   # override: A/B and ablation builds
# the laboratory build of the same sources (-DWJ_LAB): extra diagnostic entries + every A/B switch; loaded only by load("lab")
LAB_LIB_PATH = os.environ.get("WAVJEPA_HIP_LAB_LIB") or os.path.join(HERE, "lib", "libwavjepa_hip_lab.so")

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
        self.path = path
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


class Library:
    """One shared library of the package: what its header(s) declare (several headers: the union, in order), its file, the names of its
    two query entries and, once load() has bound it, its handle."""

    def __init__(self, headers: List[Header], path: str, struct_size: str = "wj_struct_size", workspace_bytes: str = "wj_workspace_bytes"):
        self.headers, self.path, self.struct_size, self.workspace_bytes = headers, path, struct_size, workspace_bytes
        self.handle = None
        for what in ("struct_types", "functions", "entry_args", "enums", "defines"):
            setattr(self, what, {k: v for h in headers for k, v in getattr(h, what).items()})


def _side(name: str) -> Library:
    """A side library: include/wavjepa_hip_<name>.h (which may embed the release header's structs), lib/libwavjepa_hip_<name>.so,
    wj_<name>_struct_size and wj_<name>_workspace_bytes.  It declares no wj_abi_version: a header, a function list and an entry map of
    its own, and what describes libwavjepa_hip.so is unchanged by it."""
    return Library([Header(os.path.join(os.path.dirname(HEADER), f"wavjepa_hip_{name}.h"), known=_HEADER)],
                   os.path.join(HERE, "lib", f"libwavjepa_hip_{name}.so"), f"wj_{name}_struct_size", f"wj_{name}_workspace_bytes")


# Every shared library, keyed as in wavjepa_amd.build.LIBRARIES; headers are parsed here, a .so is loaded on first use only.
LIBRARIES = {
    "release": Library([_HEADER], LIB_PATH),
    "dropout": _side("dropout"),     # the dropout forms of the LayerNorm / streamed-attention kernels and wj_dropout_rows
    "monitor": _side("monitor"),     # wj_masked_moments, the collapse monitor
    "act": _side("act"),             # wj_gemm_bf16_act: linear1's forward GEMM with the activation chosen per call
    "optim": _side("optim"),         # wj_adamw_groups_step: the AdamW pass with parameter groups
    # the release entries plus the diagnostic ones.  Used by tools/, the all-reduce rehearsal (bench.py --emulate-allreduce) and the
    # tests that dissect a kernel; never by the training / inference path
    "lab": Library([_HEADER, _LAB], LAB_LIB_PATH),
}
_RELEASE, _LAB_LIBRARY = LIBRARIES["release"], LIBRARIES["lab"]
# stream entry -> the library that has it (an entry of the release header: the release library, not lab)
_ENTRY_LIBRARY = {fn: library for library in reversed(list(LIBRARIES.values())) for fn in library.entry_args}

_STRUCT_FIELDS, ENUMS, DEFINES = _HEADER.structs, _HEADER.enums, _HEADER.defines
STRUCTS, LAB_STRUCTS = _HEADER.struct_types, _LAB.struct_types
FUNCTIONS, LAB_FUNCTIONS = list(_HEADER.functions), list(_LAB.functions)
ENTRY_ARGS = _LAB_LIBRARY.entry_args                             # stream entry -> its argument struct, release and lab


def loaded(name: str) -> bool:
    """True once that library is in the process (a model whose stacks all run GELU never loads "act", an optimiser with one parameter
    group never loads "optim")."""
    return LIBRARIES[name].handle is not None


def load(name: str = "release"):
    """The handle of a library of LIBRARIES, loaded and checked on first use.  Raises WavJepaHipError when it is not built."""
    library = LIBRARIES[name]
    return library.handle or _bind(library)


def _bind(library: Library):
    path = library.path
    if "wj_abi_version" not in library.functions:
        load()          # a side library goes behind the release library, so that both bind to the HIP runtime torch brought
    if not os.path.exists(path):
        raise WavJepaHipError(
            f"{path} is missing: the HIP extension is not built. Run `python -m wavjepa_amd.build` "
            "(or __graft_entry__.build()). wavjepa_amd has no CPU/PyTorch fallback by design.")
    # PyTorch-ROCm ships its own libamdhip64; the library must bind to THAT runtime (the one that owns the tensors and streams
    # it is handed), so torch is loaded first and the dynamic linker resolves our libamdhip64 dependency to the copy already
    # in the process.  Loaded the other way round there are two HIP runtimes and the first launch fails with "no ROCm-capable
    # device is detected".
    import torch  # noqa: F401
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:  # pragma: no cover
        raise WavJepaHipError(f"cannot load {path}: {e}") from e
    for header in library.headers:
        for fn, prototype in header.functions.items():
            if not hasattr(lib, fn):
                raise WavJepaHipError(f"{path} does not export {fn} (declared in include/{os.path.basename(header.path)}); rebuild it")
            f = getattr(lib, fn)
            f.restype, f.argtypes = prototype
    if "wj_abi_version" in library.functions and lib.wj_abi_version() != DEFINES["WJ_ABI_VERSION"]:
        raise WavJepaHipError(f"{path} reports ABI version {lib.wj_abi_version()}, include/wavjepa_hip.h declares "
                              f"{DEFINES['WJ_ABI_VERSION']}: stale library, rebuild it (python -m wavjepa_amd.build)")
    struct_size = getattr(lib, library.struct_size)
    for name, cls in library.struct_types.items():
        want = struct_size(name.encode())
        if want != ctypes.sizeof(cls):
            raise WavJepaHipError(f"struct {name}: header mirror is {ctypes.sizeof(cls)} bytes, library says {want}")
    library.handle = lib
    return lib


def workspace_bytes(fn_name: str, args_struct) -> int:
    """Scratch bytes the call `fn_name(args_struct)` needs (pointers in the struct are ignored), from the library that has the entry."""
    library = _ENTRY_LIBRARY.get(fn_name, _RELEASE)
    n = int(getattr(library.handle or _bind(library), library.workspace_bytes)(fn_name.encode(), ctypes.byref(args_struct)))
    if n < 0:
        raise WavJepaHipError(f"wj_workspace_bytes: unknown entry point {fn_name}")
    return n


_ERR = {-1: "invalid argument", -2: "kernel launch failed", -3: "unsupported configuration"}


def call(fn_name: str, args_struct, stream: int, lab: bool = False) -> None:
    library = _LAB_LIBRARY if lab else _ENTRY_LIBRARY.get(fn_name, _RELEASE)
    rc = getattr(library.handle or _bind(library), fn_name)(ctypes.byref(args_struct), stream)
    if rc != 0:
        raise WavJepaHipError(f"{fn_name} failed: {_ERR.get(rc, rc)}")
