"""The shared libraries of the package, one case per row of wavjepa_amd._abi.LIBRARIES: the build table and the binding table list the
same libraries, every library exports exactly what its header(s) declare, and its own queries know its structs and refuse unknown
names.  None of this needs a GPU."""
import ctypes
import os
import subprocess

import pytest

from wavjepa_amd import _abi, build

SIDE = ("dropout", "monitor", "act", "optim")


@pytest.mark.parametrize("name", list(_abi.LIBRARIES))
def test_library_exports_what_its_headers_declare_and_answers_its_queries(name):
    assert list(build.LIBRARIES) == list(_abi.LIBRARIES) == ["release", *SIDE, "lab"]
    library = _abi.LIBRARIES[name]
    if not (os.environ.get("WAVJEPA_HIP_LIB") or os.environ.get("WAVJEPA_HIP_LAB_LIB")):      # (the overrides name A/B builds)
        assert library.path == build.LIBRARIES[name].path
    assert os.path.exists(library.path)
    out = subprocess.run(["nm", "-D", "--defined-only", library.path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T wj_" in ln}
    assert exported == set(library.functions), (sorted(exported - set(library.functions)), sorted(set(library.functions) - exported))
    if name in SIDE:                                          # -fvisibility=hidden: nothing but the header's functions, mangled names included
        assert {ln.split()[-1] for ln in out.splitlines() if " T " in ln} == exported
    assert {library.struct_size, library.workspace_bytes} <= set(library.functions)
    lib = _abi.load(name)
    assert _abi.loaded(name) and library.handle is lib
    struct_size, workspace_bytes = getattr(lib, library.struct_size), getattr(lib, library.workspace_bytes)
    assert library.struct_types
    for struct, cls in library.struct_types.items():
        assert struct_size(struct.encode()) == ctypes.sizeof(cls) > 0, struct
    assert struct_size(b"wj_no_such_struct") == -1 and struct_size(None) == -1
    zeroed = next(iter(library.struct_types.values()))()
    assert workspace_bytes(b"wj_no_such_entry", ctypes.byref(zeroed)) == -1 and workspace_bytes(None, ctypes.byref(zeroed)) == -1
    for fn, struct in library.entry_args.items():             # every stream entry is in the library's table and takes a struct of its header(s)
        assert fn in exported and struct in library.struct_types


def test_no_entry_belongs_to_two_libraries():
    """Release and the four side libraries share no function and no struct name; lab is the declared superset of release."""
    owners = {}
    for name in ("release", *SIDE):
        for what in (*_abi.LIBRARIES[name].functions, *_abi.LIBRARIES[name].struct_types):
            assert owners.setdefault(what, name) == name, (what, owners[what], name)
    release, lab = _abi.LIBRARIES["release"], _abi.LIBRARIES["lab"]
    assert set(release.functions) < set(lab.functions) and set(lab.functions) - set(release.functions) == set(_abi.LAB_FUNCTIONS)
    assert not set(_abi.LAB_FUNCTIONS) & set(owners)
    for fn, library in _abi._ENTRY_LIBRARY.items():          # what call() and workspace_bytes() look up
        assert library is _abi.LIBRARIES[owners.get(fn, "lab")], fn
    assert set(_abi._ENTRY_LIBRARY) == {fn for library in _abi.LIBRARIES.values() for fn in library.entry_args}
