"""The C-ABI library loads on a CPU-only host and exports every function include/*.h declares."""
import ctypes
import re
import shutil
import subprocess

from helpers import ROOT


def _declared(header_text):
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    text = re.sub(r"//.*", "", text)
    return sorted(set(re.findall(r"\b(lutldpc_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported():
    lib = ctypes.CDLL(str(ROOT / "lut_ldpc_amd" / "lib" / "liblut_ldpc_amd.so"))
    names = []
    for h in sorted((ROOT / "include").glob("*.h")):
        names += _declared(h.read_text())
    assert len(names) >= 15
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def _arities(header_text):
    """name -> number of parameters of every function a header declares ((void) counts as 0)."""
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    text = re.sub(r"//.*", "", text)
    return {name: 0 if args.strip() in ("", "void") else args.count(",") + 1 for name, args in re.findall(r"\b(lutldpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}


def test_every_declared_function_has_its_signature_in_capi(tmp_path):
    """_capi's one table binds every function of include/*.h with as many arguments as the header declares, and its structures have
    the size the C compiler gives the header's."""
    from lut_ldpc_amd import _capi
    want = {}
    for h in sorted((ROOT / "include").glob("*.h")):
        text = h.read_text()
        want.update(_arities(text))
        assert sorted(_arities(text)) == _declared(text), h.name
    unbound = [n for n in want if n not in _capi._SIGNATURES or getattr(_capi.lib, n).argtypes is None]
    assert not unbound, unbound
    wrong = {n: (len(getattr(_capi.lib, n).argtypes), k) for n, k in want.items() if len(getattr(_capi.lib, n).argtypes) != k}
    assert not wrong, f"(bound, declared) parameters: {wrong}"
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        return                                     # (no system compiler: the arities above are what could be checked)
    structs = {"lutldpc_channel_cells": _capi.ChannelCells, "lutldpc_event_request": _capi.EventRequest, "lutldpc_packed_io": _capi.PackedIO,
               "lutldpc_llr_io": _capi.LlrIO, "lutldpc_encode_io": _capi.EncodeIO}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lut_ldpc_hip.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in structs) + "    return 0;\n}\n")
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(tmp_path / "sizes")], check=True)
    out = subprocess.run([str(tmp_path / "sizes")], check=True, capture_output=True, text=True).stdout
    sizes = {n: int(v) for n, v in (ln.split() for ln in out.splitlines())}
    assert sizes == {n: ctypes.sizeof(t) for n, t in structs.items()}


def test_cells_of_a_caller_that_declares_the_struct_itself_are_accepted():
    """Callers older than _capi.ChannelCells pass byref() of their own struct to the entries that take a cell table: the same field
    types are taken as a ChannelCells in place, anything else is refused before the library sees it."""
    import numpy as np
    import pytest
    from lut_ldpc_amd import _capi
    own = type("Cells", (ctypes.Structure,), {"_fields_": [("n", f[1]) if i == 0 else f for i, f in enumerate(_capi.ChannelCells._fields_)]})
    other = type("Other", (ctypes.Structure,), {"_fields_": _capi.ChannelCells._fields_[:-1]})
    thr, lab, stats = np.array([1 << 63], np.uint64), np.array([0, 1], np.uint8), np.zeros((3, 4), np.int32)
    lp = lab.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    cells = own(2, thr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), lp, lp, lp, lp, lp)
    seen = _capi._ccp.from_param(ctypes.byref(cells))._obj
    assert isinstance(seen, _capi.ChannelCells) and ctypes.addressof(seen) == ctypes.addressof(cells) and seen.n_cells == 2
    sp = stats.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    for name in ("lutldpc_decoder_sim_batch", "lutldpc_decoder_sim_batch_random", "lutldpc_decoder_sample_labels", "lutldpc_decoder_sim_batch_histogram",
                 "lutldpc_decoder_sim_batch_events"):
        assert _capi._SIGNATURES[name][1][1] is _capi._ccp and issubclass(_capi._ccp, ctypes.POINTER(_capi.ChannelCells))
    assert _capi.lib.lutldpc_decoder_sim_batch_random(None, ctypes.byref(cells), 7, 1, 0, 3, 1, sp, None, None) == _capi.ERR_ARG      # NULL handle: reached the guard
    for bad in (ctypes.byref(other()), ctypes.byref(ctypes.c_int32(2))):
        with pytest.raises(ctypes.ArgumentError):
            _capi.lib.lutldpc_decoder_sim_batch_random(None, bad, 7, 1, 0, 3, 1, sp, None, None)


def test_version_and_device_count_without_gpu():
    import lut_ldpc_amd as L
    from lut_ldpc_amd._capi import lib
    assert b"gfx950" in lib.lutldpc_version()
    assert L.device_count() >= 0


def test_shipped_library_is_newer_than_its_sources():
    """lut_ldpc_amd/lib/ is git-ignored and travels to the GPU box as a prebuilt binary: a stale build must not ship."""
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    lib = root / "lut_ldpc_amd" / "lib" / "liblut_ldpc_amd.so"
    srcs = [p for p in (root / "lut_ldpc_amd" / "csrc").rglob("*") if p.suffix in (".hip", ".hpp", ".cpp", ".h")] + list((root / "include").glob("*.h"))
    assert srcs
    newer = [str(p.relative_to(root)) for p in srcs if p.stat().st_mtime > lib.stat().st_mtime]
    assert not newer, f"rebuild (make -C lut_ldpc_amd/csrc): newer than the library: {newer}"
