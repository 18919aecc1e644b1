"""The boundary arrays of lutldpc_decoder_decode_llr_batch, without a GPU.  The entry quantises as quant_nonlin does -- the label of x
is the number of LEADING boundaries below it, on any array, sorted or not, NaN included -- through the one device quantiser, which
counts all boundaries below x and needs them non-decreasing.  leading_count_bounds (llr_cells.hpp) brings an array into that form;
tests/llr_cells_check.cpp holds it and llr_cell_table against the reference loop, as a stand-alone program built with
AddressSanitizer and UBSan (tests/test_57_llr_input_gpu.py decodes through it on the device)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
HIP = HERE.parent / "lut_ldpc_amd" / "csrc" / "hip"
CLANG = Path("/opt/rocm/lib/llvm/bin/clang++")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/llr_cells_check.cpp, host code only, under ASan + UBSan."""
    cxx = str(CLANG) if CLANG.exists() else shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("llr_cells") / "llr_cells_check"
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        f"-I{HIP}", str(HERE / "llr_cells_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_leading_count_on_any_boundary_array(checker):
    """4000 seeded pairs of arrays (1..31 boundaries; +-inf, NaN, +-0, repeats, descending runs), every boundary and its float64
    neighbours, NaN, +-inf and +-0 as values: the reference loop = the plain count over the normalised array = the labels of the
    value's cell in both modes; non-decreasing arrays come back unchanged; llr_cell_table keeps its own refusals."""
    r = subprocess.run([str(checker), "4000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), (r.stdout[-3000:], r.stderr[-3000:])
    m = re.search(r"4000 arrays \((\d+) unsorted, (\d+) with NaN\), (\d+) values checked", r.stdout)
    assert m and int(m.group(1)) > 2000 and int(m.group(2)) > 1000 and int(m.group(3)) > 4000 * 20, r.stdout
