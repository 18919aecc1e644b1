"""The packed root rows of a balanced variable tree (lut_program.hpp: pack_root_rows; decoder_setup.hip: add_root_rows), without
a GPU.  On nibble rows the compile-time variable kernels of degree >= 3 read ROOT[. | ch << shr] as one 64-bit word per frame and
shift it by 4 x the label of the tree's top inner node, so the table blob holds, per class, 16 packed rows and that node's table
times 4.  No accessor of a host-only handle reaches the blob: tests/root_rows_check.cpp calls the packer itself, as a stand-alone
program built with AddressSanitizer and UBSan, on random tables with alphabets of 2, 4, 8 and 16 labels on either input and on the
variable trees of designed codes; describe() of a host-only handle says where the form is in force."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

from helpers import oracle_codec, product_decoder

HERE = Path(__file__).resolve().parent
HIP = HERE.parent / "lut_ldpc_amd" / "csrc" / "hip"
CLANG = Path("/opt/rocm/lib/llvm/bin/clang++")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/root_rows_check.cpp, host code only, under ASan + UBSan."""
    cxx = str(CLANG) if CLANG.exists() else shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("root_rows") / "root_rows_check"
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        f"-I{HIP}", str(HERE / "root_rows_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(exe, *args):
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_random_tables_of_every_alphabet_pair(checker):
    """4 x 4 x 4 alphabets (top inner node, channel, root output) x 4 tables: all 256 (ch, top) positions of each against the byte
    table, absent labels 0, the scaled top table 4 x the original, and tables outside the form refused."""
    out = _run(checker, "random")
    assert f"{4 * 4 * 4 * 4 * 256} nibbles checked" in out, out


# designed codes: every variable degree of the irregular N = 500 code (2 .. 17) and of DVB-S2 (1, 2, 3, 8), message alphabets that
# change between iterations (8, 4, 2 labels: rows of 8, 4 and 2 nibbles), a 2-label channel and a 4-label one
DESIGNED = ["n500_q4_i8", "dvbs2_q4_i6", "n500_ex8421", "reg36_n1000_grow", "reg36_n1000_c2m4", "reg36_n1000_c4m4"]


@pytest.mark.parametrize("name", DESIGNED)
def test_designed_trees(name, checker, tmp_path):
    cd = oracle_codec(name)
    path = tmp_path / "var_trees.txt"
    path.write_text(cd.var_tree_txt)
    out = _run(checker, "trees", str(path))
    degs = [d for d in sorted(set(cd.code.dv.tolist())) if d >= 3]
    n_var_sets = cd.n_sets() - 1                               # the last set decides
    assert f"trees: {len(degs) * n_var_sets} classes" in out, (out, degs, n_var_sets)


@pytest.mark.parametrize("name,pack", [("n500_q4_i8", None), ("n500_q4_i8", "1"), ("dvbs2_q4_i6", None), ("reg36_n1000_q5", None), ("reg36_n1000_rootonly", None)])
def test_describe_reports_the_form(name, pack, monkeypatch):
    """root_rows per variable class: 1 exactly where the compile-time kernel runs a class of degree >= 3 on nibble rows -- not on byte
    rows (the knob, or 32 labels), and not where the tree is not the balanced one (root_only: a generated kernel)."""
    for k in [k for k in os.environ if k.startswith("LUTLDPC_") and k not in ("LUTLDPC_LIB", "LUTLDPC_DESIGN_CACHE")]:
        monkeypatch.delenv(k)
    if pack:
        monkeypatch.setenv("LUTLDPC_PACK", pack)
    dec = product_decoder(oracle_codec(name), device=-1)
    desc = dec.describe()
    assert desc["pack"] == (1 if pack or name == "reg36_n1000_q5" else 2), desc
    for c in desc["vn_classes"]:
        want = int(desc["pack"] == 2 and c["deg"] >= 3 and c["kernel"] == "vn_balanced_fast_kernel")
        assert c["root_rows"] == want, (c, desc)
    if name in ("n500_q4_i8", "dvbs2_q4_i6") and not pack:
        assert sum(c["root_rows"] for c in desc["vn_classes"]) == sum(c["deg"] >= 3 for c in desc["vn_classes"]) > 0, desc
    else:
        assert not any(c["root_rows"] for c in desc["vn_classes"]), desc
    dec.close()
