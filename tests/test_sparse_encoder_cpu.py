"""The sparse triangular encoder without a GPU: the sparse form of LDPC_Generator_Systematic against the dense form and against numpy
(same graph, same codewords), DVB-S2 itself on the host, the twin code that has no such form, codec files of both forms, the refusals
of lutldpc_decoder_set_sparse_generator on a host-only handle (argument errors before the state error; nothing changes), and the
cases of tests/sparse_encode_cases.py held to what they claim."""
import ctypes as C
import re

import numpy as np
import pytest

import encode_cases as ec
import frontend_cases as fc
import sparse_encode_cases as sc
from helpers import CODES, ROOT, product_decoder
from lut_ldpc_amd import _capi
from lut_ldpc_amd._capi import ERR_ARG, ERR_STATE, LutLdpcError, last_error, lib


@pytest.fixture(scope="module")
def alists(tmp_path_factory):
    d = tmp_path_factory.mktemp("sparse_codes")
    return lambda name: sc.zigzag_alist(name, d)


def _graph(pcd):
    return (pcd.nvar, pcd.nchk) + tuple(pcd.graph())


def test_symbol_is_declared_exported_and_bound():
    header = (ROOT / "include" / "lut_ldpc_hip.h").read_text()
    assert re.search(r"int lutldpc_decoder_set_sparse_generator\(lutldpc_decoder \*d, int K, int R, const int32_t \*row_ptr[^,]*, const int32_t \*cols\);", header)
    fn = lib.lutldpc_decoder_set_sparse_generator                  # (AttributeError if the library does not export it)
    assert "lutldpc_decoder_set_sparse_generator" in _capi._SIGNATURES and fn.restype is C.c_int and len(fn.argtypes) == 5


@pytest.mark.parametrize("name", list(sc.ZIGZAG_CODES))
def test_sparse_and_dense_host_forms_give_the_same_graph_and_the_same_codewords(name, alists):
    import lut_ldpc_amd as L
    path, N, M = alists(name)
    dense = L.Codec(path, with_generator=1, device=-1)
    sparse = L.Codec(path, with_generator="sparse", device=-1)
    K = N - M
    assert (dense.nvar, dense.ninfo, dense.rank) == (sparse.nvar, sparse.ninfo, sparse.rank) == (N, K, M)
    gd, gs = _graph(dense), _graph(sparse)
    assert all((a == b).all() if isinstance(a, np.ndarray) else a == b for a, b in zip(gd, gs))
    H = ec.parity_check_matrix(*gs)
    A = ec.systematic_rows(H, K)
    row_ptr, cols, peeled = sc.peel(H, K)
    assert peeled == M
    u = np.random.default_rng(N).integers(0, 2, (64, K)).astype(np.uint8)
    want = fc.encode(A, u).astype(np.uint8)
    assert (sc.forward_substitute(K, M, row_ptr, cols, u) == want).all()          # the two numpy statements agree
    for i in range(64):
        cd, cs = dense.encode(u[i]), sparse.encode(u[i])
        assert (cd == want[i]).all() and (cs == want[i]).all(), i
    assert want[:, K:].any() and not ((want.astype(np.int64) @ H.T.astype(np.int64)) % 2).any()
    dense.close()
    sparse.close()


@pytest.fixture(scope="module")
def dvbs2():
    import lut_ldpc_amd as L
    pcd = L.Codec(CODES / f"{sc.DVBS2}.alist", with_generator=True, known_rank=32400, device=-1)
    yield pcd
    pcd.close()


def test_dvbs2_is_encoded_on_the_host_through_its_sparse_form(dvbs2):
    N, K = 64800, 32400
    assert (dvbs2.nvar, dvbs2.ninfo, dvbs2.rank, dvbs2.nchk) == (N, K, 32400, 32400)
    dv, dc, cn = dvbs2.graph()
    var_of_edge = np.repeat(np.arange(N), dv)
    chk_of_slot = np.repeat(np.arange(dvbs2.nchk), dc)
    chk_vars = var_of_edge[cn]                                       # check by check, the nodes of its edges
    u = np.random.default_rng(64800).integers(0, 2, (3, K)).astype(np.uint8)
    cw = np.stack([dvbs2.encode(x) for x in u])
    assert (cw[:, :K] == u).all() and cw[:, K:].any()
    for c in cw:                                                     # H c = 0; with T invertible and c[:K] = u that fixes c
        assert not (np.bincount(chk_of_slot, weights=c[chk_vars], minlength=dvbs2.nchk).astype(np.int64) % 2).any()
    # ... and one of them against a forward substitution in numpy: every check holds one parity bit that no later check holds
    starts = np.concatenate([[0], np.cumsum(dc)])
    rows = [chk_vars[starts[r]:starts[r + 1]] for r in range(dvbs2.nchk)]
    count = np.bincount(np.concatenate([r[r >= K] for r in rows]), minlength=N)
    by_col = {}
    for r, vs in enumerate(rows):
        for v in vs[vs >= K]:
            by_col.setdefault(int(v), []).append(r)
    gone, define, stack = np.zeros(dvbs2.nchk, bool), {}, [v for v in range(K, N) if count[v] == 1]
    peel_order = []
    while stack:
        v = stack.pop()
        if v in define or count[v] != 1:
            continue
        r = next(r for r in by_col[v] if not gone[r])
        define[v], gone[r] = r, True
        peel_order.append(v)
        for w in rows[r][rows[r] >= K]:
            if w != v:
                count[w] -= 1
                if count[w] == 1:
                    stack.append(int(w))
    assert len(peel_order) == 32400
    ref = np.zeros(N, np.uint8)
    ref[:K] = u[1]
    for v in reversed(peel_order):                                   # the bit peeled last depends on no other parity bit
        vs = rows[define[v]]
        ref[v] = np.bitwise_xor.reduce(ref[vs[vs != v]])
    assert (ref == cw[1]).all()


def test_the_twin_code_has_no_sparse_form_and_says_how_far_the_peel_came():
    import lut_ldpc_amd as L
    for gen in (True, "sparse"):
        with pytest.raises(LutLdpcError, match=r"0 of its last 32400 columns peel"):
            L.Codec(CODES / f"{sc.TWIN}.alist", with_generator=gen, known_rank=32400, device=-1)
    with pytest.raises(ValueError):
        L.Codec(CODES / f"{sc.TWIN}.alist", with_generator="dense", device=-1)


def test_codec_files_round_trip_the_sparse_form_and_still_load_the_dense_one(alists, tmp_path):
    import lut_ldpc_amd as L
    path, N, M = alists("ira200")
    u = np.random.default_rng(7).integers(0, 2, (8, N - M)).astype(np.uint8)
    for gen in ("sparse", True):
        pcd = L.Codec(path, with_generator=gen, device=-1)
        pcd.design_luts(sigma2=0.8 ** 2, max_iters=3, allow_degree_one=True)
        want = np.stack([pcd.encode(x) for x in u])
        file = tmp_path / f"codec_{gen}.it"
        pcd.save(file)
        pcd.close()
        assert (b"sparse_lutldpc" in file.read_bytes()) == (gen == "sparse") and (b"G_A" in file.read_bytes()) == (gen is True)
        back = L.Codec(codec_path=file, device=-1)
        assert (back.nvar, back.ninfo) == (N, N - M)
        assert (np.stack([back.encode(x) for x in u]) == want).all(), gen
        back.close()


@pytest.fixture(scope="module")
def host_only():
    dec = product_decoder(fc.codec("reg36_n1000_q4"), device=-1)
    yield dec
    dec.close()


def _set(h, K, R, row_ptr, cols):
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    return lib.lutldpc_decoder_set_sparse_generator(h, K, R, p(row_ptr), p(cols))


def test_refusals_on_a_host_only_handle_arguments_before_state_and_nothing_changes(host_only):
    before = host_only.describe()
    assert "generator" not in before and host_only.nvar == 1000
    row_ptr, cols = (np.array(a) for a in sc.system(600, 400, "permuted"))
    assert _set(None, 600, 400, row_ptr, cols) == ERR_ARG
    for name, (K, R, rp, cl, word) in sc.refusals(600, 400).items():
        assert _set(host_only._h, K, R, rp, cl) == ERR_ARG, name
        assert word in last_error(), (name, last_error())
        assert host_only.describe() == before, name
    m = re.search(r"cycle through bit (\d+)", last_error())              # (the cycle is the last of the list)
    assert m and int(m.group(1)) in (607, 608, 609)
    assert _set(host_only._h, 600, 400, row_ptr, cols) == ERR_STATE      # valid arguments: the handle has no device
    assert host_only.describe() == before
    with pytest.raises(ValueError):
        host_only.set_sparse_generator(600, 400, row_ptr[:-1], cols)


def test_case_lists_hold_what_they_claim():
    assert {c[0] for c in sc.SYSTEM_CASES} == {"q4", "q4_pack1", "n10000"} and all(h in fc.HANDLES for h, *_ in sc.SYSTEM_CASES)
    assert fc.HANDLES["q4"][2] == 512 and fc.HANDLES["q4_pack1"][2] == 256
    for h in ("q4", "q4_pack1"):
        mine = [(K, R, kind) for hh, K, R, kind in sc.SYSTEM_CASES if hh == h]
        assert {1, 31, 32, 33} <= {K for K, _, _ in mine} and any(K % 32 for K, _, _ in mine) and any(R == 1 for _, R, _ in mine)
        assert {kind for _, _, kind in mine} == set(sc.KINDS)
    assert set(sc.BATCHES) >= {1, 63, 64, 65, 130, 127, 128, 129}
    for _, K, R, kind in dict.fromkeys(sc.SYSTEM_CASES):
        row_ptr, cols = sc.system(K, R, kind)
        assert row_ptr[0] == 0 and (np.diff(row_ptr) >= 0).all() and row_ptr[-1] == len(cols) and ((cols >= 0) & (cols < K + R)).all()
        n_terms = np.diff(row_ptr)
        n_par = np.array([(cols[row_ptr[i]:row_ptr[i + 1]] >= K).sum() for i in range(R)])
        assert all(K + i not in cols[row_ptr[i]:row_ptr[i + 1]] for i in range(R))
        d = sc.depth(K, R, row_ptr, cols)
        if R >= 8:
            assert (n_terms == 0).any() and ((n_par > 0) & (n_par == n_terms)).any() and (n_terms >= sc.WIDE_ROW).any(), (K, R, kind)
        if kind == "chain":
            assert d == R and (R == 1 or d > 2 * sc.BLOCK + 1)
        elif kind == "short_chains":
            assert 2 <= d <= 16
        else:
            assert n_par.max() >= 3 and 0 in n_par and 2 < d < R
        cw = sc.system_reference(K, R, kind, (K + 31) // 32)
        assert cw.shape == (max(sc.BATCHES), K + R)
        par = cw[:, K:]
        want = np.array([np.bitwise_xor.reduce(cw[:, cols[row_ptr[i]:row_ptr[i + 1]]], axis=1) if n_terms[i] else np.zeros(len(cw), np.uint8) for i in range(R)]).T
        assert (par == want).all()                                     # every row's equation holds: with T invertible that fixes the parity
        assert R < 8 or (par.any() and par.mean() < 0.9)
    for K, R in {(K, R) for _, K, R, _ in sc.SYSTEM_CASES}:
        w = sc.windows(K, R)
        assert (0, K + R) in w and (K, R) in w and any(f < K < f + c for f, c in w) and any(f % 32 for f, _ in w)
    names = set(sc.refusals())
    assert names == {"NULL row_ptr", "NULL cols", "K = 0", "R < 0", "K + R != nvar", "row_ptr not from 0", "row_ptr descends", "entry = K + R", "entry < 0",
                     "own bit", "cycle"}
    assert list(sc.refusals())[-1] == "cycle"


def test_host_half_as_a_stand_alone_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/sparse_generator_check.cpp: peel, topological sort, block inversion and upload packing on random systems, the packed arrays
    walked as the kernels walk them.  Its own main, host code only; nothing is loaded into Python."""
    import shutil
    import subprocess
    from pathlib import Path
    clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    cxx = str(clang) if clang.exists() else shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "sparse_generator_check"
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        f"-I{ROOT / 'lut_ldpc_amd' / 'csrc' / 'host'}", str(ROOT / "tests" / "sparse_generator_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), (r.stdout[-3000:], r.stderr[-3000:])
