"""The [BP] decoder's device front end, CPU side (include/lut_ldpc_bp.h): the AWGN cell table against math.erfc alone, the
refusals a host-only handle can show, and -- with the references of tests/bp_frontend_cases.py alone -- that every crafted table and
every decode case of tests/test_32_bp_frontend_gpu.py holds what its name claims."""
import ctypes as C
import math
import shutil
import subprocess

import numpy as np
import pytest

import bp_frontend_cases as BC
import lut_ldpc_amd as L
from helpers import CODES, ROOT
from lut_ldpc_amd import _capi
from lut_ldpc_amd._capi import lib, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED
from lut_ldpc_amd.bp import awgn_cells

TWO64 = 1 << 64


def _near_tail(t, N0):
    """(mass of the nearer tail of x ~ N(1, N0/2) at t in units of 2^-64 as an int, whether it is the lower tail): the formula of
    the header, evaluated with math.erfc."""
    z = (t - 1.0) / math.sqrt(N0 / 2)
    w = 0.5 * math.erfc(abs(z) * 0.70710678118654752440) * 18446744073709551616.0
    return min(int(w), TWO64 - 1), z <= 0


# the last one: the clip binds on both sides (all 2 QMAX + 1 QLLRs and the split)
@pytest.mark.parametrize("N0,d1,d4", [(1.0, 4, 28), (1.0, 12, 28), (10 ** -0.16 / 0.5, 12, 28), (0.2, 12, 28), (30.0, 4, 8), (0.02, 10, 28),
                                      (1.0, 12, 8)])
def test_awgn_table_against_erfc(N0, d1, d4):
    t = awgn_cells(N0, d1, d4)
    thr, q, neg = [int(x) for x in t["thr"]], t["qllr"].astype(np.int64), t["neg"]
    n, qmax, step = len(q), 2 ** (d4 - 1) - 1, N0 / (4 * 2.0 ** d1)
    assert len(thr) == n - 1 and all(a <= b for a, b in zip(thr[:-1], thr[1:]))
    # QLLRs contiguous and ascending, the one repeat at 0; neg exactly up to the zero split
    dq = np.diff(q)
    split = np.flatnonzero(dq == 0)
    assert set(dq.tolist()) <= {0, 1} and len(split) <= 1 and (len(split) == 0 or q[split[0]] == 0)
    assert np.abs(q).max() <= qmax
    if len(split):
        assert (neg[:split[0] + 1] == 1).all() and (neg[split[0] + 1:] == 0).all()
    else:
        assert (neg == (q < 0)).all()
    assert n == q[-1] - q[0] + 1 + len(split)                                     # the closed form from the trimmed range
    # every threshold: within 2^-50 (relative) of the nearer-tail mass, at least one unit
    uppers = [0.0 if (len(split) and j == split[0]) else (float(q[j]) + 0.5) * step for j in range(n - 1)]
    for j in range(n - 1):
        mass, lower = _near_tail(uppers[j], N0)
        got = thr[j] if lower else TWO64 - 1 - thr[j]
        assert abs(got - mass) <= max(mass >> 50, 1), (j, q[j], got, mass)
    # the trimmed range: the first threshold is positive, the one before it would not be (unless the clip binds); the last is below
    # 2^64 - 1, the one after it would not be
    assert thr[0] > 0 and thr[-1] < TWO64 - 1
    if q[0] > -qmax:
        assert _near_tail((float(q[0]) - 0.5) * step, N0)[0] <= 1
    if q[-1] < qmax:
        assert _near_tail((float(q[-1]) + 0.5) * step, N0)[0] <= 1
    if (N0, d1, d4) == (1.0, 12, 8):                                              # cells merge into +-QMAX: both outer cells carry mass
        assert q[0] == -qmax and q[-1] == qmax and n == 2 * qmax + 2 and thr[0] > 2 ** 59 and TWO64 - thr[-1] > 2 ** 63


def test_zero_split_is_the_lut_tables_threshold_at_zero():
    """The threshold of the zero split equals the x = 0 threshold of Codec.channel_cells at the same N0, integer for integer."""
    from helpers import product_codec
    cd = product_codec("n500_q4_i8")
    for snr in (0.0, 1.6, 4.0):
        lut = cd.channel_cells(snr)
        j = int(np.flatnonzero(lut["neg"])[-1])                                # the last cell on the negative side ends at x = 0
        t = awgn_cells(10 ** (-snr / 10) / cd.rate)
        k = int(np.flatnonzero(np.diff(t["qllr"]) == 0)[0])
        assert int(t["thr"][k]) == int(lut["thr"][j]), (snr, int(t["thr"][k]), int(lut["thr"][j]))


def test_awgn_cells_refusals():
    n = C.c_int32(-1)
    thr, q, neg = np.zeros(900, np.uint64), np.zeros(900, np.int32), np.zeros(900, np.uint8)
    args = (thr.ctypes.data_as(C.POINTER(C.c_uint64)), q.ctypes.data_as(C.POINTER(C.c_int32)), neg.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert lib.lutldpc_bp_awgn_cells(4, 28, 1.0, 823, C.byref(n), *args) == ERR_ARG and n.value == 824 and b"824" in lib.lutldpc_last_error()
    assert not thr.any() and not q.any() and not neg.any()
    assert lib.lutldpc_bp_awgn_cells(4, 28, 1.0, 824, C.byref(n), *args) == 0 and n.value == 824 and q[0] < 0 < q[823]
    assert lib.lutldpc_bp_awgn_cells(4, 28, 1.0, 900, None, *args) == ERR_ARG
    for bad in [(25, 28, 1.0), (4, 7, 1.0), (4, 30, 1.0), (4, 28, 0.0), (4, 28, -1.0), (4, 28, float("nan")), (4, 28, float("inf"))]:
        assert lib.lutldpc_bp_awgn_cells(*bad, 900, C.byref(n), *args) == ERR_ARG, bad
    assert lib.lutldpc_bp_awgn_cells(12, 28, 0.005, 900, C.byref(n), *args) == ERR_UNSUPPORTED      # 26 dB at rate 1/2: 3 * 10^6 cells
    assert _capi.LutLdpcError and len(awgn_cells(0.02)["qllr"]) < 2 ** 21                          # 20 dB still fits


def test_host_only_handle_argument_errors_before_state_errors():
    code = BC.graph("n33")
    dec = L.BPDecoder(code.nvar, code.nchk, code.dv, code.dc, code.cn_msg_idx, *BC.D, device=-1)
    h, N = dec._h, code.nvar
    good = _capi.BPCells.from_table(BC.named([1 << 63]))
    q, unc, st = np.full((3, N), 77, np.int32), np.full(3, 77, np.int32), np.full((3, 4), 77, np.int32)
    qp, up, sp = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in (q, unc, st))
    # set_cells: argument errors, then the host-only handle
    assert lib.lutldpc_bp_set_cells(None, C.byref(good)) == ERR_ARG and lib.lutldpc_bp_set_cells(h, None) == ERR_ARG
    for field in ("thr", "qllr", "slicer_neg"):
        c = _capi.BPCells.from_table(BC.named([1 << 63]))
        setattr(c, field, None)
        assert lib.lutldpc_bp_set_cells(h, C.byref(c)) == ERR_ARG, field
    for n_cells in (0, -1, 2 ** 21 + 1):
        c = _capi.BPCells.from_table(BC.named([1 << 63]))
        c.n_cells = n_cells
        assert lib.lutldpc_bp_set_cells(h, C.byref(c)) == ERR_ARG, n_cells
    desc = BC.named([5, 9, 12])
    desc["thr"] = np.array([5, 12, 9], np.uint64)
    over = BC.named([5, 9])
    over["qllr"] = np.array([0, BC.QMAX + 1, 1], np.int32)
    under = dict(over, qllr=np.array([0, -BC.QMAX - 1, 1], np.int32))
    for t in (desc, over, under):
        assert lib.lutldpc_bp_set_cells(h, C.byref(_capi.BPCells.from_table(t))) == ERR_ARG
    assert lib.lutldpc_bp_set_cells(h, C.byref(good)) == ERR_STATE
    with pytest.raises(L.LutLdpcError):
        dec.set_cells(BC.named([1 << 63]))
    # the batch entries: NULL handle / B, then the entry's own arguments, then the host-only handle
    S, Q = lib.lutldpc_bp_sample_qllr, lib.lutldpc_bp_sim_batch
    assert S(None, 1, 0, 0, 3, None, qp, up) == ERR_ARG and S(h, 1, 0, 0, 0, None, qp, up) == ERR_ARG and S(h, 1, 0, 0, -3, None, qp, up) == ERR_ARG
    assert S(h, 1, 0, 0, 3, None, None, up) == ERR_ARG and S(h, 1, 2 ** 31, 0, 3, None, qp, up) == ERR_ARG
    assert S(h, 1, 0, 0, 3, None, qp, up) == ERR_STATE and S(h, 1, 0, 0, 3, None, qp, None) == ERR_STATE
    assert Q(None, 1, 0, 0, 3, None, 5, sp, None, None) == ERR_ARG and Q(h, 1, 0, 0, 0, None, 5, sp, None, None) == ERR_ARG
    assert Q(h, 1, 0, 0, 3, None, 5, None, None, None) == ERR_ARG
    assert Q(h, 1, 0, 0, 3, None, -1, sp, None, None) == ERR_ARG and Q(h, 1, 0, 0, 3, None, N + 1, sp, None, None) == ERR_ARG
    assert Q(h, 1, 2 ** 31, 0, 3, None, 5, sp, None, None) == ERR_ARG
    assert Q(h, 1, 0, 0, 3, None, 0, sp, None, None) == ERR_STATE and Q(h, 1, 0, 0, 3, None, N, sp, qp, None) == ERR_STATE
    assert (q == 77).all() and (unc == 77).all() and (st == 77).all()                        # a refused call writes nothing
    dec.close()


def test_sizeof_bp_cells():
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no system C compiler to take sizeof(lutldpc_bp_cells) with")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        src = f"{tmp}/s.c"
        open(src, "w").write('#include <stdio.h>\n#include "lut_ldpc_bp.h"\nint main(void) { printf("%zu\\n", sizeof(lutldpc_bp_cells)); return 0; }\n')
        subprocess.run([cc, "-I", str(ROOT / "include"), src, "-o", f"{tmp}/s"], check=True)
        assert int(subprocess.run([f"{tmp}/s"], check=True, capture_output=True, text=True).stdout) == C.sizeof(_capi.BPCells)


# ---- the crafted tables hold what their names claim, for the frames the GPU test uses
def _cases(table):
    return [c for c in BC.SAMPLER_CASES if c[1] == table]


def test_case_lists_cover_what_the_gpu_test_claims():
    assert {c[1] for c in BC.SAMPLER_CASES} == set(BC.TABLES)
    for code in ("n127", "n33"):
        assert {c[1] for c in BC.SAMPLER_CASES if c[0] == code} == set(BC.TABLES)
    assert {c[2] for c in BC.SAMPLER_CASES} == {1, 255, 256, 257, 513}
    assert {c[3] for c in BC.SAMPLER_CASES} == {0, BC.F_CARRY, BC.F_HIGH, BC.F_WRAP}
    assert BC.graph("n127").nvar == 127 and BC.graph("n33").nvar == 33 and BC.graph("n500").nvar == 500
    assert len(BC.awgn_table(*BC.AWGN["awgn_d12"])["qllr"]) > 2 ** 16 and 100 < len(BC.awgn_table(*BC.AWGN["awgn_d4"])["qllr"]) < 1000
    for case in BC.SAMPLER_CASES:
        cells, u, N, B, cw = BC.sampler_case(case)
        assert len(cells["thr"]) == len(cells["qllr"]) - 1 == len(cells["neg"]) - 1 and np.abs(cells["qllr"].astype(np.int64)).max() <= BC.QMAX
        if cw is not None:
            assert ((cw & 1) == 1).any() and ((cw & 1) == 0).any() and (cw > 1).any()          # random bytes: only bit 0 counts
        if case[3] == BC.F_CARRY:
            assert B > 7                                                                        # the carry happens inside the batch
        if case[3] == BC.F_WRAP and B > 5:
            assert int(FC_frames(case)[5]) == 0


def FC_frames(case):
    import frontend_cases as FC
    return FC.frames(case[3], case[2])


@pytest.mark.parametrize("case", _cases("one_slice"), ids=BC.case_id)
def test_one_slice_table(case):
    _, u, N, B, _ = BC.sampler_case(case)
    cells, s, inside = BC.table_one_slice(u)
    thr = cells["thr"]
    assert len(thr) >= 3000 and ((thr >> np.uint64(64 - BC.SLICE_BITS)) == s).all()
    cell = np.searchsorted(thr, u, side="right")
    assert (cell == 0).any() and (cell == len(thr)).any()                       # samples below and above the slice
    for x in inside:                                                             # every sample of the slice ties a threshold: its cell holds only it
        j = int(np.searchsorted(thr, np.uint64(x), side="right"))
        assert int(thr[j - 1]) == x and int(thr[j]) == x + 1
    assert len(inside) >= 1 and len(np.unique(cells["qllr"])) == len(cells["qllr"])


@pytest.mark.parametrize("case", _cases("slice_ends"), ids=BC.case_id)
def test_slice_ends_table(case):
    _, u, N, B, _ = BC.sampler_case(case)
    cells, ks, both = BC.table_slice_ends(u)
    thr = [int(t) for t in cells["thr"]]
    for k in ks:
        assert {(k << 48) - 1, k << 48, (k << 48) + 1} <= set(thr)
    sl = (u >> np.uint64(48)).astype(np.int64)
    assert len(both) == 12 and set(both) <= set(ks)
    for k in both:                                                               # samples on both sides of the slice end
        assert (sl == k - 1).any() and (sl == k).any()
    assert sum(bool((sl == k).any()) for k in ks) >= 12


def test_extremes_table():
    cells, empty = BC.table_extremes()
    assert 0 in empty and {BC.QMAX, -BC.QMAX} <= set(cells["qllr"].tolist()) and int(cells["thr"][-1]) == TWO64 - 1 and int(cells["thr"][0]) == 0
    assert len(empty) >= 6
    for case in _cases("extremes"):
        _, u, N, B, _ = BC.sampler_case(case)
        hit = set(np.searchsorted(cells["thr"], u, side="right").ravel().tolist())
        unreachable = [j for j in empty if j != len(cells["qllr"]) - 1]          # the last cell holds the one value 2^64 - 1
        assert not (hit & set(unreachable)) and len(hit) >= 4                   # empty cells never hit, the others are
    last = np.searchsorted(cells["thr"], np.array([TWO64 - 1, TWO64 - 2], np.uint64), side="right")
    assert last.tolist() == [len(cells["qllr"]) - 1, len(cells["qllr"]) - 3]    # a sample in the last cell needs u = 2^64 - 1


def test_awgn_tables_are_hit_across_their_range():
    for case in _cases("awgn_d12"):
        cells, u, N, B, cw = BC.sampler_case(case)
        cell = np.searchsorted(cells["thr"], u, side="right")
        assert int(cell.max()) - int(cell.min()) > len(cells["qllr"]) // 4                      # far more cells apart than a slice holds
        q, unc = BC.sample(cells, *case[4:6], case[3], B, N, cw, u=u)
        assert (q < 0).any() and (q > 0).any() and unc.sum() > 0


# ---- the decode cases, with the oracle alone
@pytest.mark.parametrize("name", sorted(BC.SIM_CASES))
def test_decode_cases_hold_converging_and_non_converging_frames(name):
    g, cw, rate = BC.sim_code(name)
    assert not BC.syndromes(g, cw & 1).any() and (cw & 1).any() and (cw > 1).any()            # codewords of the graph, in random bytes
    iters = BC.SIM_CASES[name][2]
    for nonzero in (False, True):
        it = BC.sim_reference(name, True, False, nonzero)["iters"]
        assert (it > 0).sum() >= 10 and (it == -iters).sum() >= 10, (name, nonzero, np.unique(it, return_counts=True))
        it0 = BC.sim_reference(name, True, True, nonzero)["iters"]
        assert (it0 >= 0).any() and (it0 == -iters).any()
        r = BC.sim_reference(name, False, False, nonzero)
        assert (r["iters"] == -iters).all() and r["stats"][:, 1].any() and not r["stats"][:, 1].all()
        assert (r["stats"][:, 3] > 0).mean() > 0.8                                               # the channel alone leaves errors in most frames
    a, b = BC.sim_reference(name, True, False, False), BC.sim_reference(name, True, False, True)
    assert (a["unc"] == b["unc"]).all() and (np.abs(a["q"]) == np.abs(b["q"])).all() and (a["q"] != b["q"]).any()     # same noise, other signal
