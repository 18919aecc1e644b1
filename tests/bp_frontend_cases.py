"""References and cases of the [BP] decoder's device front end (include/lut_ldpc_bp.h: cell sampler, error counters), shared by
tests/test_bp_frontend_cpu.py (checks, with the references alone, that every crafted table and every decode case holds what its name
claims) and tests/test_32_bp_frontend_gpu.py (holds the kernels to the references through the C-ABI).  The references are the numpy
Philox of frontend_cases.py with np.searchsorted as the cell, the oracle's BP.decode_qllr_batch and plain numpy counting; nothing of
the code under test.  Everything is integer: equal bit for bit, no tolerance.

Cell tables are dicts {"thr": uint64[n - 1], "qllr": int32[n], "neg": uint8[n]}.  The crafted ones are cut from the reference's own
uniforms of the run they belong to, so that samples tie thresholds and fall where the table is meant to be hit; their QLLRs name the
cell (all different), so a wrong cell is a wrong value."""
from __future__ import annotations

import functools
import tempfile
from pathlib import Path

import numpy as np

import frontend_cases as FC
from helpers import CODES, write_degree_alist
from oracle import oracle as orc

SLICE_BITS = 16                                    # kernels_bp_frontend.hpp: kBpSliceBits, 65536 slices of the unit interval
SLICE = 1 << (64 - SLICE_BITS)
TWO64 = 1 << 64
D = (12, 300, 7, 28)                               # LLR_calc_unit of every handle here
QMAX = 2 ** (D[3] - 1) - 1
N500 = "rate0.50_dv02-17_dc08-09_lut_q4_N500"


# ---------------------------------------------------------------------------------------------------------------- references
def sample(cells, seed, stream, frame0, B, N, codewords=None, u=None):
    """(qllr [B, N] int32, uncoded errors [B] int32): cell = thresholds <= u; a sent 1 (bit 0 of the byte) mirrors the value; the
    uncoded error of a sample is the cell's neg whichever bit was sent."""
    u = FC.uniforms(seed, stream, frame0, B, N) if u is None else u
    cell = np.searchsorted(cells["thr"], u, side="right")
    q = cells["qllr"][cell].astype(np.int64)
    if codewords is not None:
        q = np.where((np.asarray(codewords).reshape(B, N) & 1).astype(bool), -q, q)
    return q.astype(np.int32), cells["neg"][cell].astype(np.int64).sum(1).astype(np.int32)


def count(bits, iters, unc, K, codewords=None):
    """frame_stats [B, 4] = {bp_decode return value, frame error, data bit errors over the first K nodes, uncoded errors}."""
    sent = 0 if codewords is None else (np.asarray(codewords)[:, :K] & 1)
    be = (bits[:, :K] ^ sent).astype(np.int64).sum(1)
    return np.stack([iters, be > 0, be, unc], axis=1).astype(np.int32)


def syndromes(code, bits):
    """[B, nchk]: the parity of every check over bits [B, nvar], from the graph arrays alone."""
    vn_of_edge = np.repeat(np.arange(code.nvar), code.dv)
    ends = np.cumsum(code.dc)
    per_edge = np.asarray(bits, np.int64)[:, vn_of_edge[np.asarray(code.cn_msg_idx)]]
    return np.add.reduceat(per_edge, np.concatenate([[0], ends[:-1]]), axis=1) % 2


# ---------------------------------------------------------------------------------------------------------------- cell tables
def named(thr):
    """The table of ascending thresholds thr: cell j carries the QLLR 3 (j - n // 2) + 1 (all different, both signs, never 0) and an
    irregular neg pattern."""
    thr = np.asarray(thr, np.uint64)
    assert all(int(a) <= int(b) for a, b in zip(thr[:-1], thr[1:]))
    j = np.arange(len(thr) + 1)
    return {"thr": thr, "qllr": (3 * (j - len(j) // 2) + 1).astype(np.int32), "neg": ((j * 5 + 1) % 3 == 0).astype(np.uint8)}


def fullest_slice(u):
    s = (u >> np.uint64(64 - SLICE_BITS)).astype(np.int64).ravel()
    return int(np.bincount(s, minlength=1 << SLICE_BITS).argmax())


def table_one_slice(u):
    """Every threshold inside ONE slice, the one that holds the most samples: 3000 evenly spaced ones (a bisection of 12 trips) and,
    for every sample of the slice, the pair (u, u + 1) -- the cell between them holds exactly the samples whose uniform equals u."""
    s = fullest_slice(u)
    lo = s * SLICE
    inside = sorted({int(x) for x in u.ravel() if lo <= int(x) < lo + SLICE})
    thr = {lo + 1 + k * ((SLICE - 2) // 3000) for k in range(3000)}
    for x in inside:
        thr |= {x, x + 1}
    return named(sorted(t for t in thr if lo < t < lo + SLICE)), s, inside


def table_slice_ends(u):
    """Thresholds on slice ends, one below and one above (k << 48 and its two neighbours): 12 ends k whose two slices k - 1 and k both
    hold samples of the batch (samples on both sides of the end; a batch of a few hundred samples has none and gets none), and the
    ends of the slices of the first 24 samples with the slices after them.  Returns (table, all ends, the two-sided ends)."""
    sl = np.unique((u >> np.uint64(64 - SLICE_BITS)).astype(np.int64))
    both = [int(k) for k in sl[1:][np.diff(sl) == 1]]
    both = both[::max(1, len(both) // 12)][:12]
    ks = sorted({int(x) >> (64 - SLICE_BITS) for x in u.ravel()[:24]})
    ks = sorted({k + d for k in ks for d in (0, 1) if 0 < k + d < (1 << SLICE_BITS)} | set(both))
    thr = sorted({(k << (64 - SLICE_BITS)) + d for k in ks for d in (-1, 0, 1)})
    return named(thr), ks, both


def table_extremes():
    """Thresholds at 0 (cell 0 unreachable) and at 2^64 - 1 (the last cell holds that one value), runs of equal thresholds (empty
    cells) in the middle and on a slice end, QLLRs at +-QMAX next to small ones.  Returns (table, cells predicted empty)."""
    thr = [0, 0, 1 << 62, 1 << 62, 1 << 62, (3 << 62) + 17, (3 << 62) + 17, 60000 << 48, 60000 << 48, TWO64 - 1, TWO64 - 1]
    assert thr == sorted(thr)
    width = np.diff(np.array([0] + thr + [TWO64], dtype=object))                    # cell j = [thr[j-1], thr[j])
    q = np.array([5, -7, -QMAX, 9, -11, QMAX, 13, QMAX - 1, -15, -(QMAX - 1), 17, -QMAX], np.int32)
    return {"thr": np.array(thr, np.uint64), "qllr": q, "neg": (np.arange(12) % 2).astype(np.uint8)}, [j for j, w in enumerate(width) if w <= 1]


AWGN = {"awgn_d4": (1.0, 4), "awgn_d12": (1.0, 12)}      # name -> (N0, d1): a few hundred cells; about 2 * 10^5, more than 2^16


@functools.lru_cache(maxsize=None)
def awgn_table(N0, d1=D[0], d4=D[3]):
    """The builder's table (lutldpc_bp_awgn_cells), an input here: tests/test_bp_frontend_cpu.py holds it to math.erfc."""
    from lut_ldpc_amd.bp import awgn_cells
    t = awgn_cells(N0, d1, d4)
    for a in t.values():
        a.setflags(write=False)
    return t


def cell_table(table, u):
    if table in AWGN:
        return awgn_table(*AWGN[table])
    if table == "one_cell":
        return {"thr": np.zeros(0, np.uint64), "qllr": np.array([-123], np.int32), "neg": np.array([1], np.uint8)}
    if table == "two_cells":
        return named([1 << 63])
    if table == "one_slice":
        return table_one_slice(u)[0]
    if table == "slice_ends":
        return table_slice_ends(u)[0]
    if table == "extremes":
        return table_extremes()[0]
    raise KeyError(table)


TABLES = ["awgn_d4", "awgn_d12", "one_cell", "two_cells", "one_slice", "slice_ends", "extremes"]


# ---------------------------------------------------------------------------------------------------------------- codes
_tmp = None


@functools.lru_cache(maxsize=None)
def graph(name):
    """The oracle's Code: the odd-N graphs of frontend_cases.SYNTHETIC (n127: 64 bit pairs, the last one half empty; n33: 17 pairs,
    fewer than one chunk of the sampler) or the N = 500 code."""
    global _tmp
    if name == "n500":
        return orc.Code(CODES / f"{N500}.alist")
    vdeg, cdeg, _ = FC.SYNTHETIC[name]
    _tmp = _tmp or tempfile.TemporaryDirectory(prefix="bp_frontend_")
    path = Path(_tmp.name) / f"{name}.alist"
    write_degree_alist(path, vdeg, cdeg, seed=FC.GRAPH_SEED)
    return orc.Code(path)


F_CARRY, F_HIGH, F_WRAP = FC.F_CARRY, FC.F_HIGH, FC.F_WRAP
SEED_BIG, STREAM_MAX = FC.SEED_BIG, FC.STREAM_MAX

# sampler cases: (code, table, B, frame0, seed, stream, codewords: None or "bytes").  A BP block is 256 frames: B = 1, 255, 256, 257,
# 513; every table on an odd-N code with and without sent bits; frame ranges that carry into the high counter word and wrap at 2^64
SAMPLER_CASES = [
    ("n127", "awgn_d4", 257, F_CARRY, 3, 0, "bytes"),
    ("n127", "awgn_d12", 513, F_HIGH, SEED_BIG, 7, "bytes"),
    ("n127", "awgn_d12", 255, 0, 3, STREAM_MAX, None),
    ("n127", "one_cell", 1, 0, 3, 7, "bytes"),
    ("n127", "two_cells", 256, F_WRAP, SEED_BIG, 0, None),
    ("n127", "one_slice", 513, 0, SEED_BIG, 7, "bytes"),
    ("n127", "slice_ends", 257, F_WRAP, 3, STREAM_MAX, "bytes"),
    ("n127", "extremes", 513, F_CARRY, SEED_BIG, 0, "bytes"),
    ("n33", "awgn_d4", 513, F_WRAP, SEED_BIG, 7, None),
    ("n33", "awgn_d12", 257, F_CARRY, 3, 0, "bytes"),
    ("n33", "one_cell", 257, F_HIGH, SEED_BIG, STREAM_MAX, None),
    ("n33", "two_cells", 1, F_HIGH, 3, STREAM_MAX, "bytes"),
    ("n33", "one_slice", 513, F_CARRY, 3, 0, None),
    ("n33", "slice_ends", 255, 0, SEED_BIG, 7, None),
    ("n33", "extremes", 256, F_HIGH, 3, 7, "bytes"),
    ("n500", "awgn_d12", 257, F_WRAP, 3, 7, "bytes"),
    ("n500", "one_slice", 1, F_HIGH, SEED_BIG, 0, "bytes"),
]


def case_id(case):
    code, table, B, f0, seed, stream, cw = case
    f = {0: "0", F_CARRY: "carry", F_HIGH: "high", F_WRAP: "wrap"}[f0]
    return f"{code}-{table}-B{B}-f{f}-s{seed % 97}-st{stream % 97}-{cw or 'zero'}"


@functools.lru_cache(maxsize=None)
def sampler_case(case):
    """(cells, u, N, B, codewords or None): the table and the reference's uniforms of a case; the codewords are random BYTES, of which
    only bit 0 counts.  Shared read-only."""
    code, table, B, f0, seed, stream, cwk = case
    N = graph(code).nvar
    u = FC.uniforms(seed, stream, f0, B, N)
    u.setflags(write=False)
    cw = None
    if cwk:
        cw = np.random.default_rng(B * 1000 + N).integers(0, 256, (B, N), dtype=np.uint8)
        cw.setflags(write=False)
    return cell_table(table, u), u, N, B, cw


# ---------------------------------------------------------------------------------------------------------------- decode cases
# name -> (code, Eb/N0 in dB, max_iters, K_info): at this SNR the batch holds frames that leave through the syndrome check and frames
# that return -max_iters (checked with the oracle alone in tests/test_bp_frontend_cpu.py)
SIM_CASES = {"n500": ("n500", 1.6, 12, 250), "n33": ("n33", 1.5, 6, 22)}
SIM_B, SIM_SEED, SIM_STREAM = 257, 11, 5
EXIT_MODES = [(True, True), (True, False), (False, False)]


@functools.lru_cache(maxsize=None)
def sim_code(name):
    """(the oracle's Code of the graph the codewords belong to, codewords [SIM_B, N] uint8 with random upper bits, rate).  The
    codewords come from the host encoder of the product's Codec (an input: the CPU test checks their syndromes with numpy), on the
    column order of its graph."""
    import lut_ldpc_amd as L
    from helpers import oracle_graph
    code = graph(name)
    path = CODES / f"{N500}.alist" if name == "n500" else Path(_tmp.name) / f"{name}.alist"
    pcd = L.Codec(path, with_generator=True, device=-1)
    g = oracle_graph(pcd)
    rng = np.random.default_rng(code.nvar)
    cw = np.stack([pcd.encode(rng.integers(0, 2, pcd.ninfo, dtype=np.uint8)) for _ in range(SIM_B)])
    cw = (cw | (rng.integers(0, 128, cw.shape, dtype=np.uint8) << 1)).astype(np.uint8)      # only bit 0 counts
    cw.setflags(write=False)
    return g, cw, pcd.ninfo / pcd.nvar


def sim_n0(name):
    return 10 ** (-SIM_CASES[name][1] / 10) / sim_code(name)[2]


@functools.lru_cache(maxsize=None)
def sim_reference(name, psc, pisc, nonzero):
    """numpy sampler -> oracle decode_qllr_batch -> numpy counts: dict(q, unc, bits, iters, stats, cw)."""
    _, _, iters, K = SIM_CASES[name]
    g, cw, _ = sim_code(name)
    cw = cw if nonzero else None
    q, unc = sample(awgn_table(sim_n0(name)), SIM_SEED, SIM_STREAM, 0, SIM_B, g.nvar, cw)
    ref = orc.BP(g, *D)
    ref.set_exit_conditions(iters, psc, pisc)
    bits, it, _ = ref.decode_qllr_batch(q)
    return dict(q=q, unc=unc, bits=bits, iters=it, stats=count(bits, it, unc, K, cw), cw=cw)
