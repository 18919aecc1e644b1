"""Shared helpers for the parity tests.  The ORACLE (oracle/) is the checker; the product is
lut_ldpc_amd.  Both sides always receive the *same* label arrays (never rely on
cross-platform float RNG equality)."""
from __future__ import annotations

import functools
import re
import tempfile
import zlib
from pathlib import Path

import numpy as np

from oracle import oracle as orc

ROOT = Path(__file__).resolve().parent.parent
CODES = ROOT / "data" / "codes"
TREES = ROOT / "data" / "trees"

# name -> (alist, design kwargs)
CONFIGS = {
    # C1 of BASELINE.json: params/ber.ini.irregular.example
    "n500_q4": ("rate0.50_dv02-17_dc08-09_lut_q4_N500", dict(sigma2=0.88 ** 2, max_iters=50, nq_cha=16, nq_msg=16)),
    "n500_q4_i8": ("rate0.50_dv02-17_dc08-09_lut_q4_N500", dict(sigma2=0.88 ** 2, max_iters=8, nq_cha=16, nq_msg=16)),
    "reg36_n1000_q4": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.88 ** 2, max_iters=20, nq_cha=16, nq_msg=16)),
    # non-uniform message resolution + LUT reuse (SURVEY step 5)
    "reg36_n1000_mixed": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.82 ** 2, max_iters=12, nq_cha=16,
                                                           nq_msg=[16, 16, 16, 8, 8, 8, 8, 8, 8, 8, 8, 8],
                                                           reuse_vec=[0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0])),
    # 5-bit labels: more than 16 labels -> byte rows (PACK = 1), 1024-entry tables -> generic kernels
    "reg36_n1000_q5": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.84 ** 2, max_iters=8, nq_cha=32, nq_msg=32)),
    "reg36_n1000_q3_chklut": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.80 ** 2, max_iters=10, nq_cha=16, nq_msg=8, min_lut=False)),
    "reg36_n1000_rootonly": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.85 ** 2, max_iters=6, nq_cha=8, nq_msg=8, tree_method="root_only")),
    "reg36_n1000_high": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.85 ** 2, max_iters=6, nq_cha=16, nq_msg=16, tree_method="auto_bin_high")),
    # three kernels inside one variable pass: degree 3 on the compile-time kernel, degrees 2, 9 and 17 (unbalanced trees) on the generated
    # one or, with LUTLDPC_JIT=0, in the interpreter
    "n500_high": ("rate0.50_dv02-17_dc08-09_lut_q4_N500", dict(sigma2=0.80 ** 2, max_iters=6, nq_cha=16, nq_msg=16, tree_method="auto_bin_high")),
    # C5 of BASELINE.json: params/ber.ini.regular.example (design_SNRdB 3.9, R = 1 - 325/2048)
    "c5_minlut": ("rate0.84_reg_v6c32_N2048", dict(sigma2=None, design_snr_db=3.9, max_iters=8, nq_cha=16, nq_msg=8,
                                                   tree_method="filename=" + str(TREES / "6_32_wide.ini"), rank=325)),
    "c5_chklut": ("rate0.84_reg_v6c32_N2048", dict(sigma2=None, design_snr_db=3.9, max_iters=8, nq_cha=16, nq_msg=8, min_lut=False,
                                                   tree_method="filename=" + str(TREES / "6_32_wide.ini"), rank=325)),
    # C2 / C3 of BASELINE.json
    "reg36_n10000_q4": ("rate0.50_dv03_dc06_N10000", dict(sigma2=0.84 ** 2, max_iters=50, nq_cha=16, nq_msg=16)),
    "dvbs2_q4": ("rate0.50_irreg_dvbs2_N64800", dict(sigma2=0.88 ** 2, max_iters=50, nq_cha=16, nq_msg=16, allow_deg1=True)),
    "dvbs2_q4_i6": ("rate0.50_irreg_dvbs2_N64800", dict(sigma2=0.88 ** 2, max_iters=6, nq_cha=16, nq_msg=16, allow_deg1=True)),
    "twin64800_q4_i6": ("rate0.50_dv02-08_dc07-08_lut_q4_N64800", dict(sigma2=0.88 ** 2, max_iters=6, nq_cha=16, nq_msg=16)),
    # label alphabets from 2 to 64 labels (tests/test_15_label_alphabets_gpu.py); the schedule 8 8 8 8 4 4 4 2 is the one
    # data/params/ber.ini.regular.example documents (qbits_messages = 3 3 3 3 2 2 2 1)
    "reg36_n1000_ex8421": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.6 ** 2, max_iters=8, nq_cha=16, nq_msg=[8, 8, 8, 8, 4, 4, 4, 2])),
    "n500_ex8421": ("rate0.50_dv02-17_dc08-09_lut_q4_N500", dict(sigma2=0.6 ** 2, max_iters=8, nq_cha=16, nq_msg=[8, 8, 8, 8, 4, 4, 4, 2])),
    "reg36_n1000_ex8421_chklut": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.6 ** 2, max_iters=8, nq_cha=16, nq_msg=[8, 8, 8, 8, 4, 4, 4, 2],
                                                                    min_lut=False)),
    "reg36_n1000_m2": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.5 ** 2, max_iters=8, nq_cha=16, nq_msg=2)),          # 1-bit messages
    "reg36_n1000_c2m4": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.6 ** 2, max_iters=8, nq_cha=2, nq_msg=4)),         # hard-decision channel
    "reg36_n1000_c4m4": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.7 ** 2, max_iters=8, nq_cha=4, nq_msg=4)),
    "reg36_n1000_grow": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.75 ** 2, max_iters=6, nq_cha=8, nq_msg=[4, 8, 8, 16, 16, 16])),
    "reg36_n1000_m12": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.8 ** 2, max_iters=8, nq_cha=16, nq_msg=12)),        # half not a power of two
    "reg36_n1000_m6": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.8 ** 2, max_iters=8, nq_cha=16, nq_msg=6)),
    "reg36_n1000_m16_12_8": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.8 ** 2, max_iters=6, nq_cha=16, nq_msg=[16, 16, 12, 12, 8, 8])),
    "reg36_n1000_c32m8": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.8 ** 2, max_iters=8, nq_cha=32, nq_msg=8)),
    "reg36_n1000_q6": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.8 ** 2, max_iters=4, nq_cha=64, nq_msg=64)),          # 6-bit labels
}


def design(code, rank, sigma2, max_iters, nq_msg, **design_kw):
    """An oracle codec of `code` with its rank and rate set and the LUTs designed; nq_msg: one alphabet size, or one per iteration."""
    cd = orc.Codec(code, skip_rank=True)
    cd.set_rank(rank)
    cd.rate = 1.0 - rank / code.nvar
    nq = np.full(max_iters, nq_msg, np.int32) if np.isscalar(nq_msg) else np.asarray(nq_msg, np.int32)
    cd.design_luts(sigma2=sigma2, max_iters=max_iters, nq_msg=nq, **design_kw)
    return cd


@functools.lru_cache(maxsize=None)
def oracle_codec(name: str):
    """Load the alist and design the LUTs with the oracle (cached per test session)."""
    alist, kw = CONFIGS[name]
    kw = dict(kw)
    code = orc.Code(CODES / f"{alist}.alist")
    rank = kw.pop("rank", code.nchk)
    snr = kw.pop("design_snr_db", None)
    sigma2 = kw.pop("sigma2")
    if sigma2 is None:   # src/LDPC_BER_Sim.cpp:482
        rate = 1.0 - rank / code.nvar
        sigma2 = 10 ** (-snr / 10) / (2 * rate)
    return design(code, rank, sigma2, kw.pop("max_iters"), kw.pop("nq_msg"), **kw)


_designed, _tmp = {}, None


def designed_codec(key, write_graph, *, sigma, max_iters, nq_msg, nq_cha=16, rank=None, **design_kw):
    """The oracle-designed code of a test, made once per session and key.  write_graph: a function that writes the alist to the path
    it is given (in the session's temporary directory), or the path of an alist that exists.  N and M come from that graph; rank:
    M unless given; the rate is 1 - rank / N; the design noise is sigma ** 2."""
    global _tmp
    if key not in _designed:
        path = write_graph
        if callable(write_graph):
            _tmp = _tmp or tempfile.TemporaryDirectory(prefix="designed_codes_")
            path = Path(_tmp.name) / f"{key}.alist"
            write_graph(path)
        code = orc.Code(path)
        _designed[key] = design(code, code.nchk if rank is None else rank, sigma ** 2, max_iters, nq_msg, nq_cha=nq_cha, **design_kw)
    return _designed[key]


def product_codec(name, device=-1):
    """The product's own design (C++ host mirror) of a configuration."""
    import lut_ldpc_amd as L
    alist, kw = CONFIGS[name]
    kw = dict(kw)
    rank = kw.pop("rank", None)
    cd = L.Codec(CODES / f"{alist}.alist", known_rank=rank or (32400 if "64800" in alist else 0), device=device)
    snr = kw.pop("design_snr_db", None)
    sigma2 = kw.pop("sigma2")
    if sigma2 is None:
        sigma2 = 10 ** (-snr / 10) / (2 * cd.rate)
    if "allow_deg1" in kw:
        kw["allow_degree_one"] = kw.pop("allow_deg1")
    cd.design_luts(sigma2=sigma2, **kw)
    return cd


C5_TREES = "filename=" + str(TREES / "6_32_wide.ini")      # config 5 (ber.ini.regular.example)


def c5_sigma2(rank=325, n=2048):
    return 10 ** (-3.9 / 10) / (2 * (1.0 - rank / n))


def oracle_graph(pcd):
    """The oracle's Code of a product codec's (column-permuted) graph."""
    dv, dc, cn = pcd.graph()
    return orc.Code(graph=(pcd.nvar, pcd.nchk, dv, dc, cn))


# the decode paths the packed and the soft-value entries run on: name -> (environment at creation, fields of describe() -> value)
PACKED_PATHS = {
    "resident": ({}, dict(resident=1)),
    "streaming": ({"LUTLDPC_RESIDENT": "0"}, dict(resident=0, skewed_pipeline=1)),
    "per_class": ({"LUTLDPC_RESIDENT": "0", "LUTLDPC_SKEW": "0"}, dict(resident=0, skewed_pipeline=0)),
    "byte_rows": ({"LUTLDPC_PACK": "1"}, dict(pack=1, tile_frames=256)),       # nibble input into byte rows
}


def product_decoder(cd, device=0):
    """Build the product's decoder from the oracle-designed tables (the reference's own tree text)."""
    import lut_ldpc_amd as L
    c = cd.code
    chk = "" if cd.min_lut else cd.chk_tree_txt
    return L.Decoder(c.nvar, c.nchk, c.dv, c.dc, c.cn_msg_idx, cd.nq_cha, cd.nq_msg, cd.reuse_vec, cd.max_iters, cd.min_lut,
                     cd.var_tree_txt, chk, device=device)


def awgn_labels(cd, B, snr_db, seed, mode=0):
    """All-zero codeword over BPSK/AWGN, LLR = 4x/N0 (src/LDPC_BER_Sim.cpp:248-278), quantised with the
    designed boundaries (src/LDPC_Code_LUT.cpp:207-221).  Returns (cha, msg0) uint8 [B, nvar]."""
    rng = np.random.default_rng(seed)
    N0 = 10 ** (-snr_db / 10) / cd.rate
    x = 1.0 + rng.normal(0.0, np.sqrt(N0 / 2), (B, cd.code.nvar))
    llr = 4 * x / N0
    cha = orc.quant_nonlin(llr, cd.qb_cha)
    msg = orc.quant_nonlin(llr, cd.qb_msg) if mode == 0 else cd.cha2msg_map[cha].astype(np.uint8)
    return cha, msg, llr


def planted_labels(cd, n, snr, seed, noise_free=(), mode=0, zero=()):
    """awgn_labels of n frames with the frames `noise_free` planted: every label at its largest, so they pass the test on the channel
    decisions; the frames `zero`: every label 0.  (cha, msg0), read-only: computed once per batch and shared."""
    cha, msg, _ = awgn_labels(cd, n, snr, seed=seed, mode=mode)
    free = np.asarray(list(noise_free), np.intp)
    cha[free] = cd.nq_cha - 1
    msg[free] = cd.nq_msg[0] - 1
    cha[list(zero)] = 0
    msg[list(zero)] = 0
    cha.setflags(write=False)
    msg.setflags(write=False)
    return cha, msg


ORACLE = {}      # key of a batch -> the cache `compare` takes: the oracle decodes a batch once per exit mode, all its decoders share the result


def oracle_cache(key):
    return ORACLE.setdefault(key, {})


def same(got, want, what, u=None):
    """Equal integer arrays, or the first mismatches (with u: the 64-bit uniform of the first one)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, f"{len(bad)} mismatches, first (frame, node)", bad[:4].tolist(), "got", got[tuple(bad[0])], "want", want[tuple(bad[0])],
                           None if u is None else hex(int(u[tuple(bad[0])])))


def compare(cd, dec, cha, msg, psc, pisc, max_iters=None, flat=False, cache=None):
    """Decode the same labels with the oracle and through the C-ABI: every decided bit and every returned iteration
    code (src/LDPC_Code_LUT.cpp:259-353) must be equal.  Returns the iteration codes.  cache: a dict that keeps the oracle's
    result per (labels, exit conditions), for callers that decode the same labels with several decoders."""
    I = max_iters or cd.max_iters
    cd.set_exit_conditions(I, psc, pisc)
    dec.set_exit_conditions(I, psc, pisc)
    key = (I, bool(psc), bool(pisc), cha.shape, zlib.crc32(np.ascontiguousarray(cha)), zlib.crc32(np.ascontiguousarray(msg)))
    if cache is not None and key in cache:
        want_bits, want_it = cache[key]
    else:
        # long codes: the oracle's flat-table mode on all cores (bit-identical to its faithful mode: tests/test_oracle_flat.py)
        want_bits, want_it = (cd.lut_decode_batch_flat if (flat or cd.code.nvar >= 10000) else cd.lut_decode_batch)(cha, msg)
        if cache is not None:
            cache[key] = (want_bits, want_it)
    got_bits, got_it = dec.lut_decode_batch(cha, msg)
    assert (want_it == got_it).all(), (np.flatnonzero(want_it != got_it)[:8], want_it[:8], got_it[:8])
    bad = np.argwhere(want_bits != got_bits)
    assert bad.size == 0, f"{len(bad)} bit mismatches, first at frame/bit {bad[:4].tolist()}"
    return want_it


def resident_variant(src):
    """Which variant of the LDS-resident kernel (jit_resident.hpp) a generated source is, read off the text Decoder.resident_source
    returns: the one place that knows the generator's wording.  U: the set of frames-per-trip values of its look-up loops."""
    reduced, per_lane = "res_flag<PACK>(L_fail, s_" in src, "atomicOr(&L_fail[s_]" in src
    assert reduced != per_lane, "resident kernel source: exit-test flag statement not recognised"
    waves = re.search(r"amdgpu_waves_per_eu\((\d+)", src)
    U = {int(u) for u in re.findall(r"fs \+= (\d+) \* BITS", src)}
    assert U, "resident kernel source: no look-up loop found"
    return {"flag_reduce": int(reduced), "cn_persistent": int(re.search(r"\bint cs_\d", src) is not None), "xcd": int("(nb & 7) == 0" in src),
            "waves_eu": int(waves.group(1)) if waves else 0, "U": U}


def _repair_double_edges(cols, rng, rounds=200):
    """cols[v]: the checks of node v's sockets.  Nodes that got the same check twice swap a socket with a random other node."""
    n = len(cols)
    for _ in range(rounds):
        bad = [v for v in range(n) if len(set(cols[v])) < len(cols[v])]
        if not bad:
            break
        for v in bad:
            for k in range(1, len(cols[v])):
                if cols[v][k] in cols[v][:k]:
                    w = int(rng.integers(n))
                    j = int(rng.integers(len(cols[w])))
                    if cols[w][j] not in cols[v] and cols[v][k] not in cols[w]:
                        cols[v][k], cols[w][j] = cols[w][j], cols[v][k]
    assert all(len(set(c)) == len(c) for c in cols)


def _write_alist(path, col_rows, M):
    """col_rows[v]: the sorted checks of node v.  Returns the check degrees."""
    row_cols = [[] for _ in range(M)]
    for v, rows in enumerate(col_rows):
        for r in rows:
            row_cols[r].append(v)
    with open(path, "w") as f:
        f.write(f"{len(col_rows)} {M}\n{max(len(c) for c in col_rows)} {max(len(r) for r in row_cols)}\n")
        f.write(" ".join(str(len(c)) for c in col_rows) + "\n" + " ".join(str(len(r)) for r in row_cols) + "\n")
        for c in col_rows:
            f.write(" ".join(str(r + 1) for r in c) + "\n")
        for r in row_cols:
            f.write(" ".join(str(v + 1) for v in sorted(r)) + "\n")
    return np.array([len(r) for r in row_cols])


def write_zigzag_runs_alist(path, runs, dv_info, seed=0):
    """A dual-diagonal (IRA / DVB-S2 style) code for the tests: information nodes of degree dv_info dealt to the information sockets
    of the checks, plus one parity node of degree 2 per check in a (tail-biting) zigzag, parity node j joining checks j and j+1.
    runs = [(checks, information sockets per check), ...]: the zigzag passes through contiguous runs of checks of degree
    sockets + 2, so every degree class holds neighbours of the zigzag.  Returns (N, M)."""
    rng = np.random.default_rng(seed)
    per = np.concatenate([np.full(n, s, int) for n, s in runs])
    M = len(per)
    assert per.sum() % dv_info == 0
    K = int(per.sum()) // dv_info
    sockets = np.repeat(np.arange(M), per)
    rng.shuffle(sockets)
    cols = [list(c) for c in sockets.reshape(K, dv_info)]
    _repair_double_edges(cols, rng)
    col_rows = [sorted(int(r) for r in c) for c in cols] + [sorted({j, (j + 1) % M}) for j in range(M)]
    _write_alist(path, col_rows, M)
    return K + M, M


def write_ira_alist(path, K, M, dv_info, seed=0):
    """The zigzag code with one run: K information nodes of degree dv_info spread evenly over M checks, check degree
    K*dv_info/M + 2.  Returns (N, M)."""
    assert (K * dv_info) % M == 0
    return write_zigzag_runs_alist(path, [(M, K * dv_info // M)], dv_info, seed)


def write_random_alist(path, N, M, dv_choices, dv_probs, seed=0):
    """A random irregular code for the fuzz tests: variable degrees drawn from dv_choices with dv_probs, edges dealt to the M
    checks as evenly as possible (check degrees differ by at most one), double edges repaired by swapping sockets.
    Returns (dv, dc) as arrays."""
    rng = np.random.default_rng(seed)
    dv = rng.choice(dv_choices, size=N, p=dv_probs).astype(int)
    E = int(dv.sum())
    sockets = np.arange(E) % M                                  # check of every socket: degrees E // M or E // M + 1
    rng.shuffle(sockets)
    ptr = np.concatenate([[0], np.cumsum(dv)])
    cols = [list(sockets[ptr[v]:ptr[v + 1]]) for v in range(N)]
    _repair_double_edges(cols, rng)
    dc = _write_alist(path, [sorted(int(r) for r in c) for c in cols], M)
    assert dc.min() >= 2
    return dv, dc


def write_degree_alist(path, vdeg, cdeg, seed=0):
    """A configuration-model code with a prescribed degree distribution on both sides: vdeg / cdeg map a degree to the number of
    variable / check nodes that have it (equal edge totals).  Nodes are numbered by ascending degree; double edges repaired by
    swapping sockets.  Returns (dv, dc) as arrays."""
    rng = np.random.default_rng(seed)
    dv = np.concatenate([np.full(n, d, int) for d, n in sorted(vdeg.items())])
    dc = np.concatenate([np.full(n, d, int) for d, n in sorted(cdeg.items())])
    assert dv.sum() == dc.sum(), (int(dv.sum()), int(dc.sum()))
    sockets = np.repeat(np.arange(len(dc)), dc)
    rng.shuffle(sockets)
    ptr = np.concatenate([[0], np.cumsum(dv)])
    cols = [list(sockets[ptr[v]:ptr[v + 1]]) for v in range(len(dv))]
    _repair_double_edges(cols, rng)
    got = _write_alist(path, [sorted(int(r) for r in c) for c in cols], len(dc))
    assert (got == dc).all()
    return dv, dc
