"""Cases and references of the sparse triangular encoder (LDPC_Generator_Systematic's sparse form, lutldpc_decoder_set_sparse_generator),
shared by tests/test_sparse_encoder_cpu.py (the host form, the refusals, and that the lists hold what they claim) and
tests/test_59_sparse_encoder_gpu.py (holds the kernels to the references through the C-ABI).  The references are plain numpy: a peel of
H written here on its own, and forward substitution over bit columns.  All integer, equal bit for bit.

The zigzag codes are those of helpers.write_zigzag_runs_alist with the zigzag OPENED: the helper's zigzag is tail-biting (parity node
M-1 joins checks M-1 and 0), which makes the parity part of H singular -- every parity column has two entries, none peels -- so such
a code has no sparse form at all.  Opened, the last parity node has degree 1, as in DVB-S2, and T is the dual diagonal."""
from __future__ import annotations

import functools

import numpy as np

import encode_cases as ec

# ---------------------------------------------------------------------------------------------------------------- codes of the host form
# name -> (runs of (checks, information sockets per check), information degree, seed): N = 200, 410, 1000
ZIGZAG_CODES = {
    "ira200": ([(100, 3)], 3, 11),
    "runs410": ([(60, 4), (90, 6)], 3, 12),
    "ira1000": ([(500, 3)], 3, 13),
}
DVBS2 = "rate0.50_irreg_dvbs2_N64800"
TWIN = "rate0.50_dv02-08_dc07-08_lut_q4_N64800"       # same size, parity part of column degrees 3 and 8: nothing peels


def write_open_zigzag_alist(path, runs, dv_info, seed=0):
    """helpers.write_zigzag_runs_alist with the zigzag opened: parity node j joins checks j and j + 1, the last one check M - 1 alone.
    Returns (N, M)."""
    from helpers import _repair_double_edges, _write_alist
    rng = np.random.default_rng(seed)
    per = np.concatenate([np.full(n, s, int) for n, s in runs])
    M = len(per)
    assert per.sum() % dv_info == 0
    K = int(per.sum()) // dv_info
    sockets = np.repeat(np.arange(M), per)
    rng.shuffle(sockets)
    cols = [list(c) for c in sockets.reshape(K, dv_info)]
    _repair_double_edges(cols, rng)
    col_rows = [sorted(int(r) for r in c) for c in cols] + [[j, j + 1] if j + 1 < M else [j] for j in range(M)]
    _write_alist(path, col_rows, M)
    return K + M, M


def zigzag_alist(name, directory):
    """The alist of a ZIGZAG_CODES entry, written into `directory` on first use: (path, N, M)."""
    from pathlib import Path
    runs, dv, seed = ZIGZAG_CODES[name]
    path = Path(directory) / f"{name}.alist"
    M = sum(n for n, _ in runs)
    N = sum(n * s for n, s in runs) // dv + M
    if not path.exists():
        assert write_open_zigzag_alist(path, runs, dv, seed) == (N, M)
    return path, N, M


def peel(H, K):
    """The sparse form of H = [A | T] (uint8 [M, N], M = N - K) in numpy: (row_ptr, cols, peeled).  A column of T peels when it has
    exactly one entry among the checks not yet removed; parity bit K + i = XOR of the other entries of its defining check."""
    M, N = H.shape
    alive = np.ones(M, bool)
    define = np.full(N - K, -1)
    while True:
        cnt = H[alive][:, K:].sum(axis=0)
        cand = np.flatnonzero((cnt == 1) & (define < 0))
        if not len(cand):
            break
        for i in cand:
            rows = np.flatnonzero(alive & (H[:, K + i] == 1))
            if len(rows) == 1 and define[i] < 0:
                define[i] = rows[0]
                alive[rows[0]] = False
    peeled = int((define >= 0).sum())
    if peeled != N - K:
        return None, None, peeled
    row_ptr, cols = [0], []
    for i in range(N - K):
        cols += [int(v) for v in np.flatnonzero(H[define[i]]) if v != K + i]
        row_ptr.append(len(cols))
    return np.array(row_ptr, np.int32), np.array(cols, np.int32), peeled


# ---------------------------------------------------------------------------------------------------------------- forward substitution
def chain_order(K, R, row_ptr, cols):
    """A topological order of the parity bits (every parity term of a bit before it): depth-first, iterative; not the library's order."""
    state = np.zeros(R, np.int8)
    order = []
    for s in range(R):
        stack = [s]
        while stack:
            i = stack[-1]
            if state[i] == 2:
                stack.pop()
                continue
            state[i] = 1
            need = [int(v) - K for v in cols[row_ptr[i]:row_ptr[i + 1]] if v >= K and state[int(v) - K] != 2]
            if not need:
                state[i] = 2
                order.append(i)
                stack.pop()
            else:
                assert all(state[j] == 0 for j in need), "dependency cycle"
                stack += need
    return order


def forward_substitute(K, R, row_ptr, cols, u):
    """[u | p] uint8 [B, K + R] for information bits u[B, K]: every parity bit, in a solve order, as the XOR of its terms."""
    cw = np.zeros((len(u), K + R), np.uint8)
    cw[:, :K] = u
    for i in chain_order(K, R, row_ptr, cols):
        t = cols[row_ptr[i]:row_ptr[i + 1]]
        cw[:, K + i] = np.bitwise_xor.reduce(cw[:, t], axis=1) if len(t) else 0
    return cw


def depth(K, R, row_ptr, cols):
    """Bits on the longest chain of parity-on-parity dependencies (0: no parity bit)."""
    lev = np.zeros(R, np.int64)
    for i in chain_order(K, R, row_ptr, cols):
        t = cols[row_ptr[i]:row_ptr[i + 1]]
        t = t[t >= K] - K
        lev[i] = 1 + (lev[t].max() if len(t) else 0)
    return int(lev.max()) if R else 0


# ---------------------------------------------------------------------------------------------------------------- synthetic systems
BLOCK = 64                                          # the block the cases are laid out for; the GPU test reads the library's from describe()
KINDS = ("chain", "permuted", "short_chains")
# (handle of frontend_cases.HANDLES, K, R, kind): the N = 1000 code in both row formats and N = 10000; K at 1, 31, 32, 33 and off the
# word grid, R = 1, and a chain of 5000 bits
SYSTEM_CASES = [(h, K, 1000 - K, kind) for h in ("q4", "q4_pack1") for K, kind in
                ((1, "chain"), (31, "permuted"), (32, "short_chains"), (33, "permuted"), (500, "chain"), (500, "permuted"), (700, "short_chains"), (999, "chain"))] + \
               [("n10000", 5000, 5000, "chain"), ("n10000", 3001, 6999, "permuted")]
BATCHES = (1, 63, 64, 65, 127, 128, 129, 130)       # the 64-frame wave step and the 128-frame slice of the solve, each at, under and over
WIDE_ROW = 40


def system_id(case):
    return f"{case[0]}-K{case[1]}-R{case[2]}-{case[3]}"


@functools.lru_cache(maxsize=None)
def system(K, R, kind):
    """(row_ptr, cols) int32 of a synthetic system, read-only.  Every kind with R >= 8 holds a row with no terms (parity 0), a row
    with parity terms only and a row of WIDE_ROW terms; the terms of a row are shuffled.
      chain         ONE chain through all R bits: bit i names bit i - 1 (and 0 - 3 information bits)
      permuted      a triangular system with 0 - 4 earlier parity terms per row, reaching into the same block of BLOCK bits, the previous
                    block and the first block, its parity bits renamed by a random permutation
      short_chains  runs of chains of 2 - 7 bits"""
    rng = np.random.default_rng(K * 1009 + R * 7 + KINDS.index(kind))
    rows = []
    start = 0                                       # first bit of the current short chain
    length = int(rng.integers(2, 8))
    for i in range(R):
        info = [int(v) for v in rng.choice(K, size=min(K, int(rng.integers(0, 4))), replace=False)]
        par = []
        if kind == "chain":
            par = [i - 1] if i else []
        elif kind == "short_chains":
            if i - start == length:
                start, length = i, int(rng.integers(2, 8))
            par = [i - 1] if i > start else []
        else:
            reach = []
            if i:
                reach.append(int(rng.integers(i // BLOCK * BLOCK, i)) if i % BLOCK else i - 1)      # same block (or the bit before)
            if i >= BLOCK:
                reach.append(int(rng.integers((i // BLOCK - 1) * BLOCK, i // BLOCK * BLOCK)))       # previous block
                reach.append(int(rng.integers(0, BLOCK)))                                           # first block
            if i > 2:
                reach.append(int(rng.integers(0, i)))
            par = sorted(set(reach[:int(rng.integers(0, 5))])) if i % 5 else sorted(set(reach))
        rows.append((info, par))
    if R >= 8:
        rows[3] = ([], rows[3][1] if kind == "chain" else [])                      # parity terms only (chain) / no terms at all
        rows[5] = ([], [4] if kind != "chain" else rows[5][1])                     # parity terms only
        if kind == "chain":
            rows[0] = ([], [])                                                     # no terms: parity 0
        wide = R - 2
        info = [int(v) for v in rng.choice(K, size=min(K, WIDE_ROW), replace=False)]
        extra = [int(v) for v in rng.choice(wide, size=WIDE_ROW - len(info), replace=False)] if len(info) < WIDE_ROW else []
        rows[wide] = (info, sorted(set(rows[wide][1]) | set(extra)))
    perm = rng.permutation(R) if kind == "permuted" else np.arange(R)              # bit i of the construction is parity bit perm[i]
    by_bit = [None] * R
    for i, (info, par) in enumerate(rows):
        t = np.array(info + [K + int(perm[j]) for j in par], np.int64)
        rng.shuffle(t)
        by_bit[int(perm[i])] = t
    row_ptr = np.zeros(R + 1, np.int32)
    row_ptr[1:] = np.cumsum([len(t) for t in by_bit])
    cols = (np.concatenate(by_bit) if R else np.zeros(0)).astype(np.int32)
    row_ptr.setflags(write=False)
    cols.setflags(write=False)
    return row_ptr, cols


@functools.lru_cache(maxsize=None)
def system_reference(K, R, kind, stride):
    """The codewords uint8 [max(BATCHES), K + R] of ec.info_words(K, stride) (a smaller batch is a prefix), read-only."""
    row_ptr, cols = system(K, R, kind)
    u = ec.unpack(ec.info_words(K, stride)[:max(BATCHES), :(K + 31) // 32], K)
    cw = forward_substitute(K, R, row_ptr, cols, u)
    cw.setflags(write=False)
    return cw


def windows(K, R):
    """ec.windows: full, information only, parity only, straddling K, off the word grid, the last bit, three random ones."""
    return ec.windows(K, R)


def dense_rows(H, K):
    """The dense generator of H = [A | T] as lutldpc_decoder_set_generator takes it: R rows of ceil(K/64) uint64 words."""
    A = ec.systematic_rows(H, K)
    R = A.shape[0]
    padded = np.zeros((R, (K + 63) // 64 * 64), np.uint8)
    padded[:, :K] = A
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").astype(np.uint64).reshape(R, -1)


# ---------------------------------------------------------------------------------------------------------------- refusals
def refusals(K=600, R=400):
    """name -> (K, R, row_ptr or None, cols or None, word the message must hold) for a handle of nvar = K + R: the ERR_ARG list of
    lutldpc_decoder_set_sparse_generator.  cycle: bits K+7 -> K+9 -> K+8 -> K+7."""
    rp, cl = (a.copy() for a in system(K, R, "permuted"))
    def patched(i, v):
        c = cl.copy()
        c[rp[i]] = v
        return c
    rows_with_terms = [i for i in range(R) if rp[i + 1] > rp[i]]
    i0 = rows_with_terms[10]
    down = rp.copy()
    down[i0 + 1] = down[i0] - 1 if down[i0] else down[i0 + 1]
    assert down[i0 + 1] < down[i0]
    cyc_rows = {7: [K + 9], 9: [K + 8], 8: [K + 7]}
    cyc_ptr, cyc_cols = [0], []
    for i in range(R):
        cyc_cols += cyc_rows.get(i, [int(v) for v in cl[rp[i]:rp[i + 1]] if v < K])
        cyc_ptr.append(len(cyc_cols))
    first = rp.copy()
    first[0] = 1
    return {
        "NULL row_ptr": (K, R, None, cl, "NULL"),
        "NULL cols": (K, R, rp, None, "NULL"),
        "K = 0": (0, K + R, np.zeros(K + R + 1, np.int32), cl, "K"),
        "R < 0": (K + R + 1, -1, rp, cl, "R"),
        "K + R != nvar": (K - 1, R, rp, cl, "nvar"),
        "row_ptr not from 0": (K, R, first, cl, "start at 0"),
        "row_ptr descends": (K, R, down, cl, "ascend"),
        "entry = K + R": (K, R, rp, patched(i0, K + R), "outside"),
        "entry < 0": (K, R, rp, patched(i0, -1), "outside"),
        "own bit": (K, R, rp, patched(i0, K + i0), "own bit"),
        "cycle": (K, R, np.array(cyc_ptr, np.int32), np.array(cyc_cols, np.int32), "cycle through bit"),
    }
