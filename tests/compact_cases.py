"""The cases of the batch entries behind a decode that compacts its frames, shared by tests/test_60_entries_behind_compaction_gpu.py
(every entry of the C-ABI against its reference on the GPU) and tests/test_compact_cases_cpu.py (describe() on host-only handles and
the oracle alone: the cases are on the path they name, and their inputs make frames move).  Compaction is the one thing that moves
frames between slots during a decode (launch_compaction permutes the message rows and the channel-label rows; launch_uncompaction
brings back the decided bits and the iteration codes only): it needs the streaming, skewed path and at least four frame groups, so
the short codes of the front-end, statistics, packed and LLR tests never reach it."""
from __future__ import annotations

import functools

import numpy as np

import frontend_cases as fc
from helpers import designed_codec, oracle_codec, planted_labels, product_decoder, write_ira_alist

# ---- the code: the dual-diagonal code of tests/test_05 and tests/test_55 (check degree 8: bucket 0 of the fused kernel, chain-rich)
K, M, DV, ITERS, SIGMA, SNR_OFFSET = 840, 420, 3, 16, 0.62, 0.25
N = K + M
# the parity zigzag is tail-biting (parity node j joins checks j and j + 1 mod M), so the checks sum to zero over the information part
# only for data of even weight: K - 1 free data bits, the last information node is their parity, then the running sums of the checks
K_INFO, R_GEN = K - 1, M + 1

# ---- the knobs.  A check point after the exit test of every second iteration from iteration 2 on, no cost margin: a permutation
#      happens whenever it frees a group
BASE = {"LUTLDPC_RESIDENT": "0", "LUTLDPC_COMPACT": "1", "LUTLDPC_COMPACT_FIRST": "2", "LUTLDPC_COMPACT_EVERY": "2", "LUTLDPC_COMPACT_MARGIN": "0"}
CHECK_POINTS = [cp for cp in range(2, ITERS, 2) if cp < ITERS - 2]
#      variant -> knobs beside BASE: nibble / byte rows, decided bits late (the frames that left keep their rows) / stored by every
#      pass (they drop them)
VARIANTS = {
    "base": {},
    "pack1": {"LUTLDPC_PACK": "1"},
    "late0": {"LUTLDPC_LATE_HARD": "0"},
    "late0_pack1": {"LUTLDPC_LATE_HARD": "0", "LUTLDPC_PACK": "1"},
}
FULL_MATRIX = ("base", "pack1")            # every entry; the other variants: the decode entries and sim_batch
OTHER = tuple(v for v in VARIANTS if v not in FULL_MATRIX)


def knobs(variant):
    return dict(BASE, **VARIANTS[variant])


def tile(variant):
    return 256 if "LUTLDPC_PACK" in VARIANTS[variant] else 512


# ---- the batches.  six: six groups, halves of three, ragged last group; four: four groups, the least compaction_on accepts
def batch(variant, which):
    return {"six": 5, "four": 3}[which] * tile(variant) + 77


BATCHES = ("six", "four")
SIZES = sorted({batch(v, w) for v in VARIANTS for w in BATCHES})      # 845, 1357, 1613, 2637
#      label seed of every batch size: the size itself (as tests/test_05), unless test_compact_cases_cpu.py asks for another
LABEL_SEED = {B: B for B in SIZES}

# ---- the front end: frames F0 .. of (SEED, STREAM) at the SNR of the batches
SEED, STREAM, F0 = 2 ** 40 + 60, 6, 2 ** 32 - 9
SOURCES = ("zero", "codewords")            # the all-zero codeword / codewords of the generator below


def codec():
    """The code, designed with the oracle (as _ira_codec of tests/test_05)."""
    cd = designed_codec("compact-ira", lambda path: write_ira_alist(path, K, M, DV, seed=K + ITERS), sigma=SIGMA, max_iters=ITERS, nq_msg=16)
    assert cd.code.nvar == N
    return cd


def snr():
    return -10 * np.log10(2 * codec().rate * SIGMA * SIGMA) + SNR_OFFSET


def planted(B):
    return [0, B // 2, B - 1]


@functools.lru_cache(maxsize=None)
def labels(B):
    """Channel and initial-message labels of a batch, three noise-free frames planted (first, middle, last: they pass the test on the
    channel decisions, so the pisc exit and hard_from_labels_masked_kernel have work).  Shared read-only."""
    return planted_labels(codec(), B, snr(), LABEL_SEED[B], noise_free=planted(B))


ORACLE = {}      # (labels id, frames, psc, pisc) -> (bits, iteration codes): the oracle decodes each batch once per exit mode


def oracle_decode(key, cha, msg, psc=True, pisc=True):
    """The oracle's flat-table decode (bit-identical to its faithful mode: tests/test_oracle_flat.py) of the labels `key` names."""
    k = (key, len(cha), bool(psc), bool(pisc))
    if k not in ORACLE:
        cd = codec()
        cd.set_exit_conditions(ITERS, psc, pisc)
        bits, it = cd.lut_decode_batch_flat(cha, msg)
        bits.setflags(write=False)
        it.setflags(write=False)
        ORACLE[k] = (bits, it)
    return ORACLE[k]


def want(B, psc=True, pisc=True):
    return oracle_decode("awgn", *labels(B), psc, pisc)


# ---- codewords.  Nodes 0 .. K-1 are the information nodes, node K + j the parity node of checks j and j + 1 mod M
@functools.lru_cache(maxsize=None)
def _info_checks():
    """[M, K] 0/1: information node k is in check c (from the code's own graph)."""
    c = codec().code
    node_of_edge = np.repeat(np.arange(N), np.asarray(c.dv, np.int64))[np.asarray(c.cn_msg_idx, np.int64)]
    check_of_slot = np.repeat(np.arange(M), np.asarray(c.dc, np.int64))
    H = np.zeros((M, N), np.uint8)
    H[check_of_slot, node_of_edge] = 1
    assert (H[:, K:].sum(0) == 2).all() and all(H[j, K + j] and H[(j + 1) % M, K + j] for j in range(M))
    return H[:, :K]


def encode_data(u):
    """[B, K_INFO] data bits -> [B, N] codewords: node K-1 makes the weight of the information part even, parity node j is the
    running sum of checks 0 .. j over it (parity node M-1, the sum of all checks, is then 0 and closes the ring)."""
    u = np.asarray(u, np.int64)
    info = np.concatenate([u, u.sum(1, keepdims=True) & 1], axis=1)
    s = (info.astype(np.float64) @ _info_checks().T.astype(np.float64)).astype(np.int64) & 1
    return np.concatenate([info, np.cumsum(s, axis=1) & 1], axis=1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def generator_rows():
    """The R_GEN rows of lutldpc_decoder_set_generator (ceil(K_INFO / 64) uint64 words each, bit j of word w = data bit 64 w + j):
    the encoder above is linear, its matrix is what it makes of the unit vectors."""
    A = encode_data(np.eye(K_INFO, dtype=np.uint8))[:, K_INFO:].T            # [R_GEN, K_INFO]
    W = (K_INFO + 63) // 64
    bits = np.zeros((R_GEN, 64 * W), np.uint64)
    bits[:, :K_INFO] = A
    rows = (bits.reshape(R_GEN, W, 64) << np.arange(64, dtype=np.uint64)[None, None, :]).sum(2, dtype=np.uint64)
    assert (fc.generator_bits(rows, K_INFO) == A).all()
    return np.ascontiguousarray(rows)


@functools.lru_cache(maxsize=None)
def codewords(B):
    """The codewords the device encoder makes of frames F0 .. F0 + B - 1 (frontend_cases.info_bits: the Philox data bits)."""
    cw = encode_data(fc.info_bits(SEED, STREAM, F0, B, K_INFO))
    cw.setflags(write=False)
    return cw


@functools.lru_cache(maxsize=None)
def sampled(B, source, frame0=F0):
    """(cha, msg, uncoded errors) of the oracle's sampler for frames frame0 .. of (SEED, STREAM); source "codewords": over the
    codewords of those frames.  Shared read-only."""
    cd = codec()
    cw = None
    if source == "codewords":
        assert frame0 >= F0
        cw = codewords(frame0 - F0 + B)[frame0 - F0:]
    out = cd.sample_labels(snr(), cd.rate, SEED, STREAM, frame0, B, cw)
    for a in out:
        a.setflags(write=False)
    return out


def want_sampled(B, source, psc=True, pisc=True):
    cha, msg, _ = sampled(B, source)
    return oracle_decode("sampled-" + source, cha, msg, psc, pisc)


def cells():
    cd = codec()
    return cd.channel_cells(snr(), cd.rate)


# ---- the boundary of compaction_fits (kPermuteMaxGroups = 32 groups per half): n500_q4_i8 in byte rows
#      (8 iterations: check points after iterations 2 and 4; at 6 dB a tenth of the frames has left by the first, the oracle says)
FITS_CODE, FITS_TILE, FITS_SNR, FITS_CHECK_POINTS = "n500_q4_i8", 256, 6.0, (2, 4)
FITS_KNOBS = {"LUTLDPC_RESIDENT": "0", "LUTLDPC_PACK": "1", "LUTLDPC_COMPACT": "1", "LUTLDPC_COMPACT_FIRST": "2", "LUTLDPC_COMPACT_EVERY": "2",
              "LUTLDPC_COMPACT_MARGIN": "0"}
FITS_B = {"fits": 64 * 256, "beyond": 65 * 256 + 3}           # halves of 32 groups: compaction runs / of 33: it cannot


# ---- what describe() must say, and what the oracle's iteration codes must show
def describe(kn, monkeypatch, device=-1, cd=None):
    """(decoder, describe()) of the code created with the knobs kn (read once, at creation) and no other LUTLDPC_ variable."""
    import os
    for k in [k for k in os.environ if k.startswith("LUTLDPC_") and k not in ("LUTLDPC_LIB", "LUTLDPC_DESIGN_CACHE")]:
        monkeypatch.delenv(k)
    for k, v in kn.items():
        monkeypatch.setenv(k, v)
    dec = product_decoder(cd or codec(), device=device)
    return dec, dec.describe()


def check_path(variant, desc, sizes):
    """The handle is on the path the case names: streaming, skewed, chain-fused, compaction forced on, the row format, and every
    batch of `sizes` reaches the check points."""
    T = tile(variant)
    want_ = {"resident": 0, "skewed_pipeline": 1, "compaction": 1, "pack": 1 if T == 256 else 2, "tile_frames": T}
    assert {k: desc[k] for k in want_} == want_, (variant, {k: desc[k] for k in want_})
    assert desc["chain_nodes"] >= M // 2, desc["chain_nodes"]
    for B in sizes:
        assert 4 <= desc["compaction_min_groups"] <= -(-B // T), (variant, B, desc["compaction_min_groups"])


def halves(B, T):
    """The frame ranges of the two halves of the skewed pipeline: [0, ceil(G/2) T) and the rest."""
    G = -(-B // T)
    cut = (G + 1) // 2 * T
    return (0, cut), (cut, B)


def moves(it, B, T, check_points=CHECK_POINTS):
    """Per half, the check points at which the frames still active (code < 0 or code > cp) fit fewer groups than were live before:
    a permutation that frees a group.  [(check point, groups before, groups after), ...] for each half."""
    out = []
    for lo, hi in halves(B, T):
        codes = np.asarray(it[lo:hi])
        live, ev = -(-(hi - lo) // T), []
        for cp in check_points:
            need = -(-int(((codes < 0) | (codes > cp)).sum()) // T)
            if need < live:
                ev.append((cp, live, need))
                live = need
        out.append(ev)
    return out


def fits_codec():
    return oracle_codec(FITS_CODE)


@functools.lru_cache(maxsize=None)
def fits_labels(which):
    B = FITS_B[which]
    return planted_labels(fits_codec(), B, FITS_SNR, B, noise_free=planted(B))


@functools.lru_cache(maxsize=None)
def fits_want(which):
    cd = fits_codec()
    cd.set_exit_conditions(cd.max_iters, True, True)
    bits, it = cd.lut_decode_batch_flat(*fits_labels(which))
    return bits, it
