"""References and cases of the Monte-Carlo front end (Philox cell sampler, device encoder, sent-bit rows, error counters), shared by
tests/test_frontend_exact_cpu.py (holds the references to published Philox vectors and the oracle to the references, and checks that
every crafted table does what it is for, with the references alone) and tests/test_21_frontend_limits_gpu.py (holds the kernels to
the references through the C-ABI).  The references are plain numpy and use no code of the product or of the oracle; only the codes
and the two real cell tables come from the oracle, as in streaming_cases.py.  Everything is integer: equal bit for bit, no tolerance.

Cell tables are dicts {"thr": uint64[max(n-1, 1)], "cha", "msg", "neg", "cha_m", "msg_m": uint8[n]} (n cells; thr beyond n-1 unused).
The crafted ones are cut from the reference's own uniforms of the (seed, stream, frame0, B, N) they run with, so that samples tie
thresholds and every cell that should be hit is hit by construction; their labels name the cell, so a wrong cell is a wrong label."""
from __future__ import annotations

import functools

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
TWO64 = 1 << 64
BUCKET_BITS = 10                                   # kernels_frontend.hpp: kBucketBits, 1024 slices of the unit interval
SLICE = 1 << (64 - BUCKET_BITS)

# Philox4x32-10 known answers of the Random123 distribution (kat_vectors): (counter, key, output)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


# ---------------------------------------------------------------------------------------------------------------- references
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays of 32-bit words held in uint64 (broadcast); returns the four output words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, np.uint64) & M32 for x in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2            # 32 x 32 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & M32, (p0 >> S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def frames(frame0, B):
    """The global frame indices of a batch: (frame0 + i) mod 2^64, as the C-ABI's uint64 arithmetic."""
    return np.array([(int(frame0) + i) % TWO64 for i in range(B)], np.uint64)


def uniforms(seed, stream, frame0, B, N):
    """u[B, N] uint64: counter (f lo, f hi, p, stream), key (seed lo, seed hi); node 2p takes c1<<32|c0, node 2p+1 c3<<32|c2."""
    f = frames(frame0, B)[:, None]
    p = np.arange((N + 1) // 2, dtype=np.uint64)[None, :]
    c = philox4x32_10(f & M32, f >> S32, p, np.uint64(stream), np.uint64(int(seed) & 0xFFFFFFFF), np.uint64(int(seed) >> 32))
    u = np.empty((B, 2 * p.shape[1]), np.uint64)
    u[:, 0::2] = (c[1] << S32) | c[0]
    u[:, 1::2] = (c[3] << S32) | c[2]
    return np.ascontiguousarray(u[:, :N])


def cells_of(cells, u):
    """cell = number of thresholds <= u."""
    n = len(cells["cha"])
    return np.searchsorted(cells["thr"][:n - 1], u, side="right")


def sample(cells, seed, stream, frame0, B, N, codewords=None, u=None):
    """(cha, msg, uncoded errors) of the sampler: the cell's labels, the mirrored ones where the sent bit (bit 0 of the byte) is 1;
    uncoded errors = the cells on the negative side, whatever the sent bit (the slicer errs on the mirrored cell of a sent 1)."""
    u = uniforms(seed, stream, frame0, B, N) if u is None else u
    cell = cells_of(cells, u)
    cha, msg = cells["cha"][cell], cells["msg"][cell]
    if codewords is not None:
        one = (np.asarray(codewords).reshape(B, N) & 1).astype(bool)
        cha, msg = np.where(one, cells["cha_m"][cell], cha), np.where(one, cells["msg_m"][cell], msg)
    return cha.astype(np.uint8), msg.astype(np.uint8), cells["neg"][cell].astype(np.int64).sum(1).astype(np.int32)


def info_bits(seed, stream, frame0, B, K):
    """[B, K] uint8: counter (f lo, f hi, k // 128, stream | 0x80000000); bit k = bit k % 32 of output word (k % 128) // 32."""
    f = frames(frame0, B)[:, None]
    blk = np.arange((K + 127) // 128, dtype=np.uint64)[None, :]
    c = philox4x32_10(f & M32, f >> S32, blk, np.uint64(int(stream) | 0x80000000), np.uint64(int(seed) & 0xFFFFFFFF), np.uint64(int(seed) >> 32))
    words = np.stack(c, axis=2).reshape(B, -1)                                          # [B, 4 * blocks]: word (k % 128) // 32 of block k // 128
    bits = (words[:, :, None] >> np.arange(32, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    return bits.reshape(B, -1)[:, :K].astype(np.uint8)


def generator_bits(rows, K):
    """The R x K matrix of generator rows given as ceil(K/64) uint64 words each (bit j of word w = information bit 64w + j), bits at
    positions >= K masked off."""
    rows = np.asarray(rows, np.uint64).reshape(-1, (K + 63) // 64)
    bits = (rows[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    return bits.reshape(len(rows), 64 * rows.shape[1])[:, :K].astype(np.uint8)


def encode(A_bits, u):
    """[u | (A u) mod 2] in int64 for information words u[B, K].  The product runs in float64, exact for sums up to K < 2^53."""
    u = np.asarray(u, np.int64)
    par = (u.astype(np.float64) @ np.asarray(A_bits, np.float64).T).astype(np.int64) % 2 if len(A_bits) else np.zeros((len(u), 0), np.int64)
    return np.concatenate([u, par], axis=1)


# ---------------------------------------------------------------------------------------------------------------- cell tables
def _coprime_step(n):
    return next(m for m in (5, 7, 11, 13, 17) if np.gcd(m, n) == 1)


def labelled(thr, nq):
    """The table of ascending thresholds thr (n = len + 1 cells): cell j carries (cha, msg) = (j % nq, j // nq), its mirror the labels
    of cell (m j + 3) % n (m coprime to n: another bijection), neg an irregular bit pattern."""
    thr = np.asarray(thr, np.uint64)
    n = len(thr) + 1
    assert n <= 72 and (n - 1) // nq < nq and all(a <= b for a, b in zip(thr[:-1], thr[1:]))
    j = np.arange(n)
    jm = (_coprime_step(n) * j + 3) % n
    neg = ((0x9A6C35 >> (j % 24)) & 1).astype(np.uint8)
    return {"thr": thr if len(thr) else np.array([0xDEADBEEFDEADBEEF], np.uint64), "cha": (j % nq).astype(np.uint8), "msg": (j // nq).astype(np.uint8),
            "neg": neg, "cha_m": (jm % nq).astype(np.uint8), "msg_m": (jm // nq).astype(np.uint8)}


def pin_samples(B, N, T, frame0):
    """The (frame, node) samples whose 64-bit uniform the table `pins` proves: first and last frame, first and last frame of a lane
    (a lane holds T/64 consecutive frames), both sides of a frame-group boundary, the frame whose low index word wraps and the one
    before it, each at the first and last nodes (the last node of an odd N has no partner in its Philox block) and one in the
    middle; filled up to 35 from a fixed random draw."""
    F = T // 64
    fr = [0, B - 1, F - 1, F, 63 * F, 64 * F - 1, T - 1, T, 2 * T - 1, 2 * T, B - 2]
    wrap = (1 << 32) - int(frame0) % (1 << 32)
    fr = [wrap - 1, wrap] + fr if int(frame0) % (1 << 32) else fr
    fr = list(dict.fromkeys(i for i in fr if 0 <= i < B))
    nodes = list(dict.fromkeys(v for v in (N - 1, 0, 1, N - 2, N // 2) if 0 <= v < N))
    out = [(i, v) for v in nodes for i in fr][:35]
    rng = np.random.default_rng(35)
    while len(out) < 35:
        s = (int(rng.integers(B)), int(rng.integers(N)))
        if s not in out:
            out.append(s)
    return out


def table_pins(u, nq, T, frame0):
    """72 cells: the threshold pairs (u_i, u_i + 1) of 35 chosen samples and one more threshold.  The cell between a pair holds
    exactly the samples whose uniform EQUALS u_i, so the device's label there proves all 64 bits of its uniform."""
    B, N = u.shape
    assert B * N >= 35
    picks = pin_samples(B, N, T, frame0)
    vals = sorted({int(u[i, v]) for i, v in picks})
    assert len(vals) == 35 and vals[-1] < TWO64 - 1 and all(b - a > 1 for a, b in zip(vals, vals[1:]))
    thr = sorted([x for v in vals for x in (v, v + 1)] + [(1 << 63) + 12345])
    return labelled(thr, nq), picks


def table_one_bucket(u, nq):
    """72 cells whose 71 thresholds all lie inside ONE of the sampler's 1024 slices (the fullest one): every k-th of the sorted uniforms
    that fall into it.  Every threshold is tied by a sample and every cell is hit."""
    srt = np.unique(u)
    cnt = np.bincount((srt >> np.uint64(64 - BUCKET_BITS)).astype(np.int64), minlength=1 << BUCKET_BITS)
    s = int(cnt.argmax())
    inside = srt[(srt >> np.uint64(64 - BUCKET_BITS)) == np.uint64(s)]
    assert len(inside) >= 71, len(inside)
    return labelled(inside[::len(inside) // 71][:71], nq), s


BOUNDARY_KS = (1, 2, 300, 511, 512, 513, 1022, 1023)


def table_boundaries():
    """Thresholds on the lower end of a slice, one below and one above it (k << 54 and its neighbours, k = 1 and 1023 among them), 0
    (cell 0 unreachable), 2^64 - 1 (the last cell holds that one value) and three equal thresholds in a row (two empty cells).
    Returns (thresholds, the cells no 64-bit value or only a single one can reach: predicted empty)."""
    thr = [0]
    for k in BOUNDARY_KS:
        thr += [(k << 54) - 1, k << 54, (k << 54) + 1]
    thr += [(700 << 54) + 98765] * 3 + [TWO64 - 1]
    thr = sorted(thr)
    width = np.diff(np.array([0] + thr + [TWO64], dtype=object))                    # cell j = [thr[j-1], thr[j])
    return thr, [j for j, w in enumerate(width) if w <= 1]


def crafted(table, u, nq, T, frame0):
    """One crafted table for the uniforms u of its run."""
    if table == "pins":
        return table_pins(u, nq, T, frame0)[0]
    if table == "one_bucket":
        return table_one_bucket(u, nq)[0]
    if table == "boundaries":
        return labelled(table_boundaries()[0], nq)
    if table == "trivial1":
        return labelled([], nq)                                                          # one cell: thr non-null, its content unused
    if table == "trivial2":
        return labelled([1 << 63], nq)
    raise KeyError(table)


def cell_table(table, u, nq, T, frame0):
    return real_dense(table) if table in REAL_DENSE else crafted(table, u, nq, T, frame0)


# the project's own tables at 12 dB: name -> (configuration of helpers.CONFIGS, thresholds in the fullest slice)
REAL_DENSE = {"dense_q4": ("n500_q4_i8", 15), "dense_q6": ("reg36_n1000_q6", 62)}
DENSE_SNR = 12.0


@functools.lru_cache(maxsize=None)
def real_dense(table):
    from helpers import oracle_codec
    cd = oracle_codec(REAL_DENSE[table][0])
    cd.set_initial_message_mode(0)
    t = cd.channel_cells(DENSE_SNR, cd.rate)
    return {k: np.ascontiguousarray(v) for k, v in t.items()}


def thresholds_per_slice(cells):
    n = len(cells["cha"])
    return np.bincount((cells["thr"][:n - 1] >> np.uint64(64 - BUCKET_BITS)).astype(np.int64), minlength=1 << BUCKET_BITS)


# ---------------------------------------------------------------------------------------------------------------- codes, handles
ITERS, GRAPH_SEED = 5, 21
# the two odd-N codes: name -> (variable degree: nodes, check degree: nodes, design sigma).  n127: 64 pairs, the last one half
# empty; n33: 17 pairs, fewer than the 32 one workgroup of the sampler covers
SYNTHETIC = {"n127": ({3: 127}, {3: 1, 6: 63}, 0.80), "n33": ({2: 33}, {6: 11}, 0.55)}
# handle -> (code, environment at creation, frames per group T)
HANDLES = {
    "q4": ("reg36_n1000_q4", {}, 512),                          # nibble rows
    "q4_pack1": ("reg36_n1000_q4", {"LUTLDPC_PACK": "1"}, 256),      # byte rows by request
    "q5": ("reg36_n1000_q5", {}, 256),                          # byte rows by alphabet
    "q6": ("reg36_n1000_q6", {}, 256),                          # (only for the 64-label dense table)
    "n127": ("n127", {}, 512),
    "n127_pack1": ("n127", {"LUTLDPC_PACK": "1"}, 256),
    "n33": ("n33", {}, 512),
    "n10000": ("reg36_n10000_q4", {}, 512),                     # (only for the generator at the LDS limit)
}


def codec(code):
    """The oracle-designed code of a handle."""
    from helpers import designed_codec, oracle_codec, write_degree_alist
    if code not in SYNTHETIC:
        return oracle_codec(code)
    vdeg, cdeg, sig = SYNTHETIC[code]
    return designed_codec("frontend-" + code, lambda path: write_degree_alist(path, vdeg, cdeg, seed=GRAPH_SEED), sigma=sig, max_iters=ITERS, nq_msg=16)


def batch_size(kind, T):
    return {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3}[kind]


F_CARRY, F_HIGH, F_WRAP = 2 ** 32 - 7, 2 ** 33 + 3, 2 ** 64 - 5      # carry into the high word inside the batch; high word set; 2^64 wrap (B >= 12)
SEED_BIG, STREAM_MAX = 2 ** 40 + 5, 2 ** 31 - 1

# sampler cases: (handle, table, batch size, frame0, seed, stream).  Every table runs on an odd-N code, in both row formats and at
# a B that is no multiple of T; the tables that need tens of samples per slice run at the larger batches.
SAMPLER_CASES = [
    ("n127", "pins", "2T+3", F_CARRY, 3, 0),
    ("n127", "one_bucket", "2T+3", 0, SEED_BIG, 7),
    ("n127", "boundaries", "T+1", F_HIGH, 3, STREAM_MAX),
    ("n127", "trivial1", "1", 0, 3, 7),
    ("n127", "trivial2", "T-1", F_WRAP, SEED_BIG, 0),
    ("n127", "dense_q4", "T+1", F_WRAP, 3, 7),
    ("n127_pack1", "pins", "T+1", F_CARRY, SEED_BIG, STREAM_MAX),
    ("n127_pack1", "boundaries", "2T+3", 0, 3, 0),
    ("n33", "pins", "T+1", F_CARRY, SEED_BIG, 7),
    ("n33", "boundaries", "2T+3", F_WRAP, 3, 0),
    ("n33", "trivial2", "1", F_HIGH, 3, STREAM_MAX),
    ("n33", "trivial1", "T+1", 0, SEED_BIG, 0),
    ("n33", "dense_q4", "T", F_CARRY, 3, 7),
    ("q4", "pins", "2T+3", F_CARRY, SEED_BIG, 7),
    ("q4", "one_bucket", "T+1", F_HIGH, 3, STREAM_MAX),
    ("q4", "boundaries", "T-1", F_WRAP, SEED_BIG, 0),
    ("q4", "trivial1", "T", 0, 3, 0),
    ("q4", "dense_q4", "1", F_HIGH, SEED_BIG, 7),
    ("q4_pack1", "pins", "T+1", F_CARRY, 3, 0),
    ("q4_pack1", "one_bucket", "2T+3", F_WRAP, SEED_BIG, 7),
    ("q4_pack1", "boundaries", "T", F_HIGH, 3, 7),
    ("q4_pack1", "trivial2", "T+1", F_CARRY, SEED_BIG, STREAM_MAX),
    ("q4_pack1", "dense_q4", "T-1", 0, 3, STREAM_MAX),
    ("q5", "pins", "2T+3", F_WRAP, 3, STREAM_MAX),
    ("q5", "one_bucket", "T+1", 0, SEED_BIG, 0),
    ("q5", "boundaries", "2T+3", F_CARRY, SEED_BIG, 7),
    ("q5", "dense_q4", "T+1", F_HIGH, 3, 0),
    ("q5", "trivial1", "T-1", F_HIGH, 3, 7),
    ("q6", "dense_q6", "T+1", F_CARRY, 3, 7),
    ("q6", "dense_q6", "1", F_WRAP - 20, SEED_BIG, 0),
]
TABLES = ["pins", "one_bucket", "boundaries", "trivial1", "trivial2", "dense_q4", "dense_q6"]


def case_id(case):
    h, t, b, f0, seed, stream = case
    return f"{h}-{t}-B{b}-f{'0' if f0 == 0 else 'carry' if f0 == F_CARRY else 'high' if f0 == F_HIGH else 'wrap'}-s{seed % 97}-st{stream % 97}"


@functools.lru_cache(maxsize=None)
def sampler_case(case):
    """(cells, u, N, B, T, codewords): the table and the reference's uniforms of a case, its random 0/1 codewords and its codewords
    of random bytes (bit 0 of those bytes is not the 0/1 array).  Shared read-only."""
    h, table, bk, f0, seed, stream = case
    code, _, T = HANDLES[h]
    cd = codec(code)
    N, B = cd.code.nvar, batch_size(bk, T)
    u = uniforms(seed, stream, f0, B, N)
    cells = cell_table(table, u, cd.nq_cha, T, f0)
    rng = np.random.default_rng(B * 1000 + N)
    cw01 = rng.integers(0, 2, (B, N), dtype=np.uint8)
    cw_bytes = rng.integers(0, 256, (B, N), dtype=np.uint8)
    for a in (u, cw01, cw_bytes):
        a.setflags(write=False)
    return cells, u, N, B, T, cw01, cw_bytes


# ---------------------------------------------------------------------------------------------------------------- error counters
# (handle, K_info values, SNR in dB of the code's own cell table): the counters over "codewords" of random bytes
STATS_CASES = [
    ("q4", (0, 1, 63, 64, 65, 255, 256, 257, 999, 1000)),
    ("q4_pack1", (0, 1, 63, 64, 65, 255, 256, 257, 999, 1000)),
    ("n127", (0, 1, 126, 127)),
]
STATS_B = ("T+1", "2T+3")
STATS_SNR = 4.0
STATS_SEED, STATS_STREAM, STATS_F0 = 2 ** 40 + 5, 7, 2 ** 32 - 7


@functools.lru_cache(maxsize=None)
def stats_reference(handle, bk, oracle_frames=24):
    """The reference of one (handle, batch) of the counters case: labels and uncoded errors from sample(), the oracle's decode of
    them (all frames, or oracle_frames evenly spaced ones)."""
    code, _, T = HANDLES[handle]
    cd = codec(code)
    cd.set_initial_message_mode(0)
    cd.set_exit_conditions(cd.max_iters, True, True)
    N, B = cd.code.nvar, batch_size(bk, T)
    cells = cd.channel_cells(STATS_SNR, cd.rate)
    cw = np.random.default_rng(B + N).integers(0, 256, (B, N), dtype=np.uint8)
    cw[::3] &= 0xFE                                  # every third frame sends the all-zero codeword (in bit 0: the other bits stay random)
    cha, msg, unc = sample(cells, STATS_SEED, STATS_STREAM, STATS_F0, B, N, cw)
    pick = np.arange(B) if oracle_frames is None else np.unique(np.linspace(0, B - 1, oracle_frames).astype(int))
    bits, iters = cd.lut_decode_batch(cha[pick], msg[pick])
    return dict(cells=cells, cw=cw, cha=cha, msg=msg, unc=unc, pick=pick, bits=bits, iters=iters, N=N, B=B, cd=cd)



# ---------------------------------------------------------------------------------------------------------------- generators
# (handle, K, R); (8193, 1807) is refused with ERR_UNSUPPORTED
GENERATOR_CASES = [(h, K, 1000 - K) for h in ("q4", "q4_pack1") for K in (1, 31, 32, 33, 127, 128, 129, 500, 968, 999, 1000)] + \
                  [("n10000", 8192, 1808), ("n127", 64, 63), ("n127_pack1", 64, 63)]
GENERATOR_REFUSED = ("n10000", 8193, 1807)
GEN_B = ("1", "63", "65", "T+1")
GEN_SEED, GEN_STREAM, GEN_F0 = 2 ** 40 + 5, 2 ** 31 - 1, 2 ** 32 - 7


def generator_rows(K, R):
    """R random dense rows of ceil(K/64) words; the words are random in all 64 bits, so bits at positions >= K are set too."""
    rng = np.random.default_rng(K * 10007 + R)
    return rng.integers(0, 1 << 64, (max(R, 1), (K + 63) // 64), dtype=np.uint64)[:R]


def gen_batch(kind, T):
    return T + 1 if kind == "T+1" else int(kind)


@functools.lru_cache(maxsize=None)
def generator_reference(K, R, B):
    """The codewords [B, K + R] uint8 of frames GEN_F0 .. of a generator case (a smaller batch is a prefix: frames are addressable)."""
    cw = encode(generator_bits(generator_rows(K, R), K), info_bits(GEN_SEED, GEN_STREAM, GEN_F0, B, K)).astype(np.uint8)
    cw.setflags(write=False)
    return cw
