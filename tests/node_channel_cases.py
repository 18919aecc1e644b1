"""Cases and reference of the sampler's per-node channel classes (lutldpc_decoder_set_node_channels), shared by
tests/test_node_channels_cpu.py (holds the cases to their conditions with the reference and the oracle alone) and
tests/test_33_node_channels_gpu.py (holds the kernel and the layers above it to the reference).  The reference is the one-table
reference of tests/frontend_cases.py applied column by column: for each class c, frontend_cases.sample(table_c, ...) on the
shared uniforms, of which the columns with node_class == c are taken.  Everything is integer: equal bit for bit, no tolerance."""
from __future__ import annotations

import functools

import numpy as np

import frontend_cases as fc

# handle -> (code, environment at creation, frames per group T): the two odd-N codes of frontend_cases in both row formats
HANDLES = {h: fc.HANDLES[h] for h in ("n127", "n127_pack1", "n33")}
HANDLES["n33_pack1"] = ("n33", {"LUTLDPC_PACK": "1"}, 256)
MAX_CLASSES = 16
WAVE_NODES = 16                                    # a wave of the sampler runs 8 pairs = 16 nodes


# ---------------------------------------------------------------------------------------------------------------- layouts
def node_classes(layout, N):
    """The class of every node.  one: one class; evenodd: every Philox pair splits over two tables; mod16: 16 classes v % 16;
    blocks: contiguous blocks with a boundary inside the first wave's run of 8 pairs (and inside a pair), one in the middle of the
    code, and the last class on node N - 1 alone; empty: class 1 of three has no node."""
    v = np.arange(N)
    if layout == "one":
        return np.zeros(N, np.uint8)
    if layout == "evenodd":
        return (v % 2).astype(np.uint8)
    if layout == "mod16":
        return (v % 16).astype(np.uint8)
    if layout == "blocks":
        cuts = [5, N // 2 + 4, N - 1]
        assert 0 < cuts[0] < WAVE_NODES and cuts[0] % 2 == 1 and cuts[0] < cuts[1] < cuts[2]
        return np.searchsorted(cuts, v, side="right").astype(np.uint8)
    if layout == "empty":
        return np.where(v % 2, 2, 0).astype(np.uint8)
    raise KeyError(layout)


# the tables of a layout's classes, by the names of frontend_cases.cell_table; "t35": 35 cells between quantiles of the uniforms;
# "big": the 72 cells inside one bucket where the batch has the samples for it, else the 72 cells of the pins
LAYOUT_TABLES = {
    "one": ["dense_q4"],
    "evenodd": ["pins", "boundaries"],
    "mod16": ["trivial1", "trivial2", "t35", "pins", "boundaries", "dense_q4", "big", "trivial2", "pins", "t35", "boundaries", "trivial1", "dense_q4", "big",
              "pins", "t35"],
    "blocks": ["dense_q4", "pins", "boundaries", "trivial2"],
    "empty": ["pins", "trivial2", "boundaries"],
}
ONE_BUCKET_MIN_SAMPLES = 100000                    # (frontend_cases runs one_bucket from 130429 samples up)


def table(name, u, nq, T, frame0):
    if name == "t35":
        srt = np.unique(u)
        return fc.labelled(srt[len(srt) // 35::len(srt) // 35][:34], nq)
    if name == "big":
        name = "one_bucket" if u.size >= ONE_BUCKET_MIN_SAMPLES else "pins"
    if name == "pins" and u.size < 35:
        name = "trivial2"
    return fc.cell_table(name, u, nq, T, frame0)


# (handle, layout, batch size, frame0, seed, stream): every layout on both codes, in both row formats, at every kind of batch, with
# frame ranges that carry into the high index word (F_CARRY) or wrap at 2^64 (F_WRAP, from 12 frames up)
CASES = [
    ("n127", "one", "T+1", fc.F_CARRY, 3, 0),
    ("n127", "evenodd", "2T+3", fc.F_WRAP, fc.SEED_BIG, 7),
    ("n127", "mod16", "2T+3", 0, 3, fc.STREAM_MAX),
    ("n127", "blocks", "T-1", fc.F_HIGH, fc.SEED_BIG, 0),
    ("n127", "empty", "1", fc.F_WRAP, 3, 7),
    ("n127_pack1", "mod16", "T+1", fc.F_CARRY, fc.SEED_BIG, 7),
    ("n127_pack1", "blocks", "2T+3", fc.F_WRAP, 3, 0),
    ("n127_pack1", "evenodd", "T", 0, 3, fc.STREAM_MAX),
    ("n33", "one", "1", fc.F_HIGH, 3, 7),
    ("n33", "mod16", "2T+3", fc.F_WRAP, fc.SEED_BIG, 0),
    ("n33", "blocks", "T+1", fc.F_CARRY, 3, fc.STREAM_MAX),
    ("n33", "empty", "T", 0, fc.SEED_BIG, 7),
    ("n33_pack1", "evenodd", "T+1", fc.F_CARRY, 3, 0),
    ("n33_pack1", "mod16", "2T+3", fc.F_WRAP, fc.SEED_BIG, 7),
]
LAYOUTS = list(LAYOUT_TABLES)


def case_id(case):
    h, layout, b, f0, seed, stream = case
    return f"{h}-{layout}-B{b}-f{'0' if f0 == 0 else 'carry' if f0 == fc.F_CARRY else 'high' if f0 == fc.F_HIGH else 'wrap'}-s{seed % 97}-st{stream % 97}"


# the generator of the device codewords of a code: (K, R), rows of frontend_cases.generator_rows
GENERATORS = {"n127": (64, 63), "n33": (17, 16)}


@functools.lru_cache(maxsize=None)
def sampler_case(case):
    """dict of a case: tables (one per class), node_class, the reference's uniforms u, N, B, T, and the three kinds of sent bits --
    none, host codewords of random bytes (bit 0 counts), the codewords of the device encoder (K, R, generator rows, reference
    codewords).  Shared read-only."""
    h, layout, bk, f0, seed, stream = case
    code, _, T = HANDLES[h]
    cd = fc.codec(code)
    N, B = cd.code.nvar, fc.batch_size(bk, T)
    u = fc.uniforms(seed, stream, f0, B, N)
    tables = [table(name, u, cd.nq_cha, T, f0) for name in LAYOUT_TABLES[layout]]
    cls = node_classes(layout, N)
    assert len(tables) <= MAX_CLASSES and cls.max() < len(tables)
    cw_bytes = np.random.default_rng(B * 1000 + N).integers(0, 256, (B, N), dtype=np.uint8)
    K, R = GENERATORS[code]
    cw_dev = fc.encode(fc.generator_bits(fc.generator_rows(K, R), K), fc.info_bits(seed, stream, f0, B, K)).astype(np.uint8)
    for a in (u, cls, cw_bytes, cw_dev):
        a.setflags(write=False)
    return dict(tables=tables, node_class=cls, u=u, N=N, B=B, T=T, seed=seed, stream=stream, f0=f0, cw_bytes=cw_bytes, K=K, R=R, cw_dev=cw_dev)


def sample(tables, node_class, seed, stream, frame0, B, N, codewords=None, u=None):
    """(cha, msg, uncoded errors) of the sampler with a table per node: frontend_cases.sample of every class's table on the shared
    uniforms, the columns of the class taken; the uncoded errors are the cells on the negative side over every node's own table."""
    u = fc.uniforms(seed, stream, frame0, B, N) if u is None else u
    node_class = np.asarray(node_class)
    cha, msg, unc = np.zeros((B, N), np.uint8), np.zeros((B, N), np.uint8), np.zeros(B, np.int64)
    for c, t in enumerate(tables):
        cols = node_class == c
        if not cols.any():
            continue
        a, m, _ = fc.sample(t, seed, stream, frame0, B, N, codewords, u=u)
        cha[:, cols], msg[:, cols] = a[:, cols], m[:, cols]
        unc += t["neg"][fc.cells_of(t, u[:, cols])].astype(np.int64).sum(1)
    return cha, msg, unc.astype(np.int32)


def reference(case, sent):
    """The reference labels of a case for sent in ("none", "bytes", "device"): (cha, msg, uncoded errors, codewords or None)."""
    c = sampler_case(case)
    cw = {"none": None, "bytes": c["cw_bytes"], "device": c["cw_dev"]}[sent]
    return sample(c["tables"], c["node_class"], c["seed"], c["stream"], c["f0"], c["B"], c["N"], cw, u=c["u"]) + (cw,)


# ---------------------------------------------------------------------------------------------------------------- limit tables
def erasure_table(qb_cha, qb_msg=None, cha2msg=None):
    """The table of a punctured node, as include/lut_ldpc_host.h states it: two cells, thr = {2^63}; cell 0 is x = 0- (cha = number of
    channel boundaries < 0, neg = 1), cell 1 is x = 0+ (boundaries <= 0, neg = 0); msg the same count over qb_msg, or cha2msg[cha];
    mirrors: alphabet size - 1 - label, or cha2msg of the mirrored channel label."""
    qc = np.asarray(qb_cha, np.float64)
    cha = np.array([(qc < 0).sum(), (qc <= 0).sum()])
    return _limit(np.array([1 << 63], np.uint64), cha, [1, 0], len(qc) + 1, qb_msg, cha2msg, lambda q: np.array([(q < 0).sum(), (q <= 0).sum()]))


def known_table(qb_cha, qb_msg=None, cha2msg=None):
    """The table of a known bit: one cell, the top labels, neg = 0; mirrors label 0 (or cha2msg[0]).  (thr: non-null, its content unused.)"""
    n = len(qb_cha) + 1
    return _limit(np.array([0xDEADBEEFDEADBEEF], np.uint64), np.array([n - 1]), [0], n, qb_msg, cha2msg, lambda q: np.array([len(q)]))


def _limit(thr, cha, neg, nq_cha, qb_msg, cha2msg, count):
    if cha2msg is not None:
        mp = np.asarray(cha2msg)
        msg, msg_m = mp[cha], mp[nq_cha - 1 - cha]
    else:
        q = np.asarray(qb_msg, np.float64)
        msg = count(q)
        msg_m = len(q) - msg
    return {"thr": thr, "cha": cha.astype(np.uint8), "msg": msg.astype(np.uint8), "neg": np.array(neg, np.uint8),
            "cha_m": (nq_cha - 1 - cha).astype(np.uint8), "msg_m": msg_m.astype(np.uint8)}


def same_table(a, b):
    n = len(a["cha"])
    return len(b["cha"]) == n and all((np.asarray(a[k])[:n] == np.asarray(b[k])[:n]).all() for k in ("cha", "msg", "neg", "cha_m", "msg_m")) and \
        (np.asarray(a["thr"], np.uint64)[:n - 1] == np.asarray(b["thr"], np.uint64)[:n - 1]).all()


# ---------------------------------------------------------------------------------------------------------------- decode cases
# (handle, batch size, SNR in dB of classes 0 and 3; class 1 is punctured, class 2 known): sampler + decode + counters, histograms,
# capture.  Classes by blocks of nodes; the SNRs are chosen so that each batch holds frames that converge and frames that do not
# (tests/test_node_channels_cpu.py asserts it on the oracle's frames).
STATS_CASES = [("n127", "T+1", 5.0, 2.0), ("n127_pack1", "2T+3", 5.0, 2.0), ("n33", "T+1", 5.0, 2.0)]
STATS_SEED, STATS_STREAM, STATS_F0 = 2 ** 40 + 5, 7, 2 ** 32 - 7
STATS_GENERATOR_K = 2                              # device codewords: a quarter of the frames sends the all-zero codeword, which the code holds


def stats_classes(N):
    """Four blocks: most nodes at the first SNR, a sixth punctured, a sixth known, the rest at the second SNR."""
    v = np.arange(N)
    return np.select([v < N // 2, v < N // 2 + N // 6, v < N // 2 + 2 * (N // 6)], [0, 1, 2], 3).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def stats_reference(handle, bk, snr_a, snr_b, sent="bytes", oracle_frames=24):
    """The reference of one decode case: tables, node_class, sent bytes, reference labels and uncoded errors, and the oracle's decode
    of oracle_frames evenly spaced frames.  sent: "bytes" (random bytes, every third frame even bytes: the all-zero codeword) or
    "device" (the codewords of a generator of STATS_GENERATOR_K information bits and random rows)."""
    code, _, T = HANDLES[handle]
    cd = fc.codec(code)
    cd.set_initial_message_mode(0)
    cd.set_exit_conditions(cd.max_iters, True, True)
    N, B = cd.code.nvar, fc.batch_size(bk, T)
    tables = [cd.channel_cells(snr_a, cd.rate), erasure_table(cd.qb_cha, cd.qb_msg), known_table(cd.qb_cha, cd.qb_msg), cd.channel_cells(snr_b, cd.rate)]
    tables = [{k: np.ascontiguousarray(v) for k, v in t.items()} for t in tables]
    cls = stats_classes(N)
    if sent == "bytes":
        cw = np.random.default_rng(B + N).integers(0, 256, (B, N), dtype=np.uint8)
        cw[::3] &= 0xFE
    else:
        K = STATS_GENERATOR_K
        cw = fc.encode(fc.generator_bits(fc.generator_rows(K, N - K), K), fc.info_bits(STATS_SEED, STATS_STREAM, STATS_F0, B, K)).astype(np.uint8)
    cha, msg, unc = sample(tables, cls, STATS_SEED, STATS_STREAM, STATS_F0, B, N, cw)
    pick = np.unique(np.linspace(0, B - 1, oracle_frames).astype(int))
    bits, iters = cd.lut_decode_batch(cha[pick], msg[pick])
    return dict(tables=tables, node_class=cls, cw=cw, cha=cha, msg=msg, unc=unc, pick=pick, bits=bits, iters=iters, N=N, B=B, K=N // 2, cd=cd)


# ---------------------------------------------------------------------------------------------------------------- ber_sim
BER_ALIST = "rate0.50_dv02-17_dc08-09_lut_q4_N500"
BER_OFFSETS = ["0", "-inf", "inf", "-3.0"]
BER_INI = """[Sim]
   SNRdB    = 3.0 4.5
   Nframes  = 300
   Nfers    = 20
   ber_min  = 1e-9
   fer_min  = 1e-9
   batch_frames = 128
[LDPC]
   parity_filename = {alist}
   zero_codeword = true
   known_rank = 250
[LUT]
   max_iter = 8
   design_thr = 0.88
   qbits_channel = 4
   qbits_message_uniform = 4
{channel}"""
BER_CHANNEL = """[Channel]
   node_classes_filename = {file}
   class_snr_offset_dB = {offsets}
"""


def ber_classes(N=500):
    """The N = 500 code: the last 20 nodes punctured, the 50 before them known, every fifth of the rest 3 dB down (with these a point
    of the sweep below sees some forty to eighty frames before its 21st frame error: frames that fail and frames that do not)."""
    v = np.arange(N)
    return np.select([v >= N - 20, v >= N - 70, v % 5 == 4], [1, 2, 3], 0).astype(np.uint8)


def write_ber_case(tmp_path, channel=True, offsets=None, classes=None, name="ber_nc.ini", section="LUT"):
    """base directory with the code (and the class file) and the parameter file; returns (params path, base path)."""
    import shutil
    from helpers import CODES
    base = tmp_path / "base"
    (base / "codes").mkdir(parents=True, exist_ok=True)
    shutil.copy(CODES / f"{BER_ALIST}.alist", base / "codes")
    cls = ber_classes() if classes is None else classes
    (base / "codes" / "classes.txt").write_text("\n".join(" ".join(str(int(c)) for c in cls[i:i + 50]) for i in range(0, len(cls), 50)) + "\n")
    ch = BER_CHANNEL.format(file="classes.txt", offsets=" ".join(BER_OFFSETS if offsets is None else offsets)) if channel else ""
    txt = BER_INI.format(alist=BER_ALIST, channel=ch)
    if section == "BP":
        txt = txt.replace("[LUT]", "[BP]")
    params = tmp_path / name
    params.write_text(txt)
    return params, base
