"""The cases of the streaming pass kernels' degree sweep, shared by tests/test_08_streaming_degrees_gpu.py (decodes them on the GPU
against the oracle) and tests/test_streaming_cases_cpu.py (computes their coverage from describe() on host-only handles and checks
with the oracle alone that their batches tell decoders apart).  The code under pass_fused_kernel, cn_minsum_fast_kernel and
vn_balanced_fast_kernel is decided by the degree at compile time (kernels_fast.hpp: the all-but-one / two-minima forms, the software
pipeline up to degree 16, the unroll factors, one balanced tree per leaf count, all of it again chained and per bucket): the codes
here hold every variable degree 1..20 and every check degree 2..32, in classes whose sizes leave the last wave and the last block of
a role ragged, and every code runs through every launch path that holds its degrees."""
from __future__ import annotations

import functools

import numpy as np

from helpers import designed_codec, oracle_cache, planted_labels, product_decoder, write_degree_alist, write_zigzag_runs_alist      # noqa: F401
from resident_cases import EXIT_MODES      # noqa: F401  (the three exit modes every case decodes in)

# kernels_fast.hpp: the degree buckets of the fused kernel, leanest first
FUSED_VN_DEG, FUSED_CN_DEG, BUCKET_ORDER, MAX_ROLES = (8, 12, 20, 8), (8, 16, 32, 10), (0, 3, 1, 2), 10
VN_DEGREES, CN_DEGREES = range(1, 21), range(2, 33)
ITERS, GRAPH_SEED = 5, 11
STREAMING = {"LUTLDPC_RESIDENT": "0"}      # every case: these code sizes would otherwise decode out of LDS

# ---- section A: degree-sweep codes (configuration model).  Degree-3 variables carry the code, the other classes are guests of
#      12 to 60 nodes; no class size is a multiple of 4 or of its nodes per wave (test_streaming_cases_cpu.py asserts it).
#      name -> (variable degree: nodes, check degree: nodes, Nq_Cha, Nq_Msg, design sigma, SNR offset to the design SNR in dB, allow_deg1)
SWEEP = {
    "s1": ({1: 13, 2: 27, 3: 606, 4: 18, 5: 14}, {2: 23, 3: 17, 4: 13, 5: 18, 6: 298}, 16, 16, 0.80, 0.5, True),
    "s2": ({3: 602, 6: 15, 7: 13, 8: 17}, {6: 17, 7: 27, 8: 229}, 16, 16, 0.70, 0.5, False),
    "s3": ({2: 27, 3: 602, 8: 15}, {8: 21, 9: 18, 10: 165}, 16, 16, 0.62, 0.5, False),
    "s4": ({3: 701, 9: 13, 10: 14, 11: 15, 12: 17}, {11: 58, 12: 59, 13: 31, 14: 70}, 16, 16, 0.55, -0.5, False),
    "s5": ({3: 601, 4: 30}, {15: 61, 16: 63}, 16, 16, 0.48, -1.0, False),
    "s6": ({3: 713, 13: 13, 14: 14, 15: 15, 16: 13}, {17: 37, 18: 39, 19: 35, 20: 25, 21: 21}, 16, 16, 0.48, -1.0, False),
    "s7": ({3: 701, 17: 13, 18: 14, 19: 13, 20: 15}, {22: 29, 23: 30, 24: 31, 25: 15, 26: 26}, 16, 16, 0.45, -1.0, False),
    "s8": ({3: 994, 4: 30}, {27: 19, 28: 21, 29: 18, 30: 22, 31: 13, 32: 13}, 16, 8, 0.38, -1.5, False),
}
#      s2 at 32 labels.  Byte rows on every path, and look-up tables of 1024 entries are beyond the balanced-tree kernels and the fused
#      pipeline: the variable side runs the generated kernel, the check side the per-class cn_minsum_fast_kernel on 16 magnitudes
WIDE_LABELS = "s2_q5"
SWEEP[WIDE_LABELS] = SWEEP["s2"][:2] + (32, 32) + SWEEP["s2"][4:]
# ---- section B: zigzag-run codes.  The parity zigzag passes through contiguous runs of checks of every degree, so every check class
#      is chain-rich (build_fast_index: at least four checks per wave) and runs the chained bodies.  Run lengths are multiples of
#      neither 4 nor the checks per wave.
#      name -> ([(checks, information sockets per check = degree - 2), ...], information degree, Nq_Cha, Nq_Msg, sigma, offset)
ZIGZAG = {
    "z0a": ([(90, 1), (85, 2), (61, 4), (63, 5)], 3, 16, 16, 0.80, 0.5),
    "z0b": ([(149, 3), (101, 6)], 3, 16, 16, 0.75, 0.5),
    "z3": ([(90, 7), (81, 8)], 3, 16, 16, 0.60, 0.5),
    "z1": ([(18, 9), (22, 10), (23, 11), (21, 12), (22, 13), (27, 14)], 3, 16, 16, 0.50, -0.5),
    "z2a": ([(15, 15), (13, 16), (14, 17), (15, 18), (13, 19), (14, 20), (15, 21), (14, 22)], 3, 16, 16, 0.42, -1.0),
    "z2b": ([(13, 23), (14, 24), (13, 25), (14, 26), (15, 27), (13, 28), (14, 29), (15, 30)], 3, 16, 8, 0.36, -1.5),
}
CODES = list(SWEEP) + list(ZIGZAG)

# ---- section C: the paths every code runs through.  B = 600: two frame groups in nibble rows (512 + a ragged 88: halves of one
#      group each), three in byte rows (halves of 2 + 1); 203: one partly filled group (the fused launches with an empty second half)
B, B_SMALL, LABEL_SEED = 600, 203, 5
#      (path id, knobs, frames).  The wider buckets are added per code (paths()).
PATHS = [
    ("natural", {}, B),
    ("pack1", {"LUTLDPC_PACK": "1"}, B),
    ("skew0", {"LUTLDPC_SKEW": "0"}, B),                        # per-class kernels, several groups
    ("skew0_pack1", {"LUTLDPC_SKEW": "0", "LUTLDPC_PACK": "1"}, B),
    ("one_group", {}, B_SMALL),
    ("ffn0", {"LUTLDPC_FIRST_FROM_NODES": "0"}, B),
]
CHAIN0 = ("chain0", {"LUTLDPC_CHAIN": "0"}, B)                  # section B only

# ---- section D: knob cases on one bucket-0 sweep code and one zigzag code: (id, knobs, fields of describe() -> value)
KNOB_CODES = ("s2", "z0a")
KNOBS = [
    ("npw1", {"LUTLDPC_NODES_PER_WAVE": "1"}, {"nodes_per_wave": 1, "nodes_per_wave_cn": 1}),
    ("npw5", {"LUTLDPC_NODES_PER_WAVE": "5"}, {"nodes_per_wave": 5, "nodes_per_wave_cn": 5}),
    ("npw4096", {"LUTLDPC_NODES_PER_WAVE": "4096"}, {"nodes_per_wave": 4096, "nodes_per_wave_cn": 4096}),     # one wave per class
    ("npw_cn1", {"LUTLDPC_NODES_PER_WAVE_CN": "1"}, {"nodes_per_wave": 0, "nodes_per_wave_cn": 1}),
    ("npw_cn3", {"LUTLDPC_NODES_PER_WAVE_CN": "3"}, {"nodes_per_wave": 0, "nodes_per_wave_cn": 3}),
    ("vn_epw1", {"LUTLDPC_VN_EDGES_PER_WAVE": "1"}, {"vn_edges_per_wave": 1}),
    ("cn_epw65536", {"LUTLDPC_CN_EDGES_PER_WAVE": "65536"}, {"cn_edges_per_wave": 65536}),
    ("tail0", {"LUTLDPC_TAIL_FRONT": "0"}, {"tail_front": 0}),
    ("tail0.89", {"LUTLDPC_TAIL_FRONT": "0.89"}, {"tail_front": 0.89}),
    ("prio1", {"LUTLDPC_PRIO": "1"}, {"fused_prio": 1}),
    ("generic_npb1", {"LUTLDPC_USE_FAST": "0", "LUTLDPC_NODES_PER_BLOCK": "1"}, {"use_fast": 0, "nodes_per_block": 1}),
    ("generic_npb7", {"LUTLDPC_USE_FAST": "0", "LUTLDPC_NODES_PER_BLOCK": "7"}, {"use_fast": 0, "nodes_per_block": 7}),
    ("generic_npb4096", {"LUTLDPC_USE_FAST": "0", "LUTLDPC_NODES_PER_BLOCK": "4096"}, {"use_fast": 0, "nodes_per_block": 4096}),
]
# compaction with the margin at its default (a permutation must pay): check points after the exit tests of iterations 1 and 2.  Four
# frame groups, halves of two; COMPACT_QUIET of the frames are noise-free and have left by the first check point, so the live groups
# of a half drop from 2 to 1 there: compact_decide_kernel sees a gain of 1 group x 3 iterations against a cost of 1.3 x 2 and
# permutes with LUTLDPC_COMPACT_MIN_SHARE=0 (also at its default); with 1 (every live group must fall idle at once) it never does
B_COMPACT, COMPACT_QUIET = 3 * 512 + 77, 0.6
COMPACT = {"LUTLDPC_COMPACT": "1", "LUTLDPC_COMPACT_FIRST": "1", "LUTLDPC_COMPACT_EVERY": "1"}
COMPACT_KNOBS = [("compact_share0", dict(COMPACT, LUTLDPC_COMPACT_MIN_SHARE="0")), ("compact_share1", dict(COMPACT, LUTLDPC_COMPACT_MIN_SHARE="1"))]
# generated check kernels on (sign, magnitude) tables: (configuration of helpers.CONFIGS, frames, SNR in dB)
CHK_FULL0 = [("reg36_n1000_q3_chklut", 251, 2.5), ("c5_chklut", 205, 4.0)]

# ---- section E: more degree classes on one side than one launch of the interpreter once held (32): check degrees 2..34, three
#      checks each, under 594 degree-3 variables.  Degrees 33 and 34 are beyond cn_minsum_fast_kernel, so a default check pass runs
#      31 classes on it and two on cn_minsum_generic_kernel; the code has no case in the fused kernel and does not fit the LDS.
MANY_VDEG, MANY_CDEG, MANY_SIGMA, MANY_B, MANY_LABEL_SEED = {3: 594}, {d: 3 for d in range(2, 35)}, 0.45, 600, 4
#      the oracle's iteration codes on the batch with both exit tests on (test_streaming_cases_cpu.py): code -> frames
MANY_CODES = {-5: 32, 0: 2, 1: 20, 2: 166, 3: 180, 4: 114, 5: 86}


def codec(name):
    """The oracle-designed code of a case, its graph written once per session."""
    if name in SWEEP:
        vdeg, cdeg, nqc, nqm, sig, _, deg1 = SWEEP[name]
        return designed_codec("streaming-" + name, lambda path: write_degree_alist(path, vdeg, cdeg, seed=GRAPH_SEED),
                              sigma=sig, max_iters=ITERS, nq_msg=nqm, nq_cha=nqc, allow_deg1=deg1)
    runs, dv_info, nqc, nqm, sig, _ = ZIGZAG[name]
    return designed_codec("streaming-" + name, lambda path: write_zigzag_runs_alist(path, runs, dv_info, seed=GRAPH_SEED),
                          sigma=sig, max_iters=ITERS, nq_msg=nqm, nq_cha=nqc, allow_deg1=False)


def many_codec():
    """Section E: the code of 33 check classes, designed with the oracle."""
    return designed_codec("streaming-many", lambda path: write_degree_alist(path, MANY_VDEG, MANY_CDEG, seed=GRAPH_SEED),
                          sigma=MANY_SIGMA, max_iters=ITERS, nq_msg=16)


@functools.lru_cache(maxsize=None)
def many_labels():
    """Section E: MANY_B frames at the design SNR (4.717 dB), frame 0 noise-free.  Shared read-only."""
    cd = many_codec()
    return planted_labels(cd, MANY_B, -10 * np.log10(2 * cd.rate * MANY_SIGMA ** 2), MANY_LABEL_SEED, noise_free=[0])


def snr(name):
    cd, (sig, off) = codec(name), (SWEEP[name][4:6] if name in SWEEP else ZIGZAG[name][4:6])
    return -10 * np.log10(2 * cd.rate * sig * sig) + off


@functools.lru_cache(maxsize=None)
def labels(name, n=B, quiet=0.0):
    """Channel and initial-message labels of the first n frames of the code's batch, three noise-free frames planted (first, middle,
    last: they pass the test on the channel decisions); quiet: that share of the frames noise-free as well.  Shared read-only."""
    free = [0, n // 2, n - 1] + np.flatnonzero(np.random.default_rng(LABEL_SEED).random(n) < quiet).tolist()
    return planted_labels(codec(name), n, snr(name), LABEL_SEED, noise_free=free)


def degrees(name):
    """(variable degrees, check degrees) of a code, from its table entry."""
    if name in SWEEP:
        return sorted(SWEEP[name][0]), sorted(SWEEP[name][1])
    return [2, ZIGZAG[name][1]], sorted(s + 2 for _, s in ZIGZAG[name][0])


def natural_bucket(name):
    dv, dc = degrees(name)
    return next(b for b in BUCKET_ORDER if dv[-1] <= FUSED_VN_DEG[b] and dc[-1] <= FUSED_CN_DEG[b])


def paths(name):
    """The paths of section C for one code: PATHS, every wider bucket in nibble and in byte rows (the labels stay: the oracle result
    is shared), LUTLDPC_CHAIN=0 for the zigzag codes."""
    if name == WIDE_LABELS:
        return [p for p in PATHS if p[0] in ("natural", "one_group")]
    out = list(PATHS)
    wider = BUCKET_ORDER[BUCKET_ORDER.index(natural_bucket(name)) + 1:]
    for b in wider:
        out.append((f"bucket{b}", {"LUTLDPC_FUSED_BUCKET_MIN": str(b)}, B))
        out.append((f"bucket{b}_pack1", {"LUTLDPC_FUSED_BUCKET_MIN": str(b), "LUTLDPC_PACK": "1"}, B))
    if name in ZIGZAG:
        out.append(CHAIN0)
    return out


def expected(name, kn):
    """What describe() must report for a code created with the knobs kn: the path the case names."""
    b = natural_bucket(name)
    if "LUTLDPC_FUSED_BUCKET_MIN" in kn:
        b = int(kn["LUTLDPC_FUSED_BUCKET_MIN"])
    fast, wide = kn.get("LUTLDPC_USE_FAST", "1") == "1", name == WIDE_LABELS
    return {"resident": 0, "fused_bucket": b, "use_fast": int(fast), "skewed_pipeline": int(fast and not wide and kn.get("LUTLDPC_SKEW", "1") == "1"),
            "pack": 1 if (wide or "LUTLDPC_PACK" in kn) else 2}


# every case of sections A to C: (id, code, knobs, frames)
CASES = [(f"{name}-{pid}", name, dict(STREAMING, **kn), n) for name in CODES for pid, kn, n in paths(name)]
# section D: (id, code, knobs, frames, share of noise-free frames, fields of describe() -> value)
KNOB_CASES = [(f"{name}-{kid}", name, dict(STREAMING, **kn), B, 0.0, want) for name in KNOB_CODES for kid, kn, want in KNOBS] + \
             [(f"{name}-{kid}", name, dict(STREAMING, **kn), B_COMPACT, COMPACT_QUIET, {"compaction": 1}) for name in KNOB_CODES for kid, kn in COMPACT_KNOBS]


def describe(name, kn, monkeypatch, device=-1, cd=None):
    """(decoder, describe()) of a code created with the knobs kn (read once, at creation) and no other LUTLDPC_ variable."""
    import os
    for k in [k for k in os.environ if k.startswith("LUTLDPC_") and k not in ("LUTLDPC_LIB", "LUTLDPC_DESIGN_CACHE")]:
        monkeypatch.delenv(k)
    for k, v in kn.items():
        monkeypatch.setenv(k, v)
    dec = product_decoder(cd or codec(name), device=device)
    return dec, dec.describe()


def check_path(name, kn, desc):
    """The case is on the path it names: bucket, pipeline, rows, and the kernel of every class."""
    want = expected(name, kn)
    assert {k: desc[k] for k in want} == want, (name, kn, {k: desc[k] for k in want}, want)
    vn, cn = {c["kernel"] for c in desc["vn_classes"]}, {c["kernel"] for c in desc["cn_classes"]}
    if name == WIDE_LABELS:
        assert vn <= {"lutldpc_jit_pass", "tree_pass_kernel<VAR>"} and cn == {"cn_minsum_fast_kernel"}, desc      # (a host-only handle generates no kernel)
    elif want["use_fast"]:
        assert vn == {"vn_balanced_fast_kernel"} and cn == {"cn_minsum_fast_kernel"}, desc
    else:
        assert vn == {"tree_pass_kernel<VAR>"} and cn == {"cn_minsum_generic_kernel"}, desc
    assert [c["deg"] for c in desc["vn_classes"]] == degrees(name)[0] and [c["deg"] for c in desc["cn_classes"]] == degrees(name)[1], desc


def bodies(desc):
    """The (kind, degree, bucket, pack) bodies of the specialised pass kernels a decoder with this description runs: the fused
    kernel's under the skewed pipeline, the per-class kernels' (bucket None) without it.  The tally of what the suite reaches."""
    if not desc["use_fast"] or desc["resident"]:
        return set()
    b = desc["fused_bucket"] if desc["skewed_pipeline"] else None
    out = {("VAR", c["deg"], b, desc["pack"]) for c in desc["vn_classes"] if c["kernel"] == "vn_balanced_fast_kernel"}
    out |= {("DEC", c["deg"], None, desc["pack"]) for c in desc["vn_classes"] if c["kernel"] == "vn_balanced_fast_kernel"}      # always per class
    for c in desc["cn_classes"]:
        if c["kernel"] == "cn_minsum_fast_kernel":
            out.add(("CHK", c["deg"], b, desc["pack"]))
            if c["chain_nodes"] and desc["skewed_pipeline"]:
                out.add(("CHK_CHAIN", c["deg"], b, desc["pack"]))
    return out
