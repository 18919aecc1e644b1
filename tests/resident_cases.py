"""The cases of the resident decoder's variant matrix and degree limits, shared by tests/test_07_resident_variants_gpu.py (decodes
them on the GPU against the oracle) and tests/test_resident_variants_cpu.py (generates and cross-compiles the same kernels on a
host-only handle).  The generator (jit_resident.hpp) branches on six knobs that resident_spec otherwise sets from tuned
thresholds; a case names the knobs it sets and expected_variant() says what the generated source must then be."""
from __future__ import annotations

import functools
import os

import numpy as np

from helpers import CONFIGS, designed_codec, oracle_cache, oracle_codec, planted_labels, product_decoder, resident_variant, write_random_alist      # noqa: F401

K = "LUTLDPC_RESIDENT_"
VARIANT_KNOBS = ("U", "FLAG_REDUCE", "CN_PERSISTENT", "XCD", "FM", "WAVES_EU")
LDS_BUDGET = 160 * 1024 - 2048
EXIT_MODES = [(True, True), (True, False), (False, False)]      # (psc, pisc)


def knobs(**kw):
    return {K + k: str(v) for k, v in kw.items()}


# ---- section 1: the smallest code of every structure -> (ragged batch, SNR in dB)
CODES = {
    "n500_q4_i8": (301, 1.9),                 # irregular, variable degrees 2/3/9/17, checks 8 and 9, nibble rows
    "reg36_n1000_q5": (203, 1.9),             # byte rows: four frames per dword
    "reg36_n1000_mixed": (297, 2.2),          # alphabets 16 -> 8 with reused stages: several code variants per class
    "reg36_n1000_q3_chklut": (251, 2.5),      # CHKTREE check update: cn_persistent has nothing to act on
    "c5_minlut": (205, 4.0),                  # check degree 32: the wide two-sweep min-sum
}
FLIPPED = "flipped"                           # every knob away from the code's automatic choice at once (flipped_knobs)
VARIANTS = [
    ("U1", knobs(U=1)), ("U2", knobs(U=2)), ("U4", knobs(U=4)),
    ("flag0", knobs(FLAG_REDUCE=0)), ("flag1", knobs(FLAG_REDUCE=1)),
    ("cnp0", knobs(CN_PERSISTENT=0)), ("cnp1", knobs(CN_PERSISTENT=1)),
    ("xcd0", knobs(XCD=0)), ("fm0", knobs(FM=0)), ("weu2", knobs(WAVES_EU=2)),
    (FLIPPED, None),
]
MATRIX = [(name, vid, kn) for name in CODES for vid, kn in VARIANTS]

# geometry interplay: (id, code, knobs, B, SNR, oracle's flat mode, workgroups a multiple of 8?)
GEOMETRY = [
    # waves that straddle two sets (class sizes are no multiples of 64): both branches of res_flag inside one launch
    ("straddle_nibble", "n500_q4_i8", knobs(FLAG_REDUCE=1, S=3, NT=256), 301, 1.9, False, False),
    ("straddle_byte", "reg36_n1000_q5", knobs(FLAG_REDUCE=1, S=3), 203, 1.9, False, False),
    # the XCD remap active on a ragged last workgroup: 256 sets / 11 -> 24 workgroups, the last one mostly beyond n_sets
    ("xcd1_ragged_grid", "reg36_n1000_q4", knobs(XCD=1, S=11, NT=512), 1797, 1.9, True, True),
    # the remap switched off by its own test: 64 sets / 3 -> 22 workgroups
    ("xcd1_grid_not_8", "n500_q4_i8", knobs(XCD=1, S=3, NT=512), 301, 1.9, False, False),
    # (XCD=0 on a grid that is a multiple of 8: the xcd0 column of the matrix, S = 1)
]

# ---- section 2: synthetic codes at the eligibility limits of resident_eligible and one step past them
#      N, M, variable degrees, shares, Nq_Cha, Nq_Msg, iterations, design sigma, SNR offset to the design SNR in dB, allow_deg1
LIMITS = {
    "dc17": (680, 120, [3], [1.0], 16, 16, 6, 0.45, 0.0, False),             # odd wide check
    "dc33": (1100, 100, [3], [1.0], 16, 8, 6, 0.36, -0.6, False),            # past kFastMaxCnDeg of the streaming kernels
    "dc64": (2040, 96, [3], [1.0], 16, 8, 5, 0.30, -0.8, False),             # check degrees 63 and 64: at the limit
    "dc65": (2080, 96, [3], [1.0], 16, 8, 5, 0.30, -0.4, False),             # one past it
    "dv24": (600, 300, [2, 3, 24], [0.5, 0.42, 0.08], 16, 16, 8, 0.85, 1.5, False),
    "dv25": (600, 300, [2, 3, 25], [0.5, 0.42, 0.08], 16, 16, 8, 0.85, 1.5, False),
    "deg1": (600, 300, [1, 2, 3, 6], [0.02, 0.38, 0.45, 0.15], 16, 16, 8, 0.80, 1.5, True),
    "cls12": (650, 325, list(range(2, 14)), [1 / 12] * 12, 16, 16, 8, 0.70, 1.0, False),      # 12 variable classes: the most
    "cls13": (650, 325, list(range(2, 15)), [1 / 13] * 13, 16, 16, 8, 0.70, 1.0, False),      # 13: streaming kernels
}
GRAPH_SEED, LABEL_SEED, LIMIT_B = 7, 1, 203
# (id, code, knobs, resident as describe() must report it)
LIMIT_CASES = [
    ("dc17", "dc17", {}, 1), ("dc17_cnp1", "dc17", knobs(CN_PERSISTENT=1), 1), ("dc17_streaming", "dc17", {"LUTLDPC_RESIDENT": "0"}, 0),
    ("dc33", "dc33", {}, 1), ("dc33_streaming", "dc33", {"LUTLDPC_RESIDENT": "0"}, 0),
    ("dc64", "dc64", {}, 1), ("dc64_streaming", "dc64", {"LUTLDPC_RESIDENT": "0"}, 0),
    ("dc65", "dc65", {}, 0),
    ("dv24", "dv24", {}, 1), ("dv25", "dv25", {}, 0),
    ("deg1", "deg1", {}, 1),
    ("cls12", "cls12", {}, 1), ("cls13", "cls13", {}, 0),
]


def codec(name):
    """oracle_codec for the named configurations, the oracle-designed synthetic code for the LIMITS."""
    if name in CONFIGS:
        return oracle_codec(name)
    N, M, dvc, dvp, nqc, nqm, I, sig, _, deg1 = LIMITS[name]
    return designed_codec("resident-" + name, lambda path: write_random_alist(path, N, M, dvc, np.asarray(dvp) / np.sum(dvp), seed=GRAPH_SEED),
                          sigma=sig, max_iters=I, nq_msg=nqm, nq_cha=nqc, allow_deg1=deg1)


def limit_snr(name):
    cd, sig, off = codec(name), LIMITS[name][7], LIMITS[name][8]
    return -10 * np.log10(2 * cd.rate * sig * sig) + off


@functools.lru_cache(maxsize=None)
def labels(name, B, snr, seed=None):
    """Channel and initial-message labels of a batch with three noise-free frames planted (first, middle, last: they pass the
    test on the channel decisions).  Computed once per batch, shared read-only."""
    return planted_labels(codec(name), B, snr, B if seed is None else seed, noise_free=(0, B // 2, B - 1), mode=1 if name.startswith("c5") else 0)


def frame_groups(dec, B):
    t = dec.describe()["tile_frames"]
    return (B + t - 1) // t


def workgroups(dec, B, S):
    return (64 * frame_groups(dec, B) + S - 1) // S


def _without_variant_knobs(env):
    return {k: v for k, v in env.items() if not (k.startswith(K) and k[len(K):] in VARIANT_KNOBS)}


def auto_variant(name, B, kn):
    """The variant resident_spec chooses by itself for this code at the geometry of the case (cn_persistent depends on it): read off
    the source of a host-only handle created with the case's geometry knobs alone.  Restores the environment."""
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith(K)}
    try:
        os.environ.update(_without_variant_knobs(kn))
        dec = product_decoder(codec(name), device=-1)
        src, _ = dec.resident_source(frame_groups(dec, B))
        dec.close()
    finally:
        for k in [k for k in os.environ if k.startswith(K)]:
            del os.environ[k]
        os.environ.update(saved)
    return resident_variant(src)


def flipped_knobs(auto):
    return knobs(U=4, FLAG_REDUCE=1 - auto["flag_reduce"], CN_PERSISTENT=1 - auto["cn_persistent"], XCD=0, FM=0, WAVES_EU=2)


def expected_variant(auto, kn, min_lut):
    """What resident_variant must report for a source generated with the knobs `kn` where `auto` is the automatic choice."""
    want = dict(auto)
    for field, knob in (("flag_reduce", "FLAG_REDUCE"), ("cn_persistent", "CN_PERSISTENT"), ("xcd", "XCD"), ("waves_eu", "WAVES_EU")):
        if K + knob in kn:
            want[field] = int(kn[K + knob])
    if not min_lut:
        want["cn_persistent"] = 0            # a CHKTREE check update has no min-sum items to keep addresses for
    if K + "U" in kn:
        want["U"] = {int(kn[K + "U"])}
    return want


def check_source(dec, name, B, kn, auto):
    """The source the decode of B frames compiles (resident_source and the decode go through resident_pick + resident_spec on the
    same options): its variant is the one the case names, its geometry the one the case forced.  Returns (src, S, NT, lds)."""
    src, (S, NT, lds) = dec.resident_source(frame_groups(dec, B))
    got, want = resident_variant(src), expected_variant(auto, kn, codec(name).min_lut)
    assert got == want, (name, kn, got, want)
    if K + "S" in kn:
        assert S == int(kn[K + "S"]), (S, kn)            # resident_pick lowers a forced S silently when LDS or the item cap says so
    if K + "NT" in kn:
        assert NT == int(kn[K + "NT"]), (NT, kn)
    assert lds <= LDS_BUDGET
    return src, S, NT, lds
