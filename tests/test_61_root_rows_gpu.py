"""The root step of the compile-time variable kernels on nibble rows: one 64-bit row read per frame (rows[ch]: 16 packed four-bit
labels), one 64-bit shift by 4 x the top inner node's label and one funnel shift per output (kernels_fast.hpp: vn_balanced_body;
lut_program.hpp: pack_root_rows).  Every case first asserts from describe() that the form is in force in every class of degree
>= 3 (root_rows; the byte-row case that it is NOT), then decodes bit-exact against the oracle, on every frame, in the three exit
modes: with the exit tests on, frozen frames and masked stores meet the funnel-shifted rows.  Shapes: variable degrees 3, 4, 8 (two
frames per trip), 9 and 20 (one per trip) in their own buckets of the fused kernel, in every wider bucket and in the per-class
kernels; alphabets (channel, message) = (16,16), (16,8), (8,16), (4,4), (2,2) and one schedule whose message alphabet changes
between iterations; 1 frame, 513 frames (a second group with one live frame) and 1030 frames.  Two frames of every batch of three
or more are planted: every label at its maximum -- ch = 15 with `top` saturated, bits 60 .. 63 of the last row -- and every label
0, nibble 0 of row 0."""
import functools

import numpy as np
import pytest

import streaming_cases as sc
from helpers import compare, designed_codec, oracle_cache, planted_labels, write_degree_alist

pytestmark = pytest.mark.gpu

# codes of this file: degrees 3, 4 and 8 under degree-6 checks (1998 edges, bucket 0), N = 635, designed per alphabet pair
VDEG, CDEG, ITERS = {3: 602, 4: 18, 8: 15}, {6: 333}, 6
#   name -> (Nq_Cha, Nq_Msg per iteration, design sigma, SNR offset in dB)
OWN = {
    "c8m16": (8, [16] * ITERS, 0.70, 0.5),
    "c4m4": (4, [4] * ITERS, 0.60, 0.5),
    "c2m2": (2, [2] * ITERS, 0.50, 3.5),                    # (one-bit messages: a frame passes on the channel decisions or never, so half of them do)
    "grow": (8, [4, 8, 8, 16, 16, 16], 0.70, 0.5),         # the message alphabet changes between iterations: rows of 4, 8 and 16 nibbles
}


def codec(name):
    if name in sc.CODES:
        return sc.codec(name)
    nqc, nqm, sig, _ = OWN[name]
    return designed_codec("root_rows-" + name, lambda path: write_degree_alist(path, VDEG, CDEG, seed=sc.GRAPH_SEED), sigma=sig, max_iters=ITERS,
                          nq_msg=nqm, nq_cha=nqc)


@functools.lru_cache(maxsize=None)
def labels(name, n):
    """n frames near the design SNR; of three or more, frame 0 carries the largest label everywhere and frame 1 label 0 everywhere."""
    cd = codec(name)
    snr = sc.snr(name) if name in sc.CODES else -10 * np.log10(2 * cd.rate * OWN[name][2] ** 2) + OWN[name][3]
    return planted_labels(cd, n, snr, 61, noise_free=[0] if n >= 3 else [], zero=[1] if n >= 3 else [])


SKEW0 = {"LUTLDPC_SKEW": "0"}


def bucket(b):
    return {"LUTLDPC_FUSED_BUCKET_MIN": str(b)}


# (code, knobs, frames).  s1: degrees 1 .. 5; s2: 3, 6, 7, 8; s3: 2, 3, 8 under checks up to degree 10 (bucket 3); s4: 3, 9 .. 12
# (bucket 1); s7: 3, 17 .. 20 (bucket 2); s8: 3, 4 with 16 channel and 8 message labels
CASES = [
    ("s2", {}, 1030), ("s2", {}, 1), ("s2", bucket(3), 513), ("s2", bucket(1), 513), ("s2", bucket(2), 513), ("s2", SKEW0, 513),
    ("s1", {}, 513), ("s1", SKEW0, 1030),
    ("s3", {}, 513),
    ("s4", {}, 513), ("s4", bucket(2), 1030), ("s4", SKEW0, 513),
    ("s7", {}, 513), ("s7", SKEW0, 1),
    ("s8", {}, 513),
    ("c8m16", {}, 513), ("c8m16", SKEW0, 1030),
    ("c4m4", {}, 513), ("c4m4", bucket(1), 1),
    ("c2m2", {}, 513), ("c2m2", SKEW0, 1030),
    ("grow", {}, 1030), ("grow", bucket(3), 513), ("grow", SKEW0, 513),
]


def _id(c):
    return f"{c[0]}-{'-'.join(k[8:].lower() + v for k, v in c[1].items()) or 'natural'}-{c[2]}"


def _create(name, kn, monkeypatch):
    dec, desc = sc.describe(None, dict(sc.STREAMING, **kn), monkeypatch, device=0, cd=codec(name))
    assert desc["resident"] == 0 and desc["use_fast"] == 1 and desc["skewed_pipeline"] == int("LUTLDPC_SKEW" not in kn), desc
    if "LUTLDPC_FUSED_BUCKET_MIN" in kn:
        assert desc["fused_bucket"] == int(kn["LUTLDPC_FUSED_BUCKET_MIN"]), desc
    elif name in sc.CODES:
        assert desc["fused_bucket"] == sc.natural_bucket(name), desc
    else:
        assert desc["fused_bucket"] == 0, desc
    assert {c["kernel"] for c in desc["vn_classes"]} == {"vn_balanced_fast_kernel"}, desc
    return dec, desc


def _decode(dec, name, n):
    cd = codec(name)
    cha, msg = labels(name, n)
    cache = oracle_cache(("root_rows", name, n))
    return [compare(cd, dec, cha, msg, psc, pisc, flat=True, cache=cache) for psc, pisc in sc.EXIT_MODES][0]


@pytest.mark.parametrize("name,kn,n", CASES, ids=[_id(c) for c in CASES])
def test_root_rows(name, kn, n, monkeypatch):
    dec, desc = _create(name, kn, monkeypatch)
    assert desc["pack"] == 2 and [c["root_rows"] for c in desc["vn_classes"]] == [int(c["deg"] >= 3) for c in desc["vn_classes"]], desc
    assert any(c["root_rows"] for c in desc["vn_classes"])
    it = _decode(dec, name, n)
    if n >= 513:           # with both exit tests on: frames that leave early (frozen under masked stores), late, and not at all
        assert (it == 0).any() and (it < 0).any() and ((it > 0).any() or name == "c2m2"), np.unique(it, return_counts=True)
    dec.close()


@pytest.mark.parametrize("name,kn,n", [("s2", {}, 513), ("s2", SKEW0, 513), ("c8m16", {}, 1030)], ids=["s2-fused", "s2-per_class", "c8m16-fused"])
def test_byte_rows_keep_the_byte_look_up(name, kn, n, monkeypatch):
    """LUTLDPC_PACK=1: the old form is reported (root_rows 0 in every class) and still exact, on the batches of the nibble-row cases."""
    dec, desc = _create(name, dict(kn, LUTLDPC_PACK="1"), monkeypatch)
    assert desc["pack"] == 1 and not any(c["root_rows"] for c in desc["vn_classes"]), desc
    _decode(dec, name, n)
    dec.close()
