"""Message statistics without a GPU: the oracle's text as the reference histogram and the rule for the dumps a frame prints,
the derived quantities on hand-made histograms, the edge groupings, and the argument errors of a host-only handle."""
import numpy as np
import pytest

import lut_ldpc_amd as L
from lut_ldpc_amd import msg_stats as ms
from lut_ldpc_amd._capi import ERR_ARG, ERR_STATE

from helpers import oracle_codec, product_decoder
from stats_helpers import EXITS, ORACLE_CASES, hist_from_printed, oracle_inputs, oracle_printed


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_last_dump_is_the_number_of_dumps_in_the_oracle_text(name):
    """Level 3: a frame that returns c prints 0 (c = 0), all 1 + 2I (|c| = I) or 2c dumps (0 < c < I) -- counted in the text."""
    cd, cha, msg = oracle_inputs(name)
    I = cd.max_iters
    for psc, pisc in EXITS:
        it, printed = oracle_printed(name, psc, pisc, 3)
        group, degrees = ms.edge_groups(cd.code.dv, cd.code.dc, cd.code.cn_msg_idx, "vn")
        hist, per_frame = hist_from_printed(printed, it, ms.n_dumps(I, 3), group, len(degrees), int(max(cd.nq_msg)))
        assert (per_frame == ms.last_dump(it, I, 3)).all(), (it[per_frame != ms.last_dump(it, I, 3)], per_frame[per_frame != ms.last_dump(it, I, 3)])
        if psc:
            assert (it == 0).sum() >= 1 and (np.abs(it) == I).sum() >= 1
        else:
            assert (np.abs(it) == I).all() and (per_frame == 1 + 2 * I).all()
        # every printed message is in the histogram: frames at a dump x edges of the group
        frames_at = (ms.last_dump(it, I, 3)[None, :] > np.arange(ms.n_dumps(I, 3))[:, None]).sum(1)
        assert (hist.sum((2, 3)) == frames_at[:, None] * np.bincount(group)[None, :]).all()
        assert hist[:, :, 1].sum() == 0


def test_last_dump_level_2():
    cd, cha, msg = oracle_inputs("n500_q4_i8")
    I = cd.max_iters
    it, printed = oracle_printed("n500_q4_i8", True, True, 2)
    assert ((it > 0) & (it < I)).sum() >= 1
    assert ([len(p) for p in printed] == ms.last_dump(it, I, 2)[it != 0]).all()
    assert ms.last_dump([0, 1, 3, I, -I], I, 2).tolist() == [0, 1, 3, 1 + I, 1 + I]
    assert ms.last_dump([0, 1, 3, I, -I], I, 3).tolist() == [0, 2, 6, 1 + 2 * I, 1 + 2 * I]


def h2(p):
    return -p * np.log2(p) - (1 - p) * np.log2(1 - p)


@pytest.mark.parametrize("nq", [2, 6, 16])
def test_fold_error_probability_and_mutual_information(nq):
    L_ = nq + 2                                                          # more label slots than the alphabet
    # noiseless: a sent 0 always gives the top label, a sent 1 the bottom one
    h = np.zeros((2, L_), np.int64)
    h[0, nq - 1], h[1, 0] = 700, 300
    assert ms.fold(h, nq).tolist() == [0.0] * (nq - 1) + [1.0]
    assert ms.error_probability(h, nq) == 0.0 and ms.mutual_information(h, nq) == pytest.approx(1.0, abs=1e-15)
    # uniform: the label says nothing
    h = np.zeros((2, L_), np.int64)
    h[:, :nq] = 5
    assert ms.mutual_information(h, nq) == pytest.approx(0.0, abs=1e-15) and ms.error_probability(h, nq) == pytest.approx(0.5)
    # the mirror: counts under a sent 1 land on nq-1-label
    h = np.zeros((2, L_), np.int64)
    h[1, 1 % nq] = 4
    assert ms.fold(h, nq)[nq - 1 - 1 % nq] == 1.0
    # leading axes are kept, empty bins give zeros instead of NaN
    hh = np.zeros((3, 2, 2, L_), np.int64)
    hh[1, 0, 0, nq - 1] = 9
    assert ms.fold(hh, nq).shape == (3, 2, nq) and ms.fold(hh, nq)[0].sum() == 0 and ms.mutual_information(hh, nq)[1, 0] == pytest.approx(1.0)
    with pytest.raises(ValueError):
        bad = np.zeros((2, L_), np.int64); bad[0, nq] = 1
        ms.fold(bad, nq)


@pytest.mark.parametrize("p", [0.11, 0.02, 0.5])
def test_two_label_bsc(p):
    n = 10 ** 6
    h = np.array([[round(p * n), n - round(p * n)], [3 * (n - round(p * n)), 3 * round(p * n)]], np.int64)      # sent 1 three times as often: folding normalises
    assert ms.error_probability(h, 2) == pytest.approx(p, abs=1e-12)
    assert ms.mutual_information(h, 2) == pytest.approx(1 - h2(p), abs=1e-12)


def test_six_label_channel_against_the_definition():
    rng = np.random.default_rng(0)
    p0 = rng.random(6); p0 /= p0.sum()
    h = np.stack([np.round(p0 * 10 ** 7), np.round(p0[::-1] * 10 ** 7)]).astype(np.int64)
    p = h[0] / h[0].sum()
    joint = 0.5 * np.stack([p, p[::-1]])
    want = (joint * np.log2(joint / (joint.sum(0, keepdims=True) * 0.5))).sum()
    assert ms.mutual_information(h, 6) == pytest.approx(want, abs=1e-12)
    assert ms.error_probability(h, 6) == pytest.approx(p[:3].sum(), abs=1e-12)


@pytest.mark.parametrize("name", ["n500_q4_i8", "reg36_n1000_q5"])
def test_edge_groups_against_a_direct_construction(name):
    c = oracle_codec(name).code
    dv, dc, cn = np.asarray(c.dv), np.asarray(c.dc), np.asarray(c.cn_msg_idx)
    E = int(dv.sum())
    # by hand: walk the variables / the checks and write the degree of the owner on every edge
    deg_v, deg_c, e = np.zeros(E, int), np.zeros(E, int), 0
    for v in range(len(dv)):
        for _ in range(dv[v]):
            deg_v[e] = dv[v]; e += 1
    k = 0
    for m in range(len(dc)):
        for _ in range(dc[m]):
            deg_c[cn[k]] = dc[m]; k += 1
    for by, deg in (("vn", deg_v), ("cn", deg_c)):
        group, degrees = ms.edge_groups(dv, dc, cn, by)
        assert group.dtype == np.int32 and degrees.tolist() == sorted(set(deg.tolist())) and (degrees[group] == deg).all()
    if name == "n500_q4_i8":
        assert len(ms.edge_groups(dv, dc, cn, "vn")[1]) == 4 and len(ms.edge_groups(dv, dc, cn, "cn")[1]) == 3
    group, degrees = ms.edge_groups(dv, dc, cn, "none")
    assert (group == 0).all() and len(group) == E and len(degrees) == 1
    with pytest.raises(ValueError):
        ms.edge_groups(dv, dc, cn, "edge")


def test_dump_alphabets():
    assert ms.dump_alphabets([16, 16, 8, 8], 3).tolist() == [16, 16, 16, 16, 8, 8, 8, 8, 8]
    assert ms.dump_alphabets([16, 16, 8, 8], 2).tolist() == [16, 16, 8, 8, 8]


def test_argument_errors_on_a_host_only_handle():
    cd = oracle_codec("n500_q4_i8")
    dec = product_decoder(cd, device=-1)
    E, N, I = cd.code.nedges, cd.code.nvar, cd.max_iters
    assert dec.histogram_shape(3) == (1 + 2 * I, 1, 16, E) and dec.histogram_shape(2)[0] == 1 + I
    cha = np.zeros((3, N), np.uint8)

    def code(fn):
        with pytest.raises(L.LutLdpcError) as e:
            fn()
        return e.value.code

    assert code(lambda: dec.message_histogram(cha, cha, level=4)) == ERR_ARG
    assert code(lambda: dec.message_histogram(cha, cha, level=1, hist=np.zeros((1 + 2 * I, 1, 2, 16), np.int64))) == ERR_ARG
    assert code(lambda: dec.message_histogram(cha, cha, level=3, hist=np.zeros((2 * I, 1, 2, 16), np.int64))) == ERR_ARG       # short hist_cap
    assert code(lambda: dec.message_histogram(cha, cha, level=3, n_labels=15)) == ERR_ARG                                     # n_labels too small
    assert code(lambda: dec.message_histogram(cha, cha, level=3, mode=2)) == ERR_ARG
    assert code(lambda: dec.set_edge_groups(np.full(E, 4, np.int32), 4)) == ERR_ARG                                           # group id out of range
    assert code(lambda: dec.set_edge_groups(np.full(E, -1, np.int32), 4)) == ERR_ARG
    assert code(lambda: dec.set_edge_groups(None, 0)) == ERR_ARG and code(lambda: dec.set_edge_groups(None, 257)) == ERR_ARG
    dec.set_edge_groups(np.arange(E, dtype=np.int32) % 256, 256)
    assert dec.histogram_shape(3)[1] == 256
    assert code(lambda: dec.message_histogram(cha, cha, level=3, hist=np.zeros((1 + 2 * I, 1, 2, 16), np.int64))) == ERR_ARG  # short for 256 groups
    # well-formed calls need a device
    assert code(lambda: dec.message_histogram(cha, cha, level=3)) == ERR_STATE
    assert code(lambda: dec.message_histogram(cha, cha, level=2, mode="active")) == ERR_STATE
    dec.set_edge_groups(None)
    assert dec.histogram_shape(3)[1] == 1
    dec.close()
