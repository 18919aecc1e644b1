"""Failed frames captured on the device (Decoder / Codec / BerSim.error_events and the command line): records, sorted error
positions, unsatisfied checks and the two profiles against a few lines of numpy fed the oracle's decided bits.  Every comparison
is exact equality of integer arrays."""
import functools

import numpy as np
import pytest

import lut_ldpc_amd as L
from lut_ldpc_amd import err_events as ee
from events_helpers import SELECTS, assert_equal, expected, syndrome
from helpers import CODES, ROOT, compare, oracle_codec, product_decoder

pytestmark = pytest.mark.gpu

SNR, SEED, STREAM = 2.5, 7, 1


@functools.lru_cache(maxsize=None)
def _oracle_case(name, B):
    """Labels of the oracle's sampler (all-zero codeword) and the oracle's decode of them with both exit tests on -- computed once."""
    cd = oracle_codec(name)
    cha, msg, unc = cd.sample_labels(SNR, cd.rate, SEED, STREAM, 0, B)
    cd.set_exit_conditions(cd.max_iters, True, True)
    bits, it = cd.lut_decode_batch(cha, msg)
    for a in (cha, msg, bits, it):
        a.setflags(write=False)
    return cd, cha, msg, bits, it


def _graph(cd):
    return cd.code.dv, cd.code.dc, cd.code.cn_msg_idx


def _check_against_helper(dec, cd, cha, msg, bits, it, sent=None, sizes=((8, 8), (128, 160)), max_frames=None):
    K, B = cd.code.nvar - cd.code.nchk, len(bits)
    for max_pos, max_chk in sizes:
        for select in SELECTS:
            mf = B if max_frames is None else max_frames
            got = dec.error_events(cha, msg, sent=sent, select=select, max_frames=mf, max_pos=max_pos, max_chk=max_chk, profiles=True)
            assert_equal(got, expected(bits, sent, it, _graph(cd), K, select, mf, max_pos, max_chk), (select, max_pos))


def _check_case(name, B):
    cd, cha, msg, bits, it = _oracle_case(name, B)
    dec = product_decoder(cd)
    dec.set_exit_conditions(cd.max_iters, True, True)
    _check_against_helper(dec, cd, cha, msg, bits, it)
    # twice into the same profile arrays doubles them; the profiles are the column sums of the error and syndrome matrices
    one = dec.error_events(cha, msg, profiles=True)
    two = dec.error_events(cha, msg, profiles=(one.node_errors.copy(), one.check_fails.copy()))
    assert (one.node_errors == bits.sum(0)).all() and (one.check_fails == syndrome(bits, *_graph(cd)).sum(0)).all()
    assert (two.node_errors == 2 * one.node_errors).all() and (two.check_fails == 2 * one.check_fails).all() and one.node_errors.sum() > 0
    # max_frames = 100: the first 100 selected frames in frame order, the total still reported
    n_fail = int((bits.sum(1) > 0).sum())
    few = dec.error_events(cha, msg, max_frames=min(100, n_fail // 2), max_pos=8, max_chk=8)
    assert few.n_selected == n_fail and few.n_stored == min(100, n_fail // 2)
    assert few.events[:, 0].tolist() == np.flatnonzero(bits.sum(1) > 0)[:few.n_stored].tolist()
    assert_equal(few, expected(bits, None, it, _graph(cd), cd.code.nvar - cd.code.nchk, "codeword", few.n_stored, 8, 8)[:4] + (None, None))
    dec.close()
    return bits, it


def test_nibble_rows_two_frame_groups_ragged_tail():
    """n500_q4_i8, 1100 frames = two groups of 512 and a tail of 76.  With the oracle: 681 frames with codeword errors, 93 of them
    with clean information bits, none undetected; largest weight 71, 574 of weight <= 8, largest syndrome weight 110; 11 frames
    left through the exit test, and the code is negative exactly where the syndrome is non-zero."""
    cd, cha, msg, bits, it = _oracle_case("n500_q4_i8", 1100)
    K = cd.code.nvar - cd.code.nchk
    cw, syn = bits.sum(1), syndrome(bits, *_graph(cd)).sum(1)
    assert ((cw > 0) & (bits[:, :K].sum(1) == 0)).sum() >= 50                # failures the counters cannot see
    assert ((cw > 0) & (cw <= 8)).sum() >= 50 and (cw > 8).sum() >= 50        # both sides of max_pos = 8
    assert cw.max() <= 128 and syn.max() <= 160                               # the large sizes truncate nothing
    assert ((it < 0) == (syn > 0)).all() and ((it > 0) & (it < cd.max_iters)).sum() >= 1
    _check_case("n500_q4_i8", 1100)


def test_byte_rows():
    """reg36_n1000_q5 (32 labels: byte rows, groups of 256 frames), 520 frames = two groups and a tail of 8.  With the oracle: 75
    failing frames, largest weight 26, 185 frames that left through the exit test."""
    cd, cha, msg, bits, it = _oracle_case("reg36_n1000_q5", 520)
    cw = bits.sum(1)
    assert (cw > 0).sum() >= 20 and cw.max() <= 128 and ((it > 0) & (it < cd.max_iters)).sum() >= 20
    assert product_decoder(cd).describe()["tile_frames"] == 256
    _check_case("reg36_n1000_q5", 520)


def test_placed_errors_through_sent():
    """sent = decided bits ^ pattern: the capture sees exactly the pattern as the error positions."""
    cd, cha, msg, bits, it = _oracle_case("n500_q4_i8", 1100)
    N, K, B, P = cd.code.nvar, cd.code.nvar - cd.code.nchk, 1100, 8
    dec = product_decoder(cd)
    dec.set_exit_conditions(cd.max_iters, True, True)
    rng = np.random.default_rng(5)
    pat = np.zeros((B, N), np.uint8)
    pat[0, 0] = 1                                                             # single errors at both ends of the node range
    pat[511, N - 1] = 1                                                       # (last frame of the first group; beyond K_info)
    pat[512, rng.choice(N, P, replace=False)] = 1                             # exactly max_pos (first frame of the second group)
    pat[B - 1, rng.choice(N, P + 1, replace=False)] = 1                       # one more than max_pos (last frame of the ragged tail)
    pat[100] = 1                                                              # all N nodes wrong
    pat[200, K + rng.choice(N - K, 5, replace=False)] = 1                     # parity part only
    _check_against_helper(dec, cd, cha, msg, bits, it, sent=bits ^ pat, sizes=((P, P), (N, 160)))
    got = {s: dec.error_events(cha, msg, sent=bits ^ pat, select=s, max_pos=P, max_chk=P) for s in ("codeword", "info")}
    assert got["codeword"].events[:, 0].tolist() == [0, 100, 200, 511, 512, B - 1]
    assert got["info"].events[:, 0].tolist() == [f for f in (0, 100, 200, 511, 512, B - 1) if pat[f, :K].any()] and 200 not in got["info"].events[:, 0]
    ev = got["codeword"]
    assert ev.events[:, 2].tolist() == [1, N, 5, 1, P, P + 1] and ev.events[:, 6].tolist() == [1, P, 5, 1, P, P]
    assert ev.positions[0].tolist() == [0] + [-1] * (P - 1) and ev.positions[3].tolist() == [N - 1] + [-1] * (P - 1)
    assert ev.positions[1].tolist() == list(range(P)) and ev.positions[4].tolist() == np.flatnonzero(pat[512]).tolist()
    assert ev.positions[5].tolist() == np.flatnonzero(pat[B - 1])[:P].tolist()
    # one pattern on a frame the decoder reported as converged, others on frames it flagged: `undetected` selects exactly that one
    good, bad = np.flatnonzero(it >= 0), np.flatnonzero(it < 0)
    assert len(good) > 10 and len(bad) > 10
    pat2 = np.zeros((B, N), np.uint8)
    pat2[good[7], 3] = 1
    pat2[bad[:3], 4] = 1
    und = dec.error_events(cha, msg, sent=bits ^ pat2, select="undetected", max_pos=P, max_chk=P)
    assert und.n_selected == 1 and und.events[:, 0].tolist() == [good[7]] and und.events[0, 1] >= 0 and und.positions[0, 0] == 3
    assert_equal(und, expected(bits, bits ^ pat2, it, _graph(cd), K, "undetected", 1024, P, P)[:4] + (None, None))
    # no error at all: nothing selected, empty arrays
    none = dec.error_events(cha, msg, sent=bits, select="codeword", max_pos=P, max_chk=P, profiles=True)
    assert none.n_selected == 0 and none.events.shape == (0, 8) and none.positions.shape == (0, P) and none.node_errors.sum() == 0
    # every frame wrong
    every = np.zeros((B, N), np.uint8)
    every[np.arange(B), np.arange(B) % N] = 1
    got = dec.error_events(cha, msg, sent=bits ^ every, max_frames=B, max_pos=P, max_chk=P)
    assert got.n_selected == B and got.n_stored == B and (got.positions[:, 0] == np.arange(B) % N).all() and (got.positions[:, 1:] == -1).all()
    dec.close()


@functools.lru_cache(maxsize=None)
def _n500_with_generator():
    pcd = L.Codec(CODES / "rate0.50_dv02-17_dc08-09_lut_q4_N500.alist", with_generator=True, device=0)
    pcd.design_luts(sigma2=0.88 ** 2, max_iters=8)
    return pcd


@pytest.mark.parametrize("zero", [True, False])
def test_three_codeword_sources(zero):
    """Codec.error_events (all-zero codeword / codewords of the device encoder) equals Decoder.error_events fed the labels of the
    same frames and their codewords from the host; its codes, data-bit errors and uncoded errors are those of sim_batch."""
    pcd = _n500_with_generator()
    pcd.set_exit_conditions(8, True, True)
    B, B1, f0 = 1100, 601, 2 ** 32 + 11
    dec = pcd.decoder()
    kw = dict(max_frames=B, max_pos=16, max_chk=16)
    got = pcd.error_events(SNR, SEED, STREAM, f0, B, zero_codeword=zero, profiles=True, **kw)
    cha, msg, cw = pcd.sample_labels(SNR, SEED, STREAM, f0, B, zero_codeword=zero)
    if not zero:
        assert (cw == pcd.encode_random(SEED, STREAM, f0, B)).all() and 0.3 < cw.mean() < 0.7
    ref = dec.error_events(cha, msg, sent=None if zero else cw, k_info=pcd.ninfo, profiles=True, **kw)
    assert got.n_selected == ref.n_selected > 100
    cols = [0, 1, 2, 3, 4, 6, 7]
    assert (got.events[:, cols] == ref.events[:, cols]).all() and (got.positions == ref.positions).all() and (got.checks == ref.checks).all()
    assert (got.node_errors == ref.node_errors).all() and (got.check_fails == ref.check_fails).all()
    stats = pcd.sim_batch(SNR, SEED, STREAM, f0, B, zero_codeword=zero)
    assert (got.events[:, [1, 3, 5]] == stats[got.events[:, 0]][:, [0, 2, 3]]).all() and got.events[:, 5].sum() > 0
    # a frame error of the counters is a captured frame
    assert set(np.flatnonzero(stats[:, 1]).tolist()) <= set(got.events[:, 0].tolist())
    # the batch split into two calls: the concatenated events, the same profile sums
    a = pcd.error_events(SNR, SEED, STREAM, f0, B1, zero_codeword=zero, profiles=True, **kw)
    b = pcd.error_events(SNR, SEED, STREAM, f0 + B1, B - B1, zero_codeword=zero, profiles=(a.node_errors, a.check_fails), **kw)
    eb = b.events.copy()
    eb[:, 0] += B1
    assert (np.concatenate([a.events, eb]) == got.events).all() and (np.concatenate([a.positions, b.positions]) == got.positions).all()
    assert (np.concatenate([a.checks, b.checks]) == got.checks).all() and a.n_selected + b.n_selected == got.n_selected
    assert (b.node_errors == got.node_errors).all() and (b.check_fails == got.check_fails).all()


def test_streaming_decode_path(monkeypatch):
    """LUTLDPC_RESIDENT=0: the streaming kernels (the N=500 code is otherwise decoded out of LDS) leave the same rows."""
    monkeypatch.setenv("LUTLDPC_RESIDENT", "0")
    cd, cha, msg, bits, it = _oracle_case("n500_q4_i8", 1100)
    dec = product_decoder(cd)
    assert dec.describe()["resident"] == 0
    dec.set_exit_conditions(cd.max_iters, True, True)
    _check_against_helper(dec, cd, cha, msg, bits, it, sizes=((8, 8),))
    dec.close()


def test_compaction_path(monkeypatch):
    """A dual-diagonal code at nine frame groups with compaction forced on as in tests/test_05: frames move between rows during
    the decode; the capture reads the rows after they are back in the caller's order."""
    from helpers import awgn_labels, designed_codec, write_ira_alist
    for k, v in (("LUTLDPC_RESIDENT", "0"), ("LUTLDPC_COMPACT", "1"), ("LUTLDPC_COMPACT_FIRST", "2"),
                 ("LUTLDPC_COMPACT_EVERY", "2"), ("LUTLDPC_COMPACT_MARGIN", "0")):
        monkeypatch.setenv(k, v)
    K, M, sig, I = 840, 420, 0.62, 16
    cd = designed_codec("test55-ira", lambda path: write_ira_alist(path, K, M, 3, seed=K + I), sigma=sig, max_iters=I, nq_msg=16)
    dec = product_decoder(cd)
    assert dec.describe()["compaction"] == 1 and dec.describe()["skewed_pipeline"] == 1
    B = 512 * 8 + 77
    cha, msg, _ = awgn_labels(cd, B, -10 * np.log10(2 * cd.rate * sig * sig) + 0.25, seed=B)
    cd.set_exit_conditions(I, True, True)
    dec.set_exit_conditions(I, True, True)
    bits, it = cd.lut_decode_batch_flat(cha, msg)
    assert (it < 0).sum() > 0 and len(set(it.tolist())) > 5
    for select in ("codeword", "failed"):
        got = dec.error_events(cha, msg, select=select, max_frames=B, max_pos=32, max_chk=32, profiles=True)
        assert_equal(got, expected(bits, None, it, _graph(cd), K, select, B, 32, 32), select)
    dec.close()


def test_the_decode_is_untouched_by_a_capture():
    cd, cha, msg, bits, it = _oracle_case("n500_q4_i8", 1100)
    dec = product_decoder(cd)
    dec.set_exit_conditions(cd.max_iters, True, True)
    ev, gb, gi = dec.error_events(cha, msg, profiles=True, decode=True)
    assert (gb == bits).all() and (gi == it).all()
    assert (compare(cd, dec, cha, msg, True, True) == it).all()
    compare(cd, dec, cha, msg, False, False)
    cd.set_exit_conditions(cd.max_iters, True, True)
    pcd = _n500_with_generator()
    pcd.set_exit_conditions(8, True, True)
    before = pcd.sim_batch(SNR, SEED, STREAM, 0, 700, zero_codeword=False)
    pcd.error_events(SNR, SEED, STREAM, 0, 700, zero_codeword=False, profiles=True)
    assert (pcd.sim_batch(SNR, SEED, STREAM, 0, 700, zero_codeword=False) == before).all()
    dec.close()


def test_bersim_error_events_and_the_command_line(tmp_path):
    """BerSim.error_events uses the simulation's own seed, stream and codeword setting; the command line loops it in batches and
    writes global frame indices, the profiles and the derived curves; a captured frame replays through sim.batch."""
    import shutil
    from lut_ldpc_amd.ber_sim import BerSim
    base = tmp_path
    (base / "codes").mkdir(); (base / "trees").mkdir()
    shutil.copy(CODES / "rate0.50_dv02-17_dc08-09_lut_q4_N500.alist", base / "codes")
    txt = (ROOT / "data" / "params" / "ber.ini.irregular.example").read_text()
    txt = txt.replace("Nframes  = 1e2", "Nframes  = 1000\n   batch_frames = 600").replace("max_iter = 50", "max_iter = 8")
    assert "batch_frames = 600" in txt and "max_iter = 8" in txt
    ini = base / "p.ini"
    ini.write_text(txt)
    out = base / "o.npz"
    assert ee.main(["-p", str(ini), "-b", str(base), "--snr-index", "5", "--frames", "1000", "--select", "info", "--max-frames", "400", "--max-pos", "12",
                    "--max-chk", "10", "-o", str(out)]) == 0
    z = np.load(out)
    sim = BerSim(ini, base, 0, "", 0)
    assert not sim.zero_codeword and sim.batch_frames == 600
    dv, dc, _, _ = sim.code()
    prof = (np.zeros(len(dv), np.int64), np.zeros(len(dc), np.int64))
    a = sim.error_events(5, 0, 600, select="info", max_frames=400, max_pos=12, max_chk=10, profiles=prof)
    b = sim.error_events(5, 600, 400, select="info", max_frames=400 - a.n_stored, max_pos=12, max_chk=10, profiles=prof)
    assert 20 < a.n_stored < 400 and b.n_stored > 20                  # (2.5 dB, 8 iterations: about half of the frames have data-bit errors)
    eb = b.events.copy()
    eb[:, 0] += 600
    want = np.concatenate([a.events, eb])
    assert len(want) == min(400, a.n_selected + b.n_selected) and (z["events"] == want).all() and (np.diff(z["events"][:, 0]) > 0).all() and z["events"][:, 0].max() >= 600
    assert (z["positions"] == np.concatenate([a.positions, b.positions])).all() and (z["checks"] == np.concatenate([a.checks, b.checks])).all()
    assert (z["node_errors"] == prof[0]).all() and (z["check_fails"] == prof[1]).all() and prof[0].sum() > 0
    assert int(z["n_selected"]) == a.n_selected + b.n_selected and int(z["frames"]) == 1000
    assert float(z["snr_db"]) == sim.snr_db[5] and int(z["stream"]) == 5 and int(z["seed"]) == 0
    d = ee.derive(want, prof[0], prof[1], dv, dc, 1000)
    for k, v in d.items():
        assert (z[k] == v).all(), k
    assert z["vn_degrees"].tolist() == sorted(set(dv.tolist())) and z["cw_error_histogram"].sum() == len(want)
    # replay: the frame index addresses the frame
    stats = sim.batch(5, 0, 1000)
    assert (want[:, [1, 3, 5]] == stats[want[:, 0]][:, [0, 2, 3]]).all()
    for r in want[[0, len(want) // 2, len(want) - 1]]:
        s = sim.batch(5, int(r[0]), 1)[0]
        assert s[0] == r[1] and s[2] == r[3] and s[2] > 0
    sim.close()
