"""Message-label histograms counted on the device (Decoder.message_histogram and the layers above it): against the oracle's text,
against the decoder's own raw trace for batches of several frame groups with ragged tails, with sent bits, accumulated over
calls -- every comparison is exact equality of int64 arrays -- and the decode of the same handle afterwards."""
import functools

import numpy as np
import pytest

import lut_ldpc_amd as L
from lut_ldpc_amd import msg_stats as ms
from helpers import CODES, awgn_labels, compare, oracle_codec, product_decoder
from stats_helpers import EXITS, ORACLE_CASES, hist_from_printed, hist_from_trace, oracle_inputs, oracle_printed

pytestmark = pytest.mark.gpu


def _groups(cd, by):
    c = cd.code
    if by == "mod256":
        return (np.arange(c.nedges) % 256).astype(np.int32), 256
    g, degrees = ms.edge_groups(c.dv, c.dc, c.cn_msg_idx, by)
    return g, len(degrees)


def _check_text(name, level):
    cd, cha, msg = oracle_inputs(name)
    I, nq = cd.max_iters, int(max(cd.nq_msg))
    dec = product_decoder(cd)
    for psc, pisc in EXITS:
        it, printed = oracle_printed(name, psc, pisc, level)
        if psc and level == 3:
            # every kind of return value the input can give is in it (zero / mid / +I / -I)
            kinds = [(it == 0).sum(), ((it > 0) & (it < I)).sum(), (it == I).sum(), (it == -I).sum()]
            assert kinds[0] >= 1 and kinds[2] >= 1 and kinds[3] >= 1, kinds
            assert kinds[1] >= 1 or name == "reg36_n1000_m6", kinds
        dec.set_exit_conditions(I, psc, pisc)
        for by in ("vn", "cn"):
            group, ng = _groups(cd, by)
            dec.set_edge_groups(group, ng)
            want_active, _ = hist_from_printed(printed, it, ms.n_dumps(I, level), group, ng, nq)
            got, bits, its = dec.message_histogram(cha, msg, level=level, mode="active")
            assert (its == it).all()
            assert got.dtype == np.int64 and got.shape == want_active.shape
            assert (got == want_active).all(), (name, psc, by, np.argwhere(got != want_active)[:4])
            if not psc:
                # exit tests off: the reference prints every dump of every frame, which is what mode "all" counts whatever the exits
                want_all = want_active
                for p2, pi2 in EXITS:
                    dec.set_exit_conditions(I, p2, pi2)
                    got_all = dec.message_histogram(cha, msg, level=level, mode="all", decode=False)
                    assert (got_all == want_all).all(), (name, p2, by)
                dec.set_exit_conditions(I, psc, pisc)
    dec.close()


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_histogram_equals_the_oracle_text_level_3(name):
    if name == "n500_q4_i8":
        cd = oracle_codec(name)
        assert _groups(cd, "vn")[1] == 4 and _groups(cd, "cn")[1] == 3
    _check_text(name, 3)


def test_histogram_equals_the_oracle_text_level_2():
    _check_text("reg36_n1000_mixed", 2)


@pytest.mark.parametrize("name,B", [("n500_q4_i8", 515), ("reg36_n1000_q5", 259), ("reg36_n1000_q6", 259), ("reg36_n1000_m2", 1027)])
def test_several_frame_groups_with_a_ragged_tail_against_the_raw_trace(name, B):
    """More than one frame group (512 frames of nibble rows, 256 of byte rows) and a last group that is almost empty; alphabets of
    2, 16, 32 and 64 labels; 256 groups, the degree classes, and the one-group default."""
    cd = oracle_codec(name)
    I, nq, E = cd.max_iters, int(max(cd.nq_msg)), cd.code.nedges
    dec = product_decoder(cd)
    assert B > dec.describe()["tile_frames"] and B % dec.describe()["tile_frames"] <= 3
    cha, msg, _ = awgn_labels(cd, B, 2.6, seed=B)
    cha[5] = cd.nq_cha - 1; msg[5] = cd.nq_msg[0] - 1
    dec.set_exit_conditions(I, False, False)
    _, _, trace = dec.lut_decode_batch_trace(cha, msg, 3, E)
    dec.set_exit_conditions(I, True, True)
    _, it = dec.lut_decode_batch(cha, msg)
    assert len(set(it.tolist())) >= 2
    last = {"all": np.full(B, ms.n_dumps(I, 3)), "active": ms.last_dump(it, I, 3)}
    for by in (("mod256", "none", "cn") if name == "n500_q4_i8" else ("none", "mod256")):
        group, ng = _groups(cd, by)
        if by == "none":
            dec.set_edge_groups(None)
        else:
            dec.set_edge_groups(group, ng)
        for mode in ("all", "active"):
            want = hist_from_trace(trace, last[mode], group, ng, nq)
            got, bits, its = dec.message_histogram(cha, msg, level=3, mode=mode)
            assert (its == it).all()
            assert (got == want).all(), (name, by, mode, np.argwhere(got != want)[:4])
    # level 2 is every second dump of level 3 plus the initial one; more label slots than the alphabet stay empty
    got2 = dec.message_histogram(cha, msg, level=2, mode="all", n_labels=nq + 3, decode=False)
    want3 = hist_from_trace(trace, last["all"], group, ng, nq)
    assert (got2[..., :nq] == want3[[0] + list(range(2, 2 * I + 1, 2))]).all() and got2[..., nq:].sum() == 0
    dec.close()


@functools.lru_cache(maxsize=None)
def _n500_with_generator():
    pcd = L.Codec(CODES / "rate0.50_dv02-17_dc08-09_lut_q4_N500.alist", with_generator=True, device=0)
    pcd.design_luts(sigma2=0.88 ** 2, max_iters=8)
    return pcd


def test_sent_bits_split_the_histogram():
    pcd = _n500_with_generator()
    I, B, snr, seed, stream, f0 = 8, 70, 2.0, 2 ** 33 + 5, 2, 2 ** 32 + 11
    dv, dc, cn = pcd.graph()
    E = pcd.nedges
    edge_vn = np.repeat(np.arange(pcd.nvar), dv)
    dec = pcd.decoder()
    assert dec.describe()["generator"]["K"] == pcd.ninfo
    cw = pcd.encode_random(seed, stream, f0, B)
    cha, msg, cw_host = pcd.sample_labels(snr, seed, stream, f0, B, zero_codeword=False)
    assert (cw == cw_host).all() and 0.3 < cw.mean() < 0.7
    for by in ("vn", "cn"):
        group, degrees = ms.edge_groups(dv, dc, cn, by)
        dec.set_edge_groups(group, len(degrees))
        for psc, pisc in EXITS:
            pcd.set_exit_conditions(I, False, False)
            _, _, trace = dec.lut_decode_batch_trace(cha, msg, 3, E)
            pcd.set_exit_conditions(I, psc, pisc)
            _, it = pcd.lut_decode_batch(cha, msg)
            for mode in ("all", "active"):
                last = ms.last_dump(it, I, 3) if mode == "active" else np.full(B, 1 + 2 * I)
                want = hist_from_trace(trace, last, group, len(degrees), 16, cw[:, edge_vn])
                got = pcd.message_histogram(snr, seed, stream, f0, B, zero_codeword=False, level=3, mode=mode)
                assert (got == want).all(), (by, psc, mode)
                assert got[:, :, 1].sum() > 0
                # the same labels and codewords through the decoder-level entry (host codewords -> sent-bit rows)
                got_d = dec.message_histogram(cha, msg, sent=cw, level=3, mode=mode, decode=False)
                assert (got_d == want).all()
    # the all-zero codeword: nothing under a sent 1
    got0 = pcd.message_histogram(snr, seed, stream, f0, B, zero_codeword=True, level=3, mode="all")
    cha0, msg0, _ = pcd.sample_labels(snr, seed, stream, f0, B, zero_codeword=True)
    pcd.set_exit_conditions(I, False, False)
    _, _, trace0 = dec.lut_decode_batch_trace(cha0, msg0, 3, E)
    assert got0[:, :, 1].sum() == 0 and (got0 == hist_from_trace(trace0, np.full(B, 1 + 2 * I), group, len(degrees), 16)).all()
    dec.set_edge_groups(None)


def test_accumulation_determinism_and_totals():
    pcd = _n500_with_generator()
    # 3.5 dB: with 8 iterations about 4 % of the frames leave through an exit test before the last iteration (the oracle on 1100
    # frames: 43 of them; none at 1.5 dB), so the mask of mode "active" has frames to remove
    I, B, B1, snr, seed, stream = 8, 1100, 601, 3.5, 7, 1
    dv, dc, cn = pcd.graph()
    group, degrees = ms.edge_groups(dv, dc, cn, "vn")
    dec = pcd.decoder()
    dec.set_edge_groups(group, len(degrees))
    pcd.set_exit_conditions(I, True, True)
    assert B1 % dec.describe()["tile_frames"] != 0
    for zero in (True, False):
        for mode in ("all", "active"):
            one = pcd.message_histogram(snr, seed, stream, 0, B, zero_codeword=zero, level=3, mode=mode)
            two = pcd.message_histogram(snr, seed, stream, 0, B1, zero_codeword=zero, level=3, mode=mode)
            ret = pcd.message_histogram(snr, seed, stream, B1, B - B1, zero_codeword=zero, level=3, mode=mode, hist=two)
            assert ret is two and (one == two).all(), (zero, mode)
            assert (pcd.message_histogram(snr, seed, stream, 0, B, zero_codeword=zero, level=3, mode=mode) == one).all()
            it = pcd.sim_batch(snr, seed, stream, 0, B, zero_codeword=zero)[:, 0]
            last = ms.last_dump(it, I, 3) if mode == "active" else np.full(B, 1 + 2 * I)
            frames_at = (last[None, :] > np.arange(1 + 2 * I)[:, None]).sum(1)
            assert (one.sum((2, 3)) == frames_at[:, None] * np.bincount(group)[None, :]).all(), (zero, mode)
            if mode == "active":
                assert 0 < frames_at[-1] < B
    dec.set_edge_groups(None)


@pytest.mark.parametrize("name", ["n500_q4_i8", "reg36_n1000_q5"])
def test_the_decode_is_untouched_by_a_histogram_call(name):
    cd, cha, msg = oracle_inputs(name)
    I = cd.max_iters
    dec = product_decoder(cd)
    group, ng = _groups(cd, "vn")
    dec.set_edge_groups(group, ng)
    for psc, pisc in ((True, True), (True, False), (False, False)):
        dec.set_exit_conditions(I, psc, pisc)
        for mode in ("all", "active"):
            _, bits, its = dec.message_histogram(cha, msg, level=3, mode=mode)
            it = compare(cd, dec, cha, msg, psc, pisc)           # (sets the same exit conditions again and decodes on both sides)
            assert (its == it).all() and (bits == dec.lut_decode_batch(cha, msg)[0]).all()
    # the exit conditions read back as they were set: a decode after the call behaves as configured, here with the early exits
    dec.set_exit_conditions(I, True, True)
    dec.message_histogram(cha, msg, level=2, mode="all", decode=False)
    _, it = dec.lut_decode_batch(cha, msg)
    cd.set_exit_conditions(I, True, True)
    assert (it == cd.lut_decode_batch(cha, msg)[1]).all() and (it == 0).sum() >= 1 and ((it > 0) & (it < I)).sum() >= 1
    dec.close()


def test_bersim_message_histogram_and_the_command_line(tmp_path):
    """BerSim.message_histogram uses the simulation's own seed, stream and codeword setting; the command line loops it in batches
    and writes the histogram with the derived curves."""
    import shutil
    from lut_ldpc_amd.ber_sim import BerSim
    from helpers import ROOT
    base = tmp_path
    (base / "codes").mkdir(); (base / "trees").mkdir()
    shutil.copy(CODES / "rate0.50_dv02-17_dc08-09_lut_q4_N500.alist", base / "codes")
    # the irregular example (random codewords: the sent bits come from the device encoder), 8 iterations, batches of 600 frames
    txt = (ROOT / "data" / "params" / "ber.ini.irregular.example").read_text()
    txt = txt.replace("Nframes  = 1e2", "Nframes  = 1000\n   batch_frames = 600").replace("max_iter = 50", "max_iter = 8")
    assert "batch_frames = 600" in txt and "max_iter = 8" in txt
    ini = base / "p.ini"
    ini.write_text(txt)
    out = base / "o.npz"
    assert ms.main(["-p", str(ini), "-b", str(base), "--snr-index", "3", "--frames", "1000", "--mode", "active", "--by", "cn", "-o", str(out)]) == 0
    z = np.load(out)
    sim = BerSim(ini, base, 0, "", 0)
    dv, dc, cn, nq = sim.code()
    group, degrees = ms.edge_groups(dv, dc, cn, "cn")
    sim.decoder().set_edge_groups(group, len(degrees))
    assert sim.snr_db[3] == 1.5 and not sim.zero_codeword and sim.batch_frames == 600
    want = sim.message_histogram(3, 0, 1000, 3, "active")
    it = sim.batch(3, 0, 1000)[:, 0]
    assert (z["hist"] == want).all() and z["group_degrees"].tolist() == degrees.tolist() and z["alphabets"].tolist() == [16] * 17
    frames_at = (ms.last_dump(it, 8, 3)[None, :] > np.arange(17)[:, None]).sum(1)
    assert (want.sum((2, 3)) == frames_at[:, None] * np.bincount(group)[None, :]).all()
    assert z["error_probability"].shape == (17, len(degrees)) and (z["mutual_information"][0] > 0.3).all()
    assert want[:, :, 1].sum() > 0
    sim.close()
