"""Per-node channel classes of the sampler on the device (lutldpc_decoder_set_node_channels, sample_labels_kernel with a class byte
per node) against the reference of tests/node_channel_cases.py -- the one-table reference of tests/frontend_cases.py, column by
column -- through the C-ABI: sample_labels, sim_batch, sim_batch_random, sim_batch_histogram and sim_batch_events with NULL cells,
the precedence of a non-NULL table (five tables of frontend_cases over a 16-class record), clearing, refused setters; the codec
layer with a punctured, a known and a 3 dB weaker class; ber_sim with the two
Channel keys through the C++ driver and the Python driver.  All integer, all equal bit for bit.  (tests/test_node_channels_cpu.py
holds the cases to the conditions they are built for.)"""
import ctypes as C
import os

import numpy as np
import pytest

import frontend_cases as fc
import node_channel_cases as nc
import lut_ldpc_amd as L
from lut_ldpc_amd._capi import ERR_ARG, LutLdpcError, last_error, lib
from helpers import CODES, oracle_codec, product_decoder, same as _same
from itfile_reader import itload

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def handles():
    """handle name of node_channel_cases.HANDLES -> device decoder, created on first use (its knobs are read at creation) and kept."""
    made = {}

    def get(name):
        if name not in made:
            code, env, T = nc.HANDLES[name]
            old = os.environ.pop("LUTLDPC_PACK", None)
            os.environ.update(env)
            try:
                dec = product_decoder(fc.codec(code), device=0)
            finally:
                os.environ.pop("LUTLDPC_PACK", None)
                if old is not None:
                    os.environ["LUTLDPC_PACK"] = old
            desc = dec.describe()
            assert desc["tile_frames"] == T and desc["pack"] == T // 256, (name, desc["tile_frames"], desc["pack"])
            made[name] = dec
        return made[name]
    yield get
    for dec in made.values():
        dec.close()


def _sample(dec, table, seed, stream, f0, B, cw):
    return dec.sample_labels(table, seed, stream, f0, B, codewords=cw, cha=np.full((B, dec.nvar), 0xEE, np.uint8), msg=np.full((B, dec.nvar), 0xEE, np.uint8))


def _sim(dec, table, seed, stream, f0, B, cw, K, random=False):
    return dec.sim_batch(table, seed, stream, f0, B, K, codewords=cw, random=random, frame_stats=np.full((B, 4), -7, np.int32),
                         cha_out=np.full((B, dec.nvar), 0xEE, np.uint8), bits_out=np.full((B, dec.nvar), 0xEE, np.uint8))


@pytest.mark.parametrize("case", nc.CASES, ids=nc.case_id)
def test_sampler_with_node_channels_equals_the_reference_label_for_label(case, handles):
    c = nc.sampler_case(case)
    dec, N, B, u = handles(case[0]), c["N"], c["B"], c["u"]
    seed, stream, f0 = c["seed"], c["stream"], c["f0"]
    assert dec.nvar == N
    dec.set_node_channels(c["node_class"], c["tables"])
    assert dec.describe()["node_channels"] == {"classes": len(c["tables"]), "nodes": np.bincount(c["node_class"], minlength=len(c["tables"])).tolist()}
    dec.set_generator(c["K"], c["R"], fc.generator_rows(c["K"], c["R"]))
    for sent in ("none", "bytes"):
        want_cha, want_msg, _, cw = nc.reference(case, sent)
        cha, msg = _sample(dec, None, seed, stream, f0, B, cw)
        _same(cha, want_cha, sent + ": channel labels", u)
        _same(msg, want_msg, sent + ": message labels", u)
    # the slicer column and the sampled labels through sim_batch, on host codewords and on those of the device encoder
    for sent in ("bytes", "device"):
        want_cha, _, want_unc, cw = nc.reference(case, sent)
        stats, cha_out, _ = _sim(dec, None, seed, stream, f0, B, None if sent == "device" else cw, N // 2, random=sent == "device")
        _same(cha_out, want_cha, sent + ": sim_batch channel labels", u)
        assert (stats[:, 3] == want_unc).all(), (sent, np.flatnonzero(stats[:, 3] != want_unc)[:8])
    # a table of the caller's wins over the handle's classes: the one-table result on every node
    one = c["tables"][-1]
    want_cha, want_msg, _ = fc.sample(one, seed, stream, f0, B, N, c["cw_bytes"], u=u)
    cha, msg = _sample(dec, one, seed, stream, f0, B, c["cw_bytes"])
    _same(cha, want_cha, "caller's table: channel labels", u)
    _same(msg, want_msg, "caller's table: message labels", u)
    if case[1] == "one":
        # one class equals the `cells` path bit for bit
        a = _sample(dec, None, seed, stream, f0, B, c["cw_bytes"])
        b = _sample(dec, c["tables"][0], seed, stream, f0, B, c["cw_bytes"])
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    dec.set_node_channels(None)
    assert "node_channels" not in dec.describe()


ONE_TABLE_NAMES = ["trivial1", "trivial2", "pins", "boundaries", "dense_q4"]


@pytest.mark.parametrize("handle,bk", [("n33", "T+1"), ("n127_pack1", "T+1"), ("n127_pack1", "1")])
def test_a_callers_table_over_sixteen_classes_equals_the_one_table_reference(handle, bk, handles):
    """With the 16 classes of `mod16` on the handle, sample_labels and sim_batch with each table of frontend_cases are the one-table
    reference frontend_cases.sample, labels and uncoded count, and NULL cells afterwards are still the class reference: the launch
    with no class bytes and one slot of LDS next to the one with 16.  Odd N with its pad node, both row formats, a ragged batch and a
    single frame (on n127: the 35-cell class table needs more than the 33 samples one frame of n33 has)."""
    code, _, T = nc.HANDLES[handle]
    dec, cd = handles(handle), fc.codec(code)
    N, B = cd.code.nvar, fc.batch_size(bk, T)
    seed, stream, f0 = fc.SEED_BIG, 7, fc.F_CARRY
    u = fc.uniforms(seed, stream, f0, B, N)
    cw = np.random.default_rng(B * 1000 + N).integers(0, 256, (B, N), dtype=np.uint8)
    cls = nc.node_classes("mod16", N)
    class_tables = [nc.table(name, u, cd.nq_cha, T, f0) for name in nc.LAYOUT_TABLES["mod16"]]
    dec.set_node_channels(cls, class_tables)

    def check(table, want_sent, want_zero, what):
        cha, msg = _sample(dec, table, seed, stream, f0, B, cw)
        _same(cha, want_sent[0], what + ": channel labels", u)
        _same(msg, want_sent[1], what + ": message labels", u)
        stats, cha_out, _ = _sim(dec, table, seed, stream, f0, B, None, N // 2)
        _same(cha_out, want_zero[0], what + ": sim_batch channel labels", u)
        assert (stats[:, 3] == want_zero[2]).all(), (what, np.flatnonzero(stats[:, 3] != want_zero[2])[:8])

    for name in ONE_TABLE_NAMES:
        one = nc.table(name, u, cd.nq_cha, T, f0)
        check(one, fc.sample(one, seed, stream, f0, B, N, cw, u=u), fc.sample(one, seed, stream, f0, B, N, None, u=u), name)
    check(None, nc.sample(class_tables, cls, seed, stream, f0, B, N, cw, u=u), nc.sample(class_tables, cls, seed, stream, f0, B, N, None, u=u), "classes")
    dec.set_node_channels(None)


def test_clearing_brings_back_the_argument_error_and_a_refused_setter_changes_nothing(handles):
    case = nc.CASES[3]                                       # n127, blocks
    c = nc.sampler_case(case)
    dec, N, B = handles(case[0]), c["N"], c["B"]
    seed, stream, f0 = c["seed"], c["stream"], c["f0"]
    dec.set_node_channels(None)
    out = np.full((B, N), 0xEE, np.uint8)
    p = out.ctypes.data_as(C.POINTER(C.c_uint8))
    stats = np.full((B, 4), -7, np.int32)
    null_cells = {
        "sample_labels": lambda: lib.lutldpc_decoder_sample_labels(dec._h, None, seed, stream, f0, B, None, p, p),
        "sim_batch": lambda: lib.lutldpc_decoder_sim_batch(dec._h, None, seed, stream, f0, B, None, N // 2, stats.ctypes.data_as(C.POINTER(C.c_int32)), None, None),
    }
    for name, call in null_cells.items():
        assert call() == ERR_ARG and "channel cells: NULL member" in last_error(), name
    assert (out == 0xEE).all() and (stats == -7).all()
    dec.set_node_channels(c["node_class"], c["tables"])
    want = nc.reference(case, "none")
    before = dec.describe()["node_channels"]
    t0 = c["tables"][0]
    over = c["node_class"].copy()
    over[N // 2] = len(c["tables"])
    refusals = [
        (c["node_class"], c["tables"] * 5, "n_classes"),                                                  # 20 classes
        (over, c["tables"], "node_class"),
        (c["node_class"], c["tables"][:3] + [dict(t0, cha=np.full_like(t0["cha"], 16))], "alphabet"),
        (c["node_class"], c["tables"][:3] + [dict(t0, thr=t0["thr"][::-1].copy())], "ascend"),
    ]
    for ids, tables, text in refusals:
        with pytest.raises(LutLdpcError, match=text) as refused:
            dec.set_node_channels(ids, tables)
        assert refused.value.code == ERR_ARG
        assert dec.describe()["node_channels"] == before
        cha, msg = _sample(dec, None, seed, stream, f0, B, None)
        assert (cha == want[0]).all() and (msg == want[1]).all(), text
    # replaced on a live handle: the new classes take effect
    dec.set_node_channels(nc.node_classes("evenodd", N), c["tables"][:2])
    w_cha, w_msg, _ = nc.sample(c["tables"][:2], nc.node_classes("evenodd", N), seed, stream, f0, B, N, None, u=c["u"])
    cha, msg = _sample(dec, None, seed, stream, f0, B, None)
    assert (cha == w_cha).all() and (msg == w_msg).all() and (w_cha != want[0]).any()
    dec.set_node_channels(None)
    assert null_cells["sample_labels"]() == ERR_ARG


@pytest.mark.parametrize("handle,bk,snr_a,snr_b", nc.STATS_CASES, ids=[c[0] for c in nc.STATS_CASES])
def test_decode_entries_with_node_channels(handle, bk, snr_a, snr_b, handles):
    """sim_batch and sim_batch_random: the oracle's decode of the reference labels on 24 frames, the handle's own decode of them on all,
    numpy counts; sim_batch_histogram = histogram_batch and sim_batch_events = events_batch fed the reference labels and sent bits."""
    dec = handles(handle)
    for sent in ("bytes", "device"):
        ref = nc.stats_reference(handle, bk, snr_a, snr_b, sent)
        cd, N, B, K, cw, pick = ref["cd"], ref["N"], ref["B"], ref["K"], ref["cw"], ref["pick"]
        dec.set_exit_conditions(cd.max_iters, True, True)
        dec.set_node_channels(ref["node_class"], ref["tables"])
        rnd = sent == "device"
        if rnd:
            G = nc.STATS_GENERATOR_K
            dec.set_generator(G, N - G, fc.generator_rows(G, N - G))
        bits, iters = dec.lut_decode_batch(ref["cha"], ref["msg"])
        assert (iters[pick] == ref["iters"]).all() and (bits[pick] == ref["bits"]).all()
        args = (fc.STATS_SEED, fc.STATS_STREAM, fc.STATS_F0, B)
        assert args[:3] == (nc.STATS_SEED, nc.STATS_STREAM, nc.STATS_F0)
        stats, cha_out, bits_out = _sim(dec, None, *args, None if rnd else cw, K, random=rnd)
        _same(cha_out, ref["cha"], sent + ": channel labels")
        _same(bits_out, bits, sent + ": decided bits")
        err = (bits[:, :K] ^ (cw[:, :K] & 1)).sum(1)
        want = np.stack([iters, err > 0, err, ref["unc"]], axis=1).astype(np.int32)
        bad = np.argwhere(stats != want)
        assert bad.size == 0, (sent, len(bad), bad[:6].tolist(), stats[bad[0][0]], want[bad[0][0]])
        assert (err > 0).any() and (err == 0).any()
        # histograms
        for mode in ("all", "active"):
            want_h = dec.message_histogram(ref["cha"], ref["msg"], sent=cw & 1, level=3, mode=mode, decode=False)
            got_h = dec.sim_batch_histogram(None, *args, codewords=None if rnd else cw, device_codewords=rnd, level=3, mode=mode)
            assert want_h.sum() > 0 and (got_h == want_h).all(), (sent, mode, np.argwhere(got_h != want_h)[:4].tolist())
        # capture
        want_e = dec.error_events(ref["cha"], ref["msg"], sent=cw & 1, select="codeword", max_frames=64, max_pos=32, max_chk=32, profiles=True, k_info=K)
        got_e, ev_stats = dec.sim_batch_events(None, *args, k_info=K, codewords=None if rnd else cw, device_codewords=rnd, select="codeword", max_frames=64,
                                               max_pos=32, max_chk=32, profiles=True)
        assert (ev_stats == want).all()
        assert got_e.n_selected == want_e.n_selected > 0 and got_e.n_stored == want_e.n_stored
        cols = [0, 1, 2, 3, 4, 6, 7]
        assert (got_e.events[:, cols] == want_e.events[:, cols]).all() and (got_e.events[:, 5] == ref["unc"][got_e.events[:, 0]]).all()
        assert (got_e.positions == want_e.positions).all() and (got_e.checks == want_e.checks).all()
        assert (got_e.node_errors == want_e.node_errors).all() and (got_e.check_fails == want_e.check_fails).all()
        # the caller's table on the same handle: the single-table result
        one = ref["tables"][0]
        o_cha, _, o_unc = fc.sample(one, *args, N, cw)
        o_stats, o_out, _ = _sim(dec, one, *args, None if rnd else cw, K, random=rnd)
        assert (o_out == o_cha).all() and (o_stats[:, 3] == o_unc).all()
    dec.set_node_channels(None)


# ---------------------------------------------------------------------------------------------------------------- codec layer
@pytest.mark.parametrize("mode", [0, 1], ids=["cont", "qcha"])
def test_codec_samples_with_its_offset_classes(mode):
    pcd = L.Codec(CODES / f"{nc.BER_ALIST}.alist", with_generator=True, device=0)
    pcd.design_luts(sigma2=0.88 ** 2, max_iters=8)
    pcd.set_initial_message_mode(mode)
    pcd.set_exit_conditions(8, True, True)
    N, snr, seed, stream, f0, B = pcd.nvar, 3.0, 12, 2, 2 ** 32 - 9, 300
    cls = nc.ber_classes(N)
    plain = pcd.sample_labels(snr, seed, stream, f0, B, zero_codeword=False)
    pcd.set_node_channels(cls, [0.0, -INF, INF, -3.0])
    tables = [pcd.node_channel_cells(snr, k) for k in range(4)]
    qm, mp = (pcd.qb_msg, None) if mode == 0 else (None, pcd.cha2msg_map)
    assert nc.same_table(tables[0], pcd.channel_cells(snr)) and nc.same_table(tables[3], pcd.channel_cells(snr - 3.0))
    assert nc.same_table(tables[1], nc.erasure_table(pcd.qb_cha, qm, mp)) and nc.same_table(tables[2], nc.known_table(pcd.qb_cha, qm, mp))
    for zero in (True, False):
        cha, msg, cw = pcd.sample_labels(snr, seed, stream, f0, B, zero_codeword=zero)
        assert cw.any() != zero
        want_cha, want_msg, want_unc = nc.sample(tables, cls, seed, stream, f0, B, N, None if zero else cw)
        _same(cha, want_cha, "codec: channel labels")
        _same(msg, want_msg, "codec: message labels")
        stats = pcd.sim_batch(snr, seed, stream, f0, B, zero_codeword=zero)
        bits, iters = pcd.lut_decode_batch(want_cha, want_msg)
        err = (bits[:, :pcd.ninfo] ^ (cw[:, :pcd.ninfo] & 1)).sum(1)
        assert (stats == np.stack([iters, err > 0, err, want_unc], axis=1)).all()
        dec = pcd.decoder()
        want_h = dec.message_histogram(want_cha, want_msg, sent=cw, level=2, decode=False)
        assert (pcd.message_histogram(snr, seed, stream, f0, B, zero_codeword=zero, level=2) == want_h).all()
        want_e = dec.error_events(want_cha, want_msg, sent=cw, k_info=pcd.ninfo)
        got_e = pcd.error_events(snr, seed, stream, f0, B, zero_codeword=zero)
        assert got_e.n_selected == want_e.n_selected and (got_e.positions == want_e.positions).all()
    assert pcd.decoder().describe()["node_channels"] == {"classes": 4, "nodes": np.bincount(cls, minlength=4).tolist()}
    pcd.set_node_channels(None)
    again = pcd.sample_labels(snr, seed, stream, f0, B, zero_codeword=False)
    assert all((a == b).all() for a, b in zip(plain, again)) and (plain[0] != cha).any()
    pcd.close()


# ---------------------------------------------------------------------------------------------------------------- ber_sim
def _cpp_run(params, base, tag):
    snr = (C.c_double * 8)()
    cnt = (C.c_int64 * 40)()
    n = lib.lutldpc_ber_sim_run(str(params).encode(), str(base).encode(), 0, tag, 0, 1, 1, snr, cnt, 8)
    assert n > 0, last_error()
    return list(snr[:n]), np.array(cnt[:n * 5]).reshape(n, 5)


def _frame_loop(ocd, snrs, tables_of, cls, nframes=300, nfers=20, K=250):
    """The sweep of ber_sim, frame by frame: reference labels -> oracle decode -> stop rule (more than nfers frame errors ends a point;
    a point without errors ends the sweep, the rest is padded with zeros)."""
    N = ocd.code.nvar
    out = np.zeros((len(snrs), 5), np.int64)
    for i, snr in enumerate(snrs):
        cha, msg, unc = nc.sample(tables_of(snr), cls, 0, i, 0, nframes, N, None)
        bits, _ = ocd.lut_decode_batch(cha, msg)
        be = bits[:, :K].sum(1)
        past = np.flatnonzero(np.cumsum(be > 0) > nfers)
        n = int(past[0]) + 1 if len(past) else nframes
        out[i] = [n, n * K, (be[:n] > 0).sum(), be[:n].sum(), unc[:n].sum()]
        if out[i][3] / out[i][1] < 1e-9 or out[i][2] / n < 1e-9:
            break
    return out


def test_ber_sim_with_the_channel_keys_equals_the_frame_loop(tmp_path):
    from lut_ldpc_amd import ber_sim
    ocd = oracle_codec("n500_q4_i8")
    ocd.set_initial_message_mode(0)
    ocd.set_exit_conditions(8, True, True)
    cls = nc.ber_classes()
    era, known = nc.erasure_table(ocd.qb_cha, ocd.qb_msg), nc.known_table(ocd.qb_cha, ocd.qb_msg)
    with_keys = lambda snr: [ocd.channel_cells(snr, 0.5), era, known, ocd.channel_cells(snr - 3.0, 0.5)]
    params, base = nc.write_ber_case(tmp_path)
    snr, got = _cpp_run(params, base, b"_cpp")
    assert snr == [3.0, 4.5]
    want = _frame_loop(ocd, snr, with_keys, cls)
    assert (got == want).all(), (got, want)
    assert want[:, 0].min() > 21 and (want[:, 2] > 0).all()                 # no point is over before the classes matter
    pts, path = ber_sim.run(params, base, seed=0, custom_name="_py", quiet=True)
    assert (np.array([c for _, c in pts]) == want).all()
    # the results file names the classes
    res = sorted((base / "results").rglob("*_cpp/*_rseed0000.it"))
    assert len(res) == 1
    it = itload(res[0])
    assert it["channel_node_classes"].tolist() == cls.tolist() and it["channel_class_snr_offset_dB"].tolist() == [0.0, -INF, INF, -3.0]
    assert itload(path)["channel_node_classes"].tolist() == cls.tolist()
    # the same file without the keys: one table on every node, no new field
    plain, _ = nc.write_ber_case(tmp_path, channel=False, name="ber_plain.ini")
    snr_p, got_p = _cpp_run(plain, base, b"_plain")
    want_p = _frame_loop(ocd, snr_p, lambda s: [ocd.channel_cells(s, 0.5)], np.zeros(500, np.uint8))
    assert (got_p == want_p).all() and (got_p != got).any()
    it = itload(sorted((base / "results").rglob("*_plain/*_rseed0000.it"))[0])
    assert "channel_node_classes" not in it and "channel_class_snr_offset_dB" not in it
