"""The Monte-Carlo front end on the device against the numpy references of tests/frontend_cases.py, through the C-ABI: the Philox cell
sampler on crafted cell tables (samples that tie thresholds, a slice of the bucket index holding all 71 thresholds, thresholds on
slice ends, at 0 and 2^64 - 1, empty cells, one and two cells), on odd N, fewer pairs than one workgroup covers, both row formats and
frame ranges that carry into the high index word or wrap at 2^64; the error counters at the edges of K_info; the device encoder at
the edges of K and R with generator words that carry bits beyond K; the refusal of streams with bit 31 set.  All integer, all equal
bit for bit.  (tests/test_frontend_exact_cpu.py holds the references themselves to published vectors and to their conditions.)"""
import ctypes as C
import os

import numpy as np
import pytest

import frontend_cases as fc
from lut_ldpc_amd._capi import ERR_ARG, ERR_UNSUPPORTED, ChannelCells, EventRequest, LutLdpcError, last_error, lib
from helpers import product_decoder, same as _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles():
    """handle name of frontend_cases.HANDLES -> device decoder, created on first use (its knobs are read at creation) and kept."""
    made = {}

    def get(name):
        if name not in made:
            code, env, T = fc.HANDLES[name]
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


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _sample(dec, table, seed, stream, f0, B, cw):
    return dec.sample_labels(table, seed, stream, f0, B, codewords=cw, cha=np.full((B, dec.nvar), 0xEE, np.uint8), msg=np.full((B, dec.nvar), 0xEE, np.uint8))


def _sim(dec, table, seed, stream, f0, B, cw, K, random=False):
    """(frame_stats, cha_out, bits_out) of sim_batch on host codewords (or none), or of sim_batch_random."""
    return dec.sim_batch(table, seed, stream, f0, B, K, codewords=cw, random=random, frame_stats=np.full((B, 4), -7, np.int32),
                         cha_out=np.full((B, dec.nvar), 0xEE, np.uint8), bits_out=np.full((B, dec.nvar), 0xEE, np.uint8))


@pytest.mark.parametrize("case", fc.SAMPLER_CASES, ids=fc.case_id)
def test_sampler_equals_the_reference_label_for_label(case, handles):
    handle, table, _, f0, seed, stream = case
    cells, u, N, B, T, cw01, cw_bytes = fc.sampler_case(case)
    dec = handles(handle)
    assert dec.nvar == N
    for name, cw in (("zero codeword", None), ("random codewords", cw01), ("codewords of random bytes", cw_bytes)):
        want_cha, want_msg, _ = fc.sample(cells, seed, stream, f0, B, N, cw, u=u)
        cha, msg = _sample(dec, cells, seed, stream, f0, B, cw)
        _same(cha, want_cha, name + ": channel labels", u)
        _same(msg, want_msg, name + ": message labels", u)
    # bit 0 of a byte is what counts
    cha1, msg1 = _sample(dec, cells, seed, stream, f0, B, cw_bytes & 1)
    assert (cha1 == cha).all() and (msg1 == msg).all()
    # the slicer column of the table (irregular in the crafted ones) through sim_batch: uncoded errors and the sampled labels
    want_cha, _, want_unc = fc.sample(cells, seed, stream, f0, B, N, cw_bytes, u=u)
    stats, cha_out, _ = _sim(dec, cells, seed, stream, f0, B, cw_bytes, N // 2)
    _same(cha_out, want_cha, "sim_batch: channel labels", u)
    assert (stats[:, 3] == want_unc).all(), np.flatnonzero(stats[:, 3] != want_unc)[:8]


@pytest.mark.parametrize("bk", fc.STATS_B)
@pytest.mark.parametrize("handle,Ks", fc.STATS_CASES, ids=[c[0] for c in fc.STATS_CASES])
def test_stats_row_at_the_edges_of_k_info(handle, Ks, bk, handles):
    """sim_batch with random bytes as "codewords" (every third frame even bytes: the all-zero codeword), on the code's own table:
    column 3 from sample(), column 0 from lut_decode_batch of the reference's labels on the same handle and from the oracle on 24
    frames, columns 1 and 2 from bits_out and the sent bits in numpy."""
    ref = fc.stats_reference(handle, bk)
    dec, cd, N, B, cw = handles(handle), ref["cd"], ref["N"], ref["B"], ref["cw"]
    dec.set_exit_conditions(cd.max_iters, True, True)
    bits, iters = dec.lut_decode_batch(ref["cha"], ref["msg"])
    assert (iters[ref["pick"]] == ref["iters"]).all() and (bits[ref["pick"]] == ref["bits"]).all()
    assert len(set(iters.tolist())) > 3 and (iters < 0).any()
    for K in Ks:
        stats, cha_out, bits_out = _sim(dec, ref["cells"], fc.STATS_SEED, fc.STATS_STREAM, fc.STATS_F0, B, cw, K)
        _same(cha_out, ref["cha"], f"K_info {K}: channel labels")
        _same(bits_out, bits, f"K_info {K}: decided bits")
        err = (bits_out[:, :K] ^ (cw[:, :K] & 1)).sum(1)
        if 0 < K:
            assert (err > 0).any() and (err == 0).any(), K
        want = np.stack([iters, err > 0, err, ref["unc"]], axis=1).astype(np.int32)
        bad = np.argwhere(stats != want)
        assert bad.size == 0, (K, len(bad), bad[:6].tolist(), stats[bad[0][0]], want[bad[0][0]])


def _set_generator(dec, K, R):
    dec.set_generator(K, R, fc.generator_rows(K, R))


def _encode(dec, seed, stream, f0, B):
    return dec.encode_random(seed, stream, f0, B, out=np.full((B, dec.nvar), 0xEE, np.uint8))


@pytest.mark.parametrize("handle,K,R", fc.GENERATOR_CASES, ids=[f"{h}-K{K}-R{R}" for h, K, R in fc.GENERATOR_CASES])
def test_encoder_equals_the_reference_at_the_edges_of_k_and_r(handle, K, R, handles):
    dec = handles(handle)
    T = fc.HANDLES[handle][2]
    _set_generator(dec, K, R)                                   # (replaces the generator of the case before on this live handle)
    assert dec.describe()["generator"] == {"K": K, "R": R}
    sizes = [fc.gen_batch(b, T) for b in fc.GEN_B]
    want = fc.generator_reference(K, R, max(sizes))
    assert want.shape == (max(sizes), K + R) and want[:, :K].any() and (R == 0 or want[:, K:].any())
    for B in sizes:
        got = _encode(dec, fc.GEN_SEED, fc.GEN_STREAM, fc.GEN_F0, B)
        _same(got[:, :K], want[:B, :K], f"B {B}: information bits")
        _same(got[:, K:], want[:B, K:], f"B {B}: parity bits")
    # a split of the batch equals the whole
    B, h = max(sizes), max(sizes) // 3
    two = np.concatenate([_encode(dec, fc.GEN_SEED, fc.GEN_STREAM, fc.GEN_F0, h), _encode(dec, fc.GEN_SEED, fc.GEN_STREAM, fc.GEN_F0 + h, B - h)])
    assert (two == want).all()
    # sim_batch_random on this handle = sim_batch fed those codewords as host bytes (the code's own table; K data bits)
    cd = fc.codec(fc.HANDLES[handle][0])
    cells = cd.channel_cells(fc.STATS_SNR, cd.rate)
    for Bs in (65, B):
        rnd = _sim(dec, cells, fc.GEN_SEED, fc.GEN_STREAM, fc.GEN_F0, Bs, None, K, random=True)
        host = _sim(dec, cells, fc.GEN_SEED, fc.GEN_STREAM, fc.GEN_F0, Bs, want[:Bs], K)
        for a, b, what in zip(rnd, host, ("frame_stats", "channel labels", "decided bits")):
            assert (a == b).all(), (Bs, what, np.argwhere(a != b)[:4].tolist())
        want_cha, _, want_unc = fc.sample(cells, fc.GEN_SEED, fc.GEN_STREAM, fc.GEN_F0, Bs, K + R, want[:Bs])
        assert (rnd[1] == want_cha).all() and (rnd[0][:, 3] == want_unc).all()


def test_generator_replaced_on_a_live_handle_takes_effect_and_a_refused_one_changes_nothing(handles):
    dec = handles("q4")
    out = {}
    for K in (33, 500, 33):
        _set_generator(dec, K, 1000 - K)
        cw = _encode(dec, fc.GEN_SEED, 7, fc.GEN_F0, 65)
        assert (cw == fc.encode(fc.generator_bits(fc.generator_rows(K, 1000 - K), K), fc.info_bits(fc.GEN_SEED, 7, fc.GEN_F0, 65, K))).all(), K
        assert K not in out or (out[K] == cw).all()
        out[K] = cw
    assert (out[33] != out[500]).any()
    big = handles("n10000")
    _set_generator(big, 8192, 1808)
    before = _encode(big, fc.GEN_SEED, 7, fc.GEN_F0, 3)
    h, K, R = fc.GENERATOR_REFUSED
    assert h == "n10000"
    with pytest.raises(LutLdpcError, match="8192") as refused:
        _set_generator(big, K, R)
    assert refused.value.code == ERR_UNSUPPORTED
    assert big.describe()["generator"] == {"K": 8192, "R": 1808}
    assert (_encode(big, fc.GEN_SEED, 7, fc.GEN_F0, 3) == before).all()


def test_stream_with_bit_31_is_refused_and_nothing_is_written(handles):
    """Counter word 3 is `stream` for the channel and `stream | 0x80000000` for the information bits: every entry that takes a stream
    answers one with bit 31 set with ERR_ARG and leaves its outputs alone; 2^31 - 1 is the largest stream and works."""
    dec = handles("q4")
    N, B, K = dec.nvar, 65, 500
    _set_generator(dec, K, N - K)
    cd = fc.codec("reg36_n1000_q4")
    table = cd.channel_cells(fc.STATS_SNR, cd.rate)
    cells = ChannelCells.from_table(table)
    nd, groups, labels, _ = dec.histogram_shape(3)
    for stream in (2 ** 31, 2 ** 32 - 1):
        cha, msg, bits, cw = (np.full((B, N), 0xEE, np.uint8) for _ in range(4))
        stats, hist, got = np.full((B, 4), -7, np.int32), np.full((nd, groups, 2, labels), -7, np.int64), C.c_int32(-7)
        ev, pos, chk = np.full((4, 8), -7, np.int32), np.full((4, 4), -7, np.int32), np.full((4, 4), -7, np.int32)
        rq = EventRequest(select=0, max_frames=4, max_pos=4, max_chk=4, events=_p(ev, C.c_int32), positions=_p(pos, C.c_int32), checks=_p(chk, C.c_int32))
        sent = np.ones((B, N), np.uint8)
        calls = {
            "sim_batch": lambda: lib.lutldpc_decoder_sim_batch(dec._h, C.byref(cells), 7, stream, 0, B, _p(sent, C.c_uint8), K, _p(stats, C.c_int32),
                                                               _p(cha, C.c_uint8), _p(bits, C.c_uint8)),
            "sim_batch_random": lambda: lib.lutldpc_decoder_sim_batch_random(dec._h, C.byref(cells), 7, stream, 0, B, K, _p(stats, C.c_int32), _p(cha, C.c_uint8),
                                                                             _p(bits, C.c_uint8)),
            "sample_labels": lambda: lib.lutldpc_decoder_sample_labels(dec._h, C.byref(cells), 7, stream, 0, B, None, _p(cha, C.c_uint8), _p(msg, C.c_uint8)),
            "encode_random": lambda: lib.lutldpc_decoder_encode_random(dec._h, 7, stream, 0, B, _p(cw, C.c_uint8)),
            "sim_batch_histogram": lambda: lib.lutldpc_decoder_sim_batch_histogram(dec._h, C.byref(cells), 7, stream, 0, B, None, 1, 3, 0, labels, _p(hist, C.c_int64),
                                                                                   hist.size, C.byref(got)),
            "sim_batch_events": lambda: lib.lutldpc_decoder_sim_batch_events(dec._h, C.byref(cells), 7, stream, 0, B, None, 1, K, _p(stats, C.c_int32), C.byref(rq)),
        }
        for name, call in calls.items():
            assert call() == ERR_ARG, (name, stream)
            assert "bit 31 separates the information-bit stream from the channel stream" in last_error(), (name, last_error())
        for a in (cha, msg, bits, cw):
            assert (a == 0xEE).all()
        for a in (stats, hist, ev, pos, chk):
            assert (a == -7).all()
        assert got.value == -7 and rq.n_selected == 0 and rq.n_stored == 0
    # the largest stream: sampler and encoder equal the references (the cases above run it on crafted tables and every generator)
    s = fc.STREAM_MAX
    assert fc.GEN_STREAM == s and any(c[5] == s for c in fc.SAMPLER_CASES)
    want = fc.encode(fc.generator_bits(fc.generator_rows(K, N - K), K), fc.info_bits(7, s, fc.F_CARRY, B, K))
    assert (_encode(dec, 7, s, fc.F_CARRY, B) == want).all()
    want_cha, want_msg, want_unc = fc.sample(table, 7, s, fc.F_CARRY, B, N, want)
    stats, cha, _ = _sim(dec, table, 7, s, fc.F_CARRY, B, None, K, random=True)
    assert (cha == want_cha).all() and (stats[:, 3] == want_unc).all()
    cha, msg = _sample(dec, table, 7, s, fc.F_CARRY, B, want.astype(np.uint8))
    assert (cha == want_cha).all() and (msg == want_msg).all()
