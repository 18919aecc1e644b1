"""The guard of the batch entries of the C-ABI without a GPU: all twelve go through one check (decoder_batch.hip: batch_entry), so
every one of them answers a NULL handle and B <= 0 with ERR_ARG -- on a host-only handle too: argument errors before state
errors -- and otherwise valid arguments on a host-only handle with ERR_STATE and the one message text.  The entry-specific
checks keep the places the older tests pin.  The six entries that take a Philox stream, and the lutldpc_codec_* wrappers over them,
refuse a stream >= 2^31 in that same guard: bit 31 separates the information-bit stream from the channel stream."""
import ctypes as C

import numpy as np
import pytest

from lut_ldpc_amd._capi import ERR_ARG, ERR_STATE, ChannelCells, EventRequest, last_error, lib

from helpers import oracle_codec, product_decoder

B0 = 3
u8p, i32p, i64p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def ctx():
    cd = oracle_codec("n500_q4_i8")               # rate0.50_dv02-17_dc08-09_lut_q4_N500, as tests/test_err_events_cpu.py
    dec = product_decoder(cd, device=-1)
    N, E, I = cd.code.nvar, cd.code.nedges, cd.max_iters
    a = dict(
        u8=np.zeros((B0, N), np.uint8), out=np.zeros((B0, N), np.uint8), it=np.zeros(B0, np.int32), stats=np.zeros((B0, 4), np.int32),
        llr=np.ones((B0, N), np.float64), qc=np.ascontiguousarray(cd.qb_cha, np.float64), qm=np.ascontiguousarray(cd.qb_msg, np.float64),
        trace=np.zeros((1 + 2 * I) * B0 * E, np.uint8), hist=np.zeros((1 + 2 * I, 1, 2, 16), np.int64),
        thr=np.array([1 << 63], np.uint64), lab=np.array([0, 1], np.uint8),
        ev=np.zeros((4, 8), np.int32), pos=np.zeros((4, 4), np.int32), chk=np.zeros((4, 4), np.int32))
    assert len(a["qc"]) == cd.nq_cha - 1 and len(a["qm"]) == cd.nq_msg[0] - 1
    p = {k: v.ctypes.data_as({np.uint8: u8p, np.int32: i32p, np.int64: i64p, np.float64: f64p, np.uint64: C.POINTER(C.c_uint64)}[v.dtype.type])
         for k, v in a.items()}
    cells = ChannelCells(2, p["thr"], p["lab"], p["lab"], p["lab"], p["lab"], p["lab"])
    yield dict(h=dec._h, N=N, I=I, p=p, cells=cells, keep=a)
    dec.close()


def _request(p, **kw):
    f = dict(select=0, max_frames=4, max_pos=4, max_chk=4, events=p["ev"], positions=p["pos"], checks=p["chk"])
    f.update(kw)
    return EventRequest(**f)


def _entries(c, stream=1):
    """name -> call(handle, B) with otherwise valid small arguments."""
    p, cells, N, I = c["p"], C.byref(c["cells"]), c["N"], c["I"]
    K, nh = N // 2, (1 + 2 * I) * 2 * 16
    rq = lambda: C.byref(_request(p))
    return {
        "decode_batch": lambda h, B: lib.lutldpc_decoder_decode_batch(h, p["u8"], p["u8"], B, p["out"], p["it"]),
        "decode_batch_device": lambda h, B: lib.lutldpc_decoder_decode_batch_device(h, p["u8"], p["u8"], B, p["out"], p["it"], 1),
        "decode_llr_batch": lambda h, B: lib.lutldpc_decoder_decode_llr_batch(h, p["llr"], B, p["qc"], 15, p["qm"], 15, 0, None, p["out"], p["it"]),
        "decode_batch_trace": lambda h, B: lib.lutldpc_decoder_decode_batch_trace(h, p["u8"], p["u8"], B, 3, p["out"], p["it"], p["trace"],
                                                                                  c["keep"]["trace"].size, None),
        "histogram_batch": lambda h, B: lib.lutldpc_decoder_histogram_batch(h, p["u8"], p["u8"], None, B, 3, 0, 16, None, None, p["hist"], nh, None),
        "sim_batch_histogram": lambda h, B: lib.lutldpc_decoder_sim_batch_histogram(h, cells, 7, stream, 0, B, None, 0, 3, 0, 16, p["hist"], nh, None),
        "events_batch": lambda h, B: lib.lutldpc_decoder_events_batch(h, p["u8"], p["u8"], None, B, K, None, None, rq()),
        "sim_batch_events": lambda h, B: lib.lutldpc_decoder_sim_batch_events(h, cells, 7, stream, 0, B, None, 0, K, p["stats"], rq()),
        "sim_batch": lambda h, B: lib.lutldpc_decoder_sim_batch(h, cells, 7, stream, 0, B, None, K, p["stats"], None, None),
        "sim_batch_random": lambda h, B: lib.lutldpc_decoder_sim_batch_random(h, cells, 7, stream, 0, B, K, p["stats"], None, None),
        "sample_labels": lambda h, B: lib.lutldpc_decoder_sample_labels(h, cells, 7, stream, 0, B, None, p["out"], p["out"]),
        "encode_random": lambda h, B: lib.lutldpc_decoder_encode_random(h, 7, stream, 0, B, p["out"]),
    }


NAMES = ["decode_batch", "decode_batch_device", "decode_llr_batch", "decode_batch_trace", "histogram_batch", "sim_batch_histogram", "events_batch",
         "sim_batch_events", "sim_batch", "sim_batch_random", "sample_labels", "encode_random"]


@pytest.mark.parametrize("name", NAMES)
def test_one_guard_for_every_batch_entry(name, ctx):
    call = _entries(ctx)[name]
    h = ctx["h"].value if isinstance(ctx["h"], C.c_void_p) else ctx["h"]
    assert call(None, B0) == ERR_ARG                                  # NULL handle
    for B in (0, -1):                                                 # host-only handle AND a bad batch size: the argument error wins
        assert call(h, B) == ERR_ARG, (name, B)
    assert call(h, B0) == ERR_STATE                                   # valid arguments: the handle has no device
    assert "host-only handle" in last_error()


STREAM_ENTRIES = ["sim_batch_histogram", "sim_batch_events", "sim_batch", "sim_batch_random", "sample_labels", "encode_random"]


@pytest.mark.parametrize("name", STREAM_ENTRIES)
def test_stream_with_bit_31_is_an_argument_error_in_the_shared_guard(name, ctx):
    h = ctx["h"].value if isinstance(ctx["h"], C.c_void_p) else ctx["h"]
    before = {k: v.copy() for k, v in ctx["keep"].items()}
    for stream in (2 ** 31, 2 ** 32 - 1):
        assert _entries(ctx, stream)[name](h, B0) == ERR_ARG, (name, stream)      # host-only handle: the argument error wins
        assert "bit 31 separates the information-bit stream from the channel stream" in last_error()
        assert _entries(ctx, stream)[name](None, B0) == ERR_ARG
    assert _entries(ctx, 2 ** 31 - 1)[name](h, B0) == ERR_STATE                  # the largest stream passes the guard
    assert "host-only handle" in last_error()
    assert all((before[k] == v).all() for k, v in ctx["keep"].items())
    assert lib.lutldpc_check_stream(2 ** 31 - 1) == 0 and lib.lutldpc_check_stream(0) == 0 and lib.lutldpc_check_stream(2 ** 31) == ERR_ARG


def test_codec_wrappers_refuse_a_stream_with_bit_31_before_they_write():
    """The lutldpc_codec_* wrappers make the cell table and the host codewords before they reach the decoder's entry: they ask the
    same check first, so nothing is computed or written (sample_labels would have filled `codewords` already)."""
    import lut_ldpc_amd as L
    from helpers import CODES
    pcd = L.Codec(CODES / "rate0.50_dv02-17_dc08-09_lut_q4_N500.alist", with_generator=True, device=-1)
    pcd.design_luts(sigma2=0.88 ** 2, max_iters=2)
    N, B = pcd.nvar, 3
    cha, msg, cw = (np.full((B, N), 0xEE, np.uint8) for _ in range(3))
    stats, hist, got = np.full((B, 4), -7, np.int32), np.full((5, 1, 2, 16), -7, np.int64), C.c_int32(-7)
    for stream in (2 ** 31, 2 ** 32 - 1):
        for zero in (1, 0):
            calls = {
                "sim_batch": lambda: lib.lutldpc_codec_sim_batch(pcd._h, 2.0, 7, stream, 0, B, zero, stats.ctypes.data_as(i32p)),
                "sample_labels": lambda: lib.lutldpc_codec_sample_labels(pcd._h, 2.0, 7, stream, 0, B, zero, cha.ctypes.data_as(u8p), msg.ctypes.data_as(u8p),
                                                                         cw.ctypes.data_as(u8p)),
                "encode_random": lambda: lib.lutldpc_codec_encode_random(pcd._h, 7, stream, 0, B, cw.ctypes.data_as(u8p)),
                "message_histogram": lambda: lib.lutldpc_codec_message_histogram(pcd._h, 2.0, 7, stream, 0, B, zero, 3, 0, 16, hist.ctypes.data_as(i64p),
                                                                                 hist.size, C.byref(got)),
            }
            for name, call in calls.items():
                assert call() == ERR_ARG, (name, stream, zero)
                assert "bit 31 separates" in last_error(), (name, last_error())
            with pytest.raises(L.LutLdpcError, match="bit 31 separates"):
                pcd.error_events(2.0, 7, stream, 0, B, zero_codeword=bool(zero))
    assert (cha == 0xEE).all() and (msg == 0xEE).all() and (cw == 0xEE).all() and (stats == -7).all() and (hist == -7).all() and got.value == -7
    with pytest.raises(L.LutLdpcError, match="host-only handle"):
        pcd.sim_batch(2.0, 7, 2 ** 31 - 1, 0, B)
    pcd.close()


def test_entry_specific_checks_keep_their_places(ctx):
    p, h, N = ctx["p"], ctx["h"], ctx["N"]
    h = h.value if isinstance(h, C.c_void_p) else h
    cells = C.byref(ctx["cells"])
    # the cells are looked at after the device: NULL cells on a host-only handle is a state error
    assert lib.lutldpc_decoder_sim_batch_random(h, None, 7, 1, 0, B0, N // 2, p["stats"], None, None) == ERR_STATE
    assert "host-only handle" in last_error()
    # NULL frame_stats and a malformed request are argument errors on any handle
    assert lib.lutldpc_decoder_sim_batch_events(h, cells, 7, 1, 0, B0, None, 0, N // 2, None, C.byref(_request(p))) == ERR_ARG
    for bad in (dict(events=None), dict(max_frames=-1), dict(select=4), dict(positions=None)):
        rq = _request(p, **bad)
        assert lib.lutldpc_decoder_sim_batch_events(h, cells, 7, 1, 0, B0, None, 0, N // 2, p["stats"], C.byref(rq)) == ERR_ARG, bad
        assert lib.lutldpc_decoder_events_batch(h, p["u8"], p["u8"], None, B0, N // 2, None, None, C.byref(rq)) == ERR_ARG, bad
        assert lib.lutldpc_decoder_events_batch(None, p["u8"], p["u8"], None, B0, N // 2, None, None, C.byref(rq)) == ERR_ARG, bad
    assert lib.lutldpc_decoder_events_batch(h, p["u8"], p["u8"], None, B0, N // 2, None, None, None) == ERR_ARG
