"""Failed-frame capture without a GPU: the argument errors of a host-only handle, the reference arrays of the test helper on a
hand-made case, and the derived curves of the command-line module on a three-frame example."""
import ctypes as C

import numpy as np
import pytest

import lut_ldpc_amd as L
from lut_ldpc_amd import err_events as ee
from lut_ldpc_amd._capi import ERR_ARG, ERR_STATE, EventRequest, lib

from events_helpers import expected, syndrome
from helpers import oracle_codec, product_decoder


def _code(fn):
    with pytest.raises(L.LutLdpcError) as e:
        fn()
    return e.value.code


def _request(**kw):
    ev, pos, chk = np.zeros((4, 8), np.int32), np.zeros((4, 4), np.int32), np.zeros((4, 4), np.int32)
    ip = C.POINTER(C.c_int32)
    f = dict(select=0, max_frames=4, max_pos=4, max_chk=4, events=ev.ctypes.data_as(ip), positions=pos.ctypes.data_as(ip), checks=chk.ctypes.data_as(ip))
    f.update(kw)
    r = EventRequest(**f)
    r._keep = (ev, pos, chk)
    return r


def test_argument_errors_on_a_host_only_handle():
    cd = oracle_codec("n500_q4_i8")
    dec = product_decoder(cd, device=-1)
    N = cd.code.nvar
    cha = np.zeros((3, N), np.uint8)
    u8 = cha.ctypes.data_as(C.POINTER(C.c_uint8))
    stats = np.zeros((3, 4), np.int32)
    sp = stats.ctypes.data_as(C.POINTER(C.c_int32))

    def batch(req, B=3, K=250):
        return lib.lutldpc_decoder_events_batch(dec._h, u8, u8, None, B, K, None, None, C.byref(req) if req is not None else None)

    def sim(req, B=3, K=250, device_codewords=0):
        return lib.lutldpc_decoder_sim_batch_events(dec._h, None, 7, 1, 0, B, None, device_codewords, K, sp, C.byref(req) if req is not None else None)

    for call in (batch, sim):
        assert call(None) == ERR_ARG                                          # NULL request
        assert call(_request(events=None)) == ERR_ARG                         # NULL events
        for k in ("max_frames", "max_pos", "max_chk"):
            assert call(_request(**{k: -1})) == ERR_ARG                       # negative sizes
        assert call(_request(select=-1)) == ERR_ARG and call(_request(select=4)) == ERR_ARG
        assert call(_request(positions=None)) == ERR_ARG and call(_request(checks=None)) == ERR_ARG     # NULL lists with a positive maximum
        assert call(_request(), B=0) == ERR_ARG and call(_request(), K=-1) == ERR_ARG and call(_request(), K=N + 1) == ERR_ARG
        assert "event" in L._capi.last_error() or "K_info" in L._capi.last_error()
        # well-formed calls need a device; NULL lists are fine when their maximum is 0
        assert call(_request()) == ERR_STATE
        assert call(_request(positions=None, checks=None, max_pos=0, max_chk=0)) == ERR_STATE
        for s in range(4):
            assert call(_request(select=s)) == ERR_STATE
    assert sim(_request(), device_codewords=1) == ERR_STATE
    assert lib.lutldpc_decoder_events_batch(dec._h, None, u8, None, 3, 250, None, None, C.byref(_request())) == ERR_ARG
    assert lib.lutldpc_decoder_sim_batch_events(dec._h, None, 7, 1, 0, 3, None, 0, 250, None, C.byref(_request())) == ERR_ARG
    # the Python layer: the same codes as exceptions, its own checks as ValueError
    assert _code(lambda: dec.error_events(cha, cha, max_pos=-1)) == ERR_ARG
    assert _code(lambda: dec.error_events(cha, cha, select=7)) == ERR_ARG
    assert _code(lambda: dec.error_events(cha, cha)) == ERR_STATE
    assert _code(lambda: dec.error_events(cha, cha, sent=cha, select="undetected", profiles=True)) == ERR_STATE
    with pytest.raises(KeyError):
        dec.error_events(cha, cha, select="parity")
    with pytest.raises(ValueError):
        dec.error_events(cha, cha, sent=cha[:2])
    with pytest.raises(ValueError):
        dec.error_events(cha, cha, profiles=(np.zeros(N, np.int32), np.zeros(cd.code.nchk, np.int64)))
    dec.close()


def test_the_helper_on_a_hand_made_code():
    """Three checks over five nodes: c0 = {0, 1, 2}, c1 = {2, 3}, c2 = {0, 3, 4}; K = 2."""
    dv, dc = np.array([2, 1, 2, 2, 1]), np.array([3, 2, 3])
    # VN-major edge ids: node 0 -> 0, 1; node 1 -> 2; node 2 -> 3, 4; node 3 -> 5, 6; node 4 -> 7
    cn = np.array([0, 2, 3, 4, 5, 1, 6, 7])
    bits = np.array([[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 1, 1, 0], [1, 1, 1, 1, 1]], np.uint8)
    assert syndrome(bits, dv, dc, cn).tolist() == [[0, 0, 0], [1, 0, 1], [1, 0, 1], [1, 0, 1]]
    it = np.array([3, -8, 8, -8])
    ev, pos, chk, n, node, check = expected(bits, None, it, (dv, dc, cn), 2, "codeword", 2, 2, 1)
    assert n == 3 and ev.tolist() == [[1, -8, 1, 1, 2, 0, 1, 1], [2, 8, 2, 0, 2, 0, 2, 1]]
    assert pos.tolist() == [[0, -1], [2, 3]] and chk.tolist() == [[0], [0]]
    assert node.tolist() == [2, 1, 2, 2, 1] and check.tolist() == [3, 0, 3]
    assert expected(bits, None, it, (dv, dc, cn), 2, "info", 9, 2, 1)[0][:, 0].tolist() == [1, 3]
    assert expected(bits, None, it, (dv, dc, cn), 2, "failed", 9, 2, 1)[0][:, 0].tolist() == [1, 3]
    assert expected(bits, None, it, (dv, dc, cn), 2, "undetected", 9, 2, 1)[0][:, 0].tolist() == [2]
    sent = bits.copy()
    sent[3, 4] = 0
    assert expected(bits, sent, it, (dv, dc, cn), 2, "codeword", 9, 5, 3)[1].tolist() == [[4, -1, -1, -1, -1]]


def test_derived_curves_of_a_three_frame_example():
    """Three frames over a code with node degrees (2, 2, 3, 3, 3, 6) and check degrees (4, 4, 5): frame 0 is clean, frame 1 has
    nodes 0 and 2 wrong, frame 2 nodes 2, 3 and 5; checks 0 / 0 and 2 unsatisfied."""
    dv, dc = np.array([2, 2, 3, 3, 3, 6]), np.array([4, 4, 5])
    node_errors, check_fails = np.array([1, 0, 2, 1, 0, 1], np.int64), np.array([2, 0, 1], np.int64)
    events = np.array([[1, -8, 2, 1, 1, 7, 2, 1], [2, -8, 3, 2, 2, 9, 3, 2]], np.int64)
    d = ee.derive(events, node_errors, check_fails, dv, dc, 3)
    assert d["vn_degrees"].tolist() == [2, 3, 6] and d["cn_degrees"].tolist() == [4, 5]
    assert d["vn_error_rate"] == pytest.approx([1 / 6, 3 / 9, 1 / 3], abs=1e-15)          # wrong (node, frame) pairs / (nodes of the degree x frames)
    assert d["cn_fail_rate"] == pytest.approx([2 / 6, 1 / 3], abs=1e-15)
    assert d["cw_error_histogram"].tolist() == [0, 0, 1, 1]
    assert ee.weight_histogram(np.zeros((0, 8), np.int64)).tolist() == [0]
    deg, rate = ee.degree_rates(np.zeros(6, np.int64), dv, 0)
    assert deg.tolist() == [2, 3, 6] and rate.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        ee.degree_rates(node_errors[:5], dv, 3)
    assert ee.SELECT == {"codeword": 0, "info": 1, "failed": 2, "undetected": 3} and len(ee.COLUMNS) == 8
