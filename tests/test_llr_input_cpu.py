"""The host half of lutldpc_decoder_decode_llr_packed, without a GPU: the cell table (lutldpc_llr_cell_table: thresholds rounded
down to the input type, cell -> label tables) against the oracle's quant_nonlin of the widened values, the argument errors of the
entry on a host-only handle, and the argument checks of Decoder.decode_llr.

cell(x) = #{j : x > thr[j]} is computed here with numpy IN THE INPUT TYPE (the comparison the kernel makes); the labels the tables
give for that cell must equal quant_nonlin(float64(x), boundaries) for every x tried: all 65536 float16 patterns, all 256 int8
values, the planted values of llr_cases.py for float32 / float64 -- with the designed boundaries and with an awkward list."""
import ctypes as C

import numpy as np
import pytest

import lut_ldpc_amd as L
from lut_ldpc_amd import _capi
from lut_ldpc_amd._capi import ERR_ARG, ERR_STATE, LlrIO, last_error, lib

import llr_cases as lc
from helpers import product_decoder

dp, i32p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
CODE = {"f64": _capi.LLR_F64, "f32": _capi.LLR_F32, "f16": _capi.LLR_F16, "i8": _capi.LLR_I8}


def make_io(dt, qc, qm=None, mp=None, scale=0.0, mode=None, stride=0, first=0, count=1, on_device=0):
    """An LlrIO and the arrays it points into (kept alive by the caller)."""
    qc = np.ascontiguousarray(qc, np.float64)
    qm = np.ascontiguousarray(qm, np.float64) if qm is not None else None
    mp = np.ascontiguousarray(mp, np.int32) if mp is not None else None
    io = LlrIO(CODE.get(dt, dt), on_device, stride, scale, qc.ctypes.data_as(dp), len(qc), qm.ctypes.data_as(dp) if qm is not None else None,
               len(qm) if qm is not None else 0, (0 if qm is not None else 1) if mode is None else mode, mp.ctypes.data_as(i32p) if mp is not None else None,
               first, count, 0)
    return io, (qc, qm, mp)


def cell_table(dt, nq_cha, nq_msg, qc, qm=None, mp=None, scale=0.0):
    io, keep = make_io(dt, qc, qm, mp, scale)
    thr = np.full(255, np.nan)
    n = C.c_int32(-1)
    lut_cha, lut_msg = np.zeros(256, np.uint8), np.zeros(256, np.uint8)
    rc = lib.lutldpc_llr_cell_table(C.byref(io), nq_cha, nq_msg, thr.ctypes.data_as(dp), 255, C.byref(n), lut_cha.ctypes.data_as(u8p), lut_msg.ctypes.data_as(u8p))
    assert rc == 0, last_error()
    return thr[:n.value], lut_cha, lut_msg


def check_table(dt, x, qc, qm, mp, mode, scale=None):
    """x: values of the dtype.  Cells in the input type -> labels through the tables == quant_nonlin of the widened values."""
    nq_cha, nq_msg = len(qc) + 1, len(qm) + 1
    thr, lut_cha, lut_msg = cell_table(dt, nq_cha, nq_msg, qc, qm if mode == 0 else None, mp if mode == 1 else None, scale or 0.0)
    if dt == "i8":
        assert len(thr) == 0
        cell = x.view(np.uint8).astype(np.int64)
        wide = x.astype(np.float64) * scale
    else:
        T = lc.DTYPES[dt]
        assert len(thr) <= 254 and (np.diff(thr) > 0).all() and not np.isnan(thr).any()
        thr_t = thr.astype(T)
        assert (thr_t.astype(np.float64) == thr).all()                      # values of the type
        both = np.concatenate([qc, qm]) if mode == 0 else np.asarray(qc)
        assert set(thr.tolist()) == set(lc.round_down(both, T).astype(np.float64).tolist())
        with np.errstate(invalid="ignore"):
            cell = (x[:, None] > thr_t[None, :]).sum(axis=1)
        wide = x.astype(np.float64)
    want_cha, want_msg = lc.ref_labels(wide, qc, qm, mp, mode)
    assert (lut_cha[cell] == want_cha).all(), (dt, mode, x[lut_cha[cell] != want_cha][:8])
    assert (lut_msg[cell] == want_msg).all(), (dt, mode, x[lut_msg[cell] != want_msg][:8])


def quantisers():
    """(id, qb_cha, qb_msg, map): the designed boundaries of the 16- and the 32-label code, and the awkward list."""
    out = []
    for name in ("nib_q4", "byte_q5"):
        out.append((name,) + lc.quantiser(name))
    out.append(("awkward", lc.AWKWARD, np.sort(lc.AWKWARD * 0.75 + 0.01), lc.AWKWARD_MAP))
    return out


def inputs(dt, qc, qm):
    if dt == "f16":
        return np.arange(65536, dtype=np.uint16).view(np.float16)
    return lc.planted((qc, qm), lc.DTYPES[dt])


@pytest.mark.parametrize("dt", ["f16", "f32", "f64"])
@pytest.mark.parametrize("mode", [0, 1])
def test_cell_table_of_the_float_types(dt, mode):
    for name, qc, qm, mp in quantisers():
        check_table(dt, inputs(dt, qc, qm), qc, qm, mp, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_cell_table_of_int8(mode):
    q = np.arange(-128, 128).astype(np.int8)
    for name, qc, qm, mp in quantisers():
        check_table("i8", q, qc, qm, mp, mode, scale=lc.i8_scale((qc, qm)))
    # products that land exactly on boundaries: x > b must stay strict
    qc = np.arange(-7, 8) * 0.5
    qm = np.arange(-7, 8) * 1.0
    check_table("i8", q, qc, qm, lc.AWKWARD_MAP, mode, scale=0.25)
    assert ((q * 0.25)[:, None] == qc[None, :]).any()


def test_cell_table_merges_boundaries_that_round_alike():
    thr, lut_cha, _ = cell_table("f32", 16, 16, lc.AWKWARD, None, lc.AWKWARD_MAP)
    assert len(thr) == 14                                                   # -1 - 2^-30 and -1 - 2^-31: one float32
    assert thr[0] == -np.inf and thr[-1] == np.inf and thr[-2] == float(np.finfo(np.float32).max)
    assert lut_cha[len(thr)] == 15 and lut_cha[0] == 0
    thr, _, _ = cell_table("f16", 16, 16, lc.AWKWARD, None, lc.AWKWARD_MAP)
    assert thr[0] == -np.inf and (thr == 65504.0).sum() == 1 and thr[-1] == np.inf


# ---- the entry's argument errors, on a host-only handle -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_handle():
    dec = product_decoder(lc.codec("nib_q4"), device=-1)
    yield dec
    dec.close()


def call(dec, io, llr, B=2, words=True, iters=True, cha=False, msg=False, handle=True):
    N = 1000
    w = np.zeros((2, 32), np.uint32)
    it = np.zeros(2, np.int32)
    a, b = np.zeros((2, N), np.uint8), np.zeros((2, N), np.uint8)
    vp = lambda x, on: C.c_void_p(x.ctypes.data) if on else None
    ptr = llr if llr is None or isinstance(llr, C.c_void_p) else C.c_void_p(llr.ctypes.data)
    return lib.lutldpc_decoder_decode_llr_packed(dec._h if handle else None, C.byref(io) if io is not None else None, ptr, B, vp(w, words), vp(it, iters),
                                                 vp(a, cha), vp(b, msg))


def test_argument_errors_come_before_the_state_error(host_handle):
    dec = host_handle
    qc, qm, mp = lc.quantiser("nib_q4")
    N = 1000
    x = {dt: np.zeros((2, N + 8), T) for dt, T in lc.DTYPES.items()}
    ok = dict(count=N)
    # valid arguments reach the handle: host-only -> ERR_STATE
    for dt in lc.DTYPES:
        for kw in (dict(qm=qm), dict(mp=mp), dict(qm=qm, stride=N + 8), dict(qm=qm, first=N - 33, count=33)):
            io, keep = make_io(dt, qc, scale=0.5, **{**ok, **kw})
            assert call(dec, io, x[dt]) == ERR_STATE and "host-only handle" in last_error(), (dt, kw, last_error())
    io, keep = make_io("f32", qc, qm=qm, count=-5)       # the window is not looked at without out_words; quantise only
    assert call(dec, io, x["f32"], words=False, iters=False, cha=True) == ERR_STATE
    # NULL handle and B <= 0 first, whatever else is wrong
    bad_io, keep2 = make_io(9, qc[:3])
    assert call(dec, bad_io, None, handle=False) == ERR_ARG and "NULL decoder" in last_error()
    assert call(dec, bad_io, None, B=0) == ERR_ARG and "B must be positive" in last_error()
    assert call(dec, bad_io, None, B=-3) == ERR_ARG and "B must be positive" in last_error()

    def refused(io, llr, text, **kw):
        assert call(dec, io, llr, **kw) == ERR_ARG, text
        assert text in last_error(), (text, last_error())

    io, keep = make_io("f32", qc, qm=qm, **ok)
    refused(None, x["f32"], "NULL argument")
    refused(io, None, "NULL argument")
    refused(make_io(4, qc, qm=qm, **ok)[0], x["f32"], "dtype")
    refused(make_io(-1, qc, qm=qm, **ok)[0], x["f32"], "dtype")
    for dt, size in (("f64", 8), ("f32", 4), ("f16", 2)):
        for off in range(1, size):
            refused(make_io(dt, qc, qm=qm, **ok)[0], C.c_void_p(x[dt].ctypes.data + off), "aligned")
    assert call(dec, make_io("i8", qc, qm=qm, scale=0.5, **ok)[0], C.c_void_p(x["i8"].ctypes.data + 1)) == ERR_STATE      # bytes have no alignment
    for stride in (N - 1, 1, -1, -N):
        refused(make_io("f32", qc, qm=qm, stride=stride, **ok)[0], x["f32"], "frame_stride")
    refused(make_io("f32", qc[:-1], qm=qm, **ok)[0], x["f32"], "qb_Cha")
    refused(make_io("f32", np.append(qc, 99.0), qm=qm, **ok)[0], x["f32"], "qb_Cha")
    refused(make_io("f32", qc, qm=qm[:-1], **ok)[0], x["f32"], "qb_Msg")
    for k in (0, 7, 14):
        b = qc.copy(); b[k] = np.nan
        refused(make_io("f32", b, qm=qm, **ok)[0], x["f32"], "qb_Cha must be non-decreasing")
        refused(make_io("f32", qc, qm=b, **ok)[0], x["f32"], "qb_Msg must be non-decreasing")
    b = qc.copy(); b[5], b[6] = qc[6], qc[5]
    refused(make_io("f32", b, qm=qm, **ok)[0], x["f32"], "qb_Cha must be non-decreasing")
    refused(make_io("f32", qc, qm=b, **ok)[0], x["f32"], "qb_Msg must be non-decreasing")
    b = qc.copy(); b[5] = b[6]                                # equal neighbours are non-decreasing
    assert call(dec, make_io("f32", b, qm=qm, **ok)[0], x["f32"]) == ERR_STATE
    # the modes
    refused(make_io("f32", qc, qm=qm, mode=2, **ok)[0], x["f32"], "initial_message_mode")
    refused(make_io("f32", qc, qm=qm, mode=-1, **ok)[0], x["f32"], "initial_message_mode")
    refused(make_io("f32", qc, mode=0, **ok)[0], x["f32"], "qb_Msg")
    refused(make_io("f32", qc, qm=qm, mp=mp, mode=0, **ok)[0], x["f32"], "cha2msg_map must be NULL")
    refused(make_io("f32", qc, qm=qm, mode=1, **ok)[0], x["f32"], "needs cha2msg_map")
    assert call(dec, make_io("f32", qc, qm=qm, mp=mp, mode=1, **ok)[0], x["f32"]) == ERR_STATE          # qb_Msg is not needed, not forbidden
    for v in (-1, 16, 255):
        m = mp.copy(); m[9] = v
        refused(make_io("f32", qc, mp=m, **ok)[0], x["f32"], "cha2msg_map entry")
    # the window, when words are asked for
    for first, count in ((-1, 5), (0, 0), (0, N + 1), (N, 1), (N - 32, 33), (2 ** 31 - 1, 2 ** 31 - 1)):
        refused(make_io("f32", qc, qm=qm, first=first, count=count)[0], x["f32"], "window")
    # the scale of int8
    for s in (0.0, -0.5, np.inf, np.nan):
        refused(make_io("i8", qc, qm=qm, scale=s, **ok)[0], x["i8"], "scale")
    assert call(dec, make_io("f32", qc, qm=qm, scale=np.nan, **ok)[0], x["f32"]) == ERR_STATE             # ignored for the float types
    refused(io, x["f32"], "no output", words=False, iters=False)


def test_cell_table_refuses_what_the_entry_refuses():
    qc, qm, mp = lc.quantiser("nib_q4")
    thr, n = np.zeros(255), C.c_int32()
    a, b = np.zeros(256, np.uint8), np.zeros(256, np.uint8)

    def rc(io, cap=255):
        return lib.lutldpc_llr_cell_table(C.byref(io), 16, 16, thr.ctypes.data_as(dp), cap, C.byref(n), a.ctypes.data_as(u8p), b.ctypes.data_as(u8p))

    qm = qc + 0.125                                          # (the design's two lists are equal: 15 thresholds; these give 30)
    assert rc(make_io("f32", qc, qm=qm)[0]) == 0 and n.value == 30
    assert rc(make_io("f32", qc, qm=qm)[0], cap=29) == ERR_ARG and "30 thresholds" in last_error()
    assert rc(make_io("f32", qc[::-1].copy(), qm=qm)[0]) == ERR_ARG
    assert rc(make_io("i8", qc, qm=qm, scale=0.0)[0]) == ERR_ARG
    assert rc(make_io(7, qc, qm=qm)[0]) == ERR_ARG
    assert rc(make_io("f32", qc, qm=qm, mp=mp, mode=0)[0]) == ERR_ARG


# ---- Decoder.decode_llr: refused before the library is called ------------------------------------------------------------------
def test_python_argument_checks(host_handle):
    dec = host_handle
    qc, qm, mp = lc.quantiser("nib_q4")
    N = 1000
    good = np.zeros((2, N), np.float32)
    for bad, text in ((np.zeros((2, N), np.int16), "float64, float32, float16 or int8"), (np.zeros((2, N), np.uint8), "float64, float32, float16 or int8"),
                      (np.zeros(N, np.float32), r"\[B, nvar\]"), (np.zeros((2, N + 1), np.float32), r"\[B, nvar\]"), (np.zeros((0, N), np.float32), r"\[B, nvar\]"),
                      ([[0.0] * N], "numpy array or a torch tensor")):
        with pytest.raises(ValueError, match=text):
            dec.decode_llr(bad, qc, qb_msg=qm)
    with pytest.raises(ValueError, match="scale"):
        dec.decode_llr(np.zeros((2, N), np.int8), qc, qb_msg=qm)
    with pytest.raises(ValueError, match="either qb_msg"):
        dec.decode_llr(good, qc)
    with pytest.raises(ValueError, match="either qb_msg"):
        dec.decode_llr(good, qc, qb_msg=qm, cha2msg_map=mp)
    with pytest.raises(ValueError, match="one entry per channel label"):
        dec.decode_llr(good, qc, cha2msg_map=mp[:-1])
    # what passes them reaches the library: a host-only handle
    with pytest.raises(L.LutLdpcError, match="host-only handle"):
        dec.decode_llr(good, qc, qb_msg=qm)
    with pytest.raises(L.LutLdpcError, match="host-only handle"):
        dec.decode_llr(np.zeros((2, N), np.int8), qc, cha2msg_map=mp, scale=0.25, decode=False)
