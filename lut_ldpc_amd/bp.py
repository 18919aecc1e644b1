"""Thin Python handle over the [BP] comparison decoder (include/lut_ldpc_bp.h): itpp::LDPC_Code::bp_decode for a batch of
frames on the MI355X.  PARITY UNPINNED against the reference's forked IT++ (absent); the header states the arithmetic."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import lib, check, last_error, BPCells, LutLdpcError, ERR_ARG

_vp = C.c_void_p


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class BPDecoder:
    """LLR_calc_unit(d1, d2, d3, d4) + LDPC_Code::bp_decode (src/LDPC_BER_Sim.cpp:199-200): defaults as the reference's
    [BP] section (qllr_scale_res 12, qllr_table_size 300, qllr_spacing_res 7, qllr_total_res 28)."""

    def __init__(self, nvar, nchk, dv, dc, cn_msg_idx, d1=12, d2=300, d3=7, d4=28, device=0):
        dv, dc, cn = (np.ascontiguousarray(a, np.int32) for a in (dv, dc, cn_msg_idx))
        self.nvar, self.nchk = int(nvar), int(nchk)
        self._h = _vp()
        check(lib.lutldpc_bp_create(self.nvar, self.nchk, _p(dv, C.c_int32), _p(dc, C.c_int32), _p(cn, C.c_int32), d1, d2, d3, d4, int(device), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            lib.lutldpc_bp_destroy(self._h)
            self._h = None

    __del__ = close

    def set_exit_conditions(self, max_iters, psc=True, pisc=False):
        check(lib.lutldpc_bp_set_exit_conditions(self._h, int(max_iters), int(psc), int(pisc)))

    def logexp_table(self) -> np.ndarray:
        n = lib.lutldpc_bp_logexp_table(self._h, None, 0)
        out = np.zeros(max(n, 1), np.int32)
        lib.lutldpc_bp_logexp_table(self._h, _p(out, C.c_int32), n)
        return out[:n]

    def _decode(self, fn, a, t, want_qllr):
        B, N = a.shape
        if N != self.nvar:
            raise ValueError("input must be [B, nvar]")
        bits, iters = np.empty((B, N), np.uint8), np.empty(B, np.int32)
        q = np.empty((B, N), np.int32) if want_qllr else None
        check(fn(self._h, _p(a, t), B, _p(bits, C.c_uint8), _p(iters, C.c_int32), _p(q, C.c_int32) if want_qllr else None))
        return (bits, iters, q) if want_qllr else (bits, iters)

    def decode_llr_batch(self, llr, want_qllr=False):
        return self._decode(lib.lutldpc_bp_decode_llr_batch, np.ascontiguousarray(llr, np.float64), C.c_double, want_qllr)

    def decode_qllr_batch(self, qllr, want_qllr=False):
        return self._decode(lib.lutldpc_bp_decode_qllr_batch, np.ascontiguousarray(qllr, np.int32), C.c_int32, want_qllr)

    # ---- device front end (include/lut_ldpc_bp.h): cell sampler -> bp_decode -> error counters, all on the device
    def set_cells(self, cells):
        """The channel's cell table: a dict {"thr", "qllr", "neg"} as awgn_cells returns it, or a _capi.BPCells."""
        c = cells if isinstance(cells, BPCells) else BPCells.from_table(cells)
        check(lib.lutldpc_bp_set_cells(self._h, C.byref(c)))

    @staticmethod
    def _codewords(codewords, B, N):
        if codewords is None:
            return None, None
        cw = np.ascontiguousarray(codewords, np.uint8)
        if cw.shape != (B, N):
            raise ValueError("codewords must be [B, nvar]")
        return cw, _p(cw, C.c_uint8)

    def sample_qllr(self, seed, stream, frame0, B, codewords=None):
        """What the sampler feeds the decoder for frames frame0 .. frame0+B-1: (qllr [B, nvar] int32, uncoded errors [B] int32)."""
        q, unc = np.empty((B, self.nvar), np.int32), np.empty(B, np.int32)
        cw, cwp = self._codewords(codewords, B, self.nvar)
        check(lib.lutldpc_bp_sample_qllr(self._h, int(seed), int(stream), int(frame0), int(B), cwp, _p(q, C.c_int32), _p(unc, C.c_int32)))
        return q, unc

    def sim_batch(self, seed, stream, frame0, B, K_info, codewords=None, want_qllr=False, want_bits=False):
        """{bp_decode return value, frame error, data bit errors over the first K_info nodes, uncoded errors} [B, 4] int32 of frames
        frame0 .. frame0+B-1 (sampler + decode + counters on the device); with want_qllr / want_bits a tuple (stats[, qllr][, bits])."""
        stats = np.empty((B, 4), np.int32)
        q = np.empty((B, self.nvar), np.int32) if want_qllr else None
        bits = np.empty((B, self.nvar), np.uint8) if want_bits else None
        cw, cwp = self._codewords(codewords, B, self.nvar)
        check(lib.lutldpc_bp_sim_batch(self._h, int(seed), int(stream), int(frame0), int(B), cwp, int(K_info), _p(stats, C.c_int32),
                                       _p(q, C.c_int32) if want_qllr else None, _p(bits, C.c_uint8) if want_bits else None))
        out = (stats,) + ((q,) if want_qllr else ()) + ((bits,) if want_bits else ())
        return out if len(out) > 1 else stats


def awgn_cells(N0, d1=12, d4=28):
    """The cell table of x ~ N(1, N0/2) for to_qllr(4x/N0) (lutldpc_bp_awgn_cells): {"thr": uint64[n - 1], "qllr": int32[n],
    "neg": uint8[n]}.  Host only."""
    n = C.c_int32(0)
    rc = lib.lutldpc_bp_awgn_cells(int(d1), int(d4), float(N0), 0, C.byref(n), None, None, None)      # the count: cap 0 is always short
    if rc != ERR_ARG or n.value < 1:
        raise LutLdpcError(rc, last_error())
    thr, q, neg = np.zeros(max(n.value - 1, 1), np.uint64), np.zeros(n.value, np.int32), np.zeros(n.value, np.uint8)
    check(lib.lutldpc_bp_awgn_cells(int(d1), int(d4), float(N0), n.value, C.byref(n), _p(thr, C.c_uint64), _p(q, C.c_int32), _p(neg, C.c_uint8)))
    return {"thr": thr[:n.value - 1], "qllr": q, "neg": neg}


def awgn_llr(seed, stream, frame0, B, N, N0, codewords=None):
    """The [BP] path's host front end (include/lut_ldpc_host.h: lutldpc_awgn_llr): (llr [B, N] float64, uncoded errors [B])."""
    llr, unc = np.empty((B, N), np.float64), np.empty(B, np.int32)
    cw = None if codewords is None else np.ascontiguousarray(codewords, np.uint8)
    check(lib.lutldpc_awgn_llr(int(seed), int(stream), int(frame0), int(B), int(N), float(N0), _p(cw, C.c_uint8) if cw is not None else None,
                               _p(llr, C.c_double), _p(unc, C.c_int32)))
    return llr, unc
