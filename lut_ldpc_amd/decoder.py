"""Thin Python handle over the HIP decoder C-ABI (include/lut_ldpc_hip.h).

`Decoder` corresponds to the decode half of the reference's LDPC_Code_LUT
(src/LDPC_Code_LUT.hpp:66-366): graph index arrays + LUT trees in, `lut_decode` /
`decode(llr)` for a batch of frames out.  All arithmetic runs in the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np

from . import _capi
from ._capi import lib, check


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _opt(a, t):
    return _p(a, t) if a is not None else None


def _out(a, rows, width, dtype, what):
    """An output [rows, width] of a batch entry: a new array for None, or the caller's own (C-contiguous, `rows` rows or more)."""
    if a is None:
        return np.empty((rows, width), dtype)
    if not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags.c_contiguous or a.ndim != 2 or a.shape[0] < rows or a.shape[1] != width:
        raise ValueError(f"{what} must be a C-contiguous {np.dtype(dtype).name} array of at least {(rows, width)}")
    return a


def _cells(cells):
    """The `cells` argument of a sampling entry: a reference to the caller's table, or None (NULL: the node channels of the handle)."""
    if cells is None:
        return None
    return C.byref(cells if isinstance(cells, _capi.ChannelCells) else _capi.ChannelCells.from_table(cells))


class _Side:
    """Where the [B, width] input of a packed entry lives -- a numpy array in host memory or a torch tensor on the device -- with its
    row stride and pointer, and the outputs allocated on the same side."""

    def __init__(self, x):
        self.on_device = not isinstance(x, np.ndarray) and hasattr(x, "data_ptr")

    def place(self, x, width, at_least):
        """Row stride of x (a tensor is read in place, its current stream synchronised first; an array is made contiguous)."""
        B = int(x.shape[0])
        if self.on_device:
            import torch
            if x.stride(1) != 1 or (B > 1 and x.stride(0) < width):
                raise ValueError("a tensor needs a contiguous last dimension and a row stride of at least " + at_least)
            self.src, self.stride, self.dev = x, int(x.stride(0)) if B > 1 else width, x.device
            torch.cuda.current_stream(self.dev).synchronize()
        else:
            self.src, self.stride = np.ascontiguousarray(x), width

    def empty(self, shape, dtype, want=True):
        """uint8 / int32 / uint32 (a tensor of words is int32: the same 32 bits)"""
        if not want:
            return None
        if self.on_device:
            import torch
            return torch.empty(shape, dtype=torch.uint8 if dtype == np.uint8 else torch.int32, device=self.dev)
        return np.empty(shape, dtype)

    def ptr(self, a):
        if a is None:
            return None
        return C.c_void_p(a.data_ptr() if self.on_device else a.ctypes.data)


MODES = {"all": 0, "active": 1}      # counting modes of the message histograms (include/lut_ldpc_hip.h)


class Decoder:
    def __init__(self, nvar, nchk, dv, dc, cn_msg_idx, nq_cha, nq_msg, reuse_vec, max_iters, min_lut,
                 var_trees_txt, chk_trees_txt="", device=0):
        self.nvar, self.nchk = int(nvar), int(nchk)
        self.max_iters = int(max_iters)
        dv, dc, cn = _i32(dv), _i32(dc), _i32(cn_msg_idx)
        nq, ru = _i32(nq_msg), np.ascontiguousarray(reuse_vec, np.uint8)
        assert len(nq) == max_iters and len(ru) == max_iters
        self._h = C.c_void_p()
        self._owned = True
        check(lib.lutldpc_decoder_create(self.nvar, self.nchk, _p(dv, C.c_int32), _p(dc, C.c_int32), _p(cn, C.c_int32),
                                         int(nq_cha), _p(nq, C.c_int32), _p(ru, C.c_uint8), self.max_iters, int(bool(min_lut)),
                                         var_trees_txt.encode(), (chk_trees_txt or "").encode(), int(device),
                                         C.byref(self._h)))
        self.device = device

    def close(self):
        if getattr(self, "_h", None) and getattr(self, "_owned", False):
            lib.lutldpc_decoder_destroy(self._h)
        self._h = None

    def __del__(self):
        self.close()

    def set_exit_conditions(self, max_iters, psc=True, pisc=False):
        check(lib.lutldpc_decoder_set_exit_conditions(self._h, int(max_iters), int(psc), int(pisc)))
        self.max_iters = int(max_iters)

    # ---- host buffers ---------------------------------------------------------------------
    def _label_rows(self, cha, msg0, sent=None):
        """cha, msg0 and the optional sent bits as C-contiguous uint8 [B, nvar]: (cha, msg0, sent, B, nvar)."""
        cha = np.ascontiguousarray(cha, np.uint8)
        msg0 = np.ascontiguousarray(msg0, np.uint8)
        B, N = cha.shape
        if N != self.nvar or msg0.shape != cha.shape:
            raise ValueError("cha/msg0 must be [B, nvar]")
        if sent is not None:
            sent = np.ascontiguousarray(sent, np.uint8)
            if sent.shape != cha.shape:
                raise ValueError("sent must be [B, nvar]")
        return cha, msg0, sent, B, N

    def lut_decode_batch(self, cha: np.ndarray, msg0: np.ndarray):
        cha, msg0, _, B, N = self._label_rows(cha, msg0)
        out = np.empty((B, N), np.uint8)
        iters = np.empty(B, np.int32)
        check(lib.lutldpc_decoder_decode_batch(self._h, _p(cha, C.c_uint8), _p(msg0, C.c_uint8), B, _p(out, C.c_uint8),
                                               _p(iters, C.c_int32)))
        return out, iters

    def decode_packed(self, cha, msg0=None, cha2msg_map=None, nibbles=False, first=0, count=None):
        """lut_decode_batch with less on the host link (lutldpc_decoder_decode_batch_packed): cha / msg0 are [B, nvar] labels, or with
        nibbles=True [B, ceil(nvar/2)] bytes as packing.pack_nibbles makes them; cha2msg_map (Nq_Cha entries) in place of msg0
        derives the initial messages from the channel labels on the device.  Returns (words uint32 [B, ceil(count/32)], iters): the
        decided bits first .. first+count-1 of every frame, one bit each (packing.unpack_bits); count=None: up to nvar."""
        cha = np.ascontiguousarray(cha, np.uint8)
        stride = (self.nvar + 1) // 2 if nibbles else self.nvar
        if cha.ndim != 2 or cha.shape[1] != stride:
            raise ValueError("cha must be [B, ceil(nvar/2)] packed bytes" if nibbles else "cha must be [B, nvar]")
        B = cha.shape[0]
        if msg0 is not None:
            msg0 = np.ascontiguousarray(msg0, np.uint8)
            if msg0.shape != cha.shape:
                raise ValueError("msg0 must have the shape and format of cha")
        mp = _i32(cha2msg_map) if cha2msg_map is not None else None
        count = self.nvar - int(first) if count is None else int(count)
        io = _capi.PackedIO(_capi.IN_NIBBLES if nibbles else _capi.IN_BYTES, _p(mp, C.c_int32) if mp is not None else None, int(first), count)
        words = np.empty((B, max((count + 31) // 32, 0)), np.uint32)
        iters = np.empty(B, np.int32)
        check(lib.lutldpc_decoder_decode_batch_packed(self._h, C.byref(io), _p(cha, C.c_uint8), _p(msg0, C.c_uint8) if msg0 is not None else None, B,
                                                      _p(words, C.c_uint32), _p(iters, C.c_int32)))
        return words, iters

    def lut_decode_batch_trace(self, cha, msg0, level, n_edges):
        """Debug path: (bits, iters, trace uint8 [n_dumps, B, E]) -- the edge messages after the initialisation, (level 3) every
        check pass and every variable pass, in the print order of output_verbosity = level (src/LDPC_Code_LUT.cpp:292-337)."""
        cha = np.ascontiguousarray(cha, np.uint8); msg0 = np.ascontiguousarray(msg0, np.uint8)
        B, N = cha.shape
        n_dumps = 1 + self.max_iters * (int(level) - 1)
        out = np.empty((B, N), np.uint8); iters = np.empty(B, np.int32)
        trace = np.empty((n_dumps, B, int(n_edges)), np.uint8)
        got = C.c_int32()
        check(lib.lutldpc_decoder_decode_batch_trace(self._h, _p(cha, C.c_uint8), _p(msg0, C.c_uint8), B, int(level), _p(out, C.c_uint8), _p(iters, C.c_int32),
                                                     _p(trace, C.c_uint8), trace.size, C.byref(got)))
        assert got.value == n_dumps
        return out, iters, trace

    # ---- message-label histograms (lut_ldpc_amd/msg_stats.py works on their result) ------------------------
    def set_edge_groups(self, edge_group=None, n_groups=1):
        """Grouping of the histograms: edge_group[E] (VN-major edge order) with values in [0, n_groups), or None for one group."""
        if edge_group is None:
            check(lib.lutldpc_decoder_set_edge_groups(self._h, None, int(n_groups)))
        else:
            eg = _i32(edge_group)
            if eg.shape != (self.histogram_shape(2)[3],):
                raise ValueError("edge_group must hold one entry per edge")
            check(lib.lutldpc_decoder_set_edge_groups(self._h, _p(eg, C.c_int32), int(n_groups)))

    def histogram_shape(self, level=3):
        """(n_dumps of `level`, n_groups, largest message alphabet, edges)"""
        out = (C.c_int32 * 4)()
        check(lib.lutldpc_decoder_histogram_shape(self._h, int(level), out))
        return tuple(out)

    def new_histogram(self, level=3, n_labels=None) -> np.ndarray:
        n_dumps, n_groups, nq, _ = self.histogram_shape(level)
        return np.zeros((n_dumps, n_groups, 2, int(n_labels or nq)), np.int64)

    def _hist(self, hist, level, n_labels):
        hist = self.new_histogram(level, n_labels) if hist is None else hist
        if hist.dtype != np.int64 or not hist.flags.c_contiguous or hist.ndim != 4:
            raise ValueError("hist must be a C-contiguous int64 array [dump, group, 2, label]")
        return hist

    def message_histogram(self, cha, msg0, sent=None, level=3, mode="all", n_labels=None, hist=None, decode=True):
        """Counts the edge-message labels of every dump of output_verbosity = level on the device: hist[dump, group, sent bit, label]
        (int64), ADDED into `hist` when given.  mode "all": every frame at every dump (exit tests off); "active": the dumps the
        reference would have printed under the decoder's exit conditions.  sent: [B, nvar] sent bits or None (all-zero codeword).
        Returns (hist, bits, iters) with decode=True (the decode of the same call), else hist alone."""
        cha, msg0, sent, B, N = self._label_rows(cha, msg0, sent)
        hist = self._hist(hist, level, n_labels)
        bits = np.empty((B, N), np.uint8) if decode else None
        iters = np.empty(B, np.int32) if decode else None
        got = C.c_int32()
        check(lib.lutldpc_decoder_histogram_batch(self._h, _p(cha, C.c_uint8), _p(msg0, C.c_uint8), _opt(sent, C.c_uint8), B,
                                                  int(level), MODES[mode] if isinstance(mode, str) else int(mode), hist.shape[3],
                                                  _opt(bits, C.c_uint8), _opt(iters, C.c_int32), _p(hist, C.c_int64), hist.size, C.byref(got)))
        assert got.value == hist.shape[0]
        return (hist, bits, iters) if decode else hist

    # ---- failed frames captured on the device (lut_ldpc_amd/err_events.py) --------------------------------------
    def error_events(self, cha, msg0, sent=None, select="codeword", max_frames=1024, max_pos=64, max_chk=64, profiles=None, k_info=None, decode=False):
        """Decodes the batch and captures its failed frames on the device: an `ErrorEvents` with one record per kept frame, the
        sorted indices of its wrong nodes (first max_pos) and unsatisfied checks (first max_chk), and the number selected.
        sent: [B, nvar] bits the decided ones are compared with (None: all-zero codeword; need not be a codeword).  select:
        "codeword" (any wrong node), "info" (a wrong data bit among the first k_info nodes, default nvar - nchk), "failed"
        (iteration code < 0), "undetected" (wrong, but code >= 0).  profiles: None, True (new arrays) or (node_errors int64 [nvar],
        check_fails int64 [nchk]) to add into.  decode=True returns (events, bits, iters)."""
        from .err_events import _Request
        cha, msg0, sent, B, N = self._label_rows(cha, msg0, sent)
        rq = _Request(self.nvar, self.nchk, select, max_frames, max_pos, max_chk, profiles)
        bits = np.empty((B, N), np.uint8) if decode else None
        iters = np.empty(B, np.int32) if decode else None
        check(lib.lutldpc_decoder_events_batch(self._h, _p(cha, C.c_uint8), _p(msg0, C.c_uint8), _opt(sent, C.c_uint8), B,
                                               int(self.nvar - self.nchk if k_info is None else k_info), _opt(bits, C.c_uint8), _opt(iters, C.c_int32),
                                               C.byref(rq.c)))
        return (rq.result(), bits, iters) if decode else rq.result()

    # ---- Monte-Carlo front end on the device: cell sampler, random codewords, error counters --------------------------------
    #      cells: a _capi.ChannelCells or the dict Codec.channel_cells returns, or None for the node channels of set_node_channels; codewords: host [B, nvar] sent bits (bit 0 of a byte
    #      counts) or None for the all-zero codeword; outputs: new arrays, or the caller's own with at least B rows
    def set_generator(self, K, R, rows):
        """The generator of the device encoder: R rows of ceil(K/64) uint64 words, K + R = nvar (replaces an earlier one)."""
        rows = np.ascontiguousarray(rows, np.uint64)
        if K < 1 or R < 0 or rows.size != R * ((K + 63) // 64):
            raise ValueError("rows must hold R rows of ceil(K/64) uint64 words")
        buf = rows if R else np.zeros(1, np.uint64)                 # (R = 0: no row is read, the pointer must not be null)
        check(lib.lutldpc_decoder_set_generator(self._h, int(K), int(R), _p(buf, C.c_uint64)))

    def set_sparse_generator(self, K, R, row_ptr, cols):
        """The generator as a sparse triangular system (lutldpc_decoder_set_sparse_generator): codeword bit K+i = XOR of the codeword
        bits cols[row_ptr[i]:row_ptr[i+1]], K + R = nvar, any K.  Replaces an earlier generator of either form."""
        row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        cols = np.ascontiguousarray(cols, np.int32)
        if row_ptr.size != R + 1:
            raise ValueError("row_ptr must hold R + 1 entries")
        buf = cols if cols.size else np.zeros(1, np.int32)          # (no terms: nothing is read, the pointer must not be null)
        check(lib.lutldpc_decoder_set_sparse_generator(self._h, int(K), int(R), _p(row_ptr, C.c_int32), _p(buf, C.c_int32)))

    def set_node_channels(self, node_class, tables=None):
        """Per-node channel classes of the sampler (lutldpc_decoder_set_node_channels): node v is sampled with tables[node_class[v]]
        by every entry called with cells=None.  node_class: nvar ids; tables: up to 16 cell tables (dicts as Codec.channel_cells
        returns them).  set_node_channels(None) clears."""
        if node_class is None:
            check(lib.lutldpc_decoder_set_node_channels(self._h, None))
            return
        ids = np.ascontiguousarray(node_class, np.uint8)
        if ids.shape != (self.nvar,):
            raise ValueError("node_class must hold one class id per node")
        check(lib.lutldpc_decoder_set_node_channels(self._h, C.byref(_capi.NodeChannels.from_tables(ids, tables))))

    def encode_random(self, seed, stream, frame0, B, fetch=True, out=None):
        """The random codewords of frames frame0 .. frame0+B-1, uint8 [B, nvar]; fetch=False keeps them on the device only."""
        cw = _out(out, B, self.nvar, np.uint8, "out") if fetch else None
        check(lib.lutldpc_decoder_encode_random(self._h, int(seed), int(stream), int(frame0), int(B), _opt(cw, C.c_uint8)))
        return cw

    def _codewords(self, codewords, B):
        if codewords is None:
            return None
        cw = np.ascontiguousarray(codewords, np.uint8)
        if cw.shape != (B, self.nvar):
            raise ValueError("codewords must be [B, nvar]")
        return cw

    def sample_labels(self, cells, seed, stream, frame0, B, codewords=None, cha=None, msg=None):
        """(cha, msg0) as the sampler makes them for those frames."""
        cells, cw = _cells(cells), self._codewords(codewords, B)
        cha, msg = _out(cha, B, self.nvar, np.uint8, "cha"), _out(msg, B, self.nvar, np.uint8, "msg")
        check(lib.lutldpc_decoder_sample_labels(self._h, cells, int(seed), int(stream), int(frame0), int(B), _opt(cw, C.c_uint8),
                                                _p(cha, C.c_uint8), _p(msg, C.c_uint8)))
        return cha, msg

    def sim_batch(self, cells, seed, stream, frame0, B, k_info, codewords=None, random=False, frame_stats=None, cha_out=None, bits_out=None):
        """Sampler + decode + counters: frame_stats int32 [B, 4] = {iteration code, frame error, data bit errors among the first k_info
        bits, uncoded errors}.  random=True: over the codewords of the device encoder (lutldpc_decoder_sim_batch_random).  Returns
        (frame_stats, cha_out, bits_out); the sampled channel labels and the decided bits only where cha_out / bits_out is True (a new
        array) or an array to fill, else None."""
        cells, cw = _cells(cells), self._codewords(codewords, B)
        stats = _out(frame_stats, B, 4, np.int32, "frame_stats")
        cha = None if cha_out is None else _out(None if cha_out is True else cha_out, B, self.nvar, np.uint8, "cha_out")
        bits = None if bits_out is None else _out(None if bits_out is True else bits_out, B, self.nvar, np.uint8, "bits_out")
        head = (self._h, cells, int(seed), int(stream), int(frame0), int(B))
        tail = (int(k_info), _p(stats, C.c_int32), _opt(cha, C.c_uint8), _opt(bits, C.c_uint8))
        if random:
            if cw is not None:
                raise ValueError("random=True takes the codewords of the device encoder, not the caller's")
            check(lib.lutldpc_decoder_sim_batch_random(*head, *tail))
        else:
            check(lib.lutldpc_decoder_sim_batch(*head, _opt(cw, C.c_uint8), *tail))
        return stats, cha, bits

    def sim_batch_histogram(self, cells, seed, stream, frame0, B, codewords=None, device_codewords=False, level=3, mode="all", n_labels=None, hist=None):
        """message_histogram of the frames sim_batch sends (device_codewords=True: sim_batch with random=True), added into `hist`."""
        cells, cw = _cells(cells), self._codewords(codewords, B)
        hist = self._hist(hist, level, n_labels)
        got = C.c_int32()
        check(lib.lutldpc_decoder_sim_batch_histogram(self._h, cells, int(seed), int(stream), int(frame0), int(B), _opt(cw, C.c_uint8),
                                                      int(device_codewords), int(level), MODES[mode] if isinstance(mode, str) else int(mode),
                                                      hist.shape[3], _p(hist, C.c_int64), hist.size, C.byref(got)))
        assert got.value == hist.shape[0]
        return hist

    def sim_batch_events(self, cells, seed, stream, frame0, B, k_info=None, codewords=None, device_codewords=False, select="codeword", max_frames=1024,
                         max_pos=64, max_chk=64, profiles=None, frame_stats=None):
        """error_events of the frames sim_batch sends: (ErrorEvents, frame_stats)."""
        from .err_events import _Request
        cells, cw = _cells(cells), self._codewords(codewords, B)
        rq = _Request(self.nvar, self.nchk, select, max_frames, max_pos, max_chk, profiles)
        stats = _out(frame_stats, B, 4, np.int32, "frame_stats")
        check(lib.lutldpc_decoder_sim_batch_events(self._h, cells, int(seed), int(stream), int(frame0), int(B), _opt(cw, C.c_uint8),
                                                   int(device_codewords), int(self.nvar - self.nchk if k_info is None else k_info),
                                                   _p(stats, C.c_int32), C.byref(rq.c)))
        return rq.result(), stats

    def decode_llr_batch(self, llr, qb_cha, qb_msg, mode=0, cha2msg_map=None):
        llr = np.ascontiguousarray(llr, np.float64)
        B, N = llr.shape
        qc = np.ascontiguousarray(qb_cha, np.float64)
        qm = np.ascontiguousarray(qb_msg if qb_msg is not None else [], np.float64)
        mp = _i32(cha2msg_map) if cha2msg_map is not None else None
        out = np.empty((B, N), np.uint8)
        iters = np.empty(B, np.int32)
        check(lib.lutldpc_decoder_decode_llr_batch(self._h, _p(llr, C.c_double), B, _p(qc, C.c_double), len(qc),
                                                   _p(qm, C.c_double), len(qm), int(mode),
                                                   _p(mp, C.c_int32) if mp is not None else None,
                                                   _p(out, C.c_uint8), _p(iters, C.c_int32)))
        return out, iters

    def decode_llr(self, llr, qb_cha, qb_msg=None, cha2msg_map=None, scale=None, first=0, count=None, want_labels=False, decode=True):
        """decode(llr) for receivers (lutldpc_decoder_decode_llr_packed): llr is [B, nvar] float64, float32, float16 or int8 (then
        LLR = scale * q), a numpy array or a torch tensor on the decoder's device (2-D, last dimension contiguous, row stride >=
        nvar; read in place).  qb_cha with either qb_msg (mode CONT) or cha2msg_map (mode QCHA).  Returns (words, iters): the decided
        bits first .. first+count-1 of every frame, one bit each (packing.unpack_bits; count=None: up to nvar), with
        want_labels=True also (cha, msg0) as the device derived them; decode=False only quantises and returns (cha, msg0).
        For a tensor the results are tensors on its device (words as int32: the same 32 bits), the tensor's current stream is
        synchronised before the call and the decoder's stream before it returns."""
        qc = np.ascontiguousarray(qb_cha, np.float64)
        qm = np.ascontiguousarray(qb_msg, np.float64) if qb_msg is not None else None
        mp = _i32(cha2msg_map) if cha2msg_map is not None else None
        if (qm is None) == (mp is None):
            raise ValueError("give either qb_msg (mode CONT) or cha2msg_map (mode QCHA)")
        if mp is not None and len(mp) != len(qc) + 1:
            raise ValueError("cha2msg_map must hold one entry per channel label")
        side = _Side(llr)
        if side.on_device:
            import torch
            names = {torch.float64: _capi.LLR_F64, torch.float32: _capi.LLR_F32, torch.float16: _capi.LLR_F16, torch.int8: _capi.LLR_I8}
            if not llr.is_cuda:
                raise ValueError("a torch tensor must live on the device; pass host values as a numpy array")
        else:
            if not isinstance(llr, np.ndarray):
                raise ValueError("llr must be a numpy array or a torch tensor on the device")
            names = {np.dtype(np.float64): _capi.LLR_F64, np.dtype(np.float32): _capi.LLR_F32, np.dtype(np.float16): _capi.LLR_F16,
                     np.dtype(np.int8): _capi.LLR_I8}
        if llr.dtype not in names:
            raise ValueError("llr must be float64, float32, float16 or int8")
        dtype = names[llr.dtype]
        if llr.ndim != 2 or llr.shape[1] != self.nvar or llr.shape[0] < 1:
            raise ValueError("llr must be [B, nvar]")
        if dtype == _capi.LLR_I8 and scale is None:
            raise ValueError("int8 values need a scale: LLR = scale * q")
        if not decode and not want_labels:
            want_labels = True
        B, N = int(llr.shape[0]), self.nvar
        count = N - int(first) if count is None else int(count)
        side.place(llr, N, "nvar")
        words, iters = side.empty((B, max((count + 31) // 32, 0)), np.uint32, decode), side.empty(B, np.int32, decode)
        cha, msg = side.empty((B, N), np.uint8, want_labels), side.empty((B, N), np.uint8, want_labels)
        io = _capi.LlrIO(dtype, int(side.on_device), side.stride, float(scale) if scale is not None else 0.0, _p(qc, C.c_double), len(qc),
                         _opt(qm, C.c_double), len(qm) if qm is not None else 0, 0 if qm is not None else 1, _opt(mp, C.c_int32), int(first), count, 1)
        check(lib.lutldpc_decoder_decode_llr_packed(self._h, C.byref(io), side.ptr(side.src), B, side.ptr(words), side.ptr(iters), side.ptr(cha),
                                                    side.ptr(msg)))
        out = (words, iters) if decode else ()
        return out + (cha, msg) if want_labels else out

    def encode_packed(self, info_words, first=0, count=None, sync=True):
        """The caller's data bits encoded on the device (lutldpc_decoder_encode_packed; the generator of set_generator): info_words
        is [B, W] with W >= ceil(K/32), bit j of word w = information bit 32w + j (packing.pack_bits) -- a numpy uint32 / int32
        array, or a torch int32 tensor on the decoder's device (2-D, last dimension contiguous; read in place).  Returns the
        codeword bits first .. first+count-1 of every frame, one bit each, [B, ceil(count/32)] (packing.unpack_bits; count=None: up
        to nvar): a numpy uint32 array, or an int32 tensor on the tensor's device.  For a tensor the tensor's current stream is
        synchronised before the call and (sync=True) the decoder's stream before it returns."""
        side = _Side(info_words)
        if side.on_device:
            import torch
            if not info_words.is_cuda:
                raise ValueError("a torch tensor must live on the device; pass host words as a numpy array")
            if info_words.dtype != torch.int32:
                raise ValueError("a tensor of information words must be int32")
        else:
            if not isinstance(info_words, np.ndarray) or info_words.dtype not in (np.dtype(np.uint32), np.dtype(np.int32)):
                raise ValueError("info_words must be a numpy uint32 / int32 array or a torch int32 tensor on the device")
        if info_words.ndim != 2 or info_words.shape[0] < 1 or info_words.shape[1] < 1:
            raise ValueError("info_words must be [B, W]")
        B, W = int(info_words.shape[0]), int(info_words.shape[1])
        count = self.nvar - int(first) if count is None else int(count)
        side.place(info_words, W, "its width")
        out = side.empty((B, max((count + 31) // 32, 0)), np.uint32)
        io = _capi.EncodeIO(int(side.on_device), side.stride, int(first), count, int(bool(sync)))
        check(lib.lutldpc_decoder_encode_packed(self._h, C.byref(io), side.ptr(side.src), B, side.ptr(out)))
        return out

    # ---- device buffers (raw pointers, e.g. torch.Tensor.data_ptr()) -------------------------
    def lut_decode_batch_device(self, d_cha: int, d_msg0: int, B: int, d_out_bits: int, d_out_iters: int, sync=False):
        check(lib.lutldpc_decoder_decode_batch_device(self._h, C.c_void_p(d_cha), C.c_void_p(d_msg0), int(B),
                                                      C.c_void_p(d_out_bits), C.c_void_p(d_out_iters), int(sync)))

    @property
    def stream(self) -> int:
        return lib.lutldpc_decoder_stream(self._h) or 0

    # ---- measurement -----------------------------------------------------------------------
    def set_profiling(self, on: bool):
        check(lib.lutldpc_decoder_set_profiling(self._h, int(on)))

    def reset_profile(self):
        check(lib.lutldpc_decoder_reset_profile(self._h))

    def profile(self) -> dict:
        out = {}
        for k, name in enumerate(_capi.KIND_NAMES):
            ms, n = C.c_double(), C.c_int64()
            check(lib.lutldpc_decoder_get_profile(self._h, k, C.byref(ms), C.byref(n)))
            out[name] = {"ms": ms.value, "launches": n.value}
        return out

    def device_bytes(self) -> int:
        return lib.lutldpc_decoder_device_bytes(self._h)

    def describe(self) -> dict:
        return json.loads(lib.lutldpc_decoder_describe(self._h).decode())

    def jit_source(self, kind: int, tree_set: int, cls: int, compile: bool = False) -> str:
        """HIP source generated for a variable (0) / check-tree (1; 1 + 32: over full labels) / decision (2) class; compile=True also
        runs hiprtc (no GPU needed)."""
        n = lib.lutldpc_selftest_jit_source(self._h, kind, tree_set, cls, None, 0, int(compile))
        if n < 0:
            check(int(n))
        buf = C.create_string_buffer(n)
        lib.lutldpc_selftest_jit_source(self._h, kind, tree_set, cls, buf, n, 0)
        return buf.value.decode()

    def resident_source(self, G: int, compile: bool = False):
        """HIP source of the LDS-resident decode kernel for G frame groups, and (sets per workgroup, threads, LDS bytes)."""
        info = (C.c_int32 * 3)()
        n = lib.lutldpc_selftest_resident_source(self._h, int(G), None, 0, int(compile), info)
        if n < 0:
            check(int(n))
        buf = C.create_string_buffer(n)
        lib.lutldpc_selftest_resident_source(self._h, int(G), buf, n, 0, info)
        return buf.value.decode(), tuple(info)

    # ---- compile-step self test (host only) ----------------------------------------------------
    def program_eval(self, kind: int, tree_set: int, cls: int, inputs, n_out: int):
        a = _i32(inputs)
        out = np.zeros(n_out, np.int32)
        check(lib.lutldpc_selftest_program_eval(self._h, kind, tree_set, cls, _p(a, C.c_int32), len(a), _p(out, C.c_int32), n_out))
        return out

    def program_stats(self, kind: int, tree_set: int, cls: int):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib.lutldpc_selftest_program_stats(self._h, kind, tree_set, cls, C.byref(a), C.byref(b), C.byref(c)))
        return {"ops": a.value, "ops_naive": b.value, "slots": c.value}
