"""Python view of the C++ host mirror of LDPC_Code_LUT (include/lut_ldpc_host.h).

`Codec` = parity-check matrix + (optional) systematic generator + LDPC_Code_LUT, i.e. what
LDPC_BER_Sim_LUT::load builds in the reference (src/LDPC_BER_Sim.cpp:434-550).  LUT design runs in
the C++ host code, decoding in the HIP kernels.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import lib, check
from .decoder import Decoder


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Codec:
    def __init__(self, alist_path=None, with_generator=False, known_rank=0, device=0, codec_path=None):
        self._h = C.c_void_p()
        if codec_path is not None:
            check(lib.lutldpc_codec_load(str(codec_path).encode(), int(device), C.byref(self._h)))
        else:
            # with_generator: False / True (dense where the matrix is small enough to eliminate, else the sparse triangular form where
            # the parity part of H peels) / "sparse" (the sparse form, or an error)
            if isinstance(with_generator, str) and with_generator != "sparse":
                raise ValueError('with_generator must be False, True or "sparse"')
            gen = 2 if with_generator == "sparse" else int(bool(with_generator))
            check(lib.lutldpc_codec_create(str(alist_path).encode(), gen, int(known_rank), int(device), C.byref(self._h)))
        n, m, e, r = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(lib.lutldpc_codec_dims(self._h, n, m, e, r))
        self.nvar, self.nchk, self.nedges, self.rank = n.value, m.value, e.value, r.value
        self.ninfo = self.nvar - self.rank
        self.max_iters = 0

    def close(self):
        if getattr(self, "_h", None):
            lib.lutldpc_codec_destroy(self._h)
            self._h = None

    __del__ = close

    # ---- set-up -------------------------------------------------------------------------------
    def design_luts(self, tree_method="auto_bin_balanced", min_lut=True, sigma2=0.88 ** 2, max_iters=50, reuse_vec=None,
                    nq_cha=16, nq_msg=16, allow_degree_one=False) -> float:
        reuse = np.zeros(max_iters, np.uint8) if reuse_vec is None else np.ascontiguousarray(reuse_vec, np.uint8)
        nq = np.full(max_iters, nq_msg, np.int32) if np.isscalar(nq_msg) else np.ascontiguousarray(nq_msg, np.int32)
        sig = C.c_double()
        check(lib.lutldpc_codec_design_luts(self._h, tree_method.encode(), int(min_lut), float(sigma2), int(max_iters),
                                            _p(reuse, C.c_uint8), int(nq_cha), _p(nq, C.c_int32), int(allow_degree_one), C.byref(sig)))
        self.max_iters = max_iters
        self.design_from_cache = bool(lib.lutldpc_codec_design_from_cache(self._h))   # LUTLDPC_DESIGN_CACHE=<dir>
        return sig.value

    def set_exit_conditions(self, max_iters, psc=True, pisc=False):
        check(lib.lutldpc_codec_set_exit_conditions(self._h, int(max_iters), int(psc), int(pisc)))

    def set_initial_message_mode(self, mode: int):
        check(lib.lutldpc_codec_set_initial_message_mode(self._h, int(mode)))

    def save(self, path):
        check(lib.lutldpc_codec_save(self._h, str(path).encode()))

    # ---- getters --------------------------------------------------------------------------------
    def graph(self):
        dv, dc, cn = np.zeros(self.nvar, np.int32), np.zeros(self.nchk, np.int32), np.zeros(self.nedges, np.int32)
        check(lib.lutldpc_codec_graph(self._h, _p(dv, C.c_int32), _p(dc, C.c_int32), _p(cn, C.c_int32)))
        return dv, dc, cn

    def _txt(self, fn) -> str:
        need = fn(self._h, None, 0)
        buf = C.create_string_buffer(int(need))
        fn(self._h, buf, need)
        return buf.value.decode()

    @property
    def var_trees_txt(self) -> str:
        return self._txt(lib.lutldpc_codec_var_trees_txt)

    @property
    def chk_trees_txt(self) -> str:
        return self._txt(lib.lutldpc_codec_chk_trees_txt)

    def qb(self, which: int) -> np.ndarray:
        n = lib.lutldpc_codec_qb(self._h, which, None, 0)
        out = np.zeros(n, np.float64)
        lib.lutldpc_codec_qb(self._h, which, _p(out, C.c_double), n)
        return out

    @property
    def qb_cha(self):
        return self.qb(0)

    @property
    def qb_msg(self):
        return self.qb(1)

    @property
    def cha2msg_map(self) -> np.ndarray:
        n = lib.lutldpc_codec_cha2msg_map(self._h, None, 0)
        out = np.zeros(n, np.int32)
        lib.lutldpc_codec_cha2msg_map(self._h, _p(out, C.c_int32), n)
        return out

    @property
    def rate(self) -> float:
        return lib.lutldpc_codec_rate(self._h)

    def decoder(self) -> Decoder:
        """The HIP decoder behind this codec (borrowed handle, for device-pointer decode and profiling)."""
        h = lib.lutldpc_codec_decoder(self._h)
        if not h:
            check(-5)
        d = Decoder.__new__(Decoder)
        d._h = C.c_void_p(h)
        d.nvar, d.nchk, d.max_iters, d.device = self.nvar, self.nchk, self.max_iters, 0
        d._owned = False            # the codec owns (and destroys) the handle
        d._owner = self
        return d

    # ---- decode -----------------------------------------------------------------------------------
    def decode_llr_batch(self, llr):
        llr = np.ascontiguousarray(llr, np.float64)
        B, N = llr.shape
        bits, iters = np.empty((B, N), np.uint8), np.empty(B, np.int32)
        check(lib.lutldpc_codec_decode_llr_batch(self._h, _p(llr, C.c_double), B, _p(bits, C.c_uint8), _p(iters, C.c_int32)))
        return bits, iters

    def lut_decode_dump(self, cha, msg0, level=2):
        """lut_decode with output_verbosity = level (2 or 3): (bits, iters, text of the message dumps as the reference prints them)."""
        cha = np.ascontiguousarray(cha, np.uint8); msg0 = np.ascontiguousarray(msg0, np.uint8)
        B = cha.shape[0]
        bits = np.empty_like(cha); iters = np.empty(B, np.int32)
        n = lib.lutldpc_codec_lut_decode_dump(self._h, _p(cha, C.c_uint8), _p(msg0, C.c_uint8), B, int(level), _p(bits, C.c_uint8), _p(iters, C.c_int32), None, 0)
        if n < 0:
            check(int(n))
        buf = C.create_string_buffer(n)
        n2 = lib.lutldpc_codec_lut_decode_dump(self._h, _p(cha, C.c_uint8), _p(msg0, C.c_uint8), B, int(level), _p(bits, C.c_uint8), _p(iters, C.c_int32), buf, n)
        if n2 < 0:
            check(int(n2))
        return bits, iters, buf.value.decode()

    def lut_decode_batch(self, cha, msg0):
        cha = np.ascontiguousarray(cha, np.uint8)
        msg0 = np.ascontiguousarray(msg0, np.uint8)
        B, N = cha.shape
        bits, iters = np.empty((B, N), np.uint8), np.empty(B, np.int32)
        check(lib.lutldpc_codec_lut_decode_batch(self._h, _p(cha, C.c_uint8), _p(msg0, C.c_uint8), B, _p(bits, C.c_uint8), _p(iters, C.c_int32)))
        return bits, iters

    def decode_packed(self, cha, nibbles=False, info_only=True):
        """Decoder.decode_packed with what the codec knows: the initial messages from its cha2msg_map on the device, and (info_only)
        only the nvar - rank(H) data bits returned.  (words, iters).  The map stands for the initial messages only in the mode
        from_quantized_channel_llrs (QCHA, set_initial_message_mode(1)); in any other mode this raises."""
        if lib.lutldpc_codec_initial_message_mode(self._h) != 1:
            raise ValueError("decode_packed derives the initial messages from the channel labels: the codec's initial-message mode must be "
                             "QCHA (set_initial_message_mode(1)); with continuous-input messages use Decoder.decode_packed(cha, msg0=...)")
        return self.decoder().decode_packed(cha, cha2msg_map=self.cha2msg_map, nibbles=nibbles, first=0, count=self.ninfo if info_only else self.nvar)

    def decode_llr(self, llr, scale=None, info_only=True):
        """Decoder.decode_llr with what the codec knows: its boundaries, its initial-message mode (CONT: qb_msg, QCHA: cha2msg_map) and
        (info_only) only the nvar - rank(H) data bits returned.  llr: [B, nvar] float64 / float32 / float16 / int8 (with scale),
        numpy or a torch tensor on the device.  (words, iters)."""
        mode = lib.lutldpc_codec_initial_message_mode(self._h)
        if mode not in (0, 1):
            raise ValueError("decode_llr needs the initial-message mode CONT (0) or QCHA (1)")
        return self.decoder().decode_llr(llr, self.qb_cha, qb_msg=self.qb_msg if mode == 0 else None, cha2msg_map=self.cha2msg_map if mode == 1 else None,
                                         scale=scale, first=0, count=self.ninfo if info_only else self.nvar)

    # ---- Monte-Carlo front end ------------------------------------------------------------------------
    def sim_batch(self, snr_db, seed, stream, frame0, B, zero_codeword=True) -> np.ndarray:
        """{iters, frame error, data bit errors, uncoded errors} of frames frame0..frame0+B-1 (device sampler + decode)."""
        stats = np.empty((B, 4), np.int32)
        check(lib.lutldpc_codec_sim_batch(self._h, float(snr_db), int(seed), int(stream), int(frame0), int(B), int(zero_codeword), _p(stats, C.c_int32)))
        return stats

    def message_histogram(self, snr_db, seed, stream, frame0, B, zero_codeword=True, level=3, mode="all", n_labels=None, hist=None) -> np.ndarray:
        """Message-label histograms hist[dump, group, sent bit, label] (int64) of the frames sim_batch would simulate, counted on the
        device (Decoder.message_histogram); added into `hist` when given.  The edge grouping is that of self.decoder()."""
        from .decoder import MODES
        hist = self.decoder().new_histogram(level, n_labels) if hist is None else hist
        got = C.c_int32()
        check(lib.lutldpc_codec_message_histogram(self._h, float(snr_db), int(seed), int(stream), int(frame0), int(B), int(zero_codeword), int(level),
                                                  MODES[mode] if isinstance(mode, str) else int(mode), hist.shape[3], _p(hist, C.c_int64), hist.size,
                                                  C.byref(got)))
        assert got.value == hist.shape[0]
        return hist

    def error_events(self, snr_db, seed, stream, frame0, B, zero_codeword=True, select="codeword", max_frames=1024, max_pos=64, max_chk=64, profiles=None):
        """Failed frames of the batch sim_batch would simulate, captured on the device (Decoder.error_events): an `ErrorEvents`.
        events[:, 0] is the offset in the batch: frame0 + offset replays the frame."""
        from .err_events import _Request
        rq = _Request(self.nvar, self.nchk, select, max_frames, max_pos, max_chk, profiles)
        check(lib.lutldpc_codec_error_events(self._h, float(snr_db), int(seed), int(stream), int(frame0), int(B), int(zero_codeword), C.byref(rq.c)))
        return rq.result()

    def sample_labels(self, snr_db, seed, stream, frame0, B, zero_codeword=True):
        cha, msg = np.empty((B, self.nvar), np.uint8), np.empty((B, self.nvar), np.uint8)
        cw = np.empty((B, self.nvar), np.uint8)
        check(lib.lutldpc_codec_sample_labels(self._h, float(snr_db), int(seed), int(stream), int(frame0), int(B), int(zero_codeword),
                                              _p(cha, C.c_uint8), _p(msg, C.c_uint8), _p(cw, C.c_uint8)))
        return cha, msg, cw

    def encode_random(self, seed, stream, frame0, B) -> np.ndarray:
        """The random codewords of frames frame0..frame0+B-1 that sim_batch(zero_codeword=False) sends, made on the device
        (Philox information bits + generator parity): (B, nvar) uint8."""
        cw = np.empty((B, self.nvar), np.uint8)
        check(lib.lutldpc_codec_encode_random(self._h, int(seed), int(stream), int(frame0), int(B), _p(cw, C.c_uint8)))
        return cw

    def encode_packed(self, data, parity_only=False):
        """The caller's data encoded on the device (Decoder.encode_packed): data is [B, W >= ceil(ninfo/32)] packed words (numpy uint32 /
        int32, or a torch int32 tensor on the device; packing.pack_bits makes them), or a 0/1 uint8 array [B, ninfo], which is packed
        first.  Returns the codewords [u | parity] as [B, ceil(nvar/32)] words, or with parity_only the rank(H) parity bits alone,
        [B, ceil(rank/32)]; same kind of array, same place."""
        dec = self.decoder()
        if "generator" not in dec.describe():
            raise ValueError("encode_packed needs the generator on the device: make the Codec with with_generator=True on a device "
                             "(a dense generator holds at most 8192 information bits there; beyond that the parity part of H must "
                             'peel to the sparse triangular form, which with_generator="sparse" asks for at any size)')
        if isinstance(data, np.ndarray) and data.dtype == np.uint8:
            from .packing import pack_bits
            if data.ndim != 2 or data.shape[1] != self.ninfo:
                raise ValueError("a uint8 array of data bits must be [B, ninfo]")
            data = pack_bits(data)
        first, count = (self.ninfo, self.rank) if parity_only else (0, self.nvar)
        return dec.encode_packed(data, first=first, count=count)

    def _cell_table(self, fn, *args):
        thr = np.zeros(72, np.uint64)
        arrs = [np.zeros(72, np.uint8) for _ in range(5)]
        n = fn(self._h, *args, _p(thr, C.c_uint64), *[_p(a, C.c_uint8) for a in arrs])
        check(min(n, 0))
        return {"thr": thr[:n - 1], "cha": arrs[0][:n], "msg": arrs[1][:n], "neg": arrs[2][:n], "cha_m": arrs[3][:n], "msg_m": arrs[4][:n]}

    def channel_cells(self, snr_db):
        return self._cell_table(lib.lutldpc_codec_channel_cells, float(snr_db))

    def set_node_channels(self, node_class, offsets_db=None):
        """Per-node channel classes of sim_batch, message_histogram, error_events and sample_labels: node v belongs to class
        node_class[v], class k sees the channel at snr_db + offsets_db[k] dB; -inf is a punctured node (an erasure), +inf a known
        bit.  N0 still comes from the SNR and the code's rate: account for the effective rate of a punctured code yourself.
        set_node_channels(None) clears."""
        if node_class is None:
            check(lib.lutldpc_codec_set_node_channels(self._h, None, 0, None))
            return
        ids = np.ascontiguousarray(node_class, np.uint8)
        off = np.ascontiguousarray(offsets_db, np.float64)
        if ids.shape != (self.nvar,) or off.ndim != 1:
            raise ValueError("node_class must hold one class id per node, offsets_db one offset per class")
        check(lib.lutldpc_codec_set_node_channels(self._h, _p(ids, C.c_uint8), len(off), _p(off, C.c_double)))

    def node_channel_cells(self, snr_db, cls):
        """The cell table of class `cls` at that SNR, as channel_cells returns the code's."""
        return self._cell_table(lib.lutldpc_codec_node_channel_cells, float(snr_db), int(cls))

    def encode(self, info):
        info = np.ascontiguousarray(info, np.uint8)
        assert info.shape == (self.ninfo,)
        cw = np.empty(self.nvar, np.uint8)
        check(lib.lutldpc_codec_encode(self._h, _p(info, C.c_uint8), _p(cw, C.c_uint8)))
        return cw


def de_threshold(dl, lam, dr, rho, qbits_cha=4, qbits_msg=4, maxiter_de=2000, min_lut=True, tree_mode="auto_bin_balanced",
                 strategy="joint_root", thr_min=1e-7, thr_prec=1e-5, pe_max=1e-10, maxiter_bisec=50, max_ni_de_iters=1,
                 llr_max=25.0, nq_fine=5000):
    dl = np.ascontiguousarray(dl, np.int32)
    dr = np.ascontiguousarray(dr, np.int32)
    lam = np.ascontiguousarray(lam, np.float64)
    rho = np.ascontiguousarray(rho, np.float64)
    thr = C.c_double()
    it = lib.lutldpc_de_threshold(_p(dl, C.c_int32), _p(lam, C.c_double), len(dl), _p(dr, C.c_int32), _p(rho, C.c_double), len(dr),
                                  qbits_cha, qbits_msg, maxiter_de, int(min_lut), tree_mode.encode(), strategy.encode(), thr_min,
                                  thr_prec, pe_max, maxiter_bisec, max_ni_de_iters, llr_max, nq_fine, C.byref(thr))
    if it < -1:
        check(it)
    return thr.value, it
