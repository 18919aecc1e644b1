"""ctypes binding of the C-ABI declared in include/lut_ldpc_hip.h (liblut_ldpc_amd.so).

There is no CPU fallback: if the shared library is missing this module raises at import, and
every decode call fails with the library's error text when no MI355X is visible.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "lib" / "liblut_ldpc_amd.so"
if os.environ.get("LUTLDPC_LIB"):          # A/B runs of two builds of the same library (tools/)
    LIB_PATH = Path(os.environ["LUTLDPC_LIB"])

OK, ERR_ARG, ERR_PARSE, ERR_UNSUPPORTED, ERR_HIP, ERR_STATE = 0, -1, -2, -3, -4, -5
K_CN_PASS, K_VN_PASS, K_DECISION, K_SYNDROME, K_LAYOUT, K_FRONTEND, K_FUSED_PASS, K_RESIDENT, K_HISTOGRAM, K_COUNT = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9
KIND_NAMES = ["cn_pass", "vn_pass", "decision", "syndrome", "layout", "frontend", "fused_pass", "resident", "histogram"]


class LutLdpcError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[{code}] {msg}")
        self.code = code


def _load() -> C.CDLL:
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C lut_ldpc_amd/csrc` (hipcc, gfx950). There is no CPU fallback."
        )
    return C.CDLL(str(LIB_PATH), mode=C.RTLD_GLOBAL)


lib = _load()

_vp, _ip, _u8p, _dp, _cp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.c_char_p
_i64p, _u32p, _u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


class EventRequest(C.Structure):
    """lutldpc_event_request (include/lut_ldpc_hip.h): what a capture of failed frames selects, how much it keeps, where it goes."""
    _fields_ = [("select", C.c_int32), ("max_frames", C.c_int32), ("max_pos", C.c_int32), ("max_chk", C.c_int32),
                ("events", _ip), ("positions", _ip), ("checks", _ip), ("node_errors", _i64p), ("check_fails", _i64p),
                ("n_selected", C.c_int32), ("n_stored", C.c_int32)]


_evp = C.POINTER(EventRequest)
IN_BYTES, IN_NIBBLES = 0, 1


class PackedIO(C.Structure):
    """lutldpc_packed_io (include/lut_ldpc_hip.h): input format, the optional channel-to-message map, the window of decided bits."""
    _fields_ = [("in_format", C.c_int32), ("cha2msg_map", _ip), ("out_first", C.c_int32), ("out_count", C.c_int32)]


LLR_F64, LLR_F32, LLR_F16, LLR_I8 = 0, 1, 2, 3


class LlrIO(C.Structure):
    """lutldpc_llr_io (include/lut_ldpc_hip.h): element type and location of the soft values, the quantiser, the window of decided bits."""
    _fields_ = [("dtype", C.c_int32), ("on_device", C.c_int32), ("frame_stride", C.c_int64), ("scale", C.c_double),
                ("qb_Cha", _dp), ("n_qb_Cha", C.c_int32), ("qb_Msg", _dp), ("n_qb_Msg", C.c_int32),
                ("initial_message_mode", C.c_int32), ("cha2msg_map", _ip), ("out_first", C.c_int32), ("out_count", C.c_int32),
                ("sync", C.c_int32)]


class EncodeIO(C.Structure):
    """lutldpc_encode_io (include/lut_ldpc_hip.h): location and frame stride of the packed information words, the window of codeword bits."""
    _fields_ = [("on_device", C.c_int32), ("in_stride", C.c_int64), ("out_first", C.c_int32), ("out_count", C.c_int32), ("sync", C.c_int32)]


class ChannelCells(C.Structure):
    """lutldpc_channel_cells (include/lut_ldpc_hip.h): the cell table of the Philox sampler."""
    _fields_ = [("n_cells", C.c_int32), ("thr", _u64p), ("cha_label", _u8p), ("msg_label", _u8p), ("slicer_neg", _u8p),
                ("cha_label_mirror", _u8p), ("msg_label_mirror", _u8p)]

    @classmethod
    def from_table(cls, t):
        """From the dict Codec.channel_cells returns (thr uint64; cha, msg, neg, cha_m, msg_m uint8, one entry per cell).  The
        arrays stay alive on the instance."""
        keep = [np.ascontiguousarray(t["thr"], np.uint64)] + [np.ascontiguousarray(t[k], np.uint8) for k in ("cha", "msg", "neg", "cha_m", "msg_m")]
        cells = cls(len(keep[1]), keep[0].ctypes.data_as(_u64p), *[a.ctypes.data_as(_u8p) for a in keep[1:]])
        cells._keep = keep
        return cells


class _ccp(C.POINTER(ChannelCells)):
    """POINTER(ChannelCells) that also takes byref() of a caller's own Structure with the same field types.  Callers written before
    ChannelCells existed declared the struct themselves -- the tests of the commit before this class among them, which every change
    here is held against -- and must keep running against this package."""

    @classmethod
    def from_param(cls, obj):
        s = getattr(obj, "_obj", None)
        if isinstance(s, C.Structure) and not isinstance(s, ChannelCells) and [t for _, t in s._fields_] == [t for _, t in ChannelCells._fields_]:
            return C.byref(ChannelCells.from_buffer(s))
        return C.POINTER(ChannelCells).from_param(obj)


class NodeChannels(C.Structure):
    """lutldpc_node_channels (include/lut_ldpc_hip.h): the cell tables of the sampler's node classes and the class of every node."""
    _fields_ = [("n_classes", C.c_int32), ("tables", C.POINTER(ChannelCells)), ("node_class", _u8p)]

    @classmethod
    def from_tables(cls, node_class, tables):
        """From the class ids of the nodes and one table per class (dicts as Codec.channel_cells returns them, or ChannelCells).
        Everything the pointers name stays alive on the instance."""
        cells = [t if isinstance(t, ChannelCells) else ChannelCells.from_table(t) for t in tables]
        arr = (ChannelCells * max(len(cells), 1))(*cells)
        ids = np.ascontiguousarray(node_class, np.uint8)
        nc = cls(len(cells), arr, ids.ctypes.data_as(_u8p))
        nc._keep = (cells, arr, ids)
        return nc


class BPCells(C.Structure):
    """lutldpc_bp_cells (include/lut_ldpc_bp.h): the cell table of the [BP] decoder's device front end."""
    _fields_ = [("n_cells", C.c_int32), ("thr", _u64p), ("qllr", _ip), ("slicer_neg", _u8p)]

    @classmethod
    def from_table(cls, t):
        """From a dict {"thr": uint64[n - 1], "qllr": int32[n], "neg": uint8[n]} (bp.awgn_cells).  The arrays stay alive on the
        instance; a table of one cell gets a placeholder threshold (the pointer must not be NULL)."""
        thr = np.ascontiguousarray(t["thr"], np.uint64)
        keep = [thr if len(thr) else np.zeros(1, np.uint64), np.ascontiguousarray(t["qllr"], np.int32), np.ascontiguousarray(t["neg"], np.uint8)]
        cells = cls(len(keep[1]), keep[0].ctypes.data_as(_u64p), keep[1].ctypes.data_as(_ip), keep[2].ctypes.data_as(_u8p))
        cells._keep = keep
        return cells


# every function include/*.h declares -> (result, arguments)
_SIGNATURES = {
    "lutldpc_decoder_encode_packed": (C.c_int, [_vp, C.POINTER(EncodeIO), _vp, C.c_int, _vp]),
    "lutldpc_decoder_decode_llr_packed": (C.c_int, [_vp, C.POINTER(LlrIO), _vp, C.c_int, _vp, _vp, _vp, _vp]),
    "lutldpc_llr_cell_table": (C.c_int, [C.POINTER(LlrIO), C.c_int, C.c_int, _dp, C.c_int32, _ip, _u8p, _u8p]),
    "lutldpc_last_error": (_cp, []),
    "lutldpc_version": (_cp, []),
    "lutldpc_device_count": (C.c_int, []),
    "lutldpc_decoder_create": (C.c_int, [C.c_int, C.c_int, _ip, _ip, _ip, C.c_int, _ip, _u8p, C.c_int, C.c_int, _cp, _cp, C.c_int,
                                         C.POINTER(_vp)]),
    "lutldpc_decoder_destroy": (C.c_int, [_vp]),
    "lutldpc_decoder_set_exit_conditions": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
    "lutldpc_decoder_decode_batch": (C.c_int, [_vp, _u8p, _u8p, C.c_int, _u8p, _ip]),
    "lutldpc_decoder_decode_batch_packed": (C.c_int, [_vp, C.POINTER(PackedIO), _u8p, _u8p, C.c_int, _u32p, _ip]),
    "lutldpc_decoder_decode_batch_device": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int]),
    "lutldpc_decoder_decode_llr_batch": (C.c_int, [_vp, _dp, C.c_int, _dp, C.c_int, _dp, C.c_int, C.c_int, _ip, _u8p, _ip]),
    "lutldpc_decoder_stream": (_vp, [_vp]),
    "lutldpc_decoder_set_profiling": (C.c_int, [_vp, C.c_int]),
    "lutldpc_decoder_get_profile": (C.c_int, [_vp, C.c_int, _dp, C.POINTER(C.c_int64)]),
    "lutldpc_decoder_reset_profile": (C.c_int, [_vp]),
    "lutldpc_decoder_device_bytes": (C.c_int64, [_vp]),
    "lutldpc_decoder_describe": (_cp, [_vp]),
    "lutldpc_selftest_program_eval": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _ip, C.c_int, _ip, C.c_int]),
    "lutldpc_selftest_program_stats": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _ip, _ip, _ip]),
    "lutldpc_decoder_decode_batch_trace": (C.c_int, [_vp, _u8p, _u8p, C.c_int, C.c_int, _u8p, _ip, _u8p, C.c_int64, _ip]),
    "lutldpc_selftest_jit_source": (C.c_int64, [_vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int64, C.c_int]),
    "lutldpc_selftest_resident_source": (C.c_int64, [_vp, C.c_int, C.c_char_p, C.c_int64, C.c_int, C.POINTER(C.c_int32)]),
    "lutldpc_check_stream": (C.c_int, [C.c_uint32]),
    "lutldpc_decoder_set_generator": (C.c_int, [_vp, C.c_int, C.c_int, _u64p]),
    "lutldpc_decoder_set_sparse_generator": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _ip]),
    "lutldpc_decoder_encode_random": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, _u8p]),
    "lutldpc_decoder_sim_batch": (C.c_int, [_vp, _ccp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, _u8p, C.c_int, _ip, _u8p, _u8p]),
    "lutldpc_decoder_sample_labels": (C.c_int, [_vp, _ccp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, _u8p, _u8p, _u8p]),
    "lutldpc_decoder_sim_batch_random": (C.c_int, [_vp, _ccp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int, _ip, _u8p, _u8p]),
    "lutldpc_decoder_set_node_channels": (C.c_int, [_vp, C.POINTER(NodeChannels)]),
    "lutldpc_decoder_set_edge_groups": (C.c_int, [_vp, _ip, C.c_int]),
    "lutldpc_decoder_histogram_shape": (C.c_int, [_vp, C.c_int, _ip]),
    "lutldpc_decoder_histogram_batch": (C.c_int, [_vp, _u8p, _u8p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, _u8p, _ip, _i64p, C.c_int64, _ip]),
    "lutldpc_decoder_sim_batch_histogram": (C.c_int, [_vp, _ccp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, _u8p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                      _i64p, C.c_int64, _ip]),
    "lutldpc_decoder_events_batch": (C.c_int, [_vp, _u8p, _u8p, _u8p, C.c_int, C.c_int, _u8p, _ip, _evp]),
    "lutldpc_decoder_sim_batch_events": (C.c_int, [_vp, _ccp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, _u8p, C.c_int, C.c_int, _ip, _evp]),
    # ---- host mirror (include/lut_ldpc_host.h)
    "lutldpc_codec_create": (C.c_int, [_cp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "lutldpc_codec_load": (C.c_int, [_cp, C.c_int, C.POINTER(_vp)]),
    "lutldpc_codec_save": (C.c_int, [_vp, _cp]),
    "lutldpc_codec_destroy": (C.c_int, [_vp]),
    "lutldpc_codec_design_luts": (C.c_int, [_vp, _cp, C.c_int, C.c_double, C.c_int, _u8p, C.c_int, _ip, C.c_int, _dp]),
    "lutldpc_codec_design_from_cache": (C.c_int, [_vp]),
    "lutldpc_codec_set_exit_conditions": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
    "lutldpc_codec_set_initial_message_mode": (C.c_int, [_vp, C.c_int]),
    "lutldpc_codec_initial_message_mode": (C.c_int, [_vp]),
    "lutldpc_codec_set_output_verbosity": (C.c_int, [_vp, C.c_int]),
    "lutldpc_codec_dims": (C.c_int, [_vp, _ip, _ip, _ip, _ip]),
    "lutldpc_codec_graph": (C.c_int, [_vp, _ip, _ip, _ip]),
    "lutldpc_codec_var_trees_txt": (C.c_int64, [_vp, C.c_char_p, C.c_int64]),
    "lutldpc_codec_chk_trees_txt": (C.c_int64, [_vp, C.c_char_p, C.c_int64]),
    "lutldpc_codec_qb": (C.c_int, [_vp, C.c_int, _dp, C.c_int]),
    "lutldpc_codec_cha2msg_map": (C.c_int, [_vp, _ip, C.c_int]),
    "lutldpc_codec_rate": (C.c_double, [_vp]),
    "lutldpc_codec_decoder": (_vp, [_vp]),
    "lutldpc_codec_decode_llr_batch": (C.c_int, [_vp, _dp, C.c_int, _u8p, _ip]),
    "lutldpc_codec_lut_decode_batch": (C.c_int, [_vp, _u8p, _u8p, C.c_int, _u8p, _ip]),
    "lutldpc_codec_lut_decode_dump": (C.c_int64, [_vp, _u8p, _u8p, C.c_int, C.c_int, _u8p, _ip, C.c_char_p, C.c_int64]),
    "lutldpc_codec_encode": (C.c_int, [_vp, _u8p, _u8p]),
    "lutldpc_de_threshold": (C.c_int, [_ip, _dp, C.c_int, _ip, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _cp, _cp, C.c_double,
                                       C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, _dp]),
    "lutldpc_codec_sim_batch": (C.c_int, [_vp, C.c_double, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int, _ip]),
    "lutldpc_codec_sample_labels": (C.c_int, [_vp, C.c_double, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int, _u8p, _u8p, _u8p]),
    "lutldpc_codec_encode_random": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, _u8p]),
    "lutldpc_codec_channel_cells": (C.c_int, [_vp, C.c_double, _u64p, _u8p, _u8p, _u8p, _u8p, _u8p]),
    "lutldpc_codec_set_node_channels": (C.c_int, [_vp, _u8p, C.c_int, _dp]),
    "lutldpc_codec_node_channel_cells": (C.c_int, [_vp, C.c_double, C.c_int, _u64p, _u8p, _u8p, _u8p, _u8p, _u8p]),
    "lutldpc_ber_sim_run": (C.c_int, [_cp, _cp, C.c_int, _cp, C.c_int, C.c_int, C.c_int, _dp, _i64p, C.c_int]),
    "lutldpc_ber_sim_main": (C.c_int, [C.c_int, C.POINTER(C.c_char_p)]),
    "lutldpc_selftest_write_results_it": (C.c_int, [_cp, _dp, _i64p, C.c_int, C.c_int, C.c_int, C.c_double]),
    "lutldpc_bersim_create": (C.c_int, [_cp, _cp, C.c_int, _cp, C.c_int, C.POINTER(_vp)]),
    "lutldpc_bersim_destroy": (C.c_int, [_vp]),
    "lutldpc_bersim_info": (C.c_int, [_vp, _i64p, _dp, _dp, C.c_int]),
    "lutldpc_bersim_batch": (C.c_int, [_vp, C.c_int, C.c_int64, C.c_int, _ip]),
    "lutldpc_bersim_add_point": (C.c_int, [_vp, C.c_double, _i64p]),
    "lutldpc_bersim_save": (C.c_int, [_vp, C.c_double]),
    "lutldpc_bersim_results_path": (C.c_int64, [_vp, C.c_char_p, C.c_int64]),
    "lutldpc_codec_message_histogram": (C.c_int, [_vp, C.c_double, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  _i64p, C.c_int64, _ip]),
    "lutldpc_bersim_message_histogram": (C.c_int, [_vp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _i64p, C.c_int64, _ip]),
    "lutldpc_codec_error_events": (C.c_int, [_vp, C.c_double, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int, _evp]),
    "lutldpc_bersim_error_events": (C.c_int, [_vp, C.c_int, C.c_int64, C.c_int, _evp]),
    "lutldpc_bersim_decoder": (_vp, [_vp]),
    "lutldpc_bersim_code": (C.c_int, [_vp, _ip, _ip, _ip, _ip, _ip]),
    # ---- [BP] comparison decoder (include/lut_ldpc_bp.h)
    "lutldpc_bp_create": (C.c_int, [C.c_int, C.c_int, _ip, _ip, _ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "lutldpc_bp_destroy": (C.c_int, [_vp]),
    "lutldpc_bp_set_exit_conditions": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
    "lutldpc_bp_logexp_table": (C.c_int, [_vp, _ip, C.c_int]),
    "lutldpc_bp_decode_llr_batch": (C.c_int, [_vp, _dp, C.c_int, _u8p, _ip, _ip]),
    "lutldpc_bp_decode_qllr_batch": (C.c_int, [_vp, _ip, C.c_int, _u8p, _ip, _ip]),
    "lutldpc_bp_awgn_cells": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_int, _ip, _u64p, _ip, _u8p]),
    "lutldpc_bp_set_cells": (C.c_int, [_vp, C.POINTER(BPCells)]),
    "lutldpc_bp_sample_qllr": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, _u8p, _ip, _ip]),
    "lutldpc_bp_sim_batch": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, _u8p, C.c_int, _ip, _ip, _u8p]),
    "lutldpc_awgn_llr": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_double, _u8p, _dp, _ip]),
}
for _name, (_res, _args) in _SIGNATURES.items():
    if hasattr(lib, _name):          # (a library selected with LUTLDPC_LIB may be an older build that lacks an entry)
        _fn = getattr(lib, _name)
        _fn.restype, _fn.argtypes = _res, _args


def last_error() -> str:
    return lib.lutldpc_last_error().decode()


def check(rc: int) -> None:
    if rc != OK:
        raise LutLdpcError(rc, last_error())


def device_count() -> int:
    return lib.lutldpc_device_count()
