"""Shared case data of the soft-value entry (lutldpc_decoder_decode_llr_packed): tests/test_llr_input_cpu.py and
tests/test_57_llr_input_gpu.py.  No GPU is touched here.

Codes and frame groups as tests/test_56_packed_io_gpu.py uses them: 16-label alphabets in nibble rows (reg36_n1000_q4), 32-label
alphabets in byte rows (reg36_n1000_q5: 31 + 31 boundaries) and the two odd-N codes of frontend_cases.py (N = 33: its float16
frames start on odd halfword pairs, its int8 stride is 33).  One batch of tile + 1 frames per code; smaller batches are prefixes.

Values: LLRs of the all-zero codeword over BPSK/AWGN, even frames at the high and odd frames at the low SNR of the code, frame 0
at twice the largest boundary (noise-free).  On such values float32 changes no label against float64, so a wrongly rounded
boundary only shows on PLANTED values: the frames from 3 on hold, for every boundary b of both lists, the largest value of the type
that is <= b, its two neighbours in the type and b itself where representable, plus +-0, +-inf, NaN, the smallest denormal and the
largest finite value (int8: all 256 values).  The reference for labels is always the oracle's quant_nonlin of the values widened
to float64 (int8: q * scale in float64), the reference for a decode the oracle's decode of those labels."""
import functools
import zlib

import numpy as np

import frontend_cases as fc
from helpers import awgn_labels, oracle_codec
from oracle import oracle as orc

# name -> frames per group, (low, high) SNR in dB of the odd / even frames (the values of test_56's CASES)
CASES = {
    "nib_q4": dict(tile=512, snr=(1.0, 3.0)),
    "byte_q5": dict(tile=256, snr=(1.0, 3.5)),
    "n127": dict(tile=512, snr=(1.0, 5.0)),
    "n33": dict(tile=512, snr=(1.0, 5.0)),
}
EXITS = [(True, False), (True, True), (False, False)]      # psc, psc + pisc, none
DTYPES = {"f64": np.float64, "f32": np.float32, "f16": np.float16, "i8": np.int8}
PLANT_FIRST = 3

# boundaries a designer would not choose, passed as arguments: values not representable in float32 / float16, a pair that rounds
# to the same value in both, +-1e-50 (below every denormal), 65504.5 (just above the largest half), +-1e39 (beyond float32), +inf
AWKWARD = np.array([-1e39, -70000.0, -65504.5, -3.3, -1.0 - 2.0 ** -30, -1.0 - 2.0 ** -31, -1e-50, 1e-50, 0.1, 1.0 / 3.0, 2.7,
                    1000.0625, 65504.5, 1e39, np.inf])      # 15 = Nq - 1 of a 16-label alphabet
AWKWARD_MAP = (np.arange(16, dtype=np.int32) * 7) % 16


@functools.lru_cache(maxsize=None)
def codec(name):
    if name == "nib_q4":
        return oracle_codec("reg36_n1000_q4")
    if name == "byte_q5":
        return oracle_codec("reg36_n1000_q5")
    return fc.codec(name)


@functools.lru_cache(maxsize=None)
def quantiser(name):
    """(qb_cha, qb_msg, cha2msg_map) of the code's design."""
    cd = codec(name)
    cd.set_initial_message_mode(1)
    mp = cd.cha2msg_map.copy()
    cd.set_initial_message_mode(0)
    return cd.qb_cha.copy(), cd.qb_msg.copy(), mp


def batches(name):
    T = CASES[name]["tile"]
    return (1, T - 1, T, T + 1)


def round_down(b, T):
    """The largest value of the float type T that is <= b (numpy's own rounding, then one step down where that went up)."""
    with np.errstate(over="ignore"):
        t = np.asarray(b, np.float64).astype(T)
        up = t.astype(np.float64) > np.asarray(b, np.float64)
        return np.where(up, np.nextafter(t, T(-np.inf)), t).astype(T)


def planted(bounds, T):
    """Planted values of the float type T for the boundaries `bounds` (any number of lists, concatenated)."""
    b = np.concatenate([np.asarray(x, np.float64) for x in bounds])
    bt = round_down(b, T)
    fi = np.finfo(T)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fi.smallest_subnormal, -fi.smallest_subnormal, fi.max, -fi.max], T)
    with np.errstate(over="ignore"):
        exact = b.astype(T)[b.astype(T).astype(np.float64) == b]
        return np.concatenate([bt, np.nextafter(bt, T(np.inf)), np.nextafter(bt, T(-np.inf)), exact, special]).astype(T)


def i8_scale(bounds):
    return float(np.float32(1.25 * max(np.abs(np.asarray(x)[np.isfinite(x)]).max() for x in bounds) / 127.0))


def plant(x, vals):
    """Frames PLANT_FIRST .. of x filled with vals, repeated to whole frames; returns the number of planted frames."""
    N = x.shape[1]
    k = min(max(3, -(-len(vals) // N)), x.shape[0] - PLANT_FIRST)
    x[PLANT_FIRST:PLANT_FIRST + k] = np.resize(vals, k * N).reshape(k, N)
    return k


@functools.lru_cache(maxsize=None)
def base_values(name):
    cd = codec(name)
    T, (lo, hi) = CASES[name]["tile"], CASES[name]["snr"]
    llr = awgn_labels(cd, T + 1, hi, seed=5701)[2].copy()
    llr[1::2] = awgn_labels(cd, T + 1, lo, seed=5801)[2][1::2]
    qc, qm, _ = quantiser(name)
    llr[0] = 2.0 * max(qc.max(), qm.max())
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def values(name, dt):
    """(x [tile + 1, N] of the dtype, scale or None, the same values as float64)."""
    qc, qm, _ = quantiser(name)
    llr = base_values(name)
    T = DTYPES[dt]
    if dt == "i8":
        scale = i8_scale((qc, qm))
        x = np.clip(np.rint(llr / scale), -128, 127).astype(np.int8)
        plant(x, np.arange(-128, 128).astype(np.int8))
        wide = x.astype(np.float64) * scale
    else:
        scale = None
        x = llr.astype(T)
        plant(x, planted((qc, qm), T))
        wide = x.astype(np.float64)
    x.setflags(write=False)
    wide.setflags(write=False)
    return x, scale, wide


def ref_labels(wide, qb_cha, qb_msg, cha2msg_map, mode):
    cha = orc.quant_nonlin(wide, qb_cha)
    msg = orc.quant_nonlin(wide, qb_msg) if mode == 0 else np.asarray(cha2msg_map)[cha].astype(np.uint8)
    return cha, msg


@functools.lru_cache(maxsize=None)
def want_labels(name, dt, mode):
    qc, qm, mp = quantiser(name)
    cha, msg = ref_labels(values(name, dt)[2], qc, qm, mp, mode)
    cha.setflags(write=False)
    msg.setflags(write=False)
    return cha, msg


_decoded = {}


def want(name, dt, mode, psc, pisc):
    """The oracle's decode of the whole batch of reference labels, once per distinct label set (float64 and float32 share theirs
    wherever the planted frames quantise alike); a smaller batch is a prefix (frames are independent)."""
    cd = codec(name)
    cha, msg = want_labels(name, dt, mode)
    key = (name, psc, pisc, zlib.crc32(cha), zlib.crc32(msg))
    if key not in _decoded:
        cd.set_exit_conditions(cd.max_iters, psc, pisc)
        bits, it = cd.lut_decode_batch_flat(cha, msg)
        bits.setflags(write=False)
        it.setflags(write=False)
        _decoded[key] = (bits, it)
    return _decoded[key]


def check_mix(name, it, pisc, B):
    """Converging and non-converging frames in the batch, from the oracle's iteration codes alone."""
    if B > 1:
        assert (it > 0).any() and (it < 0).any(), (name, B, sorted(set(it.tolist())))
        if pisc:
            assert it[0] == 0
