"""lutldpc_decoder_decode_batch_packed on the device: packed labels in (one or two per byte, the initial messages given or derived
from the channel labels through cha2msg_map on the device), a window of the decided bits out (one bit each), against the oracle's
decode of the same frames and against lut_decode_batch on the same handle.  Everything is integer: equal bit for bit.

Codes (existing fixtures and writers): 16-label alphabets in nibble rows (reg36_n1000_q4), 32-label alphabets in byte rows
(reg36_n1000_q5), a 6-label channel alphabet whose nibbles and bytes also carry labels 6..15 (clamped to 5 before the map; given
initial messages above 7 clamped to 7), and the two odd-N codes of frontend_cases.py (N = 127: frame stride 64 bytes, dword loads;
N = 33: stride 17, byte loads; both with a spare nibble, filled with ones here).
Batches 1, tile - 1, tile, tile + 1 frames (tile = 256 frames in byte rows, 512 in nibble rows): prefixes of one batch per code
whose even frames are sampled at a high and whose odd frames at a low SNR, frame 0 noise-free; that every batch of more than one
frame holds converging and non-converging frames is checked on the oracle's result alone.  A batch of one frame cannot hold both."""
import ctypes as C
import functools

import numpy as np
import pytest

import lut_ldpc_amd as L
from lut_ldpc_amd import packing
from lut_ldpc_amd._capi import IN_BYTES, IN_NIBBLES, PackedIO, check, lib

import frontend_cases as fc
from helpers import CODES as CODE_DIR, PACKED_PATHS as PATHS, awgn_labels, designed_codec, oracle_codec, product_decoder

pytestmark = pytest.mark.gpu

u8p, i32p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)

# name -> frames per group, (low, high) SNR in dB of the odd / even frames, whether the labels fit a nibble
CASES = {
    "nib_q4": dict(tile=512, snr=(1.0, 3.0), nibbles=True),
    "byte_q5": dict(tile=256, snr=(1.0, 3.5), nibbles=False),
    "six": dict(tile=512, snr=(2.0, 4.0), nibbles=True),
    "n127": dict(tile=512, snr=(1.0, 5.0), nibbles=True),
    "n33": dict(tile=512, snr=(1.0, 5.0), nibbles=True),
}
EXITS = [(True, False), (True, True), (False, False)]      # psc, psc + pisc, none


@functools.lru_cache(maxsize=None)
def codec(name):
    if name == "nib_q4":
        return oracle_codec("reg36_n1000_q4")
    if name == "byte_q5":
        return oracle_codec("reg36_n1000_q5")
    if name in ("n127", "n33"):
        return fc.codec(name)
    # "six": 6 channel labels, 8 message labels
    return designed_codec("test56-six", CODE_DIR / "rate0.50_dv03_dc06_N1000.alist", sigma=0.8, max_iters=8, nq_msg=8, nq_cha=6)


def batches(name):
    T = CASES[name]["tile"]
    return (1, T - 1, T, T + 1)


def windows(name):
    cd = codec(name)
    N, K = cd.code.nvar, cd.code.nvar - cd.code.nchk
    return list(dict.fromkeys([(0, N), (0, K), (0, 1), (0, 31), (0, 32), (0, 33), (1, 32), (N - 33, 33)]))


@functools.lru_cache(maxsize=None)
def labels(name, mode):
    """tile + 1 frames.  mode 1: the initial messages are cha2msg_map of the channel labels (sent as the map); mode 0: quantised
    from the continuous input (sent as msg0).  Returns (cha, msg) as the caller sends them and (cha, msg) as the decoder must
    understand them: equal except for "six", where labels outside the alphabets are planted."""
    cd = codec(name)
    T, (lo, hi) = CASES[name]["tile"], CASES[name]["snr"]
    cd.set_initial_message_mode(mode)
    a = awgn_labels(cd, T + 1, hi, seed=5600 + mode, mode=mode)
    b = awgn_labels(cd, T + 1, lo, seed=5700 + mode, mode=mode)
    cd.set_initial_message_mode(0)
    cha, msg = a[0].copy(), a[1].copy()
    cha[1::2], msg[1::2] = b[0][1::2], b[1][1::2]
    cha[0] = cd.nq_cha - 1                                   # noise-free: passes the test on the channel decisions
    msg[0] = cd.nq_msg[0] - 1 if mode == 0 else cd.cha2msg_map[cd.nq_cha - 1]
    sent_cha, sent_msg = cha.copy(), msg.copy()
    if name == "six":
        rng = np.random.default_rng(56 + mode)
        hit = rng.random(cha.shape) < 0.05
        hit[0] = False
        sent_cha[hit] = rng.integers(cd.nq_cha, 16, int(hit.sum()))
        cha[hit] = cd.nq_cha - 1
        if mode == 1:
            msg = cd.cha2msg_map[cha].astype(np.uint8)
            sent_msg = msg.copy()
        else:
            hit = rng.random(msg.shape) < 0.05
            hit[0] = False
            sent_msg[hit] = rng.integers(cd.nq_msg[0], 16, int(hit.sum()))
            msg[hit] = cd.nq_msg[0] - 1
        assert (sent_cha >= cd.nq_cha).sum() > 100 and sent_cha.max() == 15
    if mode == 1:
        assert (msg == cd.cha2msg_map[cha]).all()
    for x in (sent_cha, sent_msg, cha, msg):
        x.setflags(write=False)
    return sent_cha, sent_msg, cha, msg


@functools.lru_cache(maxsize=None)
def want(name, mode, psc, pisc):
    """The oracle's decode of the whole batch, once for every test; a smaller batch is a prefix (frames are independent)."""
    cd = codec(name)
    _, _, cha, msg = labels(name, mode)
    cd.set_exit_conditions(cd.max_iters, psc, pisc)
    bits, it = cd.lut_decode_batch_flat(cha, msg)
    bits.setflags(write=False)
    it.setflags(write=False)
    return bits, it


def check_mix(name, it, psc, pisc, B):
    """Converging and non-converging frames in the batch, from the oracle's iteration codes alone."""
    if B > 1:
        assert (it > 0).any() and (it < 0).any(), (name, B, sorted(set(it.tolist())))
        if pisc:
            assert it[0] == 0


def send(name, arr, nib):
    """A label array in the input format; the spare nibble of an odd N filled with ones (it must be ignored)."""
    if not nib:
        return arr
    pk = packing.pack_nibbles(arr)
    if arr.shape[1] % 2:
        pk[:, -1] |= 0xF0
    return pk


def decode(dec, name, mode, nib, B, first, count):
    cd = codec(name)
    sent_cha, sent_msg, _, _ = labels(name, mode)
    if mode == 1:
        return dec.decode_packed(send(name, sent_cha[:B], nib), cha2msg_map=cd.cha2msg_map, nibbles=nib, first=first, count=count)
    return dec.decode_packed(send(name, sent_cha[:B], nib), msg0=send(name, sent_msg[:B], nib), nibbles=nib, first=first, count=count)


def assert_window(words, it, want_bits, want_it, first, count, tag):
    assert words.dtype == np.uint32 and words.shape == (len(want_it), (count + 31) // 32), tag
    assert (it == want_it).all(), (tag, np.flatnonzero(it != want_it)[:8])
    got = packing.unpack_bits(words, count)
    bad = np.argwhere(got != want_bits[:, first:first + count])
    assert bad.size == 0, (tag, f"{len(bad)} bit mismatches, first at frame/bit {bad[:4].tolist()}")
    if count % 32:                                           # bits beyond the window are 0
        assert (words[:, -1] >> np.uint32(count % 32) == 0).all(), tag


def run_case(dec, name, B, variants_of_window=1):
    """Every exit mode: all input variants on the full window, lut_decode_batch on the same handle, then every window."""
    cd = codec(name)
    N = cd.code.nvar
    formats = (False, True) if CASES[name]["nibbles"] else (False,)
    variants = [(mode, nib) for mode in (1, 0) for nib in formats]
    for psc, pisc in EXITS:
        dec.set_exit_conditions(cd.max_iters, psc, pisc)
        for mode in (1, 0):
            wb, wi = want(name, mode, psc, pisc)
            wb, wi = wb[:B], wi[:B]
            check_mix(name, wi, psc, pisc, B)
            sent_cha, sent_msg, _, _ = labels(name, mode)
            bits, it = dec.lut_decode_batch(sent_cha[:B], sent_msg[:B])          # the byte entry of the same handle
            assert (it == wi).all() and (bits == wb).all(), (name, B, mode, psc, pisc)
            for nib in formats:
                words, it = decode(dec, name, mode, nib, B, 0, N)
                assert_window(words, it, wb, wi, 0, N, (name, B, mode, nib, psc, pisc))
                assert (packing.unpack_bits(words, N) == bits).all()
        for k, (first, count) in enumerate(windows(name)):
            for mode, nib in [variants[(k + j) % len(variants)] for j in range(variants_of_window)]:
                wb, wi = want(name, mode, psc, pisc)
                words, it = decode(dec, name, mode, nib, B, first, count)
                assert_window(words, it, wb[:B], wi[:B], first, count, (name, B, mode, nib, psc, pisc, first, count))


@pytest.mark.parametrize("name,B", [(n, B) for n in CASES for B in batches(n)])
def test_packed_decode_matches_oracle_and_the_byte_entry(name, B):
    cd = codec(name)
    dec = product_decoder(cd)
    desc = dec.describe()
    assert desc["tile_frames"] == CASES[name]["tile"] and desc["pack"] == (2 if CASES[name]["tile"] == 512 else 1), desc
    run_case(dec, name, B)
    dec.close()


@pytest.mark.parametrize("path", list(PATHS))
def test_every_decode_path_behind_the_packed_entry(path, monkeypatch):
    env, expect = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    name = "nib_q4"
    dec = product_decoder(codec(name))
    desc = dec.describe()
    assert {k: desc[k] for k in expect} == expect, desc
    # two frame groups and a ragged third (nibble rows: one and a ragged second), twice: the second decode of a streaming path is
    # the captured graph
    for _ in range(2):
        run_case(dec, name, CASES[name]["tile"] + 1)
    dec.close()


@pytest.mark.parametrize("name,B", [("nib_q4", 513), ("byte_q5", 1), ("n33", 511)])
def test_canary_words_after_the_last_frame_stay(name, B):
    cd = codec(name)
    dec = product_decoder(cd)
    dec.set_exit_conditions(cd.max_iters, True, True)
    N = cd.code.nvar
    nib = CASES[name]["nibbles"]
    sent_cha, _, _, _ = labels(name, 1)
    wb, wi = want(name, 1, True, True)
    cha = np.ascontiguousarray(send(name, sent_cha[:B], nib))
    mp = np.ascontiguousarray(cd.cha2msg_map, np.int32)
    for first, count in ((0, N), (1, 32), (N - 33, 33)):
        W = (count + 31) // 32
        words = np.full((B + 3, W), 0xC0FFEE11, np.uint32)
        iters = np.full(B + 3, -12345, np.int32)
        io = PackedIO(IN_NIBBLES if nib else IN_BYTES, mp.ctypes.data_as(i32p), first, count)
        check(lib.lutldpc_decoder_decode_batch_packed(dec._h, C.byref(io), cha.ctypes.data_as(u8p), None, B, words.ctypes.data_as(u32p), iters.ctypes.data_as(i32p)))
        assert (words[B:] == 0xC0FFEE11).all() and (iters[B:] == -12345).all()
        assert_window(words[:B], iters[:B], wb[:B], wi[:B], first, count, (name, B, first, count))
        # only the iteration codes / only the bits
        iters2 = np.full(B + 3, -12345, np.int32)
        check(lib.lutldpc_decoder_decode_batch_packed(dec._h, C.byref(io), cha.ctypes.data_as(u8p), None, B, None, iters2.ctypes.data_as(i32p)))
        assert (iters2 == iters).all()
        words2 = np.full((B + 3, W), 0xC0FFEE11, np.uint32)
        check(lib.lutldpc_decoder_decode_batch_packed(dec._h, C.byref(io), cha.ctypes.data_as(u8p), None, B, words2.ctypes.data_as(u32p), None))
        assert (words2 == words).all()
    dec.close()


def test_codec_decode_packed_returns_the_data_bits():
    """Codec.decode_packed: map and K_info from the codec (mode QCHA), against the codec's own byte entry."""
    pcd = L.Codec(CODE_DIR / "rate0.50_dv02-17_dc08-09_lut_q4_N500.alist", device=0)
    pcd.design_luts(sigma2=0.88 ** 2, max_iters=8)
    pcd.set_exit_conditions(8, True, True)
    with pytest.raises(ValueError, match="QCHA"):
        pcd.decode_packed(np.zeros((1, pcd.nvar), np.uint8))
    pcd.set_initial_message_mode(1)
    cha, _, _ = pcd.sample_labels(2.0, 7, 1, 0, 600)
    bits, it = pcd.lut_decode_batch(cha, pcd.cha2msg_map[cha].astype(np.uint8))
    assert (it > 0).any() and (it < 0).any()
    K = pcd.ninfo
    for nib in (False, True):
        words, got_it = pcd.decode_packed(packing.pack_nibbles(cha) if nib else cha, nibbles=nib)
        assert words.shape == (600, (K + 31) // 32) and (got_it == it).all()
        assert (packing.unpack_bits(words, K) == bits[:, :K]).all()
        words, got_it = pcd.decode_packed(packing.pack_nibbles(cha) if nib else cha, nibbles=nib, info_only=False)
        assert (packing.unpack_bits(words, pcd.nvar) == bits).all() and (got_it == it).all()
    pcd.close()
