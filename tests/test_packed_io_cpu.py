"""Packed label input and bit-packed output without a GPU: the host-side formats of lut_ldpc_amd.packing, and the argument
contract of lutldpc_decoder_decode_batch_packed on a host-only handle -- every argument error answers ERR_ARG before the handle's
missing device answers ERR_STATE."""
import ctypes as C
import re

import numpy as np
import pytest

from lut_ldpc_amd import packing
from lut_ldpc_amd._capi import ERR_ARG, ERR_STATE, IN_BYTES, IN_NIBBLES, PackedIO, last_error, lib

from helpers import ROOT, oracle_codec, product_decoder

u8p, i32p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)


# ------------------------------------------------------------------------------------------------- formats
@pytest.mark.parametrize("N", [1, 2, 33, 127])
def test_nibble_round_trip_and_layout(N):
    rng = np.random.default_rng(N)
    lab = rng.integers(0, 16, (5, N), dtype=np.uint8)
    pk = packing.pack_nibbles(lab)
    assert pk.dtype == np.uint8 and pk.shape == (5, (N + 1) // 2)
    for v in range(N):                                       # node v in byte v // 2, even v in bits 0-3, odd v in bits 4-7
        assert ((pk[:, v // 2] >> (4 * (v & 1))) & 15 == lab[:, v]).all(), v
    if N % 2:
        assert (pk[:, -1] >> 4 == 0).all()                   # the spare nibble is written as 0 ...
        dirty = pk.copy()
        dirty[:, -1] |= 0xA0
        assert (packing.unpack_nibbles(dirty, N) == lab).all()     # ... and ignored whatever it holds
    back = packing.unpack_nibbles(pk, N)
    assert back.dtype == np.uint8 and back.shape == (5, N) and (back == lab).all()


def test_nibble_packing_refuses_what_does_not_fit():
    with pytest.raises(ValueError):
        packing.pack_nibbles(np.full((2, 4), 16, np.uint8))
    with pytest.raises(ValueError):
        packing.pack_nibbles(np.zeros(4, np.uint8))
    with pytest.raises(ValueError):
        packing.unpack_nibbles(np.zeros((2, 3), np.uint8), 8)


@pytest.mark.parametrize("count", [1, 31, 32, 33, 64, 100])
def test_unpack_bits_is_little_endian_bit_order(count):
    rng = np.random.default_rng(count)
    W = (count + 31) // 32
    words = rng.integers(0, 2 ** 32, (7, W), dtype=np.uint32)
    want = np.unpackbits(words.astype("<u4").view(np.uint8), axis=1, bitorder="little")[:, :count]
    got = packing.unpack_bits(words, count)
    assert got.dtype == np.uint8 and got.shape == (7, count) and (got == want).all()
    one = np.zeros((1, W), np.uint32)
    one[0, (count - 1) // 32] = np.uint32(1) << np.uint32((count - 1) % 32)
    assert packing.unpack_bits(one, count)[0].tolist() == [0] * (count - 1) + [1]
    with pytest.raises(ValueError):
        packing.unpack_bits(words, 32 * W + 1)


# ------------------------------------------------------------------------------------------------- argument contract
def _handle(name):
    cd = oracle_codec(name)
    dec = product_decoder(cd, device=-1)
    return cd, dec


@pytest.fixture(scope="module")
def q4():
    cd, dec = _handle("n500_q4_i8")                  # 16 / 16 labels
    yield cd, dec
    dec.close()


@pytest.fixture(scope="module")
def q5():
    cd, dec = _handle("reg36_n1000_q5")              # 32 / 32 labels: no nibbles
    yield cd, dec
    dec.close()


@pytest.fixture(scope="module")
def c32m8():
    cd, dec = _handle("reg36_n1000_c32m8")           # 32 channel labels, 8 message labels
    yield cd, dec
    dec.close()


class Call:
    """One call of the entry with valid defaults; keyword arguments replace single arguments."""
    B = 3

    def __init__(self, cd, dec):
        self.N = cd.code.nvar
        self.h = dec._h
        self.map = np.ascontiguousarray(np.minimum(np.arange(cd.nq_cha), int(cd.nq_msg[0]) - 1), np.int32)
        self.cha = np.zeros((self.B, self.N), np.uint8)
        self.words = np.full((self.B, (self.N + 31) // 32 + 1), 0xDEADBEEF, np.uint32)
        self.iters = np.full(self.B, -77, np.int32)

    def __call__(self, h="own", io="own", fmt=IN_BYTES, map="own", first=0, count=None, cha="own", msg0=None, B=None):
        mp = self.map if isinstance(map, str) else map
        pio = PackedIO(fmt, mp.ctypes.data_as(i32p) if mp is not None else None, first, self.N if count is None else count)
        rc = lib.lutldpc_decoder_decode_batch_packed(
            self.h if isinstance(h, str) else h, C.byref(pio) if isinstance(io, str) else io,
            self.cha.ctypes.data_as(u8p) if isinstance(cha, str) else cha,
            msg0.ctypes.data_as(u8p) if msg0 is not None else None, self.B if B is None else B,
            self.words.ctypes.data_as(u32p), self.iters.ctypes.data_as(i32p))
        assert (self.words == 0xDEADBEEF).all() and (self.iters == -77).all()          # no GPU: nothing may be written
        return rc


def test_argument_errors_come_before_the_state_error(q4):
    call = Call(*q4)
    N = call.N
    assert call() == ERR_STATE and "host-only handle" in last_error()                  # valid arguments: only the device is missing
    assert call(fmt=IN_NIBBLES) == ERR_STATE
    assert call(map=None, msg0=call.cha) == ERR_STATE                                  # msg0 in place of the map
    assert call(first=N - 1, count=1) == ERR_STATE and call(first=0, count=N) == ERR_STATE
    assert call(h=None) == ERR_ARG
    for B in (0, -1):
        assert call(B=B) == ERR_ARG, B
    assert call(io=None) == ERR_ARG
    assert call(cha=None) == ERR_ARG
    for fmt in (-1, 2, 7):
        assert call(fmt=fmt) == ERR_ARG, fmt
    assert call(map=None) == ERR_ARG                                                   # neither msg0 nor a map
    assert call(msg0=call.cha) == ERR_ARG                                              # both
    for i, bad in ((0, -1), (5, 16), (15, 1000)):                                      # a map entry outside [0, Nq_Msg[0])
        mp = call.map.copy()
        mp[i] = bad
        assert call(map=mp) == ERR_ARG, (i, bad)
        assert "cha2msg_map" in last_error()
    for first, count in ((-1, 4), (0, 0), (0, -3), (0, N + 1), (N, 1), (1, N), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert call(first=first, count=count) == ERR_ARG, (first, count)
    assert call() == ERR_STATE


def test_nibbles_need_alphabets_of_at_most_sixteen_labels(q5, c32m8):
    call = Call(*q5)
    assert call() == ERR_STATE and call(map=None, msg0=call.cha) == ERR_STATE          # bytes: fine
    assert call(fmt=IN_NIBBLES) == ERR_ARG                                             # 32 channel labels do not fit
    assert call(fmt=IN_NIBBLES, map=None, msg0=call.cha) == ERR_ARG
    call = Call(*c32m8)
    assert call(fmt=IN_NIBBLES) == ERR_ARG                                             # ... whatever the message alphabet


def test_nibbles_with_a_wide_message_alphabet_need_the_map():
    """16 channel labels, 32 message labels in iteration 0: the channel labels fit a nibble, given initial messages do not."""
    import lut_ldpc_amd as L
    from helpers import CODES
    pcd = L.Codec(CODES / "rate0.50_dv03_dc06_N1000.alist", device=-1)
    pcd.design_luts(sigma2=0.84 ** 2, max_iters=3, nq_cha=16, nq_msg=[32, 32, 32])
    dec = pcd.decoder()
    N, B = pcd.nvar, 2
    mp = np.ascontiguousarray(pcd.cha2msg_map, np.int32)
    assert len(mp) == 16 and mp.max() < 32
    pk = np.zeros((B, N // 2), np.uint8)

    def call(map, msg0):
        pio = PackedIO(IN_NIBBLES, map.ctypes.data_as(i32p) if map is not None else None, 0, N)
        return lib.lutldpc_decoder_decode_batch_packed(dec._h, C.byref(pio), pk.ctypes.data_as(u8p), msg0.ctypes.data_as(u8p) if msg0 is not None else None,
                                                       B, None, None)
    assert call(mp, None) == ERR_STATE
    assert call(None, pk) == ERR_ARG and "16 labels" in last_error()
    pcd.close()


def test_python_methods_pass_the_contract_on():
    import lut_ldpc_amd as L
    from helpers import CODES
    pcd = L.Codec(CODES / "rate0.50_dv02-17_dc08-09_lut_q4_N500.alist", device=-1)
    pcd.design_luts(sigma2=0.88 ** 2, max_iters=2)
    cha = np.zeros((2, pcd.nvar), np.uint8)
    with pytest.raises(ValueError, match="QCHA"):                                      # continuous-input messages: the map is not the message
        pcd.decode_packed(cha)
    pcd.set_initial_message_mode(1)
    assert lib.lutldpc_codec_initial_message_mode(pcd._h) == 1
    for nib in (False, True):
        with pytest.raises(L.LutLdpcError, match="host-only handle"):
            pcd.decode_packed(packing.pack_nibbles(cha) if nib else cha, nibbles=nib)
    dec = pcd.decoder()
    with pytest.raises(ValueError):
        dec.decode_packed(cha, cha2msg_map=pcd.cha2msg_map, nibbles=True)              # [B, nvar] is not the packed shape
    with pytest.raises(L.LutLdpcError, match="output window"):
        dec.decode_packed(cha, cha2msg_map=pcd.cha2msg_map, first=1, count=pcd.nvar)
    pcd.close()


def test_symbol_and_constants_are_in_the_header():
    assert hasattr(lib, "lutldpc_decoder_decode_batch_packed")
    text = (ROOT / "include" / "lut_ldpc_hip.h").read_text()
    assert re.search(r"#define\s+LUTLDPC_IN_BYTES\s+0\b", text) and re.search(r"#define\s+LUTLDPC_IN_NIBBLES\s+1\b", text)
    assert re.search(r"#define\s+LUTLDPC_K_COUNT\s+9\b", text)                         # no new kernel kind: both kernels count as layout
    assert (IN_BYTES, IN_NIBBLES) == (0, 1)
