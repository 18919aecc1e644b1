"""lutldpc_decoder_encode_packed without a GPU: the symbol and its binding, the order of its refusals on a host-only handle (argument
errors before the one state error of the batch guard), packing.pack_bits against the documented bit order, and the cases of
tests/encode_cases.py held to what they claim with the references alone -- every synthetic case sets information and parity bits,
the windows cover information-only, straddling and parity-only words, the batches sit on both sides of the 64-frame workgroup,
the real codes' reference codewords satisfy H c = 0 by the oracle, and the +-L labels of the loop-back decode to the sent words at
the first exit test by the oracle, so that the GPU loop-back tests the product and not the choice of L."""
import ctypes as C
import re

import numpy as np
import pytest

import encode_cases as ec
from helpers import CONFIGS, ROOT, oracle_codec, product_decoder
from lut_ldpc_amd import _capi, packing
from lut_ldpc_amd._capi import ERR_ARG, ERR_STATE, EncodeIO, last_error, lib

B0, W0 = 3, 16                                   # n500: any K <= 500 fits 16 words


def test_symbol_is_declared_exported_and_bound():
    header = (ROOT / "include" / "lut_ldpc_hip.h").read_text()
    assert re.search(r"int lutldpc_decoder_encode_packed\(lutldpc_decoder \*d, const lutldpc_encode_io \*io, const uint32_t \*info, int B, uint32_t \*out_words\);", header)
    assert "} lutldpc_encode_io;" in header
    fn = lib.lutldpc_decoder_encode_packed                         # (AttributeError if the library does not export it)
    assert "lutldpc_decoder_encode_packed" in _capi._SIGNATURES and fn.restype is C.c_int and len(fn.argtypes) == 5
    assert [f[0] for f in EncodeIO._fields_] == ["on_device", "in_stride", "out_first", "out_count", "sync"]
    assert C.sizeof(EncodeIO) == 32 and EncodeIO.in_stride.offset == 8 and EncodeIO.out_first.offset == 16 and EncodeIO.sync.offset == 24


@pytest.fixture(scope="module")
def host_only():
    cd = oracle_codec("n500_q4_i8")
    dec = product_decoder(cd, device=-1)
    yield dec
    dec.close()


def _call(h, io, info, B, out, info_off=0, out_off=0):
    return lib.lutldpc_decoder_encode_packed(h, C.byref(io) if io is not None else None, C.c_void_p(info.ctypes.data + info_off) if info is not None else None, B,
                                             C.c_void_p(out.ctypes.data + out_off) if out is not None else None)


def test_refusals_on_a_host_only_handle_arguments_before_state(host_only):
    h, N = host_only._h, host_only.nvar
    info = np.zeros((B0, W0 + 1), np.uint32)
    out = np.full((B0, (N + 31) // 32 + 1), 0xEEEEEEEE, np.uint32)
    good = lambda **kw: EncodeIO(**{**dict(on_device=0, in_stride=W0, out_first=0, out_count=N, sync=0), **kw})
    assert _call(None, good(), info, B0, out) == ERR_ARG                            # NULL handle
    for B in (0, -1):
        assert _call(h, good(), info, B, out) == ERR_ARG, B                         # host-only handle AND a bad batch: the argument error wins
    bad = {
        "NULL io": lambda: _call(h, None, info, B0, out),
        "NULL info": lambda: _call(h, good(), None, B0, out),
        "NULL out_words": lambda: _call(h, good(), info, B0, None),
        "info off by 2 bytes": lambda: _call(h, good(), info, B0, out, info_off=2),
        "out_words off by 1 byte": lambda: _call(h, good(), info, B0, out, out_off=1),
        "negative in_stride": lambda: _call(h, good(in_stride=-1), info, B0, out),
        "out_first < 0": lambda: _call(h, good(out_first=-1, out_count=5), info, B0, out),
        "out_count < 1": lambda: _call(h, good(out_count=0), info, B0, out),
        "window past nvar": lambda: _call(h, good(out_first=1, out_count=N), info, B0, out),
        "window sum overflows int32": lambda: _call(h, good(out_first=2 ** 31 - 1, out_count=2 ** 31 - 1), info, B0, out),
    }
    for name, call in bad.items():
        assert call() == ERR_ARG, name
        assert "host-only" not in last_error(), name
    for io in (good(), good(in_stride=0), good(on_device=1, sync=1), good(out_first=N - 1, out_count=1)):
        assert _call(h, io, info, B0, out) == ERR_STATE                             # valid arguments: the handle has no device
        assert "host-only handle" in last_error()
    assert _call(h, good(), info, B0, out, info_off=4, out_off=4) == ERR_STATE      # 4-byte alignment is all that is asked
    assert (out == 0xEEEEEEEE).all() and not info.any()
    with pytest.raises(_capi.LutLdpcError, match="host-only handle"):
        host_only.encode_packed(info)
    for wrong in (np.zeros((B0, W0), np.uint8), np.zeros(W0, np.uint32), np.zeros((B0, W0), np.float32), [[0] * W0]):
        with pytest.raises(ValueError):
            host_only.encode_packed(wrong)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000])
def test_pack_bits_is_the_inverse_of_unpack_bits_in_the_documented_order(n):
    bits = np.random.default_rng(n).integers(0, 2, (5, n), dtype=np.uint8)
    bits[0], bits[1] = 0, 1
    words = packing.pack_bits(bits)
    assert words.dtype == np.uint32 and words.shape == (5, (n + 31) // 32)
    # the documented order, bit by bit: bit j of word w = bit 32w + j, spare bits 0
    want = np.zeros_like(words)
    for k in range(n):
        want[:, k // 32] |= bits[:, k].astype(np.uint32) << np.uint32(k % 32)
    assert (words == want).all() and (words == ec.pack(bits)).all()
    assert (packing.unpack_bits(words, n) == bits).all() and (ec.unpack(words, n) == bits).all()
    assert (packing.pack_bits(packing.unpack_bits(words, n)) == words).all()
    with pytest.raises(ValueError):
        packing.pack_bits(bits + 1)
    with pytest.raises(ValueError):
        packing.pack_bits(bits[0])


def test_case_lists_hold_what_they_claim():
    assert {h for h, _, _ in ec.SYNTH_CASES} == {"q4", "q4_pack1", "n127", "n10000"}
    for h in ("q4", "q4_pack1"):
        assert [K for hh, K, _ in ec.SYNTH_CASES if hh == h] == [1, 31, 32, 33, 127, 128, 129, 500, 968, 999, 1000]
    assert ("n127", 64, 63) in ec.SYNTH_CASES and ("n10000", 8192, 1808) in ec.SYNTH_CASES and ("q4", 1000, 0) in ec.SYNTH_CASES
    # the batch sizes sit on both sides of the 64-frame workgroup, and on it
    assert min(ec.BATCHES) == 1 and 63 in ec.BATCHES and 64 in ec.BATCHES and 65 in ec.BATCHES and max(ec.BATCHES) > 128 and max(ec.BATCHES) % 64
    for h, K, R in ec.SYNTH_CASES:
        N = K + R
        code = ec.fc.HANDLES[h][0]                   # the handle's code length: the synthetic code's node count, or the N of the alist's name
        assert N == (sum(ec.fc.SYNTHETIC[code][0].values()) if code in ec.fc.SYNTHETIC else int(CONFIGS[code][0].rsplit("_N", 1)[1]))
        W = (K + 31) // 32
        assert [s for s, _ in ec.strides(K)] == [0, W + 3] and [w for _, w in ec.strides(K)] == [W, W + 3]
        wins = ec.windows(K, R)
        assert len(wins) == len(set(wins)) and all(0 <= f and 1 <= c and f + c <= N for f, c in wins)
        assert (0, N) in wins and (N - 1, 1) in wins and (31, 66) in wins
        assert any(f + c <= K for f, c in wins), "an information-only window"
        if R > 0:
            assert any(f < K < f + c for f, c in wins), "a window that straddles K"
            assert any(f >= K for f, c in wins), "a parity-only window"
        else:
            assert any(f < K == f + c for f, c in wins)


@pytest.mark.parametrize("case", [c for c in ec.SYNTH_CASES if c[0] != "n10000"] + [("n10000", 8192, 1808)], ids=ec.synth_id)
def test_every_synthetic_case_sets_information_and_parity_bits(case):
    _, K, R = case
    for _, stride in ec.strides(K):
        words = ec.info_words(K, stride)
        cw = ec.synth_reference(K, R, stride)
        assert words.shape == (130, stride) and cw.shape == (130, K + R) and cw.max() <= 1
        assert cw[:, :K].any() and (R == 0 or cw[:, K:].any())
        assert (cw[:, :K] == ec.unpack(words, K)).all()
        if K % 32:                                   # bits beyond K in the last word are set in the input and must not reach the reference
            assert (words[:, K // 32] >> np.uint32(K % 32)).any()
        if stride > (K + 31) // 32:
            assert words[:, (K + 31) // 32:].any()
        # the generator carries bits beyond K too
        rows = ec.fc.generator_rows(K, R)
        if R and K % 64:
            assert (rows[:, -1] >> np.uint64(K % 64)).any()
        # a window's words: bits beyond the count are 0
        for first, count in ec.windows(K, R)[:4]:
            w = ec.window_words(cw, first, count)
            assert w.shape == (130, (count + 31) // 32) and (ec.unpack(w, count) == cw[:, first:first + count]).all()
            assert count % 32 == 0 or not (w[:, -1] >> np.uint32(count % 32)).any()


@pytest.mark.parametrize("name", list(ec.REAL_CODES))
def test_reference_codewords_of_the_real_codes_satisfy_the_parity_checks_by_the_oracle(name):
    from oracle import oracle as orc
    ref = ec.real_reference(name)
    N, K, R = ref["N"], ref["K"], ref["R"]
    assert ref["cw"].shape == (ec.REAL_B, N) and K + R == N
    if name == "N2048":
        assert R == 325 < ref["graph"][1]                        # rank-deficient H
    oc = orc.Codec(orc.Code(graph=ref["graph"]), skip_rank=True)
    assert all(oc.syndrome_ok(c) for c in ref["cw"])
    assert not oc.syndrome_ok(ref["cw"][0] ^ np.eye(N, dtype=np.uint8)[K])       # (the check can fail)
    assert (ref["cw"][:, :K] == ec.unpack(ref["words"], K)).all() and ref["cw"][:, K:].any() and ref["cw"][:, :K].any()


def test_loop_back_labels_decode_to_the_sent_words_at_the_first_exit_test_by_the_oracle():
    lp = ec.loop_reference()
    ref = ec.real_reference(ec.LOOP_CODE)
    assert lp["L"] > lp["qb_cha"].max() and -lp["L"] < lp["qb_cha"].min()
    assert float(np.float32(lp["L"])) > lp["qb_cha"].max()                     # (as the float32 the tensor holds)
    assert set(np.unique(lp["cha"]).tolist()) == {0, lp["nq_cha"] - 1}             # the two outermost labels
    assert (lp["decided"] == ec.pack(ref["cw"][:, :ref["K"]])).all()
    # psc on, pisc off: the first exit test is the syndrome test of iteration 0, whose return value is 0 + 1
    assert (lp["iters"] == 1).all() and lp["max_iters"] > 1
