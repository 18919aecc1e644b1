"""lutldpc_decoder_encode_packed on the device against the numpy references of tests/encode_cases.py: synthetic generators at the edges
of K and R (generator and information words random in all their bits) over batches around the 64-frame workgroup, both frame strides
and windows that are information-only, straddle K, are parity-only or start off the word grid, with the output pre-filled and
guarded; host memory against device memory; the real codes through Codec against H c = 0 and the host encoder; the tie to
encode_random; the loop-back data -> codewords -> LLR -> decode_llr -> data on the device; the state of the handle; the refusals.
All integer, equal bit for bit.  (tests/test_encode_packed_cpu.py holds the cases and references to what they claim.)"""
import ctypes as C
import os

import numpy as np
import pytest

import encode_cases as ec
import frontend_cases as fc
from helpers import product_decoder, same as _same
from lut_ldpc_amd import packing
from lut_ldpc_amd._capi import ERR_ARG, ERR_STATE, EncodeIO, LutLdpcError, check, last_error, lib

pytestmark = pytest.mark.gpu

FILL32 = np.uint32(ec.FILL * 0x01010101)


@pytest.fixture(scope="module")
def handles():
    """handle name of frontend_cases.HANDLES -> device decoder, created on first use (its knobs are read at creation) and kept."""
    made = {}

    def get(name):
        if name not in made:
            code, env, T = fc.HANDLES[name]
            old = os.environ.pop("LUTLDPC_PACK", None)
            os.environ.update(env)
            try:
                dec = product_decoder(fc.codec(code), device=0)
            finally:
                os.environ.pop("LUTLDPC_PACK", None)
                if old is not None:
                    os.environ["LUTLDPC_PACK"] = old
            assert dec.describe()["tile_frames"] == T
            made[name] = dec
        return made[name]
    yield get
    for dec in made.values():
        dec.close()


def _raw(dec, info, in_stride, B, first, count, io=None):
    """The raw entry on host memory: (return code, output words [B, W], guard words) -- the buffer pre-filled with 0xEE."""
    W = (count + 31) // 32
    buf = np.full(B * W + ec.GUARD_WORDS, FILL32, np.uint32)
    io = io or EncodeIO(0, in_stride, first, count, 0)
    rc = lib.lutldpc_decoder_encode_packed(dec._h, C.byref(io), C.c_void_p(info.ctypes.data), B, C.c_void_p(buf.ctypes.data))
    return rc, buf[:B * W].reshape(B, W), buf[B * W:]


@pytest.mark.parametrize("case", ec.SYNTH_CASES, ids=ec.synth_id)
def test_synthetic_generators_at_the_edges_of_k_and_r_every_window_batch_and_stride(case, handles):
    handle, K, R = case
    dec = handles(handle)
    dec.set_generator(K, R, fc.generator_rows(K, R))                            # (replaces the generator of the case before on this live handle)
    assert dec.describe()["generator"] == {"K": K, "R": R} and dec.nvar == K + R
    for in_stride, stride in ec.strides(K):
        words, cw = ec.info_words(K, stride), ec.synth_reference(K, R, stride)
        for B in ec.BATCHES:
            info = np.ascontiguousarray(words[:B])
            for first, count in ec.windows(K, R):
                rc, got, guard = _raw(dec, info, in_stride, B, first, count)
                check(rc)
                want = ec.window_words(cw[:B], first, count)
                _same(got, want, f"stride {in_stride} B {B} window ({first}, {count})")
                assert (guard == FILL32).all(), (in_stride, B, first, count)
                if count % 32:
                    assert not (got[:, -1] >> np.uint32(count % 32)).any()


def test_host_memory_equals_device_memory_strided_views_and_the_asynchronous_call(handles):
    import torch
    dec = handles("q4")
    K, R, B = 500, 500, 130
    dec.set_generator(K, R, fc.generator_rows(K, R))
    W = (K + 31) // 32
    words, cw = ec.info_words(K, W + ec.SPARE_WORDS), ec.synth_reference(K, R, W + ec.SPARE_WORDS)
    dev = torch.device("cuda", 0)
    full = torch.from_numpy(words.view(np.int32).copy()).to(dev)            # [B, W + 3]: its first W columns are a row-strided view
    view = full[:, :W]
    assert view.stride(0) == W + ec.SPARE_WORDS and not view.is_contiguous()
    for first, count in [(0, K + R), (K, R), (K - 1, 34), (31, 66)]:
        want = ec.window_words(cw, first, count)
        host = dec.encode_packed(np.ascontiguousarray(words[:, :W]), first, count)
        assert isinstance(host, np.ndarray) and host.dtype == np.uint32
        _same(host, want, f"numpy ({first}, {count})")
        _same(dec.encode_packed(words.view(np.int32), first, count), want, f"numpy int32, spare words ({first}, {count})")
        for name, t in (("contiguous tensor", view.contiguous()), ("row-strided view", view), ("tensor with spare words", full)):
            got = dec.encode_packed(t, first, count)
            assert got.dtype == torch.int32 and got.device == t.device and tuple(got.shape) == want.shape
            _same(got.cpu().numpy().view(np.uint32), want, f"{name} ({first}, {count})")
        # sync = 0 and a synchronise of the decoder's stream afterwards
        got = dec.encode_packed(view, first, count, sync=False)
        torch.cuda.synchronize(dev)
        _same(got.cpu().numpy().view(np.uint32), want, f"asynchronous ({first}, {count})")
    assert (full.cpu().numpy().view(np.uint32) == words).all()             # the input is read in place and left alone
    with pytest.raises(ValueError):
        dec.encode_packed(full.to(torch.int64))
    with pytest.raises(ValueError):
        dec.encode_packed(full.cpu())
    with pytest.raises(ValueError):
        dec.encode_packed(full.t())


def _graph_checks(ref, cw):
    """H c mod 2 over all frames, in numpy, from the graph of the reference."""
    H = ec.parity_check_matrix(*ref["graph"])
    return (cw.astype(np.float64) @ H.T.astype(np.float64)).astype(np.int64) % 2


@pytest.mark.parametrize("name", list(ec.REAL_CODES))
def test_real_codes_through_codec_satisfy_the_parity_checks_and_equal_the_host_encoder(name):
    ref = ec.real_reference(name)
    pcd = ec.product_codec(name, device=0)
    N, K, R, B = pcd.nvar, pcd.ninfo, pcd.rank, ec.REAL_B
    assert (N, K, R) == (ref["N"], ref["K"], ref["R"]) and (name != "N2048" or R == 325 < pcd.nchk)
    graph = (N, pcd.nchk) + tuple(pcd.graph())
    assert all((a == b).all() if isinstance(a, np.ndarray) else a == b for a, b in zip(graph, ref["graph"]))
    words = pcd.encode_packed(ref["words"])
    assert words.shape == (B, (N + 31) // 32) and words.dtype == np.uint32
    cw = packing.unpack_bits(words, N)
    assert not _graph_checks(ref, cw).any()
    assert (cw[:, :K] == ec.unpack(ref["words"], K)).all()                   # the first ninfo bits are the (masked) data
    _same(words, ec.pack(ref["cw"]), "reference codewords")
    for i in np.random.default_rng(58).choice(B, size=6, replace=False):
        assert (pcd.encode(cw[i, :K]) == cw[i]).all(), i
    par = pcd.encode_packed(ref["words"], parity_only=True)
    _same(par, ec.pack(cw[:, K:]), "parity_only")
    _same(pcd.encode_packed(cw[:, :K].copy()), words, "0/1 bytes in")        # uint8 [B, ninfo] is packed first
    with pytest.raises(ValueError):
        pcd.encode_packed(cw.copy())                                          # uint8 of another width
    pcd.close()


def test_codec_without_a_generator_says_so():
    import lut_ldpc_amd as L
    from helpers import CODES
    pcd = L.Codec(CODES / (ec.REAL_CODES["N500"][0] + ".alist"), with_generator=False, device=0)
    pcd.design_luts(**ec.REAL_CODES["N500"][1])
    with pytest.raises(ValueError, match="with_generator"):
        pcd.encode_packed(np.zeros((2, (pcd.ninfo + 31) // 32), np.uint32))
    with pytest.raises(LutLdpcError, match="lutldpc_decoder_set_generator") as e:
        pcd.decoder().encode_packed(np.zeros((2, (pcd.ninfo + 31) // 32), np.uint32))
    assert e.value.code == ERR_STATE
    pcd.close()


def test_encode_packed_of_the_information_bits_of_encode_random_equals_encode_random():
    pcd = ec.product_codec("N1000", device=0)
    K, B = pcd.ninfo, 65
    seed, stream, f0 = 2 ** 40 + 5, 7, 2 ** 32 + 2 ** 20                     # a frame index above 2^32
    cw = pcd.encode_random(seed, stream, f0, B)
    assert cw[:, :K].any() and cw[:, K:].any()
    _same(pcd.encode_packed(packing.pack_bits(cw[:, :K])), packing.pack_bits(cw), "encode_random")
    pcd.close()


def test_loop_back_on_the_device_returns_the_data_at_the_first_exit_test():
    import torch
    lp = ec.loop_reference()
    pcd = ec.product_codec(ec.LOOP_CODE, device=0)
    pcd.set_exit_conditions(lp["max_iters"], True, False)
    K, N, B = pcd.ninfo, pcd.nvar, ec.LOOP_B
    L = lp["L"]
    assert np.float32(L) > pcd.qb_cha.max() and -np.float32(L) < pcd.qb_cha.min()
    dev = torch.device("cuda", 0)
    data = torch.from_numpy(lp["words"][:B].view(np.int32).copy()).to(dev)
    cw_words = pcd.encode_packed(data)
    assert cw_words.is_cuda and cw_words.dtype == torch.int32 and tuple(cw_words.shape) == (B, (N + 31) // 32)
    # the caller's channel, in torch: bit k of the codeword -> LLR = L (0) or -L (1), float32
    shifts = torch.arange(32, device=dev, dtype=torch.int32)
    bits = ((cw_words[:, :, None] >> shifts[None, None, :]) & 1).reshape(B, -1)[:, :N]
    llr = (L * (1.0 - 2.0 * bits.to(torch.float32))).to(torch.float32)
    got_words, iters = pcd.decode_llr(llr)
    assert got_words.is_cuda and iters.is_cuda
    mask = torch.full((1, (K + 31) // 32), -1, dtype=torch.int32, device=dev)
    if K % 32:
        mask[0, -1] = (1 << (K % 32)) - 1
    assert bool((got_words == (data & mask)).all()) and bool((iters == 1).all())        # the one comparison that comes to the host
    assert (lp["iters"] == 1).all() and (got_words.cpu().numpy().view(np.uint32) == lp["decided"][:B]).all()
    pcd.close()


def test_state_of_the_handle_is_left_alone_and_a_new_generator_takes_effect(handles):
    import lut_ldpc_amd as L
    from helpers import CODES
    pcd = L.Codec(CODES / (ec.REAL_CODES["N500"][0] + ".alist"), with_generator=True, device=0)
    pcd.design_luts(sigma2=0.88 ** 2, max_iters=50)                  # (50 iterations at 1.5 dB: frames leave at many iteration counts)
    pcd.set_exit_conditions(50, True, True)
    B, seed = 600, 2 ** 33 + 9                                       # two frame groups, the second one partial
    before = pcd.sim_batch(1.5, seed, 2, 0, B, zero_codeword=False)
    assert (before[:, 3] > 0).all() and len(set(before[:, 0].tolist())) > 1
    words = np.random.default_rng(5).integers(0, 1 << 32, (130, (pcd.ninfo + 31) // 32), dtype=np.uint32)
    first = pcd.encode_packed(words)
    assert (pcd.sim_batch(1.5, seed, 2, 0, B, zero_codeword=False) == before).all()
    assert (pcd.encode_packed(words) == first).all()                 # ... and the decode in between left the encoder alone
    pcd.close()
    dec = handles("q4")
    out = {}
    for K in (33, 500, 33):
        dec.set_generator(K, 1000 - K, fc.generator_rows(K, 1000 - K))
        W = (K + 31) // 32
        got = dec.encode_packed(np.ascontiguousarray(ec.info_words(K, W)[:65]))
        _same(got, ec.pack(ec.synth_reference(K, 1000 - K, W)[:65]), f"K {K}")
        assert K not in out or (out[K] == got).all()
        out[K] = got
    assert (out[33] != out[500]).any()


def test_refusals_on_a_live_handle_write_nothing():
    dec = product_decoder(fc.codec("reg36_n1000_q4"), device=0)      # a fresh handle: no generator yet
    N, K, B = dec.nvar, 500, 5
    W = (K + 31) // 32
    info = np.ascontiguousarray(ec.info_words(K, W)[:B])
    rc, got, guard = _raw(dec, info, 0, B, 0, N)
    assert rc == ERR_STATE and "lutldpc_decoder_set_generator" in last_error() and (got == FILL32).all()
    dec.set_generator(K, N - K, fc.generator_rows(K, N - K))
    out = np.full((B, (N + 31) // 32 + 1), FILL32, np.uint32)
    good = lambda **kw: EncodeIO(**{**dict(on_device=0, in_stride=0, out_first=0, out_count=N, sync=0), **kw})
    call = lambda h, io, src, b, dst: lib.lutldpc_decoder_encode_packed(h, C.byref(io) if io is not None else None, src, b, dst)
    pi, po = C.c_void_p(info.ctypes.data), C.c_void_p(out.ctypes.data)
    bad = {
        "NULL handle": lambda: call(None, good(), pi, B, po),
        "B = 0": lambda: call(dec._h, good(), pi, 0, po),
        "B < 0": lambda: call(dec._h, good(), pi, -1, po),
        "NULL io": lambda: call(dec._h, None, pi, B, po),
        "NULL info": lambda: call(dec._h, good(), None, B, po),
        "NULL out_words": lambda: call(dec._h, good(), pi, B, None),
        "info off by 2 bytes": lambda: call(dec._h, good(), C.c_void_p(info.ctypes.data + 2), B, po),
        "out_words off by 1 byte": lambda: call(dec._h, good(), pi, B, C.c_void_p(out.ctypes.data + 1)),
        "in_stride below ceil(K/32)": lambda: call(dec._h, good(in_stride=W - 1), pi, B, po),
        "negative in_stride": lambda: call(dec._h, good(in_stride=-1), pi, B, po),
        "out_first < 0": lambda: call(dec._h, good(out_first=-1, out_count=5), pi, B, po),
        "out_count < 1": lambda: call(dec._h, good(out_count=0), pi, B, po),
        "window past nvar": lambda: call(dec._h, good(out_first=1, out_count=N), pi, B, po),
    }
    for name, c in bad.items():
        assert c() == ERR_ARG, name
        assert (out == FILL32).all(), name
    # the same buffers, valid arguments: the call works (4-byte alignment is all that is asked: one word into both buffers)
    spare = np.concatenate([np.zeros(1, np.uint32), info.ravel()])
    check(call(dec._h, good(in_stride=W), C.c_void_p(spare.ctypes.data + 4), B, C.c_void_p(out.ctypes.data + 4)))
    want = ec.pack(ec.synth_reference(K, N - K, W)[:B])
    assert (out.ravel()[1:1 + want.size].reshape(want.shape) == want).all() and out.ravel()[0] == FILL32 and (out.ravel()[1 + want.size:] == FILL32).all()
    dec.close()
