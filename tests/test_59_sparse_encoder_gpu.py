"""The sparse triangular encoder on the device (lutldpc_decoder_set_sparse_generator; kernels_encode_sparse.hpp) against the numpy
references of tests/sparse_encode_cases.py: synthetic systems through the raw C-ABI -- one chain longer than two blocks of the solve,
permuted triangular systems whose terms reach into the same, the previous and the first block, runs of short chains, rows with no
terms, with parity terms only and with 40 terms, K at 1, 31, 32, 33 and off the word grid, R = 1 -- over batches around the 64-frame
wave step and the 128-frame slice, both frame strides and every kind of window, the output pre-filled and guarded; host memory against
device memory; the sparse against the dense generator of one code on one handle, encode_packed and encode_random; DVB-S2 itself:
encode_packed against the host encoder and H c = 0, sim_batch_random against sim_batch on the host-encoded codewords, and the loop-back
data -> codewords -> LLR -> decode_llr -> data; the ber_sim driver on a small zigzag code with either form.  All integer, equal bit
for bit.  (tests/test_sparse_encoder_cpu.py holds the cases and references to what they claim.)"""
import ctypes as C
import os

import numpy as np
import pytest

import encode_cases as ec
import frontend_cases as fc
import sparse_encode_cases as sc
from helpers import CODES, product_decoder, same as _same
from lut_ldpc_amd import packing
from lut_ldpc_amd._capi import ChannelCells, EncodeIO, check, lib

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


def _raw(dec, info, in_stride, B, first, count):
    """The raw entry on host memory: (return code, output words [B, W], guard words) -- the buffer pre-filled with 0xEE."""
    W = (count + 31) // 32
    buf = np.full(B * W + ec.GUARD_WORDS, FILL32, np.uint32)
    io = EncodeIO(0, in_stride, first, count, 0)
    rc = lib.lutldpc_decoder_encode_packed(dec._h, C.byref(io), C.c_void_p(info.ctypes.data), B, C.c_void_p(buf.ctypes.data))
    return rc, buf[:B * W].reshape(B, W), buf[B * W:]


@pytest.mark.parametrize("case", sc.SYSTEM_CASES, ids=sc.system_id)
def test_synthetic_systems_every_window_batch_and_stride(case, handles):
    handle, K, R, kind = case
    dec = handles(handle)
    row_ptr, cols = sc.system(K, R, kind)
    dec.set_sparse_generator(K, R, row_ptr, cols)                               # (replaces the generator of the case before on this live handle)
    gen = dec.describe()["generator"]
    block = gen["block"]
    assert gen == {"K": K, "R": R, "form": "sparse", "terms": len(cols), "block": block, "depth": sc.depth(K, R, row_ptr, cols)} and dec.nvar == K + R
    assert block == sc.BLOCK and (kind != "chain" or R == 1 or gen["depth"] > 2 * block + 1)
    for in_stride, stride in ec.strides(K):
        words, cw = ec.info_words(K, stride), sc.system_reference(K, R, kind, stride)
        for B in sc.BATCHES:
            info = np.ascontiguousarray(words[:B])
            for first, count in sc.windows(K, R):
                rc, got, guard = _raw(dec, info, in_stride, B, first, count)
                check(rc)
                _same(got, ec.window_words(cw[:B], first, count), f"stride {in_stride} B {B} window ({first}, {count})")
                assert (guard == FILL32).all(), (in_stride, B, first, count)
                if count % 32:
                    assert not (got[:, -1] >> np.uint32(count % 32)).any()


def test_host_memory_equals_device_memory_strided_views_and_the_asynchronous_call(handles):
    import torch
    dec = handles("q4")
    K, R, B = 500, 500, 130
    dec.set_sparse_generator(K, R, *sc.system(K, R, "permuted"))
    W = (K + 31) // 32
    words, cw = ec.info_words(K, W + ec.SPARE_WORDS), sc.system_reference(K, R, "permuted", W + ec.SPARE_WORDS)
    dev = torch.device("cuda", 0)
    full = torch.from_numpy(words[:B].view(np.int32).copy()).to(dev)         # [B, W + 3]: its first W columns are a row-strided view
    view = full[:, :W]
    for first, count in [(0, K + R), (K, R), (K - 1, 34), (31, 66)]:
        want = ec.window_words(cw[:B], first, count)
        _same(dec.encode_packed(np.ascontiguousarray(words[:B, :W]), first, count), want, f"numpy ({first}, {count})")
        for name, t in (("contiguous tensor", view.contiguous()), ("row-strided view", view), ("tensor with spare words", full)):
            got = dec.encode_packed(t, first, count)
            assert got.dtype == torch.int32 and got.device == t.device and tuple(got.shape) == want.shape
            _same(got.cpu().numpy().view(np.uint32), want, f"{name} ({first}, {count})")
        got = dec.encode_packed(view, first, count, sync=False)              # sync = 0 and a synchronise afterwards
        torch.cuda.synchronize(dev)
        _same(got.cpu().numpy().view(np.uint32), want, f"asynchronous ({first}, {count})")
    assert (full.cpu().numpy().view(np.uint32) == words[:B]).all()           # the input is read in place and left alone


@pytest.fixture(scope="module")
def ira(tmp_path_factory):
    """The open zigzag code of N = 1000 in the column order of its generator: (K, R, H, (row_ptr, cols), dense rows)."""
    import lut_ldpc_amd as L
    path, N, M = sc.zigzag_alist("ira1000", tmp_path_factory.mktemp("sparse_codes"))
    pcd = L.Codec(path, with_generator="sparse", device=-1)
    H = ec.parity_check_matrix(N, M, *pcd.graph())
    pcd.close()
    K = N - M
    row_ptr, cols, peeled = sc.peel(H, K)
    assert peeled == M
    return K, M, H, (row_ptr, cols), sc.dense_rows(H, K)


@pytest.mark.parametrize("handle", ["q4", "q4_pack1"])
def test_sparse_and_dense_generator_of_one_code_on_one_handle_give_the_same_words_and_the_same_random_codewords(handle, handles, ira):
    dec = handles(handle)
    K, R, H, (row_ptr, cols), rows = ira
    T = dec.describe()["tile_frames"]
    words = np.ascontiguousarray(ec.info_words(K, (K + 31) // 32)[:130])
    ranges = [(2 ** 40 + 5, 7, 0, 65), (3, fc.STREAM_MAX, fc.F_CARRY, T + 1), (fc.SEED_BIG, 1, fc.F_HIGH, 130)]     # F_CARRY: carries into the high index word
    out = {}
    for form in ("dense", "sparse", "dense"):
        if form == "dense":
            dec.set_generator(K, R, rows)
            assert dec.describe()["generator"] == {"K": K, "R": R}
        else:
            dec.set_sparse_generator(K, R, row_ptr, cols)
            assert dec.describe()["generator"]["form"] == "sparse" and dec.describe()["generator"]["depth"] == R
        got = [dec.encode_packed(words)] + [dec.encode_random(*r) for r in ranges]
        if form in out:
            assert all((a == b).all() for a, b in zip(out[form], got))      # ... and the dense one again, after the sparse one
        out[form] = got
    for (a, b), what in zip(zip(out["dense"], out["sparse"]), ["encode_packed"] + [f"encode_random {r}" for r in ranges]):
        _same(b, a, what)
    cw = ec.unpack(out["sparse"][0], K + R)
    assert cw[:, K:].any() and not ((cw.astype(np.int64) @ H.T.astype(np.int64)) % 2).any()
    seed, stream, f0, B = ranges[1]
    assert (out["sparse"][2][:, :K] == fc.info_bits(seed, stream, f0, B, K)).all()


# ---------------------------------------------------------------------------------------------------------------- DVB-S2
DVB_B, DVB_ITERS = 130, 3


@pytest.fixture(scope="module")
def dvbs2():
    import lut_ldpc_amd as L
    pcd = L.Codec(CODES / f"{sc.DVBS2}.alist", with_generator=True, known_rank=32400, device=0)
    pcd.design_luts(sigma2=0.88 ** 2, max_iters=DVB_ITERS, allow_degree_one=True)
    pcd.set_exit_conditions(DVB_ITERS, True, False)
    gen = pcd.decoder().describe()["generator"]
    assert gen["form"] == "sparse" and (gen["K"], gen["R"], gen["depth"]) == (32400, 32400, 32400)
    yield pcd
    pcd.close()


def test_dvbs2_encode_packed_equals_the_host_encoder_and_satisfies_every_check(dvbs2):
    N, K = dvbs2.nvar, dvbs2.ninfo
    data = np.random.default_rng(59).integers(0, 1 << 32, (DVB_B, (K + 31) // 32), dtype=np.uint32)
    words = dvbs2.encode_packed(data)
    assert words.shape == (DVB_B, (N + 31) // 32) and words.dtype == np.uint32
    cw = packing.unpack_bits(words, N)
    assert (cw[:, :K] == ec.unpack(data, K)).all() and cw[:, K:].any()
    dv, dc, cn = dvbs2.graph()
    chk_vars, chk_of_slot = np.repeat(np.arange(N), dv)[cn], np.repeat(np.arange(dvbs2.nchk), dc)
    synd = np.zeros((DVB_B, dvbs2.nchk), np.uint8)
    np.bitwise_xor.at(synd.T, chk_of_slot, cw[:, chk_vars].T)
    assert not synd.any()                                               # H c = 0 on all frames
    for i in range(64):
        assert (dvbs2.encode(cw[i, :K]) == cw[i]).all(), i
    _same(dvbs2.encode_packed(data, parity_only=True), ec.pack(cw[:, K:]), "parity_only")


def test_dvbs2_sim_batch_random_equals_sim_batch_on_the_host_encoded_codewords(dvbs2):
    N, K, B = dvbs2.nvar, dvbs2.ninfo, DVB_B
    snr, seed, stream, f0 = 1.2, 2 ** 33 + 9, 2, 2 ** 32 - 50                 # (the frame index carries into its high word inside the batch)
    _, _, cw = dvbs2.sample_labels(snr, seed, stream, f0, B, zero_codeword=False)      # the HOST encoder's codewords of these frames
    assert cw[:, :K].any() and cw[:, K:].any()
    cells = ChannelCells.from_table(dvbs2.channel_cells(snr))
    dec = dvbs2.decoder()
    cha_h, bits_h, cha_d, bits_d = (np.full((B, N), 0xEE, np.uint8) for _ in range(4))
    want, _, _ = dec.sim_batch(cells, seed, stream, f0, B, K, codewords=cw, cha_out=cha_h, bits_out=bits_h)
    got, _, _ = dec.sim_batch(cells, seed, stream, f0, B, K, random=True, cha_out=cha_d, bits_out=bits_d)
    _same(got, want, "frame_stats")
    assert (want[:, 3] > 0).all()
    assert (cha_h == cha_d).all() and (bits_h == bits_d).all()
    _same(dvbs2.sim_batch(snr, seed, stream, f0, B, zero_codeword=False), want, "Codec.sim_batch")
    _same(dvbs2.encode_random(seed, stream, f0, B), cw, "encode_random")


def test_dvbs2_loop_back_on_the_device_returns_the_data(dvbs2):
    import torch
    N, K, B = dvbs2.nvar, dvbs2.ninfo, DVB_B
    L = ec.loop_llr_magnitude(dvbs2.qb_cha)
    dev = torch.device("cuda", 0)
    data = torch.from_numpy(np.random.default_rng(60).integers(0, 1 << 32, (B, (K + 31) // 32), dtype=np.uint32).view(np.int32)).to(dev)
    cw_words = dvbs2.encode_packed(data)
    assert cw_words.is_cuda and tuple(cw_words.shape) == (B, (N + 31) // 32)
    shifts = torch.arange(32, device=dev, dtype=torch.int32)
    bits = ((cw_words[:, :, None] >> shifts[None, None, :]) & 1).reshape(B, -1)[:, :N]
    llr = (L * (1.0 - 2.0 * bits.to(torch.float32))).to(torch.float32)
    got_words, iters = dvbs2.decode_llr(llr)
    mask = torch.full((1, (K + 31) // 32), -1, dtype=torch.int32, device=dev)
    if K % 32:
        mask[0, -1] = (1 << (K % 32)) - 1
    assert bool((got_words == (data & mask)).all()) and bool((iters == 1).all())


# ---------------------------------------------------------------------------------------------------------------- ber_sim
INI = """[Sim]
   SNRdB    = 1:1:3
   Nframes  = 300
   Nfers    = 300
[LDPC]
   parity_filename = runs410
   zero_codeword   = false
   generator_form  = {form}
[LUT]
   max_iter = 6
   design_SNRdB = 2.0
   qbits_channel = 4
   qbits_message_uniform = 4
   allow_degree_one = true
"""


def test_ber_sim_counts_the_same_with_the_dense_and_with_the_forced_sparse_generator(tmp_path):
    (tmp_path / "codes").mkdir()
    sc.zigzag_alist("runs410", tmp_path / "codes")
    got = {}
    for form in ("auto", "sparse"):
        params = tmp_path / f"ber.ini.{form}"
        params.write_text(INI.format(form=form))
        snr = (C.c_double * 8)()
        cnt = (C.c_int64 * 40)()
        n = lib.lutldpc_ber_sim_run(str(params).encode(), str(tmp_path).encode(), 0, form.encode(), 0, 0, 1, snr, cnt, 8)
        check(min(n, 0))
        assert n == 3
        got[form] = np.array(cnt[:n * 5]).reshape(n, 5)
    assert (got["auto"] == got["sparse"]).all(), (got["auto"], got["sparse"])
    assert got["auto"][0, 0] == 300 and got["auto"][0, 4] > 0 and got["auto"][0, 3] > 0      # 1 dB: all frames run, uncoded and data bit errors
