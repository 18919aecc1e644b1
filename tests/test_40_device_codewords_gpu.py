"""Random codewords made on the device (LDPC.zero_codeword = false): the device encoder against the oracle's information bits,
the parity checks of the product's graph and the host encoder; sim_batch on device codewords against lutldpc_decoder_sim_batch
fed the host-encoded ones; config 5 (ber.ini.regular.example) end to end against the oracle's frame loop."""
import ctypes as C
import shutil

import numpy as np
import pytest

import lut_ldpc_amd as L
from lut_ldpc_amd._capi import ChannelCells, check, lib
from helpers import C5_TREES, CODES, ROOT, TREES, c5_sigma2, oracle_graph
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

# every code in data/codes the host builds a generator for (the N = 64800 codes are beyond its dense elimination)
GEN_CODES = ["rate0.50_dv02-17_dc08-09_lut_q4_N500", "rate0.50_dv02-17_dc08-09_lut_q4_N1000", "rate0.50_dv03_dc06_N1000",
             "rate0.84_reg_v6c32_N2048", "rate0.50_dv03_dc06_N10000"]


@pytest.mark.parametrize("alist", GEN_CODES)
def test_device_encoder_matches_oracle_info_bits_parity_checks_and_host_encoder(alist):
    pcd = L.Codec(CODES / f"{alist}.alist", with_generator=True, device=0)
    pcd.design_luts(sigma2=0.88 ** 2, max_iters=4)                 # (the device handle needs tables)
    N, K = pcd.nvar, pcd.ninfo
    assert pcd.decoder().describe()["generator"] == {"K": K, "R": pcd.rank}
    if alist.endswith("N2048"):
        assert pcd.rank == 325 < pcd.nchk                            # rank-deficient H
    oc = orc.Codec(oracle_graph(pcd), skip_rank=True)
    seed, stream, f0 = 2 ** 32 + 77, 3, 2 ** 32 + 5
    rng = np.random.default_rng(1)
    for B in (1, 17, 4097):
        cw = pcd.encode_random(seed, stream, f0, B)
        assert cw.shape == (B, N) and cw.max() <= 1
        for i in range(B):
            assert (cw[i, :K] == orc.info_bits(seed, stream, f0 + i, K)).all(), (B, i)
            assert oc.syndrome_ok(cw[i]), (B, i)
        for i in rng.choice(B, size=min(B, 6), replace=False):
            assert (pcd.encode(cw[i, :K]) == cw[i]).all(), (B, i)
        if B > 1:
            h = B // 3
            assert (np.concatenate([pcd.encode_random(seed, stream, f0, h), pcd.encode_random(seed, stream, f0 + h, B - h)]) == cw).all()
    assert pcd.encode_random(seed + 1, stream, f0, 17)[:, :K].tolist() != pcd.encode_random(seed, stream, f0, 17)[:, :K].tolist()
    pcd.close()


def _product_c1():
    pcd = L.Codec(CODES / "rate0.50_dv02-17_dc08-09_lut_q4_N500.alist", with_generator=True, device=0)
    pcd.design_luts(sigma2=0.88 ** 2, max_iters=50)
    pcd.set_exit_conditions(50, True, True)
    return pcd, 1.5


def _product_c5():
    pcd = L.Codec(CODES / "rate0.84_reg_v6c32_N2048.alist", with_generator=True, device=0)
    pcd.design_luts(tree_method=C5_TREES, sigma2=c5_sigma2(), max_iters=8, nq_cha=16, nq_msg=8)
    pcd.set_initial_message_mode(1)                                   # from_quantized_channel_llrs
    pcd.set_exit_conditions(8, True, True)
    return pcd, 4.0


@pytest.mark.parametrize("cfg", ["c1", "c5"])
@pytest.mark.parametrize("resident", ["1", "0"])
def test_sim_batch_on_device_codewords_equals_host_codewords(cfg, resident, monkeypatch):
    monkeypatch.setenv("LUTLDPC_RESIDENT", resident)              # read when the device handle is created
    pcd, snr = (_product_c1 if cfg == "c1" else _product_c5)()
    B, seed, stream = 1337, 2 ** 33 + 9, 2                           # not a multiple of the frame group
    got = pcd.sim_batch(snr, seed, stream, 0, B, zero_codeword=False)
    # the same frames through lutldpc_decoder_sim_batch, fed the codewords of the HOST encoder (sample_labels keeps it)
    cha_host, msg_host, cw = pcd.sample_labels(snr, seed, stream, 0, B, zero_codeword=False)
    assert cw.any()
    cells = ChannelCells.from_table(pcd.channel_cells(snr))
    dec = pcd.decoder()
    assert dec.describe()["resident"] == int(resident)
    N = pcd.nvar
    cha_h, bits_h, cha_d, bits_d = (np.full((B, N), 0xEE, np.uint8) for _ in range(4))
    want, _, _ = dec.sim_batch(cells, seed, stream, 0, B, pcd.ninfo, codewords=cw, cha_out=cha_h, bits_out=bits_h)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    assert (want[:, 3] > 0).all()
    # the labels and decided bits of both: the host codewords reach the sampler and the counters as the same sent-bit rows
    rnd, _, _ = dec.sim_batch(cells, seed, stream, 0, B, pcd.ninfo, random=True, cha_out=cha_d, bits_out=bits_d)
    assert (rnd == want).all()
    assert (cha_h == cha_d).all() and (bits_h == bits_d).all()
    # ... and the test entry of the sampler, fed the same host codewords: that cha again, and the msg0 of the call above
    cha_s, msg_s = dec.sample_labels(cells, seed, stream, 0, B, codewords=cw, cha=np.full((B, N), 0xEE, np.uint8), msg=np.full((B, N), 0xEE, np.uint8))
    assert (cha_s == cha_h).all() and (cha_s == cha_host).all() and (msg_s == msg_host).all()
    # pad frames carry zero codewords and no counts: the first frames of a larger batch (no padding there) are the same frames
    big = pcd.sim_batch(snr, seed, stream, 0, 2048, zero_codeword=False)
    assert (big[:B] == got).all()
    pcd.close()


@pytest.mark.parametrize("pack,B", [("", 515), ("1", 259)])
def test_host_codewords_equal_device_codewords_in_histogram_and_events(pack, B, monkeypatch):
    """sim_batch_histogram (level 3, all frames) and sim_batch_events (select = codeword, every frame kept) on C1, once on the
    encoder's codewords and once on the bytes encode_random returns for them, passed back as host codewords: the same sent-bit
    rows either way, so identical histograms, frame_stats, records, lists and profiles.  Two frame groups, three frames in the
    second: nibble rows at B = 515, byte rows (LUTLDPC_PACK = 1) at B = 259."""
    if pack:
        monkeypatch.setenv("LUTLDPC_PACK", pack)                    # read when the device handle is created
    pcd, snr = _product_c1()
    dec = pcd.decoder()
    assert dec.describe()["pack"] == (1 if pack else 2) and -(-B // dec.describe()["tile_frames"]) == 2
    seed, stream, f0 = 2 ** 33 + 11, 4, 2 ** 32 + 3
    cw = np.ascontiguousarray(pcd.encode_random(seed, stream, f0, B))
    assert cw.any() and cw.max() <= 1
    cells = ChannelCells.from_table(pcd.channel_cells(snr))
    nd, groups, labels, _ = dec.histogram_shape(3)
    res = []
    for codewords, on_device in ((None, True), (cw, False)):
        hist = dec.sim_batch_histogram(cells, seed, stream, f0, B, codewords=codewords, device_codewords=on_device, level=3, mode="all", n_labels=labels)
        assert hist.shape == (nd, groups, 2, labels) and hist[:, :, 1].any()
        ev, stats = dec.sim_batch_events(cells, seed, stream, f0, B, k_info=pcd.ninfo, codewords=codewords, device_codewords=on_device, select="codeword",
                                         max_frames=B, max_pos=64, max_chk=64, profiles=True, frame_stats=np.full((B, 4), -7, np.int32))
        res.append((hist, stats, ev))
    (h_d, s_d, e_d), (h_h, s_h, e_h) = res
    assert (h_d == h_h).all() and (s_d == s_h).all()
    assert e_d.n_selected == e_h.n_selected > 0 and len(e_d.events) == len(e_h.events) > 0
    assert (e_d.events == e_h.events).all() and (e_d.positions == e_h.positions).all() and (e_d.checks == e_h.checks).all()
    assert (e_d.node_errors == e_h.node_errors).all() and (e_d.check_fails == e_h.check_fails).all()
    pcd.close()


def test_ber_sim_regular_example_with_random_codewords_matches_oracle(tmp_path):
    """BASELINE config 5 (ber.ini.regular.example, zero_codeword = false, output_verbosity = 1) with Nframes raised: the counters of
    every SNR point equal the oracle's frame loop on the host-encoded codewords."""
    for d in ("codes", "trees"):
        (tmp_path / d).mkdir()
    shutil.copy(CODES / "rate0.84_reg_v6c32_N2048.alist", tmp_path / "codes")
    shutil.copy(TREES / "6_32_wide.ini", tmp_path / "trees")
    ini = (ROOT / "data" / "params" / "ber.ini.regular.example").read_text()
    assert "Nframes  = 20" in ini and "zero_codeword   = false" in ini
    params = tmp_path / "ber.ini.regular.example"
    params.write_text(ini.replace("Nframes  = 20", "Nframes  = 300"))
    snr = (C.c_double * 32)(); cnt = (C.c_int64 * 160)()
    n = lib.lutldpc_ber_sim_run(str(params).encode(), str(tmp_path).encode(), 0, b"", 0, 1, 1, snr, cnt, 32)
    check(min(n, 0))
    assert n == 7 and list(snr[:n]) == [3, 3.5, 4, 4.5, 5, 5.5, 6]
    got = np.array(cnt[:n * 5]).reshape(n, 5)
    pcd, _ = _product_c5()
    ref = orc.Codec(oracle_graph(pcd), skip_rank=True)
    ref.set_rank(325)
    ref.design_luts(tree_method=C5_TREES, sigma2=c5_sigma2(), max_iters=8, nq_cha=16, nq_msg=np.full(8, 8, np.int32))
    assert ref.var_tree_txt == pcd.var_trees_txt
    ref.set_initial_message_mode(1)
    ref.set_exit_conditions(8, True, True)
    stop = False
    for i in range(n):
        if stop:
            assert (got[i] == 0).all()
            continue
        _, _, cw = pcd.sample_labels(snr[i], 0, i, 0, 300, zero_codeword=False)
        want, _, stop = ref.sim_snr_point(snr[i], 1.0 - 325 / 2048, 2048 - 325, 0, i, 300, nfers=20, codewords=cw)
        assert (got[i] == want).all(), (i, got[i], want)
    assert got[0][0] > 0
    pcd.close()
