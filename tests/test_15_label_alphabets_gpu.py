"""Label alphabets from 2 to 64 labels on the device, against the oracle: the decoder on every path it offers for an alphabet
(LDS-resident, skewed pipeline, per-class streaming, generic kernels, one label per byte), the device sampler, sim_batch,
encode_random and the device quantiser.  A label is a sign bit `sbit` over a magnitude code with nz = Nq/2 = 1 << sbit
(kernels_fast.hpp); the byte-parallel compares and selects degenerate at nz = 1 (no magnitude bits) and nz = 2 (one), and
alphabets whose half is not a power of two leave the fast kernels for the generic ones, iteration by iteration."""
import ctypes as C
import functools
import re
import shutil

import numpy as np
import pytest

import lut_ldpc_amd as L
from lut_ldpc_amd._capi import ERR_ARG, ChannelCells, check, lib
from helpers import C5_TREES, CODES, ROOT, awgn_labels, c5_sigma2, designed_codec, oracle_codec, oracle_graph, product_codec, product_decoder, write_ira_alist
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

# name in helpers.CONFIGS, test SNR (dB), initial-message modes: picked with the oracle so that every batch mixes frames that
# leave early, frames that run every iteration and failures
CASES = [
    ("reg36_n1000_ex8421", 3.5, (0,)),
    ("n500_ex8421", 3.5, (0,)),
    ("reg36_n1000_ex8421_chklut", 3.5, (0,)),
    ("reg36_n1000_m2", 8.0, (0,)),
    ("reg36_n1000_c2m4", 5.0, (0, 1)),
    ("reg36_n1000_c4m4", 4.0, (0,)),
    ("reg36_n1000_grow", 3.0, (0,)),
    ("reg36_n1000_m12", 3.0, (0,)),
    ("reg36_n1000_m6", 8.0, (0,)),
    ("reg36_n1000_m16_12_8", 5.0, (0,)),
    ("reg36_n1000_q6", 4.0, (0,)),
]
PATHS = {
    "default": {},
    "streaming": {"LUTLDPC_RESIDENT": "0"},
    "streaming_noskew": {"LUTLDPC_RESIDENT": "0", "LUTLDPC_SKEW": "0"},
    "generic": {"LUTLDPC_USE_FAST": "0"},
    "pack1": {"LUTLDPC_PACK": "1"},
}
EXITS = [(True, True), (True, False), (False, False)]
BATCHES = (777, 5)          # three frame groups with a ragged last one; fewer than 8 frames


def _pow2_half(nq):
    return (nq // 2) & (nq // 2 - 1) == 0


@functools.lru_cache(maxsize=None)
def _labels(name, snr, mode, B):
    cd = oracle_codec(name)
    cd.set_initial_message_mode(mode)
    cha, msg, _ = awgn_labels(cd, B, snr, seed=15000 + B + mode, mode=mode)
    for f in (0, B // 2):                   # noise-free frames: they pass the test on the channel decisions
        cha[f] = cd.nq_cha - 1
        msg[f] = cd.nq_msg[0] - 1 if mode == 0 else cd.cha2msg_map[cd.nq_cha - 1]
    return cha, msg


@functools.lru_cache(maxsize=None)
def _want(name, snr, mode, B, psc, pisc):
    """The oracle's decode of one batch (the same for every product path: computed once)."""
    cd = oracle_codec(name)
    cha, msg = _labels(name, snr, mode, B)
    cd.set_exit_conditions(cd.max_iters, psc, pisc)
    return cd.lut_decode_batch_flat(cha, msg)


def _widest(cd):
    return max([cd.nq_cha] + [int(q) for q in cd.nq_msg])


def _pow2(n):
    return n & (n - 1) == 0


def _expected_vn(cd, env):
    """The kernel string of a variable class: per variable pass (ii writes the alphabet of iteration ii + 1 from that of ii) the
    interpreter where the new alphabet's half is no power of two (no sign bit) or the fast kernels are off; else the compile-time
    kernel where every alphabet feeding the tables is a power of two of at most 16 labels (balanced tables of <= 256 entries), else
    the generated one.  Distinct names joined in the order fast, generated, interpreter."""
    nq = [int(q) for q in cd.nq_msg]
    used = set()
    for ii in range(len(nq) - 1):
        if env.get("LUTLDPC_USE_FAST") == "0" or not _pow2_half(nq[ii + 1]):
            used.add("tree_pass_kernel<VAR>")
        elif _pow2(nq[ii]) and _pow2(cd.nq_cha) and max(nq[ii], cd.nq_cha) <= 16:
            used.add("vn_balanced_fast_kernel")
        else:
            used.add("lutldpc_jit_pass")
    return "+".join(k for k in ("vn_balanced_fast_kernel", "lutldpc_jit_pass", "tree_pass_kernel<VAR>") if k in used)


def _expected_kinds(cd, env):
    """(resident, skewed, check kernel) for alphabets of up to 16 labels; above, the variable tables leave the compile-time
    kernels and neither the resident decoder nor the skewed pipeline is promised (None: not asserted)."""
    nq = [int(q) for q in cd.nq_msg]
    pow2 = all(_pow2_half(q) for q in nq)
    fast = env.get("LUTLDPC_USE_FAST") != "0"
    resident = pow2 and fast and env.get("LUTLDPC_RESIDENT") != "0"
    skewed = pow2 and fast and cd.min_lut and env.get("LUTLDPC_SKEW") != "0"
    if _widest(cd) > 16:
        resident = None
        skewed = False
    if not cd.min_lut:
        cn = None
    elif not fast or not any(_pow2_half(q) for q in nq):
        cn = "cn_minsum_generic_kernel"
    elif pow2:
        cn = "cn_minsum_fast_kernel"
    else:
        cn = "cn_minsum_fast_kernel+cn_minsum_generic_kernel"
    return resident, skewed, cn


# (LUTLDPC_PACK=1 only where the alphabets allow two labels per byte: above 16 labels one per byte is the default)
@pytest.mark.parametrize("name,snr,modes,path", [(n, s, m, p) for n, s, m in CASES for p in PATHS if p != "pack1" or n != "reg36_n1000_q6"])
def test_decode_at_every_alphabet_matches_oracle(name, snr, modes, path, monkeypatch):
    cd = oracle_codec(name)
    env = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dec = product_decoder(cd)
    desc = dec.describe()
    resident, skewed, cn = _expected_kinds(cd, env)
    # (CHKTREE checks of degree 6 are decoded out of LDS too; they never take the skewed pipeline)
    if resident is not None:
        assert desc["resident"] == int(resident), desc
    if desc["resident"] == 0:
        assert desc["skewed_pipeline"] == int(skewed), desc
    if cn is not None:
        assert all(c["kernel"] == cn for c in desc["cn_classes"]), desc
        assert all(c["kernel"] == _expected_vn(cd, env) for c in desc["vn_classes"]), (desc, _expected_vn(cd, env))
    assert desc["pack"] == (1 if path == "pack1" or _widest(cd) > 16 else 2), desc
    print(name, path, {k: desc[k] for k in ("resident", "skewed_pipeline", "pack")}, desc["cn_classes"][0]["kernel"], desc["vn_classes"][0]["kernel"])
    for mode in modes:
        cd.set_initial_message_mode(mode)
        for B in BATCHES:
            cha, msg = _labels(name, snr, mode, B)
            for psc, pisc in EXITS:
                want_bits, want_it = _want(name, snr, mode, B, psc, pisc)
                dec.set_exit_conditions(cd.max_iters, psc, pisc)
                got_bits, got_it = dec.lut_decode_batch(cha, msg)
                assert (got_it == want_it).all(), (mode, B, psc, pisc, np.flatnonzero(got_it != want_it)[:8])
                bad = np.argwhere(got_bits != want_bits)
                assert bad.size == 0, (mode, B, psc, pisc, f"{len(bad)} bit mismatches, first at frame/bit {bad[:4].tolist()}")
                if B > 100 and psc and pisc:
                    assert len(set(want_it.tolist())) >= 3, sorted(set(want_it.tolist()))     # early exits, full runs, failures
                    assert want_it[0] == 0 and (want_it < 0).any()
    cd.set_initial_message_mode(0)
    dec.close()


@pytest.mark.parametrize("late", ["0", "1"])
def test_chain_fusion_and_compaction_with_a_shrinking_alphabet(late, monkeypatch):
    """Dual-diagonal code, schedule 8 8 8 8 4 4 4 2: chain fusion loads each iteration's degree-2 root table, compaction of the
    surviving frames forced at every second iteration (check points across the alphabet changes), ten frame groups.  The alphabet
    changes, so every variable pass stores the decided bits and the frames that left drop their rows whatever LUTLDPC_LATE_HARD says."""
    monkeypatch.setenv("LUTLDPC_RESIDENT", "0")
    for k, v in (("COMPACT", "1"), ("COMPACT_FIRST", "2"), ("COMPACT_EVERY", "2"), ("COMPACT_MARGIN", "0"), ("LATE_HARD", late)):
        monkeypatch.setenv("LUTLDPC_" + k, v)
    K, M = 1600, 400
    cd = designed_codec("test15-ira-ex8421", lambda path: write_ira_alist(path, K, M, 3, seed=K), sigma=0.5, max_iters=8, nq_msg=[8, 8, 8, 8, 4, 4, 4, 2])
    dec = product_decoder(cd)
    desc = dec.describe()
    assert desc["chain_nodes"] >= M // 2 and desc["skewed_pipeline"] == 1 and desc["compaction"] == 1, desc
    cha, msg, _ = awgn_labels(cd, 2500, 4.5, seed=77)
    cha[3] = 15; msg[3] = 7
    for psc, pisc in EXITS:
        cd.set_exit_conditions(8, psc, pisc)
        dec.set_exit_conditions(8, psc, pisc)
        want_bits, want_it = cd.lut_decode_batch_flat(cha, msg)
        got_bits, got_it = dec.lut_decode_batch(cha, msg)
        assert (got_it == want_it).all(), np.flatnonzero(got_it != want_it)[:8]
        assert (got_bits == want_bits).all(), np.argwhere(got_bits != want_bits)[:4]
        if psc and pisc:
            assert len(set(want_it.tolist())) >= 3 and (want_it < 0).any(), sorted(set(want_it.tolist()))
    dec.close()


def test_dvbs2_with_the_example_schedule():
    """N = 64800 with degree-1 nodes and the schedule 8 8 8 8 4 4 4 2: the default path, chain fusion off and the skewed pipeline
    off decode every frame alike, and a sample of frames equals the oracle."""
    import os
    alist = CODES / "rate0.50_irreg_dvbs2_N64800.alist"
    cd = designed_codec("test15-dvbs2-ex8421", alist, sigma=0.55, max_iters=8, nq_msg=[8, 8, 8, 8, 4, 4, 4, 2], rank=32400, allow_deg1=True)
    cha, msg, _ = awgn_labels(cd, 1100, 5.8, seed=64800)             # (eight iterations with 4- and 2-label messages need a high SNR)
    cha[5] = 15; msg[5] = 7
    got = {}
    for tag, env in (("default", {}), ("nochain", {"LUTLDPC_CHAIN": "0"}), ("noskew", {"LUTLDPC_SKEW": "0", "LUTLDPC_RESIDENT": "0"})):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            dec = product_decoder(cd)
            if tag == "default":
                assert dec.describe()["chain_nodes"] > 0, dec.describe()
            dec.set_exit_conditions(8, True, True)
            got[tag] = dec.lut_decode_batch(cha, msg)
            dec.close()
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    for tag in ("nochain", "noskew"):
        assert (got[tag][1] == got["default"][1]).all() and (got[tag][0] == got["default"][0]).all(), tag
    it = got["default"][1]
    kinds = sorted(set(it.tolist()))
    assert len(kinds) >= 3 and (it < 0).any(), kinds
    rng = np.random.default_rng(1)
    pick = sorted({int(np.flatnonzero(it == k)[0]) for k in kinds} | set(rng.choice(1100, 32, replace=False).tolist()))
    cd.set_exit_conditions(8, True, True)
    want_bits, want_it = cd.lut_decode_batch_flat(cha[pick], msg[pick])
    assert (want_it == it[pick]).all() and (want_bits == got["default"][0][pick]).all()


# ------------------------------------------------------------------------------------------------- front end
@pytest.mark.parametrize("name,mode", [("reg36_n1000_c2m4", 0), ("reg36_n1000_c2m4", 1), ("reg36_n1000_c4m4", 0), ("reg36_n1000_c4m4", 1),
                                       ("reg36_n1000_m2", 0), ("reg36_n1000_m2", 1), ("reg36_n1000_q5", 0), ("reg36_n1000_q5", 1),
                                       ("reg36_n1000_c32m8", 0), ("reg36_n1000_c32m8", 1), ("reg36_n1000_q6", 0), ("reg36_n1000_q6", 1)])
def test_device_sampler_matches_oracle_at_every_alphabet(name, mode):
    """sample_labels_kernel at one (PACK = 1) and two labels per byte, label for label, ragged B, frame numbers above 2**32."""
    ocd = oracle_codec(name)
    pcd = product_codec(name, device=0)
    assert pcd.var_trees_txt == ocd.var_tree_txt
    ocd.set_initial_message_mode(mode)
    pcd.set_initial_message_mode(mode)
    if name == "reg36_n1000_q6":
        assert len(pcd.channel_cells(3.0)["cha"]) == 64
    for snr, seed, stream, f0, B in [(2.0, 3, 0, 0, 300), (5.0, 2 ** 40 + 5, 7, 2 ** 33 + 3, 17)]:
        want_cha, want_msg, want_unc = ocd.sample_labels(snr, ocd.rate, seed, stream, f0, B)
        got_cha, got_msg, _ = pcd.sample_labels(snr, seed, stream, f0, B)
        assert (want_cha == got_cha).all() and (want_msg == got_msg).all()
    ocd.set_initial_message_mode(0)
    pcd.close()


@pytest.mark.parametrize("zero_codeword", [True, False])
@pytest.mark.parametrize("resident", ["1", "0"])
@pytest.mark.parametrize("nq,sig,snr", [(32, 0.84, 2.0), (4, 0.7, 4.5)])
def test_sim_batch_at_one_and_two_bit_labels_matches_oracle_frame_loop(nq, sig, snr, zero_codeword, resident, monkeypatch):
    """sim_batch (sampler, decode, count_errors_kernel, sent-bit rows of device codewords) at 32 labels (one label per byte) and
    4 labels, against the oracle's frame loop on the same codewords."""
    monkeypatch.setenv("LUTLDPC_RESIDENT", resident)
    I = 6
    alist = CODES / "rate0.50_dv03_dc06_N1000.alist"
    pcd = L.Codec(alist, with_generator=not zero_codeword, device=0)
    pcd.design_luts(sigma2=sig ** 2, max_iters=I, nq_cha=nq, nq_msg=nq)
    pcd.set_exit_conditions(I, True, True)
    assert pcd.decoder().describe()["pack"] == (1 if nq > 16 else 2)
    dv, dc, cn = pcd.graph()
    ref = orc.Codec(orc.Code(graph=(pcd.nvar, pcd.nchk, dv, dc, cn)), skip_rank=True)
    ref.set_rank(pcd.rank)
    ref.design_luts(sigma2=sig ** 2, max_iters=I, nq_cha=nq, nq_msg=np.full(I, nq, np.int32))
    assert ref.var_tree_txt == pcd.var_trees_txt
    ref.set_exit_conditions(I, True, True)
    seed, stream, B = 2 ** 33 + 12, 2, 600
    cw = None
    if not zero_codeword:
        _, _, cw = pcd.sample_labels(snr, seed, stream, 0, B, zero_codeword=False)
        assert cw.any()
        assert (pcd.encode_random(seed, stream, 0, B) == cw).all()
    want_c, want_per, _ = ref.sim_snr_point(snr, 1.0 - pcd.rank / pcd.nvar, pcd.ninfo, seed, stream, B, nfers=10 ** 9, codewords=cw)
    got = pcd.sim_batch(snr, seed, stream, 0, B, zero_codeword=zero_codeword)
    assert (got == want_per).all(), np.argwhere(got != want_per)[:5]
    assert (got[:, 1] > 0).any() and (got[:, 1] == 0).any() and (got[:, 2] > 0).any()
    pcd.close()


def test_encode_random_is_independent_of_the_alphabet():
    """encode_random on a decoder with 32-label alphabets (sent-bit rows of 256 frames) returns the codewords of a 16-label decoder
    and the oracle's information bits."""
    alist = CODES / "rate0.50_dv03_dc06_N1000.alist"
    seed, stream, f0, B = 2 ** 32 + 77, 3, 2 ** 32 + 5, 1100
    cws = {}
    for nq in (32, 16):
        pcd = L.Codec(alist, with_generator=True, device=0)
        pcd.design_luts(sigma2=0.84 ** 2, max_iters=4, nq_cha=nq, nq_msg=nq)
        assert pcd.decoder().describe()["pack"] == (1 if nq == 32 else 2)
        cws[nq] = pcd.encode_random(seed, stream, f0, B)
        K = pcd.ninfo
        pcd.close()
    assert (cws[32] == cws[16]).all()
    for i in (0, 1, 2, 3, 255, 256, 257, 700, B - 1):
        assert (cws[32][i, :K] == orc.info_bits(seed, stream, f0 + i, K)).all(), i


@pytest.mark.parametrize("name", ["reg36_n1000_c2m4", "reg36_n1000_c4m4", "reg36_n1000_m12", "reg36_n1000_q5"])
def test_device_quantiser_at_every_alphabet(name):
    """decode_llr_batch (the device quantiser) against quant_nonlin followed by the oracle decode, both initial-message modes, LLRs
    exactly on every boundary."""
    cd = oracle_codec(name)
    dec = product_decoder(cd)
    _, _, llr = awgn_labels(cd, 300, 3.0, seed=9)
    llr[3, :len(cd.qb_cha)] = cd.qb_cha                  # x <= b stops the scan
    llr[4, :len(cd.qb_msg)] = cd.qb_msg
    llr[5, :len(cd.qb_cha)] = -cd.qb_cha[::-1]
    cha, msg = orc.quant_nonlin(llr, cd.qb_cha), orc.quant_nonlin(llr, cd.qb_msg)
    cd.set_exit_conditions(cd.max_iters, True, True)
    dec.set_exit_conditions(cd.max_iters, True, True)
    want_bits, want_it = cd.lut_decode_batch(cha, msg)
    got_bits, got_it = dec.decode_llr_batch(llr, cd.qb_cha, cd.qb_msg, mode=0)
    assert (want_it == got_it).all() and (want_bits == got_bits).all()
    msg_q = cd.cha2msg_map[cha].astype(np.uint8)
    want_bits, want_it = cd.lut_decode_batch(cha, msg_q)
    got_bits, got_it = dec.decode_llr_batch(llr, cd.qb_cha, None, mode=1, cha2msg_map=cd.cha2msg_map)
    assert (want_it == got_it).all() and (want_bits == got_bits).all()
    dec.close()


def test_more_than_72_cells_is_refused_by_the_sampler():
    """The device cell table holds 72 cells: lutldpc_decoder_sim_batch / sample_labels refuse a bigger table with ERR_ARG and a
    message instead of truncating it."""
    cd = oracle_codec("reg36_n1000_q6")
    dec = product_decoder(cd)
    n = 100
    thr = np.sort(np.random.default_rng(0).integers(0, 2 ** 63, n - 1, dtype=np.uint64))
    lab = np.minimum(np.arange(n) * 64 // n, 63).astype(np.uint8)
    cells = ChannelCells.from_table({"thr": thr, "cha": lab, "msg": lab.copy(), "neg": (np.arange(n) < n // 2).astype(np.uint8), "cha_m": lab[::-1].copy(),
                                     "msg_m": lab[::-1].copy()})
    stats = np.zeros((10, 4), np.int32)
    rc = lib.lutldpc_decoder_sim_batch(dec._h, C.byref(cells), 1, 0, 0, 10, None, 500, stats.ctypes.data_as(C.POINTER(C.c_int32)), None, None)
    assert rc == ERR_ARG
    assert "72" in lib.lutldpc_last_error().decode()
    dec.close()


# ------------------------------------------------------------------------------------------------- end to end
def test_ber_sim_regular_example_with_its_message_schedule_matches_oracle(tmp_path):
    """data/params/ber.ini.regular.example with its commented-out `qbits_messages = 3 3 3 3 2 2 2 1` in force (Nframes raised):
    the C++ driver and lut_ldpc_amd.ber_sim.run equal the oracle's frame loop at every SNR point."""
    from lut_ldpc_amd import ber_sim
    for d in ("codes", "trees"):
        (tmp_path / d).mkdir()
    shutil.copy(CODES / "rate0.84_reg_v6c32_N2048.alist", tmp_path / "codes")
    shutil.copy(ROOT / "data" / "trees" / "6_32_wide.ini", tmp_path / "trees")
    ini = (ROOT / "data" / "params" / "ber.ini.regular.example").read_text()
    ini, n_sub = re.subn(r"(?m)^(\s*);+\s*(qbits_messages\s*=\s*3 3 3 3 2 2 2 1)", r"\1\2", ini)
    assert n_sub == 1 and "Nframes  = 20" in ini
    params = tmp_path / "ber.ini.regular.example"
    params.write_text(ini.replace("Nframes  = 20", "Nframes  = 300"))
    snr = (C.c_double * 32)(); cnt = (C.c_int64 * 160)()
    n = lib.lutldpc_ber_sim_run(str(params).encode(), str(tmp_path).encode(), 0, b"", 0, 1, 1, snr, cnt, 32)
    check(min(n, 0))
    got = np.array(cnt[:n * 5]).reshape(n, 5)
    pts, _ = ber_sim.run(params, tmp_path, seed=0, custom_name="_py", quiet=True)
    assert len(pts) == n and (np.array([c for _, c in pts]) == got).all()
    nq = np.array([8, 8, 8, 8, 4, 4, 4, 2], np.int32)
    pcd = L.Codec(CODES / "rate0.84_reg_v6c32_N2048.alist", with_generator=True, device=0)
    pcd.design_luts(tree_method=C5_TREES, sigma2=c5_sigma2(), max_iters=8, nq_cha=16, nq_msg=nq)
    ref = orc.Codec(oracle_graph(pcd), skip_rank=True)
    ref.set_rank(325)
    ref.design_luts(tree_method=C5_TREES, sigma2=c5_sigma2(), max_iters=8, nq_cha=16, nq_msg=nq)
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
