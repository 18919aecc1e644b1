"""The variants of the generated LDS-resident kernel (jit_resident.hpp) that resident_spec never chooses for the codes of the other
tests, and the degree limits of resident_eligible.  The generator branches on LUTLDPC_RESIDENT_U / _FLAG_REDUCE / _CN_PERSISTENT /
_XCD / _FM / _WAVES_EU; unset, each code runs one side of every branch, picked from thresholds that are retuned by measurement.
Here every knob runs at every value it takes on a nibble-row, a byte-row, a mixed-alphabet, a CHKTREE and a wide-check code, the
reduced exit-test flags run with waves that straddle two sets, the XCD remap runs on a ragged grid, and synthetic codes walk the
limits (check degree 17 / 33 / 63-64 / 65, variable degree 24 / 25, degree-1 nodes, 12 / 13 degree classes) -- every case after
asserting, from the source its decode compiles, that the variant and the geometry it names are the ones in effect.  Then the
kernel's two I/O paths (frame-major buffers of the caller / row layout) and the device-pointer entry bench.py times.
Bit-exact against the oracle in the three exit modes; the oracle decodes a batch once per mode for all variants
(tests/resident_cases.py, whose cases tests/test_resident_variants_cpu.py generates and compiles without a GPU)."""
import numpy as np
import pytest

import resident_cases as rc
from helpers import awgn_labels, compare, product_decoder

pytestmark = pytest.mark.gpu


def _decode_case(monkeypatch, name, kn, B, snr, auto=None, flat=False, seed=None, resident=1):
    """One case: the knobs, then the decoder (knobs are read once, at creation); variant and geometry checked on the source the
    decode will compile; all three exit modes against the (shared) oracle result.  Returns (decoder description, S, iteration codes)."""
    cd = rc.codec(name)
    if resident:
        auto = auto or rc.auto_variant(name, B, kn)
    for k, v in kn.items():
        monkeypatch.setenv(k, v)
    dec = product_decoder(cd)
    desc = dec.describe()
    assert desc["resident"] == resident, desc
    S = 0
    if resident:
        _, S, _, _ = rc.check_source(dec, name, B, kn, auto)
    cha, msg = rc.labels(name, B, snr, seed)
    its = [compare(cd, dec, cha, msg, psc, pisc, flat=flat, cache=rc.oracle_cache(name)) for psc, pisc in rc.EXIT_MODES]
    assert (its[0] == 0).sum() >= 3                               # the planted frames pass the test on the channel decisions
    dec.close()
    return desc, S, its[0]


@pytest.mark.parametrize("name,vid,kn", rc.MATRIX, ids=[f"{n}-{v}" for n, v, _ in rc.MATRIX])
def test_variant_matrix(name, vid, kn, monkeypatch):
    """Every knob at every value on every code structure; `flipped`: all of them away from the code's automatic choice at once.
    (c5_minlut-cnp1: the wide min-sum with register addresses; n500_q4_i8-flag1: the reduced flags with degree-17 items.)"""
    B, snr = rc.CODES[name]
    auto = rc.auto_variant(name, B, {})
    kn = rc.flipped_knobs(auto) if vid == rc.FLIPPED else kn
    desc, S, it = _decode_case(monkeypatch, name, kn, B, snr, auto)
    assert len(set(it.tolist())) >= 3
    if vid == "xcd0":                                             # the remap switched off on a grid it would have remapped
        assert (64 * ((B + desc["tile_frames"] - 1) // desc["tile_frames"]) + S - 1) // S % 8 == 0


@pytest.mark.parametrize("cid,name,kn,B,snr,flat,grid8", rc.GEOMETRY, ids=[c[0] for c in rc.GEOMETRY])
def test_variants_that_need_a_forced_geometry(cid, name, kn, B, snr, flat, grid8, monkeypatch):
    """Several sets per workgroup (automatic geometry gives S = 1 below about 2000 frames): waves whose lanes work on two sets take
    the per-lane fallback of res_flag, the others its ballot branch, inside one launch; the XCD remap on a grid of 24 workgroups
    whose last one lies mostly beyond the batch; the remap refused by its own test on 22 workgroups."""
    desc, S, it = _decode_case(monkeypatch, name, kn, B, snr, flat=flat)
    assert S > 1 and ((64 * ((B + desc["tile_frames"] - 1) // desc["tile_frames"]) + S - 1) // S % 8 == 0) == grid8
    assert len(set(it.tolist())) >= 3


# what describe() says about the streaming kernels of the wide-check codes today: checks wider than kFastMaxCnDeg = 32 run
# cn_minsum_generic_kernel beside the specialised variable kernels, and have no case in the fused (skewed) pipeline
STREAMING = {"dc17": (1, "cn_minsum_fast_kernel"), "dc33": (0, "cn_minsum_generic_kernel"), "dc64": (0, "cn_minsum_generic_kernel"),
             "dc65": (0, "cn_minsum_generic_kernel")}


@pytest.mark.parametrize("cid,name,kn,resident", rc.LIMIT_CASES, ids=[c[0] for c in rc.LIMIT_CASES])
def test_degree_limits(cid, name, kn, resident, monkeypatch):
    """resident_eligible: check degree 2..64, variable degree <= 24, at most 12 degree classes per side.  Inside the limits the
    resident kernel decodes (odd wide checks: the (deg & 1) sign term of emit_wide_minsum; degree-1 nodes; 24 inputs per tree),
    one step past them the default dispatch hands the code to the streaming kernels.  Both sides bit-exact."""
    desc, _, it = _decode_case(monkeypatch, name, kn, rc.LIMIT_B, rc.limit_snr(name), seed=rc.LABEL_SEED, resident=resident)
    assert len(set(it.tolist())) >= 3, sorted(set(it.tolist()))
    if name in STREAMING:
        skew, kernel = STREAMING[name]
        assert desc["skewed_pipeline"] == skew, desc
        assert {c["kernel"] for c in desc["cn_classes"]} == {kernel} and {c["kernel"] for c in desc["vn_classes"]} == {"vn_balanced_fast_kernel"}, desc


# ---- the kernel's two I/O paths: fm_load / fm_store on the caller's frame-major buffers (FM = 1), the transposes (FM = 0)

@pytest.mark.parametrize("fm", ["1", "0"])
def test_out_of_range_labels_are_clamped_on_both_io_paths(fm, monkeypatch):
    """Labels outside the alphabet are clamped to the largest label, by fm_load (FM = 1) or by the transposes (FM = 0): in frame 5
    and in the only frame of the last, partial set.  The other frames decode as without them, the bad frames as their clamped
    labels, and everything equals the oracle on the clamped labels."""
    monkeypatch.setenv(rc.K + "FM", fm)
    name, B = "n500_q4_i8", 700 - 3
    cd = rc.codec(name)
    dec = product_decoder(cd)
    assert dec.describe()["resident"] == 1 and B % 8 == 1
    cha, msg, _ = awgn_labels(cd, B, 2.0, seed=31)              # (no planted frames: B - 1 must decode, not pass at once)
    bad_c, bad_m = cha.copy(), msg.copy()
    for f in (5, B - 1):
        bad_c[f, ::3] = 200
        bad_m[f, 1::3] = 255
        bad_c[f, 2::7] = 16                                       # one past the alphabet
    clamp_c, clamp_m = np.minimum(bad_c, cd.nq_cha - 1), np.minimum(bad_m, cd.nq_msg[0] - 1)
    for psc, pisc in rc.EXIT_MODES:
        compare(cd, dec, clamp_c, clamp_m, psc, pisc, flat=True, cache=rc.oracle_cache(name))
        want_bits, want_it = dec.lut_decode_batch(clamp_c, clamp_m)
        bits, it = dec.lut_decode_batch(bad_c, bad_m)
        assert (bits == want_bits).all() and (it == want_it).all()
        good_bits, good_it = dec.lut_decode_batch(cha, msg)
        keep = ~np.isin(np.arange(B), (5, B - 1))
        assert (bits[keep] == good_bits[keep]).all() and (it[keep] == good_it[keep]).all()
    dec.close()


@pytest.mark.parametrize("fm", ["1", "0"])
def test_batches_around_one_set(fm, monkeypatch):
    """One frame of a set, one short of a set, one over -- frames beyond B read as label 0 and are never stored."""
    monkeypatch.setenv(rc.K + "FM", fm)
    name = "n500_q4_i8"
    cd = rc.codec(name)
    dec = product_decoder(cd)
    assert dec.describe()["resident"] == 1
    cha, msg = rc.labels(name, 9, 2.0)
    for B in (1, 7, 9):
        for psc, pisc in rc.EXIT_MODES:
            compare(cd, dec, cha[:B], msg[:B], psc, pisc, cache=rc.oracle_cache(name))
    dec.close()


def test_fm_knob_selects_the_io_path(monkeypatch):
    """LUTLDPC_RESIDENT_FM leaves the kernel's text alone (both paths are in every source, chosen by the fm_* arguments): that the
    knob is in effect shows in the launch profile -- one resident launch either way, the transposes around it only with FM = 0."""
    name = "n500_q4_i8"
    cd = rc.codec(name)
    cha, msg = rc.labels(name, 9, 2.0)
    layout = {}
    for fm in ("1", "0"):
        monkeypatch.setenv(rc.K + "FM", fm)
        dec = product_decoder(cd)
        dec.lut_decode_batch(cha, msg)                            # (compiles the kernel, allocates)
        dec.set_profiling(True)
        dec.reset_profile()
        dec.lut_decode_batch(cha, msg)
        prof = dec.profile()
        assert prof["resident"]["launches"] == 1, prof
        layout[fm] = prof["layout"]["launches"]
        dec.close()
    assert layout["0"] > layout["1"], layout


@pytest.mark.parametrize("resident", ["1", "0"])
def test_device_pointer_entry(resident, monkeypatch):
    """Decoder.lut_decode_batch_device on torch tensors, the entry bench.py times: with the resident decoder the kernel reads the
    caller's label tensors and writes the caller's bit tensor itself.  One synchronous call, then two asynchronous ones and a
    synchronous one on different tensors: every output equals the oracle, the inputs are unchanged, and the bytes right behind
    the B rows of every output keep their pattern (fm_store guards on f < A.B: B = 203 leaves five frames of the last set)."""
    import torch
    monkeypatch.setenv("LUTLDPC_RESIDENT", resident)
    name, B = "n500_q4_i8", 203
    cd = rc.codec(name)
    N = cd.code.nvar
    dec = product_decoder(cd)
    assert dec.describe()["resident"] == int(resident)
    cd.set_exit_conditions(cd.max_iters, True, True)
    dec.set_exit_conditions(cd.max_iters, True, True)
    dev = torch.device("cuda", 0)
    PAD, CANARY = 4096, 0xA5
    jobs = []
    for k in range(4):
        cha, msg = rc.labels(name, B, 2.0, seed=70 + k)
        want = cd.lut_decode_batch_flat(cha, msg)
        t_cha, t_msg = torch.from_numpy(cha.copy()).to(dev), torch.from_numpy(msg.copy()).to(dev)
        # B rows exactly, the canary right behind them (filled on the host: copies only, none of torch's own kernels is needed)
        bits = torch.from_numpy(np.full(B * N + PAD, CANARY, np.uint8)).to(dev)
        iters = torch.from_numpy(np.full(B + PAD, -77, np.int32)).to(dev)
        jobs.append((cha, msg, want, t_cha, t_msg, bits, iters))
    torch.cuda.synchronize()
    for k, sync in enumerate([True, False, False, True]):
        _, _, _, t_cha, t_msg, bits, iters = jobs[k]
        dec.lut_decode_batch_device(t_cha.data_ptr(), t_msg.data_ptr(), B, bits.data_ptr(), iters.data_ptr(), sync=sync)
        if k == 0:                                                # the synchronous call alone: complete when it returns
            assert (iters[:B].cpu().numpy() == jobs[0][2][1]).all()
    for k, (cha, msg, (want_bits, want_it), t_cha, t_msg, bits, iters) in enumerate(jobs):
        got_bits, got_it = bits.cpu().numpy(), iters.cpu().numpy()
        assert (got_it[:B] == want_it).all(), k
        assert (got_bits[:B * N].reshape(B, N) == want_bits).all(), k
        assert (got_bits[B * N:] == CANARY).all() and (got_it[B:] == -77).all(), k
        assert (t_cha.cpu().numpy() == cha).all() and (t_msg.cpu().numpy() == msg).all(), k
    assert len({tuple(j[2][1].tolist()) for j in jobs}) == 4      # four different batches: no output can stand in for another
    dec.close()
