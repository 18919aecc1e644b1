"""Every batch entry of the C-ABI behind a decode that compacts its frames (tests/compact_cases.py; tests/test_compact_cases_cpu.py
shows that the cases are on that path and that their inputs make frames move).  launch_compaction permutes the message rows and the
channel-label rows in place, launch_uncompaction brings back the decided bits and the iteration codes only: whatever an entry hands
out or counts after the decode -- sampled labels, histograms, statistics, windows of bits -- must still be in the caller's frame
order.  Every comparison is exact equality of integer arrays over ALL frames; every entry is called three times on one handle with
the same key (plain launches, graph capture, graph replay) and the three results are equal."""
import numpy as np
import pytest
import torch

import compact_cases as cc
from events_helpers import assert_equal, expected
from lut_ldpc_amd import msg_stats as ms
from lut_ldpc_amd import packing
from helpers import same as _same
from oracle import oracle as orc
from stats_helpers import hist_from_trace

pytestmark = pytest.mark.gpu

I, N, E = cc.ITERS, cc.N, cc.K * cc.DV + cc.M * 2
LEVEL = 2                                                  # the raw trace of a four-group batch stays below 100 MB
EXITS = ((True, True), (True, False))


# ---------------------------------------------------------------------------------------------------------------- helpers
def _handle(variant, monkeypatch, sizes=None, generator=False):
    """A fresh device handle of a variant (its first decode of a key runs plainly, its second captures, its third replays), on the
    path the case names."""
    dec, desc = cc.describe(cc.knobs(variant), monkeypatch, device=0)
    cc.check_path(variant, desc, sizes if sizes is not None else [cc.batch(variant, w) for w in cc.BATCHES])
    if generator:
        dec.set_generator(cc.K_INFO, cc.R_GEN, cc.generator_rows())
        assert dec.describe()["generator"] == {"K": cc.K_INFO, "R": cc.R_GEN}
    dec.set_exit_conditions(I, True, True)
    return dec


def _flat(x):
    if isinstance(x, (tuple, list)):
        return [a for y in x for a in _flat(y)]
    return [] if x is None else [np.asarray(x)]


def thrice(call, what=""):
    """The result of the first of three equal calls: plain launches, graph capture, graph replay."""
    runs = [_flat(call()) for _ in range(3)]
    for k, r in enumerate(runs[1:], 1):
        assert len(r) == len(runs[0])
        for j, (a, b) in enumerate(zip(runs[0], r)):
            assert a.shape == b.shape and (a == b).all(), (what, f"call {k + 1} differs from call 1 in result {j}", np.argwhere(a != b)[:4].tolist())
    return runs[0]


def _sim(dec, seed, stream, f0, B, cw, K, random=False, table=None):
    """(frame_stats, cha_out, bits_out) of sim_batch on host codewords (or none) or of sim_batch_random, each with two canary rows
    after frame B - 1 that must stay as they were."""
    stats, cha, bits = np.full((B + 2, 4), -7, np.int32), np.full((B + 2, dec.nvar), 0xEE, np.uint8), np.full((B + 2, dec.nvar), 0xEE, np.uint8)
    out = dec.sim_batch(table if table is not None else cc.cells(), seed, stream, f0, B, K, codewords=cw, random=random, frame_stats=stats, cha_out=cha, bits_out=bits)
    assert all(a is b for a, b in zip(out, (stats, cha, bits)))
    assert (stats[B:] == -7).all() and (cha[B:] == 0xEE).all() and (bits[B:] == 0xEE).all(), "rows after frame B - 1 were written"
    return stats[:B], cha[:B], bits[:B]


def _check_sim(got, B, source, what):
    """sim_batch's three results against the oracle's sampler and its decode of the sampled labels."""
    stats, cha_out, bits_out = got
    want_cha, _, want_unc = cc.sampled(B, source)
    want_bits, want_it = cc.want_sampled(B, source)
    sent = cc.codewords(B) if source == "codewords" else np.zeros((B, N), np.uint8)
    _same(cha_out, want_cha, what + ": cha_out against the sampled channel labels")
    _same(bits_out, want_bits, what + ": bits_out against the oracle's decode")
    _same(stats[:, 0], want_it, what + ": iteration codes")
    err = (bits_out[:, :cc.K_INFO] ^ sent[:, :cc.K_INFO]).sum(1)
    _same(stats[:, 1:3], np.stack([err > 0, err], axis=1).astype(np.int32), what + ": frame and data-bit errors")
    _same(stats[:, 3], want_unc, what + ": uncoded errors")


def _groups(by):
    c = cc.codec().code
    g, degrees = ms.edge_groups(c.dv, c.dc, c.cn_msg_idx, by)
    return g, len(degrees)


_EDGE_HIST = {}      # (tile, labels, mode, sent) -> int64 [dumps, E, 2, 16]: the trace counted per edge, once; a grouping is a sum of it


def _edge_hist(dec, T, kind, cha, msg, it, mode, sent):
    """The reference histogram per edge: the handle's own raw trace (exit tests off: no compaction) counted in numpy by
    stats_helpers.hist_from_trace with one group per edge; last_dump from the ORACLE's codes."""
    key = (T, kind, mode, sent is not None)
    if key not in _EDGE_HIST:
        dec.set_exit_conditions(I, False, False)
        _, _, trace = dec.lut_decode_batch_trace(cha, msg, LEVEL, E)
        dec.set_exit_conditions(I, True, True)
        last = ms.last_dump(it, I, LEVEL) if mode == "active" else np.full(len(it), ms.n_dumps(I, LEVEL))
        edge_vn = np.repeat(np.arange(N), np.asarray(cc.codec().code.dv, np.int64))
        h = hist_from_trace(trace, last, np.arange(E), E, 16, None if sent is None else sent[:, edge_vn])
        h.setflags(write=False)
        _EDGE_HIST[key] = h
    return _EDGE_HIST[key]


def _by_group(edge_hist, group, ng):
    out = np.zeros((edge_hist.shape[0], ng) + edge_hist.shape[2:], np.int64)
    for g in range(ng):
        out[:, g] = edge_hist[:, np.asarray(group) == g].sum(1)
    return out


def _hist_same(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape, (what, got.shape, want.shape)
    assert (got == want).all(), (what, "first (dump, group, sent, label)", np.argwhere(got != want)[:4].tolist())


SIM_CASES = [(v, w, s) for v in cc.FULL_MATRIX for w, s in (("four", "zero"), ("four", "codewords"), ("four", "random"), ("six", "codewords"))] + \
            [(v, "four", "codewords") for v in cc.OTHER]


# ---------------------------------------------------------------------------------------------------------------- 1. sim_batch
@pytest.mark.parametrize("variant,which,source", SIM_CASES, ids=["-".join(c) for c in SIM_CASES])
def test_sim_batch_returns_every_frame_its_own_labels_bits_and_counts(variant, which, source, monkeypatch):
    """lutldpc_decoder_sim_batch (zero codeword / host codewords) and lutldpc_decoder_sim_batch_random: cha_out equals the sampled
    labels frame for frame, bits_out and column 0 the oracle's decode of them, columns 1-2 recomputed from bits_out and the sent
    bits, column 3 the oracle's uncoded count; the rows after frame B - 1 stay untouched."""
    B = cc.batch(variant, which)
    dec = _handle(variant, monkeypatch, [B], generator=source == "random")
    src = "zero" if source == "zero" else "codewords"
    cw = cc.codewords(B) if source == "codewords" else None
    got = thrice(lambda: _sim(dec, cc.SEED, cc.STREAM, cc.F0, B, cw, cc.K_INFO, random=source == "random"), (variant, which, source))
    _check_sim(got, B, src, f"{variant} {which} {source}")
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- 2. histogram_batch
@pytest.mark.parametrize("with_sent", [False, True], ids=["zero_codeword", "sent"])
@pytest.mark.parametrize("mode", ["active", "all"])
@pytest.mark.parametrize("variant", cc.FULL_MATRIX)
def test_histogram_batch_counts_every_frame_under_its_own_code(variant, mode, with_sent, monkeypatch):
    """lutldpc_decoder_histogram_batch on the four-group batch: the normal decode inside the call compacts, so the counted decode
    after it needs the labels written again (decode_moves_labels -> refill()); with decode=True the bits and codes of the call are
    the oracle's."""
    B, T = cc.batch(variant, "four"), cc.tile(variant)
    cha, msg = cc.labels(B)
    want_bits, want_it = cc.want(B)
    sent = cc.codewords(B) if with_sent else None
    dec = _handle(variant, monkeypatch, [B])
    ref = _edge_hist(dec, T, "awgn", cha, msg, want_it, mode, sent)
    for by in ("vn", "cn"):
        group, ng = _groups(by)
        dec.set_edge_groups(group, ng)
        want = _by_group(ref, group, ng)
        assert want.sum() > 0 and (not with_sent or want[:, :, 1].sum() > 0)
        hist, bits, it = thrice(lambda: dec.message_histogram(cha, msg, sent=sent, level=LEVEL, mode=mode), (variant, mode, by))
        _same(it, want_it, "iteration codes of the call")
        _same(bits, want_bits, "decided bits of the call")
        _hist_same(hist, want, (variant, mode, by, "decode=True"))
        hist, = thrice(lambda: dec.message_histogram(cha, msg, sent=sent, level=LEVEL, mode=mode, decode=False), (variant, mode, by))
        _hist_same(hist, want, (variant, mode, by, "decode=False"))
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- 3. sim_batch_histogram
def _sim_hist(dec, f0, B, cw, on_device, hist=None):
    return dec.sim_batch_histogram(cc.cells(), cc.SEED, cc.STREAM, f0, B, codewords=cw, device_codewords=on_device, level=LEVEL, mode="active", hist=hist)


@pytest.mark.parametrize("source", ["zero", "device_codewords"])
@pytest.mark.parametrize("variant", cc.FULL_MATRIX)
def test_sim_batch_histogram_samples_again_after_a_compacting_decode(variant, source, monkeypatch):
    """lutldpc_decoder_sim_batch_histogram, mode "active": against the trace of the labels the oracle's sampler returns for the same
    (seed, stream, frame0); and the same frames over two calls (the first compacts, the second is a single group) into one array."""
    B, T = cc.batch(variant, "four"), cc.tile(variant)
    src = "zero" if source == "zero" else "codewords"
    cha, msg, _ = cc.sampled(B, src)
    _, want_it = cc.want_sampled(B, src)
    sent = cc.codewords(B) if src == "codewords" else None
    dec = _handle(variant, monkeypatch, [B], generator=source != "zero")
    group, ng = _groups("vn")
    dec.set_edge_groups(group, ng)
    want = _by_group(_edge_hist(dec, T, "sampled-" + src, cha, msg, want_it, "active", sent), group, ng)
    assert (sent is None) == (want[:, :, 1].sum() == 0)
    hist, = thrice(lambda: _sim_hist(dec, cc.F0, B, None, source != "zero"), (variant, source))
    _hist_same(hist, want, (variant, source))
    B1 = 3 * T + 5
    two = _sim_hist(dec, cc.F0, B1, None, source != "zero")
    assert _sim_hist(dec, cc.F0 + B1, B - B1, None, source != "zero", hist=two) is two
    _hist_same(two, want, (variant, source, "two calls"))
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- 4, 6 and the plain entry
def _device_decode(dec, cha, msg):
    d_cha, d_msg = torch.from_numpy(np.array(cha)).to("cuda:0"), torch.from_numpy(np.array(msg)).to("cuda:0")
    bits = torch.full(cha.shape, 0xEE, dtype=torch.uint8, device="cuda:0")
    it = torch.full((len(cha),), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    dec.lut_decode_batch_device(d_cha.data_ptr(), d_msg.data_ptr(), len(cha), bits.data_ptr(), it.data_ptr(), sync=True)
    assert (d_cha.cpu().numpy() == cha).all() and (d_msg.cpu().numpy() == msg).all(), "the caller's device labels were written"
    return bits.cpu().numpy(), it.cpu().numpy()


DECODE_CASES = [(v, w) for v in cc.VARIANTS for w in cc.BATCHES]


@pytest.mark.parametrize("variant,which", DECODE_CASES, ids=["-".join(c) for c in DECODE_CASES])
def test_decode_entries_byte_packed_and_device(variant, which, monkeypatch):
    """lut_decode_batch, decode_batch_packed (nibble and byte input, the initial messages through cha2msg_map on the device, a window
    of the bits out) and decode_batch_device (torch tensors in and out) against the oracle's flat decode, psc = pisc = 1 and
    psc = 1, pisc = 0."""
    B = cc.batch(variant, which)
    cd = cc.codec()
    cha, msg = cc.labels(B)
    qmsg = cd.cha2msg_map[cha].astype(np.uint8)
    first, count = 1, cc.K_INFO + 30                                      # a window that begins and ends inside a word
    dec = _handle(variant, monkeypatch, [B])
    for psc, pisc in EXITS:
        dec.set_exit_conditions(I, psc, pisc)
        want_bits, want_it = cc.want(B, psc, pisc)
        for name, call in (("byte", lambda: dec.lut_decode_batch(cha, msg)), ("device", lambda: _device_decode(dec, cha, msg))):
            bits, it = thrice(call, (variant, which, name, pisc))
            _same(it, want_it, f"{name} pisc={pisc}: iteration codes")
            _same(bits, want_bits, f"{name} pisc={pisc}: decided bits")
        qbits, qit = cc.oracle_decode("qcha", cha, qmsg, psc, pisc)
        for nibbles in (True, False):
            src = packing.pack_nibbles(cha) if nibbles else cha
            words, it = thrice(lambda: dec.decode_packed(src, cha2msg_map=cd.cha2msg_map, nibbles=nibbles, first=first, count=count), (variant, which, nibbles))
            _same(it, qit, f"packed nibbles={nibbles} pisc={pisc}: iteration codes")
            _same(packing.unpack_bits(words, count), qbits[:, first:first + count], f"packed nibbles={nibbles} pisc={pisc}: window of the bits")
    assert not cha.flags.writeable and not msg.flags.writeable
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- 5. decode_llr_packed
@pytest.mark.parametrize("which", cc.BATCHES)
@pytest.mark.parametrize("variant", cc.FULL_MATRIX)
def test_decode_llr_packed_hands_out_labels_in_frame_order(variant, which, monkeypatch):
    """float32 LLRs from host memory and from a device tensor, out_cha / out_msg0 requested: the labels are the oracle's quant_nonlin
    of the values, the bits and codes the oracle's decode of those labels."""
    from helpers import awgn_labels
    B = cc.batch(variant, which)
    cd = cc.codec()
    llr = awgn_labels(cd, B, cc.snr(), seed=cc.LABEL_SEED[B])[2].astype(np.float32)
    llr[cc.planted(B)] = 100.0
    want_cha, want_msg = orc.quant_nonlin(llr.astype(np.float64), cd.qb_cha), orc.quant_nonlin(llr.astype(np.float64), cd.qb_msg)
    want_bits, want_it = cc.oracle_decode("llr32", want_cha, want_msg)
    assert (want_it[cc.planted(B)] == 0).all() and len(set(want_it.tolist())) > 8 and len(cc.moves(want_it, B, cc.tile(variant))[0]) >= 1
    dec = _handle(variant, monkeypatch, [B])
    for device in (False, True):
        def call():
            src = torch.from_numpy(llr.copy()).to("cuda:0") if device else llr
            out = dec.decode_llr(src, cd.qb_cha, qb_msg=cd.qb_msg, want_labels=True)
            return tuple(o.cpu().numpy() if isinstance(o, torch.Tensor) else o for o in out)
        words, it, cha, msg = thrice(call, (variant, which, device))
        _same(cha, want_cha, f"device={device}: out_cha")
        _same(msg, want_msg, f"device={device}: out_msg0")
        _same(it, want_it, f"device={device}: iteration codes")
        _same(packing.unpack_bits(words.view(np.uint32), N), want_bits, f"device={device}: decided bits")
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- 7. a sequence of calls
@pytest.mark.parametrize("variant", cc.FULL_MATRIX)
def test_one_handle_through_a_sequence_of_calls(variant, monkeypatch):
    """Compacting decode, fixed-work decode, a batch below four groups, histogram_batch, error_events, sim_batch with cha_out, the
    first decode again: every step equals its reference, the last equals the first bit for bit, the caller's arrays are unchanged."""
    B, T = cc.batch(variant, "four"), cc.tile(variant)
    cha0, msg0 = cc.labels(B)
    cha, msg = cha0.copy(), msg0.copy()
    want_bits, want_it = cc.want(B)
    c = cc.codec().code
    dec = _handle(variant, monkeypatch, [B])
    group, ng = _groups("vn")                             # (the reference of step 4: a trace, exit tests off, plain launches)
    ref = _by_group(_edge_hist(dec, T, "awgn", cha0, msg0, want_it, "active", None), group, ng)
    first = dec.lut_decode_batch(cha, msg)                                                      # 1. compacting decode
    _same(first[1], want_it, "step 1: iteration codes")
    _same(first[0], want_bits, "step 1: decided bits")
    dec.set_exit_conditions(I, False, False)                                                    # 2. fixed-work decode
    bits, it = dec.lut_decode_batch(cha, msg)
    fixed = cc.want(B, False, False)
    _same(it, fixed[1], "step 2: iteration codes")
    _same(bits, fixed[0], "step 2: decided bits")
    dec.set_exit_conditions(I, True, True)
    Bs = T + 5                                                                                  # 3. below four groups: no compaction
    assert -(-Bs // T) < dec.describe()["compaction_min_groups"]
    bits, it = dec.lut_decode_batch(cha[:Bs], msg[:Bs])
    _same(it, want_it[:Bs], "step 3: iteration codes")
    _same(bits, want_bits[:Bs], "step 3: decided bits")
    dec.set_edge_groups(group, ng)                                                              # 4. histogram_batch, mode "active"
    hist, bits, it = dec.message_histogram(cha, msg, level=LEVEL, mode="active")
    _same(it, want_it, "step 4: iteration codes")
    _same(bits, want_bits, "step 4: decided bits")
    _hist_same(hist, ref, "step 4")
    ev = dec.error_events(cha, msg, select="codeword", max_frames=B, max_pos=32, max_chk=32, profiles=True, k_info=cc.K_INFO)     # 5. error_events
    assert_equal(ev, expected(want_bits, None, want_it, (c.dv, c.dc, c.cn_msg_idx), cc.K_INFO, "codeword", B, 32, 32), "step 5")
    assert ev.n_selected >= 20
    _check_sim(_sim(dec, cc.SEED, cc.STREAM, cc.F0, B, None, cc.K_INFO), B, "zero", "step 6")  # 6. sim_batch with cha_out
    last = dec.lut_decode_batch(cha, msg)                                                       # 7. the first decode again
    _same(last[1], first[1], "step 7: iteration codes")
    _same(last[0], first[0], "step 7: decided bits")
    assert (cha == cha0).all() and (msg == msg0).all(), "the caller's label arrays were written"
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- 8. compaction_fits
@pytest.mark.parametrize("which,entry", [("fits", "decode"), ("beyond", "decode"), ("beyond", "sim_batch")])
def test_boundary_of_compaction_fits(which, entry, monkeypatch):
    """n500_q4_i8 in byte rows: halves of 32 groups (compaction runs) and of 33 (compaction_on is false: the decode must still be
    right) against the oracle's flat decode; the batch beyond the limit also through sim_batch with cha_out."""
    cd = cc.fits_codec()
    dec, desc = cc.describe(cc.FITS_KNOBS, monkeypatch, device=0, cd=cd)
    want = {"resident": 0, "skewed_pipeline": 1, "compaction": 1, "pack": 1, "tile_frames": cc.FITS_TILE, "compaction_min_groups": 4}
    assert {k: desc[k] for k in want} == want, desc
    B = cc.FITS_B[which]
    dec.set_exit_conditions(cd.max_iters, True, True)
    if entry == "decode":
        cha, msg = cc.fits_labels(which)
        want_bits, want_it = cc.fits_want(which)
        bits, it = thrice(lambda: dec.lut_decode_batch(cha, msg), which)
        _same(it, want_it, "iteration codes")
        _same(bits, want_bits, "decided bits")
    else:
        K = cd.code.nvar - cd.code.nchk
        scha, smsg, unc = cd.sample_labels(cc.FITS_SNR, cd.rate, cc.SEED, cc.STREAM, cc.F0, B)
        cd.set_exit_conditions(cd.max_iters, True, True)
        sbits, sit = cd.lut_decode_batch_flat(scha, smsg)
        assert (sit < 0).sum() >= 20 and len(set(sit.tolist())) >= 6
        stats, cha_out, bits_out = thrice(lambda: _sim(dec, cc.SEED, cc.STREAM, cc.F0, B, None, K, table=cd.channel_cells(cc.FITS_SNR, cd.rate)), which)
        _same(cha_out, scha, "cha_out against the sampled channel labels")
        _same(bits_out, sbits, "bits_out")
        err = bits_out[:, :K].sum(1)
        _same(stats, np.stack([sit, err > 0, err, unc], axis=1).astype(np.int32), "frame_stats")
    dec.close()
