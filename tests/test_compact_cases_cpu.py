"""The cases of tests/compact_cases.py without a GPU: host-only handles and the oracle alone.  What
tests/test_60_entries_behind_compaction_gpu.py relies on is computed here, not claimed: every variant is on the streaming, skewed,
chain-fused path with compaction on at the batch sizes it decodes, and the inputs -- the planted batches and the sampled ones --
make frames move: in each half the surviving frames fit fewer groups at a check point, so a permutation happens."""
import numpy as np
import pytest

import compact_cases as cc


@pytest.mark.parametrize("variant", list(cc.VARIANTS))
def test_every_variant_is_on_the_path_it_names(variant, monkeypatch):
    dec, desc = cc.describe(cc.knobs(variant), monkeypatch)
    dec.close()
    cc.check_path(variant, desc, [cc.batch(variant, w) for w in cc.BATCHES])
    assert desc["fused_bucket"] == 0 and desc["compaction_min_groups"] == 4, desc
    assert [-(-cc.batch(variant, w) // cc.tile(variant)) for w in cc.BATCHES] == [6, 4]
    assert cc.batch(variant, "six") % cc.tile(variant) == 77                 # ragged last group


def _batches():
    """(id, frames, tile, labels, oracle's codes) of every batch the GPU file decodes: planted and sampled."""
    for B in cc.SIZES:
        T = 512 if B in (cc.batch("base", "six"), cc.batch("base", "four")) else 256
        yield f"awgn-{B}", B, T, lambda B=B: cc.labels(B)[0], lambda B=B: cc.want(B)[1]
    for src, which in (("zero", "four"), ("codewords", "four"), ("codewords", "six")):
        for v in cc.FULL_MATRIX:
            B = cc.batch(v, which)
            yield f"sampled-{src}-{B}", B, cc.tile(v), lambda B=B, src=src: cc.sampled(B, src)[0], lambda B=B, src=src: cc.want_sampled(B, src)[1]


BATCH_CASES = list(_batches())


@pytest.mark.parametrize("bid,B,T,cha,codes", BATCH_CASES, ids=[c[0] for c in BATCH_CASES])
def test_batches_make_frames_move(bid, B, T, cha, codes):
    """From the oracle's iteration codes alone: in each half, at some check point the frames still active fit fewer groups than were
    live before -- at two different check points for a batch of six groups; at least 20 frames fail and at least 8 different
    positive codes occur."""
    it = codes()
    G = -(-B // T)
    assert G in (4, 6)
    ev = cc.moves(it, B, T)
    assert len(ev) == 2 and all(len(e) >= (2 if G == 6 else 1) for e in ev), (bid, ev)
    assert all(cp in cc.CHECK_POINTS for e in ev for cp, _, _ in e)
    assert (it < 0).sum() >= 20 and len(set(it[it > 0].tolist())) >= 8, ((it < 0).sum(), sorted(set(it.tolist())))
    if bid.startswith("awgn"):
        assert (it[cc.planted(B)] == 0).all() and (it == 0).sum() == 3
    print(bid, "moves per half", ev, "failed", int((it < 0).sum()), "codes", sorted(set(it.tolist())))


@pytest.mark.parametrize("bid,B,T,cha,codes", BATCH_CASES, ids=[c[0] for c in BATCH_CASES])
def test_channel_rows_differ_pairwise(bid, B, T, cha, codes):
    """A frame-order error in returned labels cannot hide: no two frames carry the same channel labels (the three planted
    noise-free frames of a decode batch are the same frame: two of them are left out)."""
    rows = cha()
    if bid.startswith("awgn"):
        rows = np.delete(rows, cc.planted(B)[1:], axis=0)
    assert len(np.unique(rows, axis=0)) == len(rows)


def test_codewords_are_codewords_of_the_code_and_the_generator_makes_them():
    """The numpy encoder of the dual-diagonal code: every codeword satisfies the oracle's parity checks, holds the Philox data bits,
    and equals [u | A u] of the generator rows the device encoder is given."""
    import frontend_cases as fc
    cd = cc.codec()
    B = 40
    cw = cc.codewords(B)
    assert cw.shape == (B, cc.N) and 0.4 < cw.mean() < 0.6
    assert all(cd.syndrome_ok(cw[i]) for i in range(B))
    u = fc.info_bits(cc.SEED, cc.STREAM, cc.F0, B, cc.K_INFO)
    assert (cw == fc.encode(fc.generator_bits(cc.generator_rows(), cc.K_INFO), u)).all()
    assert cc.K_INFO + cc.R_GEN == cc.N and cc.generator_rows().shape == (cc.R_GEN, (cc.K_INFO + 63) // 64)


@pytest.mark.parametrize("which", list(cc.FITS_B))
def test_boundary_of_the_row_permutation(which, monkeypatch):
    """n500_q4_i8 in byte rows: halves of 32 groups are the most the row permutation takes; with 33 describe() still reports
    compaction forced on (the handle does not know the batch), and frames leave before the check points in both batches."""
    dec, desc = cc.describe(cc.FITS_KNOBS, monkeypatch, cd=cc.fits_codec())
    dec.close()
    want = {"resident": 0, "skewed_pipeline": 1, "compaction": 1, "pack": 1, "tile_frames": cc.FITS_TILE}
    assert {k: desc[k] for k in want} == want, desc
    B = cc.FITS_B[which]
    G = -(-B // cc.FITS_TILE)
    assert (G + 1) // 2 == (32 if which == "fits" else 33) and desc["compaction_min_groups"] == 4
    it = cc.fits_want(which)[1]
    assert cc.FITS_CHECK_POINTS == tuple(cp for cp in range(2, 8, 2) if cp < cc.fits_codec().max_iters - 2)
    ev = cc.moves(it, B, cc.FITS_TILE, cc.FITS_CHECK_POINTS)
    assert all(len(e) >= 1 for e in ev), ev                                  # (what a batch beyond the limit would do if it could)
    assert (it < 0).sum() >= 20 and (it == 0).sum() == 3 and len(set(it[it > 0].tolist())) >= 6
