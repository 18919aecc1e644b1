"""The resident decoder's variant matrix and degree limits (tests/resident_cases.py) without a GPU: on a host-only handle every
(code, variant, geometry) that tests/test_07_resident_variants_gpu.py decodes generates its kernel, hiprtc cross-compiles it for
gfx950, the source reports the requested variant (a knob that stops reaching the generator fails here, on every machine) and the
LDS stays within the budget.  Also what the knob table documents as ignored: U = 3 and a thread count that is no multiple of 256."""
import pytest

import resident_cases as rc
from helpers import product_decoder, resident_variant

_compiled = set()      # sources hiprtc has accepted in this session: equal text is compiled once


def _generate(monkeypatch, name, B, kn, auto=None):
    auto = auto or rc.auto_variant(name, B, kn)
    for k, v in kn.items():
        monkeypatch.setenv(k, v)
    dec = product_decoder(rc.codec(name), device=-1)
    G = rc.frame_groups(dec, B)
    src, S, NT, lds = rc.check_source(dec, name, B, kn, auto)
    if src not in _compiled:
        assert dec.resident_source(G, compile=True)[0] == src
        _compiled.add(src)
    dec.close()
    return src, S, NT


@pytest.fixture
def clean_env(monkeypatch):
    import os
    for k in [k for k in os.environ if k.startswith(rc.K)]:
        monkeypatch.delenv(k)
    return monkeypatch


@pytest.mark.parametrize("name,vid,kn", rc.MATRIX, ids=[f"{n}-{v}" for n, v, _ in rc.MATRIX])
def test_variant_generates_compiles_and_reports_itself(name, vid, kn, clean_env):
    B = rc.CODES[name][0]
    auto = rc.auto_variant(name, B, {})
    kn = rc.flipped_knobs(auto) if vid == rc.FLIPPED else kn
    src, S, NT = _generate(clean_env, name, B, kn, auto)
    if vid == rc.FLIPPED:
        got = resident_variant(src)
        assert got["flag_reduce"] != auto["flag_reduce"] and got["xcd"] == 0 and got["waves_eu"] == 2 and got["U"] == {4}
        assert got["cn_persistent"] != auto["cn_persistent"] or not rc.codec(name).min_lut


@pytest.mark.parametrize("cid,name,kn,B", [(c[0], c[1], c[2], c[3]) for c in rc.GEOMETRY], ids=[c[0] for c in rc.GEOMETRY])
def test_forced_geometry_generates_and_is_kept(cid, name, kn, B, clean_env):
    want8 = {c[0]: c[6] for c in rc.GEOMETRY}[cid]
    src, S, NT = _generate(clean_env, name, B, kn)
    dec = product_decoder(rc.codec(name), device=-1)
    assert (rc.workgroups(dec, B, S) % 8 == 0) == want8           # the XCD remap tests the grid itself: (nb & 7) == 0
    if cid == "xcd1_ragged_grid":
        assert rc.workgroups(dec, B, S) == 24 and (64 * rc.frame_groups(dec, B)) % S != 0
    dec.close()


_RESIDENT_LIMIT_CASES = [c for c in rc.LIMIT_CASES if "LUTLDPC_RESIDENT" not in c[2]]      # (the others decode with the streaming kernels)


@pytest.mark.parametrize("cid,name,kn,resident", _RESIDENT_LIMIT_CASES, ids=[c[0] for c in _RESIDENT_LIMIT_CASES])
def test_limit_shape_generates_and_compiles(cid, name, kn, resident, clean_env):
    """(resident_source does not ask resident_eligible: the shapes one step past the limits generate too -- they are refused at
    creation, which the GPU tests assert through describe().)"""
    _generate(clean_env, name, rc.LIMIT_B, kn)


def test_limit_codes_hold_the_degrees_they_are_named_for():
    want_dc = {"dc17": {17}, "dc33": {33}, "dc64": {63, 64}, "dc65": {65}}
    for name, dc in want_dc.items():
        assert set(rc.codec(name).code.dc.tolist()) == dc, name
    for name, top, n in (("dv24", 24, 3), ("dv25", 25, 3), ("deg1", 6, 4), ("cls12", 13, 12), ("cls13", 14, 13)):
        dv = set(rc.codec(name).code.dv.tolist())
        assert max(dv) == top and len(dv) == n, (name, dv)
    assert min(rc.codec("deg1").code.dv.tolist()) == 1


@pytest.mark.parametrize("name", sorted(rc.LIMITS))
def test_limit_batches_tell_decoders_apart(name):
    """The condition the GPU cases rely on, checked with the oracle alone: with the planted noise-free frames the iteration codes
    of every limit batch hold at least three distinct values."""
    cd = rc.codec(name)
    cha, msg = rc.labels(name, rc.LIMIT_B, rc.limit_snr(name), rc.LABEL_SEED)
    cd.set_exit_conditions(cd.max_iters, True, True)
    _, it = cd.lut_decode_batch_flat(cha, msg)
    assert len(set(it.tolist())) >= 3 and (it == 0).sum() >= 3, sorted(set(it.tolist()))


@pytest.mark.parametrize("name", ["n500_q4_i8", "reg36_n1000_q5"])
def test_ignored_knob_values_fall_back_to_the_automatic_choice(name, clean_env):
    """LUTLDPC_RESIDENT_U=3 and a LUTLDPC_RESIDENT_NT that is no multiple of 256 are ignored: the same source, the same geometry
    as with the variable unset; the accepted neighbours change the source."""
    def source(**kw):
        with pytest.MonkeyPatch.context() as mp:
            for k, v in rc.knobs(**kw).items():
                mp.setenv(k, v)
            dec = product_decoder(rc.codec(name), device=-1)
            out = dec.resident_source(1)
            dec.close()
        return out
    unset = source()
    assert source(U=3) == unset
    assert source(U=4) != unset and resident_variant(source(U=4)[0])["U"] == {4}
    assert source(NT=300) == unset and source(NT=1000) == unset and source(NT=128) == unset
    assert source(NT=768)[1][1] == 768
    assert source(WAVES_EU=9) == unset and source(S=65) == unset


def test_resident_variant_reads_every_marker(clean_env):
    """resident_variant on the two sources that differ in every marker."""
    auto = rc.auto_variant("n500_q4_i8", 301, {})
    assert auto["xcd"] == 1 and auto["waves_eu"] == 0 and auto["U"] <= {1, 2}, auto
    for k, v in rc.flipped_knobs(auto).items():
        clean_env.setenv(k, v)
    dec = product_decoder(rc.codec("n500_q4_i8"), device=-1)
    assert resident_variant(dec.resident_source(1)[0]) == {"flag_reduce": 1 - auto["flag_reduce"], "cn_persistent": 1 - auto["cn_persistent"],
                                                           "xcd": 0, "waves_eu": 2, "U": {4}}
    dec.close()
