"""The references of tests/bp_cases.py applied to the oracle's [BP] decoder (oracle/or_bp.c), without a GPU: exact sum-product in
float64 for the check pass, int64 numpy for the variable pass with saturation, the numpy statement of to_qllr and of the table, and
the two input rules the header decides (NaN is an erasure, integer input is clipped to +-QMAX).  tests/test_31_bp_limits_gpu.py
holds the device to the same references; here they are checked themselves, and the oracle with them."""
import numpy as np
import pytest

import bp_cases as bc
from oracle import oracle as orc


@pytest.mark.parametrize("d", bc.STAR_SETTINGS, ids=str)
def test_oracle_check_pass_against_exact_boxplus(d):
    """Section 1 (bound derived in bp_cases' docstring): every check-to-variable message of checks of degree 3..40, 64 and 255 lies
    within (n - 2) * eps_op of the exact extrinsic boxplus of the quantised inputs; a degree-2 check returns the other input."""
    ref = orc.BP(orc.Code(graph=bc.star_graph()), *d)
    assert (ref.table() == bc.table(d)).all()
    ref.set_exit_conditions(1, *bc.NO_EXIT)
    _, it, q = ref.decode_llr_batch(bc.star_llr())
    assert (it == -1).all()
    worst = bc.check_star(d, q)
    print(f"star {d}: largest deviation / bound = {worst:.3f}")
    assert worst > 0.05                                       # the bound is no empty one: the table's error is seen


def test_exact_boxplus_is_the_tanh_rule_and_associative():
    """The reference itself: against 2 atanh(tanh(a/2) tanh(b/2)) where that is accurate, and fold-order independence."""
    rng = np.random.default_rng(0)
    a, b, c = rng.normal(0, 3, (3, 4000))
    assert np.allclose(bc.boxplus_exact(a, b), 2 * np.arctanh(np.tanh(a / 2) * np.tanh(b / 2)), rtol=0, atol=1e-12)
    assert np.allclose(bc.boxplus_exact(bc.boxplus_exact(a, b), c), bc.boxplus_exact(a, bc.boxplus_exact(b, c)), rtol=0, atol=1e-12)
    x = rng.normal(0, 4, (50, 9))
    want = np.stack([2 * np.arctanh(np.prod(np.tanh(np.delete(x, i, axis=1) / 2), axis=1)) for i in range(9)], axis=1)
    assert np.allclose(bc.extrinsic_exact(x), want, rtol=0, atol=1e-10)
    big = np.array([700.0, -650.0, 1e6])                      # magnitudes where tanh is 1: the minimum rule remains
    assert np.allclose(bc.extrinsic_exact(big[None])[0], [-650.0, 700.0, -650.0])


@pytest.mark.parametrize("d", bc.PAIR_SETTINGS, ids=str)
def test_oracle_variable_pass_against_int64_numpy(d):
    """Section 2: with degree-2 checks only, three iterations are sums, swaps and clips; variable degrees 1..40, 64 and 255."""
    graph, partner, vn = bc.pair_graph()
    assert graph[0] == 724 and graph[1] == 2449 and len(partner) == 4898
    want, out_share, msg_share = bc.pair_reference(d)
    print(f"pair {d}: clipped outputs {out_share:.3f}, clipped messages {msg_share:.3f}")
    if d in bc.PAIR_SATURATING:
        assert 0.1 < out_share < 0.9 and 0.1 < msg_share < 0.9     # a condition on the inputs: the case cannot pass by never clipping
    else:
        assert out_share == 0 and msg_share == 0
    ref = orc.BP(orc.Code(graph=graph), *d)
    ref.set_exit_conditions(bc.PAIR_ITERS, *bc.NO_EXIT)
    bits, it, q = ref.decode_llr_batch(bc.pair_llr())
    assert (q == want).all() and (bits == (want < 0)).all() and (it == -bc.PAIR_ITERS).all()


@pytest.mark.parametrize("d", bc.LIMIT_REFUSED, ids=str)
def test_creation_refuses_one_step_past_each_limit(d):
    import lut_ldpc_amd as L
    from lut_ldpc_amd._capi import ERR_ARG, LutLdpcError
    code = bc.real_code()
    with pytest.raises(LutLdpcError) as e:
        L.BPDecoder(code.nvar, code.nchk, code.dv, code.dc, code.cn_msg_idx, *d, device=-1)
    assert e.value.code == ERR_ARG


@pytest.mark.parametrize("d", bc.LIMIT_SETTINGS, ids=str)
def test_host_only_handle_builds_the_table_at_each_limit(d):
    """Section 3 on the host: the table of a host-only handle equals numpy's and the oracle's at every accepted limit, and the case
    is no degenerate one (bp_cases.limit_reference asserts it on the oracle)."""
    import lut_ldpc_amd as L
    code = bc.real_code()
    dec = L.BPDecoder(code.nvar, code.nchk, code.dv, code.dc, code.cn_msg_idx, *d, device=-1)
    assert (dec.logexp_table() == bc.table(d)).all() and len(bc.table(d)) == d[1]
    dec.close()
    bc.limit_reference(d)


def test_oracle_high_degree_case_is_not_degenerate():
    """Section 4: with early exit the return values of the high-degree code take more than two distinct values."""
    code = bc.high_degree_code()
    assert all(n % 4 for n in list(bc.HIGH_VDEG.values()) + list(bc.HIGH_CDEG.values()))
    for d in bc.HIGH_SETTINGS:
        ref = orc.BP(code, *d)
        ref.set_exit_conditions(bc.HIGH_ITERS, True, False)
        _, it, _ = ref.decode_llr_batch(bc.high_degree_llr())
        assert len(set(it.tolist())) > 2 and (it > 0).any() and (it < 0).any(), sorted(set(it.tolist()))


@pytest.mark.parametrize("d", [(12, 300, 7, 28), (4, 64, 2, 8)], ids=str)
def test_oracle_special_inputs_nan_is_an_erasure_and_integers_are_clipped(d):
    """Section 6 on the oracle: to_qllr of the special values equals the numpy statement; a NaN decodes like a zero; integer input
    beyond +-QMAX decodes like its clipped value; frames without such values are unaffected."""
    ref = orc.BP(bc.real_code(), *d)
    ref.set_exit_conditions(10, True, True)
    llr, zero_rows = bc.special_llr(d)
    bits, it, q = ref.decode_llr_batch(llr)
    b2, i2, q2 = ref.decode_qllr_batch(bc.to_qllr(llr, d).astype(np.int32))
    assert (q == q2).all() and (it == i2).all() and (bits == b2).all()
    assert (it[zero_rows] == 0).all() and (q[zero_rows] == 0).all()          # all-zero frame: every sign counts as 0, pisc returns 0
    ref.set_exit_conditions(10, True, False)
    assert (ref.decode_llr_batch(llr)[1][zero_rows] == 1).all()              # psc alone: one iteration on zeros, then the same test
    with_nan, with_zero = bc.nan_frames(llr)
    bn, inn, qn = ref.decode_llr_batch(with_nan)
    bz, iz, qz = ref.decode_llr_batch(with_zero)
    assert (qn == qz).all() and (inn == iz).all() and (bn == bz).all()
    qq, rows = bc.out_of_range_qllr(d)
    assert (np.abs(qq.astype(np.int64)) > bc.qmax(d)).any()
    bo, io, qo = ref.decode_qllr_batch(qq)
    bc_, ic, qc = ref.decode_qllr_batch(np.clip(qq, -bc.qmax(d), bc.qmax(d)))
    assert (qo == qc).all() and (io == ic).all() and (bo == bc_).all()
    clean = qq.copy()
    clean[rows] = 0
    others = [r for r in range(len(qq)) if r not in rows]
    assert (ref.decode_qllr_batch(clean)[2][others] == qo[others]).all()
