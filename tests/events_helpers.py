"""Expected arrays of the failed-frame capture, in a few lines of numpy: from decided bits, sent bits, iteration codes and the
graph -- no package code.  The decided bits come from the oracle, fed the same labels as the device."""
from __future__ import annotations

import numpy as np

SELECTS = ("codeword", "info", "failed", "undetected")


def syndrome(bits, dv, dc, cn_msg_idx):
    """[B, nchk] 0/1: parity of every check over the decided bits.  Edges are numbered VN-major; cn_msg_idx lists the edge ids
    check after check."""
    dv, dc, cn = np.asarray(dv, np.int64), np.asarray(dc, np.int64), np.asarray(cn_msg_idx, np.int64)
    node_of_check_edge = np.repeat(np.arange(len(dv)), dv)[cn]
    ptr = np.concatenate([[0], np.cumsum(dc)])
    run = np.concatenate([np.zeros((len(bits), 1), np.int64), np.cumsum(np.asarray(bits, np.int64)[:, node_of_check_edge], axis=1)], axis=1)
    return ((run[:, ptr[1:]] - run[:, ptr[:-1]]) & 1).astype(np.uint8)


def expected(bits, sent, iters, graph, k_info, select, max_frames, max_pos, max_chk, uncoded=None):
    """(events int32 [n, 8], positions [n, max_pos], checks [n, max_chk], n_selected, node_errors int64 [nvar], check_fails int64
    [nchk]) as the capture defines them; graph = (dv, dc, cn_msg_idx); sent None = all-zero codeword."""
    bits = np.asarray(bits, np.uint8)
    err = bits != (0 if sent is None else np.asarray(sent, np.uint8))
    syn = syndrome(bits, *graph)
    it = np.asarray(iters, np.int64)
    cw, info, unsat = err.sum(1), err[:, :k_info].sum(1), syn.sum(1)
    sel = {"codeword": cw > 0, "info": info > 0, "failed": it < 0, "undetected": (cw > 0) & (it >= 0)}[select]
    chosen = np.flatnonzero(sel)
    kept = chosen[:max_frames]
    unc = np.zeros(len(bits), np.int64) if uncoded is None else np.asarray(uncoded, np.int64)
    events = np.stack([kept, it[kept], cw[kept], info[kept], unsat[kept], unc[kept], np.minimum(cw[kept], max_pos), np.minimum(unsat[kept], max_chk)],
                      axis=1).astype(np.int32).reshape(-1, 8)
    positions = np.full((len(kept), max_pos), -1, np.int32)
    checks = np.full((len(kept), max_chk), -1, np.int32)
    for s, f in enumerate(kept):
        p, c = np.flatnonzero(err[f])[:max_pos], np.flatnonzero(syn[f])[:max_chk]
        positions[s, :len(p)] = p
        checks[s, :len(c)] = c
    return events, positions, checks, len(chosen), err.sum(0).astype(np.int64), syn.sum(0).astype(np.int64)


def assert_equal(got, want, what=""):
    """got: an ErrorEvents; want: the tuple of expected().  Exact equality of every integer array."""
    ev, pos, chk, n_sel, node, check = want
    assert got.n_selected == n_sel, (what, got.n_selected, n_sel)
    assert got.events.dtype == np.int32 and got.events.shape == ev.shape, (what, got.events.shape, ev.shape)
    assert (got.events == ev).all(), (what, np.argwhere(got.events != ev)[:4].tolist())
    assert got.positions.shape == pos.shape and (got.positions == pos).all(), (what, np.argwhere(got.positions != pos)[:4].tolist())
    assert got.checks.shape == chk.shape and (got.checks == chk).all(), (what, np.argwhere(got.checks != chk)[:4].tolist())
    if got.node_errors is not None:
        assert (got.node_errors == node).all() and (got.check_fails == check).all(), what
