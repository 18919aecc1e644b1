"""Reference histograms for the message-statistics tests: from the oracle's text (every message of every printed dump) and from
the raw trace of a decoder handle, both counted in numpy."""
from __future__ import annotations

import functools

import numpy as np

from helpers import awgn_labels, oracle_codec

# configurations whose level-3 text is the reference (tests/test_msg_stats_cpu.py, tests/test_50_msg_stats_gpu.py) and frames of each
ORACLE_CASES = {"n500_q4_i8": 70, "reg36_n1000_mixed": 70, "reg36_n1000_q3_chklut": 70, "reg36_n1000_m6": 70, "reg36_n1000_q5": 40}
EXITS = ((True, True), (False, False))


def oracle_inputs(name):
    """2.6 dB, seed 3, frame 5 saturated (it passes the test on the channel decisions), as in
    test_output_verbosity_message_dumps_match_the_oracle_text."""
    cd = oracle_codec(name)
    cha, msg, _ = awgn_labels(cd, ORACLE_CASES[name], 2.6, seed=3)
    cha[5] = cd.nq_cha - 1
    msg[5] = cd.nq_msg[0] - 1
    return cd, cha, msg


def parse_dump_text(txt, n_edges):
    """The oracle's text -> list over PRINTED frames of uint8 arrays [dumps of that frame, E].  A frame begins with the headline of
    its initial messages; every data line holds E words '%08X' followed by two blanks."""
    frames, cur = [], None
    for line in txt.split("\n"):
        if not line:
            continue
        if line.startswith("Initial"):
            cur = []
            frames.append(cur)
            continue
        if not ("0" <= line[0] <= "9" or "A" <= line[0] <= "F") or len(line) < 10 * n_edges or line[8] != " ":
            assert "messages" in line, line[:80]
            continue
        b = np.frombuffer(line[:10 * n_edges].encode(), np.uint8).reshape(n_edges, 10)
        assert (b[:, :6] == ord("0")).all() and (b[:, 8:] == ord(" ")).all()
        hexval = lambda c: np.where(c >= ord("A"), c - ord("A") + 10, c - ord("0")).astype(np.uint8)
        cur.append(hexval(b[:, 6]) * 16 + hexval(b[:, 7]))
    return [np.stack(f) for f in frames]


def hist_from_printed(printed, iters, n_dumps, edge_group, n_groups, n_labels, sent_of_edge=None):
    """(hist int64 [n_dumps, n_groups, 2, n_labels], dumps printed per frame int64 [B]) from the parsed text: frames with
    iters == 0 print nothing, the others appear in order.  sent_of_edge: [B, E] sent bit of every edge's variable node, or None."""
    E = len(edge_group)
    hist = np.zeros((n_dumps, n_groups, 2, n_labels), np.int64)
    per_frame = np.zeros(len(iters), np.int64)
    who = np.flatnonzero(np.asarray(iters) != 0)
    assert len(who) == len(printed), (len(who), len(printed))
    for f, dumps in zip(who, printed):
        per_frame[f] = len(dumps)
        x = np.zeros(E, np.int64) if sent_of_edge is None else sent_of_edge[f].astype(np.int64)
        base = (np.asarray(edge_group, np.int64) * 2 + x) * n_labels
        for k, labels in enumerate(dumps):
            hist[k] += np.bincount(base + labels, minlength=n_groups * 2 * n_labels).reshape(n_groups, 2, n_labels)
    return hist, per_frame


def hist_from_oracle_text(txt, iters, n_dumps, edge_group, n_groups, n_labels, sent_of_edge=None):
    """The same straight from the oracle's text (Codec.lut_decode_dump of the oracle)."""
    return hist_from_printed(parse_dump_text(txt, len(edge_group)), iters, n_dumps, edge_group, n_groups, n_labels, sent_of_edge)


def hist_from_trace(trace, last, edge_group, n_groups, n_labels, sent_of_edge=None):
    """Counts a raw trace [n_dumps, B, E] (Decoder.lut_decode_batch_trace, exit tests off) in numpy: frame f counts at dump k
    when k < last[f]."""
    n_dumps, B, E = trace.shape
    hist = np.zeros((n_dumps, n_groups, 2, n_labels), np.int64)
    x = np.zeros((B, E), np.int64) if sent_of_edge is None else sent_of_edge.astype(np.int64)
    grp = np.broadcast_to(np.asarray(edge_group, np.int64), (B, E))
    for k in range(n_dumps):
        on = np.asarray(last) > k
        if on.any():
            flat = (grp[on] * 2 + x[on]) * n_labels + trace[k][on].astype(np.int64)
            hist[k] = np.bincount(flat.ravel(), minlength=n_groups * 2 * n_labels).reshape(n_groups, 2, n_labels)
    return hist


@functools.lru_cache(maxsize=None)
def oracle_printed(name, psc, pisc, level=3):
    """(iters, parsed text) of the oracle for the inputs above -- computed once per session and shared (the text itself, tens of
    megabytes, is dropped)."""
    cd, cha, msg = oracle_inputs(name)
    cd.set_exit_conditions(cd.max_iters, psc, pisc)
    _, it, txt = cd.lut_decode_dump(cha, msg, level)
    return it, parse_dump_text(txt, cd.code.nedges)
