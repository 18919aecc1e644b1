"""Message-label statistics of a finite-length decode, from the histograms counted on the device.

    python -m lut_ldpc_amd.msg_stats -p <params.ini> --snr-index i --frames F [--level 3] [--mode all|active] [--by vn|cn|none] -o out.npz

`Decoder.message_histogram` / `Codec.message_histogram` / `BerSim.message_histogram` return hist[dump, group, x, label] (int64):
how often `label` sat on an edge of `group` at message dump `dump` of output_verbosity = level while the edge's variable node
had sent bit x.  The functions here turn such an array into what density evolution works with: the label pmf given a sent 0
(`fold`), its error probability and its mutual information with the sent bit -- per dump and per group, so that they can be
held against the densities the LUT design assumed, iteration by iteration and degree by degree.

Labels: a label below nq/2 decides bit 1, label l and nq-1-l are mirror images (the quantisers and tables are symmetric,
src/LDPC_Code_LUT.cpp:207-221), so the counts taken under a sent 1 fold onto those of a sent 0 as nq-1-label.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np


def edge_groups(dv, dc, cn_msg_idx, by="vn"):
    """Edge grouping for set_edge_groups: (edge_group int32[E], degrees) -- group g holds the edges whose variable node (by="vn")
    or check node (by="cn") has degree degrees[g]; by="none": one group, degrees = [0].  Edges are numbered VN-major,
    cn_msg_idx lists the edge ids check after check."""
    dv, dc, cn = np.asarray(dv, np.int64), np.asarray(dc, np.int64), np.asarray(cn_msg_idx, np.int64)
    E = int(dv.sum())
    if by == "none":
        return np.zeros(E, np.int32), np.zeros(1, np.int32)
    if by == "vn":
        deg = np.repeat(dv, dv)
    elif by == "cn":
        deg = np.empty(E, np.int64)
        deg[cn] = np.repeat(dc, dc)
    else:
        raise ValueError("by must be 'vn', 'cn' or 'none'")
    degrees, group = np.unique(deg, return_inverse=True)
    if len(degrees) > 256:
        raise ValueError("more than 256 distinct degrees")
    return group.astype(np.int32), degrees.astype(np.int32)


def n_dumps(I, level):
    return 1 + int(I) * (int(level) - 1)


def last_dump(iters, I, level):
    """Number of dumps the reference prints for a frame whose lut_decode returned iters[f]: dump k of the frame is counted in mode
    "active" exactly when k < last_dump[f].  0: none (left through the test on the channel decisions); |c| = I: all; 0 < c < I:
    (level - 1) * c -- the frame returns before the dump of its last variable update (src/LDPC_Code_LUT.cpp:327-337)."""
    c = np.asarray(iters, np.int64)
    out = np.full(c.shape, n_dumps(I, level), np.int64)
    out[c == 0] = 0
    mid = (c > 0) & (c < I)
    out[mid] = (int(level) - 1) * c[mid]
    return out


def dump_alphabets(nq_msg, level):
    """Message alphabet of every dump: the initial messages and a check update of iteration i carry Nq_Msg[i], the variable update
    of iteration i writes Nq_Msg[i+1]; the dump after the last iteration repeats the check update's messages."""
    nq = [int(q) for q in nq_msg]
    I = len(nq)
    out = [nq[0]]
    for i in range(I):
        if int(level) > 2:
            out.append(nq[i])
        out.append(nq[min(i + 1, I - 1)])
    return np.asarray(out, np.int32)


def fold(hist, nq):
    """p(label | 0 sent) over the last two axes [x, label] of hist: the x = 1 counts mirrored as nq-1-label and added to the
    x = 0 counts, normalised.  Returns [..., nq] float64 (all zero where nothing was counted)."""
    h = np.asarray(hist, np.float64)
    nq = int(nq)
    if h.shape[-2] != 2 or h.shape[-1] < nq:
        raise ValueError("hist must end in [2, >= nq]")
    if h[..., nq:].any():
        raise ValueError("counts at labels >= nq")
    f = h[..., 0, :nq] + h[..., 1, :nq][..., ::-1]
    tot = f.sum(-1, keepdims=True)
    return np.divide(f, tot, out=np.zeros_like(f), where=tot > 0)


def error_probability(hist, nq):
    """Probability that a message decides the wrong bit: the folded mass below nq/2."""
    return fold(hist, nq)[..., :int(nq) // 2].sum(-1)


def mutual_information(hist, nq):
    """I(sent bit; label) in bit for equiprobable sent bits and the folded (symmetric) channel p(l | 1) = p(nq-1-l | 0)."""
    p = fold(hist, nq)
    m = p + p[..., ::-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p > 0, p * np.log2(2 * p / m), 0.0)
    return t.sum(-1)


def curves(hist, alphabets):
    """(error probability, mutual information), each [dump, group], with the alphabet of every dump."""
    pe = np.stack([error_probability(hist[k], q) for k, q in enumerate(alphabets)])
    mi = np.stack([mutual_information(hist[k], q) for k, q in enumerate(alphabets)])
    return pe, mi


def main(argv=None):
    ap = argparse.ArgumentParser(prog="msg_stats", description="message-label histograms per iteration of a [LUT] simulation, counted on the MI355X")
    ap.add_argument("-p", "--params", required=True, help="ber_sim parameter file")
    ap.add_argument("-b", "--basedir", default=os.getcwd(), help="paths in the parameter file are relative to this directory")
    ap.add_argument("-s", "--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--snr-index", type=int, default=0, help="index of the SNR point in the parameter file")
    ap.add_argument("--frames", type=int, required=True)
    ap.add_argument("--level", type=int, default=3, choices=(2, 3))
    ap.add_argument("--mode", default="all", choices=("all", "active"))
    ap.add_argument("--by", default="vn", choices=("vn", "cn", "none"), help="edge grouping: variable degree, check degree, none")
    ap.add_argument("-o", "--out", required=True, help="output .npz")
    args = ap.parse_args(argv)
    from .ber_sim import BerSim
    params = args.params if os.path.isabs(args.params) else os.path.join(args.basedir, args.params)
    sim = BerSim(params, args.basedir, args.seed, "", args.device)
    try:
        dv, dc, cn, nq_msg = sim.code()
        group, degrees = edge_groups(dv, dc, cn, args.by)
        dec = sim.decoder()
        dec.set_edge_groups(group, len(degrees))
        hist = dec.new_histogram(args.level)
        f0 = 0
        while f0 < args.frames:
            B = min(sim.batch_frames, args.frames - f0)
            sim.message_histogram(args.snr_index, f0, B, args.level, args.mode, hist=hist)
            f0 += B
        alphabets = dump_alphabets(nq_msg, args.level)
        pe, mi = curves(hist, alphabets)
        np.savez(args.out, hist=hist, alphabets=alphabets, group_degrees=degrees, by=args.by, level=args.level, mode=args.mode, frames=args.frames,
                 snr_db=sim.snr_db[args.snr_index], edges_per_group=np.bincount(group, minlength=len(degrees)), error_probability=pe, mutual_information=mi)
        print(f"{args.frames} frames at {sim.snr_db[args.snr_index]:g} dB: {hist.shape[0]} dumps x {hist.shape[1]} groups -> {args.out}")
        for k in (0, hist.shape[0] - 1):
            print(f"  dump {k}: error probability {np.array2string(pe[k], precision=5)}  mutual information {np.array2string(mi[k], precision=5)}")
    finally:
        sim.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
