"""Failed frames of a [LUT] simulation, captured on the device: error positions, unsatisfied checks and their profiles.

    python -m lut_ldpc_amd.err_events -p <params.ini> [-b base] [-s seed] --snr-index i --frames F \\
        [--select codeword|info|failed|undetected] [--max-frames n] [--max-pos p] [--max-chk c] -o out.npz

`Decoder.error_events` / `Codec.error_events` / `BerSim.error_events` return an `ErrorEvents`: one record per kept frame
(`events[slot] = {frame, iteration code, cw_errors, data-bit errors, unsat_checks, uncoded errors, positions stored, checks
stored}`), the sorted indices of its wrong nodes and unsatisfied checks (-1 where a list is shorter than its maximum), the number
of frames the rule selected, and -- when asked for -- how often every node was wrong and every check unsatisfied over ALL frames
of the batch.  Only these arrays leave the device; the decided bits stay there.  Frames are Philox-addressed: the command line
writes seed, stream and the global frame index, and `Codec.sample_labels(snr_db, seed, stream, frame, 1)` replays a frame.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import re
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np

SELECT = {"codeword": 0, "info": 1, "failed": 2, "undetected": 3}     # include/lut_ldpc_hip.h: LUTLDPC_EV_*
COLUMNS = ("frame", "code", "cw_errors", "data_bit_errors", "unsat_checks", "uncoded_errors", "positions_stored", "checks_stored")


@dataclass
class ErrorEvents:
    events: np.ndarray                      # int32 [n_stored, 8], see COLUMNS
    positions: np.ndarray                   # int32 [n_stored, max_pos], ascending, -1 = unused
    checks: np.ndarray                      # int32 [n_stored, max_chk]
    n_selected: int                         # frames the rule selected (may exceed n_stored)
    node_errors: Optional[np.ndarray] = None    # int64 [nvar]: frames in which the node was wrong (all frames of the batch)
    check_fails: Optional[np.ndarray] = None    # int64 [nchk]: frames in which the check was unsatisfied

    @property
    def n_stored(self) -> int:
        return len(self.events)


class _Request:
    """A lutldpc_event_request and the arrays it points into."""

    def __init__(self, nvar, nchk, select, max_frames, max_pos, max_chk, profiles):
        from ._capi import EventRequest
        sel = SELECT[select] if isinstance(select, str) else int(select)
        self.events = np.zeros((max(int(max_frames), 0), 8), np.int32)
        self.positions = np.full((max(int(max_frames), 0), max(int(max_pos), 0)), -1, np.int32)
        self.checks = np.full((max(int(max_frames), 0), max(int(max_chk), 0)), -1, np.int32)
        if profiles is None or profiles is False:
            self.node_errors = self.check_fails = None
        elif profiles is True:
            self.node_errors, self.check_fails = np.zeros(nvar, np.int64), np.zeros(nchk, np.int64)
        else:
            self.node_errors, self.check_fails = profiles
            for a, n in ((self.node_errors, nvar), (self.check_fails, nchk)):
                if a.dtype != np.int64 or not a.flags.c_contiguous or a.shape != (n,):
                    raise ValueError("profiles must be (node_errors int64 [nvar], check_fails int64 [nchk]), C-contiguous")
        ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        # (an empty array still has an address: events is never NULL, positions / checks only matter when their maximum is positive)
        self.c = EventRequest(sel, int(max_frames), int(max_pos), int(max_chk), self.events.ctypes.data_as(ip),
                              self.positions.ctypes.data_as(ip), self.checks.ctypes.data_as(ip),
                              self.node_errors.ctypes.data_as(lp) if self.node_errors is not None else None,
                              self.check_fails.ctypes.data_as(lp) if self.check_fails is not None else None, 0, 0)

    def result(self) -> ErrorEvents:
        n = int(self.c.n_stored)
        return ErrorEvents(self.events[:n], self.positions[:n], self.checks[:n], int(self.c.n_selected), self.node_errors, self.check_fails)


# ------------------------------------------------------------------------------------------------
# derived quantities (pure numpy)
# ------------------------------------------------------------------------------------------------


def degree_rates(counts, degrees_of, frames):
    """(degrees, rate): per degree class the share of (node, frame) pairs that were wrong -- counts[v] summed over the nodes of
    the degree, divided by frames x nodes of that degree.  Works for checks alike (counts = check_fails, degrees_of = dc)."""
    counts, deg = np.asarray(counts, np.int64), np.asarray(degrees_of, np.int64)
    if counts.shape != deg.shape:
        raise ValueError("one count per node")
    degrees, cls = np.unique(deg, return_inverse=True)
    tot = np.bincount(cls, weights=counts.astype(np.float64), minlength=len(degrees))
    n = np.bincount(cls, minlength=len(degrees))
    return degrees.astype(np.int32), tot / (n * float(frames)) if frames > 0 else np.zeros(len(degrees))


def weight_histogram(events):
    """hist[w] = kept frames whose residual error pattern has weight w (column cw_errors)."""
    ev = np.asarray(events).reshape(-1, 8)
    return np.bincount(ev[:, 2].astype(np.int64)) if len(ev) else np.zeros(1, np.int64)


def derive(events, node_errors, check_fails, dv, dc, frames):
    """The curves the command line writes next to the raw arrays."""
    vdeg, vrate = degree_rates(node_errors, dv, frames)
    cdeg, crate = degree_rates(check_fails, dc, frames)
    return {"vn_degrees": vdeg, "vn_error_rate": vrate, "cn_degrees": cdeg, "cn_fail_rate": crate, "cw_error_histogram": weight_histogram(events)}


def main(argv=None):
    ap = argparse.ArgumentParser(prog="err_events", description="failed frames of a [LUT] simulation, captured on the MI355X")
    ap.add_argument("-p", "--params", required=True, help="ber_sim parameter file")
    ap.add_argument("-b", "--basedir", default=os.getcwd(), help="paths in the parameter file are relative to this directory")
    ap.add_argument("-s", "--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--snr-index", type=int, default=0, help="index of the SNR point in the parameter file")
    ap.add_argument("--frames", type=int, required=True)
    ap.add_argument("--select", default="codeword", choices=tuple(SELECT))
    ap.add_argument("--max-frames", type=int, default=4096, help="frames kept over the whole run")
    ap.add_argument("--max-pos", type=int, default=64, help="error positions kept per frame")
    ap.add_argument("--max-chk", type=int, default=64, help="unsatisfied checks kept per frame")
    ap.add_argument("-o", "--out", required=True, help="output .npz")
    args = ap.parse_args(argv)
    from .ber_sim import BerSim
    params = args.params if os.path.isabs(args.params) else os.path.join(args.basedir, args.params)
    sim = BerSim(params, args.basedir, args.seed, "", args.device)
    try:
        dv, dc, _, _ = sim.code()
        profiles = (np.zeros(len(dv), np.int64), np.zeros(len(dc), np.int64))
        ev, pos, chk, n_selected, f0 = [], [], [], 0, 0
        while f0 < args.frames:
            B = min(sim.batch_frames, args.frames - f0)
            room = max(args.max_frames - sum(len(e) for e in ev), 0)
            r = sim.error_events(args.snr_index, f0, B, select=args.select, max_frames=room, max_pos=args.max_pos, max_chk=args.max_chk, profiles=profiles)
            e = r.events.astype(np.int64)
            e[:, 0] += f0                                             # global frame index
            ev.append(e); pos.append(r.positions); chk.append(r.checks)
            n_selected += r.n_selected
            f0 += B
        events = np.concatenate(ev)
        # the seed the frames were drawn with: the command line's plus Sim.rand_seed_offset, as in the name of the results file
        m = re.search(r"_rseed(-?\d+)\.it$", sim.results_path())
        seed = int(m.group(1)) if m else args.seed
        d = derive(events, profiles[0], profiles[1], dv, dc, args.frames)
        np.savez(args.out, events=events, positions=np.concatenate(pos), checks=np.concatenate(chk), node_errors=profiles[0], check_fails=profiles[1],
                 n_selected=n_selected, frames=args.frames, select=args.select, seed=seed, stream=args.snr_index,
                 snr_db=sim.snr_db[args.snr_index], columns=np.array(COLUMNS), **d)
        print(f"{args.frames} frames at {sim.snr_db[args.snr_index]:g} dB: {n_selected} selected ({args.select}), {len(events)} kept -> {args.out}")
        print(f"  error rate per variable degree {dict(zip(d['vn_degrees'].tolist(), np.round(d['vn_error_rate'], 6).tolist()))}")
        print(f"  fail rate per check degree {dict(zip(d['cn_degrees'].tolist(), np.round(d['cn_fail_rate'], 6).tolist()))}")
    finally:
        sim.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
