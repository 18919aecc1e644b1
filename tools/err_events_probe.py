#!/usr/bin/env python3
"""What the capture of failed frames costs (lut_ldpc_amd/csrc/hip/kernels_events.hpp) on the flagship workload: DVB-S2 N=64800,
50 iterations, 32768 frames per step, device sampler, select = codeword.

Three variants, each in child processes of its own that alternate on the same box (a process loads ONE build of the library):
  parent   Codec.sim_batch of a build WITHOUT the capture  (--parent-lib <path>/liblut_ldpc_amd.so; skipped when not given)
  plain    Codec.sim_batch of this build
  events   Codec.error_events of this build: the same frames, the same decode, the capture on top
Every child warms every shape up (buffers, code objects, the graph of the decode), then times `--reps` calls of the same frames
with a host clock around the synchronising call.  One JSON line per child, then the medians, the ratio events / parent (bar: 1.03)
and the bytes a batch copies to the host next to what bits_out would move.  The text also goes to profiles/err_events_probe.txt.

Usage: tools/err_events_probe.py [--parent-lib PATH] [--rounds 2] [--reps 5] [--batch 32768] [--mode fixed|shipped]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def worker(variant, reps, B, mode):
    import numpy as np
    import lut_ldpc_amd as L
    sigma, I = 0.88, 50
    cd = L.Codec(ROOT / "data" / "codes" / "rate0.50_irreg_dvbs2_N64800.alist", known_rank=32400, device=0)
    cd.design_luts(sigma2=sigma * sigma, max_iters=I, nq_cha=16, nq_msg=16, allow_degree_one=True)
    psc = mode == "shipped"
    cd.set_exit_conditions(I, psc, psc)
    snr = -10 * np.log10(2 * cd.rate * sigma * sigma) + (0.4 if psc else 0.0)
    out = {"variant": variant, "mode": mode, "B": B, "snr_db": round(float(snr), 4), "lib": str(Path(L._capi.LIB_PATH).resolve().parent.parent.name)}
    if variant == "events":
        prof = (np.zeros(cd.nvar, np.int64), np.zeros(cd.nchk, np.int64))

        def call(k):
            return cd.error_events(snr, 99, 0, k * B, B, select="codeword", max_frames=1024, max_pos=64, max_chk=64, profiles=prof)
    else:
        def call(k):
            return cd.sim_batch(snr, 99, 0, k * B, B)
    for k in range(3):                                                # plain launches, graph capture, first replay
        r = call(k)
    ts = []
    for k in range(reps):
        t0 = time.perf_counter(); r = call(k); ts.append(time.perf_counter() - t0)
    out["ms"] = [round(t * 1e3, 3) for t in ts]
    if variant == "events":
        to_host = r.events.nbytes + r.positions.nbytes + r.checks.nbytes + prof[0].nbytes + prof[1].nbytes + 8 + B * 16     # (+ counters, frame_stats)
        out.update({"n_selected": r.n_selected, "n_stored": r.n_stored, "bytes_to_host": int(to_host), "bits_out_bytes": B * cd.nvar,
                    "largest_weight_kept": int(r.events[:, 2].max()) if r.n_stored else 0})
    else:
        out["frame_errors"] = int((r[:, 1] != 0).sum())
    print(json.dumps(out), flush=True)
    cd.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--mode", default="fixed", choices=("fixed", "shipped"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "err_events_probe.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.reps, args.batch, args.mode)
    variants = (["parent"] if args.parent_lib else []) + ["plain", "events"]
    lines, ms = [], {v: [] for v in variants}
    last = {}
    for _ in range(args.rounds):
        for v in variants:
            env = dict(os.environ)
            if v == "parent":
                env["LUTLDPC_LIB"] = str(Path(args.parent_lib).resolve())
            else:
                env.pop("LUTLDPC_LIB", None)
            r = subprocess.run([sys.executable, __file__, "--worker", "plain" if v == "parent" else v, "--reps", str(args.reps), "--batch", str(args.batch),
                                "--mode", args.mode], env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                print(r.stdout + r.stderr[-2000:], flush=True)
                raise SystemExit(f"worker {v} failed with {r.returncode}")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            rec["variant"] = v
            ms[v] += rec["ms"]
            last[v] = rec
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    med = {v: statistics.median(ms[v]) for v in variants}
    base = "parent" if args.parent_lib else "plain"
    summary = {"median_ms": {v: round(med[v], 3) for v in variants}, "min_ms": {v: round(min(ms[v]), 3) for v in variants},
               "max_ms": {v: round(max(ms[v]), 3) for v in variants}, "baseline": base, "events_over_baseline": round(med["events"] / med[base], 4), "bar": 1.03,
               "bytes_to_host_per_batch": last["events"]["bytes_to_host"], "bits_out_bytes_per_batch": last["events"]["bits_out_bytes"]}
    lines.append(json.dumps(summary))
    print(lines[-1], flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
