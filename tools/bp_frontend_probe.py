#!/usr/bin/env python3
"""[BP] runs of ber_sim with the host and with the device front end (BP.front_end, include/lut_ldpc_bp.h): wall clock and
frames/s of each, and for the device path the kernel times of sampler, counters and decode (rocprofv3 --kernel-trace --stats).

Drives the ber_sim program, every run a fresh child process under a time limit.  A build from before BP.front_end ignores the
key and runs the host front end both times: that run is the baseline.

    tools/bp_frontend_probe.py [--ber-sim PATH] [--out DIR] [--timeout S] [--no-trace]
"""
import argparse
import csv
import re
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

# name -> (alist, SNR dB, Nframes, batch_frames, max_iter).  One SNR point each, all-zero codeword (no generator to construct),
# Nfers out of reach: every run simulates exactly Nframes frames.  DVB-S2: 512 + 2048 + 2048 + 2048 frames, 1.9 MB of rows each.
WORKLOADS = {
    "dvbs2_N64800": ("rate0.50_irreg_dvbs2_N64800", 1.2, 6656, 2048, 30),
    "N500": ("rate0.50_dv02-17_dc08-09_lut_q4_N500", 2.5, 200000, 32768, 30),
}
PARAMS = """[Sim]
   SNRdB    = {snr}
   Nframes  = {nframes}
   Nfers    = 100000000
   batch_frames = {batch}
[LDPC]
   parity_filename = {alist}
   zero_codeword   = true
   parity_check_iter = true
[BP]
   max_iter = {iters}
   qllr_table_size = 300
   qllr_scale_res  = 12
   qllr_spacing_res = 7
   front_end = {front_end}
"""
GROUPS = [("sampler", r"bp_sample_qllr_kernel|bp_zero_kernel"), ("counters", r"bp_count_errors_kernel"),
          ("decode", r"bp_(cn|vn|syndrome|state|start|init)_kernel"), ("host-input load / store", r"bp_(load|store)_kernel")]


def run(cmd, timeout, **kw):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, timeout=timeout, capture_output=True, text=True, **kw)
    return p, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ber-sim", default=str(ROOT / "lut_ldpc_amd" / "lib" / "ber_sim"))
    ap.add_argument("--out", default=None, help="directory for parameter files, results and traces (default: a temporary one)")
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds per child process")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run of the device path")
    a = ap.parse_args()
    out = Path(a.out).resolve() if a.out else Path(tempfile.mkdtemp(prefix="bp_frontend_probe_"))
    (out / "codes").mkdir(parents=True, exist_ok=True)
    print(f"ber_sim: {a.ber_sim}")
    for name, (alist, snr, nframes, batch, iters) in WORKLOADS.items():
        shutil.copy(ROOT / "data" / "codes" / f"{alist}.alist", out / "codes")
        print(f"\n{name}: {alist}, Eb/N0 {snr} dB, {nframes} frames, batches of at most {batch}, max_iter {iters}")
        for fe in ("host", "device"):
            params = out / f"ber.ini.{name}.{fe}"
            params.write_text(PARAMS.format(snr=snr, nframes=nframes, batch=batch, alist=alist, iters=iters, front_end=fe))
            cmd = [a.ber_sim, "-p", str(params), "-b", str(out), "-s", "1", "-c", f"_{name}_{fe}"]
            p, dt = run(cmd, a.timeout)
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("SNR =")), "")
            if p.returncode != 0 or not line:
                print(f"  front_end = {fe}: exit {p.returncode}: {(p.stderr or p.stdout).strip()[-300:]}")
                return 1
            m = re.search(r"Runtime = ([0-9.eE+-]+) seconds", p.stdout)
            loop = float(m.group(1)) if m else float("nan")
            print(f"  front_end = {fe:6s}: process {dt:7.2f} s, frame loop {loop:7.3f} s = {nframes / loop:9.0f} frames/s   | {line.strip()}")
            if fe != "device" or a.no_trace or not shutil.which("rocprofv3"):
                continue
            trace = out / f"trace_{name}"
            shutil.rmtree(trace, ignore_errors=True)
            p, _ = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(trace), "--"] + cmd[:-1] + [f"_{name}_{fe}_prof"], a.timeout * 2)
            stats = sorted(trace.rglob("*kernel_stats.csv"))
            if p.returncode != 0 or not stats:
                print(f"    rocprofv3: exit {p.returncode}, no kernel_stats.csv: {p.stderr.strip()[-200:]}")
                continue
            rows = list(csv.DictReader(open(stats[0])))
            total = sum(float(r["TotalDurationNs"]) for r in rows)
            for label, pat in GROUPS:
                sel = [r for r in rows if re.search(pat, r["Name"])]
                ns = sum(float(r["TotalDurationNs"]) for r in sel)
                print(f"    {label:24s}: {ns / 1e6:9.2f} ms in {sum(int(r['Calls']) for r in sel):6d} launches ({100 * ns / max(total, 1):5.1f} % of the kernel time)")
            for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:8]:
                print(f"      {r['Name'][:70]:70s} {int(r['Calls']):6d} x {float(r['AverageNs']) / 1e3:9.1f} us")
    return 0


if __name__ == "__main__":
    sys.exit(main())
