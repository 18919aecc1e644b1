#!/usr/bin/env python3
"""sim_batch (device sampler + decode + error counts) with zero and with random codewords (LDPC.zero_codeword = false) on the
BASELINE workloads C1, C5 and C2 at bench.py's batch sizes, as-shipped exit conditions (psc AND pisc), 0.4 dB above the design
point.  One JSON line per workload: frames/s of both modes, their ratio, and the device encoder alone (encode_random without the
copy to the host).  Run it against another build of the library with LUTLDPC_LIB=<path>/liblut_ldpc_amd.so (a build without the
device encoder encodes on the host, and reports no encoder time).
Usage: tools/random_codeword_probe.py [--steps K] [workload ...]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np

import bench
import lut_ldpc_amd as L
from lut_ldpc_amd._capi import lib


def lib_name():
    """the library measured, relative to the repository (records stay free of the checkout's location)"""
    p = Path(L._capi.LIB_PATH).resolve()
    return str(p.relative_to(ROOT)) if ROOT in p.parents else p.name


def run(wl, steps):
    alist, sigma, max_iter, qc, qm, B, extra, known_rank = bench.WORKLOADS[wl]
    cd = L.Codec(ROOT / "data" / "codes" / f"{alist}.alist", with_generator=True, known_rank=known_rank, device=0)
    cd.design_luts(sigma2=sigma * sigma, max_iters=max_iter, nq_cha=1 << qc, nq_msg=1 << qm, **extra)
    if wl.startswith("c5"):
        cd.set_initial_message_mode(1)
    cd.set_exit_conditions(max_iter, True, True)
    snr = -10 * np.log10(2 * cd.rate * sigma * sigma) + 0.4
    out = {"workload": wl, "B": B, "nvar": cd.nvar, "K": cd.ninfo, "R": cd.rank, "snr_db": round(float(snr), 3), "lib": lib_name()}
    for zero in (True, False):
        for k in range(2):                                   # warm-up: placement search, graph capture
            cd.sim_batch(snr, 7, 0, k * B, B, zero_codeword=zero)
        t0 = time.perf_counter()
        for k in range(steps):
            st = cd.sim_batch(snr, 7, 0, (2 + k) * B, B, zero_codeword=zero)
        dt = (time.perf_counter() - t0) / steps
        out["zero" if zero else "random"] = {"frames_per_s": round(B / dt), "ms": round(dt * 1e3, 3), "mean_iters": round(float(np.abs(st[:, 0]).mean()), 2),
                                             "fer": round(float(st[:, 1].mean()), 5)}
    out["random_over_zero"] = round(out["random"]["frames_per_s"] / out["zero"]["frames_per_s"], 3)
    if hasattr(lib, "lutldpc_decoder_encode_random"):
        dec = cd.decoder()
        dec.encode_random(7, 0, 0, B, fetch=False)
        t0 = time.perf_counter()
        for k in range(steps):
            dec.encode_random(7, 0, k * B, B, fetch=False)                       # (synchronises)
        dt = (time.perf_counter() - t0) / steps
        valu_s = B * cd.rank * ((cd.ninfo + 31) // 32) / 7.9e13
        out["encoder"] = {"ms_per_call_host_timed": round(dt * 1e3, 4), "bound_ms": round(max(valu_s, B * cd.nvar / 8 / 8e12) * 1e3, 5)}
    print(json.dumps(out), flush=True)
    cd.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("workloads", nargs="*", default=["c1", "c5", "c2"])
    a = ap.parse_args()
    for wl in a.workloads:
        run(wl, a.steps)
