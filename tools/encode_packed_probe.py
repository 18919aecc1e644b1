#!/usr/bin/env python3
"""What it costs to encode the caller's data on the device (lutldpc_decoder_encode_packed), next to the yardstick that has not
changed: lutldpc_decoder_encode_random(codewords = NULL) on the same handle and batch -- the same R * ceil(K/32) word operations per
frame, Philox in place of loads, sent-bit rows in place of words.
Per workload (the (3,6) N = 10000 code and the (6,32) N = 2048 code at the batch sizes of bench.py), in ONE process:
  host     encode_packed on numpy words: upload, kernel, download of the codeword words
  dev      encode_packed on an int32 tensor in HBM, the codeword words left there
  random   encode_random, codewords kept on the device
Wall time per call from a host clock around calls that end in a stream synchronise, buffers made and touched before the first call,
`warmup` rounds, then `rounds` timed ones with the entries alternating; median, min, max.  Then the kernels alone from the library's
profile (LUTLDPC_K_FRONTEND: one launch per call for both), in rounds of their own with profiling on.  host and dev results are
compared word for word, and 64 frames of them with the host encoder.  One JSON line per workload after the table.
Usage: tools/encode_packed_probe.py [--rounds 7] [--warmup 2] [--frames B] [--out profiles/encode_packed_probe.txt] [workload ...]
(default: c2 c5)"""
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
from lut_ldpc_amd import packing
from lut_ldpc_amd._capi import lib


def run(wl, rounds, warmup, frames, say):
    import torch
    alist, sigma, max_iter, qc, qm, B, extra, known_rank = bench.WORKLOADS[wl]
    B = frames or B
    cd = L.Codec(ROOT / "data" / "codes" / f"{alist}.alist", with_generator=True, known_rank=known_rank, device=0)
    cd.design_luts(sigma2=sigma * sigma, max_iters=max_iter, nq_cha=1 << qc, nq_msg=1 << qm, **extra)
    dec = cd.decoder()
    N, K, R = cd.nvar, cd.ninfo, cd.rank
    assert dec.describe()["generator"] == {"K": K, "R": R}
    W, Wout = (K + 31) // 32, (N + 31) // 32
    words = np.random.default_rng(58).integers(0, 1 << 32, (B, W), dtype=np.uint32)
    d_words = torch.from_numpy(words.view(np.int32)).to("cuda")
    torch.cuda.synchronize()
    res = {}

    def random():
        dec.encode_random(58, 1, 0, B, fetch=False)

    entries = {"host": lambda: res.__setitem__("host", dec.encode_packed(words)),
               "dev": lambda: res.__setitem__("dev", dec.encode_packed(d_words)),
               "random": random}
    wall = {k: [] for k in entries}
    for r in range(warmup + rounds):
        for k, call in entries.items():
            t0 = time.perf_counter()
            call()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                wall[k].append(dt)
    same = bool((res["dev"].cpu().numpy().view(np.uint32) == res["host"]).all())
    cw = packing.unpack_bits(res["host"][:64], N)
    host_enc = bool(all((cd.encode(cw[i, :K]) == cw[i]).all() for i in range(len(cw))))
    kern = {k: [] for k in entries}
    dec.set_profiling(True)
    for r in range(warmup + rounds):
        for k, call in entries.items():
            dec.reset_profile()
            call()
            p = dec.profile()["frontend"]
            assert p["launches"] == 1, (k, p)
            if r >= warmup:
                kern[k].append(p["ms"])
    dec.set_profiling(False)
    ops = R * W                                                     # word operations (acc ^= a & u) per frame, both kernels
    out = {"workload": wl, "B": B, "nvar": N, "K": K, "R": R, "rounds": rounds, "warmup": warmup, "dev_equals_host": same, "host_encoder_equal_64_frames": host_enc,
           "word_ops_per_frame": ops, "bytes_in": 4 * B * W, "bytes_out": 4 * B * Wout}
    say(f"{wl}: {B} frames, N = {N}, K = {K}, R = {R}; {ops} word operations per frame; {4 * B * W / 1e6:.1f} MB in, {4 * B * Wout / 1e6:.1f} MB out; "
        f"dev == host: {same}; host encoder equal on 64 frames: {host_enc}")
    say(f"  {'entry':8s} {'wall median ms':>15s} {'min':>8s} {'max':>8s} {'kernel median ms':>17s} {'min':>8s} {'max':>8s} {'Gops/s (kernel)':>16s}")
    for k in entries:
        wm, km = float(np.median(wall[k])), float(np.median(kern[k]))
        out[k] = {"wall_ms_median": round(wm, 3), "wall_ms_min": round(min(wall[k]), 3), "wall_ms_max": round(max(wall[k]), 3),
                  "kernel_ms_median": round(km, 4), "kernel_ms_min": round(min(kern[k]), 4), "kernel_ms_max": round(max(kern[k]), 4)}
        say(f"  {k:8s} {wm:15.3f} {min(wall[k]):8.3f} {max(wall[k]):8.3f} {km:17.4f} {min(kern[k]):8.4f} {max(kern[k]):8.4f} {B * ops / km / 1e6:16.1f}")
    out["kernel_dev_over_random"] = round(out["dev"]["kernel_ms_median"] / out["random"]["kernel_ms_median"], 3)
    out["kernel_host_over_random"] = round(out["host"]["kernel_ms_median"] / out["random"]["kernel_ms_median"], 3)
    say(f"  encode_bits_kernel / encode_random_kernel (kernel time, medians): dev {out['kernel_dev_over_random']}, host {out['kernel_host_over_random']}")
    say(json.dumps(out))
    cd.close()
    return same and host_enc


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "encode_packed_probe.txt"))
    ap.add_argument("workloads", nargs="*", default=["c2", "c5"])
    a = ap.parse_args()
    if L.device_count() < 1:
        sys.exit("encode_packed_probe needs an MI355X: no HIP device visible")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"tools/encode_packed_probe.py --rounds {a.rounds} --warmup {a.warmup} {' '.join(a.workloads)}   ({lib.lutldpc_version().decode()})")
        ok = all([run(wl, a.rounds, a.warmup, a.frames, say) for wl in a.workloads])
    sys.exit(0 if ok else 1)
