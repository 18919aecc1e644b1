#!/usr/bin/env python3
"""What the sparse triangular encoder (lutldpc_decoder_set_sparse_generator, kernels_encode_sparse.hpp) costs, on DVB-S2 N = 64800 at
32768 frames and on an open zigzag (IRA) code of N = 10000 at 4096 frames, in ONE process:
  random     encode_random, codewords kept on the device: information rows from Philox, phase A, phase B
  dev        encode_packed on an int32 tensor in HBM: information rows from the words, phase A, phase B, the full window out
  dev_info   encode_packed, information-only window: the two row <-> word kernels alone
  host       encode_packed on numpy words: upload, the kernels, download
  sim_zero   Codec.sim_batch on the all-zero codeword (sampler, decode, counters): what the parent could run
  sim_rand   Codec.sim_batch with zero_codeword = False: the encoder in front of the same
  copy       yardstick: a device-to-device copy of as many bytes as phase A reads and writes and the row kernels write
Wall time per call from a host clock around calls that end in a stream synchronise, `warmup` rounds, then `rounds` timed ones with
the entries alternating; median, min, max.  Then the kernel time of the encoder entries from the library's profile
(LUTLDPC_K_FRONTEND: all launches of a call together; the split by kernel comes from a kernel trace of this script,
profiles/README.md says how).  dev and host results are compared word for word, and 16 frames of them with the host encoder.
Usage: tools/sparse_encoder_probe.py [--rounds 7] [--warmup 2] [--out profiles/sparse_encoder_probe.txt] [workload ...]   (default: dvbs2 ira10000)"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np

import lut_ldpc_amd as L
from lut_ldpc_amd import packing
from lut_ldpc_amd._capi import lib

SNR = 1.0


def make(wl, tmp):
    """(codec, frames, iterations)"""
    if wl == "dvbs2":
        cd = L.Codec(ROOT / "data" / "codes" / "rate0.50_irreg_dvbs2_N64800.alist", with_generator=True, known_rank=32400, device=0)
        cd.design_luts(sigma2=0.88 ** 2, max_iters=50, allow_degree_one=True)
        return cd, 32768, 50
    import sparse_encode_cases as sc
    path = Path(tmp) / "ira10000.alist"
    sc.write_open_zigzag_alist(path, [(5000, 3)], 3, seed=14)
    cd = L.Codec(path, with_generator="sparse", device=0)
    cd.design_luts(sigma2=0.88 ** 2, max_iters=30, allow_degree_one=True)
    return cd, 4096, 30


def run(wl, rounds, warmup, say, tmp):
    import torch
    cd, B, iters = make(wl, tmp)
    cd.set_exit_conditions(iters, True, False)
    dec = cd.decoder()
    N, K, R = cd.nvar, cd.ninfo, cd.rank
    gen = dec.describe()["generator"]
    assert gen["form"] == "sparse", gen
    T = dec.describe()["tile_frames"]
    G = -(-B // T)
    W = (K + 31) // 32
    words = np.random.default_rng(59).integers(0, 1 << 32, (B, W), dtype=np.uint32)
    d_words = torch.from_numpy(words.view(np.int32)).to("cuda")
    a_terms = gen["terms"] - (R - 1)                        # both codes are open zigzags: R - 1 parity-on-parity terms, the rest are phase A's
    row_bytes = T // 8
    moved = G * row_bytes * (a_terms + R + K)               # phase A reads a_terms rows and writes R, the information kernel writes K
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    res = {}

    def copy():
        dst.copy_(src)
        torch.cuda.synchronize()

    entries = {"random": lambda: dec.encode_random(59, 1, 0, B, fetch=False),
               "dev": lambda: res.__setitem__("dev", dec.encode_packed(d_words)),
               "dev_info": lambda: dec.encode_packed(d_words, 0, K),
               "host": lambda: res.__setitem__("host", dec.encode_packed(words)),
               "sim_zero": lambda: res.__setitem__("sim_zero", cd.sim_batch(SNR, 59, 1, 0, B, zero_codeword=True)),
               "sim_rand": lambda: res.__setitem__("sim_rand", cd.sim_batch(SNR, 59, 1, 0, B, zero_codeword=False)),
               "copy": copy}
    wall = {k: [] for k in entries}
    for r in range(warmup + rounds):
        for k, call in entries.items():
            t0 = time.perf_counter()
            call()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                wall[k].append(dt)
    same = bool((res["dev"].cpu().numpy().view(np.uint32) == res["host"]).all())
    cw = packing.unpack_bits(res["host"][:16], N)
    host_enc = bool(all((cd.encode(cw[i, :K]) == cw[i]).all() for i in range(len(cw))))
    kern = {k: [] for k in ("random", "dev", "dev_info")}
    dec.set_profiling(True)
    for r in range(warmup + rounds):
        for k in kern:
            dec.reset_profile()
            entries[k]()
            if r >= warmup:
                kern[k].append(dec.profile()["frontend"]["ms"])
    dec.set_profiling(False)
    out = {"workload": wl, "B": B, "nvar": N, "K": K, "R": R, "generator": gen, "rounds": rounds, "warmup": warmup, "dev_equals_host": same,
           "host_encoder_equal_16_frames": host_enc, "bytes_moved_by_phase_a_and_information_rows": moved}
    say(f"{wl}: {B} frames, N = {N}, K = {K}, R = {R}, generator {json.dumps(gen)}; dev == host: {same}; host encoder equal on 16 frames: {host_enc}")
    say(f"  {'entry':9s} {'wall median ms':>15s} {'min':>9s} {'max':>9s} {'kernel median ms':>17s} {'min':>9s} {'max':>9s}")
    for k in entries:
        wm = float(np.median(wall[k]))
        out[k] = {"wall_ms_median": round(wm, 3), "wall_ms_min": round(min(wall[k]), 3), "wall_ms_max": round(max(wall[k]), 3)}
        tail = ""
        if k in kern:
            km = float(np.median(kern[k]))
            out[k].update(kernel_ms_median=round(km, 4), kernel_ms_min=round(min(kern[k]), 4), kernel_ms_max=round(max(kern[k]), 4))
            tail = f" {km:17.4f} {min(kern[k]):9.4f} {max(kern[k]):9.4f}"
        say(f"  {k:9s} {wm:15.3f} {min(wall[k]):9.3f} {max(wall[k]):9.3f}{tail}")
    out["copy_GBps"] = round(moved / 1e6 / out["copy"]["wall_ms_median"], 1)
    out["rate_rand_over_zero"] = round(out["sim_zero"]["wall_ms_median"] / out["sim_rand"]["wall_ms_median"], 3)
    out["encoder_kernels_over_sim_zero"] = round(out["random"]["kernel_ms_median"] / out["sim_zero"]["wall_ms_median"], 4)
    say(f"  copy of {moved / 1e6:.0f} MB (read + written): {out['copy_GBps']} GB/s;  frames/s with random codewords over frames/s on the all-zero codeword: "
        f"{out['rate_rand_over_zero']} (the dense encoder reached 0.84 - 0.99 on its codes);  encoder kernels / sim_zero: {out['encoder_kernels_over_sim_zero']}")
    say(json.dumps(out))
    cd.close()
    return same and host_enc


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sparse_encoder_probe.txt"))
    ap.add_argument("workloads", nargs="*", default=["dvbs2", "ira10000"])
    a = ap.parse_args()
    if L.device_count() < 1:
        sys.exit("sparse_encoder_probe needs an MI355X: no HIP device visible")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f, tempfile.TemporaryDirectory() as tmp:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"tools/sparse_encoder_probe.py --rounds {a.rounds} --warmup {a.warmup} {' '.join(a.workloads)}   ({lib.lutldpc_version().decode()})")
        ok = all([run(wl, a.rounds, a.warmup, say, tmp) for wl in a.workloads])
    sys.exit(0 if ok else 1)
