"""The host side of the device-made random codewords without a GPU: the sanitizer build of the library on the do-nothing HIP
runtime (tests/fakehip), in a child process started as tests/test_ber_sim_multi_cpu.py starts its own.  Kernels do not run there,
so what is checked is the plumbing -- generator upload, encode_random and sim_batch(zero_codeword = False) at odd batch sizes on
N = 500 and the rank-deficient N = 2048 code, the error paths of the three C-ABI entry points -- under AddressSanitizer + UBSan,
and that no device buffer outlives its handle."""
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent

CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, {root!r})
import numpy as np
import lut_ldpc_amd as L
from lut_ldpc_amd._capi import lib, ERR_ARG, ERR_STATE, last_error

fake = C.CDLL({fake!r})
fake.fakehip_launches_of.argtypes = [C.c_char_p]
for f in ("fakehip_launches_of", "fakehip_live_allocations"):
    getattr(fake, f).restype = C.c_long
codes = {root!r} + "/data/codes/"
for name, B in (("rate0.50_dv02-17_dc08-09_lut_q4_N500", 333), ("rate0.84_reg_v6c32_N2048", 77)):
    pcd = L.Codec(codes + name + ".alist", with_generator=True, device=0)
    pcd.design_luts(sigma2=0.88 ** 2, max_iters=4)
    cw = pcd.encode_random(2 ** 33 + 1, 3, 2 ** 32 + 7, B)
    assert cw.shape == (B, pcd.nvar)
    st = pcd.sim_batch(2.0, 5, 1, 2 ** 32, B, zero_codeword=False)
    assert st.shape == (B, 4) and (st == 0).all()           # (no kernel ran)
    assert pcd.decoder().describe()["generator"] == {{"K": pcd.ninfo, "R": pcd.rank}}
    pcd.close()
assert fake.fakehip_launches_of(b"encode_random_kernel") >= 4 and fake.fakehip_launches_of(b"sent_rows_to_bytes_kernel") >= 2

# error paths
pcd = L.Codec(codes + "rate0.50_dv02-17_dc08-09_lut_q4_N500.alist", with_generator=False, device=0)
pcd.design_luts(sigma2=0.88 ** 2, max_iters=4)
h = C.c_void_p(lib.lutldpc_codec_decoder(pcd._h))
rows = np.zeros(250 * 4, np.uint64)
rp = rows.ctypes.data_as(C.POINTER(C.c_uint64))
assert lib.lutldpc_decoder_set_generator(h, 250, 251, rp) == ERR_ARG                  # K + R != nvar
assert lib.lutldpc_decoder_set_generator(h, 250, 250, None) == ERR_ARG                # rows NULL
stats = np.zeros((5, 4), np.int32)
assert lib.lutldpc_decoder_sim_batch_random(h, None, 1, 0, 0, 5, 250, stats.ctypes.data_as(C.POINTER(C.c_int32)), None, None) == ERR_STATE
assert "generator" in last_error()
assert lib.lutldpc_decoder_encode_random(h, 1, 0, 0, 5, None) == ERR_STATE
try:
    pcd.encode_random(1, 0, 0, 5)
    raise AssertionError("encode_random without a generator")
except L.LutLdpcError as e:
    assert e.code == ERR_STATE
assert lib.lutldpc_decoder_set_generator(h, 250, 250, rp) == 0                        # (valid: replaces nothing, then in use)
assert lib.lutldpc_decoder_encode_random(h, 1, 0, 0, 5, None) == 0
pcd.close()
host = L.Codec(codes + "rate0.50_dv02-17_dc08-09_lut_q4_N500.alist", with_generator=False, device=-1)
host.design_luts(sigma2=0.88 ** 2, max_iters=4)
hh = C.c_void_p(lib.lutldpc_codec_decoder(host._h))
assert lib.lutldpc_decoder_set_generator(hh, 250, 250, rp) == ERR_STATE               # host-only handle
host.close()
live = fake.fakehip_live_allocations()
assert live == 0, live
print("device codewords ok")
"""


def test_device_codewords_host_side_under_asan():
    sys.path.insert(0, str(HERE / "fakehip"))
    import replay
    subprocess.run(["make", "-s", "-j8", "-C", str(HERE / "fakehip")], check=True)
    env = replay.sanitizer_env()
    src = CHILD.format(root=str(ROOT), fake=str(HERE / "fakehip" / "_build" / "libfakehip.so"))
    r = subprocess.run([sys.executable, "-c", src], env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "device codewords ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr
