"""The owners of the library's HIP resources (jxl_rs_amd/csrc/device_owned.h) through tests/cpp/device_owned.cc: the
program defines counting stand-ins for the HIP calls the header uses, so moves, reset / adopt / ensure, the fences and a
resized vector of slots are checked for exactly-once release and for counters that return to zero.  Host-only, no GPU."""
import subprocess

from test_cpp_host import _build


def test_device_owners(tmp_path):
    exe = _build(tmp_path, "device_owned")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "device owners: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
