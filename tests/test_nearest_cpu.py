"""CPU: the nearest-sigma entry points refuse null arguments without a GPU, and their kernel compiles for gfx950 without scratch."""
import os
import re
import shutil
import subprocess

import pytest

from ibs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")


def test_null_context_and_arguments_are_refused():
    lib = _lib.lib()
    N = 513
    assert lib.ibs_solve_gcf_nearest_f64(None, 1, N, 0.05, None, None, None, None, N, None, None, None, None, None, None, None, 0) < 0
    assert b"null" in lib.ibs_last_error()
    assert lib.ibs_gamma_scan_nearest_f64(None, 1, 1, N, 0.05, *([None] * 7), N, None, None, None, None, None, None, None, 0) < 0
    assert b"null" in lib.ibs_last_error()
    if lib.ibs_device_count() > 0:          # (a context needs a GPU; the argument checks come before any device work)
        import ctypes as C
        h = C.c_void_p(None)
        assert lib.ibs_create(C.byref(h), 0) == 0
        try:
            assert lib.ibs_solve_gcf_nearest_f64(h, 1, N, 0.05, None, None, None, None, N, None, None, None, None, None, None, None, 0) < 0
            assert lib.ibs_gamma_scan_nearest_f64(h, 1, 1, N, 0.05, *([None] * 7), N, None, None, None, None, None, None, None, 0) < 0
        finally:
            lib.ibs_destroy(h)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_nearest_kernel_has_no_scratch():
    """k_solve_gcf_nearest<HAS_GH> (csrc/ibs_nearest.hip): both instantiations compile for gfx950 with ScratchSize 0"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "ibs_nearest.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    name, scratch = None, {}
    for line in r.stderr.split("\n"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    kern = {k: v for k, v in scratch.items() if "k_solve_gcf_nearest" in k}
    assert len(kern) == 2 and all(v == 0 for v in kern.values()), scratch
