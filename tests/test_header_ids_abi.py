"""The entry points of fastx_hid.hip and fastx_lines.hip without a GPU: they resolve, and the checks that come before any device call answer
with the documented status (tests/test_gpu_header_ids.py does the rest on the device)."""
import numpy as np

import crass_amd as ca


def test_the_argument_checks_need_no_device():
    lib = ca.load()
    rp = np.asarray([0, 5, 10], np.uint64)
    idx = np.asarray([0, 1], np.uint64)
    out = np.full(2, 7, np.uint64)
    off = np.zeros(3, np.uint64)
    v = ca._abi.Text()
    import ctypes as C
    assert lib.crass_hip_fastx_header_ids_device(None, 16, 10, rp.ctypes.data, 2, out.ctypes.data, 0, None) == 1
    assert lib.crass_hip_fetch_header_lines_device(None, 16, 10, rp.ctypes.data, 2, idx.ctypes.data, 2, C.byref(v), None) == 1
    assert lib.crass_hip_fetch_header_lines_device_to(None, 16, 10, rp.ctypes.data, 2, idx.ctypes.data, 2, None, 0, off.ctypes.data, None) == 1
    assert lib.crass_hip_fetch_header_lines_device_to(None, 16, 10, rp.ctypes.data, 2, idx.ctypes.data, 2, None, 0, None, None) == 1
    assert lib.crass_hip_last_header_ids_ms(None, 0) == 0.0
    assert np.all(out == 7)
