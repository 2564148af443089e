"""velo_hip::ScanMap of the header-only C++ wrapper (include/velo_scan_map.hpp) on the GPU: the 6-frame scan-to-map loop with a window
of 3 walked through the wrapper and through the C-ABI calls gives the same poses, loaded clouds, window and stored scans."""
import struct
import subprocess

import numpy as np
import pytest

import velo_amd  # noqa: F401
from velo_amd import synth
from test_scan_map_cpu import compile_driver


@pytest.mark.gpu
def test_wrapper_walks_the_loop_like_the_c_abi(tmp_path):
    exe = compile_driver(tmp_path)
    d = synth.drive(6, n_beams=16, n_azimuth=128)
    case = str(tmp_path / "case.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("iii", 6, 2, 3))
        f.write(np.asarray(d["x_true"][0], np.float64).tobytes())      # the first guess: the motion of the first pair
        for xyz, off in d["frames"]:
            f.write(struct.pack("i", len(off) - 1))
            f.write(np.asarray(off, np.int32).tobytes())
            f.write(np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3]).tobytes())
    out = subprocess.run([exe, case], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == "window 3 scans 3 evicted 3"
    assert out[1] == "batch of one equals load: 1"
    assert out[2] == "drop and clear: 1"
    assert out[3] == "walks ran: 1 1"
    assert out[4] == "poses equal: 1 clouds equal: 1 window equal: 1 stored scan equal: 1 evicted equal: 1"
    t = np.array([float(v) for v in out[5].split()[3:]])
    # the drive moves 0.6 .. 1.4 m per frame along the road (the camera's z): five registrations that follow it
    assert 2.0 < np.linalg.norm(t) < 8.0
