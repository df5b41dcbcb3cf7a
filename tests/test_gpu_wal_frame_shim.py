"""The C++ host shim's device-side framing on the GPU
(tests/cpp/wal_frame_selftest.cc): for the same records,
forst_gpu::WalWriteGroup::FrameDevice's image copied back equals Frame()'s
data() byte for byte, and size(), end_block_offset() and physical_records()
are equal -- short, empty and fragmented records, a record that ends at a block
end, a writer in the middle of its block, both header sizes."""
import os
import subprocess
import sys

import pytest

import forst_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _build(tmp_path):
    libdir = os.path.dirname(forst_amd.LIB_PATH)
    exe = str(tmp_path / "wal_frame_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "cpp", "wal_frame_selftest.cc"), "-o", exe,
                           f"-L{libdir}", "-lforst_checksum", "-L/opt/rocm/lib", "-lamdhip64",
                           f"-Wl,-rpath,{libdir}:/opt/rocm/lib", "-lpthread"])
    return exe


@pytest.mark.parametrize("recyclable", [False, True])
def test_shim_frame_device_equals_frame(tmp_path, recyclable):
    import walframe_cases as F
    hs = F.hsize(recyclable)
    exe = _build(tmp_path)
    groups = [(0, [10, 0, 40000, 16, 17, 300, 0, 70001, 1]),
              (5000, [F.BLOCK - 5000 - hs, 0, 9, 100000, 33, 4096]),
              (F.BLOCK, [3, 2 * (F.BLOCK - hs), 0, 1000])]
    for b, lens in groups:
        po, _, _, total, npad, end = F.layout_at(lens, recyclable, b)
        r = subprocess.run([exe, str(int(recyclable)), str(b), "5"] + [str(x) for x in lens],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        assert "case %d %d %d" % (total, len(po), end) in r.stdout.splitlines()
