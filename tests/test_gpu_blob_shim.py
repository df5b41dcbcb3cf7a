"""forst_gpu::BlobRecords of the C++ host shim on the GPU
(tests/cpp/blob_shim_selftest.cc): VerifyRecords' Status texts over a
reference-written blob file and a damaged copy, IsValidBlobOffset's edge cases,
FillRecordCrcs regenerating the file, VerifyFiles."""
import os
import subprocess

import pytest

import forst_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blob_shim_on_gpu(tmp_path):
    libdir = os.path.dirname(forst_amd.LIB_PATH)
    exe = str(tmp_path / "blob_shim_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "cpp", "blob_shim_selftest.cc"), "-o", exe,
                           f"-L{libdir}", "-lforst_checksum", "-L/opt/rocm/lib", "-lamdhip64",
                           f"-Wl,-rpath,{libdir}:/opt/rocm/lib", "-lpthread"])
    fixture = os.path.join(ROOT, "tests", "golden", "blob", "db_none.blob")
    r = subprocess.run([exe, fixture], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
