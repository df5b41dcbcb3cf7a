"""INTEGRATION.md §3's `wal_recover_device` snippet -- the RecoverLogFiles loop
with the record bytes staying on the device (WalRecovery::Recover,
CompactRecords, KvProtection::WriteBatchProtectionDevice, forst_xxh3_64_batch
against record_checksum) -- inside a ForSt translation unit: type-checked
against the reference's own headers, and linked -- with the shim's wal_shim.cc
and engine_shim.cc, the reference's library objects (tests/golden/refbuild.py)
and the product library -- with no undefined symbol allowed (-z defs), the way
tests/test_integration_blob_cpp.py links its blocks.

Needs the reference; skipped elsewhere."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FORST_REFERENCE", "/root/reference")

TEMPLATE = r'''
#include <hip/hip_runtime.h>
#include "rocksdb/options.h"
#include "rocksdb/status.h"
#include "forst_checksum.h"
@INCLUDES@

namespace ROCKSDB_NAMESPACE {

// the surroundings of DBImpl::RecoverLogFiles' read loop
// (db/db_impl/db_impl_open.cc:1195-1260): its reporter, options and log
Status WalRecoverDeviceSnippet(log::Reader::Reporter& reporter,
                               WALRecoveryMode wal_recovery_mode, uint64_t wal_number,
                               void* stream, const uint8_t* d_log, const uint8_t* host_log,
                               uint64_t log_len) {
  Status status;
@WAL_RECOVER_DEVICE@
  return status;
}

}  // namespace ROCKSDB_NAMESPACE
'''

MAIN = r'''
#include <cstdio>
int main(int argc, char**) {
  using namespace ROCKSDB_NAMESPACE;
  void* fns[] = {reinterpret_cast<void*>(&WalRecoverDeviceSnippet)};
  if (argc > 99) std::printf("%p", fns[0]);  // never run: link check only
  return 0;
}
'''


def source():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"<!-- snippet: wal_recover_device[^>]*-->\s*```cpp\n(.*?)```", text, re.S)
    assert m, "INTEGRATION.md has no wal_recover_device snippet"
    lines = m.group(1).splitlines()
    body = "\n".join(ln for ln in lines if not ln.startswith("#include"))
    for call in ("wal.Recover(", "wal.CompactRecords(", "kv.WriteBatchProtectionDevice(",
                 "forst_xxh3_64_batch(", "Write batch content corrupted.", "log record too small",
                 "WriteBatchInternal::kHeader"):
        assert call in body, call
    incs = sorted({ln for ln in lines if ln.startswith("#include")})
    return TEMPLATE.replace("@WAL_RECOVER_DEVICE@", body).replace("@INCLUDES@", "\n".join(incs))


needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "rocksdb")),
                               reason="needs the reference headers")
INC = [f"-I{REF}", f"-I{REF}/include", f"-I{os.path.join(ROOT, 'include')}", "-I/opt/rocm/include",
       "-D__HIP_PLATFORM_AMD__"]


@needs_ref
def test_wal_device_snippet_compiles_inside_forst(tmp_path):
    f = tmp_path / "wal_device_snippet.cc"
    f.write_text(source())
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror=shadow",
                        "-DROCKSDB_PLATFORM_POSIX", "-DOS_LINUX"] + INC + [str(f)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@needs_ref
def test_wal_device_snippet_links_against_reference_objects(tmp_path):
    if os.environ.get("FORST_LINK_CHECK") == "0":
        pytest.skip("FORST_LINK_CHECK=0")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import refbuild
    lib = refbuild.build_archive()  # (cached; built once when it is not)
    src = tmp_path / "wal_device_snippet.cc"
    src.write_text(source() + MAIN)
    csrc = os.path.join(ROOT, "forst_amd", "csrc")
    objs = []
    for f in (str(src), os.path.join(csrc, "wal_shim.cc"), os.path.join(csrc, "engine_shim.cc")):
        o = str(tmp_path / (os.path.basename(f) + ".o"))
        r = subprocess.run(["g++"] + refbuild.CXXFLAGS + INC + ["-c", f, "-o", o],
                           capture_output=True, text=True)
        assert r.returncode == 0, (f, r.stderr[-4000:])
        objs.append(o)
    libdir = os.path.join(ROOT, "forst_amd", "lib")
    exe = str(tmp_path / "wal_device_link")
    r = subprocess.run(["g++"] + refbuild.CXXFLAGS + ["-o", exe] + objs +
                       ["-Wl,--gc-sections", "-Wl,-z,defs", "-Wl,--no-undefined", lib,
                        f"-L{libdir}", "-lforst_checksum", "-L/opt/rocm/lib", "-lamdhip64",
                        "-lz", "-lpthread", "-ldl"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    syms = subprocess.run(["nm", "-C", "--defined-only", exe], capture_output=True,
                          text=True).stdout
    assert "forst_gpu::WalRecovery::CompactRecords" in syms
    assert "forst_gpu::WalRecovery::NextMeta" in syms
    assert "forst_gpu::KvProtection::WriteBatchProtectionDevice" in syms
