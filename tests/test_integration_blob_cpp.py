"""INTEGRATION.md §3d's blob call sites inside a ForSt translation unit: the
MultiGetBlob verify loop, BlobLogWriter::EmitPhysicalRecord with deferred CRCs
and the file scan are found by their headings (they carry no snippet marker),
type-checked against the reference's own headers, and linked -- with the
shim's engine_shim.cc, the reference's library objects
(tests/golden/refbuild.py) and the product library -- with no undefined symbol
allowed (-z defs), the way tests/test_integration_cpp.py links the marked
snippets.

Needs the reference; skipped elsewhere."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FORST_REFERENCE", "/root/reference")

HEADINGS = {"@MULTIGET@": "#### MultiGetBlob's verify loop",
            "@WRITER@": "#### BlobLogWriter::EmitPhysicalRecord with deferred CRCs",
            "@SCAN@": "#### A file scan"}

TEMPLATE = r'''
#include <hip/hip_runtime.h>
#include "db/blob/blob_contents.h"
#include "db/blob/blob_log_format.h"
#include "file/writable_file_writer.h"
#include "rocksdb/status.h"
#include "util/autovector.h"
@INCLUDES@

namespace ROCKSDB_NAMESPACE {

Status MultiGetBlobSnippet(
    autovector<std::pair<BlobReadRequest*, std::unique_ptr<BlobContents>>>& blob_reqs,
    const uint8_t* d_file, uint64_t file_size_, void* stream) {
  Status s;
@MULTIGET@
  return s;
}

Status BlobWriterSnippet(WritableFileWriter* dest_, const std::vector<Slice>& keys,
                         const std::vector<Slice>& values,
                         const std::vector<uint64_t>& expirations, uint8_t* d_window,
                         void* stream) {
  Status s;
@WRITER@
  return s;
}

struct StagedBlobFile {
  const uint8_t* host_bytes;
  uint64_t size;
  uint64_t arena_offset;
};
Status BlobScanSnippet(const std::vector<StagedBlobFile>& files, uint32_t column_family_id,
                       const uint8_t* d_arena, uint64_t arena_len, void* stream) {
  Status s;
@SCAN@
  return s;
}

}  // namespace ROCKSDB_NAMESPACE
'''

MAIN = r'''
#include <cstdio>
int main(int argc, char**) {
  using namespace ROCKSDB_NAMESPACE;
  void* fns[] = {reinterpret_cast<void*>(&MultiGetBlobSnippet),
                 reinterpret_cast<void*>(&BlobWriterSnippet),
                 reinterpret_cast<void*>(&BlobScanSnippet)};
  if (argc > 99) std::printf("%p", fns[argc % 3]);  // never run: link check only
  return 0;
}
'''


def source():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    src, incs = TEMPLATE, []
    for mark, heading in HEADINGS.items():
        at = text.index(heading)
        m = re.compile(r"```cpp\n(.*?)```", re.S).search(text, at)
        # the block belongs to this heading, and is not a marked snippet
        assert m and "\n#### " not in text[at + 1:m.start()] and "\n## " not in text[at:m.start()]
        assert "<!-- snippet" not in text[at:m.start()]
        lines = m.group(1).splitlines()
        incs += [ln for ln in lines if ln.startswith("#include")]
        src = src.replace(mark, "\n".join(ln for ln in lines if not ln.startswith("#include")))
    return src.replace("@INCLUDES@", "\n".join(sorted(set(incs))))


needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "rocksdb")),
                               reason="needs the reference headers")
INC = [f"-I{REF}", f"-I{REF}/include", f"-I{os.path.join(ROOT, 'include')}", "-I/opt/rocm/include",
       "-D__HIP_PLATFORM_AMD__"]


@needs_ref
def test_blob_blocks_compile_inside_forst(tmp_path):
    f = tmp_path / "blob_snippets.cc"
    f.write_text(source())
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror=shadow",
                        "-DROCKSDB_PLATFORM_POSIX", "-DOS_LINUX"] + INC + [str(f)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@needs_ref
def test_blob_blocks_link_against_reference_objects(tmp_path):
    if os.environ.get("FORST_LINK_CHECK") == "0":
        pytest.skip("FORST_LINK_CHECK=0")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import refbuild
    lib = refbuild.build_archive()  # (cached; built once when it is not)
    src = tmp_path / "blob_snippets.cc"
    src.write_text(source() + MAIN)
    objs = []
    for f in (str(src), os.path.join(ROOT, "forst_amd", "csrc", "engine_shim.cc")):
        o = str(tmp_path / (os.path.basename(f) + ".o"))
        r = subprocess.run(["g++"] + refbuild.CXXFLAGS + INC + ["-c", f, "-o", o],
                           capture_output=True, text=True)
        assert r.returncode == 0, (f, r.stderr[-4000:])
        objs.append(o)
    libdir = os.path.join(ROOT, "forst_amd", "lib")
    exe = str(tmp_path / "blob_link")
    r = subprocess.run(["g++"] + refbuild.CXXFLAGS + ["-o", exe] + objs +
                       ["-Wl,--gc-sections", "-Wl,-z,defs", "-Wl,--no-undefined", lib,
                        f"-L{libdir}", "-lforst_checksum", "-L/opt/rocm/lib", "-lamdhip64",
                        "-lz", "-lpthread", "-ldl"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    syms = subprocess.run(["nm", "-C", "--defined-only", exe], capture_output=True,
                          text=True).stdout
    assert "forst_gpu::BlobRecords::VerifyRecords" in syms
    assert "forst_gpu::BlobRecords::FillRecordCrcs" in syms
    assert "forst_gpu::BlobRecords::VerifyFiles" in syms
    assert "WritableFileWriter::Append" in syms
