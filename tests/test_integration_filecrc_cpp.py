"""INTEGRATION.md's whole-file checksum call sites compile inside a ForSt
translation unit: the table-writer block that passes the handoff CRC to
WritableFileWriter::Append(Slice, crc) (§2) and the DB::VerifyFileChecksums
block over the staged arena (§3b), type-checked (g++ -fsyntax-only) against
the reference's own headers as tests/test_integration_cpp.py does for the
marked snippets.  The two blocks carry no snippet marker; they are found by
the shim names they use.

Needs the reference headers; skipped elsewhere."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FORST_REFERENCE", "/root/reference")

TEMPLATE = r'''
#include "rocksdb/status.h"
#include "rocksdb/table.h"
#include "table/format.h"
#include "util/crc32c.h"
#include "file/writable_file_writer.h"
#include "forst/forstdb_adapter.h"

namespace ROCKSDB_NAMESPACE {

struct BuilderRep {
  WritableFileWriter* file;
  uint32_t base_context_checksum;
  uint64_t offset;
  uint64_t get_offset() const { return offset; }
};
std::string WriterCrcSnippet(const BlockBasedTableOptions& table_options, BuilderRep* r,
                             void* stream) {
@WRITER@
  return file_checksum + std::to_string(crc);
}

Status VerifyFileChecksumsSnippet(forst_gpu::BlockChecksumEngine& engine, const uint8_t* d_arena,
                                  uint64_t arena_len) {
@VERIFY@
  return crcs.empty() || recorded.empty() ? s : Status::OK();
}

}  // namespace ROCKSDB_NAMESPACE
'''


def block_with(text, needle):
    found = [m.group(1) for m in re.finditer(r"(?<!-->\n)```cpp\n(.*?)```", text, re.S)
             if needle in m.group(1)]
    assert len(found) == 1, (needle, len(found))
    return "\n".join(line for line in found[0].splitlines() if not line.startswith("#include"))


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "rocksdb")),
                    reason="needs the reference headers")
def test_file_checksum_blocks_compile_inside_forst(tmp_path):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    src = TEMPLATE.replace("@WRITER@", block_with(text, "SinkWithCrc"))
    src = src.replace("@VERIFY@", block_with(text, "VerifyFullFileChecksums"))
    f = tmp_path / "filecrc_snippets.cc"
    f.write_text(src)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror=shadow",
                        "-DROCKSDB_PLATFORM_POSIX", "-DOS_LINUX", f"-I{REF}",
                        f"-I{REF}/include", f"-I{os.path.join(ROOT, 'include')}", str(f)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
