// tests/golden/ref_filecrc_shim.cc -- TEST INFRASTRUCTURE ONLY: a C veneer
// over the reference's own FileChecksumGenCrc32c (util/file_checksum_helper.h:
// 22-48), linked against the reference archive by tests/golden/refbuild.py for
// tests/golden/gen_filecrc_golden.py.  Nothing is restated here: Update /
// Finalize / GetChecksum are the reference's.
#include <cstring>
#include <string>

#include "util/file_checksum_helper.h"

#define REF_API extern "C" __attribute__((visibility("default")))

// the generator fed data[0, split) then data[split, n); out4 = GetChecksum()
REF_API int ref_file_checksum_crc32c(const char* data, size_t n, size_t split, char* out4) {
  using namespace ROCKSDB_NAMESPACE;
  FileChecksumGenContext ctx;
  FileChecksumGenCrc32cFactory factory;
  std::unique_ptr<FileChecksumGenerator> gen = factory.CreateFileChecksumGenerator(ctx);
  if (!gen || std::strcmp(gen->Name(), "FileChecksumCrc32c") != 0 || split > n) return -1;
  gen->Update(data, split);
  gen->Update(data + split, n - split);
  gen->Finalize();
  const std::string s = gen->GetChecksum();
  if (s.size() != 4) return -2;
  std::memcpy(out4, s.data(), 4);
  return 0;
}
