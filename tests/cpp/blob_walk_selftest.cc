// tests/cpp/blob_walk_selftest.cc -- TEST INFRASTRUCTURE ONLY: a stand-alone
// program around the host walk of forst_blob_verify_files
// (forst_amd/csrc/blob_host.cc), built by tests/test_blob_walk_standalone.py
// with -fsanitize=address,undefined and run directly.
//
//   blob_walk_selftest <corpus>
// corpus = cases of [u64 length][u32 has_cf][u32 cf][bytes].  Each case is
// copied into a heap block of exactly its length (a read past either end is a
// sanitizer report), walked twice (offsets counted, then stored in an array of
// exactly that many slots) and printed as
//   <reason> <n_records> <tail_crosses> <blob_count> <total_blob_bytes> <cf> <offset sum>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "forst_checksum.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t len;
  uint32_t cfw[2];
  unsigned long cases = 0;
  while (std::fread(&len, 8, 1, f) == 1 && std::fread(cfw, 4, 2, f) == 2) {
    uint8_t* data = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    if (len && std::fread(data, 1, len, f) != len) return 3;
    const uint32_t* cf = cfw[0] ? &cfw[1] : nullptr;
    forst_blob_file_result r0, r1;
    uint64_t n0 = 0, n1 = 0;
    int t0 = 0, t1 = 0;
    if (forst_blob_walk_file(len ? data : nullptr, len, cf, nullptr, 0, &n0, &t0, &r0) != FORST_OK)
      return 4;
    std::vector<uint64_t> offs(n0);
    if (forst_blob_walk_file(len ? data : nullptr, len, cf, offs.data(), n0, &n1, &t1, &r1) !=
        FORST_OK)
      return 4;
    if (n0 != n1 || t0 != t1 || std::memcmp(&r0, &r1, sizeof(r0)) != 0) return 5;
    uint64_t sum = 0, prev = 0;
    for (uint64_t k = 0; k < n1; ++k) {
      // every header lies in front of the footer, and the walk moves forward
      if (offs[k] + 32 > len - 32 || (k && offs[k] < prev + 32)) return 6;
      prev = offs[k];
      sum += offs[k] * (k + 1);
    }
    std::printf("%d %llu %d %llu %llu %u %llu\n", r1.reason, static_cast<unsigned long long>(n1), t1,
                static_cast<unsigned long long>(r1.blob_count),
                static_cast<unsigned long long>(r1.total_blob_bytes), r1.column_family_id,
                static_cast<unsigned long long>(sum));
    std::free(data);
    ++cases;
  }
  std::fclose(f);
  std::fprintf(stderr, "%lu cases\n", cases);
  return 0;
}
