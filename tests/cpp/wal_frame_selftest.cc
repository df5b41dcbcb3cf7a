// tests/cpp/wal_frame_selftest.cc -- TEST INFRASTRUCTURE ONLY.
// forst_gpu::WalWriteGroup::FrameDevice against Frame() for the same records:
// the device image copied back equals data() byte for byte, and size(),
// end_block_offset() and physical_records() are equal -- with the caller's
// host copy of the sizes and without it.
//   wal_frame_selftest <recyclable: 0 | 1> <block offset> <seed> <length>...
// The records' bytes are a generator's; they are staged back to back (every
// source alignment) in one device buffer.
// Prints "case <image bytes> <physical records> <end block offset>", then PASS.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "forst/checksum_engine.h"

using namespace forst_gpu;

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);      \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const bool recyclable = std::atoi(argv[1]) != 0;
  const uint32_t block_offset = static_cast<uint32_t>(std::atoi(argv[2]));
  uint64_t x = std::strtoull(argv[3], nullptr, 10) * 2 + 1;
  std::vector<uint32_t> sizes;
  std::vector<uint64_t> offs;
  std::string base;
  for (int i = 4; i < argc; ++i) {
    const uint32_t n = static_cast<uint32_t>(std::strtoul(argv[i], nullptr, 10));
    offs.push_back(base.size());
    sizes.push_back(n);
    for (uint32_t k = 0; k < n; ++k) {
      x = x * 6364136223846793005ull + 1442695040888963407ull;
      base.push_back(static_cast<char>(x >> 56));
    }
  }
  const uint64_t n = sizes.size();
  std::vector<ByteRange> records;
  for (uint64_t i = 0; i < n; ++i) records.push_back({base.data() + offs[i], sizes[i]});
  WalWriteGroup host(recyclable, 7), dev(recyclable, 7);
  CHECK(host.Frame(records, block_offset).ok());

  uint8_t* d_base = nullptr;
  uint64_t* d_offs = nullptr;
  uint32_t* d_sizes = nullptr;
  CHECK(hipMalloc(&d_base, base.size() + 16) == hipSuccess);
  CHECK(hipMalloc(&d_offs, n * 8) == hipSuccess);
  CHECK(hipMalloc(&d_sizes, n * 4) == hipSuccess);
  CHECK(hipMemcpy(d_base, base.data(), base.size(), hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemcpy(d_offs, offs.data(), n * 8, hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemcpy(d_sizes, sizes.data(), n * 4, hipMemcpyHostToDevice) == hipSuccess);
  for (int pass = 0; pass < 2 && !g_fail; ++pass) {
    CHECK(dev.FrameDevice(d_base, base.size(), d_offs, d_sizes, pass ? nullptr : sizes.data(), n,
                          block_offset).ok());
    CHECK(dev.size() == host.size() && dev.size() > 0);
    CHECK(dev.end_block_offset() == host.end_block_offset());
    CHECK(dev.physical_records() == host.physical_records());
    CHECK(dev.bad_records() == 0 && dev.device_data() != nullptr);
    std::string image(dev.size(), '\0');
    CHECK(hipMemcpy(&image[0], dev.device_data(), image.size(), hipMemcpyDeviceToHost) ==
          hipSuccess);
    CHECK(image.size() == host.size() && std::memcmp(image.data(), host.data(), image.size()) == 0);
  }
  std::printf("case %llu %llu %u\n", static_cast<unsigned long long>(dev.size()),
              static_cast<unsigned long long>(dev.physical_records()), dev.end_block_offset());
  (void)hipFree(d_base), (void)hipFree(d_offs), (void)hipFree(d_sizes);
  std::printf(g_fail ? "FAILED %d\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
