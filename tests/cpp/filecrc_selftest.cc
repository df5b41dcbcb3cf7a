// tests/cpp/filecrc_selftest.cc -- the whole-file checksum side of the C++
// host shim (include/forst/checksum_engine.h) the way a ForSt call site would
// use it, on a real MI355X:
//   FileChecksums / VerifyFullFileChecksums over files staged in one device
//   arena (DB::VerifyFileChecksums), FileChecksumToString / FromString / Hex,
//   GpuTrailerWriter with Options::file_checksum and a SinkWithCrc, and the C
//   setters forst_trailer_writer_enable_file_checksum / _set_crc_sink /
//   _file_checksum.
// Prints PASS or FAIL lines; exit code 0 iff all passed.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "forst/checksum_engine.h"

using namespace forst_gpu;

static int g_fail = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                               \
    }                                                         \
  } while (0)

// test-only bytewise CRC32C (for expected values)
static uint32_t crc32c_ref(uint32_t init, const uint8_t* p, size_t n) {
  uint32_t c = ~init;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
  }
  return ~c;
}

static std::vector<uint8_t> bytes(size_t n, uint32_t seed) {
  std::vector<uint8_t> v(n);
  uint32_t x = seed * 2654435761u + 1;
  for (size_t i = 0; i < n; ++i) {
    x = x * 1664525u + 1013904223u;
    v[i] = static_cast<uint8_t>(x >> 24);
  }
  return v;
}

static void strings() {
  const std::string s = FileChecksumToString(0x0A1B2C3Du);
  CHECK(s == std::string("\x0a\x1b\x2c\x3d", 4));
  uint32_t c = 0;
  CHECK(FileChecksumFromString(s, &c) && c == 0x0A1B2C3Du);
  CHECK(!FileChecksumFromString("abc", &c) && !FileChecksumFromString("", nullptr));
  CHECK(FileChecksumHex(s) == "0A1B2C3D" && FileChecksumHex("") == "");
  CHECK(FileChecksumHex(FileChecksumToString(0xFFEE00A0u)) == "FFEE00A0");
}

static void files() {
  const size_t sizes[] = {0, 1, 65536, 65537, 300000, 70 * 65536 + 5};
  const size_t nf = sizeof(sizes) / sizeof(sizes[0]);
  std::vector<std::vector<uint8_t>> host;
  std::vector<SstFileRef> refs(nf);
  uint64_t total = 3;
  for (size_t i = 0; i < nf; ++i) {
    host.push_back(bytes(sizes[i], static_cast<uint32_t>(i + 1)));
    refs[i].file_size = sizes[i];
    refs[i].dev_offset = total;  // packed, odd offsets
    refs[i].file_name = "/db/00000" + std::to_string(i) + ".sst";
    total += sizes[i] + 1;
  }
  uint8_t* d = nullptr;
  CHECK(hipMalloc(&d, total + 256) == hipSuccess);
  CHECK(hipMemset(d, 0, total + 256) == hipSuccess);
  for (size_t i = 0; i < nf; ++i)
    if (sizes[i])
      CHECK(hipMemcpy(d + refs[i].dev_offset, host[i].data(), sizes[i], hipMemcpyHostToDevice) ==
            hipSuccess);
  BlockChecksumEngine eng;
  Status st;
  const std::vector<uint32_t> crcs = FileChecksums(eng, refs, d, total, &st);
  CHECK(st.ok() && crcs.size() == nf);
  std::vector<std::string> expected(nf);
  for (size_t i = 0; i < nf; ++i) {
    CHECK(crcs[i] == crc32c_ref(0, host[i].data(), sizes[i]));
    expected[i] = FileChecksumToString(crc32c_ref(0, host[i].data(), sizes[i]));
  }
  std::vector<Status> v = VerifyFullFileChecksums(eng, refs, d, total, expected);
  CHECK(v.size() == nf);
  for (const Status& s : v) CHECK(s.ok());
  // a wrong expectation, an unknown one over a corrupted file, a flipped data byte
  expected[2][3] ^= 1;
  expected[3].clear();
  uint8_t flip = host[3][100] ^ 0x40, flip5 = host[5][4000000] ^ 0x01;
  CHECK(hipMemcpy(d + refs[3].dev_offset + 100, &flip, 1, hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemcpy(d + refs[5].dev_offset + 4000000, &flip5, 1, hipMemcpyHostToDevice) == hipSuccess);
  host[5][4000000] = flip5;
  v = VerifyFullFileChecksums(eng, refs, d, total, expected);
  for (size_t i = 0; i < nf; ++i) {
    if (i == 2) {
      CHECK(v[i].IsCorruption());
      CHECK(v[i].ToString() == "Corruption: /db/000002.sst file checksum mismatch, expecting " +
                                   FileChecksumHex(expected[2]) + ", but actual " +
                                   FileChecksumHex(FileChecksumToString(crcs[2])));
    } else if (i == 5) {
      CHECK(v[i].ToString() ==
            "Corruption: /db/000005.sst file checksum mismatch, expecting " +
                FileChecksumHex(expected[5]) + ", but actual " +
                FileChecksumHex(FileChecksumToString(crc32c_ref(0, host[5].data(), sizes[5]))));
    } else {
      CHECK(v[i].ok());
    }
  }
  // a file reaching past the arena: InvalidArgument for the files that were read
  refs[1].dev_offset = total;
  v = VerifyFullFileChecksums(eng, refs, d, total, expected);
  CHECK(v[0].code() == Status::kInvalidArgument && v[3].ok());
  CHECK(VerifyFullFileChecksums(eng, refs, d, total, {})[0].code() == Status::kInvalidArgument);
  (void)hipFree(d);
}

struct Piece {
  std::string data;
  uint32_t crc;
};

static int c_sink(void* arg, const uint8_t* p, uint64_t n, uint32_t crc) {
  static_cast<std::vector<Piece>*>(arg)->push_back(
      Piece{std::string(reinterpret_cast<const char*>(p), n), crc});
  return 0;
}
static int c_plain_sink(void*, const uint8_t*, uint64_t) { return 1; }  // replaced before use

static void writer() {
  // the same blocks through the C++ class and through the C ABI
  const int nb = 200;
  std::vector<std::vector<uint8_t>> blocks;
  for (int i = 0; i < nb; ++i) blocks.push_back(bytes((i * 2654435761u) % 7000, 100 + i));
  GpuTrailerWriter::Options o;
  o.checksum = kCRC32c;
  o.window_bytes = 1 << 16;
  o.block_align = true;
  o.file_checksum = true;
  o.file_checksum_init = 0x13572468u;
  std::vector<Piece> a;
  GpuTrailerWriter w(o, GpuTrailerWriter::SinkWithCrc([&a](const char* p, size_t n, uint32_t crc) {
                       a.push_back(Piece{std::string(p, n), crc});
                       return Status::OK();
                     }));
  uint64_t ho, hs;
  for (int i = 0; i < nb; ++i)
    CHECK(w.AddBlock(reinterpret_cast<const char*>(blocks[i].data()), blocks[i].size(), i & 3,
                     i % 5 != 0, &ho, &hs).ok());
  CHECK(w.WriteFooter(5, 10, 20, 30, 40).ok());
  std::string all;
  for (const Piece& p : a) {
    CHECK(p.crc == crc32c_ref(0, reinterpret_cast<const uint8_t*>(p.data.data()), p.data.size()));
    all += p.data;
  }
  CHECK(a.size() > 5 && all.size() == w.offset());
  const uint32_t want =
      crc32c_ref(0x13572468u, reinterpret_cast<const uint8_t*>(all.data()), all.size());
  CHECK(w.file_checksum() == want);
  CHECK(w.FileChecksumString() == FileChecksumToString(want));
  CHECK(!w.EnableFileChecksum(0).ok());  // blocks were added

  std::vector<Piece> b;
  forst_trailer_writer* cw = nullptr;
  CHECK(forst_trailer_writer_open(FORST_kCRC32c, 0, 0, 4096, 1 << 16, c_plain_sink, nullptr, nullptr,
                                  &cw) == FORST_OK);
  CHECK(forst_trailer_writer_enable_file_checksum(cw, 0x13572468u) == FORST_OK);
  CHECK(forst_trailer_writer_set_crc_sink(cw, c_sink, &b) == FORST_OK);
  CHECK(forst_trailer_writer_set_crc_sink(cw, nullptr, &b) == FORST_EINVAL);
  for (int i = 0; i < nb; ++i)
    CHECK(forst_trailer_writer_add(cw, blocks[i].data(), blocks[i].size(), i & 3, i % 5 != 0, &ho,
                                   &hs) == FORST_OK);
  CHECK(forst_trailer_writer_enable_file_checksum(cw, 0) == FORST_EINVAL);
  CHECK(forst_trailer_writer_footer(cw, 5, 10, 20, 30, 40) == FORST_OK);
  uint32_t crc = 0;
  uint8_t be[4];
  CHECK(forst_trailer_writer_file_checksum(cw, &crc, be) == FORST_OK);
  CHECK(crc == want && std::string(reinterpret_cast<char*>(be), 4) == FileChecksumToString(want));
  CHECK(forst_trailer_writer_close(cw) == FORST_OK);
  CHECK(b.size() == a.size());
  for (size_t i = 0; i < a.size() && i < b.size(); ++i)
    CHECK(a[i].data == b[i].data && a[i].crc == b[i].crc);
}

int main() {
  strings();
  files();
  writer();
  std::printf(g_fail ? "FAILED %d\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
