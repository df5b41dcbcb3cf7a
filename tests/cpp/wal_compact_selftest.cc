// tests/cpp/wal_compact_selftest.cc -- TEST INFRASTRUCTURE ONLY.
// forst_gpu::WalRecovery::CompactRecords against the bytes Next() hands out,
// record for record, and KvProtection::WriteBatchProtectionDevice on the
// compacted records against WriteBatchProtection on the host bytes.
//   wal_compact_selftest <log file> <log number> <mode> <protect: 0 | 1> [...]
// protect = 1 for logs whose records are WriteBatch reps (on other bytes the
// header's count field asks for billions of protection slots).
// Prints one "case <file> <records> <arena bytes>" line per log, then PASS.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
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

template <class T>
static std::vector<T> down(const T* d, uint64_t n) {
  std::vector<T> v(n);
  if (n) CHECK(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
  return v;
}

static void one(const char* path, uint32_t log_number, int mode, bool protect, WalRecovery& rec,
                KvProtection& kv) {
  std::ifstream f(path, std::ios::binary);
  const std::string log((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  uint8_t* d_log = nullptr;
  CHECK(hipMalloc(&d_log, log.size() + 256) == hipSuccess);
  CHECK(hipMemcpy(d_log, log.data(), log.size(), hipMemcpyHostToDevice) == hipSuccess);
  const uint8_t* host = reinterpret_cast<const uint8_t*>(log.data());
  CHECK(rec.Recover(d_log, host, log.size(), log_number, mode).ok());
  WalDeviceRecords dev;
  CHECK(rec.CompactRecords(d_log, &dev).ok());
  const std::vector<uint8_t> arena = down(dev.arena, dev.arena_bytes);
  const std::vector<uint64_t> offs = down(dev.rep_offsets, dev.n);
  const std::vector<uint32_t> sizes = down(dev.rep_sizes, dev.n);
  const std::vector<uint8_t> st = down(dev.status, dev.n);
  // NextMeta: the same records without their bytes
  std::vector<WalRecord> meta;
  {
    WalRecord m;
    while (rec.NextMeta(&m)) {
      CHECK(m.data == nullptr);
      meta.push_back(m);
    }
    CHECK(rec.status().ok() && meta.size() == dev.n);
    CHECK(rec.Recover(d_log, host, log.size(), log_number, mode).ok());
    CHECK(rec.CompactRecords(d_log, &dev).ok());
  }
  // Next(), record for record
  std::vector<std::string> bytes;
  WalRecord r;
  uint64_t k = 0, expect_off = 0;
  bool same = true;
  while (rec.Next(&r)) {
    same &= k < dev.n && st[k] == 0 && sizes[k] == r.size && offs[k] == expect_off &&
            offs[k] + sizes[k] <= arena.size() &&
            std::memcmp(arena.data() + offs[k], r.data, r.size) == 0 &&
            k < meta.size() && meta[k].checksum == r.checksum && meta[k].size == r.size &&
            meta[k].offset == r.offset && meta[k].n_fragments == r.n_fragments &&
            meta[k].reports_before.size() == r.reports_before.size();
    const uint64_t end = expect_off + ((r.size + 15) & ~uint64_t{15});
    for (uint64_t x = expect_off + r.size; same && x < end; ++x) same &= arena[x] == 0;
    expect_off = end;
    bytes.emplace_back(r.data, r.size);
    ++k;
  }
  CHECK(rec.status().ok());
  CHECK(same && k == dev.n && expect_off == dev.arena_bytes);
  std::printf("case %s %llu %llu\n", path, static_cast<unsigned long long>(dev.n),
              static_cast<unsigned long long>(dev.arena_bytes));
  (void)hipFree(d_log);
  if (!protect) return;
  // the protection of the compacted records == of the host bytes
  std::vector<KvBytes> reps;
  for (const std::string& b : bytes) reps.push_back({b.data(), b.size()});
  std::vector<std::vector<uint64_t>> p_host, p_dev;
  std::vector<Status> s_host, s_dev;
  CHECK(kv.WriteBatchProtection(reps, &p_host, &s_host).ok());
  CHECK(kv.WriteBatchProtectionDevice(dev.arena, dev.arena_bytes, dev.rep_offsets, dev.rep_sizes,
                                      dev.n, &p_dev, &s_dev).ok());
  CHECK(p_host.size() == dev.n && p_dev.size() == dev.n && s_dev.size() == dev.n);
  bool prot_same = p_host == p_dev;
  for (uint64_t i = 0; prot_same && i < dev.n; ++i)
    prot_same &= s_host[i].ToString() == s_dev[i].ToString();
  uint64_t slots = 0, bad = 0;
  for (uint64_t i = 0; i < dev.n; ++i) {
    slots += p_dev[i].size();
    bad += !s_dev[i].ok();
  }
  CHECK(prot_same && slots > 0 && bad > 0 && bad < dev.n);
}

int main(int argc, char** argv) {
  WalRecovery rec;  // one object over every log: its device arrays are reused
  KvProtection kv;
  std::setvbuf(stdout, nullptr, _IOLBF, 0);  // (a log's line is out before the next one starts)
  for (int i = 1; i + 3 < argc; i += 4)
    one(argv[i], static_cast<uint32_t>(std::atoi(argv[i + 1])), std::atoi(argv[i + 2]),
        std::atoi(argv[i + 3]) != 0, rec, kv);
  std::printf(g_fail ? "FAILED %d\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
