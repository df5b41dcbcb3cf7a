// tests/golden/ref_wal_writer_shim.cc -- TEST INFRASTRUCTURE ONLY (fixture veneer).
//
// A C entry point over the REFERENCE's own log::Writer (db/log_writer.cc),
// compiled by tests/golden/gen_wal_writer_golden.py against the reference
// archive (tests/golden/refbuild.py) in a temporary directory and never
// shipped.  The writer appends to an in-memory FSWritableFile; each record of
// the given lengths, cut back to back from `payload`, goes through
// AddRecord (log_writer.cc:65), legacy or recyclable, and the bytes the file
// received are handed back.
#include <cstring>
#include <memory>
#include <string>

#include "db/log_writer.h"
#include "file/writable_file_writer.h"
#include "rocksdb/file_system.h"

using namespace ROCKSDB_NAMESPACE;

namespace {

class MemSink : public FSWritableFile {
 public:
  explicit MemSink(std::string* out) : out_(out) {}
  using FSWritableFile::Append;
  IOStatus Append(const Slice& data, const IOOptions&, IODebugContext*) override {
    out_->append(data.data(), data.size());
    return IOStatus::OK();
  }
  IOStatus Close(const IOOptions&, IODebugContext*) override { return IOStatus::OK(); }
  IOStatus Flush(const IOOptions&, IODebugContext*) override { return IOStatus::OK(); }
  IOStatus Sync(const IOOptions&, IODebugContext*) override { return IOStatus::OK(); }
  uint64_t GetFileSize(const IOOptions&, IODebugContext*) override { return out_->size(); }

 private:
  std::string* out_;
};

}  // namespace

// 0: *out_len = the log's size, copied to out when it fits (cap); 1: an
// AddRecord or the final flush failed
extern "C" __attribute__((visibility("default"))) int ref_wal_write(
    const char* payload, const unsigned* lengths, size_t n, int recyclable,
    unsigned long long log_number, char* out, size_t cap, size_t* out_len) {
  std::string log;
  {
    std::unique_ptr<FSWritableFile> sink(new MemSink(&log));
    std::unique_ptr<WritableFileWriter> file(
        new WritableFileWriter(std::move(sink), "wal", FileOptions()));
    log::Writer writer(std::move(file), log_number, recyclable != 0);
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {
      if (!writer.AddRecord(Slice(payload + at, lengths[i])).ok()) return 1;
      at += lengths[i];
    }
    if (!writer.WriteBuffer().ok()) return 1;
    if (!writer.Close().ok()) return 1;
  }
  *out_len = log.size();
  if (log.size() <= cap) std::memcpy(out, log.data(), log.size());
  return 0;
}
