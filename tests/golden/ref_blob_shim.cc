// tests/golden/ref_blob_shim.cc -- TEST INFRASTRUCTURE ONLY: a C veneer over
// the reference's OWN blob file code (db/blob/), linked against the reference
// archive by tests/golden/refbuild.py for tests/golden/gen_blob_golden.py.
// Nothing is restated here: the files are written by a DB with
// enable_blob_files and by BlobLogWriter, and read by BlobFileReader and
// BlobLogSequentialReader; the generator records what they say.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "db/blob/blob_contents.h"
#include "db/blob/blob_file_reader.h"
#include "db/blob/blob_log_format.h"
#include "db/blob/blob_log_sequential_reader.h"
#include "db/blob/blob_log_writer.h"
#include "file/read_write_util.h"
#include "file/filename.h"
#include "file/random_access_file_reader.h"
#include "file/writable_file_writer.h"
#include "options/cf_options.h"
#include "rocksdb/db.h"
#include "rocksdb/file_system.h"
#include "rocksdb/options.h"

#define REF_API extern "C" __attribute__((visibility("default")))

using namespace ROCKSDB_NAMESPACE;

namespace {

int put_msg(const std::string& s, char* msg, size_t cap) {
  if (s.size() + 1 > cap) return -9;
  std::memcpy(msg, s.c_str(), s.size() + 1);
  return 0;
}

struct Items {
  std::vector<Slice> v;
  Items(const char* blob, const uint64_t* lens, size_t n) {
    size_t p = 0;
    for (size_t i = 0; i < n; ++i) {
      v.emplace_back(blob + p, lens[i]);
      p += lens[i];
    }
  }
};

ImmutableOptions immutable_for(const std::string& dir, Options* options) {
  options->cf_paths.emplace_back(dir, 0);
  options->enable_blob_files = true;
  return ImmutableOptions(*options);
}

}  // namespace

// A DB with a non-default column family whose values all go to blob files
// (min_blob_size = 0), flushed: the *.blob files stay in `dir`.
REF_API int ref_blob_db_write(const char* dir, int compression, size_t n, const char* keys,
                              const uint64_t* key_lens, const char* vals,
                              const uint64_t* val_lens, uint32_t* cf_id, char* msg, size_t cap) {
  Options options;
  options.create_if_missing = true;
  DB* db = nullptr;
  Status s = DB::Open(options, dir, &db);
  if (!s.ok()) return put_msg(s.ToString(), msg, cap) ? -9 : -1;
  ColumnFamilyOptions cfo;
  cfo.enable_blob_files = true;
  cfo.min_blob_size = 0;
  cfo.blob_compression_type = static_cast<CompressionType>(compression);
  ColumnFamilyHandle* cf = nullptr;
  s = db->CreateColumnFamily(cfo, "blobs", &cf);
  const Items k(keys, key_lens, n), v(vals, val_lens, n);
  for (size_t i = 0; s.ok() && i < n; ++i) s = db->Put(WriteOptions(), cf, k.v[i], v.v[i]);
  if (s.ok()) s = db->Flush(FlushOptions(), cf);
  if (cf) {
    *cf_id = cf->GetID();
    db->DestroyColumnFamilyHandle(cf).PermitUncheckedError();
  }
  db->Close().PermitUncheckedError();
  delete db;
  put_msg(s.ToString(), msg, cap);
  return s.ok() ? 0 : -1;
}

// One blob file through BlobLogWriter (header, AddRecord per item with its
// expiration, footer): the shapes a DB does not produce.
REF_API int ref_blob_write_file(const char* dir, uint64_t number, uint32_t cf_id, int compression,
                                int has_ttl, uint64_t hdr_e0, uint64_t hdr_e1, uint64_t ftr_e0,
                                uint64_t ftr_e1, size_t n, const char* keys,
                                const uint64_t* key_lens, const char* vals,
                                const uint64_t* val_lens, const uint64_t* expirations, char* msg,
                                size_t cap) {
  Options options;
  const ImmutableOptions io = immutable_for(dir, &options);
  const std::string path = BlobFileName(dir, number);
  std::unique_ptr<FSWritableFile> file;
  Status s = NewWritableFile(io.fs.get(), path, &file, FileOptions());
  if (!s.ok()) return put_msg(s.ToString(), msg, cap) ? -9 : -1;
  std::unique_ptr<WritableFileWriter> fw(
      new WritableFileWriter(std::move(file), path, FileOptions(), io.clock));
  BlobLogWriter w(std::move(fw), io.clock, nullptr, number, /*use_fsync=*/false,
                  /*do_flush=*/false);
  BlobLogHeader header(cf_id, static_cast<CompressionType>(compression), has_ttl != 0,
                       ExpirationRange(hdr_e0, hdr_e1));
  s = w.WriteHeader(header);
  const Items k(keys, key_lens, n), v(vals, val_lens, n);
  for (size_t i = 0; s.ok() && i < n; ++i) {
    uint64_t ko = 0, bo = 0;
    s = w.AddRecord(k.v[i], v.v[i], expirations[i], &ko, &bo);
  }
  if (s.ok()) {
    BlobLogFooter footer;
    footer.blob_count = n;
    footer.expiration_range = ExpirationRange(ftr_e0, ftr_e1);
    std::string method, value;
    s = w.AppendFooter(footer, &method, &value);
  }
  put_msg(s.ToString(), msg, cap);
  return s.ok() ? 0 : -1;
}

// BlobFileReader::Create's Status string
REF_API int ref_blob_create(const char* dir, uint64_t number, uint32_t cf_id, char* msg,
                            size_t cap) {
  Options options;
  const ImmutableOptions io = immutable_for(dir, &options);
  std::unique_ptr<BlobFileReader> reader;
  const Status s = BlobFileReader::Create(io, ReadOptions(), FileOptions(), cf_id, nullptr, number,
                                          nullptr, &reader);
  return put_msg(s.ToString(), msg, cap);
}

// BlobFileReader::GetBlob with verify_checksums: its Status string
REF_API int ref_blob_get(const char* dir, uint64_t number, uint32_t cf_id, const char* key,
                         size_t key_len, uint64_t value_offset, uint64_t value_size, char* msg,
                         size_t cap) {
  Options options;
  const ImmutableOptions io = immutable_for(dir, &options);
  std::unique_ptr<BlobFileReader> reader;
  Status s = BlobFileReader::Create(io, ReadOptions(), FileOptions(), cf_id, nullptr, number,
                                    nullptr, &reader);
  if (!s.ok()) return put_msg("Create: " + s.ToString(), msg, cap);
  ReadOptions ro;
  ro.verify_checksums = true;
  std::unique_ptr<BlobContents> value;
  uint64_t bytes_read = 0;
  // (kNoCompression: the stored bytes are what the CRC covers; the value is not decoded)
  s = reader->GetBlob(ro, Slice(key, key_len), value_offset, value_size,
                      reader->GetCompressionType(), nullptr, nullptr, &value, &bytes_read);
  return put_msg(s.ToString(), msg, cap);
}

// BlobLogSequentialReader over the file: one line per step,
//   H <status>                                           ReadHeader
//   R <offset> <key_size> <value_size> <expiration> <header_crc> <blob_crc> <status>
//                                                        ReadRecord(kReadHeaderKeyBlob)
//   F <blob_count> <status>                              ReadFooter
// records until the footer offset or the first failure.
REF_API int ref_blob_sequential(const char* dir, uint64_t number, char* out, size_t cap,
                                size_t* out_len) {
  Options options;
  const ImmutableOptions io = immutable_for(dir, &options);
  const std::string path = BlobFileName(dir, number);
  uint64_t size = 0;
  Status s = io.fs->GetFileSize(path, IOOptions(), &size, nullptr);
  if (!s.ok()) return -1;
  std::unique_ptr<RandomAccessFileReader> fr;
  s = RandomAccessFileReader::Create(io.fs, path, FileOptions(), &fr, nullptr);
  if (!s.ok()) return -1;
  BlobLogSequentialReader reader(std::move(fr), io.clock, nullptr);
  std::string t;
  char buf[256];
  BlobLogHeader header;
  s = reader.ReadHeader(&header);
  t += "H " + s.ToString() + "\n";
  while (s.ok() && reader.GetNextByte() + BlobLogFooter::kSize < size) {
    BlobLogRecord rec;
    const uint64_t at = reader.GetNextByte();
    s = reader.ReadRecord(&rec, BlobLogSequentialReader::kReadHeaderKeyBlob, nullptr);
    std::snprintf(buf, sizeof(buf), "R %llu %llu %llu %llu %u %u ",
                  static_cast<unsigned long long>(at),
                  static_cast<unsigned long long>(rec.key_size),
                  static_cast<unsigned long long>(rec.value_size),
                  static_cast<unsigned long long>(rec.expiration), rec.header_crc, rec.blob_crc);
    t += buf + s.ToString() + "\n";
  }
  if (s.ok()) {
    BlobLogFooter footer;
    s = reader.ReadFooter(&footer);
    std::snprintf(buf, sizeof(buf), "F %llu ", static_cast<unsigned long long>(footer.blob_count));
    t += buf + s.ToString() + "\n";
  }
  *out_len = t.size();
  if (t.size() > cap) return 1;
  std::memcpy(out, t.data(), t.size());
  return 0;
}
