// forst_amd/csrc/engine_shim.cc -- C++ host shim (namespace forst_gpu) over the
// C ABI; see include/forst/checksum_engine.h for the reference mapping.
#include "../../include/forst/checksum_engine.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>
#include <vector>

namespace forst_gpu {

std::string Status::ToString() const {
  switch (code_) {
    case kOk:
      return "OK";
    case kCorruption:
      return "Corruption: " + msg_;
    case kNotSupported:
      return "Not implemented: " + msg_;
    case kInvalidArgument:
      return "Invalid argument: " + msg_;
    case kIOError:
      return "IO error: " + msg_;
  }
  return msg_;
}

bool GpuSupportsChecksumType(ChecksumType t) {
  return t == kNoChecksum || t == kCRC32c || t == kxxHash || t == kxxHash64 || t == kXXH3;
}

// table/block_based/reader_common.cc:55-60
std::string BlockChecksumMismatchMessage(ChecksumType type, uint32_t stored, uint32_t computed,
                                         bool context_removed, const std::string& file_name,
                                         uint64_t offset, uint64_t block_size) {
  return "block checksum mismatch: stored" +
         std::string(context_removed ? "(context removed)" : "") + " = " +
         std::to_string(stored) + ", computed = " + std::to_string(computed) +
         ", type = " + std::to_string(static_cast<int>(type)) + "  in " + file_name + " offset " +
         std::to_string(offset) + " size " + std::to_string(block_size);
}

namespace {
Status FromRc(int rc) {
  if (rc == FORST_OK) return Status::OK();
  if (rc == FORST_EUNSUPPORTED) return Status::NotSupported(forst_last_error());
  if (rc == FORST_EINVAL) return Status::InvalidArgument(forst_last_error());
  return Status::IOError(forst_last_error());
}
Status FromHip(hipError_t e, const char* what) {
  if (e == hipSuccess) return Status::OK();
  return Status::IOError(std::string(what) + ": " + hipGetErrorString(e));
}
}  // namespace

BlockChecksumEngine::~BlockChecksumEngine() {
  (void)hipFree(d_computed_);
  (void)hipFree(d_stored_);
  (void)hipFree(d_ok_);
  (void)hipFree(d_mod_);
  (void)hipFree(d_bad_);
}

Status BlockChecksumEngine::EnsureScratch(uint64_t n) {
  if (!d_bad_) {
    Status s = FromHip(hipMalloc(&d_bad_, sizeof(*d_bad_)), "hipMalloc");
    if (!s.ok()) return s;
  }
  if (n <= cap_) return Status::OK();
  (void)hipFree(d_computed_);
  (void)hipFree(d_stored_);
  (void)hipFree(d_ok_);
  (void)hipFree(d_mod_);
  d_computed_ = d_stored_ = d_mod_ = nullptr;
  d_ok_ = nullptr;
  cap_ = 0;
  Status s = FromHip(hipMalloc(&d_computed_, n * 4), "hipMalloc");
  if (s.ok()) s = FromHip(hipMalloc(&d_stored_, n * 4), "hipMalloc");
  if (s.ok()) s = FromHip(hipMalloc(&d_ok_, n), "hipMalloc");
  if (s.ok()) s = FromHip(hipMalloc(&d_mod_, n * 4), "hipMalloc");
  if (s.ok()) cap_ = n;
  return s;
}

Status BlockChecksumEngine::ComputeChecksums(ChecksumType type, const DeviceBlockBatch& b,
                                             const uint8_t* last_bytes, const uint32_t* modifiers,
                                             uint32_t* out) {
  int rc = forst_block_checksum_batch(type, b.base, b.base_len, b.offsets, b.sizes, last_bytes,
                                      modifiers, out, b.n, stream_);
  if (rc == FORST_OK) stats_.block_checksum_compute_count += b.n;
  return FromRc(rc);
}

Status BlockChecksumEngine::WriteTrailers(ChecksumType type, const DeviceBlockBatch& b,
                                          const uint8_t* last_bytes, const uint32_t* modifiers,
                                          uint32_t* out) {
  int rc = forst_block_trailer_batch(type, const_cast<uint8_t*>(b.base), b.base_len, b.offsets,
                                     b.sizes, last_bytes, modifiers, out, b.n, stream_);
  if (rc == FORST_OK) stats_.block_checksum_compute_count += b.n;
  return FromRc(rc);
}

Status BlockChecksumEngine::VerifyBlocks(ChecksumType type, uint32_t base_context_checksum,
                                         const DeviceBlockBatch& b, const std::string& file_name,
                                         const std::vector<uint64_t>& file_offsets,
                                         std::vector<uint64_t>* failed) {
  if (!IsSupportedChecksumType(type)) {
    // format.cc:385-388 (footer decode rejects unknown types)
    return Status::Corruption("Corrupt or unsupported checksum type: " +
                              std::to_string(static_cast<int>(type)));
  }
  if (b.n == 0) return Status::OK();
  if (file_offsets.size() != b.n) return Status::InvalidArgument("file_offsets.size() != n");
  // PERF_TIMER_GUARD(block_checksum_time) (reader_common.cc:29), per batch
  struct Timer {
    uint64_t* acc;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~Timer() {
      *acc += static_cast<uint64_t>(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                        std::chrono::steady_clock::now() - t0)
                                        .count());
    }
  } timer{&stats_.block_checksum_time};
  Status s = EnsureScratch(b.n);
  if (!s.ok()) return s;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  const uint32_t* mods = nullptr;
  std::vector<uint32_t> hmods;
  if (base_context_checksum != 0) {  // format_version >= 6
    hmods.resize(b.n);
    for (uint64_t i = 0; i < b.n; ++i)
      hmods[i] = ChecksumModifierForContext(base_context_checksum, file_offsets[i]);
    s = FromHip(hipMemcpyAsync(d_mod_, hmods.data(), b.n * 4, hipMemcpyHostToDevice, st),
                "hipMemcpyAsync");
    if (!s.ok()) return s;
    mods = d_mod_;
  }
  s = FromHip(hipMemsetAsync(d_bad_, 0, sizeof(*d_bad_), st), "hipMemsetAsync");
  if (!s.ok()) return s;
  int rc = forst_block_verify_batch(type, b.base, b.base_len, b.offsets, b.sizes, mods,
                                    d_computed_, d_stored_, d_ok_, d_bad_, b.n, stream_);
  if (rc != FORST_OK) return FromRc(rc);
  unsigned long long bad = 0;
  s = FromHip(hipMemcpyAsync(&bad, d_bad_, sizeof(bad), hipMemcpyDeviceToHost, st), "hipMemcpy");
  if (s.ok()) s = FromHip(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (!s.ok()) return s;
  stats_.block_checksum_compute_count += b.n;
  if (bad == 0) return Status::OK();
  stats_.block_checksum_mismatch_count += bad;
  std::vector<uint8_t> ok(b.n);
  std::vector<uint32_t> computed(b.n), stored(b.n), sizes(b.n);
  s = FromHip(hipMemcpy(ok.data(), d_ok_, b.n, hipMemcpyDeviceToHost), "hipMemcpy");
  if (s.ok()) s = FromHip(hipMemcpy(computed.data(), d_computed_, b.n * 4, hipMemcpyDeviceToHost), "hipMemcpy");
  if (s.ok()) s = FromHip(hipMemcpy(stored.data(), d_stored_, b.n * 4, hipMemcpyDeviceToHost), "hipMemcpy");
  if (s.ok()) s = FromHip(hipMemcpy(sizes.data(), b.sizes, b.n * 4, hipMemcpyDeviceToHost), "hipMemcpy");
  if (!s.ok()) return s;
  Status first = Status::OK();
  for (uint64_t i = 0; i < b.n; ++i) {
    if (ok[i]) continue;
    if (failed) failed->push_back(i);
    if (first.ok()) {
      uint32_t st_v = stored[i], co_v = computed[i];
      if (type == kCRC32c) {  // reader_common.cc:50-54
        st_v = crc32c::Unmask(st_v);
        co_v = crc32c::Unmask(co_v);
      }
      const uint32_t modifier = ChecksumModifierForContext(base_context_checksum, file_offsets[i]);
      first = Status::Corruption(BlockChecksumMismatchMessage(
          type, st_v, co_v, modifier != 0, file_name, file_offsets[i], sizes[i]));
    }
  }
  return first;
}

// ---- blob files ----------------------------------------------------------------

BlobRecords::~BlobRecords() { (void)hipFree(dev_); }

uint8_t* BlobRecords::Grow(uint64_t bytes, Status* s) {
  if (bytes > cap_) {
    (void)hipFree(dev_);
    dev_ = nullptr;
    cap_ = 0;
    *s = FromHip(hipMalloc(&dev_, bytes), "hipMalloc");
    if (!s->ok()) return nullptr;
    cap_ = bytes;
  }
  return static_cast<uint8_t*>(dev_);
}

bool BlobRecords::IsValidBlobOffset(uint64_t value_offset, uint64_t key_size, uint64_t value_size,
                                    uint64_t file_size) {
  // BlobLogHeader::kSize 30, BlobLogRecord::kHeaderSize 32, BlobLogFooter::kSize 32
  if (value_offset < 30 + 32 + key_size) return false;
  if (value_offset + value_size + 32 > file_size) return false;
  return true;
}

Status BlobRecords::RecordStatus(uint8_t code) {
  switch (code) {
    case FORST_BLOB_OK:
      return Status::OK();
    case FORST_BLOB_HEADER_CRC:
      return Status::Corruption("Error while decoding blob record: Header CRC mismatch");
    case FORST_BLOB_KEY_SIZE:
      return Status::Corruption("Key size mismatch when reading blob");
    case FORST_BLOB_VALUE_SIZE:
      return Status::Corruption("Value size mismatch when reading blob");
    case FORST_BLOB_KEY:
      return Status::Corruption("Key mismatch when reading blob");
    case FORST_BLOB_CRC:
      return Status::Corruption("Blob CRC mismatch");
    case FORST_BLOB_OUT_OF_RANGE:
      return Status::InvalidArgument("blob record outside the device buffer");
    case FORST_BLOB_TOO_LARGE:
      return Status::InvalidArgument("blob record larger than 4 GiB");
  }
  return Status::InvalidArgument("unknown blob record status " + std::to_string(code));
}

Status BlobRecords::FileStatus(const forst_blob_file_result& r) {
  if (r.reason == FORST_BLOB_FILE_OK) return Status::OK();
  const std::string text = forst_blob_file_reason_text(r.reason);  // "Corruption: <message>"
  return Status::Corruption(text.substr(text.find(": ") + 2));
}

Status BlobRecords::VerifyRecords(const uint8_t* dev_file, uint64_t file_size,
                                  const std::vector<BlobRequest>& requests,
                                  std::vector<Status>* statuses) {
  const uint64_t n = requests.size();
  statuses->assign(n, Status::OK());
  if (!n) return Status::OK();
  // one host image of the request arrays: record offsets, key sizes, value
  // sizes, user key offsets (u64 x n each), then the user keys
  uint64_t key_bytes = 0;
  for (const BlobRequest& r : requests) key_bytes += r.user_key_size;
  const uint64_t keys_at = 32 * n, status_at = (keys_at + key_bytes + 7) & ~uint64_t(7);
  std::vector<uint8_t> img(status_at + n);
  uint64_t* off = reinterpret_cast<uint64_t*>(img.data());
  uint64_t *eks = off + n, *evs = off + 2 * n, *uko = off + 3 * n;
  uint64_t kpos = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const BlobRequest& r = requests[i];
    const bool valid = IsValidBlobOffset(r.offset, r.user_key_size, r.value_size, file_size);
    // BlobIndex offset - BlobLogRecord::CalculateAdjustmentForRecordHeader(key_size)
    off[i] = valid ? r.offset - (r.user_key_size + 32) : UINT64_MAX;
    eks[i] = r.user_key_size;
    evs[i] = r.value_size;
    uko[i] = kpos;
    if (r.user_key_size) std::memcpy(img.data() + keys_at + kpos, r.user_key, r.user_key_size);
    kpos += r.user_key_size;
    if (!valid) (*statuses)[i] = Status::Corruption("Invalid blob offset");
  }
  Status s;
  uint8_t* d = Grow(img.size(), &s);
  if (!d) return s;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  // blocking copies: the pageable image is read before hipMemcpy returns
  s = FromHip(hipMemcpy(d, img.data(), status_at, hipMemcpyHostToDevice), "hipMemcpy");
  if (!s.ok()) return s;
  const uint64_t* d64 = reinterpret_cast<const uint64_t*>(d);
  s = FromRc(forst_blob_verify_batch(dev_file, file_size, d64, d64 + n, d64 + 2 * n, d + keys_at,
                                     key_bytes, d64 + 3 * n, d + status_at, nullptr, nullptr,
                                     nullptr, n, stream_));
  if (s.ok()) s = FromHip(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (s.ok())
    s = FromHip(hipMemcpy(img.data() + status_at, d + status_at, n, hipMemcpyDeviceToHost),
                "hipMemcpy");
  if (!s.ok()) return s;
  for (uint64_t i = 0; i < n; ++i)
    if ((*statuses)[i].ok()) (*statuses)[i] = RecordStatus(img[status_at + i]);
  return Status::OK();
}

Status BlobRecords::FillRecordCrcs(uint8_t* dev_image, uint64_t image_len,
                                   const std::vector<uint64_t>& record_offsets,
                                   std::vector<uint8_t>* status) {
  const uint64_t n = record_offsets.size();
  if (status) status->assign(n, 0);
  if (!n) return Status::OK();
  Status s;
  uint8_t* d = Grow(9 * n, &s);
  if (!d) return s;
  s = FromHip(hipMemcpy(d, record_offsets.data(), 8 * n, hipMemcpyHostToDevice), "hipMemcpy");
  if (!s.ok()) return s;
  s = FromRc(forst_blob_record_crc_batch(dev_image, image_len, reinterpret_cast<uint64_t*>(d),
                                         d + 8 * n, nullptr, nullptr, n, stream_));
  if (s.ok())
    s = FromHip(hipStreamSynchronize(static_cast<hipStream_t>(stream_)), "hipStreamSynchronize");
  if (s.ok() && status)
    s = FromHip(hipMemcpy(status->data(), d + 8 * n, n, hipMemcpyDeviceToHost), "hipMemcpy");
  return s;
}

std::vector<Status> BlobRecords::VerifyFiles(const std::vector<BlobFileRef>& files,
                                             const uint8_t* dev_arena, uint64_t arena_len,
                                             std::vector<forst_blob_file_result>* results) {
  const uint64_t n = files.size();
  std::vector<const uint8_t*> host(n);
  std::vector<uint64_t> sizes(n), offs(n);
  std::vector<uint32_t> cfs(n);
  for (uint64_t i = 0; i < n; ++i) {
    host[i] = files[i].host_file;
    sizes[i] = files[i].file_size;
    offs[i] = files[i].dev_offset;
    cfs[i] = files[i].column_family_id;
  }
  std::vector<forst_blob_file_result> res(n);
  const Status call = FromRc(forst_blob_verify_files(host.data(), sizes.data(), offs.data(),
                                                     dev_arena, arena_len, cfs.data(), n,
                                                     res.data(), stream_));
  std::vector<Status> out(n, call);
  if (call.ok())
    for (uint64_t i = 0; i < n; ++i) out[i] = FileStatus(res[i]);
  if (results) *results = std::move(res);
  return out;
}

}  // namespace forst_gpu
