// forst_amd/csrc/blob_host.h -- the host side of forst_blob_verify_files: the
// structure walk of one blob file (db/blob/blob_log_format.h) and the texts of
// its outcomes.  Pure functions, no HIP call: shared by the C ABI (capi.hip)
// and blob_host.cc, which exports the walk on its own.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/forst_checksum.h"

namespace forst {
namespace blobhost {

constexpr uint32_t kMagic = 2395959;  // blob_log_format.h:20
constexpr uint32_t kVersion1 = 1;     // :21
constexpr uint64_t kFileHdr = 30;     // BlobLogHeader::kSize
constexpr uint64_t kFooter = 32;      // BlobLogFooter::kSize
constexpr uint64_t kRecHdr = 32;      // BlobLogRecord::kHeaderSize

inline uint32_t le32(const uint8_t* p) {
  uint32_t v;
  std::memcpy(&v, p, 4);
  return v;  // (gfx950 hosts are little-endian)
}
inline uint64_t le64(const uint8_t* p) {
  uint64_t v;
  std::memcpy(&v, p, 8);
  return v;
}

inline const char* reason_text(int reason) {
  switch (reason) {
    case FORST_BLOB_FILE_OK:
      return "OK";
    case FORST_BLOB_FILE_MALFORMED:
      return "Corruption: Malformed blob file";
    case FORST_BLOB_FILE_HEADER_MAGIC:
      return "Corruption: Error while decoding blob log header: Magic number mismatch";
    case FORST_BLOB_FILE_HEADER_VERSION:
      return "Corruption: Error while decoding blob log header: Unknown header version";
    case FORST_BLOB_FILE_TTL:
      return "Corruption: Unexpected TTL blob file";
    case FORST_BLOB_FILE_CF_MISMATCH:
      return "Corruption: Column family ID mismatch";
    case FORST_BLOB_FILE_FOOTER_MAGIC:
      return "Corruption: Error while decoding blob log footer: Magic number mismatch";
    case FORST_BLOB_FILE_FOOTER_CRC:
      return "Corruption: Error while decoding blob log footer: CRC mismatch";
    case FORST_BLOB_FILE_RECORD_HEADER_CRC:
      return "Corruption: Error while decoding blob record: Header CRC mismatch";
    case FORST_BLOB_FILE_RECORD_BLOB_CRC:
      return "Corruption: Blob CRC mismatch";
    case FORST_BLOB_FILE_RECORD_CROSSES_FOOTER:  // (no reference twin)
      return "Corruption: Blob record crosses the blob file footer";
    case FORST_BLOB_FILE_BLOB_COUNT_MISMATCH:  // (no reference twin)
      return "Corruption: Blob count mismatch between the footer and the records";
    case FORST_BLOB_FILE_RECORD_TOO_LARGE:  // (no reference twin)
      return "Corruption: Blob record larger than 4 GiB";
  }
  return "Corruption: unknown blob file failure";
}

struct Walk {
  uint64_t n_records = 0;    // headers that fit in front of the footer
  bool tail_crosses = false; // the last of them has a payload that does not
  bool trailing = false;     // bytes left in front of the footer, too few for a header
  uint64_t end_pos = 0;      // where the walk stopped
  uint64_t footer_blob_count = 0;
  bool footer_ttl = false;   // ReadFooter's TTL check, applied after the footer CRC
};

inline void fail(forst_blob_file_result* r, int reason) {
  r->status = 2;  // Status::kCorruption
  r->reason = reason;
}

// The checks BlobFileReader::Create makes without a CRC, in its order
// (OpenFile's size check, ReadHeader, the footer's magic), then the record
// offsets from byte 30: 16 bytes read per record (key_size, value_size), a
// step of 32 + key_size + value_size.  Every step moves at least 32 bytes, so
// damaged sizes cannot loop.
//
// The walk trusts sizes it has not verified.  That is safe: the caller checks
// every listed record's header CRC and reports the FIRST failing record in
// file order, so whatever the walk derived from a damaged header lies behind
// that record and is discarded with it.
//
// emit(offset) is called per record; r receives the decoded header fields,
// blob_count / total_blob_bytes, and the host-decided failure (reason stays
// FORST_BLOB_FILE_OK when only CRC results can still fail the file).
template <typename Emit>
inline Walk walk_file(const uint8_t* f, uint64_t size, const uint32_t* expect_cf,
                      forst_blob_file_result* r, Emit emit) {
  Walk w;
  std::memset(r, 0, sizeof(*r));
  r->fail_index = UINT64_MAX;
  if (size < kFileHdr + kFooter) {  // blob_file_reader.cc:108
    fail(r, FORST_BLOB_FILE_MALFORMED);
    return w;
  }
  // BlobLogHeader::DecodeFrom (blob_log_format.cc:28-57)
  if (le32(f) != kMagic) {
    fail(r, FORST_BLOB_FILE_HEADER_MAGIC);
    return w;
  }
  if (le32(f + 4) != kVersion1) {
    fail(r, FORST_BLOB_FILE_HEADER_VERSION);
    return w;
  }
  r->column_family_id = le32(f + 8);
  r->has_ttl = (f[12] & 1) == 1;
  r->compression = f[13];
  // ReadHeader (blob_file_reader.cc:179-185)
  if (r->has_ttl || le64(f + 14) != 0 || le64(f + 22) != 0) {
    fail(r, FORST_BLOB_FILE_TTL);
    return w;
  }
  if (expect_cf && r->column_family_id != *expect_cf) {
    fail(r, FORST_BLOB_FILE_CF_MISMATCH);
    return w;
  }
  // BlobLogFooter::DecodeFrom (blob_log_format.cc:72-94): magic, then the CRC
  // (the caller's), then ReadFooter's TTL check
  const uint64_t foot = size - kFooter;
  if (le32(f + foot) != kMagic) {
    fail(r, FORST_BLOB_FILE_FOOTER_MAGIC);
    return w;
  }
  w.footer_blob_count = le64(f + foot + 4);
  w.footer_ttl = le64(f + foot + 12) != 0 || le64(f + foot + 20) != 0;
  uint64_t pos = kFileHdr;
  while (pos < foot) {
    if (foot - pos < kRecHdr) {
      w.trailing = true;
      break;
    }
    const uint64_t ks = le64(f + pos), vs = le64(f + pos + 8);
    const uint64_t room = foot - pos - kRecHdr, sum = ks + vs;
    emit(pos);
    ++w.n_records;
    if (sum < ks || sum > room) {
      w.tail_crosses = true;
      break;
    }
    r->total_blob_bytes += kRecHdr + sum;
    pos += kRecHdr + sum;
  }
  w.end_pos = pos;
  r->blob_count = w.n_records - (w.tail_crosses ? 1 : 0);
  return w;
}

// The file's outcome from the walk and the CRC results, in the order of
// forst_blob_verify_files: footer CRC, footer TTL, the first failing record,
// a record across the footer, the blob count.  rec_status[k] = the
// FORST_BLOB_* code of walked record k, footer_status that of the footer.
inline void resolve_file(const Walk& w, const uint64_t* rec_offsets, const uint8_t* rec_status,
                         uint8_t footer_status, forst_blob_file_result* r) {
  if (r->reason != FORST_BLOB_FILE_OK) return;
  if (footer_status != FORST_BLOB_OK) return fail(r, FORST_BLOB_FILE_FOOTER_CRC);
  if (w.footer_ttl) return fail(r, FORST_BLOB_FILE_TTL);
  for (uint64_t k = 0; k < w.n_records; ++k) {
    const bool last_crosses = w.tail_crosses && k + 1 == w.n_records;
    int reason = FORST_BLOB_FILE_OK;
    if (rec_status[k] == FORST_BLOB_HEADER_CRC)
      reason = FORST_BLOB_FILE_RECORD_HEADER_CRC;
    else if (last_crosses)  // (its header is sound: the sizes are what was written)
      reason = FORST_BLOB_FILE_RECORD_CROSSES_FOOTER;
    else if (rec_status[k] == FORST_BLOB_CRC)
      reason = FORST_BLOB_FILE_RECORD_BLOB_CRC;
    else if (rec_status[k] == FORST_BLOB_TOO_LARGE)
      reason = FORST_BLOB_FILE_RECORD_TOO_LARGE;
    else if (rec_status[k] != FORST_BLOB_OK)  // (the arena was range-checked: not reached)
      reason = FORST_BLOB_FILE_RECORD_CROSSES_FOOTER;
    if (reason != FORST_BLOB_FILE_OK) {
      r->fail_index = k;
      r->fail_offset = rec_offsets[k];
      // what the walk derived behind the failing record is discarded
      r->blob_count = k;
      r->total_blob_bytes = rec_offsets[k] - kFileHdr;
      return fail(r, reason);
    }
  }
  if (w.trailing) {
    r->fail_index = w.n_records;
    r->fail_offset = w.end_pos;
    return fail(r, FORST_BLOB_FILE_RECORD_CROSSES_FOOTER);
  }
  if (w.n_records != w.footer_blob_count) return fail(r, FORST_BLOB_FILE_BLOB_COUNT_MISMATCH);
}

}  // namespace blobhost
}  // namespace forst
