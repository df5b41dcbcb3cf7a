// forst_amd/csrc/blob_host.cc -- forst_blob_walk_file: the structure walk of
// forst_blob_verify_files (blob_host.h) over one blob file, as a host utility
// of its own.  No HIP call: it can be built and tested alone.
#include "blob_host.h"

extern "C" __attribute__((visibility("default"))) int forst_blob_walk_file(
    const uint8_t* file, uint64_t file_size, const uint32_t* expect_cf_id,
    uint64_t* record_offsets, uint64_t capacity, uint64_t* n_records, int* tail_crosses,
    forst_blob_file_result* out) {
  if (!out || (file_size && !file)) return FORST_EINVAL;
  uint64_t n = 0;
  const forst::blobhost::Walk w =
      forst::blobhost::walk_file(file, file_size, expect_cf_id, out, [&](uint64_t off) {
        if (record_offsets && n < capacity) record_offsets[n] = off;
        ++n;
      });
  if (n_records) *n_records = w.n_records;
  if (tail_crosses) *tail_crosses = w.tail_crosses ? 1 : 0;
  return FORST_OK;
}
