// tests/cpp/blob_shim_selftest.cc -- forst_gpu::BlobRecords (include/forst/
// checksum_engine.h) the way a ForSt call site would use it, on a real MI355X,
// over one reference-written blob file (argv[1], tests/golden/blob/) and a
// damaged copy of it: VerifyRecords' Status texts (MultiGetBlob's verify
// loop), IsValidBlobOffset's edge cases, FillRecordCrcs regenerating the file
// byte for byte, VerifyFiles.  Prints PASS or FAIL lines; exit code 0 iff all
// passed.
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

static uint64_t le64(const uint8_t* p) {
  uint64_t v;
  std::memcpy(&v, p, 8);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) return 2;
  std::vector<uint8_t> file(1 << 20);
  file.resize(std::fread(file.data(), 1, file.size(), fh));
  std::fclose(fh);
  const uint64_t size = file.size();

  // the records, by the host walk
  std::vector<uint64_t> offs(size / 32);
  uint64_t n = 0;
  int tail = 0;
  forst_blob_file_result walk;
  CHECK(forst_blob_walk_file(file.data(), size, nullptr, offs.data(), offs.size(), &n, &tail,
                             &walk) == FORST_OK);
  CHECK(walk.reason == FORST_BLOB_FILE_OK && n >= 4 && !tail);
  offs.resize(n);

  uint8_t* d = nullptr;
  CHECK(hipMalloc(&d, 2 * size + 64) == hipSuccess);
  CHECK(hipMemcpy(d, file.data(), size, hipMemcpyHostToDevice) == hipSuccess);

  BlobRecords blobs;
  // every record as MultiGetBlob would ask for it, in reverse file order
  std::vector<BlobRequest> reqs;
  for (uint64_t i = n; i-- > 0;) {
    const uint64_t ks = le64(&file[offs[i]]), vs = le64(&file[offs[i] + 8]);
    BlobRequest r;
    r.user_key = reinterpret_cast<const char*>(&file[offs[i] + 32]);
    r.user_key_size = ks;
    r.offset = offs[i] + 32 + ks;
    r.value_size = vs;
    reqs.push_back(r);
  }
  std::vector<Status> st;
  CHECK(blobs.VerifyRecords(d, size, reqs, &st).ok() && st.size() == n);
  for (const Status& s : st) CHECK(s.ok());

  // wrong key of the right length, wrong key size, wrong value size, and
  // IsValidBlobOffset's two edges (blob_log_format.h:150-162)
  const BlobRequest good = reqs[1];
  std::string wrong(good.user_key, good.user_key_size);
  wrong[0] ^= 0x20;
  std::string longer(good.user_key, good.user_key_size);
  longer += 'x';
  std::vector<BlobRequest> bad(6, good);
  bad[0].user_key = wrong.data();
  bad[1].user_key = longer.data();  // (the offset moves with the key size: same record start)
  bad[1].user_key_size = longer.size();
  bad[1].offset = good.offset + 1;
  bad[1].value_size = good.value_size - 1;
  bad[2].value_size = good.value_size - 1;
  bad[3].offset = 30 + 32 + good.user_key_size - 1;  // below the first possible value
  bad[4].value_size = size - 32 - good.offset + 1;   // the value would reach into the footer
  bad[5].offset = 30 + 32 + good.user_key_size;      // the lowest valid offset: not a record here
  CHECK(good.value_size > 1);
  CHECK(blobs.VerifyRecords(d, size, bad, &st).ok() && st.size() == 6);
  CHECK(st[0].ToString() == "Corruption: Key mismatch when reading blob");
  CHECK(st[1].ToString() == "Corruption: Key size mismatch when reading blob");
  CHECK(st[2].ToString() == "Corruption: Value size mismatch when reading blob");
  CHECK(st[3].ToString() == "Corruption: Invalid blob offset");
  CHECK(st[4].ToString() == "Corruption: Invalid blob offset");
  CHECK(st[5].ToString() != "Corruption: Invalid blob offset" && !st[5].ok());
  CHECK(!BlobRecords::IsValidBlobOffset(61 + 4, 4, 0, 1000) &&
        BlobRecords::IsValidBlobOffset(62 + 4, 4, 0, 1000) &&
        BlobRecords::IsValidBlobOffset(100, 4, 868, 1000) &&
        !BlobRecords::IsValidBlobOffset(100, 4, 869, 1000));

  // a damaged copy behind the file in the same arena: a value byte of record
  // 2, a header byte of record 3
  const uint64_t at2 = (size + 7) & ~uint64_t(7);
  std::vector<uint8_t> dam = file;
  const uint64_t ks2 = le64(&file[offs[2]]), vs2 = le64(&file[offs[2] + 8]);
  CHECK(vs2 > 0);
  dam[offs[2] + 32 + ks2 + vs2 / 2] ^= 0x04;
  CHECK(hipMemcpy(d + at2, dam.data(), size, hipMemcpyHostToDevice) == hipSuccess);
  std::vector<BlobRequest> two = {reqs[n - 1 - 2], reqs[n - 1 - 3]};
  CHECK(blobs.VerifyRecords(d + at2, size, two, &st).ok());
  CHECK(st[0].ToString() == "Corruption: Blob CRC mismatch" && st[1].ok());

  std::vector<BlobFileRef> refs(2);
  refs[0].host_file = file.data();
  refs[1].host_file = dam.data();
  refs[0].file_size = refs[1].file_size = size;
  refs[1].dev_offset = at2;
  refs[0].column_family_id = refs[1].column_family_id = walk.column_family_id;
  std::vector<forst_blob_file_result> res;
  std::vector<Status> fs = blobs.VerifyFiles(refs, d, at2 + size, &res);
  CHECK(fs.size() == 2 && fs[0].ok() && res[0].blob_count == n);
  CHECK(fs[1].ToString() == "Corruption: Blob CRC mismatch" && res[1].fail_index == 2 &&
        res[1].fail_offset == offs[2]);
  refs[0].column_family_id += 1;
  fs = blobs.VerifyFiles(refs, d, at2 + size);
  CHECK(fs[0].ToString() == "Corruption: Column family ID mismatch");
  dam[offs[3] + 9] ^= 0x01;
  CHECK(hipMemcpy(d + at2, dam.data(), size, hipMemcpyHostToDevice) == hipSuccess);
  CHECK(blobs.VerifyRecords(d + at2, size, two, &st).ok());
  CHECK(st[1].ToString() == "Corruption: Error while decoding blob record: Header CRC mismatch");

  // BlobLogWriter::EmitPhysicalRecord with the CRCs deferred: the image with
  // empty CRC fields comes back as the reference wrote it
  std::vector<uint8_t> img = file;
  for (uint64_t o : offs) std::memset(&img[o + 24], 0, 8);
  CHECK(hipMemcpy(d, img.data(), size, hipMemcpyHostToDevice) == hipSuccess);
  std::vector<uint8_t> codes;
  CHECK(blobs.FillRecordCrcs(d, size, offs, &codes).ok() && codes.size() == n);
  for (uint8_t c : codes) CHECK(c == FORST_BLOB_OK);
  CHECK(hipMemcpy(img.data(), d, size, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(img == file);
  std::vector<uint64_t> past = {size - 16, offs[0]};
  CHECK(blobs.FillRecordCrcs(d, size, past, &codes).ok());
  CHECK(codes[0] == FORST_BLOB_OUT_OF_RANGE && codes[1] == FORST_BLOB_OK);

  CHECK(BlobRecords::RecordStatus(FORST_BLOB_OK).ok());
  CHECK(BlobRecords::RecordStatus(FORST_BLOB_KEY).IsCorruption());
  CHECK(BlobRecords::RecordStatus(FORST_BLOB_OUT_OF_RANGE).code() == Status::kInvalidArgument);
  CHECK(BlobRecords::RecordStatus(FORST_BLOB_TOO_LARGE).code() == Status::kInvalidArgument);
  (void)hipFree(d);
  std::printf(g_fail ? "FAILED %d\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
