// forst_amd/csrc/blob.h -- blob file records (db/blob/blob_log_format.h), the
// other CRC32C record format beside the WAL; compiled into wal.hip.
//
// A record is a 32-byte header [key_size:8 value_size:8 expiration:8
// header_crc:4 blob_crc:4] followed by key and value (blob_log_format.h:96-116):
// header_crc = Mask(Value(header[0..24))), blob_crc = Mask(Value(key || value))
// (BlobLogRecord::EncodeHeaderTo, blob_log_format.cc:96-110).  Records start at
// any byte.  The pipeline on one stream, nothing read back:
//
//   decode  one LANE per record: the 32 header bytes, the header CRC in the
//           lane (slicing-by-4 over a 4 x 256 table in LDS: 6 steps), the
//           checks of the mode in the reference's order, one raw-CRC
//           descriptor (record + 32, key_size + value_size) and, verify mode,
//           the unmasked stored blob_crc as the raw kernel's expect / pre-fill
//   key     verify mode with user keys: record.key != user_key
//           (blob_file_reader.cc:562), one lane per record
//   crc     the CRC32C rows / lane kernels in raw mode over the descriptors
//   status  the final status per record, the mismatch counter, the computed CRCs
//   store   write mode: both CRC fields in place, a pass of its own (in-loop
//           header stores measured slower for the WAL writer)
//
// A record that is not hashed gets the descriptor (0, 0) with expect 0: the
// raw launch computes Value("", 0) = 0 for it and stores nothing; its status
// says why.  Validity is never read from a size: key_size + value_size == 0 is
// a legal record.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "crc32c_tables.h"
#include "crc_lds.h"
#include "device_common.h"
#include "engine.h"

namespace forst {

namespace {

constexpr uint32_t kBlobThreads = 256;
constexpr uint32_t kBlobHdr = 32;  // BlobLogRecord::kHeaderSize

struct BlobScratch {
  uint64_t* d_off;     // [t] raw descriptors
  uint32_t* d_len;     // [t]
  uint32_t* computed;  // [t] raw CRCs (pre-filled with stored, verify mode)
  uint32_t* stored;    // [t] unmasked stored CRC (verify mode)
  uint32_t* hcrc;      // [n] masked computed header CRC
  uint8_t* st;         // [t] status before the blob CRC compare
};

// 32 bytes at any alignment: dword-aligned 16-byte loads (as load_wal_header)
// when the 36 bytes from the dword below pos lie inside the buffer, byte loads
// otherwise.  The caller has checked pos + 32 <= len.
__device__ __forceinline__ void blob_load32(const uint8_t* base, uint64_t len, uint64_t pos,
                                            uint32_t (&w)[8]) {
  const uint64_t q = pos & ~3ull;
  if (q + 36 <= len) {
    const uint8_t* p = base + q + vzero();
    const u32x4a4 a = ld16_a4(p), b = ld16_a4(p + 16);
    const uint32_t t = ld4_a4(p + 32);
    const uint32_t o = static_cast<uint32_t>(pos & 3);
    w[0] = __builtin_amdgcn_alignbyte(a.y, a.x, o);
    w[1] = __builtin_amdgcn_alignbyte(a.z, a.y, o);
    w[2] = __builtin_amdgcn_alignbyte(a.w, a.z, o);
    w[3] = __builtin_amdgcn_alignbyte(b.x, a.w, o);
    w[4] = __builtin_amdgcn_alignbyte(b.y, b.x, o);
    w[5] = __builtin_amdgcn_alignbyte(b.z, b.y, o);
    w[6] = __builtin_amdgcn_alignbyte(b.w, b.z, o);
    w[7] = __builtin_amdgcn_alignbyte(t, b.w, o);
  } else {
    const uint8_t* p = base + pos;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      w[k] = static_cast<uint32_t>(p[4 * k]) | (static_cast<uint32_t>(p[4 * k + 1]) << 8) |
             (static_cast<uint32_t>(p[4 * k + 2]) << 16) |
             (static_cast<uint32_t>(p[4 * k + 3]) << 24);
  }
}

// the workgroup's unreplicated slicing-by-4 table (kCrcG: 4 x 256 dwords)
__device__ __forceinline__ void blob_fill_table(uint32_t* L) {
  for (uint32_t i = threadIdx.x; i < 1024; i += kBlobThreads) L[i] = kCrcG[i];
  __syncthreads();
}

// Mask(Value(w[0..nw))) of whole dwords
template <int NW>
__device__ __forceinline__ uint32_t blob_crc_words(const uint32_t* L, const uint32_t* w) {
  const uint8_t* Lb = reinterpret_cast<const uint8_t*>(L);
  uint32_t s = 0xffffffffu;
#pragma unroll
  for (int k = 0; k < NW; ++k) s = fcrc::shift_at(Lb, 0, s ^ w[k]);
  return crc_mask(~s);
}

__global__ void __launch_bounds__(kBlobThreads) blob_decode_kernel(BlobArgs a, BlobScratch s) {
  __shared__ uint32_t L[1024];
  blob_fill_table(L);
  const uint64_t total = a.n + a.n_footers;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlobThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlobThreads + threadIdx.x; i < total;
       i += stride) {
    const bool footer = i >= a.n;
    const uint64_t off = footer ? a.footer_offsets[i - a.n] : a.record_offsets[i];
    uint32_t st = FORST_BLOB_OK, hcrc = 0, stored = 0, d_len = 0;
    uint64_t d_off = 0;
    if (off > a.base_len || a.base_len - off < kBlobHdr) {
      st = FORST_BLOB_OUT_OF_RANGE;  // reported, never read
    } else {
      uint32_t w[8];
      blob_load32(a.base, a.base_len, off, w);
      if (footer) {  // BlobLogFooter::DecodeFrom: Value(footer[0..28)) vs the LE32 behind
        d_off = off;
        d_len = 28;
        stored = crc_unmask(w[7]);
      } else {
        const uint64_t ks = (static_cast<uint64_t>(w[1]) << 32) | w[0];
        const uint64_t vs = (static_cast<uint64_t>(w[3]) << 32) | w[2];
        hcrc = blob_crc_words<6>(L, w);
        if (!a.write) {  // DecodeHeaderFrom, then VerifyBlob's size checks
          if (hcrc != w[6])
            st = FORST_BLOB_HEADER_CRC;
          else if (a.expect_key_sizes && ks != a.expect_key_sizes[i])
            st = FORST_BLOB_KEY_SIZE;
          else if (a.expect_value_sizes && vs != a.expect_value_sizes[i])
            st = FORST_BLOB_VALUE_SIZE;
        }
        if (st == FORST_BLOB_OK) {
          const uint64_t sum = ks + vs;
          if (sum < ks || sum > 0xffffffffull)
            st = FORST_BLOB_TOO_LARGE;
          else if (sum > a.base_len - off - kBlobHdr)
            st = FORST_BLOB_OUT_OF_RANGE;
          else {
            d_off = off + kBlobHdr;
            d_len = static_cast<uint32_t>(sum);
            stored = crc_unmask(w[7]);
          }
        }
      }
    }
    if (st != FORST_BLOB_OK) stored = 0;
    s.d_off[i] = d_off;
    s.d_len[i] = d_len;
    s.st[i] = static_cast<uint8_t>(st);
    if (!footer) s.hcrc[i] = hcrc;
    if (!a.write) {
      s.stored[i] = stored;
      s.computed[i] = stored;  // the raw kernel stores only where the CRC differs
    }
  }
}

// record.key != user_key over the records that passed the size checks (their
// key lies inside the buffer: the payload was range-checked).  A user key
// outside [0, user_keys_len) is a mismatch, never read.
__global__ void __launch_bounds__(kBlobThreads) blob_key_kernel(BlobArgs a, BlobScratch s) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlobThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlobThreads + threadIdx.x; i < a.n;
       i += stride) {
    if (s.st[i] != FORST_BLOB_OK) continue;
    const uint64_t ks = a.expect_key_sizes[i], uo = a.user_key_offsets[i];
    bool same = uo <= a.user_keys_len && ks <= a.user_keys_len - uo;
    if (same) {
      const uint8_t* k = a.base + a.record_offsets[i] + kBlobHdr;
      const uint8_t* u = a.user_keys + uo;
      for (uint64_t j = 0; j < ks && same; ++j) same = k[j] == u[j];
    }
    if (!same) s.st[i] = FORST_BLOB_KEY;
  }
}

__global__ void __launch_bounds__(kBlobThreads) blob_status_kernel(BlobArgs a, BlobScratch s) {
  const uint64_t total = a.n + a.n_footers;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlobThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlobThreads + threadIdx.x; i < total;
       i += stride) {
    uint32_t st = s.st[i];
    // the payload was hashed unless a check before the key compare failed
    const bool hashed = st == FORST_BLOB_OK || st == FORST_BLOB_KEY;
    const uint32_t c = s.computed[i];
    if (!a.write && st == FORST_BLOB_OK && c != s.stored[i]) st = FORST_BLOB_CRC;
    a.status[i] = static_cast<uint8_t>(st);
    if (i < a.n) {
      if (a.header_crc) a.header_crc[i] = s.hcrc[i];
      if (a.blob_crc) a.blob_crc[i] = hashed ? crc_mask(c) : 0u;
    }
    if (a.mismatches && st != FORST_BLOB_OK) atomicAdd(a.mismatches, 1ull);
  }
}

// write mode: header_crc at record + 24, blob_crc at record + 28 (LE32)
__global__ void __launch_bounds__(kBlobThreads) blob_store_kernel(BlobArgs a, BlobScratch s) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlobThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlobThreads + threadIdx.x; i < a.n;
       i += stride) {
    if (s.st[i] != FORST_BLOB_OK) continue;
    uint8_t* p = a.base_w + a.record_offsets[i];
    st_le32(p + 24, s.hcrc[i]);
    st_le32(p + 28, crc_mask(s.computed[i]));
  }
}

}  // namespace

hipError_t launch_blob_records(const BlobArgs& a, hipStream_t stream, const char** name) {
  const uint64_t total = a.n + a.n_footers;
  if (total == 0) return hipSuccess;
  const auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t s8 = up(8 * total), s4 = up(4 * total), s1 = up(total);
  void* scratch = nullptr;
  hipError_t e = scratch_alloc(&scratch, s8 + 4 * s4 + s1, stream);
  if (e != hipSuccess) return e;
  uint8_t* p = static_cast<uint8_t*>(scratch);
  BlobScratch s{};
  s.d_off = reinterpret_cast<uint64_t*>(p);
  s.d_len = reinterpret_cast<uint32_t*>(p + s8);
  s.computed = reinterpret_cast<uint32_t*>(p + s8 + s4);
  s.stored = reinterpret_cast<uint32_t*>(p + s8 + 2 * s4);
  s.hcrc = reinterpret_cast<uint32_t*>(p + s8 + 3 * s4);
  s.st = p + s8 + 4 * s4;
  const dim3 grid(static_cast<uint32_t>(
      std::min<uint64_t>((total + kBlobThreads - 1) / kBlobThreads, 16384)));
  hipLaunchKernelGGL(blob_decode_kernel, grid, dim3(kBlobThreads), 0, stream, a, s);
  *name = "blob_decode_kernel";
  if (!a.write && a.user_keys && a.n)
    hipLaunchKernelGGL(blob_key_kernel, grid, dim3(kBlobThreads), 0, stream, a, s);
  e = hipGetLastError();
  // (a buffer too short for one header holds no record to hash)
  if (e == hipSuccess && a.base_len >= kBlobHdr) {
    // any order of the offsets: the raw launch's global feed deals descriptors
    // by index, and the small-batch kernel's byte ranges (stream_common.h
    // wg_range) tile [0, n) whatever the order (only their balance needs file
    // order)
    BlockArgs b{};
    b.base = a.base;
    b.base_len = a.base_len;
    b.offsets = s.d_off;
    b.sizes = s.d_len;
    b.out32 = s.computed;
    b.n = total;
    b.expect = a.write ? nullptr : s.stored;
    e = launch_crc32c_blocks(kModeRaw, b, stream, name);
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(blob_status_kernel, grid, dim3(kBlobThreads), 0, stream, a, s);
    if (a.write && a.n)
      hipLaunchKernelGGL(blob_store_kernel, grid, dim3(kBlobThreads), 0, stream, a, s);
    e = hipGetLastError();
  }
  const hipError_t f = scratch_free(scratch, stream);
  return e != hipSuccess ? e : f;
}

}  // namespace forst
