// forst_amd/csrc/wal_compact.h -- forst_wal_records_compact: the bytes
// log::Reader::ReadRecord returns for each recovered WAL record (its `record`
// Slice / scratch, db/log_reader.cc:95-213), back to back in a device arena,
// as contiguous reps for forst_write_batch_protect_batch / forst_xxh3_64_batch
// (DESIGN.md §4.11).  Compiled into wal.hip.
//
// Phase 1, wc_walk_kernel: one lane per record follows the physical records
// from the record's LastRecordOffset exactly as WalRecovery::Next does on the
// host (wal_shim.cc): block tails shorter than a header and a recyclable
// writer's 7..10-byte zero tail are skipped, control records (types 9-11) are
// stepped over uncounted, n_fragments data fragments are taken with the
// header size of their type byte, and their payloads must add up to the
// record's length.  It writes the status and size and classifies the record:
// REGULAR = laid out the way log::Writer::AddRecord writes it
// (db/log_writer.cc:65-160: every fragment but the last fills its block, the
// next starts right behind the next block's header, one header size, nothing
// in between, no fragment reaching past its block's end); anything else is
// irregular and goes on a list.  One scan of the rounded sizes
// (scan_common.h) gives the rep offsets.
//
// Phase 2, wc_copy_kernel: the arena is a flat run of 16-byte destination
// pieces, and the work is dealt by DESTINATION bytes: a workgroup owns a
// contiguous range of 16 KiB tiles, a tile is 1024 pieces, piece t + 256 k of
// it belongs to thread t -- so every wave store is 1 KiB of whole lines
// whatever the record lengths are, a 32-byte record costs two lanes, and a
// 1 GiB record is spread over every workgroup.  The record of a piece is
// found in a window of the rep offsets held in LDS (the workgroup's cursor
// moves forward with its tiles; one binary search in global memory per
// workgroup finds where it starts).  For a regular record the physical address
// of logical byte x is arithmetic from the first payload offset and the block
// geometry (as FragGeo in xxh3.hip), so no fragment list exists: a piece is a
// dword-aligned 16-byte load plus the dword behind it, realigned with
// v_alignbyte (byte loads for the few pieces whose 20-byte read would reach
// log_len); the one piece per block that straddles a header hole is
// assembled from both sides.  A thread issues the loads of its four pieces
// before the first store (stores share vmcnt with loads).
//
// Irregular records (crafted logs -- a fragment whose length field runs past
// its block's end among them, which the host walk copies contiguously --, a
// control record or a skipped tail inside a record, mixed header sizes) are
// copied per fragment by
// wc_irregular_kernel, one workgroup per record, byte by byte: it reads no
// byte outside a payload.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_common.h"
#include "engine.h"
#include "scan_common.h"
#include "wal_hash.h"

namespace forst {
namespace {

constexpr uint32_t kWcLanes = 256;
constexpr uint32_t kWcPiece = 16;                          // bytes per destination store
constexpr uint32_t kWcPer = 4;                             // pieces per thread and tile
constexpr uint32_t kWcTilePieces = kWcLanes * kWcPer;      // 1024
constexpr uint32_t kWcTile = kWcTilePieces * kWcPiece;     // 16 KiB of arena
constexpr uint32_t kWcWin = 1024;                          // LDS window (records), 1023 searched
constexpr uint32_t kWcRegular = 0x100;  // WcMeta::info: hs | kWcRegular

struct alignas(16) WcMeta {
  uint64_t p0;    // log offset of the first payload byte (first non-empty fragment)
  uint32_t size;  // record length, 0 when status != 0
  uint32_t info;  // header size | kWcRegular
};

struct WcFrag {
  uint64_t pay;  // log offset of the payload
  uint32_t hs, len;
};

// log_format.h:20-41
__device__ __forceinline__ bool wc_recyclable_type(uint32_t t) {
  return (t >= 5 && t <= 8) || t == 11;
}

// The next data fragment at or behind *p (WalRecovery::Next's inner loop);
// false: the walk leaves the log or meets a type that is neither data nor
// control.  Reads nothing at or past log_len.
__device__ __forceinline__ bool wc_next_fragment(const uint8_t* log, uint64_t log_len, uint64_t* p,
                                                 WcFrag* f) {
  for (;;) {
    if (*p > log_len) return false;
    const uint64_t left = kWhBlock - (*p & (kWhBlock - 1));
    if (left < 7) {  // a block tail the writer padded
      *p += left;
      continue;
    }
    if (log_len - *p < 7) return false;
    const WalHdr h = load_wal_header(log, log_len, *p);
    if (h.length == 0 && h.type == 0 && left < 11) {  // a recyclable writer's 7..10-byte zero tail
      *p += left;
      continue;
    }
    const uint32_t hs = wc_recyclable_type(h.type) ? 11u : 7u;
    if (log_len - *p < static_cast<uint64_t>(hs) + h.length) return false;
    if (h.type >= 9 && h.type <= 11) {  // a control record: in no record's bytes, not counted
      *p += hs + h.length;
      continue;
    }
    if (h.type == 0 || h.type > 11) return false;
    f->pay = *p + hs;
    f->hs = hs;
    f->len = h.length;
    *p += hs + h.length;
    return true;
  }
}

__global__ void __launch_bounds__(kWcLanes) wc_walk_kernel(
    const uint8_t* log, uint64_t log_len, const uint64_t* rec_offset, const uint64_t* rec_length,
    const uint32_t* rec_nfrag, uint64_t n, WcMeta* meta, uint64_t* rounded, uint32_t* rep_sizes,
    uint8_t* status, uint64_t* list, unsigned long long* n_irregular) {
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kWcLanes + threadIdx.x;
  if (j >= n) return;
  const uint64_t want = rec_length[j];
  const uint32_t nf = rec_nfrag[j];
  uint32_t st = 0;
  bool regular = true;
  uint64_t p0 = 0, prev_end = 0, got = 0;
  uint32_t hs0 = 0, nz = 0;
  if (want > 0xffffffffull) {
    st = 2;
  } else {
    uint64_t p = rec_offset[j];
    for (uint32_t q = 0; q < nf; ++q) {
      WcFrag f;
      if (!wc_next_fragment(log, log_len, &p, &f)) {
        st = 1;
        break;
      }
      got += f.len;
      if (got > want) {  // (also ends the walk of an absurd n_fragments early)
        st = 1;
        break;
      }
      const uint64_t h = f.pay - f.hs;
      if (q > 0 && (h != prev_end || (h & (kWhBlock - 1)) != 0)) regular = false;
      if (q + 1 < nf && ((f.pay + f.len) & (kWhBlock - 1)) != 0) regular = false;
      if (q == 0) hs0 = f.hs;
      if (f.hs != hs0) regular = false;
      // a payload that runs past its block's end (no writer's, but the host
      // walk takes it as it lies): the header-hole arithmetic does not hold
      if ((h & (kWhBlock - 1)) + f.hs + f.len > kWhBlock) regular = false;
      if (f.len && !nz++) p0 = f.pay;
      prev_end = f.pay + f.len;
    }
    if (st == 0 && got != want) st = 1;
  }
  const uint32_t size = st ? 0u : static_cast<uint32_t>(want);
  WcMeta m;
  m.p0 = p0;
  m.size = size;
  m.info = hs0 | (regular ? kWcRegular : 0u);
  meta[j] = m;
  rounded[j] = (static_cast<uint64_t>(size) + (kWcPiece - 1)) & ~static_cast<uint64_t>(kWcPiece - 1);
  if (rep_sizes) rep_sizes[j] = size;
  if (status) status[j] = static_cast<uint8_t>(st);
  if (size && !regular) list[atomicAdd(n_irregular, 1ull)] = j;
}

// 16 bytes at any byte offset pos < log_len of the log: reads [pos & ~3, +20),
// or, where that would reach past log_len, the bytes in front of log_len one
// by one (zero behind them)
__device__ __forceinline__ u32x4 wc_load16(const uint8_t* log, uint64_t log_len, uint64_t pos) {
  const uint32_t m = static_cast<uint32_t>(pos & 3);
  if (pos - m + 20 > log_len) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (uint32_t k = 0; k < 16 && pos + k < log_len; ++k)
      w[k >> 2] |= static_cast<uint32_t>(log[pos + k]) << (8 * (k & 3));
    // (retire: the byte loads are waited for here, not behind the join, where
    // the wait would drain the hot path's loads in flight)
    return u32x4{retire(w[0]), retire(w[1]), retire(w[2]), retire(w[3])};
  }
  const uint8_t* q = log + (pos - m);
  const u32x4a4 v = ld16_a4(q);
  const uint32_t nx = ld4_a4(q + 16);
  return u32x4{__builtin_amdgcn_alignbyte(v.y, v.x, m), __builtin_amdgcn_alignbyte(v.z, v.y, m),
               __builtin_amdgcn_alignbyte(v.w, v.z, m), __builtin_amdgcn_alignbyte(nx, v.w, m)};
}

// dword d's mask of the bytes k (of 16) with k < c
__device__ __forceinline__ uint32_t wc_below(uint32_t c, uint32_t d) {
  const int32_t r = static_cast<int32_t>(c) - static_cast<int32_t>(4 * d);
  return r <= 0 ? 0u : r >= 4 ? 0xffffffffu : (1u << (8 * r)) - 1u;
}

// bytes [lb, lb + 16) of a regular record, zero at and past its end
__device__ __forceinline__ u32x4 wc_piece(const uint8_t* log, uint64_t log_len, const WcMeta& m,
                                          uint32_t lb) {
  const uint32_t hs = m.info & 0xffu;
  const uint32_t r0 = kWhBlock - static_cast<uint32_t>(m.p0 & (kWhBlock - 1));
  uint64_t pos;
  uint32_t n1;  // bytes from pos to its block's end
  if (lb < r0) {
    pos = m.p0 + lb;
    n1 = r0 - lb;
  } else {
    const uint32_t y = lb - r0, per = kWhBlock - hs;
    const uint32_t q = hs == 7 ? y / (kWhBlock - 7) : y / (kWhBlock - 11);
    const uint32_t rem = y - q * per;
    pos = m.p0 + r0 + static_cast<uint64_t>(q) * kWhBlock + hs + rem;
    n1 = per - rem;
  }
  const uint32_t valid = m.size - lb;  // >= 1
  u32x4 v = wc_load16(log, log_len, pos);
  if (n1 < kWcPiece && n1 < valid) {
    // the piece straddles a header hole: bytes n1.. lie behind the next
    // block's header; loaded as the 16 bytes that END with them
    const u32x4 w = wc_load16(log, log_len, pos + hs);
    v.x = (v.x & wc_below(n1, 0)) | (w.x & ~wc_below(n1, 0));
    v.y = (v.y & wc_below(n1, 1)) | (w.y & ~wc_below(n1, 1));
    v.z = (v.z & wc_below(n1, 2)) | (w.z & ~wc_below(n1, 2));
    v.w = (v.w & wc_below(n1, 3)) | (w.w & ~wc_below(n1, 3));
  }
  if (valid < kWcPiece) {
    v.x &= wc_below(valid, 0);
    v.y &= wc_below(valid, 1);
    v.z &= wc_below(valid, 2);
    v.w &= wc_below(valid, 3);
  }
  return v;
}

// how many of win[0 .. 1023) are <= x (win ascending)
__device__ __forceinline__ uint32_t wc_count_le(const uint32_t* win, uint32_t x) {
  uint32_t lo = 0;
#pragma unroll
  for (uint32_t step = 512; step; step >>= 1)
    if (lo + step <= kWcWin - 1 && win[lo + step - 1] <= x) lo += step;
  return lo;
}

// Workgroup b copies the arena range [b * range, min((b + 1) * range, total))
// (range a multiple of kWcTile); the pieces of irregular records are left to
// wc_irregular_kernel.
__global__ void __launch_bounds__(kWcLanes) wc_copy_kernel(const uint8_t* log, uint64_t log_len,
                                                           const WcMeta* meta,
                                                           const uint64_t* rep_off, uint64_t n,
                                                           uint64_t total, uint64_t range,
                                                           uint8_t* arena) {
  __shared__ uint32_t win[kWcWin];
  const uint32_t t = threadIdx.x;
  const uint64_t begin = static_cast<uint64_t>(blockIdx.x) * range;
  const uint64_t end = begin + range < total ? begin + range : total;
  // the last record whose offset is <= begin (with equal offsets -- empty
  // records -- the last one is the record that has the bytes)
  uint64_t cur = 0;
  {
    uint64_t lo = 0, hi = n;  // off[lo] <= begin < off[hi]
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (rep_off[mid] <= begin) lo = mid; else hi = mid;
    }
    cur = lo;
  }
  for (uint64_t tile = begin; tile < end; tile += kWcTile) {
    const uint32_t tile_n = static_cast<uint32_t>(end - tile < kWcTile ? end - tile : kWcTile);
    uint32_t done = 0;
    for (;;) {
      __syncthreads();
#pragma unroll
      for (uint32_t k = 0; k < kWcPer; ++k) {
        const uint32_t e = t + k * kWcLanes;
        const uint64_t j = cur + e;
        uint32_t rel = 0xffffffffu;
        if (j < n) {
          const uint64_t o = rep_off[j];
          rel = o <= tile ? 0u : o - tile >= 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(o - tile);
        }
        win[e] = rel;
      }
      __syncthreads();
      u32x4 v[kWcPer];
      uint32_t store = 0;
#pragma unroll
      for (uint32_t k = 0; k < kWcPer; ++k) {
        const uint32_t x = (t + k * kWcLanes) * kWcPiece;
        v[k] = u32x4{0u, 0u, 0u, 0u};
        if (x < tile_n && !((done >> k) & 1u)) {
          const uint32_t c = wc_count_le(win, x);
          if (c < kWcWin - 1) {  // resolved inside the window (c >= 1: off[cur] <= tile)
            done |= 1u << k;
            const uint64_t j = cur + c - 1;
            const WcMeta m = meta[j];
            if (m.info & kWcRegular) {
              v[k] = wc_piece(log, log_len, m, static_cast<uint32_t>(tile + x - rep_off[j]));
              store |= 1u << k;
            }
          }
        }
      }
#pragma unroll
      for (uint32_t k = 0; k < kWcPer; ++k)
        if ((store >> k) & 1u)
          *reinterpret_cast<u32x4*>(arena + tile + (t + k * kWcLanes) * kWcPiece) = v[k];
      const uint32_t c_last = wc_count_le(win, tile_n - kWcPiece);
      if (c_last < kWcWin - 1) {  // the window reached the tile's end
        cur += c_last - 1;
        break;
      }
      cur += kWcWin - 2;  // off[cur + 1022] <= the tile's last piece
    }
  }
}

// one workgroup per irregular record: the payload bytes of its fragments and
// the zero padding behind them
__global__ void __launch_bounds__(kWcLanes) wc_irregular_kernel(
    const uint8_t* log, uint64_t log_len, const uint64_t* rec_offset, const uint32_t* rec_nfrag,
    const WcMeta* meta, const uint64_t* rep_off, const uint64_t* list, uint64_t n_list,
    uint8_t* arena) {
  for (uint64_t i = blockIdx.x; i < n_list; i += gridDim.x) {
    const uint64_t j = list[i];
    uint8_t* d = arena + rep_off[j];
    const uint32_t size = meta[j].size, nf = rec_nfrag[j];
    uint64_t p = rec_offset[j];
    uint32_t put = 0;
    for (uint32_t q = 0; q < nf; ++q) {
      WcFrag f;
      if (!wc_next_fragment(log, log_len, &p, &f) || f.len > size - put) break;  // (walked before)
      const uint8_t* src = log + f.pay;
      for (uint32_t x = threadIdx.x; x < f.len; x += kWcLanes) d[put + x] = src[x];
      put += f.len;
    }
    const uint32_t pad = (kWcPiece - (size & (kWcPiece - 1))) & (kWcPiece - 1);
    if (threadIdx.x < pad) d[size + threadIdx.x] = 0;
  }
}

}  // namespace

// Synchronous: reads the arena total (and the irregular count) back into
// *total; fails with hipErrorInvalidValue when an arena is given and *total >
// a.capacity (nothing is then written to the arena).
hipError_t launch_wal_records_compact(const WcArgs& a, hipStream_t st, uint64_t* total,
                                      const char** name) {
  *total = 0;
  const uint64_t n = a.n;
  if (n == 0) return hipSuccess;
  *name = "wc_copy_kernel";
  const uint64_t nt = n / kScanTile + 2, ntl = (n + kScanTile - 1) / kScanTile;
  const size_t s16 = wh_up256(16 * n), s8 = wh_up256(8 * n), st8 = wh_up256(8 * nt);
  void* scratch = nullptr;
  hipError_t e = scratch_alloc(&scratch, s16 + 3 * s8 + st8 + 256, st);
  if (e != hipSuccess) return e;
  uint8_t* p = static_cast<uint8_t*>(scratch);
  WcMeta* meta = reinterpret_cast<WcMeta*>(p);
  uint64_t* rounded = reinterpret_cast<uint64_t*>(p + s16);
  uint64_t* off = a.rep_offsets ? a.rep_offsets : reinterpret_cast<uint64_t*>(p + s16 + s8);
  uint64_t* list = reinterpret_cast<uint64_t*>(p + s16 + 2 * s8);
  uint64_t* tiles = reinterpret_cast<uint64_t*>(p + s16 + 3 * s8);
  unsigned long long* n_irr = reinterpret_cast<unsigned long long*>(p + s16 + 3 * s8 + st8);
  uint64_t host[2] = {0, 0};  // arena bytes, irregular records
  if ((e = hipMemsetAsync(n_irr, 0, 8, st)) == hipSuccess) {
    hipLaunchKernelGGL(wc_walk_kernel, wh_grid(n), dim3(kWcLanes), 0, st, a.log, a.log_len,
                       a.rec_offset, a.rec_length, a.rec_nfrag, n, meta, rounded, a.rep_sizes,
                       a.status, list, n_irr);
    scan_u64(rounded, n, tiles, off, st);
    if ((e = hipGetLastError()) == hipSuccess &&
        (e = hipMemcpyAsync(&host[0], tiles + ntl, 8, hipMemcpyDeviceToHost, st)) == hipSuccess &&
        (e = hipMemcpyAsync(&host[1], n_irr, 8, hipMemcpyDeviceToHost, st)) == hipSuccess)
      e = hipStreamSynchronize(st);
  }
  if (e == hipSuccess) {
    *total = host[0];
    if (a.arena && host[0] > a.capacity) e = hipErrorInvalidValue;
  }
  if (e == hipSuccess && a.arena && host[0]) {
    // ranges of whole tiles, about 16 per CU (a range amortises its one
    // search in global memory; more, smaller ranges even out the tail)
    const uint64_t cus = device_info().num_cus > 0 ? device_info().num_cus : 1;
    uint64_t range = (host[0] + cus * 16 - 1) / (cus * 16);
    range = (range + kWcTile - 1) / kWcTile * kWcTile;
    while ((host[0] + range - 1) / range > 0x7fffffffull) range *= 2;
    const uint32_t grid = static_cast<uint32_t>((host[0] + range - 1) / range);
    hipLaunchKernelGGL(wc_copy_kernel, dim3(grid), dim3(kWcLanes), 0, st, a.log, a.log_len, meta,
                       off, n, host[0], range, a.arena);
    if (host[1]) {
      const uint32_t gi = static_cast<uint32_t>(host[1] < 65536 ? host[1] : 65536);
      hipLaunchKernelGGL(wc_irregular_kernel, dim3(gi), dim3(kWcLanes), 0, st, a.log, a.log_len,
                         a.rec_offset, a.rec_nfrag, meta, off, list, host[1], a.arena);
    }
    e = hipGetLastError();
  }
  const hipError_t f = scratch_free(scratch, st);
  return e != hipSuccess ? e : f;
}

}  // namespace forst
