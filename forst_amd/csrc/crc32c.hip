// forst_amd/csrc/crc32c.hip -- CRC32C block kernels for gfx950 (CDNA4).
//
// Replaces, per block, util/crc32c.cc:1133 crc32c::Extend (SSE4.2 crc32c_3way
// on the reference's x86 path).  No carry-less multiply exists on CDNA4, so
// CRC is table driven.  The file holds, in this order:
//  * the v1 engine (wave_crc32c, fill_tables), one wavefront per block, which
//    serves crc32c_block_kernel_simple: buffers shorter than one 4 KiB round;
//  * the rows kernels (crc32c_rows_kernel<MODE>, crc32c_rows_raw_small_kernel,
//    crc32c_rows_raw_filt_kernel), one block per 16-lane row: every other
//    batch, in every mode;
//  * crc32c_raw_lane_kernel, one message per lane: the short messages of a
//    raw batch;
//  * the launchers.  A batch of more descriptors than a rows launch indexes
//    (FORST_ROWS_MAX_DESCS, engine.h) is split into several launches.
// The rows and lane kernels' LDS table lookups (Lanes, look, g_then, step_k,
// shift_at, ...) are in crc_lds.h, shared with the fused WAL-recovery kernel
// of xxh3.hip; the tables themselves come from gen_tables.py.
//
// The v1 algorithm:
//  * A block's message is covered by R rounds of 4 KiB ending at a dword
//    boundary W_end <= end; lane l owns the 64-byte segment [64l, 64l+64) of
//    each round (4 x global_load_dwordx4 per lane).  Bytes in front of the
//    message inside round 0 are garbage: the lane holding the first message
//    dword resets its state there (injecting ~init, crc32c::Extend's
//    pre-inversion) and lanes entirely in front zero their state.
//  * Each lane runs a slicing-by-4 CRC over its segment with four 256-entry
//    tables replicated 32x in LDS (entry e of copy c at dword 32e + c, lane
//    l reads copy l&31) so every ds_read_b32 is bank-conflict free.
//  * Between rounds a lane jumps over the 4032 bytes owned by the other lanes
//    with one 4-lookup GF(2) shift (x^(8*4032) mod P).
//  * 6-level xor-butterfly over the wave combines the 64 lane states with
//    shifts x^(8*64*2^k) (the algebra of crc32c::Crc32cCombine,
//    util/crc32c.cc:1279); the <= 7 tail bytes after W_end (+ the block's
//    compression-type byte on the write side) are appended byte-wise.
// The combine constants are block-size independent, so mixed 4/16/64 KiB
// batches run in one launch.  See DESIGN.md for the roofline analysis.
#include "crc32c_tables.h"
#include "crc_lds.h"
#include "device_common.h"
#include "engine.h"
#include "stream_common.h"

namespace forst {
namespace {

constexpr uint32_t kRB = FORST_CRC_ROUND_BYTES;  // bytes per wave-round
constexpr uint32_t kWaves = 16;                  // waves per workgroup
constexpr uint32_t kThreads = kWaves * 64;
constexpr uint32_t kRep = 32;                     // table replication
constexpr uint32_t kOffJump = 4 * 256 * kRep;     // dword offsets in LDS
constexpr uint32_t kOffTree = kOffJump + 1024;
constexpr uint32_t kLdsDwords = kOffTree + FORST_CRC_TREE_LEVELS * 1024;
constexpr uint32_t kSmall = 32;  // shorter messages take the byte-serial path

static_assert(kLdsDwords * 4 <= 160 * 1024, "CRC tables must fit in LDS");

__device__ __forceinline__ uint32_t lds_at(const uint32_t* __restrict__ L,
                                           uint32_t byte_addr) {
  return L[byte_addr >> 2];
}

// slicing-by-4 step on the replicated tables: G(v) = v * x^32 mod P
__device__ __forceinline__ uint32_t crc_g(const uint32_t* __restrict__ L,
                                          uint32_t lb, uint32_t v) {
  const uint32_t a0 = ((v & 0xffu) << 7) + lb;
  const uint32_t a1 = (((v >> 8) & 0xffu) << 7) + lb;
  const uint32_t a2 = (((v >> 16) & 0xffu) << 7) + lb;
  const uint32_t a3 = ((v >> 24) << 7) + lb;
  return L[(a0 >> 2)] ^ L[(a1 >> 2) + 8192] ^ L[(a2 >> 2) + 16384] ^
         L[(a3 >> 2) + 24576];
}

// byte-at-a-time step (table G[3] is the Sarwate table)
__device__ __forceinline__ uint32_t crc_byte(const uint32_t* __restrict__ L,
                                             uint32_t lb, uint32_t s,
                                             uint32_t byte) {
  const uint32_t a = (((s ^ byte) & 0xffu) << 7) + lb;
  return L[(a >> 2) + 24576] ^ (s >> 8);
}

// linear shift x^(8n) through an unreplicated 4x256 table at dword T
__device__ __forceinline__ uint32_t crc_shift(const uint32_t* __restrict__ L,
                                              uint32_t T, uint32_t v) {
  return L[T + (v & 0xffu)] ^ L[T + 256 + ((v >> 8) & 0xffu)] ^
         L[T + 512 + ((v >> 16) & 0xffu)] ^ L[T + 768 + (v >> 24)];
}

__device__ __forceinline__ void load_seg(uint32_t (&w)[16],
                                         const uint8_t* seg) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const u32x4a4 v = ld16_a4(seg + 16 * k);
    w[4 * k + 0] = v.x;
    w[4 * k + 1] = v.y;
    w[4 * k + 2] = v.z;
    w[4 * k + 3] = v.w;
  }
}

// Round-0 load for windows that start before the caller's buffer: never
// touch a dword below `lo` (those lanes' data is garbage anyway).
__device__ __forceinline__ void load_seg_checked(uint32_t (&w)[16],
                                                 const uint8_t* seg,
                                                 uint64_t lo) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint8_t* c = seg + 16 * k;
    const uint64_t ca = reinterpret_cast<uint64_t>(c);
    if (ca >= lo) {
      const u32x4a4 v = ld16_a4(c);
      w[4 * k + 0] = v.x;
      w[4 * k + 1] = v.y;
      w[4 * k + 2] = v.z;
      w[4 * k + 3] = v.w;
    } else {
#pragma unroll
      for (int d = 0; d < 4; ++d)
        w[4 * k + d] = (ca + 4 * d >= lo) ? ld4_a4(c + 4 * d) : 0u;
    }
  }
}

// crc32c::Extend(init, p, len), then extended by `nextra` (0/1) extra byte.
// All arguments are wave-uniform; every lane returns the result.  Bytes in
// [lo, p) may be read (and ignored); nothing outside [lo, p+len) is touched.
__device__ __forceinline__ uint32_t wave_crc32c(const uint32_t* __restrict__ L,
                                                uint32_t lane,
                                uint32_t lb, const uint8_t* p, uint64_t len,
                                uint32_t init, uint32_t nextra, uint32_t extra,
                                uint64_t lo) {
  uint32_t s;
  if (len < kSmall) {
    s = ~init;
    for (uint32_t i = 0; i < static_cast<uint32_t>(len); ++i)
      s = crc_byte(L, lb, s, ldu8(p + i));
  } else {
    const uint64_t A = reinterpret_cast<uint64_t>(p);
    const uint64_t E = A + len;
    const uint64_t Aal = A & ~3ull;
    const uint32_t m = static_cast<uint32_t>(A & 3);
    uint64_t Wend = E & ~3ull;
    const uint64_t D = Wend - Aal;
    uint32_t R = static_cast<uint32_t>((D + kRB - 1) / kRB);
    if (R > 1 && (D % kRB) == 4) {  // spill 4 bytes into the tail, save a round
      Wend -= 4;
      --R;
    }
    const uint64_t Wstart = Wend - static_cast<uint64_t>(R) * kRB;
    const uint32_t hA = static_cast<uint32_t>(Aal - Wstart);
    const uint32_t LA = hA >> 6;
    const uint32_t jA = (hA >> 2) & 15u;
    // pointer arithmetic from p keeps the global address space (no flat ops)
    const uint8_t* seg = p - static_cast<int64_t>(A - Wstart) + lane * 64;

    // ---- round 0: contains the head of the message ----
    uint32_t w[16];
    if (Wstart >= lo)
      load_seg(w, seg);
    else
      load_seg_checked(w, seg, lo);
    s = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (static_cast<uint32_t>(j) == jA) {
        if (m == 0) {
          const uint32_t s0 = (lane == LA) ? ~init : s;
          s = crc_g(L, lb, s0 ^ w[j]);
        } else {
          const uint32_t sn = crc_g(L, lb, s ^ w[j]);
          uint32_t sb = ~init;
          uint32_t wb = w[j] >> (8 * m);
          for (uint32_t b = m; b < 4; ++b) {
            sb = crc_byte(L, lb, sb, wb & 0xffu);
            wb >>= 8;
          }
          s = (lane == LA) ? sb : sn;
        }
      } else {
        s = crc_g(L, lb, s ^ w[j]);
      }
    }
    s = (lane < LA) ? 0u : s;

    // ---- rounds 1..R-1: plain streaming ----
    for (uint32_t r = 1; r < R; ++r) {
      seg += kRB;
      load_seg(w, seg);
      s = crc_shift(L, kOffJump, s);
#pragma unroll
      for (int j = 0; j < 16; ++j) s = crc_g(L, lb, s ^ w[j]);
    }

    // ---- combine the 64 lane states (xor butterfly, all lanes end equal) --
#pragma unroll
    for (int k = 0; k < FORST_CRC_TREE_LEVELS; ++k) {
      const uint32_t other = __shfl_xor(s, 1 << k);
      const bool right = (lane >> k) & 1;
      const uint32_t left_v = right ? other : s;
      const uint32_t right_v = right ? s : other;
      s = crc_shift(L, kOffTree + 1024u * k, left_v) ^ right_v;
    }

    // ---- tail bytes [Wend, E) ----
    const uint8_t* t = p + (Wend - A);
    const uint32_t nt = static_cast<uint32_t>(E - Wend);
    for (uint32_t i = 0; i < nt; ++i) s = crc_byte(L, lb, s, ldu8(t + i));
  }
  if (nextra) s = crc_byte(L, lb, s, extra);
  return ~s;
}

__device__ __forceinline__ void fill_tables(uint32_t* L) {
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < 4 * 256 * kRep; i += kThreads) L[i] = kCrcG[i >> 5];
  for (uint32_t i = tid; i < 1024; i += kThreads) L[kOffJump + i] = kCrcJump[i];
  for (uint32_t i = tid; i < FORST_CRC_TREE_LEVELS * 1024; i += kThreads)
    L[kOffTree + i] = kCrcTree[i];
  __syncthreads();
}

// ---------------------------------------------------------------------------
// The rows and lane kernels' tables (crc_lds.h has the layout of the first
// 64 KiB and the lookups).  LDS byte addresses; the kernel's table array is
// the __shared__ object at 0:
//   [0, 64K)       G and the kernel's hop J, replicated 8x and interleaved
//   [64K, 124K)    A[1..15]: shift by 32 lo bytes (unreplicated, 4 KiB each)
//   [124K, 128K)   B[1]: shift by 512 bytes
// ---------------------------------------------------------------------------
using namespace fcrc;
constexpr uint32_t kOffA2 = 65536;
constexpr uint32_t kOffB2 = kOffA2 + 15 * 4096;
constexpr uint32_t kSeg2 = FORST_CRC2_SEG_BYTES;  // 32: a lane's segment of a chain

// raw mode with a per-message init: S0 = ~init moved back over m bytes
__device__ __forceinline__ uint32_t unstep_m(uint32_t v, uint32_t m) {
  if (m == 0) return v;
  const uint32_t* col = kCrcUnstep + 32 * (m - 1);
  uint32_t r = 0;
  for (uint32_t i = 0; i < 32; ++i) r ^= ((v >> i) & 1u) ? col[i] : 0u;
  return r;
}

template <int MODE>
__device__ __forceinline__ bool mem_last_byte(const BlockArgs& a) {
  return MODE == kModeVerify || ((MODE == kModeCompute || MODE == kModeTrailer) && !a.last_bytes);
}

// short messages (< 64 bytes past the head dword): dword-serial, wave-uniform
__device__ __forceinline__ uint32_t small_crc2(const uint8_t* __restrict__ Lb, const Lanes& K,
                                               const uint8_t* p, uint32_t len, uint32_t init,
                                               uint32_t nextra, uint32_t extra) {
  uint32_t s = ~init;
  const uint32_t m = static_cast<uint32_t>(reinterpret_cast<uint64_t>(p) & 3);
  uint32_t nh = (4 - m) & 3;
  nh = nh < len ? nh : len;
  uint32_t y = 0;
  for (uint32_t i = 0; i < nh; ++i) y |= ldu8(p + i) << (8 * i);
  s = step_k(Lb, K, s, y, nh);
  uint32_t i = nh;
  for (; i + 4 <= len; i += 4) s = rep_map<false>(Lb, K, s ^ ld4v(p + i));
  y = 0;
  const uint32_t nt = len - i;
  for (uint32_t j = 0; j < nt; ++j) y |= ldu8(p + i + j) << (8 * j);
  s = step_k(Lb, K, s, y, nt);
  if (nextra) s = step_k(Lb, K, s, extra & 0xffu, 1);
  return ~s;
}

// ---------------------------------------------------------------------------
// CRC32C rows kernel (v3): one block per 16-lane row.
//
// In a one-block-per-wave kernel every block pays a full-wave finish
// (row-end shifts, DPP reduction, round-end shifts, tail step), a head set-up
// and a scalar block set-up; for 4 KiB blocks that is a third of the work.
// Here row r (lanes 16r..16r+15) owns a block and walks it in 1 KiB rounds:
// chain c (0, 1) of lane t owns the 32-byte segment [512c + 32t, +32) of
// every round, the hop to the next round is J3 = shift by 1024 - 32 + 4 bytes
// fused with the first dword step.  The four rows finish their blocks with
// ONE instruction stream: A[15 - t] moves each chain state to the end of the
// row, a 4-level DPP XOR reduces the row, B[1] (shift by 512) joins chain 0 to
// chain 1, and one k-byte slicing step adds the <= 3 tail bytes and the type
// byte.  Rows draw blocks dynamically from the wave's contiguous share (as in
// xxh3_rows_kernel); the head of a block is handled in round 0 of its row by
// zeroing the words in front of the message and injecting S0 into the head
// word, with rows at round 0 and rows in the middle of a block running the
// same code (J3(0) = 0).
//
// LDS: [0, 64K) G and J3 interleaved (crc_lds.h), [64K, 124K) A[1..15],
// [124K, 128K) B[1].
// ---------------------------------------------------------------------------
// block-mode results are staged in LDS and stored after the loop, not as rows
// finish: result stores in the streaming loop cost C2 verify 4.7 % (stores
// share vmcnt with the loads; profiles/ab_r04/c2_verify_stores.log)
constexpr uint32_t kStageW = 6144;  // results per workgroup (30 KiB of LDS)
constexpr uint32_t kRowRound = 1024;
constexpr uint32_t kRowChain = 512;
constexpr uint32_t kLds3Bytes = kOffB2 + 4096;
constexpr uint32_t kNoBlk = 0xffffffffu;

// NT = the workgroup's thread count: constant trip counts, so every load of
// the fill is issued before the first LDS store waits (a loop with a
// blockDim trip count waited out one round of loads per iteration)
template <uint32_t NT>
__device__ __forceinline__ void fill_tables3(uint32_t* L) {
  const uint32_t tid = threadIdx.x;
  constexpr uint32_t kN1 = (16384 + NT - 1) / NT, kN2 = (15 * 1024 + NT - 1) / NT,
                     kN3 = (1024 + NT - 1) / NT;
  uint32_t v1[kN1], v2[kN2], v3[kN3];
#pragma unroll
  for (uint32_t k = 0; k < kN1; ++k) {
    const uint32_t i = tid + k * NT;
    const uint32_t e = (i >> 6) & 255, d = i & 63, t = (d >> 3) & 3;
    v1[k] = i < 16384 ? (d < 32 ? kCrcG[t * 256 + e] : kCrcJ3[t * 256 + e]) : 0u;
  }
#pragma unroll
  for (uint32_t k = 0; k < kN2; ++k) {
    const uint32_t i = tid + k * NT;
    v2[k] = i < 15 * 1024 ? kCrcA[i] : 0u;
  }
#pragma unroll
  for (uint32_t k = 0; k < kN3; ++k) {
    const uint32_t i = tid + k * NT;
    v3[k] = i < 1024 ? kCrcB[i] : 0u;
  }
#pragma unroll
  for (uint32_t k = 0; k < kN1; ++k)
    if (tid + k * NT < 16384) L[tid + k * NT] = v1[k];
#pragma unroll
  for (uint32_t k = 0; k < kN2; ++k)
    if (tid + k * NT < 15 * 1024) L[kOffA2 / 4 + tid + k * NT] = v2[k];
#pragma unroll
  for (uint32_t k = 0; k < kN3; ++k)
    if (tid + k * NT < 1024) L[kOffB2 / 4 + tid + k * NT] = v3[k];
  __syncthreads();
}

// a row's position (block of the wave share, 1 KiB round) and the block's
// window, derived once when the block is assigned; row-uniform, one copy per
// lane.  Offsets are relative to base and kept in the form the step's loads
// use, so a step issues its loads with a few adds (the per-step address
// arithmetic was a third of a 4 KiB block's VALU instructions).
struct CRowPos {
  uint32_t rp_lo, rp_hi;  // this round's window start (int64; < 0 only in round 0 near offset 0)
  uint32_t tp_lo, tp_hi;  // fast rows: the last round's finishing word t0, minus 4; slow: block offset
  uint32_t rel;           // descriptor index (kNoBlk: none)
  uint32_t rl;            // rounds left, this one included
  // cA:1 tA:4 jA:3 q:3 nt:2 m:2 valid:1 slow:1 xtra:1 d1:2 r0:1 | 24: slow rows' size:4
  // (every field a fast row needs after the derive is here: 7 VGPRs per copy)
  uint32_t pk;
  __device__ __forceinline__ int64_t rp() const {
    return static_cast<int64_t>((static_cast<uint64_t>(rp_hi) << 32) | rp_lo);
  }
  __device__ __forceinline__ uint64_t tp() const {
    return (static_cast<uint64_t>(tp_hi) << 32) | tp_lo;
  }
  __device__ __forceinline__ uint32_t cA() const { return pk & 1u; }
  __device__ __forceinline__ uint32_t tA() const { return (pk >> 1) & 15u; }
  __device__ __forceinline__ uint32_t jA() const { return (pk >> 5) & 7u; }
  __device__ __forceinline__ uint32_t q() const { return (pk >> 8) & 7u; }
  __device__ __forceinline__ uint32_t nt() const { return (pk >> 11) & 3u; }
  __device__ __forceinline__ uint32_t m() const { return (pk >> 13) & 3u; }
  __device__ __forceinline__ bool valid() const { return (pk >> 15) & 1u; }
  __device__ __forceinline__ bool slow() const { return (pk >> 16) & 1u; }
  __device__ __forceinline__ bool xtra() const { return (pk >> 17) & 1u; }
  __device__ __forceinline__ uint32_t d1() const { return (pk >> 16) & 12u; }  // bytes: 0, 4, 8
  __device__ __forceinline__ bool r0() const { return (pk >> 20) & 1u; }
  __device__ __forceinline__ uint32_t slow_size() const { return (pk >> 24) & 15u; }
  // (length-split batches) no descriptor yet, more may come: ask again
  __device__ __forceinline__ bool wait() const { return (pk >> 21) & 1u; }
  // fast rows: offset + size of the block (where a trailer goes), from the
  // window end: E - the type byte when it is in memory
  template <int MODE>
  __device__ __forceinline__ uint64_t end(bool mlb) const {
    const uint64_t t0 = tp() + 4;
    const uint64_t we = (MODE == kModeVerify || nt() > 0) ? t0 : t0 + 4;
    return we + nt() - (mlb ? 1u : 0u);
  }
};

template <int MODE>
__device__ __forceinline__ void crow_derive(const BlockArgs& a, uint64_t off, uint32_t size,
                                            CRowPos& P) {
  const bool valid = P.rel != kNoBlk && desc_in_range<MODE>(a, Desc{off, size, 0, 0});
  const uint64_t E = off + size + (mem_last_byte<MODE>(a) ? 1u : 0u);
  const uint64_t ws = off & ~3ull;
  const uint64_t we = E & ~3ull;
  const uint64_t d4 = we - ws;
  // a window one dword longer than whole rounds (1/4 of back-to-back 4 KiB
  // blocks: 4097 checksummed bytes starting at offset = 3 mod 4) ends one
  // dword early; that dword is one slicing step in the finish instead of a
  // fifth, almost empty round
  // (block modes only: raw messages of arbitrary lengths rarely hit it)
  const bool xtra = MODE != kModeRaw && (d4 & (kRowRound - 1)) == 4 && d4 > kRowRound;
  uint32_t R = static_cast<uint32_t>(xtra ? d4 / kRowRound : (d4 + kRowRound - 1) / kRowRound);
  int64_t w0 = static_cast<int64_t>(we) - (xtra ? 4 : 0) - static_cast<int64_t>(R) * kRowRound;
  const uint32_t hA = static_cast<uint32_t>(static_cast<int64_t>(ws) - w0);
  const uint32_t cA = hA >> 9, tA = (hA >> 5) & 15u, jA = (hA >> 2) & 7u;
  const int64_t seg_head = static_cast<int64_t>(ws) - 4 * static_cast<int64_t>(jA);
  const uint32_t q = seg_head < 0 ? static_cast<uint32_t>(-seg_head) >> 2 : 0u;
  const uint32_t nt = static_cast<uint32_t>(E - we);
  const uint32_t m = static_cast<uint32_t>(off & 3);
  // the finishing words: t0 = the tail dword at the window end (verify: the
  // word holding the stored checksum when nt = 0), t1 = the word after it
  // (verify, nt > 0) or the extra window dword (compute / trailer, xtra), t2
  // = the extra window dword (verify, xtra) -- loaded at tp + 4, tp + d1 and
  // tp, so t0 >= 4 (else the slow path: messages ending in the first dwords)
  const uint64_t t0 = (nt > 0 || MODE == kModeVerify) ? we : we - 4;
  const uint32_t d1 = MODE == kModeVerify ? (nt > 0 ? 8u : 4u) : (xtra && nt > 0 ? 0u : 4u);
  // messages without one whole dword take the slow path (its loads are serial
  // and unprefetched: a WAL record of 40 B through it cost a wave ~10 dependent
  // load latencies); everything else, however short, is one prefetched round
  const bool slow = !valid || d4 < 4 || t0 < 4;
  const uint64_t tp = slow ? off : t0 - 4;
  if (slow) {  // the slow path loads on its own; dummy round loads at [0, 1 KiB)
    R = 1;
    w0 = 0;
  }
  P.rl = R;
  P.rp_lo = static_cast<uint32_t>(w0);
  P.rp_hi = static_cast<uint32_t>(static_cast<uint64_t>(w0) >> 32);
  P.tp_lo = static_cast<uint32_t>(tp);
  P.tp_hi = static_cast<uint32_t>(tp >> 32);
  // a valid slow block has fewer than 12 checksummed bytes (d4 < 4 or t0 < 4)
  P.pk = (slow ? (valid ? (size & 15u) << 24 : 0u)
               : (cA | (tA << 1) | (jA << 5) | (q << 8) | (xtra ? 1u << 17 : 0u) |
                  ((d1 >> 2) << 18))) |
         (nt << 11) | (m << 13) | (valid ? 1u << 15 : 0u) | (slow ? 1u << 16 : 0u) | (1u << 20);
}

struct CRStep {
  uint32_t w[2][8];
  uint32_t t0, t1, t2, mod, extra;  // t2: the extra window dword (xtra)
};

template <int MODE>
__device__ __forceinline__ void crow_issue(const BlockArgs& a, uint32_t lane, const CRowPos& P,
                                           uint64_t kbeg, CRStep& d) {
  const uint32_t t = lane & 15;
  // the lane's chain-0 segment; chain 1 is 512 bytes on.  Round-0 segments
  // in front of the head hold no message byte: they are loaded from where
  // they are and discarded by the head reset; only a segment in front of the
  // buffer start (a message ending in its first KiB) is loaded from 0 (the
  // head lane's is realigned by q dwords in the head step).  No branch around
  // a load: a step's loads must not depend on one, or the compiler's vmcnt
  // waits for the current step's data also wait for the step in flight.
  int64_t s0 = P.rp() + kSeg2 * t;
  int64_t s1 = s0 + kRowChain;
  if (__ballot(s0 < 0)) {  // rare (addresses only): a round in front of offset 0
    s0 = s0 < 0 ? 0 : s0;
    s1 = s1 < 0 ? 0 : s1;
  }
  // (Loading the round-0 segments in front of a raw record's head from the
  // buffer's first KiB instead, to save their HBM bytes -- 1.07x the log on
  // C5 -- measured no faster: C5 verify 0.604-0.608 vs 0.606-0.609,
  // profiles/ab_r05/raw_pre_head_redirect_C5.log.  They are mostly the
  // previous record's bytes, which its own row reads at about the same time.)
#pragma unroll
  for (uint32_t c = 0; c < 2; ++c) {
    const uint8_t* sp = a.base + (c ? s1 : s0);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const u32x4a4 v = ld16_a4(sp + 16 * q);
      d.w[c][4 * q + 0] = v.x;
      d.w[c][4 * q + 1] = v.y;
      d.w[c][4 * q + 2] = v.z;
      d.w[c][4 * q + 3] = v.w;
    }
  }
  // the finishing step's words, loaded in every step (from offset 0 when not
  // needed): a step's load count must not depend on a branch (see above)
  const bool lastr = !P.slow() && P.rl <= 1;
  const uint8_t* pb = a.base + (lastr ? P.tp() : 0);
  d.t0 = ld4_a4(pb + 4);
  d.t1 = MODE == kModeRaw ? 0u : ld4_a4(pb + P.d1());
  d.t2 = MODE == kModeVerify ? ld4_a4(pb) : 0u;
  // optional arrays: (read in the ISA) a branch around these loads keeps the
  // compiler's vmcnt waits precise, a pointer select to a zero word does not
  const uint64_t idx = kbeg + (P.rel == kNoBlk ? 0 : P.rel);
  if (MODE != kModeRaw)
    d.mod = a.modifiers ? a.modifiers[idx] : 0u;
  else
    d.mod = a.expect ? a.expect[idx] : 0u;  // (raw: the expected CRC)
  if (MODE == kModeRaw)
    d.extra = a.init_crcs ? a.init_crcs[idx] : 0u;
  else if (MODE != kModeVerify)
    d.extra = a.last_bytes ? a.last_bytes[idx] : 0u;
  else
    d.extra = 0u;
}

// Raw batches split by message length (FILT): messages shorter than
// kRawSplit bytes go to crc32c_raw_lane_kernel (one message per lane), the
// rest to the rows kernel, which drops the short ones from each descriptor
// batch as it loads it.  A short WAL record still costs a row a whole 1 KiB
// round; on C5 the records <= 512 B (40 % of them, 1.5 % of the bytes) took
// 0.69 ms of the 9.03 ms raw pass (profiles/ab_r04/c5_record_classes_raw_crc.json).
constexpr uint32_t kRawSplit = 256;

// A message goes to the rows filter kernel when it has kRawSplit bytes or
// more and its offset is below 2^58 (any larger one lies outside every
// buffer: the lane kernel reports it; batch_compact, stream_common.h).
__device__ __forceinline__ bool raw_long(uint64_t off, uint32_t size) {
  return size >= kRawSplit && (off >> 58) == 0;
}

template <int MODE, bool RAW_WG = false, bool FILT = false>
__device__ __forceinline__ void crc32c_rows_body(const BlockArgs& a) {
  static_assert(!FILT || (MODE == kModeRaw && !RAW_WG), "length split: raw global feed only");
  __shared__ uint32_t L[kLds3Bytes / 4];
  feed_init();
  fill_tables3<kThreads>(L);
  const uint8_t* Lb = reinterpret_cast<const uint8_t*>(L);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = uniform(threadIdx.x >> 6);
  const uint32_t t = lane & 15;
  const Lanes K = lanes(lane);
  __shared__ uint32_t s0t[4];  // head states by start alignment (a select, not branches)
  if (threadIdx.x < 4) s0t[threadIdx.x] = kCrcS0[threadIdx.x];
  __syncthreads();
  const uint64_t nw = static_cast<uint64_t>(gridDim.x) * kWaves;
  const uint64_t gw = static_cast<uint64_t>(blockIdx.x) * kWaves + wave;
  const bool has_extra = (MODE == kModeCompute || MODE == kModeTrailer) && a.last_bytes;

  // descriptor batches from the work feed: lane j <-> descriptor cg + j (cb),
  // ng + j (nb); a row's rel is the descriptor's index in the launch (n <=
  // FORST_ROWS_MAX_DESCS, engine.h)
  BatchFeed feed;
  // block modes: the workgroup feed in 4-descriptor batches (one block per
  // row; A/B against 8: C2 verify +2.2 %, write +1.8 %, NS16 +0.9 %, C4
  // +1.4 %, profiles/ab_r03/crc_feed_batch.log; 16 was 3 % slower than 8);
  // WAL records (raw) keep the global feed (byte-balanced workgroup ranges
  // measured within noise for them, profiles/ab_r03/wal_wg_feed.log), except
  // small raw batches (RAW_WG: crc32c_rows_raw_small_kernel)
  constexpr bool kWgFeed = MODE != kModeRaw || RAW_WG;
  constexpr uint32_t kChunk = 4;
  uint64_t cg = feed_first<kWgFeed, kChunk>(a, nw, gw, lane, feed);
  // verify: results staged in LDS, stored after the loop by the whole
  // workgroup (so every wave reaches the end: no early return)
  constexpr bool kStage = MODE != kModeRaw;
  __shared__ uint32_t st_out[kStage ? kStageW : 1];
  __shared__ uint8_t st_ok[kStage ? kStageW : 4];
  // raw mode: each wave's results collected in an LDS ring and stored 64 per
  // instruction when it fills and after the loop (stores share vmcnt with the
  // loads, so a store per finishing row delayed the next step's data)
  constexpr bool kRing = MODE == kModeRaw;
  constexpr uint32_t kRingN = 224;  // per wave (16 waves: 28 KiB beside the 128 KiB of tables)
  __shared__ uint32_t ring_i[kRing ? kWaves * kRingN : 1], ring_v[kRing ? kWaves * kRingN : 1];
  uint32_t* const ri = ring_i + (kRing ? wave * kRingN : 0);
  uint32_t* const rv = ring_v + (kRing ? wave * kRingN : 0);
  uint32_t rcount = 0;  // (wave-uniform)
  auto ring_flush = [&]() {
    wave_lds_sync();
    for (uint32_t j = lane; j < rcount; j += 64) a.out32[ri[j]] = rv[j];
    wave_lds_sync();
    rcount = 0;
  };
  if (!kStage && cg >= a.n) return;
  uint32_t clen = feed.len;  // entries of cb / nb (a batch holds up to 64)
  uint64_t ng = 0;
  uint32_t nlen = 0;
  if constexpr (!FILT) {  // (FILT: claimed after cb, whose loading may claim further)
    ng = feed_next<kWgFeed, kChunk>(a, nw, lane, feed);
    nlen = feed.len;
  }
  DescBatch cb, nb;
  uint64_t kbrel = 0;  // stream position of cb's first entry
  // FILT: the batch's messages of kRawSplit bytes or more, moved to its
  // first lanes; a batch with none is skipped (the next one claimed) so a
  // batch is empty only once the feed is exhausted.  (The ballot waits for
  // the batch's loads: one load latency per 64 descriptors.)
  auto load_f = [&](uint64_t& g, uint32_t& len, DescBatch& d) {
    load_batch<MODE>(a, g, a.n, lane, d);
    if constexpr (FILT) {
      for (;;) {
        const bool keep =
            lane < len && raw_long((static_cast<uint64_t>(d.off_hi) << 32) | d.off_lo, d.size);
        const uint64_t km = __ballot(keep);
        if (km != 0 || len == 0) {
          batch_compact<false, false>(d, km, keep, lane);
          len = static_cast<uint32_t>(__popcll(km));
          break;
        }
        g = feed_next<kWgFeed, kChunk>(a, nw, lane, feed);
        len = feed.len;
        load_batch<MODE>(a, g, a.n, lane, d);
      }
    }
  };
  load_f(cg, clen, cb);
  if constexpr (FILT) {
    ng = feed_next<kWgFeed, kChunk>(a, nw, lane, feed);
    nlen = feed.len;
  }
  load_f(ng, nlen, nb);
  const uint64_t kbeg = 0;
  auto fetch = [&](uint64_t rel, CRowPos& P) {
    const BatchSlot q = batch_slot(rel, kbrel, cg, clen, ng, nlen, a.n);
    const uint32_t lo_c = __shfl(cb.off_lo, q.src), hi_c = __shfl(cb.off_hi, q.src);
    const uint32_t sz_c = __shfl(cb.size, q.src);
    const uint32_t lo_n = __shfl(nb.off_lo, q.src), hi_n = __shfl(nb.off_hi, q.src);
    const uint32_t sz_n = __shfl(nb.size, q.src);
    uint32_t hi = q.in_n ? hi_n : hi_c;
    uint64_t gi = q.gi;
    if constexpr (FILT) {  // slot k of a compacted batch: descriptor base + its lane as loaded
      gi = (q.in_n ? ng : cg) + (hi >> 26);
      hi &= 0x03ffffffu;
    }
    const uint64_t off = (static_cast<uint64_t>(hi) << 32) | (q.in_n ? lo_n : lo_c);
    const uint32_t size = q.in_n ? sz_n : sz_c;
    P.rel = q.valid ? static_cast<uint32_t>(gi) : kNoBlk;
    crow_derive<MODE>(a, off, size, P);
  };
  // A compacted batch may hold fewer descriptors than the wave has rows
  // (FILT): positions are handed out only while cb and nb have some left, and
  // a row that finds none WAITS (asks again in the next step) unless the feed
  // is exhausted -- a position handed to no row would be a descriptor never
  // computed.  (Full batches have 64: the original rule never runs short.)
  uint64_t next = 4;
  CRowPos C;
  fetch(lane >> 4, C);
  if constexpr (FILT) {
    const uint64_t avail = clen + nlen;
    if ((lane >> 4) >= avail && nlen != 0) C.pk |= 1u << 21;
    next = avail < 4 ? avail : 4;
  }
  auto advance = [&](const CRowPos& P, CRowPos& I) {
    const bool more = P.rel != kNoBlk && !P.slow() && P.rl > 1;
    const bool need = (P.rel != kNoBlk || (FILT && P.wait())) && !more;
    const uint64_t rows = __ballot(need && t == 0);  // one bit per row leader
    I = P;
    if (more) {
      I.rl = P.rl - 1;
      I.pk = P.pk & ~(1u << 20);
      const int64_t rp = P.rp() + kRowRound;
      I.rp_lo = static_cast<uint32_t>(rp);
      I.rp_hi = static_cast<uint32_t>(static_cast<uint64_t>(rp) >> 32);
    }
    // rows in the middle of their blocks (every row, 3 steps in 4 of a batch
    // of 4 KiB blocks): no descriptor work
    if (rows) {
      // rows needing one ahead of this row: rows' bits below the lane, less
      // the row's own leader bit (rows holds leader bits only) -- v_mbcnt, no
      // per-lane 64-bit mask held across the loop
      const uint32_t below = __builtin_amdgcn_mbcnt_hi(
          static_cast<uint32_t>(rows >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(rows), 0u));
      const uint32_t rank = below - (t != 0 && need ? 1u : 0u);
      CRowPos F;
      fetch(next + rank, F);
      uint64_t got = static_cast<uint64_t>(__popcll(rows));
      if constexpr (FILT) {
        const uint64_t avail = kbrel + clen + nlen - next;
        if (got > avail) got = avail;
        if (rank >= avail && nlen != 0) F.pk |= 1u << 21;
      }
      next += got;
      if (need) I = F;
      if (next >= kbrel + clen) {  // every block of cb is assigned: slide the batches
        kbrel += clen;
        clen = nlen;
        cb = nb;
#ifndef FORST_HOST_EMULATION
        // cb's copies are made here, so the batch loads below can land in
        // nb's registers directly (a load into a temporary and a move after
        // it waited for every load in flight, the step's prefetch included)
        asm volatile("" : "+v"(cb.off_lo), "+v"(cb.off_hi), "+v"(cb.size));
#endif
        cg = ng;
        ng = feed_next<kWgFeed, kChunk>(a, nw, lane, feed);
        nlen = feed.len;
        load_f(ng, nlen, nb);
      }
    }
  };
  CRowPos I;
  advance(C, I);
  CRStep X, Y;
  crow_issue<MODE>(a, lane, C, kbeg, X);
  uint32_t s[2] = {0, 0};

  // cu: the current step's data (ready); nx: the buffer that receives the
  // loads issued now (the position one step ahead)
  auto step = [&](CRStep& cu, CRStep& nx) -> bool {
    // raw mode (WAL records, mixed sizes): no early return (see
    // xxh3_frag_kernel), both step copies issue on every path round the loop
    // and the next step's loads overlap this step's wait (C5 verify / writer
    // +1.5 %); the block modes keep the early exit, which measured better on
    // uniform blocks (A/B on one box: C2 0.600 vs 0.592)
    const bool live = __ballot(C.rel != kNoBlk || (FILT && C.wait())) != 0;
    if (MODE != kModeRaw && !live) return false;
    crow_issue<MODE>(a, lane, I, kbeg, nx);
    const bool fast = C.rel != kNoBlk && !C.slow();
    const bool r0 = C.r0();
    // ---- one 1 KiB round of every row ----
    // A row at round 0 starts its block: its chain states start at 0 (J3(0) =
    // 0), segments wholly in front of the head end the round at state 0, and
    // in the head lane the running value is RESET at the head word to
    // (word & bm) ^ S0 (the head dword without the bytes in front of the
    // message, plus the initial state moved back over them), which discards
    // whatever the words in front of it added.  Steps without a row at
    // round 0 run the plain chains.
    const bool head = __ballot(fast && r0);
    if (!head) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        uint32_t lj[4], lg[4];
        look<true>(Lb, K, r0 ? 0u : s[c], lj);
        look<false>(Lb, K, cu.w[c][0], lg);
        uint32_t x = xor3(xor3(lj[0], lj[1], lj[2]), xor3(lj[3], lg[0], lg[1]),
                          xor3(lg[2], lg[3], cu.w[c][1]));
#pragma unroll
        for (int j = 2; j < 8; ++j) x = g_then(Lb, K, x, cu.w[c][j]);
        s[c] = g_then(Lb, K, x, 0u);
      }
    } else {
      const uint32_t cA = C.cA(), tA = C.tA(), jA = C.jA(), q = C.q(), m = C.m();
      const uint32_t bm = 0xffffffffu << (8 * m);
      // raw mode with per-message inits: the GF(2) unstep; without (crc32c::Value,
      // every WAL record) S0 is the block modes' constant
      const uint32_t S0 = MODE == kModeRaw && a.init_crcs ? unstep_m(~cu.extra, m) : s0t[m];
#pragma unroll
      for (uint32_t c = 0; c < 2; ++c) {
        const bool hl = fast && r0 && c == cA && t == tA;  // the head lane of the row
        const bool pre = fast && r0 && (c < cA || (c == cA && t < tA));
        const uint32_t hj = hl ? jA : 8u;
        uint32_t wc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) wc[j] = cu.w[c][j];
        if (__ballot(hl && q != 0)) {  // head segment loaded from 0: shift up q dwords
          uint32_t sh[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            uint32_t v = 0;
#pragma unroll
            for (int qq = 1; qq < 8; ++qq)
              if (qq <= j) v = (q == static_cast<uint32_t>(qq)) ? wc[j - qq] : v;
            sh[j] = v;
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) wc[j] = (hl && q != 0) ? sh[j] : wc[j];
        }
        uint32_t lj[4], lg[4];
        look<true>(Lb, K, r0 ? 0u : s[c], lj);
        look<false>(Lb, K, hj == 0 ? ((wc[0] & bm) ^ S0) : wc[0], lg);
        uint32_t x = xor3(xor3(lj[0], lj[1], lj[2]), xor3(lj[3], lg[0], lg[1]),
                          xor3(lg[2], lg[3], wc[1]));
        x = hj == 1 ? ((wc[1] & bm) ^ S0) : x;
#pragma unroll
        for (uint32_t j = 2; j < 8; ++j) {
          x = g_then(Lb, K, x, wc[j]);
          x = hj == j ? ((wc[j] & bm) ^ S0) : x;
        }
        s[c] = pre ? 0u : g_then(Lb, K, x, 0u);
      }
    }
    // ---- rows that finish a block in this step ----
    const bool fin = C.rel != kNoBlk && (C.slow() || C.rl <= 1);
    if (__ballot(fin)) {
      // chain states to the row end (A[15 - t]), row XOR, chain 0 over chain 1
      const bool lo0 = t == 15;
      const uint32_t abase = kOffA2 + 4096 * (14 - t);
      uint32_t a0 = lo0 ? s[0] : shift_at(Lb, abase, s[0]);
      uint32_t a1 = lo0 ? s[1] : shift_at(Lb, abase, s[1]);
      a0 = row_ror_xor<1>(a0);
      a1 = row_ror_xor<1>(a1);
      a0 = row_ror_xor<2>(a0);
      a1 = row_ror_xor<2>(a1);
      a0 = row_ror_xor<4>(a0);
      a1 = row_ror_xor<4>(a1);
      a0 = row_ror_xor<8>(a0);
      a1 = row_ror_xor<8>(a1);
      uint32_t crc = 0, stored = 0;
      const uint32_t nt = C.nt();
      // lanes that finish the CRC: the row's last lane, and in trailer mode
      // lanes 11..15, which store the 5 trailer bytes with one instruction
      const bool calc = fin && (MODE == kModeTrailer ? t >= 11 : lo0);
      if (calc) {
        uint32_t st = shift_at(Lb, kOffB2, a0) ^ a1;
        if (MODE != kModeRaw && C.xtra()) st = step_k(Lb, K, st, MODE == kModeVerify ? cu.t2 : cu.t1, 4);
        uint32_t y = nt ? (cu.t0 & (0xffffffffu >> (32 - 8 * nt))) : 0u;
        uint32_t k = nt;
        if (has_extra) {
          y |= (cu.extra & 0xffu) << (8 * k);
          ++k;
        }
        crc = ~step_k(Lb, K, st, y, k);
        if (MODE == kModeVerify) stored = nt ? __builtin_amdgcn_alignbyte(cu.t1, cu.t0, nt) : cu.t0;
      }
      if (calc && C.slow() && C.valid()) {
        const uint8_t* pp = a.base + C.tp();  // slow rows: the block offset
        const uint32_t init = MODE == kModeRaw ? cu.extra : 0u;
        crc = small_crc2(Lb, K, pp, C.slow_size() + (mem_last_byte<MODE>(a) ? 1u : 0u), init,
                         has_extra ? 1u : 0u, cu.extra);
        if (MODE == kModeVerify) stored = retire(ldu32(pp + C.slow_size() + 1));
        crc = retire(crc);
      }
      const bool valid = C.valid();
      const bool mine = fin && lo0;
      const uint64_t i = kbeg + (C.rel == kNoBlk ? 0 : C.rel);
      bool ok = valid;
      if (MODE == kModeRaw) {
        // WAL writer mode: masked (log_writer.cc:263).  The in-place header
        // stores are a separate pass (wal.hip): stores share vmcnt with the
        // loads on gfx950, so scattered partial-line stores here made every
        // later step wait for them (C5 writer 9.19 -> 9.90 ms)
        const uint32_t v = a.wal_hs ? crc_mask(crc) : crc;
        const bool differs = !a.expect || !valid || v != cu.mod;
        if constexpr (kRing) {
          const bool put = mine && differs && a.out32 != nullptr;
          const uint64_t pm = __ballot(put);
          if (pm) {
            const uint32_t at = rcount + __builtin_amdgcn_mbcnt_hi(
                static_cast<uint32_t>(pm >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(pm), 0u));
            if (put) {
              ri[at] = static_cast<uint32_t>(i);
              rv[at] = valid ? v : 0u;
            }
            rcount += static_cast<uint32_t>(__popcll(pm));
            if (rcount > kRingN - 64) ring_flush();
          }
        }
      } else if (MODE == kModeVerify) {
        const uint32_t computed = crc_mask(crc);  // reader_common.cc:36-47
        const uint32_t st = stored - cu.mod;
        ok = valid && st == computed;
        // the workgroup's first kStageW results go to LDS (written after the
        // loop), the rest (ranges longer than that) directly
        const uint64_t sj = i - feed.wlo;
        const bool staged = kStage && sj < kStageW;
        if (mine && staged) {
          st_out[sj] = valid ? computed : 0u;
          st_ok[sj] = ok ? 1 : 0;
        }
        if (mine && !staged && a.out32) a.out32[i] = valid ? computed : 0u;
        if (mine && a.stored_out) a.stored_out[i] = valid ? st : 0u;
        if (mine && !staged && a.ok_out) a.ok_out[i] = ok ? 1 : 0;
        if (staged) ok = true;  // (counted in the flush)
      } else {
        const uint32_t out = crc_mask(crc) + cu.mod;  // format.cc:594-600 + builder.cc:1340-1345
        const uint64_t sj = i - feed.wlo;
        const bool staged = kStage && sj < kStageW;  // (see verify)
        if (mine && staged) {
          st_out[sj] = valid ? out : 0u;
          st_ok[sj] = valid ? 1 : 0;
        }
        if (mine && !staged && a.out32) a.out32[i] = valid ? out : 0u;
        if (MODE == kModeTrailer) {
          // the 5 trailer bytes [type][LE32] by lanes 11..15 of the row: one
          // byte store per wave instead of five per finishing row
          const uint32_t k = t - 11;
          if (!staged && calc && valid && (k != 0 || a.last_bytes)) {
            // (slow rows keep the block offset in tp and their size in pk)
            uint8_t* pw = a.base_w + (C.slow() ? C.tp() + C.slow_size()
                                               : C.template end<MODE>(mem_last_byte<MODE>(a)));
            pw[k] = static_cast<uint8_t>(k == 0 ? cu.extra : out >> (8 * (k - 1)));
          }
        }
      }
      if (MODE == kModeVerify) {
        const uint64_t badm = __ballot(mine && !ok);
        if (a.mismatches && badm && lane == 0)
          atomicAdd(a.mismatches, static_cast<unsigned long long>(__popcll(badm)));
      }
    }
#ifndef FORST_HOST_EMULATION
    // the finishing words are read only when a row finishes; a use on every
    // path retires their loads here (a precise wait, the next step's loads
    // are younger), so reusing their registers in the next step needs no
    // full vmcnt(0) wait on the step in flight
    asm volatile("" ::"v"(cu.t0), "v"(cu.t1), "v"(cu.t2), "v"(cu.mod), "v"(cu.extra));
#endif
    C = I;
    advance(C, I);
    return live;
  };
  if (MODE == kModeRaw) {
    for (bool more = true; more;) {
      step(X, Y);
      more = step(Y, X);
    }
  } else {
    while (step(X, Y) && step(Y, X)) {
    }
  }
  if constexpr (kRing) {
    if (rcount) ring_flush();
  }
  if constexpr (kStage) {  // the staged results, coalesced
    __syncthreads();
    const uint64_t lo = feed.wlo, hi = feed.whi;
    const uint64_t m = hi > lo ? (hi - lo < kStageW ? hi - lo : kStageW) : 0;
    uint32_t bad = 0;
    for (uint32_t j = threadIdx.x; j < m; j += blockDim.x) {
      const uint64_t g = lo + j;
      if (a.out32) a.out32[g] = st_out[j];
      if (MODE == kModeVerify) {
        if (a.ok_out) a.ok_out[g] = st_ok[j];
        bad += st_ok[j] ? 0u : 1u;
      }
      if (MODE == kModeTrailer && st_ok[j]) {  // [type][LE32] at offset + size
        uint8_t* pw = a.base_w + a.offsets[g] + a.sizes[g];
        const uint32_t v = st_out[j];
        if (a.last_bytes) pw[0] = a.last_bytes[g];
        pw[1] = static_cast<uint8_t>(v);
        pw[2] = static_cast<uint8_t>(v >> 8);
        pw[3] = static_cast<uint8_t>(v >> 16);
        pw[4] = static_cast<uint8_t>(v >> 24);
      }
    }
    if (MODE == kModeVerify && a.mismatches) {
      uint32_t wb = bad;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) wb += __shfl_xor(wb, o);
      if (lane == 0 && wb) atomicAdd(a.mismatches, static_cast<unsigned long long>(wb));
    }
  }
}

template <int MODE>
__global__ void __launch_bounds__(kThreads) crc32c_rows_kernel(BlockArgs a) {
  crc32c_rows_body<MODE>(a);
}
// raw batches smaller than one 64-descriptor chunk per wave of the grid (the
// records a WAL recovery's fused kernel does not cover, a WAL write of a few
// records): the global feed would hand them to a few waves in 64-descriptor
// chunks, 64 records one after another on each, while the workgroup feed
// spreads them over every wave in 4-descriptor batches
__global__ void __launch_bounds__(kThreads) crc32c_rows_raw_small_kernel(BlockArgs a) {
  crc32c_rows_body<kModeRaw, true>(a);
}
// the long messages of a raw batch (kRawSplit bytes or more)
__global__ void __launch_bounds__(kThreads) crc32c_rows_raw_filt_kernel(BlockArgs a) {
  crc32c_rows_body<kModeRaw, false, true>(a);
}

// ---- the short messages of a raw batch: one message per lane --------------
// crc32c::Value(init, p, n) of a message of n < kRawSplit bytes by lane-serial
// slicing-by-4 on the G tables (the rows kernel's layout, rows of 256 bytes,
// so each ds_read of a wave is bank-conflict free).  16-byte loads, one in
// flight ahead of the dwords being folded.  The first dword starts the chain
// at S0 (~init moved back over the m = p & 3 bytes in front of the message,
// which are masked to zero), as the rows kernel's head lane does.
constexpr uint32_t kLaneThreads = 512;
// 16-byte loads of a short message: its bytes from the dword boundary in
// front (m <= 3) plus the tail dword
constexpr uint32_t kLaneChunks = (kRawSplit + 2 + 4 + 15) / 16;
__device__ __forceinline__ uint32_t lane_raw_crc(const uint8_t* __restrict__ Lb, const Lanes& K,
                                                 const uint8_t* base, uint64_t base_len,
                                                 uint64_t off, uint32_t n, uint32_t init,
                                                 bool has_init) {
  const uint32_t m = static_cast<uint32_t>(off & 3);
  const uint32_t tot = n + m;  // bytes from the dword boundary in front
  const uint32_t nd = tot >> 2, nt = tot & 3;
  const uint32_t nc = (nd + (nt ? 1u : 0u) + 3) >> 2;  // 16-byte loads
  // messages within their first dword, and the last bytes of the buffer:
  // dword-serial with byte loads at either end (never a byte past it)
  if (nd == 0 || (off - m) + 16ull * nc > base_len)
    return small_crc2(Lb, K, base + off, n, init, 0, 0);
  const uint8_t* q = base + (off - m);
  const uint32_t S0 = has_init ? unstep_m(~init, m)
                               : m == 0 ? 0xffffffffu : m == 1 ? 0xa942e6bcu
                               : m == 2 ? 0x2804363bu : 0x96db52a8u;  // kCrcS0
  const uint32_t bm = 0xffffffffu << (8 * m);
  const uint32_t tm = (1u << (8 * nt)) - 1u;
  uint32_t s = 0;
  // every load of the message first (one memory latency per message; a
  // chunk-by-chunk loop waited one per 16 bytes: C5's 3.4 M short records
  // took 0.42 ms that way), then the chain over them
  u32x4a4 v[kLaneChunks];
#pragma unroll
  for (uint32_t c = 0; c < kLaneChunks; ++c)
    v[c] = c < nc ? ld16_a4(q + 16 * c) : u32x4a4{0u, 0u, 0u, 0u};
#pragma unroll
  for (uint32_t c = 0; c < kLaneChunks; ++c) {
    if (c < nc) {
      const uint32_t w[4] = {v[c].x, v[c].y, v[c].z, v[c].w};
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t i = 4 * c + j;
        if (i < nd)
          s = rep_map<false>(Lb, K, i == 0 ? ((w[j] & bm) ^ S0) : (s ^ w[j]));
        else if (i == nd && nt)
          s = step_k(Lb, K, s, w[j] & tm, nt);
      }
    }
  }
  return ~s;
}

// every descriptor of the batch that is not raw_long (the rows filter
// kernel takes those); the same results and stores as the rows kernel's
// raw mode (wal_hs masking, expect: only differing results stored, an
// out-of-range descriptor reported as 0).  Each wave takes windows of
// kRawLaneR x 64 descriptors on its own (no workgroup barrier): it loads
// them all at once, lists the short ones' window positions in its LDS slots
// (on C5 at a 256-byte split 3 records in 10 are short) and gives them out
// one per lane, the descriptor fields moved between lanes by ds_bpermute.
// Latency bound, so waves independent: workgroup-wide windows with
// barriers, and one descriptor per thread, measured 0.36 / 0.42 ms on C5
// against this layout's.
constexpr uint32_t kRawLaneR = 4;
constexpr uint32_t kRawLaneWaves = kLaneThreads / 64;
__global__ void __launch_bounds__(kLaneThreads) crc32c_raw_lane_kernel(BlockArgs a) {
  __shared__ uint32_t L[16384];
  __shared__ uint16_t slot[kRawLaneWaves][kRawLaneR * 64];
  for (uint32_t i = threadIdx.x; i < 16384; i += kLaneThreads) {
    const uint32_t e = i >> 6, d = i & 63;
    if (d < 32) L[i] = kCrcG[((d >> 3) & 3) * 256 + e];
  }
  __syncthreads();
  const uint8_t* Lb = reinterpret_cast<const uint8_t*>(L);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = uniform(threadIdx.x >> 6);
  const Lanes K = lanes(lane);
  const uint64_t below = (1ull << lane) - 1;
  const uint64_t nw = static_cast<uint64_t>(gridDim.x) * kRawLaneWaves;
  constexpr uint64_t W = uint64_t(kRawLaneR) * 64;
  uint16_t* sl = slot[wave];
  for (uint64_t w0 = (static_cast<uint64_t>(blockIdx.x) * kRawLaneWaves + wave) * W; w0 < a.n;
       w0 += nw * W) {
    uint32_t olo[kRawLaneR], ohi[kRawLaneR], sz[kRawLaneR];
#pragma unroll
    for (uint32_t r = 0; r < kRawLaneR; ++r) {  // every load first
      uint64_t i = w0 + 64 * r + lane;
      i = i < a.n ? i : a.n - 1;
      const uint64_t off = a.offsets[i];
      olo[r] = static_cast<uint32_t>(off);
      ohi[r] = static_cast<uint32_t>(off >> 32);
      sz[r] = a.sizes[i];
    }
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t r = 0; r < kRawLaneR; ++r) {
      uint64_t off = (static_cast<uint64_t>(ohi[r]) << 32) | olo[r];
      uint32_t size = sz[r];
      if (a.wal_hs) {  // (as load_batch: header offset + payload length)
        const bool ok = off <= a.base_len && a.base_len - off >= uint64_t(a.wal_hs) + size;
        off = ok ? off + 6 : ~0ull;
        size = ok ? a.wal_hs + size - 6 : 0u;
        olo[r] = static_cast<uint32_t>(off);
        ohi[r] = static_cast<uint32_t>(off >> 32);
        sz[r] = size;
      }
      const bool sh = w0 + 64 * r + lane < a.n && !raw_long(off, size);
      const uint64_t m = __ballot(sh);
      if (sh) sl[cnt + static_cast<uint32_t>(__popcll(m & below))] = static_cast<uint16_t>(64 * r + lane);
      cnt += static_cast<uint32_t>(__popcll(m));
    }
    wave_lds_sync();
    for (uint32_t j0 = 0; j0 < cnt; j0 += 64) {  // (wave-uniform: the bpermutes need every lane)
      const uint32_t j = j0 + lane;
      const uint32_t q = j < cnt ? sl[j] : 0u;
      const int src = static_cast<int>(4 * (q & 63));
      uint32_t lo = 0, hi = 0, size = 0;
#pragma unroll
      for (uint32_t r = 0; r < kRawLaneR; ++r) {
        const uint32_t vlo = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(src, static_cast<int>(olo[r])));
        const uint32_t vhi = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(src, static_cast<int>(ohi[r])));
        const uint32_t vsz = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(src, static_cast<int>(sz[r])));
        if ((q >> 6) == r) {
          lo = vlo;
          hi = vhi;
          size = vsz;
        }
      }
      if (j < cnt) {
        const uint64_t i = w0 + q;
        const uint64_t off = (static_cast<uint64_t>(hi) << 32) | lo;
        const bool valid = desc_in_range<kModeRaw>(a, Desc{off, size, 0, 0});
        const uint32_t init = a.init_crcs ? a.init_crcs[i] : 0u;
        uint32_t v = 0;
        if (valid) {
          const uint32_t crc = lane_raw_crc(Lb, K, a.base, a.base_len, off, size, init,
                                            a.init_crcs != nullptr);
          v = a.wal_hs ? crc_mask(crc) : crc;
        }
        const bool differs = !a.expect || !valid || v != a.expect[i];
        if (differs && a.out32) a.out32[i] = v;
      }
    }
    wave_lds_sync();  // (the slots are rewritten by the next window)
  }
}

// One wave per block, no streaming: serves buffers shorter than one 4 KiB
// round (the streaming kernels' dummy loads need that much).
template <int MODE>
__global__ void __launch_bounds__(kThreads)
    crc32c_block_kernel_simple(BlockArgs a) {
  __shared__ uint32_t L[kLdsDwords];
  fill_tables(L);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = uniform(threadIdx.x >> 6);
  const uint32_t lb = (lane & 31) << 2;
  const uint64_t lo = reinterpret_cast<uint64_t>(a.base);
  const uint64_t nw = static_cast<uint64_t>(gridDim.x) * kWaves;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWaves + wave; i < a.n;
       i += nw) {
    const uint64_t off = a.offsets[i];
    const uint32_t size = a.sizes[i];
    const uint8_t* p = a.base + off;
    uint64_t need = size;
    if (MODE == kModeVerify || MODE == kModeTrailer) need += 5;
    if (MODE == kModeCompute && a.last_bytes == nullptr) need += 1;
    const bool inb = off <= a.base_len && need <= a.base_len - off;
    if (!inb) {  // descriptor outside the buffer: report, never read
      if (lane == 0) {
        if (a.out32) a.out32[i] = 0;
        if (MODE == kModeVerify) {
          if (a.ok_out) a.ok_out[i] = 0;
          if (a.stored_out) a.stored_out[i] = 0;
          if (a.mismatches) atomicAdd(a.mismatches, 1ull);
        }
      }
      continue;
    }
    if (MODE == kModeRaw) {
      const uint32_t init = a.init_crcs ? a.init_crcs[i] : 0u;
      const uint32_t c = wave_crc32c(L, lane, lb, p, size, init, 0, 0, lo);
      if (lane == 0) a.out32[i] = c;
    } else if (MODE == kModeVerify) {
      // reader_common.cc:36-47
      const uint32_t computed =
          crc_mask(wave_crc32c(L, lane, lb, p, uint64_t(size) + 1, 0, 0, 0, lo));
      const uint32_t mod = a.modifiers ? a.modifiers[i] : 0u;
      const uint32_t stored = ldu32(p + size + 1) - mod;
      const bool ok = stored == computed;
      if (lane == 0) {
        if (a.out32) a.out32[i] = computed;
        if (a.stored_out) a.stored_out[i] = stored;
        if (a.ok_out) a.ok_out[i] = ok ? 1 : 0;
        if (!ok && a.mismatches) atomicAdd(a.mismatches, 1ull);
      }
    } else {
      // format.cc:594-600 + builder.cc:1340-1345
      const uint32_t last = a.last_bytes ? a.last_bytes[i] : ldu8(p + size);
      const uint32_t mod = a.modifiers ? a.modifiers[i] : 0u;
      const uint32_t c =
          crc_mask(wave_crc32c(L, lane, lb, p, size, 0, 1, last, lo)) + mod;
      if (lane == 0) {
        if (a.out32) a.out32[i] = c;
        if (MODE == kModeTrailer) {
          uint8_t* q = a.base_w + off + size;
          q[0] = static_cast<uint8_t>(last);
          stu32_bytes(q + 1, c);
        }
      }
    }
  }
}

}  // namespace

namespace {

enum class CrcKernel {
  kSimple,  // one wave per block: buffers shorter than one 4 KiB round
  kRows,    // one block per 16-lane row (crc32c_rows_kernel)
};

hipError_t launch_kernel(void (*k)(BlockArgs), uint32_t grid, uint32_t threads, BlockArgs a,
                         hipStream_t s) {
  hipLaunchKernelGGL(k, dim3(grid), dim3(threads), 0, s, a);
  return hipGetLastError();
}

const char* crc_kernel_name(CrcKernel k, int mode) {
  static const char* const kNames[][4] = {
      {"crc32c_block_kernel_simple<compute>", "crc32c_block_kernel_simple<trailer>",
       "crc32c_block_kernel_simple<verify>", "crc32c_block_kernel_simple<raw>"},
      {"crc32c_rows_kernel<compute>", "crc32c_rows_kernel<trailer>", "crc32c_rows_kernel<verify>",
       "crc32c_rows_kernel<raw>"},
  };
  return kNames[static_cast<int>(k)][mode & 3];
}

#ifndef FORST_CRC_BLOCK_COST
#define FORST_CRC_BLOCK_COST 0
#endif
template <int M>
hipError_t launch_crc_mode(CrcKernel k, const BlockArgs& a, uint32_t grid, hipStream_t s) {
  switch (k) {
    case CrcKernel::kSimple:
      return launch_kernel(crc32c_block_kernel_simple<M>, grid, kThreads, a, s);
    case CrcKernel::kRows:
      // block modes: the workgroup feed (stream_common.h), no ticket counter
      // (if constexpr: raw batches never launch crc32c_rows_kernel<raw>, so it
      // is not instantiated)
      if constexpr (M != kModeRaw) {
        BlockArgs b = a;
        b.wg_cost = FORST_CRC_BLOCK_COST;  // (stream_common.h wg_range)
        return launch_kernel(crc32c_rows_kernel<M>, grid, 64 * kWaves, b, s);
      } else {
        if (a.n < uint64_t(64) * grid * kWaves)
          return launch_kernel(crc32c_rows_raw_small_kernel, grid, 64 * kWaves, a, s);
        // short messages one per lane, then the rows kernel over the rest
        const hipError_t e = launch_kernel(crc32c_raw_lane_kernel, 2 * device_info().num_cus,
                                           kLaneThreads, a, s);
        if (e != hipSuccess) return e;
        return launch_fed(crc32c_rows_raw_filt_kernel, grid, kWaves, a, s);
      }
  }
  return hipErrorInvalidValue;
}

// one launch over a batch of at most FORST_ROWS_MAX_DESCS descriptors
hipError_t launch_crc32c_slice(int mode, const BlockArgs& a, hipStream_t stream,
                               const char** name) {
  const DeviceInfo& di = device_info();
  uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((a.n + kWaves - 1) / kWaves, di.num_cus));
  if (grid == 0) grid = 1;
#ifdef FORST_DEBUG_BOUNDS
  {
    DbgState st{};
    st.lo = reinterpret_cast<uint64_t>(a.base);
    st.hi = st.lo + a.base_len;
    hipError_t e = hipMemcpyToSymbolAsync(HIP_SYMBOL(g_forst_dbg), &st, sizeof(st), 0,
                                          hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
  }
#endif
  // The rows kernel (one block per 16-lane row) for every block size (a
  // one-block-per-wave kernel with two 4 KiB steps in flight won above
  // 8-20 KiB in round 1 and lost everywhere once the rows kernel had the
  // workgroup feed: DESIGN.md 4.1b).  Buffers shorter than one 4 KiB round
  // take the simple kernel (the streaming kernels' dummy loads read the
  // buffer's first KiBs).
  const CrcKernel k = a.base_len < kRB ? CrcKernel::kSimple : CrcKernel::kRows;
  // the WAL writer mode (wal_hs: header offsets + payload lengths, masked
  // output) exists in the rows kernel only
  if (a.wal_hs && (mode != kModeRaw || k != CrcKernel::kRows)) return hipErrorInvalidValue;
  *name = crc_kernel_name(k, mode);
  if (k == CrcKernel::kRows && mode == kModeRaw)
    *name = a.n < uint64_t(64) * grid * kWaves ? "crc32c_rows_raw_small_kernel"
                                               : "crc32c_rows_raw_filt_kernel";
  switch (mode) {
    case kModeCompute:
      return launch_crc_mode<kModeCompute>(k, a, grid, stream);
    case kModeTrailer:
      return launch_crc_mode<kModeTrailer>(k, a, grid, stream);
    case kModeVerify:
      return launch_crc_mode<kModeVerify>(k, a, grid, stream);
    default:
      return launch_crc_mode<kModeRaw>(k, a, grid, stream);
  }
}

}  // namespace

// raw CRCs of messages all under kRawSplit bytes: the lane kernel alone (a
// longer one would be left out: the caller guarantees the lengths)
hipError_t launch_crc32c_raw_lanes(const BlockArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  return launch_kernel(crc32c_raw_lane_kernel, 2 * device_info().num_cus, kLaneThreads, a, stream);
}

hipError_t launch_crc32c_blocks(int mode, const BlockArgs& a, hipStream_t stream,
                                const char** name) {
  // (one launch unless the batch is longer than a rows launch can index)
  for (uint64_t first = 0; first < a.n; first += FORST_ROWS_MAX_DESCS) {
    const BlockArgs b = slice_descs(a, first, std::min<uint64_t>(a.n - first, FORST_ROWS_MAX_DESCS));
    const hipError_t e = launch_crc32c_slice(mode, b, stream, name);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace forst

#ifdef FORST_DEBUG_BOUNDS
// diagnostics build only: first out-of-bounds access recorded by the CRC
// kernels since the last launch (line, offset from base, width, count)
extern "C" __attribute__((visibility("default"))) int forst_debug_fetch(unsigned long long* out) {
  forst::DbgState st{};
  if (hipMemcpyFromSymbol(&st, HIP_SYMBOL(forst::g_forst_dbg), sizeof(st)) != hipSuccess)
    return -3;
  for (int k = 0; k < 4; ++k) out[k] = st.rec[k];
  return 0;
}
#endif
