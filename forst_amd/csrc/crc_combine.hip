// forst_amd/csrc/crc_combine.hip -- crc32c::Crc32cCombine (util/crc32c.cc:1279)
// and whole-buffer CRC32C on the device.
//
// CRC32C with its pre/post conditioning is affine, and the conditioning
// cancels in the combine identity
//     crc(A || B) = M(|B|) * crc(A) ^ crc(B),   M(n) = x^(8n) mod P
// (GF(2) product in the reflected domain; the reference computes the same
// thing with gf_multiply_sw over crc32c_powers, crc32c.cc:1143-1279).  Folding
// it over chunks gives the parallel form used here:
//     Extend(init, C_0 || ... || C_{k-1})
//         = M(total) * init  ^  XOR_i M(after_i) * Value(C_i)
// so a whole buffer is one raw batch over 64 KiB chunks (the block kernels,
// at streaming rate) plus one lane per chunk shifting its CRC to the end of
// the buffer and an XOR reduction -- used by FileChecksumGenCrc32c
// (util/file_checksum_helper.h:22) and the WritableFileWriter handoff CRC
// (file/writable_file_writer.cc:100-212) style chained CRCs.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/forst_checksum.h"
#include "crc32c_tables.h"
#include "device_common.h"
#include "engine.h"

namespace forst {
namespace {

constexpr uint32_t kPoly = 0x82f63b78u;  // util/crc32c.cc (reflected Castagnoli)
constexpr uint32_t kCombThreads = 256;
constexpr uint64_t kChunk = 65536;

// a * b mod P, reflected (bit 31 = x^0)
__host__ __device__ inline uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= (a & 0x80000000u) ? b : 0u;
    a <<= 1;
    b = (b >> 1) ^ ((b & 1u) ? kPoly : 0u);
  }
  return p;
}

// M(n) = x^(8n) mod P from the powers x^(8 * 2^k) (kCrcX8Pow)
__device__ inline uint32_t x8n_dev(uint64_t n) {
  uint32_t r = 0x80000000u;  // x^0
  for (int k = 0; n; ++k, n >>= 1)
    if (n & 1) r = gf_mul(r, kCrcX8Pow[k]);
  return r;
}

inline uint32_t x8n_host(uint64_t n) {
  uint32_t r = 0x80000000u, sq = 0x00800000u;  // x^0, x^8
  for (; n; n >>= 1) {
    if (n & 1) r = gf_mul(r, sq);
    sq = gf_mul(sq, sq);
  }
  return r;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
  for (int m = 32; m >= 1; m >>= 1) v ^= __shfl_xor(v, m);
  return v;
}

__global__ void __launch_bounds__(kCombThreads)
    combine_batch_kernel(const uint32_t* crc1, const uint32_t* crc2, const uint64_t* len2,
                         uint32_t* out, uint64_t n) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kCombThreads + threadIdx.x;
  if (i < n) out[i] = gf_mul(x8n_dev(len2[i]), crc1[i]) ^ crc2[i];
}

__global__ void __launch_bounds__(kCombThreads)
    chunk_desc_kernel(uint64_t len, uint64_t n_chunks, uint64_t* offs, uint32_t* sizes) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kCombThreads + threadIdx.x;
  if (i >= n_chunks) return;
  offs[i] = i * kChunk;
  sizes[i] = static_cast<uint32_t>(i + 1 < n_chunks ? kChunk : len - i * kChunk);
}

// out ^= XOR_i M(after_i) * crc_i (+ M(total) * init from lane 0 of block 0);
// *out is zeroed on the stream before the launch
__global__ void __launch_bounds__(kCombThreads)
    chunk_fold_kernel(const uint32_t* crcs, uint64_t len, uint64_t n_chunks, uint32_t init,
                      uint32_t* out) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kCombThreads + threadIdx.x;
  uint32_t v = 0;
  if (i < n_chunks) {
    const uint64_t end = i + 1 < n_chunks ? (i + 1) * kChunk : len;
    v = gf_mul(x8n_dev(len - end), crcs[i]);
  }
  if (i == 0) v ^= gf_mul(x8n_dev(len), init);
  v = wave_xor(v);
  if ((threadIdx.x & 63) == 0 && v) atomicXor(out, v);
}

// ---- whole-file CRC32C over a set of buffers (forst_crc32c_files) ------------
// Every file is cut into 64 KiB chunks under ONE global chunk index; pre[f] =
// chunks before file f (pre[n] = all of them), built on the host.  A chunk's
// file is the last f with pre[f] <= chunk (files without chunks share their
// successor's entry and are never found: their result is the init term alone).
__device__ inline uint64_t file_of_chunk(const uint64_t* pre, uint64_t n_files, uint64_t c) {
  uint64_t lo = 0, hi = n_files;  // pre[lo] <= c < pre[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (pre[mid] <= c) lo = mid; else hi = mid;
  }
  return lo;
}

// chunk c -> (offset from the 4-byte aligned base, size); file f -> its
// init term M(length) * init, stored (not XORed), so `out` needs no memset and
// a stale value never survives.  One thread per max(chunks, files).
__global__ void __launch_bounds__(kCombThreads)
    files_desc_kernel(const uint64_t* pre, const uint64_t* foffs, const uint64_t* flens,
                      const uint32_t* inits, uint64_t n_files, uint64_t n_chunks, uint64_t delta,
                      uint64_t* offs, uint32_t* sizes, uint32_t* out) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kCombThreads + threadIdx.x;
  if (i < n_files) out[i] = inits ? gf_mul(x8n_dev(flens[i]), inits[i]) : 0u;
  if (i >= n_chunks) return;
  const uint64_t f = file_of_chunk(pre, n_files, i);
  const uint64_t at = (i - pre[f]) * kChunk, left = flens[f] - at;
  offs[i] = delta + foffs[f] + at;
  sizes[i] = static_cast<uint32_t>(left < kChunk ? left : kChunk);
}

// One lane per chunk: its CRC shifted to the end of its own file, lanes of the
// same file XOR-reduced inside the wave (a segmented reduction: files are runs
// of consecutive lanes), one atomicXor per (wave, file) from the run's first
// lane.  A wave inside one long file issues one atomic; a wave of 64
// one-chunk files issues 64.
__global__ void __launch_bounds__(kCombThreads)
    files_fold_kernel(const uint32_t* crcs, const uint64_t* pre, const uint64_t* flens,
                      uint64_t n_files, uint64_t n_chunks, uint32_t* out) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kCombThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  uint64_t f = ~uint64_t(0);  // lanes past the last chunk: a run of their own
  uint32_t v = 0;
  if (i < n_chunks) {
    f = file_of_chunk(pre, n_files, i);
    const uint64_t end = (i - pre[f] + 1) * kChunk, len = flens[f];
    v = gf_mul(x8n_dev(end < len ? len - end : 0), crcs[i]);
  }
  const uint32_t flo = static_cast<uint32_t>(f), fhi = static_cast<uint32_t>(f >> 32);
  // every lane takes part in every shuffle (no early exit above)
  const int prev = lane ? static_cast<int>(lane) - 1 : 0;
  const uint32_t plo = __shfl(flo, prev), phi = __shfl(fhi, prev);
  const bool head = lane == 0 || plo != flo || phi != fhi;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const int src = static_cast<int>(lane + d < 64 ? lane + d : 63);
    const uint32_t ov = __shfl(v, src), olo = __shfl(flo, src), ohi = __shfl(fhi, src);
    // after this step v covers lanes [lane, lane + 2d) of this lane's run
    if (lane + d < 64 && olo == flo && ohi == fhi) v ^= ov;
  }
  if (head && i < n_chunks && v) atomicXor(out + f, v);
}

}  // namespace

hipError_t launch_crc32c_combine_batch(const uint32_t* crc1, const uint32_t* crc2,
                                       const uint64_t* len2, uint32_t* out, uint64_t n,
                                       hipStream_t stream, const char** name) {
  if (n == 0) return hipSuccess;
  *name = "combine_batch_kernel";
  hipLaunchKernelGGL(combine_batch_kernel, dim3(static_cast<uint32_t>((n + kCombThreads - 1) / kCombThreads)),
                     dim3(kCombThreads), 0, stream, crc1, crc2, len2, out, n);
  return hipGetLastError();
}

hipError_t launch_crc32c_buffer(const uint8_t* base, uint64_t len, uint32_t init, uint32_t* out,
                                hipStream_t stream, const char** name) {
  hipError_t e = hipMemsetAsync(out, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  const uint64_t nc = (len + kChunk - 1) / kChunk;
  const dim3 grid(static_cast<uint32_t>(nc ? (nc + kCombThreads - 1) / kCombThreads : 1));
  if (nc == 0) {  // Extend(init, "") = init
    hipLaunchKernelGGL(chunk_fold_kernel, grid, dim3(kCombThreads), 0, stream, nullptr,
                       uint64_t(0), uint64_t(0), init, out);
    *name = "chunk_fold_kernel";
    return hipGetLastError();
  }
  void* scratch = nullptr;
  const size_t so = (8 * nc + 255) & ~size_t(255), ss = (4 * nc + 255) & ~size_t(255);
  if ((e = scratch_alloc(&scratch, so + 2 * ss, stream)) != hipSuccess) return e;
  uint64_t* offs = static_cast<uint64_t*>(scratch);
  uint32_t* sizes = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(scratch) + so);
  uint32_t* crcs = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(scratch) + so + ss);
  hipLaunchKernelGGL(chunk_desc_kernel, grid, dim3(kCombThreads), 0, stream, len, nc, offs, sizes);
  BlockArgs b{};
  b.base = base;
  b.base_len = len;
  b.offsets = offs;
  b.sizes = sizes;
  b.out32 = crcs;
  b.n = nc;
  e = launch_crc32c_blocks(kModeRaw, b, stream, name);
  hipLaunchKernelGGL(chunk_fold_kernel, grid, dim3(kCombThreads), 0, stream, crcs, len, nc, init,
                     out);
  if (e == hipSuccess) e = hipGetLastError();
  const hipError_t f = scratch_free(scratch, stream);
  return e != hipSuccess ? e : f;
}

hipError_t launch_crc32c_files(const uint8_t* arena, uint64_t arena_len, const uint64_t* offsets,
                               const uint64_t* lengths, const uint32_t* inits, uint32_t* out,
                               uint64_t n_files, hipStream_t stream, const char** name) {
  if (n_files == 0) return hipSuccess;
  // host block [pre (n + 1) | offsets n | lengths n | inits n], one upload
  const uint64_t words = 3 * n_files + 1;
  std::vector<uint64_t> host(words + (inits ? (n_files + 1) / 2 : 0));
  uint64_t* pre = host.data();
  pre[0] = 0;
  for (uint64_t f = 0; f < n_files; ++f) pre[f + 1] = pre[f] + (lengths[f] + kChunk - 1) / kChunk;
  std::memcpy(pre + n_files + 1, offsets, 8 * n_files);
  std::memcpy(pre + 2 * n_files + 1, lengths, 8 * n_files);
  if (inits) std::memcpy(pre + words, inits, 4 * n_files);
  const uint64_t nc = pre[n_files];
  const size_t sh = (8 * host.size() + 255) & ~size_t(255);
  const size_t so = (8 * nc + 255) & ~size_t(255), ss = (4 * nc + 255) & ~size_t(255);
  void* scratch = nullptr;
  hipError_t e = scratch_alloc(&scratch, sh + so + 2 * ss, stream);
  if (e != hipSuccess) return e;
  uint8_t* sc = static_cast<uint8_t*>(scratch);
  const uint64_t* d_pre = reinterpret_cast<const uint64_t*>(sc);
  const uint64_t* d_foffs = d_pre + n_files + 1;
  const uint64_t* d_flens = d_foffs + n_files;
  const uint32_t* d_inits = inits ? reinterpret_cast<const uint32_t*>(d_pre + words) : nullptr;
  uint64_t* offs = reinterpret_cast<uint64_t*>(sc + sh);
  uint32_t* sizes = reinterpret_cast<uint32_t*>(sc + sh + so);
  uint32_t* crcs = reinterpret_cast<uint32_t*>(sc + sh + so + ss);
  // (pageable source: the copy has left `host` when hipMemcpyAsync returns)
  e = hipMemcpyAsync(scratch, host.data(), 8 * host.size(), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) {
    // the block kernels want a 4-byte aligned base: step back to one, the
    // chunk offsets carry the difference
    const uint64_t delta = reinterpret_cast<uintptr_t>(arena) & 3;
    const uint64_t nt = nc > n_files ? nc : n_files;
    *name = "files_desc_kernel";
    hipLaunchKernelGGL(files_desc_kernel, dim3(static_cast<uint32_t>((nt + kCombThreads - 1) / kCombThreads)),
                       dim3(kCombThreads), 0, stream, d_pre, d_foffs, d_flens, d_inits, n_files, nc,
                       delta, offs, sizes, out);
    if (nc) {
      BlockArgs b{};
      b.base = arena - delta;
      b.base_len = arena_len + delta;
      b.offsets = offs;
      b.sizes = sizes;
      b.out32 = crcs;
      b.n = nc;
      e = launch_crc32c_blocks(kModeRaw, b, stream, name);
      if (e == hipSuccess) {
        *name = "files_fold_kernel";
        hipLaunchKernelGGL(files_fold_kernel, dim3(static_cast<uint32_t>((nc + kCombThreads - 1) / kCombThreads)),
                           dim3(kCombThreads), 0, stream, crcs, d_pre, d_flens, n_files, nc, out);
      }
    }
    if (e == hipSuccess) e = hipGetLastError();
  }
  const hipError_t f = scratch_free(scratch, stream);
  return e != hipSuccess ? e : f;
}

}  // namespace forst

// host: crc32c::Crc32cCombine (util/crc32c.h:32), no GPU involved
extern "C" __attribute__((visibility("default"))) uint32_t forst_crc32c_combine(uint32_t crc1,
                                                                                uint32_t crc2,
                                                                                uint64_t len2) {
  return forst::gf_mul(forst::x8n_host(len2), crc1) ^ crc2;
}
