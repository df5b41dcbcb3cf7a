"""tests/dispatch.py -- TEST INFRASTRUCTURE ONLY: host restatements of the
engine's kernel-dispatch rules, and builders of inputs that reach the
large-batch code paths at the smallest sizes that do.

The kernels choose their path from the batch (descriptor count, buffer
length, bytes per workgroup range) and several thresholds scale with the
number of compute units, so every builder takes the CU count: the GPU tests
(tests/test_gpu_paths.py) pass the device's, tests/test_dispatch_cpu.py passes
256 and 304 and checks the preconditions without a GPU.  Each rule quotes the
launch line it mirrors.

Two grids contain a kernel's occupancy (hipOccupancyMaxActiveBlocksPer-
Multiprocessor), which a test cannot query.  Read from a kernel trace
(rocprofv3 --kernel-trace, Grid_Size_X / Workgroup_Size_X) of these batches on
an MI355X with 256 CUs:
  xxh3_rows_kernel<raw>                      196608 / 768 = 256 workgroups:
                     1 per CU.  XX_RAW_OCCUPANCY sizes the raw batch for 2 (a
                     smaller grid only lowers the threshold of the static
                     shares, n >= 128 * 12 * grid).
  xxh3_rows_kernel<compute|trailer|verify>   196608 / 768 = 256 workgroups:
                     1 per CU (66.5 / 99 / 83 KiB of LDS), XX_BLOCK_OCCUPANCY.
  (crc32c_rows_kernel<*>, crc32c_rows_raw_filt_kernel: 262144 / 1024 = 256,
   the CU count, as crc_grid restates; crc32c_raw_lane_kernel 2 per CU.)
"""
import numpy as np

# ---- constants of the launch code -----------------------------------------
CRC_WAVES = 16           # crc32c.hip: constexpr uint32_t kWaves = 16;
XX_ROWS_WAVES = 12       # xxh3.hip: constexpr uint32_t kRowsWaves = 12;
RAW_SPLIT = 256          # crc32c.hip: kRawSplit
CRC_STAGE_W = 6144       # crc32c.hip: constexpr uint32_t kStageW = 6144;
XX_STAGE_W = 16384       # xxh3.hip: constexpr uint32_t kXxStageW = 16384;
CRC_BLOCK_COST = 0       # crc32c.hip: #define FORST_CRC_BLOCK_COST 0
XX_BLOCK_COST = 256      # xxh3.hip: #define FORST_XX_BLOCK_COST 256
SIMPLE_BELOW = 4096      # crc32c.hip: a.base_len < kRB ? CrcKernel::kSimple; xxh3.hip: a.base_len < 4096
LOG_BLOCK = 32768        # db/log_format.h:45
WAL_TILE = 256           # wal.hip: log blocks per workgroup of wal_fill_kernel (kTile)
WAL_FILL_CAP = 2560      # wal.hip: constexpr uint32_t kFillCap = 2560;
XX_RAW_OCCUPANCY = 2
XX_BLOCK_OCCUPANCY = 1

SENTINEL32 = 0x5A5A5A5A  # prefill of every result array handed to the engine
SENTINEL8 = 0xA5


# ---- dispatch rules ---------------------------------------------------------

def crc_grid(n, num_cus):
    """crc32c.hip launch_crc32c_slice (per launch of launch_crc32c_blocks):
    grid = min((a.n + kWaves - 1) / kWaves, di.num_cus); if (grid == 0) grid = 1;"""
    return max(1, min((n + CRC_WAVES - 1) // CRC_WAVES, num_cus))


def crc_raw_kernel(n, base_len, num_cus):
    """crc32c.hip launch_crc32c_slice / launch_crc_mode<kModeRaw>:
    k = a.base_len < kRB ? CrcKernel::kSimple : CrcKernel::kRows;
    if (a.n < uint64_t(64) * grid * kWaves) crc32c_rows_raw_small_kernel
    else crc32c_raw_lane_kernel + launch_fed(crc32c_rows_raw_filt_kernel)"""
    if base_len < SIMPLE_BELOW:
        return "crc32c_block_kernel_simple<raw>"
    if n < 64 * crc_grid(n, num_cus) * CRC_WAVES:
        return "crc32c_rows_raw_small_kernel"
    return "crc32c_rows_raw_filt_kernel"


def feed_share1(n, nw):
    """capi.hip feed_setup: a.share1 = a.n / (2 * 64 * nw) * 64;  (nw = grid * waves)"""
    return n // (2 * 64 * nw) * 64


def xx_rows_grid(n, num_cus, occupancy):
    """xxh3.hip launch_xxh3_mode kRows:
    grid = max(1, min((a.n + 4 * kRowsWaves - 1) / (4 * kRowsWaves),
                      num_cus * rows_occupancy<M>()))"""
    return max(1, min((n + 4 * XX_ROWS_WAVES - 1) // (4 * XX_ROWS_WAVES), num_cus * occupancy))


def _count_below(offsets, c, t):
    """stream_common.h wg_range: the 64-ary COUNTING search for byte target t
    over the keys offsets[i] + c * i (lane 0 never probes; 63 probes a level)"""
    n = len(offsets)
    lo, ln = 0, n
    lanes = np.arange(64, dtype=np.int64)
    c, t = np.uint64(c), np.uint64(t)
    while ln > 64:
        st = (ln + 63) // 64
        q = lo + lanes * st
        v = (lanes > 0) & (q < lo + ln)
        k = offsets[np.where(v, q, 0)] + c * q.astype(np.uint64)
        cnt = int((v & (k < t)).sum())
        e = lo + ln
        lo += cnt * st
        ln = min(e - lo, st)
    k = offsets[lo:lo + ln] + c * np.arange(lo, lo + ln, dtype=np.int64).astype(np.uint64)
    return lo + int((k < t).sum())


def wg_bounds(offsets, sizes, G, c):
    """stream_common.h wg_range for every workgroup b of a grid of G: range b
    is [L[b], L[b + 1]).  Keys offsets[i] + c * i, split at the G + 1 fraction
    points off0 + floor(span * b / G); L[0] = 0, L[G] = n; by count when there
    is no byte span."""
    offsets = np.ascontiguousarray(offsets).view(np.uint64)
    n = len(offsets)
    off0 = int(offsets[0])
    last = (int(offsets[n - 1]) + int(sizes[n - 1]) + c * (n - 1)) & (2**64 - 1)
    if last <= off0 or G == 1:
        W = (n + G - 1) // G
        return np.minimum(np.arange(G + 1, dtype=np.int64) * W, n)
    span = last - off0
    L = np.zeros(G + 1, np.int64)
    for b in range(1, G):
        t = off0 + (span // G) * b + ((span % G) * b) // G  # frac_point
        L[b] = _count_below(offsets, c, t)
    L[G] = n
    return L


def wal_tile_records(poffs, n_blocks, first_block=0):
    """records per 256-block tile of wal_fill_kernel (tot = the tile's sum of
    s.cnt[]; staged = tot <= kFillCap) for a clean log"""
    per_block = np.bincount((np.asarray(poffs) // LOG_BLOCK).astype(np.int64),
                            minlength=first_block + n_blocks)[first_block:first_block + n_blocks]
    pad = (-len(per_block)) % WAL_TILE
    return np.concatenate([per_block, np.zeros(pad, np.int64)]).reshape(-1, WAL_TILE).sum(axis=1)


# ---- builders ---------------------------------------------------------------

def _pack(sizes, gaps):
    offs = np.zeros(len(sizes), np.uint64)
    offs[1:] = np.cumsum(sizes[:-1].astype(np.uint64) + gaps[:-1].astype(np.uint64))
    return offs


def _bytes(total, seed, fill):
    if not fill:
        return np.zeros(total, np.uint8)
    return np.random.default_rng(seed).integers(0, 256, total, dtype=np.uint8)


STRADDLE = np.arange(RAW_SPLIT - 32, RAW_SPLIT + 32)  # the 64 lengths around the raw split


def raw_crc_batch(num_cus, fill=True, seed=0xC0C):
    """A raw CRC32C batch past the small-batch dispatch AND the static shares
    of the feed: n about 20 % above 128 * 16 * num_cus.  The 64 lengths
    straddling kRawSplit each at all 16 start alignments (16 copies in a
    row, the gap chosen so that the start moves by an odd number of bytes),
    lengths 0..16, the bulk random in 0..600, one message in a thousand
    4 KiB..70 KB, gaps 0..8, a per-message init."""
    rng = np.random.default_rng(seed)
    n = 128 * CRC_WAVES * num_cus * 6 // 5
    sizes = rng.integers(0, 601, n).astype(np.uint32)
    gaps = rng.integers(0, 9, n).astype(np.uint32)
    longs = rng.choice(np.arange(2000, n), n // 1000, replace=False)
    sizes[longs] = rng.integers(4096, 70001, len(longs))
    sizes[:1024] = np.repeat(STRADDLE, 16)
    gaps[:1024] = 1 - (sizes[:1024] & 1)
    sizes[1024:1041] = np.arange(17)
    offs = _pack(sizes, gaps)
    total = int(offs[-1]) + int(sizes[-1]) + 64
    init = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    return dict(n=n, offs=offs, sizes=sizes, init=init, total=total,
                base=_bytes(total, seed + 1, fill))


def raw_edge_descriptors(offs, sizes, total):
    """the out-of-range and end-of-buffer descriptors of
    test_emu_raw_split_short_and_long written over descriptors 5..13 of a raw
    batch: -> (offsets, sizes, indices whose result is 0)"""
    o2, s2 = offs.copy(), sizes.copy()
    o2[5], s2[5] = total - 3, 10                 # short, past the end
    o2[6], s2[6] = total - 100, 600              # long, past the end
    o2[7], s2[7] = 1 << 59, 600                  # long, offset >= 2^58
    o2[8], s2[8] = (1 << 58) - 1, 700            # long, just below 2^58
    o2[9], s2[9] = total - 509, 509              # long, ends at the buffer end
    o2[10], s2[10] = total - 1300, 1300
    o2[11], s2[11] = total - 255, 255            # short, ends at the buffer end
    o2[12], s2[12] = total - 256, 256
    o2[13], s2[13] = total - 77, 77
    return o2, s2, [5, 6, 7, 8]


XXH3_CLASSES = [(0, 0), (1, 3), (4, 8), (9, 16), (17, 128), (129, 240), (241, 600)]


def raw_xxh3_batch(num_cus, fill=True, seed=0x33C):
    """A raw XXH3 batch past the static shares of the feed at a grid of
    XX_RAW_OCCUPANCY workgroups per CU: n about 20 % above
    128 * 12 * num_cus * 2.  Lengths drawn evenly from the seven XXH3 input
    classes, one message in a thousand 4 KiB..70 KB, gaps 0..8 (every class
    at every start alignment)."""
    rng = np.random.default_rng(seed)
    n = 128 * XX_ROWS_WAVES * num_cus * XX_RAW_OCCUPANCY * 6 // 5
    cls = rng.integers(0, len(XXH3_CLASSES), n)
    lo = np.array([c[0] for c in XXH3_CLASSES])[cls]
    hi = np.array([c[1] for c in XXH3_CLASSES])[cls]
    sizes = (lo + rng.integers(0, 1 << 30, n) % (hi - lo + 1)).astype(np.uint32)
    longs = rng.choice(n, n // 1000, replace=False)
    sizes[longs] = rng.integers(4096, 70001, len(longs))
    gaps = rng.integers(0, 9, n).astype(np.uint32)
    offs = _pack(sizes, gaps)
    total = int(offs[-1]) + int(sizes[-1]) + 64
    return dict(n=n, offs=offs, sizes=sizes, total=total, base=_bytes(total, seed + 1, fill))


def xxh3_class(sizes):
    """index into XXH3_CLASSES of each length (the last class is open-ended)"""
    edges = np.array([c[0] for c in XXH3_CLASSES[1:]])
    return np.searchsorted(edges, np.asarray(sizes), side="right")


def dense_wal(num_cus, recyclable, log_number, wal_frame, fill=True, seed=0xA1):
    """One log image in three parts: logical records of 0..200 bytes (at least
    300 log blocks, and more physical records than 64 * 16 * num_cus; about
    300 records per block, so a 256-block tile far exceeds kFillCap), then at
    least 300 blocks of the log-uniform 32..32768 B mix (about 7 records per
    block: staged tiles), then a short last block.  The dense part is sized so
    that it ends in the middle half of a tile: one tile holds blocks of both
    regimes.  wal_frame: oracle.wal_frame.
    -> dict(buf, poffs, plens, n_dense (physical records of the dense part),
            boundary_block (the block of the first sparse record), n_blocks)"""
    rng = np.random.default_rng(seed + int(recyclable))
    hs = 11 if recyclable else 7
    n_dense = max(64 * CRC_WAVES * num_cus * 11 // 10, 300 * LOG_BLOCK // (100 + hs))
    dense = rng.integers(0, 201, n_dense + 2 * WAL_TILE * 330).astype(np.uint32)
    sparse = np.exp(rng.uniform(np.log(32), np.log(32768), 300 * 9)).astype(np.uint32)
    for _ in range(4):
        lens = np.concatenate([dense[:n_dense], sparse])
        lens[n_dense - 1] = 100  # (not empty: its last fragment has payload)
        payload = _bytes(int(lens.astype(np.int64).sum()), seed + 7, fill)
        buf, poffs, plens = wal_frame(payload, lens, recyclable=recyclable, log_number=log_number)
        # the first sparse record's first fragment: the first physical record
        # with all the dense payload bytes in front of it
        before = np.cumsum(plens.astype(np.int64)) - plens
        first_sparse = int(np.searchsorted(before, int(lens[:n_dense].astype(np.int64).sum())))
        boundary = int(poffs[first_sparse]) // LOG_BLOCK
        r = boundary % WAL_TILE
        if WAL_TILE // 4 <= r < 3 * WAL_TILE // 4:
            break
        n_dense += ((WAL_TILE // 2 - r) % WAL_TILE) * first_sparse // boundary
    else:
        raise AssertionError("the dense part never ended inside a tile")
    # one more record that ends 1000 bytes into a block of its own: a short last block
    left = LOG_BLOCK - len(buf) % LOG_BLOCK
    lens = np.concatenate([lens, [1000 + (left - hs if left >= hs else 0)]]).astype(np.uint32)
    payload = _bytes(int(lens.astype(np.int64).sum()), seed + 7, fill)
    buf, poffs, plens = wal_frame(payload, lens, recyclable=recyclable, log_number=log_number)
    return dict(buf=buf, poffs=poffs, plens=plens, n_dense=first_sparse, boundary_block=boundary,
                n_blocks=(len(buf) + LOG_BLOCK - 1) // LOG_BLOCK)


def wal_faults(w, log_number):
    """the log of dense_wal with faults in blocks of dense tiles, of sparse
    tiles and of the mixed tile: payload flips in the first and the last
    record of a block, a length past the block, a zeroed header, an older log
    number (recyclable).  -> (buffer, the blocks hit, ascending)"""
    buf, poffs, plens = w["buf"].copy(), w["poffs"].astype(np.int64), w["plens"]
    rec_hdr = bool(w["recyclable"])
    hs = 11 if rec_hdr else 7
    blk = poffs // LOG_BLOCK
    bb, nb = w["boundary_block"], w["n_blocks"]

    def rec(block, which):  # the first / last / a middle record of a block
        ks = np.nonzero(blk == block)[0]
        return int({"first": ks[0], "last": ks[-1], "mid": ks[len(ks) // 2]}[which])

    hit = []
    flips = [(3, "first"), (200, "last"), (bb - 20, "first"), (bb - 10, "last"),       # dense
             (bb + 5, "first"), (bb + 6, "last"),                                      # mixed tile
             (nb - 200, "first"), (nb - 100, "last"), (nb - 3, "last")]                # sparse
    for block, which in flips:
        k = rec(block, which)
        if plens[k]:
            buf[poffs[k] + hs + (int(plens[k]) - 1 if which == "last" else 0)] ^= 0x40
        else:  # an empty record: its type byte is covered by the CRC too
            buf[poffs[k] + 6] ^= 0x10
        hit.append(block)
    for block in (100, nb - 50):  # a length past the block
        k = rec(block, "mid")
        buf[poffs[k] + 4:poffs[k] + 6] = 0xFF
        hit.append(block)
    for block in (150, nb - 60):  # a zeroed header: the reader takes it for padding
        k = rec(block, "mid")
        buf[poffs[k]:poffs[k] + hs] = 0
        hit.append(block)
    if rec_hdr:  # a record left over from an older log
        for block in (170, nb - 70):
            k = rec(block, "mid")
            buf[poffs[k] + 7:poffs[k] + 11] = np.frombuffer(
                int(log_number - 1).to_bytes(4, "little"), np.uint8)
            hit.append(block)
    assert len(set(hit)) == len(hit) and bb > 220 and nb - bb > 220
    return buf, sorted(hit)


SMALL_MAX = 130  # the small blocks of the clustered batch: every size 0..130


def clustered_batch(stage_w, cost, G, large):
    """Descriptors in file order whose FIRST byte-balanced workgroup range
    (wg_bounds) is longer than the rows kernels' result stage: stage_w filler
    blocks of 0..24 bytes packed with their 5-byte trailers (starts walk every
    alignment), then every size 0..SMALL_MAX at every start alignment mod 16
    (up to 15 bytes of padding in front of a block), then as many blocks of
    `large` bytes as put the first of the G + 1 split points behind the small
    run.  -> (offsets u64, sizes u32, total bytes, n_small)"""
    filler = (np.arange(stage_w) * 7 % 25).astype(np.int64)
    sizes, offs, pos = [], [], 0
    for s in filler:
        offs.append(pos)
        sizes.append(int(s))
        pos += int(s) + 5
    for s in range(SMALL_MAX + 1):
        for a in range(16):
            pos += (a - pos) % 16
            offs.append(pos)
            sizes.append(s)
            pos += s + 5
    n_small = len(sizes)
    key_end = pos + cost * n_small  # key of the first large block
    n_large = (G * (key_end + 4 * (large + 5 + cost))) // (large + 5 + cost) + 1
    lo = pos + (large + 5) * np.arange(n_large, dtype=np.int64)
    offs = np.concatenate([np.array(offs, np.int64), lo]).astype(np.uint64)
    sizes = np.concatenate([np.array(sizes, np.int64), np.full(n_large, large)]).astype(np.uint32)
    total = int(offs[-1]) + large + 5
    return offs, sizes, total, n_small


def crc_clustered(num_cus):
    """the CRC32C rows kernels' clustered batch: 16 KiB large blocks; its grid
    is capped at the CU count (crc_grid)"""
    return clustered_batch(CRC_STAGE_W, CRC_BLOCK_COST, num_cus, 16384)


def xxh3_clustered(num_cus):
    """the XXH3 rows kernel's: 64 KiB large blocks, grid num_cus *
    XX_BLOCK_OCCUPANCY"""
    return clustered_batch(XX_STAGE_W, XX_BLOCK_COST, num_cus * XX_BLOCK_OCCUPANCY, 65536)


def direct_part(offs, sizes, G, cost, stage_w):
    """-> (L, b, idx): the ranges, the longest one, and the descriptor indices
    past position stage_w of it (stored directly, not through LDS)"""
    L = wg_bounds(offs, sizes, G, cost)
    b = int(np.argmax(np.diff(L)))
    return L, b, np.arange(L[b] + stage_w, L[b + 1])


def covers_small_sizes(offs, sizes, idx):
    """every size 0..SMALL_MAX at every start alignment among descriptors idx"""
    have = set(zip(sizes[idx].tolist(), (offs[idx] & np.uint64(15)).tolist()))
    return all((s, a) in have for s in range(SMALL_MAX + 1) for a in range(16))


def verify_faults(offs, sizes, total, G, cost, stage_w, seed=9):
    """victims for the verify pass over a clustered batch: blocks to corrupt
    in the staged part and the direct part of the long range and in other
    ranges, and 7 descriptors (3 staged, 4 direct) replaced by out-of-range
    ones (past the end by offset, by size, offsets of 2^58 and more).  The
    ranges are those of the CHANGED descriptor array.
    -> dict(staged, direct, other (indices, the first 3 / 4 of staged / direct
    are the out-of-range ones), offs, sizes, L, b)"""
    n = len(offs)
    L0, b0, dpart0 = direct_part(offs, sizes, G, cost, stage_w)
    rng = np.random.default_rng(seed)
    staged = int(L0[b0]) + rng.choice(stage_w, 24, replace=False)
    direct = rng.choice(dpart0, 40, replace=False)
    other = rng.choice(np.arange(int(L0[b0 + 1]), n), 24, replace=False)
    o2, s2 = offs.copy(), sizes.copy()
    oor = np.concatenate([staged[:3], direct[:4]])
    o2[oor] = np.array([total - 3, total + 9, 1 << 59, total - 4, total + 1, 1 << 60,
                        (1 << 58) - 1], np.uint64)
    s2[oor] = [0, 5, 100, 70000, 0, 130, 64]
    L, b, dpart = direct_part(o2, s2, G, cost, stage_w)
    assert L[b + 1] - L[b] > stage_w
    assert np.isin(direct, dpart).all() and np.isin(other, np.arange(L[b + 1], n)).all()
    assert ((staged >= L[b]) & (staged < L[b] + stage_w)).all()
    return dict(staged=staged, direct=direct, other=other, offs=o2, sizes=s2, L=L, b=b)


def small_buffers(seed=0x51):
    """buffers shorter than 4 KiB (the *_simple / group kernels): blocks with
    5-byte trailers, every size 0..200 at every start alignment mod 16 and a
    few up to 4000, in random order, plus one block filling a buffer of
    exactly 4095, 4096 and 4097 bytes (either side of the dispatch boundary).
    -> [(buffer length, offsets u64, sizes u32)]"""
    rng = np.random.default_rng(seed)
    want = [(s, a) for s in range(201) for a in range(16)]
    want += [(s, int(rng.integers(0, 16)))
             for s in (255, 256, 257, 1000, 1023, 1024, 2047, 2048, 3000, 4000)]
    out, offs, sizes, pos = [], [], [], 0

    def close():
        out.append((pos + int(rng.integers(0, 3)), np.array(offs, np.uint64),
                    np.array(sizes, np.uint32)))

    for i in rng.permutation(len(want)):
        s, a = want[i]
        p = pos + (a - pos) % 16
        if p + s + 5 > 4090:
            close()
            offs, sizes, p = [], [], a
        offs.append(p)
        sizes.append(s)
        pos = p + s + 5
    close()
    for blen in (4095, 4096, 4097):
        out.append((blen, np.array([0], np.uint64), np.array([blen - 5], np.uint32)))
    return out


LARGE_SIZES = [(1 << 20) - 1, 1 << 20, (1 << 20) + 1, (16 << 20) + 3, (64 << 20) + 5]


def large_blocks():
    """blocks of 1 MiB - 1 .. 64 MiB + 5 at start alignments 0..3, interleaved
    with 4 KiB blocks, 5-byte trailers -> (offsets u64, sizes u32, total)"""
    offs, sizes, pos = [], [], 0
    for a in range(4):
        for s in LARGE_SIZES:
            pos += (a - pos) % 4
            offs.append(pos)
            sizes.append(s)
            pos += s + 5
            offs.append(pos)
            sizes.append(4096)
            pos += 4096 + 5
    return np.array(offs, np.uint64), np.array(sizes, np.uint32), pos + 64
