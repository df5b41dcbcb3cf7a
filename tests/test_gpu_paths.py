"""GPU parity on the large-batch kernel paths, at the smallest shapes that
reach them (tests/dispatch.py builds the inputs from the device's CU count and
restates the dispatch rules; tests/test_dispatch_cpu.py checks the same
builders without a GPU).

Every comparison is bit-exact against the oracle and covers every element.
Every result array handed to the engine is prefilled with a sentinel
(0x5A5A5A5A, 0xA5 for bytes), so an element the kernels never store fails its
comparison instead of showing a previous call's value.  Each case asserts the
kernel name or the restated precondition that proves its path.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from forst_amd import ForstError, engine  # noqa: E402
from forst_amd.engine import ChecksumType as CT  # noqa: E402
from oracle import oracle as O  # noqa: E402
import dispatch as D  # noqa: E402

DEV = "cuda"
NT = O.host_threads()
CUS = torch.cuda.get_device_properties(0).multi_processor_count
ALL_TYPES = [CT.kCRC32c, CT.kXXH3, CT.kxxHash, CT.kxxHash64, CT.kNoChecksum]
HASH_TYPES = ALL_TYPES[:4]
S32, S64, S8 = D.SENTINEL32, D.SENTINEL32 * 0x100000001, D.SENTINEL8


def d(a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).to(DEV)


def host(t):
    a = t.cpu().numpy()
    unsigned = {np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32}.get(a.dtype)
    return a.view(unsigned) if unsigned else a


def s32(n):
    return torch.full((n,), S32, dtype=torch.int32, device=DEV)


def s64(n):
    return torch.full((n,), S64, dtype=torch.int64, device=DEV)


def s8(n):
    return torch.full((n,), S8, dtype=torch.uint8, device=DEV)


def counter(v=0):
    return torch.full((1,), v, dtype=torch.int64, device=DEV)


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, int(bad.size), bad[:8].tolist(),
                           [hex(int(x)) for x in got[bad[:8]]],
                           [hex(int(x)) for x in want[bad[:8]]])


def in_range(offs, sizes, need_extra, base_len):
    """stream_common.h desc_in_range: off <= base_len && need <= base_len - off"""
    offs = offs.astype(np.uint64)
    ok = offs <= np.uint64(base_len)
    room = np.where(ok, np.uint64(base_len) - np.where(ok, offs, np.uint64(0)), np.uint64(0))
    return ok & (sizes.astype(np.uint64) + np.uint64(need_extra) <= room)


def want_compute(ct, hb, offs, sizes, lasts, mods):
    """the oracle's trailer checksum per block; 0 for a descriptor out of range"""
    v = in_range(offs, sizes, 0 if lasts is not None else 1, len(hb))
    out = np.zeros(len(offs), np.uint32)
    out[v] = O.block_checksum_batch(int(ct), hb, offs[v], sizes[v],
                                    last_bytes=None if lasts is None else lasts[v],
                                    modifiers=None if mods is None else mods[v], nthreads=NT)
    return out


def le32_at(hb, pos):
    v = np.zeros(len(pos), np.uint32)
    for k in range(4):
        v |= hb[pos + k].astype(np.uint32) << np.uint32(8 * k)
    return v


def want_verify(ct, hb, offs, sizes, mods):
    """(computed, stored, ok, mismatches) of VerifyBlockChecksum per block by
    the oracle; a descriptor out of range is 0, 0, not ok and counted"""
    v = in_range(offs, sizes, 5, len(hb))
    n = len(offs)
    comp, stored, ok = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    m = None if mods is None else mods[v]
    comp[v], ok[v], bad = O.block_verify_batch(int(ct), hb, offs[v], sizes[v], modifiers=m,
                                                nthreads=NT)
    end = (offs[v] + sizes[v]).astype(np.int64)
    stored[v] = le32_at(hb, end + 1) - (np.uint32(0) if m is None else m)
    return comp, stored, ok, int(bad) + int((~v).sum())


def with_trailers(hb, offs, sizes, lasts, sums):
    """the image a table builder leaves: [type][LE32 checksum] after each block"""
    img = hb.copy()
    v = in_range(offs, sizes, 5, len(hb))
    end = (offs[v] + sizes[v]).astype(np.int64)
    img[end] = lasts[v]
    for k in range(4):
        img[end + 1 + k] = (sums[v] >> np.uint32(8 * k)).astype(np.uint8)
    return img


def run_verify(ct, dbase, doffs, dsizes, dmods, n, count=None):
    count = counter() if count is None else count
    c, s, o, bad = engine.block_verify_batch(ct, dbase, doffs, dsizes, modifiers=dmods,
                                             computed=s32(n), stored=s32(n), ok=s8(n),
                                             mismatches=count)
    return host(c), host(s), host(o), int(host(bad)[0])


# ---- A: raw batches past the small-batch dispatch ---------------------------

@pytest.fixture(scope="module")
def raw_crc():
    r = D.raw_crc_batch(CUS)
    base, offs, sizes, init = r["base"], r["offs"], r["sizes"], r["init"]
    r["want0"] = O.crc32c_batch(base, offs, sizes, nthreads=NT)
    r["want_init"] = np.array([O.crc32c_extend(int(i), base[int(o):int(o) + int(s)])
                               for i, o, s in zip(init, offs, sizes)], np.uint32)
    r["dbase"] = d(base)
    return r


@pytest.mark.parametrize("order", ["file", "permuted"])
def test_raw_crc32c_lane_and_filter_kernels_with_init(raw_crc, order):
    """crc32c::Extend(init, data, n) through crc32c_raw_lane_kernel (messages
    under kRawSplit, its unstep start from the init) and
    crc32c_rows_raw_filt_kernel (the rest, static shares then claimed chunks),
    descriptors in file order and in a random permutation"""
    r = raw_crc
    n = r["n"]
    assert n >= 128 * D.CRC_WAVES * D.crc_grid(n, CUS)
    assert D.feed_share1(n, D.crc_grid(n, CUS) * D.CRC_WAVES) > 0
    p = np.arange(n) if order == "file" else np.random.default_rng(3).permutation(n)
    got = engine.crc32c_batch(r["dbase"], d(r["offs"][p]), d(r["sizes"][p]),
                              init_crcs=d(r["init"][p]), out=s32(n))
    assert engine.last_kernel() == "crc32c_rows_raw_filt_kernel"
    same(host(got), r["want_init"][p], order)


@pytest.mark.parametrize("order", ["file", "permuted"])
def test_raw_crc32c_lane_and_filter_kernels_edge_descriptors(raw_crc, order):
    """no init; messages past the end on both sides of the split, offsets
    1 << 59 and (1 << 58) - 1 (the filter kernel reuses the top bits of an
    offset), and lengths 77, 255, 256, 509 and 1300 ending exactly at base_len:
    0 for the out-of-range ones"""
    r = raw_crc
    n = r["n"]
    base = r["base"]
    o2, s2, zero = D.raw_edge_descriptors(r["offs"], r["sizes"], len(base))
    want = r["want0"].copy()
    for k in range(5, 14):
        o, s = int(o2[k]), int(s2[k])
        want[k] = 0 if k in zero else O.crc32c_extend(0, base[o:o + s])
    p = np.arange(n) if order == "file" else np.random.default_rng(4).permutation(n)
    got = engine.crc32c_batch(r["dbase"], d(o2[p]), d(s2[p]), out=s32(n))
    assert engine.last_kernel() == "crc32c_rows_raw_filt_kernel"
    same(host(got), want[p], order)


def test_raw_xxh3_static_shares():
    """forst_xxh3_64_batch with enough messages for the static shares of the
    feed (n >= 128 * 12 * grid at up to 2 resident workgroups per CU): every
    XXH3 input class at every alignment, sparse long messages, in file order
    and permuted"""
    x = D.raw_xxh3_batch(CUS)
    n, base, offs, sizes = x["n"], x["base"], x["offs"], x["sizes"]
    grid = D.xx_rows_grid(n, CUS, D.XX_RAW_OCCUPANCY)
    assert D.feed_share1(n, grid * D.XX_ROWS_WAVES) > 0
    want = O.xxh3_batch(base, offs, sizes, nthreads=NT)
    dbase = d(base)
    for p in (np.arange(n), np.random.default_rng(5).permutation(n)):
        got = engine.xxh3_64_batch(dbase, d(offs[p]), d(sizes[p]), out=s64(n))
        assert engine.last_kernel() == "xxh3_rows_kernel<raw>"
        same(host(got), want[p])


# ---- B: wal_verify_batch on dense logs, sub-ranges, counters ----------------

LOGNUM = 0x4D2


@pytest.fixture(scope="module", params=[False, True], ids=["legacy", "recyclable"])
def dense_log(request):
    rec = request.param
    w = D.dense_wal(CUS, rec, LOGNUM, O.wal_frame)
    w["recyclable"] = rec
    tiles = D.wal_tile_records(w["poffs"], w["n_blocks"])
    assert (tiles > D.WAL_FILL_CAP).any() and ((tiles >= 1) & (tiles <= D.WAL_FILL_CAP)).any()
    assert w["n_dense"] > 64 * D.CRC_WAVES * CUS
    return w


def run_wal(dlog, first_block=0, n_blocks=None, count=None, total=None):
    n = (total - first_block) if n_blocks is None else n_blocks
    st, nr, fo, bad = engine.wal_verify_batch(dlog, log_number=LOGNUM, first_block=first_block,
                                              n_blocks=n_blocks, bad_blocks=count,
                                              status=s8(n), nrec=s32(n), fail_off=s32(n))
    return host(st), host(nr), host(fo), int(host(bad)[0])


def wal_bad(st):
    return int(((st != 0) & (st != 3)).sum())


def test_wal_verify_dense_log_clean_and_faults(dense_log):
    """wal_fill_kernel's unstaged branch (a 256-block tile of more than
    kFillCap records), the staged one and a tile of both kinds of block:
    status, nrec and fail_off of every block and bad_blocks against the
    oracle's reader, clean and with faults"""
    w = dense_log
    nb = w["n_blocks"]
    for buf, hit in ((w["buf"], []), D.wal_faults(w, LOGNUM)):
        ost, onr, ofo = O.wal_verify_blocks(buf, LOGNUM, nthreads=NT)
        assert set(np.nonzero((ost != 0) & (ost != 3))[0].tolist()) <= set(hit)
        if hit:
            want = {1, 2, 3, 4} if w["recyclable"] else {1, 2, 3}
            assert set(ost[hit].tolist()) == want
        st, nr, fo, bad = run_wal(d(buf), total=nb)
        same(st, ost, "status")
        same(nr, onr, "nrec")
        same(fo, ofo, "fail_off")
        assert bad == wal_bad(ost)


def test_wal_verify_sub_ranges_and_shared_counter(dense_log):
    """(first_block, n_blocks) sub-ranges equal the slices of the full call
    (each range starts tiles of its own at first_block); every call adds into
    one counter that starts at a non-zero value; a range beyond log_len raises"""
    w = dense_log
    nb = w["n_blocks"]
    buf, hit = D.wal_faults(w, LOGNUM)
    ost, onr, ofo = O.wal_verify_blocks(buf, LOGNUM, nthreads=NT)
    dlog = d(buf)
    count = counter(1000)
    expect = 1000
    for fb, n in ((0, 1), (1, 255), (255, 2), (257, nb - 257), (nb - 1, 1), (nb, 0)):
        st, nr, fo, bad = run_wal(dlog, fb, n, count=count)
        same(st, ost[fb:fb + n], ("status", fb, n))
        same(nr, onr[fb:fb + n], ("nrec", fb, n))
        same(fo, ofo[fb:fb + n], ("fail_off", fb, n))
        expect += wal_bad(ost[fb:fb + n])
        assert bad == expect, (fb, n)
    assert expect == 1000 + wal_bad(ost) and expect > 1000
    for fb, n in ((nb, 1), (0, nb + 1), (nb + 1, 1)):
        with pytest.raises(ForstError):
            engine.wal_verify_batch(dlog, log_number=LOGNUM, first_block=fb, n_blocks=n)
    assert int(host(count)[0]) == expect


# ---- C: the direct-store path of the CRC32C and XXH3 rows kernels -----------

class Clustered:
    """a clustered batch on the device and the host, with its ranges"""

    def __init__(self, ct):
        self.ct = ct
        if ct == CT.kCRC32c:
            self.offs, self.sizes, self.total, self.n_small = D.crc_clustered(CUS)
            self.G = D.crc_grid(len(self.offs), CUS)
            self.cost, self.stage, self.name = D.CRC_BLOCK_COST, D.CRC_STAGE_W, "crc32c_rows_kernel"
        else:
            self.offs, self.sizes, self.total, self.n_small = D.xxh3_clustered(CUS)
            self.G = D.xx_rows_grid(len(self.offs), CUS, D.XX_BLOCK_OCCUPANCY)
            self.cost, self.stage, self.name = D.XX_BLOCK_COST, D.XX_STAGE_W, "xxh3_rows_kernel"
        self.n = len(self.offs)
        self.L, self.b, self.direct = D.direct_part(self.offs, self.sizes, self.G, self.cost,
                                                    self.stage)
        assert self.L[self.b + 1] - self.L[self.b] > self.stage
        assert D.covers_small_sizes(self.offs, self.sizes, self.direct)
        dev = torch.empty((self.total + 255) // 256 * 256, dtype=torch.uint8, device=DEV)
        engine.fill_stream(dev, 0, 0xC1C + int(ct))
        self.dbase = dev[:self.total]
        self.hb = host(self.dbase)
        rng = np.random.default_rng(int(ct))
        self.lasts = rng.integers(0, 256, self.n, dtype=np.uint8)
        self.mods = rng.integers(0, 2**32, self.n, dtype=np.uint64).astype(np.uint32)
        self.doffs, self.dsizes = d(self.offs), d(self.sizes)
        self.dlasts, self.dmods = d(self.lasts), d(self.mods)
        self.sums = want_compute(ct, self.hb, self.offs, self.sizes, self.lasts, self.mods)
        self._img = None

    def image(self):
        if self._img is None:
            self._img = with_trailers(self.hb, self.offs, self.sizes, self.lasts, self.sums)
        return self._img


@pytest.fixture(scope="module")
def clustered_crc():
    c = Clustered(CT.kCRC32c)
    yield c
    c.__dict__.clear()


@pytest.fixture(scope="module")
def clustered_xxh3():
    c = Clustered(CT.kXXH3)
    yield c
    c.__dict__.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=["crc", "xxh3"])
def clustered(request):
    return request.getfixturevalue("clustered_" + request.param)


def test_rows_direct_stores_compute(clustered):
    """compute mode with a workgroup range longer than the result stage: the
    results past it are stored directly, with and without last_bytes"""
    c = clustered
    got = engine.block_checksum_batch(c.ct, c.dbase, c.doffs, c.dsizes, last_bytes=c.dlasts,
                                      modifiers=c.dmods, out=s32(c.n))
    assert engine.last_kernel() == c.name + "<compute>"
    same(host(got), c.sums, "with last_bytes")
    want = want_compute(c.ct, c.hb, c.offs, c.sizes, None, c.mods)
    got = engine.block_checksum_batch(c.ct, c.dbase, c.doffs, c.dsizes, modifiers=c.dmods,
                                      out=s32(c.n))
    same(host(got), want, "last byte from memory")


def test_rows_direct_stores_trailer(clustered):
    """trailer mode: the checksums, and the whole buffer afterwards equals the
    host-built image -- every trailer byte right (staged: written after the
    loop; direct: by lanes 11..15 of the row), no other byte changed"""
    c = clustered
    dimg = c.dbase.clone()
    out = s32(c.n)
    engine.block_trailer_batch(c.ct, dimg, c.doffs, c.dsizes, c.dlasts, c.dmods, out)
    assert engine.last_kernel() == c.name + "<trailer>"
    same(host(out), c.sums)
    got = host(dimg)
    want = c.image()
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        end = (c.offs + c.sizes).astype(np.int64)
        blk = np.searchsorted(end, bad[:8], side="right") - 1
        raise AssertionError((len(bad), bad[:8].tolist(), blk.tolist(),
                              (bad[:8] - end[blk]).tolist()))
    # without a checksum array: only the in-place bytes
    dimg = c.dbase.clone()
    engine.block_trailer_batch(c.ct, dimg, c.doffs, c.dsizes, c.dlasts, c.dmods, None)
    assert torch.equal(dimg, d(want))


def test_rows_direct_stores_verify(clustered):
    """verify mode: clean, then flips in blocks of the staged and the direct
    part of the long range and of other ranges, and descriptors out of range in
    both parts -- ok, computed, stored and the mismatch count"""
    c = clustered
    img = c.image().copy()
    dimg = d(img)
    comp, stored, ok, bad = run_verify(c.ct, dimg, c.doffs, c.dsizes, c.dmods, c.n)
    assert engine.last_kernel() == c.name + "<verify>"
    same(comp, c.sums - c.mods, "computed")
    same(stored, c.sums - c.mods, "stored")
    assert bad == 0 and (ok == 1).all()
    f = D.verify_faults(c.offs, c.sizes, c.total, c.G, c.cost, c.stage)
    staged, direct, other, o2, s2 = f["staged"], f["direct"], f["other"], f["offs"], f["sizes"]
    for j, i in enumerate(np.concatenate([staged[3:], direct[4:], other])):
        o, n = int(c.offs[i]), int(c.sizes[i])
        where = [o + n, o + n + 1 + j % 4] + ([o + (j * 7919) % n, o + n - 1, o] if n else [])
        pos = where[j % len(where)]
        img[pos] ^= 1 << (j % 8)
    wc, ws, wok, wbad = want_verify(c.ct, img, o2, s2, c.mods)
    assert wbad == len(staged) + len(direct) + len(other)
    comp, stored, ok, bad = run_verify(c.ct, d(img), d(o2), d(s2), c.dmods, c.n)
    same(comp, wc, "computed")
    same(stored, ws, "stored")
    same(ok, wok, "ok")
    assert bad == wbad


# ---- D: optional outputs and counters ---------------------------------------

SUBSETS = [(c, s, o) for c in (True, False) for s in (True, False) for o in (True, False)]


def check_verify_subsets(ct, dbase, doffs, dsizes, dmods, want):
    wc, ws, wok, wbad = want
    n = len(wc)
    assert wbad > 0
    for has_c, has_s, has_o in SUBSETS:
        count = counter(1000)
        for call in (1, 2):
            c, s, o, bad = engine.block_verify_batch(
                ct, dbase, doffs, dsizes, modifiers=dmods, computed=s32(n) if has_c else None,
                stored=s32(n) if has_s else None, ok=s8(n) if has_o else None, mismatches=count)
            assert (c is None, s is None, o is None) == (not has_c, not has_s, not has_o)
            if has_c:
                same(host(c), wc, ("computed", has_c, has_s, has_o))
            if has_s:
                same(host(s), ws, ("stored", has_c, has_s, has_o))
            if has_o:
                same(host(o), wok, ("ok", has_c, has_s, has_o))
            assert int(host(bad)[0]) == 1000 + call * wbad, (has_c, has_s, has_o, call)


def test_verify_optional_outputs_on_the_clustered_batch(clustered_crc):
    """block_verify_batch with each subset of {computed, stored, ok} absent
    (stored=None is what the benchmark times; computed=None, stored=None its
    host-streaming form), staged and direct results: the outputs present and
    the count do not depend on which others are absent; the counter
    accumulates from 1000 over two calls"""
    c = clustered_crc
    img = c.image().copy()
    rng = np.random.default_rng(10)
    for i in np.concatenate([rng.choice(c.n_small, 40, replace=False),
                             rng.choice(np.arange(c.n_small, c.n), 10, replace=False)]):
        img[int(c.offs[i]) + int(c.sizes[i]) + 2] ^= 0x08
    want = want_verify(c.ct, img, c.offs, c.sizes, c.mods)
    check_verify_subsets(c.ct, d(img), c.doffs, c.dsizes, c.dmods, want)
    assert engine.last_kernel() == "crc32c_rows_kernel<verify>"


def small_batch(ct, seed=21):
    """3000 blocks of 0..20000 bytes with trailers of the oracle, then 40 flips"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 20000, 3000).astype(np.uint32)
    sizes[:64] = np.arange(64)
    offs = np.zeros(len(sizes), np.uint64)
    offs[1:] = np.cumsum(sizes[:-1].astype(np.uint64) + np.uint64(5))
    total = int(offs[-1]) + int(sizes[-1]) + 5
    hb = rng.integers(0, 256, total, dtype=np.uint8)
    lasts = rng.integers(0, 8, len(sizes), dtype=np.uint8)
    mods = rng.integers(0, 2**32, len(sizes), dtype=np.uint64).astype(np.uint32)
    img = with_trailers(hb, offs, sizes, lasts, want_compute(ct, hb, offs, sizes, lasts, mods))
    for j, i in enumerate(rng.choice(len(sizes), 40, replace=False)):
        img[int(offs[i]) + int(sizes[i]) + j % 5] ^= 1 << (j % 8)
    return img, offs, sizes, mods


@pytest.mark.parametrize("ctype", ALL_TYPES)
def test_verify_optional_outputs_small_batch(ctype):
    img, offs, sizes, mods = small_batch(ctype)
    want = want_verify(ctype, img, offs, sizes, mods)
    check_verify_subsets(ctype, d(img), d(offs), d(sizes), d(mods), want)


def kv_case(n=400, seed=77, prot_bytes=8):
    """the layout of test_emu_kv_staged_and_direct_subtiles with the checksum
    bytes behind each value: small values, 3-6 KiB values, long keys"""
    rng = np.random.default_rng(seed)
    ks = rng.integers(0, 90, n).astype(np.uint32)
    vs = rng.integers(0, 900, n).astype(np.uint32)
    vs[rng.integers(0, n, 25)] = rng.integers(3000, 6000, 25)
    ks[rng.integers(0, n, 5)] = rng.integers(241, 700, 5)
    ko, vo, co = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    pos = 3
    for i in range(n):
        ko[i] = pos
        pos += int(ks[i])
        vo[i] = pos
        pos += int(vs[i])
        co[i] = pos
        pos += 8
    base = rng.integers(0, 256, pos, dtype=np.uint8)
    ops = rng.integers(0, 26, n).astype(np.uint8)
    seqs = rng.integers(0, 2**63, n, dtype=np.uint64)
    prot = O.kv_protect_batch(base, ko, ks, vo, vs, ops, seqs, None)
    pb = prot.view(np.uint8).reshape(n, 8)
    for k in range(prot_bytes):
        base[co.astype(np.int64) + k] = pb[:, k]
    return dict(base=base, ko=ko, ks=ks, vo=vo, vs=vs, co=co, ops=ops, seqs=seqs, prot=prot, n=n)


def test_kv_verify_optional_outputs_and_counter():
    kv = kv_case()
    n = kv["n"]
    base = kv["base"].copy()
    victims = [7, 100, 250, 399]
    for i in victims:
        base[int(kv["co"][i]) + 1] ^= 0x10
    wok = np.ones(n, np.uint8)
    wok[victims] = 0
    args = [d(base)] + [d(kv[k]) for k in ("ko", "ks", "vo", "vs")] + [8, d(kv["co"]),
                                                                      d(kv["ops"]), d(kv["seqs"])]
    for has_c, has_o in ((True, True), (False, True), (True, False), (False, False)):
        count = counter(1000)
        for call in (1, 2):
            c, o, bad = engine.kv_verify_batch(*args, computed=s64(n) if has_c else None,
                                               ok=s8(n) if has_o else None, mismatches=count)
            if has_c:
                same(host(c), kv["prot"], "computed")
            if has_o:
                same(host(o), wok, "ok")
            assert int(host(bad)[0]) == 1000 + call * len(victims)


def test_memtable_verify_optional_outputs_and_counter():
    from test_gpu_kv_sites import make_memtable
    n = 3000
    base, offs, cp = make_memtable(n, 8, 0xA15F)
    g = d(base)
    go = d(offs)
    engine.memtable_protect_batch(g, go, 8)
    hb = host(g).copy()
    for i in (9, 1000, 2999):
        hb[int(offs[i]) + 1] ^= 0x10
    wcomp, wst = O.memtable_verify_batch(hb, len(hb), offs.view(np.uint64), 8)
    assert (wst != 0).sum() == 3
    g = d(hb)
    for has_c, has_s in ((True, True), (False, True), (True, False), (False, False)):
        count = counter(1000)
        for call in (1, 2):
            c, s, bad = engine.memtable_verify_batch(g, go, 8, computed=s64(n) if has_c else None,
                                                     status=s8(n) if has_s else None,
                                                     mismatches=count)
            if has_c:
                same(host(c), wcomp, "computed")
            if has_s:
                same(host(s), wst, "status")
            assert int(host(bad)[0]) == 1000 + call * 3


def test_wal_verify_optional_outputs_and_counter(dense_log):
    """the wrapper's status / nrec / fail_off switches: each subset of outputs
    absent, the counter accumulating from 1000 over two calls"""
    w = dense_log
    buf, hit = D.wal_faults(w, LOGNUM)
    ost, onr, ofo = O.wal_verify_blocks(buf, LOGNUM, nthreads=NT)
    dlog = d(buf)
    nb = w["n_blocks"]
    for has_s, has_n, has_f in SUBSETS:
        count = counter(1000)
        for call in (1, 2):
            st, nr, fo, bad = engine.wal_verify_batch(
                dlog, log_number=LOGNUM, bad_blocks=count, status=s8(nb) if has_s else None,
                nrec=s32(nb) if has_n else None, fail_off=s32(nb) if has_f else None)
            assert (st is None, nr is None, fo is None) == (not has_s, not has_n, not has_f)
            if has_s:
                same(host(st), ost, "status")
            if has_n:
                same(host(nr), onr, "nrec")
            if has_f:
                same(host(fo), ofo, "fail_off")
            assert int(host(bad)[0]) == 1000 + call * wal_bad(ost)
    # the defaults are unchanged: all three outputs, a fresh counter
    st, nr, fo, bad = engine.wal_verify_batch(dlog, log_number=LOGNUM)
    same(host(st), ost)
    same(host(nr), onr)
    same(host(fo), ofo)
    assert int(host(bad)[0]) == wal_bad(ost)


# ---- E: bases 4, 8 and 12 bytes past 16-byte alignment ----------------------

SIMPLE_NAME = {CT.kCRC32c: "crc32c_block_kernel_simple", CT.kXXH3: "xxh3_block_kernel_simple",
               CT.kxxHash: "xxhash32_block_kernel", CT.kxxHash64: "xxhash64_block_kernel",
               CT.kNoChecksum: "noop_block_kernel"}
ROWS_NAME = {CT.kCRC32c: "crc32c_rows_kernel", CT.kXXH3: "xxh3_rows_kernel",
             CT.kxxHash: "xxhash32_lane_kernel", CT.kxxHash64: "xxhash64_lane_kernel",
             CT.kNoChecksum: "noop_block_kernel"}


EDGE_SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 30, 31, 32, 33, 63, 64, 65, 127, 128, 129,
              239, 240, 241, 255, 256, 1023, 1024, 1025, 4090, 4091, 4092, 4093, 4094, 4095,
              4096, 4097, 4098, 8191, 8192, 8193, 16383, 16384, 16385, 65535, 65536, 65537]
SHIFTS = [4, 8, 12]


def shifted(hb, k):
    """hb on the device at a base k bytes past a 16-byte boundary"""
    whole = torch.empty(len(hb) + 16, dtype=torch.uint8, device=DEV)
    assert whole.data_ptr() % 16 == 0
    view = whole[k:k + len(hb)]
    view.copy_(torch.from_numpy(hb))
    assert view.data_ptr() % 16 == k
    return view


def edge_layout(small, seed=7):
    if small:  # a buffer under 4 KiB: the simple / group kernels
        sizes = np.array(list(range(0, 70)) + [200, 255, 256, 257], np.uint32)
    else:
        sizes = np.repeat(np.array(EDGE_SIZES, np.uint32), 16)
    offs = np.zeros(len(sizes), np.uint64)
    offs[1:] = np.cumsum(sizes[:-1].astype(np.uint64) + np.uint64(5))
    total = int(offs[-1]) + int(sizes[-1]) + 5
    rng = np.random.default_rng(seed)
    hb = rng.integers(0, 256, total, dtype=np.uint8)
    lasts = rng.integers(0, 256, len(sizes), dtype=np.uint8)
    mods = rng.integers(0, 2**32, len(sizes), dtype=np.uint64).astype(np.uint32)
    assert (total < D.SIMPLE_BELOW) == small
    return hb, offs, sizes, lasts, mods


@pytest.mark.parametrize("small", [False, True], ids=["rows", "simple"])
@pytest.mark.parametrize("ctype", ALL_TYPES)
def test_block_modes_at_shifted_bases(ctype, small):
    hb, offs, sizes, lasts, mods = edge_layout(small)
    n = len(offs)
    doffs, dsizes, dlasts, dmods = d(offs), d(sizes), d(lasts), d(mods)
    sums = want_compute(ctype, hb, offs, sizes, lasts, mods)
    img = with_trailers(hb, offs, sizes, lasts, sums)
    img[int(offs[5]) + int(sizes[5]) + 1] ^= 1  # two mismatches
    img[int(offs[n - 1])] ^= 0x80
    wc, ws, wok, wbad = want_verify(ctype, img, offs, sizes, mods)
    for k in SHIFTS:
        dbase = shifted(hb, k)
        got = engine.block_checksum_batch(ctype, dbase, doffs, dsizes, last_bytes=dlasts,
                                          modifiers=dmods, out=s32(n))
        assert engine.last_kernel() == (SIMPLE_NAME if small else ROWS_NAME)[ctype] + "<compute>"
        same(host(got), sums, ("compute", k))
        out = s32(n)
        engine.block_trailer_batch(ctype, dbase, doffs, dsizes, dlasts, dmods, out)
        same(host(out), sums, ("trailer", k))
        same(host(dbase), with_trailers(hb, offs, sizes, lasts, sums), ("image", k))
        comp, stored, ok, bad = run_verify(ctype, shifted(img, k), doffs, dsizes, dmods, n)
        same(comp, wc, ("computed", k))
        same(stored, ws, ("stored", k))
        same(ok, wok, ("ok", k))
        assert bad == wbad
    for k in (1, 2, 3):
        with pytest.raises(ForstError):
            engine.block_checksum_batch(ctype, shifted(hb, k), doffs, dsizes, last_bytes=dlasts)
        with pytest.raises(ForstError):
            engine.block_verify_batch(ctype, shifted(hb, k), doffs, dsizes)
        with pytest.raises(ForstError):
            engine.block_trailer_batch(ctype, shifted(hb, k), doffs, dsizes, dlasts)


@pytest.mark.parametrize("small", [False, True], ids=["rows", "simple"])
def test_raw_modes_and_buffer_crc_at_shifted_bases(small):
    hb, offs, sizes, _, init = edge_layout(small, seed=8)
    n = len(offs)
    doffs, dsizes = d(offs), d(sizes)
    wcrc = np.array([O.crc32c_extend(int(i), hb[int(o):int(o) + int(s)])
                     for i, o, s in zip(init, offs, sizes)], np.uint32)
    wxx = O.xxh3_batch(hb, offs, sizes, nthreads=NT)
    cuts = [0, 1, 63, 4095, 4096, 65537, len(hb)]
    for k in SHIFTS:
        dbase = shifted(hb, k)
        same(host(engine.crc32c_batch(dbase, doffs, dsizes, init_crcs=d(init), out=s32(n))), wcrc,
             ("crc32c", k))
        assert engine.last_kernel() == D.crc_raw_kernel(n, len(hb), CUS)
        same(host(engine.xxh3_64_batch(dbase, doffs, dsizes, out=s64(n))), wxx, ("xxh3", k))
        for m in (c for c in cuts if c <= len(hb)):
            got = int(host(engine.crc32c_buffer(dbase[:m], 0x12345678, out=s32(1)))[0])
            assert got == O.crc32c_extend(0x12345678, hb[:m].tobytes()), (k, m)
    for k in (1, 2, 3):
        dbase = shifted(hb, k)
        with pytest.raises(ForstError):
            engine.crc32c_batch(dbase, doffs, dsizes)
        with pytest.raises(ForstError):
            engine.xxh3_64_batch(dbase, doffs, dsizes)
        with pytest.raises(ForstError):
            engine.crc32c_buffer(dbase)


def test_kv_calls_at_shifted_bases():
    """hash64_batch, kv_protect_batch and kv_verify_batch at a base that is
    not 16-byte aligned (kv_kernel switches its LDS staging off), entries in
    buffer order and reversed, 3-6 KiB values among them"""
    kv = kv_case()
    n = kv["n"]
    base = kv["base"]
    wh = O.hash64_batch(base, kv["vo"], kv["vs"], seed=O.KV_SEED_V)
    for k in [0] + SHIFTS:
        dbase = shifted(base, k)
        for p in (np.arange(n), np.arange(n)[::-1].copy()):
            a = {x: d(kv[x][p]) for x in ("ko", "ks", "vo", "vs", "co", "ops", "seqs")}
            got = engine.hash64_batch(dbase, a["vo"], a["vs"], seed=O.KV_SEED_V, out=s64(n))
            same(host(got), wh[p], ("hash64", k))
            got = engine.kv_protect_batch(dbase, a["ko"], a["ks"], a["vo"], a["vs"], a["ops"],
                                          a["seqs"], out=s64(n))
            same(host(got), kv["prot"][p], ("protect", k))
            c, o, bad = engine.kv_verify_batch(dbase, a["ko"], a["ks"], a["vo"], a["vs"], 8, a["co"],
                                               a["ops"], a["seqs"], computed=s64(n), ok=s8(n),
                                               mismatches=counter())
            same(host(c), kv["prot"][p], ("verify", k))
            assert (host(o) == 1).all() and int(host(bad)[0]) == 0


@pytest.mark.parametrize("recyclable", [False, True])
def test_wal_calls_at_shifted_bases(recyclable):
    rng = np.random.default_rng(41)
    lens = np.exp(rng.uniform(np.log(1), np.log(40000), 600)).astype(np.uint32)
    lens[:6] = [0, 1, 7, 32761, 32762, 70000]
    payload = rng.integers(0, 256, int(lens.astype(np.int64).sum()), dtype=np.uint8)
    buf, poffs, plens = O.wal_frame(payload, lens, recyclable=recyclable, log_number=LOGNUM)
    hs = 11 if recyclable else 7
    bad = buf.copy()
    k = int(np.nonzero(plens > 0)[0][len(poffs) // 2])
    bad[int(poffs[k]) + hs + int(plens[k]) // 2] ^= 0x04
    ost, onr, ofo = O.wal_verify_blocks(bad, LOGNUM, nthreads=NT)
    assert wal_bad(ost) == 1
    nb = len(ost)
    wiped = buf.copy()
    for o in poffs:
        wiped[int(o):int(o) + 4] = 0
    wcrc = le32_at(buf, poffs.astype(np.int64))
    starts = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    wxx = np.array([O.xxh3_64(payload[starts[j]:starts[j + 1]].tobytes())
                    for j in range(len(lens))], np.uint64)
    dpo, dpl = d(poffs), d(plens)
    for s in SHIFTS:
        st, nr, fo, nbad = engine.wal_verify_batch(shifted(bad, s), log_number=LOGNUM,
                                                   bad_blocks=counter(), status=s8(nb),
                                                   nrec=s32(nb), fail_off=s32(nb))
        same(host(st), ost, ("status", s))
        same(host(nr), onr, ("nrec", s))
        same(host(fo), ofo, ("fail_off", s))
        assert int(host(nbad)[0]) == 1
        for kw in ({}, {"payload_lengths": dpl, "recyclable": recyclable}):
            dl = shifted(wiped, s)
            crcs = engine.wal_record_crc_batch(dl, dpo, out=s32(len(poffs)), **kw)
            same(host(crcs), wcrc, ("writer crc", s, bool(kw)))
            same(host(dl), buf, ("writer image", s, bool(kw)))
        h, first = engine.wal_record_xxh3_batch(shifted(buf, s), dpo)
        same(host(h), wxx, ("record xxh3", s))
    for s in (1, 2, 3):
        dl = shifted(buf, s)
        with pytest.raises(ForstError):
            engine.wal_verify_batch(dl, log_number=LOGNUM)
        with pytest.raises(ForstError):
            engine.wal_record_crc_batch(dl, dpo)
        with pytest.raises(ForstError):
            engine.wal_record_crc_batch(dl, dpo, payload_lengths=dpl, recyclable=recyclable)
        with pytest.raises(ForstError):
            engine.wal_record_xxh3_batch(dl, dpo)


# ---- F: buffers under 4 KiB -------------------------------------------------

@pytest.fixture(scope="module")
def small_bufs():
    """every buffer in a 4352-byte slot of its own (a 256-aligned base each),
    the descriptors of all of them in one array, results read back once"""
    bufs = D.small_buffers()
    slot = 4352
    rng = np.random.default_rng(17)
    hb = rng.integers(0, 256, slot * len(bufs), dtype=np.uint8)
    first = np.concatenate([[0], np.cumsum([len(b[1]) for b in bufs])]).astype(np.int64)
    offs = np.concatenate([b[1] for b in bufs])
    sizes = np.concatenate([b[2] for b in bufs])
    n = len(offs)
    return dict(bufs=bufs, slot=slot, hb=hb, first=first, offs=offs, sizes=sizes, n=n,
                lasts=rng.integers(0, 256, n, dtype=np.uint8),
                mods=rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32))


def per_buffer(sb):
    for j, (blen, _, _) in enumerate(sb["bufs"]):
        yield j, blen, slice(j * sb["slot"], j * sb["slot"] + blen), \
            slice(int(sb["first"][j]), int(sb["first"][j + 1]))


@pytest.mark.parametrize("ctype", ALL_TYPES)
def test_buffers_under_4k_block_modes(small_bufs, ctype):
    """compute / trailer / verify on many buffers shorter than 4096 bytes
    (the *_simple and group kernels) and one block filling a buffer of 4095,
    4096 and 4097 bytes, either side of the dispatch boundary"""
    sb = small_bufs
    n, hb = sb["n"], sb["hb"]
    sums = np.zeros(n, np.uint32)
    img = hb.copy()
    for j, blen, bs, ds in per_buffer(sb):
        sums[ds] = want_compute(ctype, hb[bs], sb["offs"][ds], sb["sizes"][ds], sb["lasts"][ds],
                                sb["mods"][ds])
        img[bs] = with_trailers(hb[bs], sb["offs"][ds], sb["sizes"][ds], sb["lasts"][ds], sums[ds])
    dhb, dtr = d(hb), d(hb)
    doffs, dsizes, dlasts, dmods = d(sb["offs"]), d(sb["sizes"]), d(sb["lasts"]), d(sb["mods"])
    out_c, out_t = s32(n), s32(n)
    for j, blen, bs, ds in per_buffer(sb):
        want_name = SIMPLE_NAME[ctype] if blen < D.SIMPLE_BELOW else ROWS_NAME[ctype]
        engine.block_checksum_batch(ctype, dhb[bs], doffs[ds], dsizes[ds], last_bytes=dlasts[ds],
                                    modifiers=dmods[ds], out=out_c[ds])
        assert engine.last_kernel() == want_name + "<compute>", blen
        engine.block_trailer_batch(ctype, dtr[bs], doffs[ds], dsizes[ds], dlasts[ds], dmods[ds],
                                   out_t[ds])
        assert engine.last_kernel() == want_name + "<trailer>", blen
    same(host(out_c), sums, "compute")
    same(host(out_t), sums, "trailer")
    same(host(dtr), img, "image")
    # verify on the image with a flip in every 7th block
    for i in range(0, n, 7):
        j = int(np.searchsorted(sb["first"], i, side="right")) - 1
        img[j * sb["slot"] + int(sb["offs"][i]) + int(sb["sizes"][i]) + i % 5] ^= 1 << (i % 8)
    wc, ws, wok = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    wbad = 0
    for j, blen, bs, ds in per_buffer(sb):
        wc[ds], ws[ds], wok[ds], b = want_verify(ctype, img[bs], sb["offs"][ds], sb["sizes"][ds],
                                                 sb["mods"][ds])
        wbad += b
    dimg = d(img)
    comp, stored, ok, count = s32(n), s32(n), s8(n), counter(1000)
    for j, blen, bs, ds in per_buffer(sb):
        engine.block_verify_batch(ctype, dimg[bs], doffs[ds], dsizes[ds], modifiers=dmods[ds],
                                  computed=comp[ds], stored=stored[ds], ok=ok[ds], mismatches=count)
    same(host(comp), wc, "computed")
    same(host(stored), ws, "stored")
    same(host(ok), wok, "ok")
    assert int(host(count)[0]) == 1000 + wbad and wbad >= n // 10


def test_buffers_under_4k_raw_modes(small_bufs):
    sb = small_bufs
    n, hb = sb["n"], sb["hb"]
    init = sb["mods"]
    wcrc, wxx = np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    sizes = sb["sizes"].copy()
    sizes[-3:] += 5  # the single blocks fill their 4095 / 4096 / 4097-byte buffers
    for j, blen, bs, ds in per_buffer(sb):
        wxx[ds] = O.xxh3_batch(hb[bs], sb["offs"][ds], sizes[ds], nthreads=1)
        for i in range(ds.start, ds.stop):
            o = bs.start + int(sb["offs"][i])
            wcrc[i] = O.crc32c_extend(int(init[i]), hb[o:o + int(sizes[i])])
    dhb, doffs, dsizes, dinit = d(hb), d(sb["offs"]), d(sizes), d(init)
    crc, xx = s32(n), s64(n)
    for j, blen, bs, ds in per_buffer(sb):
        engine.crc32c_batch(dhb[bs], doffs[ds], dsizes[ds], init_crcs=dinit[ds], out=crc[ds])
        assert engine.last_kernel() == D.crc_raw_kernel(ds.stop - ds.start, blen, CUS)
        engine.xxh3_64_batch(dhb[bs], doffs[ds], dsizes[ds], out=xx[ds])
        assert engine.last_kernel() == ("xxh3_block_kernel_simple<raw>" if blen < D.SIMPLE_BELOW
                                        else "xxh3_rows_kernel<raw>")
    same(host(crc), wcrc, "crc32c")
    same(host(xx), wxx, "xxh3")


# ---- G: large blocks --------------------------------------------------------

@pytest.fixture(scope="module")
def large():
    offs, sizes, total = D.large_blocks()
    dev = torch.empty((total + 255) // 256 * 256, dtype=torch.uint8, device=DEV)
    engine.fill_stream(dev, 0, 0x1A26E)
    rng = np.random.default_rng(23)
    g = dict(offs=offs, sizes=sizes, n=len(offs), dbase=dev[:total], hb=host(dev[:total]),
             lasts=rng.integers(0, 256, len(offs), dtype=np.uint8),
             mods=rng.integers(0, 2**32, len(offs), dtype=np.uint64).astype(np.uint32))
    yield g
    g.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("ctype", HASH_TYPES)
def test_large_blocks_block_modes(large, ctype):
    """blocks of 1 MiB - 1 .. 64 MiB + 5 (index and filter blocks of whole-file
    verify) at start alignments 0..3 between 4 KiB blocks: compute, trailer
    (whole image) and verify with a flip in the last byte of each large block"""
    g = large
    n, hb, offs, sizes = g["n"], g["hb"], g["offs"], g["sizes"]
    doffs, dsizes, dlasts, dmods = d(offs), d(sizes), d(g["lasts"]), d(g["mods"])
    sums = want_compute(ctype, hb, offs, sizes, g["lasts"], g["mods"])
    got = engine.block_checksum_batch(ctype, g["dbase"], doffs, dsizes, last_bytes=dlasts,
                                      modifiers=dmods, out=s32(n))
    assert engine.last_kernel() == ROWS_NAME[ctype] + "<compute>"
    same(host(got), sums, "compute")
    dimg = g["dbase"].clone()
    out = s32(n)
    engine.block_trailer_batch(ctype, dimg, doffs, dsizes, dlasts, dmods, out)
    same(host(out), sums, "trailer")
    img = with_trailers(hb, offs, sizes, g["lasts"], sums)
    assert np.array_equal(host(dimg), img)
    pos = (offs[::2] + sizes[::2] - np.uint64(1)).astype(np.int64)
    img[pos] ^= 0x01
    dimg[d(pos)] ^= 0x01
    wc, ws, wok, wbad = want_verify(ctype, img, offs, sizes, g["mods"])
    assert wbad == n // 2
    comp, stored, ok, bad = run_verify(ctype, dimg, doffs, dsizes, dmods, n)
    same(comp, wc, "computed")
    same(stored, ws, "stored")
    same(ok, wok, "ok")
    assert bad == wbad


def test_large_blocks_raw_modes(large):
    g = large
    n, hb, offs, sizes = g["n"], g["hb"], g["offs"], g["sizes"]
    init = g["mods"]
    wcrc = np.array([O.crc32c_extend(int(i), hb[int(o):int(o) + int(s)])
                     for i, o, s in zip(init, offs, sizes)], np.uint32)
    got = engine.crc32c_batch(g["dbase"], d(offs), d(sizes), init_crcs=d(init), out=s32(n))
    same(host(got), wcrc, "crc32c")
    same(host(engine.xxh3_64_batch(g["dbase"], d(offs), d(sizes), out=s64(n))),
         O.xxh3_batch(hb, offs, sizes, nthreads=NT), "xxh3")
