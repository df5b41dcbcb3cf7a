"""GPU parity for a15 at the reference's own call-site layouts, through the C ABI:
encoded MemTable entries (db/memtable.cc:273-307, :676-732) and WriteBatch reps
(db/write_batch.cc:361-716, :3016-3181), decoded on the device.  Pinned by the
reference-made fixtures (tests/golden/gen_kv_golden.py: the reference's own
MemTable::Add / VerifyEntryChecksum and WriteBatch::Iterate) and, at full size,
compared entry for entry with the oracle (itself pinned to those fixtures by
tests/test_oracle_golden.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from forst_amd import engine  # noqa: E402
from oracle import oracle as O  # noqa: E402
import blockgen  # noqa: E402
import kvsites  # noqa: E402

DEV = "cuda"


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def test_memtable_fixtures(kv_sites):
    for name, base, offs, pb, want in kvsites.memtable_cases(*kv_sites):
        comp, st, bad = engine.memtable_verify_batch(d(base), d(offs.view(np.int64)), pb)
        st = host(st)
        assert [O.MEM_STATUS[int(s)] for s in st] == want, name
        ocomp, _ = O.memtable_verify_batch(base, len(base), offs, pb)
        assert (host(comp).view(np.uint64) == ocomp).all(), name
        assert int(host(bad)[0]) == int((st != 0).sum()), name
        if name.endswith("_corrupt") or name == "crafted":
            continue
        z = base.copy()
        for o in offs:
            c = kvsites.mem_checksum_pos(base, int(o))
            z[c:c + pb] = 0
        g = d(z)
        out, pst = engine.memtable_protect_batch(g, d(offs.view(np.int64)), pb)
        assert (host(pst) == 0).all() and (host(out).view(np.uint64) == ocomp).all(), name
        assert (host(g) == base).all(), name  # UpdateEntryChecksum wrote the reference's bytes


def _varint_bytes(v):
    """varint32 encodings of v (< 2^21) as (bytes u8[n, 3], lengths)"""
    v = v.astype(np.int64)
    n = 1 + (v >= 128).astype(np.int64) + (v >= 1 << 14).astype(np.int64)
    b = np.zeros((len(v), 3), np.uint8)
    b[:, 0] = (v & 127) | np.where(n > 1, 128, 0)
    b[:, 1] = ((v >> 7) & 127) | np.where(n > 2, 128, 0)
    b[:, 2] = (v >> 14) & 127
    return b, n


def make_memtable(n, prot_bytes, seed):
    """n MemTable::Add-layout entries (memtable.cc:696-732) back to back:
    varint32(klen + 8) | user key | LE64(seq << 8 | type) | varint32(vlen) |
    value | prot_bytes checksum (zero: written by the protect call)"""
    rng = np.random.default_rng(seed)
    kl = rng.integers(16, 65, n)
    vl = rng.integers(0, 1001, n)
    kl[:8] = [0, 1, 119, 120, 200, 241, 1500, 16383 - 8]
    vl[:8] = [0, 127, 128, 240, 241, 1024, 5000, 16384]
    kb, kn = _varint_bytes(kl + 8)
    vb, vn = _varint_bytes(vl)
    size = kn + kl + 8 + vn + vl + prot_bytes
    offs = np.zeros(n, np.int64)
    offs[1:] = np.cumsum(size[:-1])
    total = int(offs[-1] + size[-1])
    base = rng.integers(0, 256, (total + 255) // 256 * 256, dtype=np.uint8)
    types = rng.choice(np.array([0, 1, 2, 7, 17], np.uint64), n)
    seqs = rng.integers(1, 2**56, n, dtype=np.uint64)
    tag = (seqs << np.uint64(8)) | types
    for j in range(3):  # klen varint
        m = kn > j
        base[offs[m] + j] = kb[m, j]
    kp = offs + kn
    tp = kp + kl
    tb = tag.view(np.uint8).reshape(n, 8)
    for j in range(8):
        base[tp + j] = tb[:, j]
    for j in range(3):
        m = vn > j
        base[tp[m] + 8 + j] = vb[m, j]
    cp = tp + 8 + vn + vl
    for j in range(prot_bytes):
        base[cp + j] = 0
    return base, offs, cp


@pytest.mark.parametrize("prot_bytes", [8, 1])
def test_memtable_full_size(prot_bytes):
    """1 M entries (the a15 bench shape: 16-64 B keys, 0-1000 B values, plus
    every varint width): protect in place, every checksum byte and value
    against the oracle, verify clean, then 60 flips found exactly"""
    n = 1 << 20
    base, offs, cp = make_memtable(n, prot_bytes, 0xA15F + prot_bytes)
    g = d(base)
    go = d(offs)
    out, st = engine.memtable_protect_batch(g, go, prot_bytes)
    assert (host(st) == 0).all()
    hb = host(g)
    ocomp, ost = O.memtable_verify_batch(hb, len(hb), offs.view(np.uint64), prot_bytes)
    assert (ost == 0).all(), "the protect call wrote checksums the oracle rejects"
    assert (host(out).view(np.uint64) == ocomp).all()
    comp, st, bad = engine.memtable_verify_batch(g, go, prot_bytes)
    assert int(host(bad)[0]) == 0 and (host(st) == 0).all()
    rng = np.random.default_rng(5)
    victims = np.sort(rng.choice(np.arange(8, n), 60, replace=False))
    kp = offs[victims] + 1  # key bytes (these entries' klen varints are 1 byte)
    g[d(kp)] ^= 0x10
    comp, st, bad = engine.memtable_verify_batch(g, go, prot_bytes)
    failed = np.nonzero(host(st))[0]
    assert set(failed.tolist()) <= set(victims.tolist())
    assert (host(st)[failed] == 4).all() and int(host(bad)[0]) == len(failed)
    if prot_bytes == 8:
        assert len(failed) == 60


def test_memtable_out_of_range():
    base = np.zeros(64, np.uint8)
    base[60] = 0x20  # klen 32: runs past the buffer
    base[0] = 0x0b  # klen 11, tag, vlen 0 ... checksum past the end at offset 52
    offs = np.array([60, 0, 70, 52], np.int64)
    comp, st, bad = engine.memtable_verify_batch(d(base), d(offs), 8)
    assert host(st).tolist()[0] == 5 and host(st).tolist()[2] == 5
    assert int(host(bad)[0]) == 4


def test_write_batch_fixtures(kv_sites):
    base, offs, lens, reps = kvsites.write_batch_case(*kv_sites)
    prot, first, st, nprot = engine.write_batch_protect_batch(
        d(base), d(offs.view(np.int64)), d(lens.view(np.int32)))
    prot, first, st, nprot = host(prot).view(np.uint64), host(first), host(st), host(nprot)
    for j, (name, status, want) in enumerate(reps):
        assert O.WB_STATUS[int(st[j])] == status, name
        got = prot[first[j]:first[j] + nprot[j]]
        assert got.tolist() == [int(x) for x in want][:len(got)], name
        if status == "OK":
            assert len(got) == len(want) == first[j + 1] - first[j], name


def test_write_batch_many_reps():
    """5000 reps of 0-40 records (recovery-shaped): every protection value and
    status against the oracle's restatement"""
    rng = np.random.default_rng(77)
    reps = [kvsites.wb_rep(rng, int(rng.integers(0, 41))) for _ in range(5000)]
    reps[7] = reps[7][:-1]  # truncated
    offs = np.cumsum([0] + [len(r) + int(rng.integers(0, 4)) for r in reps[:-1]]).astype(np.int64)
    base = np.zeros(int(offs[-1]) + len(reps[-1]) + 64, np.uint8)
    for o, r in zip(offs, reps):
        base[o:o + len(r)] = np.frombuffer(r, np.uint8)
    lens = np.array([len(r) for r in reps], np.int32)
    prot, first, st, nprot = engine.write_batch_protect_batch(d(base), d(offs), d(lens))
    prot, first, st, nprot = host(prot).view(np.uint64), host(first), host(st), host(nprot)
    for j, r in enumerate(reps):
        code, want = O.write_batch_protect(r)
        assert int(st[j]) == code, j
        assert prot[first[j]:first[j] + nprot[j]].tolist() == want[:nprot[j]], j
    assert int(st[7]) != 0


def test_block_kv_checksums_fixtures(kv_sites):
    """Block::Initialize{Data,Index,MetaIndex}BlockProtectionInfo's kv_checksum_
    (block.cc:1113-1235) for the blocks of reference-written SSTs and damaged
    blocks, protection bytes 8 and 2"""
    base, offs, sizes, kinds, cases = kvsites.block_case(*kv_sites)
    for pb in (8, 2):
        enc, prot, first, st = engine.block_kv_checksum_batch(
            d(base), d(offs.view(np.int64)), d(sizes.view(np.int32)), d(kinds), pb)
        enc, prot, first, st = host(enc), host(prot).view(np.uint64), host(first), host(st)
        for j, c in enumerate(cases):
            nk = int(first[j + 1] - first[j])
            want = c[f"keys_{pb}"]
            if want < 0:
                assert st[j] != 0 and nk == 0, c
                continue
            assert st[j] == 0 and nk == want, (c["src"], c["kind_name"], nk, want)
            got = enc[int(first[j]) * pb:int(first[j + 1]) * pb].tobytes().hex()
            assert got == c[f"kv_checksum_{pb}"], (c["src"], c["kind_name"])
            low = [int(x) & ((1 << (8 * pb)) - 1) for x in prot[int(first[j]):int(first[j + 1])]]
            assert low == [int.from_bytes(bytes.fromhex(got)[k * pb:(k + 1) * pb], "little")
                           for k in range(nk)]


def test_block_kv_checksums_many_blocks(kv_sites):
    """every fixture block repeated 300 times at shifted offsets (35 K blocks,
    one launch): the same kv_checksum_ bytes each time"""
    base, offs, sizes, kinds, cases = kvsites.block_case(*kv_sites)
    good = [j for j, c in enumerate(cases) if c["keys_8"] > 0]
    blobs = [base[int(offs[j]):int(offs[j]) + int(sizes[j])] for j in good]
    reps = 300
    pos, parts = 0, []
    for r in range(reps):
        for j, b in zip(good, blobs):
            pos += 1 + (r + j) % 7
            parts.append((pos, j))
            pos += len(b)
    big = np.zeros(pos + 64, np.uint8)
    for (o, j), b in zip(parts, blobs * reps):
        big[o:o + len(b)] = b
    o2 = np.array([o for o, _ in parts], np.int64)
    s2 = np.array([int(sizes[j]) for _, j in parts], np.int32)
    k2 = np.array([int(kinds[j]) for _, j in parts], np.uint8)
    enc, prot, first, st = engine.block_kv_checksum_batch(d(big), d(o2), d(s2), d(k2), 8)
    enc, first, st = host(enc), host(first), host(st)
    assert (st == 0).all()
    for q, (o, j) in enumerate(parts):
        got = enc[int(first[q]) * 8:int(first[q + 1]) * 8].tobytes().hex()
        assert got == cases[j]["kv_checksum_8"], (q, j)


# ---- the block walk on the entry shapes the SST-cut fixtures never reach ------
# Every output handed to the engine is prefilled with a sentinel (0xA5 bytes,
# 0x5A5A... words) and is longer than asked for: what the kernels do not store
# fails its comparison, what they store past the capacity fails the guard check.
S8, S64, GUARD = 0xA5, 0x5A5A5A5A5A5A5A5A, 8


def du(a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).to(DEV)


def run_blocks(base_t, offs, sizes, kinds, pb, capacity):
    """one batch call into sentinel-filled outputs -> host (kv_checksums,
    prot u64, first_key i64[n + 1], status); the guard cells checked"""
    n = len(offs)
    enc = torch.full((capacity * pb + GUARD,), S8, dtype=torch.uint8, device=DEV)
    prot = torch.full((capacity + GUARD,), S64, dtype=torch.int64, device=DEV)
    first = torch.full((n + 1 + GUARD,), S64, dtype=torch.int64, device=DEV)
    status = torch.full((n + GUARD,), S8, dtype=torch.uint8, device=DEV)
    outs = (enc, prot, first, status)
    try:
        e, p, f, s = engine.block_kv_checksum_batch(
            base_t, du(offs), du(sizes), du(kinds), pb, capacity=capacity, kv_checksums=enc,
            prot=prot, first_key=first, status=status)
    except Exception as ex:
        ex.outputs = tuple(host(t) for t in outs)
        raise
    assert (host(enc)[capacity * pb:] == S8).all() and (host(prot)[capacity:] == S64).all()
    assert (host(first)[n + 1:] == S64).all() and (host(status)[n:] == S8).all()
    assert len(f) == n + 1 and len(s) == n
    return host(e), host(p).view(np.uint64), host(f), host(s)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, int(bad.size), bad[:8].tolist(), got[bad[:8]].tolist(),
                           want[bad[:8]].tolist())


def check_restated(got, blocks, pb, what):
    enc, prot, first, st = got
    wfirst, wst, wenc, wprot = kvsites.restated_batch(blocks, pb)
    same(st, wst, (what, "status"))
    same(first, wfirst, (what, "first_key"))
    same(enc, wenc, (what, "kv_checksums"))
    same(prot, wprot, (what, "prot"))


def _fixture_total(cases, pb):
    return sum(max(0, c[f"keys_{pb}"]) for c in cases)


@pytest.mark.parametrize("pb", [1, 2, 4, 8])
def test_block_kv_checksums_crafted_fixtures(pb):
    """the crafted blocks of kv_blocks (gen_kv_golden.py --kv-blocks), answered
    by the reference: multi-byte varints in shared / non_shared / value_length
    for every block kind, keys and values over every hash length class rebuilt
    from prefixes of every length mod 4, hash-index geometry, blocks of 64 KiB
    and 64 KiB + 1, first keys, damage the reference reads in bounds"""
    base, offs, sizes, kinds, cases = kvsites.block_case(*kvsites.kv_blocks())
    enc, prot, first, st = run_blocks(d(base), offs, sizes, kinds, pb, _fixture_total(cases, pb))
    kvsites.check_block_results(cases, pb, enc, prot, first, st)
    for j, c in enumerate(cases):  # bad contents vs bad entry: as the restatement tells them apart
        blk = base[int(offs[j]):int(offs[j]) + int(sizes[j])].tobytes()
        assert st[j] == O.block_kv_checksums(blk, int(kinds[j]), pb)[0], c["name"]


@pytest.mark.parametrize("pb", [1, 2, 4, 8])
@pytest.mark.parametrize("shift", [4, 8, 12])
def test_block_kv_checksums_shifted_base(shift, pb):
    """the same batch with base 4, 8 and 12 bytes past 16-byte alignment, every
    protection width at each"""
    base, offs, sizes, kinds, cases = kvsites.block_case(*kvsites.kv_blocks())
    buf = torch.zeros(len(base) + 64, dtype=torch.uint8, device=DEV)
    at = (-buf.data_ptr()) % 16 + shift
    view = buf[at:at + len(base)]
    view.copy_(d(base))
    assert view.data_ptr() % 16 == shift and view.is_contiguous()
    enc, prot, first, st = run_blocks(view, offs, sizes, kinds, pb, _fixture_total(cases, pb))
    kvsites.check_block_results(cases, pb, enc, prot, first, st)


_batch = {}


def random_batch():
    if not _batch:
        _batch["b"] = blockgen.batch(np.random.default_rng(0xB10C), 3 * 2048 + 5)
    return _batch["b"]


@pytest.mark.parametrize("n,pb", [(3 * 2048 + 5, 8), (2046, 1), (2047, 2), (2048, 4), (2049, 8)])
def test_block_kv_checksums_random_batch_vs_restatement(n, pb):
    """n blockgen blocks (1-8 entries mostly, a tail of larger ones; every kind
    and flag; starts at every offset mod 16, descriptors permuted; blocks
    without restarts, damaged blocks, blocks of 0..7 bytes and descriptors past
    base_len in between) against the oracle's restatement: all n + 1 first_key
    values -- a scan over 2048-value tiles, n + 1 on both sides of the tile
    edge --, every status, checksum byte and protection value"""
    base, offs, sizes, kinds, blocks = random_batch()
    offs, sizes, kinds, blocks = offs[:n], sizes[:n], kinds[:n], blocks[:n]
    want = kvsites.restated_batch(blocks, pb)
    assert {0, 1, 2, 3} <= set(want[1].tolist()) and set(kinds.tolist()) >= {0, 1, 2, 5, 9, 13}
    assert len({int(o) % 16 for o in offs}) == 16
    got = run_blocks(d(base), offs, sizes, kinds, pb, int(want[0][-1]))
    check_restated(got, blocks, pb, n)


def test_block_kv_checksums_scratch_larger_than_buffer():
    """1000-byte keys sharing 990 bytes with their predecessor: the rebuilt keys
    (the scratch kv_kernel reads them from) take over 20 times the bytes of the
    buffer the blocks lie in, so a key bound by base_len fails"""
    rng = np.random.default_rng(31)
    blocks = []
    for b in range(6):
        key, ents = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes(), []
        for j in range(64):
            key = key[:990] + rng.integers(0, 256, 10, dtype=np.uint8).tobytes()
            ents.append((key, bytes([j]) * (j % 3)))
        kind = (blockgen.DATA, blockgen.META, blockgen.INDEX | blockgen.FULL)[b % 3]
        blocks.append((blockgen.build(ents, kind=kind, interval=64, share_over_restarts=True), kind))
    offs = np.cumsum([3] + [len(b) + 5 for b, _ in blocks[:-1]]).astype(np.uint64)
    sizes = np.array([len(b) for b, _ in blocks], np.uint32)
    kinds = np.array([k for _, k in blocks], np.uint8)
    base = np.zeros(int(offs[-1]) + int(sizes[-1]), np.uint8)
    for o, (b, _) in zip(offs, blocks):
        base[int(o):int(o) + len(b)] = np.frombuffer(b, np.uint8)
    want = kvsites.restated_batch(blocks, 8)
    assert int(want[0][-1]) == 6 * 64 and 1000 * 6 * 64 > 20 * len(base)
    check_restated(run_blocks(d(base), offs, sizes, kinds, 8, 6 * 64), blocks, 8, "scratch")


def test_block_kv_checksums_capacity():
    """capacity == total succeeds; total - 1 raises with the needed total and
    stores no checksum or protection value; a batch without keys succeeds with
    capacity 0"""
    from forst_amd import ForstError

    base, offs, sizes, kinds, blocks = random_batch()
    n = 700
    offs, sizes, kinds, blocks = offs[:n], sizes[:n], kinds[:n], blocks[:n]
    want = kvsites.restated_batch(blocks, 4)
    total = int(want[0][-1])
    g = d(base)
    check_restated(run_blocks(g, offs, sizes, kinds, 4, total), blocks, 4, "capacity == total")
    with pytest.raises(ForstError) as ei:
        run_blocks(g, offs, sizes, kinds, 4, total - 1)
    assert f"< {total} keys" in str(ei.value)
    enc, prot, first, status = ei.value.outputs
    assert (enc == S8).all() and (prot.view(np.uint64) == S64).all()
    # first_key and status are expected to be written: the count pass that
    # finds the needed total fills them before the capacity is checked
    same(first[:n + 1], want[0], ("capacity - 1", "first_key"))
    same(status[:n], want[1], ("capacity - 1", "status"))
    assert (first[n + 1:] == S64).all() and (status[n:] == S8).all()
    # no keys at all: blocks without restarts, damaged blocks, descriptors past the buffer
    _, o2, s2, k2, all_blocks = random_batch()
    none = [j for j, b in enumerate(all_blocks)
            if b is None or kvsites.restated_batch([b], 4)[0][-1] == 0][:300]
    blocks0 = [all_blocks[j] for j in none]
    assert len(blocks0) == 300
    got = run_blocks(g, o2[none], s2[none], k2[none], 4, 0)
    check_restated(got, blocks0, 4, "no keys")
    assert len(got[0]) == 0 and len(got[1]) == 0 and (got[2] == 0).all()


def test_write_batch_long_varints():
    """WriteBatch reps with a 3-byte length and 3..5-byte column family varints
    (kv_blocks), answered by the reference's WriteBatch::Iterate"""
    base, offs, lens, reps = kvsites.write_batch_case(*kvsites.kv_blocks())
    prot, first, st, nprot = engine.write_batch_protect_batch(
        d(base), d(offs.view(np.int64)), d(lens.view(np.int32)))
    prot, first, st, nprot = host(prot).view(np.uint64), host(first), host(st), host(nprot)
    for j, (name, status, want) in enumerate(reps):
        assert O.WB_STATUS[int(st[j])] == status, name
        got = prot[first[j]:first[j] + nprot[j]]
        assert got.tolist() == [int(x) for x in want], name
        code, owant = O.write_batch_protect(base[int(offs[j]):int(offs[j]) + int(lens[j])].tobytes())
        assert code == int(st[j]) and owant == got.tolist(), name
