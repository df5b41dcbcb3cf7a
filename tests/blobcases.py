"""tests/blobcases.py -- TEST INFRASTRUCTURE ONLY: the blob-record batches that
tests/test_emu_blob.py runs on the SIMT emulator and tests/test_gpu_blob.py on
the device, and the comparison of a run against the restatement
(tests/blobfile.py).

A runner has
  verify(buf, offs, eks, evs, ukeys, base_len) -> (status, header_crc, blob_crc, mismatches)
  write(buf, offs, base_len)                   -> (buffer, status, header_crc, blob_crc)
with every result array pre-filled with dispatch.SENTINEL32 / SENTINEL8 and
guard slots behind it (the runner asserts that none beyond n was written).
"""
import ctypes

import numpy as np

import blobfile as B
import dispatch as D

GUARD = 3
COUNTS = [1, 63, 64, 65, 255, 256, 257]
PAYLOADS = [0, 1, 3, 4, 255, 256, 257, 1023, 1024, 1025, 4096 + 5]


def bind(L):
    """the blob entry points of a library with the engine's C ABI"""
    vp, u64, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    L.forst_blob_verify_batch.restype = i
    L.forst_blob_verify_batch.argtypes = [vp, u64, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, u64, vp]
    L.forst_blob_record_crc_batch.restype = i
    L.forst_blob_record_crc_batch.argtypes = [vp, u64, vp, vp, vp, vp, u64, vp]
    L.forst_blob_verify_files.restype = i
    L.forst_blob_verify_files.argtypes = [vp, vp, vp, vp, u64, vp, u64, vp, vp]
    L.forst_blob_file_reason_text.restype = ctypes.c_char_p
    L.forst_blob_file_reason_text.argtypes = [i]
    L.forst_last_error.restype = ctypes.c_char_p
    return L


class FileResult(ctypes.Structure):
    """forst_blob_file_result"""
    _fields_ = [("status", ctypes.c_int32), ("reason", ctypes.c_int32),
                ("fail_index", ctypes.c_uint64), ("fail_offset", ctypes.c_uint64),
                ("blob_count", ctypes.c_uint64), ("total_blob_bytes", ctypes.c_uint64),
                ("column_family_id", ctypes.c_uint32), ("compression", ctypes.c_uint8),
                ("has_ttl", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 2)]


pack_keys = B.pack_keys


def sentinels(n):
    """(status, header_crc, blob_crc) result arrays of n + GUARD slots"""
    return (np.full(n + GUARD, D.SENTINEL8, np.uint8), np.full(n + GUARD, D.SENTINEL32, np.uint32),
            np.full(n + GUARD, D.SENTINEL32, np.uint32))


def check_guards(n, st, hc, bc):
    assert (st[n:] == D.SENTINEL8).all() and (hc[n:] == D.SENTINEL32).all() \
        and (bc[n:] == D.SENTINEL32).all(), "a slot beyond n was written"


class HostRunner:
    """the C ABI of a library whose 'device' is host memory (the emulator)"""

    def __init__(self, L):
        self.L = bind(L)

    @staticmethod
    def aligned(buf, misalign=0):
        raw = np.zeros(len(buf) + 64, np.uint8)
        at = (-raw.ctypes.data) % 16 + misalign
        a = raw[at:at + len(buf)]
        a[:] = buf
        return a

    def verify(self, buf, offs, eks=None, evs=None, ukeys=None, base_len=None, outputs=True):
        a = self.aligned(buf)
        offs = np.ascontiguousarray(offs, np.uint64)
        n = len(offs)
        eks = None if eks is None else np.ascontiguousarray(eks, np.uint64)
        evs = None if evs is None else np.ascontiguousarray(evs, np.uint64)
        kb, ko = pack_keys(ukeys) if ukeys is not None else (None, None)
        st, hc, bc = sentinels(n)
        mism = np.zeros(2, np.uint64)
        p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        rc = self.L.forst_blob_verify_batch(
            a.ctypes.data, len(buf) if base_len is None else base_len, offs.ctypes.data, p(eks),
            p(evs), p(kb), 0 if kb is None else len(kb), p(ko), st.ctypes.data,
            hc.ctypes.data if outputs else None, bc.ctypes.data if outputs else None,
            mism.ctypes.data if outputs else None, n, None)
        assert rc == 0, self.L.forst_last_error()
        check_guards(n, st, hc, bc)
        assert mism[1] == 0
        return st[:n], hc[:n], bc[:n], int(mism[0])

    def write(self, buf, offs, base_len=None):
        a = self.aligned(buf)
        offs = np.ascontiguousarray(offs, np.uint64)
        n = len(offs)
        st, hc, bc = sentinels(n)
        rc = self.L.forst_blob_record_crc_batch(a.ctypes.data, len(buf) if base_len is None else base_len,
                                                offs.ctypes.data, st.ctypes.data, hc.ctypes.data,
                                                bc.ctypes.data, n, None)
        assert rc == 0, self.L.forst_last_error()
        check_guards(n, st, hc, bc)
        return a.copy(), st[:n], hc[:n], bc[:n]


# ---- comparison ---------------------------------------------------------------

def check_verify(run, buf, offs, eks=None, evs=None, ukeys=None, base_len=None, nthreads=1):
    """one verify call against the restatement -> the expected statuses"""
    est, ehc, ebc = B.verify_records(buf, offs, eks, evs, ukeys, base_len, nthreads=nthreads)
    st, hc, bc, mism = run.verify(buf, offs, eks, evs, ukeys, base_len)
    bad = np.nonzero(st != est)[0]
    assert len(bad) == 0, (bad[:8], st[bad[:8]], est[bad[:8]])
    assert (hc == ehc).all(), np.nonzero(hc != ehc)[0][:8]
    assert (bc == ebc).all(), np.nonzero(bc != ebc)[0][:8]
    assert mism == int((est != 0).sum())
    return est


def check_write(run, buf, offs, base_len=None, nthreads=1):
    """one writer call against the restatement -> the buffer it left"""
    ebuf, est, ehc, ebc = B.write_records(buf, offs, base_len, nthreads=nthreads)
    gbuf, st, hc, bc = run.write(buf, offs, base_len)
    assert (st == est).all(), (st, est)
    assert (hc == ehc).all() and (bc == ebc).all()
    diff = np.nonzero(gbuf != ebuf)[0]
    assert len(diff) == 0, diff[:8]
    return gbuf


# ---- batches ------------------------------------------------------------------

def layout(recs, starts=None, tail=0, seed=1):
    """encoded records in one buffer: record i at the next offset whose low 4
    bits are starts[i] (None: back to back), random bytes in the gaps and in
    the `tail` bytes behind the last record -> (uint8 array, offsets u64)"""
    rng = np.random.default_rng(seed)
    parts, offs, pos = [], [], 0
    for i, r in enumerate(recs):
        if starts is not None:
            pad = (starts[i] - pos) % 16
            parts.append(rng.integers(0, 256, pad, dtype=np.uint8).tobytes())
            pos += pad
        offs.append(pos)
        parts.append(r)
        pos += len(r)
    parts.append(rng.integers(0, 256, tail, dtype=np.uint8).tobytes())
    return np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(offs, np.uint64)


def kvs(n, seed, kmax=24, vmax=300):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, int(rng.integers(1, kmax + 1)), dtype=np.uint8).tobytes(),
             rng.integers(0, 256, int(rng.integers(0, vmax + 1)), dtype=np.uint8).tobytes())
            for _ in range(n)]


def count_batch(n, seed=7):
    """n records packed back to back, the last one ending exactly at base_len
    -> (buf, offs, key sizes, value sizes, keys)"""
    kv = kvs(n, seed + n)
    buf, offs = layout([B.record(k, v) for k, v in kv])
    return (buf, offs, np.array([len(k) for k, _ in kv], np.uint64),
            np.array([len(v) for _, v in kv], np.uint64), [k for k, _ in kv])


def aligned_batch(seed=11):
    """every payload size of PAYLOADS at every start alignment 0..15, the
    key / value split varying (key size 0, value size 0 and both 0 included)"""
    rng = np.random.default_rng(seed)
    recs, starts, ks, vs, keys = [], [], [], [], []
    for a in range(16):
        for p in PAYLOADS:
            k = min(p, (5 * a + p) % 31)
            pay = rng.integers(0, 256, p, dtype=np.uint8).tobytes()
            recs.append(B.record(pay[:k], pay[k:]))
            starts.append(a)
            ks.append(k)
            vs.append(p - k)
            keys.append(pay[:k])
    buf, offs = layout(recs, starts)
    return buf, offs, np.array(ks, np.uint64), np.array(vs, np.uint64), keys


def edge_batch(seed=23):
    """every status code, and the range arithmetic at its limits.
    -> dict(buf, offs, eks, evs, ukeys, expect_plain, expect_sizes, expect_keys):
    the statuses the table of forst_checksum.h gives without expectations,
    with expected sizes, and with sizes and user keys"""
    kv = kvs(9, seed, kmax=40, vmax=700)
    kv[0] = (kv[0][0], kv[0][1] + bytes(300))  # a long payload in front
    recs = [B.record(k, v) for k, v in kv]
    big = 2**64 - 1
    # headers whose sizes are not what follows (their header CRCs are sound)
    recs.append(B.record(b"", b"", key_size=big, value_size=0))          # 9: key_size 2^64 - 1
    recs.append(B.record(b"", b"", key_size=big, value_size=2))          # 10: the sum wraps
    recs.append(B.record(b"", b"", key_size=5, value_size=2**32 - 5))    # 11: sum = 2^32
    recs.append(B.record(b"", b"", key_size=5, value_size=2**32 - 6))    # 12: 2^32 - 1, past the end
    recs.append(B.record(b"kk", b"the last record ends at base_len"))     # 13
    buf, offs = layout(recs, starts=[(3 * i + 1) % 16 for i in range(len(recs))])
    n_rec = len(recs)
    eks = [len(k) for k, _ in kv] + [big, big, 5, 5, 2]
    evs = [len(v) for _, v in kv] + [0, 2, 2**32 - 5, 2**32 - 6, 32]
    ukeys = [k for k, _ in kv] + [b"", b"", b"", b"", b"kk"]
    o = [int(x) for x in offs]
    buf[o[1] + 3] ^= 0x10                      # 1: a header byte
    buf[o[2] + 25] ^= 0x01                     # 2: the stored header CRC
    eks[3] += 1                                # 3: key size expectation
    evs[4] += 1                                # 4: value size expectation
    ukeys[5] = bytes([ukeys[5][0] ^ 0x80]) + ukeys[5][1:]  # 5: a wrong key of the right length
    buf[o[6] + 32] ^= 0x04                     # 6: a key byte in the file
    buf[o[7] + 32 + eks[7] + evs[7] - 1] ^= 0x40           # 7: the last value byte
    buf[o[8] + 30] ^= 0x02                     # 8: the stored blob CRC
    # offsets that are not records at all
    n = len(buf)
    extra = [n - 31, n - 1, n, n + 1, 2**64 - 40, 2**64 - 1, n - 32]
    offs = np.concatenate([offs, np.array(extra, np.uint64)])
    eks += [0] * len(extra)
    evs += [0] * len(extra)
    ukeys += [b""] * len(extra)
    last = B.HEADER_CRC  # n - 32: 32 readable bytes that are no header
    plain = [0, 1, 1, 0, 0, 0, 5, 5, 5, 7, 7, 7, 6, 0] + [6] * 6 + [last]
    sizes = [0, 1, 1, 2, 3, 0, 5, 5, 5, 7, 7, 7, 6, 0] + [6] * 6 + [last]
    keys = [0, 1, 1, 2, 3, 4, 4, 5, 5, 7, 7, 7, 6, 0] + [6] * 6 + [last]
    assert len(plain) == len(offs) == n_rec + len(extra)
    return dict(buf=buf, offs=offs, eks=np.array(eks, np.uint64), evs=np.array(evs, np.uint64),
                ukeys=ukeys, expect_plain=np.array(plain, np.uint8),
                expect_sizes=np.array(sizes, np.uint8), expect_keys=np.array(keys, np.uint8))


def orders(n, seed=5):
    """file order, reversed, shuffled"""
    return [np.arange(n), np.arange(n)[::-1].copy(), np.random.default_rng(seed).permutation(n)]


def take(e, idx, with_keys=True):
    return (e["offs"][idx], e["eks"][idx], e["evs"][idx],
            [e["ukeys"][i] for i in idx] if with_keys else None)


def zero_crc_fields(buf, offs):
    out = buf.copy()
    for o in offs:
        out[int(o) + 24:int(o) + 32] = 0
    return out


def run_record_cases(run):
    """the cases both backends run; returns the set of status codes seen"""
    seen = set()
    # record counts, with and without expectations and user keys
    for n in COUNTS:
        buf, offs, ks, vs, keys = count_batch(n)
        seen |= set(check_verify(run, buf, offs).tolist())
        seen |= set(check_verify(run, buf, offs, ks, vs, keys).tolist())
    # alignments x payload sizes, file order / reversed / shuffled
    buf, offs, ks, vs, keys = aligned_batch()
    for idx in orders(len(offs)):
        est = check_verify(run, buf, offs[idx], ks[idx], vs[idx], [keys[i] for i in idx])
        assert (est == 0).all()
    assert (check_verify(run, buf, offs) == 0).all()
    # every status code; the limits of the range arithmetic
    e = edge_batch()
    for idx in orders(len(e["offs"])):
        o, ks_, vs_, uk = take(e, idx)
        assert (check_verify(run, e["buf"], o) == e["expect_plain"][idx]).all()
        assert (check_verify(run, e["buf"], o, ks_, vs_) == e["expect_sizes"][idx]).all()
        est = check_verify(run, e["buf"], o, ks_, vs_, uk)
        assert (est == e["expect_keys"][idx]).all()
        seen |= set(est.tolist())
        check_verify(run, e["buf"], o, ks_, None, uk)  # key sizes and keys, no value sizes
    # a header cut by base_len, a payload cut by it (the buffer itself is longer)
    buf, offs, ks, vs, keys = count_batch(65)
    last = int(offs[-1])
    for cut in (last + 31, last + 32 + int(ks[-1]) + int(vs[-1]) - 1, last, 31, 0):
        est = check_verify(run, buf, offs, base_len=cut)
        assert est[-1] == B.OUT_OF_RANGE
    return seen


def run_writer_cases(run):
    # write mode, then verify mode, on the same image
    buf, offs, ks, vs, keys = aligned_batch()
    for idx in orders(len(offs)):
        out = check_write(run, zero_crc_fields(buf, offs), offs[idx])
        assert (out == buf).all()  # byte for byte what BlobLogRecord::EncodeHeaderTo wrote
    assert (check_verify(run, out, offs, ks, vs, keys) == 0).all()
    # only 0, 6 and 7 exist, and nothing is written for a non-zero record
    e = edge_batch()
    before = e["buf"].copy()
    out = check_write(run, e["buf"], e["offs"])
    st = B.write_records(before, e["offs"])[1]
    assert set(st.tolist()) == {B.OK, B.OUT_OF_RANGE, B.TOO_LARGE}
    for o, s in zip(e["offs"], st):
        if s != B.OK and int(o) < len(before) - 32:
            assert (out[int(o):int(o) + 32] == before[int(o):int(o) + 32]).all()
    # a payload cut by base_len
    buf, offs, *_ = count_batch(64)
    check_write(run, zero_crc_fields(buf, offs), offs, base_len=len(buf) - 1)


def many_short_records(n, seed=31):
    """n records of 0..600 payload bytes, shuffled, with flips in headers, keys
    and values -> (buf, offs, key sizes, value sizes, keys)"""
    rng = np.random.default_rng(seed)
    ksz = rng.integers(1, 25, n)
    vsz = rng.integers(0, 577, n)
    pay = rng.integers(0, 256, int((ksz + vsz).sum()), dtype=np.uint8).tobytes()
    recs, keys, p = [], [], 0
    for k, v in zip(ksz, vsz):
        recs.append(B.record(pay[p:p + k], pay[p + k:p + k + v]))
        keys.append(pay[p:p + k])
        p += k + v
    buf, offs = layout(recs)
    for j, i in enumerate(rng.choice(n, 24, replace=False)):
        where = (3, 33, 32 + int(ksz[i]) + int(vsz[i]) - 1)[j % 3]
        buf[int(offs[i]) + where] ^= 1 << (j % 8)
    idx = rng.permutation(n)
    return (buf, offs[idx], ksz[idx].astype(np.uint64), vsz[idx].astype(np.uint64),
            [keys[i] for i in idx])


# ---- files ----------------------------------------------------------------------

def header_text(res, L):
    return L.forst_blob_file_reason_text(res.reason).decode()


def same_result(res, exp, L):
    """a forst_blob_file_result against blobfile.scan_file's dict"""
    got = dict(status=res.status, reason=res.reason, text=header_text(res, L),
               fail_index=res.fail_index, fail_offset=res.fail_offset, blob_count=res.blob_count,
               total_blob_bytes=res.total_blob_bytes, cf=res.column_family_id,
               compression=res.compression, has_ttl=res.has_ttl)
    assert got == {k: exp[k] for k in got}, (got, exp)


def damaged_files(seed=41):
    """crafted files and damaged copies of them: every file reason
    -> [(name, bytes, expect_cf or None)]"""
    kv = kvs(12, seed, kmax=60, vmax=900)
    good, offs = B.build_file(kv, cf=3, compression=0)
    out = [("good", good, 3), ("good_any_cf", good, None), ("wrong_cf", good, 4)]
    empty, _ = B.build_file([], cf=0)
    out.append(("no_record", empty, 0))
    out.append(("zero_sizes", B.build_file([(b"", b""), (b"k", b""), (b"", b"v")], cf=1)[0], 1))

    def flip(data, at, m=0x20):
        b = bytearray(data)
        b[at] ^= m
        return bytes(b)

    n = len(good)
    out += [("short", good[:61], None), ("size_62", good[:30] + good[-32:], 3),
            ("header_magic", flip(good, 1), 3), ("header_version", flip(good, 5), 3),
            ("header_ttl_flag", flip(good, 12, 1), 3), ("header_exp_range", flip(good, 20), 3),
            ("footer_magic", flip(good, n - 31), 3), ("footer_count", flip(good, n - 27), 3),
            ("footer_crc", flip(good, n - 2), 3),
            ("rec0_header", flip(good, 30 + 9), 3), ("rec0_key", flip(good, 30 + 32), 3),
            ("rec5_value", flip(good, offs[5] + 32 + len(kv[5][0]) + len(kv[5][1]) - 1), 3),
            ("last_blob_crc", flip(good, offs[-1] + 29), 3),
            ("last_header_crc", flip(good, offs[-1] + 24), 3),
            # a size damaged in record 3: its header CRC fails first, whatever the walk met behind
            ("rec3_size", flip(good, offs[3] + 1, 0x01), 3)]
    # a sound record whose payload crosses the footer; bytes too few for a header
    cross = bytearray(good[:offs[-1]]) + B.record(b"k", b"v" * 10, value_size=5000) + good[-32:]
    out.append(("crosses_footer", bytes(cross), 3))
    out.append(("trailing_bytes", good[:-32] + bytes(7) + good[-32:], 3))
    # one record fewer than the footer says; a footer with an expiration range
    out.append(("count_mismatch", good[:offs[-1]] + good[-32:], 3))
    out.append(("footer_ttl", good[:-32] + B.file_footer(len(kv), (5, 9)), 3))
    ttl = B.file_header(cf=3, has_ttl=True, exp_range=(1, 2)) + good[30:]
    out.append(("ttl_header", ttl, 3))
    return out


def big_batch(n, lo=16, hi=2048, flips=64, seed=77, nthreads=1):
    """n records with payloads log-uniform lo..hi bytes packed in file order
    (built with array operations: no Python loop over the records), `flips`
    flipped bytes spread over headers, keys and values, shuffled order
    -> (buf, offs, key sizes, value sizes, (packed user keys, offsets))"""
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    pay = np.exp(rng.uniform(np.log(lo), np.log(hi + 1), n)).astype(np.int64).clip(lo, hi)
    ks = np.minimum(rng.integers(1, 33, n), pay)
    vs = pay - ks
    offs = np.cumsum(pay + 32) - (pay + 32)
    total = int(offs[-1] + pay[-1] + 32)
    buf = rng.integers(0, 256, total, dtype=np.uint8)
    heads = np.zeros((n, 32), np.uint8)
    heads[:, 0:8] = ks.astype("<u8").view(np.uint8).reshape(n, 8)
    heads[:, 8:16] = vs.astype("<u8").view(np.uint8).reshape(n, 8)
    h24 = np.ascontiguousarray(heads[:, :24]).reshape(-1)
    hc = B.mask32(O.crc32c_batch(h24, np.arange(n, dtype=np.uint64) * np.uint64(24),
                                 np.full(n, 24, np.uint32), nthreads=nthreads))
    bc = B.mask32(O.crc32c_batch(buf, (offs + 32).astype(np.uint64), pay.astype(np.uint32),
                                 nthreads=nthreads))
    heads[:, 24:28] = hc.astype("<u4").view(np.uint8).reshape(n, 4)
    heads[:, 28:32] = bc.astype("<u4").view(np.uint8).reshape(n, 4)
    buf[offs[:, None] + np.arange(32)] = heads
    # the user keys, taken before the damage
    kstart = np.cumsum(ks) - ks
    within = np.arange(int(ks.sum())) - np.repeat(kstart, ks)
    kb = buf[np.repeat(offs + 32, ks) + within].copy()
    for j, i in enumerate(rng.choice(n, flips, replace=False)):
        where = (int(rng.integers(0, 32)), 32 + int(rng.integers(0, ks[i])),
                 32 + int(ks[i]) + int(rng.integers(0, max(1, vs[i]))) if vs[i] else 32)[j % 3]
        buf[int(offs[i]) + where] ^= 1 << (j % 8)
    idx = rng.permutation(n)
    return (buf, offs[idx].astype(np.uint64), ks[idx].astype(np.uint64), vs[idx].astype(np.uint64),
            (kb, kstart[idx].astype(np.uint64)))
