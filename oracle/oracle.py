"""oracle/oracle.py -- TEST INFRASTRUCTURE ONLY.

ctypes bindings for the CPU restatement in oracle/oracle.c.  Imported only by
tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg -- never by the
product package (forst_amd/), which has no CPU fallback.
"""
import ctypes
import os
import struct
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "build", "liboracle.so")
_lib = None

kNoChecksum, kCRC32c, kxxHash, kxxHash64, kXXH3 = 0, 1, 2, 3, 4

_u8p = ctypes.c_void_p


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            build()
        L = ctypes.CDLL(_LIB_PATH)
        u32, u64, sz, vp, i = (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t,
                               ctypes.c_void_p, ctypes.c_int)
        sigs = {
            "oracle_crc32c_extend": (u32, [u32, vp, sz]),
            "oracle_crc32c_extend_fast": (u32, [u32, vp, sz]),
            "oracle_crc32c_value": (u32, [vp, sz]),
            "oracle_crc32c_combine": (u32, [u32, u32, sz]),
            "oracle_crc32c_mask": (u32, [u32]),
            "oracle_crc32c_unmask": (u32, [u32]),
            "oracle_crc32c_shift": (u32, [u32, u64]),
            "oracle_xxh3_64": (u64, [vp, sz]),
            "oracle_xxh32": (u32, [vp, sz, u32]),
            "oracle_xxh64": (u64, [vp, sz, u64]),
            "oracle_compute_builtin_checksum": (u32, [i, vp, sz]),
            "oracle_compute_builtin_checksum_with_last_byte": (u32, [i, vp, sz, ctypes.c_uint8]),
            "oracle_checksum_modifier_for_context": (u32, [u32, u64]),
            "oracle_verify_block_checksum": (i, [i, vp, sz, u32, vp, vp]),
            "oracle_block_checksum_batch": (None, [i, vp, vp, vp, vp, vp, vp, sz, i]),
            "oracle_block_verify_batch": (u64, [i, vp, vp, vp, vp, vp, vp, sz, i]),
            "oracle_crc32c_batch": (None, [vp, vp, vp, vp, sz, i]),
            "oracle_xxh3_batch": (None, [vp, vp, vp, vp, sz, i]),
            "oracle_wal_record_crc": (u32, [i, u32, vp, sz]),
            "oracle_wal_record_xxh3_batch": (None, [vp, vp, vp, u64, u32, vp, vp, sz, i]),
            "oracle_wal_framed_size": (u64, [vp, sz, i]),
            "oracle_wal_frame": (u64, [vp, vp, sz, i, u32, vp, vp, vp, vp]),
            "oracle_wal_verify": (u64, [vp, u64, vp, u64, vp, i]),
            "oracle_wal_verify_blocks": (None, [vp, u64, u32, vp, vp, vp, i]),
            "oracle_hash64": (u64, [vp, sz, u64]),
            "oracle_kv_protect": (u64, [vp, sz, vp, sz, i, i, u64, i, u32]),
            "oracle_kv_verify": (i, [u64, u32, vp]),
            "oracle_hash64_batch": (None, [vp, vp, vp, vp, u64, vp, sz]),
            "oracle_kv_protect_batch": (None, [vp, vp, vp, vp, vp, vp, vp, vp, vp, sz]),
            "oracle_memtable_verify_batch": (None, [vp, sz, vp, sz, u32, vp, vp]),
            "oracle_splitmix64": (u64, [u64]),
            "oracle_fill_stream": (None, [vp, u64, u64, u64]),
        }
        for name, (res, args) in sigs.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, (bytes, bytearray)):
        return ctypes.cast(ctypes.c_char_p(bytes(a)), ctypes.c_void_p).value
    return a.ctypes.data


def _buf(data):
    """Return (pointer, length, keepalive) for bytes / numpy uint8 data."""
    if isinstance(data, np.ndarray):
        return data.ctypes.data, data.nbytes, data
    b = ctypes.create_string_buffer(bytes(data), len(data) or 1)
    return ctypes.addressof(b), len(data), b


def crc32c_value(data):
    p, n, _k = _buf(data)
    return lib().oracle_crc32c_value(p, n)


def crc32c_extend(crc, data, fast=False):
    p, n, _k = _buf(data)
    f = lib().oracle_crc32c_extend_fast if fast else lib().oracle_crc32c_extend
    return f(crc, p, n)


def crc32c_combine(a, b, blen):
    return lib().oracle_crc32c_combine(a, b, blen)


def crc32c_shift(state, nbytes):
    return lib().oracle_crc32c_shift(state, nbytes)


def mask(c):
    return lib().oracle_crc32c_mask(c)


def unmask(c):
    return lib().oracle_crc32c_unmask(c)


def xxh3_64(data):
    p, n, _k = _buf(data)
    return lib().oracle_xxh3_64(p, n)


def xxh32(data, seed=0):
    p, n, _k = _buf(data)
    return lib().oracle_xxh32(p, n, seed)


def xxh64(data, seed=0):
    p, n, _k = _buf(data)
    return lib().oracle_xxh64(p, n, seed)


def compute_builtin_checksum(ctype, data):
    p, n, _k = _buf(data)
    return lib().oracle_compute_builtin_checksum(ctype, p, n)


def compute_builtin_checksum_with_last_byte(ctype, data, last):
    p, n, _k = _buf(data)
    return lib().oracle_compute_builtin_checksum_with_last_byte(ctype, p, n, last & 0xFF)


def checksum_modifier_for_context(base, offset):
    return lib().oracle_checksum_modifier_for_context(base, offset)


def verify_block_checksum(ctype, data, block_size, modifier=0):
    p, _n, _k = _buf(data)
    c = ctypes.c_uint32()
    s = ctypes.c_uint32()
    ok = lib().oracle_verify_block_checksum(ctype, p, block_size, modifier,
                                            ctypes.byref(c), ctypes.byref(s))
    return bool(ok), c.value, s.value


def block_checksum_batch(ctype, base, offsets, sizes, last_bytes=None, modifiers=None,
                         nthreads=1):
    out = np.zeros(len(offsets), dtype=np.uint32)
    lib().oracle_block_checksum_batch(ctype, _ptr(base), _ptr(offsets), _ptr(sizes),
                                      _ptr(last_bytes), _ptr(modifiers), _ptr(out),
                                      len(offsets), nthreads)
    return out


def block_verify_batch(ctype, base, offsets, sizes, modifiers=None, nthreads=1):
    computed = np.zeros(len(offsets), dtype=np.uint32)
    ok = np.zeros(len(offsets), dtype=np.uint8)
    bad = lib().oracle_block_verify_batch(ctype, _ptr(base), _ptr(offsets), _ptr(sizes),
                                          _ptr(modifiers), _ptr(computed), _ptr(ok),
                                          len(offsets), nthreads)
    return computed, ok, bad


def crc32c_batch(base, offsets, lengths, nthreads=1):
    out = np.zeros(len(offsets), dtype=np.uint32)
    lib().oracle_crc32c_batch(_ptr(base), _ptr(offsets), _ptr(lengths), _ptr(out),
                              len(offsets), nthreads)
    return out


def xxh3_batch(base, offsets, lengths, nthreads=1):
    out = np.zeros(len(offsets), dtype=np.uint64)
    lib().oracle_xxh3_batch(_ptr(base), _ptr(offsets), _ptr(lengths), _ptr(out),
                            len(offsets), nthreads)
    return out


def wal_record_xxh3_batch(log, phys_offsets, phys_lengths, first, hs=7, nthreads=1):
    """XXH3 of every logical record: record j = payloads of physical records
    [first[j], first[j+1]) (db/log_reader.cc:95-165)"""
    po = np.ascontiguousarray(phys_offsets, np.uint64)
    pl = np.ascontiguousarray(phys_lengths, np.uint32)
    fi = np.ascontiguousarray(first, np.uint64)
    out = np.zeros(len(fi), dtype=np.uint64)
    lib().oracle_wal_record_xxh3_batch(_ptr(log), _ptr(po), _ptr(pl), len(po), hs, _ptr(fi),
                                       _ptr(out), len(fi), nthreads)
    return out


def host_threads():
    """CPU threads this process may use: the cgroup cpu.max quota where one is
    set (the GPU box: 16), else the affinity mask"""
    n = len(os.sched_getaffinity(0))
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(q) // int(per)))
    except (OSError, ValueError):
        pass
    return max(1, n)


def wal_record_crc(rtype, log_number, payload):
    p, n, _k = _buf(payload)
    return lib().oracle_wal_record_crc(rtype, log_number, p, n)


def wal_frame(payloads, lengths, recyclable=False, log_number=0):
    """Frame logical records like log::Writer::AddRecord.  Returns
    (buffer, phys_offsets, phys_lengths)."""
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    payloads = np.ascontiguousarray(payloads, dtype=np.uint8)
    total = lib().oracle_wal_framed_size(_ptr(lengths), len(lengths), int(recyclable))
    dst = np.zeros(total, dtype=np.uint8)
    # upper bound on physical records: one per 32 KiB block + one per record
    cap = len(lengths) + total // 32768 + 2
    offs = np.zeros(cap, dtype=np.uint64)
    lens = np.zeros(cap, dtype=np.uint32)
    nphys = ctypes.c_uint64()
    lib().oracle_wal_frame(_ptr(payloads), _ptr(lengths), len(lengths), int(recyclable),
                           log_number, _ptr(dst), _ptr(offs), _ptr(lens),
                           ctypes.byref(nphys))
    n = nphys.value
    return dst, offs[:n].copy(), lens[:n].copy()


def wal_verify(buf, nthreads=1):
    bad = ctypes.c_uint64()
    n = lib().oracle_wal_verify(_ptr(buf), buf.nbytes, None, 0, ctypes.byref(bad), nthreads)
    return n, bad.value


def wal_verify_blocks(buf, log_number=0, nthreads=1):
    """per 32 KiB log block: (status, records verified before the first
    failure, offset of the failing header / end of parsing), as
    forst_wal_verify_batch reports them (db/log_reader.cc:450-531)"""
    nb = (buf.nbytes + 32767) // 32768
    st = np.zeros(nb, np.uint8)
    nr = np.zeros(nb, np.uint32)
    fo = np.zeros(nb, np.uint32)
    lib().oracle_wal_verify_blocks(_ptr(buf), buf.nbytes, log_number, _ptr(st), _ptr(nr), _ptr(fo),
                                   nthreads)
    return st, nr, fo


KV_SEED_K, KV_SEED_V = 0, 0xD28AAD72F49BD50B  # db/kv_checksum.h:84-88
KV_SEED_O, KV_SEED_S, KV_SEED_C = 0xA5155AE5E937AA16, 0x77A00858DDD37F21, 0x4A2AB5CBD26F542C


def hash64(data, seed=0):
    """util/hash.cc:81 Hash64 = XXPH3_64bits_withSeed (util/xxph3.h:1733)"""
    p, n, _k = _buf(data)
    return lib().oracle_hash64(p, n, seed & (2**64 - 1))


def kv_protect(key, value, op_type=None, seq=None, cf=None):
    """ProtectionInfo64().ProtectKV[O](...)[.ProtectS(seq)][.ProtectC(cf)]"""
    kp, kn, _k1 = _buf(key)
    vp, vn, _k2 = _buf(value)
    return lib().oracle_kv_protect(kp, kn, vp, vn, -1 if op_type is None else op_type,
                                   seq is not None, seq or 0, cf is not None, cf or 0)


def hash64_batch(base, offsets, lengths, seeds=None, seed=0):
    out = np.zeros(len(offsets), dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    lengths = np.ascontiguousarray(lengths, np.uint32)
    lib().oracle_hash64_batch(_ptr(base), _ptr(offsets), _ptr(lengths),
                              _ptr(None if seeds is None else np.ascontiguousarray(seeds, np.uint64)),
                              seed, _ptr(out), len(offsets))
    return out


def kv_protect_batch(base, key_offsets, key_sizes, value_offsets, value_sizes, op_types=None,
                     seqnos=None, cf_ids=None):
    n = len(key_offsets)
    out = np.zeros(n, dtype=np.uint64)
    arrs = [np.ascontiguousarray(key_offsets, np.uint64), np.ascontiguousarray(key_sizes, np.uint32),
            np.ascontiguousarray(value_offsets, np.uint64),
            np.ascontiguousarray(value_sizes, np.uint32)]
    opt = [None if op_types is None else np.ascontiguousarray(op_types, np.uint8),
           None if seqnos is None else np.ascontiguousarray(seqnos, np.uint64),
           None if cf_ids is None else np.ascontiguousarray(cf_ids, np.uint32)]
    lib().oracle_kv_protect_batch(_ptr(base), *[_ptr(a) for a in arrs], *[_ptr(a) for a in opt],
                                  _ptr(out), n)
    return out


def memtable_verify_batch(base, base_len, offsets, prot_bytes):
    """MemTable::VerifyEntryChecksum per encoded entry (db/memtable.cc:273-307):
    (computed, status) -- status codes as include/forst_checksum.h"""
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = len(offsets)
    comp = np.zeros(n, np.uint64)
    st = np.zeros(n, np.uint8)
    lib().oracle_memtable_verify_batch(_ptr(base), base_len, _ptr(offsets), n, prot_bytes,
                                       _ptr(comp), _ptr(st))
    return comp, st


MEM_STATUS = {0: "OK",
              1: "Corruption: Unable to parse internal key length",
              2: "Corruption: Memtable entry internal key length too short.",
              3: "Corruption: Unable to parse internal key value",
              4: "Corruption: Corrupted memtable entry, per key-value checksum verification "
                 "failed."}  # db/memtable.cc:280-306

WB_STATUS = {0: "OK", 1: "Corruption: malformed WriteBatch (too small)",
             2: "Corruption: bad WriteBatch Put", 3: "Corruption: bad WriteBatch Delete",
             4: "Corruption: bad WriteBatch DeleteRange", 5: "Corruption: bad WriteBatch Merge",
             6: "Corruption: bad WriteBatch BlobIndex", 7: "Corruption: bad WriteBatch Blob",
             8: "Corruption: bad EndPrepare XID", 9: "Corruption: bad commit timestamp",
             10: "Corruption: bad Commit XID", 11: "Corruption: bad Rollback XID",
             12: "Corruption: bad WriteBatch PutEntity", 13: "Corruption: unknown WriteBatch tag",
             14: "Corruption: WriteBatch has wrong count"}  # db/write_batch.cc:361-716

# ReadRecordFromWriteBatch (write_batch.cc:361-475): tag -> (has cf, parts, error,
# ProtectionInfoUpdater op type (write_batch.cc:3023-3052) or None)
_WB_TAGS = {0x05: (1, "kv", 2, 0x01), 0x01: (0, "kv", 2, 0x01),
            0x04: (1, "k", 3, 0x00), 0x08: (1, "k", 3, 0x07), 0x00: (0, "k", 3, 0x00),
            0x07: (0, "k", 3, 0x07), 0x0E: (1, "kv", 4, 0x0F), 0x0F: (0, "kv", 4, 0x0F),
            0x06: (1, "kv", 5, 0x02), 0x02: (0, "kv", 5, 0x02), 0x10: (1, "kv", 6, 0x11),
            0x11: (0, "kv", 6, 0x11), 0x17: (1, "kv", 12, 0x16), 0x16: (0, "kv", 12, 0x16),
            0x03: (0, "x", 7, None), 0x0D: (0, "", 0, None), 0x09: (0, "", 0, None),
            0x12: (0, "", 0, None), 0x13: (0, "", 0, None), 0x0A: (0, "x", 8, None),
            0x0B: (0, "x", 10, None), 0x15: (0, "kx", 9, None), 0x0C: (0, "x", 11, None)}


def _wb_varint(b, p, end):
    """GetVarint32 over input [p, end): (value, next p) or None"""
    r = 0
    for j in range(5):
        if p + j >= end:
            return None
        x = b[p + j]
        r |= (x & 127) << (7 * j)
        if not x & 128:
            return r & 0xFFFFFFFF, p + j + 1
    return None


def write_batch_protect(rep):
    """WriteBatchInternal::UpdateProtectionInfo(wb, 8) restated
    (write_batch.cc:3164-3181, Iterate :477-716, ReadRecordFromWriteBatch
    :361-475): (status code as WB_STATUS, [protection values of the data
    records in order])"""
    b = bytes(rep)
    if len(b) < 12:
        return 1, []
    count = struct.unpack_from("<I", b, 8)[0]
    p, end, out = 12, len(b), []
    while p < end:
        tag = b[p]
        p += 1
        if tag not in _WB_TAGS:
            return 13, out
        has_cf, parts, err, op = _WB_TAGS[tag]
        cf, sl = 0, []
        if has_cf:
            v = _wb_varint(b, p, end)
            if v is None:
                return err, out
            cf, p = v
        for i, part in enumerate(parts):
            v = _wb_varint(b, p, end)
            if v is None or end - v[1] < v[0]:
                return (10 if tag == 0x15 and i == 1 else err), out
            sl.append(b[v[1]:v[1] + v[0]])
            p = v[1] + v[0]
        if op is not None:
            out.append(kv_protect(sl[0], sl[1] if len(sl) > 1 else b"", op, cf=cf))
    return (14 if len(out) != count else 0), out


BLK_STATUS = {0: "OK", 1: "bad block contents", 2: "Corruption: bad entry in block"}
_BLK_MAX_HASH_INDEX = 1 << 16  # kMaxBlockSizeSupportedByHashIndex (data_block_hash_index.h:71)


class NoReferenceTwin(Exception):
    """the reference cannot answer this block: it would not terminate, or would
    write past its kv_checksum_ allocation"""


def _varint64(b, p, end):
    """GetVarint64Ptr over [p, end) (util/coding.cc): (value, next p) or None"""
    r = 0
    for j in range(10):
        if p + j >= end:
            return None
        x = b[p + j]
        r |= (x & 127) << (7 * j)
        if not x & 128:
            return r & (2**64 - 1), p + j + 1
    return None


class _BlockIter:
    """BlockIter<TValue> (table/block_based/block.h, block.cc:635-774) as the
    release build runs it: the asserts of DecodeEntry / DecodeCurrentValue are
    no checks.  kind 0 data (DecodeEntry), 1 index (DecodeEntryV4 +
    IndexValue::DecodeFrom, or DecodeEntry when value_is_full), 2 metaindex
    (CheckAndDecodeEntry)."""

    def __init__(self, b, restarts, num_restarts, kind):
        self.b, self.n = b, len(b)
        self.restarts, self.num_restarts = restarts, num_restarts
        self.k = kind & 3
        self.delta_v4 = self.k == 1 and not kind & 4
        self.first_key = bool(kind & 8)
        self.ok = True
        self.valid = False
        self.key, self.v0, self.vlen = b"", restarts, 0
        self.stats = None  # counters of the final walk (block_entries(stats=))

    def _count(self, what):
        if self.stats is not None:
            self.stats[what] = self.stats.get(what, 0) + 1

    def restart_point(self, i):  # GetRestartPoint
        return struct.unpack_from("<I", self.b, self.restarts + 4 * i)[0]

    def next_entry_offset(self):
        return self.v0 + self.vlen

    def seek_to_restart_point(self, i):
        self.key = b""
        self.v0, self.vlen = self.restart_point(i), 0

    def _corrupt(self):  # CorruptionError(): "bad entry in block"
        self.ok = self.valid = False
        self.key = b""
        return False

    def parse_next(self):
        """ParseNextKey<DecodeEntryFunc> (+ IndexBlockIter::DecodeCurrentValue)"""
        b, limit, n = self.b, self.restarts, self.n
        p = self.next_entry_offset()
        if p >= limit:
            self.valid = False
            return False
        checked = self.k == 2
        if (checked or self.delta_v4) and limit - p < 3:
            return self._corrupt()
        if p + 3 > n:
            return self._corrupt()  # no reference twin: header bytes past the block
        shared, non_shared = b[p], b[p + 1]
        vlen = 0 if self.delta_v4 else b[p + 2]
        if (shared | non_shared | vlen) < 128:
            p += 2 if self.delta_v4 else 3
        else:
            self._count("entries_slow_path")
            for which in range(2 if self.delta_v4 else 3):
                v = _wb_varint(b, p, limit)
                if v is None:
                    return self._corrupt()
                self._count("varint_%d_bytes" % (v[1] - p))
                if which == 0:
                    shared = v[0]
                elif which == 1:
                    non_shared = v[0]
                else:
                    vlen = v[0]
                p = v[1]
        if checked and limit - p < ((non_shared + vlen) & 0xFFFFFFFF):
            return self._corrupt()
        if p + non_shared + vlen > n:
            return self._corrupt()  # no reference twin: key / value past the block
        if len(self.key) < shared:
            return self._corrupt()
        self.key = self.key[:shared] + b[p:p + non_shared]
        v0 = p + non_shared
        if self.delta_v4:
            if v0 > limit:
                return self._corrupt()  # no reference twin: Slice of negative size
            q = v0  # IndexValue::DecodeFrom (format.cc:123-148); a failure only asserts
            good = True
            for _ in range(1 if shared else 2):  # delta size | BlockHandle offset, size
                v = _varint64(b, q, limit)
                if v is None:
                    good = False
                    break
                q = v[1]
            if good and self.first_key:  # GetLengthPrefixedSlice: the varint stays consumed
                v = _wb_varint(b, q, limit)
                if v is not None:
                    q = v[1] + (v[0] if limit - v[1] >= v[0] else 0)
            vlen = q - v0
        self.v0, self.vlen = v0, vlen
        self.valid = True
        return True


def _block_geometry(b):
    """Block::Block (block.cc:1058-1111, NumRestarts :1016, IndexType :1038,
    DataBlockHashIndex::Initialize): (num_restarts, restart_offset) or None for
    the size_ = 0 error marker"""
    n = len(b)
    if n < 4:
        return None
    footer = struct.unpack_from("<I", b, n - 4)[0]
    nr, hash_index = footer, False
    if n <= _BLK_MAX_HASH_INDEX:
        hash_index = bool(footer >> 31)
        nr = footer & 0x7FFFFFFF
    if not hash_index:
        ro = (n - (1 + nr) * 4) & 0xFFFFFFFF
        return None if ro > n - 4 else (nr, ro)
    if n < 6:
        return None
    size = (n - 4) & 0xFFFF
    num_buckets = struct.unpack_from("<H", b, size - 2)[0]
    map_offset = (size - 2 - num_buckets) & 0xFFFF
    ro = (map_offset - nr * 4) & 0xFFFFFFFF
    if ro > map_offset:
        return None
    if map_offset > n and nr:
        return None  # no reference twin: the restart array lies past the block
    return nr, ro


def block_entries(block_bytes, kind, stats=None):
    """-> (status, [(key bytes, value offset, value length)]) of
    Block::Initialize{Data,Index,MetaIndex}BlockProtectionInfo's walk
    (block.cc:1113-1235): GetRestartInterval and NumberOfKeys (block.h:484-512)
    first, as they can fail the block, then SeekToFirst / Next.  stats (a
    dict) counts the slow-path entries and varint widths of that last walk."""
    b = bytes(block_bytes)
    g = _block_geometry(b)
    if g is None:
        return 1, []
    nr, ro = g
    if nr == 0:
        return 0, []
    it = _BlockIter(b, ro, nr, kind)
    if it.k == 2:  # MetaBlockIter: interval 1, num_restarts_ keys (block.h:828-829)
        num_keys = nr
    else:
        interval = 0
        if nr > 1:  # GetRestartInterval
            it.seek_to_restart_point(0)
            it.parse_next()
            end_index, interval = it.restart_point(1), 1
            while it.next_entry_offset() < end_index and it.ok:
                if not it.parse_next() and it.ok:
                    raise NoReferenceTwin("GetRestartInterval does not terminate")
                interval += 1
        num_keys = (nr - 1) * interval  # NumberOfKeys
        if it.ok:
            it.seek_to_restart_point(nr - 1)
            while it.next_entry_offset() < ro and it.ok:
                it.parse_next()
                num_keys += 1
    out = []
    if it.ok:
        it.stats = stats
        it.seek_to_restart_point(0)
        it.parse_next()
        while it.valid:
            out.append((it.key, it.v0, it.vlen))
            it.parse_next()
        if it.ok and len(out) > (num_keys & 0xFFFFFFFF):
            raise NoReferenceTwin("more entries than kv_checksum_ was sized for")
    if not it.ok:
        return 2, []
    return 0, out


def block_kv_checksums(block_bytes, kind, prot_bytes):
    """Block::Initialize{Data,Index,MetaIndex}BlockProtectionInfo restated
    (table/block_based/block.cc:1113-1235 over Block::Block :1058-1111 and the
    block iterators' entry decoding): (status -- 0 OK, 1 bad block contents,
    2 bad entry, as include/forst_checksum.h --, key count, kv_checksum_ bytes,
    the full 64-bit protection values).  kind: 0 data, 1 index, 2 metaindex,
    | 4 value_is_full, | 8 index_has_first_key."""
    b = bytes(block_bytes)
    st, ents = block_entries(b, kind)
    if not ents:
        return st, 0, b"", np.zeros(0, np.uint64)
    keys = b"".join(k for k, _, _ in ents)
    kl = np.array([len(k) for k, _, _ in ents], np.uint32)
    ko = np.zeros(len(ents), np.uint64)
    ko[1:] = np.cumsum(kl[:-1].astype(np.uint64))
    vo = np.array([v for _, v, _ in ents], np.uint64) + np.uint64(len(keys))
    vl = np.array([n for _, _, n in ents], np.uint32)
    base = np.frombuffer(keys + b + bytes(8), np.uint8)
    prot = kv_protect_batch(base, ko, kl, vo, vl)  # ProtectKV(key, value)
    enc = prot.view(np.uint8).reshape(-1, 8)[:, :prot_bytes].tobytes()  # Encode(len): LE low bytes
    return st, len(ents), enc, prot


def splitmix64(x):
    return lib().oracle_splitmix64(x)


def fill_stream(start, nbytes, seed):
    out = np.empty(nbytes, dtype=np.uint8)
    lib().oracle_fill_stream(_ptr(out), start, nbytes, seed)
    return out
