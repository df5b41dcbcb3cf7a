#!/usr/bin/env python3
"""tests/golden/gen_kv_golden.py -- TEST INFRASTRUCTURE ONLY: per-KV protection
fixtures (a15) at the reference's own call sites, from the REFERENCE's code.

The veneer tests/golden/ref_kv_shim.cc is linked against the reference archive
of tests/golden/refbuild.py (g++ over src.mk's LIB_SOURCES where they lie, in a
throwaway directory outside the repository; `-z defs` proves nothing is stood
in for) and driven through ctypes:

  memtable   MemTable::Add with memtable_protection_bytes_per_key 1/2/4/8
             (db/memtable.cc:696-732), entries read back through the
             memtable's iterator; MemTable::VerifyEntryChecksum
             (memtable.cc:273-307) on every intact entry, on single-byte
             corruptions of key / tag / value / checksum bytes, and on crafted
             headers (5-byte varint32, internal key shorter than 8, bad value
             length varint) -- its Status text recorded per case.
  writebatch WriteBatch reps of every record kind ReadRecordFromWriteBatch
             parses (write_batch.cc:361-475), default and other column
             families, iterated by the reference's WriteBatch::Iterate with a
             handler doing ProtectionInfoUpdater's ProtectKVO(...).ProtectC(cf)
             (write_batch.cc:3016-3080); truncated reps, wrong counts and
             every tag byte 0-255 in front of a record, with the Status text.
  blocks     data / index / metaindex blocks of the committed reference-written
             SSTs (tests/golden/sst/builder_*.sst), their kv_checksum_ from
             Block::Initialize{Data,Index,MetaIndex}BlockProtectionInfo
             (table/block_based/block.cc:1113-1235, TEST_GetKVChecksum).

Committed: tests/golden/kv_sites.npz (arrays only: numpy.load with
allow_pickle=False) + kv_sites.json (case lists, Status texts).

  --kv-blocks  writes only tests/golden/kv_blocks.{npz,json} (kv_sites.* are
             left alone): crafted blocks from tests/blockgen.py -- block_cases():
             2- and 3-byte varints in every header field, keys and values over
             the hash's length classes, hash-index geometry, blocks of 64 KiB
             and 64 KiB + 1, first keys, damage the reference reads inside the
             block -- answered by Block::Initialize*BlockProtectionInfo for
             protection bytes 1, 2, 4 and 8, and a few WriteBatch reps with
             3-byte lengths and 3..5-byte column family varints.  A case the
             reference could only answer by reading out of bounds, by writing
             past its kv_checksum_, or not at all (its GetRestartInterval loops
             on a bad restart array) is not recorded: oracle.block_kv_checksums
             raises NoReferenceTwin on those, try a new case there first.

Re-run:  python tests/golden/gen_kv_golden.py   (needs /root/reference + g++)
"""
import ctypes
import json
import os
import struct
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, TESTS)
import refbuild  # noqa: E402

OUT_NPZ = os.path.join(HERE, "kv_sites.npz")
OUT_JSON = os.path.join(HERE, "kv_sites.json")
ull, sz, vp, c_int = ctypes.c_ulonglong, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int


def load(path):
    L = ctypes.CDLL(path)
    L.ref_memtable_build.argtypes = [c_int, c_int, ull, vp, sz, vp, ctypes.POINTER(sz)]
    L.ref_memtable_build.restype = c_int
    L.ref_memtable_verify.argtypes = [vp, c_int, c_int, ctypes.c_char_p, sz]
    L.ref_memtable_verify.restype = c_int
    L.ref_write_batch_build.argtypes = [c_int, ull, vp, sz, ctypes.POINTER(sz)]
    L.ref_write_batch_build.restype = c_int
    L.ref_write_batch_protect.argtypes = [vp, sz, vp, sz, ctypes.POINTER(sz), ctypes.c_char_p, sz]
    L.ref_write_batch_protect.restype = c_int
    L.ref_block_kv_checksum.argtypes = [vp, sz, c_int, c_int, c_int, c_int, vp, sz]
    L.ref_block_kv_checksum.restype = ctypes.c_long
    return L


def ptr(a):
    return a.ctypes.data


def mem_verify(L, buf, off, pb):
    """VerifyEntryChecksum on buf[off:] (buf padded: the reference reads up to
    5 bytes past a varint's start regardless)"""
    msg = ctypes.create_string_buffer(4096)
    ok = L.ref_memtable_verify(ptr(buf) + off, pb, 0, msg, 4096)
    return msg.value.decode()


def varint(b, p):
    r = s = 0
    while True:
        x = int(b[p])
        p += 1
        r |= (x & 127) << s
        if not x & 128:
            return r, p
        s += 7


def gen_memtable(L, arrays, meta):
    cases = []
    for pb, n, seed in ((8, 150, 0xA15001), (1, 60, 0xA15002), (2, 60, 0xA15003),
                        (4, 60, 0xA15004)):
        cap = 1 << 23
        raw = np.zeros(cap, np.uint8)
        offs = np.zeros(n, np.uint64)
        nb = sz()
        k = L.ref_memtable_build(pb, n, seed, ptr(raw), cap, ptr(offs), ctypes.byref(nb))
        assert k == n, k
        base = raw[:nb.value + 64].copy()  # + readable padding
        tag = f"mem{pb}"
        status = [mem_verify(L, base, int(o), pb) for o in offs]
        assert all(s == "OK" for s in status), status[:3]
        # corruptions: one byte of key / tag / value / checksum of chosen entries
        corrupt = []
        rng = np.random.default_rng(seed)
        for j in range(0, n, 3):
            o = int(offs[j])
            ikl, kp = varint(base, o)
            vl, vp_ = varint(base, kp + ikl)
            region = [("key", kp, ikl - 8), ("tag", kp + ikl - 8, 8), ("value", vp_, vl),
                      ("checksum", vp_ + vl, pb)][j % 4]
            if region[2] == 0:
                region = ("tag", kp + ikl - 8, 8)
            at = region[1] + int(rng.integers(0, region[2]))
            bit = 1 << int(rng.integers(0, 8))
            b2 = base.copy()
            b2[at] ^= bit
            corrupt.append({"entry": j, "region": region[0], "at": at, "xor": bit,
                            "status": mem_verify(L, b2, o, pb)})
        arrays[tag + "_base"] = base
        arrays[tag + "_offs"] = offs
        cases.append({"tag": tag, "prot_bytes": pb, "n": n, "corrupt": corrupt})
    # crafted headers (pb 8): each a small buffer of its own
    crafted = []
    pads = bytes(32)
    for name, head in (("klen_5_continuation", b"\x80\x80\x80\x80\x80\x01"),
                       ("klen_below_8", b"\x07" + b"k" * 7 + b"\x00" * 8),
                       ("klen_0", b"\x00\x00" + b"v" * 9),
                       ("vlen_5_continuation", b"\x0b" + b"abc" + struct.pack("<Q", (9 << 8) | 1)
                        + b"\xff\xff\xff\xff\xff\x00"),
                       ("vlen_multibyte_ok", b"\x0b" + b"abc" + struct.pack("<Q", (9 << 8) | 1)
                        + b"\x81\x01" + b"w" * 129 + b"\x00" * 8),
                       ("klen_5_bytes_ok", b"\x8b\x80\x80\x80\x00" + b"abc" +
                        struct.pack("<Q", (5 << 8) | 2) + b"\x02xy" + b"\x00" * 8)):
        buf = np.frombuffer(head + pads, np.uint8).copy()
        crafted.append({"name": name, "hex": (head + pads).hex(), "len": len(head),
                        "status": mem_verify(L, buf, 0, 8)})
    meta["memtable"] = {"cases": cases, "crafted": crafted}


def wb_protect(L, rep):
    buf = np.frombuffer(rep + bytes(16), np.uint8).copy()
    out = np.zeros(4096, np.uint64)
    n = sz()
    msg = ctypes.create_string_buffer(4096)
    ok = L.ref_write_batch_protect(ptr(buf), len(rep), ptr(out), 4096, ctypes.byref(n), msg, 4096)
    return msg.value.decode(), out[:n.value].copy()


def gen_writebatch(L, arrays, meta):
    reps, batches = [], []

    def add(name, rep):
        st, prot = wb_protect(L, rep)
        batches.append({"name": name, "status": st, "n_prot": len(prot), "len": len(rep)})
        reps.append(rep)
        arrays[f"wb_prot_{len(batches) - 1}"] = prot

    cap = 1 << 22
    raw = np.zeros(cap, np.uint8)
    n = sz()
    for i, nrec in enumerate((0, 1, 2, 5, 9, 17, 40, 40, 120)):
        cnt = L.ref_write_batch_build(nrec, 0xB0001 + i, ptr(raw), cap, ctypes.byref(n))
        assert cnt >= 0
        rep = raw[:n.value].tobytes()
        add(f"random_{nrec}_{i}", rep)
        if nrec >= 2:
            add(f"truncated_{i}", rep[:len(rep) - 3])
            add(f"wrong_count_{i}", rep[:8] + struct.pack("<I", cnt + 1) + rep[12:])
            add(f"short_header_{i}", rep[:11])
    # every tag byte in front of one well-formed-looking record
    body = b"\x03abc\x04wxyz"
    for t in range(256):
        add(f"tag_{t:02x}", struct.pack("<QI", 77, 1) + bytes([t]) + b"\x05" + body)
    meta["writebatch"] = batches
    blob = b"".join(reps)
    offs = np.cumsum([0] + [len(r) for r in reps[:-1]]).astype(np.uint64)
    arrays["wb_base"] = np.frombuffer(blob + bytes(64), np.uint8).copy()
    arrays["wb_offs"] = offs
    arrays["wb_lens"] = np.array([len(r) for r in reps], np.uint32)


def gen_blocks(L, arrays, meta):
    """the blocks of the committed reference-written SSTs, uncompressed (the
    contents the reader builds Block from), with the kind / value flags the
    table reader gives them, plus crafted damaged blocks; Block::Initialize*
    ProtectionInfo's kv_checksum_ for protection bytes 8 and 2"""
    import sstwalk

    man = json.load(open(os.path.join(HERE, "sst", "builder_manifest.json")))
    blobs, cases = [], []
    for f in man["files"]:
        data = open(os.path.join(HERE, "sst", f["file"]), "rb").read()
        blocks, foot = sstwalk.walk(data)
        fv, ix = f["format_version"], f["index_type"]
        taken = {}
        for kind, o, n, _t in blocks:
            if kind in ("filter", "filter_partition", "dict"):
                continue  # not in block format
            if taken.get(kind, 0) >= 6:
                continue
            taken[kind] = taken.get(kind, 0) + 1
            try:
                blk = sstwalk.contents(data, (o, n), fv)
            except Exception:  # zlib with a compression dictionary: not decodable here
                continue
            if kind in ("data", "rangedel"):
                k = 0
            elif kind == "properties":
                continue  # never protected: MetaBlockIter assumes restart interval 1 (block.h:826-829)
            elif kind == "metaindex":
                k = 2
            else:  # index, index_partition, filter_index (index-block format)
                full = fv < 4
                first = ix == 3 and kind != "filter_index"
                k = 1 | (4 if full else 0) | (8 if first else 0)
            cases.append({"src": f["file"], "kind_name": kind, "kind": k, "bytes": blk})
    # damaged blocks: too small, restart count that wraps the offset, a first
    # entry sharing bytes with no previous key, an entry running past the block,
    # and a data block whose last value runs into the restart array
    good = next(c for c in cases if c["kind"] == 0)["bytes"]
    nr = struct.unpack_from("<I", good, len(good) - 4)[0]
    cases.append({"src": "crafted", "kind_name": "tiny", "kind": 0, "bytes": b"\x00" * 5})
    cases.append({"src": "crafted", "kind_name": "restarts_wrap", "kind": 0,
                  "bytes": good[:-4] + struct.pack("<I", 0x00ffffff)})
    cases.append({"src": "crafted", "kind_name": "first_shared", "kind": 0,
                  "bytes": b"\x05" + good[1:]})
    cases.append({"src": "crafted", "kind_name": "meta_slice_past_limit", "kind": 2,
                  "bytes": b"\x00\x04\x7f" + b"abcd" + b"\x00" * 4 + struct.pack("<II", 0, 1)})
    cases.append({"src": "crafted", "kind_name": "data_value_into_restarts", "kind": 0,
                  "bytes": b"\x00\x04\x05" + b"abcd" + b"xy" + struct.pack("<II", 0, 1)})
    cases.append({"src": "crafted", "kind_name": "empty_restarts", "kind": 0,
                  "bytes": struct.pack("<II", 0, 0)})
    for c in cases:
        blk = c.pop("bytes")
        buf = np.frombuffer(blk + bytes(64), np.uint8).copy()
        c["size"] = len(blk)
        if os.environ.get("GEN_DEBUG"):
            print(c["src"], c["kind_name"], c["kind"], len(blk), flush=True)
        for pb in (8, 2):
            out = np.zeros(1 << 20, np.uint8)
            nk = L.ref_block_kv_checksum(ptr(buf), len(blk), c["kind"] & 3, pb,
                                         1 if c["kind"] & 4 else 0, 1 if c["kind"] & 8 else 0,
                                         ptr(out), out.nbytes)
            c[f"keys_{pb}"] = int(nk)
            c[f"kv_checksum_{pb}"] = out[:max(0, nk) * pb].tobytes().hex()
        blobs.append(blk)
    offs, pos, parts = [], 0, []
    for b in blobs:
        pos += (-pos) % 4 + 3  # unaligned block starts
        parts.append(pos)
        pos += len(b)
    base = np.zeros(pos + 64, np.uint8)
    for o, b in zip(parts, blobs):
        base[o:o + len(b)] = np.frombuffer(b, np.uint8)
    arrays["blk_base"] = base
    arrays["blk_offs"] = np.array(parts, np.uint64)
    meta["blocks"] = cases


def block_cases():
    """[(name, kind, block bytes)] of kv_blocks: the entry shapes, geometries
    and in-bounds damage the SST-cut blocks of kv_sites never reach"""
    import blockgen as G
    P = G.pattern
    D, I, M, F, K = G.DATA, G.INDEX, G.META, G.FULL, G.FIRST
    out = []

    # shared / non_shared / value_length at the varint32 width edges, alone and together
    for x in (127, 128, 16383, 16384):
        k0 = P(x, 1)
        for name, kind in (("data", D), ("index_full", I | F), ("meta", M)):
            long = k0[:5] + b"yy" + P(x - 7, 3)
            ents = [(k0, b"v0"),                   # non_shared = x
                    (k0 + b"z", b"v1"),            # shared = x
                    (k0[:5] + b"yy", P(x, 2)),     # value_length = x
                    (long, b""),
                    (long + P(x, 4), P(x, 5)),     # all three = x
                    (long + b"\xfe\xff", b"")]
            out.append((f"varint_{name}_{x}", kind, G.build(ents, kind=kind, share_over_restarts=True)))
        for name, kind in (("index_v4", I), ("index_v4_first", I | K)):
            fk = (lambda j: P(j, 7)) if kind & K else (lambda j: None)
            ents = [(k0, ((1000, 50), fk(9))), (k0 + b"z", ((1055, 60), fk(0))),
                    (k0 + P(x, 8), ((1120, 40), fk(130))),  # shared = non_shared = x
                    (k0 + b"zz", ((1165, 300000), fk(3)))]
            out.append((f"varint_{name}_{x}", kind, G.build(ents, kind=kind)))

    # key lengths over the hash's length classes, rebuilt from shared prefixes of
    # every length mod 4
    for n in (16, 17, 128, 129, 240, 241, 1024, 1025, 3001):
        key = P(n, n)
        ents = [(key, b"first")]
        for r in range(4):
            for p in (max(p for p in range(n) if p % 4 == r), 4 + r):
                key = key[:p] + P(n - p, n + 10 * r + p)
                if G.common_prefix(ents[-1][0], key) != p:  # the new tail must differ at once
                    key = key[:p] + bytes([key[p] ^ 0x55]) + key[p + 1:]
                ents.append((key, P(r + 1, p)))
        out.append((f"keys_{n}", D, G.build(ents, kind=D, interval=16)))
    ents = [(P(n, 40 + n), ((n * 77, n + 1), None)) for n in (16, 17, 128, 129, 240, 241, 1025)]
    ents = [(ents[0][0][:11] + k, v) for k, v in ents]
    out.append(("keys_index_v4", I, G.build(ents, kind=I, interval=4)))

    # value lengths over the hash's length classes; restart intervals 1 and 16
    vals = (0, 1, 3, 4, 8, 9, 16, 17, 128, 129, 240, 241, 5003)
    for interval in (1, 16):
        ents = [(b"user-key-%04d" % v + b"\x01" * 8, P(v, v)) for v in vals]
        out.append((f"values_interval_{interval}", D, G.build(ents, kind=D, interval=interval)))
        out.append((f"values_index_full_interval_{interval}", I | F,
                    G.build(ents, kind=I | F, interval=interval)))
    out.append(("values_meta", M, G.build(ents, kind=M)))

    # data-block hash index: 1 bucket, many, a block of exactly 64 KiB; 64 KiB + 1
    small = [(b"hk%03d" % j + P(j % 9, j), P(j % 40, j + 1)) for j in range(40)]
    out.append(("hash_1_bucket", D, G.build(small[:3], kind=D, interval=16, hash_buckets=1)))
    out.append(("hash_many_buckets", D, G.build(small, kind=D, interval=16,
                                                hash_buckets=bytes(range(53)) * 5)))
    out.append(("hash_exactly_65536", D, G.sized(65536, small, b"zfill", kind=D, interval=16,
                                                 hash_buckets=bytes(range(37)))))
    out.append(("plain_65537", D, G.sized(65537, small, b"zfill", kind=D, interval=16)))
    # over 64 KiB the footer is the restart count as it stands: bit 31 is part
    # of the count, the 6 bytes before it are entry and restart bytes, not a
    # hash index, and the metaindex walk meets 2 stray bytes -> the error marker
    blk = G.sized(65537, [], b"only", kind=M, hash_buckets=0)
    assert struct.unpack_from("<I", blk, len(blk) - 4)[0] == 0x80000001
    out.append(("bit31_65537", M, blk))

    # format_version >= 4 index blocks with first keys: shared == 0 and > 0,
    # handles of 1..5 varint64 bytes, first keys of 0 and 200 bytes
    ents, off = [], 0
    for j, size in enumerate((1, 100, 127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21,
                              (1 << 28) - 1, 1 << 28, (1 << 35) - 1, 77, 5, 1 << 30, 9, 3)):
        ents.append((b"index-key-" + P(4 + j % 3, j), ((off, size), P(200 if j % 3 == 1 else 0 if j % 3 else 24, j))))
        off += size + 5
    for interval in (1, 4, 16):
        out.append((f"index_v4_first_interval_{interval}", I | K, G.build(ents, kind=I | K, interval=interval)))
    out.append(("index_v4_interval_4", I, G.build([(k, (h, None)) for k, (h, _f) in ents], kind=I, interval=4)))

    # damage the reference still reads inside the block: checked decoders
    # (metaindex, format_version >= 4 index) and the unchecked one (data)
    def craft(entries_bytes, restarts=(0,), **kw):
        return bytes(entries_bytes) + G.tail(list(restarts), **kw)

    e_data = b"\x00\x04\x02" + b"abcd" + b"xy"          # abcd -> xy
    e_v4 = b"\x00\x04" + b"abcd" + b"\x10\x20"          # abcd -> handle (16, 32)
    e_v4f = e_v4 + b"\x03fk0"
    for name, kind, good in (("data", D, e_data), ("meta", M, e_data), ("index_full", I | F, e_data),
                             ("index_v4", I, e_v4), ("index_v4_first", I | K, e_v4f)):
        # (metaindex: every entry a restart point)
        r2 = (0, len(good)) if kind == M else (0,)
        out.append((f"bad_varint_cut_at_restarts_{name}", kind, craft(good + b"\x85\x80\x80", r2)))
        out.append((f"bad_varint_5_continuation_{name}", kind,
                    craft(good + b"\x80\x80\x80\x80\x80\x01\x01\x01kv", r2)))
        out.append((f"bad_shared_over_previous_{name}", kind,
                    craft(good + b"\x05\x01" + (b"" if good is not e_data else b"\x01") + b"k" +
                          (b"v" if good is e_data else b"\x01" + (b"\x00" if kind & K else b"")), r2)))
        out.append((f"ok_shared_equals_previous_{name}", kind,
                    craft(good + b"\x04\x01" + (b"" if good is not e_data else b"\x01") + b"k" +
                          (b"v" if good is e_data else b"\x01" + (b"\x00" if kind & K else b"")), r2)))
    # non_shared + value_length past the restart offset: the checked decoder
    # fails, the unchecked one takes restart / hash-index bytes as value bytes
    for name, kind in (("meta", M), ("data", D), ("index_full", I | F)):
        r2 = (0, len(e_data)) if kind == M else (0,)
        out.append((f"past_limit_1_byte_{name}", kind, craft(e_data + b"\x00\x01\x06" + b"k" + b"v", r2)))
        out.append((f"past_limit_2_byte_{name}", kind,
                    craft(e_data + b"\x00\x01\x96\x01" + b"k" + b"v" * 20, r2,
                          hash_buckets=None if kind == M else 200)))
    out.append(("past_limit_2_byte_data_plain", D, craft(e_data + b"\x00\x81\x00\x05" + b"k" + b"v", (0,))))
    # an index value that does not decode inside the entries: IndexValue::DecodeFrom
    # fails (only asserted), the value is what it consumed and the walk goes on there
    out.append(("bad_v4_handle_size_cut", I, craft(e_v4 + b"\x00\x01k" + b"\x07\x80\x80\x80")))
    out.append(("bad_v4_delta_cut", I, craft(e_v4 + b"\x01\x01k" + b"\x80\x80\x80")))
    out.append(("bad_v4_handle_10_continuation", I, craft(e_v4 + b"\x00\x01k" + b"\x80" * 10 + b"\x01\x01" + e_v4)))
    out.append(("bad_v4_first_key_varint_cut", I | K, craft(e_v4f + b"\x00\x01k\x07\x08" + b"\x80\x80\x80")))
    out.append(("bad_v4_first_key_length_past_restarts", I | K,
                craft(e_v4f + b"\x00\x01k\x07\x08" + b"\x32" + b"\x7f\x01k\x01\x01\x00")))
    out.append(("v4_first_key_length_past_restarts_walk_goes_on", I | K,
                craft(e_v4f + b"\x00\x01k\x07\x08" + b"\x32" + b"\x00\x01m\x05\x06\x00")))
    # a hash index whose bucket count exceeds the block: the 16-bit map offset
    # wraps to 5 bytes before the block's end, the restart array ends there and
    # its third entry takes in the count's low byte (so it points far outside
    # and that interval is empty): 2 intervals of 2 entries
    four = (b"\x00\x02\x01aa1" + b"\x01\x01\x01b2", b"\x00\x02\x01cc3" + b"\x01\x01\x01d4")
    blk = four[0] + four[1] + struct.pack("<II", 0, len(four[0])) + b"\x00\x00\x00" + b"\xff\xff" + \
        struct.pack("<I", (1 << 31) | 3)
    out.append(("hash_bucket_count_wraps_map_offset", D, blk))
    # a hash-index footer with no restarts: entry bytes, but no protection
    for name, kind in (("data", D), ("meta", M)):
        out.append((f"hash_no_restarts_{name}", kind, e_data + G.tail([], hash_buckets=3)))
    # an index value cut off exactly at the restart offset, nothing behind it:
    # the value is what DecodeFrom consumed and the walk ends there, 2 keys
    for name, kind, good in (("", I, e_v4), ("_first", I | K, e_v4f)):
        out.append((f"v4{name}_handle_offset_cut_nothing_after", kind, craft(good + b"\x00\x01k")))
        out.append((f"v4{name}_handle_size_cut_nothing_after", kind, craft(good + b"\x00\x01k\x07")))
        out.append((f"v4{name}_delta_cut_nothing_after", kind, craft(good + b"\x01\x01k")))
    out.append(("v4_first_key_varint_cut_nothing_after", I | K, craft(e_v4f + b"\x00\x01k\x07\x08")))
    out.append(("v4_first_delta_first_key_varint_cut_nothing_after", I | K, craft(e_v4f + b"\x01\x01k\x03")))
    return out


def wb_extra_reps():
    """[(name, rep)]: WriteBatch reps with 3-byte lengths and 3..5-byte column
    family varints, which neither the reference's random batches of kv_sites nor
    the tests' own generator produce"""
    import blockgen as G
    head = struct.pack("<QI", 99, 1)
    out = [("value_20000", head + b"\x01" + b"\x03key" + G.varint(20000) + G.pattern(20000, 11))]
    for cf in (1 << 14, 1 << 21, 1 << 28, (1 << 32) - 1):
        out.append((f"cf_{cf}", head + b"\x05" + G.varint(cf) + b"\x03key" + b"\x05value"))
    out.append(("cf_5_continuation", head + b"\x05" + b"\x80\x80\x80\x80\x80\x01" + b"\x03key\x05value"))
    out.append(("two_records_big_cf", struct.pack("<QI", 7, 2) + b"\x04" + G.varint(1 << 21) + b"\x03key" +
                b"\x06" + G.varint((1 << 32) - 1) + b"\x02ab" + G.varint(16384) + G.pattern(16384, 3)))
    return out


def gen_kv_blocks(L):
    """tests/golden/kv_blocks.{json,npz}: block_cases() and wb_extra_reps(), each
    answered by the reference (protection bytes 1, 2, 4 and 8 for the blocks)"""
    arrays, meta = {}, {"generator": "tests/golden/gen_kv_golden.py --kv-blocks"}
    cases, blobs = [], []
    for name, kind, blk in block_cases():
        buf = np.frombuffer(blk + bytes(64), np.uint8).copy()
        c = {"name": name, "kind": kind, "size": len(blk)}
        for pb in (1, 2, 4, 8):
            out = np.zeros(1 << 16, np.uint8)
            nk = L.ref_block_kv_checksum(ptr(buf), len(blk), kind & 3, pb, 1 if kind & 4 else 0,
                                         1 if kind & 8 else 0, ptr(out), out.nbytes)
            c[f"keys_{pb}"] = int(nk)
            c[f"kv_checksum_{pb}"] = out[:max(0, nk) * pb].tobytes().hex()
        if os.environ.get("GEN_DEBUG"):
            print(name, kind, len(blk), c["keys_8"], flush=True)
        cases.append(c)
        blobs.append(blk)
    pos, parts = 0, []
    for j, b in enumerate(blobs):
        pos += (j % 16 - pos) % 16  # block starts at every offset mod 16
        parts.append(pos)
        pos += len(b)
    base = np.zeros(pos + 64, np.uint8)
    for o, b in zip(parts, blobs):
        base[o:o + len(b)] = np.frombuffer(b, np.uint8)
    arrays["blk_base"] = base
    arrays["blk_offs"] = np.array(parts, np.uint64)
    meta["blocks"] = cases
    reps, batches = [], []
    for name, rep in wb_extra_reps():
        st, prot = wb_protect(L, rep)
        batches.append({"name": name, "status": st, "n_prot": len(prot), "len": len(rep)})
        arrays[f"wb_prot_{len(reps)}"] = prot
        reps.append(rep)
    meta["writebatch"] = batches
    arrays["wb_base"] = np.frombuffer(b"".join(reps) + bytes(64), np.uint8).copy()
    arrays["wb_offs"] = np.cumsum([0] + [len(r) for r in reps[:-1]]).astype(np.uint64)
    arrays["wb_lens"] = np.array([len(r) for r in reps], np.uint32)
    npz, js = os.path.join(HERE, "kv_blocks.npz"), os.path.join(HERE, "kv_blocks.json")
    np.savez_compressed(npz, **arrays)
    with open(js, "w") as f:
        json.dump(meta, f, indent=1)
    print(npz, os.path.getsize(npz), js)


def main():
    with tempfile.TemporaryDirectory() as td:
        so = refbuild.link_veneer([os.path.join(HERE, "ref_kv_shim.cc")],
                                  os.path.join(td, "libref_kv.so"))
        L = load(so)
        if "--kv-blocks" in sys.argv[1:]:  # the new files only: kv_sites.* stay as they are
            gen_kv_blocks(L)
            return
        arrays, meta = {}, {"generator": "tests/golden/gen_kv_golden.py"}
        gen_memtable(L, arrays, meta)
        gen_writebatch(L, arrays, meta)
        gen_blocks(L, arrays, meta)
        np.savez_compressed(OUT_NPZ, **arrays)
        with open(OUT_JSON, "w") as f:
            json.dump(meta, f, indent=1)
    print(OUT_NPZ, os.path.getsize(OUT_NPZ), OUT_JSON)


if __name__ == "__main__":
    main()
