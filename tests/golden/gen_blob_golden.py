#!/usr/bin/env python3
"""tests/golden/gen_blob_golden.py -- TEST INFRASTRUCTURE ONLY: blob files
written by the REFERENCE's own code, and what its readers say about them and
about damaged copies of them.

The veneer tests/golden/ref_blob_shim.cc is linked against the reference
archive of tests/golden/refbuild.py (compiled outside the committed tree).
Written through it:
  db_none / db_zlib   a DB with enable_blob_files, min_blob_size = 0, a
                      non-default column family, flushed (no compression / zlib)
  w_edges             BlobLogWriter: key size 0, value size 0, both 0, payloads
                      on both sides of 255/256 and of 1 KiB, a 300-byte key
  w_expiration        records with a non-zero expiration
  w_ttl               a TTL header and footer
  w_empty             a header and a footer and no record
Recorded per file: BlobFileReader::Create's Status string and the records as
BlobLogSequentialReader::ReadRecord(kReadHeaderKeyBlob) returns them (offset,
sizes, expiration, both stored CRCs).  Per damaged copy (a byte offset + XOR
mask, or a truncation): Create's Status string, the sequential reader's count
of sound records and its first failure.  Per request: GetBlob(verify_checksums)'s
Status string for the right key, a wrong key of the right length, a wrong key
size and a wrong value size.

Only data is committed: tests/golden/blob/*.blob and tests/golden/blob_files.json.

Re-run:  python tests/golden/gen_blob_golden.py   (needs the reference + g++)
"""
import ctypes
import glob
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refbuild  # noqa: E402

MSG = 512


def _items(items):
    lens = (ctypes.c_uint64 * max(1, len(items)))(*[len(x) for x in items])
    return b"".join(items), lens


class Ref:
    def __init__(self, so):
        L = self.L = ctypes.CDLL(so)
        cp, sz, u64, u32, i = (ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32,
                               ctypes.c_int)
        vp = ctypes.c_void_p
        L.ref_blob_db_write.argtypes = [cp, i, sz, cp, vp, cp, vp, vp, cp, sz]
        L.ref_blob_write_file.argtypes = [cp, u64, u32, i, i, u64, u64, u64, u64, sz, cp, vp, cp,
                                          vp, vp, cp, sz]
        L.ref_blob_create.argtypes = [cp, u64, u32, cp, sz]
        L.ref_blob_get.argtypes = [cp, u64, u32, cp, sz, u64, u64, cp, sz]
        L.ref_blob_sequential.argtypes = [cp, u64, cp, sz, vp]

    def db_write(self, d, compression, kvs):
        keys, kl = _items([k for k, _ in kvs])
        vals, vl = _items([v for _, v in kvs])
        cf, msg = ctypes.c_uint32(), ctypes.create_string_buffer(MSG)
        rc = self.L.ref_blob_db_write(d.encode(), compression, len(kvs), keys, kl, vals, vl,
                                      ctypes.byref(cf), msg, MSG)
        assert rc == 0, msg.value
        return cf.value

    def write_file(self, d, number, cf, compression, has_ttl, hdr_range, ftr_range, kvs, exps):
        keys, kl = _items([k for k, _ in kvs])
        vals, vl = _items([v for _, v in kvs])
        ex = (ctypes.c_uint64 * max(1, len(kvs)))(*exps)
        msg = ctypes.create_string_buffer(MSG)
        rc = self.L.ref_blob_write_file(d.encode(), number, cf, compression, int(has_ttl),
                                        *hdr_range, *ftr_range, len(kvs), keys, kl, vals, vl, ex,
                                        msg, MSG)
        assert rc == 0, msg.value

    def create(self, d, number, cf):
        msg = ctypes.create_string_buffer(MSG)
        assert self.L.ref_blob_create(d.encode(), number, cf, msg, MSG) == 0
        return msg.value.decode()

    def get(self, d, number, cf, key, value_offset, value_size):
        msg = ctypes.create_string_buffer(MSG)
        assert self.L.ref_blob_get(d.encode(), number, cf, key, len(key), value_offset, value_size,
                                   msg, MSG) == 0
        return msg.value.decode()

    def sequential(self, d, number):
        cap = 1 << 20
        out, n = ctypes.create_string_buffer(cap), ctypes.c_size_t()
        assert self.L.ref_blob_sequential(d.encode(), number, out, cap, ctypes.byref(n)) == 0
        return out.raw[:n.value].decode().splitlines()


def parse_sequential(lines):
    """-> dict(seq_header, records, seq_ok_records, seq_fail, seq_footer)"""
    r = dict(seq_header=lines[0][2:], records=[], seq_ok_records=0, seq_fail=None, seq_footer=None)
    for ln in lines[1:]:
        if ln[0] == "R":
            _, off, ks, vs, ex, hc, bc, st = ln.split(" ", 7)
            if st == "OK":
                r["records"].append(dict(offset=int(off), key_size=int(ks), value_size=int(vs),
                                         expiration=int(ex), header_crc=int(hc), blob_crc=int(bc)))
                r["seq_ok_records"] += 1
            else:
                r["seq_fail"] = st
        elif ln[0] == "F":
            r["seq_footer"] = ln.split(" ", 2)[2]
    return r


def rnd(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def text(rng, n):  # compressible
    words = [b"blob", b"value", b"forst", b"state", b"checkpoint", b"window", b"0123456789"]
    out = b" ".join(words[int(i)] for i in rng.integers(0, len(words), n // 4 + 1))
    return out[:n]


def main():
    rng = np.random.default_rng(0xB10B)
    tmp = tempfile.mkdtemp(prefix="forst_ref_blob_")
    out_dir = os.path.join(HERE, "blob")
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    try:
        ref = Ref(refbuild.link_veneer([os.path.join(HERE, "ref_blob_shim.cc")],
                                       os.path.join(tmp, "libref_blob.so")))
        files = {}  # name -> dict(data, cf, kvs or None)

        # -- through a DB
        for name, comp, make in (("db_none", 0, rnd), ("db_zlib", 2, text)):
            sizes = [0, 1, 17, 100, 230, 250, 600, 1000, 1020, 2048, 4096, 6000]
            kvs = [(b"key%03d" % i + rnd(rng, int(rng.integers(0, 40))), make(rng, s))
                   for i, s in enumerate(sizes)]
            d = os.path.join(tmp, name)
            cf = ref.db_write(d, comp, kvs)
            blobs = sorted(glob.glob(os.path.join(d, "*.blob")))
            assert len(blobs) == 1 and cf != 0, (blobs, cf)
            files[name] = dict(data=open(blobs[0], "rb").read(), cf=cf, source="db",
                               kvs=sorted(kvs) if comp == 0 else None)

        # -- through BlobLogWriter
        wd = os.path.join(tmp, "writer")
        os.makedirs(wd)
        edges = [(b"", b"v" * 7), (b"k" * 5, b""), (b"", b"")]
        for pay in (255, 256, 257, 1023, 1024, 1025, 4096 + 5):
            k = int(rng.integers(1, 60))
            edges.append((rnd(rng, k), rnd(rng, pay - k)))
        edges.append((rnd(rng, 300), rnd(rng, 3000)))
        edges.append((b"a", b"b"))
        ref.write_file(wd, 1, 7, 0, False, (0, 0), (0, 0), edges, [0] * len(edges))
        files["w_edges"] = dict(cf=7, source="writer", kvs=edges, number=1)
        exp_kvs = [(rnd(rng, 9), rnd(rng, 333)), (rnd(rng, 40), rnd(rng, 1500)), (b"e", b"x" * 256)]
        ref.write_file(wd, 2, 9, 0, False, (0, 0), (0, 0), exp_kvs, [1700000000, 2**63 + 5, 1])
        files["w_expiration"] = dict(cf=9, source="writer", kvs=exp_kvs, number=2)
        ttl_kvs = [(b"ttl-key", rnd(rng, 500))]
        ref.write_file(wd, 3, 2, 0, True, (100, 200), (120, 130), ttl_kvs, [125])
        files["w_ttl"] = dict(cf=2, source="writer", kvs=ttl_kvs, number=3)
        ref.write_file(wd, 4, 5, 0, False, (0, 0), (0, 0), [], [])
        files["w_empty"] = dict(cf=5, source="writer", kvs=[], number=4)
        for name, f in files.items():
            if f["source"] == "writer":
                f["data"] = open(os.path.join(wd, "%06d.blob" % f["number"]), "rb").read()

        # -- what the reference's readers say; a scratch directory per question
        qd = os.path.join(tmp, "q")
        os.makedirs(qd)

        def ask(data, cf):
            with open(os.path.join(qd, "000001.blob"), "wb") as fh:
                fh.write(data)
            r = parse_sequential(ref.sequential(qd, 1))
            r["create_status"] = ref.create(qd, 1, cf)
            return r

        meta = {"generator": "tests/golden/gen_blob_golden.py (BlobFileReader, "
                             "BlobLogSequentialReader, BlobLogWriter; db/blob/)",
                "files": {}, "damaged": [], "requests": []}
        for name, f in files.items():
            data = f["data"]
            assert len(data) <= 64 * 1024
            with open(os.path.join(out_dir, name + ".blob"), "wb") as fh:
                fh.write(data)
            r = ask(data, f["cf"])
            assert r["seq_header"] == "OK" and r["seq_fail"] is None and r["seq_footer"] == "OK"
            meta["files"][name + ".blob"] = dict(
                size=len(data), column_family_id=f["cf"], compression=data[13],
                has_ttl=data[12] & 1, source=f["source"], create_status=r["create_status"],
                records=r["records"])

        def damage(name, **d):
            data = files[name]["data"]
            if d["kind"] == "xor":
                b = bytearray(data)
                b[d["offset"]] ^= d["mask"]
                bad = bytes(b)
            else:
                bad = data[:d["size"]]
            r = ask(bad, files[name]["cf"])
            meta["damaged"].append(dict(file=name + ".blob", **d,
                                        create_status=r["create_status"],
                                        seq_header=r["seq_header"],
                                        seq_ok_records=r["seq_ok_records"],
                                        seq_fail=r["seq_fail"], seq_footer=r["seq_footer"]))

        for name in ("db_none", "db_zlib", "w_edges", "w_expiration"):
            recs = meta["files"][name + ".blob"]["records"]
            n = len(files[name]["data"])
            for off, mask in ((0, 0x01), (2, 0x80), (4, 0x02), (8, 0x01), (12, 0x01), (13, 0x04),
                              (14, 0x10), (29, 0x08), (n - 32, 0x01), (n - 28, 0x01),
                              (n - 20, 0x40), (n - 9, 0x02), (n - 4, 0x01), (n - 1, 0x80)):
                damage(name, kind="xor", offset=off, mask=mask)
            for i in sorted({0, 1, len(recs) // 2, len(recs) - 1}):
                o, ks, vs = recs[i]["offset"], recs[i]["key_size"], recs[i]["value_size"]
                spots = [(o, 0x01), (o + 8, 0x02), (o + 9, 0x01), (o + 16, 0x80), (o + 24, 0x01),
                         (o + 27, 0x40), (o + 28, 0x01), (o + 31, 0x10)]
                if ks:
                    spots += [(o + 32, 0x01), (o + 32 + ks - 1, 0x80)]
                if vs:
                    spots += [(o + 32 + ks, 0x04), (o + 32 + ks + vs - 1, 0x20)]
                for off, mask in spots:
                    damage(name, kind="xor", offset=off, mask=mask)
        data = files["db_none"]["data"]
        recs = meta["files"]["db_none.blob"]["records"]
        for size in (0, 29, 61, 62, 63, len(data) - 1, len(data) - 32, len(data) - 33,
                     recs[3]["offset"] + 10 + 32, recs[5]["offset"] + 32):
            damage("db_none", kind="truncate", size=size)

        # -- GetBlob(verify_checksums) requests
        def request(name, i, key, voff, vsize, flip=None):
            f = files[name]
            data = f["data"]
            if flip is not None:
                b = bytearray(data)
                b[flip[0]] ^= flip[1]
                data = bytes(b)
            with open(os.path.join(qd, "000001.blob"), "wb") as fh:
                fh.write(data)
            meta["requests"].append(dict(
                file=name + ".blob", record=i, key=key.hex(), value_offset=voff, value_size=vsize,
                flip=flip, status=ref.get(qd, 1, f["cf"], key, voff, vsize)))

        for name in ("db_none", "w_edges", "w_expiration", "db_zlib"):
            recs = meta["files"][name + ".blob"]["records"]
            data = files[name]["data"]
            for i, r in enumerate(recs):
                o, ks, vs = r["offset"], r["key_size"], r["value_size"]
                key = data[o + 32:o + 32 + ks]
                request(name, i, key, o + 32 + ks, vs)
                if ks:
                    wrong = bytes([key[0] ^ 0x55]) + key[1:]
                    request(name, i, wrong, o + 32 + ks, vs)
                if vs:
                    request(name, i, key, o + 32 + ks, vs - 1)               # a wrong value size
                    request(name, i, key + b"x", o + 32 + ks + 1, vs - 1)     # a wrong key size
                if i in (1, len(recs) - 1):
                    request(name, i, key, o + 32 + ks, vs, flip=(o + 3, 0x01))    # header byte
                    request(name, i, key, o + 32 + ks, vs, flip=(o + 29, 0x01))   # stored blob CRC
                    if vs:
                        request(name, i, key, o + 32 + ks, vs, flip=(o + 32 + ks + vs // 2, 0x08))

        with open(os.path.join(HERE, "blob_files.json"), "w") as fh:
            json.dump(meta, fh, indent=None, separators=(",", ":"))
        total = sum(len(f["data"]) for f in files.values())
        print(f"{len(files)} files, {total} bytes, {len(meta['damaged'])} damaged copies, "
              f"{len(meta['requests'])} requests")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
