#!/usr/bin/env python3
"""tests/golden/gen_wal_writer_golden.py -- TEST INFRASTRUCTURE ONLY: WAL writer
fixtures from the REFERENCE's own log::Writer.

The reference's db/log_writer.cc and its link closure are compiled from the
sources under /root/reference (tests/golden/refbuild.py) and linked with the
veneer tests/golden/ref_wal_writer_shim.cc, which appends to an in-memory file
through log::Writer::AddRecord (db/log_writer.cc:65-160), legacy and
recyclable.  The payloads are the splitmix64 stream of tests/golden/stream.py
cut back to back, so a test rebuilds them from the seed.

Committed: tests/golden/wal_writer.json.gz -- per case the lengths, the stream
seed, recyclable and log_number, the log's size, every header as (offset,
header bytes in hex) and the SHA-256 of the whole log.  No payload byte is
stored.  The headers are cut from the reference's log where the writer's
layout puts them (headers() below restates db/log_writer.cc:86-151); the
SHA-256 proves them: headers + the stream's payload + zero pads rebuild the log.

Re-run:  python tests/golden/gen_wal_writer_golden.py   (needs /root/reference + g++)
"""
import ctypes
import gzip
import hashlib
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refbuild  # noqa: E402
import stream  # noqa: E402

OUT = os.path.join(HERE, "wal_writer.json.gz")
BLOCK = 32768


def cases():
    """(name, lengths, seed)"""
    yield "lengths_0_40", list(range(41)), 0x5701
    for hs in (7, 11):
        c = BLOCK - hs
        # a pad record, then a record that starts with `left` bytes left in its
        # block, left = 0 .. hs + 17, of every length around one, two and three
        # blocks (tests/walframe_cases.py block_edge_group)
        lens, bo = [], 0

        def add(n):
            nonlocal bo
            lens.append(n)
            if BLOCK - bo < hs:
                bo = 0
            pay0 = BLOCK - bo - hs
            if n <= pay0:
                bo += hs + n
            else:
                rest = n - pay0
                bo = hs + rest - (-(-rest // c) - 1) * c

        for left in range(hs + 18):
            for n in (c - 1, c, c + 1, 2 * c, 2 * c + 1, 3 * c + 5):
                pad = (BLOCK - left) - bo - hs
                if BLOCK - bo < hs or pad < 0:
                    if BLOCK - bo >= hs:
                        add(BLOCK - bo - hs)
                    pad = (BLOCK - left) - hs
                add(pad)
                add(n)
        add(BLOCK - bo - hs if BLOCK - bo >= hs else c)  # ends at a block end ...
        add(0)                                            # ... then an empty record
        yield f"block_edges_hs{hs}", lens, 0x5702 + hs
    yield "four_fragments", [100, 3 * BLOCK + 500, 7], 0x5703
    rng = np.random.default_rng(0x5704)
    yield "log_uniform_300", [int(x) for x in np.exp(rng.uniform(0, np.log(70000), 300))], 0x5704


def headers(log, lengths, hs):
    """[(offset, header bytes)] by the writer's layout (log_writer.cc:86-151)"""
    out, off = [], 0
    for n in lengths:
        left, first = n, True
        while first or left > 0:
            bo = off % BLOCK
            if BLOCK - bo < hs:
                off += BLOCK - bo
                bo = 0
            frag = min(left, BLOCK - bo - hs)
            out.append((off, bytes(log[off:off + hs])))
            off += hs + frag
            left -= frag
            first = False
    assert off == len(log), (off, len(log))
    return out


def main():
    tmp = tempfile.mkdtemp(prefix="forst_ref_walw_")
    try:
        so = refbuild.link_veneer([os.path.join(HERE, "ref_wal_writer_shim.cc")],
                                  os.path.join(tmp, "libref_walw.so"))
        L = ctypes.CDLL(so)
        L.ref_wal_write.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                    ctypes.c_ulonglong, ctypes.c_char_p, ctypes.c_size_t,
                                    ctypes.POINTER(ctypes.c_size_t)]
        L.ref_wal_write.restype = ctypes.c_int
        out = []
        for name, lengths, seed in cases():
            for rec, ln in ((False, 0), (True, 0x01020304)):
                lens = np.array(lengths, np.uint32)
                pay = stream.stream(seed, 0, int(lens.astype(np.int64).sum())).tobytes()
                cap = len(pay) + 64 * len(lens) + (len(pay) // 1024 + 64) * 32
                buf = ctypes.create_string_buffer(cap)
                n = ctypes.c_size_t()
                rc = L.ref_wal_write(pay, lens.ctypes.data, len(lens), int(rec), ln, buf, cap,
                                     ctypes.byref(n))
                assert rc == 0 and n.value <= cap, (name, rc, n.value, cap)
                log = buf.raw[:n.value]
                hdr = headers(log, lengths, 11 if rec else 7)
                out.append({"name": name, "recyclable": rec, "log_number": ln, "seed": seed,
                            "lengths": lengths, "size": len(log),
                            "headers": [[o, h.hex()] for o, h in hdr],
                            "sha256": hashlib.sha256(log).hexdigest()})
                print(name, rec, len(lengths), len(log), len(hdr))
        doc = {"generator": "tests/golden/gen_wal_writer_golden.py",
               "reference": "db/log_writer.cc log::Writer::AddRecord (compiled from "
                            "/root/reference by tests/golden/refbuild.py)",
               "cases": out}
        with gzip.open(OUT, "wt", compresslevel=9) as f:
            json.dump(doc, f, separators=(",", ":"))
        print(f"{len(out)} cases -> {OUT} ({os.path.getsize(OUT)} bytes)")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
