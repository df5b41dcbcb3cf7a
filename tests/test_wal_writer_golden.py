"""The WAL writer pinned to the REFERENCE's own log::Writer::AddRecord
(tests/golden/wal_writer.json.gz, made by tests/golden/gen_wal_writer_golden.py
from the reference's db/log_writer.cc): oracle.wal_frame -- the expected image
of every forst_wal_frame_batch test -- rebuilds each recorded log byte for byte
(size, every header, SHA-256 of the whole log), and forst_wal_layout gives the
recorded header offsets, length fields and type bytes.  CPU only."""
import ctypes
import gzip
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import stream  # noqa: E402
from forst_amd import _lib  # noqa: E402
from oracle import oracle as O  # noqa: E402

with gzip.open(os.path.join(HERE, "golden", "wal_writer.json.gz"), "rt") as f:
    CASES = json.load(f)["cases"]


def _id(c):
    return "%s-%s" % (c["name"], "recyclable" if c["recyclable"] else "legacy")


def test_fixture_has_the_cases():
    names = {c["name"] for c in CASES}
    assert names == {"lengths_0_40", "block_edges_hs7", "block_edges_hs11", "four_fragments",
                     "log_uniform_300"}
    assert all(sum(1 for c in CASES if c["name"] == n) == 2 for n in names)
    by = {_id(c): c for c in CASES}
    assert by["lengths_0_40-legacy"]["lengths"] == list(range(41))
    four = by["four_fragments-recyclable"]  # 100 B, a record of four fragments, 7 B
    assert len(four["headers"]) == 1 + 4 + 1
    assert len(by["log_uniform_300-legacy"]["lengths"]) == 300


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_oracle_frame_is_the_reference_writer(case):
    lens = np.array(case["lengths"], np.uint32)
    pay = stream.stream(case["seed"], 0, int(lens.astype(np.int64).sum()))
    img, po, pl = O.wal_frame(pay, lens, recyclable=case["recyclable"],
                              log_number=case["log_number"] & 0xFFFFFFFF)
    hs = 11 if case["recyclable"] else 7
    assert len(img) == case["size"]
    assert len(po) == len(case["headers"])
    for (o, h), got_o in zip(case["headers"], po):
        assert o == int(got_o) and bytes(img[o:o + hs]).hex() == h, (o, int(got_o))
    assert hashlib.sha256(img.tobytes()).hexdigest() == case["sha256"]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_layout_is_the_reference_writer(case):
    L = _lib.lib()
    lens = np.array(case["lengths"], np.uint32)
    k = len(case["headers"])
    po, pl, pt = np.zeros(k + 1, np.uint64), np.zeros(k + 1, np.uint32), np.zeros(k + 1, np.uint8)
    nph, npad, tot = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    rc = L.forst_wal_layout(lens.ctypes.data, len(lens), int(case["recyclable"]), po.ctypes.data,
                            pl.ctypes.data, pt.ctypes.data, k + 1, None, None, 1 << 40,
                            ctypes.byref(nph), ctypes.byref(npad), ctypes.byref(tot))
    assert rc == 0 and nph.value == k and tot.value == case["size"]
    hdr = [(o, bytes.fromhex(h)) for o, h in case["headers"]]
    assert po[:k].tolist() == [o for o, _ in hdr]
    assert pl[:k].tolist() == [h[4] | h[5] << 8 for _, h in hdr]
    assert pt[:k].tolist() == [h[6] for _, h in hdr]
    # the zero-filled block tails: the gaps the headers and payloads leave
    hs = 11 if case["recyclable"] else 7
    ends = [o + hs + (h[4] | h[5] << 8) for o, h in hdr]
    gaps = sum(1 for e, (o, _) in zip(ends, hdr[1:]) if o > e)
    assert npad.value == gaps
    if case["name"] == "block_edges_hs%d" % hs:  # (each set also runs with the other header size)
        assert gaps >= 6 * (hs - 1)
