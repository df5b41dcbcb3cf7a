"""Blob files without a GPU: the restatement of tests/blobfile.py against every
recorded reference answer of tests/golden/blob_files.json (written by
tests/golden/gen_blob_golden.py through the reference's own BlobFileReader,
BlobLogSequentialReader and BlobLogWriter), and the parts of the C calls that
run before any device call: argument checks, the host walk, and the file
failures the host decides alone."""
import ctypes
import json
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import blobcases as C  # noqa: E402
import blobfile as B  # noqa: E402
from forst_amd import _lib, blob  # noqa: E402
from oracle import oracle as O  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
FORST_EINVAL = -1


@pytest.fixture(scope="module")
def meta():
    return json.load(open(os.path.join(GOLDEN, "blob_files.json")))


def _read(name):
    return open(os.path.join(GOLDEN, "blob", name), "rb").read()


def test_fixture_set_is_small(meta):
    sizes = [os.path.getsize(os.path.join(GOLDEN, "blob", n)) for n in meta["files"]]
    assert max(sizes) <= 64 * 1024
    assert sum(sizes) + os.path.getsize(os.path.join(GOLDEN, "blob_files.json")) < 300 * 1024


def test_restatement_rebuilds_the_reference_written_records(meta):
    """the CRC fields and the bytes of every record the reference wrote"""
    shapes = set()
    for name, m in meta["files"].items():
        data = _read(name)
        assert len(data) == m["size"]
        for r in m["records"]:
            o, ks, vs = r["offset"], r["key_size"], r["value_size"]
            key, val = data[o + 32:o + 32 + ks], data[o + 32 + ks:o + 32 + ks + vs]
            assert data[o:o + 32 + ks + vs] == B.record(key, val, r["expiration"]), (name, o)
            assert struct.unpack_from("<II", data, o + 24) == (r["header_crc"], r["blob_crc"])
            shapes.add((ks == 0, vs == 0, r["expiration"] != 0))
        # the footer, and the file as the walk sees it
        assert data[-32:] == B.file_footer(len(m["records"]),
                                           struct.unpack_from("<QQ", data, len(data) - 20))
        w = B.walk_file(data, m["column_family_id"])
        if m["create_status"] == "OK":
            assert w["offsets"] == [r["offset"] for r in m["records"]]
        s = B.scan_file(data, m["column_family_id"])
        assert s["text"] == m["create_status"], name
        assert (s["cf"], s["compression"], s["has_ttl"]) == (m["column_family_id"],
                                                             m["compression"], m["has_ttl"])
    # key size 0, value size 0, both 0, a non-zero expiration
    assert {(True, False, False), (False, True, False), (True, True, False)} <= shapes
    assert any(e for _, _, e in shapes)
    # payload sizes on both sides of kRawSplit and of the 1 KiB round
    pay = {r["key_size"] + r["value_size"] for m in meta["files"].values() for r in m["records"]}
    assert {255, 256, 257, 1023, 1024, 1025} <= pay


def test_restatement_reproduces_the_damaged_copies(meta):
    texts = set()
    for d in meta["damaged"]:
        data = B.apply_damage(_read(d["file"]), d)
        s = B.scan_file(data, meta["files"][d["file"]]["column_family_id"])
        B.check_against_reference(d, s["text"], s["fail_index"], s["reason"])
        texts.add(s["text"])
    # every file failure that has a reference twin occurs
    assert {B.FILE_TEXT[r] for r in range(1, 10)} <= texts


def test_restatement_reproduces_getblob(meta):
    seen = set()
    for req in meta["requests"]:
        data, off, ks, vs, key = B.request_inputs(req, _read(req["file"]))
        st, _, _ = B.verify_records(np.frombuffer(data, np.uint8), [off], [ks], [vs], [key])
        assert B.RECORD_TEXT[int(st[0])] == req["status"], req
        seen.add(int(st[0]))
    assert seen == {B.OK, B.HEADER_CRC, B.KEY_SIZE, B.VALUE_SIZE, B.KEY, B.CRC}


# ---- the C calls, as far as they go without a device ---------------------------

@pytest.fixture(scope="module")
def L():
    return C.bind(_lib.lib())


def test_blob_calls_reject_bad_arguments_before_any_device_call(L):
    buf = np.zeros(256, np.uint8)
    a = buf[(-buf.ctypes.data) % 16:][:128]
    offs = np.zeros(4, np.uint64)
    st, hc, bc = C.sentinels(4)
    p = lambda x: x.ctypes.data  # noqa: E731

    def verify(base, base_len, o, eks, uk, uko, status, n):
        return L.forst_blob_verify_batch(base, base_len, o, eks, None, uk, 16, uko, status, p(hc),
                                         p(bc), None, n, None)

    # (a machine without a device answers FORST_ENODEV once a call gets that far)
    assert verify(None, 0, None, None, None, None, None, 0) == 0  # n == 0: a no-op
    for args, word in (((p(a), 128, None, None, None, None, p(st), 4), b"record_offsets"),
                       ((p(a), 128, p(offs), None, None, None, None, 4), b"status"),
                       ((None, 128, p(offs), None, None, None, p(st), 4), b"base"),
                       ((p(a) + 1, 127, p(offs), None, None, None, p(st), 4), b"aligned"),
                       ((p(a), 128, p(offs), p(offs), p(a), None, p(st), 4), b"go together"),
                       ((p(a), 128, p(offs), p(offs), None, p(offs), p(st), 4), b"go together"),
                       ((p(a), 128, p(offs), None, p(a), p(offs), p(st), 4), b"expect_key_sizes")):
        assert verify(*args) == FORST_EINVAL, word
        assert word in L.forst_last_error(), (word, L.forst_last_error())
    assert L.forst_blob_record_crc_batch(None, 0, None, None, None, None, 0, None) == 0
    for args, word in (((p(a), 128, None, p(st)), b"record_offsets"),
                       ((p(a), 128, p(offs), None), b"status"),
                       ((None, 128, p(offs), p(st)), b"base"),
                       ((p(a) + 2, 126, p(offs), p(st)), b"aligned")):
        assert L.forst_blob_record_crc_batch(*args, p(hc), p(bc), 4, None) == FORST_EINVAL
        assert word in L.forst_last_error()
    C.check_guards(0, st, hc, bc)  # nothing was written
    assert (a == 0).all()


def _files(L, files, arena_len, dev_offsets, cfs=None, arena=0x1000, out_ok=True):
    n = len(files)
    keep = [np.frombuffer(f, np.uint8) for f in files]
    ptrs = (ctypes.c_void_p * max(1, n))(*[k.ctypes.data if len(k) else None for k in keep])
    sizes = np.array([len(f) for f in files], np.uint64)
    doffs = np.array(dev_offsets, np.uint64)
    cf = None if cfs is None else np.array(cfs, np.uint32)
    out = (C.FileResult * max(1, n))()
    rc = L.forst_blob_verify_files(ctypes.cast(ptrs, ctypes.c_void_p), sizes.ctypes.data,
                                   doffs.ctypes.data, arena, arena_len,
                                   None if cf is None else cf.ctypes.data, n,
                                   ctypes.cast(out, ctypes.c_void_p) if out_ok else None, None)
    return rc, list(out)[:n]


def test_verify_files_argument_checks(L):
    good, _ = B.build_file(C.kvs(3, 1))
    assert L.forst_blob_verify_files(None, None, None, None, 0, None, 0, None, None) == 0
    rc, _ = _files(L, [good], len(good), [0], out_ok=False)
    assert rc == FORST_EINVAL and b"non-null" in L.forst_last_error()
    for arena_len, off in ((len(good) - 1, 0), (len(good) + 7, 8), (100, 2**64 - 8)):
        rc, _ = _files(L, [good], arena_len, [off])
        assert rc == FORST_EINVAL and b"outside the arena" in L.forst_last_error()


def test_verify_files_decides_host_failures_without_a_device(L):
    """malformed size, header magic / version / TTL, a column family mismatch
    and the footer magic need no CRC: the call returns them from the host walk
    (the arena pointer here is never dereferenced: no device call is made)"""
    host = [(n, f, cf) for n, f, cf in C.damaged_files()
            if B.scan_file(f, cf)["reason"] in (B.F_MALFORMED, B.F_HEADER_MAGIC, B.F_HEADER_VERSION,
                                               B.F_CF_MISMATCH, B.F_FOOTER_MAGIC)
            or n in ("header_ttl_flag", "header_exp_range", "ttl_header")]
    assert len(host) >= 8
    files = [f for _, f, _ in host]
    offs = np.concatenate([[0], np.cumsum([(len(f) + 7) & ~3 for f in files])])
    rc, res = _files(L, files, int(offs[-1]), offs[:-1], cfs=[c or 0 for _, _, c in host])
    assert rc == 0, L.forst_last_error()
    reasons = set()
    for (name, f, cf), r in zip(host, res):
        C.same_result(r, B.scan_file(f, cf or 0), L)
        reasons.add(r.reason)
    assert reasons == {B.F_MALFORMED, B.F_HEADER_MAGIC, B.F_HEADER_VERSION, B.F_TTL,
                       B.F_CF_MISMATCH, B.F_FOOTER_MAGIC}


def test_walk_file_matches_the_restatement(meta):
    cases = [(f, cf) for _, f, cf in C.damaged_files()]
    cases += [(_read(n), m["column_family_id"]) for n, m in meta["files"].items()]
    for data, cf in cases:
        res, offs, tail = blob.blob_walk_file(data, cf)
        w = B.walk_file(data, cf)
        assert res.reason == w["reason"] and res.text == B.FILE_TEXT[w["reason"]]
        assert offs.tolist() == w["offsets"] and tail == w["tail_crosses"]
        assert (res.column_family_id, res.compression, res.has_ttl) == \
            (w["cf"], w["compression"], w["has_ttl"])
        assert res.total_blob_bytes == w["total_blob_bytes"]


def test_reason_texts(L):
    for reason, text in B.FILE_TEXT.items():
        assert L.forst_blob_file_reason_text(reason).decode() == text
    assert blob.BlobFileReason.RECORD_TOO_LARGE == B.F_RECORD_TOO_LARGE
    assert O.mask(0) == int(B.mask32(np.zeros(1, np.uint32))[0])  # Value("", 0) = 0: Mask(0)
