"""Blob file records (forst_blob_verify_batch, forst_blob_record_crc_batch,
forst_blob_verify_files) on the CPU SIMT emulator against the restatement of
tests/blobfile.py: the decode, key, status and store kernels of
forst_amd/csrc/blob.h and the raw CRC launch under them, at the sizes where the
code takes another path.  The device twin is tests/test_gpu_blob.py; the cases
live in tests/blobcases.py."""
import ctypes
import json
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)

if shutil.which("/opt/rocm/llvm/bin/clang++") is None:
    pytest.skip("needs ROCm clang++ to build the emulator", allow_module_level=True)

import emu  # noqa: E402
import blobcases as C  # noqa: E402
import blobfile as B  # noqa: E402
import dispatch as D  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def run():
    # (the three symbols are bound here, in blobcases.bind: emu.py has no wrapper)
    return C.HostRunner(emu.lib())


def test_emu_blob_no_record_touches_nothing(run):
    st, hc, bc = C.sentinels(0)
    rc = run.L.forst_blob_verify_batch(None, 0, None, None, None, None, 0, None, st.ctypes.data,
                                       hc.ctypes.data, bc.ctypes.data, None, 0, None)
    assert rc == 0
    rc = run.L.forst_blob_record_crc_batch(None, 0, None, st.ctypes.data, hc.ctypes.data,
                                           bc.ctypes.data, 0, None)
    assert rc == 0
    C.check_guards(0, st, hc, bc)
    assert run.L.forst_blob_verify_files(None, None, None, None, 0, None, 0, None, None) == 0


def test_emu_blob_record_cases(run):
    seen = C.run_record_cases(run)
    assert seen == set(range(8))  # every status code at least once


def test_emu_blob_writer_cases(run):
    C.run_writer_cases(run)


def test_emu_blob_nullable_outputs(run):
    buf, offs, ks, vs, keys = C.count_batch(65)
    st, hc, bc, mism = run.verify(buf, offs, ks, vs, keys, outputs=False)
    assert (st == 0).all()
    assert (hc == D.SENTINEL32).all() and (bc == D.SENTINEL32).all() and mism == 0


def test_emu_blob_user_key_outside_the_key_buffer(run):
    # a user key range past user_keys_len is a key mismatch, never read
    buf, offs, ks, vs, keys = C.count_batch(5)
    a = run.aligned(buf)
    kb, ko = C.pack_keys(keys)
    ko[3] = len(kb) - 1
    ko[4] = 2**64 - 1
    st, hc, bc = C.sentinels(5)
    rc = run.L.forst_blob_verify_batch(a.ctypes.data, len(buf), offs.ctypes.data, ks.ctypes.data,
                                       vs.ctypes.data, kb.ctypes.data, len(kb), ko.ctypes.data,
                                       st.ctypes.data, hc.ctypes.data, bc.ctypes.data, None, 5, None)
    assert rc == 0
    assert st[:5].tolist() == [0, 0, 0, B.KEY, B.KEY]


def test_emu_blob_split_launch_shuffled(run):
    # more records than the small-batch dispatch takes at the emulator's CU
    # count: the lane kernel + the rows filter kernel, payloads on both sides
    # of kRawSplit, shuffled order, flips in headers, keys and values
    n = 64 * D.CRC_WAVES * 2 + 70
    assert D.crc_raw_kernel(n, 1 << 20, 2) == "crc32c_rows_raw_filt_kernel"
    buf, offs, ks, vs, keys = C.many_short_records(n)
    est = C.check_verify(run, buf, offs, ks, vs, keys, nthreads=4)
    assert {B.HEADER_CRC, B.KEY, B.CRC} <= set(est.tolist()) and (est != 0).sum() == 24


def _files_call(run, files, cfs, misalign=0):
    """all files in one arena (file i at a 4-byte aligned offset + gaps) ->
    the results"""
    n = len(files)
    offs, pos = [], 8
    for f in files:
        offs.append(pos)
        pos += (len(f) + 11) & ~3
    arena = np.random.default_rng(3).integers(0, 256, pos + 4096, dtype=np.uint8)
    for o, f in zip(offs, files):
        arena[o:o + len(f)] = np.frombuffer(f, np.uint8)
    a = run.aligned(arena)
    keep = [np.frombuffer(f, np.uint8) for f in files]
    ptrs = (ctypes.c_void_p * n)(*[k.ctypes.data for k in keep])
    sizes = np.array([len(f) for f in files], np.uint64)
    doffs = np.array(offs, np.uint64)
    have_cf = np.array([c is not None for c in cfs])
    out = (C.FileResult * (n + 1))()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    if have_cf.all() or not have_cf.any():
        cf = np.array([c or 0 for c in cfs], np.uint32)
        rc = run.L.forst_blob_verify_files(ctypes.cast(ptrs, ctypes.c_void_p), sizes.ctypes.data,
                                           doffs.ctypes.data, a.ctypes.data, len(arena),
                                           cf.ctypes.data if have_cf.all() else None, n,
                                           ctypes.cast(out, ctypes.c_void_p), None)
        assert rc == 0, run.L.forst_last_error()
        assert bytes(out[n]) == b"\xA5" * ctypes.sizeof(C.FileResult)  # the guard slot
        return list(out)[:n]
    # expectations for some files only: two calls
    res = [None] * n
    for want in (True, False):
        idx = [i for i in range(n) if have_cf[i] == want]
        got = _files_call(run, [files[i] for i in idx], [cfs[i] for i in idx])
        for i, r in zip(idx, got):
            res[i] = r
    return res


def test_emu_blob_files_crafted(run):
    cases = C.damaged_files()
    res = _files_call(run, [f for _, f, _ in cases], [c for _, _, c in cases])
    reasons = set()
    for (name, data, cf), r in zip(cases, res):
        exp = B.scan_file(data, cf)
        C.same_result(r, exp, run.L)
        reasons.add(exp["reason"])
    assert reasons == set(range(12)), reasons  # every reason but RECORD_TOO_LARGE (a 4 GiB file)


def test_emu_blob_fixture_files(run):
    meta = json.load(open(os.path.join(GOLDEN, "blob_files.json")))
    names = sorted(meta["files"])
    files = [open(os.path.join(GOLDEN, "blob", n), "rb").read() for n in names]
    res = _files_call(run, files, [meta["files"][n]["column_family_id"] for n in names])
    for n, data, r in zip(names, files, res):
        m = meta["files"][n]
        assert C.header_text(r, run.L) == m["create_status"], n
        C.same_result(r, B.scan_file(data, m["column_family_id"]), run.L)
        # write mode regenerates the reference-written file byte for byte
        offs = np.array([rec["offset"] for rec in m["records"]], np.uint64)
        if len(offs):
            buf = np.frombuffer(data, np.uint8)
            out = C.check_write(run, C.zero_crc_fields(buf, offs), offs)
            assert (out == buf).all(), n
    # the damaged copies: the reference's first failure
    dam = meta["damaged"]
    files = [B.apply_damage(open(os.path.join(GOLDEN, "blob", d["file"]), "rb").read(), d)
             for d in dam]
    res = _files_call(run, files, [meta["files"][d["file"]]["column_family_id"] for d in dam])
    for d, r in zip(dam, res):
        B.check_against_reference(d, C.header_text(r, run.L), r.fail_index, r.reason)
