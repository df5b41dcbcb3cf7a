"""Blob file records on the MI355X (forst_blob_verify_batch,
forst_blob_record_crc_batch, forst_blob_verify_files through the Python
wrappers) against the restatement of tests/blobfile.py and the recorded
reference answers of tests/golden/blob_files.json: the emulator's cases
(tests/blobcases.py) on the device, the reference-written files regenerated
byte for byte by the writer call, every fixture and damaged copy in one file
scan, the GetBlob requests, and a batch large enough for the lane kernel + the
rows filter kernel."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import blobcases as C  # noqa: E402
import blobfile as B  # noqa: E402
import dispatch as D  # noqa: E402
from forst_amd import _lib, blob, engine  # noqa: E402
from oracle import oracle as O  # noqa: E402

DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def d(a):
    """a numpy array on the device (unsigned 32 / 64-bit arrays as their signed twins)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEV)


def h(t, dtype):
    return t.cpu().numpy().view(dtype)


class GpuRunner:
    """the runner of tests/blobcases.py over engine.blob_verify_batch /
    engine.blob_record_crc_batch, results in the caller's sentinel arrays"""

    def verify(self, buf, offs, eks=None, evs=None, ukeys=None, base_len=None):
        n = len(offs)
        base = d(buf)[:len(buf) if base_len is None else base_len]
        kb, ko = (None, None) if ukeys is None else \
            (ukeys if isinstance(ukeys, tuple) else C.pack_keys(ukeys))
        st, hc, bc = (d(a) for a in C.sentinels(n))
        mism = torch.zeros(2, dtype=torch.int64, device=DEV)
        engine.blob_verify_batch(base, d(np.asarray(offs, np.uint64)),
                                 None if eks is None else d(np.asarray(eks, np.uint64)),
                                 None if evs is None else d(np.asarray(evs, np.uint64)),
                                 None if kb is None else d(kb), None if ko is None else d(ko),
                                 status=st, header_crc=hc, blob_crc=bc, mismatches=mism)
        torch.cuda.synchronize()
        st, hc, bc = h(st, np.uint8), h(hc, np.uint32), h(bc, np.uint32)
        C.check_guards(n, st, hc, bc)
        assert int(mism[1]) == 0
        return st[:n], hc[:n], bc[:n], int(mism[0])

    def write(self, buf, offs, base_len=None):
        n = len(offs)
        whole = d(buf)
        base = whole[:len(buf) if base_len is None else base_len]
        st, hc, bc = (d(a) for a in C.sentinels(n))
        engine.blob_record_crc_batch(base, d(np.asarray(offs, np.uint64)), status=st,
                                     header_crc=hc, blob_crc=bc)
        torch.cuda.synchronize()
        st, hc, bc = h(st, np.uint8), h(hc, np.uint32), h(bc, np.uint32)
        C.check_guards(n, st, hc, bc)
        return whole.cpu().numpy(), st[:n], hc[:n], bc[:n]


@pytest.fixture(scope="module")
def run():
    engine.init_device()
    return GpuRunner()


@pytest.fixture(scope="module")
def num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def meta():
    return json.load(open(os.path.join(GOLDEN, "blob_files.json")))


def _read(name):
    return open(os.path.join(GOLDEN, "blob", name), "rb").read()


def test_gpu_blob_record_cases(run):
    seen = C.run_record_cases(run)
    assert seen == set(range(8))  # every status code at least once


def test_gpu_blob_writer_cases(run):
    C.run_writer_cases(run)


def test_gpu_blob_no_record_and_optional_outputs(run):
    base = torch.zeros(64, dtype=torch.uint8, device=DEV)
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    st, hc, bc = (d(a) for a in C.sentinels(0))
    engine.blob_verify_batch(base, none, status=st, header_crc=hc, blob_crc=bc)
    engine.blob_record_crc_batch(base, none, status=st, header_crc=hc, blob_crc=bc)
    torch.cuda.synchronize()
    C.check_guards(0, h(st, np.uint8), h(hc, np.uint32), h(bc, np.uint32))
    assert not base.any() and blob.blob_verify_files([], base, []) == []
    buf, offs, ks, vs, keys = C.count_batch(65)
    st, hc, bc, mism = engine.blob_verify_batch(d(buf), d(offs), header_crc=None, blob_crc=None)
    assert hc is None and bc is None and not st.any() and int(mism[0]) == 0
    # a buffer too short for one header: every record out of range, no CRC launch
    st, hc, bc, mism = engine.blob_verify_batch(d(buf)[:31], d(offs))
    assert (st == B.OUT_OF_RANGE).all() and int(mism[0]) == 65
    assert engine.last_kernel() == "blob_decode_kernel"


def test_gpu_blob_wrappers_validate_every_array(run):
    buf, offs, ks, vs, keys = C.count_batch(8)
    base, o = d(buf), d(offs)
    kb, ko = (d(a) for a in C.pack_keys(keys))
    good = dict(expect_key_sizes=d(ks), expect_value_sizes=d(vs), user_keys=kb, user_key_offsets=ko)
    engine.blob_verify_batch(base, o, **good)
    cpu64 = torch.zeros(8, dtype=torch.int64)
    bad = [dict(record_offsets=cpu64), dict(record_offsets=o.to(torch.int32)),
           dict(record_offsets=torch.zeros(16, dtype=torch.int64, device=DEV)[::2]),
           dict(expect_key_sizes=d(ks)[:7]), dict(expect_value_sizes=cpu64),
           dict(user_key_offsets=ko.to(torch.int32)), dict(user_keys=kb.to(torch.int32)),
           dict(user_keys=None), dict(expect_key_sizes=None),
           dict(status=torch.zeros(7, dtype=torch.uint8, device=DEV)),
           dict(status=torch.zeros(8, dtype=torch.uint8)),
           dict(header_crc=torch.zeros(8, dtype=torch.int64, device=DEV)),
           dict(blob_crc=torch.zeros(4, dtype=torch.int32, device=DEV)),
           dict(mismatches=torch.zeros(1, dtype=torch.int32, device=DEV))]
    for kw in bad:
        args = dict(good, record_offsets=o)
        args.update(kw)
        with pytest.raises((ValueError, TypeError)):
            engine.blob_verify_batch(base, **args)
    for kw in (dict(status=torch.zeros(7, dtype=torch.uint8, device=DEV)),
               dict(header_crc=torch.zeros(8, dtype=torch.uint32)),
               dict(blob_crc=torch.zeros(8, dtype=torch.uint8, device=DEV))):
        with pytest.raises((ValueError, TypeError)):
            engine.blob_record_crc_batch(base, o, **kw)
    with pytest.raises((ValueError, TypeError)):
        engine.blob_record_crc_batch(base, cpu64)
    with pytest.raises(AssertionError):
        engine.blob_verify_batch(torch.from_numpy(buf), o)


def _arena(files):
    offs, pos = [], 8
    for f in files:
        offs.append(pos)
        pos += (len(f) + 11) & ~3
    arena = np.random.default_rng(3).integers(0, 256, pos + 4096, dtype=np.uint8)
    for o, f in zip(offs, files):
        arena[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return d(arena), offs


def test_gpu_blob_files_crafted(run):
    cases = C.damaged_files()
    L = C.bind(_lib.lib())
    for want in (True, False):  # with and without a column family expectation
        sel = [(f, cf) for _, f, cf in cases if (cf is not None) == want]
        arena, offs = _arena([f for f, _ in sel])
        res = blob.blob_verify_files([f for f, _ in sel], arena, offs,
                                     [cf for _, cf in sel] if want else None)
        for (f, cf), r in zip(sel, res):
            C.same_result(r, B.scan_file(f, cf), L)


def test_gpu_blob_fixtures_regenerated_byte_for_byte(run, meta):
    for name, m in meta["files"].items():
        offs = np.array([r["offset"] for r in m["records"]], np.uint64)
        if len(offs) == 0:
            continue
        data = np.frombuffer(_read(name), np.uint8)
        out = C.check_write(run, C.zero_crc_fields(data, offs), offs)
        assert (out == data).all(), name


def test_gpu_blob_fixtures_and_damaged_copies_in_one_scan(run, meta):
    names = sorted(meta["files"])
    files = [_read(n) for n in names] + [B.apply_damage(_read(x["file"]), x) for x in meta["damaged"]]
    cfs = [meta["files"][n]["column_family_id"] for n in names] + \
          [meta["files"][x["file"]]["column_family_id"] for x in meta["damaged"]]
    arena, offs = _arena(files)
    res = blob.blob_verify_files(files, arena, offs, cfs)
    L = C.bind(_lib.lib())
    for n, f, r in zip(names, files, res):
        assert r.text == meta["files"][n]["create_status"], n
        C.same_result(r, B.scan_file(f, meta["files"][n]["column_family_id"]), L)
        if r.status == 0:
            assert r.blob_count == len(meta["files"][n]["records"])
    for x, f, cf, r in zip(meta["damaged"], files[len(names):], cfs[len(names):], res[len(names):]):
        B.check_against_reference(x, r.text, r.fail_index, r.reason)
        C.same_result(r, B.scan_file(f, cf), L)


def test_gpu_blob_getblob_requests(run, meta):
    """every recorded GetBlob(verify_checksums) request in one verify batch per
    file image: the reference's Status strings"""
    reqs = meta["requests"]
    images, where = [], []
    for q in reqs:
        data, off, ks, vs, key = B.request_inputs(q, _read(q["file"]))
        images.append(data)
        where.append((off, ks, vs, key))
    arena, offs = _arena(images)
    st, _, _, mism = engine.blob_verify_batch(
        arena, d(np.array([o + w[0] for o, w in zip(offs, where)], np.uint64)),
        d(np.array([w[1] for w in where], np.uint64)), d(np.array([w[2] for w in where], np.uint64)),
        *(d(a) for a in C.pack_keys([w[3] for w in where])))
    st = h(st, np.uint8)
    for q, s in zip(reqs, st):
        assert B.RECORD_TEXT[int(s)] == q["status"], q
    assert int(mism[0]) == sum(q["status"] != "OK" for q in reqs)


def test_gpu_blob_large_shuffled_batch(run, num_cus):
    """the lane kernel + crc32c_rows_raw_filt_kernel under the blob kernels"""
    n = 64 * D.CRC_WAVES * num_cus
    threads = O.host_threads()
    buf, offs, ks, vs, keys = C.big_batch(n, nthreads=threads)
    assert D.crc_raw_kernel(n, len(buf), num_cus) == "crc32c_rows_raw_filt_kernel"
    est = C.check_verify(run, buf, offs, ks, vs, keys, nthreads=threads)
    assert engine.last_kernel() == "crc32c_rows_raw_filt_kernel"
    assert (est != 0).sum() == 64 and {B.HEADER_CRC, B.KEY, B.CRC} <= set(est.tolist())
    # the writer over the same image: both CRC fields of every record whose
    # (possibly damaged) sizes still fit are rewritten, so a verify without
    # expectations finds the flipped keys and values sound again; only records
    # with a flipped size can still fail (a size that no longer fits keeps the
    # stale header CRC; a payload grown over the next header was hashed before
    # that header's CRC fields were stored)
    out = C.check_write(run, buf, offs, nthreads=threads)
    assert engine.last_kernel() == "crc32c_rows_raw_filt_kernel"
    est = C.check_verify(run, out, offs, nthreads=threads)
    assert (est != 0).sum() <= 22


def test_gpu_blob_eight_files_of_4k_values(run, num_cus):
    rng = np.random.default_rng(99)
    files, offs_in = [], []
    for f in range(8):
        kv = [(b"key-%d-%04d" % (f, i), rng.integers(0, 256, 4096, dtype=np.uint8).tobytes())
              for i in range(48)]
        data, offs = B.build_file(kv, cf=f)
        files.append(data)
        offs_in.append(offs)
    last = bytearray(files[7])
    last[offs_in[7][-1] + 32 + 2000] ^= 0x10
    files[7] = bytes(last)
    arena, offs = _arena(files)
    res = blob.blob_verify_files(files, arena, offs, list(range(8)))
    assert engine.last_kernel() == D.crc_raw_kernel(8 * 48 + 8, arena.numel(), num_cus)
    for f, r in enumerate(res[:7]):
        assert (r.status, r.reason, r.blob_count, r.column_family_id) == (0, 0, 48, f)
        assert r.total_blob_bytes == len(files[f]) - 62
    r = res[7]
    assert (r.status, r.reason, r.fail_index, r.fail_offset) == \
        (2, B.F_RECORD_BLOB_CRC, 47, offs_in[7][-1])
    assert r.text == "Corruption: Blob CRC mismatch"
