"""Python mirror of the reference's checksum interface over the HIP engine.

Names follow the reference (table/format.h, table/block_based/reader_common.h,
util/crc32c.h, util/xxhash.h, db/log_reader.cc); every function is the batched
GPU form of the reference's per-block CPU call and runs the gfx950 kernels in
forst_amd/lib/libforst_checksum.so.  Device buffers are torch CUDA tensors
(torch is only plumbing for device memory and streams).  Calls are enqueued on
torch's current stream.
"""
import ctypes
import enum

import numpy as np
import torch

from ._lib import check, lib


class ChecksumType(enum.IntEnum):
    """include/rocksdb/table.h:54-60"""
    kNoChecksum = 0
    kCRC32c = 1
    kxxHash = 2
    kxxHash64 = 3
    kXXH3 = 4


class WalStatus(enum.IntEnum):
    """per-log-block outcome of forst_wal_verify_batch"""
    OK = 0
    BAD_CHECKSUM = 1
    BAD_LENGTH = 2
    ZERO_RECORD = 3
    OLD_RECORD = 4


def _p(t):
    return None if t is None else t.data_ptr()


def _stream(stream):
    if stream is None:
        return torch.cuda.current_stream().cuda_stream
    if isinstance(stream, torch.cuda.Stream):
        return stream.cuda_stream
    return stream


def _dev_u8(base):
    assert base.is_cuda and base.dtype == torch.uint8 and base.is_contiguous()
    return base


def _desc(offsets, sizes):
    assert offsets.is_cuda and offsets.dtype in (torch.int64, torch.uint64)
    assert sizes.is_cuda and sizes.dtype in (torch.int32, torch.uint32)
    assert offsets.is_contiguous() and sizes.is_contiguous()
    assert offsets.numel() == sizes.numel()
    return offsets.numel()


def init_device():
    check(lib().forst_init_device())


def version():
    return lib().forst_version().decode()


def last_kernel():
    return lib().forst_last_kernel().decode()


def block_checksum_batch(ctype, base, offsets, sizes, last_bytes=None, modifiers=None,
                         out=None, stream=None):
    """ComputeBuiltinChecksumWithLastByte + ChecksumModifierForContext per block
    (table/format.cc:594, table/format.h:119) -> uint32 tensor."""
    n = _desc(offsets, sizes)
    _dev_u8(base)
    if out is None:
        out = torch.empty(n, dtype=torch.uint32, device=base.device)
    check(lib().forst_block_checksum_batch(int(ctype), base.data_ptr(), base.numel(),
                                           offsets.data_ptr(), sizes.data_ptr(),
                                           _p(last_bytes), _p(modifiers), out.data_ptr(),
                                           n, _stream(stream)))
    return out


def block_trailer_batch(ctype, base, offsets, sizes, last_bytes, modifiers=None, out=None,
                        stream=None):
    """Writes [type][LE32 checksum] after each block in place, as
    BlockBasedTableBuilder::WriteMaybeCompressedBlock appends it."""
    n = _desc(offsets, sizes)
    _dev_u8(base)
    check(lib().forst_block_trailer_batch(int(ctype), base.data_ptr(), base.numel(),
                                          offsets.data_ptr(), sizes.data_ptr(),
                                          _p(last_bytes), _p(modifiers), _p(out),
                                          n, _stream(stream)))
    return out


def block_verify_batch(ctype, base, offsets, sizes, modifiers=None, computed=True,
                       stored=True, ok=True, mismatches=None, stream=None):
    """VerifyBlockChecksum per block (table/block_based/reader_common.cc:26).
    Returns (computed, stored, ok, mismatches) tensors (None where not asked)."""
    n = _desc(offsets, sizes)
    _dev_u8(base)
    dev = base.device
    c = torch.empty(n, dtype=torch.uint32, device=dev) if computed is True else computed
    s = torch.empty(n, dtype=torch.uint32, device=dev) if stored is True else stored
    o = torch.empty(n, dtype=torch.uint8, device=dev) if ok is True else ok
    if mismatches is None:
        mismatches = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib().forst_block_verify_batch(int(ctype), base.data_ptr(), base.numel(),
                                         offsets.data_ptr(), sizes.data_ptr(), _p(modifiers),
                                         _p(c), _p(s), _p(o), _p(mismatches), n,
                                         _stream(stream)))
    return c, s, o, mismatches


def crc32c_batch(base, offsets, lengths, init_crcs=None, out=None, stream=None):
    """crc32c::Extend(init, data, n) per buffer (util/crc32c.h:25), unmasked."""
    n = _desc(offsets, lengths)
    _dev_u8(base)
    if out is None:
        out = torch.empty(n, dtype=torch.uint32, device=base.device)
    check(lib().forst_crc32c_batch(base.data_ptr(), base.numel(), offsets.data_ptr(),
                                   lengths.data_ptr(), _p(init_crcs), out.data_ptr(), n,
                                   _stream(stream)))
    return out


def crc32c_buffer(base, init=0, out=None, stream=None):
    """crc32c::Extend(init, base) over one device buffer of any size
    (FileChecksumGenCrc32c, util/file_checksum_helper.h:22).  Returns a
    1-element uint32 device tensor."""
    _dev_u8(base)
    if out is None:
        out = torch.empty(1, dtype=torch.uint32, device=base.device)
    check(lib().forst_crc32c_buffer(base.data_ptr(), base.numel(), init & 0xFFFFFFFF,
                                    out.data_ptr(), _stream(stream)))
    return out


def crc32c_files(arena, offsets, lengths, inits=None, out=None, stream=None):
    """crc32c::Extend(inits[i] or 0, arena[offsets[i] : offsets[i] + lengths[i]])
    for a set of files in one call (FileChecksumGenCrc32c over every file of
    DB::VerifyFileChecksums, util/file_checksum_helper.h:22).  arena: a uint8
    device tensor; offsets / lengths / inits: HOST sequences (the caller knows
    its file sizes).  Returns a uint32 device tensor of len(offsets) entries
    (`out`: the caller's own, at least that long; entries past them are left
    alone)."""
    _dev_u8(arena)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    lens = np.ascontiguousarray(lengths, dtype=np.uint64)
    assert offs.ndim == 1 and offs.shape == lens.shape
    n = len(offs)
    ini = None
    if inits is not None:
        ini = np.ascontiguousarray(inits, dtype=np.uint32)
        assert ini.shape == offs.shape
    if out is None:
        out = torch.empty(n, dtype=torch.uint32, device=arena.device)
    assert out.device == arena.device
    _out(out, n, 4)
    check(lib().forst_crc32c_files(arena.data_ptr(), arena.numel(), offs.ctypes.data,
                                   lens.ctypes.data, None if ini is None else ini.ctypes.data,
                                   out.data_ptr(), n, _stream(stream)))
    return out[:n]


def crc32c_combine_batch(crc1, crc2, len2, out=None, stream=None):
    """crc32c::Crc32cCombine per element (util/crc32c.h:32), device arrays."""
    n = crc1.numel()
    if out is None:
        out = torch.empty(n, dtype=torch.uint32, device=crc1.device)
    check(lib().forst_crc32c_combine_batch(crc1.data_ptr(), crc2.data_ptr(), len2.data_ptr(),
                                           out.data_ptr(), n, _stream(stream)))
    return out


def crc32c_combine(crc1, crc2, len2):
    """host crc32c::Crc32cCombine (no GPU call)."""
    return lib().forst_crc32c_combine(crc1 & 0xFFFFFFFF, crc2 & 0xFFFFFFFF, len2)


def xxh3_64_batch(base, offsets, lengths, out=None, stream=None):
    """XXH3_64bits per buffer (util/xxhash.h:5311)."""
    n = _desc(offsets, lengths)
    _dev_u8(base)
    if out is None:
        out = torch.empty(n, dtype=torch.uint64, device=base.device)
    check(lib().forst_xxh3_64_batch(base.data_ptr(), base.numel(), offsets.data_ptr(),
                                    lengths.data_ptr(), out.data_ptr(), n, _stream(stream)))
    return out


def wal_verify_batch(log, log_number=0, first_block=0, n_blocks=None, bad_blocks=None,
                     stream=None, status=True, nrec=True, fail_off=True):
    """Physical-record CRC verification of 32 KiB log blocks
    (db/log_reader.cc:450-531).  Returns (status, nrec, fail_off, bad_blocks)
    (None where not asked; a tensor given for an output is filled)."""
    _dev_u8(log)
    total = (log.numel() + 32767) // 32768
    if n_blocks is None:
        n_blocks = total - first_block
    dev = log.device
    st = torch.empty(n_blocks, dtype=torch.uint8, device=dev) if status is True else status
    nr = torch.empty(n_blocks, dtype=torch.uint32, device=dev) if nrec is True else nrec
    fo = torch.empty(n_blocks, dtype=torch.uint32, device=dev) if fail_off is True else fail_off
    if bad_blocks is None:
        bad_blocks = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib().forst_wal_verify_batch(log.data_ptr(), log.numel(), first_block, n_blocks,
                                       log_number, _p(st), _p(nr), _p(fo),
                                       bad_blocks.data_ptr(), _stream(stream)))
    return st, nr, fo, bad_blocks


def wal_record_crc_batch(log, header_offsets, write_in_place=True, out=None, stream=None,
                         payload_lengths=None, recyclable=False):
    """log::Writer::EmitPhysicalRecord CRC (db/log_writer.cc:228-263) for
    headers already laid out in `log`.  With payload_lengths (device int32,
    the lengths the writer laid out: forst_wal_record_crc_lengths) the
    descriptors come from the arrays instead of a pass over the headers."""
    _dev_u8(log)
    n = header_offsets.numel()
    if out is None:
        out = torch.empty(n, dtype=torch.uint32, device=log.device)
    if payload_lengths is not None:
        assert payload_lengths.numel() == n and payload_lengths.element_size() == 4
        check(lib().forst_wal_record_crc_lengths(log.data_ptr(), log.numel(),
                                                 header_offsets.data_ptr(),
                                                 payload_lengths.data_ptr(), n, int(recyclable),
                                                 int(write_in_place), out.data_ptr(),
                                                 _stream(stream)))
        return out
    check(lib().forst_wal_record_crc_batch(log.data_ptr(), log.numel(),
                                           header_offsets.data_ptr(), n, int(write_in_place),
                                           out.data_ptr(), _stream(stream)))
    return out


def _out(t, n, size):
    """a caller's output tensor: on the device, contiguous, `size`-byte
    integers, at least n of them"""
    assert t.is_cuda and t.is_contiguous() and not t.dtype.is_floating_point
    assert t.element_size() == size and t.numel() >= n, (t.dtype, t.numel(), n)
    return t


def wal_record_xxh3_batch(log, header_offsets, stream=None, hashes=None, first=None):
    """XXH3_64bits per logical record (log_reader.cc:95-165).  Returns
    (hashes int64 [n_logical], first physical record index [n_logical]).
    hashes / first: the caller's own output tensors (64-bit, n_phys entries);
    first=False passes NULL for first_phys (None is returned for it)."""
    _dev_u8(log)
    n = header_offsets.numel()
    if hashes is None:
        hashes = torch.empty(max(n, 1), dtype=torch.int64, device=log.device)
    if first is None:
        first = torch.empty(max(n, 1), dtype=torch.int64, device=log.device)
    _out(hashes, n, 8)
    if first is not False:
        _out(first, n, 8)
    nl = ctypes.c_uint64()
    check(lib().forst_wal_record_xxh3_batch(log.data_ptr(), log.numel(), header_offsets.data_ptr(),
                                            n, hashes.data_ptr(),
                                            None if first is False else first.data_ptr(),
                                            ctypes.byref(nl), _stream(stream)))
    return hashes[:nl.value], None if first is False else first[:nl.value]


class WalRecords(ctypes.Structure):
    """forst_wal_records (device array pointers)"""
    _fields_ = [("offset", ctypes.c_void_p), ("length", ctypes.c_void_p),
                ("hash", ctypes.c_void_p), ("n_fragments", ctypes.c_void_p)]


class WalReports(ctypes.Structure):
    """forst_wal_reports (device array pointers)"""
    _fields_ = [("offset", ctypes.c_void_p), ("bytes", ctypes.c_void_p),
                ("reason", ctypes.c_void_p), ("type", ctypes.c_void_p)]


class WalRecoverResult(ctypes.Structure):
    _fields_ = [("n_records", ctypes.c_uint64), ("n_reports", ctypes.c_uint64),
                ("n_physical", ctypes.c_uint64), ("stop_offset", ctypes.c_uint64),
                ("stop_reason", ctypes.c_uint32), ("truncated", ctypes.c_uint32),
                ("unsupported", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


# forst_wal_report_reason -> the reader's Reporter::Corruption text (log_reader.cc)
WAL_REASONS = {1: "partial record without end(1)", 2: "partial record without end(2)",
               3: "missing start of fragmented record(1)",
               4: "missing start of fragmented record(2)", 5: "error in middle of record",
               6: "checksum mismatch", 7: "bad record length", 8: "truncated header",
               9: "error reading trailing data", 10: "truncated record body",
               11: "unknown record type %u"}
WAL_STOPS = {0: "eof", 1: "old_record", 2: "truncated_header", 3: "truncated_body",
             4: "recycled_tail"}
# WALRecoveryMode (include/rocksdb/options.h)
kTolerateCorruptedTailRecords, kAbsoluteConsistency, kPointInTimeRecovery, \
    kSkipAnyCorruptedRecords = 0, 1, 2, 3


def _recover_sig(L):
    f = L.forst_wal_recover_batch
    if f.argtypes is None:
        vp, u64 = ctypes.c_void_p, ctypes.c_uint64
        f.restype = ctypes.c_int
        f.argtypes = [vp, u64, ctypes.c_uint32, ctypes.c_int, WalRecords, u64, WalReports, u64,
                      vp, vp]


WAL_RECORD_FIELDS = (("offset", 8), ("length", 8), ("hash", 8), ("n_fragments", 4))
WAL_REPORT_FIELDS = (("offset", 8), ("bytes", 8), ("reason", 4), ("type", 4))


def _wal_members(given, fields, capacity, dev):
    """the tensors behind one of forst_wal_recover_batch's output structs ->
    (dict with every member; None = a NULL member, capacity).  given: None (the
    wrapper allocates `capacity` entries) or the caller's dict."""
    if given is None:
        return {k: torch.empty(capacity, dtype=torch.int64 if size == 8 else torch.int32,
                               device=dev) for k, size in fields}, capacity
    assert set(given) <= {k for k, _ in fields}, sorted(given)
    out = {k: given.get(k) for k, _ in fields}
    held = [t.numel() for t in out.values() if t is not None]
    if capacity is None:
        capacity = min(held) if held else 0
    for k, size in fields:
        if out[k] is not None:
            _out(out[k], capacity, size)
    return out, capacity


def wal_recover_batch(log, log_number=0, mode=kPointInTimeRecovery, record_capacity=None,
                      report_capacity=None, stream=None, records=None, reports=None, retry=True):
    """log::Reader::ReadRecord over a whole device log image (log_reader.cc:69-320):
    returns (records dict of device tensors offset/length/hash/n_fragments,
    reports dict of device tensors offset/bytes/reason/type, result).
    records / reports: the caller's own output tensors by member name; a member
    that is missing or None is passed as NULL (and returned as None).
    record_capacity / report_capacity may be smaller than those tensors; left
    out, they are what the tensors hold (without tensors: log bytes / 1024 and
    1024).  A call that comes back truncated is repeated with arrays of the
    reported counts -- for the arrays the wrapper allocated, and unless
    retry=False, which returns the call's result as it is: the tensors
    unsliced, result.truncated set."""
    _dev_u8(log)
    _recover_sig(lib())
    dev = log.device
    if records is None and record_capacity is None:
        record_capacity = max(1024, log.numel() // 1024)
    if reports is None and report_capacity is None:
        report_capacity = 1024
    while True:
        rec, record_capacity = _wal_members(records, WAL_RECORD_FIELDS, record_capacity, dev)
        rep, report_capacity = _wal_members(reports, WAL_REPORT_FIELDS, report_capacity, dev)
        res = WalRecoverResult()
        check(lib().forst_wal_recover_batch(
            log.data_ptr(), log.numel(), log_number, mode,
            WalRecords(*[_p(rec[k]) for k, _ in WAL_RECORD_FIELDS]), record_capacity,
            WalReports(*[_p(rep[k]) for k, _ in WAL_REPORT_FIELDS]), report_capacity,
            ctypes.byref(res), _stream(stream)))
        grow_rec = records is None and res.n_records > record_capacity
        grow_rep = reports is None and res.n_reports > report_capacity
        if not retry or not (grow_rec or grow_rep):
            break
        if grow_rec:
            record_capacity = res.n_records
        if grow_rep:
            report_capacity = res.n_reports
    if not retry:
        return rec, rep, res
    nr, np_ = min(res.n_records, record_capacity), min(res.n_reports, report_capacity)
    rec = {k: None if v is None else v[:nr] for k, v in rec.items()}
    rep = {k: None if v is None else v[:np_] for k, v in rep.items()}
    return rec, rep, res


def wal_records_compact(log, records, arena=None, stream=None):
    """The bytes log::Reader::ReadRecord returns for each record, contiguous in
    a device arena (forst_wal_records_compact): the reps
    write_batch_protect_batch and xxh3_64_batch take.  records: the dict
    wal_recover_batch returns (its offset / length / n_fragments members) or
    the tuple (offset, length, hash, n_fragments); any subset or order of a
    log's records.  Returns (arena, rep_offsets int64,
    rep_sizes int32, status uint8): record i's bytes are
    arena[rep_offsets[i]:rep_offsets[i] + rep_sizes[i]], every rep on a 16-byte
    boundary with zero padding behind it, the arena cut to the bytes used.
    arena: the caller's own uint8 tensor (16-byte aligned, apart from the log);
    left out, it is sized by a first, count-only call.  An arena below the
    total raises a ForstError whose arena_bytes is the size to call again with.
    Synchronous (one read-back of the total per call)."""
    _dev_u8(log)
    if isinstance(records, dict):
        off, length, nfrag = (records[k] for k in ("offset", "length", "n_fragments"))
    else:  # (offset, length, hash, n_fragments), the members in struct order
        off, length, _, nfrag = records
    n = off.numel()
    for t, size in ((off, 8), (length, 8), (nfrag, 4)):
        assert t.device == log.device, (t.device, log.device)
        _out(t, n, size)
        assert t.numel() == n, (t.numel(), n)
    dev = log.device
    rep_off = torch.empty(n, dtype=torch.int64, device=dev)
    rep_size = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    total = ctypes.c_uint64()
    args = (log.data_ptr(), log.numel(), off.data_ptr(), length.data_ptr(), nfrag.data_ptr(), n)
    outs = (rep_off.data_ptr(), rep_size.data_ptr(), status.data_ptr(), ctypes.byref(total),
            _stream(stream))
    if arena is None:
        check(lib().forst_wal_records_compact(*args, None, 0, *outs))
        arena = torch.empty(max(16, total.value), dtype=torch.uint8, device=dev)
    assert arena.device == dev and arena.dtype == torch.uint8 and arena.is_contiguous()
    rc = lib().forst_wal_records_compact(*args, arena.data_ptr(), arena.numel(), *outs)
    check(rc, arena_bytes=total.value)
    return arena[:total.value], rep_off, rep_size, status


class WalFrameResult(ctypes.Structure):
    """forst_wal_frame_result"""
    _fields_ = [("image_bytes", ctypes.c_uint64), ("n_physical", ctypes.c_uint64),
                ("n_pads", ctypes.c_uint64), ("bad_records", ctypes.c_uint64),
                ("end_block_offset", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def wal_frame_batch(base, rep_offsets, rep_sizes, recyclable, log_number, block_offset=0,
                    image=None, host_sizes=None, stream=None):
    """What log::Writer::AddRecord appends for the records
    base[rep_offsets[i]:rep_offsets[i] + rep_sizes[i]] (device tensors, the
    shape wal_records_compact returns and write_batch_protect_batch takes),
    framed on the device from block_offset (forst_wal_frame_batch): payloads,
    headers with their CRCs, zero block tails.  Returns (image, desc, result):
    the image cut to the appended bytes; desc with rec_offsets int64 [n],
    phys_offsets int64 / phys_lengths int32 / phys_types uint8 [n_physical]
    and status uint8 [n] (1: the rep reaches past base, framed as zeros);
    result a WalFrameResult.  image: the caller's own uint8 tensor (16-byte
    aligned, apart from base); one below the total raises a ForstError whose
    image_bytes is the size to call again with.  host_sizes: a CPU copy of
    rep_sizes (int32 tensor), read back from the device when left out.
    Synchronous."""
    _dev_u8(base)
    n = _desc(rep_offsets, rep_sizes)
    dev = base.device
    assert rep_offsets.device == dev and rep_sizes.device == dev, (rep_offsets.device, dev)
    if host_sizes is None:
        host_sizes = rep_sizes.cpu()
    assert not host_sizes.is_cuda and host_sizes.dtype in (torch.int32, torch.uint32)
    assert host_sizes.is_contiguous() and host_sizes.numel() == n, (host_sizes.numel(), n)
    res = WalFrameResult()
    args = (base.data_ptr(), base.numel(), rep_offsets.data_ptr(), rep_sizes.data_ptr(),
            host_sizes.data_ptr(), n, int(bool(recyclable)), log_number, block_offset)
    # the placement alone: sizes the image and the descriptor arrays
    check(lib().forst_wal_frame_batch(*args, None, 0, None, None, None, None, 0, None,
                                      ctypes.byref(res), _stream(stream)))
    nph = res.n_physical
    if image is None:
        image = torch.empty(max(16, res.image_bytes), dtype=torch.uint8, device=dev)
    assert image.device == dev and image.dtype == torch.uint8 and image.is_contiguous()
    desc = {"rec_offsets": torch.empty(n, dtype=torch.int64, device=dev),
            "phys_offsets": torch.empty(nph, dtype=torch.int64, device=dev),
            "phys_lengths": torch.empty(nph, dtype=torch.int32, device=dev),
            "phys_types": torch.empty(nph, dtype=torch.uint8, device=dev),
            "status": torch.empty(n, dtype=torch.uint8, device=dev)}
    rc = lib().forst_wal_frame_batch(
        *args, image.data_ptr(), image.numel(), _p(desc["rec_offsets"]), _p(desc["phys_offsets"]),
        _p(desc["phys_lengths"]), _p(desc["phys_types"]), nph, _p(desc["status"]),
        ctypes.byref(res), _stream(stream))
    check(rc, image_bytes=res.image_bytes)
    return image[:res.image_bytes], desc, res


def hash64_batch(base, offsets, lengths, seeds=None, seed=0, out=None, stream=None):
    """Hash64 / NPHash64 per buffer (util/hash.cc:81, XXPH3 0.7.2 preview)."""
    n = _desc(offsets, lengths)
    _dev_u8(base)
    if out is None:
        out = torch.empty(n, dtype=torch.uint64, device=base.device)
    check(lib().forst_hash64_batch(base.data_ptr(), base.numel(), offsets.data_ptr(),
                                   lengths.data_ptr(), _p(seeds), seed & (2**64 - 1),
                                   out.data_ptr(), n, _stream(stream)))
    return out


def kv_protect_batch(base, key_offsets, key_sizes, value_offsets, value_sizes, op_types=None,
                     seqnos=None, cf_ids=None, out=None, stream=None):
    """ProtectionInfo64 ProtectKV / ProtectKVO [+S] [+C] per entry (db/kv_checksum.h)."""
    n = _desc(key_offsets, key_sizes)
    assert _desc(value_offsets, value_sizes) == n
    _dev_u8(base)
    if out is None:
        out = torch.empty(n, dtype=torch.uint64, device=base.device)
    check(lib().forst_kv_protect_batch(base.data_ptr(), base.numel(), key_offsets.data_ptr(),
                                       key_sizes.data_ptr(), value_offsets.data_ptr(),
                                       value_sizes.data_ptr(), _p(op_types), _p(seqnos),
                                       _p(cf_ids), out.data_ptr(), n, _stream(stream)))
    return out


def kv_verify_batch(base, key_offsets, key_sizes, value_offsets, value_sizes, protection_bytes,
                    checksum_offsets, op_types=None, seqnos=None, cf_ids=None, computed=True,
                    ok=True, mismatches=None, stream=None):
    """ProtectionInfo<T>::Verify per entry (db/kv_checksum.h:117-133), e.g.
    MemTable::VerifyEntryChecksum.  Returns (computed, ok, mismatches)."""
    n = _desc(key_offsets, key_sizes)
    _dev_u8(base)
    dev = base.device
    c = torch.empty(n, dtype=torch.uint64, device=dev) if computed is True else computed
    o = torch.empty(n, dtype=torch.uint8, device=dev) if ok is True else ok
    if mismatches is None:
        mismatches = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib().forst_kv_verify_batch(base.data_ptr(), base.numel(), key_offsets.data_ptr(),
                                      key_sizes.data_ptr(), value_offsets.data_ptr(),
                                      value_sizes.data_ptr(), _p(op_types), _p(seqnos),
                                      _p(cf_ids), protection_bytes, checksum_offsets.data_ptr(),
                                      _p(c), _p(o), _p(mismatches), n, _stream(stream)))
    return c, o, mismatches


def memtable_verify_batch(base, entry_offsets, protection_bytes, computed=True, status=True,
                          mismatches=None, stream=None):
    """MemTable::VerifyEntryChecksum per encoded entry (db/memtable.cc:273-307),
    decoded on the device.  Returns (computed, status, mismatches); status
    codes as in include/forst_checksum.h."""
    _dev_u8(base)
    n = entry_offsets.numel()
    dev = base.device
    c = torch.empty(n, dtype=torch.uint64, device=dev) if computed is True else computed
    s = torch.empty(n, dtype=torch.uint8, device=dev) if status is True else status
    if mismatches is None:
        mismatches = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib().forst_memtable_verify_batch(base.data_ptr(), base.numel(), entry_offsets.data_ptr(),
                                            n, protection_bytes, _p(c), _p(s), _p(mismatches),
                                            _stream(stream)))
    return c, s, mismatches


def memtable_protect_batch(base, entry_offsets, protection_bytes, write_in_place=True, out=True,
                           status=True, stream=None):
    """MemTable::UpdateEntryChecksum per encoded entry (db/memtable.cc:676-693):
    the protection value, written in place as Encode(protection_bytes).
    Returns (out, status)."""
    _dev_u8(base)
    n = entry_offsets.numel()
    dev = base.device
    o = torch.empty(n, dtype=torch.uint64, device=dev) if out is True else out
    s = torch.empty(n, dtype=torch.uint8, device=dev) if status is True else status
    check(lib().forst_memtable_protect_batch(base.data_ptr(), base.numel(),
                                             entry_offsets.data_ptr(), n, protection_bytes,
                                             1 if write_in_place else 0, _p(o), _p(s),
                                             _stream(stream)))
    return o, s


def write_batch_protect_batch(base, rep_offsets, rep_sizes, capacity=None, stream=None, prot=None,
                              first_entry=None, status=None, n_protected=None):
    """WriteBatchInternal::UpdateProtectionInfo per WriteBatch rep
    (db/write_batch.cc:3164-3181), parsed on the device.  Returns
    (prot, first_entry, status, n_protected): rep b's protection values are
    prot[first_entry[b]:first_entry[b+1]].  Synchronous (one count read-back).
    prot / first_entry / status / n_protected: the caller's own output tensors
    (u64[capacity], i64[n + 1], u8[n], i32[n]); status=False / n_protected=False
    pass NULL (None is returned for them).  With prot given and no capacity,
    the capacity is what prot holds.  A capacity below the total raises a
    ForstError whose n_total is the capacity to call again with."""
    _dev_u8(base)
    n = _desc(rep_offsets, rep_sizes)
    dev = base.device
    first = first_entry
    if first is None:
        first = torch.empty(n + 1, dtype=torch.int64, device=dev)
    _out(first, n + 1, 8)
    if status is None:
        status = torch.empty(n, dtype=torch.uint8, device=dev)
    if n_protected is None:
        n_protected = torch.empty(n, dtype=torch.int32, device=dev)
    st = None if status is False else _out(status, n, 1)
    nprot = None if n_protected is False else _out(n_protected, n, 4)
    total = ctypes.c_uint64()
    args = (base.data_ptr(), base.numel(), rep_offsets.data_ptr(), rep_sizes.data_ptr(), n,
            first.data_ptr())
    if capacity is None and prot is not None:
        capacity = prot.numel()
    if capacity is None:  # size from the header counts: a first call with capacity 0
        rc = lib().forst_write_batch_protect_batch(*args, None, 0, None, None,
                                                   ctypes.byref(total), _stream(stream))
        if rc != 0 and total.value == 0:
            check(rc)
        capacity = total.value
    if prot is None:
        prot = torch.empty(max(1, capacity), dtype=torch.uint64, device=dev)
    _out(prot, capacity, 8)
    rc = lib().forst_write_batch_protect_batch(*args, prot.data_ptr(), capacity, _p(st),
                                               _p(nprot), ctypes.byref(total), _stream(stream))
    check(rc, n_total=total.value)
    return prot[:total.value], first[:n + 1], st if st is None else st[:n], \
        nprot if nprot is None else nprot[:n]


class BlockKind(enum.IntFlag):
    """kinds[] of block_kv_checksum_batch (include/forst_checksum.h)"""
    DATA = 0
    INDEX = 1
    META = 2
    VALUE_IS_FULL = 4
    HAS_FIRST_KEY = 8


def block_kv_checksum_batch(base, block_offsets, block_sizes, kinds, protection_bytes,
                            capacity=None, stream=None, kv_checksums=None, prot=None,
                            first_key=None, status=None):
    """Block::Initialize{Data,Index,MetaIndex}BlockProtectionInfo per block
    (table/block_based/block.cc:1113-1235), decoded on the device.  Returns
    (kv_checksums u8, prot u64, first_key, status): block b's kv_checksum_ is
    kv_checksums[first_key[b] * pb : first_key[b+1] * pb].  Synchronous.
    kv_checksums / prot / first_key / status: the caller's own output tensors
    (u8[capacity * pb], u64[capacity], i64[n + 1], u8[n]); with kv_checksums
    given and no capacity, the capacity is what kv_checksums (and prot) hold."""
    _dev_u8(base)
    n = _desc(block_offsets, block_sizes)
    dev = base.device
    first = first_key
    if first is None:
        first = torch.empty(n + 1, dtype=torch.int64, device=dev)
    assert first.is_cuda and first.dtype in (torch.int64, torch.uint64) and first.is_contiguous()
    assert first.numel() >= n + 1
    if status is None:
        status = torch.empty(n, dtype=torch.uint8, device=dev)
    assert status.is_cuda and status.dtype == torch.uint8 and status.is_contiguous()
    assert status.numel() >= n
    total = ctypes.c_uint64()
    args = (base.data_ptr(), base.numel(), block_offsets.data_ptr(), block_sizes.data_ptr(),
            kinds.data_ptr(), n, protection_bytes, first.data_ptr())
    if capacity is None and kv_checksums is not None:
        capacity = kv_checksums.numel() // protection_bytes
        if prot is not None:
            capacity = min(capacity, prot.numel())
    if capacity is None:
        rc = lib().forst_block_kv_checksum_batch(*args, None, None, 0, None, ctypes.byref(total),
                                                 _stream(stream))
        if rc != 0 and total.value == 0:
            check(rc)
        capacity = total.value
    enc = kv_checksums
    if enc is None:
        enc = torch.empty(max(1, capacity) * protection_bytes, dtype=torch.uint8, device=dev)
    _dev_u8(enc)
    assert enc.numel() >= capacity * protection_bytes
    if prot is None:
        prot = torch.empty(max(1, capacity), dtype=torch.uint64, device=dev)
    assert prot.is_cuda and prot.dtype in (torch.int64, torch.uint64) and prot.is_contiguous()
    assert prot.numel() >= capacity
    check(lib().forst_block_kv_checksum_batch(*args, enc.data_ptr(), prot.data_ptr(), capacity,
                                              status.data_ptr(), ctypes.byref(total),
                                              _stream(stream)))
    m = total.value
    return enc[:m * protection_bytes], prot[:m], first[:n + 1], status[:n]


def fill_stream(dev_u8, start, seed, stream=None):
    """Synthetic splitmix64 byte stream written on the device."""
    _dev_u8(dev_u8)
    check(lib().forst_fill_stream(dev_u8.data_ptr(), start, dev_u8.numel(), seed,
                                  _stream(stream)))
    return dev_u8


# ---- blob file records (db/blob/blob_log_format.h) ----------------------------

class BlobStatus(enum.IntEnum):
    """per-record outcome of blob_verify_batch / blob_record_crc_batch
    (FORST_BLOB_* in include/forst_checksum.h)"""
    OK = 0
    HEADER_CRC = 1
    KEY_SIZE = 2
    VALUE_SIZE = 3
    KEY = 4
    CRC = 5
    OUT_OF_RANGE = 6
    TOO_LARGE = 7


_U64 = (torch.int64, torch.uint64)
_U32 = (torch.int32, torch.uint32)


def _arr(t, what, dtypes, dev, n=None):
    """a device array handed to the engine: tensor, device, dtype, contiguity
    and (n given) at least n elements"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch tensor")
    if not t.is_cuda or t.device != dev:
        raise ValueError(f"{what} must live on {dev}, not {t.device}")
    if t.dtype not in dtypes:
        raise ValueError(f"{what} must have dtype {' or '.join(str(d) for d in dtypes)}, "
                         f"not {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    if n is not None and t.numel() < n:
        raise ValueError(f"{what} holds {t.numel()} elements, {n} needed")
    return t


def _blob_out(t, what, dtype, dev, n):
    """an optional result array: True = allocate, None / False = not wanted"""
    if t is True:
        return torch.empty(n, dtype=dtype, device=dev)
    if t is None or t is False:
        return None
    return _arr(t, what, (dtype,) if dtype == torch.uint8 else _U32, dev, n)


def blob_verify_batch(base, record_offsets, expect_key_sizes=None, expect_value_sizes=None,
                      user_keys=None, user_key_offsets=None, status=True, header_crc=True,
                      blob_crc=True, mismatches=None, stream=None):
    """BlobFileReader::VerifyBlob per record (db/blob/blob_file_reader.cc:537-579)
    over blob files resident on the device: record_offsets[i] = the start of
    record i's 32-byte header, in any order.  expect_* / user keys (one uint8
    buffer + per-record offsets, lengths = expect_key_sizes) are optional.
    Returns (status, header_crc, blob_crc, mismatches); BlobStatus codes."""
    _dev_u8(base)
    dev = base.device
    n = _arr(record_offsets, "record_offsets", _U64, dev).numel()
    for t, what in ((expect_key_sizes, "expect_key_sizes"),
                    (expect_value_sizes, "expect_value_sizes"),
                    (user_key_offsets, "user_key_offsets")):
        if t is not None:
            _arr(t, what, _U64, dev, n)
    if (user_keys is None) != (user_key_offsets is None):
        raise ValueError("user_keys and user_key_offsets go together")
    if user_keys is not None:
        _arr(user_keys, "user_keys", (torch.uint8,), dev)
        if expect_key_sizes is None:
            raise ValueError("user keys need expect_key_sizes (their lengths)")
    st = _blob_out(True if status is None else status, "status", torch.uint8, dev, n)
    hc = _blob_out(header_crc, "header_crc", torch.uint32, dev, n)
    bc = _blob_out(blob_crc, "blob_crc", torch.uint32, dev, n)
    if mismatches is None:
        mismatches = torch.zeros(1, dtype=torch.int64, device=dev)
    else:
        _arr(mismatches, "mismatches", _U64, dev, 1)
    check(lib().forst_blob_verify_batch(
        base.data_ptr(), base.numel(), record_offsets.data_ptr(), _p(expect_key_sizes),
        _p(expect_value_sizes), _p(user_keys), 0 if user_keys is None else user_keys.numel(),
        _p(user_key_offsets), st.data_ptr(), _p(hc), _p(bc), mismatches.data_ptr(), n,
        _stream(stream)))
    return st, hc, bc, mismatches


def blob_record_crc_batch(base, record_offsets, status=True, header_crc=True, blob_crc=True,
                          stream=None):
    """BlobLogRecord::EncodeHeaderTo per record (db/blob/blob_log_format.cc:96-110)
    for records laid out in a device image: fills header_crc and blob_crc in
    place.  Returns (status, header_crc, blob_crc)."""
    _dev_u8(base)
    dev = base.device
    n = _arr(record_offsets, "record_offsets", _U64, dev).numel()
    st = _blob_out(True if status is None else status, "status", torch.uint8, dev, n)
    hc = _blob_out(header_crc, "header_crc", torch.uint32, dev, n)
    bc = _blob_out(blob_crc, "blob_crc", torch.uint32, dev, n)
    check(lib().forst_blob_record_crc_batch(base.data_ptr(), base.numel(),
                                            record_offsets.data_ptr(), st.data_ptr(), _p(hc),
                                            _p(bc), n, _stream(stream)))
    return st, hc, bc
