"""Blob files (db/blob/): the whole-file scan over the HIP engine.

blob_verify_files is BlobFileReader::Create's checks (blob_file_reader.cc:28-77)
followed by every record as BlobLogSequentialReader::ReadRecord checks it
(blob_log_sequential_reader.cc:64-114), for a set of files in one call: the
structure is walked on the host, every CRC (record headers, payloads, footers)
is computed on the device in one verify batch.  The per-record calls are
engine.blob_verify_batch and engine.blob_record_crc_batch.
"""
import ctypes
import enum

import numpy as np
import torch

from ._lib import check, lib
from .engine import _arr, _dev_u8, _stream


class BlobFileReason(enum.IntEnum):
    """enum forst_blob_file_reason (include/forst_checksum.h)"""
    OK = 0
    MALFORMED = 1
    HEADER_MAGIC = 2
    HEADER_VERSION = 3
    TTL = 4
    CF_MISMATCH = 5
    FOOTER_MAGIC = 6
    FOOTER_CRC = 7
    RECORD_HEADER_CRC = 8
    RECORD_BLOB_CRC = 9
    RECORD_CROSSES_FOOTER = 10
    BLOB_COUNT_MISMATCH = 11
    RECORD_TOO_LARGE = 12


class BlobFileResult(ctypes.Structure):
    """forst_blob_file_result"""
    _fields_ = [("status", ctypes.c_int32), ("reason", ctypes.c_int32),
                ("fail_index", ctypes.c_uint64), ("fail_offset", ctypes.c_uint64),
                ("blob_count", ctypes.c_uint64), ("total_blob_bytes", ctypes.c_uint64),
                ("column_family_id", ctypes.c_uint32), ("compression", ctypes.c_uint8),
                ("has_ttl", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 2)]

    @property
    def text(self):
        """Status::ToString()"""
        return reason_text(self.reason)


def reason_text(reason):
    return lib().forst_blob_file_reason_text(int(reason)).decode()


def _host_files(files):
    """-> (keepalive arrays, pointer array, sizes)"""
    keep = [np.frombuffer(f, np.uint8) if isinstance(f, (bytes, bytearray, memoryview))
            else np.ascontiguousarray(f, np.uint8) for f in files]
    ptrs = (ctypes.c_void_p * len(keep))(*[a.ctypes.data if a.size else None for a in keep])
    sizes = np.array([a.size for a in keep], np.uint64)
    return keep, ptrs, sizes


def blob_walk_file(data, expect_cf_id=None):
    """forst_blob_walk_file (no GPU call): -> (result, record offsets,
    tail_crosses)"""
    keep, _, sizes = _host_files([data])
    n, tail, res = ctypes.c_uint64(), ctypes.c_int(), BlobFileResult()
    cf = None if expect_cf_id is None else ctypes.pointer(ctypes.c_uint32(expect_cf_id))
    cap = max(1, int(sizes[0]) // 32)
    offs = np.zeros(cap, np.uint64)
    check(lib().forst_blob_walk_file(keep[0].ctypes.data if keep[0].size else None, int(sizes[0]),
                                     None if cf is None else ctypes.cast(cf, ctypes.c_void_p),
                                     offs.ctypes.data, cap, ctypes.byref(n), ctypes.byref(tail),
                                     ctypes.byref(res)))
    return res, offs[:n.value], bool(tail.value)


def blob_verify_files(files, dev_arena, dev_offsets, expect_cf_ids=None, stream=None):
    """files: the files' bytes in host memory (bytes / uint8 arrays); dev_arena:
    a device uint8 tensor that holds file i's bytes at dev_offsets[i].
    -> list of BlobFileResult, one per file.  Synchronous."""
    n = len(files)
    if len(dev_offsets) != n or (expect_cf_ids is not None and len(expect_cf_ids) != n):
        raise ValueError("one dev_offsets / expect_cf_ids entry per file")
    if n == 0:
        return []
    _dev_u8(dev_arena)
    _arr(dev_arena, "dev_arena", (torch.uint8,), dev_arena.device)
    keep, ptrs, sizes = _host_files(files)
    offs = np.ascontiguousarray(dev_offsets, np.uint64)
    cfs = None if expect_cf_ids is None else np.ascontiguousarray(expect_cf_ids, np.uint32)
    out = (BlobFileResult * n)()
    check(lib().forst_blob_verify_files(
        ctypes.cast(ptrs, ctypes.c_void_p), sizes.ctypes.data, offs.ctypes.data,
        dev_arena.data_ptr(), dev_arena.numel(), None if cfs is None else cfs.ctypes.data, n,
        ctypes.cast(out, ctypes.c_void_p), _stream(stream)))
    return list(out)
