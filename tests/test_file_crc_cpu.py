"""Whole-file CRC32C without a GPU: the committed checksums of the golden SST
files (tests/golden/file_checksums.json, written by the reference's own
FileChecksumGenCrc32c through tests/golden/gen_filecrc_golden.py) equal the
oracle's crc32c::Value, big-endian; and forst_crc32c_files validates its host
arrays before it looks for a device."""
import ctypes
import glob
import json
import os

import numpy as np

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def test_golden_file_checksums_equal_the_oracle():
    with open(os.path.join(GOLD, "file_checksums.json")) as fh:
        g = json.load(fh)
    assert g["function"] == "FileChecksumCrc32c"
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "sst", "*.sst")))
    assert names == sorted(g["files"]) and len(names) >= 20
    for name in names:
        with open(os.path.join(GOLD, "sst", name), "rb") as fh:
            f = fh.read()
        e = g["files"][name]
        assert e["size"] == len(f)
        # FileChecksumGenCrc32c::Finalize: PutFixed32(EndianSwapValue(crc))
        assert e["checksum"] == O.crc32c_value(f).to_bytes(4, "big").hex().upper(), name
    assert len({e["checksum"] for e in g["files"].values()}) == len(names)


def test_crc32c_files_checks_its_arguments_before_any_device_call():
    from forst_amd import _lib
    L = _lib.lib()
    offs = np.array([0, 90], np.uint64)
    lens = np.array([10, 11], np.uint64)
    out = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused or a no-op
    arena = ctypes.c_void_p(0x2000)
    assert L.forst_crc32c_files(None, 0, None, None, None, None, 0, None) == 0
    assert L.forst_crc32c_files(arena, 100, offs.ctypes.data, lens.ctypes.data, None, out, 2,
                                None) == -1
    assert b"file 1 [90, +11) outside the arena of 100 bytes" in L.forst_last_error()
    assert L.forst_crc32c_files(arena, 100, None, lens.ctypes.data, None, out, 2, None) == -1
    assert L.forst_crc32c_files(arena, 100, offs.ctypes.data, lens.ctypes.data, None, None, 2,
                                None) == -1
    lens[1] = 2**64 - 1
    assert L.forst_crc32c_files(arena, 100, offs.ctypes.data, lens.ctypes.data, None, out, 2,
                                None) == -1


def test_file_checksum_string_is_big_endian():
    from forst_amd import sst
    assert sst.file_checksum_string(0x0A1B2C3D) == b"\x0a\x1b\x2c\x3d"
