"""forst_crc32c_files (whole-file CRC32C of a set of files in one call) on the
CPU SIMT emulator vs the oracle: the chunk -> file search, the segmented XOR
reduction inside a wave and the init term, at the layouts where files and waves
meet.  The device twin is tests/test_gpu_file_crc.py."""
import ctypes
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
import filecrc_cases as C  # noqa: E402

from oracle import oracle as O  # noqa: E402

FORST_EINVAL = -1


def files(arena, offs, lens, inits=None, arena_len=None, misalign=0):
    """forst_crc32c_files on emu.lib() (bound here: emu.py has no wrapper)
    -> (return code, out)"""
    L = emu.lib()
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.forst_crc32c_files.restype = ctypes.c_int
    L.forst_crc32c_files.argtypes = [vp, u64, vp, vp, vp, vp, u64, vp]
    raw = np.zeros(arena.nbytes + 64, np.uint8)
    at = (-raw.ctypes.data) % 16 + misalign
    a = raw[at:at + arena.nbytes]
    a[:] = arena
    offs = np.ascontiguousarray(offs, np.uint64)
    lens = np.ascontiguousarray(lens, np.uint64)
    ini = None if inits is None else np.ascontiguousarray(inits, np.uint32)
    out = np.full(len(offs) + 2, 0xA5A5A5A5, np.uint32)  # stale values, two guard slots
    rc = L.forst_crc32c_files(a.ctypes.data, arena.nbytes if arena_len is None else arena_len,
                              offs.ctypes.data, lens.ctypes.data,
                              None if ini is None else ini.ctypes.data, out.ctypes.data,
                              len(offs), None)
    assert (out[len(offs):] == 0xA5A5A5A5).all()
    return rc, out[:len(offs)]


@pytest.fixture(scope="module")
def arena():
    return np.random.default_rng(2024).integers(0, 256, 5 * 1024 * 1024 + 4099, dtype=np.uint8)


@pytest.mark.parametrize("with_inits", [False, True])
@pytest.mark.parametrize("lengths", [C.EDGE_LENGTHS, C.MANY_THEN_LONG], ids=["edges", "many_then_long"])
def test_emu_files_vs_oracle(arena, lengths, with_inits):
    offs, lens, need = C.layout(lengths)
    assert need <= arena.nbytes
    inits = None
    if with_inits:
        inits = np.random.default_rng(5).integers(0, 2**32, len(offs), dtype=np.uint64).astype(np.uint32)
    rc, out = files(arena, offs, lens, inits)
    assert rc == 0
    assert (out == C.expect(O, arena, offs, lens, inits)).all()


def test_emu_files_small_sets(arena):
    # no file: nothing is touched; one file; two files over the same bytes; a
    # file that ends exactly at arena_len; an arena at an odd address
    rc, out = files(arena, [], [])
    assert rc == 0 and len(out) == 0
    n = arena.nbytes
    for offs, lens, inits in (([7], [C.CHUNK + 9], None),
                              ([5, 5], [3 * C.CHUNK + 1, 3 * C.CHUNK + 1], [0, 0x89ABCDEF]),
                              ([11, n - 70001], [12, 70001], [1, 2]),
                              ([n], [0], [0x1234])):
        for mis in (0, 1):
            rc, out = files(arena, offs, lens, inits, misalign=mis)
            assert rc == 0
            assert (out == C.expect(O, arena, offs, lens, inits)).all(), (offs, lens, mis)


def test_emu_files_range_check(arena):
    n = arena.nbytes
    for offs, lens in (([n - 10], [11]), ([0, n + 1], [1, 0]), ([3], [2**64 - 2])):
        rc, out = files(arena, offs, lens)
        assert rc == FORST_EINVAL
        assert (out == 0xA5A5A5A5).all()  # refused before any launch
        assert b"outside the arena" in emu.lib().forst_last_error()
