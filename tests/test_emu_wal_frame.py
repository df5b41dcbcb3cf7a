"""forst_wal_frame_batch (forst_amd/csrc/wal_frame.h) on the CPU SIMT emulator
against the writer's image (oracle.wal_frame) and forst_wal_layout_at: the host
placement, the descriptor kernels, the flat copy with its LDS window, its
payload fast path and its byte-wise mixed pieces, and the CRC pass.  The device
twin is tests/test_gpu_wal_frame.py; the cases live in tests/walframe_cases.py.

Where a case is about reads staying inside base, base lies right in front of
an inaccessible page, so a read past its last dword ends the test."""
import ctypes
import mmap
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
import walcompact_cases as C  # noqa: E402
import walframe_cases as F  # noqa: E402


class _GuardedBuf:
    """a copy of the array whose last dword ends at an inaccessible page"""

    def __init__(self, a):
        page = mmap.PAGESIZE
        size = (a.nbytes + 3) & ~3
        total = (size + page - 1) // page * page + page
        self.m = mmap.mmap(-1, total)
        self.view = (ctypes.c_char * total).from_buffer(self.m)
        base = ctypes.addressof(self.view)
        libc = ctypes.CDLL(None, use_errno=True)
        libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        assert libc.mprotect(base + total - page, page, 0) == 0, ctypes.get_errno()
        self.ptr = base + total - page - size
        self.n = a.nbytes
        ctypes.memmove(self.ptr, a.ctypes.data, a.nbytes)

    def host(self):
        return np.frombuffer(ctypes.string_at(self.ptr, self.n), np.uint8).copy()


def guarded(a):
    return _GuardedBuf(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def run():
    # (the symbol is bound in walframe_cases.bind: emu.py has no wrapper)
    return F.runner(C.HostRunner(emu.lib()))


@pytest.mark.parametrize("recyclable", [False, True])
def test_emu_frame_length_sweep(run, recyclable):
    F.case_length_sweep(run, recyclable)


@pytest.mark.parametrize("recyclable", [False, True])
def test_emu_frame_block_edges(run, recyclable):
    F.case_block_edges(run, recyclable)


@pytest.mark.parametrize("part", ["empty", "1009", "many", "1 MiB + 1"])
def test_emu_frame_tiles_and_windows(run, part):
    F.case_tiles_and_windows(run, part)


@pytest.mark.parametrize("recyclable", [False, True])
def test_emu_frame_source_alignment_and_end(run, recyclable):
    F.case_source(run, recyclable, up_base=guarded)


@pytest.mark.parametrize("recyclable", [False, True])
def test_emu_frame_out_of_range_reps(run, recyclable):
    F.case_out_of_range(run, recyclable, up_base=guarded)


def test_emu_frame_contracts(run):
    F.case_contracts(run)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("recyclable", [False, True])
def test_emu_frame_roundtrip(run, recyclable, mode):
    F.case_roundtrip(run, recyclable, mode)


@pytest.mark.parametrize("recyclable", [False, True])
def test_emu_frame_chain(run, recyclable):
    F.case_chain(run, recyclable)


@pytest.mark.parametrize("recyclable", [False, True])
def test_emu_frame_appending(run, recyclable):
    F.case_appending(run, recyclable)
