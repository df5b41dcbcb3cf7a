"""Shapes shared by the whole-file CRC32C tests (tests/test_emu_file_crc.py on
the SIMT emulator, tests/test_gpu_file_crc.py on the device): file layouts in
one arena that put the segmented fold of forst_crc32c_files at its wave and
file boundaries."""
import numpy as np

CHUNK = 65536


def layout(lengths, first=1, gap=3):
    """files of the given lengths at odd offsets with gaps between them ->
    (offsets u64, lengths u64, arena bytes needed)"""
    offs, at = [], first
    for n in lengths:
        at |= 1
        offs.append(at)
        at += n + gap
    return np.array(offs, np.uint64), np.array(lengths, np.uint64), at


# 0 / 1 / 3 bytes, one chunk +-1, two whole chunks; empty files first, between
# and last (their result is the init alone and no lane ever finds them)
EDGE_LENGTHS = [0, 0, 1, 3, CHUNK - 1, 0, CHUNK, CHUNK + 1, 2 * CHUNK, 0]

# 70 one-chunk files then one of 65 chunks + 1 byte: waves that hold many
# files, a wave that starts inside a file, a file longer than a wave
MANY_THEN_LONG = [1 + 37 * k for k in range(70)] + [65 * CHUNK + 1]


def expect(O, arena, offs, lens, inits=None):
    return np.array([O.crc32c_extend(0 if inits is None else int(inits[i]),
                                     arena[int(o):int(o) + int(n)].tobytes())
                     for i, (o, n) in enumerate(zip(offs, lens))], np.uint32)
