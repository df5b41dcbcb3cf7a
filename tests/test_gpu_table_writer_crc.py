"""The table writer's running file checksum and per-append handoff CRC
(GpuTrailerWriter Options::file_checksum / SinkWithCrc, table_writer.cc):
every reference-written SST re-emitted block by block with both on.  The
bytes must be the file's, every sink call's CRC crc32c::Value of exactly that
call's bytes (what WritableFileWriter::Append takes as crc32c_checksum), and
the final checksum the reference's own FileChecksumGenCrc32c value
(tests/golden/file_checksums.json)."""
import glob
import json
import os
import struct

import numpy as np
import pytest

import sstwalk
from oracle import oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
FILES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "sst", "*.sst")))
with open(os.path.join(GOLD, "file_checksums.json")) as fh:
    SUMS = json.load(fh)["files"]


def read(name):
    with open(os.path.join(GOLD, "sst", name), "rb") as fh:
        return fh.read()


def emit(tr, f, blocks, foot=None):
    for kind, off, n, t in blocks:
        assert tr.add(f[off:off + n], t, is_data_block=(kind == "data")) == (off, n)
    if foot is not None:
        tr.footer(foot["fv"], foot["metaindex"], foot["index"] or (0, 0))
    else:
        tr.flush()


def check_pieces(tr, out):
    """every sink call carried crc32c::Value of its own bytes, and the calls
    tile the output"""
    pos = 0
    for at, n, crc in tr.pieces:
        assert at == pos and n > 0
        assert crc == O.crc32c_value(bytes(out[at:at + n])), (at, n)
        pos += n
    assert pos == len(out)


def test_fixture_covers_every_sst():
    assert sorted(SUMS) == FILES and len(FILES) >= 20


@pytest.mark.parametrize("window", [4096, 1 << 20, 0])
@pytest.mark.parametrize("name", FILES)
def test_rewrite_with_file_checksum_and_crc_sink(name, window):
    from forst_amd import table_writer as tw
    f = read(name)
    blocks, foot = sstwalk.walk(f)
    tr = tw.TrailerWriter(foot["checksum"], foot["bcc"], window_bytes=window,
                          file_checksum=True, crc_sink=True)
    emit(tr, f, blocks, foot)
    crc, s = tr.file_checksum, tr.file_checksum_string
    out = tr.close()
    assert out == f
    check_pieces(tr, out)
    if window == 4096:  # many windows; blocks larger than the window get their own
        assert len(tr.pieces) > 3
    assert s.hex().upper() == SUMS[name]["checksum"] and len(f) == SUMS[name]["size"]
    assert crc == int.from_bytes(s, "big") == O.crc32c_value(f)


@pytest.mark.parametrize("name", [FILES[0], FILES[len(FILES) // 2], FILES[-1]])
def test_options_off_keep_the_sink_sequence(name):
    """neither option: the same sink calls (count, lengths, bytes) as with
    them, through the plain sink; and each option alone works"""
    from forst_amd import table_writer as tw
    f = read(name)
    blocks, foot = sstwalk.walk(f)
    runs = {}
    for key, kw in (("off", {}), ("sum", {"file_checksum": True}), ("sink", {"crc_sink": True}),
                    ("both", {"file_checksum": True, "crc_sink": True})):
        tr = tw.TrailerWriter(foot["checksum"], foot["bcc"], window_bytes=8192, **kw)
        emit(tr, f, blocks, foot)
        crc = tr.file_checksum
        assert tr.close() == f
        runs[key] = (tr, crc)
    want = [(a, n) for a, n, _ in runs["off"][0].pieces]
    assert len(want) > 3
    for key, (tr, crc) in runs.items():
        assert [(a, n) for a, n, _ in tr.pieces] == want, key
        assert all((c is None) == (key in ("off", "sum")) for _, _, c in tr.pieces)
        assert crc == (O.crc32c_value(f) if key in ("sum", "both") else 0), key
    check_pieces(runs["sink"][0], f)


@pytest.mark.parametrize("name", [FILES[1], FILES[-2]])
def test_split_file_two_writers(name):
    """the file written by two writers, the second starting at the first's
    offset with the first's checksum as file_checksum_init"""
    from forst_amd import table_writer as tw
    f = read(name)
    blocks, foot = sstwalk.walk(f)
    k = len(blocks) // 2
    a = tw.TrailerWriter(foot["checksum"], foot["bcc"], window_bytes=4096, file_checksum=True,
                         crc_sink=True)
    emit(a, f, blocks[:k])
    mid, crc_a = a.offset, a.file_checksum
    out_a = a.close()
    assert mid == blocks[k][1] and crc_a == O.crc32c_value(f[:mid])
    b = tw.TrailerWriter(foot["checksum"], foot["bcc"], start_offset=mid, window_bytes=4096,
                         file_checksum=crc_a, crc_sink=True)
    emit(b, f, blocks[k:], foot)
    s = b.file_checksum_string
    out_b = b.close()
    assert out_a + out_b == f
    check_pieces(a, out_a)
    check_pieces(b, out_b)
    assert s.hex().upper() == SUMS[name]["checksum"]


def test_block_align_padding_is_covered():
    """block_align pads data blocks with zeros inside the window: the pad
    bytes are part of the handoff CRCs and of the file checksum"""
    from forst_amd import table_writer as tw
    rng = np.random.default_rng(18)
    n = 300
    sizes = rng.integers(0, 9000, n)
    sizes[:5] = [0, 1, 4091, 4092, 70000]
    types = rng.integers(0, 8, n).astype(np.uint8)
    bcc = 0x9E3779B1
    tr = tw.TrailerWriter(4, bcc, block_align=4096, window_bytes=1 << 16, file_checksum=0xCAFEF00D,
                          crc_sink=True)
    want = bytearray()
    for i in range(n):
        blk = rng.integers(0, 256, int(sizes[i]), np.uint8).tobytes()
        off = len(want)
        assert tr.add(blk, int(types[i]), is_data_block=(i % 7 != 0)) == (off, len(blk))
        c = O.compute_builtin_checksum_with_last_byte(4, blk, int(types[i]))
        c = (c + O.checksum_modifier_for_context(bcc, off)) & 0xFFFFFFFF
        want += blk + bytes([int(types[i])]) + struct.pack("<I", c)
        if i % 7 != 0:
            want += bytes((4096 - ((len(blk) + 5) & 4095)) & 4095)
    tr.flush()
    crc = tr.file_checksum
    out = tr.close()
    assert out == bytes(want)
    check_pieces(tr, out)
    assert len(tr.pieces) > 10
    assert crc == O.crc32c_extend(0xCAFEF00D, bytes(want))


def test_setters_refused_after_the_first_block():
    import ctypes

    from forst_amd import ForstError
    from forst_amd import table_writer as tw
    from forst_amd._lib import lib
    tr = tw.TrailerWriter(1)
    tr.add(b"abc")
    assert lib().forst_trailer_writer_enable_file_checksum(tr._h, 0) == -1
    cb = tw.SINK_CRC(lambda *a: 0)
    assert lib().forst_trailer_writer_set_crc_sink(tr._h, ctypes.cast(cb, ctypes.c_void_p),
                                                   None) == -1
    assert len(tr.close()) == 8
    with pytest.raises(ForstError):
        tw.TrailerWriter(1, block_align=3)
