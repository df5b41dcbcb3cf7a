"""forst_crc32c_files on the MI355X: the whole-file CRC32C of a set of files in
one call (FileChecksumGenCrc32c, util/file_checksum_helper.h:22-48, as
DB::VerifyFileChecksums runs it per live file) vs the oracle -- the emulator's
layouts (tests/test_emu_file_crc.py), a file across the fold's 256-thread
workgroup, 1000 small files, a file past 4 GiB, the output contract, and the
golden SST files against the reference's own checksums
(tests/golden/file_checksums.json) with DBImpl::VerifyFullFileChecksum's
Status text."""
import glob
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import contracts as K  # noqa: E402  (read-only: the sentinels and `untouched`)
import filecrc_cases as C  # noqa: E402
from forst_amd import ForstError, engine, sst  # noqa: E402
from oracle import oracle as O  # noqa: E402

DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def u32(t):
    return t.cpu().view(torch.int32).numpy().view(np.uint32)


@pytest.fixture(scope="module")
def arena():
    """(host bytes, the same on the device at a 16-byte aligned address, and
    shifted by one byte): 17 MiB of random bytes, shared and never written"""
    hb = np.random.default_rng(2025).integers(0, 256, 17 * 1024 * 1024 + 4099, dtype=np.uint8)
    raw = torch.empty(len(hb) + 256, dtype=torch.uint8, device=DEV)
    a0, a1 = raw[:len(hb)], raw[1:1 + len(hb)]
    return hb, a0, a1, torch.from_numpy(hb)


def run(arena, which, offs, lens, inits=None):
    hb, a0, a1, src = arena
    a = (a0, a1)[which]
    a.copy_(src)
    return u32(engine.crc32c_files(a, offs, lens, inits))


@pytest.mark.parametrize("with_inits", [False, True])
@pytest.mark.parametrize("lengths", [C.EDGE_LENGTHS, C.MANY_THEN_LONG,
                                     [5, 257 * C.CHUNK + 1, 9]],
                         ids=["edges", "many_then_long", "across_a_workgroup"])
def test_files_vs_oracle(arena, lengths, with_inits):
    offs, lens, need = C.layout(lengths)
    assert need <= len(arena[0])
    inits = None
    if with_inits:
        inits = np.random.default_rng(5).integers(0, 2**32, len(offs), dtype=np.uint64).astype(np.uint32)
    want = C.expect(O, arena[0], offs, lens, inits)
    for which in (0, 1):  # the arena at an aligned and at an odd address
        assert (run(arena, which, offs, lens, inits) == want).all(), which
    assert engine.last_kernel() == "files_fold_kernel"


def test_small_sets(arena):
    hb = arena[0]
    n = len(hb)
    assert len(run(arena, 0, [], [])) == 0
    for offs, lens, inits in (([7], [C.CHUNK + 9], None),
                              ([5, 5], [3 * C.CHUNK + 1, 3 * C.CHUNK + 1], [0, 0x89ABCDEF]),
                              ([11, n - 70001], [12, 70001], [1, 2]),
                              ([n], [0], [0x1234]),
                              ([0, 9, 9], [0, 0, 0], [7, 8, 9])):
        assert (run(arena, 0, offs, lens, inits) == C.expect(O, hb, offs, lens, inits)).all(), offs


def test_thousand_small_files(arena):
    hb = arena[0]
    rng = np.random.default_rng(77)
    lens = rng.integers(1, 3 * C.CHUNK + 1, 1000)
    lens[::97] = 0
    lens[1::101] = C.CHUNK
    lens[2::103] = 2 * C.CHUNK
    # files overlap freely (the arena is read-only): random odd starts
    offs = rng.integers(0, len(hb) - 3 * C.CHUNK, 1000) | 1
    inits = rng.integers(0, 2**32, 1000, dtype=np.uint64).astype(np.uint32)
    want = C.expect(O, hb, offs, lens, inits)
    assert (run(arena, 0, offs, lens, inits) == want).all()


def test_range_check_refuses_before_any_launch(arena):
    hb, a0 = arena[0], arena[1]
    n = len(hb)
    out = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    for offs, lens in (([n - 10], [11]), ([0, n + 1], [1, 0]), ([3], [2**64 - 2])):
        with pytest.raises(ForstError) as e:
            engine.crc32c_files(a0, offs, lens, out=out.view(torch.uint32))
        assert e.value.code == -1 and "outside the arena" in str(e.value)
    assert (out.cpu().numpy() == 0x5A5A5A5A).all()


def test_file_past_4gib():
    """one file of 4 GiB + 65537 bytes between two small ones: chunk offsets
    and the bytes-after shifts need all 64 bits"""
    n = (1 << 32) + 65537
    dev = torch.empty(n + 64 + 256, dtype=torch.uint8, device=DEV)
    engine.fill_stream(dev, 0, 0xF11E)
    half = 1 << 31
    big = dev[8:8 + n]
    c1 = int(u32(engine.crc32c_buffer(big[:half], 0x0BADCAFE))[0])
    c2 = int(u32(engine.crc32c_buffer(big[half:]))[0])
    want_big = O.crc32c_combine(c1, c2, n - half)
    offs, lens, inits = [1, 8, 8 + n + 3], [5, n, 40], [3, 0x0BADCAFE, 9]
    got = u32(engine.crc32c_files(dev, offs, lens, inits))
    head, tail = dev[:8].cpu().numpy(), dev[8 + n + 3:8 + n + 43].cpu().numpy()
    assert got[0] == O.crc32c_extend(3, head[1:6].tobytes())
    assert got[1] == want_big
    assert got[2] == O.crc32c_extend(9, tail.tobytes())


def test_output_contract(arena):
    """nothing stored past n_files or into the arena; a second call into the
    same `out` overwrites (no XOR into stale values); the same results on a
    non-default stream"""
    hb, a0, _, src = arena
    a0.copy_(src)
    offs, lens, _ = C.layout(C.EDGE_LENGTHS + [4 * C.CHUNK + 7] + [1 + 37 * k for k in range(70)])
    n = len(offs)
    rng = np.random.default_rng(9)
    ini_a = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    want_a = C.expect(O, hb, offs, lens, ini_a)
    want_0 = C.expect(O, hb, offs, lens)
    out = torch.full((n + K.GUARD,), K.S32 - (1 << 32) if K.S32 >= 1 << 31 else K.S32,
                     dtype=torch.int32, device=DEV)
    o32 = out.view(torch.uint32)
    engine.crc32c_files(a0, offs, lens, ini_a, out=o32)
    got = u32(o32)
    assert (got[:n] == want_a).all()
    K.untouched(got, n, 4, "crc32c_files out")
    engine.crc32c_files(a0, offs, lens, out=o32)  # over the stale results
    got = u32(o32)
    assert (got[:n] == want_0).all()
    K.untouched(got, n, 4, "crc32c_files out, second call")
    assert (a0.cpu().numpy() == hb).all()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        r = engine.crc32c_files(a0, offs, lens, ini_a, stream=s)
    s.synchronize()
    assert (u32(r) == want_a).all()


def test_golden_ssts_and_verify_status_text():
    """every golden SST packed into one arena gives the reference's recorded
    checksums; verify_file_checksums gives DBImpl::VerifyFullFileChecksum's
    Status (db/db_impl/db_impl.cc:6373-6402) per file"""
    with open(os.path.join(GOLD, "file_checksums.json")) as fh:
        sums = json.load(fh)["files"]
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "sst", "*.sst")))
    assert names == sorted(sums)
    files = [open(os.path.join(GOLD, "sst", x), "rb").read() for x in names]
    crcs = sst.file_checksums(files, align=1)  # packed: odd starts
    strs = [sst.file_checksum_string(c) for c in crcs]
    assert [s.hex().upper() for s in strs] == [sums[x]["checksum"] for x in names]
    assert [len(f) for f in files] == [sums[x]["size"] for x in names]
    paths = ["/db/" + x for x in names]
    expected = list(strs)
    expected[1] = expected[1][:3] + bytes([expected[1][3] ^ 1])  # last byte flipped
    expected[2] = b""  # kUnknownFileChecksum: not checked
    bad = bytearray(files[3])
    bad[len(bad) // 2] ^= 0x10  # a data byte flipped
    bad[4] ^= 0x01
    bad_crc = sst.file_checksum_string(O.crc32c_value(bytes(bad)))
    staged = list(files)
    staged[2] = bytes(len(files[2]))  # never read: its expectation is empty
    staged[3] = bytes(bad)
    got = sst.verify_file_checksums(expected, staged, file_names=paths)
    want = ["OK"] * len(names)
    want[1] = (f"Corruption: {paths[1]} file checksum mismatch, expecting "
               f"{expected[1].hex().upper()}, but actual {strs[1].hex().upper()}")
    want[3] = (f"Corruption: {paths[3]} file checksum mismatch, expecting "
               f"{strs[3].hex().upper()}, but actual {bad_crc.hex().upper()}")
    assert got == want
    assert want[1].endswith(f"expecting {sums[names[1]]['checksum'][:6]}"
                            f"{int(sums[names[1]]['checksum'][6:], 16) ^ 1:02X}, "
                            f"but actual {sums[names[1]]['checksum']}")
