#!/usr/bin/env python3
"""tests/golden/gen_filecrc_golden.py -- TEST INFRASTRUCTURE ONLY: the
whole-file checksum of every committed SST fixture, by the REFERENCE's own
FileChecksumGenCrc32c (util/file_checksum_helper.h:22-48).

The veneer tests/golden/ref_filecrc_shim.cc is linked against the reference
archive of tests/golden/refbuild.py (compiled outside the committed tree) and
run over tests/golden/sst/*.sst: Update in two uneven pieces, Finalize,
GetChecksum.  Only data is written: tests/golden/file_checksums.json maps each
file name to its size and the hex of the 4-byte checksum string (what
FileMetaData::file_checksum holds and DB::VerifyFileChecksums compares).

Re-run:  python tests/golden/gen_filecrc_golden.py   (needs the reference + g++)
"""
import ctypes
import glob
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refbuild  # noqa: E402


def main():
    tmp = tempfile.mkdtemp(prefix="forst_ref_filecrc_")
    try:
        so = refbuild.link_veneer([os.path.join(HERE, "ref_filecrc_shim.cc")],
                                  os.path.join(tmp, "libref_filecrc.so"))
        L = ctypes.CDLL(so)
        L.ref_file_checksum_crc32c.restype = ctypes.c_int
        L.ref_file_checksum_crc32c.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t,
                                               ctypes.c_char_p]
        files = {}
        for path in sorted(glob.glob(os.path.join(HERE, "sst", "*.sst"))):
            data = open(path, "rb").read()
            out = ctypes.create_string_buffer(4)
            rc = L.ref_file_checksum_crc32c(data, len(data), len(data) // 3 + 1, out)
            assert rc == 0, (path, rc)
            files[os.path.basename(path)] = {"size": len(data), "checksum": out.raw.hex().upper()}
        with open(os.path.join(HERE, "file_checksums.json"), "w") as fh:
            json.dump({"generator": "tests/golden/gen_filecrc_golden.py (FileChecksumGenCrc32c, "
                                    "util/file_checksum_helper.h:22)",
                       "function": "FileChecksumCrc32c", "files": files}, fh, indent=1)
        print(f"{len(files)} files")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
