"""The host walk of forst_blob_verify_files (forst_amd/csrc/blob_host.cc) as a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/cpp/blob_walk_selftest.cc is compiled together with blob_host.cc by g++
-fsanitize=address,undefined and run directly over the fixture files, their
damaged copies, every truncation length of one file, crafted files and seeded
random bytes.  Each case lives in a heap block of exactly its size, so a read
outside the file is a sanitizer report; the printed walks are compared with
the restatement (tests/blobfile.py)."""
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

if shutil.which("g++") is None:
    pytest.skip("needs g++", allow_module_level=True)

import blobcases as C  # noqa: E402
import blobfile as B  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")


def corpus():
    meta = json.load(open(os.path.join(GOLDEN, "blob_files.json")))
    read = lambda n: open(os.path.join(GOLDEN, "blob", n), "rb").read()  # noqa: E731
    cases = [(read(n), m["column_family_id"]) for n, m in meta["files"].items()]
    cases += [(read(n), None) for n in meta["files"]]
    cases += [(B.apply_damage(read(d["file"]), d), meta["files"][d["file"]]["column_family_id"])
              for d in meta["damaged"]]
    cases += [(f, cf) for _, f, cf in C.damaged_files()]
    one = read("w_expiration.blob")
    cases += [(one[:n], 9) for n in range(len(one) + 1)]             # every truncation length
    cases += [(one[:n] + one[-32:], 9) for n in range(30, len(one) - 32)]  # ... with a sound footer
    rng = np.random.default_rng(0xB10B5EED)
    for i in range(300):
        raw = bytearray(rng.integers(0, 256, int(rng.integers(0, 700)), dtype=np.uint8).tobytes())
        if i % 3 and len(raw) >= 62:  # sound header and footer magic: the record walk runs on noise
            raw[:30] = B.file_header(cf=9)
            raw[-32:] = B.file_footer(int(rng.integers(0, 5)))
            if i % 3 == 2:  # ... on small sizes: many steps
                for p in range(30, len(raw) - 32, 8):
                    raw[p:p + 8] = struct.pack("<Q", int(rng.integers(0, 40)))
        cases.append((bytes(raw), 9 if i % 2 else None))
    return cases


def test_blob_walk_under_sanitizers(tmp_path):
    exe = str(tmp_path / "blob_walk_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           f"-I{ROOT}/include", os.path.join(HERE, "cpp", "blob_walk_selftest.cc"),
                           os.path.join(ROOT, "forst_amd", "csrc", "blob_host.cc"), "-o", exe])
    cases = corpus()
    path = str(tmp_path / "corpus.bin")
    with open(path, "wb") as fh:
        for data, cf in cases:
            fh.write(struct.pack("<QII", len(data), cf is not None, cf or 0) + data)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases) and len(cases) > 3000
    reasons = set()
    for (data, cf), line in zip(cases, lines):
        w = B.walk_file(data, cf)
        offs = w["offsets"]
        host_failed = w["reason"] != B.F_OK
        exp = (w["reason"], len(offs), int(w["tail_crosses"]),
               0 if host_failed else len(offs) - int(w["tail_crosses"]),
               w["total_blob_bytes"], w["cf"], sum(o * (k + 1) for k, o in enumerate(offs)) % 2**64)
        assert tuple(int(x) for x in line.split()) == exp, (len(data), cf, line, exp)
        reasons.add(w["reason"])
    assert reasons == {B.F_OK, B.F_MALFORMED, B.F_HEADER_MAGIC, B.F_HEADER_VERSION, B.F_TTL,
                       B.F_CF_MISMATCH, B.F_FOOTER_MAGIC}
