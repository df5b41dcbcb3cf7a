"""The C++ host shim's device-side record join on the GPU
(tests/cpp/wal_compact_selftest.cc): forst_gpu::WalRecovery::CompactRecords
equals the bytes Next() hands out, record for record, and
KvProtection::WriteBatchProtectionDevice on the compacted records equals
WriteBatchProtection on the host bytes -- the first on WriteBatch reps framed
as WAL records, the fragment-count logs, a control record between fragments
and records of about 1 MiB, the second on the WriteBatch reps."""
import os
import subprocess
import sys

import pytest

import forst_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _build(tmp_path):
    libdir = os.path.dirname(forst_amd.LIB_PATH)
    exe = str(tmp_path / "wal_compact_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "cpp", "wal_compact_selftest.cc"), "-o", exe,
                           f"-L{libdir}", "-lforst_checksum", "-L/opt/rocm/lib", "-lamdhip64",
                           f"-Wl,-rpath,{libdir}:/opt/rocm/lib", "-lpthread"])
    return exe


@pytest.mark.parametrize("recyclable", [False, True])
def test_shim_compact_records_and_device_protection(tmp_path, recyclable):
    import walcases as W
    import walcompact_cases as C
    logs = [("chain", C.chain_log(recyclable)[0], 7, 2), ("big", C.big_record_log(recyclable), 7, 2)]
    logs += [(n, log, ln, 2) for n, log, ln in C.layout_logs(recyclable)]
    logs += [(n, log, ln, m) for n, log, ln in W.stop_and_fragment_cases(recyclable)
             if n in ("frags", "frags_x") for m in (0, 3)]
    logs += [(n, log[:12 * 32768 + 500], ln, 2) for n, log, ln in W.control_scenarios(recyclable, 43)
             if n == "ctl_frag"]
    exe = _build(tmp_path)
    args, want = [], []
    for i, (name, log, ln, mode) in enumerate(logs):
        path = str(tmp_path / f"{i:03d}.log")
        with open(path, "wb") as f:
            f.write(bytes(log))
        args += [path, str(ln), str(mode), "1" if name == "chain" else "0"]
        recs = C.reader_records(log, ln, mode)
        want.append("case %s %d %d" % (path, len(recs), sum((len(r[1]) + 15) // 16 * 16 for r in recs)))
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("case ")] == want
