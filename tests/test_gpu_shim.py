"""The C++ host shim (namespace forst_gpu) end to end on the GPU: write trailers,
verify clean, detect a corrupted block with the reference's exact
Corruption message (reader_common.cc:55-60)."""
import os
import subprocess

import pytest

import forst_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    libdir = os.path.dirname(forst_amd.LIB_PATH)
    exe = str(tmp_path / "shim_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "cpp", "shim_selftest.cc"), "-o", exe,
                           f"-L{libdir}", "-lforst_checksum", "-L/opt/rocm/lib", "-lamdhip64",
                           f"-Wl,-rpath,{libdir}:/opt/rocm/lib", "-lpthread"])
    return exe


def test_forstdb_shim_on_gpu(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr


def test_concurrent_host_threads_share_the_engine(tmp_path):
    """The header's reentrancy promise (forst_checksum.h conventions): 4 host
    threads, each on its own non-blocking HIP stream, interleave write-side
    trailers, verify, WAL writer CRC, WAL verify and raw XXH3 batches for 12
    rounds against the shared per-device scratch pool; every result equals the
    single-threaded run."""
    exe = _build(tmp_path)
    r = subprocess.run([exe, "threads"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PASS" in r.stdout and "failures 0" in r.stdout, \
        r.stdout + r.stderr


def expected_transcript(log, log_number, mode):
    """the transcript `shim_selftest walfile` prints, from the serial reader
    (oracle/wal_reader.py read_all_ex): every Corruption call in front of the
    record whose ReadRecord call made it, every record with the XXH3 of its
    bytes, the trailing calls, an OK status and the stop fields"""
    from oracle import wal_reader as R
    x = R.read_all_ex(log, log_number, mode)
    lines, seen = [], 0
    reps = x["reports"]
    for (off, n, h, nf), fresh, upto in zip(x["records"], x["payload_xxh3"], x["reports_before"]):
        lines += ["C %d %d %s" % (p, b, why) for b, why, p in reps[seen:upto]]
        lines.append("R %d %d %d %016x %016x %d" % (off, n, nf, h, fresh, upto - seen))
        seen = upto
    lines += ["C %d %d %s" % (p, b, why) for b, why, p in reps[seen:]]
    lines.append("S OK")
    lines.append("E %d %d %d %d %d" % (x["stop_offset"], x["stop_reason"], len(x["records"]),
                                       len(reps), R.n_physical(log, log_number, mode)))
    return "".join(line + "\n" for line in lines)


def shim_replay_logs(recyclable):
    """(name, log, log number): the small stop / fragment-count / tiny logs, and
    cuts of the scenario logs that hold control records between fragments,
    long control runs, CRC faults, re-typed fragments, an old record before a
    corrupt tail, a zero-filled region and a truncated (recyclable) header"""
    import walcases as W
    logs = list(W.stop_and_fragment_cases(recyclable))
    logs += [(n, log[:12 * 32768 + 500], ln) for n, log, ln in W.control_scenarios(recyclable, 43)
             if n == "ctl_frag"]
    logs += W.long_control_runs(recyclable)
    for n, log, ln in W.scenarios(recyclable, 23, n=300):
        if n in ("crc", "retype", "old+crc", "zero"):
            logs.append((n, log[:8 * 32768], ln))
        if n == "clean":  # trunc9 on the cut: 9 bytes of the last header in block 7
            pos = last = 7 * 32768
            while pos + 11 <= 8 * 32768:
                last = pos
                pos += (11 if recyclable else 7) + int(log[pos + 4]) + (int(log[pos + 5]) << 8)
            logs.append(("trunc9", log[:last + 9], ln))
    return logs


@pytest.mark.parametrize("recyclable", [False, True])
def test_wal_shim_replays_the_readers_records(tmp_path, recyclable):
    """forst_gpu::WalRecovery::Recover / Next over log files, as a ForSt caller
    replays a WAL into the memtable: every record's offset, size, fragment
    count, checksum and BYTES (their XXH3), every report in front of the
    record the reference's reporter saw it before, the trailing reports, an OK
    status and the stop fields equal the serial reader's, line for line, in
    all four WALRecoveryModes -- on every stop cause, fragment-count sequence
    and tiny log of walcases.stop_and_fragment_cases and on cuts of the
    scenario logs, control records between the fragments of a record
    included (Next steps over them: they are in no record's bytes)"""
    exe = _build(tmp_path)
    args, want = [], []
    for i, (name, log, ln) in enumerate(shim_replay_logs(recyclable)):
        path = str(tmp_path / f"{i:03d}.log")
        with open(path, "wb") as f:
            f.write(bytes(log))
        for mode in range(4):
            text = expected_transcript(log, ln, mode)
            with open(f"{path}.{mode}", "w") as f:
                f.write(text)
            args += [path, f"{path}.{mode}", str(ln), str(mode)]
            want.append((name, mode, f"case {path} {ln} {mode}\n" + text))
    r = subprocess.run([exe, "walfile"] + args, capture_output=True, text=True, timeout=300)
    got = []  # one transcript per "case" line; the binary's own PASS / FAIL lines left out
    for line in r.stdout.splitlines():
        if line.startswith("case "):
            got.append("")
        if got and line[:2] in ("ca", "C ", "R ", "S ", "E "):
            got[-1] += line + "\n"
    assert len(got) == len(want), r.stdout[-2000:] + r.stderr[-2000:]
    for (name, mode, w), g in zip(want, got):
        if g != w:
            gl, wl = g.splitlines(), w.splitlines()
            k = next((j for j, (a, b) in enumerate(zip(gl, wl)) if a != b), min(len(gl), len(wl)))
            raise AssertionError((name, mode, "line", k, "got", gl[k:k + 3], "want", wl[k:k + 3]))
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-2000:] + r.stderr


def test_wal_shim_write_group_and_recovery(tmp_path):
    """forst_gpu::WalWriteGroup frames write groups from the writer's block
    offset with every CRC from one launch (db/log_writer.cc:65-160, :228-263),
    and forst_gpu::WalRecovery hands the records back in reader order with
    the reader's reports (db/db_impl/db_impl_open.cc:1195-1260), legacy and
    recyclable logs"""
    exe = _build(tmp_path)
    r = subprocess.run([exe, "wal"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
