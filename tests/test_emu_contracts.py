"""The output contracts of forst_wal_recover_batch and
forst_write_batch_protect_batch (include/forst_checksum.h) on the CPU SIMT
emulator: the twins of tests/test_gpu_contracts.py, through tests/contracts.py.
Every output array is prefilled with a sentinel, GUARD cells longer than the
capacity passed, and compared whole.

No twin here: the scan above 1024 tiles (a log of 2.1 M records is hours on
the emulator) and the caller's-stream test (the emulator has no streams)."""
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))

if shutil.which("/opt/rocm/llvm/bin/clang++") is None:
    pytest.skip("needs ROCm clang++ to build the emulator", allow_module_level=True)

import emu  # noqa: E402

import contracts as C  # noqa: E402
import kvsites  # noqa: E402
import walcases as W  # noqa: E402
from oracle import wal_reader as R  # noqa: E402
from test_wal_recover import compare  # noqa: E402

FORST_EINVAL = -1
U = {8: np.uint64, 4: np.uint32, 1: np.uint8}


def filled(n, size):
    return np.full(n + C.GUARD, C.sentinel(size), U[size])


def recover_into(log, ln, mode, rcap, pcap, nulls="none"):
    """one call into sentinel-filled arrays of rcap / pcap + GUARD cells, the
    members of NULL set `nulls` passed as NULL -> (records, reports, result)
    as member name -> whole array or None"""
    null_rec, null_rep = C.NULL_SETS[nulls]
    recs = {k: None if k in null_rec else filled(rcap, s) for k, s in C.REC_FIELDS}
    reps = {k: None if k in null_rep else filled(pcap, s) for k, s in C.REP_FIELDS}
    _, _, res = emu.wal_recover(log, ln, mode, cap=rcap, rep_cap=pcap,
                                records=tuple(recs[k] for k, _ in C.REC_FIELDS),
                                reports=tuple(reps[k] for k, _ in C.REP_FIELDS))
    return recs, reps, res


@pytest.mark.slow  # 14 recoveries at 3-4 s each on the emulator, and its build
def test_recover_capacities_and_null_members_on_emulator():
    """the first 3 log blocks + 1000 bytes of the re-typed log (legacy headers,
    point-in-time recovery).  Ample capacity: the serial reader's records and
    reports, nothing stored behind the counts.  Then every short capacity pair
    and NULL set of contracts.short_cases: success, the full counts and stop
    fields, truncated exactly when a count exceeds its capacity, the first
    `capacity` entries of every array, every other cell untouched."""
    name, log, ln = [s for s in W.scenarios(False, 11) if s[0] == "retype"][0]
    log = log[:3 * 32768 + 1000]
    mode = R.kPointInTimeRecovery
    want_recs, want_reps = R.read_all(log, ln, mode)
    n, m = len(want_recs), len(want_reps)
    assert n > 5 + 1 and m > 1, (n, m)  # every capacity pair cuts something else
    recs, reps, res = recover_into(log, ln, mode, n + C.GUARD, m + C.GUARD)
    assert (res.n_records, res.n_reports, res.truncated) == (n, m, 0)
    compare([recs[k][:n] for k, _ in C.REC_FIELDS], [reps[k][:m] for k, _ in C.REP_FIELDS], res,
            log, ln, mode, name)
    for k, size in C.REC_FIELDS:
        C.untouched(recs[k], n, size, ("ample", k))
    for k, size in C.REP_FIELDS:
        C.untouched(reps[k], m, size, ("ample", k))
    ample = dict(rec={k: recs[k][:n].copy() for k, _ in C.REC_FIELDS},
                 rep={k: reps[k][:m].copy() for k, _ in C.REP_FIELDS},
                 res={f: getattr(res, f) for f in C.RES_FIELDS})
    cases = C.short_cases(n, m)
    assert len(cases) == 13
    for rcap, pcap, nulls in cases:
        recs, reps, res = recover_into(log, ln, mode, rcap, pcap, nulls)
        C.check_short(recs, reps, res, ample, rcap, pcap, (name, rcap, pcap, nulls))


def wb_into(wb, capacity, status=True, nprot=True):
    n = wb["n"]
    prot, first = filled(capacity, 8), filled(n + 1, 8)
    st = filled(n, 1) if status else None
    npr = filled(n, 4) if nprot else None
    rc, total = emu.write_batch_protect_into(wb["base"], wb["offs"], wb["lens"], capacity, prot,
                                             first, st, npr)
    return rc, total, prot, first, st, npr


def test_write_batch_outputs_on_emulator():
    """300 reps with header counts raised by 1, 2 and 3, lowered or zeroed, reps
    of 0..11 bytes, cut reps and descriptors past the buffer
    (kvsites.wb_contract_batch asserts that each occurs): status, n_protected,
    the filled slots, first_entry = the cumsum of the header counts, exactly 0
    in every slot no record filled, guards untouched; NULL status /
    n_protected change nothing else; capacity total - 1 fails with
    FORST_EINVAL, reports the total and stores no protection value"""
    wb = kvsites.wb_contract_batch()
    total = len(wb["prot"])
    for status, nprot in ((True, True), (False, True), (True, False)):
        rc, tot, prot, first, st, npr = wb_into(wb, total, status, nprot)
        assert (rc, tot) == (0, total)
        C.check_write_batch(prot, first, st, npr, wb, (status, nprot))
    rc, tot, prot, first, st, npr = wb_into(wb, total - 1)
    assert (rc, tot) == (FORST_EINVAL, total)
    C.untouched(prot, 0, 8, "capacity total - 1: prot")
    C.untouched(first, wb["n"] + 1, 8, "capacity total - 1: first_entry")
