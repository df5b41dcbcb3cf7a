"""tests/contracts.py -- TEST INFRASTRUCTURE ONLY: what include/forst_checksum.h
promises about the OUTPUTS of forst_wal_recover_batch beyond their values --
nothing stored past a capacity, nothing stored through a NULL member, the
first `capacity` entries and the full counts when a capacity is short -- as
checks over whole, sentinel-prefilled output arrays.  Shared by the GPU tests
(tests/test_gpu_contracts.py) and their twins on the SIMT emulator
(tests/test_emu_contracts.py).

Every output array handed to the engine is GUARD cells longer than the
capacity passed, prefilled with the sentinels of tests/dispatch.py, and read
back whole."""
import numpy as np

import dispatch as D
from forst_amd.engine import WAL_RECORD_FIELDS, WAL_REPORT_FIELDS

GUARD = 8
S32, S64, S8 = D.SENTINEL32, D.SENTINEL32 * 0x100000001, D.SENTINEL8

REC_FIELDS, REP_FIELDS = WAL_RECORD_FIELDS, WAL_REPORT_FIELDS  # (member, bytes per entry)
RES_FIELDS = ("n_records", "n_reports", "n_physical", "stop_offset", "stop_reason")

# the members passed as NULL: (of forst_wal_records, of forst_wal_reports)
NULL_SETS = {
    "none": ((), ()),
    "hash": (("hash",), ()),
    "all_but_hash_and_reason": (("offset", "length", "n_fragments"), ("offset", "bytes", "type")),
    "all": (tuple(k for k, _ in REC_FIELDS), tuple(k for k, _ in REP_FIELDS)),
}


def sentinel(size):
    return {8: S64, 4: S32, 1: S8}[size]


def capacity_pairs(n, m):
    """(record capacity, report capacity) for a log of n records and m reports"""
    return [(0, 0), (1, 1), (max(n - 1, 0), max(m - 1, 0)), (n, m), (n + 1, m + 1),
            (5, m + GUARD), (n + GUARD, 1)]


def short_cases(n, m):
    """every (record capacity, report capacity, NULL set) of the short-capacity
    contract: the seven pairs with all members present, and the pairs
    (n - 1, m - 1) and (n, m) with each NULL set"""
    pairs = capacity_pairs(n, m)
    out = [(r, p, "none") for r, p in pairs]
    for r, p in pairs[2:4]:
        out += [(r, p, s) for s in ("hash", "all_but_hash_and_reason", "all")]
    return out


def untouched(arr, start, size, what):
    """cells [start, end) of a whole output array still hold the sentinel"""
    bad = np.nonzero(arr[start:] != sentinel(size))[0]
    assert bad.size == 0, (what, "stored past its bound at", (bad[:8] + start).tolist(),
                           [hex(int(x)) for x in arr[start:][bad[:8]]])


def prefix(arr, want, cap, size, what):
    """arr (whole, cap + GUARD cells): the first min(cap, count) cells equal
    want's, every other cell is the sentinel"""
    assert len(arr) == cap + GUARD, (what, len(arr), cap)
    k = min(cap, len(want))
    bad = np.nonzero(arr[:k] != want[:k])[0]
    assert bad.size == 0, (what, int(bad.size), bad[:8].tolist(),
                           [hex(int(x)) for x in arr[bad[:8]]],
                           [hex(int(x)) for x in want[bad[:8]]])
    untouched(arr, k, size, what)


def check_short(recs, reps, res, ample, rcap, pcap, what):
    """one forst_wal_recover_batch call with capacities (rcap, pcap) against the
    ample-capacity run of the same log and mode.  recs / reps: member name ->
    the whole host array (unsigned), or None where NULL was passed; ample:
    dict(rec=, rep= the ample run's arrays cut to their counts, res= its
    RES_FIELDS)."""
    n, m = ample["res"]["n_records"], ample["res"]["n_reports"]
    for f in RES_FIELDS:
        assert getattr(res, f) == ample["res"][f], (what, f, getattr(res, f), ample["res"][f])
    assert res.truncated == int(n > rcap or m > pcap), (what, res.truncated, n, rcap, m, pcap)
    assert res.unsupported == 0, what
    for got, want, cap, fields in ((recs, ample["rec"], rcap, REC_FIELDS),
                                   (reps, ample["rep"], pcap, REP_FIELDS)):
        for k, size in fields:
            if got[k] is not None:
                prefix(got[k], want[k], cap, size, (what, k))


def check_write_batch(prot, first, status, nprot, wb, what):
    """one forst_write_batch_protect_batch call over kvsites.wb_contract_batch()
    against its oracle answer.  prot / first / status / nprot: the whole host
    arrays (unsigned; status / nprot None where NULL was passed), each GUARD
    cells longer than its capacity"""
    n, total = wb["n"], len(wb["prot"])
    assert len(first) == n + 1 + GUARD, what
    same = [("first_entry", first, wb["first"], 8), ("prot", prot, wb["prot"], 8)]
    if status is not None:
        same.append(("status", status, wb["status"], 1))
    if nprot is not None:
        same.append(("n_protected", nprot, wb["nprot"], 4))
    for name, got, want, size in same:
        bad = np.nonzero(got[:len(want)] != want)[0]
        assert bad.size == 0, (what, name, int(bad.size), bad[:8].tolist(),
                               [hex(int(x)) for x in got[bad[:8]]],
                               [hex(int(x)) for x in want[bad[:8]]])
        untouched(got, len(want), size, (what, name))
    # slots no record filled hold exactly 0, also behind records with a column family
    assert len(wb["cf_unfilled"]) > 0 and total > len(wb["unfilled"])
    assert (prot[wb["unfilled"]] == 0).all(), (what, "unfilled slots")
