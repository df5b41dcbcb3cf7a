"""What include/forst_checksum.h promises about the OUTPUTS of the WAL and
WriteBatch calls, on the GPU: nothing stored past a capacity or through a NULL
member, the first `capacity` entries and the full counts when a capacity is
short, 0 in the protection slots no record filled -- and two things no parity
test at small shapes reaches: the scan every WAL pipeline rests on above 1024
tiles, and every entry point on a caller's stream other than the null stream.

No output handed to the engine here comes from torch.empty: every one is
torch.full with the sentinels of tests/dispatch.py, GUARD cells longer than the
capacity passed, and read back whole (tests/contracts.py holds the checks, the
twins on the SIMT emulator are tests/test_emu_contracts.py).  Every comparison
is exact."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from forst_amd import ForstError, engine  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import wal_reader as R  # noqa: E402
import contracts as C  # noqa: E402
import kvsites  # noqa: E402
import walcases as W  # noqa: E402
import test_gpu_kv_sites as K  # noqa: E402
import test_gpu_paths as P  # noqa: E402
import test_wal_recover as T  # noqa: E402
from test_wal_golden import reason_text  # noqa: E402

DEV = "cuda"
NT = O.host_threads()
GUARD = C.GUARD
PIT = R.kPointInTimeRecovery
FORST_EINVAL = -1
DT = {8: torch.int64, 4: torch.int32, 1: torch.uint8}
REC_KEYS = [k for k, _ in C.REC_FIELDS]
REP_KEYS = [k for k, _ in C.REP_FIELDS]
d, host, same = P.d, P.host, P.same


def filled(n, size):
    """n + GUARD cells of the sentinel"""
    return torch.full((n + GUARD,), C.sentinel(size), dtype=DT[size], device=DEV)


# ---- forst_wal_recover_batch: capacities and NULL members --------------------

GROUPS = ["legacy", "recyclable", "paths"]
_logs, _ample, _counted = {}, {}, {}


def recovery_logs(group):
    """-> [(name, log, device log, log number, modes)], built once per module"""
    if group not in _logs:
        if group == "paths":
            # wal_short_rows_kernel; the second rw_emit_kernel pass; a raw list over
            # 64 K entries (the remainder hashing and rw_scatter_kernel)
            logs = [(f"short{int(r)}", T._short_lengths_log(r, 3, 3), 7) for r in (False, True)]
            logs += [(f"{n}{int(r)}", log, ln) for r in (False, True)
                     for n, log, ln in W.long_control_runs(r)]
            rng = np.random.default_rng(29)
            raw, po, _ = W.frame_lens(rng.integers(20, 300, 150_000).astype(np.uint32), 6)
            for off in po[1::2]:
                W.set_type(raw, int(off), 30)
            for off in rng.choice(po[1::2], 5, replace=False):
                raw[int(off) + 7] ^= 0x04
            logs.append(("raw", raw, 7))
            modes = [PIT]
        else:
            logs = W.scenarios(group == "recyclable", 37)
            modes = T.MODES
        _logs[group] = [(name, log, d(log), ln, modes) for name, log, ln in logs]
    return _logs[group]


def recover_into(dlog, ln, mode, rcap, pcap, nulls="none"):
    """one call, retry=False, into sentinel-filled arrays of rcap / pcap + GUARD
    cells (the members of NULL set `nulls` passed as NULL) -> (records, reports
    as member name -> whole host array or None, result)"""
    null_rec, null_rep = C.NULL_SETS[nulls]
    recs = {k: filled(rcap, s) for k, s in C.REC_FIELDS if k not in null_rec}
    reps = {k: filled(pcap, s) for k, s in C.REP_FIELDS if k not in null_rep}
    rec, rep, res = engine.wal_recover_batch(dlog, ln, mode, record_capacity=rcap,
                                             report_capacity=pcap, records=recs, reports=reps,
                                             retry=False)
    assert all(rec[k] is recs.get(k) for k in REC_KEYS)  # returned unsliced, NULL stays None
    assert all(rep[k] is reps.get(k) for k in REP_KEYS)
    return ({k: None if rec[k] is None else host(rec[k]) for k in REC_KEYS},
            {k: None if rep[k] is None else host(rep[k]) for k in REP_KEYS}, res)


def ample(group, i, mode):
    """log i of the group recovered with capacity count + GUARD: equal to the
    serial reader's answer, nothing stored behind the counts.  Kept per log
    and mode as the expectation of the short-capacity calls."""
    key = (group, i, mode)
    if key not in _ample:
        name, log, dlog, ln, _ = recovery_logs(group)[i]
        want_recs, want_reps = R.read_all(log, ln, mode)
        n, m = len(want_recs), len(want_reps)
        recs, reps, res = recover_into(dlog, ln, mode, n + GUARD, m + GUARD)
        assert (res.n_records, res.n_reports, res.truncated) == (n, m, 0), (name, mode)
        T.compare([recs[k][:n] for k in REC_KEYS], [reps[k][:m] for k in REP_KEYS], res, log, ln,
                  mode, name)
        for k, size in C.REC_FIELDS:
            C.untouched(recs[k], n, size, (name, mode, "records", k))
        for k, size in C.REP_FIELDS:
            C.untouched(reps[k], m, size, (name, mode, "reports", k))
        _ample[key] = dict(rec={k: recs[k][:n].copy() for k in REC_KEYS},
                           rep={k: reps[k][:m].copy() for k in REP_KEYS},
                           res={f: getattr(res, f) for f in C.RES_FIELDS})
    return _ample[key]


@pytest.mark.parametrize("group", GROUPS)
def test_recover_ample_capacity(group):
    """every scenario log in both header forms and all four modes, and in
    point-in-time mode the short-lengths log, the long control runs and the
    raw list over 64 K entries: the serial reader's records and reports, and
    cells [count, end) of all eight arrays still the sentinel"""
    cases = 0
    for i, (name, log, dlog, ln, modes) in enumerate(recovery_logs(group)):
        for mode in modes:
            a = ample(group, i, mode)
            cases += 1
            if name == "raw":
                assert a["res"]["n_physical"] > 65536
    _counted[("ample", group)] = cases
    print(f"ample-capacity (log, mode) cases [{group}]: {cases}")


@pytest.mark.parametrize("recyclable", [False, True])
def test_recover_stop_and_fragment_cases(recyclable):
    """the small logs of walcases.stop_and_fragment_cases -- each stop cause at
    a block start, mid-block, in the short last block and as the first record,
    with and without a First open; the fragment-count sequences; empty and tiny
    logs -- each uploaded once, all four modes, into sentinel-filled arrays:
    every record (fragment count included), report and result scalar equals
    the serial reader's, and nothing is stored behind the counts"""
    reasons = set()
    for name, log, ln in W.stop_and_fragment_cases(recyclable):
        assert len(log) <= 6 * 32768
        dlog = d(log)
        for mode in T.MODES:
            want = R.read_all_ex(log, ln, mode)
            n, m = len(want["records"]), len(want["reports"])
            recs, reps, res = recover_into(dlog, ln, mode, n + GUARD, m + GUARD)
            T.compare([recs[k][:n] for k in REC_KEYS], [reps[k][:m] for k in REP_KEYS], res, log,
                      ln, mode, name)
            for k, size in C.REC_FIELDS:
                C.untouched(recs[k], n, size, (name, mode, "records", k))
            for k, size in C.REP_FIELDS:
                C.untouched(reps[k], m, size, (name, mode, "reports", k))
            reasons.add(res.stop_reason)
    # (an old record and a recycled log's tolerated tail need recyclable headers)
    assert reasons == {R.STOP_EOF, R.STOP_TRUNCATED_HEADER, R.STOP_TRUNCATED_BODY} | \
        ({R.STOP_OLD_RECORD, R.STOP_RECYCLED_TAIL} if recyclable else set())


@pytest.mark.parametrize("group", GROUPS)
def test_recover_short_capacity_and_null_members(group):
    """the same logs and modes with the seven capacity pairs of
    contracts.capacity_pairs, and the pairs (n - 1, m - 1) and (n, m) with each
    NULL set: success, the ample run's counts and stop fields, truncated exactly
    when a count exceeds its capacity, cells [0, min(capacity, count)) of every
    array equal to the ample run's, every other cell (guards included) still
    the sentinel"""
    cases, cut = 0, 0
    for i, (name, log, dlog, ln, modes) in enumerate(recovery_logs(group)):
        for mode in modes:
            a = ample(group, i, mode)
            n, m = a["res"]["n_records"], a["res"]["n_reports"]
            for rcap, pcap, nulls in C.short_cases(n, m):
                recs, reps, res = recover_into(dlog, ln, mode, rcap, pcap, nulls)
                C.check_short(recs, reps, res, a, rcap, pcap, (name, mode, rcap, pcap, nulls))
                cases += 1
                cut += res.truncated
    assert cut > cases // 3  # the copy-out of a truncated call is what this is about
    _counted[("short", group)] = cases
    print(f"short-capacity (log, mode, capacity, NULL set) cases [{group}]: {cases}, "
          f"{cut} truncated")


# ---- forst_wal_record_xxh3_batch: output bounds, NULL first_phys -------------

def _xxh3_logs():
    out = []
    for recyclable in (False, True):
        buf, po, payload, lens, _ = W.frag_edge_log(recyclable, repeat=2)
        out.append((f"frag_edge{int(recyclable)}", buf, po, W.expected_hashes(payload, lens)))
    rng = np.random.default_rng(0xB3)
    lens = np.exp(rng.uniform(np.log(1), np.log(40000), 3000)).astype(np.uint32)
    payload = rng.integers(0, 256, int(lens.astype(np.int64).sum()), dtype=np.uint8)
    buf, po, _ = O.wal_frame(payload, lens, recyclable=False, log_number=9)
    out.append(("log_uniform", buf, po, W.expected_hashes(payload, lens)))
    return out


_xxh3 = {}


def xxh3_logs():
    if not _xxh3:
        _xxh3["logs"] = _xxh3_logs()
    return _xxh3["logs"]


def writer_first(buf, po):
    """index of each logical record's first physical record (Full / First)"""
    t = buf[po.astype(np.int64) + 6]
    t = np.where((t >= 5) & (t <= 8), t - 4, t)
    return np.nonzero((t == 1) | (t == 2))[0].astype(np.uint64)


def test_record_xxh3_outputs():
    """hashes = XXH3 of every logical record, first = the writer's layout, the
    cells from n_logical on untouched in both (their capacity is n_phys), and
    first_phys = NULL leaves the hashes as they are"""
    for name, buf, po, want in xxh3_logs():
        nphys, nl = len(po), len(want)
        assert nphys > nl
        dlog, dpo = d(buf), d(po)
        hashes, first = filled(nphys, 8), filled(nphys, 8)
        h, f = engine.wal_record_xxh3_batch(dlog, dpo, hashes=hashes, first=first)
        assert len(h) == nl and len(f) == nl, name
        same(host(hashes)[:nl], want, (name, "hashes"))
        same(host(first)[:nl], writer_first(buf, po), (name, "first"))
        C.untouched(host(hashes), nl, 8, (name, "hashes"))
        C.untouched(host(first), nl, 8, (name, "first"))
        hashes2 = filled(nphys, 8)
        h, f = engine.wal_record_xxh3_batch(dlog, dpo, hashes=hashes2, first=False)
        assert f is None and len(h) == nl
        same(host(hashes2), host(hashes), (name, "hashes without first"))


# ---- forst_write_batch_protect_batch: unfilled slots, NULL members, capacity --

_wb = {}


def wb_batch(seed=0xB4):
    if seed not in _wb:
        _wb[seed] = kvsites.wb_contract_batch(seed=seed)
    return _wb[seed]


def wb_outputs(wb, capacity):
    n = wb["n"]
    return dict(prot=filled(capacity, 8), first_entry=filled(n + 1, 8), status=filled(n, 1),
                n_protected=filled(n, 4))


def test_write_batch_outputs():
    """300 reps with header counts raised by 1, 2 and 3, lowered or zeroed, reps
    of 0..11 bytes, cut reps and descriptors past the buffer
    (kvsites.wb_contract_batch asserts that each occurs), against
    oracle.write_batch_protect: status, n_protected, the filled slots,
    first_entry = the cumsum of the header counts of the reps in range, exactly
    0 in every slot no record filled (reps with column family records among
    them), guards untouched; status / n_protected = NULL change nothing else;
    capacity total - 1 fails with FORST_EINVAL, reports the total and leaves
    prot untouched from end to end"""
    wb = wb_batch()
    total = len(wb["prot"])
    args = (d(wb["base"]), d(wb["offs"]), d(wb["lens"]))
    for nulls in ((), ("status",), ("n_protected",)):
        o = wb_outputs(wb, total)
        kw = {k: (False if k in nulls else v) for k, v in o.items()}
        prot, first, st, nprot = engine.write_batch_protect_batch(*args, capacity=total, **kw)
        assert len(prot) == total and len(first) == wb["n"] + 1
        assert (st is None, nprot is None) == ("status" in nulls, "n_protected" in nulls)
        C.check_write_batch(host(o["prot"]), host(o["first_entry"]),
                            None if st is None else host(o["status"]),
                            None if nprot is None else host(o["n_protected"]), wb, nulls)
        for k in nulls:  # (not handed over: still as filled)
            C.untouched(host(o[k]), 0, o[k].element_size(), (nulls, k))
    o = wb_outputs(wb, total - 1)
    with pytest.raises(ForstError) as ei:
        engine.write_batch_protect_batch(*args, capacity=total - 1, **o)
    assert ei.value.code == FORST_EINVAL and ei.value.n_total == total
    C.untouched(host(o["prot"]), 0, 8, "capacity total - 1: prot")
    C.untouched(host(o["first_entry"]), wb["n"] + 1, 8, "capacity total - 1: first_entry")


# ---- scan_u64 above 1024 tiles (scan_top_kernel's multi-tile runs) -----------

SCAN_TILE, SCAN_RUNS = 2048, 1024  # scan_common.h: kScanTile values a tile, 1024 runs of tiles


def test_recover_and_record_xxh3_above_1024_scan_tiles():
    """a clean log of 2 048 * 1024 + 4097 logical records of 0..8 bytes (every
    50 000th 40 000 bytes: fragmented records): above 1024 tiles scan_top_kernel
    gives every lane a run of several tiles.  Every record's offset, length,
    hash and fragment count and the first-fragment indices against the writer's
    layout and the oracle's XXH3 of every record; then one payload flip in each
    of three log blocks against the serial reader replayed around each flip"""
    rng = np.random.default_rng(0xB5)
    n = SCAN_TILE * SCAN_RUNS + 4097
    lens = rng.integers(0, 9, n).astype(np.uint32)
    lens[::50_000] = 40_000
    payload = rng.integers(0, 256, int(lens.astype(np.int64).sum()), dtype=np.uint8)
    log, po, pl = O.wal_frame(payload, lens, recyclable=False, log_number=0)
    types = log[po.astype(np.int64) + 6]
    starts0 = np.nonzero((types == 1) | (types == 2))[0]
    hashes = O.wal_record_xxh3_batch(log, po, pl, starts0, hs=7, nthreads=NT)
    exp, starts, ends = T.clean_expectation(po, pl, types, hashes, 7)
    nphys = len(po)
    assert n > SCAN_TILE * SCAN_RUNS and nphys > SCAN_TILE * SCAN_RUNS and len(starts) == n
    print(f"scan test: {n} logical records, {nphys} physical records, {len(log)} log bytes")
    dlog = d(log)

    def recover(n_want, m_want):
        recs = {k: filled(n_want + GUARD, s) for k, s in C.REC_FIELDS}
        reps = {k: filled(m_want + GUARD, s) for k, s in C.REP_FIELDS}
        rec, rep, res = engine.wal_recover_batch(
            dlog, 0, PIT, record_capacity=n_want + GUARD, report_capacity=m_want + GUARD,
            records=recs, reports=reps, retry=False)
        assert (res.n_records, res.n_reports, res.truncated) == (n_want, m_want, 0)
        got = {k: host(recs[k]) for k in REC_KEYS}
        rp = {k: host(reps[k]) for k in REP_KEYS}
        for k, s in C.REC_FIELDS:
            C.untouched(got[k], n_want, s, ("records", k))
        for k, s in C.REP_FIELDS:
            C.untouched(rp[k], m_want, s, ("reports", k))
        return {k: v[:n_want] for k, v in got.items()}, {k: v[:m_want] for k, v in rp.items()}, res

    got, _, res = recover(n, 0)
    assert res.n_physical == nphys
    for k in REC_KEYS:
        same(got[k], exp[k].astype(got[k].dtype) if k != "hash" else exp[k].view(np.uint64), k)
    hs_out, first_out = filled(nphys, 8), filled(nphys, 8)
    h, f = engine.wal_record_xxh3_batch(dlog, d(po), hashes=hs_out, first=first_out)
    assert len(h) == n
    same(host(hs_out)[:n], hashes, "record xxh3")
    same(host(first_out)[:n], starts.astype(np.uint64), "first")
    C.untouched(host(hs_out), n, 8, "record xxh3")
    C.untouched(host(first_out), n, 8, "first")

    nblk = (len(log) + 32767) // 32768
    victims, vblocks, pos = T.pick_flips(rng, po, pl, nblk, 3, 7)
    bad = log.copy()
    bad[pos] ^= 0x01
    dlog[d(pos.astype(np.int64))] ^= 0x01
    wo, wl, wh, want_reps, outside = T.windowed_expectation(
        lambda a, b: bad[a:b], exp, starts, victims, vblocks, len(bad), PIT, 0, False)
    got, rp, res = recover(len(wo), len(want_reps))
    same(got["offset"], wo.astype(np.uint64), "offset after flips")
    same(got["length"], wl.astype(np.uint64), "length after flips")
    same(got["hash"], wh, "hash after flips")
    sel = np.isin(got["offset"], exp["offset"][outside].astype(np.uint64))
    same(got["n_fragments"][sel], exp["n_fragments"][outside].astype(np.uint32), "n_fragments")
    gr = [(int(b), reason_text(int(r), int(t)), int(o))
          for o, b, r, t in zip(*[rp[k] for k in REP_KEYS])]
    assert gr == want_reps and sum(1 for g in gr if g[1] == "checksum mismatch") == 3
    del dlog
    torch.cuda.empty_cache()


# ---- every entry point on a caller's stream ----------------------------------

class StreamJob:
    """the calls of one stream: inputs cloned and outputs sentinel-filled on
    that stream, so everything the calls depend on is ordered by it alone;
    every tensor is kept until the final synchronise"""

    def __init__(self, stream, k):
        self.s, self.k, self.keep, self.checks = stream, k, [], []
        self.async_calls, self.sync_calls = [], []
        self.blocks()
        self.raw()
        self.kv()
        self.memtable()
        self.wal_writer()
        self.synchronous()

    def up(self, a):
        t = d(a)
        torch.cuda.synchronize()
        with torch.cuda.stream(self.s):
            c = t.clone()
        self.keep += [t, c]
        return c

    def out(self, n, size, value=None):
        with torch.cuda.stream(self.s):
            t = filled(n, size) if value is None else \
                torch.full((n,), value, dtype=DT[size], device=DEV)
        self.keep.append(t)
        return t

    def expect(self, t, want, what, n=None):
        """after the final synchronise: t[:len(want)] == want, the rest untouched"""
        def check():
            got = host(t)
            same(got[:len(want)], want, (self.k, what))
            if n is None:
                C.untouched(got, len(want), t.element_size(), (self.k, what))
        self.checks.append(check)

    def blocks(self):
        hb, offs, sizes, lasts, mods = P.edge_layout(False, seed=7 + self.k)
        n = len(offs)
        dbase, doffs, dsizes = self.up(hb), self.up(offs), self.up(sizes)
        dlasts, dmods = self.up(lasts), self.up(mods)
        self.edge = (hb, offs, sizes, mods, dbase, doffs, dsizes, dmods)
        for ct in P.HASH_TYPES:
            sums = P.want_compute(ct, hb, offs, sizes, lasts, mods)
            img = P.with_trailers(hb, offs, sizes, lasts, sums)
            damaged = img.copy()
            damaged[int(offs[5 + self.k]) + int(sizes[5 + self.k]) + 1] ^= 1
            damaged[int(offs[n - 1])] ^= 0x80
            wc, ws, wok, wbad = P.want_verify(ct, damaged, offs, sizes, mods)
            dtr, dimg = self.up(hb), self.up(damaged)
            oc, ot = self.out(n, 4), self.out(n, 4)
            comp, stored, ok = self.out(n, 4), self.out(n, 4), self.out(n, 1)
            count = self.out(1, 8, 1000)
            self.async_calls += [
                lambda ct=ct, oc=oc: engine.block_checksum_batch(
                    ct, dbase, doffs, dsizes, last_bytes=dlasts, modifiers=dmods, out=oc),
                lambda ct=ct, dtr=dtr, ot=ot: engine.block_trailer_batch(
                    ct, dtr, doffs, dsizes, dlasts, dmods, ot),
                lambda ct=ct, dimg=dimg, comp=comp, stored=stored, ok=ok, count=count:
                    engine.block_verify_batch(ct, dimg, doffs, dsizes, modifiers=dmods,
                                              computed=comp, stored=stored, ok=ok,
                                              mismatches=count)]
            self.expect(oc, sums, (ct, "compute"))
            self.expect(ot, sums, (ct, "trailer"))
            self.expect(dtr, img, (ct, "image"), n=len(img))
            self.expect(comp, wc, (ct, "computed"))
            self.expect(stored, ws, (ct, "stored"))
            self.expect(ok, wok, (ct, "ok"))
            self.expect(count, np.array([1000 + wbad], np.uint64), (ct, "mismatches"), n=1)

    def raw(self):
        hb, offs, sizes, init, dbase, doffs, dsizes, dinit = self.edge
        n = len(offs)
        wcrc = np.array([O.crc32c_extend(int(i), hb[int(o):int(o) + int(s)])
                         for i, o, s in zip(init, offs, sizes)], np.uint32)
        crc, xx, buf, comb = self.out(n, 4), self.out(n, 8), self.out(1, 4), self.out(n, 4)
        rng = np.random.default_rng(78 + self.k)
        c1 = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        c2 = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        ln = rng.integers(0, 2**40, n, dtype=np.uint64)
        ln[:6] = [0, 1, 3, 4, 65536, (1 << 63) + 5]
        d1, d2, dl = self.up(c1), self.up(c2), self.up(ln)
        self.async_calls += [
            lambda: engine.crc32c_batch(dbase, doffs, dsizes, init_crcs=dinit, out=crc),
            lambda: engine.xxh3_64_batch(dbase, doffs, dsizes, out=xx),
            lambda: engine.crc32c_buffer(dbase, 0x12345678 + self.k, out=buf),
            lambda: engine.crc32c_combine_batch(d1, d2, dl, out=comb)]
        self.expect(crc, wcrc, "crc32c_batch")
        self.expect(xx, O.xxh3_batch(hb, offs, sizes, nthreads=NT), "xxh3_64_batch")
        self.expect(buf, np.array([O.crc32c_extend(0x12345678 + self.k, hb.tobytes())], np.uint32),
                    "crc32c_buffer")
        self.expect(comb, np.array([O.crc32c_combine(int(a), int(b), int(c))
                                    for a, b, c in zip(c1, c2, ln)], np.uint32), "combine")

    def kv(self):
        kv = P.kv_case(seed=77 + self.k)
        n = kv["n"]
        a = {x: self.up(kv[x]) for x in ("base", "ko", "ks", "vo", "vs", "co", "ops", "seqs")}
        h, p, c, ok = self.out(n, 8), self.out(n, 8), self.out(n, 8), self.out(n, 1)
        count = self.out(1, 8, 1000)
        self.async_calls += [
            lambda: engine.hash64_batch(a["base"], a["vo"], a["vs"], seed=O.KV_SEED_V, out=h),
            lambda: engine.kv_protect_batch(a["base"], a["ko"], a["ks"], a["vo"], a["vs"],
                                            a["ops"], a["seqs"], out=p),
            lambda: engine.kv_verify_batch(a["base"], a["ko"], a["ks"], a["vo"], a["vs"], 8,
                                           a["co"], a["ops"], a["seqs"], computed=c, ok=ok,
                                           mismatches=count)]
        self.expect(h, O.hash64_batch(kv["base"], kv["vo"], kv["vs"], seed=O.KV_SEED_V), "hash64")
        self.expect(p, kv["prot"], "kv_protect")
        self.expect(c, kv["prot"], "kv_verify computed")
        self.expect(ok, np.ones(n, np.uint8), "kv_verify ok")
        self.expect(count, np.array([1000], np.uint64), "kv_verify mismatches", n=1)

    def memtable(self):
        n = 3000
        base, offs, cp = K.make_memtable(n, 8, 0xA15F + self.k)
        # the checksums the protect call must write, from the oracle: an entry
        # whose checksum bytes are zero fails with status 4 and its computed value
        wcomp, _ = O.memtable_verify_batch(base, len(base), offs.view(np.uint64), 8)
        img = base.copy()
        for j in range(8):
            img[cp + j] = (wcomp >> np.uint64(8 * j)).astype(np.uint8)
        g, go = self.up(base), self.up(offs)
        po, ps = self.out(n, 8), self.out(n, 1)
        vc, vs = self.out(n, 8), self.out(n, 1)
        count = self.out(1, 8, 1000)
        self.async_calls += [
            lambda: engine.memtable_protect_batch(g, go, 8, out=po, status=ps),
            lambda: engine.memtable_verify_batch(g, go, 8, computed=vc, status=vs,
                                                 mismatches=count)]  # (after the protect call)
        self.expect(po, wcomp, "memtable_protect")
        self.expect(ps, np.zeros(n, np.uint8), "memtable_protect status")
        self.expect(g, img, "memtable image", n=len(img))
        self.expect(vc, wcomp, "memtable_verify")
        self.expect(vs, np.zeros(n, np.uint8), "memtable_verify status")
        self.expect(count, np.array([1000], np.uint64), "memtable_verify mismatches", n=1)

    def wal_writer(self):
        recyclable = bool(self.k)
        rng = np.random.default_rng(41 + self.k)
        lens = np.exp(rng.uniform(np.log(1), np.log(40000), 600)).astype(np.uint32)
        payload = rng.integers(0, 256, int(lens.astype(np.int64).sum()), dtype=np.uint8)
        buf, poffs, plens = O.wal_frame(payload, lens, recyclable=recyclable, log_number=P.LOGNUM)
        wiped = buf.copy()
        for o in poffs:
            wiped[int(o):int(o) + 4] = 0
        wcrc = P.le32_at(buf, poffs.astype(np.int64))
        dpo, dpl = self.up(poffs), self.up(plens)
        for kw in ({}, {"payload_lengths": dpl, "recyclable": recyclable}):
            dl, crcs = self.up(wiped), self.out(len(poffs), 4)
            self.async_calls.append(lambda dl=dl, crcs=crcs, kw=kw: engine.wal_record_crc_batch(
                dl, dpo, out=crcs, **kw))
            self.expect(crcs, wcrc, ("wal_record_crc", bool(kw)))
            self.expect(dl, buf, ("wal_record_crc image", bool(kw)), n=len(buf))

    def synchronous(self):
        k = self.k
        # wal_verify_batch / wal_recover_batch: a scenario log of the recovery tests
        group, want_name = ("legacy", "crc") if k == 0 else ("recyclable", "retype")
        i = [c[0] for c in recovery_logs(group)].index(want_name)
        name, log, _, ln, _ = recovery_logs(group)[i]
        a = ample(group, i, PIT)
        n, m = a["res"]["n_records"], a["res"]["n_reports"]
        dlog = self.up(log)
        ost, onr, ofo = O.wal_verify_blocks(log, ln, nthreads=NT)
        nb = len(ost)
        st, nr, fo, bad = self.out(nb, 1), self.out(nb, 4), self.out(nb, 4), self.out(1, 8, 1000)
        self.sync_calls.append(lambda: engine.wal_verify_batch(
            dlog, log_number=ln, bad_blocks=bad, status=st, nrec=nr, fail_off=fo))
        self.expect(st, ost, "wal_verify status")
        self.expect(nr, onr, "wal_verify nrec")
        self.expect(fo, ofo, "wal_verify fail_off")
        self.expect(bad, np.array([1000 + P.wal_bad(ost)], np.uint64), "wal_verify bad", n=1)
        # wal_record_xxh3_batch: a fragment-edge log of test_record_xxh3_outputs
        xname, xbuf, xpo, xwant = xxh3_logs()[k]
        dx, dxpo = self.up(xbuf), self.up(xpo)
        hashes, first = self.out(len(xpo), 8), self.out(len(xpo), 8)
        self.sync_calls.append(lambda: engine.wal_record_xxh3_batch(dx, dxpo, hashes=hashes,
                                                                    first=first))
        self.expect(hashes, xwant, "record xxh3")
        self.expect(first, writer_first(xbuf, xpo), "record xxh3 first")
        # wal_recover_batch
        recs = {f: self.out(n + GUARD, s) for f, s in C.REC_FIELDS}
        reps = {f: self.out(m + GUARD, s) for f, s in C.REP_FIELDS}
        self.sync_calls.append(lambda: engine.wal_recover_batch(
            dlog, ln, PIT, record_capacity=n + GUARD, report_capacity=m + GUARD, records=recs,
            reports=reps, retry=False))
        for f in REC_KEYS:
            self.expect(recs[f], a["rec"][f], ("recover records", f))
        for f in REP_KEYS:
            self.expect(reps[f], a["rep"][f], ("recover reports", f))
        # write_batch_protect_batch
        wb = wb_batch(0xB4 + k)
        total = len(wb["prot"])
        wargs = (self.up(wb["base"]), self.up(wb["offs"]), self.up(wb["lens"]))
        o = {f: self.out(cap, s) for f, cap, s in (
            ("prot", total, 8), ("first_entry", wb["n"] + 1, 8), ("status", wb["n"], 1),
            ("n_protected", wb["n"], 4))}
        self.sync_calls.append(lambda: engine.write_batch_protect_batch(*wargs, capacity=total,
                                                                        **o))
        self.checks.append(lambda: C.check_write_batch(
            host(o["prot"]), host(o["first_entry"]), host(o["status"]), host(o["n_protected"]),
            wb, (k, "write batch")))
        # block_kv_checksum_batch: 700 blocks of the random batch of test_gpu_kv_sites
        base, offs, sizes, kinds, blocks = K.random_batch()
        sl = slice(700 * k, 700 * (k + 1))
        pb = 4 if k == 0 else 8
        wfirst, wst, wenc, wprot = kvsites.restated_batch(blocks[sl], pb)
        cap, nblk = int(wfirst[-1]), 700
        bargs = (self.up(base), self.up(offs[sl]), self.up(sizes[sl]), self.up(kinds[sl]))
        enc, prot = self.out(cap * pb, 1), self.out(cap, 8)
        bfirst, bst = self.out(nblk + 1, 8), self.out(nblk, 1)
        self.sync_calls.append(lambda: engine.block_kv_checksum_batch(
            *bargs, pb, capacity=cap, kv_checksums=enc, prot=prot, first_key=bfirst, status=bst))
        self.expect(enc, wenc, "kv_checksums")
        self.expect(prot, wprot, "block prot")
        self.expect(bfirst, wfirst.astype(np.uint64), "first_key")
        self.expect(bst, wst, "block status")


HIP_STREAM_NON_BLOCKING = 0x01  # hip_runtime_api.h: hipStreamNonBlocking


def stream_flags(s):
    """hipStreamGetFlags of a torch stream, asked of the HIP runtime this
    process already has loaded (the path from the process's own mappings, so
    that no second copy of the runtime is opened)"""
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    assert len(paths) == 1, paths
    hip = ctypes.CDLL(paths.pop())
    flags = ctypes.c_uint(0xFFFFFFFF)
    rc = hip.hipStreamGetFlags(ctypes.c_void_p(s.cuda_stream), ctypes.byref(flags))
    assert rc == 0, rc
    return flags.value


def test_entry_points_on_two_caller_streams():
    """every device-resident entry point on two torch side streams, asserted to
    be non-blocking ones (they do not synchronise with the null stream, the one
    configuration that hides an ordering mistake), each with its own batches
    whose producers ran on that stream alone.  The calls that do not
    synchronise are issued alternately for the two streams with no
    synchronisation in between, then the synchronous ones A, B, A, B; both
    streams are synchronised once and every result compared with the oracle"""
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    assert sa.cuda_stream != sb.cuda_stream and 0 not in (sa.cuda_stream, sb.cuda_stream)
    for s in (sa, sb):
        assert stream_flags(s) & HIP_STREAM_NON_BLOCKING, hex(stream_flags(s))
    ja, jb = StreamJob(sa, 0), StreamJob(sb, 1)
    torch.cuda.synchronize()
    results = []
    for calls_a, calls_b in ((ja.async_calls, jb.async_calls), (ja.sync_calls, jb.sync_calls)):
        assert len(calls_a) == len(calls_b)
        for ca, cb in zip(calls_a, calls_b):
            with torch.cuda.stream(sa):
                results.append(ca())
            with torch.cuda.stream(sb):
                results.append(cb())
    assert len(ja.async_calls) == 3 * 4 + 4 + 3 + 2 + 2 and len(ja.sync_calls) == 5
    sa.synchronize()
    sb.synchronize()
    for job in (ja, jb):
        for check in job.checks:
            check()
    del results, ja, jb
