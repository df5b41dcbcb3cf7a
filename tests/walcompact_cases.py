"""tests/walcompact_cases.py -- TEST INFRASTRUCTURE ONLY: the cases of
forst_wal_records_compact (forst_amd/csrc/wal_compact.h) that
tests/test_emu_wal_compact.py runs on the SIMT emulator and
tests/test_gpu_wal_compact.py on the device.

The oracle is the serial reader (oracle/wal_reader.py Reader.read_record): the
expected arena is its payloads laid out with the 16-byte rounding and zero
padding, built in numpy, and compared whole -- padding, and the sentinel cells
behind *arena_bytes, included.

A runner is a library with the engine's C ABI plus the memory it works on:
  up(array)   -> a handle (.ptr, .host()) of a copy of the numpy array in the
                 runner's memory, 16-byte aligned
The emulator's memory is host memory (HostRunner); the device twin lives in the
GPU test file.  Every output array is handed over prefilled with the sentinels
of tests/dispatch.py, GUARD cells longer than needed, and read back whole.
"""
import ctypes
import struct

import numpy as np

import dispatch as D
import walcases as W
from forst_amd.engine import WalRecords, WalReports, WalRecoverResult, _recover_sig
from oracle import oracle as O
from oracle import wal_reader as R

GUARD = 8
S8, S32, S64 = D.SENTINEL8, D.SENTINEL32, D.SENTINEL32 * 0x100000001
BLOCK = 32768
EINVAL = -1

# wal_compact.h: bytes per destination piece, arena bytes per wave store /
# per thread stride / per tile, records searched per LDS window; the payload
# bytes of a whole block behind a 7- / 11-byte header
PIECE, WAVE_STORE, THREAD_STRIDE, TILE, WINDOW = 16, 1024, 4096, 16384, 1023
STEPS = (WAVE_STORE, THREAD_STRIDE, TILE, BLOCK - 11, BLOCK - 7, BLOCK)


def bind(L):
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    f = L.forst_wal_records_compact
    f.restype = ctypes.c_int
    f.argtypes = [vp, u64, vp, vp, vp, u64, vp, u64, vp, vp, vp, vp, vp]
    L.forst_write_batch_protect_batch.restype = ctypes.c_int
    L.forst_write_batch_protect_batch.argtypes = [vp, u64, vp, vp, u64, vp, vp, u64, vp, vp, vp, vp]
    L.forst_xxh3_64_batch.restype = ctypes.c_int
    L.forst_xxh3_64_batch.argtypes = [vp, u64, vp, vp, vp, u64, vp]
    L.forst_last_error.restype = ctypes.c_char_p
    _recover_sig(L)
    return L


class _HostBuf:
    def __init__(self, a):
        raw = np.zeros(a.nbytes + 64, np.uint8)
        at = (-raw.ctypes.data) % 16
        self.a = raw[at:at + a.nbytes].view(a.dtype)
        self.a[:] = a
        self.ptr = self.a.ctypes.data

    def host(self):
        return self.a.copy()


class HostRunner:
    """a library whose 'device' is host memory (the emulator)"""

    def __init__(self, L):
        self.L = bind(L)

    def up(self, a):
        return _HostBuf(np.ascontiguousarray(a))


def _ptr(h):
    return None if h is None else h.ptr


# ---- the calls ------------------------------------------------------------------

class Result:
    pass


def compact(run, log, off, length, nfrag, capacity="fit", nulls=(), log_h=None, log_len=None,
            arena_h=None):
    """one forst_wal_records_compact call -> Result with rc, total and the whole
    output arrays (None where NULL was passed).  capacity: "fit" (a count-only
    call first, then an arena of exactly the total), None (count-only: arena
    NULL, capacity 0) or a number (an arena of that many bytes + GUARD)."""
    n = len(off)
    off_h = run.up(np.asarray(off, np.uint64))
    len_h = run.up(np.asarray(length, np.uint64))
    nf_h = run.up(np.asarray(nfrag, np.uint32))
    log_h = log_h or run.up(log if len(log) else np.zeros(4, np.uint8))
    log_len = len(log) if log_len is None else log_len
    total = ctypes.c_uint64(S64)

    def call(cap, arena_h):
        outs = {"rep_offsets": run.up(np.full(n + GUARD, S64, np.uint64)),
                "rep_sizes": run.up(np.full(n + GUARD, S32, np.uint32)),
                "status": run.up(np.full(n + GUARD, S8, np.uint8))}
        for k in nulls:
            outs[k] = None
        if arena_h is None and cap is not None:
            arena_h = run.up(np.full(cap + GUARD * PIECE, S8, np.uint8))
        rc = run.L.forst_wal_records_compact(
            log_h.ptr, log_len, off_h.ptr, len_h.ptr, nf_h.ptr, n, _ptr(arena_h),
            0 if cap is None else cap, _ptr(outs["rep_offsets"]), _ptr(outs["rep_sizes"]),
            _ptr(outs["status"]), ctypes.byref(total), None)
        r = Result()
        r.rc, r.total = rc, total.value
        r.arena = None if arena_h is None else arena_h.host()
        for k, h in outs.items():
            setattr(r, k, None if h is None else h.host())
        r.log_h, r.arena_h = log_h, arena_h
        return r

    if capacity == "fit":
        r = call(None, None)
        assert r.rc == 0, run.L.forst_last_error()
        capacity = r.total
    return call(capacity, arena_h)


def recover(run, log, log_number, mode=2):
    """forst_wal_recover_batch through the runner -> (offset, length, hash, n_fragments)"""
    cap = max(64, len(log) // 7 + 2)
    recs = [run.up(np.zeros(cap, t)) for t in (np.uint64, np.uint64, np.uint64, np.uint32)]
    reps = [run.up(np.zeros(cap, t)) for t in (np.uint64, np.uint64, np.uint32, np.uint32)]
    log_h = run.up(log if len(log) else np.zeros(4, np.uint8))
    res = WalRecoverResult()
    rc = run.L.forst_wal_recover_batch(log_h.ptr, len(log), log_number, mode,
                                       WalRecords(*[h.ptr for h in recs]), cap,
                                       WalReports(*[h.ptr for h in reps]), cap,
                                       ctypes.byref(res), None)
    assert rc == 0, run.L.forst_last_error()
    return tuple(h.host()[:res.n_records] for h in recs)


# ---- the oracle -----------------------------------------------------------------

def reader_records(log, log_number=0, mode=2):
    """the serial reader's records: [(LastRecordOffset, payload bytes, n_fragments)]"""
    r = R.Reader(log, log_number)
    out = []
    while True:
        got = r.read_record(mode)
        if got is None:
            return out
        out.append((got[0], bytes(got[1]), r.n_fragments))


def descriptors(records):
    return (np.array([r[0] for r in records], np.uint64),
            np.array([len(r[1]) for r in records], np.uint64),
            np.array([r[2] for r in records], np.uint32))


def expected(payloads, status=None):
    """(arena, rep_offsets, rep_sizes) for the payloads; a record with a
    non-zero status has size 0"""
    n = len(payloads)
    sizes = np.array([0 if (status is not None and status[i]) else len(p)
                      for i, p in enumerate(payloads)], np.uint64)
    rounded = (sizes + np.uint64(15)) & ~np.uint64(15)
    offs = np.concatenate([[0], np.cumsum(rounded)]).astype(np.uint64)
    arena = np.zeros(int(offs[n]), np.uint8)
    for i, p in enumerate(payloads):
        if sizes[i]:
            arena[int(offs[i]):int(offs[i]) + len(p)] = np.frombuffer(p, np.uint8)
    return arena, offs[:n], sizes.astype(np.uint32)


def check(r, payloads, status=None, what=""):
    """a Result against the expected layout, every cell of every array"""
    n = len(payloads)
    st = np.zeros(n, np.uint8) if status is None else np.asarray(status, np.uint8)
    arena, offs, sizes = expected(payloads, st)
    assert r.rc == 0 and r.total == len(arena), (what, r.rc, r.total, len(arena))
    for name, got, want, sent in (("status", r.status, st, S8), ("rep_sizes", r.rep_sizes, sizes, S32),
                                  ("rep_offsets", r.rep_offsets, offs, S64),
                                  ("arena", r.arena, arena, S8)):
        if got is None:
            continue
        bad = np.nonzero(got[:len(want)] != want)[0]
        assert bad.size == 0, (what, name, int(bad.size), bad[:8].tolist(),
                               got[bad[:8]].tolist(), want[bad[:8]].tolist())
        assert (got[len(want):] == sent).all(), (what, name, "stored past its end")


def check_log(run, log, log_number=0, mode=2, records=None, what="", order=None, want=None):
    """compact the reader's records of a log (or the given descriptors of
    them) into an arena of exactly the expected size and compare with the
    reader's payloads (want: the reader's records when the caller has them)"""
    want = reader_records(log, log_number, mode) if want is None else want
    off, length, nfrag = descriptors(want) if records is None else records
    assert len(off) == len(want), (what, len(off), len(want))
    if records is not None:
        assert (off == descriptors(want)[0]).all() and (nfrag == descriptors(want)[2]).all(), what
    pay = [w[1] for w in want]
    if order is not None:
        off, length, nfrag = off[order], length[order], nfrag[order]
        pay = [pay[i] for i in order]
    if len(off) == 0:
        return 0
    total = sum((len(p) + 15) // 16 * 16 for p in pay)
    check(compact(run, log, off, length, nfrag, capacity=total), pay, what=what)
    return len(off)


# ---- logs -----------------------------------------------------------------------

def _add_record(b, L):
    """log::Writer::AddRecord of L random bytes (log_writer.cc:65-160)"""
    hs = 11 if b.rec else 7
    left, first = L, True
    while first or left > 0:
        o = len(b.buf) % BLOCK
        if BLOCK - o < hs:
            b.buf += bytes(BLOCK - o)
            o = 0
        n = min(left, BLOCK - o - hs)
        end = n == left
        b.put(1 if first and end else 2 if first else 4 if end else 3, n)
        left -= n
        first = False


STEP_LENGTHS = sorted({s + d for s in STEPS for d in (-17, -1, 0, 1, 17)})


def sweep_log(recyclable, lengths, seed=3):
    """every one of `lengths` with its payload starting at every source
    alignment mod 16 (a pad record of 0..15 bytes in front of each moves it
    there), in shuffled order"""
    rng = np.random.default_rng(seed)
    hs = 11 if recyclable else 7
    b = W._Log(recyclable, 7, seed=seed)
    for a in range(16):
        part = list(lengths)
        rng.shuffle(part)
        for L in part:
            if BLOCK - len(b.buf) % BLOCK < 2 * hs + 16 + 1:
                b.goto(0)  # no room for the pad and the record's first byte
            b.put(1, (a - (len(b.buf) + 2 * hs)) % 16)
            assert (len(b.buf) + hs) % 16 == a
            _add_record(b, L)
    return b.array()


def alignments_seen(log, records):
    """{length: set of (first payload offset mod 16)} of the records (their
    offset is their first fragment's header here)"""
    seen = {}
    for off, pay, nf in records:
        if len(pay):
            p0 = off + W.hdr_size(log, off)
            seen.setdefault(len(pay), set()).add(p0 % 16)
    return seen


def layout_logs(recyclable):
    """(name, log, log_number): skipped block tails in front of a record and
    between its fragments, an empty First in a block's last bytes, records that
    end exactly at a block end, and a log that ends in a short block with a
    fragmented record (no read past the log)"""
    hs = 11 if recyclable else 7
    out = []
    tails = range(7, 11) if recyclable else range(1, 7)
    b = W._Log(recyclable, 7, seed=21)
    for k in tails:
        b.goto(BLOCK - k)
        b.put(1, 100 + k)                # the tail in front of a Full record
        b.goto(BLOCK - k - hs - 40)
        b.put(2, 40), b.put(4, 50 + k)   # ... and between First and Last
        b.goto(BLOCK - k - hs - 5)
        b.put(2, 5), b.put(3, BLOCK - hs), b.put(4, 3000)  # ... in a record that goes on regularly
    out.append(("tails", b.array(), 7))
    b = W._Log(recyclable, 7, seed=22)
    b.goto(BLOCK - hs)
    b.put(2, 0), b.put(3, BLOCK - hs), b.put(4, 77)  # an empty First in the block's last bytes
    b.goto(BLOCK - hs)
    b.put(2, 0), b.put(4, 5)
    b.goto(500)
    b.put(1, BLOCK - 500 - hs)                       # a Full record ends at the block end
    b.put(2, BLOCK - hs), b.put(4, BLOCK - hs)       # two whole blocks, ends at the block end
    b.put(1, 9)
    b.goto(BLOCK - hs - 16)
    b.put(2, 16), b.put(3, BLOCK - hs), b.put(3, BLOCK - hs), b.put(3, BLOCK - hs), b.put(4, 1)
    b.put(2, 300), b.put(4, 20)                      # fragments that do not fill their block
    b.goto(BLOCK - hs - 3)
    b.put(2, 3), b.put(4, 40)                        # the log ends 40 bytes into its last block
    out.append(("edges", b.array(), 7))
    return out


def big_record_log(recyclable, seed=8):
    """records of about 1 MiB (33 fragments) starting at three alignments, the
    last one ending at the log's end"""
    lens = [5, (1 << 20) + 3, 1234, (1 << 20) - 29, 6, 700001]
    return W.frame_lens(lens, seed, recyclable)[0]


def many_records_log(n=66000, seed=12):
    """more than 64 Ki records (empty ones among them) and a few long ones"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 40, n)
    lens[rng.integers(0, n, 2000)] = 0
    lens[1000:3200] = 0        # a run of empty records longer than two LDS windows
    lens[rng.integers(0, n, 6)] = 40000
    return W.frame_lens(lens, seed, False)[0]


# ---- bad descriptors --------------------------------------------------------------

def bad_descriptor_case(recyclable, seed=14):
    """(log, off, length, nfrag, payloads, status): good records with bad
    descriptors among them"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 3000, 60)
    lens[[7, 20, 33]] = [40000, 70000, 33000]
    lens[[10, 16, 21]] = [100, 200, 300]  # (behind the records that take a fragment too many)
    log = W.frame_lens(lens, seed, recyclable)[0]
    recs = reader_records(log, 7)
    off, length, nfrag = descriptors(recs)
    pay = [r[1] for r in recs]
    status = np.zeros(len(recs), np.uint8)
    hs = 11 if recyclable else 7

    def bad(i, o=None, ln=None, nf=None):
        if o is not None:
            off[i] = o
        if ln is not None:
            length[i] = ln
        if nf is not None:
            nfrag[i] = nf
        status[i] = 1

    bad(3, o=len(log) + 5)              # an offset past log_len
    bad(4, o=len(log))
    bad(5, o=2**64 - 3)
    bad(9, nf=2**31)                    # absurd fragment counts
    bad(20, nf=2**31)
    bad(11, ln=int(length[11]) + 1)     # a length one off, both ways
    bad(7, ln=int(length[7]) - 1)
    bad(13, o=int(off[13]) + hs + 2)    # an offset that points into a payload
    bad(33, o=int(off[33]) + hs + 9)
    bad(15, nf=int(nfrag[15]) + 1)      # one fragment more: takes the next record's
    bad(len(recs) - 1, nf=3)            # ... or walks off the log's end
    length[17] = 2**32                  # longer than the protect call can take
    status[17] = 2
    length[18] = 2**63 + 5
    status[18] = 2
    return log, off, length, nfrag, pay, status


# ---- the chain --------------------------------------------------------------------

def chain_log(recyclable, seed=0xC4):
    """WriteBatch reps (kvsites.wb_rep) framed as WAL records, some of them
    spanning blocks, a few malformed or shorter than the 12-byte header"""
    import kvsites as K
    rng = np.random.default_rng(seed)
    reps = [K.wb_rep(rng, int(rng.integers(0, 60))) for _ in range(40)]
    reps[5] = reps[5][:7]
    reps[9] = b""
    reps[12] = reps[12][:-3]
    lens = np.array([len(r) for r in reps], np.uint32)
    pay = np.frombuffer(b"".join(reps), np.uint8)
    buf, po, pl = O.wal_frame(pay, lens, recyclable=recyclable, log_number=7)
    assert len(po) > len(reps) + 5  # several reps span blocks
    return buf.copy(), reps


def protect(run, base_h, base_len, offs, sizes):
    """forst_write_batch_protect_batch -> (prot, first_entry, status, n_protected)"""
    n = len(offs)
    off_h, sz_h = run.up(np.asarray(offs, np.uint64)), run.up(np.asarray(sizes, np.uint32))
    first = run.up(np.zeros(n + 1, np.uint64))
    total = ctypes.c_uint64()
    run.L.forst_write_batch_protect_batch(base_h.ptr, base_len, off_h.ptr, sz_h.ptr, n, first.ptr,
                                          None, 0, None, None, ctypes.byref(total), None)
    prot = run.up(np.zeros(max(1, total.value), np.uint64))
    st, npr = run.up(np.zeros(n, np.uint8)), run.up(np.zeros(n, np.uint32))
    rc = run.L.forst_write_batch_protect_batch(base_h.ptr, base_len, off_h.ptr, sz_h.ptr, n,
                                               first.ptr, prot.ptr, total.value, st.ptr, npr.ptr,
                                               ctypes.byref(total), None)
    assert rc == 0, run.L.forst_last_error()
    return prot.host()[:total.value], first.host(), st.host(), npr.host()


def xxh3(run, base_h, base_len, offs, sizes):
    n = len(offs)
    off_h, sz_h = run.up(np.asarray(offs, np.uint64)), run.up(np.asarray(sizes, np.uint32))
    out = run.up(np.zeros(n, np.uint64))
    rc = run.L.forst_xxh3_64_batch(base_h.ptr, base_len, off_h.ptr, sz_h.ptr, out.ptr, n, None)
    assert rc == 0, run.L.forst_last_error()
    return out.host()


def run_chain(run, recyclable):
    """recover -> compact -> protect on the arena == protect on the host-joined
    reps uploaded directly; XXH3 over the arena == the reader's payload_xxh3"""
    log, reps = chain_log(recyclable)
    off, length, _, nfrag = recover(run, log, 7)
    assert len(off) == len(reps) and (length == [len(r) for r in reps]).all()
    assert int((nfrag > 1).sum()) >= 3
    r = compact(run, log, off, length, nfrag)
    check(r, reps, what="chain")
    n = len(reps)
    got = protect(run, r.arena_h, r.total, r.rep_offsets[:n], r.rep_sizes[:n])
    # the host-joined reps, 8-byte aligned, as KvProtection::Stage lays them out
    offs, img = [], bytearray()
    for rep in reps:
        offs.append(len(img))
        img += rep + bytes(-len(rep) % 8)
    img += bytes(16)
    want = protect(run, run.up(np.frombuffer(bytes(img), np.uint8)), len(img), offs,
                   [len(x) for x in reps])
    for name, g, w in zip(("prot", "first_entry", "status", "n_protected"), got, want):
        assert len(g) == len(w) and (g == w).all(), name
    assert len(set(want[2].tolist())) > 1  # good and malformed reps
    h = xxh3(run, r.arena_h, r.total, r.rep_offsets[:n], r.rep_sizes[:n])
    ex = R.read_all_ex(log, 7)
    assert (h == np.array(ex["payload_xxh3"], np.uint64)).all()


# ---- the cases, as the two test files run them ------------------------------------

def case_sweep(run, recyclable, lengths=range(301)):
    """every length at every source alignment mod 16 (asserted on the log)"""
    log = sweep_log(recyclable, lengths)
    recs = reader_records(log, 7)
    seen = alignments_seen(log, recs)
    for L in lengths:
        if L:
            assert seen[L] == set(range(16)), (L, seen[L])
    assert check_log(run, log, 7, what="sweep", want=recs) == len(recs)


def case_sweep_steps(run, recyclable):
    """the lengths s, s +- 1, s +- 17 around every step of the kernel, each at
    every source alignment mod 16"""
    assert len(STEP_LENGTHS) >= 26
    case_sweep(run, recyclable, STEP_LENGTHS)


def overlong_fragment_case(recyclable, seed=17):
    """(log, off, length, nfrag, payloads): data fragments whose 16-bit length
    runs past their block's end -- no writer's, but the walk WalRecovery::Next
    does (the one this call ports) takes such a payload as it lies,
    contiguous -- as a record of one fragment, as the First of two, and one
    that ends 2 bytes in front of the log's end; a good record around them"""
    rng = np.random.default_rng(seed)
    hs = 11 if recyclable else 7
    base = 4 if recyclable else 0
    log = rng.integers(0, 256, 5 * BLOCK, np.uint8)

    def header(at, t, n):
        log[at + 4:at + 6] = np.frombuffer(struct.pack("<H", n), np.uint8)
        log[at + 6] = t + base
        return at + hs + n

    recs = []
    e = header(100, 1, 40000)                      # one fragment over a block end
    recs.append((100, [(100 + hs, 40000)], 1))
    e2 = header(e, 1, 50)                          # a good record behind it
    recs.append((e, [(e + hs, 50)], 1))
    f1 = header(e2, 2, 30000)                      # First over the next block end, then Last
    f2 = header(f1, 4, 700)
    recs.append((e2, [(e2 + hs, 30000), (f1 + hs, 700)], 2))
    at = 3 * BLOCK - hs - 1                        # header in a block's last bytes, 65535 bytes
    end = header(at, 1, 65535)
    recs.append((at, [(at + hs, 65535)], 1))
    log = log[:end + 2].copy()
    off = np.array([r[0] for r in recs], np.uint64)
    pay = [b"".join(bytes(log[p:p + n]) for p, n in r[1]) for r in recs]
    return (log, off, np.array([len(p) for p in pay], np.uint64),
            np.array([r[2] for r in recs], np.uint32), pay)


def case_overlong_fragments(run, recyclable, up_log=None):
    log, off, length, nfrag, pay = overlong_fragment_case(recyclable)
    r = compact(run, log, off, length, nfrag, log_h=(up_log or run.up)(log))
    check(r, pay, what="overlong fragments")


def case_fragment_edges(run, recyclable):
    buf = W.frag_edge_log(recyclable)[0]
    assert check_log(run, buf, 9, what="frag_edge") > 100
    for name, log, ln in layout_logs(recyclable):
        n = check_log(run, log, ln, what=name)
        assert n >= 9, (name, n)
    frags = inside = 0
    for name, log, ln in W.stop_and_fragment_cases(recyclable):
        recs = reader_records(log, ln)
        frags = max([frags] + [r[2] for r in recs])
        inside += _control_offsets(log, recs)
        check_log(run, log, ln, what=name)
    assert frags >= 5 and inside >= 6, (frags, inside)


def case_big_records(run, recyclable):
    log = big_record_log(recyclable)
    recs = reader_records(log, 7)
    assert max(r[2] for r in recs) >= 33 and recs[-1][2] > 20
    check_log(run, log, 7, what="big")


def _control_offsets(log, records):
    """records whose offset is a control record (it lay between their fragments)"""
    return sum(1 for o, _, nf in records if 9 <= log[o + 6] <= 11)


def case_control(run, recyclable, via_recover=("ctl_frag",)):
    """via_recover: the scenarios whose descriptors come from
    forst_wal_recover_batch through the runner (None: all); the others take
    the serial reader's (tests/test_wal_recover.py and tests/test_wal_golden.py
    pin the recovery's records to the reader's, on the emulator too) -- one
    emulated recovery of these logs takes 2-3 s, so all of them in four modes
    would add minutes to the CPU suite; the device run takes every one"""
    inside = 0
    for name, log, ln in W.control_scenarios(recyclable, 19, n=120):
        records = None
        if via_recover is None or name in via_recover:
            got = recover(run, log, ln)
            records = (got[0], got[1], got[3])
        inside += _control_offsets(log, reader_records(log, ln))
        check_log(run, log, ln, records=records, what=name)
    assert inside >= 1, inside


def case_scenarios(run, recyclable, mode, via_recover=("retype",)):
    total = 0
    for name, log, ln in W.scenarios(recyclable, 29, n=120):
        records = None
        if via_recover is None or name in via_recover:
            got = recover(run, log, ln, mode)
            records = (got[0], got[1], got[3])
        total += check_log(run, log, ln, mode, records=records, what=(name, mode))
    assert total > 500


def case_many_records(run):
    log = many_records_log()
    recs = reader_records(log, 7)
    n = len(recs)
    assert n > 65536
    assert check_log(run, log, 7, what="many", want=recs) == n
    check_log(run, log, 7, what="reversed", order=np.arange(n)[::-1], want=recs)
    check_log(run, log, 7, what="strided", order=np.arange(5, n, 7), want=recs)


def case_contracts(run):
    log = W.frame_lens([10, 0, 40000, 16, 17, 300, 0], 4, False)[0]
    recs = reader_records(log, 7)
    off, length, nfrag = descriptors(recs)
    pay = [r[1] for r in recs]
    arena, offs, sizes = expected(pay)
    n, total = len(recs), len(arena)
    # the count-only call: offsets, sizes, status and the total, no arena
    r = compact(run, log, off, length, nfrag, capacity=None)
    assert r.arena is None
    check(r, pay, what="count-only")
    # every NULL set: the others are as before, nothing else is written
    for nulls in (("rep_offsets",), ("rep_sizes",), ("status",),
                  ("rep_offsets", "rep_sizes", "status")):
        r = compact(run, log, off, length, nfrag, nulls=nulls)
        assert all(getattr(r, k) is None for k in nulls)
        check(r, pay, what=nulls)
    # a larger arena: bytes at and past *arena_bytes stay as they were
    check(compact(run, log, off, length, nfrag, capacity=total + 100), pay, what="ample")
    # a short arena: FORST_EINVAL with the total, the arena untouched, the
    # per-record outputs filled
    for cap in (total - 1, total - 16, 16, 1):
        r = compact(run, log, off, length, nfrag, capacity=cap)
        assert r.rc == EINVAL and r.total == total, (cap, r.rc, r.total)
        assert (r.arena == S8).all(), cap
        assert (r.rep_offsets[:n] == offs).all() and (r.rep_sizes[:n] == sizes).all()
        assert (r.status[:n] == 0).all()
        assert b"arena_capacity" in run.L.forst_last_error()
    # no record: *arena_bytes = 0, nothing else touched
    r = compact(run, log, off[:0], length[:0], nfrag[:0], capacity=64)
    assert r.rc == 0 and r.total == 0
    assert (r.arena == S8).all() and (r.rep_offsets == S64).all() \
        and (r.rep_sizes == S32).all() and (r.status == S8).all()
    # an arena that overlaps the log
    whole = run.up(np.concatenate([log, np.zeros((-len(log)) % 16 + total + 64, np.uint8)]))

    class Part:
        def __init__(self, at):
            self.ptr = whole.ptr + at

        def host(self):
            return whole.host()[self.ptr - whole.ptr:]

    for at in (0, len(log) // 16 * 16 - 16, 16):
        r = compact(run, log, off, length, nfrag, capacity=total, log_h=whole, arena_h=Part(at))
        assert r.rc == EINVAL and b"overlap" in run.L.forst_last_error(), at
    before = whole.host()
    at = (len(log) + 15) // 16 * 16  # right behind the log: allowed
    r = compact(run, log, off, length, nfrag, capacity=total, log_h=whole, arena_h=Part(at))
    assert r.rc == 0 and r.total == total
    after = whole.host()
    assert (after[at:at + total] == arena).all() and (after[:at] == before[:at]).all() \
        and (after[at + total:] == before[at + total:]).all()


def case_bad_descriptors(run, recyclable, up_log=None):
    log, off, length, nfrag, pay, status = bad_descriptor_case(recyclable)
    assert int((status == 0).sum()) > 40
    log_h = (up_log or run.up)(log)
    r = compact(run, log, off, length, nfrag, log_h=log_h)
    check(r, pay, status, what="bad descriptors")
    # the good records alone give the same bytes
    good = np.nonzero(status == 0)[0]
    r2 = compact(run, log, off[good], length[good], nfrag[good], log_h=log_h)
    assert r2.total == r.total and (r2.arena == r.arena).all()
