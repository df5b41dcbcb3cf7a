"""WAL logs whose multi-fragment records cross log-block boundaries at chosen
places -- the cases the fragment-aware XXH3 (forst_amd/csrc/wal_hash.h,
xxh3.hip xxh3_frag_kernel) maps logical offsets for.

A record whose header lands at block offset o has its first fragment end at
the block end, so its first boundary is l0 = 32768 - o - hs logical bytes in
(log_writer.cc:65-160).  frag_edge_log() places each target record at the
offset giving a chosen l0 by writing a pad record in front of it, and covers:
the boundary at every byte of a 16-byte lane slot and of a 64-byte stripe, at
1 KiB window edges, in the last stripe, the last fragment at 63 / 64 / 65
bytes, records of 241..300 bytes across a boundary, an empty first fragment
(leftover exactly hs), three- and four-fragment records, and short records
(<= 240 bytes) across a boundary (gathered)."""
import struct

import numpy as np

from oracle import oracle as O

BLOCK = 32768


def _advance(o, L, hs):
    """block offset after log::Writer::AddRecord of L bytes at offset o"""
    left = L
    first = True
    while first or left > 0:
        first = False
        if BLOCK - o < hs:
            o = 0
        avail = BLOCK - o - hs
        frag = min(left, avail)
        o += hs + frag
        left -= frag
    return o


def _pad_to(o, target, hs):
    """a record length that moves the writer from block offset o to target"""
    if BLOCK - o < hs:
        o = 0
    if target >= o + hs:
        return target - o - hs
    return (BLOCK - o - hs) + (target - hs)  # ends target bytes into the next block


def cases(rng):
    """(l0, L) pairs: first boundary l0 logical bytes in, record length L"""
    out = []
    for c in range(16):  # boundary at every byte of a lane slot, stripe positions
        for k in (0, 1, 5):
            l0 = 1024 * k + 16 * int(rng.integers(0, 64)) + c
            if l0 == 0:
                l0 = 16
            out.append((l0, l0 + int(rng.integers(64, 4000))))
    for l0 in (1024, 2048, 1023, 1025, 64, 63, 65, 1, 2, 3):  # window / stripe edges
        out.append((l0, l0 + 700))
    for last in (63, 64, 65, 66, 100):  # last fragment length
        out.append((3000, 3000 + last))
        out.append((5, 5 + last + 200))
    for L in range(241, 301, 3):  # just above the short-input limit
        out.append((int(rng.integers(1, L - 63)), L))
    for L in (100, 200, 240, 16):  # short records across a boundary (gathered)
        out.append((int(rng.integers(1, L)), L))
    for l0 in (7, 500, 1000, 30000):  # three and four fragments
        out.append((l0, l0 + 32761 + int(rng.integers(64, 30000))))
        out.append((l0, l0 + 2 * 32761 + int(rng.integers(64, 3000))))
    out.append((0, 5000))  # empty first fragment (header exactly at block end - hs)
    out.append((0, 32761 + 100))
    rng.shuffle(out)
    return out


def frag_edge_log(recyclable=False, seed=5, log_number=9, repeat=1):
    """(log, header offsets, payload, logical lengths, [(record index, l0)])"""
    rng = np.random.default_rng(seed)
    hs = 11 if recyclable else 7
    lens, targets = [], []
    o = 0
    for _ in range(repeat):
        for l0, L in cases(rng):
            want = BLOCK - hs - l0
            pad = _pad_to(o, want, hs)
            lens.append(pad)
            o = _advance(o, pad, hs)
            targets.append((len(lens), l0))
            lens.append(L)
            o = _advance(o, L, hs)
            if rng.integers(0, 3) == 0:  # a small full record between cases
                n = int(rng.integers(0, 300))
                lens.append(n)
                o = _advance(o, n, hs)
    lens = np.array(lens, np.uint32)
    payload = rng.integers(0, 256, int(lens.astype(np.int64).sum()), np.uint8)
    buf, po, pl = O.wal_frame(payload, lens, recyclable=recyclable, log_number=log_number)
    return buf, po, payload, lens, targets


def first_fragment_offsets(buf, po):
    """header offset of each logical record's first fragment (Full / First)"""
    t = buf[po.astype(np.int64) + 6]
    t = np.where((t >= 5) & (t <= 8), t - 4, t)
    return po[(t == 1) | (t == 2)]


def expected_hashes(payload, lens):
    starts = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    return np.array([O.xxh3_64(payload[starts[j]:starts[j + 1]].tobytes())
                     for j in range(len(lens))], np.uint64)


# ---- recovery scenarios (forst_wal_recover_batch; pinned to the reference's
# own log::Reader by tests/golden/gen_wal_golden.py) --------------------------

def frame(n, seed, recyclable=False, log_number=7, hi=70000):
    rng = np.random.default_rng(seed)
    lens = (np.exp(rng.uniform(0, np.log(hi), n))).astype(np.uint32)
    lens[:4] = [0, 32761, 5, 32750]
    pay = rng.integers(0, 256, int(lens.astype(np.int64).sum()), np.uint8)
    buf, po, pl = O.wal_frame(pay, lens, recyclable=recyclable, log_number=log_number)
    return buf.copy(), po, pl


def hdr_size(buf, off):
    t = buf[off + 6]
    return 11 if (5 <= t <= 8 or t == 11) else 7


def set_type(buf, off, t, log_number=None):
    """re-type a physical record and rewrite its CRC (log_writer.cc:240-263)"""
    buf[off + 6] = t
    hs = hdr_size(buf, off)
    n = int(buf[off + 4]) | (int(buf[off + 5]) << 8)
    c = O.mask(O.crc32c_value(bytes(buf[off + 6:off + hs + n])))
    buf[off:off + 4] = np.frombuffer(struct.pack("<I", c), np.uint8)


def set_payload(buf, off, data):
    """overwrite a physical record's leading payload bytes and re-CRC it"""
    hs = hdr_size(buf, off)
    buf[off + hs:off + hs + len(data)] = np.frombuffer(bytes(data), np.uint8)
    set_type(buf, off, int(buf[off + 6]))


def scenarios(recyclable, seed, n=600):
    """(name, log bytes, log_number) cases with every reader outcome"""
    ln = 7
    buf, po, pl = frame(n, seed, recyclable, ln)
    rng = np.random.default_rng(seed + 1)
    types = buf[po.astype(np.int64) + 6]
    out = [("clean", buf, ln)]
    b = buf.copy()  # CRC mismatches (payload flips) in a few blocks
    for k in rng.choice(len(po), 6, replace=False):
        if pl[k]:
            b[int(po[k]) + hdr_size(b, int(po[k])) + int(rng.integers(0, pl[k]))] ^= 0x10
    out.append(("crc", b, ln))
    b = buf.copy()  # re-typed fragments: missing starts, partial records, unknown types
    base = 4 if recyclable else 0
    for k in rng.choice(len(po), 12, replace=False):
        t = int(types[k]) - base
        new = {1: 4, 2: 3, 3: 1, 4: 2}[t] if t in (1, 2, 3, 4) else 1
        if k % 5 == 0:
            new = 12 - base  # 12 = the reader's kEof (log_reader.h:173): reading ends
        set_type(b, int(po[k]), new + base if new < 9 else 12, ln)
    out.append(("retype", b, ln))
    b = buf.copy()  # a zero-filled region (kZeroType + length 0: preallocated space)
    z = int(po[len(po) // 3])
    b[z:z + 300] = 0
    out.append(("zero", b, ln))
    for cut in (3, 9, 5000):  # truncated tail: header / recyclable header / body
        e = int(po[-1]) + min(cut, int(pl[-1]) + 6)
        out.append((f"trunc{cut}", buf[:e].copy(), ln))
    b = buf.copy()  # bad length in a middle block
    k = len(po) // 2
    b[int(po[k]) + 4:int(po[k]) + 6] = 0xFF
    out.append(("badlen", b, ln))
    if recyclable:
        b = buf.copy()  # a record of an older log incarnation
        o = int(po[len(po) // 2])
        b[o + 7:o + 11] = np.frombuffer(struct.pack("<I", ln + 1), np.uint8)
        set_type(b, o, int(b[o + 6]), ln)
        out.append(("old", b, ln))
        b2 = b.copy()  # ... and a corrupt tail of a recycled log
        b2[int(po[-3]) + 12] ^= 1
        out.append(("old+crc", b2, ln))
    return out


def pseudo_type_scenarios(recyclable, seed, n=300):
    """records re-typed (valid CRC) into the reader's own result codes
    12..17 (log_reader.h:173-186), unknown types 18 / 0x7F, and type bytes
    >= 0x80 (sign-extended, log_reader.cc:469), one kind per log, plus a mix
    in which re-typed fragments sit inside fragmented records"""
    ln = 7
    buf, po, pl = frame(n, seed, recyclable, ln)
    rng = np.random.default_rng(seed + 2)
    out = []
    for t in (12, 13, 14, 15, 16, 17, 18, 0x7F, 0x80, 0xFF):
        b = buf.copy()
        for k in sorted(rng.choice(np.arange(8, len(po)), 3, replace=False)):
            set_type(b, int(po[k]), t, ln)
        out.append((f"type{t}", b, ln))
    # a pseudo type in the last (short) log block: kBadRecordLen at eof_
    b = buf.copy()
    set_type(b, int(po[-2]), 16, ln)
    out.append(("type16eof", b, ln))
    b = buf.copy()
    for k, t in zip(sorted(rng.choice(np.arange(8, len(po)), 6, replace=False)),
                    (13, 16, 17, 0x80, 0xFF, 13)):
        set_type(b, int(po[k]), t, ln)
    out.append(("mixed", b, ln))
    # partial records: a First whose Last is re-typed Full (partial ...(1)) or
    # First (partial ...(2) at the following First)
    base = 4 if recyclable else 0
    types = buf[po.astype(np.int64) + 6].astype(int) - base
    two = [k for k in range(len(po) - 1) if types[k] == 2 and types[k + 1] == 4 and pl[k]]
    b = buf.copy()
    for i, k in enumerate(two[1:7]):
        set_type(b, int(po[k + 1]), (1 if i % 2 else 2) + base, ln)
    out.append(("partials", b, ln))
    return out


def frame_lens(lens, seed, recyclable=False, log_number=7):
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.uint32)
    pay = rng.integers(0, 256, int(lens.astype(np.int64).sum()), np.uint8)
    buf, po, pl = O.wal_frame(pay, lens, recyclable=recyclable, log_number=log_number)
    return buf.copy(), po, pl


def make_control(buf, off, rtype, payload):
    """rewrite the Full physical record at `off` as a control record the way
    log::Writer emits one (log_writer.cc:228-263: kSetCompressionType always
    with the 7-byte header, the recyclable timestamp-size type with the
    11-byte one); the record must span exactly header + len(payload)"""
    old_hs = hdr_size(buf, off)
    old_n = int(buf[off + 4]) | (int(buf[off + 5]) << 8)
    hs = 11 if rtype == 11 else 7
    assert old_hs + old_n == hs + len(payload), (old_hs, old_n, hs, len(payload))
    buf[off + 4:off + 6] = np.frombuffer(struct.pack("<H", len(payload)), np.uint8)
    buf[off + hs:off + hs + len(payload)] = np.frombuffer(bytes(payload), np.uint8)
    set_type(buf, off, rtype)


def control_scenarios(recyclable, seed, n=300):
    """kSetCompressionType and user-defined-timestamp-size records
    (log_format.h:37-41) written where a writer puts them and where it never
    does: first in the log, repeated, mid-log, between the fragments of a
    record, with undecodable payloads, zero timestamp sizes and repeated
    column families (log_reader.cc:167-213, UpdateRecordedTimestampSize)"""
    ln = 7
    rng = np.random.default_rng(seed)
    lens = (np.exp(rng.uniform(0, np.log(70000), n))).astype(np.uint32)
    ts_type = 11 if recyclable else 10

    def ts(pairs):
        return b"".join(struct.pack("<IH", cf, t) for cf, t in pairs)

    plan = {
        "ctl_ok": [(0, 9, struct.pack("<I", 0)), (3, ts_type, ts([(1, 8), (2, 16)])),
                   (9, ts_type, ts([(3, 8)])), (40, ts_type, ts([(4, 8), (5, 8), (6, 24)]))],
        "ctl_comp": [(0, 9, struct.pack("<I", 0)), (2, 9, struct.pack("<I", 0)),
                     (5, 9, struct.pack("<I", 0x100)), (8, 9, struct.pack("<I", 3)),
                     (11, 9, struct.pack("<I", 0x205))],
        "ctl_ts": [(1, ts_type, ts([(1, 8)])), (4, ts_type, ts([(2, 0)])),
                   (7, ts_type, ts([(3, 4), (1, 8)])), (10, ts_type, b"\x01" * 7),
                   (13, ts_type, b""), (16, ts_type, ts([(9, 2), (10, 0), (11, 4)]))],
    }
    out = []
    for name, items in plan.items():
        L = lens.copy()
        for k, t, p in items:  # a Full record of the control record's span
            L[k] = len(p) - 4 if (t == 9 and recyclable) else len(p)
        buf, po, pl = frame_lens(L, seed + 1, recyclable, ln)
        first_phys = {}
        j = 0
        types = buf[po.astype(np.int64) + 6]
        for q in range(len(po)):  # logical record -> its first physical record
            t = int(types[q]) - (4 if recyclable else 0)
            if t in (1, 2):
                first_phys[j] = q
                j += 1
        for k, t, p in items:
            q = first_phys[k]
            if int(types[q]) - (4 if recyclable else 0) != 1:
                continue  # (straddles a block: not a single Full record)
            make_control(buf, int(po[q]), t, p)
        out.append((name, buf, ln))
    # control records in place of Middle / Last fragments (a writer never
    # does this; the reader keeps in_fragmented_record across them)
    buf, po, pl = frame(n, seed + 2, recyclable, ln)
    base = 4 if recyclable else 0
    types = buf[po.astype(np.int64) + 6].astype(int) - base
    mids = [k for k in range(len(po)) if types[k] in (3, 4) and pl[k] >= 12]
    b = buf.copy()
    for i, k in enumerate(sorted(np.random.default_rng(seed + 3).choice(mids, 8, replace=False))):
        o = int(po[k])
        n_ = int(pl[k])
        if i % 2:  # a timestamp-size record of the fragment's own length (ragged or not)
            b[o + 6] = ts_type if recyclable else 10
            if n_ % 6 == 0:
                b[o + hdr_size(b, o):o + hdr_size(b, o) + n_] = np.frombuffer(
                    ts([(200 + i * 1000 + x, 8) for x in range(n_ // 6)]), np.uint8)
            set_type(b, o, int(b[o + 6]))
        else:  # a compression record (7-byte header) over the fragment's span
            hs = hdr_size(b, o)
            pay = struct.pack("<I", 0) + bytes(n_ + hs - 7 - 4)
            b[o + 4:o + 6] = np.frombuffer(struct.pack("<H", len(pay)), np.uint8)
            b[o + 7:o + 7 + len(pay)] = np.frombuffer(pay, np.uint8)
            set_type(b, o, 9)
    out.append(("ctl_frag", b, ln))
    return out


def zero_tail_log(recyclable, total=64 << 20, n=40, seed=31):
    """a few records followed by a zero-filled (preallocated) tail"""
    buf, po, pl = frame(n, seed, recyclable, 7, hi=20000)
    out = np.zeros(total, np.uint8)
    out[:len(buf)] = buf
    return out


def old_tail_log(total_blocks=600, seed=33):
    """a recycled log: this incarnation's records followed by an older
    incarnation's (other log number) in the remaining blocks"""
    new, _, _ = frame(200, seed, True, 8, hi=20000)
    old, _, _ = frame(3000, seed + 1, True, 5, hi=20000)
    n = total_blocks * 32768
    out = old[:n].copy() if len(old) >= n else np.concatenate([old, np.zeros(n - len(old), np.uint8)])
    cut = (len(new) // 32768) * 32768 + 32768
    out[:len(new)] = new
    return out[:max(n, cut)]


def long_control_runs(recyclable, run=200, seed=41):
    """runs of `run` consecutive control records (far more than the walk-back
    cap of rw_live_kernel, so the linear fallback decides liveness): inside a
    fragmented record (First ... Last), after a First that never completes,
    and between Full records; timestamp-size records alternate with
    kSetCompressionType ones, one cf is recorded twice with another size"""
    ln = 7
    base = 4 if recyclable else 0
    ts_type = 11 if recyclable else 10
    lens = np.full(4 * run + 80, 12, np.uint32)
    buf, po, pl = frame_lens(lens, seed, recyclable, ln)
    assert len(po) == len(lens)

    def control(k, i):
        o = int(po[k])
        hs = hdr_size(buf, o)
        if i % 2 == 0:  # two (cf, size) pairs: exactly the 12-byte payload
            cf = 5 if i == 40 else 1000 + i  # cf 5 recorded again (8 -> 16) at i == 40
            sz = 16 if i == 40 else 8
            pay = struct.pack("<IHIH", cf, sz, 2000 + i, 8)
            buf[o + 6] = ts_type
            buf[o + hs:o + hs + len(pay)] = np.frombuffer(pay, np.uint8)
            set_type(buf, o, ts_type)
        else:  # compression record with the 7-byte header over the same span
            pay = struct.pack("<I", 0) + bytes(12 + hs - 7 - 4)
            buf[o + 4:o + 6] = np.frombuffer(struct.pack("<H", len(pay)), np.uint8)
            buf[o + 7:o + 7 + len(pay)] = np.frombuffer(pay, np.uint8)
            set_type(buf, o, 9)

    k = 5
    set_type(buf, int(po[k]), 2 + base)          # First ... run ... Last
    for i in range(run):
        control(k + 1 + i, i)
    set_type(buf, int(po[k + 1 + run]), 4 + base)
    k += run + 10
    set_type(buf, int(po[k]), 2 + base)          # First ... run ... Full (partial record)
    for i in range(run):
        control(k + 1 + i, i)
    k += run + 10
    for i in range(run):                          # Full ... run ... Full
        control(k + i, i)
    k += run + 10
    for i in range(run):                          # Full ... run ... First Last
        control(k + i, i)                         # (the Last's hash start walks back
    set_type(buf, int(po[k + run]), 2 + base)     # over the run: rw_emit's capped walk)
    set_type(buf, int(po[k + run + 1]), 4 + base)
    return [("long_ctl", buf, ln)]


# ---- stop causes, fragment counts and tiny logs, built record by record -----

class _Log:
    """a log written one physical record at a time, the writer's block rule
    kept (a block tail shorter than the header is zero-filled,
    log_writer.cc:91-100), so every header is one the reader's chain reaches"""

    def __init__(self, recyclable, log_number=7, seed=1):
        self.rec, self.ln = recyclable, log_number
        self.buf = bytearray()
        self.rng = np.random.default_rng(seed)

    def data(self, n):
        return self.rng.integers(0, 256, n, np.uint8).tobytes()

    def put(self, t, payload=b"", log_number=None):
        """t in 1..4: Full / First / Middle / Last in this log's header kind;
        any other value is the type byte itself (9 always has the 7-byte
        header, 11 the 11-byte one, log_writer.cc:228-263)"""
        if isinstance(payload, int):
            payload = self.data(payload)
        if 1 <= t <= 4 and self.rec:
            t += 4
        hs = 11 if (5 <= t <= 8 or t == 11) else 7
        o = len(self.buf) % BLOCK
        if BLOCK - o < hs:
            self.buf += bytes(BLOCK - o)
            o = 0
        assert o + hs + len(payload) <= BLOCK
        h = bytearray(hs)
        h[4:6] = struct.pack("<H", len(payload))
        h[6] = t
        if hs == 11:
            h[7:11] = struct.pack("<I", self.ln if log_number is None else log_number)
        h[0:4] = struct.pack("<I", O.mask(O.crc32c_value(bytes(h[6:]) + payload)))
        at = len(self.buf)
        self.buf += h + payload
        return at

    def goto(self, target):
        """Full records up to block offset `target` (of this block or the next)"""
        hs = 11 if self.rec else 7
        while len(self.buf) % BLOCK != target:
            o = len(self.buf) % BLOCK
            if target >= o + hs:
                self.put(1, target - o - hs)
            elif BLOCK - o < hs:
                self.buf += bytes(BLOCK - o)
            else:
                self.put(1, BLOCK - o - hs)

    def array(self):
        return np.frombuffer(bytes(self.buf), np.uint8).copy()


def stop_and_fragment_cases(recyclable):
    """(name, log, log_number): small logs (<= 6 log blocks) for the outputs no
    scenario above reaches.

    Stop cases -- one cause of ReadRecord returning false per log, with no
    fragment open and right behind a First ("+open": the "error reading
    trailing data" paths), at the first byte of a block ("blk"), mid-block in
    a full block ("mid"), in the short last block ("last") and as the very
    first record ("first"): the log's end ("eof"), a truncated header ("hdr"),
    a truncated body ("body"), and kEof in front of the log's end from a
    record of the reader's own result type 12 ("p12"; types 14 and 16 are in
    the fixture logs); on recyclable headers an old record ("old": reading
    goes on in kSkipAnyCorruptedRecords) and, on the recycled log, a CRC and a
    length fault ("crc", "len": the tolerated corrupt tail of mode 0, reports
    in the others).  Every cause that does not need the log's end is followed
    by good records.

    Fragment-count cases ("frags", and "frags_x" with the same records laid
    across a block boundary): First First Last; First(empty) Middle Last; an
    empty record in one fragment and in three; five fragments; First control
    Last and First control control Middle Last with each control type, one
    control payload of exactly the Last's length; a fragmented record right
    after an aborted one (its XXH3 covers the aborted fragments, its count
    does not); a Middle and a Last with no start, then a good record.

    Empty and tiny logs: 0, 1..6, 7 and 11 bytes of a log, and 100 zero bytes
    (those under 7 bytes and the zeros with the legacy headers only: no type
    byte of theirs is read, log_reader.cc:454-461)."""
    ln = 7
    hs = 11 if recyclable else 7
    ts_type = 11 if recyclable else 10
    out = []
    eof_only = ("eof", "hdr", "body")
    causes = [("eof", ("blk", "last")), ("hdr", ("blk", "last")),
              ("body", ("blk", "last", "first")), ("p12", ("blk", "mid", "first"))]
    if recyclable:
        causes += [("crc", ("blk", "mid", "last", "first")), ("len", ("mid",)),
                   ("old", ("blk", "mid", "last", "first"))]
    for cause, places in causes:
        for pos in places:
            for open_ in (False, True):
                if open_ and pos == "first":
                    continue
                b = _Log(recyclable, ln, seed=len(out) + 1)
                lead = hs + 20 if open_ else 0  # the First in front of the cause
                if pos != "first":
                    b.put(1, 40)
                if pos == "blk":
                    b.goto((BLOCK - lead) % BLOCK)
                elif pos == "mid":
                    b.goto(9000)
                elif pos == "last":
                    b.goto(0)
                    b.put(1, 5)
                    b.goto(3000)
                if open_:
                    b.put(2, 20)
                if cause == "hdr":
                    b.buf += b.data(3)
                elif cause == "body":
                    at = b.put(1, 500)
                    del b.buf[at + hs + 100:]
                elif cause[0] == "p":
                    b.put(int(cause[1:]), 30)
                elif cause == "crc":
                    b.buf[b.put(1, 30) + hs + 4] ^= 0x20
                elif cause == "len":
                    at = b.put(1, 30)
                    b.buf[at + 4:at + 6] = b"\xff\xff"
                elif cause == "old":
                    b.put(1, 30, log_number=ln + 1)
                if cause not in eof_only:  # reading would go on: good records behind it
                    b.put(1, 10)
                    b.put(2, 33)
                    b.put(4, 44)
                    if pos != "last":  # (a full block: its faults are not the log's end)
                        b.goto(0)
                        b.put(2, 12)
                        b.put(4, 13)
                        b.put(1, 77)
                out.append((f"{cause}@{pos}" + ("+open" if open_ else ""), b.array(), ln))

    def ts(*pairs):
        return b"".join(struct.pack("<IH", cf, t) for cf, t in pairs)

    for name, start in (("frags", 0), ("frags_x", BLOCK - 60)):
        b = _Log(recyclable, ln, seed=77)
        b.put(1, 10)
        b.goto(start)
        b.put(2, 8), b.put(2, 9), b.put(4, 10)              # First First Last
        b.put(2, 0), b.put(3, 7), b.put(4, 3)               # First(empty) Middle Last
        b.put(1, 0)                                         # empty, one fragment
        b.put(2, 0), b.put(3, 0), b.put(4, 0)               # empty, three fragments
        b.put(2, 5), b.put(3, 300), b.put(3, 0), b.put(3, 17), b.put(4, 6)  # five fragments
        cf = 100
        for c in (9, ts_type):
            def ctl(n_pairs=1):
                nonlocal cf
                cf += n_pairs
                return struct.pack("<I", 0) if c == 9 else \
                    ts(*[(cf - k, 8) for k in range(n_pairs)])
            b.put(2, 12), b.put(c, ctl()), b.put(4, 15)     # First control Last
            b.put(2, 12), b.put(c, ctl()), b.put(c, ctl()), b.put(3, 9), b.put(4, 21)
            p = ctl(2)                                       # ... the Last as long as the control
            b.put(2, 12), b.put(c, p), b.put(4, len(p))
        b.put(2, 30), b.put(3, 10), b.put(30, 4)            # aborted by an unknown type ...
        b.put(2, 5), b.put(4, 6)                            # ... its XXH3 state still fed
        b.put(3, 9), b.put(4, 9), b.put(1, 20)              # no start, no start, good
        b.put(2, 4000), b.put(3, 2), b.put(4, 1)
        out.append((name, b.array(), ln))

    one = _Log(recyclable, ln, seed=5)
    one.put(1, 20)
    whole = one.array()
    for n in (7, 11) if recyclable else (0, 1, 2, 3, 4, 5, 6, 7, 11):
        out.append((f"len{n}", whole[:n].copy(), ln))
    if not recyclable:
        out.append(("zeros", np.zeros(100, np.uint8), ln))
    return out
