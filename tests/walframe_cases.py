"""tests/walframe_cases.py -- TEST INFRASTRUCTURE ONLY: the cases of
forst_wal_frame_batch (forst_amd/csrc/wal_frame.h) that
tests/test_emu_wal_frame.py runs on the SIMT emulator and
tests/test_gpu_wal_frame.py on the device.

The expected image is oracle.wal_frame (pinned to the reference's log::Writer
by tests/test_wal_writer_golden.py); for a writer that stands at block_offset
b the records [b - hs] + lens are framed and the image is cut at b.  The
physical-record arrays are checked against forst_wal_layout_at (a host
utility of the product library, no GPU call).  Every output is handed over
prefilled with the sentinels of tests/dispatch.py, GUARD cells longer than
needed, and compared whole -- the image cells behind image_bytes included.

The runners are those of tests/walcompact_cases.py (up(array) -> a handle with
.ptr and .host()).
"""
import ctypes

import numpy as np

import walcompact_cases as C
from forst_amd import _lib
from oracle import oracle as O

GUARD = C.GUARD
S8, S32, S64 = C.S8, C.S32, C.S64
BLOCK = 32768
EINVAL = -1
PIECE, TILE, WINDOW = 16, 16384, 1023  # wal_frame.h (wal_compact.h's constants)


class FrameResult(ctypes.Structure):
    _fields_ = [("image_bytes", ctypes.c_uint64), ("n_physical", ctypes.c_uint64),
                ("n_pads", ctypes.c_uint64), ("bad_records", ctypes.c_uint64),
                ("end_block_offset", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def bind(L):
    vp, u64, u32, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    C.bind(L)
    L.forst_wal_frame_batch.restype = i
    L.forst_wal_frame_batch.argtypes = [vp, u64, vp, vp, vp, u64, i, u32, u32, vp, u64, vp, vp, vp,
                                        vp, u64, vp, vp, vp]
    L.forst_wal_verify_batch.restype = i
    L.forst_wal_verify_batch.argtypes = [vp, u64, u64, u64, u32, vp, vp, vp, vp, vp]
    return L


def runner(run):
    bind(run.L)
    return run


def hsize(recyclable):
    return 11 if recyclable else 7


# ---- the oracle -------------------------------------------------------------------

def layout_at(lens, recyclable, b):
    """forst_wal_layout_at: (offsets, lengths, types, total, n_pads, end_block_offset)"""
    L = _lib.lib()
    lens = np.ascontiguousarray(lens, np.uint32)
    n = len(lens)
    nph, npad, tot = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    end = ctypes.c_uint32()
    rc = L.forst_wal_layout_at(lens.ctypes.data, n, int(recyclable), b, None, None, None, 0, None,
                               None, 0, ctypes.byref(nph), ctypes.byref(npad), ctypes.byref(tot),
                               ctypes.byref(end))
    assert rc == 0
    k = nph.value
    po, pl, pt = np.zeros(k, np.uint64), np.zeros(k, np.uint32), np.zeros(k, np.uint8)
    rc = L.forst_wal_layout_at(lens.ctypes.data, n, int(recyclable), b, po.ctypes.data,
                               pl.ctypes.data, pt.ctypes.data, k, None, None, npad.value,
                               ctypes.byref(nph),
                               ctypes.byref(npad), ctypes.byref(tot), ctypes.byref(end))
    assert rc == 0
    return po, pl, pt, tot.value, npad.value, end.value


def oracle_image(payloads, recyclable, log_number, b):
    """what log::Writer appends for the payloads from block_offset b"""
    hs = hsize(recyclable)
    lens = [len(p) for p in payloads]
    if b:
        assert hs <= b <= BLOCK
        lens = [b - hs] + lens
        payloads = [bytes(b - hs)] + list(payloads)
    pay = np.frombuffer(b"".join(payloads), np.uint8)
    img = O.wal_frame(pay, np.array(lens, np.uint32), recyclable=recyclable,
                      log_number=log_number)[0]
    return img[b:].copy()


def stage(reps, order=None):
    """the reps back to back in one buffer (no rounding: every source alignment
    occurs), laid down in `order` when given -> (base, offsets, sizes) in rep
    order; base ends at the last byte of the rep laid down last"""
    n = len(reps)
    order = range(n) if order is None else order
    offs = np.zeros(n, np.uint64)
    at = 0
    for i in order:
        offs[i] = at
        at += len(reps[i])
    base = np.frombuffer(b"".join(reps[i] for i in order), np.uint8)
    return base.copy(), offs, np.array([len(r) for r in reps], np.uint32)


def random_reps(lens, seed):
    rng = np.random.default_rng(seed)
    # (1..255: a zero-filled payload of a bad rep differs from every good byte)
    data = rng.integers(1, 256, int(np.asarray(lens, np.int64).sum()), np.uint8).tobytes()
    out, at = [], 0
    for n in lens:
        out.append(data[at:at + int(n)])
        at += int(n)
    return out


# ---- the call ---------------------------------------------------------------------

class Result:
    pass


OUTS = ("rec_offsets", "phys_offsets", "phys_lengths", "phys_types", "status")


def frame(run, base, offs, sizes, recyclable, log_number=7, b=0, capacity="fit", nulls=(),
          host_sizes=True, base_h=None, base_len=None, image_h=None, phys_cap=None):
    """one forst_wal_frame_batch call -> Result with rc, the result struct and
    the whole output arrays (None where NULL was passed).  capacity: "fit" (an
    image of exactly the layout's total), None (count-only: image NULL,
    capacity 0) or a number (an image of that many bytes + GUARD pieces)."""
    n = len(offs)
    sizes = np.ascontiguousarray(sizes, np.uint32)
    lay = layout_at(sizes, recyclable, b)
    nph = len(lay[0])
    if capacity == "fit":
        capacity = lay[3]
    phys_cap = nph if phys_cap is None else phys_cap
    off_h, sz_h = run.up(np.asarray(offs, np.uint64)), run.up(sizes)
    base_h = base_h or run.up(base if len(base) else np.zeros(4, np.uint8))
    base_len = len(base) if base_len is None else base_len
    outs = {"rec_offsets": run.up(np.full(n + GUARD, S64, np.uint64)),
            "phys_offsets": run.up(np.full(phys_cap + GUARD, S64, np.uint64)),
            "phys_lengths": run.up(np.full(phys_cap + GUARD, S32, np.uint32)),
            "phys_types": run.up(np.full(phys_cap + GUARD, S8, np.uint8)),
            "status": run.up(np.full(n + GUARD, S8, np.uint8))}
    for k in nulls:
        outs[k] = None
    if image_h is None and capacity is not None:
        image_h = run.up(np.full(capacity + GUARD * PIECE, S8, np.uint8))
    res = FrameResult()
    ctypes.memset(ctypes.byref(res), 0x5A, ctypes.sizeof(res))
    rc = run.L.forst_wal_frame_batch(
        base_h.ptr, base_len, off_h.ptr, sz_h.ptr, sizes.ctypes.data if host_sizes else None, n,
        int(recyclable), log_number, b, C._ptr(image_h), 0 if capacity is None else capacity,
        C._ptr(outs["rec_offsets"]), C._ptr(outs["phys_offsets"]), C._ptr(outs["phys_lengths"]),
        C._ptr(outs["phys_types"]), phys_cap, C._ptr(outs["status"]), ctypes.byref(res), None)
    r = Result()
    r.rc, r.res, r.layout = rc, res, lay
    r.image = None if image_h is None else image_h.host()
    for k, h in outs.items():
        setattr(r, k, None if h is None else h.host())
    r.base_h, r.image_h = base_h, image_h
    return r


def _same(what, name, got, want, sent):
    if got is None:
        return
    bad = np.nonzero(got[:len(want)] != want)[0]
    assert bad.size == 0, (what, name, int(bad.size), bad[:8].tolist(), got[bad[:8]].tolist(),
                           np.asarray(want)[bad[:8]].tolist())
    assert (got[len(want):] == sent).all(), (what, name, "stored past its end")


def check(r, reps, recyclable, log_number=7, b=0, status=None, what="", image=True):
    """a Result against the writer's image and forst_wal_layout_at, every cell
    of every array; a rep with status 1 is framed as zeros"""
    n = len(reps)
    st = np.zeros(n, np.uint8) if status is None else np.asarray(status, np.uint8)
    po, pl, pt, total, npad, end = r.layout
    assert r.rc == 0, (what, r.rc)
    assert (r.res.image_bytes, r.res.n_physical, r.res.n_pads, r.res.end_block_offset,
            r.res.bad_records) == (total, len(po), npad, end, int(st.sum())), what
    types = np.where(pt > 4, pt - 4, pt)
    _same(what, "rec_offsets", r.rec_offsets, po[(types == 1) | (types == 2)], S64)
    _same(what, "phys_offsets", r.phys_offsets, po, S64)
    _same(what, "phys_lengths", r.phys_lengths, pl, S32)
    _same(what, "phys_types", r.phys_types, pt, S8)
    _same(what, "status", r.status, st, S8)
    if image and r.image is not None:
        pay = [bytes(len(p)) if st[i] else p for i, p in enumerate(reps)]
        want = oracle_image(pay, recyclable, log_number, b)
        assert len(want) == total, (what, len(want), total)
        _same(what, "image", r.image, want, S8)


def frame_check(run, reps, recyclable, b=0, what="", order=None, up_base=None, **kw):
    base, offs, sizes = stage(reps, order)
    base_h = up_base(base) if up_base and len(base) else None
    r = frame(run, base, offs, sizes, recyclable, b=b, base_h=base_h, **kw)
    check(r, reps, recyclable, b=b, what=what)
    return r, base, offs, sizes


# ---- the cases, as the two test files run them ------------------------------------

def case_length_sweep(run, recyclable):
    """lengths 0..300 at block_offset 0, hs, 5000 and 32768: a header at every
    offset mod 16 (asserted), mixed pieces with one to three headers"""
    hs = hsize(recyclable)
    reps = random_reps(range(301), 3)
    for b in (0, hs, 5000, BLOCK):
        r, _, _, _ = frame_check(run, reps, recyclable, b=b, what=("sweep", b))
        assert set((r.phys_offsets[:r.res.n_physical] % 16).tolist()) == set(range(16))
    # ... and 40 empty or tiny records: three headers in one piece
    tiny = random_reps([0, 0, 0, 1, 0, 0, 2, 0, 0, 0] * 4, 4)
    for b in (0, hs, 5000, BLOCK - hs - 2):
        frame_check(run, tiny, recyclable, b=b, what=("tiny", b))


def edge_lengths(recyclable):
    c = BLOCK - hsize(recyclable)
    return (c - 1, c, c + 1, 2 * c, 2 * c + 1, 3 * c + 5)


def _advance(bo, n, hs):
    """Writer::block_offset_ behind a record of n bytes added at bo"""
    if BLOCK - bo < hs:
        bo = 0
    pay0 = BLOCK - bo - hs
    if n <= pay0:
        return bo + hs + n
    rest, per = n - pay0, BLOCK - hs
    return hs + rest - (-(-rest // per) - 1) * per


def block_edge_group(recyclable, leftovers):
    """[pad record, record] pairs: the pad record ends where the writer has
    `leftover` bytes left in its block, for every leftover given and every
    length of edge_lengths -> (lens, the indices of the edge records)"""
    hs = hsize(recyclable)
    lens, at, bo = [], [], 0
    for left in leftovers:
        for n in edge_lengths(recyclable):
            pad = (BLOCK - left) - bo - hs
            if BLOCK - bo < hs or pad < 0:
                if BLOCK - bo >= hs:  # a record that ends at the block's end first
                    lens.append(BLOCK - bo - hs)
                pad = (BLOCK - left) - hs
                bo = 0
            lens.append(pad)
            bo = _advance(bo, pad, hs)
            assert BLOCK - bo == left
            at.append(len(lens))
            lens.append(n)
            bo = _advance(bo, n, hs)
    return lens, at


def case_block_edges(run, recyclable, leftovers=None):
    """a record starting with 0..hs+17 bytes left in its block (1..hs-1: the
    zero pad; hs: the empty First fragment), of lengths around one, two and
    three blocks; a record ending at a block end, then an empty one"""
    hs = hsize(recyclable)
    leftovers = list(range(hs + 18)) if leftovers is None else leftovers
    lens, at = block_edge_group(recyclable, leftovers)
    po, pl, pt, _, npad, _ = layout_at(lens, recyclable, 0)
    # the group is what it claims, by forst_wal_layout_at: a pad per leftover
    # 1..hs-1 and edge length, an empty First fragment per edge length
    k = len(edge_lengths(recyclable))
    t = np.where(pt > 4, pt - 4, pt)
    first = po[(t == 1) | (t == 2)]
    assert npad >= k * len([x for x in leftovers if 0 < x < hs])
    if hs in leftovers:
        assert int(((pl == 0) & (t == 2)).sum()) >= k
    for i, left in zip(at, np.repeat(leftovers, k)):
        o = int(first[i]) % BLOCK
        assert o == (BLOCK - left if left >= hs else 0), (i, left, o)
    frame_check(run, random_reps(lens, 5), recyclable, what="block edges")
    # a record that ends exactly at a block end, then an empty record
    for b in (0, 5000):
        frame_check(run, random_reps([BLOCK - b - hs, 0, 9, 2 * (BLOCK - hs) - (2 * hs + 9), 0], 6),
                    recyclable, b=b, what=("block end", b))


def case_tiles_and_windows(run, part):
    if part == "empty":
        # 3000 empty records: more than 1023 in one 16 KiB tile, the LDS window slides
        assert 3000 * 7 > TILE and TILE // 7 > 2 * WINDOW
        for recyclable in (False, True):
            frame_check(run, [b""] * 3000, recyclable, what="empty")
    elif part == "1009":
        frame_check(run, random_reps([1009] * 70, 7), False, b=5000, what="1009")
        frame_check(run, random_reps([1009] * 70, 7), True, what="1009r")
    elif part == "many":
        rng = np.random.default_rng(12)
        lens = rng.integers(0, 41, 66000)
        assert len(lens) > 65536
        frame_check(run, random_reps(lens, 8), False, what="many")
    else:
        frame_check(run, random_reps([5, (1 << 20) + 1, 3], 9), True, b=777, what="1 MiB + 1")


def case_source(run, recyclable, up_base=None):
    """every source alignment, the reps in reverse order in base, base ending
    at the last rep's last byte (up_base: in front of an inaccessible page)"""
    lens = list(range(0, 70)) + [16, 17, 31, 32, 33, 4096, 40000, 1, 20, 19]
    reps = random_reps(lens, 10)
    base, offs, sizes = stage(reps)
    seen = {(int(o) % 16) for o, s in zip(offs, sizes) if s >= 16}
    assert seen == set(range(16))
    r = frame(run, base, offs, sizes, recyclable, b=100,
              base_h=up_base(base) if up_base else None)
    check(r, reps, recyclable, b=100, what="aligned")
    n = len(reps)
    frame_check(run, reps, recyclable, what="reversed", order=range(n - 1, -1, -1),
                up_base=up_base)
    # short bases: the byte path of the last 20 bytes is all there is
    for k in (1, 3, 16, 19, 20, 21, 35):
        frame_check(run, random_reps([k], 11), recyclable, what=("short", k), up_base=up_base)
        frame_check(run, random_reps([0, k], 11), recyclable, what=("short2", k), up_base=up_base)


def case_out_of_range(run, recyclable, up_base=None):
    """reps that reach past base_len: status 1, a zero payload under valid
    CRCs, the neighbours intact"""
    lens = [30, 100, 0, 40000, 17, 5, 0, 64]
    reps = random_reps(lens, 13)
    base, offs, sizes = stage(reps)
    n_base = len(base)
    offs = offs.copy()
    status = np.zeros(len(reps), np.uint8)
    offs[1] = n_base - 99          # one byte past the end
    offs[3] = n_base - 10          # far past
    offs[5] = 2**64 - 3            # offset + size wraps
    offs[6] = n_base + 1           # an empty rep behind the end
    offs[7] = n_base               # at the end, 64 bytes
    status[[1, 3, 5, 6, 7]] = 1
    r = frame(run, base, offs, sizes, recyclable, b=BLOCK - 200,
              base_h=up_base(base) if up_base else None)
    check(r, reps, recyclable, b=BLOCK - 200, status=status, what="out of range")
    return r, reps, status


def verify_blocks(run, image_h, total, log_number):
    nb = (total + BLOCK - 1) // BLOCK
    st = run.up(np.full(nb, S8, np.uint8))
    bad = run.up(np.zeros(1, np.uint64))
    rc = run.L.forst_wal_verify_batch(image_h.ptr, total, 0, nb, log_number, st.ptr, None, None,
                                      bad.ptr, None)
    assert rc == 0, run.L.forst_last_error()
    return st.host(), int(bad.host()[0])


def case_contracts(run):
    reps = random_reps([10, 0, 40000, 16, 17, 300, 0], 4)
    base, offs, sizes = stage(reps)
    n = len(reps)
    total = layout_at(sizes, False, 0)[3]
    # count-only: the result and the descriptors, no image
    r = frame(run, base, offs, sizes, False, capacity=None)
    assert r.image is None
    check(r, reps, False, what="count-only")
    # exact fit and ample: bytes at and past image_bytes stay as they were
    check(frame(run, base, offs, sizes, True, b=11), reps, True, b=11, what="fit")
    check(frame(run, base, offs, sizes, False, capacity=total + 100), reps, False, what="ample")
    # one byte short (and shorter): FORST_EINVAL, image_bytes set, the image untouched
    for cap in (total - 1, total - 16, 16, 1, 0):
        r = frame(run, base, offs, sizes, False, capacity=cap,
                  image_h=run.up(np.full(GUARD * PIECE, S8, np.uint8)) if cap == 0 else None)
        assert r.rc == EINVAL and r.res.image_bytes == total, (cap, r.rc, r.res.image_bytes)
        assert (r.image == S8).all(), cap
        assert b"image_capacity" in run.L.forst_last_error()
    # every nullable output NULL in turn, and all of them
    for nulls in tuple((k,) for k in OUTS) + (OUTS,):
        for cap in ("fit", None):
            r = frame(run, base, offs, sizes, True, capacity=cap, nulls=nulls)
            assert all(getattr(r, k) is None for k in nulls)
            check(r, reps, True, what=(nulls, cap))
    # host_sizes NULL against given: identical output
    a = frame(run, base, offs, sizes, True, b=BLOCK - 5, host_sizes=True)
    b = frame(run, base, offs, sizes, True, b=BLOCK - 5, host_sizes=False)
    check(a, reps, True, b=BLOCK - 5, what="host sizes")
    check(b, reps, True, b=BLOCK - 5, what="no host sizes")
    for k in OUTS + ("image",):
        assert (getattr(a, k) == getattr(b, k)).all(), k
    # descriptor arrays shorter than the physical records: FORST_EINVAL, nothing written
    r = frame(run, base, offs, sizes, False, phys_cap=len(layout_at(sizes, False, 0)[0]) - 1)
    assert r.rc == EINVAL and b"phys_capacity" in run.L.forst_last_error()
    assert r.res.image_bytes == total and (r.image == S8).all()
    assert (r.phys_offsets == S64).all() and (r.status == S8).all()
    # no record: image_bytes = 0, nothing touched
    r = frame(run, base, offs[:0], sizes[:0], False, b=123, capacity=64)
    assert r.rc == 0 and r.res.image_bytes == 0 and r.res.n_physical == 0
    assert r.res.end_block_offset == 123
    assert (r.image == S8).all() and all((getattr(r, k) == s).all() for k, s in
                                         zip(OUTS, (S64, S64, S32, S8, S8)))
    # a block_offset forst_wal_layout_at rejects
    L = _lib.lib()
    for bo in (BLOCK + 1, 2**32 - 1):
        assert L.forst_wal_layout_at(sizes.ctypes.data, n, 0, bo, None, None, None, 0, None, None,
                                     0, None, None, None, None) == EINVAL
        r0 = FrameResult()
        for nn in (n, 0):
            h = run.up(base)
            rc = run.L.forst_wal_frame_batch(h.ptr, len(base), run.up(offs).ptr,
                                             run.up(sizes).ptr, sizes.ctypes.data, nn, 0, 7, bo,
                                             None, 0, None, None, None, None, 0, None,
                                             ctypes.byref(r0), None)
            assert rc == EINVAL and b"block_offset" in run.L.forst_last_error()
    assert L.forst_wal_layout_at(sizes.ctypes.data, n, 0, BLOCK, None, None, None, 0, None, None,
                                 0, None, None, None, None) == 0
    check(frame(run, base, offs, sizes, False, b=BLOCK), reps, False, b=BLOCK, what="b = 32768")
    # a misaligned image, an image that overlaps base
    whole = run.up(np.concatenate([base, np.full((-len(base)) % 16 + total + 64, S8, np.uint8)]))

    class Part:
        def __init__(self, at):
            self.ptr = whole.ptr + at

        def host(self):
            return whole.host()[self.ptr - whole.ptr:]

    at = (len(base) + 15) // 16 * 16  # right behind base: allowed
    for mis in (1, 4, 8):
        r = frame(run, base, offs, sizes, False, base_h=whole, image_h=Part(at + mis))
        assert r.rc == EINVAL and b"aligned" in run.L.forst_last_error(), mis
    for bad in (0, len(base) // 16 * 16 - 16, 16):
        r = frame(run, base, offs, sizes, False, base_h=whole, image_h=Part(bad))
        assert r.rc == EINVAL and b"overlap" in run.L.forst_last_error(), bad
    before = whole.host()
    r = frame(run, base, offs, sizes, False, base_h=whole, image_h=Part(at))
    assert r.rc == 0 and r.res.image_bytes == total
    after = whole.host()
    assert (after[at:at + total] == oracle_image(reps, False, 7, 0)).all()
    assert (after[:at] == before[:at]).all() and (after[at + total:] == before[at + total:]).all()


def roundtrip_group(recyclable):
    lens = [0, 5, 33000, 12, 300, 0, 70000, 1, 32768 - 2 * hsize(recyclable) - 5 - 33000 % 7, 250]
    return random_reps(lens, 15)


def case_roundtrip(run, recyclable, mode):
    """the image through forst_wal_recover_batch: n records, no report, the rep
    sizes, xxh3(rep); forst_wal_records_compact of it gives the reps back;
    forst_wal_verify_batch reports every block OK"""
    reps = roundtrip_group(recyclable)
    n = len(reps)
    base, offs, sizes = stage(reps)
    r = frame(run, base, offs, sizes, recyclable)
    check(r, reps, recyclable, what="roundtrip")
    total = r.res.image_bytes
    image = r.image[:total]
    cap = n + 8
    recs = [run.up(np.zeros(cap, t)) for t in (np.uint64, np.uint64, np.uint64, np.uint32)]
    rpts = [run.up(np.zeros(cap, t)) for t in (np.uint64, np.uint64, np.uint32, np.uint32)]
    res = C.WalRecoverResult()
    rc = run.L.forst_wal_recover_batch(r.image_h.ptr, total, 7, mode,
                                       C.WalRecords(*[h.ptr for h in recs]), cap,
                                       C.WalReports(*[h.ptr for h in rpts]), cap,
                                       ctypes.byref(res), None)
    assert rc == 0, run.L.forst_last_error()
    assert res.n_records == n and res.n_reports == 0 and not res.truncated
    off, length, hsh, nfrag = (h.host()[:n] for h in recs)
    assert (length == sizes).all()
    assert (hsh == np.array([O.xxh3_64(x) for x in reps], np.uint64)).all()
    assert (off == r.rec_offsets[:n]).all()
    if mode == 2:
        c = C.compact(run, image, off, length, nfrag, log_h=r.image_h, log_len=total)
        C.check(c, reps, what="compact of the image")
        st, bad = verify_blocks(run, r.image_h, total, 7)
        assert bad == 0 and (st == 0).all(), (st.tolist(), bad)


def case_chain(run, recyclable):
    """one staged base feeds forst_write_batch_protect_batch and the frame call"""
    log, reps = C.chain_log(recyclable)
    base, offs, sizes = stage(reps)
    base_h = run.up(base)
    r = frame(run, base, offs, sizes, recyclable, base_h=base_h)
    check(r, reps, recyclable, what="chain")
    assert (r.image[:r.res.image_bytes] == log).all()  # the log walcompact's chain recovers
    got = C.protect(run, base_h, len(base), offs, sizes)
    # ... against the reps 8-byte aligned, as KvProtection::Stage lays them out
    aoffs, img = [], bytearray()
    for rep in reps:
        aoffs.append(len(img))
        img += rep + bytes(-len(rep) % 8)
    img += bytes(16)
    want = C.protect(run, run.up(np.frombuffer(bytes(img), np.uint8)), len(img), aoffs, sizes)
    for name, g, w in zip(("prot", "first_entry", "status", "n_protected"), got, want):
        assert len(g) == len(w) and (g == w).all(), name
    assert len(got[0]) > 100 and len(set(got[2].tolist())) > 1  # good and malformed reps
    codes = [O.write_batch_protect(rep)[0] for rep in reps]
    assert (got[2] == np.array(codes, np.uint8)).all()


def case_appending(run, recyclable):
    """a group framed in three calls, each at the previous call's
    end_block_offset: the concatenation is the group framed in one call"""
    rng = np.random.default_rng(16)
    lens = rng.integers(0, 9000, 40)
    lens[[3, 17, 30]] = [40000, 32768 - hsize(recyclable), 70000]
    reps = random_reps(lens, 17)
    b0 = 20000
    whole, _, _, _ = frame_check(run, reps, recyclable, b=b0, what="whole")
    parts, b = [], b0
    for lo, hi in ((0, 10), (10, 18), (18, 40)):
        r, _, _, _ = frame_check(run, reps[lo:hi], recyclable, b=b, what=("part", lo))
        parts.append(r.image[:r.res.image_bytes])
        b = r.res.end_block_offset
    joined = np.concatenate(parts)
    assert len(joined) == whole.res.image_bytes and (joined == whole.image[:len(joined)]).all()
    assert b == whole.res.end_block_offset
