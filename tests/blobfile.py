"""tests/blobfile.py -- TEST INFRASTRUCTURE ONLY: a CPU restatement of the blob
file format (db/blob/blob_log_format.h/.cc), of the per-record verify and
writer calls of the engine (forst_blob_verify_batch, forst_blob_record_crc_batch)
and of the file scan (forst_blob_verify_files), on top of the oracle's CRC32C.

File: BlobLogHeader (30 B) | records | BlobLogFooter (32 B).
Record: key_size u64 | value_size u64 | expiration u64 | header_crc u32 |
blob_crc u32 | key | value, header_crc = Mask(Value(header[0..24))), blob_crc =
Mask(Value(key || value)).
"""
import struct

import numpy as np

from oracle import oracle as O

MAGIC = 2395959  # blob_log_format.h:20
VERSION1 = 1
FILE_HDR, FOOTER, REC_HDR = 30, 32, 32

# per-record status (include/forst_checksum.h FORST_BLOB_*)
OK, HEADER_CRC, KEY_SIZE, VALUE_SIZE, KEY, CRC, OUT_OF_RANGE, TOO_LARGE = range(8)
RECORD_TEXT = {  # Status::ToString() of the codes with a reference twin
    OK: "OK",
    HEADER_CRC: "Corruption: Error while decoding blob record: Header CRC mismatch",
    KEY_SIZE: "Corruption: Key size mismatch when reading blob",
    VALUE_SIZE: "Corruption: Value size mismatch when reading blob",
    KEY: "Corruption: Key mismatch when reading blob",
    CRC: "Corruption: Blob CRC mismatch",
}

# file reasons (enum forst_blob_file_reason)
(F_OK, F_MALFORMED, F_HEADER_MAGIC, F_HEADER_VERSION, F_TTL, F_CF_MISMATCH, F_FOOTER_MAGIC,
 F_FOOTER_CRC, F_RECORD_HEADER_CRC, F_RECORD_BLOB_CRC, F_RECORD_CROSSES_FOOTER,
 F_BLOB_COUNT_MISMATCH, F_RECORD_TOO_LARGE) = range(13)
FILE_TEXT = {
    F_OK: "OK",
    F_MALFORMED: "Corruption: Malformed blob file",
    F_HEADER_MAGIC: "Corruption: Error while decoding blob log header: Magic number mismatch",
    F_HEADER_VERSION: "Corruption: Error while decoding blob log header: Unknown header version",
    F_TTL: "Corruption: Unexpected TTL blob file",
    F_CF_MISMATCH: "Corruption: Column family ID mismatch",
    F_FOOTER_MAGIC: "Corruption: Error while decoding blob log footer: Magic number mismatch",
    F_FOOTER_CRC: "Corruption: Error while decoding blob log footer: CRC mismatch",
    F_RECORD_HEADER_CRC: RECORD_TEXT[HEADER_CRC],
    F_RECORD_BLOB_CRC: RECORD_TEXT[CRC],
    F_RECORD_CROSSES_FOOTER: "Corruption: Blob record crosses the blob file footer",
    F_BLOB_COUNT_MISMATCH: "Corruption: Blob count mismatch between the footer and the records",
    F_RECORD_TOO_LARGE: "Corruption: Blob record larger than 4 GiB",
}
NO_INDEX = 2**64 - 1


def mask32(c):
    """crc32c::Mask (util/crc32c.h:33) of a uint32 array"""
    c = np.asarray(c, np.uint64)
    return ((((c >> np.uint64(15)) | (c << np.uint64(17))) + np.uint64(0xA282EAD8))
            & np.uint64(0xFFFFFFFF)).astype(np.uint32)


# ---- build ------------------------------------------------------------------

def record(key, value, expiration=0, key_size=None, value_size=None):
    """BlobLogRecord::EncodeHeaderTo + key + value (key_size / value_size: the
    header's fields when they are to differ from the bytes that follow)"""
    ks = len(key) if key_size is None else key_size
    vs = len(value) if value_size is None else value_size
    head = struct.pack("<QQQ", ks, vs, expiration)
    hcrc = O.mask(O.crc32c_value(head))
    bcrc = O.mask(O.crc32c_value(bytes(key) + bytes(value)))
    return head + struct.pack("<II", hcrc, bcrc) + bytes(key) + bytes(value)


def file_header(cf=0, compression=0, has_ttl=False, exp_range=(0, 0), magic=MAGIC,
                version=VERSION1):
    return struct.pack("<IIIBBQQ", magic, version, cf, 1 if has_ttl else 0, compression,
                       *exp_range)


def file_footer(blob_count, exp_range=(0, 0), magic=MAGIC):
    body = struct.pack("<IQQQ", magic, blob_count, *exp_range)
    return body + struct.pack("<I", O.mask(O.crc32c_value(body)))


def build_file(kvs, cf=0, compression=0, expirations=None):
    """-> (file bytes, record header offsets)"""
    out, offs = bytearray(file_header(cf, compression)), []
    for i, (k, v) in enumerate(kvs):
        offs.append(len(out))
        out += record(k, v, 0 if expirations is None else expirations[i])
    out += file_footer(len(kvs))
    return bytes(out), offs


# ---- records ----------------------------------------------------------------

def _decode(buf, base_len, offsets):
    """header fields of every record whose 32 header bytes lie in [0, base_len)"""
    offs = np.asarray(offsets, np.uint64)
    n = len(offs)
    inr = (offs <= np.uint64(base_len)) & (np.uint64(base_len) - np.minimum(offs, np.uint64(base_len))
                                           >= np.uint64(REC_HDR))
    heads = np.zeros((n, REC_HDR), np.uint8)
    idx = np.nonzero(inr)[0]
    if len(idx):
        heads[idx] = buf[offs[idx].astype(np.int64)[:, None] + np.arange(REC_HDR)]
    f64 = heads[:, :24].copy().view("<u8")
    f32 = heads[:, 24:].copy().view("<u4")
    return inr, heads, f64[:, 0], f64[:, 1], f32[:, 0], f32[:, 1]


def _header_crcs(heads, nthreads):
    h24 = np.ascontiguousarray(heads[:, :24]).reshape(-1)
    n = len(heads)
    return mask32(O.crc32c_batch(h24, np.arange(n, dtype=np.uint64) * np.uint64(24),
                                 np.full(n, 24, np.uint32), nthreads=nthreads))


def _sizes(st, inr, ks, vs, offs, base_len):
    """TOO_LARGE, then the payload's OUT_OF_RANGE, for the records still OK
    -> (status, payload length where hashed)"""
    ks_i = [int(x) for x in ks]
    vs_i = [int(x) for x in vs]
    plen = np.zeros(len(st), np.uint32)
    for i in np.nonzero(st == OK)[0]:
        s = ks_i[i] + vs_i[i]
        if s > 0xFFFFFFFF:
            st[i] = TOO_LARGE
        elif s > base_len - int(offs[i]) - REC_HDR:
            st[i] = OUT_OF_RANGE
        else:
            plen[i] = s
    return plen


def pack_keys(ukeys):
    """a list of user keys -> (one uint8 buffer, offsets u64)"""
    offs = np.zeros(len(ukeys), np.uint64)
    pos = 0
    for i, k in enumerate(ukeys):
        offs[i] = pos
        pos += len(k)
    return np.frombuffer(b"".join(bytes(k) for k in ukeys) + b"\0", np.uint8)[:max(pos, 1)].copy(), offs


def _keys_differ(buf, koff, klen, ubuf, uoff):
    """record.key != user_key per record: keys of klen bytes at buf[koff] and at
    ubuf[uoff] (a user key that reaches past ubuf differs)"""
    n = len(klen)
    differ = (uoff > len(ubuf)) | (klen > len(ubuf) - np.minimum(uoff, len(ubuf)))
    lens = np.where(differ, 0, klen)
    starts = np.cumsum(lens) - lens
    within = np.arange(int(lens.sum())) - np.repeat(starts, lens)
    neq = buf[np.repeat(koff, lens) + within] != ubuf[np.repeat(uoff, lens) + within]
    nz = lens > 0
    if nz.any():
        differ[nz] |= np.add.reduceat(neq.astype(np.int64), starts[nz]) > 0
    assert len(differ) == n
    return differ


def verify_records(buf, offsets, expect_ks=None, expect_vs=None, user_keys=None, base_len=None,
                   nthreads=1):
    """forst_blob_verify_batch: -> (status u8, header_crc u32, blob_crc u32).
    user_keys: a list of bytes (one per record) or (packed uint8 buffer, offsets
    u64), with expect_ks."""
    buf = np.ascontiguousarray(buf, np.uint8)
    base_len = len(buf) if base_len is None else base_len
    offs = np.asarray(offsets, np.uint64)
    n = len(offs)
    inr, heads, ks, vs, hc, bc = _decode(buf, base_len, offs)
    st = np.where(inr, OK, OUT_OF_RANGE).astype(np.uint8)
    hcrc = np.where(inr, _header_crcs(heads, nthreads), 0).astype(np.uint32) if n else \
        np.zeros(0, np.uint32)
    st[(st == OK) & (hcrc != hc)] = HEADER_CRC
    if expect_ks is not None:
        st[(st == OK) & (ks != np.asarray(expect_ks, np.uint64))] = KEY_SIZE
    if expect_vs is not None:
        st[(st == OK) & (vs != np.asarray(expect_vs, np.uint64))] = VALUE_SIZE
    plen = _sizes(st, inr, ks, vs, offs, base_len)
    hashed = st == OK
    if user_keys is not None:
        kb, ko = user_keys if isinstance(user_keys, tuple) else pack_keys(user_keys)
        idx = np.nonzero(st == OK)[0]
        differ = _keys_differ(buf, offs[idx].astype(np.int64) + REC_HDR, ks[idx].astype(np.int64),
                              kb, np.asarray(ko, np.uint64)[idx].astype(np.int64))
        st[idx[differ]] = KEY
    poff = np.where(hashed, offs + np.uint64(REC_HDR), 0).astype(np.uint64)
    comp = mask32(O.crc32c_batch(buf, poff, plen, nthreads=nthreads)) if n else np.zeros(0, np.uint32)
    st[(st == OK) & (comp != bc)] = CRC
    return st, hcrc, np.where(hashed, comp, 0).astype(np.uint32)


def write_records(buf, offsets, base_len=None, nthreads=1):
    """forst_blob_record_crc_batch: -> (buffer with both CRC fields filled in,
    status, header_crc, blob_crc)"""
    buf = np.ascontiguousarray(buf, np.uint8).copy()
    base_len = len(buf) if base_len is None else base_len
    offs = np.asarray(offsets, np.uint64)
    n = len(offs)
    inr, heads, ks, vs, _hc, _bc = _decode(buf, base_len, offs)
    st = np.where(inr, OK, OUT_OF_RANGE).astype(np.uint8)
    hcrc = np.where(inr, _header_crcs(heads, nthreads), 0).astype(np.uint32) if n else \
        np.zeros(0, np.uint32)
    plen = _sizes(st, inr, ks, vs, offs, base_len)
    ok = st == OK
    poff = np.where(ok, offs + np.uint64(REC_HDR), 0).astype(np.uint64)
    comp = mask32(O.crc32c_batch(buf, poff, plen, nthreads=nthreads)) if n else np.zeros(0, np.uint32)
    bcrc = np.where(ok, comp, 0).astype(np.uint32)
    for i in np.nonzero(ok)[0]:
        o = int(offs[i])
        buf[o + 24:o + 32] = np.frombuffer(struct.pack("<II", int(hcrc[i]), int(bcrc[i])), np.uint8)
    return buf, st, hcrc, bcrc


# ---- file scan --------------------------------------------------------------

def walk_file(data, expect_cf=None):
    """the host walk (blob_host.h walk_file) -> dict: reason (host-decided, or
    F_OK), offsets, tail_crosses, trailing, end_pos, footer_blob_count,
    footer_ttl, cf, compression, has_ttl, total_blob_bytes"""
    size = len(data)
    w = dict(reason=F_OK, offsets=[], tail_crosses=False, trailing=False, end_pos=0,
             footer_blob_count=0, footer_ttl=False, cf=0, compression=0, has_ttl=0,
             total_blob_bytes=0)
    if size < FILE_HDR + FOOTER:
        return dict(w, reason=F_MALFORMED)
    magic, version, cf, flags, comp, e0, e1 = struct.unpack_from("<IIIBBQQ", data, 0)
    if magic != MAGIC:
        return dict(w, reason=F_HEADER_MAGIC)
    if version != VERSION1:
        return dict(w, reason=F_HEADER_VERSION)
    w.update(cf=cf, compression=comp, has_ttl=flags & 1)
    if flags & 1 or e0 or e1:
        return dict(w, reason=F_TTL)
    if expect_cf is not None and cf != expect_cf:
        return dict(w, reason=F_CF_MISMATCH)
    foot = size - FOOTER
    fmagic, count, f0, f1 = struct.unpack_from("<IQQQ", data, foot)
    if fmagic != MAGIC:
        return dict(w, reason=F_FOOTER_MAGIC)
    w.update(footer_blob_count=count, footer_ttl=bool(f0 or f1))
    pos = FILE_HDR
    while pos < foot:
        if foot - pos < REC_HDR:
            w["trailing"] = True
            break
        ks, vs = struct.unpack_from("<QQ", data, pos)
        w["offsets"].append(pos)
        if ks + vs > foot - pos - REC_HDR:
            w["tail_crosses"] = True
            break
        w["total_blob_bytes"] += REC_HDR + ks + vs
        pos += REC_HDR + ks + vs
    w["end_pos"] = pos
    return w


def scan_file(data, expect_cf=None):
    """forst_blob_verify_files over one file -> dict(status, reason, text,
    fail_index, fail_offset, blob_count, total_blob_bytes, cf, compression,
    has_ttl)"""
    data = bytes(data)
    w = walk_file(data, expect_cf)
    offs = w["offsets"]
    r = dict(reason=w["reason"], fail_index=NO_INDEX, fail_offset=0,
             blob_count=len(offs) - (1 if w["tail_crosses"] else 0),
             total_blob_bytes=w["total_blob_bytes"], cf=w["cf"], compression=w["compression"],
             has_ttl=w["has_ttl"])

    def done():
        r["status"] = 0 if r["reason"] == F_OK else 2
        r["text"] = FILE_TEXT[r["reason"]]
        return r

    if r["reason"] != F_OK:
        r["blob_count"] = r["total_blob_bytes"] = 0
        return done()
    foot = len(data) - FOOTER
    if O.mask(O.crc32c_value(data[foot:foot + 28])) != struct.unpack_from("<I", data, foot + 28)[0]:
        r["reason"] = F_FOOTER_CRC
        return done()
    if w["footer_ttl"]:
        r["reason"] = F_TTL
        return done()
    buf = np.frombuffer(data, np.uint8)
    st, _, _ = verify_records(buf, np.array(offs, np.uint64)) if offs else (np.zeros(0, np.uint8), 0, 0)
    for k, o in enumerate(offs):
        last_crosses = w["tail_crosses"] and k + 1 == len(offs)
        reason = F_OK
        if st[k] == HEADER_CRC:
            reason = F_RECORD_HEADER_CRC
        elif last_crosses:
            reason = F_RECORD_CROSSES_FOOTER
        elif st[k] == CRC:
            reason = F_RECORD_BLOB_CRC
        elif st[k] == TOO_LARGE:
            reason = F_RECORD_TOO_LARGE
        elif st[k] != OK:
            reason = F_RECORD_CROSSES_FOOTER
        if reason != F_OK:
            r.update(reason=reason, fail_index=k, fail_offset=o, blob_count=k,
                     total_blob_bytes=o - FILE_HDR)
            return done()
    if w["trailing"]:
        r.update(reason=F_RECORD_CROSSES_FOOTER, fail_index=len(offs), fail_offset=w["end_pos"])
        return done()
    if len(offs) != w["footer_blob_count"]:
        r["reason"] = F_BLOB_COUNT_MISMATCH
    return done()


# ---- the recorded reference answers (tests/golden/blob_files.json) -------------

NO_TWIN = {F_RECORD_CROSSES_FOOTER, F_BLOB_COUNT_MISMATCH, F_RECORD_TOO_LARGE}


def apply_damage(data, d):
    """a damaged copy of a fixture file: one XOR mask at a byte offset, or a
    truncation"""
    if d["kind"] == "truncate":
        return data[:d["size"]]
    b = bytearray(data)
    b[d["offset"]] ^= d["mask"]
    return bytes(b)


def check_against_reference(d, text, fail_index, reason):
    """a file scan's outcome (Status string, first failing record, reason)
    against what the reference said about the same damaged copy:
    BlobFileReader::Create's Status where it fails, else the sequential
    reader's first failing record.  Where the reference's reader runs into the
    end of the file (it does not know where the footer starts), the scan must
    give one of its reasons without a reference twin."""
    if d["create_status"] != "OK":
        assert text == d["create_status"] and fail_index == NO_INDEX, (d, text, fail_index)
    elif d["seq_fail"] is None:
        assert d["seq_footer"] == "OK" and text == "OK" and fail_index == NO_INDEX, (d, text)
    elif "EOF reached" in d["seq_fail"]:
        assert reason in NO_TWIN, (d, text)
    else:
        assert text == d["seq_fail"] and fail_index == d["seq_ok_records"], (d, text, fail_index)


def request_inputs(req, data):
    """a recorded GetBlob request in the engine's terms -> (file bytes, record
    offset, expected key size, expected value size, user key).  The record
    offset is the BlobIndex offset minus
    BlobLogRecord::CalculateAdjustmentForRecordHeader(key_size)."""
    if req["flip"] is not None:
        data = apply_damage(data, dict(kind="xor", offset=req["flip"][0], mask=req["flip"][1]))
    key = bytes.fromhex(req["key"])
    return data, req["value_offset"] - REC_HDR - len(key), len(key), req["value_size"], key
