"""tests/kvsites.py -- TEST INFRASTRUCTURE: the a15 call-site cases of
tests/golden/kv_sites.{json,npz} (reference-made, gen_kv_golden.py) laid out
as the engine's batch calls take them: memtable entry buffers with their
corrupted copies, and the WriteBatch reps back to back."""
import functools
import json
import os
import struct

import numpy as np


def memtable_cases(meta, arrays):
    """-> [(name, base u8, entry offsets u64, prot_bytes, expected status texts)]
    intact buffers, one per protection size, then each buffer with ALL its
    corruptions applied at once (they hit distinct entries), then the crafted
    headers as one buffer"""
    out = []
    for c in meta["memtable"]["cases"]:
        base = arrays[c["tag"] + "_base"]
        offs = arrays[c["tag"] + "_offs"]
        out.append((c["tag"], base, offs, c["prot_bytes"], ["OK"] * c["n"]))
        b2 = base.copy()
        want = ["OK"] * c["n"]
        for x in c["corrupt"]:
            b2[x["at"]] ^= x["xor"]
            want[x["entry"]] = x["status"]
        out.append((c["tag"] + "_corrupt", b2, offs, c["prot_bytes"], want))
    parts, offs, want, pos = [], [], [], 0
    for x in meta["memtable"]["crafted"]:
        raw = bytes.fromhex(x["hex"])
        parts.append(raw)
        offs.append(pos)
        want.append(x["status"])
        pos += len(raw)
    out.append(("crafted", np.frombuffer(b"".join(parts) + bytes(64), np.uint8).copy(),
                np.array(offs, np.uint64), 8, want))
    return out


def write_batch_case(meta, arrays):
    """-> (base u8, rep offsets u64, rep sizes u32, [(name, status text, prot u64[])])"""
    reps = [(b["name"], b["status"], arrays[f"wb_prot_{i}"]) for i, b in enumerate(meta["writebatch"])]
    return arrays["wb_base"], arrays["wb_offs"], arrays["wb_lens"], reps


def wb_rep(rng, nrec, tags=None):
    """a WriteBatch rep (write_batch.cc record layout) of nrec random records;
    tags (a list): the record tags written are appended to it"""
    out = bytearray(struct.pack("<QI", int(rng.integers(0, 2**56)), 0))
    cnt = 0
    for _ in range(nrec):
        tag = int(rng.choice([0x01, 0x05, 0x00, 0x04, 0x07, 0x08, 0x02, 0x06, 0x0F, 0x0E, 0x11,
                              0x10, 0x16, 0x17, 0x03, 0x0D]))
        out.append(tag)
        if tags is not None:
            tags.append(tag)
        if tag in WB_CF_TAGS:
            cf = int(rng.integers(1, 300))
            while cf >= 128:
                out.append((cf & 127) | 128)
                cf >>= 7
            out.append(cf)
        parts = {0x03: 1, 0x0D: 0, 0x00: 1, 0x04: 1, 0x07: 1, 0x08: 1}.get(tag, 2)
        for p in range(parts):
            ln = int(rng.integers(0, 300 if p == 0 else 1500))
            v = ln
            while v >= 128:
                out.append((v & 127) | 128)
                v >>= 7
            out.append(v)
            out += rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
        cnt += tag not in (0x03, 0x0D)
    out[8:12] = struct.pack("<I", cnt)
    return bytes(out)


WB_OUT_OF_RANGE = 15  # include/forst_checksum.h: the rep reaches past base_len
WB_CF_TAGS = (0x05, 0x04, 0x08, 0x06, 0x0E, 0x10, 0x17)  # records with a column family varint
WB_KINDS = ("raise", "lower", "zero", "short", "cut", "past")
WB_SHORT = (0, 1, 11, 4, 8)  # lengths of the reps under the 12-byte header


def wb_contract_batch(n=300, seed=0xB4, max_records=12):
    """n wb_rep reps back to back (gaps 0..3) with one edit on every second rep,
    the kinds of WB_KINDS in turn, the j-th rep of a kind varying with j: the
    header count raised by 1 + j % 3 (slots no record fills), lowered by 1,
    set to 0 with records present; the rep cut to WB_SHORT[j % 5] bytes, under
    its 12-byte header; the rep cut by 1 + j % 5 bytes (inside its last
    record); a descriptor that starts inside the buffer and runs past
    base_len, and one that starts past it.  -> dict(base, offs u64, lens u32,
    n, and the answer of oracle.write_batch_protect per rep: status u8, first
    u64[n + 1] (the cumsum of the header counts of the reps in range), nprot
    u32, prot u64[total] with 0 in the slots no record filled, unfilled = those
    slots' indices, cf_unfilled = those of them in reps whose records carry
    column family tags)"""
    from oracle import oracle as O

    rng = np.random.default_rng(seed)
    reps, kinds, has_cf, raised = [], [], [], {}
    for b in range(n):
        tags = []
        r = bytearray(wb_rep(rng, int(rng.integers(0, max_records + 1)), tags))
        cnt = struct.unpack_from("<I", r, 8)[0]
        kind = WB_KINDS[b // 2 % 6] if b % 2 else "plain"
        j = b // 12  # the occurrence of this kind
        if kind == "raise":
            raised[b] = 1 + j % 3
            r[8:12] = struct.pack("<I", cnt + raised[b])
        elif kind == "lower" and cnt > 0:
            r[8:12] = struct.pack("<I", cnt - 1)
        elif kind == "zero":
            r[8:12] = struct.pack("<I", 0)
        elif kind == "short":
            r = r[:WB_SHORT[j % 5]]
        elif kind == "cut" and len(r) > 12 + 5:
            r = r[:len(r) - 1 - j % 5]
        reps.append(bytes(r))
        kinds.append(kind)
        has_cf.append(bool(set(tags) & set(WB_CF_TAGS)))
    offs = np.cumsum([0] + [len(r) + int(rng.integers(0, 4)) for r in reps[:-1]]).astype(np.uint64)
    lens = np.array([len(r) for r in reps], np.uint32)
    base = np.zeros(int(offs[-1]) + len(reps[-1]), np.uint8)
    for o, r in zip(offs, reps):
        base[int(o):int(o) + len(r)] = np.frombuffer(r, np.uint8)
    past = [b for b, k in enumerate(kinds) if k == "past"]
    for i, b in enumerate(past):  # descriptors past the buffer end (the rep's bytes stay where they are)
        offs[b] = len(base) - 20 if i % 2 == 0 else len(base) + 1 + i
        lens[b] = 21 + i if i % 2 == 0 else 40
    status, nprot, counts, vals, unfilled, cf_unfilled = [], [], [], [], [], []
    pos = 0
    for b, r in enumerate(reps):
        if kinds[b] == "past":
            status.append(WB_OUT_OF_RANGE)
            nprot.append(0)
            counts.append(0)
            continue
        code, want = O.write_batch_protect(r)
        cnt = struct.unpack_from("<I", r, 8)[0] if len(r) >= 12 else 0
        k = min(len(want), cnt)
        if b in raised:  # parsed whole, the raised slots and no others left unfilled
            assert (code, cnt - k) == (14, raised[b]), (b, code, cnt, k)
        status.append(code)
        nprot.append(k)
        counts.append(cnt)
        vals += want[:k] + [0] * (cnt - k)
        unfilled += list(range(pos + k, pos + cnt))
        if has_cf[b]:
            cf_unfilled += list(range(pos + k, pos + cnt))
        pos += cnt
    assert set(raised.values()) == {1, 2, 3}
    assert {len(r) for r, k in zip(reps, kinds) if k == "short"} == set(WB_SHORT)
    return dict(base=base, offs=offs, lens=lens, n=n, kinds=kinds,
                status=np.array(status, np.uint8), nprot=np.array(nprot, np.uint32),
                first=np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64),
                prot=np.array(vals, np.uint64), unfilled=np.array(unfilled, np.int64),
                cf_unfilled=np.array(cf_unfilled, np.int64))


def _varint(b, p):
    r = sh = 0
    while True:
        x = int(b[p])
        p += 1
        r |= (x & 127) << sh
        if not x & 128:
            return r, p
        sh += 7


def mem_checksum_pos(base, off):
    """position of a well-formed memtable entry's checksum bytes"""
    ikl, kp = _varint(base, off)
    vl, vp = _varint(base, kp + ikl)
    return vp + vl


@functools.lru_cache(maxsize=None)
def kv_blocks():
    """tests/golden/kv_blocks.{json,npz} (gen_kv_golden.py --kv-blocks): crafted
    blocks and WriteBatch reps answered by the reference -> (meta, arrays), in
    the layout of kv_sites (block_case / write_batch_case take both)"""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(golden, "kv_blocks.json")) as f:
        meta = json.load(f)
    z = np.load(os.path.join(golden, "kv_blocks.npz"), allow_pickle=False)
    return meta, {k: z[k] for k in z.files}


def check_block_results(cases, pb, enc, prot, first, st):
    """one batch call's outputs against the reference's answers of `cases`
    (block b = case b): the error marker or the key count, every kv_checksum_
    byte, and prot's low bytes = the encoded bytes"""
    assert int(first[0]) == 0
    for j, c in enumerate(cases):
        name = c.get("name") or (c["src"], c["kind_name"])
        nk = int(first[j + 1]) - int(first[j])
        want = c[f"keys_{pb}"]
        if want < 0:
            assert st[j] in (1, 2) and nk == 0, (name, pb, int(st[j]), nk)
            continue
        assert st[j] == 0 and nk == want, (name, pb, int(st[j]), nk, want)
        got = enc[int(first[j]) * pb:int(first[j + 1]) * pb].tobytes()
        assert got.hex() == c[f"kv_checksum_{pb}"], (name, pb)
        if prot is not None:
            low = prot[int(first[j]):int(first[j + 1])].astype(np.uint64).view(np.uint8)
            assert low.reshape(-1, 8)[:, :pb].tobytes() == got, (name, pb)
    assert int(first[len(cases)]) * pb == len(enc)


_restated = {}


def restated_batch(blocks, pb):
    """the restatement's answer for one batch call over blockgen.batch()'s
    blocks -> (first_key i64[n + 1], status u8[n], kv_checksums u8, prot u64);
    a None block (descriptor past the buffer) is status 3 without keys"""
    from oracle import oracle as O

    first, status, encs, prots = [0], [], [], []
    for b in blocks:
        if b is None:
            st, nk, enc, prot = 3, 0, b"", np.zeros(0, np.uint64)
        else:
            key = (b[0], b[1], pb)
            if key not in _restated:
                _restated[key] = O.block_kv_checksums(b[0], b[1], pb)
            st, nk, enc, prot = _restated[key]
        first.append(first[-1] + nk)
        status.append(st)
        encs.append(enc)
        prots.append(prot)
    return (np.array(first, np.int64), np.array(status, np.uint8),
            np.frombuffer(b"".join(encs), np.uint8), np.concatenate(prots + [np.zeros(0, np.uint64)]))


def block_case(meta, arrays):
    """-> (base u8, offsets u64, sizes u32, kinds u8, cases): every block of the
    fixture (reference-written SSTs' blocks + crafted damaged ones)"""
    cases = meta["blocks"]
    return (arrays["blk_base"], arrays["blk_offs"],
            np.array([c["size"] for c in cases], np.uint32),
            np.array([c["kind"] for c in cases], np.uint8), cases)
