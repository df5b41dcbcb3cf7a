"""tests/kvsites.py -- TEST INFRASTRUCTURE: the a15 call-site cases of
tests/golden/kv_sites.{json,npz} (reference-made, gen_kv_golden.py) laid out
as the engine's batch calls take them: memtable entry buffers with their
corrupted copies, and the WriteBatch reps back to back."""
import functools
import json
import os

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
