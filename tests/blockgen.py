"""tests/blockgen.py -- TEST INFRASTRUCTURE: a small deterministic builder of
block-based-table blocks (the BlockBuilder layout: entries, restart array,
optional data-block hash index, footer) for the block kv-checksum tests.

  entry (data, metaindex, full-value index):
      varint32 shared | varint32 non_shared | varint32 value_length | key delta | value
  entry (format_version >= 4 index, values delta-encoded):
      varint32 shared | varint32 non_shared | key delta | index value
      index value = varint64 offset, varint64 size when shared == 0, else one
      zigzag varint64 (the size delta); then, with first keys, varint32 length
      + first key
  tail: fixed32 restart offsets, [hash buckets u8[n], fixed16 n], fixed32
        num_restarts (| 1 << 31 with a hash index)

kind values are forst_block_kv_checksum_batch's: 0 data, 1 index, 2 metaindex,
| 4 index values not delta-encoded, | 8 index values carry a first key."""
import struct

import numpy as np

DATA, INDEX, META, FULL, FIRST = 0, 1, 2, 4, 8


def varint(v):
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def zigzag(v):
    """PutVarsignedint64 (util/coding.h i64ToZigzag)"""
    return varint(v << 1 if v >= 0 else ((-v) << 1) - 1)


def index_value(shared, handle, first_key=None):
    """IndexValue::EncodeTo: handle = (offset, size) or, when the entry shares
    key bytes, the size delta"""
    if shared:
        out = zigzag(handle if isinstance(handle, int) else handle[1])
    else:
        out = varint(handle[0]) + varint(handle[1])
    if first_key is not None:
        out += varint(len(first_key)) + first_key
    return out


def common_prefix(a, b):
    n = 0
    for x, y in zip(a, b):
        if x != y:
            break
        n += 1
    return n


def tail(restarts, hash_buckets=None, footer=None):
    """restart array [+ hash index] + footer; hash_buckets: bytes of the bucket
    map, or a count (every bucket 'no entry' = 255)"""
    out = b"".join(struct.pack("<I", r) for r in restarts)
    foot = len(restarts)
    if hash_buckets is not None:
        if isinstance(hash_buckets, int):
            hash_buckets = bytes([255]) * hash_buckets
        out += hash_buckets + struct.pack("<H", len(hash_buckets))
        foot |= 1 << 31
    return out + struct.pack("<I", foot if footer is None else footer)


def build(entries, kind=DATA, interval=16, hash_buckets=None, share=True, share_over_restarts=False,
          footer=None):
    """entries: [(key bytes, value)]; value = bytes, or for delta-encoded index
    blocks ((offset, size), first key or None).  Keys share their common prefix
    with the previous key inside a restart interval (share_over_restarts: at
    restart points too, which the sequential walk of the protection code
    accepts)."""
    delta_v4 = (kind & 3) == INDEX and not kind & FULL
    if (kind & 3) == META:
        interval = 1  # MetaBlockIter assumes it (block.h:826-829)
    out, restarts, prev, prev_size = bytearray(), [], b"", 0
    for i, (key, value) in enumerate(entries):
        at_restart = i % interval == 0
        if at_restart:
            restarts.append(len(out))
        shared = common_prefix(prev, key) if share and (share_over_restarts or not at_restart) else 0
        if delta_v4:
            handle, fk = value
            v = index_value(shared, handle[1] - prev_size if shared else handle, fk)
            prev_size = handle[1]
            out += varint(shared) + varint(len(key) - shared) + key[shared:] + v
        else:
            out += varint(shared) + varint(len(key) - shared) + varint(len(value)) + key[shared:] + value
        prev = key
    if not restarts:
        restarts = [0]  # BlockBuilder: an empty block still has one restart
    return bytes(out) + tail(restarts, hash_buckets, footer)


def sized(target, entries, filler_key, **kw):
    """build(entries + one filler entry) of exactly `target` bytes"""
    n = max(0, target - len(build(entries + [(filler_key, b"")], **kw)))
    for _ in range(8):
        blk = build(entries + [(filler_key, bytes(n))], **kw)
        if len(blk) == target:
            return blk
        n += target - len(blk)
    raise ValueError("cannot reach the size")


def pattern(n, salt):
    """n deterministic bytes of period 251 (every 4- and 16-byte window of a
    period differs; long fixtures still compress)"""
    return (((np.arange(n, dtype=np.int64) + salt) * 7) % 251).astype(np.uint8).tobytes()


def keys_with_prefix(rng, n, prefix_len, key_len):
    """n sorted distinct keys of key_len bytes sharing their first prefix_len bytes"""
    pre = rng.integers(0, 256, prefix_len, dtype=np.uint8).tobytes()
    tails = sorted({rng.integers(0, 256, max(1, key_len - prefix_len), dtype=np.uint8).tobytes()
                    for _ in range(n)})
    return [(pre + t)[:max(key_len, prefix_len + 1)] for t in tails]


def odd_block(rng):
    """-> (bytes, kind): a block with no restarts, a damaged block, or one of
    0..7 bytes"""
    kind = int(rng.choice([DATA, META, INDEX, INDEX | FIRST, INDEX | FULL]))
    what = int(rng.integers(0, 7))
    if what == 0:  # no restarts: no protection (block.cc:1116)
        junk = rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8).tobytes()
        # ... also with the hash-index bit: a bucket map, or junk as the bucket count
        return junk + (bytes(4), tail([], hash_buckets=2), struct.pack("<I", 1 << 31))[int(rng.integers(0, 3))], kind
    if what == 1:  # 0..7 bytes
        n = int(rng.integers(0, 8))
        foot = struct.pack("<I", int(rng.choice([0, 1, 2, 1 << 31, (1 << 31) | 1, 0xFFFFFFFF])))
        return (rng.integers(0, 256, 4, dtype=np.uint8).tobytes() + foot)[8 - n:], kind
    if what == 6:  # a delta-encoded index value cut off at the restart offset, nothing behind it
        kind = INDEX | (FIRST if rng.random() < 0.5 else 0)
        good = b"\x00\x04abcd\x10\x20" + (b"\x02fk" if kind & FIRST else b"")
        cuts = [b"\x00\x01k", b"\x00\x01k\x07", b"\x01\x01k", b"\x00\x01k\x80", b"\x00\x01k\x07\x80"]
        if kind & FIRST:  # ... the first-key length varint, or the first key itself
            cuts += [b"\x00\x01k\x07\x08", b"\x01\x01k\x03", b"\x00\x01k\x07\x08\x80", b"\x01\x01k\x03\x05fk"]
        return good * int(rng.integers(1, 4)) + cuts[int(rng.integers(0, len(cuts)))] + tail((0,)), kind
    blk, kind = random_block(rng, n_entries=int(rng.integers(1, 6)))
    if what == 2:  # the first entry shares bytes with no key
        return b"\x05" + blk[1:], kind
    if what == 3:  # a restart count that wraps the restart offset
        return blk[:-4] + struct.pack("<I", (len(blk) // 4 + int(rng.integers(0, 1 << 20))) |
                                      (struct.unpack_from("<I", blk, len(blk) - 4)[0] & (1 << 31))), kind
    # an entry header cut off by the restart array / a 5-byte varint that goes on
    good = b"\x00\x04\x02abcdxy" if not ((kind & 3) == INDEX and not kind & FULL) else \
        b"\x00\x04abcd\x10\x20" + (b"\x00" if kind & FIRST else b"")
    bad = b"\x85\x80\x80" if what == 4 else b"\x80\x80\x80\x80\x80\x01\x01\x01kv"
    return good + bad + tail((0, len(good)) if (kind & 3) == META else (0,)), kind


def batch(rng, n, tail_len=0):
    """n descriptors for one batch call -> (base u8, offsets u64, sizes u32,
    kinds u8, blocks): random well-formed blocks interleaved with odd_block()s
    and descriptors that run past the buffer (blocks[j] None), block starts at
    every offset mod 16, the descriptors in another order than the bytes.
    base ends right behind the last block (+ tail_len spare bytes)."""
    blocks = []
    for j in range(n):
        r = rng.random()
        blocks.append(None if r < 0.02 else odd_block(rng) if r < 0.2 else random_block(rng))
    pos, starts = 0, []
    for j, b in enumerate(blocks):
        pos += (j - pos) % 16
        starts.append(pos)
        pos += len(b[0]) if b else 0
    base = np.zeros(pos + tail_len, np.uint8)
    offs, sizes, kinds = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    for j, (b, o) in enumerate(zip(blocks, starts)):
        if b is None:  # the offset, or the size from an inside offset, past base_len
            offs[j] = len(base) + 1 + j if j % 2 else max(0, len(base) - 5)
            sizes[j] = 12 if j % 2 else 6 + j % 50
            kinds[j] = j % 3
            continue
        base[o:o + len(b[0])] = np.frombuffer(b[0], np.uint8)
        offs[j], sizes[j], kinds[j] = o, len(b[0]), b[1]
    perm = rng.permutation(n)
    return base, offs[perm], sizes[perm], kinds[perm], [blocks[i] for i in perm]


def random_block(rng, kind=None, n_entries=None):
    """a well-formed random block -> (bytes, kind)"""
    if kind is None:
        kind = int(rng.choice([DATA, DATA, DATA, META, INDEX, INDEX | FIRST, INDEX | FULL,
                               INDEX | FULL | FIRST]))
    if n_entries is None:
        n_entries = int(rng.integers(1, 9)) if rng.random() < 0.9 else int(rng.integers(9, 120))
    interval = int(rng.choice([1, 2, 3, 16]))
    klen = int(rng.choice([4, 8, 17, 24, 40, 130, 250]))
    plen = int(rng.integers(0, klen))
    keys = keys_with_prefix(rng, n_entries, plen, klen)
    delta_v4 = (kind & 3) == INDEX and not kind & FULL
    ents, off = [], int(rng.integers(0, 1 << 20))
    for k in keys:
        if delta_v4:
            size = int(rng.integers(1, 1 << int(rng.integers(1, 30))))
            fk = None
            if kind & FIRST:
                fk = rng.integers(0, 256, int(rng.choice([0, 8, 24, 200])), dtype=np.uint8).tobytes()
            ents.append((k, ((off, size), fk)))
            off += size + 5
        else:
            vlen = int(rng.choice([0, 1, 5, 16, 17, 40, 100, 129, 241, 300]))
            ents.append((k, rng.integers(0, 256, vlen, dtype=np.uint8).tobytes()))
    hb = None
    if kind == DATA and rng.random() < 0.3:
        hb = int(rng.integers(1, 40))
    return build(ents, kind=kind, interval=interval, hash_buckets=hb), kind
