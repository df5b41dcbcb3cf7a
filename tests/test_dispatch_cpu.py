"""The inputs of tests/test_gpu_paths.py reach their intended kernel paths:
the builders of tests/dispatch.py at 256 and 304 compute units, checked
against the host restatements of the dispatch rules -- no GPU needed.
(Layouts only: the payload bytes play no part in any dispatch rule.)"""
import numpy as np
import pytest

import dispatch as D
from oracle import oracle as O

CUS = [256, 304]


def test_counting_search_is_lower_bound_in_file_order_and_tiles_any_order():
    """wg_bounds against numpy's lower_bound where the keys are sorted, and
    an exact monotone cover of [0, n) for a permuted batch"""
    rng = np.random.default_rng(1)
    sizes = rng.integers(0, 20000, 70000).astype(np.uint32)
    offs = np.zeros(len(sizes), np.uint64)
    offs[1:] = np.cumsum(sizes[:-1].astype(np.uint64) + np.uint64(5))
    for G, c in ((256, 0), (304, 256), (7, 256)):
        L = D.wg_bounds(offs, sizes, G, c)
        keys = offs + np.uint64(c) * np.arange(len(offs), dtype=np.uint64)
        span = int(offs[-1]) + int(sizes[-1]) + c * (len(offs) - 1) - int(offs[0])
        want = [0] + [int(np.searchsorted(keys, np.uint64(span * b // G))) for b in range(1, G)]
        assert L.tolist() == want + [len(offs)]
    p = rng.permutation(len(offs))
    L = D.wg_bounds(offs[p], sizes[p], 256, 0)
    assert L[0] == 0 and L[-1] == len(offs) and (np.diff(L) >= 0).all()
    # fewer descriptors than one probe level, and no byte span (all empty at 0)
    assert D.wg_bounds(offs[:40], sizes[:40], 8, 0)[-1] == 40
    z = np.zeros(100, np.uint64)
    assert D.wg_bounds(z, z.astype(np.uint32), 8, 0).tolist() == [0, 13, 26, 39, 52, 65, 78, 91, 100]


@pytest.mark.parametrize("cus", CUS)
def test_raw_crc_batch_reaches_lane_and_filter_kernels(cus):
    r = D.raw_crc_batch(cus, fill=False)
    n, offs, sizes = r["n"], r["offs"], r["sizes"]
    grid = D.crc_grid(n, cus)
    assert grid == cus
    assert D.crc_raw_kernel(n, r["total"], cus) == "crc32c_rows_raw_filt_kernel"
    assert n >= 128 * grid * D.CRC_WAVES and D.feed_share1(n, grid * D.CRC_WAVES) > 0
    assert n < 1.25 * 128 * D.CRC_WAVES * cus  # (no larger than it has to be)
    have = set(zip(sizes.tolist(), (offs & np.uint64(15)).tolist()))
    assert all((int(s), a) in have for s in D.STRADDLE for a in range(16))
    assert set(range(17)) <= set(sizes.tolist())
    assert ((sizes >= 4096) & (sizes <= 70000)).sum() == n // 1000
    assert sizes[sizes < 4096].max() <= 600 and (sizes < D.RAW_SPLIT).sum() > n // 3
    gaps = (offs[1:] - offs[:-1] - sizes[:-1]).astype(np.int64)
    assert gaps.min() == 0 and gaps.max() == 8
    assert int(offs[-1]) + int(sizes[-1]) <= r["total"]
    # the edge descriptors keep the batch on the same path
    o2, s2, zero = D.raw_edge_descriptors(offs, sizes, r["total"])
    for k in range(5, 14):
        inside = int(o2[k]) + int(s2[k]) <= r["total"]
        assert inside == (k not in zero)
    assert sorted(int(s2[k]) for k in (9, 10, 11, 12, 13)) == [77, 255, 256, 509, 1300]
    assert all(int(o2[k]) + int(s2[k]) == r["total"] for k in (9, 10, 11, 12, 13))


@pytest.mark.parametrize("cus", CUS)
def test_raw_xxh3_batch_reaches_static_shares(cus):
    x = D.raw_xxh3_batch(cus, fill=False)
    n, offs, sizes = x["n"], x["offs"], x["sizes"]
    for occ in (1, D.XX_RAW_OCCUPANCY):
        grid = D.xx_rows_grid(n, cus, occ)
        assert grid == cus * occ
        assert n >= 128 * D.XX_ROWS_WAVES * grid and D.feed_share1(n, grid * D.XX_ROWS_WAVES) > 0
    assert x["total"] >= D.SIMPLE_BELOW  # (the rows kernel, not the simple one)
    cls = D.xxh3_class(sizes)
    have = set(zip(cls.tolist(), (offs & np.uint64(15)).tolist()))
    assert have == {(c, a) for c in range(len(D.XXH3_CLASSES)) for a in range(16)}
    for c, (lo, hi) in enumerate(D.XXH3_CLASSES[:-1]):  # both ends of every class
        assert {lo, hi} <= set(sizes[cls == c].tolist())
    assert (sizes >= 4096).sum() == n // 1000


@pytest.mark.parametrize("recyclable", [False, True])
@pytest.mark.parametrize("cus", CUS)
def test_dense_wal_reaches_the_unstaged_fill(cus, recyclable):
    w = D.dense_wal(cus, recyclable, 77, O.wal_frame, fill=False)
    poffs, plens, nb, nd, bb = w["poffs"], w["plens"], w["n_blocks"], w["n_dense"], w["boundary_block"]
    assert nd > 64 * D.CRC_WAVES * cus              # physical records of the dense part
    assert bb >= 300 and nb - 1 - bb >= 300         # blocks of each part
    assert plens[:nd].max() <= 200 and plens[nd:].max() > 20000
    assert len(w["buf"]) % D.LOG_BLOCK == 1000 + (11 if recyclable else 7)  # a short last block
    tiles = D.wal_tile_records(poffs, nb)
    assert len(tiles) == (nb + D.WAL_TILE - 1) // D.WAL_TILE and tiles.sum() == len(poffs)
    assert (tiles > D.WAL_FILL_CAP).any()                       # direct stores
    assert ((tiles >= 1) & (tiles <= D.WAL_FILL_CAP)).any()     # staged in LDS
    # the tile of the first sparse block holds blocks of both regimes
    t = bb // D.WAL_TILE
    per_block = np.bincount((poffs // D.LOG_BLOCK).astype(np.int64), minlength=nb)
    mixed = per_block[t * D.WAL_TILE:(t + 1) * D.WAL_TILE]
    assert mixed[:bb % D.WAL_TILE].min() > 100 and mixed[bb % D.WAL_TILE + 1:].max() < 100
    assert bb % D.WAL_TILE >= 64 and len(mixed) - bb % D.WAL_TILE >= 64
    # the sub-ranges of the GPU test start tiles of their own at first_block
    for fb, n in ((1, 255), (255, 2), (257, nb - 257)):
        st = D.wal_tile_records(poffs, n, fb)
        assert st.sum() == per_block[fb:fb + n].sum()
    assert D.wal_tile_records(poffs, nb - 257, 257).max() > D.WAL_FILL_CAP
    # the faults of the GPU test: one per block, every status the reader has
    w["recyclable"] = recyclable
    buf, hit = D.wal_faults(w, 77)
    st, nr, fo = O.wal_verify_blocks(buf, 77, nthreads=4)
    st0 = O.wal_verify_blocks(w["buf"], 77, nthreads=4)[0]
    assert set(st0.tolist()) <= {0, 3}  # (3: a block's tail of 7..10 zero bytes, recyclable)
    assert np.nonzero(st != st0)[0].tolist() == hit
    assert set(st[hit].tolist()) == ({1, 2, 3, 4} if recyclable else {1, 2, 3})
    tile_of = {b // D.WAL_TILE for b in hit}
    assert any(tiles[t] > D.WAL_FILL_CAP for t in tile_of)
    assert any(tiles[t] <= D.WAL_FILL_CAP for t in tile_of) and bb // D.WAL_TILE in tile_of


@pytest.mark.parametrize("kind", ["crc32c", "xxh3"])
@pytest.mark.parametrize("cus", CUS)
def test_clustered_batch_reaches_direct_stores(cus, kind):
    if kind == "crc32c":
        offs, sizes, total, n_small = D.crc_clustered(cus)
        G, cost, stage = D.crc_grid(len(offs), cus), D.CRC_BLOCK_COST, D.CRC_STAGE_W
    else:
        offs, sizes, total, n_small = D.xxh3_clustered(cus)
        G = D.xx_rows_grid(len(offs), cus, D.XX_BLOCK_OCCUPANCY)
        cost, stage = D.XX_BLOCK_COST, D.XX_STAGE_W
        assert total < int(2.5 * 2**30)
    assert G == cus and total >= D.SIMPLE_BELOW and len(offs) < 0xffffffff
    assert (np.diff(offs.astype(np.int64)) >= sizes[:-1].astype(np.int64) + 5).all()  # file order
    L, b, direct = D.direct_part(offs, sizes, G, cost, stage)
    assert L[b + 1] - L[b] > stage and len(direct) > 0
    assert D.covers_small_sizes(offs, sizes, direct)
    # ... and the staged part holds small blocks at every alignment too
    staged = np.arange(L[b], L[b] + stage)
    assert {int(o) & 15 for o in offs[staged]} == set(range(16))
    assert sizes[direct].max() > 130  # large blocks finish in the direct part as well
    # every other range is staged whole
    others = np.delete(np.diff(L), b)
    assert others.max() <= stage and others.min() >= 1
    # the verify pass's victims and out-of-range descriptors lie in both parts
    f = D.verify_faults(offs, sizes, total, G, cost, stage)
    assert f["b"] == b and len(f["staged"]) == 24 and len(f["direct"]) == 40
    assert (f["offs"][f["staged"][:3]] != offs[f["staged"][:3]]).all()
    assert (f["offs"][f["direct"][:4]] != offs[f["direct"][:4]]).all()


def test_small_buffers_and_large_blocks_layouts():
    bufs = D.small_buffers()
    assert all(blen < D.SIMPLE_BELOW for blen, _, _ in bufs[:-2]) and len(bufs) > 10
    assert [b[0] for b in bufs[-3:]] == [4095, 4096, 4097]
    have = set()
    for blen, offs, sizes in bufs:
        assert (offs.astype(np.int64) + sizes + 5 <= blen).all()
        have |= set(zip(sizes.tolist(), (offs & np.uint64(15)).tolist()))
    assert {(s, a) for s in range(201) for a in range(16)} <= have
    assert {1024, 4000} <= {s for s, _ in have}
    offs, sizes, total = D.large_blocks()
    big = sizes > 4096
    assert sorted(set(sizes[big].tolist())) == D.LARGE_SIZES
    assert {(int(s), int(o) & 3) for s, o in zip(sizes[big], offs[big])} == \
        {(s, a) for s in D.LARGE_SIZES for a in range(4)}
    assert (sizes[1::2] == 4096).all() and int(offs[-1]) + 4096 + 5 <= total
