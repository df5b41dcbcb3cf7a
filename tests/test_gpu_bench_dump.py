"""bench.py --dump-outputs (dump_outputs) on a small config: the .npy files
hold what the timed path's last step left for its caller -- the trailers the
write side stored, the checksums and verdicts of the read side -- bit-exact
against the oracle, in float32 / float64, whole while they fit the budget and
as a fixed sorted sample of the blocks when they do not."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 3001  # odd, several workgroups; sizes off every tile boundary
SPEC = (37, 4097, 16384)


@pytest.fixture(scope="module")
def bench():
    import bench as B

    B.CONFIGS["T1"] = (N, SPEC, 1, "test: mixed sizes kCRC32c")
    B.CONFIGS["T4"] = (N, SPEC, 4, "test: mixed sizes kXXH3")
    B.SEEDS["T1"] = B.SEEDS["T4"] = 0x7E57
    yield B
    for k in ("T1", "T4"):
        del B.CONFIGS[k], B.SEEDS[k]


def _load(d):
    return {p.name[:-4]: np.load(p) for p in sorted(d.iterdir())}


@pytest.mark.parametrize("cfg", ["T1", "T4"])
def test_dump_outputs_equal_the_oracle(bench, cfg, tmp_path, monkeypatch):
    from forst_amd import engine
    from oracle import oracle as O

    engine.init_device()
    res = bench.run_config(cfg, 2, 1, 0, 1)
    b = res["batch"]
    bench.dump_outputs(str(tmp_path / "full"), res, b, 0, 1)
    full = _load(tmp_path / "full")
    assert sorted(full) == ["block_index", "computed", "mismatches", "ok", "trailers"]
    assert full["trailers"].dtype == np.float32 and full["ok"].dtype == np.float32
    assert all(full[k].dtype == np.float64 for k in ("computed", "mismatches", "block_index"))
    assert sum(a.nbytes for a in full.values()) <= 64 << 20
    assert (full["block_index"] == np.arange(N)).all()
    assert full["trailers"].shape == (N, 5) and full["computed"].shape == (N,)

    hb = b.base.cpu().numpy()
    offs = b.offsets.cpu().numpy()
    sizes = b.sizes.cpu().numpy().astype(np.uint32)
    ocomp, ook, obad = O.block_verify_batch(res["ctype"], hb, offs, sizes, nthreads=4)
    assert obad == 0 and full["mismatches"].tolist() == [0.0]
    assert (full["computed"] == ocomp.astype(np.uint64).astype(np.float64)).all()
    assert (full["ok"] == 1).all()
    t = full["trailers"].astype(np.float64)
    assert (t[:, 0] == 0).all()  # kNoCompression type byte
    assert (t[:, 1] + t[:, 2] * 2**8 + t[:, 3] * 2**16 + t[:, 4] * 2**24 == full["computed"]).all()

    # over the budget: the same fixed sample of blocks each time, rows unchanged
    monkeypatch.setattr(bench, "DUMP_BUDGET", 1000 * bench.DUMP_ROW)
    for name in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / name), res, b, 0, 1)
    s1, s2 = _load(tmp_path / "s1"), _load(tmp_path / "s2")
    idx = s1["block_index"].astype(np.int64)
    assert len(idx) == 1000 and (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < N
    for k in ("trailers", "computed", "ok", "block_index"):
        assert np.array_equal(s1[k], s2[k]) and np.array_equal(s1[k], full[k][idx]), k
