"""forst_wal_frame_batch on the MI355X against the writer's image
(oracle.wal_frame) and forst_wal_layout_at: the cases of tests/walframe_cases.py
(the emulator twin is tests/test_emu_wal_frame.py) through the C ABI on device
memory, and the Python wrapper engine.wal_frame_batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import walframe_cases as F  # noqa: E402
from forst_amd import _lib, engine  # noqa: E402

DEV = "cuda"


class _DevBuf:
    def __init__(self, a):
        self.dtype = a.dtype
        self.t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(DEV)
        if self.t.numel() == 0:
            self.t = torch.zeros(16, dtype=torch.uint8, device=DEV)[:0]
        self.ptr = self.t.data_ptr()

    def host(self):
        torch.cuda.synchronize()
        return self.t.cpu().numpy().view(self.dtype)


class GpuRunner:
    """the runner of tests/walcompact_cases.py on device memory (the calls go
    to the null stream; host() waits for the device)"""

    def __init__(self):
        self.L = F.bind(_lib.lib())

    def up(self, a):
        return _DevBuf(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def run():
    engine.init_device()
    return GpuRunner()


@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_frame_length_sweep(run, recyclable):
    F.case_length_sweep(run, recyclable)


@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_frame_block_edges(run, recyclable):
    F.case_block_edges(run, recyclable)


@pytest.mark.parametrize("part", ["empty", "1009", "many", "1 MiB + 1"])
def test_gpu_frame_tiles_and_windows(run, part):
    F.case_tiles_and_windows(run, part)


@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_frame_source_alignment_and_end(run, recyclable):
    F.case_source(run, recyclable)


@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_frame_out_of_range_reps(run, recyclable):
    F.case_out_of_range(run, recyclable)


def test_gpu_frame_contracts(run):
    F.case_contracts(run)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_frame_roundtrip(run, recyclable, mode):
    F.case_roundtrip(run, recyclable, mode)


@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_frame_chain(run, recyclable):
    F.case_chain(run, recyclable)


@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_frame_appending(run, recyclable):
    F.case_appending(run, recyclable)


def test_gpu_frame_python_wrapper(run):
    """engine.wal_frame_batch with the wrapper's own image, the caller's, one
    that is too small, with and without the host sizes; its argument checks"""
    reps = F.random_reps([10, 0, 40000, 16, 17, 300, 0, 70001], 4)
    base, offs, sizes = F.stage(reps)
    b = 5000
    want = F.oracle_image(reps, True, 7, b)
    po, pl, pt, total, npad, end = F.layout_at(sizes, True, b)
    dbase = torch.from_numpy(base).to(DEV)
    doffs = torch.from_numpy(offs.view(np.int64)).to(DEV)
    dsizes = torch.from_numpy(sizes.view(np.int32)).to(DEV)
    for hsz in (None, torch.from_numpy(sizes.view(np.int32).copy())):
        img, desc, res = engine.wal_frame_batch(dbase, doffs, dsizes, True, 7, block_offset=b,
                                                host_sizes=hsz)
        torch.cuda.synchronize()
        assert img.numel() == total and (img.cpu().numpy() == want).all()
        assert (res.image_bytes, res.n_physical, res.n_pads, res.end_block_offset,
                res.bad_records) == (total, len(po), npad, end, 0)
        assert (desc["phys_offsets"].cpu().numpy().view(np.uint64) == po).all()
        assert (desc["phys_lengths"].cpu().numpy().view(np.uint32) == pl).all()
        assert (desc["phys_types"].cpu().numpy() == pt).all()
        assert (desc["status"].cpu().numpy() == 0).all()
        t = np.where(pt > 4, pt - 4, pt)
        assert (desc["rec_offsets"].cpu().numpy().view(np.uint64) == po[(t == 1) | (t == 2)]).all()
    mine = torch.full((total + 64,), F.S8, dtype=torch.uint8, device=DEV)
    img, _, _ = engine.wal_frame_batch(dbase, doffs, dsizes, True, 7, block_offset=b, image=mine)
    torch.cuda.synchronize()
    assert img.data_ptr() == mine.data_ptr() and (img.cpu().numpy() == want).all()
    assert (mine[total:].cpu().numpy() == F.S8).all()
    with pytest.raises(_lib.ForstError) as e:
        engine.wal_frame_batch(dbase, doffs, dsizes, True, 7, block_offset=b, image=mine[:total - 1])
    assert e.value.code == F.EINVAL and e.value.image_bytes == total
    with pytest.raises(_lib.ForstError) as e:
        engine.wal_frame_batch(dbase, doffs, dsizes, True, 7, block_offset=F.BLOCK + 1)
    assert e.value.code == F.EINVAL
    for bad in ((dbase.cpu(), doffs, dsizes), (dbase, doffs.cpu(), dsizes),
                (dbase, doffs, dsizes.cpu()), (dbase, doffs.to(torch.int32), dsizes),
                (dbase, doffs, dsizes.to(torch.int64)), (dbase.to(torch.int8), doffs, dsizes),
                (dbase, doffs[::2], dsizes[::2]), (dbase, doffs, dsizes[:-1])):
        with pytest.raises(AssertionError):
            engine.wal_frame_batch(*bad, True, 7)
    with pytest.raises(AssertionError):
        engine.wal_frame_batch(dbase, doffs, dsizes, True, 7, host_sizes=dsizes)
    with pytest.raises(AssertionError):
        engine.wal_frame_batch(dbase, doffs, dsizes, True, 7, image=mine.cpu())
    with pytest.raises(AssertionError):
        engine.wal_frame_batch(dbase, doffs, dsizes, True, 7, image=mine.to(torch.int8))
