"""forst_wal_records_compact on the MI355X against the serial reader's payloads
(oracle/wal_reader.py): the cases of tests/walcompact_cases.py (the emulator
twin is tests/test_emu_wal_compact.py) through the C ABI on device memory, every
scenario's descriptors taken from forst_wal_recover_batch on the device, and the
Python wrapper engine.wal_records_compact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import walcases as W  # noqa: E402
import walcompact_cases as C  # noqa: E402
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
        self.L = C.bind(_lib.lib())

    def up(self, a):
        return _DevBuf(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def run():
    engine.init_device()
    return GpuRunner()


@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_compact_length_sweep(run, recyclable):
    C.case_sweep(run, recyclable)


@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_compact_step_lengths(run, recyclable):
    C.case_sweep_steps(run, recyclable)


@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_compact_overlong_fragments(run, recyclable):
    C.case_overlong_fragments(run, recyclable)


@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_compact_fragment_edges(run, recyclable):
    C.case_fragment_edges(run, recyclable)


@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_compact_big_records(run, recyclable):
    C.case_big_records(run, recyclable)


@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_compact_control_records(run, recyclable):
    C.case_control(run, recyclable, via_recover=None)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_compact_recovery_scenarios(run, recyclable, mode):
    C.case_scenarios(run, recyclable, mode, via_recover=None)


def test_gpu_compact_many_records(run):
    C.case_many_records(run)


def test_gpu_compact_contracts(run):
    C.case_contracts(run)


@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_compact_bad_descriptors(run, recyclable):
    C.case_bad_descriptors(run, recyclable)


@pytest.mark.parametrize("recyclable", [False, True])
def test_gpu_compact_chain(run, recyclable):
    C.run_chain(run, recyclable)


def test_gpu_compact_python_wrapper(run):
    """engine.wal_records_compact on what engine.wal_recover_batch returns, with
    the wrapper's own arena, the caller's, and one that is too small"""
    log = W.frame_lens([10, 0, 40000, 16, 17, 300, 0, 70001], 4, True)[0]
    want = C.reader_records(log, 7)
    arena, offs, sizes = C.expected([w[1] for w in want])
    dlog = torch.from_numpy(log).to(DEV)
    rec, _, res = engine.wal_recover_batch(dlog, 7)
    assert res.n_records == len(want)
    for records in (rec, (rec["offset"], rec["length"], rec["hash"], rec["n_fragments"])):
        a, o, s, st = engine.wal_records_compact(dlog, records)
        torch.cuda.synchronize()
        assert a.numel() == len(arena) and (a.cpu().numpy() == arena).all()
        assert (o.cpu().numpy().view(np.uint64) == offs).all()
        assert (s.cpu().numpy().view(np.uint32) == sizes).all()
        assert (st.cpu().numpy() == 0).all()
    mine = torch.full((len(arena) + 64,), C.S8, dtype=torch.uint8, device=DEV)
    a, o, s, st = engine.wal_records_compact(dlog, rec, arena=mine)
    torch.cuda.synchronize()
    assert a.data_ptr() == mine.data_ptr() and (a.cpu().numpy() == arena).all()
    assert (mine[len(arena):].cpu().numpy() == C.S8).all()
    with pytest.raises(_lib.ForstError) as e:
        engine.wal_records_compact(dlog, rec, arena=mine[:len(arena) - 16])
    assert e.value.code == C.EINVAL and e.value.arena_bytes == len(arena)
    with pytest.raises(AssertionError):
        engine.wal_records_compact(dlog.cpu(), rec)
    with pytest.raises(AssertionError):
        engine.wal_records_compact(dlog, {**rec, "n_fragments": rec["n_fragments"].to(torch.int64)})
