#!/usr/bin/env python3
"""tools/wal_compact_time.py -- speed of forst_wal_records_compact on the MI355X
against the chip's own device-to-device copy of the same byte count.

A C5-shaped log (forst_amd/workload.py make_wal_batch: record lengths
log-uniform 32 B..32 KiB, framed by log::Writer's rules) is built and recovered
on the device (forst_wal_recover_batch).  After the warm-up rounds, in one
process and alternating, each round times by HIP events
  compact   forst_wal_records_compact into a preallocated arena (the whole
            call: walk, scan, the read-back of the total, copy kernels)
  count     the same call without an arena (walk, scan and read-back only)
  memcpy    hipMemcpyAsync device-to-device of *arena_bytes bytes: the yardstick
Before timing, XXH3 over the compacted reps is compared with the recovery's
record hashes (the result at the timed size is the right one).  Reported per
call: median (min-max) in ms and, for compact and memcpy, bytes read + written
over the median.  One JSON line at the end.

The default of 2 M records (7.7 GB of log, the same again of arena) is C5
scaled down so that log, arena and copy target fit beside each other with room
to spare; the full C5 log has 11.4 M records.  The run stops on the first
failing HIP or engine call and at the time limit.

  python tools/wal_compact_time.py [--records 2000000] [--reps 10] [--warmup 3] [--limit 420]
"""
import argparse
import ctypes
import json
import os
import signal
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from forst_amd import engine, workload  # noqa: E402
from forst_amd._lib import check, lib  # noqa: E402

D2D = 3  # hipMemcpyDeviceToDevice


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=420, help="seconds before the run is ended")
    ap.add_argument("--recyclable", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: no timing is taken anywhere else"
    signal.alarm(args.limit)  # the default action ends the process
    engine.init_device()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                   ctypes.c_void_p]
    w = workload.make_wal_batch(args.records, workload.SEEDS["C5"], recyclable=args.recyclable,
                                log_number=7)
    log = w.log
    rec, _, res = engine.wal_recover_batch(log, 7)
    n = res.n_records
    assert n == args.records and res.n_reports == 0, (n, res.n_reports)
    arena, rep_off, rep_size, status = engine.wal_records_compact(log, rec)
    total = arena.numel()
    assert not bool(status.any()), "a record's layout was not followed"
    h = engine.xxh3_64_batch(arena, rep_off, rep_size)
    assert bool((h.view(torch.int64) == rec["hash"].view(torch.int64)).all()), \
        "XXH3 over the compacted reps differs from the recovery's record hashes"
    payload = int(rec["length"].sum().item())
    copy_dst = torch.empty(total, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    got = ctypes.c_uint64()
    ins = (log.data_ptr(), log.numel(), rec["offset"].data_ptr(), rec["length"].data_ptr(),
           rec["n_fragments"].data_ptr(), n)
    outs = (rep_off.data_ptr(), rep_size.data_ptr(), status.data_ptr(), ctypes.byref(got), stream)

    def compact():
        check(lib().forst_wal_records_compact(*ins, arena.data_ptr(), total, *outs))
        assert got.value == total

    def count():
        check(lib().forst_wal_records_compact(*ins, None, 0, *outs))

    def memcpy():
        rc = hip.hipMemcpyAsync(copy_dst.data_ptr(), arena.data_ptr(), total, D2D, stream)
        if rc != 0:
            raise RuntimeError(f"hipMemcpyAsync failed ({rc})")

    calls = (("compact", compact), ("count", count), ("memcpy", memcpy))
    times = {name: [] for name, _ in calls}
    for r in range(args.warmup + args.reps):
        for name, fn in calls:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if r >= args.warmup:
                times[name].append(t0.elapsed_time(t1))
    torch.cuda.synchronize()
    kernel = engine.last_kernel()
    row = dict(records=n, log_bytes=log.numel(), arena_bytes=total, payload_bytes=payload,
               recyclable=bool(args.recyclable), reps=args.reps, warmup=args.warmup)
    print(f"C5-shaped log: {n} records, {log.numel() / 1e9:.3f} GB log, {total / 1e9:.3f} GB arena, "
          f"{payload / 1e9:.3f} GB payload; device {torch.cuda.get_device_name(0)}")
    for name, _ in calls:
        ms = np.array(times[name])
        med = float(np.median(ms))
        row[name] = dict(median_ms=round(med, 4), min_ms=round(float(ms.min()), 4),
                         max_ms=round(float(ms.max()), 4))
        line = f"  {name:8s} {med:9.3f} ms ({ms.min():.3f}-{ms.max():.3f})"
        if name != "count":
            # compact reads the payloads and writes the arena; the copy reads and writes it
            moved = payload + total if name == "compact" else 2 * total
            row[name]["read_plus_written_TBs"] = round(moved / (med * 1e-3) / 1e12, 4)
            line += f"  {moved / (med * 1e-3) / 1e12:.3f} TB/s read + written"
        print(line)
    row["compact_over_memcpy"] = round(row["compact"]["median_ms"] / row["memcpy"]["median_ms"], 4)
    row["copy_phase_over_memcpy"] = round(
        (row["compact"]["median_ms"] - row["count"]["median_ms"]) / row["memcpy"]["median_ms"], 4)
    print(f"  compact / memcpy = {row['compact_over_memcpy']:.3f}; without the walk, scan and "
          f"read-back (compact - count): {row['copy_phase_over_memcpy']:.3f}; last kernel {kernel}")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
