#!/usr/bin/env python3
"""tools/wal_frame_time.py -- speed of forst_wal_frame_batch on the MI355X
against the path it replaces and against its inverse.

A C5-shaped log (forst_amd/workload.py make_wal_batch: record lengths
log-uniform 32 B..32 KiB, framed by log::Writer's rules) is built, recovered and
compacted on the device; the compacted reps (base, rep_offsets, rep_sizes) are
the write group.  Before timing, the image forst_wal_frame_batch makes of them
is compared with the log they came from, byte for byte.  After the warm-up
rounds, in one process and alternating, each round times by HIP events
  frame     forst_wal_frame_batch into a preallocated image with the host
            sizes given (the whole call: host placement, the upload of the
            start positions, descriptors, copy kernel, CRC pass, read-back)
  place     the same call without an image (placement and descriptors only)
  crc       forst_wal_record_crc_lengths over the image with the descriptors
            the frame call wrote, in place: the CRC pass on its own
  compact   forst_wal_records_compact of the image: the inverse copy, the
            natural ceiling of this access pattern
  parent    what WalWriteGroup::Frame does for the same records, at its
            cheapest: ONE host memcpy of the payload bytes into the host image
            (Frame does one per fragment, and writes the headers), the upload
            of the image and of the descriptor arrays from pageable memory,
            the CRC launch (forst_wal_record_crc_lengths, crc_out) and the
            read-back of the CRCs -- a lower bound of the parent path, so the
            comparison errs against the new call
The copy kernel's share is frame - place - crc (the three are timed apart
because the call's kernels run back to back inside it).  Reported per call:
median (min-max) in ms, image bytes per second for frame, its copy share and
compact.  One JSON line at the end.

The run stops on the first failing HIP or engine call and at the time limit.

  python tools/wal_frame_time.py [--records 500000] [--reps 10] [--warmup 3] [--limit 420]
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

H2D, D2H = 1, 2  # hipMemcpyHostToDevice, hipMemcpyDeviceToHost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=500_000)
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
    rec_flag = int(args.recyclable)
    w = workload.make_wal_batch(args.records, workload.SEEDS["C5"], recyclable=args.recyclable,
                                log_number=7)
    log = w.log
    rec, _, res = engine.wal_recover_batch(log, 7)
    n = res.n_records
    assert n == args.records and res.n_reports == 0, (n, res.n_reports)
    base, rep_off, rep_size, status = engine.wal_records_compact(log, rec)
    assert not bool(status.any()), "a record's layout was not followed"
    host_sizes = rep_size.cpu()
    payload = int(host_sizes.to(torch.int64).sum().item())
    # the result at the timed size is the right one: the image is the log
    image, desc, fres = engine.wal_frame_batch(base, rep_off, rep_size, args.recyclable, 7,
                                               host_sizes=host_sizes)
    total, nph = fres.image_bytes, fres.n_physical
    assert total == log.numel() and fres.bad_records == 0, (total, log.numel())
    assert bool((image == log).all()), "the framed image differs from the log"
    stream = torch.cuda.current_stream().cuda_stream
    L = lib()
    fr = engine.WalFrameResult()
    ins = (base.data_ptr(), base.numel(), rep_off.data_ptr(), rep_size.data_ptr(),
           host_sizes.data_ptr(), n, rec_flag, 7, 0)
    outs = (desc["rec_offsets"].data_ptr(), desc["phys_offsets"].data_ptr(),
            desc["phys_lengths"].data_ptr(), desc["phys_types"].data_ptr(), nph,
            desc["status"].data_ptr(), ctypes.byref(fr), stream)
    # the inverse call's outputs
    c_off = torch.empty(n, dtype=torch.int64, device="cuda")
    c_size = torch.empty(n, dtype=torch.int32, device="cuda")
    c_st = torch.empty(n, dtype=torch.uint8, device="cuda")
    arena = torch.empty(base.numel(), dtype=torch.uint8, device="cuda")
    got = ctypes.c_uint64()
    # the parent path's host side: the staged reps, the host image, the descriptors
    h_base = base.cpu().numpy()
    h_image = np.zeros(total, np.uint8)
    h_off = desc["phys_offsets"].cpu().numpy()
    h_len = desc["phys_lengths"].cpu().numpy()
    h_crc = np.zeros(nph, np.uint32)
    d_image = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(nph, dtype=torch.int64, device="cuda")
    d_len = torch.empty(nph, dtype=torch.int32, device="cuda")
    d_crc = torch.empty(nph, dtype=torch.int32, device="cuda")

    def hip_copy(dst, src, nbytes, kind):
        rc = hip.hipMemcpyAsync(dst, src, nbytes, kind, stream)
        if rc != 0:
            raise RuntimeError(f"hipMemcpyAsync failed ({rc})")

    def frame():
        check(L.forst_wal_frame_batch(*ins, image.data_ptr(), total, *outs))
        assert fr.image_bytes == total

    def place():
        check(L.forst_wal_frame_batch(*ins, None, 0, *outs))

    def crc():
        check(L.forst_wal_record_crc_lengths(image.data_ptr(), total, desc["phys_offsets"].data_ptr(),
                                             desc["phys_lengths"].data_ptr(), nph, rec_flag, 1,
                                             None, stream))

    def compact():
        check(L.forst_wal_records_compact(
            image.data_ptr(), total, rec["offset"].data_ptr(), rec["length"].data_ptr(),
            rec["n_fragments"].data_ptr(), n, arena.data_ptr(), arena.numel(), c_off.data_ptr(),
            c_size.data_ptr(), c_st.data_ptr(), ctypes.byref(got), stream))

    def parent():
        h_image[:payload] = h_base[:payload]
        hip_copy(d_image.data_ptr(), h_image.ctypes.data, total, H2D)
        hip_copy(d_off.data_ptr(), h_off.ctypes.data, 8 * nph, H2D)
        hip_copy(d_len.data_ptr(), h_len.ctypes.data, 4 * nph, H2D)
        check(L.forst_wal_record_crc_lengths(d_image.data_ptr(), total, d_off.data_ptr(),
                                             d_len.data_ptr(), nph, rec_flag, 0, d_crc.data_ptr(),
                                             stream))
        hip_copy(h_crc.ctypes.data, d_crc.data_ptr(), 4 * nph, D2H)

    calls = (("frame", frame), ("place", place), ("crc", crc), ("compact", compact),
             ("parent", parent))
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
    row = dict(records=n, image_bytes=total, payload_bytes=payload, physical_records=nph,
               recyclable=bool(args.recyclable), reps=args.reps, warmup=args.warmup)
    print(f"C5-shaped write group: {n} records, {total / 1e9:.3f} GB image, {nph} physical "
          f"records; device {torch.cuda.get_device_name(0)}")
    med = {}
    for name, _ in calls:
        ms = np.array(times[name])
        med[name] = float(np.median(ms))
        row[name] = dict(median_ms=round(med[name], 4), min_ms=round(float(ms.min()), 4),
                         max_ms=round(float(ms.max()), 4))
        line = f"  {name:8s} {med[name]:9.3f} ms ({ms.min():.3f}-{ms.max():.3f})"
        if name in ("frame", "compact"):
            row[name]["image_GBs"] = round(total / (med[name] * 1e-3) / 1e9, 2)
            line += f"  {row[name]['image_GBs']:.1f} GB/s of image"
        print(line)
    copy_ms = med["frame"] - med["place"] - med["crc"]
    row["copy_share_ms"] = round(copy_ms, 4)
    row["copy_share_image_GBs"] = round(total / (copy_ms * 1e-3) / 1e9, 2) if copy_ms > 0 else None
    row["frame_over_parent"] = round(med["frame"] / med["parent"], 4)
    row["copy_share_over_compact"] = round(copy_ms / med["compact"], 4)
    print(f"  copy kernel's share (frame - place - crc) {copy_ms:.3f} ms; frame / parent = "
          f"{row['frame_over_parent']:.3f}; copy share / compact = "
          f"{row['copy_share_over_compact']:.3f}")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
