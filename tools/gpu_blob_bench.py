#!/usr/bin/env python3
"""tools/gpu_blob_bench.py -- speed of the blob record calls on the MI355X.

Two device-resident sets, filled with forst_fill_stream and given correct CRCs
by forst_blob_record_crc_batch:
  4k      1 M records of 16..64 B keys and 4 KiB values
  mixed   1 M records of 16..64 B keys and log-uniform 256 B..64 KiB values
In one process, alternating, after 3 warm-ups, 12 HIP-event timings each of
  verify    forst_blob_verify_batch (expected sizes given, no user keys)
  write     forst_blob_record_crc_batch
  raw       forst_crc32c_batch over the same payload descriptors: the yardstick
            (it does strictly less: no header decode, no status, no stores)
Reported per call: median (min-max) in ms, the ratio to the yardstick's median,
and the algorithmic bytes (headers + payloads; payloads alone for raw) over
the median as a share of 8 TB/s.  One JSON line per set at the end.

  python tools/gpu_blob_bench.py [--records 1000000] [--reps 12] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from forst_amd import engine, workload  # noqa: E402

PEAK = 8e12  # HBM bytes / s


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def build(n, vsizes, seed):
    """-> (image, record offsets, key sizes, value sizes, payload offsets,
    payload lengths), all on the device, CRC fields filled by the writer call"""
    ks = (16 + (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(58))
          % np.uint64(49)).astype(np.uint64)
    vs = vsizes.astype(np.uint64)
    rec = np.uint64(32) + ks + vs
    offs = np.cumsum(rec) - rec
    total = int(offs[-1] + rec[-1])
    image = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    engine.fill_stream(image, 0, seed)
    heads = np.zeros((n, 24), np.uint8)
    heads[:, 0:8] = ks.astype("<u8").view(np.uint8).reshape(n, 8)
    heads[:, 8:16] = vs.astype("<u8").view(np.uint8).reshape(n, 8)
    d_offs = dev(offs)
    step = 1 << 18  # (the scatter's index tensor in pieces)
    col = torch.arange(24, device="cuda")
    for a in range(0, n, step):
        idx = (d_offs[a:a + step, None] + col).reshape(-1)
        image[idx] = torch.from_numpy(heads[a:a + step].reshape(-1)).cuda()
    st, _, _ = engine.blob_record_crc_batch(image, d_offs, header_crc=None, blob_crc=None)
    assert not st.any(), "the writer refused a record"
    return (image, d_offs, dev(ks), dev(vs), dev(offs + np.uint64(32)),
            dev((ks + vs).astype(np.uint32)), total, int((ks + vs).sum()))


def time_calls(calls, reps, warmup):
    """alternating: each round runs every call once between two events"""
    times = {name: [] for name, _ in calls}
    for r in range(warmup + reps):
        for name, fn in calls:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if r >= warmup:
                times[name].append(t0.elapsed_time(t1))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: no timing is taken anywhere else"
    engine.init_device()
    n = args.records
    sets = (("4k", np.full(n, 4096, np.uint32)),
            ("mixed", workload.log_uniform_lengths(n, 256, 65536, 0xB10B)))
    results = []
    for name, vsizes in sets:
        image, offs, ks, vs, poffs, plens, total, payload = build(n, vsizes, 0xB0B + len(results))
        st = torch.empty(n, dtype=torch.uint8, device="cuda")
        mism = torch.zeros(1, dtype=torch.int64, device="cuda")
        raw = torch.empty(n, dtype=torch.uint32, device="cuda")
        calls = (("verify", lambda: engine.blob_verify_batch(image, offs, ks, vs, status=st,
                                                             header_crc=None, blob_crc=None,
                                                             mismatches=mism)),
                 ("write", lambda: engine.blob_record_crc_batch(image, offs, status=st,
                                                                header_crc=None, blob_crc=None)),
                 ("raw", lambda: engine.crc32c_batch(image, poffs, plens, out=raw)))
        t = time_calls(calls, args.reps, args.warmup)
        torch.cuda.synchronize()
        assert int(mism[0]) == 0, "a record the writer filled did not verify"
        base = float(np.median(t["raw"]))
        row = dict(set=name, records=n, image_bytes=total, payload_bytes=payload)
        print(f"{name}: {n} records, {total / 1e9:.2f} GB image, kernel {engine.last_kernel()}")
        for call, _ in calls:
            ms = np.array(t[call])
            med = float(np.median(ms))
            nbytes = payload if call == "raw" else total
            row[call] = dict(median_ms=round(med, 4), min_ms=round(float(ms.min()), 4),
                             max_ms=round(float(ms.max()), 4), ratio_to_raw=round(med / base, 4),
                             share_of_8TBs=round(nbytes / (med * 1e-3) / PEAK, 4))
            print(f"  {call:6s} {med:8.3f} ms ({ms.min():.3f}-{ms.max():.3f})  x{med / base:.3f} of raw"
                  f"  {nbytes / (med * 1e-3) / PEAK:.3f} of 8 TB/s")
        results.append(row)
        del image, offs, ks, vs, poffs, plens, st, raw
        torch.cuda.empty_cache()
    for row in results:
        print(json.dumps(row))


if __name__ == "__main__":
    main()
