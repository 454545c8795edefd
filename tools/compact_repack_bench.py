#!/usr/bin/env python3
"""Time the compact-mode repack kernel (vptq_sliced_layout_repack, vptq_amd/csrc/repack.hip) on the two shapes of the issue:
v8-k65536-256 8192 x 8192 (one part) and 8192 x 28672 columns (two column parts).  Random weights; every repack is checked
against the packed indices once.  Kernel times come from a profiler run around it:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/compact_repack_bench.py

Prints one JSON line: host-timed microseconds per repack (events around `--iters` launches) and the bytes each one moves."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    from test_compact_gpu import make_layer
    dev = torch.device("cuda", 0)
    res = {}
    for name, (I, O) in (("8192x8192", (8192, 8192)), ("28672x8192", (28672, 8192))):
        m = make_layer(I, O, 8, 65536, 256, torch.float16, seed=I, dev=dev)
        ref = m.indices.detach().clone()
        assert m.compact() > 0, m.compact_skipped
        sl = m._sliced_gemv()
        out = torch.empty_like(ref)
        assert torch.equal(sl.repack(out), ref)
        for _ in range(10):
            sl.repack(out)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            sl.repack(out)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.iters
        rb = m.resident_bytes()
        res[name] = dict(parts=sl.parts, slices=sl.slices, us_per_repack_events=us, layout_bytes_read=rb["layout"],
                         packed_bytes_written=ref.numel() * 4, GBps=(rb["layout"] + ref.numel() * 4) / us / 1e3)
        del m, sl, out, ref
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
