#!/usr/bin/env python3
"""Same-box, same-process A/B of vptq_dequant between builds of libvptq_hip.so (GPU box only).

    python tools/ab_dequant.py --libs parent=path/to/parent/libvptq_hip.so,new=vptq_amd/libvptq_hip.so [--hidden 8192] [--reps 9]
        [--out ab_dequant.json]

Every build is loaded into ONE process (ctypes; only vptq_dequant is bound, so builds of different ABI versions load), the layers
are made once, every build gets its own captured graph of `--launches` dequant launches per case, and the replays are taken in
turns - parent, new, parent, new ... - so that drift hits every build alike.  Per case: the median and the min .. max of each
build's repeated runs; a build "sits inside" when its median lies within the FIRST build's min .. max.  Every build's W must be the
first build's bit for bit."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from vptq_amd import _backend as B  # noqa: E402
import _gpu_util  # noqa: E402
from test_compact_gpu import make_layer  # noqa: E402

CASES = [("v8-k256+256", 256, 256), ("v8-k65536-256", 65536, 256)]


def load(path):
    l = C.CDLL(os.path.abspath(path))
    l.vptq_dequant.restype, l.vptq_dequant.argtypes = B.EXPORTS["vptq_dequant"]
    l.vptq_last_error.restype = C.c_char_p
    return l


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True, help="name=path,name=path,... (the first is the yardstick)")
    ap.add_argument("--hidden", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    H = a.hidden
    libs = [(kv.split("=")[0], load(kv.split("=")[1])) for kv in a.libs.split(",")]
    stream = torch.cuda.Stream()
    report = {}
    for fmt, k, kr in CASES:
        for dt in (torch.float16, torch.bfloat16):
            case = f"{fmt} {str(dt).split('.')[-1]}"
            m = make_layer(H, H, 8, k, kr, dt, seed=k + kr, dev=dev)
            desc, keep = _gpu_util.module_desc(m, need_inv_perm=True)
            Ws = {name: torch.empty(H, H, dtype=dt, device=dev) for name, _ in libs}
            graphs = {}
            for name, l in libs:
                def run(l=l, W=Ws[name]):
                    for _ in range(a.launches):
                        rc = l.vptq_dequant(desc, W.data_ptr(), torch.cuda.current_stream().cuda_stream)
                        assert rc == 0, l.vptq_last_error()
                with torch.cuda.stream(stream):
                    run()
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=stream):
                        run()
                    g.replay()
                    torch.cuda.synchronize()
                graphs[name] = g
                assert torch.equal(Ws[name].view(torch.int16), Ws[libs[0][0]].view(torch.int16)), f"{case}: {name} writes other bits than {libs[0][0]}"
            times = {name: [] for name, _ in libs}
            for rep in range(a.reps):
                for name, _ in libs:
                    with torch.cuda.stream(stream):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        for _ in range(a.iters):
                            graphs[name].replay()
                        e1.record(stream)
                        torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / (a.iters * a.launches))
            lo, hi = min(times[libs[0][0]]), max(times[libs[0][0]])
            report[case] = {}
            for name, _ in libs:
                v = times[name]
                med = statistics.median(v)
                report[case][name] = dict(median_us=med, min_us=min(v), max_us=max(v), inside_first_builds_spread=bool(lo <= med <= hi), runs_us=v)
                print(f"{case:24s} {name:8s} median {med:7.2f} us [{min(v):7.2f} .. {max(v):7.2f}]  inside {libs[0][0]}'s spread: {lo <= med <= hi}", flush=True)
            del m, desc, keep, Ws, graphs
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(hidden=H, reps=a.reps, iters=a.iters, launches=a.launches, cases=report), f, indent=1)


if __name__ == "__main__":
    main()
