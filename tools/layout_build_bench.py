#!/usr/bin/env python3
"""What building a sliced layout costs: the HIP builder (vptq_sliced_layout_plan / _fill, vptq_amd/csrc/layout_build.hip) against the
torch recipe (`sliced.layout_from_indices`, the parent's code path, kept in the tree) on the same device and the same indices.

    --part layers   per layer shape - 4096^2, 8192^2, 14336 x 4096, 4096 x 14336, 28672 x 8192 in v8-k65536-256; 8192^2 in
                    v8-k65536-0, v8-k65536-65536 (exact and folded), v16-k65536-65536: every layout `SlicedGemv` builds for the
                    layer; HIP events around the build, wall time (the read-back of the block count included) and the peak of
                    device memory above the level before the build, for both builders
    --part model    `prepare_model` on the Llama-3-8B shapes of tools/llama_decode.py (v8-k65536-256): seconds; the first decode
                    step with and without it, and the second one (nothing left to build)

One JSON line per measurement.  Each part is a process of its own; run them chained, each under its own time limit:

    timeout -k 10 300 python tools/layout_build_bench.py --part layers && timeout -k 10 420 python tools/layout_build_bench.py --part model
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (in x out, v, k, kr, exact)
LAYERS = [(4096, 4096, 8, 65536, 256, True), (8192, 8192, 8, 65536, 256, True), (14336, 4096, 8, 65536, 256, True),
          (4096, 14336, 8, 65536, 256, True), (28672, 8192, 8, 65536, 256, True), (8192, 8192, 8, 65536, 0, True),
          (8192, 8192, 8, 65536, 65536, True), (8192, 8192, 8, 65536, 65536, False), (8192, 8192, 16, 65536, 65536, True)]


def _measure(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated(dev) - base
    return out, dict(ms_events=e0.elapsed_time(e1), ms_wall=wall * 1e3, peak_MiB=peak / 2**20)


def part_layers(dev):
    from test_compact_gpu import make_layer
    from vptq_amd.utils import sliced as S
    hip_on = S.device_builder_enabled
    for I, O, v, k, kr, exact in LAYERS:
        m = make_layer(I, O, v, k, kr, torch.float16, seed=I + O, dev=dev)
        m._descriptor()
        res = {}
        layouts = {}
        for name in ("hip", "hip", "torch"):     # (the first kernel build of a process pays the code object's load: measured twice)
            S.device_builder_enabled = hip_on if name == "hip" else (lambda t: False)
            sl, res[name] = _measure(lambda: S.SlicedGemv(m, exact=exact), dev)
            layouts[name] = sl._tensors
            res[name]["layout_MiB"] = sl.extra_bytes / 2**20
            parts, slices, tables = sl.parts, sl.slices, len(sl._tensors)
            del sl
        S.device_builder_enabled = hip_on
        same = all((a is None and b is None) or torch.equal(a, b) for x, y in zip(layouts["hip"], layouts["torch"]) for a, b in zip(x, y))
        print(json.dumps(dict(layer=f"{I}x{O}", format=f"v{v}-k{k}-{kr}", arithmetic="exact" if exact else "folded", parts=parts,
                              slices=slices, layouts=tables, identical=same, hip=res["hip"], torch=res["torch"],
                              speedup_events=res["torch"]["ms_events"] / res["hip"]["ms_events"])), flush=True)
        del m, layouts
        torch.cuda.empty_cache()


@torch.no_grad()
def part_model(dev):
    import vptq_amd
    from llama_decode import build_model
    from vptq_amd.utils import sliced as S
    hip_on = S.device_builder_enabled
    ids = torch.randint(0, 1000, (1, 1), device=dev)
    for mode in ("prepared", "lazy-hip", "lazy-torch"):
        S.device_builder_enabled = (lambda t: False) if mode == "lazy-torch" else hip_on
        model, cfg, qlayers = build_model(0, dev, k=65536, kr=256)
        torch.cuda.synchronize()
        rep = None
        if mode == "prepared":
            t0 = time.perf_counter()
            rep = vptq_amd.prepare_model(model)
            torch.cuda.synchronize()
            rep = dict(seconds=time.perf_counter() - t0, built=rep["built"], layout_MiB=rep["bytes"] / 2**20, layers=len(rep["layers"]))
        steps = []
        past = None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model(ids, past_key_values=past, use_cache=True)
            past = out.past_key_values
            torch.cuda.synchronize()
            steps.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps(dict(model="Llama-3-8B shapes, v8-k65536-256", mode=mode, prepare_model=rep,
                              decode_step_ms=dict(first=steps[0], second=steps[1], third=steps[2]))), flush=True)
        del model, qlayers, past, out
        torch.cuda.empty_cache()
    S.device_builder_enabled = hip_on


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["layers", "model"], required=True)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    (part_layers if args.part == "layers" else part_model)(dev)


if __name__ == "__main__":
    main()
