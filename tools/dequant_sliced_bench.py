#!/usr/bin/env python3
"""The dense W of a large-codebook layer by three paths, as graph replays over a ring of distinct layers (each with a W of its own):
  (a) vptq_dequant over the packed indices                    - what an uncompacted layer's many-token route launches
  (b) vptq_sliced_layout_repack into a scratch + vptq_dequant - a compacted layer's route before vptq_dequant_sliced
  (c) vptq_dequant_sliced over the exact layouts              - a compacted layer's route now (vptq_amd/csrc/dequant_sliced.hip)
The three graphs are replayed in turns, `--rounds` times each; per path the median over the rounds and the spread (max - min), in us
per layer.  (c) is checked against (a) bit for bit once per row.  One JSON line per row; "ok" = median(c) <= median(b) + spread(b).

    python tools/dequant_sliced_bench.py                       # the shapes and formats of profiles/r12/README.md
    python tools/dequant_sliced_bench.py --shapes 8192,8192 --formats 8,65536,256 --dtypes f16
    python tools/dequant_sliced_bench.py --resident 32         # resident_bytes() of an 8B-shaped compact model, prefill + decode

VPTQ_TUNING=1 VPTQ_DQS_TILE=<columns> in the environment: another largest tile of the kernel (A/B)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (rows O, columns I): 4096^2, 14336 x 4096, 4096 x 14336, 8192^2, 4096 rows x 28672 columns (two column parts)
SHAPES = "4096,4096;14336,4096;4096,14336;8192,8192;4096,28672"
FORMATS = "8,65536,256;8,65536,0;8,65536,65536;16,65536,65536"   # v, k, kr
LLAMA_8B = [(4096, 4096), (1024, 4096), (1024, 4096), (4096, 4096), (14336, 4096), (14336, 4096), (4096, 14336)]   # (O, I) of q k v o gate up down


def bench_row(O, I, v, k, kr, dt, args, dev):
    from test_compact_gpu import make_layer
    from vptq_amd import _backend as B
    from vptq_amd.utils.sliced import SlicedGemv
    lib = B.lib()
    ring = []
    for i in range(args.ring):
        m = make_layer(I, O, v, k, kr, dt, seed=1000 * i + I + O + kr, dev=dev)
        sl = SlicedGemv(m, exact=True)
        desc, keep = B.make_layer_desc(bias=None, need_inv_perm=True, **m._layer_desc_keywords())
        scratch_desc = B.LayerDesc.from_buffer_copy(desc)
        W = torch.empty((O, I), dtype=dt, device=dev)
        ring.append((m, sl, desc, keep, scratch_desc, W))
    scratch = torch.empty(ring[0][0].indices.numel() + 4, dtype=torch.int32, device=dev)
    for r in ring:
        r[4].indices = scratch.data_ptr()

    def sp():
        return torch.cuda.current_stream(dev).cuda_stream

    def path_a():
        s = sp()
        for m, sl, desc, _, _, W in ring:
            B.check(lib.vptq_dequant(desc, W.data_ptr(), s), "vptq_dequant")

    def path_b():
        s = sp()
        for m, sl, _, _, sdesc, W in ring:
            B.check(lib.vptq_sliced_layout_repack(sl.desc, sl._lay_ref, sl.parts, scratch.data_ptr(), s), "vptq_sliced_layout_repack")
            B.check(lib.vptq_dequant(sdesc, W.data_ptr(), s), "vptq_dequant")

    def path_c():
        s = sp()
        for m, sl, _, _, _, W in ring:
            B.check(lib.vptq_dequant_sliced(sl.desc, sl._lay_ref, sl.parts, W.data_ptr(), s), "vptq_dequant_sliced")

    # (c) and (b) against (a), bit for bit, on the first layer
    path_a()
    want = ring[0][5].clone()
    for f in (path_b, path_c):
        ring[0][5].fill_(1.0)
        f()
        torch.cuda.synchronize()
        assert torch.equal(ring[0][5].view(torch.int16), want.view(torch.int16)), f.__name__
    st = torch.cuda.Stream()
    graphs = {}
    with torch.cuda.stream(st):
        for name, f in (("a", path_a), ("b", path_b), ("c", path_c)):
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                f()
            g.replay()
            graphs[name] = g
        torch.cuda.synchronize()
        times = {n: [] for n in graphs}
        for _ in range(args.rounds):
            for name, g in graphs.items():   # in turns: a b c a b c ...
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(args.iters):
                    g.replay()
                e1.record(st)
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / args.iters / args.ring)
    row = dict(rows=O, cols=I, v=v, k=k, kr=kr, dtype=str(dt).split(".")[-1], parts=ring[0][1].parts, slices=ring[0][1].slices)
    for n, t in times.items():
        row[n + "_us"] = round(statistics.median(t), 2)
        row[n + "_spread"] = round(max(t) - min(t), 2)
    row["c_over_b"] = round(row["c_us"] / row["b_us"], 3)
    row["c_over_a"] = round(row["c_us"] / row["a_us"], 3)
    row["W_TBps_c"] = round(2.0 * O * I / row["c_us"] / 1e6, 2)
    row["ok"] = row["c_us"] <= row["b_us"] + row["b_spread"]
    return row


def resident(layers, tokens, dev):
    """resident_bytes() summed over an 8B-shaped stack of compacted v8-k65536-256 layers after a prefill and a one-token call each"""
    from test_compact_gpu import make_layer
    from vptq_amd import _backend as B
    mods = []
    for i in range(layers):
        for j, (O, I) in enumerate(LLAMA_8B):
            m = make_layer(I, O, 8, 65536, 256, torch.float16, seed=10 * i + j, dev=dev)
            assert m.compact(force=True) > 0, m.compact_skipped
            mods.append(m)
    with torch.no_grad():
        for m in mods:
            m(torch.randn(1, tokens, m.in_features, device=dev).half())
        for m in mods:
            m(torch.randn(1, 1, m.in_features, device=dev).half())
    torch.cuda.synchronize()
    tot = dict(packed=0, layout=0, scratch=0, total=0)
    for m in mods:
        for key, val in m.resident_bytes().items():
            tot[key] += val
    return dict(resident=tot, layers=len(mods), prefill_tokens=tokens, compact_scratch_bytes=B.compact_scratch_bytes(dev.index))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="rows,cols;rows,cols;...")
    ap.add_argument("--formats", default=FORMATS, help="v,k,kr;...")
    ap.add_argument("--dtypes", default="f16,bf16")
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--resident", type=int, default=0, help="decoder layers of the 8B-shaped stack (0: the timing table)")
    ap.add_argument("--tokens", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda", 0)
    if args.resident:
        print(json.dumps(resident(args.resident, args.tokens, dev)), flush=True)
        return
    dts = {"f16": torch.float16, "bf16": torch.bfloat16}
    for dname in args.dtypes.split(","):
        for v, k, kr in [tuple(int(x) for x in f.split(",")) for f in args.formats.split(";")]:
            for O, I in [tuple(int(x) for x in s.split(",")) for s in args.shapes.split(";")]:
                print(json.dumps(bench_row(O, I, v, k, kr, dts[dname], args, dev)), flush=True)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
