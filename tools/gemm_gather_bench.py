#!/usr/bin/env python3
"""5 - 16 tokens of the large-codebook formats: the one-launch batched-decode kernels against the route they would replace, in ONE
process on one box, the routes in turns.  The entry is the one that serves the format:
    v8-k65536-0 / -256 / -65536      vptq_quant_gemm_gather  (gemm_gather.hip)
    every other large-codebook one   vptq_quant_gemm_gatherx (gemm_gatherx.hip): v16-k65536-*, v8-k65536-4096, v8-k32768-0, ...
and the route replaced is the parent's:
    5 - 8 tokens    vptq_quant_gemv (gemv_gather TOK = 8; gemv_gatherx: one launch of 8 slots for v = 8, two of 4 for v = 16)
    9 - 16 tokens   VQuantLinear's dense route (vptq_dequant + F.linear); vptq_quant_gemv's launches of <= 8 tokens for reference
                    where it takes that many
Ring of distinct layers in a hipGraph (the indices of one layer do not stay in the caches for the next replay), us per layer: the
median of --reps turns and their spread, (max - min) / median.  A cell "wins" where the new kernel beats the parent's route by more
than the larger of 5 % and three times the larger spread of the two.  One JSON line per cell; --md appends a markdown table.
    python tools/gemm_gather_bench.py --kr 0,256,65536 --dtypes f16,bf16 --md profiles/r15/table.md
    python tools/gemm_gather_bench.py --formats v16-k65536-65536,v16-k65536-1024,v16-k65536-0,v8-k65536-4096,v8-k32768-0 \\
        --shapes "8192,8192;4096,4096;4096,14336;14336,4096;28672,8192" --md profiles/r16/table.md"""
import argparse, json, math, os, re, statistics, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
from vptq_amd import _backend as B  # noqa
from _gpu_util import module_desc  # noqa
from microbench import time_graph  # noqa
from shape_bench import mk  # noqa

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="8192,8192;4096,4096;4096,14336;14336,4096;28672,8192;4096,1024", help="I,O;I,O;... (input columns, outputs)")
ap.add_argument("--kr", default="0,256,65536", help="residual centroids of v8-k65536-* formats (when --formats is not given)")
ap.add_argument("--formats", default="", help="vV-kK-KR,... (any large-codebook format; the entry that serves it is timed)")
ap.add_argument("--dtypes", default="f16,bf16")
ap.add_argument("--tokens", default="5,8,9,12,16")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--ring-bytes", type=int, default=512 << 20)
ap.add_argument("--md", default="")
a = ap.parse_args()
dev = torch.device("cuda", 0); g = torch.Generator(device=dev).manual_seed(0); lib = B.lib()
box = f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs"
print(json.dumps(dict(box=box)), flush=True)
rows = []
formats = [tuple(int(n) for n in re.fullmatch(r"v(\d+)-k(\d+)-(\d+)", f.strip()).groups()) for f in a.formats.split(",")] if a.formats \
    else [(8, 65536, int(kr)) for kr in a.kr.split(",")]


def stat(v):
    med = statistics.median(v)
    return round(med, 2), round((max(v) - min(v)) / med, 3)


def write_md(r):
    """one table row per cell, appended as it is measured (a run that is cut short leaves what it measured)"""
    if not a.md:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "a") as f:
        if len(rows) == 1:
            f.write(f"\nBox: {box}.  us per layer, median of {a.reps} turns (spread = (max - min) / median).\n\n")
            f.write("| format | dtype | columns x outputs | tokens | entry | new | spread | gemv (<= 8 per launch) | spread | dense route | spread | wins |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        f.write(f"| {r['format']} | {r['dtype']} | {r['I']} x {r['O']} | {r['tokens']} | {r['entry']} | {r['new_us']} | {r['new_spread']} | "
                f"{r.get('gemv_us', '-')} | {r.get('gemv_spread', '-')} | {r.get('dense_us', '-')} | {r.get('dense_spread', '-')} | "
                f"{'yes' if r['wins'] else 'no'} |\n")


for v, k, kr in formats:
    T = int(math.log2(k)) + (int(math.log2(kr)) if kr else 0)
    fmt = f"v{v}-k{k}-{kr}"
    for dname in a.dtypes.split(","):
        dt = torch.bfloat16 if dname == "bf16" else torch.float16
        for I, O in [tuple(int(n) for n in p.split(",")) for p in a.shapes.split(";")]:
            idx_bytes = (O // v) * ((I * T + 31) // 32) * 4
            ring = max(2, min(32, a.ring_bytes // idx_bytes))
            layers = [mk(I, O, dev, g, k=k, kr=kr, v=v) for _ in range(ring)]
            if dname == "bf16":
                layers = [m.to(torch.bfloat16) for m in layers]
            descs = [module_desc(m) for m in layers]
            if lib.vptq_quant_gemm_gather_supported(descs[0][0], 16) == 1:
                entry, new_call = "gemm_gather", lib.vptq_quant_gemm_gather
            else:
                assert lib.vptq_quant_gemm_gatherx_supported(descs[0][0], 16) == 1, fmt
                entry, new_call = "gemm_gatherx", lib.vptq_quant_gemm_gatherx
            for tok in [int(t) for t in a.tokens.split(",")]:
                x = torch.randn(1, tok, I, device=dev).to(dt)
                y = torch.empty(1, tok, O, device=dev, dtype=dt)
                sp = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

                def run_new():
                    for d, _ in descs:
                        B.check(new_call(d, x.data_ptr(), y.data_ptr(), tok, 0, sp()), entry)

                def run_gemv():   # (launches of <= 8 tokens: what vptq_quant_gemv does with more itself, where it takes them)
                    for d, _ in descs:
                        B.check(lib.vptq_quant_gemv(d, x.data_ptr(), y.data_ptr(), tok, B.GEMV_EXACT, None, 0, sp()), "gemv")

                def run_dense():
                    for m in layers:
                        m._dense_cached(x)
                B.check(new_call(descs[0][0], x.data_ptr(), y.data_ptr(), tok, 0, sp()), entry)   # (the first layer of the ring, both routes)
                got = y.clone()
                has_gemv = lib.vptq_quant_gemv(descs[0][0], x.data_ptr(), y.data_ptr(), tok, B.GEMV_EXACT, None, 0, sp()) == 0
                if not has_gemv:
                    assert tok > 8, (fmt, tok)
                    y.copy_(layers[0]._dense_cached(x))
                torch.cuda.synchronize()
                rel = ((got.float() - y.float()).abs().max() / y.float().abs().max()).item()
                t_new, t_gemv, t_dense = [], [], []
                for _ in range(a.reps):   # the routes in turns
                    t_new.append(time_graph(run_new, a.iters) / ring)
                    if has_gemv:
                        t_gemv.append(time_graph(run_gemv, a.iters) / ring)
                    if tok > 8:
                        t_dense.append(time_graph(run_dense, a.iters) / ring)
                new, s_new = stat(t_new)
                r = dict(format=fmt, entry=entry, kr=kr, dtype=dname, I=I, O=O, tokens=tok, ring=ring, new_us=new, new_spread=s_new,
                         rel_diff_vs_parent=round(rel, 6))
                if has_gemv:
                    parent, s_parent = stat(t_gemv)
                    r.update(gemv_us=parent, gemv_spread=s_parent)
                if tok > 8:
                    parent, s_parent = stat(t_dense)
                    r.update(dense_us=parent, dense_spread=s_parent)
                r["parent_us"] = parent
                r["wins"] = bool(new < parent * (1 - max(0.05, 3 * max(s_new, s_parent))))
                rows.append(r)
                write_md(r)
                print(json.dumps(r), flush=True)
            del layers, descs
            torch.cuda.empty_cache()

