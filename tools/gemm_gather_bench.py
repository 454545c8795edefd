#!/usr/bin/env python3
"""5 - 16 tokens of the large-codebook formats (v8-k65536-0 / -256 / -65536): the one-launch batched-decode kernel
(vptq_quant_gemm_gather, gemm_gather.hip) against the route it would replace, in ONE process on one box, the two in turns:
    5 - 8 tokens    vptq_quant_gemv (gemv_gather, TOK = 8)
    9 - 16 tokens   VQuantLinear's dense route (vptq_dequant + F.linear), and two vptq_quant_gemv launches of <= 8 tokens for reference
Ring of distinct layers in a hipGraph (the indices of one layer do not stay in the caches for the next replay), us per layer: the
median of --reps turns and their spread, (max - min) / median.  A cell "wins" where the new kernel beats the parent's route by more
than the larger of 5 % and three times the larger spread of the two.  One JSON line per cell; --md appends a markdown table.
    python tools/gemm_gather_bench.py --kr 0,256,65536 --dtypes f16,bf16 --md profiles/r15/table.md"""
import argparse, json, os, statistics, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
from vptq_amd import _backend as B  # noqa
from _gpu_util import module_desc  # noqa
from microbench import time_graph  # noqa
from shape_bench import mk  # noqa

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="8192,8192;4096,4096;4096,14336;14336,4096;28672,8192;4096,1024", help="I,O;I,O;... (input columns, outputs)")
ap.add_argument("--kr", default="0,256,65536")
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


def stat(v):
    med = statistics.median(v)
    return round(med, 2), round((max(v) - min(v)) / med, 3)


for kr in [int(v) for v in a.kr.split(",")]:
    T = 16 + (0 if kr == 0 else 8 if kr == 256 else 16)
    for dname in a.dtypes.split(","):
        dt = torch.bfloat16 if dname == "bf16" else torch.float16
        for I, O in [tuple(int(v) for v in p.split(",")) for p in a.shapes.split(";")]:
            idx_bytes = (O // 8) * (I * T // 32) * 4
            ring = max(2, min(32, a.ring_bytes // idx_bytes))
            layers = [mk(I, O, dev, g, k=65536, kr=kr) for _ in range(ring)]
            if dname == "bf16":
                layers = [m.to(torch.bfloat16) for m in layers]
            descs = [module_desc(m) for m in layers]
            assert lib.vptq_quant_gemm_gather_supported(descs[0][0], 16) == 1
            for tok in [int(t) for t in a.tokens.split(",")]:
                x = torch.randn(1, tok, I, device=dev).to(dt)
                y = torch.empty(1, tok, O, device=dev, dtype=dt)
                sp = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

                def run_new():
                    for d, _ in descs:
                        B.check(lib.vptq_quant_gemm_gather(d, x.data_ptr(), y.data_ptr(), tok, 0, sp()), "gemm_gather")

                def run_gemv():   # (launches of <= 8 tokens: what vptq_quant_gemv does with 9 - 16 itself)
                    for d, _ in descs:
                        B.check(lib.vptq_quant_gemv(d, x.data_ptr(), y.data_ptr(), tok, B.GEMV_EXACT, None, 0, sp()), "gemv")

                def run_dense():
                    for m in layers:
                        m._dense_cached(x)
                run_new()
                got = y.clone()
                run_gemv()
                torch.cuda.synchronize()
                rel = ((got.float() - y.float()).abs().max() / y.float().abs().max()).item()
                t_new, t_gemv, t_dense = [], [], []
                for _ in range(a.reps):   # the routes in turns
                    t_new.append(time_graph(run_new, a.iters) / ring)
                    t_gemv.append(time_graph(run_gemv, a.iters) / ring)
                    if tok > 8:
                        t_dense.append(time_graph(run_dense, a.iters) / ring)
                new, s_new = stat(t_new)
                gemv, s_gemv = stat(t_gemv)
                r = dict(kr=kr, dtype=dname, I=I, O=O, tokens=tok, ring=ring, new_us=new, new_spread=s_new, gemv_us=gemv, gemv_spread=s_gemv,
                         rel_diff_vs_gemv=round(rel, 6))
                parent, s_parent = gemv, s_gemv
                if tok > 8:
                    parent, s_parent = stat(t_dense)
                    r.update(dense_us=parent, dense_spread=s_parent)
                r["parent_us"] = parent
                r["wins"] = bool(new < parent * (1 - max(0.05, 3 * max(s_new, s_parent))))
                rows.append(r)
                print(json.dumps(r), flush=True)
            del layers, descs
            torch.cuda.empty_cache()

if a.md:
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "a") as f:
        f.write(f"\nBox: {box}.  us per layer, median of {a.reps} turns (spread = (max - min) / median).\n\n")
        f.write("| format | dtype | columns x outputs | tokens | gemm_gather | spread | gemv (<= 8 per launch) | spread | dense route | spread | wins |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| v8-k65536-{r['kr']} | {r['dtype']} | {r['I']} x {r['O']} | {r['tokens']} | {r['new_us']} | {r['new_spread']} | {r['gemv_us']} | "
                    f"{r['gemv_spread']} | {r.get('dense_us', '-')} | {r.get('dense_spread', '-')} | {'yes' if r['wins'] else 'no'} |\n")
