#!/usr/bin/env python3
"""17 - 64 tokens of the canonical format (v = 8, 256 + 256 centroids) in the reference's roundings: the one-launch kernel
(vptq_quant_gemm_k256w, gemm_k256w_kernel in gemm_k256.hip) against the routes it would replace, in ONE process on one box, the routes
in turns:
    gemv    vptq_quant_gemv(VPTQ_GEMV_EXACT): launches of 16 tokens of gemm_k256_kernel (it accepts up to 64)
    dense   VQuantLinear's dense route (vptq_dequant + F.linear)
The parent of a cell is the route `VQuantLinear.forward` takes without the entry: gemv up to 48 tokens, dense from 49.
Ring of distinct layers in a hipGraph (the indices of one layer do not stay in the caches for the next replay), us per layer: the
median of --reps turns and their spread, (max - min) / median.  A cell "wins" where the new kernel beats its parent by more than the
larger of 5 % and three times the larger spread of the two.  One JSON line per cell; --md appends a markdown table.
    python tools/gemm_k256w_bench.py --md profiles/r19/table.md"""
import argparse, ctypes, json, os, statistics, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
from vptq_amd import _backend as B  # noqa
from _gpu_util import module_desc  # noqa
from microbench import time_graph  # noqa
from shape_bench import mk  # noqa

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="4096,4096;4096,14336;14336,4096;8192,8192;8192,28672", help="I,O;I,O;... (input columns, outputs)")
ap.add_argument("--dtypes", default="f16,bf16")
ap.add_argument("--tokens", default="17,24,32,33,48,49,64")
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


def write_md(r):
    """one table row per cell, appended as it is measured (a run that is cut short leaves what it measured)"""
    if not a.md:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "a") as f:
        if len(rows) == 1:
            f.write(f"\nBox: {box}.  us per layer, median of {a.reps} turns (spread = (max - min) / median).\n\n")
            f.write("| dtype | columns x outputs | tokens | instance | new | spread | gemv (16 per launch) | spread | dense route | spread | parent | new / parent | wins |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        f.write(f"| {r['dtype']} | {r['I']} x {r['O']} | {r['tokens']} | {r['instance']} | {r['new_us']} | {r['new_spread']} | {r['gemv_us']} | "
                f"{r['gemv_spread']} | {r['dense_us']} | {r['dense_spread']} | {r['parent']} | {r['ratio']} | {'yes' if r['wins'] else 'no'} |\n")


for dname in a.dtypes.split(","):
    dt = torch.bfloat16 if dname == "bf16" else torch.float16
    for I, O in [tuple(int(n) for n in p.split(",")) for p in a.shapes.split(";")]:
        idx_bytes = (O // 8) * ((I * 16 + 31) // 32) * 4
        ring = max(2, min(32, a.ring_bytes // idx_bytes))
        layers = [mk(I, O, dev, g) for _ in range(ring)]
        if dname == "bf16":
            layers = [m.to(torch.bfloat16) for m in layers]
        descs = [module_desc(m) for m in layers]
        for tok in [int(t) for t in a.tokens.split(",")]:
            assert lib.vptq_quant_gemm_k256w_supported(descs[0][0], tok) == 1, (I, O, tok)
            text = ctypes.create_string_buffer(256)
            B.check(lib.vptq_quant_gemm_k256w_instance(descs[0][0], tok, 0, text, len(text)), "instance")
            x = torch.randn(1, tok, I, device=dev).to(dt)
            y = torch.empty(1, tok, O, device=dev, dtype=dt)
            sp = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

            def run_new():
                for d, _ in descs:
                    B.check(lib.vptq_quant_gemm_k256w(d, x.data_ptr(), y.data_ptr(), tok, 0, sp()), "gemm_k256w")

            def run_gemv():
                for d, _ in descs:
                    B.check(lib.vptq_quant_gemv(d, x.data_ptr(), y.data_ptr(), tok, B.GEMV_EXACT, None, 0, sp()), "gemv")

            def run_dense():
                for m in layers:
                    m._dense_cached(x)
            # (the first layer of the ring through both kernels: the same order of sums, so the same bits)
            B.check(lib.vptq_quant_gemm_k256w(descs[0][0], x.data_ptr(), y.data_ptr(), tok, 0, sp()), "gemm_k256w")
            got = y.clone()
            B.check(lib.vptq_quant_gemv(descs[0][0], x.data_ptr(), y.data_ptr(), tok, B.GEMV_EXACT, None, 0, sp()), "gemv")
            torch.cuda.synchronize()
            same = bool(torch.equal(got.view(torch.int16), y.view(torch.int16)))
            t_new, t_gemv, t_dense = [], [], []
            for _ in range(a.reps):   # the routes in turns
                t_new.append(time_graph(run_new, a.iters) / ring)
                t_gemv.append(time_graph(run_gemv, a.iters) / ring)
                t_dense.append(time_graph(run_dense, a.iters) / ring)
            (new, s_new), (gemv, s_gemv), (dense, s_dense) = stat(t_new), stat(t_gemv), stat(t_dense)
            parent, p_us, s_parent = ("gemv", gemv, s_gemv) if tok <= 48 else ("dense", dense, s_dense)
            r = dict(dtype=dname, I=I, O=O, tokens=tok, ring=ring, instance=text.value.decode(), new_us=new, new_spread=s_new,
                     gemv_us=gemv, gemv_spread=s_gemv, dense_us=dense, dense_spread=s_dense, parent=parent, parent_us=p_us,
                     ratio=round(new / p_us, 3), bits_equal_gemv=same,
                     wins=bool(new < p_us * (1 - max(0.05, 3 * max(s_new, s_parent)))))
            rows.append(r)
            write_md(r)
            print(json.dumps(r), flush=True)
        del layers, descs
        torch.cuda.empty_cache()
