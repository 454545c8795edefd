#!/usr/bin/env python3
"""17 - 48 tokens of the large-codebook formats v8-k65536-0 / -256 / -65536: the one-launch kernel (vptq_quant_gemm_gatherw,
gemm_gatherw_kernel in gemm_gatherw.hip) against the route it would replace, in ONE process on one box, the routes in turns:
    dense   VQuantLinear's dense route (vptq_dequant + F.linear): what `VQuantLinear.forward` does with 17+ tokens of these layers
            without the entry - the parent of every cell
Ring of distinct layers in a hipGraph (the indices of one layer do not stay in the caches for the next replay), us per layer: the
median of --reps turns and their spread, (max - min) / median.  A cell "wins" where the new kernel beats its parent by more than the
larger of 5 % and three times the larger spread of the two.  `bits16`: the launch's first 16 tokens have the bits of
vptq_quant_gemm_gather on those tokens (first layer of the ring).  --perm 1: layers with a column permutation (the tables of
profiles/ were measured without).  One JSON line per cell; --md appends a markdown table.
    python tools/gemm_gatherw_bench.py --md profiles/r23/table.md"""
import argparse, ctypes, json, os, statistics, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import vptq_amd  # noqa
from vptq_amd import _backend as B  # noqa
from _gpu_util import module_desc  # noqa
from microbench import time_graph  # noqa
from shape_bench import mk  # noqa

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="8192,8192;4096,14336;14336,4096;28672,8192;4096,4096", help="I,O;I,O;... (input columns, outputs)")
ap.add_argument("--kr", default="0,256,65536", help="residual centroids of the v8-k65536-* formats")
ap.add_argument("--dtypes", default="f16,bf16")
ap.add_argument("--tokens", default="17,24,32,33,40,48")
ap.add_argument("--perm", type=int, default=0)
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


def mk_perm(I, O, kr):
    """shape_bench.mk's layer with a random column permutation"""
    m = vptq_amd.VQuantLinear(I, O, vector_lens=[-1, 8], num_centroids=[-1, 65536], num_res_centroids=[-1, kr if kr > 0 else -1],
                              group_num=1, group_size=I, outlier_size=0, indices_as_float=False, enable_norm=True, enable_perm=True,
                              is_indice_packed=True, bias=False, dtype=torch.float16, device=dev, enable_proxy_error=False)
    src = mk(I, O, dev, g, k=65536, kr=kr)
    m.indices.data, m.centroids.weight.data = src.indices.data, src.centroids.weight.data
    if kr > 0:
        m.res_centroids.weight.data = src.res_centroids.weight.data
    m.weight_scale.data, m.weight_bias.data = src.weight_scale.data, src.weight_bias.data
    m.perm.data = torch.randperm(I, generator=g, device=dev).to(torch.uint16).view(torch.int16)
    return m


def write_md(r):
    """one table row per cell, appended as it is measured (a run that is cut short leaves what it measured)"""
    if not a.md:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "a") as f:
        if len(rows) == 1:
            f.write(f"\nBox: {box}.  us per layer, median of {a.reps} turns (spread = (max - min) / median).\n\n")
            f.write("| format | dtype | columns x outputs | index elements | tokens | instance | new | spread | dense route (parent) | spread | new / parent | bits16 | wins |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        f.write(f"| {r['format']} | {r['dtype']} | {r['I']} x {r['O']} | {r['elements'] / (1 << 20):.1f} M | {r['tokens']} | {r['instance']} | {r['new_us']} | "
                f"{r['new_spread']} | {r['dense_us']} | {r['dense_spread']} | {r['ratio']} | {'yes' if r['bits16'] else 'NO'} | {'yes' if r['wins'] else 'no'} |\n")


for kr in [int(n) for n in a.kr.split(",")]:
    T = 16 + (kr.bit_length() - 1 if kr else 0)
    fmt = f"v8-k65536-{kr}"
    for dname in a.dtypes.split(","):
        dt = torch.bfloat16 if dname == "bf16" else torch.float16
        for I, O in [tuple(int(n) for n in p.split(",")) for p in a.shapes.split(";")]:
            idx_bytes = (O // 8) * ((I * T + 31) // 32) * 4
            ring = max(2, min(32, a.ring_bytes // idx_bytes))
            layers = [mk_perm(I, O, kr) if a.perm else mk(I, O, dev, g, k=65536, kr=kr) for _ in range(ring)]
            if dname == "bf16":
                layers = [m.to(torch.bfloat16) for m in layers]
            descs = [module_desc(m) for m in layers]
            for tok in [int(t) for t in a.tokens.split(",")]:
                assert lib.vptq_quant_gemm_gatherw_supported(descs[0][0], tok) == 1, (fmt, I, O, tok)
                text = ctypes.create_string_buffer(256)
                B.check(lib.vptq_quant_gemm_gatherw_instance(descs[0][0], tok, 0, text, len(text)), "instance")
                x = torch.randn(1, tok, I, device=dev).to(dt)
                y = torch.empty(1, tok, O, device=dev, dtype=dt)
                sp = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

                def run_new():
                    for d, _ in descs:
                        B.check(lib.vptq_quant_gemm_gatherw(d, x.data_ptr(), y.data_ptr(), tok, 0, sp()), "gemm_gatherw")

                def run_dense():
                    for m in layers:
                        m._dense_cached(x)
                # (the first layer of the ring: the launch's first 16 tokens against the 16-token kernel, and all against the parent)
                B.check(lib.vptq_quant_gemm_gatherw(descs[0][0], x.data_ptr(), y.data_ptr(), tok, 0, sp()), "gemm_gatherw")
                got = y.clone()
                B.check(lib.vptq_quant_gemm_gather(descs[0][0], x.data_ptr(), y.data_ptr(), 16, 0, sp()), "gemm_gather")
                torch.cuda.synchronize()
                same = bool(torch.equal(got[0, :16].view(torch.int16), y[0, :16].view(torch.int16)))
                ref = layers[0]._dense_cached(x).float()
                rel = ((got.float() - ref).abs().max() / ref.abs().max()).item()
                t_new, t_dense = [], []
                for _ in range(a.reps):   # the routes in turns
                    t_new.append(time_graph(run_new, a.iters) / ring)
                    t_dense.append(time_graph(run_dense, a.iters) / ring)
                (new, s_new), (dense, s_dense) = stat(t_new), stat(t_dense)
                r = dict(format=fmt, kr=kr, dtype=dname, perm=a.perm, I=I, O=O, elements=(O // 8) * I, tokens=tok, ring=ring,
                         instance=text.value.decode(), new_us=new, new_spread=s_new, dense_us=dense, dense_spread=s_dense, parent="dense",
                         parent_us=dense, ratio=round(new / dense, 3), bits16=same, rel_diff_vs_parent=round(rel, 6),
                         wins=bool(new < dense * (1 - max(0.05, 3 * max(s_new, s_dense)))))
                rows.append(r)
                write_md(r)
                print(json.dumps(r), flush=True)
            del layers, descs
            torch.cuda.empty_cache()
