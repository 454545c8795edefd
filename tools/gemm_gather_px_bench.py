#!/usr/bin/env python3
"""5 - 48 tokens of large-codebook layers WITH a column permutation: vptq_quant_gemm_gather_px (gemm_gather_px.hip: x[perm] written
once into a workspace, then the layer's kernel in its form without a permutation) against the route such a layer takes without it,
in ONE process on one box, the routes in turns:
    parent  what `VQuantLinear.forward` does with the px route switched off (the module itself is called, so the parent is whatever
            the committed cells of the other routes say): 5 - 8 tokens the gemv_gather / gemv_gatherx launches (or the in-kernel
            permuted gemm_gatherx where its cells start at 5), 9 - 16 the in-kernel permuted gemm_gather / gemm_gatherx where their
            cells route the shape, else the dense route, 17 - 48 the dense route.  The entries it called are recorded per row.
    dense   vptq_dequant + F.linear, in every row
    plain   the inner kernel alone: the layer's own entry on the descriptor stripped of its permutation (px without the permute
            launch; not a route - its x is not permuted).  px - plain is what the permute launch costs inside the call.
Ring of distinct layers in a hipGraph (the indices of one layer do not stay in the caches for the next replay), us per layer: the
median of --reps turns and their spread, (max - min) / median.  A cell "wins" where px beats its parent by more than the larger of
5 % and three times the larger spread of the two.  `bits`: px has the bits of the layer's own entry on the same descriptor (first
layer of the ring).  One JSON line per cell; --md appends a markdown table, row by row; --budget-s stops before a new shape once
that many seconds have passed (what was measured stays).
    python tools/gemm_gather_px_bench.py --md profiles/r25/table.md"""
import argparse, ctypes, json, math, os, statistics, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import vptq_amd  # noqa
from vptq_amd import _backend as B, batched_decode  # noqa
from _gpu_util import module_desc  # noqa
from microbench import time_graph  # noqa
from shape_bench import mk  # noqa

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="4096,4096;8192,8192;4096,14336;14336,4096;28672,8192", help="I,O;I,O;... (input columns, outputs)")
ap.add_argument("--formats", default="8,65536,0;8,65536,256;8,65536,65536;16,65536,0;16,65536,1024;8,32768,0;8,65536,4096",
                help="v,k,kr;... (vector length, main centroids, residual centroids)")
ap.add_argument("--dtypes", default="f16,bf16")
ap.add_argument("--tokens", default="5,8,9,12,16,17,24,32,33,40,48")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--ring-bytes", type=int, default=512 << 20)
ap.add_argument("--budget-s", type=float, default=0.0)
ap.add_argument("--md", default="")
a = ap.parse_args()
t_start = time.time()
dev = torch.device("cuda", 0); g = torch.Generator(device=dev).manual_seed(0); lib = B.lib()
box = f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs"
print(json.dumps(dict(box=box)), flush=True)
batched_decode._GEMM_GATHER_PX_MODE = "0"   # the modules of this process take the PARENT's route; px is called through the library
rows = []
LAUNCHES = ("vptq_quant_gemm_gather_px", "vptq_quant_gemm_gatherw", "vptq_quant_gemm_gather", "vptq_quant_gemm_gatherx", "vptq_quant_gemv", "vptq_dequant")


class Spy:
    def __init__(self, real, calls):
        self.real, self.calls = real, calls

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name not in LAUNCHES:
            return fn

        def spy(*args):
            self.calls.append(name.replace("vptq_quant_", "").replace("vptq_", ""))
            return fn(*args)
        return spy


def stat(v):
    med = statistics.median(v)
    return round(med, 2), round((max(v) - min(v)) / med, 3)


def mk_perm(I, O, v, k, kr):
    """shape_bench.mk's layer with a random column permutation"""
    m = vptq_amd.VQuantLinear(I, O, vector_lens=[-1, v], num_centroids=[-1, k], num_res_centroids=[-1, kr if kr > 0 else -1],
                              group_num=1, group_size=I, outlier_size=0, indices_as_float=False, enable_norm=True, enable_perm=True,
                              is_indice_packed=True, bias=False, dtype=torch.float16, device=dev, enable_proxy_error=False)
    src = mk(I, O, dev, g, k=k, kr=kr, v=v)
    m.indices.data, m.centroids.weight.data = src.indices.data, src.centroids.weight.data
    if kr > 0:
        m.res_centroids.weight.data = src.res_centroids.weight.data
    m.weight_scale.data, m.weight_bias.data = src.weight_scale.data, src.weight_bias.data
    m.perm.data = torch.randperm(I, generator=g, device=dev).to(torch.uint16).view(torch.int16)
    return m


def stripped(desc):
    p = B.LayerDesc.from_buffer_copy(desc)
    p.weight_scale, p.weight_bias = desc.scale_permuted, desc.bias_permuted
    p.perm, p.inv_perm, p.scale_permuted, p.bias_permuted = None, None, None, None
    return p


def write_md(r):
    """one table row per cell, appended as it is measured (a run that is cut short leaves what it measured)"""
    if not a.md:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "a") as f:
        if len(rows) == 1:
            f.write(f"\nBox: {box}.  Layers with a random column permutation.  us per layer, median of {a.reps} turns (spread = (max - min) / median).\n\n")
            f.write("| format | dtype | columns x outputs | index elements | tokens | px | spread | parent route | parent | spread | px / parent | "
                    "dense route | spread | plain kernel | px - plain (permute launch) | bits | wins |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        f.write(f"| {r['format']} | {r['dtype']} | {r['I']} x {r['O']} | {r['elements'] / (1 << 20):.1f} M | {r['tokens']} | {r['px_us']} | {r['px_spread']} | "
                f"{r['parent']} | {r['parent_us']} | {r['parent_spread']} | {r['ratio']} | {r['dense_us']} | {r['dense_spread']} | {r['plain_us']} | "
                f"{r['permute_us']} | {'yes' if r['bits'] else 'NO'} | {'yes' if r['wins'] else 'no'} |\n")


for v, k, kr in [tuple(int(n) for n in p.split(",")) for p in a.formats.split(";")]:
    T = int(math.log2(k)) + (int(math.log2(kr)) if kr else 0)
    fmt = f"v{v}-k{k}-{kr}"
    for dname in a.dtypes.split(","):
        dt = torch.bfloat16 if dname == "bf16" else torch.float16
        for I, O in [tuple(int(n) for n in p.split(",")) for p in a.shapes.split(";")]:
            if a.budget_s and time.time() - t_start > a.budget_s:
                print(json.dumps(dict(stopped="budget", before=[fmt, dname, I, O])), flush=True)
                sys.exit(0)
            idx_bytes = (O // v) * ((I * T + 31) // 32) * 4
            ring = max(2, min(32, a.ring_bytes // idx_bytes))
            layers = [mk_perm(I, O, v, k, kr) for _ in range(ring)]
            if dname == "bf16":
                layers = [m.to(torch.bfloat16) for m in layers]
            descs = [module_desc(m) for m in layers]
            plains = [stripped(d) for d, _ in descs]
            for tok in [int(t) for t in a.tokens.split(",")]:
                if lib.vptq_quant_gemm_gather_px_supported(descs[0][0], tok) != 1:
                    continue   # (gemm_gatherx's formats end at 16 tokens)
                own = lib.vptq_quant_gemm_gatherw if tok > 16 else \
                    lib.vptq_quant_gemm_gather if lib.vptq_quant_gemm_gather_supported(descs[0][0], tok) else lib.vptq_quant_gemm_gatherx
                text = ctypes.create_string_buffer(256)
                B.check(lib.vptq_quant_gemm_gather_px_instance(descs[0][0], tok, 0, text, len(text)), "instance")
                x = torch.randn(1, tok, I, device=dev).to(dt)
                y = torch.empty(1, tok, O, device=dev, dtype=dt)
                need = lib.vptq_quant_gemm_gather_px_workspace_bytes(descs[0][0], tok)
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
                sp = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

                def run_px():
                    for d, _ in descs:
                        B.check(lib.vptq_quant_gemm_gather_px(d, x.data_ptr(), y.data_ptr(), tok, 0, ws.data_ptr(), need, sp()), "gemm_gather_px")

                def run_parent():
                    for m in layers:
                        m(x)

                def run_dense():
                    for m in layers:
                        m._dense_cached(x)

                def run_plain():
                    for p in plains:
                        B.check(own(p, x.data_ptr(), y.data_ptr(), tok, 0, sp()), "plain")
                # (the first layer of the ring: px against the layer's own entry, bit for bit; the entries the parent route calls)
                B.check(lib.vptq_quant_gemm_gather_px(descs[0][0], x.data_ptr(), y.data_ptr(), tok, 0, ws.data_ptr(), need, sp()), "gemm_gather_px")
                got = y.clone()
                B.check(own(descs[0][0], x.data_ptr(), y.data_ptr(), tok, 0, sp()), "own entry")
                torch.cuda.synchronize()
                same = bool(torch.equal(got.view(torch.int16), y.view(torch.int16)))
                calls, real = [], B.lib
                B.lib = lambda: Spy(lib, calls)
                try:
                    probe = mk_perm(I, O, v, k, kr)   # (a module of its own: a descriptor built under the spy keeps the spy's functions)
                    probe = probe.to(torch.bfloat16) if dname == "bf16" else probe
                    probe(x)
                finally:
                    B.lib = real
                calls = list(calls)
                del probe
                t_px, t_parent, t_dense, t_plain = [], [], [], []
                for _ in range(a.reps):   # the routes in turns
                    t_px.append(time_graph(run_px, a.iters) / ring)
                    t_parent.append(time_graph(run_parent, a.iters) / ring)
                    t_dense.append(time_graph(run_dense, a.iters) / ring)
                    t_plain.append(time_graph(run_plain, a.iters) / ring)
                (px, s_px), (parent, s_parent), (dense, s_dense), (plain, _) = stat(t_px), stat(t_parent), stat(t_dense), stat(t_plain)
                r = dict(format=fmt, v=v, k=k, kr=kr, dtype=dname, I=I, O=O, elements=(O // v) * I, tokens=tok, ring=ring, instance=text.value.decode(),
                         px_us=px, px_spread=s_px, parent="+".join(calls), parent_us=parent, parent_spread=s_parent, dense_us=dense,
                         dense_spread=s_dense, plain_us=plain, permute_us=round(px - plain, 2), ratio=round(px / parent, 3), bits=same,
                         wins=bool(px < parent * (1 - max(0.05, 3 * max(s_px, s_parent)))))
                rows.append(r)
                write_md(r)
                print(json.dumps(r), flush=True)
            del layers, descs, plains
            torch.cuda.empty_cache()
