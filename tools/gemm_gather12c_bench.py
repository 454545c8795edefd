#!/usr/bin/env python3
"""5 - 16 tokens of v = 12 layers with few outputs: the column-parts entry (vptq_quant_gemm_gather12c: gemm_gather12c_kernel +
gemm_gather12c_sum_kernel in gemm_gather12c.hip; a layer with a column permutation: the x[perm] launch in front is timed with them)
against the route the same layer takes at the parent commit, in ONE process on one box, the routes in turns:
    parent  `VQuantLinear.forward` with the new knob at 0 (`_GEMM_GATHER12C_MODE = "0"`): `vptq_quant_gemm_gather12` where its cells
            route the layer, else 5 - 8 tokens two gemv_gatherx launches and 9 - 16 tokens the dense route (vptq_dequant + F.linear)
Ring of distinct layers in a hipGraph (HBM-cold: the indices of one layer do not stay in the caches for the next replay), us per layer:
the median of --reps turns and their spread, (max - min) / median.  --parts: the forced part counts to measure beside 0 (the library's
rule) - the sweep the rule is chosen from; a forced count the layer cannot be cut into differently from a smaller one is skipped.  A cell
"wins" where the entry beats its parent by more than the larger of 5 % and three times the larger spread of the two.  `bits`: a second
launch gives the same bits, and they lie within one unit of the last place + the fp32 summation bound of the product of the same x with
vptq_dequant's W summed in fp64 (first layer of the ring).  One JSON line per row; --md appends a markdown table row per measured row;
--budget-s: no new layer is started after that many seconds (the cells not reached are printed as "not measured").
--wide: the 17 - 48 token entry instead (vptq_quant_gemm_gather12w: gemm_gather12w_kernel [+ gemm_gather12w_sum_kernel] in
gemm_gather12w.hip) at 17 / 24 / 32 / 33 / 40 / 48 tokens unless --tokens says otherwise, against `VQuantLinear.forward` with ITS knob at 0
(`_GEMM_GATHER12W_MODE = "0"`): the dense route; parts 1 = no split can be asked for beside 0 and the forced counts.
    python tools/gemm_gather12c_bench.py --md profiles/r38/table.md
    python tools/gemm_gather12c_bench.py --wide --md profiles/r39/table.md"""
import argparse, ctypes, json, os, statistics, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import vptq_amd  # noqa
from vptq_amd import _backend as B, batched_decode as bd  # noqa
from _gpu_util import module_desc  # noqa
from microbench import time_graph  # noqa
from shape_bench import mk  # noqa

ap = argparse.ArgumentParser()
ap.add_argument("--formats", default="65536,4096;65536,256;65536,0", help="k,kr;... (vector length 12)")
ap.add_argument("--shapes", default="4096,4096;14336,4096;4096,1024;4096,14336;8192,8192", help="I,O;I,O;... (input columns, outputs)")
ap.add_argument("--dtypes", default="f16,bf16")
ap.add_argument("--tokens", default="")
ap.add_argument("--wide", action="store_true", help="time vptq_quant_gemm_gather12w (17 - 48 tokens) instead")
ap.add_argument("--perms", default="0,1")
ap.add_argument("--parts", default="0", help="part counts: 0 = the library's rule; the sweep: 0,2,3,4,6,8,14,16")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--ring-bytes", type=int, default=512 << 20)
ap.add_argument("--budget-s", type=float, default=0.0)
ap.add_argument("--md", default="")
a = ap.parse_args()
a.tokens = a.tokens or ("17,24,32,33,40,48" if a.wide else "5,8,9,12,16")
NAME = "gemm_gather12w" if a.wide else "gemm_gather12c"
t_start = time.time()
dev = torch.device("cuda", 0); g = torch.Generator(device=dev).manual_seed(0); lib = B.lib()
box = f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs"
print(json.dumps(dict(box=box)), flush=True)
setattr(bd, "_GEMM_GATHER12W_MODE" if a.wide else "_GEMM_GATHER12C_MODE", "0")   # the parent is the route of the parent commit
rows, skipped = [], []
V = 12


def stat(v):
    med = statistics.median(v)
    return round(med, 2), round((max(v) - min(v)) / med, 3)


def mk_layer(I, O, k, kr, perm, dev, g):
    """shape_bench.mk's layer with a random column permutation where asked (tools/gemm_gather12_bench.py's)"""
    src = mk(I, O, dev, g, k=k, kr=kr, v=V)
    if not perm:
        return src
    m = vptq_amd.VQuantLinear(I, O, vector_lens=[-1, V], num_centroids=[-1, k], num_res_centroids=[-1, kr if kr > 0 else -1],
                              group_num=1, group_size=I, outlier_size=0, indices_as_float=False, enable_norm=True, enable_perm=True,
                              is_indice_packed=True, bias=False, dtype=torch.float16, device=dev, enable_proxy_error=False)
    m.indices.data, m.centroids.weight.data = src.indices.data, src.centroids.weight.data
    if kr > 0:
        m.res_centroids.weight.data = src.res_centroids.weight.data
    m.weight_scale.data, m.weight_bias.data = src.weight_scale.data, src.weight_bias.data
    m.perm.data = torch.randperm(I, generator=g, device=dev).to(torch.uint16).view(torch.int16)
    return m


def write_md(r):
    """one table row per measured row, appended as it is measured (a run that is cut short leaves what it measured)"""
    if not a.md:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "a") as f:
        if len(rows) == 1:
            f.write(f"\nBox: {box}.  us per layer, median of {a.reps} turns (spread = (max - min) / median).\n\n")
            f.write("| format | dtype | perm | columns x outputs | index elements | tokens | parts asked | instance | new | spread | parent | parent us | spread | new / parent | bits | wins |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        f.write(f"| {r['format']} | {r['dtype']} | {r['perm']} | {r['I']} x {r['O']} | {r['elements'] / (1 << 20):.1f} M | {r['tokens']} | {r['parts']} | {r['instance']} | "
                f"{r['new_us']} | {r['new_spread']} | {r['parent']} | {r['parent_us']} | {r['parent_spread']} | {r['ratio']} | {'yes' if r['bits'] else 'NO'} | "
                f"{'yes' if r['wins'] else 'no'} |\n")


cells = [(I, O, k, kr, perm, dname)
         for k, kr in [tuple(int(n) for n in p.split(",")) for p in a.formats.split(";")]
         for I, O in [tuple(int(n) for n in p.split(",")) for p in a.shapes.split(";")]
         for perm in [int(p) for p in a.perms.split(",")] for dname in a.dtypes.split(",")]
for I, O, k, kr, perm, dname in cells:
    fmt = f"v{V}-k{k}-{kr}"
    if a.budget_s and time.time() - t_start > a.budget_s:
        skipped.append(dict(format=fmt, dtype=dname, perm=perm, I=I, O=O))
        continue
    dt = torch.bfloat16 if dname == "bf16" else torch.float16
    T = (k.bit_length() - 1) + (kr.bit_length() - 1 if kr else 0)
    N = (O + V - 1) // V
    idx_bytes = N * ((I * T + 31) // 32) * 4
    ring = max(2, min(32, a.ring_bytes // idx_bytes))
    layers = [mk_layer(I, O, k, kr, perm, dev, g) for _ in range(ring)]
    if dname == "bf16":
        layers = [m.to(torch.bfloat16) for m in layers]
    descs = [module_desc(m) for m in layers]
    d0 = descs[0][0]
    W0 = layers[0].dequant().double()
    for tok in [int(t) for t in a.tokens.split(",")]:
        x = torch.randn(1, tok, I, device=dev).to(dt)
        y = torch.empty(1, tok, O, device=dev, dtype=dt)
        sp = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
        ref, mag = x[0].double() @ W0.t(), x[0].double().abs() @ W0.abs().t()
        # one rounding of the output + fp32 sums in the kernels' order (2^-18 of the sum of the terms' magnitudes, with room)
        bound = ref.abs() * (2.0 ** (-7 if dname == "bf16" else -10)) + mag * 2.0 ** -18 + 2.0 ** -24
        parent_name = "dense" if a.wide else "gemm_gather12" if bd.gemm_gather12_route(V, k, kr, O, I, tok, bool(perm)) else "2 x gemv_gatherx" if tok <= 8 else "dense"

        def run_parent():
            for m in layers:
                m(x)
        seen, t_par = set(), None
        for parts in [int(p) for p in a.parts.split(",")]:
            text = ctypes.create_string_buffer(320)
            if getattr(lib, f"vptq_quant_{NAME}_supported")(d0, tok, parts) != 1:
                continue
            B.check(getattr(lib, f"vptq_quant_{NAME}_instance")(d0, tok, 0, parts, text, len(text)), "instance")
            inst = text.value.decode()
            if parts and inst in seen:   # (a forced count that cuts the layer as a smaller one did)
                continue
            seen.add(inst)
            need = getattr(lib, f"vptq_quant_{NAME}_workspace_bytes")(d0, tok, parts)
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            entry = getattr(lib, f"vptq_quant_{NAME}")

            def run_new():
                for d, _ in descs:
                    B.check(entry(d, x.data_ptr(), y.data_ptr(), tok, 0, parts, ws.data_ptr(), need, sp()), NAME)
            # (the first layer of the ring: the entry against dequant's W in fp64, and twice, the second time over a refilled workspace)
            B.check(entry(d0, x.data_ptr(), y.data_ptr(), tok, 0, parts, ws.data_ptr(), need, sp()), NAME)
            got = y.clone()
            ws.fill_(0xCD)
            B.check(entry(d0, x.data_ptr(), y.data_ptr(), tok, 0, parts, ws.data_ptr(), need, sp()), NAME)
            torch.cuda.synchronize()
            same = bool(torch.equal(got.view(torch.int16), y.view(torch.int16))) and bool(((got[0].double() - ref).abs() <= bound).all())
            t_new, first = [], t_par is None
            if first:
                t_par = []
            for _ in range(a.reps):   # the routes in turns (the parent once per cell: the forced counts share it)
                t_new.append(time_graph(run_new, a.iters) / ring)
                if first:
                    t_par.append(time_graph(run_parent, a.iters) / ring)
            (new, s_new), (par, s_par) = stat(t_new), stat(t_par)
            r = dict(format=fmt, k=k, kr=kr, dtype=dname, perm=perm, I=I, O=O, elements=N * I, tokens=tok, parts=parts, ring=ring,
                     instance=inst, new_us=new, new_spread=s_new, parent=parent_name, parent_us=par, parent_spread=s_par,
                     ratio=round(new / par, 3), bits=same, wins=bool(new < par * (1 - max(0.05, 3 * max(s_new, s_par)))))
            rows.append(r)
            write_md(r)
            print(json.dumps(r), flush=True)
    del layers, descs, W0
    torch.cuda.empty_cache()
print(json.dumps(dict(measured=len(rows), not_measured=skipped)), flush=True)
