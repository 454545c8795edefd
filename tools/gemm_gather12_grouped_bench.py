#!/usr/bin/env python3
"""5 - 16 tokens of SIBLING GROUPS of v = 12 layers (q / k / v, gate / up): the grouped entry (vptq_quant_gemm_gather12_grouped:
gemm_gather12_grouped_kernel [+ gemm_gather12_grouped_sum_kernel] in gemm_gather12_grouped.hip, behind one x[perm] launch per distinct
permutation, all timed together) against the SUM of the members' own routes on the same build, in ONE process on one box, in turns:
    parent  every member's `VQuantLinear.forward`, un-linked, with the new knob at 0 (`_GEMM_GATHER12_GROUPED_MODE = "0"`):
            `vptq_quant_gemm_gather12` / `vptq_quant_gemm_gather12c` where their cells route the member, else 5 - 8 tokens two
            gemv_gatherx launches and 9 - 16 tokens the dense route (vptq_dequant + F.linear)
Ring of distinct groups in a hipGraph (HBM-cold: the indices of one group do not stay in the caches for the next replay), us per group:
the median of --reps turns and their spread, (max - min) / median.  --parts: the part counts to measure (0: the library's rule).  A
cell "wins" where the entry beats its parent by more than the larger of 5 % and three times the larger spread of the two.  `bits`: a
second launch over a refilled workspace gives the same bits, and every member has the bits of its own entry at the same split
(vptq_quant_gemm_gather12c, at one part vptq_quant_gemm_gather12; first group of the ring).  With a permutation the members of a group
share one.  One JSON line per row; --md appends a markdown table row per measured row; --budget-s: no new group is started after that
many seconds (the cells not reached are printed as "not measured").
--wide: 17 - 48 tokens (17 / 24 / 32 / 33 / 40 / 48 unless --tokens says otherwise) through vptq_quant_gemm_gather12w_grouped
(gemm_gather12w_grouped.hip); the parent is every member's own route with the knob `_GEMM_GATHER12W_GROUPED_MODE` at 0 (the dense route,
or vptq_quant_gemm_gather12w where its knob or cells route the member), and `bits` compares every member with
vptq_quant_gemm_gather12w at the same split.
    python tools/gemm_gather12_grouped_bench.py --md profiles/r40/table.md
    python tools/gemm_gather12_grouped_bench.py --wide --md profiles/r41/table.md"""
import argparse, ctypes, json, os, statistics, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import vptq_amd  # noqa
from vptq_amd import _backend as B, batched_decode as bd, grouped_decode as gd  # noqa
from _gpu_util import module_desc  # noqa
from microbench import time_graph  # noqa
from shape_bench import mk  # noqa

ap = argparse.ArgumentParser()
ap.add_argument("--formats", default="65536,4096;65536,256;65536,0", help="k,kr;... (vector length 12)")
ap.add_argument("--groups", default="4096:4096,1024,1024;4096:14336,14336;8192:8192,1024,1024;8192:28672,28672",
                help="I:O,O[,O[,O]];... (input columns: the members' outputs) - q / k / v and gate / up of the 8B and 70B shapes")
ap.add_argument("--dtypes", default="f16,bf16")
ap.add_argument("--tokens", default="")
ap.add_argument("--wide", action="store_true", help="17 - 48 tokens: vptq_quant_gemm_gather12w_grouped")
ap.add_argument("--perms", default="0,1")
ap.add_argument("--parts", default="0")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--ring-bytes", type=int, default=512 << 20)
ap.add_argument("--budget-s", type=float, default=0.0)
ap.add_argument("--md", default="")
a = ap.parse_args()
NAME, V = "vptq_quant_gemm_gather12w_grouped" if a.wide else "vptq_quant_gemm_gather12_grouped", 12
a.tokens = a.tokens or ("17,24,32,33,40,48" if a.wide else "5,8,16")
t_start = time.time()
dev = torch.device("cuda", 0); g = torch.Generator(device=dev).manual_seed(0); lib = B.lib()
box = f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs"
print(json.dumps(dict(box=box)), flush=True)
gd._GEMM_GATHER12_GROUPED_MODE = gd._GEMM_GATHER12W_GROUPED_MODE = "0"   # the parent is every member's own route
rows, skipped = [], []


def stat(v):
    med = statistics.median(v)
    return round(med, 2), round((max(v) - min(v)) / med, 3)


def mk_layer(I, O, k, kr, perm, dt):
    """shape_bench.mk's layer, with the column permutation `perm` (a tensor, shared by the group) where there is one"""
    src = mk(I, O, dev, g, k=k, kr=kr, v=V)
    if perm is not None:
        m = vptq_amd.VQuantLinear(I, O, vector_lens=[-1, V], num_centroids=[-1, k], num_res_centroids=[-1, kr if kr > 0 else -1],
                                  group_num=1, group_size=I, outlier_size=0, indices_as_float=False, enable_norm=True, enable_perm=True,
                                  is_indice_packed=True, bias=False, dtype=torch.float16, device=dev, enable_proxy_error=False)
        m.indices.data, m.centroids.weight.data = src.indices.data, src.centroids.weight.data
        if kr > 0:
            m.res_centroids.weight.data = src.res_centroids.weight.data
        m.weight_scale.data, m.weight_bias.data = src.weight_scale.data, src.weight_bias.data
        m.perm.data = perm.clone()
        src = m
    return src.to(dt)


def group_array(ms):
    """the members' descriptors as the entry takes them: one perm pointer for the shared permutation"""
    pairs = [module_desc(m) for m in ms]
    ds = [B.LayerDesc.from_buffer_copy(d) for d, _ in pairs]
    for d in ds[1:]:
        if d.perm:
            d.perm = ds[0].perm
    return (B.LayerDesc * len(ds))(*ds), ds, pairs


def write_md(r):
    if not a.md:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "a") as f:
        if len(rows) == 1:
            f.write(f"\nBox: {box}.  us per group, median of {a.reps} turns (spread = (max - min) / median).\n\n")
            f.write("| format | dtype | perm | columns : outputs | index elements | tokens | parts asked | instance | new | spread | parent | parent us | spread | new / parent | bits | wins |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        f.write(f"| {r['format']} | {r['dtype']} | {r['perm']} | {r['I']} : {r['outs']} | {r['elements'] / (1 << 20):.1f} M | {r['tokens']} | {r['parts']} | {r['instance']} | "
                f"{r['new_us']} | {r['new_spread']} | {r['parent']} | {r['parent_us']} | {r['parent_spread']} | {r['ratio']} | {'yes' if r['bits'] else 'NO'} | "
                f"{'yes' if r['wins'] else 'no'} |\n")


def parent_name(k, kr, O, I, tok, perm):
    if a.wide:
        return "12w" if bd.gemm_gather12w_route(V, k, kr, O, I, tok, perm) else "dense"
    if bd.gemm_gather12c_route(V, k, kr, O, I, tok, perm):
        return "12c"
    return "12" if bd.gemm_gather12_route(V, k, kr, O, I, tok, perm) else "2 x gemv_gatherx" if tok <= 8 else "dense"


cells = [(I, outs, k, kr, perm, dname)
         for k, kr in [tuple(int(n) for n in p.split(",")) for p in a.formats.split(";")]
         for I, outs in [(int(p.split(":")[0]), tuple(int(n) for n in p.split(":")[1].split(","))) for p in a.groups.split(";")]
         for perm in [int(p) for p in a.perms.split(",")] for dname in a.dtypes.split(",")]
for I, outs, k, kr, perm, dname in cells:
    fmt, n = f"v{V}-k{k}-{kr}", len(outs)
    if a.budget_s and time.time() - t_start > a.budget_s:
        skipped.append(dict(format=fmt, dtype=dname, perm=perm, I=I, outs=outs))
        continue
    dt = torch.bfloat16 if dname == "bf16" else torch.float16
    T = (k.bit_length() - 1) + (kr.bit_length() - 1 if kr else 0)
    rows_total = sum((O + V - 1) // V for O in outs)
    ring = max(2, min(32, a.ring_bytes // (rows_total * ((I * T + 31) // 32) * 4)))
    groups = []
    for _ in range(ring):
        p = torch.randperm(I, generator=g, device=dev).to(torch.uint16).view(torch.int16) if perm else None
        groups.append([mk_layer(I, O, k, kr, p, dt) for O in outs])
    arrays = [group_array(ms) for ms in groups]
    for tok in [int(t) for t in a.tokens.split(",")]:
        x = torch.randn(1, tok, I, device=dev).to(dt)
        ys = [torch.empty(1, tok, O, device=dev, dtype=dt) for O in outs]
        yp = (ctypes.c_void_p * n)(*[y.data_ptr() for y in ys])
        sp = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

        def run_parent():
            for ms in groups:
                for m in ms:
                    m(x)
        t_par = None
        for parts in [int(p) for p in a.parts.split(",")]:
            descs0, ds0, _ = arrays[0]
            if getattr(lib, NAME + "_supported")(descs0, n, tok, parts) != 1:
                continue
            text = ctypes.create_string_buffer(384)
            B.check(getattr(lib, NAME + "_instance")(descs0, n, tok, 0, parts, text, len(text)), "instance")
            inst = text.value.decode()
            S = int(inst.split(" parts=")[1].split()[0])
            need = getattr(lib, NAME + "_workspace_bytes")(descs0, n, tok, parts)
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            entry = getattr(lib, NAME)

            def run_new():
                for descs, _, _ in arrays:
                    B.check(entry(descs, n, x.data_ptr(), yp, tok, 0, parts, ws.data_ptr(), need, sp()), NAME)
            # (the first group of the ring: twice, the second time over a refilled workspace, and against every member's own entry)
            B.check(entry(descs0, n, x.data_ptr(), yp, tok, 0, parts, ws.data_ptr(), need, sp()), NAME)
            got = [y.clone() for y in ys]
            ws.fill_(0xCD)
            B.check(entry(descs0, n, x.data_ptr(), yp, tok, 0, parts, ws.data_ptr(), need, sp()), NAME)
            torch.cuda.synchronize()
            same = all(torch.equal(p.view(torch.int16), q.view(torch.int16)) for p, q in zip(got, ys))
            for d, O, want in zip(ds0, outs, got):
                own, y1 = ("vptq_quant_gemm_gather12c", (S,)) if S >= 2 else ("vptq_quant_gemm_gather12", ()), torch.empty(1, tok, O, device=dev, dtype=dt)
                if a.wide:
                    own = ("vptq_quant_gemm_gather12w", (S,))
                need1 = getattr(lib, own[0] + "_workspace_bytes")(d, tok, *own[1])
                ws1 = torch.empty(max(need1, 16), dtype=torch.uint8, device=dev)
                B.check(getattr(lib, own[0])(d, x.data_ptr(), y1.data_ptr(), tok, 0, *own[1], ws1.data_ptr(), need1, sp()), own[0])
                torch.cuda.synchronize()
                same = same and torch.equal(want.view(torch.int16), y1.view(torch.int16))
            t_new, first = [], t_par is None
            if first:
                t_par = []
            for _ in range(a.reps):   # the routes in turns (the parent once per cell: the part counts share it)
                t_new.append(time_graph(run_new, a.iters) / ring)
                if first:
                    t_par.append(time_graph(run_parent, a.iters) / ring)
            (new, s_new), (par, s_par) = stat(t_new), stat(t_par)
            r = dict(format=fmt, k=k, kr=kr, dtype=dname, perm=perm, I=I, outs=",".join(map(str, outs)), elements=rows_total * I, tokens=tok,
                     parts=parts, ring=ring, instance=inst, new_us=new, new_spread=s_new,
                     parent=" + ".join(parent_name(k, kr, O, I, tok, bool(perm)) for O in outs), parent_us=par, parent_spread=s_par,
                     ratio=round(new / par, 3), bits=bool(same), wins=bool(new < par * (1 - max(0.05, 3 * max(s_new, s_par)))))
            rows.append(r)
            write_md(r)
            print(json.dumps(r), flush=True)
    del groups, arrays
    torch.cuda.empty_cache()
print(json.dumps(dict(measured=len(rows), not_measured=skipped)), flush=True)
