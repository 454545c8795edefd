#!/usr/bin/env python3
"""5 - 16 tokens of SIBLING layers (q / k / v, gate / up) of gemm_gatherx's large-codebook formats: vptq_quant_gemm_gatherx_grouped
(gemm_gatherx_grouped.hip: gemm_gatherx's row-group body over the members' row groups as one list in ONE launch, one x[perm] gather per
distinct permutation) against the
SUM of what the members take without it, in ONE process on one box, the routes in turns:
    grouped  the library entry on the members' descriptors (with a permutation: ONE perm pointer for the group, as
             `SiblingGroup.forward_batched` hands equal permutations over)
    parent   every member through `VQuantLinear.forward` with VPTQ_GEMM_GATHERX_GROUPED=0 in the reference arithmetic, one after the
             other: whatever the committed cells of the layers' routes say (the px route, gemm_gatherx, gemv_gatherx, the dense route).  The
             entries it called are recorded per row.  The parent is never the code under test.
Ring of distinct groups in a hipGraph (the indices of one group do not stay in the caches for the next replay), us per GROUP: the
median of --reps turns and their spread, (max - min) / median.  A cell "wins" where grouped beats its parent by more than the larger
of 5 % and three times the larger spread of the two.  `bits`: every member has the bits of its own entry on the same descriptor
(first group of the ring).  One JSON line per cell; --md appends a markdown table, row by row; --budget-s stops before a new group
once that many seconds have passed (what was measured stays).
    python tools/gemm_gatherx_grouped_bench.py --md profiles/r34/table.md"""
import argparse, ctypes, json, os, statistics, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import vptq_amd  # noqa
from vptq_amd import _backend as B, grouped_decode  # noqa
from _gpu_util import module_desc  # noqa
from microbench import time_graph  # noqa
from shape_bench import mk  # noqa

ap = argparse.ArgumentParser()
ap.add_argument("--groups", default="4096:4096,1024,1024;8192:8192,1024,1024;4096:14336,14336;8192:28672,28672",
                help="I:O,O[,O[,O]];... (input columns : the members' outputs)")
ap.add_argument("--formats", default="16,65536,65536;16,65536,1024;16,65536,0;8,65536,4096;8,32768,0", help="v,k,kr;... (the five formats profiles/r16 measured)")
ap.add_argument("--dtypes", default="f16,bf16")
ap.add_argument("--perms", default="shared,none", help="shared: every member has one random column permutation; none")
ap.add_argument("--tokens", default="5,8,9,12,16")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--ring-bytes", type=int, default=512 << 20)
ap.add_argument("--budget-s", type=float, default=0.0)
ap.add_argument("--md", default="")
a = ap.parse_args()
t_start = time.time()
dev = torch.device("cuda", 0); g = torch.Generator(device=dev).manual_seed(0); lib = B.lib()
box = f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs"
print(json.dumps(dict(box=box, arithmetic=vptq_amd.arithmetic())), flush=True)
grouped_decode._GEMM_GATHERX_GROUPED_MODE = "0"   # the modules of this process take the PARENT's routes; the grouped entry is called through the library
rows = []
LAUNCHES = ("vptq_quant_gemm_gatherx_grouped", "vptq_quant_gemm_gatherw_grouped", "vptq_quant_gemm_gather_grouped", "vptq_quant_gemm_gather_px", "vptq_quant_gemm_gatherw", "vptq_quant_gemm_gather", "vptq_quant_gemm_gatherx",
            "vptq_quant_gemv", "vptq_dequant")


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


def mk_member(I, O, v, k, kr, perm, dt):
    """shape_bench.mk's layer, with the group's column permutation where it has one"""
    m = vptq_amd.VQuantLinear(I, O, vector_lens=[-1, v], num_centroids=[-1, k], num_res_centroids=[-1, kr if kr > 0 else -1],
                              group_num=1, group_size=I, outlier_size=0, indices_as_float=False, enable_norm=True, enable_perm=perm is not None,
                              is_indice_packed=True, bias=False, dtype=torch.float16, device=dev, enable_proxy_error=False)
    src = mk(I, O, dev, g, k=k, kr=kr, v=v)
    m.indices.data, m.centroids.weight.data = src.indices.data, src.centroids.weight.data
    if kr > 0:
        m.res_centroids.weight.data = src.res_centroids.weight.data
    m.weight_scale.data, m.weight_bias.data = src.weight_scale.data, src.weight_bias.data
    if perm is not None:
        m.perm.data = perm.clone()
    return m.to(torch.bfloat16) if dt == torch.bfloat16 else m


def mk_group(I, outs, v, k, kr, shared, dt):
    perm = torch.randperm(I, generator=g, device=dev).to(torch.uint16).view(torch.int16) if shared else None
    return [mk_member(I, O, v, k, kr, perm, dt) for O in outs]


def group_array(members):
    """-> (descriptor array with ONE perm pointer for the group, the members' own (desc, keep) pairs)"""
    pairs = [module_desc(m) for m in members]
    ds = [B.LayerDesc.from_buffer_copy(d) for d, _ in pairs]
    for d in ds[1:]:
        if d.perm:
            d.perm = ds[0].perm
    return (B.LayerDesc * len(ds))(*ds), ds, pairs


def write_md(r):
    """one table row per cell, appended as it is measured (a run that is cut short leaves what it measured)"""
    if not a.md:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "a") as f:
        if len(rows) == 1:
            f.write(f"\nBox: {box}.  us per group, median of {a.reps} turns (spread = (max - min) / median).\n\n")
            f.write("| format | dtype | columns : outputs | total index elements | permutation | tokens | grouped | spread | parent routes | parent (sum) | "
                    "spread | grouped / parent | bits | wins |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        f.write(f"| {r['format']} | {r['dtype']} | {r['I']} : {'+'.join(map(str, r['outs']))} | {r['elements'] / (1 << 20):.1f} M | {r['perm']} | {r['tokens']} | "
                f"{r['grouped_us']} | {r['grouped_spread']} | {r['parent']} | {r['parent_us']} | {r['parent_spread']} | {r['ratio']} | "
                f"{'yes' if r['bits'] else 'NO'} | {'yes' if r['wins'] else 'no'} |\n")


for v, k, kr in [tuple(int(n) for n in p.split(",")) for p in a.formats.split(";")]:
    T = (k.bit_length() - 1) + (kr.bit_length() - 1 if kr else 0)
    fmt = f"v{v}-k{k}-{kr}"
    for dname in a.dtypes.split(","):
        dt = torch.bfloat16 if dname == "bf16" else torch.float16
        for spec, pname in [(s, p) for s in a.groups.split(";") for p in a.perms.split(",")]:
            I, outs = int(spec.split(":")[0]), tuple(int(o) for o in spec.split(":")[1].split(","))
            if a.budget_s and time.time() - t_start > a.budget_s:
                print(json.dumps(dict(stopped="budget", before=[fmt, dname, spec, pname])), flush=True)
                sys.exit(0)
            n = len(outs)
            idx_bytes = sum(O // v for O in outs) * ((I * T + 31) // 32) * 4
            ring = max(2, min(32, a.ring_bytes // idx_bytes))
            groups = [mk_group(I, outs, v, k, kr, pname == "shared", dt) for _ in range(ring)]
            arrays = [group_array(ms) for ms in groups]
            for tok in [int(t) for t in a.tokens.split(",")]:
                if lib.vptq_quant_gemm_gatherx_grouped_supported(arrays[0][0], n, tok) != 1:
                    continue
                text = ctypes.create_string_buffer(320)
                B.check(lib.vptq_quant_gemm_gatherx_grouped_instance(arrays[0][0], n, tok, 0, text, len(text)), "instance")
                x = torch.randn(1, tok, I, device=dev).to(dt)
                ys = [torch.empty(1, tok, O, device=dev, dtype=dt) for O in outs]
                yp = (ctypes.c_void_p * n)(*[y.data_ptr() for y in ys])
                need = lib.vptq_quant_gemm_gatherx_grouped_workspace_bytes(arrays[0][0], n, tok)
                ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
                sp = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

                def run_grouped():
                    for descs, _, _ in arrays:
                        B.check(lib.vptq_quant_gemm_gatherx_grouped(descs, n, x.data_ptr(), yp, tok, 0, ws.data_ptr(), need, sp()), "gemm_gatherx_grouped")

                def run_parent():
                    for ms in groups:
                        for m in ms:
                            m(x)
                # (the first group of the ring: every member against its own entry, bit for bit; the entries the parent routes call)
                descs, ds, _ = arrays[0]
                B.check(lib.vptq_quant_gemm_gatherx_grouped(descs, n, x.data_ptr(), yp, tok, 0, ws.data_ptr(), need, sp()), "gemm_gatherx_grouped")
                got = [y.clone() for y in ys]
                same = True
                for d, y, want in zip(ds, ys, got):
                    if d.perm:
                        pneed = lib.vptq_quant_gemm_gather_px_workspace_bytes(d, tok)
                        assert pneed <= ws.numel(), (pneed, ws.numel())   # (the group's workspace serves the member's own call)
                        B.check(lib.vptq_quant_gemm_gather_px(d, x.data_ptr(), y.data_ptr(), tok, 0, ws.data_ptr(), pneed, sp()), "own entry")
                    else:
                        B.check(lib.vptq_quant_gemm_gatherx(d, x.data_ptr(), y.data_ptr(), tok, 0, sp()), "own entry")
                    torch.cuda.synchronize()
                    same = same and bool(torch.equal(want.view(torch.int16), y.view(torch.int16)))
                calls, real = [], B.lib
                B.lib = lambda: Spy(lib, calls)
                try:
                    probe = mk_group(I, outs, v, k, kr, pname == "shared", dt)   # (modules of their own: a descriptor built under the spy keeps the spy's functions)
                    for m in probe:
                        m(x)
                finally:
                    B.lib = real
                calls = list(calls)
                del probe
                t_grouped, t_parent = [], []
                for _ in range(a.reps):   # the routes in turns
                    t_grouped.append(time_graph(run_grouped, a.iters) / ring)
                    t_parent.append(time_graph(run_parent, a.iters) / ring)
                (grouped, s_grouped), (parent, s_parent) = stat(t_grouped), stat(t_parent)
                r = dict(format=fmt, v=v, k=k, kr=kr, dtype=dname, I=I, outs=outs, elements=sum((O + v - 1) // v for O in outs) * I, perm=pname, tokens=tok, ring=ring,
                         instance=text.value.decode(), grouped_us=grouped, grouped_spread=s_grouped, parent="+".join(calls), parent_us=parent,
                         parent_spread=s_parent, ratio=round(grouped / parent, 3), bits=same,
                         wins=bool(grouped < parent * (1 - max(0.05, 3 * max(s_grouped, s_parent)))))
                rows.append(r)
                write_md(r)
                print(json.dumps(r), flush=True)
            del groups, arrays
            torch.cuda.empty_cache()
