"""How the persistent chain launch (gemv_k256c.hip) deals its row groups, and the chains the schedule tests run.

The library reports one launch's plan (vptq_quant_gemv_chain_plan): the visit length, the grid, and per layer the
workgroup that owns block 0 and the row groups per block.  `expand` follows the kernel's enter_layer: block k of layer L
goes to workgroup (first_wg[L] + k) mod grid, and a workgroup walks the layers in order.  `coverage` derives what a plan
exercises: layer switches, image buffers handed to a third layer, partial-sum slots that wrap, switches between layers
of different sweeps per row group, partial last blocks, layers whose blocks wrap past the last workgroup.

The second half builds seeded chains (layers and activations) and runs them through the C ABI; the GPU test and the
runner it starts in a child process (_chain_schedule_run.py) share it, so both see the same bits."""
import ctypes as C

import numpy as np

ROWS = 8            # vector-rows per row group (kCRows)
SWEEP = 2048        # columns per sweep (kCSweepCols)
MAX_LAYERS = 32     # layers of one persistent launch
EXACT, MFMA, F32, DEP, SEL = 1 << 2, 1 << 3, 1 << 5, 1 << 6, 1 << 9


def groups(num_indices):
    return -(-num_indices // ROWS)


def sweeps(group_size):
    return -(-group_size // SWEEP)


def plan(descs, flags, workgroups):
    """-> dict(visit, grid, first, rpw) of one launch of the LayerDesc array `descs`; workgroups = 0: what a call uses"""
    from vptq_amd import _backend as B
    n = len(descs)
    visit, grid = C.c_int(-1), C.c_int(-1)
    first, rpw = (C.c_int * n)(), (C.c_int * n)()
    rc = B.lib().vptq_quant_gemv_chain_plan(descs, n, flags, workgroups, C.byref(visit), C.byref(grid), first, rpw)
    if rc:
        B.check(rc, "vptq_quant_gemv_chain_plan")
    return dict(visit=visit.value, grid=grid.value, first=list(first), rpw=list(rpw))


def expand(p, ng, ns):
    """-> per workgroup the list of its visits (layer, first row group, end row group, sweeps per row group), in the order
    it walks them.  ng / ns: row groups and sweeps per row group of each layer."""
    grid = p["grid"]
    per_wg = [[] for _ in range(grid)]
    for L, (f, r, g, s) in enumerate(zip(p["first"], p["rpw"], ng, ns)):
        for k in range(-(-g // r)):
            per_wg[(f + k) % grid].append((L, k * r, min((k + 1) * r, g), s))
    for v in per_wg:
        v.sort()
    return per_wg


def coverage(p, ng, ns):
    """what a plan exercises (the numbers the GPU test's coverage check looks at)"""
    per_wg = expand(p, ng, ns)
    grid = p["grid"]
    blocks = [-(-g // r) for g, r in zip(ng, p["rpw"])]
    return dict(
        visit=p["visit"], grid=grid,
        max_layers=max(len(v) for v in per_wg),                               # >= 2: a layer switch; >= 3: an image buffer reused
        max_rows=max(sum(e - b for _, b, e, _ in v) for v in per_wg),        # row groups of one workgroup (> 4: the slots wrap)
        max_block=max(e - b for v in per_wg for _, b, e, _ in v),            # row groups of one layer in one workgroup
        ns_switches=sum(any(a[3] != b[3] for a, b in zip(v, v[1:])) for v in per_wg),   # workgroups switching sweep counts
        partial=sum(g % r != 0 for g, r in zip(ng, p["rpw"])),                # layers whose last block is shorter
        wrapped=sum(f + b > grid for f, b in zip(p["first"], blocks)),        # layers whose blocks wrap past the last workgroup
    )


def fake_desc(I, O, dtype=0, bias=False):
    """a descriptor of the canonical format with aligned, never dereferenced pointers: enough for the plan query"""
    from vptq_amd import _backend as B
    d = B.LayerDesc()
    d.in_features, d.out_features, d.vector_len, d.num_codebooks, d.group_size = I, O, 8, 1, I
    d.num_centroids, d.num_res_centroids, d.index_bits, d.res_bits = 256, 256, 8, 8
    d.row_words, d.num_indices, d.dtype = I // 2, -(-O // 8), dtype
    d.indices, d.centroids, d.res_centroids = 1 << 20, 2 << 20, 3 << 20
    d.weight_scale, d.weight_bias = 4 << 20, 5 << 20
    if bias:
        d.bias = 6 << 20
    return d


def fake_descs(shapes, dtype=0):
    """-> LayerDesc array of (I, O, kwargs) shapes"""
    from vptq_amd import _backend as B
    return (B.LayerDesc * len(shapes))(*[fake_desc(I, O, dtype, kw.get("bias", False)) for I, O, kw in shapes])


def layer_counts(descs):
    """-> (row groups, sweeps per row group) of each layer"""
    return [groups(d.num_indices) for d in descs], [sweeps(d.group_size) for d in descs]


# ---------------------------------------------------------------------------------------------- the chains
LLM = dict(dist="llm")
# the route-model test's chain (tests/test_route_models_gpu.py CHAIN_SHAPES), twice over: 20 layers, 10 distinct
ROUTE_SHAPES = [(1024, 512, dict(LLM)), (4104, 264, dict(LLM, bias=True)), (8192 + 512, 264, dict(LLM)), (512, 1000, dict(LLM, bias=True)),
                (2048, 2048 * 3, dict(LLM)), (6144, 520, dict(LLM)), (256, 1032, dict(LLM)), (4096, 264, dict(LLM)), (1024, 1032, dict(LLM)),
                (2048, 2048, dict(LLM, bias=True))]
# (I, O, kwargs) per layer; a layer that appears again is the same layer (same bits) with its own activation
CHAINS = {
    "routes": ROUTE_SHAPES + ROUTE_SHAPES,
    # one Llama-3-8B decoder block: q, k, v, o, gate, up, down
    "llama8b": [(4096, 4096, dict(LLM)), (4096, 1024, dict(LLM)), (4096, 1024, dict(LLM)), (4096, 4096, dict(LLM)),
                (4096, 14336, dict(LLM)), (4096, 14336, dict(LLM)), (14336, 4096, dict(LLM))],
    # tall, narrow layers (a sweep is short): long visits at the full device.  Tails: O not a multiple of 64, I not a
    # multiple of 2048 (one layer of two sweeps per row group), bias
    "visit32": [(128, 131072, dict(LLM)), (136, 131072 - 8, dict(LLM, bias=True)), (128, 131072 + 512, dict(LLM)),
                (120, 131072, dict(LLM, bias=True)), (2056, 1032, dict(LLM)), (128, 131072 - 64, dict(LLM)),
                (64, 131072 + 72, dict(LLM)), (128, 131072, dict(LLM, bias=True)), (136, 131072, dict(LLM))],
    "visit16": [(128, 65536 + 8, dict(LLM)), (136, 65536, dict(LLM, bias=True)), (2056, 2056, dict(LLM)), (128, 65536 - 72, dict(LLM)),
                (128, 65536, dict(LLM, bias=True)), (120, 65536 + 136, dict(LLM)), (128, 65536, dict(LLM)),
                (136, 65536 + 64, dict(LLM)), (128, 65536, dict(LLM))],
    "visit8": [(256, 32768 + 8, dict(LLM)), (264, 32768, dict(LLM, bias=True)), (2056, 1032, dict(LLM)), (256, 32768 - 72, dict(LLM)),
               (128, 32768, dict(LLM, bias=True)), (248, 32768 + 136, dict(LLM)), (256, 32768, dict(LLM)),
               (136, 32768 + 64, dict(LLM)), (256, 32768, dict(LLM))],
    # dependent (x of layer i + 1 = y of layer i): the route-model test's dimensions
    "dependent": [(a, b, dict(LLM, bias=i % 3 == 0)) for i, (a, b) in
                  enumerate(zip([1024, 2048, 1032, 4096, 512, 1024, 2048, 1024, 264], [2048, 1032, 4096, 512, 1024, 2048, 1024, 264, 1024]))],
}
DEPENDENT = {"dependent"}
ARITH_FLAGS = {"exact": EXACT, "folded": 0, "selective": SEL}


def distinct(chain):
    """-> (list of distinct shapes, index of each layer's shape in it)"""
    shapes, where = [], []
    for s in CHAINS[chain]:
        key = (s[0], s[1], tuple(sorted(s[2].items())))
        keys = [(a[0], a[1], tuple(sorted(a[2].items()))) for a in shapes]
        if key not in keys:
            shapes.append(s)
            keys.append(key)
        where.append(keys.index(key))
    return shapes, where


def layer_specs(chain, dt):
    """-> the chain's oracle layers (a repeated layer is the same object)"""
    from oracle import vptq_oracle as vo
    shapes, where = distinct(chain)
    specs = []
    for j, (I, O, kw) in enumerate(shapes):
        kw = dict(kw)
        dist = kw.pop("dist", "ref-test")
        specs.append(vo.make_layer(I, O, dist=dist, seed=1000 * j + I + O, dtype=dt, **kw))
    return [specs[w] for w in where]


def activation(chain, dt, arith, i, I):
    """-> (x bits [1, 1, I], hot blocks) of layer i: planted for the folded and selective forms, dense for exact.  A layer of
    up to 512 columns gets one planted column: three would carry the rms and stand near the hot-block threshold"""
    import test_route_models_gpu as rm
    seed = 7919 * (i + 1) + I + (0 if dt == "f16" else 1)
    if arith == "exact":
        return rm._dense(I, 1, dt, seed)
    return rm._planted(I, 1, dt, seed, n=1 if I <= 512 else 3)


class Chain:
    """a chain on a device: modules, descriptors, activations; run() = one vptq_quant_gemv_chain call"""

    def __init__(self, chain, dt, dev):
        from _gpu_util import spec_to_module, module_desc
        from vptq_amd import _backend as B
        self.name, self.dt, self.dev = chain, dt, dev
        self.dependent = chain in DEPENDENT
        self.specs = layer_specs(chain, dt)
        assert len(self.specs) <= MAX_LAYERS, "one persistent launch"
        mods = {}
        for L in self.specs:
            if id(L) not in mods:
                mods[id(L)] = spec_to_module(L, dev)
        self.mods = [mods[id(L)] for L in self.specs]
        self._keep = [module_desc(m) for m in self.mods]
        self.descs = (B.LayerDesc * len(self.mods))(*[k[0] for k in self._keep])
        self.ng, self.ns = layer_counts(self.descs)

    def flags(self, arith, f32=False):
        return MFMA | ARITH_FLAGS[arith] | (F32 if f32 else 0) | (DEP if self.dependent else 0)

    def kernel_name(self, arith):
        from vptq_amd import _backend as B
        name = B.lib().vptq_quant_gemv_chain_kernel_name(self.descs, len(self.mods), 1, self.flags(arith))
        return None if name is None else name.decode()

    def plan(self, arith, workgroups=0):
        return plan(self.descs, self.flags(arith), workgroups)

    def inputs(self, arith):
        """-> [(x bits, hot blocks)] per layer (dependent: the first layer's only)"""
        n = 1 if self.dependent else len(self.specs)
        return [activation(self.name, self.dt, arith, i, self.specs[i].in_features) for i in range(n)]

    def run(self, arith, f32=False):
        """-> outputs per layer: uint16 bits, or float32 with f32"""
        import torch
        from _gpu_util import bits_to_tensor, TORCH_DT
        from vptq_amd import _backend as B
        n = len(self.mods)
        flags = self.flags(arith, f32)
        xs = [bits_to_tensor(x, self.dt, self.dev).reshape(-1) for x, _ in self.inputs(arith)]
        ys = [torch.empty(L.out_features, dtype=torch.float32 if f32 else TORCH_DT[self.dt], device=self.dev) for L in self.specs]
        xp = (C.c_void_p * n)(*[(xs[0] if self.dependent and i == 0 else ys[i - 1] if self.dependent else xs[i]).data_ptr()
                                for i in range(n)])
        yp = (C.c_void_p * n)(*[y.data_ptr() for y in ys])
        nbytes = B.lib().vptq_quant_gemv_chain_workspace_bytes_for(self.descs, n, flags)
        ws = torch.zeros(max(nbytes, 4) // 4, dtype=torch.int32, device=self.dev) if nbytes else None
        B.check(B.lib().vptq_quant_gemv_chain(self.descs, n, xp, yp, 1, flags, None if ws is None else ws.data_ptr(), nbytes,
                                              B.current_stream_ptr(self.dev)), "vptq_quant_gemv_chain")
        torch.cuda.synchronize()
        if f32:
            return [y.cpu().numpy() for y in ys]
        return [y.view(torch.int16).cpu().numpy().view(np.uint16) for y in ys]


def run_jobs(jobs, dev):
    """jobs: [(chain, dt, arith)] -> {"chain.dt.arith.y16|y32.i": array, "chain.dt.arith.plan": [visit, grid, first..., rpw...]}
    (what the child process writes and the parent process produces for the production grid)"""
    out = {}
    chains = {}
    for chain, dt, arith in jobs:
        if (chain, dt) not in chains:
            chains[(chain, dt)] = Chain(chain, dt, dev)
        ch = chains[(chain, dt)]
        assert ch.kernel_name(arith) == "gemv_k256c_kernel", (chain, dt, arith, ch.kernel_name(arith))
        p = ch.plan(arith)
        key = f"{chain}.{dt}.{arith}"
        out[key + ".plan"] = np.array([p["visit"], p["grid"]] + p["first"] + p["rpw"], dtype=np.int64)
        for f32 in (False,) if ch.dependent else (False, True):
            for i, y in enumerate(ch.run(arith, f32)):
                out[f"{key}.{'y32' if f32 else 'y16'}.{i}"] = y
    return out
