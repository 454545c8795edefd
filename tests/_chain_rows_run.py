"""The chains of the rows-geometry tests, how the launch deals them, and the child process of test_chain_rows_gpu.py.

The first half needs no device: the pool of layers, the chains built from it, the table (chain x workgroup count -> what the entry
exists to cover), a restatement of the deal (tasks round-robin over all workgroups, the layers continuing each other's round
robin, a workgroup walking its tasks in layer order) and the covers computed from it.  tests/test_chain_rows_cpu.py holds the
restatement to vptq_quant_gemv_chain_rows_plan and asserts every cover of the table.

The second half is the child: it runs the jobs named on its command line with the persistent launch forced into the rows
geometry (VPTQ_K256C_ROWS=1 and VPTQ_K256C_WGS, read once per process, set by the parent) and writes every output to an .npz; the
parent does the checking.

    python tests/_chain_rows_run.py OUT.npz JOB...      JOB = a chain name, "special" or "variants" """
import ctypes as C
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

EXACT, MFMA = 1 << 2, 1 << 3
TASK_GROUPS, STEP_COLS, QUEUE_DEPTH = 16, 128, 3   # kRTaskGroups, kRStepCols, kCDepth
# (I, O, bias).  "switch" at 4 workgroups: 13 workgroup-tasks - 3 or 4 per workgroup, workgroup 0 walks four layers (both image
# buffers reused in both directions), layer 4 gives three workgroups one task and one two (the next task of the same layer);
# vector-rows that are no multiple of 8 or of 128, O no multiple of 8, idle waves in most layers' last task; widths of one step
# (128), columns past G (136, 2056), many steps (4096), different widths following each other.  "few": 3 tasks, so one of 4
# workgroups returns at once.
CHAINS = {
    "switch": [(128, 2100, True), (136, 1100, False), (2056, 520, True), (4096, 264, False), (136, 4100, False), (128, 1004, True)],
    "few": [(2056, 264, False), (128, 1100, True)],
}
# the pool: small layers, each the same bits and the same x wherever it stands.  Widths of 8 columns (no column before the last
# chunk), 120 (one short step), 128, 136 and 248 / 264 (one and two steps, columns past G), 2056, 4096, 8192 and 14336 (17 - 112
# steps); one vector-row (I), O = 4 mod 8 (B, D, K), last tasks of 1 row group (D, H, K), of 16 (B) and in between
POOL = {"A": (8, 72, True), "B": (128, 1004, True), "C": (136, 1100, False), "D": (264, 2100, True), "E": (2056, 520, True),
        "F": (4096, 264, False), "G": (14336, 72, True), "H": (128, 8200, False), "I": (120, 8, False), "J": (8192, 136, True),
        "K": (248, 4100, False)}
POOL_ORDER = "ABCDEFGHIJK"
_SPARSE = "A B I E A F B J I G A B E I F A J B I A E B G I A F B J I A B E".split()
NAMED = {"sparse32": _SPARSE, "sparse31": _SPARSE[:31], "sparse30": _SPARSE[:30], "dense": "A B I C H D K E A I B F C G J H I A".split()}
NAMED.update({"one" + c: [c] for c in POOL_ORDER})   # every pool layer alone in a launch
for _name, _layers in NAMED.items():
    CHAINS[_name] = [POOL[c] for c in _layers]
ONES = tuple("one" + c for c in POOL_ORDER)

# ---------------------------------------------------------------------------------------------- the table
# (chain, workgroups, covers); the workgroup counts are child processes, one per count
TABLE = [
    ("dense", 1, ("one_wg", "same_layer3", "run1", "phases", "shapes")),
    ("sparse32", 1, ("one_wg",)),
    ("dense", 2, ("visits", "phases")),
    ("dense", 3, ("same_layer3", "phases")),
    ("sparse32", 3, ("run1",)),
    ("switch", 4, ()),
    ("few", 4, ("idle_wg",)),
    ("sparse32", 8, ("search2", "late_start", "tail", "run1")),
    ("sparse31", 8, ("search2", "ragged_n")),
    ("sparse30", 8, ("search2", "ragged_n")),
    ("sparse32", 16, ("search2", "search4", "late_start", "tail")),
    ("sparse32", 37, ("late_start", "tail", "idle_wg")),
]
ONES_AT = 16    # the one-layer launches run in this count's child
WGS = tuple(sorted({w for _, w, _ in TABLE}))


def jobs_at(w):
    return [c for c, ww, _ in TABLE if ww == w] + (list(ONES) if w == ONES_AT else []) + (["special", "variants"] if w == 4 else [])


def cdiv(a, b):
    return -(-a // b)


def tasks_of(O):
    return cdiv(cdiv(cdiv(O, 8), 8), TASK_GROUPS)


def steps_of(I):
    return cdiv(I, STEP_COLS)


def deal(shapes, w):
    """-> (first, tasks, steps, per_wg): per layer the workgroup of its task 0, its tasks and its steps per task; per workgroup its
    visits [(layer, tasks there, steps per task)] in the order it walks them"""
    first, tasks, steps, run = [], [], [], 0
    per_wg = [[] for _ in range(w)]
    for L, (I, O, _) in enumerate(shapes):
        nt, ns = tasks_of(O), steps_of(I)
        first.append(run % w)
        tasks.append(nt)
        steps.append(ns)
        for k in range(nt):
            v = per_wg[(run + k) % w]
            if v and v[-1][0] == L:
                v[-1] = (L, v[-1][1] + 1, ns)
            else:
                v.append((L, 1, ns))
        run += nt
    return first, tasks, steps, per_wg


def facts(shapes, w):
    """what a deal exercises: the numbers COVERS looks at"""
    n = len(shapes)
    _, _, _, per_wg = deal(shapes, w)
    busy = [v for v in per_wg if v]
    run1 = same3 = 0
    lengths, residues = set(), set()
    for v in busy:
        r = cum = 0
        for i, (L, nt, ns) in enumerate(v):
            r = r + 1 if nt * ns == 1 else 0
            run1 = max(run1, r)
            lengths.add(nt * ns)
            cum += nt * ns
            if i + 1 < len(v):
                residues.add(cum % QUEUE_DEPTH)
                same3 = max(same3, nt)
    N = [cdiv(O, 8) for _, O, _ in shapes]
    G = [cdiv(x, 8) for x in N]
    return dict(
        n=n, ahead=max([b[0] - a[0] - 1 for v in busy for a, b in zip(v, v[1:])] + [0]), late=max(v[0][0] for v in busy),
        behind=max(n - 1 - v[-1][0] for v in busy), idle=len(per_wg) - len(busy), entered=max(len(v) for v in busy), same3=same3,
        run1=run1, lengths=lengths, residues=residues, widths={I for I, _, _ in shapes},
        shapes=(any(x % 8 for x in N) and any(O % 8 == 4 for _, O, _ in shapes) and any(O % 8 for _, O, _ in shapes) and 1 in N
                and {0, 1} <= {g % 16 for g in G} and any(g % 16 > 1 for g in G)))


COVERS = {
    "search2": lambda f: f["ahead"] >= 4,                         # the layer search goes into its second round of four headers
    "search4": lambda f: f["ahead"] >= 12,                        # ... and its fourth
    "late_start": lambda f: f["late"] >= 4,                       # a workgroup's first task is found in a later round
    "tail": lambda f: f["behind"] >= 4 and f["n"] == 32,          # the search behind a last task runs into the padding headers
    "ragged_n": lambda f: f["behind"] >= 4 and f["n"] % 4 in (2, 3),   # ... and overshoots n_layers (the clamp)
    "idle_wg": lambda f: f["idle"] > 0,                           # workgroups that return at once
    "one_wg": lambda f: f["entered"] >= 18,                       # every threshold of the free / ready counters up to use = 17
    "same_layer3": lambda f: f["same3"] >= 3,                     # >= 3 consecutive tasks of one layer, then a switch
    "run1": lambda f: f["run1"] >= 3,                             # switch, fill request and landing in the same step, thrice
    "visits": lambda f: f["lengths"] >= {1, 2, 3, 4, 5},          # a fill lands before, at and after the end of a visit
    "phases": lambda f: f["residues"] == set(range(QUEUE_DEPTH)),   # a switch at every queue slot
    "shapes": lambda f: f["shapes"] and f["widths"] >= {8, 120, 128, 136, 248, 264, 2056, 4096, 8192, 14336},
}


# ---------------------------------------------------------------------------------------------- the launch the product takes
def natural_shapes(cus):
    """32 narrow layers (I, O, bias) whose launch the rule gives to the rows geometry on a device of `cus` compute units: widths
    128 / 136 / 248 / 264 in turns, ceil(cus / 32) full tasks per layer, O 4 short of that in every third layer (a short last vector-row)
    and 8 past it in every third (one more task, of one row group): at least `cus` tasks"""
    base = cdiv(cus, 32) * 1024
    return [((128, 136, 248, 264)[i % 4], base + (-4, 8, 0)[i % 3], i % 2 == 0) for i in range(32)]


def natural_layer(cus, i):
    from oracle import vptq_oracle as vo
    I, O, bias = natural_shapes(cus)[i]
    return vo.make_layer(I, O, dist="llm", seed=17 * i + I + O, dtype="f16", bias=bias)


def natural_x(cus, i, seed=0):
    import test_route_models_gpu as rm
    return rm._dense(natural_shapes(cus)[i][0], 1, "f16", 300 + i + 1000 * seed)[0]


# ---------------------------------------------------------------------------------------------- layers and activations
SPECIAL_COLS, PERIOD, TAIL = 2040, 1856, 64   # the special-value table: 2040 columns (16 steps, the last one short)
GUARD = 64                                    # sentinel elements in front of and behind every y
SENTINEL = 12345.0                            # (exact in fp16)


@functools.lru_cache(maxsize=None)
def pool_layer(c):
    from oracle import vptq_oracle as vo
    I, O, bias = POOL[c]
    return vo.make_layer(I, O, dist="llm", seed=31 * POOL_ORDER.index(c) + I + O, dtype="f16", bias=bias)


@functools.lru_cache(maxsize=None)
def pool_x(c):
    import test_route_models_gpu as rm
    return rm._dense(POOL[c][0], 1, "f16", 100 + POOL_ORDER.index(c))[0]


def layer_of(chain, i):
    if chain in NAMED:
        return pool_layer(NAMED[chain][i])
    from oracle import vptq_oracle as vo
    I, O, bias = CHAINS[chain][i]
    return vo.make_layer(I, O, dist="llm", seed=31 * i + I + O, dtype="f16", bias=bias)


def x_of(chain, i):
    if chain in NAMED:
        return pool_x(NAMED[chain][i])
    import test_route_models_gpu as rm
    return rm._dense(CHAINS[chain][i][0], 1, "f16", 100 + i)[0]


def y_layout(outs):
    """-> (offsets, total): the element offset of every y in one buffer with GUARD elements in front of, between and behind them"""
    offs, at = [], GUARD
    for O in outs:
        offs.append(at)
        at += O + GUARD
    return offs, at


def special_layer():
    import _dequant_specials as sp
    return sp.special_layer("f16", 8, 256, 256, finite=True, cols=SPECIAL_COLS)


def special_features():
    import numpy as np
    return np.concatenate([np.arange(PERIOD), np.arange(SPECIAL_COLS - TAIL, SPECIAL_COLS)])


def variant_row():
    """the row tests/test_weight_bits_gpu.py's activation variants take through this geometry: 32 copies of a 2040-column layer"""
    import test_weight_bits_gpu as wb
    inst = f"gemv_k256c dt=f16 dep=0 mode=exact layers=32 sweeps={','.join(['1'] * 32)} perm={','.join(['0'] * 32)} geom=rows"
    return wb.Wr("k256c-rows-n32", "chain", "f16", 32, inst, cols=SPECIAL_COLS, flags=EXACT | MFMA, edges=(1024,)).values[0]


VARIANTS = ("test_subnormal_activations_vs_the_model", "test_zeros_and_the_largest_value_vs_the_model",
            "test_overflowing_weights_vs_the_model")


def guarded_ys(outs, dev):
    """-> (buffer, views): one allocation prefilled with the sentinel, every y NaN inside it"""
    import torch
    offs, total = y_layout(outs)
    buf = torch.full((total,), SENTINEL, dtype=torch.float16, device=dev)
    ys = [buf[o:o + O] for o, O in zip(offs, outs)]
    for y in ys:
        y.fill_(float("nan"))
    return buf, ys


def main(argv):
    import numpy as np
    import torch
    from vptq_amd import _backend as B
    from _gpu_util import spec_to_module, module_desc, bits_to_tensor, tensor_to_bits, gemv_abi
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lib = B.lib()
    out = {}
    path, jobs = argv[0], argv[1:]

    def chain_call(descs, n, xs, ys, flags):
        xp = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
        yp = (C.c_void_p * n)(*[y.data_ptr() for y in ys])
        B.check(lib.vptq_quant_gemv_chain(descs, n, xp, yp, 1, flags, None, 0, B.current_stream_ptr(dev)), "vptq_quant_gemv_chain")

    def instance(descs, n, flags):
        buf = C.create_string_buffer(4096)
        B.check(lib.vptq_quant_gemv_chain_instance(descs, n, 1, flags, buf, len(buf)), "vptq_quant_gemv_chain_instance")
        return buf.value.decode()

    pool = {}   # pool layer -> (module, descriptor + what it keeps alive, x, one launch per layer)

    def member(chain, i):
        c = NAMED[chain][i] if chain in NAMED else None
        if c is not None and c in pool:
            return pool[c]
        m = spec_to_module(layer_of(chain, i), dev)
        x = bits_to_tensor(x_of(chain, i), "f16", dev).reshape(-1)
        # one launch per layer in the reference's roundings
        got = (m, module_desc(m), x, tensor_to_bits(gemv_abi(m, x.reshape(1, 1, -1), EXACT | MFMA)).reshape(-1))
        if c is not None:
            pool[c] = got
        return got

    for chain in [j for j in jobs if j in CHAINS]:
        shapes = CHAINS[chain]
        n = len(shapes)
        mem = [member(chain, i) for i in range(n)]
        descs = (B.LayerDesc * n)(*[k[1][0] for k in mem])
        xs = [k[2] for k in mem]
        buf, ys = guarded_ys([O for _, O, _ in shapes], dev)
        out[f"{chain}.instance"] = np.array(instance(descs, n, EXACT | MFMA))
        chain_call(descs, n, xs, ys, EXACT | MFMA)
        torch.cuda.synchronize()
        out[f"{chain}.buf"] = tensor_to_bits(buf)
        chain_call(descs, n, xs, ys, EXACT | MFMA)                    # again into the same buffers
        torch.cuda.synchronize()
        out[f"{chain}.again"] = tensor_to_bits(buf)
        other = [torch.empty_like(y) for y in ys]
        out[f"{chain}.folded_instance"] = np.array(instance(descs, n, MFMA))
        chain_call(descs, n, xs, other, MFMA)                         # a launch of gemv_k256c_kernel (the folded form) ...
        chain_call(descs, n, xs, ys, EXACT | MFMA)                    # ... and the rows geometry behind it
        torch.cuda.synchronize()
        out[f"{chain}.after"] = tensor_to_bits(buf)
        for i in range(n):
            out[f"{chain}.single.{i}"] = mem[i][3]

    if "special" in jobs:
        # W through one-hot activations: 32 copies of the special-value layer per launch, one column each
        L = special_layer()
        m = spec_to_module(L, dev)
        desc, keep1 = module_desc(m)
        per = 32
        descs = (B.LayerDesc * per)(*([desc] * per))
        out["special.instance"] = np.array(instance(descs, per, EXACT | MFMA))
        feats = special_features()
        padded = np.concatenate([feats, np.repeat(feats[-1:], (-len(feats)) % per)])
        x = torch.zeros(len(padded), L.in_features, dtype=torch.float16, device=dev)
        x[torch.arange(len(padded), device=dev), torch.from_numpy(padded).to(dev)] = 1.0
        y = torch.full((len(padded), L.out_features), float("nan"), dtype=torch.float16, device=dev)
        for j in range(0, len(padded), per):
            chain_call(descs, per, [x[j + i] for i in range(per)], [y[j + i] for i in range(per)], EXACT | MFMA)
        torch.cuda.synchronize()
        out["special.columns"] = tensor_to_bits(y[:len(feats)])
        out["special.W"] = tensor_to_bits(m.dequant())

    if "variants" in jobs:
        # tests/test_weight_bits_gpu.py's own checks with its own expectations for gemv_k256c, run in this process so that their
        # launches take this geometry (Route asserts the instance string, " geom=rows" included); the parent asserts the verdicts
        import warnings
        import test_weight_bits_gpu as wb
        e = variant_row()
        for name in VARIANTS:
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    getattr(wb, name)(e, dev)
                out[f"variant.{name}"] = np.array("")
            except AssertionError as err:
                out[f"variant.{name}"] = np.array("AssertionError: " + str(err)[:3000])
    np.savez(path, **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
