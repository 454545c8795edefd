"""The instantiation-level twin of test_route_table_reaches_every_kernel, without a GPU: which instances of the canonical
format's five kernels the dispatch can be asked for on a 256-CU device - enumerated through vptq_quant_gemv*_instance, i.e. by
the library's own *_supported rules and launch-shape code - and whether the per-output tables (test_route_models_gpu.py,
test_route_models_k256_gpu.py) reach each of them.

A CELL is a projection of an instance onto a group of axes that share code (a VIEW): the full template-argument tuple of an
instantiation, a permutation with the staging-phase count and the scale / bias staging, an entry point with the arithmetic, the
row groups a workgroup walks with the arithmetic, ...  Enumerated cells the tables leave out must be named in NOT_COVERED with
a reason; that list may hold at most 10 % of the cells and no whole value of any axis.  A shape class added to a kernel later
appears in the enumeration and fails this test until someone adds its row.

The launch-shape facts (units, slots, passes, rgs) depend on the CU count.  Without a device the library takes 256, the
MI355X's; with a device it asks it.  The tables' instance strings, and so this census, are those of a 256-CU device: on another
part test_table_instances_are_what_the_library_answers says so at its first row (its probe of the CU count).

The second half does the same for the sliced family - gemv_sliced, gemv_sliced_tok, gemv_hot - through
vptq_quant_gemv_sliced_instance / _tokens_instance and the rows of tests/test_route_models_sliced_gpu.py (their launch shapes do
not depend on the CU count: the layouts' rows per wave come with the layout structs).

The third part does it for the remaining families - gemv_gather, gemv_gatherx, gemv_generic, gemv_lds, gemv_lds_mfma and the v2
entry's gemv_v2 - through vptq_quant_gemv_instance / vptq_quant_gemv_v2_instance and the rows of
tests/test_route_models_other_gpu.py (gemv_lds' rows per row group depend on the CU count: 256 here).

The fourth part does it for vptq_dequant - dequant_kernel<DT, V, TAB> and the paths its threads take to their index elements - through
vptq_dequant_instance and the rows of tests/test_dequant_models_gpu.py (nothing there depends on the CU count)."""
import ctypes as C
import os

import pytest

from vptq_amd import _backend as B
import test_route_models_gpu as rm
import test_route_models_k256_gpu as k256
import test_route_models_sliced_gpu as sliced
from test_route_models_gpu import EXACT, MFMA, VALU, BATCHED, SEL


@pytest.fixture
def untuned():
    """the library reads its tuning knobs (VPTQ_K256_KERNEL, VPTQ_K256_ROWS, VPTQ_K256M_WGS, ...) only with VPTQ_TUNING=1
    (csrc/tune_env.h); a census of a tuned dispatch would be a census of something else: fail loudly, do not skip"""
    assert os.environ.get("VPTQ_TUNING") != "1", "unset VPTQ_TUNING: the census describes the untuned dispatch"


DTYPES = {"f16": 0, "bf16": 1}


def fake_desc(I, O, dt="f16", perm=False):
    """a descriptor of the canonical 2-bit format with fake (aligned, never dereferenced) pointers"""
    d = B.LayerDesc()
    d.in_features, d.out_features, d.vector_len, d.num_codebooks, d.group_size = I, O, 8, 1, I
    d.num_centroids, d.num_res_centroids, d.index_bits, d.res_bits = 256, 256, 8, 8
    d.row_words, d.num_indices, d.dtype = I // 2, (O + 7) // 8, DTYPES[dt]
    d.indices, d.centroids, d.res_centroids = 1 << 20, 2 << 20, 3 << 20
    d.weight_scale, d.weight_bias = 4 << 20, 5 << 20
    if perm:
        d.perm, d.scale_permuted, d.bias_permuted = 6 << 20, 7 << 20, 8 << 20
    return d


def parse(instance):
    """'name k=v ...' -> (name, {k: v})"""
    name, *kv = instance.split()
    return name, dict(p.split("=", 1) for p in kv)


def bucket(name, f, tokens):
    """the axes as the census counts them: row groups per workgroup as 1 / 2 / 3+, sweep and row-group counts of gemm_k256t as
    1 / n, and the tokens asked for beside the token slots"""
    f = dict(f, tokens=str(tokens))
    if "units" in f:
        f["units"] = f["units"] if int(f["units"]) < 3 else "3+"
    for k in ("sweeps", "rgs"):
        if name == "gemm_k256t":
            f[k] = "1" if f[k] == "1" else "n"
    return f


VIEWS = {
    "gemv_k256m": [("dt", "fast", "sel", "tok", "ns", "nst", "sb"),          # every instantiation (without PERM)
                   ("perm", "fast", "sel", "tok", "nst", "sb"),              # PERM x staging phases x scale / bias staging x form
                   ("perm", "dt", "fast", "sel"),
                   ("entry", "dt", "fast", "sel", "perm"),                   # both entry points
                   ("units", "fast", "sel", "tok"),                          # one / two / more row groups per workgroup
                   ("slots",), ("tok", "tokens")],
    "gemv_k256": [("dt", "rows", "tok", "sw", "perm", "fast"), ("entry", "dt", "fast", "rows", "sw"), ("tok", "tokens")],
    "gemm_k256": [("dt", "perm", "tok"), ("passes",)],
    "gemm_k256t": [("dt", "perm", "tok"), ("sweeps",), ("rgs",)],
}


def cells_of(instance, tokens):
    out = set()
    for one in instance.split(" | "):
        name, f = parse(one)
        if name in VIEWS:
            f = bucket(name, f, tokens)
            for vi, view in enumerate(VIEWS[name]):
                out.add((name, vi, tuple(f[k] for k in view)))
    return out


# widths of 1 ... 7 sweeps (both ragged forms) and the unstaged one; heights of 1, 2 and 3 row groups per workgroup on 256 CUs
WIDTHS = [2040, 8, 4096, 2056, 4104, 6136, 8192, 8184, 8200, 10240, 11008, 12280, 14336, 12296, 14344, 28672]
HEIGHTS = [264, 32 * 257 + 8, 32 * 513 - 8, 32 * 769 + 16]


def enumerate_cells():
    """every cell the dispatch produces over the grid of requests"""
    cells = set()
    for dt in DTYPES:
        for perm in (False, True):
            for tokens in (1, 2, 3, 4):
                for flags in (MFMA, MFMA | EXACT, MFMA | SEL, VALU, VALU | EXACT):
                    for I in WIDTHS:
                        for O in HEIGHTS:
                            d = fake_desc(I, O, dt, perm)
                            cells |= cells_of(k256.instance_of([d], tokens, flags), tokens)
                            if tokens == 1:
                                cells |= cells_of(k256.instance_of([d, d], 1, flags, "grouped"), 1)
            for tokens in (5, 8, 16):
                for k in range(1, 8):
                    cells |= cells_of(k256.instance_of([fake_desc(512, 32 * (256 * (k - 1) + 96) + 8, dt, perm)], tokens, EXACT), tokens)
            for tokens in (1, 2, 16):
                for I in (2048, 6136):
                    for O in (264, 32 * 257 + 8):
                        cells |= cells_of(k256.instance_of([fake_desc(I, O, dt, perm)], tokens, BATCHED), tokens)
    return cells


def table_cells():
    cells = set()
    for p in rm.ONE_LAYER + k256.K256_ONE_LAYER:
        e = p.values[0]
        if "instance" in e:
            cells |= cells_of(e["instance"], e["tokens"])
    for g in k256.K256_GROUPS:
        cells |= cells_of(g[5], g[2])
    return cells


# (kernel, view, cell, reason): enumerated cells the tables leave out
NOT_COVERED = [
    ("gemv_k256", 1, ("1", "f16", "0", "2", "2"), "ROWS = 2 x SW = 2 through the one-layer entry needs 1023 vector-rows of more than 4096 "
     "columns: a 33 M-weight model; the instantiation is reached through the grouped entry (two layers of 512 vector-rows)"),
    ("gemv_k256", 1, ("1", "f16", "1", "2", "2"), "as above, folded form"),
]


def test_tables_reach_every_instance_the_dispatch_produces(untuned):
    want, have = enumerate_cells(), table_cells()
    named = {(k, v, c) for k, v, c, _ in NOT_COVERED}
    assert all(reason for _, _, _, reason in NOT_COVERED)
    assert named <= want, f"NOT_COVERED names cells the dispatch does not produce: {sorted(named - want)}"
    assert not (named & have), f"NOT_COVERED names covered cells: {sorted(named & have)}"
    missing = want - have - named
    assert not missing, f"{len(missing)} instance cells without a table row, e.g. {sorted(missing)[:12]}"
    assert len(want) >= 150, len(want)
    assert len(named) * 10 <= len(want), f"NOT_COVERED holds {len(named)} of {len(want)} cells: more than 10 %"
    # no whole value of any axis is left out
    for kernel, views in VIEWS.items():
        for vi, view in enumerate(views):
            for pos, axis in enumerate(view):
                w = {c[pos] for k, v, c in want if k == kernel and v == vi}
                h = {c[pos] for k, v, c in have if k == kernel and v == vi}
                assert w <= h, f"{kernel}: no row with {axis} in {sorted(w - h)}"
    # the axis values the issue lists are in the enumeration (a census that lost a kernel would pass vacuously)
    m = {c for k, v, c in want if k == "gemv_k256m" and v == 0}
    assert {c[4] for c in m} == {str(n) for n in range(1, 8)} and {c[5] for c in m} == {"0", "1", "2"} and {c[0] for c in m} == set(DTYPES)
    assert {c[3] for c in m} == {"1", "2", "4"} and {c[6] for c in m} == {"0", "1"}
    assert {c[0] for k, v, c in want if k == "gemv_k256m" and v == 4} == {"1", "2", "3+"}
    assert {c[0] for k, v, c in want if k == "gemm_k256" and v == 1} == {"1", "2", "2+1", "4", "4+1", "4+2", "4+2+1"}
    assert {c[1] for k, v, c in want if k == "gemv_k256" and v == 0} == {"1", "2"}


def test_chain_tables_reach_every_instance_of_the_chain_kernel(untuned):
    """gemv_k256c<DT, DEP, MODE>: every (dtype, dependent, mode) the chain call takes the persistent launch for is a case of the
    chain tests; their lists mix 1 ... 7 sweeps, and the independent one layers with and without a permutation, in one launch"""
    want = set()
    for dt in DTYPES:
        descs = [fake_desc(I, O, dt, bool(p)) for I, O, p in k256.K256_CHAIN_SHAPES]
        plain = [fake_desc(I, O, dt) for I, O, p in k256.K256_CHAIN_SHAPES]
        for dep in (0, B.GEMV_CHAIN_DEPENDENT):
            for mode in (0, EXACT, SEL):
                name, f = parse(k256.instance_of(plain if dep else descs, 1, MFMA | dep | mode, "chain").split(": ")[-1].split(" | ")[0])
                if name == "gemv_k256c":
                    want.add((f["dt"], f["dep"], f["mode"]))
                    if not dep:
                        assert f"sweeps={f['sweeps']} perm={f['perm']}" == k256.K256_CHAIN_SWEEPS
    # (the cases the chain tests are parametrised over: their own constants)
    have = {(dt, "0", a) for dt in k256.K256_CHAIN_DTYPES for a in k256.K256_CHAIN_INDEPENDENT}
    have |= {(dt, "1", a) for dt in k256.K256_CHAIN_DTYPES for a in k256.K256_CHAIN_DEPENDENT}
    assert want == have, (sorted(want - have), sorted(have - want))
    sweeps, perms = (set(s.split("=")[1].split(",")) for s in k256.K256_CHAIN_SWEEPS.split())
    assert sweeps == {str(n) for n in range(1, 8)} and perms == {"0", "1"}
    assert set(k256.K256_CHAIN_DEP_SWEEPS.split()[0].split("=")[1].split(",")) >= {"1", "3", "4", "5", "7"}


def test_table_instances_are_what_the_library_answers(untuned):
    """every row's instance string is the library's answer for a descriptor of the row's shape (the GPU tests assert the same on
    the real layer): a routing change shows here first, without a GPU"""
    # 257 row groups of 4 vector-rows: two per workgroup on 256 CUs and on no other count
    probe = parse(k256.instance_of([fake_desc(256, 32 * 257)], 1, MFMA))[1]
    assert probe["units"] == "2" and parse(k256.instance_of([fake_desc(256, 32 * 256)], 1, MFMA))[1]["units"] == "1", \
        "the tables are written for a 256-CU device (MI355X); this one has another CU count"
    for p in rm.ONE_LAYER + k256.K256_ONE_LAYER:
        e = p.values[0]
        if "instance" not in e:
            continue
        I, O, kw = e["layer"]
        d = fake_desc(I, O, e["dt"], bool(kw.get("enable_perm")))
        assert k256.instance_of([d], e["tokens"], e["flags"]) == e["instance"], p.id
        assert B.lib().vptq_quant_gemv_kernel_name(d, e["tokens"], e["flags"]).decode() == e["route"], p.id
    for shapes, dt, tokens, flags, route, instance, twin in k256.K256_GROUPS:
        ds = [fake_desc(I, O, dt, bool(p)) for I, O, p in shapes]
        assert k256.instance_of(ds, tokens, flags, "grouped") == instance


def test_instance_queries_validate_and_need_no_device():
    lib = B.lib()
    d = fake_desc(4096, 4096)
    buf = C.create_string_buffer(256)
    assert lib.vptq_quant_gemv_instance(d, 1, 0, buf, 256) == 0 and buf.value.startswith(b"gemv_k256 dt=f16 rows=1 tok=1 sw=1 perm=0 fast=1")
    assert lib.vptq_quant_gemv_instance(d, 1, 0, buf, 8) == B.E_WORKSPACE          # too small a buffer
    assert lib.vptq_quant_gemv_instance(d, 1, 0, None, 256) == B.E_NULL
    assert lib.vptq_quant_gemv_instance(d, 0, 0, buf, 256) == B.E_TOKENS
    two = (B.LayerDesc * 2)(d, fake_desc(4096, 4096, "bf16"))
    assert lib.vptq_quant_gemv_grouped_instance(two, 2, 1, 0, buf, 256) == B.E_UNSUPPORTED   # one dtype per group
    assert lib.vptq_quant_gemv_grouped_instance(two, 0, 1, 0, buf, 256) == B.E_SHAPE
    assert lib.vptq_quant_gemv_chain_instance(two, 0, 1, 0, buf, 256) == B.E_SHAPE
    # the kernel-name queries and the instance queries agree on the kernel
    for flags, tokens in ((0, 1), (EXACT, 1), (EXACT, 2), (0, 5), (EXACT, 16), (MFMA | SEL, 1)):
        big = fake_desc(8192, 8192)
        name = lib.vptq_quant_gemv_kernel_name(big, tokens, flags).decode()
        assert lib.vptq_quant_gemv_instance(big, tokens, flags, buf, 256) == 0
        assert name.split("_kernel")[0] == buf.value.decode().split()[0], (name, buf.value)
    # a chain the call hands to the grouped / per-layer routes says so
    four = (B.LayerDesc * 4)(*[fake_desc(8192, 8192)] * 4)
    big_buf = C.create_string_buffer(4096)
    assert lib.vptq_quant_gemv_chain_instance(four, 4, 1, 0, big_buf, 4096) == 0 and big_buf.value.startswith(b"grouped: gemv_k256m ")
    assert lib.vptq_quant_gemv_chain_instance(four, 1, 1, 0, big_buf, 4096) == 0 and big_buf.value.startswith(b"per-layer: gemv_k256m ")


# ---------------------------------------------------------------------------------------------- the sliced family
# gemv_sliced_kernel, gemv_sliced_tok_kernel and gemv_hot_kernel: enumerated through vptq_quant_gemv_sliced_instance / _tokens_instance
# over fake descriptors and fake layout structs filled from vptq_sliced_layout_set (scalar fields and aligned, never dereferenced
# pointers), held to the rows of tests/test_route_models_sliced_gpu.py and the sliced tables of test_route_models_gpu.py.
def fake_sliced_desc(I, O, dt="f16", v=8, k=65536, kr=0, perm=False):
    d = B.LayerDesc()
    ib, rb = k.bit_length() - 1, (kr.bit_length() - 1 if kr else 0)
    d.in_features, d.out_features, d.vector_len, d.num_codebooks, d.group_size = I, O, v, 1, I
    d.num_centroids, d.num_res_centroids, d.index_bits, d.res_bits = k, kr, ib, rb
    d.row_words, d.num_indices, d.dtype = (I * (ib + rb) + 31) // 32, (O + v - 1) // v, DTYPES[dt]
    d.indices, d.centroids, d.res_centroids = 1 << 20, 2 << 20, (3 << 20 if kr else None)
    d.weight_scale, d.weight_bias = 4 << 20, 5 << 20
    if perm:
        d.perm, d.scale_permuted, d.bias_permuted = 6 << 20, 7 << 20, 8 << 20
    return d


def fake_call(I, Os, dt, v, k, kr, perm, mode, rpw=0):
    """-> (descs, layouts, n, extra flags, entry kind) of the call a row (or a grid point) makes, as SlicedGemv / SlicedGroupGemv
    would build it: the layout set, the column parts and the rows-per-wave rule of vptq_amd/utils/sliced.py; None: not served"""
    from vptq_amd.utils.sliced import layout_set, part_desc, rows_per_wave_for
    exact = mode == "exact"
    descs = [fake_sliced_desc(I, O, dt, v, k, kr, perm) for O in Os]
    if mode == "sel" and not B.lib().vptq_quant_gemv_sliced_selective_supported(descs[0]):
        return None
    ls = layout_set(descs[0], exact)
    parts, tables = int(ls.parts), int(ls.tables)
    if not parts or (parts > 1 and len(Os) > 1):
        return None
    if parts > 1:
        w = I // parts
        descs = [part_desc(descs[0], p * w, (p + 1) * w) for p in range(parts)]
    # (SlicedGemv counts a layer's column parts as tables here; SlicedGroupGemv sums its members' rows)
    rpw = rpw or rows_per_wave_for(sum(int(d.num_indices) for d in descs) if parts == 1 else int(descs[0].num_indices),
                                   int(ls.n_slices) * tables * parts)
    lay = [B.SlicedLayout(16 << 20, 17 << 20, 18 << 20, (19 << 20) if (t == 0 and ls.side_bytes) else None, rpw, 1, int(ls.n_slices),
                          int(ls.whole_table[t]), 20 << 20) for _ in descs for t in range(tables)]
    return (B.LayerDesc * len(descs))(*descs), (B.SlicedLayout * len(lay))(*lay), len(descs), (sliced.PARTS if parts > 1 else 0), parts


def sliced_query(I, Os, dt, tokens, mode, v=8, k=65536, kr=0, perm=False, rpw=0):
    """the instance string of that call, or None where the library turns it down (not served)"""
    c = fake_call(I, Os, dt, v, k, kr, perm, mode, rpw)
    if c is None:
        return None
    descs, lay, n, extra, parts = c
    buf = C.create_string_buffer(1024)
    fn = B.lib().vptq_quant_gemv_sliced_instance if tokens == 1 else B.lib().vptq_quant_gemv_sliced_tokens_instance
    rc = fn(descs, lay, n, tokens, sliced.MODE_FLAGS[mode] | extra, buf, len(buf))
    assert rc in (0, B.E_UNSUPPORTED) or (rc == B.E_TOKENS and tokens > 8), (rc, B.lib().vptq_last_error())
    return buf.value.decode() if rc == 0 else None


def entry_of(Os, entry, instance):
    """the entry point as the census counts it"""
    if " parts=2" in instance or " parts=3" in instance:
        return "parts"
    return "grouped" if len(Os) > 1 or entry == "grouped" else "single"


def sliced_bucket(name, f, tokens, entry, k, kr):
    """the axes as the census counts them: the tokens asked for, the entry point, the main table's size and the residual table's
    (neither is in the instance string: the per-slice table bytes and the width of the residual index change with them), and the
    one-token layouts' rows per wave as 1 / 2 - 16 / 17+"""
    f = dict(f, tokens=str(tokens), entry=entry, k=str(k), kr=str(kr))
    if name == "gemv_sliced":
        r = int(f["rpw"])
        f["rpw"] = "1" if r == 1 else "2-16" if r <= 16 else "17+"   # (past 16 the lanes holding the rows' words come round again)
    return f


VIEWS.update({
    "gemv_sliced": [("dt", "nsl", "res", "v", "two", "ex", "rg", "tok", "wpt"),      # every instantiation
                    ("wparts", "tok"), ("parts", "tok", "perm", "dt"), ("whole1", "two"), ("side", "nsl"), ("perm", "ex", "tok"),
                    ("entry", "ex", "tok"), ("n", "ex", "dt"), ("rpw", "ex", "dt"), ("corr", "two", "dt", "v"),
                    ("k", "ex", "dt"), ("kr", "ex", "dt", "v"), ("perm", "ex", "dt")],
    "gemv_sliced_tok": [("dt", "nsl", "res", "v", "two", "tok", "ex"),              # every instantiation
                        ("phases", "ex", "tok"), ("regsums", "tok", "dt"), ("whole1", "two"), ("perm", "ex", "dt"), ("n", "ex", "dt"),
                        ("tok", "tokens"), ("entry", "ex", "tok"), ("k", "ex", "dt"), ("kr", "ex", "dt")],
    "gemv_hot": [("dt", "v")],
})
SLICED_KERNELS = ("gemv_sliced", "gemv_sliced_tok", "gemv_hot")
# full template tuples per dtype the enumeration must contain, as counted from the launchers
SLICED_INSTANTIATIONS = {"gemv_sliced": 42, "gemv_sliced_tok": 42, "gemv_hot": 2}


def sliced_cells_of(instance, tokens, entry, k=65536, kr=0):
    out = set()
    for one in instance.split(" | "):
        name, f = parse(one)
        f = sliced_bucket(name, f, tokens, entry, k, kr) if name != "gemv_hot" else f
        for vi, view in enumerate(VIEWS[name]):
            out.add((name, vi, tuple(f[k] for k in view)))
    return out


# widths on both sides of every edge: slice count of the exact layouts (5376 / 4704, 16288 / 15616), of the folded ones (14336 /
# 14080), window parts (4096, 14336), column parts (16392 = 3 x 5464, 28672 = 2 x 14336), column phases
SLICED_WIDTHS = [1000, 1024, 4096, 4104, 4704, 4712, 5376, 5384, 8192, 14080, 14088, 14336, 14344, 15616, 15624, 16288, 16296, 16392, 28672]
SLICED_HEIGHTS = [72, 264, 8200]
KR_CLASSES = [0, 256, 4, 1024, 4096, 65536]


def enumerate_sliced_cells():
    """every cell the sliced dispatch produces over the grid of requests (a form no public shape reaches is not listed)"""
    cells = set()
    for dt in DTYPES:
        for v in (8, 16):
            for k, krs in ((65536, KR_CLASSES), (32768, (0, 256)), (16384, (0, 256))):
                for kr in krs:
                    for I in SLICED_WIDTHS:
                        for perm in (False, True):
                            for mode in ("folded", "exact", "sel"):
                                for Os in ([(O,) for O in SLICED_HEIGHTS] + [(264, 72), (264, 72, 8200)]):
                                    if perm and (Os[0] == 8200 or len(Os) == 2):
                                        continue
                                    for tokens in range(1, 10):   # (9: the entries take 2 - 8, the query turns it down - nothing to list)
                                        if tokens > 1 and mode == "sel":
                                            continue
                                        inst = sliced_query(I, Os, dt, tokens, mode, v, k, kr, perm)
                                        if inst:
                                            cells |= sliced_cells_of(inst, tokens, entry_of(Os, "single", inst), k, kr)
                                            if len(Os) == 1 and mode != "sel" and entry_of(Os, "single", inst) == "single":
                                                cells |= sliced_cells_of(inst, tokens, "grouped", k, kr)   # (a group of one launches the same)
            # rows per wave of the one-token layouts beyond the objects' rule: 2 - 16 and past 16
            for rpw in (2, 18):
                for mode in ("folded", "exact"):
                    inst = sliced_query(1024, (264,), dt, 1, mode, v, rpw=rpw)
                    cells |= sliced_cells_of(inst, 1, "single")
    return cells


def sliced_table_cells():
    cells = set()
    for p in sliced.ROWS:
        e = p.values[0]
        ents = ("single", "grouped") if e["entry"] == "both" else (entry_of(e["Os"], e["entry"], e["instance"]),)
        for ent in ents:
            cells |= sliced_cells_of(e["instance"], e["tokens"], ent, e["k"], e["kr"])
    for I, O, kw, dt, exact, slices, parts, inst in rm.SLICED:
        cells |= sliced_cells_of(inst, 1, entry_of((O,), "single", inst), 65536, kw.get("num_res_centroids", 0))
    for I, O, kw, dt, exact, tokens, one_pass, wparts, inst in rm.SLICED_TOKENS:
        cells |= sliced_cells_of(inst, tokens, entry_of((O,), "single", inst))
    return cells


# (kernel, view, cell, reason): enumerated cells of the sliced family the tables leave out
SLICED_NOT_COVERED = [
]


def test_sliced_tables_reach_every_instance_the_dispatch_produces(untuned):
    want, have = enumerate_sliced_cells(), sliced_table_cells()
    named = {(k, v, c) for k, v, c, _ in SLICED_NOT_COVERED}
    assert all(reason for _, _, _, reason in SLICED_NOT_COVERED)
    assert named <= want, f"SLICED_NOT_COVERED names cells the dispatch does not produce: {sorted(named - want)}"
    assert not (named & have), f"SLICED_NOT_COVERED names covered cells: {sorted(named & have)}"
    missing = want - have - named
    assert not missing, f"{len(missing)} of {len(want)} instance cells without a row, e.g. {sorted(missing)[:12]}"
    assert len(named) * 10 <= len(want), f"SLICED_NOT_COVERED holds {len(named)} of {len(want)} cells: more than 10 %"
    for kernel in SLICED_KERNELS:   # no whole value of any axis is left out
        for vi, view in enumerate(VIEWS[kernel]):
            for pos, axis in enumerate(view):
                w = {c[pos] for k, v, c in want if k == kernel and v == vi}
                h = {c[pos] for k, v, c in have if k == kernel and v == vi}
                assert w <= h, f"{kernel}: no row with {axis} in {sorted(w - h)}"
    # the instantiations counted from the launchers are in the enumeration (a census that lost a kernel would pass vacuously)
    for dt in DTYPES:
        for kernel, count in SLICED_INSTANTIATIONS.items():
            got = {c for k, v, c in want if k == kernel and v == 0 and c[0] == dt}
            assert len(got) == count, f"{kernel} {dt}: {len(got)} instantiations enumerated, {count} expected: {sorted(got)}"


def test_sliced_table_instances_are_what_the_library_answers(untuned):
    """every sliced row's instance string is the library's answer for fake descriptors and layout structs of the row's shape"""
    for p in sliced.ROWS:
        e = p.values[0]
        assert sliced_query(e["I"], e["Os"], e["dt"], e["tokens"], e["mode"], e["v"], e["k"], e["kr"], bool(e["perm"]), e["rpw"]) == e["instance"], p.id
    for I, O, kw, dt, exact, slices, parts, inst in rm.SLICED:
        assert sliced_query(I, (O,), dt, 1, "exact" if exact else "folded", kw.get("vector_len", 8), 65536, kw.get("num_res_centroids", 0),
                            bool(kw.get("enable_perm"))) == inst, (I, O)
    for I, O, kw, dt, exact, tokens, one_pass, wparts, inst in rm.SLICED_TOKENS:
        assert sliced_query(I, (O,), dt, tokens, "exact" if exact else "folded") == inst, (I, O, tokens)


def test_sliced_instance_queries_validate_and_need_no_device():
    lib = B.lib()
    descs, lay, n, _, _ = fake_call(4096, (264,), "f16", 8, 65536, 0, False, "exact")
    buf = C.create_string_buffer(512)
    assert lib.vptq_quant_gemv_sliced_instance(descs, lay, 1, 1, EXACT, buf, 512) == 0 and buf.value.startswith(b"gemv_sliced dt=f16 nsl=8 ")
    assert lib.vptq_quant_gemv_sliced_instance(descs, lay, 1, 1, EXACT, buf, 8) == B.E_WORKSPACE
    assert lib.vptq_quant_gemv_sliced_instance(descs, lay, 1, 1, EXACT, None, 512) == B.E_NULL
    assert lib.vptq_quant_gemv_sliced_instance(descs, None, 1, 1, EXACT, buf, 512) == B.E_NULL
    assert lib.vptq_quant_gemv_sliced_instance(descs, lay, 1, 2, EXACT, buf, 512) == B.E_TOKENS
    assert lib.vptq_quant_gemv_sliced_instance(descs, lay, 0, 1, EXACT, buf, 512) == B.E_SHAPE
    assert lib.vptq_quant_gemv_sliced_instance(descs, lay, 4, 1, EXACT, buf, 512) == B.E_SHAPE
    assert lib.vptq_quant_gemv_sliced_tokens_instance(descs, lay, 1, 1, EXACT, buf, 512) == B.E_TOKENS
    assert lib.vptq_quant_gemv_sliced_tokens_instance(descs, lay, 1, 9, EXACT, buf, 512) == B.E_TOKENS
    assert lib.vptq_quant_gemv_sliced_tokens_instance(descs, lay, 1, 5, EXACT, buf, 8) == B.E_WORKSPACE
    assert lib.vptq_quant_gemv_sliced_tokens_instance(descs, lay, 1, 5, EXACT, buf, 512) == 0 and buf.value.startswith(b"gemv_sliced_tok dt=f16 ")
    # 2 tokens over 4096 columns: the one pass of the one-token kernel, in two window parts
    assert lib.vptq_quant_gemv_sliced_tokens_instance(descs, lay, 1, 2, EXACT, buf, 512) == 0 and b" tok=2 wpt=1 wparts=2 " in buf.value
    # a folded layout is not an exact one (the slice counts differ at this width only beyond 5376 columns: the flags decide the kernel)
    assert lib.vptq_quant_gemv_sliced_instance(descs, lay, 1, 1, 0, buf, 512) == 0 and b" ex=0 " in buf.value
    # the selective call: the pre-pass in front
    assert lib.vptq_quant_gemv_sliced_instance(descs, lay, 1, 1, SEL, buf, 512) == 0
    assert buf.value.startswith(b"gemv_hot dt=f16 v=8 | gemv_sliced ") and buf.value.endswith(b"corr=1")


# ---------------------------------------------------------------------------------------------- the remaining families
# gemv_gather, gemv_gatherx, gemv_generic, gemv_lds / gemv_lds_mfma (packed layers, vptq_quant_gemv_instance) and the v2 entry
# (gemv_lds* with fmt=v2*, gemv_v2: vptq_quant_gemv_v2_instance), over fake descriptors built from a row's own fields - the grid
# points are rows without an instance string - and held to the rows of tests/test_route_models_other_gpu.py.
import test_route_models_other_gpu as other  # noqa: E402
from test_route_models_gpu import GENERIC  # noqa: E402


def _bits(n):
    return (n - 1).bit_length() if n > 0 else 0


def fake_other_desc(e):
    """the descriptor spec_to_module + module_desc give for the layer of a packed row, with fake (aligned, never dereferenced)
    pointers"""
    d = B.LayerDesc()
    I, O, v, C_, S = e["I"], e["O"], e["v"], e["C"], e["S"]
    G = (I - S) // C_
    ib, rb = _bits(e["k"]), _bits(e["kr"])
    d.in_features, d.out_features, d.vector_len, d.num_codebooks, d.group_size = I, O, v, C_, G
    d.num_centroids, d.num_res_centroids, d.index_bits, d.res_bits = e["k"], e["kr"], ib, rb
    d.row_words, d.num_indices, d.dtype = (G * (ib + rb) + 31) // 32, (O + v - 1) // v, DTYPES[e["dt"]]
    d.indices, d.centroids, d.res_centroids = 1 << 20, 2 << 20, (3 << 20 if e["kr"] else None)
    if S:
        d.outlier_size, d.outlier_vector_len, d.num_outlier_centroids = S, e["ov"], 256
        d.num_outlier_indices = (O + e["ov"] - 1) // e["ov"]
        d.outlier_indices, d.outlier_centroids = 9 << 20, 10 << 20
    if e["norm"]:
        d.weight_scale, d.weight_bias = 4 << 20, 5 << 20
    if e["perm"]:
        d.perm = 6 << 20
        if e["norm"]:
            d.scale_permuted, d.bias_permuted = 7 << 20, 8 << 20
    if e["bias"]:
        d.bias = 11 << 20
    return d


def fake_v2_desc(e):
    d = B.V2Desc()
    d.in_features, d.out_features, d.vector_len, d.num_centroids = e["I"], e["O"], e["v"], e["k"]
    d.num_res_centroids, d.res_index_bytes, d.dtype = e["kr"], e["rb"], DTYPES[e["dt"]]
    d.indices, d.centroids = 1 << 20, 2 << 20
    if e["kr"]:
        d.res_indices, d.res_centroids = 3 << 20, 4 << 20
    if e["norm"]:
        d.scale_weights, d.scale_bias = 5 << 20, 6 << 20
    if e["bias"]:
        d.bias = 7 << 20
    return d


def other_query(e):
    """the instance string of the call a row (or a grid point) makes, or None where the library turns it down"""
    buf = C.create_string_buffer(512)
    if e["entry"] == "v2":
        rc = B.lib().vptq_quant_gemv_v2_instance(fake_v2_desc(e), e["tokens"], e["flags"], buf, len(buf))
    else:
        rc = B.lib().vptq_quant_gemv_instance(fake_other_desc(e), e["tokens"], e["flags"], buf, len(buf))
    return buf.value.decode() if rc == 0 else None


OTHER_VIEWS = {
    "gemv_gather": [("dt", "t", "rows", "tok", "perm", "wide"), ("tok", "tokens")],                 # every instantiation
    "gemv_gatherx": [("dt", "v", "tok", "perm"), ("reslds", "v"), ("outl", "v"), ("groups",), ("tok", "tokens")],
    "gemv_generic": [("dt", "v", "tok"), ("tok", "tokens")],
    "gemv_lds": [("dt", "fmt", "tok"), ("rw", "tok"), ("dma", "fmt"), ("perm", "dt"), ("tok", "tokens")],
    "gemv_lds_mfma": [("dt", "fmt"), ("rw",), ("dma", "fmt"), ("stages", "dt"), ("perm", "dt")],
    "gemv_v2": [("dt", "v", "tok"), ("tok", "tokens")],
}
VIEWS.update(OTHER_VIEWS)
# full template tuples (view 0) the enumeration must contain, as counted from the launch code
OTHER_INSTANTIATIONS = {"gemv_gather": 68, "gemv_gatherx": 100, "gemv_generic": 56, "gemv_lds": 40, "gemv_lds_mfma": 16, "gemv_v2": 24}


def other_cells_of(instance, tokens):
    name, f = parse(instance)
    if name not in OTHER_VIEWS:
        return set()
    f = dict(f, tokens=str(tokens) if tokens < 10 else "10+")   # (tokens past every family's slots twice over: one class)
    return {(name, vi, tuple(f[k] for k in view)) for vi, view in enumerate(OTHER_VIEWS[name])}


def _P(I, O, dt, tokens, **kw):
    return other.R(I, O, dt, tokens, "?", **kw).values[0]


def _Q(I, O, dt, tokens, **kw):
    return other.V(I, O, dt, tokens, "?", **kw).values[0]


# residual tables on both sides of the 32 KiB an LDS copy takes, per vector length (2 kr v bytes; not a multiple of 16: L2 as well)
X_FORMATS = [(256, 0), (256, 16), (32768, 0), (65536, 2), (4096, 256), (32768, 256), (65536, 1024), (512, 2048), (32768, 4096),
             (32768, 65536), (65536, 65536), (256, 16384), (1024, 2)]
LDS_FORMATS = [(4096, 0), (1024, 4), (8192, 0), (4096, 256), (2048, 512), (4096, 512), (8192, 256), (8192, 512)]
LDS_SHAPES = [(264, 60), (520, 60), (1032, 136), (264, 4804), (264, 8806), (264, 16804), (264, 32804)]


def other_grid():
    """the requests the census makes: row specs without an instance string (dtype x format x tokens 1 - 16 x perm x widths x
    heights; the shapes that cannot be small only where they decide an axis)"""
    for dt in DTYPES:
        for tokens in range(1, 17):
            for perm in (0, 1):
                # k = 65536, v = 8: cache gathers; 2049 vector-rows (ROWS = 2) and 6152 columns (WIDE) at one token
                for kr in (0, 256, 65536):
                    for I, O in ((264, 72), (520, 100), (6136, 72), (6152, 72)) + (((264, 16392), (6152, 16392)) if tokens == 1 else ()):
                        if I * O < (1 << 24) or kr == 256:
                            yield _P(I, O, dt, tokens, k=65536, kr=kr, perm=perm, big=int(I * O > (1 << 24)))
                # LDS-resident tables: every row-group height on 256 CUs
                for k, kr in LDS_FORMATS:
                    for I, O in LDS_SHAPES:
                        for flags in (0, EXACT):
                            yield _P(I, O, dt, tokens, k=k, kr=kr, perm=perm, flags=flags)
                # L2 gathers of every other format; the generic kernel by flag
                for v in (2, 4, 6, 8, 10, 12, 16):
                    for k, kr in X_FORMATS:
                        for I, O in ((260, 72), (520, 100), (1028, 72)):
                            yield _P(I, O, dt, tokens, v=v, k=k, kr=kr, perm=perm)
                    for C_ in (2, 4):
                        yield _P(260 * C_, 100, dt, tokens, v=v, k=4096, kr=16, C=C_, perm=perm)
                    for ov in ((v, 4) if v in (8, 12, 16) else (v,)):
                        yield _P(520 + 8, 100 - 2, dt, tokens, v=v, k=32768, kr=16, S=8, ov=ov, perm=perm)
                    for k, kr in ((256, 256), (4096, 4096)):
                        yield _P(264, 100, dt, tokens, v=v, k=k, kr=kr, perm=perm, flags=GENERIC)
            # the staging passes of the MFMA variant: 1024 vector-rows of more than 8192 / 24576 columns
            if tokens == 1:
                for I in (8200, 24584):
                    yield _P(I, 8192, dt, 1, k=4096, kr=0, big=1)
            # the v2 entry: LDS-resident up to k = 8192 at v = 8 (k not a multiple of 64: the main table through registers), else gemv_v2
            if tokens < 16:
                for v in (4, 8, 16):
                    for k in (8192, 5000, 16384):
                        for kr, rb in ((0, 0), (256, 1), (256, 2), (512, 2)):
                            for I, O in ((264, 64), (520, 4800), (264, 8816)):
                                for flags in (0, GENERIC):
                                    if O > 64 and (v != 8 or flags or k > 8192):
                                        continue   # (the heights matter to the LDS kernels' row groups only)
                                    yield _Q(I, O, dt, tokens, v=v, k=k, kr=kr, rb=rb, flags=flags)


def enumerate_other_cells():
    cells = set()
    for e in other_grid():
        inst = other_query(e)
        if inst:
            cells |= other_cells_of(inst, e["tokens"])
    return cells


def other_table_cells():
    cells = set()
    for p in other.ALL_ROWS:
        e = p.values[0]
        cells |= other_cells_of(e["instance"], e["tokens"])
    return cells


# (kernel, view, cell, reason): enumerated cells of these families the tables leave out
OTHER_NOT_COVERED = [
]


def test_other_tables_reach_every_instance_the_dispatch_produces(untuned):
    want, have = enumerate_other_cells(), other_table_cells()
    named = {(k, v, c) for k, v, c, _ in OTHER_NOT_COVERED}
    assert all(reason for _, _, _, reason in OTHER_NOT_COVERED)
    assert named <= want, f"OTHER_NOT_COVERED names cells the dispatch does not produce: {sorted(named - want)}"
    assert not (named & have), f"OTHER_NOT_COVERED names covered cells: {sorted(named & have)}"
    missing = want - have - named
    assert not missing, f"{len(missing)} of {len(want)} instance cells without a row, e.g. {sorted(missing)[:12]}"
    assert len(named) * 10 <= len(want), f"OTHER_NOT_COVERED holds {len(named)} of {len(want)} cells: more than 10 %"
    for kernel, views in OTHER_VIEWS.items():   # no whole value of any axis is left out
        for vi, view in enumerate(views):
            for pos, axis in enumerate(view):
                w = {c[pos] for k, v, c in want if k == kernel and v == vi}
                h = {c[pos] for k, v, c in have if k == kernel and v == vi}
                assert w <= h, f"{kernel}: no row with {axis} in {sorted(w - h)}"
    # the instantiations counted from the launch code are in the enumeration (a census that lost a kernel would pass vacuously)
    for kernel, count in OTHER_INSTANTIATIONS.items():
        got = {c for k, v, c in want if k == kernel and v == 0}
        assert len(got) == count, f"{kernel}: {len(got)} instantiations enumerated, {count} expected: {sorted(got)}"
    assert {c[0] for k, v, c in want if k == "gemv_lds" and v == 1} == {"1", "2", "4", "8", "16"}
    assert {c[0] for k, v, c in want if k == "gemv_lds_mfma" and v == 1} == {"4", "8", "16"}
    assert {c[0] for k, v, c in want if k == "gemv_lds_mfma" and v == 3} == {"1", "2", "4"}
    assert {c[0] for k, v, c in want if k == "gemv_lds" and v == 2} == {"0", "1"}
    assert {c[0] for k, v, c in want if k == "gemv_gatherx" and v == 2} == {"0", "same", "4"}
    assert {c[0] for k, v, c in want if k == "gemv_gatherx" and v == 3} == {"1", "2", "4"}


def test_other_table_instances_are_what_the_library_answers(untuned):
    """every row's instance string is the library's answer for a fake descriptor of the row's shape (the GPU test asserts the same
    on the real layer), and the kernel-name query agrees on the kernel"""
    # 1101 vector-rows: row groups of 4 on 256 CUs (276 groups), of 2 or 8 on parts with more or fewer
    probe = parse(other_query(_P(264, 8806, "f16", 2, k=4096)))[1]
    assert probe["rw"] == "4", "the tables are written for a 256-CU device (MI355X); this one has another CU count"
    for p in other.ALL_ROWS:
        e = p.values[0]
        assert other_query(e) == e["instance"], p.id
        if e["entry"] == "packed":
            name = B.lib().vptq_quant_gemv_kernel_name(fake_other_desc(e), e["tokens"], e["flags"]).decode()
            assert name == e["instance"].split()[0] + "_kernel", p.id


def test_other_instance_queries_validate_and_need_no_device():
    lib = B.lib()
    buf = C.create_string_buffer(256)
    d = fake_v2_desc(_Q(264, 64, "f16", 1, k=8192, kr=256))
    assert lib.vptq_quant_gemv_v2_instance(d, 1, 0, buf, 256) == 0 and buf.value.startswith(b"gemv_lds dt=f16 fmt=v2u8 tok=1 rw=1 ")
    assert lib.vptq_quant_gemv_v2_instance(d, 1, GENERIC, buf, 256) == 0 and buf.value == b"gemv_v2 dt=f16 v=8 tok=1"
    assert lib.vptq_quant_gemv_v2_instance(d, 1, 0, buf, 8) == B.E_WORKSPACE
    assert lib.vptq_quant_gemv_v2_instance(d, 1, 0, None, 256) == B.E_NULL
    assert lib.vptq_quant_gemv_v2_instance(None, 1, 0, buf, 256) == B.E_NULL
    assert lib.vptq_quant_gemv_v2_instance(d, 0, 0, buf, 256) == B.E_TOKENS
    assert lib.vptq_quant_gemv_v2_instance(d, 16, 0, buf, 256) == B.E_TOKENS
    d.vector_len = 6
    assert lib.vptq_quant_gemv_v2_instance(d, 1, 0, buf, 256) == B.E_UNSUPPORTED
    # every family's line starts with its kernel's name
    for e in (_P(264, 72, "f16", 3, k=65536, kr=256), _P(264, 72, "bf16", 2, k=4096, kr=256), _P(260, 72, "f16", 1, v=6, k=4096),
              _P(264, 72, "f16", 9, k=256, kr=256, flags=GENERIC), _P(264, 8806, "f16", 1, k=4096)):
        fd = fake_other_desc(e)
        name = lib.vptq_quant_gemv_kernel_name(fd, e["tokens"], e["flags"]).decode()
        assert lib.vptq_quant_gemv_instance(fd, e["tokens"], e["flags"], buf, 256) == 0
        assert name.split("_kernel")[0] == buf.value.decode().split()[0], (name, buf.value)


# ---------------------------------------------------------------------------------------------- vptq_dequant
# dequant_kernel<DT, V, TAB>: enumerated through vptq_dequant_instance over fake descriptors built from a row's own fields - the grid
# points are rows without an instance string - and held to the rows of tests/test_dequant_models_gpu.py.  The line carries the launch
# decision and, per path to a thread's 8 index elements, the chunks of one vector-row that take it (dequant_paths.h: the kernel's
# own predicates).
import test_dequant_models_gpu as dq  # noqa: E402

DQ_LDS_MAX = 16384   # dequant_paths.h:kDqLdsMax - only to name the side of the limit a request's tables lie on


def fake_dequant_desc(e):
    """-> (descriptor, W): what module_desc gives for the layer of a dequant row, with fake (never dereferenced) pointers at the
    row's alignments"""
    d = B.LayerDesc()
    I, O, v, C_, S = e["I"], e["O"], e["v"], e["C"], e["S"]
    G = (I - S) // C_
    ib, rb = _bits(e["k"]), _bits(e["kr"])
    d.in_features, d.out_features, d.vector_len, d.num_codebooks, d.group_size = I, O, v, C_, G
    d.num_centroids, d.num_res_centroids, d.index_bits, d.res_bits = e["k"], e["kr"], ib, rb
    d.row_words, d.num_indices, d.dtype = (G * (ib + rb) + 31) // 32, (O + v - 1) // v, DTYPES[e["dt"]]
    d.indices, d.centroids, d.res_centroids = (1 << 20) + e["idx_off"], 2 << 20, (3 << 20 if e["kr"] else None)
    if S:
        d.outlier_size, d.outlier_vector_len, d.num_outlier_centroids = S, e["ov"], 256
        d.num_outlier_indices = (O + e["ov"] - 1) // e["ov"]
        d.outlier_indices, d.outlier_centroids = 9 << 20, 10 << 20
    if e["norm"]:
        d.weight_scale, d.weight_bias = (4 << 20) + e["norm_off"], (5 << 20) + e["norm_off"]
    if e["perm"]:
        d.perm, d.inv_perm = 6 << 20, 7 << 20
    return d, (16 << 20) + e["w_off"]


def dequant_query(e):
    d, W = fake_dequant_desc(e)
    buf = C.create_string_buffer(512)
    rc = B.lib().vptq_dequant_instance(d, W, buf, len(buf))
    assert rc == 0, (rc, B.lib().vptq_last_error(), e)
    return buf.value.decode()


DEQUANT_VIEWS = [("dt", "v", "tab"),               # every instantiation
                 ("t", "idxclasses"),              # the set of paths with a chunk, per index width
                 ("norm", "store", "dt"), ("colblocks",), ("ragged", "dt"), ("perm", "outl", "groups"), ("lds_edge",)]
DEQUANT_INSTANTIATIONS = 42   # 2 dtypes x 7 vector lengths x TAB 0 / 1 / 2 (dequant.hip: launch_dt, launch_v)


def _side(nbytes):
    return "none" if nbytes == 0 else "below" if nbytes < DQ_LDS_MAX else "at" if nbytes == DQ_LDS_MAX else "above"


def dequant_cells_of(instance, e):
    name, f = parse(instance)
    assert name == "dequant"
    f["idxclasses"] = "+".join(c.split(":")[0] for c in f["idx"].split(","))
    f["colblocks"] = "1" if f["colblocks"] == "1" else "2+"
    # which side of the LDS limit both tables together, and the residual table alone, lie on (of the REQUEST: the line says what came of it)
    f["lds_edge"] = f"tab={f['tab']} both={_side((e['k'] + e['kr']) * e['v'] * 2)} res={_side(e['kr'] * e['v'] * 2)} groups={'1' if e['C'] == 1 else 'n'}"
    return {("dequant", vi, tuple(f[k] for k in view)) for vi, view in enumerate(DEQUANT_VIEWS)}


def _DQ(I, O, dt, **kw):
    return dq.D(I, O, dt, "?", **kw).values[0]


DQ_VECTOR_LENS = (2, 4, 6, 8, 10, 12, 16)
# (k, kr): TAB 1 / 2 / 0 of every vector length, then both sides of the limit - 16384 bytes are (k + kr) v 2 = 512 entries at v = 16
# and 1024 at v = 8
DQ_FORMATS = [(256, 256), (65536, 256), (65536, 0), (512, 256), (65536, 512), (65536, 1024), (256, 0)]
DQ_WIDTHS = [264, 8, 2040, 2048, 2056, 1001, 7]
# (perm, S, ov, C, I): a permutation, outlier columns of length 4 and of the layer's, 2 / 4 groups of 136 (whole chunks) and of 132
# columns, all of them together
DQ_ELEMENT_CAUSES = [(1, 0, 0, 1, 264), (0, 12, 4, 1, 280), (0, 8, 8, 1, 272), (0, 0, 0, 2, 272), (0, 0, 0, 4, 544), (0, 0, 0, 2, 264),
                     (0, 0, 0, 4, 528), (1, 8, 4, 2, 272)]
DQ_ALIGNMENTS = [dict(), dict(w_off=2), dict(norm_off=2), dict(idx_off=4), dict(norm=0)]


def split_bits(T):
    """(k, kr) of an index width: the main table up to 16 bits, the residual one making up the rest"""
    return 1 << min(T, 16), (1 << (T - 16)) if T > 16 else 0


def dequant_grid():
    """the requests the census makes: dtype x vector length x format, every index width 1 ... 32 x width, the causes of the
    element path and the alignment variants at 16 and 24 bits"""
    for dt in DTYPES:
        for v in DQ_VECTOR_LENS:
            for k, kr in DQ_FORMATS:
                yield _DQ(264, 5 * v - 3, dt, v=v, k=k, kr=kr)
            yield _DQ(272, 5 * v - 3, dt, v=v, k=256, kr=256, C=2)   # two groups whose tables would fit
        for T in range(1, 33):
            k, kr = split_bits(T)
            for I in DQ_WIDTHS:
                if dt == "f16" or I in (264, 2056, 1001):
                    yield _DQ(I, 37, dt, k=k, kr=kr)
            yield _DQ(264, 77, dt, v=16, k=k, kr=kr)
        for k, kr in ((256, 16384), (512, 2048)):   # res_bits > index_bits
            yield _DQ(264, 37, dt, k=k, kr=kr)
        for kr in (0, 256):
            for perm, S, ov, C_, I in DQ_ELEMENT_CAUSES:
                yield _DQ(I, 37, dt, k=65536, kr=kr, perm=perm, S=S, ov=ov, C=C_)
            for kw in DQ_ALIGNMENTS:
                yield _DQ(264, 37, dt, k=65536, kr=kr, **kw)


def enumerate_dequant_cells():
    cells = set()
    for e in dequant_grid():
        cells |= dequant_cells_of(dequant_query(e), e)
    return cells


def dequant_table_cells():
    cells = set()
    for p in dq.ROWS:
        e = p.values[0]
        cells |= dequant_cells_of(e["instance"], e)
    return cells


# (kernel, view, cell, reason): enumerated cells of vptq_dequant the table leaves out
DEQUANT_NOT_COVERED = [
]


def test_dequant_table_reaches_every_instance_the_launcher_produces():
    want, have = enumerate_dequant_cells(), dequant_table_cells()
    named = {(k, v, c) for k, v, c, _ in DEQUANT_NOT_COVERED}
    assert all(reason for _, _, _, reason in DEQUANT_NOT_COVERED)
    assert named <= want, f"DEQUANT_NOT_COVERED names cells the launcher does not produce: {sorted(named - want)}"
    assert not (named & have), f"DEQUANT_NOT_COVERED names covered cells: {sorted(named & have)}"
    missing = want - have - named
    assert not missing, f"{len(missing)} of {len(want)} instance cells without a row, e.g. {sorted(missing)[:12]}"
    assert len(named) * 10 <= len(want), f"DEQUANT_NOT_COVERED holds {len(named)} of {len(want)} cells: more than 10 %"
    for vi, view in enumerate(DEQUANT_VIEWS):   # no whole value of any axis is left out
        for pos, axis in enumerate(view):
            w = {c[pos] for k, v, c in want if v == vi}
            h = {c[pos] for k, v, c in have if v == vi}
            assert w <= h, f"dequant: no row with {axis} in {sorted(w - h)}"
    # the instantiations counted from the launcher are in the enumeration (a census that lost one would pass vacuously)
    got = {c for k, v, c in want if v == 0}
    assert len(got) == DEQUANT_INSTANTIATIONS and got == {(dt, str(v), str(tab)) for dt in DTYPES for v in DQ_VECTOR_LENS for tab in (0, 1, 2)}
    # every index width occurs; the fifth-word windows at exactly four of them, the 16-byte piece at exactly one
    paths = {}
    for k, v, c in want:
        if v == 1:
            paths.setdefault(int(c[0]), set()).update(c[1].split("+"))
    assert sorted(paths) == list(range(1, 33))
    assert {t for t, p in paths.items() if "win5" in p} == {27, 29, 30, 31}
    assert {t for t, p in paths.items() if "vec" in p} == {16}
    assert {t for t, p in paths.items() if "win" in p} == set(range(1, 33)) - {16, 27, 29, 30, 31}
    assert all("elem" in p for p in paths.values())
    assert {c[0] for k, v, c in want if v == 3} == {"1", "2+"}
    assert {c[:2] for k, v, c in want if v == 2} == {("vec", "vec"), ("vec", "scalar"), ("scalar", "vec"), ("scalar", "scalar"), ("none", "vec")}
    edges = {c[0] for k, v, c in want if v == 6}
    assert {"tab=1 both=at res=below groups=1", "tab=2 both=above res=at groups=1", "tab=0 both=above res=above groups=1",
            "tab=0 both=below res=below groups=n", "tab=1 both=below res=none groups=1", "tab=0 both=above res=none groups=1"} <= edges


def test_dequant_table_instances_are_what_the_library_answers():
    """every row's instance string is the library's answer for a fake descriptor of the row's shape and alignments (the GPU test
    asserts the same on the real layer): a change of the launcher or of a path predicate shows here first, without a GPU"""
    assert len(dq.ROWS) >= DEQUANT_INSTANTIATIONS
    for p in dq.ROWS:
        e = p.values[0]
        assert dequant_query(e) == e["instance"], p.id


def test_dequant_instance_query_validates_and_needs_no_device():
    lib = B.lib()
    buf = C.create_string_buffer(256)
    d, W = fake_dequant_desc(_DQ(4104, 37, "f16", k=65536, kr=256))
    assert lib.vptq_dequant_instance(d, W, buf, 256) == 0
    assert buf.value == (b"dequant dt=f16 v=8 tab=2 lds=4096 colblocks=3 t=24 norm=vec store=vec idx=win:512,elem:1 perm=0 outl=0 groups=1 "
                         b"ragged=0")
    assert lib.vptq_dequant_instance(d, W, buf, 8) == B.E_WORKSPACE and buf.value == b""
    assert lib.vptq_dequant_instance(d, W, None, 256) == B.E_NULL
    assert lib.vptq_dequant_instance(None, W, buf, 256) == B.E_NULL
    # vptq_dequant's own validation in front: W, the inverse permutation, the layer
    assert lib.vptq_dequant_instance(d, None, buf, 256) == B.E_NULL
    d.perm = 6 << 20
    assert lib.vptq_dequant_instance(d, W, buf, 256) == B.E_NULL and b"inv_perm" in lib.vptq_last_error()
    d.inv_perm = 7 << 20
    assert lib.vptq_dequant_instance(d, W, buf, 256) == 0 and b" idx=elem:513 perm=1 " in buf.value
    d.vector_len = 5
    assert lib.vptq_dequant_instance(d, W, buf, 256) == B.E_UNSUPPORTED
    d.vector_len, d.row_words = 8, 10
    assert lib.vptq_dequant_instance(d, W, buf, 256) == B.E_SHAPE
    d.row_words, d.indices = 4104 * 24 // 32, (1 << 20) + 2
    assert lib.vptq_dequant_instance(d, W, buf, 256) == B.E_ALIGN
