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
part test_table_instances_are_what_the_library_answers says so at its first row (its probe of the CU count)."""
import ctypes as C
import os

import pytest

from vptq_amd import _backend as B
import test_route_models_gpu as rm
import test_route_models_k256_gpu as k256
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
