"""The rule that gives a persistent chain launch its second geometry, "rows per wave" (gemv_k256c_rows_kernel), no device:
vptq_quant_gemv_chain_rows_plan against a written-out restatement over a grid of launches, and every launch the existing
tests name keeps its kernel name and its plan and instance texts.

The rule (gemv_k256c.hip, next to gemv_k256c_fills_device): fp16, VPTQ_GEMV_EXACT, independent layers, 16-bit outputs; a
workgroup-task = 16 consecutive row groups of 8 vector-rows of one layer, ceil(G / 128) steps long, dealt round-robin over all
workgroups, the layers continuing each other's round robin.  Taken when the tasks number at least the workgroups AND the
busiest workgroup walks no more steps than the busiest one of the first geometry's plan (vptq_quant_gemv_chain_plan) would.
The rule is what the plan query answers and what a launch follows; the tuning knob VPTQ_K256C_ROWS overrides it (0: never, 1:
wherever the geometry serves the launch).

The last section holds the schedule table of tests/test_chain_rows_gpu.py (tests/_chain_rows_run.py:TABLE) without a device: the
deal its covers are computed from is the restatement's and the library's, every entry reaches the covers it names, a shortened
chain loses them, and the rule takes the launch that test runs without a knob."""
import ctypes as C

import pytest

import _chain_rows_run as run
import _chain_schedule as cs
from vptq_amd import _backend as B


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------- the restatement
def c_plan(layers, cus):
    """the first geometry's plan of [(vector-rows N, columns G)] -> (visit, grid, first, rpw)"""
    def rpw_of(N, G, visit):
        ng, ns = cdiv(N, 8), cdiv(G, 2048)
        r = cdiv(ng, cus)
        if visit > 0:
            r = max(r, cdiv(visit, ns))
        return max(r, 1)

    def blocks(visit):
        return sum(cdiv(cdiv(N, 8), rpw_of(N, G, visit)) for N, G in layers)
    visit = next((v for v in (32, 16, 8) if blocks(v) >= 2 * cus), 0)
    grid = min(blocks(visit), cus)
    first, rpws, run = [], [], 0
    for N, G in layers:
        r = rpw_of(N, G, visit)
        first.append(run % grid)
        rpws.append(r)
        run += cdiv(cdiv(N, 8), r)
    return visit, grid, first, rpws


def c_longest(layers, cus):
    _, grid, first, rpws = c_plan(layers, cus)
    steps = [0] * grid
    for (N, G), f, r in zip(layers, first, rpws):
        ng, ns = cdiv(N, 8), cdiv(G, 2048)
        for k in range(cdiv(ng, r)):
            steps[(f + k) % grid] += (min((k + 1) * r, ng) - k * r) * ns
    return max(steps)


def r_plan(layers, cus):
    """-> (taken, first, tasks, steps, longest of the rows geometry, longest of the first geometry)"""
    first, tasks, steps, run = [], [], [], 0
    per_wg = [0] * cus
    for N, G in layers:
        nt, ns = cdiv(cdiv(N, 8), 16), cdiv(G, 128)
        first.append(run % cus)
        tasks.append(nt)
        steps.append(ns)
        for k in range(nt):
            per_wg[(run + k) % cus] += ns
        run += nt
    lr, lc = max(per_wg), c_longest(layers, cus)
    return int(run >= cus and lr <= lc), first, tasks, steps, lr, lc


# ---------------------------------------------------------------------------------------------- the library's answer
def lib_rows_plan(descs, flags, workgroups):
    n = len(descs)
    taken, grid = C.c_int(-1), C.c_int(-1)
    first, tasks, steps, longest = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * 2)()
    rc = B.lib().vptq_quant_gemv_chain_rows_plan(descs, n, flags, workgroups, C.byref(taken), C.byref(grid), first, tasks, steps, longest)
    if rc:
        return rc, None
    return 0, (taken.value, grid.value, list(first), list(tasks), list(steps), longest[0], longest[1])


def instance(descs, flags):
    buf = C.create_string_buffer(4096)
    B.check(B.lib().vptq_quant_gemv_chain_instance(descs, len(descs), 1, flags, buf, len(buf)), "vptq_quant_gemv_chain_instance")
    return buf.value.decode()


def name(descs, flags):
    r = B.lib().vptq_quant_gemv_chain_kernel_name(descs, len(descs), 1, flags)
    return None if r is None else r.decode()


HEIGHTS = (64, 72, 1000, 1032, 4096, 8192, 14336, 28672)          # outputs
WIDTHS = (128, 136, 1024, 2056, 4096, 8192, 14336, 28672)
COUNTS = (1, 2, 3, 5, 9, 16, 32)                                  # layers
WORKGROUPS = (1, 4, 64, 256, 304)


def _grid():
    """uniform launches and mixed ones (a tall, a wide and a small layer in turns)"""
    for n in COUNTS:
        for O in HEIGHTS:
            for I in WIDTHS:
                yield [(I, O)] * n
        for k, O in enumerate(HEIGHTS):
            mix = [(WIDTHS[(k + j) % len(WIDTHS)], HEIGHTS[(k + 2 * j) % len(HEIGHTS)]) for j in range(n)]
            yield mix


def test_rule_matches_its_restatement_over_the_grid():
    taken_n = cells = 0
    for shapes in _grid():
        descs = cs.fake_descs([(I, O, {}) for I, O in shapes])
        layers = [(cdiv(O, 8), I) for I, O in shapes]
        for w in WORKGROUPS:
            rc, got = lib_rows_plan(descs, cs.EXACT | cs.MFMA, w)
            assert rc == 0, (shapes, w, rc)
            taken, first, tasks, steps, lr, lc = r_plan(layers, w)
            assert got == (taken, w, first, tasks, steps, lr, lc), (shapes, w, got, (taken, w, first, tasks, steps, lr, lc))
            # the first geometry's query goes on describing the first geometry
            p = cs.plan(descs, cs.EXACT | cs.MFMA, w)
            v, g, f, r = c_plan(layers, w)
            assert (p["visit"], p["grid"], p["first"], p["rpw"]) == (v, g, f, r), (shapes, w)
            taken_n += taken
            cells += 1
    assert cells >= 2000 and 0.05 < taken_n / cells < 0.95, (cells, taken_n)   # (the grid sees both answers often)


def test_the_headline_ring_takes_it_and_narrower_layers_do_not():
    big = cs.fake_descs([(8192, 8192, {})] * 32)
    rc, got = lib_rows_plan(big, cs.EXACT, 256)
    assert rc == 0 and got[0] == 1 and got[3] == [8] * 32 and got[4] == [64] * 32 and got[5:] == (64, 64), got
    assert got[2] == [(8 * i) % 256 for i in range(32)]
    small = cs.fake_descs([(4096, 4096, {})] * 32)
    rc, got = lib_rows_plan(small, cs.EXACT, 256)
    assert rc == 0 and got[0] == 0 and sum(got[3]) == 128, got      # 128 tasks do not fill 256 workgroups
    rc, got = lib_rows_plan(big, cs.EXACT, 304)
    assert rc == 0 and got[0] == 0, got                              # 256 tasks, 304 workgroups
    rc, got = lib_rows_plan(cs.fake_descs([(8192, 8192, {})] * 9), cs.EXACT, 256)
    assert rc == 0 and got[0] == 0, got


def test_what_the_geometry_does_not_serve():
    """bf16, the folded and selective forms, dependent lists, fp32 outputs: VPTQ_E_UNSUPPORTED, and the launch is the first geometry's"""
    f16 = cs.fake_descs([(8192, 8192, {})] * 32)
    bf16 = cs.fake_descs([(8192, 8192, {})] * 32, dtype=1)
    for descs, flags in ((bf16, cs.EXACT), (f16, 0), (f16, cs.SEL), (f16, cs.EXACT | cs.F32), (f16, cs.DEP), (f16, cs.EXACT | cs.DEP)):
        rc, _ = lib_rows_plan(descs, flags, 256)
        assert rc == B.E_UNSUPPORTED, (flags, rc)
    for descs, flags in ((bf16, cs.EXACT), (f16, 0), (f16, cs.SEL), (f16, cs.EXACT | cs.F32), (f16, cs.DEP)):
        assert name(descs, flags) == "gemv_k256c_kernel" and "geom=" not in instance(descs, flags), flags
    n = 3
    one = (C.c_int * n)()
    assert B.lib().vptq_quant_gemv_chain_rows_plan(f16, n, cs.EXACT, 64, None, one, one, one, one, one) == B.E_NULL
    assert B.lib().vptq_quant_gemv_chain_rows_plan(f16, 0, cs.EXACT, 64, one, one, one, one, one, one) == B.E_SHAPE
    assert B.lib().vptq_quant_gemv_chain_rows_plan(f16, n, cs.EXACT, -1, one, one, one, one, one, one) == B.E_SHAPE


_KNOB_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import test_chain_rows_cpu as t
import _chain_schedule as cs
big = cs.fake_descs([(8192, 8192, {{}})] * 32)
small = cs.fake_descs([(4096, 4096, {{}})] * 32)
print(t.name(big, cs.EXACT), "|", t.instance(big, cs.EXACT), "|", t.instance(small, cs.EXACT), "|", t.instance(big, 0), "|",
      t.lib_rows_plan(big, cs.EXACT, 256)[1][0], t.lib_rows_plan(small, cs.EXACT, 256)[1][0])
"""


def _with_knob(value):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("VPTQ_") or k == "VPTQ_HIP_LIB"}
    if value is not None:
        env.update(VPTQ_TUNING="1", VPTQ_K256C_ROWS=str(value))
    r = subprocess.run([sys.executable, "-c", _KNOB_CHILD.format(root=root, tests=os.path.join(root, "tests"))], env=env, cwd=root,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return [s.strip() for s in r.stdout.strip().split("|")]


@pytest.mark.parametrize("knob", [None, 0, 1, 2])
def test_the_knob_decides_what_a_launch_takes(knob):
    """VPTQ_K256C_ROWS (read once per process, with VPTQ_TUNING=1): 0 never, 1 wherever the geometry serves the launch, unset / 2 where
    the rule says so; the family name and the rule's own answer do not move"""
    sweeps8, sweeps4, perm = ",".join(["4"] * 32), ",".join(["2"] * 32), ",".join(["0"] * 32)
    big = f"gemv_k256c dt=f16 dep=0 mode=exact layers=32 sweeps={sweeps8} perm={perm}"
    small = f"gemv_k256c dt=f16 dep=0 mode=exact layers=32 sweeps={sweeps4} perm={perm}"
    nm, ibig, ismall, ifold, rule = _with_knob(knob)
    assert nm == "gemv_k256c_kernel" and rule == "1 0"
    assert ibig == big + (" geom=rows" if knob != 0 else "")
    assert ismall == small + (" geom=rows" if knob == 1 else "")
    assert ifold == big.replace("mode=exact", "mode=folded")


def test_name_and_texts_of_the_launches_existing_tests_pin():
    """the family name stays; the instance text gains ' geom=rows' only where the geometry is taken (device-less queries answer
    for 256 workgroups)"""
    big = cs.fake_descs([(8192, 8192, {})] * 32)
    sweeps = ",".join(["4"] * 32)
    perm = ",".join(["0"] * 32)
    assert name(big, cs.EXACT) == "gemv_k256c_kernel"
    assert instance(big, cs.EXACT) == f"gemv_k256c dt=f16 dep=0 mode=exact layers=32 sweeps={sweeps} perm={perm} geom=rows"
    assert instance(big, 0) == f"gemv_k256c dt=f16 dep=0 mode=folded layers=32 sweeps={sweeps} perm={perm}"
    assert instance(big, cs.EXACT | cs.F32) == f"gemv_k256c dt=f16 dep=0 mode=exact layers=32 sweeps={sweeps} perm={perm}"
    # the chains of the schedule, route-model and weight-bits tests at the production grid and at the forced counts
    for chain, shapes in cs.CHAINS.items():
        descs = cs.fake_descs(shapes)
        layers = [(cdiv(O, 8), I) for I, O, _ in shapes]
        flags = cs.MFMA | cs.EXACT
        if chain in cs.DEPENDENT:
            continue
        assert name(descs, flags) == "gemv_k256c_kernel"
        for w in (256, 3, 13, 23, 37):
            rc, got = lib_rows_plan(descs, flags, w)
            assert rc == 0 and got[0] == r_plan(layers, w)[0], (chain, w, got)
            p = cs.plan(descs, flags, w)
            assert (p["visit"], p["grid"], p["first"], p["rpw"]) == c_plan(layers, w), (chain, w)
    # "routes" is compared bit for bit across workgroup counts by tests/test_chain_schedule_gpu.py: one geometry at all of them
    routes = [(cdiv(O, 8), I) for I, O, _ in cs.CHAINS["routes"]]
    assert {r_plan(routes, w)[0] for w in (256, 304, 3, 13, 23, 37)} == {0}
    k256 = [(2048 - 8, 264), (4096, 264), (6144 + 8, 264), (8192, 264), (10240, 264), (11008, 264), (14336, 264), (1024, 520), (4096 + 8, 264), (2048, 1032)]
    d = cs.fake_descs([(I, O, {}) for I, O in k256])
    assert instance(d, cs.MFMA | cs.EXACT) == "gemv_k256c dt=f16 dep=0 mode=exact layers=10 sweeps=1,2,4,4,5,6,7,1,3,1 perm=0,0,0,0,0,0,0,0,0,0"
    bits = cs.fake_descs([(4096, 72, {})] * 32)
    assert instance(bits, cs.MFMA | cs.EXACT).endswith("perm=" + perm)


# ---------------------------------------------------------------------------------------------- the schedule table of the GPU test
def _descs(shapes):
    return cs.fake_descs([(I, O, dict(bias=b)) for I, O, b in shapes])


@pytest.mark.parametrize("chain,w,covers", run.TABLE, ids=[f"{c}-wg{w}" for c, w, _ in run.TABLE])
def test_table_entry_is_dealt_as_restated_and_covers_what_it_names(chain, w, covers):
    """tests/test_chain_rows_gpu.py's table, no device: the deal the covers are computed from (tests/_chain_rows_run.py:deal) is
    r_plan's and the library's at that workgroup count, and the entry reaches every cover it exists for"""
    shapes = run.CHAINS[chain]
    first, tasks, steps, per_wg = run.deal(shapes, w)
    taken, f2, t2, s2, lr, lc = r_plan([(cdiv(O, 8), I) for I, O, _ in shapes], w)
    assert (first, tasks, steps) == (f2, t2, s2)
    assert max(sum(nt * ns for _, nt, ns in v) for v in per_wg) == lr
    assert sorted((L, nt) for v in per_wg for L, nt, _ in v) == sorted(
        (L, len(range(k, tasks[L], w))) for L in range(len(shapes)) for k in range(min(w, tasks[L])))   # every task dealt once
    rc, got = lib_rows_plan(_descs(shapes), cs.EXACT | cs.MFMA, w)
    assert rc == 0 and got == (taken, w, first, tasks, steps, lr, lc), got
    f = run.facts(shapes, w)
    for c in covers:
        assert run.COVERS[c](f), f"{chain} at {w} workgroups does not cover {c}: {f}"


def test_the_table_reaches_every_cover_and_notices_a_shortened_chain():
    reached = {c for _, _, covers in run.TABLE for c in covers}
    assert reached == set(run.COVERS), set(run.COVERS) ^ reached
    at = lambda chain, w: {c for c, fn in run.COVERS.items() if fn(run.facts(run.CHAINS[chain], w))}   # noqa: E731
    # the figures the chains were written for
    assert "search2" in at("sparse32", 8) and {"search4", "late_start"} <= at("sparse32", 16)
    assert all("tail" in at("sparse32", w) for w in (8, 16, 37)) and "ragged_n" in at("sparse30", 8) & at("sparse31", 8)
    assert run.facts(run.CHAINS["sparse32"], 37)["idle"] == 5 and run.facts(run.CHAINS["sparse32"], 1)["entered"] == 32
    assert run.facts(run.CHAINS["dense"], 1)["entered"] == 18 and run.facts(run.CHAINS["dense"], 1)["same3"] == 9
    assert run.facts(run.CHAINS["dense"], 3)["same3"] == 3 and "visits" in at("dense", 2)
    assert all("phases" in at("dense", w) for w in (1, 2, 3)) and "shapes" in at("dense", 1)
    assert sum(run.tasks_of(O) for _, O, _ in run.CHAINS["dense"]) == 42 and len(run.CHAINS["sparse32"]) == 32
    assert all(run.tasks_of(O) == 1 for _, O, _ in run.CHAINS["sparse32"])
    # a chain cut short loses covers: without its last 4 layers sparse32 has no tail at any count, cut to 16 layers no workgroup of 16 has a second task
    for w in (8, 16, 37):
        assert not run.COVERS["tail"](run.facts(run.CHAINS["sparse32"][:28], w))
    assert not run.COVERS["search4"](run.facts(run.CHAINS["sparse32"][:16], 16))
    assert not run.COVERS["one_wg"](run.facts(run.CHAINS["dense"][:-1], 1))
    # every pool layer stands in several launches (what the schedule-independence check compares) and alone in one
    for c in run.POOL_ORDER:
        assert sum(c in run.NAMED[chain] for chain, _, _ in run.TABLE if chain in run.NAMED) >= 2 and run.NAMED["one" + c] == [c]
    assert max(I * O for I, O, _ in run.POOL.values()) < 16 << 20
    assert set(run.WGS) == {1, 2, 3, 4, 8, 16, 37} and run.ONES_AT in run.WGS


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_the_rule_takes_the_natural_launch(cus):
    """the launch tests/test_chain_rows_gpu.py and tests/test_operand_placement_gpu.py run without a knob: the rule gives it to the
    rows geometry at the workgroup counts of the devices the library knows"""
    shapes = run.natural_shapes(cus)
    assert len(shapes) == 32 and {I for I, _, _ in shapes} == {128, 136, 248, 264}
    assert {O % 8 for _, O, _ in shapes} == {0, 4} and len({run.tasks_of(O) for _, O, _ in shapes}) == 2   # ragged last tasks
    rc, got = lib_rows_plan(_descs(shapes), cs.EXACT, cus)
    assert rc == 0 and got[0] == 1 and got[1] == cus and sum(got[3]) >= cus, got
    assert got[:5] == (1, cus) + run.deal(shapes, cus)[:3]
