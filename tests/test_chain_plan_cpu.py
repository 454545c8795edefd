"""vptq_quant_gemv_chain_plan (ABI 11) on the library built here, no device: how one persistent chain launch deals its row
groups to explicit workgroup counts, for seeded random lists of eligible layers (tests/_chain_schedule.py expands a plan)."""
import numpy as np
import pytest

import _chain_schedule as cs
from vptq_amd import _backend as B

WORKGROUPS = (256, 37, 13, 7, 3)
VISITS = (32, 16, 8)   # sweeps per visit the blocks are sized for, longest first (gemv_k256c.hip: c_visit)


def _random_shapes(rng, n):
    """eligible layers: I a multiple of 8 (1 - 6 sweeps per row group), O any, some with bias"""
    shapes = []
    for _ in range(n):
        I = 8 * int(rng.choice([rng.integers(1, 257), rng.integers(257, 1537)]))
        O = int(rng.choice([rng.integers(1, 600), rng.integers(600, 40000)]))
        shapes.append((I, O, dict(bias=bool(rng.integers(0, 2)))))
    return shapes


def _blocks(descs, workgroups, visit):
    """blocks of a list at a visit length: rpw = max(ceil(groups / workgroups), ceil(visit / sweeps))"""
    total = 0
    for d in descs:
        g, s = cs.groups(d.num_indices), cs.sweeps(d.group_size)
        rpw = max(-(-g // workgroups), -(-visit // s) if visit else 1, 1)
        total += -(-g // rpw)
    return total


CASES = [(seed, wg, dep) for seed in range(6) for wg in WORKGROUPS for dep in (False, True)]


@pytest.mark.parametrize("seed,wg,dep", CASES, ids=[f"s{s}-wg{w}-{'dep' if d else 'ind'}" for s, w, d in CASES])
def test_plan_deals_every_row_group_once(seed, wg, dep):
    rng = np.random.default_rng(1000 * seed + wg + dep)
    n = int(rng.integers(1, 33))
    shapes = _random_shapes(rng, n)
    descs = cs.fake_descs(shapes, dtype=int(rng.integers(0, 2)))
    p = cs.plan(descs, cs.MFMA | (cs.DEP if dep else 0), wg)
    ng, ns = cs.layer_counts(descs)
    blocks = [-(-g // r) for g, r in zip(ng, p["rpw"])]
    # grid = min(blocks, workgroups)
    assert p["grid"] == min(sum(blocks), wg)
    # the visit: the longest of 32 / 16 / 8 whose blocks number at least 2 x the workgroups, else 0; dependent lists: 0
    want = 0 if dep else next((v for v in VISITS if _blocks(descs, wg, v) >= 2 * wg), 0)
    assert p["visit"] == want
    assert sum(blocks) == _blocks(descs, wg, p["visit"])
    if dep:
        assert p["first"] == [0] * n, "dependent: every layer starts at workgroup 0"
    else:
        # the layers continue each other's round robin
        assert p["first"] == [int(np.sum(blocks[:i])) % p["grid"] for i in range(n)]
    per_wg = cs.expand(p, ng, ns)
    for L in range(n):
        owners = [w for w, v in enumerate(per_wg) for e in v if e[0] == L]
        assert len(owners) == len(set(owners)), f"layer {L}: a workgroup owns two of its blocks"
        rows = sorted((b, e) for v in per_wg for (l, b, e, _) in v if l == L)
        assert rows[0][0] == 0 and rows[-1][1] == ng[L] and all(a[1] == b[0] for a, b in zip(rows, rows[1:])), \
            f"layer {L}: row groups not dealt exactly once"
        assert all(e - b <= p["rpw"][L] for b, e in rows)


def test_plan_of_the_route_chain_at_the_table_counts():
    """the schedule test's chain (the route-model chain twice over) reaches every visit length at its forced counts"""
    descs = cs.fake_descs(cs.CHAINS["routes"])
    ng, ns = cs.layer_counts(descs)
    got = {wg: cs.plan(descs, cs.MFMA, wg) for wg in (256, 37, 23, 13, 3)}
    assert {wg: p["visit"] for wg, p in got.items()} == {256: 0, 37: 0, 23: 8, 13: 16, 3: 32}
    c = cs.coverage(got[3], ng, ns)
    assert c["max_layers"] >= 3 and c["max_block"] >= 5 and c["ns_switches"] > 0 and c["partial"] > 0 and c["wrapped"] > 0, c


def test_plan_refuses_what_the_persistent_launch_does_not_take():
    ok = cs.fake_descs([(4096, 4096, {})] * 3)
    v, g = B.C.c_int(), B.C.c_int()
    first, rpw = (B.C.c_int * 3)(), (B.C.c_int * 3)()
    lib = B.lib()
    assert lib.vptq_quant_gemv_chain_plan(ok, 3, cs.MFMA, 64, B.C.byref(v), B.C.byref(g), first, rpw) == 0
    assert lib.vptq_quant_gemv_chain_plan(ok, 0, 0, 64, B.C.byref(v), B.C.byref(g), first, rpw) == B.E_SHAPE
    assert lib.vptq_quant_gemv_chain_plan(ok, 3, 0, -1, B.C.byref(v), B.C.byref(g), first, rpw) == B.E_SHAPE
    assert lib.vptq_quant_gemv_chain_plan(ok, 3, 0, 64, None, B.C.byref(g), first, rpw) == B.E_NULL
    mixed = cs.fake_descs([(4096, 4096, {})] * 3)
    mixed[1].dtype = 1
    assert lib.vptq_quant_gemv_chain_plan(mixed, 3, 0, 64, B.C.byref(v), B.C.byref(g), first, rpw) == B.E_UNSUPPORTED
    # the reference's roundings / selective: independent lists only
    assert lib.vptq_quant_gemv_chain_plan(ok, 3, cs.EXACT | cs.DEP, 64, B.C.byref(v), B.C.byref(g), first, rpw) == B.E_UNSUPPORTED
    assert lib.vptq_quant_gemv_chain_plan(ok, 3, cs.SEL | cs.DEP, 64, B.C.byref(v), B.C.byref(g), first, rpw) == B.E_UNSUPPORTED
    # the selective launch covers up to 32768 columns
    wide = cs.fake_descs([(32768 + 8, 64, {})])
    assert lib.vptq_quant_gemv_chain_plan(wide, 1, cs.SEL, 64, B.C.byref(v), B.C.byref(g), first, rpw) == B.E_UNSUPPORTED
    assert lib.vptq_quant_gemv_chain_plan(wide, 1, 0, 64, B.C.byref(v), B.C.byref(g), first, rpw) == 0
