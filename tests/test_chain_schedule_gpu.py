"""The persistent chain launch (gemv_k256c.hip) under the schedules it deals: a table of chains x workgroup counts x arithmetics.

Each entry asserts its plan through vptq_quant_gemv_chain_plan (visit length, grid, what it exists to cover: layer
switches, an image buffer handed to a third layer, partial-sum slots that wrap, switches between sweep counts, partial
blocks, wrapped layers), runs the chain, checks every output of every layer - 16-bit and VPTQ_GEMV_OUT_F32 - against the
layer's float64 model (tests/_arith_model.py), and asserts that the outputs are bit-identical to the same chain's at the
production grid: a row group is summed by one workgroup, over its sweeps in order, with a fixed tree over the waves, so
the schedule must not change a bit.  Forced workgroup counts (VPTQ_K256C_WGS, read once per process) run in a child process
(tests/_chain_schedule_run.py), one at a time.  The file runs in about 45 s on one MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _arith_model as am
import _chain_schedule as cs
import test_route_models_gpu as rm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROD = 0   # the production grid: no override
ARITHS = ("exact", "folded", "selective")


def E(chain, dt, arith, wgs, visit, covers=()):
    """covers: what the entry's plan must exercise (names of COVERS)"""
    e = dict(chain=chain, dt=dt, arith=arith, wgs=wgs, visit=visit, covers=tuple(covers))
    return pytest.param(e, id=f"{chain}-{dt}-{arith}-{'prod' if wgs == PROD else f'wg{wgs}'}")


COVERS = {
    "switch": lambda c: c["max_layers"] >= 2,          # a layer switch
    "reuse": lambda c: c["max_layers"] >= 3,           # an image buffer handed to a third layer
    "slots": lambda c: c["max_block"] >= 5,            # >= 5 row groups of one layer: the 4 partial-sum slots wrap
    "ns_switch": lambda c: c["ns_switches"] > 0,       # a switch between layers of different sweeps per row group
    "partial": lambda c: c["partial"] > 0,             # a block shorter than the others
    "wrap": lambda c: c["wrapped"] > 0,                # a layer whose blocks wrap past the last workgroup
}
ALL = tuple(COVERS)

ENTRIES = []
for dt in ("f16", "bf16"):
    for a in ARITHS:
        ENTRIES += [E("routes", dt, a, PROD, 0, ("switch", "ns_switch", "wrap")),
                    E("routes", dt, a, 3, 32, ALL),
                    E("routes", dt, a, 13, 16, ALL),
                    E("routes", dt, a, 23, 8, ALL),
                    E("routes", dt, a, 37, 0, ("switch", "reuse", "ns_switch", "wrap"))]
ENTRIES += [
    E("llama8b", "f16", "exact", PROD, 0, ("switch", "reuse", "ns_switch", "wrap")),
    E("visit32", "f16", "exact", PROD, 32, ALL),
    E("visit16", "bf16", "folded", PROD, 16, ALL),
    E("visit8", "f16", "selective", PROD, 8, ALL),
    E("dependent", "f16", "folded", PROD, 0, ("switch", "reuse", "ns_switch")),
    E("dependent", "f16", "folded", 3, 0, ("switch", "reuse", "slots", "ns_switch", "partial")),
    E("dependent", "bf16", "folded", PROD, 0, ("switch", "reuse", "ns_switch")),
    E("dependent", "bf16", "folded", 7, 0, ("switch", "reuse", "slots", "ns_switch", "partial")),
]


def _jobs(wgs):
    return sorted({(e.values[0]["chain"], e.values[0]["dt"], e.values[0]["arith"]) for e in ENTRIES if e.values[0]["wgs"] == wgs})


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vptq_amd import _backend as B
    B.lib()
    return torch.device("cuda", 0)


_OUT = {}      # workgroup count -> outputs of every job at that count
_CHAINS = {}   # (chain, dt) -> cs.Chain


def _chain(chain, dt, dev):
    if (chain, dt) not in _CHAINS:
        _CHAINS[(chain, dt)] = cs.Chain(chain, dt, dev)
    return _CHAINS[(chain, dt)]


def _child_env(wgs):
    env = {k: v for k, v in os.environ.items() if not k.startswith("VPTQ_") or k == "VPTQ_HIP_LIB"}
    env.update(VPTQ_TUNING="1", VPTQ_K256C_WGS=str(wgs))
    return env


def _outputs(wgs, dev, tmp_path_factory):
    if wgs not in _OUT:
        if wgs == PROD:
            _OUT[wgs] = cs.run_jobs(_jobs(PROD), dev)
        else:
            assert wgs <= torch.cuda.get_device_properties(dev).multi_processor_count, "forced counts stay within the CUs"
            path = str(tmp_path_factory.mktemp(f"wg{wgs}") / "out.npz")
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_chain_schedule_run.py"), path]
                               + [":".join(j) for j in _jobs(wgs)], cwd=ROOT, env=_child_env(wgs), capture_output=True,
                               text=True, timeout=300)
            assert r.returncode == 0, f"child at {wgs} workgroups: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
            with np.load(path) as z:
                _OUT[wgs] = {k: z[k] for k in z.files}
    return _OUT[wgs]


_MODELS = {}   # (chain, dt, arith) -> [(m, a)] per layer (independent chains)


def _models(ch, arith):
    """the fp64 model of every layer; pieces computed once per distinct layer and shared by the arithmetics of the table"""
    key = (ch.name, ch.dt)
    if (key + (arith,)) not in _MODELS:
        ariths = sorted({e.values[0]["arith"] for e in ENTRIES if (e.values[0]["chain"], e.values[0]["dt"]) == key})
        xs = {a: ch.inputs(a) for a in ariths}
        res = {a: [None] * len(ch.specs) for a in ariths}
        users = {}
        for i, L in enumerate(ch.specs):
            users.setdefault(id(L), []).append(i)
        for idx in users.values():   # (one distinct layer's pieces at a time: the tall layers' are hundreds of MB)
            P = am.pieces(ch.specs[idx[0]])
            for i in idx:
                for a in ariths:
                    x, hot = xs[a][i]
                    if a == "selective":
                        rm._hot_rules_agree(P, x, hot)
                    res[a][i] = am.model(P, x, a, hot_blocks=hot if a == "selective" else ())
            del P
        for a in ariths:
            _MODELS[key + (a,)] = res[a]
    return _MODELS[key + (arith,)]


def _check_independent(ch, arith, out, key):
    models = _models(ch, arith)
    xs = ch.inputs(arith)
    for i, L in enumerate(ch.specs):
        m, a = models[i]
        y16 = cs_f64(out[f"{key}.y16.{i}"], ch.dt)
        y32 = out[f"{key}.y32.{i}"].astype(np.float64)
        try:
            am.check_outputs(y16.reshape(1, -1), m, a, ch.dt, False, what=f"{key} layer {i} [16-bit]")
            am.check_outputs(y32.reshape(1, -1), m, a, ch.dt, True, what=f"{key} layer {i} [fp32]")
        except AssertionError:
            # (name the models the output would meet; no fallback - this raises)
            rm._check(y16, y32, L, xs[i][0], dict(arith=arith), xs[i][1], what=f"{key} layer {i}")
            raise


_DEP_PIECES = {}


def _check_dependent(ch, arith, out, key):
    """layer i is checked on the input it actually read: layer i - 1's 16-bit output"""
    xin = ch.inputs(arith)[0][0]
    for i, L in enumerate(ch.specs):
        if (ch.dt, i) not in _DEP_PIECES:
            _DEP_PIECES[(ch.dt, i)] = am.pieces(L)
        bits = out[f"{key}.y16.{i}"]
        m, a = am.model(_DEP_PIECES[(ch.dt, i)], xin, arith)
        am.check_outputs(cs_f64(bits, ch.dt).reshape(1, -1), m, a, ch.dt, False, what=f"{key} layer {i} [16-bit]")
        xin = bits.reshape(1, 1, -1)


def cs_f64(bits, dt):
    from oracle import vptq_oracle as vo
    return vo.to_f32(np.asarray(bits), dt).astype(np.float64)


@pytest.mark.parametrize("e", ENTRIES)
def test_chain_schedule_vs_model_and_production(e, dev, tmp_path_factory):
    ch = _chain(e["chain"], e["dt"], dev)
    # 1. the plan: through the query, as the kernel gets it
    p = ch.plan(e["arith"], e["wgs"])
    cov = cs.coverage(p, ch.ng, ch.ns)
    assert p["visit"] == e["visit"], cov
    if e["wgs"] != PROD:
        assert p["grid"] == e["wgs"], cov
    for c in e["covers"]:
        assert COVERS[c](cov), f"the plan does not cover {c}: {cov}"
    # 2. the run (a child process for a forced count); the launch's own plan is the one asserted
    out = _outputs(e["wgs"], dev, tmp_path_factory)
    key = f"{e['chain']}.{e['dt']}.{e['arith']}"
    seen = out[key + ".plan"].tolist()
    assert seen == [p["visit"], p["grid"]] + p["first"] + p["rpw"], "the plan of the call differs from the query's"
    # 3. every output of every layer against its model
    if ch.dependent:
        _check_dependent(ch, e["arith"], out, key)
    else:
        _check_independent(ch, e["arith"], out, key)
    # 4. bit-identical to the production grid
    if e["wgs"] != PROD:
        prod = _outputs(PROD, dev, tmp_path_factory)
        for k in sorted(k for k in out if k.startswith(key + ".y")):
            a, b = out[k], prod[k]
            diff = int((a.view(np.uint16 if a.dtype == np.uint16 else np.uint32)
                        != b.view(np.uint16 if b.dtype == np.uint16 else np.uint32)).sum())
            assert diff == 0, f"{k}: {diff} of {a.size} outputs differ in their bits from the production grid"


def test_schedule_table_coverage(dev):
    """the table reaches every visit length in every arithmetic (fp16), two per arithmetic in bf16, and each schedule
    property somewhere"""
    visits, covered = {}, set()
    for prm in ENTRIES:
        e = prm.values[0]
        ch = _chain(e["chain"], e["dt"], dev)
        p = ch.plan(e["arith"], e["wgs"])
        cov = cs.coverage(p, ch.ng, ch.ns)
        visits.setdefault((e["dt"], e["arith"]), set()).add(p["visit"])
        covered |= {c for c, f in COVERS.items() if f(cov)}
    for a in ARITHS:
        assert visits[("f16", a)] >= {0, 8, 16, 32}, (a, visits[("f16", a)])
        assert len(visits[("bf16", a)]) >= 2, (a, visits[("bf16", a)])
    assert covered == set(COVERS), set(COVERS) - covered
