"""The persistent chain launch in its second geometry, "rows per wave" (gemv_k256c_rows_kernel, gemv_k256r.hip), under the schedules
it deals and in the launch the product takes.

1. THE SCHEDULE TABLE (tests/_chain_rows_run.py:TABLE): chains x forced workgroup counts, the geometry forced with
VPTQ_K256C_ROWS=1 (VPTQ_K256C_WGS; both read once per process: one child process per workgroup count, tests/_chain_rows_run.py,
runs all of that count's chains and the tests here check what it wrote).  What each entry exists to cover - layer searches of several
rounds of four headers, searches into the padding headers and past n_layers, idle workgroups, one workgroup walking 18 and 32 layers,
consecutive tasks of one layer, runs of one-step visits, every visit length from 1 to 5, a switch at every queue slot, the edge
shapes of the pool - is asserted without a device in tests/test_chain_rows_cpu.py.  The older chains "switch" and "few" at 4
workgroups: vector-rows that are no multiple of 8 or 128 and O no multiple of 8 (a ragged last workgroup-task, idle waves, rows past
N), widths 128, 136, 2048 + 8 and 4096 (a single step, columns past G, many steps), layers of different widths following each other
(a workgroup switches images), 3 - 4 tasks per workgroup over four layers (both image buffers reused in both directions), a second
task of the same layer, fewer tasks than workgroups (a workgroup returns at once), output bias present and absent.

Bars, per (chain, workgroups), every layer, every output:
  (a) the instance text ends in " geom=rows";
  (b) the fp64 model of the reference's roundings with _arith_model.check_outputs' own bound (what
      tests/test_route_models_k256_gpu.py holds the exact chain rows to);
  (c) at least 0.95 of a layer's outputs bit-identical to one launch per layer with VPTQ_GEMV_EXACT (bench.py's bar);
  (d) SCHEDULE INDEPENDENCE: a pool layer's 16-bit outputs are the same bits in every chain, at every position and at every
      workgroup count in which the layer (with its x) occurs, and the bits of a launch of that layer alone.  An equality, not a
      measurement: a row group belongs to one wave, each lane sums its column chunk over the column blocks in order, and the 16
      lane partials are added in one fixed tree - neither the workgroup that runs the task, nor its neighbours, nor what it ran before
      enter a sum;
  (e) the same launch again into the same buffers, and again behind a launch of gemv_k256c_kernel, repeats the bits;
  (f) every y of a chain lies in ONE allocation prefilled with a sentinel, >= 64 sentinel elements in front of and behind each: the
      guards come back untouched and no NaN prefill survives inside a y.
W through one-hot activations is vptq_dequant's bit for bit over the finite special-value table (tests/test_weight_bits_gpu.py's
check_bits: -0 == +0, fp16 has no excepted class), and that file's activation variants (subnormal-only, +-0 / largest value, the
overflow layer with its NaN-for-infinity class) run through this geometry in the 4-workgroup child with its own checks.

2. THE LAUNCH THE PRODUCT TAKES, in this process and without a knob: 32 narrow layers sized by the device's compute units
(tests/_chain_rows_run.py:natural_shapes) which the rule itself gives to this geometry; bars (b), (c), (f), bit identity to the same
launch with its layers in reversed order, and hipGraph replay after every x was rewritten in place.

A child that does not end with exit code 0 (a signal, an abort, a timeout, a HIP error) is remembered: no further child and no
further launch of this file starts after it - the remaining tests fail at once with that child's tail."""
import ctypes as C
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import _arith_model as am
import _chain_rows_run as run
from oracle import vptq_oracle as vo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WGS = 4
EXACT, MFMA = run.EXACT, run.MFMA

_OUT = {}       # workgroup count -> what its child wrote
_DEAD = []      # [(workgroups, what happened)] of the first child that did not end well


def _stop_if_dead():
    assert not _DEAD, f"not run: the child at {_DEAD[0][0]} workgroups did not end well, nothing is launched after it\n{_DEAD[0][1]}"


def _child(w, tmp_path_factory):
    if w in _OUT:
        return _OUT[w]
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _stop_if_dead()
    assert w <= torch.cuda.get_device_properties(0).multi_processor_count, "forced counts stay within the CUs"
    path = str(tmp_path_factory.mktemp(f"rows{w}") / "out.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("VPTQ_") or k == "VPTQ_HIP_LIB"}
    env.update(VPTQ_TUNING="1", VPTQ_K256C_ROWS="1", VPTQ_K256C_WGS=str(w))
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_chain_rows_run.py"), path] + run.jobs_at(w), cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as err:
        _DEAD.append((w, f"timeout after {err.timeout} s\n{str(err.stdout)[-3000:]}\n{str(err.stderr)[-3000:]}"))
        _stop_if_dead()
    if r.returncode != 0:
        _DEAD.append((w, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"))
        _stop_if_dead()
    print(f"child at {w} workgroups, jobs {run.jobs_at(w)}: {time.time() - t0:.1f} s")
    with np.load(path) as z:
        _OUT[w] = {k: z[k] for k in z.files}
    return _OUT[w]


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    return _child(WGS, tmp_path_factory)


def _cdiv(a, b):
    return -(-a // b)


def _groups(O):
    return _cdiv(_cdiv(O, 8), 8)   # row groups of 8 vector-rows


def _tasks(chain):
    return [_cdiv(_groups(O), 16) for _, O, _ in run.CHAINS[chain]]


def _ys(out, chain, key="buf"):
    """the outputs of every layer out of the chain's one buffer"""
    outs = [O for _, O, _ in run.CHAINS[chain]]
    offs, total = run.y_layout(outs)
    buf = out[f"{chain}.{key}"]
    assert buf.shape == (total,)
    return [buf[o:o + O] for o, O in zip(offs, outs)]


def _guards_of(buf, outs, what):
    """bar (f) of one buffer that holds a y of each of `outs` elements (tests/_chain_rows_run.py:guarded_ys)"""
    offs, total = run.y_layout(outs)
    assert buf.shape == (total,)
    inside = np.zeros(total, bool)
    for o, O in zip(offs, outs):
        assert o >= run.GUARD and not inside[o - run.GUARD:o].any()
        inside[o:o + O] = True
    assert not inside[-run.GUARD:].any()
    sentinel = vo.from_f32(np.array([run.SENTINEL], np.float32), "f16")[0]
    bad = np.flatnonzero((buf != sentinel) & ~inside)
    assert bad.size == 0, f"{what}: {bad.size} guard elements written, first at elements {bad[:8].tolist()} of {total} (y offsets {offs})"
    nan = np.flatnonzero(((buf & 0x7fff) > 0x7c00) & inside)
    assert nan.size == 0, f"{what}: {nan.size} outputs not written (the NaN prefill is still there), first at {nan[:8].tolist()}"


def _guards_intact(out, chain, key="buf"):
    _guards_of(out[f"{chain}.{key}"], [O for _, O, _ in run.CHAINS[chain]], f"{chain} [{key}]")


def test_the_chains_cover_what_they_are_for():
    t = _tasks("switch")
    per_wg = [[] for _ in range(WGS)]
    k = 0
    for L, n in enumerate(t):
        for _ in range(n):
            per_wg[k % WGS].append(L)
            k += 1
    assert min(len(v) for v in per_wg) >= 3                                       # >= 3 tasks per workgroup
    assert max(len(set(v)) for v in per_wg) >= 4                                  # four layers: both buffers reused both ways
    assert any(len(v) != len(set(v)) for v in per_wg)                             # a second task of the same layer
    assert sum(_tasks("few")) < WGS                                               # a workgroup returns at once
    shapes = run.CHAINS["switch"] + run.CHAINS["few"]
    assert {I for I, _, _ in shapes} >= {128, 136, 2048 + 8, 4096}
    assert any(O % 8 for _, O, _ in shapes) and all(_cdiv(O, 8) % 8 for _, O, _ in run.CHAINS["switch"])
    assert sum(_groups(O) % 16 != 0 for _, O, _ in shapes) >= 5                   # idle waves in a last task ...
    assert any(_groups(O) % 16 == 0 for _, O, _ in shapes)                        # ... and a full one whose last row group is short
    assert {b for _, _, b in shapes} == {True, False}


OLD = ("few", "switch")


@pytest.mark.parametrize("chain", OLD)
def test_geometry_is_the_one_asked_for(chain, out):
    assert str(out[f"{chain}.instance"]).startswith("gemv_k256c dt=f16 dep=0 mode=exact ") and str(out[f"{chain}.instance"]).endswith(" geom=rows")
    assert "geom=" not in str(out[f"{chain}.folded_instance"]) and "mode=folded" in str(out[f"{chain}.folded_instance"])
    assert str(out["special.instance"]).endswith(" geom=rows")


@functools.lru_cache(maxsize=None)
def _model(chain, i):
    """the fp64 model of layer i of a chain; a pool layer's is computed once for all its places"""
    if chain in run.NAMED and chain != "one" + run.NAMED[chain][i]:
        return _model("one" + run.NAMED[chain][i], 0)
    return am.model(am.pieces(run.layer_of(chain, i)), run.x_of(chain, i), "exact")


def _check_models(out, chain, what):
    for i, y in enumerate(_ys(out, chain)):
        m, a = _model(chain, i)
        am.check_outputs(vo.to_f32(y, "f16").astype(np.float64).reshape(1, -1), m, a, "f16", False,
                         what=f"{what} layer {i} {run.CHAINS[chain][i]}")


def _check_shares(out, chain, what):
    for i, got in enumerate(_ys(out, chain)):
        ref = out[f"{chain}.single.{i}"]
        assert got.shape == ref.shape
        frac = float((got == ref).mean())
        print(f"{what} layer {i} {run.CHAINS[chain][i]}: {frac:.4f} bit-identical to the one-layer launch")
        assert frac >= 0.95, (what, i, frac)


def _check_relaunches(out, chain, what):
    for i, (y, again, after) in enumerate(zip(_ys(out, chain), _ys(out, chain, "again"), _ys(out, chain, "after"))):
        assert np.array_equal(y, again), f"{what} layer {i}: the second launch differs"
        assert np.array_equal(y, after), f"{what} layer {i}: differs behind a gemv_k256c launch"


@pytest.mark.parametrize("chain", OLD)
def test_every_output_vs_the_fp64_model(chain, out):
    _check_models(out, chain, chain)


@pytest.mark.parametrize("chain", OLD)
def test_bit_identical_share_vs_one_launch_per_layer(chain, out):
    _check_shares(out, chain, chain)


@pytest.mark.parametrize("chain", OLD)
def test_relaunches_repeat_the_bits(chain, out):
    _check_relaunches(out, chain, chain)


def test_special_weights_read_back(out):
    from test_weight_bits_gpu import check_bits
    import _dequant_specials as sp
    L = run.special_layer()
    W = out["special.W"]
    assert W.shape == (L.out_features, L.in_features)
    sp.same_bits(W, vo.dequant(L, ref_residual_mask_quirk=False), "f16", "vptq_dequant against the oracle")
    feats = run.special_features()
    used, _ = check_bits(out["special.columns"], W, feats, "f16", "gemv_k256c", "rows geometry, f16 special table")
    assert used == 0


@pytest.mark.parametrize("variant", run.VARIANTS)
def test_activation_variants_through_this_geometry(variant, out):
    """tests/test_weight_bits_gpu.py's check of that name, run by the 4-workgroup child on 32 copies of a 2040-column layer whose
    instance text it asserts to end in " geom=rows": the child's verdict"""
    verdict = str(out[f"variant.{variant}"])
    assert verdict == "", verdict


# ---------------------------------------------------------------------------------------------- the schedule table
@pytest.mark.parametrize("chain,w", [pytest.param(c, w, id=f"{c}-wg{w}") for c, w, _ in run.TABLE])
def test_table_entry(chain, w, tmp_path_factory):
    """bars (a), (b), (c), (e) and (f) of one (chain, workgroups) of the table"""
    o = _child(w, tmp_path_factory)
    what = f"{chain} at {w} workgroups"
    inst = str(o[f"{chain}.instance"])
    assert inst.startswith(f"gemv_k256c dt=f16 dep=0 mode=exact layers={len(run.CHAINS[chain])} ") and inst.endswith(" geom=rows"), inst
    for key in ("buf", "again", "after"):
        _guards_intact(o, chain, key)
    _check_models(o, chain, what)
    _check_shares(o, chain, what)
    _check_relaunches(o, chain, what)


@pytest.mark.parametrize("c", run.POOL_ORDER)
def test_schedule_independence_of_a_pool_layer(c, tmp_path_factory):
    """bar (d): the layer's bits in every chain, position and workgroup count of the table against its launch alone"""
    one = _child(run.ONES_AT, tmp_path_factory)
    chain1 = "one" + c
    assert str(one[f"{chain1}.instance"]).endswith(" geom=rows")
    _guards_intact(one, chain1)
    _check_models(one, chain1, f"{c} alone")
    _check_shares(one, chain1, f"{c} alone")
    want = _ys(one, chain1)[0]
    places = 0
    for chain, w, _ in run.TABLE:
        if chain not in run.NAMED:
            continue
        o = _child(w, tmp_path_factory)
        for i, y in enumerate(_ys(o, chain)):
            if run.NAMED[chain][i] != c:
                continue
            diff = np.flatnonzero(y != want)
            assert diff.size == 0, (f"pool layer {c} {run.POOL[c]}: {diff.size} of {y.size} outputs of layer {i} of {chain} at {w} workgroups differ "
                                    f"in their bits from the layer's launch alone, first outputs {diff[:8].tolist()}")
            places += 1
    assert places >= 2, (c, places)
    print(f"pool layer {c} {run.POOL[c]}: the same bits in {places} places and alone")


# ---------------------------------------------------------------------------------------------- the launch the product takes
def _chain_call(descs, n, xs, ys, flags, dev):
    from vptq_amd import _backend as B
    xp = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
    yp = (C.c_void_p * n)(*[y.data_ptr() for y in ys])
    B.check(B.lib().vptq_quant_gemv_chain(descs, n, xp, yp, 1, flags, None, 0, B.current_stream_ptr(dev)), "vptq_quant_gemv_chain")


class Natural:
    """the natural launch on this device: modules, descriptors in the given order, activations"""

    def __init__(self, dev):
        from vptq_amd import _backend as B
        from _gpu_util import spec_to_module, module_desc, bits_to_tensor
        self.dev, self.cus = dev, torch.cuda.get_device_properties(dev).multi_processor_count
        self.shapes = run.natural_shapes(self.cus)
        self.n = len(self.shapes)
        self.specs = [run.natural_layer(self.cus, i) for i in range(self.n)]
        self.mods = [spec_to_module(L, dev) for L in self.specs]
        self.keep = [module_desc(m) for m in self.mods]
        self.xbits = [run.natural_x(self.cus, i) for i in range(self.n)]
        self.xs = [bits_to_tensor(x, "f16", dev).reshape(-1) for x in self.xbits]
        self.B = B

    def descs(self, order):
        return (self.B.LayerDesc * self.n)(*[self.keep[i][0] for i in order])

    def launch(self, order):
        """-> (the guarded buffer's bits, the y bits of every layer by LAYER number)"""
        from _gpu_util import tensor_to_bits
        buf, ys = run.guarded_ys([self.shapes[i][1] for i in order], self.dev)
        _chain_call(self.descs(order), self.n, [self.xs[i] for i in order], ys, EXACT, self.dev)
        torch.cuda.synchronize()
        bits = tensor_to_bits(buf)
        offs, _ = run.y_layout([self.shapes[i][1] for i in order])
        return bits, {i: bits[o:o + self.shapes[i][1]] for i, o in zip(order, offs)}


@pytest.fixture(scope="module")
def natural():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _stop_if_dead()
    from vptq_amd import _backend as B
    B.lib()
    nat = Natural(torch.device("cuda", 0))
    order = list(range(nat.n))
    nat.buf, nat.y = nat.launch(order)
    nat.rbuf, nat.ry = nat.launch(order[::-1])
    return nat


def test_natural_launch_takes_the_rows_geometry(natural):
    """no knob: the rule itself (workgroups = 0: what a launch uses) gives the chooser's launch to this geometry on this device"""
    import test_chain_rows_cpu as cpu
    nat = natural
    descs = nat.descs(range(nat.n))
    rc, got = cpu.lib_rows_plan(descs, EXACT, 0)
    assert rc == 0 and got[0] == 1 and got[1] == nat.cus and sum(got[3]) >= nat.cus, (nat.cus, got)
    assert got[:5] == (1, nat.cus) + run.deal(nat.shapes, nat.cus)[:3]
    assert cpu.name(descs, EXACT) == "gemv_k256c_kernel"
    inst = cpu.instance(descs, EXACT)
    assert inst.startswith("gemv_k256c dt=f16 dep=0 mode=exact layers=32 ") and inst.endswith(" geom=rows"), inst
    assert cpu.instance(nat.descs(range(nat.n)[::-1]), EXACT).endswith(" geom=rows")


def test_natural_launch_vs_the_fp64_model_and_one_launch_per_layer(natural):
    from _gpu_util import gemv_abi, tensor_to_bits
    nat = natural
    _guards_of(nat.buf, [s[1] for s in nat.shapes], "the natural launch")
    for i, L in enumerate(nat.specs):
        m, a = am.model(am.pieces(L), nat.xbits[i], "exact")
        am.check_outputs(vo.to_f32(nat.y[i], "f16").astype(np.float64).reshape(1, -1), m, a, "f16", False,
                         what=f"natural launch layer {i} {nat.shapes[i]}")
        ref = tensor_to_bits(gemv_abi(nat.mods[i], nat.xs[i].reshape(1, 1, -1), EXACT | MFMA)).reshape(-1)
        frac = float((nat.y[i] == ref).mean())
        print(f"natural launch layer {i} {nat.shapes[i]}: {frac:.4f} bit-identical to the one-layer launch")
        assert frac >= 0.95, (i, frac)


def test_natural_launch_in_reversed_order_gives_the_same_bits(natural):
    """bar (d) for the natural launch: every layer gets other workgroups, other neighbours and another place in their walks"""
    nat = natural
    _guards_of(nat.rbuf, [s[1] for s in nat.shapes][::-1], "the reversed natural launch")
    for i in range(nat.n):
        diff = np.flatnonzero(nat.y[i] != nat.ry[i])
        assert diff.size == 0, f"layer {i} {nat.shapes[i]}: {diff.size} outputs differ between the two orders, first {diff[:8].tolist()}"


def test_natural_launch_replayed_from_a_graph(natural):
    """captured on a side stream; every x rewritten in place, replayed, twice: the bits of an eager launch on the same x"""
    from _gpu_util import bits_to_tensor, tensor_to_bits
    nat = natural
    _stop_if_dead()
    dev, n = nat.dev, nat.n
    order = list(range(n))
    descs = nat.descs(order)
    xs = [x.clone() for x in nat.xs]
    outs = [s[1] for s in nat.shapes]
    gbuf, gys = run.guarded_ys(outs, dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _chain_call(descs, n, xs, gys, EXACT, dev)
    torch.cuda.current_stream(dev).wait_stream(s)
    seen = [nat.buf]
    for k in (1, 2):
        for i in range(n):
            xs[i].copy_(bits_to_tensor(run.natural_x(nat.cus, i, seed=k), "f16", dev).reshape(-1))
        for y in gys:
            y.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize(dev)
        replayed = tensor_to_bits(gbuf)
        _guards_of(replayed, outs, f"replay {k}")
        ebuf, eys = run.guarded_ys(outs, dev)
        _chain_call(descs, n, xs, eys, EXACT, dev)
        torch.cuda.synchronize(dev)
        eager = tensor_to_bits(ebuf)
        assert np.array_equal(replayed, eager), f"replay {k}: {int((replayed != eager).sum())} elements differ from the eager launch on the same x"
        assert all(not np.array_equal(replayed, b) for b in seen), "the replay did not read the rewritten x"
        seen.append(replayed)
