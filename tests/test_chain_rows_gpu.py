"""The persistent chain launch in its second geometry, "rows per wave" (gemv_k256c_rows_kernel, gemv_k256r.hip), forced with
VPTQ_K256C_ROWS=1 at 4 workgroups (VPTQ_K256C_WGS; both read once per process: one child process, tests/_chain_rows_run.py,
runs everything and the tests here check what it wrote).

The chains (tests/_chain_rows_run.py:CHAINS): vector-rows that are no multiple of 8 or 128 and O no multiple of 8 (a ragged last
workgroup-task, idle waves, rows past N), widths 128, 136, 2048 + 8 and 4096 (a single step, columns past G, many steps), layers of
different widths following each other (a workgroup switches images), 3 - 4 tasks per workgroup over four layers (both image buffers
reused in both directions), a second task of the same layer, fewer tasks than workgroups (a workgroup returns at once), output bias
present and absent, the same launch twice into the same buffers and again behind a launch of gemv_k256c_kernel.

Bars: the fp64 model of the reference's roundings with _arith_model.check_outputs' own bound (what
tests/test_route_models_k256_gpu.py holds the exact chain rows to); at least 0.95 of a layer's outputs bit-identical to one
launch per layer with VPTQ_GEMV_EXACT (bench.py's bar); W through one-hot activations bit for bit vptq_dequant's over the finite
special-value table (tests/test_weight_bits_gpu.py's check_bits: -0 == +0, fp16 has no excepted class)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _arith_model as am
import _chain_rows_run as run
from oracle import vptq_oracle as vo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WGS = 4


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    path = str(tmp_path_factory.mktemp("rows") / "out.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("VPTQ_") or k == "VPTQ_HIP_LIB"}
    env.update(VPTQ_TUNING="1", VPTQ_K256C_ROWS="1", VPTQ_K256C_WGS=str(WGS))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_chain_rows_run.py"), path], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _cdiv(a, b):
    return -(-a // b)


def _groups(O):
    return _cdiv(_cdiv(O, 8), 8)   # row groups of 8 vector-rows


def _tasks(chain):
    return [_cdiv(_groups(O), 16) for _, O, _ in run.CHAINS[chain]]


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


@pytest.mark.parametrize("chain", sorted(run.CHAINS))
def test_geometry_is_the_one_asked_for(chain, out):
    assert str(out[f"{chain}.instance"]).startswith("gemv_k256c dt=f16 dep=0 mode=exact ") and str(out[f"{chain}.instance"]).endswith(" geom=rows")
    assert "geom=" not in str(out[f"{chain}.folded_instance"]) and "mode=folded" in str(out[f"{chain}.folded_instance"])
    assert str(out["special.instance"]).endswith(" geom=rows")


@pytest.mark.parametrize("chain", sorted(run.CHAINS))
def test_every_output_vs_the_fp64_model(chain, out):
    for i in range(len(run.CHAINS[chain])):
        L = run.layer_of(chain, i)
        m, a = am.model(am.pieces(L), run.x_of(chain, i), "exact")
        y = vo.to_f32(out[f"{chain}.y.{i}"], "f16").astype(np.float64)
        am.check_outputs(y.reshape(1, -1), m, a, "f16", False, what=f"{chain} layer {i} {run.CHAINS[chain][i]}")


@pytest.mark.parametrize("chain", sorted(run.CHAINS))
def test_bit_identical_share_vs_one_launch_per_layer(chain, out):
    for i in range(len(run.CHAINS[chain])):
        got, ref = out[f"{chain}.y.{i}"], out[f"{chain}.single.{i}"]
        assert got.shape == ref.shape
        frac = float((got == ref).mean())
        print(f"{chain} layer {i} {run.CHAINS[chain][i]}: {frac:.4f} bit-identical to the one-layer launch")
        assert frac >= 0.95, (chain, i, frac)


@pytest.mark.parametrize("chain", sorted(run.CHAINS))
def test_relaunches_repeat_the_bits(chain, out):
    for i in range(len(run.CHAINS[chain])):
        assert np.array_equal(out[f"{chain}.y.{i}"], out[f"{chain}.again.{i}"]), f"{chain} layer {i}: the second launch differs"
        assert np.array_equal(out[f"{chain}.y.{i}"], out[f"{chain}.after.{i}"]), f"{chain} layer {i}: differs behind a gemv_k256c launch"


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
