"""The special-value layers (tests/_dequant_specials.py) without a GPU: what the oracle makes of them is what torch's own CPU
arithmetic makes of them - through the restatement of the reference's tensor ops in oracle/torch_ref.py - NaN by position, every
other element bit for bit.  The GPU rows then hold the kernels to the reference's semantics, not to the oracle's opinion of them.
The C oracle agrees on the same layers, and the tables still reach every class they were written for."""
import numpy as np
import pytest
import torch

from oracle import vptq_oracle as vo
from oracle import c_oracle, torch_ref
import _dequant_specials as sp

# (numpy reports the overflows and invalid operations the tables are there to provoke)
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")
TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16}
# (v, k, kr): the layers of test_dequant_models_gpu.py (TAB 1, 2, 0) and of test_dequant_sliced_gpu.py
LAYERS = [(8, 16, 16), (8, 65536, 16), (8, 65536, 2048), (8, 65536, 0), (8, 65536, 256), (16, 65536, 65536)]


def _t(bits, dt):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(TORCH_DT[dt])


def torch_dequant(L):
    dt = L.dtype
    W = torch_ref.dequant(torch.from_numpy(np.ascontiguousarray(L.indices).view(np.int32).copy()), _t(L.centroids, dt),
                          _t(L.res_centroids, dt) if L.num_res_centroids > 0 else None, _t(L.weight_scale, dt), _t(L.weight_bias, dt),
                          num_centroids=L.num_centroids, num_res_centroids=L.num_res_centroids, vector_len=L.vector_len,
                          group_size=L.group_size, out_features=L.out_features)
    return W.contiguous().view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("v,k,kr", LAYERS, ids=lambda p: str(p))
def test_oracle_is_torch_cpu_arithmetic_on_the_special_values(v, k, kr, dt):
    L = sp.special_layer(dt, v, k, kr)
    want = torch_dequant(L)
    sp.same_bits(vo.dequant(L, ref_residual_mask_quirk=False), want, dt, "oracle against torch")
    # (res_bits <= index_bits in every layer: the reference's residual mask is the same)
    sp.same_bits(vo.dequant(L, ref_residual_mask_quirk=True), want, dt, "oracle (reference's mask) against torch")
    if c_oracle.available():
        sp.same_bits(c_oracle.dequant(L, quirk=False), want, dt, "C oracle against torch")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_the_table_reaches_its_classes(dt):
    """every (centroid, residual) pair meets every (scale, bias) pair, and W holds NaNs, infinities from overflow, both zeros and
    subnormals - counted on the oracle's result"""
    L = sp.special_layer(dt)
    idx, ridx = vo.unpack_indices(L.indices, L.index_bits, L.group_size, L.res_bits, False)
    sb = np.arange(L.in_features) // sp.COLS_PER_SB
    seen = {(int(c), int(r), int(p)) for n in range(sp.ROWS) for c, r, p in zip(idx[0, n], ridx[0, n], sb)}
    assert len(seen) == 16 * 16 * 64
    cov = sp.coverage(L)
    assert all(cov[key] > 0 for key in ("nan", "inf", "pos_zero", "neg_zero", "subnormal", "finite")), cov
    cent, res, scale, bias = sp.tables(dt)
    f = sp.FMT[dt]
    r16 = lambda x: float(vo.round_to(np.array([x], np.float32), dt)[0])   # noqa: E731
    # the ties the table was written for are ties: the exact sum lies halfway between two neighbours, and both parities occur
    one, nxt = 1.0, 1.0 + f["eps"]
    assert r16(one + f["eps"] / 2) == one and r16(nxt + f["eps"] / 2) == nxt + f["eps"]
    assert r16(one + 3 * f["eps"] / 2) == nxt + f["eps"] and r16(nxt + 3 * f["eps"] / 2) == nxt + f["eps"]
    assert r16(f["big"] + f["half_ulp_big"]) == float("inf") and r16(f["big"] + f["half_ulp_big"] / 2) == f["big"]
    assert r16(3 * f["sub"] * 0.5) == 2 * f["sub"] and r16(f["sub"] * 0.5) == 0.0 and r16(f["root"] * f["root"]) == float("inf")
    assert r16(nxt * 1.5) == 1.5 + 2 * f["eps"]
    for need, have in ((one, cent), (nxt, cent), (f["eps"] / 2, res[0]), (3 * f["eps"] / 2, res[0]), (f["half_ulp_big"], res[0]),
                       (3 * f["sub"], cent), (f["sub"], cent), (f["root"], cent), (0.5, scale), (1.5, scale), (f["root"], scale),
                       (f["eps"] / 2, bias)):
        assert need in have
