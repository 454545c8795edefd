"""Pin the oracle against the real reference (golden vectors and recorded results of the reference)."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import vptq_oracle as vo
from _cases import (golden_names, load_golden, rel_err, bit_identical_frac, big_names, load_big, fmt_names, load_fmt, stored_rows,
                    v2_names, load_v2, RECORDED_DIR)

# fp16: 1 ulp ~ 4.9e-4 relative; bf16: 3.9e-3.  The reference's F.linear and the
# oracle's float64 dot differ only by summation order -> <= ~1 output ulp.
Y_TOL = {"f16": 1e-3, "bf16": 8e-3}


@pytest.mark.parametrize("name", golden_names())
def test_oracle_dequant_bit_exact_vs_reference(name):
    L, x, y, cfg, W_head = load_golden(name)
    W = vo.dequant(L)
    assert W.shape == (cfg["out_features"], cfg["in_features"])
    assert (W[:16] == W_head).all()
    assert hashlib.sha256(W.tobytes()).hexdigest() == cfg["W_sha256"]


@pytest.mark.parametrize("name", golden_names())
def test_oracle_forward_vs_reference(name):
    L, x, y, cfg, _ = load_golden(name)
    out = vo.forward(L, x)
    assert out.shape == y.shape
    assert rel_err(out, y, cfg["dtype"]) <= Y_TOL[cfg["dtype"]]
    # near bit-identity: only summation-order noise remains
    assert bit_identical_frac(out, y) >= 0.90


def test_pack_unpack_roundtrip_and_edges():
    rng = np.random.default_rng(7)
    for ib, rb, G in [(8, 8, 64), (12, 0, 7), (13, 8, 33), (16, 8, 5), (16, 16, 3),
                      (4, 2, 1), (10, 4, 96), (15, 12, 17), (1, 0, 40)]:
        idx = rng.integers(0, 1 << ib, size=(2, 3, G))
        r = rng.integers(0, 1 << rb, size=(2, 3, G)) if rb else None
        p = vo.pack_indices(idx, ib, r, rb)
        assert p.dtype == np.int32 and p.shape == (2, 3, (G * (ib + rb) + 31) // 32)
        a, b = vo.unpack_indices(p, ib, G, rb, ref_residual_mask_quirk=False)
        assert (a == idx).all()
        if rb:
            assert (b == r).all()
    # all-ones / zero patterns and the max index survive
    for val in (0, (1 << 16) - 1):
        idx = np.full((1, 1, 9), val)
        p = vo.pack_indices(idx, 16, idx, 16)
        a, b = vo.unpack_indices(p, 16, 9, 16)
        assert (a == val).all() and (b == val).all()


def test_residual_mask_quirk_documented():
    """pack.py:137 masks the residual with index_bits; differs only if rb>ib."""
    idx = np.array([[[3, 1]]]); r = np.array([[[200, 77]]])
    p = vo.pack_indices(idx, 2, r, 8)
    _, rq = vo.unpack_indices(p, 2, 2, 8, ref_residual_mask_quirk=True)
    _, rc = vo.unpack_indices(p, 2, 2, 8, ref_residual_mask_quirk=False)
    assert (rc == r).all() and (rq == (r & 3)).all()


def test_oracle_vs_live_reference_random_layers():
    """Three seeded random layers built as the reference's own VQuantLinear (outliers, three codebooks, perm, bias,
    bf16, vector lengths 2 / 8 / 10): the numpy oracle rebuilds the reference's whole dense W bit for bit and its
    forward output (tests/golden/recorded/oracle_r*.npz, written by tests/golden/gen_golden_recorded.py)."""
    for name in ("r1", "r2", "r3"):
        L, x, y, cfg, _ = load_golden("oracle_" + name, RECORDED_DIR)
        W = np.load(os.path.join(RECORDED_DIR, f"oracle_{name}.npz"))["W"]
        assert (vo.dequant(L) == W).all(), name
        out = vo.forward(L, x)
        assert rel_err(out, y, cfg["dtype"]) <= Y_TOL[cfg["dtype"]], name


# ---------------------------------------------------------------- BASELINE sizes
@pytest.mark.parametrize("name", big_names())
def test_c_oracle_vs_reference_at_baseline_sizes(name):
    """hidden 4096 / 8192 (BASELINE configs[0], [1]): the reference's own dense W (sha256) and
    forward output, every input procedural (tests/golden/gen_golden_big.py)."""
    from oracle import c_oracle as co
    if not co.available():
        pytest.skip("run __graft_entry__.build() first")
    L, x, y, cfg, W_head = load_big(name)
    W = co.dequant(L)
    assert (W[:2] == W_head).all()
    assert hashlib.sha256(W.tobytes()).hexdigest() == cfg["W_sha256"]
    # (thousands of tokens: only the token rows the fixture stores go through the oracle - rows are independent)
    out = co.forward(L, np.ascontiguousarray(x[:, cfg["y_rows"]])) if cfg["tokens"] > 1024 else stored_rows(co.forward(L, x), cfg)
    assert rel_err(out, y, cfg["dtype"]) <= Y_TOL[cfg["dtype"]]
    assert bit_identical_frac(out, y) >= 0.98


@pytest.mark.parametrize("name", [n for n in big_names() if n.startswith("h4096")])
def test_numpy_oracle_vs_reference_at_hidden_4096(name):
    L, x, y, cfg, W_head = load_big(name)
    W = vo.dequant(L)
    assert hashlib.sha256(W.tobytes()).hexdigest() == cfg["W_sha256"]
    out = vo.forward(L, np.ascontiguousarray(x[:, cfg["y_rows"]])) if cfg["tokens"] > 1024 else stored_rows(vo.forward(L, x), cfg)
    assert rel_err(out, y, cfg["dtype"]) <= Y_TOL[cfg["dtype"]]
    assert bit_identical_frac(out, y) >= 0.98


@pytest.mark.parametrize("name", fmt_names())
def test_oracles_vs_reference_other_formats(name):
    """The non-canonical formats at the sizes / token counts where their own kernels run (tall layers of the
    LDS-resident formats, 5-8 tokens of the k = 65536 formats, vector lengths 2 / 4 / 6 / 10): the reference's
    dense W (sha256) and forward output, every input procedural (tests/golden/gen_golden_fmt.py); numpy and C."""
    from oracle import c_oracle as co
    L, x, y, cfg, W_head = load_fmt(name)
    dt = cfg["dtype"]
    W = vo.dequant(L)
    assert (W[:2] == W_head).all()
    assert hashlib.sha256(W.tobytes()).hexdigest() == cfg["W_sha256"]
    out = vo.gemv(W, x, dt, L.bias)
    assert rel_err(out, y, dt) <= Y_TOL[dt]
    assert bit_identical_frac(out, y) >= 0.98
    if co.available():
        Wc = co.dequant(L)
        assert hashlib.sha256(Wc.tobytes()).hexdigest() == cfg["W_sha256"]
        outc = co.forward(L, x)
        assert rel_err(outc, y, dt) <= Y_TOL[dt] and bit_identical_frac(outc, y) >= 0.98


# ---------------------------------------------------------------- v2 wire format
def _v2_oracle(d):
    c = d["cfg"]
    return vo.gemv_v2_ground_truth(
        d["x"], d["bias"], d["indices"].astype(np.int64), d["centroids"],
        d["res_indices"].astype(np.int64), d["res_centroids"], d["scale_weights"], d["scale_bias"],
        c["vector_len"], c["out_features"], c["dtype"])


@pytest.mark.parametrize("name", v2_names())
def test_v2_oracle_vs_reference_ground_truth_fixture(name):
    """`gemv_v2_ground_truth` against the output of the reference test file's `ground_truth`
    (tests/test_quant_gemv.py:49-109) on that file's own data recipe - the pin of the v2 oracle."""
    d = load_v2(name)
    dt = d["cfg"]["dtype"]
    out = _v2_oracle(d).reshape(d["y"].shape)
    assert rel_err(out, d["y"], dt) <= Y_TOL[dt]
    assert bit_identical_frac(out, d["y"]) >= 0.98


def test_v2_oracle_vs_live_reference_ground_truth():
    """`gemv_v2_ground_truth` bit for bit against the reference test file's `ground_truth` on two small inputs of
    its `create_test_data` (bf16 and fp16, 1 and 3 tokens; tests/golden/recorded/v2_*.npz)."""
    for dtype in ("bf16", "f16"):
        z = np.load(os.path.join(RECORDED_DIR, f"v2_{dtype}.npz"))
        c = json.loads(bytes(z["config"]).decode())
        out = vo.gemv_v2_ground_truth(
            z["x"], None, z["indices"], z["centroids"], z["res_indices"], z["res_centroids"],
            z["scale_weights"], z["scale_bias"], 8, c["out_features"], dtype)
        assert (out.reshape(-1) == z["y"].reshape(-1)).all(), (dtype, c["num_centroids"], c["num_res_centroids"])


def test_reference_test_file_binds_to_this_package():
    """The reference's kernel test (tests/test_quant_gemv.py) passes the dict of its `create_test_data` to
    `vptq.ops.quant_gemv_v2(**test_data)` (:236): with `vptq` resolving to this repo's alias package, that keyword
    set (recorded in tests/golden/recorded/reference_test_file.json) binds to our signature.  (The GPU test
    `test_quant_gemv_v2_reference_fixture` replays its data and its comparison.)"""
    import inspect
    import sys
    rec = json.load(open(os.path.join(RECORDED_DIR, "reference_test_file.json")))
    assert rec["test_configs"] and rec["has_test_quant_gemv"]
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "vptq" or k.startswith("vptq.")}
    try:
        import vptq  # the alias at the repo root
        assert "vptq_amd" in vptq.VQuantLinear.__module__
        inspect.signature(vptq.ops.quant_gemv_v2).bind(**{k: None for k in rec["create_test_data_keys"]})   # TypeError on a mismatch
    finally:
        for k in [k for k in sys.modules if k == "vptq" or k.startswith("vptq.")]:
            del sys.modules[k]
        sys.modules.update(saved)


# ---------------------------------------------------------------- torch restatement (bench.py's cpu_baseline)
@pytest.mark.parametrize("name", ["canon_k256x2", "canon_llm", "canon_bf16", "canon_t4_bias", "k8192_r256_t21",
                                  "k65536_nores_nonorm"])
def test_torch_restatement_vs_reference_golden(name):
    """oracle/torch_ref.py - the same tensor-op sequence as the reference's CPU path, what
    bench.py times as `cpu_baseline` - reproduces the real reference's W bit for bit and its y."""
    import torch
    from oracle import torch_ref as tr
    L, x, y, cfg, W_head = load_golden(name)
    dt = torch.float16 if cfg["dtype"] == "f16" else torch.bfloat16
    t16 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).view(dt)  # noqa: E731
    kw = dict(num_centroids=L.num_centroids, num_res_centroids=max(L.num_res_centroids, 0), vector_len=L.vector_len,
              group_size=L.group_size, out_features=L.out_features)
    args = (torch.from_numpy(L.indices.copy()), t16(L.centroids),
            t16(L.res_centroids) if L.num_res_centroids > 0 else None,
            t16(L.weight_scale) if L.weight_scale is not None else None,
            t16(L.weight_bias) if L.weight_bias is not None else None)
    W = tr.dequant(*args, **kw)
    Wb = W.contiguous().view(torch.int16).numpy().view(np.uint16)
    assert hashlib.sha256(Wb.tobytes()).hexdigest() == cfg["W_sha256"]
    out = tr.forward(t16(x).reshape(x.shape), *args, bias=t16(L.bias) if L.bias is not None else None, **kw)
    ob = out.contiguous().view(torch.int16).numpy().view(np.uint16)
    assert rel_err(ob, y, cfg["dtype"]) <= Y_TOL[cfg["dtype"]]
    assert bit_identical_frac(ob, y) >= 0.9
