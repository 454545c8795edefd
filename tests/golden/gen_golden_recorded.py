#!/usr/bin/env python3
"""Record what the reference-comparison tests check against (run where the reference tree is).

    python tests/golden/gen_golden_recorded.py     # writes tests/golden/recorded/*

The tests of tests/test_oracle_golden.py, tests/test_host_cpu.py and tests/test_pack_model_cpu.py
that compare this package with microsoft/VPTQ itself read these files, so that they run on every
checkout.  Imports the reference read-only (two shims, see _refshim.py) and records

* ``oracle_r1..r3.npz``: three seeded random layers built as reference ``VQuantLinear`` modules
  (gen_golden.build): every parameter, the reference's dense W (all of it) and its forward output;
* ``v2_<dtype>.npz``: the reference test file's ``create_test_data`` inputs (index tensors
  included) and its ``ground_truth`` output for two small configurations;
* ``reference_test_file.json``: the keyword names ``create_test_data`` returns (what that test file
  passes to ``vptq.ops.quant_gemv_v2``) and the number of its test configurations;
* ``reference_modules.json``: the state-dict keys, shapes, dtypes and derived attributes of a
  reference ``VQuantLinear`` for every configuration of gen_golden.CASES;
* ``pack_model.npz``: the reference's ``convert_idx_dtype`` (``pack_model`` without the HF config
  fix-up) applied to tests/test_pack_model_cpu.py's stand-in model: packed tensors + layer configs;
* ``reference_cli_flags.json``: the long options of the reference's ``python -m vptq`` parser.
"""
import json
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (HERE, TESTS, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
from _refshim import load_reference, REFERENCE_PATH  # noqa: E402
import gen_golden as gg  # noqa: E402

OUT = os.path.join(HERE, "recorded")

# (name, I, O, ctor kwargs, dtype, tokens, dist) - seed 99 + position
RANDOM_LAYERS = [
    ("r1", 640, 136, dict(vector_lens=[-1, 8], num_centroids=[-1, 256], num_res_centroids=[-1, 256], group_num=1, outlier_size=0, enable_norm=True, enable_perm=True, bias=True), "f16", 2, "ref-test"),
    ("r2", 8 + 3 * 64, 70, dict(vector_lens=[2, 10], num_centroids=[16, 512], num_res_centroids=[-1, 64], group_num=3, outlier_size=8, enable_norm=True, enable_perm=False, bias=False), "bf16", 1, "llm"),
    ("r3", 192, 66, dict(vector_lens=[-1, 2], num_centroids=[-1, 16], num_res_centroids=[-1, -1], group_num=1, outlier_size=0, enable_norm=False, enable_perm=True, bias=False), "f16", 4, "ref-test"),
]

# (dtype, k, k_res, I, O, tokens)
V2_LIVE = [("bf16", 512, 256, 128, 64, 1), ("f16", 1024, 512, 256, 32, 3)]


def _cfg_bytes(cfg):
    return np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8)


def random_layers(vptq):
    for ci, (name, I, O, kw, dtype, tokens, dist) in enumerate(RANDOM_LAYERS):
        m, x, proc = gg.build(vptq, name, I, O, kw, dtype, tokens, dist, seed=99 + ci)
        assert not proc
        with torch.no_grad():
            W = gg.ref_dequant(vptq, m)
            y = m(x)
        cfg = dict(name=name, in_features=I, out_features=O, dtype=dtype, tokens=tokens, dist=dist,
                   vector_len=m.vector_len, num_centroids=m.num_centroids, num_res_centroids=m.num_res_centroids,
                   num_codebooks=m.num_codebooks, group_size=m.group_size, outlier_size=m.outlier_size,
                   outlier_vector_len=m.outlier_vector_len, num_outlier_centroids=m.num_outlier_centroids,
                   enable_norm=m.enable_norm, enable_perm=m.enable_perm, has_bias=m.bias is not None,
                   ctor=kw, proc={}, torch=torch.__version__)
        Wb = gg.bits(W)
        arrs = dict(config=_cfg_bytes(cfg), indices=gg.bits(m.indices), x=gg.bits(x), y=gg.bits(y), W=Wb,
                    W_head=Wb[:16].copy(), centroids=gg.bits(m.centroids.weight))
        if m.enable_residual:
            arrs["res_centroids"] = gg.bits(m.res_centroids.weight)
        if m.enable_outlier:
            arrs["outlier_indices"] = gg.bits(m.outlier_indices)
            arrs["outlier_centroids"] = gg.bits(m.outlier_centroids.weight)
        if m.enable_perm:
            arrs["perm"] = gg.bits(m.perm)
        if m.enable_norm:
            arrs["weight_scale"] = gg.bits(m.weight_scale)
            arrs["weight_bias"] = gg.bits(m.weight_bias)
        if m.bias is not None:
            arrs["bias"] = gg.bits(m.bias)
        np.savez_compressed(os.path.join(OUT, f"oracle_{name}.npz"), **arrs)


def v2_live():
    import gen_golden_v2 as g2
    rt = g2.load_reference_test_module()
    for dtype, k, kr, I, O, T in V2_LIVE:
        cfg = dict(in_features=I, out_features=O, num_centroids=k, num_res_centroids=kr, length=T,
                   vector_length=8, device=torch.device("cpu"), dtype=gg.TORCH_DT[dtype])
        d = rt.create_test_data(cfg)
        y = rt.ground_truth(x=d["x"], bias=None, indices=d["indices"], centroids=d["centroids"],
                            res_indices=d["residual_indices"], res_centroids=d["residual_centroids"],
                            scale_weights=d["scale_weights"], scale_bias=d["scale_bias"],
                            vector_len=8, out_features=O)
        meta = dict(dtype=dtype, num_centroids=k, num_res_centroids=kr, in_features=I, out_features=O, length=T,
                    vector_len=8, torch=torch.__version__)
        np.savez_compressed(os.path.join(OUT, f"v2_{dtype}.npz"), config=_cfg_bytes(meta), x=gg.bits(d["x"]),
                            indices=d["indices"].numpy().astype(np.int64), centroids=gg.bits(d["centroids"]),
                            res_indices=d["residual_indices"].numpy().astype(np.int64),
                            res_centroids=gg.bits(d["residual_centroids"]), scale_weights=gg.bits(d["scale_weights"]),
                            scale_bias=gg.bits(d["scale_bias"]), y=gg.bits(y))
    # the keyword set the reference test passes to vptq.ops.quant_gemv_v2(**test_data)
    d = rt.create_test_data(dict(in_features=64, out_features=64, num_centroids=64, num_res_centroids=16,
                                 device=torch.device("cpu")))
    rec = dict(create_test_data_keys=list(d), test_configs=len(rt.test_configs),
               has_test_quant_gemv=callable(getattr(rt, "test_quant_gemv", None)))
    with open(os.path.join(OUT, "reference_test_file.json"), "w") as f:
        json.dump(rec, f, indent=1)


def reference_modules(ref):
    rec = {}
    for name, I, O, kw, dtype, tokens, dist in gg.CASES:
        C, S = kw["group_num"], kw["outlier_size"]
        common = dict(group_size=(I - S) // C, indices_as_float=False, is_indice_packed=True,
                      dtype=gg.TORCH_DT[dtype], enable_proxy_error=False, **kw)
        rm = ref.VQuantLinear(I, O, **common)
        sd = rm.state_dict()
        rec[name] = dict(state_dict=[[k, list(t.shape), str(t.dtype)] for k, t in sd.items()],
                         attrs={a: getattr(rm, a) for a in ("padding", "num_indices", "outlier_padding", "vector_len",
                                                            "num_codebooks", "num_centroids", "num_res_centroids",
                                                            "enable_outlier", "enable_residual")})
    with open(os.path.join(OUT, "reference_modules.json"), "w") as f:
        json.dump(rec, f, indent=1)


def pack_model():
    """tests/test_pack_model_cpu.py's unpacked checkpoint through the reference's convert_idx_dtype, on a stand-in
    model whose layers carry the reference's attribute names (it finds them by type name)."""
    import test_pack_model_cpu as tp
    from vptq.utils.pack import convert_idx_dtype

    class VQuantLinear(torch.nn.Module):
        pass

    class Model(torch.nn.Module):
        class config:                          # noqa: N801 - stands in for a HF config
            pass

    state, conf = tp._state_and_config()
    model = Model()
    mods = {}
    for name, (C, N, G, k, kr, as_f, perm, outl) in tp.LAYERS.items():
        m = VQuantLinear()
        for key in ("indices", "res_indices", "outlier_indices", "perm"):
            t = state.get(f"{name}.{key}")
            setattr(m, key, None if t is None else torch.nn.Parameter(t.clone(), requires_grad=False))
        if m.perm is None:                      # the reference converts perm unconditionally
            m.perm = torch.nn.Parameter(torch.arange(C * G), requires_grad=False)
        m.num_centroids, m.num_res_centroids = k, (kr if kr else -1)
        m.init_args = dict(conf[name])
        mods[name] = m
    for name, m in mods.items():                # nest the modules under their dotted names
        parent = model
        parts = name.split(".")
        for p in parts[:-1]:
            if not hasattr(parent, p):
                parent.add_module(p, torch.nn.Module())
            parent = getattr(parent, p)
        parent.add_module(parts[-1], m)
    packed = convert_idx_dtype(model, torch.uint16, torch.uint16, torch.int16)
    arrs, res_none = {}, {}
    for name, m in mods.items():
        for key in ("indices", "perm", "outlier_indices"):
            t = getattr(m, key)
            if t is not None:
                arrs[f"{name}.{key}"] = t.data.numpy()
        res_none[name] = m.res_indices is None
    meta = dict(config_for_layers=Model.config.quantization_config["config_for_layers"], res_indices_is_none=res_none,
                returns_the_model=packed is model)
    np.savez_compressed(os.path.join(OUT, "pack_model.npz"), config=_cfg_bytes(meta), **arrs)


def cli_flags():
    src = open(os.path.join(REFERENCE_PATH, "vptq", "app_utils.py")).read()
    with open(os.path.join(OUT, "reference_cli_flags.json"), "w") as f:
        json.dump(sorted(set(re.findall(r'"(--[a-z-]+)"', src))), f, indent=1)


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(1)
    vptq = load_reference()
    random_layers(vptq)
    reference_modules(vptq)
    v2_live()
    pack_model()
    cli_flags()
    for f in sorted(os.listdir(OUT)):
        print(f"{f}: {os.path.getsize(os.path.join(OUT, f)) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
