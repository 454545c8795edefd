"""The one batched-decode path of `VQuantLinear.forward` and of `ops.quant_gemm` (vptq_amd/batched_decode.py): for each of the five
entries, a layer its route takes makes exactly that library call from both callers, with the bits of the public wrapper on the
module's descriptor.  A routing test - it runs no device code of its own; the bits against the fp64 models are held by the five
test_gemm_*_gpu.py files."""
import copy

import pytest
import torch

from test_route_models_gpu import _dense, dev   # noqa: F401  (dev: the module-scoped device fixture)
from test_gemm_gather_gpu import layer as layer_g
from test_gemm_gatherx_gpu import layer as layer_x
from test_gemm_k256w_gpu import layer as layer_k
from test_gemm_gather_px_gpu import _op_keywords
from _gpu_util import spec_to_module, bits_to_tensor, module_desc

pytestmark = pytest.mark.gpu
I, O = 2048, 512
LAUNCHES = ("vptq_quant_gemm_gather_px", "vptq_quant_gemm_gather", "vptq_quant_gemm_gatherx", "vptq_quant_gemm_k256w",
            "vptq_quant_gemm_gatherw", "vptq_quant_gemv", "vptq_dequant")
CASES = {   # entry: (the layer, dtype, tokens)
    "vptq_quant_gemm_gather": (lambda dt: layer_g(I, O, 24, dt, bias=1), "f16", 12),                     # v8-k65536-256
    "vptq_quant_gemm_gatherx": (lambda dt: layer_x(I, O, "v16-k65536-1024", dt, bias=1), "bf16", 5),
    "vptq_quant_gemm_gatherw": (lambda dt: layer_g(I, O, 16, dt, bias=1), "bf16", 24),                   # v8-k65536-0
    "vptq_quant_gemm_k256w": (lambda dt: layer_k(I, O, dt, bias=1), "f16", 33),                          # the canonical format
    "vptq_quant_gemm_gather_px": (lambda dt: layer_g(I, O, 24, dt, perm=1, bias=1), "bf16", 24),         # v8-k65536-256, a random permutation
}


class _Spy:
    """B.lib() with the names of the launching entries called through it recorded"""
    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in LAUNCHES:
            return fn

        def spy(*a):
            self._calls.append(name)
            return fn(*a)
        return spy


def _spied(call, monkeypatch):
    from vptq_amd import _backend as B
    calls, real = [], B.lib()
    monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls))
    try:
        y = call()
    finally:
        monkeypatch.setattr(B, "lib", lambda: real)
    return y, calls


def _bits(y):
    return y.view(torch.int16)


@pytest.mark.parametrize("entry", list(CASES))
def test_module_and_op_make_the_one_call_of_the_route_and_agree_bit_for_bit(entry, dev, monkeypatch):
    import vptq_amd
    from vptq_amd import ops, _backend as B, batched_decode as bd
    make, dt, tokens = CASES[entry]
    route = {r.entry: r for r in bd.BATCHED_DECODE_ROUTES}[entry]
    assert vptq_amd.arithmetic() == "reference"
    monkeypatch.setattr(bd, route.knob, "1")
    L = make(dt)
    assert (L.perm is not None) == (entry == "vptq_quant_gemm_gather_px")
    m = spec_to_module(L, dev)
    xt = bits_to_tensor(_dense(I, tokens, dt, 9 + tokens)[0], dt, dev).reshape(1, tokens, I)
    y, calls = _spied(lambda: m(xt), monkeypatch)
    assert calls == [entry], calls
    yo, calls = _spied(lambda: ops.quant_gemm(xt, **_op_keywords(m)), monkeypatch)
    assert calls == [entry], calls
    assert y.shape == yo.shape == (1, tokens, O) and torch.equal(_bits(y), _bits(yo))
    desc, keep = module_desc(m)
    yw = getattr(ops, "quant_gemm_" + entry[len("vptq_quant_gemm_"):])(xt, desc, O)
    assert torch.equal(_bits(y), _bits(yw))
    # one cached answer per (entry, side of 16 tokens) of this descriptor; one static tuple, which holds the route
    gen, served = m.__dict__["_bd_supported"]
    assert gen == m._descriptor().generation and served == {(entry, tokens > 16): True}
    assert route in m.__dict__["_bd_routes"]
    if route.off_flags == B.GEMV_FORCE_ANY:
        return
    # a copy carries neither: it asks this process's library again, and routes and computes the same
    m2 = copy.deepcopy(m)
    assert "_bd_supported" not in m2.__dict__ and "_bd_routes" not in m2.__dict__ and "_desc_cache" not in m2.__dict__
    y2, calls = _spied(lambda: m2(xt), monkeypatch)
    assert calls == [entry], calls
    assert torch.equal(_bits(y), _bits(y2))
    assert m2.__dict__["_bd_supported"][1] == {(entry, tokens > 16): True} and route in m2.__dict__["_bd_routes"]
