"""Compact mode on the GPU: a large-codebook layer whose exact sliced layout is the only copy of its indices
(`VQuantLinear.compact`, the repack kernel vptq_amd/csrc/repack.hip) computes bit for bit what an uncompacted twin of the same
weights computes over the same kernels, at every token count, and gives back its packed indices bit for bit wherever they are read:
dequant(), state_dict(), copies.  The twin calls enable_sliced_layout(True), so that both take the same kernel at every count."""
import copy

import pytest
import torch

import vptq_amd
from vptq_amd import VQuantLinear, compact_model
from vptq_amd import _backend as B
from vptq_amd.utils.pack import pack_index

pytestmark = pytest.mark.gpu
TOKENS = (1, 2, 3, 4, 5, 8, 16, 17, 64)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    B.lib()
    return torch.device("cuda", 0)


def _as16(t):
    return torch.where(t >= 32768, t - 65536, t).to(torch.int16)


def make_layer(I, O, v, k, kr, dt, seed, dev):
    m = VQuantLinear(I, O, [-1, v], [-1, k], [-1, kr if kr else -1], 1, I, 0, False, enable_norm=True, is_indice_packed=True,
                     enable_proxy_error=False, dtype=dt, device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    ib, rb = k.bit_length() - 1, (kr.bit_length() - 1 if kr else 0)
    with torch.no_grad():
        N = m.indices.shape[1]
        idx = torch.randint(0, k, (1, N, I), generator=g, device=dev)
        ridx = torch.randint(0, kr, (1, N, I), generator=g, device=dev) if kr else None
        m.indices.data = pack_index(_as16(idx), ib, None if ridx is None else _as16(ridx), rb)
        m.centroids.weight.data = (torch.randn(m.centroids.weight.shape, generator=g, device=dev) * 0.02).to(dt)
        if kr:
            m.res_centroids.weight.data = (torch.randn(m.res_centroids.weight.shape, generator=g, device=dev) * 0.005).to(dt)
        m.weight_scale.data = (1 + 0.1 * torch.randn(I, generator=g, device=dev)).to(dt)
        m.weight_bias.data = (0.002 * torch.randn(I, generator=g, device=dev)).to(dt)
    return m.eval()


def twin_of(m):
    t = VQuantLinear(m.in_features, m.out_features, [-1, m.vector_len], [-1, m.num_centroids],
                     [-1, m.num_res_centroids if m.enable_residual else -1], 1, m.group_size, 0, False, enable_norm=True,
                     is_indice_packed=True, enable_proxy_error=False, dtype=m.centroids.weight.dtype, device=m.centroids.weight.device)
    t.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    t.enable_sliced_layout(True)
    return t.eval()


# (I, O, v, k, kr): the published formats, a layer with T = 22 (not a multiple of 4) in two column parts that share words
# (12296 columns per part: 12296 x 22 bits is no whole number of words), a 28672-column layer in two parts
FORMATS = [(4096, 4096, 8, 65536, 0), (4096, 4096, 8, 65536, 256), (4096, 4096, 8, 65536, 65536), (4096, 8192, 16, 65536, 65536),
           (24592, 1024, 8, 16384, 256), (28672, 4096, 8, 65536, 256)]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("I,O,v,k,kr", FORMATS, ids=lambda p: str(p))
def test_compact_layer_bit_identical(I, O, v, k, kr, dt, dev):
    from vptq_amd.utils.sliced import SlicedGemv, exact_column_parts
    m = make_layer(I, O, v, k, kr, dt, seed=I + O + k + kr, dev=dev)
    ref = m.indices.detach().clone()
    parts = exact_column_parts(m._descriptor().desc, I)[0]
    if I in (24592, 28672):
        assert parts == 2
    # the kernel's repack of a fresh exact layout equals the packed indices
    sl = SlicedGemv(m, exact=True)
    assert torch.equal(sl.repack(), ref)
    del sl
    twin = twin_of(m)
    xs = {t: (torch.randn(1, t, I, device=dev) * 0.5).to(dt) for t in TOKENS}
    m.enable_sliced_layout(True)   # (the layout exists before the measurement: compact() reuses it)
    m(xs[1])
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    a0 = torch.cuda.memory_allocated(dev)
    freed = m.compact(force=True)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    a1 = torch.cuda.memory_allocated(dev)
    assert freed == ref.numel() * 4, m.compact_skipped
    assert m.is_compact() and m.indices.is_meta and m.indices.shape == ref.shape and m.indices.dtype == torch.int32
    assert a0 - a1 >= freed, (a0, a1, freed)
    sl = m._sliced_gemv()
    rb = m.resident_bytes()
    assert rb["packed"] == 0 and rb["layout"] == sum(t.numel() * t.element_size() for tup in sl._tensors for t in tup if t is not None)
    for t in TOKENS:
        y, yt = m(xs[t]), twin(xs[t])
        assert torch.equal(y.view(torch.int16), yt.view(torch.int16)), (t, (y.float() - yt.float()).abs().max().item())
    assert torch.equal(m.dequant().view(torch.int16), twin.dequant().view(torch.int16))
    sd = m.state_dict()
    assert torch.equal(sd["indices"], ref) and sd["indices"].device == ref.device
    assert m.is_compact()
    # a copy: uncompacted, with the packed indices
    c = copy.deepcopy(m)
    assert not c.is_compact() and torch.equal(c.indices, ref)
    c.enable_sliced_layout(True)
    assert torch.equal(c(xs[1]).view(torch.int16), twin(xs[1]).view(torch.int16))
    assert torch.equal(c(xs[8]).view(torch.int16), twin(xs[8]).view(torch.int16))
    del c
    # every arithmetic: a compacted layer takes the reference's roundings
    y1 = m(xs[1])
    for mode in ("selective", "folded"):
        vptq_amd.set_arithmetic(mode)
        try:
            assert torch.equal(m(xs[1]).view(torch.int16), y1.view(torch.int16)), mode
        finally:
            vptq_amd.set_arithmetic("reference")
    # moving refuses
    with pytest.raises(RuntimeError, match="uncompact"):
        m.to("cpu")
    assert m.is_compact()
    # different weights loaded into the compacted layer: the new weights' outputs
    other = make_layer(I, O, v, k, kr, dt, seed=I + O + k + kr + 1, dev=dev)
    m.load_state_dict(other.state_dict())
    assert not m.is_compact() and torch.equal(m.indices, other.indices)
    for t in (1, 8):
        assert torch.equal(m(xs[t]).view(torch.int16), other(xs[t]).view(torch.int16)), t


def test_compact_graph_capture_and_uncompact(dev):
    m = make_layer(4096, 4096, 8, 65536, 256, torch.float16, seed=5, dev=dev)
    ref = m.indices.detach().clone()
    assert m.compact() > 0, m.compact_skipped      # (4096 x 4096: served from the exact layout at one token by the product)
    x1 = torch.randn(1, 1, 4096, device=dev).half()
    x8 = torch.randn(1, 8, 4096, device=dev).half()
    y1, y8 = m(x1), m(x8)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            m(x1), m(x8)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        g1, g8 = m(x1), m(x8)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(g1.view(torch.int16), y1.view(torch.int16)) and torch.equal(g8.view(torch.int16), y8.view(torch.int16))
    m.uncompact()
    assert not m.is_compact() and torch.equal(m.indices, ref)
    assert torch.equal(m(x8).view(torch.int16), y8.view(torch.int16))


def test_canonical_and_small_layers_are_skipped(dev):
    can = make_layer(1024, 1024, 8, 256, 256, torch.float16, seed=1, dev=dev)
    ref = can.indices.detach().clone()
    small = make_layer(1024, 512, 8, 65536, 256, torch.float16, seed=2, dev=dev)
    model = torch.nn.Sequential(can, small)
    rep = compact_model(model)
    assert set(rep["skipped"]) == {"0", "1"} and rep["freed"] == 0
    assert "format" in rep["skipped"]["0"] and "force" in rep["skipped"]["1"]
    assert not can.is_compact() and torch.equal(can.indices, ref)
    assert compact_model(model, force=True)["layers"].keys() == {"1"}


def _tiny_llama(dev, dt):
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(hidden_size=1024, intermediate_size=2816, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=4,
                      vocab_size=512, max_position_embeddings=256, tie_word_embeddings=False)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).to(dev, dt)
    seed = 100
    for name, mod in list(model.named_modules()):
        if isinstance(mod, torch.nn.Linear) and name != "lm_head":
            seed += 1
            new = make_layer(mod.in_features, mod.out_features, 8, 65536, 256, dt, seed, dev)
            new.weight_scale.data *= 2.0
            model.set_submodule(name, new)
    return model.eval()


def test_compact_model_greedy_decode(dev):
    model = _tiny_llama(dev, torch.float16)
    qs = [m for m in model.modules() if isinstance(m, VQuantLinear)]
    for m in qs:
        m.enable_sliced_layout(True)
    ids = torch.randint(0, 512, (1, 8), device=dev)
    with torch.no_grad():
        want = model.generate(ids, max_new_tokens=5, do_sample=False)
        rep = compact_model(model, force=True)
        assert len(rep["layers"]) == len(qs) and not rep["skipped"] and rep["after"] < rep["before"]
        assert all(m.is_compact() for m in qs)
        got = model.generate(ids, max_new_tokens=5, do_sample=False)
    assert torch.equal(got, want)


def test_sibling_group_and_chain_with_a_compacted_member(dev):
    """a grouped (non-sliced) sibling launch with a compacted member runs per layer; a chain refuses compacted layers"""
    from vptq_amd.layers import SiblingGroup
    from vptq_amd.ops.chain import GemvChain
    a = make_layer(4096, 4096, 8, 65536, 256, torch.float16, seed=11, dev=dev)
    b = make_layer(4096, 4096, 8, 65536, 256, torch.float16, seed=12, dev=dev)
    ta, tb = twin_of(a), twin_of(b)
    group = SiblingGroup([a, b])
    for m in (a, b):
        object.__setattr__(m, "_siblings", group)
    x4 = torch.randn(1, 4, 4096, device=dev).half()
    ya, yb = a(x4), b(x4)            # (grouped launch, both uncompacted)
    assert a.compact() > 0, a.compact_skipped
    za, zb = a(x4), b(x4)
    assert torch.equal(za.view(torch.int16), ta(x4).view(torch.int16)) and torch.equal(zb.view(torch.int16), yb.view(torch.int16))
    assert torch.equal(zb.view(torch.int16), tb(x4).view(torch.int16))
    x1 = torch.randn(1, 1, 4096, device=dev).half()
    with pytest.raises(ValueError, match="uncompact"):
        GemvChain([a, b])([x1, x1])
    a.uncompact()
    assert torch.equal(a(x4).view(torch.int16), ya.view(torch.int16))
