"""vptq_dequant_sliced on the GPU (vptq_amd/csrc/dequant_sliced.hip): the dense W built straight from a layer's exact sliced layouts
is, bit for bit, what vptq_dequant writes for the packed indices the layouts were built from - at the smallest shapes at which
each mechanism of the kernel exists (they live in the columns, so rows are few) - and the dense route and dequant() of a compacted layer of up to 4096 x 4096
take it: no repack, no scratch buffer, the same bits as an uncompacted twin, also when replayed from a graph."""
import pytest
import torch

from vptq_amd import _backend as B
from vptq_amd.utils.sliced import SlicedGemv, exact_column_parts

from test_compact_gpu import make_layer, twin_of

pytestmark = pytest.mark.gpu
F16, BF16 = torch.float16, torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    B.lib()
    return torch.device("cuda", 0)


def _bits(t):
    return t.view(torch.int16)


def _perm_layer(I, O, v, k, kr, dt, seed, dev):
    """`make_layer` with enable_perm=True and a random permutation"""
    from vptq_amd import VQuantLinear
    src = make_layer(I, O, v, k, kr, dt, seed, dev)
    m = VQuantLinear(I, O, [-1, v], [-1, k], [-1, kr if kr else -1], 1, I, 0, False, enable_norm=True, enable_perm=True,
                     is_indice_packed=True, enable_proxy_error=False, dtype=dt, device=dev)
    sd = {n: t.clone() for n, t in src.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 7)
    sd["perm"] = torch.randperm(I, generator=g).to(torch.int32).to(torch.int16).to(dev)
    m.load_state_dict(sd)
    return m.eval()


# (I, O, v, k, kr, what it exercises)
ROWS_1024 = [
    (1024, 264, 8, 65536, 0, "8 slices, one tile, no side stream"),
    (1024, 264, 8, 65536, 256, "8 slices, one tile, uint8 side stream, table in LDS"),
    (1024, 264, 8, 65536, 65536, "8 slices, one tile, uint16 side stream, table gathered"),
    (1024, 264, 16, 65536, 0, "v = 16, no side stream; 264 rows: the last vector-row is padded"),
    (1024, 264, 16, 65536, 65536, "v = 16, uint16 side stream"),
]
ROWS_WIDE = [
    (5384, 64, 8, 65536, 256, "16 slices"),
    (8200, 32, 16, 65536, 0, "three tiles per row (v = 16: at most 4096 columns per tile), lists walked by window"),
    (4104, 64, 8, 32768, 0, "width not a multiple of 64: list padding"),
]
ROWS_TWO_PARTS = [
    (24592, 64, 8, 16384, 256, "two column parts that share words of the packed row, T = 22, four tiles"),
    (28672, 64, 8, 65536, 256, "two parts of 14336 columns, four tiles"),
]
CASES = [(r, F16) for r in ROWS_1024 + ROWS_WIDE + ROWS_TWO_PARTS] + [(r, BF16) for r in ROWS_1024 + ROWS_TWO_PARTS]


@pytest.mark.parametrize("row,dt", CASES, ids=lambda p: f"{p[0]}x{p[1]}-v{p[2]}-k{p[3]}-{p[4]}" if isinstance(p, tuple) else str(p).split(".")[-1])
def test_bit_identical_to_vptq_dequant(row, dt, dev):
    I, O, v, k, kr, _ = row
    m = make_layer(I, O, v, k, kr, dt, seed=I + O + v + k + kr, dev=dev)
    want = m.dequant()                       # vptq_dequant over the packed indices
    sl = SlicedGemv(m, exact=True)           # (a layer the library has no exact layout for raises here: a failure, not a skip)
    if I in (24592, 28672):
        assert exact_column_parts(m._descriptor().desc, I)[0] == 2 == sl.parts
    got = sl.dequant()
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == want.dtype
    assert torch.equal(_bits(got), _bits(want)), (got.float() - want.float()).abs().max().item()


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_rows_past_out_features_are_not_stored(dt, dev):
    """136 rows of v = 16: the ninth vector-row holds 8 real rows; W has guard rows behind it"""
    I, O = 1024, 136
    m = make_layer(I, O, 16, 65536, 65536, dt, seed=136, dev=dev)
    want = m.dequant()
    sl = SlicedGemv(m, exact=True)
    buf = torch.full((O + 16, I), 0x5a5a, dtype=torch.int16, device=dev).view(dt)
    sl.dequant(out=buf[:O])
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf[:O]), _bits(want))
    assert bool((_bits(buf[O:]) == 0x5a5a).all())


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("v,k,kr", [(8, 65536, 0), (8, 65536, 256), (16, 65536, 65536)], ids=lambda p: str(p))
def test_special_values_against_the_oracle(v, k, kr, dt, dev):
    """the kernel has its own arithmetic (and otherwise inherits its reference from vptq_dequant): the hand-written tables of
    tests/_dequant_specials.py - signed zeros, subnormals, infinities, NaN, ties, overflow, underflow - against the oracle itself,
    which tests/test_dequant_specials_cpu.py pins to torch's CPU arithmetic.  NaN by position, everything else by bits."""
    import numpy as np
    from oracle import vptq_oracle as vo
    from _gpu_util import spec_to_module, tensor_to_bits
    import _dequant_specials as sp
    L = sp.special_layer(dt, v, k, kr)
    with np.errstate(all="ignore"):
        want = vo.dequant(L, ref_residual_mask_quirk=False)
    got = SlicedGemv(spec_to_module(L, dev), exact=True).dequant()
    torch.cuda.synchronize()
    sp.same_bits(tensor_to_bits(got), want, dt, f"vptq_dequant_sliced v{v}-k{k}-{kr} {dt}")


@pytest.mark.parametrize("I,O", [(1024, 264), (5384, 64)])
def test_with_a_permutation(I, O, dev):
    m = _perm_layer(I, O, 8, 65536, 256, F16, seed=I + O, dev=dev)
    assert m.enable_perm and not torch.equal(m.perm.cpu().long() & 0xffff, torch.arange(I))
    want = m.dequant()
    got = SlicedGemv(m, exact=True).dequant()
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("I,O,v,k,kr", [(1024, 264, 8, 65536, 256), (8200, 32, 16, 65536, 0), (28672, 64, 8, 65536, 256)])
def test_relaunch_into_a_dirty_buffer(I, O, v, k, kr, dev):
    """no tile depends on what W or the LDS held before"""
    m = make_layer(I, O, v, k, kr, F16, seed=3 + I, dev=dev)
    want = m.dequant()
    sl = SlicedGemv(m, exact=True)
    W = torch.full((O, I), 0x3c01, dtype=torch.int16, device=dev).view(F16)
    first = sl.dequant(out=W).clone()
    second = sl.dequant(out=W)
    assert torch.equal(_bits(first), _bits(want)) and torch.equal(_bits(second), _bits(want))


class _Count:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


# (the module takes the new kernel for layers of up to 4096 x 4096 - vptq_amd/sliced_routes.py:dense_from_layout, by measurement;
# 4096 x 8192 v16-k65536-65536 keeps the repack route, so the bf16 two-plane case runs at 4096 x 4096)
@pytest.mark.parametrize("I,O,v,k,kr,dt", [(4096, 4096, 8, 65536, 256, F16), (4096, 4096, 16, 65536, 65536, BF16)],
                         ids=["4096x4096-v8-k65536-256-f16", "4096x4096-v16-k65536-65536-bf16"])
def test_compact_layer_dense_route_without_repack(I, O, v, k, kr, dt, dev, monkeypatch):
    m = make_layer(I, O, v, k, kr, dt, seed=I + O + kr, dev=dev)
    twin = twin_of(m)
    xs = {t: (torch.randn(1, t, I, device=dev) * 0.5).to(dt) for t in (8, 17, 64)}
    want = {t: twin(xs[t]) for t in xs}
    want_w = twin.dequant()
    assert m.compact(force=True) > 0, m.compact_skipped
    scratch = _Count(B.compact_scratch)
    repack = _Count(B.lib().vptq_sliced_layout_repack)
    monkeypatch.setattr(B, "compact_scratch", scratch)
    monkeypatch.setattr(B.lib(), "vptq_sliced_layout_repack", repack)
    before = B.compact_scratch_bytes(dev.index)
    assert torch.equal(_bits(m.dequant()), _bits(want_w))
    for t in (17, 64):
        assert torch.equal(_bits(m(xs[t])), _bits(want[t])), t
    torch.cuda.synchronize()
    assert scratch.calls == 0 and repack.calls == 0
    assert B.compact_scratch_bytes(dev.index) == before
    # 8 tokens: still the gather kernel over a repack, still the twin's bits
    y8 = m(xs[8])
    assert repack.calls >= 1
    assert torch.equal(_bits(y8), _bits(want[8]))


def test_larger_compact_layers_keep_the_repack_route(dev, monkeypatch):
    """the routing rule: a layer wider than 4096 columns still takes repack + vptq_dequant on its dense route - the twin's bits"""
    m = make_layer(8192, 64, 8, 65536, 256, F16, seed=77, dev=dev)
    twin = twin_of(m)
    x = (torch.randn(1, 17, 8192, device=dev) * 0.5).half()
    want = twin(x)
    assert m.compact(force=True) > 0, m.compact_skipped
    repack = _Count(B.lib().vptq_sliced_layout_repack)
    monkeypatch.setattr(B.lib(), "vptq_sliced_layout_repack", repack)
    assert torch.equal(_bits(m(x)), _bits(want))
    assert repack.calls >= 1


def test_compact_dense_route_graph_capture(dev):
    m = make_layer(4096, 4096, 8, 65536, 256, F16, seed=5, dev=dev)
    assert m.compact() > 0, m.compact_skipped
    x = torch.randn(1, 17, 4096, device=dev).half()
    y = m(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            m(x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        gy = m(x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(gy), _bits(y))
