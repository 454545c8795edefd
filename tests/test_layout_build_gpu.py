"""The device-side layout builder on the GPU (vptq_sliced_layout_plan / _fill, vptq_amd/csrc/layout_build.hip; `sliced.layout_on_device`):
byte for byte what the torch recipe `layout_from_indices` builds on CPU copies of the same indices - every kind of layout `SlicedGemv`
builds, every index width, column parts, skewed rows -, deterministic, inverted bit for bit by the repack kernel, without
temporaries; and the product on top: `prepare()` / `prepare_model` build at load what the first one-token call would build lazily.

Ties.  The recipe orders the surplus elements of a (slice, window) segment by a float64 key with an argsort that is not asked to be
stable, so it leaves the order of EQUAL keys open; the kernel breaks a tie the way a stable sort does (class, then column).  The test
restates the key (`_second_key`, from sliced.py:layout_from_indices), builds the stable arrangement with the recipe itself
(`stable=True` passed to its second argsort) and holds the kernel to THAT position by position; the plain recipe may differ from it
only on elements whose key is tied, and there only as a set of (word, side) pairs.  At most 1 segment in 1000 over the whole
parametrisation may hold a tie (`test_tie_share`)."""
import pytest
import torch

import vptq_amd
from vptq_amd import compact_model, prepare_model
from vptq_amd import _backend as B
from vptq_amd.utils import sliced as S
from vptq_amd.utils.pack import pack_index
from vptq_amd.utils.sliced import SlicedGemv, layout_from_indices, layout_on_device, window_cols

from test_compact_cpu import _random_layer
from test_compact_gpu import FORMATS, make_layer, twin_of

pytestmark = pytest.mark.gpu

_SEGMENTS = {"all": 0, "tied": 0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    B.lib()
    return torch.device("cuda", 0)


def _as16(t):
    return torch.where(t >= 32768, t - 65536, t).to(torch.int16)


def _desc(packed, G, ib, rb, N, v=8):
    """descriptor over real packed indices (the other pointers are fake and aligned: the builder never reads through them)"""
    d = B.LayerDesc()
    d.in_features, d.out_features, d.vector_len, d.num_codebooks, d.group_size = G, N * v, v, 1, G
    d.num_centroids, d.num_res_centroids, d.index_bits, d.res_bits = 1 << ib, (1 << rb if rb else 0), ib, rb
    d.row_words, d.num_indices, d.dtype = packed.shape[-1], N, 0
    d.indices, d.centroids, d.res_centroids = packed.data_ptr(), 2 << 20, (3 << 20 if rb else None)
    d.weight_scale, d.weight_bias = 4 << 20, 5 << 20
    return d


def _second_key(idx, slices, index_bits, whole_table=False):
    """the recipe's second sort key per element, restated from vptq_amd/utils/sliced.py:layout_from_indices (the lines that build
    `order1` ... `order2`): (key [N, G] in the recipe's first order, segment id (slice * 4 + window) [N, G], column [N, G])"""
    lg = {8: 3, 16: 4, 32: 5}[slices]
    sb = max(index_bits - lg, 0)
    N, G = idx.shape
    col = torch.arange(G, dtype=torch.int64)
    sl = (col * slices // G)[None, :].expand(N, G).contiguous() if whole_table else idx >> sb
    local = idx if whole_table else idx & ((1 << sb) - 1)
    cls = local & 15
    win = torch.clamp(col // window_cols(G), max=3)[None, :].expand(N, G)
    sw = sl * 4 + win
    order1 = torch.argsort((sw * 16 + cls) * G + col[None, :], dim=1)
    seg1 = torch.gather(sw * 16 + cls, 1, order1)
    cnt1 = torch.zeros(N, slices * 4 * 16, dtype=torch.int64)
    cnt1.scatter_add_(1, seg1, torch.ones_like(seg1))
    rank1 = col[None, :] - torch.gather(torch.cumsum(cnt1, 1) - cnt1, 1, seg1)
    cnt3 = cnt1.reshape(N, slices * 4, 16)
    full = cnt3.min(2).values
    rest = cnt3.sum(2) - 16 * full
    b1 = seg1 >> 4
    full_e, rest_e, cnt_e = torch.gather(full, 1, b1), torch.gather(rest, 1, b1), torch.gather(cnt1, 1, seg1)
    spread = 16 * full_e + ((rank1 - full_e).double() + 0.5) * rest_e.double() / (cnt_e - full_e).clamp(min=1).double()
    place = torch.where(rank1 < full_e, (rank1 * 16 + (seg1 & 15)).double(), spread)
    key = (b1 * (2 * G)).double() + place + (seg1 & 15).double() / 64.0
    return key, b1, order1


def _tied_columns(idx, slices, index_bits, whole_table=False):
    """(bool [N, G]: the element of this column has a key equal to another one's; number of segments with a tie)"""
    key, b1, order1 = _second_key(idx, slices, index_bits, whole_table)
    ks, o2 = torch.sort(key, dim=1, stable=True)
    eq = ks[:, 1:] == ks[:, :-1]
    tied_sorted = torch.zeros_like(key, dtype=torch.bool)
    tied_sorted[:, 1:] |= eq
    tied_sorted[:, :-1] |= eq
    cols_sorted = torch.gather(order1, 1, o2)
    tied = torch.zeros_like(tied_sorted)
    tied.scatter_(1, cols_sorted, tied_sorted)
    seg_sorted = torch.gather(b1, 1, o2)
    rows = torch.arange(idx.shape[0])[:, None].expand_as(seg_sorted)
    n_seg = int(torch.unique((rows * 1024 + seg_sorted)[tied_sorted]).numel())
    return tied, n_seg


def _stable_recipe(monkeypatch, *args, **kw):
    """`layout_from_indices` with its (second) argsort made stable: the order the kernel documents for equal keys.  (The first
    argsort's keys are distinct - they contain the column -, so stability changes nothing there.)"""
    plain = torch.argsort
    with monkeypatch.context() as mp:
        mp.setattr(torch, "argsort", lambda t, dim=-1, **k: plain(t, dim=dim, stable=True))
        return layout_from_indices(*args, **kw)


def _rows_of(blocks):
    """row of every element position of a layout (lists in (slice, row) order, 64 elements per block)"""
    N = blocks.shape[1]
    sn = torch.repeat_interleave(torch.arange(blocks.numel()), blocks.reshape(-1).to(torch.int64)).repeat_interleave(64)
    return sn % N


def _check(monkeypatch, got, idx, slices, side_idx, index_bits, whole=False, side_dtype=torch.uint8, expect_tie=False):
    """`got` (the kernel's five tensors) against the recipe on the CPU indices: see the module docstring"""
    got = [None if t is None else t.cpu() for t in got]
    ref = layout_from_indices(idx, slices, side_idx, index_bits, whole, side_dtype)
    tied, n_seg = _tied_columns(idx, slices, index_bits, whole)
    # (without a tie every key of a row is distinct and the sort has one answer: the stable arrangement is the recipe's)
    stable = _stable_recipe(monkeypatch, idx, slices, side_idx, index_bits, whole, side_dtype) if n_seg else ref
    _SEGMENTS["all"] += idx.shape[0] * slices * 4
    _SEGMENTS["tied"] += n_seg
    if expect_tie:
        assert n_seg >= 1
    names = ("elems", "blocks", "first", "res", "wstart")
    for name, g, s in zip(names, got, stable):
        assert (g is None) == (s is None), name
        if g is not None:
            assert g.dtype == s.dtype and g.shape == s.shape, (name, g.dtype, s.dtype, g.shape, s.shape)
            assert torch.equal(g, s), (name, int((g != s).sum()), n_seg)
    # the plain recipe: identical except where keys are tied, and there the same (word, side) pairs per row
    for i in (1, 2, 4):
        assert torch.equal(ref[i], stable[i]), names[i]
    diff = ref[0] != stable[0]
    if ref[3] is not None:
        diff |= ref[3] != stable[3]
    if bool(diff.any()):
        rows = _rows_of(ref[1])[: diff.numel()]
        for lay in (ref, stable):
            w = lay[0][diff].to(torch.int64) & 0xFFFFFFFF
            assert bool(tied[rows[diff], w & 0xFFFF].all()), "the recipe's orders differ on an element whose key is not tied"
        pack = lambda lay: torch.sort(rows[diff] << 48 | (lay[0][diff].to(torch.int64) & 0xFFFFFFFF) << 16 |   # noqa: E731
                                      ((lay[3][diff].to(torch.int64) & 0xFFFF) if lay[3] is not None else 0)).values
        assert torch.equal(pack(ref), pack(stable))
    return n_seg


def _inputs(N, G, ib, rb, seed):
    """the skewed rows of test_compact_cpu._random_layer + one row with a single index everywhere (one class, one slice) + one row
    whose indices all fall in one slice"""
    idx, ridx, _ = _random_layer(N, G, ib, rb, seed)
    if N > 2:
        idx[1, :] = 5 + (3 << (ib - 3))
        idx[2, :] &= (1 << (ib - 5)) - 1
        if ridx is not None:
            ridx[1, :] = (1 << rb) - 1
            ridx[2, :] &= (1 << max(rb - 5, 0)) - 1
    packed = pack_index(_as16(idx)[None], ib, None if ridx is None else _as16(ridx)[None], rb)
    return idx, ridx, packed


@pytest.mark.parametrize("N", [37, 64])
@pytest.mark.parametrize("ib,rb,side", [(14, 0, None), (16, 0, None), (14, 8, torch.uint8), (16, 8, torch.uint8),
                                        (16, 12, torch.int16), (16, 16, torch.int16), (15, 8, torch.int16)])
@pytest.mark.parametrize("G,parts,slices", [(8192, 1, 16), (8192, 1, 8), (200, 1, 8), (1032, 2, 16), (216, 3, 8), (96, 3, 32),
                                            (14336, 1, 16), (72, 1, 8)])
def test_byte_identity(G, parts, slices, ib, rb, side, N, dev, monkeypatch):
    """every row of the issue's table: main bucket without / with a uint8 / uint16 side stream, the residual index as the bucket of a
    second table - sliced or whole -, column parts (1032 = 2 x 516 and 216 = 3 x 72 columns: parts share words of the packed row)"""
    idx, ridx, packed = _inputs(N, G, ib, rb, seed=ib * 100 + rb + G + N)
    pk = packed.to(dev)
    d = _desc(pk, G, ib, rb, N)
    sb = 0 if side is None else (1 if side == torch.uint8 else 2)
    w = G // parts
    for p in range(parts):
        got = layout_on_device(pk, d, slices, side_bytes=sb, parts=parts, part=p, any_shape=True)
        _check(monkeypatch, got, idx[:, p * w:(p + 1) * w].contiguous(), slices,
               None if ridx is None else ridx[:, p * w:(p + 1) * w].contiguous(), ib, side_dtype=side or torch.uint8)
    if rb and parts == 1:
        # the folded two-table form: table 0 without a side stream, table 1 bucketed by the residual index - sliced, and whole
        _check(monkeypatch, layout_on_device(pk, d, slices, any_shape=True), idx, slices, None, ib)
        _check(monkeypatch, layout_on_device(pk, d, slices, table=1, any_shape=True), ridx, slices, None, rb)
        _check(monkeypatch, layout_on_device(pk, d, slices, table=1, whole_table=True, any_shape=True), ridx, slices, None, rb, whole=True)


def test_one_row_layer_and_small_whole_tables(dev, monkeypatch):
    for G, slices in ((8192, 16), (72, 8)):
        idx, ridx, packed = _inputs(1, G, 16, 8, seed=G)
        pk = packed.to(dev)
        d = _desc(pk, G, 16, 8, 1)
        _check(monkeypatch, layout_on_device(pk, d, slices, side_bytes=1, any_shape=True), idx, slices, ridx, 16)
    # residual tables of 4 and 64 entries held whole (fewer than 16 classes: every element is surplus), and bucketed by an index
    # with fewer values than slices
    for rb in (2, 6):
        idx, ridx, packed = _random_layer(9, 4096, 16, rb, seed=rb)
        pk = packed.to(dev)
        d = _desc(pk, 4096, 16, rb, 9)
        _check(monkeypatch, layout_on_device(pk, d, 16, table=1, whole_table=True, any_shape=True), ridx, 16, None, rb, whole=True)
        _check(monkeypatch, layout_on_device(pk, d, 16, table=1, any_shape=True), ridx, 16, None, rb)


def test_tie_rule_is_the_stable_sorts(dev, monkeypatch):
    """64 rows x 8192 columns, 16 slices, seed 1: the recipe's keys hold at least one tie there; the kernel's order is that of
    `torch.argsort(key, stable=True)` (`_check` holds it to the stable arrangement position by position)"""
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, 65536, (64, 8192), generator=g, dtype=torch.int64)
    packed = pack_index(_as16(idx)[None], 16, None, 0)
    pk = packed.to(dev)
    got = layout_on_device(pk, _desc(pk, 8192, 16, 0, 64), 16, exact=True)
    assert _check(monkeypatch, got, idx, 16, None, 16, expect_tie=True) >= 1


def test_tie_share():
    """at most 1 segment in 1000 over the whole parametrisation above was compared under the tie rule"""
    assert _SEGMENTS["all"] > 0, "run the whole file: this test sums up the tests above"
    print(f"segments {_SEGMENTS['all']}, with tied keys {_SEGMENTS['tied']}")
    assert _SEGMENTS["tied"] * 1000 <= _SEGMENTS["all"], _SEGMENTS


def test_two_builds_on_two_streams_are_identical(dev):
    m = make_layer(4096, 4096, 8, 65536, 256, torch.float16, seed=3, dev=dev)
    d = m._descriptor().desc
    n = B.lib().vptq_sliced_layout_supported_for(d, B.GEMV_EXACT)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            outs.append(layout_on_device(m.indices.data, d, n, exact=True, side_bytes=1))
        s.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert outs[0][0].data_ptr() != outs[1][0].data_ptr()


@pytest.mark.parametrize("I,O,v,k,kr", FORMATS, ids=lambda p: str(p))
def test_repack_round_trip(I, O, v, k, kr, dev):
    """the repack kernel over kernel-built exact layouts returns the packed indices bit for bit (24592 columns, T = 22: two column
    parts that share words of the packed row)"""
    m = make_layer(I, O, v, k, kr, torch.float16, seed=I + k + kr, dev=dev)
    assert S.device_builder_enabled(m.indices.data)
    sl = SlicedGemv(m, exact=True)
    if I == 24592:
        assert sl.parts == 2
    assert torch.equal(sl.repack(), m.indices.data)


def test_build_memory(dev):
    """a kernel build of an 8192^2 v8-k65536-256 layer takes the returned tensors and nothing else (+ 1 MiB: allocator rounding);
    the torch recipe's peak on the same indices is printed"""
    m = make_layer(8192, 8192, 8, 65536, 256, torch.float16, seed=9, dev=dev)
    d = m._descriptor().desc
    n = B.lib().vptq_sliced_layout_supported_for(d, B.GEMV_EXACT)
    peaks = {}
    for name in ("kernel", "torch"):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        if name == "kernel":
            out = layout_on_device(m.indices.data, d, n, exact=True, side_bytes=1)
        else:
            idx, ridx = S.split_index_streams(m.indices.data, 8192, 8, 16)
            out = layout_from_indices(idx, n, ridx, 16)
            del idx, ridx
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated(dev) - base
        returned = sum(t.numel() * t.element_size() for t in out if t is not None)
        print(f"{name} build of 8192 x 8192 v8-k65536-256: peak {peaks[name] / 2**20:.1f} MiB above the level before, returned tensors {returned / 2**20:.1f} MiB")
        if name == "kernel":
            assert peaks[name] <= returned + (1 << 20), (peaks[name], returned)
        del out


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("I,O,v,k,kr", FORMATS, ids=lambda p: str(p))
def test_prepare_equals_the_lazy_torch_build(I, O, v, k, kr, dt, dev, monkeypatch):
    m = make_layer(I, O, v, k, kr, dt, seed=I + O + k + kr + 7, dev=dev)
    m.enable_sliced_layout(True)
    twin = twin_of(m)
    calls = []
    real = S.layout_on_device
    monkeypatch.setattr(S, "layout_on_device", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    rep = m.prepare()
    assert rep["built"] == "exact" and rep["bytes"] > 0 and rep["seconds"] > 0 and calls, rep
    st = m.__dict__["_sliced"]
    assert st[1] is not None and st[1].exact and m._sliced_gemv() is st[1]      # (cached under the stamp the lazy path uses)
    assert rep["bytes"] == sum(t.numel() * t.element_size() for tup in st[1]._tensors for t in tup if t is not None)
    n_calls = len(calls)
    monkeypatch.setattr(S, "device_builder_enabled", lambda t: False)           # the twin: the torch recipe, at its first call
    xs = {t: (torch.randn(1, t, I, device=dev) * 0.5).to(dt) for t in (1, 2, 3, 4)}
    for t in (1, 2, 3, 4):
        y, yt = m(xs[t]), twin(xs[t])
        assert torch.equal(y.view(torch.int16), yt.view(torch.int16)), (t, (y.float() - yt.float()).abs().max().item())
    assert len(calls) == n_calls and twin.__dict__["_sliced"][1] is not None
    for a, b in zip(st[1]._tensors, twin.__dict__["_sliced"][1]._tensors):      # (and the layouts themselves, tensor by tensor)
        for ta, tb in zip(a, b):
            assert (ta is None) == (tb is None) and (ta is None or torch.equal(ta, tb))


def test_prepare_folded_and_selective_kinds(dev):
    """the kinds `prepare` reports follow the arithmetic, as the lazy build does"""
    m = make_layer(4096, 4096, 8, 65536, 65536, torch.float16, seed=21, dev=dev)
    m.enable_sliced_layout(True)
    try:
        vptq_amd.set_arithmetic("folded")
        rep = m.prepare()
        sl = m._sliced_gemv()
        assert (rep["built"] == "folded" and sl is not None and not sl.exact and len(sl._tensors) == 2) or \
            (sl is None and "gather" in rep["built"]), rep     # (the gate may refuse the folded form of a layer: then none)
    finally:
        vptq_amd.set_arithmetic("reference")
    small = make_layer(1024, 512, 8, 65536, 256, torch.float16, seed=22, dev=dev)
    assert "gather" in small.prepare()["built"] and small.__dict__["_sliced"][1] is None
    can = make_layer(1024, 1024, 8, 256, 256, torch.float16, seed=23, dev=dev)
    assert "format" in can.prepare()["built"]


def test_prepare_makes_a_first_captured_call_sliced(dev):
    m = make_layer(4096, 4096, 8, 65536, 256, torch.float16, seed=31, dev=dev)
    cold = twin_of(m)
    cold.__dict__.pop("_sliced_on")
    x = torch.randn(1, 1, 4096, device=dev).half()
    s = torch.cuda.Stream()
    rep = m.prepare(stream=s)
    assert rep["built"] == "exact"
    sl = m.__dict__["_sliced"][1]
    assert set(sl._ws) == {s.cuda_stream}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        y = m(x)
    assert m.__dict__["_sliced"][1] is sl and set(sl._ws) == {s.cuda_stream}
    # the sliced route was taken: the launch went through this object's one-token entry
    g.replay()
    torch.cuda.synchronize()
    eager = m(x)
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), eager.view(torch.int16))
    # an unprepared twin captured the same way is captured on the gather kernel: no layout, no workspace
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        cold._descriptor()
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=s2):
        y2 = cold(x)
    assert cold.__dict__.get("_sliced") is None
    g2.replay()
    torch.cuda.synchronize()
    assert torch.allclose(y2.float(), eager.float(), atol=2e-2, rtol=2e-2)


def test_prepare_counts_the_sliced_launch_inside_a_capture(dev, monkeypatch):
    """... seen from the launch itself: the captured one-token call of a prepared layer goes through SlicedGemv._launch"""
    m = make_layer(4096, 4096, 8, 65536, 256, torch.float16, seed=32, dev=dev)
    s = torch.cuda.Stream()
    assert m.prepare(stream=s)["built"] == "exact"
    x = torch.randn(1, 1, 4096, device=dev).half()
    hits = []
    real = SlicedGemv._launch
    monkeypatch.setattr(SlicedGemv, "_launch", lambda self, *a: (hits.append(torch.cuda.is_current_stream_capturing()), real(self, *a))[1])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        y = m(x)
    assert hits == [True] and y is not None


def test_prepare_model_then_compact_model(dev):
    def build():
        torch.manual_seed(0)
        return torch.nn.Sequential(*[make_layer(4096, 4096, 8, 65536, kr, torch.float16, seed=40 + i, dev=dev)
                                     for i, kr in enumerate((256, 0, 256))]).eval()
    a, b = build(), build()
    rep = prepare_model(a)
    assert set(rep["layers"]) == {"0", "1", "2"} and rep["built"] == 3 and rep["bytes"] > 0
    assert all(r["built"] == "exact" for r in rep["layers"].values())
    ra, rb = compact_model(a), compact_model(b)
    assert ra["freed"] == rb["freed"] > 0 and ra["after"] == rb["after"] and ra["layers"].keys() == rb["layers"].keys() == {"0", "1", "2"}
    for t in (1, 4, 8):
        x = (torch.randn(1, t, 4096, device=dev) * 0.5).half()
        assert torch.equal(a(x).view(torch.int16), b(x).view(torch.int16)), t
