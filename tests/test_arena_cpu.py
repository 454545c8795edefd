"""tests/_arena.py tested without a device: CPU tensors and fake "kernels" in torch.  A stray store on either side of a placed
operand breaks intact(); an over-read that a zero multiplies away is invisible under the benign fill and NaN under the hostile one;
the offset alone decides the alignment class; contents, shape and dtype survive."""
import pytest
import torch

import _arena as ar

DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.int32, torch.int16, torch.uint8]
SMALL = 1 << 10   # (a small margin keeps these quick; MARGIN itself is checked once)


def _sample(dtype, shape=(3, 7)):
    n = 1
    for s in shape:
        n *= s
    t = torch.arange(1, n + 1, dtype=torch.float32).reshape(shape)
    return t.to(dtype)


def _past(view, arena, k):
    """element k past the end (k >= 0) or k elements before the start (k < 0) of a placed view, as a 0-dim view INTO the arena"""
    es = view.element_size()
    side = arena.post if k >= 0 else arena.pre
    typed = side.view(arena.itype).view(view.dtype) if view.dtype.is_floating_point else side.view(arena.itype)
    assert typed.element_size() == es
    return typed[k]


def test_margin_is_the_safety_condition():
    assert ar.MARGIN >= 64 << 10
    assert ar.MARGIN >= 4 * 8192 * 2      # gemv_k256m: 8192 columns x 2 bytes per staging extent
    assert ar.MARGIN >= 4 * 32768 * 2     # the sliced kernels: a whole layer's activations, up to 32768 columns
    v, a = ar.place(torch.zeros(5, dtype=torch.float16), ar.HOSTILE)
    assert a.pre.numel() == ar.MARGIN and a.post.numel() == ar.MARGIN and a.intact()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fill", [ar.BENIGN, ar.HOSTILE])
def test_contents_shape_and_dtype_survive(dtype, fill):
    t = _sample(dtype)
    v, a = ar.place(t, fill, offset=16, margin=SMALL)
    assert v.shape == t.shape and v.dtype == t.dtype and v.is_contiguous()
    assert torch.equal(v, t)
    assert a.intact() and a.damage() == []


@pytest.mark.parametrize("dtype", [torch.float16, torch.int32, torch.uint8])
@pytest.mark.parametrize("offset", [0, 4, 8, 16, 32, 48, 64, 128, 144, 240, 256, 272, 10928])
def test_offset_decides_the_alignment_class(dtype, offset):
    v, a = ar.place(_sample(dtype), ar.BENIGN, offset=offset, margin=SMALL)
    assert v.data_ptr() % 256 == offset % 256
    assert a.pre.numel() == SMALL + offset and a.post.numel() == SMALL


def test_element_sized_offsets():
    for dtype, es in ((torch.float16, 2), (torch.uint8, 1), (torch.float32, 4)):
        v, _ = ar.place(_sample(dtype), ar.HOSTILE, offset=es, margin=SMALL)
        assert v.data_ptr() % 256 == es
    with pytest.raises(AssertionError):
        ar.place(_sample(torch.float32), ar.BENIGN, offset=2, margin=SMALL)


def test_hostile_fill_is_the_documented_bit_pattern():
    for dtype, itype, bits in ((torch.float16, torch.int16, 0x7E00), (torch.bfloat16, torch.int16, 0x7FC0),
                               (torch.float32, torch.int32, 0x7FC00000)):
        v, a = ar.place(_sample(dtype), ar.HOSTILE, margin=SMALL)
        for side in (a.pre, a.post):
            assert bool((side.view(itype) == bits).all())
            assert bool(torch.isnan(side.view(itype).view(dtype)).all())
    for dtype in (torch.int32, torch.int16, torch.uint8):
        v, a = ar.place(_sample(dtype), ar.HOSTILE, margin=SMALL)
        assert bool((a.pre == 255).all()) and bool((a.post == 255).all())
    v, a = ar.place(_sample(torch.float16), ar.BENIGN, margin=SMALL)
    assert bool((a.pre == 0).all()) and bool((a.post == 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fill", [ar.BENIGN, ar.HOSTILE])
@pytest.mark.parametrize("k", [-1, 0], ids=["one-before", "one-after"])
def test_a_stray_store_breaks_intact(dtype, fill, k):
    v, a = ar.place(_sample(dtype), fill, offset=16, margin=SMALL)
    assert a.intact()
    _past(v, a, k).fill_(3)
    assert not a.intact()
    (side, dist, nbytes), = a.damage()
    assert side == ("after" if k == 0 else "before")
    assert dist == (0 if k == 0 else v.element_size())
    assert torch.equal(v, _sample(dtype))     # (the view itself was not touched)


def test_a_store_at_the_far_end_of_a_margin_breaks_intact():
    v, a = ar.place(_sample(torch.float16), ar.HOSTILE, margin=SMALL)
    a.post[-1] = 0x55
    assert not a.intact()
    v, a = ar.place(_sample(torch.float16), ar.HOSTILE, margin=SMALL)
    a.pre[0] = 0x55      # (0x7E00's low byte is zero: any other byte)
    assert not a.intact()


def _fake_kernel(x, a):
    """a "kernel" that reads one element PAST x and multiplies it by a zero weight: y = sum(x) + 0 * x[n]"""
    return x.float().sum() + 0.0 * _past(x, a, 0).float()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_a_masked_over_read_shows_only_under_the_hostile_fill(dtype):
    t = _sample(dtype)
    want = t.float().sum()
    xb, ab = ar.place(t, ar.BENIGN, margin=SMALL)
    xh, ah = ar.place(t, ar.HOSTILE, margin=SMALL)
    yb, yh = _fake_kernel(xb, ab), _fake_kernel(xh, ah)
    assert yb.view(torch.int32).item() == want.view(torch.int32).item()     # benign: the same bits as without the over-read
    assert bool(torch.isnan(yh))                                            # hostile: 0 x NaN
    assert ab.intact() and ah.intact()                                      # (a read breaks nothing)


def test_guarded_out():
    y, a = ar.guarded_out((2, 5), torch.float16, "cpu", offset=2, margin=SMALL)
    assert y.shape == (2, 5) and bool(torch.isnan(y).all()) and y.data_ptr() % 256 == 2
    assert bool((a.pre.view(torch.int16).view(torch.float16) == ar.SENTINEL).all())
    assert a.intact()
    y.fill_(1.0)
    assert a.intact()
    _past(y, a, 0).fill_(1.0)
    assert not a.intact()
    y, a = ar.guarded_out((3,), torch.float32, "cpu", offset=4, margin=SMALL)
    assert y.data_ptr() % 256 == 4 and bool((a.post.view(torch.int32).view(torch.float32) == ar.SENTINEL).all())


@pytest.mark.parametrize("align", [16, 256])
@pytest.mark.parametrize("zeroed", [True, False])
def test_guarded_workspace(align, zeroed):
    ws, a = ar.guarded_workspace(1000, zeroed, "cpu", align=align, margin=SMALL)
    assert ws.numel() == 1000 and ws.dtype == torch.uint8
    assert ws.data_ptr() % align == 0 and (align == 256 or ws.data_ptr() % (2 * align) != 0)
    assert bool((ws == (0 if zeroed else 255)).all())
    assert a.intact()
    ws.fill_(7)
    assert a.intact()
    a.post[0] = 0x55       # one byte past the size the query returned
    assert not a.intact()


def test_place_module_reseats_every_tensor():
    """an object with the attributes place_module touches (the real one needs the library): every tensor is re-seated at its
    offset with its contents, absent operands are left out, unknown names are refused"""
    import types
    P = lambda t: torch.nn.Parameter(t, requires_grad=False)   # noqa: E731
    m = types.SimpleNamespace(indices=P(_sample(torch.int32)), centroids=types.SimpleNamespace(weight=P(_sample(torch.float16))),
                              res_centroids=types.SimpleNamespace(weight=P(_sample(torch.float16))), enable_residual=True,
                              enable_outlier=False, enable_perm=True, perm=P(_sample(torch.int16, (8,))),
                              weight_scale=P(_sample(torch.float16, (8,))), weight_bias=P(_sample(torch.float16, (8,))), bias=None)
    before = {k: v.data.clone() for k, v in ar._module_params(m).items()}
    arenas = ar.place_module(m, ar.HOSTILE, {"indices": 16, "perm": 2, "weight_scale": 4})
    assert sorted(arenas) == sorted(["indices", "centroids", "res_centroids", "perm", "weight_scale", "weight_bias"])
    for k, p in ar._module_params(m).items():
        assert torch.equal(p.data, before[k]) and arenas[k].intact()
        assert p.data_ptr() % 256 == {"indices": 16, "perm": 2, "weight_scale": 4}.get(k, 0)
    with pytest.raises(AssertionError):
        ar.place_module(m, ar.BENIGN, {"scale_permuted": 16})


def test_place_layouts_reseats_every_tensor_and_rebuilds_the_structs():
    """an object with the attributes place_layouts touches (a real SlicedGemv needs a device): two structs - the second without a side
    stream -, every tensor re-seated at its offset with its contents, and the B.SlicedLayout array rebuilt over the views with the rows
    per wave, slice count and whole-table flags it had"""
    import types
    from vptq_amd.utils.sliced import _layout_structs

    def tup(res):
        return (_sample(torch.int32, (128,)), _sample(torch.int32, (8, 3)), _sample(torch.int32, (8, 3)), res, _sample(torch.int32, (8, 3, 5)))
    tensors = [tup(_sample(torch.uint8, (128,))), tup(None)]
    sl = types.SimpleNamespace(_tensors=tensors, _whole=[False, True], slices=8, layout=_layout_structs(tensors, [False, True], 3, 8))
    before = [[None if t is None else t.clone() for t in tp] for tp in tensors]
    offs = {"elems": 4, "blocks": 4, "first": 8, "res": 1, "wstart": 16}
    arenas = ar.place_layouts(sl, ar.HOSTILE, offs)
    assert len(arenas) == 9 and all(a.intact() for a in arenas)
    assert sl._lay_ref is sl.layout and len(sl.layout) == 2
    assert (sl.elems, sl.blocks, sl.first, sl.res, sl.wstart) == sl._tensors[0]
    for i, (tp, old) in enumerate(zip(sl._tensors, before)):
        st = sl.layout[i]
        assert (st.rows_per_wave, st.n_slices, st.whole_table) == (3, 8, i)
        for name, t, o in zip(ar.LAYOUT_OPERANDS, tp, old):
            if o is None:
                assert t is None and getattr(st, name) is None
                continue
            assert torch.equal(t, o) and t.data_ptr() % 256 == offs[name] and getattr(st, name) == t.data_ptr()
    with pytest.raises(AssertionError):
        ar.place_layouts(sl, ar.BENIGN, {"total": 8})
