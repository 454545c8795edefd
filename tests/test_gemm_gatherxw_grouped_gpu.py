"""vptq_quant_gemm_gatherxw_grouped (gemm_gatherxw_grouped.hip): 17 - 48 tokens of 2 - 4 sibling layers of gemm_gatherx's formats in
ONE launch - on the GPU.  Helpers, formats and shapes are tests/test_gemm_gatherx_grouped_gpu.py's.  The contract is BITS: member m's
y equals what vptq_quant_gemm_gatherxw (the parent's code) gives on the member's own descriptor, the same x and token count.
  1. bits: every (format, dtype, token count), hence all 24 instantiations; one row per (format, dtype) also against the float64 model
  2. a member switch inside a workgroup  3. the module: one launch, a captured step after prepare_model, a compacted member"""
import ctypes as C
import itertools

import pytest
import torch

from test_route_models_gpu import _np, dev   # noqa: F401  (dev: the module-scoped device fixture)
from test_gemm_gather_gpu import _Spy, GUARD, SENTINEL, F32
from test_gemm_gatherx_gpu import FMT, TILE
from test_gemm_gather_px_gpu import _stream_without_a_workspace
from test_gemm_gatherw_gpu import _bits
from test_gemm_gatherxw_gpu import call as own_call
from test_gemm_gather_grouped_gpu import group_descs, distinct_perms, _x, _Block, QKV, GU, PX_THREADS, PX_TOK
from test_gemm_gatherx_grouped_gpu import make_group, FMTS, RES, GS, OUTS, PERM_CASES
import _arith_model as am
from _gpu_util import spec_to_module

pytestmark = pytest.mark.gpu

ENTRY = "vptq_quant_gemm_gatherxw_grouped"
TOKS = (17, 32, 33, 48)   # one live row in the last block, a full last block, on either side of the TB switch


def instance(descs, n, tokens):
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(320)
    B.check(getattr(B.lib(), ENTRY + "_instance")(descs, n, tokens, 0, buf, len(buf)), ENTRY + "_instance")
    return buf.value.decode()


def want_instance(ds, tokens, fmt, dt):
    v, G, tb, k = FMT[fmt][0], ds[0].group_size, (tokens + 15) // 16, distinct_perms(ds)
    wgcu = min(2 if fmt == "v16-k65536-1024" else 4, 1 if RES[fmt] and tb == 3 else 2)   # resident: the LDS bound, the register bound
    groups = [(d.num_indices + 16 // v - 1) // (16 // v) for d in ds]
    grid = min(sum(groups), torch.cuda.get_device_properties(0).multi_processor_count * wgcu)
    head = "none" if k == 0 else \
        f"permute_x_tokens g={G} tok={tokens} grid={(G // 8 + PX_THREADS - 1) // PX_THREADS}x{(tokens + PX_TOK - 1) // PX_TOK} tpt={PX_TOK} perms={k}"
    return (f"{head} | gemm_gatherxw_grouped dt={dt} v={v} ib={ds[0].index_bits} rb={ds[0].res_bits} res={('none', 'lds', 'l2')[RES[fmt]]} "
            f"tok={tokens} tb={tb} n={len(ds)} groups={'+'.join(map(str, groups))} tiles={(G + TILE - 1) // TILE} wgcu={wgcu} grid={grid} "
            f"rgs={(sum(groups) + grid - 1) // grid}")


def grouped_call(descs, n, xt, outs, out_f32=False):
    # every y NaN between guard rows, a workspace of EXACTLY the query's bytes (0xFF)
    from vptq_amd import _backend as B
    tokens = xt.numel() // xt.shape[-1]
    need = getattr(B.lib(), ENTRY + "_workspace_bytes")(descs, n, tokens)
    assert need == distinct_perms([descs[i] for i in range(n)]) * ((tokens * xt.shape[-1] * 2 + 255) // 256 * 256)
    ws = torch.full((need,), 255, dtype=torch.uint8, device=xt.device) if need else None
    bufs = [torch.full((tokens + 2 * GUARD, O), SENTINEL, dtype=torch.float32 if out_f32 else xt.dtype, device=xt.device) for O in outs]
    ys = [b[GUARD:GUARD + tokens].fill_(float("nan")) for b in bufs]
    yp = (C.c_void_p * n)(*[y.data_ptr() for y in ys])
    assert getattr(B.lib(), ENTRY + "_supported")(descs, n, tokens) == 1
    B.check(getattr(B.lib(), ENTRY)(descs, n, xt.data_ptr(), yp, tokens, F32 if out_f32 else 0, ws.data_ptr() if need else None, need,
                                    B.current_stream_ptr(xt.device)), ENTRY)
    torch.cuda.current_stream(xt.device).synchronize()
    for b in bufs:
        assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + tokens:] == SENTINEL).all()), "a store outside y's token rows"
    return [y.clone() for y in ys]


def assert_own_bits(ys, ds, xt, outs, f32):
    for m, (y, d, O) in enumerate(zip(ys, ds, outs)):
        want = own_call(d, xt, O, out_f32=f32)
        assert torch.equal(_bits(y), _bits(want)), f"member {m}: {int((_bits(y) != _bits(want)).sum())} of {y.numel()} outputs differ from its own entry"


def _bit_rows():
    rows = []   # every (format, dtype, tokens); columns, permutation case and group size at strides of their own: every pair of them occurs
    for i, (fmt, dt, tokens) in enumerate(itertools.product(FMTS, ("f16", "bf16"), TOKS)):
        n = (2, 3, 4)[(i + i // 5) % 3]
        rows.append(pytest.param(dict(fmt=fmt, dt=dt, tokens=tokens, G=GS[(i + i // 8) % 4], case=PERM_CASES[(i + i // 4 + i // 8) % 4],
                                      outs=tuple(OUTS[(i + j) % 4] for j in range(n)), bias=(i // 2) % 2, model=tokens == TOKS[(i // 8) % 4]),
                                 id=f"{fmt}-{dt}-t{tokens}-i{i}"))
    return rows


@pytest.mark.parametrize("e", _bit_rows())
def test_bits_equal_every_members_own_entry(e, dev):
    G, fmt, tokens, outs = e["G"], e["fmt"], e["tokens"], e["outs"]
    Ls = make_group(G, outs, fmt, e["dt"], e["case"], bias=e["bias"])
    descs, ds, ms, keep = group_descs(Ls, dev)
    assert distinct_perms(ds) == {"shared": 1, "distinct": len(outs), "mixed": 1, "none": 0}[e["case"]]
    text = instance(descs, len(ds), tokens)
    assert text == want_instance(ds, tokens, fmt, e["dt"]), (text, want_instance(ds, tokens, fmt, e["dt"]))
    x, xt = _x(G, tokens, e["dt"], G + tokens, dev)
    out = {f32: grouped_call(descs, len(ds), xt, outs, out_f32=f32) for f32 in (False, True)}
    for f32 in (False, True):
        assert_own_bits(out[f32], ds, xt, outs, f32)
    if e["model"]:   # one row per (format, dtype): the project's float64 bar, unchanged
        for m, L in enumerate(Ls):
            mm, aa = am.model(am.pieces(L), x, arith="exact")
            am.check_both(_np(out[False][m]), _np(out[True][m]), mm, aa, L.dtype, what=f"member {m} of {text}")


@pytest.mark.parametrize("tokens", [20, 40])
@pytest.mark.parametrize("fmt,dt,case", [("v16-k65536-1024", "f16", "none"), ("v8-k65536-4", "bf16", "mixed"), ("v8-k32768-0", "f16", "shared"),
                                         ("v16-k65536-32768", "bf16", "distinct")])
def test_member_switch_inside_a_workgroup_keeps_every_members_bits(fmt, dt, case, tokens, dev):
    """2 CUs - 20, 30 and 40 row groups of 64 columns: a grid of 2 workgroups per CU ends inside member 1 and workgroups 10 .. 49 go from
    member 0 to member 2; one of 1 per CU ends inside member 0 and they reach member 2 in their third row group"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = [2 * cus - 20, 30, 40]
    outs = (16 * groups[0], 16 * groups[1] - 12, 16 * groups[2])
    Ls = make_group(64, outs, fmt, dt, case)
    descs, ds, ms, keep = group_descs(Ls, dev)
    text = instance(descs, 3, tokens)
    assert text == want_instance(ds, tokens, fmt, dt), text
    grid = int(text.rsplit(" grid=", 1)[1].split()[0])   # (the kernel's: the gather head has a grid of its own)
    first = [0, groups[0], groups[0] + groups[1], sum(groups)]
    member = lambda g: max(m for m in range(3) if first[m] <= g)
    walks = {tuple(sorted({member(g) for g in range(w, first[3], grid)})) for w in range(grid)}
    assert grid < first[3] and grid not in first and (0, 2) in walks, (grid, walks)
    _, xt = _x(64, tokens, dt, 7, dev)
    for f32 in (False, True):
        assert_own_bits(grouped_call(descs, 3, xt, outs, out_f32=f32), ds, xt, outs, f32)


def _spied(fn, monkeypatch):
    from vptq_amd import _backend as B
    calls, real = [], B.lib()
    monkeypatch.setattr(B, "lib", lambda: _Spy(real, calls))
    try:
        y = fn()
    finally:
        monkeypatch.setattr(B, "lib", lambda: real)
    return y, [c for c in calls if not c.endswith(("_supported", "_workspace_bytes", "_instance"))]


@pytest.mark.parametrize("names,outs,fmt,dt,case,tokens,extra", [
    (QKV, (512, 128, 132), "v16-k65536-1024", "f16", "shared", 24, None), (GU, (264, 260), "v8-k65536-4096", "bf16", "mixed", 48, None),
    (QKV, (128, 512, 136), "v16-k65536-65536", "bf16", "shared", 48, None), (GU, (260, 264), "v8-k32768-0", "f16", "mixed", 24, None),
    (QKV, (132, 512, 128), "v16-k65536-1024", "bf16", "distinct", 48, "graph"), (QKV, (512, 128, 132), "v16-k65536-0", "f16", "shared", 24, "compact")])
def test_linked_siblings_take_one_grouped_launch_with_their_own_bits(names, outs, fmt, dt, case, tokens, extra, dev, monkeypatch):
    import vptq_amd
    from vptq_amd import batched_decode as bd, grouped_decode as gd
    from vptq_amd.layers import link_siblings
    I = 2048
    monkeypatch.setattr(gd, "_GEMM_GATHERXW_GROUPED_MODE", "1")
    monkeypatch.setattr(bd, "_GEMM_GATHERXW_MODE", "1")       # an un-linked member's forward is its own vptq_quant_gemm_gatherxw launch
    Ls = make_group(I, outs, fmt, dt, case)
    xs = [_x(I, tokens, dt, s, dev)[1].reshape(1, tokens, I) for s in (9, 10)]
    twins, blk = (_Block(names, [spec_to_module(L, dev) for L in Ls]) for _ in range(2))
    assert link_siblings(blk) == 1
    if extra == "compact":   # a compacted member: the group steps aside, every member keeps its route and bits
        for b in (twins, blk):
            b.k_proj.compact(force=True)
            assert b.k_proj.is_compact()
    y_own, own = _spied(lambda: twins(xs[0]), monkeypatch)
    assert ENTRY not in own and (extra == "compact" or own == ["vptq_quant_gemm_gatherxw"] * len(outs)), own
    if extra == "graph":     # a fresh stream, its workspace sized by prepare_model: the captured step keeps the route
        s = _stream_without_a_workspace(dev)
        vptq_amd.prepare_model(blk, s)
        xg, g = xs[0].clone(), torch.cuda.CUDAGraph()
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                ys, calls = _spied(lambda: blk(xg), monkeypatch)
        torch.cuda.current_stream(dev).wait_stream(s)
        assert calls == [ENTRY], calls
        for x in (xs[1], xs[0], xs[1]):   # replays on new activations: the un-linked forward's bits
            xg.copy_(x)
            g.replay()
            torch.cuda.synchronize(dev)
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ys, twins(x)))
        return
    ys, calls = _spied(lambda: blk(xs[0]), monkeypatch)
    assert calls == (own if extra == "compact" else [ENTRY]), calls
    assert all(y.shape == (1, tokens, O) and torch.equal(_bits(y), _bits(w)) for y, w, O in zip(ys, y_own, outs))
