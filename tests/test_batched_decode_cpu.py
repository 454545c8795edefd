"""vptq_amd/batched_decode.py: the ordered table of batched-decode routes gives, for every call, the entries the five route functions
gave when `VQuantLinear.forward` composed them by hand - no device, no library."""
import ast
import itertools
import os

import pytest

from vptq_amd import _backend as B
from vptq_amd import batched_decode as bd
from vptq_amd.layers import vqlinear as vq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ((8, 65536, 0), (8, 65536, 256), (8, 65536, 65536), (16, 65536, 0), (16, 65536, 1024), (16, 65536, 65536), (8, 32768, 0),
           (8, 65536, 4096), (8, 256, 256), (8, 4096, 256), (4, 65536, 0))
SHAPES = ((8192, 8192), (4096, 4096), (14336, 4096), (28672, 8192), (512, 2048), (36, 1032), (8192, 8196))   # (out_features, in_features)
FLAGS = (0, B.GEMV_FORCE_GENERIC, B.GEMV_FORCE_BATCHED)
KNOBS = ("_GEMM_GATHER_PX_MODE", "_GEMM_GATHER_MODE", "_GEMM_GATHERX_MODE", "_GEMM_K256W_MODE", "_GEMM_GATHERW_MODE")
GATHER, GATHERX, K256W, GATHERW, PX = ("vptq_quant_gemm_gather", "vptq_quant_gemm_gatherx", "vptq_quant_gemm_k256w",
                                       "vptq_quant_gemm_gatherw", "vptq_quant_gemm_gather_px")


def ladder(v, k, kr, O, I, tokens, flags, perm, exact):
    """the four blocks of `VQuantLinear.forward` and the predicates of the four methods behind them as they stood before the table,
    line for line, for a layer of one codebook, no outliers, scale and bias whose library has every entry"""
    out = []
    entry = bd._batched_decode_entry(v, k, kr)
    # the permuted-layer block (px)
    if perm and 5 <= tokens <= 48 and entry is not None and vq.gemm_gather_px_route(v, k, kr, O, I, tokens) and \
            not (flags & B.GEMV_FORCE_GENERIC):
        out.append(PX)
    # the 5 - 16 token block (gather / gatherx)
    if 5 <= tokens <= 16 and entry is not None:
        route = vq.gemm_gather_route if entry == GATHER else vq.gemm_gatherx_route
        if route(v, k, kr, O, I, tokens) and not (flags & B.GEMV_FORCE_GENERIC):
            out.append(entry)
    # the canonical-format block (k256w)
    if 17 <= tokens <= 64 and (v, k, kr) == (8, 256, 256) and vq.gemm_k256w_route(O, I, tokens) and not (flags & B.GEMV_FORCE_ANY) and exact:
        out.append(K256W)
    # the 17 - 48 token block (gatherw)
    if 17 <= tokens <= 48 and entry == GATHER and vq.gemm_gatherw_route(v, k, kr, O, I, tokens) and not (flags & B.GEMV_FORCE_GENERIC) and \
            not (perm and bd._GEMM_GATHERW_MODE not in ("1", "on")):
        out.append(GATHERW)
    return out


def _route_everything(monkeypatch):
    """the table tests/test_gemm_gather_px_gpu.py routes its small layers with: every layer of the three kernels goes to px"""
    monkeypatch.setattr(bd, "GEMM_GATHERW_MIN_ELEMENTS", 0)
    monkeypatch.setattr(bd, "_GEMM_GATHER_PX_CELLS", tuple((8, 65536, kr, 0, 5, 48) for kr in (0, 256, 65536)) + tuple(
        f + (0, 5, 16) for f in ((16, 65536, 0), (16, 65536, 1024), (16, 65536, 65536), (8, 32768, 0), (8, 65536, 4096))))


@pytest.mark.parametrize("setting", ["committed", "everything"] + [f"{k}={m}" for k in KNOBS for m in "10"])
def test_the_table_gives_the_entries_the_route_functions_gave_composed_by_hand(setting, monkeypatch):
    """Every (format, shape, permutation, 0 - 70 tokens, flags, arithmetic): the routes of the table that take the call, in order, with "reference
    roundings only" applied last as both callers apply it, are `ladder`'s entries.  `ops.quant_gemm` wrote the same predicates with
    gatherw ahead of k256w; their formats are disjoint, so for a layer of one codebook, no outliers, scale and bias the op's ladder
    is this one (other layers: the library's `_supported` refused them there, the empty static tuple does here)."""
    if setting == "everything":
        _route_everything(monkeypatch)
    elif setting != "committed":
        monkeypatch.setattr(bd, *setting.split("="))
    seen = set()
    for (v, k, kr), (O, I), perm in itertools.product(FORMATS, SHAPES, (False, True)):
        routes = bd.batched_decode_routes(v, k, kr, 1, False, True, perm)
        assert all(r in bd.BATCHED_DECODE_ROUTES for r in routes)
        for tokens, flags in itertools.product(range(0, 71), FLAGS):
            got = [r for r in routes if bd.batched_decode_takes(r, v, k, kr, O, I, tokens, flags, perm)]   # (the callers' walk)
            for exact in (False, True):
                entries = [r.entry for r in got if exact or not r.exact_only]
                assert entries == ladder(v, k, kr, O, I, tokens, flags, perm, exact), (v, k, kr, O, I, perm, tokens, flags, exact)
                seen.update(entries)
            if got:
                assert bd.BATCHED_DECODE_MIN_TOKENS <= tokens <= bd.BATCHED_DECODE_MAX_TOKENS   # the callers' one guard
    knob, _, mode = setting.partition("=")
    off = {KNOBS[i]: e for i, e in enumerate((PX, GATHER, GATHERX, K256W, GATHERW))}.get(knob) if mode == "0" else None
    assert seen == {PX, GATHER, GATHERX, K256W, GATHERW} - {off}   # (the enumeration reaches every route in every setting)


def test_the_table_is_the_five_entries_in_priority_order():
    assert [r.entry for r in bd.BATCHED_DECODE_ROUTES] == [PX, GATHER, GATHERX, K256W, GATHERW]
    assert [r.knob for r in bd.BATCHED_DECODE_ROUTES] == list(KNOBS) and all(hasattr(bd, k) for k in KNOBS)
    assert (bd.BATCHED_DECODE_MIN_TOKENS, bd.BATCHED_DECODE_MAX_TOKENS) == (5, 64)
    assert [(r.min_tokens, r.max_tokens) for r in bd.BATCHED_DECODE_ROUTES] == [(5, 48), (5, 16), (5, 16), (17, 64), (17, 48)]
    assert [r.off_flags for r in bd.BATCHED_DECODE_ROUTES] == [B.GEMV_FORCE_GENERIC] * 3 + [B.GEMV_FORCE_ANY, B.GEMV_FORCE_GENERIC]
    assert [r.entry for r in bd.BATCHED_DECODE_ROUTES if r.exact_only] == [K256W]
    assert [r.entry for r in bd.BATCHED_DECODE_ROUTES if r.workspace] == [PX]


def test_layers_no_entry_serves_get_the_empty_static_tuple():
    for (v, k, kr), perm in itertools.product(FORMATS, (False, True)):
        assert bd.batched_decode_routes(v, k, kr, 2, False, True, perm) == ()     # two codebooks
        assert bd.batched_decode_routes(v, k, kr, 1, True, True, perm) == ()      # outliers
        assert bd.batched_decode_routes(v, k, kr, 1, False, False, perm) == ()    # no scale / bias
    assert bd.batched_decode_routes(8, 4096, 256, 1, False, True, True) == () and bd.batched_decode_routes(4, 65536, 0, 1, False, True, True) == ()
    entries = lambda *a: [r.entry for r in bd.batched_decode_routes(*a)]   # noqa: E731
    assert entries(8, 65536, 256, 1, False, True, True) == [PX, GATHER, GATHERW] and entries(8, 65536, 256, 1, False, True, False) == [GATHER, GATHERW]
    assert entries(16, 65536, 1024, 1, False, True, True) == [PX, GATHERX] and entries(8, 256, 256, 1, False, True, True) == [K256W]


def test_the_rules_module_stands_alone_and_the_callers_import_it_at_the_top():
    """batched_decode.py imports `_backend` and nothing of `layers` / `ops`; `ops/quant_gemm.py` no longer imports `vqlinear` inside a
    function body; `vqlinear` re-exports the route functions and the token windows, not the knobs and the cell tables"""
    tree = ast.parse(open(os.path.join(ROOT, "vptq_amd", "batched_decode.py")).read())
    mods = [f"{n.module}.{a.name}" if isinstance(n, ast.ImportFrom) else a.name for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom))
            for a in n.names]
    assert [m for m in mods if m.startswith("vptq_amd")] == ["vptq_amd._backend"] and not [m for m in mods if m.startswith("torch")], mods
    tree = ast.parse(open(os.path.join(ROOT, "vptq_amd", "ops", "quant_gemm.py")).read())
    for fn in (n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))):
        for n in (n for n in ast.walk(fn) if isinstance(n, (ast.Import, ast.ImportFrom))):
            named = [getattr(n, "module", None) or ""] + [a.name for a in n.names]
            assert not any("vqlinear" in s for s in named), (fn.name, named)
    for name in ("gemm_gather_route", "gemm_gatherx_route", "gemm_k256w_route", "gemm_gatherw_route", "gemm_gather_px_route",
                 "GEMM_GATHER_MAX_TOKENS", "GEMM_K256W_MIN_TOKENS", "GEMM_K256W_MAX_TOKENS", "GEMM_GATHERW_MIN_TOKENS", "GEMM_GATHERW_MAX_TOKENS",
                 "GEMM_GATHER_PX_MIN_TOKENS", "GEMM_GATHER_PX_MAX_TOKENS"):
        assert getattr(vq, name) is getattr(bd, name), name
    for name in KNOBS + tuple(k.replace("_MODE", "_CELLS") for k in KNOBS) + ("GEMM_GATHERW_MIN_ELEMENTS",):
        assert hasattr(bd, name) and not hasattr(vq, name), name
