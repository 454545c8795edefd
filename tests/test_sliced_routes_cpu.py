"""vptq_amd/sliced_routes.py: the sliced-layout rules (1 - 4 tokens) as pure functions give, for every cell of a grid, the answers of
the rules as they stood in `vptq_amd/layers/vqlinear.py` - written out here line for line over the stand-in objects they took -, and
`VQuantLinear` reads them and remembers their answers as before.  No device."""
import itertools
import os
import subprocess
import sys
import types
import warnings

import pytest
import torch

from vptq_amd import _backend as B
from vptq_amd import sliced_routes as R
from vptq_amd.layers import vqlinear as vq
from test_host_cpu import _family_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rule_layer(I, O, v, kr, **more):
    """stands in for a VQuantLinear in the sliced-route rules: what `_index_elements` / `_res_centroids` and the glue read"""
    return types.SimpleNamespace(indices=torch.empty(1, O // v, 1), group_size=I, vector_len=v, out_features=O,
                                 num_res_centroids=kr, enable_residual=kr > 0, **more)


# ---- the three rule tests that stood in tests/test_host_cpu.py --------------------------------------------------------------------

def test_one_launch_rule_for_two_to_four_tokens():
    """VQuantLinear._sliced_one_launch: which layers send 2 - 4 tokens through the token kernel over the sliced layouts (the
    measured table of profiles/r04/sliced_tokens_one_launch.txt as a rule) - host logic, no GPU"""
    from vptq_amd.layers.vqlinear import VQuantLinear

    def layer(I, O, v, kr):
        return types.SimpleNamespace(indices=torch.empty(1, O // v, 1), group_size=I, vector_len=v, out_features=O,
                                     num_res_centroids=kr, enable_residual=kr > 0)

    def rule(I, O, v, kr, tokens, supported=True, exact=False, slices=8, one_pass=False):
        class SL:       # (stands in for vptq_amd.utils.sliced.SlicedGemv: what the library answers + the per-layout cache)
            def tokens_supported(self, t):
                return supported
        sl = SL()
        sl.exact, sl.slices = exact, slices
        sl.tokens_one_pass = lambda t: bool(one_pass)
        sl.tokens_window_parts = lambda t: int(one_pass)
        return VQuantLinear._sliced_one_launch(layer(I, O, v, kr), sl, tokens)
    for t in (2, 3, 4):
        assert rule(8192, 8192, 8, 0, t) and rule(4096, 4096, 8, 256, t) and rule(4096, 14336, 8, 65536, t) and rule(8192, 8192, 16, 0, t)
        assert not rule(2048, 512, 8, 256, t)                     # tiny: launch-bound on every route
        assert not rule(8192, 8192, 16, 1024, t)                  # v = 16 with a small residual table: the gather kernel holds it in LDS
        assert not rule(8192, 8192, 8, 0, t, supported=False)     # the library does not take it (no wstart, no room in LDS)
    assert rule(4096, 14336, 16, 65536, 2) and not rule(4096, 14336, 16, 65536, 4) and rule(8192, 8192, 16, 65536, 4)
    # the reference's roundings (profiles/r05/sliced_tokens_exact.txt): large v = 8 layers whose exact layout has 16 slices
    assert not rule(8192, 8192, 8, 256, 2, exact=True, slices=16)      # 2 tokens: two launches of the one-token kernel instead
    for t in (3, 4):
        assert rule(8192, 8192, 8, 256, t, exact=True, slices=16) and rule(14336, 4096, 8, 0, t, exact=True, slices=16)
        assert not rule(4096, 14336, 8, 256, t, exact=True, slices=8) and not rule(4096, 4096, 8, 0, t, exact=True, slices=8)
        assert not rule(8192, 8192, 16, 0, t, exact=True, slices=32) and not rule(8192, 2048, 8, 0, t, exact=True, slices=16)
        assert not rule(8192, 8192, 8, 256, t, exact=True, slices=16, supported=False)
    # ... and 2 / 3 tokens in ONE PASS of the one-token kernel wherever the library takes that (16-slice layouts, any size)
    for t in (2, 3):
        assert rule(8192, 8192, 8, 256, t, exact=True, slices=16, one_pass=True) and rule(8192, 1024, 8, 0, t, exact=True, slices=16, one_pass=True)
        assert not rule(2048, 8192, 8, 0, t, exact=True, slices=8, one_pass=True) and not rule(8192, 8192, 16, 0, t, exact=True, slices=32, one_pass=True)
        # two tables of v = 8: large layers with >= 4096 residual centroids (the one-token rule's sizes)
        assert rule(8192, 8192, 8, 65536, t, exact=True, slices=16, one_pass=True) and rule(8192, 8192, 8, 4096, t, exact=True, slices=16, one_pass=True)
        assert not rule(8192, 1024, 8, 65536, t, exact=True, slices=16, one_pass=True) and not rule(8192, 8192, 8, 1024, t, exact=True, slices=16, one_pass=True)
        assert not rule(8192, 8192, 8, 65536, t, exact=True, slices=16, one_pass=False)
    assert not rule(8192, 8192, 8, 65536, 4, exact=True, slices=16, one_pass=True)
    # ... and in WINDOW PARTS (the library's answer 2 / 4: half / a quarter of the columns staged per workgroup) on layers of >= 6 M index elements
    for t in (2, 3):
        assert rule(14336, 4096, 8, 256, t, exact=True, slices=16, one_pass=2) and rule(4096, 14336, 8, 0, t, exact=True, slices=8, one_pass=2)
        assert not rule(4096, 4096, 8, 0, t, exact=True, slices=8, one_pass=2) and not rule(14336, 512, 8, 0, t, exact=True, slices=16, one_pass=2)
    # (the glue remembers the answer on the layout, per token count)
    sl = types.SimpleNamespace(exact=False, slices=8, tokens_supported=lambda t: True, tokens_window_parts=lambda t: 0)
    assert VQuantLinear._sliced_one_launch(layer(8192, 8192, 8, 0), sl, 2) is True and sl.__dict__[("_one_launch", 2)] is True


def test_exact_route_size_rule_is_stated_once(monkeypatch):
    """`exact_route_is_large`, the one-token size rule of the reference arithmetic, at its boundaries (read from the constants), and
    `_compact_refusal(force=False)` answering with that very function: compact mode keeps a layer's one-token speed BECAUSE it asks
    the rule `_sliced_gemv` routes with - host logic, no GPU"""
    import vptq_amd.utils.sliced as sliced
    one, two = R._SLICED_EXACT_MIN_ELEMENTS, R._SLICED_EXACT_RG_MIN_ELEMENTS
    assert (one, two) == (1 << 20, 2 << 20)
    size_refusal = "one token takes the gather kernel for this layer (smaller than the exact sliced route's threshold; force=True compacts it)"
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(sliced, "exact_column_parts", lambda desc, group_size: (1, 16))   # (the library serves every case: the size rule is asked)

    class Indices:      # (packed indices "on a ROCm device", all zero: no bits past the end of a row)
        is_cuda = True

        def __init__(self, rows):
            self.shape = (1, rows, 1)

        def detach(self):
            return torch.zeros(1, 1, 1, dtype=torch.int32)

    def refusal(I, O, v, kr):
        m = _rule_layer(I, O, v, kr, num_centroids=65536, num_codebooks=1, enable_outlier=False, enable_norm=True, total_index_bits=0)
        m.indices = Indices(O // v)
        m._parameters = {"indices": m.indices}
        cache = vq.LayerCache("key", _family_desc(I, O, v, 65536, kr), [], torch.device("cpu"), None, 16, 1, torch.float16, 0, B.GEMV_EXACT, 0)
        m._descriptor = lambda: cache
        return vq.VQuantLinear._compact_refusal(m, False)

    # (v, kr, I, O, the bound the case sits AT (want) or just below (not want) - None: no size is large enough -, want)
    cases = ((8, 0, 4096, 2048, one, True), (8, 0, 4096, 2040, one, False), (8, 256, 4096, 2048, one, True), (8, 256, 4096, 2040, one, False),
             (8, 4096, 8192, 2048, two, True), (8, 4096, 8192, 2040, two, False),
             (8, 1024, 8192, 8192, None, False),     # a residual table under 4096 entries: the gather kernel holds it in LDS
             (16, 256, 8192, 8192, None, False))     # v = 16 has no byte side stream: the "other residual" branch
    for v, kr, I, O, bound, want in cases:
        m = _rule_layer(I, O, v, kr)
        if bound is not None:
            assert vq._index_elements(m) == bound if want else bound - bound // 256 <= vq._index_elements(m) < bound
        assert vq._res_centroids(m) == kr
        assert R.exact_route_is_large(v, kr, vq._index_elements(m)) is want, (v, kr, I, O)
        assert refusal(I, O, v, kr) == (None if want else size_refusal), (v, kr, I, O)
    # one rule, not two that agree today: the refusal follows whatever the function says - and so does the layout choice
    for v, kr, I, O, _, _ in cases:
        monkeypatch.setattr(R, "exact_route_is_large", lambda vector_len, res_centroids, index_elements: True)
        assert refusal(I, O, v, kr) is None
        assert R.sliced_layout_kind(B.GEMV_EXACT, v, kr, (O // v) * I, False, False, True, False) == ("exact", True)
        monkeypatch.setattr(R, "exact_route_is_large", lambda vector_len, res_centroids, index_elements: False)
        assert refusal(I, O, v, kr) == size_refusal
        assert R.sliced_layout_kind(B.GEMV_EXACT, v, kr, (O // v) * I, False, False, True, False) == ("exact", False)


def test_sliced_token_limit_rule(monkeypatch):
    """VQuantLinear._sliced_token_limit: most tokens served as one sliced launch per token (profiles/r04/sliced_tokens.txt, profiles/r05/
    sliced_tokens_exact.txt as a rule) - host logic, no GPU"""
    monkeypatch.setattr(R, "_SLICED_TOKENS_ENV", None)   # (the tuning override of the folded layouts' rule)

    def limit(I, O, v, kr, exact, slices, tables=1):
        sl = types.SimpleNamespace(exact=exact, slices=slices, layout=[None] * tables)
        return vq.VQuantLinear._sliced_token_limit(_rule_layer(I, O, v, kr), sl)
    assert limit(8192, 8192, 8, 256, True, 16) == 2
    assert limit(8192, 8192, 8, 256, True, 8) == 1 and limit(4096, 4096, 8, 256, True, 16) == 1
    assert limit(8192, 8192, 8, 65536, False, 16, 2) == 3
    assert limit(8192, 8192, 16, 65536, False, 16, 2) == 2
    assert limit(8192, 8192, 16, 1024, False, 16, 2) == 1
    sl = types.SimpleNamespace(exact=True, slices=16, layout=[None])
    assert vq.VQuantLinear._sliced_token_limit(_rule_layer(8192, 8192, 8, 256), sl) == 2 and sl._token_limit == 2   # (remembered on the layout)


# ---- the rules as they stood in vqlinear.py, line for line (their module globals read from `R`, so that a knob set there reaches both) ----

def _old_has_sliced_format(layer) -> bool:
    return bool(layer.num_centroids >= 16384 and layer.vector_len in (8, 16) and layer.num_codebooks == 1 and
                not layer.enable_outlier and layer.enable_norm)


def _old_exact_route_is_large(layer) -> bool:
    n_el, kr = vq._index_elements(layer), vq._res_centroids(layer)
    if kr > 0 and not (layer.vector_len == 8 and kr == 256):
        return kr >= 4096 and n_el >= R._SLICED_EXACT_RG_MIN_ELEMENTS
    return n_el >= R._SLICED_EXACT_MIN_ELEMENTS


def _old_kind(self, cache, lib, exact_column_parts):
    """the kind choice of `_sliced_gemv`"""
    desc, flags, n_el = cache.desc, cache.arithmetic_flags, vq._index_elements(self)
    opted = "_sliced_on" in self.__dict__   # (enable_sliced_layout() asks for a layout on any layer)
    if flags & B.GEMV_SELECTIVE and not flags & B.GEMV_EXACT and vq._res_centroids(self) >= 4096 and \
            (n_el >= R._SLICED_SELECTIVE_MIN_ELEMENTS or opted) and \
            lib.vptq_quant_gemv_sliced_selective_supported(desc) and lib.vptq_sliced_layout_supported_for(desc, 0):
        kind, wanted = "selective", True
    elif flags & (B.GEMV_EXACT | B.GEMV_SELECTIVE):
        kind, wanted = "exact", (_old_exact_route_is_large(self) or opted) and bool(exact_column_parts(desc, self.group_size)[0])
    else:   # the opt-in folded form: the folded layouts wherever the library has them
        kind, wanted = "folded", bool(lib.vptq_sliced_layout_supported_for(desc, 0))
    return kind, wanted


def _old_sliced_token_limit(self, sl) -> int:
    lim = sl.__dict__.get("_token_limit")
    if lim is None:
        n_el, kr = vq._index_elements(self), vq._res_centroids(self)
        if sl.exact:
            lim = 2 if (self.vector_len == 8 and kr in (0, 256) and sl.slices >= 16 and n_el >= 6 << 20) else 1
        elif R._SLICED_TOKENS_ENV is not None:
            lim = R._SLICED_TOKENS_ENV[1 if len(sl.layout) == 2 else 0]
        else:
            lim = 1
            if self.vector_len == 8 and kr in (0, 256) and n_el >= 6 << 20:
                lim = 2
            elif kr >= 16384 and n_el >= 3 << 20:
                lim = 3 if (self.vector_len == 8 and kr == 65536 and n_el >= 6 << 20) else 2
        sl.__dict__["_token_limit"] = lim
    return lim


def _old_sliced_one_launch(self, sl, tokens: int) -> bool:
    key = ("_one_launch", tokens)
    ok = sl.__dict__.get(key)
    if ok is None:
        n_el, kr = vq._index_elements(self), vq._res_centroids(self)
        if R._SLICED_ONE_LAUNCH in ("0", "off", "false", "no") or not sl.tokens_supported(tokens):
            ok = False
        elif R._SLICED_ONE_LAUNCH in ("1", "on", "true", "yes", "always"):
            ok = True
        elif sl.exact:
            if self.vector_len != 8:
                ok = False
            elif kr not in (0, 256):
                ok = sl.slices >= 16 and tokens <= 3 and kr >= 4096 and n_el >= R._SLICED_EXACT_RG_MIN_ELEMENTS and sl.tokens_one_pass(tokens)
            else:
                wparts = sl.tokens_window_parts(tokens) if tokens <= 3 else 0
                if wparts == 1:
                    ok = sl.slices >= 16
                elif wparts > 1:
                    ok = n_el >= 6 << 20
                else:
                    ok = sl.slices >= 16 and 3 <= tokens <= 4 and n_el >= 6 << 20
        else:
            if n_el < 1 << 19:       # (smaller layers are launch-bound on every route and were not measured)
                ok = False
            elif self.vector_len == 8 or kr == 0:
                ok = True
            elif kr <= 1024:
                ok = False
            else:
                ok = tokens == 2 or self.out_features <= 8192
        sl.__dict__[key] = ok
    return ok


V, KR = (8, 16), (0, 4, 256, 1024, 4096, 16384, 65536)
IN, OUT = (1024, 2048, 4096, 8192, 14336, 28672), (512, 1024, 2040, 2048, 4096, 8192, 14336, 28672)
LAYERS = [(I, O, v, kr) for v in V for kr in KR for I in IN for O in OUT]   # 672
EXACT, SELECTIVE = B.GEMV_EXACT, B.GEMV_SELECTIVE


def test_the_pure_rules_give_the_answers_of_the_rules_that_took_the_objects(monkeypatch):
    """Every cell of the grid: the five rules of vptq_amd/sliced_routes.py, handed plain integers, against the bodies they had in
    vqlinear.py, handed the stand-in layer / layout / library they read.  The grid holds the boundary cases of the three tests
    above (4096 x 2048 and 4096 x 2040 of v8-k65536-0 / -256, 8192 x 2048 and x 2040 of -4096, -1024 and v = 16) and every knob setting."""
    cells = 0
    # the format rule
    for v, k, books, outliers, norm in itertools.product((4, 8, 12, 16), (8192, 16384, 65536), (1, 2), (False, True), (False, True)):
        m = types.SimpleNamespace(vector_len=v, num_centroids=k, num_codebooks=books, enable_outlier=outliers, enable_norm=norm)
        assert R.has_sliced_format(v, k, books, outliers, norm) is _old_has_sliced_format(m), (v, k, books, outliers, norm)
        cells += 1
    layers = [(_rule_layer(I, O, v, kr), v, kr, (O // v) * I, O) for I, O, v, kr in LAYERS]
    # the one-token size rule and the kind choice
    for m, v, kr, n_el, O in layers:
        assert vq._index_elements(m) == n_el and vq._res_centroids(m) == kr
        assert R.exact_route_is_large(v, kr, n_el) is _old_exact_route_is_large(m), (v, kr, n_el)
        cells += 1
        for flags, opted, sel, fold, ex in itertools.product((0, EXACT, SELECTIVE, EXACT | SELECTIVE), (False, True), (0, 1), (0, 8), (0, 2)):
            m.__dict__.pop("_sliced_on", None)
            if opted:
                m.__dict__["_sliced_on"] = True
            lib = types.SimpleNamespace(vptq_quant_gemv_sliced_selective_supported=lambda desc: sel,
                                        vptq_sliced_layout_supported_for=lambda desc, f: fold)
            old = _old_kind(m, types.SimpleNamespace(desc=None, arithmetic_flags=flags), lib, lambda desc, group_size: (ex, 16))
            new = R.sliced_layout_kind(flags, v, kr, n_el, opted, bool(sel and fold), bool(ex), bool(fold))
            assert new == old and type(new[1]) is bool, (v, kr, n_el, flags, opted, sel, fold, ex)
            cells += 1
        m.__dict__.pop("_sliced_on", None)
    # the launch-per-token limit
    for env in (None, (3, 3), (4, 4)):
        monkeypatch.setattr(R, "_SLICED_TOKENS_ENV", env)
        for (m, v, kr, n_el, O), exact, slices, tables in itertools.product(layers, (False, True), (8, 16, 32), (1, 2)):
            sl = types.SimpleNamespace(exact=exact, slices=slices, layout=[None] * tables)
            assert R.sliced_token_limit(v, kr, n_el, exact, slices, tables) == _old_sliced_token_limit(m, sl), (env, v, kr, n_el, exact, slices, tables)
            cells += 1
    # 2 - 4 tokens in one launch (1 and 5 tokens: whatever the library's answer stands for, the rule does not widen it)
    for knob in ("auto", "0", "1"):
        monkeypatch.setattr(R, "_SLICED_ONE_LAUNCH", knob)
        for exact, slices, supported, wparts in itertools.product((False, True), (8, 16, 32), (False, True), (0, 1, 2, 4)):
            sl = types.SimpleNamespace(exact=exact, slices=slices, tokens_supported=lambda t: supported,
                                       tokens_one_pass=lambda t: wparts >= 1, tokens_window_parts=lambda t: wparts)
            for (m, v, kr, n_el, O), tokens in itertools.product(layers, (1, 2, 3, 4, 5)):
                sl.__dict__.pop(("_one_launch", tokens), None)
                assert R.sliced_one_launch(v, kr, n_el, O, tokens, exact, slices, supported, wparts) is _old_sliced_one_launch(m, sl, tokens), \
                    (knob, v, kr, n_el, O, tokens, exact, slices, supported, wparts)
                cells += 1
    assert cells == 96 + 672 * (1 + 64) + 3 * 672 * 12 + 3 * 48 * 672 * 5 == 551808 and cells >= 41130


# ---- the module is pure --------------------------------------------------------------------------------------------------------------

def test_the_rule_module_is_pure():
    """every rule runs on plain integers, and the module's own imports are `vptq_amd._backend` and nothing else of the package: a
    subprocess imports it under a bare stand-in for the package (`vptq_amd/__init__.py` itself imports the layers) and looks at
    `sys.modules`"""
    code = ("import sys, types\n"
            "pkg = types.ModuleType('vptq_amd'); pkg.__path__ = [%r]; sys.modules['vptq_amd'] = pkg\n"
            "import vptq_amd.sliced_routes as R\n"
            "mine = sorted(m for m in sys.modules if m.startswith('vptq_amd.'))\n"
            "assert mine == ['vptq_amd._backend', 'vptq_amd.sliced_routes'], mine\n"
            "assert 'vptq_amd.layers.vqlinear' not in sys.modules and 'vptq_amd.utils.sliced' not in sys.modules\n"
            "assert R.has_sliced_format(8, 65536, 1, False, True) is True and R.exact_route_is_large(8, 256, 1 << 20) is True\n"
            "assert R.sliced_layout_kind(R.B.GEMV_EXACT, 8, 256, 1 << 20, False, False, True, False) == ('exact', True)\n"
            "assert R.sliced_token_limit(8, 256, 8 << 20, True, 16, 1) == 2\n"
            "assert R.sliced_one_launch(8, 256, 8 << 20, 8192, 3, True, 16, True, 1) is True\n"
            "assert R.dense_from_layout(4096, 4096, True) is True and R.dense_from_layout(4096, 4096, False) is False\n"
            "assert R.sliced_build_bytes(1 << 20, False, True) == 5 << 20 and R.sliced_build_bytes(1 << 20, True, False) == 168 << 20\n"
            "print('pure')\n") % os.path.join(ROOT, "vptq_amd")
    env = {k: v for k, v in os.environ.items() if k not in ("VPTQ_TUNING", "VPTQ_SLICED_LAYOUT")}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "pure", out.stdout + out.stderr[-2000:]


def test_knob_spellings_are_the_sets_they_were(monkeypatch):
    """VPTQ_SLICED_LAYOUT and VPTQ_SLICED_ONE_LAUNCH take "0" / "off" / "false" / "no" and "1" / "on" / "true" / "yes" / "always",
    VPTQ_DEQUANT_SLICED "0" / "off" and "1" / "on"; the 160 bytes per element of the torch builder's temporaries have one name"""
    assert R._KNOB_OFF == ("0", "off", "false", "no") and R._KNOB_ON == ("1", "on", "true", "yes", "always")
    for word in R._KNOB_OFF + R._KNOB_ON + ("auto", "2", ""):
        monkeypatch.setattr(R, "_SLICED_ONE_LAUNCH", word)
        assert R.sliced_one_launch(8, 0, 1 << 10, 64, 2, False, 8, True, 0) is (word in R._KNOB_ON)      # (a tiny layer: "auto" says no)
        assert R.sliced_one_launch(8, 0, 8 << 20, 8192, 2, False, 8, True, 0) is (word not in R._KNOB_OFF)
        monkeypatch.setattr(R, "_DEQUANT_SLICED_MODE", word)
        assert R.dense_from_layout(8192, 8192, True) is (word in ("1", "on")) and R.dense_from_layout(64, 64, True) is (word not in ("0", "off"))
    assert R._SLICED_LAYOUT_ENV is (R._SLICED_LAYOUT_MODE not in R._KNOB_OFF) and R._SLICED_LAYOUT_ALWAYS is (R._SLICED_LAYOUT_MODE in R._KNOB_ON)
    assert R._SLICED_TORCH_BUILDER_BYTES == 160 and R._SLICED_SELECTIVE_MIN_ELEMENTS == 6 << 20
    for name in ("_SLICED_ONE_LAUNCH", "_SLICED_TOKENS_ENV", "_DEQUANT_SLICED_MODE"):   # (assigned to by tests and tools: no alias to go stale)
        assert not hasattr(vq, name), name


# ---- `_sliced_gemv`: what it remembers under the stamp and what it does not ---------------------------------------------------------

def _cpu_layer(monkeypatch):
    """a VQuantLinear built on the CPU whose descriptor builds (the device-only steps stood in for), opted in to a sliced layout"""
    m = vq.VQuantLinear(64, 32, vector_lens=[-1, 8], num_centroids=[-1, 256], num_res_centroids=[-1, 256], group_num=1,
                        group_size=64, outlier_size=0, indices_as_float=False, enable_norm=True, enable_perm=False,
                        is_indice_packed=True, bias=True, dtype=torch.float16, device="cpu", enable_proxy_error=False)
    monkeypatch.setattr(B, "require_device", lambda *tensors: torch.device("cuda", 0))
    monkeypatch.setattr(vq.VQuantLinear, "_folded_form_is_safe", lambda self, tensors, desc=None: False)   # (the gate's probes run on a GPU)
    m.enable_sliced_layout()
    cache = m._descriptor()
    return m, (cache.generation, B.tensor_version(m._parameters["indices"]))


def test_sliced_gemv_does_not_remember_a_capture(monkeypatch):
    m, stamp = _cpu_layer(monkeypatch)
    asked = []
    monkeypatch.setattr(R, "sliced_layout_kind", lambda *a: asked.append(a) or ("exact", False))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert m._sliced_gemv() is None and "_sliced" not in m.__dict__ and not asked
    # ... so the call after the capture decides, and THAT answer - the rule's "not wanted" - is stored under the stamp and not asked again
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    assert m._sliced_gemv() is None and m.__dict__["_sliced"] == (stamp, None) and len(asked) == 1
    assert m._sliced_gemv() is None and len(asked) == 1
    flags, v, kr, n_el, opted = asked[0][:5]
    assert (flags, v, kr, n_el, opted) == (B.GEMV_EXACT, 8, 256, 4 * 64, True) and all(type(a) is bool for a in asked[0][5:])


def test_sliced_gemv_does_not_remember_the_out_of_memory_back_off(monkeypatch):
    import vptq_amd.utils.sliced as sliced
    m, stamp = _cpu_layer(monkeypatch)
    monkeypatch.setattr(R, "sliced_layout_kind", lambda *a: ("exact", True))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(torch.cuda, "empty_cache", lambda: None)
    free = [1 << 30]
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (free[0], 4 << 30))
    builds, built = [], types.SimpleNamespace(exact=True, selective=False)

    def build(layer, exact=False, selective=False):
        builds.append((exact, selective))
        if len(builds) <= 2:    # (the first two attempts run out of device memory)
            raise torch.cuda.OutOfMemoryError("out of memory (stand-in)")
        return built
    monkeypatch.setattr(sliced, "SlicedGemv", build)
    with pytest.warns(UserWarning, match="sliced layout of a 64 x 32 layer not built") as seen:
        assert m._sliced_gemv() is None
    assert len(seen) == 1 and builds == [(True, False)] and "_sliced" not in m.__dict__
    assert m.__dict__["_sliced_oom"] == [R._SLICED_OOM_RETRY_CALLS, 2 * (1 << 30) + 4 * 64 * 160]
    with warnings.catch_warnings():
        warnings.simplefilter("error")      # (one warning per layer)
        assert m._sliced_gemv() is None     # inside the back-off: no second build attempt, nothing remembered
        assert len(builds) == 1 and "_sliced" not in m.__dict__ and m.__dict__["_sliced_oom"][0] == R._SLICED_OOM_RETRY_CALLS - 1
        free[0] = 3 << 30                   # twice the free bytes + the builder's temporaries: the build is tried again - and fails again
        assert m._sliced_gemv() is None and len(builds) == 2 and "_sliced" not in m.__dict__
        assert m.__dict__["_sliced_oom"] == [R._SLICED_OOM_RETRY_CALLS, 2 * (3 << 30) + 4 * 64 * 160]
        free[0] = 7 << 30
        assert m._sliced_gemv() is built and len(builds) == 3   # a successful build: stored under the stamp, the back-off cleared
    assert m.__dict__["_sliced"] == (stamp, built) and "_sliced_oom" not in m.__dict__
    assert m._sliced_gemv() is built and len(builds) == 3
