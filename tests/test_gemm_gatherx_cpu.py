"""Host side of vptq_quant_gemm_gatherx (gemm_gatherx.hip; added within ABI 12), without a GPU: the symbols, the `_supported` truth
table (every large-codebook format vptq_quant_gemm_gather does not own, and nothing it does), the entry's validation order (every error
returns before a launch), the instance line against a Python restatement of the launcher's decision, a census of the 2 x 2 x 3 x 2
instantiations against the lines, and the Python route function."""
import ctypes
import itertools
import os
import re

from test_gemm_gather_cpu import desc, X, Y, CUS   # the descriptor with fake aligned pointers; nothing is dereferenced by host logic
from vptq_amd import _backend as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vptq_quant_gemm_gatherx_supported", "vptq_quant_gemm_gatherx", "vptq_quant_gemm_gatherx_instance")
TILE, TILE_BYTES, RES_LDS_MAX, LDS_PER_CU, MAX_WG_PER_CU = 1024, 32768, 32768, 160 * 1024, 4   # the kernel's constants
# (vector length, main centroids, residual centroids): the formats of the issue
FORMATS = [(16, 65536, 65536), (16, 65536, 32768), (16, 65536, 1024), (16, 65536, 256), (16, 65536, 64), (16, 65536, 0),
           (8, 65536, 4096), (8, 65536, 4), (8, 32768, 0), (8, 16384, 0)]
GATHER_OWNED = [(8, 65536, 0), (8, 65536, 256), (8, 65536, 65536)]


def fdesc(v, k, kr, **kw):
    kw.setdefault("O", 4096)
    return desc(kr, v=v, k=k, **kw)


def line(d, tokens, flags=0):
    buf = ctypes.create_string_buffer(256)
    rc = B.lib().vptq_quant_gemm_gatherx_instance(d, tokens, flags, buf, len(buf))
    return rc, buf.value.decode()


def test_symbols_are_declared_exported_and_bound_within_abi_12():
    hdr = open(os.path.join(ROOT, "include", "vptq_hip.h")).read()
    declared = set(re.findall(r"VPTQ_API[^;(]*?\b(vptq_\w+)\s*\(", hdr))
    raw = ctypes.CDLL(B.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, f"{s} not declared in include/vptq_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in B.EXPORTS and getattr(B.lib(), s).argtypes == B.EXPORTS[s][1], f"{s} not bound"
    assert B.lib().vptq_abi_version() == B.ABI_VERSION == 12
    from vptq_amd import ops
    assert callable(ops.quant_gemm_gatherx)


def test_supported_truth_table():
    sup, gsup = B.lib().vptq_quant_gemm_gatherx_supported, B.lib().vptq_quant_gemm_gather_supported
    for (v, k, kr), tokens in itertools.product(FORMATS, (1, 16)):
        assert sup(fdesc(v, k, kr), tokens) == 1, (v, k, kr, tokens)
        assert sup(fdesc(v, k, kr, perm=True, dtype=1), tokens) == 1
        assert gsup(fdesc(v, k, kr), tokens) == 0                       # a layer has ONE batched-decode kernel
    for (v, k, kr), tokens in itertools.product(GATHER_OWNED, (1, 5, 16)):
        assert gsup(fdesc(v, k, kr), tokens) == 1 and sup(fdesc(v, k, kr), tokens) == 0, (v, k, kr, tokens)
    assert sup(None, 1) == 0
    for tokens in (0, 17, -1):
        assert sup(fdesc(16, 65536, 1024), tokens) == 0
    assert sup(fdesc(8, 256, 256), 16) == 0 and sup(fdesc(8, 8192, 0), 16) == 0 and sup(fdesc(16, 8192, 256), 16) == 0   # small main codebooks
    assert sup(fdesc(12, 65536, 4096, O=12 * 300), 16) == 0                  # v = 12
    assert sup(fdesc(16, 65536, 1024, outliers=128), 16) == 0                # outlier columns
    assert sup(fdesc(16, 65536, 1024, C=2), 16) == 0                         # two codebook groups
    assert sup(fdesc(16, 65536, 1024, norm=False), 16) == 0                  # no scale / bias
    assert sup(fdesc(16, 65536, 0, I=4100), 16) == 0                         # G % 8 != 0
    for field in ("indices", "centroids", "res_centroids"):                  # a table that is not 16-byte aligned
        d = fdesc(16, 65536, 1024)
        setattr(d, field, getattr(d, field) + 8)
        assert sup(d, 16) == 0, field
    d = fdesc(16, 65536, 1024, perm=True)
    d.scale_permuted = None                                                  # a permutation without scale / bias in column order
    assert sup(d, 16) == 0
    d = fdesc(8, 65536, 4096)
    d.row_words -= 1                                                         # a row shorter than its G x T bits
    assert sup(d, 16) == 0
    d = fdesc(8, 65536, 256)
    d.row_words += 2                                                         # a padded row: not gemm_gather's exact layout - the generic one's
    assert gsup(d, 16) == 0 and sup(d, 16) == 1
    # ... and the queries of the routes it sits beside are what they were
    lib = B.lib()
    assert lib.vptq_quant_gemv_max_tokens(fdesc(16, 65536, 1024)) == 8 and lib.vptq_quant_gemv_max_tokens(fdesc(8, 32768, 0)) == 8   # (v = 16: two launches of 4)
    for v, k, kr in FORMATS:
        assert lib.vptq_quant_gemv_kernel_name(fdesc(v, k, kr), 4, 0) == b"gemv_gatherx_kernel"
    for v, k, kr in GATHER_OWNED:
        assert lib.vptq_quant_gemv_kernel_name(fdesc(v, k, kr), 16, 0) == b"gemv_gather_kernel"


def test_validation_order_null_tokens_unsupported():
    """every error is a VPTQ_E_* code: returned before a launch (there is no device here - a launch would answer with a HIP error)"""
    call = B.lib().vptq_quant_gemm_gatherx
    d, bad, owned = fdesc(16, 65536, 1024), fdesc(8, 256, 256), fdesc(8, 65536, 256)
    assert call(None, X, Y, 4, 0, None) == B.E_NULL
    assert call(d, None, Y, 4, 0, None) == B.E_NULL and call(d, X, None, 4, 0, None) == B.E_NULL
    assert call(bad, None, Y, 17, 0, None) == B.E_NULL          # NULL before tokens before unsupported
    for tokens in (0, 17, -3):
        assert call(d, X, Y, tokens, 0, None) == B.E_TOKENS
        assert call(bad, X, Y, tokens, 0, None) == B.E_TOKENS   # tokens before unsupported
    assert call(bad, X, Y, 4, 0, None) == B.E_UNSUPPORTED
    assert call(owned, X, Y, 4, 0, None) == B.E_UNSUPPORTED     # gemm_gather's layer
    assert call(fdesc(16, 65536, 1024, C=2), X, Y, 16, 0, None) == B.E_UNSUPPORTED
    for off in (2, 4, 8):
        assert call(d, X + off, Y, 4, 0, None) == B.E_UNSUPPORTED   # x not 16-byte aligned
    assert b"x must be 16-byte" in B.lib().vptq_last_error()
    assert call(bad, X + 8, Y, 4, 0, None) == B.E_UNSUPPORTED and b"x must be" not in B.lib().vptq_last_error()   # unsupported before x alignment
    for flags in (B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):   # flags do not change the validation
        assert call(d, X + 8, Y, 4, flags, None) == B.E_UNSUPPORTED and call(d, X, Y, 17, flags, None) == B.E_TOKENS


def want(d, tokens, cus=CUS):
    """the launcher's decision (gemm_gatherx_decide), restated"""
    v, kr = d.vector_len, d.num_res_centroids
    res_bytes = kr * v * 2
    res = "none" if res_bytes == 0 else "lds" if res_bytes <= RES_LDS_MAX else "l2"
    lds = TILE_BYTES + (res_bytes if res == "lds" else 0)
    wgcu = min(MAX_WG_PER_CU, LDS_PER_CU // lds)
    rows = 16 // v
    groups = (d.num_indices + rows - 1) // rows
    grid = min(groups, cus * wgcu)
    return (f"gemm_gatherx dt={'f16' if d.dtype == 0 else 'bf16'} v={v} ib={d.index_bits} rb={d.res_bits} res={res} "
            f"perm={int(bool(d.perm))} tok={tokens} tiles={(d.group_size + TILE - 1) // TILE} wgcu={wgcu} rgs={(groups + grid - 1) // grid}")


def test_instance_line_fields():
    cases = [(fdesc(16, 65536, 0), 1), (fdesc(16, 65536, 1024, I=8192, O=8192, dtype=1), 9), (fdesc(16, 65536, 65536, I=1032, O=20, perm=True), 16),
             (fdesc(16, 65536, 256, I=8, O=5), 5), (fdesc(16, 65536, 64, I=28672, O=8192, dtype=1, perm=True), 12),
             (fdesc(16, 65536, 32768, I=64, O=16 * (4 * CUS + 3) - 12), 8), (fdesc(16, 65536, 1024, I=64, O=16 * (2 * CUS + 3) - 12), 8),
             (fdesc(8, 65536, 4096, I=4096, O=14336), 15), (fdesc(8, 65536, 4, I=2312, O=20, perm=True), 6), (fdesc(8, 32768, 0, dtype=1), 16),
             (fdesc(8, 16384, 0, I=14336), 7), (fdesc(8, 65536, 2048), 5), (fdesc(8, 32768, 0, I=64, O=8 * (2 * 4 * CUS + 3) - 4), 8)]
    for d, tokens in cases:
        rc, text = line(d, tokens)
        assert rc == 0 and text == want(d, tokens), (text, want(d, tokens))
    assert line(cases[0][0], 1)[1] == "gemm_gatherx dt=f16 v=16 ib=16 rb=0 res=none perm=0 tok=1 tiles=4 wgcu=4 rgs=1"
    assert line(cases[1][0], 9)[1] == "gemm_gatherx dt=bf16 v=16 ib=16 rb=10 res=lds perm=0 tok=9 tiles=8 wgcu=2 rgs=1"   # 32 + 32 KiB of LDS
    assert line(cases[7][0], 15)[1] == "gemm_gatherx dt=f16 v=8 ib=16 rb=12 res=l2 perm=0 tok=15 tiles=4 wgcu=4 rgs=1"    # a 64 KiB table: from L2
    assert " rb=11 res=lds " in line(cases[11][0], 5)[1] and " wgcu=2 " in line(cases[11][0], 5)[1]                       # v = 8: 32 KiB at kr = 2048
    for i in (5, 6, 12):                                               # more row groups than workgroups of the launch
        assert line(*cases[i])[1].endswith("tiles=1 wgcu=%d rgs=2" % (2 if i == 6 else 4))
    # flags that change nothing leave the line as it is
    for flags in (B.GEMV_FAST_MATH, B.GEMV_SELECTIVE, B.GEMV_EXACT, B.GEMV_OUT_F32):
        assert line(cases[1][0], 9, flags) == line(cases[1][0], 9)
    # the call's own errors, and a buffer that is too small
    assert line(fdesc(16, 65536, 1024), 17)[0] == B.E_TOKENS and line(fdesc(8, 256, 256), 4)[0] == B.E_UNSUPPORTED
    assert line(fdesc(8, 65536, 256), 4)[0] == B.E_UNSUPPORTED
    small = ctypes.create_string_buffer(16)
    assert B.lib().vptq_quant_gemm_gatherx_instance(fdesc(16, 65536, 1024), 4, 0, small, len(small)) == B.E_WORKSPACE and small.value == b""
    assert B.lib().vptq_quant_gemm_gatherx_instance(fdesc(16, 65536, 1024), 4, 0, None, 0) == B.E_NULL


def test_census_of_the_instantiations():
    """gemm_gatherx_kernel<DT, V, RES, PERM>: 2 x 2 x 3 x 2 instantiations in the source, each reachable and named by a line"""
    src = open(os.path.join(ROOT, "vptq_amd", "csrc", "gemm_gatherx.hip")).read()
    assert re.search(r"template <typename DT, int V, int RES, bool PERM>\s*__global__", src)
    assert set(re.findall(r"gemm_gatherx_kernel<DT, V, RES, (true|false)>", src)) == {"true", "false"}
    assert set(re.findall(r"case (\d+): return launch_gx<DT, V, \1>", src)) == {"0", "1", "2"}
    assert set(re.findall(r"case (\d+): return launch_gx_v<DT, \1>", src)) == {"8", "16"}
    assert "launch_gx_dt<F16>" in src and "launch_gx_dt<BF16>" in src
    by_res = {(8, "none"): (32768, 0), (8, "lds"): (65536, 4), (8, "l2"): (65536, 4096),
              (16, "none"): (65536, 0), (16, "lds"): (65536, 1024), (16, "l2"): (65536, 32768)}
    seen = set()
    for dtype, ((v, res), (k, kr)), perm in itertools.product((0, 1), by_res.items(), (False, True)):
        rc, text = line(fdesc(v, k, kr, dtype=dtype, perm=perm), 16)
        assert rc == 0
        m = re.fullmatch(r"gemm_gatherx dt=(f16|bf16) v=(8|16) ib=\d+ rb=\d+ res=(none|lds|l2) perm=([01]) tok=16 tiles=4 wgcu=[24] rgs=1", text)
        assert m, text
        assert m.groups() == ("f16" if dtype == 0 else "bf16", str(v), res, str(int(perm)))
        seen.add(m.groups())
    assert len(seen) == 2 * 2 * 3 * 2
    assert "gemm_gatherx.hip" in open(os.path.join(ROOT, "vptq_amd", "csrc", "Makefile")).read()


SHAPES = ((8192, 8192), (4096, 4096), (14336, 4096), (4096, 14336), (8192, 28672), (1024, 4096), (512, 2048))


def test_route_function_is_pure_and_bounded(monkeypatch):
    from vptq_amd import batched_decode as bd
    from vptq_amd.layers import vqlinear as vq
    route = vq.gemm_gatherx_route
    assert bd._GEMM_GATHERX_MODE == "auto"          # (the knob is read with VPTQ_TUNING=1 only)
    for mode in ("auto", "1", "0"):
        monkeypatch.setattr(bd, "_GEMM_GATHERX_MODE", mode)
        for tokens in range(0, 20):
            for v, k, kr in GATHER_OWNED:           # the formats gemm_gather owns never route here
                assert not route(v, k, kr, 8192, 8192, tokens)
            assert not route(8, 256, 256, 8192, 8192, tokens) and not route(8, 8192, 256, 8192, 8192, tokens)   # small main codebooks
            assert not route(12, 65536, 4096, 8184, 8192, tokens) and not route(4, 65536, 0, 8192, 8192, tokens)
            assert not route(16, 65536, 1024, 8192, 8196, tokens)                                               # columns % 8
            assert not route(16, 65536, 1000, 8192, 8192, tokens)
        for (v, k, kr), (O, I) in itertools.product(FORMATS, SHAPES):
            for tokens in (0, 1, 4, 17, 64):
                assert not route(v, k, kr, O, I, tokens)          # outside 5 .. 16: never
    monkeypatch.setattr(bd, "_GEMM_GATHERX_MODE", "auto")
    for cells in (bd._GEMM_GATHERX_CELLS, ((16, 65536, 1024, 4 << 20, 9), (16, 65536, 1024, 16 << 20, 5), (8, 32768, 0, 0, 12))):
        monkeypatch.setattr(bd, "_GEMM_GATHERX_CELLS", cells)
        for (v, k, kr), (O, I) in itertools.product(FORMATS, SHAPES):
            on = [t for t in range(0, 20) if route(v, k, kr, O, I, t)]
            assert on == (list(range(on[0], 17)) if on else []) and (not on or on[0] >= 5)   # from some token count on, up to 16
            assert on == [t for t in range(0, 20) if route(v, k, kr, O, I, t)]               # pure: asked twice, the same
            for cell in cells:                                                              # ... and exactly what the cells say
                assert len(cell) == 5
            first = min((c[4] for c in cells if c[:3] == (v, k, kr) and ((O + v - 1) // v) * I >= c[3]), default=None)
            assert (on[0] if on else None) == (None if first is None else max(first, 5))
    monkeypatch.setattr(bd, "_GEMM_GATHERX_CELLS", ((16, 65536, 1024, 4 << 20, 9),))
    assert route(16, 65536, 1024, 8192, 8192, 9) and not route(16, 65536, 1024, 8192, 8192, 8)
    assert not route(16, 65536, 1024, 4096, 4096, 16) and not route(16, 65536, 256, 8192, 8192, 16)
    # the knob: every format of the kernel from 5 tokens / none
    monkeypatch.setattr(bd, "_GEMM_GATHERX_MODE", "1")
    for v, k, kr in FORMATS:
        assert all(route(v, k, kr, 512, 2048, t) for t in range(5, 17)) and not route(v, k, kr, 512, 2048, 4)
        assert not route(v, k, kr, 512, 2048, 17)
    monkeypatch.setattr(bd, "_GEMM_GATHERX_MODE", "0")
    assert not any(route(v, k, kr, 8192, 8192, t) for v, k, kr in FORMATS for t in range(0, 20))
    # gemm_gather_route is what it was: it never takes a format of this kernel
    monkeypatch.setattr(bd, "_GEMM_GATHER_MODE", "1")
    assert not any(vq.gemm_gather_route(v, k, kr, 8192, 8192, t) for v, k, kr in FORMATS for t in range(0, 20))


def test_knob_is_read_only_under_tuning(monkeypatch):
    """VPTQ_GEMM_GATHERX reaches the module through tune_env alone: without VPTQ_TUNING=1 it is ignored"""
    assert "VPTQ_GEMM_GATHERX" not in open(os.path.join(ROOT, "vptq_amd", "layers", "vqlinear.py")).read()
    src = open(os.path.join(ROOT, "vptq_amd", "batched_decode.py")).read()
    assert re.findall(r"VPTQ_GEMM_GATHERX\b[^=]", src.replace("VPTQ_GEMM_GATHERX=1 / 0", "")) == ['VPTQ_GEMM_GATHERX"']   # read once ...
    assert '_GEMM_GATHERX_MODE = (B.tune_env("VPTQ_GEMM_GATHERX", "auto") or "auto").strip().lower()' in src              # ... like this
    monkeypatch.setenv("VPTQ_GEMM_GATHERX", "1")
    monkeypatch.delenv("VPTQ_TUNING", raising=False)
    assert B.tune_env("VPTQ_GEMM_GATHERX", "auto") == "auto"
    monkeypatch.setenv("VPTQ_TUNING", "1")
    assert B.tune_env("VPTQ_GEMM_GATHERX", "auto") == "1"
