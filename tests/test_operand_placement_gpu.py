"""Every kernel entry under hostile operand placement (tests/_arena.py): the same call must give the same bits whatever surrounds its
operands and down to the least alignment its kernel accepts, and must write nothing outside y and its workspace.

One table, one row per (entry, kernel family, edge).  A row runs its call under three placements, ONE launch each (one more with
VPTQ_GEMV_OUT_F32 where the entry has an fp32 output), and asserts the instance string the library gives for each placement first:

  A  benign     every operand in an arena of zero bytes, 256-byte aligned.  Anchors the row to the REFERENCE: the outputs meet the
                row's float64 model (tests/_arith_model.py, bounds unchanged) or, for vptq_dequant / vptq_dequant_sliced / repack / the
                layout build, equal the oracle's / the packed stream's / the recipe's bytes.  Guards intact.
  B  hostile    quiet NaN around every floating-point operand, 0xFF bytes around every integer one, same offsets: the outputs are
                A's BIT FOR BIT; the input arenas and the guards of y and of the workspace are intact.
  C  hostile, least aligned   every operand `a` bytes past a 256-byte boundary, a = the least alignment that keeps the row's kernel
                (ALIGN below, from include/vptq_hip.h): aligned to that and not to twice that.  Same instance as A: same bits.
     "entry" rows put every operand at the least alignment the ENTRY accepts instead (tables 4 bytes, everything else its element
                size): the call leaves the fast kernels for the documented fallback, which the row names (`fallback`) and whose model
                (the reference's roundings) the outputs must meet.  The instance queries take no x: a row of this kind is also the
                one whose x is 2-byte aligned.

No tolerance anywhere: bit identity is a condition.  NOT_BIT_DETERMINISTIC names the rows whose route is not run-to-run identical
under ONE placement - they would be held to the model under all three placements instead; it is empty (fixed summation orders,
integer fixed-point atomics in the sliced family).

Out of reach (tests/_arena.py): scale_permuted, bias_permuted and inv_perm, which the library's Python side derives and owns."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _arena as ar
import _arith_model as am
import _chain_rows_run as rows
import test_route_models_gpu as rm
import test_route_models_k256_gpu as k256
import test_route_models_other_gpu as other
import test_route_models_sliced_gpu as sliced
import test_gemm_gather_gpu as gg
import test_gemm_gatherx_gpu as gx
import test_gemm_k256w_gpu as kw
import test_layout_build_gpu as lb
from test_route_models_gpu import EXACT, MFMA, VALU, F32, BATCHED, SEL, _np
from oracle import vptq_oracle as vo
from _gpu_util import spec_to_module, bits_to_tensor, tensor_to_bits, module_desc, v2_desc

pytestmark = pytest.mark.gpu
dev = rm.dev

NOT_BIT_DETERMINISTIC = {}   # row id -> reason; such a row is held to its model under B and C instead of to A's bits

# ---------------------------------------------------------------------------------------------- least alignments (include/vptq_hip.h)
EL = 0   # the element's own size (2 bytes for 16-bit tensors, 4 for float32 / int32, 1 for uint8)
_K256 = dict(indices=16, centroids=16, res_centroids=16, weight_scale=16, weight_bias=16, perm=16, bias=EL, x=16, y=EL, ws=16)
_GATHER = dict(indices=16, centroids=16, res_centroids=16, weight_scale=4, weight_bias=4, perm=4, bias=EL, x=4, y=EL, ws=16)
ALIGN = {
    # vptq_quant_gemv, by the kernel a row is about
    "k256": _K256, "gather": _GATHER,
    "k256t": dict(_K256, x=EL),   # gemm_k256t: its pre-pass reads x element by element where x is not 16-byte aligned
    "lds": dict(indices=4, centroids=16, res_centroids=16, weight_scale=16, weight_bias=16, perm=16, bias=EL, x=16, y=EL, ws=16),
    "gatherx": dict(indices=4, centroids=lambda e: _entry_align(e["v"]), res_centroids=lambda e: _entry_align(e["v"]),
                    outlier_centroids=lambda e: _entry_align(e["ov"]), outlier_indices=2, weight_scale=4, weight_bias=4, perm=4, bias=EL,
                    x=4, y=EL, ws=16),
    "generic": dict(indices=4, centroids=4, res_centroids=4, outlier_centroids=EL, outlier_indices=2, weight_scale=EL, weight_bias=EL,
                    perm=EL, bias=EL, x=EL, y=EL, ws=16),
    # vptq_quant_gemv_v2: the LDS-resident kernels / gemv_v2
    "v2lds": dict(ids=16, cent=16, rcent=16, rids=8, scale=16, sbias=16, bias=EL, x=16, y=EL),
    "v2": dict(ids=EL, cent=EL, rcent=EL, rids=EL, scale=EL, sbias=EL, bias=EL, x=EL, y=EL),
    # the chain launch: gemv_k256's rules, x 4 bytes - so a dependent list's y, which is the next layer's x, 4 bytes too (a list that
    # misses that goes layer by layer) -, the workspace by its kind
    "chain": dict(_K256, x=4, ws=256), "chain_dep": dict(_K256, x=4, y=4, ws=4),
    # ... a dependent list that misses it: the descriptors by gemv_k256's rule, x[0] and every y[i] = x[i + 1] element-aligned
    "chain_dep_min": dict(_K256, x=EL, y=EL, ws=4),
    # the sliced entries: descriptor tensors, layout tensors, x, y, workspace (selective: 256)
    "sliced": dict(indices=4, centroids=16, res_centroids=16, weight_scale=16, weight_bias=16, perm=16, bias=EL, x=16, y=EL, ws=16,
                   elems=4, blocks=4, first=4, res=2, wstart=4),
    # ... a FOLDED layout's uint8 res (v = 8 with 256 residual centroids): any address
    "sliced_res1": dict(indices=4, centroids=16, res_centroids=16, weight_scale=16, weight_bias=16, perm=16, bias=EL, x=16, y=EL, ws=16,
                        elems=4, blocks=4, first=4, res=1, wstart=4),
    # the batched-decode entries and the fused GEMM
    "gemm_gather": dict(_GATHER, x=16), "gemm_gatherx": dict(_GATHER, x=16), "gemm_gatherw": dict(_GATHER, x=16),
    "gemm_k256w": _K256, "gemm": _K256,
    # dense W and the layout tools
    "dequant": dict(indices=16, centroids=4, res_centroids=4, outlier_centroids=EL, outlier_indices=2, weight_scale=16, weight_bias=16,
                    perm=EL, W=16),
    "dequant_min": dict(indices=4, centroids=4, res_centroids=4, outlier_centroids=EL, outlier_indices=2, weight_scale=EL, weight_bias=EL,
                        perm=EL, W=EL),
    # (their descriptor is validated like the sliced entries': the layer must have its exact layouts at these pointers)
    "dequant_sliced": dict(indices=4, centroids=16, res_centroids=16, weight_scale=16, weight_bias=16, perm=16, W=16, elems=16, blocks=4,
                           first=4, res=8, wstart=4),
    "repack": dict(indices=4, centroids=16, res_centroids=16, weight_scale=16, weight_bias=16, perm=16, out=16, elems=16, blocks=4, first=4,
                   res=8, wstart=4),
    "layout": dict(indices=4, blocks=4, first=4, wstart=4, total=8, elems=16, res=4),
}


def _entry_align(v):
    """gemv_gatherx: the largest power of two that divides a codebook entry of 2 v bytes, at most 16"""
    return 16 if v in (8, 16) else 8 if v in (4, 12) else 4


class Placement:
    def __init__(self, name, fill, least, table=None):
        self.name, self.fill, self.least, self.table = name, fill, least, table

    def off(self, e, operand, es):
        """the byte offset of an operand of row e with elements of es bytes"""
        if not self.least:
            return 0
        a = ALIGN[self.table or e["align"]].get(operand, EL)
        return (a(e) if callable(a) else a) or es


PL_A, PL_B = Placement("A", ar.BENIGN, False), Placement("B", ar.HOSTILE, False)
PL_C = Placement("C", ar.HOSTILE, True)


def placement_c(e):
    return Placement("C", ar.HOSTILE, True, e["entry_min"]) if e.get("entry_min") else PL_C


class Run:
    """what one placement of a row gave: the instance string, the outputs (device tensors), the input arenas, the guards of y / workspace"""

    def __init__(self, instance):
        self.instance, self.outs, self.inputs, self.guards = instance, [], [], []


_ES = dict(indices=4, perm=2, outlier_indices=2)


def _place_module(e, m, pl, run):
    offs = {name: pl.off(e, name, _ES.get(name, 2)) for name in ar._module_params(m)}
    run.inputs += [(name, a) for name, a in ar.place_module(m, pl.fill, offs).items()]


def _place_x(e, x, dt, tokens, I, dev, pl, run):
    xt, a = ar.place(bits_to_tensor(x, dt, dev).reshape(tokens, I), pl.fill, pl.off(e, "x", 2))
    run.inputs.append(("x", a))
    return xt


def _out(e, shape, dtype, dev, pl, run, name="y", fill=None):
    """a NaN-prefilled output between margins of the finite sentinel - or, fill given (an output that a later layer of the same launch
    READS: a dependent chain's y[i] = x[i + 1]), of the placement's own fill, so that an over-read past it shows like one past x"""
    off = pl.off(e, name, torch.empty(0, dtype=dtype).element_size())
    if fill is None:
        y, a = ar.guarded_out(shape, dtype, dev, off)
    else:
        y, a = ar.place(torch.full(tuple(shape), float("nan"), dtype=dtype, device=dev), fill, off)
    run.guards.append((name, a))
    return y


def _ws(e, nbytes, zeroed, dev, pl, run):
    """(pointer, bytes) of a guarded workspace of exactly nbytes at the least alignment the entry asks for (every placement: the header
    asks for no more), or (None, 0)"""
    if not nbytes:
        return None, 0, None
    ws, a = ar.guarded_workspace(int(nbytes), zeroed, dev, align=ALIGN[e["align"]]["ws"])
    run.guards.append(("workspace", a))
    return ws.data_ptr(), int(nbytes), ws


def _text(fn, *args):
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(8192)
    B.check(fn(*args, buf, len(buf)), "instance query")
    return buf.value.decode()


def _sync_clone(run, ys):
    torch.cuda.synchronize()
    run.outs += [y.clone() for y in ys]


# ---------------------------------------------------------------------------------------------- the rows' layers (computed once, never written)
@functools.lru_cache(maxsize=8)
def _case(key):
    """(L, pieces, x bits, hot blocks) of a packed row"""
    e = ROW_BY_ID[key]
    L = e["layer"]()
    x, hot = e["x"](L)
    return L, am.pieces(L), x, hot


# ---------------------------------------------------------------------------------------------- runners: one per entry
def run_gemv(e, dev, pl):
    """vptq_quant_gemv"""
    from vptq_amd import _backend as B
    L, P, x, hot = _case(e["id"])
    m = spec_to_module(L, dev)
    run = Run(None)
    _place_module(e, m, pl, run)
    desc, keep = module_desc(m)
    T = e["tokens"]
    run.instance = _text(B.lib().vptq_quant_gemv_instance, desc, T, e["flags"])
    xt = _place_x(e, x, L.dtype, T, L.in_features, dev, pl, run)
    for f32 in (False, True):
        y = _out(e, (T, L.out_features), torch.float32 if f32 else xt.dtype, dev, pl, run)
        wp, wb, _ = _ws(e, B.lib().vptq_quant_gemv_workspace_bytes(desc, T, e["flags"]), False, dev, pl, run)
        B.check(B.lib().vptq_quant_gemv(desc, xt.data_ptr(), y.data_ptr(), T, e["flags"] | (F32 if f32 else 0), wp, wb,
                                        B.current_stream_ptr(dev)), "vptq_quant_gemv")
        _sync_clone(run, [y])
    run.keep = (m, keep)
    return run


@functools.lru_cache(maxsize=4)
def _v2_case(key):
    e = ROW_BY_ID[key]
    t = other.v2_tensors(e)
    x, hot = other.x_of(e)
    return t, other.v2_pieces(e, t), x, hot


_V2_FLOAT = ("cent", "rcent", "scale", "sbias", "bias")


def run_v2(e, dev, pl):
    """vptq_quant_gemv_v2"""
    from vptq_amd import _backend as B
    t, P, x, hot = _v2_case(e["id"])
    dt = e["dt"]
    run = Run(None)
    td = {}
    for key, val in t.items():
        if not isinstance(val, np.ndarray):
            td[key] = val
            continue
        dv = bits_to_tensor(val, dt, dev).reshape(val.shape) if key in _V2_FLOAT else \
            torch.from_numpy(val.view(np.int16) if val.dtype == np.uint16 else val).to(dev)
        td[key], a = ar.place(dv, pl.fill, pl.off(e, key, dv.element_size()))
        run.inputs.append((key, a))
    desc, keep = v2_desc(td, dt)
    T = e["tokens"]
    run.instance = _text(B.lib().vptq_quant_gemv_v2_instance, desc, T, e["flags"])
    xt = _place_x(e, x, dt, T, e["I"], dev, pl, run)
    for f32 in (False, True):
        y = _out(e, (T, e["O"]), torch.float32 if f32 else xt.dtype, dev, pl, run)
        B.check(B.lib().vptq_quant_gemv_v2(desc, xt.data_ptr(), y.data_ptr(), T, e["flags"] | (F32 if f32 else 0),
                                           B.current_stream_ptr(dev)), "vptq_quant_gemv_v2")
        _sync_clone(run, [y])
    run.keep = keep
    return run


@functools.lru_cache(maxsize=2)
def _list_case(key):
    """[(L, pieces, x bits, hot)] of a grouped / chain row"""
    e = ROW_BY_ID[key]
    out = []
    for i, (I, O, perm, bias) in enumerate(e["shapes"]):
        L = vo.make_layer(I, O, dist="llm", seed=I + O + i, dtype=e["dt"], enable_perm=bool(perm), bias=bool(bias))
        ee = dict(arith=e["arith"], tokens=e["tokens"])
        x, hot = k256._x_for(L, ee, 40 + i)
        out.append((L, am.pieces(L), x, hot))
    return out


def _list_operands(e, dev, pl, run):
    from vptq_amd import _backend as B
    cases = _list_case(e["id"])
    ms = [spec_to_module(L, dev) for L, _, _, _ in cases]
    for m in ms:
        _place_module(e, m, pl, run)
    keep = [module_desc(m) for m in ms]
    descs = (B.LayerDesc * len(ms))(*[k[0] for k in keep])
    return cases, ms, keep, descs


def run_grouped(e, dev, pl):
    """vptq_quant_gemv_grouped"""
    from vptq_amd import _backend as B
    run = Run(None)
    cases, ms, keep, descs = _list_operands(e, dev, pl, run)
    n, T = len(ms), e["tokens"]
    name = B.lib().vptq_quant_gemv_grouped_kernel_name(descs, n, T, e["flags"])
    run.route_name = None if name is None else name.decode()
    run.instance = _text(B.lib().vptq_quant_gemv_grouped_instance, descs, n, T, e["flags"])
    xts = [_place_x(e, x, e["dt"], T, L.in_features, dev, pl, run) for L, _, x, _ in cases]
    for f32 in (False, True):
        ys = [_out(e, (T, L.out_features), torch.float32 if f32 else xts[0].dtype, dev, pl, run, "y") for L, _, _, _ in cases]
        xp = (C.c_void_p * n)(*[t.data_ptr() for t in xts])
        yp = (C.c_void_p * n)(*[y.data_ptr() for y in ys])
        B.check(B.lib().vptq_quant_gemv_grouped(descs, n, xp, yp, T, e["flags"] | (F32 if f32 else 0), B.current_stream_ptr(dev)),
                "vptq_quant_gemv_grouped")
        _sync_clone(run, ys)
    run.keep = (ms, keep)
    return run


def run_chain(e, dev, pl):
    """vptq_quant_gemv_chain: independent lists (exact / folded / selective; a list with permutations and the selective form need the
    256-byte aligned workspace vptq_quant_gemv_chain_workspace_bytes_for asks for, contents don't matter) and dependent lists (x[i + 1]
    = y[i]; vptq_quant_gemv_chain_workspace_bytes(n, flags) bytes, 4-byte aligned, cleared by the call).  A dependent list's y[i] sit
    between margins of the placement's fill (NaN under B and C): they are the next layer's x.
    A limit of these rows: the instance and kernel-name queries see the descriptors only.  Whether the CALL stayed in gemv_k256c with
    this x and this workspace is held indirectly: the rows keep x and the workspace at the rule the header states for the persistent
    launch, and the rows that break it (entry-min) must meet ANOTHER arithmetic's model - the reference's roundings of the per-layer
    kernels where A is folded."""
    from vptq_amd import _backend as B
    run = Run(None)
    cases, ms, keep, descs = _list_operands(e, dev, pl, run)
    n, flags, dep = len(ms), e["flags"], bool(e["flags"] & B.GEMV_CHAIN_DEPENDENT)
    name = B.lib().vptq_quant_gemv_chain_kernel_name(descs, n, 1, flags)
    run.route_name = None if name is None else name.decode()
    run.instance = _text(B.lib().vptq_quant_gemv_chain_instance, descs, n, 1, flags)
    x0 = _place_x(e, cases[0][2], e["dt"], 1, cases[0][0].in_features, dev, pl, run)
    xts = [x0] if dep else [x0] + [_place_x(e, x, e["dt"], 1, L.in_features, dev, pl, run) for L, _, x, _ in cases[1:]]
    for f32 in ((False,) if dep else (False, True)):
        ys = [_out(e, (1, L.out_features), torch.float32 if f32 else x0.dtype, dev, pl, run, fill=pl.fill if dep else None)
              for L, _, _, _ in cases]
        nb = B.lib().vptq_quant_gemv_chain_workspace_bytes(n, flags) if dep else B.lib().vptq_quant_gemv_chain_workspace_bytes_for(descs, n, flags)
        wp, wb, _ = _ws(e, nb, False, dev, pl, run)
        xin = [x0] + ys[:-1] if dep else xts
        xp = (C.c_void_p * n)(*[t.data_ptr() for t in xin])
        yp = (C.c_void_p * n)(*[y.data_ptr() for y in ys])
        B.check(B.lib().vptq_quant_gemv_chain(descs, n, xp, yp, 1, flags | (F32 if f32 else 0), wp, wb, B.current_stream_ptr(dev)),
                "vptq_quant_gemv_chain")
        _sync_clone(run, ys)
    run.keep = (ms, keep)
    return run


@functools.lru_cache(maxsize=4)
def _sliced_case(key):
    e = ROW_BY_ID[key]
    Ls = [sliced._layer(e["I"], O, e["dt"], e["v"], e["k"], e["kr"], e["perm"], e["bias"]) for O in e["Os"]]
    L0 = Ls[0][0]
    x, hot = (rm._dense(e["I"], e["tokens"], e["dt"], e["I"] + e["tokens"]) if e["mode"] == "exact" else
              rm._planted(e["I"], e["tokens"], e["dt"], e["I"] + e["tokens"], perm=L0.perm))
    return Ls, x, hot


def _layout_offsets(e, sl, pl):
    """the byte offset of every layout tensor of a SlicedGemv (res: by its own element size, uint8 or uint16)"""
    res = sl._tensors[0][3]
    return {name: pl.off(e, name, res.element_size() if name == "res" and res is not None else 4) for name in ar.LAYOUT_OPERANDS}


def _sliced_objects(e, dev, pl, run):
    """the row's SlicedGemv objects over PLACED parameters and PLACED layout tensors (and, for several members or the grouped entry,
    their SlicedGroupGemv)"""
    from vptq_amd.utils.sliced import SlicedGemv, SlicedGroupGemv
    Ls, x, hot = _sliced_case(e["id"])
    sls = []
    for L, _ in Ls:
        m = spec_to_module(L, dev)
        _place_module(e, m, pl, run)
        sl = SlicedGemv(m, rows_per_wave=e["rpw"], exact=e["mode"] == "exact", selective=e["mode"] == "sel")
        run.inputs += [("layout", a) for a in ar.place_layouts(sl, pl.fill, _layout_offsets(e, sl, pl))]
        sls.append(sl)
    grouped = len(sls) > 1 or e["entry"] == "grouped"
    return Ls, x, hot, sls, (SlicedGroupGemv(sls) if grouped else None)


def run_sliced(e, dev, pl):
    """vptq_quant_gemv_sliced / _tokens / _grouped / _tokens_grouped (column parts: the grouped entries with VPTQ_GEMV_COLUMN_PARTS).
    Workspaces: exactly the bytes the entry's query returns, zero-filled (the header: zero-filled once), 16-byte aligned - the
    selective launch 256 - and, after a one-token call, zero again (the header: every call leaves the workspace zero)"""
    from vptq_amd import _backend as B
    run = Run(None)
    Ls, x, hot, sls, g = _sliced_objects(e, dev, pl, run)
    sl, T, flags = sls[0], e["tokens"], sliced.MODE_FLAGS[e["mode"]]
    lib = B.lib()
    assert (sl.parts > 1) == (e["entry"] == "parts")
    if sl.parts > 1:
        descs, lays, n, iflags = sl._part_descs, sl._lay_ref, sl.parts, flags | sliced.PARTS
    elif g is not None:
        descs, lays, n, iflags = g.descs, g.layouts, len(sls), flags
    else:
        descs, lays, n, iflags = (B.LayerDesc * 1)(sl.desc), sl._lay_ref, 1, flags
    run.instance = sliced.sliced_instance_of(descs, lays, n, T, iflags)
    xt = _place_x(e, x, e["dt"], T, e["I"], dev, pl, run)
    sp = B.current_stream_ptr(dev)
    members = sls if sl.parts == 1 else [sl]
    for f32 in (False, True):
        ys = [_out(e, (T, m.layer.out_features), torch.float32 if f32 else xt.dtype, dev, pl, run) for m in members]
        wss = []
        for m in members:
            wd = m._part_descs[0] if m.parts > 1 else m.desc
            nb = (lib.vptq_quant_gemv_sliced_workspace_bytes_for(m.desc, flags) if e["mode"] == "sel" else
                  lib.vptq_quant_gemv_sliced_workspace_bytes(wd)) if T == 1 else lib.vptq_quant_gemv_sliced_tokens_workspace_bytes(wd, T)
            assert nb > 0
            wss.append(_ws(dict(e, align="sliced_sel" if e["mode"] == "sel" else e["align"]), nb, True, dev, pl, run))
        fl = iflags | (F32 if f32 else 0)
        if n == 1 and g is None:
            rc = (lib.vptq_quant_gemv_sliced(sl.desc, lays, xt.data_ptr(), ys[0].data_ptr(), fl, wss[0][0], wss[0][1], sp) if T == 1 else
                  lib.vptq_quant_gemv_sliced_tokens(sl.desc, lays, xt.data_ptr(), ys[0].data_ptr(), T, fl, wss[0][0], wss[0][1], sp))
        else:
            k = 1 if sl.parts > 1 else len(members)
            yp = (C.c_void_p * n)(*[ys[i % k].data_ptr() for i in range(n)])
            wp = (C.c_void_p * n)(*[wss[i % k][0] for i in range(n)])
            wb = (C.c_size_t * n)(*[wss[i % k][1] for i in range(n)])
            rc = (lib.vptq_quant_gemv_sliced_grouped(descs, lays, n, xt.data_ptr(), yp, fl, wp, wb, sp) if T == 1 else
                  lib.vptq_quant_gemv_sliced_tokens_grouped(descs, lays, n, xt.data_ptr(), yp, T, fl, wp, wb, sp))
        B.check(rc, "sliced call")
        _sync_clone(run, ys)
        if T == 1 and e["mode"] != "sel":
            for _, _, ws in wss:
                assert not bool(ws.any()), f"{e['id']} placement {pl.name}: the call left its workspace non-zero"
    run.keep = (sls, g)
    return run


ALIGN["sliced_sel"] = dict(ALIGN["sliced"], ws=256)


@functools.lru_cache(maxsize=4)
def _bd_case(key):
    e = ROW_BY_ID[key]
    L = e["layer"]()
    kind = rm._dense if e["xkind"] == "dense" else rm._planted
    x = kind(L.in_features, e["tokens"], L.dtype, L.in_features + e["tokens"], **(dict(perm=L.perm) if e["xkind"] == "planted" else {}))
    return L, am.pieces(L), x[0], x[1]


def run_bd(e, dev, pl):
    """vptq_quant_gemm_gather / _gatherx / _gatherw / _k256w (no workspace) and vptq_quant_gemm (bf16: its workspace, no fp32 output)"""
    from vptq_amd import _backend as B
    L, P, x, hot = _bd_case(e["id"])
    m = spec_to_module(L, dev)
    run = Run(None)
    _place_module(e, m, pl, run)
    desc, keep = module_desc(m)
    T, lib, name = e["tokens"], B.lib(), e["entry"]
    xt = _place_x(e, x, L.dtype, T, L.in_features, dev, pl, run)
    sp = B.current_stream_ptr(dev)
    if name == "vptq_quant_gemm":
        assert lib.vptq_quant_gemm_supported(desc) == 1
        run.instance = "vptq_quant_gemm dt=" + L.dtype    # (the entry has no instance query: one fused kernel per dtype)
        y = _out(e, (T, L.out_features), xt.dtype, dev, pl, run)
        wp, wb, _ = _ws(e, lib.vptq_quant_gemm_workspace_bytes(desc, T), False, dev, pl, run)
        B.check(lib.vptq_quant_gemm(desc, xt.data_ptr(), y.data_ptr(), T, 0, wp, wb, sp), name)
        _sync_clone(run, [y])
    else:
        assert getattr(lib, name + "_supported")(desc, T) == 1
        run.instance = _text(getattr(lib, name + "_instance"), desc, T, 0)
        for f32 in (False, True):
            y = _out(e, (T, L.out_features), torch.float32 if f32 else xt.dtype, dev, pl, run)
            B.check(getattr(lib, name)(desc, xt.data_ptr(), y.data_ptr(), T, F32 if f32 else 0, sp), name)
            _sync_clone(run, [y])
    run.keep = (m, keep)
    return run


@functools.lru_cache(maxsize=4)
def _dq_case(key):
    e = ROW_BY_ID[key]
    L = e["layer"]()
    with np.errstate(all="ignore"):
        W = vo.dequant(L, ref_residual_mask_quirk=False)
    return L, np.ascontiguousarray(W).view(np.uint16).reshape(L.out_features, L.in_features)


def run_dequant(e, dev, pl):
    """vptq_dequant"""
    from vptq_amd import _backend as B
    L, want = _dq_case(e["id"])
    m = spec_to_module(L, dev)
    run = Run(None)
    _place_module(e, m, pl, run)
    desc, keep = module_desc(m, need_inv_perm=True)
    W = _out(e, (L.out_features, L.in_features), bits_to_tensor(np.zeros(1, np.uint16), L.dtype, dev).dtype, dev, pl, run, "W")
    run.instance = _text(B.lib().vptq_dequant_instance, desc, W.data_ptr())
    B.check(B.lib().vptq_dequant(desc, W.data_ptr(), B.current_stream_ptr(dev)), "vptq_dequant")
    _sync_clone(run, [W])
    run.keep = (m, keep)
    return run


def _exact_layout(e, L, dev, pl, run):
    from vptq_amd.utils.sliced import SlicedGemv
    m = spec_to_module(L, dev)
    _place_module(e, m, pl, run)
    sl = SlicedGemv(m, exact=True)
    run.inputs += [("layout", a) for a in ar.place_layouts(sl, pl.fill, _layout_offsets(e, sl, pl))]
    return m, sl


def run_dequant_sliced(e, dev, pl):
    """vptq_dequant_sliced: W from the exact layout(s)"""
    from vptq_amd import _backend as B
    L, want = _dq_case(e["id"])
    run = Run(None)
    m, sl = _exact_layout(e, L, dev, pl, run)
    run.instance = f"dequant_sliced dt={L.dtype} v={L.vector_len} nsl={sl.slices} parts={sl.parts} side={2 if sl._side16 else int(sl.res is not None)}"
    W = _out(e, (L.out_features, L.in_features), sl._dtype, dev, pl, run, "W")
    B.check(B.lib().vptq_dequant_sliced(sl.desc, sl._lay_ref, sl.parts, W.data_ptr(), B.current_stream_ptr(dev)), "vptq_dequant_sliced")
    _sync_clone(run, [W])
    run.keep = (m, sl)
    return run


def run_repack(e, dev, pl):
    """vptq_sliced_layout_repack: the packed stream from the exact layout(s)"""
    from vptq_amd import _backend as B
    L, _ = _dq_case(e["id"])
    run = Run(None)
    m, sl = _exact_layout(e, L, dev, pl, run)
    run.instance = f"sliced_layout_repack v={L.vector_len} nsl={sl.slices} parts={sl.parts} side={2 if sl._side16 else int(sl.res is not None)}"
    shape = (1, int(sl.desc.num_indices), int(sl.desc.row_words))
    out, a = ar.place(torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device=dev), ar.HOSTILE, pl.off(e, "out", 4))
    run.guards.append(("indices_out", a))
    B.check(B.lib().vptq_sliced_layout_repack(sl.desc, sl._lay_ref, sl.parts, out.data_ptr(), B.current_stream_ptr(dev)), "vptq_sliced_layout_repack")
    _sync_clone(run, [out])
    run.keep = (m, sl)
    return run


@functools.lru_cache(maxsize=4)
def _layout_case(key):
    e = ROW_BY_ID[key]
    return lb._inputs(e["N"], e["G"], e["ib"], e["rb"], seed=e["ib"] * 100 + e["rb"] + e["G"] + e["N"])


def run_layout(e, dev, pl):
    """vptq_sliced_layout_plan + vptq_sliced_layout_fill (one device -> host read between them, as the header describes): every
    output tensor guarded, the packed indices placed"""
    from vptq_amd import _backend as B
    idx, ridx, packed = _layout_case(e["id"])
    run = Run(None)
    pk, a = ar.place(packed.to(dev), pl.fill, pl.off(e, "indices", 4))
    run.inputs.append(("indices", a))
    N, S, sb = e["N"], e["slices"], e["side"]
    d = lb._desc(pk, e["G"], e["ib"], e["rb"], N)
    spec = B.SlicedLayoutSpec(B.LAYOUT_ANY_SHAPE, S, 0, 0, sb, 1, 0, 0)
    run.instance = f"sliced_layout_build nsl={S} side={sb} G={e['G']} N={N}"

    def out(shape, dtype, name):
        t, g = ar.place(torch.full(shape, 0x5A, dtype=dtype, device=dev), ar.HOSTILE, pl.off(e, name, torch.empty(0, dtype=dtype).element_size()))
        run.guards.append((name, g))
        return t
    blocks, first, wstart = out((S, N), torch.int32, "blocks"), out((S, N), torch.int32, "first"), out((S, N, 5), torch.int32, "wstart")
    total = out((1,), torch.int64, "total")
    sp = B.current_stream_ptr(dev)
    B.check(B.lib().vptq_sliced_layout_plan(d, spec, blocks.data_ptr(), first.data_ptr(), wstart.data_ptr(), total.data_ptr(), sp), "plan")
    nblk = int(total.item())
    elems = out((max(nblk, 1) * 64,), torch.int32, "elems")
    res = out((elems.numel(),), torch.uint8 if sb == 1 else torch.int16, "res") if sb else None
    lay = B.SlicedLayout(elems.data_ptr(), blocks.data_ptr(), first.data_ptr(), res.data_ptr() if sb else None, 1, 1, S, 0, wstart.data_ptr())
    B.check(B.lib().vptq_sliced_layout_fill(d, spec, lay, nblk, sp), "fill")
    torch.cuda.synchronize()
    run.outs = [None if t is None else t.clone() for t in (elems, blocks, first, res, wstart)]
    return run


RUNNERS = dict(gemv=run_gemv, v2=run_v2, grouped=run_grouped, chain=run_chain, sliced=run_sliced, bd=run_bd, dequant=run_dequant,
               dequant_sliced=run_dequant_sliced, repack=run_repack, layout=run_layout)


# ---------------------------------------------------------------------------------------------- placement A against the reference
def check_reference(e, run, monkeypatch, arith=None, what=""):
    """the outputs of a run against the row's float64 model (am.check_outputs' bounds, nothing added) or the oracle's / the packed
    stream's / the recipe's bytes.  arith: another route's model (a fallback), else the row's own."""
    kind = e["kind"]
    ee = dict(arith=arith or e["arith"], rounded=e.get("rounded", False) and not arith, round_sx=e.get("round_sx", True) or bool(arith)) \
        if "arith" in e else None
    if kind == "gemv":
        L, P, x, hot = _case(e["id"])
        rm._check(_np(run.outs[0]), _np(run.outs[1]), L, x, ee, hot, P=P, what=what)
    elif kind == "v2":
        import types
        t, P, x, hot = _v2_case(e["id"])
        rm._check(_np(run.outs[0]), _np(run.outs[1]), types.SimpleNamespace(in_features=e["I"], perm=None, dtype=e["dt"]), x, ee, hot, P=P, what=what)
    elif kind in ("grouped", "chain"):
        cases = _list_case(e["id"])
        n = len(cases)
        y32 = run.outs[n:] if len(run.outs) > n else [None] * n
        xin = None
        for i, (L, P, x, hot) in enumerate(cases):
            dep = kind == "chain" and len(run.outs) == n
            xi, hi = (x, hot) if not dep or i == 0 else (xin, ())
            y16 = vo.to_f32(tensor_to_bits(run.outs[i]), L.dtype).astype(np.float64) if dep else _np(run.outs[i])
            rm._check(y16, None if y32[i] is None else _np(y32[i]), L, xi, ee, hi, P=P, what=f"{what} layer {i}")
            xin = tensor_to_bits(run.outs[i])
    elif kind == "sliced":
        Ls, x, hot = _sliced_case(e["id"])
        last = run.instance.split(" | ")[-1]
        f = dict(p.split("=") for p in last.split()[1:])
        extra = am.sliced_extra_abs(e["dt"], int(f["arrivals"])) if last.split()[0] == "gemv_sliced" else 0.0
        k = len(run.outs) // 2
        for i in range(k):
            L, P = Ls[i]
            rm._check(_np(run.outs[i]), _np(run.outs[k + i]), L, x, ee, hot, extra, P, what=f"{what} member {i}")
    elif kind == "bd":
        L, P, x, hot = _bd_case(e["id"])
        rm._check(_np(run.outs[0]), _np(run.outs[1]) if len(run.outs) > 1 else None, L, x, ee, hot, P=P, what=what)
    elif kind in ("dequant", "dequant_sliced"):
        L, want = _dq_case(e["id"])
        got = tensor_to_bits(run.outs[0]).reshape(want.shape)
        bad = got != want
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ from the oracle's, first at {np.argwhere(bad)[:4].tolist()}"
    elif kind == "repack":
        L, _ = _dq_case(e["id"])
        want = np.ascontiguousarray(L.indices).view(np.int32).reshape(run.outs[0].shape)
        assert np.array_equal(run.outs[0].cpu().numpy(), want), f"{what}: not the packed stream the layout was built from"
    elif kind == "layout":
        idx, ridx, packed = _layout_case(e["id"])
        lb._check(monkeypatch, run.outs, idx, e["slices"], ridx if e["side"] else None, e["ib"],
                  side_dtype=torch.uint8 if e["side"] < 2 else torch.int16)
    else:
        raise ValueError(kind)


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _assert_intact(e, run, pl):
    for name, a in run.inputs:
        assert a.intact(), f"{e['id']} placement {pl.name}: the arena of input `{name}` was written: {a.damage()}"
    for name, a in run.guards:
        assert a.intact(), f"{e['id']} placement {pl.name}: a store outside `{name}`: {a.damage()}"


# ---------------------------------------------------------------------------------------------- the table
TABLE = []


def _row(e, id):
    e["id"] = id
    TABLE.append(e)


def _from_census(params, pred, cap, keyf):
    """rows of a census table that meet pred, at most `cap` per key, in table order"""
    seen, out = {}, []
    for p in params:
        e = p.values[0]
        if pred(e) and seen.get(keyf(e), 0) < cap:
            seen[keyf(e)] = seen.get(keyf(e), 0) + 1
            out.append((e, p.id))
    return out


_FAMILY_ALIGN = dict(gemv_k256="k256", gemv_k256m="k256", gemm_k256="k256", gemm_k256t="k256", gemv_gather="gather", gemv_lds="lds",
                     gemv_lds_mfma="lds", gemv_gatherx="gatherx", gemv_generic="generic")


def _ragged(I):
    return I % 2048 != 0


# vptq_quant_gemv, canonical format: the ragged rows of K256_ONE_LAYER (2040 / 4104 / 8200 / 6136 / 2056 columns; O = 264, 136: a last
# row group short of rows), every form, 1 - 16 tokens, with and without perm and bias: per kernel, dtype and token count one row with
# and one without a permutation - gemv_k256m: one per sweep count (2040, 4104, 8200 columns)
for _e, _id in _from_census(k256.K256_ONE_LAYER, lambda e: e["layer"][1] <= 264 and _ragged(e["layer"][0]) and e["layer"][0] <= 8200, 1,
                            lambda e: (e["route"], e["dt"], e["tokens"] if e["tokens"] <= 4 else 5 if e["tokens"] < 16 else 16,
                                       e["layer"][0] if "k256m" in e["route"] else bool(e["layer"][2].get("enable_perm")))):
    _row(dict(kind="gemv", align="k256t" if _e["route"] == k256.KT else "k256", layer=functools.partial(rm._layer, _e),
              x=lambda L, e=_e: k256._x_for(L, e, L.in_features + e["tokens"]),
              **{k: v for k, v in _e.items() if k not in ("layer", "route")}), "gemv-" + _id)
# gemm_k256t with an x that is 2-byte aligned and no more (no permutation: its pre-pass then leaves the 16-byte loads for element loads),
# a ragged last sweep (2056 columns), 5 and 16 tokens, both dtypes - the same instance and the same bits
for _dt, _tok in (("f16", 5), ("f16", 16), ("bf16", 5), ("bf16", 16)):
    _e = k256.K(k256.KT, 2056, 264, _dt, _tok, BATCHED, f"gemm_k256t dt={_dt} perm=0 tok={_tok} sweeps=2 rgs=1", bias=_tok == 5).values[0]
    _row(dict(kind="gemv", align="k256t", layer=functools.partial(rm._layer, _e), x=lambda L, e=_e: k256._x_for(L, e, L.in_features + e["tokens"]),
              **{k: v for k, v in _e.items() if k not in ("layer", "route")}), f"gemv-gemm_k256t-x2-{_dt}-2056x264-t{_tok}")
# ... one canonical row per dtype at the entry's own minimum: every operand element-aligned (tables 4 bytes), x 2 bytes -> gemv_generic
for _dt, _tok, _fl in (("f16", 1, 0), ("bf16", 3, EXACT)):
    _e = dict(layer=(2040, 100, dict(dist="llm", enable_perm=True, bias=True)), dt=_dt, tokens=_tok, flags=_fl,
              arith="exact" if _fl or _dt == "bf16" else "folded", **({} if _fl or _dt == "bf16" else rm.VALU_FOLDED))
    _row(dict(_e, kind="gemv", align="k256", layer=functools.partial(rm._layer, _e),
              x=lambda L, e=_e: k256._x_for(L, e, L.in_features + e["tokens"]),
              instance=f"gemv_k256 dt={_dt} rows=1 tok={1 if _tok == 1 else 4} sw=1 perm=1 fast={int(not _fl and _dt == 'f16')} entry={int(_tok == 1)}",
              entry_min="generic", fallback=f"gemv_generic dt={_dt} v=8 tok={1 if _tok == 1 else 4}"), f"gemv-entry-min-k256-{_dt}-t{_tok}")

# vptq_quant_gemv, every other family: the hand-chosen EDGES of the census (O = 100, 72, 40, 5, 3 ...: ragged vector-rows and short row
# groups; I = 8, 520, 1028, 1032, 4104: ragged tiles; tokens at and past the slot counts), the smallest gemv_lds_mfma rows
for _e, _id in _from_census(other.EDGES, lambda e: e["entry"] == "packed" and (e["O"] <= 264 or (e["instance"].startswith("gemv_lds_mfma") and e["I"] <= 1000)), 2,
                            lambda e: (e["instance"].split()[0], e["dt"], bool(e["perm"]), bool(e["S"]), e["C"] > 1)):
    _row(dict(_e, kind="gemv", align=_FAMILY_ALIGN[_e["instance"].split()[0]], layer=functools.partial(other.layer_of, _e),
              x=lambda L, e=_e: other.x_of(e, L.perm)), "gemv-" + _id)
# gemv_generic with outlier columns AND two codebook groups (1030 columns per group + 8 outlier columns: no multiple of 4)
for _dt in ("f16", "bf16"):
    _e = other.R(2068, 100, _dt, 3, f"gemv_generic dt={_dt} v=8 tok=4", kr=16, C=2, perm=1, bias=1, S=8, ov=4).values[0]
    _row(dict(_e, kind="gemv", align="generic", layer=functools.partial(other.layer_of, _e), x=lambda L, e=_e: other.x_of(e, L.perm)),
         f"gemv-generic-outliers-two-groups-{_dt}")
# ... the other families at the entry's minimum -> the documented fallback (gemv_gather / gemv_lds -> gemv_gatherx needs 4-byte scale
# and x: with 2-byte ones gemv_generic)
for _e, _fb in ((other.R(1032, 72, "f16", 2, "gemv_gather dt=f16 t=16 rows=1 tok=2 perm=0 wide=0", k=65536, dist='ref-test').values[0], "gemv_generic dt=f16 v=8 tok=2"),
                (other.R(520, 100, "bf16", 3, "gemv_lds dt=bf16 fmt=20 tok=2 rw=1 dma=1 perm=0", kr=256, bias=1).values[0], "gemv_generic dt=bf16 v=8 tok=4"),
                (other.R(1028, 72, "f16", 3, "gemv_gatherx dt=f16 v=8 tok=4 perm=1 reslds=0 outl=0 groups=1", k=32768, perm=1, dist='ref-test').values[0],
                 "gemv_generic dt=f16 v=8 tok=4")):
    _row(dict(_e, kind="gemv", align=_FAMILY_ALIGN[_e["instance"].split()[0]], layer=functools.partial(other.layer_of, _e),
              x=lambda L, e=_e: other.x_of(e, L.perm), entry_min="generic", fallback=_fb), "gemv-entry-min-" + _e["instance"].split()[0] + "-" + _e["dt"])

# vptq_quant_gemv_v2: gemv_v2 and the LDS-resident kernels (fmt=v2*)
for _e, _id in _from_census(other.EDGES, lambda e: e["entry"] == "v2" and (e["O"] <= 264 or e["I"] <= 264), 2,
                            lambda e: (e["instance"].split()[0], e["instance"].split()[2] if "fmt=" in e["instance"] else "", e["dt"])):
    _row(dict(_e, kind="v2", align="v2" if _e["instance"].startswith("gemv_v2") else "v2lds"), _id)
_e = other.V(520, 96, "f16", 5, "gemv_lds dt=f16 fmt=v2u8 tok=4 rw=1 dma=1 perm=0", kr=256, bias=1).values[0]
_row(dict(_e, kind="v2", align="v2lds", entry_min="v2", fallback="gemv_v2 dt=f16 v=8 tok=8"), "v2-entry-min-gemv_lds-f16")

# vptq_quant_gemv_grouped: equal shapes (the twins of the census) and mixed ones
_seen = {}
for _shapes, _dt, _tok, _fl, _route, _inst, _twin in k256.K256_GROUPS:
    _equal = len(set(_shapes)) == 1
    if not ((_equal and _shapes[0][:2] == (4104, 264)) or (not _equal and _shapes[0][0] <= 1024)) or _seen.get((_equal, _dt), 0) >= 2:
        continue
    _seen[(_equal, _dt)] = _seen.get((_equal, _dt), 0) + 1
    _row(dict(kind="grouped", align="k256", shapes=tuple((I, O, p, int(i == 0 or _equal)) for i, (I, O, p) in enumerate(_shapes)), dt=_dt,
              tokens=_tok, flags=_fl, instance=_inst, arith=k256.ARITH[_route], **(rm.VALU_FOLDED if _route == k256.KVF else {})),
         f"grouped-{'equal' if _equal else 'mixed'}-{_route}-{_dt}-{_shapes[0][0]}x{_shapes[0][1]}-p{_shapes[0][2]}-f{_fl}")

# ... at the entry's minimum (every member element-aligned, tables 4 bytes, x[i] 2 bytes): "per-layer", every member by gemv_generic
for _dt, _shapes, _tok, _fl, _inst in (
        ("f16", ((4104, 264, 1, 1), (4104, 264, 1, 1)), 1, EXACT | VALU, "gemv_k256 dt=f16 rows=1 tok=1 sw=2 perm=1 fast=0 entry=0"),
        ("bf16", ((1024, 100, 0, 1), (1024, 264, 0, 0), (1024, 72, 0, 0)), 2, EXACT, "gemv_k256 dt=bf16 ")):
    _row(dict(kind="grouped", align="k256", shapes=_shapes, dt=_dt, tokens=_tok, flags=_fl, instance=_inst, arith="exact", entry_min="generic",
              grouped_name="per-layer", fallback=" | ".join([f"gemv_generic dt={_dt} v=8 tok={_tok}"] * len(_shapes))), f"grouped-entry-min-{_dt}-n{len(_shapes)}")

# vptq_quant_gemv_chain: 10 layers (more than 8: the persistent launch), ragged sweeps, with and without perm and bias
_CHAIN = ((2040, 72, 0, 1), (4104, 100, 1, 0), (1024, 136, 0, 0), (8200, 72, 0, 1), (520, 264, 1, 0), (2056, 40, 0, 0), (264, 264, 0, 1),
          (6136, 72, 1, 0), (1032, 100, 0, 0), (520, 72, 0, 1))
_CHAIN_DEP = tuple((a, b, 0, int(i % 3 == 0)) for i, (a, b) in enumerate(zip((1024, 264, 2040, 520, 1032, 72, 4104, 136, 264, 104),
                                                                             (264, 2040, 520, 1032, 72, 4104, 136, 264, 104, 40))))
for _dt in ("f16", "bf16"):
    for _mode, _fl in (("exact", EXACT), ("folded", 0), ("selective", SEL)):
        _row(dict(kind="chain", align="chain", shapes=_CHAIN, dt=_dt, tokens=1, flags=MFMA | _fl, arith=_mode,
                  instance=f"gemv_k256c dt={_dt} dep=0 mode={_mode} layers=10 "), f"chain-independent-{_mode}-{_dt}")
    _row(dict(kind="chain", align="chain_dep", shapes=_CHAIN_DEP, dt=_dt, tokens=1, flags=MFMA | (1 << 6), arith="folded",
              instance=f"gemv_k256c dt={_dt} dep=1 mode=folded layers=10 "), f"chain-dependent-folded-{_dt}")
    # ... lists that miss the persistent launch's rule go to the grouped / per-layer calls, here down to gemv_generic (the reference's
    # roundings): an independent list with every operand at the entry's minimum; a dependent list whose descriptors keep gemv_k256's rule
    # while x[0] and every y[i] = x[i + 1] sit at 2 bytes (the queries see the descriptors only: they still name gemv_k256c)
    _row(dict(kind="chain", align="chain", shapes=_CHAIN, dt=_dt, tokens=1, flags=MFMA | EXACT, arith="exact", entry_min="generic",
              instance=f"gemv_k256c dt={_dt} dep=0 mode=exact layers=10 ", chain_name_c="grouped",
              fallback="grouped: " + " | ".join([f"gemv_generic dt={_dt} v=8 tok=1"] * 10)), f"chain-entry-min-independent-{_dt}")
    _row(dict(kind="chain", align="chain_dep", shapes=_CHAIN_DEP, dt=_dt, tokens=1, flags=MFMA | (1 << 6), arith="folded", entry_min="chain_dep_min",
              instance=f"gemv_k256c dt={_dt} dep=1 mode=folded layers=10 ", chain_name_c="gemv_k256c_kernel",
              fallback=f"gemv_k256c dt={_dt} dep=1 mode=folded layers=10 "), f"chain-entry-min-dependent-y2-{_dt}")

# ... and the launch the rule gives to the second geometry, "rows per wave" (gemv_k256r.hip): 32 narrow layers sized by the device's
# compute units (tests/_chain_rows_run.py:natural_shapes; the device-less queries answer for 256), no knob.  The fp32 launch of the
# same row is the first geometry's.  At the entry's minimum x sits at 2 bytes and the list goes to one grouped call of gemv_generic
_ROWS_CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
_CHAIN_ROWS = tuple((I, O, 0, int(b)) for I, O, b in rows.natural_shapes(_ROWS_CUS))
_row(dict(kind="chain", align="chain", shapes=_CHAIN_ROWS, dt="f16", tokens=1, flags=EXACT, arith="exact",
          instance="gemv_k256c dt=f16 dep=0 mode=exact layers=32 ", instance_suffix=" geom=rows"), "chain-rows-natural-f16")
_row(dict(kind="chain", align="chain", shapes=_CHAIN_ROWS, dt="f16", tokens=1, flags=EXACT, arith="exact", entry_min="generic",
          instance="gemv_k256c dt=f16 dep=0 mode=exact layers=32 ", instance_suffix=" geom=rows", chain_name_c="grouped",
          fallback="grouped: " + " | ".join(["gemv_generic dt=f16 v=8 tok=1"] * 32)), "chain-rows-natural-entry-min-f16")


# the sliced entries: rows of the sliced census (1000-column layers, O = 72: ragged windows, short row blocks; 14080 / 16392-column
# layers with O = 72 - 136 for window parts and column parts), every form and entry
def _sliced_key(e):
    last = e["instance"].split(" | ")[-1]
    f = dict(p.split("=") for p in last.split()[1:])
    return (last.split()[0], "|" in e["instance"], e["mode"], e["entry"] if e["entry"] != "both" else "single", f.get("rg"), f.get("two"),
            f.get("wparts", "1") != "1", f.get("parts", "1") != "1", min(e["tokens"], 4))


_SMALL_SLICED = lambda e: max(e["Os"]) <= 264 and e["I"] <= 16392 and (e["I"] <= 1024 or max(e["Os"]) <= 136)   # noqa: E731
_picked = _from_census(sliced.ROWS, _SMALL_SLICED, 1, _sliced_key)
# (both dtypes in every family: the first row of each (kernel, selective pre-pass, dtype) the pass above left out)
_have = {_sliced_key(e)[:2] + (e["dt"],) for e, _ in _picked}
_picked += _from_census(sliced.ROWS, lambda e: _SMALL_SLICED(e) and _sliced_key(e)[:2] + (e["dt"],) not in _have, 1,
                        lambda e: _sliced_key(e)[:2] + (e["dt"],))
for _e, _id in _picked:
    # (a folded layout's uint8 res - v = 8 with 256 residual centroids - may sit at any address: those rows put it at an odd one)
    _res1 = _e["mode"] != "exact" and _e["v"] == 8 and _e["kr"] == 256
    _row(dict(_e, kind="sliced", align="sliced_res1" if _res1 else "sliced", arith=sliced.MODE_ARITH[_e["mode"]]), "sliced-" + _id)


# the batched-decode entries and the fused GEMM: GS of their own tests (8, TILE - 8, TILE + 8 columns), tokens at the slot count and past it
def _bd(entry, align, layer, tokens, xkind, id, instance, arith="exact", **kw):
    _row(dict(kind="bd", entry=entry, align=align, layer=layer, tokens=tokens, xkind=xkind, instance=instance, arith=arith, **kw), id)


for _i, (_T, _dt, _G, _tok, _perm, _O) in enumerate(((16, "f16", 8, 1, 0, 12), (24, "bf16", gg.TILE + 8, 16, 1, 20), (32, "f16", gg.TILE - 8, 9, 1, 100),
                                                     (24, "f16", 2 * gg.TILE + 264, 5, 0, 20), (32, "bf16", 8, 15, 0, 4))):
    _bd("vptq_quant_gemm_gather", "gemm_gather", functools.partial(gg.layer, _G, _O, _T, _dt, _perm, _i % 2), _tok, ("dense", "planted")[_i % 2],
        f"gemm_gather-t{_T}-{_dt}-G{_G}-tok{_tok}-p{_perm}", f"gemm_gather dt={_dt} t={_T} perm={_perm} tok={_tok} tiles={(_G + 1023) // 1024} rgs=1")
for _i, (_T, _dt, _G, _tok, _perm, _O) in enumerate(((16, "bf16", 8, 17, 1, 12), (24, "f16", gg.TILE + 8, 33, 0, 20), (32, "bf16", gg.TILE - 8, 48, 0, 100),
                                                     (16, "f16", gg.TILE + 8, 32, 1, 20))):
    _bd("vptq_quant_gemm_gatherw", "gemm_gatherw", functools.partial(gg.layer, _G, _O, _T, _dt, _perm, _i % 2), _tok, ("dense", "planted")[_i % 2],
        f"gemm_gatherw-t{_T}-{_dt}-G{_G}-tok{_tok}-p{_perm}",
        f"gemm_gatherw dt={_dt} t={_T} perm={_perm} tok={_tok} tb={(_tok + 15) // 16} tiles={(_G + 1023) // 1024} rgs=1")
for _i, (_fmt, _dt, _G, _tok, _perm, _O) in enumerate((("v16-k65536-0", "f16", 8, 1, 0, 13), ("v16-k65536-1024", "bf16", gx.TILE + 8, 16, 1, 40),
                                                       ("v16-k65536-65536", "f16", gx.TILE - 8, 9, 0, 100), ("v8-k65536-4096", "bf16", gx.TILE + 8, 5, 1, 20),
                                                       ("v8-k32768-0", "f16", 8, 16, 1, 4))):
    _bd("vptq_quant_gemm_gatherx", "gemm_gatherx", functools.partial(gx.layer, _G, _O, _fmt, _dt, _perm, _i % 2), _tok, ("dense", "planted")[_i % 2],
        f"gemm_gatherx-{_fmt}-{_dt}-G{_G}-tok{_tok}-p{_perm}", "gemm_gatherx want()", fmt=_fmt, dt=_dt)
for _i, (_dt, _G, _tok, _perm, _O) in enumerate((("f16", 8, 17, 0, 40), ("bf16", kw.TILE + 8, 64, 1, 100), ("f16", kw.TILE - 8, 33, 1, 264), ("bf16", 8, 48, 0, 8))):
    _bd("vptq_quant_gemm_k256w", "gemm_k256w", functools.partial(kw.layer, _G, _O, _dt, _perm, _i % 2), _tok, ("dense", "planted")[_i % 2],
        f"gemm_k256w-{_dt}-G{_G}-tok{_tok}-p{_perm}", f"gemm_k256w dt={_dt} perm={_perm} tok={_tok} tb={(_tok + 15) // 16} rgs=1 pass=1x{(_tok + 15) // 16}")
for _I, _O, _dt, _tok, _arith, _kw in rm.FUSED:
    _bd("vptq_quant_gemm", "gemm", functools.partial(rm._layer, dict(layer=(_I, _O, _kw), dt=_dt), _tok), _tok, "dense" if _arith == "exact" else "planted",
        f"gemm-{_dt}-{_I}x{_O}-tok{_tok}", "vptq_quant_gemm dt=" + _dt, arith=_arith, rounded=_arith == "folded")


# vptq_dequant, vptq_dequant_sliced, vptq_sliced_layout_repack, the layout build
def _dq_layer(I, O, dt, **kw):
    return functools.partial(vo.make_layer, I, O, dtype=dt, dist="llm", seed=I + 3 * O, **kw)


for _id, _layer, _inst in (
        ("dequant-f16-k256-1032x100-perm", _dq_layer(1032, 100, "f16", enable_perm=True), "dequant dt=f16 v=8 "),
        ("dequant-bf16-k4096r16-v6-520x100", _dq_layer(520, 100, "bf16", vector_len=6, num_centroids=4096, num_res_centroids=16), "dequant dt=bf16 v=6 "),
        ("dequant-f16-k65536r256-4104x72", _dq_layer(4104, 72, "f16", num_centroids=65536, num_res_centroids=256), "dequant dt=f16 v=8 "),
        ("dequant-bf16-outliers-groups-2068x100", _dq_layer(2068, 100, "bf16", num_centroids=4096, num_res_centroids=16, num_codebooks=2, outlier_size=8,
                                                          outlier_vector_len=4, num_outlier_centroids=256, enable_perm=True), "dequant dt=bf16 v=8 ")):
    _row(dict(kind="dequant", align="dequant", layer=_layer, instance=_inst), _id)
# ... and at the entry's minimum (W and the norm tensors 2-byte, the indices 4-byte aligned): element loads and stores
_row(dict(kind="dequant", align="dequant", layer=_dq_layer(520, 100, "bf16", vector_len=6, num_centroids=4096, num_res_centroids=16),
          instance="dequant dt=bf16 v=6 tab=2 lds=192 colblocks=1 t=16 norm=vec store=vec idx=vec:65 perm=0 outl=0 groups=1 ragged=0",
          entry_min="dequant_min", fallback="dequant dt=bf16 v=6 tab=2 lds=192 colblocks=1 t=16 norm=scalar store=scalar idx=elem:65 perm=0 outl=0 groups=1 ragged=0"), "dequant-entry-min-bf16-v6-520x100")
for _dt, _I, _O, _v, _kr, _perm in (("f16", 1000, 100, 8, 256, 1), ("bf16", 1032, 72, 16, 65536, 0), ("f16", 4104, 40, 8, 0, 0), ("bf16", 16392, 72, 8, 0, 1)):
    _lay = _dq_layer(_I, _O, _dt, vector_len=_v, num_centroids=65536, num_res_centroids=_kr, enable_perm=bool(_perm))
    _row(dict(kind="dequant_sliced", align="dequant_sliced", layer=_lay, instance=f"dequant_sliced dt={_dt} v={_v} "), f"dequant_sliced-{_dt}-v{_v}-r{_kr}-{_I}x{_O}-p{_perm}")
    _row(dict(kind="repack", align="repack", layer=_lay, instance=f"sliced_layout_repack v={_v} "), f"repack-{_dt}-v{_v}-r{_kr}-{_I}x{_O}-p{_perm}")
for _G, _S, _ib, _rb, _side, _N in ((200, 8, 16, 0, 0, 37), (1032, 16, 16, 8, 1, 5), (8200, 16, 14, 8, 1, 9), (72, 8, 16, 16, 2, 13)):
    _row(dict(kind="layout", align="layout", G=_G, slices=_S, ib=_ib, rb=_rb, side=_side, N=_N, instance=f"sliced_layout_build nsl={_S} side={_side} G={_G} N={_N}"),
         f"layout-G{_G}-nsl{_S}-ib{_ib}-rb{_rb}-side{_side}-N{_N}")

ROW_BY_ID = {e["id"]: e for e in TABLE}
assert len(ROW_BY_ID) == len(TABLE), "row ids must be distinct"


def _expect_instance(e, got):
    """the row's instance: whole strings from the census tables; a prefix (ending in a blank) where the rest is launch shape the
    row does not pin; gemm_gatherx: its own test's formula"""
    want = e["instance"]
    if want == "gemm_gatherx want()":
        return got.startswith(f"gemm_gatherx dt={e['layer']().dtype} ") and f" tok={e['tokens']} " in got
    if not got.endswith(e.get("instance_suffix", "")):
        return False
    return got.startswith(want) if want.endswith(" ") else got == want


@pytest.mark.parametrize("e", [pytest.param(e, id=e["id"]) for e in TABLE])
def test_same_bits_under_every_placement(e, dev, monkeypatch):
    run = RUNNERS[e["kind"]]
    nondet = e["id"] in NOT_BIT_DETERMINISTIC
    # A: benign, 256-byte aligned - against the reference
    a = run(e, dev, PL_A)
    assert _expect_instance(e, a.instance), f"placement A launches {a.instance!r}, the row names {e['instance']!r}"
    if e["kind"] == "chain":
        assert a.route_name == "gemv_k256c_kernel"
    check_reference(e, a, monkeypatch, what=f"{e['id']} A")
    _assert_intact(e, a, PL_A)
    # B: hostile fills, same offsets - A's bits
    b = run(e, dev, PL_B)
    assert b.instance == a.instance
    if nondet:
        check_reference(e, b, monkeypatch, what=f"{e['id']} B")
    else:
        for i, (ya, yb) in enumerate(zip(a.outs, b.outs)):
            assert _same_bits(ya, yb), f"{e['id']}: output {i} differs between the benign and the hostile placement ({a.instance})"
    _assert_intact(e, b, PL_B)
    # C: hostile fills, every operand at its least alignment
    plc = placement_c(e)
    c = run(e, dev, plc)
    if e.get("entry_min"):
        if e["kind"] == "chain":
            assert c.route_name == e["chain_name_c"]
        if e["kind"] == "grouped":
            assert a.route_name != "per-layer" and c.route_name == e["grouped_name"]
        fb = e["fallback"]
        assert c.instance.startswith(fb) if fb.endswith(" ") else c.instance == fb, f"placement C launches {c.instance!r}, the row names the fallback {fb!r}"
        check_reference(e, c, monkeypatch, arith="exact", what=f"{e['id']} C ({c.instance})")
    else:
        assert c.instance == a.instance, f"placement C launches {c.instance!r}, A {a.instance!r}"
        assert getattr(c, "route_name", None) == getattr(a, "route_name", None)
        if nondet:
            check_reference(e, c, monkeypatch, what=f"{e['id']} C")
        else:
            for i, (ya, yc) in enumerate(zip(a.outs, c.outs)):
                assert _same_bits(ya, yc), f"{e['id']}: output {i} differs between 256-byte and least-aligned operands ({a.instance})"
    _assert_intact(e, c, plc)


# ---------------------------------------------------------------------------------------------- coverage of the table
REQUIRED_FAMILIES = {"gemv_k256", "gemv_k256m", "gemm_k256", "gemm_k256t", "gemv_lds", "gemv_lds_mfma", "gemv_gather", "gemv_gatherx",
                     "gemv_generic", "gemv_v2", "gemv_k256c", "gemv_sliced", "gemv_sliced_tok", "gemv_hot", "gemm_gather", "gemm_gatherx",
                     "gemm_gatherw", "gemm_k256w", "vptq_quant_gemm", "dequant", "dequant_sliced", "sliced_layout_repack", "sliced_layout_build"}


def _words(e):
    return {part.split()[0] for part in e["instance"].split(" | ")}


def test_the_table_reaches_every_entry_and_family():
    """the set of instance-string first words the rows reach covers the issue's list, in the forms it names: coverage cannot shrink
    unnoticed"""
    reached = set().union(*[_words(e) for e in TABLE])
    assert REQUIRED_FAMILIES <= reached, sorted(REQUIRED_FAMILIES - reached)
    has = lambda pred: any(pred(e) for e in TABLE)   # noqa: E731
    inst = lambda e: e["instance"]                     # noqa: E731
    for dt in ("f16", "bf16"):
        for fam in REQUIRED_FAMILIES - {"sliced_layout_repack", "sliced_layout_build"}:
            assert has(lambda e: fam in _words(e) and (e.get("dt") == dt or f"dt={dt}" in inst(e))), (fam, dt)
    # vptq_quant_gemv: gemv_k256 exact and <fast>; gemv_k256m exact, folded and selective; generic with outliers and two groups
    assert has(lambda e: inst(e).startswith("gemv_k256 ") and "fast=0" in inst(e)) and has(lambda e: inst(e).startswith("gemv_k256 ") and "fast=1" in inst(e))
    for frag in ("fast=0", "fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", "sel=1"):
        assert has(lambda e: inst(e).startswith("gemv_k256m ") and frag in inst(e)), frag
    assert has(lambda e: inst(e).startswith("gemv_generic") and e.get("S") and e.get("C", 1) == 2)
    # v2: gemv_v2 and gemv_lds fmt=v2*
    assert has(lambda e: e["kind"] == "v2" and inst(e).startswith("gemv_v2")) and has(lambda e: e["kind"] == "v2" and "fmt=v2" in inst(e))
    # grouped: equal and mixed shapes; chain: independent x {exact, folded, selective}, dependent
    assert has(lambda e: e["kind"] == "grouped" and len(set(s[:3] for s in e["shapes"])) == 1)
    assert has(lambda e: e["kind"] == "grouped" and len(set(s[:3] for s in e["shapes"])) > 1)
    for frag in ("dep=0 mode=exact", "dep=0 mode=folded", "dep=0 mode=selective", "dep=1 mode=folded"):
        assert has(lambda e: e["kind"] == "chain" and frag in inst(e)), frag
    assert has(lambda e: e["kind"] == "chain" and "dep=0 mode=exact" in inst(e) and e.get("instance_suffix") == " geom=rows" and not e.get("entry_min"))
    assert has(lambda e: e["kind"] == "chain" and e.get("instance_suffix") == " geom=rows" and e.get("entry_min"))
    # sliced: folded, EX, EX+RG; column parts; one-pass window parts; the token kernel; gemv_hot; the four entries
    sl = [e for e in TABLE if e["kind"] == "sliced"]
    f = lambda e: dict(p.split("=") for p in inst(e).split(" | ")[-1].split()[1:])   # noqa: E731
    for want in (dict(ex="0"), dict(ex="1", rg="0"), dict(ex="1", rg="1")):
        assert any(inst(e).split(" | ")[-1].startswith("gemv_sliced ") and all(f(e)[k] == v for k, v in want.items()) for e in sl), want
    assert any(f(e).get("parts", "1") != "1" for e in sl), "column parts"
    assert any(f(e).get("wparts", "1") != "1" and e["tokens"] in (2, 3) for e in sl), "one-pass window parts"
    assert any(inst(e).startswith("gemv_sliced_tok") for e in sl) and any(inst(e).startswith("gemv_hot") for e in sl)
    assert {(e["tokens"] == 1, e["entry"] in ("grouped", "parts") or len(e["Os"]) > 1) for e in sl} == {(True, False), (True, True), (False, False), (False, True)}
    # every alignment table above is exercised by a placement-C row
    used = {e["align"] for e in TABLE} | {e["entry_min"] for e in TABLE if e.get("entry_min")} | {"sliced_sel"}
    assert any(e["align"] == "sliced_res1" and e["tokens"] == 1 for e in TABLE), "a folded uint8 res at an odd address"
    assert {(e["dt"], e["tokens"]) for e in TABLE if e["align"] == "k256t" and "perm=0" in inst(e)} >= {("f16", 5), ("f16", 16), ("bf16", 5), ("bf16", 16)}
    assert used == set(ALIGN), sorted(set(ALIGN) ^ used)
    assert not NOT_BIT_DETERMINISTIC or all(k in ROW_BY_ID for k in NOT_BIT_DETERMINISTIC)
