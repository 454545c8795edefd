"""`VQuantLinear`: drop-in for microsoft/VPTQ's quantised linear layer
(reference vptq/layers/vqlinear.py:17-240 ctor, :351-397 forward).

What must match the reference byte for byte is the *state-dict contract* HF
checkpoints rely on — parameter names, shapes and dtypes:

    centroids.weight       [C, k*v]            fp16/bf16
    res_centroids.weight   [C, kr*v]           (when num_res_centroids[1] > 0)
    indices                [C, N, ceil(G*T/32)] int32   (packed: idx | ridx << log2 k)
    outlier_centroids.weight [1, ko*ov], outlier_indices [1, M, S] int16
    perm                   [I] int16 (uint16 bit pattern)
    weight_scale, weight_bias [I];  bias [O]

and the constructor keyword arguments HF's `replace_with_vptq_linear` passes
(transformers/integrations/vptq.py).  The module may be built on the `meta`
device; nothing derived from tensor contents is computed in `__init__`.

Only the inference path is implemented: packed indices, `vector_quant_dim="out"`.
The reference's layer-wise fine-tuning helpers (proxy_error_forward,
set_l2_indices, init_parameters from k-means dictionaries) belong to the
quantisation algorithm, which is not part of this hot path.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Sequence

import weakref

import torch
import torch.nn as nn
from torch.nn.parameter import Parameter

from vptq_amd import _backend as B
from vptq_amd import ops
# the batched-decode rules live in vptq_amd/batched_decode.py; the route functions and the token windows are re-exported here (the
# knobs and the cell tables are NOT: tests and tools assign to them, and an alias would keep the old value)
from vptq_amd.batched_decode import (  # noqa: F401
    BATCHED_DECODE_MAX_TOKENS, BATCHED_DECODE_MIN_TOKENS, GEMM_GATHER_MAX_TOKENS, GEMM_GATHER_PX_MAX_TOKENS, GEMM_GATHER_PX_MIN_TOKENS,
    GEMM_GATHERW_MAX_TOKENS, GEMM_GATHERW_MIN_TOKENS, GEMM_K256W_MAX_TOKENS, GEMM_K256W_MIN_TOKENS, batched_decode_routes,
    batched_decode_takes, gemm_gather_px_route, gemm_gather_route, gemm_gatherw_route, gemm_gatherx_route, gemm_k256w_route)
# the batched-decode rules of a GROUP of siblings live in vptq_amd/grouped_decode.py: `GROUPED_DECODE_ROUTES`, one record per group
# route (the knobs and cells are read there, at call time); the guard's window is the union of the routes' windows
from vptq_amd.grouped_decode import (  # noqa: F401
    GROUPED_DECODE_MAX_TOKENS, GROUPED_DECODE_MIN_TOKENS, gemm_gather_grouped_route, gemm_gather_grouped_tokens, gemm_k256_grouped_route,
    gemm_k256_grouped_tokens, grouped_decode_route, grouped_decode_routes, sibling_decode_routes)
# the sliced-layout rules (1 - 4 tokens) live in vptq_amd/sliced_routes.py and are read through the module (`R.exact_route_is_large`:
# one monkeypatch changes every reader); only import-time constants that nothing assigns to are imported by name, for the hot guard
from vptq_amd import sliced_routes as R
from vptq_amd.sliced_routes import _SLICED_FORMATS, _SLICED_LAYOUT_ENV, _SLICED_MAX_TOKENS


def chain_prefetch(layers, circular: bool = False):
    """Tell each layer which one runs next so that its fused GEMV reads the next layer's
    packed indices ahead into L2 / Infinity Cache (pure performance hint)."""
    layers = list(layers)
    for a, b in zip(layers, layers[1:] + ([layers[0]] if circular else [None])):
        object.__setattr__(a, "_prefetch_next", b)
    return layers


def _raw_stream(device_index: int) -> int:
    """hipStream_t of torch's current stream on `device_index` (no Stream object)."""
    return torch._C._cuda_getCurrentRawStream(device_index)


_COMPACTED = weakref.WeakSet()   # compacted layers (their share of the compact-mode scratch)


class LayerCache(NamedTuple):
    """What `VQuantLinear._descriptor()` builds once per set of parameter storages.  The ORDER is part of the contract (`_gemv_cached`
    unpacks it by position: one unpack is cheaper than eleven attribute reads per call; the benchmark reads `[1]`): new fields go last."""
    key: tuple              # storage pointers, version counters, arithmetic generation: a different key rebuilds the whole record
    desc: object            # the C-ABI LayerDesc: what every launch of this layer passes to the library
    keep: list              # the tensors `desc` points at, derived ones included: alive as long as the record is
    device: torch.device    # the parameters' device: activations are checked against it, launches run under it
    gemv: object            # the library's vptq_quant_gemv entry: called by `_gemv_cached`
    max_tokens: int         # most tokens the fused GEMV takes for this format: `forward` and the shards route on it
    generation: int         # unique per record built: SiblingGroup, GemvChain, the sliced layout, the dense descriptor and compact mode key on it
    dtype: torch.dtype      # the centroids' dtype: activations are checked against it, outputs are allocated in it
    device_index: int       # `device` as an index: the raw-stream and workspace look-ups of every launch
    arithmetic_flags: int   # load-time arithmetic gate (GEMV_EXACT / GEMV_SELECTIVE / 0), or-ed into every launch's flags; set_arithmetic renews it via `key`
    workspace_bytes: int    # scratch bytes of the batched-decode kernel: `B.gemv_workspace` of 2+ token launches


def _index_elements(layer) -> int:   # index elements per table: vector-rows x columns
    return layer.indices.shape[1] * layer.group_size


def _res_centroids(layer) -> int:   # entries of the residual codebook; 0 without one
    return layer.num_res_centroids if layer.enable_residual else 0


def _compact_state_dict_hook(module, state_dict, prefix, local_metadata):
    """state_dict() of a compacted layer: the packed indices, bit-identical, rebuilt from the layout"""
    if "_compact" in module.__dict__ and prefix + "indices" in state_dict:
        state_dict[prefix + "indices"] = module.packed_indices()
    return state_dict


def _compact_load_pre_hook(module, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
    """load_state_dict into a compacted layer: a real `indices` parameter again (torch does not load into a meta one), the
    layout and the frozen descriptor dropped - the layer is uncompacted and routes as any other"""
    cp = module.__dict__.get("_compact")
    if cp is not None and prefix + "indices" in state_dict:
        dev = cp["sl"].dev
        module._parameters["indices"] = Parameter(torch.empty(cp["shape"], dtype=torch.int32, device=dev), requires_grad=False)
        module._compact_drop()


def compact_model(model: nn.Module, force: bool = False) -> dict:
    """`VQuantLinear.compact(force)` over every layer of `model`, one at a time (the peak is one layer's build temporaries).
    Returns {"layers": {name: {"before", "after", "freed"}}, "skipped": {name: reason}, "before", "after", "freed"} in bytes of
    index data (`resident_bytes()["total"]`; scratch excluded)."""
    rep = {"layers": {}, "skipped": {}, "before": 0, "after": 0, "freed": 0}
    for name, m in model.named_modules():
        if not isinstance(m, VQuantLinear):
            continue
        b0 = m.resident_bytes()
        freed = m.compact(force)
        b1 = m.resident_bytes()
        before, after = b0["packed"] + b0["layout"], b1["packed"] + b1["layout"]
        rep["before"] += before
        rep["after"] += after
        if m.is_compact() and freed:
            rep["layers"][name] = {"before": before, "after": after, "freed": freed}
            rep["freed"] += freed
        else:
            rep["skipped"][name] = m.__dict__.get("compact_skipped") or "already compacted"
    if torch.cuda.is_available():
        torch.cuda.empty_cache()
    return rep


def prepare_model(model: nn.Module, stream=None) -> dict:
    """`VQuantLinear.prepare(stream)` over every layer of `model`: the sliced layouts of the large-codebook formats are built now (by
    the library's builder, layer by layer) instead of inside the first decode step, and every layer has its one-token workspace for
    `stream` - so a first one-token step captured on `stream` takes the sliced kernels.  The stream's `B.gemv_workspace` is grown to
    the largest x[perm] copy (`vptq_quant_gemm_gather_px_workspace_bytes` at 48 tokens) of the permuted layers `gemm_gather_px_route`
    routes, and to the x[perm] copies `vptq_quant_gemm_gather_grouped` / `vptq_quant_gemm_gatherw_grouped` / `vptq_quant_gemm_gatherx_grouped` /
    `vptq_quant_gemm_k256_grouped` need for the linked sibling groups their routes (`gemm_gather_grouped_route` /
    `gemm_gatherw_grouped_route` / `gemm_gatherx_grouped_route` / `gemm_k256_grouped_route`) route (the largest need over a format's records, each at its largest routed token count), so a 5 - 48 token step captured afterwards keeps those routes.  Returns {"layers": {name: {"built", "bytes", "seconds"}},
    "built": layers with a layout, "bytes", "seconds"}."""
    rep = {"layers": {}, "built": 0, "bytes": 0, "seconds": 0.0}
    px = {}   # device index -> (device, most workspace bytes of its routed permuted layers)
    for name, m in model.named_modules():
        if not isinstance(m, VQuantLinear):
            continue
        r = m.prepare(stream)
        rep["layers"][name] = r
        rep["built"] += int(r["built"] in ("exact", "folded", "selective"))
        rep["bytes"] += r["bytes"]
        rep["seconds"] += r["seconds"]
        need = m._gemm_gather_px_workspace_bytes()
        if need:
            cache = m._descriptor()
            px[cache.device_index] = (cache.device, max(need, px.get(cache.device_index, (None, 0))[1]))
    if not torch.cuda.is_available() or torch.cuda.is_current_stream_capturing():
        return rep
    # ... and to the x[perm] copies of the sibling groups their batched-decode route takes, at the largest routed token count
    groups = {id(g): g for g in (m.__dict__.get("_siblings") for m in model.modules() if isinstance(m, VQuantLinear)) if g is not None}
    for g in groups.values():
        if all(m._parameters["indices"].is_cuda for m in g.members if "_compact" not in m.__dict__):
            need = g._batched_workspace_bytes()
            if need is not None and need[2]:
                px[need[1]] = (need[0], max(need[2], px.get(need[1], (None, 0))[1]))
    for dev_index, (dev, need) in px.items():
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream(dev) if stream is None else stream
            with torch.cuda.stream(s):
                B.gemv_workspace(dev_index, s.cuda_stream, need)
    return rep


class SiblingGroup:
    """Layers that are applied to the SAME activation one after the other (q / k / v, gate / up).
    The first member called with a tensor launches all members in one grouped kernel
    (`vptq_quant_gemv_grouped`: their workgroups share the launch, the prologue and the HBM
    stream); the others return their share of that launch when they are called with the very
    same tensor object (held alive, version checked), and fall back to their own launch
    otherwise.  Pure scheduling: the arithmetic per layer is that of a single launch."""
    MAX_TOKENS = 4

    def __init__(self, members):
        self.members = list(members)
        self._x = None
        self._version = -1
        self._out = {}
        self._arrays = None
        self._bx = None       # forward_batched's leader tensor, its version and the followers' outputs
        self._bversion = -1
        self._bout = {}

    def forward_sliced(self, layer, x, tokens=1):
        """one token (2 - 4: `SlicedGroupGemv.forward_tokens`) of large-codebook siblings over their sliced layouts: ONE launch for the group
        (`vptq_amd/utils/sliced.py:SlicedGroupGemv`); same protocol as `forward` - the first member called launches, the
        others pick their output up when they are called with the very same tensor.  None = not this group's route (a
        member without a layout, mixed formats, a tensor without version counter, ...): the caller goes on alone."""
        ver = B.tensor_version(x)
        if ver >= 0 and self.__dict__.get("_sx") is x and ver == self._sversion and id(layer) in self._sout:
            y = self._sout.pop(id(layer))
            if not self._sout:
                self._sx = None
            return y
        if ver < 0:
            return None
        sls = [m._sliced_gemv() for m in self.members]
        if any(sl is None for sl in sls):
            return None
        key = tuple(id(sl) for sl in sls)
        sg = self.__dict__.get("_sgroup")
        if sg is None or sg[0] != key:
            from vptq_amd.utils.sliced import SlicedGroupGemv
            try:
                sg = (key, SlicedGroupGemv(sls))
            except ValueError:
                # mixed formats / arithmetics: every member launches for itself - remembered for THESE layouts only (the key):
                # a rebuilt layout or another arithmetic (set_arithmetic) makes new objects and the group is looked at again
                sg = (key, None)
            self._sgroup = sg
        group = sg[1]
        if group is None:
            return None
        if tokens == 1:
            ys = group(x)
        else:   # (every member must be a layer this route was measured faster for: VQuantLinear._sliced_one_launch)
            if not all(m._sliced_one_launch(sl, tokens) for m, sl in zip(self.members, sls)):
                return None
            ys = group.forward_tokens(x)
        if ys is None:
            return None
        self._sx, self._sversion, self._keep_sx = x, ver, x
        self._sout = {id(m): y for m, y in zip(self.members, ys) if m is not layer}
        return ys[self.members.index(layer)]

    def _batched_static(self):
        """what the group's batched-decode route is asked with, from the members' static configuration: (vector length, main
        centroids, residual centroids, output widths, input width, has_perm: True - every member has a permutation, False - none,
        None - some), or None where the members do not share format and width or are not one-codebook layers with scale and bias.
        `_batched_route` is the first record of the format's group routes (`sibling_decode_routes`, vptq_amd/grouped_decode.py: the
        owner in `GROUPED_DECODE_ROUTES`, then its wide routes; for gemm_gatherx's formats the record of `GROUPED_DECODE_X_ROUTES`), or
        None; with a token count, the record of the format whose window holds it."""
        st = self.__dict__.get("_bstatic")
        if st is None:
            ms = self.members
            fmt = {(m.vector_len, m.num_centroids, _res_centroids(m), m.in_features) for m in ms}
            if len(fmt) != 1 or any(m.num_codebooks != 1 or m.enable_outlier or not m.enable_norm for m in ms):
                st = (None,)
            else:
                perms = {bool(m.enable_perm) for m in ms}
                v, k, kr, width = next(iter(fmt))
                st = ((v, k, kr, tuple(m.out_features for m in ms), width, perms.pop() if len(perms) == 1 else None),)
            self._bstatic = st
            self._broutes = sibling_decode_routes(*st[0][:3]) if st[0] is not None else ()
            self._broute = self._broutes[0] if self._broutes else None
        return st[0]

    def _batched_route(self, tokens=None):
        if self._batched_static() is None:
            return None
        if tokens is None:
            return self._broute
        for r in self._broutes:   # (the windows of one format are disjoint)
            if r.min_tokens <= tokens <= r.max_tokens:
                return r
        return None

    def _batched_plan(self, r=None):
        """the descriptor array the group route's entry (`vptq_quant_gemm_gather_grouped` / `vptq_quant_gemm_gatherw_grouped` / `vptq_quant_gemm_gatherx_grouped` /
        `vptq_quant_gemm_k256_grouped`) is called
        with, (descs, caches), decided once per entry (r: a record of the format, default its first) and per set of descriptor generations - or None: no route has the format, a compacted member, a library without the entry, members on several devices or of
        several dtypes, a group the library does not serve.  Members whose `perm` tensors are `torch.equal` get ONE perm pointer in
        their descriptor copies (the first such member's): the entry then gathers x once for them.  Not decided inside a stream
        capture (the comparison reads the device): the caller goes on alone and a later call asks again."""
        caches = [m._descriptor() for m in self.members]
        key = tuple(c.generation for c in caches)   # a rebuilt descriptor never matches
        if r is None:
            r = self._batched_route()
        plans = self.__dict__.setdefault("_bplan", {})   # entry -> (generations, plan)
        st = plans.get(r.entry) if r is not None else plans.get(None)
        if st is not None and st[0] == key:
            return st[1]
        plan = None
        lib = B.lib()
        if r is not None and not any("_compact" in m.__dict__ for m in self.members) and getattr(lib, r.entry, None) is not None \
                and len({(c.device, c.dtype) for c in caches}) == 1:
            perms = [m._parameters.get("perm") if m.enable_perm else None for m in self.members]
            if any(p is not None and p.is_cuda for p in perms) and torch.cuda.is_current_stream_capturing():
                return None
            n = len(caches)
            descs = (B.LayerDesc * n)(*[B.LayerDesc.from_buffer_copy(c.desc) for c in caches])
            first = []   # (perm tensor, perm pointer) of every distinct permutation so far
            for i, p in enumerate(perms):
                if p is None or not descs[i].perm:
                    continue
                for q, ptr in first:
                    if p.shape == q.shape and torch.equal(p, q):
                        descs[i].perm = ptr
                        break
                else:
                    first.append((p, descs[i].perm))
            if getattr(lib, r.entry + "_supported")(descs, n, r.min_tokens):
                plan = (descs, caches)   # (the caches keep what the descriptors point at alive)
        plans[r.entry if r is not None else None] = (key, plan)
        return plan

    def _batched_workspace_bytes(self):
        """(device, device index, bytes) of stream workspace the largest call the group's batched-decode route can take needs
        (`prepare_model` grows the stream's buffer to it) - the largest need over the format's records, each at its largest routed
        token count - or None: the group never takes such a route"""
        st = self._batched_static()
        if self._batched_route() is None:
            return None
        best = None
        for r in self._broutes:
            routed = r.tokens(*st)
            plan = self._batched_plan(r) if routed else None
            if plan is None:
                continue
            descs, caches = plan
            if r.exact_only and not all(c.arithmetic_flags & B.GEMV_EXACT for c in caches):
                continue
            need = int(getattr(B.lib(), r.entry + "_workspace_bytes")(descs, len(caches), routed[-1]))
            if best is None or need > best[2]:
                best = (caches[0].device, caches[0].device_index, need)
        return best

    def forward_batched(self, layer, x, tokens):
        """5 - 48 tokens of large-codebook and of canonical-format siblings: ONE launch for the group (the entry of the group's record
        whose window holds the token count: `vptq_quant_gemm_gather_grouped` up to 16 tokens / `vptq_quant_gemm_gatherw_grouped` from 17 /
        `vptq_quant_gemm_gatherx_grouped` (gemm_gatherx's formats, up to 16 tokens) / `vptq_quant_gemm_k256_grouped`, one x gather per distinct permutation) where the group's route (vptq_amd/grouped_decode.py) takes the call; same protocol as `forward` -
        the first member called launches, the others pick their output up when they are called with the very same tensor at the
        same version.  None = not this group's route (no route has the format, the route function says no, a compacted member,
        mixed formats or dtypes, a group the library does not serve, a member whose arithmetic is not the reference's roundings where
        the kernel has no other, an x that is not what the entry takes, a tensor without version counter, a capture with too small a
        workspace): the caller goes on alone over the routes it had."""
        D = self.__dict__
        ver = B.tensor_version(x)
        if ver >= 0 and D.get("_bx") is x and ver == self._bversion and id(layer) in self._bout:
            y = self._bout.pop(id(layer))
            if not self._bout:
                self._bx = self._keep_bx = None
            return y
        st, r = self._batched_static(), self._batched_route(tokens)
        if r is None or not r.route(st[0], st[1], st[2], st[3], st[4], tokens, st[5]):
            return None
        if ver < 0 or ops.quant_gemm_flags() & r.off_flags:
            self._bx, self._bout = None, {}
            return None
        self._bx, self._bout = None, {}     # a new leader call: whatever an earlier one left unconsumed is stale
        plan = self._batched_plan(r)
        if plan is None:
            return None
        descs, caches = plan
        if r.exact_only and not all(c.arithmetic_flags & B.GEMV_EXACT for c in caches):
            return None   # (set_arithmetic("folded" / "selective"), or a member the load-time gate moved: the members keep their routes)
        if x.shape[-1] != st[4] or x.dtype != caches[0].dtype or x.device != caches[0].device:
            return None   # (the member's own routes raise the shape / dtype / device errors)
        xc = x if x.is_contiguous() else x.contiguous()
        if xc.data_ptr() % 16:
            return None
        ys = getattr(ops, r.entry[len("vptq_"):])(xc, descs, st[3])
        if ys is None:
            return None
        self._bx, self._bversion, self._keep_bx = x, ver, xc
        self._bout = {id(m): y for m, y in zip(self.members, ys) if m is not layer}
        return ys[self.members.index(layer)]

    def forward(self, layer, x, tokens):
        # Tensors made under inference_mode track no version (-1): whether x was rewritten in place since the
        # leader's launch cannot be told then, so sibling outputs are not reused at all - every layer launches
        # for itself, as without a group.
        ver = B.tensor_version(x)
        if ver >= 0 and self._x is x and ver == self._version and id(layer) in self._out:
            y = self._out.pop(id(layer))
            if not self._out:
                self._x = None
            return y
        if ver < 0:
            self._x, self._out = None, {}
            return None
        self._out = {}     # a new leader call: whatever an earlier one left unconsumed is stale
        xc = layer._check_activation(x)
        caches = [m._descriptor() for m in self.members]
        dev = caches[0].device
        if any(c.device != dev for c in caches) or xc.device != dev or \
                any(m.in_features != layer.in_features for m in self.members):
            raise RuntimeError("sibling layers must share the device and the input width")
        key = tuple(c.generation for c in caches)  # a rebuilt descriptor never matches
        stale = self._arrays is None or self._arrays[0] != key
        if stale and any("_compact" in m.__dict__ for m in self.members):
            # a compacted member has no packed indices for the grouped launch to read: every member launches for itself (compacting
            # or uncompacting a layer rebuilds its descriptor: a new key)
            self._arrays = (key, None, None)
        elif stale:
            import ctypes as C
            # one launch per ARITHMETIC: the members the load-time gate sends to the reference's roundings (VPTQ_GEMV_EXACT) go out as a
            # launch of their own, so that one such layer does not drag its siblings out of the selective / folded form (bf16 layers sit
            # close to the gate: with every group exact as soon as one member is, a decoder ran at the reference's speed)
            parts = []
            for want in (False, True):
                idx = [i for i, c in enumerate(caches) if bool(c.arithmetic_flags & B.GEMV_EXACT) == want]
                if idx:
                    fl = 0
                    for i in idx:
                        fl |= caches[i].arithmetic_flags
                    parts.append((idx, (B.LayerDesc * len(idx))(*[caches[i].desc for i in idx]), (C.c_void_p * len(idx))(),
                                  (C.c_void_p * len(idx))(), fl))
            self._arrays = (key, parts, B.lib().vptq_quant_gemv_grouped)
        _, parts, fn = self._arrays
        if parts is None:
            return None
        ys = [torch.empty(xc.shape[:-1] + (m.out_features,), dtype=xc.dtype, device=dev)
              for m in self.members]
        dev_index = caches[0].device_index
        base_flags = ops.quant_gemm_flags()

        def launch(sp):
            for idx, descs, xp, yp, fl in parts:
                for j, i in enumerate(idx):
                    xp[j] = xc.data_ptr()
                    yp[j] = ys[i].data_ptr()
                rc = fn(descs, len(idx), xp, yp, tokens, base_flags | fl, sp)
                if rc:
                    B.check(rc, "vptq_quant_gemv_grouped")
        if torch.cuda.current_device() != dev_index:
            with torch.cuda.device(dev):
                launch(B.current_stream_ptr(dev))
        else:
            launch(_raw_stream(dev_index))
        self._x, self._version = x, B.tensor_version(x)
        self._keep_x = xc
        self._out = {id(m): y for m, y in zip(self.members, ys) if m is not layer}
        return ys[self.members.index(layer)]


SIBLING_PATTERNS = (("q_proj", "k_proj", "v_proj"), ("gate_proj", "up_proj"))


def link_siblings(model: nn.Module, patterns=SIBLING_PATTERNS) -> int:
    """Find, under every sub-module of `model`, children named like one of `patterns` that are all
    `VQuantLinear` layers of the same input width and dtype, and make each set a
    `SiblingGroup`.  Returns the number of groups.  Decode-time optimisation (1-4 tokens; 5-16 tokens of the large-codebook
    formats and 5-48 of the canonical format where the group's route of vptq_amd/grouped_decode.py routes the group:
    `SiblingGroup.forward_batched`)."""
    n = 0
    for parent in model.modules():
        for names in patterns:
            kids = [getattr(parent, nm, None) for nm in names]
            if not all(isinstance(k, VQuantLinear) for k in kids):
                continue
            if len({(k.in_features, k.centroids.weight.dtype) for k in kids}) != 1:
                continue
            group = SiblingGroup(kids)
            for k in kids:
                object.__setattr__(k, "_siblings", group)
            n += 1
    return n


class VQuantLinear(nn.Module):
    _desc_generation = 0  # bumped for every descriptor built (SiblingGroup keys on it)

    def __init__(
        self,
        in_features: int,
        out_features: int,
        vector_lens: Sequence[int],
        num_centroids: Sequence[int],
        num_res_centroids: Sequence[int],
        group_num: int,
        group_size: int,
        outlier_size: int,
        indices_as_float: bool,
        enable_norm: bool = False,
        enable_perm: bool = False,
        is_indice_packed: bool = False,
        bias: bool = False,
        vector_quant_dim: str = "out",
        device=None,
        dtype=None,
        enable_proxy_error=True,
        **unused_kwargs,  # e.g. `norm_dim`, written by the reference's pack tools
    ):
        super().__init__()
        if vector_quant_dim not in ("in", "out"):
            raise ValueError("vector_quant_dim must be 'in' or 'out'.")
        if vector_quant_dim == "in":
            raise RuntimeError("Not implemented yet.")
        if not is_indice_packed:
            raise RuntimeError(
                "vptq_amd.VQuantLinear supports packed indices only (is_indice_packed=True): "
                "that is the format of every published VPTQ checkpoint; the reference's "
                "unpacked mode exists for fine-tuning.")
        fk = {"device": device, "dtype": dtype}
        self.vector_quant_dim = vector_quant_dim
        self.in_features, self.out_features = in_features, out_features
        self.enable_proxy_error = enable_proxy_error
        self.indices_as_float = indices_as_float
        self.is_indice_packed = True
        index_type = torch.float16 if indices_as_float else torch.int16

        if bias:
            self.bias = Parameter(torch.empty(out_features, **fk))
        else:
            self.register_parameter("bias", None)

        # main codebook(s): second element of the (outlier, main) pairs
        self.vector_len = vector_lens[1]
        self.num_centroids = num_centroids[1]
        self.group_num = self.num_codebooks = group_num
        self.group_size = group_size
        self.centroids = nn.Embedding(group_num, self.num_centroids * self.vector_len, **fk)

        # outlier columns: first element of the pairs
        self.outlier_size = outlier_size
        self.outlier_vector_len = vector_lens[0]
        self.num_outlier_centroids = num_centroids[0]
        self.outlier_num_res_centroids = num_res_centroids[0]
        self.enable_outlier = bool(self.outlier_vector_len > 1 and self.num_outlier_centroids > 0)
        self.outlier_padding = 0
        self.ouliter_num_indices = 0  # (sic) attribute name kept from the reference
        self.outlier_centroids = None
        self.outlier_indices = None
        if self.enable_outlier:
            if self.outlier_num_res_centroids != -1:
                raise ValueError("Current implementation does not support residual "
                                 "quantization on outliers yet.")
            self.outlier_padding = (-out_features) % self.outlier_vector_len
            self.ouliter_num_indices = (out_features + self.outlier_padding) // self.outlier_vector_len
            self.outlier_centroids = nn.Embedding(
                1, self.num_outlier_centroids * self.outlier_vector_len, **fk)
            self.outlier_indices = Parameter(
                torch.empty((1, self.ouliter_num_indices, outlier_size), dtype=index_type,
                            device=device), requires_grad=False)

        # residual codebook (indices ride inside the packed stream)
        self.num_res_centroids = num_res_centroids[1]
        self.enable_residual = self.num_res_centroids > 0
        self.res_indices = None
        if self.enable_residual:
            self.res_centroids = nn.Embedding(
                group_num, self.num_res_centroids * self.vector_len, **fk)
        else:
            self.register_parameter("res_centroids", None)

        self.enable_perm = enable_perm
        if enable_perm:
            self.perm = Parameter(torch.arange(in_features, device=device).to(torch.int16),
                                  requires_grad=False)

        self.enable_norm = enable_norm
        self.weight_scale = self.weight_bias = None
        if enable_norm:
            self.weight_scale = Parameter(torch.empty(in_features, **fk))
            self.weight_bias = Parameter(torch.empty(in_features, **fk))

        self.padding = (-out_features) % self.vector_len
        self.num_indices = (out_features + self.padding) // self.vector_len
        self.index_bits = int(math.log2(self.num_centroids))
        self.res_index_bits = int(math.log2(self.num_res_centroids)) if self.enable_residual else 0
        self.total_index_bits = self.index_bits + self.res_index_bits
        packed_groupsize = math.ceil(group_size * self.total_index_bits / 32)
        self.indices = Parameter(
            torch.empty((group_num, self.num_indices, packed_groupsize), dtype=torch.int32,
                        device=device), requires_grad=False)
        # optional: the layer that runs after this one (set by `chain_prefetch`); its packed
        # indices are read ahead by this layer's GEMV.  Not a parameter / buffer.
        self._prefetch_next = None

    def forward(self, x: torch.Tensor, W=None, H=None) -> torch.Tensor:
        """x [..., in_features] fp16/bf16 -> [..., out_features]."""
        if self.enable_proxy_error:
            raise RuntimeError(
                "enable_proxy_error=True selects the reference's layer-wise fine-tuning debug "
                "path, which is outside this inference package; construct the layer with "
                "enable_proxy_error=False (HF does).")
        tokens = x.numel() // x.shape[-1] if x.shape[-1] else 0
        if GROUPED_DECODE_MIN_TOKENS <= tokens <= GROUPED_DECODE_MAX_TOKENS and x.is_cuda:
            group = self.__dict__.get("_siblings")
            if group is not None:     # q / k / v, gate / up: one launch for the group where its route (vptq_amd/grouped_decode.py) takes the call
                y = group.forward_batched(self, x, tokens)
                if y is not None:
                    return y
        if BATCHED_DECODE_MIN_TOKENS <= tokens <= BATCHED_DECODE_MAX_TOKENS and x.is_cuda and self.__dict__.get("_bd_routes", True):
            y = self._batched_decode_cached(x, tokens)   # (5 - 64 tokens in one launch, where a route of vptq_amd/batched_decode.py takes the call)
            if y is not None:
                return y
        if 1 <= tokens <= B.GEMV_MAX_TOKENS and x.is_cuda and \
                (tokens <= B.GEMV_ANY_FORMAT_TOKENS or tokens <= self._descriptor().max_tokens):
            return self._gemv_cached(x, tokens)
        if tokens >= 1 and x.is_cuda and ops.fused_gemm_max_tokens() < tokens:
            return self._dense_cached(x)
        return ops.quant_gemm(
            x,
            bias=self.bias,
            indices=self.packed_indices(),
            centroids=self.centroids.weight,
            outlier_indices=self.outlier_indices,
            outlier_centroids=self.outlier_centroids.weight if self.enable_outlier else None,
            residual_indices=None,
            residual_centroids=self.res_centroids.weight if self.enable_residual else None,
            perm=self.perm if self.enable_perm else None,
            weight_scale=self.weight_scale,
            weight_bias=self.weight_bias,
            vector_len=self.vector_len,
            outlier_vector_len=self.outlier_vector_len,
            num_codebooks=self.num_codebooks,
            num_centroids=self.num_centroids,
            num_outlier_centroids=self.num_outlier_centroids,
            num_res_centroids=self.num_res_centroids,
            is_indice_packed=True,
            group_size=self.group_size,
            outlier_size=self.outlier_size,
            in_features=self.in_features,
            out_features=self.out_features,
            padding=self.padding,
            outlier_padding=self.outlier_padding,
            vector_quant_dim=self.vector_quant_dim,
            prefetch=None if self._prefetch_next is None or "_compact" in self._prefetch_next.__dict__ else self._prefetch_next.indices,
        )

    def _descriptor(self):
        """This layer's `LayerCache`: the C-ABI descriptor and what the launches need beside it, built once
        and reused while the parameter storages stay the same (building it costs ~25 us of Python per
        call, several times the kernel itself)."""
        # parameters straight out of the module's dicts: nn.Module.__getattr__ costs ~0.4 us per name,
        # ten names per call were a third of this function (tools/py_overhead.py)
        P, M = self._parameters, self._modules
        nxt = self._prefetch_next
        # (an absent tensor is either a None entry of _parameters or a plain None attribute: .get covers both)
        perm = P.get("perm") if self.enable_perm else None
        tensors = (P["indices"], M["centroids"]._parameters["weight"],
                   M["res_centroids"]._parameters["weight"] if self.enable_residual else None,
                   P.get("outlier_indices"),
                   M["outlier_centroids"]._parameters["weight"] if self.enable_outlier else None,
                   perm, P.get("weight_scale"), P.get("weight_bias"),
                   P.get("bias"), None if nxt is None else nxt._parameters["indices"])
        # storage pointers of everything; version counters of the tensors the descriptor holds DERIVED
        # copies of (scale / bias in column order for `perm` layers), which an in-place update of the
        # parameters (load_state_dict's copy_, an optimizer step) must invalidate
        key = tuple(0 if t is None else t.data_ptr() for t in tensors) + (B.arithmetic_generation(),)
        if perm is not None:
            key += (B.tensor_version(perm), B.tensor_version(tensors[6]), B.tensor_version(tensors[7]))
        cache = self.__dict__.get("_desc_cache")
        if cache is None or cache.key != key:
            # compact mode (the meta `indices` of a compacted layer are part of the key with pointer 0): the descriptor's `indices` is the
            # layout's stand-in, and there is no prefetch from or of a layer without packed indices
            cp = self.__dict__.get("_compact")
            if cp is not None or (nxt is not None and "_compact" in nxt.__dict__):
                tensors = (tensors[0] if cp is None else cp["standin"],) + tensors[1:9] + (None,)
            dev = B.require_device(*[t for t in tensors if t is not None])
            desc, keep = B.make_layer_desc(bias=tensors[8], prefetch=tensors[9], **self._layer_desc_keywords())
            VQuantLinear._desc_generation += 1
            cache = LayerCache(
                key, desc, keep, dev, B.lib().vptq_quant_gemv, B.lib().vptq_quant_gemv_max_tokens(desc), VQuantLinear._desc_generation,
                tensors[1].dtype, dev.index if dev.index is not None else torch.cuda.current_device(),
                # (compact mode: the gate is frozen at "refused" - it would read index data -, i.e. the reference's roundings in every
                # arithmetic, the documented fallback of every route without a selective form)
                B.GEMV_EXACT if cp is not None else B.layer_arithmetic_flags(self._folded_form_is_safe(tensors, desc)),
                B.lib().vptq_quant_gemv_workspace_bytes(desc, 16, 0))
            self.__dict__["_desc_cache"] = cache
        return cache

    def _layer_desc_keywords(self) -> dict:
        """the `B.make_layer_desc` keywords every descriptor of this layer shares (compact mode: `indices` is the layout's stand-in);
        the caller adds `bias` and `prefetch` or `need_inv_perm`"""
        P, M = self._parameters, self._modules
        cp = self.__dict__.get("_compact")
        return dict(
            indices=P["indices"] if cp is None else cp["standin"], centroids=M["centroids"]._parameters["weight"],
            res_centroids=M["res_centroids"]._parameters["weight"] if self.enable_residual else None,
            outlier_indices=P.get("outlier_indices"),
            outlier_centroids=M["outlier_centroids"]._parameters["weight"] if self.enable_outlier else None,
            perm=P.get("perm") if self.enable_perm else None, weight_scale=P.get("weight_scale"), weight_bias=P.get("weight_bias"),
            in_features=self.in_features, out_features=self.out_features, vector_len=self.vector_len,
            num_codebooks=self.num_codebooks, num_centroids=self.num_centroids, num_res_centroids=_res_centroids(self),
            group_size=self.group_size, outlier_size=self.outlier_size if self.enable_outlier else 0,
            outlier_vector_len=self.outlier_vector_len, num_outlier_centroids=self.num_outlier_centroids)

    def _folded_form_is_safe(self, tensors, desc=None) -> bool:
        """Load-time gate of the library's default ("folded") decode arithmetic (`_backend.folded_form_is_safe`): the layer
        runs both forms on probe activations and keeps the folded one while their un-rounded outputs stay within
        `FOLDED_MAX_PROBE_DISTANCE` of max|y|; bias-dominated layers and layers with few distinct vector-rows get
        VPTQ_GEMV_EXACT (the reference's three roundings per weight).  One device -> host read per descriptor build, i.e.
        per layer load."""
        return B.folded_form_is_safe(tensors[0], tensors[1], tensors[2], tensors[6], tensors[7], desc,
                                     self.in_features, self.out_features)

    def _check_activation(self, x: torch.Tensor) -> torch.Tensor:
        if x.shape[-1] != self.in_features:
            raise RuntimeError(f"x has {x.shape[-1]} features, layer expects {self.in_features}")
        cw = self.centroids.weight
        if x.dtype != cw.dtype:
            raise RuntimeError(f"activation dtype {x.dtype} != weight dtype {cw.dtype}")
        if not x.is_cuda:
            raise RuntimeError("vptq_amd has no CPU path: x must be on the GPU")
        return x if x.is_contiguous() else x.contiguous()

    # derived, device-bound state (ctypes descriptors, the sliced layout, sibling links) is rebuilt on demand: it is
    # neither pickled nor deep-copied with the module (torch.save(model), copy.deepcopy(model)); the same holds for the batched-decode
    # routes of THIS process's library and its `_supported` answers (descriptor generations restart at 0 in every process)
    _DERIVED_STATE = ("_desc_cache", "_desc_dense", "_sliced", "_sliced_cand", "_siblings", "_bd_routes", "_bd_supported")

    def __getstate__(self):
        state = dict(self.__dict__)
        for k in self._DERIVED_STATE:
            state.pop(k, None)
        if state.pop("_compact", None) is not None:   # (a compacted layer is saved / copied with its packed indices, uncompacted)
            state["_parameters"] = dict(state["_parameters"], indices=Parameter(self.packed_indices(), requires_grad=False))
        return state

    def __deepcopy__(self, memo):
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k not in self._DERIVED_STATE and k != "_compact":
                new.__dict__[k] = copy.deepcopy(v, memo)
        if "_compact" in self.__dict__:   # (the copy is uncompacted: it gets the packed indices, not a second layout)
            new._parameters["indices"] = Parameter(self.packed_indices(), requires_grad=False)
        return new

    def enable_sliced_layout(self, enable: bool = True):
        """Opt this layer in to (out of) the load-time derived "sliced" layout of the large-codebook formats
        v8-k65536-0 / v8-k65536-256 (vptq_amd/utils/sliced.py, gemv_sliced.hip): one-token calls then run 2-2.8x
        faster (8192^2: 40 -> 14-19 us) for 1.7-2x the packed indices of extra device memory.  The layout is built
        at the first one-token call; the state-dict tensors are untouched.  Process-wide: VPTQ_SLICED_LAYOUT=1."""
        self.__dict__["_sliced_on"] = bool(enable)
        self.__dict__.pop("_sliced", None)

    def prepare(self, stream=None) -> dict:
        """Make this layer ready NOW for one-token calls on `stream` (default: the current stream of the layer's device): the
        descriptor's derived state, the sliced layout(s) `_sliced_gemv()` would otherwise build at the first one-token call in the
        current arithmetic - same routing rule, same gate, cached under the same stamp - and the zeroed one-token workspace of
        `stream` (workspaces are per stream and are not allocated during a capture: a caller who will capture on stream s passes
        s).  Returns {"built": "exact" | "folded" | "selective" | the reason no layout was built, "bytes": device bytes of the
        layout tensors, "seconds": wall time including the build's read-back}.  A first one-token call inside
        `torch.cuda.graph(g, stream=s)` after `prepare(stream=s)` takes the sliced kernel."""
        import time
        t0 = time.perf_counter()
        rep = {"built": None, "bytes": 0, "seconds": 0.0}
        ind = self._parameters["indices"]
        cp = self.__dict__.get("_compact")
        why = None
        if cp is None and not ind.is_cuda:
            why = "indices are not on a ROCm device"
        elif torch.cuda.is_current_stream_capturing():
            why = "inside a stream capture"
        elif not R.has_sliced_format(self.vector_len, self.num_centroids, self.num_codebooks, self.enable_outlier, self.enable_norm):
            self._descriptor()
            why = f"format has no sliced layout ({_SLICED_FORMATS})"
        if why is None:
            dev = self._descriptor().device
            with torch.cuda.device(dev):
                s = torch.cuda.current_stream(dev) if stream is None else stream
                with torch.cuda.stream(s):
                    sl = self._sliced_gemv()
                    if sl is not None:
                        sl._workspace(s.cuda_stream)
                        s.synchronize()   # (the layout and the zeroed workspace are complete before any other stream uses them)
            if sl is None:
                if not self.__dict__.get("_sliced_on", _SLICED_LAYOUT_ENV):
                    why = "sliced layouts are switched off (VPTQ_SLICED_LAYOUT=0 / enable_sliced_layout(False))"
                elif "_sliced_oom" in self.__dict__:
                    why = "out of device memory building the layout"
                else:
                    why = "one token takes the gather kernel for this layer (no sliced route for its size, width or arithmetic, or " \
                          "too little free device memory for the layout)"
            else:
                rep["built"] = "exact" if sl.exact else ("selective" if sl.selective else "folded")
                rep["bytes"] = sl.layout_bytes()
        if why is not None:
            rep["built"] = why
        rep["seconds"] = time.perf_counter() - t0
        return rep

    def _sliced_gemv(self):
        """This layer's `SlicedGemv` in the current arithmetic, built at the first call and remembered under a stamp (the descriptor's
        generation, the indices' version counter), or None: the regular route serves the layer.  Every outcome is stored under the
        stamp but two: a "no" because a stream capture is in progress and a "no" of the out-of-memory back-off (`_sliced_build`) -
        a later call asks again."""
        cp = self.__dict__.get("_compact")
        if cp is not None:
            # compact mode: the exact layout is the only copy of the indices - served in every arithmetic, whatever
            # VPTQ_SLICED_LAYOUT says, never rebuilt (a rebuilt descriptor is only re-attached)
            cache = self._descriptor()
            if cp["gen"] != cache.generation:
                cp["sl"], cp["gen"] = cp["sl"].rebound(cache.desc), cache.generation
            return cp["sl"]
        on = self.__dict__.get("_sliced_on", _SLICED_LAYOUT_ENV)   # (`enable_sliced_layout()`'s word, else VPTQ_SLICED_LAYOUT's)
        if not on:
            return None
        cache = self._descriptor()
        st = self.__dict__.get("_sliced")
        # (a rebuilt descriptor = other tensors; a bumped version counter = indices rewritten in place: rebuild)
        stamp = (cache.generation, B.tensor_version(self._parameters["indices"]))
        if st is None or st[0] != stamp:
            if torch.cuda.is_current_stream_capturing():
                return None   # (no layout is built inside a capture - and the "no" is not remembered: a later call builds it)
            obj = None
            kind, wanted = self._sliced_kind(cache)
            if wanted and self._sliced_fits(cache, on):
                obj = self._sliced_build(cache, kind)
                if obj is None:
                    return None   # (the back-off of a build that ran out of device memory: not remembered either)
                obj = self._sliced_gate(cache, kind, obj, on)
            st = self.__dict__["_sliced"] = (stamp, obj)
        return st[1]

    def _sliced_kind(self, cache):
        """(kind, wanted) of `R.sliced_layout_kind` for this layer: its arithmetic, format and size, whether `enable_sliced_layout()`
        asked, and the library's three answers (host-only queries without side effects, asked once per layout build)"""
        from vptq_amd.utils.sliced import exact_column_parts
        lib, desc = B.lib(), cache.desc
        folded = bool(lib.vptq_sliced_layout_supported_for(desc, 0))   # (the folded layouts, which the selective form runs over as well)
        return R.sliced_layout_kind(cache.arithmetic_flags, self.vector_len, _res_centroids(self), _index_elements(self),
                                    "_sliced_on" in self.__dict__, bool(lib.vptq_quant_gemv_sliced_selective_supported(desc)) and folded,
                                    bool(exact_column_parts(desc, self.group_size)[0]), folded)

    def _sliced_build(self, cache, kind):
        """The guarded build: a `SlicedGemv` of `kind`, or None - out of device memory now, or inside the back-off after that.  The
        caller does NOT store that None under the stamp: every later call counts the back-off down here.  The warning is issued once
        per layer; a successful build clears `_sliced_oom`."""
        from vptq_amd.utils.sliced import SlicedGemv
        # (a build that ran out of device memory is retried only after a back-off: every attempt costs int64 / float64
        # temporaries of ~160 bytes per element, an empty_cache() and a warning - per decode call, while memory stays tight)
        oom = self.__dict__.get("_sliced_oom")
        if oom is not None:
            oom[0] -= 1
            if oom[0] > 0 and torch.cuda.mem_get_info(cache.device)[0] < oom[1]:
                return None
        try:
            obj = SlicedGemv(self, exact=kind == "exact", selective=kind == "selective")
            self.__dict__.pop("_sliced_oom", None)
            return obj
        except torch.cuda.OutOfMemoryError as e:
            # out of device memory while building: the regular route serves the calls until _SLICED_OOM_RETRY_CALLS further
            # ones have passed or the device reports twice the free bytes it had now.  Any other error is a bug and propagates.
            import warnings
            torch.cuda.empty_cache()
            if oom is None:   # (warn once per layer)
                warnings.warn(f"sliced layout of a {self.in_features} x {self.out_features} layer not built "
                              f"({str(e)[:120]}); the layer keeps the gather kernel for now", stacklevel=4)
            self.__dict__["_sliced_oom"] = [R._SLICED_OOM_RETRY_CALLS, 2 * torch.cuda.mem_get_info(cache.device)[0] + _index_elements(self) * R._SLICED_TORCH_BUILDER_BYTES]
            return None

    def _sliced_gate(self, cache, kind, obj, on):
        """The load-time gate of a layout just built: `obj` where it passes (exact layouts are not asked), else - a selective layout
        - an exact build where `exact_column_parts` and `_sliced_fits` allow one, else None.  `OutOfMemoryError` and `ValueError`
        are swallowed in that fallback build only.  Whatever comes back is stored under the stamp."""
        # the kernel over the layouts evaluates the folded form: the same measured gate as every folded route
        # (_backend.folded_form_is_safe) - its float32 outputs against the gather kernel's (the reference's roundings)
        # on the probe activations
        lim = None if kind == "exact" else (B.SELECTIVE_MAX_PROBE_DISTANCE if kind == "selective" else B.FOLDED_MAX_PROBE_DISTANCE).get(cache.dtype)
        if lim is None or self._parameters.get("weight_bias") is None:
            return obj
        from vptq_amd.utils.sliced import SlicedGemv, exact_column_parts
        d = B.folded_probe_distance(cache.desc, self.in_features, self.out_features, self._parameters["weight_bias"], cache.dtype, cache.device,
                                    folded=lambda xr, yr: obj(xr.view(1, 1, -1), yr.view(1, 1, -1), flags=B.GEMV_OUT_F32) is not None)
        if bool((d <= lim).item()):
            return obj
        # the gate refused the selective form of this layer: the reference's roundings over an exact layout
        # (main entry from LDS, residual entry from L2), where that route serves it
        if kind == "selective" and exact_column_parts(cache.desc, self.group_size)[0] and self._sliced_fits(cache, on):
            try:
                return SlicedGemv(self, exact=True)
            except (torch.cuda.OutOfMemoryError, ValueError):
                pass
        return None

    def _sliced_token_limit(self, sl) -> int:
        """most tokens served as one sliced launch per token: `R.sliced_token_limit` (the measured table is there) of this layer and
        layout, remembered on the layout"""
        lim = sl.__dict__.get("_token_limit")
        if lim is None:
            lim = sl.__dict__["_token_limit"] = R.sliced_token_limit(self.vector_len, _res_centroids(self), _index_elements(self),
                                                                     sl.exact, sl.slices, len(sl.layout))
        return lim

    def _sliced_one_launch(self, sl, tokens: int) -> bool:
        """2 - 4 tokens in ONE launch over the layouts?  `R.sliced_one_launch` (the measured table is there) of this layer, the layout
        and the library's two answers for it, remembered on the layout per token count"""
        key = ("_one_launch", tokens)
        ok = sl.__dict__.get(key)
        if ok is None:
            ok = sl.__dict__[key] = R.sliced_one_launch(self.vector_len, _res_centroids(self), _index_elements(self), self.out_features, tokens,
                                                        sl.exact, sl.slices, sl.tokens_supported(tokens), sl.tokens_window_parts(tokens))
        return ok

    def _sliced_fits(self, cache, on) -> bool:
        """auto mode: build only while the layout (5 / 4 bytes per element + the builder's temporaries) leaves
        _SLICED_MIN_FREE_FRACTION of the device memory free, and never inside a stream capture"""
        if torch.cuda.is_current_stream_capturing():
            return False
        if on is True and "_sliced_on" in self.__dict__ or R._SLICED_LAYOUT_ALWAYS:
            return True
        free, total = torch.cuda.mem_get_info(cache.device)
        from vptq_amd.utils.sliced import device_builder_enabled
        need = R.sliced_build_bytes(_index_elements(self), B.lib().vptq_sliced_layout_tables(cache.desc) == 2,   # (one layout per table)
                                    device_builder_enabled(self._parameters["indices"]))
        return free - need > R._SLICED_MIN_FREE_FRACTION * total

    def _sliced_cached(self, x: torch.Tensor, tokens: int):
        """1 - 4 tokens over this layer's sliced layout(s): y, or None where they do not serve the call (no layout, a launch flag
        that rules them out, a token count no rule routes, a launch that steps aside) - `_gemv_cached` goes on with its own route.
        Siblings first, then the layer's own launch."""
        if "_sliced_cand" not in self.__dict__:
            # (static module configuration: decided once, so that every other layer pays one dict look-up per call)
            self.__dict__["_sliced_cand"] = R.has_sliced_format(self.vector_len, self.num_centroids, self.num_codebooks, self.enable_outlier, self.enable_norm)
        sl = self._sliced_gemv() if self.__dict__["_sliced_cand"] else None
        gf = ops.quant_gemm_flags()
        if sl is None or gf & B.GEMV_FORCE_GENERIC or not (sl.exact or not (gf & B.GEMV_EXACT)):
            return None
        if tokens == 1 or (tokens <= 4 and self._sliced_one_launch(sl, tokens) and x.is_contiguous()):
            sib = self.__dict__.get("_siblings")
            if sib is not None:      # q / k / v, gate / up: one sliced launch for the group
                y = sib.forward_sliced(self, x, tokens)
                if y is not None:
                    return y
            # (None: misaligned activation, capture on a stream the layer has not run on / without a workspace yet, ...)
            return sl(x) if tokens == 1 else sl.forward_tokens(x)
        if tokens <= self._sliced_token_limit(sl) and x.is_contiguous() and (self.in_features * x.element_size()) % 16 == 0:
            # 2 (the 4-bit format: 3) tokens of a LARGE layer = one launch per token over the layouts: the gather
            # kernels cost about as much for one token as for four (they are bound by the table gathers, not by
            # the FMAs), the sliced kernel a third to a half of that per token (profiles/r04/sliced_tokens.txt)
            x2 = x.reshape(tokens, self.in_features)
            y = torch.empty(x.shape[:-1] + (self.out_features,), dtype=x.dtype, device=x.device)
            y2 = y.view(tokens, self.out_features)
            for t in range(tokens):
                if sl(x2[t], y2[t]) is None:
                    return None
            return y
        return None

    def _gemv_cached(self, x: torch.Tensor, tokens: int) -> torch.Tensor:
        """Decode fast path: identical to `ops.quant_gemm` for 1..8 (canonical format: 16) tokens with a cached
        descriptor; layers linked by `link_siblings` share one grouped launch."""
        if tokens <= _SLICED_MAX_TOKENS and self.__dict__.get("_sliced_cand", True) and (_SLICED_LAYOUT_ENV or "_sliced_on" in self.__dict__ or
                                                                                         "_compact" in self.__dict__):
            y = self._sliced_cached(x, tokens)   # (1 - 4 tokens over the sliced layouts, where a rule of vptq_amd/sliced_routes.py takes the call)
            if y is not None:
                return y
        group = self.__dict__.get("_siblings")
        if group is not None and tokens <= group.MAX_TOKENS:
            y = group.forward(self, x, tokens)
            if y is not None:
                return y
        _, desc, _, dev, fn, _, _, wdtype, dev_index, safe_flags, ws_bytes = self._descriptor()
        # (the checks of _check_activation against the cached dtype / device: no module attribute look-ups)
        if x.shape[-1] != self.in_features:
            raise RuntimeError(f"x has {x.shape[-1]} features, layer expects {self.in_features}")
        if x.dtype != wdtype:
            raise RuntimeError(f"activation dtype {x.dtype} != weight dtype {wdtype}")
        if x.device != dev:
            if not x.is_cuda:
                raise RuntimeError("vptq_amd has no CPU path: x must be on the GPU")
            raise RuntimeError(f"tensors on different devices: {dev} vs {x.device}")
        if not x.is_contiguous():
            x = x.contiguous()
        y = torch.empty(x.shape[:-1] + (self.out_features,), dtype=wdtype, device=dev)
        # the current stream of the layer's device as a raw handle (torch.cuda.current_stream builds a
        # Stream object per call: 4 us of the 15 this function took)
        cp = self.__dict__.get("_compact")
        if torch.cuda.current_device() != dev_index:
            with torch.cuda.device(dev):
                sp = B.current_stream_ptr(dev)
                if cp is not None:
                    desc = self._repacked_desc(desc, dev_index, sp)
                ws, wsb = B.gemv_workspace(dev_index, sp, ws_bytes) if tokens > 1 else (None, 0)
                rc = fn(desc, x.data_ptr(), y.data_ptr(), tokens, ops.quant_gemm_flags() | safe_flags, ws, wsb, sp)
        else:
            sp = _raw_stream(dev_index)
            if cp is not None:   # (compact mode: the packed stream rebuilt into this stream's scratch first)
                desc = self._repacked_desc(desc, dev_index, sp)
            # 2+ tokens of the canonical format: the one-pass batched-decode kernel wants scratch memory
            ws, wsb = B.gemv_workspace(dev_index, sp, ws_bytes) if tokens > 1 else (None, 0)
            rc = fn(desc, x.data_ptr(), y.data_ptr(), tokens, ops.quant_gemm_flags() | safe_flags, ws, wsb, sp)
        if rc == -5 and tokens > B.GEMV_ANY_FORMAT_TOKENS:
            # VPTQ_E_TOKENS: the fused path takes this layer's 17+ tokens only under run-time conditions the
            # descriptor cannot promise (16-byte aligned activations, no FORCE_* flag): the dense route
            return self._dense_cached(x)
        if rc:
            B.check(rc, "vptq_quant_gemv")
        return y

    def _batched_decode_routes(self) -> tuple:
        """the batched-decode routes that can ever serve this layer (`batched_decode_routes` of its static configuration) and whose
        entry this process's library has: decided once per layer, so that every other layer pays one dict look-up per call"""
        routes = self.__dict__.get("_bd_routes")
        if routes is None:
            lib = B.lib()
            routes = tuple(r for r in batched_decode_routes(self.vector_len, self.num_centroids, _res_centroids(self), self.num_codebooks,
                                                            self.enable_outlier, self.enable_norm, bool(self.enable_perm))
                           if getattr(lib, r.entry, None) is not None)
            self.__dict__["_bd_routes"] = routes
        return routes

    def _batched_decode_cached(self, x: torch.Tensor, tokens: int):
        """5 - 64 tokens in ONE launch of the first batched-decode route (vptq_amd/batched_decode.py) that takes this call: its route
        function gives the layer's (format, shape, tokens) to it, its off-flags are not set, the layer's arithmetic is the
        reference's roundings where the kernel has no other, and the library serves the layer.  None: the routes of before - also
        where x is not what the entries take (the other routes raise the shape / dtype / device errors) or where a stream capture
        is in progress and the stream's workspace is too small for x[perm] (`prepare_model` sizes it).  Compact layers hand the
        entry the repacked stream, as the gather route does."""
        D = self.__dict__
        routes = D.get("_bd_routes")
        if routes is None:
            routes = self._batched_decode_routes()
        cache, gf, kr, perm = None, ops.quant_gemm_flags(), _res_centroids(self), bool(self.enable_perm)
        for r in routes:
            if not batched_decode_takes(r, self.vector_len, self.num_centroids, kr, self.out_features, self.in_features, tokens, gf, perm):
                continue
            if cache is None:
                cache = self._descriptor()
                if x.shape[-1] != self.in_features or x.dtype != cache.dtype or x.device != cache.device:
                    return None
                if not x.is_contiguous():
                    x = x.contiguous()
                if x.data_ptr() % 16:
                    return None
                ok = D.get("_bd_supported")
                if ok is None or ok[0] != cache.generation:
                    ok = D["_bd_supported"] = (cache.generation, {})
            if r.exact_only and not (cache.arithmetic_flags & B.GEMV_EXACT):
                continue
            # `_supported` is asked at the call's own token count, as `ops.quant_gemm` asks it: every entry's answer depends on the
            # count only through its window, and through which side of 16 tokens it lies where the inner kernel changes there (px)
            key = (r.entry, tokens > GEMM_GATHER_MAX_TOKENS)
            served = ok[1].get(key)
            if served is None:
                served = ok[1][key] = bool(getattr(B.lib(), r.entry + "_supported")(cache.desc, tokens))
            if served:
                y = ops.quant_gemm_batched_launch(r.entry, cache.desc, x, self.out_features, gf | cache.arithmetic_flags, r.workspace,
                                                  self._repacked_desc if "_compact" in D else None)
                if y is not None:
                    return y
        return None

    def _gemm_gather_px_workspace_bytes(self) -> int:
        """bytes of stream workspace the largest call the permuted-layer route (`vptq_quant_gemm_gather_px`) can take for this
        layer needs (`prepare_model` grows the stream's buffer to it); 0: the layer never takes that route"""
        if "_compact" not in self.__dict__ and not self._parameters["indices"].is_cuda:
            return 0
        px = [r for r in self._batched_decode_routes() if r.workspace]
        if not px:
            return 0
        routed = [t for t in range(px[0].min_tokens, px[0].max_tokens + 1)
                  if px[0].route(self.vector_len, self.num_centroids, _res_centroids(self), self.out_features, self.in_features, t)]
        query = getattr(B.lib(), px[0].entry + "_workspace_bytes", None)
        if not routed or query is None:
            return 0
        return int(query(self._descriptor().desc, routed[-1]))

    def _dense_cached(self, x: torch.Tensor) -> torch.Tensor:
        """Many tokens: `vptq_dequant` into a fresh dense W + `F.linear` (the reference's route,
        vptq/ops/quant_gemm.py:231-274) - what `ops.quant_gemm` does, with the descriptor (and its
        argsort(perm)) cached: marshalling 28 keyword arguments and rebuilding the descriptor cost
        ~45 us of Python per layer, a third of the prompt pass of an 8B-shaped model at 128 tokens."""
        cache = self._descriptor()
        dev, wdtype, dev_index = cache.device, cache.dtype, cache.device_index
        if x.shape[-1] != self.in_features:
            raise RuntimeError(f"x has {x.shape[-1]} features, layer expects {self.in_features}")
        if x.dtype != wdtype:
            raise RuntimeError(f"activation dtype {x.dtype} != weight dtype {wdtype}")
        if x.device != dev:
            raise RuntimeError(f"tensors on different devices: {dev} vs {x.device}")
        dense = self.__dict__.get("_desc_dense")
        if dense is None or dense[0] != cache.generation:
            desc, keep = B.make_layer_desc(bias=None, need_inv_perm=True, **self._layer_desc_keywords())
            dense = (cache.generation, desc, keep, B.lib().vptq_dequant)
            self.__dict__["_desc_dense"] = dense
        _, desc, _, dequant = dense
        W = torch.empty((self.out_features, self.in_features), dtype=wdtype, device=dev)
        cp = self.__dict__.get("_compact")
        # (compact mode: W straight from the layout where that is the faster route - no repack, no scratch; `R.dense_from_layout`)
        sl = self._sliced_gemv() if cp is not None and self._dense_from_layout() else None
        if torch.cuda.current_device() != dev_index:
            with torch.cuda.device(dev):
                sp = B.current_stream_ptr(dev)
                if sl is not None:
                    sl.dequant(W, sp)
                    rc = 0
                else:
                    rc = dequant(desc if cp is None else self._repacked_desc(desc, dev_index, sp), W.data_ptr(), sp)
        else:
            sp = _raw_stream(dev_index)
            if sl is not None:
                sl.dequant(W, sp)
                rc = 0
            else:
                rc = dequant(desc if cp is None else self._repacked_desc(desc, dev_index, sp), W.data_ptr(), sp)
        if rc:
            B.check(rc, "vptq_dequant")
        return torch.nn.functional.linear(x, W, self._parameters.get("bias"))

    def _dense_from_layout(self) -> bool:
        """does this COMPACTED layer build its dense W with `vptq_dequant_sliced`?  (`R.dense_from_layout` of its shape and of whether
        the library has the entry)"""
        return R.dense_from_layout(self.out_features, self.in_features, getattr(B.lib(), "vptq_dequant_sliced", None) is not None)

    def dequant(self) -> torch.Tensor:
        """Dense W[out_features, in_features] (what the reference calls
        `ops.dequant(...)` with this layer's fields)."""
        if "_compact" in self.__dict__ and self._dense_from_layout():
            return self._sliced_gemv().dequant()   # (compact mode: straight from the layout, the same bits)
        return ops.dequant(
            indices=self.packed_indices(), centroids=self.centroids.weight,
            outlier_indices=self.outlier_indices,
            outlier_centroids=self.outlier_centroids.weight if self.enable_outlier else None,
            res_indices=None,
            res_centroids=self.res_centroids.weight if self.enable_residual else None,
            perm=self.perm if self.enable_perm else None, weight_scale=self.weight_scale,
            weight_bias=self.weight_bias, is_indice_packed=True,
            enable_outlier=self.enable_outlier, enable_residual=self.enable_residual,
            enable_perm=self.enable_perm, enable_norm=self.enable_norm,
            num_centroids=self.num_centroids, num_outlier_centroids=self.num_outlier_centroids,
            num_res_centroids=self.num_res_centroids, padding=self.padding,
            outlier_padding=self.outlier_padding, num_codebooks=self.num_codebooks,
            group_size=self.group_size, outlier_size=self.outlier_size,
            vector_len=self.vector_len, outlier_vector_len=self.outlier_vector_len)

    # ---- compact mode: the exact sliced layout as the ONLY copy of the indices ----------------------------------------------------
    # The exact layout (vptq_amd/utils/sliced.py, SlicedGemv(exact=True)) holds every bit of the packed stream (include/vptq_hip.h,
    # vptq_sliced_layout_repack), so a layer served from it at one token can drop its packed `indices`: about a third of the resident
    # weights of the large-codebook formats.  1 - 4 tokens take the sliced kernels as before; the dense route (many tokens) and
    # dequant() of layers up to 4096 x 4096 build W straight from the layout (vptq_dequant_sliced: the bits of vptq_dequant, no packed
    # stream in between; `dense_from_layout` in vptq_amd/sliced_routes.py has the rule and its numbers); every path that still reads the packed stream (the
    # gather kernels of 5 - 8 tokens, the dense route of larger layers, state_dict(), shards, copies) gets it rebuilt by the repack kernel - into a per-stream scratch buffer for launches,
    # into a fresh tensor otherwise.  `indices` is a meta-device parameter of the same shape meanwhile.

    def compact(self, force: bool = False) -> int:
        """Hold this layer's indices in its exact sliced layout only; returns the bytes freed (0: not compacted - the reason is
        `layer.compact_skipped`).  Without `force`, only layers the product already serves from an exact layout at one token
        (the reference arithmetic's rule `R.exact_route_is_large`): their one-token speed is unchanged by construction.  Refused, the
        layer untouched, for: formats without an exact layout, non-zero bits past G T in a row, a stream capture, a layout build
        that runs out of device memory.  A compacted layer takes the reference's roundings in every arithmetic; `.to()` refuses
        it (`uncompact()` first); `load_state_dict` uncompacts it."""
        if "_compact" in self.__dict__:
            return 0
        why = self._compact_refusal(force)
        if why is None:
            why = self._compact_install()
        self.__dict__["compact_skipped"] = why
        return 0 if why else self.__dict__["_compact"]["packed_bytes"]

    def _compact_refusal(self, force: bool):
        """None, or why this layer cannot be compacted (nothing is changed here)"""
        from vptq_amd.utils.sliced import exact_column_parts, tail_bits_clear
        ind = self._parameters["indices"]
        if not R.has_sliced_format(self.vector_len, self.num_centroids, self.num_codebooks, self.enable_outlier, self.enable_norm):
            return f"format has no exact sliced layout ({_SLICED_FORMATS})"
        if not tail_bits_clear(ind.detach(), self.group_size, self.total_index_bits):
            return "non-zero bits past group_size x index bits in a row of the packed indices: a layout cannot hold them"
        if not ind.is_cuda:
            return "indices are not on a ROCm device"
        if torch.cuda.is_current_stream_capturing():
            return "inside a stream capture"
        if not exact_column_parts(self._descriptor().desc, self.group_size)[0]:
            return "no exact sliced layout serves this layer (too wide, or the format's LDS budget)"
        if not force and not R.exact_route_is_large(self.vector_len, _res_centroids(self), _index_elements(self)):
            return "one token takes the gather kernel for this layer (smaller than the exact sliced route's threshold; force=True compacts it)"
        return None

    def _compact_install(self):
        from vptq_amd.utils.sliced import SlicedGemv
        ind = self._parameters["indices"]
        cache = self._descriptor()
        st = self.__dict__.get("_sliced")
        sl = st[1] if st is not None and st[0] == (cache.generation, B.tensor_version(ind)) else None
        if sl is None or not sl.exact:
            try:
                sl = SlicedGemv(self, exact=True)
            except torch.cuda.OutOfMemoryError as e:
                torch.cuda.empty_cache()
                return f"out of device memory building the exact layout ({str(e)[:120]})"
        with torch.cuda.device(cache.device):
            same = torch.equal(sl.repack(), ind.detach())
        if not same:
            return "the repacked layout differs from the packed indices"
        w = ind.shape[2]
        packed_bytes = ind.numel() * ind.element_size()
        # the descriptors' `indices`: the layout's element words (the sliced entries check the pointer, never read through it; every
        # launch that reads the stream gets a copy pointing at a repack) - a [1, 1, row_words] view: the descriptor takes row_words
        # from its last dimension
        standin = sl.elems[:w].view(1, 1, w) if sl.elems.numel() >= w else torch.zeros(1, 1, w, dtype=torch.int32, device=sl.dev)
        self.__dict__["_compact"] = {"sl": sl, "gen": -1, "standin": standin, "shape": tuple(ind.shape), "packed_bytes": packed_bytes}
        self._parameters["indices"] = Parameter(torch.empty(ind.shape, dtype=ind.dtype, device="meta"), requires_grad=False)
        for k in ("_desc_cache", "_desc_dense", "_sliced", "_sliced_oom"):
            self.__dict__.pop(k, None)
        del ind, st
        if not self.__dict__.get("_compact_hooked"):
            self._register_state_dict_hook(_compact_state_dict_hook)
            self._register_load_state_dict_pre_hook(_compact_load_pre_hook, with_module=True)
            self.__dict__["_compact_hooked"] = True
        self._sliced_gemv()   # (the frozen descriptor: built over the layout's element words as the stand-in `indices` pointer)
        _COMPACTED.add(self)
        return None

    def is_compact(self) -> bool:
        return "_compact" in self.__dict__

    def packed_indices(self) -> torch.Tensor:
        """the packed int32 indices: the parameter itself, or (compacted) a fresh repack on the layer's device"""
        cp = self.__dict__.get("_compact")
        if cp is None:
            return self._parameters["indices"]
        return self._sliced_gemv().repack()

    def _repacked_desc(self, desc, dev_index: int, sp: int):
        """a copy of `desc` whose `indices` point at this stream's scratch, the packed stream rebuilt there (stream order)"""
        cp = self.__dict__["_compact"]
        sl = self._sliced_gemv()
        buf = B.compact_scratch(dev_index, sp, cp["packed_bytes"])
        B.check(B.lib().vptq_sliced_layout_repack(sl.desc, sl._lay_ref, sl.parts, buf.data_ptr(), sp), "vptq_sliced_layout_repack")
        d = B.LayerDesc.from_buffer_copy(desc)
        d.indices, d.prefetch, d.prefetch_bytes = buf.data_ptr(), None, 0
        return d

    def uncompact(self) -> None:
        """restore the packed `indices` parameter (from a repack); the layer then routes as any other"""
        cp = self.__dict__.get("_compact")
        if cp is None:
            return
        self._parameters["indices"] = Parameter(self.packed_indices(), requires_grad=False)
        self._compact_drop()

    def _compact_drop(self):
        for k in ("_compact", "_desc_cache", "_desc_dense", "_sliced", "_sliced_oom"):
            self.__dict__.pop(k, None)
        _COMPACTED.discard(self)

    def resident_bytes(self) -> dict:
        """device bytes of this layer's index data: packed indices, sliced layout tensors, its share of the compact-mode scratch
        (the per-stream buffers of its device divided among the compacted layers there)"""
        ind = self._parameters["indices"]
        packed = 0 if ind.is_meta else ind.numel() * ind.element_size()
        cp = self.__dict__.get("_compact")
        st = self.__dict__.get("_sliced")
        sl = cp["sl"] if cp is not None else (st[1] if st is not None else None)
        layout = 0
        if sl is not None:
            layout = sl.layout_bytes()
        scratch = 0
        if cp is not None:
            di = sl._dev_index
            peers = sum(1 for m in list(_COMPACTED) if m.__dict__.get("_compact") is not None and m._sliced_gemv()._dev_index == di)
            scratch = B.compact_scratch_bytes(di) // max(peers, 1)
        return {"packed": packed, "layout": layout, "scratch": scratch, "total": packed + layout + scratch}

    def _apply(self, fn, *args, **kwargs):
        if "_compact" in self.__dict__:
            raise RuntimeError("this VQuantLinear is compacted (its indices live in its sliced layout on its device): call "
                               "layer.uncompact() before moving or converting it")
        return super()._apply(fn, *args, **kwargs)

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, "
                f"v={self.vector_len}, k={self.num_centroids}, k_res={self.num_res_centroids}, "
                f"codebooks={self.num_codebooks}, group_size={self.group_size}, "
                f"outlier_size={self.outlier_size}, perm={self.enable_perm}, "
                f"norm={self.enable_norm}")
