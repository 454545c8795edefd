"""Load-time derived layout for large-codebook layers (v = 8, k = 65536, residual none, 256 or 65536: "v8-k65536-0",
"v8-k65536-256", "v8-k65536-65536"), the formats of most published VPTQ checkpoints, and the one-token GEMV over it
(`vptq_quant_gemv_sliced`, vptq_amd/csrc/gemv_sliced.hip).

The reference gathers centroid rows from the 1 MiB codebook through the caches for every index
(csrc/kernels/quant_gemv.cuh:11-186); on MI355X that is bound by the L2 -> L1 fill rate (39.6 us per 8192^2
layer).  Bucketing every row's elements ONCE by the top 3 (wide layers: 4) bits of their index
lets a workgroup keep its 8192- (4096-) entry slice of the codebook in LDS.  The state-dict tensors are untouched (they stay
the contract, and the many-token / dequant paths keep using them); the derived tensors cost 2x (T = 16) / 1.7x
(T = 24: 5 instead of 3 bytes per element) the packed indices in device memory on top.

    sl = SlicedGemv(layer)          # builds the layout (the library's builder for indices on a ROCm device: `layout_on_device`;
                                    # the torch recipe `layout_from_indices`, its model, otherwise)
    y = sl(x)                       # one token; same result as layer(x) within the parity bar

Round 5: `SlicedGemv(layer, exact=True)` - the reference's roundings per weight (the product default) over ONE layout bucketed by
the main index (a residual codebook other than v8's 256-entry one rides along as 16-bit indices, its entries gathered from L2);
layers too wide for that arithmetic's 6 bytes of LDS per column in one piece (28672 columns) as 2 - 3 COLUMN PARTS with a layout
each (`exact_column_parts`, `part_desc`); `forward_tokens` for 2 - 8 tokens: 2 / 3 in one pass of the one-token kernel where the
operands fit - whole (`tokens_window_parts` = 1) or in window parts (2 / 4) -, else column phases on the matrix pipe.
"""
from __future__ import annotations

import ctypes as C

import torch

from vptq_amd import _backend as B

INDEX_BITS = 16   # 65536 main centroids
WINDOWS = 4       # column windows the lists are ordered by (VPTQ_SLICED_WINDOWS in include/vptq_hip.h)


def window_cols(G: int) -> int:
    """columns per window: G / WINDOWS rounded up to a multiple of 8 (the last window takes what is left)"""
    return (G + WINDOWS * 8 - 1) // (WINDOWS * 8) * 8


def split_index_streams(indices: torch.Tensor, group_size: int, res_bits: int, index_bits: int = INDEX_BITS):
    """the layer's packed int32 `indices` [1, N, row_words] -> (main index [N, G] int64, residual index [N, G] int64 or None):
    a little-endian bit stream per row, element g at bits [T g, T g + T) with value (residual index << index_bits) | main
    index, T = index_bits + res_bits (vptq/utils/pack.py:26-89)."""
    assert indices.dtype == torch.int32 and indices.dim() == 3 and indices.shape[0] == 1
    from vptq_amd.utils.pack import unpack_index_tensor
    idx, ridx = unpack_index_tensor(indices, index_bits, group_size, res_bits, group_size, res_mask_bits=res_bits)
    return idx[0], (None if ridx is None else ridx[0])


def build_sliced_layout(indices: torch.Tensor, group_size: int, slices: int = 8, residual: bool = False):
    """indices: the layer's packed int32 `indices` [1, N, row_words] (T = 16 without a residual codebook, 24 with 256
    residual centroids).  slices: 8 or 16 (vptq_sliced_layout_supported tells).
    Returns (elems uint32-as-int32 [blocks * 64], blocks int32 [slices, N], first int32 [slices, N], res uint8
    [like elems] or None, wstart int32 [slices, N, WINDOWS + 1]) as described in include/vptq_hip.h (VptqSlicedLayout)."""
    idx, ridx = split_index_streams(indices, group_size, 8 if residual else 0)
    return layout_from_indices(idx, slices, ridx)


def layout_from_indices(idx: torch.Tensor, slices: int = 8, ridx: torch.Tensor = None, index_bits: int = INDEX_BITS,
                        whole_table: bool = False, side_dtype=torch.uint8):
    """idx [N, G] int64 (values < 2^index_bits): the index each element gathers with from the table this layout is for;
    ridx: a side index carried along per element, or None - 8 bits (the 256-entry residual table of v = 8, held in LDS) or, for
    the reference's roundings with any other residual codebook, 16 bits as int16 bit patterns (`side_dtype=torch.int16`: the
    residual entry is gathered from device memory).  Elements are
    bucketed by the top log2(slices) bits of idx and the element word carries idx inside its slice; or - whole_table:
    every workgroup of the table holds the whole (small) table - split into equal column ranges, the word carrying idx itself."""
    assert slices in (8, 16, 32) and 1 <= index_bits <= 16
    SLICES = slices
    lg = {8: 3, 16: 4, 32: 5}[slices]
    SLICE_BITS = max(index_bits - lg, 0)
    dev = idx.device
    N, G = idx.shape
    residual = ridx is not None
    col = torch.arange(G, device=dev, dtype=torch.int64)
    if whole_table:
        # every workgroup of the table holds all of it, so ANY split of a row's elements is valid: equal column ranges
        # (bucketing a 4- or 64-entry table by its index would leave most of the slices - workgroups - empty)
        sl = (col * SLICES // G)[None, :].expand(N, G).contiguous()
    else:
        sl = idx >> SLICE_BITS
    # Order inside a (row, slice) list is free (a sum): arrange it so that 16 CONSECUTIVE elements - the lanes one
    # pass of the kernel's ds_read_b128 gather serves - hit 16 different LDS bank groups (entry & 15): elements are
    # ranked inside their (slice, entry & 15) class and laid out rank-major, i.e. one element of every class in turn.
    # (Column order gave 3-way conflicts on average: SQ_LDS_BANK_CONFLICT = 60 % of the LDS cycles.)
    local = idx if whole_table else idx & ((1 << SLICE_BITS) - 1)
    cls = local & 15
    # ... and, before that, by COLUMN WINDOW (WINDOWS equal ranges of window_cols(G) columns): the kernel for 2 - 4 tokens
    # (gemv_sliced_tok.hip) stages one window of the activations at a time - T tokens of G / T columns fill the room one token of
    # G columns has - and walks the window's part of every list; `wstart` tells where it begins.  One token ignores it.
    wcols = window_cols(G)
    win = torch.clamp(col // wcols, max=WINDOWS - 1)[None, :].expand(N, G)
    sw = sl * WINDOWS + win
    order1 = torch.argsort((sw * 16 + cls) * G + col[None, :], dim=1)
    seg1 = torch.gather(sw * 16 + cls, 1, order1)                                       # sorted (slice, window, class) id
    cnt1 = torch.zeros(N, SLICES * WINDOWS * 16, dtype=torch.int64, device=dev)
    cnt1.scatter_add_(1, seg1, torch.ones_like(seg1))
    rank1 = col[None, :] - torch.gather(torch.cumsum(cnt1, 1) - cnt1, 1, seg1)          # rank inside the class
    # rank-major while every class still has an element (rows of 16 different classes); what is left over - the surplus of
    # the classes that have more than the smallest one - is spread evenly over the rest of the (slice, window) list (an
    # element's place = (its rank + 1/2) / its class's surplus of the way through), not bunched class by class at its end
    cnt3 = cnt1.reshape(N, SLICES * WINDOWS, 16)
    full = cnt3.min(2).values                                                               # complete rows per (slice, window)
    rest = cnt3.sum(2) - 16 * full
    b1 = seg1 >> 4
    full_e, rest_e, cnt_e = torch.gather(full, 1, b1), torch.gather(rest, 1, b1), torch.gather(cnt1, 1, seg1)
    spread = 16 * full_e + ((rank1 - full_e).double() + 0.5) * rest_e.double() / (cnt_e - full_e).clamp(min=1).double()
    place = torch.where(rank1 < full_e, (rank1 * 16 + (seg1 & 15)).double(), spread)
    order2 = torch.argsort((b1 * (2 * G)).double() + place + (seg1 & 15).double() / 64.0, dim=1)   # (slice, window, place)
    order = torch.gather(order1, 1, order2)
    s_sorted = torch.gather(sl, 1, order)
    word = order | (torch.gather(local, 1, order) << 16)                                # column | local << 16
    counts = torch.zeros(N, SLICES, dtype=torch.int64, device=dev)
    counts.scatter_add_(1, sl, torch.ones_like(sl))
    seg_start = torch.cumsum(counts, 1) - counts                                        # first position of (n, s) in the sorted row
    bs = 64                                                                             # elements per block
    blocks = (counts + bs - 1) // bs                                                    # [N, 8]
    blocks_sn = blocks.t().contiguous()                                                 # [8, N]
    first_sn = (torch.cumsum(blocks_sn.reshape(-1), 0) - blocks_sn.reshape(-1)).reshape(SLICES, N)
    total = int(blocks_sn.sum().item())
    elems = torch.full((max(total, 1) * bs,), G, dtype=torch.int64, device=dev)         # padding: column G, local 0
    pos = col[None, :] - torch.gather(seg_start, 1, s_sorted)                           # rank inside its (n, s) list
    rows = torch.arange(N, device=dev)[:, None].expand(N, G)
    dest = first_sn[s_sorted, rows] * bs + pos
    elems[dest.reshape(-1)] = word.reshape(-1)
    elems32 = (elems & 0xffffffff).to(torch.int64)
    elems32 = torch.where(elems32 >= (1 << 31), elems32 - (1 << 32), elems32).to(torch.int32)
    res = None
    if residual:
        res = torch.zeros(elems.numel(), dtype=side_dtype, device=dev)
        rv = torch.gather(ridx, 1, order).reshape(-1)
        if side_dtype == torch.int16:       # (uint16 bit patterns)
            rv = torch.where(rv >= 32768, rv - 65536, rv)
        res[dest.reshape(-1)] = rv.to(side_dtype)
    # wstart [slices][N][WINDOWS + 1]: position inside the (s, n) list at which window w begins; [WINDOWS] = the list's length
    cntw = torch.zeros(N, SLICES * WINDOWS, dtype=torch.int64, device=dev)
    cntw.scatter_add_(1, sw, torch.ones_like(sw))
    cntw = cntw.reshape(N, SLICES, WINDOWS)
    wstart = torch.zeros(N, SLICES, WINDOWS + 1, dtype=torch.int64, device=dev)
    wstart[:, :, 1:] = torch.cumsum(cntw, 2)
    wstart = wstart.permute(1, 0, 2).to(torch.int32).contiguous()
    return elems32, blocks_sn.to(torch.int32).contiguous(), first_sn.to(torch.int32).contiguous(), res, wstart


def device_builder_enabled(indices: torch.Tensor) -> bool:
    """is a layout of these packed indices built by the HIP kernel (`layout_on_device`)?  Indices on a ROCm device: yes; CPU
    tensors take the torch recipe above, which is also the kernel's model.  (A/B: VPTQ_TUNING=1 VPTQ_LAYOUT_BUILDER=torch.)"""
    return bool(indices.is_cuda) and (B.tune_env("VPTQ_LAYOUT_BUILDER", "hip") or "hip").strip().lower() != "torch"


def layout_on_device(indices: torch.Tensor, desc, slices: int, exact: bool = False, table: int = 0, whole_table: bool = False,
                     side_bytes: int = 0, parts: int = 1, part: int = 0, any_shape: bool = False):
    """The same 5-tuple as `layout_from_indices`, byte for byte, built from the PACKED int32 `indices` [1, N, row_words] on their
    ROCm device by the library (`vptq_sliced_layout_plan` / `_fill`, vptq_amd/csrc/layout_build.hip) on the current stream.  `desc`:
    the layer's descriptor (shape of the stream and the format; its `indices` pointer is replaced by the tensor's).  table 0 / 1: bucketed
    by the main / the residual index; side_bytes 0 / 1 / 2: no side stream / uint8 / uint16 (int16 bit patterns) residual indices;
    part of parts: the columns [part G / parts, (part + 1) G / parts).  any_shape: the spec is not checked against the layouts the
    GEMV entries take for the layer (tests, tools).  Device memory: the five tensors returned and one int64 - nothing else; one
    device -> host read (the number of blocks) between the two steps."""
    assert indices.dtype == torch.int32 and indices.dim() == 3 and indices.shape[0] == 1 and indices.is_cuda
    if not indices.is_contiguous():
        indices = indices.contiguous()
    dev = indices.device
    d = B.LayerDesc.from_buffer_copy(desc)
    d.indices, d.prefetch, d.prefetch_bytes = indices.data_ptr(), None, 0
    N = int(d.num_indices)
    lib = B.lib()
    spec = B.SlicedLayoutSpec((B.GEMV_EXACT if exact else 0) | (B.LAYOUT_ANY_SHAPE if any_shape else 0), int(slices), int(table),
                              int(bool(whole_table)), int(side_bytes), int(parts), int(part), 0)
    with torch.cuda.device(dev):
        sp = B.current_stream_ptr(dev)
        blocks = torch.empty(slices, N, dtype=torch.int32, device=dev)
        first = torch.empty(slices, N, dtype=torch.int32, device=dev)
        wstart = torch.empty(slices, N, WINDOWS + 1, dtype=torch.int32, device=dev)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        B.check(lib.vptq_sliced_layout_plan(d, spec, blocks.data_ptr(), first.data_ptr(), wstart.data_ptr(), total.data_ptr(), sp),
                "vptq_sliced_layout_plan")
        n_blocks = int(total.item())
        elems = torch.empty(max(n_blocks, 1) * 64, dtype=torch.int32, device=dev)
        res = torch.empty(elems.numel(), dtype=torch.uint8 if side_bytes == 1 else torch.int16, device=dev) if side_bytes else None
        out = B.SlicedLayout(elems.data_ptr(), blocks.data_ptr(), first.data_ptr(), res.data_ptr() if res is not None else None, 1, 1,
                             int(slices), int(bool(whole_table)), wstart.data_ptr())
        B.check(lib.vptq_sliced_layout_fill(d, spec, out, n_blocks, sp), "vptq_sliced_layout_fill")
    return elems, blocks, first, res, wstart


def repack_reference(layouts, group_size: int, index_bits: int, res_bits: int, row_words: int, slices: int) -> torch.Tensor:
    """Pure-torch model of `vptq_sliced_layout_repack` (tests and docs only): the packed int32 indices [1, N, row_words] rebuilt from
    the EXACT layout(s) `layout_from_indices` returned - one tuple (elems, blocks, first, res, wstart) per column part, part p
    covering columns [p G / parts, (p + 1) G / parts).  An element word is `column | local << 16`; the (slice, row) list it sits in
    gives index = slice << (index_bits - log2(slices)) | local; `res` (uint8, or int16 bit patterns) the residual index above it."""
    G, parts = group_size, len(layouts)
    T, w = index_bits + res_bits, group_size // len(layouts)
    sb = index_bits - {8: 3, 16: 4, 32: 5}[slices]
    N = layouts[0][1].shape[1]
    dev = layouts[0][0].device
    vals = torch.zeros(N, G, dtype=torch.int64, device=dev)
    for p, (e, b, f, r, _) in enumerate(layouts):
        # block k belongs to the (s, n) list with first[s, n] <= k < first[s, n] + blocks[s, n]: lists in (s, n) order
        sn = torch.repeat_interleave(torch.arange(b.numel(), device=dev), b.reshape(-1).to(torch.int64))
        sn = sn.repeat_interleave(64)
        word = e[:sn.numel()].to(torch.int64) & 0xFFFFFFFF
        col, local = word & 0xFFFF, word >> 16
        val = ((sn // N) << sb) | local
        if r is not None:
            val |= (r[:sn.numel()].to(torch.int64) & (0xFF if r.dtype == torch.uint8 else 0xFFFF)) << index_bits
        keep = col < w                       # (padding: column = part width)
        vals[(sn % N)[keep], p * w + col[keep]] = val[keep]
    bitpos = torch.arange(G, device=dev, dtype=torch.int64) * T
    shifted = vals << (bitpos & 31)
    flat = torch.zeros(N, row_words + 1, dtype=torch.int64, device=dev)
    flat.index_add_(1, bitpos >> 5, shifted & 0xFFFFFFFF)
    flat.index_add_(1, (bitpos >> 5) + 1, shifted >> 32)
    out = flat[:, :row_words]
    return torch.where(out >= 2**31, out - 2**32, out).to(torch.int32).reshape(1, N, row_words)


def tail_bits_clear(indices: torch.Tensor, group_size: int, total_bits: int) -> bool:
    """no bit past G T in any row of the packed indices (`pack_index` never writes one; a layout cannot hold one).  One device -> host read."""
    nbits = group_size * total_bits
    full, rem = nbits // 32, nbits % 32
    rows = indices.reshape(-1, indices.shape[-1])
    bad = rows[:, full + (1 if rem else 0):].ne(0).any()
    if rem:
        bad = bad | ((rows[:, full].to(torch.int64) & 0xFFFFFFFF) >> rem).ne(0).any()
    return not bool(bad.item())


def rows_per_wave_for(n_rows: int, slices: int = 8, workgroups: int = 256) -> int:
    """consecutive rows per wave so that slices x row blocks of 16 waves give about `workgroups` workgroups"""
    r = max(1, (n_rows * slices + 16 * workgroups - 1) // (16 * workgroups))
    return min(r, 64)


def part_desc(desc, c0: int, c1: int):
    """copy of a layer's descriptor that stands for its columns [c0, c1) alone (`VPTQ_GEMV_COLUMN_PARTS`, include/vptq_hip.h): widths
    and the column-order tensors advanced to c0 (16-bit elements).  The tensors stay owned by the layer's own descriptor.  The twin of
    the library's `sl_part_desc` (vptq_amd/csrc/sliced_host.hip), which the part rule of `vptq_sliced_layout_set` is stated with."""
    d = B.LayerDesc.from_buffer_copy(desc)
    d.in_features = d.group_size = c1 - c0
    for f in ("weight_scale", "weight_bias", "perm", "scale_permuted", "bias_permuted"):
        p = getattr(desc, f)
        if p:
            setattr(d, f, p + 2 * c0)
    return d


def layout_set(desc, exact: bool):
    """the layouts the library serves this layer from in one arithmetic (`vptq_sliced_layout_set`, include/vptq_hip.h): column parts
    (0: not served), tables per part, slices, which table is held whole, bytes per element of the residual side stream"""
    out = B.SlicedLayoutSet()
    B.check(B.lib().vptq_sliced_layout_set(desc, B.GEMV_EXACT if exact else 0, out), "vptq_sliced_layout_set")
    return out


def exact_column_parts(desc, group_size: int):
    """(parts, slices) with which the reference's roundings are served over sliced layouts: (1, n) where the layer fits in one
    piece, (2 or 3, n) where equal column parts of a multiple of 8 columns do (28672-column layers: 2 x 14336), (0, 0) else -
    the library's answer (`layout_set`), which reads the descriptor's own group_size: the argument is kept for the signature only"""
    s = layout_set(desc, True)
    return int(s.parts), int(s.n_slices)


def _layout_structs(tensors, whole, rpw: int, slices: int):
    """the `B.SlicedLayout` array of these layout tuples (elems, blocks, first, res, wstart); whole[i]: table i is held whole by its workgroups"""
    structs = [B.SlicedLayout(e.data_ptr(), b.data_ptr(), f.data_ptr(), r.data_ptr() if r is not None else None, rpw, 1, slices, int(w),
                              ws.data_ptr()) for (e, b, f, r, ws), w in zip(tensors, whole)]
    return (B.SlicedLayout * len(structs))(*structs)


def _launch_activation(obj, lay, x: torch.Tensor, tokens=None, served: bool = True):
    """The pre-checks of every entry point of `obj` (SlicedGemv / SlicedGroupGemv over layers like `lay`): x as the kernels take it, or None
    where the call cannot take them (not `served`; x - several tokens: or its rows - not 16-byte aligned).  tokens None: the one-token entry."""
    n = lay.in_features
    if tokens is None:
        if x.shape[-1] != n or x.numel() != n:
            raise ValueError("the sliced path takes one token of in_features values")
    elif x.shape[-1] != n or not 2 <= tokens <= 8:
        raise ValueError("forward_tokens takes 2 - 8 tokens of in_features values")
    elif not served:
        return None
    if x.dtype != obj._dtype or x.device != obj.dev:   # (the checks of VQuantLinear._check_activation: this is the per-token path)
        x = lay._check_activation(x)
    if not x.is_contiguous():
        x = x.contiguous()
    if x.data_ptr() & 15 or (tokens is not None and (n * x.element_size()) & 15):
        return None
    return x


def _new_output(obj, x: torch.Tensor, out_features: int, flags: int = 0):
    """the output tensor of a launch of `obj` over the activation x: its leading dimensions, float32 with `GEMV_OUT_F32`"""
    return torch.empty(x.shape[:-1] + (out_features,), dtype=torch.float32 if (flags & B.GEMV_OUT_F32) else obj._dtype, device=obj.dev)


def _launch_failed(rc: int, what: str, workspaces):
    """the tail of every launch whose return code is not 0: None where the library says "unsupported" (the caller takes the regular
    route); else the error, after zeroing the workspaces - a launch that did not happen or did not finish may have left accumulator
    words or arrival counters behind; the buffers themselves stay: a captured graph may hold their addresses"""
    if rc != B.E_UNSUPPORTED:
        for ws in workspaces:
            ws.zero_()
        B.check(rc, what)
    return None


class SlicedGemv:
    """One-token forward of a v8-k65536-0 `VQuantLinear` over its sliced layout."""

    def __init__(self, layer, rows_per_wave: int = 0, exact: bool = False, selective: bool = False):
        """exact: the reference's roundings per weight (`VPTQ_GEMV_EXACT`, the product default arithmetic) instead of the
        folded form - layers without a residual codebook or with the 256-entry one of v = 8; the layout then has the slice
        count that arithmetic needs (scale, bias and x of every column sit beside the slice in LDS).
        selective (round 6, one token): the FOLDED layouts with `VPTQ_GEMV_SELECTIVE` - a pre-pass finds the blocks of 128 columns an
        activation dominates, the folded launch reads them as zeros and adds their exact products (gemv_hot.hip)."""
        self.layer = layer
        self.exact = bool(exact)
        self.selective = bool(selective) and not self.exact
        self._flags = B.GEMV_EXACT if self.exact else (B.GEMV_SELECTIVE if self.selective else 0)
        if self.selective and not B.lib().vptq_quant_gemv_sliced_selective_supported(layer._descriptor().desc):
            raise ValueError("selective roundings over the sliced layouts: fp16 layers with scale and bias")
        cache = layer._descriptor()
        self.desc, self.dev = cache.desc, cache.device
        # (a layer too wide for the exact arithmetic's 6 bytes of LDS per column in one piece: equal column parts, one layout each; the
        # reference's roundings need c and r in one lane: always ONE table, a residual codebook other than v8's 256-entry one rides
        # along as a 16-bit side stream; folded: a second table whose slice would be under 16 KiB is held WHOLE by its workgroups)
        lset = layout_set(self.desc, self.exact)
        self.parts, self.slices, n_tables, side = int(lset.parts), int(lset.n_slices), int(lset.tables), int(lset.side_bytes)
        if not self.parts:
            raise ValueError("the sliced layout serves v = 8 / 16 layers with 16384 ... 65536 main centroids, group_size <= 32768"
                             " (reference roundings: one table, up to ~16000 columns)")
        self._side16 = side == 2
        ib, rb = int(self.desc.index_bits), int(self.desc.res_bits)
        packed = layer.indices.data
        if device_builder_enabled(packed):
            # indices on a ROCm device: the library builds the same tensors, byte for byte, from the packed stream (layout_build.hip) -
            # no index matrices, no sorts: the tensors themselves are the only memory the build takes
            def build(table, whole_table, side, part):
                return layout_on_device(packed, self.desc, self.slices, exact=self.exact, table=table, whole_table=whole_table,
                                        side_bytes=side, parts=self.parts, part=part)
        else:
            idx, ridx = split_index_streams(packed, layer.group_size, rb, ib)
            w = layer.group_size // self.parts

            def build(table, whole_table, side, part):
                cols = slice(part * w, (part + 1) * w)
                src, bits = (ridx, rb) if table else (idx, ib)
                return layout_from_indices(src[:, cols].contiguous(), self.slices, ridx[:, cols].contiguous() if side else None, bits,
                                           whole_table, side_dtype=torch.int16 if side == 2 else torch.uint8)
        # ((c + r) s x = c s x + r s x: a second table is a layout bucketed by ITS index; the side stream rides beside table 0)
        self._whole = [bool(lset.whole_table[t]) for _ in range(self.parts) for t in range(n_tables)]
        self._tensors = [build(t, bool(lset.whole_table[t]), 0 if t else side, p) for p in range(self.parts) for t in range(n_tables)]
        if self.parts > 1:
            self._part_descs = self._make_part_descs(self.desc)
        self.elems, self.blocks, self.first, self.res, self.wstart = self._tensors[0]
        # (a two-table layer runs 2 x slices workgroups per row block in its one launch)
        rpw = rows_per_wave or rows_per_wave_for(self.blocks.shape[1], self.slices * len(self._tensors))
        self.layout = _layout_structs(self._tensors, self._whole, rpw, self.slices)
        self._ws_bytes = B.lib().vptq_quant_gemv_sliced_workspace_bytes(self._part_descs[0] if self.parts > 1 else self.desc)
        if self.selective:   # (+ header, x with the hot blocks zeroed, the hot blocks' exact products)
            self._ws_bytes = B.lib().vptq_quant_gemv_sliced_workspace_bytes_for(self.desc, self._flags)
        if self.parts > 1:
            self._pp = ((C.c_void_p * self.parts)(), (C.c_void_p * self.parts)(), (C.c_size_t * self.parts)(*([self._ws_bytes] * self.parts)))
        # partial sums + arrival counters, ONE PER STREAM (two streams - or a graph replay next to an eager call on
        # another stream - running the same layer would race on a shared one); zeroed once, every call leaves the
        # counters zero
        self._ws = {}
        self._ws_tok = {}   # stream -> workspace of the 2 - 8 token kernel
        self._retired = []  # workspaces that were ever handed to a launch stay alive as long as the layer does
        self._fn = B.lib().vptq_quant_gemv_sliced
        self._fn_tok = B.lib().vptq_quant_gemv_sliced_tokens
        self._lay_ref = self.layout   # (an array of 1 or 2 structs: passed as a pointer to the first)
        self._dtype = cache.dtype
        self._dev_index = cache.device_index
        self.extra_bytes = sum(e.numel() * (4 + (r.element_size() if r is not None else 0)) + b.numel() * 8 for e, b, f, r, _ in self._tensors)

    def _make_part_descs(self, desc):
        """one descriptor per column part of `desc` (`part_desc`), as the array the grouped entries take"""
        w = self.layer.group_size // self.parts
        return (B.LayerDesc * self.parts)(*[part_desc(desc, p * w, (p + 1) * w) for p in range(self.parts)])

    def layout_bytes(self) -> int:
        """device bytes of the layout tensors"""
        return sum(t.numel() * t.element_size() for tup in self._tensors for t in tup if t is not None)

    def repack(self, out: torch.Tensor = None) -> torch.Tensor:
        """the layer's packed int32 indices rebuilt from this EXACT layout on the current stream (`vptq_sliced_layout_repack`): into
        `out` (int32, the shape of `indices`, 16-byte aligned) or a fresh tensor"""
        if not self.exact:
            raise ValueError("only an exact layout holds the packed stream")
        shape = (1, int(self.desc.num_indices), int(self.desc.row_words))
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=self.dev)
        with torch.cuda.device(self.dev):
            B.check(B.lib().vptq_sliced_layout_repack(self.desc, self._lay_ref, self.parts, out.data_ptr(),
                                                      B.current_stream_ptr(self.dev)), "vptq_sliced_layout_repack")
        return out

    def dequant(self, out: torch.Tensor = None, stream: int = None) -> torch.Tensor:
        """the layer's dense W [out_features, in_features] straight from this EXACT layout (`vptq_dequant_sliced`): bit for bit what
        `vptq_dequant` writes for the packed indices the layout was built from, without rebuilding them.  Into `out` (the layer's
        dtype, contiguous, 16-byte aligned) or a fresh tensor; on `stream` (a raw handle of the layer's device) or the current one."""
        if not self.exact:
            raise ValueError("only an exact layout holds the packed stream")
        if out is None:
            out = torch.empty((int(self.desc.out_features), int(self.desc.in_features)), dtype=self._dtype, device=self.dev)
        if stream is None:
            with torch.cuda.device(self.dev):
                stream = B.current_stream_ptr(self.dev)
        B.check(B.lib().vptq_dequant_sliced(self.desc, self._lay_ref, self.parts, out.data_ptr(), stream), "vptq_dequant_sliced")
        return out

    def rebound(self, desc) -> "SlicedGemv":
        """a copy of this object over the same layout tensors and workspaces for another descriptor of the same layer (a compacted
        layer's descriptor is rebuilt after set_arithmetic or a parameter change; its layout never is)"""
        import copy
        new = copy.copy(self)
        new.desc = desc
        if self.parts > 1:
            new._part_descs = self._make_part_descs(desc)
        return new

    def _workspace(self, stream_ptr: int):
        ws = self._ws.get(stream_ptr)
        if ws is None:
            if torch.cuda.is_current_stream_capturing():
                return None   # (no allocation + memset inside a capture: warm the layer up on the capture stream first)
            ws = torch.zeros(self._ws_bytes, dtype=torch.uint8, device=self.dev)
            self._ws[stream_ptr] = ws
        return ws

    def __call__(self, x: torch.Tensor, out: torch.Tensor = None, flags: int = 0):
        """y, or None where this call cannot take the sliced kernel (activation not 16-byte aligned, no workspace for a
        capturing stream, the library says "unsupported"): the caller then takes the regular route."""
        x = _launch_activation(self, self.layer, x)
        if x is None:
            return None
        if torch.cuda.current_device() != self._dev_index:
            with torch.cuda.device(self.dev):
                return self._launch(x, out, flags)
        return self._launch(x, out, flags)

    def tokens_supported(self, tokens: int) -> bool:
        """does the library's kernel for 2 - 4 tokens over these layouts take this layer (its activations must fit the LDS
        beside the slice in at most 4 column phases)?"""
        if self.exact and (self.parts > 1 or self._side16):   # (column parts, and the reference's roundings over two-table formats:
            return self.tokens_one_pass(tokens)               # 2 / 3 tokens where every part takes them in one pass, nothing else)
        if self.selective:                   # (one token: several tokens of such a layer take the module's regular route)
            return False
        return bool(B.lib().vptq_quant_gemv_sliced_tokens_supported_for(self.desc, self._lay_ref, int(tokens), self._flags))

    def tokens_one_pass(self, tokens: int) -> bool:
        """(reference roundings) does the library take these 2 / 3 tokens in ONE PASS of the one-token kernel (gemv_sliced.hip, TOK:
        slice + (2 tokens + 4) bytes per column fit the LDS) - the route that needs no column windows?"""
        if not self.exact or not 2 <= tokens <= 3:
            return False
        return self.tokens_window_parts(tokens) >= 1

    def tokens_window_parts(self, tokens: int) -> int:
        """0, or in how many window parts the library takes these tokens in one pass: 1 = every column staged beside the slice; 2 / 4 =
        that many workgroups per (slice, row block), each with its column windows (`vptq_quant_gemv_sliced_tokens_one_pass`)"""
        if not self.exact or not 2 <= tokens <= 3:
            return 0
        key = ("_one_pass", tokens)
        n = self.__dict__.get(key)
        if n is None:
            d = self._part_descs[0] if self.parts > 1 else self.desc     # (column parts: every part is asked - they have one width)
            n = int(B.lib().vptq_quant_gemv_sliced_tokens_one_pass(d, int(tokens), self._flags))
            if n and not B.lib().vptq_quant_gemv_sliced_tokens_supported_for(d, self._lay_ref, int(tokens), self._flags):
                n = 0
            self.__dict__[key] = n
        return n

    def forward_tokens(self, x: torch.Tensor, out: torch.Tensor = None, flags: int = 0):
        """2 - 4 tokens in ONE launch (`vptq_quant_gemv_sliced_tokens`, gemv_sliced_tok.hip): x [..., in_features] with 2 - 4
        rows, contiguous.  Returns y, or None where the call cannot be served (the caller takes the regular route)."""
        tokens = x.numel() // self.layer.in_features
        x = _launch_activation(self, self.layer, x, tokens, not (
            self.selective or (self.exact and (self.parts > 1 or self._side16) and not self.tokens_one_pass(tokens))))
        if x is None:
            return None
        if torch.cuda.current_device() != self._dev_index:
            with torch.cuda.device(self.dev):
                return self._launch_tokens(x, out, flags, tokens)
        return self._launch_tokens(x, out, flags, tokens)

    def _tokens_workspace(self, stream_ptr: int, tokens: int = 4):
        """the workspace of the token kernel for this stream, or None inside a capture on a stream the layer has not run on.
        Sized ONCE for the most tokens the library serves for this layer (8, else 4 - a workspace for T tokens serves fewer)
        and never replaced or freed afterwards: a hipGraph captured on this stream holds its address (one workspace per
        stream = per capture; a graph replayed on another stream than the one it was captured on races with eager calls on
        the first - replay where you captured)."""
        ws = self._ws_tok.get(stream_ptr)
        need = 8 if tokens > 4 else 4
        if ws is None or ws[1] < need:
            if torch.cuda.is_current_stream_capturing():
                return None
            wd = self._part_descs[0] if self.parts > 1 else self.desc
            size, nbytes = 8, B.lib().vptq_quant_gemv_sliced_tokens_workspace_bytes(wd, 8)
            if not nbytes:
                size, nbytes = 4, B.lib().vptq_quant_gemv_sliced_tokens_workspace_bytes(wd, 4)
            if not nbytes or size < need:
                return None
            if ws is not None:
                self._retired.append(ws[0])   # (cannot happen with the sizing above; kept alive if it ever does)
            ws = (torch.zeros(nbytes, dtype=torch.uint8, device=self.dev), size)
            self._ws_tok[stream_ptr] = ws
        return ws[0]

    def _launch_tokens(self, x, out, flags, tokens):
        sp = B.current_stream_ptr(self.dev)
        ws = self._tokens_workspace(sp, tokens)
        if ws is None:
            return None
        if out is None:
            out = _new_output(self, x, self.layer.out_features, flags)
        if self.parts > 1:   # column parts of one layer: one grouped launch, shared output and workspace
            yp, wp, _ = self._pp
            for i in range(self.parts):
                yp[i] = out.data_ptr()
                wp[i] = ws.data_ptr()
            wb = (C.c_size_t * self.parts)(*([ws.numel()] * self.parts))
            rc = B.lib().vptq_quant_gemv_sliced_tokens_grouped(self._part_descs, self._lay_ref, self.parts, x.data_ptr(), yp, tokens,
                                                               flags | self._flags | B.GEMV_COLUMN_PARTS, wp, wb, sp)
        else:
            rc = self._fn_tok(self.desc, self._lay_ref, x.data_ptr(), out.data_ptr(), tokens, flags | self._flags, ws.data_ptr(), ws.numel(), sp)
        return _launch_failed(rc, "vptq_quant_gemv_sliced_tokens", (ws,)) if rc else out

    def _launch(self, x, out, flags):
        sp = B.current_stream_ptr(self.dev)
        ws = self._workspace(sp)
        if ws is None:
            return None
        if out is None:   # (written out, here and in SlicedGroupGemv._launch: the one-token path, a call per token and layer)
            out = torch.empty(x.shape[:-1] + (self.layer.out_features,),
                              dtype=torch.float32 if (flags & B.GEMV_OUT_F32) else self._dtype, device=self.dev)
        if self.parts > 1:   # column parts of one layer: one grouped launch, shared output and accumulator words
            yp, wp, wb = self._pp
            for i in range(self.parts):
                yp[i] = out.data_ptr()
                wp[i] = ws.data_ptr()
            rc = B.lib().vptq_quant_gemv_sliced_grouped(self._part_descs, self._lay_ref, self.parts, x.data_ptr(), yp,
                                                        flags | self._flags | B.GEMV_COLUMN_PARTS, wp, wb, sp)
        else:
            rc = self._fn(self.desc, self._lay_ref, x.data_ptr(), out.data_ptr(), flags | self._flags, ws.data_ptr(), self._ws_bytes, sp)
        return _launch_failed(rc, "vptq_quant_gemv_sliced", (ws,)) if rc else out


class SlicedGroupGemv:
    """One token through up to 3 sibling layers (q / k / v, gate / up: one format, one input width, the SAME activation)
    in ONE launch of the sliced kernel (`vptq_quant_gemv_sliced_grouped`): the fixed part of a sliced launch - boundary,
    slice copy, staging, the cross-slice hand-over: ~7 of the 10 us of a 4096 x 4096 layer - is paid once.  `members`:
    the layers' `SlicedGemv` objects (their tensors are shared, only the rows per wave are the group's)."""

    def __init__(self, members):
        self.members = list(members)
        n = len(self.members)
        m0 = self.members[0]
        tables = len(m0.layout)
        kind = lambda m: (m.layer.vector_len, m.layer.num_centroids,   # noqa: E731
                          m.layer.num_res_centroids if m.layer.enable_residual else 0, tuple(m._whole), m.exact)
        if not 1 <= n <= 3 or any(m.parts > 1 or getattr(m, "selective", False) for m in self.members) or any(len(m.layout) != tables or m.slices != m0.slices or m._dtype != m0._dtype or m.dev != m0.dev or
                                  m.layer.in_features != m0.layer.in_features or kind(m) != kind(m0) for m in self.members):
            raise ValueError("a sliced group takes 1..3 layers of one format (vector length, codebook sizes), dtype, device and input width")
        rpw = rows_per_wave_for(sum(m.blocks.shape[1] for m in self.members), m0.slices * tables)   # one round of workgroups over ALL layers
        self.layouts = _layout_structs([t for m in self.members for t in m._tensors], [w for m in self.members for w in m._whole], rpw, m0.slices)
        self.descs = (B.LayerDesc * n)(*[m.desc for m in self.members])
        self._yp, self._wp = (C.c_void_p * n)(), (C.c_void_p * n)()
        self._wb = (C.c_size_t * n)(*[m._ws_bytes for m in self.members])
        self._fn = B.lib().vptq_quant_gemv_sliced_grouped
        self.dev, self._dtype, self._dev_index = m0.dev, m0._dtype, m0._dev_index
        self.exact, self._flags, self._side16 = m0.exact, m0._flags, m0._side16

    def __call__(self, x: torch.Tensor):
        """list of outputs (one per member), or None where the call cannot take the sliced kernel (as SlicedGemv.__call__)"""
        x = _launch_activation(self, self.members[0].layer, x)
        if x is None:
            return None
        if torch.cuda.current_device() != self._dev_index:
            with torch.cuda.device(self.dev):
                return self._launch(x)
        return self._launch(x)

    def tokens_supported(self, tokens: int) -> bool:
        return all(m.tokens_supported(tokens) for m in self.members)

    def forward_tokens(self, x: torch.Tensor):
        """2 - 4 tokens through every member in ONE launch (`vptq_quant_gemv_sliced_tokens_grouped`): list of outputs, or None
        where the call cannot be served (as SlicedGemv.forward_tokens)"""
        lay = self.members[0].layer
        tokens = x.numel() // lay.in_features
        x = _launch_activation(self, lay, x, tokens, not (self.exact and self._side16 and not all(m.tokens_one_pass(tokens) for m in self.members)))
        if x is None:
            return None
        if torch.cuda.current_device() != self._dev_index:
            with torch.cuda.device(self.dev):
                return self._launch_tokens(x, tokens)
        return self._launch_tokens(x, tokens)

    def _launch_tokens(self, x, tokens):
        sp = B.current_stream_ptr(self.dev)
        wss = []
        for m in self.members:
            ws = m._tokens_workspace(sp, tokens)
            if ws is None:
                return None
            wss.append(ws)
        ys = [_new_output(self, x, m.layer.out_features) for m in self.members]
        wb = (C.c_size_t * len(wss))(*[w.numel() for w in wss])
        for i, (y, w) in enumerate(zip(ys, wss)):
            self._yp[i] = y.data_ptr()
            self._wp[i] = w.data_ptr()
        rc = B.lib().vptq_quant_gemv_sliced_tokens_grouped(self.descs, self.layouts, len(ys), x.data_ptr(), self._yp, tokens, self._flags, self._wp, wb, sp)
        return _launch_failed(rc, "vptq_quant_gemv_sliced_tokens_grouped", wss) if rc else ys

    def _launch(self, x):
        sp = B.current_stream_ptr(self.dev)
        wss = [m._workspace(sp) for m in self.members]
        if any(w is None for w in wss):
            return None
        ys = [torch.empty(x.shape[:-1] + (m.layer.out_features,), dtype=self._dtype, device=self.dev) for m in self.members]
        for i, (y, w) in enumerate(zip(ys, wss)):
            self._yp[i] = y.data_ptr()
            self._wp[i] = w.data_ptr()
        rc = self._fn(self.descs, self.layouts, len(ys), x.data_ptr(), self._yp, self._flags, self._wp, self._wb, sp)
        return _launch_failed(rc, "vptq_quant_gemv_sliced_grouped", wss) if rc else ys
