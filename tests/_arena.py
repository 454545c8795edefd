"""Operand placement for the kernel tests: every operand of a launch inside a byte arena of its own, at a chosen alignment, between
margins of a chosen fill - plain torch, CPU tensors included (tests/test_arena_cpu.py tests this file without a device).

Why: a tensor from torch's caching allocator is 256-byte aligned (at least), its size is rounded up to 512 bytes and what follows it is
whatever finite data the pool holds.  A store a few elements past y lands in padding, a load past the last column of x reads a finite
number that a masked weight multiplies away - and the same load next to a NaN bit pattern makes the output row NaN.  Here the SAME
call runs under a benign placement (zero bytes around every operand, 256-byte aligned) and a hostile one (quiet NaN around every
floating-point operand, 0xFF bytes around every integer one, every operand at the least alignment its entry accepts) and must give
the same bits; the margins of the inputs, of y and of the workspace must come back untouched.

    view, h = place(t, HOSTILE, offset=16)        # t's shape, dtype and contents; data_ptr() % 256 == 16
    ...launch...
    assert h.intact()                             # both margins byte for byte what they were filled with

MARGIN is a safety condition, not a measurement: every over-read or over-write these tests can detect stays INSIDE the operand's own
allocation, so nothing here can fault.  It is at least 64 KiB per side and at least four times the largest single staging extent a
kernel file names: gemv_k256m and layout_build stage 8192 columns x 2 bytes = 16 KiB at a time, gemv_lds_mfma kLMStageIt = 4 passes of
8192 columns and the sliced kernels (sliced.h: kSLMaxG16) the activations of a whole layer of up to 32768 columns = 64 KiB - so
4 x 64 KiB = 256 KiB.

Out of reach: the tensors the library's Python side derives and owns cannot be re-seated - `scale_permuted` and `bias_permuted`
(vptq_amd/_backend.py:permuted_norm, built by make_layer_desc for a layer with a permutation) and the inverse permutation `inv_perm`
(_backend.py:inverse_perm, need_inv_perm=True: vptq_dequant).  They come from torch's allocator whatever the placement.  Everything
else a descriptor or a layout struct points to is placed: indices, centroids, res_centroids, outlier_indices, outlier_centroids,
perm, weight_scale, weight_bias, bias; elems, blocks, first, res, wstart; x, y and the workspace."""
import torch

MARGIN = 256 << 10
assert MARGIN >= 64 << 10 and MARGIN >= 4 * 32768 * 2
BASE_ALIGN = 256

BENIGN, HOSTILE = "benign", "hostile"
SENTINEL = 12345.0     # the finite value around a guarded y (exact in fp16, bf16 and fp32)
QNAN = {torch.float16: 0x7E00, torch.bfloat16: 0x7FC0, torch.float32: 0x7FC00000}
_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def fill_pattern(fill, dtype):
    """-> (integer dtype of the operand's element size, the element's bit pattern as a signed value of that dtype) of a fill:
    BENIGN zero bytes; HOSTILE a quiet NaN of a floating-point operand's dtype, 0xFF bytes for an integer operand; a float: that
    value in the operand's dtype (guarded outputs)"""
    it = _INT_OF_SIZE[torch.empty(0, dtype=dtype).element_size()]
    if fill == BENIGN:
        return it, 0
    if fill == HOSTILE:
        if dtype in QNAN:
            return it, QNAN[dtype]
        return it, (255 if it == torch.uint8 else -1)
    if isinstance(fill, float):
        assert dtype.is_floating_point
        return it, int(torch.tensor([fill], dtype=dtype).view(it).item())
    raise ValueError(fill)


class Arena:
    """what place() returns beside the view: the buffer (kept alive), the two margins and what they were filled with"""

    def __init__(self, buf, pre, post, itype, value, view):
        self.buf, self.pre, self.post, self.itype, self.value, self.view = buf, pre, post, itype, value, view

    def intact(self):
        """both margins, byte for byte, still hold the fill"""
        return bool((self.pre.view(self.itype) == self.value).all()) and bool((self.post.view(self.itype) == self.value).all())

    def damage(self):
        """-> [(side, byte distance from the view, bytes changed)] for a failure message"""
        out = []
        es = self.pre.view(self.itype).element_size()
        for side, m in (("before", self.pre), ("after", self.post)):
            bad = torch.nonzero(m.view(self.itype) != self.value).reshape(-1)
            if bad.numel():
                first = int(bad[-1].item() if side == "before" else bad[0].item())
                dist = (m.numel() // es - first) * es if side == "before" else first * es
                out.append((side, dist, int(bad.numel()) * es))
        return out


def place(t, fill, offset=0, margin=MARGIN):
    """-> (view, Arena): a view with t's shape, dtype and contents that starts margin + offset bytes after a 256-byte aligned base
    inside a byte buffer of its own, so `offset` alone decides the pointer's alignment class (data_ptr() % 256 == offset % 256).
    The bytes in front of the view (margin + offset of them) and `margin` bytes behind it hold `fill`, written element by element
    in t's element size and in phase with the view."""
    t = t.detach()
    es = t.element_size()
    assert offset >= 0 and offset % es == 0, "the offset must keep the element alignment"
    assert margin % 8 == 0
    nbytes = t.numel() * es
    pre_n = margin + offset
    buf = torch.empty(BASE_ALIGN + pre_n + nbytes + margin, dtype=torch.uint8, device=t.device)
    s = (-buf.data_ptr()) % BASE_ALIGN
    itype, value = fill_pattern(fill, t.dtype)
    pre = buf[s:s + pre_n]
    body = buf[s + pre_n:s + pre_n + nbytes]
    post = buf[s + pre_n + nbytes:s + pre_n + nbytes + margin]
    pre.view(itype).fill_(value)
    post.view(itype).fill_(value)
    view = body.view(t.dtype).reshape(t.shape)
    view.copy_(t.contiguous())
    assert view.data_ptr() % BASE_ALIGN == offset % BASE_ALIGN and view.is_contiguous()
    return view, Arena(buf, pre, post, itype, value, view)


MODULE_OPERANDS = ("indices", "centroids", "res_centroids", "outlier_indices", "outlier_centroids", "perm", "weight_scale",
                   "weight_bias", "bias")


def _module_params(m):
    """-> {operand name: the parameter object} of a VQuantLinear, only the ones the layer has"""
    out = {"indices": m.indices, "centroids": m.centroids.weight}
    if getattr(m, "enable_residual", False):
        out["res_centroids"] = m.res_centroids.weight
    if getattr(m, "enable_outlier", False):
        out["outlier_indices"] = m.outlier_indices
        out["outlier_centroids"] = m.outlier_centroids.weight
    if getattr(m, "enable_perm", False):
        out["perm"] = m.perm
    if m.weight_scale is not None and m.weight_bias is not None:
        out["weight_scale"], out["weight_bias"] = m.weight_scale, m.weight_bias
    if m.bias is not None:
        out["bias"] = m.bias
    return out


def place_module(m, fill, offsets=None):
    """re-seat every parameter of a VQuantLinear built by _gpu_util.spec_to_module (param.data = view): indices, centroids.weight,
    res_centroids.weight, outlier_indices, outlier_centroids.weight, perm, weight_scale, weight_bias, bias.  _gpu_util.module_desc(m)
    then hands those pointers to the ABI unchanged.  offsets: {operand name: byte offset} (absent: 0).  -> {operand name: Arena}"""
    offsets = offsets or {}
    assert set(offsets) <= set(MODULE_OPERANDS), sorted(set(offsets) - set(MODULE_OPERANDS))
    arenas = {}
    for name, p in _module_params(m).items():
        view, arenas[name] = place(p.data, fill, offsets.get(name, 0))
        p.data = view
    return arenas


LAYOUT_OPERANDS = ("elems", "blocks", "first", "res", "wstart")


def place_layouts(sl, fill, offsets=None):
    """re-seat the layout tensors of a SlicedGemv - (elems, blocks, first, res, wstart) of every table and column part - and rebuild
    its B.SlicedLayout array over the views, as vptq_amd/utils/sliced.py:_layout_structs does (same rows per wave, slices and
    whole-table flags).  offsets: {tensor name: byte offset}, the same for every struct.  -> [Arena]"""
    from vptq_amd.utils.sliced import _layout_structs
    offsets = offsets or {}
    assert set(offsets) <= set(LAYOUT_OPERANDS)
    arenas, tensors = [], []
    for tup in sl._tensors:
        new = []
        for name, t in zip(LAYOUT_OPERANDS, tup):
            if t is None:
                new.append(None)
                continue
            view, a = place(t, fill, offsets.get(name, 0))
            new.append(view)
            arenas.append(a)
        tensors.append(tuple(new))
    rpw = int(sl.layout[0].rows_per_wave)
    sl._tensors = tensors
    sl.elems, sl.blocks, sl.first, sl.res, sl.wstart = tensors[0]
    sl.layout = _layout_structs(tensors, sl._whole, rpw, sl.slices)
    sl._lay_ref = sl.layout
    return arenas


def guarded_out(shape, dtype, device, offset=0, margin=MARGIN):
    """-> (y, Arena): y filled with NaN - an output the launch does not write stays NaN - inside an arena filled with the finite
    SENTINEL (the idea of tests/test_gemm_gather_gpu.py's guard rows): a store outside y breaks intact()"""
    y, a = place(torch.full(tuple(shape), float("nan"), dtype=dtype, device=device), SENTINEL, offset, margin)
    return y, a


def guarded_workspace(nbytes, zeroed, device, align=16, margin=MARGIN):
    """-> (uint8 view of EXACTLY nbytes - what the entry's *_workspace_bytes* query returned -, Arena): zero where the header says
    zero-initialised / zero-filled, else 0xFF bytes ("contents don't matter"); the margins hold 0xA5 bytes, which are neither; the
    pointer is aligned to `align` bytes (16 or 256, as the header asks) and, below 256, not to twice that"""
    assert align in (4, 8, 16, 32, 64, 128, 256)
    body = torch.zeros(nbytes, dtype=torch.uint8, device=device) if zeroed else torch.full((nbytes,), 255, dtype=torch.uint8, device=device)
    es = body.element_size()
    pre_n = margin + (0 if align == BASE_ALIGN else align)
    buf = torch.empty(BASE_ALIGN + pre_n + nbytes + margin, dtype=torch.uint8, device=device)
    s = (-buf.data_ptr()) % BASE_ALIGN
    pre, view, post = buf[s:s + pre_n], buf[s + pre_n:s + pre_n + nbytes], buf[s + pre_n + nbytes:s + pre_n + nbytes + margin]
    pre.fill_(0xA5)
    post.fill_(0xA5)
    view.copy_(body)
    assert es == 1 and view.data_ptr() % align == 0 and (align == BASE_ALIGN or view.data_ptr() % (2 * align) != 0)
    return view, Arena(buf, pre, post, torch.uint8, 0xA5, view)
