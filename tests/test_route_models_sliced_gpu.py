"""The sliced-layout kernels (gemv_sliced, gemv_sliced_tok, gemv_hot) held to the per-output float64 models of
test_route_models_gpu.py at EVERY INSTANTIATION and launch-shape class: a kernel name is a family of separately compiled
instantiations - gemv_sliced_kernel<DT, NSL, RES, V, TWO, EX, RG, TOK, WPT>, gemv_sliced_tok_kernel<DT, NSL, RES, V, TWO, TOK, EX>,
gemv_hot_kernel<DT, V> - that the launch code picks by the layer's format, width and token count.  Each row builds its layer(s)
with vo.make_layer and their layouts through SlicedGemv / SlicedGroupGemv, asserts the instance string
vptq_quant_gemv_sliced_instance / _tokens_instance gives for the real descriptors and layouts, then checks the 16-bit and the
VPTQ_GEMV_OUT_F32 output of every token against the model, with the route table's bounds and nothing added:
    gemv_sliced (one token, one pass of 2 / 3)  extra_abs = am.sliced_extra_abs(dt, arrivals), arrivals read from the instance
    gemv_sliced_tok (column phases)             extra_abs = 0 - fp32 partial sums in a fixed order
    exact rows: the exact model on a dense activation; folded rows: the folded model on a planted one; selective rows: the
    selective model (the hot-set agreement check is on).  fp16 with the 256-entry residual table of v = 8: the folded part adds the
    two entries with ONE packed fp16 add, f16(c + r), as gemv_sliced.hip states - the model's `rounded` form (bf16 keeps c x + r x).
tests/test_instance_census_cpu.py enumerates the instances the dispatch can be asked for and holds ROWS to them;
tools/gen_sliced_rows.py wrote ROWS as a cover of that enumeration and writes it again when the census grows.

Shapes are the smallest that select the form: O = 72 (9 vector-rows of v = 8, 4.5 of v = 16: a ragged last one), 264 (33 rows: not
a multiple of the 16 waves); widths on both sides of every slice-count, window-part, column-part and phase edge."""
import ctypes as C
import functools

import pytest
import torch

import test_route_models_gpu as rm
from test_route_models_gpu import EXACT, F32, SEL, _check, _np, _dense, _planted
from oracle import vptq_oracle as vo
import _arith_model as am
from _gpu_util import spec_to_module, bits_to_tensor

pytestmark = pytest.mark.gpu
dev = rm.dev

PARTS = 1 << 8   # VPTQ_GEMV_COLUMN_PARTS
MODE_FLAGS = {"folded": 0, "exact": EXACT, "sel": SEL}
MODE_ARITH = {"folded": "folded", "exact": "exact", "sel": "selective"}


def sliced_instance_of(descs, layouts, n, tokens, flags):
    """vptq_quant_gemv_sliced_instance (one token) / _tokens_instance (2 - 8) for these descriptors and layout structs"""
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(1024)
    fn = B.lib().vptq_quant_gemv_sliced_instance if tokens == 1 else B.lib().vptq_quant_gemv_sliced_tokens_instance
    B.check(fn(descs, layouts, n, tokens, flags, buf, len(buf)), "sliced instance query")
    return buf.value.decode()


def S(I, Os, dt, tokens, mode, instance, v=8, k=65536, kr=0, perm=0, bias=0, rpw=0, entry="single", rounded=0):
    """one row.  Os: the layer's height, or the heights of a group's members (one launch); mode: folded / exact / sel; rpw: rows
    per wave of the layout structs (0: the objects' rule); entry: single (vptq_quant_gemv_sliced / _tokens), grouped (_grouped /
    _tokens_grouped), parts (the grouped entries with VPTQ_GEMV_COLUMN_PARTS), both (single AND grouped of the one layer: identical
    bits required); rounded: the folded part of the row's model is its r16(c + r) form"""
    Os = (Os,) if isinstance(Os, int) else tuple(Os)
    e = dict(I=I, Os=Os, dt=dt, tokens=tokens, mode=mode, instance=instance, v=v, k=k, kr=kr, perm=perm, bias=bias, rpw=rpw, entry=entry, rounded=bool(rounded))
    return pytest.param(e, id=f"{instance.split()[0]}-{dt}-v{v}-k{k}-r{kr}-{I}x{'+'.join(map(str, Os))}-t{tokens}-{mode}-{entry}-p{perm}b{bias}w{rpw}")


# ---------------------------------------------------------------------------------------------- the rows
ROWS = [
    S(1000, 72, "bf16", 1, "sel",
      "gemv_hot dt=bf16 v=8 | gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=0 perm=0 corr=1"),
    S(1000, 72, "bf16", 1, "sel",
      "gemv_hot dt=bf16 v=8 | gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=1 side=0 perm=1 corr=1", kr=4, perm=1),
    S(1000, 72, "bf16", 1, "sel",
      "gemv_hot dt=bf16 v=16 | gemv_sliced dt=bf16 nsl=16 res=0 v=16 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=0 corr=1", v=16, bias=1),
    S(1000, 72, "bf16", 1, "sel",
      "gemv_hot dt=bf16 v=16 | gemv_sliced dt=bf16 nsl=16 res=0 v=16 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=0 side=0 perm=0 corr=1", v=16, kr=65536),
    S(1000, 72, "f16", 1, "sel",
      "gemv_hot dt=f16 v=8 | gemv_sliced dt=f16 nsl=8 res=1 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=1 perm=1 corr=1", kr=256, perm=1, rounded=1),
    S(1000, 72, "f16", 1, "sel",
      "gemv_hot dt=f16 v=8 | gemv_sliced dt=f16 nsl=8 res=0 v=8 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=1 side=0 perm=0 corr=1", kr=1024, bias=1),
    S(1000, 72, "f16", 1, "sel",
      "gemv_hot dt=f16 v=16 | gemv_sliced dt=f16 nsl=16 res=0 v=16 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=0 corr=1", v=16, bias=1),
    S(1000, 72, "f16", 1, "sel",
      "gemv_hot dt=f16 v=16 | gemv_sliced dt=f16 nsl=16 res=0 v=16 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=1 side=0 perm=0 corr=1", v=16, kr=4),
    S(1000, 72, "bf16", 3, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=0 perm=0 corr=0", k=16384, entry='both'),
    S(1000, 72, "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=8 res=1 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=1 perm=0 corr=0", k=32768, kr=256, entry='both', bias=1),
    S(1000, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=0 perm=0 corr=0", entry='both'),
    S(1000, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=0 perm=0 corr=0", entry='both'),
    S(1000, (264, 72), "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=2 rpw=1 arrivals=8 whole1=0 side=0 perm=0 corr=0", entry='grouped'),
    S(1000, (264, 72), "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=2 rpw=1 arrivals=8 whole1=0 side=0 perm=0 corr=0", entry='grouped'),
    S(1000, (264, 72, 8200), "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=3 rpw=3 arrivals=8 whole1=0 side=0 perm=0 corr=0", entry='grouped'),
    S(1000, (264, 72, 8200), "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=3 rpw=3 arrivals=8 whole1=0 side=0 perm=0 corr=0", entry='grouped'),
    S(1024, 264, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=18 arrivals=8 whole1=0 side=0 perm=0 corr=0", rpw=18, bias=1),
    S(1024, 264, "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=2 arrivals=8 whole1=0 side=0 perm=0 corr=0", rpw=2, bias=1),
    S(1024, 264, "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=18 arrivals=8 whole1=0 side=0 perm=0 corr=0", rpw=18, bias=1),
    S(4096, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=2 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=16 whole1=0 side=0 perm=0 corr=0", entry='both', bias=1),
    S(4096, 72, "bf16", 3, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=3 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=16 whole1=0 side=0 perm=0 corr=0", entry='both', bias=1),
    S(8192, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=0 corr=0", entry='both', bias=1),
    S(8192, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=0 corr=0", entry='both', bias=1),
    S(8192, 72, "bf16", 3, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=0 corr=0", entry='both', bias=1),
    S(14080, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=2 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=32 whole1=0 side=0 perm=0 corr=0", entry='both', bias=1),
    S(14080, 72, "bf16", 3, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=3 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=32 whole1=0 side=0 perm=0 corr=0", entry='both', bias=1),
    S(14344, 72, "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=0 corr=0", entry='both'),
    S(1000, 72, "bf16", 3, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=1 rg=1 tok=3 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=2 perm=1 corr=0", kr=4, perm=1, entry='both'),
    S(8192, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=8 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", kr=4, entry='both'),
    S(8192, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=8 two=0 ex=1 rg=1 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", kr=4, entry='both'),
    S(8192, 72, "bf16", 3, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=8 two=0 ex=1 rg=1 tok=3 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", kr=4, entry='both'),
    S(14344, 72, "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=8 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=1 side=0 perm=0 corr=0", kr=4, entry='both', bias=1),
    S(1000, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=1 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both', bias=1),
    S(1000, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=1 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both', bias=1),
    S(1000, 72, "bf16", 3, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=1 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both', bias=1),
    S(4096, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=1 v=8 two=0 ex=1 rg=0 tok=2 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=16 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both'),
    S(4096, 72, "bf16", 3, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=1 v=8 two=0 ex=1 rg=0 tok=3 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=16 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both'),
    S(4712, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both', bias=1),
    S(4712, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both', bias=1),
    S(4712, 72, "bf16", 3, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both', bias=1),
    S(14080, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=2 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=32 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both'),
    S(14080, 72, "bf16", 3, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=3 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=32 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both'),
    S(14088, 72, "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both', bias=1),
    S(16288, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=2 n=1 rpw=1 arrivals=32 whole1=0 side=1 perm=0 corr=0", kr=256, entry='parts'),
    S(16288, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=2 n=1 rpw=1 arrivals=32 whole1=0 side=1 perm=0 corr=0", kr=256, entry='parts'),
    S(16288, 72, "bf16", 3, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=2 n=1 rpw=1 arrivals=32 whole1=0 side=1 perm=0 corr=0", kr=256, entry='parts'),
    S(16288, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=2 n=1 rpw=1 arrivals=32 whole1=0 side=1 perm=1 corr=0", kr=256, perm=1, entry='parts', bias=1),
    S(16288, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=2 n=1 rpw=1 arrivals=32 whole1=0 side=1 perm=1 corr=0", kr=256, perm=1, entry='parts', bias=1),
    S(16288, 72, "bf16", 3, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=2 n=1 rpw=1 arrivals=32 whole1=0 side=1 perm=1 corr=0", kr=256, perm=1, entry='parts', bias=1),
    S(16296, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=3 n=1 rpw=1 arrivals=48 whole1=0 side=1 perm=0 corr=0", kr=256, entry='parts', bias=1),
    S(16296, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=3 n=1 rpw=1 arrivals=48 whole1=0 side=1 perm=0 corr=0", kr=256, entry='parts', bias=1),
    S(16296, 72, "bf16", 3, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=3 n=1 rpw=1 arrivals=48 whole1=0 side=1 perm=0 corr=0", kr=256, entry='parts', bias=1),
    S(16296, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=3 n=1 rpw=1 arrivals=48 whole1=0 side=1 perm=1 corr=0", kr=256, perm=1, entry='parts'),
    S(16296, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=3 n=1 rpw=1 arrivals=48 whole1=0 side=1 perm=1 corr=0", kr=256, perm=1, entry='parts'),
    S(16296, 72, "bf16", 3, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=3 n=1 rpw=1 arrivals=48 whole1=0 side=1 perm=1 corr=0", kr=256, perm=1, entry='parts'),
    S(1000, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=2 perm=0 corr=0", kr=1024, entry='both', bias=1),
    S(1000, 72, "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=1 side=0 perm=0 corr=0", kr=1024, entry='both', bias=1),
    S(1000, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=1 rg=1 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=2 perm=0 corr=0", kr=4096, entry='both', bias=1),
    S(1000, 72, "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=1 side=0 perm=0 corr=0", kr=4096, entry='both', bias=1),
    S(1000, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=2 perm=0 corr=0", kr=65536, entry='both', bias=1),
    S(1000, 72, "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=8 res=0 v=8 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=0 corr=0", kr=65536, entry='both', bias=1),
    S(1000, 72, "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=16 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=1 side=0 perm=0 corr=0", v=16, k=16384, kr=256, entry='both'),
    S(1000, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=16 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=1 corr=0", v=16, k=32768, perm=1, entry='both'),
    S(1000, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=16 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=0 corr=0", v=16, entry='both', bias=1),
    S(8192, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=32 res=0 v=16 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=0 side=0 perm=0 corr=0", v=16, entry='both'),
    S(8192, 72, "bf16", 2, "exact",
      "gemv_sliced dt=bf16 nsl=32 res=0 v=16 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=0 side=0 perm=0 corr=0", v=16, entry='both'),
    S(14344, 72, "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=32 res=0 v=16 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=0 side=0 perm=0 corr=0", v=16, entry='both', bias=1),
    S(1000, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=16 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", v=16, kr=4, entry='both'),
    S(1000, 72, "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=16 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=1 side=0 perm=0 corr=0", v=16, kr=4, entry='both'),
    S(1000, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=16 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", v=16, kr=256, entry='both'),
    S(8192, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=32 res=0 v=16 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=0 side=2 perm=0 corr=0", v=16, kr=256, entry='both', bias=1),
    S(14344, 72, "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=32 res=0 v=16 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=64 whole1=1 side=0 perm=0 corr=0", v=16, kr=256, entry='both'),
    S(1000, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=16 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", v=16, kr=1024, entry='both'),
    S(1000, 72, "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=16 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=1 side=0 perm=0 corr=0", v=16, kr=1024, entry='both'),
    S(1000, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=16 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", v=16, kr=4096, entry='both'),
    S(1000, 72, "bf16", 1, "folded",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=16 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=1 side=0 perm=0 corr=0", v=16, kr=4096, entry='both'),
    S(1000, 72, "bf16", 1, "exact",
      "gemv_sliced dt=bf16 nsl=16 res=0 v=16 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", v=16, kr=65536, entry='both'),
    S(1000, 72, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=0 perm=0 corr=0", k=16384, entry='both'),
    S(1000, 72, "f16", 3, "exact",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=0 perm=1 corr=0", k=16384, perm=1, entry='both', bias=1),
    S(1000, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=0 perm=0 corr=0", entry='both'),
    S(1000, 72, "f16", 2, "exact",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=0 perm=0 corr=0", entry='both'),
    S(1000, 72, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=0 perm=0 corr=0", entry='both'),
    S(1000, (264, 72), "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=2 rpw=1 arrivals=8 whole1=0 side=0 perm=0 corr=0", entry='grouped'),
    S(1000, (264, 72), "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=2 rpw=1 arrivals=8 whole1=0 side=0 perm=0 corr=0", entry='grouped'),
    S(1000, (264, 72, 8200), "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=3 rpw=3 arrivals=8 whole1=0 side=0 perm=0 corr=0", entry='grouped'),
    S(1000, (264, 72, 8200), "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=3 rpw=3 arrivals=8 whole1=0 side=0 perm=0 corr=0", entry='grouped'),
    S(1024, 264, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=18 arrivals=8 whole1=0 side=0 perm=0 corr=0", rpw=18, bias=1),
    S(1024, 264, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=2 arrivals=8 whole1=0 side=0 perm=0 corr=0", rpw=2, bias=1),
    S(1024, 264, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=18 arrivals=8 whole1=0 side=0 perm=0 corr=0", rpw=18, bias=1),
    S(4096, 72, "f16", 2, "exact",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=2 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=16 whole1=0 side=0 perm=0 corr=0", entry='both', bias=1),
    S(4096, 72, "f16", 3, "exact",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=1 rg=0 tok=3 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=16 whole1=0 side=0 perm=0 corr=0", entry='both', bias=1),
    S(14080, 72, "f16", 2, "exact",
      "gemv_sliced dt=f16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=2 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=32 whole1=0 side=0 perm=0 corr=0", entry='both', bias=1),
    S(14080, 72, "f16", 3, "exact",
      "gemv_sliced dt=f16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=3 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=32 whole1=0 side=0 perm=0 corr=0", entry='both', bias=1),
    S(14344, 72, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=16 res=0 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=0 corr=0", entry='both'),
    S(16392, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=3 n=1 rpw=1 arrivals=48 whole1=0 side=0 perm=0 corr=0", entry='parts'),
    S(16392, 72, "f16", 2, "exact",
      "gemv_sliced dt=f16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=3 n=1 rpw=1 arrivals=48 whole1=0 side=0 perm=0 corr=0", entry='parts'),
    S(16392, 72, "f16", 3, "exact",
      "gemv_sliced dt=f16 nsl=16 res=0 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=3 n=1 rpw=1 arrivals=48 whole1=0 side=0 perm=0 corr=0", entry='parts'),
    S(1000, 72, "f16", 3, "exact",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=1 rg=1 tok=3 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=2 perm=0 corr=0", kr=4, entry='both', bias=1),
    S(1000, 72, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=1 side=0 perm=0 corr=0", kr=4, entry='both', bias=1),
    S(8192, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=16 res=0 v=8 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", kr=4, entry='both'),
    S(8192, 72, "f16", 2, "exact",
      "gemv_sliced dt=f16 nsl=16 res=0 v=8 two=0 ex=1 rg=1 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", kr=4, entry='both'),
    S(8192, 72, "f16", 3, "exact",
      "gemv_sliced dt=f16 nsl=16 res=0 v=8 two=0 ex=1 rg=1 tok=3 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", kr=4, entry='both'),
    S(14344, 72, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=16 res=0 v=8 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=1 side=0 perm=0 corr=0", kr=4, entry='both', bias=1),
    S(1000, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=8 res=1 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both', bias=1),
    S(1000, 72, "f16", 2, "exact",
      "gemv_sliced dt=f16 nsl=8 res=1 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both', bias=1),
    S(1000, 72, "f16", 3, "exact",
      "gemv_sliced dt=f16 nsl=8 res=1 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both', bias=1),
    S(4096, 72, "f16", 2, "exact",
      "gemv_sliced dt=f16 nsl=8 res=1 v=8 two=0 ex=1 rg=0 tok=2 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=16 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both'),
    S(4096, 72, "f16", 3, "exact",
      "gemv_sliced dt=f16 nsl=8 res=1 v=8 two=0 ex=1 rg=0 tok=3 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=16 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both'),
    S(4712, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both', bias=1),
    S(4712, 72, "f16", 2, "exact",
      "gemv_sliced dt=f16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both', bias=1),
    S(4712, 72, "f16", 3, "exact",
      "gemv_sliced dt=f16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both', bias=1),
    S(14080, 72, "f16", 2, "exact",
      "gemv_sliced dt=f16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=2 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=32 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both'),
    S(14080, 72, "f16", 3, "exact",
      "gemv_sliced dt=f16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=3 wpt=1 wparts=2 parts=1 n=1 rpw=2 arrivals=32 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both'),
    S(14088, 72, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=16 res=1 v=8 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=1 perm=0 corr=0", kr=256, entry='both', rounded=1, bias=1),
    S(16288, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=2 n=1 rpw=1 arrivals=32 whole1=0 side=1 perm=0 corr=0", kr=256, entry='parts'),
    S(16288, 72, "f16", 2, "exact",
      "gemv_sliced dt=f16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=2 n=1 rpw=1 arrivals=32 whole1=0 side=1 perm=0 corr=0", kr=256, entry='parts'),
    S(16288, 72, "f16", 3, "exact",
      "gemv_sliced dt=f16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=2 n=1 rpw=1 arrivals=32 whole1=0 side=1 perm=0 corr=0", kr=256, entry='parts'),
    S(16288, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=2 n=1 rpw=1 arrivals=32 whole1=0 side=1 perm=1 corr=0", kr=256, perm=1, entry='parts', bias=1),
    S(16288, 72, "f16", 2, "exact",
      "gemv_sliced dt=f16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=2 n=1 rpw=1 arrivals=32 whole1=0 side=1 perm=1 corr=0", kr=256, perm=1, entry='parts', bias=1),
    S(16288, 72, "f16", 3, "exact",
      "gemv_sliced dt=f16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=2 n=1 rpw=1 arrivals=32 whole1=0 side=1 perm=1 corr=0", kr=256, perm=1, entry='parts', bias=1),
    S(16296, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=3 n=1 rpw=1 arrivals=48 whole1=0 side=1 perm=1 corr=0", kr=256, perm=1, entry='parts'),
    S(16296, 72, "f16", 2, "exact",
      "gemv_sliced dt=f16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=3 n=1 rpw=1 arrivals=48 whole1=0 side=1 perm=1 corr=0", kr=256, perm=1, entry='parts'),
    S(16296, 72, "f16", 3, "exact",
      "gemv_sliced dt=f16 nsl=16 res=1 v=8 two=0 ex=1 rg=0 tok=3 wpt=0 wparts=1 parts=3 n=1 rpw=1 arrivals=48 whole1=0 side=1 perm=1 corr=0", kr=256, perm=1, entry='parts'),
    S(1000, 72, "f16", 2, "exact",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=1 rg=1 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=2 perm=1 corr=0", kr=1024, perm=1, entry='both'),
    S(1000, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=2 perm=0 corr=0", kr=4096, entry='both', bias=1),
    S(1000, 72, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=1 side=0 perm=0 corr=0", kr=4096, entry='both', bias=1),
    S(1000, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=8 whole1=0 side=2 perm=0 corr=0", kr=65536, entry='both', bias=1),
    S(1000, 72, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=8 res=0 v=8 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=0 corr=0", kr=65536, entry='both', bias=1),
    S(1000, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=16 res=0 v=16 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", v=16, k=32768, kr=256, entry='both'),
    S(1000, 72, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=16 res=0 v=16 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=1 side=0 perm=0 corr=0", v=16, k=32768, kr=256, entry='both'),
    S(1000, 72, "f16", 2, "exact",
      "gemv_sliced dt=f16 nsl=16 res=0 v=16 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=0 corr=0", v=16, entry='both', bias=1),
    S(1000, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=16 res=0 v=16 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=0 perm=1 corr=0", v=16, perm=1, entry='both'),
    S(8192, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=32 res=0 v=16 two=0 ex=1 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=0 side=0 perm=0 corr=0", v=16, entry='both'),
    S(8192, 72, "f16", 2, "exact",
      "gemv_sliced dt=f16 nsl=32 res=0 v=16 two=0 ex=1 rg=0 tok=2 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=0 side=0 perm=0 corr=0", v=16, entry='both'),
    S(14344, 72, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=32 res=0 v=16 two=0 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=0 side=0 perm=0 corr=0", v=16, entry='both', bias=1),
    S(1000, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=16 res=0 v=16 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", v=16, kr=4, entry='both'),
    S(8192, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=32 res=0 v=16 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=0 side=2 perm=0 corr=0", v=16, kr=256, entry='both', bias=1),
    S(14344, 72, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=32 res=0 v=16 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=64 whole1=1 side=0 perm=0 corr=0", v=16, kr=256, entry='both'),
    S(1000, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=16 res=0 v=16 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", v=16, kr=1024, entry='both'),
    S(1000, 72, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=16 res=0 v=16 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=1 side=0 perm=0 corr=0", v=16, kr=1024, entry='both'),
    S(1000, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=16 res=0 v=16 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", v=16, kr=4096, entry='both'),
    S(1000, 72, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=16 res=0 v=16 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=1 side=0 perm=0 corr=0", v=16, kr=4096, entry='both'),
    S(1000, 72, "f16", 1, "exact",
      "gemv_sliced dt=f16 nsl=16 res=0 v=16 two=0 ex=1 rg=1 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=16 whole1=0 side=2 perm=0 corr=0", v=16, kr=65536, entry='both'),
    S(1000, 72, "f16", 1, "folded",
      "gemv_sliced dt=f16 nsl=16 res=0 v=16 two=1 ex=0 rg=0 tok=1 wpt=0 wparts=1 parts=1 n=1 rpw=1 arrivals=32 whole1=0 side=0 perm=0 corr=0", v=16, kr=65536, entry='both'),
    S(1000, 72, "bf16", 2, "folded",
      "gemv_sliced_tok dt=bf16 nsl=8 res=1 v=8 two=0 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=0 perm=0", k=16384, kr=256, entry='both', bias=1),
    S(1000, 72, "bf16", 2, "folded",
      "gemv_sliced_tok dt=bf16 nsl=8 res=0 v=8 two=0 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=0 perm=1", k=32768, perm=1, entry='both', bias=1),
    S(1000, 72, "bf16", 4, "exact",
      "gemv_sliced_tok dt=bf16 nsl=8 res=1 v=8 two=0 tok=4 ex=1 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=1", k=32768, kr=256, perm=1, entry='both'),
    S(1000, 72, "bf16", 4, "exact",
      "gemv_sliced_tok dt=bf16 nsl=8 res=0 v=8 two=0 tok=4 ex=1 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both'),
    S(1000, 72, "bf16", 5, "exact",
      "gemv_sliced_tok dt=bf16 nsl=8 res=0 v=8 two=0 tok=8 ex=1 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both'),
    S(1000, 72, "bf16", 3, "folded",
      "gemv_sliced_tok dt=bf16 nsl=8 res=0 v=8 two=0 tok=4 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both'),
    S(1000, 72, "bf16", 5, "folded",
      "gemv_sliced_tok dt=bf16 nsl=8 res=0 v=8 two=0 tok=8 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both'),
    S(1000, (264, 72), "bf16", 2, "folded",
      "gemv_sliced_tok dt=bf16 nsl=8 res=0 v=8 two=0 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=2 whole1=0 perm=0", entry='grouped'),
    S(1000, (264, 72, 8200), "bf16", 2, "folded",
      "gemv_sliced_tok dt=bf16 nsl=8 res=0 v=8 two=0 tok=2 ex=0 phases=1 rpw=3 regsums=0 n=3 whole1=0 perm=0", entry='grouped'),
    S(8192, 72, "bf16", 4, "exact",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=8 two=0 tok=4 ex=1 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both', bias=1),
    S(8192, 72, "bf16", 5, "exact",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=8 two=0 tok=8 ex=1 phases=4 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both', bias=1),
    S(14344, 72, "bf16", 2, "folded",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=8 two=0 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=0 perm=0", entry='both'),
    S(14344, 72, "bf16", 3, "folded",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=8 two=0 tok=4 ex=0 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both'),
    S(14344, 72, "bf16", 5, "folded",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=8 two=0 tok=8 ex=0 phases=4 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both'),
    S(1000, 72, "bf16", 3, "folded",
      "gemv_sliced_tok dt=bf16 nsl=8 res=0 v=8 two=1 tok=4 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=1 perm=0", kr=4, entry='both', bias=1),
    S(1000, 72, "bf16", 5, "folded",
      "gemv_sliced_tok dt=bf16 nsl=8 res=0 v=8 two=1 tok=8 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=1 perm=0", kr=4, entry='both', bias=1),
    S(1000, 8200, "bf16", 3, "folded",
      "gemv_sliced_tok dt=bf16 nsl=8 res=0 v=8 two=1 tok=4 ex=0 phases=1 rpw=5 regsums=0 n=1 whole1=1 perm=0", kr=4, entry='both', bias=1),
    S(1000, 8200, "bf16", 5, "folded",
      "gemv_sliced_tok dt=bf16 nsl=8 res=0 v=8 two=1 tok=8 ex=0 phases=2 rpw=5 regsums=0 n=1 whole1=1 perm=0", kr=4, entry='both', bias=1),
    S(14344, 72, "bf16", 2, "folded",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=8 two=1 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=1 perm=0", kr=4, entry='both', bias=1),
    S(14344, 72, "bf16", 3, "folded",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=8 two=1 tok=4 ex=0 phases=2 rpw=1 regsums=1 n=1 whole1=1 perm=0", kr=4, entry='both', bias=1),
    S(14344, 72, "bf16", 5, "folded",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=8 two=1 tok=8 ex=0 phases=4 rpw=1 regsums=1 n=1 whole1=1 perm=0", kr=4, entry='both', bias=1),
    S(1000, 72, "bf16", 5, "exact",
      "gemv_sliced_tok dt=bf16 nsl=8 res=1 v=8 two=0 tok=8 ex=1 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", kr=256, entry='both', bias=1),
    S(1000, 72, "bf16", 3, "folded",
      "gemv_sliced_tok dt=bf16 nsl=8 res=1 v=8 two=0 tok=4 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", kr=256, entry='both', bias=1),
    S(1000, 72, "bf16", 5, "folded",
      "gemv_sliced_tok dt=bf16 nsl=8 res=1 v=8 two=0 tok=8 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", kr=256, entry='both', bias=1),
    S(4712, 72, "bf16", 4, "exact",
      "gemv_sliced_tok dt=bf16 nsl=16 res=1 v=8 two=0 tok=4 ex=1 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", kr=256, entry='both', bias=1),
    S(4712, 72, "bf16", 5, "exact",
      "gemv_sliced_tok dt=bf16 nsl=16 res=1 v=8 two=0 tok=8 ex=1 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0", kr=256, entry='both', bias=1),
    S(14088, 72, "bf16", 2, "folded",
      "gemv_sliced_tok dt=bf16 nsl=16 res=1 v=8 two=0 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=0 perm=0", kr=256, entry='both', bias=1),
    S(14088, 72, "bf16", 3, "folded",
      "gemv_sliced_tok dt=bf16 nsl=16 res=1 v=8 two=0 tok=4 ex=0 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0", kr=256, entry='both', bias=1),
    S(14088, 72, "bf16", 5, "folded",
      "gemv_sliced_tok dt=bf16 nsl=16 res=1 v=8 two=0 tok=8 ex=0 phases=4 rpw=1 regsums=1 n=1 whole1=0 perm=0", kr=256, entry='both', bias=1),
    S(1000, 72, "bf16", 2, "folded",
      "gemv_sliced_tok dt=bf16 nsl=8 res=0 v=8 two=1 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=1 perm=0", kr=1024, entry='both', bias=1),
    S(1000, 72, "bf16", 3, "exact",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=16 two=0 tok=4 ex=1 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, k=16384, entry='both', bias=1),
    S(1000, 72, "bf16", 5, "exact",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=16 two=0 tok=8 ex=1 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both', bias=1),
    S(1000, 72, "bf16", 2, "folded",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=16 two=0 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=0 perm=0", v=16, entry='both', bias=1),
    S(1000, 72, "bf16", 3, "folded",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=16 two=0 tok=4 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both', bias=1),
    S(1000, 72, "bf16", 5, "folded",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=16 two=0 tok=8 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both', bias=1),
    S(1000, (264, 72), "bf16", 3, "exact",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=16 two=0 tok=4 ex=1 phases=1 rpw=1 regsums=1 n=2 whole1=0 perm=0", v=16, entry='grouped', bias=1),
    S(1000, (264, 72, 8200), "bf16", 3, "exact",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=16 two=0 tok=4 ex=1 phases=1 rpw=3 regsums=1 n=3 whole1=0 perm=0", v=16, entry='grouped', bias=1),
    S(8192, 72, "bf16", 3, "exact",
      "gemv_sliced_tok dt=bf16 nsl=32 res=0 v=16 two=0 tok=4 ex=1 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both'),
    S(8192, 72, "bf16", 5, "exact",
      "gemv_sliced_tok dt=bf16 nsl=32 res=0 v=16 two=0 tok=8 ex=1 phases=4 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both'),
    S(14344, 72, "bf16", 2, "folded",
      "gemv_sliced_tok dt=bf16 nsl=32 res=0 v=16 two=0 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=0 perm=0", v=16, entry='both', bias=1),
    S(14344, 72, "bf16", 3, "folded",
      "gemv_sliced_tok dt=bf16 nsl=32 res=0 v=16 two=0 tok=4 ex=0 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both', bias=1),
    S(14344, 72, "bf16", 5, "folded",
      "gemv_sliced_tok dt=bf16 nsl=32 res=0 v=16 two=0 tok=8 ex=0 phases=4 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both', bias=1),
    S(1000, 72, "bf16", 5, "folded",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=16 two=1 tok=8 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=1 perm=0", v=16, kr=256, entry='both'),
    S(14344, 72, "bf16", 3, "folded",
      "gemv_sliced_tok dt=bf16 nsl=32 res=0 v=16 two=1 tok=4 ex=0 phases=2 rpw=1 regsums=1 n=1 whole1=1 perm=0", v=16, kr=256, entry='both'),
    S(14344, 72, "bf16", 5, "folded",
      "gemv_sliced_tok dt=bf16 nsl=32 res=0 v=16 two=1 tok=8 ex=0 phases=4 rpw=1 regsums=1 n=1 whole1=1 perm=0", v=16, kr=256, entry='both'),
    S(1000, 72, "bf16", 2, "folded",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=16 two=1 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=1 perm=0", v=16, kr=4096, entry='both'),
    S(15616, 72, "bf16", 2, "folded",
      "gemv_sliced_tok dt=bf16 nsl=32 res=0 v=16 two=1 tok=2 ex=0 phases=4 rpw=1 regsums=0 n=1 whole1=1 perm=0", v=16, kr=4096, entry='both', bias=1),
    S(1000, 72, "bf16", 3, "folded",
      "gemv_sliced_tok dt=bf16 nsl=16 res=0 v=16 two=1 tok=4 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, kr=65536, entry='both'),
    S(1000, 72, "f16", 7, "exact",
      "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=0 tok=8 ex=1 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", k=16384, entry='both'),
    S(1000, 72, "f16", 2, "folded",
      "gemv_sliced_tok dt=f16 nsl=8 res=1 v=8 two=0 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=0 perm=0", k=32768, kr=256, entry='both', bias=1),
    S(1000, 72, "f16", 4, "exact",
      "gemv_sliced_tok dt=f16 nsl=8 res=1 v=8 two=0 tok=4 ex=1 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=1", k=32768, kr=256, perm=1, entry='both'),
    S(14088, 72, "f16", 5, "folded",
      "gemv_sliced_tok dt=f16 nsl=16 res=1 v=8 two=0 tok=8 ex=0 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0", k=32768, kr=256, entry='both', bias=1),
    S(1000, 72, "f16", 4, "exact",
      "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=0 tok=4 ex=1 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both'),
    S(1000, 72, "f16", 2, "folded",
      "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=0 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=0 perm=0", entry='both'),
    S(1000, 72, "f16", 3, "folded",
      "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=0 tok=4 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both'),
    S(1000, 72, "f16", 8, "folded",
      "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=0 tok=8 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both'),
    S(1000, (264, 72), "f16", 2, "folded",
      "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=0 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=2 whole1=0 perm=0", entry='grouped'),
    S(1000, (264, 72, 8200), "f16", 2, "folded",
      "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=0 tok=2 ex=0 phases=1 rpw=3 regsums=0 n=3 whole1=0 perm=0", entry='grouped'),
    S(4096, 72, "f16", 5, "exact",
      "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=0 tok=8 ex=1 phases=4 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both', bias=1),
    S(4096, 72, "f16", 3, "folded",
      "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=0 tok=4 ex=0 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both', bias=1),
    S(4096, 72, "f16", 5, "folded",
      "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=0 tok=8 ex=0 phases=4 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both', bias=1),
    S(8192, 72, "f16", 4, "exact",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=8 two=0 tok=4 ex=1 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both', bias=1),
    S(8192, 72, "f16", 5, "exact",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=8 two=0 tok=8 ex=1 phases=4 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both', bias=1),
    S(14344, 72, "f16", 2, "folded",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=8 two=0 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=0 perm=0", entry='both'),
    S(14344, 72, "f16", 3, "folded",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=8 two=0 tok=4 ex=0 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both'),
    S(14344, 72, "f16", 5, "folded",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=8 two=0 tok=8 ex=0 phases=4 rpw=1 regsums=1 n=1 whole1=0 perm=0", entry='both'),
    S(1000, 72, "f16", 2, "folded",
      "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=1 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=1 perm=0", kr=4, entry='both', bias=1),
    S(1000, 8200, "f16", 3, "folded",
      "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=1 tok=4 ex=0 phases=1 rpw=5 regsums=0 n=1 whole1=1 perm=0", kr=4, entry='both', bias=1),
    S(1000, 8200, "f16", 5, "folded",
      "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=1 tok=8 ex=0 phases=2 rpw=5 regsums=0 n=1 whole1=1 perm=0", kr=4, entry='both', bias=1),
    S(14344, 72, "f16", 2, "folded",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=8 two=1 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=1 perm=0", kr=4, entry='both', bias=1),
    S(14344, 72, "f16", 3, "folded",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=8 two=1 tok=4 ex=0 phases=2 rpw=1 regsums=1 n=1 whole1=1 perm=0", kr=4, entry='both', bias=1),
    S(14344, 72, "f16", 5, "folded",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=8 two=1 tok=8 ex=0 phases=4 rpw=1 regsums=1 n=1 whole1=1 perm=0", kr=4, entry='both', bias=1),
    S(1000, 72, "f16", 5, "exact",
      "gemv_sliced_tok dt=f16 nsl=8 res=1 v=8 two=0 tok=8 ex=1 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", kr=256, entry='both', bias=1),
    S(1000, 72, "f16", 3, "folded",
      "gemv_sliced_tok dt=f16 nsl=8 res=1 v=8 two=0 tok=4 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", kr=256, entry='both', bias=1),
    S(1000, 72, "f16", 5, "folded",
      "gemv_sliced_tok dt=f16 nsl=8 res=1 v=8 two=0 tok=8 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", kr=256, entry='both', bias=1),
    S(4712, 72, "f16", 4, "exact",
      "gemv_sliced_tok dt=f16 nsl=16 res=1 v=8 two=0 tok=4 ex=1 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", kr=256, entry='both', bias=1),
    S(4712, 72, "f16", 5, "exact",
      "gemv_sliced_tok dt=f16 nsl=16 res=1 v=8 two=0 tok=8 ex=1 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0", kr=256, entry='both', bias=1),
    S(14088, 72, "f16", 2, "folded",
      "gemv_sliced_tok dt=f16 nsl=16 res=1 v=8 two=0 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=0 perm=0", kr=256, entry='both', bias=1),
    S(14088, 72, "f16", 3, "folded",
      "gemv_sliced_tok dt=f16 nsl=16 res=1 v=8 two=0 tok=4 ex=0 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0", kr=256, entry='both', bias=1),
    S(1000, 72, "f16", 3, "folded",
      "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=1 tok=4 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=1 perm=0", kr=4096, entry='both', bias=1),
    S(1000, 72, "f16", 6, "folded",
      "gemv_sliced_tok dt=f16 nsl=8 res=0 v=8 two=1 tok=8 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=1", kr=65536, perm=1, entry='both'),
    S(1000, 72, "f16", 2, "folded",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=16 two=0 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=0 perm=0", v=16, k=16384, entry='both', bias=1),
    S(1000, 72, "f16", 3, "exact",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=16 two=0 tok=4 ex=1 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both', bias=1),
    S(1000, 72, "f16", 5, "exact",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=16 two=0 tok=8 ex=1 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both', bias=1),
    S(1000, 72, "f16", 3, "folded",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=16 two=0 tok=4 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both', bias=1),
    S(1000, 72, "f16", 5, "folded",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=16 two=0 tok=8 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both', bias=1),
    S(1000, (264, 72), "f16", 3, "exact",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=16 two=0 tok=4 ex=1 phases=1 rpw=1 regsums=1 n=2 whole1=0 perm=0", v=16, entry='grouped', bias=1),
    S(1000, (264, 72, 8200), "f16", 3, "exact",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=16 two=0 tok=4 ex=1 phases=1 rpw=3 regsums=1 n=3 whole1=0 perm=0", v=16, entry='grouped', bias=1),
    S(4096, 72, "f16", 2, "exact",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=16 two=0 tok=4 ex=1 phases=4 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both'),
    S(8192, 72, "f16", 3, "exact",
      "gemv_sliced_tok dt=f16 nsl=32 res=0 v=16 two=0 tok=4 ex=1 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both'),
    S(8192, 72, "f16", 5, "exact",
      "gemv_sliced_tok dt=f16 nsl=32 res=0 v=16 two=0 tok=8 ex=1 phases=4 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both'),
    S(14344, 72, "f16", 2, "folded",
      "gemv_sliced_tok dt=f16 nsl=32 res=0 v=16 two=0 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=0 perm=0", v=16, entry='both', bias=1),
    S(14344, 72, "f16", 3, "folded",
      "gemv_sliced_tok dt=f16 nsl=32 res=0 v=16 two=0 tok=4 ex=0 phases=2 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both', bias=1),
    S(14344, 72, "f16", 5, "folded",
      "gemv_sliced_tok dt=f16 nsl=32 res=0 v=16 two=0 tok=8 ex=0 phases=4 rpw=1 regsums=1 n=1 whole1=0 perm=0", v=16, entry='both', bias=1),
    S(1000, 72, "f16", 3, "folded",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=16 two=1 tok=4 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=1 perm=0", v=16, kr=256, entry='both'),
    S(1000, 72, "f16", 5, "folded",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=16 two=1 tok=8 ex=0 phases=1 rpw=1 regsums=1 n=1 whole1=1 perm=0", v=16, kr=256, entry='both'),
    S(14344, 72, "f16", 5, "folded",
      "gemv_sliced_tok dt=f16 nsl=32 res=0 v=16 two=1 tok=8 ex=0 phases=4 rpw=1 regsums=1 n=1 whole1=1 perm=0", v=16, kr=256, entry='both'),
    S(1000, 72, "f16", 2, "folded",
      "gemv_sliced_tok dt=f16 nsl=16 res=0 v=16 two=1 tok=2 ex=0 phases=1 rpw=1 regsums=0 n=1 whole1=1 perm=0", v=16, kr=1024, entry='both'),
    S(14344, 72, "f16", 2, "folded",
      "gemv_sliced_tok dt=f16 nsl=32 res=0 v=16 two=1 tok=2 ex=0 phases=2 rpw=1 regsums=0 n=1 whole1=1 perm=0", v=16, kr=4096, entry='both'),
    S(14344, 72, "f16", 3, "folded",
      "gemv_sliced_tok dt=f16 nsl=32 res=0 v=16 two=1 tok=4 ex=0 phases=4 rpw=1 regsums=1 n=1 whole1=1 perm=0", v=16, kr=4096, entry='both'),
]


@functools.lru_cache(maxsize=6)
def _layer(I, O, dt, v, k, kr, perm, bias):
    L = vo.make_layer(I, O, dist="llm", seed=I + O + v + kr % 97, dtype=dt, vector_len=v, num_centroids=k, num_res_centroids=kr,
                      enable_perm=bool(perm), bias=bool(bias))
    return L, am.pieces(L)


@functools.lru_cache(maxsize=6)
def _object(I, O, dt, v, k, kr, perm, bias, mode, rpw, device):
    from vptq_amd.utils.sliced import SlicedGemv
    L, _ = _layer(I, O, dt, v, k, kr, perm, bias)
    m = spec_to_module(L, device)
    return m, SlicedGemv(m, rows_per_wave=rpw, exact=mode == "exact", selective=mode == "sel")


def _group_call(g, x, tokens, flags):
    """vptq_quant_gemv_sliced_grouped / _tokens_grouped over the group's members with `flags` added -> outputs"""
    from vptq_amd import _backend as B
    sp = B.current_stream_ptr(g.dev)
    n = len(g.members)
    wss = [m._workspace(sp) if tokens == 1 else m._tokens_workspace(sp, tokens) for m in g.members]
    ys = [torch.empty(1, tokens, m.layer.out_features, dtype=torch.float32 if flags & F32 else x.dtype, device=g.dev) for m in g.members]
    yp = (C.c_void_p * n)(*[y.data_ptr() for y in ys])
    wp = (C.c_void_p * n)(*[w.data_ptr() for w in wss])
    wb = (C.c_size_t * n)(*[(m._ws_bytes if tokens == 1 else w.numel()) for m, w in zip(g.members, wss)])
    if tokens == 1:
        rc = B.lib().vptq_quant_gemv_sliced_grouped(g.descs, g.layouts, n, x.data_ptr(), yp, g._flags | flags, wp, wb, sp)
    else:
        rc = B.lib().vptq_quant_gemv_sliced_tokens_grouped(g.descs, g.layouts, n, x.data_ptr(), yp, tokens, g._flags | flags, wp, wb, sp)
    torch.cuda.synchronize()
    B.check(rc, "grouped sliced call")
    return ys


def _single_call(sl, x, tokens, flags):
    """vptq_quant_gemv_sliced / _tokens (a layer in column parts: the grouped entries with VPTQ_GEMV_COLUMN_PARTS)"""
    y = sl(x, flags=flags) if tokens == 1 else sl.forward_tokens(x, flags=flags)
    assert y is not None, "the sliced entry turned the call down"
    torch.cuda.synchronize()
    return [y]


@pytest.mark.parametrize("e", ROWS)
def test_sliced_instance_vs_its_model(e, dev):
    from vptq_amd.utils.sliced import SlicedGroupGemv
    I, dt, tokens, mode = e["I"], e["dt"], e["tokens"], e["mode"]
    key = lambda O: (I, O, dt, e["v"], e["k"], e["kr"], e["perm"], e["bias"])   # noqa: E731
    Ls = [_layer(*key(O)) for O in e["Os"]]
    sls = [_object(*key(O), mode, e["rpw"], dev)[1] for O in e["Os"]]
    sl = sls[0]
    grouped = len(sls) > 1 or e["entry"] in ("grouped", "both")
    assert (sl.parts > 1) == (e["entry"] == "parts")
    g = SlicedGroupGemv(sls) if grouped else None
    flags = MODE_FLAGS[mode]
    # the instantiation the library says this call launches
    if sl.parts > 1:
        got = sliced_instance_of(sl._part_descs, sl._lay_ref, sl.parts, tokens, flags | PARTS)
    elif len(sls) > 1 or e["entry"] == "grouped":
        got = sliced_instance_of(g.descs, g.layouts, len(sls), tokens, flags)
    else:
        from vptq_amd import _backend as B
        got = sliced_instance_of((B.LayerDesc * 1)(sl.desc), sl._lay_ref, 1, tokens, flags)
    assert got == e["instance"]
    if e["entry"] == "both":   # the group of this one layer launches the same
        assert sliced_instance_of(g.descs, g.layouts, 1, tokens, flags) == e["instance"]
    name, f = got.split(" | ")[-1].split()[0], dict(p.split("=") for p in got.split(" | ")[-1].split()[1:])
    extra = am.sliced_extra_abs(dt, int(f["arrivals"])) if name == "gemv_sliced" else 0.0
    x, hot = (_dense(I, tokens, dt, I + tokens) if mode == "exact" else _planted(I, tokens, dt, I + tokens, perm=Ls[0][0].perm))
    xt = bits_to_tensor(x, dt, dev).reshape(1, tokens, I)
    run = (lambda fl: _group_call(g, xt, tokens, fl)) if (len(sls) > 1 or e["entry"] == "grouped") else (lambda fl: _single_call(sl, xt, tokens, fl))
    y16, y32 = run(0), run(F32)
    for i, (L, P) in enumerate(Ls):
        _check(_np(y16[i]), _np(y32[i]), L, x, dict(arith=MODE_ARITH[mode], rounded=e["rounded"]), hot, extra, P, what=f"{name} member {i}")
    if e["entry"] == "both":
        twin = _group_call(g, xt, tokens, 0)[0]
        assert torch.equal(twin.view(torch.int16).reshape(-1), y16[0].view(torch.int16).reshape(-1)), "single and grouped entry: not the same bits"
