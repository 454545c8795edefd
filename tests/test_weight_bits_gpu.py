"""Every GEMV route of the reference's roundings (VPTQ_GEMV_EXACT, the default arithmetic) held to vptq_dequant's WEIGHT BITS, and
to the float64 model on activations and weights at the edges of the number formats.

The promise (include/vptq_hip.h, VPTQ_GEMV_EXACT): every weight is rebuilt as r16(r16(r16(c + r) s) + b), vptq_dequant's W bit for
bit, and accumulated in fp32.  The route tables hold sums of thousands of terms to ulp(m) + 2^-20 sum |terms|, which one wrong
last bit of one weight never reaches.  Here the kernels are asked for single weights:

  1. one-hot activation rows (x = e_j, value 1.0) read columns of W through the kernel: y must be vptq_dequant's bits of the same
     module (-0 == +0).  A one-token route takes one launch per column into its own row of one output buffer, a route of T tokens
     reads T columns per launch, a grouped / chain launch reads one column per copy of the descriptor (up to 32); one sync at the end.
     Two layers per row: the FINITE SPECIAL-VALUE TABLE of tests/_dequant_specials.py in the row's format (signed zeros, subnormals,
     ties behind each of the three roundings in both parities, products that underflow; tests/test_dequant_specials_cpu.py pins
     that it tells a fused multiply-add, an unrounded sum, a flushed subnormal or a truncation in any step from the reference in
     thousands of weights) - one full period of 1856 stored columns plus the last 64 where the width repeats it - and 64 columns
     of a vo.make_layer(dist="llm") layer of the same format: the first and last chunk of 8 and both sides of the row's edges.
  2. special activations (fp16 subnormals only; +0 / -0 / the largest finite value / ordinary values) and a layer whose finite
     parameters overflow in a few weights (tests/_dequant_specials.py:overflow_layer), against the float64 model with
     _arith_model.check_outputs' bounds and nothing added - through every row, so every family at each of its rows' token counts.

REBUILD PATHS.  What changes the instructions between an index and the rebuilt weight, per kernel file, and the rows that run it
(every row in fp16 and bf16 unless noted; launch-shape classes - sweeps, units, slots, passes, rows per wave - have no rows here):

  kernel            argument / branch                                    instructions                                   rows
  gemv_k256         DT (FAST = 0); TOK only adds multiply-adds           f16: packed add2_g / mul2_bcast_g / add2_bcast_g k256 t1, t3
                                                                         bf16: BF16::add4 / scale_bias4 / fma4 dot blocks
  gemv_k256m        FAST = 0: kSB = 0 (scale, bias from registers:      f16: add2 / mul2_bcast / add2_bcast, weights     k256m sb0, sb1,
                    fp16, 1 token, up to 5 sweeps) / kSB = 1 (from      as operands of the 4x4x4 MFMA                    tok2, tok4
                    LDS: bf16; fp16 wider or 2+ tokens); TOK = 2 / 4     bf16: three roundings on the matrix pipe
                    (more_tokens: the same weight registers again)       (one-hot first operands, 11 MFMAs per index)
  gemv_k256c        MODE = exact (scale and bias always staged in LDS    as gemv_k256m; fp16 two row subgroups at once    k256c n32, n9
                    beside x: one path per type); permuted layers read
                    x[perm] gathered by a launch in front
  gemm_k256         DT; TB = 1 (gemm_k256), TB = 2 / 3 / 4 (gemm_k256w)  DT::add4 / scale_bias4 (bf16: dot blocks), the   gemm_k256 t16,
                                                                         tile as 16x16x32 MFMA operands                  k256w tb2 - tb4
  grouped entry     vptq_quant_gemv_grouped of the canonical format      gemv_k256m's kernel, entry = 0                   grouped n8
  gemv_sliced<EX>   RES = 0 / 1 (256-entry residual table in LDS),       f16: add2_g ... ; bf16: add4 / scale_bias4 /     sliced res0, res1,
                    RG = 1 (residual entry gathered from L2), V = 8 /    fma4 dot blocks; sums in 2^-30 / 2^-28 fixed     rg v8, rg v16,
                    16, TOK = 2 / 3, WPT (window parts), column parts    point                                            v16, tok2, tok3,
                                                                                                                          wparts, parts
  gemv_sliced_tok   EX = 1: TOK = 4 / 8 (16x16x32 MFMA, weights and      DT::add2 / mul2 (widened for bf16), weights as   sliced_tok t4, t5,
                    activations as 16-bit operands), V, RES              MFMA operands, fp32 sums                         t8, v16
  gemv_gather       T = 16 / 24 / 32 (kResLds for T = 24), TOK,          add2 / mul2_bcast / add2_bcast                   gather t16, t24,
                    WIDE = 1 (T = 24, one token, >= 6144 columns: 8                                                       t32, t8, wide
                    24-bit elements out of 6 words, Fmt<24, true>)
  gemv_gatherx      V = 8 / 16 (and 2 - 12 by the same loop), reslds,    the same; outlier columns: one entry, add2(mul2) gatherx v8, v16,
                    has_res, odd index widths (unpack_elem), groups,                                                      r65536, odd, t8,
                    outlier columns, TOK                                                                                  v16-t4, groups,
                                                                                                                          outliers
  gemv_generic      V, TOK                                               add2(mul2(w, s), b) per pair                     generic (t2), t1, t8
  gemv_lds          fp16 only (bf16 with VPTQ_GEMV_EXACT goes to         add2 / mul2_bcast / add2_bcast                   lds (f16),
                    gemv_gatherx: row lds-bf16)                                                                           lds-bf16
  gemv_v2           V, TOK; uint8 / uint16 residual ids                  add2, mul2, add2                                 v2, v2-t3, v2-t8
  gemm_gather       T = 16 (gt_rebuild<DT, false>: no add4, no first     gemm_gather_tile.h: DT::add4 / scale_bias4       gemm_gather t16,
                    rounding), 24 (residual table in LDS), 32 (residual  (bf16: dot blocks), the weight of a column past  (t24), t32
                    entry from L2)                                       the last one masked
  gemm_gatherx      V = 8 / 16; RES = 0 (none: gt_rebuild<DT, false>),   the same                                         gemm_gatherx
                    1 (LDS), 2 (L2)                                                                                       (v16 lds), none,
                                                                                                                          l2, v8-l2, v8-none
  gemm_fused        fp16 tile: add2 / mul2_bcast / add2_bcast            (bf16 is the folded form: no row)                fused (f16)

EXCEPTIONS, derived from the sources (common.h, the comment above BF16::dotp; gemv_sliced.hip, the accumulator word), never from
what the GPU returned:
  fp16                      none
  bf16, dot-block kernels   (gemv_k256, gemm_k256, gemm_k256w, gemm_gather, gemm_gatherx) a weight in the bf16 subnormal range may
                            read as a zero: v_dot2_f32_bf16 flushes denormal results
  bf16, gemv_sliced         a non-zero weight below 2^-21 in magnitude may read as a zero: the accumulator's unit is 2^-28 (and
                            its rebuild uses the dot blocks)
  everything else           none
A row computes its excepted set from the oracle's W, requires bit-equality outside it and a zero inside it wherever the bits
differ; the set is by construction a subset of the oracle's class (so never larger than its count), whose share of the finite table tests/test_dequant_specials_cpu.py keeps
below 15 %.
Overflowing weights: an output whose row holds an infinite weight must be the inf of the model's sign (NaN where contributions of
both signs meet).  NaN instead of that inf is accepted from gemv_sliced (the accumulator word holds no infinity: vptq_hip.h,
VPTQ_GEMV_OUT_F32), from gemv_k256m / gemv_k256c (the weight is an operand of a 4x4x4 MFMA whose other operand is x in one row
and zeros elsewhere: 0 x inf - gemv_k256m.hip's comment on the bf16 path, the same operand layout in fp16), from gemv_sliced_tok
(its 16x16x32 MFMA pairs the rebuilt weight with the zero column in the lanes that carry no token and for elements of another
column phase, whose scale and bias are 0 as well: inf x 0) and from the bf16
dot-block kernels (a dot instruction multiplies the OTHER half of the weight pair by 0: common.h, above BF16::dotp); never a
finite value.  vptq_hip.h states them beside VPTQ_GEMV_EXACT."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_route_models_gpu as rm
from test_route_models_gpu import EXACT, MFMA, VALU, F32, GENERIC
from test_route_models_k256_gpu import instance_of
from test_route_models_sliced_gpu import sliced_instance_of, PARTS
from oracle import vptq_oracle as vo
import _arith_model as am
import _dequant_specials as sp
from _gpu_util import TORCH_DT, spec_to_module, bits_to_tensor, tensor_to_bits, module_desc, v2_desc

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
dev = rm.dev

# which bf16 weights a kernel may read as a zero (the first word of the instance string -> class)
DOT, SLICED = "subnormal", "below 2^-21"
BF16_MAY_READ_ZERO = {"gemv_k256": DOT, "gemm_k256": DOT, "gemm_k256w": DOT, "gemm_gather": DOT, "gemm_gatherx": DOT, "gemv_sliced": SLICED}
NAN_FOR_INF = {"gemv_sliced", "gemv_sliced_tok", "gemv_k256m", "gemv_k256c"}   # (both types; bf16: + the dot-block kernels, nan_for_inf)
PERIOD, TAIL, LLM_COLUMNS = 1856, 64, 64


def nan_for_inf(kernel, dt):
    return kernel in NAN_FOR_INF or (dt == "bf16" and BF16_MAY_READ_ZERO.get(kernel) == DOT)


def Wr(name, kind, dt, per, instance, v=8, k=256, kr=256, cols=PERIOD + TAIL, perm=0, flags=EXACT, edges=(), C=1, S=0, ov=0, special=1):
    """one row.  kind: the entry (gemv, grouped, chain, sliced, gemm_gather, gemm_gatherx, gemm_k256w, fused, v2); per: columns read
    per launch - the tokens of the call, or the copies of the descriptor in a grouped / chain launch; edges: stored columns c
    whose two sides (c - 1, c) the llm layer's sample includes; special: the finite table (and the overflow layer) can express
    the format"""
    e = dict(name=name, kind=kind, dt=dt, per=per, instance=instance, v=v, k=k, kr=kr, cols=cols, perm=perm, flags=flags, edges=edges, C=C, S=S,
             ov=ov, special=special)
    return pytest.param(e, id=f"{name}-{dt}")


def _both(fn):
    return [fn(dt) for dt in ("f16", "bf16")]


K256M = "gemv_k256m dt={dt} ns={ns} nst={nst} perm={p} fast=0 tok={tok} sb={sb} entry={en} slots=4 units=1 sel=0"
SL = "gemv_sliced dt={dt} nsl={nsl} res={res} v={v} two=0 ex=1 rg={rg} tok={tok} wpt={wpt} wparts={wp} parts={parts} n=1 rpw={rpw} arrivals={arr} whole1=0 side={side} perm={p} corr=0"
ST = "gemv_sliced_tok dt={dt} nsl={nsl} res={res} v={v} two=0 tok={tok} ex=1 phases={ph} rpw=1 regsums=1 n=1 whole1=0 perm={p}"
BIG = dict(k=65536, kr=0)
ROWS = [r for pair in [
    # ---- the canonical format
    _both(lambda dt: Wr("k256-t1", "gemv", dt, 1, f"gemv_k256 dt={dt} rows=1 tok=1 sw=2 perm=1 fast=0 entry=1", cols=4104, perm=1, flags=EXACT | VALU,
                        edges=(2048, 4096))),
    _both(lambda dt: Wr("k256-t3", "gemv", dt, 3, f"gemv_k256 dt={dt} rows=1 tok=4 sw=1 perm=0 fast=0 entry=0", cols=2040, flags=EXACT | VALU)),
    [Wr("k256m-sb0", "gemv", "f16", 1, K256M.format(dt="f16", ns=2, nst=1, p=0, tok=1, sb=0, en=1), cols=4096, flags=EXACT | MFMA, edges=(512, 2048)),
     Wr("k256m-sb1", "gemv", "bf16", 1, K256M.format(dt="bf16", ns=2, nst=1, p=0, tok=1, sb=1, en=1), cols=4096, flags=EXACT | MFMA, edges=(512, 2048))],
    _both(lambda dt: Wr("k256m-wide", "gemv", dt, 1, K256M.format(dt=dt, ns=6, nst=2, p=1, tok=1, sb=1, en=1), cols=11008, perm=1, flags=EXACT | MFMA,
                        edges=(2048, 8192, 10240))),
    _both(lambda dt: Wr("k256m-tok2", "gemv", dt, 2, K256M.format(dt=dt, ns=1, nst=1, p=1, tok=2, sb=1, en=0), cols=2040, perm=1, flags=EXACT | MFMA,
                        edges=(512, 1024))),
    _both(lambda dt: Wr("k256m-tok4", "gemv", dt, 4, K256M.format(dt=dt, ns=1, nst=1, p=0, tok=4, sb=1, en=0), cols=2040, flags=EXACT | MFMA,
                        edges=(512, 1024))),
    _both(lambda dt: Wr("grouped-n8", "grouped", dt, 8, K256M.format(dt=dt, ns=1, nst=1, p=0, tok=1, sb=int(dt == "bf16"), en=0), cols=2040,
                        flags=EXACT | MFMA, edges=(512,))),
    _both(lambda dt: Wr("k256c-n32", "chain", dt, 32, f"gemv_k256c dt={dt} dep=0 mode=exact layers=32 sweeps={','.join(['2'] * 32)} perm={','.join(['0'] * 32)}",
                        cols=4096, flags=EXACT | MFMA, edges=(2048,))),
    _both(lambda dt: Wr("k256c-n9-perm", "chain", dt, 9, f"gemv_k256c dt={dt} dep=0 mode=exact layers=9 sweeps={','.join(['1'] * 9)} perm={','.join(['1'] * 9)}",
                        cols=2040, perm=1, flags=EXACT | MFMA, edges=(1024,))),
    _both(lambda dt: Wr("gemm_k256-t16", "gemv", dt, 16, f"gemm_k256 dt={dt} perm=1 tok=16 passes=1", cols=2056, perm=1, edges=(64, 1024, 2048))),
    _both(lambda dt: Wr("gemm_k256-t5", "gemv", dt, 5, f"gemm_k256 dt={dt} perm=0 tok=5 passes=1", cols=2056, edges=(64, 1024, 2048))),
    _both(lambda dt: Wr("k256w-tb2", "gemm_k256w", dt, 32, f"gemm_k256w dt={dt} perm=0 tok=32 tb=2 rgs=1 pass=1x2", cols=2056, flags=0, edges=(64, 2048))),
    _both(lambda dt: Wr("k256w-tb3", "gemm_k256w", dt, 48, f"gemm_k256w dt={dt} perm=1 tok=48 tb=3 rgs=1 pass=1x3", cols=2056, perm=1, flags=0, edges=(64, 2048))),
    _both(lambda dt: Wr("k256w-tb4", "gemm_k256w", dt, 64, f"gemm_k256w dt={dt} perm=0 tok=64 tb=4 rgs=1 pass=1x4", cols=2056, flags=0, edges=(64, 2048))),
    [Wr("fused", "fused", "f16", 64, None, cols=2056, flags=0, edges=(64, 1024, 2048))],
    _both(lambda dt: Wr("generic", "gemv", dt, 2, f"gemv_generic dt={dt} v=8 tok=2", perm=1, flags=EXACT | GENERIC, edges=(256, 1024))),
    # ---- the sliced layouts (k = 65536): one pass of 1 - 3 tokens, column phases of 4 - 8
    _both(lambda dt: Wr("sliced-res0", "sliced", dt, 1, SL.format(dt=dt, nsl=8, res=0, v=8, rg=0, tok=1, wpt=0, wp=1, parts=1, rpw=1, arr=8, side=0, p=1),
                        perm=1, edges=(480, 960, 1440), **BIG)),
    _both(lambda dt: Wr("sliced-res1", "sliced", dt, 1, SL.format(dt=dt, nsl=8, res=1, v=8, rg=0, tok=1, wpt=0, wp=1, parts=1, rpw=1, arr=8, side=1, p=0),
                        k=65536, kr=256, edges=(480, 960, 1440))),
    _both(lambda dt: Wr("sliced-rg-v8", "sliced", dt, 1, SL.format(dt=dt, nsl=8, res=0, v=8, rg=1, tok=1, wpt=0, wp=1, parts=1, rpw=1, arr=8, side=2, p=1),
                        k=65536, kr=65536, perm=1, edges=(480, 960))),
    _both(lambda dt: Wr("sliced-rg-v16", "sliced", dt, 1, SL.format(dt=dt, nsl=16, res=0, v=16, rg=1, tok=1, wpt=0, wp=1, parts=1, rpw=1, arr=16, side=2, p=0),
                        v=16, k=65536, kr=256, edges=(480, 960))),
    _both(lambda dt: Wr("sliced-v16", "sliced", dt, 1, SL.format(dt=dt, nsl=16, res=0, v=16, rg=0, tok=1, wpt=0, wp=1, parts=1, rpw=1, arr=16, side=0, p=1),
                        v=16, perm=1, edges=(480, 960), **BIG)),
    _both(lambda dt: Wr("sliced-tok2", "sliced", dt, 2, SL.format(dt=dt, nsl=8, res=1, v=8, rg=0, tok=2, wpt=0, wp=1, parts=1, rpw=1, arr=8, side=1, p=1),
                        k=65536, kr=256, perm=1, edges=(480, 960))),
    _both(lambda dt: Wr("sliced-tok3", "sliced", dt, 3, SL.format(dt=dt, nsl=8, res=0, v=8, rg=0, tok=3, wpt=0, wp=1, parts=1, rpw=1, arr=8, side=0, p=0),
                        edges=(480, 960), **BIG)),
    _both(lambda dt: Wr("sliced-wparts", "sliced", dt, 2, SL.format(dt=dt, nsl=8, res=1, v=8, rg=0, tok=2, wpt=1, wp=2, parts=1, rpw=2, arr=16, side=1, p=0),
                        k=65536, kr=256, cols=4096, edges=(1024, 2048, 3072))),
    _both(lambda dt: Wr("sliced-parts", "sliced", dt, 1, SL.format(dt=dt, nsl=16, res=1, v=8, rg=0, tok=1, wpt=0, wp=1, parts=2, rpw=1, arr=32, side=1, p=1),
                        k=65536, kr=256, cols=16288, perm=1, edges=(4072, 8144, 12216))),
    _both(lambda dt: Wr("sliced_tok-t4", "sliced", dt, 4, ST.format(dt=dt, nsl=8, res=1, v=8, tok=4, ph=2, p=1), k=65536, kr=256, perm=1,
                        edges=(480, 960, 1440))),
    _both(lambda dt: Wr("sliced_tok-t5", "sliced", dt, 5, ST.format(dt=dt, nsl=8, res=0, v=8, tok=8, ph=2, p=0), edges=(480, 960, 1440), **BIG)),
    _both(lambda dt: Wr("sliced_tok-v16", "sliced", dt, 4, ST.format(dt=dt, nsl=16, res=0, v=16, tok=4, ph=1, p=0), v=16, edges=(480, 960), **BIG)),
    # ---- cache gathers, LDS tables, the v2 entry, batched decode of the large-codebook formats
    _both(lambda dt: Wr("gather-t16", "gemv", dt, 1, f"gemv_gather dt={dt} t=16 rows=1 tok=1 perm=1 wide=0", perm=1, edges=(512, 1024), **BIG)),
    _both(lambda dt: Wr("gather-t24", "gemv", dt, 3, f"gemv_gather dt={dt} t=24 rows=1 tok=4 perm=0 wide=0", k=65536, kr=256, edges=(512, 1024))),
    _both(lambda dt: Wr("gather-t32", "gemv", dt, 1, f"gemv_gather dt={dt} t=32 rows=1 tok=1 perm=1 wide=0", k=65536, kr=65536, perm=1, edges=(512, 1024))),
    _both(lambda dt: Wr("gatherx-v8", "gemv", dt, 1, f"gemv_gatherx dt={dt} v=8 tok=1 perm=1 reslds=1 outl=0 groups=1", k=32768, kr=512, perm=1,
                        edges=(512, 1024))),
    _both(lambda dt: Wr("gatherx-v16", "gemv", dt, 2, f"gemv_gatherx dt={dt} v=16 tok=2 perm=0 reslds=1 outl=0 groups=1", v=16, k=65536, kr=256,
                        edges=(512, 1024))),
    _both(lambda dt: Wr("gatherx-r65536", "gemv", dt, 1, f"gemv_gatherx dt={dt} v=16 tok=1 perm=0 reslds=0 outl=0 groups=1", v=16, k=65536, kr=65536,
                        edges=(512, 1024))),
    _both(lambda dt: Wr("gatherx-odd", "gemv", dt, 1, f"gemv_gatherx dt={dt} v=8 tok=1 perm=1 reslds=1 outl=0 groups=1", k=8192, kr=32, perm=1,
                        edges=(512, 1024))),
    _both(lambda dt: Wr("gatherx-groups", "gemv", dt, 2, f"gemv_gatherx dt={dt} v=6 tok=2 perm=0 reslds=0 outl=0 groups=2", v=6, k=4096, kr=4096, C=2,
                        cols=1032, edges=(516,), special=0)),
    _both(lambda dt: Wr("gatherx-outliers", "gemv", dt, 1, f"gemv_gatherx dt={dt} v=8 tok=1 perm=1 reslds=0 outl=4 groups=1", k=4096, kr=4096, S=64, ov=4,
                        cols=576, perm=1, edges=(64,), special=0)),
    [Wr("lds", "gemv", "f16", 1, "gemv_lds dt=f16 fmt=21 tok=1 rw=1 dma=1 perm=1", k=4096, kr=512, perm=1, edges=(512, 1024)),
     Wr("lds-bf16", "gemv", "bf16", 1, "gemv_gatherx dt=bf16 v=8 tok=1 perm=1 reslds=1 outl=0 groups=1", k=4096, kr=512, perm=1, edges=(512, 1024))],
    [Wr("lds-t3", "gemv", "f16", 3, "gemv_lds dt=f16 fmt=13 tok=4 rw=1 dma=1 perm=0", k=8192, kr=0, edges=(512, 1024))],
    _both(lambda dt: Wr("v2", "v2", dt, 1, f"gemv_v2 dt={dt} v=8 tok=1", k=65536, kr=256, flags=0, edges=(512, 1024))),
    _both(lambda dt: Wr("v2-t3", "v2", dt, 3, f"gemv_v2 dt={dt} v=8 tok=4", k=4096, kr=4096, flags=0, edges=(512, 1024))),
    _both(lambda dt: Wr("gather-wide", "gemv", dt, 1, f"gemv_gather dt={dt} t=24 rows=1 tok=1 perm=1 wide=1", k=65536, kr=256, cols=6144, perm=1,
                        edges=(2048, 4096))),
    _both(lambda dt: Wr("gather-t8", "gemv", dt, 8, f"gemv_gather dt={dt} t=24 rows=1 tok=8 perm=0 wide=0", k=65536, kr=256, edges=(512, 1024))),
    _both(lambda dt: Wr("gatherx-t8", "gemv", dt, 8, f"gemv_gatherx dt={dt} v=8 tok=8 perm=0 reslds=1 outl=0 groups=1", k=32768, kr=512, edges=(512, 1024))),
    _both(lambda dt: Wr("gatherx-v16-t4", "gemv", dt, 4, f"gemv_gatherx dt={dt} v=16 tok=4 perm=0 reslds=1 outl=0 groups=1", v=16, k=65536, kr=256,
                        edges=(512, 1024))),
    _both(lambda dt: Wr("generic-t1", "gemv", dt, 1, f"gemv_generic dt={dt} v=8 tok=1", flags=EXACT | GENERIC, edges=(256, 1024))),
    _both(lambda dt: Wr("generic-t8", "gemv", dt, 8, f"gemv_generic dt={dt} v=8 tok=8", perm=1, flags=EXACT | GENERIC, edges=(256, 1024))),
    _both(lambda dt: Wr("v2-t8", "v2", dt, 8, f"gemv_v2 dt={dt} v=8 tok=8", k=65536, kr=256, flags=0, edges=(512, 1024))),
    _both(lambda dt: Wr("sliced_tok-t8", "sliced", dt, 8, ST.format(dt=dt, nsl=8, res=1, v=8, tok=8, ph=2, p=0), k=65536, kr=256, edges=(480, 960, 1440))),
    _both(lambda dt: Wr("gemm_gather-t16", "gemm_gather", dt, 16, f"gemm_gather dt={dt} t=16 perm=0 tok=16 tiles=2 rgs=1", flags=0, edges=(1024,), **BIG)),
    _both(lambda dt: Wr("gemm_gather-t32", "gemm_gather", dt, 16, f"gemm_gather dt={dt} t=32 perm=1 tok=16 tiles=2 rgs=1", k=65536, kr=65536, perm=1, flags=0,
                        edges=(1024,))),
    _both(lambda dt: Wr("gemm_gatherx-none", "gemm_gatherx", dt, 16, f"gemm_gatherx dt={dt} v=16 ib=16 rb=0 res=none perm=1 tok=16 tiles=2 wgcu=4 rgs=1", v=16,
                        perm=1, flags=0, edges=(1024,), **BIG)),
    _both(lambda dt: Wr("gemm_gatherx-l2", "gemm_gatherx", dt, 16, f"gemm_gatherx dt={dt} v=16 ib=16 rb=16 res=l2 perm=0 tok=16 tiles=2 wgcu=4 rgs=1", v=16,
                        k=65536, kr=65536, flags=0, edges=(1024,))),
    _both(lambda dt: Wr("gemm_gatherx-v8-l2", "gemm_gatherx", dt, 16, f"gemm_gatherx dt={dt} v=8 ib=16 rb=12 res=l2 perm=1 tok=16 tiles=2 wgcu=4 rgs=1",
                        k=65536, kr=4096, perm=1, flags=0, edges=(1024,))),
    _both(lambda dt: Wr("gemm_gatherx-v8-none", "gemm_gatherx", dt, 16, f"gemm_gatherx dt={dt} v=8 ib=14 rb=0 res=none perm=0 tok=16 tiles=2 wgcu=4 rgs=1",
                        k=16384, kr=0, flags=0, edges=(1024,))),
    _both(lambda dt: Wr("gemm_gather", "gemm_gather", dt, 16, f"gemm_gather dt={dt} t=24 perm=1 tok=16 tiles=2 rgs=1", k=65536, kr=256, perm=1, flags=0,
                        edges=(1024,))),
    _both(lambda dt: Wr("gemm_gatherx", "gemm_gatherx", dt, 16, f"gemm_gatherx dt={dt} v=16 ib=16 rb=8 res=lds perm=0 tok=16 tiles=2 wgcu=4 rgs=1", v=16,
                        k=65536, kr=256, flags=0, edges=(1024,))),
] for r in pair]
SPECIAL_ROWS = [r for r in ROWS if r.values[0]["special"]]


# ---------------------------------------------------------------------------------------------- a row's launch
class Route:
    """the row's entry over the layer L: asserts the instance string, then launch(x [per, I], y [per, O]) - per tokens of one
    call, or one column for each of per copies of the descriptor"""

    def __init__(self, e, L, dev):
        from vptq_amd import _backend as B
        self.e, self.L, self.dev, self.per = e, L, dev, e["per"]
        self.m = spec_to_module(L, dev)
        desc, self.keep = module_desc(self.m)
        lib, kind, per, flags = B.lib(), e["kind"], e["per"], e["flags"]
        sp_ = lambda: B.current_stream_ptr(dev)   # noqa: E731
        self.f32 = kind != "fused"
        if kind == "gemv":
            got = instance_of([desc], per, flags)
            nb = lib.vptq_quant_gemv_workspace_bytes(desc, per, flags)
            self.ws = torch.empty(nb, dtype=torch.uint8, device=dev) if nb else None
            wp = None if self.ws is None else self.ws.data_ptr()
            self.run = lambda x, y, f: lib.vptq_quant_gemv(desc, x.data_ptr(), y.data_ptr(), per, flags | f, wp, nb, sp_())
        elif kind in ("grouped", "chain"):
            descs = (B.LayerDesc * per)(*([desc] * per))
            got = instance_of([desc] * per, 1, flags, kind)
            xp, yp = (C.c_void_p * per)(), (C.c_void_p * per)()

            def pointers(x, y):
                for i in range(per):
                    xp[i], yp[i] = x[i].data_ptr(), y[i].data_ptr()
            if kind == "grouped":
                def run(x, y, f):
                    pointers(x, y)
                    return lib.vptq_quant_gemv_grouped(descs, per, xp, yp, 1, flags | f, sp_())
            else:
                name = lib.vptq_quant_gemv_chain_kernel_name(descs, per, 1, flags)
                assert name is not None and name.decode() == "gemv_k256c_kernel"
                nb = lib.vptq_quant_gemv_chain_workspace_bytes_for(descs, per, flags)
                self.ws = torch.zeros(max(nb, 16), dtype=torch.uint8, device=dev)

                def run(x, y, f):
                    pointers(x, y)
                    return lib.vptq_quant_gemv_chain(descs, per, xp, yp, 1, flags | f, self.ws.data_ptr(), nb, sp_())
            self.run = run
        elif kind == "sliced":
            from vptq_amd.utils.sliced import SlicedGemv
            sl = self.sl = SlicedGemv(self.m, exact=True)
            if sl.parts > 1:
                got = sliced_instance_of(sl._part_descs, sl._lay_ref, sl.parts, per, EXACT | PARTS)
            else:
                got = sliced_instance_of((B.LayerDesc * 1)(sl.desc), sl._lay_ref, 1, per, EXACT)

            def run(x, y, f):
                out = sl(x, out=y, flags=f) if per == 1 else sl.forward_tokens(x, out=y, flags=f)
                assert out is not None, "the sliced entry turned the call down"
                return 0
            self.run = run
        elif kind in ("gemm_gather", "gemm_gatherx", "gemm_k256w"):
            buf = C.create_string_buffer(512)
            B.check(getattr(lib, f"vptq_quant_{kind}_instance")(desc, per, flags, buf, len(buf)), f"vptq_quant_{kind}_instance")
            got = buf.value.decode()
            fn = getattr(lib, f"vptq_quant_{kind}")
            self.run = lambda x, y, f: fn(desc, x.data_ptr(), y.data_ptr(), per, flags | f, sp_())
        elif kind == "fused":
            assert lib.vptq_quant_gemm_supported(desc) == 1
            got = None
            nb = lib.vptq_quant_gemm_workspace_bytes(desc, per)
            self.ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
            self.run = lambda x, y, f: lib.vptq_quant_gemm(desc, x.data_ptr(), y.data_ptr(), per, flags, self.ws.data_ptr() if nb else None, nb, sp_())
        elif kind == "v2":
            idx, ridx = vo.unpack_indices(L.indices, L.index_bits, L.group_size, L.res_bits, False)
            t = dict(I=L.in_features, O=L.out_features, v=L.vector_len, k=L.num_centroids, kr=L.num_res_centroids,
                     ids=torch.from_numpy(idx[0].astype(np.uint16).view(np.int16).copy()).to(dev), cent=self.m.centroids.weight,
                     rids=torch.from_numpy((ridx[0].astype(np.uint8) if L.num_res_centroids <= 256 else
                                            ridx[0].astype(np.uint16).view(np.int16)).copy()).to(dev),
                     rcent=self.m.res_centroids.weight, scale=self.m.weight_scale, sbias=self.m.weight_bias)
            vd, self.keep2 = v2_desc(t, L.dtype)
            buf = C.create_string_buffer(512)
            B.check(lib.vptq_quant_gemv_v2_instance(vd, per, flags, buf, len(buf)), "vptq_quant_gemv_v2_instance")
            got = buf.value.decode()
            self.run = lambda x, y, f: lib.vptq_quant_gemv_v2(vd, x.data_ptr(), y.data_ptr(), per, flags | f, sp_())
        else:
            raise ValueError(kind)
        assert got == e["instance"], got
        self.kernel = (e["instance"] or "gemm_fused").split()[0]

    def launch(self, x, y, f32=False):
        from vptq_amd import _backend as B
        assert x.shape[0] == self.per and x.is_contiguous() and y.is_contiguous()
        B.check(self.run(x, y, F32 if f32 else 0), self.e["instance"] or "vptq_quant_gemm")

    def tokens(self, xbits, f32=False):
        """y [per, O] (float64) of the activation rows xbits [per, I]; NaN where the launch wrote nothing"""
        x = bits_to_tensor(xbits, self.L.dtype, self.dev).reshape(self.per, self.L.in_features)
        y = torch.full((self.per, self.L.out_features), float("nan"), dtype=torch.float32 if f32 else x.dtype, device=self.dev)
        self.launch(x, y, f32)
        torch.cuda.synchronize()
        return y.double().cpu().numpy()


def _layer(e, kind):
    dt, v, k, kr, I, perm = e["dt"], e["v"], e["k"], e["kr"], e["cols"], bool(e["perm"])
    if kind == "special":
        return sp.special_layer(dt, v, k, kr, finite=True, cols=I, perm=perm)
    if kind == "overflow":
        return sp.overflow_layer(dt, v, k, kr, cols=I, perm=perm)[0]
    kw = dict(outlier_size=e["S"], outlier_vector_len=e["ov"], num_outlier_centroids=256) if e["S"] else {}
    return vo.make_layer(I, sp.ROWS * v, dist="llm", seed=I + v + kr % 97 + len(e["name"]), dtype=dt, vector_len=v, num_centroids=k,
                         num_res_centroids=kr, num_codebooks=e["C"], enable_perm=perm, **kw)


def _features(L, stored):
    """the input features the stored columns read: x[perm[c]] meets stored column c"""
    stored = np.asarray(stored, dtype=np.int64)
    return stored if L.perm is None else np.ascontiguousarray(L.perm).view(np.uint16).astype(np.int64)[stored]


def read_columns(route, features):
    """-> bits [len(features), O]: W[:, features] as the route's kernel rebuilds it, one one-hot activation row per feature"""
    L, dev, per = route.L, route.dev, route.per
    n = len(features)
    padded = np.concatenate([features, np.repeat(features[-1:], (-n) % per)])
    x = torch.zeros(len(padded), L.in_features, dtype=TORCH_DT[L.dtype], device=dev)
    x[torch.arange(len(padded), device=dev), torch.from_numpy(padded).to(dev)] = 1.0
    y = torch.full((len(padded), L.out_features), float("nan"), dtype=x.dtype, device=dev)
    for j in range(0, len(padded), per):
        route.launch(x[j:j + per], y[j:j + per])
    torch.cuda.synchronize()
    return tensor_to_bits(y[:n])


def check_bits(got, W, features, dt, kernel, what):
    """got [n, O] against vptq_dequant's W [O, I] at `features`: bit-equal (-0 == +0) outside the kernel's excepted class, equal or
    a zero inside it; -> (weights excepted, weights of the class)"""
    want = np.ascontiguousarray(W[:, features].T)
    zero = lambda a: (a & 0x7fff) == 0   # noqa: E731
    same = (got == want) | (zero(got) & zero(want))
    cls = BF16_MAY_READ_ZERO.get(kernel) if dt == "bf16" else None
    may = sp.subnormal_mask(want, dt) if cls == DOT else sp.tiny_mask(want, dt, 2.0 ** -21) if cls == SLICED else np.zeros(want.shape, bool)
    used = ~same & may & zero(got)
    bad = ~same & ~used
    print(f"{what}: {want.size} weights, class '{cls}': {int(may.sum())} ({may.mean():.4f}), read as a zero: {int(used.sum())}, wrong: {int(bad.sum())}")
    if bad.any():
        at = np.argwhere(bad)
        sub, tiny = sp.subnormal_mask(want, dt), sp.tiny_mask(want, dt, 2.0 ** -21)
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.size} weights differ from vptq_dequant's ({int((bad & sub).sum())} subnormal, "
            f"{int((bad & tiny).sum())} below 2^-21, {int((bad & zero(got)).sum())} read as a zero, {int((bad & zero(want)).sum())} zeros read as something), e.g. " +
            ", ".join(f"[col {int(features[c])}, out {r}] got {got[c, r]:#06x} want {want[c, r]:#06x}" for c, r in at[:8]))
    return int(used.sum()), int(may.sum())


def _dequant_bits(route):
    W = tensor_to_bits(route.m.dequant())
    assert W.shape == (route.L.out_features, route.L.in_features)
    return W


# ---------------------------------------------------------------------------------------------- 1. weights bit for bit
@pytest.mark.parametrize("e", SPECIAL_ROWS)
def test_special_weights_read_back(e, dev):
    L = _layer(e, "special")
    route = Route(e, L, dev)
    I = L.in_features
    stored = np.arange(min(PERIOD, I)) if I <= PERIOD + TAIL else np.concatenate([np.arange(PERIOD), np.arange(I - TAIL, I)])
    features = _features(L, stored)
    W = _dequant_bits(route)
    sp.same_bits(W, vo.dequant(L, ref_residual_mask_quirk=False), L.dtype, "vptq_dequant against the oracle")
    check_bits(read_columns(route, features), W, features, L.dtype, route.kernel, f"{e['name']} {L.dtype} special table")


def _llm_sample(e, I):
    cols = set(range(8)) | set(range(I - 8, I))
    for c in e["edges"]:
        assert 0 < c < I
        cols |= {c - 1, c}
    rng = np.random.default_rng(I + len(cols))
    while len(cols) < LLM_COLUMNS:
        cols.add(int(rng.integers(0, I)))
    return np.array(sorted(cols))


@pytest.mark.parametrize("e", ROWS)
def test_llm_weights_read_back(e, dev):
    L = _layer(e, "llm")
    route = Route(e, L, dev)
    features = _features(L, _llm_sample(e, L.in_features))
    W = _dequant_bits(route)
    check_bits(read_columns(route, features), W, features, L.dtype, route.kernel, f"{e['name']} {L.dtype} llm layer")


# ---------------------------------------------------------------------------------------------- 2. activations and weights at the edges
def _extra(route):
    if route.kernel != "gemv_sliced":
        return 0.0
    return am.sliced_extra_abs(route.L.dtype, int(dict(p.split("=") for p in route.e["instance"].split()[1:])["arrivals"]))


def _check_tokens(route, L, x, what):
    mm, aa = am.model(am.pieces(L), x, arith="exact")
    y16 = route.tokens(x)
    am.check_outputs(y16, mm, aa, L.dtype, False, _extra(route), what=what + " [16-bit]")
    if route.f32:
        am.check_outputs(route.tokens(x, f32=True), mm, aa, L.dtype, True, _extra(route), what=what + " [fp32]")
    return y16


def _scaled(L, factor):
    import dataclasses
    s = vo.from_f32((vo.to_f32(L.weight_scale, L.dtype).astype(np.float64) * factor).astype(np.float32), L.dtype)
    assert np.isfinite(vo.to_f32(s, L.dtype)).all()
    return dataclasses.replace(L, weight_scale=s)


@pytest.mark.parametrize("e", ROWS)
def test_subnormal_activations_vs_the_model(e, dev):
    """fp16: x of subnormals only, |x| in [2^-24, 2^-15], the scale times 2^12 so that the outputs are normal numbers; bf16: |x| in
    [2^-120, 2^-110] and the scale times 2^100.  A kernel that flushes such operands returns zeros"""
    dt = e["dt"]
    L = _scaled(_layer(e, "llm"), 2.0 ** (12 if dt == "f16" else 100))
    route = Route(e, L, dev)
    rng = np.random.default_rng(7 + e["per"])
    shape = (e["per"], L.in_features)
    if dt == "f16":
        mag = rng.integers(1, 513, size=shape) * 2.0 ** -24
    else:
        mag = (1 + rng.integers(0, 128, size=shape) / 128.0) * 2.0 ** rng.integers(-120, -110, size=shape)
    x = vo.from_f32((mag * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32), dt)
    xf = np.abs(vo.to_f32(x, dt).astype(np.float64))
    assert xf.min() > 0 and (xf.max() <= 2.0 ** -15 if dt == "f16" else xf.max() < 2.0 ** -109)
    y = _check_tokens(route, L, x, f"{e['name']} {dt} subnormal activations")
    assert (np.abs(y) >= sp.FMT[dt]["norm"]).mean() > 0.9, "the outputs were meant to be normal numbers"


@pytest.mark.parametrize("e", ROWS)
def test_zeros_and_the_largest_value_vs_the_model(e, dev):
    """x mixing +0, -0, the largest finite value at three columns per token, small values and ordinary ones.  The sliced one-pass
    kernels take the largest power of two whose products stay inside their accumulator word's share per arrival instead (vptq_hip.h,
    VPTQ_GEMV_OUT_F32: a partial sum beyond it is NaN by contract)"""
    dt = e["dt"]
    L = _layer(e, "llm")
    route = Route(e, L, dev)
    rng = np.random.default_rng(11 + e["per"])
    T, I = e["per"], L.in_features
    big = sp.FMT[dt]["big"]
    if route.kernel == "gemv_sliced":
        arrivals = int(dict(p.split("=") for p in e["instance"].split()[1:])["arrivals"])
        wmax = float(np.abs(vo.to_f32(vo.dequant(L, ref_residual_mask_quirk=False), dt)).max())
        big = min(big, 2.0 ** np.floor(np.log2(2.0 ** (19 if dt == "f16" else 21) / arrivals / (16 * wmax))))
    x = rng.standard_normal((T, I)) * 2.0 ** -6
    kind = rng.integers(0, 8, size=(T, I))
    x[kind == 0], x[kind == 1] = 0.0, -0.0
    x[kind == 2] = rng.standard_normal(int((kind == 2).sum()))
    for t in range(T):
        x[t, rng.choice(I, 3, replace=False)] = big * rng.choice([-1.0, 1.0], size=3)
    xb = vo.from_f32(x.astype(np.float32), dt)
    assert (xb == 0x8000).any() and (xb == 0).any()
    _check_tokens(route, L, xb, f"{e['name']} {dt} zeros and the largest value")


@pytest.mark.parametrize("e", SPECIAL_ROWS)
def test_overflowing_weights_vs_the_model(e, dev):
    """overflow_layer in the row's format and a dense activation without a zero: an output whose row holds an infinite weight is the
    inf of the model's sign (NaN where both signs meet; NaN for inf where nan_for_inf says so), every other output meets the model"""
    dt = e["dt"]
    L = _layer(e, "overflow")
    route = Route(e, L, dev)
    rng = np.random.default_rng(13 + e["per"])
    x = rng.standard_normal((e["per"], L.in_features))
    x = np.sign(x) * np.maximum(np.abs(x), 2.0 ** -4)
    if route.kernel == "gemv_sliced" and dt == "bf16":
        # (the columns whose scale is 2^64: ordinary weights times it are beyond the accumulator word's 2^21 - NaN by contract,
        # vptq_hip.h, VPTQ_GEMV_OUT_F32 - unless the activation there is small.  Still no zero; the planted products are inf.)
        x[:, vo.to_f32(L.weight_scale, dt) == sp.FMT[dt]["root"]] *= 2.0 ** -62
    x = vo.from_f32(x.astype(np.float32), dt)
    assert not ((x & 0x7fff) == 0).any()
    P = am.pieces(L)
    hot = np.isinf(P["W"]).any(axis=1)
    assert hot.any() and (~hot).any()
    mm, aa = am.model(P, x, arith="exact")
    assert np.isfinite(mm[:, ~hot]).all() and not np.isfinite(mm[:, hot]).any()
    for f32 in ((False, True) if route.f32 else (False,)):
        y = route.tokens(x, f32=f32)
        what = f"{e['name']} {dt} overflowing weights [{'fp32' if f32 else '16-bit'}]"
        am.check_outputs(y[:, ~hot], mm[:, ~hot], aa[:, ~hot], dt, f32, _extra(route), what=what)
        yh, mh = y[:, hot], mm[:, hot]
        assert not np.isfinite(yh).any(), f"{what}: {int(np.isfinite(yh).sum())} finite outputs in rows that hold an infinite weight"
        assert np.isnan(yh[np.isnan(mh)]).all(), f"{what}: +inf and -inf meet in a sum that is not NaN"
        ok = (yh == mh) | (np.isnan(yh) if nan_for_inf(route.kernel, dt) else False)
        wrong = np.argwhere(~ok & np.isinf(mh))
        assert not len(wrong), (f"{what}: {len(wrong)} outputs are not the inf of the model's sign, e.g. " +
                                ", ".join(f"[token {t}, hot output {o}] got {yh[t, o]} model {mh[t, o]}" for t, o in wrong[:6]))


# ---------------------------------------------------------------------------------------------- the two documented 0 x inf cases, pinned
def _rows(*names):
    return [r for r in ROWS if r.values[0]["name"] in names]


def _dense_nonzero(L, per, seed):
    x = np.random.default_rng(seed).standard_normal((per, L.in_features))
    return vo.from_f32((np.sign(x) * np.maximum(np.abs(x), 2.0 ** -4)).astype(np.float32), L.dtype)


TAIL_LANES = {"gemv_k256", "gemv_gather"}   # lanes past the last column rebuild the last chunk of 8 again, against x = 0


@pytest.mark.parametrize("e", _rows("k256-t1", "k256-t3", "gather-t24", "gather-t8", "gatherx-v8", "generic", "lds"))
def test_an_infinite_weight_in_the_last_chunk(e, dev):
    """vptq_hip.h, VPTQ_GEMV_EXACT: gemv_k256 and gemv_gather give NaN, not inf, in the outputs of a vector-row whose infinite weight
    sits in the last 8 columns (these widths leave lanes past the last column); the other kernels of the list, whose tails do not
    rebuild a weight twice, give the model's inf or NaN.  Everywhere: never finite, and the other rows meet the model."""
    dt = e["dt"]
    L, planted = sp.overflow_layer(dt, e["v"], e["k"], e["kr"], cols=e["cols"], perm=bool(e["perm"]), tail=True)
    route = Route(e, L, dev)
    x = _dense_nonzero(L, e["per"], 17 + e["per"])
    P = am.pieces(L)
    hot = np.isinf(P["W"]).any(axis=1)
    mm, aa = am.model(P, x, arith="exact")
    y = route.tokens(x)
    am.check_outputs(y[:, ~hot], mm[:, ~hot], aa[:, ~hot], dt, False, what=f"{e['name']} {dt} rows without an infinite weight")
    assert not np.isfinite(y[:, hot]).any()
    row2 = slice(2 * e["v"], 3 * e["v"])   # the vector-row of the infinity in the last chunk
    if route.kernel in TAIL_LANES:
        assert np.isnan(y[:, row2]).all(), "the tail lanes' 0 x inf: documented as NaN"
    rest = hot.copy()
    if route.kernel in TAIL_LANES:
        rest[row2] = False
    yh, mh = y[:, rest], mm[:, rest]
    assert np.isnan(yh[np.isnan(mh)]).all()
    ok = (yh == mh) | (np.isnan(yh) if nan_for_inf(route.kernel, dt) else False)
    assert ok[np.isinf(mh)].all(), f"{e['name']} {dt}: an output that is neither the model's inf nor an allowed NaN"


@pytest.mark.parametrize("e", _rows("sliced-res1", "sliced-tok2", "sliced_tok-t4", "sliced_tok-t8", "gather-t24", "gatherx-v16"))
def test_entries_zero_that_overflow_together(e, dev):
    """vptq_hip.h, VPTQ_GEMV_EXACT: the padding elements of a sliced layout rebuild (entry 0 of a slice + residual entry 0) x 0.  Here that
    sum is big + half_ulp_big and no index of the layer points at either entry: W is finite outside the planted rows.  The sliced
    kernels' outputs there meet the model or are NaN - never a wrong finite value - and NaN does occur (every row of these layers
    carries padding in slice 0); kernels without a layout (the last two rows) meet the model as if the entries were not there."""
    dt = e["dt"]
    L, _ = sp.overflow_layer(dt, e["v"], e["k"], e["kr"], cols=e["cols"], perm=bool(e["perm"]), entry0=True)
    route = Route(e, L, dev)
    x = _dense_nonzero(L, e["per"], 19 + e["per"])
    if route.kernel == "gemv_sliced" and dt == "bf16":   # (as in test_overflowing_weights_vs_the_model)
        x = vo.to_f32(x, dt).astype(np.float64)
        x[:, vo.to_f32(L.weight_scale, dt) == sp.FMT[dt]["root"]] *= 2.0 ** -62
        x = vo.from_f32(x.astype(np.float32), dt)
    P = am.pieces(L)
    cold = ~np.isinf(P["W"]).any(axis=1)
    mm, aa = am.model(P, x, arith="exact")
    y = route.tokens(x)
    sliced = route.kernel in ("gemv_sliced", "gemv_sliced_tok")
    bad = am.violations(y[:, cold], mm[:, cold], aa[:, cold], dt, False, _extra(route), allow_nan=sliced)[0]
    assert not bad.any(), f"{e['name']} {dt}: {int(bad.sum())} outputs of rows without an infinite weight are neither the model's nor NaN"
    print(f"{e['name']} {dt}: {int(np.isnan(y[:, cold]).sum())} of {y[:, cold].size} outputs NaN")
    if sliced:
        assert np.isnan(y[:, cold]).any(), "the padding's 0 x inf: documented as NaN"
