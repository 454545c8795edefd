"""The remaining GEMV families - gemv_gather, gemv_gatherx, gemv_generic, gemv_lds, gemv_lds_mfma and the v2 entry's gemv_v2 - held
to the per-output float64 models of tests/_arith_model.py at EVERY INSTANTIATION, as tests/test_route_models_k256_gpu.py does for
the canonical format and tests/test_route_models_sliced_gpu.py for the sliced family.  Each row names the instance string
vptq_quant_gemv_instance / vptq_quant_gemv_v2_instance must give (the kernel is its first word) before the 16-bit and the
VPTQ_GEMV_OUT_F32 outputs of every output element are checked, with check_outputs' bounds and nothing added.  y is filled with NaN
before each call: an output the launch does not write fails its row.

Models: the reference's roundings (exact) for gemv_gather, gemv_gatherx, gemv_generic, gemv_v2 and fp16 gemv_lds; the folded form
with s x unrounded and c + r kept in fp32 for bf16 gemv_lds (gemv_lds.hip's file comment); the folded form with f16(s x) for
gemv_lds_mfma.  Folded rows take the planted activation, exact rows the dense one.

ROWS is written by tools/gen_other_rows.py: a greedy cover, cheapest layers first, of the cells tests/test_instance_census_cpu.py
enumerates for these families; EDGES are the shapes chosen by hand (tokens past one launch's slots, ragged and short columns,
spare outputs and spare rows, N = 1, the residual table at and past 32 KiB, the LDS budget's last width, ...).  BIG rows cannot be
small (gemv_gather<WIDE> with ROWS = 2 needs 2048 vector-rows of 6144 columns, gemv_lds_mfma's later staging passes more than
8192 columns of 1024 vector-rows): their model is built in row blocks of at most 16 M weights (am.pieces_blocks) and every output
is still checked (profiles/r13/README.md has the seconds these rows take)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import test_route_models_gpu as rm
from test_route_models_gpu import EXACT, GENERIC, _check, _np, _dense, _planted
from oracle import vptq_oracle as vo
import _arith_model as am
from _gpu_util import spec_to_module, bits_to_tensor, gemv_abi_nan, gemv_v2_abi_nan, v2_desc, kernel_name, module_desc

pytestmark = pytest.mark.gpu
dev = rm.dev

FOLDED_UNROUNDED = dict(rounded=False, round_sx=False)   # bf16 gemv_lds: (c + r) in fp32 times s x in fp32, + sum b x


def arith_of(instance, dt):
    """-> (arith, model kwargs) of the family a row's instance names"""
    name = instance.split()[0]
    if name == "gemv_lds_mfma":
        return "folded", {}
    if name == "gemv_lds" and dt == "bf16":
        return "folded", dict(FOLDED_UNROUNDED)
    return "exact", {}


def R(I, O, dt, tokens, instance, v=8, k=4096, kr=0, C=1, perm=0, bias=0, norm=1, S=0, ov=0, flags=0, dist="llm", x=None, big=0):
    """a packed layer through vptq_quant_gemv: I input columns (S outlier columns of an ov-long codebook + C groups), O outputs"""
    arith, kw = arith_of(instance, dt)
    e = dict(entry="packed", I=I, O=O, dt=dt, tokens=tokens, instance=instance, v=v, k=k, kr=kr, C=C, perm=perm, bias=bias, norm=norm, S=S,
             ov=ov, flags=flags, dist=dist, x=x or ("dense" if arith == "exact" else "planted"), big=big, arith=arith, **kw)
    name = instance.split()[0]
    return pytest.param(e, id=f"{name}-{dt}-{I}x{O}-v{v}k{k}r{kr}c{C}-t{tokens}-f{flags}-p{perm}b{bias}n{norm}s{S}o{ov}-{dist}-{e['x']}")


def V(I, O, dt, tokens, instance, v=8, k=8192, kr=0, rb=0, bias=0, norm=1, flags=0, dist="llm", x=None):
    """a layer of the v2 wire format through vptq_quant_gemv_v2: rb bytes per residual id (0: by kr, uint8 up to 256 entries)"""
    arith, kw = arith_of(instance, dt)
    e = dict(entry="v2", I=I, O=O, dt=dt, tokens=tokens, instance=instance, v=v, k=k, kr=kr, rb=rb or (0 if not kr else 1 if kr <= 256 else 2),
             bias=bias, norm=norm, flags=flags, dist=dist, x=x or ("dense" if arith == "exact" else "planted"), arith=arith, **kw)
    name = instance.split()[0]
    return pytest.param(e, id=f"v2-{name}-{dt}-{I}x{O}-v{v}k{k}r{kr}b{e['rb']}-t{tokens}-f{flags}-b{bias}n{norm}-{dist}-{e['x']}")


# ---------------------------------------------------------------------------------------------- the edges, chosen by hand
EDGES = [
    R(520, 100, "f16", 5,
      "gemv_lds dt=f16 fmt=20 tok=4 rw=1 dma=1 perm=0", kr=256, bias=1),   # 5 fp16 tokens: 4 + 1
    R(520, 100, "bf16", 3,
      "gemv_lds dt=bf16 fmt=20 tok=2 rw=1 dma=1 perm=0", kr=256, bias=1),   # 3 bf16 tokens: 2 + 1
    R(520, 100, "f16", 6,
      "gemv_gatherx dt=f16 v=16 tok=4 perm=1 reslds=1 outl=0 groups=1", v=16, k=65536, kr=1024, perm=1),   # 6 tokens at v = 16: 4 + 2
    R(520, 100, "bf16", 11,
      "gemv_gatherx dt=bf16 v=6 tok=8 perm=0 reslds=1 outl=0 groups=1", v=6, kr=16, bias=1),   # 11 tokens at v = 6: 8 + 3
    R(520, 100, "f16", 9,
      "gemv_gather dt=f16 t=24 rows=1 tok=8 perm=1 wide=0", k=65536, kr=256, perm=1, bias=1),   # 9 tokens: 8 + 1
    R(520, 100, "bf16", 9,
      "gemv_gather dt=bf16 t=16 rows=1 tok=8 perm=0 wide=0", k=65536),   # 9 tokens: 8 + 1
    R(520, 100, "f16", 9,
      "gemv_generic dt=f16 v=8 tok=8", k=256, kr=256, bias=1, flags=GENERIC, x="planted"),   # 9 tokens: 8 + 1
    R(264, 100, "bf16", 13,
      "gemv_generic dt=bf16 v=12 tok=8", v=12, kr=4096, perm=1, flags=GENERIC),   # 13 tokens: 8 + 5
    V(520, 96, "f16", 9,
      "gemv_v2 dt=f16 v=16 tok=8", v=16, k=16384, kr=256, bias=1),   # v2, 9 tokens: 8 + 1
    V(520, 96, "bf16", 9,
      "gemv_v2 dt=bf16 v=4 tok=8", v=4, k=16384, kr=512),   # v2, 9 tokens: 8 + 1
    V(520, 96, "f16", 5,
      "gemv_lds dt=f16 fmt=v2u8 tok=4 rw=1 dma=1 perm=0", kr=256, bias=1),   # v2 LDS-resident, 5 tokens: 4 + 1
    V(520, 96, "bf16", 5,
      "gemv_lds dt=bf16 fmt=v2u16 tok=2 rw=1 dma=1 perm=0", kr=512, bias=1),   # v2 LDS-resident, 5 bf16 tokens: 2 + 2 + 1
    R(8, 72, "f16", 1,
      "gemv_gather dt=f16 t=24 rows=1 tok=1 perm=0 wide=0", k=65536, kr=256),   # 8 columns: less than one piece
    R(8, 72, "bf16", 3,
      "gemv_gather dt=bf16 t=32 rows=1 tok=4 perm=1 wide=0", k=65536, kr=65536, perm=1),   # 8 columns
    R(1032, 72, "f16", 2,
      "gemv_gather dt=f16 t=16 rows=1 tok=2 perm=0 wide=0", k=65536, dist='ref-test'),   # 1032 columns: a ragged piece
    R(4104, 72, "f16", 1,
      "gemv_gather dt=f16 t=32 rows=1 tok=1 perm=0 wide=0", k=65536, kr=65536, bias=1, x="planted"),   # 4104 columns
    R(4096, 72, "bf16", 4,
      "gemv_gather dt=bf16 t=24 rows=1 tok=4 perm=0 wide=0", k=65536, kr=256),   # whole pieces
    R(4, 72, "f16", 1,
      "gemv_gatherx dt=f16 v=6 tok=1 perm=0 reslds=0 outl=0 groups=1", v=6),   # 4 columns: one lane
    R(4, 40, "bf16", 2,
      "gemv_gatherx dt=bf16 v=16 tok=2 perm=0 reslds=1 outl=0 groups=1", v=16, k=256, kr=16, norm=0),   # 4 columns, no norm
    R(1028, 72, "f16", 3,
      "gemv_gatherx dt=f16 v=8 tok=4 perm=1 reslds=0 outl=0 groups=1", k=32768, perm=1, dist='ref-test'),   # 1028 columns: a multiple of 4, not of 8
    R(1028, 100, "bf16", 1,
      "gemv_gatherx dt=bf16 v=12 tok=1 perm=0 reslds=0 outl=0 groups=1", v=12, k=65536, kr=4096, bias=1, x="planted"),   # 1028 columns, T = 28
    R(4100, 40, "f16", 1,
      "gemv_gatherx dt=f16 v=10 tok=1 perm=0 reslds=1 outl=0 groups=1", v=10, kr=256),   # 4100 columns
    R(1024, 72, "f16", 8,
      "gemv_gatherx dt=f16 v=4 tok=8 perm=0 reslds=0 outl=0 groups=1", v=4, k=256, bias=1, norm=0),   # whole pieces, no norm
    R(8, 72, "f16", 1,
      "gemv_lds dt=f16 fmt=20 tok=1 rw=1 dma=1 perm=0", kr=256),   # 8 columns: less than one chunk, most waves idle
    R(8, 72, "bf16", 2,
      "gemv_lds dt=bf16 fmt=13 tok=2 rw=1 dma=1 perm=1", k=8192, perm=1),   # 8 columns
    R(520, 72, "f16", 2,
      "gemv_lds dt=f16 fmt=22 tok=2 rw=1 dma=1 perm=0", k=8192, kr=512, bias=1, dist='ref-test', x="planted"),   # 520 columns: one chunk + 8
    R(4104, 72, "f16", 1,
      "gemv_lds dt=f16 fmt=21 tok=1 rw=1 dma=1 perm=1", kr=512, perm=1),   # 4104 columns, T = 21 = 12 + 9
    R(4104, 72, "bf16", 1,
      "gemv_lds dt=bf16 fmt=21 tok=1 rw=1 dma=1 perm=0", k=8192, kr=256),   # 4104 columns, T = 21 = 13 + 8
    R(4096, 72, "f16", 4,
      "gemv_lds dt=f16 fmt=12 tok=4 rw=1 dma=1 perm=0", k=1024, kr=4, norm=0),   # whole chunks, T = 12 = 10 + 2, no norm
    R(512, 136, "bf16", 2,
      "gemv_lds dt=bf16 fmt=20 tok=2 rw=1 dma=1 perm=0", k=2048, kr=512, bias=1, norm=0),   # T = 20 = 11 + 9, no norm
    R(2, 72, "f16", 1,
      "gemv_generic dt=f16 v=2 tok=1", v=2, k=256, kr=256, flags=GENERIC),   # 2 columns
    R(1030, 72, "bf16", 2,
      "gemv_generic dt=bf16 v=6 tok=2", v=6, kr=16, bias=1, norm=0, flags=GENERIC),   # 1030 columns: no multiple of 4 (gemv_gatherx refuses)
    R(1030, 72, "f16", 1,
      "gemv_generic dt=f16 v=8 tok=1", kr=16),   # 1030 columns without the flag: what gemv_gatherx does not take
    V(8, 64, "f16", 1,
      "gemv_lds dt=f16 fmt=v2u8 tok=1 rw=1 dma=1 perm=0", kr=256),   # v2, 8 columns
    V(1032, 64, "f16", 1,
      "gemv_lds dt=f16 fmt=v2 tok=1 rw=1 dma=1 perm=0", norm=0),   # v2, no residual, no norm
    V(1032, 64, "bf16", 2,
      "gemv_lds dt=bf16 fmt=v2 tok=2 rw=1 dma=1 perm=0", bias=1),   # v2, no residual
    V(1030, 64, "f16", 3,
      "gemv_v2 dt=f16 v=8 tok=4", kr=256),   # v2, 1030 columns: no multiple of 8 (the LDS kernels refuse)
    R(264, 5, "f16", 1,
      "gemv_gather dt=f16 t=24 rows=1 tok=1 perm=0 wide=0", k=65536, kr=256, bias=1),   # N = 1, 5 of its 8 outputs
    R(264, 8, "bf16", 2,
      "gemv_lds dt=bf16 fmt=20 tok=2 rw=1 dma=1 perm=0", kr=256, bias=1),   # N = 1
    R(264, 3, "f16", 1,
      "gemv_lds dt=f16 fmt=22 tok=1 rw=1 dma=1 perm=0", k=8192, kr=512),   # N = 1, 3 of its 8 outputs
    R(260, 13, "f16", 2,
      "gemv_gatherx dt=f16 v=16 tok=2 perm=0 reslds=0 outl=0 groups=1", v=16, k=65536, kr=65536, bias=1),   # N = 1, 13 of its 16 outputs
    R(260, 2, "bf16", 1,
      "gemv_gatherx dt=bf16 v=2 tok=1 perm=0 reslds=1 outl=0 groups=1", v=2, k=256, kr=16),   # N = 1 at v = 2
    R(264, 7, "f16", 3,
      "gemv_generic dt=f16 v=10 tok=4", v=10, k=256, kr=256, bias=1, flags=GENERIC),   # N = 1, 7 of its 10 outputs
    V(264, 8, "f16", 1,
      "gemv_lds dt=f16 fmt=v2u16 tok=1 rw=1 dma=1 perm=0", kr=512),   # v2, N = 1
    V(264, 16, "bf16", 2,
      "gemv_v2 dt=bf16 v=16 tok=2", v=16, k=16384, bias=1),   # v2, N = 1 at v = 16
    R(6152, 264, "f16", 1,
      "gemv_gather dt=f16 t=24 rows=1 tok=1 perm=0 wide=1", k=65536, kr=256, bias=1),   # G = 6152: WIDE, a ragged last piece
    R(6152, 264, "bf16", 1,
      "gemv_gather dt=bf16 t=24 rows=1 tok=1 perm=1 wide=1", k=65536, kr=256, perm=1),   # WIDE with a permutation
    R(6136, 264, "f16", 1,
      "gemv_gather dt=f16 t=24 rows=1 tok=1 perm=0 wide=0", k=65536, kr=256),   # G = 6136: just below the switch
    R(264, 16392, "f16", 1,
      "gemv_gather dt=f16 t=16 rows=2 tok=1 perm=0 wide=0", k=65536, bias=1),   # 2049 vector-rows: ROWS = 2, the last group one row
    R(264, 16389, "bf16", 1,
      "gemv_gather dt=bf16 t=32 rows=2 tok=1 perm=1 wide=0", k=65536, kr=65536, perm=1),   # ROWS = 2, spare row and spare outputs
    R(520, 100, "f16", 1,
      "gemv_gatherx dt=f16 v=8 tok=1 perm=0 reslds=1 outl=0 groups=1", k=512, kr=2048, bias=1),   # residual table exactly 32 KiB (v = 8)
    R(520, 100, "f16", 2,
      "gemv_gatherx dt=f16 v=8 tok=2 perm=0 reslds=0 outl=0 groups=1", k=512, kr=4096),   # 64 KiB: gathered from L2
    R(520, 100, "bf16", 1,
      "gemv_gatherx dt=bf16 v=16 tok=1 perm=1 reslds=1 outl=0 groups=1", v=16, k=65536, kr=1024, perm=1),   # exactly 32 KiB (v = 16)
    R(520, 100, "bf16", 4,
      "gemv_gatherx dt=bf16 v=16 tok=4 perm=0 reslds=0 outl=0 groups=1", v=16, k=65536, kr=2048),   # 64 KiB (v = 16)
    R(520, 100, "f16", 1,
      "gemv_gatherx dt=f16 v=6 tok=1 perm=0 reslds=0 outl=0 groups=1", v=6, kr=2),   # 24 bytes: no whole 16-byte units
    R(1028, 40, "f16", 1,
      "gemv_gatherx dt=f16 v=4 tok=1 perm=0 reslds=0 outl=0 groups=1", v=4, k=256),   # T = 8
    R(1028, 40, "bf16", 2,
      "gemv_gatherx dt=bf16 v=8 tok=2 perm=0 reslds=1 outl=0 groups=1", k=512, kr=2, dist='ref-test'),   # T = 10
    R(1028, 40, "f16", 3,
      "gemv_gatherx dt=f16 v=12 tok=4 perm=1 reslds=0 outl=0 groups=1", v=12, k=2048, perm=1),   # T = 11: windows straddle words
    R(1028, 40, "f16", 1,
      "gemv_gatherx dt=f16 v=8 tok=1 perm=0 reslds=0 outl=0 groups=1", k=32768),   # T = 15: the last window ends at the row end
    R(1028, 40, "bf16", 1,
      "gemv_gatherx dt=bf16 v=8 tok=1 perm=0 reslds=1 outl=0 groups=1", k=65536, kr=2),   # T = 17
    R(1028, 40, "f16", 4,
      "gemv_gatherx dt=f16 v=16 tok=4 perm=0 reslds=1 outl=0 groups=1", v=16, k=65536, kr=8, bias=1),   # T = 19
    R(1028, 40, "f16", 1,
      "gemv_gatherx dt=f16 v=8 tok=1 perm=0 reslds=1 outl=0 groups=1", k=32768, kr=256),   # T = 23
    R(1028, 40, "bf16", 1,
      "gemv_gatherx dt=bf16 v=10 tok=1 perm=1 reslds=0 outl=0 groups=1", v=10, k=65536, kr=2048, perm=1),   # T = 27
    R(1028, 40, "f16", 2,
      "gemv_gatherx dt=f16 v=8 tok=2 perm=0 reslds=0 outl=0 groups=1", k=32768, kr=16384),   # T = 29
    R(1028, 40, "f16", 1,
      "gemv_gatherx dt=f16 v=8 tok=1 perm=0 reslds=0 outl=0 groups=1", k=32768, kr=65536),   # T = 31
    R(1028, 40, "bf16", 3,
      "gemv_gatherx dt=bf16 v=16 tok=4 perm=0 reslds=0 outl=0 groups=1", v=16, k=65536, kr=65536, dist='ref-test'),   # T = 32
    R(528, 98, "f16", 1,
      "gemv_gatherx dt=f16 v=8 tok=1 perm=0 reslds=1 outl=same groups=1", k=32768, kr=16, bias=1, S=8, ov=8),   # outliers of the layer's length, O inside a vector
    R(528, 98, "bf16", 2,
      "gemv_gatherx dt=bf16 v=8 tok=2 perm=1 reslds=1 outl=4 groups=1", k=32768, kr=16, perm=1, S=8, ov=4),   # outliers of length 4 under v = 8, O inside an outlier vector
    R(584, 98, "f16", 3,
      "gemv_gatherx dt=f16 v=12 tok=4 perm=0 reslds=0 outl=4 groups=1", v=12, k=65536, S=64, ov=4),   # ... under v = 12
    R(584, 98, "f16", 1,
      "gemv_gatherx dt=f16 v=12 tok=1 perm=1 reslds=0 outl=same groups=1", v=12, k=65536, perm=1, S=64, ov=12),   # ... of length 12
    R(528, 98, "bf16", 1,
      "gemv_gatherx dt=bf16 v=16 tok=1 perm=0 reslds=0 outl=4 groups=1", v=16, kr=4096, bias=1, S=8, ov=4),   # ... under v = 16
    R(528, 98, "f16", 4,
      "gemv_gatherx dt=f16 v=16 tok=4 perm=0 reslds=0 outl=same groups=1", v=16, kr=4096, S=8, ov=16),   # ... of length 16
    R(1040, 100, "f16", 1,
      "gemv_gatherx dt=f16 v=8 tok=1 perm=0 reslds=1 outl=0 groups=2", k=32768, kr=512, C=2, bias=1),   # 2 codebook groups
    R(1040, 100, "bf16", 2,
      "gemv_gatherx dt=bf16 v=6 tok=2 perm=1 reslds=0 outl=0 groups=4", v=6, kr=4096, C=4, perm=1),   # 4 codebook groups
    R(1048, 98, "f16", 1,
      "gemv_gatherx dt=f16 v=8 tok=1 perm=0 reslds=1 outl=4 groups=4", kr=16, C=4, norm=0, S=8, ov=4),   # groups + outliers, no norm
    R(264, 4804, "f16", 1,
      "gemv_lds dt=f16 fmt=20 tok=1 rw=2 dma=1 perm=0", kr=256, bias=1),   # 601 vector-rows: groups of 2
    R(264, 8806, "f16", 1,
      "gemv_lds dt=f16 fmt=20 tok=1 rw=4 dma=1 perm=0", kr=256, flags=EXACT),   # 1101: groups of 4 (one token: by VPTQ_GEMV_EXACT)
    R(264, 16804, "bf16", 2,
      "gemv_lds dt=bf16 fmt=13 tok=2 rw=8 dma=1 perm=1", k=8192, perm=1),   # 2101: groups of 8, waves without a chunk of their own
    R(264, 32804, "f16", 3,
      "gemv_lds dt=f16 fmt=12 tok=4 rw=16 dma=1 perm=0", bias=1),   # 4101: groups of 16
    R(1000, 8806, "f16", 1,
      "gemv_lds_mfma dt=f16 fmt=13 rw=4 stages=1 dma=1 perm=0", k=8192, bias=1),   # 1101 vector-rows, 1000 columns
    R(520, 16804, "bf16", 1,
      "gemv_lds_mfma dt=bf16 fmt=21 rw=8 stages=1 dma=1 perm=1", kr=512, perm=1),   # groups of 8
    R(264, 32804, "f16", 1,
      "gemv_lds_mfma dt=f16 fmt=20 rw=16 stages=1 dma=1 perm=1", kr=256, perm=1, bias=1),   # groups of 16
    R(264, 8806, "bf16", 1,
      "gemv_lds_mfma dt=bf16 fmt=20 rw=4 stages=1 dma=1 perm=0", k=2048, kr=512, norm=0),   # no norm
    V(520, 4800, "f16", 2,
      "gemv_lds dt=f16 fmt=v2u16 tok=2 rw=2 dma=1 perm=0", kr=256, bias=1, rb=2),   # uint16 ids of a 256-entry table
    V(520, 4800, "bf16", 1,
      "gemv_lds dt=bf16 fmt=v2u16 tok=1 rw=2 dma=0 perm=0", k=5000, kr=300),   # k = 5000: no multiple of 64, the table through registers
    V(264, 8808, "f16", 1,
      "gemv_lds_mfma dt=f16 fmt=v2u8 rw=4 stages=1 dma=1 perm=0", kr=256, bias=1),   # v2 on the MFMA variant
    V(264, 8808, "bf16", 1,
      "gemv_lds_mfma dt=bf16 fmt=v2 rw=4 stages=1 dma=0 perm=0", k=1000),   # ... the table through registers
    V(264, 8808, "f16", 1,
      "gemv_lds dt=f16 fmt=v2u16 tok=1 rw=4 dma=1 perm=0", kr=512, flags=EXACT),   # one token by VPTQ_GEMV_EXACT
    V(520, 64, "f16", 1,
      "gemv_v2 dt=f16 v=8 tok=1", kr=256, flags=GENERIC),   # VPTQ_GEMV_FORCE_GENERIC
    V(520, 96, "f16", 3,
      "gemv_v2 dt=f16 v=4 tok=4", v=4, k=16384, kr=256, dist='ref-test', x="planted"),   # k = 16384, v = 4
    V(520, 96, "bf16", 7,
      "gemv_v2 dt=bf16 v=16 tok=8", v=16, k=16384, kr=512, bias=1),   # k = 16384, v = 16, 7 tokens in 8 slots
]

# ---------------------------------------------------------------------------------------------- rows that cannot be small
BIG = [
    R(6152, 16392, "f16", 1,
      "gemv_gather dt=f16 t=24 rows=2 tok=1 perm=0 wide=1", k=65536, kr=256, bias=1, big=1),   # WIDE x ROWS = 2: 100 M weights
    R(6152, 16392, "f16", 1,
      "gemv_gather dt=f16 t=24 rows=2 tok=1 perm=1 wide=1", k=65536, kr=256, perm=1, big=1),
    R(6152, 16392, "bf16", 1,
      "gemv_gather dt=bf16 t=24 rows=2 tok=1 perm=0 wide=1", k=65536, kr=256, big=1),
    R(6152, 16392, "bf16", 1,
      "gemv_gather dt=bf16 t=24 rows=2 tok=1 perm=1 wide=1", k=65536, kr=256, perm=1, bias=1, big=1),
    R(8200, 8192, "bf16", 1,
      "gemv_lds_mfma dt=bf16 fmt=12 rw=4 stages=2 dma=1 perm=0", big=1),   # 2 staging passes: 67 M weights
    R(24584, 8192, "f16", 1,
      "gemv_lds_mfma dt=f16 fmt=12 rw=4 stages=4 dma=1 perm=0", bias=1, big=1),   # 4 staging passes: 201 M weights
    R(24584, 8192, "bf16", 1,
      "gemv_lds_mfma dt=bf16 fmt=12 rw=4 stages=4 dma=1 perm=0", big=1),
    R(11192, 8192, "f16", 1,
      "gemv_lds_mfma dt=f16 fmt=22 rw=4 stages=2 dma=1 perm=0", k=8192, kr=512, big=1),   # the widest G the LDS budget admits at k = 8192 + 512
    R(11200, 8192, "f16", 1,
      "gemv_lds dt=f16 fmt=22 tok=1 rw=4 dma=1 perm=0", k=8192, kr=512, big=1),   # ... and 8 columns more: the kernel with the reference's roundings
]

# ---------------------------------------------------------------------------------------------- one row per census cell
ROWS = [
    R(264, 72, "bf16", 1,
      "gemv_gather dt=bf16 t=16 rows=1 tok=1 perm=0 wide=0", k=65536, bias=1),
    R(264, 72, "bf16", 2,
      "gemv_gather dt=bf16 t=16 rows=1 tok=2 perm=0 wide=0", k=65536, dist='ref-test'),
    R(264, 72, "bf16", 3,
      "gemv_gather dt=bf16 t=16 rows=1 tok=4 perm=0 wide=0", k=65536, bias=1),
    R(264, 72, "bf16", 1,
      "gemv_gather dt=bf16 t=16 rows=1 tok=1 perm=1 wide=0", k=65536, perm=1, dist='ref-test'),
    R(264, 72, "bf16", 2,
      "gemv_gather dt=bf16 t=16 rows=1 tok=2 perm=1 wide=0", k=65536, perm=1, bias=1),
    R(264, 72, "bf16", 3,
      "gemv_gather dt=bf16 t=16 rows=1 tok=4 perm=1 wide=0", k=65536, perm=1, x="planted"),
    R(264, 72, "bf16", 5,
      "gemv_gather dt=bf16 t=16 rows=1 tok=8 perm=1 wide=0", k=65536, perm=1),
    R(264, 16392, "bf16", 1,
      "gemv_gather dt=bf16 t=16 rows=2 tok=1 perm=0 wide=0", k=65536, bias=1),
    R(264, 16392, "bf16", 1,
      "gemv_gather dt=bf16 t=16 rows=2 tok=1 perm=1 wide=0", k=65536, perm=1, dist='ref-test'),
    R(264, 72, "bf16", 1,
      "gemv_gather dt=bf16 t=24 rows=1 tok=1 perm=0 wide=0", k=65536, kr=256, bias=1, dist='ref-test', x="planted"),
    R(264, 72, "bf16", 2,
      "gemv_gather dt=bf16 t=24 rows=1 tok=2 perm=0 wide=0", k=65536, kr=256),
    R(264, 72, "bf16", 5,
      "gemv_gather dt=bf16 t=24 rows=1 tok=8 perm=0 wide=0", k=65536, kr=256, bias=1),
    R(264, 72, "bf16", 1,
      "gemv_gather dt=bf16 t=24 rows=1 tok=1 perm=1 wide=0", k=65536, kr=256, perm=1),
    R(264, 72, "bf16", 2,
      "gemv_gather dt=bf16 t=24 rows=1 tok=2 perm=1 wide=0", k=65536, kr=256, perm=1, bias=1),
    R(264, 72, "bf16", 3,
      "gemv_gather dt=bf16 t=24 rows=1 tok=4 perm=1 wide=0", k=65536, kr=256, perm=1),
    R(264, 72, "bf16", 5,
      "gemv_gather dt=bf16 t=24 rows=1 tok=8 perm=1 wide=0", k=65536, kr=256, perm=1, dist='ref-test'),
    R(264, 16392, "bf16", 1,
      "gemv_gather dt=bf16 t=24 rows=2 tok=1 perm=0 wide=0", k=65536, kr=256, bias=1, dist='ref-test'),
    R(264, 16392, "bf16", 1,
      "gemv_gather dt=bf16 t=24 rows=2 tok=1 perm=1 wide=0", k=65536, kr=256, perm=1),
    R(6152, 72, "bf16", 1,
      "gemv_gather dt=bf16 t=24 rows=1 tok=1 perm=0 wide=1", k=65536, kr=256, bias=1),
    R(264, 72, "bf16", 1,
      "gemv_gather dt=bf16 t=32 rows=1 tok=1 perm=0 wide=0", k=65536, kr=65536, bias=1, dist='ref-test'),
    R(264, 72, "bf16", 2,
      "gemv_gather dt=bf16 t=32 rows=1 tok=2 perm=0 wide=0", k=65536, kr=65536),
    R(264, 72, "bf16", 3,
      "gemv_gather dt=bf16 t=32 rows=1 tok=4 perm=0 wide=0", k=65536, kr=65536, bias=1),
    R(264, 72, "bf16", 5,
      "gemv_gather dt=bf16 t=32 rows=1 tok=8 perm=0 wide=0", k=65536, kr=65536, bias=1),
    R(264, 72, "bf16", 1,
      "gemv_gather dt=bf16 t=32 rows=1 tok=1 perm=1 wide=0", k=65536, kr=65536, perm=1),
    R(264, 72, "bf16", 2,
      "gemv_gather dt=bf16 t=32 rows=1 tok=2 perm=1 wide=0", k=65536, kr=65536, perm=1, bias=1),
    R(264, 72, "bf16", 5,
      "gemv_gather dt=bf16 t=32 rows=1 tok=8 perm=1 wide=0", k=65536, kr=65536, perm=1, dist='ref-test', x="planted"),
    R(264, 16392, "bf16", 1,
      "gemv_gather dt=bf16 t=32 rows=2 tok=1 perm=0 wide=0", k=65536, kr=65536, bias=1, dist='ref-test'),
    R(264, 72, "f16", 1,
      "gemv_gather dt=f16 t=16 rows=1 tok=1 perm=0 wide=0", k=65536),
    R(264, 72, "f16", 3,
      "gemv_gather dt=f16 t=16 rows=1 tok=4 perm=0 wide=0", k=65536, dist='ref-test'),
    R(264, 72, "f16", 5,
      "gemv_gather dt=f16 t=16 rows=1 tok=8 perm=0 wide=0", k=65536, x="planted"),
    R(264, 72, "f16", 1,
      "gemv_gather dt=f16 t=16 rows=1 tok=1 perm=1 wide=0", k=65536, perm=1, bias=1),
    R(264, 72, "f16", 2,
      "gemv_gather dt=f16 t=16 rows=1 tok=2 perm=1 wide=0", k=65536, perm=1, dist='ref-test'),
    R(264, 72, "f16", 3,
      "gemv_gather dt=f16 t=16 rows=1 tok=4 perm=1 wide=0", k=65536, perm=1, bias=1),
    R(264, 72, "f16", 8,
      "gemv_gather dt=f16 t=16 rows=1 tok=8 perm=1 wide=0", k=65536, perm=1),
    R(264, 16392, "f16", 1,
      "gemv_gather dt=f16 t=16 rows=2 tok=1 perm=1 wide=0", k=65536, perm=1, bias=1),
    R(264, 72, "f16", 2,
      "gemv_gather dt=f16 t=24 rows=1 tok=2 perm=0 wide=0", k=65536, kr=256, bias=1, dist='ref-test', x="planted"),
    R(264, 72, "f16", 3,
      "gemv_gather dt=f16 t=24 rows=1 tok=4 perm=0 wide=0", k=65536, kr=256),
    R(264, 72, "f16", 6,
      "gemv_gather dt=f16 t=24 rows=1 tok=8 perm=0 wide=0", k=65536, kr=256, bias=1),
    R(264, 72, "f16", 1,
      "gemv_gather dt=f16 t=24 rows=1 tok=1 perm=1 wide=0", k=65536, kr=256, perm=1, bias=1, dist='ref-test', x="planted"),
    R(264, 72, "f16", 2,
      "gemv_gather dt=f16 t=24 rows=1 tok=2 perm=1 wide=0", k=65536, kr=256, perm=1),
    R(264, 72, "f16", 3,
      "gemv_gather dt=f16 t=24 rows=1 tok=4 perm=1 wide=0", k=65536, kr=256, perm=1, bias=1),
    R(264, 16392, "f16", 1,
      "gemv_gather dt=f16 t=24 rows=2 tok=1 perm=0 wide=0", k=65536, kr=256),
    R(264, 16392, "f16", 1,
      "gemv_gather dt=f16 t=24 rows=2 tok=1 perm=1 wide=0", k=65536, kr=256, perm=1, bias=1, dist='ref-test'),
    R(6152, 72, "f16", 1,
      "gemv_gather dt=f16 t=24 rows=1 tok=1 perm=1 wide=1", k=65536, kr=256, perm=1, bias=1),
    R(264, 72, "f16", 2,
      "gemv_gather dt=f16 t=32 rows=1 tok=2 perm=0 wide=0", k=65536, kr=65536, bias=1, dist='ref-test'),
    R(264, 72, "f16", 3,
      "gemv_gather dt=f16 t=32 rows=1 tok=4 perm=0 wide=0", k=65536, kr=65536),
    R(264, 72, "f16", 7,
      "gemv_gather dt=f16 t=32 rows=1 tok=8 perm=0 wide=0", k=65536, kr=65536, dist='ref-test', x="planted"),
    R(264, 72, "f16", 1,
      "gemv_gather dt=f16 t=32 rows=1 tok=1 perm=1 wide=0", k=65536, kr=65536, perm=1, bias=1, dist='ref-test'),
    R(264, 72, "f16", 2,
      "gemv_gather dt=f16 t=32 rows=1 tok=2 perm=1 wide=0", k=65536, kr=65536, perm=1),
    R(264, 72, "f16", 3,
      "gemv_gather dt=f16 t=32 rows=1 tok=4 perm=1 wide=0", k=65536, kr=65536, perm=1, bias=1),
    R(264, 72, "f16", 10,
      "gemv_gather dt=f16 t=32 rows=1 tok=8 perm=1 wide=0", k=65536, kr=65536, perm=1),
    R(264, 16392, "f16", 1,
      "gemv_gather dt=f16 t=32 rows=2 tok=1 perm=0 wide=0", k=65536, kr=65536),
    R(264, 16392, "f16", 1,
      "gemv_gather dt=f16 t=32 rows=2 tok=1 perm=1 wide=0", k=65536, kr=65536, perm=1, bias=1, dist='ref-test'),
    R(260, 72, "bf16", 2,
      "gemv_gatherx dt=bf16 v=2 tok=2 perm=0 reslds=0 outl=0 groups=1", v=2, k=256, x="planted"),
    R(260, 72, "bf16", 3,
      "gemv_gatherx dt=bf16 v=2 tok=4 perm=0 reslds=0 outl=0 groups=1", v=2, k=256, bias=1),
    R(260, 72, "bf16", 5,
      "gemv_gatherx dt=bf16 v=2 tok=8 perm=0 reslds=0 outl=0 groups=1", v=2, k=256, bias=1),
    R(260, 72, "bf16", 1,
      "gemv_gatherx dt=bf16 v=2 tok=1 perm=1 reslds=0 outl=0 groups=1", v=2, k=256, perm=1, x="planted"),
    R(260, 72, "bf16", 2,
      "gemv_gatherx dt=bf16 v=2 tok=2 perm=1 reslds=0 outl=0 groups=1", v=2, k=256, perm=1, bias=1),
    R(260, 72, "bf16", 3,
      "gemv_gatherx dt=bf16 v=2 tok=4 perm=1 reslds=0 outl=0 groups=1", v=2, k=256, perm=1, dist='ref-test'),
    R(260, 72, "bf16", 5,
      "gemv_gatherx dt=bf16 v=2 tok=8 perm=1 reslds=0 outl=0 groups=1", v=2, k=256, perm=1, norm=0),
    R(260, 72, "bf16", 1,
      "gemv_gatherx dt=bf16 v=4 tok=1 perm=0 reslds=0 outl=0 groups=1", v=4, k=256, bias=1),
    R(260, 72, "bf16", 2,
      "gemv_gatherx dt=bf16 v=4 tok=2 perm=0 reslds=0 outl=0 groups=1", v=4, k=256, dist='ref-test'),
    R(260, 72, "bf16", 3,
      "gemv_gatherx dt=bf16 v=4 tok=4 perm=0 reslds=0 outl=0 groups=1", v=4, k=256, bias=1),
    R(260, 72, "bf16", 5,
      "gemv_gatherx dt=bf16 v=4 tok=8 perm=0 reslds=0 outl=0 groups=1", v=4, k=256, bias=1),
    R(260, 72, "bf16", 1,
      "gemv_gatherx dt=bf16 v=4 tok=1 perm=1 reslds=0 outl=0 groups=1", v=4, k=256, perm=1, dist='ref-test'),
    R(260, 72, "bf16", 2,
      "gemv_gatherx dt=bf16 v=4 tok=2 perm=1 reslds=0 outl=0 groups=1", v=4, k=256, perm=1, bias=1),
    R(260, 72, "bf16", 3,
      "gemv_gatherx dt=bf16 v=4 tok=4 perm=1 reslds=0 outl=0 groups=1", v=4, k=256, perm=1, norm=0),
    R(260, 72, "bf16", 5,
      "gemv_gatherx dt=bf16 v=4 tok=8 perm=1 reslds=0 outl=0 groups=1", v=4, k=256, perm=1),
    R(260, 72, "bf16", 1,
      "gemv_gatherx dt=bf16 v=6 tok=1 perm=0 reslds=0 outl=0 groups=1", v=6, k=256, bias=1),
    R(260, 72, "bf16", 2,
      "gemv_gatherx dt=bf16 v=6 tok=2 perm=0 reslds=0 outl=0 groups=1", v=6, k=256, norm=0),
    R(260, 72, "bf16", 3,
      "gemv_gatherx dt=bf16 v=6 tok=4 perm=0 reslds=0 outl=0 groups=1", v=6, k=256, bias=1),
    R(260, 72, "bf16", 1,
      "gemv_gatherx dt=bf16 v=6 tok=1 perm=1 reslds=0 outl=0 groups=1", v=6, k=256, perm=1, norm=0),
    R(260, 72, "bf16", 3,
      "gemv_gatherx dt=bf16 v=6 tok=4 perm=1 reslds=0 outl=0 groups=1", v=6, k=256, perm=1),
    R(260, 72, "bf16", 5,
      "gemv_gatherx dt=bf16 v=6 tok=8 perm=1 reslds=0 outl=0 groups=1", v=6, k=256, perm=1),
    R(264, 60, "bf16", 3,
      "gemv_gatherx dt=bf16 v=8 tok=4 perm=0 reslds=0 outl=0 groups=1", bias=1, norm=0, flags=EXACT, x="planted"),
    R(264, 60, "bf16", 5,
      "gemv_gatherx dt=bf16 v=8 tok=8 perm=0 reslds=0 outl=0 groups=1", bias=1, flags=EXACT),
    R(264, 60, "bf16", 1,
      "gemv_gatherx dt=bf16 v=8 tok=1 perm=1 reslds=0 outl=0 groups=1", perm=1, flags=EXACT),
    R(264, 60, "bf16", 3,
      "gemv_gatherx dt=bf16 v=8 tok=4 perm=1 reslds=0 outl=0 groups=1", perm=1, flags=EXACT, dist='ref-test'),
    R(264, 60, "bf16", 6,
      "gemv_gatherx dt=bf16 v=8 tok=8 perm=1 reslds=0 outl=0 groups=1", perm=1, bias=1, flags=EXACT),
    R(260, 72, "bf16", 1,
      "gemv_gatherx dt=bf16 v=10 tok=1 perm=0 reslds=0 outl=0 groups=1", v=10, k=256, bias=1, dist='ref-test'),
    R(260, 72, "bf16", 2,
      "gemv_gatherx dt=bf16 v=10 tok=2 perm=0 reslds=0 outl=0 groups=1", v=10, k=256),
    R(260, 72, "bf16", 8,
      "gemv_gatherx dt=bf16 v=10 tok=4 perm=0 reslds=0 outl=0 groups=1", v=10, k=256),
    R(260, 72, "bf16", 2,
      "gemv_gatherx dt=bf16 v=10 tok=2 perm=1 reslds=0 outl=0 groups=1", v=10, k=256, perm=1, bias=1),
    R(260, 72, "bf16", 10,
      "gemv_gatherx dt=bf16 v=10 tok=4 perm=1 reslds=0 outl=0 groups=1", v=10, k=256, perm=1, bias=1, dist='ref-test'),
    R(260, 72, "bf16", 2,
      "gemv_gatherx dt=bf16 v=12 tok=2 perm=0 reslds=0 outl=0 groups=1", v=12, k=256),
    R(260, 72, "bf16", 9,
      "gemv_gatherx dt=bf16 v=12 tok=4 perm=0 reslds=0 outl=0 groups=1", v=12, k=256, bias=1, dist='ref-test'),
    R(260, 72, "bf16", 1,
      "gemv_gatherx dt=bf16 v=12 tok=1 perm=1 reslds=0 outl=0 groups=1", v=12, k=256, perm=1),
    R(260, 72, "bf16", 2,
      "gemv_gatherx dt=bf16 v=12 tok=2 perm=1 reslds=0 outl=0 groups=1", v=12, k=256, perm=1, bias=1, norm=0, x="planted"),
    R(260, 72, "bf16", 3,
      "gemv_gatherx dt=bf16 v=12 tok=4 perm=1 reslds=0 outl=0 groups=1", v=12, k=256, perm=1, dist='ref-test'),
    R(260, 72, "bf16", 2,
      "gemv_gatherx dt=bf16 v=16 tok=2 perm=1 reslds=0 outl=0 groups=1", v=16, k=256, perm=1, bias=1),
    R(260, 72, "bf16", 3,
      "gemv_gatherx dt=bf16 v=16 tok=4 perm=1 reslds=0 outl=0 groups=1", v=16, k=256, perm=1),
    R(260, 72, "f16", 1,
      "gemv_gatherx dt=f16 v=2 tok=1 perm=0 reslds=0 outl=0 groups=1", v=2, k=256),
    R(260, 72, "f16", 2,
      "gemv_gatherx dt=f16 v=2 tok=2 perm=0 reslds=0 outl=0 groups=1", v=2, k=256, bias=1),
    R(260, 72, "f16", 3,
      "gemv_gatherx dt=f16 v=2 tok=4 perm=0 reslds=0 outl=0 groups=1", v=2, k=256, x="planted"),
    R(260, 72, "f16", 7,
      "gemv_gatherx dt=f16 v=2 tok=8 perm=0 reslds=0 outl=0 groups=1", v=2, k=256, norm=0),
    R(260, 72, "f16", 1,
      "gemv_gatherx dt=f16 v=2 tok=1 perm=1 reslds=0 outl=0 groups=1", v=2, k=256, perm=1, bias=1),
    R(260, 72, "f16", 2,
      "gemv_gatherx dt=f16 v=2 tok=2 perm=1 reslds=0 outl=0 groups=1", v=2, k=256, perm=1, x="planted"),
    R(260, 72, "f16", 3,
      "gemv_gatherx dt=f16 v=2 tok=4 perm=1 reslds=0 outl=0 groups=1", v=2, k=256, perm=1, bias=1),
    R(260, 72, "f16", 5,
      "gemv_gatherx dt=f16 v=2 tok=8 perm=1 reslds=0 outl=0 groups=1", v=2, k=256, perm=1, bias=1),
    R(528, 98, "f16", 1,
      "gemv_gatherx dt=f16 v=2 tok=1 perm=0 reslds=1 outl=same groups=1", v=2, k=32768, kr=16, S=8, ov=2),
    R(260, 72, "f16", 2,
      "gemv_gatherx dt=f16 v=4 tok=2 perm=0 reslds=0 outl=0 groups=1", v=4, k=256, bias=1),
    R(260, 72, "f16", 3,
      "gemv_gatherx dt=f16 v=4 tok=4 perm=0 reslds=0 outl=0 groups=1", v=4, k=256, dist='ref-test'),
    R(260, 72, "f16", 2,
      "gemv_gatherx dt=f16 v=4 tok=2 perm=1 reslds=0 outl=0 groups=1", v=4, k=256, perm=1, dist='ref-test'),
    R(260, 72, "f16", 3,
      "gemv_gatherx dt=f16 v=4 tok=4 perm=1 reslds=0 outl=0 groups=1", v=4, k=256, perm=1, bias=1),
    R(260, 72, "f16", 5,
      "gemv_gatherx dt=f16 v=4 tok=8 perm=1 reslds=0 outl=0 groups=1", v=4, k=256, perm=1, bias=1),
    R(260, 72, "f16", 1,
      "gemv_gatherx dt=f16 v=4 tok=1 perm=1 reslds=1 outl=0 groups=1", v=4, k=256, kr=16, perm=1, bias=1, dist='ref-test'),
    R(528, 98, "f16", 1,
      "gemv_gatherx dt=f16 v=4 tok=1 perm=0 reslds=1 outl=same groups=1", v=4, k=32768, kr=16, S=8, ov=4),
    R(260, 72, "f16", 2,
      "gemv_gatherx dt=f16 v=6 tok=2 perm=0 reslds=0 outl=0 groups=1", v=6, k=256, bias=1),
    R(260, 72, "f16", 3,
      "gemv_gatherx dt=f16 v=6 tok=4 perm=0 reslds=0 outl=0 groups=1", v=6, k=256, norm=0),
    R(260, 72, "f16", 9,
      "gemv_gatherx dt=f16 v=6 tok=8 perm=0 reslds=0 outl=0 groups=1", v=6, k=256),
    R(260, 72, "f16", 1,
      "gemv_gatherx dt=f16 v=6 tok=1 perm=1 reslds=0 outl=0 groups=1", v=6, k=256, perm=1, bias=1),
    R(260, 72, "f16", 2,
      "gemv_gatherx dt=f16 v=6 tok=2 perm=1 reslds=0 outl=0 groups=1", v=6, k=256, perm=1, norm=0),
    R(260, 72, "f16", 3,
      "gemv_gatherx dt=f16 v=6 tok=4 perm=1 reslds=0 outl=0 groups=1", v=6, k=256, perm=1, bias=1),
    R(260, 72, "f16", 5,
      "gemv_gatherx dt=f16 v=6 tok=8 perm=1 reslds=0 outl=0 groups=1", v=6, k=256, perm=1, bias=1, dist='ref-test'),
    R(528, 98, "f16", 1,
      "gemv_gatherx dt=f16 v=6 tok=1 perm=0 reslds=1 outl=same groups=1", v=6, k=32768, kr=16, S=8, ov=6),
    R(260, 72, "f16", 3,
      "gemv_gatherx dt=f16 v=8 tok=4 perm=0 reslds=0 outl=0 groups=1", k=256),
    R(260, 72, "f16", 5,
      "gemv_gatherx dt=f16 v=8 tok=8 perm=0 reslds=0 outl=0 groups=1", k=256),
    R(260, 72, "f16", 1,
      "gemv_gatherx dt=f16 v=8 tok=1 perm=1 reslds=0 outl=0 groups=1", k=256, perm=1, bias=1),
    R(260, 72, "f16", 2,
      "gemv_gatherx dt=f16 v=8 tok=2 perm=1 reslds=0 outl=0 groups=1", k=256, perm=1),
    R(260, 72, "f16", 5,
      "gemv_gatherx dt=f16 v=8 tok=8 perm=1 reslds=0 outl=0 groups=1", k=256, perm=1, bias=1),
    R(260, 72, "f16", 2,
      "gemv_gatherx dt=f16 v=10 tok=2 perm=0 reslds=0 outl=0 groups=1", v=10, k=256, bias=1, dist='ref-test'),
    R(260, 72, "f16", 5,
      "gemv_gatherx dt=f16 v=10 tok=4 perm=0 reslds=0 outl=0 groups=1", v=10, k=256),
    R(260, 72, "f16", 1,
      "gemv_gatherx dt=f16 v=10 tok=1 perm=1 reslds=0 outl=0 groups=1", v=10, k=256, perm=1, bias=1, dist='ref-test'),
    R(260, 72, "f16", 2,
      "gemv_gatherx dt=f16 v=10 tok=2 perm=1 reslds=0 outl=0 groups=1", v=10, k=256, perm=1),
    R(260, 72, "f16", 7,
      "gemv_gatherx dt=f16 v=10 tok=4 perm=1 reslds=0 outl=0 groups=1", v=10, k=256, perm=1, bias=1),
    R(528, 98, "f16", 1,
      "gemv_gatherx dt=f16 v=10 tok=1 perm=0 reslds=1 outl=same groups=1", v=10, k=32768, kr=16, norm=0, S=8, ov=10, dist='ref-test', x="planted"),
    R(260, 72, "f16", 2,
      "gemv_gatherx dt=f16 v=12 tok=2 perm=0 reslds=0 outl=0 groups=1", v=12, k=256, bias=1),
    R(260, 72, "f16", 2,
      "gemv_gatherx dt=f16 v=12 tok=2 perm=1 reslds=0 outl=0 groups=1", v=12, k=256, perm=1),
    R(260, 72, "f16", 1,
      "gemv_gatherx dt=f16 v=12 tok=1 perm=0 reslds=1 outl=0 groups=1", v=12, k=256, kr=16),
    R(260, 72, "f16", 1,
      "gemv_gatherx dt=f16 v=16 tok=1 perm=0 reslds=0 outl=0 groups=1", v=16, k=256, dist='ref-test'),
    R(260, 72, "f16", 1,
      "gemv_gatherx dt=f16 v=16 tok=1 perm=1 reslds=0 outl=0 groups=1", v=16, k=256, perm=1, bias=1),
    R(260, 72, "f16", 2,
      "gemv_gatherx dt=f16 v=16 tok=2 perm=1 reslds=0 outl=0 groups=1", v=16, k=256, perm=1),
    R(264, 100, "bf16", 1,
      "gemv_generic dt=bf16 v=2 tok=1", v=2, k=256, kr=256, norm=0, flags=GENERIC),
    R(264, 100, "bf16", 2,
      "gemv_generic dt=bf16 v=2 tok=2", v=2, k=256, kr=256, bias=1, flags=GENERIC),
    R(264, 100, "bf16", 3,
      "gemv_generic dt=bf16 v=2 tok=4", v=2, k=256, kr=256, flags=GENERIC, x="planted"),
    R(264, 100, "bf16", 5,
      "gemv_generic dt=bf16 v=2 tok=8", v=2, k=256, kr=256, flags=GENERIC),
    R(264, 100, "bf16", 1,
      "gemv_generic dt=bf16 v=4 tok=1", v=4, k=256, kr=256, flags=GENERIC, x="planted"),
    R(264, 100, "bf16", 2,
      "gemv_generic dt=bf16 v=4 tok=2", v=4, k=256, kr=256, bias=1, flags=GENERIC, dist='ref-test'),
    R(264, 100, "bf16", 3,
      "gemv_generic dt=bf16 v=4 tok=4", v=4, k=256, kr=256, flags=GENERIC),
    R(264, 100, "bf16", 5,
      "gemv_generic dt=bf16 v=4 tok=8", v=4, k=256, kr=256, flags=GENERIC),
    R(264, 100, "bf16", 1,
      "gemv_generic dt=bf16 v=6 tok=1", v=6, k=256, kr=256, flags=GENERIC),
    R(264, 100, "bf16", 3,
      "gemv_generic dt=bf16 v=6 tok=4", v=6, k=256, kr=256, flags=GENERIC),
    R(264, 100, "bf16", 5,
      "gemv_generic dt=bf16 v=6 tok=8", v=6, k=256, kr=256, flags=GENERIC, dist='ref-test'),
    R(264, 100, "bf16", 1,
      "gemv_generic dt=bf16 v=8 tok=1", k=256, kr=256, flags=GENERIC),
    R(264, 100, "bf16", 2,
      "gemv_generic dt=bf16 v=8 tok=2", k=256, kr=256, bias=1, norm=0, flags=GENERIC),
    R(264, 100, "bf16", 3,
      "gemv_generic dt=bf16 v=8 tok=4", k=256, kr=256, flags=GENERIC, dist='ref-test'),
    R(264, 100, "bf16", 5,
      "gemv_generic dt=bf16 v=8 tok=8", k=256, kr=256, flags=GENERIC),
    R(264, 100, "bf16", 1,
      "gemv_generic dt=bf16 v=10 tok=1", v=10, k=256, kr=256, flags=GENERIC, dist='ref-test'),
    R(264, 100, "bf16", 2,
      "gemv_generic dt=bf16 v=10 tok=2", v=10, k=256, kr=256, bias=1, flags=GENERIC),
    R(264, 100, "bf16", 3,
      "gemv_generic dt=bf16 v=10 tok=4", v=10, k=256, kr=256, flags=GENERIC),
    R(264, 100, "bf16", 5,
      "gemv_generic dt=bf16 v=10 tok=8", v=10, k=256, kr=256, flags=GENERIC),
    R(264, 100, "bf16", 1,
      "gemv_generic dt=bf16 v=12 tok=1", v=12, k=256, kr=256, flags=GENERIC),
    R(264, 100, "bf16", 2,
      "gemv_generic dt=bf16 v=12 tok=2", v=12, k=256, kr=256, bias=1, flags=GENERIC),
    R(264, 100, "bf16", 3,
      "gemv_generic dt=bf16 v=12 tok=4", v=12, k=256, kr=256, flags=GENERIC),
    R(264, 100, "bf16", 1,
      "gemv_generic dt=bf16 v=16 tok=1", v=16, k=256, kr=256, norm=0, flags=GENERIC),
    R(264, 100, "bf16", 2,
      "gemv_generic dt=bf16 v=16 tok=2", v=16, k=256, kr=256, bias=1, flags=GENERIC),
    R(264, 100, "bf16", 3,
      "gemv_generic dt=bf16 v=16 tok=4", v=16, k=256, kr=256, flags=GENERIC),
    R(264, 100, "bf16", 5,
      "gemv_generic dt=bf16 v=16 tok=8", v=16, k=256, kr=256, flags=GENERIC, dist='ref-test'),
    R(264, 100, "f16", 2,
      "gemv_generic dt=f16 v=2 tok=2", v=2, k=256, kr=256, norm=0, flags=GENERIC),
    R(264, 100, "f16", 4,
      "gemv_generic dt=f16 v=2 tok=4", v=2, k=256, kr=256, flags=GENERIC, x="planted"),
    R(264, 100, "f16", 5,
      "gemv_generic dt=f16 v=2 tok=8", v=2, k=256, kr=256, bias=1, flags=GENERIC, dist='ref-test'),
    R(264, 100, "f16", 1,
      "gemv_generic dt=f16 v=4 tok=1", v=4, k=256, kr=256, bias=1, flags=GENERIC),
    R(264, 100, "f16", 2,
      "gemv_generic dt=f16 v=4 tok=2", v=4, k=256, kr=256, flags=GENERIC, x="planted"),
    R(264, 100, "f16", 3,
      "gemv_generic dt=f16 v=4 tok=4", v=4, k=256, kr=256, bias=1, flags=GENERIC, dist='ref-test'),
    R(264, 100, "f16", 6,
      "gemv_generic dt=f16 v=4 tok=8", v=4, k=256, kr=256, flags=GENERIC),
    R(264, 100, "f16", 1,
      "gemv_generic dt=f16 v=6 tok=1", v=6, k=256, kr=256, bias=1, flags=GENERIC, dist='ref-test'),
    R(264, 100, "f16", 2,
      "gemv_generic dt=f16 v=6 tok=2", v=6, k=256, kr=256, flags=GENERIC),
    R(264, 100, "f16", 3,
      "gemv_generic dt=f16 v=6 tok=4", v=6, k=256, kr=256, bias=1, flags=GENERIC),
    R(264, 100, "f16", 7,
      "gemv_generic dt=f16 v=6 tok=8", v=6, k=256, kr=256, bias=1, flags=GENERIC),
    R(264, 100, "f16", 2,
      "gemv_generic dt=f16 v=8 tok=2", k=256, kr=256, flags=GENERIC),
    R(264, 100, "f16", 3,
      "gemv_generic dt=f16 v=8 tok=4", k=256, kr=256, bias=1, norm=0, flags=GENERIC),
    R(264, 100, "f16", 1,
      "gemv_generic dt=f16 v=10 tok=1", v=10, k=256, kr=256, bias=1, norm=0, flags=GENERIC),
    R(264, 100, "f16", 2,
      "gemv_generic dt=f16 v=10 tok=2", v=10, k=256, kr=256, flags=GENERIC, dist='ref-test'),
    R(264, 100, "f16", 8,
      "gemv_generic dt=f16 v=10 tok=8", v=10, k=256, kr=256, norm=0, flags=GENERIC),
    R(264, 100, "f16", 1,
      "gemv_generic dt=f16 v=12 tok=1", v=12, k=256, kr=256, bias=1, flags=GENERIC),
    R(264, 100, "f16", 2,
      "gemv_generic dt=f16 v=12 tok=2", v=12, k=256, kr=256, flags=GENERIC),
    R(264, 100, "f16", 3,
      "gemv_generic dt=f16 v=12 tok=4", v=12, k=256, kr=256, bias=1, flags=GENERIC),
    R(264, 100, "f16", 5,
      "gemv_generic dt=f16 v=12 tok=8", v=12, k=256, kr=256, bias=1, flags=GENERIC, dist='ref-test', x="planted"),
    R(264, 100, "f16", 1,
      "gemv_generic dt=f16 v=16 tok=1", v=16, k=256, kr=256, bias=1, flags=GENERIC, dist='ref-test', x="planted"),
    R(264, 100, "f16", 2,
      "gemv_generic dt=f16 v=16 tok=2", v=16, k=256, kr=256, norm=0, flags=GENERIC),
    R(264, 100, "f16", 3,
      "gemv_generic dt=f16 v=16 tok=4", v=16, k=256, kr=256, bias=1, flags=GENERIC),
    R(264, 100, "f16", 5,
      "gemv_generic dt=f16 v=16 tok=8", v=16, k=256, kr=256, bias=1, flags=GENERIC),
    R(264, 60, "bf16", 1,
      "gemv_lds dt=bf16 fmt=12 tok=1 rw=1 dma=1 perm=0", bias=1),
    R(264, 60, "bf16", 6,
      "gemv_lds dt=bf16 fmt=12 tok=2 rw=1 dma=1 perm=0"),
    R(264, 60, "bf16", 9,
      "gemv_lds dt=bf16 fmt=12 tok=2 rw=1 dma=1 perm=0", bias=1, dist='ref-test'),
    R(264, 60, "bf16", 10,
      "gemv_lds dt=bf16 fmt=12 tok=2 rw=1 dma=1 perm=0"),
    R(264, 60, "bf16", 1,
      "gemv_lds dt=bf16 fmt=20 tok=1 rw=1 dma=1 perm=0", kr=256, bias=1),
    R(264, 60, "bf16", 7,
      "gemv_lds dt=bf16 fmt=21 tok=2 rw=1 dma=1 perm=0", kr=512, bias=1, dist='ref-test'),
    R(264, 60, "bf16", 1,
      "gemv_lds dt=bf16 fmt=13 tok=1 rw=1 dma=1 perm=0", k=8192, bias=1),
    R(264, 60, "bf16", 1,
      "gemv_lds dt=bf16 fmt=22 tok=1 rw=1 dma=1 perm=0", k=8192, kr=512, bias=1, dist='ref-test'),
    R(264, 60, "bf16", 8,
      "gemv_lds dt=bf16 fmt=22 tok=2 rw=1 dma=1 perm=0", k=8192, kr=512),
    R(264, 60, "f16", 1,
      "gemv_lds dt=f16 fmt=12 tok=1 rw=1 dma=1 perm=0"),
    R(264, 60, "f16", 2,
      "gemv_lds dt=f16 fmt=12 tok=2 rw=1 dma=1 perm=0", bias=1),
    R(264, 4804, "f16", 3,
      "gemv_lds dt=f16 fmt=12 tok=4 rw=2 dma=1 perm=0"),
    R(264, 8806, "f16", 2,
      "gemv_lds dt=f16 fmt=12 tok=2 rw=4 dma=1 perm=0", bias=1),
    R(264, 8806, "f16", 3,
      "gemv_lds dt=f16 fmt=12 tok=4 rw=4 dma=1 perm=0", x="planted"),
    R(264, 16804, "f16", 1,
      "gemv_lds dt=f16 fmt=12 tok=1 rw=8 dma=1 perm=0", flags=EXACT, dist='ref-test'),
    R(264, 16804, "f16", 3,
      "gemv_lds dt=f16 fmt=12 tok=4 rw=8 dma=1 perm=0"),
    R(264, 32804, "f16", 1,
      "gemv_lds dt=f16 fmt=12 tok=1 rw=16 dma=1 perm=0", flags=EXACT, dist='ref-test'),
    R(264, 32804, "f16", 2,
      "gemv_lds dt=f16 fmt=12 tok=2 rw=16 dma=1 perm=0", bias=1),
    R(264, 60, "f16", 2,
      "gemv_lds dt=f16 fmt=20 tok=2 rw=1 dma=1 perm=0", kr=256, bias=1),
    R(264, 60, "f16", 2,
      "gemv_lds dt=f16 fmt=21 tok=2 rw=1 dma=1 perm=0", kr=512, bias=1),
    R(264, 60, "f16", 7,
      "gemv_lds dt=f16 fmt=21 tok=4 rw=1 dma=1 perm=0", kr=512),
    R(264, 60, "f16", 1,
      "gemv_lds dt=f16 fmt=13 tok=1 rw=1 dma=1 perm=0", k=8192),
    R(264, 60, "f16", 2,
      "gemv_lds dt=f16 fmt=13 tok=2 rw=1 dma=1 perm=0", k=8192, bias=1, norm=0),
    R(264, 60, "f16", 6,
      "gemv_lds dt=f16 fmt=13 tok=4 rw=1 dma=1 perm=0", k=8192, bias=1),
    R(264, 60, "f16", 8,
      "gemv_lds dt=f16 fmt=22 tok=4 rw=1 dma=1 perm=0", k=8192, kr=512, bias=1, norm=0),
    R(264, 8806, "bf16", 1,
      "gemv_lds_mfma dt=bf16 fmt=13 rw=4 stages=1 dma=1 perm=0", k=8192, bias=1),
    R(264, 8806, "bf16", 1,
      "gemv_lds_mfma dt=bf16 fmt=22 rw=4 stages=1 dma=1 perm=0", k=8192, kr=512, bias=1),
    R(264, 8806, "f16", 1,
      "gemv_lds_mfma dt=f16 fmt=21 rw=4 stages=1 dma=1 perm=0", kr=512),
    V(264, 64, "bf16", 1,
      "gemv_lds dt=bf16 fmt=v2 tok=1 rw=1 dma=0 perm=0", k=5000),
    V(264, 64, "bf16", 4,
      "gemv_lds dt=bf16 fmt=v2u8 tok=2 rw=1 dma=0 perm=0", k=5000, kr=256, bias=1),
    V(264, 64, "bf16", 1,
      "gemv_lds dt=bf16 fmt=v2u8 tok=1 rw=1 dma=1 perm=0", kr=256, bias=1),
    V(264, 64, "f16", 2,
      "gemv_lds dt=f16 fmt=v2 tok=2 rw=1 dma=1 perm=0", bias=1),
    V(264, 64, "f16", 9,
      "gemv_lds dt=f16 fmt=v2 tok=4 rw=1 dma=1 perm=0"),
    V(264, 64, "f16", 2,
      "gemv_lds dt=f16 fmt=v2u8 tok=2 rw=1 dma=1 perm=0", kr=256, bias=1),
    V(264, 64, "f16", 10,
      "gemv_lds dt=f16 fmt=v2u16 tok=4 rw=1 dma=1 perm=0", kr=256, bias=1, rb=2),
    V(264, 8816, "bf16", 1,
      "gemv_lds_mfma dt=bf16 fmt=v2u8 rw=4 stages=1 dma=0 perm=0", k=5000, kr=256),
    V(264, 8816, "bf16", 1,
      "gemv_lds_mfma dt=bf16 fmt=v2u16 rw=4 stages=1 dma=0 perm=0", k=5000, kr=256, rb=2),
    V(264, 8816, "f16", 1,
      "gemv_lds_mfma dt=f16 fmt=v2 rw=4 stages=1 dma=1 perm=0"),
    V(264, 8816, "f16", 1,
      "gemv_lds_mfma dt=f16 fmt=v2u16 rw=4 stages=1 dma=1 perm=0", kr=256, rb=2),
    V(264, 64, "bf16", 1,
      "gemv_v2 dt=bf16 v=4 tok=1", v=4, bias=1, norm=0),
    V(264, 64, "bf16", 2,
      "gemv_v2 dt=bf16 v=4 tok=2", v=4),
    V(264, 64, "bf16", 3,
      "gemv_v2 dt=bf16 v=4 tok=4", v=4, bias=1, dist='ref-test'),
    V(264, 64, "bf16", 1,
      "gemv_v2 dt=bf16 v=8 tok=1", bias=1, flags=GENERIC),
    V(264, 64, "bf16", 2,
      "gemv_v2 dt=bf16 v=8 tok=2", flags=GENERIC),
    V(264, 64, "bf16", 3,
      "gemv_v2 dt=bf16 v=8 tok=4", bias=1, flags=GENERIC),
    V(264, 64, "bf16", 8,
      "gemv_v2 dt=bf16 v=8 tok=8", flags=GENERIC),
    V(264, 64, "bf16", 1,
      "gemv_v2 dt=bf16 v=16 tok=1", v=16, bias=1, dist='ref-test'),
    V(264, 64, "bf16", 3,
      "gemv_v2 dt=bf16 v=16 tok=4", v=16, bias=1, norm=0),
    V(264, 64, "f16", 1,
      "gemv_v2 dt=f16 v=4 tok=1", v=4),
    V(264, 64, "f16", 2,
      "gemv_v2 dt=f16 v=4 tok=2", v=4, bias=1, norm=0),
    V(264, 64, "f16", 5,
      "gemv_v2 dt=f16 v=4 tok=8", v=4),
    V(264, 64, "f16", 10,
      "gemv_v2 dt=f16 v=4 tok=8", v=4, bias=1, x="planted"),
    V(264, 64, "f16", 2,
      "gemv_v2 dt=f16 v=8 tok=2", bias=1, flags=GENERIC),
    V(264, 64, "f16", 6,
      "gemv_v2 dt=f16 v=8 tok=8", bias=1, flags=GENERIC, x="planted"),
    V(264, 64, "f16", 1,
      "gemv_v2 dt=f16 v=16 tok=1", v=16),
    V(264, 64, "f16", 2,
      "gemv_v2 dt=f16 v=16 tok=2", v=16, bias=1, dist='ref-test'),
    V(264, 64, "f16", 4,
      "gemv_v2 dt=f16 v=16 tok=4", v=16, bias=1, norm=0),
]

ALL_ROWS = EDGES + BIG + ROWS


# ---------------------------------------------------------------------------------------------- the rows' layers and inputs
def layer_of(e):
    """the oracle layer of a packed row (seeded by its shape)"""
    kw = dict(vector_len=e["v"], num_centroids=e["k"], num_res_centroids=e["kr"], num_codebooks=e["C"], enable_perm=bool(e["perm"]),
              bias=bool(e["bias"]), enable_norm=bool(e["norm"]))
    if e["S"]:
        kw.update(outlier_size=e["S"], outlier_vector_len=e["ov"], num_outlier_centroids=256)
    return vo.make_layer(e["I"], e["O"], dist=e["dist"], seed=e["I"] + e["O"] + e["k"] + e["kr"], dtype=e["dt"], **kw)


def v2_tensors(e):
    """the v2 tensors of a v2 row as uint16 bit patterns / integer ids (numpy): RANDOM ids over the whole codebooks"""
    rng = np.random.default_rng(e["I"] + e["O"] + e["k"] + e["kr"])
    I, O, v, k, kr, dt = e["I"], e["O"], e["v"], e["k"], e["kr"], e["dt"]
    p = dict(c=(0.02, 0.5), r=(0.02, 0.5), s=(0.02, 0.5), b=(0.02, 0.5), o=0.5) if e["dist"] == "ref-test" else \
        dict(c=(0.0, 0.02), r=(0.0, 0.005), s=(1.0, 0.1), b=(0.0, 0.01), o=0.02)
    nrm = lambda shape, ms: vo.from_f32((rng.standard_normal(shape) * ms[1] + ms[0]).astype(np.float32), dt)   # noqa: E731
    n = I * (O // v)
    t = dict(I=I, O=O, v=v, k=k, kr=kr, ids=rng.integers(0, k, n).astype(np.uint16), cent=nrm((1, k, v), p["c"]))
    if kr:
        t["rids"] = rng.integers(0, kr, n).astype(np.uint8 if e["rb"] == 1 else np.uint16)
        t["rcent"] = nrm((1, kr, v), p["r"])
    if e["norm"]:
        t["scale"], t["sbias"] = nrm((I, 1), p["s"]), nrm((I, 1), p["b"])
    if e["bias"]:
        t["bias"] = nrm((1, O), (0.0, p["o"]))
    return t


def v2_pieces(e, t):
    return am.pieces_v2(e["dt"], e["I"], e["O"], e["v"], t["ids"], t["cent"], t.get("rids"), t.get("rcent"), t.get("scale"), t.get("sbias"),
                        t.get("bias"))


def x_of(e, perm=None):
    """the row's activation: dense, or planted (2 - 4 columns of magnitude 60 among ordinary ones)"""
    kind = _dense if e["x"] == "dense" else _planted
    kw = dict(perm=perm) if e["x"] == "planted" else {}
    return kind(e["I"], e["tokens"], e["dt"], e["I"] + e["tokens"], **kw)


def instance_of(desc, tokens, flags):
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(1024)
    B.check(B.lib().vptq_quant_gemv_instance(desc, tokens, flags, buf, len(buf)), "vptq_quant_gemv_instance")
    return buf.value.decode()


def v2_instance_of(desc, tokens, flags):
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(1024)
    B.check(B.lib().vptq_quant_gemv_v2_instance(desc, tokens, flags, buf, len(buf)), "vptq_quant_gemv_v2_instance")
    return buf.value.decode()


def _check_big(y16, y32, L, x, e, what):
    """the model in row blocks of at most am.MAX_WEIGHTS weights: every output, block by block"""
    T = e["tokens"]
    y16, y32 = y16.reshape(T, -1), y32.reshape(T, -1)
    kw = dict(rounded=e.get("rounded", False), round_sx=e.get("round_sx", True))
    for (o0, o1), mm, aa in am.model_blocks(L, x, e["arith"], **kw):
        am.check_outputs(y16[:, o0:o1], mm, aa, L.dtype, False, what=f"{what} outputs {o0} - {o1} [16-bit]")
        am.check_outputs(y32[:, o0:o1], mm, aa, L.dtype, True, what=f"{what} outputs {o0} - {o1} [fp32]")


@pytest.mark.parametrize("e", ALL_ROWS)
def test_other_instance_vs_its_model(e, dev):
    route = e["instance"].split()[0] + "_kernel"
    if e["entry"] == "v2":
        t = v2_tensors(e)
        dt = e["dt"]
        td = {key: (val if not isinstance(val, np.ndarray) else
                    bits_to_tensor(val, dt, dev).reshape(val.shape) if key in ("cent", "rcent", "scale", "sbias", "bias") else
                    torch.from_numpy(val.view(np.int16) if val.dtype == np.uint16 else val).to(dev)) for key, val in t.items()}
        desc, keep = v2_desc(td, dt)
        assert v2_instance_of(desc, e["tokens"], e["flags"]) == e["instance"]
        x, hot = x_of(e)
        xt = bits_to_tensor(x, dt, dev).reshape(x.shape)
        y16 = _np(gemv_v2_abi_nan(desc, xt, e["O"], e["flags"]))
        y32 = _np(gemv_v2_abi_nan(desc, xt, e["O"], e["flags"], out_f32=True))
        shim = types.SimpleNamespace(in_features=e["I"], perm=None, dtype=dt)
        _check(y16, y32, shim, x, e, hot, P=v2_pieces(e, t), what=e["instance"])
        return
    L = layer_of(e)
    m = spec_to_module(L, dev)
    assert kernel_name(m, e["tokens"], e["flags"]) == route
    assert instance_of(module_desc(m)[0], e["tokens"], e["flags"]) == e["instance"]
    x, hot = x_of(e, L.perm)
    xt = bits_to_tensor(x, L.dtype, dev).reshape(x.shape)
    y16 = _np(gemv_abi_nan(m, xt, e["flags"]))
    y32 = _np(gemv_abi_nan(m, xt, e["flags"], out_f32=True))
    if e["big"]:
        _check_big(y16, y32, L, x, e, e["instance"])
    else:
        _check(y16, y32, L, x, e, hot, what=e["instance"])
