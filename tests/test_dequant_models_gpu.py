"""vptq_dequant (vptq_amd/csrc/dequant.hip) - the kernel the sliced, compact and GEMM tests use as their bit-level partner and every
exact GEMV kernel documents its weights against - held to the oracle at EVERY INSTANTIATION of dequant_kernel<DT, V, TAB> and on every
path a thread can take to its 8 index elements, as tests/test_route_models_other_gpu.py does for the GEMV families.  Each row names
the line vptq_dequant_instance must give for its layer (the launch decision and the kernel's own path predicates, evaluated by the
library), then the dense W the launch writes is compared with vo.dequant(L, ref_residual_mask_quirk=False) BIT FOR BIT - there is no
tolerance anywhere, the reference is exact.  W is a region inside a larger buffer filled with a sentinel: 8 guard rows in front of
row 0 and 8 behind row O - 1 must come back untouched.

The mechanisms live in the columns and in the format, so the layers are at most 77 rows of at most 2056 columns; O = 5 v - 3 leaves the
last vector-row ragged at every vector length.  The instance strings below were printed by the library for these layers and read
against dequant_paths.h; tests/test_instance_census_cpu.py enumerates what the library can answer and fails when a cell has no row.

SPECIAL rows carry the hand-written tables of tests/_dequant_specials.py instead of random draws (signed zeros, subnormals, the
largest finite value, infinities, NaN, ties, overflow, underflow); tests/test_dequant_specials_cpu.py pins the oracle's result on them
against torch's CPU arithmetic.  NaN is compared by position, everything else by bits.

What the GEMV kernels do with special values is not covered here: their arithmetic on such weights is a later issue."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import vptq_oracle as vo
from vptq_amd import _backend as B
from _gpu_util import spec_to_module, module_desc
import _dequant_specials as sp

pytestmark = pytest.mark.gpu

GUARD_ROWS = 8        # (8 rows of I elements: 16 I bytes - the region keeps the buffer's 16-byte alignment)
SENTINEL = 0x5a5a


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    B.lib()
    return torch.device("cuda", 0)


def D(I, O, dt, instance, v=8, k=256, kr=256, C=1, perm=0, S=0, ov=0, norm=1, w_off=0, norm_off=0, idx_off=0, special=0):
    """a layer through vptq_dequant: I columns (S outlier columns of an ov-long codebook + C groups), O rows; w_off / norm_off /
    idx_off: W, weight_scale and weight_bias, indices that many bytes past a 16-byte boundary; special: the hand-written tables"""
    e = dict(I=I, O=O, dt=dt, instance=instance, v=v, k=k, kr=kr, C=C, perm=perm, S=S, ov=ov, norm=norm, w_off=w_off, norm_off=norm_off,
             idx_off=idx_off, special=special)
    return pytest.param(e, id=f"{dt}-{I}x{O}-v{v}k{k}r{kr}c{C}-p{perm}s{S}o{ov}n{norm}-w{w_off}n{norm_off}i{idx_off}" + ("-special" if special else ""))


# ROWS-BEGIN (tools/gen_dequant_rows.py)
ROWS = [
    D(264, 7, "f16",
      "dequant dt=f16 v=2 tab=1 lds=2048 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=2),   # TAB 1
    D(264, 7, "f16",
      "dequant dt=f16 v=2 tab=2 lds=1024 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=2, k=65536),   # TAB 2
    D(264, 7, "f16",
      "dequant dt=f16 v=2 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=2, k=65536, kr=0),   # TAB 0
    D(264, 17, "f16",
      "dequant dt=f16 v=4 tab=1 lds=4096 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=4),   # TAB 1
    D(264, 17, "f16",
      "dequant dt=f16 v=4 tab=2 lds=2048 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=4, k=65536),   # TAB 2
    D(264, 17, "f16",
      "dequant dt=f16 v=4 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=4, k=65536, kr=0),   # TAB 0
    D(264, 27, "f16",
      "dequant dt=f16 v=6 tab=1 lds=6144 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=6),   # TAB 1
    D(264, 27, "f16",
      "dequant dt=f16 v=6 tab=2 lds=3072 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=6, k=65536),   # TAB 2
    D(264, 27, "f16",
      "dequant dt=f16 v=6 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=6, k=65536, kr=0),   # TAB 0
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=8192 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0"),   # TAB 1
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536),   # TAB 2
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0),   # TAB 0
    D(264, 47, "f16",
      "dequant dt=f16 v=10 tab=1 lds=10240 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=10),   # TAB 1
    D(264, 47, "f16",
      "dequant dt=f16 v=10 tab=2 lds=5120 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=10, k=65536),   # TAB 2
    D(264, 47, "f16",
      "dequant dt=f16 v=10 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=10, k=65536, kr=0),   # TAB 0
    D(264, 57, "f16",
      "dequant dt=f16 v=12 tab=1 lds=12288 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=12),   # TAB 1
    D(264, 57, "f16",
      "dequant dt=f16 v=12 tab=2 lds=6144 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=12, k=65536),   # TAB 2
    D(264, 57, "f16",
      "dequant dt=f16 v=12 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=12, k=65536, kr=0),   # TAB 0
    D(264, 77, "f16",
      "dequant dt=f16 v=16 tab=1 lds=16384 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=16),   # TAB 1: 16384 bytes, the limit itself
    D(264, 77, "f16",
      "dequant dt=f16 v=16 tab=2 lds=8192 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=16, k=65536),   # TAB 2
    D(264, 77, "f16",
      "dequant dt=f16 v=16 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=16, k=65536, kr=0),   # TAB 0
    D(264, 7, "bf16",
      "dequant dt=bf16 v=2 tab=1 lds=2048 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=2),   # TAB 1
    D(264, 7, "bf16",
      "dequant dt=bf16 v=2 tab=2 lds=1024 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=2, k=65536),   # TAB 2
    D(264, 7, "bf16",
      "dequant dt=bf16 v=2 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=2, k=65536, kr=0),   # TAB 0
    D(264, 17, "bf16",
      "dequant dt=bf16 v=4 tab=1 lds=4096 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=4),   # TAB 1
    D(264, 17, "bf16",
      "dequant dt=bf16 v=4 tab=2 lds=2048 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=4, k=65536),   # TAB 2
    D(264, 17, "bf16",
      "dequant dt=bf16 v=4 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=4, k=65536, kr=0),   # TAB 0
    D(264, 27, "bf16",
      "dequant dt=bf16 v=6 tab=1 lds=6144 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=6),   # TAB 1
    D(264, 27, "bf16",
      "dequant dt=bf16 v=6 tab=2 lds=3072 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=6, k=65536),   # TAB 2
    D(264, 27, "bf16",
      "dequant dt=bf16 v=6 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=6, k=65536, kr=0),   # TAB 0
    D(264, 37, "bf16",
      "dequant dt=bf16 v=8 tab=1 lds=8192 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0"),   # TAB 1
    D(264, 37, "bf16",
      "dequant dt=bf16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536),   # TAB 2
    D(264, 37, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0),   # TAB 0
    D(264, 47, "bf16",
      "dequant dt=bf16 v=10 tab=1 lds=10240 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=10),   # TAB 1
    D(264, 47, "bf16",
      "dequant dt=bf16 v=10 tab=2 lds=5120 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=10, k=65536),   # TAB 2
    D(264, 47, "bf16",
      "dequant dt=bf16 v=10 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=10, k=65536, kr=0),   # TAB 0
    D(264, 57, "bf16",
      "dequant dt=bf16 v=12 tab=1 lds=12288 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=12),   # TAB 1
    D(264, 57, "bf16",
      "dequant dt=bf16 v=12 tab=2 lds=6144 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=12, k=65536),   # TAB 2
    D(264, 57, "bf16",
      "dequant dt=bf16 v=12 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=12, k=65536, kr=0),   # TAB 0
    D(264, 77, "bf16",
      "dequant dt=bf16 v=16 tab=1 lds=16384 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=16),   # TAB 1: 16384 bytes, the limit itself
    D(264, 77, "bf16",
      "dequant dt=bf16 v=16 tab=2 lds=8192 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=16, k=65536),   # TAB 2
    D(264, 77, "bf16",
      "dequant dt=bf16 v=16 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", v=16, k=65536, kr=0),   # TAB 0
    D(264, 77, "f16",
      "dequant dt=f16 v=16 tab=2 lds=8192 colblocks=1 t=17 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=16, k=512),   # one step above the limit of both tables: TAB 2
    D(264, 77, "f16",
      "dequant dt=f16 v=16 tab=2 lds=16384 colblocks=1 t=25 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=16, k=65536, kr=512),   # TAB 2 at its limit
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=16384 colblocks=1 t=26 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=1024),   # TAB 2 at its limit, v = 8
    D(264, 77, "f16",
      "dequant dt=f16 v=16 tab=0 lds=0 colblocks=1 t=26 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=16, k=65536, kr=1024),   # one step above: TAB 0
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=4096 colblocks=1 t=8 norm=vec store=vec idx=win:31,elem:2 perm=0 outl=0 groups=1 ragged=0", kr=0),   # TAB 1 with an empty residual part
    D(272, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:34 perm=0 outl=0 groups=2 ragged=0", C=2),   # two codebook groups whose tables would fit: TAB 0
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=32 colblocks=1 t=1 norm=vec store=vec idx=win:20,elem:13 perm=0 outl=0 groups=1 ragged=0", k=2, kr=0),   # T = 1
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=64 colblocks=1 t=2 norm=vec store=vec idx=win:26,elem:7 perm=0 outl=0 groups=1 ragged=0", k=4, kr=0),   # T = 2
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=128 colblocks=1 t=3 norm=vec store=vec idx=win:28,elem:5 perm=0 outl=0 groups=1 ragged=0", k=8, kr=0),   # T = 3
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=256 colblocks=1 t=4 norm=vec store=vec idx=win:29,elem:4 perm=0 outl=0 groups=1 ragged=0", k=16, kr=0),   # T = 4
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=512 colblocks=1 t=5 norm=vec store=vec idx=win:30,elem:3 perm=0 outl=0 groups=1 ragged=0", k=32, kr=0),   # T = 5
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=1024 colblocks=1 t=6 norm=vec store=vec idx=win:31,elem:2 perm=0 outl=0 groups=1 ragged=0", k=64, kr=0),   # T = 6
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=2048 colblocks=1 t=7 norm=vec store=vec idx=win:31,elem:2 perm=0 outl=0 groups=1 ragged=0", k=128, kr=0),   # T = 7
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=4096 colblocks=1 t=8 norm=vec store=vec idx=win:31,elem:2 perm=0 outl=0 groups=1 ragged=0", kr=0),   # T = 8
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=8192 colblocks=1 t=9 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=512, kr=0),   # T = 9
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=16384 colblocks=1 t=10 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=1024, kr=0),   # T = 10
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=11 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=2048, kr=0),   # T = 11
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=12 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=4096, kr=0),   # T = 12
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=13 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=8192, kr=0),   # T = 13
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=14 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=16384, kr=0),   # T = 14
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=15 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=32768, kr=0),   # T = 15
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0),   # T = 16
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=32 colblocks=1 t=17 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=2),   # T = 17
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=64 colblocks=1 t=18 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=4),   # T = 18
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=128 colblocks=1 t=19 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=8),   # T = 19
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=256 colblocks=1 t=20 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=16),   # T = 20
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=512 colblocks=1 t=21 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=32),   # T = 21
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=1024 colblocks=1 t=22 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=64),   # T = 22
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=2048 colblocks=1 t=23 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=128),   # T = 23
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536),   # T = 24
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=8192 colblocks=1 t=25 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=512),   # T = 25
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=16384 colblocks=1 t=26 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=1024),   # T = 26
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=27 norm=vec store=vec idx=win5:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=2048),   # T = 27
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=28 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=4096),   # T = 28
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=29 norm=vec store=vec idx=win5:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=8192),   # T = 29
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=30 norm=vec store=vec idx=win5:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=16384),   # T = 30
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=31 norm=vec store=vec idx=win5:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=32768),   # T = 31
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=32 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=65536),   # T = 32
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=22 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", kr=16384),   # res_bits > index_bits
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=20 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=512, kr=2048),   # res_bits > index_bits
    D(264, 37, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=27 norm=vec store=vec idx=win5:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=2048),   # T = 27: the fifth word, bf16
    D(264, 77, "f16",
      "dequant dt=f16 v=16 tab=0 lds=0 colblocks=1 t=27 norm=vec store=vec idx=win5:32,elem:1 perm=0 outl=0 groups=1 ragged=0", v=16, k=65536, kr=2048),   # T = 27: the fifth word, v = 16
    D(2056, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=2 t=27 norm=vec store=vec idx=win5:256,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=2048),   # T = 27: the fifth word, a second column block
    D(264, 37, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=29 norm=vec store=vec idx=win5:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=8192),   # T = 29: the fifth word, bf16
    D(264, 77, "f16",
      "dequant dt=f16 v=16 tab=0 lds=0 colblocks=1 t=29 norm=vec store=vec idx=win5:33 perm=0 outl=0 groups=1 ragged=0", v=16, k=65536, kr=8192),   # T = 29: the fifth word, v = 16
    D(2056, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=2 t=29 norm=vec store=vec idx=win5:257 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=8192),   # T = 29: the fifth word, a second column block
    D(264, 37, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=30 norm=vec store=vec idx=win5:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=16384),   # T = 30: the fifth word, bf16
    D(264, 77, "f16",
      "dequant dt=f16 v=16 tab=0 lds=0 colblocks=1 t=30 norm=vec store=vec idx=win5:33 perm=0 outl=0 groups=1 ragged=0", v=16, k=65536, kr=16384),   # T = 30: the fifth word, v = 16
    D(2056, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=2 t=30 norm=vec store=vec idx=win5:257 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=16384),   # T = 30: the fifth word, a second column block
    D(264, 37, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=31 norm=vec store=vec idx=win5:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=32768),   # T = 31: the fifth word, bf16
    D(264, 77, "f16",
      "dequant dt=f16 v=16 tab=0 lds=0 colblocks=1 t=31 norm=vec store=vec idx=win5:33 perm=0 outl=0 groups=1 ragged=0", v=16, k=65536, kr=32768),   # T = 31: the fifth word, v = 16
    D(2056, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=2 t=31 norm=vec store=vec idx=win5:257 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=32768),   # T = 31: the fifth word, a second column block
    D(8, 29, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0),   # one chunk, the window would pass the row end
    D(2040, 29, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:255 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0),   # one column block, not full
    D(2048, 29, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:256 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0),   # exactly one column block
    D(2056, 29, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=2 t=16 norm=vec store=vec idx=vec:257 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0),   # a second column block with one live thread
    D(1001, 29, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=scalar store=scalar idx=elem:126 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=0),   # I % 8 != 0: all elem, scalar stores, clamped last column
    D(7, 29, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=0),   # less than one chunk
    D(2056, 29, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=2 t=16 norm=vec store=vec idx=vec:257 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0),   # a second column block with one live thread
    D(1001, 29, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=scalar store=scalar idx=elem:126 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=0),   # I % 8 != 0: all elem, scalar stores, clamped last column
    D(8, 29, "f16",
      "dequant dt=f16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=vec store=vec idx=elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536),   # one chunk, the window would pass the row end
    D(2040, 29, "f16",
      "dequant dt=f16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=vec store=vec idx=win:254,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536),   # one column block, not full
    D(2048, 29, "f16",
      "dequant dt=f16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=vec store=vec idx=win:255,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536),   # exactly one column block
    D(2056, 29, "f16",
      "dequant dt=f16 v=8 tab=2 lds=4096 colblocks=2 t=24 norm=vec store=vec idx=win:256,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536),   # a second column block with one live thread
    D(1001, 29, "f16",
      "dequant dt=f16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=scalar store=scalar idx=elem:126 perm=0 outl=0 groups=1 ragged=1", k=65536),   # I % 8 != 0: all elem, scalar stores, clamped last column
    D(7, 29, "f16",
      "dequant dt=f16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536),   # less than one chunk
    D(2056, 29, "bf16",
      "dequant dt=bf16 v=8 tab=2 lds=4096 colblocks=2 t=24 norm=vec store=vec idx=win:256,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536),   # a second column block with one live thread
    D(1001, 29, "bf16",
      "dequant dt=bf16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=scalar store=scalar idx=elem:126 perm=0 outl=0 groups=1 ragged=1", k=65536),   # I % 8 != 0: all elem, scalar stores, clamped last column
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=vec store=vec idx=elem:33 perm=1 outl=0 groups=1 ragged=0", k=65536, perm=1),   # a permutation
    D(280, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=vec store=vec idx=elem:35 perm=0 outl=4 groups=1 ragged=0", k=65536, S=12, ov=4),   # outlier columns: S = 12, ov = 4
    D(272, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=vec store=vec idx=elem:34 perm=0 outl=8 groups=1 ragged=0", k=65536, S=8, ov=8),   # outlier columns: S = 8, ov = v
    D(272, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:2 perm=0 outl=0 groups=2 ragged=0", k=65536, C=2),   # two groups of 136 columns
    D(544, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=24 norm=vec store=vec idx=win:64,elem:4 perm=0 outl=0 groups=4 ragged=0", k=65536, C=4),   # four groups of 136 columns
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=24 norm=vec store=vec idx=elem:33 perm=0 outl=0 groups=2 ragged=0", k=65536, C=2),   # two groups of 132 columns: G % 8 == 4
    D(528, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=24 norm=vec store=vec idx=elem:66 perm=0 outl=0 groups=4 ragged=0", k=65536, C=4),   # four groups of 132 columns
    D(272, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=24 norm=vec store=vec idx=elem:34 perm=1 outl=4 groups=2 ragged=0", k=65536, C=2, perm=1, S=8, ov=4),   # a permutation, outliers and groups together
    D(264, 37, "bf16",
      "dequant dt=bf16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=vec store=vec idx=elem:33 perm=1 outl=0 groups=1 ragged=0", k=65536, perm=1),   # a permutation
    D(280, 37, "bf16",
      "dequant dt=bf16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=vec store=vec idx=elem:35 perm=0 outl=4 groups=1 ragged=0", k=65536, S=12, ov=4),   # outlier columns: S = 12, ov = 4
    D(272, 37, "bf16",
      "dequant dt=bf16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=vec store=vec idx=elem:34 perm=0 outl=8 groups=1 ragged=0", k=65536, S=8, ov=8),   # outlier columns: S = 8, ov = v
    D(272, 37, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:2 perm=0 outl=0 groups=2 ragged=0", k=65536, C=2),   # two groups of 136 columns
    D(544, 37, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=24 norm=vec store=vec idx=win:64,elem:4 perm=0 outl=0 groups=4 ragged=0", k=65536, C=4),   # four groups of 136 columns
    D(264, 37, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=24 norm=vec store=vec idx=elem:33 perm=0 outl=0 groups=2 ragged=0", k=65536, C=2),   # two groups of 132 columns: G % 8 == 4
    D(528, 37, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=24 norm=vec store=vec idx=elem:66 perm=0 outl=0 groups=4 ragged=0", k=65536, C=4),   # four groups of 132 columns
    D(272, 37, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=24 norm=vec store=vec idx=elem:34 perm=1 outl=4 groups=2 ragged=0", k=65536, C=2, perm=1, S=8, ov=4),   # a permutation, outliers and groups together
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=elem:33 perm=1 outl=0 groups=1 ragged=0", k=65536, kr=0, perm=1),   # a permutation
    D(280, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=elem:35 perm=0 outl=4 groups=1 ragged=0", k=65536, kr=0, S=12, ov=4),   # outlier columns: S = 12, ov = 4
    D(272, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=elem:34 perm=0 outl=8 groups=1 ragged=0", k=65536, kr=0, S=8, ov=8),   # outlier columns: S = 8, ov = v
    D(272, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:34 perm=0 outl=0 groups=2 ragged=0", k=65536, kr=0, C=2),   # two groups of 136 columns
    D(544, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:68 perm=0 outl=0 groups=4 ragged=0", k=65536, kr=0, C=4),   # four groups of 136 columns
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=elem:33 perm=0 outl=0 groups=2 ragged=0", k=65536, kr=0, C=2),   # two groups of 132 columns: G % 8 == 4
    D(528, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=elem:66 perm=0 outl=0 groups=4 ragged=0", k=65536, kr=0, C=4),   # four groups of 132 columns
    D(272, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=elem:34 perm=1 outl=4 groups=2 ragged=0", k=65536, kr=0, C=2, perm=1, S=8, ov=4),   # a permutation, outliers and groups together
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0),   # aligned
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=scalar idx=vec:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0, w_off=2),   # W at + 2 bytes
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=scalar store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0, norm_off=2),   # scale / bias at + 2 bytes
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=elem:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0, idx_off=4),   # indices at + 4 bytes
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=none store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0, norm=0),   # no scale / bias
    D(264, 37, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0),   # aligned
    D(264, 37, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=scalar idx=vec:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0, w_off=2),   # W at + 2 bytes
    D(264, 37, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=scalar store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0, norm_off=2),   # scale / bias at + 2 bytes
    D(264, 37, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=elem:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0, idx_off=4),   # indices at + 4 bytes
    D(264, 37, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=16 norm=none store=vec idx=vec:33 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=0, norm=0),   # no scale / bias
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=vec store=scalar idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, w_off=2),   # W at + 2 bytes
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=scalar store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, norm_off=2),   # scale / bias at + 2 bytes
    D(264, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=4096 colblocks=1 t=24 norm=vec store=vec idx=win:32,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, idx_off=4),   # indices at + 4 bytes
    D(1856, 72, "f16",
      "dequant dt=f16 v=8 tab=1 lds=512 colblocks=1 t=8 norm=vec store=vec idx=win:230,elem:2 perm=0 outl=0 groups=1 ragged=0", k=16, kr=16, special=1),   # special values, TAB 1
    D(1856, 72, "f16",
      "dequant dt=f16 v=8 tab=2 lds=256 colblocks=1 t=20 norm=vec store=vec idx=win:231,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=16, special=1),   # special values, TAB 2
    D(1856, 72, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=27 norm=vec store=vec idx=win5:231,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=2048, special=1),   # special values, TAB 0, T = 27
    D(1856, 72, "bf16",
      "dequant dt=bf16 v=8 tab=1 lds=512 colblocks=1 t=8 norm=vec store=vec idx=win:230,elem:2 perm=0 outl=0 groups=1 ragged=0", k=16, kr=16, special=1),   # special values, TAB 1
    D(1856, 72, "bf16",
      "dequant dt=bf16 v=8 tab=2 lds=256 colblocks=1 t=20 norm=vec store=vec idx=win:231,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=16, special=1),   # special values, TAB 2
    D(1856, 72, "bf16",
      "dequant dt=bf16 v=8 tab=0 lds=0 colblocks=1 t=27 norm=vec store=vec idx=win5:231,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=2048, special=1),   # special values, TAB 0, T = 27
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=32 colblocks=1 t=1 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=2, kr=0),   # census cell 1: 1 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=16384 colblocks=1 t=10 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=1024, kr=0),   # census cell 1: 10 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=11 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=2048, kr=0),   # census cell 1: 11 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=12 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=4096, kr=0),   # census cell 1: 12 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=13 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=8192, kr=0),   # census cell 1: 13 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=14 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=16384, kr=0),   # census cell 1: 14 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=15 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=32768, kr=0),   # census cell 1: 15 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=32 colblocks=1 t=17 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=2),   # census cell 1: 17 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=64 colblocks=1 t=18 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=4),   # census cell 1: 18 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=128 colblocks=1 t=19 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=8),   # census cell 1: 19 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=64 colblocks=1 t=2 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=4, kr=0),   # census cell 1: 2 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=256 colblocks=1 t=20 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=16),   # census cell 1: 20 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=512 colblocks=1 t=21 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=32),   # census cell 1: 21 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=1024 colblocks=1 t=22 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=64),   # census cell 1: 22 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=2048 colblocks=1 t=23 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=128),   # census cell 1: 23 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=8192 colblocks=1 t=25 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=512),   # census cell 1: 25 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=2 lds=16384 colblocks=1 t=26 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=1024),   # census cell 1: 26 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=27 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=2048),   # census cell 1: 27 elem
    D(2040, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=27 norm=vec store=vec idx=win5:255 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=2048),   # census cell 1: 27 win5
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=28 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=4096),   # census cell 1: 28 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=29 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=8192),   # census cell 1: 29 elem
    D(2040, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=29 norm=vec store=vec idx=win5:254,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=8192),   # census cell 1: 29 win5+elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=128 colblocks=1 t=3 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=8, kr=0),   # census cell 1: 3 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=30 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=16384),   # census cell 1: 30 elem
    D(2048, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=30 norm=vec store=vec idx=win5:255,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=16384),   # census cell 1: 30 win5+elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=31 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=32768),   # census cell 1: 31 elem
    D(2048, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=31 norm=vec store=vec idx=win5:255,elem:1 perm=0 outl=0 groups=1 ragged=0", k=65536, kr=32768),   # census cell 1: 31 win5+elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=0 lds=0 colblocks=1 t=32 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=65536, kr=65536),   # census cell 1: 32 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=256 colblocks=1 t=4 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=16, kr=0),   # census cell 1: 4 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=512 colblocks=1 t=5 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=32, kr=0),   # census cell 1: 5 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=1024 colblocks=1 t=6 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=64, kr=0),   # census cell 1: 6 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=2048 colblocks=1 t=7 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=128, kr=0),   # census cell 1: 7 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=4096 colblocks=1 t=8 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", kr=0),   # census cell 1: 8 elem
    D(7, 37, "f16",
      "dequant dt=f16 v=8 tab=1 lds=8192 colblocks=1 t=9 norm=scalar store=scalar idx=elem:1 perm=0 outl=0 groups=1 ragged=1", k=512, kr=0),   # census cell 1: 9 elem
    D(272, 77, "f16",
      "dequant dt=f16 v=16 tab=0 lds=0 colblocks=1 t=16 norm=vec store=vec idx=vec:34 perm=0 outl=0 groups=2 ragged=0", v=16, C=2),   # census cell 6: tab=0 both=at res=below groups=n
]
# ROWS-END


LAYER_KEYS = ("I", "O", "dt", "v", "k", "kr", "C", "perm", "S", "ov", "norm", "special")


@functools.lru_cache(maxsize=4)
def _layer_and_reference(key):
    """(LayerSpec, the oracle's dense W): computed once per layer - the alignment variants of a row share it - and never written"""
    e = dict(zip(LAYER_KEYS, key))
    if e["special"]:
        L = sp.special_layer(e["dt"], e["v"], e["k"], e["kr"])
        assert (L.in_features, L.out_features) == (e["I"], e["O"])
    else:
        L = vo.make_layer(e["I"], e["O"], vector_len=e["v"], num_centroids=e["k"], num_res_centroids=e["kr"], num_codebooks=e["C"],
                          outlier_size=e["S"], outlier_vector_len=e["ov"] if e["S"] else -1, num_outlier_centroids=256 if e["S"] else -1,
                          enable_norm=bool(e["norm"]), enable_perm=bool(e["perm"]), dtype=e["dt"], dist="llm",
                          seed=e["I"] + 3 * e["O"] + 5 * e["v"] + (e["k"] + e["kr"]) % 1009)
    with np.errstate(all="ignore"):
        W = vo.dequant(L, ref_residual_mask_quirk=False)
    W.setflags(write=False)
    return L, W


def layer_and_reference(e):
    return _layer_and_reference(tuple(e[key] for key in LAYER_KEYS))


def shifted(t, off):
    """a copy of tensor t that starts `off` bytes past a 16-byte boundary -> (pointer, the buffer that holds it)"""
    raw = t.detach().contiguous().reshape(-1).view(torch.uint8)
    buf = torch.zeros(raw.numel() + 64, dtype=torch.uint8, device=t.device)
    assert buf.data_ptr() % 16 == 0
    buf[off:off + raw.numel()] = raw
    return buf.data_ptr() + off, buf


def instance_of(desc, w_ptr):
    buf = C.create_string_buffer(512)
    B.check(B.lib().vptq_dequant_instance(desc, w_ptr, buf, len(buf)), "vptq_dequant_instance")
    return buf.value.decode()


def dequant_guarded(L, e, dev):
    """-> (the instance line, W [O, I] as bit patterns, the guard elements in front of and behind it)"""
    m = spec_to_module(L, dev)
    desc, keep = module_desc(m, need_inv_perm=True)
    if e["norm_off"]:
        desc.weight_scale, ks = shifted(m.weight_scale, e["norm_off"])
        desc.weight_bias, kb = shifted(m.weight_bias, e["norm_off"])
        keep += [ks, kb]
    if e["idx_off"]:
        desc.indices, ki = shifted(m.indices, e["idx_off"])
        keep.append(ki)
    I, O = e["I"], e["O"]
    assert e["w_off"] % 2 == 0
    start = GUARD_ROWS * I + e["w_off"] // 2
    buf = torch.full(((O + 2 * GUARD_ROWS) * I + 8,), SENTINEL, dtype=torch.int16, device=dev)
    assert buf.data_ptr() % 16 == 0
    w_ptr = buf.data_ptr() + 2 * start
    inst = instance_of(desc, w_ptr)
    B.check(B.lib().vptq_dequant(desc, w_ptr, B.current_stream_ptr(dev)), "vptq_dequant")
    torch.cuda.synchronize()
    out = buf.cpu().numpy().view(np.uint16)
    return inst, out[start:start + O * I].reshape(O, I), np.concatenate([out[:start], out[start + O * I:]])


@pytest.mark.parametrize("e", ROWS)
def test_dequant_instance_vs_the_oracle(e, dev):
    L, want = layer_and_reference(e)
    inst, got, guards = dequant_guarded(L, e, dev)
    assert inst == e["instance"]
    if e["special"]:
        sp.same_bits(got, want, e["dt"], e["instance"])
    else:
        bad = got != want
        assert not bad.any(), f"{e['instance']}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[:4].tolist()}"
    assert (guards == SENTINEL).all(), f"{e['instance']}: {int((guards != SENTINEL).sum())} guard elements written"
