"""The canonical format's five kernels (gemv_k256m, gemv_k256, gemm_k256, gemm_k256t, gemv_k256c) held to the per-output float64
models of test_route_models_gpu.py at EVERY INSTANTIATION: a kernel name is a family of separately compiled instantiations that
the launch code picks by the layer's shape.  Each row names the kernel AND the instance string vptq_quant_gemv*_instance must
give for it - the template arguments and launch-shape facts the dispatch decided - before its 16-bit and VPTQ_GEMV_OUT_F32
outputs are checked, with the route table's bounds and nothing added.  tests/test_instance_census_cpu.py enumerates the
instances the dispatch can be asked for and holds these tables to them.

Shapes: NS = sweeps of 2048 columns; ragged last sweeps and last 8-column chunks (2048 k - 8, 2048 (k - 1) + 8) beside the
4096 / 8192 / 11008 / 14336 of real checkpoints; O = 264 / 136 / 72 keeps a wide layer's model small, I = 256 ... 1024 a tall
one's (every case's model stays below ~16 M weights)."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_route_models_gpu as rm
from test_route_models_gpu import EXACT, MFMA, VALU, F32, BATCHED, SEL, VALU_FOLDED, _check, _np, _dense, _planted
from oracle import vptq_oracle as vo
import _arith_model as am
from _gpu_util import spec_to_module, bits_to_tensor, gemv_abi, kernel_name, module_desc

pytestmark = pytest.mark.gpu
dev = rm.dev

KM, KMF, KMS = "gemv_k256m_kernel", "gemv_k256m_kernel<fast>", "gemv_k256m_kernel<selective>"
KV, KVF, KG, KT = "gemv_k256_kernel", "gemv_k256_kernel<fast>", "gemm_k256_kernel", "gemm_k256t_kernel"
ARITH = {KM: "exact", KMF: "folded", KMS: "selective", KV: "exact", KVF: "folded", KG: "exact", KT: "folded"}


def K(route, I, O, dt, tokens, flags, instance, perm=0, bias=0):
    e = dict(route=route, layer=(I, O, dict(dist="llm", enable_perm=bool(perm), bias=bool(bias))), dt=dt, tokens=tokens, flags=flags,
             arith=ARITH[route], instance=instance, **(VALU_FOLDED if route == KVF else {}))
    return pytest.param(e, id=f"{route}-{dt}-{I}x{O}-t{tokens}-f{flags}-p{perm}")


# ---------------------------------------------------------------------------------------------- one layer, one call
K256_ONE_LAYER = [
    # gemv_k256m: NS = 1 ... 7 x dtype x {exact, folded, selective}, one token
    K(KM, 2040, 264, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=0 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KM, 4096, 264, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=2 nst=1 perm=0 fast=0 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    K(KM, 4104, 264, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=3 nst=1 perm=0 fast=0 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KM, 8192, 264, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=4 nst=1 perm=0 fast=0 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    K(KM, 8200, 264, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=5 nst=2 perm=0 fast=0 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KM, 11008, 136, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=6 nst=2 perm=0 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0"),
    K(KM, 14336, 136, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=7 nst=2 perm=0 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KMF, 2040, 264, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KMF, 4096, 264, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=2 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    K(KMF, 4104, 264, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=3 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KMF, 8192, 264, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=4 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    K(KMF, 8200, 264, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=5 nst=2 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KMF, 11008, 136, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=6 nst=2 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    K(KMF, 14336, 136, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=7 nst=2 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KMS, 2040, 264, "f16", 1, SEL | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", bias=1),
    K(KMS, 4096, 264, "f16", 1, SEL | MFMA, "gemv_k256m dt=f16 ns=2 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1"),
    K(KMS, 4104, 264, "f16", 1, SEL | MFMA, "gemv_k256m dt=f16 ns=3 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", bias=1),
    K(KMS, 8192, 264, "f16", 1, SEL | MFMA, "gemv_k256m dt=f16 ns=4 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1"),
    K(KMS, 8200, 264, "f16", 1, SEL | MFMA, "gemv_k256m dt=f16 ns=5 nst=2 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", bias=1),
    K(KMS, 11008, 136, "f16", 1, SEL | MFMA, "gemv_k256m dt=f16 ns=6 nst=2 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1"),
    K(KMS, 14336, 136, "f16", 1, SEL | MFMA, "gemv_k256m dt=f16 ns=7 nst=2 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", bias=1),
    K(KM, 2040, 264, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KM, 4096, 264, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=2 nst=1 perm=0 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0"),
    K(KM, 4104, 264, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=3 nst=1 perm=0 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KM, 8192, 264, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=4 nst=1 perm=0 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0"),
    K(KM, 8200, 264, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=5 nst=2 perm=0 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KM, 11008, 136, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=6 nst=2 perm=0 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0"),
    K(KM, 14336, 136, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=7 nst=2 perm=0 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KMF, 2040, 264, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KMF, 4096, 264, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=2 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    K(KMF, 4104, 264, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=3 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KMF, 8192, 264, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=4 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    K(KMF, 8200, 264, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=5 nst=2 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KMF, 11008, 136, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=6 nst=2 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    K(KMF, 14336, 136, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=7 nst=2 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KMS, 2040, 264, "bf16", 1, SEL | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", bias=1),
    K(KMS, 4096, 264, "bf16", 1, SEL | MFMA, "gemv_k256m dt=bf16 ns=2 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1"),
    K(KMS, 4104, 264, "bf16", 1, SEL | MFMA, "gemv_k256m dt=bf16 ns=3 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", bias=1),
    K(KMS, 8192, 264, "bf16", 1, SEL | MFMA, "gemv_k256m dt=bf16 ns=4 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1"),
    K(KMS, 8200, 264, "bf16", 1, SEL | MFMA, "gemv_k256m dt=bf16 ns=5 nst=2 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", bias=1),
    K(KMS, 11008, 136, "bf16", 1, SEL | MFMA, "gemv_k256m dt=bf16 ns=6 nst=2 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1"),
    K(KMS, 14336, 136, "bf16", 1, SEL | MFMA, "gemv_k256m dt=bf16 ns=7 nst=2 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", bias=1),
    K(KM, 8, 136, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0"),
    K(KMF, 2056, 136, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=2 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    K(KMF, 6136, 136, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=3 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    K(KM, 8184, 136, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=4 nst=1 perm=0 fast=0 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    K(KM, 10240, 136, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=5 nst=2 perm=0 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0"),
    K(KMF, 12280, 136, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=6 nst=2 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    K(KMF, 12296, 136, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=7 nst=2 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    # ... with an input permutation: both staging-phase counts, both sides of the fp16 kSB switch, every form
    K(KM, 2040, 136, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=1 fast=0 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMF, 2040, 136, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMS, 2040, 136, "f16", 1, SEL | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", perm=1, bias=1),
    K(KM, 2040, 136, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=1 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMF, 2040, 136, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMS, 2040, 136, "bf16", 1, SEL | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", perm=1, bias=1),
    K(KM, 8192, 136, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=4 nst=1 perm=1 fast=0 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMF, 8192, 136, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=4 nst=1 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMS, 8192, 136, "f16", 1, SEL | MFMA, "gemv_k256m dt=f16 ns=4 nst=1 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", perm=1, bias=1),
    K(KM, 8192, 136, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=4 nst=1 perm=1 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMF, 8192, 136, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=4 nst=1 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMS, 8192, 136, "bf16", 1, SEL | MFMA, "gemv_k256m dt=bf16 ns=4 nst=1 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", perm=1, bias=1),
    K(KM, 10240, 136, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=5 nst=2 perm=1 fast=0 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMF, 10240, 136, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=5 nst=2 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMS, 10240, 136, "f16", 1, SEL | MFMA, "gemv_k256m dt=f16 ns=5 nst=2 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", perm=1, bias=1),
    K(KM, 10240, 136, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=5 nst=2 perm=1 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMF, 10240, 136, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=5 nst=2 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMS, 10240, 136, "bf16", 1, SEL | MFMA, "gemv_k256m dt=bf16 ns=5 nst=2 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", perm=1, bias=1),
    K(KM, 14336, 136, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=7 nst=2 perm=1 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMF, 14336, 136, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=7 nst=2 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMS, 14336, 136, "f16", 1, SEL | MFMA, "gemv_k256m dt=f16 ns=7 nst=2 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", perm=1, bias=1),
    K(KM, 14336, 136, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=7 nst=2 perm=1 fast=0 tok=1 sb=1 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMF, 14336, 136, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=7 nst=2 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", perm=1, bias=1),
    K(KMS, 14336, 136, "bf16", 1, SEL | MFMA, "gemv_k256m dt=bf16 ns=7 nst=2 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=1", perm=1, bias=1),
    # ... token slots 2 and 4 (3 tokens: an unused slot), every supported width, + a permutation
    K(KM, 2040, 136, "f16", 2, EXACT | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=0 tok=2 sb=1 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KM, 4096, 136, "f16", 2, EXACT | MFMA, "gemv_k256m dt=f16 ns=2 nst=1 perm=0 fast=0 tok=2 sb=1 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KM, 4104, 136, "f16", 2, EXACT | MFMA, "gemv_k256m dt=f16 ns=3 nst=1 perm=0 fast=0 tok=2 sb=1 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KM, 8192, 136, "f16", 2, EXACT | MFMA, "gemv_k256m dt=f16 ns=4 nst=1 perm=0 fast=0 tok=2 sb=1 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KM, 8200, 136, "f16", 2, EXACT | MFMA, "gemv_k256m dt=f16 ns=5 nst=2 perm=0 fast=0 tok=2 sb=1 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KM, 11008, 136, "f16", 2, EXACT | MFMA, "gemv_k256m dt=f16 ns=6 nst=2 perm=0 fast=0 tok=2 sb=1 entry=0 slots=2 units=1 sel=0", bias=1),
    K(KM, 2040, 136, "f16", 3, EXACT | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=0 tok=4 sb=1 entry=0 slots=4 units=1 sel=0"),
    K(KM, 4096, 136, "f16", 3, EXACT | MFMA, "gemv_k256m dt=f16 ns=2 nst=1 perm=0 fast=0 tok=4 sb=1 entry=0 slots=4 units=1 sel=0"),
    K(KM, 2040, 136, "f16", 4, EXACT | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=0 tok=4 sb=1 entry=0 slots=4 units=1 sel=0"),
    K(KM, 4096, 136, "f16", 4, EXACT | MFMA, "gemv_k256m dt=f16 ns=2 nst=1 perm=0 fast=0 tok=4 sb=1 entry=0 slots=4 units=1 sel=0"),
    K(KMF, 2040, 136, "f16", 2, MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KMF, 4096, 136, "f16", 2, MFMA, "gemv_k256m dt=f16 ns=2 nst=1 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KMF, 4104, 136, "f16", 2, MFMA, "gemv_k256m dt=f16 ns=3 nst=1 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KMF, 8192, 136, "f16", 2, MFMA, "gemv_k256m dt=f16 ns=4 nst=1 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KMF, 8200, 136, "f16", 2, MFMA, "gemv_k256m dt=f16 ns=5 nst=2 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KMF, 11008, 136, "f16", 2, MFMA, "gemv_k256m dt=f16 ns=6 nst=2 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KMF, 14336, 136, "f16", 2, MFMA, "gemv_k256m dt=f16 ns=7 nst=2 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KMF, 2040, 136, "f16", 3, MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=1 sel=0"),
    K(KMF, 4096, 136, "f16", 3, MFMA, "gemv_k256m dt=f16 ns=2 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=1 sel=0"),
    K(KMF, 4104, 136, "f16", 3, MFMA, "gemv_k256m dt=f16 ns=3 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=1 sel=0"),
    K(KMF, 8192, 136, "f16", 3, MFMA, "gemv_k256m dt=f16 ns=4 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=3 units=1 sel=0"),
    K(KMF, 8200, 136, "f16", 3, MFMA, "gemv_k256m dt=f16 ns=5 nst=2 perm=0 fast=1 tok=4 sb=0 entry=0 slots=3 units=1 sel=0"),
    K(KMF, 11008, 136, "f16", 3, MFMA, "gemv_k256m dt=f16 ns=6 nst=2 perm=0 fast=1 tok=4 sb=0 entry=0 slots=1 units=1 sel=0"),
    K(KMF, 2040, 136, "f16", 4, MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=1 sel=0"),
    K(KMF, 4096, 136, "f16", 4, MFMA, "gemv_k256m dt=f16 ns=2 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=1 sel=0"),
    K(KMF, 4104, 136, "f16", 4, MFMA, "gemv_k256m dt=f16 ns=3 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=1 sel=0"),
    K(KMF, 8192, 136, "f16", 4, MFMA, "gemv_k256m dt=f16 ns=4 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=3 units=1 sel=0"),
    K(KMF, 8200, 136, "f16", 4, MFMA, "gemv_k256m dt=f16 ns=5 nst=2 perm=0 fast=1 tok=4 sb=0 entry=0 slots=3 units=1 sel=0"),
    K(KMF, 11008, 136, "f16", 4, MFMA, "gemv_k256m dt=f16 ns=6 nst=2 perm=0 fast=1 tok=4 sb=0 entry=0 slots=1 units=1 sel=0"),
    K(KM, 2040, 136, "bf16", 2, EXACT | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=0 tok=2 sb=1 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KM, 4096, 136, "bf16", 2, EXACT | MFMA, "gemv_k256m dt=bf16 ns=2 nst=1 perm=0 fast=0 tok=2 sb=1 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KM, 4104, 136, "bf16", 2, EXACT | MFMA, "gemv_k256m dt=bf16 ns=3 nst=1 perm=0 fast=0 tok=2 sb=1 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KM, 8192, 136, "bf16", 2, EXACT | MFMA, "gemv_k256m dt=bf16 ns=4 nst=1 perm=0 fast=0 tok=2 sb=1 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KM, 8200, 136, "bf16", 2, EXACT | MFMA, "gemv_k256m dt=bf16 ns=5 nst=2 perm=0 fast=0 tok=2 sb=1 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KM, 11008, 136, "bf16", 2, EXACT | MFMA, "gemv_k256m dt=bf16 ns=6 nst=2 perm=0 fast=0 tok=2 sb=1 entry=0 slots=2 units=1 sel=0", bias=1),
    K(KM, 2040, 136, "bf16", 3, EXACT | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=0 tok=4 sb=1 entry=0 slots=4 units=1 sel=0"),
    K(KM, 2040, 136, "bf16", 4, EXACT | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=0 tok=4 sb=1 entry=0 slots=4 units=1 sel=0"),
    K(KMF, 2040, 136, "bf16", 2, MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KMF, 4096, 136, "bf16", 2, MFMA, "gemv_k256m dt=bf16 ns=2 nst=1 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KMF, 4104, 136, "bf16", 2, MFMA, "gemv_k256m dt=bf16 ns=3 nst=1 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KMF, 8192, 136, "bf16", 2, MFMA, "gemv_k256m dt=bf16 ns=4 nst=1 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KMF, 8200, 136, "bf16", 2, MFMA, "gemv_k256m dt=bf16 ns=5 nst=2 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KMF, 11008, 136, "bf16", 2, MFMA, "gemv_k256m dt=bf16 ns=6 nst=2 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KMF, 14336, 136, "bf16", 2, MFMA, "gemv_k256m dt=bf16 ns=7 nst=2 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", bias=1),
    K(KMF, 2040, 136, "bf16", 3, MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=1 sel=0"),
    K(KMF, 4096, 136, "bf16", 3, MFMA, "gemv_k256m dt=bf16 ns=2 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=1 sel=0"),
    K(KMF, 4104, 136, "bf16", 3, MFMA, "gemv_k256m dt=bf16 ns=3 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=1 sel=0"),
    K(KMF, 8192, 136, "bf16", 3, MFMA, "gemv_k256m dt=bf16 ns=4 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=3 units=1 sel=0"),
    K(KMF, 8200, 136, "bf16", 3, MFMA, "gemv_k256m dt=bf16 ns=5 nst=2 perm=0 fast=1 tok=4 sb=0 entry=0 slots=3 units=1 sel=0"),
    K(KMF, 11008, 136, "bf16", 3, MFMA, "gemv_k256m dt=bf16 ns=6 nst=2 perm=0 fast=1 tok=4 sb=0 entry=0 slots=1 units=1 sel=0"),
    K(KMF, 2040, 136, "bf16", 4, MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=1 sel=0"),
    K(KMF, 4096, 136, "bf16", 4, MFMA, "gemv_k256m dt=bf16 ns=2 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=1 sel=0"),
    K(KMF, 4104, 136, "bf16", 4, MFMA, "gemv_k256m dt=bf16 ns=3 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=1 sel=0"),
    K(KMF, 8192, 136, "bf16", 4, MFMA, "gemv_k256m dt=bf16 ns=4 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=3 units=1 sel=0"),
    K(KMF, 8200, 136, "bf16", 4, MFMA, "gemv_k256m dt=bf16 ns=5 nst=2 perm=0 fast=1 tok=4 sb=0 entry=0 slots=3 units=1 sel=0"),
    K(KMF, 11008, 136, "bf16", 4, MFMA, "gemv_k256m dt=bf16 ns=6 nst=2 perm=0 fast=1 tok=4 sb=0 entry=0 slots=1 units=1 sel=0"),
    K(KM, 2048, 264, "f16", 2, EXACT | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=1 fast=0 tok=2 sb=1 entry=0 slots=4 units=1 sel=0", perm=1),
    K(KM, 2040, 264, "f16", 4, EXACT | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=1 fast=0 tok=4 sb=1 entry=0 slots=4 units=1 sel=0", perm=1),
    K(KM, 8200, 136, "f16", 2, EXACT | MFMA, "gemv_k256m dt=f16 ns=5 nst=2 perm=1 fast=0 tok=2 sb=1 entry=0 slots=4 units=1 sel=0", perm=1),
    K(KMF, 2048, 264, "f16", 2, MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=1 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", perm=1),
    K(KMF, 2040, 264, "f16", 4, MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=1 fast=1 tok=4 sb=0 entry=0 slots=4 units=1 sel=0", perm=1),
    K(KMF, 8200, 136, "f16", 2, MFMA, "gemv_k256m dt=f16 ns=5 nst=2 perm=1 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", perm=1),
    K(KM, 2048, 264, "bf16", 2, EXACT | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=1 fast=0 tok=2 sb=1 entry=0 slots=4 units=1 sel=0", perm=1),
    K(KM, 2040, 264, "bf16", 4, EXACT | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=1 fast=0 tok=4 sb=1 entry=0 slots=4 units=1 sel=0", perm=1),
    K(KM, 8200, 136, "bf16", 2, EXACT | MFMA, "gemv_k256m dt=bf16 ns=5 nst=2 perm=1 fast=0 tok=2 sb=1 entry=0 slots=4 units=1 sel=0", perm=1),
    K(KMF, 2048, 264, "bf16", 2, MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=1 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", perm=1),
    K(KMF, 2040, 264, "bf16", 4, MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=1 fast=1 tok=4 sb=0 entry=0 slots=4 units=1 sel=0", perm=1),
    K(KMF, 8200, 136, "bf16", 2, MFMA, "gemv_k256m dt=bf16 ns=5 nst=2 perm=1 fast=1 tok=2 sb=0 entry=0 slots=4 units=1 sel=0", perm=1),
    # ... the unstaged wide form (folded, beyond 14336 columns)
    K(KMF, 28672, 264, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=2 nst=0 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0", bias=1),
    K(KMF, 14344, 136, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=2 nst=0 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    K(KMF, 18424, 136, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=2 nst=0 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=1 sel=0"),
    # ... several row groups per workgroup (more than 256 / 512 / 768 row groups of 4 vector-rows), the last one partial
    K(KM, 256, 8224, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=0 tok=1 sb=0 entry=1 slots=4 units=2 sel=0"),
    K(KM, 512, 8232, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=0 tok=1 sb=0 entry=1 slots=4 units=2 sel=0", bias=1),
    K(KM, 264, 16408, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=0 tok=1 sb=0 entry=1 slots=4 units=3 sel=0"),
    K(KMF, 256, 8224, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=2 sel=0"),
    K(KMF, 512, 8232, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=2 sel=0", bias=1),
    K(KMF, 264, 16408, "f16", 1, MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=3 sel=0"),
    K(KMS, 256, 8224, "f16", 1, SEL | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=2 sel=1"),
    K(KMS, 512, 8232, "f16", 1, SEL | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=2 sel=1", bias=1),
    K(KMS, 264, 16408, "f16", 1, SEL | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=3 sel=1"),
    K(KM, 256, 8224, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=0 tok=1 sb=1 entry=1 slots=4 units=2 sel=0"),
    K(KM, 512, 8232, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=0 tok=1 sb=1 entry=1 slots=4 units=2 sel=0", bias=1),
    K(KM, 264, 16408, "bf16", 1, EXACT | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=0 tok=1 sb=1 entry=1 slots=4 units=3 sel=0"),
    K(KMF, 256, 8224, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=2 sel=0"),
    K(KMF, 512, 8232, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=2 sel=0", bias=1),
    K(KMF, 264, 16408, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=3 sel=0"),
    K(KMS, 256, 8224, "bf16", 1, SEL | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=2 sel=1"),
    K(KMS, 512, 8232, "bf16", 1, SEL | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=2 sel=1", bias=1),
    K(KMS, 264, 16408, "bf16", 1, SEL | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=1 slots=4 units=3 sel=1"),
    K(KM, 2056, 8224, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=2 nst=1 perm=0 fast=0 tok=1 sb=0 entry=1 slots=4 units=2 sel=0"),
    K(KMF, 256, 24624, "bf16", 1, MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=1 fast=1 tok=1 sb=0 entry=1 slots=4 units=4 sel=0", perm=1),
    K(KM, 256, 8232, "f16", 2, EXACT | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=0 tok=2 sb=1 entry=0 slots=4 units=2 sel=0"),
    K(KMF, 256, 8232, "bf16", 4, MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=2 sel=0"),
    K(KM, 256, 8232, "f16", 1, EXACT | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=1 fast=0 tok=1 sb=0 entry=1 slots=4 units=2 sel=0", perm=1),
    K(KM, 264, 16408, "bf16", 2, EXACT | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=0 tok=2 sb=1 entry=0 slots=4 units=3 sel=0", bias=1),
    K(KMF, 256, 8232, "bf16", 2, MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=2 sel=0"),
    K(KMF, 264, 16408, "f16", 2, MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=2 sb=0 entry=0 slots=4 units=3 sel=0", bias=1),
    K(KM, 256, 8232, "f16", 4, EXACT | MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=0 tok=4 sb=1 entry=0 slots=4 units=2 sel=0"),
    K(KM, 264, 16408, "bf16", 4, EXACT | MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=0 tok=4 sb=1 entry=0 slots=4 units=3 sel=0", bias=1),
    K(KMF, 264, 16408, "f16", 4, MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=3 sel=0", bias=1),
    K(KMF, 256, 8232, "f16", 3, MFMA, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=2 sel=0"),
    K(KMF, 264, 16408, "bf16", 3, MFMA, "gemv_k256m dt=bf16 ns=1 nst=1 perm=0 fast=1 tok=4 sb=0 entry=0 slots=4 units=3 sel=0", bias=1),
    K(KMF, 10240, 136, "f16", 4, MFMA, "gemv_k256m dt=f16 ns=5 nst=2 perm=1 fast=1 tok=4 sb=0 entry=0 slots=1 units=1 sel=0", perm=1),
    K(KMF, 8200, 136, "bf16", 3, MFMA, "gemv_k256m dt=bf16 ns=5 nst=2 perm=1 fast=1 tok=4 sb=0 entry=0 slots=3 units=1 sel=0", perm=1),
    # gemv_k256: ROWS x SW x PERM (ROWS = 2: fp16, one token, from 1023 vector-rows on), TOK, folded, bf16
    K(KV, 1024, 264, "f16", 1, EXACT | VALU, "gemv_k256 dt=f16 rows=1 tok=1 sw=1 perm=0 fast=0 entry=1"),
    K(KVF, 1024, 264, "f16", 1, VALU, "gemv_k256 dt=f16 rows=1 tok=1 sw=1 perm=0 fast=1 entry=1"),
    K(KV, 1024, 264, "f16", 1, EXACT | VALU, "gemv_k256 dt=f16 rows=1 tok=1 sw=1 perm=1 fast=0 entry=1", perm=1, bias=1),
    K(KVF, 1024, 264, "f16", 1, VALU, "gemv_k256 dt=f16 rows=1 tok=1 sw=1 perm=1 fast=1 entry=1", perm=1),
    K(KV, 4104, 264, "f16", 1, EXACT | VALU, "gemv_k256 dt=f16 rows=1 tok=1 sw=2 perm=0 fast=0 entry=1"),
    K(KVF, 4104, 264, "f16", 1, VALU, "gemv_k256 dt=f16 rows=1 tok=1 sw=2 perm=0 fast=1 entry=1"),
    K(KV, 4104, 264, "f16", 1, EXACT | VALU, "gemv_k256 dt=f16 rows=1 tok=1 sw=2 perm=1 fast=0 entry=1", perm=1, bias=1),
    K(KVF, 4104, 264, "f16", 1, VALU, "gemv_k256 dt=f16 rows=1 tok=1 sw=2 perm=1 fast=1 entry=1", perm=1),
    K(KV, 1024, 8184, "f16", 1, EXACT | VALU, "gemv_k256 dt=f16 rows=2 tok=1 sw=1 perm=0 fast=0 entry=1"),
    K(KVF, 1024, 8184, "f16", 1, VALU, "gemv_k256 dt=f16 rows=2 tok=1 sw=1 perm=0 fast=1 entry=1"),
    K(KV, 1024, 8184, "f16", 1, EXACT | VALU, "gemv_k256 dt=f16 rows=2 tok=1 sw=1 perm=1 fast=0 entry=1", perm=1, bias=1),
    K(KVF, 1024, 8184, "f16", 1, VALU, "gemv_k256 dt=f16 rows=2 tok=1 sw=1 perm=1 fast=1 entry=1", perm=1),
    K(KV, 1536, 8200, "f16", 1, EXACT | VALU, "gemv_k256 dt=f16 rows=2 tok=1 sw=1 perm=0 fast=0 entry=1"),
    K(KV, 4104, 4096, "f16", 1, EXACT | VALU, "gemv_k256 dt=f16 rows=1 tok=1 sw=2 perm=1 fast=0 entry=1", perm=1),
    K(KVF, 4104, 4088, "f16", 1, VALU, "gemv_k256 dt=f16 rows=1 tok=1 sw=2 perm=0 fast=1 entry=1"),
    K(KVF, 4104, 4096, "f16", 1, VALU, "gemv_k256 dt=f16 rows=1 tok=1 sw=2 perm=1 fast=1 entry=1", perm=1),
    K(KV, 2040, 264, "f16", 1, EXACT | VALU, "gemv_k256 dt=f16 rows=1 tok=1 sw=1 perm=1 fast=0 entry=1", perm=1, bias=1),
    K(KV, 2040, 264, "f16", 2, EXACT | VALU, "gemv_k256 dt=f16 rows=1 tok=2 sw=1 perm=0 fast=0 entry=0"),
    K(KV, 4104, 264, "f16", 2, EXACT | VALU, "gemv_k256 dt=f16 rows=1 tok=2 sw=2 perm=1 fast=0 entry=0", perm=1),
    K(KV, 2040, 264, "f16", 3, EXACT | VALU, "gemv_k256 dt=f16 rows=1 tok=4 sw=1 perm=1 fast=0 entry=0", perm=1, bias=1),
    K(KV, 4104, 264, "f16", 3, EXACT | VALU, "gemv_k256 dt=f16 rows=1 tok=4 sw=1 perm=0 fast=0 entry=0", bias=1),
    K(KV, 2040, 264, "f16", 4, EXACT | VALU, "gemv_k256 dt=f16 rows=1 tok=4 sw=1 perm=0 fast=0 entry=0"),
    K(KV, 4104, 264, "f16", 4, EXACT | VALU, "gemv_k256 dt=f16 rows=1 tok=4 sw=1 perm=1 fast=0 entry=0", perm=1),
    K(KV, 2040, 264, "bf16", 1, EXACT | VALU, "gemv_k256 dt=bf16 rows=1 tok=1 sw=1 perm=1 fast=0 entry=1", perm=1, bias=1),
    K(KV, 4104, 264, "bf16", 1, EXACT | VALU, "gemv_k256 dt=bf16 rows=1 tok=1 sw=2 perm=0 fast=0 entry=1", bias=1),
    K(KV, 2040, 264, "bf16", 2, EXACT | VALU, "gemv_k256 dt=bf16 rows=1 tok=2 sw=1 perm=0 fast=0 entry=0"),
    K(KV, 4104, 264, "bf16", 2, EXACT | VALU, "gemv_k256 dt=bf16 rows=1 tok=2 sw=2 perm=1 fast=0 entry=0", perm=1),
    K(KV, 2040, 264, "bf16", 3, EXACT | VALU, "gemv_k256 dt=bf16 rows=1 tok=4 sw=1 perm=1 fast=0 entry=0", perm=1, bias=1),
    K(KV, 4104, 264, "bf16", 3, EXACT | VALU, "gemv_k256 dt=bf16 rows=1 tok=4 sw=1 perm=0 fast=0 entry=0", bias=1),
    K(KV, 2040, 264, "bf16", 4, EXACT | VALU, "gemv_k256 dt=bf16 rows=1 tok=4 sw=1 perm=0 fast=0 entry=0"),
    K(KV, 4104, 264, "bf16", 4, EXACT | VALU, "gemv_k256 dt=bf16 rows=1 tok=4 sw=1 perm=1 fast=0 entry=0", perm=1),
    K(KV, 2040, 264, "f16", 2, EXACT | VALU, "gemv_k256 dt=f16 rows=1 tok=2 sw=1 perm=1 fast=0 entry=0", perm=1),
    K(KV, 4104, 264, "f16", 2, EXACT | VALU, "gemv_k256 dt=f16 rows=1 tok=2 sw=2 perm=0 fast=0 entry=0"),
    K(KV, 2040, 264, "bf16", 2, EXACT | VALU, "gemv_k256 dt=bf16 rows=1 tok=2 sw=1 perm=1 fast=0 entry=0", perm=1),
    K(KV, 4104, 264, "bf16", 2, EXACT | VALU, "gemv_k256 dt=bf16 rows=1 tok=2 sw=2 perm=0 fast=0 entry=0"),
    K(KVF, 2048, 264, "f16", 2, VALU, "gemv_k256 dt=f16 rows=1 tok=2 sw=1 perm=0 fast=1 entry=0"),
    K(KVF, 2048, 136, "f16", 2, VALU, "gemv_k256 dt=f16 rows=1 tok=2 sw=1 perm=1 fast=1 entry=0", perm=1),
    K(KVF, 6136, 264, "f16", 2, VALU, "gemv_k256 dt=f16 rows=1 tok=2 sw=2 perm=1 fast=1 entry=0", perm=1),
    K(KVF, 6136, 136, "f16", 2, VALU, "gemv_k256 dt=f16 rows=1 tok=2 sw=2 perm=0 fast=1 entry=0"),
    # gemm_k256: tokens 5 / 8 / 16 x dtype x PERM; the pass sets of the busiest workgroup (with an output bias:
    # each pass adds it per row group)
    K(KG, 2056, 264, "f16", 5, EXACT, "gemm_k256 dt=f16 perm=0 tok=5 passes=1"),
    K(KG, 2056, 264, "f16", 5, EXACT, "gemm_k256 dt=f16 perm=1 tok=5 passes=1", perm=1, bias=1),
    K(KG, 2056, 264, "f16", 8, EXACT, "gemm_k256 dt=f16 perm=0 tok=8 passes=1"),
    K(KG, 2056, 264, "f16", 8, EXACT, "gemm_k256 dt=f16 perm=1 tok=8 passes=1", perm=1, bias=1),
    K(KG, 2056, 264, "f16", 16, EXACT, "gemm_k256 dt=f16 perm=0 tok=16 passes=1"),
    K(KG, 2056, 264, "f16", 16, EXACT, "gemm_k256 dt=f16 perm=1 tok=16 passes=1", perm=1, bias=1),
    K(KG, 2056, 264, "bf16", 5, EXACT, "gemm_k256 dt=bf16 perm=0 tok=5 passes=1"),
    K(KG, 2056, 264, "bf16", 5, EXACT, "gemm_k256 dt=bf16 perm=1 tok=5 passes=1", perm=1, bias=1),
    K(KG, 2056, 264, "bf16", 8, EXACT, "gemm_k256 dt=bf16 perm=0 tok=8 passes=1"),
    K(KG, 2056, 264, "bf16", 8, EXACT, "gemm_k256 dt=bf16 perm=1 tok=8 passes=1", perm=1, bias=1),
    K(KG, 2056, 264, "bf16", 16, EXACT, "gemm_k256 dt=bf16 perm=0 tok=16 passes=1"),
    K(KG, 2056, 264, "bf16", 16, EXACT, "gemm_k256 dt=bf16 perm=1 tok=16 passes=1", perm=1, bias=1),
    K(KG, 512, 3080, "f16", 5, EXACT, "gemm_k256 dt=f16 perm=0 tok=5 passes=1", bias=1),
    K(KG, 512, 11272, "bf16", 16, EXACT, "gemm_k256 dt=bf16 perm=1 tok=16 passes=2", perm=1, bias=1),
    K(KG, 512, 19464, "f16", 8, EXACT, "gemm_k256 dt=f16 perm=1 tok=8 passes=2+1", perm=1, bias=1),
    K(KG, 512, 27656, "bf16", 5, EXACT, "gemm_k256 dt=bf16 perm=0 tok=5 passes=4", bias=1),
    K(KG, 256, 35848, "f16", 16, EXACT, "gemm_k256 dt=f16 perm=0 tok=16 passes=4+1", bias=1),
    K(KG, 256, 44040, "bf16", 8, EXACT, "gemm_k256 dt=bf16 perm=1 tok=8 passes=4+2", perm=1, bias=1),
    K(KG, 256, 52232, "f16", 5, EXACT, "gemm_k256 dt=f16 perm=1 tok=5 passes=4+2+1", perm=1, bias=1),
    # gemm_k256t: 1 / 2 / 16 tokens x dtype x PERM; one sweep, several, a ragged last one; one and several row groups per workgroup
    K(KT, 8704, 264, "f16", 1, BATCHED, "gemm_k256t dt=f16 perm=0 tok=1 sweeps=5 rgs=1", bias=1),
    K(KT, 2048, 264, "f16", 1, BATCHED, "gemm_k256t dt=f16 perm=1 tok=1 sweeps=1 rgs=1", perm=1),
    K(KT, 1024, 264, "f16", 2, BATCHED, "gemm_k256t dt=f16 perm=0 tok=2 sweeps=1 rgs=1", bias=1),
    K(KT, 4104, 264, "f16", 2, BATCHED, "gemm_k256t dt=f16 perm=1 tok=2 sweeps=3 rgs=1", perm=1),
    K(KT, 2056, 264, "f16", 16, BATCHED, "gemm_k256t dt=f16 perm=0 tok=16 sweeps=2 rgs=1", bias=1),
    K(KT, 6136, 264, "f16", 16, BATCHED, "gemm_k256t dt=f16 perm=1 tok=16 sweeps=3 rgs=1", perm=1),
    K(KT, 2048, 264, "bf16", 1, BATCHED, "gemm_k256t dt=bf16 perm=0 tok=1 sweeps=1 rgs=1", bias=1),
    K(KT, 8704, 264, "bf16", 1, BATCHED, "gemm_k256t dt=bf16 perm=1 tok=1 sweeps=5 rgs=1", perm=1),
    K(KT, 4104, 264, "bf16", 2, BATCHED, "gemm_k256t dt=bf16 perm=0 tok=2 sweeps=3 rgs=1", bias=1),
    K(KT, 1024, 264, "bf16", 2, BATCHED, "gemm_k256t dt=bf16 perm=1 tok=2 sweeps=1 rgs=1", perm=1),
    K(KT, 6136, 264, "bf16", 16, BATCHED, "gemm_k256t dt=bf16 perm=0 tok=16 sweeps=3 rgs=1", bias=1),
    K(KT, 2056, 264, "bf16", 16, BATCHED, "gemm_k256t dt=bf16 perm=1 tok=16 sweeps=2 rgs=1", perm=1),
    K(KT, 512, 8232, "f16", 16, 0, "gemm_k256t dt=f16 perm=0 tok=16 sweeps=1 rgs=2"),
    K(KT, 1024, 16408, "bf16", 7, 0, "gemm_k256t dt=bf16 perm=1 tok=7 sweeps=1 rgs=3", perm=1),
    K(KT, 2056, 6400, "f16", 2, BATCHED, "gemm_k256t dt=f16 perm=1 tok=2 sweeps=2 rgs=1", perm=1),
]


def instance_of(descs, tokens, flags, entry="one"):
    """the library's answer for a one-layer call ("one"), a grouped call or a chain call of these descriptors"""
    from vptq_amd import _backend as B
    buf = C.create_string_buffer(8192)
    if entry == "one":
        rc = B.lib().vptq_quant_gemv_instance(descs[0], tokens, flags, buf, len(buf))
    else:
        arr = (B.LayerDesc * len(descs))(*descs)
        fn = B.lib().vptq_quant_gemv_grouped_instance if entry == "grouped" else B.lib().vptq_quant_gemv_chain_instance
        rc = fn(arr, len(descs), tokens, flags, buf, len(buf))
    B.check(rc, "vptq_quant_gemv*_instance")
    return buf.value.decode()


def _x_for(L, e, seed):
    if e["arith"] == "exact":
        return _dense(L.in_features, e["tokens"], L.dtype, seed)
    # (beyond 8192 columns gemv_k256m stages in two phases and a wave's threshold runs over its 512 columns of both: a window
    # whose partner lies past the last column has a threshold lower by sqrt(2) - the ordinary columns stay within 1.8 there, so
    # that every rule still picks the planted set, test_route_models_gpu._hot_rules_agree)
    return _planted(L.in_features, e["tokens"], L.dtype, seed, perm=L.perm, clip=1.8 if L.in_features > rm.SEL_STAGE else 2.5)


@pytest.mark.parametrize("e", K256_ONE_LAYER)
def test_k256_instance_vs_its_model(e, dev):
    L = rm._layer(e)
    m = spec_to_module(L, dev)
    assert kernel_name(m, e["tokens"], e["flags"]) == e["route"]
    desc, keep = module_desc(m)
    assert instance_of([desc], e["tokens"], e["flags"]) == e["instance"]
    x, hot = _x_for(L, e, L.in_features + e["tokens"])
    xt = bits_to_tensor(x, L.dtype, dev).reshape(x.shape)
    y16 = _np(gemv_abi(m, xt, e["flags"]))
    y32 = _np(gemv_abi(m, xt, e["flags"], out_f32=True))
    _check(y16, y32, L, x, e, hot, what=f"{e['instance']}")


# ---------------------------------------------------------------------------------------------- grouped launches
# (layers, dtype, tokens, flags, route, instance, twin).  Two copies of one layer: the grouped entry (layer = blockIdx.y) of the
# instantiation whose preloaded-argument entry (..._kernel_1) the one-layer call of the same layer takes (twin) - both are
# checked against the model, and their outputs must be bit-identical.  (Not twins: ROWS = 2 x SW = 2 of gemv_k256 needs 1023
# vector-rows in the launch and more than 4096 columns - two layers of 512 vector-rows reach it, one alone takes ROWS = 1.)
K256_GROUPS = [
    ([(4104, 264, 0), (4104, 264, 0)], "f16", 1, EXACT | MFMA, KM, "gemv_k256m dt=f16 ns=3 nst=1 perm=0 fast=0 tok=1 sb=0 entry=0 slots=4 units=1 sel=0", True),
    ([(10240, 136, 1), (10240, 136, 1)], "f16", 1, EXACT | MFMA, KM, "gemv_k256m dt=f16 ns=5 nst=2 perm=1 fast=0 tok=1 sb=0 entry=0 slots=4 units=1 sel=0", True),
    ([(4104, 264, 0), (4104, 264, 0)], "f16", 1, MFMA, KMF, "gemv_k256m dt=f16 ns=3 nst=1 perm=0 fast=1 tok=1 sb=0 entry=0 slots=4 units=1 sel=0", True),
    ([(10240, 136, 1), (10240, 136, 1)], "f16", 1, MFMA, KMF, "gemv_k256m dt=f16 ns=5 nst=2 perm=1 fast=1 tok=1 sb=0 entry=0 slots=4 units=1 sel=0", True),
    ([(4104, 264, 0), (4104, 264, 0)], "f16", 1, SEL | MFMA, KMS, "gemv_k256m dt=f16 ns=3 nst=1 perm=0 fast=1 tok=1 sb=0 entry=0 slots=4 units=1 sel=1", True),
    ([(10240, 136, 1), (10240, 136, 1)], "f16", 1, SEL | MFMA, KMS, "gemv_k256m dt=f16 ns=5 nst=2 perm=1 fast=1 tok=1 sb=0 entry=0 slots=4 units=1 sel=1", True),
    ([(2048, 264, 0), (2048, 264, 0)], "f16", 1, EXACT | VALU, KV, "gemv_k256 dt=f16 rows=1 tok=1 sw=1 perm=0 fast=0 entry=0", True),
    ([(4104, 264, 1), (4104, 264, 1)], "f16", 1, EXACT | VALU, KV, "gemv_k256 dt=f16 rows=1 tok=1 sw=2 perm=1 fast=0 entry=0", True),
    ([(4104, 264, 0), (4104, 264, 0)], "bf16", 1, EXACT | MFMA, KM, "gemv_k256m dt=bf16 ns=3 nst=1 perm=0 fast=0 tok=1 sb=1 entry=0 slots=4 units=1 sel=0", True),
    ([(10240, 136, 1), (10240, 136, 1)], "bf16", 1, EXACT | MFMA, KM, "gemv_k256m dt=bf16 ns=5 nst=2 perm=1 fast=0 tok=1 sb=1 entry=0 slots=4 units=1 sel=0", True),
    ([(4104, 264, 0), (4104, 264, 0)], "bf16", 1, MFMA, KMF, "gemv_k256m dt=bf16 ns=3 nst=1 perm=0 fast=1 tok=1 sb=0 entry=0 slots=4 units=1 sel=0", True),
    ([(10240, 136, 1), (10240, 136, 1)], "bf16", 1, MFMA, KMF, "gemv_k256m dt=bf16 ns=5 nst=2 perm=1 fast=1 tok=1 sb=0 entry=0 slots=4 units=1 sel=0", True),
    ([(4104, 264, 0), (4104, 264, 0)], "bf16", 1, SEL | MFMA, KMS, "gemv_k256m dt=bf16 ns=3 nst=1 perm=0 fast=1 tok=1 sb=0 entry=0 slots=4 units=1 sel=1", True),
    ([(10240, 136, 1), (10240, 136, 1)], "bf16", 1, SEL | MFMA, KMS, "gemv_k256m dt=bf16 ns=5 nst=2 perm=1 fast=1 tok=1 sb=0 entry=0 slots=4 units=1 sel=1", True),
    ([(2048, 264, 0), (2048, 264, 0)], "bf16", 1, EXACT | VALU, KV, "gemv_k256 dt=bf16 rows=1 tok=1 sw=1 perm=0 fast=0 entry=0", True),
    ([(4104, 264, 1), (4104, 264, 1)], "bf16", 1, EXACT | VALU, KV, "gemv_k256 dt=bf16 rows=1 tok=1 sw=2 perm=1 fast=0 entry=0", True),
    ([(4104, 264, 0), (4104, 264, 0)], "f16", 1, VALU, KVF, "gemv_k256 dt=f16 rows=1 tok=1 sw=2 perm=0 fast=1 entry=0", True),
    ([(2048, 4096, 1), (2048, 4096, 1)], "f16", 1, VALU, KVF, "gemv_k256 dt=f16 rows=2 tok=1 sw=1 perm=1 fast=1 entry=0", False),
    ([(1024, 4104, 0), (1024, 4104, 0)], "f16", 1, EXACT | VALU, KV, "gemv_k256 dt=f16 rows=2 tok=1 sw=1 perm=0 fast=0 entry=0", False),
    ([(4104, 4096, 0), (4104, 4096, 0)], "f16", 1, EXACT | VALU, KV, "gemv_k256 dt=f16 rows=2 tok=1 sw=2 perm=0 fast=0 entry=0", False),
    ([(4104, 4096, 1), (4104, 4096, 1)], "f16", 1, VALU, KVF, "gemv_k256 dt=f16 rows=2 tok=1 sw=2 perm=1 fast=1 entry=0", False),
    ([(4104, 4096, 0), (4104, 4096, 0)], "f16", 1, VALU, KVF, "gemv_k256 dt=f16 rows=2 tok=1 sw=2 perm=0 fast=1 entry=0", False),
    ([(4104, 4096, 1), (4104, 4096, 1)], "f16", 1, EXACT | VALU, KV, "gemv_k256 dt=f16 rows=2 tok=1 sw=2 perm=1 fast=0 entry=0", False),
    ([(512, 9600, 0), (512, 264, 0), (512, 3208, 0)], "f16", 1, EXACT | MFMA, KM, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=0 tok=1 sb=0 entry=0 slots=4 units=2 sel=0", False),
    ([(512, 9600, 1), (512, 3208, 1)], "bf16", 1, MFMA, KMF, "gemv_k256m dt=bf16 ns=1 nst=1 perm=1 fast=1 tok=1 sb=0 entry=0 slots=4 units=2 sel=0", False),
    ([(1024, 6408, 0), (1024, 3840, 0)], "f16", 2, EXACT | MFMA, KM, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=0 tok=2 sb=1 entry=0 slots=4 units=2 sel=0", False),
    ([(512, 9600, 0), (512, 3208, 0)], "f16", 1, SEL | MFMA, KMS, "gemv_k256m dt=f16 ns=1 nst=1 perm=0 fast=1 tok=1 sb=0 entry=0 slots=4 units=2 sel=1", False),
]


@pytest.mark.parametrize("g", K256_GROUPS, ids=[f"{g[4]}-{g[1]}-{g[0][0][0]}x{g[0][0][1]}-n{len(g[0])}-p{int(g[0][0][2])}" for g in K256_GROUPS])
def test_k256_grouped_instance_vs_its_model(g, dev):
    from vptq_amd import _backend as B
    shapes, dt, tokens, flags, route, instance, twin = g
    twins = len(shapes) == 2 and shapes[0] == shapes[1]
    es = [dict(layer=(I, O, dict(dist="llm", enable_perm=bool(p), bias=i == 0 or twins)), dt=dt, tokens=tokens, arith=ARITH[route],
               **(VALU_FOLDED if route == KVF else {})) for i, (I, O, p) in enumerate(shapes)]
    Ls = [rm._layer(e, seed=0 if twins else i) for i, e in enumerate(es)]
    ms = [spec_to_module(L, dev) for L in Ls]
    keep = [module_desc(m) for m in ms]
    descs = (B.LayerDesc * len(ms))(*[k[0] for k in keep])
    name = B.lib().vptq_quant_gemv_grouped_kernel_name(descs, len(ms), tokens, flags)
    assert name is not None and name.decode() == route
    assert instance_of([k[0] for k in keep], tokens, flags, "grouped") == instance
    xs = [_x_for(L, es[0], 5 + tokens) for L in Ls]   # (a permuted layer's planted columns follow its own permutation)
    xt = [bits_to_tensor(x, dt, dev).reshape(x.shape) for x, _ in xs]
    outs = {}
    for f32 in (False, True):
        ys = [torch.empty(1, tokens, L.out_features, dtype=torch.float32 if f32 else xt[0].dtype, device=dev) for L in Ls]
        xp = (C.c_void_p * len(ms))(*[t.data_ptr() for t in xt])
        yp = (C.c_void_p * len(ms))(*[y.data_ptr() for y in ys])
        B.check(B.lib().vptq_quant_gemv_grouped(descs, len(ms), xp, yp, tokens, flags | (F32 if f32 else 0), B.current_stream_ptr(dev)),
                "vptq_quant_gemv_grouped")
        torch.cuda.synchronize()
        outs[f32] = ys
    for i, L in enumerate(Ls):
        _check(_np(outs[False][i]), _np(outs[True][i]), L, xs[i][0], es[i], xs[i][1], what=f"grouped {instance} layer {i}")
    if twins and tokens == 1:
        one = instance_of([keep[0][0]], 1, flags)
        assert (one == instance.replace("entry=0", "entry=1")) == twin, f"the one-layer call takes {one}"
    if twin:
        for f32 in (False, True):
            y1 = gemv_abi(ms[0], xt[0], flags, out_f32=f32)
            for y in outs[f32]:
                assert torch.equal(y.view(torch.int32 if f32 else torch.int16), y1.view(torch.int32 if f32 else torch.int16)), \
                    f"{instance}: the two entries' outputs differ"


# ---------------------------------------------------------------------------------------------- the persistent chain launch
# lists that mix 1 ... 7 sweeps and layers with and without an input permutation in ONE launch (O >= 264: none the load-time gate
# hands to the reference's roundings)
K256_CHAIN_SHAPES = [(2048 - 8, 264, 0), (4096, 264, 1), (6144 + 8, 264, 0), (8192, 264, 0), (10240, 264, 1), (11008, 264, 0), (14336, 264, 1),
                     (1024, 520, 0), (4096 + 8, 264, 1), (2048, 1032, 0)]
K256_CHAIN_SWEEPS = "sweeps=1,2,4,4,5,6,7,1,3,1 perm=0,1,0,0,1,0,1,0,1,0"
K256_CHAIN_INDEPENDENT = ["exact", "folded", "selective"]
K256_CHAIN_DTYPES = ["f16", "bf16"]             # of the independent and of the dependent lists (the census reads both)
K256_CHAIN_DEPENDENT = ["folded"]
# dependent lists (folded form, no permutations: those go layer by layer): layer i reads layer i - 1's output.  (The O >= 264
# remark above is about the independent shapes; of these, the load-time probe gates bf16 layer 4 - see the test.)
K256_CHAIN_DIMS = [1024, 4104, 2048, 6144, 1032, 10240, 520, 14336, 264, 8192, 1024]
K256_CHAIN_DEP_SWEEPS = "sweeps=1,3,1,3,1,5,1,7,1,4 perm=0,0,0,0,0,0,0,0,0,0"


def _chain_instance(chain, flags):
    _, subs, _, _, _ = chain._prepare()
    assert len(subs) == 1, "a layer of the list is gated to the reference's roundings"
    idx, descs, _, _, safe, _, _ = subs[0]
    return instance_of(list(descs), 1, flags | safe, "chain")


@pytest.mark.parametrize("arith", K256_CHAIN_INDEPENDENT)
@pytest.mark.parametrize("dt", K256_CHAIN_DTYPES)
def test_k256_independent_chain_vs_its_model(arith, dt, dev):
    import vptq_amd
    from vptq_amd.ops.chain import GemvChain
    before = vptq_amd.arithmetic()
    vptq_amd.set_arithmetic({"exact": "reference"}.get(arith, arith))
    try:
        es = [dict(layer=(I, O, dict(dist="llm", enable_perm=bool(p), bias=i % 3 == 1)), dt=dt, tokens=1, arith=arith)
              for i, (I, O, p) in enumerate(K256_CHAIN_SHAPES)]
        Ls = [rm._layer(e, seed=i) for i, e in enumerate(es)]
        ms = [spec_to_module(L, dev) for L in Ls]
        xs = [_x_for(L, es[i], 40 + i) for i, L in enumerate(Ls)]
        xt = [bits_to_tensor(x, dt, dev).reshape(x.shape) for x, _ in xs]
        chain = GemvChain(ms)
        flags = MFMA | (EXACT if arith == "exact" else SEL if arith == "selective" else 0)
        assert chain.kernel_name(1, flags) == "gemv_k256c_kernel"
        assert _chain_instance(chain, flags) == f"gemv_k256c dt={dt} dep=0 mode={arith} layers={len(Ls)} {K256_CHAIN_SWEEPS}"
        y16 = [_np(y) for y in chain(xt, flags=flags)]
        y32 = [_np(y) for y in chain(xt, flags=flags | F32)]
        torch.cuda.synchronize()
    finally:
        vptq_amd.set_arithmetic(before)
    for i, L in enumerate(Ls):
        _check(y16[i], y32[i], L, xs[i][0], es[i], xs[i][1], what=f"chain {arith} layer {i} ({K256_CHAIN_SHAPES[i]})")


@pytest.mark.parametrize("arith", K256_CHAIN_DEPENDENT)
@pytest.mark.parametrize("dt", K256_CHAIN_DTYPES)
def test_k256_dependent_chain_vs_its_model(arith, dt, dev):
    """each layer is checked on the input it actually read: the 16-bit output of the layer before it"""
    import vptq_amd
    from _gpu_util import tensor_to_bits
    before = vptq_amd.arithmetic()
    vptq_amd.set_arithmetic("folded")
    try:
        dims = K256_CHAIN_DIMS
        Ls = [vo.make_layer(dims[i], dims[i + 1], dist="llm", seed=170 + i, dtype=dt, bias=i % 3 == 0) for i in range(len(dims) - 1)]
        ms = [spec_to_module(L, dev) for L in Ls]
        x0, _ = _dense(dims[0], 1, dt, 3)
        # Through the C ABI, on purpose: VQuantLinear's load-time probe (_folded_form_is_safe) gates the bf16 copy of layer 4
        # (1032 -> 10240) to the reference's roundings, and GemvChain then hands the whole dependent list over with
        # VPTQ_GEMV_EXACT, which the library runs layer by layer - no gemv_k256c<DEP> launch to check.  The product would not send
        # that layer to the folded chain kernel; the kernel's arithmetic on it is what this test holds to the folded model.
        # Do not route this back through GemvChain.
        from vptq_amd import _backend as B
        keep = [module_desc(m) for m in ms]
        n = len(ms)
        descs = (B.LayerDesc * n)(*[k[0] for k in keep])
        flags = MFMA | B.GEMV_CHAIN_DEPENDENT
        name = B.lib().vptq_quant_gemv_chain_kernel_name(descs, n, 1, flags)
        assert name is not None and name.decode() == "gemv_k256c_kernel"
        assert instance_of([k[0] for k in keep], 1, flags, "chain") == f"gemv_k256c dt={dt} dep=1 mode=folded layers={n} {K256_CHAIN_DEP_SWEEPS}"
        xt = bits_to_tensor(x0, dt, dev).reshape(x0.shape)
        ys = [torch.empty(1, 1, L.out_features, dtype=xt.dtype, device=dev) for L in Ls]
        nb = B.lib().vptq_quant_gemv_chain_workspace_bytes(n, flags)
        ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
        xp = (C.c_void_p * n)(*([xt.data_ptr()] + [y.data_ptr() for y in ys[:-1]]))
        yp = (C.c_void_p * n)(*[y.data_ptr() for y in ys])
        B.check(B.lib().vptq_quant_gemv_chain(descs, n, xp, yp, 1, flags, ws.data_ptr(), nb, B.current_stream_ptr(dev)), "vptq_quant_gemv_chain")
        torch.cuda.synchronize()
        ybits = [tensor_to_bits(y) for y in ys]
    finally:
        vptq_amd.set_arithmetic(before)
    xin = x0
    for i, L in enumerate(Ls):
        _check(vo.to_f32(ybits[i], dt), None, L, xin, dict(arith="folded"), (), what=f"dependent chain layer {i} ({dims[i]} -> {dims[i + 1]})")
        xin = ybits[i]
