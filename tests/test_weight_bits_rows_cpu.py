"""The rows of tests/test_weight_bits_gpu.py without a GPU: the instance string of every row is what the library answers for a
descriptor of the row's format, width and token count (fake, never dereferenced pointers, as tests/test_instance_census_cpu.py
builds them) - a row whose string went stale fails here, not only on the GPU - every reference-roundings kernel has a row in both
types, and a permutation is on in about half of them."""
import ctypes as C

import pytest

from vptq_amd import _backend as B
import test_instance_census_cpu as cs
import test_route_models_k256_gpu as k256
import test_weight_bits_gpu as wb
import _dequant_specials as sp

ENTRIES = [p.values[0] for p in wb.ROWS]
untuned = cs.untuned


def _other(e, tokens):
    return dict(entry="packed", I=e["cols"], O=sp.ROWS * e["v"], dt=e["dt"], tokens=tokens, flags=e["flags"], v=e["v"], k=e["k"], kr=e["kr"], C=e["C"],
                perm=e["perm"], bias=0, norm=1, S=e["S"], ov=e["ov"])


def answer(e):
    kind, per = e["kind"], e["per"]
    if kind == "gemv":
        return cs.other_query(_other(e, per))
    if kind in ("grouped", "chain"):
        return k256.instance_of([cs.fake_desc(e["cols"], sp.ROWS * 8, e["dt"], perm=bool(e["perm"])) for _ in range(per)], 1, e["flags"], kind)
    if kind == "sliced":
        return cs.sliced_query(e["cols"], (sp.ROWS * e["v"],), e["dt"], per, "exact", e["v"], e["k"], e["kr"], bool(e["perm"]))
    if kind == "v2":
        return cs.other_query(dict(entry="v2", I=e["cols"], O=sp.ROWS * e["v"], v=e["v"], k=e["k"], kr=e["kr"], rb=1 if e["kr"] <= 256 else 2,
                                   dt=e["dt"], norm=1, bias=0, tokens=per, flags=e["flags"]))
    buf = C.create_string_buffer(512)
    B.check(getattr(B.lib(), f"vptq_quant_{kind}_instance")(cs.fake_other_desc(_other(e, per)), per, e["flags"], buf, len(buf)), kind)
    return buf.value.decode()


@pytest.mark.parametrize("e", [e for e in ENTRIES if e["instance"]], ids=lambda e: f"{e['name']}-{e['dt']}")
def test_row_instances_are_what_the_library_answers(e, untuned):
    assert answer(e) == e["instance"]


def test_rows_reach_every_reference_roundings_kernel_in_both_types():
    kernels = {"gemv_k256", "gemv_k256m", "gemv_k256c", "gemm_k256", "gemm_k256w", "gemv_sliced", "gemv_sliced_tok", "gemv_gather", "gemv_gatherx",
               "gemv_generic", "gemv_v2", "gemm_gather", "gemm_gatherx"}
    for dt in ("f16", "bf16"):
        assert {e["instance"].split()[0] for e in ENTRIES if e["instance"] and e["dt"] == dt} == kernels | ({"gemv_lds"} if dt == "f16" else set())
    assert [e["dt"] for e in ENTRIES if e["kind"] == "fused"] == ["f16"]   # (bf16 vptq_quant_gemm is the folded form)
    assert 0.4 <= sum(e["perm"] for e in ENTRIES) / len(ENTRIES) <= 0.6
    names = [(e["name"], e["dt"]) for e in ENTRIES]
    assert len(set(names)) == len(names)
    # the exception tables name only kernels that have a row
    assert set(wb.BF16_MAY_READ_ZERO) | wb.NAN_FOR_INF <= kernels
