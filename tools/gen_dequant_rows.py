#!/usr/bin/env python3
"""Writes the ROWS table of tests/test_dequant_models_gpu.py (between its ROWS-BEGIN / ROWS-END marks): the rows chosen by hand
below - every instantiation, the LDS limits, every index width, the widths, the causes of the element path, the alignment
variants, the special-value tables - each with the line vptq_dequant_instance answers for a descriptor of its shape, then, cheapest
first, a request of the census grid (tests/test_instance_census_cpu.py:dequant_grid) for every cell the rows above leave out.
No GPU needed.  Read the strings it prints against vptq_amd/csrc/dequant_paths.h before committing them: the test asserts them.

    python tools/gen_dequant_rows.py"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_instance_census_cpu as census  # noqa: E402
import _dequant_specials as sp  # noqa: E402

DEFAULTS = dict(v=8, k=256, kr=256, C=1, perm=0, S=0, ov=0, norm=1, w_off=0, norm_off=0, idx_off=0, special=0)
NEED5 = (27, 29, 30, 31)


def chosen():
    """(row spec, comment)"""
    Q, T = census._DQ, census.split_bits
    for dt in ("f16", "bf16"):
        for v in census.DQ_VECTOR_LENS:
            yield Q(264, 5 * v - 3, dt, v=v, k=256, kr=256), "TAB 1" + (": 16384 bytes, the limit itself" if v == 16 else "")
            yield Q(264, 5 * v - 3, dt, v=v, k=65536, kr=256), "TAB 2"
            yield Q(264, 5 * v - 3, dt, v=v, k=65536, kr=0), "TAB 0"
    yield Q(264, 77, "f16", v=16, k=512, kr=256), "one step above the limit of both tables: TAB 2"
    yield Q(264, 77, "f16", v=16, k=65536, kr=512), "TAB 2 at its limit"
    yield Q(264, 37, "f16", k=65536, kr=1024), "TAB 2 at its limit, v = 8"
    yield Q(264, 77, "f16", v=16, k=65536, kr=1024), "one step above: TAB 0"
    yield Q(264, 37, "f16", k=256, kr=0), "TAB 1 with an empty residual part"
    yield Q(272, 37, "f16", k=256, kr=256, C=2), "two codebook groups whose tables would fit: TAB 0"
    for t in range(1, 33):
        yield Q(264, 37, "f16", k=T(t)[0], kr=T(t)[1]), f"T = {t}"
    for k, kr in ((256, 16384), (512, 2048)):
        yield Q(264, 37, "f16", k=k, kr=kr), "res_bits > index_bits"
    for t in NEED5:
        yield Q(264, 37, "bf16", k=T(t)[0], kr=T(t)[1]), f"T = {t}: the fifth word, bf16"
        yield Q(264, 77, "f16", v=16, k=T(t)[0], kr=T(t)[1]), f"T = {t}: the fifth word, v = 16"
        yield Q(2056, 37, "f16", k=T(t)[0], kr=T(t)[1]), f"T = {t}: the fifth word, a second column block"
    what = {8: "one chunk, the window would pass the row end", 2040: "one column block, not full", 2048: "exactly one column block",
            2056: "a second column block with one live thread", 1001: "I % 8 != 0: all elem, scalar stores, clamped last column",
            7: "less than one chunk"}
    for kr in (0, 256):
        for I in (8, 2040, 2048, 2056, 1001, 7):
            yield Q(I, 29, "f16", k=65536, kr=kr), what[I]
        for I in (2056, 1001):
            yield Q(I, 29, "bf16", k=65536, kr=kr), what[I]
    cause = ["a permutation", "outlier columns: S = 12, ov = 4", "outlier columns: S = 8, ov = v", "two groups of 136 columns", "four groups of 136 columns",
             "two groups of 132 columns: G % 8 == 4", "four groups of 132 columns", "a permutation, outliers and groups together"]
    for dt, kr in (("f16", 256), ("bf16", 256), ("f16", 0)):
        for (perm, S, ov, C_, I), c in zip(census.DQ_ELEMENT_CAUSES, cause):
            yield Q(I, 37, dt, k=65536, kr=kr, perm=perm, S=S, ov=ov, C=C_), c
    align = ["aligned", "W at + 2 bytes", "scale / bias at + 2 bytes", "indices at + 4 bytes", "no scale / bias"]
    for dt, kr in (("f16", 0), ("bf16", 0), ("f16", 256)):
        for kw, c in zip(census.DQ_ALIGNMENTS, align):
            if kr == 0 or "off" in "".join(kw):
                yield Q(264, 37, dt, k=65536, kr=kr, **kw), c
    for dt in ("f16", "bf16"):
        for (k, kr), c in zip(((16, 16), (65536, 16), (65536, 2048)), ("TAB 1", "TAB 2", "TAB 0, T = 27")):
            yield Q(sp.width(), sp.ROWS * 8, dt, k=k, kr=kr, special=1), "special values, " + c


def cost(e):
    return e["I"] * e["O"] + (e["k"] + e["kr"]) * e["v"]


def line(e, comment):
    kw = ", ".join(f"{key}={e[key]!r}" for key in DEFAULTS if e[key] != DEFAULTS[key])
    return f'    D({e["I"]}, {e["O"]}, "{e["dt"]}",\n      "{e["instance"]}"{", " + kw if kw else ""}),   # {comment}'


def main():
    rows, have = [], set()
    for e, c in chosen():
        e = dict(e, instance=census.dequant_query(e))
        if (e, c) not in rows:
            rows.append((e, c))
        have |= census.dequant_cells_of(e["instance"], e)
    n_chosen = len(rows)
    want = {}
    for e in sorted(census.dequant_grid(), key=cost):
        inst = census.dequant_query(e)
        for cell in census.dequant_cells_of(inst, e):
            want.setdefault(cell, dict(e, instance=inst))
    for cell in sorted(set(want) - have):
        if cell in have:
            continue
        e = want[cell]
        rows.append((e, f"census cell {cell[1]}: {' '.join(cell[2])}"))
        have |= census.dequant_cells_of(e["instance"], e)
    path = os.path.join(ROOT, "tests", "test_dequant_models_gpu.py")
    src = open(path).read()
    body = "# ROWS-BEGIN (tools/gen_dequant_rows.py)\nROWS = [\n" + "\n".join(line(e, c) for e, c in rows) + "\n]\n# ROWS-END"
    src = re.sub(r"# ROWS-BEGIN.*?# ROWS-END", lambda m: body, src, flags=re.S)
    open(path, "w").write(src)
    print(f"{n_chosen} chosen rows + {len(rows) - n_chosen} for census cells they left out; {len(want)} cells")


if __name__ == "__main__":
    main()
