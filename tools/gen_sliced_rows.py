"""Rewrites the ROWS table of tests/test_route_models_sliced_gpu.py in place: a greedy cover of the cells
tests/test_instance_census_cpu.py enumerates for the sliced kernels, cheapest layers first (weights x tokens).  No GPU: candidates and
cells come from vptq_quant_gemv_sliced_instance / _tokens_instance over fake descriptors, as the census does.

    python tools/gen_sliced_rows.py

A census cell without a row (a new view, a new shape class): add the view or the grid point there and rerun this."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_instance_census_cpu as cs  # noqa: E402

want = cs.enumerate_sliced_cells()
print("cells", len(want), file=sys.stderr)
for k in cs.SLICED_KERNELS:
    for dt in cs.DTYPES:
        print(k, dt, len({c for kk, v, c in want if kk == k and v == 0 and c[0] == dt}), file=sys.stderr)

cands = []
for dt in cs.DTYPES:
    for v in (8, 16):
        for k, krs in ((65536, cs.KR_CLASSES), (32768, (0, 256)), (16384, (0, 256))):
            for kr in krs:
                for I in cs.SLICED_WIDTHS:
                    for perm in (False, True):
                        for mode in ("folded", "exact", "sel"):
                            for Os in ([(72,), (264,), (8200,), (264, 72), (264, 72, 8200)]):
                                if perm and (Os[0] == 8200 or len(Os) == 2):
                                    continue
                                for tokens in range(1, 9):
                                    if tokens > 1 and mode == "sel":
                                        continue
                                    inst = cs.sliced_query(I, Os, dt, tokens, mode, v, k, kr, perm)
                                    if not inst:
                                        continue
                                    ent = cs.entry_of(Os, "single", inst)
                                    cells = cs.sliced_cells_of(inst, tokens, ent, k, kr)
                                    entry = ent
                                    if len(Os) == 1 and mode != "sel" and ent == "single":
                                        cells = cells | cs.sliced_cells_of(inst, tokens, "grouped", k, kr)
                                        entry = "both"
                                    cost = I * sum(Os) * (1 + 0.15 * tokens)
                                    cands.append((cost, dict(I=I, Os=Os, dt=dt, tokens=tokens, mode=mode, instance=inst, v=v, k=k, kr=kr,
                                                             perm=int(perm), rpw=0, entry=entry), cells))
        for rpw in (2, 18):
            for mode in ("folded", "exact"):
                inst = cs.sliced_query(1024, (264,), dt, 1, mode, v, rpw=rpw)
                cands.append((1024 * 264, dict(I=1024, Os=(264,), dt=dt, tokens=1, mode=mode, instance=inst, v=v, k=65536, kr=0, perm=0, rpw=rpw,
                                               entry="single"), cs.sliced_cells_of(inst, 1, "single")))
print("cands", len(cands), file=sys.stderr)
rows = []
missing = set(want)
cands.sort(key=lambda c: c[0])
while missing:
    # the rarest missing cell first: the cheapest candidate that covers it, ties by how much else it covers
    best = None
    for cost, e, cells in cands:
        gain = len(cells & missing)
        if not gain:
            continue
        score = gain / cost
        if best is None or score > best[0]:
            best = (score, cost, e, cells)
    if best is None:
        sys.exit(f"no candidate covers {sorted(missing)[:20]}")
    rows.append(best[2])
    missing -= best[3]
print("rows", len(rows), "weights", sum(e["I"] * sum(e["Os"]) for e in rows) / 1e6, "M", file=sys.stderr)
rows.sort(key=lambda e: (e["instance"].split()[0], e["dt"], e["v"], e["k"], e["kr"], e["I"], e["Os"], e["perm"], e["mode"], e["tokens"]))
text = []
for e in rows:
    Os = e["Os"][0] if len(e["Os"]) == 1 else e["Os"]
    opt = "".join(f", {k}={e[k]!r}" for k, d in (("v", 8), ("k", 65536), ("kr", 0), ("perm", 0), ("rpw", 0), ("entry", "single")) if e[k] != d)
    # fp16 with the 256-entry residual table of v = 8, folded part: one packed add f16(c + r) (gemv_sliced.hip) - the `rounded` model
    if e["mode"] != "exact" and e["dt"] == "f16" and e["v"] == 8 and e["kr"] == 256 and e["instance"].split(" | ")[-1].startswith("gemv_sliced "):
        opt += ", rounded=1"
    bias = ", bias=1" if (e["I"] // 8 + e["Os"][0] // 8 + e["v"] // 8 + (e["kr"] > 0) + e["perm"]) % 2 == 0 else ""
    text.append(f'    S({e["I"]}, {Os}, "{e["dt"]}", {e["tokens"]}, "{e["mode"]}",\n      "{e["instance"]}"{opt}{bias}),\n')
path = os.path.join(ROOT, "tests", "test_route_models_sliced_gpu.py")
src = open(path).read()
new, n = re.subn(r"(?ms)^ROWS = \[\n.*?^\]\n", lambda m: "ROWS = [\n" + "".join(text) + "]\n", src)
assert n == 1, "ROWS = [ ... ] not found once"
open(path, "w").write(new)
