"""Child process of test_chain_rows_gpu.py: runs its chains with the persistent launch forced into the rows geometry
(VPTQ_K256C_ROWS=1 and VPTQ_K256C_WGS, read once per process, set by the parent) and writes every output to an .npz; the
parent does the checking.

    python tests/_chain_rows_run.py OUT.npz"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

EXACT, MFMA = 1 << 2, 1 << 3
# (I, O, bias).  "switch" at 4 workgroups: 13 workgroup-tasks - 3 or 4 per workgroup, workgroup 0 walks four layers (both image
# buffers reused in both directions), layer 4 gives three workgroups one task and one two (the next task of the same layer);
# vector-rows that are no multiple of 8 or of 128, O no multiple of 8, idle waves in most layers' last task; widths of one step
# (128), columns past G (136, 2056), many steps (4096), different widths following each other.  "few": 3 tasks, so one of 4
# workgroups returns at once.
CHAINS = {
    "switch": [(128, 2100, True), (136, 1100, False), (2056, 520, True), (4096, 264, False), (136, 4100, False), (128, 1004, True)],
    "few": [(2056, 264, False), (128, 1100, True)],
}
SPECIAL_COLS, PERIOD, TAIL = 2040, 1856, 64   # the special-value table: 2040 columns (16 steps, the last one short)


def layer_of(chain, i):
    from oracle import vptq_oracle as vo
    I, O, bias = CHAINS[chain][i]
    return vo.make_layer(I, O, dist="llm", seed=31 * i + I + O, dtype="f16", bias=bias)


def x_of(chain, i):
    import test_route_models_gpu as rm
    return rm._dense(CHAINS[chain][i][0], 1, "f16", 100 + i)[0]


def special_layer():
    import _dequant_specials as sp
    return sp.special_layer("f16", 8, 256, 256, finite=True, cols=SPECIAL_COLS)


def special_features():
    import numpy as np
    return np.concatenate([np.arange(PERIOD), np.arange(SPECIAL_COLS - TAIL, SPECIAL_COLS)])


def main(argv):
    import numpy as np
    import torch
    from vptq_amd import _backend as B
    from _gpu_util import spec_to_module, module_desc, bits_to_tensor, tensor_to_bits, gemv_abi
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lib = B.lib()
    out = {}

    def chain_call(descs, n, xs, ys, flags):
        xp = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
        yp = (C.c_void_p * n)(*[y.data_ptr() for y in ys])
        B.check(lib.vptq_quant_gemv_chain(descs, n, xp, yp, 1, flags, None, 0, B.current_stream_ptr(dev)), "vptq_quant_gemv_chain")

    def instance(descs, n, flags):
        buf = C.create_string_buffer(4096)
        B.check(lib.vptq_quant_gemv_chain_instance(descs, n, 1, flags, buf, len(buf)), "vptq_quant_gemv_chain_instance")
        return buf.value.decode()

    for chain, shapes in CHAINS.items():
        n = len(shapes)
        mods = [spec_to_module(layer_of(chain, i), dev) for i in range(n)]
        keep = [module_desc(m) for m in mods]
        descs = (B.LayerDesc * n)(*[k[0] for k in keep])
        xs = [bits_to_tensor(x_of(chain, i), "f16", dev).reshape(-1) for i in range(n)]
        ys = [torch.full((shapes[i][1],), float("nan"), dtype=torch.float16, device=dev) for i in range(n)]
        out[f"{chain}.instance"] = np.array(instance(descs, n, EXACT | MFMA))
        chain_call(descs, n, xs, ys, EXACT | MFMA)
        torch.cuda.synchronize()
        first = [tensor_to_bits(y) for y in ys]
        chain_call(descs, n, xs, ys, EXACT | MFMA)                    # again into the same buffers
        torch.cuda.synchronize()
        second = [tensor_to_bits(y) for y in ys]
        other = [torch.empty_like(y) for y in ys]
        out[f"{chain}.folded_instance"] = np.array(instance(descs, n, MFMA))
        chain_call(descs, n, xs, other, MFMA)                         # a launch of gemv_k256c_kernel (the folded form) ...
        chain_call(descs, n, xs, ys, EXACT | MFMA)                    # ... and the rows geometry behind it
        torch.cuda.synchronize()
        third = [tensor_to_bits(y) for y in ys]
        for i in range(n):
            out[f"{chain}.y.{i}"], out[f"{chain}.again.{i}"], out[f"{chain}.after.{i}"] = first[i], second[i], third[i]
            # one launch per layer in the reference's roundings
            out[f"{chain}.single.{i}"] = tensor_to_bits(gemv_abi(mods[i], xs[i].reshape(1, 1, -1), EXACT | MFMA)).reshape(-1)

    # W through one-hot activations: 32 copies of the special-value layer per launch, one column each
    L = special_layer()
    m = spec_to_module(L, dev)
    desc, keep1 = module_desc(m)
    per = 32
    descs = (B.LayerDesc * per)(*([desc] * per))
    out["special.instance"] = np.array(instance(descs, per, EXACT | MFMA))
    feats = special_features()
    padded = np.concatenate([feats, np.repeat(feats[-1:], (-len(feats)) % per)])
    x = torch.zeros(len(padded), L.in_features, dtype=torch.float16, device=dev)
    x[torch.arange(len(padded), device=dev), torch.from_numpy(padded).to(dev)] = 1.0
    y = torch.full((len(padded), L.out_features), float("nan"), dtype=torch.float16, device=dev)
    for j in range(0, len(padded), per):
        chain_call(descs, per, [x[j + i] for i in range(per)], [y[j + i] for i in range(per)], EXACT | MFMA)
    torch.cuda.synchronize()
    out["special.columns"] = tensor_to_bits(y[:len(feats)])
    out["special.W"] = tensor_to_bits(m.dequant())
    np.savez(argv[0], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
