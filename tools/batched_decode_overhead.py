"""Python time of `VQuantLinear.forward` on the batched-decode path and on the one-token path in front of which it stands:
us per call to ENQUEUE (the loop's wall time before the one synchronize) of

  * 1 token of an 8192 x 8192 canonical layer (v8-k256-256): the decode call, which pays the batched-decode guard and nothing else;
  * 12 and 24 tokens of a small v8-k65536-256 layer (2048 -> 512: the kernel is shorter than the Python in front of it) with the
    knobs of `gemm_gather` and `gemm_gatherw` at "1";
  * 1 and 3 tokens of another such layer over its sliced layout (`enable_sliced_layout()`, the one-launch knob at "1"): the path
    of `_gemv_cached` in front of the gather kernels.

    python tools/batched_decode_overhead.py [--tree DIR] [--calls 2000] [--reps 7]

--tree DIR: import `vptq_amd` from DIR (another checkout with its library built) instead of this one, to compare two commits in
one session on one box.  Prints one JSON line per case: median, least and largest of --reps loops.
"""
import argparse, json, os, statistics, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--calls", type=int, default=2000)
ap.add_argument("--reps", type=int, default=7)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree)); sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "tools"))
import torch  # noqa
import vptq_amd  # noqa
from shape_bench import mk  # noqa
try:
    from vptq_amd import batched_decode as rules   # the home of the knobs
except ImportError:
    from vptq_amd.layers import vqlinear as rules  # (a checkout from before that module)
rules._GEMM_GATHER_MODE = rules._GEMM_GATHERW_MODE = "1"
try:
    from vptq_amd import sliced_routes as sliced_rules   # the home of the sliced-route knobs
except ImportError:
    from vptq_amd.layers import vqlinear as sliced_rules  # (a checkout from before that module)
sliced_rules._SLICED_ONE_LAUNCH = "1"

dev = torch.device("cuda", 0); g = torch.Generator(device=dev).manual_seed(0)
cases = [("v8-k256-256 8192x8192", mk(8192, 8192, dev, g), 1)]
big = mk(2048, 512, dev, g, k=65536, kr=256)
cases += [("v8-k65536-256 2048x512", big, 12), ("v8-k65536-256 2048x512", big, 24)]
sliced = mk(2048, 512, dev, g, k=65536, kr=256)
sliced.enable_sliced_layout()
cases += [("v8-k65536-256 2048x512 sliced", sliced, 1), ("v8-k65536-256 2048x512 sliced", sliced, 3)]
with torch.no_grad():
    for name, m, tokens in cases:
        x = torch.randn(1, tokens, m.in_features, device=dev, dtype=torch.float16)
        for _ in range(200):
            m(x)
        torch.cuda.synchronize()
        enq, tot = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                m(x)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            enq.append((t1 - t0) / a.calls * 1e6); tot.append((t2 - t0) / a.calls * 1e6)
        print(json.dumps(dict(tree=os.path.abspath(a.tree), vptq_amd=os.path.dirname(vptq_amd.__file__), layer=name, tokens=tokens,
                              enqueue_us=round(statistics.median(enq), 2), enqueue_min=round(min(enq), 2), enqueue_max=round(max(enq), 2),
                              with_drain_us=round(statistics.median(tot), 2))), flush=True)
