"""Child process of test_chain_schedule_gpu.py: runs seeded chains (tests/_chain_schedule.py) under the workgroup count the
parent put in VPTQ_K256C_WGS (read once per process) and writes every output to an .npz; the parent does the checking.

    python tests/_chain_schedule_run.py OUT.npz chain:dtype:arith ..."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv):
    import numpy as np
    import torch
    import _chain_schedule as cs
    assert torch.cuda.is_available(), "needs a GPU"
    jobs = [tuple(j.split(":")) for j in argv[1:]]
    out = cs.run_jobs(jobs, torch.device("cuda", 0))
    np.savez(argv[0], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
