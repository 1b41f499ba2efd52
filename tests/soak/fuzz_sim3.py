#!/usr/bin/env python3
"""Differential soak of the device Sim3Solver (orbs_*) against the restatement (tools/sim3_ref.hpp via
tests/sim3_cases.py): random family, size, scale mode, RANSAC parameters, batch size and iterate step; every hypothesis
and every iterate result equal as bits.  On a machine with the GPU:
    python tests/soak/fuzz_sim3.py [cases] [seed]
Exit code 1 on the first difference (the case is printed)."""
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sim3_cases as sc  # noqa: E402
from orbslamm_amd import ORBmatcher  # noqa: E402
from orbslamm_amd.sim3 import run_all  # noqa: E402


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    rng = np.random.default_rng(seed)
    gm = ORBmatcher(0.9, True, device=0)
    names = sorted(sc.FAMILIES)
    hyps = 0
    t0 = time.time()
    k = 0
    while k < cases:
        batch = int(rng.choice([1, 1, 2, 5, 9]))
        descs, built = [], []
        try:
            for b in range(batch):
                name = str(rng.choice(names))
                over = dict(fix_scale=bool(rng.integers(0, 2)))
                if not name.startswith("n_"):
                    over["n"] = int(rng.choice([3, 4, 5, 19, 63, 64, 65, 100, 257, 1023, 1024, 1025, 2500]))
                    m = int(rng.choice([2, 6, 10, 20]))
                    over["ransac"] = (float(rng.choice([0.9, 0.99, 0.999])), min(m, max(over["n"] - 1, 2)), int(rng.choice([1, 7, 64, 300, 1000])))
                    if name.startswith(("behind", "zero")) and over["n"] < 20:
                        over["n"] = 63
                cs = int(rng.integers(0, 2 ** 31))
                descs.append(dict(case=k + b, family=name, case_seed=cs, seed=seed, **over))
                kw = dict(sc.FAMILIES[name][0])
                kw.update(over)
                case = sc.make_case(np.random.default_rng(cs), **kw)
                dev = sc.device_solver(gm, case)
                built.append((case, dev, sc.case_sets(case, dev.max_iterations, seed=cs % 1000)))
            run_all([d for _, d, _ in built], [s for _, _, s in built])
            step = int(rng.choice([1, 5, 50, 5000]))
            for (case, dev, sets), desc in zip(built, descs):
                sc.compare_solver(dev, case, sets, step, repr(desc))
                hyps += dev.max_iterations
                dev.close()
        except Exception:
            traceback.print_exc()
            print("FAILED", descs)
            return 1
        k += batch
    print("sim3 soak: %d cases, %d hypotheses equal as bits in %.1f s" % (cases, hyps, time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
