#!/usr/bin/env python3
"""Differential soak of the device PnPsolver (orbp_*) against the restatement (tools/pnp_ref.hpp via tests/pnp_cases.py):
random family, size, RANSAC parameters, batch size and iterate step; every hypothesis (count, pose, record flag, Refine's
count, flag and pose) and every iterate result equal as bits.  On a machine with the GPU:
    python tests/soak/fuzz_pnp.py [cases] [seed]
Exit code 1 on the first difference (the case is printed)."""
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnp_cases as pc  # noqa: E402
from orbslamm_amd import ORBmatcher  # noqa: E402
from orbslamm_amd.pnp import EXTRA_SETS, run_all  # noqa: E402


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    rng = np.random.default_rng(seed)
    gm = ORBmatcher(0.9, True, device=0)
    names = sorted(pc.FAMILIES)
    hyps = 0
    t0 = time.time()
    k = 0
    while k < cases:
        batch = int(rng.choice([1, 1, 2, 5, 9]))
        step = int(rng.choice([1, 5, 50]))
        descs, built = [], []
        try:
            for b in range(batch):
                name = str(rng.choice(names))
                over = {}
                if not name.startswith("n_"):
                    over["n"] = int(rng.choice([4, 5, 19, 63, 64, 65, 100, 257, 2047, 2048, 2049, 5000]))
                    over["ransac"] = (float(rng.choice([0.9, 0.99, 0.999])), int(rng.choice([4, 8, 10, 20])), int(rng.choice([1, 7, 64, 300, 1000])),
                                      4, float(rng.choice([0.05, 0.2, 0.4, 0.5])), float(rng.choice([5.991, 9.21])))
                    if name == "behind_camera" and over["n"] < 20:
                        over["n"] = 63
                cs = int(rng.integers(0, 2 ** 31))
                descs.append(dict(case=k + b, family=name, case_seed=cs, seed=seed, step=step, **over))
                kw = dict(pc.FAMILIES[name][0])
                kw.update(over)
                case = pc.make_case(np.random.default_rng(cs), **kw)
                dev = pc.device_solver(gm, case)
                built.append((case, dev, pc.case_sets(case, dev.max_iterations + max(EXTRA_SETS, step), seed=cs % 1000)))
            run_all([d for _, d, _ in built], [s for _, _, s in built])
            for (case, dev, sets), desc in zip(built, descs):
                pc.compare_solver(dev, case, sets, step, repr(desc))
                hyps += len(dev.hypotheses())
                dev.close()
        except Exception:
            traceback.print_exc()
            print("FAILED", descs)
            return 1
        k += batch
    print("pnp soak: %d cases, %d hypotheses equal as bits in %.1f s" % (cases, hyps, time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
