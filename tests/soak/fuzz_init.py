#!/usr/bin/env python3
"""Differential soak of the device Initializer (orbi_*) against the restatement (tools/init_ref.hpp via
tests/init_cases.py): random scene family, size, iterations, sigma, intrinsics, noise, outlier rate, model and seed;
every output and diagnostic equal as bits, and the float64 geometric check (init_cases.check_result) on the device's
result.  On a machine with the GPU:
    python tests/soak/fuzz_init.py [cases] [seed]
Exit code 1 on the first difference (the case is printed)."""
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import init_cases as ic  # noqa: E402
from orbslamm_amd import ORBmatcher  # noqa: E402
from orbslamm_amd.initializer import Initializer  # noqa: E402


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    rng = np.random.default_rng(seed)
    gm = ORBmatcher(0.9, True, device=0)
    counts = {}
    t0 = time.time()
    for k in range(cases):
        family = str(rng.choice(ic.FAMILIES))
        variant = str(rng.choice(list(ic.VARIANTS)))
        n = int(rng.choice([8, 9, 31, 64, 127, 128, 129, 200, 255, 256, 257, 300, 511, 513, 1000, 2500]))
        iterations = int(rng.choice([1, 8, 31, 32, 33, 64, 200, 257, 1000]))
        sigma = float(rng.choice([0.5, 1.0, 1.0, 2.0]))
        K = ic.K_TUM if rng.integers(0, 2) else np.array([rng.uniform(400, 800), rng.uniform(400, 800), rng.uniform(300, 340),
                                                          rng.uniform(220, 260)], np.float32)
        noise = None if rng.integers(0, 3) else float(rng.uniform(0.0, 1.5))
        model = str(rng.choice(["HF", "F"]))
        case_seed = int(rng.integers(0, 2 ** 31))
        desc = dict(case=k, family=family, variant=variant, n=n, iterations=iterations, sigma=sigma, K=[float(v) for v in K], noise=noise,
                    model=model, case_seed=case_seed, seed=seed)
        try:
            crng = np.random.default_rng(case_seed)
            case = ic.make_case(family, crng, variant, n_match=n, K=K, noise=noise)
            # (the suite's noiseless expectations are for its sizes, iterations and intrinsics: here only the rotation-only
            # and collapsed families keep theirs, and the model a noiseless scene picks with 100 matches and 32 sets)
            case["succeeds"] = False
            if noise is not None or n < 100 or iterations < 32:
                case["expect"] = None if case["expect"] in ("H", "F") else case["expect"]
            sets = ic.random_sets(crng, int((case["m12"] >= 0).sum()), iterations)
            ini = Initializer(gm, case["keys1"], case["K"], sigma=sigma, iterations=iterations, model=model)
            got = ini.initialize(case["keys2"], case["m12"], sets)
            ini.close()
            want = ic.ref_initialize(case["keys1"], case["keys2"], case["m12"], sets, K=case["K"], sigma=sigma, model=model)
            ic.assert_equal_results(got, want)
            ic.check_result(case, got, sigma=sigma, model=model)
        except AssertionError:
            traceback.print_exc()
            print("DIFFERENCE:", desc)
            return 1
        for o in ic.outcomes(got):
            counts[o] = counts.get(o, 0) + 1
    print("init soak: %d cases (seed %d), device against the restatement and the float64 check -- all outputs equal; "
          "outcomes %s; %.0f s" % (cases, seed, dict(sorted(counts.items())), time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
