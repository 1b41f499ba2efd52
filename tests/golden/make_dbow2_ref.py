#!/usr/bin/env python3
"""Regenerates tests/golden/dbow2_ref.npz.

PROVENANCE: the outputs of the REFERENCE's own DBoW2::BowVector / DBoW2::FeatureVector object code
(oracle/_ref/libdbow2_ref.so, oracle/Makefile target _ref, built from the reference checkout) for exactly the calls
tests/test_oracle_vs_reference_cpu.py makes.  The tests are run once against the live library with every call
written down; inputs are regenerated from seeds by the tests, only outputs are stored, keyed by a digest of the
inputs.  Needs the library: `make -C oracle _ref` where the reference checkout exists."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]
from oracle import binding as ob  # noqa: E402
import test_oracle_vs_reference_cpu as t  # noqa: E402


def main():
    ob.build()
    if ob.ref_lib() is None:
        sys.exit("oracle/_ref/libdbow2_ref.so is not built: run `make -C oracle _ref` where the reference checkout exists")
    rec = t.RecordedRef(ob, record=True)
    for weighting in (0, 1, 2, 3):
        for scoring in (0, 1, 2, 3, 4, 5):
            t.test_transform_assembly_equals_reference_object_code(rec, scoring, weighting)
    for norm in (1, 2):
        t.test_summation_order_matters_and_is_the_references(rec, norm)
    t.test_add_if_not_exist_keeps_the_first_weight(rec)
    np.savez_compressed(t.GOLDEN, **rec.calls)
    print("wrote %s: %d arrays, %d bytes" % (t.GOLDEN, len(rec.calls), os.path.getsize(t.GOLDEN)))


if __name__ == "__main__":
    main()
