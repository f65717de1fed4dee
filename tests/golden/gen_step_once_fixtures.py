"""Writes tests/golden/step_once_steps.npz: what StepOracle.step_once returns for the two cases of tests/step_rhs.golden_step_cases, two steps each.
Recorded before step_once was split into form_function + the solve; tests/test_step_rhs.py asserts that the split changed no bit.
Run from the repository root: python tests/golden/gen_step_once_fixtures.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import step_rhs as sr  # noqa: E402

if __name__ == "__main__":
    out = {}
    for name in sr.golden_step_cases():
        out.update(sr.run_golden_steps(name))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_once_steps.npz")
    np.savez_compressed(path, **out)
    print(path, {k: v.shape for k, v in out.items() if k.endswith("_its") or k.endswith("_v")}, {k: v for k, v in out.items() if "its" in k or "rnorm" in k})
