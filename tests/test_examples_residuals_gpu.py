"""The goodness-of-fit example runs end to end on the GPU: the fitted process passes its own check, the process without
excitation fails it."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_fit_check_example():
    fitted, flat, res = importlib.import_module("discrete_gaussian_standard_hawkes_fit_check").main(duration=3000)
    assert fitted.pvalue > 0.01 and flat.pvalue < 1e-6
    assert np.all(np.abs(fitted.dispersion - 1.0) < 0.15) and np.all(flat.dispersion > fitted.dispersion)
    assert np.allclose(res.cumulative[:, -1], res.expected, rtol=1e-12) and res.impossible == 0
