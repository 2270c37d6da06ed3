"""The standard-errors example runs end to end on the GPU and prints finite standard errors."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_standard_errors_example(capsys):
    truth, res, out = importlib.import_module("continuous_exponential_standard_hawkes_se").main(duration=1000.0)
    assert out.pd.all() and out.free.all()
    assert np.all(np.isfinite(out.se)) and np.all(out.se > 0) and np.all(out.lower_ci < res.maximizer) and np.all(res.maximizer < out.upper_ci)
    assert np.all(np.abs(res.maximizer - truth) < 6.0 * out.se)          # the estimate is where its standard errors say
    printed = capsys.readouterr().out
    assert "positive definite, column by column: [True, True]" in printed and "nan" not in printed
