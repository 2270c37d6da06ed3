"""The discrete standard-errors example runs end to end on the GPU: every column positive definite, every free parameter
with a finite standard error."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_discrete_standard_errors_example(capsys):
    truth, res, out = importlib.import_module("discrete_gaussian_standard_hawkes_se").main(duration=8000)
    assert out.pd.all() and out.free.any()
    assert np.all(np.isfinite(out.se[out.free])) and np.all(out.se[out.free] > 0) and np.all(np.isnan(out.se[~out.free]))
    f = out.free
    assert np.all(out.lower_ci[f] < res.maximizer[f]) and np.all(res.maximizer[f] < out.upper_ci[f])
    assert np.all(np.isfinite(out.se_W)) and out.se_theta.shape == (3, 3, 3)
    printed = capsys.readouterr().out
    assert "positive definite, column by column: [True, True, True]" in printed and "true values fall inside their intervals" in printed
