"""The trials example runs end to end on the GPU: three fits, and the fit on the list of trials is the best of the three on
the trials' own log-likelihood (the objective is concave, so its maximum is the global one)."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_discrete_trials_example(nhp, capsys):
    truth, trials, fits = importlib.import_module("discrete_gaussian_standard_hawkes_trials").main(ntrials=8, bins=400)
    assert len(trials) == 8 and all(x.shape == (3, 400) for x in trials)
    assert set(fits) == {"first trial alone", "naive concatenation", "trials"}
    ll = {k: nhp.loglikelihood(p, trials) for k, (p, _, _) in fits.items()}
    slack = 1e-3 * abs(ll["trials"]) ** 0.5
    assert ll["trials"] >= ll["naive concatenation"] - slack and ll["trials"] >= ll["first trial alone"] - slack
    assert abs(fits["trials"][1].maximum - ll["trials"]) < 1e-9 * abs(ll["trials"])      # the process holds the estimate
    assert all(np.isfinite(e) for _, _, e in fits.values())
    assert fits["trials"][2] < fits["first trial alone"][2]                               # eight trials say more than one
    printed = capsys.readouterr().out
    assert "naive concatenation" in printed and "W fitted on the trials" in printed
