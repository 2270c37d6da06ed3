"""The continuous trials example runs end to end on the GPU: three mle! fits, an EM fit and the time-rescaling test, and the fit
on the list of trials is the best of the three on the trials' own log-likelihood."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_continuous_trials_example(nhp, capsys):
    truth, trials, fits, res_em, test = importlib.import_module("continuous_exponential_standard_hawkes_trials").main(ntrials=12, duration=20.0)
    assert len(trials) == 12 and all(len(tr) == 3 and tr[2] == 20.0 for tr in trials)
    assert set(fits) == {"first trial alone", "naive concatenation", "trials"}
    ll = {k: nhp.loglikelihood(p, trials) for k, (p, _, _) in fits.items()}
    slack = 1e-3 * abs(ll["trials"]) ** 0.5                              # the optimizer's stopping rule (f_abstol) leaves this much
    assert ll["trials"] >= ll["naive concatenation"] - slack and ll["trials"] >= ll["first trial alone"] - slack
    assert abs(fits["trials"][1].maximum - ll["trials"]) < 1e-9 * abs(ll["trials"])      # the process holds the estimate
    assert all(np.isfinite(e) for _, _, e in fits.values())
    assert np.isfinite(res_em.maximum) and res_em.maximum >= ll["first trial alone"] - slack
    assert 0.0 <= test.pvalue <= 1.0 and test.counts.sum() == sum(len(tr[0]) for tr in trials)
    printed = capsys.readouterr().out
    assert "naive concatenation" in printed and "time rescaling of the trials" in printed
