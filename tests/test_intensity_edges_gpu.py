"""intensity(process, data, times) held to an exact reference at its edges (csrc/cont_intensity.hip: k_transpose_params,
k_intensity), and total_intensity at the events against the same bound.  Expected values and the per-entry bound come from
tests/compensator_exact_ref.py (intensity_at, event_intensity: long double; the bound is the gradient reference's for λ_i);
tests/test_compensator_edges_host.py ties them to the oracle.  Every (query, child) is compared.

Queries per case (compensator_exact_ref.query_times): 0 and a time before the first event, every tied time, t_j and
t_j + Δtmax with the neighbouring doubles of both for a dozen j (both interval ends are strict), midpoints inside the densest
stretch, every grid point of G-W, T, and T + 5 under a homogeneous baseline.  Cases: the W cases and G-W (N = 7, one
transpose tile), L-exp / L-logit (Δtmax >= T: up to 300 parents), S-tiny, N-70 (three tiles a side, the last ragged, network,
logit-normal) and N-300 (ten tiles a side and a second pass of the child loop: N > NHP_BLOCK = 256).

Largest error/bound seen on an MI355X, intensity(): 0.16 (G-W); W-exp 0.097, W-logit 0.090, W-net 0.087, W-net-logit 0.076,
L-exp 0.066, L-logit 0.042, S-tiny 0.092, N-70 0.062, N-300 0.12.  total_intensity on the exact records: W-exp 0.11, W-logit 0.091;
on the default records W-logit 0.078 and W-exp 0.9996 -- by construction, not by luck: the pair list stores the
delay 0 of a tie as one step δ, the term θ·w·e^{-θδ} then misses its value θ·w by θ·w·(1 - e^{-θδ}) <= δ·θ·(θ·w), and the
allowance δ·Σθ·term is exactly that first-order figure (θ = 2000 on one link with ties).  No kernel defect was found.
"""
import numpy as np
import pytest

import compensator_exact_ref as ce
import cont_grad_ref as gr

pytestmark = pytest.mark.gpu


def data_of(case):
    return (case["times"].copy(), case["nodes"].copy(), case["T"])


@pytest.mark.parametrize("name", ce.INTENSITY_CASES)
def test_every_query_and_child_within_its_bound(nhp, name):
    case, q, lam = ce.prepared_intensity(name)
    proc, data = gr.process_of(nhp, case), data_of(case)
    got = nhp.intensity(proc, data, q)
    assert got.shape == (len(q), case["N"]) and np.all(np.isfinite(got))
    ratio, bad = ce.check_intensity(got, lam)
    print(f"{name}: Q {len(q)}, largest K {int(lam.K.max())}: error/bound {ratio:.3g}")
    assert len(bad) == 0, f"{name}: {len(bad)} (query, child) outside the bound, the first {bad[:8].tolist()}, q = {q[bad[:8, 0]].tolist()}"
    # the order of the queries and duplicates do not matter, to the bit
    rng = np.random.default_rng(3)
    pick = np.concatenate([rng.permutation(len(q)), rng.integers(0, len(q), 17)])
    again = nhp.intensity(proc, data, q[pick])
    assert np.array_equal(again.view(np.int64), got[pick].view(np.int64))
    # Q = 1 and the scalar form
    mid = len(q) // 2
    one = nhp.intensity(proc, data, q[mid:mid + 1])
    assert one.shape == (1, case["N"]) and np.array_equal(one[0].view(np.int64), got[mid].view(np.int64))
    scalar = nhp.intensity(proc, data, float(q[mid]))
    assert scalar.shape == (case["N"],) and np.array_equal(scalar.view(np.int64), got[mid].view(np.int64))


@pytest.mark.parametrize("name", ["W-exp", "W-net-logit", "G-W"])
def test_empty_dataset_and_no_query(nhp, name):
    case = ce.case_of(name)
    proc = gr.process_of(nhp, case)
    m = gr.model_of(case)
    empty = (np.zeros(0), np.zeros(0, dtype=np.int64), case["T"])
    q = np.array([0.0, 0.5 * case["T"], case["T"]])
    got = nhp.intensity(proc, empty, q)
    lam = ce.intensity_at(m, empty[0], empty[1], q)
    ratio, bad = ce.check_intensity(got, lam)
    assert got.shape == (3, case["N"]) and len(bad) == 0 and np.all(lam.K == 0)
    if case["grid_x"] is None:
        assert np.array_equal(got, np.tile(case["lam0"], (3, 1)))
    none = nhp.intensity(proc, data_of(case), np.zeros(0))
    assert none.shape == (0, case["N"])


@pytest.mark.parametrize("name", ["W-exp", "G-W"])
def test_domain_errors_leave_the_output_untouched(nhp, name):
    from nhp_amd import _lib, continuous
    case = ce.case_of(name)
    proc, data = gr.process_of(nhp, case), data_of(case)
    ctx = nhp.default_context()
    bad = [np.array([1.0, -1.0])] if case["grid_x"] is None else [np.array([1.0, -1.0]), np.array([1.0, np.nextafter(case["T"], np.inf)])]
    for q in bad:
        with pytest.raises(nhp.DomainError):
            nhp.intensity(proc, data, q)
        ds, model = continuous.device_dataset(proc, data, ctx), proc.device_model(ctx)
        out = np.full((case["N"], len(q)), np.nan)
        rc = _lib.lib().nhp_cont_intensity(ctx.h, ds.h, model.h, _lib.dptr(q), len(q), _lib.dptr(out))
        assert rc == _lib.EDOMAIN and np.all(np.isnan(out))
    if case["grid_x"] is not None:                                      # the support's two ends themselves are inside
        assert np.all(np.isfinite(nhp.intensity(proc, data, np.array([0.0, case["T"]]))))


EXACT = {"NHP_PLIST": "0", "NHP_EV8": "0"}                               # the exact 16-byte records (test_cont_grad_edges_gpu.py)


@pytest.mark.parametrize("name", ["W-exp", "W-logit"])
def test_total_intensity_at_the_events(nhp, monkeypatch, name):
    """The bound of intensity_at holds on the exact records.  The default route of the exponential kind reads the 8-byte pair
    list, whose delays are rounded to Δtmax·2⁻⁴⁸ (a tie moves by one whole step): δ·Σθ·term is added there, as the gradient
    suite adds its δ·Q.  The logit-normal route reads exact delays either way."""
    case, lam = ce.prepared_events(name)
    proc = gr.process_of(nhp, case)
    try:
        for env, delta in ((EXACT, 0.0), ({}, case["dt_max"] * 2.0 ** -48 if case["kind"] == "exponential" else 0.0)):
            for k in EXACT:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            nhp.invalidate_device_datasets()
            got = nhp.total_intensity(proc, data_of(case))
            ratio, bad = ce.check_intensity(got, lam, delta)
            print(f"{name} {'exact records' if env else 'default records'}: total_intensity error/bound {ratio:.3g}")
            assert len(bad) == 0, f"{name} {env}: events {bad[:8].ravel().tolist()} outside the bound"
    finally:
        monkeypatch.undo()
        nhp.invalidate_device_datasets()
