"""nhp_cont_loglik_grad held to an exact reference at its edges, route by route (csrc/cont_grad.hip: k_grad_init,
k_grad_windowed<IMP,G,TH>, k_grad_recursive_waves<PQ,H>, grad_lgcp_scatter; csrc/cont_slices.hip: k_windowed_slices<..,GRAD>).
The expected gradient, its scales and the per-entry bound come from tests/cont_grad_ref.py (long double; the bound's derivation
is in its docstring); tests/test_cont_grad_host.py ties that restatement to the definitions and shows by a census that the
inputs contain what the cases are named for.  Every entry is compared: |g - g_ref| <= bound, and an entry without a single pair
equals its parameter-independent term exactly.  The log-likelihood keeps the suite's 1e-11.

    W-exp, W-logit, W-net   N=7 M=3000 T=200 Δtmax=1, times on a dyadic grid: ties, pairs at Δ = Δtmax exactly (not pairs), a
    (W-net-logit besides)   burst of 90 events in 0.6, node 7 empty, node 6 with one event, node 5 outside every other column's
                            windows (the != 0 guards), W with exact zeros, A with a zero row and a zero column and W = 0 under
                            A = 1, θΔtmax from 0.5 to 40 and one of 2000 whose exponential flushes, x = 2⁻⁴¹ and 1 - 2⁻⁴¹ under
                            μ = -28 / +28.  Two-pass route with the exact records for NHP_GROUP = 1..64 (δ = 0), once with pass A
                            on the 8-byte pair list (δ = Δtmax·2⁻⁴⁸); slice route for all 15 (BLOCK, C).
                            Size adjusted for the route: with the default items of 32 children the build does not keep slices at
                            N = 7 (rows·64 = 160 896 > 2·pairs + 4096 = 102 218), so the slice runs set NHP_CHUNK=256: 16 items,
                            two or more per node, one with a single child, one without children; all_sole = 0.
    D                       N=3 M=900, NHP_CHUNK=4096: one item per node, all_sole = 1: the slices store every entry themselves,
                            the empty node's column as constants only; two builds give the same bits; the two-pass route too
    L-exp, L-logit          N=2 M=600 Δtmax=64 >= T: 179 700 pairs in 20 items, 8985 per item >= 4096: TH = 512
    R-1 .. R-1025           the full recursion (LL_RECURSIVE | LL_FULL_RECURSION) in the shapes 1x1, 1x1, 1x2, 2x4, 4x4, 4x8; M = 1500
                            (N = 1: 1.1e6 pairs), 2500, 2000; three events at t = 0, ties, node 2 without events, N = 257: nodes
                            129..256 without events (a part none of whose nodes has events), a network mask from N = 64 on.
                            Shape 4x16 (N > 2048) is left out: 8.4e6 entries and as many pair sums do not fit a few seconds.
    C, C-net                the data of test_recursive_through_the_truncated_window_matches_the_recursion (standard and network
                            process: the window's k_grad_init must NOT mask the integral) against the FULL-history
                            restatement, + the 2⁻⁶⁰ tail.  The route is asserted through nhp_probe_recursive_window: θ in [20, 40]
                            with 10 events per unit time puts the cut near 2 and the window's cost below the recursion's
    G-W, G-D, G-R           a non-uniform grid of 5 points under W-exp (two-pass and slices), D (slices, not direct: the grid block
                            is accumulated) and R-65; events on grid points, in the last cell, at t = x[4] = T
    S                       W-exp (both routes) and R-65 as column shards [0,3) + [3,N) and the single column [2,3): foreign
                            entries exactly 0.0, the shards' sum inside the whole's bound

The two-pass route's 160 KiB refusal (N > 5100) is left out: its gradient has 2·N² = 5e7 entries, 400 MB.

Largest error/bound seen on an MI355X: 0.22 (R-513; the float64 host evaluation reaches 0.14 there); case by case, next to the
host's figures, in DESIGN.md 3.1e.

Mistakes planted in scratch builds (arithmetic only, one build each, every route's copy of the line), and the cases that went
red on an MI355X (error/bound 1e13 to 3e14, or a constant entry that differs):
    (1 - θΔ) -> (1 + θΔ)                       W-exp W-net (two-pass and slices) D L-exp R-1 R-64 R-65 R-257 C C-net G S
    the 0.5/τ factor dropped                    W-logit W-net-logit L-logit
    k_grad_init never masks the integral        W-net W-net-logit (two-pass) W-net (slices)
    k_grad_init always masks the integral       C-net (the truncated window's W entries under A = 0: 0.0 where -cnt belongs)
    the baseline's share from every wave        G (G-R: 1x2, the grid block gets every g twice).  With a homogeneous baseline
    of the recursion (`h == 0` dropped)         the line cannot matter: only thread 0 stores gsum, and it is in wave 0
    the two LGCP interpolation weights swapped  G (G-W on both routes)
    gap·S dropped from the R update             R-1 R-64 R-65 R-257 G (G-R) S (R-65)
    av dropped from the W entry                 W-net W-net-logit (two-pass) W-net (slices) R-64 R-65 R-257 C-net G (G-R) S (R-65)
(R-513 and R-1025 were not part of the planted runs.)
"""
import ctypes as C

import numpy as np
import pytest

import cont_grad_ref as cr
from helpers import window_routes

pytestmark = pytest.mark.gpu

REL_LL = 1e-11
ROUTE_ENV = ("NHP_GRAD_SLICES", "NHP_PLIST", "NHP_EV8", "NHP_GROUP", "NHP_CHUNK", "NHP_SLICES_CFG", "NHP_SLICES", "NHP_SLICES_LN",
             "NHP_XCD", "NHP_SORT")
EXACT = {"NHP_GRAD_SLICES": "0", "NHP_PLIST": "0", "NHP_EV8": "0"}       # the two-pass route on the 16-byte records
FULL = 3                                                                  # LL_RECURSIVE | LL_FULL_RECURSION
SLICE_CFGS = ["%d,%d" % (b, c) for b in (64, 128, 256, 512, 1024) for c in (2, 4, 8)]
REC_SHAPE = {1: (1, 1), 64: (1, 1), 65: (1, 2), 257: (2, 4), 513: (4, 4), 1025: (4, 8)}


@pytest.fixture
def route(monkeypatch, nhp):
    """Sets the route switches for one evaluation and builds the dataset anew; everything is cleared afterwards."""
    def use(env):
        for k in ROUTE_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        nhp.invalidate_device_datasets()
    yield use
    for k in ROUTE_ENV:
        monkeypatch.delenv(k, raising=False)
    nhp.invalidate_device_datasets()


def gradient(nhp, case, P, flags=0, columns=None):
    """(ll, grad, scalars) of nhp_cont_loglik_grad on a freshly built dataset."""
    from nhp_amd import _lib, continuous
    assert _lib.LL_RECURSIVE | _lib.LL_FULL_RECURSION == FULL
    proc = cr.process_of(nhp, case)
    ctx = nhp.default_context()
    data = (case["times"], case["nodes"], case["T"])
    ds = continuous.DeviceDataset(ctx, data, case["N"], case["dt_max"], columns=columns)
    model = proc.device_model(ctx)
    g, ll = np.full(P, np.nan), C.c_double()
    _lib.check(_lib.lib().nhp_cont_loglik_grad(ctx.h, ds.h, model.h, flags, C.byref(ll), _lib.dptr(g), P), ctx.h)
    return ll.value, g, ds.scalars()


def hold(label, got_ll, got, res, N, delta=0.0, tail=None):
    assert abs(got_ll - float(res.ll)) <= REL_LL * abs(float(res.ll)), (label, got_ll, float(res.ll))
    ratio, bad, err, B = cr.check(got, res, delta, tail)
    print(f"{label}: error/bound {ratio:.3g}, {int((B == 0).sum())} entries equal to their constant")
    assert len(bad) == 0, f"{label}: {len(bad)} entries outside the bound\n" + cr.explain(got, res, N, bad, err, B)
    return ratio


def bit_length(v):
    return int(v).bit_length()


def slice_step(case, sc):
    """δ of the 6-byte records: the child slices keep 48 - bit_length(N) bits of Δtmax, the parent slices
    48 - bit_length(max_item) (cont_data.hip: nhp_cont_slices_keep; cont_slices.hip: ensure_parent_slices)."""
    assert sc["sl_nb"] == bit_length(case["N"])
    return case["dt_max"] * 2.0 ** -(48 - max(sc["sl_nb"], bit_length(sc["max_item"])))


def two_pass_preconditions(case, sc, group, th):
    """nhp_grad_enqueue's last branch: items exist, the group width is the one asked for, the column fits the 160 KiB, and
    pairs per item select TH."""
    N, expo = case["N"], case["kind"] == "exponential"
    assert sc["n_items"] > 0 and sc["pairs"] > 0
    assert group is None or sc["group"] == group
    assert 64 + 16 * N + 8 * N * (2 if expo else 3) + (512 if expo else 0) <= 160 * 1024
    assert (sc["pairs"] / sc["n_items"] >= 4096.0) == (th == 512), (sc["pairs"], sc["n_items"])


def slice_preconditions(case, sc, sole):
    """launch_slices: the dataset kept its slices, exponential impulses, the item's LDS fits; all_sole picks store or add."""
    assert case["kind"] == "exponential" and sc["sl_rows"] > 0 and sc["n_items"] > 0
    assert sc["pairs"] <= 160 * sc["M"] and sc["sl_rows"] * 64 <= 2 * sc["pairs"] + 4096
    assert 320 + 16 * (case["N"] + 1) + 512 + 8 * (sc["max_item"] + 1) <= 160 * 1024
    assert sc["all_sole"] == int(sole)


@pytest.mark.parametrize("name", ["W-exp", "W-logit", "W-net", "W-net-logit"])
def test_two_pass_route_every_group_width(nhp, route, name):
    case, res = cr.prepared(name)
    P = len(res.grad)
    for group in (1, 2, 4, 8, 16, 32, 64):
        route(dict(EXACT, NHP_GROUP=str(group)))
        ll, g, sc = gradient(nhp, case, P)
        two_pass_preconditions(case, sc, group, 256)
        hold(f"{name} G={group}", ll, g, res, case["N"])
    # pass A on its default records: the 8-byte pair list for exponential impulses (48 bits of Δtmax; widths up to 16), the
    # planes of logit(x) made from the exact times for logit-normal ones
    route({"NHP_GRAD_SLICES": "0", "NHP_GROUP": "4"})
    ll, g, sc = gradient(nhp, case, P)
    two_pass_preconditions(case, sc, 4, 256)
    assert sc["pairs"] <= 40 * sc["M"]                                  # the pair list exists (cont_data.hip: plist_maxk)
    hold(f"{name} G=4, default pass A", ll, g, res, case["N"], delta=case["dt_max"] * 2.0 ** -48 if case["kind"] == "exponential" else 0.0)


@pytest.mark.parametrize("name", ["W-exp", "W-net"])
def test_slice_route_every_workgroup_shape(nhp, route, name):
    case, res = cr.prepared(name)
    P = len(res.grad)
    for cfg in SLICE_CFGS:
        route({"NHP_CHUNK": "256", "NHP_SLICES_CFG": cfg})
        ll, g, sc = gradient(nhp, case, P)
        slice_preconditions(case, sc, sole=False)
        assert sc["n_items"] > case["N"] and sc["max_item"] <= 256
        hold(f"{name} slices {cfg}", ll, g, res, case["N"], delta=slice_step(case, sc))


def test_slices_store_every_entry_when_each_node_is_one_item(nhp, route):
    case, res = cr.prepared("D")
    P = len(res.grad)
    route({"NHP_CHUNK": "4096"})
    ll, g, sc = gradient(nhp, case, P)
    slice_preconditions(case, sc, sole=True)
    assert sc["n_items"] == case["N"] == 3
    hold("D slices, direct store", ll, g, res, 3, delta=slice_step(case, sc))
    empty = 2                                                           # node 3: -T, zeros, -cnt
    assert g[empty] == -case["T"] and np.all(g[3 + 3 * empty:3 + 3 * empty + 3] == 0.0)
    assert np.array_equal(g[12 + 3 * empty:12 + 3 * empty + 3], -np.bincount(case["nodes"] - 1, minlength=3).astype(np.float64))
    route({"NHP_CHUNK": "4096"})                                        # a second build: the same bits
    ll2, g2, _ = gradient(nhp, case, P)
    assert ll2 == ll and np.array_equal(g, g2)
    route(dict(EXACT, NHP_CHUNK="4096"))
    ll, g, sc = gradient(nhp, case, P)
    two_pass_preconditions(case, sc, None, 256)
    assert sc["all_sole"] == 1
    hold("D two-pass", ll, g, res, 3)


@pytest.mark.parametrize("name", ["L-exp", "L-logit"])
def test_long_windows_take_512_threads(nhp, route, name):
    case, res = cr.prepared(name)
    route({})
    ll, g, sc = gradient(nhp, case, len(res.grad))
    assert sc["sl_rows"] == 0 and sc["pairs"] > 160 * sc["M"]           # not sliced, no pair list: the exact records
    two_pass_preconditions(case, sc, None, 512)
    hold(name, ll, g, res, case["N"])


@pytest.mark.parametrize("N", list(cr.REC_M))
def test_full_recursion_every_shape(nhp, route, N):
    case, res = cr.prepared("R-%d" % N)
    PQ = 1 if N <= 256 else 2 if N <= 512 else 4                        # nhp_rec_parts_for
    H = 1
    while 64 * PQ * H < N:
        H *= 2
    assert (PQ, H) == REC_SHAPE[N] and N <= 4096
    route({})
    ll, g, sc = gradient(nhp, case, len(res.grad), flags=FULL)
    assert sc["n_zero_time"] == 3
    hold(f"R-{N} {PQ}x{H}", ll, g, res, N)


@pytest.mark.parametrize("name", ["C", "C-net"])
def test_recursive_objective_through_its_truncated_window(nhp, route, name):
    case, res = cr.prepared(name)
    route({})
    assert window_routes(nhp, cr.process_of(nhp, case), (case["times"], case["nodes"], case["T"])) == [1, 1, 1]
    ll, g, sc = gradient(nhp, case, len(res.grad), flags=1)
    tail = cr.window_tail(res, cr.model_of(case), case["times"], case["nodes"], case["T"])
    hold(name, ll, g, res, case["N"], tail=tail)


def test_grid_baselines(nhp, route):
    case, res = cr.prepared("G-W")
    P = len(res.grad)
    route(dict(EXACT))
    ll, g, sc = gradient(nhp, case, P)
    two_pass_preconditions(case, sc, None, 256)
    hold("G-W two-pass", ll, g, res, case["N"])
    route({"NHP_CHUNK": "256"})
    ll, g, sc = gradient(nhp, case, P)
    slice_preconditions(case, sc, sole=False)
    hold("G-W slices", ll, g, res, case["N"], delta=slice_step(case, sc))
    case, res = cr.prepared("G-D")
    route({"NHP_CHUNK": "4096"})
    ll, g, sc = gradient(nhp, case, len(res.grad))
    slice_preconditions(case, sc, sole=True)                            # (one item per node, but a grid block is accumulated: no direct store)
    hold("G-D slices", ll, g, res, case["N"], delta=slice_step(case, sc))
    case, res = cr.prepared("G-R")
    route({})
    ll, g, sc = gradient(nhp, case, len(res.grad), flags=FULL)
    hold("G-R 1x2", ll, g, res, case["N"])


@pytest.mark.parametrize("name,env,flags", [("W-exp", EXACT, 0), ("W-exp", {"NHP_CHUNK": "256"}, 0), ("R-65", {}, FULL)])
def test_column_shards(nhp, route, name, env, flags):
    case, whole = cr.prepared(name)
    N, P = case["N"], len(whole.grad)
    col = np.concatenate([np.arange(N), np.tile(np.repeat(np.arange(N), N), 2)])
    total = np.zeros(P)
    sliced, step = "NHP_CHUNK" in env, 0.0
    for cols in ((0, 3), (3, N), (2, 3)):
        _, res = cr.prepared(name, cols)
        route(dict(env))
        ll, g, sc = gradient(nhp, case, P, flags=flags, columns=cols)
        if sliced:
            slice_preconditions(case, sc, sole=False)
        foreign = (col < cols[0]) | (col >= cols[1])
        assert np.all(g[foreign] == 0.0) and not np.any(np.signbit(g[foreign])), f"{name} {cols}: foreign entries must be exactly 0.0"
        step = max(step, slice_step(case, sc)) if sliced else 0.0
        hold(f"{name} shard {cols}", ll, g, res, N, delta=step)
        if cols != (2, 3):
            total += g
    ratio, bad, err, B = cr.check(total, whole, step)
    assert len(bad) == 0, cr.explain(total, whole, N, bad, err, B)
