#!/usr/bin/env python3
"""What scoring a discrete chain costs, at the scale of the discrete Gibbs kernels (N = 512, B = 8, T = 1e5),
standard and network process, the chain fitted on the first 80 % of the bins:
  - one nhp_disc_score_accumulate -- bump table, the GEMM on the scored rows, k_disc_score, k_disc_score_fold -- as hipEvent
    time over back-to-back launches, for the WAIC scorer (the training bins) and the held-out one (the last 20 %), next to
    the bytes the pass over the cells must move (64 per cell: λ, the count, three planes read and written);
  - one chain step of the resident route (nhp_disc_mcmc_run) with WAIC attached, with WAIC and the held-out scorer, and with
    nothing attached: wall time around synchronised mcmc_ calls of `s2` and `s1` steps, (t(s2) - t(s1)) / (s2 - s1), so that
    the convolution and the set-up drop out; alternating rounds in one process, the median and the spread of the rounds.
`--step [TREE]` instead prints the ms per resident chain step with nothing attached (`keep_samples=False, moments=True`),
standard and network, three rounds, and the sum of `res.mean` as a checksum -- for the checkout at TREE (default: this one),
which need not know the scorer.  Run it in turn on a checkout of the parent commit and on this one, each call a process of
its own, to hold an unscored step against the parent:
   for i in 1 2 3; do python tools/score_discrete.py --step ../parent; python tools/score_discrete.py --step; done
`--kernels` runs the accumulates alone, for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/score_discrete.py
--kernels): the times of k_disc_score, k_disc_score_fold and the range GEMM come from there.
   python tools/score_discrete.py [--kernels | --step [TREE]] [N] [B] [T] [rounds]"""
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = [a for a in sys.argv[1:] if a != "--kernels"]
KERNELS = "--kernels" in sys.argv[1:]
STEP = "--step" in argv
if STEP:                                                        # --step [TREE]: the package of another checkout
    i = argv.index("--step")
    tree = argv[i + 1] if len(argv) > i + 1 and not argv[i + 1].lstrip("-").isdigit() else None
    del argv[i:i + (2 if tree else 1)]
    ROOT = os.path.abspath(tree) if tree else ROOT
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import __graft_entry__ as entry  # noqa: E402

nhp = entry.load_package()
N = int(argv[0]) if len(argv) > 0 else 512
B = int(argv[1]) if len(argv) > 1 else 8
T = int(argv[2]) if len(argv) > 2 else 100_000
ROUNDS = int(argv[3]) if len(argv) > 3 else 5
S1, S2, L, LAUNCHES = 1, 5, 32, 20
SPLIT = (4 * T) // 5

ctx = nhp.Context(0)
rng = np.random.default_rng(7)                                  # the discrete workload of bench.py
data = rng.poisson(0.05, (N, T)).astype(np.int64)
th = np.asfortranarray(np.full((N, N, B), 1.0 / B))
imp = nhp.DiscreteGaussianImpulseResponse(th, L, 1.0)
base = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(rng.uniform(0.02, 0.08, N), 1.0), imp,
                                         nhp.DenseWeightModel(np.asfortranarray(rng.uniform(0, 1, (N, N)) / N)), 1.0)
A0 = (rng.uniform(size=(N, N)) < 0.5).astype(np.float64)
if not STEP:
    from nhp_amd import discrete  # noqa: E402
    train, full = nhp.DiscreteDataset(ctx, data[:, :SPLIT]), nhp.DiscreteDataset(ctx, data)


def fresh(kind):
    p = copy.deepcopy(base)
    if kind == "network":
        p = nhp.DiscreteNetworkHawkesProcess(p.baseline, p.impulses, p.weights, A0.copy(), nhp.BernoulliNetworkModel(0.5, N), 1.0)
    return p


if STEP:                                                        # an unscored resident step on the whole matrix, for any checkout
    dsd = nhp.DiscreteDataset(ctx, data)

    def plain_seconds(kind, steps):
        p = fresh(kind)
        ctx.synchronize()
        t0 = time.perf_counter()
        res = nhp.mcmc_(p, dsd, nsteps=steps, seed=1, ctx=ctx, keep_samples=False, moments=True)
        ctx.synchronize()
        return time.perf_counter() - t0, res

    out = {"tree": tree or ".", "N": N, "B": B, "T": T}
    for kind in ("standard", "network"):
        plain_seconds(kind, S1)
        ms = []
        for _ in range(3):
            (a, _), (b, res) = plain_seconds(kind, S1), plain_seconds(kind, S2)
            ms.append(round(1e3 * (b - a) / (S2 - S1), 3))
        out[kind] = ms
        out[kind + "_mean_checksum"] = float(np.sum(res.mean))
    print(json.dumps(out))
    sys.exit(0)

out = {"N": N, "B": B, "T": T, "train_bins": SPLIT, "events": int(data.sum()), "rounds": ROUNDS}

# ---- one accumulate ---------------------------------------------------------------------------------------------------------
acc = {}
for kind in ("standard", "network"):
    proc = fresh(kind)
    model = discrete.DiscreteDeviceModel(ctx, proc)
    nhp.convolve(proc, train, ctx)
    nhp.convolve(proc, full, ctx)
    for name, ds, bins in (("waic", train, (0, SPLIT)), ("heldout", full, (SPLIT, T))):
        s = discrete._DeviceScore(ctx, ds, bins)
        us = []
        for _ in range(1 if KERNELS else ROUNDS):
            for _ in range(3):
                s.accumulate(model)
            ctx.synchronize()
            ctx.timer_start()
            for _ in range(LAUNCHES):
                s.accumulate(model)
            us.append(1e3 * ctx.timer_stop() / LAUNCHES)
        cells = (bins[1] - bins[0]) * N
        med = float(np.median(us))
        acc[f"{kind}_{name}"] = {"cells": cells, "us": round(med, 1), "us_all": [round(x, 1) for x in us],
                                 "score_pass_bytes_needed": 64 * cells, "planes_bytes": 24 * cells, "scratch_lambda_bytes": 8 * cells}
        s.close()
    model.close()
out["accumulate"] = acc
if KERNELS:
    print(json.dumps(out))
    sys.exit(0)

# ---- one chain step, scored and not ---------------------------------------------------------------------------------------------
MODES = {"plain": {}, "waic": dict(waic=True), "waic_heldout": dict(waic=True, heldout=(full, (SPLIT, T)))}


def chain_seconds(kind, mode, steps):
    p = fresh(kind)
    ctx.synchronize()
    t0 = time.perf_counter()
    nhp.mcmc_(p, train, nsteps=steps, seed=1, ctx=ctx, keep_samples=False, **MODES[mode])
    ctx.synchronize()
    return time.perf_counter() - t0


steps = {}
for kind in ("standard", "network"):
    for mode in MODES:                                          # warm every mode once
        chain_seconds(kind, mode, S1)
    ms = {m: [] for m in MODES}
    for _ in range(ROUNDS):
        for mode in MODES:
            a, b = chain_seconds(kind, mode, S1), chain_seconds(kind, mode, S2)
            ms[mode].append(1e3 * (b - a) / (S2 - S1))
    med = {m: float(np.median(v)) for m, v in ms.items()}
    steps[kind] = {"ms_per_step": {m: round(v, 2) for m, v in med.items()}, "ms_all": {m: [round(x, 2) for x in v] for m, v in ms.items()},
                   "spread_ms": {m: round(float(np.max(v) - np.min(v)), 2) for m, v in ms.items()},
                   "waic_adds_ms": round(med["waic"] - med["plain"], 2), "waic_heldout_adds_ms": round(med["waic_heldout"] - med["plain"], 2)}
out["step"] = steps
print(json.dumps(out))
