#!/usr/bin/env python3
"""What the device-resident discrete chain costs and saves, at the scale of the discrete Gibbs kernels
(N = 512, B = 8, T = 1e5), standard and network process:
  - host memory: the peak of a keep_samples=False chain of `mem_steps` steps (tracemalloc, which sees numpy's buffers, and
    the growth of the process's peak resident set) next to the mem_steps x params bytes the default route holds -- taken
    first, before anything else has raised the peak;
  - one chain step on three routes -- resident with keep_samples=False (nhp_disc_mcmc_run), resident with keep_samples=True
    (one download per step), and the default route (every step uploads and downloads the model) -- as wall time around
    synchronised mcmc_ calls of `s2` and of `s1` steps, (t(s2) - t(s1)) / (s2 - s1), so that the convolution and the set-up
    of a call drop out; alternating rounds in one process, the median round and the spread of the rounds;
  - the accumulate kernels of both sources (the block of a network process, the product W∘θ of a standard one): hipEvent
    times of the moments-only pass, the fused pass inside a batch and on a batch boundary, alternating rounds, the median.
    The condition carried over from the continuous kernel: a fused step inside a batch costs less than TWO moments-only
    passes.
   python tools/mcmc_discrete.py [N] [B] [T] [rounds] [mem_steps]"""
import copy
import ctypes as C
import json
import os
import resource
import sys
import time
import tracemalloc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import __graft_entry__ as entry  # noqa: E402

nhp = entry.load_package()
from nhp_amd import _lib, discrete  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
B = int(sys.argv[2]) if len(sys.argv) > 2 else 8
T = int(sys.argv[3]) if len(sys.argv) > 3 else 100_000
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
MEM_STEPS = int(sys.argv[5]) if len(sys.argv) > 5 else 200
S1, S2, L, LAUNCHES = 1, 5, 32, 100

ctx = nhp.Context(0)
lib = _lib.lib()
rng = np.random.default_rng(7)                                  # the discrete workload of bench.py
data = rng.poisson(0.05, (N, T)).astype(np.int64)
th = np.asfortranarray(np.full((N, N, B), 1.0 / B))
imp = nhp.DiscreteGaussianImpulseResponse(th, L, 1.0)
base = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(rng.uniform(0.02, 0.08, N), 1.0), imp,
                                         nhp.DenseWeightModel(np.asfortranarray(rng.uniform(0, 1, (N, N)) / N)), 1.0)
A0 = (rng.uniform(size=(N, N)) < 0.5).astype(np.float64)
dsd = nhp.DiscreteDataset(ctx, data)


def fresh(kind):
    p = copy.deepcopy(base)
    if kind == "network":
        p = nhp.DiscreteNetworkHawkesProcess(p.baseline, p.impulses, p.weights, A0.copy(), nhp.BernoulliNetworkModel(0.5, N), 1.0)
    return p


ROUTES = {"resident": dict(keep_samples=False), "resident_keep_samples": dict(keep_samples=True, moments=True), "default": {}}


def chain_seconds(kind, route, steps):
    p = fresh(kind)
    ctx.synchronize()
    t0 = time.perf_counter()
    nhp.mcmc_(p, dsd, nsteps=steps, seed=1, ctx=ctx, **ROUTES[route])
    ctx.synchronize()
    return time.perf_counter() - t0


out = {"N": N, "B": B, "T": T, "events": int(data.sum()), "rounds": ROUNDS}

# ---- host memory, first ---------------------------------------------------------------------------------------------------
p = fresh("network")
nhp.mcmc_(p, dsd, nsteps=1, seed=1, ctx=ctx, keep_samples=False)        # (code objects, scratch and staging buffers exist)
rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
tracemalloc.start()
p = fresh("network")
t0 = time.perf_counter()
res = nhp.mcmc_(p, dsd, nsteps=MEM_STEPS, seed=1, ctx=ctx, keep_samples=False, moments=True, diagnostics=True)
mem_s = time.perf_counter() - t0
_, peak = tracemalloc.get_traced_memory()
tracemalloc.stop()
rss1 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
out["host_memory"] = {"steps": MEM_STEPS, "params_bytes": int(8 * len(p.params())),
                      "default_route_samples_bytes": int(8 * len(p.params()) * MEM_STEPS),
                      "resident_tracemalloc_peak_bytes": int(peak), "resident_peak_rss_growth_bytes": int(1024 * (rss1 - rss0)),
                      "chain_seconds": round(mem_s, 3), "kept": int(res.n)}

# ---- step time ------------------------------------------------------------------------------------------------------------
steps = {}
for kind in ("standard", "network"):
    for route in ROUTES:                                        # warm every route once
        chain_seconds(kind, route, S1)
    ms = {r: [] for r in ROUTES}
    for _ in range(ROUNDS):
        for route in ROUTES:
            a, b = chain_seconds(kind, route, S1), chain_seconds(kind, route, S2)
            ms[route].append(1e3 * (b - a) / (S2 - S1))
    med = {r: float(np.median(v)) for r, v in ms.items()}
    steps[kind] = {"ms_per_step": {r: round(v, 2) for r, v in med.items()},
                   "ms_all": {r: [round(x, 2) for x in v] for r, v in ms.items()},
                   "spread_ms": {r: round(float(np.max(v) - np.min(v)), 2) for r, v in ms.items()},
                   "default_over_resident": round(med["default"] / med["resident"], 3),
                   "condition_resident_not_slower": bool(med["resident"] <= med["default"] + (max(ms["default"]) - min(ms["default"]))
                                                         + (max(ms["resident"]) - min(ms["resident"])))}
out["step"] = steps

# ---- the accumulate kernels -------------------------------------------------------------------------------------------------
acc = {}
for kind in ("standard", "network"):
    proc = fresh(kind)
    model = discrete.DiscreteDeviceModel(ctx, proc)
    Lsum = discrete.disc_moments_length(proc)

    def configure(b, n_planned):
        _lib.check(lib.nhp_disc_model_diagnostics_configure(ctx.h, model.h, b, n_planned), ctx.h)
        _lib.check(lib.nhp_disc_model_moments_reset(ctx.h, model.h), ctx.h)

    def accumulate(n):
        for _ in range(n):
            _lib.check(lib.nhp_disc_model_moments_accumulate(ctx.h, model.h), ctx.h)

    def timed(n):
        accumulate(3)
        ctx.synchronize()
        ctx.timer_start()
        accumulate(n)
        return 1e3 * ctx.timer_stop() / n          # µs per launch

    modes = {"moments": (0, 0), "fused": (1 << 40, 0), "fused_boundary": (1, 0)}
    us = {m: [] for m in modes}
    for _ in range(ROUNDS):
        for m, (b, n_planned) in modes.items():
            configure(b, n_planned)
            us[m].append(timed(LAUNCHES))
    configure(0, 0)
    model.close()
    med = {m: float(np.median(v)) for m, v in us.items()}
    # planes moved per entry: x (the product reads θ and, out of cache, W) + read and write of Σx, Σx² [, B [, SB, QB]]
    acc[kind] = {"entries": Lsum, "us": {m: round(v, 2) for m, v in med.items()},
                 "us_all": {m: [round(x, 2) for x in v] for m, v in us.items()},
                 "fused_over_moments": round(med["fused"] / med["moments"], 3),
                 "boundary_over_moments": round(med["fused_boundary"] / med["moments"], 3),
                 "GB_per_s": {m: round(8e-3 * Lsum * pl / med[m], 1) for m, pl in (("moments", 5), ("fused", 7), ("fused_boundary", 11))},
                 "condition_fused_below_two_passes": bool(med["fused"] < 2.0 * med["moments"])}
out["accumulate"] = acc
print(json.dumps(out))
