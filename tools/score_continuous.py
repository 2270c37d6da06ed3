#!/usr/bin/env python3
"""What scoring a continuous chain costs, at the metric size (N = 1024, M = 1e6, K̄ = 8, exponential impulses),
with K = 1000 and K = 100 blocks over the whole recording:
  - one nhp_cont_score_accumulate -- λ[M], the row-major tables, k_cscore_block, k_cont_score, k_score_fold -- as hipEvent time
    around ONE call, the median of 20 after a warm-up, set beside nhp_cont_compensator (every output, on the device) +
    nhp_cont_event_intensity (which downloads its M doubles) timed the same way in the same process, the two alternated;
    a scored draw does the same O(M·N) gathers and fewer CDF terms, so it is expected not to exceed their sum.
`--kernels` runs the accumulates alone, for a kernel trace of its own
   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/score_continuous.py --kernels
from which the split over the λ kernel, k_cscore_tables, k_cscore_block, k_cont_score and k_score_fold comes (few blocks
leave k_cont_score at most K busy lanes per node column, each walking M / (N·K) logarithms: K = 100 is where that shows).
`--step [TREE]` instead prints the ms per resident network chain step with nothing attached (`keep_samples=False,
moments=True`) as (t(550 steps) - t(50 steps)) / 500 around synchronised calls, three rounds, and the sum of `res.mean` as
a checksum -- for the checkout at TREE (default: this one), which need not know the scorer.  Run it in turn on a checkout of
the parent commit and on this one, each call a process of its own:
   for i in 1 2 3; do python tools/score_continuous.py --step ../parent; python tools/score_continuous.py --step; done
   python tools/score_continuous.py [--kernels | --step [TREE]] [N] [M] [rounds]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = [a for a in sys.argv[1:] if a != "--kernels"]
KERNELS = "--kernels" in sys.argv[1:]
STEP = "--step" in argv
tree = None
if STEP:                                                        # --step [TREE]: the package of another checkout
    i = argv.index("--step")
    tree = argv[i + 1] if len(argv) > i + 1 and not argv[i + 1].lstrip("-").isdigit() else None
    del argv[i:i + (2 if tree else 1)]
    ROOT = os.path.abspath(tree) if tree else ROOT
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import __graft_entry__ as entry  # noqa: E402

nhp = entry.load_package()
from nhp_amd import _lib  # noqa: E402

N = int(argv[0]) if len(argv) > 0 else 1024
M = int(argv[1]) if len(argv) > 1 else 1_000_000
ROUNDS = int(argv[2]) if len(argv) > 2 else 20
S1, S2 = 50, 550                                               # 500 steps apart: ~0.2 s of device work per difference

ctx = nhp.Context(0)
lib = _lib.lib()
times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=8.0)
base = nhp.synthetic.s_metric_process(N, M, T, "exponential", 1.0)
data = (times, nodes, T)


def network_process():
    return nhp.synthetic.s_metric_process(N, M, T, "exponential", 1.0, network=True)


if STEP:                                                        # an unscored resident network step, for any checkout
    ds = nhp.device_dataset(base, data, ctx)

    def plain_seconds(steps):
        p = network_process()
        ctx.synchronize()
        t0 = time.perf_counter()
        res = nhp.mcmc_(p, ds, nsteps=steps, seed=1, ctx=ctx, keep_samples=False, moments=True)
        ctx.synchronize()
        return time.perf_counter() - t0, res

    plain_seconds(S1)
    ms = []
    for _ in range(3):
        (a, _), (b, res) = plain_seconds(S1), plain_seconds(S2)
        ms.append(round(1e3 * (b - a) / (S2 - S1), 4))
    print(json.dumps({"tree": tree or ".", "N": N, "M": M, "network_ms_per_step": ms, "mean_checksum": float(np.sum(res.mean))}))
    sys.exit(0)

import torch  # noqa: E402
from nhp_amd import inference  # noqa: E402

ds = nhp.device_dataset(base, data, ctx)
model = base.device_model(ctx)
dev = torch.device("cuda", ctx.device)
at, resid, tot = (torch.empty(n, dtype=torch.float64, device=dev) for n in (M, M, N))
lam = np.empty(M)
torch.cuda.synchronize(dev)


def timed(fn):
    ctx.synchronize()
    ctx.timer_start()
    fn()
    return 1e3 * ctx.timer_stop()                                # µs


def parts():
    _lib.check(lib.nhp_cont_compensator(ctx.h, ds.h, model.h, 1, at.data_ptr(), resid.data_ptr(), tot.data_ptr()), ctx.h)
    _lib.check(lib.nhp_cont_event_intensity(ctx.h, ds.h, model.h, _lib.dptr(lam)), ctx.h)


out = {"N": N, "M": M, "pairs": int(lib.nhp_cont_dataset_pairs(ds.h)), "rounds": ROUNDS, "accumulate": {}}
for K in (1000, 100):
    s = inference._DeviceScore(ctx, ds, np.linspace(0.0, T, K + 1))
    for _ in range(3):
        s.accumulate(model)
        if not KERNELS:
            parts()
    a_us, p_us = [], []
    for _ in range(ROUNDS):
        a_us.append(timed(lambda: s.accumulate(model)))
        if not KERNELS:
            p_us.append(timed(parts))
    row = {"cells": K * N, "planes_bytes": 24 * K * N, "accumulate_us": round(float(np.median(a_us)), 1),
           "accumulate_us_range": [round(min(a_us), 1), round(max(a_us), 1)]}
    if not KERNELS:
        row.update(compensator_plus_event_intensity_us=round(float(np.median(p_us)), 1),
                   compensator_plus_event_intensity_us_range=[round(min(p_us), 1), round(max(p_us), 1)])
    out["accumulate"][f"K={K}"] = row
    s.close()
print(json.dumps(out))
