#!/usr/bin/env python3
"""What the streaming convergence diagnostics cost per kept step: at N = 1024, logit-normal network model
(len = N + 4N² entries), hipEvent times of
  - the moments-only accumulate (k_moments: 5 planes of traffic),
  - the fused accumulate on a step inside a batch (7 planes) and on a batch boundary (11 planes),
  - the finalize (nhp_cont_model_diagnostics_fetch, summary only),
in alternating rounds of `launches` launches each; the median round counts.  The condition the fused kernel is held to: a
step inside a batch costs less than TWO moments-only passes (what an unfused second kernel would cost).
   python tools/chain_diagnostics.py [N] [launches] [rounds]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import __graft_entry__ as entry  # noqa: E402

nhp = entry.load_package()
from nhp_amd import _lib, inference  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
K = int(sys.argv[2]) if len(sys.argv) > 2 else 100
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
STEP_MS = 0.41          # a whole network mcmc_ step at N = 1024, logit-normal (README)

ctx = nhp.Context(0)
proc = nhp.synthetic.s_metric_process(N, 1_000_000, 125_000.0, "logitnormal", 1.0, network=True)
model = proc.device_model(ctx)
lib = _lib.lib()
L = inference.moments_length(proc)
_lib.check(lib.nhp_cont_model_set_rho(ctx.h, model.h, 0.5), ctx.h)


def configure(b, n_planned):
    _lib.check(lib.nhp_cont_model_diagnostics_configure(ctx.h, model.h, b, n_planned), ctx.h)
    _lib.check(lib.nhp_cont_model_moments_reset(ctx.h, model.h), ctx.h)


def accumulate(n):
    for _ in range(n):
        _lib.check(lib.nhp_cont_model_moments_accumulate(ctx.h, model.h), ctx.h)


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
        us[m].append(timed(K))
configure(10, K)
accumulate(K)
summary = np.empty(_lib.DIAG_GROUPS * _lib.DIAG_FIELDS)
fin = []
for _ in range(ROUNDS):
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(K):
        _lib.check(lib.nhp_cont_model_diagnostics_fetch(ctx.h, model.h, 100.0, 1.01, _lib.dptr(summary), None, None, None, L), ctx.h)
    fin.append(1e3 * ctx.timer_stop() / K)
configure(0, 0)
med = {m: float(np.median(v)) for m, v in us.items()}
out = {"N": N, "entries": L, "launches": K, "rounds": ROUNDS, "us": {m: round(v, 2) for m, v in med.items()},
       "us_all": {m: [round(x, 2) for x in v] for m, v in us.items()}, "finalize_us": round(float(np.median(fin)), 2),
       "fused_over_moments": round(med["fused"] / med["moments"], 3), "boundary_over_moments": round(med["fused_boundary"] / med["moments"], 3),
       "by_planes": {"fused": 7 / 5, "fused_boundary": 11 / 5},
       "GB_per_s": {m: round(8e-3 * L * p / med[m], 1) for m, p in (("moments", 5), ("fused", 7), ("fused_boundary", 11))},
       "extra_share_of_step": round(1e-3 * (med["fused"] - med["moments"]) / STEP_MS, 4),
       "condition_fused_below_two_passes": bool(med["fused"] < 2.0 * med["moments"])}
print(json.dumps(out))
