"""Continuous datasets of several trials against one recording, at N = 1024, M = 1e6, mean window 8:

    plain    one recording: the dataset's cold call (wall time of DeviceDataset(...), host and device pre-pass), one windowed
             log-likelihood and one recursive=True log-likelihood (hipEvent time through the ctx timer), one device mle_ step
             and one compensator call (wall time), with the pair counts
    trials   the same events cut into R = 1000 trials of equal length: the same figures

One JSON line with every sample and min / median / max per figure.

    python tools/trials_continuous.py [--repeats 8] [--plain-only] [--root TREE --label parent]

--root loads the package from another checkout (a built tree of the parent commit, say): a package without trials is timed
on the plain figures alone.  --plain-only times the plain figures alone in this tree too: the process then makes the same
calls in the same order as the parent's (a dataset's cold call is mostly allocation, and what a process allocated and freed
before changes it by more than any code does), which is the run to compare with the parent.  Run the two trees in turn, several
times, and compare the plain figures with the spread between runs of the same tree before reading anything into a difference."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=8)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this")
ap.add_argument("--nodes", type=int, default=1024)
ap.add_argument("--events", type=int, default=1_000_000)
ap.add_argument("--trials", type=int, default=1000)
ap.add_argument("--plain-only", action="store_true")
args = ap.parse_args()

spec = importlib.util.spec_from_file_location("__graft_entry__", os.path.join(args.root, "__graft_entry__.py"))
entry = importlib.util.module_from_spec(spec)
sys.modules["__graft_entry__"] = entry
spec.loader.exec_module(entry)
nhp = entry.load_package()
from nhp_amd import _lib, continuous                                    # noqa: E402

ctx = nhp.default_context()
N, M, R = args.nodes, args.events, args.trials
times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=8.0)
proc = nhp.synthetic.s_metric_process(N, M, T, "exponential", 1.0)
dt_max = float(proc.impulses.Δtmax)
plain = (times, nodes, T)
has_trials = hasattr(nhp, "stack_event_trials") and not args.plain_only
stacked = None
if has_trials:
    edge = np.searchsorted(times, np.arange(R + 1) * (T / R), side="left")
    edge[0], edge[-1] = 0, M
    stacked = nhp.stack_event_trials([(times[a:b] - r * (T / R), nodes[a:b], T / R) for r, (a, b) in enumerate(zip(edge[:-1], edge[1:]))])


def build(data, how):
    nhp.invalidate_device_datasets()
    ctx.synchronize()
    t0 = time.perf_counter()
    ds = continuous.DeviceDataset(ctx, data, N, dt_max, build=how)
    ctx.synchronize()
    return ds, (time.perf_counter() - t0) * 1e3


def evaluate(ds, model, flags):
    import ctypes as C
    ll = C.c_double()
    ctx.synchronize()
    ctx.timer_start()
    _lib.check(_lib.lib().nhp_cont_loglik(ctx.h, ds.h, model.h, flags, C.byref(ll)), ctx.h)
    return ctx.timer_stop(), ll.value


model = proc.device_model(ctx)
ms, info = {}, {}
for _ in range(args.repeats + 1):                   # the first round is the warm-up (code objects, allocations) and is dropped
    for kind, data in (("plain", plain), ("trials", stacked)):
        if data is None:
            continue
        for how in ("host", "device"):
            ds, t = build(data, how)
            ms.setdefault(f"{kind}_build_{how}", []).append(t)
        info[f"{kind}_pairs"] = int(ds.pairs)
        evaluate(ds, model, 0)
        ms.setdefault(f"{kind}_loglik", []).append(evaluate(ds, model, 0)[0])
        evaluate(ds, model, _lib.LL_RECURSIVE)
        ms.setdefault(f"{kind}_loglik_recursive", []).append(evaluate(ds, model, _lib.LL_RECURSIVE)[0])
        out = np.full(4, np.nan)
        _lib.check(_lib.lib().nhp_probe_recursive_window(ctx.h, ds.h, model.h, 1.0, _lib.dptr(out)), ctx.h)
        info[f"{kind}_recursive_window"], info[f"{kind}_recursive_pairs"], info[f"{kind}_recursive_cut"] = int(out[1]), int(out[3]), float(out[0])
        fit = nhp.synthetic.s_metric_process(N, M, T, "exponential", 1.0)
        t0 = time.perf_counter()
        nhp.mle_(fit, ds, optimizer="device", guess=proc.params(), recursive=False, max_steps=1)
        ms.setdefault(f"{kind}_mle_device_step", []).append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        nhp.compensator(proc, ds, ctx=ctx, model=model)
        ms.setdefault(f"{kind}_compensator", []).append((time.perf_counter() - t0) * 1e3)
        del ds
summary = {k: {"min": min(v[1:]), "median": float(np.median(v[1:])), "max": max(v[1:]), "samples": v[1:]} for k, v in ms.items()}
print(json.dumps({"tool": "trials_continuous", "label": args.label, "N": N, "M": M, "R": R if has_trials else 1, "unit": "ms", **info,
                  **summary}))
