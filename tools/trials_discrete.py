"""The convolution on trials against the plain route, at BASELINE config 4 (N=512, B=8, L=32, T=1e5, 5 % of the bins occupied):
hipEvent time of the nhp_disc_convolve call (the ctx timer: basis upload, the convolution kernel, the column-sum kernel) for
two inputs with the same counts -- one recording of 1e5 bins (the plain route), and R = 100 trials of 1000 bins.  The two are
timed in turn, call by call, after a warm-up of each; one JSON line with every sample and min / median / max.

    python tools/trials_discrete.py [--repeats 20] [--root TREE --label parent]

--root loads the package from another checkout (a built tree of the parent commit, say): a package without trials is timed
on the plain route alone.  --label names the tree in the output line ("this" by default).  Run the two trees in turn, several times, and compare the plain route's figures with the spread
between runs of the same tree before reading anything into a difference."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this")
ap.add_argument("--rate", type=float, default=0.05)
ap.add_argument("--bins", type=int, default=100_000)
ap.add_argument("--trials", type=int, default=100)
args = ap.parse_args()

spec = importlib.util.spec_from_file_location("__graft_entry__", os.path.join(args.root, "__graft_entry__.py"))
entry = importlib.util.module_from_spec(spec)
sys.modules["__graft_entry__"] = entry
spec.loader.exec_module(entry)
nhp = entry.load_package()

ctx = nhp.Context(0)
N, B, L, T, R = 512, 8, 32, args.bins, args.trials
assert T % R == 0
rng = np.random.default_rng(7)
data = rng.poisson(args.rate, (N, T)).astype(np.int64)
th = np.asfortranarray(np.full((N, N, B), 1.0 / B))
proc = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(rng.uniform(0.02, 0.08, N), 1.0), nhp.DiscreteGaussianImpulseResponse(th, L, 1.0),
                                         nhp.DenseWeightModel(np.asfortranarray(rng.uniform(0, 1, (N, N)) / N)), 1.0)
inputs = {"plain": nhp.DiscreteDataset(ctx, data)}
if hasattr(nhp, "stack_trials"):
    inputs["trials"] = nhp.DiscreteDataset(ctx, data, trial_offsets=np.arange(R + 1, dtype=np.int64) * (T // R))
    assert inputs["trials"].ntrials == R and inputs["plain"].ntrials == 1


def timed(ds):
    ctx.synchronize()
    ctx.timer_start()
    nhp.convolve(proc, ds, ctx=ctx)
    return ctx.timer_stop()


for ds in inputs.values():                       # warm-up: code objects, the Ŝ allocation
    for _ in range(3):
        timed(ds)
ms = {k: [] for k in inputs}
for _ in range(args.repeats):
    for k, ds in inputs.items():
        ms[k].append(timed(ds))
out = dict(tool="trials_discrete", tree=args.label, N=N, B=B, L=L, T=T, ntrials=R, rate=args.rate, repeats=args.repeats,
           bytes_stored=8 * T * N * B)
for k, v in ms.items():
    out[k] = dict(min_ms=min(v), median_ms=float(np.median(v)), max_ms=max(v), samples_ms=[round(x, 4) for x in v])
print(json.dumps(out))
