"""The discrete information blocks of both kinds and one information-vector product at a chosen size, beside one gradient call.

    python tools/information_discrete.py [--n 64] [--basis 4] [--bins 100000] [--lags 8] [--rates 0.4,0.01] [--reps 10] [--commit HASH]

Prints one JSON line per event rate (events per bin and node, Poisson counts) with hipEvent times (ms, median and minimum
over --reps, after one warm-up call each) on the context's stream of
  observed / fisher   nhp_disc_information of that kind, all columns, into a device buffer (the parameter upload, both GEMM-1
                      launches, the weights, the chunk lists, the Gram kernel, the finish and the log-likelihood's readback)
  hvp                 nhp_disc_hessian_vec (observed kind) with device vectors
  loglik_grad         one nhp_disc_loglik_grad call (its 8·P-byte download is part of the call and of the time)
the two ratios the design is judged by -- blocks / (D · loglik_grad): D perturbed gradient calls would also yield every block,
so the blocks call earns its place only below 1; and hvp / loglik_grad -- and the achieved TFLOP/s on the useful flops,
D(D+1)·n_t per column (n_t: the bins with a non-zero weight; every bin for the Fisher kind).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, call, reps):
    call()                                                 # warm-up: code objects, scratch
    ms = []
    for _ in range(reps):
        ctx.synchronize()
        ctx.timer_start()
        call()
        ms.append(ctx.timer_stop())
    return round(statistics.median(ms), 4), round(min(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--basis", type=int, default=4)
    ap.add_argument("--bins", type=int, default=100_000)
    ap.add_argument("--lags", type=int, default=8)
    ap.add_argument("--rates", default="0.4,0.01")
    ap.add_argument("--tile-rows", type=int, default=0)
    ap.add_argument("--slab-bins", type=int, default=0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--commit", default="")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as entry
    nhp = entry.load_package()
    from nhp_amd import _lib

    N, B, T, L, dt = args.n, args.basis, args.bins, args.lags, 1.0
    D, P = 1 + N * B, N + N * N * B
    ctx = nhp.default_context()
    lib = _lib.lib()
    dev = torch.device("cuda", ctx.device)
    for rate in (float(r) for r in args.rates.split(",")):
        rng = np.random.default_rng(12)
        data = rng.poisson(rate, (N, T)).astype(np.int64)
        # a stable model whose mean intensity is about the data's rate: half from the baseline, half from the links
        q = np.floor(rng.dirichlet(np.ones(B), (N, N)) * 2.0 ** 20)          # multiples of 2^-20: every Σ_b θ is exactly 1
        q[:, :, -1] = 2.0 ** 20 - q[:, :, :-1].sum(axis=2)
        proc = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(np.full(N, 0.5 * rate) * rng.uniform(0.8, 1.2, N), dt),
                                                 nhp.DiscreteGaussianImpulseResponse(q / 2.0 ** 20, L, dt),
                                                 nhp.DenseWeightModel(rng.uniform(0.5, 1.5, (N, N)) * 0.5 / N), dt)
        ds = nhp.convolve(proc, data, ctx)
        l0, W, th, _ = proc._lowered()
        blocks = torch.empty(N * D * D, dtype=torch.float64, device=dev)
        v = torch.as_tensor(rng.normal(size=P), device=dev)
        hv = torch.empty(P, dtype=torch.float64, device=dev)
        g, ll = np.empty(P), C.c_double()
        torch.cuda.synchronize()

        def info(kind):
            _lib.check(lib.nhp_disc_information(ctx.h, ds.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), dt, kind, None, 0, args.tile_rows,
                                                args.slab_bins, C.byref(ll), blocks.data_ptr()), ctx.h)

        def product():
            _lib.check(lib.nhp_disc_hessian_vec(ctx.h, ds.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), dt, 0, v.data_ptr(), hv.data_ptr()), ctx.h)

        def loglik_grad():
            _lib.check(lib.nhp_disc_loglik_grad(ctx.h, ds.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), dt, C.byref(ll), _lib.dptr(g), P), ctx.h)

        occupied = int(np.count_nonzero(data))
        chunks = int(sum(np.count_nonzero(np.add.reduceat(row != 0, np.arange(0, T, 16))) for row in data))
        out = {"tool": "information_discrete", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device), "N": N, "B": B,
               "T": T, "L": L, "rate": rate, "D": D, "P": P, "occupied_bins": occupied, "occupied_chunks": chunks,
               "all_chunks": N * ((T + 15) // 16), "tile_rows": args.tile_rows, "slab_bins": args.slab_bins, "reps": args.reps}
        out["loglik_grad_ms"], out["loglik_grad_ms_min"] = timed(ctx, loglik_grad, args.reps)
        for kind, name, n_t in ((0, "observed", occupied), (1, "fisher", N * T)):
            out[name + "_ms"], out[name + "_ms_min"] = timed(ctx, lambda: info(kind), args.reps)
            out[name + "_over_D_gradients"] = round(out[name + "_ms"] / (D * out["loglik_grad_ms"]), 5)
            out[name + "_useful_tflops"] = round(D * (D + 1) * n_t / (out[name + "_ms"] * 1e-3) / 1e12, 3)
        # the product against the observed blocks: the two routes agree
        info(0)
        out["hvp_ms"], out["hvp_ms_min"] = timed(ctx, product, args.reps)
        out["hvp_over_gradient"] = round(out["hvp_ms"] / out["loglik_grad_ms"], 3)
        b = blocks.view(N, D, D)
        idx = torch.as_tensor(np.stack([nhp.discrete.disc_block_index(N, B, c) for c in range(N)]), device=dev)
        want = torch.zeros(P, dtype=torch.float64, device=dev)
        want[idx.reshape(-1)] = torch.bmm(b, v[idx].unsqueeze(2)).reshape(-1)
        out["hvp_vs_blocks_rel"] = float((hv - want).abs().max() / want.abs().max())
        print(json.dumps(out), flush=True)
        del ds


if __name__ == "__main__":
    main()
