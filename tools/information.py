"""The observed-information blocks and one Hessian-vector product at a chosen size, beside one fused gradient call.

    python tools/information.py [--n 64] [--events 1000000] [--kbar 8] [--impulse exponential] [--reps 10] [--commit HASH]

Prints one JSON line with hipEvent times (ms, median and minimum over --reps, after one warm-up call each) on the context's
stream of
  blocks        nhp_cont_information into a device buffer (pass A, the blocks kernel, the mirror, the log-likelihood's readback)
  hvp           nhp_cont_hessian_vec with device vectors (pass A, the two window walks)
  loglik_grad   one nhp_cont_loglik_grad call (its 8·P-byte download is part of the call and of the time)
and the two ratios the design is judged by: blocks / (D · loglik_grad) -- D perturbed gradient calls would also yield every
block, so the blocks kernel earns its place only below 1 -- and hvp / loglik_grad.  The windowed objective
(recursive=False), data of synthetic.s_metric_data, parameters of synthetic.s_metric_process.
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
    call()                                                 # warm-up: code objects, scratch, lazily built layouts
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
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--kbar", type=float, default=8.0)
    ap.add_argument("--impulse", default="exponential", choices=("exponential", "logit-normal"))
    ap.add_argument("--tile-nodes", type=int, default=0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--commit", default="")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as entry
    nhp = entry.load_package()
    from nhp_amd import _lib

    N, M = args.n, args.events
    ctx = nhp.default_context()
    lib = _lib.lib()
    times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=args.kbar)
    proc = nhp.synthetic.s_metric_process(N, M, T, args.impulse, 1.0)
    ds = nhp.device_dataset(proc, (times, nodes, T), ctx)
    model = proc.device_model(ctx)
    kinds = 2 if args.impulse == "exponential" else 3
    D, P = 1 + kinds * N, N + kinds * N * N
    dev = torch.device("cuda", ctx.device)
    blocks = torch.empty(N * D * D, dtype=torch.float64, device=dev)
    v = torch.as_tensor(np.random.default_rng(0).normal(size=P), device=dev)
    hv = torch.empty(P, dtype=torch.float64, device=dev)
    g, ll = np.empty(P), C.c_double()
    torch.cuda.synchronize()

    def info():
        _lib.check(lib.nhp_cont_information(ctx.h, ds.h, model.h, 0, None, 0, args.tile_nodes, 1, C.byref(ll), blocks.data_ptr()), ctx.h)

    def product():
        _lib.check(lib.nhp_cont_hessian_vec(ctx.h, ds.h, model.h, 0, 1, v.data_ptr(), hv.data_ptr(), P), ctx.h)

    def loglik_grad():
        _lib.check(lib.nhp_cont_loglik_grad(ctx.h, ds.h, model.h, 0, C.byref(ll), _lib.dptr(g), P), ctx.h)

    out = {"tool": "information", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device), "N": N, "M": M,
           "kbar": args.kbar, "pairs": int(ds.pairs), "impulse": args.impulse, "D": D, "P": P, "tile_nodes": args.tile_nodes,
           "reps": args.reps}
    out["blocks_ms"], out["blocks_ms_min"] = timed(ctx, info, args.reps)
    out["hvp_ms"], out["hvp_ms_min"] = timed(ctx, product, args.reps)
    out["loglik_grad_ms"], out["loglik_grad_ms_min"] = timed(ctx, loglik_grad, args.reps)
    out["blocks_over_D_gradients"] = round(out["blocks_ms"] / (D * out["loglik_grad_ms"]), 4)
    out["hvp_over_gradient"] = round(out["hvp_ms"] / out["loglik_grad_ms"], 3)
    # the product against the blocks: the two kernels agree
    b = blocks.view(N, D, D)
    idx = torch.as_tensor(np.stack([nhp.inference.block_index(N, kinds, c) for c in range(N)]), device=dev)
    want = torch.zeros(P, dtype=torch.float64, device=dev)
    want[idx.reshape(-1)] = -torch.bmm(b, v[idx].unsqueeze(2)).reshape(-1)
    out["hvp_vs_blocks_rel"] = float((hv - want).abs().max() / want.abs().max())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
