"""Stochastic block network model at N = 1024, K = 8 (argv: N K): the whole block-model network step, the same step without
its label sweep (labels_every beyond the run), their difference = the label sweep inside the chain, the sweep by itself
through the stand-alone entry, and the Bernoulli network step on the same data, in ms per call.
Device-resident calls timed with the context's event timer over `reps` enqueued calls."""
import ctypes as C, json, os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as e


def main():
    nhp = e.load_package()
    from nhp_amd import _lib, inference
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    M, reps = 1_000_000 * N // 1024, 20
    lib, ctx = _lib.lib(), nhp.Context(0)
    rng = np.random.default_rng(0)
    times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=8.0)
    proc = nhp.synthetic.s_metric_process(N, M, T, "exponential", 1.0, network=True)
    ds = nhp.device_dataset(proc, (times, nodes, T), ctx)
    model, pri = proc.device_model(ctx), inference._priors(proc)
    z = rng.integers(0, K, N).astype(np.int32)
    rho = rng.uniform(0.2, 0.8, (K, K))
    pi = np.full(K, 1.0 / K)

    def timed(call, n=reps):
        call(0)                                                   # first call: pair lists, LDS attributes
        ctx.synchronize()
        ctx.timer_start()
        for i in range(n):
            call(1 + i)
        return ctx.timer_stop() / n

    _lib.check(lib.nhp_cont_model_set_rho(ctx.h, model.h, 0.5), ctx.h)
    t_bern = timed(lambda s: _lib.check(lib.nhp_cont_network_step(ctx.h, None, ds.h, model.h, 1.0, 1.0, 1, s), ctx.h))
    t_gibbs = timed(lambda s: _lib.check(lib.nhp_cont_gibbs_step(ctx.h, ds.h, model.h, C.byref(pri), 1, s), ctx.h))
    out = {"N": N, "K": K, "bernoulli_network_step_ms": t_bern, "gibbs_step_ms": t_gibbs}
    _lib.check(lib.nhp_cont_model_set_sbm(ctx.h, model.h, K, z.ctypes.data, _lib.dptr(_lib.colmajor(rho)), _lib.dptr(pi), 1.0, 1.0, 1.0), ctx.h)
    _lib.check(lib.nhp_cont_model_set_sbm_labels_every(ctx.h, model.h, 1), ctx.h)
    t_step = timed(lambda s: _lib.check(lib.nhp_cont_sbm_step(ctx.h, ds.h, model.h, 1, s), ctx.h))
    _lib.check(lib.nhp_cont_model_set_sbm_labels_every(ctx.h, model.h, 1 << 30), ctx.h)
    t_nolabels = timed(lambda s: _lib.check(lib.nhp_cont_sbm_step(ctx.h, ds.h, model.h, 1, s), ctx.h))
    out["sbm_step_ms"], out["sbm_step_without_labels_ms"], out["label_sweep_ms"] = t_step, t_nolabels, t_step - t_nolabels
    # the sweep by itself, through the stand-alone entry on the chain's current A and state: a call with 21 sweeps against a
    # call with 1 (uploads, packing and tables are the same in both), per sweep; the labels settle over the sweeps, so this
    # is the cost of a sweep in which few nodes move, where the figure above is that of the chain's own steps
    A, zz, rr, pp = np.empty(N * N), np.empty(N, dtype=np.int32), np.empty(K * K), np.empty(K)
    _lib.check(lib.nhp_cont_model_get_adjacency(ctx.h, model.h, _lib.dptr(A), N * N), ctx.h)
    _lib.check(lib.nhp_cont_model_get_sbm(ctx.h, model.h, zz.ctypes.data, _lib.dptr(rr), _lib.dptr(pp), None, None), ctx.h)

    def blocks(n_sweeps):
        z1 = zz.copy()
        t0 = time.perf_counter()
        _lib.check(lib.nhp_sbm_resample_blocks(ctx.h, _lib.dptr(A), N, K, z1.ctypes.data, _lib.dptr(rr), _lib.dptr(pp), None, 1, 0, n_sweeps,
                                               None, None), ctx.h)
        return 1e3 * (time.perf_counter() - t0)
    blocks(1)
    out["label_sweep_ms_settled"] = (min(blocks(21) for _ in range(3)) - min(blocks(1) for _ in range(3))) / 20
    try:
        out["commit"] = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        out["commit"] = None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
