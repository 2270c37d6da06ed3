"""Latent distance network model at N = 1024, D = 2 (argv: N D) on data simulated from the model: the position sweep and the
offset update by themselves through the stand-alone entry, the whole latent network step and the same step without its
position sweep inside a chain, the Bernoulli and the block-model (K = 8) network steps on the same data, and the mean
number of slice attempts per node -- in ms per call, median and range over `runs` repeats after a warm-up.
Device-resident calls are timed with the context's event timer over `reps` enqueued calls; the stand-alone entry by the
difference of a call with 1 + n sweeps and a call with 1 (uploads and packing are the same in both)."""
import ctypes as C, json, os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as e


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "runs": len(xs)}


def main():
    nhp = e.load_package()
    from nhp_amd import _lib, inference
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    D = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    K, M, reps, runs = 8, 1_000_000 * N // 1024, 10, 5
    lib, ctx = _lib.lib(), nhp.Context(0)
    rng = np.random.default_rng(0)
    # a network drawn from the model (positions from the prior, b chosen for about 8 links per node), events on it
    truth = nhp.LatentDistanceNetworkModel(N, D, b=float(np.log(8.0 / N) + 2.0), σ=1.0)
    A = truth.rand(rng)
    times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=8.0)
    proc = nhp.synthetic.s_metric_process(N, M, T, "exponential", 1.0, network=True)
    proc.adjacency_matrix = A
    ds = nhp.device_dataset(proc, (times, nodes, T), ctx)
    model, pri = proc.device_model(ctx), inference._priors(proc)

    def timed(call):
        call(0)                                                   # warm-up: pair lists, LDS attributes
        ctx.synchronize()
        out = []
        for r in range(runs):
            ctx.timer_start()
            for i in range(reps):
                call(1 + r * reps + i)
            out.append(ctx.timer_stop() / reps)
        return spread(out)

    out = {"N": N, "D": D, "links_per_node": float(A.sum() / N)}
    _lib.check(lib.nhp_cont_model_set_rho(ctx.h, model.h, 0.5), ctx.h)
    out["bernoulli_network_step_ms"] = timed(lambda s: _lib.check(lib.nhp_cont_network_step(ctx.h, None, ds.h, model.h, 1.0, 1.0, 1, s), ctx.h))
    z8 = rng.integers(0, K, N).astype(np.int32)
    _lib.check(lib.nhp_cont_model_set_sbm(ctx.h, model.h, K, z8.ctypes.data, _lib.dptr(_lib.colmajor(rng.uniform(0.2, 0.8, (K, K)))),
                                          _lib.dptr(np.full(K, 1.0 / K)), 1.0, 1.0, 1.0), ctx.h)
    out["sbm_network_step_ms"] = timed(lambda s: _lib.check(lib.nhp_cont_sbm_step(ctx.h, ds.h, model.h, 1, s), ctx.h))
    z0 = _lib.colmajor(truth.z)
    _lib.check(lib.nhp_cont_model_set_latent(ctx.h, model.h, D, _lib.dptr(z0), truth.b, 1.0, 0.0, 2.0), ctx.h)
    out["latent_network_step_ms"] = timed(lambda s: _lib.check(lib.nhp_cont_latent_step(ctx.h, ds.h, model.h, 1, s), ctx.h))
    _lib.check(lib.nhp_cont_model_set_latent_positions_every(ctx.h, model.h, 1 << 30), ctx.h)
    out["latent_network_step_without_positions_ms"] = timed(lambda s: _lib.check(lib.nhp_cont_latent_step(ctx.h, ds.h, model.h, 1, s), ctx.h))
    ex = C.c_int64()
    _lib.check(lib.nhp_cont_model_get_latent(ctx.h, model.h, None, None, None, None, C.byref(ex)), ctx.h)
    out["exhausted_in_chain"] = int(ex.value)

    # the two parts by themselves, on the model's own A: n extra sweeps (or offset updates) in one call
    def standalone(n_sweeps, do_offset, want_attempts=False):
        z, b = z0.copy(), C.c_double(truth.b)
        att = np.zeros(max(1, n_sweeps) * (N + 1 if n_sweeps else 1), dtype=np.int32) if want_attempts else None
        t0 = time.perf_counter()
        _lib.check(lib.nhp_latent_resample(ctx.h, _lib.dptr(_lib.colmajor(A)), N, D, _lib.dptr(z), C.byref(b), 1.0, 0.0, 2.0, None, 1, 0,
                                           n_sweeps, do_offset, None, None if att is None else att.ctypes.data, None, None), ctx.h)
        return 1e3 * (time.perf_counter() - t0), att
    standalone(1, 0)
    extra = 10
    out["position_sweep_ms"] = spread([(standalone(1 + extra, 0)[0] - standalone(1, 0)[0]) / extra for _ in range(runs)])
    out["sweep_and_offset_ms"] = spread([(standalone(1 + extra, 1)[0] - standalone(1, 1)[0]) / extra for _ in range(runs)])
    out["offset_update_ms"] = {k: (v if k == "runs" else v - out["position_sweep_ms"]["median"]) for k, v in out["sweep_and_offset_ms"].items()}
    att = standalone(extra, 1, want_attempts=True)[1].reshape((extra, N + 1))
    out["mean_attempts_per_node"] = float(att[:, :N].mean())
    out["max_attempts_per_node"] = int(att[:, :N].max())
    out["mean_attempts_offset"] = float(att[:, N].mean())
    out["share_of_node_steps_in_the_first_batch"] = float(np.mean(att[:, :N] <= 7))
    try:
        out["commit"] = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        out["commit"] = None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
