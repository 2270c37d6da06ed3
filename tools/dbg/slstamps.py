"""Phase timeline of k_windowed_slices -- PAIR=1: of k_slices_batch<BLOCK, C, 2, DEFER>, one enqueued pair, stamped at the same
phase boundaries -- from a -DNHP_STAMP build (NHP_LIB=... python tools/dbg/slstamps.py): wave 0 of every
workgroup stamps s_memrealtime (100 MHz, the same clock on every XCD) at its start, after the column is staged, after its
slices, after the block sums, after the ticket (ENQUEUE=1: after the stores of the deferred exit); EVERY wave stamps the end of its own slices, and the spread between a
workgroup's first and last wave to finish is what the dealing of slices to waves (nhp_slice_of) is there to shrink: the early
waves wait at the block-sum barrier for the last one.  Times in us from the launch's first workgroup start."""
import os, sys, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import __graft_entry__ as e
nhp = e.load_package()
from nhp_amd import _lib
ctx = nhp.Context(0)
N, M = 1024, 1_000_000
times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=float(os.environ.get("KBAR", 8.0)))
proc = nhp.synthetic.s_metric_process(N, M, T, "exponential", 1.0)
if os.environ.get("PAIR"):
    # one pass of two, alone on the device: a single evaluation opens the streak (only inside a streak is an enqueue held) and has
    # long ended, unjoined, when the next enqueue is held and the one after it shares its pass; the pair's 1024 workgroups stamp last
    import time
    ds0, model, model2 = nhp.device_dataset(proc, (times, nodes, T), ctx), proc.device_model(ctx), proc.device_model(ctx)
    count = _lib.lib().nhp_debug_pair_launches
    count.restype, count.argtypes = C.c_int64, [C.c_void_p]
    for _ in range(5):
        p0 = int(count(ctx.h))
        _lib.check(_lib.lib().nhp_cont_loglik_enqueue(ctx.h, ds0.h, model.h, 0, 0), ctx.h)
        time.sleep(0.005)
        _lib.check(_lib.lib().nhp_cont_loglik_enqueue(ctx.h, ds0.h, model.h, 0, 1), ctx.h)
        _lib.check(_lib.lib().nhp_cont_loglik_enqueue(ctx.h, ds0.h, model2.h, 0, 2), ctx.h)
        ctx.synchronize()
        assert int(count(ctx.h)) - p0 == 1, "the two evaluations did not share a pass"
    print("one pass of two (k_slices_batch, deferred exit)")
elif os.environ.get("ENQUEUE"):                        # the enqueue route: its last stamp is the deferred exit (NHP_DEFER_FINALIZE=0: the ticket)
    ds0, model = nhp.device_dataset(proc, (times, nodes, T), ctx), proc.device_model(ctx)
    for _ in range(5):
        _lib.check(_lib.lib().nhp_cont_loglik_enqueue(ctx.h, ds0.h, model.h, 0, 0), ctx.h)
        ctx.synchronize()
else:
    for _ in range(5):
        nhp.loglikelihood(proc, (times, nodes, T), recursive=False, ctx=ctx)
n = 1024
buf = np.zeros(8 * n, dtype=np.uint64)
fn = _lib.lib().nhp_debug_stamps_slices
fn.restype = C.c_int
assert fn(buf.ctypes.data_as(C.POINTER(C.c_uint64)), 8 * n) == 0
st = buf.reshape(n, 8)[:, :5].astype(np.int64)
t = (st - st[:, 0].min()) / 100.0                   # us
names = ("start", "column staged", "slices done", "block sums done", "ticket drawn")
for k, name in enumerate(names):
    v = t[:, k]
    print(f"{name:18s} min {v.min():6.2f}  p10 {np.percentile(v, 10):6.2f}  p50 {np.percentile(v, 50):6.2f}  p90 {np.percentile(v, 90):6.2f}  max {v.max():6.2f}")
d = np.diff(t, axis=1)
for k, name in enumerate(("column staging", "slices (pair rows)", "log + block sums", "partials + ticket")):
    print(f"phase {name:20s} mean {d[:, k].mean():6.2f}  p10 {np.percentile(d[:, k], 10):6.2f}  p90 {np.percentile(d[:, k], 90):6.2f}")
print("workgroup lifetime mean %.2f us, max %.2f; last ticket at %.2f us after the first start" % ((t[:, 4] - t[:, 0]).mean(), (t[:, 4] - t[:, 0]).max(), t[:, 4].max()))
order = np.argsort(t[:, 0])
print("start time by dispatch order (every 128th workgroup):", " ".join(f"{t[order[i], 0]:.2f}" for i in range(0, n, 128)))

# every wave's end of slices: the waves that have a slice at all (w < slices of the item), workgroup by workgroup
ds = nhp.device_dataset(proc, (times, nodes, T), ctx)
sc = ds.scalars()
per_item = (sc["max_item"] + 63) // 64
B = 512 if per_item >= 12 else 256 if per_item >= 6 else 128 if per_item >= 3 else 64      # launch_slices' choice
if os.environ.get("NHP_SLICES_CFG"):
    B = int(os.environ["NHP_SLICES_CFG"].split(",")[0])
NW = B // 64
ns = np.diff(ds.array("sl_item0"))[:n]
wbuf = np.zeros(16 * n, dtype=np.uint64)
fw = _lib.lib().nhp_debug_stamps_slices_waves
fw.restype = C.c_int
assert fw(wbuf.ctypes.data_as(C.POINTER(C.c_uint64)), 16 * n) == 0
we = (wbuf.reshape(n, 16).astype(np.int64) - st[:, 0].min()) / 100.0
busy = np.arange(16)[None, :] < np.minimum(ns, NW)[:, None]
has = busy.any(axis=1)
first = np.where(busy, we, np.inf).min(axis=1)[has]
last = np.where(busy, we, -np.inf).max(axis=1)[has]
spread = last - first
print(f"{NW} waves per workgroup, {ns.mean():.2f} slices per item")
print(f"spread between a workgroup's first and last wave to end its slices: mean {spread.mean():6.2f}  p10 {np.percentile(spread, 10):6.2f}  "
      f"p50 {np.percentile(spread, 50):6.2f}  p90 {np.percentile(spread, 90):6.2f}  max {spread.max():6.2f} us")
since = we[has] - t[has, 1][:, None]                  # from the column's barrier to the wave's last slice
mean_w = [float(since[busy[has][:, w], w].mean()) if busy[has][:, w].any() else float("nan") for w in range(NW)]
print("slices phase by wave (mean us after the column is staged):", " ".join(f"{v:.2f}" for v in mean_w))
print(f"last wave {(last - t[has, 1]).mean():6.2f} us, mean wave {np.nanmean(np.where(busy[has], since, np.nan), axis=1).mean():6.2f} us after the column is staged")
