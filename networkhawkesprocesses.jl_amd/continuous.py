"""Continuous-time process models: host mirror of src/continuous.jl on top of libnhp.so.

Same entry points and argument meaning as the reference --
loglikelihood(process, data; recursive=true), intensity(process, data, times),
params / params!, resample_parents -- but every inner loop runs in a HIP kernel.
`data` is the reference's tuple (events sorted ascending, nodes 1-based, duration)
(src/continuous.jl:14,29-36).
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import DomainError
from .components import (BernoulliNetworkModel, DenseNetworkModel, ExponentialImpulseResponse,
                         HomogeneousProcess, LogGaussianCoxProcess, LogitNormalImpulseResponse, host_array, param_layout)


class HawkesProcess:
    pass


class ContinuousHawkesProcess(HawkesProcess):
    def ndims(self):
        return self.baseline.ndims()

    # ---- lowering: components -> nhp_cont_model_desc
    def lower(self):
        N = self.ndims()
        keep = {}
        d = _lib.ModelDesc()
        d.n_nodes = N
        if isinstance(self.baseline, HomogeneousProcess):
            d.baseline_kind, d.grid_n = _lib.BASELINE_HOMOGENEOUS, 0
            keep["l0"] = _lib.f64(self.baseline.λ)
        elif isinstance(self.baseline, LogGaussianCoxProcess):
            d.baseline_kind, d.grid_n = _lib.BASELINE_LGCP, len(self.baseline.x)
            keep["l0"] = _lib.f64(np.concatenate(self.baseline.λ))
            keep["gx"] = _lib.f64(self.baseline.x)
            d.grid_x = _lib.dptr(keep["gx"])
        else:
            raise TypeError("unsupported baseline")
        if len(keep["l0"]) != (N if d.grid_n == 0 else N * d.grid_n):
            raise ValueError("Parameter vector length does not match model parameter length.")
        d.lambda0 = _lib.dptr(keep["l0"])
        imp = self.impulses
        if isinstance(imp, ExponentialImpulseResponse):
            d.impulse_kind = _lib.IMPULSE_EXPONENTIAL
            keep["th"] = _lib.colmajor(imp.θ)
            d.theta = _lib.dptr(keep["th"])
            shapes = [imp.θ.shape]
        elif isinstance(imp, LogitNormalImpulseResponse):
            d.impulse_kind = _lib.IMPULSE_LOGITNORMAL
            keep["mu"], keep["tau"] = _lib.colmajor(imp.μ), _lib.colmajor(imp.τ)
            d.mu, d.tau = _lib.dptr(keep["mu"]), _lib.dptr(keep["tau"])
            shapes = [imp.μ.shape, imp.τ.shape]
        else:
            raise TypeError("unsupported impulse response")
        d.dt_max = float(imp.Δtmax)
        keep["W"] = _lib.colmajor(self.weights.W)
        d.W = _lib.dptr(keep["W"])
        shapes.append(self.weights.W.shape)
        A = getattr(self, "adjacency_matrix", None)
        if A is not None:
            keep["A"] = _lib.colmajor(np.asarray(A, dtype=np.float64))
            d.A = _lib.dptr(keep["A"])
            shapes.append(np.asarray(A).shape)
        if any(s != (N, N) for s in shapes):
            raise ValueError("Parameter vector length does not match model parameter length.")
        return d, keep

    def device_model(self, ctx=None):
        """Create (first call) or refresh the device-resident parameter blob."""
        ctx = ctx or _lib.default_context()
        d, keep = self.lower()
        cached = getattr(self, "_dev", None)
        if cached is not None and cached.ctx is ctx and cached.signature == _signature(d):
            cached.update(d)
        else:
            self._dev = cached = DeviceModel(ctx, d)
        del keep
        return cached


def _signature(d):
    return (d.n_nodes, d.baseline_kind, d.grid_n, d.impulse_kind, bool(d.A))


class DeviceModel:
    """nhp_cont_model handle."""

    def __init__(self, ctx, desc):
        self.ctx, self.signature = ctx, _signature(desc)
        h = C.c_void_p()
        _lib.check(_lib.lib().nhp_cont_model_create(ctx.h, C.byref(desc), C.byref(h)), ctx.h)
        self.h = h
        self._fin = weakref.finalize(self, _lib.lib().nhp_cont_model_destroy, h)

    def update(self, desc):
        _lib.check(_lib.lib().nhp_cont_model_update(self.ctx.h, self.h, C.byref(desc)), self.ctx.h)

    def set_params(self, x):
        x = _lib.f64(x)
        _lib.check(_lib.lib().nhp_cont_model_set_params(self.ctx.h, self.h, _lib.dptr(x), len(x)), self.ctx.h)

    def simulate(self, duration, seed=0, max_events=5_000_000, return_parents=False):
        """rand(process, duration) from the parameters this handle holds on the device (nhp_cont_simulate): (times, nodes,
        duration), float64 / int64 torch tensors on the context's device, with `parents` (0 = baseline event, else the
        1-based index of the parent) appended when return_parents.  More than max_events kept events raise RuntimeError."""
        import torch
        duration, max_events = float(duration), int(max_events)
        if not 0 <= max_events < 2 ** 31:
            raise ValueError(f"max_events = {max_events} outside [0, 2^31)")
        dev = torch.device("cuda", self.ctx.device)
        cap = max(max_events, 1)
        t = torch.empty(cap, dtype=torch.float64, device=dev)
        nd = torch.empty(cap, dtype=torch.int64, device=dev)
        par = torch.empty(cap, dtype=torch.int64, device=dev) if return_parents else None
        torch.cuda.current_stream(dev).synchronize()          # earlier users of the buffers' memory are done before the library writes
        n = C.c_int64()
        _lib.check(_lib.lib().nhp_cont_simulate(self.ctx.h, self.h, duration, int(seed) & (2 ** 64 - 1), max_events, 1, t.data_ptr(),
                                                nd.data_ptr(), par.data_ptr() if return_parents else None, C.byref(n)), self.ctx.h)
        k = n.value
        out = (t[:k].clone(), nd[:k].clone(), duration)
        return out + (par[:k].clone(),) if return_parents else out


_CHILD = np.dtype([("t", np.float64), ("first", np.int32), ("idx", np.int32)])
# nhp_cont_dataset_export: name -> (NHP_DS_* id, element type)
DATASET_ARRAYS = {
    "times": (0, np.dtype(np.float64)), "nodes": (1, np.dtype(np.int32)),
    "ev": (2, np.dtype([("t", np.float64), ("node", np.int32), ("pad", np.int32)])), "ev8": (3, np.dtype(np.uint64)),
    "poff": (4, np.dtype(np.uint32)), "sl_row": (5, np.dtype(np.uint32)), "sl_item0": (6, np.dtype(np.int32)),
    "child": (7, _CHILD), "child_w": (8, _CHILD), "wpos": (9, np.dtype(np.int32)), "boff": (10, np.dtype(np.int32)),
    "items": (11, np.dtype([("node", np.int32), ("kbeg", np.int32), ("kend", np.int32), ("first", np.int32)])),
    "cnt": (12, np.dtype(np.float64)), "pair_off": (13, np.dtype(np.int64)),
    "child_cut": (14, _CHILD),
}
# nhp_cont_dataset_scalars, in order (the last three are the bit patterns of doubles)
DATASET_SCALARS = ("M", "N", "pairs", "group", "n_items", "max_item", "max_window", "n_zero_time", "all_sole", "sl_rows",
                   "n_slices", "sl_nb", "sl_max_rows", "t_last", "ev8_t0", "ev8_scale")


def _is_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def _on_device(x):
    return _is_tensor(x) and x.device.type != "cpu"


def _device_tensors(events, nodes, ctx):
    """The (events, nodes) of a torch data triple, checked for the device route: float64 / int64, 1-D, contiguous, both on
    ctx's device."""
    if not (_is_tensor(events) and _is_tensor(nodes)):
        raise ValueError("events and nodes must both be torch tensors on the context's device, or both host arrays")
    for name, t, dt in (("events", events, "float64"), ("nodes", nodes, "int64")):
        if str(t.dtype) != "torch." + dt:
            raise TypeError(f"{name} must be a {dt} tensor, got {t.dtype}")
        if t.device.type != "cuda" or t.device.index != ctx.device:
            raise ValueError(f"{name} is on {t.device}, the context on cuda:{ctx.device}")
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{name} must be a 1-D contiguous tensor")
    if events.numel() != nodes.numel():
        raise ValueError("events and nodes must have the same length")
    return events, nodes


class StackedEvents:
    """Several independent trials as one recording on a stacked clock (stack_event_trials): trial r owns the events
    [event_offsets[r], event_offsets[r + 1]) and the interval [time_offsets[r], time_offsets[r + 1]] of the clock;
    `events` are the stacked times, `duration` = time_offsets[-1].  Unpacks like the triple (events, nodes, duration)."""

    def __init__(self, events, nodes, duration, event_offsets, time_offsets):
        self.events, self.nodes, self.duration = events, nodes, float(duration)
        self.event_offsets = np.ascontiguousarray(event_offsets, dtype=np.int64)
        self.time_offsets = np.ascontiguousarray(time_offsets, dtype=np.float64)

    @property
    def ntrials(self):
        return len(self.event_offsets) - 1

    def __iter__(self):
        return iter((self.events, self.nodes, self.duration))

    def __getitem__(self, k):
        return (self.events, self.nodes, self.duration)[k]

    def __len__(self):
        return 3

    def __repr__(self):
        return f"StackedEvents(trials={self.ntrials}, events={int(self.event_offsets[-1])}, duration={self.duration:g})"


def _is_trial_list(data):
    """A Python list whose entries are all 3-tuples: trials.  (A 3-tuple, or a list [events, nodes, duration], is one
    recording, as ever.)"""
    return isinstance(data, list) and len(data) > 0 and all(isinstance(tr, tuple) and len(tr) == 3 for tr in data)


def stack_event_trials(trials):
    """Stack independent trials [(events_r, nodes_r, T_r), ...] over the same nodes along one clock -> StackedEvents.  Trial r
    takes the interval [o_r, o_r + T_r] with o_0 = 0, o_{r+1} = o_r + T_r, and its events move to o_r + t.  A trial may be empty
    (it then adds exposure only), T_r must be positive and finite, and the events of a trial sorted inside [0, T_r].

    The shift rounds every time once: a delay between two events of one trial changes by at most one ulp of ΣT_r (not at all
    when times and durations are multiples of one power of two and ΣT_r stays below 2^53 of them).

    Host arrays are stacked with numpy; when every trial's events and nodes are torch tensors on one device they are stacked
    there and never cross to the host (the checks then cost one small read-back per trial)."""
    if isinstance(trials, StackedEvents):
        return trials
    if not isinstance(trials, (list, tuple)) or len(trials) == 0:
        raise ValueError("trials must be a non-empty list of (events, nodes, duration) tuples")
    for r, tr in enumerate(trials):
        if not isinstance(tr, (tuple, list)) or len(tr) != 3:
            raise ValueError(f"trial {r} is not an (events, nodes, duration) tuple")
    on_dev = [_on_device(tr[0]) or _on_device(tr[1]) for tr in trials]
    if any(on_dev) and not all(_on_device(tr[0]) and _on_device(tr[1]) for tr in trials):
        raise ValueError("the trials' events and nodes must all be torch tensors on one device, or all host arrays")
    device = all(on_dev)
    f, o = np.zeros(len(trials) + 1, dtype=np.int64), np.zeros(len(trials) + 1)
    ev, nd = [], []
    for r, (e, n, T) in enumerate(trials):
        T = float(T)
        if not (np.isfinite(T) and T > 0.0):
            raise DomainError(f"trial {r}: duration {T} must be positive and finite")
        if device:
            import torch
            if e.dim() != 1 or n.dim() != 1 or e.numel() != n.numel():
                raise ValueError(f"trial {r}: events and nodes must be 1-D and of the same length")
            if e.device != n.device or e.device != trials[0][0].device:
                raise ValueError(f"trial {r}: every tensor must be on the same device")
            e, n = e.to(torch.float64), n.to(torch.int64)
            if e.numel():
                bad = torch.stack([(e[1:] < e[:-1]).any(), (e < 0.0).any() | (e > T).any() | torch.isnan(e).any()]).cpu().numpy()
            else:
                bad = (False, False)
        else:
            e, n = host_array(e, np.float64), np.asarray(host_array(n, np.int64))
            if e.ndim != 1 or n.ndim != 1 or len(e) != len(n):
                raise ValueError(f"trial {r}: events and nodes must be 1-D and of the same length")
            bad = (bool(np.any(e[1:] < e[:-1])), not bool(np.all((e >= 0.0) & (e <= T))))
        if bad[0]:
            raise ValueError(f"trial {r}: events must be sorted")
        if bad[1]:
            raise DomainError(f"trial {r}: events must lie in [0, {T}]")
        o[r + 1] = o[r] + T
        f[r + 1] = f[r] + len(e)
        ev.append(e + o[r])
        nd.append(n)
    if not np.isfinite(o[-1]):
        raise DomainError("the durations of the trials do not add up to a finite number")
    if device:
        import torch
        return StackedEvents(torch.cat(ev).contiguous(), torch.cat(nd).contiguous(), o[-1], f, o)
    return StackedEvents(np.ascontiguousarray(np.concatenate(ev), dtype=np.float64),
                         np.ascontiguousarray(np.concatenate(nd), dtype=np.int64), o[-1], f, o)


def as_data(data):
    """`data` as the entry points take it: a list of (events, nodes, duration) tuples becomes a StackedEvents; anything else is
    returned as is.  Nothing is kept: a caller that evaluates the same trials again and again stacks them once itself
    (stack_event_trials) and passes the StackedEvents, or the DeviceDataset, whose device copy device_dataset then reuses."""
    return stack_event_trials(data) if _is_trial_list(data) else data


def ntrials_of(data):
    """How many trials `data` holds, without stacking or uploading anything."""
    if isinstance(data, (DeviceDataset, StackedEvents)):
        return data.ntrials
    return len(data) if _is_trial_list(data) else 1


class DeviceDataset:
    """nhp_cont_dataset handle: (events, nodes, duration) uploaded once, pre-pass done for Δtmax."""

    def __init__(self, ctx, data, nnodes, Δtmax, columns=None, build="host", trial_offsets=None):
        """columns = (begin, end), 0-based half-open: a column shard (sharded.py) that evaluates only the children on
        those nodes; None = the whole dataset.  build = "host" (the pre-pass on the host) or "device" (on the GPU,
        nhp_cont_dataset_create_device: the same dataset, byte for byte).  events / nodes given as torch tensors on
        ctx's device always take the device route and are copied on the device; no host copy is kept."""
        if build not in ("host", "device"):
            raise ValueError(f'build must be "host" or "device", not {build!r}')
        data = as_data(data)
        if trial_offsets is None and isinstance(data, StackedEvents):
            trial_offsets = (data.event_offsets, data.time_offsets)
        events, nodes, duration = data
        if trial_offsets is not None:
            if columns is not None and tuple(columns) != (0, int(nnodes)):
                raise NotImplementedError("a dataset of trials is a whole dataset: no column shard (sharded.ShardedDataset)")
            self._init_trials(ctx, events, nodes, nnodes, Δtmax, build, trial_offsets)
            return
        self.duration, self.Δtmax, self.nnodes, self.ctx = float(duration), float(Δtmax), int(nnodes), ctx
        h = C.c_void_p()
        self.columns = (0, int(nnodes)) if columns is None else (int(columns[0]), int(columns[1]))
        lib = _lib.lib()
        if _on_device(events) or _on_device(nodes):
            import torch
            ev, nd = _device_tensors(events, nodes, ctx)
            self.events = self.nodes = None
            self.M, self.build = int(ev.numel()), "device"
            torch.cuda.current_stream(ev.device).synchronize()      # the producer's work is done before the library reads
            rc = lib.nhp_cont_dataset_create_device(ctx.h, ev.data_ptr(), nd.data_ptr(), self.M, nnodes, self.duration,
                                                    self.Δtmax, self.columns[0], self.columns[1], 1, C.byref(h))
        else:
            self.events = _lib.f64(host_array(events, np.float64))
            self.nodes = np.ascontiguousarray(host_array(nodes, np.int64))
            if len(self.events) != len(self.nodes):
                raise ValueError("events and nodes must have the same length")
            self.M, self.build = len(self.events), build
            if build == "device":
                rc = lib.nhp_cont_dataset_create_device(ctx.h, self.events.ctypes.data, self.nodes.ctypes.data, self.M, nnodes,
                                                        self.duration, self.Δtmax, self.columns[0], self.columns[1], 0,
                                                        C.byref(h))
            else:
                rc = lib.nhp_cont_dataset_create_columns(ctx.h, _lib.dptr(self.events), _lib.iptr(self.nodes), self.M, nnodes,
                                                         self.duration, self.Δtmax, self.columns[0], self.columns[1],
                                                         C.byref(h))
        _lib.check(rc, ctx.h)
        self.h = h
        self._fin = weakref.finalize(self, _lib.lib().nhp_cont_dataset_destroy, h)

    def _init_trials(self, ctx, events, nodes, nnodes, Δtmax, build, trial_offsets):
        """trial_offsets = (event_offsets, time_offsets), R + 1 entries each, over stacked times (StackedEvents;
        nhp_cont_dataset_create_trials, which checks them).  duration = time_offsets[-1]."""
        f = np.ascontiguousarray(trial_offsets[0], dtype=np.int64)
        o = np.ascontiguousarray(trial_offsets[1], dtype=np.float64)
        if f.ndim != 1 or o.ndim != 1 or len(f) != len(o) or len(f) < 2:
            raise ValueError("trial_offsets = (event_offsets, time_offsets): two 1-D tables of R + 1 entries, R >= 1")
        self.duration, self.Δtmax, self.nnodes, self.ctx = float(o[-1]), float(Δtmax), int(nnodes), ctx
        self.columns = (0, int(nnodes))
        h = C.c_void_p()
        lib = _lib.lib()
        if _on_device(events) or _on_device(nodes):
            import torch
            ev, nd = _device_tensors(events, nodes, ctx)
            self.events = self.nodes = None
            self.M, self.build = int(ev.numel()), "device"
            torch.cuda.current_stream(ev.device).synchronize()      # the producer's work is done before the library reads
            ep, np_, where = ev.data_ptr(), nd.data_ptr(), 2
        else:
            self.events = _lib.f64(host_array(events, np.float64))
            self.nodes = np.ascontiguousarray(host_array(nodes, np.int64))
            if len(self.events) != len(self.nodes):
                raise ValueError("events and nodes must have the same length")
            self.M, self.build = len(self.events), build
            ep, np_, where = self.events.ctypes.data, self.nodes.ctypes.data, 1 if build == "device" else 0
        _lib.check(lib.nhp_cont_dataset_create_trials(ctx.h, ep, np_, self.M, nnodes, _lib.iptr(f), _lib.dptr(o), len(f) - 1,
                                                      self.Δtmax, where, C.byref(h)), ctx.h)
        self.h = h
        self._fin = weakref.finalize(self, _lib.lib().nhp_cont_dataset_destroy, h)

    def trials(self):
        """(event_offsets [R + 1], time_offsets [R + 1], first_positive [R]) of the dataset (nhp_cont_dataset_get_trials);
        one recording is one trial."""
        n = C.c_int32()
        lib = _lib.lib()
        _lib.check(lib.nhp_cont_dataset_get_trials(self.h, C.byref(n), None, None, None), self.ctx.h)
        f, o, g = np.empty(n.value + 1, dtype=np.int64), np.empty(n.value + 1), np.empty(n.value, dtype=np.int64)
        _lib.check(lib.nhp_cont_dataset_get_trials(self.h, C.byref(n), _lib.iptr(f), _lib.dptr(o), _lib.iptr(g)), self.ctx.h)
        return f, o, g

    @property
    def ntrials(self):
        n = C.c_int32()
        _lib.check(_lib.lib().nhp_cont_dataset_get_trials(self.h, C.byref(n), None, None, None), self.ctx.h)
        return n.value

    def trial_events(self, r):
        """(first, end): the events [first, end) of trial r."""
        f = self.trials()[0]
        return int(f[r]), int(f[r + 1])

    def trial_interval(self, r):
        """(start, end) of trial r on the stacked clock."""
        o = self.trials()[1]
        return float(o[r]), float(o[r + 1])

    def __len__(self):
        return self.M

    @property
    def pairs(self):
        return _lib.lib().nhp_cont_dataset_pairs(self.h)

    def scalars(self):
        """The dataset's scalars (DATASET_SCALARS) as a dict of ints; t_last, ev8_t0, ev8_scale as float64 bit patterns."""
        buf = (C.c_int64 * len(DATASET_SCALARS))()
        _lib.check(_lib.lib().nhp_cont_dataset_scalars(self.h, buf, len(buf)), self.ctx.h)
        return dict(zip(DATASET_SCALARS, (int(v) for v in buf)))

    def array(self, name):
        """One of the dataset's arrays (DATASET_ARRAYS) as a host numpy copy; empty if the dataset has none."""
        which, dt = DATASET_ARRAYS[name]
        n = C.c_int64()
        lib = _lib.lib()
        _lib.check(lib.nhp_cont_dataset_export(self.ctx.h, self.h, which, None, 0, C.byref(n)), self.ctx.h)
        out = np.empty(n.value, dtype=np.uint8)
        if n.value:
            _lib.check(lib.nhp_cont_dataset_export(self.ctx.h, self.h, which, out.ctypes.data, n.value, C.byref(n)), self.ctx.h)
        return out.view(dt)

    def layout(self):
        """Every exported array and the scalars: {"arrays": {name: ndarray}, "scalars": {name: int}} (tests, tools)."""
        return {"arrays": {k: self.array(k) for k in DATASET_ARRAYS}, "scalars": self.scalars()}


_ds_cache = {}


def device_dataset(process, data, ctx=None, build="host"):
    """Upload `data` once per (arrays, Δtmax); repeated calls (mle!, mcmc!) reuse the device copy.  build = "host" |
    "device" picks where the pre-pass runs for host arrays (DeviceDataset); torch tensors on the context's device always
    take the device route."""
    if isinstance(data, DeviceDataset):
        return data
    ctx = ctx or _lib.default_context()
    if isinstance(process.baseline, LogGaussianCoxProcess) and ntrials_of(data) > 1:
        raise NotImplementedError("a LogGaussianCoxProcess baseline is not available on several trials: its grid spans one recording")
    N, Δtmax = process.ndims(), float(process.impulses.Δtmax)
    if _is_trial_list(data):            # stacked for this call and not kept (as_data): the list may change between calls
        return DeviceDataset(ctx, as_data(data), N, Δtmax, build=build)
    events, nodes, duration = data
    trials = isinstance(data, StackedEvents)
    offsets = (data.event_offsets.tobytes(), data.time_offsets.tobytes()) if trials else None
    if _on_device(events) or _on_device(nodes):
        # (data_ptr, numel, version): an in-place refill of the tensors bumps their version and so builds again
        key = ("tensor", events.data_ptr(), events.numel(), events._version, nodes.data_ptr(), nodes.numel(), nodes._version,
               float(duration), Δtmax, N, id(ctx), offsets)
        hit = _ds_cache.get(key)
        if hit is not None and hit[1]() is events and hit[2]() is nodes:
            return hit[0]
        ds = DeviceDataset(ctx, data, N, Δtmax, build="device")
        if len(_ds_cache) > 16:
            _ds_cache.clear()
        _ds_cache[key] = (ds, weakref.ref(events), weakref.ref(nodes))
        return ds
    key = (id(events), id(nodes), len(events), float(duration), Δtmax, N, id(ctx), build, offsets)
    hit = _ds_cache.get(key)
    # the arrays may have been refilled in place since the upload (a preallocated buffer reused for the next dataset):
    # a cheap content fingerprint decides, not the identity alone
    if hit is not None and hit[1]() is events and hit[2] == _fingerprint(events, nodes):
        return hit[0]
    ds = DeviceDataset(ctx, data, N, Δtmax, build=build)
    try:
        ref = weakref.ref(events)
    except TypeError:
        return ds          # plain lists cannot be weak-referenced: no caching
    if len(_ds_cache) > 16:
        _ds_cache.clear()
    _ds_cache[key] = (ds, ref, _fingerprint(events, nodes))
    return ds


def _fingerprint(events, nodes):
    """First, last and sum of the events, sum of the nodes, and a strided sample of both: O(M) adds (≈1 ms at M = 10⁶)
    against an upload + pre-pass of tens of ms; not a hash, but any refill of the buffers changes it."""
    e, n = np.asarray(events), np.asarray(nodes)
    if len(e) == 0:
        return (0,)
    return (float(e[0]), float(e[-1]), float(e.sum()), int(n.sum()), float(e[::97].sum()), int(n[::89].sum()))


def invalidate_device_datasets():
    """Forget every cached device copy (call after mutating data arrays in place if in doubt)."""
    _ds_cache.clear()


class ContinuousStandardHawkesProcess(ContinuousHawkesProcess):
    """ContinuousStandardHawkesProcess(baseline, impulses, weights) -- src/continuous.jl:108-112."""

    def __init__(self, baseline, impulses, weights):
        self.baseline, self.impulses, self.weights = baseline, impulses, weights

    def isstable(self):
        """src/continuous.jl:114"""
        return np.max(np.abs(np.linalg.eigvals(self.weights.W))) < 1.0

    def params(self):
        """[baseline; impulses; weights] -- src/continuous.jl:116-119"""
        return np.concatenate([self.baseline.params(), self.impulses.params(), self.weights.params()])

    def params_(self, x):
        """params!(process, x) -- src/continuous.jl:121-129"""
        nb, nw, ni = len(self.baseline.params()), len(self.weights.params()), len(self.impulses.params())
        x = np.asarray(x, dtype=np.float64)
        if len(x) != nb + ni + nw:
            raise ValueError("Parameter vector length does not match model parameter length.")
        self.baseline.params_(x[:nb])
        self.impulses.params_(x[nb:nb + ni])
        self.weights.params_(x[nb + ni:nb + ni + nw])


class ContinuousNetworkHawkesProcess(ContinuousHawkesProcess):
    """ContinuousNetworkHawkesProcess(baseline, impulses, weights, adjacency_matrix, network)
    -- src/continuous.jl:315-321."""

    def __init__(self, baseline, impulses, weights, adjacency_matrix, network):
        self.baseline, self.impulses, self.weights = baseline, impulses, weights
        self.adjacency_matrix = np.array(adjacency_matrix, dtype=np.float64)
        self.network = network

    def isstable(self):
        """src/continuous.jl:323"""
        return np.max(np.abs(np.linalg.eigvals(self.adjacency_matrix * self.weights.W))) < 1.0

    def params(self):
        """[ρ; λ0; W; θ; vec(A)] -- src/continuous.jl:325-333"""
        return np.concatenate([self.network.params(), self.baseline.params(), self.weights.params(),
                               self.impulses.params(), self.adjacency_matrix.ravel(order="F")])


def _check_recursive(process, recursive):
    return _lib.LL_RECURSIVE if (recursive and isinstance(process.impulses, ExponentialImpulseResponse)) else 0


def loglikelihood(process, data, recursive=True, ctx=None, model=None):
    """loglikelihood(process, data; recursive=true) -- src/continuous.jl:210-239,360-389.

    Exponential impulses with `recursive` take the O(M·N) recursion that ignores Δtmax
    (:212-214); everything else takes the windowed sum.  A `sharded.ShardedDataset` evaluates it on all ranks together.
    `model`: a device-resident model (process.device_model(ctx)) to evaluate as is, skipping the parameter upload
    that otherwise precedes every call."""
    from .sharded import ShardedDataset, sharded_loglikelihood
    if isinstance(data, ShardedDataset):
        return sharded_loglikelihood(process, data, recursive=recursive, model=model)
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    model = model or process.device_model(ctx)
    ll = C.c_double()
    _lib.check(_lib.lib().nhp_cont_loglik(ctx.h, ds.h, model.h, _check_recursive(process, recursive), C.byref(ll)), ctx.h)
    return ll.value


def total_intensity(process, data, ctx=None):
    """total_intensity for every event -- src/continuous.jl:286-300,391-405 (vectorised)."""
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    model = process.device_model(ctx)
    out = np.empty(len(ds))
    _lib.check(_lib.lib().nhp_cont_event_intensity(ctx.h, ds.h, model.h, _lib.dptr(out)), ctx.h)
    return out


def intensity(process, data, times, ctx=None):
    """intensity(process, data, times) -> len(times) x N; a scalar time gives a length-N vector
    -- src/continuous.jl:76-96."""
    if ntrials_of(data) > 1:            # (before a context is made or anything is stacked or uploaded)
        raise NotImplementedError("intensity at query times is not available on several trials (a stacked query time names "
                                  "no trial): evaluate the trial alone")
    ctx = ctx or _lib.default_context()
    scalar = np.isscalar(times)
    q = _lib.f64(np.atleast_1d(times))
    if isinstance(process.baseline, HomogeneousProcess) and np.any(q < 0):
        raise DomainError("time must be non-negative")
    ds = device_dataset(process, data, ctx)
    model = process.device_model(ctx)
    N = process.ndims()
    out = np.empty((N, len(q)))
    _lib.check(_lib.lib().nhp_cont_intensity(ctx.h, ds.h, model.h, _lib.dptr(q), len(q), _lib.dptr(out)), ctx.h)
    res = out.T.copy()
    return res[0] if scalar else res


def gradient_length(process):
    """len(params(process)) of the standard process, without building the vector (three column-major N x N copies)."""
    return param_layout(process).weights.stop


def loglikelihood_gradient(process, data, recursive=True, ctx=None, model=None):
    """(ll, ∇ll) with the gradient in params! order [λ0; θ | μ; τ; W].  The reference supplies no
    gradient to Optim (src/continuous.jl:190), which then spends 2P objective calls on finite
    differences; this is one fused pass."""
    from .sharded import ShardedDataset, sharded_loglikelihood_gradient
    if isinstance(data, ShardedDataset):
        return sharded_loglikelihood_gradient(process, data, recursive=recursive, model=model)
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    model = model or process.device_model(ctx)
    P = gradient_length(process)
    g = np.empty(P)
    ll = C.c_double()
    _lib.check(_lib.lib().nhp_cont_loglik_grad(ctx.h, ds.h, model.h, _check_recursive(process, recursive),
                                               C.byref(ll), _lib.dptr(g), P), ctx.h)
    return ll.value, g


class Compensator:
    """Result of compensator(): at_events [M] and residuals [M] in the order of the events, total [N] (numpy arrays, or
    float64 torch tensors on the context's device)."""

    def __init__(self, at_events, residuals, total):
        self.at_events, self.residuals, self.total = at_events, residuals, total

    def __iter__(self):
        return iter((self.at_events, self.residuals, self.total))

    def __repr__(self):
        return f"Compensator(events={len(self.at_events)}, nodes={len(self.total)})"


def _continuous_only(process, what):
    if not isinstance(process, ContinuousHawkesProcess):
        raise TypeError(f"{what} takes a ContinuousStandardHawkesProcess or a ContinuousNetworkHawkesProcess, "
                        f"not {type(process).__name__}")


def compensator(process, data, ctx=None, model=None, device=False):
    """The exact compensator Λ_c(t) = ∫₀ᵗ λ_c(s) ds of the intensity that intensity(process, data, t) evaluates
    (src/continuous.jl:84-96; strict window, cut exponential, logit-normal pdf not divided by Δtmax), nhp_cont_compensator:

        at_events[k] = Λ_{n_k}(t_k);  residuals[k] = Λ_{n_k}(t_k) - Λ_{n_k}(previous event of node n_k)  (Exp(1) under the
        true model: time rescaling);  total[c] = Λ_c(duration), the expected number of events of node c.

    device=False: numpy arrays.  device=True: float64 torch tensors on the context's device -- with `data` as device
    tensors (rand(..., device=True)) no event crosses to the host.  `model`: a device-resident model to evaluate as is."""
    from .sharded import ShardedDataset
    _continuous_only(process, "compensator")
    if isinstance(data, ShardedDataset):
        raise NotImplementedError("compensator: not available on a column shard (sharded.ShardedDataset)")
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    model = model or process.device_model(ctx)
    M, N = len(ds), process.ndims()
    fn = _lib.lib().nhp_cont_compensator
    if device:
        import torch
        dev = torch.device("cuda", ctx.device)
        at, res, tot = (torch.empty(n, dtype=torch.float64, device=dev) for n in (M, M, N))
        torch.cuda.current_stream(dev).synchronize()          # earlier users of the buffers' memory are done before the library writes
        _lib.check(fn(ctx.h, ds.h, model.h, 1, at.data_ptr(), res.data_ptr(), tot.data_ptr()), ctx.h)
    else:
        at, res, tot = np.empty(M), np.empty(M), np.empty(N)
        _lib.check(fn(ctx.h, ds.h, model.h, 0, at.ctypes.data, res.ctypes.data, tot.ctypes.data), ctx.h)
    return Compensator(at, res, tot)


class Forecast:
    """Result of forecast(): counts [S, N] int64 (events of node c in (T, T + horizon] in replica r), carry [N] (the
    expected number of carry-over events per node), paths = None or (times, nodes, offsets): replica r owns
    [offsets[r], offsets[r + 1]) of the absolute, ascending times and the 1-based nodes.  numpy arrays, or torch tensors
    on the context's device."""

    def __init__(self, counts, carry, paths, duration, horizon, phase_ms=None):
        self.counts, self.carry, self.paths, self.duration, self.horizon, self.phase_ms = counts, carry, paths, duration, horizon, phase_ms

    def __iter__(self):
        return iter((self.counts, self.carry, self.paths))

    def __repr__(self):
        return f"Forecast(nsamples={self.counts.shape[0]}, nodes={self.counts.shape[1]}, paths={self.paths is not None})"

    def path(self, r):
        """(times, nodes) of replica r."""
        times, nodes, offsets = self.paths
        lo, hi = int(offsets[r]), int(offsets[r + 1])
        return times[lo:hi], nodes[lo:hi]


def forecast(process, data, horizon, nsamples=1000, seed=0, *, return_paths=False, device=False, max_events=5_000_000, ctx=None,
             model=None):
    """`nsamples` independent continuations of `data` = (events, nodes, T) on (T, T + horizon], conditional on the observed
    events (nhp_cont_forecast): the carry-over children of the observed events, new immigrants, and the descendants of both.
    The law is the generative model's, the one rand(process, duration) samples -- exponential delays are not cut at Δtmax
    and a link has W[p,c]·A[p,c] expected children for both impulse kinds -- not the likelihood's convention (compensator).
    Homogeneous baselines only: a LogGaussianCoxProcess grid ends where the data end.

    Returns Forecast(counts, carry, paths); paths only with return_paths.  device=False: numpy arrays; device=True: torch
    tensors on the context's device.  `data`: a host triple, a device-tensor triple or a DeviceDataset.  The sample depends on
    (process, data, horizon, nsamples, seed) only; replica r's draws are not the same for different nsamples.  `max_events`
    caps the events of all replicas together; past it RuntimeError ("branching process exploded").  A path appended to the
    history, with duration T + horizon, is data for loglikelihood and compensator."""
    from .sharded import ShardedDataset
    _continuous_only(process, "forecast")
    if isinstance(process.baseline, LogGaussianCoxProcess):
        raise NotImplementedError("forecast: not available with a LogGaussianCoxProcess baseline (the grid ends where the data end)")
    if isinstance(data, ShardedDataset):
        raise NotImplementedError("forecast: not available on a column shard (sharded.ShardedDataset)")
    if ntrials_of(data) > 1:            # (before a context is made or anything is stacked or uploaded)
        raise NotImplementedError("forecast is not available on several trials: a forecast continues one recording, pass the "
                                  "trial to continue")
    horizon, S, max_events = float(horizon), int(nsamples), int(max_events)
    if S != nsamples or S < 1:
        raise ValueError(f"nsamples = {nsamples} must be a positive integer")
    if not 0.0 <= horizon < float("inf"):
        raise DomainError(f"horizon must be non-negative and finite, got {horizon}")
    if not 0 <= max_events < 2 ** 31:
        raise ValueError(f"max_events = {max_events} outside [0, 2^31)")
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    model = model or process.device_model(ctx)
    N, cap = process.ndims(), max(max_events, 1)
    fn = _lib.lib().nhp_cont_forecast
    phase = np.zeros(2)
    seed = int(seed) & (2 ** 64 - 1)
    if device:
        import torch
        dev = torch.device("cuda", ctx.device)
        counts = torch.empty((S, N), dtype=torch.int64, device=dev)
        carry = torch.empty(N, dtype=torch.float64, device=dev)
        t = nd = off = None
        if return_paths:
            t = torch.empty(cap, dtype=torch.float64, device=dev)
            nd = torch.empty(cap, dtype=torch.int64, device=dev)
            off = torch.empty(S + 1, dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()          # earlier users of the buffers' memory are done before the library writes
        ptr = [x.data_ptr() if x is not None else None for x in (carry, counts, t, nd, off)]
    else:
        counts, carry = np.empty((S, N), dtype=np.int64), np.empty(N)
        t = nd = off = None
        if return_paths:
            t, nd, off = np.empty(cap), np.empty(cap, dtype=np.int64), np.empty(S + 1, dtype=np.int64)
        ptr = [x.ctypes.data if x is not None else None for x in (carry, counts, t, nd, off)]
    _lib.check(fn(ctx.h, ds.h, model.h, horizon, S, seed, max_events, 1 if device else 0, *ptr, _lib.dptr(phase)), ctx.h)
    paths = None
    if return_paths:
        n = int(off[-1])
        paths = (t[:n].clone(), nd[:n].clone(), off) if device else (t[:n].copy(), nd[:n].copy(), off)
    return Forecast(counts, carry, paths, ds.duration, horizon, phase_ms=(float(phase[0]), float(phase[1])))


def kolmogorov_pvalue(d, n):
    """P(D_n > d) of the one-sample Kolmogorov-Smirnov statistic: the asymptotic series at Stephens' effective
    x = d (√n + 0.12 + 0.11/√n)."""
    if not n or not np.isfinite(d):
        return float("nan")
    x = float(d) * (np.sqrt(n) + 0.12 + 0.11 / np.sqrt(n))
    if x < 0.2:
        return 1.0
    k = np.arange(1, 101)
    return float(min(1.0, max(0.0, 2.0 * np.sum((-1.0) ** (k - 1) * np.exp(-2.0 * k * k * x * x)))))


class TimeRescalingTest:
    """Kolmogorov-Smirnov test of the residuals against Exp(1): `statistic` / `pvalue` pooled over all events,
    `node_statistic` / `node_pvalue` [N] per node (NaN for a node without events), `counts` [N]."""

    def __init__(self, statistic, pvalue, node_statistic, node_pvalue, counts):
        self.statistic, self.pvalue, self.counts = statistic, pvalue, counts
        self.node_statistic, self.node_pvalue = node_statistic, node_pvalue

    def __repr__(self):
        return f"TimeRescalingTest(statistic={self.statistic:.4g}, pvalue={self.pvalue:.4g}, nodes={len(self.counts)})"


def _ks_sorted(u):
    """sup |F_n - U(0,1)| of an ascending sample (numpy array or torch tensor)."""
    n = len(u)
    if n == 0:
        return float("nan")
    if _is_tensor(u):
        import torch
        i = torch.arange(1, n + 1, dtype=torch.float64, device=u.device)
        return float(torch.maximum((i / n - u).max(), (u - (i - 1) / n).max()))
    i = np.arange(1, n + 1)
    return float(max(np.max(i / n - u), np.max(u - (i - 1) / n)))


def time_rescaling_test(process, data, ctx=None, model=None, device=None, residuals=None):
    """Time-rescaling goodness of fit: under the true model the residuals of compensator(process, data) are i.i.d. Exp(1),
    so u = 1 - exp(-residual) is uniform on (0, 1); returns the Kolmogorov-Smirnov statistic and p-value per node and
    pooled (TimeRescalingTest).  device (default: where the events are) sorts with torch on the GPU instead of numpy on the
    host; `residuals` reuses the result of an earlier compensator() call."""
    _continuous_only(process, "time_rescaling_test")
    data = as_data(data)
    events, nodes = data[0], data[1]
    if device is None:
        device = _on_device(events)
    if residuals is None:
        residuals = compensator(process, data, ctx=ctx, model=model, device=device).residuals
    N = process.ndims()
    if _is_tensor(residuals):
        import torch
        nd = nodes if _is_tensor(nodes) else torch.as_tensor(np.asarray(nodes, dtype=np.int64))
        nd = nd.to(residuals.device)
        u = -torch.expm1(-residuals)
        pooled = _ks_sorted(torch.sort(u).values)
        # per node: sort by (node, u) -- u lies in [0, 1], so node + u/2 orders both at once
        order = torch.argsort(nd.to(torch.float64) + 0.5 * u)
        us, counts = u[order], torch.bincount(nd - 1, minlength=N)
        counts_h = counts.cpu().numpy()
        off = np.concatenate([[0], np.cumsum(counts_h)])
        stats = np.array([_ks_sorted(us[off[c]:off[c + 1]]) for c in range(N)])
    else:
        nd = np.asarray(nodes.cpu() if _is_tensor(nodes) else nodes, dtype=np.int64)
        u = -np.expm1(-np.asarray(residuals, dtype=np.float64))
        pooled = _ks_sorted(np.sort(u))
        counts_h = np.bincount(nd - 1, minlength=N)
        stats = np.array([_ks_sorted(np.sort(u[nd == c + 1])) for c in range(N)])
    pvals = np.array([kolmogorov_pvalue(s, n) for s, n in zip(stats, counts_h)])
    return TimeRescalingTest(pooled, kolmogorov_pvalue(pooled, int(counts_h.sum())), stats, pvals, counts_h)
