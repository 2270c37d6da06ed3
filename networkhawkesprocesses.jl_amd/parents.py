"""Parent assignment (host mirror of src/parents.jl:1-79 on top of libnhp.so)."""
import ctypes as C

import numpy as np

from . import _lib
from .continuous import DeviceDataset, _continuous_only, _is_tensor, _on_device, as_data, device_dataset


def resample_parents(process, data, u=None, seed=0, step=0, with_stats=False, want_parents=True, ctx=None):
    """resample_parents(process, data) -> (parents, parentnodes) -- src/parents.jl:1-23.

    parents[i] is the 1-based index of the sampled parent event (0 = baseline), parentnodes[i]
    its node (0 = baseline).  The reference draws from Julia's task-local RNG, which is not
    reproducible under threads; here the uniform stream is explicit: `u` (one value per event) or
    Philox4x32-10 keyed (seed, step, event index).  With `with_stats` the Gibbs sufficient
    statistics (src/baselines.jl:87-96, src/parents.jl:61-79, src/impulses.jl:84-96,216-252) come
    back from the same call as a dict of [parent, child]-indexed arrays."""
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    model = process.device_model(ctx)
    M, N = len(ds), process.ndims()
    parents = np.empty(M, dtype=np.int64) if want_parents else None
    pnodes = np.empty(M, dtype=np.int64) if want_parents else None
    uu = None if u is None else _lib.f64(u)
    if uu is not None and len(uu) != M:
        raise ValueError("u must hold one uniform per event")
    st, keep = None, {}
    if with_stats:
        keep = {k: np.empty(N if k in ("cnt0", "Mn") else N * N) for k in ("cnt0", "Mn", "Mnm", "Xnm", "Vnm")}
        st = _lib.Stats(*[_lib.dptr(keep[k]) for k in ("cnt0", "Mn", "Mnm", "Xnm", "Vnm")])
    _lib.check(_lib.lib().nhp_cont_resample_parents(
        ctx.h, ds.h, model.h, _lib.dptr(uu), seed, step, _lib.iptr(parents), _lib.iptr(pnodes),
        C.byref(st) if st is not None else None), ctx.h)
    if not with_stats:
        return parents, pnodes
    stats = {k: (v if k in ("cnt0", "Mn") else v.reshape((N, N), order="F")) for k, v in keep.items()}
    return parents, pnodes, stats


def _whole_dataset(data, what):
    from .sharded import ShardedDataset
    if isinstance(data, ShardedDataset):
        raise NotImplementedError(f"{what}: not available on a column shard (sharded.ShardedDataset)")


def map_parents(process, data, device=False, ctx=None, model=None):
    """map_parents(process, data) -> (parents, parentnodes, prob): the posterior-mode parent of every event under the
    categories resample_parents draws from (the events of the look-back window, most recent first, then the baseline) and
    its posterior probability w_max / Σw (nhp_cont_map_parents).  parents[i] is the 1-based index of the most likely
    parent event (0 = baseline), parentnodes[i] its node (0 = baseline).  The first maximum wins: of equal parent weights
    the most recent, a parent before the baseline.

    device=False: numpy arrays.  device=True: int64 / float64 torch tensors on the context's device -- with `data` as device
    tensors (rand(..., device=True)) or a DeviceDataset nothing crosses to the host.  `model`: a device-resident model to
    evaluate as is."""
    _continuous_only(process, "map_parents")
    _whole_dataset(data, "map_parents")
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    model = model or process.device_model(ctx)
    M = len(ds)
    fn = _lib.lib().nhp_cont_map_parents
    if device:
        import torch
        dev = torch.device("cuda", ctx.device)
        par, pno = (torch.empty(M, dtype=torch.int64, device=dev) for _ in range(2))
        prob = torch.empty(M, dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()          # earlier users of the buffers' memory are done before the library writes
        _lib.check(fn(ctx.h, ds.h, model.h, 1, par.data_ptr(), pno.data_ptr(), prob.data_ptr()), ctx.h)
    else:
        par, pno, prob = np.empty(M, dtype=np.int64), np.empty(M, dtype=np.int64), np.empty(M)
        _lib.check(fn(ctx.h, ds.h, model.h, 0, par.ctypes.data, pno.ctypes.data, prob.ctypes.data), ctx.h)
    return par, pno, prob


class Cascades:
    """Result of cascades(): per event (in the order of the events) parents, root (1-based index of the immigrant ancestor),
    generation (0 = immigrant), descendants (events of the subtree, the event excluded); per cascade, in ascending root
    order, cascade_root, cascade_size (root included), cascade_depth (largest generation), cascade_end (time of the last
    event); per node immigrants [N], offspring [N] (Σ descendants over the node's events) and reach [N, N]: reach[p, c] =
    events on node c whose root is on node p, roots included.  numpy arrays, or torch tensors on the context's device;
    rounds = the pointer-doubling rounds the forest took."""

    FIELDS = ("parents", "root", "generation", "descendants", "cascade_root", "cascade_size", "cascade_depth", "cascade_end",
              "immigrants", "offspring", "reach")

    def __init__(self, rounds=0, **fields):
        self.rounds = rounds
        for k in self.FIELDS:
            setattr(self, k, fields[k])

    def __repr__(self):
        depth = int(self.cascade_depth.max()) if len(self.cascade_depth) else 0
        size = int(self.cascade_size.max()) if len(self.cascade_size) else 0
        return (f"Cascades(events={len(self.root)}, cascades={len(self.cascade_root)}, nodes={len(self.immigrants)}, "
                f"largest={size}, deepest={depth})")


def _event_count(data):
    if isinstance(data, DeviceDataset):
        return len(data)
    ev = as_data(data)[0]
    return int(ev.numel()) if _is_tensor(ev) else len(ev)


def cascades(process, data, parents="map", seed=0, device=False, ctx=None):
    """cascades(process, data, parents) -> Cascades: the forest a parent assignment forms on the events of `data`
    (nhp_cont_cascades).  parents = "map" (map_parents), "sample" (one draw of resample_parents with `seed`) or an integer
    array / device tensor of length M in the convention of resample_parents and rand(..., return_parents=True): 0 = immigrant,
    else the 1-based index of an earlier event (anything else raises DomainError, a ValueError).

    device=False: numpy arrays.  device=True: torch tensors on the context's device; a device tensor of parents with device
    data never crosses to the host."""
    _continuous_only(process, "cascades")
    _whole_dataset(data, "cascades")
    M = _event_count(data)
    if isinstance(parents, str):
        if parents not in ("map", "sample"):
            raise ValueError(f'parents must be "map", "sample" or an integer array of length {M}, not {parents!r}')
    else:
        if _is_tensor(parents):
            integer = str(parents.dtype) in ("torch.int64", "torch.int32", "torch.int16", "torch.int8", "torch.uint8")
            shape = tuple(parents.shape)
        else:
            parents = np.asarray(parents)
            integer, shape = parents.dtype.kind in "iu", parents.shape
        if not integer:
            raise ValueError(f"parents must hold integers (0 = immigrant, else the 1-based index of an earlier event), got {parents.dtype}")
        if shape != (M,):
            raise ValueError(f"parents must hold one entry per event: expected length {M}, got shape {shape}")
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    N = process.ndims()
    if isinstance(parents, str):
        if parents == "map":
            parents = map_parents(process, ds, device=device, ctx=ctx)[0]
        else:
            parents = resample_parents(process, ds, seed=seed, ctx=ctx)[0]
    if _on_device(parents):
        import torch
        if parents.device.index != ctx.device:
            raise ValueError(f"parents is on {parents.device}, the context on cuda:{ctx.device}")
        par = parents.to(torch.int64).contiguous()
        torch.cuda.current_stream(par.device).synchronize()   # the producer's work is done before the library reads
        par_ptr, par_dev = par.data_ptr(), 1
    else:
        par = np.ascontiguousarray(parents.cpu().numpy() if _is_tensor(parents) else parents, dtype=np.int64)
        par_ptr, par_dev = par.ctypes.data, 0
    ncasc, rounds = C.c_int64(), C.c_int32()
    lens = (M, M, M, M, M, M, M, N, N, N * N)
    if device:
        import torch
        dev = torch.device("cuda", ctx.device)
        out = [torch.empty(n, dtype=torch.float64 if k == 6 else torch.int64, device=dev) for k, n in enumerate(lens)]
        torch.cuda.current_stream(dev).synchronize()          # earlier users of the buffers' memory are done before the library writes
        ptrs = [o.data_ptr() for o in out]
        if not _on_device(par):
            par = torch.from_numpy(par).to(dev)
    else:
        out = [np.empty(n, dtype=np.float64 if k == 6 else np.int64) for k, n in enumerate(lens)]
        ptrs = [o.ctypes.data for o in out]
        if _is_tensor(par):
            par = par.cpu().numpy()
    _lib.check(_lib.lib().nhp_cont_cascades(ctx.h, ds.h, par_ptr, par_dev, 1 if device else 0, *ptrs[:7], C.byref(ncasc),
                                            *ptrs[7:], C.byref(rounds)), ctx.h)
    k = ncasc.value
    root, gen, desc, croot, csize, cdepth, cend, imm, off, reach = out
    reach = reach.reshape(N, N).T if device else reach.reshape((N, N), order="F")
    return Cascades(rounds=rounds.value, parents=par, root=root, generation=gen, descendants=desc, cascade_root=croot[:k],
                    cascade_size=csize[:k], cascade_depth=cdepth[:k], cascade_end=cend[:k], immigrants=imm, offspring=off,
                    reach=reach)


def uniform_stream(seed, step, n):
    """The Philox4x32-10 stream the kernel draws from, evaluated on the host."""
    u = np.empty(n)
    _lib.lib().nhp_uniform_stream(seed, step, n, _lib.dptr(u))
    return u


def node_counts(nodes, nnodes):
    """src/parents.jl:61-68"""
    return np.bincount(np.asarray(nodes, dtype=np.int64) - 1, minlength=nnodes).astype(np.float64)


def parent_counts(nodes, parentnodes, nnodes):
    """src/parents.jl:70-79"""
    nodes, parentnodes = np.asarray(nodes, dtype=np.int64), np.asarray(parentnodes, dtype=np.int64)
    cnts = np.zeros((nnodes, nnodes))
    m = parentnodes > 0
    np.add.at(cnts, (parentnodes[m] - 1, nodes[m] - 1), 1.0)
    return cnts
