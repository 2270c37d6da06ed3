"""The layout rule of a continuous dataset restated in numpy (csrc/cont_data.hip: the windows of
nhp_cont_dataset_create_columns, nhp_cont_partition, the child slices and nhp_cont_slices_keep), so that a test can say on the
CPU whether its input keeps its child slices, and where every child sits in them.

    layout(times, nodes, N, dt_max, chunk=None, columns=None) -> Layout

Windows are strict: event j < i is a parent of i when t_j > t_i - dt_max (an earlier event at the same time is one).  The
children of a node, in time order, are cut into items of at most `chunk` children (every node gets at least one item); inside
an item they are sorted, stably, by window length, longest first; every 64 children of an item are one slice whose rows are
its longest window.  The slices are kept when rows < 2^25, rows·64 <= 2·pairs + 4096 and the plan slices at all (0 < pairs <=
160·M, a finite positive dt_max, N <= 65534).

Inputs that would be laid out in XCD time parts (a mean window of 192 pairs, or of 24 on a dataset that is not sliced, with
N >= 8 and M >= 16·N) are refused: no test here uses them."""
from dataclasses import dataclass

import numpy as np

SLICES_MAXK = 160


@dataclass
class Layout:
    M: int
    N: int
    pairs: int
    max_window: int
    chunk: int
    n_items: int
    max_item: int
    kept: bool
    sl_rows: int                 # 0 when the slices are not kept, like the dataset's scalars
    n_slices: int
    sl_max_rows: int
    sl_nb: int
    rows_built: int              # rows, slices and longest slice before the keep rule
    slices_built: int
    max_rows_built: int
    items: np.ndarray            # [n_items, 3]: node (0-based), kbeg, kend
    sl_row: np.ndarray           # [slices_built + 1] first row of every slice, then the total
    sl_item0: np.ndarray         # [n_items + 1] first slice of every item
    window: np.ndarray           # per event: parents in its window
    item: np.ndarray             # per event: its item, -1 on a node outside `columns`
    slice: np.ndarray            # per event: its slice (index into sl_row), -1 likewise
    lane: np.ndarray             # per event: its lane in the slice, -1 likewise
    slice_rows: np.ndarray       # [slices_built] rows of every slice
    slice_lanes: np.ndarray      # [slices_built] children in every slice
    item_slices: np.ndarray      # [n_items] slices of every item

    def scalars(self):
        """The fields of DeviceDataset.scalars() this restatement covers."""
        return {"pairs": self.pairs, "n_items": self.n_items, "max_item": self.max_item, "max_window": self.max_window,
                "sl_rows": self.sl_rows, "n_slices": self.n_slices, "sl_max_rows": self.sl_max_rows}


def windows(times, dt_max):
    """first[i]: the first event of i's window; i - first[i] parents."""
    t = np.asarray(times, dtype=np.float64)
    M = len(t)
    thr = t - dt_max
    first = np.minimum(np.searchsorted(t, thr, side="right"), np.arange(M))       # first f with t_f > t_i - dt_max, at most i
    return first.astype(np.int64)


def item_size(M, N, chunk=None):
    c = int(1.3 * float(M) / float(N)) + 1 if N >= 1024 else (M + 1023) // 1024
    c = max(32, min(4096, c))
    if chunk is not None and int(chunk) > 0:                     # NHP_CHUNK
        c = min(int(chunk), 4096)
    return c


def layout(times, nodes, N, dt_max, chunk=None, columns=None):
    t = np.asarray(times, dtype=np.float64)
    node = np.asarray(nodes, dtype=np.int64) - 1
    M, N = len(t), int(N)
    assert len(node) == M and (M == 0 or (node.min() >= 0 and node.max() < N)) and np.all(np.diff(t) >= 0.0)
    first = windows(t, dt_max)
    win = np.arange(M, dtype=np.int64) - first
    pairs = int(win.sum())
    max_window = int(win.max()) if M else 0
    csize = item_size(M, N, chunk)
    sliced = 0 < pairs <= SLICES_MAXK * M and np.isfinite(dt_max) and dt_max > 0.0 and N <= 65534
    kbar = pairs / M if M else 0.0
    TP = 4 if kbar >= 192.0 else (2 if kbar >= 24.0 and not sliced else 0)
    if TP and N >= 8 and M >= 16 * N:
        raise ValueError("this input is laid out in XCD time parts: not restated here")
    # the children of every node in time order (a stable counting sort), cut into items
    order = np.argsort(node, kind="stable")
    boff = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=N))]).astype(np.int64)
    c0, c1 = (0, N) if columns is None else (int(columns[0]), int(columns[1]))
    items = []
    for c in range(N):
        b, n = int(boff[c]), int(boff[c + 1] - boff[c])
        parts = max(1, (n + csize - 1) // csize)
        for q in range(parts):
            if c0 <= c < c1:
                items.append((c, b + n * q // parts, b + n * (q + 1) // parts))
    items = np.array(items, dtype=np.int64).reshape(-1, 3)
    n_items = len(items)
    max_item = int((items[:, 2] - items[:, 1]).max()) if n_items else 0
    # inside an item: longest window first, stable; one slice per 64 children, rows = its longest window
    ev_item, ev_slice, ev_lane = (np.full(M, -1, dtype=np.int64) for _ in range(3))
    sl_row, sl_item0, slice_rows, slice_lanes = [], [], [], []
    rows, max_rows = 0, 0
    for q, (c, kb, ke) in enumerate(items):
        sl_item0.append(len(sl_row))
        ev = order[kb:ke]
        ev = ev[np.argsort(-win[ev], kind="stable")]
        ev_item[ev] = q
        for k0 in range(0, len(ev), 64):
            sl = ev[k0:k0 + 64]
            longest = int(win[sl].max())
            ev_slice[sl] = len(sl_row)
            ev_lane[sl] = np.arange(len(sl))
            sl_row.append(rows)
            slice_rows.append(longest)
            slice_lanes.append(len(sl))
            rows += longest
            max_rows = max(max_rows, longest)
    sl_item0.append(len(sl_row))
    n_slices = len(sl_row)
    sl_row.append(rows)
    kept = bool(sliced and rows < (1 << 25) and rows * 64 <= 2 * pairs + 4096)
    sl_item0 = np.array(sl_item0, dtype=np.int64)
    return Layout(M=M, N=N, pairs=pairs, max_window=max_window, chunk=csize, n_items=n_items, max_item=max_item, kept=kept,
                  sl_rows=rows if kept else 0, n_slices=n_slices if kept else 0, sl_max_rows=max_rows if kept else 0,
                  sl_nb=int(N).bit_length(), rows_built=rows, slices_built=n_slices, max_rows_built=max_rows, items=items,
                  sl_row=np.array(sl_row, dtype=np.int64), sl_item0=sl_item0, window=win, item=ev_item, slice=ev_slice,
                  lane=ev_lane, slice_rows=np.array(slice_rows, dtype=np.int64), slice_lanes=np.array(slice_lanes, dtype=np.int64),
                  item_slices=np.diff(sl_item0))
