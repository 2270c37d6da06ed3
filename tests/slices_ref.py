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
N >= 8 and M >= 16·N) are refused by layout(); their item table is restated apart, from the rule, by

    time_parts(times, nodes, N, dt_max, columns=None) -> None | (TP, items [n_items, 4]: node, kbeg, kend, first)

which tests/test_time_parts_host.py holds to the properties of a partition and tests/test_time_parts_gpu.py compares with
what the dataset exports."""
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


def time_part_count(pairs, M, N, dt_max):
    """TP of the default rule: 4 from a mean window of 192 pairs on, 2 from 24 on where the plan does not slice (pairs > 160·M
    or no finite positive Δtmax), and only with N >= 8 and M >= 16·N; otherwise 0."""
    if M == 0 or N < 8 or M < 16 * N:
        return 0
    sliced = 0 < pairs <= SLICES_MAXK * M and np.isfinite(dt_max) and dt_max > 0.0 and N <= 65534
    kbar = pairs / M
    return 4 if kbar >= 192.0 else (2 if kbar >= 24.0 and not sliced else 0)


def time_parts(times, nodes, N, dt_max, columns=None, parts=None):
    """The XCD time-part layout restated from its rule: None where the rule gives TP = 0, otherwise (TP, items) with items an
    [n_items, 4] table of node (0-based), kbeg, kend, first.

    Workgroup b runs on XCD b % 8.  XCD x = s·(8/TP) + g gets time part s -- the events with index in [M·s/TP, M·(s+1)/TP) --
    of the nodes c with c % (8/TP) == g, so the table is one run of 8 items per group of 8/TP consecutive nodes; kbeg and
    kend count positions in the node-sorted child array, where a node's children stand in time order.  Only the s = 0 item of
    a node is `first` (bit 0); bit 1 (the node's only item) is never set, every node having TP >= 2 items.  Where N is no
    multiple of 8/TP the last run is filled with empty items that name node N - 1 and are not first.  A column shard keeps
    the items whose node it owns (the padding with node N - 1).  parts: NHP_XCD's value instead of the rule's (2, 4 or 8)."""
    t = np.asarray(times, dtype=np.float64)
    node = np.asarray(nodes, dtype=np.int64) - 1
    M, N = len(t), int(N)
    assert len(node) == M and (M == 0 or (node.min() >= 0 and node.max() < N)) and np.all(np.diff(t) >= 0.0)
    pairs = int((np.arange(M, dtype=np.int64) - windows(t, dt_max)).sum())
    TP = time_part_count(pairs, M, N, dt_max) if parts is None else (int(parts) if N >= 8 and M >= 16 * N else 0)
    if TP == 0:
        return None
    assert TP in (2, 4, 8)
    per_run = 8 // TP                                                     # nodes per run of 8 items
    runs = -(-N // per_run)
    boff = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=N))]).astype(np.int64)
    cuts = [M * s // TP for s in range(TP + 1)]
    # children of node c with an event index below each cut: c's events are the sorted indices where node == c
    below = np.stack([np.bincount(node[:cut], minlength=N) for cut in cuts], axis=1)
    c0, c1 = (0, N) if columns is None else (int(columns[0]), int(columns[1]))
    items = []
    for b in range(runs * 8):
        x = b % 8
        s, g = x // per_run, x % per_run
        c = (b // 8) * per_run + g
        if c < N:
            row = (c, boff[c] + below[c, s], boff[c] + below[c, s + 1], 1 if s == 0 else 0)
        else:
            row = (N - 1, boff[N - 1], boff[N - 1], 0)
        if c0 <= row[0] < c1:
            items.append(row)
    return TP, np.array(items, dtype=np.int64).reshape(-1, 4)


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
