"""Array-level host API over the C ABI: a chromosome resident in HBM and clustering runs on it.

This is what the reference-shaped wrappers (cDBSCAN.py, cDBSCAN2.py, blockDBSCAN.py,
pipe.py) and bench.py are built on.
"""
import ctypes
import math
import os

import numpy as np

from . import _lib

VARIANTS = {"v1": _lib.VARIANT_CDBSCAN1, "cDBSCAN": _lib.VARIANT_CDBSCAN1, 1: 1,
            "v2": _lib.VARIANT_CDBSCAN2, "cDBSCAN2": _lib.VARIANT_CDBSCAN2, 2: 2,
            "block": _lib.VARIANT_BLOCK, "blockDBSCAN": _lib.VARIANT_BLOCK, 3: 3}

BOX_DTYPE = np.dtype([("min_x", "<i4"), ("max_x", "<i4"), ("min_y", "<i4"), ("max_y", "<i4"), ("count", "<i4")])


# developer / test knob: every new handle is switched to this traversal level (cl_set_traversal; None = the library's default).
# The library itself reads no environment variable.
TRAVERSAL_OVERRIDE = int(os.environ["CLOOPS_TRAVERSAL"]) if os.environ.get("CLOOPS_TRAVERSAL", "") != "" else None


def device_count():
    return _lib.load().cl_device_count()


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _as_i32(a, name):
    a = np.asarray(a)
    if a.ndim != 1:
        raise ValueError("%s must be one-dimensional" % name)
    if a.dtype.kind == "f":
        if a.size and not np.all(a == np.floor(a)):
            raise TypeError("%s: integer coordinates required (the reference's PET mid-points are ints)" % name)
    elif a.dtype.kind not in "iu":
        raise TypeError("%s: integer coordinates required" % name)
    if a.size and (a.min() <= -(1 << 29) or a.max() >= (1 << 29)):
        raise _lib.CloopsHipError(_lib.CL_ERR_DOMAIN, "coordinates must satisfy |X|,|Y| < 2^29")
    return np.ascontiguousarray(a, dtype=np.int32)


class ClusterResult(object):
    """labels: int32[n] aligned to the input rows (-1 = not in the reference's `.labels`);
    boxes: structured array indexed by cluster id (count == 0 marks an id gap of variant 1)."""
    __slots__ = ("labels", "n_clusters", "max_label", "boxes", "timing")

    def __init__(self, labels, n_clusters, max_label, boxes, timing):
        self.labels = labels
        self.n_clusters = n_clusters
        self.max_label = max_label
        self.boxes = boxes
        self.timing = timing


class _Handle(object):
    """the lifetime of one library handle: _open() makes it, close() destroys it once (also when the object is collected)"""
    _DESTROY = None                                # the entry that destroys the handle

    def _open(self, create, *args):
        """`create(*args, &handle)`: every cl_*_create entry takes its out-pointer last"""
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        _lib.check(getattr(self._lib, create)(*args, ctypes.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self._lib, self._DESTROY)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:                                               # noqa: BLE001
            pass


class Chromosome(_Handle):
    """One chromosome's PET coordinates resident in HBM (cl_chrom of include/cloops_hip.h)."""
    _DESTROY = "cl_chrom_destroy"

    def __init__(self, X, Y, device=0, stream=None):
        X = _as_i32(X, "X")
        Y = _as_i32(Y, "Y")
        if X.shape != Y.shape:
            raise ValueError("X and Y differ in length")
        self._create(X.shape[0], device, "cl_chrom_create", int(device), ctypes.c_void_p(stream), X.ctypes.data_as(ctypes.c_void_p),
                     Y.ctypes.data_as(ctypes.c_void_p), int(X.shape[0]), 0)

    def _create(self, n, device, create, *args):
        """the one constructor step of all three ways to make a chromosome: the fields, the handle, the traversal override"""
        self.n = int(n)
        self.device = device
        self._profiling = False
        self._pins = {}                            # (kind, slot) -> (address, int32 view or None): every page-locked block this object owns
        self._inflight = []
        self._enq = 0
        self._open(create, *args)
        if TRAVERSAL_OVERRIDE is not None:
            self._lib.cl_set_traversal(self._h, int(TRAVERSAL_OVERRIDE))

    @classmethod
    def from_device_pointers(cls, x_ptr, y_ptr, n, device=0, stream=None, keepalive=None):
        """Wrap int32 device arrays (e.g. torch tensors' data_ptr()) without copying."""
        self = cls.__new__(cls)
        self._keepalive = keepalive
        self._create(n, device, "cl_chrom_create", int(device), ctypes.c_void_p(stream), ctypes.c_void_p(x_ptr), ctypes.c_void_p(y_ptr),
                     int(n), 1)
        return self

    def subsample(self, rows):
        """a new resident chromosome made of `rows` of this one, in the order given (`mat[rows, :]` of
        scripts/jd2saturation:46-47), gathered on the device (cl_chrom_subsample)"""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        new = Chromosome.__new__(Chromosome)
        new._create(rows.shape[0], self.device, "cl_chrom_subsample", self._h, rows.ctypes.data_as(ctypes.c_void_p), int(rows.shape[0]))
        return new

    def close(self):
        _Handle.close(self)
        pins, self._pins = getattr(self, "_pins", {}), {}
        for p, _ in pins.values():
            self._lib.cl_host_free(ctypes.c_void_p(p))

    def _pin(self, kind, slot, nbytes, shape=None):
        """the page-locked block `kind` of result slot `slot` (two per kind: a run takes slot `enq & 1`), made on first use
        -> (address, int32 view of `shape` or None)"""
        e = self._pins.get((kind, slot))
        if e is None:
            p = _lib.host_alloc(nbytes)
            view = None if shape is None else np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_int32)), shape=shape)
            e = self._pins[kind, slot] = (p, view)
        return e

    def _pinned_labels(self, which=0):
        """Page-locked int32[n] result buffers owned by this object (two: one per result slot)."""
        return self._pin("labels", which, max(4, self.n * 4), (self.n,))[1]

    def set_profiling(self, on=True):
        self._profiling = bool(on)
        self._lib.cl_set_profiling(self._h, 1 if on else 0)

    def set_device_labels(self, on=True):
        """row-aligned device labels for runs without a host destination (default on); the sweep driver switches
        them off: it only needs tables and distance statistics (cl_set_device_labels)"""
        self._lib.cl_set_device_labels(self._h, 1 if on else 0)

    def set_table_export(self, on=True):
        """copy of the cluster table to pinned host memory at the end of a run (default on; cl_set_table_export)"""
        if getattr(self, "_export", True) != bool(on):
            self._lib.cl_set_table_export(self._h, 1 if on else 0)
            self._export = bool(on)

    # ---- candidate loops of a sweep, kept on the device (K10) ----
    def cand_reset(self):
        _lib.check(self._lib.cl_cand_reset(self._h))

    def cand_append(self, step):
        """classify the last run's cluster table (pipe.py:83-97) and append its inter-ligation boxes under `step`
        -> (n_inter, n_self)"""
        ni, ns = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self._lib.cl_cand_append(self._h, int(step), ctypes.byref(ni), ctypes.byref(ns)))
        return int(ni.value), int(ns.value)

    def step_async(self, variant, eps, minPts, cut, step, fine_lo=-1):
        """one sweep step in one asynchronous call (cl_cluster_step_async): the run, then -- in its own stream -- the
        classification of its table, the append of its inter-ligation boxes under `step` and the distance summary;
        pair with wait(), then read step_result()"""
        _lib.check(self._lib.cl_cluster_step_async(self._h, VARIANTS[variant], int(eps), int(minPts), int(cut), int(step), int(fine_lo)))
        self._export = False
        self._inflight.append((None, False))
        self._enq += 1

    def step_result(self):
        """-> (n_inter, n_self, summary dict as dist_summary) of the last completed sweep step (no GPU work)"""
        ni, ns = ctypes.c_int64(0), ctypes.c_int64(0)
        st = _lib.ClDsummary()
        _lib.check(self._lib.cl_step_result(self._h, ctypes.byref(ni), ctypes.byref(ns), ctypes.byref(st)))
        return int(ni.value), int(ns.value), self._summary_dict(st)

    def cand_finish(self, final_cut, capacity):
        """combineTwice + filterClusterByDis over everything appended since cand_reset -> int32 [k, 4] boxes
        (minX, maxX, minY, maxY) in append order"""
        # the rows land in a host buffer the handle keeps (grown on demand) and the kept ones are copied out: a fresh
        # capacity-sized array per call (tens of MB of untouched pages under a pageable device-to-host copy, 23 at once) made
        # one sweep in five 20-30 ms slower (200 M genome: 0.165-0.184 s outliers among 0.155 s sweeps)
        buf = getattr(self, "_cand_buf", None)
        if buf is None or len(buf) < capacity:
            buf = self._cand_buf = np.zeros((max(int(capacity) + int(capacity) // 4, 1), 4), dtype=np.int32)
        k = ctypes.c_int64(0)
        _lib.check(self._lib.cl_cand_finish(self._h, int(final_cut), buf.ctypes.data_as(ctypes.c_void_p), int(capacity), ctypes.byref(k)))
        return buf[: int(k.value)].copy()

    def cand_finish_device(self, final_cut):
        """the same, leaving the boxes on the device -> (device pointer, rows); valid until the handle's next sweep finishes
        (cl_cand_finish_device: what comm.Comm.gather_device sends to the merging rank)"""
        ptr, k = ctypes.c_void_p(), ctypes.c_int64(0)
        _lib.check(self._lib.cl_cand_finish_device(self._h, int(final_cut), ctypes.byref(ptr), ctypes.byref(k)))
        return (ptr.value or 0), int(k.value)

    def set_sort_index(self, mode=1):
        """rows kept sorted by the in-strip coordinate, every eps' layout from a 2-pass strip sort of that order:
        0 = built at the handle's second sort (default), 1 = at the first, -1 = never (cl_set_sort_index)"""
        self._lib.cl_set_sort_index(self._h, int(mode))

    def set_count_reuse(self, on=True):
        """region-query words of the first run at an eps re-used by the later runs at that eps (default on; results
        identical either way -- cl_set_count_reuse of include/cloops_hip.h)"""
        self._lib.cl_set_count_reuse(self._h, 1 if on else 0)

    def sweep_plan(self, eps_list, min_pts_list):
        """announce a sweep `for ep in eps: for m in minPts:` (cLoops/pipe.py:241-281) in one call (cl_sweep_plan): one sort for all
        layouts, one region query per eps, the cut band only for the later runs.  Two empty lists end the plan."""
        ev = sorted(set(int(e) for e in eps_list))
        mv = sorted(set(int(m) for m in min_pts_list))
        ea = (ctypes.c_int32 * max(len(ev), 1))(*ev)
        ma = (ctypes.c_int32 * max(len(mv), 1))(*mv)
        _lib.check(self._lib.cl_sweep_plan(self._h, ea, len(ev), ma, len(mv)))

    def drop_indexes(self):
        """forget the q index, the fine layout, the last eps' layout and the cached counts (cl_chrom_drop_indexes): the next run
        sorts like the first run on a fresh dataset, allocations stay"""
        _lib.check(self._lib.cl_chrom_drop_indexes(self._h))

    def set_traversal(self, level=4):
        """how far a run works on its core / walker lists instead of LDS tiles over every PET: 0 .. 4 (default 4; results
        identical at every level -- cl_set_traversal of include/cloops_hip.h)"""
        self._lib.cl_set_traversal(self._h, int(level))

    def set_count_floor(self, min_pts):
        """the smallest minPts that will follow at the current eps (cl_set_count_floor); 0 = unknown"""
        self._lib.cl_set_count_floor(self._h, int(min_pts))

    def set_count_thresholds(self, min_pts_list):
        """the minPts values that will be asked for at the current eps (cl_set_count_thresholds); empty = unknown"""
        vals = [int(m) for m in min_pts_list]
        arr = (ctypes.c_int32 * max(1, len(vals)))(*vals)
        self._lib.cl_set_count_thresholds(self._h, arr, len(vals))

    def set_stream(self, stream):
        """move the idle handle to another caller-made / library-made stream of its device (cl_chrom_set_stream)"""
        _lib.check(self._lib.cl_chrom_set_stream(self._h, ctypes.c_void_p(stream)))

    def set_eps_list(self, eps_list):
        """the eps values that will be asked for (cl_set_eps_list): with a common divisor the layouts come from one fine sort; empty = unknown"""
        vals = [int(e) for e in eps_list]
        arr = (ctypes.c_int32 * max(1, len(vals)))(*vals)
        self._lib.cl_set_eps_list(self._h, arr, len(vals))

    def last_region_mode(self):
        """0 = the last enqueued run did a full region query, 1 = re-used the kept words, 2 = re-used them outside the cut band"""
        return int(self._lib.cl_last_region_mode(self._h))

    def base_rows(self):
        """rows of the handle's current base layout (cl_base_rows): fewer than len(self) while a sweep's layout leaves out the rows far
        below the chain's cut, len(self) otherwise"""
        return int(self._lib.cl_base_rows(self._h))

    def set_layout_reuse(self, on=True):
        """keep the sorted arrays of the last eps and start further runs at that eps from a compaction by the cut
        (default on; results identical either way -- cl_set_layout_reuse of include/cloops_hip.h)"""
        self._lib.cl_set_layout_reuse(self._h, 1 if on else 0)

    def timing(self):
        t = _lib.ClTiming()
        _lib.check(self._lib.cl_get_timing(self._h, ctypes.byref(t)))
        return {k: getattr(t, k) for k, _ in _lib.ClTiming._fields_}

    def _boxes(self, max_label, copy):
        k = max_label + 1
        if k <= 0:
            return np.zeros(0, dtype=BOX_DTYPE)
        ptr = self._lib.cl_boxes_host(self._h)
        if not ptr:                                # (no result, or a run made with the export off: nothing to view)
            raise _lib.CloopsHipError(_lib.CL_ERR_ARG, "the last run has no exported cluster table")
        view = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_int32)), shape=(k * 5,)).view(BOX_DTYPE)
        return view.copy() if copy else view

    def cluster_async(self, variant, eps, minPts, cut=0, want_labels=True, want_boxes=True):
        """Enqueue one run without blocking (at most two in flight); pair with wait().
        Labels land in one of two reusable pinned buffers (or stay on the device); `want_boxes=False`
        leaves the cluster table on the device too (cand_append / the distance statistics read it there)."""
        v = VARIANTS[variant]
        self.set_table_export(want_boxes)
        labels = self._pinned_labels(self._enq & 1) if want_labels else None
        _lib.check(self._lib.cl_cluster_async(self._h, v, int(eps), int(minPts), int(cut),
                                              labels.ctypes.data_as(ctypes.c_void_p) if want_labels else None))
        self._inflight.append((labels, bool(want_boxes)))
        self._enq += 1

    def cluster_pairs_async(self, variant, eps, minPts, cut=0, want_boxes=True):
        """Enqueue a run whose labels come back the way the reference holds them -- clustered PETs only (cDBSCAN2.py:186-191): one
        (row, label) pair per labelled PET in a page-locked buffer (cl_cluster_pairs_async); pair with wait_pairs()."""
        v = VARIANTS[variant]
        self.set_table_export(want_boxes)
        buf = self._pin("pairs", self._enq & 1, max(8, self.n * 8), (self.n, 2))[1]
        _lib.check(self._lib.cl_cluster_pairs_async(self._h, v, int(eps), int(minPts), int(cut), buf.ctypes.data_as(ctypes.c_void_p), self.n))
        self._inflight.append((buf, bool(want_boxes)))
        self._enq += 1

    def wait_pairs(self, copy=False, defer=False):
        """completes the oldest run enqueued by cluster_pairs_async -> (ClusterResult with labels None, pairs int32 [K, 2]: row, label).
        defer=True: the pairs are still crossing PCIe when this returns -- call pairs_sync() before reading them (a loop over many
        chromosomes waits for all of them first: their copies then run side by side)"""
        buf, exported = self._inflight.pop(0)
        nc, ml = ctypes.c_int32(0), ctypes.c_int32(-1)
        self._lib.cl_set_pairs_defer(self._h, 1 if defer else 0)
        _lib.check(self._lib.cl_wait(self._h, ctypes.byref(nc), ctypes.byref(ml)))
        k = int(self._lib.cl_last_n_labelled(self._h))
        pairs = buf[:k].copy() if copy else buf[:k]
        boxes = self._boxes(ml.value, copy) if exported else None
        return ClusterResult(None, nc.value, ml.value, boxes, self.timing() if self._profiling else None), pairs

    def pairs_sync(self):
        _lib.check(self._lib.cl_pairs_sync(self._h))

    def cluster_rowmask_async(self, variant, eps, minPts, cut=0, want_boxes=True):
        """Enqueue a run whose labels come back in their smallest form: one bit per input row (set = clustered) and the labels of the
        set rows in ascending row order (cl_cluster_rowmask_async) -- 4 bytes per clustered PET + n / 8 bytes over PCIe instead of
        the 8 bytes per clustered PET of cluster_pairs_async; pair with wait_rowmask()."""
        v = VARIANTS[variant]
        self.set_table_export(want_boxes)
        p = self._pin("rowmask", self._enq & 1, 8 * ((self.n + 63) // 64) + 4 * max(self.n, 1))[0]
        _lib.check(self._lib.cl_cluster_rowmask_async(self._h, v, int(eps), int(minPts), int(cut), ctypes.c_void_p(p), max(self.n, 1)))
        self._inflight.append((p, bool(want_boxes)))
        self._enq += 1

    def wait_rowmask(self, copy=False, defer=False):
        """completes the oldest run enqueued by cluster_rowmask_async -> (ClusterResult with labels None, mask uint64 [ceil(n / 64)],
        labels int32 [K] of the set rows in ascending row order); rows_of_mask(mask) gives the rows.  defer as in wait_pairs()."""
        p, exported = self._inflight.pop(0)
        nc, ml = ctypes.c_int32(0), ctypes.c_int32(-1)
        self._lib.cl_set_pairs_defer(self._h, 1 if defer else 0)
        _lib.check(self._lib.cl_wait(self._h, ctypes.byref(nc), ctypes.byref(ml)))
        k = int(self._lib.cl_last_n_labelled(self._h))
        nw = (self.n + 63) // 64
        mask = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64)), shape=(nw,))
        labels = np.ctypeslib.as_array(ctypes.cast(p + 8 * nw, ctypes.POINTER(ctypes.c_int32)), shape=(max(k, 1),))[:k]
        if copy:
            mask, labels = mask.copy(), labels.copy()
        boxes = self._boxes(ml.value, copy) if exported else None
        return ClusterResult(None, nc.value, ml.value, boxes, self.timing() if self._profiling else None), mask, labels

    def rows_of_mask(self, mask):
        """the set rows of a wait_rowmask() mask, ascending (int64)"""
        bits = np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), bitorder="little")[: self.n]
        return np.flatnonzero(bits)

    def wait(self, copy=False):
        """Complete the oldest in-flight run -> ClusterResult (labels / boxes are VIEWS of pinned
        buffers that stay valid until two more runs have been enqueued, unless copy=True)."""
        labels, exported = self._inflight.pop(0)
        nc = ctypes.c_int32(0)
        ml = ctypes.c_int32(-1)
        _lib.check(self._lib.cl_wait(self._h, ctypes.byref(nc), ctypes.byref(ml)))
        boxes = self._boxes(ml.value, copy) if exported else None
        if labels is not None and copy:
            labels = labels.copy()
        return ClusterResult(labels, nc.value, ml.value, boxes, self.timing() if self._profiling else None)

    def cluster(self, variant, eps, minPts, cut=0, want_labels=True, want_boxes=True, pinned=False):
        """One synchronous run.  `pinned=True` returns labels and boxes as VIEWS of reusable
        page-locked buffers (valid until the next run on this chromosome) -- the fast path used
        by the sweep driver and bench."""
        v = VARIANTS[variant]
        if self._inflight:
            raise RuntimeError("asynchronous runs in flight: call wait() first")
        self.set_table_export(True)
        if want_labels:
            labels = self._pinned_labels(0) if pinned else np.empty(self.n, dtype=np.int32)
        else:
            labels = None
        nc = ctypes.c_int32(0)
        ml = ctypes.c_int32(-1)
        lp = labels.ctypes.data_as(ctypes.c_void_p) if want_labels else None
        _lib.check(self._lib.cl_cluster(self._h, v, int(eps), int(minPts), int(cut), lp,
                                        ctypes.byref(nc), ctypes.byref(ml)))
        boxes = self._boxes(ml.value, copy=not pinned) if want_boxes else None
        return ClusterResult(labels, nc.value, ml.value, boxes, self.timing() if self._profiling else None)

    def cluster_weighted(self, eps, minPts, wx=1, wy=1):
        """Variant 1 under the metric wx*|dX| + wy*|dY| <= eps: the labels of
        `cDBSCAN(mat * [1, wx, wy], eps, minPts)` (scripts/callStripes:37-52); boxes in unscaled
        coordinates (cl_cluster_weighted of include/cloops_hip.h)."""
        if self._inflight:
            raise RuntimeError("asynchronous runs in flight: call wait() first")
        self.set_table_export(True)                 # (a run with want_boxes=False may have switched it off: the boxes below are read)
        labels = np.empty(self.n, dtype=np.int32)
        nc = ctypes.c_int32(0)
        ml = ctypes.c_int32(-1)
        _lib.check(self._lib.cl_cluster_weighted(self._h, int(eps), int(minPts), int(wx), int(wy),
                                                 labels.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nc), ctypes.byref(ml)))
        return ClusterResult(labels, nc.value, ml.value, self._boxes(ml.value, copy=True), self.timing() if self._profiling else None)

    def last_n_in(self):
        """PETs of the last completed run that entered DBSCAN (after the cut filter)."""
        return int(self._lib.cl_last_n_in(self._h))

    # ---- distance statistics of the last completed run (K7; inputs of ests.estIntSelCutFrag) ----
    def dist_summary(self, cut=0):
        """-> dict(n_all=[inter, self], n_pos=[...], sumx=[...], sumxx=[...], xshift, loghist=uint64[3840])
        (cl_dist_summary: one pass; x = log2|d| - xshift)."""
        st = _lib.ClDsummary()
        _lib.check(self._lib.cl_dist_summary(self._h, int(cut), ctypes.byref(st)))
        return self._summary_dict(st)

    @staticmethod
    def _summary_dict(st):
        return {"n_all": [int(st.n_all[0]), int(st.n_all[1])], "n_pos": [int(st.n_pos[0]), int(st.n_pos[1])],
                "sumx": [float(st.sumx[0]), float(st.sumx[1])], "sumxx": [float(st.sumxx[0]), float(st.sumxx[1])],
                "xshift": float(st.xshift), "loghist": np.ctypeslib.as_array(st.loghist).astype(np.int64),
                "fine_lo": int(st.fine_lo), "fine": np.ctypeslib.as_array(st.fine).astype(np.int64) if st.fine_lo >= 0 else None}

    def dist_bin_hist(self, cut, lo, hi, shift):
        """histogram (int64[2048]) of (|d| - lo) >> shift over the self group's lo <= |d| < hi (cl_dist_bin_hist)"""
        out = np.zeros(2048, dtype=np.uint64)
        _lib.check(self._lib.cl_dist_bin_hist(self._h, int(cut), int(lo), int(hi), int(shift),
                                              out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out.astype(np.int64)

    # ---- kernel density sums of log2|d| of the last completed run (K17; the curves of cPlots.plotIntSelCutFrag) ----
    def dist_collect(self, cut=0):
        """pack and sort the (|d|, weight) entries with |d| > 0 of both groups on the device (cl_dist_collect; same `cut` as
        the run) -> dict(n_pos=[inter, self], dmin=[...], dmax=[...]); an empty group has n_pos 0 and dmin = dmax = 0"""
        out = [(ctypes.c_int64 * 2)() for _ in range(3)]
        _lib.check(self._lib.cl_dist_collect(self._h, int(cut), *out))
        return {k: [int(a[0]), int(a[1])] for k, a in zip(("n_pos", "dmin", "dmax"), out)}

    def dist_kde(self, group, lo, step, inv_h, gridsize):
        """-> float64[gridsize]: S[j] = sum over the collected entries of `group` (0 = inter, 1 = self) of
        weight * exp(-((log2|d| - (lo + j step)) inv_h)^2 / 2), unnormalised (cl_dist_kde); needs dist_collect() after the run"""
        out = np.zeros(max(int(gridsize), 1), dtype=np.float64)
        _lib.check(self._lib.cl_dist_kde(self._h, int(group), float(lo), float(step), float(inv_h), int(gridsize),
                                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return out

    def sig_counts(self, windows, cut=0):
        """K8: interval counts for the significance test.  windows: int32 [R, 44] (lo[22], hi[22];
        A0..A10 then B0..B10) -> (int32 [R, 144] counts, N)  (cl_sig_counts of include/cloops_hip.h)."""
        w = np.ascontiguousarray(windows, dtype=np.int32).reshape(-1, 44)
        out = np.zeros((len(w), 144), dtype=np.int32)
        npets = ctypes.c_int64(0)
        _lib.check(self._lib.cl_sig_counts(self._h, int(cut), len(w), w.ctypes.data_as(ctypes.c_void_p),
                                           out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(npets)))
        return out, int(npets.value)

    def quant_counts(self, windows, cut=0):
        """K11: directed interval counts for quantifyLoops / deLoops.  windows: int32 [R, 44] as for sig_counts ->
        (int32 [R, 123] counts: ra, rb, then |{X in A_k} & {Y in B_l}| at 2 + 11 k + l; N)  (cl_quant_counts)."""
        w = np.ascontiguousarray(windows, dtype=np.int32).reshape(-1, 44)
        out = np.zeros((len(w), 123), dtype=np.int32)
        npets = ctypes.c_int64(0)
        _lib.check(self._lib.cl_quant_counts(self._h, int(cut), len(w), w.ctypes.data_as(ctypes.c_void_p),
                                             out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(npets)))
        return out, int(npets.value)

    def contact_hist(self, bin_size, cut=0):
        """K12: histogram of the cell counts of the upper contact matrix (scripts/jd2fingerprint:32-50) of the PETs with
        Y - X >= cut (cut > 0) at `bin_size` -> (values int64 ascending, mult int64, n_kept, min_c): mult[k] cells hold values[k]
        PETs each; min_c is None when no PET passes the cut  (cl_contact_hist)."""
        if int(bin_size) < 1:
            raise ValueError("bin_size must be >= 1, got %s" % bin_size)
        cap = math.isqrt(2 * self.n) + 2                               # D (D + 1) / 2 <= kept PETs <= n
        values = np.zeros(cap, dtype=np.int64)
        mult = np.zeros(cap, dtype=np.int64)
        nd, ncells, nkept, minc = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0)
        _lib.check(self._lib.cl_contact_hist(self._h, int(cut), int(bin_size), cap, values.ctypes.data_as(ctypes.c_void_p),
                                             mult.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nd), ctypes.byref(ncells),
                                             ctypes.byref(nkept), ctypes.byref(minc)))
        d = int(nd.value)
        return values[:d].copy(), mult[:d].copy(), int(nkept.value), (int(minc.value) if nkept.value else None)

    def anchor_mask(self, starts, ends):
        """K13: the rows with X or Y inside one of the closed intervals [starts[k], ends[k]] (scripts/jd2cleanWashuPETs.py:200-227;
        any order, overlaps allowed) -> (mask uint64 [ceil(n / 64)], n_merged, n_kept): n_merged = intervals after merging the
        overlapping or touching ones, n_kept = set rows; rows_of_mask(mask) gives the rows  (cl_anchor_mask)."""
        s = np.ascontiguousarray(starts, dtype=np.int64).ravel()
        e = np.ascontiguousarray(ends, dtype=np.int64).ravel()
        if len(s) != len(e):
            raise ValueError("starts and ends differ in length (%d, %d)" % (len(s), len(e)))
        nw = (self.n + 63) // 64
        mask = np.zeros(max(nw, 1), dtype=np.uint64)
        nm, nk = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self._lib.cl_anchor_mask(self._h, len(s), s.ctypes.data_as(ctypes.c_void_p), e.ctypes.data_as(ctypes.c_void_p),
                                            mask.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nm), ctypes.byref(nk)))
        return mask[:nw], int(nm.value), int(nk.value)

    def agg_loops(self, cx, cy, res, w=10, corner=3, cut=0, want_stats=True, want_mats=False):
        """K19: the PETs with Y - X >= cut (cut > 0) piled up around the loop centres (cx[k], cy[k]) in W x W bins of `res` bp,
        W = 2 w + 1: a row falls into cell ((X - ox) // res, (Y - oy) // res) of loop k when both differences lie in [0, W res),
        ox = cx - w res - res // 2, oy likewise -> (S int64 [W, W] = the sum of the loops' matrices, stats int32 [n, 6] (total,
        centre, ll, ul, ur, lr: corner x corner sums) or None, mats int32 [n, W, W] or None, n_kept = rows passing the cut)
        (cl_agg_loops of include/cloops_hip.h)."""
        res, w, corner = int(res), int(w), int(corner)
        if res < 1 or not 1 <= w <= 20 or not 1 <= corner <= w or (2 * w + 1) * res >= 1 << 29:
            raise ValueError("agg_loops needs res >= 1, 1 <= w <= 20, 1 <= corner <= w and (2 w + 1) res < 2^29, got res=%s w=%s corner=%s"
                             % (res, w, corner))
        cx = np.ascontiguousarray(cx, dtype=np.int64).ravel()
        cy = np.ascontiguousarray(cy, dtype=np.int64).ravel()
        if len(cx) != len(cy):
            raise ValueError("cx and cy differ in length (%d, %d)" % (len(cx), len(cy)))
        lim = np.iinfo(np.int32)
        if len(cx) and (min(cx.min(), cy.min()) < lim.min or max(cx.max(), cy.max()) > lim.max):
            raise ValueError("loop centres must fit int32")
        cx, cy = cx.astype(np.int32), cy.astype(np.int32)
        n, W = len(cx), 2 * w + 1
        S = np.zeros((W, W), dtype=np.int64)
        stats = np.zeros((n, 6), dtype=np.int32) if want_stats else None
        mats = np.zeros((n, W, W), dtype=np.int32) if want_mats else None
        ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        nkept = ctypes.c_int64(0)
        _lib.check(self._lib.cl_agg_loops(self._h, int(cut), res, w, corner, n, ptr(cx), ptr(cy), ptr(S), ptr(stats), ptr(mats),
                                          ctypes.byref(nkept)))
        return S, stats, mats, int(nkept.value)

    # ---- text that the device writes (K14 tracks, K20 coverage): chunk bounds, one chunk, all chunks double-buffered ----
    def _text_chunks(self, entry, attr, budget):
        """`entry`: cl_track_chunks / cl_cov_chunks -> (line bounds, byte bounds), also kept as self.<attr> for _text_render"""
        nc = ctypes.c_int64(0)
        _lib.check(entry(self._h, int(budget), 0, None, None, ctypes.byref(nc)))
        rec = np.zeros(nc.value + 1, dtype=np.int64)
        byt = np.zeros(nc.value + 1, dtype=np.int64)
        _lib.check(entry(self._h, int(budget), len(rec), _vp(rec), _vp(byt), ctypes.byref(nc)))
        setattr(self, attr, (rec, byt))
        return rec, byt

    def _text_render(self, entry, bounds, chunk, out):
        """`entry`: cl_track_render / cl_cov_render; bounds: what _text_chunks kept -> bytes, or with `out` their number"""
        nb = ctypes.c_int64(0)
        if out is None:
            rec, byt = bounds
            cap = max(1, int(byt[chunk + 1] - byt[chunk])) if 0 <= chunk < len(rec) - 1 else 1     # (the library reports the index)
            buf = np.empty(cap, dtype=np.uint8)
            _lib.check(entry(self._h, int(chunk), _vp(buf), len(buf), ctypes.byref(nb)))
            return buf[:nb.value].tobytes()
        if isinstance(out, tuple):
            ptr, cap = out
        else:
            a = np.frombuffer(out, dtype=np.uint8)
            ptr, cap = a.ctypes.data, len(a)
        _lib.check(entry(self._h, int(chunk), ctypes.c_void_p(ptr), int(cap), ctypes.byref(nb)))
        return int(nb.value)

    def _text_iter(self, render, chunks, budget):
        """the chunks of `chunks(budget)` in order, as memoryviews of two page-locked buffers: chunk k + 1 is rendered and copied to
        the host by `render` (on a helper thread; the library call releases the GIL) while the caller consumes chunk k"""
        rec, byt = chunks(budget)
        K = len(rec) - 1
        if K == 0:
            return
        size = int(np.max(np.diff(byt)))
        bufs = []
        pool = None
        fut = None
        try:
            for _ in range(2):
                bufs.append(_lib.host_alloc(size))
            from concurrent.futures import ThreadPoolExecutor
            pool = ThreadPoolExecutor(1)
            fut = pool.submit(render, 0, (bufs[0], size))
            for k in range(K):
                nb = fut.result()
                fut = pool.submit(render, k + 1, (bufs[(k + 1) & 1], size)) if k + 1 < K else None
                yield memoryview((ctypes.c_char * nb).from_address(bufs[k & 1])).cast("B")
        finally:                                   # (also when the caller abandons the generator: no render may outlive its buffer)
            if fut is not None:
                try:
                    fut.result()
                except Exception:
                    pass
            if pool is not None:
                pool.shutdown()
            for p in bufs:
                self._lib.cl_host_free(ctypes.c_void_p(p))

    # ---- ranged read-back (the *_get methods) and interval arguments ----
    def _range(self, size_attr, first, count):
        """-> (first, count, entries to allocate): count None = all from `first` on of the self.<size_attr> results on the device"""
        first = int(first)
        count = max(0, getattr(self, size_attr, 0) - first) if count is None else int(count)
        return first, count, max(0, count)

    def _get(self, entry, size_attr, first, count, dtypes, *lead):
        """`entry(handle, *lead, first, count, one array per dtype)` -> those arrays"""
        first, count, n = self._range(size_attr, first, count)
        out = tuple(np.zeros(n, dtype=t) for t in dtypes)
        _lib.check(entry(self._h, *lead, first, count, *[_vp(a) for a in out]))
        return out

    @staticmethod
    def _intervals(starts, ends, who):
        s, e = np.ascontiguousarray(starts, dtype=np.int64), np.ascontiguousarray(ends, dtype=np.int64)
        if s.ndim != 1 or s.shape != e.shape:
            raise ValueError("%s: starts and ends must be one-dimensional and of equal length" % who)
        return s, e

    TRACK_KINDS = {"washu": _lib.CL_TRACK_WASHU, "juice": _lib.CL_TRACK_JUICE}
    TRACK_NAME_MAX = _lib.CL_TRACK_NAME_MAX
    TRACK_BUDGET = 64 << 20                        # default bytes per rendered chunk

    def track_build(self, kind, cut, ext, ids, chr_a, chr_b):
        """K14: the browser-track lines of this chromosome's PETs (cLoops/io.py jd2washU / jd2hic, parseJd's cut) made on the device
        and kept for track_chunks / track_render.  kind "washu" (two lines per PET, sorted by start, end, row, side) or "juice"
        (one line per PET, row order); ids: the .jd's first column (int64 [n]) or None for the row numbers -> (records, bytes of
        the whole text)  (cl_track_build)"""
        if kind not in self.TRACK_KINDS:
            raise ValueError("unknown track kind %r (washu or juice)" % (kind,))
        ptr = None
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.int64).ravel()
            if len(ids) != self.n:
                raise ValueError("ids: %d entries for %d rows" % (len(ids), self.n))
            ptr = ids.ctypes.data_as(ctypes.c_void_p)
        nr, nb = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self._lib.cl_track_build(self._h, self.TRACK_KINDS[kind], int(cut), int(ext), ptr, chr_a.encode(), chr_b.encode(),
                                            ctypes.byref(nr), ctypes.byref(nb)))
        return int(nr.value), int(nb.value)

    def track_chunks(self, budget=TRACK_BUDGET):
        """the built track split into chunks of at most `budget` bytes, none splitting a line -> (record bounds, byte bounds), int64
        [chunks + 1]: chunk k is records rec[k] .. rec[k + 1] - 1, bytes byt[k] .. byt[k + 1] - 1 of the text  (cl_track_chunks)"""
        return self._text_chunks(self._lib.cl_track_chunks, "_track_bounds", budget)

    def track_render(self, chunk, out=None):
        """the text of chunk `chunk` of the last track_chunks -> bytes; with `out` (a writable buffer: bytearray, numpy uint8, or
        a (pointer, capacity) pair of page-locked memory) it is written there and its length returned  (cl_track_render)"""
        return self._text_render(self._lib.cl_track_render, getattr(self, "_track_bounds", ([0], [0])), chunk, out)

    def track_free(self):
        """releases the device scratch of track_build  (cl_track_free)"""
        _lib.check(self._lib.cl_track_free(self._h))

    def track_iter(self, budget=TRACK_BUDGET):
        """the chunks of the built track in order, as memoryviews of two page-locked buffers: chunk k + 1 is rendered and copied
        to the host (by a helper thread; the library call releases the GIL) while the caller consumes chunk k.  A view is valid
        until the next one is requested."""
        return self._text_iter(self.track_render, self.track_chunks, budget)

    COVERAGE_SCALE_MAX = 1 << 30                   # largest scale numerator of coverage_text

    def coverage_build(self, cut=0, ends=3, ext=75, res=0):
        """K20: the coverage of the genome by this chromosome's PET ends, built on the device and kept for coverage_runs /
        coverage_text.  Rows with Y - X >= cut (all for cut <= 0); ends: 1 = X, 2 = Y, 3 = both; an end point p stands for
        [max(0, p - ext), p + ext) (res == 0) or for its bin [floor(p / res) res, ... + res) (res >= 1, ext ignored) ->
        (n_runs, max_depth, n_ends, area): the maximal runs of constant depth > 0, the largest depth, the end points taken, the sum
        of depth * length over the runs  (cl_cov_build)"""
        res = int(res)
        nr, md, ne, ar = ctypes.c_int64(0), ctypes.c_uint32(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self._lib.cl_cov_build(self._h, int(cut), int(ends), 0 if res > 0 else int(ext), res, ctypes.byref(nr), ctypes.byref(md),
                                          ctypes.byref(ne), ctypes.byref(ar)))
        self._cov_runs = int(nr.value)
        self._cov_bounds = ([0], [0])
        return int(nr.value), int(md.value), int(ne.value), int(ar.value)

    def coverage_runs(self, first=0, count=None):
        """runs [first, first + count) of the built coverage (all from `first` on by default) -> (start int32, end int32, depth
        uint32)  (cl_cov_runs)"""
        return self._get(self._lib.cl_cov_runs, "_cov_runs", first, count, (np.int32, np.int32, np.uint32))

    def coverage_text(self, name, scale=None):
        """the bedGraph text of the built runs, one line `name\\tstart\\tend\\tvalue\\n` per run, laid out on the device -> its bytes.
        scale None: value = the depth; scale (num, den): the fixed-point number (depth * num + den // 2) // den thousandths with
        three decimals (counts per million: num = 10^9, den = the end points of every chromosome written)  (cl_cov_text)"""
        num, den = (0, 0) if scale is None else (int(scale[0]), int(scale[1]))
        if scale is not None and den < 1:
            raise ValueError("coverage_text: the scale's denominator must be >= 1, got %s" % (den,))
        nb = ctypes.c_int64(0)
        _lib.check(self._lib.cl_cov_text(self._h, name.encode(), num, den, ctypes.byref(nb)))
        return int(nb.value)

    def coverage_chunks(self, budget=TRACK_BUDGET):
        """the coverage text split into chunks of at most `budget` bytes, none splitting a line -> (run bounds, byte bounds), int64
        [chunks + 1]  (cl_cov_chunks)"""
        return self._text_chunks(self._lib.cl_cov_chunks, "_cov_bounds", budget)

    def coverage_render(self, chunk, out=None):
        """the text of chunk `chunk` of the last coverage_chunks -> bytes; with `out` (a writable buffer or a (pointer, capacity)
        pair of page-locked memory) it is written there and its length returned  (cl_cov_render)"""
        return self._text_render(self._lib.cl_cov_render, getattr(self, "_cov_bounds", ([0], [0])), chunk, out)

    def coverage_free(self):
        """releases the device scratch of coverage_build  (cl_cov_free)"""
        _lib.check(self._lib.cl_cov_free(self._h))
        self._cov_runs = 0

    def coverage_iter(self, budget=TRACK_BUDGET):
        """the chunks of the coverage text in order, as memoryviews of two page-locked buffers, like track_iter: chunk k + 1 is
        rendered and copied while the caller consumes chunk k.  A view is valid until the next one is requested."""
        return self._text_iter(self.coverage_render, self.coverage_chunks, budget)

    def peaks_sort(self, cut=0, ends=3):
        """K21: this chromosome's PET ends sorted once on the device and kept for peaks_call / peaks_count / peaks_summits.  Rows
        with Y - X >= cut (all for cut <= 0); ends: 1 = X, 2 = Y, 3 = both -> (n_ends, vmin, vmax): the end points taken, the
        smallest and the largest of them (0, 0, 0 without end points)  (cl_peak_sort)"""
        ne, lo, hi = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._peaks = 0
        _lib.check(self._lib.cl_peak_sort(self._h, int(cut), int(ends), ctypes.byref(ne), ctypes.byref(lo), ctypes.byref(hi)))
        return int(ne.value), int(lo.value), int(hi.value)

    def peaks_call(self, eps, minPts):
        """the candidate peaks of (eps, minPts) over the sorted end points: 1D DBSCAN in the order of the positions, a border point
        between two chains of cores going to the left one -> (n_peaks, n_cores, n_clustered); the peaks stay on the device for
        peaks_get until the next call or sort  (cl_peak_call)"""
        npk, nc, ncl = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._peaks = 0
        _lib.check(self._lib.cl_peak_call(self._h, int(eps), int(minPts), ctypes.byref(npk), ctypes.byref(nc), ctypes.byref(ncl)))
        self._peaks = int(npk.value)
        return int(npk.value), int(nc.value), int(ncl.value)

    def peaks_get(self, first=0, count=None):
        """peaks [first, first + count) of the last peaks_call (all from `first` on by default) -> (start int32, end int32, n_points
        uint32, n_cores uint32); [start, end) is half-open  (cl_peak_get)"""
        return self._get(self._lib.cl_peak_get, "_peaks", first, count, (np.int32, np.int32, np.uint32, np.uint32))

    def peaks_count(self, starts, ends):
        """the sorted end points in every half-open interval [starts[k], ends[k]) (int64 bounds; any order, overlapping, empty or
        beyond the end points) -> uint32 counts  (cl_peak_count)"""
        s, e = self._intervals(starts, ends, "peaks_count")
        out = np.zeros(len(s), dtype=np.uint32)
        _lib.check(self._lib.cl_peak_count(self._h, s.ctypes.data_as(ctypes.c_void_p), e.ctypes.data_as(ctypes.c_void_p), len(s),
                                           out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def peaks_summits(self, starts, ends, w):
        """the summit of every interval [starts[k], ends[k]) (ascending and disjoint): the position of its end point with the most
        end points within w bp, the smallest on ties, and that number -> (pos int32, -1 for an interval without points; cnt
        uint32)  (cl_peak_summits)"""
        s, e = self._intervals(starts, ends, "peaks_summits")
        pos, cnt = np.zeros(len(s), dtype=np.int32), np.zeros(len(s), dtype=np.uint32)
        _lib.check(self._lib.cl_peak_summits(self._h, s.ctypes.data_as(ctypes.c_void_p), e.ctypes.data_as(ctypes.c_void_p), len(s), int(w),
                                             pos.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(ctypes.c_void_p)))
        return pos, cnt

    def peaks_free(self):
        """releases the device scratch of peaks_sort and the calls after it  (cl_peak_free)"""
        _lib.check(self._lib.cl_peak_free(self._h))
        self._peaks = 0

    def domains_tracks(self, cut=0, res=10000, w=10):
        """K22: the three insulation tracks of this chromosome over bins of `res` bp with a window of `w` bins, kept on the device for
        domains_get / domains_count.  Rows with Y - X >= cut (all for cut <= 0), sorted by X once per cut (K19's table, shared with
        agg_loops): another w or res sorts nothing -> (n_bins, bin0, n_kept); entry k of a track stands for the boundary at the start
        of bin bin0 + k (0, 0, 0 without rows)  (cl_dom_tracks)"""
        nb, b0, nk = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self._lib.cl_dom_tracks(self._h, int(cut), int(res), int(w), ctypes.byref(nb), ctypes.byref(b0), ctypes.byref(nk)))
        self._dom_bins = int(nb.value)
        return int(nb.value), int(b0.value), int(nk.value)                   # (a refused call leaves the earlier tracks and their size)

    def domains_get(self, first=0, count=None):
        """entries [first, first + count) of the last domains_tracks (all from `first` on by default) -> (cross, up, down) uint32: the
        rows that cross the boundary inside the window, and those that stay in the window before / behind it  (cl_dom_get)"""
        return self._get(self._lib.cl_dom_get, "_dom_bins", first, count, (np.uint32, np.uint32, np.uint32))

    def domains_count(self, starts, ends):
        """the kept rows of the last domains_tracks in every half-open interval [starts[k], ends[k]) (int64 bounds; ascending and
        disjoint, possibly empty or abutting) -> (intra, nx, ny) uint32: rows with both ends, with X, with Y inside  (cl_dom_count)"""
        s, e = self._intervals(starts, ends, "domains_count")
        a, b, d = (np.zeros(len(s), dtype=np.uint32) for _ in range(3))
        _lib.check(self._lib.cl_dom_count(self._h, s.ctypes.data_as(ctypes.c_void_p), e.ctypes.data_as(ctypes.c_void_p), len(s),
                                          a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p),
                                          d.ctypes.data_as(ctypes.c_void_p)))
        return a, b, d

    def domains_free(self):
        """releases the tracks and the device scratch of domains_tracks / domains_count  (cl_dom_free)"""
        _lib.check(self._lib.cl_dom_free(self._h))
        self._dom_bins = 0

    def kdis_build(self, ks, cut=0):
        """K23: the distance |dx| + |dy| of every kept row to its k-th nearest other kept row, for up to 8 strictly ascending k in
        [1, 64] in one pass, and the log-binned histogram per k, kept on the device for kdis_get / kdis_hist.  Rows with Y - X >= cut
        (all for cut <= 0) in the order of K19's table (ascending X, equal X in input order; shared with agg_loops and
        domains_tracks).  k = minPts - 1: a row is a core of (eps, minPts) iff its d_k <= eps -> n_kept  (cl_kdis_build)"""
        ks = np.ascontiguousarray(np.atleast_1d(np.asarray(ks)), dtype=np.int32)
        if ks.ndim != 1:
            raise ValueError("kdis_build: ks must be one-dimensional")
        nk = ctypes.c_int64(0)
        _lib.check(self._lib.cl_kdis_build(self._h, int(cut), ks.ctypes.data_as(ctypes.c_void_p), len(ks), ctypes.byref(nk)))
        self._kdis_rows = int(nk.value)                                      # (a refused call leaves the earlier results and their size)
        return int(nk.value)

    def kdis_get(self, which=0, first=0, count=None):
        """entries [first, first + count) of the last kdis_build for its ks[which], in table order (all from `first` on by default)
        -> (x, y, d) int32: the row's coordinates and its k-distance, -1 where the kept rows have no k-th neighbour  (cl_kdis_get)"""
        return self._get(self._lib.cl_kdis_get, "_kdis_rows", first, count, (np.int32, np.int32, np.int32), int(which))

    def kdis_hist(self, which=0):
        """the histogram of the last kdis_build for its ks[which] -> (hist uint64[CL_KDIS_BINS] over the log bins of ests.logbin for
        d >= 1, n_zero: rows with d == 0, n_none: rows without a k-th neighbour)  (cl_kdis_hist)"""
        hist = np.zeros(_lib.CL_KDIS_BINS, dtype=np.uint64)
        nz, nn = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _lib.check(self._lib.cl_kdis_hist(self._h, int(which), hist.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nz), ctypes.byref(nn)))
        return hist, int(nz.value), int(nn.value)

    def kdis_free(self):
        """releases the k-distances and histograms of kdis_build  (cl_kdis_free)"""
        _lib.check(self._lib.cl_kdis_free(self._h))
        self._kdis_rows = 0

    def mat_window(self, res, bx0, by0, nx, ny, cut=0, mirror=False):
        """K24: the dense contact matrix of the bins [bx0, bx0 + nx) x [by0, by0 + ny) of `res` bp (bin of p = floor(p / res)) over the
        rows with Y - X >= cut (all for cut <= 0).  With `mirror` a row with bx != by also counts at its transposed cell, so a window on
        the diagonal is symmetric with its diagonal counted once -> (uint32 [nx, ny], n_in: the sum, n_kept)  (cl_mat_window)"""
        nx, ny = int(nx), int(ny)
        if not (1 <= nx <= _lib.CL_MAT_WMAX and 1 <= ny <= _lib.CL_MAT_WMAX and nx * ny <= _lib.CL_MAT_CELLS_MAX):
            raise ValueError("mat_window: needs 1 <= nx, ny <= %d and nx ny <= %d, got %d x %d" % (_lib.CL_MAT_WMAX, _lib.CL_MAT_CELLS_MAX, nx, ny))
        out = np.zeros((nx, ny), dtype=np.uint32)
        n_in, nk = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self._lib.cl_mat_window(self._h, int(cut), int(res), int(bx0), int(by0), nx, ny, 1 if mirror else 0,
                                           out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_in), ctypes.byref(nk)))
        return out, int(n_in.value), int(nk.value)

    def mat_cells(self, res, cut=0, fold=False):
        """K24: the non-empty cells (bx, by) of the kept rows at `res` bp, ascending by bx then by, with their counts, kept on the device
        for mat_cells_get; `fold` puts a row into (min(bx, by), max(bx, by)) -> (n_cells, n_kept, max_count)  (cl_mat_cells)"""
        nc, nk, mc = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self._lib.cl_mat_cells(self._h, int(cut), int(res), 1 if fold else 0, ctypes.byref(nc), ctypes.byref(nk), ctypes.byref(mc)))
        self._mat_cells = int(nc.value)                                      # (a refused call leaves the earlier cells and their number)
        self._bal_bins = 0                                                   # (K25's and K26's state went with the earlier cells)
        self._exp_diags = 0
        return int(nc.value), int(nk.value), int(mc.value)

    def mat_cells_get(self, first=0, count=None):
        """cells [first, first + count) of the last mat_cells (all from `first` on by default) -> (bx int32, by int32, cnt uint32)
        (cl_mat_cells_get)"""
        return self._get(self._lib.cl_mat_cells_get, "_mat_cells", first, count, (np.int32, np.int32, np.uint32))

    def mat_v4c(self, res, v0, v1, b0, nb, cut=0):
        """K24: the virtual-4C profile of the viewpoint [v0, v1) bp over the bins [b0, b0 + nb) of `res` bp: a kept row adds 1 at the bin
        of its Y when its X lies in the viewpoint, and 1 at the bin of its X when its Y does -> (uint32 [nb], n_x, n_y: the rows with X /
        Y in the viewpoint, n_kept)  (cl_mat_v4c)"""
        nb = int(nb)
        if not 0 <= nb <= (1 << 24):
            raise ValueError("mat_v4c: nb must lie in [0, 2^24], got %d" % nb)
        if int(v0) > int(v1):
            raise ValueError("mat_v4c: the viewpoint needs v0 <= v1, got [%d, %d)" % (int(v0), int(v1)))
        out = np.zeros(nb, dtype=np.uint32)
        nx, ny, nk = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self._lib.cl_mat_v4c(self._h, int(cut), int(res), int(v0), int(v1), int(b0), nb, out.ctypes.data_as(ctypes.c_void_p),
                                        ctypes.byref(nx), ctypes.byref(ny), ctypes.byref(nk)))
        return out, int(nx.value), int(ny.value), int(nk.value)

    def mat_free(self):
        """releases the cells of mat_cells and the device scratch of the mat_* calls  (cl_mat_free)"""
        _lib.check(self._lib.cl_mat_free(self._h))
        self._mat_cells = 0
        self._bal_bins = 0
        self._exp_diags = 0

    def bal_marginals(self, ignore_diags=2):
        """K25: the raw marginals of the folded cells of the last mat_cells(fold=True), kept on the device with the cells' transposed
        order for bal_iterate.  A cell is used iff by - bx >= ignore_diags; the bins are b0 = the first cell's bx .. the largest by
        -> (b0, nb, n_used)  (cl_bal_marginals)"""
        b0, nb, nu = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self._lib.cl_bal_marginals(self._h, int(ignore_diags), ctypes.byref(b0), ctypes.byref(nb), ctypes.byref(nu)))
        self._bal_bins = int(nb.value)
        self._exp_diags = 0                                                  # (K26's diagonals were those of the earlier marginals)
        return int(b0.value), int(nb.value), int(nu.value)

    def bal_marginals_get(self, first=0, count=None):
        """bins [first, first + count) of the last bal_marginals (all from `first` on by default) -> (sum uint64: the counts of the used
        cells that touch the bin, nnz uint32: their number)  (cl_bal_marginals_get)"""
        return self._get(self._lib.cl_bal_marginals_get, "_bal_bins", first, count, (np.uint64, np.uint32))

    def bal_iterate(self, valid, max_iters=200, tol=1e-5):
        """K25: iterative correction over the used cells, from w = 1 on the bins with valid != 0, until the variance of the non-zero
        marginals falls below tol or max_iters iterations are done -> (iters, converged, var, scale); the weights stay on the device
        for bal_weights / bal_cells_get.  May be repeated with another mask or tol  (cl_bal_iterate)"""
        valid = np.asarray(valid)
        nb = getattr(self, "_bal_bins", 0)
        if valid.ndim != 1 or len(valid) != nb:
            raise ValueError("bal_iterate: the mask needs one entry per bin (%d), got shape %s" % (nb, valid.shape))
        v = np.ascontiguousarray(valid != 0, dtype=np.uint32)
        it, cv, var, sc = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        _lib.check(self._lib.cl_bal_iterate(self._h, v.ctypes.data_as(ctypes.c_void_p), int(max_iters), float(tol), ctypes.byref(it),
                                            ctypes.byref(cv), ctypes.byref(var), ctypes.byref(sc)))
        self._exp_diags = 0                                                  # (... and of the earlier weights)
        return int(it.value), bool(cv.value), float(var.value), float(sc.value)

    def bal_weights(self, first=0, count=None):
        """the weights of the bins [first, first + count) after the last bal_iterate -> float64, NaN at the bins that are masked or
        got no weight  (cl_bal_weights_get)"""
        return self._get(self._lib.cl_bal_weights_get, "_bal_bins", first, count, (np.float64,))[0]

    def bal_cells_get(self, first=0, count=None):
        """the balanced values cnt weight[bx] weight[by] of the cells [first, first + count) of mat_cells, in their order -> float64
        (cl_bal_cells_get)"""
        return self._get(self._lib.cl_bal_cells_get, "_mat_cells", first, count, (np.float64,))[0]

    def bal_free(self):
        """releases the marginals, weights and device scratch of the bal_* calls; the cells stay  (cl_bal_free)"""
        _lib.check(self._lib.cl_bal_free(self._h))
        self._bal_bins = 0
        self._exp_diags = 0

    def exp_diagonals(self, valid=None, balanced=True):
        """K26: per diagonal d = by - bx of the folded cells the valid bin pairs, the count sum and the value sum of the used cells (d >=
        the ignore_diags of bal_marginals, both bins valid), kept on the device for exp_diagonals_get / exp_set / exp_cells_get.
        balanced: the weights of the last bal_iterate, a bin being valid iff its weight is a number (valid must be None); else the
        raw counts over the bins with valid != 0 (None: all bins) -> (nd, n_used)  (cl_exp_diagonals)"""
        ptr = None
        if valid is not None:
            valid = np.asarray(valid)
            nb = getattr(self, "_bal_bins", 0)
            if valid.ndim != 1 or len(valid) != nb:
                raise ValueError("exp_diagonals: the mask needs one entry per bin (%d), got shape %s" % (nb, valid.shape))
            v = np.ascontiguousarray(valid != 0, dtype=np.uint32)
            ptr = _vp(v)
        nd, nu = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self._lib.cl_exp_diagonals(self._h, ptr, 1 if balanced else 0, ctypes.byref(nd), ctypes.byref(nu)))
        self._exp_diags = int(nd.value)
        return int(nd.value), int(nu.value)

    def exp_diagonals_get(self, first=0, count=None):
        """diagonals [first, first + count) of the last exp_diagonals (all from `first` on by default) -> (n_pairs int64, cnt_sum
        uint64, val_sum float64)  (cl_exp_diagonals_get)"""
        return self._get(self._lib.cl_exp_diagonals_get, "_exp_diags", first, count, (np.int64, np.uint64, np.float64))

    def exp_set(self, expected):
        """the expected value of every diagonal of the last exp_diagonals (float64 [nd]; NaN or 0: no O/E on that diagonal), for
        exp_cells_get.  May be repeated  (cl_exp_set)"""
        e = np.ascontiguousarray(expected, dtype=np.float64)
        if e.ndim != 1:
            raise ValueError("exp_set: the expected values must be one-dimensional")
        _lib.check(self._lib.cl_exp_set(self._h, _vp(e), len(e)))

    def exp_cells_get(self, first=0, count=None):
        """the O/E values ((w[bx] cnt) w[by]) / expected[by - bx] of the cells [first, first + count) of mat_cells, in their order ->
        float64, NaN where the cell is not used or its diagonal has no expected value  (cl_exp_cells_get)"""
        return self._get(self._lib.cl_exp_cells_get, "_mat_cells", first, count, (np.float64,))[0]

    def exp_free(self):
        """releases the diagonals, expected values and device scratch of the exp_* calls; cells, marginals and weights stay
        (cl_exp_free)"""
        _lib.check(self._lib.cl_exp_free(self._h))
        self._exp_diags = 0

    def eig_build(self, clip=float("inf"), dmax=None):
        """K27: describes M = min(O/E, clip) - 1 over the valid bin pairs with ignore_diags <= |i - j| < dmax (0 elsewhere; O/E is 0
        where there is no cell) from the cells, weights and expected values of the last exp_set, kept on the device for eig_apply /
        eig_iterate.  dmax None: all diagonals (nb).  Refused when a diagonal of the band with valid pairs has no finite positive
        expected value -> (n_valid, n_in: the cells inside the band)  (cl_eig_build)"""
        nv, ni = ctypes.c_int64(0), ctypes.c_int64(0)
        dmax = getattr(self, "_bal_bins", 0) if dmax is None else int(dmax)
        _lib.check(self._lib.cl_eig_build(self._h, float(clip), dmax, ctypes.byref(nv), ctypes.byref(ni)))
        return int(nv.value), int(ni.value)

    def eig_apply(self, x):
        """y = M x for the vectors x: float64 [nb] or [n_vec, nb], 1 <= n_vec <= CL_EIG_BLOCK; the invalid bins of x read as 0 -> y of
        the same shape  (cl_eig_apply)"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        nb = getattr(self, "_bal_bins", 0)
        if x.ndim not in (1, 2) or x.shape[-1] != nb:
            raise ValueError("eig_apply: the vectors need one entry per bin (%d), got shape %s" % (nb, x.shape))
        n_vec = 1 if x.ndim == 1 else x.shape[0]
        if not 1 <= n_vec <= _lib.CL_EIG_BLOCK:
            raise ValueError("eig_apply: needs 1 .. %d vectors, got %d" % (_lib.CL_EIG_BLOCK, n_vec))
        y = np.zeros_like(x)
        _lib.check(self._lib.cl_eig_apply(self._h, _vp(x), n_vec, _vp(y)))
        return y

    def eig_iterate(self, n_eigs=3, max_iters=1000, tol=1e-8):
        """K27: subspace iteration for the n_eigs (1 .. CL_EIG_MAX) eigenpairs of M of largest |lambda|, until every residual |M v -
        lambda v| is at most tol |lambda_0| or max_iters iterations are done -> (iters, converged, eigvals float64 [n_eigs] by |lambda|
        descending, resid float64 [n_eigs]); NaN where there are fewer valid bins than n_eigs.  The vectors stay on the device for
        eig_vectors  (cl_eig_iterate)"""
        n_eigs = int(n_eigs)
        if not 1 <= n_eigs <= _lib.CL_EIG_MAX:
            raise ValueError("eig_iterate: n_eigs must lie in [1, %d], got %d" % (_lib.CL_EIG_MAX, n_eigs))
        it, cv = ctypes.c_int32(0), ctypes.c_int32(0)
        lam, res = np.full(n_eigs, np.nan), np.full(n_eigs, np.nan)
        _lib.check(self._lib.cl_eig_iterate(self._h, n_eigs, int(max_iters), float(tol), ctypes.byref(it), ctypes.byref(cv), _vp(lam), _vp(res)))
        return int(it.value), bool(cv.value), lam, res

    def eig_vectors(self, which=0, first=0, count=None):
        """entries [first, first + count) of vector `which` of the last eig_iterate (all from `first` on by default) -> float64: unit
        2-norm over the valid bins, NaN on the others, the entry of largest magnitude positive  (cl_eig_vectors_get)"""
        return self._get(self._lib.cl_eig_vectors_get, "_bal_bins", first, count, (np.float64,), int(which))[0]

    def eig_free(self):
        """releases the matrix, the vectors and the device scratch of the eig_* calls; everything up to the expected values stays
        (cl_eig_free)"""
        _lib.check(self._lib.cl_eig_free(self._h))

    def scc_moments(self, other, b0, nb, h=0, n_diags=None):
        """K28: the moments of the stratum-adjusted correlation of this handle's and `other`'s contact matrix (both after
        mat_cells(res, fold=True) at one res; `other` may be this handle) over the bins [b0, b0 + nb): both matrices under a (2h+1)^2
        box sum, and per diagonal d < n_diags (None: nb) over the positions where either sum is non-zero -> (n int64, sx, sy, sxx, syy,
        sxy uint64), n_diags entries each.  The scratch stays with this handle  (cl_scc_moments)"""
        if not isinstance(other, Chromosome):
            raise ValueError("scc_moments: the other sample must be a Chromosome, got %r" % (other,))
        nb, h = int(nb), int(h)
        D = nb if n_diags is None else int(n_diags)
        if not 0 <= h <= _lib.CL_SCC_HMAX:
            raise ValueError("scc_moments: h must lie in [0, %d], got %d" % (_lib.CL_SCC_HMAX, h))
        if nb < 0 or not (1 <= D <= nb or D == nb == 0):
            raise ValueError("scc_moments: needs nb >= 0 and 1 <= n_diags <= nb (0 with nb = 0), got nb %d, n_diags %d" % (nb, D))
        if nb * (D + 4 * h) > _lib.CL_SCC_BAND_MAX:
            raise ValueError("scc_moments: the band nb (n_diags + 4 h) = %d has more than %d entries: fewer diagonals, a smaller h or a "
                             "larger res" % (nb * (D + 4 * h), _lib.CL_SCC_BAND_MAX))
        n = np.zeros(D, dtype=np.int64)
        m = [np.zeros(D, dtype=np.uint64) for _ in range(5)]
        ptr = [a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if D else None for a in m]
        _lib.check(self._lib.cl_scc_moments(self._h, other._h, int(b0), nb, h, D, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if D else None,
                                            *ptr))
        return (n,) + tuple(m)

    def scc_free(self):
        """releases the device scratch of scc_moments; the cells stay  (cl_scc_free)"""
        _lib.check(self._lib.cl_scc_free(self._h))

    def dot_lambdas(self, p, w, dmin, dmax=None):
        """K29: the four neighbourhood sums (donut, lower-left, horizontal, vertical; inner half-width p, outer w) of observed and
        expected around every pixel (i, i + d), dmin <= d < dmax, of the matrix of the last exp_set, and the local expected counts la_k
        they imply, kept on the device for dot_lambdas_get / dot_cells / dot_hist / dot_call.  dmin: at or above the
        ignore_diags of bal_marginals; dmax None: all diagonals (nb) -> (n_cand, n_full)  (cl_dot_lambdas)"""
        p, w = int(p), int(w)
        if not 0 <= p < w <= _lib.CL_DOT_WMAX:
            raise ValueError("dot_lambdas: needs 0 <= p < w <= %d, got p %d, w %d" % (_lib.CL_DOT_WMAX, p, w))
        nb = getattr(self, "_bal_bins", 0)
        dmax = nb if dmax is None else int(dmax)
        nc, nf = ctypes.c_int64(0), ctypes.c_int64(0)
        dmin = int(dmin)
        if nb * (dmax + 4 * w) > _lib.CL_DOT_BAND_MAX:
            raise ValueError("dot_lambdas: the band nb (dmax + 4 w) = %d has more than %d entries: fewer diagonals, a smaller w or a larger "
                             "res" % (nb * (dmax + 4 * w), _lib.CL_DOT_BAND_MAX))
        _lib.check(self._lib.cl_dot_lambdas(self._h, p, w, dmin, dmax, ctypes.byref(nc), ctypes.byref(nf)))
        self._dot_bins, self._dot_nd, self._dot_chunks, self._dot_sig = nb, dmax - dmin, 0, 0
        return int(nc.value), int(nf.value)

    def dot_lambdas_get(self, kernel, first_bin=0, n_bins=None):
        """la of neighbourhood `kernel` (0 donut, 1 lower-left, 2 horizontal, 3 vertical) for the bins [first_bin, first_bin + n_bins)
        (all from `first_bin` on by default) -> float64 [n_bins, dmax - dmin]: row = bin i, column = d - dmin; NaN where the pixel is no
        candidate or the neighbourhood's expected sum is 0  (cl_dot_lambdas_get)"""
        first, count, n = self._range("_dot_bins", first_bin, n_bins)
        out = np.zeros((n, getattr(self, "_dot_nd", 0)), dtype=np.float64)
        _lib.check(self._lib.cl_dot_lambdas_get(self._h, int(kernel), first, count, _vp(out) if out.size else None))
        return out

    def dot_cells(self, first=0, count=None):
        """the four la of the cells [first, first + count) of mat_cells, in their order -> float64 [count, 4], NaN where the cell's pixel
        is no candidate  (cl_dot_cells_get)"""
        first, count, n = self._range("_mat_cells", first, count)
        out = np.zeros((n, 4), dtype=np.float64)
        _lib.check(self._lib.cl_dot_cells_get(self._h, first, count, _vp(out) if n else None))
        return out

    def dot_hist(self, edges):
        """K29: the histogram of the full pixels of the last dot_lambdas over the chunks of la (chunk(x) = the smallest l with x <=
        edges[l]; edges finite, above 0, strictly ascending, at most CL_DOT_CHUNKS_MAX) and their raw counts, saturated at CL_DOT_CMAX
        -> (uint64 [4, n_chunks, CL_DOT_CMAX + 1], n_beyond: the full pixels with a la above the last edge, left out)  (cl_dot_hist)"""
        e = np.ascontiguousarray(edges, dtype=np.float64)
        if e.ndim != 1 or not 1 <= len(e) <= _lib.CL_DOT_CHUNKS_MAX:
            raise ValueError("dot_hist: needs 1 .. %d edges, got shape %s" % (_lib.CL_DOT_CHUNKS_MAX, e.shape))
        hist = np.zeros((4, len(e), _lib.CL_DOT_CMAX + 1), dtype=np.uint64)
        nbey = ctypes.c_uint64(0)
        _lib.check(self._lib.cl_dot_hist(self._h, _vp(e), len(e), _vp(hist), ctypes.byref(nbey)))
        self._dot_chunks, self._dot_sig = len(e), 0
        return hist, int(nbey.value)

    def dot_call(self, thr):
        """K29: the cells whose pixel is full, not beyond, and has cnt >= thr[k][chunk(la_k)] for all four k; thr: uint32 [4, n_chunks]
        over the edges of the last dot_hist -> n_sig; the list stays on the device for dot_sig  (cl_dot_call)"""
        t = np.ascontiguousarray(thr, dtype=np.uint32)
        n = getattr(self, "_dot_chunks", 0)                                  # (0: no histogram; the library refuses before it reads thr)
        if n and t.shape != (4, n):
            raise ValueError("dot_call: the thresholds need shape (4, %d), got %s" % (n, t.shape))
        ns = ctypes.c_int64(0)
        _lib.check(self._lib.cl_dot_call(self._h, _vp(t), ctypes.byref(ns)))
        self._dot_sig = int(ns.value)
        return int(ns.value)

    def dot_sig(self, first=0, count=None):
        """entries [first, first + count) of the last dot_call's list (all from `first` on by default) -> int64, ascending: indices
        into the order of mat_cells  (cl_dot_sig_get)"""
        return self._get(self._lib.cl_dot_sig_get, "_dot_sig", first, count, (np.int64,))[0]

    def dot_free(self):
        """releases the band, the la, the histogram and the list of the dot_* calls; everything up to the expected values stays
        (cl_dot_free)"""
        _lib.check(self._lib.cl_dot_free(self._h))
        self._dot_bins = self._dot_nd = self._dot_chunks = self._dot_sig = 0

    def sad_sums(self, cls, n_cls, lo, hi):
        """K30: the saddle tables of the matrix of the last exp_set.  cls: the class of every bin (int [nb]; -1: the bin takes no part,
        else 0 <= cls < n_cls <= CL_SAD_CLASSES_MAX); the band max(ignore_diags, 1) <= lo <= hi <= nb.  Over the pairs i < j of valid
        classed bins with lo <= j - i < hi, per (class of i, class of j): their number, their cells and the sum of the cells' O/E, kept
        for sad_get.  Refused when a diagonal of the band with valid pairs has no finite positive expected value -> (n_binned: the
        valid bins with a class, n_pairs, n_in: the totals of the pairs and of the cells)  (cl_sad_sums)"""
        cls = np.asarray(cls)
        nb, n_cls = getattr(self, "_bal_bins", 0), int(n_cls)
        if cls.ndim != 1 or len(cls) != nb or (cls.size and cls.dtype.kind not in "iu"):
            raise ValueError("sad_sums: the classes need one integer per bin (%d), got %s of shape %s" % (nb, cls.dtype, cls.shape))
        if not 1 <= n_cls <= _lib.CL_SAD_CLASSES_MAX:
            raise ValueError("sad_sums: n_cls must lie in [1, %d], got %d" % (_lib.CL_SAD_CLASSES_MAX, n_cls))
        if cls.size and (int(cls.min()) < -1 or int(cls.max()) >= n_cls):
            raise ValueError("sad_sums: a class outside [-1, %d)" % n_cls)
        k = np.ascontiguousarray(cls, dtype=np.int32)
        nbin, npair, nin = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self._lib.cl_sad_sums(self._h, _vp(k) if nb else None, nb, n_cls, int(lo), int(hi), ctypes.byref(nbin), ctypes.byref(npair),
                                         ctypes.byref(nin)))
        self._sad_cls = n_cls
        return int(nbin.value), int(npair.value), int(nin.value)

    def sad_get(self):
        """the tables of the last sad_sums -> (sum float64, pairs int64, cells int64), each [n_cls, n_cls]: row = the class of the
        lower bin, column = the class of the upper bin  (cl_sad_get)"""
        n = getattr(self, "_sad_cls", 0) or 1                                # (no tables: the library refuses before it writes)
        s, p, c = np.zeros((n, n), np.float64), np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
        _lib.check(self._lib.cl_sad_get(self._h, _vp(s), _vp(p), _vp(c)))
        return s, p, c

    def sad_free(self):
        """releases the tables and the device scratch of the sad_* calls; everything up to the expected values stays  (cl_sad_free)"""
        _lib.check(self._lib.cl_sad_free(self._h))
        self._sad_cls = 0

    def neighbor_counts(self, eps, cut=0):
        out = np.full(self.n, -1, dtype=np.int32)
        _lib.check(self._lib.cl_neighbor_counts(self._h, int(eps), int(cut), out.ctypes.data_as(ctypes.c_void_p)))
        return out


def kde_array(d, lo, step, inv_h, gridsize, device=0):
    """K17 over a plain array of integer distances, each of weight 1 (|d| is taken, zeros are dropped) -> float64[gridsize]:
    S[j] = sum_i exp(-((log2|d_i| - (lo + j step)) inv_h)^2 / 2), unnormalised (cl_kde_array)"""
    d = np.asarray(d)
    if d.ndim != 1 or (d.size and d.dtype.kind not in "iu"):
        raise TypeError("kde_array: a one-dimensional integer array required")
    if d.size and (d.min() < -(2 ** 31 - 1) or d.max() > 2 ** 31 - 1):
        raise _lib.CloopsHipError(_lib.CL_ERR_DOMAIN, "distances must satisfy |d| < 2^31")
    d = np.ascontiguousarray(d, dtype=np.int32)
    out = np.zeros(max(int(gridsize), 1), dtype=np.float64)
    _lib.check(_lib.load().cl_kde_array(int(device), d.ctypes.data_as(ctypes.c_void_p), int(d.shape[0]), float(lo), float(step),
                                        float(inv_h), int(gridsize), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return out


class Converter(_Handle):
    """K15: a pairs-to-BEDPE converter on the device (cl_conv of include/cloops_hip.h), shaped like Chromosome.track_*: feed a chunk of
    complete lines, render their BEDPE text.  fmt "hicpro" (scripts/hicpropairs2bedpe), "juicer" (scripts/juicerLong2bedpe.py) or
    "pairs" (4DN pairs: hicpro's rule on other columns, no script of the reference)."""
    FORMATS = {"hicpro": _lib.CL_CONV_HICPRO, "juicer": _lib.CL_CONV_JUICER}      # the two scripts of the reference
    OWN_FORMATS = {"pairs": _lib.CL_CONV_PAIRS}
    KINDS = {_lib.CL_CONV_E_FIELDS: "fewer than 7 fields", _lib.CL_CONV_E_INT: "not an integer", _lib.CL_CONV_E_RANGE: "integer outside int64",
             _lib.CL_CONV_E_LONG: "line longer than the chunk budget"}
    BUDGET = 64 << 20                              # default bytes per chunk
    _DESTROY = "cl_conv_destroy"

    def __init__(self, fmt, ext, budget=BUDGET, device=0, stream=None):
        formats = dict(self.FORMATS, **self.OWN_FORMATS)
        if fmt not in formats:
            raise ValueError("unknown pairs format %r (hicpro, juicer or pairs)" % (fmt,))
        self.fmt, self.ext, self.budget = fmt, int(ext), int(budget)
        self._open("cl_conv_create", int(device), ctypes.c_void_p(stream), formats[fmt], self.ext, self.budget)

    def feed(self, ptr, n, last):
        """the complete lines of the n bytes at host address `ptr` (all of them with `last`) -> (bytes consumed, lines converted,
        bytes of their text, error): error None, or (line number counted over this handle's feeds, reason) of the first line the
        reference would raise on -- the lines in front of it are converted  (cl_conv_feed, cl_conv_error)"""
        used, nl, nb = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        rc = self._lib.cl_conv_feed(self._h, ctypes.c_void_p(ptr), int(n), int(bool(last)), ctypes.byref(used), ctypes.byref(nl),
                                    ctypes.byref(nb))
        err = None
        if rc == _lib.CL_ERR_PARSE:
            line, kind = ctypes.c_int64(0), ctypes.c_int32(0)
            _lib.check(self._lib.cl_conv_error(self._h, ctypes.byref(line), ctypes.byref(kind)))
            err = (int(line.value), self.KINDS.get(int(kind.value), "error %d" % kind.value))
        else:
            _lib.check(rc)
        return int(used.value), int(nl.value), int(nb.value), err

    def render(self, ptr, cap):
        """the text of the last feed's lines into `cap` bytes of host memory at `ptr` -> its length  (cl_conv_render)"""
        nb = ctypes.c_int64(0)
        _lib.check(self._lib.cl_conv_render(self._h, ctypes.c_void_p(ptr), int(cap), ctypes.byref(nb)))
        return int(nb.value)

    def timing(self):
        """device ms of the last feed and render: h2d, feed kernels, render kernel, d2h  (cl_conv_timing)"""
        ms = (ctypes.c_float * 4)()
        _lib.check(self._lib.cl_conv_timing(self._h, ms))
        return {"h2d": ms[0], "feed": ms[1], "render": ms[2], "d2h": ms[3]}


class Ingest(_Handle):
    """K16: a BEDPE reader on the device (cl_ingest of include/cloops_hip.h), shaped like Converter: feed a chunk of complete lines,
    read its distinct chromosome names, commit the host's table for them; finish joins two handles and leaves every chromosome's
    mid-points in HBM.  fmt "pairs" (K18) reads 4DN pairs text as the BEDPE that Converter("pairs", ext) makes of it."""
    FORMATS = {"bedpe": _lib.CL_INGEST_BEDPE, "pairs": _lib.CL_INGEST_PAIRS}
    TIMES = ("h2d", "index", "parse", "names", "commit", "finish")       # CL_INGEST_TIMES of them
    BUDGET = 64 << 20                              # default bytes per chunk
    _DESTROY = "cl_ingest_destroy"

    def __init__(self, budget=BUDGET, cut=0, want_distances=False, device=0, stream=None, fmt="bedpe", ext=0):
        if fmt not in self.FORMATS:
            raise ValueError("unknown input format %r (bedpe or pairs)" % (fmt,))
        self.device, self.budget, self.fmt, self.ext = int(device), int(budget), fmt, int(ext)
        self._open("cl_ingest_create", int(device), ctypes.c_void_p(stream), self.budget, int(cut), int(bool(want_distances)))
        if fmt != "bedpe":
            try:
                _lib.check(self._lib.cl_ingest_set_format(self._h, self.FORMATS[fmt], self.ext))
            except BaseException:
                self.close()
                raise

    def feed(self, ptr, n):
        """the n bytes of complete lines at host address `ptr` -> (lines, first exotic line or -1, distinct names or -1 for too
        many)  (cl_ingest_feed)"""
        nl, ex, nn = ctypes.c_int64(0), ctypes.c_int64(-1), ctypes.c_int64(0)
        _lib.check(self._lib.cl_ingest_feed(self._h, ctypes.c_void_p(ptr), int(n), ctypes.byref(nl), ctypes.byref(ex), ctypes.byref(nn)))
        return int(nl.value), int(ex.value), int(nn.value)

    def error(self):
        """pairs: the first line of the last feed the converter raises on -> (line in the feed, 1-based, headers counted; reason), or
        None  (cl_ingest_error)"""
        line, kind = ctypes.c_int64(0), ctypes.c_int32(0)
        _lib.check(self._lib.cl_ingest_error(self._h, ctypes.byref(line), ctypes.byref(kind)))
        if line.value == 0:
            return None
        return int(line.value), Converter.KINDS.get(int(kind.value), "error %d" % kind.value)

    def headers(self):
        """pairs: the header lines among the last feed's lines  (cl_ingest_headers)"""
        n = ctypes.c_int64(0)
        _lib.check(self._lib.cl_ingest_headers(self._h, ctypes.byref(n)))
        return int(n.value)

    def names(self, n):
        """the last feed's distinct names -> [(hash, first line, offset, length)], by first line  (cl_ingest_names)"""
        if n <= 0:
            return []
        arr = (_lib.ClIngestName * n)()
        got = ctypes.c_int64(0)
        _lib.check(self._lib.cl_ingest_names(self._h, arr, n, ctypes.byref(got)))
        return sorted(((int(e.hash), int(e.first), int(e.off), int(e.len)) for e in arr[:got.value]), key=lambda t: t[1])

    def commit(self, chunk, line0, table, n_ids):
        """the host's answer for the last feed: table = [(hash, id or -1, name bytes)] -> (PETs appended per id, status)
        (cl_ingest_commit)"""
        table = sorted(table)
        nt = len(table)
        hashes = np.array([t[0] for t in table], dtype=np.uint64)
        ids = np.array([t[1] for t in table], dtype=np.int32)
        lens = np.array([len(t[2]) for t in table], dtype=np.uint32)
        offs = np.zeros(nt, dtype=np.uint32)
        if nt:
            offs[1:] = np.cumsum(lens[:-1])
        blob = b"".join(t[2] for t in table)
        counts = np.zeros(max(n_ids, 1), dtype=np.int64)
        status = ctypes.c_int32(0)
        vp = ctypes.c_void_p
        _lib.check(self._lib.cl_ingest_commit(self._h, int(chunk), int(line0), hashes.ctypes.data_as(vp), ids.ctypes.data_as(vp),
                                              offs.ctypes.data_as(vp), lens.ctypes.data_as(vp), nt, ctypes.c_char_p(blob), len(blob), int(n_ids),
                                              counts.ctypes.data_as(vp), ctypes.byref(status)))
        return counts[:n_ids], int(status.value)

    def finish(self, other, n_ids, unique):
        """-> (rows per id, number of distances)  (cl_ingest_finish)"""
        rows = np.zeros(max(n_ids, 1), dtype=np.int64)
        nd = ctypes.c_int64(0)
        _lib.check(self._lib.cl_ingest_finish(self._h, other._h if other is not None else None, int(n_ids), int(bool(unique)),
                                              rows.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nd)))
        return rows[:n_ids], int(nd.value)

    def rows(self, cid, n):
        """the int64 mid-points (cA, cB) of chromosome `cid`  (cl_ingest_rows)"""
        a, b = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
        _lib.check(self._lib.cl_ingest_rows(self._h, int(cid), a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), n))
        return a, b

    def chrom_arrays(self, cid):
        """-> (n, device address of X, of Y): int32 arrays that live as long as this object  (cl_ingest_chrom_arrays)"""
        n, x, y = ctypes.c_int64(0), ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(self._lib.cl_ingest_chrom_arrays(self._h, int(cid), ctypes.byref(n), ctypes.byref(x), ctypes.byref(y)))
        return int(n.value), x.value, y.value

    def distances(self, n):
        out = np.empty(n, dtype=np.int64)
        _lib.check(self._lib.cl_ingest_distances(self._h, out.ctypes.data_as(ctypes.c_void_p), n))
        return out

    def timing(self):
        """device ms summed over this handle's calls  (cl_ingest_timing)"""
        ms = (ctypes.c_float * len(self.TIMES))()
        _lib.check(self._lib.cl_ingest_timing(self._h, ms))
        return dict(zip(self.TIMES, ms))
