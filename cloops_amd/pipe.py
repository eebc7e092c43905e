"""Per-chromosome dispatch of the clustering hot path -- drop-in for the reference's
cLoops/pipe.py:52-174 (`singleDBSCAN`, `runDBSCAN`, `filterClusterByDis`, `checkSameLoop`,
`combineTwice`) plus the (eps, minPts) sweep loop of cLoops/pipe.py:241-281 (`runSweep`).

Same names, argument meaning, return shapes and stderr report lines as the reference.
What differs is where the work happens:

  * a chromosome's .jd matrix is loaded ONCE and stays resident in HBM across the sweep
    (the reference re-reads the file in every step, io.py:206-217 via pipe.py:58);
  * the cut filter (pipe.py:59-63), the clustering (pipe.py:70) and the per-cluster
    bounding boxes (the O(K*N) pandas loop of pipe.py:78-102) run on the GPU;
  * `runDBSCAN` spreads chromosomes over the visible GPUs (one host thread per GPU) instead
    of joblib worker processes (pipe.py:117).
"""
import contextlib
import itertools
import os
import sys
import threading
import time
from collections import OrderedDict, namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import api
from . import _roctx
from ._lib import DIST_LOGBINS
from .cDBSCAN2 import cDBSCAN as DBSCAN          # pipe.py:42  (production variant)
from .dist import lpt_assign
from .ests import estIntSelCutFrag, estIntSelCutFrag_bounded, logbin, logbin_range

#: clustering variant used by singleDBSCAN; "block" mirrors the alternative import at pipe.py:43
DBSCAN_VARIANT = "v2"


def parseJd(f, cut=0):
    """cLoops/io.py:206-217: `.jd` = joblib-pickled int64 [n,3] rows [id, X, Y]; key from the
    file name 'chrA-chrB.jd'."""
    import joblib
    key = os.path.split(f)[1].replace(".jd", "")
    key = tuple(key.split("-"))
    mat = joblib.load(f)
    if cut > 0:
        d = mat[:, 2] - mat[:, 1]
        p = np.where(d >= cut)[0]
        mat = mat[p, :]
    return key, mat


# ---------------------------------------------------------------------------------------
# resident chromosomes
# ---------------------------------------------------------------------------------------
#: The chromosomes of one GPU share this many HIP streams (0: every chromosome gets a stream of its own).  A sweep step
#: enqueues every chromosome's run and then collects them; how many of those runs execute side by side is what the streams
#: decide.  One stream per chromosome leaves that to how the HIP runtime maps 23+ streams onto its hardware queues
#: (GPU_MAX_HW_QUEUES, default 4): measured on the 200 M-PET mode-3 sweep 1 queue 0.270 s, 2: 0.190, 3: 0.175, 4: 0.195,
#: 8: 0.174, 12+: 0.24-0.32 -- and the forms that copy labels to the host every run fell off a cliff at 8 (DESIGN.md
#: section 8).  Three shared streams, filled largest chromosome first, are the measured optimum made explicit: the same
#: schedule whatever the environment says.
SWEEP_STREAMS = 3


class _StreamPool(object):
    """per device: up to SWEEP_STREAMS library-made streams (_lib.stream_create), handed out to the least loaded one; they
    live as long as the process (handles may outlive the cache entry that made them)"""

    def __init__(self):
        self._by_dev = {}
        self._lock = threading.Lock()

    def pick(self, device, n):
        if SWEEP_STREAMS <= 0:
            return None, None
        from . import _lib
        with self._lock:
            slots = self._by_dev.setdefault(device, [])
            if len(slots) < SWEEP_STREAMS:
                try:
                    ptr = _lib.stream_create(device)
                except _lib.CloopsHipError:               # (no such device: the handle's own creation reports it)
                    return None, None
                slots.append([ptr, 0])
            slot = min(slots, key=lambda s: s[1])
            slot[1] += max(1, int(n))
            return slot[0], slot

    @staticmethod
    def release(slot, n):
        if slot is not None:
            slot[1] -= max(1, int(n))


    def rebalance(self, chroms):
        """`chroms` = the idle handles of one sweep [(chromosome made by _make_chrom, n PETs)]: dealt again over their device's
        shared streams, largest first (LPT).  A handle is bound to a stream when it is uploaded -- in arrival order, before anyone
        knows which chromosomes a sweep will take: chr1 .. chrX of a 200 M genome arrive as 72 / 63 / 65 M PETs on the three
        streams, and a step lasts as long as its fullest stream."""
        if SWEEP_STREAMS <= 0:
            return
        by_dev = {}
        for ch, n in chroms:
            slot = getattr(ch.close, "slot", None)
            if slot is not None:
                by_dev.setdefault(ch.device, []).append((ch, max(1, int(n)), slot))
        with self._lock:
            for dev, items in by_dev.items():
                slots = self._by_dev.get(dev, [])
                if len(slots) < 2:
                    continue
                load = {id(s): 0 for s in slots}
                for ch, n, slot in sorted(items, key=lambda t: -t[1]):
                    best = min(slots, key=lambda s: load[id(s)])
                    load[id(best)] += n
                    if best is not slot:
                        ch.set_stream(best[0])
                        slot[1] -= n
                        best[1] += n
                        ch.close.slot = best


STREAMS = _StreamPool()


def _make_chrom(X, Y, device, make=None):
    """a resident chromosome on one of the device's shared streams (its close() also gives the stream's slot back) -> chromosome.
    `make(stream)` builds the handle from arrays that are on the device already (cloops_amd.ingest) instead of uploading X, Y"""
    stream, slot = STREAMS.pick(device, len(X))
    try:
        if make is not None:
            ch = make(stream)
        else:
            ch = api.Chromosome(X, Y, device=device, stream=stream) if stream else api.Chromosome(X, Y, device=device)
    except Exception:
        _StreamPool.release(slot, len(X))
        raise
    close = ch.close

    def close_and_release():
        close()
        _StreamPool.release(close_and_release.slot, len(X))
        close_and_release.slot = None
    close_and_release.slot = slot
    ch.close = close_and_release
    return ch
class _Resident(object):
    """a chromosome resident in HBM + its host copies.  `ids` (the row ids of cLoops/io.py:181-183) and `d` (the distances Y - X the
    reference-shaped wrappers hand out, pipe.py:59-63) are made on FIRST USE: the sweep on the device needs neither, and for a 200 M-PET
    genome they are 3.2 GB of int64 that took as long to fill as the upload itself."""
    __slots__ = ("key", "_ids", "X", "Y", "_d", "chrom", "device", "stamp", "lock", "pins", "sweep_lock", "replaced")

    @property
    def ids(self):
        if self._ids is None:
            self._ids = np.arange(len(self.X), dtype=np.int64)
        return self._ids

    @ids.setter
    def ids(self, v):
        self._ids = v

    @property
    def d(self):
        if self._d is None:
            self._d = self.Y.astype(np.int64) - self.X.astype(np.int64)
        return self._d

    @d.setter
    def d(self, v):
        self._d = v

    def __len__(self):
        return len(self.X)


class ChromCache(object):
    """path -> chromosome resident in HBM (+ host copies of ids and distances).

    `max_items` bounds the number of IDLE residents kept around; a resident that is pinned (a sweep holds it,
    `pinned()`) or whose lock is held is never evicted, so a sweep over any number of chromosomes keeps all of
    its handles alive (the reference has no such limit: it re-reads every .jd in every step)."""

    def __init__(self, max_items=64):
        self._items = OrderedDict()
        self._lock = threading.Lock()
        self.max_items = max_items

    def _evict_idle(self):
        """called with self._lock held: drop the oldest residents that nobody uses while over the limit"""
        if len(self._items) <= self.max_items:
            return []
        out = []
        for f in list(self._items.keys()):
            if len(self._items) - len(out) <= self.max_items:
                break
            r = self._items[f]
            if r.pins > 0 or r.lock.locked():
                continue
            out.append(f)
        return [self._items.pop(f) for f in out]

    def pinned(self, fs, devices=None):
        """context manager: the residents of `fs` (loaded on demand, file k on devices[k % len]; None = wherever it
        already is), pinned against eviction until the block ends"""
        cache = self

        class _Pinned(object):
            def __enter__(self_inner):
                self_inner.rs = []
                try:
                    for k, f in enumerate(fs):
                        dev = None if devices is None else devices[k % len(devices)]
                        self_inner.rs.append(cache.get(f, dev, _pin=True))
                except Exception:
                    self_inner.__exit__(None, None, None)
                    raise
                return self_inner.rs

            def __exit__(self_inner, *exc):
                with cache._lock:
                    for r in self_inner.rs:
                        r.pins -= 1
                    victims = cache._evict_idle()
                    # a resident that was replaced in the cache while a sweep held it is closed by its last user
                    victims += [r for r in self_inner.rs if r.replaced and r.pins == 0]
                    for r in victims:
                        r.replaced = False
                for v in victims:
                    v.chrom.close()
                return False
        return _Pinned()

    def put_arrays(self, name, X, Y, device=0, ids=None, key=None):
        """Register an in-memory chromosome under the pseudo path 'mem://<chrA>-<chrB>' (no .jd
        file, no disk): what a direct BEDPE -> HBM loader hands to the sweep.  `key`: the pair of chromosome names when `name`
        does not spell it (a prefix, a '-' inside a name)."""
        f = "mem://" + name
        r = _Resident()
        r.key = tuple(key) if key is not None else (tuple(name.split("-")) if "-" in name else (name, name))
        r.stamp, r.device = ("mem", len(X)), device
        r.lock = threading.Lock()
        r.sweep_lock = threading.Lock()
        r.replaced = False
        r.pins = 0
        r.X = np.ascontiguousarray(X)
        r.Y = np.ascontiguousarray(Y)
        r.ids = None if ids is None else np.asarray(ids)
        r.d = None
        r.chrom = _make_chrom(r.X, r.Y, device)
        r.chrom.set_device_labels(False)        # runs without a host destination (the sweep) skip the row-order scatter
        with self._lock:
            old = self._items.pop(f, None)
            self._items[f] = r
            if old is not None and old.pins > 0:
                old.replaced, old = True, None            # still held by a sweep: its last user closes it
        if old is not None:
            old.chrom.close()
        return f

    def put_chrom(self, name, chrom, X, Y, ids=None, key=None, device=0):
        """register a chromosome that is ALREADY resident (e.g. api.Chromosome.subsample of another resident) under the
        pseudo path `name` ('mem://...'); X, Y: its host copies (distances, ids for the reference-shaped wrappers)"""
        r = _Resident()
        tail = name[len("mem://"):].split("/")[-1]
        r.key = tuple(key) if key is not None else (tuple(tail.split("-")) if "-" in tail else (tail, tail))
        r.stamp, r.device = ("mem", len(X)), device
        r.lock = threading.Lock()
        r.sweep_lock = threading.Lock()
        r.replaced = False
        r.pins = 0
        r.X = np.ascontiguousarray(X)
        r.Y = np.ascontiguousarray(Y)
        r.ids = None if ids is None else np.asarray(ids)
        r.d = None
        r.chrom = chrom
        r.chrom.set_device_labels(False)
        with self._lock:
            old = self._items.pop(name, None)
            self._items[name] = r
            if old is not None and old.pins > 0:
                old.replaced, old = True, None
        if old is not None:
            old.chrom.close()
        return name

    def drop(self, f):
        """forget one resident (closed at once unless a sweep still holds it)"""
        with self._lock:
            r = self._items.pop(f, None)
            if r is not None and r.pins > 0:
                r.replaced, r = True, None
        if r is not None:
            r.chrom.close()

    def get(self, f, device=None, _pin=False):
        """the resident of `f`; `device=None` takes it wherever it already lives (GPU 0 if it has to be loaded),
        an explicit device reloads a chromosome that lives on another GPU"""
        if f.startswith("mem://"):
            with self._lock:
                r = self._items[f]
                r.pins += 1 if _pin else 0
                return r
        st = os.stat(f)
        stamp = (st.st_mtime_ns, st.st_size)
        with self._lock:
            r = self._items.get(f)
            if r is not None and r.stamp == stamp and (device is None or r.device == device):
                self._items.move_to_end(f)
                r.pins += 1 if _pin else 0
                return r
        device = 0 if device is None else device
        key, mat = parseJd(f, cut=0)
        mat = np.asarray(mat)
        r = _Resident()
        r.key, r.stamp, r.device = key, stamp, device
        r.lock = threading.Lock()
        r.sweep_lock = threading.Lock()
        r.replaced = False
        r.pins = 1 if _pin else 0
        if len(mat):
            r.ids = mat[:, 0]
            r.X = np.ascontiguousarray(mat[:, 1])
            r.Y = np.ascontiguousarray(mat[:, 2])
        else:
            r.ids = r.X = r.Y = np.zeros(0, np.int64)
        r.d = r.Y - r.X
        r.chrom = _make_chrom(r.X, r.Y, device)
        r.chrom.set_device_labels(False)
        with self._lock:
            old = self._items.pop(f, None)
            self._items[f] = r
            victims = self._evict_idle()
            if old is not None and old.pins > 0:
                old.replaced, old = True, None            # still held by a sweep: its last user closes it
        for v in victims:
            v.chrom.close()
        if old is not None:
            old.chrom.close()
        return r

    def clear(self):
        with self._lock:
            for r in self._items.values():
                r.chrom.close()
            self._items.clear()


CACHE = ChromCache()


def _cluster_arrays(res_chrom, eps, minPts, cut, variant=None):
    """One chromosome, one (eps, minPts, cut): the array-level equivalent of pipe.py:57-110.

    Returns (dataI_boxes int64[kI,4], dataS_boxes int64[kS,4], dis float64[], dss float64[],
    n_readI, n_readS, n_in).  Boxes are (minX, maxX, minY, maxY) in ascending cluster id
    (the iteration order of `set(labels.values)`, pipe.py:76-78)."""
    r = res_chrom
    variant = variant or DBSCAN_VARIANT
    d = r.d
    dss_parts = []
    n_in = len(d)
    if cut > 0:                                           # pipe.py:59-63
        short = d < cut
        dss_parts.append(d[short].astype(np.float64))
        n_in = int(len(d) - short.sum())
    empty4 = np.zeros((0, 4), np.int64)
    if n_in == 0:                                         # pipe.py:64-65
        return empty4, empty4, np.zeros(0), (dss_parts[0] if dss_parts else np.zeros(0)), 0, 0, 0
    with r.lock:
        res = r.chrom.cluster(variant, eps, minPts, cut, pinned=True)
        lab = res.labels
        b = res.boxes
        K = len(b)
        cls = np.zeros(K + 1, np.int8)                    # 0 skip, 1 inter, 2 self; slot K for noise
        if K:
            ok = (b["count"] > 0) & (b["min_x"] != b["max_x"]) & (b["min_y"] != b["max_y"])   # pipe.py:83-85
            inter = ok & (b["max_x"] < b["min_y"])                                             # pipe.py:97
            cls[:K][inter] = 1
            cls[:K][ok & ~inter] = 2
        pc = cls[np.where(lab >= 0, lab, K)]
        selI = pc == 1
        selS = pc == 2
        dis = d[selI].astype(np.float64)                  # pipe.py:106-107 (row order)
        dss_parts.append(d[selS].astype(np.float64))      # pipe.py:108-109
    box = np.stack([b["min_x"], b["max_x"], b["min_y"], b["max_y"]], 1).astype(np.int64) if K else empty4
    dataI = box[cls[:K] == 1]
    dataS = box[cls[:K] == 2]
    dss = np.concatenate(dss_parts) if len(dss_parts) > 1 else dss_parts[0]
    return dataI, dataS, dis, dss, int(selI.sum()), int(selS.sum()), n_in


def _records(key, boxes):
    return [[key[0], int(x0), int(x1), key[1], int(y0), int(y1)] for x0, x1, y0, y1 in boxes]


def singleDBSCAN(f, eps, minPts, cut=0, device=None):
    """Run DBSCAN to detect interactions for one chromosome (cLoops/pipe.py:52-110).

    Returns (key, f, dataI, dataS, dis, dss) exactly shaped like the reference: record rows
    [chrA, minX, maxX, chrB, minY, maxY]; dis/dss are lists of float distances."""
    r = CACHE.get(f, device)
    key = r.key
    if cut > 0 and not (r.d >= cut).any() or len(r.d) == 0:
        dss = list(r.d[r.d < cut].astype(np.float64)) if cut > 0 else []
        return key, f, [], [], [], dss
    report = "Clustering %s and %s using eps as %s, minPts as %s,pre-set distance cutoff as > %s\n" % (
        key[0], key[1], eps, minPts, cut)
    sys.stderr.write(report)
    dataI, dataS, dis, dss, nI, nS, _ = _cluster_arrays(r, eps, minPts, cut)
    report = "Clustering %s and %s finished. Estimated %s self-ligation reads and %s inter-ligation reads\n" % (
        key[0], key[1], nS, nI)
    sys.stderr.write(report)
    return key, f, _records(key, dataI), _records(key, dataS), list(dis), list(dss)


def _devices():
    env = os.environ.get("CLOOPS_DEVICES")
    if env:
        return [int(x) for x in env.split(",") if x != ""]
    return list(range(max(1, api.device_count())))


def _run_many(fs, eps, minPts, cut, fn):
    """fn(f, eps, minPts, cut, device) for every file: chromosomes LPT-assigned to the
    visible GPUs, one host thread per GPU; results in `fs` order."""
    devs = _devices()
    if len(devs) <= 1 or len(fs) <= 1:
        return [fn(f, eps, minPts, cut, devs[0]) for f in fs]
    sizes = [len(CACHE.get(f)) if f.startswith("mem://") else os.path.getsize(f) for f in fs]
    parts = lpt_assign(sizes, len(devs))
    out = [None] * len(fs)

    def work(k):
        for i in parts[k]:
            out[i] = fn(fs[i], eps, minPts, cut, devs[k])
    with ThreadPoolExecutor(max_workers=len(devs)) as ex:
        list(ex.map(work, range(len(devs))))
    return out


def runDBSCAN(fs, eps, minPts, cut=0, cpu=1):
    """Run DBSCAN to detect interactions for all chromosomes (cLoops/pipe.py:113-127).
    `cpu` is accepted for signature compatibility; parallelism is over GPUs."""
    ds = _run_many(fs, eps, minPts, cut, singleDBSCAN)
    dataI, dataS, dis, dss = {}, [], [], []
    for d in ds:
        if len(d[2]) == 0:
            continue
        dataI[d[0]] = {"f": d[1], "records": d[2]}
        dataS.extend(d[3])
        dis.extend(d[4])
        dss.extend(d[5])
    return dataI, dataS, dis, dss


def filterClusterByDis(data, cut):
    """Filter inter-ligation clusters by distances (cLoops/pipe.py:130-143): keep a record when the distance
    between its anchor mid-points is >= cut.  The reference is Python 2: `/` on the int mid-points is FLOOR
    division (pipe.py:138).  Mutates and returns `data` like the reference."""
    def mid_distance(rec):
        return (rec[4] + rec[5]) // 2 - (rec[1] + rec[2]) // 2
    for entry in data.values():
        entry["records"] = [rec for rec in entry["records"] if mid_distance(rec) >= cut]
    return data


def checkSameLoop(ra, rb):
    """check if two anchors are exact same (cLoops/pipe.py:146-152)."""
    return (ra[1], ra[2], ra[4], ra[5]) == (rb[1], rb[2], rb[4], rb[5])


def combineTwice(dataI, dataI_2):
    """Combining multiple clustering result (cLoops/pipe.py:155-174): records of `dataI_2` whose exact box is not
    already in `dataI` are appended (the set of known boxes is taken BEFORE appending, so duplicates inside
    `dataI_2` all come through, like the reference)."""
    box = lambda rec: (rec[1], rec[2], rec[4], rec[5])
    for key, new in dataI_2.items():
        have = dataI.get(key)
        if have is None:
            dataI[key] = {"f": new["f"], "records": new["records"]}
            continue
        known = {box(rec) for rec in have["records"]}
        have["records"].extend(rec for rec in new["records"] if box(rec) not in known)
    return dataI


def _single_arrays(f, eps, minPts, cut, device):
    r = CACHE.get(f, device)
    if len(r.d) == 0:
        e4 = np.zeros((0, 4), np.int64)
        return r.key, f, e4, e4, np.zeros(0), np.zeros(0), 0
    dataI, dataS, dis, dss, nI, nS, n_in = _cluster_arrays(r, eps, minPts, cut)
    return r.key, f, dataI, dataS, dis, dss, n_in


def _combine_steps(step_boxes, _hash_bits=None):
    """combineTwice (pipe.py:155-174) applied over all steps at once, on arrays: a box is kept
    in the step where it FIRST appears (duplicates inside one step are all kept, like the
    reference, whose `ds` set is built before the loop).  step_boxes: list of int64[k,4].

    One value sort of `hash << ibits | position` (numpy's SIMD sort, no argsort): equal boxes become
    one run whose first element carries the smallest position, i.e. the first step."""
    step_boxes = [b for b in step_boxes if len(b)]
    if not step_boxes:
        return np.zeros((0, 4), np.int64)
    if len(step_boxes) == 1:
        return step_boxes[0]
    rows = np.concatenate(step_boxes)
    n = len(rows)
    step = np.repeat(np.arange(len(step_boxes), dtype=np.int32), [len(b) for b in step_boxes])
    ibits = max(1, int(n - 1).bit_length())
    u = rows.astype(np.uint64)
    h = (u[:, 0] * np.uint64(0x9E3779B97F4A7C15)) ^ (u[:, 1] * np.uint64(0xC2B2AE3D27D4EB4F)) \
        ^ (u[:, 2] * np.uint64(0x165667B19E3779F9)) ^ (u[:, 3] * np.uint64(0xD6E8FEB86659FD93))
    h ^= h >> np.uint64(29)
    if _hash_bits:                                                        # tests: force hash collisions
        h = (h & np.uint64((1 << _hash_bits) - 1)) << np.uint64(64 - _hash_bits)
    key = ((h >> np.uint64(ibits)) << np.uint64(ibits)) | np.arange(n, dtype=np.uint64)
    key.sort()
    pos = (key & np.uint64((1 << ibits) - 1)).astype(np.int64)          # original positions, grouped by hash
    hs = key >> np.uint64(ibits)
    head = np.empty(n, dtype=bool)
    head[0] = True
    np.not_equal(hs[1:], hs[:-1], out=head[1:])
    first_sorted = np.maximum.accumulate(np.where(head, np.arange(n), 0))    # index (in sorted order) of the run head
    first_pos = pos[first_sorted]                                        # smallest position of the run
    dup = np.flatnonzero(~head)                                          # elements of runs longer than 1
    keep = np.ones(n, dtype=bool)
    if len(dup) == 0:
        return rows
    keep[pos[dup]] = step[pos[dup]] == step[first_pos[dup]]
    # exact check: an element whose row differs from its run head shares only the (truncated) hash with
    # it.  Those few runs are redone exactly; everything else is settled.
    mism = dup[(rows[first_pos[dup]] != rows[pos[dup]]).any(axis=1)]
    if len(mism):
        bad = np.flatnonzero(np.isin(first_sorted, np.unique(first_sorted[mism])))
        bpos = pos[bad]
        _, inv = np.unique(rows[bpos], axis=0, return_inverse=True)
        inv = inv.ravel()
        first_step = np.full(int(inv.max()) + 1, np.iinfo(np.int32).max, np.int32)
        np.minimum.at(first_step, inv, step[bpos])
        keep[bpos] = step[bpos] == first_step[inv]
    return rows[keep]


def _pmap(pool, fn, items):
    """fn over items on the host thread pool (ctypes calls and numpy kernels release the GIL, so the
    per-chromosome waits / small synchronous statistics calls overlap instead of adding up)."""
    if pool is None or len(items) <= 1:
        return [fn(x) for x in items]
    return list(pool.map(fn, items))


def _select_kth(chroms, cut, loghist, ranks, allsum=None, pool=None, fine=None):
    """Exact order statistics (0-based `ranks`, ascending) of the self group's |d| over the union of the chromosomes
    (of all ranks).  `loghist` = the genome-wide log-binned histogram of cl_dist_summary (bins monotone in |d|): it
    locates the bin of a rank; the bin is then refined with 2048-bin histograms of (|d| - lo) >> shift summed over the
    chromosomes (and, with `allsum`, over the ranks) until single distances are resolved -- one refinement pass for
    bins up to 2048 distances wide (|d| < 2^18), two beyond."""
    cum = np.cumsum(np.asarray(loghist, dtype=np.int64))
    out, cache = [], {}
    if fine is not None and fine[0] >= 1:
        # `fine` = (lo, exact histogram of lo <= |d| < lo + 2048), lo a lower bin edge: a rank inside it needs no further pass
        b0 = logbin(fine[0])
        below = int(cum[b0 - 1]) if b0 > 0 else 0
        fcum = np.cumsum(fine[1])
    for rank in ranks:
        if fine is not None and fine[0] >= 1 and below <= rank < below + int(fcum[-1]):
            out.append(fine[0] + int(np.searchsorted(fcum, rank - below, side="right")))
            continue
        b = int(np.searchsorted(cum, rank, side="right"))
        rem = rank - (int(cum[b - 1]) if b > 0 else 0)
        lo, hi = logbin_range(b)
        while hi - lo > 1:
            shift = 0
            while ((hi - lo + (1 << shift) - 1) >> shift) > 2048:
                shift += 1
            key = (lo, hi, shift)
            if key not in cache:
                h = np.zeros(2048, dtype=np.int64)
                for hh in _pmap(pool, lambda r: r.chrom.dist_bin_hist(cut, lo, hi, shift), chroms):
                    h += hh
                cache[key] = allsum(h) if allsum is not None else h
            c = np.cumsum(cache[key])
            k = int(np.searchsorted(c, rem, side="right"))
            rem -= int(c[k - 1]) if k > 0 else 0
            lo, hi = lo + (k << shift), min(hi, lo + ((k + 1) << shift))
        out.append(lo)
    return out


def _step_kde(chroms, cut, n_pos, sumx, sumxx, xshift, pool=None, gridsize=None):
    """The density curves of cPlots.plotIntSelCutFrag for the step whose runs are the last completed ones on `chroms` (K17): per
    chromosome one collect pass, the genome-wide extremes of |d| and Scott's bandwidth from the step's own sums (n_pos, sumx, sumxx
    of log2|d| - xshift, both groups) give each group its grid, the unnormalised sums of all chromosomes are added and normalised
    once.  -> {"grid": float64[2, G], "density": float64[2, G], "n": [n0, n1], "h": [h0, h1]}; a group without a density
    (fewer than two PETs, or equal distances) has NaN rows."""
    from . import plots
    G = int(gridsize or plots.GRIDSIZE)

    def collect(r):
        with r.lock:
            return r.chrom.dist_collect(cut)

    cols = _pmap(pool, collect, chroms)
    grid = np.full((2, G), np.nan)
    dens = np.full((2, G), np.nan)
    ns, hs = [], []
    for g in (0, 1):
        n = int(n_pos[g])
        h = plots.scott_bandwidth(n, sumx[g], sumxx[g], xshift)
        ns.append(n)
        hs.append(float(h))
        live = [(r, c) for r, c in zip(chroms, cols) if c["n_pos"][g] > 0]
        if sum(c["n_pos"][g] for _, c in live) != n:
            raise RuntimeError("distance entries of group %d: %d collected, %d in the step's statistics" % (g, sum(c["n_pos"][g] for _, c in live), n))
        if not plots.drawable(n, h):
            continue
        lo, step = plots.support(min(c["dmin"][g] for _, c in live), max(c["dmax"][g] for _, c in live), h, G)

        def kde(rc):
            with rc[0].lock:
                return rc[0].chrom.dist_kde(g, lo, step, 1.0 / h, G)

        S = np.zeros(G)
        for part in _pmap(pool, kde, live):                   # (file order: the sum does not depend on which finishes first)
            S += part
        grid[g] = plots.grid_points(lo, step, G)
        dens[g] = plots.density(S, n, h)
    return {"grid": grid, "density": dens, "n": ns, "h": hs}


def _plot_step(kde, cut, prefix, log=None):
    """`<prefix>.pdf` from a step's curves (cLoops/pipe.py:261-267)"""
    from . import plots
    curves = [(kde["grid"][g], kde["density"][g], kde["n"][g]) if np.isfinite(kde["density"][g][0]) else None for g in (0, 1)]
    plots.plot_cut_curves(curves, cut, prefix, warn=log)


SWEEP_THREADS = 8
#: enqueue the chromosomes of a sweep step from the pool's threads instead of one after the other from the calling thread.
#: Measured on the 200 M-PET mode-3 sweep: 0.212 s against 0.208 s -- the serial order (largest chromosome first) is worth more
#: than the 2 ms of host time the 23 enqueues take, so it stays off.
PARALLEL_ENQUEUE = False
#: developer hook (tools/step_gap.py): a list -> marks (step, label, t) are appended to it.  Per step: "enqueue" (before the largest
#: chromosome's), "waited" (once per chromosome, as its wait returns), "collected", "reduced", "stats" and, after an estimate, "cut"
STEP_TRACE = None

#: |2**cut - nearest integer| below which runSweepFast re-derives the cut from the distance lists (ests.py:57 truncates) even
#: when the error bound of ests.estIntSelCutFrag_bounded would settle it (a floor under that bound)
CUT_RECHECK_MARGIN = 1e-6


def _trace(step_no, label):
    if STEP_TRACE is not None:
        STEP_TRACE.append((step_no, label, time.perf_counter()))


def _log_no_inter(log, ep, m):
    if log:                                                   # pipe.py:251-255
        log("ERROR: no inter-ligation PETs detected for eps %s minPts %s,can't model the distance cutoff,continue anyway" % (ep, m))


def _final_cut(cuts, max_cut):
    """pipe.py:276-280: the largest or the smallest of the positive cuts of a sweep"""
    pos = [c for c in cuts if c > 0]
    if not pos:
        # np.min([]) raises in the reference; keep that behaviour observable
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    return int(np.max(pos)) if max_cut else int(np.min(pos))


class _StepStats(object):
    """The statistics of one sweep step.  The xshift aside, every field is a sum: over the chromosomes of this rank (`add`), then
    over the ranks (`over_ranks`).  What crosses the ranks is ONE float64 vector, and its layout is stated here and nowhere else in the package
    (bench.py times an all-reduce of its length): the integers, then the floats,

        integers   [0:4]  n_inter, n_self, n_in, n_chroms
                   [4:6]  n_all (inter, self)      [6:8]  n_pos (inter, self)
                   [8 : 8 + DIST_LOGBINS]  loghist      then FINE_BINS words: fine
        floats     [0:2]  sumx      [2:4]  sumxx      [4]  xshift      [5]  1 on a rank that reports an xshift, else 0

    n_inter / n_self: inter- and self-ligation boxes; n_in: PETs that entered DBSCAN; n_chroms: chromosomes with an inter-ligation
    box.  Only those chromosomes count from n_all on (runDBSCAN skips the others entirely, pipe.py:121-122): n_all / n_pos / sumx /
    sumxx per group (x = log2|d| - xshift) and the self group's loghist / fine as cl_dist_summary makes them."""
    FINE_BINS = 2048
    __slots__ = ("n_inter", "n_self", "n_in", "n_chroms", "n_all", "n_pos", "loghist", "fine", "sumx", "sumxx", "xshift")

    def __init__(self):
        self.n_inter = self.n_self = self.n_in = self.n_chroms = 0
        self.n_all, self.n_pos, self.sumx, self.sumxx = [0, 0], [0, 0], [0.0, 0.0], [0.0, 0.0]
        self.loghist = np.zeros(DIST_LOGBINS, dtype=np.int64)
        self.fine = np.zeros(self.FINE_BINS, dtype=np.int64)
        self.xshift = 0.0

    def add(self, n_inter, n_self, n_in, s):
        """one chromosome's step_result() and last_n_in() -> whether the chromosome counts (it has an inter-ligation box)"""
        self.n_self += n_self
        self.n_in += n_in
        if n_inter == 0:
            return False
        self.n_inter += n_inter
        self.n_chroms += 1
        for g in (0, 1):
            self.n_all[g] += s["n_all"][g]
            self.n_pos[g] += s["n_pos"][g]
            self.sumx[g] += s["sumx"][g]
            self.sumxx[g] += s["sumxx"][g]
        self.loghist += s["loghist"]                          # (integer histograms: exact in any order)
        if s.get("fine") is not None:
            self.fine += s["fine"]
        self.xshift = s["xshift"]
        return True

    def pack(self):
        """-> (integers int64, floats float64) in the layout above"""
        ints = np.concatenate([np.asarray([self.n_inter, self.n_self, self.n_in, self.n_chroms] + self.n_all + self.n_pos, dtype=np.int64),
                               self.loghist, self.fine])
        return ints, np.asarray(self.sumx + self.sumxx + [self.xshift, 1.0 if self.n_chroms else 0.0], dtype=np.float64)

    @classmethod
    def unpack(cls, ints, floats):
        """the record of packed (and summed) vectors; its histograms and float sums are views of them"""
        t = cls.__new__(cls)
        t.n_inter, t.n_self, t.n_in, t.n_chroms = (int(v) for v in ints[:4])
        t.n_all, t.n_pos = [int(ints[4]), int(ints[5])], [int(ints[6]), int(ints[7])]
        t.loghist, t.fine = ints[8:8 + DIST_LOGBINS], ints[8 + DIST_LOGBINS:]
        t.sumx, t.sumxx = floats[0:2], floats[2:4]
        # xshift is a constant of the library, the same on every rank that has one: the sum over the ranks divided by the number
        # of ranks that reported (a rank without a counted chromosome reports 0 and counts as 0)
        t.xshift = float(floats[4]) / max(float(floats[5]), 1.0)
        return t

    def over_ranks(self, allsum, step_no):
        """-> the genome-wide record: with `allsum` ONE exchange, the counts riding as float64 next to the sums (every count and
        every sum of counts stays far below 2^53, so they come back exact); without it this rank's record is the genome's and
        nothing is packed, exchanged or converted"""
        if allsum is None:
            _trace(step_no, "reduced")
            return self
        ints, floats = self.pack()
        _trace(step_no, "reduced")
        both = allsum(np.concatenate([ints.astype(np.float64), floats]))
        return self.unpack(np.rint(both[:len(ints)]).astype(np.int64), both[len(ints):])


class _DataI(dict):
    """runSweepFast's candidate tables; `.gathered` = what `device_consumer` returned"""
    gathered = None


#: one (eps, minPts) step of a sweep: its number, the cut it filters with and where its summary counts distances exactly
_Step = namedtuple("_Step", "no eps minPts cut fine_lo")


@contextlib.contextmanager
def _sweep_hold(fs, res_all, eps, minPts):
    """One sweep's hold on its handles -> live = [(f, resident)] of the non-empty chromosomes, in file order.  The candidate
    buffer, the layout and the sort index of a handle are state of ONE sweep: a second sweep over the same residents waits (locks
    taken in one global order, so two sweeps over overlapping sets cannot deadlock)."""
    live = [(f, r) for f, r in zip(fs, res_all) if len(r)]
    held = sorted({id(r): r for _, r in live}.values(), key=id)
    for r in held:
        r.sweep_lock.acquire()
    try:
        # (a synchronous call on a handle -- cluster(), sig_counts() -- holds its r.lock: no stream is swapped under one)
        for r in held:
            r.lock.acquire()
        try:
            STREAMS.rebalance([(r.chrom, len(r)) for _, r in live])
        finally:
            for r in held:
                r.lock.release()
        for f, r in live:
            r.chrom.cand_reset()
            # the region query of the first run at an eps serves the later runs at that eps (their minPts are smaller: the
            # reference sorts them descending, pipe.py:316-320) -- its counts have to tell `count >= m` for every m of the list
            # (cl_sweep_plan: with several eps the q index pays from the first sort on and, if the values share a divisor, one fine
            #  sort serves all of them; the counts of an eps are bracketed for the whole minPts list)
            r.chrom.sweep_plan(eps, minPts)
        yield live
    finally:
        for f, r in live:
            # the announced minPts list belongs to this sweep: a later one-off run on the handle serves its own minPts only
            try:
                r.chrom.sweep_plan([], [])
            except Exception:
                pass
        for r in held:
            r.sweep_lock.release()


def _enqueue_step(step, by_size, variant, pool):
    """The step's run of every chromosome enqueued, in the order of `by_size` (largest first).  Chromosomes are independent inside
    a step and the handles share the device's streams: the kernels of different chromosomes overlap on the GPU.  A handle's r.lock
    is held from here until _collect_step has taken its result."""
    def enqueue(fr):
        f, r = fr
        if fr is by_size[0]:
            _trace(step.no, "enqueue")
        r.lock.acquire()
        try:
            r.chrom.step_async(variant, step.eps, step.minPts, step.cut, step.no, step.fine_lo)
        except Exception as e:
            r.lock.release()
            return e
        return None

    errs = _pmap(pool if PARALLEL_ENQUEUE else None, enqueue, by_size)
    if any(e is not None for e in errs):
        # a failed enqueue must not leave the other chromosomes locked with a run in flight
        for (f, r), e in zip(by_size, errs):
            if e is None:
                try:
                    r.chrom.wait()
                except Exception:
                    pass
                r.lock.release()
        raise [e for e in errs if e is not None][0]


def _collect_step(step, live, pool, probe, appended):
    """The step's results summed over this rank's chromosomes -> (_StepStats, the residents that count: those with an inter-ligation
    box); `appended` (f -> inter-ligation boxes appended on the device so far) grows by them.  A run carries its own tail on the
    device: the table classified (pipe.py:83-97), its inter-ligation boxes appended to the chromosome's candidate buffer under this
    step's number, the distance statistics reduced -- everything is on the host with the run's completion."""
    def collect(fr):
        f, r = fr
        try:
            res = r.chrom.wait()
            _trace(step.no, "waited")
            if probe is not None:
                probe(f, step.eps, step.minPts, step.cut, res)
            n_inter, n_self, s = r.chrom.step_result()
            n_in = r.chrom.last_n_in()
        finally:
            r.lock.release()
        return f, r, n_inter, n_self, n_in, s

    tot, used = _StepStats(), []
    # (results are taken in file order AS THEY ARRIVE: the sums of the chromosomes that finished early are done while the others
    #  still run, behind the step's last wait only that chromosome's share is left.  Not pool.map: when one result raises, its
    #  iterator cancels the calls that have not started, and their chromosomes would stay locked with a run in flight)
    futs = [] if pool is None else [pool.submit(collect, fr) for fr in live][::-1]        # (popped from the end: a result is let go once summed)
    for f, r, n_inter, n_self, n_in, s in (map(collect, live) if pool is None else (futs.pop().result() for _ in live)):
        if tot.add(n_inter, n_self, n_in, s):
            appended[f] = appended.get(f, 0) + n_inter
            used.append(r)
    _trace(step.no, "collected")
    return tot, used


def _estimate_cut(step, tot, used, st, variant, allsum, pool, plot, log):
    """pipe.py:251-267 on the genome-wide statistics `tot` of a step (`used`: this rank's chromosomes that count in them) ->
    (cut_2, frags, fine_lo of the next step), or None where the reference estimates nothing: no inter-ligation PETs anywhere, or
    one of the two distance groups is empty.  Notes on how the cut was settled, and the curves of a plot, go into `st`."""
    if tot.n_chroms == 0:
        _log_no_inter(log, step.eps, step.minPts)
        return None
    if not (tot.n_all[0] > 0 and tot.n_all[1] > 0):           # pipe.py:256-259
        return None
    if tot.n_pos[0] == 0 or tot.n_pos[1] == 0:
        raise ValueError("cannot convert float NaN to integer")      # what int(2 ** nan) raises in ests.py:57
    n1 = tot.n_pos[1]
    med = _select_kth(used, step.cut, tot.loghist, sorted({(n1 - 1) // 2, n1 // 2}), allsum, pool,
                      fine=(step.fine_lo, tot.fine) if step.fine_lo >= 1 else None)
    # the next step's summary also counts the distances around this median exactly (the median moves little from step to step):
    # lower edge of the log bin 1024 below it, so that the ranks below it are known
    fine_lo = logbin_range(logbin(max(1, med[0] - 1024)))[0]
    # the cut from sum x and sum x^2 (x = log2|d| - xshift), with the range that the reduction's rounding leaves for the
    # reference's int(2 ** cut) (ests.estIntSelCutFrag_bounded)
    cut_2, frags, (rc_lo, rc_hi), margin = estIntSelCutFrag_bounded(tot.n_all, tot.n_pos, tot.sumx, tot.sumxx, tot.xshift,
                                                                    (med[0], med[-1]), n_parts=tot.n_chroms)
    if rc_lo != rc_hi or margin < CUT_RECHECK_MARGIN:
        if allsum is None:
            # 2**cut may sit on either side of an integer within the error of the statistics: settle it the reference's way, from
            # the distance lists with numpy's own sums (rare -- a group of (nearly) equal distances, or 2**cut within ~1e-6 of an
            # integer; one extra run per chromosome with labels on the host)
            parts = [_cluster_arrays(r, step.eps, step.minPts, step.cut, variant) for r in used]
            cut_2, frags = estIntSelCutFrag(np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts]))
            st["cut_rechecked"] = True
        else:
            # several ranks: the lists are spread over them -- keep the statistics' cut, inside the bound
            st["cut_range"] = (int(rc_lo), int(rc_hi))
            if log and rc_lo != rc_hi:
                log("WARNING: the distance statistics of eps=%s,minPts=%s bound the cutoff only to [%s, %s]" % (step.eps, step.minPts, rc_lo, rc_hi))
    if plot is not None:
        # pipe.py:261-267: the picture of this step's two distance groups with the estimated cut drawn in; the handles still hold
        # the step's runs (a re-check above repeated them with the same parameters)
        t_plot0 = time.perf_counter()
        st["kde"] = _step_kde(used, step.cut, tot.n_pos, tot.sumx, tot.sumxx, tot.xshift, pool)
        _plot_step(st["kde"], cut_2, "%s_eps%s_minPts%s_disCutoff" % (plot, step.eps, step.minPts), log)
        st["plot_s"] = time.perf_counter() - t_plot0
    if log:
        log("Estimated inter-ligation and self-ligation distance cutoff as %s for eps=%s,minPts=%s" % (cut_2, step.eps, step.minPts))
    return cut_2, frags, fine_lo


def _finish_sweep(live, appended, final_cut, pool, finish_device, device_consumer):
    """combineTwice over all steps (pipe.py:257,275), then filterClusterByDis (pipe.py:130-143, floor division): on the device, per
    chromosome; only the surviving boxes cross PCIe -> _DataI"""
    def finish(fr):
        f, r = fr
        with r.lock:
            if finish_device:
                ptr, k = r.chrom.cand_finish_device(final_cut)
                return r.key, {"f": f, "boxes": None, "dev_rows": ptr, "n_rows": k}
            b = r.chrom.cand_finish(final_cut, appended[f])
        return r.key, {"f": f, "boxes": b}                    # int32 [k, 4] rows (minX, maxX, minY, maxY), append order

    # key order = first appearance over the steps, file order inside a step: what combineTwice's dict inserts
    # (pipe.py:155-174) and runStat later walks -- `appended` was filled in exactly that order
    res_of = dict(live)
    dataI = _DataI(_pmap(pool, finish, [(f, res_of[f]) for f in appended]))
    if finish_device and device_consumer is not None:
        dataI.gathered = device_consumer(dataI)               # (residents pinned, sweep locks held: the pointers are alive)
    return dataI


def runSweepFast(fs, eps, minPts, cut=0, max_cut=False, log=None, variant=None, allsum=None, probe=None, forced_cuts=None, finish_device=False,
                 device_consumer=None, plot=None):
    """runSweep with the per-step statistics reduced on the GPUs: neither labels nor distance
    lists come back to the host -- per chromosome only the K-row cluster table, a few sums, and
    the 256-bin histograms of an exact radix select for the median (all additive over chromosomes
    and over GPUs).  Same chain, same cuts, same candidate boxes as runSweep / the reference's
    pipe.py:241-281; candidate boxes stay numpy arrays:

    `allsum` (optional): element-wise global sum of a small numpy array over all ranks
    (cloops_amd.dist.make_allsum) -- with it every rank passes ITS chromosomes as `fs` and the
    chained cut is estimated from the genome-wide statistics; the per-step exchange is one
    vector (_StepStats) and, where the median needs them, the histograms of its refinement.

    `probe` (optional): called as probe(f, eps, minPts, cut_in, result) for every completed run (bench.py reads
    the HIP-event kernel timings of profiled handles through it).

    `forced_cuts` (optional): one cut per step that REPLACES the cut estimated by that step (every step still does all
    of its work, the estimate included) -- bench.py replays the genome-wide chain on one emulated rank's share of the
    chromosomes with it.

    `finish_device`: the candidate tables stay on the device ({"f": f, "dev_rows": pointer, "n_rows": k, "boxes": None} per
    chromosome, valid until the handle's next sweep finishes): a multi-rank run hands them to comm.Comm.gather_device, which sends
    exact sizes to the merging rank without a detour through the host (cLoops/pipe.py:119-127 merges in the parent).

    `device_consumer` (with finish_device): called as device_consumer(dataI) WHILE the residents are still pinned in the cache and
    the sweep locks are held -- the device pointers cannot be evicted, freed or overwritten by another sweep before it returns; what
    it returns is `dataI.gathered` (bench.py: the RCCL gather of the tables to the merging rank).  Without a consumer the caller
    must use the pointers before anything else touches these handles.

    `plot` (optional): a file prefix switches the distance-cutoff pictures of cLoops/pipe.py:261-267 on: every step that estimates
    a cut also gets st["kde"] = {"grid", "density": float64[2, G], "n", "h"} -- the Gaussian kernel densities of log2|d| of its
    inter- and self-ligation PETs, summed on the GPUs (K17, cloops_amd.plots) -- st["plot_s"], the wall time of that, and the file
    `<plot>_eps<ep>_minPts<m>_disCutoff.pdf`.  Nothing is re-clustered for it and the steps, cuts and candidates do not change;
    with None (the default) not one extra call is made.  Not with `allsum`: the extremes of |d| are no sums (ValueError).

    returns (dataI {key: {"f": f, "boxes": int32[k,4]}} of the local chromosomes, cut, cuts, steps)."""
    variant = variant or DBSCAN_VARIANT
    if plot is not None and allsum is not None:
        raise ValueError("runSweepFast: plot needs the whole genome on one rank (it cannot be combined with allsum)")
    cuts, steps = [cut], []
    appended = {}                                             # f -> inter-ligation boxes appended on the device so far
    # where a step's summary should look for the median (see _select_kth).  The first step has no earlier median to go by: it
    # counts the distances 1 .. 2048 exactly (self-ligation distances are a few hundred bp: ests.py's cut model) and falls back
    # to the refinement passes if the median lies beyond
    fine_lo = 1
    with CACHE.pinned(fs, _devices()) as res_all, _sweep_hold(fs, res_all, eps, minPts) as live, \
            (ThreadPoolExecutor(max_workers=SWEEP_THREADS) if len(live) > 1 else contextlib.nullcontext()) as pool:
        by_size = sorted(live, key=lambda fr: -len(fr[1]))    # enqueue order: largest first (results are collected in file order)
        for ep, m in itertools.product(eps, minPts):
            step = _Step(len(steps), ep, m, cut, fine_lo)
            t_step0 = time.perf_counter()
            # one roctx range per step, from the enqueue to this rank's statistics on the host (rocprofv3 --marker-trace); wall_s
            # covers the same: enqueue .. statistics of this rank on the host (+ the exchange); the cut follows
            with _roctx.range_("cloops sweep step %d: eps %d minPts %d cut %d" % (step.no, ep, m, cut)):
                _enqueue_step(step, by_size, variant, pool)
                local, used = _collect_step(step, live, pool, probe, appended)
                tot = local.over_ranks(allsum, step.no)
                st = {"eps": ep, "minPts": m, "cut_in": int(cut), "n_inter": tot.n_inter, "n_self": tot.n_self, "n_in": tot.n_in,
                      "wall_s": time.perf_counter() - t_step0}
            steps.append(st)
            _trace(step.no, "stats")
            est = _estimate_cut(step, tot, used, st, variant, allsum, pool, plot, log)
            # a forced cut replaces what the step estimated -- or did not estimate -- as the cut it hands on
            forced = forced_cuts[step.no] if forced_cuts is not None else None
            if est is not None or forced is not None:
                cut = int(forced) if forced is not None else est[0]         # pipe.py:274
                st["cut_out"] = int(cut)
                cuts.append(cut)
            if est is not None:
                st["frags"] = int(est[1])
                fine_lo = est[2]
                _trace(step.no, "cut")
        cut = _final_cut(cuts, max_cut)
        dataI = _finish_sweep(live, appended, cut, pool, finish_device, device_consumer)
    return dataI, cut, cuts, steps


def runSweep(fs, eps, minPts, cut=0, cpu=1, max_cut=False, log=None):
    """The (eps, minPts) sweep of cLoops/pipe.py:241-281 with its chained distance cutoff:
    the cut estimated from step k (`cut = cut_2`, pipe.py:274) pre-filters step k+1.

    eps: list ascending, minPts: list descending (the order `main` establishes,
    pipe.py:310-324).  Returns (dataI, cut, cuts, steps): dataI after `combineTwice` and
    `filterClusterByDis`, the final cut (min or max of the positive cuts, pipe.py:276-280),
    every cut seen, and one dict per executed step."""
    dataI = {}
    cuts = [cut]
    steps = []
    for ep in eps:
        for m in minPts:
            rs = _run_many(fs, ep, m, cut, _single_arrays)
            dataI_2, dis_2, dss_2, nS, n_in = {}, [], [], 0, 0
            for key, f, dI, dS, dis, dss, nin in rs:     # runDBSCAN merge, pipe.py:119-127
                n_in += nin
                if len(dI) == 0:
                    continue
                dataI_2[key] = {"f": f, "records": _records(key, dI)}
                nS += len(dS)
                dis_2.append(dis)
                dss_2.append(dss)
            st = {"eps": ep, "minPts": m, "cut_in": int(cut), "n_inter": sum(len(v["records"]) for v in dataI_2.values()),
                  "n_self": nS, "n_in": n_in}
            steps.append(st)
            if len(dataI_2) == 0:
                _log_no_inter(log, ep, m)
                continue
            dis_2 = np.concatenate(dis_2) if dis_2 else np.zeros(0)
            dss_2 = np.concatenate(dss_2) if dss_2 else np.zeros(0)
            if len(dis_2) == 0 or len(dss_2) == 0:       # pipe.py:256-257
                dataI = combineTwice(dataI, dataI_2)
            else:
                cut_2, frags = estIntSelCutFrag(dis_2, dss_2)
                if log:
                    log("Estimated inter-ligation and self-ligation distance cutoff as %s for eps=%s,minPts=%s" % (cut_2, ep, m))
                st["cut_out"] = int(cut_2)
                st["frags"] = int(frags)
                cuts.append(cut_2)
                cut = cut_2                               # pipe.py:274
                dataI = combineTwice(dataI, dataI_2)
    cut = _final_cut(cuts, max_cut)
    dataI = filterClusterByDis(dataI, cut)
    return dataI, cut, cuts, steps


# ---------------------------------------------------------------------------------------
# the whole flow of cLoops/pipe.py:206-295
# ---------------------------------------------------------------------------------------
MODES = {1: ([500, 1000, 2000], [5], 0), 2: ([1000, 2000, 5000], [5], 0),
         3: ([5000, 7500, 10000], [50, 40, 30, 20], 1), 4: ([2500, 5000, 7500, 10000], [30, 20], 1)}   # pipe.py:329-344


_PIPE_RUNS = itertools.count()


def _read_gpu(fs, fout, chroms, cut, auto_eps, tmp, fmt="bedpe", ext=50):
    """the input through the GPU reader (cloops_amd.ingest.load_bedpe, for 4DN pairs cloops_amd.pairs.load_pairs): -> ('mem://'
    names, distances or None); with `tmp` the `.jd` files of the host reader are written from the host copies"""
    from . import ingest
    ds = [] if auto_eps else None
    prefix = "pipe-%d-%d" % (os.getpid(), next(_PIPE_RUNS))
    if fmt == "pairs":
        from . import pairs
        cfs = pairs.load_pairs(fs, chroms, cut, unique=auto_eps, strand_distances=ds, ext=ext, prefix=prefix)
    else:
        cfs = ingest.load_bedpe(fs, chroms, cut, unique=auto_eps, strand_distances=ds, prefix=prefix)
    if tmp:
        import joblib
        try:
            for f in cfs:
                r = CACHE.get(f)
                joblib.dump(ingest.rows_matrix(r.X, r.Y), os.path.join(fout, "%s-%s.jd" % r.key))
        except BaseException:
            for f in cfs:
                CACHE.drop(f)
            raise
    return cfs, ds


def pipe(fs, fout, eps, minPts, chroms="", cpu=1, tmp=0, hic=0, washU=0, juice=0, cut=0, plot=0, max_cut=False,
         log=None, reader="gpu", fmt="auto", ext=50, agg=0, agg_res=0, bdg=0, bdg_ext=75, peaks=0, peak_eps=(100, 200),
         peak_minPts=(5, 10), domains=0, dom_res=10000, dom_w=(10,), kdis=0, kdis_k=(4, 9, 19), mat=0, mat_res=10000):
    """cLoops/pipe.py:206-295: BEDPE -> per-chromosome PETs -> (eps, minPts) sweep with the chained
    distance cutoff on the GPU(s) -> candidate loops -> significance -> `<fout>.loop`.

    `plot` writes `<fout>_eps<ep>_minPts<m>_disCutoff.pdf` for every step that estimates a cut (pipe.py:261-267; the densities
    are summed on the GPU and are those of seaborn under Python 3, cloops_amd.plots / INTEGRATION.md).  `washU` /
    `juice` write `<fout>_loops_washU.txt` / `<fout>_loops_juicebox.txt` after `<fout>.loop` (pipe.py:288-292, cloops_amd.tracks).
    `eps == 0` estimates eps from the distances of the PETs mapped to different strands (io.py:62-129, ests.py:23-33).
    `reader`: "gpu" reads the BEDPE files on the device (K16, cloops_amd.ingest): the chromosomes go from the text to HBM
    without `.jd` files, which are written only with `tmp`; "host" is cloops_amd.io's Python loop and its `.jd` files.
    `fmt`: "bedpe", "pairs" (4DN pairs read with the extension `ext`, K18, cloops_amd.pairs) or "auto": pairs exactly when the
    first file's first line starts with `## pairs format`.
    `agg` writes `<fout>_agg.txt`, `<fout>_agg_loops.txt` and `<fout>_agg.json` after `<fout>.loop`: the aggregate pile-up of the PETs
    around the significant loops just called (K19, cloops_amd.agg), from the chromosomes still resident, in bins of `agg_res` bp
    (0: the largest eps of the run).
    `bdg` writes `<fout>.bedGraph` and `<fout>_bedGraph.json` after `<fout>.loop`: the coverage of the genome by both ends of every PET
    (raw depth, cut 0, K20, cloops_amd.coverage), from the chromosomes still resident, each end standing for `bdg_ext` bp to either side.
    `peaks` writes `<fout>_peaks.txt`, `<fout>_peaks.bed` and `<fout>_peaks.json` after `<fout>.loop`: the peaks of both ends of every PET
    (cut 0, K21, cloops_amd.peaks) for every (eps, minPts) of `peak_eps` x `peak_minPts`, from the chromosomes still resident.
    `domains` writes `<fout>_domains.txt`, `<fout>_domains.bed`, `<fout>_boundaries.txt`, `<fout>_insulation_w<W>.bedGraph` and
    `<fout>_domains.json` after `<fout>.loop`: the domains of every chromosome (cut 0, K22, cloops_amd.domains) in bins of `dom_res` bp
    for every window of `dom_w`, from the chromosomes still resident.
    `kdis` writes `<fout>_kdis.txt` and `<fout>_kdis.json` after `<fout>.loop`: the k-distance curves of the PETs and the eps they
    suggest (cut 0, K23, cloops_amd.esteps) for every k = minPts - 1 of `kdis_k`, from the chromosomes still resident.  The suggestion
    is reported, not fed into the sweep.
    `mat` writes `<fout>_cells.txt` (bg2: `chrom start1 end1 chrom start2 end2 count`) and `<fout>_cells.json` after `<fout>.loop`: the
    non-empty cells of every chromosome's contact matrix in bins of `mat_res` bp (folded onto the upper triangle, cut 0, K24,
    cloops_amd.matrix), from the chromosomes still resident."""
    import shutil
    if reader not in ("gpu", "host"):
        raise ValueError("reader must be 'gpu' or 'host', got %r" % (reader,))
    if fmt not in ("auto", "bedpe", "pairs"):
        raise ValueError("fmt must be 'auto', 'bedpe' or 'pairs', got %r" % (fmt,))
    if fmt == "auto":
        from . import pairs
        fmt = pairs.sniff(fs[0]) if fs else "bedpe"
    from . import io as cio
    from . import cModel
    if chroms == "":
        chroms = []
    else:
        chroms = set(chroms.split(","))
    if os.path.isdir(fout):                                   # pipe.py:225-228
        if log:
            log("working directory %s exists, return." % fout)
        return
    os.mkdir(fout)
    auto_eps = eps == 0 or eps == [0]                         # pipe.py:231-239: eps from the data
    mem = []
    try:
        if reader == "gpu":
            cfs, ds = _read_gpu(fs, fout, chroms, cut, auto_eps, tmp, fmt, ext)
            mem = cfs
        elif fmt == "pairs":
            from . import pairs
            if auto_eps:
                cfs, ds = pairs.parseRawPairs(fs, fout, chroms, cut, ext=ext, reader="host")
            else:
                cfs = pairs.parseRawPairs2(fs, fout, chroms, cut, ext=ext, reader="host")
        elif auto_eps:
            cfs, ds = cio.parseRawBedpe(fs, fout, chroms, cut)
            cfs = [cio.txt2jd(f) for f in cfs]
        else:
            cfs = [cio.txt2jd(f) for f in cio.parseRawBedpe2(fs, fout, chroms, cut)]
        if auto_eps:
            from .ests import estFragSize
            eps = [estFragSize(ds) * 2]
        dataI, cut, cuts, steps = runSweepFast(cfs, eps, minPts, cut=cut, max_cut=max_cut, log=log, plot=fout if plot else None)
        records = {key: {"f": v["f"], "records": _records(key, v["boxes"])} for key, v in dataI.items()}
        e = cModel.runStat(records, minPts, 0, cpu, fout, hic)    # pipe.py:284 passes cut = 0
        if agg and not e:
            from .agg import aggLoops
            aggLoops(fout + ".loop", list(cfs), fout, res=int(agg_res) if agg_res else int(max(eps)))
        if bdg and not e:
            from .coverage import jd2bedgraph
            jd2bedgraph(list(cfs), fout, ext=int(bdg_ext))
        if peaks and not e:
            from .peaks import jd2peaks
            jd2peaks(list(cfs), fout, eps=peak_eps, minPts=peak_minPts)
        if domains and not e:
            from .domains import jd2domains
            jd2domains(list(cfs), fout, res=int(dom_res), w=dom_w)
        if kdis and not e:
            from .esteps import jd2esteps
            jd2esteps(list(cfs), fout, ks=kdis_k)
        if mat and not e:
            from .matrix import jd2cells
            jd2cells(list(cfs), fout, res=int(mat_res))
    finally:
        for f in mem:                                         # 'mem://' residents are never evicted by age
            CACHE.drop(f)
    if e:
        shutil.rmtree(fout)
        return
    if washU:                                                 # pipe.py:288-292
        from .tracks import loops2washU
        loops2washU(fout + ".loop", fout + "_loops_washU.txt")
    if juice:
        from .tracks import loops2juice
        loops2juice(fout + ".loop", fout + "_loops_juicebox.txt")
    if tmp == False:                                          # noqa: E712  (pipe.py:294)
        shutil.rmtree(fout)
    return steps


def main(argv=None):
    """`python -m cloops_amd -f a.bedpe.gz -o out -m 1` -- the flags of cLoops/utils.py:73-204 that
    drive the hot path (same names; -w / -j write the loop tracks, -plot the distance-cutoff picture of every sweep step, -agg the
    aggregate pile-up around the called loops in bins of -res bp, -bdg the coverage of the PET ends as a bedGraph with -bdgext bp
    to either side of an end, -peaks the peaks of the PET ends for every setting of -peakeps x -peakminPts, -domains the domains and
    boundaries in bins of -domres bp for every window of -domw bins, -kdis the k-distance curves of the PETs and the eps they suggest for
    every k = minPts - 1 of -kdisk, -mat the non-empty cells of the contact matrices in bins of -matres bp)."""
    import argparse
    ap = argparse.ArgumentParser(prog="cloops_amd")
    ap.add_argument("-f", dest="fnIn", required=True)
    ap.add_argument("-o", dest="fnOut", required=True)
    ap.add_argument("-m", dest="mode", type=int, default=0, choices=[0, 1, 2, 3, 4])
    ap.add_argument("-eps", dest="eps", default="0")
    ap.add_argument("-minPts", dest="minPts", default="0")
    ap.add_argument("-p", dest="cpu", type=int, default=1)
    ap.add_argument("-c", dest="chroms", default="")
    ap.add_argument("-w", dest="washU", action="store_true")
    ap.add_argument("-j", dest="juice", action="store_true")
    ap.add_argument("-s", dest="tmp", action="store_true")
    ap.add_argument("-hic", dest="hic", action="store_true")
    ap.add_argument("-cut", dest="cut", type=int, default=0)
    ap.add_argument("-plot", dest="plot", action="store_true")
    ap.add_argument("-max_cut", dest="max_cut", action="store_true")
    ap.add_argument("-reader", dest="reader", default="gpu", choices=["host", "gpu"])
    ap.add_argument("-fmt", dest="fmt", default="auto", choices=["auto", "bedpe", "pairs"])
    ap.add_argument("-ext", dest="ext", type=int, default=50)
    ap.add_argument("-agg", dest="agg", action="store_true")
    ap.add_argument("-res", dest="res", type=int, default=0)
    ap.add_argument("-bdg", dest="bdg", action="store_true")
    ap.add_argument("-bdgext", dest="bdgext", type=int, default=75)
    ap.add_argument("-peaks", dest="peaks", action="store_true")
    ap.add_argument("-peakeps", dest="peakeps", default="100,200")
    ap.add_argument("-peakminPts", dest="peakminPts", default="5,10")
    ap.add_argument("-domains", dest="domains", action="store_true")
    ap.add_argument("-domres", dest="domres", type=int, default=10000)
    ap.add_argument("-domw", dest="domw", default="10")
    ap.add_argument("-kdis", dest="kdis", action="store_true")
    ap.add_argument("-kdisk", dest="kdisk", default="4,9,19")
    ap.add_argument("-mat", dest="mat", action="store_true")
    ap.add_argument("-matres", dest="matres", type=int, default=10000)
    op = ap.parse_args(argv)
    if op.mode == 0:                                          # pipe.py:306-327
        eps = sorted(int(x) for x in str(op.eps).split(","))
        minPts = sorted((int(x) for x in str(op.minPts).split(",")), reverse=True)
        if minPts == [0]:
            sys.stderr.write("minPts not assigned!\n")
            return 1
        hic = int(op.hic)
    else:
        eps, minPts, hic = MODES[op.mode]
    sys.stderr.write("mode:%s\t eps:%s\t minPts:%s\t hic:%s\t\n" % (op.mode, eps, minPts, hic))
    pipe(op.fnIn.split(","), op.fnOut, eps, minPts, op.chroms, op.cpu, op.tmp, hic, op.washU, op.juice, op.cut,
         op.plot, op.max_cut, log=lambda m: sys.stderr.write(m + "\n"), reader=op.reader, fmt=op.fmt, ext=op.ext,
         agg=op.agg, agg_res=op.res, bdg=op.bdg, bdg_ext=op.bdgext, peaks=op.peaks, peak_eps=op.peakeps,
         peak_minPts=op.peakminPts, domains=op.domains, dom_res=op.domres, dom_w=op.domw, kdis=op.kdis, kdis_k=op.kdisk,
         mat=op.mat, mat_res=op.matres)
    return 0
