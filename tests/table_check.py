"""The one reference for the cluster table {min_x, max_x, min_y, max_y, count} per id (cLoops/pipe.py:78-102): numpy on labels, exact
integer equality, every row.  Used by every GPU test that clusters and has labels to compare with (no GPU needed here)."""
import numpy as np

from cloops_amd import api

FIELDS = ("count", "min_x", "max_x", "min_y", "max_y")


def table_from_labels(X, Y, labels, K):
    """count, min and max per id 0 .. K - 1 of the rows with labels >= 0, by one sort and reduceat -> api.BOX_DTYPE[K].  An id
    without members has count 0 and all-zero coordinates, as k_export_table writes it."""
    X = np.asarray(X, np.int64)
    Y = np.asarray(Y, np.int64)
    labels = np.asarray(labels)
    out = np.zeros(max(int(K), 0), api.BOX_DTYPE)
    sel = np.flatnonzero(labels >= 0)
    if len(sel) == 0:
        return out
    order = sel[np.argsort(labels[sel], kind="stable")]
    ls = labels[order]
    starts = np.flatnonzero(np.concatenate([[True], ls[1:] != ls[:-1]]))
    ids = ls[starts]
    assert int(ids[-1]) < K, (int(ids[-1]), K)
    xo, yo = X[order], Y[order]
    out["count"][ids] = np.diff(np.concatenate([starts, [len(ls)]]))
    out["min_x"][ids] = np.minimum.reduceat(xo, starts)
    out["max_x"][ids] = np.maximum.reduceat(xo, starts)
    out["min_y"][ids] = np.minimum.reduceat(yo, starts)
    out["max_y"][ids] = np.maximum.reduceat(yo, starts)
    return out


def label_stats(labels):
    """-> (n_clusters, max_label) of row labels: the ids in use and the largest of them (-1 without any)"""
    labels = np.asarray(labels)
    used = np.unique(labels[labels >= 0])
    return len(used), (int(used[-1]) if len(used) else -1)


def check_table(X, Y, labels, res, tag=None):
    """every field of every row of res.boxes against table_from_labels(X, Y, labels), and the two numbers of the header"""
    nc, ml = label_stats(labels)
    assert res.max_label == ml, (tag, res.max_label, ml)
    assert res.boxes is not None and len(res.boxes) == res.max_label + 1, (tag, res.max_label)
    want = table_from_labels(X, Y, labels, ml + 1)
    for f in FIELDS:
        bad = np.flatnonzero(res.boxes[f] != want[f])
        assert len(bad) == 0, (tag, f, len(bad), int(bad[0]), int(res.boxes[f][bad[0]]), int(want[f][bad[0]]))
    assert int((want["count"] > 0).sum()) == nc
    assert res.n_clusters == nc, (tag, res.n_clusters, nc)
