"""Access to the committed golden vectors (tests/golden/, made by make_golden.py)."""
import hashlib
import json
import os

import numpy as np

import cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_cache = {}


def _npz(name):
    if name not in _cache:
        _cache[name] = np.load(os.path.join(GOLD, name))
    return _cache[name]


def meta():
    with open(os.path.join(GOLD, "golden_meta.json")) as fh:
        return json.load(fh)


def chr21_xy():
    z = _npz("chr21_input.npz")
    return z["X"].astype(np.int64), z["Y"].astype(np.int64)


def chr21_labels(variant, eps, minPts):
    return _npz("chr21_labels.npz")["%s_%d_%d" % (variant, eps, minPts)]


def chr21_chain_labels(variant, eps):
    return _npz("chr21_chain_labels.npz")["%s_%d" % (variant, eps)]


def family_cases(family, ncase=60):
    """Yield (k, ids, X, Y, eps, minPts, {variant: golden labels})."""
    z = _npz("families.npz")
    for k in range(ncase):
        ids, X, Y = z["%s_%d_in" % (family, k)].astype(np.int64)
        eps, minPts = (int(v) for v in z["%s_%d_par" % (family, k)])
        yield k, ids, X, Y, eps, minPts, {v: z["%s_%d_%s" % (family, k, v)] for v in ("v1", "v2", "block")}


def synth150k():
    from cloops_amd.synth import synth_chrom
    X, Y = synth_chrom(150000, 46709983, 424242)
    z = _npz("synth150k_labels.npz")
    chk = z["XY_sha_check"]
    assert int(X.astype(np.int64).sum() % (1 << 31)) == int(chk[0]), "synthetic generator drifted"
    assert int(Y.astype(np.int64).sum() % (1 << 31)) == int(chk[1]), "synthetic generator drifted"
    return X.astype(np.int64), Y.astype(np.int64), z


def dense400k():
    """-> (X, Y, npz of label arrays, meta): the headline regime, labels made by the REAL classes (golden/make_golden_dense.py)"""
    import hashlib
    from cloops_amd.synth import synth_chrom
    with open(os.path.join(GOLD, "dense400k_meta.json")) as fh:
        m = json.load(fh)
    X, Y = synth_chrom(m["n"], m["length"], m["seed"])
    assert hashlib.sha1(np.stack([X, Y]).astype(np.int32).tobytes()).hexdigest() == m["input_sha1"], "synthetic generator drifted"
    return X.astype(np.int64), Y.astype(np.int64), _npz("dense400k_labels.npz"), m


DENSE_SETTINGS = ((5000, 50, 0), (7500, 30, 5004), (10000, 20, 6250))

FAMILY_SEEDS = {"adversarial": 0, "plain": 1, "clumpy": 2}


def regenerate_family(family, ncase=60):
    rng = np.random.default_rng(FAMILY_SEEDS[family])
    gen = getattr(cases, family + "_case")
    return [gen(rng, k) for k in range(ncase)]


_MIX = np.array([0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x27D4EB2F165667C5], dtype=np.uint64)


def box_checksum(boxes):
    """order-independent checksum of int rows (minX, maxX, minY, maxY): sum over rows of a 64-bit mix, mod 2^64"""
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = (b * _MIX[None, :]).sum(axis=1, dtype=np.uint64)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
        return int(h.sum(dtype=np.uint64))


# ---- what the reference's OWN code returned, for the tests that pin against it (golden/make_golden_reference_checks.py) ----
REFERENCE_NAME = "GSM1872886_GM12878_CTCF_ChIA-PET_chr21_hg38.bedpe.gz"     # the reference's bundled example (GEO GSM1872886, chr21)
STRANDS = ("+", "-")
CMODEL_TABLE = os.path.join(GOLD, "chr21_cmodel_table.json")
ORACLE_FAMILIES = (("adversarial", 0, 120), ("plain", 1, 120), ("clumpy", 2, 120))
FAMILY_NCASE = 60                                          # cases per family in families.npz
SCALES = ((50, 1), (1, 50))


def reference_checks():
    return _npz("reference_checks.npz")


def cmodel_table():
    with open(CMODEL_TABLE) as fh:
        return json.load(fh)


def digest(a):
    """sha1 of an integer array (shape included), as int64"""
    a = np.ascontiguousarray(a, dtype=np.int64)
    return hashlib.sha1(repr(a.shape).encode() + a.tobytes()).hexdigest()


def hash_case(h, ids, X, Y, eps, minPts):
    for a in (ids, X, Y, [eps, minPts]):
        h.update(np.ascontiguousarray(a, dtype=np.int64).tobytes())


def oracle_reference_labels(family, k, variant):
    """the real class's labels on case k of a seeded family: cases 0-59 are those of families.npz (make_golden.py), the later ones
    are stored in reference_checks.npz"""
    if k < FAMILY_NCASE:
        return _npz("families.npz")["%s_%d_%s" % (family, k, variant)]
    return reference_checks()["oracle_%s_%d_%s" % (family, k, variant)]


def oracle_family(family, seed, ncase):
    """-> [(k, ids, X, Y, eps, minPts)] regenerated from the seed, checked against the sha1 the golden was made on"""
    rng = np.random.default_rng(seed)
    gen = getattr(cases, family + "_case")
    h, out = hashlib.sha1(), []
    for k in range(ncase):
        ids, X, Y, eps, minPts = gen(rng, k)
        hash_case(h, ids, X, Y, eps, minPts)
        out.append((k, ids, X, Y, eps, minPts))
    assert h.hexdigest() == str(reference_checks()["oracle_%s_in_sha1" % family]), "case generator drifted"
    return out


def scaled_cases():
    """-> [(k, X, Y)]: int64 coordinates near 1e8 with vertical stripes, to be stretched x50 along one axis"""
    rng = np.random.default_rng(3)
    out = []
    for k in range(8):
        n = int(rng.integers(200, 1500))
        X = rng.integers(10 ** 8, 10 ** 8 + 40000, n).astype(np.int64)
        Y = X + rng.integers(0, 400000, n)
        if k % 2:
            X[: n // 3] = X[0] + rng.integers(-3, 4, n // 3)      # a vertical stripe
        out.append((k, X, Y))
    return out


def ests_draws():
    """-> 20 (inter, self) distance draws for estIntSelCutFrag"""
    rng = np.random.default_rng(3)
    out = []
    for _ in range(20):
        di = np.exp(rng.normal(10, 1.5, 3000)).astype(np.int64).astype(float)
        ds = np.exp(rng.normal(6, 1.0, 5000)).astype(np.int64).astype(float)
        out.append((di, ds))
    return out


def example_columns(text):
    """the example BEDPE's text -> the arrays chr21_example_bedpe.npz stores next to chr21_input.npz's mid-points (X, Y):
    per line the two fragment lengths, whether the PET rule swapped the ends (cLoops/io.py:49-57), the two strands"""
    f = [l.split("\t") for l in text.split("\n") if l]
    s1, e1, s2, e2 = (np.asarray([int(x[c]) for x in f], np.int64) for c in (1, 2, 4, 5))
    return {"len1": (e1 - s1).astype(np.uint8), "len2": (e2 - s2).astype(np.uint8), "swap": s1 + e1 > s2 + e2,
            "strand1": np.asarray([STRANDS.index(x[8]) for x in f], np.uint8), "strand2": np.asarray([STRANDS.index(x[9]) for x in f], np.uint8),
            "text_sha1": np.asarray(hashlib.sha1(text.encode()).hexdigest())}


def write_example_bedpe(dirpath):
    """the reference's bundled example BEDPE rebuilt byte for byte (checked against the original's sha1) from the chr21 mid-points
    and tests/golden/chr21_example_bedpe.npz; written gzipped into `dirpath` -> its path"""
    import gzip
    z = _npz("chr21_example_bedpe.npz")
    X, Y = chr21_xy()
    swap = z["swap"].astype(bool)
    l1, l2 = z["len1"].astype(np.int64), z["len2"].astype(np.int64)
    s1 = np.where(swap, Y, X) - l1 // 2                  # mid (2s + l) // 2 == s + l // 2
    s2 = np.where(swap, X, Y) - l2 // 2
    text = "".join("chr21\t%d\t%d\tchr21\t%d\t%d\t%d\t.\t%s\t%s\n" % (a, a + la, b, b + lb, i, STRANDS[p], STRANDS[q])
                   for i, (a, la, b, lb, p, q) in enumerate(zip(s1.tolist(), l1.tolist(), s2.tolist(), l2.tolist(),
                                                                z["strand1"].tolist(), z["strand2"].tolist())))
    assert hashlib.sha1(text.encode()).hexdigest() == str(z["text_sha1"]), "example BEDPE not rebuilt exactly"
    path = os.path.join(str(dirpath), "chr21_example.bedpe.gz")
    with gzip.open(path, "wt", compresslevel=1) as fh:
        fh.write(text)
    return path


def write_dup(dirpath, example):
    """a BEDPE with duplicated PETs (the example holds none): the example's first 3000 lines followed by its first 1000 again"""
    import gzip
    dup = os.path.join(str(dirpath), "dup.bedpe")
    with gzip.open(example, "rt") as fh:
        head = [next(fh) for _ in range(3000)]
    with open(dup, "w") as fh:
        fh.writelines(head + head[:1000])
    return dup
