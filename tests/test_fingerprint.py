"""CPU: contact-matrix fingerprints (cloops_amd.fingerprint, scripts/jd2fingerprint).  The K12 count histogram is replaced by a
numpy brute force over the PETs (`brute_hist`, also the yardstick of the GPU tests in test_gpu_fingerprint.py); fed through the
host functions it must reproduce the goldens that the script's own functions wrote (tests/golden/make_golden_fingerprint.py)
array for array and text for text."""
import json
import logging
import os

import joblib
import numpy as np
import pytest

import golden_util as G

GOLD = G.GOLD
DIRS = ("chr21_A", "chr21_B", "synth_C")


def brute_hist(X, Y, bs, cut=0):
    """numpy restatement of cl_contact_hist: (values ascending, mult, kept PETs, minC or None).  Rows with Y - X >= cut when
    cut > 0; cell ((x - minC) // bs, (y - minC) // bs), minC over both columns of the kept rows."""
    X = np.asarray(X, np.int64)
    Y = np.asarray(Y, np.int64)
    if cut > 0:
        keep = (Y - X) >= cut
        X, Y = X[keep], Y[keep]
    if len(X) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0, None
    mn = min(X.min(), Y.min())
    _, counts = np.unique(np.stack([(X - mn) // bs, (Y - mn) // bs], 1), axis=0, return_counts=True)
    values, mult = np.unique(counts, return_counts=True)
    return values.astype(np.int64), mult.astype(np.int64), len(X), int(mn)


def expand(values, mult):
    return np.repeat(np.asarray(values, np.int64), np.asarray(mult, np.int64))


def brute_backend(monkeypatch):
    """route fingerprint._cell_hist (K12 on the resident chromosome) to brute_hist on the .jd file"""
    from cloops_amd import fingerprint, pipe

    def cell_hist(f, cut, bs):
        _, mat = pipe.parseJd(f, 0)
        mat = np.asarray(mat).reshape(-1, 3)
        v, m, kept, _ = brute_hist(mat[:, 1], mat[:, 2], bs, cut)
        return v, m, kept
    monkeypatch.setattr(fingerprint, "_cell_hist", cell_hist)


def datasets():
    """{dir name: {chrom: (X, Y)}}: A = the chr21 example, B = its subsample, C = the two-chromosome set of the golden script"""
    X, Y = G.chr21_xy()
    zs = np.load(os.path.join(GOLD, "chr21_quant_subsample.npz"))
    rows = np.flatnonzero(np.unpackbits(zs["mask"])[:int(zs["n"])])
    z = np.load(os.path.join(GOLD, "fingerprint_setC.npz"))
    c = {k[2:]: (z[k].astype(np.int64), z["Y_" + k[2:]].astype(np.int64)) for k in z.files if k.startswith("X_")}
    return {"chr21_A": {"chr21": (X, Y)}, "chr21_B": {"chr21": (X[rows], Y[rows])}, "synth_C": c}


def write_datasets(root):
    """.jd directories of A, B, C under `root` -> {name: dir}"""
    out = {}
    for name, chroms in datasets().items():
        d = os.path.join(str(root), name)
        os.makedirs(d)
        for chrom, (x, y) in chroms.items():
            joblib.dump(np.stack([np.arange(len(x)), x, y], 1).astype(np.int64), os.path.join(d, "%s-%s.jd" % (chrom, chrom)))
        out[name] = d
    return out


def golden_arrays():
    return np.load(os.path.join(GOLD, "fingerprint_arrays.npz"))


def golden_meta():
    with open(os.path.join(GOLD, "fingerprint_meta.json")) as fh:
        return json.load(fh)


def golden_cases():
    """(dataset, bs, cut, tag) of every golden array"""
    meta = golden_meta()
    out = [(name, bs, 0, "bs%d" % bs) for name in DIRS for bs in meta["bin_sizes"]]
    return out + [(name, 2000, meta["cut"], "bs2000_cut%d" % meta["cut"]) for name in DIRS]


def _read(path):
    with open(path) as fh:
        return fh.read()


def reference_bins(ds, bins=100):
    """scripts/jd2fingerprint:53-65 restated literally (Python-2 integer step): sort, slice, sum, cumsum, divide"""
    ds = np.sort(np.asarray(ds, np.int64))
    nn = []
    step = len(ds) // bins
    for i in range(0, len(ds), step):
        if i + step > len(ds):
            break
        nn.append(ds[i:i + step].sum())
    nn = np.array(nn)
    return np.cumsum(nn) / float(nn.sum())


def test_brute_force_counts_match_golden():
    ga = golden_arrays()
    data = datasets()
    for name, bs, cut, tag in golden_cases():
        hs = [brute_hist(x, y, bs, cut) for x, y in data[name].values()]
        got = np.sort(np.concatenate([expand(v, m) for v, m, _, _ in hs]))
        assert np.array_equal(got, ga["counts_%s_%s" % (name, tag)]), (name, tag)


def test_groups_match_golden():
    from cloops_amd import fingerprint
    ga = golden_arrays()
    raises = golden_meta()["raises"]
    for name, bs, cut, tag in golden_cases():
        counts = ga["counts_%s_%s" % (name, tag)]
        hist = tuple(np.unique(counts, return_counts=True))
        key = "groups_%s_%s" % (name, tag)
        if key in raises:
            with pytest.raises(ValueError):
                fingerprint.contactMatrixUpper2Bins(hist)
            continue
        want = ga[key]
        assert np.array_equal(fingerprint.contactMatrixUpper2Bins(hist), want), key      # bit for bit
        assert np.array_equal(fingerprint.contactMatrixUpper2Bins(counts[::-1].copy()), want), key


def test_jds2fingerprint_genome_wide(tmp_path, monkeypatch):
    """the .jd files of a directory merged genome-wide (C has two chromosomes), with and without a cut"""
    from cloops_amd import fingerprint
    brute_backend(monkeypatch)
    dirs = write_datasets(tmp_path)
    ga = golden_arrays()
    raises = golden_meta()["raises"]
    for name, bs, cut, tag in golden_cases():
        jds = [os.path.join(dirs[name], f) for f in sorted(os.listdir(dirs[name]))]
        key = "groups_%s_%s" % (name, tag)
        if key in raises:
            with pytest.raises(ValueError):
                fingerprint.jds2FingerPrint(jds, cut, bs, 1)
        else:
            assert np.array_equal(fingerprint.jds2FingerPrint(jds, cut, bs, 1), ga[key]), key
    with pytest.raises(ValueError):
        fingerprint.jds2FingerPrint([], 0, 2000)


def test_cli_matches_golden(tmp_path, monkeypatch):
    from cloops_amd import fingerprint
    brute_backend(monkeypatch)
    dirs = write_datasets(tmp_path)
    d = ",".join(dirs[n] for n in DIRS)
    out = os.path.join(str(tmp_path), "x")
    assert fingerprint.main(["-d", d, "-o", out, "-labels", "A,B,C", "-bs", "2000"]) == 0
    assert _read(out + "_fingerprint.txt") == _read(os.path.join(GOLD, "fp_labels_fingerprint.txt"))
    assert not os.path.exists(out + "_fingerprint.pdf")
    out = os.path.join(str(tmp_path), "y")
    assert fingerprint.main(["-d", d, "-o", out, "-bs", "10000", "-p", "8"]) == 0
    assert _read(out + "_fingerprint.txt") == _read(os.path.join(GOLD, "fp_bs10000_fingerprint.txt"))


def test_cut_flag_has_no_effect(tmp_path, monkeypatch):
    """-cut is accepted and not passed on (scripts/jd2fingerprint:91-95); at function level cut filters"""
    from cloops_amd import fingerprint
    brute_backend(monkeypatch)
    dirs = write_datasets(tmp_path)
    out = os.path.join(str(tmp_path), "x")
    assert fingerprint.main(["-d", ",".join(dirs[n] for n in DIRS), "-o", out, "-labels", "A,B,C", "-cut", "4601"]) == 0
    assert _read(out + "_fingerprint.txt") == _read(os.path.join(GOLD, "fp_labels_fingerprint.txt"))
    ga = golden_arrays()
    jd = os.path.join(dirs["chr21_A"], "chr21-chr21.jd")
    got = fingerprint.jds2FingerPrint([jd], cut=4601, binSize=2000)
    assert np.array_equal(got, ga["groups_chr21_A_bs2000_cut4601"])
    assert not np.array_equal(got, ga["groups_chr21_A_bs2000"])


@pytest.mark.parametrize("name", ["chr21_A", "synth_C"])
def test_raises_write_nothing(tmp_path, monkeypatch, name):
    """A at bs 1e6: 672 cells, step 6, 112 groups -> pandas' ValueError; C at bs 1e6: 2 cells, step 0 -> ValueError"""
    from cloops_amd import fingerprint
    brute_backend(monkeypatch)
    dirs = write_datasets(tmp_path)
    assert golden_meta()["raises"]["getFingerPrint_%s_bs1000000" % name] == "ValueError"
    out = os.path.join(str(tmp_path), "x")
    with pytest.raises(ValueError):
        fingerprint.main(["-d", dirs[name], "-o", out, "-bs", "1000000"])
    assert not os.path.exists(out + "_fingerprint.txt")


def test_label_quirks(tmp_path, monkeypatch, caplog):
    from cloops_amd import fingerprint
    brute_backend(monkeypatch)
    dirs = write_datasets(tmp_path)
    a, b, c = (dirs[n] for n in DIRS)
    ga = golden_arrays()
    pre = os.path.join(str(tmp_path), "q")
    # a trailing slash makes the default label ""
    df = fingerprint.getFingerPrint(a + "/," + b, "", pre, plot=0)
    assert list(df.columns) == ["random", "", "chr21_B"]
    assert _read(pre + "_fingerprint.txt").split("\n")[0] == ",random,,chr21_B"
    # an empty entry of -labels falls back to the directory name
    df = fingerprint.getFingerPrint(",".join((a, b, c)), "A,,C", pre, plot=0)
    assert list(df.columns) == ["random", "A", "chr21_B", "C"]
    # a repeated label replaces the earlier column's values and keeps its position
    df = fingerprint.getFingerPrint(",".join((a, b, c)), "X,Y,X", pre, plot=0)
    assert list(df.columns) == ["random", "X", "Y"]
    assert np.array_equal(df["X"].values, ga["groups_synth_C_bs2000"])
    assert np.array_equal(df["Y"].values, ga["groups_chr21_B_bs2000"])
    # a label count that differs from the directory count: an error, nothing written
    pre2 = os.path.join(str(tmp_path), "none")
    with caplog.at_level(logging.ERROR, logger="cloops_amd.fingerprint"):
        assert fingerprint.getFingerPrint(",".join((a, b)), "A,B,C", pre2, plot=0) is None
    assert "not equal" in caplog.text
    assert not os.path.exists(pre2 + "_fingerprint.txt")
    assert fingerprint.main(["-d", a, "-o", pre2, "-labels", "A,B"]) == 0
    assert not os.path.exists(pre2 + "_fingerprint.txt")


def test_bin_size_below_one(tmp_path, monkeypatch):
    """binSize < 1 is refused before any counting (documented deviation: the script divides by zero / mirrors cells)"""
    from cloops_amd import fingerprint

    def no_counting(*a):
        raise AssertionError("counted with binSize < 1")
    monkeypatch.setattr(fingerprint, "_cell_hist", no_counting)
    dirs = write_datasets(tmp_path)
    jd = os.path.join(dirs["chr21_A"], "chr21-chr21.jd")
    for bs in (0, -1, -2000):
        with pytest.raises(ValueError):
            fingerprint.jd2contactMatrixUpper(jd, 0, bs)
        with pytest.raises(ValueError):
            fingerprint.jds2FingerPrint([jd], 0, bs)
        with pytest.raises(ValueError):
            fingerprint.main(["-d", dirs["chr21_A"], "-o", os.path.join(str(tmp_path), "z"), "-bs", str(bs)])
    assert not os.path.exists(os.path.join(str(tmp_path), "z_fingerprint.txt"))


def test_no_rows_after_cut(tmp_path, monkeypatch):
    from cloops_amd import fingerprint
    brute_backend(monkeypatch)
    jd = os.path.join(str(tmp_path), "chrZ-chrZ.jd")
    joblib.dump(np.array([[0, 100, 150], [1, 200, 260]], np.int64), jd)
    with pytest.raises(ValueError):
        fingerprint.jd2contactMatrixUpper(jd, 1000, 10)
    v, m = fingerprint.jd2contactMatrixUpper(jd, 55, 10)
    assert v.tolist() == [1] and m.tolist() == [1]


@pytest.mark.parametrize("plot", ["1", "0"])
def test_plot_flag_is_bool(tmp_path, monkeypatch, plot):
    """-plot is type=bool: any non-empty value plots, 0 included"""
    from cloops_amd import fingerprint
    brute_backend(monkeypatch)
    dirs = write_datasets(tmp_path)
    out = os.path.join(str(tmp_path), "p")
    assert fingerprint.main(["-d", dirs["chr21_B"], "-o", out, "-plot", plot]) == 0
    assert os.path.getsize(out + "_fingerprint.pdf") > 0


def test_grouping_matches_sort_and_slice():
    """group_sums / contactMatrixUpper2Bins on seeded random histograms against the literal sort-and-slice, bit for bit --
    steps that split runs of equal counts, partial tails dropped, more groups than bins"""
    from cloops_amd import fingerprint
    rng = np.random.default_rng(7)
    for trial in range(300):
        nd = int(rng.integers(1, 40))
        values = np.sort(rng.choice(np.arange(1, 5000), nd, replace=False)).astype(np.int64)
        mult = rng.integers(1, 400, nd).astype(np.int64)
        if trial % 3 == 0:
            mult[0] = int(rng.integers(1000, 20000))                       # one long run of 1-ish counts
        bins = int(rng.choice([1, 3, 7, 100, 101, 1000]))
        ds = expand(values, mult)
        if len(ds) // bins == 0:
            with pytest.raises(ValueError):
                fingerprint.contactMatrixUpper2Bins((values, mult), bins)
            continue
        perm = rng.permutation(nd)                                          # histogram order does not matter
        got = fingerprint.contactMatrixUpper2Bins((values[perm], mult[perm]), bins)
        want = reference_bins(ds, bins)
        assert got.dtype == want.dtype and np.array_equal(got, want), trial
        step = len(ds) // bins
        gs = fingerprint.group_sums(values, mult, bins)
        assert np.array_equal(gs, ds[:len(gs) * step].reshape(-1, step).sum(axis=1))


def test_merge_hists():
    from cloops_amd import fingerprint
    rng = np.random.default_rng(5)
    parts = [rng.integers(1, 30, int(rng.integers(1, 200))) for _ in range(5)]
    hs = [tuple(np.unique(p, return_counts=True)) for p in parts]
    v, m = fingerprint.merge_hists(hs)
    assert np.array_equal(expand(v, m), np.sort(np.concatenate(parts)))
    with pytest.raises(ValueError):
        fingerprint.merge_hists([])


def test_brute_hist_by_dicts():
    """the brute force against the script's dict of dicts (Python-2 floor division) on a small case with negative offsets"""
    rng = np.random.default_rng(9)
    X = rng.integers(-5000, 5000, 3000)
    Y = X + rng.integers(0, 3000, 3000)
    for bs, cut in ((1, 0), (7, 0), (250, 0), (250, 800), (100000, 0)):
        keep = (Y - X >= cut) if cut > 0 else np.ones(len(X), bool)
        x, y = X[keep], Y[keep]
        mn = min(x.min(), y.min())
        ds = {}
        for a, b in zip(x.tolist(), y.tolist()):
            k = ((a - mn) // bs, (b - mn) // bs)
            ds[k] = ds.get(k, 0) + 1
        v, m, kept, minc = brute_hist(X, Y, bs, cut)
        assert kept == len(x) and minc == mn
        assert np.array_equal(expand(v, m), np.sort(np.array(list(ds.values()))))
