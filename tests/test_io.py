"""CPU: BEDPE input side (cLoops/io.py:30-59,132-217 restated in cloops_amd/io.py)."""
import gzip
import os

import numpy as np
import pytest

import golden_util as G
from cloops_amd import io as cio


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """the reference's bundled example BEDPE, rebuilt from the stored columns (golden_util.write_example_bedpe)"""
    return G.write_example_bedpe(tmp_path_factory.mktemp("example"))


LINES = [
    "chr1\t100\t201\tchr1\t5000\t5100\tid1\t1\t+\t-",        # mid 150 (floor of 150.5), 5050
    "chr1\t9000\t9100\tchr1\t300\t401\tid2\t1\t+\t-",        # ends swapped: left = (300,401) -> 350
    "chr1\t10\t20\tchr2\t30\t40\tid3\t1\t+\t-",              # trans: dropped
    "chr1\t*\t-1\tchr1\t30\t40\tid4\t1\t+\t-",               # '*' and '-1': dropped
    "chr1\t10\t20\tchr1",                                    # < 6 fields: dropped
    "chr1\tx\t20\tchr1\t30\t40\tid5\t1\t+\t-",               # non-integer: dropped
    "chr2\t7\t8\tchr2\t7\t9\tid6\t1\t-\t-",                  # 7 , 8
    "chr1\t1000\t1001\tchr1\t1100\t1101\tid7\t1\t+\t+",      # distance 100
]


def test_pet_rule_and_filters(tmp_path):
    f = tmp_path / "t.bedpe"
    f.write_text("\n".join(LINES) + "\n")
    mats, n_lines, n_cis = cio.parse_bedpe([str(f)])
    assert n_lines == 8 and n_cis == 4
    assert list(mats.keys()) == ["chr1", "chr2"]
    assert mats["chr1"].tolist() == [[0, 150, 5050], [1, 350, 9050], [2, 1000, 1100]]
    assert mats["chr2"].tolist() == [[0, 7, 8]]
    mats, _, _ = cio.parse_bedpe([str(f)], cs=["chr1"], cut=200)
    assert list(mats.keys()) == ["chr1"] and mats["chr1"].tolist() == [[0, 150, 5050], [1, 350, 9050]]


def test_jd_round_trip(tmp_path):
    f = tmp_path / "t.bedpe.gz"
    with gzip.open(str(f), "wt") as fh:
        fh.write("\n".join(LINES) + "\n")
    cfs = [cio.txt2jd(c) for c in cio.parseRawBedpe2([str(f)], str(tmp_path), [], 0)]
    assert sorted(os.path.basename(c) for c in cfs) == ["chr1-chr1.jd", "chr2-chr2.jd"]
    key, mat = cio.parseJd([c for c in cfs if "chr1" in c][0])
    assert key == ("chr1", "chr1") and mat.dtype == np.int64 and mat.shape == (3, 3)
    key, mat = cio.parseJd([c for c in cfs if "chr1" in c][0], cut=200)
    assert mat.shape == (2, 3)


def test_example_bedpe_matches_golden_input(example):
    mats, n_lines, n_cis = cio.parse_bedpe([example])
    X, Y = G.chr21_xy()
    assert list(mats.keys()) == ["chr21"] and n_cis == 99674
    assert np.array_equal(mats["chr21"][:, 1], X) and np.array_equal(mats["chr21"][:, 2], Y)
    m = G.meta()["chr21"]
    assert (int(X.min()), int(X.max()), int(Y.min()), int(Y.max())) == (m["xmin"], m["xmax"], m["ymin"], m["ymax"])


def test_against_reference_parser_with_py2_semantics(example):
    """The reference's own PET class + parseRawBedpe2 (sliced out of the py2-only io.py, with the
    two py2->py3 semantic patches `/ 2` -> `// 2` and "rb" -> "rt") on the example file: its output
    is stored as a digest in tests/golden/reference_checks.npz (tests/golden/make_golden_reference_checks.py)."""
    mats, _, _ = cio.parse_bedpe([example])
    assert G.digest(mats["chr21"]) == str(G.reference_checks()["parse2_sha1"])


def test_auto_eps_path_against_the_reference(example, tmp_path):
    """`eps = 0` (cLoops/pipe.py:231-239): the reference's parseRawBedpe (duplicate removal, distances of the PETs mapped to
    different strands; sliced out of the py2-only io.py with the same two py2 -> py3 patches as above) and its own
    estFragSize (ests.py:23-33) on the example file, against cloops_amd.io.parseRawBedpe / cloops_amd.ests.estFragSize.
    What the reference returned is stored in tests/golden/reference_checks.npz."""
    import joblib
    from cloops_amd import ests
    z = G.reference_checks()
    # the example file, and a file with duplicated PETs (the example holds none): the first 3000 lines followed by the
    # first 1000 again
    dup = G.write_dup(tmp_path, example)
    for k, f in enumerate((example, dup)):
        mine = tmp_path / ("mine%d" % k)
        mine.mkdir()
        cfs2, ds2 = cio.parseRawBedpe([f], str(mine), [], 0)
        assert len(cfs2) == 1
        rows = joblib.load(cfs2[0])
        assert G.digest(rows) == str(z["raw%d_sha1" % k]) and len(rows) == int(z["raw%d_rows" % k])
        n = int(z["raw%d_ds_len" % k])
        assert G.digest(ds2) == str(z["raw%d_ds_sha1" % k]) and len(ds2) == n and n > 100 and n < len(rows)
        want = int(z["raw%d_fragsize" % k])
        assert ests.estFragSize(ds2) == want and want > 0
        if k == 1:
            mats, _, _ = cio.parse_bedpe([f])
            assert len(rows) < len(mats["chr21"])            # the duplicate filter really dropped PETs
