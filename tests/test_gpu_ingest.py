"""GPU: kernel K16 (cl_ingest_*) through cloops_amd.ingest, cloops_amd.pipe and the command lines against cloops_amd.io.parse_bedpe
(the reference-pinned host parser) and the reference's own digests: the corner corpus at every chunk budget, the fallback decision,
the example file and its duplicated head, the seeded synthetic, chromosomes left in HBM for the sweep, and whole runs with both
readers."""
import hashlib
import os
import subprocess
import sys

import joblib
import numpy as np
import pytest

import golden_util as G
import ingest_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = C.corpus()


def _env():
    return dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    return G.write_example_bedpe(tmp_path_factory.mktemp("example"))


@pytest.mark.parametrize("name,files,exotic", CORPUS, ids=[c[0] for c in CORPUS])
def test_corpus_every_budget(tmp_path, name, files, exotic):
    """every case x argument set x chunk budget equals cio.parse_bedpe (or raises what it raises) and the reference's digests; the
    device reads every case that is not exotic, the host exactly the exotic ones"""
    from cloops_amd import ingest
    from cloops_amd import io as cio
    fs = C.write_case(tmp_path, name, files)
    g = C.golden()
    long_last = 0 if all(f.endswith(b"\n") or not f for f in files) else 1
    for cs, cut, unique in C.ARGSETS:
        want = C.run(cio.parse_bedpe, fs, cs, cut, unique)
        for b in C.budgets(files):
            stats = {}
            kw = {"stats": stats} if b is None else {"stats": stats, "budget": b}
            got = C.run(ingest.parse_bedpe_gpu, fs, cs, cut, unique, **kw)
            C.assert_same(got, want, (name, cs, cut, unique, b))
            if got[0] == "ok":
                C.check_against_golden(g, name, cs, cut, unique, got[1], got[4])
            if exotic:
                assert stats["fallback"] is not None, (name, b)
            elif b is None or b >= C.longest_line(files) + long_last:
                assert stats["fallback"] is None, (name, b, stats["fallback"])


def test_example_and_duplicated_head(example, tmp_path):
    """the reference's digests of tests/test_io.py (parse2_sha1, raw0_*, raw1_*) from the device, without a fallback"""
    from cloops_amd import ests, ingest
    z = G.reference_checks()
    stats = {}
    mats, n_lines, n_cis = ingest.parse_bedpe_gpu([example], stats=stats)
    assert stats["fallback"] is None and (n_lines, n_cis) == (99674, 99674) and list(mats.keys()) == ["chr21"]
    assert G.digest(mats["chr21"]) == str(z["parse2_sha1"])
    for k, f in enumerate((example, G.write_dup(tmp_path, example))):
        d = tmp_path / ("raw%d" % k)
        d.mkdir()
        cfs, ds = ingest.parseRawBedpe([f], str(d), [], 0)
        rows = joblib.load(cfs[0])
        assert len(cfs) == 1 and G.digest(rows) == str(z["raw%d_sha1" % k]) and len(rows) == int(z["raw%d_rows" % k])
        assert G.digest(ds) == str(z["raw%d_ds_sha1" % k]) and len(ds) == int(z["raw%d_ds_len" % k])
        assert ests.estFragSize(ds) == int(z["raw%d_fragsize" % k])
        stats = {}
        ingest.parse_bedpe_gpu([f], unique=True, strand_distances=[], stats=stats, budget=1 << 16)
        assert stats["fallback"] is None


def test_synthetic_200k_against_the_reference(tmp_path):
    from cloops_amd import ingest
    fs = C.write_synth(tmp_path, 200000)
    g = C.golden()
    for cs, cut, unique in C.ARGSETS:
        for b in (None, 1 << 16):
            stats = {}
            got = C.run(ingest.parse_bedpe_gpu, fs, cs, cut, unique, stats=stats, **({} if b is None else {"budget": b}))
            assert stats["fallback"] is None
            assert C.check_against_golden(g, "synth200k", cs, cut, unique, got[1], got[4])


def test_synthetic_5m(tmp_path):
    """5 * 10^6 lines over 23 chromosomes in two files (plain, then .gz), with and without `unique`: equal to cio.parse_bedpe; two
    runs byte-identical"""
    from cloops_amd import ingest
    from cloops_amd import io as cio
    fs = C.write_synth(tmp_path, 5000000)
    for unique in (False, True):
        want = C.run(cio.parse_bedpe, fs, (), 0, unique)
        stats = {}
        got = C.run(ingest.parse_bedpe_gpu, fs, (), 0, unique, stats=stats, budget=32 << 20)
        assert stats["fallback"] is None and len(got[1]) == 23
        C.assert_same(got, want, unique)
        again = C.run(ingest.parse_bedpe_gpu, fs, (), 0, unique, budget=32 << 20)
        for c, m in got[1].items():
            assert m.tobytes() == again[1][c].tobytes()
        assert got[4] == again[4]


def test_wide_coordinates_and_domain(tmp_path):
    """mid-points beyond 31 bits and below zero: the duplicate filter's general path; load_bedpe raises the domain error of
    api.Chromosome while parse_bedpe_gpu returns the int64 rows"""
    from cloops_amd import _lib, ingest, pipe
    from cloops_amd import io as cio
    big = 1 << 40
    lines = [C.pet("chr1", big, big + 2, big + 500, big + 600), C.pet("chr1", -900, -800, -300, -200), C.pet("chr1", big, big + 2, big + 500, big + 600),
             C.pet("chr1", -900, -800, -300, -200, "+", "+"), C.pet("chr1", 5, 6, big, big), C.pet("chr1", -900, -800, -300, -201)]
    fs = C.write_case(tmp_path, "wide", [C._t(lines * 50)])
    for unique in (False, True):
        stats = {}
        C.assert_same(C.run(ingest.parse_bedpe_gpu, fs, (), 0, unique, stats=stats), C.run(cio.parse_bedpe, fs, (), 0, unique), unique)
        assert stats["fallback"] is None
    with pytest.raises(_lib.CloopsHipError) as ei:
        ingest.load_bedpe(fs, prefix="wide")
    assert ei.value.code == _lib.CL_ERR_DOMAIN
    assert not [f for f in pipe.CACHE._items if f.startswith("mem://wide/")]


def test_load_bedpe_feeds_the_sweep(example, tmp_path):
    """load_bedpe, then pipe.runSweepFast on its mem:// names: the candidates, cuts and steps of the same sweep on
    cio.parseRawBedpe2's .jd files (example file, mode 1)"""
    from cloops_amd import ingest, pipe
    from cloops_amd import io as cio
    eps, minPts = pipe.MODES[1][:2]
    d = tmp_path / "jd"
    d.mkdir()
    cfs = cio.parseRawBedpe2([example], str(d), [], 0)
    a = pipe.runSweepFast(cfs, eps, minPts)
    stats = {}
    names = ingest.load_bedpe([example], prefix="t", stats=stats)
    try:
        assert names == ["mem://t/chr21-chr21"] and stats["fallback"] is None and stats["cis"] == 99674
        r = pipe.CACHE.get(names[0])
        key, mat = pipe.parseJd(cfs[0])
        assert r.key == ("chr21", "chr21") and np.array_equal(r.X, mat[:, 1]) and np.array_equal(r.Y, mat[:, 2])
        b = pipe.runSweepFast(names, eps, minPts)
    finally:
        for f in names:
            pipe.CACHE.drop(f)
    strip = lambda steps: [{k: v for k, v in st.items() if k != "wall_s"} for st in steps]      # noqa: E731
    assert a[1:3] == b[1:3] and strip(a[3]) == strip(b[3])
    assert list(a[0].keys()) == list(b[0].keys())
    for key in a[0]:
        assert np.array_equal(np.asarray(a[0][key]["boxes"]), np.asarray(b[0][key]["boxes"]))
    pipe.CACHE.clear()


def test_exotic_input_loads_through_the_host(tmp_path):
    from cloops_amd import ingest, pipe
    files = dict((c[0], c[1]) for c in CORPUS)["underscore"]
    fs = C.write_case(tmp_path, "ex", files)
    stats = {}
    names = ingest.load_bedpe(fs, prefix="ex", stats=stats)
    try:
        assert names == ["mem://ex/chr1-chr1", "mem://ex/chr2-chr2"] and stats["fallback"] is not None
        r = pipe.CACHE.get(names[0])
        assert r.key == ("chr1", "chr1") and r.X.tolist() == [150, 350, 150] and len(r.chrom.neighbor_counts(1000)) == 3
    finally:
        for f in names:
            pipe.CACHE.drop(f)


def _run_cli(tmp_path, bed, out, extra):
    p = subprocess.run([sys.executable, "-m", "cloops_amd", "-f", bed, "-o", out, "-m", "1"] + extra, env=_env(), cwd=str(tmp_path), timeout=600,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    with open(os.path.join(str(tmp_path), out + ".loop"), "rb") as fh:
        return fh.read()


def test_command_line_both_readers(example, tmp_path):
    """`python -m cloops_amd -f example -o out -m 1 -s` with both readers: the same .loop (the golden's) and the same .jd; the same
    with -eps 0 -minPts 5 (duplicate filter and distances in the path); without -s no .jd is left"""
    with open(os.path.join(G.GOLD, "chr21_v2.loop"), "rb") as fh:
        golden = fh.read()
    loops = {r: _run_cli(tmp_path, example, "m1_" + r, ["-s", "-reader", r]) for r in ("gpu", "host")}
    assert loops["gpu"] == loops["host"] == golden
    jd = {}
    for r in ("gpu", "host"):
        assert os.listdir(str(tmp_path / ("m1_" + r))) == ["chr21-chr21.jd"]
        with open(str(tmp_path / ("m1_" + r) / "chr21-chr21.jd"), "rb") as fh:
            jd[r] = fh.read()
    assert jd["gpu"] == jd["host"]
    p = subprocess.run([sys.executable, "-m", "cloops_amd", "-f", example, "-o", "auto_gpu", "-eps", "0", "-minPts", "5", "-s"], env=_env(),
                       cwd=str(tmp_path), timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([sys.executable, "-m", "cloops_amd", "-f", example, "-o", "auto_host", "-eps", "0", "-minPts", "5", "-s", "-reader", "host"],
                       env=_env(), cwd=str(tmp_path), timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    for name in ("auto_%s.loop", os.path.join("auto_%s", "chr21-chr21.jd")):
        with open(str(tmp_path / (name % "gpu")), "rb") as fa, open(str(tmp_path / (name % "host")), "rb") as fb:
            assert fa.read() == fb.read(), name
    assert _run_cli(tmp_path, example, "nos", []) == golden
    assert not os.path.exists(str(tmp_path / "nos"))
    assert not [f for _, _, fl in os.walk(str(tmp_path)) for f in fl if f.endswith(".jd") and "nos" in f]


def test_ingest_command_line(example, tmp_path):
    from cloops_amd import io as cio
    p = subprocess.run([sys.executable, "-m", "cloops_amd.ingest", "-f", example, "-o", "jd", "-cut", "1000"], env=_env(), cwd=str(tmp_path),
                       timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    want = cio.parse_bedpe([example], cut=1000)[0]["chr21"]
    assert os.listdir(str(tmp_path / "jd")) == ["chr21-chr21.jd"]
    assert np.array_equal(joblib.load(str(tmp_path / "jd" / "chr21-chr21.jd")), want)


def test_read_between_sweep_steps_changes_nothing(example, tmp_path):
    """a read on the same device between two steps of a resident chromosome's sweep leaves the steps as they are"""
    from cloops_amd import api, ingest
    X, Y = G.chr21_xy()

    def sweep(with_k16):
        ch = api.Chromosome(X, Y)
        ch.set_device_labels(False)
        ch.cand_reset()
        out = []
        for step, (eps, cut) in enumerate(((1000, 0), (2000, 4601), (2000, 13532))):
            ch.step_async("v2", eps, 5, cut, step)
            ch.wait()
            ni, ns, st = ch.step_result()
            out.append((ni, ns, st["n_all"], st["sumx"], st["loghist"].tolist()))
            if with_k16:
                assert ingest.parse_bedpe_gpu([example], unique=True, strand_distances=[], budget=1 << 20)[2] == 99674
        out.append(ch.cand_finish(4601, 100000).tolist())
        ch.close()
        return out
    assert sweep(True) == sweep(False)
