"""GPU: kernel K15 (cl_conv_create / cl_conv_feed / cl_conv_render) through cloops_amd.convert and its command line against the
reference's goldens (tests/golden/make_golden_convert.py) and the brute-force restatement of convert_cases.py: every chunk
boundary kind, gz input, errors and their written prefixes, the seeded synthetics, determinism, its effect on a sweep (none),
and a converted pairs file run through `python -m cloops_amd`."""
import gzip
import hashlib
import os
import subprocess
import sys

import joblib
import numpy as np
import pytest

import convert_cases as C
import golden_util as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    return dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))


def _write(path, data):
    with open(str(path), "wb") as fh:
        fh.write(data)
    return str(path)


def _read_out(path):
    with open(str(path), "rb") as fh:
        raw = fh.read()
    return gzip.decompress(raw) if str(path).endswith(".gz") else raw


def _conv(fmt, f, out, ext, budget=None, threads=8):
    from cloops_amd import convert
    kw = {"ext": ext, "budget": budget or convert.BUDGET}
    if fmt == "hicpro":
        return convert.pairs2bedpe(f, out, threads=threads, **kw)
    return convert.long2bedpe(f, out, **kw)


def _longest(data):
    return max([len(l) + 1 for l in C.split_lines(data)] or [1])


def test_goldens_every_budget(tmp_path):
    """every golden byte-exact, at the default budget and at budgets from the longest line upwards; errors raise at the
    reference's line and leave exactly its prefix (a valid gzip file for hicpro)"""
    for g in C.golden_meta()["cases"]:
        data, want = C.golden_case(g["name"])
        f = _write(tmp_path / "in.txt", data)
        out = str(tmp_path / ("o.bedpe.gz" if g["format"] == "hicpro" else "o.bedpe"))
        L = _longest(data)
        for budget in [None] + sorted(b for b in {L, L + 1, L + 7, 2 * L + 1, 4096} if b >= L):
            if g["error"] is None:
                assert _conv(g["format"], f, out, g["ext"], budget) == (g["lines"], len(want)), (g["name"], budget)
            else:
                with pytest.raises(ValueError) as ei:
                    _conv(g["format"], f, out, g["ext"], budget)
                assert str(ei.value).startswith("%s:%d: " % (f, g["lines"] + 1)), (g["name"], budget, str(ei.value))
            assert _read_out(out) == want, (g["name"], budget)
            assert hashlib.sha256(_read_out(out)).hexdigest() == g["sha256"]


def test_chunk_boundaries(tmp_path):
    """CRLF split across chunks, a line exactly filling a chunk, no final newline, an empty file, a file of only '\\n', a line
    longer than the budget"""
    line = b"r\tc\t10\t+\tc\t20\t-\r\n"
    data = line * 7 + b"r\tc\t10\t+\tc\t20\t-"
    f = _write(tmp_path / "in", data)
    want = C.brute("hicpro", data, 50)[0]
    for budget in range(len(line), 4 * len(line) + 3):
        assert _conv("hicpro", f, str(tmp_path / "o.gz"), 50, budget) == (8, len(want)), budget
        assert _read_out(tmp_path / "o.gz") == want, budget
    jl = b"0 c 10 0 16 c 20\r\n"
    jd = jl * 9
    fj = _write(tmp_path / "j", jd)
    for budget in range(len(jl), 3 * len(jl) + 2):
        assert _conv("juicer", fj, str(tmp_path / "o.txt"), 75, budget) == (9, len(C.brute("juicer", jd, 75)[0]))
        assert _read_out(tmp_path / "o.txt") == C.brute("juicer", jd, 75)[0]
    with pytest.raises(ValueError, match=r":1: line longer than the chunk budget"):
        _conv("hicpro", f, str(tmp_path / "o.gz"), 50, len(line) - 1)
    assert _read_out(tmp_path / "o.gz") == b""
    e = _write(tmp_path / "empty", b"")
    assert _conv("hicpro", e, str(tmp_path / "e.gz"), 50) == (0, 0)
    assert _read_out(tmp_path / "e.gz") == b""
    assert _conv("juicer", e, str(tmp_path / "e.txt"), 75) == (0, 0)
    assert _read_out(tmp_path / "e.txt") == b""
    nl = _write(tmp_path / "nl", b"\n")
    for fmt in ("hicpro", "juicer"):
        with pytest.raises(ValueError, match=r":1: fewer than 7 fields"):
            _conv(fmt, nl, str(tmp_path / "nl.gz"), 50)


def test_short_lines_and_line_numbers(tmp_path):
    """more lines than one feed takes (budget / 16 + 256): the feed stops early and the rest is fed again; line numbers count
    across feeds and chunks"""
    from cloops_amd import api
    row = b"0 c 1 0 0 c 2\n"
    data = row * 20000
    f = _write(tmp_path / "short", data)
    want = C.brute("juicer", data, 3)[0]
    assert _conv("juicer", f, str(tmp_path / "o"), 3, 65536) == (20000, len(want))
    assert _read_out(tmp_path / "o") == want
    bad = row * 15000 + b"0 c x 0 0 c 2\n" + row * 10
    fb = _write(tmp_path / "bad", bad)
    with pytest.raises(ValueError, match=r":15001: not an integer"):
        _conv("juicer", fb, str(tmp_path / "o"), 3, 65536)
    assert _read_out(tmp_path / "o") == C.brute("juicer", row * 15000, 3)[0]
    # the handle directly: consumed bytes, global line numbers, an error in the second feed
    from cloops_amd import _lib
    lib = _lib.load()
    cv = api.Converter("hicpro", 50, 1024)
    pin = lib.cl_host_alloc(2048)
    try:
        import ctypes
        buf = (ctypes.c_char * 2048).from_address(pin)
        chunk = b"r\tc\t10\t+\tc\t20\t-\n" * 3 + b"r\tc\t1"
        buf[:len(chunk)] = chunk
        used, nl, nb, err = cv.feed(pin, len(chunk), False)
        assert (used, nl, err) == (len(chunk) - 5, 3, None)
        got = cv.render(pin + 1024, 1024)
        assert bytes(buf[1024:1024 + got]) == C.brute("hicpro", chunk[:used], 50)[0] and got == nb
        chunk = b"r\tc\t10\t+\tc\t20\t-\nr\tc\t1\t+\n"
        buf[:len(chunk)] = chunk
        used, nl, nb, err = cv.feed(pin, len(chunk), True)
        assert (nl, err) == (1, (5, "fewer than 7 fields"))
        t = cv.timing()
        assert set(t) == {"h2d", "feed", "render", "d2h"}
    finally:
        cv.close()
        lib.cl_host_free(ctypes.c_void_p(pin))


def test_gz_input_same_as_plain(tmp_path):
    data = C.gen_hicpro(50000, 21)
    want = C.brute("hicpro", data, 50)[0]
    plain = _write(tmp_path / "p_allValidPairs", data)
    gz = str(tmp_path / "g_allValidPairs.gz")
    with gzip.open(gz, "wb", compresslevel=1) as fh:
        fh.write(data)
    for f in (plain, gz):
        assert _conv("hicpro", f, str(tmp_path / "o.gz"), 50, 1 << 20) == (50000, len(want))
        assert _read_out(tmp_path / "o.gz") == want


def test_synthetics_and_determinism(tmp_path):
    """both seeded synthetics (about 5e6 lines) match the sha256 of the reference's output; two runs give identical bytes"""
    for s in C.golden_meta()["synth"]:
        data = C.GEN[s["format"]](s["n"], s["seed"])
        assert hashlib.sha256(data).hexdigest() == s["in_sha256"]
        f = _write(tmp_path / ("%s_allValidPairs" % s["name"]), data)
        del data
        outs = []
        for rep in range(2):
            out = str(tmp_path / ("%s_%d%s" % (s["name"], rep, ".bedpe.gz" if s["format"] == "hicpro" else ".bedpe")))
            nl, nb = _conv(s["format"], f, out, s["ext"])
            text = _read_out(out)
            assert nl == s["lines"] and len(text) == nb and hashlib.sha256(text).hexdigest() == s["sha256"], s["name"]
            outs.append(open(out, "rb").read())
        assert outs[0] == outs[1]
        os.remove(f)


def test_between_sweep_steps(tmp_path):
    """a conversion between two sweep steps of a resident chromosome on the same device leaves the steps' results unchanged"""
    from cloops_amd import api
    X, Y = G.chr21_xy()
    data = C.gen_hicpro(100000, 5)
    f = _write(tmp_path / "s_allValidPairs", data)

    def sweep(with_k15):
        ch = api.Chromosome(X, Y)
        ch.set_device_labels(False)
        ch.cand_reset()
        out = []
        for step, (eps, cut) in enumerate(((1000, 0), (2000, 4601), (2000, 13532))):
            ch.step_async("v2", eps, 5, cut, step)
            ch.wait()
            ni, ns, st = ch.step_result()
            out.append((ni, ns, st["n_all"], st["sumx"], st["loghist"].tolist()))
            if with_k15:
                _conv("hicpro", f, str(tmp_path / "s.bedpe.gz"), 50, 1 << 20)
        out.append(ch.cand_finish(4601, 100000).tolist())
        ch.close()
        return out
    assert sweep(True) == sweep(False)


def test_command_lines_on_goldens(tmp_path):
    meta = C.golden_meta()
    d = tmp_path / "hp"
    d.mkdir()
    ok = [g for g in meta["cases"] if g["format"] == "hicpro" and g["error"] is None]
    for g in ok:
        _write(d / ("%s_allValidPairs" % g["name"]), C.golden_case(g["name"])[0])
    o = tmp_path / "out"
    p = subprocess.run([sys.executable, "-m", "cloops_amd.convert", "hicpro", str(d), "-o", str(o), "-ext", "50", "-p", "4"],
                       env=_env(), cwd=str(tmp_path), timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    for g in ok:
        got = _read_out(o / ("%s.bedpe.gz" % g["name"]))
        want = C.golden_case(g["name"])[1]
        assert (got == want) == (g["ext"] == 50), g["name"]                     # the command line's -ext applies to all
    for g in meta["cases"]:
        data, want = C.golden_case(g["name"])
        if g["format"] == "hicpro":
            f = _write(tmp_path / ("%s_allValidPairs" % g["name"]), data)
            cmd = ["hicpro", f, "-ext", str(g["ext"])]
            out = tmp_path / ("%s.bedpe.gz" % g["name"])
        else:
            if g["ext"] != 75:                                                  # the juicer script has no -ext
                continue
            f = _write(tmp_path / ("%s.txt" % g["name"]), data)
            out = tmp_path / ("%s.bedpe" % g["name"])
            cmd = ["juicer", "-i", f, "-o", str(out)]
        p = subprocess.run([sys.executable, "-m", "cloops_amd.convert"] + cmd, env=_env(), cwd=str(tmp_path), timeout=300,
                           capture_output=True, text=True)
        assert p.returncode == (0 if g["error"] is None else 1), (g["name"], p.stderr)
        if g["error"] is not None:
            assert "%s:%d: " % (f, g["lines"] + 1) in p.stderr
        assert _read_out(out) == want, g["name"]


def test_end_to_end_chr21(tmp_path):
    """a HiC-Pro pairs file made from the chr21 example, converted and run through `python -m cloops_amd -f ... -m 1 -s`: the
    PETs of the run are those cio.parse_bedpe reads from the expected text"""
    from cloops_amd import io as cio
    bed = G.write_example_bedpe(tmp_path)
    with gzip.open(bed, "rb") as fh:
        rows = [l.split(b"\t") for l in fh.read().split(b"\n") if l]
    pairs = b"".join(b"\t".join([r[6], r[0], r[1], r[8], r[3], r[4], r[9], b"HIC_x", b"HIC_y"]) + b"\n" for r in rows)
    f = _write(tmp_path / "chr21_allValidPairs", pairs)
    want = C.brute("hicpro", pairs, 50)[0]
    exp = _write(tmp_path / "expected.bedpe", want)
    p = subprocess.run([sys.executable, "-m", "cloops_amd.convert", "hicpro", f, "-o", str(tmp_path / "conv")], env=_env(),
                       cwd=str(tmp_path), timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    conv = str(tmp_path / "conv" / "chr21.bedpe.gz")
    assert _read_out(conv) == want
    run = str(tmp_path / "run")
    p = subprocess.run([sys.executable, "-m", "cloops_amd", "-f", conv, "-o", run, "-m", "1", "-s"], env=_env(), cwd=str(tmp_path),
                       timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    mats = cio.parse_bedpe([exp])[0]
    got = joblib.load(os.path.join(run, "chr21-chr21.jd"))
    assert len(mats["chr21"]) == len(rows)
    assert np.array_equal(np.asarray(got), mats["chr21"])
