"""GPU: the text writer that K14 (tracks), K20 (coverage) and K15 (converter) share (cloops_amd/csrc/cl_textout.h) at the edges of
its render tiles, the double-buffered iterator when its consumer walks away, and the handle's destruction after every analysis unit
has left buffers on it.  Expected bytes come from the host: coverage lines formatted from coverage_runs, the brute-force renderers
of test_tracks.py and convert_cases.py.

Already pinned elsewhere and not repeated: juice tracks of K14_T and K14_T + 1 records and washU tracks of K14_T and K14_T + 2 at
the default budget (test_gpu_tracks.py::test_edges, n = 128, 129, 256, 257)."""
import ctypes

import numpy as np
import pytest

import convert_cases as C
from test_tracks import brute_text

pytestmark = pytest.mark.gpu

K14_T = 256          # k_track.hip K14_T: lines per render tile
K20_T = 256          # k_cover.hip K20_T
K15_T = 256          # k_convert.hip K15_T
K15_LDS = 40 * 1024  # k_convert.hip K15_LDS: the widest output span a converter tile stages in LDS
NAME_MAX = 64        # CL_TRACK_NAME_MAX


def chrom(X, Y):
    from cloops_amd import api
    return api.Chromosome(np.asarray(X, np.int64), np.asarray(Y, np.int64))


def cov_lines(name, runs):
    return ["%s\t%d\t%d\t%d\n" % (name, s, e, d) for s, e, d in zip(*[a.tolist() for a in runs])]


def isolated_runs(ch_of, R):
    """a handle whose coverage (ends = 1, ext = 1) is exactly R runs [3 k, 3 k + 2) of depth 1: lines of 8 to 14 bytes"""
    X = 3 * np.arange(R, dtype=np.int64) + 1
    ch = ch_of(X, X + 1000000)
    assert ch.coverage_build(0, 1, 1, 0)[0] == R
    return ch


@pytest.mark.parametrize("R", [1, K20_T - 1, K20_T, K20_T + 1, 2 * K20_T + 1])
def test_coverage_text_at_render_tile_edges(R):
    """a one-byte name: a last tile of one line lies inside one or two 16-byte words of the output, so the flush writes it byte by
    byte.  At the smallest budget every chunk is one line (every alignment of a span in its words); at the default one chunk holds
    all tiles."""
    ch = isolated_runs(chrom, R)
    lines = cov_lines("c", ch.coverage_runs())
    want = "".join(lines).encode()
    assert len(lines) == R and 8 <= min(map(len, lines)) and max(map(len, lines)) <= 14
    assert ch.coverage_text("c") == len(want)
    smallest = 1 + 44                                                   # k20_lcap: name + 4 + 2 * 10 + 20
    with pytest.raises(Exception):
        ch.coverage_chunks(smallest - 1)
    run_b, byte_b = ch.coverage_chunks(smallest)
    assert len(run_b) - 1 == R                                          # a line per chunk
    assert [ch.coverage_render(k) for k in range(R)] == [l.encode() for l in lines]
    run_b, byte_b = ch.coverage_chunks()
    assert run_b.tolist() == [0, R] and byte_b.tolist() == [0, len(want)]
    assert ch.coverage_render(0) == want
    ch.close()


@pytest.mark.parametrize("kind,n", [("juice", K14_T), ("juice", K14_T + 1), ("washu", K14_T // 2), ("washu", K14_T // 2 + 1)])
def test_tracks_at_render_tile_edges_smallest_budget(kind, n):
    """K14_T and K14_T + 1 records (washU writes two per PET: K14_T and K14_T + 2) at the smallest budget the entry accepts: every
    chunk is one line, rendered by a tile of one line"""
    rng = np.random.default_rng(5)
    x = rng.integers(0, 100000, n)
    y = x + rng.integers(0, 100000, n)
    ids = np.arange(n, dtype=np.int64)
    ch = chrom(x, y)
    want = brute_text(kind, ("c", "c"), ids, x, y, 0, 75)
    nr, nb = ch.track_build(kind, 0, 75, ids, "c", "c")
    assert nr == (2 * n if kind == "washu" else n) and nb == len(want)
    smallest = 2 + (11 + 5 * 20 if kind == "washu" else 12 + 2 * 20)     # k14_lcap
    with pytest.raises(Exception):
        ch.track_chunks(smallest - 1)
    rec, byt = ch.track_chunks(smallest)
    assert len(rec) - 1 == nr
    parts = [ch.track_render(k) for k in range(nr)]
    assert all(p.count(b"\n") == 1 for p in parts) and b"".join(parts) == want
    ch.close()


@pytest.mark.parametrize("name_len", [220, 3])
def test_converter_direct_and_staged_tiles(name_len):
    """K15_T + 1 lines.  With read names of 220 bytes the first tile's output span exceeds K15_LDS and is written straight to global
    memory, the one-line second tile is staged in LDS and flushed; with short names both tiles are staged"""
    from cloops_amd import _lib, api
    n = K15_T + 1
    rows = [b"%s\tchr%d\t%d\t+\tchrX\t%d\t-\n" % ((b"r%04d" % k).ljust(name_len, b"q"), k % 7, 1000 + 37 * k, 900000 - 11 * k) for k in range(n)]
    data = b"".join(rows)
    want, lines, reason = C.brute("hicpro", data, 50)
    assert lines == n and reason is None
    first = len(C.brute("hicpro", b"".join(rows[:K15_T]), 50)[0])
    assert (first > K15_LDS) == (name_len == 220)
    lib = _lib.load()
    cap = 1 << 17
    assert len(data) <= cap and len(want) <= cap
    cv = api.Converter("hicpro", 50, cap)
    pin = lib.cl_host_alloc(2 * cap)
    try:
        buf = (ctypes.c_char * (2 * cap)).from_address(pin)
        buf[:len(data)] = data
        used, nl, nb, err = cv.feed(pin, len(data), True)
        assert (used, nl, nb, err) == (len(data), n, len(want), None)
        got = cv.render(pin + cap, cap)
        assert got == len(want) and bytes(buf[cap:cap + got]) == want
    finally:
        cv.close()
        lib.cl_host_free(ctypes.c_void_p(pin))


def test_iterators_abandoned_then_reused():
    """the generator is dropped after its first chunk with chunks pending (a render of the next chunk is in flight on the helper
    thread); its clean-up must wait for that render and free both buffers, and the handle must then serve a new build in full"""
    rng = np.random.default_rng(9)
    x = rng.integers(0, 3000000, 600)
    y = x + rng.integers(0, 20000, 600)
    ch = chrom(x, y)
    ids = np.arange(600, dtype=np.int64)
    for _ in range(2):
        want = brute_text("juice", ("c", "c"), ids, x, y, 0, 0)
        ch.track_build("juice", 0, 0, ids, "c", "c")
        assert len(ch.track_chunks(2000)[0]) - 1 >= 4                  # at least three chunks behind the first
        it = ch.track_iter(2000)
        head = bytes(next(it))
        assert want.startswith(head) and 0 < len(head) <= 2000
        it.close()
        ch.track_build("juice", 0, 0, ids, "c", "c")
        assert b"".join(bytes(m) for m in ch.track_iter(2000)) == want
        ch.coverage_build(0, 3, 40, 0)
        want = "".join(cov_lines("c", ch.coverage_runs())).encode()
        assert ch.coverage_text("c") == len(want)
        assert len(ch.coverage_chunks(2000)[0]) - 1 >= 4
        it = ch.coverage_iter(2000)
        head = bytes(next(it))
        assert want.startswith(head) and 0 < len(head) <= 2000
        del it                                                          # collected, not closed: the same clean-up
        ch.coverage_build(0, 3, 40, 0)
        assert ch.coverage_text("c") == len(want)
        assert b"".join(bytes(m) for m in ch.coverage_iter(2000)) == want
    ch.close()


def test_destroy_after_every_unit():
    """every analysis unit leaves its buffers on one small handle, then the handle is destroyed (each unit's own release function,
    called by the destruction); a second handle repeats it"""
    rng = np.random.default_rng(21)
    n = 3000
    x = rng.integers(0, 400000, n)
    y = x + rng.integers(0, 60000, n)
    for _ in range(2):
        ch = chrom(x, y)
        nr, nb = ch.track_build("washu", 0, 75, None, "c", "c")
        assert nr == 2 * n and len(b"".join(bytes(m) for m in ch.track_iter(1 << 16))) == nb
        runs = ch.coverage_build(0, 3, 75, 0)[0]
        nb = ch.coverage_text("c")
        assert runs > 0 and len(b"".join(bytes(m) for m in ch.coverage_iter(1 << 16))) == nb
        assert ch.peaks_sort()[0] == 2 * n
        npk = ch.peaks_call(500, 5)[0]
        assert len(ch.peaks_get()[0]) == npk
        assert int(ch.peaks_count([0], [1 << 30])[0]) == 2 * n
        bins = ch.domains_tracks(0, 10000, 5)[0]
        assert len(ch.domains_get()[0]) == bins
        assert int(ch.domains_count([0], [1 << 30])[0][0]) == n
        assert ch.kdis_build([4]) == n and len(ch.kdis_get()[2]) == n
        cells = ch.mat_cells(10000, 0, True)[0]
        assert int(ch.mat_cells_get()[2].sum()) == n
        b0, nbins, used = ch.bal_marginals(0)
        assert used == cells and len(ch.bal_marginals_get()[0]) == nbins
        ch.bal_iterate(np.ones(nbins, np.uint32), 20, 1e-3)
        assert len(ch.bal_weights()) == nbins and len(ch.bal_cells_get()) == cells
        assert ch.contact_hist(10000)[2] == n and ch.anchor_mask([0], [1 << 29])[2] == n
        assert ch.agg_loops(np.array([100000]), np.array([150000]), 5000, w=2, corner=1)[3] == n
        ch.close()
