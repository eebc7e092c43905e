"""GPU: who frees what on a chromosome handle.  Every analysis unit with a public free (K14 tracks, K20 coverage, K21 peaks, K22
domains, K23 k-distances, K24 cells, K25 weights, K26 diagonals) is built, read, freed, refused and built again on one small handle:
the second build must give the bytes of the first.  Then the chain K24 -> K25 -> K26 (a free or a rebuild drops what depends on it
and nothing else), and handles created, filled by every unit and destroyed over and over."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 3000
RES = 10000


def rows():
    rng = np.random.default_rng(21)
    x = rng.integers(0, 400000, N)
    return x, x + rng.integers(0, 60000, N)


def chrom():
    from cloops_amd import api
    x, y = rows()
    return api.Chromosome(np.asarray(x, np.int64), np.asarray(y, np.int64))


@pytest.fixture(scope="module")
def ch():
    h = chrom()
    yield h
    h.close()


def blob(*arrays):
    return tuple(np.asarray(a).tobytes() for a in arrays)


def cells(ch, res=RES):
    assert ch.mat_cells(res, 0, True)[1] == N
    return blob(*ch.mat_cells_get())


def weights(ch):
    b0, nb, used = ch.bal_marginals(0)
    it = ch.bal_iterate(np.ones(nb, np.uint32), 20, 1e-3)
    return blob(*ch.bal_marginals_get(), ch.bal_weights(), ch.bal_cells_get()) + ((b0, nb, used), it)


def diagonals(ch):
    nd, used = ch.exp_diagonals()
    p, c, v = ch.exp_diagonals_get()
    ch.exp_set(np.where(p > 0, v / np.maximum(p, 1), np.nan))
    return blob(p, c, v, ch.exp_cells_get()) + ((nd, used),)


# ---- per unit: (what it needs first, build and read, free, a getter and the words of its refusal) -----------------------------
def track(ch):
    nr, nb = ch.track_build("washu", 0, 75, None, "c", "c")
    text = b"".join(bytes(m) for m in ch.track_iter(1 << 16))
    assert nr == 2 * N and len(text) == nb
    return text


def coverage(ch):
    runs = ch.coverage_build(0, 3, 75, 0)
    nb = ch.coverage_text("c")
    text = b"".join(bytes(m) for m in ch.coverage_iter(1 << 16))
    assert runs[0] > 0 and len(text) == nb
    return blob(*ch.coverage_runs()) + (text, runs)


def peaks(ch):
    assert ch.peaks_sort()[0] == 2 * N
    called = ch.peaks_call(500, 5)
    got = ch.peaks_get()
    assert called[0] > 0 and len(got[0]) == called[0]
    return blob(*got, ch.peaks_count([0, 100000], [1 << 30, 200000])) + (called,)


def domains(ch):
    made = ch.domains_tracks(0, RES, 5)
    got = ch.domains_get()
    assert made[2] == N and len(got[0]) == made[0]
    return blob(*got, *ch.domains_count([0, 100000], [100000, 1 << 30])) + (made,)


def kdis(ch):
    assert ch.kdis_build([4, 9]) == N
    hist, nz, nn = ch.kdis_hist(1)
    return blob(*ch.kdis_get(0), *ch.kdis_get(1), hist) + ((nz, nn),)


UNITS = {
    "track": (None, track, lambda ch: ch.track_free(), lambda ch: ch.track_chunks(), "no track built on this handle"),
    "coverage": (None, coverage, lambda ch: ch.coverage_free(), lambda ch: ch.coverage_runs(), "no coverage built on this handle"),
    "peaks": (None, peaks, lambda ch: ch.peaks_free(), lambda ch: ch.peaks_get(), "no peaks called on this handle"),
    "domains": (None, domains, lambda ch: ch.domains_free(), lambda ch: ch.domains_get(), "no tracks on this handle"),
    "kdis": (None, kdis, lambda ch: ch.kdis_free(), lambda ch: ch.kdis_get(), "no k-distances on this handle"),
    "mat": (None, cells, lambda ch: ch.mat_free(), lambda ch: ch.mat_cells_get(), "no cells on this handle"),
    "bal": (cells, weights, lambda ch: ch.bal_free(), lambda ch: ch.bal_marginals_get(), "no marginals on this handle"),
    "exp": (lambda ch: (cells(ch), weights(ch)), diagonals, lambda ch: ch.exp_free(), lambda ch: ch.exp_diagonals_get(),
            "no diagonals on this handle"),
}


def refused(call, words):
    from cloops_amd import _lib
    with pytest.raises(_lib.CloopsHipError, match=words):
        call()


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_free_refuse_rebuild(ch, unit):
    before, build, free, getter, words = UNITS[unit]
    if before:
        before(ch)
    first = build(ch)
    free(ch)
    refused(lambda: getter(ch), words)
    free(ch)                                                                # (a second free of nothing is no error)
    refused(lambda: getter(ch), words)
    assert build(ch) == first


def test_bal_free_keeps_the_cells_and_drops_the_diagonals(ch):
    c, w = cells(ch), weights(ch)
    diagonals(ch)
    ch.bal_free()
    refused(ch.bal_marginals_get, "no marginals on this handle")
    refused(ch.exp_diagonals_get, "no marginals on this handle")
    assert blob(*ch.mat_cells_get()) == c
    assert weights(ch) == w
    refused(ch.exp_diagonals_get, "no diagonals on this handle")            # (K26's state did not come back with the marginals)


def test_exp_free_keeps_cells_and_weights(ch):
    c, w = cells(ch), weights(ch)
    d = diagonals(ch)
    ch.exp_free()
    refused(ch.exp_diagonals_get, "no diagonals on this handle")
    assert blob(*ch.mat_cells_get()) == c
    assert blob(*ch.bal_marginals_get(), ch.bal_weights(), ch.bal_cells_get()) == w[:4]
    assert diagonals(ch) == d


def all_dropped(ch, c):
    """the cells are `c`; of K25 and K26 nothing is left"""
    assert blob(*ch.mat_cells_get()) == c
    refused(ch.bal_marginals_get, "no marginals on this handle")
    ch.bal_marginals(0)
    refused(ch.bal_weights, "no weights on this handle")
    ch.bal_iterate(np.ones(ch._bal_bins, np.uint32), 20, 1e-3)
    refused(ch.exp_diagonals_get, "no diagonals on this handle")


def test_mat_free_drops_all_three(ch):
    c, w = cells(ch), weights(ch)
    d = diagonals(ch)
    ch.mat_free()
    refused(ch.mat_cells_get, "no cells on this handle")
    refused(ch.bal_marginals_get, "no cells on this handle")
    refused(ch.exp_diagonals_get, "no marginals on this handle")
    all_dropped(ch, cells(ch))
    assert (cells(ch), weights(ch), diagonals(ch)) == (c, w, d)


def test_cells_at_another_resolution_drop_weights_and_diagonals(ch):
    c, w = cells(ch), weights(ch)
    d = diagonals(ch)
    other = cells(ch, RES // 2)
    assert other != c
    all_dropped(ch, other)
    assert (cells(ch), weights(ch), diagonals(ch)) == (c, w, d)


def test_twenty_handles_filled_and_destroyed():
    x, y = rows()
    first = None
    for _ in range(20):
        h = chrom()
        got = (track(h), coverage(h), peaks(h), domains(h), kdis(h), cells(h), weights(h), diagonals(h))
        assert h.contact_hist(RES)[2] == N and h.anchor_mask([0], [1 << 29])[2] == N
        assert h.agg_loops(np.array([100000]), np.array([150000]), 5000, w=2, corner=1)[3] == N
        h.close()
        first = first or got
        assert got == first
