"""Seeded inputs and a plain reference for the interval counts of the significance step (K8, cl_sig_counts) and of the
re-quantification (K11, cl_quant_counts) at their edges (no GPU needed).

K8 counts, per record of 22 windows (A_0..A_10, B_0..B_10; both ends inclusive), the PETs of S(W) = {X in W} | {Y in W}: |S(A_k)|,
|S(B_l)|, all |S(A_k) & S(B_l)|, the directed rab = |{X in A_0} & {Y in B_0}| and the PETs N that pass the cut.  The kernel finds
the PETs of a side as two slices of an X-sorted and a Y-sorted table (bound searches over the *hull* of the side's 11 windows),
walks them with a stride of TPB threads, drops from the Y slice the PETs whose X lies in the hull, and bumps LDS counters.  The
families, each a `Case` (X, Y, windows [R, 44] = lo[22] then hi[22], two cuts, the facts it is built for):

  stride_slices      six records whose A hull and B hull hold exactly s PETs by X and s other PETs by Y, s = 0, 1, TPB - 1, TPB,
                     TPB + 1, 2 TPB + 1: every slice length around the stride; the partner ends lie outside every window
  on_the_bounds      22 disjoint windows with PET ends exactly on lo, hi, lo - 1 and hi + 1 of each (as X and as Y)
  hull_with_holes    hand-written windows, disjoint inside the hull and not in ascending order: X in a hole and Y in a window of the
                     same side, both ends in different windows of a side, X == Y
  directed           X in A_0 & Y in B_0 and as many the other way round -- as reversed rows and, in a second record with A above B,
                     as forward rows: rab counts one kind, the intersection both
  overlapping_sides  A == B, B inside A, A and B half overlapping, B below A
  extremes           coordinates +-(2^29 - 1), 0, -1 with reversed rows; windows at the ends of int32 and of the coordinate domain,
                     inverted windows (all of a side, window 0 only, the shifted ones only), windows clamped to [0, 0]
  pile_up            70 000 PETs, 66 000 of them with both ends in one window that is A_3 and B_7: counts above 2^16 on one counter
  duplicates         300 distinct PETs repeated 1 .. 40 times, windows on their coordinates
  many_records       5000 records of cModel._windows over 2000 PETs (clamped, empty and distance-0 ones among them)
  tiny_1, tiny_2     one and two PETs

`mask_counts` restates the counts with boolean masks (no sorting, no searches); tests/test_sig_cases.py checks it against the set
model of fake_backend and the reference's own functions and proves the stated facts, tests/test_gpu_sig_counts.py and
tests/test_gpu_quant.py run the cases on the GPU."""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "name X Y windows cuts info")

TPB = 256                       # cl_common.h: the stride of k8_counts / k11_quant over a slice
SIG_W = 11                      # cl_chrom.h
SIG_OUT = 2 * SIG_W + 1 + SIG_W * SIG_W
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
CMAX = (1 << 29) - 1            # api._as_i32: |X|, |Y| < 2^29
BIAS = 1 << 30                  # k8_split: the sort keys are coordinate + 2^30
CUT_ALL = 1 << 30               # Y - X <= 2^30 - 2: no row passes
STRIDE_SIZES = (0, 1, TPB - 1, TPB, TPB + 1, 2 * TPB + 1)


def mask_counts(X, Y, windows, cut=0):
    """(int32 [R, 144], N) of cl_sig_counts from boolean masks in int64: [0..21] |S(W_k)|, [22] |{X in A_0} & {Y in B_0}|,
    [23 + 11 k + l] |S(A_k) & S(B_l)|; rows with Y - X < cut dropped when cut > 0."""
    X = np.asarray(X, np.int64).ravel()
    Y = np.asarray(Y, np.int64).ravel()
    if cut > 0:
        keep = (Y - X) >= cut
        X, Y = X[keep], Y[keep]
    w = np.asarray(windows, np.int64).reshape(-1, 4 * SIG_W)
    out = np.zeros((len(w), SIG_OUT), np.int32)
    for r in range(len(w)):
        lo, hi = w[r, :2 * SIG_W], w[r, 2 * SIG_W:]
        inX = (X[:, None] >= lo) & (X[:, None] <= hi)
        inY = (Y[:, None] >= lo) & (Y[:, None] <= hi)
        S = inX | inY
        out[r, :2 * SIG_W] = S.sum(0)
        out[r, 2 * SIG_W] = np.count_nonzero(inX[:, 0] & inY[:, SIG_W])
        S = S[S.any(1)].astype(np.int64)                 # the rows in no window add nothing to the products
        out[r, 2 * SIG_W + 1:] = (S[:, :SIG_W].T @ S[:, SIG_W:]).reshape(-1)
    return out, len(X)


def row(A, B):
    """the 44 ints of one record from 11 + 11 (lo, hi) pairs"""
    assert len(A) == SIG_W and len(B) == SIG_W
    return [a for a, _ in A] + [b for b, _ in B] + [a for _, a in A] + [b for _, b in B]


def split(table):
    """[R, 144] -> (c_a [R, 11], c_b [R, 11], rab [R], c_ab [R, 11, 11])"""
    t = np.asarray(table)
    return t[:, :SIG_W], t[:, SIG_W:2 * SIG_W], t[:, 2 * SIG_W], t[:, 2 * SIG_W + 1:].reshape(-1, SIG_W, SIG_W)


def hulls(windows):
    """[R, 44] -> (lo [R, 2], hi [R, 2]): smallest lo and largest hi of the A and of the B windows, as the kernel takes them"""
    w = np.asarray(windows, np.int64).reshape(-1, 4 * SIG_W)
    lo, hi = w[:, :2 * SIG_W].reshape(-1, 2, SIG_W), w[:, 2 * SIG_W:].reshape(-1, 2, SIG_W)
    return lo.min(2), hi.max(2)


def _windows_of(recs):
    from cloops_amd import cModel
    return cModel._windows([["c", a, b, "c", c, d] for a, b, c, d in recs])[3]


def _case(name, X, Y, windows, cuts, **info):
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    w = np.asarray(windows, np.int64).reshape(-1, 4 * SIG_W)
    assert X.shape == Y.shape and X.ndim == 1
    assert len(X) == 0 or max(np.abs(X).max(), np.abs(Y).max()) <= CMAX
    assert w.min() >= I32_MIN and w.max() <= I32_MAX
    w = w.astype(np.int32)
    for a in (X, Y, w):
        a.setflags(write=False)
    return Case(name, X, Y, w, tuple(cuts), info)


def _shuffled(rng, X, Y):
    p = rng.permutation(len(X))
    return np.asarray(X, np.int64)[p], np.asarray(Y, np.int64)[p]


def stride_slices(seed=8101):
    """record q: the A hull and the B hull each hold STRIDE_SIZES[q] PETs by X and as many others by Y"""
    rng = np.random.default_rng(seed)
    X, Y, rows = [], [], []
    for q, s in enumerate(STRIDE_SIZES):
        sides = []
        for side in (0, 1):
            base = 1000000 + (2 * q + side) * 100000
            wins = [(base + 900 * k, base + 900 * k + 799) for k in range(SIG_W)]          # hull [base, base + 9799], holes of 100
            sides.append(wins[4:] + wins[:4])                                              # window 0 is not the lowest
            for end in (0, 1):
                c = rng.integers(base, base + 9800, s)
                far = rng.random(s) < 0.5
                gap = np.where(far, 150000000, 40000000) + rng.integers(0, 1000000, s)     # the partner: far outside every window
                X.append(c if end == 0 else c - gap)
                Y.append(c + gap if end == 0 else c)
        rows.append(row(*sides))
    bx = rng.integers(3000000, 4000000, 300)                                               # background: in no window
    X.append(bx)
    Y.append(bx + rng.integers(0, 200000000, 300))
    X, Y = _shuffled(rng, np.concatenate(X), np.concatenate(Y))
    return _case("stride_slices", X, Y, rows, (100000000, CUT_ALL), sizes=STRIDE_SIZES)


def on_the_bounds(seed=8102):
    """record 0: 22 disjoint windows; per window a PET with X (and one with Y) on lo, hi, lo - 1, hi + 1, the partner far away; per k
    the PETs (A_k.lo, B_k.hi), (A_k.hi + 1, B_k.lo) and (B_k.hi, A_k.lo).  Hence at cut 0: |S(A_k)| = 6, |S(B_k)| = 7, rab = 1,
    |S(A_k) & S(B_l)| = 2 for k == l and 0 otherwise.  Record 1: the one-point windows [lo, lo] / [hi, hi]; record 2: every window
    one wider on both sides."""
    rng = np.random.default_rng(seed)
    slot = rng.permutation(2 * SIG_W)
    wins = [(10000 * (int(s) + 1), 10000 * (int(s) + 1) + 1000 + int(s)) for s in slot]
    A, B = wins[:SIG_W], wins[SIG_W:]
    X, Y = [], []
    for i, (lo, hi) in enumerate(wins):
        for j, v in enumerate((lo, hi, lo - 1, hi + 1)):
            X += [v, -5000000 - 4 * i - j]
            Y += [5000000 + 4 * i + j, v]
    for k in range(SIG_W):
        X += [A[k][0], A[k][1] + 1, B[k][1]]
        Y += [B[k][1], B[k][0], A[k][0]]
    rows = [row(A, B), row([(lo, lo) for lo, _ in A], [(hi, hi) for _, hi in B]),
            row([(lo - 1, hi + 1) for lo, hi in A], [(lo - 1, hi + 1) for lo, hi in B])]
    X, Y = _shuffled(rng, X, Y)
    return _case("on_the_bounds", X, Y, rows, (1000000, CUT_ALL))


def hull_with_holes(seed=8103):
    """windows of 100 with holes of 100 between them, in the orders (5 + 4 k) % 11 and (3 + 7 k) % 11"""
    rng = np.random.default_rng(seed)
    m = 40
    win = lambda base, k: (base + 200 * k, base + 200 * k + 99)
    hole = lambda base, k: (base + 200 * k + 100, base + 200 * k + 199)
    a0, b0 = 1000, 10000
    A = [win(a0, (5 + 4 * k) % SIG_W) for k in range(SIG_W)]
    B = [win(b0, (3 + 7 * k) % SIG_W) for k in range(SIG_W)]
    inside = lambda iv: rng.integers(iv[0], iv[1] + 1)
    in_win = lambda base: inside(win(base, rng.integers(0, SIG_W)))
    in_hole = lambda base: inside(hole(base, rng.integers(0, SIG_W - 1)))

    def two_windows(base):
        i, j = rng.choice(SIG_W, 2, replace=False)
        return inside(win(base, i)), inside(win(base, j))
    groups = {"hole_a_win_a": lambda: (in_hole(a0), in_win(a0)), "hole_b_win_b": lambda: (in_hole(b0), in_win(b0)),
              "win_a_win_a": lambda: two_windows(a0), "win_b_win_b": lambda: two_windows(b0),
              "same_point_a": lambda: (in_win(a0),) * 2, "same_point_b": lambda: (in_win(b0),) * 2,
              "hole_a_win_b": lambda: (in_hole(a0), in_win(b0)), "win_a_hole_b": lambda: (in_win(a0), in_hole(b0)),
              "hole_b_win_a": lambda: (in_hole(b0), in_win(a0)), "hole_a_hole_a": lambda: (in_hole(a0), in_hole(a0)),
              "below_win_a": lambda: (rng.integers(0, 900), in_win(a0)), "win_b_above": lambda: (in_win(b0), rng.integers(13000, 20000))}
    X, Y, group = [], [], []
    for g, (name, draw) in enumerate(groups.items()):
        for _ in range(m):
            x, y = draw()
            X.append(int(x)), Y.append(int(y)), group.append(g)
    bx = rng.integers(20000, 40000, 200)
    X, Y = np.concatenate([X, bx]), np.concatenate([Y, bx + rng.integers(0, 5000, 200)])
    group = np.concatenate([group, np.full(200, -1)])
    p = rng.permutation(len(X))
    rows = [row(A, B), row(B, A), row(sorted(A), sorted(B))]
    return _case("hull_with_holes", X[p], Y[p], rows, (500, CUT_ALL), group=group[p], groups=tuple(groups), m=m)


def directed(seed=8104):
    """record 0: A_0 = [1000, 1999] below B_0 = [5000, 5999]; 37 PETs (X in A_0, Y in B_0) and 37 stored the other way round (rows
    with Y < X).  Record 1: A_0 = [25000, 25999] ABOVE B_0 = [21000, 21999]; 37 rows (X in A_0, Y in B_0: reversed rows) and 37
    forward rows (X in B_0, Y in A_0).  The shifted windows move by 300.  PETs with one end in an anchor only, and a far background."""
    rng = np.random.default_rng(seed)
    m = 37
    shifted = lambda lo, hi: [(lo, hi)] + [(lo + 300 * i, hi + 300 * i) for i in range(-5, 6) if i]
    X, Y, rows = [], [], []
    for a, b in ((1000, 5000), (25000, 21000)):
        rows.append(row(shifted(a, a + 999), shifted(b, b + 999)))
        X += [rng.integers(a, a + 1000, m), rng.integers(b, b + 1000, m)]          # X in A_0 & Y in B_0; X in B_0 & Y in A_0
        Y += [rng.integers(b, b + 1000, m), rng.integers(a, a + 1000, m)]
        X += [rng.integers(a, a + 1000, 25), rng.integers(100000, 200000, 25)]     # one end in an anchor, the other in no window
        Y += [rng.integers(100000, 200000, 25), rng.integers(b, b + 1000, 25)]
    bx = rng.integers(50000, 90000, 300)
    X.append(bx)
    Y.append(bx + rng.integers(-3000, 3000, 300))
    X, Y = _shuffled(rng, np.concatenate(X), np.concatenate(Y))
    return _case("directed", X, Y, rows, (1, CUT_ALL), m=m)


def overlapping_sides(seed=8105):
    """A == B, B inside A, A and B half overlapping, B below A and overlapping it; positive coordinates, some reversed rows"""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 15000, 600)
    Y = np.maximum(0, X + rng.integers(-500, 4000, 600))
    recs = [(5000, 7000, 5000, 7000), (4000, 9000, 5000, 6000), (4000, 7000, 5500, 8500), (9000, 12000, 3000, 10000)]
    return _case("overlapping_sides", X, Y, _windows_of(recs), (1000, CUT_ALL), records=recs)


EXTREME_CLAMPED = (2, 10, 30, 60)        # ca = 6, sa = 4, sb = 15, step = 9: the A windows of i = -5 .. -2 collapse to [0, 0]


def extremes(seed=8106):
    """every pair of the coordinates {+-CMAX, +-(CMAX - 1), 0, +-1, 5, 7, +-1000} as a PET (reversed rows and X == Y among them)
    plus 200 random PETs over the whole domain.  Records: 0 the ends of int32 and of the domain; 1 a side whose hull ends at
    INT32_MAX and one whose hull starts at INT32_MIN; 2 all A windows inverted (their hull [1000, 1090] is not empty); 3 window 0
    of both sides inverted; 4 only the shifted windows inverted; 5 cModel._windows of an anchor next to 0."""
    rng = np.random.default_rng(seed)
    pool = [-CMAX, -CMAX + 1, -1000, -1, 0, 1, 5, 7, 1000, CMAX - 1, CMAX]
    X = np.concatenate([np.repeat(pool, len(pool)), rng.integers(-CMAX, CMAX + 1, 200)])
    Y = np.concatenate([np.tile(pool, len(pool)), rng.integers(-CMAX, CMAX + 1, 200)])
    M = CMAX
    small = lambda base: [(base + 3 * k, base + 3 * k + 4) for k in range(SIG_W)]
    r0 = row([(I32_MIN, I32_MAX), (-BIAS - 1, -BIAS - 1), (M, M), (-M, -M), (0, 0), (-1, 0), (I32_MIN, I32_MIN), (-M - 1, -M - 1),
              (M - 1, M - 1), (-BIAS, -M), (1, 7)],
             [(-BIAS, -BIAS + 1), (M, I32_MAX), (-M, -M), (M, M), (-1, -1), (I32_MIN, -M), (I32_MAX, I32_MAX), (M + 1, M + 1),
              (-M + 1, -M + 1), (M, BIAS), (I32_MIN, I32_MAX)])
    r1 = row([(M, I32_MAX)] + [(M - 1 + k, I32_MAX - k) for k in range(1, SIG_W)],
             [(I32_MIN, -M)] + [(I32_MIN + k, -M + 1 - k % 2) for k in range(1, SIG_W)])
    r2 = row([(1000 + 10 * k, 990 + 10 * k) for k in range(SIG_W)], small(-10))
    r3 = row([(7, 0)] + small(-10)[1:], [(CMAX, -CMAX)] + small(990)[1:])
    r4 = row([(-1, 7)] + [(1000 + k, -1000 - k) for k in range(1, SIG_W)], [(-CMAX, 0)] + [(5, 4 - k) for k in range(1, SIG_W)])
    r5 = _windows_of([EXTREME_CLAMPED])[0].tolist()
    inverted = {2: list(range(SIG_W)), 3: [0, SIG_W], 4: [k for k in range(1, 2 * SIG_W) if k != SIG_W]}
    X, Y = _shuffled(rng, X, Y)
    return _case("extremes", X, Y, [r0, r1, r2, r3, r4, r5], (1, CUT_ALL), inverted=inverted, clamped_record=5)


PILE = (1000000, 1099999)


def pile_up(seed=8107):
    """66 000 PETs with both ends in PILE = A_3 = B_7 of record 0 (windows of 100 000 side by side), 4000 PETs around; two records
    of cModel._windows"""
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.integers(PILE[0], PILE[1] + 1, 66000), rng.integers(0, 2000000, 4000)])
    Y = np.concatenate([rng.integers(PILE[0], PILE[1] + 1, 66000), rng.integers(0, 2000000, 4000)])
    tile = lambda base: [(base + 100000 * k, base + 100000 * k + 99999) for k in range(SIG_W)]
    A, B = tile(PILE[0] - 300000), tile(PILE[0] - 700000)
    assert A[3] == PILE and B[7] == PILE
    rows = [row(A, B)] + _windows_of([(500000, 520000, 900000, 930000), (1050000, 1060000, 1200000, 1250000)]).tolist()
    X, Y = _shuffled(rng, X, Y)
    return _case("pile_up", X, Y, rows, (1, CUT_ALL), pile=(0, 3, 7))


def duplicates(seed=8108):
    """300 distinct PETs, PET i repeated 1 .. 40 times; every window bound of the 8 records is a coordinate of a PET"""
    rng = np.random.default_rng(seed)
    x = rng.choice(5000, 300, replace=False)
    y = x + rng.integers(-200, 3000, 300)
    reps = rng.integers(1, 41, 300)
    X, Y = _shuffled(rng, np.repeat(x, reps), np.repeat(y, reps))
    pool = np.concatenate([x, y])
    rows = []
    for _ in range(8):
        ab = np.sort(rng.choice(pool, (2 * SIG_W, 2)), 1)
        rows.append(ab[:, 0].tolist() + ab[:, 1].tolist())
    return _case("duplicates", X, Y, rows, (1000, CUT_ALL), distinct=300)


MANY = 5000


def many_records(seed=8109):
    """2000 PETs (20 blobs and a background, forward rows, positive coordinates: every clustering variant takes them) and 5000
    records of cModel._windows: anchors next to 0 (windows clamped), beyond the data (empty), and B == A (distance 0)"""
    rng = np.random.default_rng(seed)
    cx = rng.integers(5000, 200000, 20)
    cy = cx + rng.integers(8000, 60000, 20)
    X = np.concatenate([np.repeat(cx, 50) + rng.integers(-400, 400, 1000), rng.integers(0, 200000, 1000)])
    Y = np.concatenate([np.repeat(cy, 50) + rng.integers(-400, 400, 1000), np.zeros(1000, np.int64)])
    Y[1000:] = X[1000:] + rng.integers(0, 60000, 1000)
    a0 = rng.integers(0, 260000, MANY)
    a0[::10] = rng.integers(0, 50, len(a0[::10]))                        # next to 0
    a0[5::10] = rng.integers(400000, 500000, len(a0[5::10]))             # beyond every PET
    a1 = a0 + rng.integers(0, 3000, MANY)
    b0 = a0 + rng.integers(0, 50000, MANY)
    b1 = b0 + rng.integers(0, 3000, MANY)
    b0[3::10], b1[3::10] = a0[3::10], a1[3::10]                          # distance 0
    recs = np.stack([a0, a1, b0, b1], 1)
    p = rng.permutation(MANY)                                            # every kind among the first records as well
    X, Y = _shuffled(rng, X, Y)
    return _case("many_records", X, Y, _windows_of(recs[p].tolist()), (20000, CUT_ALL), records=recs[p], prefixes=(3, 2))


def tiny(n):
    """one or two PETs (the second a reversed row) against two records; a cut of 15 keeps the first PET only"""
    X, Y = np.array([10, 25], np.int64)[:n], np.array([30, 5], np.int64)[:n]
    return _case("tiny_%d" % n, X, Y, _windows_of([(0, 20, 25, 40), (50, 60, 70, 90)]), (15, CUT_ALL))


BUILDERS = (stride_slices, on_the_bounds, hull_with_holes, directed, overlapping_sides, extremes, pile_up, duplicates, many_records,
            functools.partial(tiny, 1), functools.partial(tiny, 2))
NAMES = ("stride_slices", "on_the_bounds", "hull_with_holes", "directed", "overlapping_sides", "extremes", "pile_up", "duplicates",
         "many_records", "tiny_1", "tiny_2")
QUANT_NAMES = ("extremes", "directed", "hull_with_holes", "stride_slices")          # the cases K11 runs as well


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[NAMES.index(name)]()
    assert c.name == name
    return c


def cuts_of(c):
    """0, a cut that keeps part of the rows (all of them where there is one row only), a cut that keeps none"""
    return (0,) + c.cuts


@functools.lru_cache(maxsize=None)
def reference(name, cut):
    """(table [R, 144], N) of mask_counts for a case and a cut: computed once, read-only, shared by the tests"""
    c = case(name)
    table, n = mask_counts(c.X, c.Y, c.windows, cut)
    table.setflags(write=False)
    return table, n
