"""CPU: the rule by which k_union_c (cloops_amd/csrc/k_lists.hip) leaves dominated cores out of the cross-strip search, restated in
plain numpy and loops, and the claim that makes it exact: the cores that survive find the same set of (chain, chain) pairs as all
cores do.

The cores of a strip lie in the core array in the order of (q, sp).  With the key (sp, index) -- a strict total order -- a core a is
dominated when a core in front of it and a core behind it, both of its strip and within eps in q, have a smaller key.  The kernel
looks at K neighbours on either side; a side without a dominator among them counts as not dominated.  A core b of strip s - 1 is a
neighbour of a core a of strip s iff |q_b - q_a| <= eps and sp_b >= sp_a - peps."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

EPS = 100
PEPS = 128                       # the strip field of sp: sp = strip * PEPS + (p mod eps)
KS = (1, 2, 4, 8, 16)


def _sorted(strip, q, r):
    """-> (q, sp, strip) in core-array order"""
    strip, q, r = (np.asarray(v, np.int64) for v in (strip, q, r))
    sp = strip * PEPS + r
    o = np.lexsort((sp, q, strip))
    return q[o], sp[o], strip[o]


def dominated(q, sp, strip, K):
    """the rule, one core at a time"""
    n = len(q)
    out = np.zeros(n, bool)
    for a in range(n):
        left = right = False
        for d in range(1, K + 1):
            b = a - d
            if b >= 0 and strip[b] == strip[a] and q[a] - q[b] <= EPS and (sp[b], b) < (sp[a], a):
                left = True
            b = a + d
            if b < n and strip[b] == strip[a] and q[b] - q[a] <= EPS and (sp[b], b) < (sp[a], a):
                right = True
        out[a] = left and right
    return out


def chain_of(q, strip):
    ch = np.zeros(len(q), np.int64)
    for i in range(1, len(q)):
        ch[i] = ch[i - 1] + (1 if strip[i] != strip[i - 1] or q[i] - q[i - 1] > EPS else 0)
    return ch


def pairs_found(q, sp, strip, who):
    ch = chain_of(q, strip)
    out = set()
    for a in np.flatnonzero(who):
        for b in np.flatnonzero((strip == strip[a] - 1) & (np.abs(q - q[a]) <= EPS) & (sp >= sp[a] - PEPS)):
            out.add((int(ch[a]), int(ch[b])))
    return out


def _random_set(seed, kind):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(40, 160))
    strip = rng.integers(0, 3, n)
    if kind == "plain":
        q = rng.integers(0, 12 * EPS, n); r = rng.integers(0, EPS, n)
    elif kind == "equal_sp":                             # a handful of remainders: most keys tie on sp, the index decides
        q = rng.integers(0, 12 * EPS, n); r = rng.choice([0, 7, 7, 7, 50, EPS - 1], n)
    elif kind == "equal_q":                              # a handful of q values: long runs of equal q, ordered by sp
        q = rng.choice(np.arange(0, 12 * EPS, EPS // 2), n); r = rng.integers(0, EPS, n)
    elif kind == "equal_both":
        q = rng.choice(np.arange(0, 12 * EPS, EPS // 2), n); r = rng.choice([0, 7, 7, 50], n)
    else:                                                # "gaps": q on a lattice whose steps are exactly eps and eps + 1, with doubles
        steps = rng.choice([0, 0, 1, EPS // 3, EPS, EPS, EPS + 1], n)
        q = np.cumsum(steps); r = rng.integers(0, EPS, n)
        strip = np.sort(strip)                           # (each strip gets a stretch of the lattice; the stretches overlap in q)
        q = q - np.where(strip > 0, q[np.searchsorted(strip, strip)], 0)
    return _sorted(strip, q, r)


KINDS = ("plain", "equal_sp", "equal_q", "equal_both", "gaps")


@pytest.mark.parametrize("kind", KINDS)
def test_survivors_find_every_pair_of_chains(kind):
    some_dominated = False
    for seed in range(40):
        q, sp, strip = _random_set(1000 * KINDS.index(kind) + seed, kind)
        everyone = pairs_found(q, sp, strip, np.ones(len(q), bool))
        for K in KS:
            dom = dominated(q, sp, strip, K)
            some_dominated |= bool(dom.any())
            assert pairs_found(q, sp, strip, ~dom) == everyone, (kind, seed, K)
    assert some_dominated, kind


def test_gaps_of_eps_and_eps_plus_one():
    """chain mates exactly eps apart dominate one another, cores eps + 1 apart do not (they are not chain mates at all)"""
    for gap, want in ((EPS, True), (EPS + 1, False)):
        q, sp, strip = _sorted([1, 1, 1], [0, gap, 2 * gap], [5, 9, 5])
        assert bool(dominated(q, sp, strip, 4)[1]) == want, gap
        assert (chain_of(q, strip)[-1] == 0) == want, gap


def test_ties_go_by_the_index():
    """a run of cores equal in (q, sp): behind its first core every one has a dominator in front (the smaller index); none of them has
    one behind unless a core of smaller sp follows.  So of a run on its own every core survives (an order that let equal keys
    dominate one another would skip them all); with a lower core behind it the run's last (largest-key) core is dominated and its
    first (smallest-key) core is not."""
    run = 6
    q, sp, strip = _sorted([1] * run, [300] * run, [40] * run)
    assert not dominated(q, sp, strip, 8).any()
    q, sp, strip = _sorted([1] * (run + 1), [300] * run + [300 + EPS], [40] * run + [10])
    dom = dominated(q, sp, strip, 8)
    assert dom[run - 1] and not dom[0] and not dom[run]
    assert dom[1:run].all()
    # the lower core farther away than K neighbours of the run's second core: that one survives, the last is still dominated
    dom = dominated(q, sp, strip, 2)
    assert not dom[1] and dom[run - 1] and not dom[0]


def test_the_vectorised_model_agrees():
    """tools/union_filter_model.py states the same rule with whole-array shifts"""
    import union_filter_model as M
    for kind in KINDS:
        for seed in range(10):
            q, sp, strip = _random_set(77000 + 100 * KINDS.index(kind) + seed, kind)
            for K in KS:
                assert np.array_equal(M.survivors(q, sp, strip, EPS, K), ~dominated(q, sp, strip, K)), (kind, seed, K)
            assert np.array_equal(M.chains(q, strip, EPS), chain_of(q, strip))
