"""Timing of K26 (cl_exp_diagonals / cl_exp_cells_get) on one chr1-sized chromosome, against numpy on the same cells.

The chromosome is chr1 of the 200 M-PET genome of bench.py (cloops_amd.synth, 16.4 M PETs, the same seed); the cells are K24's folded
ones at 10 kb and at 1 kb, balanced by K25 at the defaults of cloops_amd.balance.  Reports, as one JSON document (stdout, and --out, by
default profiles/expected_timing.json), each figure as the median of --reps runs after a warm-up call, in wall clock (every call ends
in a stream synchronise) and between two events recorded on the handle's stream around the call:
  diagonals           cl_exp_diagonals, balanced: the mask, the valid pairs per diagonal, the diagonal order, the sums
  diagonals_raw       the same in raw mode with K25's mask (its copy to the device included)
  oe_get              cl_exp_set and cl_exp_cells_get over all cells in chunks of matrix.CHUNK (the copies to the host included)
  numpy_*             one core over the same cells: the valid pairs by FFT autocorrelation of the mask (np.correlate's direct sum takes
                      nb^2 operations: timed at 10 kb only), the sums per diagonal with np.add.at / np.bincount (the oracle of
                      tests/expected_cases.py), O/E of every cell; and whether the device's arrays equal them (integers exactly, val_sum
                      within (L + 2) 2^-53 per diagonal)
  pieces              with --kernel-trace DIR: kernel times from a rocprofv3 kernel trace of `--trace-only` (a run of its own: tracing
                      slows the host), per cl_exp_diagonals call the mask, the pair kernel, the diagonal order (keys, rocPRIM's sort,
                      gather) and the sums (tile scan, carry fold), and the O/E kernel per pass over the cells; the pair kernel's lane
                      word operations (256 lanes x the words with a partner, summed over its workgroups) per second against what the
                      vector issue rate allows

    timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/expected_bench.py --trace-only
    timeout -k 10 600 python tools/expected_bench.py --kernel-trace DIR [--reps 5] [--out FILE]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

TRACE_CALLS = 4                        # cl_exp_diagonals calls per case of a --trace-only run (the first is the warm-up)
DIAG_BLOCK = 256                       # K26_DB
# what the vector issue rate allows (MI355X: 256 CUs x 4 SIMDs, 2.4 GHz, a wave64 instruction of 32 bits issues in 2 cycles): a word
# needs two ands and two popcounts at the least (8 cycles per wave and word); k26_pairs' loop issues 9 instructions per word (two
# funnel shifts, two selects, two ands, two popcounts, one add: 18 cycles)
SIMDS, CLOCK = 256 * 4, 2.4e9
RATE_AND_POPCOUNT = SIMDS * CLOCK / 8 * 64
RATE_LOOP = SIMDS * CLOCK / 18 * 64


def say(msg):
    sys.stderr.write("expected_bench: %s\n" % msg)
    sys.stderr.flush()


def timed(stream, reps, fn):
    """-> (result of the last run, figures); one warm-up call, then `reps` timed ones"""
    import torch
    fn()
    walls, evs, r = [], [], None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        r = fn()
        walls.append(time.perf_counter() - t0)
        e1.record(stream)
        e1.synchronize()
        evs.append(e0.elapsed_time(e1) * 1e-3)
    return r, {"wall_s": round(float(np.median(walls)), 6), "events_s": round(float(np.median(evs)), 6),
               "events_min_max_s": [round(min(evs), 6), round(max(evs), 6)]}


def host_time(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, round(time.perf_counter() - t0, 4)


def pairs_fft(valid, ign):
    """the valid pairs per diagonal by FFT autocorrelation of the mask, rounded (exact: the values stay below 2^24)"""
    v = np.asarray(valid, np.float64)
    nb = len(v)
    n = 1
    while n < 2 * nb:
        n *= 2
    f = np.fft.rfft(v, n)
    out = np.rint(np.fft.irfft(f * np.conj(f), n)[:nb]).astype(np.int64)
    out[:ign] = 0
    return out


def pair_word_ops(nb):
    """lane word operations of k26_pairs: per workgroup 256 lanes x the mask words with a partner"""
    W = (nb + 63) // 64
    return sum(DIAG_BLOCK * (W - (d0 >> 6)) for d0 in range(0, nb, DIAG_BLOCK))


def trace_groups(d):
    """the kernel trace of a --trace-only run -> (per cl_exp_diagonals call {piece: seconds}, the k26_oe durations in order)"""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        raise SystemExit("no *kernel_trace.csv under %s" % d)
    rows = list(csv.DictReader(open(f[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls, oe, cur, piece = [], [], None, None
    for r in rows:
        name, t = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
        if "k26_oe" in name:
            oe.append(t)
            continue
        if "k26_mask" in name:
            cur, piece = {"mask": 0.0, "pairs": 0.0, "order": 0.0, "sums": 0.0}, "mask"
            calls.append(cur)
        elif cur is None:
            continue
        elif "k26_pairs" in name:
            piece = "pairs"
        elif "k26_keys" in name:
            piece = "order"                                                  # ... and rocPRIM's kernels up to k26_gather
        elif "K26V" in name:
            piece = "sums"
        elif piece != "order":
            cur = None                                                       # (a kernel of another unit: the call is over)
            continue
        cur[piece] += t
        if "k25_fold" in name:
            cur = None
    return calls, oe


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expected_timing.json"))
    ap.add_argument("--trace-only", action="store_true", help="the calls of a kernel trace: no timing, no numpy, no file")
    ap.add_argument("--kernel-trace", default=None, help="directory of a rocprofv3 kernel trace of --trace-only: adds the pieces")
    op = ap.parse_args(argv)
    import torch
    import bench
    import balance_cases as BC
    import expected_cases as EC
    from cloops_amd import api, balance, matrix
    from cloops_amd.synth import chrom_sizes, synth_chrom
    name, length, n = chrom_sizes(int(op.n_total))[0]
    X, Y = synth_chrom(n, length, 1000 * bench.CFG)
    out = {"chrom": name, "pets": int(n), "device": torch.cuda.get_device_name(0), "reps": op.reps, "cases": {},
           "rate_and_popcount_per_s": RATE_AND_POPCOUNT, "rate_loop_per_s": RATE_LOOP}
    traced = trace_groups(op.kernel_trace) if op.kernel_trace else None
    ok = True
    stream = torch.cuda.Stream()
    ch = api.Chromosome(X, Y, stream=stream.cuda_stream)
    for k, (label, res) in enumerate((("10kb", 10000), ("1kb", 1000))):
        c = out["cases"][label] = {"res": res}
        n_cells = ch.mat_cells(res, fold=True)[0]
        b0, nb, _ = ch.bal_marginals(2)
        s, z = ch.bal_marginals_get()
        valid = balance.valid_bins(s, z)
        it = ch.bal_iterate(valid)
        chunks = [(f, min(matrix.CHUNK, n_cells - f)) for f in range(0, n_cells, matrix.CHUNK)]

        def oe_pass(e):
            ch.exp_set(e)
            return [ch.exp_cells_get(f, m) for f, m in chunks]
        if op.trace_only:
            for _ in range(TRACE_CALLS):
                ch.exp_diagonals()
            oe_pass(np.ones(nb))
            continue
        (nd, n_used), c["diagonals"] = timed(stream, op.reps, lambda: ch.exp_diagonals())
        p, cs, vs = ch.exp_diagonals_get()
        w = ch.bal_weights()
        c.update(n_cells=int(n_cells), nb=int(nb), n_used=int(n_used), n_valid=int((~np.isnan(w)).sum()), iters=it[0], converged=bool(it[1]),
                 pair_word_ops=pair_word_ops(nb))
        e = np.full(nb, np.nan)
        e[p > 0] = vs[p > 0] / p[p > 0]
        oe, c["oe_get"] = timed(stream, max(2, op.reps // 2), lambda: oe_pass(e))
        oe = np.concatenate(oe) if oe else np.zeros(0)
        # numpy on one core over the same cells (and the device's own weights)
        bx, by, cnt = ch.mat_cells_get()
        ok_w = ~np.isnan(w)
        pf, c["numpy_pairs_fft_s"] = host_time(lambda: pairs_fft(ok_w, 2))
        same = bool(np.array_equal(pf, p))
        if nb <= 40000:
            pc, c["numpy_pairs_correlate_s"] = host_time(lambda: EC.pairs_oracle(ok_w, 2))
            same &= bool(np.array_equal(pc, p))
        u = EC.used_of(bx, by, b0, 2, ok_w)

        def sums():
            d = (by.astype(np.int64) - bx)[u]
            a = np.zeros(nb, np.int64)
            np.add.at(a, d, cnt[u].astype(np.int64))
            return a, np.bincount(d, EC.terms_of(bx[u], by[u], cnt[u], b0, w), nb)
        (wc, wv), c["numpy_sums_s"] = host_time(sums)
        bound, L = EC.sum_bound(bx, by, b0, nb, 2, ok_w)
        live = L > 0
        dev = np.abs(vs[live] - wv[live]) / wv[live] / bound[live]
        same &= bool(np.array_equal(wc.astype(np.uint64), cs) and int(u.sum()) == n_used and dev.max() <= 1.0 and not vs[~live].any())
        woe, c["numpy_oe_s"] = host_time(lambda: EC.oe_oracle(bx, by, cnt, b0, nb, 2, ok_w, w, e))
        fin = ~np.isnan(woe)
        same &= bool(np.array_equal(np.isnan(oe), ~fin) and (np.abs(oe[fin] - woe[fin]) <= 4 * EC.EPS * woe[fin]).all())
        c["val_sum_over_bound"] = float(dev.max())
        c["numpy_diagonals_s"] = round(c["numpy_pairs_fft_s"] + c["numpy_sums_s"], 4)
        c["speedup_diagonals"] = round(c["numpy_diagonals_s"] / c["diagonals"]["wall_s"], 1)
        c["speedup_oe_get"] = round(c["numpy_oe_s"] / c["oe_get"]["wall_s"], 1)
        _, c["diagonals_raw"] = timed(stream, op.reps, lambda: ch.exp_diagonals(valid=valid, balanced=False))
        c["equal_numpy"] = same
        ok &= same
        if traced:
            calls, toe = traced
            mine = calls[k * TRACE_CALLS + 1:(k + 1) * TRACE_CALLS]
            if len(mine) != TRACE_CALLS - 1:
                raise SystemExit("the kernel trace does not hold %d cl_exp_diagonals calls per case" % TRACE_CALLS)
            c["pieces_s"] = {q: round(float(np.median([m[q] for m in mine])), 7) for q in ("mask", "pairs", "order", "sums")}
            first = sum(len(range(0, int(out["cases"][lab]["n_cells"]), matrix.CHUNK)) for lab in list(out["cases"])[:k])
            c["pieces_s"]["oe_pass"] = round(float(sum(toe[first:first + len(chunks)])), 7)
            rate = c["pair_word_ops"] / c["pieces_s"]["pairs"]
            c["pair_word_ops_per_s"] = float("%.4g" % rate)
            c["pair_share_of_and_popcount_rate"] = round(rate / RATE_AND_POPCOUNT, 4)
            c["pair_share_of_loop_rate"] = round(rate / RATE_LOOP, 4)
        say("%s %s" % (label, c))
    ch.mat_free()
    ch.close()
    if op.trace_only:
        return 0
    js = json.dumps(out, indent=1)
    print(js)
    if op.out:
        os.makedirs(os.path.dirname(os.path.abspath(op.out)), exist_ok=True)
        with open(op.out, "w") as fh:
            fh.write(js + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
