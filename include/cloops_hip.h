/*
 * cloops_hip.h -- C ABI of libcloops_hip.so, the MI355X (gfx950) implementation of the
 * cDBSCAN / cDBSCAN2 / blockDBSCAN hot path of YaqiangCao/cLoops.
 *
 * Plain C: opaque handles, plain pointers and sizes, integer error codes; no exceptions
 * and no torch / numpy types cross this boundary.  Every entry point cites the reference
 * interface it replaces (paths relative to the reference checkout).
 *
 * The reference classes take `mat` = int64[N,3] rows [pointId, X, Y] (cLoops/io.py:192-217)
 * and produce `.labels` = {pointId: clusterId} for clustered points only.  Here a
 * chromosome's X and Y live in HBM as two int32 arrays (|X|,|Y| < 2^29, n < 2^31 - 1024 rows) and labels come
 * back as an int32 array ALIGNED TO THE INPUT ROWS (-1 = absent from `.labels`); the host
 * wrapper (cloops_amd/) turns that into the dict lazily.
 */
#ifndef CLOOPS_HIP_H
#define CLOOPS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (return values; 0 = success) ------------------------------------- */
#define CL_OK             0
#define CL_ERR_ARG       -1   /* bad argument (null pointer, eps <= 0, unknown variant ...)   */
#define CL_ERR_HIP       -2   /* a HIP runtime call failed; see cl_last_error()               */
#define CL_ERR_EMPTY     -3   /* empty input where the reference raises IndexError
                                 (cLoops/cDBSCAN.py:77, cLoops/blockDBSCAN.py:74)             */
#define CL_ERR_DOMAIN    -4   /* coordinates outside the supported domain: |X|,|Y| >= 2^29, or
                                 (variant 2) X > Y / negative coordinate, where cDBSCAN2's
                                 trunc-toward-zero cell rule (cLoops/cDBSCAN2.py:69-70) stops
                                 being an exact grid                                          */
#define CL_ERR_GRID      -5   /* eps so small that the strip/row table would exceed 2^28 rows, or coordinate
                                 extent so large that (X+Y range / eps + 2) * 2^ceil(log2 eps) leaves int32
                                 (never for |X|,|Y| < 2^28).  (The candidate buffer of a sweep grows on demand.)      */
#define CL_ERR_NODEVICE  -6   /* no usable HIP device                                         */
#define CL_ERR_HASH      -7   /* cl_cand_finish: two different boxes shared a 64-bit hash under each of four independent
                                 salts (the pass is redone under another salt three times before this is reported) */

/* ---- clustering variants ---------------------------------------------------------- */
#define CL_VARIANT_CDBSCAN1  1   /* cLoops/cDBSCAN.py:6      class cDBSCAN      (scripts/callStripes:29,
                                    scripts/jd2saturation:23)                                  */
#define CL_VARIANT_CDBSCAN2  2   /* cLoops/cDBSCAN2.py:7     class cDBSCAN      (production, pipe.py:42) */
#define CL_VARIANT_BLOCK     3   /* cLoops/blockDBSCAN.py:6  class blockDBSCAN  (pipe.py:43)   */

/* A chromosome's PETs resident in HBM (+ the reusable device workspace and the result of
 * the last clustering run on it).  Replaces the per-step `joblib.load` of the .jd file
 * (cLoops/io.py:206-217, called at cLoops/pipe.py:58): X,Y cross PCIe once per chromosome,
 * not once per (eps, minPts) step. */
typedef struct cl_chrom cl_chrom;

/* One candidate-loop row: what cLoops/pipe.py:78-102 derives per cluster label. */
typedef struct {
    int32_t min_x, max_x, min_y, max_y;   /* bounding box of the member PETs            */
    int32_t count;                        /* number of member PETs                       */
} cl_box;

/* Per-kernel device timings of the last cl_cluster() call, HIP-event measured on the
 * stream the kernels ran on (only filled when profiling is enabled, see cl_set_profiling). */
typedef struct {
    float ms_keys;        /* K0  filter + key build                                      */
    float ms_sort;        /* K1  radix sort + gather + strip table                       */
    float ms_region;      /* K2  region query (neighbour count)  <- the roofline kernel  */
    float ms_union;       /* K3  core union-find + flatten + component keys              */
    float ms_border;      /* K4  border assignment (+ release fix-up / small-cluster drop) */
    float ms_table;       /* K5  ranks, labels scatter, cluster table                    */
    float ms_d2h;         /* labels + table to host                                      */
    float ms_total;       /* first kernel -> results on host                             */
    int64_t n_in;         /* PETs that entered DBSCAN (after the cut filter)             */
    int64_t n_strips;     /* rows of the strip table (C+1 term of the algorithmic bytes) */
    float ms_bracket;     /* calibration: the same event bracket around an EMPTY kernel (event packets +
                             dispatch gap + ~1 us of empty kernel); a phase that is one kernel (ms_region)
                             reads kernel time + about this much                                    */
    float ms_band;        /* K2 on the cut band of a run that re-uses the counts of its eps (traversal level 4: a kernel
                             of its own, inside the ms_sort phase; 0 = none)                        */
    int64_t n_queried;    /* PETs the region query of ms_region covered (0 = none ran; level 4 queries the whole base
                             layout once per eps: all rows)                                         */
} cl_timing;

/* Human-readable description of the last error on the calling thread. */
const char* cl_last_error(void);

/* Number of visible HIP devices (0 if none / no driver). */
int cl_device_count(void);

/*
 * Upload one chromosome.  `x`, `y`: n int32 coordinates (anchor mid-points, the X and Y
 * columns of the reference's `mat`, cLoops/io.py:49-57,192-203), host pointers if
 * `on_device` == 0, else device pointers on `device` that must stay valid for the life of
 * the handle (no copy is made).  `stream`: a hipStream_t to run on, or NULL for a private
 * stream.  n may be 0.  The handle reserves its whole per-PET workspace here (about 225 B/PET in
 * one allocation: sorted layouts, component / border / label arrays, both result slots, the sweep's
 * q index and a first candidate buffer), so that no run pays for device or pinned-host allocations.
 */
int cl_chrom_create(int device, void* stream, const int32_t* x, const int32_t* y, int64_t n,
                    int on_device, cl_chrom** out);
void cl_chrom_destroy(cl_chrom* c);
int64_t cl_chrom_size(const cl_chrom* c);

/*
 * One clustering run = `DBSCAN(mat, eps, minPts)` of cLoops/pipe.py:70 preceded by the
 * distance pre-filter of cLoops/pipe.py:59-63 (`cut` > 0 keeps rows with Y-X >= cut; pass 0
 * for the bare class constructors cLoops/cDBSCAN.py:12, cLoops/cDBSCAN2.py:13,
 * cLoops/blockDBSCAN.py:13).
 *
 *   labels_out   n int32, host memory (or NULL to leave labels on the device):
 *                cluster id of every input row, -1 for rows that are filtered, noise, or
 *                otherwise absent from the reference's `.labels`.  Ids are exactly the
 *                reference's ids (variant 1 keeps its gaps).
 *   n_clusters   number of distinct cluster ids;   max_label: largest id (or -1).
 *
 * Errors: CL_ERR_EMPTY for variants 1/3 when no row survives the filter and cut == 0
 * (the reference's IndexError); with cut > 0 an empty survivor set is not an error
 * (cLoops/pipe.py:64-65 returns early) and yields zero clusters.
 */
int cl_cluster(cl_chrom* c, int variant, int32_t eps, int32_t min_pts, int32_t cut,
               int32_t* labels_out, int32_t* n_clusters, int32_t* max_label);

/*
 * Variant 1 under an axis-weighted city-block metric: the result of
 *     cDBSCAN(mat * [1, wx, wy], eps, minPts)            (cLoops/cDBSCAN.py:12)
 * i.e. of scripts/callStripes:37-52 (singleStripDBSCAN), which multiplies the X or the Y column by
 * `ext` (50) before clustering to find stripes: two PETs are neighbours iff wx*|dX| + wy*|dY| <= eps.
 * The scaled coordinates (up to 1.25e10) never exist as int32: the kernels work on 64-bit rotated
 * coordinates.  labels_out / n_clusters / max_label as for cl_cluster (ids of variant 1, gaps kept);
 * cl_get_boxes() afterwards returns the boxes in UNSCALED coordinates (callStripes:59-66 divides the
 * scaled extrema by ext again).  1 <= wx, wy <= 4096.  Synchronous; no cut (callStripes uses none).
 */
int cl_cluster_weighted(cl_chrom* c, int32_t eps, int32_t min_pts, int32_t wx, int32_t wy,
                        int32_t* labels_out, int32_t* n_clusters, int32_t* max_label);

/*
 * Asynchronous form for sweeps with a fixed cut (every (eps, minPts) step of the same
 * chromosome is independent there): cl_cluster_async() enqueues one run and returns without
 * blocking; cl_wait() completes the OLDEST outstanding run and reports its cluster count.
 * At most two runs may be in flight; the D2H copy of run k then overlaps the kernels of run
 * k+1.  `labels_out` must stay valid (and should be pinned, cl_host_alloc) until the matching
 * cl_wait() returns; use a different buffer for the second in-flight run.
 * cl_cluster() == cl_cluster_async() + cl_wait().
 */
int cl_cluster_async(cl_chrom* c, int variant, int32_t eps, int32_t min_pts, int32_t cut,
                     int32_t* labels_out);
int cl_wait(cl_chrom* c, int32_t* n_clusters, int32_t* max_label);

/*
 * Cluster table of the last run, indexed by cluster id 0..max_label (count == 0 for the
 * id gaps of variant 1): bounding box + size per label, the inputs of cLoops/pipe.py:83-102.
 * `boxes_out`: (max_label+1) rows of host memory.
 */
int cl_get_boxes(cl_chrom* c, cl_box* boxes_out);
/* Zero-copy view of the same table: (max_label+1) rows in pinned host memory owned by the
 * handle, valid until the next cl_wait()/cl_cluster() that lands in the same result slot
 * (i.e. for at least one more run).  NULL if there is no result or no cluster. */
const cl_box* cl_boxes_host(const cl_chrom* c);
/* Number of PETs of the last completed run that passed the cut filter and entered DBSCAN
 * (`len(mat)` after cLoops/pipe.py:59-62). */
int64_t cl_last_n_in(const cl_chrom* c);

/*
 * Region query alone (kernel K2): neighbour counts |{q : |Xp-Xq|+|Yp-Yq| <= eps}|, self
 * included, per input row (-1 for rows removed by `cut`) -- the quantity the reference
 * compares with minPts (cLoops/cDBSCAN.py:168,177 `len(regionQuery)`,
 * cLoops/cDBSCAN2.py:333-334 `n + cell_pt_num`).  Exposed for parity tests and for the
 * roofline measurement of bench.py.
 */
int cl_neighbor_counts(cl_chrom* c, int32_t eps, int32_t cut, int32_t* counts_out);

/*
 * Distance statistics of the last completed run -- the inputs of cLoops/ests.py:36-61
 * (estIntSelCutFrag), reduced on the GPU instead of materialising the reference's `dis` / `dss`
 * lists (cLoops/pipe.py:63,106-109).  Group 0 = PETs of inter-ligation clusters, group 1 = PETs of
 * self-ligation clusters plus the PETs removed by `cut` (pass the SAME cut as to cl_cluster).
 *   cl_dist_summary  : ONE pass: n_all = len(dis) / len(dss); n_pos, sumx, sumxx = count, sum and sum of squares of
 *                      x = log2|d| - xshift over d != 0 (mean and standard deviation follow from them); loghist =
 *                      histogram of the self group's |d| over bins that are monotone in |d|:
 *                      bin = floor(log2 d) * 128 + (the 7 bits below the leading one)  -- the first level of the EXACT
 *                      median (ests.py:52,58), fine enough to end the search in one more pass for any realistic data
 *   cl_dist_bin_hist : refinement: histogram of (|d| - lo) >> shift over the self group's lo <= |d| < hi (2048 bins)
 * Both are additive over chromosomes (and over GPUs), which is what the sweep driver uses.  The kernels read the
 * run's sorted arrays (distance = the in-strip coordinate) and its labels in sorted order -- no row-aligned labels
 * are needed.
 */
#define CL_DIST_LOGBINS 3840
typedef struct {
    int64_t n_all[2];
    int64_t n_pos[2];
    double sumx[2];
    double sumxx[2];
    double xshift;
    uint64_t loghist[CL_DIST_LOGBINS];
    int64_t fine_lo;                 /* >= 0: `fine` holds the exact histogram of the self group's fine_lo <= |d| < fine_lo + 2048 */
    uint64_t fine[2048];
} cl_dsummary;
int cl_dist_summary(cl_chrom* c, int32_t cut, cl_dsummary* out);
int cl_dist_bin_hist(cl_chrom* c, int32_t cut, uint32_t lo, uint32_t hi, int shift, uint64_t* hist2048);

/*
 * Kernel density sums of log2|d| (kernel K17) -- the curves of cLoops/cPlots.py:42-75 (plotIntSelCutFrag: sns.kdeplot of
 * log2|d| over d != 0 of `dis` and of `dss`), which cLoops/pipe.py:261-267 draws for every step under -plot.  Same groups and
 * same `cut` as cl_dist_summary.
 *   cl_dist_collect : ONE pass over the last completed run: the entries (|d|, weight) with |d| > 0 of both groups go to
 *                     device lists the handle keeps (all PETs under the cut of one distance are one weighted entry), each
 *                     list sorted, so that everything computed from it is the same from call to call.  n_pos[2] = PETs
 *                     with d != 0 per group, dmin[2] / dmax[2] = smallest / largest |d| > 0 (0 for an empty group).
 *   cl_dist_kde     : sums[j] = sum_i w_i exp(-((log2|d_i| - grid_j) inv_h)^2 / 2) over the collected entries of `group`,
 *                     grid_j = lo + j step, 0 <= j < gridsize, 2 <= gridsize <= CL_KDE_MAX_GRID.  UNNORMALISED, hence
 *                     additive over chromosomes: density = sum over chromosomes / (n h sqrt(2 pi)) with h = 1 / inv_h.
 *                     The difference and its product with inv_h are formed in double, the exponential in float32, weight
 *                     and sum in double: relative error below 4e-5.  Two calls on one run return identical arrays.
 *                     Needs cl_dist_collect after the last completed run (CL_ERR_ARG otherwise).
 *   cl_kde_array    : the same sums over a host array of n int32 distances, each of weight 1 (|d| is taken, zeros are
 *                     dropped), without a chromosome handle: what cPlots.plotIntSelCutFrag(di, ds, ...) runs on.
 */
#define CL_KDE_MAX_GRID 1024
int cl_dist_collect(cl_chrom* c, int32_t cut, int64_t* n_pos, int64_t* dmin, int64_t* dmax);
int cl_dist_kde(cl_chrom* c, int group, double lo, double step, double inv_h, int gridsize, double* sums);
int cl_kde_array(int device, const int32_t* d_host, int64_t n, double lo, double step, double inv_h, int gridsize, double* sums);

/*
 * Interval counting for the significance test of candidate loops (cLoops/cModel.py:60-80,108-143):
 * for every record, 11 A windows (the anchor iva + the 10 shifted windows of getNearbyPairRegions,
 * cModel.py:83-105) and 11 B windows, each [lo, hi] inclusive.  `windows`: n_records x 44 int32 laid
 * out as lo[22] (A0..A10, B0..B10) then hi[22].  `out`: n_records x 144 int32:
 *   [0..10]   |S(A_k)|   with S(W) = {PETs with X in W} | {PETs with Y in W}     (ra = [0])
 *   [11..21]  |S(B_l)|                                                            (rb = [11])
 *   [22]      rab = |{X in A_0} & {Y in B_0}|                                     (cModel.py:79)
 *   [23 + 11*k + l]  |S(A_k) & S(B_l)|
 * `cut` > 0 restricts the PETs to Y-X >= cut like parseJd(f, cut) (cLoops/io.py:213-216);
 * *n_pets = number of PETs in the model (N of cModel.py:270).
 */
int cl_sig_counts(cl_chrom* c, int32_t cut, int32_t n_records, const int32_t* windows, int32_t* out, int64_t* n_pets);

/*
 * Interval counts for re-quantifying loops on a dataset (scripts/quantifyLoops.py:124-134) and for differential
 * loops (scripts/deLoops): getPETsforRegions (cLoops/cModel.py:60-80) over the same 11 A and 11 B windows as
 * cl_sig_counts, same `windows` layout (n_records x 44 int32: lo[22] then hi[22], A0..A10 then B0..B10), but the
 * DIRECTED pair counts.  `out`: n_records x 123 int32:
 *   [0]   ra = |S(A_0)|   with S(W) = {PETs with X in W} | {PETs with Y in W}
 *   [1]   rb = |S(B_0)|
 *   [2 + 11*k + l]  |{X in A_k} & {Y in B_l}|                                     ([2] = rab)
 * `cut` > 0 restricts the PETs to Y-X >= cut like parseJd(f, cut) (cLoops/io.py:213-216); *n_pets = number of
 * PETs in the model (N of getGenomeCoverage, cModel.py:45-57).  Reads the sorted tables cl_sig_counts builds.
 */
int cl_quant_counts(cl_chrom* c, int32_t cut, int32_t n_records, const int32_t* windows, int32_t* out, int64_t* n_pets);

/*
 * Histogram of the cell counts of the upper contact matrix (scripts/jd2fingerprint:32-50, jd2contactMatrixUpper):
 * the PETs with Y-X >= cut (cut > 0; parseJd(jd, cut), cLoops/io.py:213-216) fall into the cells
 * ((X - minC) / bin_size, (Y - minC) / bin_size), integer division, minC = the minimum of both coordinate
 * columns of those PETs.  Returns the distinct cell counts in ascending order, `values[k]`, with the number of
 * cells holding that many PETs, `mult[k]`, k < *n_distinct.  The distinct counts D satisfy D (D + 1) / 2 <= *n_kept.
 * *n_cells = number of non-empty cells (sum of mult), *n_kept = PETs that pass the cut, *min_c = minC
 * (n_cells / n_kept / min_c may be NULL).  No PET passing the cut: *n_kept = *n_distinct = 0 and CL_OK (the
 * script's np.min raises there: the caller decides).  Errors: CL_ERR_ARG for a NULL handle or n_distinct,
 * bin_size < 1, cap < 0, cap > 0 with NULL values / mult, runs in flight, or cap < D (then *n_distinct = D and
 * nothing is written to values / mult).  Uses scratch of its own, freed before returning; leaves the handle's
 * layouts, count cache and K8 tables untouched.
 */
int cl_contact_hist(cl_chrom* c, int32_t cut, int32_t bin_size, int64_t cap, int64_t* values, int64_t* mult,
                    int64_t* n_distinct, int64_t* n_cells, int64_t* n_kept, int32_t* min_c);

/*
 * The PETs with an end inside a loop anchor (scripts/jd2cleanWashuPETs.py:162-227, getAnchors + getAnchorPETs): the n_iv
 * closed intervals [starts[k], ends[k]] (any order, overlaps and duplicates allowed) are merged on the host until none
 * overlap or share an endpoint (mergeAllAnchors, :162-180, at its fixed point: [1,5] and [5,9] merge, [1,5] and [6,9]
 * do not), and `mask`, (n + 63) / 64 words, gets bit r % 64 of word r / 64 set iff X[r] or Y[r] lies in a merged
 * interval (the closed searchsorted pair of :214-222); bits past n are 0.  *n_merged = number of merged intervals
 * (the "merged anchors" of the script's log line), *n_kept = number of set rows.  n_iv == 0: a zero mask, zero
 * counts, CL_OK.  Errors: CL_ERR_ARG for a NULL handle, NULL mask / n_merged / n_kept, n_iv < 0, NULL starts / ends
 * with n_iv > 0, any starts[k] > ends[k], or runs in flight.  Uses scratch of its own that stays with the handle;
 * leaves the handle's layouts, count cache and K8 tables untouched.
 */
int cl_anchor_mask(cl_chrom* c, int64_t n_iv, const int64_t* starts, const int64_t* ends,
                   uint64_t* mask, int64_t* n_merged, int64_t* n_kept);

/*
 * Aggregate pile-up of the PETs around loop centres (K19; the aggregate peak analysis of Rao et al. 2014 -- the reference
 * has no counterpart).  The rows with Y - X >= cut take part (all rows for cut <= 0).  With W = 2 w + 1, the window of the
 * loop with centre (cx, cy) starts at ox = cx - w res - res / 2, oy = cy - w res - res / 2 (res / 2 rounded down); a row belongs
 * to it iff 0 <= X - ox < W res and 0 <= Y - oy < W res, and falls into cell i = (X - ox) / res (the X bin), j = (Y - oy) / res
 * (the Y bin) of the loop's matrix M (no negative number is ever divided; duplicated rows count each time; a window may reach
 * below 0 or beyond the last row: those cells are 0).
 *   sum_out    W x W int64, row-major [i][j]: the sum of M over all loops
 *   stats_out  NULL, or n_loops x 6 int32 in the caller's loop order: total = sum of M, centre = M[w][w], and the sums of the four
 *              corner x corner blocks ll = M[W-corner.., ..corner) (nearest the diagonal), ul = M[..corner, ..corner),
 *              ur = M[..corner, W-corner..), lr = M[W-corner.., W-corner..)
 *   mats_out   NULL, or n_loops x W x W int32: every loop's M
 *   n_kept     NULL, or the number of rows that pass the cut
 * Every value is an integer count, so nothing depends on how the loops are scheduled.  Centres may lie anywhere in int32: they are
 * CLAMPED to [-2^30, 2^30], which changes no count (every coordinate of a handle satisfies |v| < 2^29 and W res < 2^29, so the
 * window of a centre at or beyond +-2^30 is as empty as that of its clamped twin) and keeps the window arithmetic inside 32 bits.
 * n_loops == 0, a handle without rows, or a cut that removes every row: zero outputs and CL_OK.  Errors: CL_ERR_ARG for a NULL
 * handle or sum_out, res < 1, w outside [1, 20], corner outside [1, w], W res >= 2^29, n_loops < 0, NULL cx / cy with
 * n_loops > 0, or runs in flight.  Keeps the rows that pass `cut`, sorted by X, in scratch of its own that stays with the handle
 * (rebuilt when another cut is asked for); leaves the handle's layouts, count cache and K8 tables untouched.
 */
int cl_agg_loops(cl_chrom* c, int32_t cut, int32_t res, int32_t w, int32_t corner, int64_t n_loops, const int32_t* cx,
                 const int32_t* cy, int64_t* sum_out, int32_t* stats_out, int32_t* mats_out, int64_t* n_kept);

/*
 * Browser-track text of the PETs (K14): the lines cLoops/io.py:292-348 writes per PET, made on the device in chunks.
 *
 * cl_track_build -- jd2washU / jd2hic's loop over parseJd(f, cut) (io.py:206-217, :301-318, :336-342).  Rows with
 * cut > 0 and Y - X < cut are dropped.  kind CL_TRACK_WASHU: two records per kept row, side 0 anchored at p = X, side 1
 * at p = Y, each line `own\tstart\tend\tpartner:pstart-pend,1\tid\t.\n` with start = max(0, p - ext), end = p + ext
 * (the partner's interval the same way from the other end; int64 arithmetic that wraps as numpy's does), own / partner
 * = name_a / name_b for side 0 and the other way round for side 1; the records are in the order (start, end, row,
 * side) -- the order `bedtools sort` gives up to its unordered ties.  kind CL_TRACK_JUICE: one record per kept row in
 * row order, `0\tname_a\tX\t0\t1\tname_b\tY\t1\n`.  ids: n host int64 (the .jd's first column) or NULL for the row
 * numbers.  -> *n_records, *n_bytes of the whole text.  Errors: CL_ERR_ARG for a NULL handle or NULL outputs / names,
 * an unknown kind, cut < 0, a name longer than CL_TRACK_NAME_MAX bytes, or runs in flight.  The scratch it keeps
 * (device memory of its own: the kept rows, the sorted keys, the line offsets) lives until the next build,
 * cl_track_free or cl_chrom_destroy; the handle's layouts, count cache and K8 tables stay untouched.
 *
 * cl_track_chunks -- splits the built text into chunks of at most `budget` bytes, never inside a line: chunk k is
 * records [rec_bounds[k], rec_bounds[k + 1]), bytes [byte_bounds[k], byte_bounds[k + 1]) of the text; *n_chunks
 * chunks, none empty (0 for an empty track).  rec_bounds and byte_bounds both NULL: only *n_chunks; else both hold
 * cap >= *n_chunks + 1 entries.  The chunks are kept for cl_track_render until the next call.  Errors: CL_ERR_ARG for
 * no built track, budget below the longest line the template allows (2 * CL_TRACK_NAME_MAX + 111 bytes covers every
 * template), cap too small, or runs in flight.
 *
 * cl_track_render -- the text of chunk `chunk` into host memory `out` (cap >= its bytes; page-locked memory from
 * cl_host_alloc copies fastest); *n_bytes = its length.  Errors: CL_ERR_ARG for no chunks, an index out of range, cap
 * too small, or runs in flight.
 *
 * cl_track_free -- releases the scratch of cl_track_build.
 */
#define CL_TRACK_WASHU 0
#define CL_TRACK_JUICE 1
#define CL_TRACK_NAME_MAX 64
int cl_track_build(cl_chrom* c, int32_t kind, int64_t cut, int64_t ext, const int64_t* ids, const char* name_a,
                   const char* name_b, int64_t* n_records, int64_t* n_bytes);
int cl_track_chunks(cl_chrom* c, int64_t budget, int64_t cap, int64_t* rec_bounds, int64_t* byte_bounds, int64_t* n_chunks);
int cl_track_render(cl_chrom* c, int64_t chunk, char* out, int64_t cap, int64_t* n_bytes);
int cl_track_free(cl_chrom* c);

/*
 * 1D coverage of the genome by the PET ends (K20): the signal track that is loaded next to a loop track, as the runs of a
 * bedGraph.  The reference has no counterpart; every value is an integer.
 *
 * Kept rows: all rows for cut <= 0, otherwise the rows with Y - X >= cut.  End points: `ends` is a bit set -- 1 takes every
 * kept row's X, 2 every kept row's Y, 3 both (a row with X == Y then contributes twice); *n_ends is their number, those whose
 * interval turns out empty included.  The interval of an end point p:
 *   window mode (res == 0, ext >= 1)   [max(0, p - ext), p + ext): the start / end of a washU record (cLoops/io.py:306-307)
 *   bin mode (res >= 1, ext == 0)      [b, b + res) with b = floor(p / res) * res (floor also for negative p), start clamped to 0
 * An interval with end <= start after the clamp is dropped (only p < 0 can do that).  depth(t) is the number of intervals that
 * contain base t.  The runs are the maximal [start, end) of constant depth > 0 in ascending order: zero depth is not reported, and
 * two adjacent stretches of equal depth are ONE run (as many intervals end as begin at a position).
 *
 * cl_cov_build -- builds the runs on the device in scratch of its own -> *n_runs, *max_depth (the largest depth; n_ends < 2^32),
 * *n_ends, *area = the sum of depth * (end - start) over the runs (= the sum of the kept intervals' lengths).  An empty handle, a
 * cut that removes every row, or only empty intervals: zero runs and CL_OK.  Errors: CL_ERR_ARG for a NULL handle or NULL outputs,
 * ends outside 1..3, ext < 1 in window mode or ext >= 2^29, res < 0, res >= 2^29, res > 0 with ext != 0, more than 2^31 - 4096 end
 * points, or runs in flight.  The scratch lives until the next build (which rebuilds it: nothing of an earlier build is read
 * again), cl_cov_free or cl_chrom_destroy; the handle's layouts, count cache, K8 / K13 / K14 / K19 state and results stay untouched.
 *
 * cl_cov_runs -- runs [first, first + count) of the last build into host memory: start and end as int32, depth as uint32.
 * Errors: CL_ERR_ARG for no build, a range outside [0, n_runs], NULL outputs with count > 0, or runs in flight.
 *
 * cl_cov_text -- line lengths and offsets of the text of the built runs, one line per run, `name\tstart\tend\tvalue\n` ->
 * *n_bytes of the whole text.  scale_den == 0: value = the depth in decimal.  Otherwise a fixed-point number with exactly three
 * decimals: q = (depth * scale_num + scale_den / 2) / scale_den in unsigned 64-bit arithmetic (both divisions round down), value
 * = q / 1000, '.', q % 1000 with three digits; scale_num <= 2^30 keeps depth * scale_num inside 64 bits.  Counts per million end
 * points: scale_num = 10^9, scale_den = the n_ends of every chromosome written.  No floating point touches the text.  Errors:
 * CL_ERR_ARG for no build, a NULL name / n_bytes, a name longer than CL_TRACK_NAME_MAX bytes, scale_den < 0, scale_num outside
 * [0, 2^30] (outside [1, 2^30] with scale_den > 0), or runs in flight.
 *
 * cl_cov_chunks, cl_cov_render -- as cl_track_chunks / cl_track_render over that text: chunk k is runs [run_bounds[k],
 * run_bounds[k + 1]), bytes [byte_bounds[k], byte_bounds[k + 1]); no chunk is empty and none splits a line.  Errors: CL_ERR_ARG
 * for no built text, a budget below the longest line the template allows (CL_TRACK_NAME_MAX + 44 bytes covers every template), cap
 * too small, a chunk index out of range, or runs in flight.
 *
 * cl_cov_free -- releases the scratch of cl_cov_build.
 */
int cl_cov_build(cl_chrom* c, int64_t cut, int32_t ends, int64_t ext, int64_t res, int64_t* n_runs, uint32_t* max_depth,
                 int64_t* n_ends, int64_t* area);
int cl_cov_runs(cl_chrom* c, int64_t first, int64_t count, int32_t* start_out, int32_t* end_out, uint32_t* depth_out);
int cl_cov_text(cl_chrom* c, const char* name, int64_t scale_num, int64_t scale_den, int64_t* n_bytes);
int cl_cov_chunks(cl_chrom* c, int64_t budget, int64_t cap, int64_t* run_bounds, int64_t* byte_bounds, int64_t* n_chunks);
int cl_cov_render(cl_chrom* c, int64_t chunk, char* out, int64_t cap, int64_t* n_bytes);
int cl_cov_free(cl_chrom* c);

/*
 * Peaks of the PET ends (K21): where the ends themselves pile up -- the binding sites or anchors looked at next to the loops -- as
 * 1D density clustering of the end points, counts of end points in intervals and the summits of intervals.  The reference has no
 * counterpart; every value is an integer (the significance test stays on the host, cloops_amd/peaks.py).
 *
 * End points, as for cl_cov_build: the rows with Y - X >= cut take part (all for cut <= 0); `ends` is 1, 2 or 3 for X, Y or both
 * (a row with X == Y counts twice under 3).  S is the ascending multiset of these m values; equal values are separate points.
 * m <= 2^31 - 4096.  lb(x) = #{p in S : p < x}, ub(x) = #{p in S : p <= x}.
 *
 * Candidate peaks of a setting (eps, min_pts), 1 <= eps < 2^29, min_pts >= 1:
 *   n(i) = #{j : |S[j] - S[i]| <= eps} = ub(S[i] + eps) - lb(S[i] - eps), the point itself included; point i is a core iff
 *   n(i) >= min_pts.  A chain is a maximal set of cores in which neighbouring cores, in the order of S, lie at most eps apart
 *   (equal positions are 0 apart); chain k has its first core at position a_k and its last at b_k.  The members of peak k are the
 *   points at positions p with max(a_k - eps, b_(k-1) + eps + 1) <= p <= b_k + eps (b_(-1) = -infinity): a border point within eps
 *   of the cores of two chains belongs to the left one, as in sequential DBSCAN over ascending points.  They are a contiguous index
 *   range [i0, i1) of S, and the peak is start = S[i0], end = S[i1 - 1] + 1 (half-open, BED), n_points = i1 - i0, n_cores = the
 *   cores of the chain.  Peaks come in ascending order and are disjoint.
 * Counts: for any half-open interval [s, e) with int64 bounds, #{p in S : s <= p < e}; intervals may overlap, be unordered, be
 * empty (e <= s: 0), and reach below S[0] or beyond S[m - 1].
 * Summits: for ascending, pairwise disjoint intervals (starts[k] <= ends[k] <= starts[k + 1]) and a half-width w, 1 <= w < 2^29:
 * the position of the member point with the largest n_w(i) = #{j : |S[j] - S[i]| <= w}, the smallest such position on ties, and
 * that n_w; an interval without points gives position -1 and count 0.
 *
 * cl_peak_sort -- the end points as keys, sorted once on the device in scratch of its own -> *n_ends = m, *vmin = S[0], *vmax =
 * S[m - 1].  The sorted array stays until the next sort, cl_peak_free or cl_chrom_destroy, and serves every call, get, count and
 * summit call in between.  An empty handle or a cut that removes every row: zero end points, vmin = vmax = 0 and CL_OK.  A sort
 * forgets the peaks called before it.
 * cl_peak_call -- the candidate peaks of (eps, min_pts) over the sorted end points -> *n_peaks, *n_cores (all cores), *n_clustered
 * (the sum of n_points).  A setting without cores (or no end points): zeros and CL_OK.  It replaces the peaks of the call before.
 * cl_peak_get -- peaks [first, first + count) of the last call into host memory: start and end as int32, n_points and n_cores as
 * uint32.
 * cl_peak_count -- counts[k] = the end points in [starts[k], ends[k]) for n intervals.
 * cl_peak_summits -- pos[k], cnt[k] = the summit of [starts[k], ends[k]) for n intervals and the half-width w.
 * cl_peak_free -- releases the scratch of cl_peak_sort and of the calls after it.
 *
 * Errors: CL_ERR_ARG for a NULL handle or NULL outputs (arrays may be NULL when their count is 0), ends outside 1..3, eps or w
 * outside [1, 2^29), min_pts < 1, a call, get, count or summit before a sort, a get before a call, a range outside [0, n_peaks],
 * summit intervals that are not ascending and disjoint, more than 2^31 - 4096 end points (or intervals), or runs in flight; all of
 * them are found on the host before any launch.  The handle's layouts, count cache, K8 / K13 / K14 / K19 / K20 state and results
 * stay untouched.
 */
int cl_peak_sort(cl_chrom* c, int64_t cut, int32_t ends, int64_t* n_ends, int64_t* vmin, int64_t* vmax);
int cl_peak_call(cl_chrom* c, int64_t eps, int64_t min_pts, int64_t* n_peaks, int64_t* n_cores, int64_t* n_clustered);
int cl_peak_get(cl_chrom* c, int64_t first, int64_t count, int32_t* start, int32_t* end, uint32_t* n_points, uint32_t* n_cores);
int cl_peak_count(cl_chrom* c, const int64_t* starts, const int64_t* ends, int64_t n, uint32_t* counts);
int cl_peak_summits(cl_chrom* c, const int64_t* starts, const int64_t* ends, int64_t n, int64_t w, int32_t* pos, uint32_t* cnt);
int cl_peak_free(cl_chrom* c);

/*
 * Domains (K22): the integers behind a domain call -- three insulation tracks over the bins of a chromosome and the PETs of called
 * domains.  The reference has no counterpart, so these definitions are the specification; the scores and thresholds stay on the host
 * (cloops_amd/domains.py).
 *
 * Kept rows, as for cl_agg_loops, cl_cov_build and cl_peak_sort: the rows with Y - X >= cut take part (all for cut <= 0).
 * Bins: res >= 1; the bin of a coordinate p is floor(p / res), floor also for negative p.  bx, by: the bins of a row's X and Y; bmin,
 * bmax: the smallest and largest bin over the X and Y of the kept rows.  The tracks have n_bins = bmax - bmin + 2 entries, for
 * b = bmin .. bmax + 1; entry b describes the boundary at the START of bin b, at position b res.  With the window w >= 1 (in bins):
 *   cross(b) = #{rows : b - w <= bx <  b <= by < b + w}     the insulation square of Crane et al. 2015
 *   up(b)    = #{rows : b - w <= bx <= by < b}              the upstream triangle
 *   down(b)  = #{rows : b <= bx <= by < b + w}              the downstream triangle
 * A row with by < bx adds to none of them, but counts in n_kept, bmin and bmax.  Duplicated rows count each time.
 * Range form (what the kernel does): a row with bx <= by adds 1 to cross on [max(bx + 1, by - w + 1), min(bx + w, by)], to up on
 * [by + 1, bx + w] and to down on [by - w + 1, bx], each only where the interval is not empty (and inside bmin .. bmax + 1).
 * Domain counts, over the kept rows of the last cl_dom_tracks, for ascending, pairwise disjoint half-open intervals [s_k, e_k) in bp
 * (int64 bounds; intervals may be empty or abut): nx_k = #{X in [s_k, e_k)}, ny_k = #{Y in [s_k, e_k)}, intra_k = #{X and Y both in
 * [s_k, e_k)}.
 *
 * cl_dom_tracks -- the three tracks of (cut, res, w) on the device -> *n_bins, *bin0 = bmin, *n_kept.  The kept rows sorted by X are
 * K19's table, shared with cl_agg_loops: it is built when the handle does not hold it for this cut, so a second call with another w
 * (or res) does not sort again, and cl_agg_loops at another cut rebuilds it for itself (cl_dom_count then builds it again).  The
 * tracks stay until the next cl_dom_tracks, cl_dom_free or cl_chrom_destroy.  An empty handle or a cut that removes every row:
 * n_bins = 0, bin0 = 0, n_kept = 0 and CL_OK.
 * cl_dom_get -- entries [first, first + count) of the three tracks into host memory, entry k standing for b = bin0 + k.
 * cl_dom_count -- intra[k], nx[k], ny[k] of the n intervals.
 * cl_dom_free -- releases the tracks and the scratch of the calls (K19's table stays with the handle).
 *
 * Errors: CL_ERR_ARG for a NULL handle or NULL outputs (arrays may be NULL when their count is 0), res outside [1, 2^29), w outside
 * [1, 1024], w res >= 2^29, the span of ALL rows of the handle (whatever the cut) giving more than 2^24 bins at res, a get or count
 * before tracks, a get range outside [0, n_bins], count intervals that are not ascending and disjoint (starts[k] <= ends[k] <=
 * starts[k + 1]), n < 0 or more than 2^31 - 4096 intervals, or runs in flight; all of them are found on the host before any launch.  A
 * refused call zeroes its scalar outputs and leaves the earlier state usable.  The handle's layouts, count cache, K8 / K13 / K14 /
 * K20 / K21 state and results stay untouched.
 */
int cl_dom_tracks(cl_chrom* c, int64_t cut, int64_t res, int64_t w, int64_t* n_bins, int64_t* bin0, int64_t* n_kept);
int cl_dom_get(cl_chrom* c, int64_t first, int64_t count, uint32_t* cross, uint32_t* up, uint32_t* down);
int cl_dom_count(cl_chrom* c, const int64_t* starts, const int64_t* ends, int64_t n, uint32_t* intra, uint32_t* nx, uint32_t* ny);
int cl_dom_free(cl_chrom* c);

/*
 * k-distances (K23): the distance of every PET to its k-th nearest neighbour, and its log-binned histogram -- the curve a user reads
 * a sensible eps of DBSCAN from.  The reference has no counterpart, so these definitions are the specification; quantiles and the
 * suggested eps stay on the host (cloops_amd/esteps.py).
 *
 * Kept rows, as for cl_agg_loops and cl_dom_tracks: the rows with Y - X >= cut take part (all for cut <= 0), m of them.  Duplicated
 * rows are separate points.
 * Table order: the kept rows ascending by X, rows of equal X in input order (K19's table, a stable sort).
 * k-distance: for a kept row p and 1 <= k <= CL_KDIS_KMAX, d_k(p) is the k-th smallest of |Xp - Xq| + |Yp - Yq| over the kept rows
 * q != p; a duplicate of p is a neighbour at distance 0.  With m - 1 < k there is no k-th neighbour and d_k = -1 for every row.  Every
 * coordinate of a handle satisfies |v| < 2^29, so d_k <= 2^31 - 4 fits int32.  A row is a core of (eps, minPts) -- its neighbour count,
 * itself included, is >= minPts -- iff d_(minPts - 1) <= eps: k = minPts - 1.
 * Histogram, per k: hist[b] = #{rows : d_k >= 1 and logbin(d_k) == b} with the log bins of cl_dist_summary (bin = floor(log2 d) * 128
 * + the 7 bits below the leading one), CL_KDIS_BINS = 31 * 128 of them for d < 2^31; n_zero = #{rows : d_k == 0}; n_none = #{rows :
 * d_k == -1}.  Histograms of different chromosomes add.
 * Cost: a row reads the rows whose X lies within its d_kmax of its own X, hundreds to a few thousand on ChIA-PET / HiChIP densities;
 * it is quadratic only on an input with almost all X equal.
 *
 * cl_kdis_build -- d_k of every kept row for the n_k values of ks (1 <= n_k <= 8, strictly ascending, each in [1, CL_KDIS_KMAX]) in
 * ONE pass that keeps the ks[n_k - 1] smallest distances per row, and their histograms, on the device -> *n_kept.  A build with
 * (5, 10, 20) equals three builds with one k each.  The kept rows sorted by X are K19's table: it is built when the handle does not
 * hold it for this cut, exactly as by cl_dom_tracks.  The results stay until the next build, cl_kdis_free or cl_chrom_destroy (X and
 * Y of the table are copied beside them, so cl_agg_loops at another cut does not disturb them).  An empty handle or a cut that
 * removes every row: n_kept = 0, empty gets, zero histograms and CL_OK.
 * cl_kdis_get -- entries [first, first + count) in table order for ks[which]: the row's X and Y, and its d.
 * cl_kdis_hist -- hist[CL_KDIS_BINS], *n_zero and *n_none for ks[which].
 * cl_kdis_free -- releases the results (K19's table stays with the handle).
 *
 * Errors: CL_ERR_ARG for a NULL handle or NULL outputs (the arrays of a get may be NULL when count is 0), n_k outside 1..8, a k
 * outside 1..CL_KDIS_KMAX or ks not strictly ascending, which outside 0..n_k - 1, a get or hist before a build, a range outside
 * [0, n_kept], or runs in flight; all of them are found on the host before any launch.  A refused call zeroes its scalar outputs and
 * leaves the earlier state usable.  The handle's layouts, count cache, K8 / K13 / K14 / K20 / K21 / K22 state and results stay
 * untouched.
 */
#define CL_KDIS_KMAX 64
#define CL_KDIS_BINS 3968
int cl_kdis_build(cl_chrom* c, int64_t cut, const int32_t* ks, int32_t n_k, int64_t* n_kept);
int cl_kdis_get(cl_chrom* c, int32_t which, int64_t first, int64_t count, int32_t* x, int32_t* y, int32_t* d);
int cl_kdis_hist(cl_chrom* c, int32_t which, uint64_t* hist, uint64_t* n_zero, uint64_t* n_none);
int cl_kdis_free(cl_chrom* c);

/*
 * Contact matrices (K24): the binned contact map of a chromosome in the three forms a contact workflow asks for -- a dense window for
 * a heatmap, the non-empty cells of the whole chromosome for an export or a comparison, and the profile of one viewpoint (virtual
 * 4C).  The reference has no counterpart, so these definitions are the specification; labels, text and scaling stay on the host
 * (cloops_amd/matrix.py).  cl_contact_hist (K12) bins from the data's minimum and returns only the histogram of the cell counts; the
 * bins here are genome coordinates.
 *
 * Kept rows, as for cl_dom_tracks: the rows with Y - X >= cut take part (all for cut <= 0), n_kept of them.  Duplicated rows count each
 * time.
 * Bins: res >= 1; the bin of a coordinate p is floor(p / res), floor also for negative p (the rule of cl_dom_tracks).  bx, by: the
 * bins of a row's X and Y.
 *
 * cl_mat_window -- out is nx * ny uint32, row-major [i][j]: out[i][j] = #{kept rows : bx - bx0 == i and by - by0 == j}.  With
 * mirror != 0 a row with bx != by additionally counts at (by - bx0, bx - by0) when that cell lies in the window: a window on the
 * diagonal (bx0 == by0, nx == ny) is then a symmetric matrix whose diagonal cells are counted once.  *n_in = the sum of out.  The
 * window may lie anywhere; cells beyond the data are 0.  Limits: 1 <= nx, ny <= CL_MAT_WMAX, nx * ny <= CL_MAT_CELLS_MAX, |bx0|,
 * |by0| <= 2^30, res in [1, 2^29).
 * cl_mat_cells -- the distinct (bx, by) of the kept rows, ascending by bx then by, each with its count, kept on the device ->
 * *n_cells, *n_kept, *max_count (the largest count).  With fold != 0 a row's cell is (min(bx, by), max(bx, by)).  The sum of the
 * counts is n_kept.  No limit on the number of bins (64-bit keys, sorted over the bits in use only).  The cells stay with the handle
 * until the next cl_mat_cells, cl_mat_free or cl_chrom_destroy (copies: cl_agg_loops at another cut does not disturb them).
 * cl_mat_cells_get -- cells [first, first + count) inside [0, n_cells] into host memory; the arrays may be NULL when count is 0.
 * cl_mat_v4c -- the viewpoint is the half-open interval [v0, v1) in bp, v0 <= v1.  Every kept row adds 1 at bin by if its X lies in
 * the viewpoint, and 1 at bin bx if its Y lies in it (both may happen).  out[k], k < nb, is the total at bin b0 + k; *n_x = #{X in
 * viewpoint}, *n_y = #{Y in viewpoint} over all kept rows, whether or not their other end falls in [b0, b0 + nb).  Limits: 0 <= nb <=
 * 2^24 (out may be NULL for nb == 0), |b0| <= 2^30, res in [1, 2^29).
 * cl_mat_free -- releases the cells and the scratch of the calls (K19's table stays with the handle).
 *
 * The kept rows sorted by X are K19's table, built when the handle does not hold it for this cut, exactly as by cl_dom_tracks and
 * cl_kdis_build.  An empty handle or a cut that removes every row: zero outputs, n_cells = 0 and CL_OK.
 * Errors: CL_ERR_ARG for a NULL handle or NULL outputs, a limit violated, v0 > v1, a get before cl_mat_cells or outside its range, or
 * runs in flight; all of them are found on the host before any launch.  A refused call zeroes its scalar outputs and leaves the
 * earlier state usable.  The handle's layouts, count cache, K8 / K13 / K14 / K20 - K23 state and results stay untouched.
 */
#define CL_MAT_WMAX 8192
#define CL_MAT_CELLS_MAX 16777216
int cl_mat_window(cl_chrom* c, int64_t cut, int64_t res, int64_t bx0, int64_t by0, int64_t nx, int64_t ny, int32_t mirror,
                  uint32_t* out, int64_t* n_in, int64_t* n_kept);
int cl_mat_cells(cl_chrom* c, int64_t cut, int64_t res, int32_t fold, int64_t* n_cells, int64_t* n_kept, int64_t* max_count);
int cl_mat_cells_get(cl_chrom* c, int64_t first, int64_t count, int32_t* bx, int32_t* by, uint32_t* cnt);
int cl_mat_v4c(cl_chrom* c, int64_t cut, int64_t res, int64_t v0, int64_t v1, int64_t b0, int64_t nb, uint32_t* out, int64_t* n_x,
               int64_t* n_y, int64_t* n_kept);
int cl_mat_free(cl_chrom* c);

/*
 * Matrix balancing (K25): iterative correction (ICE, Imakaev 2012) of the folded cells of the last cl_mat_cells -- one weight per bin
 * so that every valid row of the weighted matrix has the same sum.  The reference has no counterpart, so these definitions are the
 * specification (tests/balance_cases.py restates them in numpy); the mask's rule, the texts and the files stay on the host
 * (cloops_amd/balance.py).
 *
 * Input: the cells (bx, by, cnt) of cl_mat_cells(c, cut, res, fold = 1), bx <= by, ascending.  They stand for the symmetric matrix A with
 * A[i][j] = A[j][i] = cnt; a diagonal cell counts once.  Bins: b0 = bx of the first cell .. b1 = the largest by, nb = b1 - b0 + 1.  A
 * cell is used iff by - bx >= ignore_diags (0 uses every cell).
 * Raw marginals (exact integers): sum[i] = the sum of cnt over the used cells that touch bin b0 + i (an off-diagonal cell touches both
 * of its bins, a diagonal cell its bin once), nnz[i] = the number of such cells.  *n_used = the number of used cells.
 * Iteration (fp64): w[i] = 1 where valid[i] != 0, else 0.  Up to max_iters times: (1) s[i] = the sum over the used cells that touch i
 * of (w[bx] cnt) w[by]; (2) over the bins with s[i] != 0: mean = their mean, var = the mean of (s[i] / mean - 1)^2; (3) w[i] /=
 * s[i] / mean on those bins; (4) the iteration counts, and the loop stops as converged if var < tol.  No s[i] != 0 at all: 0
 * iterations, not converged, var = scale = NaN (also with max_iters = 0 or nb = 0).
 * Result: scale = the last mean; weight[i] = w[i] / sqrt(scale) where w[i] > 0, NaN elsewhere; the balanced value of a cell -- of
 * EVERY cell, also those nearer the diagonal than ignore_diags -- is ((double)cnt weight[bx]) weight[by], NaN where a weight is NaN.
 *
 * cl_bal_marginals -- builds the transposed order of the cells (sorted by (by, bx): both halves of a marginal are then sums over runs
 * of sorted keys) and the raw marginals -> *b0, *nb, *n_used.  nb <= CL_BAL_BINS_MAX.
 * cl_bal_marginals_get -- sum / nnz of the bins [first, first + count) inside [0, nb].
 * cl_bal_iterate -- valid: nb words (may be NULL when nb is 0).  May be called again with another mask, max_iters or tol without
 * another cl_bal_marginals.  Sums are taken in a fixed order: two calls with the same input give the same bytes.
 * cl_bal_weights_get, cl_bal_cells_get -- the weights of the bins / the balanced values of the cells [first, first + count) of the
 * last cl_bal_iterate.
 * cl_bal_free -- releases the state (the cells stay).  The next cl_mat_cells, cl_mat_free and cl_chrom_destroy release it as well.
 *
 * A handle with no rows or no cells: nb = 0 and CL_OK everywhere.  Errors: CL_ERR_ARG for a NULL handle or NULL outputs, no cells on
 * the handle or cells that are not folded, ignore_diags < 0, nb > CL_BAL_BINS_MAX, max_iters < 0, tol < 0 or NaN, cl_bal_iterate or a
 * get before cl_bal_marginals, weights or balanced values before cl_bal_iterate, a range outside the bins or cells, or runs in flight.
 */
#define CL_BAL_BINS_MAX 16777216
int cl_bal_marginals(cl_chrom* c, int32_t ignore_diags, int64_t* b0, int64_t* nb, int64_t* n_used);
int cl_bal_marginals_get(cl_chrom* c, int64_t first, int64_t count, uint64_t* sum, uint32_t* nnz);
int cl_bal_iterate(cl_chrom* c, const uint32_t* valid, int32_t max_iters, double tol, int32_t* iters, int32_t* converged, double* var,
                   double* scale);
int cl_bal_weights_get(cl_chrom* c, int64_t first, int64_t count, double* weight);
int cl_bal_cells_get(cl_chrom* c, int64_t first, int64_t count, double* balanced);
int cl_bal_free(cl_chrom* c);

/*
 * Expected contacts by distance and observed / expected (K26): per diagonal of the contact matrix the number of valid bin pairs, the
 * sum of the counts and the sum of the (balanced) values of its cells -- what the P(s) curve and `cooltools expected-cis` are made
 * of -- and, once the host has decided the expected value of every diagonal, the observed / expected value of every cell.  The
 * reference has no counterpart, so these definitions are the specification (tests/expected_cases.py restates them in numpy); the
 * smoothing of the curve, the texts and the files stay on the host (cloops_amd/expected.py).
 *
 * Input: the state after cl_mat_cells(c, cut, res, fold = 1) and cl_bal_marginals(c, ignore_diags, ..): the cells (bx, by, cnt), bx <=
 * by, and the bins b0 .. b0 + nb - 1.  Two modes.  Balanced (balanced = 1): needs a finished cl_bal_iterate; bin i is valid iff its
 * weight is not NaN, w[i] is that weight, and valid must be NULL.  Raw (balanced = 0): valid is nb words, nonzero meaning valid (NULL:
 * every bin is valid), and w[i] = 1 on the valid bins.
 * For every diagonal d = 0 .. nd - 1, nd = nb:
 *   n_pairs[d] (int64)  = #{ i : 0 <= i, i + d < nb, valid[i] and valid[i + d] }, and 0 for d < ignore_diags;
 *   cnt_sum[d] (uint64) = the sum of cnt over the USED cells of the diagonal: by - bx == d, d >= ignore_diags, both bins valid;
 *   val_sum[d] (fp64)   = the sum of (w[bx] cnt) w[by] over the same cells (the order of operations inside a term is K25's).  The terms
 *                         of a diagonal are added in an order that depends on the cells and nb alone: two calls with the same input give
 *                         the same bytes; no fp64 atomics.  In raw mode val_sum equals cnt_sum exactly while it is below 2^53;
 *   *n_used = the number of used cells over all diagonals.
 * With expected[d] set (cl_exp_set): the O/E of a cell is ((w[bx] cnt) w[by]) / expected[by - bx]; NaN when the cell is not used or
 * expected[by - bx] is NaN or 0.
 *
 * cl_exp_diagonals -- packs the mask to one bit per bin and counts the valid pairs of every diagonal (the autocorrelation of the
 * mask: nb^2 / 64 and-popcount operations on 64-bit words at most, half of them with a partner word -- some 10^9 at 250 000 bins and
 * 4 10^12 at CL_BAL_BINS_MAX), builds the diagonal order of the cells (one radix sort of (d, cell index) pairs) and takes the sums
 * -> *nd, *n_used.
 * cl_exp_diagonals_get -- the three arrays of the diagonals [first, first + count) inside [0, nd].
 * cl_exp_set -- the expected value of every diagonal, count == nd; may be called again without another cl_exp_diagonals.
 * cl_exp_cells_get -- the O/E of the cells [first, first + count) of cl_mat_cells, in their order.
 * cl_exp_free -- releases the state (the cells, marginals and weights stay).  The next cl_exp_diagonals, cl_bal_marginals,
 * cl_bal_iterate, cl_bal_free, cl_mat_cells, cl_mat_free and cl_chrom_destroy release it as well.
 *
 * nb == 0 is not an error: nd = 0, n_used = 0, and gets of count 0 succeed with NULL arrays.  Errors: CL_ERR_ARG for a NULL handle or
 * NULL outputs, balanced not 0 or 1, balanced = 1 before cl_bal_iterate or with a mask, any call before cl_bal_marginals, a get or
 * cl_exp_set before cl_exp_diagonals, cl_exp_cells_get before cl_exp_set, count != nd in cl_exp_set, a range outside the diagonals or
 * the cells, or runs in flight.
 */
int cl_exp_diagonals(cl_chrom* c, const uint32_t* valid, int32_t balanced, int64_t* nd, int64_t* n_used);
int cl_exp_diagonals_get(cl_chrom* c, int64_t first, int64_t count, int64_t* n_pairs, uint64_t* cnt_sum, double* val_sum);
int cl_exp_set(cl_chrom* c, const double* expected, int64_t count);
int cl_exp_cells_get(cl_chrom* c, int64_t first, int64_t count, double* oe);
int cl_exp_free(cl_chrom* c);

/*
 * Compartments (K27): the leading eigenpairs of the chromosome's O/E matrix minus one -- the A/B compartment track, what `cooltools
 * eigs-cis` computes -- by subspace iteration over the cells resident on the device.  The reference has no counterpart, so these
 * definitions are the specification (tests/compartments_cases.py restates them in numpy); the orientation of the vectors, the clip's
 * percentile, the texts and the files stay on the host (cloops_amd/compartments.py).
 *
 * Input: the state after cl_mat_cells(fold = 1), cl_bal_marginals, cl_exp_diagonals (either mode) and cl_exp_set: the cells (bx, by,
 * cnt), the bins b0 .. b0 + nb - 1, K26's validity of a bin and its w, ign = ignore_diags and expected[d].  From the caller: clip (fp64,
 * > 0, or +inf) and dmax, ign <= dmax <= nb; the diagonals at or beyond dmax take no part.
 * The symmetric matrix M (nb x nb):
 *   M[i][j] = min(oe(i, j), clip) - 1   where both bins are valid and ign <= |i - j| < dmax,
 *   M[i][j] = 0                         everywhere else;
 *   oe(i, j) is K26's O/E of the cell of the two bins, ((w[bx] cnt) w[by]) / expected[by - bx], in that order of operations, and 0
 *   without a cell (the entry is then -1).  A diagonal cell counts once.
 * M is never stored densely.  M = S - B: S the sparse matrix of min(oe, clip) over the used cells inside the band, B the 0/1 matrix of
 * the valid pairs inside the band; (B x)[i] is a difference of prefix sums of valid x, at most four look-ups per bin.
 * cl_eig_build refuses expected values that are NaN, infinite or <= 0 on a diagonal ign <= d < dmax that holds at least one valid pair:
 * the host picks dmax so that there is none.
 *
 * Result of cl_eig_iterate, 1 <= n_eigs <= CL_EIG_MAX: the n_eigs eigenpairs of M of largest |lambda|, ordered by |lambda| descending,
 * the sign of lambda kept.  A vector has unit 2-norm over the valid bins and NaN on the others; its sign makes its entry of largest
 * magnitude positive (the lowest bin on a tie).  resid[k] = |M v_k - lambda_k v_k|_2; *converged iff every resid[k] <= tol |lambda_0|.
 * With fewer than n_eigs valid bins there are n_valid pairs and the others are NaN (values, residuals and vectors).  Without a valid
 * bin, and with max_iters = 0: 0 iterations, not converged, everything NaN.
 * Method: subspace iteration on a block Q of CL_EIG_BLOCK orthonormal columns (n_valid of them when there are fewer valid bins).  An
 * iteration is Z = M Q; H = Q^T Z; the Ritz pairs (lambda, W) of the 8 x 8 H by cyclic Jacobi; v = Q W with the residuals |Z W - Q W
 * lambda|; Q = the orthonormalised Z W (Gram-Schmidt, twice).  The start block is a fixed integer hash of (column, bin); a column that
 * vanishes under the projections (its remainder below 2^-40 of its squared norm) is replaced by the next hash vector and
 * orthogonalised.  M = 0 gives eigenvalues 0, orthonormal vectors and *converged after one iteration.  Every sum is taken in an order
 * that depends on the cells, nb and the block alone: two calls on the same input give the same bytes; no fp64 atomics.
 *
 * cl_eig_build -- the values of the cells inside the band in both orders and their row pointers -> *n_valid, *n_in (the cells inside
 * the band: used, ign <= by - bx < dmax).
 * cl_eig_apply -- y = M x for n_vec vectors, x and y n_vec x nb row-major, 1 <= n_vec <= CL_EIG_BLOCK; the invalid bins of x read as 0,
 * those of y are 0.  Leaves the result of cl_eig_iterate alone.
 * cl_eig_iterate -- at most max_iters iterations -> *iters, *converged, eigval and resid (n_eigs values each); the vectors stay on
 * the device.  May be repeated with other arguments.
 * cl_eig_vectors_get -- entries [first, first + count) inside [0, nb] of vector `which`, 0 <= which < the n_eigs of the last
 * cl_eig_iterate.
 * cl_eig_free -- releases the state (cells, marginals, weights, diagonals and expected values stay).  The next cl_eig_build,
 * cl_exp_set, cl_exp_diagonals, cl_exp_free and everything that releases K26's state release it as well.
 *
 * nb == 0 is not an error (dmax must then be 0): n_valid = n_in = 0, 0 iterations, NaN values, and calls of count 0 succeed with NULL
 * arrays.  Errors:
 * CL_ERR_ARG, found on the host before any launch, scalar outputs zeroed and the earlier state left usable, for a NULL handle or NULL
 * outputs, any call before cl_exp_set, clip not above 0 or NaN, dmax outside [ign, nb], the rule on the expected values, nb >
 * CL_EIG_BINS_MAX, n_eigs or n_vec out of range, max_iters < 0, tol < 0 or NaN, cl_eig_apply, cl_eig_iterate or cl_eig_vectors_get
 * before cl_eig_build, cl_eig_vectors_get before cl_eig_iterate, `which` or a range outside, or runs in flight.
 */
#define CL_EIG_MAX 6
#define CL_EIG_BLOCK 8
#define CL_EIG_BINS_MAX 1048576
int cl_eig_build(cl_chrom* c, double clip, int64_t dmax, int64_t* n_valid, int64_t* n_in);
int cl_eig_apply(cl_chrom* c, const double* x, int32_t n_vec, double* y);
int cl_eig_iterate(cl_chrom* c, int32_t n_eigs, int32_t max_iters, double tol, int32_t* iters, int32_t* converged, double* eigval,
                   double* resid);
int cl_eig_vectors_get(cl_chrom* c, int32_t which, int64_t first, int64_t count, double* v);
int cl_eig_free(cl_chrom* c);

/*
 * Two samples compared (K28): the integer moments of the stratum-adjusted correlation coefficient (SCC, HiCRep: Yang et al. 2017) of
 * two contact matrices.  The reference has no counterpart, so these definitions are the specification (tests/similarity_cases.py
 * restates them in numpy); the coefficients, the weights, the texts and the files stay on the host (cloops_amd/similarity.py).
 *
 * Input: two handles a and b on one device, each with the cells of a cl_mat_cells(c, cut, res, fold = 1) of the same res (the cuts may
 * differ; a == b is allowed).  From the caller: the window of bins [b0, b0 + nb), h (0 <= h <= CL_SCC_HMAX) and n_diags = D (1 <= D <=
 * nb, or D = 0 with nb = 0).
 * For a sample s, A_s is the symmetric nb x nb matrix of its cells inside the window: A[u][v] = A[v][u] = cnt with u = bx - b0 and v =
 * by - b0; a diagonal cell counts once; a cell with a bin outside the window takes no part; everything else is 0.
 * Box sums (zero padding at the window's edge; sums, not means -- Pearson's coefficient does not tell them apart):
 *   S_s[i][j] = the sum of A_s[u][v] over |u - i| <= h, |v - j| <= h, 0 <= u, v < nb.
 * Strata: for d = 0 .. D - 1 the positions (i, i + d), 0 <= i < nb - d.  A position is counted iff S_a != 0 or S_b != 0.  Over the
 * counted positions of d, with x = S_a and y = S_b:
 *   n[d] (int64)                          = their number,
 *   sx[d], sy[d] (uint64)                 = the sums of x and of y,
 *   sxx[d], syy[d], sxy[d] (uint64)       = the sums of x x, y y and x y.
 * Everything is an integer: two calls give the same bytes, and a test may ask for equality.
 * Overflow rule, decided on the host in exact arithmetic before any launch: with Smax_s = min((2h+1)^2 max_count_s, 2 n_kept_s) of
 * what cl_mat_cells recorded, the call is refused unless max(Smax_a, Smax_b)^2 nb < 2^64 -- no box sum then passes 2^32 and no sum
 * of a diagonal 2^64.
 * Memory: each matrix is held in band form, nb x (D + 4h) uint32; the call is refused unless nb (D + 4h) <= CL_SCC_BAND_MAX.
 *
 * cl_scc_moments -- synchronous: waits for both handles' streams before it reads either handle's cells, enqueues on a's stream and
 * returns with the six arrays (D entries each) on the host.  Neither handle's cells, K25-K27 state, layouts or results are touched.
 * The scratch (two band arrays, the accumulators) stays with a and is reused when large enough; nothing is kept on b.
 * cl_scc_free -- releases the scratch.  The next cl_mat_cells, cl_mat_free and cl_chrom_destroy of a release it as well.
 *
 * nb == 0 gives CL_OK with NULL arrays.  A sample without cells (an empty handle, or a cut that removes every row) is a zero matrix.
 * Errors: CL_ERR_ARG, found on the host before any launch, the earlier state left usable and the outputs zeroed (each non-NULL array
 * must hold n_diags entries whenever 1 <= n_diags <= CL_SCC_BAND_MAX), for a NULL handle or NULL output, handles on different devices,
 * no cells or unfolded cells on either handle, different res, h, n_diags or nb out of range (negative, or beyond the band limit), |b0| >
 * 2^30, the overflow rule (the message says so), or runs in flight on either handle.
 */
#define CL_SCC_HMAX 20
#define CL_SCC_BAND_MAX 268435456
int cl_scc_moments(cl_chrom* a, cl_chrom* b, int64_t b0, int64_t nb, int32_t h, int64_t n_diags, int64_t* n, uint64_t* sx, uint64_t* sy,
                   uint64_t* sxx, uint64_t* syy, uint64_t* sxy);
int cl_scc_free(cl_chrom* a);

/*
 * Loops from the contact matrix (K29): the local-enrichment ("donut") test of HiCCUPS (Rao et al. 2014; `cooltools dots` restates it)
 * over every pixel of a band of the matrix -- four neighbourhood sums of observed and expected per pixel, the local expected count
 * la_k they imply, the histogram of the raw counts per chunk of la_k, and the call against the caller's thresholds.  The reference has
 * no counterpart, so these definitions are the specification (tests/dots_cases.py restates them in numpy); the thresholds from the
 * histogram (FDR), the enrichment filter, the merging of pixels into loops, the texts and the files stay on the host
 * (cloops_amd/dots.py).
 *
 * Input: the state after cl_mat_cells(fold = 1), cl_bal_marginals, cl_exp_diagonals (either mode) and cl_exp_set: the cells (bx, by,
 * cnt), the bins b0 .. b0 + nb - 1, K26's validity of a bin and its w (1 on the valid bins in raw mode), ign = ignore_diags and
 * expected[e].  From the caller: p and w, 0 <= p < w <= CL_DOT_WMAX, and dmin, dmax with ign <= dmin < dmax <= nb (dmin = dmax = 0
 * with nb = 0).
 * Two symmetric nb x nb matrices:
 *   V[u][v] = (w[u] cnt) w[v], in K25's order of operations, where the pair has a cell, both bins are valid and |u - v| >= ign, and 0
 *             everywhere else; a diagonal cell counts once;
 *   E[u][v] = expected[|u - v|] where both bins are valid and |u - v| >= ign, and 0 everywhere else.
 *   Positions outside [0, nb) read as 0 in both.
 * Four neighbourhoods around a pixel (i, j), j = i + d, as offsets (a, b) added to (i, j); inner(a, b) = |a| <= p and |b| <= p:
 *   k = 0  donut       |a| <= w, |b| <= w, a != 0, b != 0, not inner;
 *   k = 1  lower-left  1 <= a <= w, -w <= b <= -1, not inner (the side towards the diagonal);
 *   k = 2  horizontal  |a| <= 1, p < |b| <= w;
 *   k = 3  vertical    |b| <= 1, p < |a| <= w.
 * A footprint may cross the main diagonal: the matrices are symmetric.
 * NO_k(i, j) / NE_k(i, j) = the sum of V / of E over neighbourhood k.  The local expected raw count of the pixel is
 *   la_k = ((NO_k / NE_k) expected[d]) / (w[i] w[j]),   in that order of operations;
 * la_k is NaN when the pixel is no candidate -- d outside [dmin, dmax), or i or j invalid (j >= nb included) -- or NE_k is 0.  A pixel
 * is FULL when its four la_k are numbers; only full pixels take part in the histogram and the call.
 * Summation rule: NO and NE are sums of at most T = (2w+1)^2 non-negative fp64 terms; the device adds terms or partial sums only and
 * never subtracts one fp64 sum from another (no running sums, no summed-area differences in fp64; integers may be subtracted freely);
 * the order of the additions is fixed by the geometry alone; no fp64 atomics: two calls give the same bytes.  Any two orders of
 * adding at most T non-negative terms lie within 2 (T - 1) 2^-53 of each other, relatively.
 * Chunks: edges[0 .. n_chunks), finite, above 0, strictly ascending, 1 <= n_chunks <= CL_DOT_CHUNKS_MAX; chunk(x) = the smallest l
 * with x <= edges[l], by comparisons alone; a value above the last edge is in no chunk, and a full pixel with such a la_k is BEYOND.
 * Histogram: hist[k][l][c] (uint64, 4 x n_chunks x (CL_DOT_CMAX + 1)) = the number of full pixels that are not beyond, have
 * chunk(la_k) == l and min(cnt, CL_DOT_CMAX) == c, cnt the raw count of the pixel's cell and 0 without a cell (the zero-count pixels
 * of the band are most of the tests an FDR corrects for); *n_beyond = the full pixels left out because they are beyond.
 * Call: thr[k][l] (uint32, 4 x n_chunks, over the edges of the last cl_dot_hist); a cell is significant iff its pixel is full, is not
 * beyond and cnt >= thr[k][chunk(la_k)] for all four k.  The result is the ascending list of the significant cells' indices into
 * the order of cl_mat_cells.
 * Memory: V is held in band form, nb x (dmax + 4w) fp64, the la in a dense array of nb x (dmax - dmin) x 4 fp64; the call is refused
 * unless nb (dmax + 4w) <= CL_DOT_BAND_MAX.  E is never stored.
 *
 * cl_dot_lambdas -- the band, the four la of every pixel (i, d), 0 <= i < nb, dmin <= d < dmax -> *n_cand (the candidates), *n_full.
 * cl_dot_lambdas_get -- la of kernel k for the bins [first_bin, first_bin + n_bins) inside [0, nb]: n_bins x (dmax - dmin), row-major,
 * row = bin i, column = d - dmin.
 * cl_dot_cells_get -- the four la of the cells [first, first + count) of cl_mat_cells: count x 4, NaN where the cell's pixel is no
 * candidate.
 * cl_dot_hist -- the histogram over the dense array -> hist, *n_beyond.  May be repeated with other edges.
 * cl_dot_call -- -> *n_sig; the list stays on the device.  May be repeated with other thresholds.
 * cl_dot_sig_get -- entries [first, first + count) inside [0, n_sig] of the list.
 * cl_dot_free -- releases the state (cells and the K25-K27 state stay).  The next cl_dot_lambdas, cl_exp_set, cl_exp_diagonals,
 * cl_exp_free and everything that releases K26's state release it as well.  K27's state and K29's do not touch each other.
 *
 * The calls are synchronous on the handle's stream.  nb == 0 is not an error: n_cand = n_full = n_beyond = n_sig = 0, a histogram of
 * zeros, and the arrays may be NULL.  Errors: CL_ERR_ARG, found on the host before any launch, scalar outputs zeroed and the earlier
 * state left usable, for a NULL handle or NULL output, any call before cl_exp_set, p, w, dmin or dmax outside the rules above, the
 * band limit, an expected[e] that is NaN, infinite or negative on a diagonal ign <= e < min(nb, dmax + 2w) that holds a valid pair
 * (zero is allowed), edges that are not finite, positive and strictly ascending, n_chunks out of range, cl_dot_hist or a get before
 * cl_dot_lambdas, cl_dot_call before cl_dot_hist, cl_dot_sig_get before cl_dot_call, a kernel index outside [0, 3], a range outside
 * its array, or runs in flight.
 */
#define CL_DOT_WMAX 16
#define CL_DOT_CHUNKS_MAX 64
#define CL_DOT_CMAX 4095
#define CL_DOT_BAND_MAX 134217728
int cl_dot_lambdas(cl_chrom* c, int32_t p, int32_t w, int64_t dmin, int64_t dmax, int64_t* n_cand, int64_t* n_full);
int cl_dot_lambdas_get(cl_chrom* c, int32_t kernel, int64_t first_bin, int64_t n_bins, double* la);
int cl_dot_cells_get(cl_chrom* c, int64_t first, int64_t count, double* la4);
int cl_dot_hist(cl_chrom* c, const double* edges, int32_t n_chunks, uint64_t* hist, uint64_t* n_beyond);
int cl_dot_call(cl_chrom* c, const uint32_t* thr, int64_t* n_sig);
int cl_dot_sig_get(cl_chrom* c, int64_t first, int64_t count, int64_t* cell_index);
int cl_dot_free(cl_chrom* c);

/*
 * Saddle tables (K30): how strongly the map segregates by a per-bin class -- the sums that `cooltools saddle` is made of: the bins are
 * sorted into classes (quantiles of a compartment track), and every pair of classes gets the number of its bin pairs, the number of
 * its cells and the sum of their O/E.  The reference has no counterpart, so these definitions are the specification
 * (tests/saddle_cases.py restates them in numpy); the track, the class edges, the symmetrising, the strength, the texts and the files
 * stay on the host (cloops_amd/saddle.py).
 *
 * Input: the state after cl_mat_cells(fold = 1), cl_bal_marginals, cl_exp_diagonals (either mode) and cl_exp_set: the cells (bx, by,
 * cnt), the bins b0 .. b0 + nb - 1, K26's validity of a bin and its w, ign = ignore_diags and expected[d].  From the caller: cls[nb]
 * (int32), the class of every bin: -1 means the bin takes no part, otherwise 0 <= cls[i] < n_cls; n_cls, 1 <= n_cls <=
 * CL_SAD_CLASSES_MAX; and a band lo <= d < hi with max(ign, 1) <= lo <= hi <= nb: the main diagonal never takes part.
 * The pair set P: all (i, j) with 0 <= i < j < nb, lo <= j - i < hi, both bins valid and both classes >= 0.
 * Three n_cls x n_cls tables, row-major, a the class of the lower bin and b the class of the upper bin:
 *   pairs[a][b] (int64) = the number of (i, j) in P with cls[i] = a and cls[j] = b; pairs without a cell count too;
 *   cells[a][b] (int64) = the number of cells whose bin pair is in P with those classes;
 *   sum[a][b] (fp64)    = the sum of K26's O/E over those cells, ((w[bx] cnt) w[by]) / expected[by - bx] in that order of operations;
 *                         a pair without a cell adds 0.
 * As cl_eig_build does, cl_sad_sums refuses an expected[d] that is NaN, infinite or <= 0 on a diagonal lo <= d < hi that holds at
 * least one valid pair, on the host before any launch: the host picks hi so that there is none.
 * The terms of an entry of `sum` are added in an order that depends on the cells, nb, cls, lo and hi alone -- neither on the device's
 * CU count nor on timing: two calls with the same input give the same bytes.  No fp64 atomics.
 *
 * cl_sad_sums -- count == nb -> *n_binned (the valid bins with a class), *n_pairs (the total of pairs), *n_in (the total of cells).
 * The pair counts cost nb n_cls look-ups (differences of per-class prefix counts), not nb (hi - lo); the sums stream the cells once
 * in the order they lie.
 * cl_sad_get -- the three tables, n_cls * n_cls entries each.
 * cl_sad_free -- releases the state (cells and the K25-K26 state stay).  The next cl_sad_sums, cl_exp_set, cl_exp_diagonals,
 * cl_exp_free and everything that releases K26's state release it as well.  K27's and K29's state and K30's do not touch each other.
 *
 * The calls are synchronous on the handle's stream.  nb == 0 is not an error: lo = hi = 0 and the totals are all zero; lo == hi is
 * not an error: the tables are all zero.  Errors: CL_ERR_ARG, found on the host before any launch, scalar outputs zeroed and the
 * earlier state left usable, for a NULL handle or NULL outputs, any call before cl_exp_set, count != nb, a class outside [-1, n_cls),
 * n_cls out of range, a band outside the rule above, the rule on the expected values, cl_sad_get before cl_sad_sums, or runs in
 * flight.
 */
#define CL_SAD_CLASSES_MAX 64
int cl_sad_sums(cl_chrom* c, const int32_t* cls, int64_t count, int32_t n_cls, int64_t lo, int64_t hi, int64_t* n_binned, int64_t* n_pairs,
                int64_t* n_in);
int cl_sad_get(cl_chrom* c, double* sum, int64_t* pairs, int64_t* cells);
int cl_sad_free(cl_chrom* c);

/*
 * Pairs files to BEDPE (K15): the per-line loops of scripts/hicpropairs2bedpe (pairs2bedpe, :9-35) and
 * scripts/juicerLong2bedpe.py (long2bedpe, :10-32), one chunk of input text at a time.  A converter is not tied to a
 * chromosome: it is a handle of its own.
 *
 * cl_conv_create -- a converter on `device` for `format` (CL_CONV_HICPRO: HiC-Pro allValidPairs, fields split at '\t'
 * after strip(), A = [f1, p1, p1 + ext] on "+" else [f1, p1 - ext, p1], B the same from f4 f5 f6, line
 * `A B f0 . f3 f6`; CL_CONV_JUICER: Juicer "long" format, fields split at whitespace runs, line
 * `f1 max(0, p1 - ext) p1 + ext f5 max(0, p2 - ext) p2 + ext . . s1 s2`, s = "+" where f0 / f4 is "0"; CL_CONV_PAIRS:
 * 4DN pairs v1.0, `readID chr1 pos1 chr2 pos2 strand1 strand2`, which replaces reordering the columns to HiC-Pro's by hand:
 * CL_CONV_HICPRO's rule on f0 f1 f2 f5 f3 f4 f6, line `A B f0 . f5 f6`; a line whose first byte is '#' is a header line: it
 * is counted in *n_lines and in cl_conv_error's line numbers and has no text), on `stream` (NULL:
 * a stream of its own), taking chunks of at most `budget` bytes (1 .. CL_CONV_BUDGET_MAX).  Errors: CL_ERR_NODEVICE
 * without a device (there is no CPU path); CL_ERR_ARG for a NULL out, an unknown format or a budget out of range.
 *
 * cl_conv_feed -- converts the complete lines of bytes[0 .. n) (n <= budget; page-locked memory from cl_host_alloc copies
 * fastest): with last == 0 the bytes after the last '\n' are left over (*consumed stops there) and go in front of the
 * next feed; with last != 0 the input ends here and its last line may lack the '\n'.  A feed may also stop early on very
 * short lines (at most budget / 16 + 256 lines per feed): the caller feeds bytes[*consumed ..] again.  *n_lines /
 * *n_bytes: the lines converted and the bytes of their text, for cl_conv_render.  Reading rules: lines end at '\n' only,
 * whitespace is ASCII \t \n \v \f \r and space, an integer is an optional sign and ASCII digits with optional whitespace
 * around it, and must fit int64 with +-ext applied.  CL_ERR_PARSE: a line the reference would raise on (fewer than 7
 * fields, a bad integer, a blank line), a value out of int64, or (last == 0) n == budget bytes with no '\n'; the lines in
 * front of it are converted and counted, cl_conv_error tells which line and why.  Errors: CL_ERR_ARG for NULL outputs,
 * n < 0 or n > budget.
 *
 * cl_conv_render -- the text of the last feed's lines into host memory `out` (cap >= *n_bytes of that feed);
 * *n_bytes = its length.  Errors: CL_ERR_ARG for no feed since creation, or cap too small.
 *
 * cl_conv_error -- the last feed's error: *line counts every line fed to this handle (1-based), *kind is one of
 * CL_CONV_E_* (0: none).
 *
 * cl_conv_timing -- device times of the last feed and render, in ms: ms[0] copy to the device, ms[1] the feed's kernels
 * (the index, parse and scan, with one read-back of the line count between them), ms[2] the render kernel, ms[3] the
 * copy to the host.
 *
 * cl_conv_destroy -- waits for the handle's stream and frees the handle.
 */
typedef struct cl_conv cl_conv;
#define CL_ERR_PARSE        -8   /* cl_conv_feed: a line the reference's script would raise on (cl_conv_error)   */
#define CL_CONV_HICPRO       0
#define CL_CONV_JUICER       1
#define CL_CONV_PAIRS        2
#define CL_CONV_E_FIELDS     1   /* fewer than 7 fields (a blank line included): the reference's IndexError      */
#define CL_CONV_E_INT        2   /* a position that is not an integer: the reference's ValueError               */
#define CL_CONV_E_RANGE      3   /* a position, or a position +- ext, outside int64                              */
#define CL_CONV_E_LONG       4   /* a line longer than the chunk budget                                          */
#define CL_CONV_BUDGET_MAX   (1LL << 30)
int cl_conv_create(int device, void* stream, int32_t format, int64_t ext, int64_t budget, cl_conv** out);
int cl_conv_feed(cl_conv* c, const char* bytes, int64_t n, int32_t last, int64_t* consumed, int64_t* n_lines,
                 int64_t* n_bytes);
int cl_conv_render(cl_conv* c, char* out, int64_t cap, int64_t* n_bytes);
int cl_conv_error(cl_conv* c, int64_t* line, int32_t* kind);
int cl_conv_timing(cl_conv* c, float* ms);
int cl_conv_destroy(cl_conv* c);

/*
 * BEDPE input (K16): the per-line loops of cLoops/io.py:62-129 (parseRawBedpe) and :132-189 (parseRawBedpe2) with the PET
 * rule of :30-59 (class PET), one chunk of BEDPE text at a time; the PETs stay on the device, grouped by chromosome in
 * file order, ready for cl_chrom_create(..., on_device = 1).  The host reads (or inflates) the bytes and keeps the
 * dictionary chromosome name -> id; it never touches a PET.  A handle works on one stream; two handles on two streams
 * take the chunks in turn (chunk k on handle k % 2) and cl_ingest_finish joins them.
 *
 * Reading rules (cloops_amd/io.py:parse_bedpe under Python 3's text mode): a line ends at '\n', "\r\n" counts as '\n';
 * fields split at '\t' only; a line is skipped when a field is exactly "*" and a field is exactly "-1" (io.py:84-85,
 * :159-160), when it has fewer than 10 fields (:43, :47 read the strands), when field 1, 2, 4 or 5 is no integer (:87-93,
 * :162-166), when fields 0 and 3 differ (:96, :168) or when cB - cA < cut for cut > 0 (:103-104, :174-175); the ends are
 * swapped when startA + endA > startB + endB (:50-53); cA, cB are the floors of the half sums (:55-56).  An integer is
 * [+-]?[0-9]+ with |value| < 2^62; a field of bytes 0x21 .. 0x7e without '_' that is not one makes the line skipped; any
 * other numeric field, a byte >= 0x80, a '\r' not followed by '\n' or a chromosome name longer than 255 bytes makes the
 * line EXOTIC: the device does not restate what Python's int() and text decoding do with it, the caller reads the files on the host.
 *
 * cl_ingest_create -- a reader on `device` and `stream` (NULL: a stream of its own) for chunks of at most `budget` bytes
 * (1 .. CL_CONV_BUDGET_MAX), with the distance filter `cut` (io.py:103, :174); want_distances != 0 keeps what
 * cl_ingest_distances needs (io.py:122-123).  Errors: CL_ERR_NODEVICE without a device (there is no CPU path); CL_ERR_ARG.
 *
 * cl_ingest_set_format -- what the handle reads, allowed only before its first feed (CL_ERR_ARG after it, or for an unknown
 * format): CL_INGEST_BEDPE (what cl_ingest_create leaves) or CL_INGEST_PAIRS, 4DN pairs text.  It replaces converting the
 * file with cl_conv_* (CL_CONV_PAIRS, `ext`) and feeding the BEDPE text: every data line gives the record of the line the
 * converter writes for it (`A0 A1 A2 B0 B1 B2 f0 . f5 f6`: the "*" / "-1" rule on these ten fields, a coordinate equal to
 * -1 being a "-1" field; chr1 against chr2; strand1 against strand2; the swap, the floors and `cut` as above).  A line
 * whose first byte is '#' is a header line: no PET.  A byte >= 0x80, a '\r' that is not the last byte before the '\n', a
 * coordinate of 2^62 or more in magnitude or a chromosome name longer than 255 bytes makes a data line EXOTIC.
 *
 * cl_ingest_error -- CL_INGEST_PAIRS: the first line of the last feed on which the converter raises (cl_conv_error's
 * counterpart; it replaces looking for that line with a converter run): *line counts the lines of that feed, header
 * lines included (1-based; 0: none), *kind is its CL_CONV_E_* (0: none).  The caller stops the read there.
 *
 * cl_ingest_headers -- CL_INGEST_PAIRS: *n = the header lines among the last feed's *n_lines (it replaces counting the
 * lines of the converted text: the lines of a read are its data lines).
 *
 * cl_ingest_feed -- the loop bodies of io.py:80-105 / :155-176 for the n bytes of complete lines at `bytes` (n <= budget;
 * only the last line may lack its '\n'; page-locked memory copies fastest): *n_lines = the lines of the chunk (blank ones
 * count, io.py:82, :157), *first_exotic = the first exotic line of the chunk (0-based) or -1, *n_names = the distinct
 * chromosome names of the kept lines, or -1 when they are more than 65536 (the caller reads the files on the host).
 *
 * cl_ingest_names -- the distinct names of the last feed, one entry each: the name's 64-bit hash, the first line it
 * occurs on and where its bytes are in the chunk (any order; what is copied is sized by the names, not by the lines).
 *
 * cl_ingest_commit -- io.py:98-99 / :171-172 (the wanted chromosomes) and :106-121 / :177-185 (the PET appended to its
 * chromosome): the host's table for the last feed -- `hashes` ascending, ids[k] the chromosome id (0 .. n_ids - 1) of
 * hashes[k] or -1 to drop it, its name at names[name_off[k] .. + name_len[k]) -- is applied to every kept line and the
 * PETs are appended to their chromosomes in line order; `chunk` orders the chunks of all handles, `line0` is the global
 * number of the chunk's first line.  counts[id] = the PETs appended per chromosome.  *status: 0; 1 when a line's name
 * differs from the dictionary's bytes under the same hash, 2 when a hash is missing from the table -- nothing is
 * appended then (two names with one hash never merge).
 *
 * cl_ingest_finish -- ends the read on `c` and on `other` (the second handle or NULL; its chunks move to `c`): per
 * chromosome id the chunks' PETs become one array each in file order; unique != 0 drops every PET whose (cA, cB)
 * occurred earlier on its chromosome (io.py:113-116); n_rows[id] = the PETs left, *n_distances = the kept PETs whose
 * strand fields differ (io.py:122-123).  After it only the calls below and cl_ingest_destroy are allowed on `c`, only
 * cl_ingest_destroy on `other`.
 *
 * cl_ingest_rows -- the int64 mid-points of chromosome `id` into host arrays a, b of cap >= n_rows[id] values.
 * cl_ingest_chrom_arrays -- *x, *y: int32 device arrays of *n mid-points for cl_chrom_create(..., on_device = 1); they
 * live until cl_ingest_destroy.  CL_ERR_DOMAIN when a value is outside |v| < 2^29 (what cl_chrom_create requires).
 * cl_ingest_distances -- cB - cA of the PETs counted by *n_distances, in global line order (io.py:122-123), into `out`.
 *
 * cl_ingest_timing -- device times summed over the handle's calls, in ms: ms[0] copies to the device, ms[1] the line
 * index, ms[2] the parse kernel, ms[3] the names table, ms[4] commit (apply, sort, gather), ms[5] finish.
 *
 * cl_ingest_destroy -- waits for the handle's stream and frees the handle and every array it handed out.
 */
typedef struct cl_ingest cl_ingest;
typedef struct cl_ingest_name {
    uint64_t hash;
    uint32_t first, off, len, pad;
} cl_ingest_name;
#define CL_INGEST_TIMES 6
#define CL_INGEST_BEDPE 0
#define CL_INGEST_PAIRS 1
int cl_ingest_create(int device, void* stream, int64_t budget, int64_t cut, int32_t want_distances, cl_ingest** out);
int cl_ingest_set_format(cl_ingest* c, int32_t format, int64_t ext);
int cl_ingest_feed(cl_ingest* c, const char* bytes, int64_t n, int64_t* n_lines, int64_t* first_exotic, int64_t* n_names);
int cl_ingest_error(cl_ingest* c, int64_t* line, int32_t* kind);
int cl_ingest_headers(cl_ingest* c, int64_t* n);
int cl_ingest_names(cl_ingest* c, cl_ingest_name* out, int64_t cap, int64_t* n);
int cl_ingest_commit(cl_ingest* c, int64_t chunk, int64_t line0, const uint64_t* hashes, const int32_t* ids,
                     const uint32_t* name_off, const uint32_t* name_len, int32_t n_table, const char* names,
                     int64_t names_bytes, int32_t n_ids, int64_t* counts, int32_t* status);
int cl_ingest_finish(cl_ingest* c, cl_ingest* other, int32_t n_ids, int32_t unique, int64_t* n_rows, int64_t* n_distances);
int cl_ingest_rows(cl_ingest* c, int32_t id, int64_t* a, int64_t* b, int64_t cap);
int cl_ingest_chrom_arrays(cl_ingest* c, int32_t id, int64_t* n, void** x, void** y);
int cl_ingest_distances(cl_ingest* c, int64_t* out, int64_t cap);
int cl_ingest_timing(cl_ingest* c, float* ms);
int cl_ingest_destroy(cl_ingest* c);

/* Device pointer to the labels of the last run (n int32, row aligned) -- lets the caller
 * keep results on the GPU (e.g. to hand them to RCCL) without a host round trip.  NULL if the run did not
 * produce row-aligned labels (see cl_set_device_labels). */
const int32_t* cl_labels_device(const cl_chrom* c);

/*
 * Candidate loops of a sweep, kept on the device (kernels K10).  Replaces, for one chromosome, the record lists that
 * cLoops/pipe.py:241-281 carries from step to step: `cl_cand_append` classifies the cluster table of the last
 * completed run like pipe.py:83-97 (skip degenerate boxes; inter-ligation iff maxX < minY) and appends the
 * inter-ligation boxes, in ascending cluster id, with the given step number; it returns how many inter- and
 * self-ligation boxes the run had.  `cl_cand_finish` applies combineTwice (pipe.py:155-174: a box survives in the
 * step of its first appearance, duplicates inside one step all stay) and filterClusterByDis (pipe.py:130-143:
 * floor mid-point distance >= final_cut) and copies the surviving boxes {minX, maxX, minY, maxY} to boxes_out in
 * append order -- the order of the reference's record list.  capacity / *n_out in rows of 4 int32.
 * cl_cand_reset starts a new sweep.
 */
int cl_cand_reset(cl_chrom* c);
/* The labels of a run as the reference holds them: cDBSCAN(mat, eps, minPts).labels is a dict of the CLUSTERED points only
 * (cDBSCAN2.py:186-191, cDBSCAN.py:143-152).  Like cl_cluster_async, but instead of n row-aligned labels the run leaves one
 * (row, label) int32 pair per labelled PET, in no particular order: its last kernel stages them in device memory and
 * cl_wait copies exactly cl_last_n_labelled(c) of them into `pinned_pairs_out` (page-locked host memory: cl_host_alloc;
 * capacity_pairs pairs -- n always suffices; a run that labels MORE than capacity_pairs PETs makes cl_wait return
 * CL_ERR_ARG and copies nothing).  A sweep that wants labels on the host every run moves 8 bytes per clustered PET
 * over PCIe instead of 4 bytes per PET.  Rotated variants at traversal level >= 3 and minPts 2 .. 128 only (CL_ERR_ARG
 * otherwise). */
int cl_cluster_pairs_async(cl_chrom* c, int variant, int32_t eps, int32_t min_pts, int32_t cut, int32_t* pinned_pairs_out,
                           int64_t capacity_pairs);
/* cl_last_n_labelled: the labelled PETs of the last completed pairs / row-mask run: what cl_wait copied.  After a cl_wait that
 * returned CL_ERR_ARG for capacity it is the number that run labelled -- the capacity the caller needs, larger than the one it gave --
 * until the handle's next cl_wait or synchronous run completes; nothing else of the refused run is available (the results the
 * other getters return stay those of the run completed before it).  -1: no handle, or no completed run. */
int64_t cl_last_n_labelled(const cl_chrom* c);
/* The same set -- the clustered points and their cluster ids, what cDBSCAN(mat, eps, minPts).labels holds (cDBSCAN2.py:186-191,
 * cDBSCAN.py:143-152) -- in its smallest form: ceil(n / 64) 64-bit mask words (bit r % 64 of word r / 64 set <=> input row r is
 * clustered), followed by one int32 label per set bit in ASCENDING ROW ORDER.  4 bytes per clustered PET + n / 8 bytes cross PCIe
 * instead of 8 bytes per clustered PET: the label-inclusive sweep is bound by that copy.  `pinned_out` (page-locked host memory:
 * cl_host_alloc) must hold 8 * ceil(n / 64) + 4 * capacity_labels bytes; cl_wait copies the mask and exactly
 * cl_last_n_labelled(c) labels (a run that labels MORE than capacity_labels PETs makes cl_wait return CL_ERR_ARG and copies
 * nothing; n always suffices); cl_set_pairs_defer / cl_pairs_sync apply to this copy as well.  Same restrictions as
 * cl_cluster_pairs_async. */
int cl_cluster_rowmask_async(cl_chrom* c, int variant, int32_t eps, int32_t min_pts, int32_t cut, void* pinned_out,
                             int64_t capacity_labels);
/* cl_set_pairs_defer(c, 1): cl_wait of a pairs run returns with the copy of the pairs to the host still in flight (their number
 * is known: cl_last_n_labelled); cl_pairs_sync(c) completes it.  A host that collects many chromosomes waits for all of them
 * first and syncs afterwards, so that their copies cross PCIe side by side. */
void cl_set_pairs_defer(cl_chrom* c, int enabled);
int cl_pairs_sync(cl_chrom* c);

/* One step of a sweep in ONE asynchronous call: cl_cluster_async(labels_out = NULL) followed, in the run's own stream,
 * by what cl_cand_append and cl_dist_summary do for that run (same `cut`).  After cl_wait the results are on the host:
 * cl_step_result copies them out without touching the GPU.  One step in flight per chromosome.  `fine_lo` >= 0 (a guess
 * of where the self group's median will fall, e.g. the previous step's) makes the summary also histogram the distances
 * fine_lo .. fine_lo + 2047 exactly: when the median lands there no refinement pass (cl_dist_bin_hist) is needed. */
int cl_cluster_step_async(cl_chrom* c, int variant, int32_t eps, int32_t min_pts, int32_t cut, int32_t step, int64_t fine_lo);
int cl_step_result(cl_chrom* c, int64_t* n_inter, int64_t* n_self, cl_dsummary* out);
int cl_cand_append(cl_chrom* c, int32_t step, int64_t* n_inter, int64_t* n_self);
int cl_cand_finish(cl_chrom* c, int32_t final_cut, int32_t* boxes_out, int64_t capacity, int64_t* n_out);
/* The same, leaving the surviving boxes ON THE DEVICE: *dev_rows_out = n_out rows of {minX, maxX, minY, maxY} int32 in device
 * memory of the handle (valid until its next sweep finishes or it is destroyed) -- what cl_comm_gather_device
 * (include/cloops_comm.h) sends to the rank that merges the ranks' tables (cLoops/pipe.py:119-127 merges in the parent),
 * without a detour through the host on the sending ranks. */
int cl_cand_finish_device(cl_chrom* c, int32_t final_cut, const int32_t** dev_rows_out, int64_t* n_out);

/* The cluster table of a run goes to pinned host memory at its end (cl_boxes_host / cl_get_boxes); enabled = 0
 * skips that copy for the following runs (callers that only use cl_cand_append / the distance statistics). */
void cl_set_table_export(cl_chrom* c, int enabled);

/* Row-aligned device labels for runs WITHOUT a host destination (labels_out == NULL): enabled = 1 (default) keeps
 * producing them (for cl_labels_device); enabled = 0 skips the scatter to input-row order -- the sweep driver only
 * needs the cluster table and the distance statistics, which work on the sorted order. */
void cl_set_device_labels(cl_chrom* c, int enabled);

/* Enable (1) / disable (0) HIP-event timing of the kernels of subsequent runs. */
void cl_set_profiling(cl_chrom* c, int enabled);
int cl_get_timing(const cl_chrom* c, cl_timing* out);

/* ---- A sweep in one call -------------------------------------------------------------------------------------------------
 * The reference's driver runs `for ep in eps: for m in minPts:` over every chromosome (cLoops/pipe.py:241-281, the lists of a mode:
 * pipe.py:310-344).  A caller that is about to do the same tells the handle ONCE:
 *     cl_sweep_plan(c, eps, n_eps, min_pts, n_min_pts);
 * and then calls cl_cluster / cl_cluster_async / cl_cluster_step_async per (eps, minPts, cut) as before.  With the plan the handle
 * sorts its rows once for all announced eps (when they share a divisor), keeps the layout of an eps for its runs, makes the
 * neighbour counts of an eps once -- exact enough for every announced minPts -- and re-queries only the cut band of the later runs.
 * Results are identical with and without a plan; without one every run pays for itself.  n_eps = n_min_pts = 0 ends the plan.
 * (The plan is the announcement of the two lists: cl_set_sort_index(1) + cl_set_eps_list + cl_set_count_thresholds.  Layout reuse,
 * count reuse and the traversal level keep their values -- on / on / 4 unless the caller changed them.)
 * The cl_set_* entries below are the plan's parts, kept for tests and measurements (each documents what it switches); a caller
 * needs none of them. */
int cl_sweep_plan(cl_chrom* c, const int32_t* eps, int32_t n_eps, const int32_t* min_pts, int32_t n_min_pts);

/* Sorted-layout reuse (default: enabled).  The sorted order of a chromosome's PETs depends on eps only (not on
 * minPts; a cut only removes rows), and the sweep of cLoops/pipe.py:241-281 walks eps in its OUTER loop: with reuse
 * enabled the handle keeps the sorted arrays of the last eps and every further run at that eps starts from one
 * stable stream compaction by the cut (pipe.py:59-62) instead of a sort.  Results are identical either way; nothing
 * of a result is kept between runs.  enabled = 0: every run sorts for itself (used by benchmarks that repeat one
 * (eps, minPts) and must pay the whole run every time). */
void cl_set_layout_reuse(cl_chrom* c, int enabled);

/* The q index.  A run's sorted order is (strip, q) with ties in input-row order, and only the strip depends on eps.
 * A handle that sorts more than one layout (the eps loop of cLoops/pipe.py:241-281) keeps its rows sorted by q once
 * (12 B/PET, 4 radix passes) and gets every layout from a stable sort of that sequence by the strip bits alone
 * (2 passes instead of 5) -- the same permutation.  mode 0 (default): the index is built at the handle's second
 * sort, so a one-shot run never pays for it; 1: at the first sort (the sweep driver, which knows more eps are
 * coming); -1: never.  Results are identical in every mode. */
void cl_set_sort_index(cl_chrom* c, int mode);

/* Region-query reuse inside one eps (default: enabled; needs layout reuse).  The neighbour count of a PET
 * (cDBSCAN.py:186-205 regionQuery, cDBSCAN2.py:333-334) does not depend on minPts, and a cut (pipe.py:59-62) removes
 * only PETs whose distance is below it -- in the sorted layout a prefix of every strip -- so the count of a PET changes
 * between two runs of one eps only if its distance lies within eps above the larger of their cuts.  The sweep of
 * cLoops/pipe.py:247-250 walks minPts (descending) INSIDE eps: the handle keeps the per-PET words of the first run at
 * an eps (counts saturated at its minPts) and every later run at that eps with an announced minPts runs the region
 * query on the cut band alone; the other PETs' words are read in place.  Results are identical with enabled = 0
 * (every run does its own full region query).
 * cl_set_count_thresholds: the minPts values the caller will ask for at the current eps (the inner loop of
 * cLoops/pipe.py:247-250; the sweep driver knows its list; values outside 2..128 are ignored).  The first run then
 * keeps every count as exact as the tests `count >= minPts` of those values need it (a PET whose count is known to lie
 * between two neighbouring values of the list is not counted further).
 * cl_set_count_floor: the older, coarser form -- every minPts from min_pts up to the first run's is served (counts
 * exact from there up).  Either call replaces what the other announced; nothing announced (default) = only runs that
 * repeat the first run's minPts re-use its words.
 * cl_last_region_mode: what the last enqueued run did -- 0 full region query, 1 words re-used as they were (same
 * cut), 2 words carried through the compaction + region query on the band. */
/* cl_set_eps_list: the eps values the caller will ask for (the outer loop of cLoops/pipe.py:241-281; the sweep driver knows its
 * list).  When they share a divisor w >= 16 with max(eps) / w <= 8 (Hi-C mode 3: 5000 / 7500 / 10000 -> 2500) the handle sorts its
 * rows once by strips of width w; the layout of every announced eps is then a per-strip merge of that order (a strip of width
 * k w = k consecutive strips of width w) instead of a sort -- the same (strip, distance) order; PETs of one strip at EQUAL distance
 * follow each other by run instead of by input row, an order no result depends on.  n = 0 forgets the list. */
void cl_set_eps_list(cl_chrom* c, const int32_t* eps, int32_t n);
/* cl_chrom_drop_indexes: forget every order and count the handle has derived from its rows (q index, fine layout, the layout of the
 * last eps, cached neighbour counts); allocations stay.  The next run pays what the first run on a fresh dataset pays for its
 * sorts -- measurements of "one dataset, one sweep" (cLoops/pipe.py:247-275 sweeps a dataset once) without re-uploading. */
int cl_chrom_drop_indexes(cl_chrom* c);
void cl_set_count_reuse(cl_chrom* c, int enabled);
void cl_set_count_floor(cl_chrom* c, int32_t min_pts);
void cl_set_count_thresholds(cl_chrom* c, const int32_t* min_pts, int32_t n);
int cl_last_region_mode(const cl_chrom* c);
/* cl_base_rows: the rows the handle's current base layout holds (read-only).  Inside an announced sweep (cl_sweep_plan) a layout
 * that is built for a run under a cut leaves out the rows with Y - X below half of that cut -- every later run of the eps whose
 * cut is not below that floor treats them as absent anyway; a run below it (a smaller cut, no cut, exact counts) rebuilds the
 * layout with every row.  Results never depend on it.  n when the handle holds no layout or the layout holds every row. */
int64_t cl_base_rows(const cl_chrom* c);

/* How the part of a rotated run behind the region query (components, border rule, labels) walks the data.  The reference
 * expands clusters from core points only (cDBSCAN2.py:114-192 queryGrid, cDBSCAN.py:155-184 expandCluster); levels 3 and 4
 * do the same: the run's cores and its non-core PETs that have a neighbour are compacted into two lists right behind the
 * region query and nothing else is touched again -- level 3 from a copy of the layout compacted by the run's cut, level 4
 * (DEFAULT) straight from the eps' base layout (a cut removes a prefix of every strip: nothing is copied, the count cache
 * lives in base positions).  Levels 0..2 keep the LDS-tile kernels over every PET of the run for the components (0), the
 * border rule (<= 1) and the labels (<= 2).  Results are identical at every level (the tests compare all five); values
 * outside 0..4 are clamped. */
void cl_set_traversal(cl_chrom* c, int level);

/* A HIP stream for cl_chrom_create(..., stream, ...) made by the library (for callers without a HIP binding of their
 * own, like the ctypes host side).  Several handles may share one stream: their runs then execute in enqueue order in
 * that stream; their D2H copies go through ONE copy stream that belongs to the stream (made when the first handle has
 * labels to copy), behind an event of the run, so that a run's labels cross PCIe while the next handle's kernels
 * execute.  (A handle on a stream the caller made otherwise issues its copies in that stream; a handle with a stream of
 * its own -- stream == NULL at creation -- overlaps them with its next run through a copy stream of its own.)  Make the
 * streams before anything else that makes streams: the runtime deals its hardware queues in creation order.  The sweep driver keeps a few shared streams per
 * device instead of one per chromosome: how many kernels run side by side is then the application's choice, not a
 * property of how the runtime maps dozens of streams onto its hardware queues.  Destroy a stream after its handles. */
void* cl_stream_create(int device);
/* cl_chrom_set_stream: move an idle handle (no run in flight) that was created on a caller's / library-made stream to another
 * stream of the same device -- the sweep driver balances its chromosomes over its shared streams when a sweep starts (a handle is
 * bound to a stream when it is uploaded, long before the set of chromosomes of a sweep is known).  Waits for the handle's old
 * stream.  CL_ERR_ARG for a handle with a stream of its own (stream == NULL at creation) or a NULL stream. */
int cl_chrom_set_stream(cl_chrom* c, void* stream);
void cl_stream_destroy(void* stream);

/* Page-locked host memory for result buffers (labels_out / boxes_out / counts_out): D2H
 * copies into pinned memory run at PCIe rate instead of through a staging buffer.  Plain
 * malloc'ed memory works everywhere too, only slower. */
void* cl_host_alloc(int64_t bytes);
void cl_host_free(void* p);

/* A new chromosome handle made of `m` rows of a resident one, in the order given (rows may repeat): what
 * scripts/jd2saturation:32-55 does with `mat[ns, :]` + joblib.dump for every re-sampling depth -- here the rows are
 * gathered on the device, only the row list crosses PCIe.  The new handle is independent of `src` (own device memory,
 * own stream); destroy it with cl_chrom_destroy. */
int cl_chrom_subsample(cl_chrom* src, const int64_t* rows, int64_t m, cl_chrom** out);

/* Testing hook: the per-PET workspace of a handle is reserved as ONE allocation when the chromosome is uploaded (best
 * effort: if that allocation fails the buffers are allocated one by one at the first run).  extra_bytes > 0 is added to
 * the size of that allocation for the handles created afterwards, so that a test can make it fail; 0 restores it. */
void cl_debug_arena_overcommit(int64_t extra_bytes);

/* Library version: major*10000 + minor*100 + patch. */
int cl_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CLOOPS_HIP_H */
