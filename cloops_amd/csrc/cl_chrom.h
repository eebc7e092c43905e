// cl_chrom.h -- host side shared by the translation units: what one call asks for (RunRequest), the chromosome handle (device
// buffers, result slots, sweep state), the structures the step tail exchanges with the K7 / K10 kernels, and the functions /
// kernels one unit uses from another.  A __global__ function may be launched from a unit that only sees its declaration: the
// launch goes through the defining unit's host stub.
//
// Three kinds of thing, kept apart:
//   RunRequest      what the caller of ONE run asked for.  The entry point builds it, enqueue() and the run functions take it by
//                   reference; nothing of it is stored in the handle (the run's record notes where its output goes).
//   cl_chrom::Run   the working set of the run BEING ENQUEUED (c->run): where its sorted arrays and K2 words live, its traversal
//                   level, what its kernels have done already, and the record it will leave in its result slot (Run::held).  Assigned
//                   fresh by run_begin() at the start of every run, read by nobody after the enqueue (the developer build's
//                   cl_debug_time_lists aside).  finish_enqueue() commits the record to the slot in one assignment once the run is
//                   completely enqueued; nothing else writes a slot's record (finish_wait() clears the destination it has served).
//   Base, Counts, Fine, Kde, Sig, Cand and K12 .. K30
//                   state that outlives a run: one struct each, the buffers together with the flags that say what they hold, and
//                   one invalidate() where several flags fall together.
// What reports on the LAST run (last_k2_mode, dbg_g / dbg_nm, refused_labelled, the slots' records) stays in the handle: callers
// read it after the enqueue.
#pragma once
#include "cl_common.h"
#include "cl_table.h"
#include "cl_prim.h"
#include "cl_textout.h"

#define BIGTPB 1024
#define AGG_H 512
// slot of `key` in a workgroup's LDS hash table of AGG_H keys (-1 = table crowded: the caller goes to global memory)
__device__ __forceinline__ int agg_slot(int* keys, int key)
{
    unsigned h = ((unsigned)key * 2654435761u) >> 23;            // 9 bits
    for (int probe = 0; probe < 24; ++probe) {
        const int old = atomicCAS(&keys[h], -1, key);
        if (old == -1 || old == key) return (int)h;
        h = (h + 1) & (AGG_H - 1);
    }
    return -1;                                                    // table crowded: caller goes to global memory
}
#define FLAT_PER 4          // PETs per thread
struct Stats { int amin, amax, vmin, vmax, xmin, xmax, ymin, ymax; };
__device__ __forceinline__ int je_minus(const int* __restrict__ cstart, int j) { return cstart[j + 1] - cstart[j]; }
static inline int bits_for(unsigned v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }


#define CL_FINE_KMAX 8           // most runs per strip a layout is merged from (cl_set_eps_list)
#define K7_BLOCKS 2048           // workgroups (= fixed partial sums) of the K7 reductions: 8 waves per SIMD (512 left the loads
#define K7_STEP_BLOCKS 256       // ... of the sweep step's k7_summary: 1024 threads each (every workgroup ends with up to 5 888 atomics into the two
#define K7_STEP_THREADS 1024      //     histograms -- 2048 x 256 threads: 67 us per chr1 step, 256 x 1024: 47 us)
#define K7_LOGBINS 3840          // 30 octaves x 128: bin = floor(log2 d) * 128 + the next 7 bits of d (monotone in d)
__device__ __forceinline__ int k7_logbin(unsigned d)      // d >= 1 (shared by K7 in k_sweep.hip and K23 in k_kdis.hip)
{
    const int e = 31 - __clz((int)d);
    const unsigned m = e >= 7 ? ((d >> (e - 7)) & 127u) : ((d << (7 - e)) & 127u);
    return e * 128 + (int)m;
}
#define K7_FINE 2048
#define K7_XSHIFT 11.0           // sums are taken over x = log2|d| - K7_XSHIFT (less cancellation in sum x^2 - (sum x)^2 / n)
#define CAND_BLOCK 2048

struct K7Src {
    int sorted;                                         // 0 = input rows, 1 = the run's sorted arrays, 2 = the run's lists (sv / slab hold one entry per core and
                                                        // walker, dM their number)
    int n; int M; int v0;
    const int* dM;                                      // if set: M is read from the device (the run has not been waited for yet)
    const int* X; const int* Y; const int* labels;      // input rows (+ row-order labels)
    const int* sv; const int* slab;                     // sorted q and sorted-order labels of [0, M)
    const int* dh;                                      // if set: dh[d] = number of input rows with Y - X == d for 0 <= d < cut, and no row has
                                                        // Y - X < 0: the PETs dropped by the cut come from it, not from a pass over the rows
};

struct K7Part { double sx[2]; double sxx[2]; long long n_all[2]; long long n_pos[2]; };

// The header of a result slot, HDR_WORDS ints on the device (cl_chrom::hdr), the first eight copied to the slot's pinned h_hdr: ids
// handed out, internal error (0: none), PETs that entered DBSCAN, non-empty ids and the largest of them (k_export_table; -1: none),
// 1 = the pinned table rows were too few, labelled PETs handed out as pairs / under the row mask
enum { HDR_K = 0, HDR_ERR = 1, HDR_M = 2, HDR_NCLUSTERS = 3, HDR_MAXLABEL = 4, HDR_TRUNC = 5, HDR_LABELLED = 6, HDR_WORDS = 16 };
// values of HDR_ERR (the device counter CTR_OVERFLOW); any other non-zero value: the release records overflowed
enum { HDR_ERR_STRIP = 4 /* strip longer than the hybrid sort accepts */, HDR_ERR_COUNT = 8 /* M differs from the host's count */ };

// What one call asks of the handle.  cl_cluster, cl_cluster_async, cl_cluster_pairs_async, cl_cluster_rowmask_async,
// cl_cluster_step_async and cl_cluster_weighted each build one and hand it to enqueue() (cloops_hip.hip)
struct RunRequest {
    int variant = CL_VARIANT_CDBSCAN1, eps = 0, minPts = 0, cut = 0;
    int32_t* labels_out = nullptr;    // row-aligned labels to the host (pinned or pageable), or null
    int2* pairs_out = nullptr;        // cl_cluster_pairs_async: (row, label) of every labelled PET, staged by the label kernel in the slot's
    long long pairs_cap = 0;          // device buffer and copied by cl_wait into the caller's page-locked buffer (their count: header word 6)
    void* mask_out = nullptr;         // cl_cluster_rowmask_async: one bit per row + the labels of the set rows in row order, made on the device from the
    long long mask_cap = 0;           // row-aligned labels (k_rowmask_count / k_rowmask_write) in the slot's `pairs` buffer, copied out by cl_wait like the pairs
    int step = -1;                    // >= 0: the run is step `step` of a sweep (cl_cluster_step_async), -1: it is not
    long long fine_lo = -1;           // >= 0: the step's summary also histograms the self group's [fine_lo, fine_lo + 2048) exactly
    int wx = 0, wy = 0;               // cl_cluster_weighted: the metric's weights (0: not the weighted form)
};

struct cl_chrom {
    long long tmp_n = -1;             // n the rocPRIM temporary storage was last sized for
    DevBuf arena;                     // ONE allocation behind the per-PET workspace of the handle (ensure_workspace): the first
                                      // run of a handle pays one hipMalloc instead of forty.  The buffers that adopt a slice of it
                                      // do not own it and never free it, so the order in which the members die does not matter
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int64_t n = 0;
    int *d_x = nullptr, *d_y = nullptr;
    bool own_xy = false;
    Stats st{};
    // workspace
    DevBuf keys_in, keys_out, vals_in, vals_out, sort_tmp, scan_tmp;
    DevBuf qb_key, qb_val;            // the q index (k_make_qkeys): rows sorted by q, persistent
    int qindex_layout = -1;           // layout the q index was built for (-1: none)
    // the fine layout (cl_set_eps_list): rows sorted by (strip of width w, q) once; the layout of an eps = k w is a per-strip merge of it
    struct Fine {
        DevBuf q, sp, row, strip;
        DevBuf dead;                  // a layout with a floor: per fine strip the rows below it, and their exclusive sums
        int w = 0;                    // announced common divisor of the sweep's eps values (0: none)
        int valid_w = 0, layout = -1; // what the buffers hold
        GridParams g;
        void invalidate() { valid_w = 0; layout = -1; }
    } fine;
    int sort_index_mode = 0;          // cl_set_sort_index: 0 = build at the second sort, 1 = at the first, -1 = never
    long long n_sorts = 0;            // layouts sorted on this handle so far
    DevBuf sv, sa, strip, cnt, parent, root, head, headidx, cellfirst, compkey, ncore, bsize, owner, state;
    DevBuf flag, rankscan, ulist, lo, hi, recs, counters, chainflag, chainhead, usize, b_cstart, b_ckey, b_nb, b_cx, b_cy, tile_s0;
    int* h_pinned = nullptr;          // small pinned staging (stats, block scalars)
    struct StripPlan { int layout, eps, maxlen; };
    std::vector<StripPlan> plans;     // longest strip over all rows per (layout, eps): picks the sort path
    // The record of ONE run in its result slot (Slot::held, below); the defaults are those of a run that sets nothing
    struct Held {
        int32_t* labels_out = nullptr;
        // the pairs (kp (row, label) of 8 bytes) or the row mask (ceil(n / 64) words, then kp labels): cl_wait copies `fixed` + kp * `per`
        // bytes from the slot's `pairs` to the caller once the header tells the number kp of labelled PETs
        struct Extra {
            void* dst = nullptr;          // the caller's page-locked buffer (null: the run has no such output)
            long long cap = 0;            // its capacity in labelled PETs: cl_wait refuses a run that labelled more
            size_t fixed = 0; int per = 0;
            bool copy_empty = false;      // kp == 0 still copies (the fixed part)
            const char* refusal = nullptr;    // cl_wait's error text for a run that labelled more than `cap`
        } extra;
        int n_strips = 0;
        bool band_timed = false;      // ev[8], ev[9] were recorded
        long long n_queried = 0;      // PETs the run's region query covered (0: none)
        bool exported = false;        // the table rows were stored to h_boxes
        bool step_valid = false;      // the run carried the sweep-step tail (classification, candidate append, distance summary)
        bool host_written = false;    // ... and its last kernel stored header + step output in pinned host memory itself
        bool wait_done = false;       // cl_wait waits for ev_done (nothing went through the copy stream)
        long long fine_lo = -1;       // fine window of that tail's summary (-1 = none)
        bool rows_valid = false;      // `labels` (row order) was produced by the run
        bool sorted_src = false;      // the run left sorted (q, label) arrays for the distance statistics
        const int* k7_sv = nullptr;   // sorted q of the run (list form: q of every core and walker)
        const int* k7_lcnt = nullptr; // list form (k_lists.hip): device {cores, walkers} -- slab / k7_sv hold one entry per core and walker
        int k7_v0 = 0;                // d = q + k7_v0
    };
    // Working set of the run being enqueued.  run_begin() assigns a fresh one first thing in run_rotated, run_block, run_weighted and
    // cl_neighbor_counts: no run sees what an earlier one -- of whatever kind, finished or failed half-way -- left here.
    struct Run {
        u32* srow = nullptr;          // sorted position -> input row
        // sorted (q, sp), strip table, tile table: they alias either the workspace buffers (sv, sa, strip, tile_s0) or, for a run
        // without cut filter, the base layout itself
        int *sv = nullptr, *sa = nullptr, *strip = nullptr, *tile = nullptr;
        int* cnt = nullptr;           // where K2 writes the run's words (the work buffer or the count cache)
        WordSrc ws{};                 // where their consumers read them
        int init_nclr = 0;            // > 0: the run has not cleared its key bitmap / counters yet (words to clear)
        int level = 0;                // traversal level (run_sort_and_count decides: level 4 needs the count cache's tables)
        const int* dM = nullptr;      // device: PETs that entered DBSCAN
        int m = 0;                    // ... on the host (exact when m_exact, else n)
        bool m_exact = false;
        bool rows = true;             // the run produces row-aligned labels
        bool l4_make_base = false;    // level 4: the run makes the words of its eps -- K2 on the base layout, launched behind the band query
        bool l4_cut = false;          // level 4: the run has a cut (the per-strip tables of k_cut_strips apply)
        bool l4_band = false;         // ... and re-uses counts under another cut (the band's words are fresh: c->cnt, by run position)
        bool k2_make = false;         // the run made the words itself (level 4 under a cut: on the base layout, then its band)
        const int* k_total = nullptr; // device: where the run left the number of ids handed out (null: rankscan[n])
        bool hdr_packed = false;      // the run's own kernels have written the slot header (no k_pack_header)
        int kmax = 0;                 // upper bound of the number of cluster ids of the run (host-known; the count itself is on the device)
        Held held;                    // the record the run will leave in its slot (finish_enqueue completes and commits it)
    } run;
    // Base layout: the sorted arrays of ALL rows (cut = 0) for one (variant layout, eps), kept until eps changes.
    // The sort order does not depend on minPts and a cut only REMOVES rows, so every further run of a sweep at this
    // eps is one stable stream compaction of the base layout instead of five radix passes (cLoops/pipe.py:241-281
    // walks eps in the outer loop).  Nothing of a result is kept: neighbour counts, components, labels are redone.
    // ... and variant 2's cell minima of it (key: traversal level 4, once per eps)
    // Inside an announced sweep a layout that is built for a run under a cut leaves out the rows far below that cut (floor_q > 0:
    // the rows with q < floor_q, a prefix of every strip -- exactly what a cut removes): every later run of the eps whose
    // threshold is >= floor_q treats those rows as absent anyway, and no pass over base positions reads them again.  A run below
    // the floor (a cut that fell, no cut, exact counts) rebuilds the layout with floor 0 (run_sort_and_count).
    struct Base {
        DevBuf q, sp, row, strip, tile, key;
        bool valid = false; int layout = -1, eps = 0;
        bool key_valid = false;       // `key` belongs to the layout
        int floor_q = 0;              // the layout holds the rows with q >= floor_q only (0: all rows)
        int rows = 0;                 // ... their number: the base positions are [0, rows)
        long long pad_rows = -1;      // `rows` the sentinel pads behind q / sp were last written for (-1: never)
        void invalidate() { valid = false; key_valid = false; floor_q = 0; }
    } base;
    bool sweep_planned = false;       // cl_sweep_plan announced a sweep (a non-empty eps list): its layouts may carry a floor
    DevBuf sel_tmp;
    // Count cache: the K2 words (cl_common.h "K2W") of the FIRST run on a base layout, kept while the layout lives.  A word
    // holds the PET's neighbour count (saturated at `cap`, exact as far as the minPts values of `tmask` need it: GridParams::tmask) and does not depend on minPts otherwise;
    // a cut removes a prefix of every strip (q IS the distance), so between two runs of one eps the count of a PET changes
    // only if q - eps < max(the two cuts): every later run with a minPts of the set takes the words of the PETs beyond that
    // band as they are (k_cut_copy<true> carries them through its compaction) and runs K2 on the band alone.  Results are
    // identical with the cache switched off (cl_set_count_reuse); cLoops/pipe.py:247-250 walks minPts inside eps, descending.
    struct Counts {
        bool valid = false;
        bool cut_on_base = false;     // made on the base layout by a run under a cut: the PETs within eps above thr counted removed
                                      // neighbours -- every run under a cut re-queries its band
        bool base_space = false;      // level 4: words by base position, hints in base positions (k_lists.hip)
        int layout = -1, eps = 0, thr = 0 /* q threshold of the run's cut, 0 = none */, cap = 0;
        u32 tmask[4] = {0, 0, 0, 0};  // the minPts values the words serve, bit t - 1
        DevBuf cnt, pre, poff, dpre, D, blen;   // the words in the sorted order of the run that made them; per strip: PETs its cut removed
                                      // from the strip / from all strips up to and including it
        void invalidate() { valid = false; }
    } rc;
    bool reuse_counts = true;         // cl_set_count_reuse
    int count_floor = 0;              // cl_set_count_floor: smallest minPts later runs of this eps will ask for (0 = unknown)
    u32 count_tmask[4] = {0, 0, 0, 0}; // cl_set_count_thresholds: the minPts values themselves (bit t - 1; all zero = not announced)
    DevBuf blk_tmp;                   // block sums / offsets of the in-kernel scan over the key bitmap (k_rank_scan)
    DevBuf rootlist, cflag8;          // K3: the components' roots (k_flatten); per PET: core / opens a chain / ends one (k_chain_flags)
    // List form of a run (k_lists.hip): the run's CORES and its WALKERS (non-core PETs with a neighbour: the only ones a border
    // rule can label) as compact arrays in sorted order, plus a rank index over the run's positions (one bit per PET and the
    // exclusive core / walker count in front of every 64-PET group), so that any position range of the layout maps to a
    // contiguous range of the core array in O(1).  K3 / K4 / K5 then touch nothing else.
    DevBuf l_mask, l_rank, l_blk, l_cstrip, l_wpos, l_wenc, l_dist, l_aux;
    // ... built straight from the BASE layout (traversal level 4): a cut removes a prefix of every strip, so the list kernels
    // apply it by index (per strip: first kept base index, end of the cut band, PETs removed: l_tab) and a re-using run
    // copies nothing at all; variant 2's cell minima are a property of the base layout (base.key, once per eps) except in the one
    // cell per strip the cut goes through (l_fix, per run)
    DevBuf l_tab, l_fix;
    bool pairs_defer = false, pairs_copy_pending = false;      // cl_set_pairs_defer / cl_pairs_sync
    bool fuse_chains = true;          // the chains of a run are made inside k_union_c (false: k_chain_c, a kernel of its own -- developer A/B)
    bool l_sup_dirty = false;         // k_classify's superblock sums may be non-zero (a run that failed between k_classify and k_chain_c)
    GridParams dbg_g{}; int dbg_nm = 0;   // the last rotated run's grid and size (developer build: kernels timed on their own)
    int traversal = 4;                // cl_set_traversal: 0 = tile kernels over every PET (rounds 1-4), 1 = K3 on the core list,
                                      // 2 = + border rule on the walker list, 3 = + labels / table / statistics from the lists,
                                      // 4 = + the lists built from the base layout (no copy of the layout for a run that re-uses counts)
    int last_k2_mode = 0;             // 0 = full K2, 1 = words re-used as they are (same cut), 2 = remapped + K2 on the band
    std::vector<long long> dcum;      // dcum[k] = number of PETs with Y - X < k, k = 0 .. 65536 (empty: unknown)
    DevBuf dhist;                     // device: number of PETs with Y - X == d, d = 0 .. 65535 (+ one slot for d < 0)
    long long n_neg = 0;              // PETs with Y - X < 0
    bool reuse_layout = true;
    // Result slots: two runs may be in flight (cl_cluster_async) -- the labels / table / header of
    // run k live in slot k & 1, so the D2H copy of run k (copy stream) overlaps the kernels of run k+1.
    // A slot is RESOURCES (buffers, events, pinned memory: they live as long as the handle and are used while a run is enqueued) and
    // the RECORD `held` of the run it holds.  A run builds its record in c->run.held; finish_enqueue() commits it in ONE assignment,
    // the last act of an enqueue that succeeded, and nothing else writes it (finish_wait() clears the host destination it has
    // served): a run that fails leaves the slot describing the last run completely enqueued there, cl_neighbor_counts writes none.
    struct Slot {
        DevBuf labels, table;         // row-order labels and the cluster table of the run
        DevBuf slab;                  // labels in sorted order (rotated variants)
        DevBuf pairs;                 // the output a run's cl_wait copies to the caller (Held::Extra), staged on the device: its size is only
                                      // known when the run has completed
        DevBuf d_step;                // device: {n_inter, n_self} + K7 partials + log histogram of a sweep step's tail
        hipEvent_t ev_done = nullptr, ev_copied = nullptr;
        hipEvent_t ev[10]{};          // profiling marks of the run that used this slot (8, 9: around the band query of a level-4 run)
        int* h_hdr = nullptr;         // pinned: the slot header (HDR_K ...)
        char* h_step = nullptr;       // pinned host copy of d_step
        cl_box* h_boxes = nullptr;    // pinned host copy of the cluster table
        size_t h_boxes_cap = 0;
        bool pending = false;         // a run has been enqueued here and not been waited for
        Held held;                    // what the run that the slot holds left here (cl_chrom::Held)
    } slot[2];
    bool device_labels = true;        // produce row-order device labels even without a host destination (cl_set_device_labels)
    bool export_table = true;         // copy the cluster table to pinned host memory at the end of a run (cl_set_table_export)
    // K10: candidate loops of the running sweep (boxes, their steps, the keep flags and the output of cl_cand_finish)
    struct Cand { DevBuf box, step, keep, out; long long n = 0, cap = 0; } cand;
    DevBuf hdr;                       // device result headers, 16 ints per slot
    DevBuf k7_cls, k7_parts;          // K7: class per cluster id, per-workgroup partials
    // K17 (k_sweep.hip): the (|d|, weight) entries of the two distance groups as cl_dist_collect appended them (group 0 from the
    // front, group 1 from the back of ONE buffer of `cap` entries) and sorted, counters, sort scratch, the evaluation's partials
    struct Kde {
        DevBuf ent, sorted, ctr, tmp, part;
        int run = -1;                 // `deq` at the cl_dist_collect that filled them (-1: none): valid while no further run completes
        long long cap = 0, cnt[2] = {0, 0};
    } kde;
    // K8: sorted PET tables (built for `cut` when ready), sort scratch, their number, windows, counts
    struct Sig { DevBuf tx, ty, tmp, sorttmp, m, win, out; bool ready = false; int cut = 0; } sig;
    // ---- the analysis units: one struct each, released by assigning a fresh one (the unit's *_release) ----
    // K12 (k_fingerprint.hip): scratch of one call, freed when it returns
    struct Fp { DevBuf small, keys, sorted, tmp, pairs; } fp;
    // K13 (k_anchor.hip): anchors, directory, row mask, workgroup totals; kept between calls
    struct Anchor { DevBuf s, e, dir, mask, wsum; } an;
    // K19 (k_agg.hip): the rows that pass `cut` sorted by X (keys in / out, Y in / out, sort scratch, their number), the loop
    // centres and their order by cx (keys in / out, numbers in / out, sort scratch), the sum, per-loop statistics and matrices; kept
    // between calls
    struct Agg {
        DevBuf kin, vin, sx, sy, tmp, m, cx, cy, lkin, lkout, lvin, order, ltmp, sum, stats, mats;
        bool ready = false; int cut = 0, kept = 0;                   // the table is built for `cut` and holds `kept` rows
    } ag;
    // K14 (k_track.hip): tile counts / offsets, kept rows, keys, scratch, ids, names; the text itself (line lengths / ends, chunk
    // bounds, render output: cl_textout.h); kept from cl_track_build to the next build, cl_track_free or destruction
    struct Track {
        DevBuf tcnt, toff, row, keys, sorted, tmp, ids, names;
        TextOut txt;
        struct State {
            bool built = false, ids = false;
            int kind = 0, la = 0, lb = 0, gbits = 0;
            long long cut = 0, ext = 0;
        } st;
    } tk;
    // K20 (k_cover.hip): the sorted end-point keys (in / out, sort scratch), per candidate break point its depth after / before and
    // its rank among the other side's candidates, the run-start flags and their scan, counters, the runs (start, end, depth), the
    // name; the text of the runs (cl_textout.h); kept from cl_cov_build to the next build, cl_cov_free or destruction
    struct Cov {
        DevBuf kin, key, tmp, dcur, dprev, xr, flag, scan, ctr, start, end, depth, name;
        TextOut txt;
        struct State {
            bool built = false, text = false;
            int la = 0;
            long long R = 0, num = 0, den = 0;                           // runs; the scale of their text (cl_cov_text)
        } st;
    } cv;
    // K21 (k_peak.hip): the sorted end-point keys (in / out, sort scratch), per element the ranks of its window's two edges, the core
    // flags and their scan, the chain-head flags and their scan, per peak the indices of its first / last core and the four results,
    // counters; the intervals of a count / summit call with their results; kept from cl_peak_sort to the next sort, cl_peak_free or
    // destruction
    struct Peak {
        DevBuf kin, key, tmp, lo, hi, flag, C, head, H, a, b, start, end, np, nc, ctr, ivs, ive, best, opos, ocnt;
        struct State {
            bool sorted = false, called = false;
            int base = 0;                                                // the value of key 0
            long long m = 0, P = 0;                                      // end points; peaks of the last cl_peak_call
        } st;
    } pk;
    // K22 (k_domain.hip): the three difference arrays over the bins (n_bins + 1 entries each) and their scans (cross, up, down: n_bins
    // entries each), the scan's scratch, the range of the kept rows' coordinates; the intervals of a count call and their three
    // counters.  The rows themselves are K19's X-sorted table (ag.sx / ag.sy / ag.kept, agg_table), shared.  Kept from cl_dom_tracks
    // to the next one, cl_dom_free or destruction
    struct Dom {
        DevBuf diff, trk, tmp, rng, ivs, ive, cnt;
        struct State {
            bool ready = false;
            int cut = 0, res = 0, w = 0;
            int pmin = 0, pmax = 0;                                      // smallest / largest coordinate of the kept rows (of `cut`)
            long long bmin = 0, n_bins = 0, n_kept = 0;
        } st;
    } dm;
    // K23 (k_kdis.hip): X, Y of the kept rows in table order (copies: cl_agg_loops at another cut may rebuild K19's table while the
    // results live), d_k of every row for every asked k (n_k arrays of n_kept), per k the histogram + n_zero + n_none.  Kept from
    // cl_kdis_build to the next build, cl_kdis_free or destruction
    struct Kdis {
        DevBuf x, y, d, hist;
        struct State {
            bool ready = false;
            int cut = 0, n_k = 0;
            int ks[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            long long n_kept = 0;
        } st;
    } kd;
    // K24 (k_matrix.hip): the dense output of a window / virtual-4C call, the table ranges and counters of a call, and for the cells
    // the keys (in / sorted, sort and scan scratch), head flags, their scan, the run starts and the result (bx, by, cnt of every cell:
    // copies, so cl_agg_loops at another cut does not disturb them).  The rows are K19's table, shared.  The cells are kept from
    // cl_mat_cells to the next one, cl_mat_free or destruction
    struct Mat {
        DevBuf out, ctr, key, sorted, tmp, flag, scan, start, bx, by, cnt;
        struct State {
            bool ready = false;
            long long n_cells = 0, n_kept = 0, max_count = 0;
            int res = 0; bool fold = false;                              // what the cells were made with (K25 refuses unfolded cells)
        } st;
    } mx;
    // K25 (k_balance.hip): the transposed order of K24's folded cells (sort scratch, then by / bx / cnt of every cell ascending by
    // (by, bx)), the integer marginals (sum, nnz per bin), the caller's mask, the weights w, the marginals s of an iteration, the
    // per-tile carry records of both orders (integer and fp64), the partial sums of the update's reduction, the 32-byte record of a
    // loop and the balanced values of a get.  Kept from cl_bal_marginals to the next cl_mat_cells, cl_mat_free, cl_bal_free or
    // destruction
    struct Bal {
        DevBuf kin, kout, vin, vout, tmp, tby, tbx, tcnt, sum, nnz, valid, w, s, icar, dcar, part, rec, out;
        struct State {
            bool ready = false, iterated = false;
            int ignore_diags = 0;
            long long b0 = 0, nb = 0, n_used = 0, n_cells = 0;
        } st;
    } bl;
    // K26 (k_expected.hip): the effective weight of every bin (the ICE weight, or 1 on the caller's valid bins; NaN on the others) and
    // the mask of the valid bins, one bit per bin; the diagonal order of the cells (sort scratch, then d = by - bx, bx - b0 and cnt of
    // every cell ascending by d, inside a diagonal as the cells lie) and the tiles' carry records; per diagonal the valid pairs, the
    // count sum and the value sum; the expected values of cl_exp_set; the O/E values of a get.  Kept from cl_exp_diagonals to the next
    // one, cl_exp_free, anything that releases or rebuilds K25's state (bal_release, cl_bal_marginals, cl_bal_iterate) or destruction
    struct Exp {
        DevBuf valid, w, mask, kin, kout, vin, vout, tmp, dk, dx, dc, car, ctr, pairs, cnt, val, exp, out;
        struct State {
            bool ready = false, expected = false;                        // the diagonals are built; cl_exp_set has been called since
            int balanced = 0;
            long long nd = 0, n_used = 0;
        } st;
    } ex;
    // K27 (k_eig.hip): the value of every cell inside the band in both orders (min(O/E, clip), 0 outside), the row pointers of both
    // orders, the prefix sums of a block inside the scan's tiles, the tile totals and their exclusive sums, the counter of the cells
    // inside the band; the blocks of the iteration (Q, Z, Y, the first pass of an orthonormalisation, the Ritz vectors), the partial
    // sums of its reductions, the 8 x 8 coefficients and the loop's record, the result vectors; the staging and the two blocks of a
    // cl_eig_apply.  Kept from cl_eig_build to the next one, cl_eig_free, anything that releases or rebuilds K26's state (exp_release,
    // cl_exp_diagonals, cl_exp_set) or destruction
    struct Eig {
        DevBuf val, rows, pl, tot, ctr, q, part, sm, vec, io, ax;
        struct State {
            bool built = false, iterated = false;                        // M is described; cl_eig_iterate has run since
            double clip = 0.0;
            long long dmax = 0, n_valid = 0, n_in = 0;
            int n_eigs = 0;                                              // the vectors cl_eig_vectors_get serves
        } st;
    } eg;
    // K28 (k_scc.hip): the band forms of this handle's and the other handle's matrix (nb x (D + 4h) u32 each; tb unused when a sample is
    // compared with itself) and the six accumulators per diagonal.  Scratch of the first handle of cl_scc_moments, reused when large
    // enough; kept to cl_scc_free, the next cl_mat_cells, cl_mat_free or destruction.  Nothing is kept on the second handle
    struct Scc {
        DevBuf ta, tb, acc;
    } sc;
    // K29 (k_dots.hip): the value band (nb x (dmax + 4w) fp64), the four planes of la over the dense nb x (dmax - dmin) pixels and the
    // plane of their raw counts, counters; the edges and the histogram of cl_dot_hist; the thresholds, the cells' flags, their scan (and
    // its scratch) and the significant cells of cl_dot_call; the la of a cl_dot_cells_get.  Kept from cl_dot_lambdas to the next one,
    // cl_dot_free, anything that releases or rebuilds K26's state (exp_release, cl_exp_diagonals, cl_exp_set) or destruction
    struct Dot {
        DevBuf band, la, pix, ctr, edges, hist, thr, flag, scan, tmp, sig, out;
        struct State {
            bool lambdas = false, hist = false, called = false;          // cl_dot_lambdas / cl_dot_hist / cl_dot_call have run since
            int p = 0, w = 0, n_chunks = 0;
            long long dmin = 0, dmax = 0, n_sig = 0;
        } st;
    } dt;
    // K30 (k_saddle.hip): the effective class of every bin (-1: invalid or without a class), the per-tile class counts of the pair
    // counts and their exclusive sums, the per-chunk tables of the sums (fp64 sums, then cell counts), the three folded tables; the
    // tables of the last cl_sad_sums on the host, where cl_sad_get reads them.  Kept from cl_sad_sums to the next one, cl_sad_free,
    // anything that releases or rebuilds K26's state (exp_release, cl_exp_diagonals, cl_exp_set) or destruction
    struct Sad {
        DevBuf cls, th, tb, part, out;
        struct State {
            bool ready = false;
            int n_cls = 0;
            long long lo = 0, hi = 0, n_binned = 0, n_pairs = 0, n_in = 0;
            std::vector<double> sum;
            std::vector<long long> pairs, cells;
        } st;
    } sd;
    bool k7_classified = false;       // k7_cls matches the last completed run
    hipStream_t copy_stream = nullptr, aux_stream = nullptr;
    int copy_mode = 0;                // 0: the D2H copies of a run go through copy_stream, 1: they are issued in `stream` (caller's stream),
                                      // 2: through the copy stream that cl_stream_create made for `stream` (shared by its handles)
    hipStream_t shared_copy = nullptr;
    int enq = 0, deq = 0;             // runs enqueued / completed
    int cur = 0;                      // slot of the run being enqueued
    // last completed result
    int last_slot = -1;
    int last_K = 0;                   // max_label + 1
    bool have_result = false;
    long long refused_labelled = -1;  // labelled PETs of the run whose cl_wait was refused for capacity (pairs / row-mask form); -1: the last wait refused nothing
    // profiling
    bool profiling = false;
    cl_timing timing{};
    bool ev_ready = false;
    float ev_bracket_ms = 0.f;        // event bracket around an empty kernel (calibration, see cl_timing)
};


#define LAUNCH(kernel, nthreads, ...) \
    hipLaunchKernelGGL(kernel, dim3(nblocks(nthreads)), dim3(TPB), 0, c->stream, __VA_ARGS__)

// first thing of every run (run_rotated, run_block, run_weighted, cl_neighbor_counts): a fresh working set
static inline void run_begin(cl_chrom* c) { c->run = cl_chrom::Run(); }
// base positions of the current base layout (all rows, or those above its floor)
static inline int base_rows(const cl_chrom* c) { return c->base.valid ? c->base.rows : (int)c->n; }
// the floor of a layout built under cut `c` is the distance c * CL_FLOOR_NUM / CL_FLOOR_DEN: the chained cuts of a sweep never
// fell below 0.6 of an earlier one (docs/history_r1-r4.md), and nearly all rows below a Hi-C cut lie below half of it too
#define CL_FLOOR_NUM 1
#define CL_FLOOR_DEN 2

// A run that fails half-way (allocation, a HIP error between two launches) must not leave state behind that a later run would
// trust: the count cache it may have marked valid before its words were written, the tickets of the in-kernel scans and the
// superblock sums of the list kernels (all "zero between kernels").  Disarmed by the run that reaches its end.
struct RunGuard {
    cl_chrom* c; bool armed = true;
    explicit RunGuard(cl_chrom* cc) : c(cc) {}
    ~RunGuard()
    {
        if (!armed) return;
        c->rc.invalidate();
        c->l_sup_dirty = true;
        if (c->counters.p) (void)hipMemsetAsync(c->counters.as<int>() + CTR_TICKET_A, 0, 8, c->stream);
        (void)hipGetLastError();
    }
};

// ---- ranged read-back of a unit's results (the cl_*_get entry points) ----
// [first, first + count) lies inside [0, size)
static inline bool range_ok(int64_t first, int64_t count, int64_t size)
{
    return first >= 0 && count >= 0 && first <= size && count <= size - first;
}
// the parts to the host through c->stream, one synchronisation, one joint report under the entry point's name
struct CopyOut { void* dst; const void* src; size_t bytes; };
static inline int read_back(cl_chrom* c, const char* who, std::initializer_list<CopyOut> parts)
{
    hipError_t e = hipSuccess;
    for (const CopyOut& p : parts)
        if (e == hipSuccess) e = hipMemcpyAsync(p.dst, p.src, p.bytes, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    if (e != hipSuccess || e2 != hipSuccess) return fail_at(CL_ERR_HIP, who, "copy", hipGetErrorString(e != hipSuccess ? e : e2));
    return CL_OK;
}

// cloops_hip.hip
int ensure_workspace(cl_chrom* c, int S);
int ensure_events(cl_chrom* c);
void ev_record(cl_chrom* c, int k);
int ensure_cand_capacity(cl_chrom* c, long long need);
Table make_table_slot(cl_chrom* c, int slot);
Table make_table(cl_chrom* c);
const int* k7_hist_for(cl_chrom* c, int cut);
K7Src k7_src(cl_chrom* c, const cl_chrom::Held& r, cl_chrom::Slot& sl, int cut, int M, const int* dM);
int finish_enqueue(cl_chrom* c, const RunRequest& req, int n_strips, const int* d_M);
// A unit drops its buffers and its state by assigning a fresh struct, and with them what was made from them: K25's marginals and
// weights belong to K24's cells, K26's diagonals to K25's marginals and weights, K27's matrix, K29's lambdas and K30's tables to K26's
// expected values.  Called by
// the units' entry points; the handle's destruction needs none of them
static inline void track_release(cl_chrom* c) { c->tk = cl_chrom::Track(); }
static inline void cov_release(cl_chrom* c) { c->cv = cl_chrom::Cov(); }
static inline void peak_release(cl_chrom* c) { c->pk = cl_chrom::Peak(); }
static inline void dom_release(cl_chrom* c) { c->dm = cl_chrom::Dom(); }
static inline void kdis_release(cl_chrom* c) { c->kd = cl_chrom::Kdis(); }
static inline void eig_release(cl_chrom* c) { c->eg = cl_chrom::Eig(); }
static inline void dot_release(cl_chrom* c) { c->dt = cl_chrom::Dot(); }
static inline void sad_release(cl_chrom* c) { c->sd = cl_chrom::Sad(); }
static inline void exp_release(cl_chrom* c) { eig_release(c); dot_release(c); sad_release(c); c->ex = cl_chrom::Exp(); }
static inline void bal_release(cl_chrom* c) { exp_release(c); c->bl = cl_chrom::Bal(); }
static inline void scc_release(cl_chrom* c) { c->sc = cl_chrom::Scc(); }
static inline void mat_release(cl_chrom* c) { c->mx = cl_chrom::Mat(); bal_release(c); scc_release(c); }
// what a unit's cl_*_free entry point does around its release function
static inline int unit_free(cl_chrom* c, const char* who, void (*release)(cl_chrom*))
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, who, "asynchronous runs still in flight");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    release(c);
    return CL_OK;
}
// k_block.hip, k_weighted.hip
int run_block(cl_chrom* c, const RunRequest& req);
int run_weighted(cl_chrom* c, const RunRequest& req);

// kernels of cloops_hip.hip that k_block.hip / k_weighted.hip launch
__global__ void k_init_table(Table t, const int* __restrict__ rankscan, int n);
__global__ void k_init_arrays(int n, int* __restrict__ parent, int* __restrict__ compkey, int* __restrict__ ncore,
                              int* __restrict__ bsize, int* __restrict__ usize, int* __restrict__ cellfirst,
                              int* __restrict__ flag, int* __restrict__ state, int* __restrict__ counters);
__global__ void k_strip_table(const u64* __restrict__ skeys, int n, int S, int shift, int* __restrict__ strip_start);
__global__ void k_root_labels(GridParams g, const int* __restrict__ strip_start, const int* __restrict__ root,
                              const int* __restrict__ compkey, const int* __restrict__ ncore, const int* __restrict__ bsize,
                              const int* __restrict__ state, const int* __restrict__ rankscan, int* __restrict__ rlabel);
__global__ void k_rank_flags(GridParams g, const int* __restrict__ strip_start, const int* __restrict__ root,
                             const int* __restrict__ compkey, const int* __restrict__ state, int* __restrict__ flag);
__global__ void __launch_bounds__(BIGTPB)
k_flatten(GridParams g, const int* __restrict__ strip_start, const int* __restrict__ cnt,
          const int* __restrict__ chainid, int* parent, const u32* __restrict__ srow,
          const int* __restrict__ head, const int* __restrict__ cellfirst,
          int* __restrict__ root, int* __restrict__ compkey, int* __restrict__ ncore,
          int* __restrict__ rootlist , int* __restrict__ counters);

// ---- variant 2 release rule: a border point's adjacent components in ascending key order (cloops_hip.hip) ----
struct Rec { int pt; int r[4]; };
#define OWNER_CONTESTED 0x40000000
__device__ __forceinline__ int owner_root(int o) { return o < 0 ? -1 : (o & (OWNER_CONTESTED - 1)); }

// k_lists.hip: the list form of K3 / K4 / K5 (host side; every function enqueues on c->stream)
struct ListRun {                                        // device views of the run's lists (valid after lists_build)
    int npos;                                           // positions of the layout the lists index (the run's layout: PETs of the run; the base layout: all rows)
    const int* pstrip;                                  // ... and its strip table
    const int* lcnt;                                    // {C, W}: cores, walkers
    const unsigned long long* cmask; const unsigned long long* wmask;
    const int* cgrank; const int* wgrank;
    int2* cpair; int* cpos; int* ckey; int2* wpair; int* wpos; int* wenc; int* cstrip;
};
int lists_build(cl_chrom* c, const GridParams& g, int nm, ListRun* out);
int lists_build_base(cl_chrom* c, const GridParams& g, int nm, ListRun* out);      // level 4: from the base layout + the cut's per-strip tables
int lists_base_keys(cl_chrom* c, const GridParams& g);
int lists_words_to_base(cl_chrom* c, const GridParams& g);                         // level 4, first run of an eps under a cut: its words to base positions                             // variant 2: cell minima of the base layout (once per eps)
int lists_union_flatten(cl_chrom* c, const GridParams& g, int nm, const ListRun& L);
int lists_scatter_root(cl_chrom* c, int nm, const ListRun& L);
int lists_border(cl_chrom* c, const GridParams& g, int nm, const ListRun& L);
int lists_emit_records(cl_chrom* c, const GridParams& g, int nm, const ListRun& L);
int lists_scatter_owner(cl_chrom* c, int nm, const ListRun& L);
int lists_final(cl_chrom* c, const RunRequest& req, const GridParams& g, int nm, const ListRun& L, bool rows, int* pair_count);
int lists_rowmask(cl_chrom* c, const RunRequest& req, int* total);

// kernels of k_sweep.hip that the step tail (finish_enqueue) launches
__global__ void __launch_bounds__(256)
k_step_classify_count(const int* __restrict__ dK, Table t, signed char* __restrict__ cls, int* __restrict__ bcount, int nb,
                      unsigned long long* __restrict__ zero, int nzero);
__global__ void __launch_bounds__(256)
k_cand_append(const int* __restrict__ dK, const signed char* __restrict__ cls, Table t, const int* __restrict__ boff ,
              const int* __restrict__ bcount, int base, int step, int cap, int4* __restrict__ cbox, int* __restrict__ cstep);
__global__ void __launch_bounds__(TPB)
k7_summary(K7Src s, int cut, const signed char* __restrict__ cls, K7Part* __restrict__ parts, unsigned long long* __restrict__ loghist,
           unsigned fine_lo, unsigned long long* __restrict__ fine );
__global__ void __launch_bounds__(256)
k7_reduce_parts(const K7Part* __restrict__ parts, int nparts, K7Part* out, const int* __restrict__ bcount , int nb,
                long long* totals, const volatile unsigned long long* dev_step , int step_words,
                unsigned long long* __restrict__ host_step, const int* __restrict__ dev_hdr, int* __restrict__ host_hdr);

// K8's X-sorted and Y-sorted PET tables (k_sweep.hip), shared with K11 (k_quant.hip): entry = (coordinate + 2^30) << 32 |
// (other coordinate + 2^30), the PETs that fail the cut sorted to the end as ~0
#define SIG_W 11                       // window 0 = the anchor itself, 1..10 = cModel.getNearbyPairRegions
struct SigWin { int lo[2 * SIG_W]; int hi[2 * SIG_W]; };      // [0..10] = A windows, [11..21] = B windows

// first index with (key >> 32) >= v   /   > v   in a sorted u64 table of m valid entries
__device__ __forceinline__ int k8_lb(const u64* __restrict__ t, int m, long long v)
{
    const u64 target = v <= -(1ll << 30) ? 0ull : ((u64)(u32)(v + (1 << 30)) << 32);
    int lo = 0, hi = m;
    while (lo < hi) { int mid = (lo + hi) >> 1; if (t[mid] < target) lo = mid + 1; else hi = mid; }
    return lo;
}
__device__ __forceinline__ int k8_ub(const u64* __restrict__ t, int m, long long v)
{
    return k8_lb(t, m, v + 1);
}
// builds the tables of (chromosome, cut) unless the handle holds them already (c->sig.tx / sig.ty; c->sig.m[0] on the device = the
// number of valid entries); enqueued on c->stream, c->n > 0
int sig_tables(cl_chrom* c, int cut);
// K19's table (k_agg.hip), shared with K22 (k_domain.hip), K23 (k_kdis.hip) and K24 (k_matrix.hip): the rows with Y - X >= cut sorted by X (c->ag.sx: X + 2^30 as u32, c->ag.sy:
// their Y, c->ag.kept rows) unless the handle holds it for this cut already; c->n > 0
int agg_table(cl_chrom* c, int cut);

// first index of [0, m) with sx[idx] >= t (m if none), by the 64 lanes of a wave together (all call, with the same arguments):
// 64 probes cut the range into 65 parts per round; sx ascends, so the lanes whose probe is below t are a prefix and a ballot
// counts them
__device__ __forceinline__ int k19_lb_wave(const u32* __restrict__ sx, int m, u32 t)
{
    const int lane = threadIdx.x & 63;
    int lo = 0, len = m;                                     // the answer lies in [lo, lo + len]
    while (len > 0) {
        const int step = len / 65 + 1;
        const long long pos = (long long)lo + (long long)(lane + 1) * step - 1;
        const bool below = pos < (long long)lo + len && sx[pos] < t;
        const int nb = __popcll(__ballot(below));
        // probe nb - 1 is below t, probe nb (if inside the range) is not
        const long long nlo = (long long)lo + (long long)nb * step;
        const long long end = (long long)lo + len, nhi = nlo + step - 1 < end ? nlo + step - 1 : end;
        lo = (int)nlo; len = (int)(nhi - nlo);
    }
    return lo;
}


// v / d by multiply-shift (Granlund-Montgomery, exact for all u32 v), the divisor made on the host: K12 (k_fingerprint.hip) and K24
// (k_matrix.hip)
struct K12Div { u32 magic; int sh1, sh2; };
__device__ __forceinline__ u32 k12_div(const K12Div& d, u32 v)
{
    const u32 t1 = __umulhi(d.magic, v);
    return (t1 + ((v - t1) >> d.sh1)) >> d.sh2;
}
static inline K12Div k12_divisor(u32 d)
{
    K12Div r;
    int l = 0; while ((1ull << l) < d) ++l;                          // ceil(log2 d)
    r.magic = (u32)((((1ull << 32) * ((1ull << l) - d)) / d) + 1);
    r.sh1 = l < 1 ? l : 1; r.sh2 = l > 1 ? l - 1 : 0;
    return r;
}

// K22 (k_domain.hip) and K24 (k_matrix.hip): wave aggregation in front of an atomic
#define K22_NONE INT_MIN                // no target (bins and domain numbers lie far above)
// What this lane has to add at `target` for a wave whose lanes each add `delta` at their target (K22_NONE: none): the lanes that share
// the first active lane's target are summed into that lane.  Called by all 64 lanes together.
__device__ __forceinline__ u32 k22_agg(int target, u32 delta)
{
    const u64 act = __ballot(target != K22_NONE);
    if (!act) return 0u;                                                        // (the same in every lane)
    const int leader = __ffsll((long long)act) - 1;
    const int lt = __shfl(target, leader);
    const u64 same = __ballot(target == lt);
    if (target == K22_NONE) return 0u;
    if (target != lt) return delta;
    return (int)(threadIdx.x & 63) == leader ? (u32)__popcll(same) * delta : 0u;
}
