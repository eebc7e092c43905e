"""ctypes binding of libcloops_hip.so (C ABI: include/cloops_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or no MI355X is
visible, every entry point raises.  (The CPU oracle under oracle/ is test infrastructure
and is never imported from here.)
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libcloops_hip.so")

CL_OK = 0
CL_ERR_ARG = -1
CL_ERR_HIP = -2
CL_ERR_EMPTY = -3
CL_ERR_DOMAIN = -4
CL_ERR_GRID = -5
CL_ERR_NODEVICE = -6
CL_ERR_HASH = -7
CL_ERR_PARSE = -8

VARIANT_CDBSCAN1 = 1
VARIANT_CDBSCAN2 = 2
VARIANT_BLOCK = 3

# the other integer #defines of include/cloops_hip.h that the host side restates: this is their one home (tests/test_abi.py
# compares every one with the header)
CL_TRACK_WASHU, CL_TRACK_JUICE = 0, 1
CL_TRACK_NAME_MAX = 64
CL_CONV_HICPRO, CL_CONV_JUICER, CL_CONV_PAIRS = 0, 1, 2
CL_CONV_E_FIELDS, CL_CONV_E_INT, CL_CONV_E_RANGE, CL_CONV_E_LONG = 1, 2, 3, 4
CL_INGEST_TIMES = 6
CL_INGEST_BEDPE, CL_INGEST_PAIRS = 0, 1
DIST_LOGBINS = 3840          # CL_DIST_LOGBINS
CL_KDE_MAX_GRID = 1024
CL_KDIS_KMAX = 64
CL_KDIS_BINS = 3968          # 31 octaves x 128 log bins: d < 2^31
CL_MAT_WMAX = 8192           # bins a side of a dense window
CL_MAT_CELLS_MAX = 16777216  # 2^24 cells of a dense window
CL_BAL_BINS_MAX = 16777216   # 2^24 bins of a balanced chromosome
CL_EIG_MAX = 6               # eigenpairs of a cl_eig_iterate
CL_EIG_BLOCK = 8             # columns of the iteration's block, vectors of a cl_eig_apply
CL_EIG_BINS_MAX = 1048576    # 2^20 bins of a chromosome's compartments
CL_SCC_HMAX = 20             # largest half-width of the SCC's box
CL_SCC_BAND_MAX = 268435456  # 2^28 entries nb (n_diags + 4 h) of a band array of cl_scc_moments
CL_DOT_WMAX = 16             # largest half-width of the donut's footprint
CL_DOT_CHUNKS_MAX = 64       # chunks of la of a cl_dot_hist
CL_DOT_CMAX = 4095           # counts at or above it share the histogram's last column
CL_DOT_BAND_MAX = 134217728  # 2^27 entries nb (dmax + 4 w) of the value band of cl_dot_lambdas
CL_SAD_CLASSES_MAX = 64      # classes of a cl_sad_sums


class ClBox(ctypes.Structure):
    _fields_ = [("min_x", ctypes.c_int32), ("max_x", ctypes.c_int32), ("min_y", ctypes.c_int32),
                ("max_y", ctypes.c_int32), ("count", ctypes.c_int32)]


class ClTiming(ctypes.Structure):
    _fields_ = [("ms_keys", ctypes.c_float), ("ms_sort", ctypes.c_float), ("ms_region", ctypes.c_float),
                ("ms_union", ctypes.c_float), ("ms_border", ctypes.c_float), ("ms_table", ctypes.c_float),
                ("ms_d2h", ctypes.c_float), ("ms_total", ctypes.c_float), ("n_in", ctypes.c_int64),
                ("n_strips", ctypes.c_int64), ("ms_bracket", ctypes.c_float), ("ms_band", ctypes.c_float),
                ("n_queried", ctypes.c_int64)]


class ClIngestName(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint64), ("first", ctypes.c_uint32), ("off", ctypes.c_uint32), ("len", ctypes.c_uint32),
                ("pad", ctypes.c_uint32)]


class ClDsummary(ctypes.Structure):
    _fields_ = [("n_all", ctypes.c_int64 * 2), ("n_pos", ctypes.c_int64 * 2), ("sumx", ctypes.c_double * 2),
                ("sumxx", ctypes.c_double * 2), ("xshift", ctypes.c_double), ("loghist", ctypes.c_uint64 * DIST_LOGBINS),
                ("fine_lo", ctypes.c_int64), ("fine", ctypes.c_uint64 * 2048)]


_int, _i32, _u32, _i64, _vp, _cp = ctypes.c_int, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_char_p
_i32p, _i64p, _u64p, _f32p, _vpp = (ctypes.POINTER(t) for t in (_i32, _i64, ctypes.c_uint64, ctypes.c_float, _vp))
_f64, _f64p = ctypes.c_double, ctypes.POINTER(ctypes.c_double)

# The C ABI of include/cloops_hip.h, one line per function: name -> (restype, argtypes).  load() applies it once; tests/test_abi.py
# checks every entry, the structs above and the constants against the header.
PROTOTYPES = {
    "cl_last_error": (_cp, []),
    "cl_device_count": (_int, []),
    "cl_version": (_int, []),
    "cl_chrom_create": (_int, [_int, _vp, _vp, _vp, _i64, _int, _vpp]),
    "cl_chrom_destroy": (None, [_vp]),
    "cl_chrom_size": (_i64, [_vp]),
    "cl_chrom_subsample": (_int, [_vp, _vp, _i64, _vpp]),
    "cl_chrom_set_stream": (_int, [_vp, _vp]),
    "cl_chrom_drop_indexes": (_int, [_vp]),
    "cl_cluster": (_int, [_vp, _int, _i32, _i32, _i32, _vp, _i32p, _i32p]),
    "cl_cluster_weighted": (_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32p, _i32p]),
    "cl_cluster_async": (_int, [_vp, _int, _i32, _i32, _i32, _vp]),
    "cl_cluster_pairs_async": (_int, [_vp, _int, _i32, _i32, _i32, _vp, _i64]),
    "cl_cluster_rowmask_async": (_int, [_vp, _int, _i32, _i32, _i32, _vp, _i64]),
    "cl_cluster_step_async": (_int, [_vp, _int, _i32, _i32, _i32, _i32, _i64]),
    "cl_wait": (_int, [_vp, _i32p, _i32p]),
    "cl_step_result": (_int, [_vp, _i64p, _i64p, ctypes.POINTER(ClDsummary)]),
    "cl_set_pairs_defer": (None, [_vp, _int]),
    "cl_pairs_sync": (_int, [_vp]),
    "cl_last_n_labelled": (_i64, [_vp]),
    "cl_last_n_in": (_i64, [_vp]),
    "cl_last_region_mode": (_int, [_vp]),
    "cl_base_rows": (_i64, [_vp]),
    "cl_get_boxes": (_int, [_vp, _vp]),
    "cl_boxes_host": (_vp, [_vp]),
    "cl_labels_device": (_vp, [_vp]),
    "cl_neighbor_counts": (_int, [_vp, _i32, _i32, _vp]),
    "cl_dist_summary": (_int, [_vp, _i32, ctypes.POINTER(ClDsummary)]),
    "cl_dist_bin_hist": (_int, [_vp, _i32, _u32, _u32, _int, _u64p]),
    "cl_dist_collect": (_int, [_vp, _i32, _i64p, _i64p, _i64p]),
    "cl_dist_kde": (_int, [_vp, _int, _f64, _f64, _f64, _int, _f64p]),
    "cl_kde_array": (_int, [_int, _vp, _i64, _f64, _f64, _f64, _int, _f64p]),
    "cl_sig_counts": (_int, [_vp, _i32, _i32, _vp, _vp, _i64p]),
    "cl_quant_counts": (_int, [_vp, _i32, _i32, _vp, _vp, _i64p]),
    "cl_contact_hist": (_int, [_vp, _i32, _i32, _i64, _vp, _vp, _i64p, _i64p, _i64p, _i32p]),
    "cl_anchor_mask": (_int, [_vp, _i64, _vp, _vp, _vp, _i64p, _i64p]),
    "cl_agg_loops": (_int, [_vp, _i32, _i32, _i32, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i64p]),
    "cl_track_build": (_int, [_vp, _i32, _i64, _i64, _vp, _cp, _cp, _i64p, _i64p]),
    "cl_track_chunks": (_int, [_vp, _i64, _i64, _vp, _vp, _i64p]),
    "cl_track_render": (_int, [_vp, _i64, _vp, _i64, _i64p]),
    "cl_track_free": (_int, [_vp]),
    "cl_cov_build": (_int, [_vp, _i64, _i32, _i64, _i64, _i64p, ctypes.POINTER(_u32), _i64p, _i64p]),
    "cl_cov_runs": (_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "cl_cov_text": (_int, [_vp, _cp, _i64, _i64, _i64p]),
    "cl_cov_chunks": (_int, [_vp, _i64, _i64, _vp, _vp, _i64p]),
    "cl_cov_render": (_int, [_vp, _i64, _vp, _i64, _i64p]),
    "cl_cov_free": (_int, [_vp]),
    "cl_peak_sort": (_int, [_vp, _i64, _i32, _i64p, _i64p, _i64p]),
    "cl_peak_call": (_int, [_vp, _i64, _i64, _i64p, _i64p, _i64p]),
    "cl_peak_get": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "cl_peak_count": (_int, [_vp, _vp, _vp, _i64, _vp]),
    "cl_peak_summits": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "cl_peak_free": (_int, [_vp]),
    "cl_dom_tracks": (_int, [_vp, _i64, _i64, _i64, _i64p, _i64p, _i64p]),
    "cl_dom_get": (_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "cl_dom_count": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "cl_dom_free": (_int, [_vp]),
    "cl_kdis_build": (_int, [_vp, _i64, _vp, _i32, _i64p]),
    "cl_kdis_get": (_int, [_vp, _i32, _i64, _i64, _vp, _vp, _vp]),
    "cl_kdis_hist": (_int, [_vp, _i32, _vp, _u64p, _u64p]),
    "cl_kdis_free": (_int, [_vp]),
    "cl_mat_window": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp, _i64p, _i64p]),
    "cl_mat_cells": (_int, [_vp, _i64, _i64, _i32, _i64p, _i64p, _i64p]),
    "cl_mat_cells_get": (_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "cl_mat_v4c": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _i64p, _i64p, _i64p]),
    "cl_mat_free": (_int, [_vp]),
    "cl_bal_marginals": (_int, [_vp, _i32, _i64p, _i64p, _i64p]),
    "cl_bal_marginals_get": (_int, [_vp, _i64, _i64, _vp, _vp]),
    "cl_bal_iterate": (_int, [_vp, _vp, _i32, _f64, _i32p, _i32p, _f64p, _f64p]),
    "cl_bal_weights_get": (_int, [_vp, _i64, _i64, _vp]),
    "cl_bal_cells_get": (_int, [_vp, _i64, _i64, _vp]),
    "cl_bal_free": (_int, [_vp]),
    "cl_exp_diagonals": (_int, [_vp, _vp, _i32, _i64p, _i64p]),
    "cl_exp_diagonals_get": (_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "cl_exp_set": (_int, [_vp, _vp, _i64]),
    "cl_exp_cells_get": (_int, [_vp, _i64, _i64, _vp]),
    "cl_exp_free": (_int, [_vp]),
    "cl_eig_build": (_int, [_vp, _f64, _i64, _i64p, _i64p]),
    "cl_eig_apply": (_int, [_vp, _vp, _i32, _vp]),
    "cl_eig_iterate": (_int, [_vp, _i32, _i32, _f64, _i32p, _i32p, _vp, _vp]),
    "cl_eig_vectors_get": (_int, [_vp, _i32, _i64, _i64, _vp]),
    "cl_eig_free": (_int, [_vp]),
    "cl_scc_moments": (_int, [_vp, _vp, _i64, _i64, _i32, _i64, _i64p, _u64p, _u64p, _u64p, _u64p, _u64p]),
    "cl_scc_free": (_int, [_vp]),
    "cl_dot_lambdas": (_int, [_vp, _i32, _i32, _i64, _i64, _i64p, _i64p]),
    "cl_dot_lambdas_get": (_int, [_vp, _i32, _i64, _i64, _vp]),
    "cl_dot_cells_get": (_int, [_vp, _i64, _i64, _vp]),
    "cl_dot_hist": (_int, [_vp, _vp, _i32, _vp, _u64p]),
    "cl_dot_call": (_int, [_vp, _vp, _i64p]),
    "cl_dot_sig_get": (_int, [_vp, _i64, _i64, _vp]),
    "cl_dot_free": (_int, [_vp]),
    "cl_sad_sums": (_int, [_vp, _vp, _i64, _i32, _i64, _i64, _i64p, _i64p, _i64p]),
    "cl_sad_get": (_int, [_vp, _vp, _vp, _vp]),
    "cl_sad_free": (_int, [_vp]),
    "cl_conv_create": (_int, [_int, _vp, _i32, _i64, _i64, _vpp]),
    "cl_conv_feed": (_int, [_vp, _vp, _i64, _i32, _i64p, _i64p, _i64p]),
    "cl_conv_render": (_int, [_vp, _vp, _i64, _i64p]),
    "cl_conv_error": (_int, [_vp, _i64p, _i32p]),
    "cl_conv_timing": (_int, [_vp, _f32p]),
    "cl_conv_destroy": (_int, [_vp]),
    "cl_ingest_create": (_int, [_int, _vp, _i64, _i64, _i32, _vpp]),
    "cl_ingest_set_format": (_int, [_vp, _i32, _i64]),
    "cl_ingest_feed": (_int, [_vp, _vp, _i64, _i64p, _i64p, _i64p]),
    "cl_ingest_error": (_int, [_vp, _i64p, _i32p]),
    "cl_ingest_headers": (_int, [_vp, _i64p]),
    "cl_ingest_names": (_int, [_vp, _vp, _i64, _i64p]),
    "cl_ingest_commit": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _vp, _i32p]),
    "cl_ingest_finish": (_int, [_vp, _vp, _i32, _i32, _vp, _i64p]),
    "cl_ingest_rows": (_int, [_vp, _i32, _vp, _vp, _i64]),
    "cl_ingest_chrom_arrays": (_int, [_vp, _i32, _i64p, _vpp, _vpp]),
    "cl_ingest_distances": (_int, [_vp, _vp, _i64]),
    "cl_ingest_timing": (_int, [_vp, _f32p]),
    "cl_ingest_destroy": (_int, [_vp]),
    "cl_cand_reset": (_int, [_vp]),
    "cl_cand_append": (_int, [_vp, _i32, _i64p, _i64p]),
    "cl_cand_finish": (_int, [_vp, _i32, _vp, _i64, _i64p]),
    "cl_cand_finish_device": (_int, [_vp, _i32, _vpp, _i64p]),
    "cl_set_table_export": (None, [_vp, _int]),
    "cl_set_device_labels": (None, [_vp, _int]),
    "cl_set_profiling": (None, [_vp, _int]),
    "cl_get_timing": (_int, [_vp, ctypes.POINTER(ClTiming)]),
    "cl_sweep_plan": (_int, [_vp, _i32p, _i32, _i32p, _i32]),
    "cl_set_layout_reuse": (None, [_vp, _int]),
    "cl_set_sort_index": (None, [_vp, _int]),
    "cl_set_count_reuse": (None, [_vp, _int]),
    "cl_set_count_floor": (None, [_vp, _i32]),
    "cl_set_count_thresholds": (None, [_vp, _i32p, _i32]),
    "cl_set_eps_list": (None, [_vp, _i32p, _i32]),
    "cl_set_traversal": (None, [_vp, _int]),
    "cl_stream_create": (_vp, [_int]),
    "cl_stream_destroy": (None, [_vp]),
    "cl_host_alloc": (_vp, [_i64]),
    "cl_host_free": (None, [_vp]),
    "cl_debug_arena_overcommit": (None, [_i64]),
}
SYMBOLS = list(PROTOTYPES)


def bind(lib, table):
    """state the prototypes of `table` (name -> (restype, argtypes)) on a loaded library -> the library"""
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


class CloopsHipError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "libcloops_hip error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load():
    """Load the shared library (raises if it has not been built -- see cloops_amd/build.py)."""
    global _lib
    if _lib is not None:
        return _lib
    # (The library reads and writes no environment variable; how many runs execute side by side is decided by the streams the
    # application hands to cl_chrom_create -- the sweep driver shares three per GPU)
    path = SO_PATH
    if os.environ.get("CLOOPS_DEVEL_LIB") == "1":          # developer build with ablation knobs (cloops_amd/build.py --devel)
        path = SO_PATH.replace(".so", "_devel.so")
    if not os.path.exists(path):
        raise ImportError(
            "libcloops_hip.so is missing (%s). Build it with `python -m cloops_amd.build` "
            "(needs hipcc); there is no CPU fallback." % path)
    _lib = bind(ctypes.CDLL(path), PROTOTYPES)
    return _lib


def check(rc):
    if rc != CL_OK:
        msg = load().cl_last_error()
        raise CloopsHipError(rc, msg.decode() if msg else "")


def host_alloc(nbytes):
    """page-locked host memory of the library (its cl_host_alloc entry) -> address; the owner frees it with lib.cl_host_free"""
    p = load().cl_host_alloc(int(nbytes))
    if not p:
        raise MemoryError("no page-locked host memory of %d bytes" % nbytes)
    return p


def stream_create(device):
    """a HIP stream made by the library (its cl_stream_create entry) -> address; the owner ends it with lib.cl_stream_destroy"""
    s = load().cl_stream_create(int(device))
    if not s:
        raise CloopsHipError(CL_ERR_HIP, (load().cl_last_error() or b"").decode())
    return s
