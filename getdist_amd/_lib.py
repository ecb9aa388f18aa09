"""
ctypes binding of libgdhip.so (the C ABI in include/gdhip.h).  This is the thin Python->HIP seam; there
is NO CPU fallback: if the library or a GPU is missing, every compute entry point raises.
"""

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgdhip.so")

GD_OK, GD_ERR_BADARG, GD_ERR_NOMEM, GD_ERR_HIP, GD_ERR_EMPTY, GD_ERR_SOLVER, GD_ERR_FFT, GD_ERR_NODEVICE, GD_ERR_TIMEOUT = \
    0, -1, -2, -3, -4, -5, -6, -7, -8


class GdhipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libgdhip error %d: %s" % (code, msg))
        self.code = code


class GdhipTimeout(GdhipError):
    """GD_ERR_TIMEOUT: a collective or the communicator set-up gave up waiting for a peer; the library has aborted and dropped
    the communicator, so the ranks renegotiate over the host application's own channel (parallel.init_library_comm)."""


def build_native(force=False):
    """Compile libgdhip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    script = os.path.join(_HERE, "csrc", "build.sh")
    if force:
        for f in os.listdir(os.path.join(_HERE, "csrc")):
            if f.endswith(".o") or f.endswith(".so"):
                os.remove(os.path.join(_HERE, "csrc", f))
    subprocess.run(["bash", script], check=True)
    return LIB_PATH


_p = C.c_void_p
_i32, _i64, _f64 = C.c_int32, C.c_int64, C.c_double
_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_pi64 = C.POINTER(C.c_int64)

# name -> (restype, argtypes); must list every symbol include/gdhip.h declares (tests check this)
SIGNATURES = {
    "gd_device_count": (C.c_int, []),
    "gd_create": (C.c_int, [C.c_int, C.POINTER(_p)]),
    "gd_destroy": (None, [_p]),
    "gd_last_error": (C.c_char_p, [_p]),
    "gd_version": (C.c_char_p, []),
    "gd_device_info": (C.c_int, [_p, _pi64]),
    "gd_sync": (C.c_int, [_p]),
    "gd_dev_alloc": (C.c_int, [_p, _i64, C.POINTER(_p)]),
    "gd_dev_free": (C.c_int, [_p, _p]),
    "gd_memcpy_h2d": (C.c_int, [_p, _p, _p, _i64]),
    "gd_memcpy_d2h": (C.c_int, [_p, _p, _p, _i64]),
    "gd_memcpy_d2h_async": (C.c_int, [_p, _p, _p, _i64]),
    "gd_copy_sync": (C.c_int, [_p]),
    "gd_memcpy_d2d": (C.c_int, [_p, _p, _p, _i64]),
    "gd_memset": (C.c_int, [_p, _p, C.c_int, _i64]),
    "gd_gather_items": (C.c_int, [_p, _p, _p, _pi32, _i32, _i64]),
    "gd_host_alloc": (C.c_int, [_p, _i64, C.POINTER(_p)]),
    "gd_host_free": (C.c_int, [_p, _p]),
    "gd_kde_lag_sums_2d": (C.c_int, [_p, _i32, _i32, _pd, _pi64, _i32, _pd]),
    "gd_autocov_lags_batch": (C.c_int, [_p, _pi32, _i32, _pd, _i64, _i32, _pd]),
    "gd_kde_lag_sums_batch": (C.c_int, [_p, _pi32, _i32, _pd, _pi64, _i32, _pd]),
    "gd_autocov_lags_range_batch": (C.c_int, [_p, _pi32, _i32, _pd, _i64, _i64, _i64, _i32, _pd]),
    "gd_timer_start": (C.c_int, [_p]),
    "gd_timer_stop_ms": (C.c_int, [_p, _pd]),
    "gd_upload": (C.c_int, [_p, _p, _i64, _i64, _i64, _i64, _p]),
    "gd_num_rows": (C.c_int, [_p, _pi64, _pi64]),
    "gd_column_ptr": (C.c_int, [_p, _i64, C.POINTER(_p)]),
    "gd_weight_stats": (C.c_int, [_p, _i64, _i64, _f64, _pd]),
    "gd_col_stats": (C.c_int, [_p, _i64, _i64, _pd]),
    "gd_cov": (C.c_int, [_p, _pi32, _i32, _i64, _i64, _pd, _pd, _pd, _pd]),
    "gd_quantiles": (C.c_int, [_p, _pi32, _i32, _i64, _i64, _pd, _i32, _pd]),
    "gd_quantiles_mm_probe": (C.c_int, [_p, _pi32, _i32, _i64, _i64, _pd, _i32, _pd, _pd, _pd, _pd, C.POINTER(C.c_int32)]),
    "gd_quantiles_mm": (C.c_int, [_p, _pi32, _i32, _i64, _i64, _pd, _i32, _pd, _pd]),
    "gd_autocov_lags": (C.c_int, [_p, _i32, _f64, _i64, _i32, _pd]),
    "gd_kde_lag_sums": (C.c_int, [_p, _i32, _f64, _pi64, _i32, _pd]),
    "gd_hist1d": (C.c_int, [_p, _pi32, _i32, _pd, _pd, _i32, _pd]),
    "gd_hist1d_dev": (C.c_int, [_p, _pi32, _i32, _pd, _pd, _i32, _p]),
    "gd_bin_indices": (C.c_int, [_p, _i32, _f64, _f64, _i32, _i32, _pi32, _pi64]),
    "gd_prebin": (C.c_int, [_p, _i32, _f64, _f64, _i32, _p]),
    "gd_prebin_batch": (C.c_int, [_p, _pi32, _i32, _pd, _pd, _i32, C.POINTER(_p)]),
    "gd_prebin8_batch": (C.c_int, [_p, _pi32, _i32, _pd, _pd, _i32, C.POINTER(_p), _pi64]),
    "gd_hist2d_prebinned8": (C.c_int, [_p, _i32, C.POINTER(_p), C.POINTER(_p), _p]),
    "gd_prebin8_hist2d": (C.c_int, [_p, _pi32, _i32, _pd, _pd, C.POINTER(_p), _pi64, _i32, C.POINTER(_p), C.POINTER(_p), _p]),
    "gd_hist2d": (C.c_int, [_p, _i32, _pi32, _pi32, _pd, _pd, _pd, _pd, _i32, _p]),
    "gd_hist2d_prebinned": (C.c_int, [_p, _i32, C.POINTER(_p), C.POINTER(_p), _i32, _p]),
    "gd_minmax_affine": (C.c_int, [_p, _i32, _pi32, _pi32, _pd, _pd, _pd]),
    "gd_hist2d_sheared": (C.c_int, [_p, _i32, _pi32, _pi32, _pd, _pd, _pd, _pd, _pd, _pd, _i32, _p]),
    "gd_dct1d": (C.c_int, [_p, _i32, _i32, _pd, _pd]),
    "gd_isj1d": (C.c_int, [_p, _i32, _i32, _pd, _pd, _pd, _pi32]),
    "gd_isj1d_dev": (C.c_int, [_p, _i32, _i32, _p, _pd, _pd, _pi32]),
    "gd_density1d": (C.c_int, [_p, _i32, _i32, _pd, _pd, _pi32, _pi32, _i32, _i32, _pd, _pi32]),
    "gd_density1d_dev": (C.c_int, [_p, _i32, _i32, _p, _pd, _pi32, _pi32, _i32, _i32, _pd, _pi32]),
    "gd_density1d_batch": (C.c_int, [_p, _p, _p, _i32, _pi32, _i32, _pd, _pd, _pd]),
    "gd_kopt2d": (C.c_int, [_p, _i32, _i32, _p, _pd, _pi32, _pd, _pd, _pd]),
    "gd_kopt2d_enqueue": (C.c_int, [_p, _i32, _i32, _p, _pd, _pi32, _pd, _pd, _p, _pi32]),
    "gd_kopt2d_finish": (C.c_int, [_p, _p, _i32, _i32, _p, _pd]),
    "gd_get_h": (C.c_int, [_p, _i32, _pd, _pd, _pd, _pi32, _pd]),
    "gd_density2d": (C.c_int, [_p, _i32, _i32, _p, _pd, _pd, _pd, _pi32, _pi32, _i32, _i32, _p, _pi32]),
    "gd_copy_mark": (C.c_int, [_p, _pi32]),
    "gd_copy_wait": (C.c_int, [_p, _i32]),
    "gd_density2d_enqueue": (C.c_int, [_p, _i32, _i32, _p, _pd, _pd, _pd, _pi32, _pi32, _i32, _i32, _p, _p]),
    "gd_density2d_enqueue_indexed": (C.c_int, [_p, _i32, _i32, _p, _pi32, _pd, _pd, _pd, _pi32, _pi32, _i32, _i32, _p, _p]),
    "gd_attach_samples": (C.c_int, [_p, _p]),
    "gd_clone_samples": (C.c_int, [_p, _p]),
    "gd_bind_thread": (C.c_int, [_p]),
    "gd_contour_levels": (C.c_int, [_p, _i32, _i32, _p, _pd, _i32, _pd, _pi32]),
    "gd_contour_paths": (C.c_int, [_p, _i32, _p, _pi64, _pi32, _pi32, _pd, _pi64, _i64, _pd, _pi64, _i64, _pd, _i32, _p, _p, _pi64,
                                   _pi64, _pi32]),
    "gd_limits1d": (C.c_int, [_p, _i32, _i32, _pd, _pd, _pd, _pd, _i32, _i32, _pd, _pi32]),
    "gd_set_extra_column": (C.c_int, [_p, _i32, _pd]),
    "gd_aux_weights": (C.c_int, [_p, _pd]),
    "gd_col_minmax": (C.c_int, [_p, _pi32, _i32, _i64, _i64, _i32, C.c_double, _pd]),
    "gd_weights_integral": (C.c_int, [_p, _pi32]),
    "gd_thin_rows": (C.c_int, [_p, _i64, _i64, _i64, _i32, _p, _i64, C.POINTER(C.c_int64)]),
    "gd_binary_transitions": (C.c_int, [_p, _pi32, _i32, _p, _i64, _pd, _i32, C.POINTER(C.c_int64)]),
    "gd_thinned_lag_sums": (C.c_int, [_p, _pi32, _i32, _pd, _p, _i64, _i32, _pd]),
    "gd_density2d_masked": (C.c_int, [_p, _i32, _p, C.c_double, C.c_double, C.c_double, _i32, _i32, _i32, _i32, _pd, _pd,
                                      C.POINTER(C.c_ubyte), _p, _pi32]),
    "gd_like_weights": (C.c_int, [_p, _pd, _i32, C.c_double, _pd]),
    "gd_select_weights": (C.c_int, [_p, _i32]),
    "gd_likes1d": (C.c_int, [_p, _i32, _i32, _pd, _pd, _pd, _pd, _pi32, _pi32, _i32, _pd, _pi32]),
    "gd_likes2d": (C.c_int, [_p, _i32, _i32, _p, _p, _pd, _pd, _pd, _pi32, _pi32, _i32, _p, _pi32]),
    "gd_circ_convolve": (C.c_int, [_p, _i32, _i32, _pd, _pd, _pd]),
    "gd_convolve1d_direct": (C.c_int, [_p, _pd, _i64, _pd, _i64, _pd]),
    "gd_autoconvolve": (C.c_int, [_p, _i32, _f64, _i32, _pd, _i64, _i64, _i64, _i32, _pd]),
    "gd_like_stats": (C.c_int, [_p, _i32, _pd]),
    "gd_batch2d_grid_sizes": (C.c_int, [_p, _i32, _pd, _pi32, _i32, _pi32]),
    "gd_density2d_batch": (C.c_int, [_p, _p, _p, _p, _i32, _pd, _pd, _pd, _pi32, _i32, _p, _p, _p, _i64, _pi32, _pd, _pd, _pi32,
                                     _pi32]),
    "gd_comm_unique_id": (C.c_int, [_p]),
    "gd_comm_init": (C.c_int, [_p, _i32, _i32, _p]),
    "gd_comm_info": (C.c_int, [_p, _pi32, _pi32]),
    "gd_comm_destroy": (C.c_int, [_p]),
    "gd_comm_abandon": (C.c_int, [_p]),
    "gd_comm_allgather": (C.c_int, [_p, _pd, _i64, _pd]),
    "gd_comm_allreduce_sum": (C.c_int, [_p, _pd, _i64]),
    "gd_comm_allgather_dev": (C.c_int, [_p, _p, _i64, _p]),
    "gd_comm_allreduce_sum_dev": (C.c_int, [_p, _p, _i64, _p]),
    "gd_batch2d_finish": (C.c_int, [_p]),
    "gd_batch2d_invalidate": (C.c_int, [_p]),
    "gd_batch2d_exchanges": (C.c_int, [_p, C.POINTER(C.c_int64)]),
    "gd_prepare_params": (C.c_int, [_p, _p, _p, _pi32, _i32, _pd, _pd, _pd, _pd, _pd, _pd, _pd, _pd, C.POINTER(C.c_int32), _p]),
    "gd_prepare_ahead_counts": (C.c_int, [_p, C.POINTER(C.c_int64)]),
    "gd_comm_rccl_path": (C.c_int, [C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]),
    "gd_upload_shard": (C.c_int, [_p, _p, _i64, _i64, _i64, _i64, _i64, _p]),
    "gd_comm_share_columns": (C.c_int, [_p, C.POINTER(C.c_int64)]),
    "gd_histnd_batch": (C.c_int, [_p, _i32, _pi32, _pi32, _pd, _pd, _i32, _i32, _i32, _pd, _pd, _pd]),
    "gd_pca_corr": (C.c_int, [_p, _pi32, _i32, _pi32, _pd, _pd, _pd]),
    "gd_pca_project": (C.c_int, [_p, _pi32, _i32, _pi32, _pd, _pd, _pd, _i32, _i32, _pd, _pd, _pd, _pd, _pd, _pd]),
    "gd_mixture_nll": (C.c_int, [_p, _pi32, _i32, _i32, _pd, _pd, _pd, _i64, _i64, _pd]),
    "gd_draw_single_rows": (C.c_int, [_p, C.POINTER(C.c_uint64), _p, _f64, _f64, _i32, _p, _i64, _pi64]),
    "gd_gather_rows": (C.c_int, [_p, _p, _i64, _pi32, _i32, _p]),
    "gd_format_rows": (C.c_int, [_p, _pi32, _i32, _i64, _i64, _p, _i64, _i32, _i32, _i32, _i32, _p, _i64, _pi64]),
    "gd_format_matrix": (C.c_int, [_p, _p, _i64, _i32, _i64, _i64, _i32, _i32, _i32, _i32, _p, _i64, _pi64]),
    "gd_parse_scan": (C.c_int, [_p, _p, _i64, _i32, _pi64, _pi32, _pi64]),
    "gd_parse_rows": (C.c_int, [_p, _p, _i64, _i32, _i64, _i32, _p, _i64, _i64, _p, _i64, _pi64]),
    "gd_expr_eval": (C.c_int, [_p, _pi32, _i32, _pd, _i32, _i32, _i32, _i64, _i64, _p, _pd]),
    "gd_expr_eval_tab": (C.c_int, [_p, _pi32, _i32, _pd, _i32, _i32, _i32, _i64, _i64, _p, _pd, _p, _i32]),
    "gd_upload_device": (C.c_int, [_p, _p, _i32, _i32, _i32, _pi32, _i32, C.POINTER(_p), _i32]),
    "gd_pointer_info": (C.c_int, [_p, _p, _pi32, _pi32]),
    "gd_fetch_device_array": (C.c_int, [_p, _p, _i64, _i64, _i64, _i64, _i32, _p, _pd]),
    "gd_download_samples": (C.c_int, [_p, _pd]),
    "gd_select_samples": (C.c_int, [_p, _p, _pi64]),
    "gd_set_weights": (C.c_int, [_p, _pd]),
    "gd_export_device": (C.c_int, [_p, _p, _pi64]),
    "gd_export_alloc": (C.c_int, [_i32, _i64, C.POINTER(_p)]),
    "gd_export_free": (C.c_int, [_i32, _p]),
    "gd_export_fetch": (C.c_int, [_i32, _p, _p, _i64]),
}

GD_HISTND_MAXD, GD_HISTND_MAX_BINS = 25, 1 << 25
GD_HISTND_H, GD_HISTND_LIKES, GD_HISTND_LMIN = 1, 2, 4
GD_PCA_MAX_PROJ = 448
GD_DRAW_MORE_ROWS = -21
GD_FORMAT_MORE_BYTES = -22
GD_FMT_SRC_WEIGHT, GD_FMT_SRC_ZERO, GD_FMT_SRC_ONE = -1, -2, -3
GD_FMT_MAX_PREC, GD_FMT_MAX_WIDTH = 17, 32
GD_PARSE_NOT_PLAIN = -23
# gd_upload_device / gd_fetch_device_array: a valid description the call does not serve -- memory the host can read as well
# (page-locked, managed) or negative strides; device memory of another device; a pointer the runtime does not know
GD_ERR_DECLINED, GD_ERR_OTHER_DEVICE, GD_ERR_NOT_DEVICE = -24, -25, -26
GD_PTR_DEVICE, GD_PTR_PINNED, GD_PTR_MANAGED, GD_PTR_UNKNOWN = 0, 1, 2, 3
GD_PARSE_MAX_LINE = 8192
GD_EX_MAX_CODE, GD_EX_MAX_STACK, GD_EX_MAX_CONST, GD_EX_MAX_COLS = 128, 16, 32, 16
GD_EX_WEIGHT = -1
GD_EX_OPS = ("COL CONST NEG ABS SQRT SQUARE RECIP EXP LOG LOG10 LOG2 SIN COS TAN ATAN TANH NOT ADD SUB MUL DIV POW ATAN2 MIN MAX "
             "LT LE GT GE EQ NE AND OR WHERE").split()  # GD_EX_<name> = its position
GD_EX_TO_COLUMN, GD_EX_TO_AUXW, GD_EX_TO_HOST_F64, GD_EX_TO_HOST_U8 = 0, 1, 2, 3
# the table look-ups of gd_expr_eval_tab: op codes behind the GD_EX_ set, and its limits
GD_TAB_OPS = {"INTERP": 34, "SPLINE1": 35, "SPLINE2": 36}  # GD_TAB_<name>
GD_TAB_MAX_TABLES, GD_TAB_MAX_DOUBLES = 4, 1 << 22
GD_PATHS_XY, GD_PATHS_FLAG, GD_PATHS_LOOPS = 0, 1, 2
PATHS_ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, _i32, _i64)  # gd_paths_alloc_fn


class GdExprTable(C.Structure):
    """gd_expr_table of gdhip.h"""

    _fields_ = [("kind", _i32), ("deriv", _i32), ("nx", _i32), ("ny", _i32), ("p0", _pd), ("p1", _pd), ("p2", _pd),
                ("left", _f64), ("right", _f64)]


def expr_table_structs(tables):
    """The gd_expr_table array for the tables of a compiled expression (colexpr.Table objects, whose arrays it points
    into: they must outlive the call it is passed to)."""
    arr = (GdExprTable * len(tables))()
    for t, st in zip(tables, arr):
        st.kind, st.deriv, st.nx, st.ny = GD_TAB_OPS[t.kind], t.deriv, t.nx, t.ny
        for name, a in zip(("p0", "p1", "p2"), t.arrays):
            setattr(st, name, _dp(a))
        st.left, st.right = t.left, t.right
    return arr


def format_field_bytes(width, prec):
    """Upper bound of one formatted field, separator or newline included (gd_format_rows / gd_format_matrix)."""
    return max(int(width), int(prec) + 8) + 1


def skipped_text_bytes(f, skiprows):
    """Bytes that the first ``skiprows`` lines of the binary file ``f`` take, read off ``f``; None when only a text-mode
    reader can tell.  np.loadtxt and pandas skip lines of a file opened as text, where a lone '\\r' ends a line as well and
    the bytes must decode; the device never sees the skipped bytes, so a '\\r' that is not directly followed by '\\n', a
    NUL or a byte >= 0x80 among them is left to the host parser (Context.parse_text declines)."""
    start = 0
    for _ in range(int(skiprows or 0)):
        line = f.readline()  # up to and including the next '\n'
        if not line:
            break
        if b"\r" in line.replace(b"\r\n", b"") or b"\0" in line or not line.isascii():
            return None
        start += len(line)
    return start


class GdDevPart(C.Structure):
    """gd_dev_part of gdhip.h"""

    _fields_ = [("base", _p), ("rows", _i64), ("cols", _i64), ("row_stride", _i64), ("col_stride", _i64), ("weights", _p),
                ("w_stride", _i64)]


class GdSelection(C.Structure):
    """gd_selection of gdhip.h"""

    _fields_ = [("row_kind", _i32), ("flags", _i32), ("lo", _i64), ("hi", _i64), ("rows", _p), ("K", _i64), ("thr", _f64),
                ("keep", _p), ("m", _i32), ("append_kind", _i32), ("append_slot", _i32), ("weight_kind", _i32),
                ("append_host", _p), ("new_weights", _p)]


class GdExport(C.Structure):
    """gd_export of gdhip.h"""

    _fields_ = [("row_kind", _i32), ("flags", _i32), ("lo", _i64), ("hi", _i64), ("rows", _p), ("K", _i64), ("thr", _f64),
                ("mask_col", _i32), ("m", _i32), ("cols", _p), ("base", _p), ("rows_capacity", _i64), ("row_stride", _i64),
                ("col_stride", _i64), ("dtype", _i32), ("reserved", _i32), ("consumer_stream", _p)]


GD_EXP_ROWS_COLUMN_NZ = 5  # gd_export_device: the rows whose value in a resident column is != 0

# gd_select_samples: row kinds, weight kinds, append kinds, flags, rows per tile of the count / placement passes
GD_SEL_ALL, GD_SEL_RANGE, GD_SEL_MASK_U8, GD_SEL_WEIGHT_GT, GD_SEL_ROWS_I32 = range(5)
GD_SEL_W_KEEP, GD_SEL_W_UNIT, GD_SEL_W_REPLACE = range(3)
GD_SEL_APPEND_NONE, GD_SEL_APPEND_HOST, GD_SEL_APPEND_SLOT = range(3)
GD_SEL_ROWS_ON_DEVICE = 1
GD_SEL_TILE = 1024

_lib = None


def load_library():
    """dlopen libgdhip.so and attach prototypes.  Raises if the library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libgdhip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or getdist_amd/csrc/build.sh (there is no CPU fallback)")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class PrepareSettings(C.Structure):
    """gd_prepare_settings"""

    _fields_ = [("fine_bins_2D", C.c_int32), ("auto_bandwidth", C.c_int32), ("uncorrelated_sampler", C.c_int32),
                ("ahead", C.c_int32)]


# gd_prepared_param
PREPARED_PARAM = np.dtype([("range_min", np.float64), ("range_max", np.float64), ("sigma_range", np.float64),
                           ("has_limits_bot", np.int32), ("has_limits_top", np.int32)])


def _dp(a):
    return a.ctypes.data_as(_pd)


def _ip(a):
    return a.ctypes.data_as(_pi32)


def _f64arr(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32arr(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class DevBuf:
    """
    A device allocation owned by a Context.  free() returns the block to the context's free list (hipFree
    synchronises the device and costs ~0.25 ms; a triangle makes ~100 short-lived buffers per step).
    """

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        self.ptr, self.capacity = ctx._take_block(self.nbytes)

    def free(self):
        if self.ptr and self.ctx.h:
            self.ctx._give_block(self.ptr, self.capacity)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def to_host(self, shape, dtype=np.float64, offset_bytes=0, pinned=False):
        out = self.ctx.pinned_array(shape, dtype) if pinned else np.empty(shape, dtype=dtype)
        self.ctx._check(self.ctx.lib.gd_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr + offset_bytes, out.nbytes))
        return out

    def to_host_async(self, shape, dtype=np.float64):
        """Start a D2H copy into page-locked memory on the copy stream; call ctx.copy_sync() before reading."""
        out = self.ctx.pinned_array(shape, dtype)
        self.ctx._check(self.ctx.lib.gd_memcpy_d2h_async(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def from_host(self, arr, offset_bytes=0):
        arr = np.ascontiguousarray(arr)
        self.ctx._check(self.ctx.lib.gd_memcpy_h2d(self.ctx.h, self.ptr + offset_bytes, arr.ctypes.data, arr.nbytes))


class ExportBlock:
    """Device memory that belongs to no Context (gd_export_alloc): what a devarray.DeviceArray owns.  It stays valid across
    every mutator, re-upload and Context.close(), never enters a context's block cache, and is freed -- with the device
    index alone -- when the last reference to it goes."""

    def __init__(self, device, nbytes):
        self.lib, self.device, self.nbytes = load_library(), int(device), int(nbytes)
        p = _p()
        rc = self.lib.gd_export_alloc(self.device, self.nbytes, C.byref(p))
        if rc == GD_ERR_NOMEM:
            raise MemoryError("no room for a device array of %d bytes on device %d" % (self.nbytes, self.device))
        if rc != 0:
            raise GdhipError(rc, "gd_export_alloc(%d bytes) failed" % self.nbytes)
        self.ptr = p.value

    def fetch(self, out):
        """the block's first out.nbytes bytes into the C-contiguous host array ``out``"""
        rc = self.lib.gd_export_fetch(self.device, out.ctypes.data, self.ptr, out.nbytes)
        if rc != 0:
            raise GdhipError(rc, "gd_export_fetch failed")
        return out

    def __del__(self):
        try:
            if self.ptr:
                self.lib.gd_export_free(self.device, self.ptr)
            self.ptr = None
        except Exception:
            pass


class Context:
    """One GPU, one stream, one resident sample set.  Thin, typed wrappers over the C ABI."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.h = None
        if self.lib.gd_device_count() <= 0:
            raise RuntimeError("getdist_amd needs a HIP device (no CPU fallback): none visible")
        h = _p()
        rc = self.lib.gd_create(int(device), C.byref(h))
        if rc != 0:
            raise GdhipError(rc, "gd_create(device=%d) failed" % device)
        self.h = h
        self.device = device
        self.N = self.n = 0
        self.weighted = False
        self._pinned = []  # (ptr, nbytes, ctypes buffer): page-locked result buffers, recycled when unreferenced
        self._free_blocks = []  # (device ptr, capacity) returned by DevBuf.free(), reused by alloc()
        self._pinned_blocks = []
        self.comm_world = self.comm_rank = 0

    PINNED_POOL_LIMIT = 8 << 30

    def pinned_array(self, shape, dtype=np.float64):
        """
        A numpy array in page-locked host memory (D2H at full PCIe rate).  Blocks are recycled once no array
        view references them any more (every view keeps the block's ctypes buffer alive, so its refcount tells).
        """
        import sys

        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        best = None
        for k, (ptr, nb, buf) in enumerate(self._pinned):
            if nb >= nbytes and sys.getrefcount(buf) <= 3 and (best is None or nb < self._pinned[best][1]):
                best = k
        if best is None:
            if sum(nb for _, nb, _ in self._pinned) + nbytes > self.PINNED_POOL_LIMIT:
                return np.empty(shape, dtype=dtype)
            p = _p()
            self._check(self.lib.gd_host_alloc(self.h, max(nbytes, 1 << 20), C.byref(p)))
            nb = max(nbytes, 1 << 20)
            buf = (C.c_ubyte * nb).from_address(p.value)
            self._pinned.append((p.value, nb, buf))
            best = len(self._pinned) - 1
        buf = self._pinned[best][2]
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def pinned_block(self, shape, dtype=np.float64):
        """A page-locked array outside the recycling pool (freed with the context): the landing buffer of the binary
        chain cache, from which the sample columns are DMA'd to the device."""
        nbytes = max(int(np.prod(shape)) * np.dtype(dtype).itemsize, 8)
        p = _p()
        self._check(self.lib.gd_host_alloc(self.h, nbytes, C.byref(p)))
        buf = (C.c_ubyte * nbytes).from_address(p.value)
        self._pinned_blocks.append((p.value, buf))
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def reserve_pinned_twin(self):
        """Allocate a second block for every pooled page-locked block (callers that keep one result set alive while
        computing the next need two sets; doing it up front keeps hipHostMalloc out of the steady state)."""
        for ptr, nb, buf in list(self._pinned):
            p = _p()
            self._check(self.lib.gd_host_alloc(self.h, nb, C.byref(p)))
            self._pinned.append((p.value, nb, (C.c_ubyte * nb).from_address(p.value)))

    def close(self):
        """Free the device side.  Page-locked host blocks that some numpy array still views (mc.samples loaded from the
        binary cache, a Density2D.P the user kept) are NOT freed: every view holds the block's ctypes buffer, so its
        reference count tells; such a block stays valid for the life of the process instead of dangling."""
        import sys

        if self.h:
            self.lib.gd_copy_sync(self.h)  # result copies in flight land before their targets could go away
            self.release_cached_blocks()
            for ptr, _, buf in getattr(self, "_pinned", []):
                if sys.getrefcount(buf) <= 3:
                    self.lib.gd_host_free(self.h, ptr)
            self._pinned = []
            for ptr, buf in getattr(self, "_pinned_blocks", []):
                if sys.getrefcount(buf) <= 3:
                    self.lib.gd_host_free(self.h, ptr)
            self._pinned_blocks = []
            self.lib.gd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            msg = self.lib.gd_last_error(self.h)
            if rc == GD_ERR_TIMEOUT:
                self.comm_world = self.comm_rank = 0  # the library has aborted and dropped the communicator
                raise GdhipTimeout(rc, msg.decode() if msg else "?")
            raise GdhipError(rc, msg.decode() if msg else "?")

    # ---- memory / info
    def device_info(self):
        a = np.zeros(6, dtype=np.int64)
        self._check(self.lib.gd_device_info(self.h, a.ctypes.data_as(_pi64)))
        return dict(cu_count=int(a[0]), lds_bytes=int(a[1]), hbm_total=int(a[2]), hbm_free=int(a[3]),
                    clock_khz=int(a[4]), wave=int(a[5]))

    def alloc(self, nbytes):
        return DevBuf(self, nbytes)

    DEVICE_CACHE_LIMIT = 16 << 30

    def _take_block(self, nbytes):
        best = None
        for k, (ptr, cap) in enumerate(self._free_blocks):
            if cap >= nbytes and cap <= 2 * nbytes + (1 << 20) and (best is None or cap < self._free_blocks[best][1]):
                best = k
        if best is not None:
            return self._free_blocks.pop(best)
        p = _p()
        rc = self.lib.gd_dev_alloc(self.h, int(nbytes), C.byref(p))
        if rc == GD_ERR_NOMEM and self._free_blocks:  # give cached blocks back and retry once
            self.release_cached_blocks()
            rc = self.lib.gd_dev_alloc(self.h, int(nbytes), C.byref(p))
        self._check(rc)
        return p.value, int(nbytes)

    def _give_block(self, ptr, cap):
        if sum(c for _, c in self._free_blocks) + cap > self.DEVICE_CACHE_LIMIT:
            self.lib.gd_dev_free(self.h, ptr)
        else:
            self._free_blocks.append((ptr, cap))

    def release_cached_blocks(self):
        for ptr, _ in self._free_blocks:
            self.lib.gd_dev_free(self.h, ptr)
        self._free_blocks = []

    def sync(self):
        self._check(self.lib.gd_sync(self.h))

    def gather_items(self, dst, src, index, item_bytes, dst_offset=0):
        """dst[dst_offset + q] = src[index[q]] for fixed-size items (one gather kernel)."""
        index = _i32arr(index)
        self._check(self.lib.gd_gather_items(self.h, dst.ptr + int(dst_offset) * int(item_bytes), src.ptr, _ip(index),
                                             len(index), int(item_bytes)))

    def autocov_lags_batch(self, cols, means, k0, nlags):
        cols, means = _i32arr(cols), _f64arr(means)
        out = np.zeros((len(cols), nlags))
        self._check(self.lib.gd_autocov_lags_batch(self.h, _ip(cols), len(cols), _dp(means), int(k0), int(nlags), _dp(out)))
        return out

    def autocov_lags_range_batch(self, cols, means, lo, hi, k0, nlags):
        cols, means = _i32arr(cols), _f64arr(means)
        out = np.zeros((len(cols), nlags))
        self._check(self.lib.gd_autocov_lags_range_batch(self.h, _ip(cols), len(cols), _dp(means), int(lo), int(hi), int(k0),
                                                         int(nlags), _dp(out)))
        return out

    def kde_lag_sums_2d(self, coli, colj, kinv3, lags):
        kinv3 = _f64arr(kinv3)
        lags = np.ascontiguousarray(lags, dtype=np.int64)
        out = np.zeros(len(lags))
        self._check(self.lib.gd_kde_lag_sums_2d(self.h, int(coli), int(colj), _dp(kinv3), lags.ctypes.data_as(_pi64),
                                                len(lags), _dp(out)))
        return out

    def kde_lag_sums_batch(self, cols, inv4s2, lags):
        cols, inv4s2 = _i32arr(cols), _f64arr(inv4s2)
        lags = np.ascontiguousarray(lags, dtype=np.int64)
        out = np.zeros((len(cols), len(lags)))
        self._check(self.lib.gd_kde_lag_sums_batch(self.h, _ip(cols), len(cols), _dp(inv4s2), lags.ctypes.data_as(_pi64),
                                                   len(lags), _dp(out)))
        return out

    def copy_sync(self):
        self._check(self.lib.gd_copy_sync(self.h))

    def copy_mark(self):
        """A token for 'every result copy issued so far'; copy_wait(token) blocks until those have landed."""
        tok = C.c_int32(0)
        self._check(self.lib.gd_copy_mark(self.h, C.byref(tok)))
        return int(tok.value)

    def copy_wait(self, token):
        self._check(self.lib.gd_copy_wait(self.h, int(token)))

    def copy_d2d(self, dst, dst_off, src, src_off, nbytes):
        self._check(self.lib.gd_memcpy_d2d(self.h, dst.ptr + dst_off, src.ptr + src_off, int(nbytes)))

    def timer_start(self):
        self._check(self.lib.gd_timer_start(self.h))

    def timer_stop_ms(self):
        ms = C.c_double()
        self._check(self.lib.gd_timer_stop_ms(self.h, C.byref(ms)))
        return ms.value

    # ---- sample set
    def upload(self, samples, weights=None):
        s = np.asarray(samples)
        if s.dtype != np.float64:
            s = s.astype(np.float64)
        if s.ndim == 1:
            s = s.reshape(-1, 1)
        if not (s.flags.c_contiguous or s.flags.f_contiguous):
            s = np.ascontiguousarray(s)
        N, n = s.shape
        rs, cs = s.strides[0] // 8, s.strides[1] // 8
        if n == 1:
            rs, cs = 1, N
        w = None if weights is None else _f64arr(weights)
        self._keep = (s, w)
        self._check(self.lib.gd_upload(self.h, s.ctypes.data, N, n, rs, cs, None if w is None else w.ctypes.data))
        self._keep = None
        self.N, self.n, self.weighted = N, n, w is not None

    def upload_device(self, parts, weights=None, keep=None):
        """A sample set of this context's own from device arrays (gd_upload_device).  ``parts``: one 2-D devarray.DevArray per
        chain, of one element type and column count; ``weights``: None or one 1-D DevArray per part, of one element type;
        ``keep``: the source columns to keep (None: all).  The context's stream is ordered behind the arrays' producer
        streams (events, no host wait); the source is copied, never adopted.  False when the library declines (page-locked or
        managed memory, negative strides): the caller takes the host route and the previous set is still resident.
        ValueError for memory of another device."""
        arr = (GdDevPart * len(parts))()
        for k, (st, d) in enumerate(zip(arr, parts)):
            st.base, (st.rows, st.cols), (st.row_stride, st.col_stride) = d.ptr or None, d.shape, d.strides
            if weights is not None:
                st.weights, st.w_stride = weights[k].ptr or None, weights[k].strides[0]
        everything = list(parts) + list(weights or [])
        streams = []
        for d in everything:
            if d.stream is not None and d.shape[0] and d.stream not in streams:
                streams.append(d.stream)
        handles = (_p * max(len(streams), 1))(*streams)
        keep = None if keep is None else _i32arr(keep)
        rc = self.lib.gd_upload_device(self.h, arr, len(parts), int(parts[0].dtype), int(weights[0].dtype) if weights else 0,
                                       None if keep is None else _ip(keep), 0 if keep is None else len(keep), handles, len(streams))
        if not self._served(rc, everything):
            return False
        self.N = int(sum(d.shape[0] for d in parts))
        self.n, self.weighted = int(parts[0].shape[1] if keep is None else len(keep)), weights is not None
        return True

    def pointer_info(self, ptr):
        """(GD_PTR_* kind, device index or -1) of a pointer, as the runtime sees it (gd_pointer_info)"""
        kind, dev = C.c_int32(), C.c_int32()
        self._check(self.lib.gd_pointer_info(self.h, int(ptr), C.byref(kind), C.byref(dev)))
        return int(kind.value), int(dev.value)

    def _served(self, rc, arrays):
        """True for success, False for GD_ERR_DECLINED (memory the host can read as well, or negative strides: the caller takes
        the host route).  Device memory of another device is a ValueError that names the device to pass; anything else
        raises as usual (a pointer the runtime does not know included)."""
        if rc == GD_ERR_DECLINED:
            return False
        if rc == GD_ERR_OTHER_DEVICE:
            for d in arrays:
                kind, dev = self.pointer_info(d.ptr) if d.ptr else (GD_PTR_UNKNOWN, -1)
                if kind == GD_PTR_DEVICE and dev != self.device:
                    raise ValueError("the array lives on device %d: pass device=%d" % (dev, dev))
        self._check(rc)
        return True

    def fetch_device_array(self, desc):
        """The 1-D or 2-D devarray.DevArray as a float64 host array (gd_fetch_device_array), negative strides included; None
        when the library declines the memory."""
        fwd, flipped = desc.forward()
        d2 = fwd.as2d()
        out = np.empty(d2.shape)
        if out.size:
            rc = self.lib.gd_fetch_device_array(self.h, d2.ptr, d2.shape[0], d2.shape[1], d2.strides[0], d2.strides[1],
                                                int(d2.dtype), d2.stream, _dp(out))
            if not self._served(rc, [d2]):
                return None
        out = out.reshape(desc.shape)
        for ax in flipped:
            out = np.flip(out, ax)
        return out

    def download_samples(self):
        """The resident columns as an (N, n) row-major float64 array in page-locked memory (gd_download_samples)."""
        out = self.pinned_array((self.N, self.n))
        self._check(self.lib.gd_download_samples(self.h, _dp(out)))
        return out

    def read_row(self, i):
        """Row ``i`` of the resident columns (n values) by one gather of 16-byte items (gd_gather_items): the pair of
        rows that holds it, per column."""
        import types

        ld, i = (self.N + 511) // 512 * 512, int(i)
        if self.n * ld // 2 >= 1 << 31:
            raise ValueError("row read: the resident set is too large for 32-bit item indices")
        src = types.SimpleNamespace(ptr=self.column_ptr(0))
        dst = self.alloc(self.n * 16)
        try:
            self.gather_items(dst, src, (np.arange(self.n, dtype=np.int64) * ld + i) // 2, 16)
            return dst.to_host((self.n, 2))[:, i & 1].copy()
        finally:
            dst.free()

    def read_column(self, j):
        """Resident column ``j`` as a host vector of N doubles"""
        out = np.empty(self.N)
        self._check(self.lib.gd_memcpy_d2h(self.h, out.ctypes.data, self.column_ptr(j), out.nbytes))
        return out

    def upload_shard(self, cols_f, N, n, col_first, weights=None):
        """This rank's block of columns only (``cols_f``: (N, count) Fortran-ordered fp64, the columns
        [col_first, col_first + count) of the (N, n) set); the rest arrives by comm_share_columns."""
        c = np.asfortranarray(cols_f, dtype=np.float64)
        if c.ndim == 1:
            c = c.reshape(-1, 1, order="F")
        count = c.shape[1]
        assert c.shape[0] == N or count == 0
        w = None if weights is None else _f64arr(weights)
        self._keep = (c, w)
        self._check(self.lib.gd_upload_shard(self.h, c.ctypes.data if count else None, int(N), int(n), int(col_first), int(count),
                                             int(c.strides[1] // 8) if count else int(N), None if w is None else w.ctypes.data))
        self._keep = None
        self.N, self.n, self.weighted = int(N), int(n), w is not None

    def comm_share_columns(self, first_by_rank):
        f = np.ascontiguousarray(first_by_rank, dtype=np.int64)
        assert f.size == self.comm_world + 1
        self._check(self.lib.gd_comm_share_columns(self.h, f.ctypes.data_as(C.POINTER(C.c_int64))))

    @staticmethod
    def comm_rccl_path():
        lib = load_library()
        buf = C.create_string_buffer(1024)
        pre = C.c_int32(0)
        rc = lib.gd_comm_rccl_path(buf, 1024, C.byref(pre))
        if rc != 0:
            raise GdhipError(rc, "librccl.so could not be loaded")
        return buf.value.decode(), bool(pre.value)

    def attach(self, owner):
        """Borrow ``owner``'s resident sample set (same device, no copy): this context becomes a second lane."""
        self._check(self.lib.gd_attach_samples(self.h, owner.h))
        self.N, self.n, self.weighted = owner.N, owner.n, owner.weighted

    def clone_samples(self, src):
        """A resident sample set of this context's OWN with the columns and weights of ``src``'s (same device), copied
        device to device; ``src`` may be re-uploaded or closed afterwards."""
        self._check(self.lib.gd_clone_samples(self.h, src.h))
        self.N, self.n, self.weighted = src.N, src.n, src.weighted

    def select_samples(self, rows=None, keep_cols=None, append=None, weights="keep"):
        """Replace the resident sample set by a selection of itself, device to device (gd_select_samples); returns the new
        row count.  ``rows``: None (all), ``("range", lo, hi)``, ``("mask", m)`` with m a bool / uint8 host array of N
        entries or a device buffer (anything with ``.ptr``) of N bytes, ``("weight_gt", thr)``, ``("rows", r)`` with r a host
        index array or ``("rows", buf, K)`` with a device int32 buffer.  ``keep_cols``: ascending resident columns (None:
        all).  ``append``: None, a host vector of N doubles, or ``("slot", s)`` for spare column s.  ``weights``: "keep",
        "unit", or a host vector with one weight per selected row.  A refusal raises and leaves the set as it was."""
        sel = GdSelection()
        alive = []  # host arrays the structure points into
        kind = "all" if rows is None else rows[0]
        if kind == "range":
            sel.row_kind, sel.lo, sel.hi = GD_SEL_RANGE, int(rows[1]), int(rows[2])
        elif kind in ("mask", "rows"):
            sel.row_kind = GD_SEL_MASK_U8 if kind == "mask" else GD_SEL_ROWS_I32
            v = rows[1]
            if hasattr(v, "ptr"):
                sel.flags, sel.rows = GD_SEL_ROWS_ON_DEVICE, v.ptr
                sel.K = int(rows[2]) if kind == "rows" else 0
            else:
                if kind == "mask":
                    v = np.ascontiguousarray(v)
                    v = v.view(np.uint8) if v.dtype == bool else np.ascontiguousarray(v != 0).view(np.uint8)
                    if v.shape != (self.N,):
                        raise ValueError("the row mask must have one entry per sample row")
                else:
                    v = _i32arr(v).ravel()
                    sel.K = v.size
                alive.append(v)
                sel.rows = v.ctypes.data
        elif kind == "weight_gt":
            sel.row_kind, sel.thr = GD_SEL_WEIGHT_GT, float(rows[1])
        elif kind != "all":
            raise ValueError("unknown row selection %r" % (kind,))
        n_new = self.n
        if keep_cols is not None:
            k = _i32arr(keep_cols).ravel()
            alive.append(k)
            sel.keep, sel.m, n_new = k.ctypes.data, k.size, k.size
        if isinstance(append, tuple):
            sel.append_kind, sel.append_slot = GD_SEL_APPEND_SLOT, int(append[1])
            n_new += 1
        elif append is not None:
            a = _f64arr(append).ravel()
            if a.shape != (self.N,):
                raise ValueError("the appended vector must have one entry per sample row")
            alive.append(a)
            sel.append_kind, sel.append_host = GD_SEL_APPEND_HOST, a.ctypes.data
            n_new += 1
        weighted = self.weighted
        if isinstance(weights, str):
            if weights not in ("keep", "unit"):
                raise ValueError("weights must be 'keep', 'unit' or a vector")
            sel.weight_kind = GD_SEL_W_KEEP if weights == "keep" else GD_SEL_W_UNIT
            weighted = weighted and weights == "keep"
        else:
            w = _f64arr(weights).ravel()
            if sel.row_kind == GD_SEL_ROWS_I32 and w.size != sel.K:
                raise ValueError("one new weight per selected row")
            alive.append(w)
            sel.weight_kind, sel.new_weights, sel.K, weighted = GD_SEL_W_REPLACE, w.ctypes.data, w.size, True
        count = C.c_int64()
        self._check(self.lib.gd_select_samples(self.h, C.byref(sel), C.byref(count)))
        self._keep = None
        self.N, self.n, self.weighted = int(count.value), int(n_new), weighted
        return self.N

    def export_block(self, nbytes):
        """device memory for an exported array, owned by the array and not by this context (ExportBlock)"""
        return ExportBlock(self.device, nbytes)

    def export_device(self, rows=None, cols=None, dest=None, stream=None):
        """Selected rows of resident columns into a device array (gd_export_device); returns K, the number of rows selected.
        ``rows``: as select_samples takes them (None, ``("range", lo, hi)``, ``("mask", m)``, ``("weight_gt", thr)``,
        ``("rows", r)`` / ``("rows", buf, K)``), or ``("nonzero", j)``: the rows where resident column j is != 0.  ``cols``: resident
        column indices in any order, repeats and spare columns allowed; None: the sample weights (ones for a unit-weight set).
        ``dest``: a 2-D devarray.DevArray of K rows and len(cols) columns (1 for the weights) in any of the four element
        types, any non-negative strides; None: nothing is written, the call only counts.  ``stream``: the consumer's stream
        (None: the call returns when the destination is written; else the two streams are ordered by events and the host
        does not wait).  ValueError when ``dest`` has fewer rows than are selected, when its elements overlap, and for memory
        that is not plain device memory of this device; nothing is written then."""
        ex = GdExport()
        alive = []
        kind = "all" if rows is None else rows[0]
        if kind == "range":
            ex.row_kind, ex.lo, ex.hi = GD_SEL_RANGE, int(rows[1]), int(rows[2])
        elif kind in ("mask", "rows"):
            ex.row_kind = GD_SEL_MASK_U8 if kind == "mask" else GD_SEL_ROWS_I32
            v = rows[1]
            if hasattr(v, "ptr"):
                ex.flags, ex.rows = GD_SEL_ROWS_ON_DEVICE, v.ptr
                ex.K = int(rows[2]) if kind == "rows" else 0
            else:
                if kind == "mask":
                    v = np.ascontiguousarray(v)
                    v = v.view(np.uint8) if v.dtype == bool else np.ascontiguousarray(v != 0).view(np.uint8)
                    if v.shape != (self.N,):
                        raise ValueError("the row mask must have one entry per sample row")
                else:
                    v = _i32arr(v).ravel()
                    ex.K = v.size
                alive.append(v)
                ex.rows = v.ctypes.data
        elif kind == "weight_gt":
            ex.row_kind, ex.thr = GD_SEL_WEIGHT_GT, float(rows[1])
        elif kind == "nonzero":
            ex.row_kind, ex.mask_col = GD_EXP_ROWS_COLUMN_NZ, int(rows[1])
        elif kind != "all":
            raise ValueError("unknown row selection %r" % (kind,))
        if cols is not None:
            c = _i32arr(cols).ravel()
            alive.append(c)
            ex.cols, ex.m = c.ctypes.data, c.size
        if dest is not None:
            if dest.ndim != 2 or dest.shape[1] != (1 if cols is None else len(c)):
                raise ValueError("the destination must be 2-D with one column per exported column")
            ex.base, ex.rows_capacity = dest.ptr or None, dest.shape[0]
            ex.row_stride, ex.col_stride, ex.dtype = dest.strides[0], dest.strides[1], int(dest.dtype)
        ex.consumer_stream = stream
        count = C.c_int64()
        rc = self.lib.gd_export_device(self.h, C.byref(ex), C.byref(count))
        if rc == GD_DRAW_MORE_ROWS:
            if dest is None:
                return int(count.value)
            raise ValueError("the destination has %d rows, %d are selected" % (dest.shape[0], count.value))
        if rc == GD_ERR_DECLINED:
            raise ValueError("out= must be plain device memory with non-negative strides (%s)" % self.lib.gd_last_error(self.h).decode())
        if rc == GD_ERR_BADARG:
            raise ValueError(self.lib.gd_last_error(self.h).decode())
        self._served(rc, [] if dest is None else [dest])
        return int(count.value)

    def set_weights(self, w):
        """Replace only the sample weights of the resident set (gd_set_weights): N host doubles, or None for unit weights."""
        if w is not None:
            w = _f64arr(w)
            if w.shape != (self.N,):
                raise ValueError("weights must have one entry per sample row")
        self._check(self.lib.gd_set_weights(self.h, None if w is None else _dp(w)))
        self._keep = None
        self.weighted = w is not None

    def bind_thread(self):
        self._check(self.lib.gd_bind_thread(self.h))

    def column_ptr(self, j):
        p = _p()
        self._check(self.lib.gd_column_ptr(self.h, int(j), C.byref(p)))
        return p.value

    # ---- moments
    def weight_stats(self, lo=0, hi=None, thresh=np.inf):
        out = np.zeros(4)
        self._check(self.lib.gd_weight_stats(self.h, lo, self.N if hi is None else hi, float(thresh), _dp(out)))
        return dict(norm=out[0], max_w=out[1], sum_w2=out[2], n_above=out[3])

    def col_stats(self, lo=0, hi=None):
        out = np.zeros((self.n, 4))
        self._check(self.lib.gd_col_stats(self.h, lo, self.N if hi is None else hi, _dp(out)))
        return out

    def cov(self, cols=None, lo=0, hi=None, minmax=False):
        """(means, cov, norm) of the columns over rows [lo, hi); with ``minmax`` also the (m, 2) column extrema."""
        cols = _i32arr(np.arange(self.n) if cols is None else cols)
        m = len(cols)
        means, cov, norm = np.zeros(m), np.zeros((m, m)), C.c_double()
        mm = np.zeros((m, 2)) if minmax else None
        self._check(self.lib.gd_cov(self.h, _ip(cols), m, lo, self.N if hi is None else hi, _dp(means), _dp(cov),
                                    C.byref(norm), None if mm is None else _dp(mm)))
        return (means, cov, norm.value, mm) if minmax else (means, cov, norm.value)

    def quantiles(self, cols, targets, lo=0, hi=None, minmax=None):
        """Weighted quantile selection; ``minmax`` (len(cols) x 2: each column's min and max over the rows, or over a
        superset of them) enables the two-pass linear-bucket path."""
        cols = _i32arr(cols)
        targets = _f64arr(targets).reshape(len(cols), -1)
        out = np.zeros_like(targets)
        mm = None if minmax is None else _f64arr(minmax).reshape(len(cols), 2)
        self._check(self.lib.gd_quantiles_mm(self.h, _ip(cols), len(cols), lo, self.N if hi is None else hi, _dp(targets),
                                             targets.shape[1], None if mm is None else _dp(mm), _dp(out)))
        return out

    def quantiles_probe(self, cols, targets, minmax, means):
        """gd_quantiles_mm_probe over whole columns: (quantiles, lag probe or None).  The probe -- the first 8
        autocovariance lag sums of the columns about ``means``, what autocov_lags_batch(cols, means, 0, 8) returns -- rides on
        the select's counting pass; None when the select took a path without it."""
        cols = _i32arr(cols)
        targets = _f64arr(targets).reshape(len(cols), -1)
        out = np.zeros_like(targets)
        mm = _f64arr(minmax).reshape(len(cols), 2)
        means = _f64arr(means)
        probe = np.zeros((len(cols), 8))
        done = C.c_int32(0)
        self._check(self.lib.gd_quantiles_mm_probe(self.h, _ip(cols), len(cols), 0, self.N, _dp(targets), targets.shape[1], _dp(mm),
                                                   _dp(out), _dp(means), _dp(probe), C.byref(done)))
        return out, (probe if done.value else None)

    def prepare_params(self, cols, targets, minmax, means, variances, err, limits, has_bot, has_top, twin=None, fine_bins_2D=0,
                       auto_bandwidth=False, uncorrelated_sampler=False, ahead=0):
        """gd_prepare_params over whole columns: (quantiles, lag probe or None, records).  ``records`` holds a row
        (range_min, range_max, sigma_range, has_limits_bot, has_limits_top) per column, the scalar tail of _initParam worked
        out by the library; ``ahead`` (bit 0: N_eff lag sums, bit 1: index columns) lets it enqueue, without waiting, what the
        next batched 2D call over these columns starts with."""
        cols = _i32arr(cols)
        m = len(cols)
        targets = _f64arr(targets).reshape(m, 11)
        mm = _f64arr(minmax).reshape(m, 2)
        means, variances, err = _f64arr(means), _f64arr(variances), _f64arr(err)
        limits = _f64arr(limits).reshape(m, 2)
        out, probe = np.zeros_like(targets), np.zeros((m, 8))
        recs = np.zeros(m, dtype=PREPARED_PARAM)
        recs["has_limits_bot"], recs["has_limits_top"] = has_bot, has_top
        settings = PrepareSettings(int(fine_bins_2D), int(bool(auto_bandwidth)), int(bool(uncorrelated_sampler)), int(ahead))
        done = C.c_int32(0)
        self._check(self.lib.gd_prepare_params(self.h, None if twin is None else twin.h, C.byref(settings), _ip(cols), m, _dp(targets),
                                               _dp(mm), _dp(means), _dp(variances), _dp(err), _dp(limits), _dp(out), _dp(probe),
                                               C.byref(done), recs.ctypes.data))
        return out, (probe if done.value else None), recs

    def prepare_ahead_counts(self):
        """(enqueued, consumed, discarded): pieces gd_prepare_params has enqueued ahead on this context, how many a batched
        call used, how many were waited for and dropped."""
        out = np.zeros(3, dtype=np.int64)
        self._check(self.lib.gd_prepare_ahead_counts(self.h, out.ctypes.data_as(_pi64)))
        return tuple(int(v) for v in out)

    def autocov_lags(self, col, mean, k0, nlags):
        out = np.zeros(nlags)
        self._check(self.lib.gd_autocov_lags(self.h, int(col), float(mean), int(k0), int(nlags), _dp(out)))
        return out

    def kde_lag_sums(self, col, inv4s2, lags):
        lags = np.ascontiguousarray(lags, dtype=np.int64)
        out = np.zeros(len(lags))
        self._check(self.lib.gd_kde_lag_sums(self.h, int(col), float(inv4s2), lags.ctypes.data_as(_pi64), len(lags),
                                             _dp(out)))
        return out

    # ---- binning
    def hist1d(self, cols, binmin, width, F):
        cols, binmin, width = _i32arr(cols), _f64arr(binmin), _f64arr(width)
        out = np.zeros((len(cols), F))
        self._check(self.lib.gd_hist1d(self.h, _ip(cols), len(cols), _dp(binmin), _dp(width), int(F), _dp(out)))
        return out

    def bin_indices(self, col, binmin, width, F, round_half=True):
        idx = np.zeros(self.N, dtype=np.int32)
        bad = C.c_int64()
        self._check(self.lib.gd_bin_indices(self.h, int(col), float(binmin), float(width), int(bool(round_half)), int(F),
                                            _ip(idx), C.byref(bad)))
        return idx, bad.value

    def prebin(self, col, binmin, width, F, buf=None):
        buf = buf or self.alloc(self.N * 2 + 64)
        self._check(self.lib.gd_prebin(self.h, int(col), float(binmin), float(width), int(F), buf.ptr))
        return buf

    def prebin_batch(self, cols, binmin, width, F, bufs):
        cols, binmin, width = _i32arr(cols), _f64arr(binmin), _f64arr(width)
        arr = (_p * len(cols))(*[b.ptr for b in bufs])
        self._check(self.lib.gd_prebin_batch(self.h, _ip(cols), len(cols), _dp(binmin), _dp(width), int(F), arr))

    def prebin8_batch(self, cols, binmin, width, F, bufs):
        """Byte index columns (F <= 256) for several sample columns in one launch; returns the out-of-range counts."""
        cols, binmin, width = _i32arr(cols), _f64arr(binmin), _f64arr(width)
        arr = (_p * len(cols))(*[b.ptr for b in bufs])
        bad = np.zeros(len(cols), dtype=np.int64)
        self._check(self.lib.gd_prebin8_batch(self.h, _ip(cols), len(cols), _dp(binmin), _dp(width), int(F), arr,
                                              bad.ctypes.data_as(_pi64)))
        return bad

    def hist2d_prebinned8(self, idx_x, idx_y, out=None):
        """B histograms of 256 x 256 bins from byte index columns (unit weights); raises GdhipError(-5) on counter wrap."""
        B = len(idx_x)
        out = out or self.alloc(B * 65536 * 8)
        if isinstance(idx_x, np.ndarray):  # device addresses already gathered (uint64), e.g. from a per-column table
            px, py = np.ascontiguousarray(idx_x, dtype=np.uint64), np.ascontiguousarray(idx_y, dtype=np.uint64)
            ax, ay = px.ctypes.data_as(C.POINTER(_p)), py.ctypes.data_as(C.POINTER(_p))
        else:
            ax = (_p * B)(*[b.ptr for b in idx_x])
            ay = (_p * B)(*[b.ptr for b in idx_y])
        self._check(self.lib.gd_hist2d_prebinned8(self.h, B, ax, ay, out.ptr))
        return out

    def hist2d(self, colx, coly, bx, wx, by, wy, F, out=None):
        colx, coly = _i32arr(colx), _i32arr(coly)
        B = len(colx)
        out = out or self.alloc(B * F * F * 8)
        bx, wx, by, wy = _f64arr(bx), _f64arr(wx), _f64arr(by), _f64arr(wy)
        self._check(self.lib.gd_hist2d(self.h, B, _ip(colx), _ip(coly), _dp(bx), _dp(wx), _dp(by), _dp(wy), int(F),
                                       out.ptr))
        return out

    def hist2d_prebinned(self, idx_x, idx_y, F, out=None):
        B = len(idx_x)
        out = out or self.alloc(B * F * F * 8)
        ax = (_p * B)(*[b.ptr for b in idx_x])
        ay = (_p * B)(*[b.ptr for b in idx_y])
        self._check(self.lib.gd_hist2d_prebinned(self.h, B, ax, ay, int(F), out.ptr))
        return out

    def minmax_affine(self, coli, colj, a, b):
        coli, colj, a, b = _i32arr(coli), _i32arr(colj), _f64arr(a), _f64arr(b)
        out = np.zeros((len(coli), 2))
        self._check(self.lib.gd_minmax_affine(self.h, len(coli), _ip(coli), _ip(colj), _dp(a), _dp(b), _dp(out)))
        return out

    def hist2d_sheared(self, coli, colj, r0, r1, xmin, dx, ymin, dy, F, out=None):
        coli, colj = _i32arr(coli), _i32arr(colj)
        B = len(coli)
        out = out or self.alloc(B * F * F * 8)
        arrs = [_f64arr(v) for v in (r0, r1, xmin, dx, ymin, dy)]
        self._check(self.lib.gd_hist2d_sheared(self.h, B, _ip(coli), _ip(colj), *[_dp(v) for v in arrs], int(F),
                                               out.ptr))
        return out

    # ---- densities
    def dct1d(self, hist):
        hist = _f64arr(hist)
        B, F = hist.shape
        out = np.zeros_like(hist)
        self._check(self.lib.gd_dct1d(self.h, B, F, _dp(hist), _dp(out)))
        return out

    def isj1d(self, hist, neff):
        """(hfrac[B], status[B]): the 1D ISJ bandwidths of B histograms, solved on the device."""
        hist, neff = _f64arr(hist), _f64arr(neff)
        B, F = hist.shape
        h = np.zeros(B)
        status = np.zeros(B, dtype=np.int32)
        self._check(self.lib.gd_isj1d(self.h, B, F, _dp(hist), _dp(neff), _dp(h), _ip(status)))
        return h, status

    def density1d(self, hist, smooth, winw, flags, bco, mbc):
        hist = _f64arr(hist)
        B, F = hist.shape
        smooth, winw, flags = _f64arr(smooth), _i32arr(winw), _i32arr(flags)
        P = np.zeros_like(hist)
        status = np.zeros(B, dtype=np.int32)
        self._check(self.lib.gd_density1d(self.h, B, F, _dp(hist), _dp(smooth), _ip(winw), _ip(flags), int(bco),
                                          int(mbc), _dp(P), _ip(status)))
        return P, status

    def density2d_masked(self, d_hist, pos, F, rx, ry, corr, winw, flags, bco, mbc, mask_bc, mask_mbc, zero_mask):
        """Pair ``pos`` of the histogram batch ``d_hist`` with an explicit prior mask (mask_function);
        returns (device grid, status)."""
        out = self.alloc(F * F * 8)
        status = np.zeros(1, dtype=np.int32)
        mb = None if mask_bc is None else _f64arr(mask_bc)
        mm = None if mask_mbc is None else _f64arr(mask_mbc)
        zm = None if zero_mask is None else np.ascontiguousarray(zero_mask, dtype=np.uint8)
        self._check(self.lib.gd_density2d_masked(
            self.h, int(F), d_hist.ptr + int(pos) * F * F * 8, float(rx), float(ry), float(corr),
            int(winw), int(flags), int(bco), int(mbc), None if mb is None else _dp(mb), None if mm is None else _dp(mm),
            None if zm is None else zm.ctypes.data_as(C.POINTER(C.c_ubyte)), out.ptr, _ip(status)))
        return out, status

    def histnd_batch(self, dims, cols, binmin, width, nb, want_h=True, want_likes=False, want_lmin=False, loglike_col=-1):
        """Raw N-D histograms of B densities in one call (gd_histnd_batch): density b bins the dims[b] columns
        cols[o_b:o_b + dims[b]] (axis 0 first; binmin / width laid out like cols) into nb bins per axis.  Returns
        (H, HL, Lmin): flat host arrays holding the B grids back to back (density b: nb**dims[b] entries, axis 0 fastest),
        None for an output not asked for.  HL needs the like weights of like_weights(..., mode=0)."""
        dims, cols, binmin, width = _i32arr(dims), _i32arr(cols), _f64arr(binmin), _f64arr(width)
        if cols.size != int(dims.sum()) or binmin.size != cols.size or width.size != cols.size:
            raise ValueError("cols, binmin and width need one entry per axis of every density")
        total = int(sum(int(nb) ** int(d) for d in dims))
        flags = (GD_HISTND_H if want_h else 0) | (GD_HISTND_LIKES if want_likes else 0) | (GD_HISTND_LMIN if want_lmin else 0)
        out = [np.empty(total) if f & flags else None for f in (GD_HISTND_H, GD_HISTND_LIKES, GD_HISTND_LMIN)]
        self._check(self.lib.gd_histnd_batch(self.h, len(dims), _ip(dims), _ip(cols), _dp(binmin), _dp(width), int(nb),
                                             flags, int(loglike_col), *[None if a is None else _dp(a) for a in out]))
        return tuple(out)

    def pca_corr(self, cols, maps):
        """Steps 1-2 of MCSamples.PCA (gd_pca_corr) over resident columns ``cols`` with per-column maps (0 N, 1 L, 2 M),
        sample weights.  Returns (mean, sd, corr): the weighted means of the mapped columns, their standard deviations,
        and the n x n weighted correlation matrix of the standardised columns (diagonal 1)."""
        cols, maps = _i32arr(cols), _i32arr(maps)
        if maps.size != cols.size:
            raise ValueError("one map per column")
        n = cols.size
        mean, sd, corr = np.empty(n), np.empty(n), np.empty((n, n))
        self._check(self.lib.gd_pca_corr(self.h, _ip(cols), n, _ip(maps), _dp(mean), _dp(sd), _dp(corr)))
        return mean, sd, corr

    def pca_project(self, cols, maps, mean, sd, U, doexp, all_means, all_sd):
        """Steps 4-5 of MCSamples.PCA (gd_pca_project): per row p = U z (z: the standardised mapped columns), exp(p) when
        ``doexp``.  Returns (newmean, newsd, pcpc, pcpar): weighted mean and standard deviation of each component, the
        np x np correlations of the standardised components and their np x n_all correlations with the first n_all
        resident columns standardised by ``all_means`` / ``all_sd``."""
        cols, maps, mean, sd = _i32arr(cols), _i32arr(maps), _f64arr(mean), _f64arr(sd)
        U, all_means, all_sd = _f64arr(U), _f64arr(all_means), _f64arr(all_sd)
        n, n_all = cols.size, all_means.size
        if maps.size != n or mean.size != n or sd.size != n or U.shape != (n, n) or all_sd.size != n_all:
            raise ValueError("pca_project: inconsistent shapes")
        newmean, newsd, pcpc, pcpar = np.empty(n), np.empty(n), np.empty((n, n)), np.empty((n, n_all))
        self._check(self.lib.gd_pca_project(self.h, _ip(cols), n, _ip(maps), _dp(mean), _dp(sd), _dp(U), int(bool(doexp)),
                                            n_all, _dp(all_means), _dp(all_sd), _dp(newmean), _dp(newsd), _dp(pcpc),
                                            _dp(pcpar)))
        return newmean, newsd, pcpc, pcpar

    def mixture_nll(self, cols, means, whiten, logcoef, lo=0, hi=None):
        """-log pdf of a Gaussian mixture at the rows [lo, hi) of the resident columns ``cols`` (gd_mixture_nll):
        ``means`` (K, d), ``whiten`` (K, d, d) lower-triangular inverse Cholesky factors of the covariances, ``logcoef`` (K)
        = log(weight) - log(norm).  Returns a host float64 vector of hi - lo values (a view of page-locked memory)."""
        cols, means, whiten, logcoef = _i32arr(cols), _f64arr(means), _f64arr(whiten), _f64arr(logcoef)
        d, K = cols.size, logcoef.size
        if means.shape != (K, d) or whiten.shape != (K, d, d):
            raise ValueError("mixture_nll: inconsistent shapes")
        hi = self.N if hi is None else int(hi)
        out = self.pinned_array((max(hi - int(lo), 0),))
        self._check(self.lib.gd_mixture_nll(self.h, _ip(cols), d, K, _dp(means), _dp(whiten), _dp(logcoef), int(lo), hi,
                                            _dp(out)))
        return out

    # ---- auxiliary vectors
    EXTRA_COLS = 4

    def set_extra_column(self, slot, x):
        """Copy a host vector into spare column ``slot``; returns the column index (n + slot) it is addressed by."""
        x = _f64arr(x)
        if x.shape != (self.N,):
            raise ValueError("vector must have one entry per sample row")
        self._check(self.lib.gd_set_extra_column(self.h, int(slot), _dp(x)))
        return self.n + int(slot)

    def aux_weights(self, w):
        w = _f64arr(w)
        if w.shape != (self.N,):
            raise ValueError("weights must have one entry per sample row")
        self._check(self.lib.gd_aux_weights(self.h, _dp(w)))

    def expr_eval(self, code, consts, dst, dst_arg=0, lo=0, hi=None, stats=False, tables=None):
        """Evaluate the postfix program ``code`` ((ncode, 2) int32 of (op, arg), constants ``consts``) over the rows [lo, hi)
        of the resident columns (gd_expr_eval).  ``dst``: GD_EX_TO_COLUMN (spare slot ``dst_arg``; returns the column index
        n + dst_arg), GD_EX_TO_AUXW (the auxiliary weight buffer receives sample weight * value; returns None),
        GD_EX_TO_HOST_F64 / GD_EX_TO_HOST_U8 (returns the hi - lo values as float64 / as bytes value != 0: views of
        page-locked memory that the context recycles).  With ``stats`` the result is (that, [min, max, non-zero, NaNs]).
        ``tables``: the colexpr.Table objects the program's look-up ops refer to by slot (gd_expr_eval_tab); None or
        empty for a program without."""
        code = np.ascontiguousarray(code, dtype=np.int32).reshape(-1, 2)
        consts = _f64arr(consts).ravel()
        hi = self.N if hi is None else int(hi)
        out = None
        if dst in (GD_EX_TO_HOST_F64, GD_EX_TO_HOST_U8):
            out = self.pinned_array((max(hi - int(lo), 0),), np.float64 if dst == GD_EX_TO_HOST_F64 else np.uint8)
        st = np.zeros(4) if stats else None
        args = (self.h, _ip(code), len(code), _dp(consts), consts.size, int(dst), int(dst_arg), int(lo), hi,
                None if out is None else out.ctypes.data, None if st is None else _dp(st))
        if tables:
            self._check(self.lib.gd_expr_eval_tab(*args, expr_table_structs(tables), len(tables)))
        else:
            self._check(self.lib.gd_expr_eval(*args))
        res = self.n + int(dst_arg) if dst == GD_EX_TO_COLUMN else out
        return (res, st) if stats else res

    def col_minmax(self, cols, lo=0, hi=None, cond_col=-1, cond_below=0.0):
        """min / max per column over the rows whose ``cond_col`` value is < ``cond_below`` (cond_col < 0: all rows)."""
        cols = _i32arr(cols)
        out = np.zeros((len(cols), 2))
        self._check(self.lib.gd_col_minmax(self.h, _ip(cols), len(cols), lo, self.N if hi is None else hi,
                                           int(cond_col), float(cond_below), _dp(out)))
        return out

    # ---- contour levels
    def contour_levels(self, d_P, B, F, contours):
        contours = _f64arr(contours)
        out = np.zeros((B, len(contours)))
        status = np.zeros(B, dtype=np.int32)
        self._check(self.lib.gd_contour_levels(self.h, int(B), int(F), d_P.ptr, _dp(contours), len(contours), _dp(out),
                                               _ip(status)))
        return out, status

    # ---- contour paths
    def contour_paths(self, d_grids, grid_off, ny, nx, x_axes, x_off, y_axes, y_off, levels):
        """gd_contour_paths over B grids at ``d_grids`` (a device buffer or address; grid b is ny[b] x nx[b] doubles from element
        grid_off[b] on), its axes the nx[b] entries of ``x_axes`` from x_off[b] on and the ny[b] of ``y_axes`` from y_off[b] on
        (grids may share an axis), and ``levels`` (B, nc).  Returns (xy (V, 2)
        float64, flag (V) uint8, loops (L) int32, task_vert_off (B*nc + 1) int64, task_loop_off (B*nc + 1) int64, status (B)
        int32): task b*nc + c owns the vertices [task_vert_off[t], task_vert_off[t+1]) and the loops
        [task_loop_off[t], task_loop_off[t+1]), ``loops`` holding each loop's first vertex relative to its task's;
        status[b] != 0 marks a grid with a non-finite value (then nothing was traced).  Results above 1 MB are views of
        page-locked memory that the context recycles once they are released."""
        grid_off = np.ascontiguousarray(grid_off, dtype=np.int64)
        ny, nx, x_axes, y_axes = _i32arr(ny), _i32arr(nx), _f64arr(x_axes).reshape(-1), _f64arr(y_axes).reshape(-1)
        x_off, y_off = np.ascontiguousarray(x_off, dtype=np.int64), np.ascontiguousarray(y_off, dtype=np.int64)
        levels = _f64arr(levels)
        B = len(ny)
        if levels.ndim != 2 or levels.shape[0] != B or not (len(nx) == len(grid_off) == len(x_off) == len(y_off) == B):
            raise ValueError("contour_paths: one size, one grid offset, two axis offsets and one row of levels per grid")
        nc = levels.shape[1]
        T = B * nc
        voff, loff = np.zeros(T + 1, dtype=np.int64), np.zeros(T + 1, dtype=np.int64)
        status = np.zeros(max(B, 1), dtype=np.int32)
        kinds = {GD_PATHS_XY: (np.float64, 2), GD_PATHS_FLAG: (np.uint8, 1), GD_PATHS_LOOPS: (np.int32, 1)}
        got = {}

        def alloc(user, which, count):
            try:  # (never let an exception unwind through the C frames)
                dtype, per = kinds[which]
                n = int(count) * per
                if n * np.dtype(dtype).itemsize > (1 << 20):
                    a = self.pinned_array((n,), dtype)
                else:
                    a = np.empty(max(n, 1), dtype=dtype)[:n]
                got[which] = a
                return a.ctypes.data
            except Exception:
                return None

        cb = PATHS_ALLOC_FN(alloc)
        ptr = d_grids.ptr if isinstance(d_grids, DevBuf) else d_grids
        self._check(self.lib.gd_contour_paths(self.h, B, ptr, grid_off.ctypes.data_as(_pi64), _ip(ny), _ip(nx), _dp(x_axes),
                                              x_off.ctypes.data_as(_pi64), x_axes.size, _dp(y_axes),
                                              y_off.ctypes.data_as(_pi64), y_axes.size, _dp(levels), nc, C.cast(cb, _p), None, voff.ctypes.data_as(_pi64),
                                              loff.ctypes.data_as(_pi64), _ip(status)))
        # (pop: the callback object and its closure form a cycle that only the collector frees; what it still held would
        # keep the page-locked blocks from being recycled until then)
        xy = got.pop(GD_PATHS_XY, np.zeros(0)).reshape(-1, 2)
        flag = got.pop(GD_PATHS_FLAG, np.zeros(0, dtype=np.uint8))
        loops = got.pop(GD_PATHS_LOOPS, np.zeros(0, dtype=np.int32))
        return xy, flag, loops, voff, loff, status[:B]

    def density2d_enqueue(self, d_hist, B, F, rx, ry, corr, winw, flags, bco, mbc, status):
        """density2d without the final wait: ``status`` is a page-locked int32 array of length B (pinned_array) that is
        valid after sync() / copy_sync() of a later to_host_async; the returned grids likewise."""
        out = self.alloc(B * F * F * 8)
        rx, ry, corr, winw, flags = _f64arr(rx), _f64arr(ry), _f64arr(corr), _i32arr(winw), _i32arr(flags)
        assert status.dtype == np.int32 and status.size == B and status.flags.c_contiguous
        self._check(self.lib.gd_density2d_enqueue(self.h, B, F, d_hist.ptr if isinstance(d_hist, DevBuf) else d_hist,
                                                  _dp(rx), _dp(ry), _dp(corr), _ip(winw), _ip(flags), int(bco), int(mbc),
                                                  out.ptr, status.ctypes.data))
        return out

    # ---- credible limits
    def limits1d(self, P, x0, spacing, contours, factor=0):
        """(limits[B, nc, 4] = lower, upper, has_min, has_top; status[B]) of B densities P[B, F] on regular grids."""
        P, x0, spacing, contours = _f64arr(P), _f64arr(x0), _f64arr(spacing), _f64arr(contours)
        B, F = P.shape
        out = np.zeros((B, len(contours), 4))
        status = np.zeros(B, dtype=np.int32)
        self._check(self.lib.gd_limits1d(self.h, B, F, _dp(P), _dp(x0), _dp(spacing), _dp(contours), len(contours),
                                         int(factor), _dp(out), _ip(status)))
        return out, status

    # ---- thinned chains
    def weights_integral(self):
        out = C.c_int32()
        self._check(self.lib.gd_weights_integral(self.h, C.byref(out)))
        return bool(out.value)

    def thin_rows(self, lo, hi, factor, unique_mode, capacity):
        """Thinned row list (device int32 buffer, count) of chain rows [lo,hi); see gd_thin_rows."""
        buf = self.alloc(max(int(capacity), 1) * 4)
        n = C.c_int64()
        self._check(self.lib.gd_thin_rows(self.h, int(lo), int(hi), int(factor), int(bool(unique_mode)), buf.ptr,
                                          int(capacity), C.byref(n)))
        return buf, n.value

    def binary_transitions(self, cols, rows, K, thresholds):
        cols = _i32arr(cols)
        thresholds = _f64arr(thresholds).reshape(len(cols), -1)
        out = np.zeros((len(cols), thresholds.shape[1], 12), dtype=np.int64)
        self._check(self.lib.gd_binary_transitions(self.h, _ip(cols), len(cols), rows.ptr, int(K), _dp(thresholds),
                                                   thresholds.shape[1], out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def thinned_lag_sums(self, cols, means, rows, K, maxoff):
        cols, means = _i32arr(cols), _f64arr(means)
        out = np.zeros((len(cols), int(maxoff)))
        self._check(self.lib.gd_thinned_lag_sums(self.h, _ip(cols), len(cols), _dp(means), rows.ptr, int(K), int(maxoff),
                                                 _dp(out)))
        return out

    # ---- weight-one sample draws
    def draw_single_rows(self, a, b, mode=0, pcg=None, rand=None, capacity=None):
        """Rows kept by a weight-one draw (gd_draw_single_rows): row i when rand_i <= w_i / (a * b) (mode 0) or
        (w_i / a) / b (mode 1).  ``pcg`` = (state, inc), the two 128-bit integers of a PCG64 bit generator's state, draws the
        variates on the device; ``rand`` (N doubles drawn on the host) is the route of every other generator.  Returns
        (rows, K): a device int32 buffer with the K kept rows in ascending order.  ``capacity`` (default N, which always
        fits) bounds the buffer; when the draw keeps more, nothing is written and (None, K) comes back."""
        if (pcg is None) == (rand is None):
            raise ValueError("draw_single_rows takes the PCG64 state or a vector of variates")
        capacity = self.N if capacity is None else int(capacity)
        st, d_rand = None, None
        if pcg is not None:
            m64 = (1 << 64) - 1
            state, inc = int(pcg[0]), int(pcg[1])
            st = (C.c_uint64 * 4)(state >> 64, state & m64, inc >> 64, inc & m64)
        else:
            rand = _f64arr(rand)
            if rand.shape != (self.N,):
                raise ValueError("one variate per sample row")
            d_rand = self.alloc(rand.nbytes)
            d_rand.from_host(rand)
        buf = self.alloc(max(capacity, 1) * 4)
        n = C.c_int64()
        try:
            rc = self.lib.gd_draw_single_rows(self.h, st, None if d_rand is None else d_rand.ptr, float(a), float(b), int(mode),
                                              buf.ptr, capacity, C.byref(n))
        finally:
            if d_rand is not None:
                d_rand.free()
        if rc == GD_DRAW_MORE_ROWS:
            buf.free()
            return None, n.value
        if rc != 0:
            buf.free()
        self._check(rc)
        return buf, n.value

    def gather_rows(self, rows, K, cols):
        """(K, len(cols)) host array of the resident columns ``cols`` (any order, repeats allowed) at the K rows of the
        device row list ``rows`` (gd_gather_rows)."""
        cols = _i32arr(cols)
        K = int(K)
        out = np.empty((K, cols.size))
        if cols.size == 0:
            return out
        d_out = self.alloc(max(out.nbytes, 8))
        try:
            self._check(self.lib.gd_gather_rows(self.h, rows.ptr, K, _ip(cols), cols.size, d_out.ptr))
            self._check(self.lib.gd_memcpy_d2h(self.h, out.ctypes.data, d_out.ptr, out.nbytes))
        finally:
            d_out.free()
        return out

    # ---- chain export
    def _format_finish(self, call, rows, m, width, prec, out, host):
        need = max(int(rows) * int(m) * format_field_bytes(width, prec), 1)
        buf = self.alloc(need) if out is None else out
        n = C.c_int64()
        rc = call(buf.ptr, int(buf.nbytes), C.byref(n))
        if rc == GD_FORMAT_MORE_BYTES:  # only a caller-supplied buffer can be too small
            return None, n.value
        if rc != 0 and out is None:
            buf.free()
        self._check(rc)
        if host is not None and n.value:
            view = np.asarray(host).reshape(-1).view(np.uint8)
            if view.size < n.value:
                raise ValueError("host buffer holds %d bytes, the text takes %d" % (view.size, n.value))
            self._check(self.lib.gd_memcpy_d2h(self.h, view.ctypes.data, buf.ptr, n.value))
        return buf, n.value

    def format_rows(self, srcs, lo=None, hi=None, rows=None, K=None, row_offset=0, width=0, prec=8, upper=False, sep=True,
                    out=None, host=None):
        """Text of sample rows as np.savetxt(fmt="%W.Pe") writes it (gd_format_rows): field j is the resident column
        srcs[j] (spare columns included), GD_FMT_SRC_WEIGHT, GD_FMT_SRC_ZERO or GD_FMT_SRC_ONE; the rows are [lo, hi) or the K
        rows of the device int32 list ``rows`` from entry ``row_offset`` on.  Returns (device buffer, bytes); ``out`` supplies the buffer (when it is too
        small nothing is written and (None, bytes needed) comes back), ``host`` (page-locked uint8) also receives the text."""
        srcs = _i32arr(srcs)
        if (rows is None) == (lo is None):
            raise ValueError("format_rows takes a row interval or a device row list")
        if rows is None:
            nrows, sel = int(hi) - int(lo), (int(lo), int(hi), None, 0)
        else:
            nrows, sel = int(K), (0, 0, rows.ptr + 4 * int(row_offset), int(K))

        def call(ptr, cap, n):
            return self.lib.gd_format_rows(self.h, _ip(srcs), srcs.size, sel[0], sel[1], sel[2], sel[3], int(width), int(prec),
                                           int(bool(upper)), int(bool(sep)), ptr, cap, n)

        return self._format_finish(call, max(nrows, 0), srcs.size, width, prec, out, host)

    def format_matrix(self, x, width=0, prec=8, upper=False, sep=True, out=None, host=None, shape=None, strides=None):
        """Text of a 2D fp64 matrix (gd_format_matrix).  ``x`` is a host array (uploaded here) or a device buffer with
        ``shape`` = (K, m) and ``strides`` = (row, column) in elements.  Returns (device buffer, bytes) as format_rows."""
        tmp = None
        if isinstance(x, DevBuf) or shape is not None:
            (K, m), (rs, cs), src = shape, strides, x
        else:
            x = np.ascontiguousarray(x, dtype=np.float64)
            if x.ndim != 2:
                raise ValueError("format_matrix takes a 2D array")
            (K, m), (rs, cs) = x.shape, (x.shape[1], 1)
            tmp = src = self.alloc(max(x.nbytes, 8))
            src.from_host(x)
        ptr0 = src.ptr

        def call(ptr, cap, n):
            return self.lib.gd_format_matrix(self.h, ptr0 if K else None, int(K), int(m), int(rs), int(cs), int(width), int(prec),
                                             int(bool(upper)), int(bool(sep)), ptr, cap, n)

        try:
            return self._format_finish(call, K, m, width, prec, out, host)
        finally:
            if tmp is not None:
                tmp.free()

    def fetch_bytes_async(self, buf, host, nbytes):
        """Start the copy of the first ``nbytes`` of a device buffer into the page-locked uint8 array ``host`` on the copy
        stream (ordered after the compute stream's work so far); copy_mark() / copy_wait() tell when it has landed."""
        if nbytes:
            self._check(self.lib.gd_memcpy_d2h_async(self.h, host.ctypes.data, buf.ptr, int(nbytes)))

    # ---- chain ingestion
    PARSE_CHUNK_BYTES = 64 << 20  # text per read / copy / scan step of parse_text: two page-locked blocks of this size
    PARSE_MEMORY_SHARE = 0.5      # parse_text declines a text that, with its output, exceeds this share of the free HBM
    PARSE_FIX_CAPACITY = 1 << 16  # undecided tokens listed per parse_rows call; more makes parse_text decline

    def parse_scan(self, text, nbytes, last=True, offset=0):
        """gd_parse_scan of ``nbytes`` bytes of the device buffer ``text`` from ``offset`` on: (status, data rows, fields per
        row, bytes consumed) with status GD_OK or GD_PARSE_NOT_PLAIN; any other error raises."""
        rows, m, used = C.c_int64(), C.c_int32(), C.c_int64()
        rc = self.lib.gd_parse_scan(self.h, (text.ptr + int(offset)) if text is not None else None, int(nbytes), int(bool(last)),
                                    C.byref(rows), C.byref(m), C.byref(used))
        if rc != GD_PARSE_NOT_PLAIN:
            self._check(rc)
        return rc, rows.value, m.value, used.value

    def parse_rows(self, text, nbytes, rows, m, out, ld, row_offset=0, last=True, fix_capacity=None, offset=0):
        """gd_parse_rows: field j of data row r of the text goes to element j * ld + row_offset + r of the fp64 device
        buffer ``out``.  Returns (status, fixes, fix count): ``fixes`` is the (k, 4) int64 array of the listed undecided
        tokens -- (row in ``out``, field, byte offset from ``offset``, length) -- and k < fix count when the list was
        short.  ``out`` must hold at least m * ld values (checked here: the library sees only a pointer)."""
        cap = self.PARSE_FIX_CAPACITY if fix_capacity is None else int(fix_capacity)
        if out is not None and int(m) * int(ld) * 8 > out.nbytes:
            raise ValueError("the output buffer holds %d bytes, m * ld values take %d" % (out.nbytes, int(m) * int(ld) * 8))
        fix = self.alloc(cap * 32) if cap > 0 else None
        n = C.c_int64()
        try:
            rc = self.lib.gd_parse_rows(self.h, (text.ptr + int(offset)) if text is not None else None, int(nbytes), int(bool(last)),
                                        int(rows), int(m), out.ptr if out is not None else None, int(ld), int(row_offset),
                                        fix.ptr if fix is not None else None, cap, C.byref(n))
            if rc != GD_PARSE_NOT_PLAIN:
                self._check(rc)
            k = min(n.value, cap) if rc == 0 else 0
            fixes = fix.to_host((k, 4), dtype=np.int64) if k else np.zeros((0, 4), dtype=np.int64)
        finally:
            if fix is not None:
                fix.free()
        return rc, fixes, n.value

    def parse_text(self, source, skiprows=0, chunk_bytes=None, alloc=None):
        """
        np.loadtxt of a whole text on the device.  ``source`` is a path or a bytes-like object; ``skiprows`` line ends are
        passed over on the host first.  The text is read in chunks of ``chunk_bytes`` into two page-locked blocks by a
        helper thread and copied into ONE device buffer that holds the whole text; the read of chunk k + 1 overlaps the
        copy and the gd_parse_scan of chunk k.  Every scan starts behind the last line end the previous one consumed, so a
        line that straddles a chunk boundary is scanned once it is whole.  With the row and field counts known the
        m x N output is allocated, gd_parse_rows runs once per scanned piece, and the block is fetched once into
        page-locked memory (``alloc``, default pinned_block).

        Returns None when the device route declines -- a text that is not plain (GD_PARSE_NOT_PLAIN), skipped lines that
        only a text-mode reader can count (skipped_text_bytes), no rows, a short fix list, text plus output above
        PARSE_MEMORY_SHARE of the free device memory, or an allocation that fails (GD_ERR_NOMEM) -- and otherwise
        dict(array=(N, m) column-major view, fixes=[(row, field, byte offset in the source, length), ...]): the listed
        tokens hold NaN and are the caller's to convert (chainfiles.loadNumpyTxt uses float()).
        """
        import io
        import threading
        import queue

        if isinstance(source, (bytes, bytearray, memoryview)):
            f = io.BytesIO(bytes(source))
            size = len(source)
        else:
            f = open(os.fspath(source), "rb")
            size = os.path.getsize(os.fspath(source))
        text = out = None
        reader = None
        stop = []
        try:
            start = skipped_text_bytes(f, skiprows)
            if start is None:
                return None
            total = size - start
            if total <= 0:
                return None
            free_hbm = self.device_info()["hbm_free"]
            if total > self.PARSE_MEMORY_SHARE * free_hbm:
                return None
            chunk = max(int(chunk_bytes or self.PARSE_CHUNK_BYTES), 1)
            chunk = min(chunk, total)
            text = self.alloc(total)
            host = [self.pinned_array((chunk,), np.uint8) for _ in range(2 if total > chunk else 1)]
            free, todo = queue.Queue(), queue.Queue()
            for b in range(len(host)):
                free.put(b)

            def read_chunks():  # fills the page-locked blocks in turn; the caller's thread copies and scans them
                try:
                    done = 0
                    while done < total and not stop:
                        b = free.get()
                        if b is None:
                            return
                        want = min(chunk, total - done)
                        got = f.readinto(memoryview(host[b])[:want])
                        if got != want:
                            raise OSError("short read: the file changed while it was being parsed")
                        done += got
                        todo.put((b, got))
                    todo.put(None)
                except BaseException as e:  # noqa: BLE001 -- handed to the caller's thread
                    todo.put(e)

            reader = threading.Thread(target=read_chunks, name="getdist_amd-text-reader")
            reader.start()
            pieces, m, N = [], 0, 0  # (offset, bytes, rows, last) of every scanned piece
            have = scanned = 0
            while True:
                item = todo.get()
                if isinstance(item, BaseException):
                    raise item
                if item is not None:
                    b, got = item
                    self._check(self.lib.gd_memcpy_h2d(self.h, text.ptr + have, host[b].ctypes.data, got))
                    free.put(b)
                    have += got
                last = have == total
                rc, rows, fields, used = self.parse_scan(text, have - scanned, last=last, offset=scanned)
                if rc != 0:
                    return None
                if rows:
                    if m and fields != m:
                        return None
                    m = fields
                if used:
                    pieces.append((scanned, used, rows, last))
                    scanned += used
                    N += rows
                if last:
                    break
            if N == 0:
                return None
            if total + 8 * m * N > self.PARSE_MEMORY_SHARE * free_hbm:
                return None
            out = self.alloc(8 * m * N)
            fixes, row0 = [], 0
            for off, nb, rows, last in pieces:
                if rows:
                    rc, fx, count = self.parse_rows(text, nb, rows, m, out, N, row_offset=row0, last=last, offset=off)
                    if rc != 0 or count > len(fx):
                        return None
                    fixes += [(int(r), int(j), int(o) + off + start, int(ln)) for r, j, o, ln in fx]
                row0 += rows
            flat = (alloc or self.pinned_block)((m * N,), np.float64)
            self._check(self.lib.gd_memcpy_d2h(self.h, flat.ctypes.data, out.ptr, flat.nbytes))
            return dict(array=flat.reshape((m, N)).T, fixes=fixes)
        except GdhipError as e:
            if e.code != GD_ERR_NOMEM:
                raise
            return None  # the share of free memory was there, a block of it was not: the host route needs none
        finally:
            stop.append(True)
            if reader is not None:
                free.put(None)
                free.put(None)
                reader.join()
            f.close()
            for d in (text, out):
                if d is not None:
                    d.free()

    # ---- mean likelihoods
    def like_weights(self, loglikes, mode, mean_loglike):
        """Build (or with loglikes=None drop) the device vector w*exp(mean_loglike-loglikes) / w*loglikes."""
        if loglikes is None:
            self._check(self.lib.gd_like_weights(self.h, None, 0, 0.0, None))
            return None
        ll = _f64arr(loglikes)
        if ll.shape != (self.N,):
            raise ValueError("loglikes must have one entry per sample row")
        tot = C.c_double()
        self._check(self.lib.gd_like_weights(self.h, _dp(ll), int(mode), float(mean_loglike), C.byref(tot)))
        return tot.value

    def select_weights(self, which):
        self._check(self.lib.gd_select_weights(self.h, int(which)))

    def likes1d(self, hist, likehist, P, smooth, winw, flags, shade_mean_loglikes):
        hist, likehist, P = _f64arr(hist), _f64arr(likehist), _f64arr(P)
        B, F = hist.shape
        smooth, winw, flags = _f64arr(smooth), _i32arr(winw), _i32arr(flags)
        out = np.zeros_like(hist)
        status = np.zeros(B, dtype=np.int32)
        self._check(self.lib.gd_likes1d(self.h, B, F, _dp(hist), _dp(likehist), _dp(P), _dp(smooth), _ip(winw),
                                        _ip(flags), int(bool(shade_mean_loglikes)), _dp(out), _ip(status)))
        return out, status

    def likes2d(self, d_hist, d_likehist, B, F, rx, ry, corr, winw, flags, mbc):
        out = self.alloc(B * F * F * 8)
        rx, ry, corr, winw, flags = _f64arr(rx), _f64arr(ry), _f64arr(corr), _i32arr(winw), _i32arr(flags)
        status = np.zeros(B, dtype=np.int32)
        self._check(self.lib.gd_likes2d(self.h, B, F, d_hist.ptr, d_likehist.ptr, _dp(rx), _dp(ry), _dp(corr),
                                        _ip(winw), _ip(flags), int(mbc), out.ptr, _ip(status)))
        return out, status

    # ---- stand-alone convolutions / likelihood statistics
    def circ_convolve(self, a, b):
        """irfft(rfft(a) * rfft(b)) of two equal-shape real arrays (1-D or 2-D) through rocFFT."""
        a, b = _f64arr(a), _f64arr(b)
        if a.shape != b.shape or a.ndim not in (1, 2):
            raise ValueError("circ_convolve needs two arrays of one shape, one- or two-dimensional")
        n0, n1 = (1, a.shape[0]) if a.ndim == 1 else a.shape
        out = np.empty_like(a)
        self._check(self.lib.gd_circ_convolve(self.h, int(n0), int(n1), _dp(a), _dp(b), _dp(out)))
        return out

    def convolve1d_direct(self, x, y):
        x, y = _f64arr(x), _f64arr(y)
        out = np.empty(x.size + y.size - 1)
        self._check(self.lib.gd_convolve1d_direct(self.h, _dp(x), x.size, _dp(y), y.size, _dp(out)))
        return out

    def autoconvolve(self, s, n, normalize=True, x=None, col=-1, mean=0.0, use_weights=False):
        """autoConvolve of a host vector ``x`` or of (column - mean) * weights; ``s`` = nearestFFTnumber(2 N)."""
        out = np.empty(int(n))
        xx = None if x is None else _f64arr(x)
        self._check(self.lib.gd_autoconvolve(self.h, int(col), float(mean), int(bool(use_weights)),
                                             None if xx is None else _dp(xx), 0 if xx is None else xx.size, int(s), int(n),
                                             int(bool(normalize)), _dp(out)))
        return out

    def like_stats(self, col):
        out = np.zeros(8)
        self._check(self.lib.gd_like_stats(self.h, int(col), _dp(out)))
        return dict(min=out[0], max=out[1], norm=out[2], sum_wl=out[3], sum_wl2=out[4], sum_w_exp_plus=out[5],
                    sum_w_exp_minus=out[6], argmin=int(out[7]))

    # ---- one native entry for a batch of pairs (getdist_amd/batch2d.py packs the arguments)
    def batch2d_grid_sizes(self, settings, n, corr, pairs32):
        F = np.zeros(len(pairs32), dtype=np.int32)
        rc = self.lib.gd_batch2d_grid_sizes(C.byref(settings), int(n), _dp(corr), _ip(pairs32), len(pairs32), _ip(F))
        if rc != 0:
            raise GdhipError(rc, "gd_batch2d_grid_sizes: bad argument")
        return F

    def density2d_batch(self, twin, settings, params, n, corr, cov, lag_probe, pairs32, exchange, grids, status, meta, levels,
                        level_status):
        """gd_density2d_batch; returns the copy-stream tokens (this context's, the twin's)."""
        tokens = np.full(2, -1, dtype=np.int32)
        self._check(self.lib.gd_density2d_batch(
            self.h, None if twin is None else twin.h, C.byref(settings), C.cast(params, _p), int(n), _dp(corr), _dp(cov),
            None if lag_probe is None else _dp(lag_probe), _ip(pairs32), len(pairs32),
            None if exchange is None else C.cast(exchange, _p), None, grids.ctypes.data, int(grids.size),
            status.ctypes.data_as(_pi32), _dp(meta), None if levels is None else _dp(levels),
            None if level_status is None else _ip(level_status), _ip(tokens)))
        return int(tokens[0]), int(tokens[1])

    # ---- RCCL communicator of a multi-GPU job (one process per GPU)
    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(128)
        rc = load_library().gd_comm_unique_id(buf)
        if rc != 0:
            raise GdhipError(rc, "gd_comm_unique_id failed (librccl.so missing?)")
        return buf.raw

    def comm_init(self, world, rank, id128):
        self._check(self.lib.gd_comm_init(self.h, int(world), int(rank), C.create_string_buffer(bytes(id128), 128)))
        self.comm_world, self.comm_rank = int(world), int(rank)

    def comm_allgather(self, vec):
        """(world, len(vec)) array: every rank's vector, through ncclAllGather on the context's stream."""
        v = _f64arr(vec).ravel()
        out = np.empty((self.comm_world, v.size))
        self._check(self.lib.gd_comm_allgather(self.h, _dp(v), v.size, _dp(out)))
        return out

    def comm_allreduce_sum(self, vec):
        v = _f64arr(vec).ravel().copy()
        self._check(self.lib.gd_comm_allreduce_sum(self.h, _dp(v), v.size))
        return v

    def comm_destroy(self):
        self._check(self.lib.gd_comm_destroy(self.h))
        self.comm_world = 0

    def comm_info(self):
        """(world, rank) of the context's communicator as the LIBRARY sees it; (0, 0) when there is none (never made, or
        aborted and dropped after a timeout)."""
        wd, rk = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.gd_comm_info(self.h, C.byref(wd), C.byref(rk)))
        return int(wd.value), int(rk.value)

    def comm_abandon(self):
        """The one call that may be made from another thread while a gd_comm_* call of this context has not returned: a
        gd_comm_init that comes back after its caller gave up installs nothing."""
        if self.h is not None:
            self.lib.gd_comm_abandon(self.h)

    def density1d_batch(self, settings, params, n, cols32, want_hist=False):
        """gd_density1d_batch: (P[B, F], hist[B, F] or None, meta[B, 9]) of the listed columns."""
        cols32 = _i32arr(cols32)
        B, F = len(cols32), int(settings.fine_bins)
        P = np.zeros((B, F))
        hist = np.zeros((B, F)) if want_hist else None
        meta = np.zeros((B, 9))
        self._check(self.lib.gd_density1d_batch(self.h, C.byref(settings), C.cast(params, _p), int(n), _ip(cols32), B, _dp(P),
                                                None if hist is None else _dp(hist), _dp(meta)))
        return P, hist, meta

    def batch2d_finish(self):
        self._check(self.lib.gd_batch2d_finish(self.h))

    def batch2d_invalidate(self):
        self._check(self.lib.gd_batch2d_invalidate(self.h))

    def batch2d_exchanges(self):
        """N_eff collectives gd_density2d_batch has entered on this context so far (also by calls that failed later)."""
        c = C.c_int64(0)
        self._check(self.lib.gd_batch2d_exchanges(self.h, C.byref(c)))
        return int(c.value)

    def kopt2d(self, d_hist, B, F, neff, do_corr, fallback_t, corr):
        """B x 12: {t*, psi_02, psi_20, psi_11, psi_00, psi_13, psi_31, status, hx, hy, corr, get_h status}"""
        neff, do_corr, fallback_t, corr = _f64arr(neff), _i32arr(do_corr), _f64arr(fallback_t), _f64arr(corr)
        out = np.zeros((B, 12))
        self._check(self.lib.gd_kopt2d(self.h, B, F, d_hist.ptr if isinstance(d_hist, DevBuf) else d_hist, _dp(neff),
                                       _ip(do_corr), _dp(fallback_t), _dp(corr), _dp(out)))
        return out

    def get_h(self, psi, neff, corr, do_corr):
        """B x 4 {hx, hy, corr, status} from the functionals psi (B x 6): KernelOptimizer2D.get_h on the device."""
        psi, neff, corr, do_corr = _f64arr(psi).reshape(-1, 6), _f64arr(neff), _f64arr(corr), _i32arr(do_corr)
        out = np.zeros((len(psi), 4))
        self._check(self.lib.gd_get_h(self.h, len(psi), _dp(psi), _dp(neff), _dp(corr), _ip(do_corr), _dp(out)))
        return out

    def density2d(self, d_hist, B, F, rx, ry, corr, winw, flags, bco, mbc, out=None):
        out = out or self.alloc(B * F * F * 8)
        rx, ry, corr, winw, flags = _f64arr(rx), _f64arr(ry), _f64arr(corr), _i32arr(winw), _i32arr(flags)
        status = np.zeros(B, dtype=np.int32)
        self._check(self.lib.gd_density2d(self.h, B, F, d_hist.ptr if isinstance(d_hist, DevBuf) else d_hist, _dp(rx),
                                          _dp(ry), _dp(corr), _ip(winw), _ip(flags), int(bco), int(mbc), out.ptr,
                                          _ip(status)))
        return out, status
