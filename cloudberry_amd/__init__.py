"""cloudberry_amd — Python plumbing around libgpuexec.so (the C-ABI product
path; see include/gpuexec.h).  This wrapper exists for tests and the bench
harness; the library itself has no Python or torch dependency.

The GPU path NEVER falls back to CPU: if the HIP library is missing or no
device is usable, every entry point raises."""
import ctypes
import os

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(_ROOT, "cloudberry_amd", "libgpuexec.so")

TPCH_CUSTOMER, TPCH_ORDERS, TPCH_LINEITEM = 0, 1, 2
TPCH_LINEITEM_NUMERIC = 3
TPCH_LINEITEM_RLEKEY = 4
TPCH_LINEITEM_Q1 = 5
CUTOFF_19950315 = -1753  # DateADT of 1995-03-15 (validated vs oracle in tests)

_STATUS = {0: "GX_OK", 1: "GX_ERR_HIP", 2: "GX_ERR_RCCL", 3: "GX_ERR_INVALID",
           4: "GX_ERR_CHECKSUM", 5: "GX_ERR_OOM", 6: "GX_ERR_NOGPU", 7: "GX_ERR_STATE"}


class GxError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        super().__init__(f"{_STATUS.get(status, status)}: {detail}")


class _Group(ctypes.Structure):
    _fields_ = [("l_orderkey", ctypes.c_int64),
                ("o_orderdate", ctypes.c_int32),
                ("o_shippriority", ctypes.c_int32),
                ("revenue", ctypes.c_double),
                ("revenue_num", ctypes.c_int64),
                ("nitems", ctypes.c_int64),
                ("key_is_null", ctypes.c_uint8),
                ("attrs_null", ctypes.c_uint8),
                ("_pad", ctypes.c_uint8 * 6)]


# numpy mirror of gx_q3_group (48 B)
Q3_GROUP_DTYPE = np.dtype([("l_orderkey", np.int64), ("o_orderdate", np.int32),
                           ("o_shippriority", np.int32),
                           ("revenue", np.float64), ("revenue_num", np.int64),
                           ("nitems", np.int64), ("key_is_null", np.uint8),
                           ("attrs_null", np.uint8), ("_pad", np.uint8, (6,))])


class _Stats(ctypes.Structure):
    _fields_ = [("ms_cust_build", ctypes.c_double),
                ("ms_orders_build", ctypes.c_double),
                ("ms_probe_agg", ctypes.c_double),
                ("ms_extract", ctypes.c_double),
                ("ms_motion", ctypes.c_double),
                ("ms_total", ctypes.c_double),
                ("cust_rows", ctypes.c_int64),
                ("ord_rows", ctypes.c_int64),
                ("li_rows", ctypes.c_int64),
                ("probe_hits", ctypes.c_int64),
                ("groups", ctypes.c_int64),
                ("bytes_scanned", ctypes.c_double),
                ("ms_motion_counts", ctypes.c_double),
                ("ms_motion_payload", ctypes.c_double)]


class _KvGroup(ctypes.Structure):
    _fields_ = [("key", ctypes.c_int64), ("key_is_null", ctypes.c_uint8),
                ("_pad", ctypes.c_uint8 * 7), ("sum", ctypes.c_double),
                ("count", ctypes.c_int64)]


# numpy mirror of gx_kv_group (the two-stage GROUP BY wire row, 32 B)
KV_GROUP_DTYPE = np.dtype([("key", np.int64), ("key_is_null", np.uint8),
                           ("_pad", np.uint8, (7,)), ("sum", np.float64),
                           ("count", np.int64)])


class _GbStats(ctypes.Structure):
    _fields_ = [("ms_partial", ctypes.c_double),
                ("ms_partition", ctypes.c_double),
                ("ms_exchange", ctypes.c_double),
                ("ms_combine", ctypes.c_double),
                ("rows_in", ctypes.c_int64),
                ("partial_groups", ctypes.c_int64),
                ("sent_rows", ctypes.c_int64),
                ("recv_rows", ctypes.c_int64),
                ("final_groups", ctypes.c_int64)]


class _Filter(ctypes.Structure):
    _fields_ = [("col", ctypes.c_int32), ("op", ctypes.c_int32),
                ("literal", ctypes.c_int64)]


GB_MAX_KEYS, GB_MAX_AGGS, MAX_EXTRA_QUALS = 4, 8, 4
AGG_COUNT_STAR, AGG_COUNT, AGG_SUM, AGG_MIN, AGG_MAX = 0, 1, 2, 3, 4
_AGG_FNS = {"count*": AGG_COUNT_STAR, "count": AGG_COUNT, "sum": AGG_SUM,
            "min": AGG_MIN, "max": AGG_MAX}


class _Agg(ctypes.Structure):
    _fields_ = [("fn", ctypes.c_int32), ("col", ctypes.c_int32),
                ("is_f64", ctypes.c_int32), ("_pad", ctypes.c_int32)]


class _GbDesc(ctypes.Structure):
    _fields_ = [("t", ctypes.c_void_p),
                ("nkeys", ctypes.c_int32),
                ("key_cols", ctypes.c_int32 * GB_MAX_KEYS),
                ("naggs", ctypes.c_int32),
                ("aggs", _Agg * GB_MAX_AGGS),
                ("nquals", ctypes.c_int32),
                ("quals", _Filter * MAX_EXTRA_QUALS),
                ("max_groups", ctypes.c_int64)]


GB_MAX_FACTORS, GB_MAX_FQUALS, GB_MAX_OPERANDS = 3, 4, 8
FACTOR_COL, FACTOR_ONE_MINUS, FACTOR_ONE_PLUS = 0, 1, 2
_FACTOR_FORMS = {"": FACTOR_COL, "1-": FACTOR_ONE_MINUS, "1+": FACTOR_ONE_PLUS}


class _Factor(ctypes.Structure):
    _fields_ = [("col", ctypes.c_int32), ("form", ctypes.c_int32)]


class _Expr(ctypes.Structure):
    _fields_ = [("nfactors", ctypes.c_int32), ("_pad", ctypes.c_int32),
                ("f", _Factor * GB_MAX_FACTORS)]


class _FQual(ctypes.Structure):
    _fields_ = [("col", ctypes.c_int32), ("op", ctypes.c_int32),
                ("literal", ctypes.c_double)]


class _GbExt(ctypes.Structure):
    _fields_ = [("nexprs", ctypes.c_int32), ("nfquals", ctypes.c_int32),
                ("exprs", _Expr * GB_MAX_AGGS),
                ("agg_expr", ctypes.c_int32 * GB_MAX_AGGS),
                ("fquals", _FQual * GB_MAX_FQUALS)]


GBJ_MAX_JOINS = 2


class _GbJoin(ctypes.Structure):
    _fields_ = [("dim", ctypes.c_void_p),
                ("fact_col", ctypes.c_int32), ("dim_key_col", ctypes.c_int32),
                ("nquals", ctypes.c_int32), ("_pad", ctypes.c_int32),
                ("quals", _Filter * MAX_EXTRA_QUALS)]


class _GbjExt(ctypes.Structure):
    _fields_ = [("njoins", ctypes.c_int32), ("_pad", ctypes.c_int32),
                ("joins", _GbJoin * GBJ_MAX_JOINS),
                ("key_side", ctypes.c_int32 * GB_MAX_KEYS),
                ("agg_side", ctypes.c_int32 * GB_MAX_AGGS)]


class _GbjStats(ctypes.Structure):
    _fields_ = [("ms_build", ctypes.c_double), ("ms_kernel", ctypes.c_double),
                ("rows_in", ctypes.c_int64), ("rows_probed", ctypes.c_int64),
                ("rows_pass", ctypes.c_int64), ("rows_lds", ctypes.c_int64),
                ("rows_global", ctypes.c_int64), ("groups", ctypes.c_int64),
                ("dim_rows", ctypes.c_int64 * GBJ_MAX_JOINS)]


class DimCol:
    """A group key, or a column aggregate's column, read from the matched row
    of joins[j]'s dimension table (Context.groupby_join): DimCol(j, col)."""

    def __init__(self, j, col):
        self.j, self.col = j, col

    def __repr__(self):
        return f"DimCol({self.j}, {self.col})"


class _GbResult(ctypes.Structure):
    _fields_ = [("ngroups", ctypes.c_int64),
                ("nkeys", ctypes.c_int32), ("naggs", ctypes.c_int32),
                ("keys", ctypes.c_void_p), ("key_null", ctypes.c_void_p),
                ("aggs", ctypes.c_void_p), ("agg_null", ctypes.c_void_p)]


class _GbdStats(ctypes.Structure):
    _fields_ = [("ms_kernel", ctypes.c_double),
                ("rows_in", ctypes.c_int64), ("rows_pass", ctypes.c_int64),
                ("rows_lds", ctypes.c_int64), ("rows_global", ctypes.c_int64),
                ("groups", ctypes.c_int64)]


class _TblLayout(ctypes.Structure):
    _fields_ = [("key_width", ctypes.c_int32), ("interpolated", ctypes.c_int32),
                ("slots", ctypes.c_uint64), ("kmin", ctypes.c_int64),
                ("scale", ctypes.c_double), ("slot_kmin", ctypes.c_uint64),
                ("slot_kmax", ctypes.c_uint64)]


_OPS = {"<": 0, ">": 1, "==": 2, "!=": 3, "<=": 4, ">=": 5}
_DIM_JOINS = {"semi": 0, "anti": 1, "anti_notin": 2}

# numpy mirrors of the Motion wire rows (gx_ord_row, gx_qual_row_abi)
ORD_ROW_DTYPE = np.dtype([("okey", np.int64), ("ocust", np.int64),
                          ("odate", np.int32), ("oprio", np.int32)])
QUAL_ROW_DTYPE = np.dtype([("okey", np.int64), ("odate", np.int32),
                           ("oprio", np.int32)])


def _opcode(op):                # symbol, or a raw gx_filter op code
    return op if isinstance(op, int) else _OPS[op]


class _Q3Desc(ctypes.Structure):
    _fields_ = [("dim", ctypes.c_void_p), ("dim_key_col", ctypes.c_int32),
                ("dim_filter", _Filter),
                ("mid", ctypes.c_void_p), ("mid_key_col", ctypes.c_int32),
                ("mid_fk_col", ctypes.c_int32), ("mid_attr1_col", ctypes.c_int32),
                ("mid_attr2_col", ctypes.c_int32), ("mid_filter", _Filter),
                ("fact", ctypes.c_void_p), ("fact_key_col", ctypes.c_int32),
                ("fact_a_col", ctypes.c_int32), ("fact_b_col", ctypes.c_int32),
                ("fact_filter", _Filter),
                ("dim_text", ctypes.c_char * 64),
                ("dim_text_len", ctypes.c_int32),
                ("dim_extra", _Filter * 4), ("mid_extra", _Filter * 4),
                ("fact_extra", _Filter * 4),
                ("n_dim_extra", ctypes.c_int32),
                ("n_mid_extra", ctypes.c_int32),
                ("n_fact_extra", ctypes.c_int32),
                ("dim_join", ctypes.c_int32),
                ("fact_join", ctypes.c_int32)]


class _ColDesc(ctypes.Structure):
    _fields_ = [("host_stream", ctypes.c_void_p),
                ("nbytes", ctypes.c_int64),
                ("width", ctypes.c_int32),
                ("nrows", ctypes.c_int64),
                ("blocksize", ctypes.c_int32),
                ("format", ctypes.c_int32),
                ("codec", ctypes.c_int32)]


def _load():
    if not os.path.exists(_SO):
        raise RuntimeError(
            f"HIP extension missing: {_SO}. Build it with "
            f"`python -c \"import __graft_entry__; __graft_entry__.build()\"` — "
            f"the GPU executor has no CPU fallback.")
    lib = ctypes.CDLL(_SO)
    lib.gx_last_error.restype = ctypes.c_char_p
    lib.gx_last_error.argtypes = [ctypes.c_void_p]
    lib.gx_version.restype = ctypes.c_char_p
    lib.gx_init.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int,
                            ctypes.POINTER(ctypes.c_void_p)]
    lib.gx_shutdown.argtypes = [ctypes.c_void_p]
    lib.gx_comm_unique_id.argtypes = [ctypes.c_char_p]
    lib.gx_comm_init.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    lib.gx_table_bind.argtypes = [ctypes.c_void_p, ctypes.POINTER(_ColDesc),
                                  ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    lib.gx_table_free.argtypes = [ctypes.c_void_p]
    lib.gx_table_nrows.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]
    lib.gx_table_logical_bytes.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    lib.gx_tpch_gen.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double,
                                ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]
    lib.gx_table_dump_stream.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_int, ctypes.c_void_p,
                                         ctypes.c_int64,
                                         ctypes.POINTER(ctypes.c_int64)]
    lib.gx_decode_column.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                     ctypes.c_void_p, ctypes.c_int64, ctypes.c_int]
    lib.gx_decode_column_nullable.restype = ctypes.c_int
    lib.gx_decode_column_nullable.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int]
    lib.gx_table_set_visimap.restype = ctypes.c_int
    lib.gx_table_set_visimap.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_int64]
    lib.gx_decode_column_varlena.restype = ctypes.c_int
    lib.gx_decode_column_varlena.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int]
    lib.gx_q1.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                          ctypes.POINTER(ctypes.c_double)]
    lib.gx_scan_filter.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int64,
                                   ctypes.POINTER(ctypes.c_int64),
                                   ctypes.POINTER(ctypes.c_double)]
    lib.gx_partition.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                 ctypes.c_int32, ctypes.c_void_p]
    lib.gx_groupby.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                               ctypes.c_int,
                               ctypes.POINTER(ctypes.POINTER(_KvGroup)),
                               ctypes.POINTER(ctypes.c_int64)]
    lib.gx_groupby_dist.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_int, ctypes.c_int,
                                    ctypes.POINTER(ctypes.POINTER(_KvGroup)),
                                    ctypes.POINTER(ctypes.c_int64),
                                    ctypes.POINTER(_GbStats)]
    lib.gx_test_gb_partial.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int64,
                                       ctypes.POINTER(ctypes.c_int64)]
    lib.gx_test_gb_combine.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int64,
                                       ctypes.POINTER(ctypes.POINTER(_KvGroup)),
                                       ctypes.POINTER(ctypes.c_int64)]
    lib.gx_partition_multi.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int32, ctypes.c_int64,
                                       ctypes.c_int32, ctypes.c_void_p]
    lib.gx_q3_prepare.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int32,
                                  ctypes.POINTER(ctypes.c_void_p)]
    lib.gx_q3_prepare_desc.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Q3Desc),
                                       ctypes.POINTER(ctypes.c_void_p)]
    lib.gx_q3_set_numeric.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.gx_q3_run.argtypes = [ctypes.c_void_p]
    lib.gx_q3_stats_get.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Stats)]
    lib.gx_q3_dim_mode.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    lib.gx_q3_table_mode.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    lib.gx_selftest_rank_eligible.restype = ctypes.c_int
    lib.gx_selftest_rank_eligible.argtypes = [ctypes.c_int64, ctypes.c_uint64,
                                              ctypes.c_uint64, ctypes.c_int]
    lib.gx_rank_scan_block_keys.restype = ctypes.c_int64
    lib.gx_rank_scan_block_keys.argtypes = []
    lib.gx_q3_orders_mode.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    lib.gx_q3_orders_stage_claims.argtypes = [ctypes.c_void_p,
                                              ctypes.POINTER(ctypes.c_int64),
                                              ctypes.POINTER(ctypes.c_int64),
                                              ctypes.POINTER(ctypes.c_int64)]
    lib.gx_q3_test_set_orders_grid.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    lib.gx_selftest_orders_staged.restype = ctypes.c_int
    lib.gx_selftest_orders_staged.argtypes = [ctypes.c_int64, ctypes.c_int64,
                                              ctypes.c_int]
    lib.gx_orders_stage_rule_k.restype = ctypes.c_int64
    lib.gx_orders_stage_rule_k.argtypes = []
    lib.gx_selftest_orders_stage_grid.restype = ctypes.c_int64
    lib.gx_selftest_orders_stage_grid.argtypes = [ctypes.c_int64, ctypes.c_int64]
    lib.gx_orders_stage_wave_records.restype = ctypes.c_int64
    lib.gx_orders_stage_wave_records.argtypes = []
    lib.gx_q3_result.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.POINTER(_Group)),
                                 ctypes.POINTER(ctypes.c_int64)]
    lib.gx_q3_topn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                               ctypes.POINTER(ctypes.c_int64)]
    lib.gx_q3_free.argtypes = [ctypes.c_void_p]
    lib.gx_free.argtypes = [ctypes.c_void_p]
    lib.gx_test_motion1.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                    ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    lib.gx_test_qual.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_int64, ctypes.c_int, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_int64,
                                 ctypes.POINTER(ctypes.c_int64)]
    lib.gx_test_q3_from_qual.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_int32,
                                         ctypes.POINTER(ctypes.POINTER(_Group)),
                                         ctypes.POINTER(ctypes.c_int64)]
    lib.gx_test_m1.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.POINTER(_Filter), ctypes.c_int,
                               ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                               ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    lib.gx_test_dim.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_int32, ctypes.c_int64,
                                ctypes.c_uint64, ctypes.c_void_p,
                                ctypes.POINTER(ctypes.c_int64),
                                ctypes.POINTER(ctypes.c_int32)]
    lib.gx_test_m2.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64,
                               ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                               ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
                               ctypes.POINTER(ctypes.c_int32)]
    lib.gx_test_m3.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                               ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                               ctypes.POINTER(ctypes.POINTER(_Group)),
                               ctypes.POINTER(ctypes.c_int64),
                               ctypes.POINTER(_TblLayout)]
    lib.gx_groupby_desc.argtypes = [ctypes.c_void_p, ctypes.POINTER(_GbDesc),
                                    ctypes.POINTER(_GbResult),
                                    ctypes.POINTER(_GbdStats)]
    lib.gx_test_groupby_desc.argtypes = [ctypes.c_void_p,
                                         ctypes.POINTER(_GbDesc), ctypes.c_int,
                                         ctypes.c_int,
                                         ctypes.POINTER(_GbResult),
                                         ctypes.POINTER(_GbdStats)]
    lib.gx_groupby_desc_dist.argtypes = [ctypes.c_void_p, ctypes.POINTER(_GbDesc),
                                         ctypes.POINTER(_GbResult),
                                         ctypes.POINTER(_GbStats)]
    lib.gx_groupby_expr.argtypes = [ctypes.c_void_p, ctypes.POINTER(_GbDesc),
                                    ctypes.POINTER(_GbExt),
                                    ctypes.POINTER(_GbResult),
                                    ctypes.POINTER(_GbdStats)]
    lib.gx_test_groupby_expr.argtypes = [ctypes.c_void_p,
                                         ctypes.POINTER(_GbDesc),
                                         ctypes.POINTER(_GbExt), ctypes.c_int,
                                         ctypes.c_int,
                                         ctypes.POINTER(_GbResult),
                                         ctypes.POINTER(_GbdStats)]
    lib.gx_groupby_expr_dist.argtypes = [ctypes.c_void_p, ctypes.POINTER(_GbDesc),
                                         ctypes.POINTER(_GbExt),
                                         ctypes.POINTER(_GbResult),
                                         ctypes.POINTER(_GbStats)]
    lib.gx_groupby_join.argtypes = [ctypes.c_void_p, ctypes.POINTER(_GbDesc),
                                    ctypes.POINTER(_GbjExt),
                                    ctypes.POINTER(_GbExt),
                                    ctypes.POINTER(_GbResult),
                                    ctypes.POINTER(_GbjStats)]
    lib.gx_test_groupby_join.argtypes = [ctypes.c_void_p,
                                         ctypes.POINTER(_GbDesc),
                                         ctypes.POINTER(_GbjExt),
                                         ctypes.POINTER(_GbExt), ctypes.c_int,
                                         ctypes.c_int,
                                         ctypes.POINTER(_GbResult),
                                         ctypes.POINTER(_GbjStats)]
    lib.gx_groupby_join_dist.argtypes = [ctypes.c_void_p, ctypes.POINTER(_GbDesc),
                                         ctypes.POINTER(_GbjExt),
                                         ctypes.POINTER(_GbExt),
                                         ctypes.POINTER(_GbResult),
                                         ctypes.POINTER(_GbStats)]
    lib.gx_test_gbj_partial.argtypes = [ctypes.c_void_p, ctypes.POINTER(_GbDesc),
                                        ctypes.POINTER(_GbjExt), ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_int64,
                                        ctypes.POINTER(ctypes.c_int64)]
    lib.gx_selftest_gbj_join.restype = ctypes.c_int64
    lib.gx_selftest_gbj_join.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.c_void_p,
                                         ctypes.POINTER(ctypes.c_int64)]
    lib.gx_selftest_gbj_slots.restype = ctypes.c_int64
    lib.gx_selftest_gbj_slots.argtypes = [ctypes.c_void_p, ctypes.c_int64,
                                          ctypes.c_int64, ctypes.c_void_p]
    lib.gx_selftest_expr_eval.restype = ctypes.c_int
    lib.gx_selftest_expr_eval.argtypes = [ctypes.POINTER(_Expr), ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_int64,
                                          ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_void_p]
    lib.gx_selftest_fqual.restype = ctypes.c_int
    lib.gx_selftest_fqual.argtypes = [ctypes.c_int, ctypes.c_double,
                                      ctypes.c_double]
    lib.gx_gbd_wire_stride.restype = ctypes.c_int64
    lib.gx_gbd_wire_stride.argtypes = [ctypes.POINTER(_GbDesc)]
    lib.gx_test_gbd_partial.argtypes = [ctypes.c_void_p, ctypes.POINTER(_GbDesc),
                                        ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.POINTER(ctypes.c_int64)]
    lib.gx_test_gbd_combine.argtypes = [ctypes.c_void_p, ctypes.POINTER(_GbDesc),
                                        ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_int, ctypes.POINTER(_GbResult)]
    lib.gx_selftest_gbd_route.restype = ctypes.c_int
    lib.gx_selftest_gbd_route.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_int,
                                          ctypes.c_int64, ctypes.c_int,
                                          ctypes.c_void_p]
    lib.gx_gb_result_free.restype = None
    lib.gx_gb_result_free.argtypes = [ctypes.POINTER(_GbResult)]
    lib.gx_gb_lds_groups.restype = ctypes.c_int32
    lib.gx_gb_lds_groups.argtypes = [ctypes.c_int]
    lib.gx_selftest_gb_sort.restype = ctypes.c_int
    lib.gx_selftest_gb_sort.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_int64, ctypes.c_int,
                                        ctypes.c_void_p]
    lib.gx_selftest_motion_layout.restype = ctypes.c_int
    lib.gx_selftest_motion_layout.argtypes = [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
        ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
        ctypes.POINTER(_TblLayout)]
    lib.gx_test_topn.argtypes = [ctypes.c_void_p] * 7 + [
        ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
        ctypes.POINTER(ctypes.c_int64)]
    lib.gx_selftest_topn_merge.restype = ctypes.c_int
    lib.gx_selftest_topn_merge.argtypes = [ctypes.c_void_p] * 7 + [
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
        ctypes.POINTER(ctypes.c_int64)]
    lib.gx_selftest_unmatched_bound.restype = ctypes.c_uint64
    lib.gx_selftest_unmatched_bound.argtypes = [ctypes.c_int64, ctypes.c_uint64,
                                                ctypes.c_uint64]
    lib.gx_selftest_rle_block_class.restype = ctypes.c_int64
    lib.gx_selftest_rle_block_class.argtypes = [ctypes.c_void_p, ctypes.c_int64,
                                                ctypes.c_void_p, ctypes.c_int64]
    return lib


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


def _layout_dict(lay):
    return {f: getattr(lay, f) for f, _ in lay._fields_}


def motion_exchange_layout(cnts_all, seg):
    """The Motion path's send/receive bookkeeping (host only, no GPU):
    cnts_all is the all-gathered n×n count matrix, row r = rank r's
    per-destination counts.  Returns (scnt, soff, rcnt, roff) of rank seg as
    uint64 arrays; the offsets have n + 1 entries, the last the total."""
    c = np.ascontiguousarray(cnts_all, np.uint64)
    n = c.shape[0]
    assert c.shape == (n, n)
    scnt, rcnt = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    soff, roff = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    rc = lib().gx_selftest_motion_layout(
        c.ctypes.data, n, seg, scnt.ctypes.data, soff.ctypes.data,
        rcnt.ctypes.data, roff.ctypes.data, 0, 0, 0, 1, 300, None)
    if rc != 0:
        raise ValueError(f"gx_selftest_motion_layout: bad arguments ({rc})")
    return scnt, soff, rcnt, roff


def motion_table_layout(qual, kmin, kmax, nsegs, tf_pct=300):
    """The Motion path's join-table layout for qual received keys spanning
    [kmin, kmax] (host only, no GPU): gx_test_tbl_layout as a dict."""
    lay = _TblLayout()
    rc = lib().gx_selftest_motion_layout(None, 0, 0, None, None, None, None,
                                         qual, kmin, kmax, nsegs, tf_pct,
                                         ctypes.byref(lay))
    if rc != 0:
        raise ValueError(f"gx_selftest_motion_layout: bad arguments ({rc})")
    return _layout_dict(lay)


def unmatched_bound(nrows, lmin, lmax):
    """Sizing's bound on the LEFT-OUTER unmatched groups of a fact key column
    of nrows rows whose keys span [lmin, lmax] as unsigned 64-bit words (host
    only, no GPU)."""
    return int(lib().gx_selftest_unmatched_bound(
        int(nrows), int(lmin) & (2**64 - 1), int(lmax) & (2**64 - 1)))


def rank_eligible(qual, kmin, kmax, enabled=True):
    """Sizing's rule for the rank form of the Q3 join/agg table: qual
    qualifying mid rows whose keys span [kmin, kmax] as unsigned 64-bit words
    (host only, no GPU)."""
    return bool(lib().gx_selftest_rank_eligible(
        int(qual), int(kmin) & (2**64 - 1), int(kmax) & (2**64 - 1),
        1 if enabled else 0))


def rank_scan_block_keys():
    """Keys one block of the rank table's prefix-popcount scan covers."""
    return int(lib().gx_rank_scan_block_keys())


def orders_staged(qual, nrows, env=None):
    """The rank-form orders stage's form rule: True = staged, False =
    two-pass, for qual qualifying of nrows mid rows.  env is the value of
    GX_ORDERS_STAGED (0 or 1 forces a form, None = unset).  Host only."""
    return bool(lib().gx_selftest_orders_staged(
        int(qual), int(nrows), -1 if env is None else int(env)))


def orders_stage_k():
    """K of that rule: staged iff qual * K <= nrows."""
    return int(lib().gx_orders_stage_rule_k())


def orders_stage_grid(qual, nrows):
    """Blocks of the staged form's filter grid for those counts (host only)."""
    return int(lib().gx_selftest_orders_stage_grid(int(qual), int(nrows)))


def orders_stage_wave_records():
    """Records of one wave's LDS segment in the staged filter kernel."""
    return int(lib().gx_orders_stage_wave_records())


def gb_lds_groups(naggs):
    """Groups one workgroup's LDS table of the descriptor GROUP BY holds for
    a call with naggs aggregates (host only, no GPU)."""
    return int(lib().gx_gb_lds_groups(naggs))


def gb_sort(keys, key_null):
    """The result order of the descriptor GROUP BY (host only, no GPU): the
    permutation that sorts (n, nkeys) keys / key_null lexicographically by
    column, ascending, NULLS LAST per column, stable."""
    keys = np.ascontiguousarray(keys, np.int64)
    key_null = np.ascontiguousarray(key_null, np.uint8)
    assert keys.ndim == 2 and keys.shape == key_null.shape
    n, nkeys = keys.shape
    perm = np.zeros(n, np.int64)
    rc = lib().gx_selftest_gb_sort(keys.ctypes.data, key_null.ctypes.data, n,
                                   nkeys, perm.ctypes.data)
    if rc != 0:
        raise ValueError(f"gx_selftest_gb_sort: bad arguments ({rc})")
    return perm


def _gb_desc(table, keys, aggs, quals, max_groups):
    """gx_gb_desc from the Python argument shapes; table None leaves t NULL"""
    d = _GbDesc()
    d.t = None if table is None else table._t
    d.nkeys = len(keys)
    for i, c in enumerate(keys[:GB_MAX_KEYS]):
        d.key_cols[i] = c
    d.naggs = len(aggs)
    for i, spec in enumerate(aggs[:GB_MAX_AGGS]):
        fn, col = spec[0], spec[1]
        d.aggs[i] = _Agg(fn if isinstance(fn, int) else _AGG_FNS[fn],
                         -1 if col is None else col,
                         1 if len(spec) > 2 and spec[2] else 0, 0)
    d.nquals = len(quals)
    for i, (col, op, lit) in enumerate(quals[:MAX_EXTRA_QUALS]):
        d.quals[i] = _Filter(col, _opcode(op), int(lit))
    d.max_groups = max_groups
    return d


def _factor(f):
    """one factor: a column index, or (form, col) with form '1-' / '1+' / ''
    or a raw gx_factor_form code"""
    if isinstance(f, (tuple, list)):
        form, col = f
        return _Factor(col, form if isinstance(form, int) else _FACTOR_FORMS[form])
    return _Factor(f, FACTOR_COL)


def _expr(factors):
    """gx_expr from a list of factors; the count goes through unclipped so
    that the library's own range check answers"""
    e = _Expr()
    e.nfactors = len(factors)
    for i, f in enumerate(factors[:GB_MAX_FACTORS]):
        e.f[i] = _factor(f)
    return e


def _gb_expr_desc(table, keys, aggs, quals, fquals, max_groups):
    """(gx_gb_desc, gx_gb_ext, aggs as groupby_desc specs) from the
    groupby_expr argument shapes: an aggregate whose col is a list of factors
    becomes an expression aggregate (one gx_expr per distinct factor list)"""
    ext = _GbExt()
    plain, exprs = [], []
    for j in range(GB_MAX_AGGS):
        ext.agg_expr[j] = -1
    for j, spec in enumerate(aggs):
        if isinstance(spec[1], (list, tuple)):
            fac = [tuple(f) if isinstance(f, (list, tuple)) else f for f in spec[1]]
            if fac not in exprs:
                exprs.append(fac)
            if j < GB_MAX_AGGS:
                ext.agg_expr[j] = exprs.index(fac)
            # float8 values; COUNT(expr) stays the int64 count
            plain.append((spec[0], -1, spec[0] not in ("count", AGG_COUNT)))
        else:
            plain.append(tuple(spec))
    ext.nexprs = len(exprs)
    for e, fac in enumerate(exprs[:GB_MAX_AGGS]):
        ext.exprs[e] = _expr(fac)
    ext.nfquals = len(fquals)
    for q, (col, op, lit) in enumerate(fquals[:GB_MAX_FQUALS]):
        ext.fquals[q] = _FQual(col, _opcode(op), float(lit))
    return _gb_desc(table, keys, plain, quals, max_groups), ext, plain


def _gbj_desc(table, keys, aggs, joins, quals, fquals, max_groups):
    """(gx_gb_desc, gx_gbj_ext, gx_gb_ext, aggs as groupby_desc specs) from the
    groupby_join argument shapes: a DimCol key or aggregate column sets its
    side to the join's dimension; counts go through unclipped so that the
    library's own range checks answer"""
    jext = _GbjExt()
    kcols, specs = [], []
    for k, c in enumerate(keys):
        if isinstance(c, DimCol):
            if k < GB_MAX_KEYS:
                jext.key_side[k] = c.j + 1
            c = c.col
        kcols.append(c)
    for j, spec in enumerate(aggs):
        if isinstance(spec[1], DimCol):
            if j < GB_MAX_AGGS:
                jext.agg_side[j] = spec[1].j + 1
            spec = (spec[0], spec[1].col) + tuple(spec[2:])
        specs.append(tuple(spec))
    jext.njoins = len(joins)
    for j, jn in enumerate(joins[:GBJ_MAX_JOINS]):
        dim, fact_col, dim_key_col = jn[:3]
        jq = list(jn[3]) if len(jn) > 3 else []
        jext.joins[j].dim = None if dim is None else dim._t
        jext.joins[j].fact_col = fact_col
        jext.joins[j].dim_key_col = dim_key_col
        jext.joins[j].nquals = len(jq)
        for q, (col, op, lit) in enumerate(jq[:MAX_EXTRA_QUALS]):
            jext.joins[j].quals[q] = _Filter(col, _opcode(op), int(lit))
    d, ext, plain = _gb_expr_desc(table, kcols, specs, quals, fquals, max_groups)
    return d, jext, ext, plain


def selftest_gbj_join(dim_keys, fact_keys, dim_null=None, fact_null=None):
    """The join table of the descriptor GROUP BY over a join, restated on the
    host through the hash, slot and compare functions the kernels call (no
    GPU): a serial build over dim_keys (dim_null marks NULL keys, never
    inserted) and one probe per fact key.  Returns (rows, None), rows[i] the
    matched dimension row or -1, or (None, key) for a duplicated key."""
    dk = np.ascontiguousarray(dim_keys, np.int64)
    fk = np.ascontiguousarray(fact_keys, np.int64)
    dn = None if dim_null is None else np.ascontiguousarray(dim_null, np.uint8)
    fn = None if fact_null is None else np.ascontiguousarray(fact_null, np.uint8)
    assert dn is None or dn.shape == dk.shape
    assert fn is None or fn.shape == fk.shape
    out = np.full(len(fk), -2, np.int64)
    dup = ctypes.c_int64()
    rc = lib().gx_selftest_gbj_join(
        dk.ctypes.data if len(dk) else None, None if dn is None else dn.ctypes.data,
        len(dk), fk.ctypes.data if len(fk) else None,
        None if fn is None else fn.ctypes.data, len(fk),
        out.ctypes.data if len(fk) else None, ctypes.byref(dup))
    if rc < 0:
        raise ValueError(f"gx_selftest_gbj_join: bad arguments ({rc})")
    return (None, dup.value) if rc == 1 else (out, None)


def selftest_gbj_slots(keys, ndim):
    """(home slot of every key, slot count) of the join table of a dimension
    of ndim rows (host only, no GPU)."""
    k = np.ascontiguousarray(keys, np.int64)
    out = np.zeros(len(k), np.uint32)
    n = lib().gx_selftest_gbj_slots(k.ctypes.data if len(k) else None, len(k),
                                    ndim, out.ctypes.data if len(k) else None)
    if n < 0:
        raise ValueError(f"gx_selftest_gbj_slots: bad arguments ({n})")
    return out, int(n)


def selftest_expr_eval(factors, vals, isnull=None):
    """The value of one expression over the rows of vals (n, ncols) float64
    through the functions the scan kernel calls (host only, no GPU):
    (values, nulls).  factors as in Context.groupby_expr."""
    vals = np.ascontiguousarray(vals, np.float64)
    n, ncols = vals.shape
    nl = None
    if isnull is not None:
        nl = np.ascontiguousarray(isnull, np.uint8)
        assert nl.shape == vals.shape
    out, out_null = np.zeros(n, np.float64), np.zeros(n, np.uint8)
    e = _expr(list(factors))
    rc = lib().gx_selftest_expr_eval(ctypes.byref(e), vals.ctypes.data,
                                     None if nl is None else nl.ctypes.data,
                                     n, ncols, out.ctypes.data,
                                     out_null.ctypes.data)
    if rc != 0:
        raise ValueError(f"gx_selftest_expr_eval: bad arguments ({rc})")
    return out, out_null.astype(np.bool_)


def selftest_fqual(op, x, literal):
    """`x op literal` under float8_cmp_internal as the scan kernel evaluates
    a float8 qual (host only, no GPU): 1 pass, 0 fail, -1 for a bad op."""
    return int(lib().gx_selftest_fqual(_opcode(op), float(x), float(literal)))


def gbd_wire_stride(keys, aggs):
    """Bytes of one wire row of the two-stage descriptor GROUP BY for these
    keys and aggregates (gx_gbd_wire_stride; host only, no GPU), or -1."""
    d = _gb_desc(None, list(keys), list(aggs), [], 0)
    return int(lib().gx_gbd_wire_stride(ctypes.byref(d)))


def gbd_wire_dtype(keys, aggs):
    """numpy mirror of that wire row: keys (nkeys int64, 0 where NULL),
    key_null (nkeys uint8), _pad (zero bytes up to 8), acc (the state words,
    opaque).  keys / key_null / _pad are absent for a plain aggregate."""
    stride = gbd_wire_stride(keys, aggs)
    if stride < 0:
        raise ValueError("gx_gbd_wire_stride: bad descriptor")
    nk = len(keys)
    head = 8 * nk + (8 if nk else 0)
    fields = []
    if nk:
        fields = [("keys", np.int64, (nk,)), ("key_null", np.uint8, (nk,)),
                  ("_pad", np.uint8, (8 - nk,))]
    fields.append(("acc", np.uint64, ((stride - head) // 8,)))
    dt = np.dtype(fields)
    assert dt.itemsize == stride
    return dt


def gbd_route(keys, key_null, widths, nsegs):
    """Owner segment of every (n, nkeys) key row under the two-stage
    descriptor GROUP BY's routing (host only, no GPU): widths[k] is the byte
    width of key column k."""
    keys = np.ascontiguousarray(keys, np.int64)
    key_null = np.ascontiguousarray(key_null, np.uint8)
    widths = np.ascontiguousarray(widths, np.int32)
    assert keys.ndim == 2 and keys.shape == key_null.shape
    n, nkeys = keys.shape
    assert len(widths) == nkeys
    out = np.zeros(n, np.int32)
    rc = lib().gx_selftest_gbd_route(keys.ctypes.data, key_null.ctypes.data,
                                     widths.ctypes.data, nkeys, n, nsegs,
                                     out.ctypes.data)
    if rc != 0:
        raise ValueError(f"gx_selftest_gbd_route: bad arguments ({rc})")
    return out


RLEBLK_UNFUSED, RLEBLK_NOBITMAP, RLEBLK_VARINT, RLEBLK_FIXED2 = 0, 1, 2, 3


def rle_block_classes(stream):
    """How bind routes each block of a format-1 int64 stream for the fused RLE
    fact-key probe (host only, no GPU): an int32 array of RLEBLK_* values, one
    per block.  One RLEBLK_UNFUSED block sends the column to materialize."""
    arr = np.frombuffer(stream, np.uint8)
    n = lib().gx_selftest_rle_block_class(arr.ctypes.data, len(arr), None, 0)
    if n < 0:
        raise ValueError("gx_selftest_rle_block_class: bad stream")
    out = np.zeros(n, np.int32)
    lib().gx_selftest_rle_block_class(arr.ctypes.data, len(arr),
                                      out.ctypes.data, n)
    return out


def _topn_soa(okey, odate, oprio, rev, cnt, flags, numeric):
    okey = np.ascontiguousarray(okey, np.int64)
    n = len(okey)
    rev = np.ascontiguousarray(rev, np.int64 if numeric else np.float64)
    arrs = [okey, np.ascontiguousarray(odate, np.int32),
            np.ascontiguousarray(oprio, np.int32), rev,
            np.ascontiguousarray(cnt, np.int64),
            None if flags is None else np.ascontiguousarray(flags, np.uint8)]
    assert all(a is None or len(a) == n for a in arrs)
    return n, arrs


def topn_merge(cidx, okey, odate, oprio, rev, cnt, flags, topn=10,
               numeric=False):
    """The host merge of the top-N stage over candidate arrays (host only, no
    GPU): cidx < 0 marks an empty candidate; rev is int64 numerators when
    numeric.  Returns the selected rows as a Q3_GROUP_DTYPE array."""
    n, arrs = _topn_soa(okey, odate, oprio, rev, cnt, flags, numeric)
    cidx = np.ascontiguousarray(cidx, np.int64)
    assert len(cidx) == n and arrs[5] is not None
    out = np.zeros(max(topn, 1), Q3_GROUP_DTYPE)
    m = ctypes.c_int64()
    rc = lib().gx_selftest_topn_merge(
        cidx.ctypes.data, *[a.ctypes.data for a in arrs], n,
        1 if numeric else 0, topn, out.ctypes.data, ctypes.byref(m))
    if rc != 0:
        raise ValueError(f"gx_selftest_topn_merge: bad arguments ({rc})")
    return out[:m.value]


class Context:
    def __init__(self, device=0, seg=0, nsegs=1):
        self._lib = lib()
        self._h = ctypes.c_void_p()
        self._chk(self._lib.gx_init(device, seg, nsegs, ctypes.byref(self._h)), None)
        self.seg, self.nsegs = seg, nsegs

    def _chk(self, st, h="self"):
        if st != 0:
            handle = self._h if h == "self" else h
            msg = self._lib.gx_last_error(handle)
            raise GxError(st, (msg or b"").decode())

    def comm_unique_id(self):
        buf = ctypes.create_string_buffer(128)
        self._chk(self._lib.gx_comm_unique_id(buf), None)
        return buf.raw

    def comm_init(self, uid: bytes):
        assert len(uid) == 128
        self._chk(self._lib.gx_comm_init(self._h, uid))

    def tpch_gen(self, which, sf, seed=42):
        t = ctypes.c_void_p()
        self._chk(self._lib.gx_tpch_gen(self._h, which, sf, seed, ctypes.byref(t)))
        return Table(self, t)

    def bind(self, streams):
        """streams: list of (bytes, width, nrows[, format[, codec[,
        blocksize]]]) AOCS column streams; format 0 = Orig fixed, 1 =
        Dense/RLE; blocksize = the AO blocksize the stream was written
        with (default 32768)."""
        descs = (_ColDesc * len(streams))()
        keep = []
        for i, spec in enumerate(streams):
            data, width, nrows = spec[:3]
            arr = np.frombuffer(data, np.uint8)
            keep.append(arr)
            descs[i].host_stream = arr.ctypes.data
            descs[i].nbytes = len(arr)
            descs[i].width = width
            descs[i].nrows = nrows
            descs[i].blocksize = spec[5] if len(spec) > 5 else 32768
            descs[i].format = spec[3] if len(spec) > 3 else 0
            descs[i].codec = spec[4] if len(spec) > 4 else 0
        t = ctypes.c_void_p()
        self._chk(self._lib.gx_table_bind(self._h, descs, len(streams), ctypes.byref(t)))
        tb = Table(self, t)
        tb._col_nbytes = [len(s[0]) for s in streams]
        return tb

    def partition(self, keys, nsegs):
        keys = np.ascontiguousarray(keys, np.int64)
        out = np.zeros(len(keys), np.int32)
        self._chk(self._lib.gx_partition(self._h, keys.ctypes.data, len(keys),
                                         nsegs, out.ctypes.data))
        return out

    def partition_multi(self, vals, types, nsegs, isnull=None):
        """Multi-column distribution-key routing (cdbhash rotate-combine);
        vals (n, nkeys) int64; types[k] 0 = int8, 1 = int4/date."""
        vals = np.ascontiguousarray(vals, np.int64)
        n, nkeys = vals.shape
        types = np.ascontiguousarray(types, np.int32)
        nul_ptr = None
        if isnull is not None:
            nul = np.ascontiguousarray(isnull, np.uint8)
            assert nul.shape == vals.shape
            nul_ptr = nul.ctypes.data
        out = np.zeros(n, np.int32)
        self._chk(self._lib.gx_partition_multi(
            self._h, vals.ctypes.data, nul_ptr, types.ctypes.data,
            nkeys, n, nsegs, out.ctypes.data))
        return out

    def groupby(self, table, key_col, val_col):
        """GROUP BY key_col with COUNT(*)/SUM(val_col); NULL keys form one
        group (returned last, key_is_null True)."""
        gp = ctypes.POINTER(_KvGroup)()
        n = ctypes.c_int64()
        self._chk(self._lib.gx_groupby(self._h, table._t, key_col, val_col,
                                       ctypes.byref(gp), ctypes.byref(n)))
        n = n.value
        res = {"key": np.array([gp[i].key for i in range(n)], np.int64),
               "key_is_null": np.array([gp[i].key_is_null for i in range(n)],
                                       np.bool_),
               "sum": np.array([gp[i].sum for i in range(n)], np.float64),
               "count": np.array([gp[i].count for i in range(n)], np.int64)}
        self._lib.gx_free(gp)
        return res

    def _kv_result(self, gp, n):
        """gx_kv_group array -> the groupby dict shape; frees gp."""
        raw = ctypes.string_at(gp, n * KV_GROUP_DTYPE.itemsize) if n else b""
        self._lib.gx_free(gp)
        g = np.frombuffer(raw, KV_GROUP_DTYPE)
        return {"key": g["key"].copy(),
                "key_is_null": g["key_is_null"].astype(np.bool_),
                "sum": g["sum"].copy(), "count": g["count"].copy()}

    def groupby_dist(self, table, key_col, val_col, stats=False):
        """Two-stage GROUP BY across all segments of this context (partial
        agg, hash Motion of the partial groups by key, combine agg): returns
        the groups THIS segment owns, in the same dict shape as groupby();
        with stats=True returns (groups, gx_gb_stats as a dict)."""
        gp = ctypes.POINTER(_KvGroup)()
        n = ctypes.c_int64()
        st = _GbStats()
        self._chk(self._lib.gx_groupby_dist(self._h, table._t, key_col, val_col,
                                            ctypes.byref(gp), ctypes.byref(n),
                                            ctypes.byref(st)))
        res = self._kv_result(gp, n.value)
        if stats:
            return res, {f: getattr(st, f) for f, _ in st._fields_}
        return res

    def _gb_desc(self, table, keys, aggs, quals, max_groups):
        return _gb_desc(table, keys, aggs, quals, max_groups)

    def _gb_result(self, res, aggs):
        """gx_gb_result -> numpy; frees the native arrays."""
        n, nk, na = res.ngroups, res.nkeys, res.naggs

        def grab(ptr, count, dtype):
            if not count:
                return np.zeros(0, dtype)
            raw = ctypes.string_at(ptr, count * np.dtype(dtype).itemsize)
            return np.frombuffer(raw, dtype).copy()
        keys = grab(res.keys, n * nk, np.int64).reshape(n, nk)
        key_null = grab(res.key_null, n * nk, np.uint8).reshape(n, nk)
        words = grab(res.aggs, n * na, np.uint64).reshape(n, na)
        agg_null = grab(res.agg_null, n * na, np.uint8).reshape(n, na)
        self._lib.gx_gb_result_free(ctypes.byref(res))
        cols = [np.ascontiguousarray(words[:, j]).view(
                    np.float64 if len(spec) > 2 and spec[2] else np.int64)
                for j, spec in enumerate(aggs)]
        return {"ngroups": n, "keys": keys, "key_null": key_null.astype(np.bool_),
                "aggs": cols, "agg_null": agg_null.astype(np.bool_)}

    def groupby_desc(self, table, keys, aggs, quals=(), max_groups=0,
                     stats=False):
        """Descriptor-form GROUP BY (gx_groupby_desc).  keys: up to 4 integer
        column indexes (none = a plain aggregate); aggs: 1..8 tuples (fn,
        col[, is_f64]) with fn in 'count*', 'count', 'sum', 'min', 'max' (col
        None for 'count*'); quals: AND-ed (col, op, literal) triples.
        Returns a dict: keys (ngroups, nkeys) int64, key_null bool, aggs = one
        array per aggregate (float64 where is_f64, else int64), agg_null
        (ngroups, naggs) bool; groups sorted by key, NULLS LAST per column.
        With stats=True returns (result, gx_gbd_stats as a dict)."""
        return self._gb_run("gx_groupby_desc", _GbdStats(), table, keys, aggs,
                            quals, max_groups, stats)

    def test_groupby_desc(self, table, keys, aggs, quals=(), max_groups=0,
                          stats=False, grid=0, wide_rowid=False):
        """groupby_desc through the test seam: grid workgroups scan the input
        (0 = production) and wide_rowid forces the 8-byte slot word."""
        return self._gb_run("gx_test_groupby_desc", _GbdStats(), table, keys,
                            aggs, quals, max_groups, stats,
                            seam=(grid, 1 if wide_rowid else 0))

    def _gb_run(self, entry, st, table, keys, aggs, quals, max_groups, stats,
                fquals=None, joins=None, seam=(), ext=True, jext=None):
        """The one path behind groupby_desc / _expr / _join, their test seams
        and their _dist forms: build the descriptors the family takes (fquals
        None: gx_gb_desc alone; joins None: and gx_gb_ext; else and
        gx_gbj_ext), call `entry` with the seam's arguments before the result
        and the stats struct `st`, check, convert."""
        keys, aggs, quals = list(keys), list(aggs), list(quals)
        if fquals is None:
            d, descs, plain = self._gb_desc(table, keys, aggs, quals, max_groups), [], aggs
        else:
            if joins is None:
                d, x, plain = _gb_expr_desc(table, keys, aggs, quals, list(fquals),
                                            max_groups)
                descs = []
            else:
                d, jx, x, plain = _gbj_desc(table, keys, aggs, list(joins), quals,
                                            list(fquals), max_groups)
                if callable(jext):
                    jext(jx)
                descs = [ctypes.byref(jx)]
            if callable(ext):
                ext(x)
            descs.append(ctypes.byref(x) if ext is not None else None)
        res = _GbResult()
        self._chk(getattr(self._lib, entry)(
            self._h, ctypes.byref(d), *descs, *seam, ctypes.byref(res),
            ctypes.byref(st)))
        out = self._gb_result(res, plain)
        if not stats:
            return out
        sd = {f: getattr(st, f) for f, _ in st._fields_}
        if "dim_rows" in sd:
            sd["dim_rows"] = list(st.dim_rows)
        return out, sd

    def groupby_desc_dist(self, table, keys, aggs, quals=(), max_groups=0,
                          stats=False):
        """Two-stage descriptor GROUP BY across all segments of this context
        (gx_groupby_desc_dist): the arguments and the result shape of
        groupby_desc, holding the groups THIS segment owns; with stats=True
        returns (result, gx_gb_stats as a dict)."""
        return self._gb_run("gx_groupby_desc_dist", _GbStats(), table, keys,
                            aggs, quals, max_groups, stats)

    def groupby_expr(self, table, keys, aggs, quals=(), fquals=(),
                     max_groups=0, stats=False):
        """groupby_desc with float8 expression aggregates and float8 quals
        (gx_groupby_expr).  An aggregate's col may be a list of up to 3
        factors, each a float8 column index or ('1-', col) / ('1+', col):
        ("sum", [2, ("1-", 3), ("1+", 5)]) is SUM(c2 * (1 - c3) * (1 + c5));
        those aggregates come back as float64 arrays (COUNT as int64).  fquals: AND-ed (col,
        op, float) triples over float8 columns, compared in the reference's
        float8 order (NaN above +inf, -0 = +0).  Everything else as
        groupby_desc."""
        return self._gb_run("gx_groupby_expr", _GbdStats(), table, keys, aggs,
                            quals, max_groups, stats, fquals)

    def test_groupby_expr(self, table, keys, aggs, quals=(), fquals=(),
                          max_groups=0, stats=False, grid=0, wide_rowid=False,
                          ext=True):
        """groupby_expr through the test seam (grid, wide_rowid as for
        test_groupby_desc).  ext=None passes a NULL gx_gb_ext; a callable is
        given the filled gx_gb_ext mirror to alter before the call (raw
        counts, forms and indexes for the error paths)."""
        return self._gb_run("gx_test_groupby_expr", _GbdStats(), table, keys,
                            aggs, quals, max_groups, stats, fquals,
                            seam=(grid, 1 if wide_rowid else 0), ext=ext)

    def groupby_expr_dist(self, table, keys, aggs, quals=(), fquals=(),
                          max_groups=0, stats=False):
        """Two-stage groupby_expr across all segments of this context
        (gx_groupby_expr_dist): the groups THIS segment owns; with stats=True
        returns (result, gx_gb_stats as a dict)."""
        return self._gb_run("gx_groupby_expr_dist", _GbStats(), table, keys,
                            aggs, quals, max_groups, stats, fquals)

    def groupby_join(self, table, keys, aggs, joins, quals=(), fquals=(),
                     max_groups=0, stats=False):
        """groupby_expr over a join (gx_groupby_join): table is the fact side
        of up to 2 inner equi-joins, joins = [(dim_table, fact_col,
        dim_key_col[, quals])] with AND-ed (col, op, literal) quals over the
        dimension.  A key, or a column aggregate's col, may be DimCol(j, col):
        column col of joins[j]'s dimension at the matched row.  Dimension
        keys must be unique among the rows that take part; a fact row that
        misses any join is dropped.  Everything else, and the result, as
        groupby_expr; with stats=True returns (result, gx_gbj_stats as a
        dict, its dim_rows a list)."""
        return self._gb_run("gx_groupby_join", _GbjStats(), table, keys, aggs,
                            quals, max_groups, stats, fquals, joins)

    def test_groupby_join(self, table, keys, aggs, joins, quals=(), fquals=(),
                          max_groups=0, stats=False, grid=0, wide_rowid=False,
                          jext=None):
        """groupby_join through the test seam (grid, wide_rowid as for
        test_groupby_desc).  A callable jext is given the filled gx_gbj_ext
        mirror to alter before the call (raw counts, sides and indexes for
        the error paths)."""
        return self._gb_run("gx_test_groupby_join", _GbjStats(), table, keys,
                            aggs, quals, max_groups, stats, fquals, joins,
                            seam=(grid, 1 if wide_rowid else 0), jext=jext)

    def groupby_join_dist(self, table, keys, aggs, joins, quals=(), fquals=(),
                          max_groups=0, stats=False):
        """Two-stage groupby_join across all segments of this context
        (gx_groupby_join_dist): every segment holds each dimension complete;
        returns the groups THIS segment owns; with stats=True returns
        (result, gx_gb_stats as a dict)."""
        return self._gb_run("gx_groupby_join_dist", _GbStats(), table, keys,
                            aggs, quals, max_groups, stats, fquals, joins)

    def test_gbj_partial(self, table, keys, aggs, joins, nsegs, quals=(),
                         max_groups=0):
        """Partial agg + partition kernels of groupby_join_dist on one GPU:
        (counts, rows) as test_gbd_partial."""
        d, jext, _, plain = _gbj_desc(table, list(keys), list(aggs), list(joins),
                                      list(quals), [], max_groups)
        cap = max(table.nrows, 1)
        counts = np.zeros(max(nsegs, 1), np.int64)
        rows = np.zeros(cap, gbd_wire_dtype([0] * len(keys), plain))
        total = ctypes.c_int64()
        self._chk(self._lib.gx_test_gbj_partial(
            self._h, ctypes.byref(d), ctypes.byref(jext), nsegs,
            counts.ctypes.data, rows.ctypes.data, cap, ctypes.byref(total)))
        return counts[:nsegs], rows[:total.value]

    def selftest_gbj_join(self, dim_keys, fact_keys, dim_null=None,
                          fact_null=None):
        """The module's selftest_gbj_join (host only; needs no GPU work)."""
        return selftest_gbj_join(dim_keys, fact_keys, dim_null, fact_null)

    def test_gbd_partial(self, table, keys, aggs, nsegs, quals=(),
                         max_groups=0):
        """Partial agg + partition kernels of groupby_desc_dist on one GPU:
        returns (counts, rows), rows a gbd_wire_dtype array packed by
        destination."""
        keys, aggs, quals = list(keys), list(aggs), list(quals)
        d = self._gb_desc(table, keys, aggs, quals, max_groups)
        cap = max(table.nrows, 1)
        counts = np.zeros(max(nsegs, 1), np.int64)
        rows = np.zeros(cap, gbd_wire_dtype(keys, aggs))
        total = ctypes.c_int64()
        self._chk(self._lib.gx_test_gbd_partial(
            self._h, ctypes.byref(d), nsegs, counts.ctypes.data,
            rows.ctypes.data, cap, ctypes.byref(total)))
        return counts[:nsegs], rows[:total.value]

    def test_gbd_combine(self, rows, keys, aggs, max_groups=0,
                         wide_rowid=False):
        """Combine stage of groupby_desc_dist over wire rows (a
        gbd_wire_dtype array): the groupby_desc result shape.  keys only
        counts: the rows carry the key values."""
        keys, aggs = list(keys), list(aggs)
        rows = np.ascontiguousarray(rows, gbd_wire_dtype(keys, aggs))
        d = self._gb_desc(None, keys, aggs, [], max_groups)
        res = _GbResult()
        self._chk(self._lib.gx_test_gbd_combine(
            self._h, ctypes.byref(d), rows.ctypes.data if len(rows) else None,
            len(rows), 1 if wide_rowid else 0, ctypes.byref(res)))
        return self._gb_result(res, aggs)

    def test_gb_partial(self, table, key_col, val_col, nsegs):
        """Partial agg + partition kernels on one GPU: returns (counts,
        rows) — rows is a KV_GROUP_DTYPE array grouped by destination."""
        cap = table.nrows + 1              # distinct keys + the NULL group
        counts = np.zeros(nsegs, np.int64)
        rows = np.zeros(cap, KV_GROUP_DTYPE)
        total = ctypes.c_int64()
        self._chk(self._lib.gx_test_gb_partial(
            self._h, table._t, key_col, val_col, nsegs, counts.ctypes.data,
            rows.ctypes.data, cap, ctypes.byref(total)))
        return counts, rows[:total.value]

    def test_gb_combine(self, rows):
        """Combine agg over partial rows (KV_GROUP_DTYPE array)."""
        rows = np.ascontiguousarray(rows, KV_GROUP_DTYPE)
        gp = ctypes.POINTER(_KvGroup)()
        n = ctypes.c_int64()
        self._chk(self._lib.gx_test_gb_combine(
            self._h, rows.ctypes.data if len(rows) else None, len(rows),
            ctypes.byref(gp), ctypes.byref(n)))
        return self._kv_result(gp, n.value)

    def test_motion1(self, orders, nsegs, cutoff=CUTOFF_19950315):
        """Run the Motion-1 partition kernels; returns (counts, rows dict)."""
        cap = orders.nrows
        counts = np.zeros(nsegs, np.int64)
        rows = np.zeros(cap, dtype=[("okey", np.int64), ("ocust", np.int64),
                                    ("odate", np.int32), ("oprio", np.int32)])
        total = ctypes.c_int64()
        self._chk(self._lib.gx_test_motion1(self._h, orders._t, cutoff, nsegs,
                                            counts.ctypes.data, rows.ctypes.data,
                                            cap, ctypes.byref(total)))
        return counts, rows[:total.value]

    QUAL_DTYPE = np.dtype([("okey", np.int64), ("odate", np.int32),
                           ("oprio", np.int32)])

    def test_qual(self, customer, rows, nsegs, ):
        """Motion stage 2 on one GPU: semijoin received orders rows against
        this segment's customer set, route qualifiers by o_orderkey."""
        counts = np.zeros(nsegs, np.int64)
        out = np.zeros(len(rows), self.QUAL_DTYPE)
        total = ctypes.c_int64()
        self._chk(self._lib.gx_test_qual(self._h, customer._t, rows.ctypes.data,
                                         len(rows), nsegs, counts.ctypes.data,
                                         out.ctypes.data, len(rows),
                                         ctypes.byref(total)))
        return counts, out[:total.value]

    def test_q3_from_qual(self, qual_rows, lineitem, cutoff=CUTOFF_19950315):
        """Motion stage 3 on one GPU: build table from qual rows, probe the
        local lineitem, return groups sorted by key."""
        gp = ctypes.POINTER(_Group)()
        n = ctypes.c_int64()
        self._chk(self._lib.gx_test_q3_from_qual(self._h, qual_rows.ctypes.data,
                                                 len(qual_rows), lineitem._t,
                                                 cutoff, ctypes.byref(gp),
                                                 ctypes.byref(n)))
        n = n.value
        res = {"l_orderkey": np.array([gp[i].l_orderkey for i in range(n)], np.int64),
               "o_orderdate": np.array([gp[i].o_orderdate for i in range(n)], np.int32),
               "o_shippriority": np.array([gp[i].o_shippriority for i in range(n)], np.int32),
               "revenue": np.array([gp[i].revenue for i in range(n)], np.float64),
               "nitems": np.array([gp[i].nitems for i in range(n)], np.int64),
               "key_is_null": np.array([gp[i].key_is_null for i in range(n)],
                                       np.bool_),
               "attrs_null": np.array([gp[i].attrs_null for i in range(n)],
                                      np.bool_)}
        self._lib.gx_free(gp)
        return res

    # ---- Motion stages of the nsegs>1 Q3 path, one rank at a time ----

    def test_m1(self, orders, mid_filter, nsegs, dim_join="semi",
                bloom_all=None):
        """Motion 1 of one rank: mid_filter = (col, op, literal) on orders
        (visimap honoured); bloom_all = (nsegs, bwords) uint64 array of every
        rank's dim bloom, or None.  Returns (counts, ORD_ROW_DTYPE rows packed
        by destination)."""
        col, op, lit = mid_filter
        f = _Filter(col, _opcode(op), int(lit))
        cap = orders.nrows
        counts = np.zeros(nsegs, np.int64)
        rows = np.zeros(cap, ORD_ROW_DTYPE)
        total = ctypes.c_int64()
        bptr, bwords = None, 0
        if bloom_all is not None:
            bloom_all = np.ascontiguousarray(bloom_all, np.uint64)
            assert bloom_all.ndim == 2 and bloom_all.shape[0] == nsegs
            bptr, bwords = bloom_all.ctypes.data, bloom_all.shape[1]
        self._chk(self._lib.gx_test_m1(
            self._h, orders._t, ctypes.byref(f), nsegs, _DIM_JOINS[dim_join],
            bptr, bwords, counts.ctypes.data, rows.ctypes.data, cap,
            ctypes.byref(total)))
        return counts, rows[:total.value]

    def test_dim(self, customer, dim_filter, bwords):
        """Dim side of one rank: dim_filter = (op, literal) on the int8
        column.  Returns (bloom words uint64[bwords], selected rows, set
        width production picks)."""
        op, lit = dim_filter
        bloom = np.zeros(bwords, np.uint64)
        nsel = ctypes.c_int64()
        width = ctypes.c_int32()
        self._chk(self._lib.gx_test_dim(
            self._h, customer._t, _opcode(op), int(lit), bwords,
            bloom.ctypes.data, ctypes.byref(nsel), ctypes.byref(width)))
        return bloom, nsel.value, width.value

    def test_m2(self, customer, dim_filter, rows, nsegs, dim_join="semi",
                bwords=0):
        """Motion 2 of one rank: received ORD_ROW_DTYPE rows against this
        rank's dim set.  Returns (counts, QUAL_ROW_DTYPE rows packed by
        destination, set width)."""
        op, lit = dim_filter
        rows = np.ascontiguousarray(rows, ORD_ROW_DTYPE)
        n = len(rows)
        counts = np.zeros(nsegs, np.int64)
        out = np.zeros(n, QUAL_ROW_DTYPE)
        total = ctypes.c_int64()
        width = ctypes.c_int32()
        self._chk(self._lib.gx_test_m2(
            self._h, customer._t, _opcode(op), int(lit), bwords,
            rows.ctypes.data if n else None, n, _DIM_JOINS[dim_join], nsegs,
            counts.ctypes.data, out.ctypes.data if n else None, n,
            ctypes.byref(total), ctypes.byref(width)))
        return counts, out[:total.value], width.value

    def test_m3(self, qual_rows, lineitem, fact_filter):
        """Motion 3 of one rank (nsegs of this context): table from received
        QUAL_ROW_DTYPE rows, probe + aggregate lineitem under fact_filter =
        (op, literal) on shipdate, visimap honoured.  Returns (groups dict
        sorted by key, table layout dict)."""
        op, lit = fact_filter
        qual_rows = np.ascontiguousarray(qual_rows, QUAL_ROW_DTYPE)
        n = len(qual_rows)
        gp = ctypes.POINTER(_Group)()
        ng = ctypes.c_int64()
        lay = _TblLayout()
        self._chk(self._lib.gx_test_m3(
            self._h, qual_rows.ctypes.data if n else None, n, lineitem._t,
            _opcode(op), int(lit), ctypes.byref(gp), ctypes.byref(ng),
            ctypes.byref(lay)))
        m = ng.value
        raw = ctypes.string_at(gp, m * ctypes.sizeof(_Group)) if m else b""
        self._lib.gx_free(gp)
        g = np.frombuffer(raw, Q3_GROUP_DTYPE)
        res = {"l_orderkey": g["l_orderkey"].copy(),
               "o_orderdate": g["o_orderdate"].copy(),
               "o_shippriority": g["o_shippriority"].copy(),
               "revenue": g["revenue"].copy(),
               "revenue_num": g["revenue_num"].copy(),
               "nitems": g["nitems"].copy(),
               "key_is_null": g["key_is_null"].copy(),
               "attrs_null": g["attrs_null"].copy(),
               "_pad": g["_pad"].copy()}
        return res, _layout_dict(lay)

    def test_topn(self, okey, odate, oprio, rev, cnt, flags=None, topn=10,
                  numeric=False, out=None):
        """The top-N stage of gx_q3_topn over host SoA arrays of groups (rev:
        float64, or int64 numerators when numeric; flags optional).  Returns
        the selected rows as a Q3_GROUP_DTYPE array; `out` (a Q3_GROUP_DTYPE
        array of >= 10 rows) replaces the internal output buffer."""
        n, arrs = _topn_soa(okey, odate, oprio, rev, cnt, flags, numeric)
        if out is None:
            out = np.zeros(10, Q3_GROUP_DTYPE)
        assert out.dtype == Q3_GROUP_DTYPE and len(out) >= 10
        m = ctypes.c_int64(-1)
        self._chk(self._lib.gx_test_topn(
            self._h, *[None if a is None else a.ctypes.data for a in arrs], n,
            1 if numeric else 0, topn, out.ctypes.data, ctypes.byref(m)))
        return out[:m.value]

    def q1(self, lineitem_q1, cutoff):
        """TPC-H Q1 core: returns dict of 6-group arrays + kernel ms."""
        counts = np.zeros(6, np.int64)
        sp = np.zeros(6, np.float64)
        sr = np.zeros(6, np.float64)
        ms = ctypes.c_double()
        self._chk(self._lib.gx_q1(self._h, lineitem_q1._t, cutoff,
                                  counts.ctypes.data, sp.ctypes.data,
                                  sr.ctypes.data, ctypes.byref(ms)))
        return {"count": counts, "sum_price": sp, "sum_revenue": sr,
                "avg_price": np.divide(sp, counts, out=np.zeros(6),
                                       where=counts > 0),
                "ms": ms.value}

    def q3_desc(self, desc_dict):
        """Plan-descriptor Q3 slice: column roles + filter
        {col, op, literal} triples chosen by the caller."""
        ops = {"<": 0, ">": 1, "==": 2, "!=": 3, "<=": 4, ">=": 5}

        def opcode(op):         # symbol, or a raw gx_filter op code
            return op if isinstance(op, int) else ops[op]
        d = _Q3Desc()
        for role in ("dim", "mid", "fact"):
            setattr(d, role, desc_dict[role]._t)
        d.dim_key_col = desc_dict["dim_key_col"]
        d.mid_key_col = desc_dict["mid_key_col"]
        d.mid_fk_col = desc_dict["mid_fk_col"]
        d.mid_attr1_col = desc_dict["mid_attr1_col"]
        d.mid_attr2_col = desc_dict["mid_attr2_col"]
        d.fact_key_col = desc_dict["fact_key_col"]
        d.fact_a_col = desc_dict["fact_a_col"]
        d.fact_b_col = desc_dict["fact_b_col"]
        for role in ("dim_filter", "mid_filter", "fact_filter"):
            col, op, lit = desc_dict[role]
            if isinstance(lit, (str, bytes)):
                # TEXT predicate (texteq on a varlena column, dim only)
                assert role == "dim_filter" and op == "=="
                blit = lit.encode() if isinstance(lit, str) else lit
                d.dim_text = blit
                d.dim_text_len = len(blit)
                setattr(d, role, _Filter(col, opcode(op), 0))
            else:
                setattr(d, role, _Filter(col, opcode(op), int(lit)))
        # AND-ed extra qual lists (execScan.c:241 semantics)
        for role, arr, cnt in (("dim_extra", d.dim_extra, "n_dim_extra"),
                               ("mid_extra", d.mid_extra, "n_mid_extra"),
                               ("fact_extra", d.fact_extra, "n_fact_extra")):
            quals = desc_dict.get(role, [])
            assert len(quals) <= 4
            for i, (col, op, lit) in enumerate(quals):
                arr[i] = _Filter(col, opcode(op), int(lit))
            setattr(d, cnt, len(quals))
        d.dim_join = {"semi": 0, "anti": 1, "anti_notin": 2}[
            desc_dict.get("dim_join", "semi")]
        d.fact_join = {"inner": 0, "left_outer": 1}[
            desc_dict.get("fact_join", "inner")]
        q = ctypes.c_void_p()
        self._chk(self._lib.gx_q3_prepare_desc(self._h, ctypes.byref(d),
                                               ctypes.byref(q)))
        return Q3(self, q,
                  tables=(desc_dict["dim"], desc_dict["mid"], desc_dict["fact"]))

    def q3(self, cust, orders, lineitem, cutoff=CUTOFF_19950315, numeric=False):
        q = ctypes.c_void_p()
        self._chk(self._lib.gx_q3_prepare(self._h, cust._t, orders._t, lineitem._t,
                                          cutoff, ctypes.byref(q)))
        if numeric:
            st = self._lib.gx_q3_set_numeric(q, 1)
            if st != 0:
                self._lib.gx_q3_free(q)
            self._chk(st)
        return Q3(self, q, tables=(cust, orders, lineitem))

    def close(self):
        if self._h:
            self._lib.gx_shutdown(self._h)
            self._h = None


class Table:
    def __init__(self, ctx, t):
        self.ctx = ctx
        self._t = t

    @property
    def nrows(self):
        n = ctypes.c_int64()
        self.ctx._chk(self.ctx._lib.gx_table_nrows(self._t, ctypes.byref(n)))
        return n.value

    @property
    def logical_bytes(self):
        b = ctypes.c_double()
        self.ctx._chk(self.ctx._lib.gx_table_logical_bytes(self._t, ctypes.byref(b)))
        return b.value

    def scan_filter(self, col, op, literal):
        """SeqScan+qual count; op in {'<','>','==','!=','<=','>='} or a raw
        gx_filter op code; returns (count, ms)."""
        opc = op if isinstance(op, int) else \
            {"<": 0, ">": 1, "==": 2, "!=": 3, "<=": 4, ">=": 5}[op]
        n = ctypes.c_int64()
        ms = ctypes.c_double()
        self.ctx._chk(self.ctx._lib.gx_scan_filter(self.ctx._h, self._t, col, opc,
                                                   literal, ctypes.byref(n),
                                                   ctypes.byref(ms)))
        return n.value, ms.value

    def dump_stream(self, col):
        """Raw AOCS stream bytes of a column (byte-level parity tests)."""
        cap = self.nrows * 16 + (1 << 22)
        buf = np.zeros(cap, np.uint8)
        n = ctypes.c_int64()
        self.ctx._chk(self.ctx._lib.gx_table_dump_stream(
            self.ctx._h, self._t, col, buf.ctypes.data, cap, ctypes.byref(n)))
        return buf[:n.value].tobytes()

    def decode_column(self, col, dtype, verify=True):
        n = self.nrows
        out = np.zeros(n, dtype)
        self.ctx._chk(self.ctx._lib.gx_decode_column(
            self.ctx._h, self._t, col, out.ctypes.data, n, 1 if verify else 0))
        return out

    def _coldesc_nbytes(self, col):
        return self._col_nbytes[col] if hasattr(self, "_col_nbytes") else 1 << 22

    def decode_column_varlena(self, col, verify=True):
        """Decode a varlena (text) directory column -> list of bytes|None.
        RLE streams expand past the stream size; grow the buffer on demand."""
        n = self.nrows
        cap = self._coldesc_nbytes(col) + 16
        while True:
            offsets = np.zeros(n + 1, np.int64)
            payload = np.zeros(cap, np.uint8)
            validity = np.zeros(max(n, 1), np.uint8)
            try:
                self.ctx._chk(self.ctx._lib.gx_decode_column_varlena(
                    self.ctx._h, self._t, col, offsets.ctypes.data,
                    payload.ctypes.data, cap, validity.ctypes.data,
                    1 if verify else 0))
            except GxError as e:
                if "too small" in str(e):
                    cap *= 4
                    continue
                raise
            break
        return [None if not validity[i]
                else payload[offsets[i]:offsets[i + 1]].tobytes()
                for i in range(n)]

    def decode_column_nullable(self, col, dtype, verify=True):
        """Decode a (possibly NULL-bearing) block-directory column.
        Returns (values, validity) — null datums decode as zero."""
        n = self.nrows
        out = np.zeros(n, dtype)
        validity = np.zeros(n, np.uint8)
        self.ctx._chk(self.ctx._lib.gx_decode_column_nullable(
            self.ctx._h, self._t, col, out.ctypes.data, validity.ctypes.data,
            n, 1 if verify else 0))
        return out, validity

    def free(self):
        if self._t:
            self.ctx._lib.gx_table_free(self._t)
            self._t = None

    def set_visimap(self, deleted):
        """Attach an AO visimap: `deleted` is a per-row bool array
        (True = tuple hidden/deleted); None clears.  Set before ctx.q3()."""
        if deleted is None:
            self.ctx._chk(self.ctx._lib.gx_table_set_visimap(
                self.ctx._h, self._t, None, 0))
            self._vmap = None
            return
        deleted = np.ascontiguousarray(deleted, np.uint8)
        assert len(deleted) == self.nrows
        bits = np.packbits(deleted, bitorder="little")
        self.ctx._chk(self.ctx._lib.gx_table_set_visimap(
            self.ctx._h, self._t, bits.ctypes.data, len(deleted)))
        self._vmap = bits        # keep the host copy alive until replaced

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass            # interpreter teardown / context already gone


class Q3:
    def __init__(self, ctx, q, tables=()):
        self.ctx = ctx
        self._q = q
        self._tables = tables    # keep the Tables alive: the native Q3
                                 # holds raw device pointers into them

    def run(self):
        self.ctx._chk(self.ctx._lib.gx_q3_run(self._q))
        return self

    def stats(self):
        s = _Stats()
        self.ctx._chk(self.ctx._lib.gx_q3_stats_get(self._q, ctypes.byref(s)))
        return {f: getattr(s, f) for f, _ in s._fields_}

    def dim_mode(self):
        """Dim membership form the last run read: 0 = bloom + hash set,
        1 = exact bitmap (dense keys, local path)."""
        m = ctypes.c_int()
        self.ctx._chk(self.ctx._lib.gx_q3_dim_mode(self._q, ctypes.byref(m)))
        return m.value

    def set_numeric(self, on=True):
        """Switch numeric(15,2) mode (scaled-int64 measures) for later runs."""
        self.ctx._chk(self.ctx._lib.gx_q3_set_numeric(self._q, 1 if on else 0))
        return self

    def table_mode(self):
        """Join/agg table form the last run used: 0 = open-addressing hash
        table, 1 = rank table (dense mid keys, local f64 path)."""
        m = ctypes.c_int()
        self.ctx._chk(self.ctx._lib.gx_q3_table_mode(self._q, ctypes.byref(m)))
        return m.value

    def orders_mode(self):
        """Form the last run's rank-form orders stage took: 0 = two-pass
        (row mask, second walk), 1 = staged (compacted records)."""
        m = ctypes.c_int()
        self.ctx._chk(self.ctx._lib.gx_q3_orders_mode(self._q, ctypes.byref(m)))
        return m.value

    def orders_stage_claims(self):
        """(blocks, mid-loop flushes, records) of the last run's staged orders
        stage: its cursor claims number at most blocks + flushes, and they
        added up to `records` qualifying rows."""
        b, f, r = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self.ctx._chk(self.ctx._lib.gx_q3_orders_stage_claims(
            self._q, ctypes.byref(b), ctypes.byref(f), ctypes.byref(r)))
        return b.value, f.value, r.value

    def _test_set_orders_grid(self, blocks):
        """Test seam: grid of the staged filter kernel; 0 = production rule."""
        self.ctx._chk(self.ctx._lib.gx_q3_test_set_orders_grid(self._q, int(blocks)))
        return self

    def result(self):
        gp = ctypes.POINTER(_Group)()
        n = ctypes.c_int64()
        self.ctx._chk(self.ctx._lib.gx_q3_result(self._q, ctypes.byref(gp),
                                                 ctypes.byref(n)))
        n = n.value
        res = {"l_orderkey": np.array([gp[i].l_orderkey for i in range(n)], np.int64),
               "o_orderdate": np.array([gp[i].o_orderdate for i in range(n)], np.int32),
               "o_shippriority": np.array([gp[i].o_shippriority for i in range(n)], np.int32),
               "revenue": np.array([gp[i].revenue for i in range(n)], np.float64),
               "revenue_num": np.array([gp[i].revenue_num for i in range(n)], np.int64),
               "nitems": np.array([gp[i].nitems for i in range(n)], np.int64),
               "key_is_null": np.array([gp[i].key_is_null for i in range(n)],
                                       np.bool_),
               "attrs_null": np.array([gp[i].attrs_null for i in range(n)],
                                      np.bool_)}
        self.ctx._lib.gx_free(gp)
        return res

    def topn(self, n=10):
        out = (_Group * n)()
        m = ctypes.c_int64()
        self.ctx._chk(self.ctx._lib.gx_q3_topn(self._q, n, out, ctypes.byref(m)))
        m = m.value
        return {"l_orderkey": np.array([out[i].l_orderkey for i in range(m)], np.int64),
                "o_orderdate": np.array([out[i].o_orderdate for i in range(m)], np.int32),
                "o_shippriority": np.array([out[i].o_shippriority for i in range(m)], np.int32),
                "revenue": np.array([out[i].revenue for i in range(m)], np.float64),
                "revenue_num": np.array([out[i].revenue_num for i in range(m)], np.int64),
                "nitems": np.array([out[i].nitems for i in range(m)], np.int64),
                "key_is_null": np.array([out[i].key_is_null for i in range(m)],
                                        np.bool_),
                "attrs_null": np.array([out[i].attrs_null for i in range(m)],
                                       np.bool_)}

    def free(self):
        if self._q:
            self.ctx._lib.gx_q3_free(self._q)
            self._q = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

