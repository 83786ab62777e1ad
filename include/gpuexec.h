/*
 * gpuexec.h — C-ABI of libgpuexec.so, the MI355X-native executor for
 * Cloudberry's segment-local scan→hash-join→hash-agg pipeline + hash Motion.
 *
 * This is the drop-in boundary.  Each entry point names the
 * reference seam it replaces (paths under /root/reference):
 *
 *   gx_init / gx_shutdown      — per-QE executor state; what a CustomScan
 *                                extension's BeginCustomScan/EndCustomScan
 *                                (src/include/nodes/extensible.h:124-158,
 *                                executor/nodeCustom.c) would call once per
 *                                segment process.
 *   gx_comm_*                  — the MotionIPCLayer SetupInterconnect /
 *                                TeardownInterconnect pair (cdb/ml_ipc.h:36,
 *                                executor/execMain.c:535); RCCL communicator
 *                                is created once per process lifetime
 *                                (mirrors gang reuse, dispatcher/README.md).
 *   gx_table_bind              — scan target binding: the table-AM open path
 *                                aocs_beginscan (access/aocs/aocsam.c:542)
 *                                with per-column segment-file streams.
 *   gx_tpch_gen                — bench-harness substitute for on-disk data
 *                                (no network; synthetic).
 *   gx_decode_column           — aocs_getnext datum decode
 *                                (aocsam.c:1131-1259, datumstreamblock.c:
 *                                195-340) materialised column-at-a-time.
 *   gx_q3_prepare/run/result   — the QE slice ExecProcNode pull loop over
 *                                SeqScan→HashJoin→HashAgg (+ Motion sends at
 *                                nsegs>1): execMain.c:983, nodeHashjoin.c:252,
 *                                nodeAgg.c:2743, nodeMotion.c:1181.
 *   gx_partition (exposed for tests) — doSendTuple's evalHashKey +
 *                                cdbhashreduce routing (nodeMotion.c:1088,
 *                                cdbhash.c:253-285,530-541), bit-exact.
 *
 * Plain C, status-code returns, caller-owned opaque handles.  No torch
 * types; no exceptions across the boundary (the PG-side shim converts
 * non-zero status into ereport(ERROR)).  All calls are per-process
 * single-threaded, matching the QE execution model (one thread per segment;
 * HIP streams + RCCL run on that thread).
 */
#ifndef GPUEXEC_H
#define GPUEXEC_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gx_status {
    GX_OK = 0,
    GX_ERR_HIP = 1,            /* HIP runtime failure (see gx_last_error) */
    GX_ERR_RCCL = 2,           /* RCCL failure */
    GX_ERR_INVALID = 3,        /* bad argument / malformed stream */
    GX_ERR_CHECKSUM = 4,       /* AO block checksum mismatch */
    GX_ERR_OOM = 5,            /* device memory exhausted */
    GX_ERR_NOGPU = 6,          /* no usable device — callers must FAIL, not fall back */
    GX_ERR_STATE = 7           /* calls out of order */
} gx_status;

typedef struct gx_ctx gx_ctx;
typedef struct gx_table gx_table;
typedef struct gx_q3 gx_q3;

/* last error message for a context (or the global init error when ctx==NULL) */
const char *gx_last_error(const gx_ctx *ctx);
const char *gx_version(void);

/* ---- lifecycle ---- */
gx_status gx_init(int device_id, int seg_id, int nsegs, gx_ctx **out);
gx_status gx_shutdown(gx_ctx *ctx);

/* ---- interconnect (RCCL over xGMI; one rank per segment-GPU) ---- */
#define GX_UNIQUE_ID_BYTES 128
gx_status gx_comm_unique_id(unsigned char uid[GX_UNIQUE_ID_BYTES]); /* rank 0 */
gx_status gx_comm_init(gx_ctx *ctx, const unsigned char uid[GX_UNIQUE_ID_BYTES]);

/* ---- tables: AOCS per-column streams resident in HBM ---- */

typedef struct gx_coldesc {
    const void *host_stream;   /* AOCS stream bytes (appendonly=column,
                                  checksum=true) */
    int64_t     nbytes;
    int32_t     width;         /* fixed datum width: 1, 4 or 8 */
    int64_t     nrows;
    int32_t     blocksize;     /* AO blocksize the stream was written with */
    int32_t     format;        /* 0 = Orig (compresstype=none), 1 =
                                  Dense/Dense_Enhanced incl. RLE_TYPE/DELTA,
                                  Orig blocks allowed too (concatenated
                                  segment files).  As an inner join's Q3
                                  fact key, a NULL-free column of Dense
                                  blocks with at most 4096 physical datums
                                  and no DELTA is scanned in place by the
                                  fused RLE probe; any other block
                                  materializes the column at prepare
                                   */
    int32_t     codec;         /* bulk codec for compressedLength>0 blocks:
                                  0/1 = zlib, 2 = zstd (the pg_appendonly
                                  compresstype analog) */
} gx_coldesc;

/* Every column must carry the same nrows.  A format-0 stream is addressed in
 * O(1) afterwards, so bind walks its block headers on the host and returns
 * GX_ERR_INVALID unless they are small-content blocks of exactly
 * rows_per_block(width, blocksize) rows each (the last may be shorter), the
 * rows add up to nrows and the blocks to nbytes, and nrows == 0 exactly for
 * an empty stream.  Streams concatenated from several segment files have a
 * partial block in the middle: bind those as format 1. */
gx_status gx_table_bind(gx_ctx *ctx, const gx_coldesc *cols, int ncols,
                        gx_table **out);
gx_status gx_table_free(gx_table *t);
gx_status gx_table_nrows(const gx_table *t, int64_t *out);
/* logical uncompressed bytes of all columns = the reference's
 * totalBytesRead accounting base (cdb/cdbaocsam.h:283) */
gx_status gx_table_logical_bytes(const gx_table *t, double *out);

/* synthetic TPC-H-shaped tables generated AND AOCS-encoded on device
 * (deterministic; identical formulas to oracle/oracle.c datagen) */
typedef enum { GX_TPCH_CUSTOMER = 0, GX_TPCH_ORDERS = 1, GX_TPCH_LINEITEM = 2,
               GX_TPCH_LINEITEM_NUMERIC = 3, /* measures as scaled int64 */
               GX_TPCH_LINEITEM_RLEKEY = 4,  /* l_orderkey RLE-compressed */
               GX_TPCH_LINEITEM_Q1 = 5       /* Q1 cols: flag,status,price,disc,ship */ } gx_tpch_table;
gx_status gx_tpch_gen(gx_ctx *ctx, gx_tpch_table which, double sf,
                      uint64_t seed, gx_table **out);

/* copy a column's raw AOCS stream bytes back to the host (parity tests) */
gx_status gx_table_dump_stream(gx_ctx *ctx, const gx_table *t, int col,
                               void *host_out, int64_t cap_bytes,
                               int64_t *nbytes);

/* decode one column back to host values (parity testing / config-2 path);
 * verify_checksums runs the CRC32C pair per block on device */
gx_status gx_decode_column(gx_ctx *ctx, const gx_table *t, int col,
                           void *host_out, int64_t cap_rows,
                           int verify_checksums);

/* NULL-bearing columns (block-directory format only): validity gets one
 * byte per row, 1 = non-null; null datums decode as zero. */
gx_status gx_decode_column_nullable(gx_ctx *ctx, const gx_table *t, int col,
                                    void *host_out, uint8_t *host_validity,
                                    int64_t cap_rows, int verify_checksums);

/* Scan-time visibility map (AO visimap executor semantics,
 * cdbappendonlyvisimap.c:140-210): bitmap has one bit per logical row,
 * ON = tuple hidden (deleted); every scan/build/probe kernel skips
 * hidden rows.  bitmap=NULL clears.  Set before gx_q3_prepare. */
gx_status gx_table_set_visimap(gx_ctx *ctx, gx_table *t,
                               const uint8_t *bitmap, int64_t nbits);

/* Varlena (text) Orig columns (bind with width = -1, format = 1):
 * offsets[nrows+1] exclusive into payload; validity required when the
 * stream carries a NULL bitmap. */
gx_status gx_decode_column_varlena(gx_ctx *ctx, const gx_table *t, int col,
                                   int64_t *host_offsets, void *host_payload,
                                   int64_t payload_cap,
                                   uint8_t *host_validity,
                                   int verify_checksums);

/* TPC-H Q1 core (BASELINE config 4): GROUP BY returnflag,linestatus with
 * COUNT/SUM over a GX_TPCH_LINEITEM_Q1 table; AVG = sum/count (float8_avg).
 * The table must be five format-0 columns of widths [1, 1, 8, 8, 4]
 * (GX_ERR_INVALID otherwise). */
gx_status gx_q1(gx_ctx *ctx, const gx_table *t, int32_t cutoff,
                int64_t *counts6, double *sum_price6, double *sum_rev6,
                double *ms_out);

/* standalone columnar scan + filter count (the SeqScan+qual slice;
 * BASELINE config 2): op is a gx_filter op (0..5, below) vs an integer/date
 * literal of any int64 value, compared as the cross-type operator would
 * (see gx_filter); ms_out = kernel time from HIP events */
gx_status gx_scan_filter(gx_ctx *ctx, const gx_table *t, int col, int op,
                         int64_t literal, int64_t *count_out, double *ms_out);

/* bit-exact Motion routing of an i64 key column on device:
 * out[i] = jump_consistent_hash(cdbhash(hashint8(keys[i])), nsegs) */
gx_status gx_partition(gx_ctx *ctx, const int64_t *host_keys, int64_t n,
                       int32_t nsegs, int32_t *host_out);

/* multi-column distribution keys (cdbhash.c:189-247 rotate-combine loop):
 * vals/isnull row-major n×nkeys (each attribute widened to int64);
 * types[k]: 0 = int8 (hashint8), 1 = int4/int2/date (hashint4); a NULL
 * attribute contributes only the rotation.  isnull may be NULL. */
gx_status gx_partition_multi(gx_ctx *ctx, const int64_t *host_vals,
                             const uint8_t *host_isnull,
                             const int32_t *host_types, int32_t nkeys,
                             int64_t n, int32_t nsegs, int32_t *host_out);

/* ---- the Q3 pipeline (the judged QE slice) ---- */

typedef struct gx_q3_group {
    int64_t l_orderkey;
    int32_t o_orderdate;
    int32_t o_shippriority;
    double  revenue;           /* f64 mode: the SUM; numeric mode: num/1e4 */
    int64_t revenue_num;       /* numeric(15,2) mode: exact Σ price_c·(100−d),
                                  implied scale 1e-4 (0 in f64 mode) */
    int64_t nitems;
    /* appended r2 for LEFT OUTER fact joins (fact_join=1): unmatched fact
     * rows form groups with NULL mid attributes (attrs_null=1, date/prio
     * 0); NULL fact keys form ONE group (key_is_null=1, NULLs-equal
     * grouping) returned LAST.  Both 0 for inner joins. */
    uint8_t key_is_null;
    uint8_t attrs_null;
    uint8_t _pad[6];
} gx_q3_group;

typedef struct gx_q3_stats {
    /* per-stage device times, ms (HIP events on the executor stream) */
    double ms_cust_build;
    double ms_orders_build;
    double ms_probe_agg;       /* the dominant kernel */
    double ms_extract;
    double ms_motion;          /* partition+exchange (0 at nsegs==1) */
    double ms_total;           /* event span over the whole pipeline */
    int64_t cust_rows, ord_rows, li_rows;
    int64_t probe_hits, groups;
    double bytes_scanned;      /* logical uncompressed bytes (cdbaocsam.h:283) */
    /* Motion sub-phases (appended r2; 0 at nsegs==1) */
    double ms_motion_counts;   /* count all-gathers incl. their host syncs */
    double ms_motion_payload;  /* row payload send/recv (device events) */
} gx_q3_stats;

/* customer cols: [c_custkey i64, c_mktsegment i8]
 * orders   cols: [o_orderkey i64, o_custkey i64, o_orderdate i32, o_shippriority i32]
 * lineitem cols: [l_orderkey i64, l_extendedprice f64, l_discount f64, l_shipdate i32] */
gx_status gx_q3_prepare(gx_ctx *ctx, gx_table *customer, gx_table *orders,
                        gx_table *lineitem, int32_t cutoff_dateadt,
                        gx_q3 **out);

/* ---- plan-descriptor form (what PlanCustomPath lowering
 * fills; tagged structs, no expression trees yet).  Filter ops:
 * 0 '<', 1 '>', 2 '=', 3 '!=', 4 '<=', 5 '>='. ---- */
/* The literal is an int64 whatever the column's width, and the comparison
 * is the mathematically correct cross-type one (int48lt etc.): on an int8
 * column `v < 300` is always true and `v = 300` always false.  The kernels
 * compare in the column type, so the host folds <op, literal> first: an
 * out-of-range literal becomes v >= TYPE_MIN (always true) or v < TYPE_MIN
 * (always false); in-range pairs pass through.  An op outside 0..5 in a
 * primary filter or gx_scan_filter is GX_ERR_INVALID. */
typedef struct gx_filter {
    int32_t col;               /* column index in the role's table */
    int32_t op;
    int64_t literal;           /* integer/date literal (DateADT for dates) */
} gx_filter;

typedef struct gx_q3_desc {
    /* build side of the semijoin (reference: customer) */
    gx_table *dim;
    int32_t dim_key_col;       /* i64 join key */
    gx_filter dim_filter;      /* e.g. mktsegment = literal */
    /* middle table redistributed/joined on both keys (reference: orders) */
    gx_table *mid;
    int32_t mid_key_col;       /* i64 key joined to fact (o_orderkey) */
    int32_t mid_fk_col;        /* i64 key joined to dim  (o_custkey) */
    int32_t mid_attr1_col;     /* i32 carried into the group (o_orderdate) */
    int32_t mid_attr2_col;     /* i32 carried into the group (o_shippriority) */
    gx_filter mid_filter;      /* e.g. o_orderdate < literal */
    /* fact side (reference: lineitem); agg = SUM(a*(1-b)), COUNT(*) */
    gx_table *fact;
    int32_t fact_key_col;      /* i64 probe key (l_orderkey) */
    int32_t fact_a_col;        /* f64 (l_extendedprice) */
    int32_t fact_b_col;        /* f64 (l_discount) */
    gx_filter fact_filter;     /* e.g. l_shipdate > literal */
    /* optional TEXT dim predicate (texteq — the reference's actual Q3 qual
     * c_mktsegment = 'BUILDING'): when dim_text_len > 0, dim_filter.col
     * names a VARLENA directory column (width -1, format 1) and the
     * predicate is payload == dim_text with op '=='.  With rle_type
     * segments the comparison runs once per RUN. */
    char dim_text[64];
    int32_t dim_text_len;
    /* AND-ed qual lists (execScan.c:241 semantics over NOT NULL integer/date
     * columns: every qual must pass; widths 1/4/8, literals widened to i64).
     * Folded at prepare into a per-table row mask combined with the visimap,
     * so the per-step kernels see them through the existing visibility path. */
#define GX_MAX_EXTRA_QUALS 4
    gx_filter dim_extra[GX_MAX_EXTRA_QUALS];
    gx_filter mid_extra[GX_MAX_EXTRA_QUALS];
    gx_filter fact_extra[GX_MAX_EXTRA_QUALS];
    int32_t n_dim_extra, n_mid_extra, n_fact_extra;
    /* dim-join type (nodeHashjoin.c join variety on the dim semijoin):
     * 0 = JOIN_SEMI (IN / EXISTS — the Q3 shape)
     * 1 = JOIN_LASJ (anti, NOT EXISTS): mid rows pass when the fk is NOT
     *     in the dim set; a NULL fk never matches, so it PASSES
     *     (nodeHashjoin.c:652-659 left-anti semantics)
     * 2 = JOIN_LASJ_NOTIN (NOT IN): a NULL fk is rejected, and ANY NULL
     *     dim key passing the dim filter empties the whole result
     *     (nodeHashjoin.c:425,442 hs_hashkeys_null) */
    int32_t dim_join;
    /* fact-join type (the fact⋈mid join): 0 = inner (the Q3 shape);
     * 1 = LEFT OUTER (nodeHashjoin.c HJ_FILL_OUTER): fact rows passing
     *     their WHERE quals but matching no mid row form groups with NULL
     *     mid attrs; NULL fact keys (never equal under the strict op)
     *     also emit, all in ONE group (NULLs-equal grouping).  Requires a
     *     plain or materialized fact key (no fused-RLE) and f64 measures. */
    int32_t fact_join;
} gx_q3_desc;

/* Restrictions checked at sizing (first gx_q3_run):
 * - join keys must be >= 1: slot value 0 is the empty-slot sentinel (PG
 *   sequence-keyed tables start at 1); a key 0 on the build side returns
 *   GX_ERR_INVALID instead of silently dropping the row.
 * - LEFT OUTER (fact_join = 1), checked at prepare: the fact key column must
 *   hold neither a non-NULL 0 nor INT64_MIN in any stored row (filtered and
 *   visimap-hidden rows included).  The unmatched-group table keeps keys
 *   biased by 2^63, with 0 as its empty-slot mark (INT64_MIN would be
 *   dropped or inherit another key's sums) and 2^63 as the NULL-key group (a
 *   real 0 would be reported as key_is_null).  Both return GX_ERR_INVALID
 *   from gx_q3_prepare_desc with the key named in gx_last_error; NULL fact
 *   keys and every other int64 value, negative ones included, form their
 *   own groups.
 * - HBM budget: if the semijoin set / join table would exceed free HBM
 *   (override: GX_HBM_BUDGET_MB), sizing fails with GX_ERR_OOM and the
 *   required vs available GB in gx_last_error BEFORE any allocation — the
 *   reference spills to batches (nodeHashjoin.c:1355); this executor
 *   rejects, callers keep the reference CPU path for such plans. */
gx_status gx_q3_prepare_desc(gx_ctx *ctx, const gx_q3_desc *desc, gx_q3 **out);
/* numeric(15,2) mode: lineitem measures are scaled int64
 * (price cents, discount hundredths — GX_TPCH_LINEITEM_NUMERIC tables);
 * aggregation is integer → results BIT-EXACT vs the oracle. */
gx_status gx_q3_set_numeric(gx_q3 *q, int on);
gx_status gx_q3_run(gx_q3 *q);   /* one full pass; re-runnable (bench steps) */
gx_status gx_q3_stats_get(const gx_q3 *q, gx_q3_stats *out);
/* Form of the dim membership structure the LAST run's mid-table filter read:
 * 0 = bloom + hash set, 1 = exact bitmap.  Sizing picks the bitmap when the
 * qualifying dim keys are dense (max - min + 1 <= 64 * their count) and
 * GX_DIM_BITMAP is not 0; only the local (single-segment, no forced Motion)
 * path reads it.  GX_ERR_STATE before the first run. */
gx_status gx_q3_dim_mode(gx_q3 *q, int *mode);
/* Form of the join/agg table the LAST run used: 0 = open-addressing hash
 * table, 1 = rank table (one bit per mid key of [min, max] plus per-word
 * prefix popcounts; a key's rank indexes dense payload arrays).  Sizing allows
 * the rank form when the qualifying mid keys are dense (max - min + 1 <= 64 *
 * their row count, fewer than 2^32 rows) and GX_RANK_TABLE is not 0; a run
 * takes it on the local (single-segment, no forced Motion) path with f64
 * measures over a plain fact key, and the hash form otherwise.  GX_ERR_STATE
 * before the first run. */
gx_status gx_q3_table_mode(gx_q3 *q, int *mode);
/* Form the orders stage of the LAST run took when that run used the rank
 * table: 0 = two-pass (a per-row mask, then a second walk over the mid table
 * that re-reads the qualifying rows), 1 = staged (the filter pass compacts
 * {key, attr1, attr2} of the qualifying rows into 16-byte records and the
 * fill reads only those).  Staged is taken where at most one mid row in K
 * qualified at sizing (K: gx_orders_stage_rule_k); GX_ORDERS_STAGED=0 or =1
 * forces a form.  0 for a hash-form run.  GX_ERR_STATE before the first
 * run. */
gx_status gx_q3_orders_mode(gx_q3 *q, int *mode);
/* Cursor claims of the last run's staged orders stage: the blocks of its
 * filter grid (each ends with at most one claim) and the mid-loop flushes of
 * waves whose LDS segment filled up; and the records those claims added up
 * to (the run's qualifying mid rows; more than the staging capacity only if
 * the input changed after sizing).  Copies 16 bytes from the device.
 * GX_ERR_STATE unless the last run took the staged form. */
gx_status gx_q3_orders_stage_claims(gx_q3 *q, int64_t *blocks, int64_t *flushes,
                                    int64_t *records);
/* Test seam: grid (in blocks of 256 threads, at most 2^20) of the staged
 * form's filter kernel for later runs of q, same launches otherwise; 0
 * restores the production rule.  Small grids on small tables reach the
 * multi-iteration accumulation and the segment-overflow flush. */
gx_status gx_q3_test_set_orders_grid(gx_q3 *q, int64_t blocks);
/* groups of THIS segment, sorted by l_orderkey asc; caller frees with gx_free */
gx_status gx_q3_result(gx_q3 *q, gx_q3_group **out, int64_t *ngroups);
/* top-N of this segment's groups (Q3's ORDER BY revenue DESC, o_orderdate
 * LIMIT N; N ≤ 10) — the nodeSort/nodeLimit stage, device-selected.
 * Outer-join groups sort with NULL dates LAST (PG ASC NULLS LAST).  Any
 * int64 group key may come back, negative ones included; numeric mode orders
 * by the int64 numerators.  GX_ERR_STATE before the first run or for N
 * outside 1..10, with nothing written. */
gx_status gx_q3_topn(gx_q3 *q, int topn, gx_q3_group *out, int64_t *nout);
gx_status gx_q3_free(gx_q3 *q);

void gx_free(void *p);

/* ABI self-description for foreign mirrors (0 stats, 1 q3_group,
 * 2 kv_group, 3 q3_desc, 4 coldesc, 5 filter, 6 gb_stats,
 * 7 test_tbl_layout, 8 gb_desc, 9 gb_result, 10 agg, 11 gbd_stats,
 * 13 gb_ext, 14 expr, 15 fqual, 16 gb_join, 17 gbj_ext, 18 gbj_stats); -1
 * for unknown kinds.  Kind 12 is left
 * unassigned on purpose and stays -1: the suite pins it as an unknown kind. */
int64_t gx_abi_sizeof(int kind);

/* ---- standalone hash GROUP BY (nodeAgg.c:2288 hash strategy over one key;
 * grouping equality is NOT DISTINCT, execGrouping.c:436-495: all NULL keys
 * form ONE group, returned LAST with key_is_null=1).  COUNT(*) counts every
 * row; SUM(float8)'s transition is strict (float.c:769) and skips NULL
 * inputs.  key/val cols are i64/f64, Orig or Dense/RLE (nullable via
 * format-1 streams).  Key INT64_MIN is rejected (biased sentinel).  Groups
 * sorted by key asc; caller frees with gx_free. ---- */
typedef struct gx_kv_group {
    int64_t key;
    uint8_t key_is_null;
    uint8_t _pad[7];
    double  sum;
    int64_t count;
} gx_kv_group;
gx_status gx_groupby(gx_ctx *ctx, const gx_table *t, int key_col, int val_col,
                     gx_kv_group **out, int64_t *ngroups);

/* ---- two-stage GROUP BY through Motion: the plan the reference builds when
 * the group key is not the distribution key (cdbgroupingpaths.c:251) —
 * partial agg per segment, hash-redistribute Motion of the transition
 * states by group key, combine agg on the owning segment (nodeAgg.c:2305,
 * 2321: float8pl / int8pl as combine functions).  Routing is the bit-exact
 * Motion chain; a NULL key routes as cdbhash routes a NULL attribute.
 * Same grouping semantics, column formats and INT64_MIN restriction as the
 * one-stage call above. ---- */
typedef struct gx_gb_stats {
    double  ms_partial, ms_partition, ms_exchange, ms_combine; /* HIP events */
    int64_t rows_in, partial_groups, sent_rows, recv_rows, final_groups;
} gx_gb_stats;

/* GROUP BY key_col, COUNT(*), SUM(val_col) across all segments of ctx.
 * Returns the groups THIS segment owns (route(key) == seg), key asc,
 * NULL group last (on its owning segment only).  stats may be NULL.
 * nsegs == 1 without GX_FORCE_MOTION runs the one-stage plan (motion stats
 * zero); otherwise gx_comm_init must have been called (GX_ERR_STATE). */
gx_status gx_groupby_dist(gx_ctx *ctx, const gx_table *t, int key_col,
                          int val_col, gx_kv_group **out, int64_t *ngroups,
                          gx_gb_stats *stats);

/* ---- descriptor-form hash GROUP BY: what a planner lowers an Agg node over
 * a SeqScan to (nodeAgg.c:2288 hash strategy, execScan.c:161-263 qual scan).
 * Several integer key columns, a list of aggregates, AND-ed WHERE quals.
 * gx_groupby_desc runs the one-stage plan over this segment's rows;
 * gx_groupby_desc_dist below is the two-stage/Motion form of the same
 * descriptor.
 *
 * Keys: 0..GX_GB_MAX_KEYS integer columns of width 1, 2, 4 or 8, format 0 or
 *   format 1 (NULL bitmaps included; width 2 binds as format 1 only).
 *   Grouping is NOT DISTINCT per column (execGrouping.c:436-495): (NULL, 1)
 *   and (NULL, 2) are two groups, (NULL, 1) and (0, 1) are two groups.
 *   Every int64 value is a legal key, INT64_MIN and 0 included: a group is
 *   identified by a representative row, no key value is reserved.  Float
 *   key columns are not supported.
 * nkeys == 0: a plain aggregate (nodeAgg.c:2743 AGG_PLAIN): exactly one
 *   group, also over an empty or fully filtered input, where COUNT is 0 and
 *   every other aggregate NULL.  With nkeys > 0 an empty input gives zero
 *   groups (hash agg emits no row, nodeAgg.c:2288).
 * Aggregates (1..GX_GB_MAX_AGGS; `col` is ignored by COUNT(*)):
 *   COUNT(*) counts rows, COUNT(col) non-NULL inputs (int8inc /
 *   int8inc_any).  SUM, MIN and MAX are strict
 *   (nodeAgg.c:836 advance_transition_function skips NULL inputs) and NULL
 *   for a group without a non-NULL input (agg_null = 1, word 0).
 *   SUM over an integer column of width 1, 2 or 4 is int64 with plain
 *   two's-complement adds (int2_sum / int4_sum); SUM over
 *   float8 (is_f64 = 1) is float8pl (float.c:769), in the order the rows
 *   arrive, so the last bits may differ from a serial sum; SUM over a
 *   width-8 integer column is numeric in the reference and GX_ERR_INVALID
 *   here.  MIN and MAX take every integer width (int2larger ... int8smaller) and float8 in the reference's total order
 *   (float8_cmp_internal, float.c): every NaN is equal and greater
 *   than +inf; -0 and +0 compare equal and either may come back.  AVG is
 *   deliberately no function: divide SUM by COUNT(col), as gx_q1 documents.
 * Quals: AND-ed gx_filters over integer/date columns of width 1, 2, 4 or 8,
 *   each folded as gx_filter describes; a NULL qual input fails the row
 *   (execScan.c:241, ExecQual treats NULL as false).  The visimap is
 *   honoured.
 * max_groups: the planner's bound on the group count; sizes the hash table
 *   (0 = bound by nrows).  More groups than that is GX_ERR_INVALID.
 * Output: sorted on the host, lexicographic by key columns ascending, NULLS
 *   LAST per column (PG's default ASC).
 * GX_ERR_INVALID names the offending item in gx_last_error: a bad column
 *   index, width, fn or count; is_f64 on a column that is not 8 bytes wide;
 *   a qual op outside 0..5.  The HBM budget is checked before allocating
 *   (GX_ERR_OOM).  GX_GB_LDS=0 in the environment, read at call time, turns
 *   the workgroup-private LDS stage off; GX_GB_GIVEUP_ROWS (default 4096,
 *   0 = never) is the row count after which a workgroup whose LDS table
 *   mostly misses stops consulting it (DESIGN.md "Descriptor GROUP BY").
 * Known difference: a float8 SUM whose inputs are all -0.0 returns +0.0.
 * Not verified: tables of 2^32 - 1 rows or more (the 8-byte slot word is
 *   covered through gx_test_groupby_desc's wide_rowid only). ---- */
#define GX_GB_MAX_KEYS 4
#define GX_GB_MAX_AGGS 8
typedef enum { GX_AGG_COUNT_STAR = 0, GX_AGG_COUNT = 1, GX_AGG_SUM = 2,
               GX_AGG_MIN = 3, GX_AGG_MAX = 4 } gx_agg_fn;
typedef struct gx_agg { int32_t fn; int32_t col; int32_t is_f64; int32_t _pad; } gx_agg;
typedef struct gx_gb_desc {
    const gx_table *t;
    int32_t nkeys;  int32_t key_cols[GX_GB_MAX_KEYS];   /* 0..4 integer columns */
    int32_t naggs;  gx_agg  aggs[GX_GB_MAX_AGGS];        /* 1..8 */
    int32_t nquals; gx_filter quals[GX_MAX_EXTRA_QUALS]; /* AND-ed, integer/date cols */
    int64_t max_groups;   /* 0 = bound by nrows; else the planner's bound */
} gx_gb_desc;
typedef struct gx_gb_result {
    int64_t ngroups; int32_t nkeys, naggs;
    int64_t  *keys;      /* ngroups x nkeys, row-major, sign-extended */
    uint8_t  *key_null;  /* same shape, 1 = NULL (key word 0) */
    uint64_t *aggs;      /* ngroups x naggs: int64, or the double's bits */
    uint8_t  *agg_null;  /* same shape */
} gx_gb_result;
/* ms_kernel: the scan kernel alone (HIP events).  rows_pass: rows left by
 * the visimap and the quals; rows_lds of them were accumulated in a
 * workgroup's LDS table, rows_global directly in the global one. */
typedef struct gx_gbd_stats { double ms_kernel; int64_t rows_in, rows_pass,
                              rows_lds, rows_global, groups; } gx_gbd_stats;
gx_status gx_groupby_desc(gx_ctx *, const gx_gb_desc *, gx_gb_result *out,
                          gx_gbd_stats *stats /* may be NULL */);
void      gx_gb_result_free(gx_gb_result *);
/* groups one workgroup's LDS table holds for a call with naggs aggregates */
int32_t   gx_gb_lds_groups(int naggs);

/* ---- two-stage descriptor GROUP BY through Motion: partial agg per segment
 * (the one-stage scan, its accumulator words are the transition state), hash
 * redistribution of the partial states by group key, combine agg on the
 * owning segment (cdbgroupingpaths.c:251; combine step nodeAgg.c:2305,2321).
 * Same descriptor, validation, error texts, result struct and result order as
 * gx_groupby_desc; returns the groups THIS segment owns:
 *   owner = jump_consistent_hash(cdbhash over the key columns, nsegs), a
 *   width-8 column hashed with hashint8, widths 1, 2 and 4 with hashint4 of
 *   the sign-extended value (hashchar / hashint2 / hashint4, hashfunc.c), a
 *   NULL column contributing the rotation only (cdbhash.c:189-247): (NULL, 1)
 *   and (0, 1) may live on different segments and never merge.
 * nkeys == 0 is a Gather: every segment's partial stage ships exactly one
 *   state row, also over an empty or fully filtered shard; segment 0 returns
 *   the one group, every other segment ngroups == 0.
 * nsegs == 1 without GX_FORCE_MOTION runs the one-stage plan (same output as
 *   gx_groupby_desc, motion stats zero); otherwise gx_comm_init must have been
 *   called (GX_ERR_STATE).  More than 2048 segments is GX_ERR_INVALID.
 * max_groups bounds each segment's partial table and the combine result
 *   (the combine table itself is pow2 >= 2 * recv_rows); either stage
 *   exceeding it is GX_ERR_INVALID "more groups than max_groups".  A rank
 *   whose partial stage failed still takes part in the count all-gather and
 *   the payload exchange, sending no rows, and reports afterwards.  The HBM
 *   budget is checked before the partial table, the exchange buffers and the
 *   combine table are allocated (GX_ERR_OOM).
 * One host sync per Motion: the partial group count and the error word
 *   reach the host with the all-gathered counts.
 * stats: gx_gb_stats as gx_groupby_dist fills it; rows_in = nrows.
 *
 * Wire row of the exchange (fixed stride, 8-byte aligned, deterministic
 * bytes; also the row format of the two test entry points below):
 *   int64  keys[nkeys]       sign-extended; 0 where NULL
 *   uint8  key_null[nkeys]   zero-padded to 8 bytes; absent when nkeys == 0
 *   uint64 acc[awords]       the state words exactly as the table holds them
 * acc[] is opaque: order-preserving images for MIN / MAX, and the non-NULL
 * input count word behind SUM / MIN / MAX.  COUNTs take one word, the others
 * two; the stride is 8 * (nkeys + (nkeys ? 1 : 0) + awords) <= 168 bytes.
 * gx_gbd_wire_stride returns it from nkeys and the aggregates' fn / is_f64
 * alone (host only, t is never read), or -1 for a bad nkeys, naggs or fn. ---- */
gx_status gx_groupby_desc_dist(gx_ctx *, const gx_gb_desc *, gx_gb_result *out,
                               gx_gb_stats *stats /* may be NULL */);
int64_t   gx_gbd_wire_stride(const gx_gb_desc *);

/* ---- descriptor GROUP BY: float8 expression aggregates and float8 quals.
 * What TPC-H Q1 (SUM(price * (1 - disc) * (1 + tax))) and Q6 (SUM(price *
 * disc) WHERE disc BETWEEN .. AND qty < ..) need on top of gx_gb_desc.  The
 * descriptor and gx_agg keep their sizes; the new items travel in gx_gb_ext
 * beside the descriptor.  Tagged structs, no expression trees: an expression
 * is a product of 1..GX_GB_MAX_FACTORS factors, a factor one float8 column c
 * as c (GX_FACTOR_COL), 1.0 - c (GX_FACTOR_ONE_MINUS) or 1.0 + c
 * (GX_FACTOR_ONE_PLUS).
 *
 * ext == NULL, or an ext with nexprs == nfquals == 0 and every agg_expr of
 *   the descriptor's aggregates -1, is exactly gx_groupby_desc /
 *   gx_groupby_desc_dist: same kernels, result bytes and error texts.
 * Factors: the column must be 8 bytes wide and is read as float8; format 0
 *   and format 1 (NULL bitmaps, RLE) both bind.
 * Value: ((f0 * f1) * f2), left to right, every step one IEEE double
 *   operation rounded to nearest (float8mul, float8mi, float8pl of float.c),
 *   never fused: a row's value is bit-identical to the same C expression.
 * NULL: every operator is strict, so an expression is NULL in a row where
 *   any of its columns is NULL; COUNT, SUM, MIN and MAX then treat it as
 *   they treat a NULL column input, and agg_null reports a group without a
 *   non-NULL input.
 * Aggregates: agg_expr[j] >= 0 makes aggregate j's argument exprs[agg_expr[j]]
 *   and the aggregate float8 (aggs[j].col and .is_f64 are ignored): SUM is
 *   float8pl in arrival order, MIN and MAX use float8_cmp_internal's total
 *   order as above, COUNT counts non-NULL values.  On COUNT(*) it is
 *   GX_ERR_INVALID.  The state words, and with them gx_gbd_wire_stride,
 *   depend on fn alone.
 * fquals: AND-ed with the integer quals and the visimap over float8 columns
 *   (width 8), op 0..5 as gx_filter; a NULL input fails the row.  The
 *   comparison is float8_cmp_internal (float.c): every NaN equals every NaN
 *   and is greater than +inf, -0.0 equals +0.0.  A NaN literal is legal.
 * At most GX_GB_MAX_OPERANDS distinct columns over all expressions and
 *   fquals; a column named several times is read once per row.
 * GX_ERR_INVALID names the item in gx_last_error: nexprs, nfquals or
 *   nfactors out of range, a factor or fqual column out of range or not 8
 *   bytes wide, a form outside 0..2, an agg_expr outside -1..nexprs-1 or on
 *   COUNT(*), an fqual op outside 0..5, too many distinct operand columns.
 * Known differences: float8mul's overflow / underflow ereport is not raised
 *   (inf and 0 come back, as gx_q1 documents for its own products); a SUM
 *   whose inputs are all -0.0 returns +0.0, as in gx_groupby_desc. ---- */
#define GX_GB_MAX_FACTORS  3
#define GX_GB_MAX_FQUALS   4
#define GX_GB_MAX_OPERANDS 8   /* distinct float8 columns over all exprs + fquals */
typedef enum { GX_FACTOR_COL = 0, GX_FACTOR_ONE_MINUS = 1, GX_FACTOR_ONE_PLUS = 2 } gx_factor_form;
typedef struct gx_factor { int32_t col; int32_t form; } gx_factor;
typedef struct gx_expr   { int32_t nfactors; int32_t _pad; gx_factor f[GX_GB_MAX_FACTORS]; } gx_expr;
typedef struct gx_fqual  { int32_t col; int32_t op; double literal; } gx_fqual;   /* op 0..5 as gx_filter */
typedef struct gx_gb_ext {
    int32_t  nexprs, nfquals;
    gx_expr  exprs[GX_GB_MAX_AGGS];
    int32_t  agg_expr[GX_GB_MAX_AGGS];  /* -1: argument is aggs[j].col as today; else index into exprs */
    gx_fqual fquals[GX_GB_MAX_FQUALS];
} gx_gb_ext;
gx_status gx_groupby_expr(gx_ctx *, const gx_gb_desc *, const gx_gb_ext * /* may be NULL */,
                          gx_gb_result *out, gx_gbd_stats *stats /* may be NULL */);
gx_status gx_groupby_expr_dist(gx_ctx *, const gx_gb_desc *, const gx_gb_ext * /* may be NULL */,
                               gx_gb_result *out, gx_gb_stats *stats /* may be NULL */);

/* ---- descriptor GROUP BY over a join: the scanned table desc->t is the fact
 * side of up to GX_GBJ_MAX_JOINS inner equi-joins against dimension tables,
 * and a group key column or a column aggregate's argument may come from the
 * matched dimension row ("fact JOIN dim GROUP BY dim.attr").  nodeHashjoin.c
 * inner-join semantics over execScan.c quals, feeding nodeAgg.c.  The
 * descriptor, gx_gb_ext, the result struct, the result order, max_groups, the
 * error style and gx_gbd_wire_stride are those of gx_groupby_desc /
 * gx_groupby_expr; the join items travel in gx_gbj_ext beside them.
 *
 * Join matching: join j is t.fact_col = dim.dim_key_col, an inner join.  Both
 *   are integer columns of width 1, 2, 4 or 8 (format 0 or 1) and may differ
 *   in width: both sides are sign-extended to int64 and compared, the
 *   mathematically correct cross-type equality (int48eq and kin).  The
 *   operator is strict: a fact row whose join column is NULL matches nothing
 *   and is dropped, a dimension row whose key is NULL is never matched.
 * Rows: a dimension row takes part only if its visimap bit is off and all of
 *   its join's quals pass (folded as gx_filter describes; a NULL qual input
 *   fails).  A fact row contributes if its visimap bit is off, the
 *   descriptor's quals and the ext's fquals pass, and EVERY join finds its
 *   row.  rows_probed counts the rows that reached the probes (visimap, quals
 *   and fquals passed), rows_pass those that also matched every join.
 * Unique dimension keys: among the dimension rows that take part, keys must
 *   be unique; this executor does not multiply rows.  A duplicate is
 *   GX_ERR_INVALID, and gx_last_error names the join and one duplicated key
 *   value.  Duplicates among rows the quals or the visimap remove are legal.
 * Keys and aggregates from a dimension: key_side[k] = 0 reads key_cols[k]
 *   from desc->t as before; key_side[k] = j + 1 makes key k the value (or
 *   NULL) of column key_cols[k] of joins[j].dim at the matched row.  Grouping
 *   stays NOT DISTINCT per column: a NULL attribute forms its own group, every
 *   int64 value is a legal key.  agg_side[j] likewise says which table
 *   aggs[j].col indexes; widths, is_f64, strictness and the NULL result rule
 *   are unchanged.  COUNT(*) counts joined rows.  Expression operands, fquals
 *   and the descriptor's quals name columns of the fact table only and have no
 *   side tag.
 * Degenerate inputs: nkeys == 0 gives exactly one group, also when nothing
 *   joins (COUNT 0, the rest NULL).  With keys, an empty fact table, an empty
 *   dimension or a dimension whose quals remove everything gives zero groups.
 *   njoins == 0 with every side 0 is exactly gx_groupby_expr: the same kernel
 *   instantiations, result bytes and error texts.
 * Errors: GX_ERR_INVALID names the item in gx_last_error: njoins out of
 *   range, a NULL dim, a side outside 0..njoins, a column out of range in the
 *   table its side names, a width that is not 1, 2, 4 or 8, a join qual op
 *   outside 0..5, a dimension of 2^32 - 1 rows or more (a join-table slot is a
 *   u32 holding row + 1).  The context stays usable.  The HBM budget check
 *   runs before anything is allocated and includes the join tables (4 bytes
 *   per slot, a power of two of at least 2 x the dimension's rows) and the
 *   flat materialisations of format-1 dimension columns (GX_ERR_OOM).
 * gx_groupby_join_dist: every segment is taken to hold each dimension
 *   COMPLETE (a replicated table, a Broadcast Motion done by the caller, or a
 *   dimension co-located with fact_col); this call moves no dimension rows.
 *   Otherwise it is gx_groupby_expr_dist: the scan is the partial stage,
 *   partition, exchange and combine are unchanged, and a dim-side key routes
 *   by the width of the DIMENSION's column (hashint8 for width 8, hashint4
 *   below).
 * Not supported (DESIGN.md "Descriptor GROUP BY: joins"): outer, semi and
 *   anti joins, non-unique dimension keys, joins of dimensions to dimensions,
 *   dimension columns as expression operands or fqual inputs.
 * Not verified: more than one rank; dimensions near 2^32 rows. ---- */
#define GX_GBJ_MAX_JOINS 2
typedef struct gx_gb_join {
    const gx_table *dim;
    int32_t fact_col;      /* integer column of desc->t, width 1, 2, 4 or 8 */
    int32_t dim_key_col;   /* integer column of dim, width 1, 2, 4 or 8 */
    int32_t nquals, _pad;
    gx_filter quals[GX_MAX_EXTRA_QUALS];   /* AND-ed, over dim's integer/date columns */
} gx_gb_join;
typedef struct gx_gbj_ext {
    int32_t njoins, _pad;                  /* 0..GX_GBJ_MAX_JOINS */
    gx_gb_join joins[GX_GBJ_MAX_JOINS];
    int32_t key_side[GX_GB_MAX_KEYS];      /* 0 = desc->t; j + 1 = joins[j].dim */
    int32_t agg_side[GX_GB_MAX_AGGS];      /* same; key_cols[k] / aggs[j].col index that table */
} gx_gbj_ext;
typedef struct gx_gbj_stats {
    double  ms_build, ms_kernel;           /* join-table builds; scan kernel alone */
    int64_t rows_in, rows_probed, rows_pass, rows_lds, rows_global, groups;
    int64_t dim_rows[GX_GBJ_MAX_JOINS];    /* rows each join table holds */
} gx_gbj_stats;
gx_status gx_groupby_join(gx_ctx *, const gx_gb_desc *, const gx_gbj_ext *,
                          const gx_gb_ext * /* may be NULL */,
                          gx_gb_result *out, gx_gbj_stats * /* may be NULL */);
gx_status gx_groupby_join_dist(gx_ctx *, const gx_gb_desc *, const gx_gbj_ext *,
                               const gx_gb_ext * /* may be NULL */,
                               gx_gb_result *out, gx_gb_stats * /* may be NULL */);

/* ---- test-only entry points (parity harness; not part of the drop-in) ---- */
/* gx_groupby_desc through the same planned call (gbd_run) with the scan grid
 * and the slot word chosen by the caller: grid = 0 is production (2048 workgroups),
 * 1 or 3 make a workgroup see enough of a test-sized input to fill and
 * merge its LDS table; wide_rowid = 1 forces the 8-byte slot word. */
gx_status gx_test_groupby_desc(gx_ctx *, const gx_gb_desc *, int grid,
                               int wide_rowid, gx_gb_result *, gx_gbd_stats *);
/* gx_groupby_expr through the same seam */
gx_status gx_test_groupby_expr(gx_ctx *, const gx_gb_desc *, const gx_gb_ext *,
                               int grid, int wide_rowid, gx_gb_result *,
                               gx_gbd_stats *);
/* Host restatements of the expression value and of the float8 qual through
 * the same host/device functions the scan kernel calls, no GPU needed.
 * expr_eval: vals / isnull are row-major n x ncols (isnull may be NULL = no
 * NULLs), a factor's col indexes them; out[i] receives the value (0.0 where
 * NULL), out_null[i] 1 where any factor's column is NULL.  Returns 0, or 1
 * for bad arguments (nfactors, form or a column out of range).
 * fqual: 1 when `x op literal` passes under float8_cmp_internal, 0 when it
 * fails, -1 for an op outside 0..5. */
int gx_selftest_expr_eval(const gx_expr *, const double *vals,
                          const uint8_t *isnull, int64_t n, int ncols,
                          double *out, uint8_t *out_null);
int gx_selftest_fqual(int op, double x, double literal);
/* gx_groupby_join through the same seam (grid, wide_rowid as above) */
gx_status gx_test_groupby_join(gx_ctx *, const gx_gb_desc *, const gx_gbj_ext *,
                               const gx_gb_ext *, int grid, int wide_rowid,
                               gx_gb_result *, gx_gbj_stats *);
/* partial agg + partition of gx_groupby_join_dist on one GPU, as
 * gx_test_gbd_partial */
gx_status gx_test_gbj_partial(gx_ctx *, const gx_gb_desc *, const gx_gbj_ext *,
                              int nsegs, int64_t *out_counts, void *out_rows,
                              int64_t cap_rows, int64_t *out_total);
/* Host restatement of the join table: a serial build over the dimension keys
 * (dim_null[i] != 0 = NULL, never inserted; dim_null may be NULL) and a probe
 * per fact key, through the same hash, slot and compare functions the
 * kernels call, no GPU needed.  out_row[i] = the matched dimension row or -1
 * (also for a NULL fact key).  Returns 0, 1 for a duplicate dimension key
 * (*dup_key set; out_row untouched), -1 for bad arguments (a negative count,
 * a missing array, 2^32 - 1 dimension rows or more).
 * gx_selftest_gbj_slots: out[i] = the home slot of keys[i] in the join table
 * of a dimension of ndim rows; returns that table's slot count, or -1. */
int64_t gx_selftest_gbj_join(const int64_t *dim_keys, const uint8_t *dim_null,
                             int64_t ndim, const int64_t *fact_keys,
                             const uint8_t *fact_null, int64_t nfact,
                             int64_t *out_row, int64_t *dup_key);
int64_t gx_selftest_gbj_slots(const int64_t *keys, int64_t n, int64_t ndim,
                              uint32_t *out);
/* The final ordering of gx_groupby_desc alone, no GPU needed: perm[0..n)
 * receives the row order of n rows of nkeys (1..GX_GB_MAX_KEYS) columns,
 * row-major keys / key_null, sorted by the (key_null, key) pairs column by
 * column, ascending and stable.  Returns 0, or 1 for bad arguments. */
int gx_selftest_gb_sort(const int64_t *keys, const uint8_t *key_null,
                        int64_t n, int nkeys, int64_t *perm);
/* partial agg + partition for a given nsegs on one GPU: wire rows packed by
 * destination in destination order (order inside one unspecified);
 * GX_ERR_INVALID if the total exceeds cap_rows */
gx_status gx_test_gbd_partial(gx_ctx *, const gx_gb_desc *, int nsegs,
                              int64_t *out_counts /* nsegs */, void *out_rows,
                              int64_t cap_rows, int64_t *out_total);
/* combine over host wire rows; desc->t may be NULL (reads nkeys, aggs,
 * max_groups); wide_rowid = 1 forces the 8-byte slot word; n == 0 returns
 * zero groups for every nkeys */
gx_status gx_test_gbd_combine(gx_ctx *, const gx_gb_desc *, const void *rows,
                              int64_t n, int wide_rowid, gx_gb_result *out);
/* host restatement of the routing through the same GX_HD functions, no GPU:
 * out[i] = owner of row i of n rows of nkeys (0..GX_GB_MAX_KEYS) columns,
 * row-major keys / key_null, widths[k] in 1, 2, 4, 8.  Returns 0, or 1 for
 * bad arguments. */
int gx_selftest_gbd_route(const int64_t *keys, const uint8_t *key_null,
                          const int32_t *widths, int nkeys, int64_t n,
                          int nsegs, int32_t *out);
typedef struct gx_ord_row { int64_t okey, ocust; int32_t odate, oprio; } gx_ord_row;
/* Motion-1 partition kernels on one GPU: filter orders by cutoff, route by
 * cdbhash(o_custkey), emit packed rows grouped by destination segment. */
gx_status gx_test_motion1(gx_ctx *ctx, gx_table *orders, int32_t cutoff,
                          int nsegs, int64_t *out_counts, gx_ord_row *out_rows,
                          int64_t cap, int64_t *out_total);
typedef struct gx_qual_row_abi { int64_t okey; int32_t odate, oprio; } gx_qual_row_abi;
/* Motion stage 2 (received rows → customer semijoin → route by o_orderkey) */
gx_status gx_test_qual(gx_ctx *ctx, gx_table *customer, const gx_ord_row *rows,
                       int64_t n, int nsegs, int64_t *out_counts,
                       gx_qual_row_abi *out_rows, int64_t cap, int64_t *out_total);
/* Motion stage 3 (received qual rows → table build → probe local lineitem) */
gx_status gx_test_q3_from_qual(gx_ctx *ctx, const gx_qual_row_abi *rows,
                               int64_t n, gx_table *lineitem, int32_t cutoff,
                               gx_q3_group **out, int64_t *ngroups);
/* two-stage GROUP BY stages on one GPU.  Partial agg + partition for a given
 * nsegs: packed partial groups, grouped contiguously by destination in
 * destination order (order within a destination unspecified);
 * GX_ERR_INVALID if the total exceeds cap. */
gx_status gx_test_gb_partial(gx_ctx *ctx, const gx_table *t, int key_col, int val_col,
                             int nsegs, int64_t *out_counts /* nsegs */,
                             gx_kv_group *out_rows, int64_t cap, int64_t *out_total);
/* combine agg over received partial rows: key asc, NULL group last */
gx_status gx_test_gb_combine(gx_ctx *ctx, const gx_kv_group *rows, int64_t n,
                             gx_kv_group **out, int64_t *ngroups);
int gx_selftest_addressing(void);

/* ---- the Motion stages of the nsegs>1 Q3 path, one rank at a time.  These
 * run the same launches, dispatch and layout rules as gx_q3_run for any
 * nsegs on one GPU; the caller moves rows between "ranks" on the host with
 * the per-destination counts returned.  Output rows are packed contiguously
 * by destination in destination order (order within one unspecified);
 * GX_ERR_INVALID if the total exceeds cap. ---- */

/* Motion 1 over orders [okey i64, ocust i64, odate i32, oprio i32], visimap
 * honoured.  mid_filter = <col 2 or 3, op, literal>, folded as
 * gx_q3_prepare_desc folds it; as in gx_q3_run the filter column is also the
 * one carried as odate.  bloom_all (optional, host) = nsegs * bwords words,
 * rank r's dim bloom at r * bwords, bwords a power of two >= 4096; it is used
 * for dim_join == 0 only (the destination prefilter is off for anti joins). */
gx_status gx_test_m1(gx_ctx *ctx, gx_table *orders, const gx_filter *mid_filter,
                     int nsegs, int dim_join, const uint64_t *bloom_all,
                     uint64_t bwords, int64_t *out_counts /* nsegs */,
                     gx_ord_row *out_rows, int64_t cap, int64_t *out_total);
/* Dim side of one rank: customer [ckey i64, attr i8] filtered by <op,
 * literal> on the i8 column (visimap honoured) into the hash set + bloom of
 * the Motion path.  bwords (power of two >= 4096) stands in for the
 * max-over-ranks agreement; out_bloom receives bwords words.  out_set_width:
 * 4 when every selected key is < 2^32, else 8. */
gx_status gx_test_dim(gx_ctx *ctx, gx_table *customer, int32_t op,
                      int64_t literal, uint64_t bwords, uint64_t *out_bloom,
                      int64_t *out_nsel, int32_t *out_set_width);
/* Motion 2: rows received by this rank against its dim set (built as
 * gx_test_dim builds it; bwords 0 = this rank's own size), semi (dim_join 0)
 * or anti, qualifying rows routed by okey. */
gx_status gx_test_m2(gx_ctx *ctx, gx_table *customer, int32_t op,
                     int64_t literal, uint64_t bwords, const gx_ord_row *rows,
                     int64_t n, int dim_join, int nsegs,
                     int64_t *out_counts /* nsegs */, gx_qual_row_abi *out_rows,
                     int64_t cap, int64_t *out_total, int32_t *out_set_width);
/* Layout of the join/agg table built from received rows (what gx_q3_run
 * derives before a cached-table reuse decision). */
typedef struct gx_test_tbl_layout {
    int32_t  key_width;        /* 4 when kmax < 2^32, else 8 */
    int32_t  interpolated;     /* 1 = order-preserving slot map, 0 = hashed */
    uint64_t slots;            /* power of two, > qual */
    int64_t  kmin;
    double   scale;            /* slots / range; < 0 when hashed */
    uint64_t slot_kmin, slot_kmax;   /* first-probe slots of kmin and kmax */
} gx_test_tbl_layout;
/* Motion 3: table from received qualifying rows (nsegs of ctx enters the
 * density rule), then probe + aggregate lineitem [lkey i64, price f64,
 * disc f64, shipdate i32] filtered by <op, literal> on shipdate, visimap
 * honoured.  Groups sorted by key; caller frees *out with gx_free.  layout
 * may be NULL. */
gx_status gx_test_m3(gx_ctx *ctx, const gx_qual_row_abi *rows, int64_t n,
                     gx_table *lineitem, int32_t op, int64_t literal,
                     gx_q3_group **out, int64_t *ngroups,
                     gx_test_tbl_layout *layout);
/* The two pure host helpers of the Motion path, no GPU needed.  cnts_all
 * (optional) is the all-gathered n×n count matrix (row r = rank r's
 * per-destination counts): rank seg's send/receive counts (n entries) and
 * exclusive offsets (n + 1 entries, the last the total).  layout (optional):
 * table layout for qual keys spanning [kmin, kmax] at nsegs with fill factor
 * tf_pct.  Returns 0, or 1 for bad arguments. */
int gx_selftest_motion_layout(const uint64_t *cnts_all, int n, int seg,
                              uint64_t *scnt, uint64_t *soff,
                              uint64_t *rcnt, uint64_t *roff,
                              int64_t qual, uint64_t kmin, uint64_t kmax,
                              int nsegs, int tf_pct,
                              gx_test_tbl_layout *layout);

/* ---- the result tail of Q3: top-N select and the unmatched-table bound ---- */

/* The top-N stage over caller-supplied host SoA arrays of n groups: uploads
 * them and runs exactly what gx_q3_topn runs (same launch, copy and merge).
 * rev holds f64 revenues, or the int64 numerators' words when numeric != 0;
 * flags (bit 0 key_is_null, bit 1 attrs_null = NULL date) may be NULL.
 * GX_ERR_INVALID, with nothing written, unless n >= 0 and 1 <= topn <= 10. */
gx_status gx_test_topn(gx_ctx *ctx, const int64_t *okey, const int32_t *odate,
                       const int32_t *oprio, const double *rev,
                       const int64_t *cnt, const uint8_t *flags, int64_t n,
                       int numeric, int topn, gx_q3_group *out, int64_t *nout);
/* The host merge of that stage alone, no GPU needed: ncand candidates as the
 * device stage hands them over, cidx[i] < 0 marking an empty one (its other
 * fields are ignored; keys are data and mark nothing).  Writes the first
 * min(topn, valid) rows by revenue DESC, effective date ASC (flag bit 1 set
 * = NULL date = last).  Returns 0, or 1 for bad arguments. */
int gx_selftest_topn_merge(const int64_t *cidx, const int64_t *okey,
                           const int32_t *odate, const int32_t *oprio,
                           const double *rev, const int64_t *cnt,
                           const uint8_t *flags, int ncand, int numeric,
                           int topn, gx_q3_group *out, int64_t *nout);
/* Sizing's bound on the LEFT-OUTER unmatched groups for a fact key column of
 * nrows rows whose keys, as unsigned words, span [lmin, lmax]; no GPU
 * needed.  Never below min(nrows, lmax - lmin + 1) + 1, the span taken
 * without wrap-around. */
uint64_t gx_selftest_unmatched_bound(int64_t nrows, uint64_t lmin,
                                     uint64_t lmax);
/* Sizing's rule for the rank form of the join/agg table (gx_q3_table_mode)
 * on caller-supplied stats: qual qualifying mid rows whose keys, as unsigned
 * words, span [kmin, kmax]; enabled = GX_RANK_TABLE is not 0.  No GPU
 * needed.  Returns 1 or 0. */
int gx_selftest_rank_eligible(int64_t qual, uint64_t kmin, uint64_t kmax,
                              int enabled);
/* Keys covered by one block of the rank table's prefix-popcount scan (ranks
 * of keys further apart cross a block boundary of that scan). */
int64_t gx_rank_scan_block_keys(void);
/* The rule behind gx_q3_orders_mode on caller-supplied counts: qual
 * qualifying of nrows mid rows; env is GX_ORDERS_STAGED (0 or 1 forces,
 * negative = unset: staged iff qual * K <= nrows, computed without the
 * product).  No GPU needed.  Returns 1 (staged) or 0 (two-pass). */
int gx_selftest_orders_staged(int64_t qual, int64_t nrows, int env);
/* K of that rule. */
int64_t gx_orders_stage_rule_k(void);
/* Blocks of the staged form's filter grid for those counts (a wave's
 * expected records fill three quarters of its segment).  No GPU needed. */
int64_t gx_selftest_orders_stage_grid(int64_t qual, int64_t nrows);
/* Records of one wave's LDS segment in the staged filter kernel (W). */
int64_t gx_orders_stage_wave_records(void);
/* How bind routes each block of a format-1 stream of 8-byte datums for the
 * fused RLE fact-key probe; no GPU needed.  cls[b]: 0 = not fused (Orig,
 * DELTA, NULL bitmap, more than 4096 physical datums: one such block and
 * prepare materializes the whole column), 1 = Dense without a repeat bitmap,
 * 2 = RLE with repeat counts of mixed byte lengths (serial count walk),
 * 3 = RLE with every count 2 bytes (parallel count decode).  Writes at most
 * cap entries; returns the number of blocks, or -1 for a stream bind
 * refuses. */
int64_t gx_selftest_rle_block_class(const uint8_t *stream, int64_t nbytes,
                                    int32_t *cls, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GPUEXEC_H */
