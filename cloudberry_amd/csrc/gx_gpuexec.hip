/*
 * gx_gpuexec.hip — MI355X-native (gfx950) executor for Cloudberry's
 * segment-local scan→hash-join→hash-agg pipeline + hash-redistribute Motion.
 *
 * Implements include/gpuexec.h.  This is the PRODUCT path: hand-written HIP
 * kernels over AOCS column streams resident in HBM, RCCL over xGMI for the
 * Motion exchange.  The oracle (oracle/) is never referenced here.
 *
 * Reference semantics being replaced, per stage (paths under /root/reference):
 *   scan+filter   executor/nodeSeqscan.c:57, execScan.c:161-263,
 *                 access/aocs/aocsam.c:1131-1259 (per-row datum fetch → here:
 *                 O(1) block addressing + coalesced loads, headers skipped)
 *   hash join     executor/nodeHash.c:1886,2098-2251, nodeHashjoin.c:252-834
 *                 (chain buckets → here: SoA open addressing, build-then-probe;
 *                 layout/internal hash parity-irrelevant)
 *   hash agg      executor/nodeAgg.c:836,2288,2743 + float.c:769 float8pl
 *                 (per-row transition → here: f64 atomic add per group slot)
 *   two-stage agg cdb/cdbgroupingpaths.c:251 + executor/nodeAgg.c:2305,2321
 *                 (partial agg → Redistribute Motion → combine agg → here:
 *                 the partial table's groups routed and merged on device)
 *   Motion        executor/nodeMotion.c:1088,1181 + cdb/cdbhash.c:189-285,
 *                 530-541 (bit-exact routing), cdb/motion/* + contrib/
 *                 interconnect UDP (→ RCCL grouped send/recv, columnar batches)
 */
#include "gx_internal.h"
#include "../../include/gpuexec.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <zlib.h>

/* libzstd.so.1 ships without headers in this image — single-shot API */
extern "C" size_t ZSTD_decompress(void *dst, size_t dstCap, const void *src,
                                  size_t srcSize);
extern "C" unsigned ZSTD_isError(size_t code);

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <map>
#include <set>
#include <utility>

/* ================= error plumbing ================= */

static char g_global_err[512] = "";

struct gx_ctx {
    int device = -1;
    int seg = 0;
    int nsegs = 1;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   /* Motion overlap (r2): the exchange
                                        runs here concurrently with the
                                        dim build on `stream` */
    ncclComm_t comm = nullptr;
    char err[512] = "";
};

static void set_err(gx_ctx *ctx, const char *fmt, const char *detail)
{
    char *dst = ctx ? ctx->err : g_global_err;
    snprintf(dst, 512, fmt, detail);
}

#define HIP_CHK(ctx, call)                                                    \
    do {                                                                      \
        hipError_t _e = (call);                                               \
        if (_e != hipSuccess) {                                               \
            set_err(ctx, "HIP error: %s (" #call ")", hipGetErrorString(_e)); \
            return (_e == hipErrorOutOfMemory) ? GX_ERR_OOM : GX_ERR_HIP;     \
        }                                                                     \
    } while (0)

#define RCCL_CHK(ctx, call)                                                   \
    do {                                                                      \
        ncclResult_t _r = (call);                                             \
        if (_r != ncclSuccess) {                                              \
            set_err(ctx, "RCCL error: %s (" #call ")", ncclGetErrorString(_r)); \
            return GX_ERR_RCCL;                                               \
        }                                                                     \
    } while (0)

extern "C" const char *gx_last_error(const gx_ctx *ctx)
{
    return ctx ? ctx->err : g_global_err;
}

extern "C" const char *gx_version(void) { return "gpuexec 0.1 (gfx950)"; }

/* ================= small device helpers ================= */

static constexpr int TPB = 256;          /* threads per block (4 waves) */
static constexpr int GRID = 2048;        /* grid-stride grid (fills 256 CUs) */
static constexpr int ORDERS_GRID = 32768; /* k_orders_build: measured optimum */

/* Owning device buffer, move-only.  As a local, early returns
 * (HIP_CHK/RCCL_CHK) free it; as a member of gx_q3 it is the run state, freed
 * with the q.  alloc replaces what the buffer held; reserve only ever grows
 * it (contents are not kept). */
struct devbuf {
    void *p = nullptr;
    size_t cap = 0;
    devbuf() = default;
    devbuf(const devbuf &) = delete;
    devbuf &operator=(const devbuf &) = delete;
    devbuf(devbuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    devbuf &operator=(devbuf &&o) noexcept
    {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~devbuf() { reset(); }
    void reset() { if (p) (void) hipFree(p); p = nullptr; cap = 0; }
    hipError_t alloc(size_t bytes)
    {
        reset();
        hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
        if (e == hipSuccess) cap = bytes ? bytes : 1;
        else p = nullptr;
        return e;
    }
    hipError_t reserve(size_t bytes) { return bytes <= cap ? hipSuccess : alloc(bytes); }
    template <typename T> T *as() const { return (T *) p; }
};
static_assert(!std::is_copy_constructible<devbuf>::value, "devbuf owns its allocation");

/* RAII for HIP events: early returns (HIP_CHK/RCCL_CHK/OOM) destroy them
 * automatically instead of accumulating across repeated failing steps */
struct evholder {
    hipEvent_t e = nullptr;
    ~evholder() { if (e) (void) hipEventDestroy(e); }
    hipError_t create() { return hipEventCreate(&e); }
    operator hipEvent_t() const { return e; }
};

static inline int env_int(const char *name, int dflt)
{
    const char *v = getenv(name);
    return v ? atoi(v) : dflt;
}

static inline int64_t pow2_at_least(int64_t want)
{
    int64_t sz = 1024;
    while (sz < want) sz <<= 1;
    return sz;
}

/* launch dispatch: kernels are compiled per key width and per boolean mode;
 * these turn the run-time (width, void *) pair or flag into the typed call.
 * f receives the pointer as unsigned int * (width 4) or unsigned long long *
 * (any other width), resp. std::true_type / std::false_type. */
template <typename F>
static inline void by_width(int width, const void *p, F &&f)
{
    if (width == 4) f((const unsigned int *) p);
    else f((const unsigned long long *) p);
}

template <typename F>
static inline void by_width(int width, void *p, F &&f)
{
    if (width == 4) f((unsigned int *) p);
    else f((unsigned long long *) p);
}

template <typename F>
static inline void by_flag(bool on, F &&f)
{
    if (on) f(std::true_type{});
    else f(std::false_type{});
}

/* ================= generation: count / scan / emit ================= */
/* Deterministic sharded generation: each thread owns a contiguous chunk of
 * GLOBAL units (rows for customer/orders, orders for lineitem), counts the
 * rows it keeps for this segment, host exclusive-scans the per-thread
 * counts (stable order = global order, matching the oracle), then emit. */

static constexpr int64_t GEN_CHUNK = 512;

__global__ void k_count_cust(uint64_t seed, int64_t n, int seg, int nsegs, uint32_t *counts)
{
    int64_t t = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t lo = t * GEN_CHUNK, hi = min(lo + GEN_CHUNK, n);
    if (lo >= n) { counts[t] = 0; return; }
    uint32_t c = 0;
    for (int64_t i = lo; i < hi; i++)
        if (nsegs == 1 || gx_route_i64(i + 1, nsegs) == seg) c++;
    counts[t] = c;
}

__global__ void k_emit_cust(uint64_t seed, int64_t n, int seg, int nsegs,
                            const uint64_t *offs, int64_t *custkey, uint8_t *mkt)
{
    int64_t t = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t lo = t * GEN_CHUNK, hi = min(lo + GEN_CHUNK, n);
    if (lo >= n) return;
    uint64_t w = offs[t];
    for (int64_t i = lo; i < hi; i++)
        if (nsegs == 1 || gx_route_i64(i + 1, nsegs) == seg)
        {
            custkey[w] = i + 1;
            mkt[w] = gx_gen_mktsegment(seed, i);
            w++;
        }
}

__global__ void k_count_ord(uint64_t seed, int64_t n, int seg, int nsegs, uint32_t *counts)
{
    int64_t t = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t lo = t * GEN_CHUNK, hi = min(lo + GEN_CHUNK, n);
    if (lo >= n) { counts[t] = 0; return; }
    uint32_t c = 0;
    for (int64_t i = lo; i < hi; i++)
        if (nsegs == 1 || gx_route_i64(i + 1, nsegs) == seg) c++;
    counts[t] = c;
}

__global__ void k_emit_ord(uint64_t seed, int64_t n, int64_t ncust, int seg, int nsegs,
                           const uint64_t *offs, int64_t *okey, int64_t *ocust,
                           int32_t *odate, int32_t *oprio)
{
    int64_t t = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t lo = t * GEN_CHUNK, hi = min(lo + GEN_CHUNK, n);
    if (lo >= n) return;
    uint64_t w = offs[t];
    for (int64_t i = lo; i < hi; i++)
        if (nsegs == 1 || gx_route_i64(i + 1, nsegs) == seg)
        {
            okey[w] = i + 1;
            ocust[w] = gx_gen_ocustkey(seed, i, ncust);
            odate[w] = gx_gen_odate(seed, i);
            oprio[w] = gx_gen_oprio(seed, i);
            w++;
        }
}

__global__ void k_count_li(uint64_t seed, int64_t nord, int seg, int nsegs, uint32_t *counts)
{
    int64_t t = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t lo = t * GEN_CHUNK, hi = min(lo + GEN_CHUNK, nord);
    if (lo >= nord) { counts[t] = 0; return; }
    uint32_t c = 0;
    for (int64_t o = lo + 1; o <= hi; o++)
        if (nsegs == 1 || gx_route_i64(o, nsegs) == seg)
            c += gx_gen_nlines(seed, o);
    counts[t] = c;
}

__global__ void k_emit_li(uint64_t seed, int64_t nord, int seg, int nsegs,
                          const uint64_t *offs, int64_t *lkey, double *price,
                          double *disc, int32_t *ship)
{
    int64_t t = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t lo = t * GEN_CHUNK, hi = min(lo + GEN_CHUNK, nord);
    if (lo >= nord) return;
    uint64_t w = offs[t];
    for (int64_t o = lo + 1; o <= hi; o++)
    {
        if (!(nsegs == 1 || gx_route_i64(o, nsegs) == seg)) continue;
        int32_t nl = gx_gen_nlines(seed, o);
        for (int32_t j = 0; j < nl; j++)
        {
            lkey[w] = o;
            price[w] = gx_gen_price(seed, o, j);
            disc[w] = gx_gen_discount(seed, o, j);
            ship[w] = gx_gen_shipdate(seed, o, j);
            w++;
        }
    }
}

__global__ void k_emit_li_num(uint64_t seed, int64_t nord, int seg, int nsegs,
                              const uint64_t *offs, int64_t *lkey,
                              int64_t *price_c, int64_t *disc_c, int32_t *ship)
{
    int64_t t = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t lo = t * GEN_CHUNK, hi = min(lo + GEN_CHUNK, nord);
    if (lo >= nord) return;
    uint64_t w = offs[t];
    for (int64_t o = lo + 1; o <= hi; o++)
    {
        if (!(nsegs == 1 || gx_route_i64(o, nsegs) == seg)) continue;
        int32_t nl = gx_gen_nlines(seed, o);
        for (int32_t j = 0; j < nl; j++)
        {
            lkey[w] = o;
            /* the exact scaled-integer forms of gx_gen_price/_discount */
            price_c[w] = (int64_t) (90000 + gx_mix(seed, GX_ST_LI_PRICE,
                                                   (uint64_t) o * 8 + j) % 10410001ULL);
            disc_c[w] = (int64_t) (gx_mix(seed, GX_ST_LI_DISC,
                                          (uint64_t) o * 8 + j) % 11);
            ship[w] = gx_gen_shipdate(seed, o, j);
            w++;
        }
    }
}

__global__ void k_emit_li_q1(uint64_t seed, int64_t nord, int seg, int nsegs,
                             const uint64_t *offs, int8_t *flag, int8_t *status,
                             double *price, double *disc, int32_t *ship)
{
    int64_t t = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t lo = t * GEN_CHUNK, hi = min(lo + GEN_CHUNK, nord);
    if (lo >= nord) return;
    uint64_t w = offs[t];
    for (int64_t o = lo + 1; o <= hi; o++)
    {
        if (!(nsegs == 1 || gx_route_i64(o, nsegs) == seg)) continue;
        int32_t nl = gx_gen_nlines(seed, o);
        for (int32_t j = 0; j < nl; j++)
        {
            flag[w] = (int8_t) gx_gen_returnflag(seed, o, j);
            status[w] = (int8_t) gx_gen_linestatus(seed, o, j);
            price[w] = gx_gen_price(seed, o, j);
            disc[w] = gx_gen_discount(seed, o, j);
            ship[w] = gx_gen_shipdate(seed, o, j);
            w++;
        }
    }
}

/* TPC-H Q1 core (BASELINE config 4): GROUP BY l_returnflag,l_linestatus —
 * 6 fixed groups, so each THREAD accumulates privately in registers, each
 * wave shuffle-reduces, and one lane per wave issues 18 atomics
 * (cdna_hip_programming.md Appendix B Reduction pattern; replaces the
 * per-row simplehash transition of nodeAgg.c:2288,836). */
__global__ void k_q1_agg(const uint8_t *fl_s, gx_colmeta fl_m,
                         const uint8_t *st_s, gx_colmeta st_m,
                         const uint8_t *pr_s, gx_colmeta pr_m,
                         const uint8_t *di_s, gx_colmeta di_m,
                         const uint8_t *sh_s, gx_colmeta sh_m,
                         const uint8_t *vmap, int32_t cutoff,
                         unsigned long long *g_count, double *g_price,
                         double *g_rev)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
    double sp[6] = {0, 0, 0, 0, 0, 0};
    double sr[6] = {0, 0, 0, 0, 0, 0};
    for (; i < fl_m.nrows; i += stride)
    {
        if (gx_vm_hidden(vmap, i)) continue;
        if (!(gx_col_get<int32_t>(sh_s, sh_m, i) <= cutoff)) continue;
        int g = gx_col_get<int8_t>(fl_s, fl_m, i) * 2 +
                gx_col_get<int8_t>(st_s, st_m, i);
        double p = gx_col_get<double>(pr_s, pr_m, i);
        double d = gx_col_get<double>(di_s, di_m, i);
        cnt[g]++;
        sp[g] += p;
        sr[g] += p * (1.0 - d);
    }
#pragma unroll
    for (int g = 0; g < 6; g++)
    {
        for (int o = 32; o; o >>= 1)
        {
            cnt[g] += __shfl_down(cnt[g], o, 64);
            sp[g] += __shfl_down(sp[g], o, 64);
            sr[g] += __shfl_down(sr[g], o, 64);
        }
        if ((threadIdx.x & 63) == 0 && cnt[g])
        {
            atomicAdd(&g_count[g], cnt[g]);
            atomicAdd(&g_price[g], sp[g]);
            atomicAdd(&g_rev[g], sr[g]);
        }
    }
}

/* ================= AOCS encode / decode ================= */

/* Writes headers + datums for one AO block per workgroup (CRCs in a second
 * pass).  The stream buffer must be zeroed first (pad bytes stay 0). */
template <typename T>
__global__ void k_encode(const T *vals, int64_t nrows, int32_t rpb,
                         int64_t full_len, int64_t nblocks, uint8_t *stream)
{
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x)
    {
        int64_t base = b * (int64_t) rpb;
        int32_t rows = (int32_t) min((int64_t) rpb, nrows - base);
        uint8_t *blk = stream + b * full_len;
        T *datum = (T *) (blk + GX_AOCS_DATUM_OFF);
        for (int32_t i = threadIdx.x; i < rows; i += blockDim.x)
            datum[i] = vals[base + i];
        if (threadIdx.x == 0)
        {
            int32_t sz = rows * (int32_t) sizeof(T);
            int32_t content = 16 + sz;
            /* AOSmallContentHeader (cdbappendonlystorage_int.h:150-170) */
            uint32_t b03 = (1u << 28) | (1u << 27) | (1u << 24) |
                           (0x00FFFC00u & ((uint32_t) rows << 10)) |
                           (((uint32_t) content >> 11) & 0x3FFu);
            uint32_t b47 = ((uint32_t) content & 0x7FFu) << 21;
            ((uint32_t *) blk)[0] = b03;
            ((uint32_t *) blk)[1] = b47;
            ((int64_t *) blk)[2] = base + 1;     /* firstRowNum */
            /* DatumStreamBlock_Orig (datumstreamblock.h:73-84) */
            uint8_t *c = blk + 24;
            ((int16_t *) c)[0] = 0;               /* version Original */
            ((int16_t *) c)[1] = 0;               /* flags */
            ((int16_t *) c)[2] = (int16_t) rows;  /* ndatum */
            ((int16_t *) c)[3] = 0;               /* encrypted */
            ((int32_t *) c)[2] = 0;               /* nullsz */
            ((int32_t *) c)[3] = sz;              /* sz */
        }
    }
}

/* CRC32C (pg COMP_CRC32C state, no final xor — cdbappendonlystorageformat.c:
 * 41-47), SLICE-BY-8: 8 derived tables collapse the byte-serial chain to
 * one XOR tree per 8 input bytes (the standard Intel slicing scheme —
 * same polynomial, bit-identical result).  Tables built in LDS per
 * workgroup (8 KB). */
__device__ __forceinline__ uint32_t d_crc32c(const uint32_t (*tab)[256],
                                             uint32_t crc,
                                             const uint8_t *p, int64_t len)
{
    while (len > 0 && ((uintptr_t) p & 7))
    {
        crc = tab[0][(crc ^ *p++) & 0xFF] ^ (crc >> 8);
        len--;
    }
    while (len >= 8)
    {
        uint64_t v = *(const uint64_t *) p;
        uint32_t lo = (uint32_t) v ^ crc;
        uint32_t hi = (uint32_t) (v >> 32);
        crc = tab[7][lo & 0xFF] ^ tab[6][(lo >> 8) & 0xFF] ^
              tab[5][(lo >> 16) & 0xFF] ^ tab[4][lo >> 24] ^
              tab[3][hi & 0xFF] ^ tab[2][(hi >> 8) & 0xFF] ^
              tab[1][(hi >> 16) & 0xFF] ^ tab[0][hi >> 24];
        p += 8;
        len -= 8;
    }
    while (len--)
        crc = tab[0][(crc ^ *p++) & 0xFF] ^ (crc >> 8);
    return crc;
}

__device__ void d_crc_table_init(uint32_t (*tab)[256])
{
    for (int i = threadIdx.x; i < 256; i += blockDim.x)
    {
        uint32_t c = i;
        for (int k = 0; k < 8; k++)
            c = (c & 1) ? (0x82F63B78u ^ (c >> 1)) : (c >> 1);
        tab[0][i] = c;
    }
    __syncthreads();
    /* tab[k][i] = crc of byte i followed by k zero bytes */
    for (int k = 1; k < 8; k++)
    {
        for (int i = threadIdx.x; i < 256; i += blockDim.x)
        {
            uint32_t c = tab[k - 1][i];
            tab[k][i] = tab[0][c & 0xFF] ^ (c >> 8);
        }
        __syncthreads();
    }
}

__global__ void k_crc_fill(uint8_t *stream, int64_t nblocks, int64_t full_len,
                           int64_t nrows, int32_t rpb, int32_t width)
{
    __shared__ uint32_t tab[8][256];
    d_crc_table_init(tab);
    int64_t t = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    for (int64_t b = t; b < nblocks; b += gridDim.x * (int64_t) blockDim.x)
    {
        int64_t base = b * (int64_t) rpb;
        int64_t rows = min((int64_t) rpb, nrows - base);
        int64_t blen = gx_aocs_block_len(width, rows);
        uint8_t *blk = stream + b * full_len;
        ((uint32_t *) blk)[2] = d_crc32c(tab, 0xFFFFFFFFu, blk + 16, blen - 16);
        ((uint32_t *) blk)[3] = d_crc32c(tab, 0xFFFFFFFFu, blk, 12);
    }
}

/* decode: one workgroup per AO block → flat values; header sanity-checked */
template <typename T>
__global__ void k_decode(const uint8_t *stream, int64_t nblocks, int64_t full_len,
                         int64_t nrows, int32_t rpb, T *out, int *err)
{
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x)
    {
        const uint8_t *blk = stream + b * full_len;
        uint32_t b03 = ((const uint32_t *) blk)[0];
        uint32_t rows = (b03 & 0x00FFFC00u) >> 10;
        if (threadIdx.x == 0)
        {
            uint32_t b47 = ((const uint32_t *) blk)[1];
            uint32_t datalen = ((b03 & 0x3FFu) << 11) | ((b47 & 0xFFE00000u) >> 21);
            int64_t frn = ((const int64_t *) blk)[2];
            int16_t version = ((const int16_t *) (blk + 24))[0];
            int16_t ndatum = ((const int16_t *) (blk + 24))[2];
            int32_t sz = ((const int32_t *) (blk + 24))[3];
            if (((b03 >> 28) & 7) != 1 || !((b03 >> 27) & 1) ||
                (b47 & 0x1FFFFFu) != 0 || version != 0 ||
                (uint32_t) ndatum != rows || sz != (int32_t) rows * (int32_t) sizeof(T) ||
                datalen != 16 + (uint32_t) sz || frn != b * (int64_t) rpb + 1)
                atomicOr(err, 1);
        }
        const T *datum = (const T *) (blk + GX_AOCS_DATUM_OFF);
        int64_t base = b * (int64_t) rpb;
        int64_t rows_i = min((int64_t) rows, nrows - base);
        for (int64_t i = threadIdx.x; i < rows_i; i += blockDim.x)
            out[base + i] = datum[i];
    }
}

__global__ void k_verify_crc(const uint8_t *stream, int64_t nblocks, int64_t full_len,
                             int64_t nrows, int32_t rpb, int32_t width, int *err)
{
    __shared__ uint32_t tab[8][256];
    d_crc_table_init(tab);
    int64_t t = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    for (int64_t b = t; b < nblocks; b += gridDim.x * (int64_t) blockDim.x)
    {
        int64_t base = b * (int64_t) rpb;
        int64_t rows = min((int64_t) rpb, nrows - base);
        int64_t blen = gx_aocs_block_len(width, rows);
        const uint8_t *blk = stream + b * full_len;
        if (((const uint32_t *) blk)[3] != d_crc32c(tab, 0xFFFFFFFFu, blk, 12) ||
            ((const uint32_t *) blk)[2] != d_crc32c(tab, 0xFFFFFFFFu, blk + 16, blen - 16))
            atomicOr(err, 2);
    }
}

__global__ void k_verify_crc_dir(const uint8_t *stream, const gx_blockref *dir,
                                 int64_t nblocks, int *err)
{
    __shared__ uint32_t tab[8][256];
    d_crc_table_init(tab);
    int64_t t = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    for (int64_t b = t; b < nblocks; b += gridDim.x * (int64_t) blockDim.x)
    {
        const uint8_t *blk = stream + dir[b].offset;
        uint32_t b03 = ((const uint32_t *) blk)[0];
        uint32_t b47 = ((const uint32_t *) blk)[1];
        uint32_t kind = (b03 >> 28) & 7;
        uint32_t datalen = (kind == 1)
            ? (((b03 & 0x3FFu) << 11) | ((b47 & 0xFFE00000u) >> 21))
            : (b03 & 0x1FFFFFu);
        int64_t blen = (24 + (int64_t) datalen + 7) & ~7LL;
        if (((const uint32_t *) blk)[3] != d_crc32c(tab, 0xFFFFFFFFu, blk, 12) ||
            ((const uint32_t *) blk)[2] != d_crc32c(tab, 0xFFFFFFFFu, blk + 16, blen - 16))
            atomicOr(err, 2);
    }
}

/* Dense(±RLE±DELTA±NULL) and Orig(±NULL) block decode — one THREAD per AO
 * block (blocks decode in parallel across the grid; the per-block walk is
 * inherently serial).  Walker mirrors DatumStreamBlockRead_AdvanceDense/
 * …DenseDelta (datumstreamblock.h:1624-1912) and oracle/oracle.c
 * decode_dense_content_v.  validity: one byte per row (1 = non-null, null
 * datums decode as zero); nullptr REFUSES null-bearing blocks. */
template <typename T>
__global__ void k_decode_dense(const uint8_t *stream, const gx_blockref *dir,
                               int64_t nblocks, int64_t nrows, T *out,
                               uint8_t *validity, int *err)
{
    int64_t t = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    for (int64_t b = t; b < nblocks; b += gridDim.x * (int64_t) blockDim.x)
    {
        const uint8_t *blk = stream + dir[b].offset;
        const uint8_t *c = blk + 24;
        int16_t version = ((const int16_t *) c)[0];
        int16_t flags = ((const int16_t *) c)[1];
        int32_t logical = ((const int32_t *) c)[1];
        int32_t phys = ((const int32_t *) c)[2];
        int32_t psize = ((const int32_t *) c)[3];
        T *dst = out + dir[b].first_row;
        uint8_t *vdst = validity ? validity + dir[b].first_row : nullptr;
        if (dir[b].first_row + logical > nrows || logical != dir[b].rows)
        { atomicOr(err, 1); continue; }
        if (version == 0)
        {
            /* Orig: flags at +2, ndatum at +4 (int16), nullsz at +8,
             * null bitmap at +16, datums at +16+nullsz */
            int16_t oflags = ((const int16_t *) c)[1];
            int16_t nd = ((const int16_t *) c)[2];
            int32_t nullsz = ((const int32_t *) c)[2];
            if (nd != logical) { atomicOr(err, 1); continue; }
            if (!(oflags & 1))
            {
                if (nullsz != 0) { atomicOr(err, 1); continue; }
                const T *d = (const T *) (c + 16);
                for (int32_t i = 0; i < logical; i++) dst[i] = d[i];
                if (vdst)
                    for (int32_t i = 0; i < logical; i++) vdst[i] = 1;
                continue;
            }
            if (!vdst) { atomicOr(err, 1); continue; }
            {
                const uint8_t *nbmp = c + 16;
                const T *d = (const T *) (c + 16 + nullsz);
                int32_t vi = 0;
                for (int32_t i = 0; i < logical; i++)
                {
                    if ((nbmp[i >> 3] >> (i & 7)) & 1)
                    { dst[i] = (T) 0; vdst[i] = 0; }
                    else
                    { dst[i] = d[vi++]; vdst[i] = 1; }
                }
            }
            continue;
        }
        bool has_null = (flags & 0x1) != 0;
        if ((version != 1 && version != 2) || (has_null && !vdst) ||
            psize != phys * (int32_t) sizeof(T))
        { atomicOr(err, 1); continue; }
        bool rle = (flags & 0x2) != 0, delta = (flags & 0x4) != 0;
        if (!rle && !delta && !has_null)
        {
            if (logical != phys) { atomicOr(err, 1); continue; }
            const T *d = (const T *) (c + 16);
            for (int32_t i = 0; i < logical; i++) dst[i] = d[i];
            if (vdst)
                for (int32_t i = 0; i < logical; i++) vdst[i] = 1;
            continue;
        }
        const uint8_t *p = c + 16;
        int32_t bmbits = 0, csize = 0, dbmbits = 0, dsize = 0;
        int32_t nullbits = has_null ? logical : 0;   /* no-RLE: bit per row */
        if (rle)
        {
            int32_t norepeats = ((const int32_t *) p)[0];
            if (has_null) nullbits = norepeats;
            else if (norepeats != 0) { atomicOr(err, 1); continue; }
            bmbits = ((const int32_t *) p)[1];
            csize = ((const int32_t *) p)[3];
            p += 16;
        }
        if (delta)
        {
            dbmbits = *(const int32_t *) p;
            dsize = ((const int32_t *) p)[2];
            p += 12;
        }
        const uint8_t *nbmp = nullptr, *bmp = nullptr, *cnts = nullptr,
                      *dbm = nullptr, *dbs = nullptr;
        if (has_null) { nbmp = p; p += (nullbits + 7) >> 3; }
        if (rle) { bmp = p; p += (bmbits + 7) >> 3; cnts = p; p += csize; }
        if (delta) { dbm = p; p += (dbmbits + 7) >> 3; dbs = p; p += dsize; }
        int32_t hdr = (int32_t) (p - c);
        const T *datum = (const T *) (c + ((hdr + 7) & ~7));

        int64_t w = 0;
        int32_t item = 0, phys_idx = 0, coff = 0, doff = 0, npos = 0;
        T cur = (T) 0;
        bool bad = false;
        while (w < logical)
        {
            if (has_null)
            {
                if (npos >= nullbits) { bad = true; break; }
                int nbit = (nbmp[npos >> 3] >> (npos & 7)) & 1;
                npos++;
                if (nbit)
                {
                    dst[w] = (T) 0;
                    vdst[w] = 0;
                    w++;
                    continue;
                }
            }
            if ((rle && item >= bmbits) || (delta && item >= dbmbits))
            { bad = true; break; }
            int64_t reps = 1;
            if (rle && (bmp[item >> 3] & (1u << (item & 7))))
            {
                int32_t n = (cnts[coff] >> 6) + 1;
                uint32_t v = cnts[coff] & 0x3F;
                for (int32_t i = 1; i < n; i++) v = (v << 8) | cnts[coff + i];
                coff += n;
                reps += v;
            }
            if (delta && (dbm[item >> 3] & (1u << (item & 7))))
            {
                int32_t n = (dbs[doff] >> 6) + 1;
                bool pos = (dbs[doff] >> 5) & 1;
                uint64_t mag = dbs[doff] & 0x1F;
                for (int32_t i = 1; i < n; i++) mag = (mag << 8) | dbs[doff + i];
                doff += n;
                if constexpr (sizeof(T) == 8)
                    cur = (T) (pos ? (uint64_t) cur + mag : (uint64_t) cur - mag);
                else
                    cur = (T) (pos ? (uint32_t) cur + (uint32_t) mag
                                   : (uint32_t) cur - (uint32_t) mag);
            }
            else
            {
                if (phys_idx >= phys) { bad = true; break; }
                cur = datum[phys_idx++];
            }
            if (w + reps > logical) { bad = true; break; }
            for (int64_t r = 0; r < reps; r++) dst[w + r] = cur;
            if (vdst)
                for (int64_t r = 0; r < reps; r++) vdst[w + r] = 1;
            w += reps;
            item++;
        }
        if (bad || w != logical || phys_idx != phys ||
            (rle && coff != csize) || (delta && doff != dsize) ||
            (has_null && npos != nullbits))
            atomicOr(err, 1);
    }
}

/* ================= Motion routing ================= */

__global__ void k_route(const int64_t *keys, int64_t n, int32_t nsegs, int32_t *out)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (; i < n; i += stride)
        out[i] = gx_route_i64(keys[i], nsegs);
}

/* multi-column distribution keys (cdbhash.c:189-247 rotate-combine loop):
 * row-major vals/isnull, per-key type tags in constant-ish arg memory */
__global__ void k_route_multi(const int64_t *vals, const uint8_t *isnull,
                              const int32_t *types, int32_t nkeys, int64_t n,
                              int32_t nsegs, int32_t *out)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (; i < n; i += stride)
        out[i] = gx_jump_consistent_hash(
            (uint64_t) gx_cdbhash_multi(vals + i * nkeys,
                                        isnull ? isnull + i * nkeys : nullptr,
                                        types, nkeys),
            nsegs);
}

/* Hash GROUP BY with the reference's grouping semantics (nodeAgg.c:2288 +
 * execGrouping.c:436-495): group keys compare NOT DISTINCT, so ALL NULL
 * keys land in ONE group; SUM's transition fn is strict (skips NULL
 * inputs, float.c:769) while COUNT(*) counts every row.  Keys are stored
 * biased (k ^ 2^63) so slot 0 stays the empty sentinel for any int64 key
 * except INT64_MIN (rejected with an error flag). */
__global__ void k_groupby(const uint8_t *k_s, gx_colmeta k_m,
                          const uint8_t *k_val,
                          const uint8_t *v_s, gx_colmeta v_m,
                          const uint8_t *v_val,
                          const uint8_t *vmap,
                          unsigned long long *tkey, double *tsum,
                          unsigned long long *tcnt, uint64_t tmask,
                          double *null_sum, unsigned long long *null_cnt,
                          int *err)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (; i < k_m.nrows; i += stride)
    {
        if (gx_vm_hidden(vmap, i)) continue;
        bool vnull = v_val && !v_val[i];
        double v = vnull ? 0.0 : gx_col_get<double>(v_s, v_m, i);
        if (k_val && !k_val[i])
        {
            /* NULLs-equal grouping: one shared group */
            if (!vnull) atomicAdd(null_sum, v);
            atomicAdd(null_cnt, 1ULL);
            continue;
        }
        uint64_t bk = (uint64_t) gx_col_get<int64_t>(k_s, k_m, i) ^
                      (1ULL << 63);
        if (bk == 0) { atomicOr(err, 4); continue; }
        uint64_t slot = gx_hmix64(bk) & tmask;
        while (true)
        {
            unsigned long long prev = atomicCAS(&tkey[slot], 0ULL, bk);
            if (prev == 0ULL || prev == bk) break;
            slot = (slot + 1) & tmask;
        }
        if (!vnull) atomicAdd(&tsum[slot], v);
        atomicAdd(&tcnt[slot], 1ULL);
    }
}

/* ================= Q3 kernels ================= */

/* Join-table slot mapping.  When the build keys' [min,max] stats admit it
 * (detected at sizing), use an ORDER-PRESERVING interpolation map:
 * slot0 = (key-kmin)*scale.  TPC-H lineitem is clustered by l_orderkey
 * (the reference's own table order, tpch500GB.sql:83), so consecutive
 * probes then touch adjacent slots — cache lines instead of random L3
 * round-trips.  Falls back to the multiplicative hash for sparse/skewed
 * ranges.  Bucket choice is parity-irrelevant: the table is
 * still an exact-key open-addressing hash join table. */
struct gx_slotmap {
    uint64_t mask;
    int64_t kmin;
    double scale;          /* tslots / (range+1); <0 ⇒ use hmix */
    __host__ __device__ __forceinline__ uint64_t slot0(uint64_t k) const
    {
        if (scale < 0.0)
            return gx_hmix64(k) & mask;
        uint64_t s = (uint64_t) ((double) (int64_t) (k - (uint64_t) kmin) * scale);
        return s > mask ? mask : s;
    }
};

/* Dimension membership has two forms, chosen once at sizing (gx_q3.dim_bitmap)
 * and compiled in by template parameter, never tested per row:
 *
 * - HASH: a blocked bloom filter in front of an open-addressing key set.
 *   The bloom is the GPU counterpart of the reference's runtime filter
 *   pushdown (nodeRuntimeFilter.c, CreateRuntimeFilter nodeHashjoin.c:2297,
 *   consumed nodeSeqscan.c:83-116): one 64-bit word per key carries two bits,
 *   so a negative costs a single load instead of an open-addressing walk.
 *   Always used by the Motion path, whose destination prefilter all-gathers
 *   the bloom.
 * - BITMAP: one bit per key of [kmin, kmin+range), for dense (sequence) keys.
 *   Exact, so there is no second structure, no hash and no walk: a lookup is
 *   one load from an array that is 1.9 MB at SF100 against 4 MB of bloom plus
 *   32 MB of set (profiles/dimbitmap_kernels.txt). */
struct gx_dimbits {
    const unsigned long long *bits;    /* ceil(range/64) words */
    uint64_t kmin;
    uint64_t range;                    /* kmax - kmin + 1 */
};

/* Set the bits of one wave's qualifying keys.  Dimension rows commonly
 * arrive in key order, so the lanes of a wave share one or two words: lanes
 * with the same word OR their bits together and the first of them issues ONE
 * atomic.  Correct for any row order and for duplicate keys (a lone lane
 * just issues its own atomic).  Every lane of the wave must call this.
 * Measured at SF100: customer stage 0.08 ms, against 0.15 ms with one plain
 * atomicOr per key and 0.30 ms for bloom + CAS inserts
 * (profiles/dimbitmap_kernels.txt).
 * STRIDE is the distance between bit words in 8-byte units: 1 for a plain
 * bitmap, 2 for the rank table's interleaved {bits, base} entries. */
template <int STRIDE = 1>
__device__ __forceinline__ void d_dimbits_set_wave(unsigned long long *bits,
                                                   uint64_t kmin, uint64_t range,
                                                   bool act, uint64_t k)
{
    uint64_t d = k - kmin;
    act = act && d < range;            /* never write outside the allocation */
    unsigned long long w = d >> 6;
    unsigned long long bit = 1ULL << (d & 63);
    int lane = (int) (threadIdx.x & 63);
    unsigned long long todo = __ballot(act);
    while (todo)
    {
        int lead = __ffsll((long long) todo) - 1;
        unsigned long long w0 = __shfl(w, lead, 64);
        bool same = ((todo >> lane) & 1ULL) && w == w0;
        unsigned long long grp = __ballot(same);
        unsigned long long v = same ? bit : 0ULL;
        if (grp & (grp - 1))           /* more than one lane: OR-reduce */
            for (int o = 32; o; o >>= 1)
                v |= __shfl_xor(v, o, 64);
        if (lane == lead)
            atomicOr(&bits[w0 * STRIDE], v);
        todo &= ~grp;
    }
}

/* Rank-addressed join/agg table for dense mid keys (the local f64 path):
 * one bit per key of [kmin, kmin+range) and, per 64-bit word, the number of
 * set bits in all words before it.  rank(k) = base[word] + popcount of the
 * word's bits below k's is then a dense, collision-free group index in
 * [0, distinct keys): a lookup is one load and no walk, and the payload
 * arrays hold `qual` slots instead of 3 x qual hashed ones.
 * The two sit interleaved in 16-byte entries {u64 bits; u64 base}, one load;
 * separate bits[] and u32 base[] arrays (two independent loads, 12 B per
 * word) measured 0.01-0.02 ms slower in the probe
 * (profiles/rank_table_kernels.txt).
 * qual is the number of payload slots: an index at or past it is a miss, so
 * input that changed after sizing can drop rows but never leaves an
 * allocation. */
struct gx_rankview {
    const ulonglong2 *ent;             /* ceil(range/64) x {bits, base} */
    uint64_t kmin, range, qual;
};

/* words of one block of the prefix-popcount scan (k_rank_*), 8 per thread */
static constexpr int GX_RANK_SCAN_WORDS = 8 * TPB;

/* dense index of key k, or ~0ULL when k is not in the table */
__device__ __forceinline__ uint64_t d_rank_find(const gx_rankview &rv, uint64_t k)
{
    uint64_t d = k - rv.kmin;          /* k < kmin wraps to d >= range */
    if (d >= rv.range) return ~0ULL;
    ulonglong2 e = rv.ent[d >> 6];
    int sh = (int) (d & 63);
    uint64_t idx = e.y + (uint64_t) __popcll(e.x & ((1ULL << sh) - 1ULL));
    return (((e.x >> sh) & 1ULL) && idx < rv.qual) ? idx : ~0ULL;
}

/* the bloom half of the HASH form */
__device__ __forceinline__ unsigned long long d_bloom_mask_of(uint64_t h)
{
    int b1 = (int) ((h >> 32) & 63);
    int b2 = (int) ((h >> 38) & 63);
    return (1ULL << b1) | (1ULL << b2);
}

__device__ __forceinline__ void d_bloom_set(unsigned long long *bloom,
                                            uint64_t wmask, uint64_t k)
{
    uint64_t h = gx_hmix64(k);
    atomicOr(&bloom[h & wmask], d_bloom_mask_of(h));
}

__device__ __forceinline__ bool d_bloom_test(const unsigned long long *bloom,
                                             uint64_t wmask, uint64_t k)
{
    uint64_t h = gx_hmix64(k);
    unsigned long long m = d_bloom_mask_of(h);
    return (bloom[h & wmask] & m) == m;
}

/* wave-aggregated counter add: ONE atomic per 64-lane wave (G12) */
__device__ __forceinline__ void gx_wave_count_add(unsigned long long *dst,
                                                  unsigned long long v)
{
    for (int o = 32; o; o >>= 1)
        v += __shfl_down((unsigned long long) v, o, 64);
    if ((threadIdx.x & 63) == 0 && v)
        atomicAdd(dst, v);
}

/* wave min/max of unsigned keys, then ONE atomicMax/atomicMin per wave.
 * GUARD skips a wave that saw no key (kmax still 0 / kmin still ~0);
 * k_col_minmax alone commits unconditionally, as it always has. */
template <bool GUARD = true>
__device__ __forceinline__ void d_wave_minmax_commit(unsigned long long kmax,
                                                     unsigned long long kmin,
                                                     unsigned long long *maxkey,
                                                     unsigned long long *minkey)
{
    for (int o = 32; o; o >>= 1)
    {
        unsigned long long v = __shfl_down(kmax, o, 64);
        if (v > kmax) kmax = v;
        unsigned long long w = __shfl_down(kmin, o, 64);
        if (w < kmin) kmin = w;
    }
    if ((threadIdx.x & 63) == 0)
    {
        if (!GUARD || kmax) atomicMax(maxkey, kmax);
        if (!GUARD || kmin != ~0ULL) atomicMin(minkey, kmin);
    }
}

/* Probe walk over an open-addressing key array (empty slot = 0), continuing
 * from a first slot whose word v the caller has already loaded.  Returns the
 * slot that holds k, or ~0ULL when k is absent.  The compare ZERO-EXTENDS
 * the stored key, so in u32 mode a probe key >= 2^32 never matches —
 * width-safe without a hot-loop branch (a per-row guard here measured +57%,
 * the r1 visimap lesson). */
template <typename KT>
__device__ __forceinline__ uint64_t d_table_find(const KT *tkey, uint64_t tmask,
                                                 uint64_t slot, KT v, uint64_t k)
{
    while (true)
    {
        if (v == (KT) 0) return ~0ULL;
        if ((uint64_t) v == k) return slot;
        slot = (slot + 1) & tmask;
        v = tkey[slot];
    }
}

/* The same walk for callers that have not loaded the first word: leaves the
 * slot that holds k in `slot` and returns whether k is there.  Kept beside
 * d_table_find on purpose: calling that one from k_li_probe_agg_num and
 * k_li_probe_agg_rle compiles their loops differently (fewer SGPRs/VGPRs, one
 * occupancy step, profiles/refactor_kernel_resources.txt), and the numeric
 * probe has no benchmark leg that could show such a change costs nothing. */
template <typename KT>
__device__ __forceinline__ bool d_table_find_from(const KT *tkey, uint64_t tmask,
                                                  uint64_t &slot, uint64_t k)
{
    bool found = false;
    while (true)
    {
        KT v = tkey[slot];
        if (v == (KT) 0) break;
        if ((uint64_t) v == k) { found = true; break; }  /* zext */
        slot = (slot + 1) & tmask;
    }
    return found;
}

/* insert k into an open-addressing key set (empty slot = 0; duplicates
 * collapse) */
template <typename KS>
__device__ __forceinline__ void d_set_insert(KS *set, uint64_t mask, uint64_t k)
{
    uint64_t slot = gx_hmix64(k) & mask;
    while (true)
    {
        KS prev = atomicCAS(&set[slot], (KS) 0, (KS) k);
        if (prev == (KS) 0 || prev == (KS) k) break;
        slot = (slot + 1) & mask;
    }
}

/* LEFT OUTER (HJ_FILL_OUTER): claim the slot of unmatched fact key k in the
 * second table.  Keys are stored biased (k ^ 2^63) so 0 stays the empty
 * mark; NULL fact keys (decoded 0) coalesce into one group.  Returns the
 * slot. */
__device__ __forceinline__ uint64_t d_unmatched_claim(unsigned long long *ukey,
                                                      uint64_t umask, uint64_t k)
{
    uint64_t bk = k ^ (1ULL << 63);
    uint64_t slot = gx_hmix64(bk) & umask;
    while (true)
    {
        unsigned long long prev = atomicCAS(&ukey[slot], 0ULL, bk);
        if (prev == 0ULL || prev == bk) break;
        slot = (slot + 1) & umask;
    }
    return slot;
}

/* Block exclusive scan of n values into out[0..n): thread t scans the
 * contiguous chunk [t*C, (t+1)*C) serially (val(i) is read before out[i] is
 * written, so val may read out itself), the per-thread sums are scanned by
 * thread 0 through s_part[blockDim.x], and the bases are added back.  The
 * grand total is stored to *total (when given) by thread 0 before the
 * second barrier.  Three __syncthreads; every thread of the block calls. */
template <typename F>
__device__ __forceinline__ void d_block_excl_scan(uint32_t *out, int n,
                                                  uint32_t *s_part,
                                                  uint32_t *total, F val)
{
    int C = (n + blockDim.x - 1) / blockDim.x;
    int lo = threadIdx.x * C, hi = min(lo + C, n);
    uint32_t acc = 0;
    for (int i = lo; i < hi; i++)
    {
        uint32_t v = val(i);
        out[i] = acc;
        acc += v;
    }
    s_part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        uint32_t run = 0;
        for (int t = 0; t < (int) blockDim.x; t++)
        {
            uint32_t v = s_part[t];
            s_part[t] = run;
            run += v;
        }
        if (total) *total = run;
    }
    __syncthreads();
    uint32_t base = s_part[threadIdx.x];
    for (int i = lo; i < hi; i++)
        out[i] += base;
    __syncthreads();
}

/* Standalone columnar scan + filter (BASELINE config 2; the SeqScan+qual
 * slice without a join): count rows of one column passing <op, literal>.
 * op: the six gx_filter ops (gx_cmp); three-valued logic degenerates to
 * two-valued on NOT NULL columns (execScan.c:241). */
template <typename T>
__global__ void k_scan_filter(const uint8_t *col_s, gx_colmeta m,
                              const uint8_t *vmap,
                              int op, T lit, unsigned long long *count)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    unsigned long long local = 0;
    for (; i < m.nrows; i += stride)
    {
        if (gx_vm_hidden(vmap, i)) continue;
        T v = gx_col_get<T>(col_s, m, i);
        if (gx_cmp<T>(op, v, lit)) local++;
    }
    gx_wave_count_add(count, local);
}

/* TEXT dim predicate (texteq on a varlena RLE column — the reference's
 * actual Q3 qual c_mktsegment = 'BUILDING', execQual over text).  One
 * THREAD per varlena AO block; with rle_type segments the comparison runs
 * ONCE PER RUN, the run's rows then stream through.  NOT NULL scope. */
__device__ __forceinline__ bool d_texteq(const uint8_t *a, int64_t alen,
                                         const uint8_t *b, int64_t blen)
{
    if (alen != blen) return false;
    for (int64_t i = 0; i < alen; i++)
        if (a[i] != b[i]) return false;
    return true;
}

/* texteq over a decoded varlena column (device offsets+payload) → one
 * match byte per row.  Runs ONCE at prepare: a constant predicate over an
 * immutable column is evaluated once and cached, the per-step scans then
 * read the mask on the fast fixed-width path (what dictionary-aware
 * executors do for constant text quals). */
__global__ void k_texteq_mask(const int64_t *offsets, const uint8_t *payload,
                              int64_t n, const uint8_t *lit, int32_t lit_len,
                              uint8_t *mask)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (; i < n; i += stride)
    {
        int64_t len = offsets[i + 1] - offsets[i];
        mask[i] = (uint8_t) d_texteq(payload + offsets[i], len, lit, lit_len);
    }
}

/* AND-ed extra qual lists (execScan.c:241: every qual in the list must
 * pass; three-valued logic degenerates to two-valued on NOT NULL columns).
 * Folded ONCE at prepare into a per-table HIDDEN bitmap (same encoding as
 * the AO visimap, OR-combined with it), which every scan/build/probe
 * kernel already honors through its visibility parameter. */
struct gx_qualargs {
    int32_t n;
    const uint8_t *s[GX_MAX_EXTRA_QUALS];
    gx_colmeta m[GX_MAX_EXTRA_QUALS];
    int32_t op[GX_MAX_EXTRA_QUALS];
    int64_t lit[GX_MAX_EXTRA_QUALS];
};

__global__ void k_qualmask(gx_qualargs qa, const uint8_t *vmap, int64_t nrows,
                           uint8_t *hidden)
{
    int64_t nbytes = (nrows + 7) >> 3;
    int64_t b = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (; b < nbytes; b += stride)
    {
        uint8_t h = vmap ? vmap[b] : 0;
        int64_t row0 = b << 3;
        int lim = (int) min((int64_t) 8, nrows - row0);
        for (int r = 0; r < lim; r++)
        {
            int64_t i = row0 + r;
            bool pass = true;
            for (int qn = 0; qn < qa.n && pass; qn++)
            {
                int64_t v;
                switch (qa.m[qn].width)
                {
                    case 1: v = gx_col_get<int8_t>(qa.s[qn], qa.m[qn], i); break;
                    case 4: v = gx_col_get<int32_t>(qa.s[qn], qa.m[qn], i); break;
                    default: v = gx_col_get<int64_t>(qa.s[qn], qa.m[qn], i); break;
                }
                pass = gx_cmp(qa.op[qn], v, qa.lit[qn]);
            }
            if (!pass) h |= (uint8_t) (1u << r);
        }
        hidden[b] = h;
    }
}

/* OR rows with validity==0 into a hidden bitmap: strict-NULL reject for
 * join keys (nodeHash.c:2168-2181 — a NULL key cannot pass a strict hash
 * operator on either side of an inner join) and three-valued filter
 * semantics for qual columns (execScan.c:241 — a NULL qual result filters
 * the row) */
__global__ void k_validity_or_hidden(const uint8_t *validity, int64_t nrows,
                                     uint8_t *hidden)
{
    int64_t nbytes = (nrows + 7) >> 3;
    int64_t b = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (; b < nbytes; b += stride)
    {
        uint8_t h = 0;
        int64_t row0 = b << 3;
        int lim = (int) min((int64_t) 8, nrows - row0);
        for (int r = 0; r < lim; r++)
            if (!validity[row0 + r]) h |= (uint8_t) (1u << r);
        if (h) hidden[b] |= h;
    }
}

/* Constant texteq evaluated DIRECTLY over varlena AO blocks, one compare
 * per PHYSICAL datum (i.e. once per RLE run — what a dictionary-aware
 * executor does), mask bytes fanned out over the run's rows.  Replaces
 * the decode-whole-column-then-compare prepare path (r2: the SF100
 * prepare cost was dominated by the payload materialization).  NULL
 * datums fail the qual (three-valued texteq). */
__global__ void k_texteq_mask_blocks(const uint8_t *stream,
                                     const gx_blockref *dir, int64_t nblocks,
                                     int64_t nrows, const uint8_t *lit,
                                     int32_t lit_len, uint8_t *mask, int *err)
{
    int64_t t = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    for (int64_t b = t; b < nblocks; b += gridDim.x * (int64_t) blockDim.x)
    {
        const uint8_t *c = stream + dir[b].offset + 24;
        int16_t version = ((const int16_t *) c)[0];
        int16_t flags = ((const int16_t *) c)[1];
        int32_t logical = dir[b].rows;
        if ((version != 0 && version != 1 && version != 2) ||
            dir[b].first_row + logical > nrows || (flags & 4))
        { atomicOr(err, 1); continue; }
        bool rle = false;
        const uint8_t *nbmp = nullptr, *bmp = nullptr, *cnts = nullptr;
        int32_t bmbits = 0, csize = 0, nullbits = 0, psize = 0;
        const uint8_t *p0;
        if (version == 0)
        {
            int16_t nd = ((const int16_t *) c)[2];
            int32_t nullsz = ((const int32_t *) c)[2];
            psize = ((const int32_t *) c)[3];
            if (nd != logical) { atomicOr(err, 1); continue; }
            nullbits = (flags & 1) ? logical : 0;
            nbmp = c + 16;
            p0 = c + 16 + nullsz;
        }
        else
        {
            int32_t hlogical = ((const int32_t *) c)[1];
            psize = ((const int32_t *) c)[3];
            if (hlogical != logical) { atomicOr(err, 1); continue; }
            rle = (flags & 2) != 0;
            const uint8_t *q = c + 16;
            nullbits = (flags & 1) ? logical : 0;
            if (rle)
            {
                int32_t norepeats = ((const int32_t *) q)[0];
                bmbits = ((const int32_t *) q)[1];
                csize = ((const int32_t *) q)[3];
                if (flags & 1) nullbits = norepeats;
                else if (norepeats != 0) { atomicOr(err, 1); continue; }
                q += 16;
            }
            if (flags & 1) { nbmp = q; q += (nullbits + 7) >> 3; }
            if (rle) { bmp = q; q += (bmbits + 7) >> 3; cnts = q; q += csize; }
            int32_t hdr = (int32_t) (q - c);
            p0 = c + ((hdr + 7) & ~7);
        }
        const uint8_t *p = p0, *pend = p0 + psize;
        int64_t out = 0;
        int32_t item = 0, coff = 0, npos = 0;
        bool bad = false;
        while (out < logical)
        {
            int64_t row = dir[b].first_row + out;
            if (nbmp != nullptr && nullbits > 0)
            {
                if (npos >= nullbits) { bad = true; break; }
                int nb = (nbmp[npos >> 3] >> (npos & 7)) & 1;
                npos++;
                if (nb)
                {
                    mask[row] = 0;          /* NULL fails the qual */
                    out++;
                    continue;
                }
            }
            if (rle && item >= bmbits) { bad = true; break; }
            if (p < pend && *p == 0)
                p = p0 + (((p - p0) + 3) & ~(int64_t) 3);
            if (p >= pend) { bad = true; break; }
            int64_t len;
            const uint8_t *data;
            if (*p & 1)
            {
                len = (int64_t) (*p >> 1) - 1;
                data = p + 1;
                p += 1 + len;
            }
            else
            {
                uint32_t hdr;
                memcpy(&hdr, p, 4);
                len = (int64_t) (hdr >> 2) - 4;
                data = p + 4;
                p += 4 + len;
            }
            if (len < 0 || p > pend) { bad = true; break; }
            /* ONE compare per physical datum (per run) */
            uint8_t m = (uint8_t) d_texteq(data, len, lit, lit_len);
            int64_t reps = 1;
            if (rle && (bmp[item >> 3] & (1u << (item & 7))))
            {
                int32_t nn = (cnts[coff] >> 6) + 1;
                uint32_t v = cnts[coff] & 0x3F;
                for (int32_t i = 1; i < nn; i++) v = (v << 8) | cnts[coff + i];
                coff += nn;
                reps += v;
            }
            if (out + reps > logical) { bad = true; break; }
            for (int64_t rr = 0; rr < reps; rr++)
            {
                mask[dir[b].first_row + out] = m;
                out++;
            }
            item++;
        }
        if (bad || (rle && (coff != csize || item != bmbits)))
            atomicOr(err, 1);
    }
}

/* The dimension row predicate of the customer scans, in the two forms
 * prepare can choose: a flat per-row mask (built once by k_texteq_mask for a
 * text qual) or an int8 column compare (mktsegment = BUILDING). */
struct gx_dim_pred_mask {
    const uint8_t *mask;
    __device__ __forceinline__ bool operator()(int64_t i) const
    {
        return mask[i] != 0;
    }
};

struct gx_dim_pred_cmp {
    const uint8_t *mkt_s;
    gx_colmeta mkt_m;
    int cop;
    int8_t clit;
    __device__ __forceinline__ bool operator()(int64_t i) const
    {
        return gx_cmp(cop, gx_col_get<int8_t>(mkt_s, mkt_m, i), clit);
    }
};

/* customer: count qualifying rows and their key range (for set sizing) */
template <typename PRED>
__global__ void k_cust_count(const uint8_t *key_s, gx_colmeta key_m,
                             PRED pred, const uint8_t *vmap,
                             unsigned long long *count,
                             unsigned long long *maxkey,
                             unsigned long long *minkey)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    unsigned long long local = 0, kmax = 0, kmin = ~0ULL;
    for (; i < key_m.nrows; i += stride)
        if (!gx_vm_hidden(vmap, i) && pred(i))
        {
            local++;
            unsigned long long k = (unsigned long long)
                gx_col_get<int64_t>(key_s, key_m, i);
            if (k > kmax) kmax = k;
            if (k < kmin) kmin = k;
        }
    gx_wave_count_add(count, local);
    d_wave_minmax_commit(kmax, kmin, maxkey, minkey);
}

/* customer: record the c_custkey of every qualifying row in the dimension
 * membership structure: its bit of the bitmap (BM), or bloom + open set.
 * Replaces the build side of the cust⋈orders join (nodeHash.c:1886). */
template <typename KS, bool BM, typename PRED>
__global__ void k_cust_build(const uint8_t *key_s, gx_colmeta key_m,
                             PRED pred, const uint8_t *vmap,
                             KS *set, uint64_t mask,
                             unsigned long long *bloom, uint64_t bwmask,
                             unsigned long long *bits, uint64_t kmin,
                             uint64_t range)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    if constexpr (BM)
    {
        /* bitmap form: whole waves iterate together (d_dimbits_set_wave) */
        for (int64_t base = i - (threadIdx.x & 63); base < key_m.nrows;
             base += stride)
        {
            int64_t r = base + (threadIdx.x & 63);
            bool act = r < key_m.nrows && !gx_vm_hidden(vmap, r) && pred(r);
            uint64_t k = act ? (uint64_t) gx_col_get<int64_t>(key_s, key_m, r) : 0;
            d_dimbits_set_wave(bits, kmin, range, act, k);
        }
        return;
    }
    for (; i < key_m.nrows; i += stride)
    {
        if (gx_vm_hidden(vmap, i) || !pred(i)) continue;
        uint64_t k = (uint64_t) gx_col_get<int64_t>(key_s, key_m, i);
        d_bloom_set(bloom, bwmask, k);
        d_set_insert(set, mask, k);
    }
}

template <typename KS>
__device__ __forceinline__ bool d_set_contains(const KS *set,
                                               uint64_t mask, uint64_t k)
{
    /* u32 slots hold only resident keys < 2^32 (sizing max); the compare
     * zero-extends the stored key so a wider probe key never matches */
    uint64_t slot = gx_hmix64(k) & mask;
    while (true)
    {
        KS v = set[slot];
        if (v == (KS) 0) return false;
        if ((uint64_t) v == k) return true;   /* zext compare: width-safe */
        slot = (slot + 1) & mask;
    }
}

/* dimension membership of fk k in the form the caller was compiled for.
 * BITMAP: the unsigned subtraction puts every k < kmin (0 and negative fks
 * included) and every k > kmax at d >= range, so nothing outside the
 * ceil(range/64) allocated words is ever read. */
template <bool BM, typename KS>
__device__ __forceinline__ bool d_dim_contains(const KS *set, uint64_t cmask,
                                               const unsigned long long *bloom,
                                               uint64_t bwmask,
                                               const gx_dimbits &bm, uint64_t k)
{
    if constexpr (BM)
    {
        uint64_t d = k - bm.kmin;
        return d < bm.range && ((bm.bits[d >> 6] >> (d & 63)) & 1ULL);
    }
    else
        return d_bloom_test(bloom, bwmask, k) && d_set_contains(set, cmask, k);
}

/* orders local path: count qualifying rows (date filter + dim semi/anti
 * join; ANTI = JOIN_LASJ/LASJ_NOTIN — keep rows whose fk is NOT in the
 * set, nodeHashjoin.c:652-659) */
template <typename KS, bool ANTI = false, bool BM = false>
__global__ void k_orders_count(const uint8_t *ok_s, gx_colmeta ok_m,
                               const uint8_t *od_s, gx_colmeta od_m,
                               const uint8_t *oc_s, gx_colmeta oc_m,
                               const uint8_t *vmap, int oop, int32_t olit,
                               const KS *cset, uint64_t cmask,
                               const unsigned long long *bloom, uint64_t bwmask,
                               gx_dimbits bm,
                               unsigned long long *count,
                               unsigned long long *maxkey,
                               unsigned long long *minkey)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    unsigned long long local = 0, kmax = 0, kmin = ~0ULL;
    for (; i < od_m.nrows; i += stride)
    {
        if (gx_vm_hidden(vmap, i)) continue;
        if (!gx_cmp(oop, gx_col_get<int32_t>(od_s, od_m, i), olit)) continue;
        uint64_t ck = (uint64_t) gx_col_get<int64_t>(oc_s, oc_m, i);
        bool in_set = d_dim_contains<BM>(cset, cmask, bloom, bwmask, bm, ck);
        if (in_set == ANTI) continue;
        local++;
        unsigned long long k = (unsigned long long) gx_col_get<int64_t>(ok_s, ok_m, i);
        if (k > kmax) kmax = k;
        if (k < kmin) kmin = k;
    }
    gx_wave_count_add(count, local);
    d_wave_minmax_commit(kmax, kmin, maxkey, minkey);
}

/* Join/agg table payload, beside the SoA key array tkey[]: one 16-byte
 * aggregation slot and one 8-byte attr pair per table slot.
 *
 * NEITHER ARRAY IS CLEARED PER RUN.  Only tkey[] is memset; the build thread
 * whose CAS claims a slot stores the attr pair and one 16-byte zero to the
 * agg slot.  Slots whose key is 0 therefore hold garbage (a previous run's
 * sums, or whatever hipMalloc returned) BY DESIGN: every reader must gate on
 * tkey[slot] != 0 before touching tagg[slot] / tattr[slot].
 *
 * f64 mode: {double sum; double cnt} — the count is an f64 everywhere
 * (exact below 2^53; extract converts it to int64).  numeric mode: the same
 * 16 bytes viewed as {u64 numerator; u64 cnt} (gx_aggslot_num). */
struct alignas(16) gx_aggslot { double sum; double cnt; };
struct alignas(16) gx_aggslot_num { unsigned long long sum; unsigned long long cnt; };
struct alignas(8) gx_attrpair { int32_t attr1; int32_t attr2; };
static_assert(sizeof(gx_aggslot) == 16 && sizeof(gx_aggslot_num) == 16 &&
              sizeof(gx_attrpair) == 8, "table payload layout");

/* claim-time init of a freshly CAS-won slot: one 8-B and one 16-B store
 * (all-zero bits are 0.0 and 0ULL alike, so both modes share it) */
__device__ __forceinline__ void d_slot_claim(gx_attrpair *tattr, gx_aggslot *tagg,
                                             uint64_t slot, int32_t a1, int32_t a2)
{
    *reinterpret_cast<int2 *>(&tattr[slot]) = make_int2(a1, a2);
    *reinterpret_cast<ulonglong2 *>(&tagg[slot]) = make_ulonglong2(0ULL, 0ULL);
}

/* orders local path: build the join/agg table keyed by o_orderkey.
 * (ExecHashTableInsert nodeHash.c:1886; o_orderkey unique → 1 entry/key;
 *  payload doubles as the agg group state, nodeAgg.c group = join row) */
/* KT = u32 when every qualifying o_orderkey < 2^32 (detected at sizing; the
 * key array then sits comfortably in the 256 MiB Infinity Cache), u64
 * otherwise.  Key compares stay exact either way (PG narrow-int hashing
 * spirit; sentinel 0 is safe — orderkeys start at 1). */
template <typename KT, typename KS, bool VM = false, bool ANTI = false,
          bool BM = false>
__global__ void k_orders_build(const uint8_t *ok_s, gx_colmeta ok_m,
                               const uint8_t *oc_s, gx_colmeta oc_m,
                               const uint8_t *od_s, gx_colmeta od_m,
                               const uint8_t *op_s, gx_colmeta op_m,
                               const uint8_t *vmap, int oop, int32_t olit,
                               const KS *cset, uint64_t cmask,
                               const unsigned long long *bloom, uint64_t bwmask,
                               gx_dimbits bm,
                               KT *tkey,
                               gx_attrpair *tattr, gx_aggslot *tagg,
                               gx_slotmap smap)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    uint64_t tmask = smap.mask;
    for (; i < ok_m.nrows; i += stride)
    {
        if constexpr (VM)
            if (gx_vm_hidden(vmap, i)) continue;
        int32_t od;
        uint64_t ck, k;
        if constexpr (BM)
        {
            /* bitmap form: the fk is loaded beside the date, not after the
             * date test (about half the rows pass, so every sector of the
             * column is fetched anyway: one dependent latency less), and
             * the three streamed columns load non-temporally so they do not
             * push the bitmap out of L2.  At SF100 the stage went 1.66-1.69
             * -> 1.60-1.61 -> 1.56 ms with the two steps
             * (profiles/dimbitmap_kernels.txt).  The hash form is as it
             * was. */
            od = gx_col_get_nt<int32_t>(od_s, od_m, i);
            ck = (uint64_t) gx_col_get_nt<int64_t>(oc_s, oc_m, i);
            if (!gx_cmp(oop, od, olit)) continue;
        }
        else
        {
            od = gx_col_get<int32_t>(od_s, od_m, i);
            if (!gx_cmp(oop, od, olit)) continue;
            ck = (uint64_t) gx_col_get<int64_t>(oc_s, oc_m, i);
        }
        bool in_set = d_dim_contains<BM>(cset, cmask, bloom, bwmask, bm, ck);
        if (in_set == ANTI) continue;
        if constexpr (BM)
            k = (uint64_t) gx_col_get_nt<int64_t>(ok_s, ok_m, i);
        else
            k = (uint64_t) gx_col_get<int64_t>(ok_s, ok_m, i);
        uint64_t slot = smap.slot0(k);
        while (true)
        {
            KT prev = atomicCAS(&tkey[slot], (KT) 0, (KT) k);
            if (prev == (KT) 0)
            {
                d_slot_claim(tattr, tagg, slot, od,
                             gx_col_get<int32_t>(op_s, op_m, i));
                break;
            }
            if (prev == (KT) k) break;   /* unique keys: no-op */
            slot = (slot + 1) & tmask;
        }
    }
}

/* ---- orders stage in rank form (gx_rankview): mark, prefix popcounts, fill.
 * Replaces k_orders_build when the run uses the rank table.  The stage has
 * two forms, chosen per run by q3_orders_staged from the selectivity sizing
 * measured (GX_ORDERS_STAGED forces one):
 *
 * - two-pass: k_orders_mark writes a per-row mask, and k_orders_fill walks
 *   every mid row again and re-reads key, date and attr2 of the rows whose
 *   mask bit is set.  Wastes little where most rows qualify.
 * - staged: k_orders_mark<STAGE> compacts {key, attr1, attr2} of the
 *   qualifying rows, which it has in registers when it decides, into a
 *   staging array of local_qual 16-byte records, and k_orders_fill_staged
 *   reads only those.  Where few rows qualify the second walk over three
 *   columns, a third to a half of whose sectors it touched for one lane in
 *   ten, is gone (profiles/orders_stage_kernels.txt). ---- */

/* records one wave collects in LDS before it has to claim staging space
 * (W): 4 waves x 256 x 16 B = 16 KiB per block, 8 blocks per CU */
static constexpr int GX_STAGE_WAVE_RECS = 256;
static_assert(GX_STAGE_WAVE_RECS >= 64, "a segment takes one wave iteration");

/* staging record {u64 key; i32 attr1; i32 attr2}, moved as one ulonglong2 */
__device__ __forceinline__ ulonglong2 d_stage_pack(uint64_t k, int32_t a1, int32_t a2)
{
    return make_ulonglong2(k, (unsigned long long) (uint32_t) a1 |
                                  ((unsigned long long) (uint32_t) a2 << 32));
}

/* Copy n records of this wave's LDS segment to stage[off ..), clamped to the
 * staging capacity: input that changed after sizing drops rows but never
 * leaves the allocation.  Coalesced 16-byte stores.  Every lane calls it. */
__device__ __forceinline__ void d_stage_copy_out(const ulonglong2 *seg, uint32_t n,
                                                 unsigned long long off,
                                                 ulonglong2 *stage, uint64_t cap,
                                                 int lane)
{
    uint64_t o = off < cap ? off : cap;
    uint64_t room = cap - o;
    uint32_t m = (uint64_t) n < room ? n : (uint32_t) room;
    for (uint32_t j = (uint32_t) lane; j < m; j += 64)
        stage[o + j] = seg[j];
}

/* Mark: k_orders_build's filters and dim test; a qualifying row sets its
 * key's bit (d_dimbits_set_wave, so whole waves iterate together: no
 * `continue`, wave-uniform bounds).  blockDim.x must be a multiple of 64.
 *
 * Two-pass form: the wave's qualifying mask goes to rowmask[row / 64] with
 * one plain store — every word of the mask is rewritten each run.  The fill
 * kernel selects rows by that mask, not by the key's bit, so a key on two
 * rows of which one fails the filter keeps the qualifying row's attrs.
 *
 * STAGE form (blockDim.x == TPB): no rowmask.  A qualifying lane also loads
 * attr2 and appends its record to its wave's LDS segment of
 * GX_STAGE_WAVE_RECS records, at the wave's count plus its rank in the
 * ballot; nothing in the row loop waits on another wave.  After the loop the
 * block claims one contiguous staging region with ONE returning atomic on
 * cursor[0] and every wave copies its segment out.  A wave whose segment
 * cannot take an iteration's records first flushes on its own (one claim, a
 * coalesced copy, cursor[1] counts these); the host sizes the grid so that
 * this stays the exception, because same-address atomics cost 6 ms per
 * 500 k (d_wave_claim).  The template flag is compile-time so that the
 * two-pass instantiations are what they were before it existed. */
template <typename KS, bool VM = false, bool ANTI = false, bool BM = false,
          bool STAGE = false>
__global__ void k_orders_mark(const uint8_t *ok_s, gx_colmeta ok_m,
                              const uint8_t *oc_s, gx_colmeta oc_m,
                              const uint8_t *od_s, gx_colmeta od_m,
                              const uint8_t *vmap, int oop, int32_t olit,
                              const KS *cset, uint64_t cmask,
                              const unsigned long long *bloom, uint64_t bwmask,
                              gx_dimbits bm,
                              ulonglong2 *rent, uint64_t kmin,
                              uint64_t range, unsigned long long *rowmask,
                              const uint8_t *op_s, gx_colmeta op_m,
                              ulonglong2 *stage, unsigned long long *cursor,
                              uint64_t cap)
{
    __shared__ ulonglong2 s_rec[STAGE ? (TPB / 64) * GX_STAGE_WAVE_RECS : 1];
    __shared__ uint32_t s_cnt[TPB / 64];
    __shared__ unsigned long long s_off;
    const int lane = (int) (threadIdx.x & 63);
    const int wave = (int) (threadIdx.x >> 6);
    uint32_t wn = 0;                   /* records in this wave's segment */
    int64_t base = blockIdx.x * (int64_t) blockDim.x + threadIdx.x - lane;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (; base < ok_m.nrows; base += stride)
    {
        int64_t r = base + lane;
        bool act = r < ok_m.nrows;
        if constexpr (VM)
            act = act && !gx_vm_hidden(vmap, r);
        uint64_t ck = 0, k = 0;
        int32_t od = 0;
        if constexpr (BM)
        {
            /* early fk load, non-temporal streams: see k_orders_build */
            if (act)
            {
                od = gx_col_get_nt<int32_t>(od_s, od_m, r);
                ck = (uint64_t) gx_col_get_nt<int64_t>(oc_s, oc_m, r);
            }
            act = act && gx_cmp(oop, od, olit);
        }
        else
        {
            if (act) od = gx_col_get<int32_t>(od_s, od_m, r);
            act = act && gx_cmp(oop, od, olit);
            if (act) ck = (uint64_t) gx_col_get<int64_t>(oc_s, oc_m, r);
        }
        if (act)
            act = d_dim_contains<BM>(cset, cmask, bloom, bwmask, bm, ck) != ANTI;
        if (act)
        {
            if constexpr (BM)
                k = (uint64_t) gx_col_get_nt<int64_t>(ok_s, ok_m, r);
            else
                k = (uint64_t) gx_col_get<int64_t>(ok_s, ok_m, r);
        }
        act = act && (k - kmin) < range;
        d_dimbits_set_wave<2>(reinterpret_cast<unsigned long long *>(rent),
                              kmin, range, act, k);
        unsigned long long m = __ballot(act);
        if constexpr (STAGE)
        {
            if (m == 0) continue;          /* wave-uniform */
            ulonglong2 *seg = s_rec + wave * GX_STAGE_WAVE_RECS;
            int32_t a2 = 0;
            if (act)
            {
                if constexpr (BM)
                    a2 = gx_col_get_nt<int32_t>(op_s, op_m, r);
                else
                    a2 = gx_col_get<int32_t>(op_s, op_m, r);
            }
            uint32_t c = (uint32_t) __popcll(m);
            if (wn + c > (uint32_t) GX_STAGE_WAVE_RECS)   /* wave-uniform */
            {
                unsigned long long off = 0;
                if (lane == 0)
                {
                    off = atomicAdd(&cursor[0], (unsigned long long) wn);
                    atomicAdd(&cursor[1], 1ULL);
                }
                off = __shfl(off, 0, 64);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                d_stage_copy_out(seg, wn, off, stage, cap, lane);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                wn = 0;
            }
            if (act)
                seg[wn + (uint32_t) __popcll(m & ((1ULL << lane) - 1ULL))] =
                    d_stage_pack(k, od, a2);
            wn += c;
        }
        else
        {
            if (lane == 0) rowmask[base >> 6] = m;
        }
    }
    if constexpr (STAGE)
    {
        const int nw = (int) (blockDim.x >> 6);
        if (lane == 0) s_cnt[wave] = wn;
        __syncthreads();                   /* counts and segments complete */
        uint32_t before = 0, total = 0;
        for (int w = 0; w < nw; w++)
        {
            uint32_t c = s_cnt[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (threadIdx.x == 0 && total)
            s_off = atomicAdd(&cursor[0], (unsigned long long) total);
        __syncthreads();                   /* the claim, to every wave */
        if (total)
            d_stage_copy_out(s_rec + wave * GX_STAGE_WAVE_RECS, wn,
                             s_off + before, stage, cap, lane);
    }
}

/* Prefix popcounts, three launches and no workgroup waits on another:
 * k_rank_blocksum (set bits of each block of GX_RANK_SCAN_WORDS words),
 * k_rank_topscan (one block: exclusive scan of the block sums in place),
 * k_rank_localscan (per block: exclusive scan of its words + block base). */
__global__ void __launch_bounds__(TPB)
k_rank_blocksum(const ulonglong2 *rent, uint64_t nwords, uint32_t *blk)
{
    __shared__ uint32_t s_w[TPB / 64];
    uint64_t w0 = (uint64_t) blockIdx.x * GX_RANK_SCAN_WORDS;
    uint32_t acc = 0;
    for (int j = threadIdx.x; j < GX_RANK_SCAN_WORDS; j += TPB)
    {
        uint64_t w = w0 + (uint64_t) j;
        if (w < nwords)
            acc += (uint32_t) __popcll(rent[w].x);
    }
    for (int o = 32; o; o >>= 1)
        acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        uint32_t t = 0;
        for (int i = 0; i < TPB / 64; i++) t += s_w[i];
        blk[blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(TPB)
k_rank_topscan(uint32_t *blk, int nblk)
{
    __shared__ uint32_t s_part[TPB];
    d_block_excl_scan(blk, nblk, s_part, nullptr, [&](int i) { return blk[i]; });
}

__global__ void __launch_bounds__(TPB)
k_rank_localscan(ulonglong2 *rent, uint64_t nwords, const uint32_t *blk)
{
    __shared__ uint32_t s_scan[GX_RANK_SCAN_WORDS];
    __shared__ uint32_t s_part[TPB];
    uint64_t w0 = (uint64_t) blockIdx.x * GX_RANK_SCAN_WORDS;
    int n = (nwords - w0 < (uint64_t) GX_RANK_SCAN_WORDS)
                ? (int) (nwords - w0) : GX_RANK_SCAN_WORDS;
    d_block_excl_scan(s_scan, n, s_part, nullptr, [&](int i) {
        return (uint32_t) __popcll(rent[w0 + (uint64_t) i].x);
    });
    uint32_t b0 = blk[blockIdx.x];
    for (int j = threadIdx.x; j < n; j += TPB)
        rent[w0 + (uint64_t) j].y = (unsigned long long) (b0 + s_scan[j]);
}

/* Fill: for the rows the mark kernel kept, store key and attr pair at the
 * key's rank and zero its agg slot (the d_slot_claim idea: no per-run clear
 * of the aggregation array).  Mid rows in key order give consecutive ranks,
 * so a wave's stores are dense.  A duplicate key stores twice to one slot. */
template <typename KT>
__global__ void k_orders_fill(const uint8_t *ok_s, gx_colmeta ok_m,
                              const uint8_t *od_s, gx_colmeta od_m,
                              const uint8_t *op_s, gx_colmeta op_m,
                              const unsigned long long *rowmask, gx_rankview rv,
                              KT *dkey, gx_attrpair *dattr, gx_aggslot *dagg)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (; i < ok_m.nrows; i += stride)
    {
        if (!((rowmask[i >> 6] >> (i & 63)) & 1ULL)) continue;
        uint64_t k = (uint64_t) gx_col_get<int64_t>(ok_s, ok_m, i);
        int32_t a1 = gx_col_get<int32_t>(od_s, od_m, i);
        int32_t a2 = gx_col_get<int32_t>(op_s, op_m, i);
        uint64_t idx = d_rank_find(rv, k);
        if (idx == ~0ULL) continue;
        dkey[idx] = (KT) k;
        d_slot_claim(dattr, dagg, idx, a1, a2);
    }
}

/* Fill of the staged form: the same three stores, driven by the records
 * k_orders_mark<STAGE> compacted instead of a second walk over the mid
 * table.  The record count is what the mark kernel's claims added up to,
 * read from the device cursor (no host sync between mark, scans and fill)
 * and clamped to the staging capacity. */
template <typename KT>
__global__ void k_orders_fill_staged(const ulonglong2 *stage,
                                     const unsigned long long *cursor,
                                     uint64_t cap, gx_rankview rv,
                                     KT *dkey, gx_attrpair *dattr, gx_aggslot *dagg)
{
    unsigned long long have = cursor[0];
    uint64_t n = have < cap ? have : cap;
    uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x;
    uint64_t stride = gridDim.x * (uint64_t) blockDim.x;
    for (; i < n; i += stride)
    {
        ulonglong2 rec = stage[i];
        uint64_t idx = d_rank_find(rv, rec.x);
        if (idx == ~0ULL) continue;
        dkey[idx] = (KT) rec.x;
        d_slot_claim(dattr, dagg, idx, (int32_t) (uint32_t) rec.y,
                     (int32_t) (uint32_t) (rec.y >> 32));
    }
}

/* lineitem probe + aggregate — THE dominant kernel.
 * scan (aocsam.c:1131 semantics) + probe (nodeHashjoin.c:553-652) +
 * SUM transition (nodeAgg.c:836 + float.c:769) fused; build slots ARE the
 * agg groups (group key functionally determined by l_orderkey).
 * One row per thread per grid-stride iteration.  The kernel is latency-bound
 * at full occupancy (PMC: 85% WAIT_ANY, ~300M L3 probe round-trips); every
 * batched, tiled and LDS-staged form measured slower and was removed
 * (DESIGN.md "Measured bandwidth ceiling").
 * The table lookup has two compile-time forms: the open-addressing walk over
 * tkey[] (slot0, then d_table_find), and RANK, one 16-byte load from the rank
 * table (d_rank_find) whose result indexes the dense agg array — what dense
 * mid keys run on the local path.  At SF100 the kernel takes 4.39-4.43 ms in
 * the hash form and 3.79-3.86 ms in the rank form
 * (profiles/rank_table_kernels.txt). */
template <typename KT, bool VM = false, bool OUTER = false, bool RANK = false>
__global__ void k_li_probe_agg_t(const uint8_t *lk_s, gx_colmeta lk_m,
                                 const uint8_t *pr_s, gx_colmeta pr_m,
                                 const uint8_t *di_s, gx_colmeta di_m,
                                 const uint8_t *sh_s, gx_colmeta sh_m,
                                 const uint8_t *vmap, int fop, int32_t flit,
                                 const KT *tkey,
                                 gx_aggslot *tagg,
                                 gx_slotmap smap,
                                 unsigned long long *hits,
                                 /* LEFT OUTER (HJ_FILL_OUTER): unmatched
                                  * fact rows aggregate into a second
                                  * biased-key table; NULL fact keys
                                  * (decoded 0) coalesce into one group */
                                 unsigned long long *ukey = nullptr,
                                 double *urev = nullptr,
                                 unsigned long long *ucnt = nullptr,
                                 uint64_t umask = 0,
                                 /* RANK: the group index is the key's rank in rv and
                                  * tagg the dense agg array; tkey and smap
                                  * are not read.  Trailing, so the hash
                                  * forms never load it. */
                                 gx_rankview rv = {})
{
    uint64_t tmask = smap.mask;
    unsigned long long local_hits = 0;
    auto umiss = [&](uint64_t k, int64_t i) {
        if constexpr (OUTER)
        {
            uint64_t slot = d_unmatched_claim(ukey, umask, k);
            double price = gx_col_get<double>(pr_s, pr_m, i);
            double disc = gx_col_get<double>(di_s, di_m, i);
            atomicAdd(&urev[slot], price * (1.0 - disc));
            atomicAdd(&ucnt[slot], 1ULL);
        }
        else
        {
            (void) k; (void) i;
        }
    };
    auto hit = [&](uint64_t slot, int64_t i) {
        double price = gx_col_get<double>(pr_s, pr_m, i);
        double disc = gx_col_get<double>(di_s, di_m, i);
        atomicAdd(&tagg[slot].sum, price * (1.0 - disc));
        atomicAdd(&tagg[slot].cnt, 1.0);
        local_hits++;
    };
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    /* visimap via a compile-time template split (VM): the default
     * instantiation carries no per-row check at all — a runtime guard
     * here cost 57% (measured, profiles/bw_probe_r01.txt).  The two
     * adds stay two plain atomics: pairing them into one wave
     * instruction through an LDS queue measured 6.17 ms against 4.41
     * (profiles/aggslot_probe_ab.txt).
     * On the packed 16-B slot this kernel is 0.05-0.10 ms SLOWER than
     * on separate sum/count arrays (4.37-4.42 against 4.30-4.32 ms at
     * SF100: 4 slots per 64-B line instead of 8, so a wave's adds
     * cover more lines).  The layout is kept because the orders build
     * gives the same amount back (one 16-B claim store instead of two
     * 8-B ones: 2.28 against 2.35-2.37 ms) and the whole step is equal
     * within spread — three-way A/B in profiles/aggslot_abc.json. */
    for (; i < lk_m.nrows; i += stride)
    {
        if constexpr (VM)
            if (gx_vm_hidden(vmap, i)) continue;
        if (!gx_cmp(fop, gx_col_get<int32_t>(sh_s, sh_m, i), flit)) continue;
        uint64_t k = (uint64_t) gx_col_get<int64_t>(lk_s, lk_m, i);
        uint64_t r;
        if constexpr (RANK)
            r = d_rank_find(rv, k);            /* one load, no walk */
        else
        {
            uint64_t slot = smap.slot0(k);
            r = d_table_find(tkey, tmask, slot, tkey[slot], k);
        }
        if (r != ~0ULL) hit(r, i);
        else umiss(k, i);
    }
    gx_wave_count_add(hits, local_hits);
}

/* Fused Q3 probe+agg over an RLE-compressed l_orderkey column (the real
 * §8f-2 payoff): one workgroup per Dense/RLE block, ONE probe per RUN
 * (lineitem is clustered by l_orderkey — the reference's own table order —
 * so a run is one order's lineitems), and the ship/price/discount columns
 * are touched only for runs whose key is in the join table.
 * The fast parallel count decode needs every repeat count of the block to
 * be 2 bytes (this writer's fixed form, or a reference block whose runs all
 * hold 65..16384 rows); the host decides that per block at bind
 * (rle_block_class, gx_blockref.cls) and other conforming blocks take the
 * serial per-block walk.  Columns with a block this kernel does not read
 * (Orig, DELTA, NULLs, phys > RLE_MAX_PHYS) never get here: prepare
 * materializes them. */
static constexpr int RLE_MAX_PHYS = 4096;

template <typename KT, bool VM = false>
__global__ void k_li_probe_agg_rle(const uint8_t *lk_s, const gx_blockref *dir,
                                   int64_t nblocks,
                                   const uint8_t *pr_s, gx_colmeta pr_m,
                                   const uint8_t *di_s, gx_colmeta di_m,
                                   const uint8_t *sh_s, gx_colmeta sh_m,
                                   const uint8_t *vmap, int fop, int32_t flit,
                                   const KT *tkey,
                                   gx_aggslot *tagg,
                                   gx_slotmap smap,
                                   unsigned long long *hits, int *err)
{
    __shared__ uint32_t s_starts[RLE_MAX_PHYS + 1];   /* exclusive row starts */
    __shared__ uint32_t s_part[256];
    __shared__ uint32_t s_bytepop[RLE_MAX_PHYS / 8];  /* bitmap byte popcount prefix */
    uint64_t tmask = smap.mask;
    unsigned long long local_hits = 0;

    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x)
    {
        const uint8_t *blk = lk_s + dir[b].offset;
        const uint8_t *c = blk + 24;
        int16_t version = ((const int16_t *) c)[0];
        int16_t flags = ((const int16_t *) c)[1];
        int32_t logical = ((const int32_t *) c)[1];
        int32_t phys = ((const int32_t *) c)[2];
        if ((version != 1 && version != 2) || (flags & 0x5) || phys > RLE_MAX_PHYS ||
            logical != dir[b].rows)
        {
            if (threadIdx.x == 0) atomicOr(err, 1);
            __syncthreads();
            continue;
        }
        const int64_t *datum;
        const uint8_t *bmp = nullptr, *cnts = nullptr;
        int32_t csize = 0;
        if (flags & 0x2)
        {
            int32_t bmbits = ((const int32_t *) c)[5];
            csize = ((const int32_t *) c)[7];
            bmp = c + 32;
            cnts = bmp + ((bmbits + 7) >> 3);
            int32_t hdr = 32 + ((bmbits + 7) >> 3) + csize;
            datum = (const int64_t *) (c + ((hdr + 7) & ~7));
            if (bmbits != phys)
            {
                if (threadIdx.x == 0) atomicOr(err, 1);
                __syncthreads();
                continue;
            }
        }
        else
            datum = (const int64_t *) (c + 16);

        /* ---- phase 1: per-physical repeat counts into s_starts[p] ---- */
        if (bmp && dir[b].cls == GX_RLEBLK_FIXED2)
        {
            /* parallel: byte-popcount prefix of the bitmap, then fixed-stride
             * count lookup per ON bit */
            int nbytes = (phys + 7) >> 3;
            d_block_excl_scan(s_bytepop, nbytes, s_part, nullptr, [&](int i) {
                return (uint32_t) __popc((unsigned) bmp[i]);
            });
            for (int p = threadIdx.x; p < phys; p += blockDim.x)
            {
                uint32_t reps = 1;
                uint8_t byte = bmp[p >> 3];
                if (byte & (1u << (p & 7)))
                {
                    uint32_t rank = s_bytepop[p >> 3] +
                                    __popc((unsigned) (byte & ((1u << (p & 7)) - 1)));
                    reps += (((uint32_t) cnts[2 * rank] & 0x3Fu) << 8) |
                            cnts[2 * rank + 1];
                }
                s_starts[p] = reps;
            }
            __syncthreads();
        }
        else if (bmp)
        {
            if (threadIdx.x == 0)   /* conforming varint stream: serial walk */
            {
                int32_t coff = 0;
                for (int p = 0; p < phys; p++)
                {
                    uint32_t reps = 1;
                    if (bmp[p >> 3] & (1u << (p & 7)))
                    {
                        int n = (cnts[coff] >> 6) + 1;
                        uint32_t v = cnts[coff] & 0x3F;
                        for (int i = 1; i < n; i++) v = (v << 8) | cnts[coff + i];
                        coff += n;
                        reps += v;
                    }
                    s_starts[p] = reps;
                }
                if (coff != csize) atomicOr(err, 1);
            }
            __syncthreads();
        }
        else
        {
            for (int p = threadIdx.x; p < phys; p += blockDim.x)
                s_starts[p] = 1;
            __syncthreads();
        }

        /* ---- phase 2: exclusive scan of repeats → row starts ---- */
        {
            /* s_starts[phys] = the total (== logical, checked below) */
            d_block_excl_scan(s_starts, phys, s_part, &s_starts[phys],
                              [&](int i) { return s_starts[i]; });
            if (threadIdx.x == 0 && (int32_t) s_starts[phys] != logical)
                atomicOr(err, 1);
        }

        /* ---- phase 3: one probe per run; rows only for table hits ---- */
        int64_t first = dir[b].first_row;
        for (int p = threadIdx.x; p < phys; p += blockDim.x)
        {
            uint64_t k = (uint64_t) datum[p];
            uint64_t slot = smap.slot0(k);
            if (!d_table_find_from(tkey, tmask, slot, k)) continue;
            uint32_t rs = s_starts[p], re = s_starts[p + 1];
            for (uint32_t r = rs; r < re; r++)
            {
                int64_t g = first + r;
                if constexpr (VM)
                    if (gx_vm_hidden(vmap, g)) continue;
                if (!gx_cmp(fop, gx_col_get<int32_t>(sh_s, sh_m, g), flit)) continue;
                double price = gx_col_get<double>(pr_s, pr_m, g);
                double disc = gx_col_get<double>(di_s, di_m, g);
                atomicAdd(&tagg[slot].sum, price * (1.0 - disc));
                atomicAdd(&tagg[slot].cnt, 1.0);
                local_hits++;
            }
        }
        __syncthreads();
    }
    gx_wave_count_add(hits, local_hits);
}

/* numeric(15,2) probe+agg: measures are scaled int64 (price
 * in cents, discount in hundredths); revenue numerator = Σ price_c·(100−d)
 * accumulated with integer atomics — BIT-EXACT, order-independent, equal to
 * the PG numeric SUM for these ranges.  The numerator lives in the agg
 * slot's sum word (gx_aggslot_num view).  Overflow guard: numerators past 2^62 set the
 * error flag (impossible for sane groups; detects corrupt input). */
template <typename KT, bool VM = false, bool OUTER = false>
__global__ void k_li_probe_agg_num(const uint8_t *lk_s, gx_colmeta lk_m,
                                   const uint8_t *pr_s, gx_colmeta pr_m,
                                   const uint8_t *di_s, gx_colmeta di_m,
                                   const uint8_t *sh_s, gx_colmeta sh_m,
                                   const uint8_t *vmap, int fop, int32_t flit,
                                   const KT *tkey,
                                   gx_aggslot_num *tagg,
                                   gx_slotmap smap,
                                   unsigned long long *hits, int *err,
                                   unsigned long long *ukey = nullptr,
                                   unsigned long long *unum = nullptr,
                                   unsigned long long *ucnt = nullptr,
                                   uint64_t umask = 0)
{
    uint64_t tmask = smap.mask;
    unsigned long long local_hits = 0;
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (; i < lk_m.nrows; i += stride)
    {
        if constexpr (VM)
            if (gx_vm_hidden(vmap, i)) continue;
        if (!gx_cmp(fop, gx_col_get<int32_t>(sh_s, sh_m, i), flit)) continue;
        uint64_t k = (uint64_t) gx_col_get<int64_t>(lk_s, lk_m, i);
        uint64_t slot = smap.slot0(k);
        if (!d_table_find_from(tkey, tmask, slot, k))
        {
            if constexpr (OUTER)
            {
                uint64_t uslot = d_unmatched_claim(ukey, umask, k);
                int64_t pc = gx_col_get<int64_t>(pr_s, pr_m, i);
                int64_t dc = gx_col_get<int64_t>(di_s, di_m, i);
                unsigned long long uadd =
                    (unsigned long long) (pc * (100 - dc));
                unsigned long long uold = atomicAdd(&unum[uslot], uadd);
                if (uold + uadd > (1ULL << 62)) atomicOr(err, 4);
                atomicAdd(&ucnt[uslot], 1ULL);
            }
            continue;
        }
        int64_t price_c = gx_col_get<int64_t>(pr_s, pr_m, i);
        int64_t disc_c = gx_col_get<int64_t>(di_s, di_m, i);
        unsigned long long add = (unsigned long long) (price_c * (100 - disc_c));
        unsigned long long old = atomicAdd(&tagg[slot].sum, add);
        if (old + add > (1ULL << 62)) atomicOr(err, 4);
        atomicAdd(&tagg[slot].cnt, 1ULL);
        local_hits++;
    }
    gx_wave_count_add(hits, local_hits);
}

/* extract groups with ≥1 matched lineitem into SoA result arrays.
 * Per-workgroup compaction (k_extract below): each workgroup owns a
 * contiguous slot tile, counts its keeps, claims an output region with ONE
 * atomic, then writes (cdna_hip_programming.md G12 — a single shared cursor
 * serializes; the first version lost 6 ms to ~500k same-address atomics).
 * d_wave_claim is the per-wave form used by the small side tables. */
__device__ __forceinline__ unsigned long long
d_wave_claim(unsigned long long *ctr, bool mine, int lane,
             unsigned long long *out_off)
{
    unsigned long long m = __ballot(mine);
    if (m == 0) return 0;
    int leader = __ffsll((long long) m) - 1;
    unsigned long long wb = 0;
    if (lane == leader)
        wb = atomicAdd(ctr, (unsigned long long) __popcll(m));
    wb = __shfl(wb, leader, 64);
    *out_off = wb + __popcll(m & ((lane == 0) ? 0ULL
                                              : (~0ULL >> (64 - lane))));
    return m;
}

/* append LEFT-OUTER unmatched groups after the matched extract: same
 * cursor, NULL mid attrs (attrs_null), biased key 2^63 = the NULL-key
 * group (key_is_null).  flags bit0 = key_is_null, bit1 = attrs_null.
 * Rows past cap (the result arrays' capacity) are counted but not written;
 * the host turns cursor > cap into an error. */
__global__ void k_extract_u(const unsigned long long *ukey, const double *urev,
                            const unsigned long long *ucnt, uint64_t uslots,
                            int64_t *okey, int32_t *odate, int32_t *oprio,
                            double *rev, int64_t *cnt, uint8_t *flags,
                            unsigned long long *cursor, int64_t cap)
{
    int lane = threadIdx.x & 63;
    int64_t base0 = blockIdx.x * (int64_t) blockDim.x + threadIdx.x - lane;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (int64_t base = base0; base < (int64_t) uslots; base += stride)
    {
        int64_t i = base + lane;
        bool mine = i < (int64_t) uslots && ukey[i] != 0ULL;
        unsigned long long w;
        unsigned long long m = d_wave_claim(cursor, mine, lane, &w);
        if (m && mine && w < (unsigned long long) cap)
        {
            int64_t k = (int64_t) (ukey[i] ^ (1ULL << 63));
            okey[w] = k;
            odate[w] = 0;
            oprio[w] = 0;
            rev[w] = urev[i];
            cnt[w] = (int64_t) ucnt[i];
            flags[w] = (uint8_t) (k == 0 ? 3 : 2);
        }
    }
}

/* Single-read, block-ordered extract.  A block owns one fixed tile of
 * GX_EXTRACT_ROWS rows x 256 slots; thread t handles slot t of every row, so
 * key loads are fully coalesced and each table byte is read once: the key
 * always, the 16-B agg slot and 8-B attr pair only where the key is non-zero
 * (unclaimed payload is garbage — see gx_aggslot).  Everything a thread will
 * emit stays in registers.  Keeps (key != 0 and count != 0) are ranked with
 * one ballot per (row, wave); the 32 ballot counts are scanned by wave 0,
 * which claims the block's output region with ONE cursor atomic (G12), and a
 * wave's stores for a row then land on consecutive output positions.
 * Output order is slot order within a block.  blockDim.x must be TPB. */
static constexpr int GX_EXTRACT_ROWS = 8;
static constexpr int GX_EXTRACT_TILE = GX_EXTRACT_ROWS * TPB;

template <typename KT>
__global__ void __launch_bounds__(TPB)
k_extract(const KT *tkey, const gx_attrpair *tattr, const gx_aggslot *tagg,
          uint64_t tslots, int numeric,
          int64_t *okey, int32_t *odate, int32_t *oprio,
          double *rev, int64_t *cnt, unsigned long long *cursor)
{
    constexpr int R = GX_EXTRACT_ROWS, NW = TPB / 64;
    /* wave 0 scans the R*NW ballot counts with one lane each */
    static_assert(TPB % 64 == 0 && R * NW <= 64, "k_extract tile geometry");
    __shared__ unsigned long long s_off[R * NW];   /* [row][wave] */
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t) blockIdx.x * GX_EXTRACT_TILE + threadIdx.x;

    KT key[R];
    ulonglong2 agg[R];        /* raw bits: .x = sum, .y = count */
    int2 attr[R];
#pragma unroll
    for (int r = 0; r < R; r++)
    {
        uint64_t i = base + (uint64_t) r * TPB;
        key[r] = (i < tslots) ? tkey[i] : (KT) 0;    /* tslots < tile: tail */
    }
#pragma unroll
    for (int r = 0; r < R; r++)
    {
        uint64_t i = base + (uint64_t) r * TPB;
        agg[r] = make_ulonglong2(0ULL, 0ULL);
        attr[r] = make_int2(0, 0);
        if (key[r] != (KT) 0)
        {
            agg[r] = *reinterpret_cast<const ulonglong2 *>(&tagg[i]);
            attr[r] = *reinterpret_cast<const int2 *>(&tattr[i]);
        }
    }
    /* count bits != 0 is "count != 0" for the f64 and the u64 view alike */
    unsigned long long m[R];
#pragma unroll
    for (int r = 0; r < R; r++)
    {
        m[r] = __ballot(key[r] != (KT) 0 && agg[r].y != 0ULL);
        if (lane == 0) s_off[r * NW + wave] = (unsigned long long) __popcll(m[r]);
    }
    __syncthreads();
    if (wave == 0)
    {
        /* exclusive scan of the R*NW (= 32) counts in (row, wave) order */
        unsigned long long v = (lane < R * NW) ? s_off[lane] : 0ULL, incl = v;
#pragma unroll
        for (int o = 1; o < R * NW; o <<= 1)
        {
            unsigned long long u = __shfl_up(incl, o, 64);
            if (lane >= o) incl += u;
        }
        unsigned long long total = __shfl(incl, R * NW - 1, 64);
        unsigned long long b = 0;
        if (lane == 0 && total) b = atomicAdd(cursor, total);
        b = __shfl(b, 0, 64);
        if (lane < R * NW) s_off[lane] = b + incl - v;
    }
    __syncthreads();
    const unsigned long long below = (lane == 0) ? 0ULL : (~0ULL >> (64 - lane));
#pragma unroll
    for (int r = 0; r < R; r++)
    {
        if (!((m[r] >> lane) & 1ULL)) continue;
        unsigned long long w = s_off[r * NW + wave] + __popcll(m[r] & below);
        okey[w] = (int64_t) key[r];
        odate[w] = attr[r].x;
        oprio[w] = attr[r].y;
        rev[w] = __longlong_as_double((long long) agg[r].x);   /* raw bits */
        cnt[w] = numeric ? (int64_t) agg[r].y
                         : (int64_t) __longlong_as_double((long long) agg[r].y);
    }
}

/* ----- Motion path (nsegs>1) ----- */

/* RCCL send/recv chunking: this pool's RCCL corrupts single self-sends
 * over ~1 GiB (observed: SF100 Motion-1 self-exchange lost half its rows,
 * profiles/bw_probe_r01.txt); self-shares bypass RCCL entirely and all
 * peer transfers are split into <=512 MiB pieces, identically derived on
 * both sides from the exchanged counts. */
static const size_t GX_NCCL_CHUNK = 512ULL << 20;

static ncclResult_t gx_nccl_send_chunked(const void *buf, size_t bytes,
                                         int peer, ncclComm_t comm,
                                         hipStream_t s)
{
    const uint8_t *p = (const uint8_t *) buf;
    while (bytes > 0)
    {
        size_t c = bytes < GX_NCCL_CHUNK ? bytes : GX_NCCL_CHUNK;
        ncclResult_t r = ncclSend(p, c, ncclInt8, peer, comm, s);
        if (r != ncclSuccess) return r;
        p += c;
        bytes -= c;
    }
    return ncclSuccess;
}

static ncclResult_t gx_nccl_recv_chunked(void *buf, size_t bytes, int peer,
                                         ncclComm_t comm, hipStream_t s)
{
    uint8_t *p = (uint8_t *) buf;
    while (bytes > 0)
    {
        size_t c = bytes < GX_NCCL_CHUNK ? bytes : GX_NCCL_CHUNK;
        ncclResult_t r = ncclRecv(p, c, ncclInt8, peer, comm, s);
        if (r != ncclSuccess) return r;
        p += c;
        bytes -= c;
    }
    return ncclSuccess;
}

/* Send/receive layout of one Motion (pure host).  cnts_all is the
 * all-gathered n×n count matrix, row r = rank r's per-destination histogram.
 * Rank seg sends its own row (cnts_all[seg*n + i] rows to rank i) and
 * receives its column (cnts_all[r*n + seg] rows from rank r); the offsets
 * are the exclusive prefix sums, entry n the totals. */
struct gx_mlayout {
    std::vector<unsigned long long> scnt, soff, rcnt, roff;
    unsigned long long send_n = 0, recv_n = 0;
};

static gx_mlayout m_exchange_layout(const unsigned long long *cnts_all, int n,
                                    int seg)
{
    gx_mlayout L;
    L.scnt.assign(n, 0); L.rcnt.assign(n, 0);
    L.soff.assign(n + 1, 0); L.roff.assign(n + 1, 0);
    for (int i = 0; i < n; i++) L.scnt[i] = cnts_all[(int64_t) seg * n + i];
    for (int i = 0; i < n; i++) L.soff[i + 1] = L.soff[i] + L.scnt[i];
    for (int r = 0; r < n; r++) L.rcnt[r] = cnts_all[(int64_t) r * n + seg];
    for (int r = 0; r < n; r++) L.roff[r + 1] = L.roff[r] + L.rcnt[r];
    L.send_n = L.soff[n];
    L.recv_n = L.roff[n];
    return L;
}

/* Payload exchange of one Motion on stream s: rank seg's rows for rank r
 * sit at send + soff[r] rows, the rows from rank r land at recv + roff[r].
 * The self-share bypasses RCCL entirely (a device copy is both faster and
 * avoids self-send at GB sizes, alltoallv standard practice); all peer
 * transfers go through the <=512 MiB chunk helpers in one grouped call. */
static gx_status m_exchange_payload(gx_ctx *ctx, hipStream_t s,
                                    const void *send_rows, void *recv_rows,
                                    const gx_mlayout &L, size_t row_bytes)
{
    const uint8_t *send = (const uint8_t *) send_rows;
    uint8_t *recv = (uint8_t *) recv_rows;
    const int n = ctx->nsegs;
    if (L.scnt[ctx->seg])
        HIP_CHK(ctx, hipMemcpyAsync(recv + L.roff[ctx->seg] * row_bytes,
                                    send + L.soff[ctx->seg] * row_bytes,
                                    L.scnt[ctx->seg] * row_bytes,
                                    hipMemcpyDeviceToDevice, s));
    RCCL_CHK(ctx, ncclGroupStart());
    for (int r = 0; r < n; r++)
    {
        if (r == ctx->seg) continue;
        if (L.scnt[r])
            RCCL_CHK(ctx, gx_nccl_send_chunked(send + L.soff[r] * row_bytes,
                                               L.scnt[r] * row_bytes,
                                               r, ctx->comm, s));
        if (L.rcnt[r])
            RCCL_CHK(ctx, gx_nccl_recv_chunked(recv + L.roff[r] * row_bytes,
                                               L.rcnt[r] * row_bytes,
                                               r, ctx->comm, s));
    }
    RCCL_CHK(ctx, ncclGroupEnd());
    return GX_OK;
}

/* wave-aggregated per-destination counter claims: ONE atomic per wave per
 * destination instead of one per row (a single shared cursor serializes —
 * cdna_hip_programming.md G12; measured 68M same-address atomics ≈ 2 s). */

/* compact non-empty groupby slots into SoA outputs (wave-aggregated
 * cursor claims — a per-slot shared cursor serializes, G12) */
__global__ void k_kv_extract(const unsigned long long *tkey,
                             const double *tsum,
                             const unsigned long long *tcnt, uint64_t tslots,
                             unsigned long long *okey, double *osum,
                             unsigned long long *ocnt,
                             unsigned long long *cursor)
{
    int lane = threadIdx.x & 63;
    int64_t base0 = blockIdx.x * (int64_t) blockDim.x + threadIdx.x - lane;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (int64_t base = base0; base < (int64_t) tslots; base += stride)
    {
        int64_t i = base + lane;
        bool mine = i < (int64_t) tslots && tkey[i] != 0ULL;
        unsigned long long w;
        unsigned long long m = d_wave_claim(cursor, mine, lane, &w);
        if (m && mine)
        {
            okey[w] = tkey[i];
            osum[w] = tsum[i];
            ocnt[w] = tcnt[i];
        }
    }
}

/* ----- two-stage GROUP BY (partial agg → Motion → combine agg) -----
 * The plan cdbgroupingpaths.c:251 builds when the group key is not the
 * distribution key: k_groupby's table is the PARTIAL agg state; its groups
 * are hash-redistributed by the group key and merged on the owning segment
 * with the aggregates' combine functions (nodeAgg.c:2305,2321). */

/* partial-agg table → per-destination histogram by route(group key).
 * Same two-pass hist/emit shape as k_ord_m1_hist/k_ord_m1_emit, scanning
 * table slots instead of rows.  Claims are aggregated twice: one LDS atomic
 * per wave per destination, then ONE global atomic per workgroup per
 * destination.  (Per-wave GLOBAL claims were measured first: a 2^28-slot
 * table is 4.2M wave iterations, and at one destination their same-address
 * atomics serialized to 45.7 ms per kernel — G12.)  The NULL-key group
 * (k_groupby's separate accumulators) is one extra row for null_dest — the
 * segment cdbhash assigns a NULL attribute (rotation only, computed on the
 * host with gx_cdbhash_multi) — when its count is > 0.
 * Dynamic LDS: nsegs u64 (hist), 2·nsegs u64 (emit). */
static constexpr int GB_MAX_SEGS = 2048;   /* emit LDS = 32 KiB at the cap */

/* one workgroup's per-destination group counts into LDS cnt[nsegs] */
__device__ __forceinline__ void d_gb_block_hist(const unsigned long long *tkey,
                                                uint64_t tslots, int nsegs,
                                                unsigned long long *cnt)
{
    int lane = threadIdx.x & 63;
    for (int j = threadIdx.x; j < nsegs; j += blockDim.x) cnt[j] = 0ULL;
    __syncthreads();
    int64_t base0 = blockIdx.x * (int64_t) blockDim.x + threadIdx.x - lane;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (int64_t base = base0; base < (int64_t) tslots; base += stride)
    {
        int64_t i = base + lane;
        unsigned long long bk = i < (int64_t) tslots ? tkey[i] : 0ULL;
        bool keep = bk != 0ULL;
        if (__ballot(keep) == 0ULL) continue;            /* wave-uniform */
        int32_t d = keep ? gx_route_i64((int64_t) (bk ^ (1ULL << 63)), nsegs)
                         : 0;
        for (int dd = 0; dd < nsegs; dd++)
        {
            unsigned long long m = __ballot(keep && d == dd);
            if (m && lane == __ffsll((long long) m) - 1)
                atomicAdd(&cnt[dd], (unsigned long long) __popcll(m));
        }
    }
    __syncthreads();
}

__global__ void k_gb_part_hist(const unsigned long long *tkey, uint64_t tslots,
                               const unsigned long long *null_cnt,
                               int null_dest, int nsegs,
                               unsigned long long *hist)
{
    extern __shared__ unsigned long long gb_lds[];
    d_gb_block_hist(tkey, tslots, nsegs, gb_lds);
    for (int j = threadIdx.x; j < nsegs; j += blockDim.x)
        if (gb_lds[j]) atomicAdd(&hist[j], gb_lds[j]);
    if (blockIdx.x == 0 && threadIdx.x == 0 && *null_cnt != 0ULL)
        atomicAdd(&hist[null_dest], 1ULL);
}

/* partial-agg table → packed gx_kv_group wire rows (unbiased key), grouped
 * contiguously by destination; cursors are pre-set to the region starts.
 * Each workgroup counts its groups per destination, claims one contiguous
 * piece of every destination's region, then its waves claim inside those
 * pieces through LDS cursors. */
__global__ void k_gb_part_emit(const unsigned long long *tkey,
                               const double *tsum,
                               const unsigned long long *tcnt, uint64_t tslots,
                               const double *null_sum,
                               const unsigned long long *null_cnt,
                               int null_dest, int nsegs,
                               unsigned long long *cursors, gx_kv_group *out)
{
    extern __shared__ unsigned long long gb_lds[];
    unsigned long long *cnt = gb_lds, *cur = gb_lds + nsegs;
    d_gb_block_hist(tkey, tslots, nsegs, cnt);
    for (int j = threadIdx.x; j < nsegs; j += blockDim.x)
        cur[j] = cnt[j] ? atomicAdd(&cursors[j], cnt[j]) : 0ULL;
    __syncthreads();

    int lane = threadIdx.x & 63;
    int64_t base0 = blockIdx.x * (int64_t) blockDim.x + threadIdx.x - lane;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (int64_t base = base0; base < (int64_t) tslots; base += stride)
    {
        int64_t i = base + lane;
        unsigned long long bk = i < (int64_t) tslots ? tkey[i] : 0ULL;
        bool keep = bk != 0ULL;
        if (__ballot(keep) == 0ULL) continue;            /* wave-uniform */
        int64_t key = (int64_t) (bk ^ (1ULL << 63));
        int32_t d = keep ? gx_route_i64(key, nsegs) : 0;
        for (int dd = 0; dd < nsegs; dd++)
        {
            unsigned long long w;
            unsigned long long m = d_wave_claim(&cur[dd], keep && d == dd,
                                                lane, &w);
            if (m && keep && d == dd)
            {
                gx_kv_group g{};
                g.key = key;
                g.sum = tsum[i];
                g.count = (int64_t) tcnt[i];
                out[w] = g;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && *null_cnt != 0ULL)
    {
        unsigned long long w = atomicAdd(&cursors[null_dest], 1ULL);
        gx_kv_group g{};
        g.key_is_null = 1;
        g.sum = *null_sum;
        g.count = (int64_t) *null_cnt;
        out[w] = g;
    }
}

/* combine agg: merge received partial states into a fresh table with the
 * two-stage plan's combine functions — sum += partial.sum (float8pl),
 * count += partial.count (int8pl).  Same biased-key/sentinel-0/atomicCAS
 * walk as k_groupby, so duplicate keys merge whichever sender they came
 * from; key_is_null rows merge into the single NULL group. */
__global__ void k_gb_combine(const gx_kv_group *rows, int64_t n,
                             unsigned long long *tkey, double *tsum,
                             unsigned long long *tcnt, uint64_t tmask,
                             double *null_sum, unsigned long long *null_cnt,
                             int *err)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (; i < n; i += stride)
    {
        gx_kv_group g = rows[i];
        if (g.key_is_null)
        {
            atomicAdd(null_sum, g.sum);
            atomicAdd(null_cnt, (unsigned long long) g.count);
            continue;
        }
        uint64_t bk = (uint64_t) g.key ^ (1ULL << 63);
        if (bk == 0) { atomicOr(err, 4); continue; }
        uint64_t slot = gx_hmix64(bk) & tmask;
        while (true)
        {
            unsigned long long prev = atomicCAS(&tkey[slot], 0ULL, bk);
            if (prev == 0ULL || prev == bk) break;
            slot = (slot + 1) & tmask;
        }
        atomicAdd(&tsum[slot], g.sum);
        atomicAdd(&tcnt[slot], (unsigned long long) g.count);
    }
}

/* Motion-1 histogram/emit carry an optional DESTINATION-AWARE bloom
 * prefilter (bloom_all = all ranks' dim blooms, all-gathered): an order
 * only ships when its custkey passes the bloom of the rank it routes to —
 * the reference's runtime-filter pushdown (nodeRuntimeFilter.c) applied
 * ACROSS the interconnect.  False positives only ship extra rows (the
 * destination's exact set probe filters them); results stay bit-exact.
 * Disabled (nullptr) for anti joins, where non-membership is the keep
 * condition. */

/* keep-and-route of mid row i, shared by the two Motion-1 passes: does the
 * row pass visibility, the date filter and the destination's bloom, and
 * which rank does route(fk) send it to?  The loaded date and fk come back
 * in od / oc for the emit pass's output row (read only when kept). */
__device__ __forceinline__ bool
d_m1_keep_route(const uint8_t *od_s, const gx_colmeta &od_m,
                const uint8_t *oc_s, const gx_colmeta &oc_m,
                const uint8_t *vmap, int oop, int32_t olit, int nsegs,
                const unsigned long long *bloom_all, uint64_t bwmask,
                int64_t i, int32_t &d, int32_t &od, int64_t &oc)
{
    if (i >= od_m.nrows || gx_vm_hidden(vmap, i)) return false;
    od = gx_col_get<int32_t>(od_s, od_m, i);
    if (!gx_cmp(oop, od, olit)) return false;
    oc = gx_col_get<int64_t>(oc_s, oc_m, i);
    d = gx_route_i64(oc, nsegs);
    return bloom_all == nullptr ||
           d_bloom_test(bloom_all + (int64_t) d * (bwmask + 1), bwmask,
                        (uint64_t) oc);
}

/* filtered orders → per-destination histogram by route(o_custkey) (Motion 1) */
__global__ void k_ord_m1_hist(const uint8_t *od_s, gx_colmeta od_m,
                              const uint8_t *oc_s, gx_colmeta oc_m,
                              const uint8_t *vmap,
                              int oop, int32_t olit, int nsegs,
                              const unsigned long long *bloom_all,
                              uint64_t bwmask,
                              unsigned long long *hist)
{
    int lane = threadIdx.x & 63;
    int64_t base0 = blockIdx.x * (int64_t) blockDim.x + threadIdx.x - lane;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (int64_t base = base0; base < od_m.nrows; base += stride)
    {
        int64_t i = base + lane;
        int32_t d = 0, od = 0;
        int64_t oc = 0;
        bool keep = d_m1_keep_route(od_s, od_m, oc_s, oc_m, vmap, oop, olit,
                                    nsegs, bloom_all, bwmask, i, d, od, oc);
        for (int dd = 0; dd < nsegs; dd++)
        {
            unsigned long long m = __ballot(keep && d == dd);
            if (m && lane == __ffsll((long long) m) - 1)
                atomicAdd(&hist[dd], (unsigned long long) __popcll(m));
        }
    }
}

__global__ void k_ord_m1_emit(const uint8_t *ok_s, gx_colmeta ok_m,
                              const uint8_t *oc_s, gx_colmeta oc_m,
                              const uint8_t *od_s, gx_colmeta od_m,
                              const uint8_t *op_s, gx_colmeta op_m,
                              const uint8_t *vmap,
                              int oop, int32_t olit, int nsegs,
                              const unsigned long long *bloom_all,
                              uint64_t bwmask,
                              unsigned long long *cursors, /* pre-set to region starts */
                              gx_ord_row *out)
{
    int lane = threadIdx.x & 63;
    int64_t base0 = blockIdx.x * (int64_t) blockDim.x + threadIdx.x - lane;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (int64_t base = base0; base < od_m.nrows; base += stride)
    {
        int64_t i = base + lane;
        int32_t d = 0, od = 0;
        int64_t oc = 0;
        bool keep = d_m1_keep_route(od_s, od_m, oc_s, oc_m, vmap, oop, olit,
                                    nsegs, bloom_all, bwmask, i, d, od, oc);
        for (int dd = 0; dd < nsegs; dd++)
        {
            unsigned long long w;
            unsigned long long m = d_wave_claim(&cursors[dd],
                                                keep && d == dd, lane, &w);
            if (m && keep && d == dd)
            {
                out[w].okey = gx_col_get<int64_t>(ok_s, ok_m, i);
                out[w].ocust = oc;
                out[w].odate = od;
                out[w].oprio = gx_col_get<int32_t>(op_s, op_m, i);
            }
        }
    }
}

/* keep-and-route of received row i, shared by the two Motion-2 passes: is
 * its fk in the local dim set (semi) or not (ANTI), and which rank does
 * route(mid key) send it to? */
template <typename KS, bool ANTI>
__device__ __forceinline__ bool
d_m2_keep_route(const gx_ord_row *rows, int64_t n,
                const KS *cset, uint64_t cmask,
                const unsigned long long *bloom, uint64_t bwmask,
                int nsegs, int64_t i, int32_t &d)
{
    if (i >= n) return false;
    bool in_set = d_bloom_test(bloom, bwmask, (uint64_t) rows[i].ocust) &&
                  d_set_contains(cset, cmask, (uint64_t) rows[i].ocust);
    if (in_set == ANTI) return false;
    d = gx_route_i64(rows[i].okey, nsegs);
    return true;
}

/* received orders rows: probe local customer set, histogram by route(okey) */
template <typename KS, bool ANTI = false>
__global__ void k_qual_hist(const gx_ord_row *rows, int64_t n,
                            const KS *cset, uint64_t cmask,
                            const unsigned long long *bloom, uint64_t bwmask,
                            int nsegs, unsigned long long *hist)
{
    int lane = threadIdx.x & 63;
    int64_t base0 = blockIdx.x * (int64_t) blockDim.x + threadIdx.x - lane;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (int64_t base = base0; base < n; base += stride)
    {
        int64_t i = base + lane;
        int32_t d = 0;
        bool keep = d_m2_keep_route<KS, ANTI>(rows, n, cset, cmask, bloom,
                                              bwmask, nsegs, i, d);
        for (int dd = 0; dd < nsegs; dd++)
        {
            unsigned long long m = __ballot(keep && d == dd);
            if (m && lane == __ffsll((long long) m) - 1)
                atomicAdd(&hist[dd], (unsigned long long) __popcll(m));
        }
    }
}

template <typename KS, bool ANTI = false>
__global__ void k_qual_emit(const gx_ord_row *rows, int64_t n,
                            const KS *cset, uint64_t cmask,
                            const unsigned long long *bloom, uint64_t bwmask,
                            int nsegs, unsigned long long *cursors,
                            gx_qual_row *out)
{
    int lane = threadIdx.x & 63;
    int64_t base0 = blockIdx.x * (int64_t) blockDim.x + threadIdx.x - lane;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (int64_t base = base0; base < n; base += stride)
    {
        int64_t i = base + lane;
        int32_t d = 0;
        bool keep = d_m2_keep_route<KS, ANTI>(rows, n, cset, cmask, bloom,
                                              bwmask, nsegs, i, d);
        for (int dd = 0; dd < nsegs; dd++)
        {
            unsigned long long w;
            unsigned long long m = d_wave_claim(&cursors[dd],
                                                keep && d == dd, lane, &w);
            if (m && keep && d == dd)
            {
                out[w].okey = rows[i].okey;
                out[w].odate = rows[i].odate;
                out[w].oprio = rows[i].oprio;
            }
        }
    }
}

/* min/max over an i64 column (sizing bound for the LEFT-OUTER unmatched
 * table: distinct keys <= min(nrows, range)) */
__global__ void k_col_minmax(const uint8_t *col_s, gx_colmeta m,
                             unsigned long long *maxkey,
                             unsigned long long *minkey)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    unsigned long long kmax = 0, kmin = ~0ULL;
    for (; i < m.nrows; i += stride)
    {
        unsigned long long k = (unsigned long long) gx_col_get<int64_t>(col_s, m, i);
        if (k > kmax) kmax = k;
        if (k < kmin) kmin = k;
    }
    d_wave_minmax_commit<false>(kmax, kmin, maxkey, minkey);
}

/* LEFT-OUTER prepare check: count the non-NULL rows of an i64 key column
 * that hold one of the two values the unmatched table cannot represent —
 * counts[0]: key 0 (biased 2^63 = the NULL-key group), counts[1]: key
 * INT64_MIN (biased 0 = the empty-slot mark).  validity (optional): one
 * byte per row, 0 = NULL (decoded as 0, not counted). */
__global__ void k_col_count_reserved(const uint8_t *col_s, gx_colmeta m,
                                     const uint8_t *validity,
                                     unsigned long long *counts)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    unsigned long long nzero = 0, nmin = 0;
    for (; i < m.nrows; i += stride)
    {
        if (validity && !validity[i]) continue;
        int64_t k = gx_col_get<int64_t>(col_s, m, i);
        if (k == 0) nzero++;
        if (k == INT64_MIN) nmin++;
    }
    gx_wave_count_add(&counts[0], nzero);
    gx_wave_count_add(&counts[1], nmin);
}

/* min/max key stats over received qualifying orders (sizes the motion
 * path's table layout exactly like the local path's counting pass) */
__global__ void k_rows_minmax(const gx_qual_row *rows, int64_t n,
                              unsigned long long *maxkey,
                              unsigned long long *minkey)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    unsigned long long kmax = 0, kmin = ~0ULL;
    for (; i < n; i += stride)
    {
        unsigned long long k = (unsigned long long) rows[i].okey;
        if (k > kmax) kmax = k;
        if (k < kmin) kmin = k;
    }
    d_wave_minmax_commit(kmax, kmin, maxkey, minkey);
}

/* received qualifying orders → build the join/agg table */
template <typename KT>
__global__ void k_build_from_rows(const gx_qual_row *rows, int64_t n,
                                  KT *tkey,
                                  gx_attrpair *tattr, gx_aggslot *tagg,
                                  gx_slotmap smap)
{
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    uint64_t tmask = smap.mask;
    for (; i < n; i += stride)
    {
        uint64_t k = (uint64_t) rows[i].okey;
        uint64_t slot = smap.slot0(k);
        while (true)
        {
            KT prev = atomicCAS(&tkey[slot], (KT) 0, (KT) k);
            if (prev == (KT) 0)
            {
                d_slot_claim(tattr, tagg, slot, rows[i].odate, rows[i].oprio);
                break;
            }
            if (prev == (KT) k) break;
            slot = (slot + 1) & tmask;
        }
    }
}

/* Q3's final ORDER BY revenue DESC, o_orderdate ASC LIMIT K (SURVEY §8f-3;
 * nodeSort.c/nodeLimit.c territory in the reference, run on the QD over
 * trivial row counts).  Each THREAD keeps an exact top-K of its strided
 * slice (insertion against the current K-th; almost every element fails the
 * first compare), each BLOCK then selects top-K of its threads' candidates,
 * and the host merges blocks×K.  Any global top-K member survives each
 * stage, so the result is exact. */
static constexpr int TOPK = 10;

/* "a ranks after b"? ORDER BY revenue DESC, o_orderdate ASC.  NUM: the
 * revenue words are the numeric mode's int64 numerators stored in the f64
 * result array; they are compared as the integers they are, never through
 * their bit patterns read as doubles (small numerators are denormal
 * patterns and would tie under a flush-to-zero mode).  Host and device. */
template <bool NUM>
__host__ __device__ __forceinline__ bool topn_less(double ra, int32_t da,
                                                   double rb, int32_t db)
{
    if constexpr (NUM)
    {
        int64_t ia, ib;
        memcpy(&ia, &ra, 8);
        memcpy(&ib, &rb, 8);
        if (ia != ib) return ia < ib;
    }
    else if (ra != rb) return ra < rb;
    return da > db;
}

/* c_idx carries a candidate's validity: the source row index, or -1 for an
 * empty candidate (fewer than K rows in the block's slices).  Keys are data
 * and take any int64 value, so they cannot mark anything. */
template <bool NUM>
__global__ void __launch_bounds__(64)
k_topn(const int64_t *okey, const int32_t *odate,
       const int32_t *oprio, const double *rev,
       const int64_t *cnt, const uint8_t *flags, int64_t n,
       int64_t *c_idx, int64_t *c_okey, int32_t *c_odate, int32_t *c_oprio,
       double *c_rev, int64_t *c_cnt, uint8_t *c_flags)
{
    /* one wave per block: 64 threads × K candidates → 640 in LDS */
    __shared__ double s_rev[64 * TOPK];
    __shared__ int32_t s_date[64 * TOPK];
    __shared__ int64_t s_idx[64 * TOPK];
    int tid = threadIdx.x;
    double t_rev[TOPK];
    int32_t t_date[TOPK];
    int64_t t_idx[TOPK];
#pragma unroll
    for (int k = 0; k < TOPK; k++) { t_rev[k] = -1.0; t_idx[k] = -1; t_date[k] = 0; }

    int64_t start = blockIdx.x * (int64_t) blockDim.x + tid;
    int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (int64_t i = start; i < n; i += stride)
    {
        double r = rev[i];
        /* NULL dates (outer-join groups) rank LAST on revenue ties: PG
         * ORDER BY o_orderdate ASC defaults to NULLS LAST */
        int32_t d = (flags && (flags[i] & 2)) ? INT32_MAX : odate[i];
        /* fails here for all but ~K·blocks·log(n) elements */
        if (t_idx[TOPK - 1] >= 0 && topn_less<NUM>(r, d, t_rev[TOPK - 1], t_date[TOPK - 1]))
            continue;
        /* sorted insert as a carry walking down the list: the carry swaps
         * with every entry that ranks after it (or is empty), so the old
         * entries move down one place and the last one falls out.  Every
         * index is a compile-time constant after unrolling.  The earlier
         * form, a shift loop over a run-time index k, lost t[0] whenever a
         * new row went in front of an occupied t[0]: in the gfx950 code
         * the compiler made of it, that path left t[1] as it was. */
        double cr = r;
        int32_t cd = d;
        int64_t ci = i;
#pragma unroll
        for (int k = 0; k < TOPK; k++)
        {
            bool take = ci >= 0 &&
                        (t_idx[k] < 0 ||
                         topn_less<NUM>(t_rev[k], t_date[k], cr, cd));
            double xr = t_rev[k];
            int32_t xd = t_date[k];
            int64_t xi = t_idx[k];
            t_rev[k] = take ? cr : xr;
            t_date[k] = take ? cd : xd;
            t_idx[k] = take ? ci : xi;
            cr = take ? xr : cr;
            cd = take ? xd : cd;
            ci = take ? xi : ci;
        }
    }
#pragma unroll
    for (int k = 0; k < TOPK; k++)
    {
        s_rev[tid * TOPK + k] = t_rev[k];
        s_date[tid * TOPK + k] = t_date[k];
        s_idx[tid * TOPK + k] = t_idx[k];
    }
    __syncthreads();
    if (tid == 0)
    {
        for (int k = 0; k < TOPK; k++)
        {
            int best = -1;
            for (int j = 0; j < 64 * TOPK; j++)
            {
                if (s_idx[j] < 0) continue;
                if (best < 0 || topn_less<NUM>(s_rev[best], s_date[best],
                                          s_rev[j], s_date[j]))
                    best = j;
            }
            int64_t w = (int64_t) blockIdx.x * TOPK + k;
            if (best < 0) { c_idx[w] = -1; c_okey[w] = 0; c_rev[w] = 0.0;
                            c_odate[w] = 0; c_oprio[w] = 0; c_cnt[w] = 0;
                            c_flags[w] = 0; continue; }
            int64_t ib = s_idx[best];
            c_idx[w] = ib;
            c_okey[w] = okey[ib];
            c_odate[w] = odate[ib];
            c_oprio[w] = oprio[ib];
            c_rev[w] = rev[ib];
            c_cnt[w] = cnt[ib];
            c_flags[w] = flags ? flags[ib] : 0;
            s_idx[best] = -1;
        }
    }
}

/* ================= descriptor-form GROUP BY ================= */
/* gx_groupby_desc (include/gpuexec.h): several integer key columns, a list of
 * aggregates, AND-ed quals; one scan kernel.
 *
 * GROUP IDENTITY IS A REPRESENTATIVE ROW.  A table slot holds row + 1 of the
 * first row that claimed it (CAS from 0; u32 or u64 word, template ST).  A
 * thread that meets an occupied slot compares its own key columns and
 * validity with those of the slot's row and walks on if they differ.  The
 * input is immutable, so a claimed slot's key is visible the moment the claim
 * is: no key value is reserved and key columns cost no table bytes.
 *
 * ACCUMULATORS are 8-byte words, aword[j] the first word of aggregate j;
 * SUM, MIN and MAX carry a second word counting their non-NULL inputs (the
 * result is NULL when it is 0).  Every word's identity is the all-zero word,
 * so a memset (global) or a zero fill (LDS) BEFORE the scan initialises a
 * table: counts and integer sums add from 0, a float8 sum from +0.0, and MIN
 * and MAX are both an unsigned atomic max over an order-preserving image of
 * the value (MIN: of its complement), which starts at 0 = below every image.
 * Claim-time initialisation would be wrong: a second thread can match a slot
 * before the claimer's stores land.
 *
 * LDS STAGE (template LDS).  Each workgroup keeps a table of the same shape
 * in LDS (lds_slots slots), inserts and accumulates there with LDS atomics,
 * and merges every occupied slot into the global table when its rows are
 * done: one insert plus one atomic per non-identity word per group per
 * workgroup, instead of one set per row on the group's global address.  A
 * row that finds neither its group nor a free slot within GBD_LDS_PROBE
 * steps accumulates directly in the global table, and a workgroup that has
 * seen giveup_rows rows (GBD_GIVEUP_ROWS) with more than 3 of 4 missing stops
 * consulting its LDS table (high cardinality: it is full of other groups). */

struct gbd_col {
    const uint8_t *s;          /* Orig stream, or the flat materialization */
    const uint8_t *val;        /* validity bytes (1 = non-null), or nullptr */
    gx_colmeta m;
};

/* per-aggregate row ops (aop) and per-word merge ops (wop) */
enum { GBD_COUNT_STAR = 0, GBD_COUNT, GBD_SUM_INT, GBD_SUM_F64,
       GBD_MAX_INT, GBD_MIN_INT, GBD_MAX_F64, GBD_MIN_F64 };
enum { GBD_W_ADD = 0, GBD_W_FADD = 1, GBD_W_MAX = 2 };

static constexpr int GBD_MAX_WORDS = 2 * GX_GB_MAX_AGGS;
static constexpr int GBD_LDS_PROBE = 8;
static constexpr unsigned GBD_GIVEUP_ROWS = 4096;   /* GX_GB_GIVEUP_ROWS */
static constexpr int GBD_LDS_BYTES = 40960;   /* 3 workgroups per 160-KiB CU */

struct gbd_args {
    gbd_col key[GX_GB_MAX_KEYS];
    gbd_col agg[GX_GB_MAX_AGGS];
    gbd_col qual[GX_MAX_EXTRA_QUALS];
    int64_t qlit[GX_MAX_EXTRA_QUALS];
    int32_t qop[GX_MAX_EXTRA_QUALS];
    int32_t aop[GX_GB_MAX_AGGS];
    int32_t aword[GX_GB_MAX_AGGS];
    int32_t wop[GBD_MAX_WORDS];
    int32_t nkeys, naggs, nquals, awords;
    int64_t nrows;
    const uint8_t *vmap;
    uint32_t lds_slots;        /* power of two */
    uint32_t giveup_rows;      /* rows a workgroup tries before it may stop */
};

/* sign-extended integer datum of any supported width */
__device__ __forceinline__ int64_t gbd_load(const gbd_col &c, int64_t row)
{
    switch (c.m.width)
    {
        case 1: return gx_col_get<int8_t>(c.s, c.m, row);
        case 2: return gx_col_get<int16_t>(c.s, c.m, row);
        case 4: return gx_col_get<int32_t>(c.s, c.m, row);
        default: return gx_col_get<int64_t>(c.s, c.m, row);
    }
}

__device__ __forceinline__ bool gbd_isnull(const gbd_col &c, int64_t row)
{
    return c.val != nullptr && !c.val[row];
}

/* Order-preserving u64 image of a float8 under float8_cmp_internal: NaNs
 * canonicalised to one value above +inf, negative values reversed.  -0 and
 * +0 keep distinct images (-0 below +0); they compare equal in the reference,
 * so either is a right answer. */
GX_HD uint64_t gbd_f64_image(uint64_t bits)
{
    if ((bits & 0x7FFFFFFFFFFFFFFFULL) > 0x7FF0000000000000ULL)
        bits = 0x7FF8000000000000ULL;
    return (bits >> 63) ? ~bits : bits | (1ULL << 63);
}

GX_HD uint64_t gbd_f64_unimage(uint64_t img)
{
    return (img >> 63) ? img ^ (1ULL << 63) : ~img;
}

/* ---- float8 expression aggregates and float8 quals (gx_gb_ext) ----
 * Only the EXPR instantiations of k_groupby_desc receive gbd_xargs; the
 * others take the empty gbd_noexpr and compile as before.  opnd[] are the
 * DISTINCT float8 columns over all expressions and fquals (deduplicated at
 * plan time); factors, fquals and expression NULL masks name them by index. */
struct gbd_xargs {
    gbd_col  opnd[GX_GB_MAX_OPERANDS];
    uint64_t fqimg[GX_GB_MAX_FQUALS];    /* gbd_fq_image of the literal */
    int32_t  fqop[GX_GB_MAX_FQUALS];
    int32_t  fqopnd[GX_GB_MAX_FQUALS];
    int32_t  fopnd[GX_GB_MAX_AGGS][GX_GB_MAX_FACTORS];
    int32_t  fform[GX_GB_MAX_AGGS][GX_GB_MAX_FACTORS];
    int32_t  nfactors[GX_GB_MAX_AGGS];
    uint32_t emask[GX_GB_MAX_AGGS];      /* operands of expression e, as bits */
    int32_t  aexpr[GX_GB_MAX_AGGS];      /* expression of aggregate j, or -1 */
    int32_t  nopnd, nexprs, nfquals, _pad;
};
struct gbd_noexpr {};

/* One IEEE operation each, rounded to nearest, never contracted: hipcc
 * contracts by default and __dmul_rn and its kin are plain operators in its
 * headers, so the pragma is the fence.  float8mul / float8mi / float8pl of
 * float.c without the overflow / underflow ereport. */
GX_HD double gbd_factor(double c, int form)
{
#pragma clang fp contract(off)
    if (form == GX_FACTOR_ONE_MINUS) return 1.0 - c;
    if (form == GX_FACTOR_ONE_PLUS) return 1.0 + c;
    return c;
}

GX_HD double gbd_fmul(double x, double y)
{
#pragma clang fp contract(off)
    return x * y;
}

/* Image of a float8 for the fqual comparison: gbd_f64_image after -0.0 is
 * made +0.0, so that unsigned order and equality of two images are
 * float8_cmp_internal's (every NaN equal and above +inf, -0 = +0). */
GX_HD uint64_t gbd_fq_image(uint64_t bits)
{
    if (bits == 0x8000000000000000ULL) bits = 0;
    return gbd_f64_image(bits);
}

GX_HD bool gbd_fqual_pass(int op, uint64_t xbits, uint64_t litimg)
{
    return gx_cmp<uint64_t>(op, gbd_fq_image(xbits), litimg);
}

/* A row's operand values, and its expression values: one vector VALUE of
 * eight doubles each, not an array.  An array indexed by the plan's tables
 * stayed in memory (80-144 bytes of scratch per lane, or 16 KiB of LDS,
 * when first built that way); a vector element picked by a wave-uniform
 * index is a register-indexed move. */
typedef double gbd_d8 __attribute__((ext_vector_type(8)));
static_assert(GX_GB_MAX_OPERANDS == 8 && GX_GB_MAX_AGGS == 8, "gbd_d8 holds either");

/* Where a representative row's key columns come from: the input's column
 * streams (the scan), or wire rows (gx_gbd_wire_stride: the combine stage of
 * the two-stage plan, whose received buffer is as immutable as the input). */
struct gbd_key_cols {
    __device__ __forceinline__ bool isnull(const gbd_args &a, int k, int64_t r) const
    { return gbd_isnull(a.key[k], r); }
    __device__ __forceinline__ int64_t load(const gbd_args &a, int k, int64_t r) const
    { return gbd_load(a.key[k], r); }
};

struct gbd_key_wire {
    const unsigned long long *rows;
    int64_t stride;            /* 8-byte words per row */
    __device__ __forceinline__ bool isnull(const gbd_args &a, int k, int64_t r) const
    { return ((rows[r * stride + a.nkeys] >> (8 * k)) & 0xFFULL) != 0ULL; }
    __device__ __forceinline__ int64_t load(const gbd_args &a, int k, int64_t r) const
    { (void) a; return (int64_t) rows[r * stride + k]; }
    /* the state words of row r */
    __device__ __forceinline__ const unsigned long long *
    acc(const gbd_args &a, int64_t r) const
    { return rows + r * stride + a.nkeys + (a.nkeys ? 1 : 0); }
};

/* ---- joins (gx_gbj_ext): the scanned table is the fact side of up to two
 * inner equi-joins; a key or an aggregate's argument may be a column of the
 * matched dimension row.  Only the JOIN instantiations of k_groupby_desc
 * receive gbd_jargs; the others take the empty gbd_nojoin.
 *
 * JOIN TABLE, built like the group tables: u32 slots, a slot holds the
 * dimension row + 1 of the row that claimed it (CAS from 0), a power-of-two
 * slot count of at least 2 x the dimension's rows, linear probing.  A key is
 * compared by reading the dimension's key column at the slot's row (the
 * input is immutable, so it is visible the moment the claim is): no key value
 * is reserved.  The scan only reads the table, after the build has finished
 * on the same stream.  The hash, step and compare below are also what the
 * host restatement gx_selftest_gbj_join runs. */
GX_HD uint64_t gbj_home(int64_t key, uint64_t mask)
{
    return gx_hmix64((uint64_t) key + 0x9E3779B97F4A7C15ULL) & mask;
}

GX_HD uint64_t gbj_next(uint64_t slot, uint64_t mask) { return (slot + 1) & mask; }

GX_HD bool gbj_key_eq(int64_t dim_key, int64_t key) { return dim_key == key; }

/* the dimension row whose key equals `key`, or -1; keyat(r) is the key of
 * dimension row r */
template <typename KEYAT>
GX_HD int64_t gbj_probe(const uint32_t *slots, uint64_t mask, int64_t key,
                        const KEYAT &keyat)
{
    uint64_t s = gbj_home(key, mask);
    for (uint64_t n = 0; n <= mask; n++)
    {
        const uint32_t cur = slots[s];
        if (cur == 0u) return -1;
        if (gbj_key_eq(keyat((int64_t) cur - 1), key)) return (int64_t) cur - 1;
        s = gbj_next(s, mask);
    }
    return -1;
}

struct gbj_col_key {
    const gbd_col &c;
    __device__ __forceinline__ int64_t operator()(int64_t r) const
    { return gbd_load(c, r); }
};

struct gbd_join1 {
    gbd_col fact;              /* join column of the scanned table */
    gbd_col dkey;              /* key column of the dimension */
    const uint32_t *slots;
    uint64_t mask;
};

/* key[k] / agg[j] of gbd_args are bound to the table their side names */
struct gbd_jargs {
    gbd_join1 j[GX_GBJ_MAX_JOINS];
    int32_t njoins;
    uint32_t key_joins;        /* bit j: some key reads joins[j].dim */
    int32_t key_side[GX_GB_MAX_KEYS];
    int32_t agg_side[GX_GB_MAX_AGGS];
};
struct gbd_nojoin {};
static_assert(GX_GBJ_MAX_JOINS == 2, "a row's matches are the two scalars d0, d1");

/* the dimension row fact row r matches in join J (J a compile-time index at
 * every call site), or -1 */
__device__ __forceinline__ int64_t gbj_match(const gbd_join1 &J, int64_t key)
{
    return gbj_probe(J.slots, J.mask, key, gbj_col_key{J.dkey});
}

/* Key source of ONE fact row whose matched dimension rows are d0 / d1: a
 * fact-side key reads the row itself, a dim-side key the dimension's column
 * at that row's match.  Two scalars, not an array indexed by the side: an
 * indexed array would live in scratch. */
struct gbd_key_joined {
    const gbd_jargs &jx;
    int64_t d0, d1;
    __device__ __forceinline__ int64_t at(int k, int64_t r) const
    {
        const int side = jx.key_side[k];
        return side == 0 ? r : side == 1 ? d0 : d1;
    }
    __device__ __forceinline__ bool isnull(const gbd_args &a, int k, int64_t r) const
    { return gbd_isnull(a.key[k], at(k, r)); }
    __device__ __forceinline__ int64_t load(const gbd_args &a, int k, int64_t r) const
    { return gbd_load(a.key[k], at(k, r)); }
};

/* Key source of a REPRESENTATIVE row of a join scan: it finds the row's OWN
 * matched dimension rows by probing again (the row passed, so the probes
 * succeed) and never reads through the match of the row at hand.  No side
 * array of matched rows: a store at claim time is not visible to a thread
 * that sees the claim (header comment above), and the table the probe reads
 * is immutable during the scan. */
struct gbd_key_join {
    const gbd_jargs &jx;
    /* the source of row r with the joins its keys use probed once */
    __device__ __forceinline__ gbd_key_joined of(int64_t r) const
    {
        int64_t d0 = 0, d1 = 0;
        if (jx.key_joins & 1u) d0 = gbj_match(jx.j[0], gbd_load(jx.j[0].fact, r));
        if (jx.key_joins & 2u) d1 = gbj_match(jx.j[1], gbd_load(jx.j[1].fact, r));
        return gbd_key_joined{jx, d0, d1};
    }
    __device__ __forceinline__ bool isnull(const gbd_args &a, int k, int64_t r) const
    { return of(r).isnull(a, k, r); }
    __device__ __forceinline__ int64_t load(const gbd_args &a, int k, int64_t r) const
    { return of(r).load(a, k, r); }
};

/* the same as a kernel argument (k_gbd_extract after a join scan) */
struct gbd_key_join_args {
    gbd_jargs jx;
    __device__ __forceinline__ bool isnull(const gbd_args &a, int k, int64_t r) const
    { return gbd_key_join{jx}.isnull(a, k, r); }
    __device__ __forceinline__ int64_t load(const gbd_args &a, int k, int64_t r) const
    { return gbd_key_join{jx}.load(a, k, r); }
};

/* the key source of the scan kernel's representatives */
__device__ __forceinline__ gbd_key_cols gbd_scan_src(const gbd_nojoin &)
{ return gbd_key_cols{}; }
__device__ __forceinline__ gbd_key_join gbd_scan_src(const gbd_jargs &jx)
{ return gbd_key_join{jx}; }

/* the group hash: its seed, and the step that folds one key column (value 0
 * where NULL) into it */
static constexpr uint64_t GBD_HASH_SEED = 0x9E3779B97F4A7C15ULL;
static constexpr uint64_t GBD_HASH_NULL = 0xD6E8FEB86659FD93ULL;
__device__ __forceinline__ uint64_t gbd_hash_key(uint64_t h, int64_t v, bool isnull)
{
    return gx_hmix64((h ^ (uint64_t) v) + (isnull ? GBD_HASH_NULL : 0ULL));
}

/* key values (0 where NULL), null bits and hash of one row; each key is
 * folded in as it arrives */
template <typename SRC>
__device__ __forceinline__ uint64_t gbd_row_keys(const SRC &src, const gbd_args &a,
                                                 int64_t row,
                                                 int64_t (&kv)[GX_GB_MAX_KEYS],
                                                 unsigned &kn)
{
    uint64_t h = GBD_HASH_SEED;
    kn = 0;
#pragma unroll
    for (int k = 0; k < GX_GB_MAX_KEYS; k++)
    {
        kv[k] = 0;
        if (k < a.nkeys)
        {
            bool isnull = src.isnull(a, k, row);
            kv[k] = isnull ? 0 : src.load(a, k, row);
            kn |= (unsigned) isnull << k;
            h = gbd_hash_key(h, kv[k], isnull);
        }
    }
    return h;
}

/* gbd_row_keys' hash over key values already gathered (a join scan loads a
 * row's fact-side keys before its probes and its dim-side keys after them).
 * The step is written out on the null BIT: through gbd_hash_key's bool the
 * two LDS-off JOIN instantiations spill two more SGPRs. */
__device__ __forceinline__ uint64_t gbd_keys_hash(const gbd_args &a,
                                                  const int64_t (&kv)[GX_GB_MAX_KEYS],
                                                  unsigned kn)
{
    uint64_t h = GBD_HASH_SEED;
#pragma unroll
    for (int k = 0; k < GX_GB_MAX_KEYS; k++)
        if (k < a.nkeys)
            h = gx_hmix64((h ^ (uint64_t) kv[k]) +
                          (((kn >> k) & 1u) ? GBD_HASH_NULL : 0ULL));
    return h;
}

/* NOT DISTINCT equality, column by column, with the keys of row r */
template <typename SRC>
__device__ __forceinline__ bool gbd_keys_eq(const SRC &src, const gbd_args &a,
                                            const int64_t (&kv)[GX_GB_MAX_KEYS],
                                            unsigned kn, int64_t r)
{
    bool eq = true;
#pragma unroll
    for (int k = 0; k < GX_GB_MAX_KEYS; k++)
        if (k < a.nkeys)
        {
            bool rnull = src.isnull(a, k, r);
            eq = eq && rnull == (bool) ((kn >> k) & 1) &&
                 (rnull || src.load(a, k, r) == kv[k]);
        }
    return eq;
}

/* a join scan's representative: probe once per row, not once per column */
__device__ __forceinline__ uint64_t gbd_row_keys(const gbd_key_join &src,
                                                 const gbd_args &a, int64_t row,
                                                 int64_t (&kv)[GX_GB_MAX_KEYS],
                                                 unsigned &kn)
{
    return gbd_row_keys(src.of(row), a, row, kv, kn);
}

__device__ __forceinline__ bool gbd_keys_eq(const gbd_key_join &src, const gbd_args &a,
                                            const int64_t (&kv)[GX_GB_MAX_KEYS],
                                            unsigned kn, int64_t r)
{
    return gbd_keys_eq(src.of(r), a, kv, kn, r);
}

/* find or claim the global slot of the group of row i (keys kv/kn, hash h);
 * ~0 and the error bit when the bounded walk runs out (more groups than the
 * table was sized for) */
template <typename ST, typename SRC>
__device__ __forceinline__ uint64_t gbd_ginsert(const SRC &src, const gbd_args &a,
                                                ST *trow, uint64_t tmask, uint64_t h,
                                                const int64_t (&kv)[GX_GB_MAX_KEYS],
                                                unsigned kn, int64_t i, int *err)
{
    uint64_t slot = h & tmask;
    for (uint64_t n = 0; n <= tmask; n++)
    {
        /* a slot only ever goes 0 -> row + 1: a non-zero read is final, a
         * zero one is settled by the CAS */
        ST cur = trow[slot];
        if (cur == (ST) 0)
        {
            cur = atomicCAS(&trow[slot], (ST) 0, (ST) (i + 1));
            if (cur == (ST) 0) return slot;
        }
        if (gbd_keys_eq(src, a, kv, kn, (int64_t) cur - 1)) return slot;
        slot = (slot + 1) & tmask;
    }
    atomicOr(err, 1);
    return ~0ULL;
}

/* merge the state words l of one group into the global words g of the same
 * group, word by word through wop[]; a word still at its all-zero identity
 * costs nothing.  The combine function of every aggregate (nodeAgg.c:2305). */
__device__ __forceinline__ void d_gbd_merge_words(const gbd_args &a,
                                                  const unsigned long long *l,
                                                  unsigned long long *g)
{
#pragma unroll
    for (int w = 0; w < GBD_MAX_WORDS; w++)
    {
        if (w >= a.awords) continue;
        const unsigned long long v = l[w];
        if (v == 0ULL) continue;              /* still the identity */
        if (a.wop[w] == GBD_W_ADD) atomicAdd(&g[w], v);
        else if (a.wop[w] == GBD_W_FADD)
            atomicAdd((double *) &g[w], __longlong_as_double((long long) v));
        else atomicMax(&g[w], v);
    }
}

/* row i's transition on the first word p of one column aggregate j */
__device__ __forceinline__ void gbd_accum_col(const gbd_args &a, int j, int64_t i,
                                              unsigned long long *p)
{
    const gbd_col &c = a.agg[j];
    const int op = a.aop[j];
    if (op == GBD_COUNT_STAR) { atomicAdd(p, 1ULL); return; }
    if (gbd_isnull(c, i)) return;                    /* strict transitions */
    if (op == GBD_COUNT) { atomicAdd(p, 1ULL); return; }
    switch (op)
    {
        case GBD_SUM_INT:
            atomicAdd(p, (unsigned long long) gbd_load(c, i));
            break;
        case GBD_SUM_F64:
            atomicAdd((double *) p, gx_col_get<double>(c.s, c.m, i));
            break;
        case GBD_MAX_INT:
            atomicMax(p, (unsigned long long) gbd_load(c, i) ^ (1ULL << 63));
            break;
        case GBD_MIN_INT:
            atomicMax(p, ~((unsigned long long) gbd_load(c, i) ^ (1ULL << 63)));
            break;
        case GBD_MAX_F64:
            atomicMax(p, (unsigned long long) gbd_f64_image(
                             gx_col_get<uint64_t>(c.s, c.m, i)));
            break;
        default:
            atomicMax(p, (unsigned long long) ~gbd_f64_image(
                             gx_col_get<uint64_t>(c.s, c.m, i)));
            break;
    }
    atomicAdd(p + 1, 1ULL);
}

/* the transition of a float8 value v (an expression's) on the first word p
 * of an aggregate of transition op; the caller has dealt with NULL */
__device__ __forceinline__ void gbd_accum_f64(int op, double v, unsigned long long *p)
{
    if (op == GBD_COUNT) { atomicAdd(p, 1ULL); return; }
    const uint64_t bits = (uint64_t) __double_as_longlong(v);
    if (op == GBD_SUM_F64) atomicAdd((double *) p, v);
    else if (op == GBD_MAX_F64)
        atomicMax(p, (unsigned long long) gbd_f64_image(bits));
    else atomicMax(p, (unsigned long long) ~gbd_f64_image(bits));
    atomicAdd(p + 1, 1ULL);
}

/* row i's transitions on the accumulator words w of its group; w is an LDS
 * or a global pointer at the two call sites, so each gets its own atomics.
 * EXPR: aggregate j with aexpr[j] >= 0 takes its float8 input from the row's
 * expression registers ev (bit e of enull: expression e is NULL in this
 * row), every other one from its column.  JOIN: a column aggregate reads its
 * argument in the table its side names, at fact row i or at the row's
 * matches d0 / d1. */
template <bool EXPR, bool JOIN, typename X, typename JX>
__device__ __forceinline__ void gbd_accum(const gbd_args &a, const X &x, const JX &jx,
                                          int64_t i, int64_t d0, int64_t d1,
                                          unsigned long long *w, const gbd_d8 &ev,
                                          unsigned enull)
{
#pragma unroll
    for (int j = 0; j < GX_GB_MAX_AGGS; j++)
    {
        if (j >= a.naggs) continue;
        unsigned long long *p = w + a.aword[j];
        if constexpr (EXPR)
        {
            const int e = x.aexpr[j];
            if (e >= 0)
            {
                if ((enull >> e) & 1u) continue;         /* strict transitions */
                gbd_accum_f64(a.aop[j], ev[e], p);
                continue;
            }
        }
        if constexpr (JOIN)
        {
            const int side = jx.agg_side[j];
            gbd_accum_col(a, j, side == 0 ? i : side == 1 ? d0 : d1, p);
        }
        else
            gbd_accum_col(a, j, i, p);
    }
}

/* stats: [0] rows passing visimap + quals (JOIN: and matching every join),
 * [1] rows accumulated in LDS, [4] JOIN: rows that reached the probes */
template <typename ST, bool LDS, bool EXPR, bool JOIN>
__global__ void __launch_bounds__(TPB)
k_groupby_desc(const gbd_args a,
               const std::conditional_t<EXPR, gbd_xargs, gbd_noexpr> x,
               const std::conditional_t<JOIN, gbd_jargs, gbd_nojoin> jx, ST *trow,
               unsigned long long *tacc, uint64_t tmask,
               unsigned long long *stats, int *err)
{
    extern __shared__ unsigned long long gbd_smem[];
    __shared__ unsigned int s_seen, s_miss;
    const uint32_t L = a.lds_slots;
    unsigned long long *lacc = gbd_smem;
    ST *lrow = (ST *) (gbd_smem + (size_t) L * a.awords);
    if (LDS)
    {
        for (uint32_t s = threadIdx.x; s < L * (uint32_t) a.awords; s += TPB)
            lacc[s] = 0ULL;
        for (uint32_t s = threadIdx.x; s < L; s += TPB) lrow[s] = (ST) 0;
        if (threadIdx.x == 0) { s_seen = 0; s_miss = 0; }
        __syncthreads();
    }
    /* where a representative row's keys are read */
    const auto src = gbd_scan_src(jx);
    unsigned long long n_pass = 0, n_lds = 0, n_probed = 0;
    int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    const int64_t stride = gridDim.x * (int64_t) blockDim.x;
    for (; i < a.nrows; i += stride)
    {
        if (gx_vm_hidden(a.vmap, i)) continue;
        /* the key loads go out with the qual loads, not behind their
         * outcome: one memory round trip per row instead of two */
        int64_t kv[GX_GB_MAX_KEYS];
        unsigned kn;
        uint64_t h;
        /* JOIN: the fact-side keys and the join columns go out here as well;
         * the dim-side keys and the hash follow the probes */
        int64_t jv0 = 0, jv1 = 0;
        bool jnull = false;
        if constexpr (JOIN)
        {
            kn = 0;
#pragma unroll
            for (int k = 0; k < GX_GB_MAX_KEYS; k++)
            {
                kv[k] = 0;
                if (k < a.nkeys && jx.key_side[k] == 0)
                {
                    const bool isnull = gbd_isnull(a.key[k], i);
                    kv[k] = isnull ? 0 : gbd_load(a.key[k], i);
                    kn |= (unsigned) isnull << k;
                }
            }
            if (jx.njoins > 0)
            {
                jnull = gbd_isnull(jx.j[0].fact, i);
                jv0 = gbd_load(jx.j[0].fact, i);
            }
            if (jx.njoins > 1)
            {
                jnull = jnull || gbd_isnull(jx.j[1].fact, i);
                jv1 = gbd_load(jx.j[1].fact, i);
            }
        }
        else
            h = gbd_row_keys(gbd_key_cols{}, a, i, kv, kn);
        /* EXPR: every distinct operand column once per row, value and
         * validity, in the same round trip */
        gbd_d8 ov = 0.0, ev = 0.0;
        unsigned onull = 0, enull = 0;
        if constexpr (EXPR)
        {
#pragma unroll
            for (int o = 0; o < GX_GB_MAX_OPERANDS; o++)
            {
                if (o < x.nopnd)
                {
                    onull |= (unsigned) gbd_isnull(x.opnd[o], i) << o;
                    ov[o] = gx_col_get<double>(x.opnd[o].s, x.opnd[o].m, i);
                }
            }
        }
        bool pass = true;
#pragma unroll
        for (int q = 0; q < GX_MAX_EXTRA_QUALS; q++)
            if (q < a.nquals)
                pass = pass && !gbd_isnull(a.qual[q], i) &&   /* NULL fails */
                       gx_cmp<int64_t>(a.qop[q], gbd_load(a.qual[q], i),
                                       a.qlit[q]);
        if constexpr (EXPR)
        {
#pragma unroll
            for (int q = 0; q < GX_GB_MAX_FQUALS; q++)
                if (q < x.nfquals)
                    pass = pass && !((onull >> x.fqopnd[q]) & 1u) &&
                           gbd_fqual_pass(x.fqop[q],
                                          (uint64_t) __double_as_longlong(
                                              ov[x.fqopnd[q]]),
                                          x.fqimg[q]);
        }
        if (!pass) continue;
        /* JOIN: the quals are decided; now the probes, each a chain of
         * dependent random reads.  The join operator is strict, and a row
         * that misses any join is dropped (inner join). */
        int64_t d0 = 0, d1 = 0;
        if constexpr (JOIN)
        {
            n_probed++;
            if (jnull) continue;
            if (jx.njoins > 0)
            {
                d0 = gbj_match(jx.j[0], jv0);
                if (d0 < 0) continue;
            }
            if (jx.njoins > 1)
            {
                d1 = gbj_match(jx.j[1], jv1);
                if (d1 < 0) continue;
            }
            const gbd_key_joined own{jx, d0, d1};
#pragma unroll
            for (int k = 0; k < GX_GB_MAX_KEYS; k++)
                if (k < a.nkeys && jx.key_side[k] != 0)
                {
                    const bool isnull = own.isnull(a, k, i);
                    kv[k] = isnull ? 0 : own.load(a, k, i);
                    kn |= (unsigned) isnull << k;
                }
            h = gbd_keys_hash(a, kv, kn);
        }
        n_pass++;
        if constexpr (EXPR)
        {
#pragma unroll
            for (int e = 0; e < GX_GB_MAX_AGGS; e++)
            {
                if (e < x.nexprs)
                {
                    double v = gbd_factor(ov[x.fopnd[e][0]], x.fform[e][0]);
#pragma unroll
                    for (int f = 1; f < GX_GB_MAX_FACTORS; f++)
                        if (f < x.nfactors[e])
                            v = gbd_fmul(v, gbd_factor(ov[x.fopnd[e][f]],
                                                       x.fform[e][f]));
                    ev[e] = v;
                    enull |= (unsigned) ((onull & x.emask[e]) != 0u) << e;
                }
            }
        }
        bool done = false;
        if (LDS)
        {
            /* racy read on purpose: either answer is correct */
            const unsigned seen = s_seen, miss = s_miss;
            if (!(seen >= a.giveup_rows && miss > seen - (seen >> 2)))
            {
                uint32_t ls = (uint32_t) (h >> 32) & (L - 1);
                for (int p = 0; p < GBD_LDS_PROBE; p++)
                {
                    ST cur = __hip_atomic_load(&lrow[ls], __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (cur == (ST) 0)
                    {
                        cur = atomicCAS(&lrow[ls], (ST) 0, (ST) (i + 1));
                        if (cur == (ST) 0) { done = true; break; }
                    }
                    if (gbd_keys_eq(src, a, kv, kn, (int64_t) cur - 1))
                    { done = true; break; }
                    ls = (ls + 1) & (L - 1);
                }
                if (done)
                {
                    gbd_accum<EXPR, JOIN>(a, x, jx, i, d0, d1,
                                          lacc + (size_t) ls * a.awords, ev, enull);
                    n_lds++;
                }
                /* one pair of counter updates per wave and iteration */
                const unsigned long long act = __ballot(1);
                const unsigned long long mis = __ballot(!done);
                if ((int) (threadIdx.x & 63) == __ffsll((long long) act) - 1)
                {
                    atomicAdd(&s_seen, (unsigned) __popcll(act));
                    if (mis) atomicAdd(&s_miss, (unsigned) __popcll(mis));
                }
            }
        }
        if (!done)
        {
            uint64_t slot = gbd_ginsert<ST>(src, a, trow, tmask, h, kv, kn, i, err);
            if (slot != ~0ULL)
                gbd_accum<EXPR, JOIN>(a, x, jx, i, d0, d1, tacc + slot * a.awords, ev,
                                      enull);
        }
    }
    if (LDS)
    {
        __syncthreads();
        for (uint32_t s = threadIdx.x; s < L; s += TPB)
        {
            const ST r1 = lrow[s];
            if (r1 == (ST) 0) continue;
            const int64_t r = (int64_t) r1 - 1;
            int64_t kv[GX_GB_MAX_KEYS];
            unsigned kn;
            const uint64_t h = gbd_row_keys(src, a, r, kv, kn);
            uint64_t slot = gbd_ginsert<ST>(src, a, trow, tmask, h, kv, kn, r, err);
            if (slot == ~0ULL) continue;
            d_gbd_merge_words(a, lacc + (size_t) s * a.awords,
                              tacc + slot * a.awords);
        }
    }
    gx_wave_count_add(stats + 0, n_pass);
    gx_wave_count_add(stats + 1, n_lds);
    if constexpr (JOIN) gx_wave_count_add(stats + 4, n_probed);
}

/* Compact the occupied slots: representative row -> sign-extended keys and
 * null flags, accumulator words copied.  Each workgroup counts the keeps of
 * its 256-slot tile and claims its output region with ONE cursor atomic
 * (k_extract's way).  Groups past cap are counted, not written; the host
 * turns cursor > cap into an error.  SRC says where a representative's keys
 * are read: gbd_key_cols after the scan, gbd_key_wire after the combine. */
template <typename ST, typename SRC>
__global__ void __launch_bounds__(TPB)
k_gbd_extract(const gbd_args a, const SRC src, const ST *trow,
              const unsigned long long *tacc,
              uint64_t tslots, int64_t *okeys, uint8_t *oknull,
              unsigned long long *oacc, unsigned long long *cursor, int64_t cap)
{
    constexpr int NW = TPB / 64;
    __shared__ unsigned long long s_off[NW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (lane == 0) ? 0ULL : (~0ULL >> (64 - lane));
    for (uint64_t base = (uint64_t) blockIdx.x * TPB; base < tslots;
         base += (uint64_t) gridDim.x * TPB)
    {
        const uint64_t i = base + threadIdx.x;
        const ST r1 = (i < tslots) ? trow[i] : (ST) 0;
        const unsigned long long m = __ballot(r1 != (ST) 0);
        if (lane == 0) s_off[wave] = (unsigned long long) __popcll(m);
        __syncthreads();
        if (threadIdx.x == 0)
        {
            unsigned long long tot = 0;
            for (int w = 0; w < NW; w++) tot += s_off[w];
            unsigned long long b = tot ? atomicAdd(cursor, tot) : 0ULL;
            for (int w = 0; w < NW; w++)
            {
                unsigned long long c = s_off[w];
                s_off[w] = b;
                b += c;
            }
        }
        __syncthreads();
        const unsigned long long w = s_off[wave] + __popcll(m & below);
        if (r1 != (ST) 0 && w < (unsigned long long) cap)
        {
            const int64_t r = (int64_t) r1 - 1;
#pragma unroll
            for (int k = 0; k < GX_GB_MAX_KEYS; k++)
                if (k < a.nkeys)
                {
                    bool isnull = src.isnull(a, k, r);
                    okeys[w * a.nkeys + k] = isnull ? 0 : src.load(a, k, r);
                    oknull[w * a.nkeys + k] = (uint8_t) isnull;
                }
            for (int x = 0; x < a.awords; x++)
                oacc[w * a.awords + x] = tacc[i * a.awords + x];
        }
        __syncthreads();
    }
}

/* Build one join table: every dimension row that its visimap, the join's
 * quals (a NULL input fails) and the key's validity leave is inserted by CAS
 * from 0.  A slot whose row carries an equal key is a duplicate among the
 * participating rows: the error bit is set and the key recorded (any one of
 * them).  misc: [0] rows inserted, [1] error bit, [2] a duplicated key. */
struct gbj_build_args {
    gbd_col key;
    gbd_col qual[GX_MAX_EXTRA_QUALS];
    int64_t qlit[GX_MAX_EXTRA_QUALS];
    int32_t qop[GX_MAX_EXTRA_QUALS];
    int32_t nquals, _pad;
    int64_t nrows;
    const uint8_t *vmap;
};

__global__ void __launch_bounds__(TPB)
k_gbj_build(const gbj_build_args b, uint32_t *slots, uint64_t mask,
            unsigned long long *misc)
{
    unsigned long long n_ins = 0;
    const int64_t stride = gridDim.x * (int64_t) TPB;
    for (int64_t i = blockIdx.x * (int64_t) TPB + threadIdx.x; i < b.nrows; i += stride)
    {
        if (gx_vm_hidden(b.vmap, i)) continue;
        bool pass = !gbd_isnull(b.key, i);               /* strict operator */
        const int64_t key = gbd_load(b.key, i);
#pragma unroll
        for (int q = 0; q < GX_MAX_EXTRA_QUALS; q++)
            if (q < b.nquals)
                pass = pass && !gbd_isnull(b.qual[q], i) &&
                       gx_cmp<int64_t>(b.qop[q], gbd_load(b.qual[q], i), b.qlit[q]);
        if (!pass) continue;
        uint64_t s = gbj_home(key, mask);
        /* at most nrows <= (mask + 1) / 2 slots are ever claimed, so a free
         * one is met within the bound */
        for (uint64_t n = 0; n <= mask; n++)
        {
            uint32_t cur = slots[s];
            if (cur == 0u)
            {
                cur = atomicCAS(&slots[s], 0u, (uint32_t) (i + 1));
                if (cur == 0u) { n_ins++; break; }
            }
            if (gbj_key_eq(gbd_load(b.key, (int64_t) cur - 1), key))
            {
                misc[2] = (unsigned long long) key;
                atomicOr((unsigned int *) (misc + 1), 1u);
                break;
            }
            s = gbj_next(s, mask);
        }
    }
    gx_wave_count_add(misc + 0, n_ins);
}

/* ----- two-stage descriptor GROUP BY (gx_groupby_desc_dist) -----
 * partial agg (k_groupby_desc + k_gbd_extract) -> hash Motion of the partial
 * states by group key -> combine agg on the owning segment.  The partition
 * kernels read the COMPACTED partial groups (okeys / oknull / oacc), not the
 * table slots, and the group count from device memory (the extract cursor),
 * so no host sync stands between the scan and the count all-gather. */

/* owner segment of a group: the reference's cdbhash chain over the key
 * columns, hashint8 for a width-8 column and hashint4 of the value for the
 * narrower ones (wide bit k set = width 8), then the jump hash.  A plain
 * aggregate (no key) is gathered on segment 0.  Host and device. */
GX_HD int32_t gbd_owner(const int64_t (&kv)[GX_GB_MAX_KEYS], unsigned kn,
                        unsigned wide, int nkeys, int nsegs)
{
    uint8_t nb[GX_GB_MAX_KEYS];
    int32_t ty[GX_GB_MAX_KEYS];
#pragma unroll
    for (int k = 0; k < GX_GB_MAX_KEYS; k++)
    {
        nb[k] = (uint8_t) ((kn >> k) & 1);
        ty[k] = ((wide >> k) & 1) ? 0 : 1;
    }
    uint32_t h;
    /* a constant column count per call: the chain unrolls over registers */
    switch (nkeys)
    {
        case 1: h = gx_cdbhash_multi(kv, nb, ty, 1); break;
        case 2: h = gx_cdbhash_multi(kv, nb, ty, 2); break;
        case 3: h = gx_cdbhash_multi(kv, nb, ty, 3); break;
        case 4: h = gx_cdbhash_multi(kv, nb, ty, 4); break;
        default: return 0;
    }
    return gx_jump_consistent_hash((uint64_t) h, nsegs);
}

/* groups the partial stage hands to the Motion.  misc is the partial stage's
 * word block: [2] the extract cursor, [3] the error word.  A failed stage
 * (error bit, or more groups than cap) ships nothing, so its peers' receives
 * still complete; a plain aggregate ships its one state row also when no row
 * reached it (row 0 of oacc is zeroed before the extract). */
__device__ __forceinline__ int64_t d_gbd_part_groups(const unsigned long long *misc,
                                                     int64_t cap, int nkeys)
{
    const unsigned long long ng = misc[2];
    if ((*(const int *) (misc + 3) & 1) || ng > (unsigned long long) cap) return 0;
    return nkeys == 0 ? 1 : (int64_t) ng;
}

/* partial groups -> destination of each (dest[], read back by the emit pass:
 * the jump loop has an f64 divide per iteration) and the per-destination
 * histogram.  One LDS atomic per group on cnt[dest], then one global atomic
 * per workgroup per non-empty destination.  Dynamic LDS: nsegs u32. */
__global__ void __launch_bounds__(TPB)
k_gbd_part_hist(const int64_t *okeys, const uint8_t *oknull,
                const unsigned long long *misc, int64_t cap, int nkeys,
                unsigned wide, int nsegs, uint16_t *dest,
                unsigned long long *hist)
{
    extern __shared__ unsigned int gbd_hist_lds[];
    unsigned int *cnt = gbd_hist_lds;
    for (int j = threadIdx.x; j < nsegs; j += TPB) cnt[j] = 0u;
    __syncthreads();
    const int64_t ng = d_gbd_part_groups(misc, cap, nkeys);
    const int64_t stride = gridDim.x * (int64_t) TPB;
    for (int64_t g = blockIdx.x * (int64_t) TPB + threadIdx.x; g < ng; g += stride)
    {
        int64_t kv[GX_GB_MAX_KEYS];
        unsigned kn = 0;
#pragma unroll
        for (int k = 0; k < GX_GB_MAX_KEYS; k++)
        {
            kv[k] = 0;
            if (k < nkeys)
            {
                kv[k] = okeys[g * nkeys + k];
                kn |= (unsigned) (oknull[g * nkeys + k] != 0) << k;
            }
        }
        const int32_t d = gbd_owner(kv, kn, wide, nkeys, nsegs);
        dest[g] = (uint16_t) d;
        atomicAdd(&cnt[d], 1u);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < nsegs; j += TPB)
        if (cnt[j]) atomicAdd(&hist[j], (unsigned long long) cnt[j]);
}

/* partial groups -> wire rows (gx_gbd_wire_stride) packed by destination;
 * cursors are pre-set to the region starts.  A workgroup counts its groups
 * per destination in LDS, claims one contiguous piece of every non-empty
 * destination's region with one global atomic, then each group claims its
 * row inside the piece with one returning LDS atomic.  Rows are written with
 * 8-byte stores, the null bytes as one zero-padded word.
 * Dynamic LDS: nsegs u64 (piece starts) + nsegs u32 (counts). */
__global__ void __launch_bounds__(TPB)
k_gbd_part_emit(const int64_t *okeys, const uint8_t *oknull,
                const unsigned long long *oacc, const unsigned long long *misc,
                int64_t cap, int nkeys, int awords, int nsegs,
                const uint16_t *dest, unsigned long long *cursors,
                unsigned long long *out)
{
    extern __shared__ unsigned long long gbd_emit_lds[];
    unsigned long long *piece = gbd_emit_lds;
    unsigned int *cnt = (unsigned int *) (gbd_emit_lds + nsegs);
    for (int j = threadIdx.x; j < nsegs; j += TPB) cnt[j] = 0u;
    __syncthreads();
    const int64_t ng = d_gbd_part_groups(misc, cap, nkeys);
    const int64_t stride = gridDim.x * (int64_t) TPB;
    const int64_t g0 = blockIdx.x * (int64_t) TPB + threadIdx.x;
    for (int64_t g = g0; g < ng; g += stride) atomicAdd(&cnt[dest[g]], 1u);
    __syncthreads();
    for (int j = threadIdx.x; j < nsegs; j += TPB)
    {
        const unsigned int c = cnt[j];
        piece[j] = c ? atomicAdd(&cursors[j], (unsigned long long) c) : 0ULL;
        cnt[j] = 0u;
    }
    __syncthreads();
    const int64_t rw = nkeys + (nkeys ? 1 : 0) + awords;
    for (int64_t g = g0; g < ng; g += stride)
    {
        const int d = dest[g];
        const unsigned long long w = piece[d] + atomicAdd(&cnt[d], 1u);
        unsigned long long *row = out + w * rw;
        unsigned long long nullw = 0ULL;
#pragma unroll
        for (int k = 0; k < GX_GB_MAX_KEYS; k++)
            if (k < nkeys)
            {
                row[k] = (unsigned long long) okeys[g * nkeys + k];
                nullw |= (unsigned long long) (oknull[g * nkeys + k] != 0) << (8 * k);
            }
        if (nkeys) row[nkeys] = nullw;
        unsigned long long *acc = row + nkeys + (nkeys ? 1 : 0);
        for (int x = 0; x < awords; x++) acc[x] = oacc[g * awords + x];
    }
}

/* combine agg over n received wire rows: the representative-row table of
 * k_groupby_desc over the received buffer (a slot holds row + 1, keys are
 * compared by reading the slot's wire row, NOT DISTINCT per column; rows
 * hash as gbd_row_keys hashes input rows), the state merged word by word
 * with the aggregates' combine ops.  No LDS stage: at low cardinality the
 * input is nsegs x groups rows, at high cardinality nearly distinct. */
template <typename ST>
__global__ void __launch_bounds__(TPB)
k_gbd_combine(const gbd_args a, const gbd_key_wire src, int64_t n, ST *trow,
              unsigned long long *tacc, uint64_t tmask, int *err)
{
    const int64_t stride = gridDim.x * (int64_t) TPB;
    for (int64_t i = blockIdx.x * (int64_t) TPB + threadIdx.x; i < n; i += stride)
    {
        int64_t kv[GX_GB_MAX_KEYS];
        unsigned kn;
        const uint64_t h = gbd_row_keys(src, a, i, kv, kn);
        const uint64_t slot = gbd_ginsert<ST>(src, a, trow, tmask, h, kv, kn, i, err);
        if (slot != ~0ULL)
            d_gbd_merge_words(a, src.acc(a, i), tacc + slot * a.awords);
    }
}

/* ================= host-side structures ================= */

struct gx_col {
    uint8_t *dstream = nullptr;  /* device AOCS stream */
    gx_colmeta m{};
    int format = 0;              /* 0 = fixed Orig blocks (O(1) addressing),
                                    1 = Dense/RLE (directory-based) */
    gx_blockref *ddir = nullptr; /* device block directory (format 1) */
    int64_t nblocks = 0;
    bool has_null = false;       /* any block carries a NULL bitmap (flags&1) */
    bool fused_ok = false;       /* format 1: every block is one the fused RLE
                                    probe reads (no GX_RLEBLK_UNFUSED) */
};

struct gx_table {
    gx_ctx *ctx = nullptr;
    std::vector<gx_col> cols;
    int64_t nrows = 0;
    uint8_t *dvmap = nullptr;    /* device visimap (1 bit/row, ON = hidden) */
};

/* The device structures of a Q3 run.  Each group below is what a launch
 * helper takes whole; production (gx_q3) and the test entry points of the
 * Motion stages hold the same structs, sized by the same rules. */

/* named scratch words, read back on the host after a launch.  Each word has
 * a 128-byte line of its own: the kernels commit to them with one atomic per
 * wave, and words that share a line make those atomics queue behind each
 * other. */
struct q3_scratch {
    enum { GROUPS, HITS, ERR, COUNT, KMAX, KMIN, NWORDS };
    static constexpr int STRIDE = 16;            /* u64 words per line */
    devbuf buf;
    hipError_t ensure() { return buf.reserve(NWORDS * STRIDE * 8); }
    unsigned long long *word(int w) const
    {
        return buf.as<unsigned long long>() + w * STRIDE;
    }
};

/* what a counting pass leaves in the {COUNT, KMAX, KMIN} words, in that
 * order; kmin is ~0 when nothing was counted */
struct q3_keystats {
    unsigned long long count, kmax, kmin;
};

/* Clear the {count, kmax, kmin} triple on s, run launch(count, kmax, kmin),
 * and bring the triple back: one copy (of the span its three lines cover),
 * one sync. */
template <typename F>
static gx_status q3_read_keystats(gx_ctx *ctx, hipStream_t s, const q3_scratch &sc,
                                  q3_keystats &out, F &&launch)
{
    constexpr int ST = q3_scratch::STRIDE;
    static_assert(q3_scratch::KMAX == q3_scratch::COUNT + 1 &&
                  q3_scratch::KMIN == q3_scratch::COUNT + 2, "triple is contiguous");
    unsigned long long *t = sc.word(q3_scratch::COUNT);
    unsigned long long h[2 * ST + 1];
    HIP_CHK(ctx, hipMemsetAsync(t, 0, 2 * ST * 8, s));
    HIP_CHK(ctx, hipMemsetAsync(t + 2 * ST, 0xFF, 8, s));
    launch(t, t + ST, t + 2 * ST);
    HIP_CHK(ctx, hipMemcpyAsync(h, t, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    out = {h[0], h[ST], h[2 * ST]};
    return GX_OK;
}

/* dimension membership: hash set + blocked bloom, and for dense keys on a
 * single segment the exact bitmap over [kmin, kmin+range) as well.  The local
 * path reads the bitmap INSTEAD of set+bloom; the Motion path keeps
 * set+bloom, so each run builds only the one its path reads. */
struct q3_dimset {
    devbuf set;                      /* u32 or u64 slots, see width */
    devbuf bloom, bits;
    int width = 8;
    uint64_t cmask = 0, bwmask = 0;  /* set slot mask, bloom word-index mask */
    uint64_t kmin = 0, range = 0;
    int bitmap = 0;                  /* decided at sizing */
    gx_dimbits dimbits() const { return {bits.as<unsigned long long>(), kmin, range}; }
};

/* hash form of the join/agg table.  attrs/aggs: claimed slots only, never
 * memset — see gx_aggslot */
struct q3_hashtbl {
    devbuf keys, attrs, aggs;
    int width = 8;                   /* key bytes, 4 or 8 */
    uint64_t mask = 0;
    gx_slotmap smap{};               /* slot mapping (interpolation or hash) */
    uint64_t slots() const { return mask + 1; }
};

/* rank form of the join/agg table (gx_rankview): chosen per run when sizing
 * found the qualifying mid keys dense (ok); each part is allocated by the
 * first run that takes it */
struct q3_ranktbl {
    int ok = 0, kw = 8;
    uint64_t kmin = 0, range = 0;
    devbuf ent;                      /* ulonglong2 {bits, base} per 64 keys */
    devbuf blk;                      /* u32 per-scan-block popcounts */
    devbuf dkey, dattr, dagg;        /* dense arrays, one slot per qualifying row */
    devbuf rowmask;                  /* two-pass orders stage: per mid row */
    devbuf stage, stage_cur;         /* staged orders stage: records and
                                        {record cursor, mid-loop flush count} */
    uint64_t nwords() const { return (range + 63) / 64; }
    gx_rankview view(int64_t qual) const
    {
        return {ent.as<ulonglong2>(), kmin, range, (uint64_t) qual};
    }
};

/* LEFT OUTER: unmatched-row aggregation table (biased keys); empty (all
 * null) for an inner join */
struct q3_unmatched {
    devbuf key, rev, cnt;
    uint64_t mask = 0;
    int64_t cap = 0;                 /* bound on unmatched groups */
    hipError_t clear(hipStream_t s) const
    {
        hipError_t e = hipMemsetAsync(key.p, 0, (mask + 1) * 8, s);
        if (e == hipSuccess) e = hipMemsetAsync(rev.p, 0, (mask + 1) * 8, s);
        if (e == hipSuccess) e = hipMemsetAsync(cnt.p, 0, (mask + 1) * 8, s);
        return e;
    }
};

/* result (device SoA), cap rows */
struct q3_results {
    devbuf okey, odate, oprio, rev, cnt;
    devbuf flags;                    /* per-group key/attr NULL flags */
    int64_t cap = 0;
    hipError_t alloc(int64_t rows)
    {
        cap = 0;
        hipError_t e = okey.alloc(rows * 8);
        if (e == hipSuccess) e = odate.alloc(rows * 4);
        if (e == hipSuccess) e = oprio.alloc(rows * 4);
        if (e == hipSuccess) e = rev.alloc(rows * 8);
        if (e == hipSuccess) e = cnt.alloc(rows * 8);
        if (e == hipSuccess) e = flags.alloc(rows);
        if (e == hipSuccess) cap = rows;
        return e;
    }
};

struct gx_q3 {
    gx_ctx *ctx = nullptr;
    gx_table *cust = nullptr, *ord = nullptr, *li = nullptr;
    gx_q3_desc desc{};          /* column roles + filters (plan descriptor) */
    /* run state (device) — allocated on first run, reused across steps
     * (a re-run rebuilds every table; only the ALLOCATIONS persist).  A
     * sizing that was refused leaves sized false; the next run sizes again
     * and every buffer replaces what it held. */
    bool sized = false;
    q3_scratch sc;
    q3_dimset dim;
    int dim_mode = 0;                /* form the last run's filter read */
    q3_hashtbl tbl;
    uint64_t hash_tslots = 0;        /* local path: slots sizing wants; the
                                        hash table itself is allocated by the
                                        first run that needs it */
    int64_t local_qual = 0;          /* sizing's qualifying mid rows (local) */
    q3_ranktbl rank;
    int table_mode = 0;              /* form the last run used: 0 hash, 1 rank */
    int orders_mode = 0;             /* form the last rank-form run's orders
                                        stage took: 0 two-pass, 1 staged */
    int64_t test_orders_grid = 0;    /* gx_q3_test_set_orders_grid; 0 = rule */
    int64_t stage_blocks = 0;        /* mark grid of the last staged run */
    /* motion-path exchange state (nsegs>1), cached across steps; the
     * send/recv buffers only grow */
    devbuf m_hist, m_cur, m_cnts_all;
    devbuf m_bloom_all;              /* all ranks' dim blooms */
    devbuf m_send1, m_recv1;         /* gx_ord_row */
    devbuf m_send2, m_recv2;         /* gx_qual_row */
    devbuf dtext;                    /* device dim TEXT literal (texteq) */
    devbuf dmask;                    /* per-row texteq result (built once
                                        at prepare over the varlena col) */
    /* extra AND-ed quals folded at prepare into per-table HIDDEN bitmaps
     * (combined with the table visimap); kernels read them through the
     * existing visibility parameter — execScan.c:241 qual-list semantics */
    devbuf qvm_dim, qvm_mid, qvm_fact;
    /* flat materializations of null-bearing / RLE role columns (built at
     * prepare; strict-NULL reject folds their validity into the qvm masks) */
    std::map<std::pair<const gx_table *, int>, gx_col> mat;
    std::vector<devbuf> mat_mem;
    q3_results res;
    q3_unmatched un;
    int numeric = 0;                 /* numeric(15,2) scaled-i64 measures */
    int empty = 0;                   /* LASJ_NOTIN with a NULL dim key:
                                        the whole result is empty
                                        (nodeHashjoin.c:442) */
    int64_t ngroups = 0;
    int64_t qual_orders = 0;
    gx_q3_stats stats{};
    bool ran = false;
};

/* ================= lifecycle ================= */

extern "C" gx_status gx_init(int device_id, int seg_id, int nsegs, gx_ctx **out)
{
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
    {
        snprintf(g_global_err, sizeof g_global_err,
                 "no usable HIP device (%s) — the GPU executor does not fall back to CPU",
                 hipGetErrorString(e));
        return GX_ERR_NOGPU;
    }
    gx_ctx *ctx = new gx_ctx();
    ctx->device = device_id;
    ctx->seg = seg_id;
    ctx->nsegs = nsegs;
    hipError_t e2 = hipSetDevice(device_id);
    if (e2 != hipSuccess) { set_err(nullptr, "hipSetDevice: %s", hipGetErrorString(e2)); delete ctx; return GX_ERR_HIP; }
    e2 = hipStreamCreate(&ctx->stream);
    if (e2 != hipSuccess) { set_err(nullptr, "hipStreamCreate: %s", hipGetErrorString(e2)); delete ctx; return GX_ERR_HIP; }
    e2 = hipStreamCreate(&ctx->stream2);
    if (e2 != hipSuccess) { set_err(nullptr, "hipStreamCreate2: %s", hipGetErrorString(e2)); (void) hipStreamDestroy(ctx->stream); delete ctx; return GX_ERR_HIP; }
    *out = ctx;
    return GX_OK;
}

extern "C" gx_status gx_shutdown(gx_ctx *ctx)
{
    if (!ctx) return GX_OK;
    if (ctx->comm) ncclCommDestroy(ctx->comm);
    if (ctx->stream2) (void) hipStreamDestroy(ctx->stream2);
    if (ctx->stream) (void) hipStreamDestroy(ctx->stream);
    delete ctx;
    return GX_OK;
}

extern "C" gx_status gx_comm_unique_id(unsigned char uid[GX_UNIQUE_ID_BYTES])
{
    static_assert(sizeof(ncclUniqueId) == GX_UNIQUE_ID_BYTES, "uid size");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return GX_ERR_RCCL;
    memcpy(uid, &id, GX_UNIQUE_ID_BYTES);
    return GX_OK;
}

extern "C" gx_status gx_comm_init(gx_ctx *ctx, const unsigned char uid[GX_UNIQUE_ID_BYTES])
{
    if (!ctx) return GX_ERR_INVALID;
    if (ctx->comm) return GX_OK;   /* one communicator per process lifetime
                                    * (mirrors gang reuse; gpuexec.h) */
    ncclUniqueId id;
    memcpy(&id, uid, GX_UNIQUE_ID_BYTES);
    RCCL_CHK(ctx, ncclCommInitRank(&ctx->comm, ctx->nsegs, id, ctx->seg));
    return GX_OK;
}

/* ================= tables ================= */

static gx_status encode_column_device(gx_ctx *ctx, const void *dvals, int width,
                                      int64_t nrows, gx_col *col)
{
    int32_t rpb = gx_aocs_rows_per_block(width, 32768);
    int64_t nblocks = (nrows + rpb - 1) / rpb;
    int64_t full_len = gx_aocs_block_len(width, rpb);
    int64_t last_rows = nrows - (nblocks - 1) * (int64_t) rpb;
    int64_t bytes = (nblocks - 1) * full_len + gx_aocs_block_len(width, last_rows);
    uint8_t *stream = nullptr;
    HIP_CHK(ctx, hipMalloc(&stream, bytes));
    HIP_CHK(ctx, hipMemsetAsync(stream, 0, bytes, ctx->stream));
    int grid = (int) std::min<int64_t>(std::max<int64_t>(nblocks, 1), 65535);
    if (width == 8)
        hipLaunchKernelGGL(k_encode<int64_t>, dim3(grid), dim3(TPB), 0, ctx->stream,
                           (const int64_t *) dvals, nrows, rpb, full_len, nblocks, stream);
    else if (width == 4)
        hipLaunchKernelGGL(k_encode<int32_t>, dim3(grid), dim3(TPB), 0, ctx->stream,
                           (const int32_t *) dvals, nrows, rpb, full_len, nblocks, stream);
    else
        hipLaunchKernelGGL(k_encode<int8_t>, dim3(grid), dim3(TPB), 0, ctx->stream,
                           (const int8_t *) dvals, nrows, rpb, full_len, nblocks, stream);
    hipLaunchKernelGGL(k_crc_fill, dim3(GRID), dim3(64), 0, ctx->stream,
                       stream, nblocks, full_len, nrows, rpb, width);
    HIP_CHK(ctx, hipGetLastError());
    col->dstream = stream;
    col->m.width = width;
    col->m.rpb = rpb;
    col->m.nrows = nrows;
    col->m.full_block_len = full_len;
    col->m.nbytes = bytes;
    gx_colmeta_finish(&col->m);
    return GX_OK;
}

/* HOST-side RLE_TYPE writer (Dense_Enhanced, no-null no-delta; format notes
 * in oracle/oracle.c — independent implementation, parity-tested against the
 * oracle decoder).  Repeat counts are always emitted as 2-byte Int32Compress
 * encodings (len bits = 01) — conforming, and fixed stride lets the fused
 * scan kernel locate counts in parallel.  Runs longer than 0x3FFF extras are
 * split.  Only needed where the device generator can't write RLE directly. */
static void host_crc32c_table(uint32_t *tab)
{
    for (uint32_t i = 0; i < 256; i++)
    {
        uint32_t c = i;
        for (int k = 0; k < 8; k++)
            c = (c & 1) ? (0x82F63B78u ^ (c >> 1)) : (c >> 1);
        tab[i] = c;
    }
}
static uint32_t host_crc32c(const uint32_t *tab, uint32_t crc,
                            const uint8_t *p, int64_t len)
{
    while (len--) crc = tab[(crc ^ *p++) & 0xFF] ^ (crc >> 8);
    return crc;
}

static int64_t host_rle_encode(const uint8_t *src_v, int width, int64_t nrows,
                               int32_t blocksize, std::vector<uint8_t> &out)
{
    uint32_t tab[256];
    host_crc32c_table(tab);
    const int32_t maxdata = blocksize - 32;
    int64_t row = 0;
    std::vector<uint8_t> pvals;
    std::vector<int32_t> extra;
    while (row < nrows)
    {
        pvals.clear();
        extra.clear();
        int32_t non = 0;
        int64_t logical = 0;
        while (row + logical < nrows)
        {
            const uint8_t *d = src_v + (row + logical) * width;
            int phys = (int) extra.size();
            bool same = phys > 0 &&
                        memcmp(&pvals[(size_t) (phys - 1) * width], d, width) == 0 &&
                        extra[phys - 1] < 0x3FFF;
            int new_phys = phys + (same ? 0 : 1);
            int new_non = non + (same && extra[phys - 1] == 0 ? 1 : 0);
            int32_t bm = (new_phys + 7) >> 3;
            int32_t hdr = 16 + (new_non ? 16 + bm + 2 * new_non : 0);
            int64_t tot = ((hdr + 7) & ~7) + (int64_t) new_phys * width;
            if (tot >= maxdata && logical > 0)
                break;
            if (same)
            {
                if (extra[phys - 1] == 0) non++;
                extra[phys - 1]++;
            }
            else
            {
                pvals.insert(pvals.end(), d, d + width);
                extra.push_back(0);
            }
            logical++;
        }
        int phys = (int) extra.size();
        bool has_rle = non > 0;
        int32_t bm = (phys + 7) >> 3;
        int32_t hdr = 16 + (has_rle ? 16 + bm + 2 * non : 0);
        int32_t datum_off = (hdr + 7) & ~7;
        int32_t content = datum_off + phys * width;
        int64_t blocklen = (24 + content + 7) & ~7LL;
        size_t base = out.size();
        out.resize(base + blocklen, 0);
        uint8_t *blk = out.data() + base;
        uint32_t kind = (logical <= 16383) ? 1u : 3u;
        uint32_t b03 = (kind << 28) | (1u << 27) | (1u << 24);
        uint32_t b47 = 0;
        if (kind == 1)
        {
            b03 |= (0x00FFFC00u & ((uint32_t) logical << 10)) |
                   (((uint32_t) content >> 11) & 0x3FFu);
            b47 = ((uint32_t) content & 0x7FFu) << 21;
        }
        else
        {
            b03 |= ((uint32_t) content & 0x1FFFFFu);
            b47 = (uint32_t) logical & 0x3FFFFFFFu;
        }
        memcpy(blk, &b03, 4);
        memcpy(blk + 4, &b47, 4);
        int64_t frn = row + 1;
        memcpy(blk + 16, &frn, 8);
        uint8_t *c = blk + 24;
        int16_t v16 = 2; memcpy(c, &v16, 2);
        v16 = has_rle ? 2 : 0; memcpy(c + 2, &v16, 2);
        int32_t v32 = (int32_t) logical; memcpy(c + 4, &v32, 4);
        v32 = phys; memcpy(c + 8, &v32, 4);
        v32 = phys * width; memcpy(c + 12, &v32, 4);
        if (has_rle)
        {
            v32 = 0; memcpy(c + 16, &v32, 4);
            v32 = phys; memcpy(c + 20, &v32, 4);
            v32 = non; memcpy(c + 24, &v32, 4);
            v32 = 2 * non; memcpy(c + 28, &v32, 4);
            uint8_t *bmp = c + 32;
            uint8_t *cnts = bmp + bm;
            int w = 0;
            for (int pi = 0; pi < phys; pi++)
                if (extra[pi] > 0)
                {
                    bmp[pi >> 3] |= (uint8_t) (1u << (pi & 7));
                    cnts[w] = (uint8_t) ((1 << 6) | (extra[pi] >> 8));
                    cnts[w + 1] = (uint8_t) extra[pi];
                    w += 2;
                }
        }
        memcpy(c + datum_off, pvals.data(), (size_t) phys * width);
        uint32_t crc = host_crc32c(tab, 0xFFFFFFFFu, blk + 16, blocklen - 16);
        memcpy(blk + 8, &crc, 4);
        crc = host_crc32c(tab, 0xFFFFFFFFu, blk, 12);
        memcpy(blk + 12, &crc, 4);
        row += logical;
    }
    return (int64_t) out.size();
}

/* Bulk-decompressed bind: blocks with compressedLength>0 (compresstype=
 * zlib) are inflated on the HOST at bind time — the reference decompresses
 * on the CPU during scan too (datumstream.c:1258-1290); we pay it once and
 * keep the working set uncompressed in HBM.  Returns false when the stream
 * has no compressed blocks (no copy made). */
static bool host_decompress_stream(const uint8_t *s, int64_t nbytes,
                                   int codec, std::vector<uint8_t> &out)
{
    /* pass 0: anything compressed at all? (avoid copying plain streams) */
    {
        int64_t o = 0;
        bool found = false;
        while (o + 24 <= nbytes)
        {
            uint32_t b03, b47;
            memcpy(&b03, s + o, 4);
            memcpy(&b47, s + o + 4, 4);
            if (b03 == 0 && b47 == 0) break;
            uint32_t kind = (b03 >> 28) & 7;
            uint32_t datalen, complen = 0;
            if (kind == 1)
            {
                datalen = ((b03 & 0x3FFu) << 11) | ((b47 & 0xFFE00000u) >> 21);
                complen = b47 & 0x1FFFFFu;
            }
            else if (kind == 3)
                datalen = b03 & 0x1FFFFFu;
            else
                return false;
            if (complen) { found = true; break; }
            o += (24 + (int64_t) datalen + 7) & ~7LL;
        }
        if (!found) return false;
    }
    uint32_t tab[256];
    host_crc32c_table(tab);
    bool any = false;
    int64_t off = 0;
    while (off + 24 <= nbytes)
    {
        uint32_t b03, b47;
        memcpy(&b03, s + off, 4);
        memcpy(&b47, s + off + 4, 4);
        if (b03 == 0 && b47 == 0) break;
        uint32_t kind = (b03 >> 28) & 7;
        uint32_t datalen, complen = 0;
        if (kind == 1)
        {
            datalen = ((b03 & 0x3FFu) << 11) | ((b47 & 0xFFE00000u) >> 21);
            complen = b47 & 0x1FFFFFu;
        }
        else if (kind == 3)
            datalen = b03 & 0x1FFFFFu;
        else
            return false;
        int64_t blocklen = (24 + (int64_t) (complen ? complen : datalen) + 7) & ~7LL;
        if (off + blocklen > nbytes) return false;
        int64_t newlen = (24 + (int64_t) datalen + 7) & ~7LL;
        size_t base = out.size();
        out.resize(base + newlen, 0);
        uint8_t *blk = out.data() + base;
        memcpy(blk, s + off, 24);
        if (complen)
        {
            any = true;
            if (codec == 2)
            {
                size_t r = ZSTD_decompress(blk + 24, datalen, s + off + 24, complen);
                if (ZSTD_isError(r) || r != datalen)
                    return false;
            }
            else
            {
                unsigned long dl = datalen;
                if (uncompress(blk + 24, &dl, s + off + 24, complen) != Z_OK ||
                    dl != datalen)
                    return false;
            }
            uint32_t nb47;
            memcpy(&nb47, blk + 4, 4);
            nb47 &= ~0x1FFFFFu;                 /* compressedLength = 0 */
            memcpy(blk + 4, &nb47, 4);
            uint32_t crc = host_crc32c(tab, 0xFFFFFFFFu, blk + 16, newlen - 16);
            memcpy(blk + 8, &crc, 4);
            crc = host_crc32c(tab, 0xFFFFFFFFu, blk, 12);
            memcpy(blk + 12, &crc, 4);
        }
        else
            memcpy(blk + 24, s + off + 24, blocklen - 24);
        off += blocklen;
    }
    return any;
}

/* Class of one DatumStreamBlock for the fused RLE fact-key probe: c points at
 * the block content (past the 24-byte AO envelope), datalen is its length,
 * rows the envelope's row count.  The fused scan reads Dense/Dense_Enhanced
 * blocks of 8-byte datums with at most RLE_MAX_PHYS physical datums and
 * neither NULL bitmap nor DELTA; everything else, and any header whose
 * sections do not fit datalen, is GX_RLEBLK_UNFUSED.  FIXED2 is claimed only
 * when the leading byte of EVERY count says "2 bytes" and the bitmap has one
 * ON bit per count: csize == 2*ncnt alone also holds for a 1-byte + 3-byte
 * mix.  Pure host function; gx_selftest_rle_block_class. */
static int rle_block_class(const uint8_t *c, int64_t datalen, int64_t rows)
{
    if (datalen < 16) return GX_RLEBLK_UNFUSED;
    int16_t version, flags;
    int32_t logical, phys, psize;
    memcpy(&version, c, 2);
    memcpy(&flags, c + 2, 2);
    memcpy(&logical, c + 4, 4);
    memcpy(&phys, c + 8, 4);
    memcpy(&psize, c + 12, 4);
    if ((version != 1 && version != 2) || (flags & ~0x2) != 0 ||
        phys < 0 || phys > RLE_MAX_PHYS || psize != phys * 8 ||
        logical != rows)
        return GX_RLEBLK_UNFUSED;
    if (!(flags & 0x2))
        return (logical == phys && 16 + (int64_t) psize <= datalen)
                   ? GX_RLEBLK_NOBITMAP : GX_RLEBLK_UNFUSED;
    if (datalen < 32) return GX_RLEBLK_UNFUSED;
    int32_t bmbits, ncnt, csize;
    memcpy(&bmbits, c + 20, 4);
    memcpy(&ncnt, c + 24, 4);
    memcpy(&csize, c + 28, 4);
    if (bmbits != phys || ncnt < 0 || csize < 0) return GX_RLEBLK_UNFUSED;
    int64_t bmbytes = (bmbits + 7) >> 3;
    int64_t hdr = 32 + bmbytes + csize;
    if (((hdr + 7) & ~7LL) + psize > datalen) return GX_RLEBLK_UNFUSED;
    if (csize != 2 * (int64_t) ncnt) return GX_RLEBLK_VARINT;
    const uint8_t *bmp = c + 32, *cnts = bmp + bmbytes;
    int64_t on = 0;
    for (int32_t p = 0; p < phys; p++)
        on += (bmp[p >> 3] >> (p & 7)) & 1;
    if (on != ncnt) return GX_RLEBLK_VARINT;
    for (int32_t i = 0; i < ncnt; i++)
        if ((cnts[2 * i] >> 6) != 1) return GX_RLEBLK_VARINT;
    return GX_RLEBLK_FIXED2;
}

/* walk a stream's AO envelope headers on the HOST, building the per-block
 * directory a variable-geometry (Dense/RLE) stream needs.  fused_ok_out:
 * every block is one the fused RLE probe reads (rle_block_class). */
static gx_status parse_block_dir(const uint8_t *s, int64_t nbytes,
                                 std::vector<gx_blockref> &dir, int64_t *rows_out,
                                 bool *has_null_out = nullptr,
                                 bool *fused_ok_out = nullptr)
{
    int64_t off = 0, row = 0;
    if (has_null_out) *has_null_out = false;
    if (fused_ok_out) *fused_ok_out = true;
    while (off + 24 <= nbytes)
    {
        uint32_t b03, b47;
        memcpy(&b03, s + off, 4);
        memcpy(&b47, s + off + 4, 4);
        if (b03 == 0 && b47 == 0) break;
        uint32_t kind = (b03 >> 28) & 7;
        uint32_t rows, datalen;
        if (kind == 1)
        {
            rows = (b03 & 0x00FFFC00u) >> 10;
            datalen = ((b03 & 0x3FFu) << 11) | ((b47 & 0xFFE00000u) >> 21);
            if ((b47 & 0x1FFFFFu) != 0) return GX_ERR_INVALID;
        }
        else if (kind == 3)
        {
            rows = b47 & 0x3FFFFFFFu;
            datalen = b03 & 0x1FFFFFu;
        }
        else
            return GX_ERR_INVALID;
        int64_t blocklen = (24 + (int64_t) datalen + 7) & ~7LL;
        if (off + blocklen > nbytes) return GX_ERR_INVALID;
        if (has_null_out && blocklen >= 28)
        {
            int16_t flags;                       /* DatumStreamBlock flags */
            memcpy(&flags, s + off + 26, 2);
            if (flags & 1) *has_null_out = true; /* HAS_NULLBITMAP */
        }
        int cls = rle_block_class(s + off + 24, datalen, rows);
        if (fused_ok_out && cls == GX_RLEBLK_UNFUSED) *fused_ok_out = false;
        dir.push_back({off, row, (int32_t) rows, cls});
        row += rows;
        off += blocklen;
    }
    *rows_out = row;
    return GX_OK;
}

/* A format-0 column is addressed in O(1) (gx_col_get): block b starts at
 * b*full_block_len and every block but the last holds exactly rpb rows.
 * Nothing on the device re-checks that, so walk the envelope headers on the
 * HOST at bind and refuse any stream the arithmetic would mis-address: a
 * truncated stream, a wrong width or blocksize, a partial block in the
 * middle (two segment files concatenated — bind those as format 1). */
static const char *check_orig_geometry(const uint8_t *s, int64_t nbytes,
                                       const gx_colmeta &m)
{
    if (m.width != 1 && m.width != 4 && m.width != 8)
        return "format-0 width must be 1, 4 or 8";
    if (m.nrows < 0 || m.rpb <= 0) return "bad nrows/blocksize";
    int64_t off = 0, row = 0;
    while (off < nbytes)
    {
        if (off + 24 > nbytes) return "truncated block header";
        uint32_t b03, b47;
        memcpy(&b03, s + off, 4);
        memcpy(&b47, s + off + 4, 4);
        if (((b03 >> 28) & 7) != 1 || (b47 & 0x1FFFFFu) != 0)
            return "not a small-content block";
        int64_t rows = (b03 & 0x00FFFC00u) >> 10;
        int64_t datalen = ((b03 & 0x3FFu) << 11) | ((b47 & 0xFFE00000u) >> 21);
        int64_t blocklen = (24 + datalen + 7) & ~7LL;
        if (off + blocklen > nbytes) return "truncated block";
        int64_t want = std::min<int64_t>(m.rpb, m.nrows - row);
        if (want <= 0) return "more rows than nrows";
        if (rows != want)
            return "a block before the last is not full (wrong width or "
                   "blocksize, or concatenated streams: bind as format 1)";
        if (datalen != 16 + rows * m.width) return "block length does not match width";
        row += rows;
        off += blocklen;
    }
    if (row != m.nrows) return "fewer rows than nrows";
    return nullptr;
}

extern "C" gx_status gx_table_bind(gx_ctx *ctx, const gx_coldesc *cols, int ncols,
                                   gx_table **out)
{
    if (!ctx || !cols || ncols <= 0) return GX_ERR_INVALID;
    for (int c = 1; c < ncols; c++)
        if (cols[c].nrows != cols[0].nrows)
        {
            set_err(ctx, "bind: every column of a table needs the same nrows%s", "");
            return GX_ERR_INVALID;
        }
    gx_table *t = new gx_table();
    t->ctx = ctx;
    t->nrows = cols[0].nrows;
    for (int c = 0; c < ncols; c++)
    {
        gx_col col;
        col.format = cols[c].format;
        const void *stream_src = cols[c].host_stream;
        int64_t stream_len = cols[c].nbytes;
        std::vector<uint8_t> inflated;
        if (host_decompress_stream((const uint8_t *) stream_src, stream_len,
                                   cols[c].codec, inflated))
        {
            stream_src = inflated.data();
            stream_len = (int64_t) inflated.size();
        }
        if (cols[c].width < 0 && cols[c].format != 1)
        {
            set_err(ctx, "varlena columns need a block directory (format 1)%s", "");
            delete t;
            return GX_ERR_INVALID;
        }
        col.m.width = cols[c].width;
        col.m.rpb = gx_aocs_rows_per_block(std::max(cols[c].width, 1),
                                           cols[c].blocksize);
        col.m.nrows = cols[c].nrows;
        col.m.full_block_len = gx_aocs_block_len(cols[c].width, col.m.rpb);
        col.m.nbytes = stream_len;
        if (col.m.rpb <= 0)
        {
            set_err(ctx, "bind: blocksize too small for one row%s", "");
            gx_table_free(t);
            return GX_ERR_INVALID;
        }
        gx_colmeta_finish(&col.m);
        if (col.format == 0)
        {
            const char *why = check_orig_geometry((const uint8_t *) stream_src,
                                                  stream_len, col.m);
            if (why)
            {
                set_err(ctx, "bad Orig stream: %s", why);
                gx_table_free(t);
                return GX_ERR_INVALID;
            }
        }
        if (col.format == 1)
        {
            std::vector<gx_blockref> dir;
            int64_t rows = 0;
            gx_status st = parse_block_dir((const uint8_t *) stream_src,
                                           stream_len, dir, &rows,
                                           &col.has_null, &col.fused_ok);
            if (st != GX_OK || rows != cols[c].nrows)
            {
                set_err(ctx, "bad Dense/RLE stream%s", "");
                delete t;
                return GX_ERR_INVALID;
            }
            col.nblocks = (int64_t) dir.size();
            hipError_t e = hipMalloc(&col.ddir, dir.size() * sizeof(gx_blockref));
            if (e != hipSuccess) { delete t; return GX_ERR_OOM; }
            e = hipMemcpyAsync(col.ddir, dir.data(),
                               dir.size() * sizeof(gx_blockref),
                               hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess)
                e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess)
            {
                set_err(ctx, "dir upload: %s", hipGetErrorString(e));
                delete t;
                return GX_ERR_HIP;
            }
        }
        hipError_t e = hipMalloc(&col.dstream, stream_len);
        if (e != hipSuccess) { set_err(ctx, "hipMalloc: %s", hipGetErrorString(e)); delete t; return GX_ERR_OOM; }
        e = hipMemcpyAsync(col.dstream, stream_src, stream_len,
                           hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) { set_err(ctx, "hipMemcpy: %s", hipGetErrorString(e)); delete t; return GX_ERR_HIP; }
        e = hipStreamSynchronize(ctx->stream);  /* inflated buffer is stack-local */
        if (e != hipSuccess) { set_err(ctx, "bind sync: %s", hipGetErrorString(e)); delete t; return GX_ERR_HIP; }
        t->cols.push_back(col);
    }
    (void) hipStreamSynchronize(ctx->stream);
    *out = t;
    return GX_OK;
}

extern "C" gx_status gx_table_free(gx_table *t)
{
    if (!t) return GX_OK;
    for (auto &c : t->cols)
    {
        if (c.dstream) (void) hipFree(c.dstream);
        if (c.ddir) (void) hipFree(c.ddir);
    }
    if (t->dvmap) (void) hipFree(t->dvmap);
    delete t;
    return GX_OK;
}

/* Attach / clear a scan-time visibility map: one bit per logical row,
 * ON = tuple hidden (deleted) — the executor-visible semantics of
 * AppendOnlyVisimap_IsVisible (cdbappendonlyvisimap.c:140-210), which
 * every AOCS scan consults per tuple (aocsam.c:1205-1230).  Set it
 * BEFORE gx_q3_prepare so table sizing sees the same row set. */
extern "C" gx_status gx_table_set_visimap(gx_ctx *ctx, gx_table *t,
                                          const uint8_t *bitmap, int64_t nbits)
{
    if (!ctx || !t) return GX_ERR_INVALID;
    if (t->dvmap)
    {
        (void) hipFree(t->dvmap);
        t->dvmap = nullptr;
    }
    if (bitmap)
    {
        if (nbits != t->nrows)
        {
            set_err(ctx, "visimap bits != table rows%s", "");
            return GX_ERR_INVALID;
        }
        int64_t bytes = (nbits + 7) >> 3;
        HIP_CHK(ctx, hipMalloc(&t->dvmap, std::max<int64_t>(bytes, 1)));
        HIP_CHK(ctx, hipMemcpy(t->dvmap, bitmap, bytes, hipMemcpyHostToDevice));
    }
    return GX_OK;
}

extern "C" gx_status gx_table_nrows(const gx_table *t, int64_t *out)
{
    if (!t) return GX_ERR_INVALID;
    *out = t->nrows;
    return GX_OK;
}

extern "C" gx_status gx_table_logical_bytes(const gx_table *t, double *out)
{
    if (!t) return GX_ERR_INVALID;
    double b = 0;
    for (auto &c : t->cols)
        b += (double) c.m.nrows * c.m.width;
    *out = b;
    return GX_OK;
}

/* count/scan/emit helper */
static gx_status scan_counts(gx_ctx *ctx, uint32_t *dcounts, int64_t nthreads,
                             uint64_t **doffs_out, int64_t *total_out)
{
    std::vector<uint32_t> h(nthreads);
    HIP_CHK(ctx, hipMemcpyAsync(h.data(), dcounts, nthreads * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> offs(nthreads);
    uint64_t acc = 0;
    for (int64_t i = 0; i < nthreads; i++) { offs[i] = acc; acc += h[i]; }
    uint64_t *doffs = nullptr;
    HIP_CHK(ctx, hipMalloc(&doffs, nthreads * 8));
    HIP_CHK(ctx, hipMemcpyAsync(doffs, offs.data(), nthreads * 8, hipMemcpyHostToDevice, ctx->stream));
    *doffs_out = doffs;
    *total_out = (int64_t) acc;
    return GX_OK;
}

extern "C" gx_status gx_tpch_gen(gx_ctx *ctx, gx_tpch_table which, double sf,
                                 uint64_t seed, gx_table **out)
{
    if (!ctx) return GX_ERR_INVALID;
    int64_t ncust = (int64_t) (150000.0 * sf + 0.5);
    int64_t nord = (int64_t) (1500000.0 * sf + 0.5);
    int64_t nglobal = (which == GX_TPCH_CUSTOMER) ? ncust : nord;
    bool li_numeric = ((int) which == 3);   /* GX_TPCH_LINEITEM_NUMERIC */
    bool li_rlekey = ((int) which == 4);    /* GX_TPCH_LINEITEM_RLEKEY */
    bool li_q1 = ((int) which == 5);        /* GX_TPCH_LINEITEM_Q1 */
    if (li_numeric || li_rlekey || li_q1) which = GX_TPCH_LINEITEM;
    int64_t nthreads = (nglobal + GEN_CHUNK - 1) / GEN_CHUNK;
    int64_t blocks = std::max<int64_t>((nthreads + TPB - 1) / TPB, 1);
    /* the count kernels write counts[t] for EVERY launched thread */
    int64_t nthreads_alloc = blocks * TPB;
    uint32_t *dcounts = nullptr;
    HIP_CHK(ctx, hipMalloc(&dcounts, std::max<int64_t>(nthreads_alloc, 1) * 4));

    gx_table *t = new gx_table();
    t->ctx = ctx;
    gx_status st = GX_OK;

    if (which == GX_TPCH_CUSTOMER)
    {
        hipLaunchKernelGGL(k_count_cust, dim3(blocks), dim3(TPB), 0, ctx->stream,
                           seed, nglobal, ctx->seg, ctx->nsegs, dcounts);
        uint64_t *doffs; int64_t n;
        st = scan_counts(ctx, dcounts, nthreads, &doffs, &n);
        if (st != GX_OK) { delete t; (void) hipFree(dcounts); return st; }
        int64_t *dkey; uint8_t *dmkt;
        HIP_CHK(ctx, hipMalloc(&dkey, n * 8));
        HIP_CHK(ctx, hipMalloc(&dmkt, std::max<int64_t>(n, 1)));
        hipLaunchKernelGGL(k_emit_cust, dim3(blocks), dim3(TPB), 0, ctx->stream,
                           seed, nglobal, ctx->seg, ctx->nsegs, doffs, dkey, dmkt);
        gx_col c0, c1;
        st = encode_column_device(ctx, dkey, 8, n, &c0);
        if (st == GX_OK) st = encode_column_device(ctx, dmkt, 1, n, &c1);
        HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
        (void) hipFree(dkey); (void) hipFree(dmkt); (void) hipFree(doffs);
        t->cols = {c0, c1};
        t->nrows = n;
    }
    else if (which == GX_TPCH_ORDERS)
    {
        hipLaunchKernelGGL(k_count_ord, dim3(blocks), dim3(TPB), 0, ctx->stream,
                           seed, nglobal, ctx->seg, ctx->nsegs, dcounts);
        uint64_t *doffs; int64_t n;
        st = scan_counts(ctx, dcounts, nthreads, &doffs, &n);
        if (st != GX_OK) { delete t; (void) hipFree(dcounts); return st; }
        int64_t *dok, *doc; int32_t *dod, *dop;
        HIP_CHK(ctx, hipMalloc(&dok, n * 8));
        HIP_CHK(ctx, hipMalloc(&doc, n * 8));
        HIP_CHK(ctx, hipMalloc(&dod, n * 4));
        HIP_CHK(ctx, hipMalloc(&dop, n * 4));
        hipLaunchKernelGGL(k_emit_ord, dim3(blocks), dim3(TPB), 0, ctx->stream,
                           seed, nglobal, ncust, ctx->seg, ctx->nsegs, doffs, dok, doc, dod, dop);
        gx_col c0, c1, c2, c3;
        /* free each flat right after its encode: halves the generator's
         * transient footprint (hipFree synchronizes prior stream work) */
        st = encode_column_device(ctx, dok, 8, n, &c0);
        (void) hipFree(dok);
        if (st == GX_OK) st = encode_column_device(ctx, doc, 8, n, &c1);
        (void) hipFree(doc);
        if (st == GX_OK) st = encode_column_device(ctx, dod, 4, n, &c2);
        (void) hipFree(dod);
        if (st == GX_OK) st = encode_column_device(ctx, dop, 4, n, &c3);
        (void) hipFree(dop);
        HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
        (void) hipFree(doffs);
        t->cols = {c0, c1, c2, c3};
        t->nrows = n;
    }
    else
    {
        hipLaunchKernelGGL(k_count_li, dim3(blocks), dim3(TPB), 0, ctx->stream,
                           seed, nglobal, ctx->seg, ctx->nsegs, dcounts);
        uint64_t *doffs; int64_t n;
        st = scan_counts(ctx, dcounts, nthreads, &doffs, &n);
        if (st != GX_OK) { delete t; (void) hipFree(dcounts); return st; }
        if (li_q1)
        {
            int8_t *dfl, *dst2;
            double *dpr1, *ddi1;
            int32_t *dsh1;
            HIP_CHK(ctx, hipMalloc(&dfl, n));
            HIP_CHK(ctx, hipMalloc(&dst2, n));
            HIP_CHK(ctx, hipMalloc(&dpr1, n * 8));
            HIP_CHK(ctx, hipMalloc(&ddi1, n * 8));
            HIP_CHK(ctx, hipMalloc(&dsh1, n * 4));
            hipLaunchKernelGGL(k_emit_li_q1, dim3(blocks), dim3(TPB), 0, ctx->stream,
                               seed, nglobal, ctx->seg, ctx->nsegs, doffs,
                               dfl, dst2, dpr1, ddi1, dsh1);
            gx_col q0, q1c, q2, q3c, q4;
            st = encode_column_device(ctx, dfl, 1, n, &q0);
            (void) hipFree(dfl);
            if (st == GX_OK) st = encode_column_device(ctx, dst2, 1, n, &q1c);
            (void) hipFree(dst2);
            if (st == GX_OK) st = encode_column_device(ctx, dpr1, 8, n, &q2);
            (void) hipFree(dpr1);
            if (st == GX_OK) st = encode_column_device(ctx, ddi1, 8, n, &q3c);
            (void) hipFree(ddi1);
            if (st == GX_OK) st = encode_column_device(ctx, dsh1, 4, n, &q4);
            (void) hipFree(dsh1);
            HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
            (void) hipFree(doffs); (void) hipFree(dcounts);
            if (st != GX_OK) { gx_table_free(t); return st; }
            t->cols = {q0, q1c, q2, q3c, q4};
            t->nrows = n;
            *out = t;
            return GX_OK;
        }
        int64_t *dlk; double *dpr, *ddi; int32_t *dsh;
        HIP_CHK(ctx, hipMalloc(&dlk, n * 8));
        HIP_CHK(ctx, hipMalloc(&dpr, n * 8));
        HIP_CHK(ctx, hipMalloc(&ddi, n * 8));
        HIP_CHK(ctx, hipMalloc(&dsh, n * 4));
        if (li_numeric)
            hipLaunchKernelGGL(k_emit_li_num, dim3(blocks), dim3(TPB), 0, ctx->stream,
                               seed, nglobal, ctx->seg, ctx->nsegs, doffs, dlk,
                               (int64_t *) dpr, (int64_t *) ddi, dsh);
        else
            hipLaunchKernelGGL(k_emit_li, dim3(blocks), dim3(TPB), 0, ctx->stream,
                               seed, nglobal, ctx->seg, ctx->nsegs, doffs, dlk, dpr, ddi, dsh);
        gx_col c0, c1, c2, c3;
        if (li_rlekey)
        {
            /* keys → host, RLE-encode, re-upload with a block directory */
            std::vector<int64_t> hkeys(n);
            HIP_CHK(ctx, hipMemcpyAsync(hkeys.data(), dlk, n * 8,
                                        hipMemcpyDeviceToHost, ctx->stream));
            HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
            std::vector<uint8_t> stream_bytes;
            host_rle_encode((const uint8_t *) hkeys.data(), 8, n, 32768, stream_bytes);
            std::vector<gx_blockref> dir;
            int64_t rows = 0;
            if (parse_block_dir(stream_bytes.data(), (int64_t) stream_bytes.size(),
                                dir, &rows, &c0.has_null, &c0.fused_ok) != GX_OK ||
                rows != n)
            { set_err(ctx, "rle self-encode mismatch%s", ""); delete t; (void) hipFree(dcounts); return GX_ERR_INVALID; }
            c0.format = 1;
            c0.nblocks = (int64_t) dir.size();
            c0.m.width = 8;
            c0.m.rpb = gx_aocs_rows_per_block(8, 32768);
            c0.m.nrows = n;
            c0.m.full_block_len = gx_aocs_block_len(8, c0.m.rpb);
            c0.m.nbytes = (int64_t) stream_bytes.size();
            gx_colmeta_finish(&c0.m);
            HIP_CHK(ctx, hipMalloc(&c0.dstream, stream_bytes.size()));
            HIP_CHK(ctx, hipMalloc(&c0.ddir, dir.size() * sizeof(gx_blockref)));
            HIP_CHK(ctx, hipMemcpyAsync(c0.dstream, stream_bytes.data(),
                                        stream_bytes.size(), hipMemcpyHostToDevice,
                                        ctx->stream));
            HIP_CHK(ctx, hipMemcpyAsync(c0.ddir, dir.data(),
                                        dir.size() * sizeof(gx_blockref),
                                        hipMemcpyHostToDevice, ctx->stream));
            /* stream_bytes/dir are block-local: drain the copies before
             * they go out of scope */
            HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
        }
        else
            st = encode_column_device(ctx, dlk, 8, n, &c0);
        /* free each flat right after its encode: halves the generator's
         * transient footprint — SF1000 (206 GB of tables) now fits one
         * GPU's 288 GiB (hipFree synchronizes prior stream work) */
        (void) hipFree(dlk);
        if (st == GX_OK) st = encode_column_device(ctx, dpr, 8, n, &c1);
        (void) hipFree(dpr);
        if (st == GX_OK) st = encode_column_device(ctx, ddi, 8, n, &c2);
        (void) hipFree(ddi);
        if (st == GX_OK) st = encode_column_device(ctx, dsh, 4, n, &c3);
        (void) hipFree(dsh);
        HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
        (void) hipFree(doffs);
        t->cols = {c0, c1, c2, c3};
        t->nrows = n;
    }
    (void) hipFree(dcounts);
    HIP_CHK(ctx, hipGetLastError());
    if (st != GX_OK) { gx_table_free(t); return st; }
    *out = t;
    return GX_OK;
}

/* copy a column's raw device stream back to the host (parity testing:
 * byte-compare the GPU encoder against the oracle/reference writer) */
extern "C" gx_status gx_table_dump_stream(gx_ctx *ctx, const gx_table *t,
                                          int col, void *host_out,
                                          int64_t cap_bytes, int64_t *nbytes)
{
    if (!ctx || !t || col < 0 || col >= (int) t->cols.size()) return GX_ERR_INVALID;
    const gx_col &c = t->cols[col];
    if (c.m.nbytes > cap_bytes) return GX_ERR_INVALID;
    HIP_CHK(ctx, hipMemcpyAsync(host_out, c.dstream, c.m.nbytes,
                                hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
    *nbytes = c.m.nbytes;
    return GX_OK;
}

extern "C" gx_status gx_decode_column(gx_ctx *ctx, const gx_table *t, int colidx,
                                      void *host_out, int64_t cap_rows,
                                      int verify_checksums)
{
    if (!ctx || !t || colidx < 0 || colidx >= (int) t->cols.size()) return GX_ERR_INVALID;
    const gx_col &c = t->cols[colidx];
    if (c.m.nrows > cap_rows) return GX_ERR_INVALID;
    int64_t nblocks = (c.m.nrows + c.m.rpb - 1) / c.m.rpb;
    if (c.m.nrows == 0)
    {
        /* empty stream: nothing to decode (reference: zero AO blocks) */
        return GX_OK;
    }
    devbuf dout_b, derr_b;
    HIP_CHK(ctx, dout_b.alloc(c.m.nrows * (int64_t) c.m.width));
    HIP_CHK(ctx, derr_b.alloc(4));
    void *dout = dout_b.p;
    int *derr = derr_b.as<int>();
    HIP_CHK(ctx, hipMemsetAsync(derr, 0, 4, ctx->stream));
    int grid = (int) std::min<int64_t>(nblocks, 65535);
    if (c.format == 1)
    {
        if (c.m.width == 8)
            hipLaunchKernelGGL(k_decode_dense<int64_t>, dim3(GRID), dim3(64), 0, ctx->stream,
                               c.dstream, c.ddir, c.nblocks, c.m.nrows, (int64_t *) dout,
                               (uint8_t *) nullptr, derr);
        else if (c.m.width == 4)
            hipLaunchKernelGGL(k_decode_dense<int32_t>, dim3(GRID), dim3(64), 0, ctx->stream,
                               c.dstream, c.ddir, c.nblocks, c.m.nrows, (int32_t *) dout,
                               (uint8_t *) nullptr, derr);
        else
            hipLaunchKernelGGL(k_decode_dense<int8_t>, dim3(GRID), dim3(64), 0, ctx->stream,
                               c.dstream, c.ddir, c.nblocks, c.m.nrows, (int8_t *) dout,
                               (uint8_t *) nullptr, derr);
        if (verify_checksums)
            hipLaunchKernelGGL(k_verify_crc_dir, dim3(GRID), dim3(64), 0, ctx->stream,
                               c.dstream, c.ddir, c.nblocks, derr);
    }
    else if (c.m.width == 8)
        hipLaunchKernelGGL(k_decode<int64_t>, dim3(grid), dim3(TPB), 0, ctx->stream,
                           c.dstream, nblocks, c.m.full_block_len, c.m.nrows, c.m.rpb,
                           (int64_t *) dout, derr);
    else if (c.m.width == 4)
        hipLaunchKernelGGL(k_decode<int32_t>, dim3(grid), dim3(TPB), 0, ctx->stream,
                           c.dstream, nblocks, c.m.full_block_len, c.m.nrows, c.m.rpb,
                           (int32_t *) dout, derr);
    else
        hipLaunchKernelGGL(k_decode<int8_t>, dim3(grid), dim3(TPB), 0, ctx->stream,
                           c.dstream, nblocks, c.m.full_block_len, c.m.nrows, c.m.rpb,
                           (int8_t *) dout, derr);
    if (verify_checksums && c.format == 0)
        hipLaunchKernelGGL(k_verify_crc, dim3(GRID), dim3(64), 0, ctx->stream,
                           c.dstream, nblocks, c.m.full_block_len, c.m.nrows, c.m.rpb,
                           c.m.width, derr);
    int herr = 0;
    HIP_CHK(ctx, hipMemcpyAsync(host_out, dout, c.m.nrows * (int64_t) c.m.width,
                                hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHK(ctx, hipMemcpyAsync(&herr, derr, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
    HIP_CHK(ctx, hipGetLastError());
    if (herr & 1) { set_err(ctx, "decode: malformed block header%s", ""); return GX_ERR_INVALID; }
    if (herr & 2) { set_err(ctx, "decode: CRC32C mismatch%s", ""); return GX_ERR_CHECKSUM; }
    return GX_OK;
}

/* Varlena (text) Orig block decode — one THREAD per AO block; the walk
 * mirrors the reader's VARSIZE_ANY advance + zero-pad skip
 * (datumstreamblock.h:1509-1545).  pass 0 counts payload bytes per block;
 * pass 1 (with per-block bases from a host scan) writes payload bytes,
 * exclusive offsets and optional validity. */
__global__ void k_decode_varlena(const uint8_t *stream, const gx_blockref *dir,
                                 int64_t nblocks, int64_t nrows,
                                 const int64_t *base,
                                 uint8_t *out_payload, int64_t *out_offsets,
                                 uint8_t *validity, int64_t *blk_bytes,
                                 int pass, int *err)
{
    int64_t t = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    for (int64_t b = t; b < nblocks; b += gridDim.x * (int64_t) blockDim.x)
    {
        const uint8_t *c = stream + dir[b].offset + 24;
        int16_t version = ((const int16_t *) c)[0];
        int16_t flags = ((const int16_t *) c)[1];
        int32_t logical = dir[b].rows;
        if ((version != 0 && version != 1 && version != 2) ||
            dir[b].first_row + logical > nrows ||
            ((flags & 1) && validity == nullptr) || (flags & 4))
        { atomicOr(err, 1); continue; }
        bool rle = false;
        const uint8_t *nbmp = nullptr, *bmp = nullptr, *cnts = nullptr;
        int32_t bmbits = 0, csize = 0, nullbits = 0, psize = 0;
        const uint8_t *p0;
        if (version == 0)
        {
            int16_t nd = ((const int16_t *) c)[2];
            int32_t nullsz = ((const int32_t *) c)[2];
            psize = ((const int32_t *) c)[3];
            if (nd != logical) { atomicOr(err, 1); continue; }
            nullbits = (flags & 1) ? logical : 0;
            nbmp = c + 16;
            p0 = c + 16 + nullsz;
        }
        else
        {
            /* Dense(±RLE) varlena: same section order as fixed-width */
            int32_t hlogical = ((const int32_t *) c)[1];
            psize = ((const int32_t *) c)[3];
            if (hlogical != logical) { atomicOr(err, 1); continue; }
            rle = (flags & 2) != 0;
            const uint8_t *q = c + 16;
            nullbits = (flags & 1) ? logical : 0;
            if (rle)
            {
                int32_t norepeats = ((const int32_t *) q)[0];
                bmbits = ((const int32_t *) q)[1];
                csize = ((const int32_t *) q)[3];
                if (flags & 1) nullbits = norepeats;
                else if (norepeats != 0) { atomicOr(err, 1); continue; }
                q += 16;
            }
            if (flags & 1) { nbmp = q; q += (nullbits + 7) >> 3; }
            if (rle) { bmp = q; q += (bmbits + 7) >> 3; cnts = q; q += csize; }
            int32_t hdr = (int32_t) (q - c);
            p0 = c + ((hdr + 7) & ~7);
        }
        const uint8_t *p = p0, *pend = p0 + psize;
        int64_t w = pass ? base[b] : 0;
        int64_t out = 0;
        int32_t item = 0, coff = 0, npos = 0;
        bool bad = false;
        while (out < logical)
        {
            int64_t row = dir[b].first_row + out;
            if (nbmp != nullptr && nullbits > 0)
            {
                if (npos >= nullbits) { bad = true; break; }
                int nb = (nbmp[npos >> 3] >> (npos & 7)) & 1;
                npos++;
                if (nb)
                {
                    if (pass)
                    {
                        validity[row] = 0;
                        out_offsets[row + 1] = w;
                    }
                    out++;
                    continue;
                }
            }
            if (rle && item >= bmbits) { bad = true; break; }
            if (p < pend && *p == 0)
                p = p0 + (((p - p0) + 3) & ~(int64_t) 3);
            if (p >= pend) { bad = true; break; }
            int64_t len;
            const uint8_t *data;
            if (*p & 1)
            {
                len = (int64_t) (*p >> 1) - 1;
                data = p + 1;
                p += 1 + len;
            }
            else
            {
                uint32_t hdr;
                memcpy(&hdr, p, 4);
                len = (int64_t) (hdr >> 2) - 4;
                data = p + 4;
                p += 4 + len;
            }
            if (len < 0 || p > pend) { bad = true; break; }
            int64_t reps = 1;
            if (rle && (bmp[item >> 3] & (1u << (item & 7))))
            {
                int32_t n = (cnts[coff] >> 6) + 1;
                uint32_t v = cnts[coff] & 0x3F;
                for (int32_t i = 1; i < n; i++) v = (v << 8) | cnts[coff + i];
                coff += n;
                reps += v;
            }
            if (out + reps > logical) { bad = true; break; }
            for (int64_t rr = 0; rr < reps; rr++)
            {
                if (pass)
                {
                    for (int64_t i = 0; i < len; i++)
                        out_payload[w + i] = data[i];
                    if (validity) validity[dir[b].first_row + out] = 1;
                    out_offsets[dir[b].first_row + out + 1] = w + len;
                }
                w += len;
                out++;
            }
            item++;
        }
        if (bad || (rle && (coff != csize || item != bmbits)))
        { atomicOr(err, 1); continue; }
        if (!pass) blk_bytes[b] = w;
    }
}

/* NULL-bearing column decode (aocs_getnext with a null bitmap,
 * datumstreamblock.h:1624-1912 null walk): host_validity gets one byte per
 * row (1 = non-null; null datums decode as zero).  Requires a block-
 * directory column (format 1 — variable geometry). */
extern "C" gx_status gx_decode_column_nullable(gx_ctx *ctx, const gx_table *t,
                                               int colidx, void *host_out,
                                               uint8_t *host_validity,
                                               int64_t cap_rows,
                                               int verify_checksums)
{
    if (!ctx || !t || colidx < 0 || colidx >= (int) t->cols.size()) return GX_ERR_INVALID;
    const gx_col &c = t->cols[colidx];
    if (c.m.nrows > cap_rows) return GX_ERR_INVALID;
    if (c.format != 1)
    { set_err(ctx, "nullable decode requires a block-directory column%s", ""); return GX_ERR_INVALID; }
    devbuf dout_b, dval_b, derr_b;
    HIP_CHK(ctx, dout_b.alloc(c.m.nrows * (int64_t) c.m.width));
    HIP_CHK(ctx, dval_b.alloc(c.m.nrows));
    HIP_CHK(ctx, derr_b.alloc(4));
    int *derr = derr_b.as<int>();
    HIP_CHK(ctx, hipMemsetAsync(derr, 0, 4, ctx->stream));
    if (c.m.width == 8)
        hipLaunchKernelGGL(k_decode_dense<int64_t>, dim3(GRID), dim3(64), 0, ctx->stream,
                           c.dstream, c.ddir, c.nblocks, c.m.nrows,
                           dout_b.as<int64_t>(), dval_b.as<uint8_t>(), derr);
    else if (c.m.width == 4)
        hipLaunchKernelGGL(k_decode_dense<int32_t>, dim3(GRID), dim3(64), 0, ctx->stream,
                           c.dstream, c.ddir, c.nblocks, c.m.nrows,
                           dout_b.as<int32_t>(), dval_b.as<uint8_t>(), derr);
    else
        hipLaunchKernelGGL(k_decode_dense<int8_t>, dim3(GRID), dim3(64), 0, ctx->stream,
                           c.dstream, c.ddir, c.nblocks, c.m.nrows,
                           dout_b.as<int8_t>(), dval_b.as<uint8_t>(), derr);
    if (verify_checksums)
        hipLaunchKernelGGL(k_verify_crc_dir, dim3(GRID), dim3(64), 0, ctx->stream,
                           c.dstream, c.ddir, c.nblocks, derr);
    int herr = 0;
    HIP_CHK(ctx, hipMemcpyAsync(host_out, dout_b.p, c.m.nrows * (int64_t) c.m.width,
                                hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHK(ctx, hipMemcpyAsync(host_validity, dval_b.p, c.m.nrows,
                                hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHK(ctx, hipMemcpyAsync(&herr, derr, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
    HIP_CHK(ctx, hipGetLastError());
    if (herr & 1) { set_err(ctx, "decode: malformed block header%s", ""); return GX_ERR_INVALID; }
    if (herr & 2) { set_err(ctx, "decode: CRC32C mismatch%s", ""); return GX_ERR_CHECKSUM; }
    return GX_OK;
}

/* Varlena (text) column decode: out_offsets[nrows+1] exclusive offsets into
 * out_payload; optional validity byte per row (required when the stream has
 * a NULL bitmap).  Requires a block-directory column with width -1. */
extern "C" gx_status gx_decode_column_varlena(gx_ctx *ctx, const gx_table *t,
                                              int colidx,
                                              int64_t *host_offsets,
                                              void *host_payload,
                                              int64_t payload_cap,
                                              uint8_t *host_validity,
                                              int verify_checksums)
{
    if (!ctx || !t || colidx < 0 || colidx >= (int) t->cols.size()) return GX_ERR_INVALID;
    const gx_col &c = t->cols[colidx];
    if (c.format != 1 || c.m.width >= 0)
    { set_err(ctx, "varlena decode needs a width=-1 directory column%s", ""); return GX_ERR_INVALID; }
    int64_t n = c.m.nrows;
    devbuf dbase_b, doff_b, dval_b, dpay_b, derr_b;
    HIP_CHK(ctx, dbase_b.alloc(std::max<int64_t>(c.nblocks, 1) * 8));
    HIP_CHK(ctx, doff_b.alloc((n + 1) * 8));
    HIP_CHK(ctx, dval_b.alloc(std::max<int64_t>(n, 1)));
    HIP_CHK(ctx, derr_b.alloc(4));
    int *derr = derr_b.as<int>();
    HIP_CHK(ctx, hipMemsetAsync(derr, 0, 4, ctx->stream));
    /* pass 0: per-block payload byte counts */
    hipLaunchKernelGGL(k_decode_varlena, dim3(GRID), dim3(64), 0, ctx->stream,
                       c.dstream, c.ddir, c.nblocks, n,
                       (const int64_t *) nullptr, (uint8_t *) nullptr,
                       (int64_t *) nullptr,
                       host_validity ? dval_b.as<uint8_t>() : nullptr,
                       dbase_b.as<int64_t>(), 0, derr);
    std::vector<int64_t> bases(std::max<int64_t>(c.nblocks, 1));
    HIP_CHK(ctx, hipMemcpyAsync(bases.data(), dbase_b.p, c.nblocks * 8,
                                hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
    int64_t total = 0;
    for (int64_t b = 0; b < c.nblocks; b++)
    {
        int64_t v = bases[b];
        bases[b] = total;
        total += v;
    }
    if (total > payload_cap)
    { set_err(ctx, "varlena payload buffer too small%s", ""); return GX_ERR_INVALID; }
    HIP_CHK(ctx, dpay_b.alloc(std::max<int64_t>(total, 1)));
    HIP_CHK(ctx, hipMemcpyAsync(dbase_b.p, bases.data(), c.nblocks * 8,
                                hipMemcpyHostToDevice, ctx->stream));
    HIP_CHK(ctx, hipMemsetAsync(doff_b.p, 0, 8, ctx->stream));   /* offsets[0] */
    hipLaunchKernelGGL(k_decode_varlena, dim3(GRID), dim3(64), 0, ctx->stream,
                       c.dstream, c.ddir, c.nblocks, n,
                       dbase_b.as<int64_t>(), dpay_b.as<uint8_t>(),
                       doff_b.as<int64_t>(), dval_b.as<uint8_t>(),
                       (int64_t *) nullptr, 1, derr);
    if (verify_checksums)
        hipLaunchKernelGGL(k_verify_crc_dir, dim3(GRID), dim3(64), 0, ctx->stream,
                           c.dstream, c.ddir, c.nblocks, derr);
    int herr = 0;
    HIP_CHK(ctx, hipMemcpyAsync(host_offsets, doff_b.p, (n + 1) * 8,
                                hipMemcpyDeviceToHost, ctx->stream));
    if (total > 0)
        HIP_CHK(ctx, hipMemcpyAsync(host_payload, dpay_b.p, total,
                                    hipMemcpyDeviceToHost, ctx->stream));
    if (host_validity && n > 0)
        HIP_CHK(ctx, hipMemcpyAsync(host_validity, dval_b.p, n,
                                    hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHK(ctx, hipMemcpyAsync(&herr, derr, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
    HIP_CHK(ctx, hipGetLastError());
    if (herr & 1) { set_err(ctx, "varlena decode: malformed block%s", ""); return GX_ERR_INVALID; }
    if (herr & 2) { set_err(ctx, "decode: CRC32C mismatch%s", ""); return GX_ERR_CHECKSUM; }
    return GX_OK;
}

/* Primary filters compare in the COLUMN type (the kernels take a T literal),
 * but the plan's literal is an int64 and the reference evaluates the
 * cross-type operator (int48lt etc.) with the mathematically correct result.
 * Before the literal is narrowed, fold <op, literal> over a width-byte signed
 * column into an equivalent pair whose literal fits the type: an
 * out-of-range literal makes the qual constant, always-true becomes
 * v >= TYPE_MIN and always-false v < TYPE_MIN.  Returns false for an op
 * outside 0..5 (gx_cmp would silently read it as '>='). */
static bool gx_fold_filter(int width, int32_t *op, int64_t *literal)
{
    if (*op < 0 || *op > 5) return false;
    if (width != 1 && width != 4) return true;     /* i64: nothing to narrow */
    const int64_t lo = (width == 1) ? INT8_MIN : INT32_MIN;
    const int64_t hi = (width == 1) ? INT8_MAX : INT32_MAX;
    if (*literal >= lo && *literal <= hi) return true;
    const bool above = *literal > hi;               /* every v < literal */
    bool pass;
    switch (*op)
    {
        case 0: case 4: pass = above; break;        /* v <  lit, v <= lit */
        case 1: case 5: pass = !above; break;       /* v >  lit, v >= lit */
        case 2: pass = false; break;                /* v == lit */
        default: pass = true; break;                /* v != lit */
    }
    *op = pass ? 5 : 0;
    *literal = lo;
    return true;
}

/* TPC-H Q1 core aggregation over a GX_TPCH_LINEITEM_Q1 table: 6 fixed
 * groups (returnflag×linestatus); out arrays of 6: counts, sum_price,
 * sum_revenue.  AVG = sum/count on the caller side (float8_avg = Sx/N). */
extern "C" gx_status gx_q1(gx_ctx *ctx, const gx_table *t, int32_t cutoff,
                           int64_t *counts6, double *sum_price6,
                           double *sum_rev6, double *ms_out)
{
    if (!ctx || !t || t->cols.size() != 5) return GX_ERR_INVALID;
    static const int32_t q1_width[5] = {1, 1, 8, 8, 4};
    for (int c = 0; c < 5; c++)
        if (t->cols[c].format != 0 || t->cols[c].m.width != q1_width[c])
        {
            set_err(ctx, "gx_q1 needs Orig columns [flag i8, status i8, "
                         "price f64, discount f64, shipdate i32]%s", "");
            return GX_ERR_INVALID;
        }
    hipStream_t s = ctx->stream;
    devbuf cnt, spr, srv;
    HIP_CHK(ctx, cnt.alloc(6 * 8));
    HIP_CHK(ctx, spr.alloc(6 * 8));
    HIP_CHK(ctx, srv.alloc(6 * 8));
    HIP_CHK(ctx, hipMemsetAsync(cnt.p, 0, 48, s));
    HIP_CHK(ctx, hipMemsetAsync(spr.p, 0, 48, s));
    HIP_CHK(ctx, hipMemsetAsync(srv.p, 0, 48, s));
    evholder e0, e1;
    HIP_CHK(ctx, e0.create()); HIP_CHK(ctx, e1.create());
    HIP_CHK(ctx, hipEventRecord(e0, s));
    hipLaunchKernelGGL(k_q1_agg, dim3(GRID), dim3(TPB), 0, s,
                       t->cols[0].dstream, t->cols[0].m,
                       t->cols[1].dstream, t->cols[1].m,
                       t->cols[2].dstream, t->cols[2].m,
                       t->cols[3].dstream, t->cols[3].m,
                       t->cols[4].dstream, t->cols[4].m,
                       t->dvmap, cutoff, cnt.as<unsigned long long>(),
                       spr.as<double>(), srv.as<double>());
    HIP_CHK(ctx, hipEventRecord(e1, s));
    HIP_CHK(ctx, hipMemcpyAsync(counts6, cnt.p, 48, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipMemcpyAsync(sum_price6, spr.p, 48, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipMemcpyAsync(sum_rev6, srv.p, 48, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    float ms = 0;
    (void) hipEventElapsedTime(&ms, e0, e1);
    if (ms_out) *ms_out = (double) ms;
    return GX_OK;
}

/* scan+filter count over one column; ms_out = kernel time (HIP events) */
extern "C" gx_status gx_scan_filter(gx_ctx *ctx, const gx_table *t, int col,
                                    int op, int64_t literal,
                                    int64_t *count_out, double *ms_out)
{
    if (!ctx || !t || col < 0 || col >= (int) t->cols.size())
        return GX_ERR_INVALID;
    const gx_col &c = t->cols[col];
    if (c.format != 0) { set_err(ctx, "scan_filter requires fixed-format column%s", ""); return GX_ERR_INVALID; }
    int32_t fop = op;
    if (!gx_fold_filter(c.m.width, &fop, &literal))
    {
        set_err(ctx, "scan_filter: op must be in 0..5%s", "");
        return GX_ERR_INVALID;
    }
    op = fop;
    hipStream_t s = ctx->stream;
    devbuf cnt;
    HIP_CHK(ctx, cnt.alloc(8));
    HIP_CHK(ctx, hipMemsetAsync(cnt.p, 0, 8, s));
    evholder e0, e1;
    HIP_CHK(ctx, e0.create()); HIP_CHK(ctx, e1.create());
    HIP_CHK(ctx, hipEventRecord(e0, s));
    if (c.m.width == 8)
        hipLaunchKernelGGL(k_scan_filter<int64_t>, dim3(GRID), dim3(TPB), 0, s,
                           c.dstream, c.m, t->dvmap, op, (int64_t) literal,
                           cnt.as<unsigned long long>());
    else if (c.m.width == 4)
        hipLaunchKernelGGL(k_scan_filter<int32_t>, dim3(GRID), dim3(TPB), 0, s,
                           c.dstream, c.m, t->dvmap, op, (int32_t) literal,
                           cnt.as<unsigned long long>());
    else
        hipLaunchKernelGGL(k_scan_filter<int8_t>, dim3(GRID), dim3(TPB), 0, s,
                           c.dstream, c.m, t->dvmap, op, (int8_t) literal,
                           cnt.as<unsigned long long>());
    HIP_CHK(ctx, hipEventRecord(e1, s));
    unsigned long long n = 0;
    HIP_CHK(ctx, hipMemcpyAsync(&n, cnt.p, 8, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    float ms = 0;
    (void) hipEventElapsedTime(&ms, e0, e1);
    *count_out = (int64_t) n;
    if (ms_out) *ms_out = (double) ms;
    return GX_OK;
}

/* Standalone hash GROUP BY (nodeAgg.c hash strategy + execGrouping.c
 * NOT-DISTINCT grouping): GROUP BY key_col with COUNT(*) and SUM(val_col).
 * Key col: i64, Orig or Dense/RLE (nullable — all NULL keys form ONE
 * group, returned last with key_is_null=1); val col: f64, same formats
 * (NULL inputs are skipped by SUM, counted by COUNT(*)).  Groups are
 * returned sorted by key; caller frees with gx_free. */
static gx_status hbm_budget_check(gx_ctx *ctx, uint64_t want, const char *what);

static gx_status gb_flat(gx_ctx *ctx, const gx_col &c, devbuf &flat,
                         devbuf &val, const uint8_t **s_out, gx_colmeta *m_out,
                         const uint8_t **val_out)
{
    if (c.format == 0)
    {
        if (c.has_null)
        { set_err(ctx, "null-bearing Orig stream needs format 1 bind%s", ""); return GX_ERR_INVALID; }
        *s_out = c.dstream;
        *m_out = c.m;
        *val_out = nullptr;
        return GX_OK;
    }
    int64_t n = c.m.nrows;
    if (n >= (int64_t) INT32_MAX) return GX_ERR_INVALID;
    devbuf errb;
    HIP_CHK(ctx, flat.alloc((size_t) (GX_AOCS_DATUM_OFF +
                                      std::max<int64_t>(n, 1) * c.m.width)));
    HIP_CHK(ctx, val.alloc((size_t) std::max<int64_t>(n, 1)));
    HIP_CHK(ctx, errb.alloc(4));
    HIP_CHK(ctx, hipMemsetAsync(errb.p, 0, 4, ctx->stream));
    uint8_t *dv = flat.as<uint8_t>() + GX_AOCS_DATUM_OFF;
    if (c.m.width == 8)
        hipLaunchKernelGGL(k_decode_dense<int64_t>, dim3(GRID), dim3(64), 0,
                           ctx->stream, c.dstream, c.ddir, c.nblocks, n,
                           (int64_t *) dv, val.as<uint8_t>(), errb.as<int>());
    else if (c.m.width == 4)
        hipLaunchKernelGGL(k_decode_dense<int32_t>, dim3(GRID), dim3(64), 0,
                           ctx->stream, c.dstream, c.ddir, c.nblocks, n,
                           (int32_t *) dv, val.as<uint8_t>(), errb.as<int>());
    else if (c.m.width == 2)
        hipLaunchKernelGGL(k_decode_dense<int16_t>, dim3(GRID), dim3(64), 0,
                           ctx->stream, c.dstream, c.ddir, c.nblocks, n,
                           (int16_t *) dv, val.as<uint8_t>(), errb.as<int>());
    else
        hipLaunchKernelGGL(k_decode_dense<int8_t>, dim3(GRID), dim3(64), 0,
                           ctx->stream, c.dstream, c.ddir, c.nblocks, n,
                           (int8_t *) dv, val.as<uint8_t>(), errb.as<int>());
    int herr = 0;
    HIP_CHK(ctx, hipMemcpyAsync(&herr, errb.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
    HIP_CHK(ctx, hipGetLastError());
    if (herr) { set_err(ctx, "groupby: malformed block%s", ""); return GX_ERR_INVALID; }
    gx_colmeta m{};
    m.width = c.m.width;
    m.rpb = (int32_t) std::max<int64_t>(n, 1);
    m.nrows = n;
    m.full_block_len = GX_AOCS_DATUM_OFF + n * c.m.width;
    m.nbytes = m.full_block_len;
    gx_colmeta_finish(&m);
    *s_out = flat.as<uint8_t>();
    *m_out = m;
    *val_out = c.has_null ? val.as<uint8_t>() : nullptr;
    return GX_OK;
}

/* device hash-agg state: SoA open-addressing table (biased keys, sentinel
 * 0) plus the separate NULL-group accumulators (nacc: [sum f64, count u64])
 * and the error flag.  Shared by the one-stage agg, the partial agg and the
 * combine agg of the two-stage plan. */
struct gb_table {
    devbuf kflat, kval, vflat, vval;   /* flattened Dense/RLE inputs */
    devbuf tk, ts, tc, nacc, errb;
    uint64_t tslots = 0;
    int64_t cap = 0;                   /* most groups the table can hold */
};

/* budget-check, allocate and clear a table for up to n input rows */
static gx_status gb_table_alloc(gx_ctx *ctx, gb_table &T, int64_t n,
                                const char *what)
{
    hipStream_t s = ctx->stream;
    uint64_t tslots = (uint64_t) pow2_at_least(n * 2);
    T.tslots = tslots;
    T.cap = std::min<int64_t>((int64_t) tslots, std::max<int64_t>(n, 1));
    gx_status bs = hbm_budget_check(ctx, tslots * 24 + (uint64_t) T.cap * 24 + 64,
                                    what);
    if (bs != GX_OK) return bs;
    HIP_CHK(ctx, T.tk.alloc(tslots * 8));
    HIP_CHK(ctx, T.ts.alloc(tslots * 8));
    HIP_CHK(ctx, T.tc.alloc(tslots * 8));
    HIP_CHK(ctx, T.nacc.alloc(16));
    HIP_CHK(ctx, T.errb.alloc(4));
    HIP_CHK(ctx, hipMemsetAsync(T.tk.p, 0, tslots * 8, s));
    HIP_CHK(ctx, hipMemsetAsync(T.ts.p, 0, tslots * 8, s));
    HIP_CHK(ctx, hipMemsetAsync(T.tc.p, 0, tslots * 8, s));
    HIP_CHK(ctx, hipMemsetAsync(T.nacc.p, 0, 16, s));
    HIP_CHK(ctx, hipMemsetAsync(T.errb.p, 0, 4, s));
    return GX_OK;
}

/* scan key_col/val_col of t into a fresh table (enqueue only, no sync) */
static gx_status gb_build(gx_ctx *ctx, const gx_table *t, int key_col,
                          int val_col, gb_table &T)
{
    if (!ctx || !t || key_col < 0 || key_col >= (int) t->cols.size() ||
        val_col < 0 || val_col >= (int) t->cols.size())
        return GX_ERR_INVALID;
    const gx_col &kc = t->cols[key_col], &vc = t->cols[val_col];
    if (kc.m.width != 8 || vc.m.width != 8) return GX_ERR_INVALID;
    const uint8_t *k_s, *v_s, *k_val, *v_val;
    gx_colmeta k_m, v_m;
    gx_status st = gb_flat(ctx, kc, T.kflat, T.kval, &k_s, &k_m, &k_val);
    if (st != GX_OK) return st;
    st = gb_flat(ctx, vc, T.vflat, T.vval, &v_s, &v_m, &v_val);
    if (st != GX_OK) return st;
    st = gb_table_alloc(ctx, T, t->nrows, "groupby table");
    if (st != GX_OK) return st;
    hipLaunchKernelGGL(k_groupby, dim3(GRID), dim3(TPB), 0, ctx->stream,
                       k_s, k_m, k_val, v_s, v_m, v_val, t->dvmap,
                       T.tk.as<unsigned long long>(), T.ts.as<double>(),
                       T.tc.as<unsigned long long>(), T.tslots - 1,
                       T.nacc.as<double>(),
                       T.nacc.as<unsigned long long>() + 1, T.errb.as<int>());
    return GX_OK;
}

/* compact a table's groups on device, bring them to the host, sort by key
 * asc and append the NULL group last; ev_done (optional) is recorded after
 * the last kernel.  Caller frees *out with gx_free. */
static gx_status gb_extract_sorted(gx_ctx *ctx, gb_table &T, hipEvent_t ev_done,
                                   gx_kv_group **out, int64_t *ngroups)
{
    hipStream_t s = ctx->stream;
    uint64_t tslots = T.tslots;
    devbuf &tk = T.tk, &ts = T.ts, &tc = T.tc, &nacc = T.nacc, &errb = T.errb;
    /* device-side compaction: only the actual groups travel to the host
     * (the slot table itself can be tens of GB at SF-scale inputs) */
    int64_t cap = T.cap;
    devbuf ok_b, os_b, oc_b, cur_b;
    HIP_CHK(ctx, ok_b.alloc((size_t) cap * 8));
    HIP_CHK(ctx, os_b.alloc((size_t) cap * 8));
    HIP_CHK(ctx, oc_b.alloc((size_t) cap * 8));
    HIP_CHK(ctx, cur_b.alloc(8));
    HIP_CHK(ctx, hipMemsetAsync(cur_b.p, 0, 8, s));
    hipLaunchKernelGGL(k_kv_extract, dim3(GRID), dim3(TPB), 0, s,
                       tk.as<unsigned long long>(), ts.as<double>(),
                       tc.as<unsigned long long>(), tslots,
                       ok_b.as<unsigned long long>(), os_b.as<double>(),
                       oc_b.as<unsigned long long>(),
                       cur_b.as<unsigned long long>());
    if (ev_done) HIP_CHK(ctx, hipEventRecord(ev_done, s));
    int herr = 0;
    double nsum = 0;
    unsigned long long ncnt = 0, ng = 0;
    HIP_CHK(ctx, hipMemcpyAsync(&ng, cur_b.p, 8, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipMemcpyAsync(&nsum, nacc.p, 8, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipMemcpyAsync(&ncnt, (char *) nacc.p + 8, 8, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipMemcpyAsync(&herr, errb.p, 4, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    if (herr & 4)
    { set_err(ctx, "groupby: key INT64_MIN unsupported (biased sentinel)%s", ""); return GX_ERR_INVALID; }
    if ((int64_t) ng > cap)
    { set_err(ctx, "groupby: extract overflow%s", ""); return GX_ERR_INVALID; }
    std::vector<unsigned long long> hk(ng), hc(ng);
    std::vector<double> hs(ng);
    if (ng)
    {
        HIP_CHK(ctx, hipMemcpyAsync(hk.data(), ok_b.p, ng * 8, hipMemcpyDeviceToHost, s));
        HIP_CHK(ctx, hipMemcpyAsync(hs.data(), os_b.p, ng * 8, hipMemcpyDeviceToHost, s));
        HIP_CHK(ctx, hipMemcpyAsync(hc.data(), oc_b.p, ng * 8, hipMemcpyDeviceToHost, s));
        HIP_CHK(ctx, hipStreamSynchronize(s));
    }

    std::vector<gx_kv_group> groups;
    groups.reserve((size_t) ng);
    for (uint64_t i = 0; i < ng; i++)
    {
        gx_kv_group g{};
        g.key = (int64_t) (hk[i] ^ (1ULL << 63));
        g.sum = hs[i];
        g.count = (int64_t) hc[i];
        groups.push_back(g);
    }
    std::sort(groups.begin(), groups.end(),
              [](const gx_kv_group &a, const gx_kv_group &b)
              { return a.key < b.key; });
    if (ncnt)
    {
        gx_kv_group g{};
        g.key_is_null = 1;
        g.sum = nsum;
        g.count = (int64_t) ncnt;
        groups.push_back(g);
    }
    *ngroups = (int64_t) groups.size();
    *out = (gx_kv_group *) malloc(std::max<size_t>(groups.size(), 1) *
                                  sizeof(gx_kv_group));
    if (!*out) return GX_ERR_OOM;
    memcpy(*out, groups.data(), groups.size() * sizeof(gx_kv_group));
    return GX_OK;
}

extern "C" gx_status gx_groupby(gx_ctx *ctx, const gx_table *t, int key_col,
                                int val_col, gx_kv_group **out,
                                int64_t *ngroups)
{
    if (!out || !ngroups) return GX_ERR_INVALID;
    gb_table T;
    gx_status st = gb_build(ctx, t, key_col, val_col, T);
    if (st != GX_OK) return st;
    return gb_extract_sorted(ctx, T, nullptr, out, ngroups);
}

/* ---- two-stage GROUP BY: partial agg → hash Motion → combine agg ----
 * (cdbgroupingpaths.c:251 plan shape; nodeAgg.c:2305,2321 combine step) */

/* destination of the NULL-key group: cdbhash of one NULL int8 attribute is
 * the rotation of the init value only (cdbhash.c:189-247) */
static int gb_null_dest(int nsegs)
{
    int64_t v = 0;
    uint8_t isnull = 1;
    return gx_jump_consistent_hash(
        (uint64_t) gx_cdbhash_multi(&v, &isnull, nullptr, 1), nsegs);
}

static void gb_part_hist(gx_ctx *ctx, gb_table &T, int nsegs,
                         unsigned long long *dhist)
{
    hipLaunchKernelGGL(k_gb_part_hist, dim3(GRID), dim3(TPB),
                       (size_t) nsegs * 8, ctx->stream,
                       T.tk.as<unsigned long long>(), T.tslots,
                       T.nacc.as<unsigned long long>() + 1,
                       gb_null_dest(nsegs), nsegs, dhist);
}

static void gb_part_emit(gx_ctx *ctx, gb_table &T, int nsegs,
                         unsigned long long *dcur, gx_kv_group *dsend)
{
    hipLaunchKernelGGL(k_gb_part_emit, dim3(GRID), dim3(TPB),
                       (size_t) nsegs * 16, ctx->stream,
                       T.tk.as<unsigned long long>(), T.ts.as<double>(),
                       T.tc.as<unsigned long long>(), T.tslots,
                       T.nacc.as<double>(),
                       T.nacc.as<unsigned long long>() + 1,
                       gb_null_dest(nsegs), nsegs, dcur, dsend);
}

/* combine stage over n device-resident partial rows */
static gx_status gb_combine(gx_ctx *ctx, const gx_kv_group *drows, int64_t n,
                            hipEvent_t ev_done, gx_kv_group **out,
                            int64_t *ngroups)
{
    gb_table T;
    gx_status st = gb_table_alloc(ctx, T, n, "groupby combine table");
    if (st != GX_OK) return st;
    hipLaunchKernelGGL(k_gb_combine, dim3(GRID), dim3(TPB), 0, ctx->stream,
                       drows, n, T.tk.as<unsigned long long>(),
                       T.ts.as<double>(), T.tc.as<unsigned long long>(),
                       T.tslots - 1, T.nacc.as<double>(),
                       T.nacc.as<unsigned long long>() + 1, T.errb.as<int>());
    return gb_extract_sorted(ctx, T, ev_done, out, ngroups);
}

extern "C" gx_status gx_groupby_dist(gx_ctx *ctx, const gx_table *t,
                                     int key_col, int val_col,
                                     gx_kv_group **out, int64_t *ngroups,
                                     gx_gb_stats *stats)
{
    if (!ctx || !t || !out || !ngroups) return GX_ERR_INVALID;
    /* one-stage plan: the group key needs no redistribution on a single
     * segment.  GX_FORCE_MOTION=1 routes a single-segment run through the
     * full exchange branch, as in gx_q3_run. */
    bool one_stage = ctx->nsegs == 1 && env_int("GX_FORCE_MOTION", 0) == 0;
    if (!one_stage && !ctx->comm)
    { set_err(ctx, "nsegs>1 but gx_comm_init not called%s", ""); return GX_ERR_STATE; }
    gx_gb_stats S{};
    S.rows_in = t->nrows;
    hipStream_t s = ctx->stream;
    evholder ev[7];
    for (auto &e : ev) HIP_CHK(ctx, e.create());
    auto ms_between = [](hipEvent_t a, hipEvent_t b) {
        float ms = 0;
        (void) hipEventElapsedTime(&ms, a, b);
        return (double) ms;
    };

    if (one_stage)
    {
        gb_table T;
        HIP_CHK(ctx, hipEventRecord(ev[0], s));
        gx_status st = gb_build(ctx, t, key_col, val_col, T);
        if (st != GX_OK) return st;
        st = gb_extract_sorted(ctx, T, ev[1], out, ngroups);
        if (st != GX_OK) return st;
        S.ms_partial = ms_between(ev[0], ev[1]);
        S.partial_groups = S.final_groups = *ngroups;
        if (stats) *stats = S;
        return GX_OK;
    }

    int n = ctx->nsegs;
    if (n > GB_MAX_SEGS)
    { set_err(ctx, "groupby_dist: more segments than the partition kernels' LDS histogram holds%s", ""); return GX_ERR_INVALID; }

    /* stage 1: partial agg — the groups stay on the device */
    gb_table T;
    HIP_CHK(ctx, hipEventRecord(ev[0], s));
    gx_status st = gb_build(ctx, t, key_col, val_col, T);
    if (st != GX_OK) return st;
    HIP_CHK(ctx, hipEventRecord(ev[1], s));

    /* stage 2: partition.  The per-destination histogram goes straight
     * into the all-gather, so ONE host sync yields both this rank's send
     * layout (its own row) and every peer's counts. */
    devbuf hist_b, cur_b, all_b;
    HIP_CHK(ctx, hist_b.alloc(n * 8));
    HIP_CHK(ctx, cur_b.alloc(n * 8));
    HIP_CHK(ctx, all_b.alloc((size_t) n * n * 8));
    unsigned long long *dhist = hist_b.as<unsigned long long>();
    HIP_CHK(ctx, hipMemsetAsync(dhist, 0, n * 8, s));
    gb_part_hist(ctx, T, n, dhist);
    HIP_CHK(ctx, hipEventRecord(ev[2], s));
    RCCL_CHK(ctx, ncclAllGather(dhist, all_b.p, n, ncclUint64, ctx->comm, s));
    std::vector<unsigned long long> cnts_all((size_t) n * n);
    int herr = 0;
    HIP_CHK(ctx, hipMemcpyAsync(cnts_all.data(), all_b.p, (size_t) n * n * 8,
                                hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipMemcpyAsync(&herr, T.errb.p, 4, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    const gx_mlayout L = m_exchange_layout(cnts_all.data(), n, ctx->seg);
    unsigned long long send_n = L.send_n, recv_n = L.recv_n;
    if ((int64_t) send_n > T.cap + 1)
    { set_err(ctx, "groupby_dist: partition overflow%s", ""); return GX_ERR_INVALID; }
    st = hbm_budget_check(ctx, (send_n + recv_n) * sizeof(gx_kv_group) + 64,
                          "groupby exchange buffers");
    if (st != GX_OK) return st;
    devbuf send_b, recv_b;
    HIP_CHK(ctx, send_b.alloc(send_n * sizeof(gx_kv_group)));
    HIP_CHK(ctx, recv_b.alloc(recv_n * sizeof(gx_kv_group)));
    gx_kv_group *send = send_b.as<gx_kv_group>(), *recv = recv_b.as<gx_kv_group>();
    HIP_CHK(ctx, hipMemcpyAsync(cur_b.p, L.soff.data(), n * 8, hipMemcpyHostToDevice, s));
    HIP_CHK(ctx, hipEventRecord(ev[3], s));
    gb_part_emit(ctx, T, n, cur_b.as<unsigned long long>(), send);
    HIP_CHK(ctx, hipEventRecord(ev[4], s));

    /* stage 3: exchange */
    st = m_exchange_payload(ctx, s, send, recv, L, sizeof(gx_kv_group));
    if (st != GX_OK) return st;
    HIP_CHK(ctx, hipEventRecord(ev[5], s));
    /* a rejected key is reported only now, after this rank's sends and
     * receives are enqueued, so the peers' matching calls still complete */
    if (herr & 4)
    {
        HIP_CHK(ctx, hipStreamSynchronize(s));
        set_err(ctx, "groupby: key INT64_MIN unsupported (biased sentinel)%s", "");
        return GX_ERR_INVALID;
    }

    /* stage 4: combine agg over the received partial states */
    st = gb_combine(ctx, recv, (int64_t) recv_n, ev[6], out, ngroups);
    if (st != GX_OK) return st;

    S.ms_partial = ms_between(ev[0], ev[1]);
    S.ms_partition = ms_between(ev[1], ev[2]) + ms_between(ev[3], ev[4]);
    S.ms_exchange = ms_between(ev[2], ev[3]) + ms_between(ev[4], ev[5]);
    S.ms_combine = ms_between(ev[5], ev[6]);
    S.partial_groups = S.sent_rows = (int64_t) send_n;
    S.recv_rows = (int64_t) recv_n;
    S.final_groups = *ngroups;
    if (stats) *stats = S;
    return GX_OK;
}

/* Test ABI: partial agg + partition kernels on one GPU for a given nsegs,
 * returning the packed wire rows and per-destination counts to the host. */
extern "C" gx_status gx_test_gb_partial(gx_ctx *ctx, const gx_table *t,
                                        int key_col, int val_col, int nsegs,
                                        int64_t *out_counts /* nsegs */,
                                        gx_kv_group *out_rows /* cap */,
                                        int64_t cap, int64_t *out_total)
{
    if (!ctx || !t || nsegs < 1 || nsegs > GB_MAX_SEGS || !out_counts ||
        !out_total || cap < 0 ||
        (cap > 0 && !out_rows))
        return GX_ERR_INVALID;
    hipStream_t s = ctx->stream;
    gb_table T;
    gx_status st = gb_build(ctx, t, key_col, val_col, T);
    if (st != GX_OK) return st;
    devbuf hist_b, cur_b, send_b;
    HIP_CHK(ctx, hist_b.alloc(nsegs * 8));
    HIP_CHK(ctx, cur_b.alloc(nsegs * 8));
    HIP_CHK(ctx, hipMemsetAsync(hist_b.p, 0, nsegs * 8, s));
    gb_part_hist(ctx, T, nsegs, hist_b.as<unsigned long long>());
    std::vector<unsigned long long> h(nsegs), off(nsegs + 1, 0);
    int herr = 0;
    HIP_CHK(ctx, hipMemcpyAsync(h.data(), hist_b.p, nsegs * 8, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipMemcpyAsync(&herr, T.errb.p, 4, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    if (herr & 4)
    { set_err(ctx, "groupby: key INT64_MIN unsupported (biased sentinel)%s", ""); return GX_ERR_INVALID; }
    for (int i = 0; i < nsegs; i++) off[i + 1] = off[i] + h[i];
    int64_t total = (int64_t) off[nsegs];
    if (total > cap)
    { set_err(ctx, "gb_partial: output capacity too small%s", ""); return GX_ERR_INVALID; }
    st = hbm_budget_check(ctx, (uint64_t) total * sizeof(gx_kv_group) + 64,
                          "groupby exchange buffers");
    if (st != GX_OK) return st;
    HIP_CHK(ctx, send_b.alloc((size_t) total * sizeof(gx_kv_group)));
    HIP_CHK(ctx, hipMemcpyAsync(cur_b.p, off.data(), nsegs * 8, hipMemcpyHostToDevice, s));
    gb_part_emit(ctx, T, nsegs, cur_b.as<unsigned long long>(),
                 send_b.as<gx_kv_group>());
    if (total)
        HIP_CHK(ctx, hipMemcpyAsync(out_rows, send_b.p,
                                    (size_t) total * sizeof(gx_kv_group),
                                    hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    for (int i = 0; i < nsegs; i++) out_counts[i] = (int64_t) h[i];
    *out_total = total;
    return GX_OK;
}

/* Test ABI: the combine stage over host-supplied partial rows */
extern "C" gx_status gx_test_gb_combine(gx_ctx *ctx, const gx_kv_group *rows,
                                        int64_t n, gx_kv_group **out,
                                        int64_t *ngroups)
{
    if (!ctx || n < 0 || (n > 0 && !rows) || !out || !ngroups)
        return GX_ERR_INVALID;
    devbuf rows_b;
    HIP_CHK(ctx, rows_b.alloc((size_t) n * sizeof(gx_kv_group)));
    if (n)
        HIP_CHK(ctx, hipMemcpyAsync(rows_b.p, rows, (size_t) n * sizeof(gx_kv_group),
                                    hipMemcpyHostToDevice, ctx->stream));
    return gb_combine(ctx, rows_b.as<gx_kv_group>(), n, nullptr, out, ngroups);
}

extern "C" gx_status gx_partition(gx_ctx *ctx, const int64_t *host_keys, int64_t n,
                                  int32_t nsegs, int32_t *host_out)
{
    if (!ctx || n < 0) return GX_ERR_INVALID;
    devbuf dk, dr;
    HIP_CHK(ctx, dk.alloc(n * 8));
    HIP_CHK(ctx, dr.alloc(n * 4));
    HIP_CHK(ctx, hipMemcpyAsync(dk.p, host_keys, n * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_route, dim3(GRID), dim3(TPB), 0, ctx->stream,
                       dk.as<int64_t>(), n, nsegs, dr.as<int32_t>());
    HIP_CHK(ctx, hipMemcpyAsync(host_out, dr.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
    HIP_CHK(ctx, hipGetLastError());
    return GX_OK;
}

/* multi-column distribution-key routing (cdbhash.c:189-247 rotate-combine +
 * REDUCE_JUMP_HASH) — bit-exact with the oracle's orc_route_multi_batch.
 * vals/isnull row-major n×nkeys; types[k]: 0 = int8, 1 = int4/date.
 * isnull may be NULL (all NOT NULL). */
extern "C" gx_status gx_partition_multi(gx_ctx *ctx, const int64_t *host_vals,
                                        const uint8_t *host_isnull,
                                        const int32_t *host_types,
                                        int32_t nkeys, int64_t n, int32_t nsegs,
                                        int32_t *host_out)
{
    if (!ctx || n < 0 || nkeys < 1 || nkeys > 32) return GX_ERR_INVALID;
    devbuf dv, dn, dt, dr;
    HIP_CHK(ctx, dv.alloc(n * nkeys * 8));
    HIP_CHK(ctx, dt.alloc(nkeys * 4));
    HIP_CHK(ctx, dr.alloc(n * 4));
    HIP_CHK(ctx, hipMemcpyAsync(dv.p, host_vals, n * nkeys * 8,
                                hipMemcpyHostToDevice, ctx->stream));
    HIP_CHK(ctx, hipMemcpyAsync(dt.p, host_types, nkeys * 4,
                                hipMemcpyHostToDevice, ctx->stream));
    if (host_isnull)
    {
        HIP_CHK(ctx, dn.alloc(n * nkeys));
        HIP_CHK(ctx, hipMemcpyAsync(dn.p, host_isnull, n * nkeys,
                                    hipMemcpyHostToDevice, ctx->stream));
    }
    hipLaunchKernelGGL(k_route_multi, dim3(GRID), dim3(TPB), 0, ctx->stream,
                       dv.as<int64_t>(), dn.as<uint8_t>(), dt.as<int32_t>(),
                       nkeys, n, nsegs, dr.as<int32_t>());
    HIP_CHK(ctx, hipMemcpyAsync(host_out, dr.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
    HIP_CHK(ctx, hipGetLastError());
    return GX_OK;
}

/* ================= Q3 ================= */

/* Evaluate the constant TEXT dim predicate ONCE over the varlena column
 * (device two-pass decode + texteq) into a per-row match mask; the
 * per-step customer scans then run on the fast fixed-width path. */
static gx_status q3_build_text_mask(gx_ctx *ctx, gx_q3 *q)
{
    const gx_col &cm = q->cust->cols[q->desc.dim_filter.col];
    int64_t n = cm.m.nrows;
    hipStream_t s = ctx->stream;
    devbuf derrb;
    HIP_CHK(ctx, derrb.alloc(4));
    int *derr = derrb.as<int>();
    HIP_CHK(ctx, hipMemsetAsync(derr, 0, 4, s));
    HIP_CHK(ctx, q->dmask.alloc((size_t) n));
    /* single pass, one texteq per RLE run — no payload materialization
     * (the r1 path decoded the whole column first: 510 ms at SF100) */
    hipLaunchKernelGGL(k_texteq_mask_blocks, dim3(GRID), dim3(64), 0, s,
                       cm.dstream, cm.ddir, cm.nblocks, n,
                       q->dtext.as<uint8_t>(), q->desc.dim_text_len,
                       q->dmask.as<uint8_t>(), derr);
    int herr = 0;
    HIP_CHK(ctx, hipMemcpyAsync(&herr, derr, 4, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    if (herr)
    {
        set_err(ctx, "malformed varlena dim column%s", "");
        return GX_ERR_INVALID;
    }
    return GX_OK;
}

/* role-column accessor: materialized flat override or the bound column */
static inline const gx_col &q3_col(const gx_q3 *q, const gx_table *t, int c)
{
    auto it = q->mat.find(std::make_pair((const gx_table *) t, c));
    return it != q->mat.end() ? it->second : t->cols[c];
}

/* ensure a per-table hidden bitmap exists (seeded from the visimap) */
static gx_status q3_ensure_hidden(gx_ctx *ctx, gx_table *t, devbuf *hidden);

/* Decode a Dense/RLE (possibly null-bearing) ROLE column once at prepare
 * into a flat device array readable through the standard gx_col_get
 * addressing (rpb >= nrows -> always block 0, datums at +GX_AOCS_DATUM_OFF),
 * and OR its NULL rows into the table's hidden mask: strict-NULL reject for
 * join keys (nodeHash.c:2168-2181), NULL-qual filtering for filter columns
 * (execScan.c:241).  The per-step kernels run unchanged. */
static gx_status q3_materialize_col(gx_ctx *ctx, gx_q3 *q, gx_table *t,
                                    int cidx, devbuf *hidden,
                                    bool fold_nulls = true,
                                    devbuf *val_out = nullptr)
{
    const gx_col &c = t->cols[cidx];
    int64_t n = c.m.nrows;
    int w = c.m.width;
    if (n >= (int64_t) INT32_MAX)
    {
        set_err(ctx, "materialized column too large (rpb is int32)%s", "");
        return GX_ERR_INVALID;
    }
    hipStream_t st = ctx->stream;
    devbuf flat, val, errb;
    HIP_CHK(ctx, flat.alloc((size_t) (GX_AOCS_DATUM_OFF +
                                      std::max<int64_t>(n, 1) * w)));
    HIP_CHK(ctx, val.alloc((size_t) std::max<int64_t>(n, 1)));
    HIP_CHK(ctx, errb.alloc(4));
    HIP_CHK(ctx, hipMemsetAsync(errb.p, 0, 4, st));
    uint8_t *dvals = flat.as<uint8_t>() + GX_AOCS_DATUM_OFF;
    if (w == 8)
        hipLaunchKernelGGL(k_decode_dense<int64_t>, dim3(GRID), dim3(64), 0, st,
                           c.dstream, c.ddir, c.nblocks, n,
                           (int64_t *) dvals, val.as<uint8_t>(), errb.as<int>());
    else if (w == 4)
        hipLaunchKernelGGL(k_decode_dense<int32_t>, dim3(GRID), dim3(64), 0, st,
                           c.dstream, c.ddir, c.nblocks, n,
                           (int32_t *) dvals, val.as<uint8_t>(), errb.as<int>());
    else
        hipLaunchKernelGGL(k_decode_dense<int8_t>, dim3(GRID), dim3(64), 0, st,
                           c.dstream, c.ddir, c.nblocks, n,
                           (int8_t *) dvals, val.as<uint8_t>(), errb.as<int>());
    hipLaunchKernelGGL(k_verify_crc_dir, dim3(GRID), dim3(64), 0, st,
                       c.dstream, c.ddir, c.nblocks, errb.as<int>());
    int herr = 0;
    HIP_CHK(ctx, hipMemcpyAsync(&herr, errb.p, 4, hipMemcpyDeviceToHost, st));
    HIP_CHK(ctx, hipStreamSynchronize(st));
    HIP_CHK(ctx, hipGetLastError());
    if (herr & 1) { set_err(ctx, "materialize: malformed block%s", ""); return GX_ERR_INVALID; }
    if (herr & 2) { set_err(ctx, "materialize: CRC32C mismatch%s", ""); return GX_ERR_CHECKSUM; }
    if (c.has_null && fold_nulls)
    {
        gx_status rs = q3_ensure_hidden(ctx, t, hidden);
        if (rs != GX_OK) return rs;
        hipLaunchKernelGGL(k_validity_or_hidden, dim3(GRID), dim3(TPB), 0, st,
                           val.as<uint8_t>(), n, hidden->as<uint8_t>());
        HIP_CHK(ctx, hipStreamSynchronize(st));
        HIP_CHK(ctx, hipGetLastError());
    }
    gx_col oc{};
    oc.dstream = flat.as<uint8_t>();
    oc.m.width = w;
    oc.m.rpb = (int32_t) std::max<int64_t>(n, 1);
    oc.m.nrows = n;
    oc.m.full_block_len = GX_AOCS_DATUM_OFF + n * w;
    oc.m.nbytes = GX_AOCS_DATUM_OFF + n * w;
    gx_colmeta_finish(&oc.m);
    oc.format = 0;
    oc.has_null = c.has_null;    /* sizing consults this (NOTIN emptiness) */
    q->mat[std::make_pair((const gx_table *) t, cidx)] = oc;
    q->mat_mem.push_back(std::move(flat));
    if (val_out)                 /* the caller wants the per-row validity */
        *val_out = std::move(val);
    return GX_OK;
}

/* LEFT OUTER restriction (gpuexec.h gx_q3_prepare_desc): the unmatched-group
 * table stores keys biased by 2^63 with 0 as its empty-slot mark and 2^63 as
 * the NULL-key group, so a non-NULL fact key INT64_MIN or 0 has no slot of
 * its own.  Reject both here, by name, instead of dropping or merging rows.
 * validity: the fact key's per-row validity when it was materialized. */
static gx_status q3_check_outer_fact_keys(gx_ctx *ctx, gx_q3 *q,
                                          const uint8_t *validity)
{
    const gx_col &lk = q3_col(q, q->li, q->desc.fact_key_col);
    hipStream_t s = ctx->stream;
    devbuf cb;
    HIP_CHK(ctx, cb.alloc(16));
    HIP_CHK(ctx, hipMemsetAsync(cb.p, 0, 16, s));
    hipLaunchKernelGGL(k_col_count_reserved, dim3(GRID), dim3(TPB), 0, s,
                       lk.dstream, lk.m, validity,
                       cb.as<unsigned long long>());
    unsigned long long hc[2] = {0, 0};
    HIP_CHK(ctx, hipMemcpyAsync(hc, cb.p, 16, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    if (hc[1])
    {
        set_err(ctx, "LEFT OUTER: fact key INT64_MIN "
                     "(-9223372036854775808) is the unmatched table's "
                     "empty-slot mark (gpuexec.h gx_q3_prepare_desc)%s", "");
        return GX_ERR_INVALID;
    }
    if (hc[0])
    {
        set_err(ctx, "LEFT OUTER: non-NULL fact key 0 would be filed into "
                     "the NULL-key group (gpuexec.h gx_q3_prepare_desc)%s", "");
        return GX_ERR_INVALID;
    }
    return GX_OK;
}

/* fold an AND-ed extra-qual list into a device HIDDEN bitmap (combined with
 * the table's visimap); runs once at prepare — the per-step kernels then
 * read one bit per row through the existing visibility path.  q resolves the
 * quals' columns (q3_col) and may be null only when nq == 0. */
static gx_status q3_build_qualmask(gx_ctx *ctx, gx_q3 *q, gx_table *t,
                                   const gx_filter *quals, int nq,
                                   devbuf *out)
{
    gx_qualargs qa{};
    qa.n = nq;
    for (int i = 0; i < nq; i++)
    {
        int c = quals[i].col;
        if (c < 0 || c >= (int) t->cols.size())
        {
            set_err(ctx, "extra qual column out of range%s", "");
            return GX_ERR_INVALID;
        }
        /* materialized (formerly format-1) role columns qualify too —
         * materialization runs BEFORE the qual masks */
        const gx_col &col = q3_col(q, t, c);
        if (col.format != 0 || quals[i].op < 0 || quals[i].op > 5 ||
            (col.m.width != 1 && col.m.width != 4 && col.m.width != 8))
        {
            set_err(ctx, "extra qual needs a fixed-width Orig column and "
                         "op in 0..5%s", "");
            return GX_ERR_INVALID;
        }
        qa.s[i] = col.dstream;
        qa.m[i] = col.m;
        qa.op[i] = quals[i].op;
        qa.lit[i] = quals[i].literal;
    }
    /* a hidden mask may already exist (NULL folds from materialization):
     * the quals are then AND-ed in, IN PLACE (seed == output is
     * element-aliased); otherwise the visimap seeds a new one */
    const uint8_t *seed = out->p ? out->as<uint8_t>() : t->dvmap;
    if (!out->p)
        HIP_CHK(ctx, out->alloc((size_t) ((t->nrows + 7) >> 3)));
    hipLaunchKernelGGL(k_qualmask, dim3(GRID), dim3(TPB), 0, ctx->stream,
                       qa, seed, t->nrows, out->as<uint8_t>());
    HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
    HIP_CHK(ctx, hipGetLastError());
    return GX_OK;
}

static gx_status q3_ensure_hidden(gx_ctx *ctx, gx_table *t, devbuf *hidden)
{
    if (hidden->p) return GX_OK;
    /* no quals: copies the visimap (or zeros); q is not needed then */
    return q3_build_qualmask(ctx, nullptr, t, nullptr, 0, hidden);
}

extern "C" gx_status gx_q3_prepare_desc(gx_ctx *ctx, const gx_q3_desc *desc,
                                        gx_q3 **out)
{
    if (!ctx || !desc || !desc->dim || !desc->mid || !desc->fact)
        return GX_ERR_INVALID;
    gx_table *customer = desc->dim, *orders = desc->mid, *lineitem = desc->fact;
    auto colw = [](gx_table *t, int c) {
        return (c >= 0 && c < (int) t->cols.size()) ? t->cols[c].m.width : -1;
    };
    bool dim_text = desc->dim_text_len > 0;
    if (dim_text &&
        (desc->dim_text_len > (int32_t) sizeof(desc->dim_text) ||
         desc->dim_filter.op != 2 ||
         colw(customer, desc->dim_filter.col) != -1 ||
         customer->cols[desc->dim_filter.col].format != 1))
    {
        set_err(ctx, "TEXT dim filter needs op '==' on a varlena dir column%s", "");
        return GX_ERR_INVALID;
    }
    if (colw(customer, desc->dim_key_col) != 8 ||
        (!dim_text && colw(customer, desc->dim_filter.col) != 1) ||
        colw(orders, desc->mid_key_col) != 8 ||
        colw(orders, desc->mid_fk_col) != 8 ||
        colw(orders, desc->mid_attr1_col) != 4 ||
        colw(orders, desc->mid_attr2_col) != 4 ||
        colw(orders, desc->mid_filter.col) != 4 ||
        colw(lineitem, desc->fact_key_col) != 8 ||
        colw(lineitem, desc->fact_a_col) != 8 ||
        colw(lineitem, desc->fact_b_col) != 8 ||
        colw(lineitem, desc->fact_filter.col) != 4)
    {
        set_err(ctx, "gx_q3_desc: column role/width mismatch%s", "");
        return GX_ERR_INVALID;
    }
    if (desc->mid_filter.col != desc->mid_attr1_col &&
        desc->mid_filter.col == desc->mid_key_col)
        return GX_ERR_INVALID;
    /* format-1 (Dense/RLE/null-bearing) columns: the fused probe scans RLE
     * on the fact key directly (no-null); other KEY/FILTER role columns are
     * materialized to flat arrays at prepare with strict-NULL reject;
     * measure/attr roles must be plain fixed-width */
    auto is_matable = [&](gx_table *t, int ci) {
        if (t == customer) return ci == desc->dim_key_col ||
                                  (!dim_text && ci == desc->dim_filter.col);
        if (t == orders) return ci == desc->mid_key_col ||
                                ci == desc->mid_fk_col ||
                                ci == desc->mid_filter.col;
        return ci == desc->fact_key_col || ci == desc->fact_filter.col;
    };
    auto is_used = [&](gx_table *t, int ci) {
        if (t == customer) return ci == desc->dim_key_col ||
                                  ci == desc->dim_filter.col;
        if (t == orders) return ci == desc->mid_key_col ||
                                ci == desc->mid_fk_col ||
                                ci == desc->mid_attr1_col ||
                                ci == desc->mid_attr2_col ||
                                ci == desc->mid_filter.col;
        return ci == desc->fact_key_col || ci == desc->fact_a_col ||
               ci == desc->fact_b_col || ci == desc->fact_filter.col;
    };
    /* the one column the fused RLE probe scans in place: an inner join's
     * NULL-free fact key whose every block the kernel reads (classified at
     * bind, gx_col.fused_ok).  Orig, DELTA and over-wide blocks send the
     * column down the materialize route with the NULL-bearing ones. */
    auto is_fused_key = [&](gx_table *t, int ci) {
        const gx_col &c = t->cols[ci];
        return t == lineitem && ci == desc->fact_key_col && c.format == 1 &&
               !c.has_null && c.fused_ok && desc->fact_join == 0;
    };
    for (auto *t : {customer, orders, lineitem})
        for (size_t ci = 0; ci < t->cols.size(); ci++)
        {
            const gx_col &c = t->cols[ci];
            if (c.format == 0 || !is_used(t, (int) ci)) continue;
            if (dim_text && t == customer && (int) ci == desc->dim_filter.col)
                continue;                              /* varlena texteq path */
            if (is_fused_key(t, (int) ci))
                continue;                              /* fused RLE scan */
            if (!is_matable(t, (int) ci))
            {
                set_err(ctx, "Dense/RLE/null-bearing streams are supported on "
                             "key and filter roles (materialized at prepare) "
                             "and the fact key (fused RLE); decode "
                             "measure/attr columns first%s", "");
                return GX_ERR_INVALID;
            }
        }
    gx_q3 *q = new gx_q3();
    q->ctx = ctx;
    q->cust = customer;
    q->ord = orders;
    q->li = lineitem;
    q->desc = *desc;
    /* every primary-filter launch reads q->desc: fold the literals into the
     * column types here, once (the TEXT dim filter carries no literal) */
    if ((!dim_text && !gx_fold_filter(1, &q->desc.dim_filter.op,
                                      &q->desc.dim_filter.literal)) ||
        !gx_fold_filter(4, &q->desc.mid_filter.op, &q->desc.mid_filter.literal) ||
        !gx_fold_filter(4, &q->desc.fact_filter.op, &q->desc.fact_filter.literal))
    {
        set_err(ctx, "gx_q3_desc: primary filter op must be in 0..5%s", "");
        delete q;
        return GX_ERR_INVALID;
    }
    if (dim_text)
    {
        hipError_t e = q->dtext.alloc(desc->dim_text_len);
        if (e == hipSuccess)
            e = hipMemcpy(q->dtext.p, desc->dim_text, desc->dim_text_len,
                          hipMemcpyHostToDevice);
        if (e != hipSuccess) { delete q; return GX_ERR_OOM; }
        gx_status st = q3_build_text_mask(ctx, q);
        if (st != GX_OK)
        {
            delete q;
            return st;
        }
    }
    /* extra AND-ed qual lists → per-table hidden bitmaps */
    if (desc->fact_join < 0 || desc->fact_join > 1 ||
        desc->dim_join < 0 || desc->dim_join > 2 ||
        desc->n_dim_extra < 0 || desc->n_dim_extra > GX_MAX_EXTRA_QUALS ||
        desc->n_mid_extra < 0 || desc->n_mid_extra > GX_MAX_EXTRA_QUALS ||
        desc->n_fact_extra < 0 || desc->n_fact_extra > GX_MAX_EXTRA_QUALS)
    {
        gx_q3_free(q);
        return GX_ERR_INVALID;
    }
    struct { gx_table *t; const gx_filter *qs; int nq; devbuf *dst; } ex[3] = {
        {customer, desc->dim_extra, desc->n_dim_extra, &q->qvm_dim},
        {orders, desc->mid_extra, desc->n_mid_extra, &q->qvm_mid},
        {lineitem, desc->fact_extra, desc->n_fact_extra, &q->qvm_fact},
    };
    /* materialize format-1 key/filter role columns FIRST (strict-NULL
     * reject seeds the hidden masks; the qual masks then AND into them
     * and may reference the materialized columns) */
    devbuf fact_key_val;                /* LEFT OUTER fact key validity */
    for (auto &e : ex)                  /* table/mask trio */
        for (size_t ci = 0; ci < e.t->cols.size(); ci++)
        {
            const gx_col &c = e.t->cols[ci];
            if (c.format == 0 || !is_used(e.t, (int) ci) ||
                !is_matable(e.t, (int) ci))
                continue;
            if (is_fused_key(e.t, (int) ci))
                continue;               /* fused RLE path */
            /* join-variety NULL rules (nodeHashjoin.c:425,442,652-659):
             * - LASJ (anti): a NULL mid fk never matches the dim set, so
             *   the row PASSES — do NOT hide it; its decoded 0 misses the
             *   set (0 is the rejected sentinel) and the anti test keeps it
             * - LASJ_NOTIN: a NULL DIM key empties the result — do not
             *   hide such rows either; sizing sees the decoded 0 on a
             *   has_null column and flags q->empty */
            bool fold = true;
            if (desc->dim_join == 1 && e.t == orders &&
                (int) ci == desc->mid_fk_col)
                fold = false;
            if (desc->dim_join == 2 && e.t == customer &&
                (int) ci == desc->dim_key_col)
                fold = false;
            /* LEFT OUTER keeps fact rows that fail the ON clause: a NULL
             * fact key never matches, so the row EMITS with NULL attrs
             * (decoded 0 -> the NULL-key group) — do not hide it */
            bool outer_key = desc->fact_join == 1 && e.t == lineitem &&
                             (int) ci == desc->fact_key_col;
            if (outer_key)
                fold = false;
            gx_status st = q3_materialize_col(ctx, q, e.t, (int) ci, e.dst,
                                              fold,
                                              outer_key ? &fact_key_val
                                                        : nullptr);
            if (st != GX_OK)
            {
                gx_q3_free(q);
                return st;
            }
        }
    if (desc->fact_join == 1)
    {
        gx_status st = q3_check_outer_fact_keys(ctx, q,
                                                fact_key_val.as<uint8_t>());
        if (st != GX_OK)
        {
            gx_q3_free(q);
            return st;
        }
    }
    /* AND-ed extra qual lists → per-table hidden bitmaps */
    for (auto &e : ex)
        if (e.nq > 0)
        {
            gx_status st = q3_build_qualmask(ctx, q, e.t, e.qs, e.nq, e.dst);
            if (st != GX_OK)
            {
                gx_q3_free(q);
                return st;
            }
        }
    *out = q;
    return GX_OK;
}

/* classic entry: the standard Q3 column layout and filters */
extern "C" gx_status gx_q3_prepare(gx_ctx *ctx, gx_table *customer, gx_table *orders,
                                   gx_table *lineitem, int32_t cutoff, gx_q3 **out)
{
    if (!customer || !orders || !lineitem) return GX_ERR_INVALID;
    if (customer->cols.size() != 2 || orders->cols.size() != 4 ||
        lineitem->cols.size() != 4) return GX_ERR_INVALID;
    gx_q3_desc d{};
    d.dim = customer;
    d.dim_key_col = 0;
    d.dim_filter = {1, 2, 0};              /* c_mktsegment = BUILDING */
    d.mid = orders;
    d.mid_key_col = 0;
    d.mid_fk_col = 1;
    d.mid_attr1_col = 2;
    d.mid_attr2_col = 3;
    d.mid_filter = {2, 0, cutoff};         /* o_orderdate < cutoff */
    d.fact = lineitem;
    d.fact_key_col = 0;
    d.fact_a_col = 1;
    d.fact_b_col = 2;
    d.fact_filter = {3, 1, cutoff};        /* l_shipdate > cutoff */
    return gx_q3_prepare_desc(ctx, &d, out);
}

/* HBM-budget guard: the reference batches/spills when the
 * build side exceeds its memory budget (ExecChooseHashTableSize nodeHash.c:812,
 * batch split nodeHashjoin.c:1355); the GPU path instead sizes up front and
 * REJECTS with the numbers in the message before allocating — no silent
 * fallback (GX_ERR_NOGPU semantics: callers must fail, not fall back).
 * GX_HBM_BUDGET_MB overrides the free-memory query (tests). */
static gx_status hbm_budget_check(gx_ctx *ctx, uint64_t want, const char *what)
{
    size_t free_b = 0, total_b = 0;
    HIP_CHK(ctx, hipMemGetInfo(&free_b, &total_b));
    long mb = env_int("GX_HBM_BUDGET_MB", 0);
    uint64_t budget = mb > 0 ? (uint64_t) mb << 20
                             : (uint64_t) free_b - ((uint64_t) free_b >> 4);
    if (want > budget)
    {
        char buf[200];
        snprintf(buf, sizeof buf,
                 "%s needs %.2f GB but HBM budget is %.2f GB (free %.2f of "
                 "%.2f GB); reduce the build side or add segments",
                 what, want / 1073741824.0, budget / 1073741824.0,
                 free_b / 1073741824.0, total_b / 1073741824.0);
        set_err(ctx, "%s", buf);
        return GX_ERR_OOM;
    }
    return GX_OK;
}

/* The customer scans, as the Q3 run and the test entry points launch them.
 * dmask != nullptr selects the flat-mask row predicate, otherwise the int8
 * compare <op, literal> on column cm. */
struct q3_dimscan {
    const gx_col &ck, &cm;           /* key column, filter column */
    const uint8_t *dmask;
    int32_t op;
    int64_t literal;
    const uint8_t *cvm;              /* effective visibility */
};

template <typename F>
static inline void by_dim_pred(const q3_dimscan &sc, F &&f)
{
    if (sc.dmask) f(gx_dim_pred_mask{sc.dmask});
    else f(gx_dim_pred_cmp{sc.cm.dstream, sc.cm.m, sc.op, (int8_t) sc.literal});
}

static void dim_launch_count(hipStream_t s, const q3_dimscan &sc,
                             unsigned long long *count,
                             unsigned long long *maxkey,
                             unsigned long long *minkey)
{
    by_dim_pred(sc, [&](auto pred) {
        hipLaunchKernelGGL(k_cust_count<decltype(pred)>,
                           dim3(GRID), dim3(TPB), 0, s,
                           sc.ck.dstream, sc.ck.m, pred, sc.cvm, count, maxkey,
                           minkey);
    });
}

/* Clear and fill the membership structure the caller's path reads: the
 * bitmap (no key set: one set-width instantiation), or bloom + the
 * width-byte key set.  Only that one is touched; the other keeps whatever
 * it held. */
static gx_status dim_launch_build(gx_ctx *ctx, hipStream_t s,
                                  const q3_dimscan &sc, const q3_dimset &ds,
                                  bool bitmap)
{
    if (bitmap)
        HIP_CHK(ctx, hipMemsetAsync(ds.bits.p, 0, (ds.range + 63) / 64 * 8, s));
    else
    {
        HIP_CHK(ctx, hipMemsetAsync(ds.set.p, 0, (ds.cmask + 1) * ds.width, s));
        HIP_CHK(ctx, hipMemsetAsync(ds.bloom.p, 0, (ds.bwmask + 1) * 8, s));
    }
    by_dim_pred(sc, [&](auto pred) {
        auto go = [&](auto *cs, auto bmode) {
            hipLaunchKernelGGL((k_cust_build<std::decay_t<decltype(*cs)>,
                                             decltype(bmode)::value,
                                             decltype(pred)>),
                               dim3(GRID), dim3(TPB), 0, s,
                               sc.ck.dstream, sc.ck.m, pred, sc.cvm, cs, ds.cmask,
                               ds.bloom.as<unsigned long long>(), ds.bwmask,
                               bitmap ? ds.bits.as<unsigned long long>() : nullptr,
                               ds.kmin, ds.range);
        };
        if (bitmap)
            go((unsigned int *) nullptr, std::true_type{});
        else
            by_width(ds.width, ds.set.p,
                     [&](auto *cs) { go(cs, std::false_type{}); });
    });
    return GX_OK;
}

/* the dim scan of a q: its role columns, filter and effective visibility
 * (the extra-qual mask already holds the visimap) */
static q3_dimscan q3_dim_scan(const gx_q3 *q)
{
    const gx_q3_desc &D = q->desc;
    return {q3_col(q, q->cust, D.dim_key_col),
            q3_col(q, q->cust, D.dim_filter.col),
            D.dim_text_len > 0 ? q->dmask.as<uint8_t>() : nullptr,
            D.dim_filter.op, D.dim_filter.literal,
            q->qvm_dim.p ? q->qvm_dim.as<uint8_t>() : q->cust->dvmap};
}

/* Bound on the LEFT-OUTER unmatched groups of a fact key column with nrows
 * rows whose raw keys, reduced as UNSIGNED words (k_col_minmax), span
 * [lmin, lmax]: distinct keys <= min(nrows, span), plus one for the NULL-key
 * group.  The span lmax - lmin + 1 is computed modulo 2^64: a column holding
 * both 0 and -1 (2^64-1) spans all 2^64 values and the sum wraps to 0, so a
 * zero span (or inverted stats) falls back to nrows, which always bounds the
 * distinct count.  Pure host function; gx_selftest_unmatched_bound. */
static uint64_t q3_unmatched_bound(int64_t nrows, uint64_t lmin, uint64_t lmax)
{
    if (nrows <= 0) return 1;
    uint64_t span = lmax - lmin + 1;
    if (lmax < lmin || span == 0) span = (uint64_t) nrows;
    return std::min<uint64_t>((uint64_t) nrows, span) + 1;
}

/* (Re)allocate the hash-form join/agg table of tslots slots of
 * q->tbl.width-byte keys and the result arrays for qual groups plus the
 * LEFT-OUTER bound, freeing what was there.  The Motion path calls it at its
 * first run and whenever a run's exchanged counts outgrow the cached table;
 * the local path allocates the two halves separately (results at sizing, the
 * table at the first hash-form run). */
static gx_status q3_alloc_results(gx_q3 *q, int64_t qual);
static gx_status q3_alloc_hash(gx_ctx *ctx, q3_hashtbl &t, uint64_t tslots);

static gx_status q3_alloc_table(gx_q3 *q, uint64_t tslots, int64_t qual)
{
    gx_status st = q3_alloc_hash(q->ctx, q->tbl, tslots);
    if (st != GX_OK) return st;
    return q3_alloc_results(q, qual);
}

/* The result arrays are shared by both table forms and both paths: they
 * never hold fewer than the local path's sizing asked for (local_qual), so a
 * re-allocation by the Motion path leaves a later local run valid. */
static gx_status q3_alloc_results(gx_q3 *q, int64_t qual)
{
    HIP_CHK(q->ctx, q->res.alloc(std::max<int64_t>(
                        std::max(qual, q->local_qual) + q->un.cap, 1)));
    return GX_OK;
}

/* the hash form's storage: tslots slots of t.width-byte keys, replacing what
 * t held */
static gx_status q3_alloc_hash(gx_ctx *ctx, q3_hashtbl &t, uint64_t tslots)
{
    t.keys.reset(); t.attrs.reset(); t.aggs.reset();
    gx_status st = hbm_budget_check(
        ctx, tslots * (t.width + sizeof(gx_attrpair) + sizeof(gx_aggslot)),
        "join/agg table");
    if (st != GX_OK) return st;
    HIP_CHK(ctx, t.keys.alloc(tslots * t.width));
    HIP_CHK(ctx, t.attrs.alloc(tslots * sizeof(gx_attrpair)));
    HIP_CHK(ctx, t.aggs.alloc(tslots * sizeof(gx_aggslot)));
    t.mask = tslots - 1;
    return GX_OK;
}

/* Whether sizing may pick the rank form (gx_rankview) for qual qualifying
 * mid rows whose keys span [kmin, kmax]: at least one row, a range of at
 * most 64 keys per row (the density rule of the interpolation layout and of
 * the dim bitmap: bits, prefix counts and dense payload then cost at most
 * 16 B more per row than the payload alone), fewer than 2^32 rows (u32
 * prefix counts) and the switch not off.  Pure host function;
 * gx_selftest_rank_eligible. */
static bool q3_rank_eligible(int64_t qual, uint64_t kmin, uint64_t kmax,
                             int enabled)
{
    if (!enabled || qual <= 0 || kmax < kmin) return false;
    if ((uint64_t) qual >= (1ULL << 32)) return false;
    uint64_t span = kmax - kmin;       /* range - 1: cannot wrap */
    return span < 64 * (uint64_t) qual;
}

/* Which form the rank-form orders stage takes for qual qualifying of nrows
 * mid rows: staged (k_orders_mark<STAGE>, k_orders_fill_staged) where at
 * most one row in GX_ORDERS_STAGE_K qualifies, two-pass (rowmask,
 * k_orders_fill) above.  The staged form saves the second walk over the mid
 * table and pays 32 B of staging traffic per qualifying row; the threshold
 * is where the SF100 sweep stops showing a win
 * (profiles/orders_stage_ab.json).  env is GX_ORDERS_STAGED: 0 or 1 forces
 * a form, anything negative (unset) means the rule.  Pure host function;
 * gx_selftest_orders_staged. */
static constexpr int64_t GX_ORDERS_STAGE_K = 4;
static bool q3_orders_staged(int64_t qual, int64_t nrows, int env)
{
    if (env >= 0) return env != 0;
    if (qual < 0 || nrows < 0) return false;
    return qual <= nrows / GX_ORDERS_STAGE_K;   /* qual * K <= nrows, no product */
}

/* Mark grid of the staged form: enough row iterations per wave that the
 * records a wave expects (64 x selectivity each) fill three quarters of its
 * LDS segment, so nearly every block ends with ONE cursor claim and a
 * mid-loop flush is rare.  At 10 % and 256 records that is 30 iterations,
 * 19.5 k blocks at SF100.  Never fewer blocks than fill the machine a few
 * times over (unless the table is smaller), never more than 2^20. */
static int64_t q3_stage_grid(int64_t qual, int64_t nrows)
{
    int64_t rowblocks = std::max<int64_t>((nrows + TPB - 1) / TPB, 1);
    int64_t iters = qual > 0
        ? (int64_t) ((3.0 * GX_STAGE_WAVE_RECS / 4.0) * (double) nrows /
                     (64.0 * (double) qual))
        : rowblocks;
    iters = std::max<int64_t>(iters, 1);
    int64_t blocks = (rowblocks + iters - 1) / iters;
    blocks = std::max<int64_t>(blocks, std::min<int64_t>(rowblocks, 8192));
    return std::min<int64_t>(blocks, 1 << 20);
}

/* first rank-form run of a q: allocate the rank storage.  What only one
 * form of the orders stage needs (rowmask; staging records) is allocated by
 * that form's first run. */
static gx_status q3_alloc_rank(gx_ctx *ctx, q3_ranktbl &r, uint64_t qual)
{
    uint64_t nwords = r.nwords();
    uint64_t nblk = (nwords + GX_RANK_SCAN_WORDS - 1) / GX_RANK_SCAN_WORDS;
    r.ent.reset(); r.blk.reset();               /* a failed earlier try */
    r.dkey.reset(); r.dattr.reset(); r.dagg.reset();
    gx_status st = hbm_budget_check(
        ctx,
        nwords * 16 + nblk * 4 +
            qual * (r.kw + sizeof(gx_attrpair) + sizeof(gx_aggslot)),
        "rank join/agg table");
    if (st != GX_OK) return st;
    HIP_CHK(ctx, r.ent.alloc(nwords * sizeof(ulonglong2)));
    HIP_CHK(ctx, r.blk.alloc(nblk * 4));
    HIP_CHK(ctx, r.dkey.alloc(qual * r.kw));
    HIP_CHK(ctx, r.dattr.alloc(qual * sizeof(gx_attrpair)));
    HIP_CHK(ctx, r.dagg.alloc(qual * sizeof(gx_aggslot)));
    return GX_OK;
}

/* first two-pass run of a q: the per-row mask */
static gx_status q3_alloc_rowmask(gx_q3 *q)
{
    gx_ctx *ctx = q->ctx;
    uint64_t mwords = ((uint64_t) q->ord->nrows + 63) / 64;
    gx_status st = hbm_budget_check(ctx, mwords * 8, "orders row mask");
    if (st != GX_OK) return st;
    HIP_CHK(ctx, q->rank.rowmask.alloc(mwords * 8));
    return GX_OK;
}

/* first staged run of a q: local_qual staging records (sizing counted
 * qualifying ROWS, so they all fit while the input is what it was) and the
 * cursor pair */
static gx_status q3_alloc_stage(gx_q3 *q)
{
    gx_ctx *ctx = q->ctx;
    uint64_t cap = (uint64_t) q->local_qual;
    q->rank.stage.reset(); q->rank.stage_cur.reset();   /* a failed earlier try */
    gx_status st = hbm_budget_check(ctx, cap * sizeof(ulonglong2) + 16,
                                    "orders staging records");
    if (st != GX_OK) return st;
    HIP_CHK(ctx, q->rank.stage.alloc(cap * sizeof(ulonglong2)));
    HIP_CHK(ctx, q->rank.stage_cur.alloc(16));
    return GX_OK;
}

/* max over ranks of one word; v is left alone on a single segment */
static gx_status comm_max_u64(gx_ctx *ctx, hipStream_t s, uint64_t &v)
{
    if (!(ctx->nsegs > 1 && ctx->comm)) return GX_OK;
    devbuf w;
    HIP_CHK(ctx, w.alloc(8));
    unsigned long long hv = v;
    HIP_CHK(ctx, hipMemcpyAsync(w.p, &hv, 8, hipMemcpyHostToDevice, s));
    RCCL_CHK(ctx, ncclAllReduce(w.p, w.p, 1, ncclUint64, ncclMax, ctx->comm, s));
    HIP_CHK(ctx, hipMemcpyAsync(&hv, w.p, 8, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    v = hv;
    return GX_OK;
}

/* Dimension set layout for n_building filtered rows whose keys span
 * [cmin, cmax] (pure host): 4-byte set slots when every key fits, two slots
 * per key, 8 bloom bits per key (at least 4096 words).  Dense keys (range
 * <= 64 per qualifying key: the bitmap is then never larger than the 8 B/key
 * u32 set) on a single segment get the exact bitmap as well, unless the
 * switch is off. */
struct gx_dim_layout {
    int width;
    uint64_t cslots, bwords;
    int bitmap;
    uint64_t kmin, range;
};

static gx_dim_layout q3_dim_layout(uint64_t n_building, uint64_t cmin,
                                   uint64_t cmax, int nsegs, bool bitmap_on)
{
    gx_dim_layout L;
    L.width = (cmax < (1ULL << 32)) ? 4 : 8;
    L.cslots = (uint64_t) pow2_at_least((int64_t) n_building * 2);
    L.bwords = (uint64_t) pow2_at_least(
        std::max<int64_t>((int64_t) n_building * 8 / 64, 4096));
    uint64_t drange = (n_building > 0 && cmax >= cmin) ? cmax - cmin + 1 : 0;
    L.bitmap = nsegs == 1 && drange > 0 && drange <= 64 * n_building && bitmap_on;
    L.kmin = L.bitmap ? cmin : 0;
    L.range = L.bitmap ? drange : 0;
    return L;
}

/* Count the filtered dim rows, check key 0, size, allocate and build the
 * membership structures: what sizing does for a q and what the test entry
 * points do for one rank's dim set.  bwords_fixed != 0 stands in for the
 * bloom size the ranks would agree on.  state: 0 built, 1 empty (NOTIN with
 * a NULL inner key, nodeHashjoin.c:442; nothing is allocated).  At nsegs>1
 * the key-0 / NOTIN-NULL / over-budget verdict must be GLOBAL and agreed by
 * every rank BEFORE any early return — a lone rank bailing out of sizing
 * while its peers continue into the collectives would hang the job. */
static gx_status q3_dim_size_build(gx_ctx *ctx, hipStream_t s,
                                   const q3_scratch &sc, const q3_dimscan &scan,
                                   bool notin_null, bool bitmap_on,
                                   uint64_t bwords_fixed, q3_dimset &ds,
                                   int *state, int64_t *nsel = nullptr)
{
    q3_keystats ks;
    gx_status st = q3_read_keystats(
        ctx, s, sc, ks, [&](auto *count, auto *kmax, auto *kmin) {
            dim_launch_count(s, scan, count, kmax, kmin);
        });
    if (st != GX_OK) return st;
    /* 2: invalid (real key 0 vs the slot sentinel) */
    uint64_t verdict = 0;
    if (ks.count > 0 && ks.kmin == 0) verdict = notin_null ? 1 : 2;
    const gx_dim_layout L = q3_dim_layout(ks.count, ks.kmin, ks.kmax,
                                          ctx->nsegs, bitmap_on);
    const uint64_t want = L.cslots * L.width + L.bwords * 8 +
                          (L.range + 63) / 64 * 8;
    if (verdict == 0 &&
        hbm_budget_check(ctx, want, "dim semijoin set") != GX_OK)
        verdict = 3;                   /* over budget — agree collectively */
    st = comm_max_u64(ctx, s, verdict);
    if (st != GX_OK) return st;
    *state = (int) verdict;
    if (verdict == 1) return GX_OK;
    if (verdict == 2)
    {
        /* slot value 0 is the empty-slot sentinel (keys start at 1 in every
         * PG sequence-keyed table); a real key 0 would be silently dropped.
         * All ranks agree on this verdict, so everyone errors together. */
        set_err(ctx, "dim join key 0 found: 0 is reserved as the empty-slot "
                     "sentinel (gpuexec.h gx_q3_prepare_desc)%s", "");
        return GX_ERR_INVALID;
    }
    if (verdict == 3)
    {
        /* re-derive the message on every rank (the verdict is global) */
        st = hbm_budget_check(ctx, want, "dim semijoin set");
        if (st != GX_OK) return st;
        set_err(ctx, "dim semijoin set over HBM budget on a peer rank%s", "");
        return GX_ERR_OOM;
    }
    if (nsel) *nsel = (int64_t) ks.count;
    ds.width = L.width;
    ds.bitmap = L.bitmap;
    ds.kmin = L.kmin;
    ds.range = L.range;
    HIP_CHK(ctx, ds.set.alloc(L.cslots * L.width));
    ds.cmask = L.cslots - 1;
    /* the Motion-1 destination-bloom prefilter all-gathers every rank's
     * bloom — sizes must agree: take the max over ranks */
    uint64_t bwords = bwords_fixed ? bwords_fixed : L.bwords;
    st = comm_max_u64(ctx, s, bwords);
    if (st != GX_OK) return st;
    HIP_CHK(ctx, ds.bloom.alloc(bwords * 8));
    ds.bwmask = bwords - 1;
    ds.bits.reset();
    if (L.bitmap)
        HIP_CHK(ctx, ds.bits.alloc((L.range + 63) / 64 * 8));
    return dim_launch_build(ctx, s, scan, ds, L.bitmap != 0);
}

/* Slot map of a join/agg table of `slots` slots over qual keys in
 * [kmin,kmax]: order-preserving interpolation when their density over the
 * range is high enough that runs stay short (at least one key per 64,
 * relaxed by nsegs on the Motion path since each rank holds ~1/nsegs of a
 * globally dense key range), otherwise multiplicative hashing (scale < 0). */
static gx_slotmap q3_slotmap(int64_t qual, unsigned long long kmin,
                             unsigned long long kmax, int nsegs, uint64_t slots)
{
    gx_slotmap sm;
    sm.mask = slots - 1;
    sm.kmin = (int64_t) kmin;
    sm.scale = -1.0;
    if (qual > 0 && kmax >= kmin)
    {
        double range = (double) (kmax - kmin) + 1.0;
        if ((double) qual >= range / ((double) nsegs * 64.0))
            sm.scale = (double) slots / range;
    }
    return sm;
}

/* Hash-form table layout for qual keys in [kmin,kmax] (pure host), the one
 * rule of the local path (nsegs 1) and the Motion path: 4-byte keys when
 * every key fits, slots = qual * tf_pct/100 pow2-rounded and always > qual
 * (an open-addressing table with no free slot would never terminate an
 * insert), slot map for exactly that many slots.  Whether a larger cached
 * table is reused instead is the caller's decision; it then re-derives the
 * slot map with q3_slotmap for the slots it really has.
 * Fill factor: the r2 sweep (profiles/rocprof_r2_kernels.txt) took the probe
 * 4.86 -> 4.43 ms and the whole step 8.21 -> 8.07 ms at tf=300 (2^26 slots
 * at SF100, load factor 0.19).  Re-swept with the single-read extract
 * (profiles/aggslot_kernels.txt): tf>=600 still gains 0.38 ms of probe and
 * the extract gives 0.38-0.45 ms of it back (twice the key array to
 * stream), stage sum 7.66-7.70 against 7.59-7.60 at tf=300 — 300 stays. */
struct gx_tbl_layout {
    int key_width;
    uint64_t slots;
    gx_slotmap smap;
};

static gx_tbl_layout q3_table_layout(int64_t qual, unsigned long long kmin,
                                     unsigned long long kmax, int nsegs,
                                     int tf_pct)
{
    gx_tbl_layout L;
    L.key_width = (kmax < (1ULL << 32)) ? 4 : 8;
    L.slots = (uint64_t) pow2_at_least(
        std::max<int64_t>(qual * tf_pct / 100, qual) + 1);
    L.smap = q3_slotmap(qual, kmin, kmax, nsegs, L.slots);
    return L;
}

static inline int q3_table_factor() { return env_int("GX_TABLE_FACTOR_PCT", 300); }

/* first run only: size the dimension membership structures and join/agg
 * table from counting passes; allocate the dimension structures and the
 * result arrays (reused across bench steps).  The join/agg table has two
 * forms, hash and rank (gx_rankview); sizing decides whether the rank form
 * is allowed and records both forms' dimensions, and the first run that
 * uses a form allocates its storage. */
static gx_status q3_size_and_alloc(gx_q3 *q)
{
    gx_ctx *ctx = q->ctx;
    hipStream_t s = ctx->stream;
    const gx_q3_desc &D = q->desc;
    const gx_col &oc = q3_col(q, q->ord, D.mid_fk_col),
                 &od = q3_col(q, q->ord, D.mid_filter.col);
    /* effective visibility = extra-qual mask (already OR-combined with the
     * table visimap at prepare) or the bare visimap */
    const uint8_t *ovm = q->qvm_mid.p ? q->qvm_mid.as<uint8_t>() : q->ord->dvmap;

    HIP_CHK(ctx, q->sc.ensure());
    /* GX_DIM_BITMAP=0 forces the hash form (A/B in one binary).  The orders
     * count below reads the bitmap when there is one. */
    int dim_state = 0;
    {
        gx_status st = q3_dim_size_build(
            ctx, s, q->sc, q3_dim_scan(q),
            D.dim_join == 2 && q3_col(q, q->cust, D.dim_key_col).has_null,
            env_int("GX_DIM_BITMAP", 1) != 0, 0, q->dim, &dim_state);
        if (st != GX_OK) return st;
    }
    if (dim_state == 1)
    {
        /* NOT IN with a NULL key on the inner side anywhere: the whole
         * join yields nothing (nodeHashjoin.c:442 hs_hashkeys_null) */
        q->empty = 1;
        gx_status st = q3_alloc_results(q, 0);
        if (st != GX_OK) return st;
        q->sized = true;
        return GX_OK;
    }

    if (D.fact_join == 1)
    {
        /* LEFT OUTER: bound the unmatched table by the fact key stats
         * (q3_unmatched_bound; NULL-decoded zeros only widen the span,
         * which stays a valid bound).  Sized here for
         * BOTH the local and Motion paths — the unmatched side is always
         * this rank's local fact shard. */
        const gx_col &lkc = q3_col(q, q->li, D.fact_key_col);
        q3_keystats ls;
        gx_status st = q3_read_keystats(
            ctx, s, q->sc, ls, [&](auto *, auto *kmax, auto *kmin) {
                hipLaunchKernelGGL(k_col_minmax, dim3(GRID), dim3(TPB), 0, s,
                                   lkc.dstream, lkc.m, kmax, kmin);
            });
        if (st != GX_OK) return st;
        uint64_t bound = q3_unmatched_bound(q->li->nrows, ls.kmin, ls.kmax);
        uint64_t uslots = (uint64_t) pow2_at_least((int64_t) bound * 2);
        st = hbm_budget_check(
            ctx, uslots * 24 + (bound + 1) * 33, "left-outer unmatched table");
        if (st != GX_OK) return st;
        HIP_CHK(ctx, q->un.key.alloc(uslots * 8));
        HIP_CHK(ctx, q->un.rev.alloc(uslots * 8));
        HIP_CHK(ctx, q->un.cnt.alloc(uslots * 8));
        q->un.mask = uslots - 1;
        q->un.cap = (int64_t) bound;
    }

    /* local qualifying-order count bounds the table for BOTH paths: at
     * nsegs>1 the table holds rows received for THIS segment; the global
     * qualifying count is conserved by the Motions, and each rank's received
     * share ~ 1/nsegs of it.  To stay safe under skew we still size from
     * the exchanged counts in the motion path (re-alloc if bigger). */
    if (ctx->nsegs == 1)
    {
        const q3_dimset &ds = q->dim;
        auto launch_ocount = [&](auto *cs, auto bmode, auto *count, auto *kmax,
                                 auto *kmin) {
            by_flag(D.dim_join != 0, [&](auto anti) {
                hipLaunchKernelGGL((k_orders_count<std::decay_t<decltype(*cs)>,
                                                   decltype(anti)::value,
                                                   decltype(bmode)::value>),
                                   dim3(GRID), dim3(TPB), 0, s,
                                   q3_col(q, q->ord, D.mid_key_col).dstream,
                                   q3_col(q, q->ord, D.mid_key_col).m,
                                   od.dstream, od.m, oc.dstream, oc.m,
                                   ovm,
                                   D.mid_filter.op, (int32_t) D.mid_filter.literal,
                                   cs, ds.cmask,
                                   ds.bloom.as<unsigned long long>(), ds.bwmask,
                                   ds.dimbits(), count, kmax, kmin);
            });
        };
        q3_keystats ks;
        gx_status st = q3_read_keystats(
            ctx, s, q->sc, ks, [&](auto *count, auto *kmax, auto *kmin) {
                if (ds.bitmap)  /* no key set: one set-width instantiation */
                    launch_ocount((const unsigned int *) nullptr,
                                  std::true_type{}, count, kmax, kmin);
                else
                    by_width(ds.width, (const void *) ds.set.p, [&](auto *cs) {
                        launch_ocount(cs, std::false_type{}, count, kmax, kmin);
                    });
            });
        if (st != GX_OK) return st;
        const int64_t qual = (int64_t) ks.count;
        if (qual > 0 && ks.kmin == 0)
        {
            set_err(ctx, "mid join key 0 found among qualifying rows: 0 is "
                         "the empty-slot sentinel (gpuexec.h "
                         "gx_q3_prepare_desc)%s", "");
            return GX_ERR_INVALID;
        }
        const gx_tbl_layout TL = q3_table_layout(qual, ks.kmin, ks.kmax, 1,
                                                 q3_table_factor());
        /* Dense keys also get the rank form (gx_rankview): a run on the
         * local f64 path over a plain fact key then resolves a key with one
         * load instead of the open-addressing walk, into qual dense slots
         * instead of tslots hashed ones.  The verdict and (kmin, range, qual)
         * hold for the life of the q, as the dim bitmap's do; every rank
         * write is guarded by d < range and idx < qual.  GX_RANK_TABLE=0
         * forces the hash form (A/B in one binary).  Only the result arrays
         * are allocated here: each form's table is allocated, and
         * budget-checked, by the first run that uses it (q3_orders_local,
         * q3_orders_rank, q3_orders_motion), so a rank-form q never holds
         * the hash table. */
        q->rank.ok = q3_rank_eligible(qual, ks.kmin, ks.kmax,
                                      env_int("GX_RANK_TABLE", 1) != 0);
        q->rank.kmin = q->rank.ok ? ks.kmin : 0;
        q->rank.range = q->rank.ok ? ks.kmax - ks.kmin + 1 : 0;
        q->rank.kw = q->tbl.width = TL.key_width;
        q->tbl.smap = TL.smap;
        q->local_qual = qual;
        q->hash_tslots = TL.slots;
        /* Admission stays what it was: the q is refused here unless the
         * hash form (the larger one) and the result arrays fit the budget,
         * even when its first run will take the rank form — set_numeric or
         * a forced Motion may move a later run of the same q to the hash
         * form, and a q that ran must not start failing for memory.  The
         * allocations themselves are checked again where they happen. */
        st = hbm_budget_check(
            ctx,
            TL.slots * (TL.key_width + 4 + 4 + 8 + 8) +
                (uint64_t) std::max<int64_t>(qual, 1) * (8 + 4 + 4 + 8 + 8),
            "join/agg table");
        if (st != GX_OK) return st;
        st = q3_alloc_results(q, qual);
        if (st != GX_OK) return st;
    }
    HIP_CHK(ctx, hipStreamSynchronize(s));
    q->sized = true;
    return GX_OK;
}

/* ================= Motion stage seams =================
 * Everything of the nsegs>1 branch of gx_q3_run that is not an RCCL call
 * lives in the helpers below and in the sizing functions above
 * (q3_dim_size_build, q3_table_layout).  They take the run-state structs
 * (q3_dimset, q3_hashtbl, q3_unmatched, q3_results, q3_scratch) as arguments
 * and never reach into gx_q3, so the test-only entry points at the end of
 * this file hold the same structs and drive the very same launches,
 * dispatch, sizing and layout rules with any nsegs on one GPU (DESIGN.md,
 * "Test seams of the Motion path"). */

/* the destination-bloom prefilter of Motion 1 applies to the semi join only:
 * for the anti joins non-membership is the keep condition */
static inline bool m1_prefilter_on(int dim_join) { return dim_join == 0; }

/* Motion 1, pass 1: per-destination histogram of the filtered mid rows.
 * bloom_all (nsegs * (bwmask + 1) words, rank-major) is ignored unless the
 * prefilter applies to dim_join. */
static void m1_launch_hist(hipStream_t s, const gx_col &od, const gx_col &oc,
                           const uint8_t *vmap, int32_t fop, int32_t flit,
                           int nsegs, int dim_join,
                           const unsigned long long *bloom_all, uint64_t bwmask,
                           unsigned long long *dhist)
{
    if (!m1_prefilter_on(dim_join)) bloom_all = nullptr;
    hipLaunchKernelGGL(k_ord_m1_hist, dim3(GRID), dim3(TPB), 0, s,
                       od.dstream, od.m, oc.dstream, oc.m, vmap,
                       fop, flit, nsegs, bloom_all, bwmask, dhist);
}

/* Motion 1, pass 2: emit the packed rows; dcur holds the region starts */
static void m1_launch_emit(hipStream_t s, const gx_col &ok, const gx_col &oc,
                           const gx_col &od, const gx_col &op,
                           const uint8_t *vmap, int32_t fop, int32_t flit,
                           int nsegs, int dim_join,
                           const unsigned long long *bloom_all, uint64_t bwmask,
                           unsigned long long *dcur, gx_ord_row *send)
{
    if (!m1_prefilter_on(dim_join)) bloom_all = nullptr;
    hipLaunchKernelGGL(k_ord_m1_emit, dim3(GRID), dim3(TPB), 0, s,
                       ok.dstream, ok.m, oc.dstream, oc.m, od.dstream, od.m,
                       op.dstream, op.m, vmap, fop, flit, nsegs,
                       bloom_all, bwmask, dcur, send);
}

/* Motion 2: probe the local dim set with the received rows, histogram /
 * emit by route(mid key).  Dispatch on the dim-set width (4 or 8 bytes) and
 * on semi (dim_join == 0) against anti. */
static void m2_launch_hist(hipStream_t s, const gx_ord_row *recv, int64_t n,
                           const q3_dimset &ds, int dim_join, int nsegs,
                           unsigned long long *dhist)
{
    by_width(ds.width, (const void *) ds.set.p, [&](auto *cs) {
        by_flag(dim_join != 0, [&](auto anti) {
            hipLaunchKernelGGL((k_qual_hist<std::decay_t<decltype(*cs)>,
                                            decltype(anti)::value>),
                               dim3(GRID), dim3(TPB), 0, s,
                               recv, n, cs, ds.cmask,
                               ds.bloom.as<const unsigned long long>(),
                               ds.bwmask, nsegs, dhist);
        });
    });
}

static void m2_launch_emit(hipStream_t s, const gx_ord_row *recv, int64_t n,
                           const q3_dimset &ds, int dim_join, int nsegs,
                           unsigned long long *dcur, gx_qual_row *send)
{
    by_width(ds.width, (const void *) ds.set.p, [&](auto *cs) {
        by_flag(dim_join != 0, [&](auto anti) {
            hipLaunchKernelGGL((k_qual_emit<std::decay_t<decltype(*cs)>,
                                            decltype(anti)::value>),
                               dim3(GRID), dim3(TPB), 0, s,
                               recv, n, cs, ds.cmask,
                               ds.bloom.as<const unsigned long long>(),
                               ds.bwmask, nsegs, dcur, send);
        });
    });
}

/* Key stats of the received qualifying rows, the key-0 check and the table
 * layout they get (nsegs from ctx): the Motion run and its test entry point
 * size the join/agg table from this */
static gx_status m3_recv_layout(gx_ctx *ctx, hipStream_t s, const q3_scratch &sc,
                                const gx_qual_row *rows, int64_t n,
                                q3_keystats &ks, gx_tbl_layout &TL)
{
    gx_status st = q3_read_keystats(
        ctx, s, sc, ks, [&](auto *, auto *kmax, auto *kmin) {
            hipLaunchKernelGGL(k_rows_minmax, dim3(GRID), dim3(TPB), 0, s,
                               rows, n, kmax, kmin);
        });
    if (st != GX_OK) return st;
    if (n > 0 && ks.kmin == 0)
    {
        set_err(ctx, "mid join key 0 received: 0 is the empty-slot "
                     "sentinel (gpuexec.h gx_q3_prepare_desc)%s", "");
        return GX_ERR_INVALID;
    }
    TL = q3_table_layout(n, ks.kmin, ks.kmax, ctx->nsegs, q3_table_factor());
    return GX_OK;
}

/* Build the join/agg table from packed qualifying rows */
static void m3_launch_build(hipStream_t s, const gx_qual_row *rows, int64_t n,
                            const q3_hashtbl &t)
{
    by_width(t.width, t.keys.p, [&](auto *tk) {
        hipLaunchKernelGGL(k_build_from_rows<std::decay_t<decltype(*tk)>>,
                           dim3(GRID), dim3(TPB), 0, s, rows, n,
                           tk, t.attrs.as<gx_attrpair>(),
                           t.aggs.as<gx_aggslot>(), t.smap);
    });
}

/* Stage 3, f64 measures over a plain fact key: probe + aggregate, compiled
 * per key width x visimap x LEFT OUTER */
static void q3_launch_probe(hipStream_t s,
                            const gx_col &lk, const gx_col &lp,
                            const gx_col &ld, const gx_col &ls,
                            const uint8_t *lvm, int32_t fop, int32_t flit,
                            const q3_hashtbl &t, unsigned long long *dhits,
                            bool outer, const q3_unmatched &un)
{
    by_width(t.width, (const void *) t.keys.p, [&](auto *keys) {
        by_flag(lvm != nullptr, [&](auto vm) {
            by_flag(outer, [&](auto ou) {
                hipLaunchKernelGGL((k_li_probe_agg_t<std::decay_t<decltype(*keys)>,
                                                     decltype(vm)::value,
                                                     decltype(ou)::value>),
                                   dim3(GRID), dim3(TPB), 0, s,
                                   lk.dstream, lk.m, lp.dstream, lp.m,
                                   ld.dstream, ld.m, ls.dstream, ls.m, lvm,
                                   fop, flit, keys, t.aggs.as<gx_aggslot>(),
                                   t.smap, dhits,
                                   un.key.as<unsigned long long>(),
                                   un.rev.as<double>(),
                                   un.cnt.as<unsigned long long>(), un.mask);
            });
        });
    });
}

/* The same stage over the rank form: the key's rank in rv indexes the dense
 * agg array; compiled per visimap x LEFT OUTER */
static void q3_launch_probe_rank(hipStream_t s,
                                 const gx_col &lk, const gx_col &lp,
                                 const gx_col &ld, const gx_col &ls,
                                 const uint8_t *lvm, int32_t fop, int32_t flit,
                                 gx_rankview rv, gx_aggslot *dagg,
                                 unsigned long long *dhits, bool outer,
                                 const q3_unmatched &un)
{
    by_flag(lvm != nullptr, [&](auto vm) {
        by_flag(outer, [&](auto ou) {
            hipLaunchKernelGGL((k_li_probe_agg_t<uint32_t, decltype(vm)::value,
                                                 decltype(ou)::value, true>),
                               dim3(GRID), dim3(TPB), 0, s,
                               lk.dstream, lk.m, lp.dstream, lp.m,
                               ld.dstream, ld.m, ls.dstream, ls.m, lvm,
                               fop, flit, (const uint32_t *) nullptr, dagg,
                               gx_slotmap{}, dhits,
                               un.key.as<unsigned long long>(),
                               un.rev.as<double>(),
                               un.cnt.as<unsigned long long>(), un.mask, rv);
        });
    });
}

/* Stage 4: one block per fixed tile of the table, block-ordered extract */
static gx_status q3_launch_extract(gx_ctx *ctx, hipStream_t s, int key_width,
                                   const void *tkey, const gx_attrpair *tattr,
                                   const gx_aggslot *tagg, uint64_t tslots,
                                   int numeric, const q3_results &r,
                                   unsigned long long *dcount)
{
    uint64_t etiles = (tslots + GX_EXTRACT_TILE - 1) / GX_EXTRACT_TILE;
    if (etiles > 0x7FFFFFFFULL)
    {
        set_err(ctx, "join/agg table too large for the extract grid%s", "");
        return GX_ERR_INVALID;
    }
    by_width(key_width, tkey, [&](auto *keys) {
        hipLaunchKernelGGL(k_extract<std::decay_t<decltype(*keys)>>,
                           dim3((unsigned) etiles), dim3(TPB), 0, s,
                           keys, tattr, tagg, tslots, numeric,
                           r.okey.as<int64_t>(), r.odate.as<int32_t>(),
                           r.oprio.as<int32_t>(), r.rev.as<double>(),
                           r.cnt.as<int64_t>(), dcount);
    });
    return GX_OK;
}

extern "C" gx_status gx_q3_set_numeric(gx_q3 *q, int on)
{
    if (!q) return GX_ERR_INVALID;
    /* the fused RLE probe has no integer-aggregation form: say so here, the
     * earliest point the mode is known, not at the first run.  A format-1
     * fact key that prepare materialized is a flat column and is fine. */
    if (on && q3_col(q, q->li, q->desc.fact_key_col).format == 1)
    {
        set_err(q->ctx, "numeric mode is not supported with a fused RLE fact "
                        "key (numeric+RLE); bind the key plain%s", "");
        return GX_ERR_INVALID;
    }
    q->numeric = on ? 1 : 0;
    return GX_OK;
}

extern "C" gx_status gx_q3_dim_mode(gx_q3 *q, int *mode)
{
    if (!q || !mode) return GX_ERR_INVALID;
    if (!q->ran) return GX_ERR_STATE;
    *mode = q->dim_mode;
    return GX_OK;
}

extern "C" gx_status gx_q3_table_mode(gx_q3 *q, int *mode)
{
    if (!q || !mode) return GX_ERR_INVALID;
    if (!q->ran) return GX_ERR_STATE;
    *mode = q->table_mode;
    return GX_OK;
}

extern "C" gx_status gx_q3_orders_mode(gx_q3 *q, int *mode)
{
    if (!q || !mode) return GX_ERR_INVALID;
    if (!q->ran) return GX_ERR_STATE;
    *mode = q->table_mode == 1 ? q->orders_mode : 0;
    return GX_OK;
}

extern "C" gx_status gx_q3_orders_stage_claims(gx_q3 *q, int64_t *blocks,
                                               int64_t *flushes, int64_t *records)
{
    if (!q || !blocks || !flushes || !records) return GX_ERR_INVALID;
    if (!q->ran || q->table_mode != 1 || q->orders_mode != 1 ||
        !q->rank.stage_cur.p)
        return GX_ERR_STATE;
    unsigned long long cur[2] = {0, 0};
    HIP_CHK(q->ctx, hipMemcpy(cur, q->rank.stage_cur.p, sizeof cur, hipMemcpyDeviceToHost));
    *blocks = q->stage_blocks;
    *flushes = (int64_t) cur[1];
    *records = (int64_t) cur[0];
    return GX_OK;
}

extern "C" gx_status gx_q3_test_set_orders_grid(gx_q3 *q, int64_t blocks)
{
    if (!q || blocks < 0 || blocks > (1 << 20)) return GX_ERR_INVALID;
    q->test_orders_grid = blocks;
    return GX_OK;
}

/* the columns and effective visibility masks one Q3 run reads (extra-qual
 * masks fold the visimap in) */
struct q3_runcols {
    const gx_col &ok, &oc, &od, &op;     /* mid: key, fk, filter, attr2 */
    const gx_col &lk, &lp, &ld, &ls;     /* fact: key, a, b, filter */
    const uint8_t *ovm, *lvm;
};

/* Stage 2, single segment: build the join/agg table straight from the mid
 * table's columns (date filter + dim semi/anti join + insert in one pass) */
static gx_status q3_orders_local(gx_q3 *q, const q3_runcols &C, bool use_bitmap)
{
    gx_ctx *ctx = q->ctx;
    hipStream_t s = ctx->stream;
    const gx_q3_desc &D = q->desc;
    const gx_col &ok = C.ok, &oc = C.oc, &od = C.od, &op = C.op;
    const q3_dimset &ds = q->dim;
    q3_hashtbl &t = q->tbl;
    if (!t.keys.p)              /* first hash-form run of this q */
    {
        gx_status st = q3_alloc_hash(ctx, t, q->hash_tslots);
        if (st != GX_OK) return st;
    }
    /* keys only: agg/attr slots are initialised at claim (gx_aggslot) */
    HIP_CHK(ctx, hipMemsetAsync(t.keys.p, 0, t.slots() * t.width, s));
    if (D.fact_join == 1)
        HIP_CHK(ctx, q->un.clear(s));
    auto launch_build = [&](auto *tk, auto *cs, auto bmode) {
        by_flag(C.ovm != nullptr, [&](auto vm) {
            by_flag(D.dim_join != 0, [&](auto anti) {
                hipLaunchKernelGGL((k_orders_build<std::decay_t<decltype(*tk)>,
                                                   std::decay_t<decltype(*cs)>,
                                                   decltype(vm)::value,
                                                   decltype(anti)::value,
                                                   decltype(bmode)::value>),
                                   dim3(ORDERS_GRID), dim3(TPB), 0, s,
                                   ok.dstream, ok.m, oc.dstream, oc.m, od.dstream, od.m,
                                   op.dstream, op.m, C.ovm, D.mid_filter.op,
                                   (int32_t) D.mid_filter.literal, cs, ds.cmask,
                                   ds.bloom.as<unsigned long long>(), ds.bwmask,
                                   ds.dimbits(), tk, t.attrs.as<gx_attrpair>(),
                                   t.aggs.as<gx_aggslot>(), t.smap);
            });
        });
    };
    by_width(t.width, t.keys.p, [&](auto *tk) {
        if (use_bitmap)     /* no key set: one set-width instantiation */
            launch_build(tk, (const unsigned int *) nullptr, std::true_type{});
        else
            by_width(ds.width, (const void *) ds.set.p, [&](auto *cs) {
                launch_build(tk, cs, std::false_type{});
            });
    });
    return GX_OK;
}

/* Stage 2, single segment, rank form: mark the qualifying keys' bits and the
 * qualifying rows, turn the bit words into ranks (prefix popcounts), then
 * store each qualifying row's key and attrs at its key's rank.  The rows
 * reach the fill kernel as a per-row mask (two-pass) or as compacted records
 * (staged): q3_orders_staged picks per run. */
static gx_status q3_orders_rank(gx_q3 *q, const q3_runcols &C, bool use_bitmap)
{
    gx_ctx *ctx = q->ctx;
    hipStream_t s = ctx->stream;
    const gx_q3_desc &D = q->desc;
    const gx_col &ok = C.ok, &oc = C.oc, &od = C.od, &op = C.op;
    const q3_dimset &ds = q->dim;
    q3_ranktbl &r = q->rank;
    if (!r.dagg.p)              /* first rank-form run of this q */
    {
        gx_status st = q3_alloc_rank(ctx, r, (uint64_t) q->local_qual);
        if (st != GX_OK) return st;
    }
    const bool staged = q3_orders_staged(q->local_qual, ok.m.nrows,
                                         env_int("GX_ORDERS_STAGED", -1));
    q->orders_mode = staged ? 1 : 0;
    if (staged && !r.stage_cur.p)               /* first staged run */
    {
        gx_status st = q3_alloc_stage(q);
        if (st != GX_OK) return st;
    }
    if (!staged && !r.rowmask.p)                /* first two-pass run */
    {
        gx_status st = q3_alloc_rowmask(q);
        if (st != GX_OK) return st;
    }
    uint64_t nwords = r.nwords();
    uint64_t nblk = (nwords + GX_RANK_SCAN_WORDS - 1) / GX_RANK_SCAN_WORDS;
    if (nblk > 0x7FFFFFFFULL)
    {
        set_err(ctx, "rank table too large for the scan grid%s", "");
        return GX_ERR_INVALID;
    }
    /* the entries (their bit words), and the dense keys so that extract emits no slot past
     * this run's distinct qualifying keys; dattr/dagg are initialised by the
     * fill kernel where a key lands (gx_aggslot) */
    HIP_CHK(ctx, hipMemsetAsync(r.ent.p, 0, nwords * sizeof(ulonglong2), s));
    HIP_CHK(ctx, hipMemsetAsync(r.dkey.p, 0,
                                (uint64_t) q->local_qual * r.kw, s));
    if (staged)
        HIP_CHK(ctx, hipMemsetAsync(r.stage_cur.p, 0, 16, s));
    if (D.fact_join == 1)
        HIP_CHK(ctx, q->un.clear(s));
    const gx_rankview rv = r.view(q->local_qual);
    const uint64_t cap = (uint64_t) q->local_qual;
    /* two-pass: the grid k_orders_build measured best.  staged: sized from
     * the selectivity (q3_stage_grid), or the caller's in tests. */
    int64_t mark_grid = ORDERS_GRID;
    if (staged)
    {
        mark_grid = q->test_orders_grid > 0
            ? q->test_orders_grid
            : q3_stage_grid(q->local_qual, ok.m.nrows);
        q->stage_blocks = mark_grid;
    }
    auto launch_mark = [&](auto *cs, auto bmode) {
        by_flag(C.ovm != nullptr, [&](auto vm) {
            by_flag(D.dim_join != 0, [&](auto anti) {
                by_flag(staged, [&](auto stg) {
                    hipLaunchKernelGGL((k_orders_mark<std::decay_t<decltype(*cs)>,
                                                      decltype(vm)::value,
                                                      decltype(anti)::value,
                                                      decltype(bmode)::value,
                                                      decltype(stg)::value>),
                                       dim3((unsigned) mark_grid), dim3(TPB), 0, s,
                                       ok.dstream, ok.m, oc.dstream, oc.m,
                                       od.dstream, od.m, C.ovm, D.mid_filter.op,
                                       (int32_t) D.mid_filter.literal, cs, ds.cmask,
                                       ds.bloom.as<unsigned long long>(),
                                       ds.bwmask, ds.dimbits(),
                                       r.ent.as<ulonglong2>(), r.kmin, r.range,
                                       r.rowmask.as<unsigned long long>(),
                                       op.dstream, op.m,
                                       r.stage.as<ulonglong2>(),
                                       r.stage_cur.as<unsigned long long>(), cap);
                });
            });
        });
    };
    if (use_bitmap)     /* no key set: one set-width instantiation */
        launch_mark((const unsigned int *) nullptr, std::true_type{});
    else
        by_width(ds.width, (const void *) ds.set.p, [&](auto *cs) {
            launch_mark(cs, std::false_type{});
        });
    hipLaunchKernelGGL(k_rank_blocksum, dim3((unsigned) nblk), dim3(TPB), 0, s,
                       r.ent.as<ulonglong2>(), nwords, r.blk.as<uint32_t>());
    hipLaunchKernelGGL(k_rank_topscan, dim3(1), dim3(TPB), 0, s,
                       r.blk.as<uint32_t>(), (int) nblk);
    hipLaunchKernelGGL(k_rank_localscan, dim3((unsigned) nblk), dim3(TPB), 0, s,
                       r.ent.as<ulonglong2>(), nwords, r.blk.as<uint32_t>());
    by_width(r.kw, r.dkey.p, [&](auto *dk) {
        if (staged)
        {
            /* the record count is on the device: grid from the capacity */
            uint64_t fb = std::min<uint64_t>(
                std::max<uint64_t>((cap + TPB - 1) / TPB, 1), ORDERS_GRID);
            hipLaunchKernelGGL(k_orders_fill_staged<std::decay_t<decltype(*dk)>>,
                               dim3((unsigned) fb), dim3(TPB), 0, s,
                               r.stage.as<ulonglong2>(),
                               r.stage_cur.as<unsigned long long>(), cap, rv, dk,
                               r.dattr.as<gx_attrpair>(), r.dagg.as<gx_aggslot>());
        }
        else
            hipLaunchKernelGGL(k_orders_fill<std::decay_t<decltype(*dk)>>,
                               dim3(ORDERS_GRID), dim3(TPB), 0, s,
                               ok.dstream, ok.m, od.dstream, od.m,
                               op.dstream, op.m,
                               r.rowmask.as<unsigned long long>(), rv, dk,
                               r.dattr.as<gx_attrpair>(), r.dagg.as<gx_aggslot>());
    });
    return GX_OK;
}

/* Stage 2, nsegs > 1 (or GX_FORCE_MOTION): Motion 1 ships the filtered mid
 * rows by route(fk), the local dim set filters them, Motion 2 ships the
 * qualifying ones by route(mid key), and the join/agg table is built from
 * what arrives.  dim_done: the dim build's completion on the primary stream.
 * Ends in a host sync of the Motion stream. */
static gx_status q3_orders_motion(gx_q3 *q, const q3_runcols &C,
                                  hipEvent_t dim_done, int64_t *qual_out,
                                  double *ms_motion)
{
    gx_ctx *ctx = q->ctx;
    const gx_q3_desc &D = q->desc;
    const gx_col &ok = C.ok, &oc = C.oc, &od = C.od, &op = C.op;
    if (!ctx->comm) { set_err(ctx, "nsegs>1 but gx_comm_init not called%s", ""); return GX_ERR_STATE; }
    int n = ctx->nsegs;
    /* the exchange runs on stream2, concurrent with the dim-set build
     * still in flight on the primary stream (they only meet at the
     * local semijoin below, via a cross-stream event wait); the branch
     * ends in a host sync, so stage 3 on the primary stream is ordered */
    hipStream_t ms = ctx->stream2;
    evholder mev0, mev1;
    HIP_CHK(ctx, mev0.create()); HIP_CHK(ctx, mev1.create());
    HIP_CHK(ctx, hipEventRecord(mev0, ms));

    /* Motion 1: filtered orders by route(o_custkey).  Exchange buffers
     * are cached in gx_q3 (grow-only) — per-step allocation would
     * dominate at high rank counts. */
    const q3_dimset &ds = q->dim;
    HIP_CHK(ctx, q->m_hist.reserve(n * 8));
    HIP_CHK(ctx, q->m_cur.reserve(n * 8));
    HIP_CHK(ctx, q->m_cnts_all.reserve((int64_t) n * n * 8));
    /* Motion-1 count exchange: the per-dest histogram goes straight
     * into the all-gather, so ONE host sync yields both this rank's
     * send layout (its own row) and every peer's counts (r2: the two
     * separate count syncs were ~half the fixed motion latency) */
    unsigned long long *dhist = q->m_hist.as<unsigned long long>();
    /* destination-aware bloom prefilter (semi join only): all-gather
     * every rank's dim bloom, then only ship orders whose fk passes
     * the DESTINATION's bloom — the runtime filter pushed across the
     * interconnect.  Requires the local dim build (primary stream). */
    const unsigned long long *bloom_all = nullptr;
    if (m1_prefilter_on(D.dim_join))
    {
        uint64_t bwords = ds.bwmask + 1;
        HIP_CHK(ctx, q->m_bloom_all.reserve((uint64_t) n * bwords * 8));
        HIP_CHK(ctx, hipStreamWaitEvent(ms, dim_done, 0));
        RCCL_CHK(ctx, ncclAllGather(ds.bloom.p, q->m_bloom_all.p, bwords,
                                    ncclUint64, ctx->comm, ms));
        bloom_all = q->m_bloom_all.as<unsigned long long>();
    }
    HIP_CHK(ctx, hipMemsetAsync(dhist, 0, n * 8, ms));
    m1_launch_hist(ms, od, oc, C.ovm, D.mid_filter.op,
                   (int32_t) D.mid_filter.literal, n, D.dim_join,
                   bloom_all, ds.bwmask, dhist);
    unsigned long long *dcnts_all = q->m_cnts_all.as<unsigned long long>();
    double t_counts = 0;
    auto now_ms = []() {
        return (double) std::chrono::duration_cast<std::chrono::nanoseconds>(
                   std::chrono::steady_clock::now().time_since_epoch())
                   .count() / 1e6;
    };
    double tc0 = now_ms();
    RCCL_CHK(ctx, ncclAllGather(dhist, dcnts_all, n, ncclUint64, ctx->comm, ms));
    std::vector<unsigned long long> cnts_all(n * n);
    HIP_CHK(ctx, hipMemcpyAsync(cnts_all.data(), dcnts_all, (int64_t) n * n * 8,
                                hipMemcpyDeviceToHost, ms));
    HIP_CHK(ctx, hipStreamSynchronize(ms));
    t_counts += now_ms() - tc0;
    const gx_mlayout L1 = m_exchange_layout(cnts_all.data(), n, ctx->seg);
    if (q->m_send1.reserve(L1.send_n * sizeof(gx_ord_row)) != hipSuccess)
        return GX_ERR_OOM;
    gx_ord_row *send1 = q->m_send1.as<gx_ord_row>();
    unsigned long long *dcur = q->m_cur.as<unsigned long long>();
    HIP_CHK(ctx, hipMemcpyAsync(dcur, L1.soff.data(), n * 8, hipMemcpyHostToDevice, ms));
    m1_launch_emit(ms, ok, oc, od, op, C.ovm, D.mid_filter.op,
                   (int32_t) D.mid_filter.literal, n, D.dim_join,
                   bloom_all, ds.bwmask, dcur, send1);
    unsigned long long recv1_n = L1.recv_n;
    if (q->m_recv1.reserve(recv1_n * sizeof(gx_ord_row)) != hipSuccess)
        return GX_ERR_OOM;
    gx_ord_row *recv1 = q->m_recv1.as<gx_ord_row>();
    evholder pev0, pev1, pev2, pev3;
    HIP_CHK(ctx, pev0.create()); HIP_CHK(ctx, pev1.create());
    HIP_CHK(ctx, pev2.create()); HIP_CHK(ctx, pev3.create());
    HIP_CHK(ctx, hipEventRecord(pev0, ms));
    {
        gx_status xst = m_exchange_payload(ctx, ms, send1, recv1, L1,
                                           sizeof(gx_ord_row));
        if (xst != GX_OK) return xst;
    }
    HIP_CHK(ctx, hipEventRecord(pev1, ms));

    /* Motion 2: probe local customer set, route qualifying by o_orderkey
     * — first wait (on-stream) for the dim-set build on the primary
     * stream to finish */
    HIP_CHK(ctx, hipStreamWaitEvent(ms, dim_done, 0));
    HIP_CHK(ctx, hipMemsetAsync(dhist, 0, n * 8, ms));
    m2_launch_hist(ms, recv1, (int64_t) recv1_n, ds, D.dim_join, n, dhist);
    /* Motion-2 count exchange: same single-sync shape */
    tc0 = now_ms();
    RCCL_CHK(ctx, ncclAllGather(dhist, dcnts_all, n, ncclUint64, ctx->comm, ms));
    HIP_CHK(ctx, hipMemcpyAsync(cnts_all.data(), dcnts_all, (int64_t) n * n * 8,
                                hipMemcpyDeviceToHost, ms));
    HIP_CHK(ctx, hipStreamSynchronize(ms));
    t_counts += now_ms() - tc0;
    const gx_mlayout L2 = m_exchange_layout(cnts_all.data(), n, ctx->seg);
    if (q->m_send2.reserve(L2.send_n * sizeof(gx_qual_row)) != hipSuccess)
        return GX_ERR_OOM;
    gx_qual_row *send2 = q->m_send2.as<gx_qual_row>();
    HIP_CHK(ctx, hipMemcpyAsync(dcur, L2.soff.data(), n * 8, hipMemcpyHostToDevice, ms));
    m2_launch_emit(ms, recv1, (int64_t) recv1_n, ds, D.dim_join, n, dcur, send2);
    unsigned long long recv2_n = L2.recv_n;
    if (q->m_recv2.reserve(recv2_n * sizeof(gx_qual_row)) != hipSuccess)
        return GX_ERR_OOM;
    gx_qual_row *recv2 = q->m_recv2.as<gx_qual_row>();
    HIP_CHK(ctx, hipEventRecord(pev2, ms));
    {
        gx_status xst = m_exchange_payload(ctx, ms, send2, recv2, L2,
                                           sizeof(gx_qual_row));
        if (xst != GX_OK) return xst;
    }
    HIP_CHK(ctx, hipEventRecord(pev3, ms));

    int64_t qual = (int64_t) recv2_n;
    /* key stats over the received rows — the motion path then gets the
     * same u32/interpolation table layout as the local path */
    q3_keystats ks;
    gx_tbl_layout TL;
    {
        gx_status lst = m3_recv_layout(ctx, ms, q->sc, recv2, qual, ks, TL);
        if (lst != GX_OK) return lst;
    }
    q3_hashtbl &t = q->tbl;
    /* motion path sizes from the exchanged counts each run; qual can
     * grow within the same pow2 table size, so the result capacity is
     * checked too */
    if (!t.keys.p || TL.slots > t.slots() || TL.key_width != t.width ||
        qual + q->un.cap > q->res.cap)
    {
        t.width = TL.key_width;
        gx_status ast = q3_alloc_table(q, TL.slots, qual);
        if (ast != GX_OK) return ast;
    }
    /* keys only: agg/attr slots are initialised at claim (gx_aggslot) */
    HIP_CHK(ctx, hipMemsetAsync(t.keys.p, 0, t.slots() * t.width, ms));
    if (D.fact_join == 1)
        HIP_CHK(ctx, q->un.clear(ms));
    /* a reused cached table may be larger than this run's layout */
    t.smap = (t.slots() == TL.slots)
                 ? TL.smap
                 : q3_slotmap(qual, ks.kmin, ks.kmax, ctx->nsegs, t.slots());
    m3_launch_build(ms, recv2, qual, t);
    HIP_CHK(ctx, hipEventRecord(mev1, ms));
    HIP_CHK(ctx, hipStreamSynchronize(ms));
    float mms = 0, p01 = 0, p23 = 0;
    (void) hipEventElapsedTime(&mms, mev0, mev1);
    (void) hipEventElapsedTime(&p01, pev0, pev1);
    (void) hipEventElapsedTime(&p23, pev2, pev3);
    *ms_motion = mms;
    q->stats.ms_motion_counts = t_counts;
    q->stats.ms_motion_payload = (double) p01 + (double) p23;
    *qual_out = qual;
    return GX_OK;
}

/* Stage 3: lineitem scan+probe+agg (dominant kernel), in the form the fact
 * key's format and the aggregation mode select: fused RLE, numeric, f64 */
static gx_status q3_probe_agg(gx_q3 *q, const q3_runcols &C)
{
    gx_ctx *ctx = q->ctx;
    hipStream_t s = ctx->stream;
    const gx_q3_desc &D = q->desc;
    const gx_col &lk = C.lk, &lp = C.lp, &ld = C.ld, &ls = C.ls;
    const q3_hashtbl &t = q->tbl;
    unsigned long long *dhits = q->sc.word(q3_scratch::HITS);
    unsigned long long *derr = q->sc.word(q3_scratch::ERR);
    HIP_CHK(ctx, hipMemsetAsync(dhits, 0, 8, s));
    if (lk.format == 1)
    {
        if (q->numeric) { set_err(ctx, "numeric+RLE combo not supported%s", ""); return GX_ERR_INVALID; }
        HIP_CHK(ctx, hipMemsetAsync(derr, 0, 8, s));
        int64_t nb = lk.nblocks;
        int rgrid = (int) std::min<int64_t>(std::max<int64_t>(nb, 1), 16384);
        by_width(t.width, (const void *) t.keys.p, [&](auto *keys) {
            by_flag(C.lvm != nullptr, [&](auto vm) {
                hipLaunchKernelGGL((k_li_probe_agg_rle<std::decay_t<decltype(*keys)>,
                                                       decltype(vm)::value>),
                                   dim3(rgrid), dim3(TPB), 0, s,
                                   lk.dstream, lk.ddir, nb, lp.dstream, lp.m,
                                   ld.dstream, ld.m, ls.dstream, ls.m, C.lvm,
                                   D.fact_filter.op, (int32_t) D.fact_filter.literal,
                                   keys, t.aggs.as<gx_aggslot>(), t.smap, dhits,
                                   (int *) derr);
            });
        });
        int herr = 0;
        HIP_CHK(ctx, hipMemcpyAsync(&herr, derr, 4, hipMemcpyDeviceToHost, s));
        HIP_CHK(ctx, hipStreamSynchronize(s));
        if (herr) { set_err(ctx, "malformed RLE block in fused scan%s", ""); return GX_ERR_INVALID; }
    }
    else if (q->numeric)
    {
        HIP_CHK(ctx, hipMemsetAsync(derr, 0, 8, s));
        by_width(t.width, (const void *) t.keys.p, [&](auto *keys) {
            by_flag(C.lvm != nullptr, [&](auto vm) {
                by_flag(D.fact_join == 1, [&](auto outer) {
                    hipLaunchKernelGGL((k_li_probe_agg_num<std::decay_t<decltype(*keys)>,
                                                           decltype(vm)::value,
                                                           decltype(outer)::value>),
                                       dim3(GRID), dim3(TPB), 0, s,
                                       lk.dstream, lk.m, lp.dstream, lp.m, ld.dstream, ld.m,
                                       ls.dstream, ls.m, C.lvm, D.fact_filter.op,
                                       (int32_t) D.fact_filter.literal, keys,
                                       t.aggs.as<gx_aggslot_num>(), t.smap,
                                       dhits, (int *) derr,
                                       q->un.key.as<unsigned long long>(),
                                       q->un.rev.as<unsigned long long>(),
                                       q->un.cnt.as<unsigned long long>(),
                                       q->un.mask);
                });
            });
        });
        int herr = 0;
        HIP_CHK(ctx, hipMemcpyAsync(&herr, derr, 4, hipMemcpyDeviceToHost, s));
        HIP_CHK(ctx, hipStreamSynchronize(s));
        if (herr) { set_err(ctx, "numeric overflow in aggregation%s", ""); return GX_ERR_INVALID; }
    }
    else if (q->table_mode == 1)
        q3_launch_probe_rank(
            s, lk, lp, ld, ls, C.lvm, D.fact_filter.op,
            (int32_t) D.fact_filter.literal, q->rank.view(q->local_qual),
            q->rank.dagg.as<gx_aggslot>(), dhits, D.fact_join == 1, q->un);
    else
        q3_launch_probe(
            s, lk, lp, ld, ls, C.lvm, D.fact_filter.op,
            (int32_t) D.fact_filter.literal, t, dhits, D.fact_join == 1, q->un);
    return GX_OK;
}

/* Stage 4: extract the groups (and the LEFT-OUTER unmatched ones) into the
 * result arrays; the group count lands in the GROUPS scratch word */
static gx_status q3_extract(gx_q3 *q)
{
    gx_ctx *ctx = q->ctx;
    hipStream_t s = ctx->stream;
    const q3_results &r = q->res;
    unsigned long long *dcount = q->sc.word(q3_scratch::GROUPS);
    HIP_CHK(ctx, hipMemsetAsync(dcount, 0, 8, s));
    HIP_CHK(ctx, hipMemsetAsync(r.flags.p, 0, r.cap, s));
    /* one block per fixed tile of the table; k_extract_u keeps its own grid */
    const int egrid = 32768;
    {
        /* rank form: the same kernel over the dense arrays, whose slots at
         * or past this run's distinct keys hold key 0 (cleared per run) */
        gx_status est = q->table_mode == 1
            ? q3_launch_extract(ctx, s, q->rank.kw, q->rank.dkey.p,
                                q->rank.dattr.as<gx_attrpair>(),
                                q->rank.dagg.as<gx_aggslot>(),
                                (uint64_t) q->local_qual, q->numeric, r, dcount)
            : q3_launch_extract(ctx, s, q->tbl.width, q->tbl.keys.p,
                                q->tbl.attrs.as<gx_attrpair>(),
                                q->tbl.aggs.as<gx_aggslot>(), q->tbl.slots(),
                                q->numeric, r, dcount);
        if (est != GX_OK) return est;
    }
    if (q->desc.fact_join == 1)
        hipLaunchKernelGGL(k_extract_u, dim3(egrid), dim3(TPB), 0, s,
                           q->un.key.as<unsigned long long>(),
                           q->un.rev.as<double>(),
                           q->un.cnt.as<unsigned long long>(), q->un.mask + 1,
                           r.okey.as<int64_t>(), r.odate.as<int32_t>(),
                           r.oprio.as<int32_t>(), r.rev.as<double>(),
                           r.cnt.as<int64_t>(), r.flags.as<uint8_t>(), dcount,
                           r.cap);
    return GX_OK;
}

extern "C" gx_status gx_q3_run(gx_q3 *q)
{
    if (!q) return GX_ERR_INVALID;
    gx_ctx *ctx = q->ctx;
    hipStream_t s = ctx->stream;
    memset(&q->stats, 0, sizeof q->stats);
    if (!q->sized)
    {
        gx_status st = q3_size_and_alloc(q);
        if (st != GX_OK) return st;
    }
    if (q->empty)
    {
        /* LASJ_NOTIN with a NULL inner key: nothing qualifies */
        q->ngroups = 0;
        q->stats.cust_rows = q->cust->nrows;
        q->stats.ord_rows = q->ord->nrows;
        q->stats.li_rows = q->li->nrows;
        q->ran = true;
        return GX_OK;
    }

    evholder ev[8];
    for (auto &e : ev) HIP_CHK(ctx, e.create());

    const gx_q3_desc &D = q->desc;
    const q3_runcols C = {
        q3_col(q, q->ord, D.mid_key_col), q3_col(q, q->ord, D.mid_fk_col),
        q3_col(q, q->ord, D.mid_filter.col), q3_col(q, q->ord, D.mid_attr2_col),
        q3_col(q, q->li, D.fact_key_col), q3_col(q, q->li, D.fact_a_col),
        q3_col(q, q->li, D.fact_b_col), q3_col(q, q->li, D.fact_filter.col),
        q->qvm_mid.p ? q->qvm_mid.as<uint8_t>() : q->ord->dvmap,
        q->qvm_fact.p ? q->qvm_fact.as<uint8_t>()
                      : (q->li ? q->li->dvmap : nullptr)};

    /* ---- stage 1: customer BUILDING membership (rebuilt every run) ----
     * the local path reads the bitmap when sizing chose one; the Motion path
     * reads set+bloom.  Only that one is cleared and filled. */
    bool local_path = ctx->nsegs == 1 && env_int("GX_FORCE_MOTION", 0) == 0;
    bool use_bitmap = q->dim.bitmap && local_path;
    q->dim_mode = use_bitmap ? 1 : 0;
    HIP_CHK(ctx, hipEventRecord(ev[0], s));
    {
        gx_status st = dim_launch_build(ctx, s, q3_dim_scan(q), q->dim, use_bitmap);
        if (st != GX_OK) return st;
    }
    HIP_CHK(ctx, hipEventRecord(ev[1], s));

    /* ---- stage 2: orders build (local or via Motions) ----
     * GX_FORCE_MOTION=1 routes a single-segment run through the FULL
     * RCCL exchange branch (self send/recv) — the exact code the
     * multi-GPU scale bench executes, testable on one GPU. */
    int64_t qual = 0;
    double ms_motion = 0.0;
    /* table form of this run: rank for dense keys on the local path under
     * the plain f64 probe over a flat fact key; hash for everything else */
    q->table_mode = (q->rank.ok && local_path && !q->numeric &&
                     C.lk.format == 0) ? 1 : 0;
    if (local_path)
    {
        gx_status st = q->table_mode == 1 ? q3_orders_rank(q, C, use_bitmap)
                                          : q3_orders_local(q, C, use_bitmap);
        if (st != GX_OK) return st;
        qual = q->res.cap;
    }
    else
    {
        gx_status st = q3_orders_motion(q, C, ev[1], &qual, &ms_motion);
        if (st != GX_OK) return st;
    }
    q->qual_orders = qual;
    HIP_CHK(ctx, hipEventRecord(ev[2], s));

    /* ---- stage 3: lineitem scan+probe+agg (dominant kernel) ---- */
    {
        gx_status st = q3_probe_agg(q, C);
        if (st != GX_OK) return st;
    }
    HIP_CHK(ctx, hipEventRecord(ev[3], s));

    /* ---- stage 4: extract ---- */
    {
        gx_status st = q3_extract(q);
        if (st != GX_OK) return st;
    }
    HIP_CHK(ctx, hipEventRecord(ev[4], s));

    unsigned long long ngroups = 0, hits = 0;
    HIP_CHK(ctx, hipMemcpyAsync(&ngroups, q->sc.word(q3_scratch::GROUPS), 8,
                                hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipMemcpyAsync(&hits, q->sc.word(q3_scratch::HITS), 8,
                                hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    if (q->desc.fact_join == 1 && (int64_t) ngroups > q->res.cap)
    {
        /* a sizing error must be an error, not a stray write: k_extract_u
         * stopped writing at the result capacity */
        q->ran = false;
        char buf[96];
        snprintf(buf, sizeof buf, "%lld groups, capacity %lld",
                 (long long) ngroups, (long long) q->res.cap);
        set_err(ctx, "q3: extract overflow (%s)", buf);
        return GX_ERR_INVALID;
    }
    q->ngroups = (int64_t) ngroups;

    float t01 = 0, t12 = 0, t23 = 0, t34 = 0, t04 = 0;
    (void) hipEventElapsedTime(&t01, ev[0], ev[1]);
    (void) hipEventElapsedTime(&t12, ev[1], ev[2]);
    (void) hipEventElapsedTime(&t23, ev[2], ev[3]);
    (void) hipEventElapsedTime(&t34, ev[3], ev[4]);
    (void) hipEventElapsedTime(&t04, ev[0], ev[4]);
    q->stats.ms_cust_build = t01;
    q->stats.ms_orders_build = std::max(0.0, (double) t12 - ms_motion);
    q->stats.ms_motion = ms_motion;
    q->stats.ms_probe_agg = t23;
    q->stats.ms_extract = t34;
    q->stats.ms_total = t04;
    q->stats.cust_rows = q->cust->nrows;
    q->stats.ord_rows = q->ord->nrows;
    q->stats.li_rows = q->li->nrows;
    q->stats.probe_hits = (int64_t) hits;
    q->stats.groups = q->ngroups;
    double b = 0, bb = 0;
    gx_table_logical_bytes(q->cust, &b); bb += b;
    gx_table_logical_bytes(q->ord, &b); bb += b;
    gx_table_logical_bytes(q->li, &b); bb += b;
    q->stats.bytes_scanned = bb;

    q->ran = true;
    return GX_OK;
}

extern "C" gx_status gx_q3_stats_get(const gx_q3 *q, gx_q3_stats *out)
{
    if (!q || !q->ran) return GX_ERR_STATE;
    *out = q->stats;
    return GX_OK;
}

extern "C" gx_status gx_q3_result(gx_q3 *q, gx_q3_group **out, int64_t *ngroups)
{
    if (!q || !q->ran) return GX_ERR_STATE;
    gx_ctx *ctx = q->ctx;
    int64_t n = q->ngroups;
    std::vector<int64_t> okey(n), cnt(n);
    std::vector<int32_t> odate(n), oprio(n);
    std::vector<double> rev(n);
    std::vector<uint8_t> flags(n, 0);
    if (n)
    {
        HIP_CHK(ctx, hipMemcpy(okey.data(), q->res.okey.p, n * 8, hipMemcpyDeviceToHost));
        HIP_CHK(ctx, hipMemcpy(odate.data(), q->res.odate.p, n * 4, hipMemcpyDeviceToHost));
        HIP_CHK(ctx, hipMemcpy(oprio.data(), q->res.oprio.p, n * 4, hipMemcpyDeviceToHost));
        HIP_CHK(ctx, hipMemcpy(rev.data(), q->res.rev.p, n * 8, hipMemcpyDeviceToHost));
        HIP_CHK(ctx, hipMemcpy(cnt.data(), q->res.cnt.p, n * 8, hipMemcpyDeviceToHost));
        HIP_CHK(ctx, hipMemcpy(flags.data(), q->res.flags.p, n, hipMemcpyDeviceToHost));
    }
    std::vector<int64_t> idx(n);
    for (int64_t i = 0; i < n; i++) idx[i] = i;
    std::sort(idx.begin(), idx.end(),
              [&](int64_t a, int64_t b) {
                  int an = flags[a] & 1, bn = flags[b] & 1;
                  if (an != bn) return an < bn;   /* NULL-key group LAST */
                  return okey[a] < okey[b];
              });
    gx_q3_group *g = (gx_q3_group *) malloc(sizeof(gx_q3_group) * std::max<int64_t>(n, 1));
    for (int64_t i = 0; i < n; i++)
    {
        g[i].l_orderkey = okey[idx[i]];
        g[i].o_orderdate = odate[idx[i]];
        g[i].o_shippriority = oprio[idx[i]];
        if (q->numeric)
        {
            int64_t num;
            memcpy(&num, &rev[idx[i]], 8);   /* agg slot held integer numerators */
            g[i].revenue_num = num;
            g[i].revenue = (double) num / 1e4;
        }
        else
        {
            g[i].revenue = rev[idx[i]];
            g[i].revenue_num = 0;
        }
        g[i].nitems = cnt[idx[i]];
        g[i].key_is_null = (uint8_t) (flags[idx[i]] & 1);
        g[i].attrs_null = (uint8_t) ((flags[idx[i]] >> 1) & 1);
        memset(g[i]._pad, 0, sizeof(g[i]._pad));
    }
    *out = g;
    *ngroups = n;
    return GX_OK;
}

/* top-N of THIS segment's groups (ORDER BY revenue DESC, o_orderdate ASC);
 * device-side per-block selection, host merge of blocks×K candidates.
 * At nsegs>1 each rank returns its local top-N; the coordinator-side merge
 * of nsegs×N rows is the reference's final Gather/Limit (trivial).
 * Two pieces, shared by gx_q3_topn and the test-only entry points: the
 * launch + copy over device SoA pointers, and a pure host merge. */
static constexpr int TOPN_GRID = 256;

struct topn_cands {
    std::vector<int64_t> idx, okey, cnt;  /* idx < 0: empty candidate */
    std::vector<int32_t> odate, oprio;
    std::vector<double> rev;
    std::vector<uint8_t> flags;
};

static gx_status topn_launch_copy(gx_ctx *ctx, const int64_t *okey,
                                  const int32_t *odate, const int32_t *oprio,
                                  const double *rev, const int64_t *cnt,
                                  const uint8_t *flags, int64_t n, int numeric,
                                  topn_cands &C)
{
    hipStream_t s = ctx->stream;
    const int nc = TOPN_GRID * TOPK;
    devbuf c_idx, c_okey, c_odate, c_oprio, c_rev, c_cnt, c_fl;
    HIP_CHK(ctx, c_idx.alloc(nc * 8));
    HIP_CHK(ctx, c_okey.alloc(nc * 8));
    HIP_CHK(ctx, c_odate.alloc(nc * 4));
    HIP_CHK(ctx, c_oprio.alloc(nc * 4));
    HIP_CHK(ctx, c_rev.alloc(nc * 8));
    HIP_CHK(ctx, c_cnt.alloc(nc * 8));
    HIP_CHK(ctx, c_fl.alloc(nc));
    auto launch = [&](auto num) {
        hipLaunchKernelGGL((k_topn<decltype(num)::value>), dim3(TOPN_GRID),
                           dim3(64), 0, s,
                           okey, odate, oprio, rev, cnt, flags, n,
                           c_idx.as<int64_t>(),
                           c_okey.as<int64_t>(), c_odate.as<int32_t>(),
                           c_oprio.as<int32_t>(), c_rev.as<double>(),
                           c_cnt.as<int64_t>(), c_fl.as<uint8_t>());
    };
    if (numeric) launch(std::true_type{});
    else launch(std::false_type{});
    C.idx.resize(nc); C.okey.resize(nc); C.cnt.resize(nc);
    C.odate.resize(nc); C.oprio.resize(nc); C.rev.resize(nc);
    C.flags.resize(nc);
    HIP_CHK(ctx, hipMemcpyAsync(C.idx.data(), c_idx.p, nc * 8, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipMemcpyAsync(C.flags.data(), c_fl.p, nc, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipMemcpyAsync(C.okey.data(), c_okey.p, nc * 8, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipMemcpyAsync(C.odate.data(), c_odate.p, nc * 4, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipMemcpyAsync(C.oprio.data(), c_oprio.p, nc * 4, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipMemcpyAsync(C.rev.data(), c_rev.p, nc * 8, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipMemcpyAsync(C.cnt.data(), c_cnt.p, nc * 8, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    return GX_OK;
}

/* pure host: order the valid candidates (idx >= 0) by revenue DESC, then
 * effective date ASC (flag bit 1 = NULL date = INT32_MAX, i.e. last), and
 * write the first topn as result rows.  Returns the number written. */
static int64_t topn_merge(const int64_t *cidx, const int64_t *okey,
                          const int32_t *odate, const int32_t *oprio,
                          const double *rev, const int64_t *cnt,
                          const uint8_t *flags, int ncand, int numeric,
                          int topn, gx_q3_group *out)
{
    std::vector<int> idx;
    for (int i = 0; i < ncand; i++)
        if (cidx[i] >= 0) idx.push_back(i);
    auto eff = [&](int i) { return (flags[i] & 2) ? INT32_MAX : odate[i]; };
    /* "a before b" = "b ranks after a" */
    if (numeric)
        std::sort(idx.begin(), idx.end(), [&](int a, int b) {
            return topn_less<true>(rev[b], eff(b), rev[a], eff(a));
        });
    else
        std::sort(idx.begin(), idx.end(), [&](int a, int b) {
            return topn_less<false>(rev[b], eff(b), rev[a], eff(a));
        });
    int64_t m = std::min<int64_t>(topn, (int64_t) idx.size());
    for (int64_t i = 0; i < m; i++)
    {
        int c = idx[i];
        out[i].l_orderkey = okey[c];
        out[i].o_orderdate = odate[c];
        out[i].o_shippriority = oprio[c];
        if (numeric)
        {
            int64_t num;
            memcpy(&num, &rev[c], 8);
            out[i].revenue_num = num;
            out[i].revenue = (double) num / 1e4;
        }
        else
        {
            out[i].revenue = rev[c];
            out[i].revenue_num = 0;
        }
        out[i].nitems = cnt[c];
        out[i].key_is_null = (uint8_t) (flags[c] & 1);
        out[i].attrs_null = (uint8_t) ((flags[c] >> 1) & 1);
        memset(out[i]._pad, 0, sizeof(out[i]._pad));
    }
    return m;
}

static gx_status topn_run(gx_ctx *ctx, const int64_t *okey,
                          const int32_t *odate, const int32_t *oprio,
                          const double *rev, const int64_t *cnt,
                          const uint8_t *flags, int64_t n, int numeric,
                          int topn, gx_q3_group *out, int64_t *nout)
{
    topn_cands C;
    gx_status st = topn_launch_copy(ctx, okey, odate, oprio, rev, cnt, flags,
                                    n, numeric, C);
    if (st != GX_OK) return st;
    *nout = topn_merge(C.idx.data(), C.okey.data(), C.odate.data(),
                       C.oprio.data(), C.rev.data(), C.cnt.data(),
                       C.flags.data(), (int) C.idx.size(), numeric, topn, out);
    return GX_OK;
}

extern "C" gx_status gx_q3_topn(gx_q3 *q, int topn, gx_q3_group *out, int64_t *nout)
{
    if (!q || !q->ran || topn <= 0 || topn > TOPK) return GX_ERR_STATE;
    const q3_results &r = q->res;
    const uint8_t *gflags = q->desc.fact_join == 1 ? r.flags.as<uint8_t>() : nullptr;
    return topn_run(q->ctx, r.okey.as<int64_t>(), r.odate.as<int32_t>(),
                    r.oprio.as<int32_t>(), r.rev.as<double>(),
                    r.cnt.as<int64_t>(), gflags, q->ngroups, q->numeric, topn,
                    out, nout);
}

/* test-only: the top-N stage over caller-supplied host SoA arrays (rev holds
 * int64 numerators when numeric != 0; flags may be NULL) — uploads them and
 * runs exactly what gx_q3_topn runs */
extern "C" gx_status gx_test_topn(gx_ctx *ctx, const int64_t *okey,
                                  const int32_t *odate, const int32_t *oprio,
                                  const double *rev, const int64_t *cnt,
                                  const uint8_t *flags, int64_t n, int numeric,
                                  int topn, gx_q3_group *out, int64_t *nout)
{
    if (!ctx) return GX_ERR_INVALID;
    if (n < 0 || topn <= 0 || topn > TOPK || !out || !nout ||
        (n > 0 && (!okey || !odate || !oprio || !rev || !cnt)))
    {
        set_err(ctx, "gx_test_topn: need n >= 0, 1 <= topn <= 10 and the "
                     "five SoA arrays%s", "");
        return GX_ERR_INVALID;
    }
    hipStream_t s = ctx->stream;
    devbuf d_okey, d_odate, d_oprio, d_rev, d_cnt, d_fl;
    HIP_CHK(ctx, d_okey.alloc(n * 8));
    HIP_CHK(ctx, d_odate.alloc(n * 4));
    HIP_CHK(ctx, d_oprio.alloc(n * 4));
    HIP_CHK(ctx, d_rev.alloc(n * 8));
    HIP_CHK(ctx, d_cnt.alloc(n * 8));
    if (flags) HIP_CHK(ctx, d_fl.alloc(n));
    if (n > 0)
    {
        HIP_CHK(ctx, hipMemcpyAsync(d_okey.p, okey, n * 8, hipMemcpyHostToDevice, s));
        HIP_CHK(ctx, hipMemcpyAsync(d_odate.p, odate, n * 4, hipMemcpyHostToDevice, s));
        HIP_CHK(ctx, hipMemcpyAsync(d_oprio.p, oprio, n * 4, hipMemcpyHostToDevice, s));
        HIP_CHK(ctx, hipMemcpyAsync(d_rev.p, rev, n * 8, hipMemcpyHostToDevice, s));
        HIP_CHK(ctx, hipMemcpyAsync(d_cnt.p, cnt, n * 8, hipMemcpyHostToDevice, s));
        if (flags)
            HIP_CHK(ctx, hipMemcpyAsync(d_fl.p, flags, n, hipMemcpyHostToDevice, s));
        HIP_CHK(ctx, hipStreamSynchronize(s));
    }
    return topn_run(ctx, d_okey.as<int64_t>(), d_odate.as<int32_t>(),
                    d_oprio.as<int32_t>(), d_rev.as<double>(),
                    d_cnt.as<int64_t>(), flags ? d_fl.as<uint8_t>() : nullptr,
                    n, numeric ? 1 : 0, topn, out, nout);
}

/* the host merge alone on caller-supplied candidate arrays (callable
 * without a GPU): cidx < 0 marks an empty candidate.  Returns 0, or 1 for
 * bad arguments. */
extern "C" int gx_selftest_topn_merge(const int64_t *cidx, const int64_t *okey,
                                      const int32_t *odate, const int32_t *oprio,
                                      const double *rev, const int64_t *cnt,
                                      const uint8_t *flags, int ncand,
                                      int numeric, int topn, gx_q3_group *out,
                                      int64_t *nout)
{
    if (ncand < 0 || topn <= 0 || topn > TOPK || !out || !nout ||
        (ncand > 0 && (!cidx || !okey || !odate || !oprio || !rev || !cnt ||
                       !flags)))
        return 1;
    *nout = topn_merge(cidx, okey, odate, oprio, rev, cnt, flags, ncand,
                       numeric ? 1 : 0, topn, out);
    return 0;
}

extern "C" gx_status gx_q3_free(gx_q3 *q)
{
    delete q;
    return GX_OK;
}

extern "C" void gx_free(void *p) { free(p); }

/* ---- descriptor-form GROUP BY: host side (kernels: k_groupby_desc) ---- */

/* LDS table slots of one workgroup, a power of two: sized for the worst
 * slot of naggs aggregates (two words each and an 8-byte row word) within
 * GBD_LDS_BYTES, whatever the aggregates' functions, so the capacity depends
 * on naggs alone. */
static uint32_t gbd_lds_slots(int naggs)
{
    uint32_t slots = 1024;
    while (slots > 1 && (size_t) slots * (16 * (size_t) naggs + 8) > GBD_LDS_BYTES)
        slots >>= 1;
    return slots;
}

extern "C" int32_t gx_gb_lds_groups(int naggs)
{
    if (naggs < 1 || naggs > GX_GB_MAX_AGGS) return 0;
    return (int32_t) gbd_lds_slots(naggs);
}

/* the result order: (key_null, key) pairs column by column, ascending =
 * lexicographic by key with NULLS LAST per column; stable */
static void gbd_sort_perm(const int64_t *keys, const uint8_t *key_null,
                          int64_t n, int nkeys, int64_t *perm)
{
    for (int64_t i = 0; i < n; i++) perm[i] = i;
    std::stable_sort(perm, perm + n, [&](int64_t x, int64_t y) {
        for (int k = 0; k < nkeys; k++)
        {
            uint8_t nx = key_null[x * nkeys + k], ny = key_null[y * nkeys + k];
            if (nx != ny) return nx < ny;
            int64_t kx = keys[x * nkeys + k], ky = keys[y * nkeys + k];
            if (kx != ky) return kx < ky;
        }
        return false;
    });
}

extern "C" int gx_selftest_gb_sort(const int64_t *keys, const uint8_t *key_null,
                                   int64_t n, int nkeys, int64_t *perm)
{
    if (n < 0 || nkeys < 1 || nkeys > GX_GB_MAX_KEYS || !perm ||
        (n > 0 && (!keys || !key_null)))
        return 1;
    gbd_sort_perm(keys, key_null, n, nkeys, perm);
    return 0;
}

extern "C" void gx_gb_result_free(gx_gb_result *r)
{
    if (!r) return;
    free(r->keys); free(r->key_null); free(r->aggs); free(r->agg_null);
    memset(r, 0, sizeof *r);
}

static gx_status gbd_invalid(gx_ctx *ctx, const char *fmt, long a, long b = 0,
                             long c = 0)
{
    char buf[200];
    snprintf(buf, sizeof buf, fmt, a, b, c);
    set_err(ctx, "groupby_desc: %s", buf);
    return GX_ERR_INVALID;
}

/* flattened inputs of one call; a table column used in several roles is
 * materialized once */
struct gbd_inputs {
    devbuf flat[GX_GB_MAX_KEYS + GX_GB_MAX_AGGS + GX_MAX_EXTRA_QUALS +
                GX_GB_MAX_OPERANDS + GX_GBJ_MAX_JOINS];
    devbuf val[GX_GB_MAX_KEYS + GX_GB_MAX_AGGS + GX_MAX_EXTRA_QUALS +
               GX_GB_MAX_OPERANDS + GX_GBJ_MAX_JOINS];
    int nflat = 0;
    std::map<int, gbd_col> done;
};

static gx_status gbd_bind_col(gx_ctx *ctx, const gx_table *t, int col,
                              gbd_inputs &in, gbd_col *out)
{
    auto it = in.done.find(col);
    if (it != in.done.end()) { *out = it->second; return GX_OK; }
    gbd_col c{};
    gx_status st = gb_flat(ctx, t->cols[col], in.flat[in.nflat], in.val[in.nflat],
                           &c.s, &c.m, &c.val);
    if (st != GX_OK) return st;
    in.nflat++;
    in.done[col] = c;
    *out = c;
    return GX_OK;
}

static bool gbd_int_width(int w) { return w == 1 || w == 2 || w == 4 || w == 8; }

/* state words of one aggregate: COUNTs one, SUM / MIN / MAX a second one
 * counting their non-NULL inputs */
static int gbd_fn_words(int fn) { return fn <= GX_AGG_COUNT ? 1 : 2; }

/* the expression side of a planned call: on = the EXPR instantiations run
 * (the ext names an expression or an fqual); opnd_col[o] = the table column
 * of operand o */
struct gbd_xplan {
    gbd_xargs x{};
    bool on = false;
    int opnd_col[GX_GB_MAX_OPERANDS] = {};
};

/* index of table column c among the operands, appended when new; -1 when
 * the table is full */
static int gbd_operand(gbd_xplan &xp, int c)
{
    for (int o = 0; o < xp.x.nopnd; o++)
        if (xp.opnd_col[o] == c) return o;
    if (xp.x.nopnd == GX_GB_MAX_OPERANDS) return -1;
    xp.opnd_col[xp.x.nopnd] = c;
    return xp.x.nopnd++;
}

/* validate a gx_gb_ext against the table and fill the operand, factor and
 * fqual tables; agg_expr is checked with the aggregates in gbd_plan */
static gx_status gbd_plan_ext(gx_ctx *ctx, const gx_gb_ext *ext, const gx_table *t,
                              gbd_xplan &xp)
{
    const int ncols = (int) t->cols.size();
    if (ext->nexprs < 0 || ext->nexprs > GX_GB_MAX_AGGS)
        return gbd_invalid(ctx, "nexprs %ld outside 0..%ld", ext->nexprs, GX_GB_MAX_AGGS);
    if (ext->nfquals < 0 || ext->nfquals > GX_GB_MAX_FQUALS)
        return gbd_invalid(ctx, "nfquals %ld outside 0..%ld", ext->nfquals, GX_GB_MAX_FQUALS);
    gbd_xargs &x = xp.x;
    x.nexprs = ext->nexprs;
    x.nfquals = ext->nfquals;
    for (int e = 0; e < ext->nexprs; e++)
    {
        const gx_expr &ex = ext->exprs[e];
        if (ex.nfactors < 1 || ex.nfactors > GX_GB_MAX_FACTORS)
            return gbd_invalid(ctx, "expr %ld: nfactors %ld outside 1..%ld", e,
                               ex.nfactors, GX_GB_MAX_FACTORS);
        x.nfactors[e] = ex.nfactors;
        for (int f = 0; f < ex.nfactors; f++)
        {
            const int c = ex.f[f].col;
            if (c < 0 || c >= ncols)
                return gbd_invalid(ctx, "expr %ld factor %ld: column %ld out of range", e, f, c);
            if (t->cols[c].m.width != 8)
                return gbd_invalid(ctx, "expr %ld factor %ld: column width %ld is not 8",
                                   e, f, t->cols[c].m.width);
            if (ex.f[f].form < GX_FACTOR_COL || ex.f[f].form > GX_FACTOR_ONE_PLUS)
                return gbd_invalid(ctx, "expr %ld factor %ld: form %ld outside 0..2", e, f,
                                   ex.f[f].form);
            const int o = gbd_operand(xp, c);
            if (o < 0)
                return gbd_invalid(ctx, "more than %ld distinct float8 operand columns",
                                   GX_GB_MAX_OPERANDS);
            x.fopnd[e][f] = o;
            x.fform[e][f] = ex.f[f].form;
            x.emask[e] |= 1u << o;
        }
    }
    for (int q = 0; q < ext->nfquals; q++)
    {
        const gx_fqual &fq = ext->fquals[q];
        if (fq.col < 0 || fq.col >= ncols)
            return gbd_invalid(ctx, "fqual %ld: column %ld out of range", q, fq.col);
        if (t->cols[fq.col].m.width != 8)
            return gbd_invalid(ctx, "fqual %ld: column width %ld is not 8", q,
                               t->cols[fq.col].m.width);
        if (fq.op < 0 || fq.op > 5)
            return gbd_invalid(ctx, "fqual %ld: op %ld outside 0..5", q, fq.op);
        const int o = gbd_operand(xp, fq.col);
        if (o < 0)
            return gbd_invalid(ctx, "more than %ld distinct float8 operand columns",
                               GX_GB_MAX_OPERANDS);
        uint64_t bits;
        memcpy(&bits, &fq.literal, 8);
        x.fqopnd[q] = o;
        x.fqop[q] = fq.op;
        x.fqimg[q] = gbd_fq_image(bits);
    }
    xp.on = ext->nexprs > 0 || ext->nfquals > 0;
    return GX_OK;
}

/* the join side of a planned call: on = the JOIN instantiations run (the
 * ext names a join); b[j] / slots[j] = join j's build arguments and table */
struct gbj_plan {
    gbd_jargs jx{};
    bool on = false;
    const gx_gbj_ext *ext = nullptr;
    gbj_build_args b[GX_GBJ_MAX_JOINS] = {};
    uint64_t nslots[GX_GBJ_MAX_JOINS] = {};
    gbd_inputs din[GX_GBJ_MAX_JOINS];
    devbuf slots[GX_GBJ_MAX_JOINS], misc;
    int64_t dim_rows[GX_GBJ_MAX_JOINS] = {};
    double ms_build = 0;
    /* the table side `side` of a key or an aggregate names */
    const gx_table *table(const gx_table *fact, int side) const
    { return side == 0 ? fact : ext->joins[side - 1].dim; }
};

static uint64_t gbj_slots(int64_t dim_rows)
{
    return (uint64_t) pow2_at_least(dim_rows * 2);
}

/* validate a gx_gbj_ext against the tables: the joins, their quals and the
 * sides; the key and aggregate columns are checked in gbd_plan against the
 * table their side names */
static gx_status gbj_plan_ext(gx_ctx *ctx, const gx_gb_desc *d,
                              const gx_gbj_ext *jext, gbj_plan &jp)
{
    const gx_table *t = d->t;
    if (jext->njoins < 0 || jext->njoins > GX_GBJ_MAX_JOINS)
        return gbd_invalid(ctx, "njoins %ld outside 0..%ld", jext->njoins,
                           GX_GBJ_MAX_JOINS);
    jp.ext = jext;
    jp.on = jext->njoins > 0;
    gbd_jargs &jx = jp.jx;
    jx.njoins = jext->njoins;
    for (int j = 0; j < jext->njoins; j++)
    {
        const gx_gb_join &J = jext->joins[j];
        if (!J.dim) return gbd_invalid(ctx, "join %ld: no dimension table", j);
        if (J.dim->nrows >= (int64_t) UINT32_MAX)
            return gbd_invalid(ctx, "join %ld: a dimension of %ld rows does not fit "
                                    "the 4-byte join-table slot", j, (long) J.dim->nrows);
        const int nf = (int) t->cols.size(), nd = (int) J.dim->cols.size();
        if (J.fact_col < 0 || J.fact_col >= nf)
            return gbd_invalid(ctx, "join %ld: fact column %ld out of range", j, J.fact_col);
        if (!gbd_int_width(t->cols[J.fact_col].m.width))
            return gbd_invalid(ctx, "join %ld: fact column width %ld is not 1, 2, 4 or 8",
                               j, t->cols[J.fact_col].m.width);
        if (J.dim_key_col < 0 || J.dim_key_col >= nd)
            return gbd_invalid(ctx, "join %ld: dimension key column %ld out of range", j,
                               J.dim_key_col);
        if (!gbd_int_width(J.dim->cols[J.dim_key_col].m.width))
            return gbd_invalid(ctx, "join %ld: dimension key column width %ld is not "
                                    "1, 2, 4 or 8", j, J.dim->cols[J.dim_key_col].m.width);
        if (J.nquals < 0 || J.nquals > GX_MAX_EXTRA_QUALS)
            return gbd_invalid(ctx, "join %ld: nquals %ld outside 0..%ld", j, J.nquals,
                               GX_MAX_EXTRA_QUALS);
        gbj_build_args &b = jp.b[j];
        b.nquals = J.nquals;
        b.nrows = J.dim->nrows;
        b.vmap = J.dim->dvmap;
        for (int q = 0; q < J.nquals; q++)
        {
            const gx_filter &f = J.quals[q];
            if (f.col < 0 || f.col >= nd)
                return gbd_invalid(ctx, "join %ld qual %ld: column %ld out of range", j, q,
                                   f.col);
            const int w = J.dim->cols[f.col].m.width;
            if (!gbd_int_width(w))
                return gbd_invalid(ctx, "join %ld qual %ld: column width %ld is not "
                                        "1, 2, 4 or 8", j, q, w);
            b.qop[q] = f.op;
            b.qlit[q] = f.literal;
            if (!gx_fold_filter(w, &b.qop[q], &b.qlit[q]))
                return gbd_invalid(ctx, "join %ld qual %ld: op %ld outside 0..5", j, q, f.op);
        }
        jp.nslots[j] = gbj_slots(J.dim->nrows);
    }
    for (int k = 0; k < d->nkeys; k++)
    {
        const int side = jext->key_side[k];
        if (side < 0 || side > jext->njoins)
            return gbd_invalid(ctx, "key %ld: side %ld outside 0..%ld", k, side,
                               jext->njoins);
        jx.key_side[k] = side;
        if (side) jx.key_joins |= 1u << (side - 1);
    }
    for (int j = 0; j < d->naggs; j++)
    {
        const int side = jext->agg_side[j];
        if (side < 0 || side > jext->njoins)
            return gbd_invalid(ctx, "aggregate %ld: side %ld outside 0..%ld", j, side,
                               jext->njoins);
        jx.agg_side[j] = side;
    }
    return GX_OK;
}

/* One planned call: the descriptors as the caller gave them and everything
 * planned from them.  t is the scanned table, nullptr for the combine-only
 * plan over wire rows (d->t is then never read); ext and jext may be null (a
 * table is required with either).  Without ext xp.on is false, without jext
 * jp.on is false and every side is 0, so no reader asks for the pointers. */
struct gbd_call {
    const gx_gb_desc *d;
    const gx_table *t;
    const gx_gb_ext *ext;
    const gx_gbj_ext *jext;
    gbd_args a;
    gbd_xplan xp;
    gbj_plan jp;
    gbd_inputs in;
    gbd_call(const gx_gb_desc *d_, const gx_table *t_, const gx_gb_ext *ext_,
             const gx_gbj_ext *jext_) : d(d_), t(t_), ext(ext_), jext(jext_) {}
    /* the table key k / column aggregate j reads (its side's) */
    const gx_table *key_table(int k) const { return jp.table(t, jp.jx.key_side[k]); }
    const gx_table *agg_table(int j) const { return jp.table(t, jp.jx.agg_side[j]); }
    /* aggregate j takes an expression's value, not a column's */
    bool agg_is_expr(int j) const { return xp.on && xp.x.aexpr[j] >= 0; }
    /* aggregate j reads a column that has to be bound */
    bool agg_reads_col(int j) const
    { return d->aggs[j].fn != GX_AGG_COUNT_STAR && !agg_is_expr(j); }
};

/* PLAN: validate the descriptors and fill everything of the call that needs
 * no device memory.  The combine-only plan checks and reads nkeys, the
 * aggregates' fn / is_f64 and max_groups only.  With a join, a key or a
 * column aggregate is checked against the table its side names. */
static gx_status gbd_plan(gx_ctx *ctx, gbd_call &c)
{
    const gx_gb_desc *d = c.d;
    const gx_table *t = c.t;
    const gx_gb_ext *ext = c.ext;
    gbd_args &a = c.a;
    const int ncols = t ? (int) t->cols.size() : 0;
    if (d->nkeys < 0 || d->nkeys > GX_GB_MAX_KEYS)
        return gbd_invalid(ctx, "nkeys %ld outside 0..%ld", d->nkeys, GX_GB_MAX_KEYS);
    if (d->naggs < 1 || d->naggs > GX_GB_MAX_AGGS)
        return gbd_invalid(ctx, "naggs %ld outside 1..%ld", d->naggs, GX_GB_MAX_AGGS);
    if (t && (d->nquals < 0 || d->nquals > GX_MAX_EXTRA_QUALS))
        return gbd_invalid(ctx, "nquals %ld outside 0..%ld", d->nquals, GX_MAX_EXTRA_QUALS);
    if (d->max_groups < 0)
        return gbd_invalid(ctx, "max_groups %ld is negative", (long) d->max_groups);

    if (ext)
    {
        gx_status st = gbd_plan_ext(ctx, ext, t, c.xp);
        if (st != GX_OK) return st;
    }
    if (c.jext)
    {
        gx_status st = gbj_plan_ext(ctx, d, c.jext, c.jp);
        if (st != GX_OK) return st;
    }
    a = gbd_args{};
    a.nkeys = d->nkeys; a.naggs = d->naggs; a.nquals = t ? d->nquals : 0;
    a.nrows = t ? t->nrows : 0;
    a.vmap = t ? t->dvmap : nullptr;
    /* validate everything before the first flatten launches */
    for (int k = 0; t && k < d->nkeys; k++)
    {
        const int col = d->key_cols[k];
        const gx_table *kt = c.key_table(k);
        if (col < 0 || col >= (int) kt->cols.size())
            return gbd_invalid(ctx, "key %ld: column %ld out of range", k, col);
        if (!gbd_int_width(kt->cols[col].m.width))
            return gbd_invalid(ctx, "key %ld: column width %ld is not 1, 2, 4 or 8",
                               k, kt->cols[col].m.width);
    }
    int words = 0;
    for (int j = 0; j < d->naggs; j++)
    {
        gx_agg g = d->aggs[j];
        if (g.fn < GX_AGG_COUNT_STAR || g.fn > GX_AGG_MAX)
            return gbd_invalid(ctx, "aggregate %ld: unknown fn %ld", j, g.fn);
        a.aword[j] = words;
        const int ae = ext ? ext->agg_expr[j] : -1;
        if (ext)
        {
            if (ae < -1 || ae >= ext->nexprs)
                return gbd_invalid(ctx, "aggregate %ld: agg_expr %ld outside -1..%ld", j,
                                   ae, ext->nexprs - 1);
            if (ae >= 0 && g.fn == GX_AGG_COUNT_STAR)
                return gbd_invalid(ctx, "aggregate %ld: agg_expr %ld on COUNT(*)", j, ae);
            c.xp.x.aexpr[j] = ae;
        }
        /* an expression aggregate is "float8 of that fn": col is not read */
        if (ae >= 0) g.is_f64 = 1;
        if (g.fn == GX_AGG_COUNT_STAR)
        {
            a.aop[j] = GBD_COUNT_STAR;
            a.wop[words++] = GBD_W_ADD;
            continue;
        }
        int w = ae >= 0 ? 8 : 0;
        if (t && ae < 0)
        {
            const gx_table *at = c.agg_table(j);
            if (g.col < 0 || g.col >= (int) at->cols.size())
                return gbd_invalid(ctx, "aggregate %ld: column %ld out of range", j, g.col);
            w = at->cols[g.col].m.width;
            if (g.is_f64 ? w != 8 : !gbd_int_width(w))
                return gbd_invalid(ctx, g.is_f64
                                       ? "aggregate %ld: is_f64 on a column of width %ld"
                                       : "aggregate %ld: column width %ld is not 1, 2, 4 or 8",
                                   j, w);
        }
        if (g.fn == GX_AGG_COUNT)
        {
            a.aop[j] = GBD_COUNT;
            a.wop[words++] = GBD_W_ADD;
            continue;
        }
        if (g.fn == GX_AGG_SUM && !g.is_f64 && w == 8)
            return gbd_invalid(ctx, "aggregate %ld: SUM over a width-8 integer "
                                    "column (%ld) is numeric in the reference", j, g.col);
        if (g.fn == GX_AGG_SUM)
        {
            a.aop[j] = g.is_f64 ? GBD_SUM_F64 : GBD_SUM_INT;
            a.wop[words++] = g.is_f64 ? GBD_W_FADD : GBD_W_ADD;
        }
        else
        {
            a.aop[j] = g.fn == GX_AGG_MAX ? (g.is_f64 ? GBD_MAX_F64 : GBD_MAX_INT)
                                          : (g.is_f64 ? GBD_MIN_F64 : GBD_MIN_INT);
            a.wop[words++] = GBD_W_MAX;
        }
        a.wop[words++] = GBD_W_ADD;                  /* non-NULL input count */
    }
    a.awords = words;
    for (int q = 0; t && q < d->nquals; q++)
    {
        const gx_filter &f = d->quals[q];
        if (f.col < 0 || f.col >= ncols)
            return gbd_invalid(ctx, "qual %ld: column %ld out of range", q, f.col);
        int w = t->cols[f.col].m.width;
        if (!gbd_int_width(w))
            return gbd_invalid(ctx, "qual %ld: column width %ld is not 1, 2, 4 or 8", q, w);
        a.qop[q] = f.op;
        a.qlit[q] = f.literal;
        if (!gx_fold_filter(w, &a.qop[q], &a.qlit[q]))
            return gbd_invalid(ctx, "qual %ld: op %ld outside 0..5", q, f.op);
    }
    a.lds_slots = gbd_lds_slots(d->naggs);
    /* measurement knob: 0 = never give up */
    int gr = env_int("GX_GB_GIVEUP_ROWS", (int) GBD_GIVEUP_ROWS);
    a.giveup_rows = gr > 0 ? (uint32_t) gr : UINT32_MAX;
    return GX_OK;
}

extern "C" int64_t gx_gbd_wire_stride(const gx_gb_desc *d)
{
    if (!d || d->nkeys < 0 || d->nkeys > GX_GB_MAX_KEYS || d->naggs < 1 ||
        d->naggs > GX_GB_MAX_AGGS)
        return -1;
    int words = 0;
    for (int j = 0; j < d->naggs; j++)
    {
        if (d->aggs[j].fn < GX_AGG_COUNT_STAR || d->aggs[j].fn > GX_AGG_MAX) return -1;
        words += gbd_fn_words(d->aggs[j].fn);
    }
    return 8 * (int64_t) (d->nkeys + (d->nkeys ? 1 : 0) + words);
}

/* BIND: flatten every column the plan reads */
static gx_status gbd_bind(gx_ctx *ctx, gbd_call &c)
{
    const gx_gb_desc *d = c.d;
    const gx_table *t = c.t;
    gbd_args &a = c.a;
    gbj_plan &jp = c.jp;
    gx_status st;
    /* a dim-side key or aggregate binds the dimension's column */
    auto bind_side = [&](int side, int col, gbd_col *out) {
        return side == 0 ? gbd_bind_col(ctx, t, col, c.in, out)
                         : gbd_bind_col(ctx, jp.ext->joins[side - 1].dim, col,
                                        jp.din[side - 1], out);
    };
    for (int k = 0; k < d->nkeys; k++)
        if ((st = bind_side(jp.jx.key_side[k], d->key_cols[k], &a.key[k])) != GX_OK)
            return st;
    for (int j = 0; j < d->naggs; j++)
        if (c.agg_reads_col(j) &&
            (st = bind_side(jp.jx.agg_side[j], d->aggs[j].col, &a.agg[j])) != GX_OK)
            return st;
    for (int q = 0; q < d->nquals; q++)
        if ((st = gbd_bind_col(ctx, t, d->quals[q].col, c.in, &a.qual[q])) != GX_OK) return st;
    for (int o = 0; c.xp.on && o < c.xp.x.nopnd; o++)
        if ((st = gbd_bind_col(ctx, t, c.xp.opnd_col[o], c.in, &c.xp.x.opnd[o])) != GX_OK)
            return st;
    for (int j = 0; j < jp.jx.njoins; j++)
    {
        const gx_gb_join &J = jp.ext->joins[j];
        if ((st = gbd_bind_col(ctx, t, J.fact_col, c.in, &jp.jx.j[j].fact)) != GX_OK ||
            (st = gbd_bind_col(ctx, J.dim, J.dim_key_col, jp.din[j],
                               &jp.jx.j[j].dkey)) != GX_OK)
            return st;
        jp.b[j].key = jp.jx.j[j].dkey;
        for (int q = 0; q < J.nquals; q++)
            if ((st = gbd_bind_col(ctx, J.dim, J.quals[q].col, jp.din[j],
                                   &jp.b[j].qual[q])) != GX_OK) return st;
    }
    return GX_OK;
}

/* bytes a join scan allocates beside the group table: the join tables and the
 * flat copies (value and validity bytes) gbd_bind materialises for format-1
 * dimension columns; for the budget check before anything is bound */
static uint64_t gbj_bytes(const gbd_call &c)
{
    const gx_gb_desc *d = c.d;
    const gbj_plan &jp = c.jp;
    if (!jp.on) return 0;
    uint64_t b = 64;
    std::set<std::pair<int, int>> seen;
    auto col = [&](int j, int cc) {
        const gx_table *dim = jp.ext->joins[j].dim;
        if (dim->cols[cc].format != 0 && seen.insert({j, cc}).second)
            b += GX_AOCS_DATUM_OFF + (uint64_t) std::max<int64_t>(dim->nrows, 1) *
                                         (uint64_t) (dim->cols[cc].m.width + 1);
    };
    for (int j = 0; j < jp.jx.njoins; j++)
    {
        b += jp.nslots[j] * 4;
        col(j, jp.ext->joins[j].dim_key_col);
        for (int q = 0; q < jp.ext->joins[j].nquals; q++)
            col(j, jp.ext->joins[j].quals[q].col);
    }
    for (int k = 0; k < d->nkeys; k++)
        if (jp.jx.key_side[k]) col(jp.jx.key_side[k] - 1, d->key_cols[k]);
    for (int j = 0; j < d->naggs; j++)
        if (jp.jx.agg_side[j] && c.agg_reads_col(j))
            col(jp.jx.agg_side[j] - 1, d->aggs[j].col);
    return b;
}

/* BUILD the join tables of a bound plan and report a duplicate key among the
 * participating rows of a dimension (one host sync) */
static gx_status gbj_build(gx_ctx *ctx, gbj_plan &jp)
{
    hipStream_t s = ctx->stream;
    const int nj = jp.jx.njoins;
    evholder e0, e1;
    HIP_CHK(ctx, e0.create()); HIP_CHK(ctx, e1.create());
    HIP_CHK(ctx, jp.misc.alloc(32 * GX_GBJ_MAX_JOINS));
    HIP_CHK(ctx, hipMemsetAsync(jp.misc.p, 0, 32 * GX_GBJ_MAX_JOINS, s));
    for (int j = 0; j < nj; j++)
    {
        HIP_CHK(ctx, jp.slots[j].alloc(jp.nslots[j] * 4));
        HIP_CHK(ctx, hipMemsetAsync(jp.slots[j].p, 0, jp.nslots[j] * 4, s));
    }
    HIP_CHK(ctx, hipEventRecord(e0, s));
    for (int j = 0; j < nj; j++)
    {
        const int grid = (int) std::max<int64_t>(
            1, std::min<int64_t>(GRID, (jp.b[j].nrows + TPB - 1) / TPB));
        hipLaunchKernelGGL(k_gbj_build, dim3(grid), dim3(TPB), 0, s, jp.b[j],
                           jp.slots[j].as<uint32_t>(), jp.nslots[j] - 1,
                           jp.misc.as<unsigned long long>() + 4 * j);
        jp.jx.j[j].slots = jp.slots[j].as<uint32_t>();
        jp.jx.j[j].mask = jp.nslots[j] - 1;
    }
    HIP_CHK(ctx, hipEventRecord(e1, s));
    unsigned long long hm[4 * GX_GBJ_MAX_JOINS] = {};
    HIP_CHK(ctx, hipMemcpyAsync(hm, jp.misc.p, sizeof hm, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    float ms = 0;
    (void) hipEventElapsedTime(&ms, e0, e1);
    jp.ms_build = (double) ms;
    for (int j = 0; j < nj; j++)
    {
        if (hm[4 * j + 1] & 1)
        {
            char buf[120];
            snprintf(buf, sizeof buf, "join %d: duplicate dimension key %lld among the "
                                      "rows that take part", j, (long long) hm[4 * j + 2]);
            set_err(ctx, "groupby_desc: %s", buf);
            return GX_ERR_INVALID;
        }
        jp.dim_rows[j] = (int64_t) hm[4 * j];
    }
    return GX_OK;
}

/* bytes gbd_bind materialises for the operand columns (format 1: a flat
 * copy and validity bytes), for the budget check before anything is bound */
static uint64_t gbd_operand_flat_bytes(const gbd_call &c)
{
    uint64_t b = 0;
    for (int o = 0; c.xp.on && o < c.xp.x.nopnd; o++)
        if (c.t->cols[c.xp.opnd_col[o]].format != 0)
            b += GX_AOCS_DATUM_OFF + (uint64_t) std::max<int64_t>(c.t->nrows, 1) * 9;
    return b;
}

/* one aggregation table on the device and its compacted groups: the scan's
 * over input rows, or the combine stage's over wire rows */
struct gbd_table {
    devbuf trow, tacc, misc;       /* misc: [0..1] stats, [2] cursor, [3] err,
                                      [4] a join scan's probed rows */
    devbuf okeys, oknull, oacc;    /* compacted groups, SoA, up to bound */
    uint64_t tslots = 0;
    int64_t bound = 0;
    size_t sw = 4;                 /* bytes of the slot word */
    unsigned long long hm[5] = {}; /* misc on the host: read_stats, then a sync */
    unsigned long long *stat() const { return misc.as<unsigned long long>(); }
    unsigned long long *cursor() const { return stat() + 2; }
    int *err() const { return (int *) (stat() + 3); }
    /* enqueue the one copy of the stat words a call makes */
    hipError_t read_stats(hipStream_t s)
    { return hipMemcpyAsync(hm, misc.p, sizeof hm, hipMemcpyDeviceToHost, s); }
    int64_t ngroups() const { return (int64_t) hm[2]; }
};

/* the rule for the slot word: 8 bytes from 2^32 - 1 rows on, or when a test
 * seam forces it */
static bool gbd_wide(int64_t nrows, bool force)
{
    return force || nrows >= (int64_t) UINT32_MAX;
}

/* the overflow verdict on a table whose stat words are on the host: the
 * bounded walk ran out, or the extract counted more groups than the table
 * was sized for (bound never exceeds a positive max_groups) */
static gx_status gbd_verdict(gx_ctx *ctx, const gbd_table &T)
{
    if (!(T.hm[3] & 1) && T.ngroups() <= T.bound) return GX_OK;
    set_err(ctx, "groupby_desc: more groups than max_groups%s", "");
    return GX_ERR_INVALID;
}

/* HBM budget of a table for up to `bound` groups at a fill of 1/2 at most,
 * plus `extra` bytes the caller allocates beside it */
static gx_status gbd_table_budget(gx_ctx *ctx, const gbd_args &a, int64_t bound,
                                  bool wide, uint64_t extra, const char *what)
{
    const uint64_t tslots = (uint64_t) pow2_at_least(bound * 2);
    return hbm_budget_check(
        ctx, tslots * ((wide ? 8 : 4) + (uint64_t) a.awords * 8) +
                 (uint64_t) bound * ((uint64_t) a.awords * 8 + (uint64_t) a.nkeys * 9) +
                 64 + extra,
        what);
}

/* allocate and clear (enqueue only) */
static gx_status gbd_table_alloc(gx_ctx *ctx, gbd_table &T, const gbd_args &a,
                                 int64_t bound, bool wide)
{
    hipStream_t s = ctx->stream;
    const int words = a.awords, nk = a.nkeys;
    T.bound = bound;
    T.tslots = (uint64_t) pow2_at_least(bound * 2);
    T.sw = wide ? 8 : 4;
    HIP_CHK(ctx, T.trow.alloc(T.tslots * T.sw));
    HIP_CHK(ctx, T.tacc.alloc(T.tslots * (size_t) words * 8));
    HIP_CHK(ctx, T.misc.alloc(40));
    HIP_CHK(ctx, T.okeys.alloc((size_t) bound * std::max(nk, 1) * 8));
    HIP_CHK(ctx, T.oknull.alloc((size_t) bound * std::max(nk, 1)));
    HIP_CHK(ctx, T.oacc.alloc((size_t) bound * words * 8));
    HIP_CHK(ctx, hipMemsetAsync(T.trow.p, 0, T.tslots * T.sw, s));
    HIP_CHK(ctx, hipMemsetAsync(T.tacc.p, 0, T.tslots * (size_t) words * 8, s));
    HIP_CHK(ctx, hipMemsetAsync(T.misc.p, 0, 40, s));
    /* a plain aggregate's one group is all-identity until the extract writes
     * it: the state row the two-stage plan ships for an empty shard */
    if (nk == 0)
        HIP_CHK(ctx, hipMemsetAsync(T.oacc.p, 0, (size_t) words * 8, s));
    return GX_OK;
}

/* EXTRACT: the table's groups into okeys / oknull / oacc, their count into
 * the cursor (enqueue only); src reads a representative row's keys */
template <typename SRC>
static void gbd_extract(gx_ctx *ctx, const gbd_args &a, const SRC &src, gbd_table &T)
{
    const int xgrid = (int) std::min<uint64_t>(GRID, (T.tslots + TPB - 1) / TPB);
    by_width((int) T.sw, (const void *) T.trow.p, [&](auto *rows) {
        hipLaunchKernelGGL((k_gbd_extract<std::decay_t<decltype(*rows)>, SRC>),
                           dim3(xgrid), dim3(TPB), 0, ctx->stream, a, src, rows,
                           T.tacc.as<unsigned long long>(), T.tslots,
                           T.okeys.as<int64_t>(), T.oknull.as<uint8_t>(),
                           T.oacc.as<unsigned long long>(), T.cursor(), T.bound);
    });
}

/* what a production entry point and its test seam differ in: the scan
 * kernel's grid and whether the 8-byte slot word is forced */
struct gbd_launch {
    int grid;
    bool force_wide;
};
static const gbd_launch GBD_PRODUCTION = {GRID, false};
static gbd_launch gbd_test_launch(int grid, int wide_rowid)
{
    return gbd_launch{grid == 0 ? GRID : grid, wide_rowid != 0};
}

static bool gbd_env_lds() { return env_int("GX_GB_LDS", 1) != 0; }

/* SCAN stage of a planned call: budget, bind, table, k_groupby_desc (between
 * e0 and e1 when given), extract.  Enqueue only: the group count and the
 * error word stay on the device (T.misc) until the caller syncs.  extra:
 * bytes the caller allocates beside the table. */
static gx_status gbd_scan_stage(gx_ctx *ctx, gbd_call &c, gbd_table &T,
                                const gbd_launch &launch, uint64_t extra,
                                hipEvent_t e0, hipEvent_t e1)
{
    const gbd_args &a = c.a;
    const int grid = launch.grid;
    if (grid < 1) return gbd_invalid(ctx, "grid %ld", grid);
    /* sizing: the table holds up to `bound` groups */
    const int64_t n = c.t->nrows;
    const int64_t bound = std::max<int64_t>(
        1, c.d->max_groups > 0 ? std::min<int64_t>(c.d->max_groups, n) : n);
    const bool wide = gbd_wide(n, launch.force_wide);
    const bool lds = gbd_env_lds(), jn = c.jp.on;
    gx_status st = gbd_table_budget(ctx, a, bound, wide,
                                    extra + gbd_operand_flat_bytes(c) + gbj_bytes(c),
                                    jn ? "groupby_desc table and join tables"
                                       : "groupby_desc table");
    if (st != GX_OK) return st;
    if ((st = gbd_bind(ctx, c)) != GX_OK) return st;
    if (jn && (st = gbj_build(ctx, c.jp)) != GX_OK) return st;
    if ((st = gbd_table_alloc(ctx, T, a, bound, wide)) != GX_OK) return st;
    hipStream_t s = ctx->stream;
    const size_t lds_bytes = lds ? (size_t) a.lds_slots * ((size_t) a.awords * 8 + T.sw) : 0;
    if (e0) HIP_CHK(ctx, hipEventRecord(e0, s));
    by_width((int) T.sw, T.trow.p, [&](auto *rows) {
        by_flag(lds, [&](auto use_lds) {
            by_flag(c.xp.on, [&](auto use_expr) {
                by_flag(jn, [&](auto use_join) {
                    constexpr bool EX = decltype(use_expr)::value;
                    constexpr bool JN = decltype(use_join)::value;
                    std::conditional_t<EX, gbd_xargs, gbd_noexpr> x{};
                    std::conditional_t<JN, gbd_jargs, gbd_nojoin> jx{};
                    if constexpr (EX) x = c.xp.x;
                    if constexpr (JN) jx = c.jp.jx;
                    hipLaunchKernelGGL((k_groupby_desc<std::decay_t<decltype(*rows)>,
                                                       decltype(use_lds)::value, EX, JN>),
                                       dim3(grid), dim3(TPB), lds_bytes, s, a, x, jx,
                                       rows, T.tacc.as<unsigned long long>(),
                                       T.tslots - 1, T.stat(), T.err());
                });
            });
        });
    });
    if (e1) HIP_CHK(ctx, hipEventRecord(e1, s));
    if (jn) gbd_extract(ctx, a, gbd_key_join_args{c.jp.jx}, T);
    else gbd_extract(ctx, a, gbd_key_cols{}, T);
    return GX_OK;
}

/* the groups a finished table holds, on the host */
struct gbd_host_groups {
    std::vector<int64_t> k;
    std::vector<uint8_t> n;
    std::vector<unsigned long long> a;
    int64_t ng = 0;
};

/* the table's stat words (one sync), the overflow verdict, then its ng
 * compacted groups */
static gx_status gbd_fetch(gx_ctx *ctx, const gbd_args &a, gbd_table &T,
                           gbd_host_groups &H)
{
    hipStream_t s = ctx->stream;
    HIP_CHK(ctx, T.read_stats(s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    gx_status st = gbd_verdict(ctx, T);
    if (st != GX_OK) return st;
    const int64_t ng = T.ngroups();
    const int nk = a.nkeys, words = a.awords;
    H.ng = ng;
    H.k.resize((size_t) ng * nk);
    H.n.resize((size_t) ng * nk);
    H.a.resize((size_t) ng * words);
    if (ng)
    {
        if (nk)
        {
            HIP_CHK(ctx, hipMemcpyAsync(H.k.data(), T.okeys.p, H.k.size() * 8, hipMemcpyDeviceToHost, s));
            HIP_CHK(ctx, hipMemcpyAsync(H.n.data(), T.oknull.p, H.n.size(), hipMemcpyDeviceToHost, s));
        }
        HIP_CHK(ctx, hipMemcpyAsync(H.a.data(), T.oacc.p, H.a.size() * 8, hipMemcpyDeviceToHost, s));
        HIP_CHK(ctx, hipStreamSynchronize(s));
    }
    return GX_OK;
}

/* FINISH (pure host): sort the groups, un-image MIN / MAX, apply the NULL
 * rule, fill the result.  plain_one: a plain aggregate returns its one group
 * over no rows as well. */
static gx_status gbd_finish(const gbd_args &a, const gbd_host_groups &H,
                            bool plain_one, gx_gb_result *out)
{
    const int nk = a.nkeys, na = a.naggs, words = a.awords;
    const int64_t ng = H.ng;
    const int64_t nres = (nk == 0 && plain_one) ? 1 : ng;
    std::vector<int64_t> perm((size_t) ng);
    if (nk) gbd_sort_perm(H.k.data(), H.n.data(), ng, nk, perm.data());
    else for (int64_t i = 0; i < ng; i++) perm[i] = i;

    out->keys = (int64_t *) calloc(std::max<size_t>((size_t) nres * nk, 1), 8);
    out->key_null = (uint8_t *) calloc(std::max<size_t>((size_t) nres * nk, 1), 1);
    out->aggs = (uint64_t *) calloc(std::max<size_t>((size_t) nres * na, 1), 8);
    out->agg_null = (uint8_t *) calloc(std::max<size_t>((size_t) nres * na, 1), 1);
    if (!out->keys || !out->key_null || !out->aggs || !out->agg_null)
    {
        gx_gb_result_free(out);
        return GX_ERR_OOM;
    }
    out->ngroups = nres; out->nkeys = nk; out->naggs = na;
    for (int64_t gi = 0; gi < nres; gi++)
    {
        /* acc stays all-identity for the plain aggregate over no rows */
        static const unsigned long long zero[GBD_MAX_WORDS] = {};
        const unsigned long long *acc = ng ? &H.a[(size_t) perm[gi] * words] : zero;
        for (int k = 0; k < nk; k++)
        {
            out->keys[gi * nk + k] = H.k[(size_t) perm[gi] * nk + k];
            out->key_null[gi * nk + k] = H.n[(size_t) perm[gi] * nk + k];
        }
        for (int j = 0; j < na; j++)
        {
            const unsigned long long v = acc[a.aword[j]];
            uint64_t r = v;
            bool isnull = false;
            if (a.aop[j] >= GBD_SUM_INT)
            {
                isnull = acc[a.aword[j] + 1] == 0;
                switch (a.aop[j])
                {
                    case GBD_MAX_INT: r = v ^ (1ULL << 63); break;
                    case GBD_MIN_INT: r = ~v ^ (1ULL << 63); break;
                    case GBD_MAX_F64: r = gbd_f64_unimage(v); break;
                    case GBD_MIN_F64: r = gbd_f64_unimage(~v); break;
                    default: break;              /* sums: the word itself */
                }
            }
            out->aggs[gi * na + j] = isnull ? 0 : r;
            out->agg_null[gi * na + j] = (uint8_t) isnull;
        }
    }
    return GX_OK;
}

/* the argument checks every entry point starts with */
static gx_status gbd_check_call(gx_ctx *ctx, const gx_gb_desc *d, gx_gb_result *out)
{
    if (!ctx || !d || !out) return GX_ERR_INVALID;
    memset(out, 0, sizeof *out);
    if (!d->t) { set_err(ctx, "groupby_desc: no table%s", ""); return GX_ERR_INVALID; }
    return GX_OK;
}

/* the join entry points need their join descriptor */
static gx_status gbj_check_call(gx_ctx *ctx, const gx_gbj_ext *jext, gx_gb_result *out)
{
    if (!ctx || jext) return GX_OK;               /* no ctx: gbd_check_call answers */
    if (out) memset(out, 0, sizeof *out);
    set_err(ctx, "groupby_desc: no join descriptor%s", "");
    return GX_ERR_INVALID;
}

/* The one-stage plan: plan, bind, scan, extract, finish.  The public call
 * and the test entry run the same launches; they differ in `launch` alone.
 * stats (may be null) is the superset gx_gbj_stats for every family. */
static gx_status gbd_run(gx_ctx *ctx, const gx_gb_desc *d, const gx_gb_ext *ext,
                         const gx_gbj_ext *jext, const gbd_launch &launch,
                         gx_gb_result *out, gx_gbj_stats *stats)
{
    gx_status st = gbd_check_call(ctx, d, out);
    if (stats) memset(stats, 0, sizeof *stats);
    if (st != GX_OK) return st;
    gbd_call c(d, d->t, ext, jext);
    if ((st = gbd_plan(ctx, c)) != GX_OK) return st;
    gbd_table T;
    evholder e0, e1;
    HIP_CHK(ctx, e0.create()); HIP_CHK(ctx, e1.create());
    if ((st = gbd_scan_stage(ctx, c, T, launch, 0, e0, e1)) != GX_OK) return st;
    gbd_host_groups H;
    if ((st = gbd_fetch(ctx, c.a, T, H)) != GX_OK) return st;
    if ((st = gbd_finish(c.a, H, true, out)) != GX_OK) return st;
    if (stats)
    {
        float ms = 0;
        (void) hipEventElapsedTime(&ms, e0, e1);
        stats->ms_build = c.jp.ms_build;
        stats->ms_kernel = (double) ms;
        stats->rows_in = c.t->nrows;
        /* without a join every row the quals leave "reaches the probes" */
        stats->rows_probed = (int64_t) (c.jp.on ? T.hm[4] : T.hm[0]);
        stats->rows_pass = (int64_t) T.hm[0];
        stats->rows_lds = (int64_t) T.hm[1];
        stats->rows_global = (int64_t) (T.hm[0] - T.hm[1]);
        stats->groups = out->ngroups;
        for (int j = 0; j < c.jp.jx.njoins; j++) stats->dim_rows[j] = c.jp.dim_rows[j];
    }
    return GX_OK;
}

/* gbd_run for the join-less families, whose gx_gbd_stats is the part of
 * gx_gbj_stats that needs no join */
static gx_status gbd_run_nojoin(gx_ctx *ctx, const gx_gb_desc *d, const gx_gb_ext *ext,
                                const gbd_launch &launch, gx_gb_result *out,
                                gx_gbd_stats *stats)
{
    gx_gbj_stats js;
    gx_status st = gbd_run(ctx, d, ext, nullptr, launch, out, &js);
    if (stats)
        *stats = gx_gbd_stats{js.ms_kernel, js.rows_in, js.rows_pass, js.rows_lds,
                              js.rows_global, js.groups};
    return st;
}

extern "C" gx_status gx_groupby_desc(gx_ctx *ctx, const gx_gb_desc *d,
                                     gx_gb_result *out, gx_gbd_stats *stats)
{
    return gbd_run_nojoin(ctx, d, nullptr, GBD_PRODUCTION, out, stats);
}

extern "C" gx_status gx_test_groupby_desc(gx_ctx *ctx, const gx_gb_desc *d,
                                          int grid, int wide_rowid,
                                          gx_gb_result *out, gx_gbd_stats *stats)
{
    return gbd_run_nojoin(ctx, d, nullptr, gbd_test_launch(grid, wide_rowid), out, stats);
}

extern "C" gx_status gx_groupby_expr(gx_ctx *ctx, const gx_gb_desc *d,
                                     const gx_gb_ext *ext, gx_gb_result *out,
                                     gx_gbd_stats *stats)
{
    return gbd_run_nojoin(ctx, d, ext, GBD_PRODUCTION, out, stats);
}

extern "C" gx_status gx_test_groupby_expr(gx_ctx *ctx, const gx_gb_desc *d,
                                          const gx_gb_ext *ext, int grid,
                                          int wide_rowid, gx_gb_result *out,
                                          gx_gbd_stats *stats)
{
    return gbd_run_nojoin(ctx, d, ext, gbd_test_launch(grid, wide_rowid), out, stats);
}

extern "C" gx_status gx_groupby_join(gx_ctx *ctx, const gx_gb_desc *d,
                                     const gx_gbj_ext *jext, const gx_gb_ext *ext,
                                     gx_gb_result *out, gx_gbj_stats *stats)
{
    gx_status st = gbj_check_call(ctx, jext, out);
    if (st != GX_OK) return st;
    return gbd_run(ctx, d, ext, jext, GBD_PRODUCTION, out, stats);
}

extern "C" gx_status gx_test_groupby_join(gx_ctx *ctx, const gx_gb_desc *d,
                                          const gx_gbj_ext *jext,
                                          const gx_gb_ext *ext, int grid,
                                          int wide_rowid, gx_gb_result *out,
                                          gx_gbj_stats *stats)
{
    gx_status st = gbj_check_call(ctx, jext, out);
    if (st != GX_OK) return st;
    return gbd_run(ctx, d, ext, jext, gbd_test_launch(grid, wide_rowid), out, stats);
}

/* ---- two-stage descriptor GROUP BY: host side ----
 * (kernels: k_gbd_part_hist, k_gbd_part_emit, k_gbd_combine) */

/* bit k set: key column k is 8 bytes wide (hashint8; the others hashint4); a
 * dim-side key takes its width from the dimension's column */
static unsigned gbd_wide_mask(const gbd_call &c)
{
    unsigned m = 0;
    for (int k = 0; k < c.d->nkeys; k++)
        if (c.key_table(k)->cols[c.d->key_cols[k]].m.width == 8) m |= 1u << k;
    return m;
}

static int64_t gbd_wire_words(const gbd_args &a)
{
    return a.nkeys + (a.nkeys ? 1 : 0) + a.awords;
}

/* PARTITION stage over the compacted groups of a scan table, shared by the
 * two-stage call and its test seam: the buffers, the histogram launch, and
 * the emit from the send offsets the caller derives from the histogram(s).
 * Both walk at most T.bound groups.  Enqueue only. */
struct gbd_partition {
    devbuf hist, cur, dest, send;
    int nsegs = 0;
    unsigned long long *dhist() const { return hist.as<unsigned long long>(); }
};

static gx_status gbd_part_hist(gx_ctx *ctx, const gbd_call &c, const gbd_table &T,
                               int nsegs, gbd_partition &P)
{
    hipStream_t s = ctx->stream;
    P.nsegs = nsegs;
    HIP_CHK(ctx, P.hist.alloc((size_t) nsegs * 8));
    HIP_CHK(ctx, P.cur.alloc((size_t) nsegs * 8));
    HIP_CHK(ctx, P.dest.alloc((size_t) T.bound * 2));
    HIP_CHK(ctx, hipMemsetAsync(P.hist.p, 0, (size_t) nsegs * 8, s));
    const int grid = (int) std::min<int64_t>(GRID, (T.bound + TPB - 1) / TPB);
    hipLaunchKernelGGL(k_gbd_part_hist, dim3(grid), dim3(TPB), (size_t) nsegs * 4, s,
                       T.okeys.as<int64_t>(), T.oknull.as<uint8_t>(), T.stat(),
                       T.bound, c.a.nkeys, gbd_wide_mask(c), nsegs,
                       P.dest.as<uint16_t>(), P.dhist());
    return GX_OK;
}

/* send_off[r]: the wire row in P.send where destination r's rows start; e0
 * (optional) is recorded in front of the kernel */
static gx_status gbd_part_emit(gx_ctx *ctx, const gbd_call &c, const gbd_table &T,
                               gbd_partition &P, const unsigned long long *send_off,
                               uint64_t send_rows, hipEvent_t e0)
{
    hipStream_t s = ctx->stream;
    HIP_CHK(ctx, P.send.alloc(send_rows * (size_t) gbd_wire_words(c.a) * 8));
    HIP_CHK(ctx, hipMemcpyAsync(P.cur.p, send_off, (size_t) P.nsegs * 8,
                                hipMemcpyHostToDevice, s));
    if (e0) HIP_CHK(ctx, hipEventRecord(e0, s));
    const int grid = (int) std::min<int64_t>(GRID, (T.bound + TPB - 1) / TPB);
    hipLaunchKernelGGL(k_gbd_part_emit, dim3(grid), dim3(TPB), (size_t) P.nsegs * 12, s,
                       T.okeys.as<int64_t>(), T.oknull.as<uint8_t>(),
                       T.oacc.as<unsigned long long>(), T.stat(), T.bound, c.a.nkeys,
                       c.a.awords, P.nsegs, P.dest.as<uint16_t>(),
                       P.cur.as<unsigned long long>(),
                       P.send.as<unsigned long long>());
    return GX_OK;
}

/* COMBINE stage over n device-resident wire rows: budget, table, merge,
 * extract, finish.  ev_done (optional) is recorded after the last kernel. */
static gx_status gbd_combine(gx_ctx *ctx, const gbd_call &c, const void *drows,
                             int64_t n, bool force_wide, hipEvent_t ev_done,
                             gx_gb_result *out)
{
    const gbd_args &a = c.a;
    const int64_t max_groups = c.d->max_groups;
    const bool wide = gbd_wide(n, force_wide);
    /* the table is pow2 >= 2 * recv_rows; the groups are bounded by the
     * rows and by the planner's bound */
    gbd_table T;
    const int64_t rows_bound = std::max<int64_t>(n, 1);
    gx_status st = gbd_table_budget(ctx, a, rows_bound, wide, 0,
                                    "groupby_desc combine table");
    if (st != GX_OK) return st;
    if ((st = gbd_table_alloc(ctx, T, a, rows_bound, wide)) != GX_OK) return st;
    if (max_groups > 0) T.bound = std::min<int64_t>(T.bound, max_groups);
    const gbd_key_wire src{(const unsigned long long *) drows, gbd_wire_words(a)};
    if (n)
    {
        const int grid = (int) std::min<int64_t>(GRID, (n + TPB - 1) / TPB);
        by_width((int) T.sw, T.trow.p, [&](auto *rows) {
            hipLaunchKernelGGL(k_gbd_combine<std::decay_t<decltype(*rows)>>,
                               dim3(grid), dim3(TPB), 0, ctx->stream, a, src, n,
                               rows, T.tacc.as<unsigned long long>(),
                               T.tslots - 1, T.err());
        });
        gbd_extract(ctx, a, src, T);
    }
    if (ev_done) HIP_CHK(ctx, hipEventRecord(ev_done, ctx->stream));
    gbd_host_groups H;
    if ((st = gbd_fetch(ctx, a, T, H)) != GX_OK) return st;
    return gbd_finish(a, H, false, out);
}

static gx_status gbd_run_dist(gx_ctx *ctx, const gx_gb_desc *d, const gx_gb_ext *ext,
                              const gx_gbj_ext *jext, gx_gb_result *out,
                              gx_gb_stats *stats)
{
    gx_status st = gbd_check_call(ctx, d, out);
    if (stats) memset(stats, 0, sizeof *stats);
    if (st != GX_OK) return st;
    const gx_table *t = d->t;
    gx_gb_stats S{};
    S.rows_in = t->nrows;
    /* one-stage plan: nothing to redistribute on a single segment.
     * GX_FORCE_MOTION=1 routes a single-segment run through the full
     * exchange branch, as in gx_groupby_dist. */
    if (ctx->nsegs == 1 && env_int("GX_FORCE_MOTION", 0) == 0)
    {
        gx_gbj_stats one;
        st = gbd_run(ctx, d, ext, jext, GBD_PRODUCTION, out, &one);
        if (st != GX_OK) return st;
        S.ms_partial = one.ms_kernel;
        S.partial_groups = S.final_groups = out->ngroups;
        if (stats) *stats = S;
        return GX_OK;
    }
    gbd_call c(d, t, ext, jext);
    if ((st = gbd_plan(ctx, c)) != GX_OK) return st;
    if (!ctx->comm)
    { set_err(ctx, "nsegs>1 but gx_comm_init not called%s", ""); return GX_ERR_STATE; }
    const int n = ctx->nsegs;
    if (n > GB_MAX_SEGS)
    { set_err(ctx, "groupby_desc_dist: more segments than the partition kernels' LDS histogram holds%s", ""); return GX_ERR_INVALID; }

    hipStream_t s = ctx->stream;
    evholder ev[7];
    for (auto &e : ev) HIP_CHK(ctx, e.create());
    auto ms_between = [](hipEvent_t x, hipEvent_t y) {
        float ms = 0;
        (void) hipEventElapsedTime(&ms, x, y);
        return (double) ms;
    };

    /* stage 1: partial agg; the groups, their count and the error word stay
     * on the device */
    gbd_table T;
    const uint64_t side = (uint64_t) std::max<int64_t>(t->nrows, 1) * 2 +
                          (uint64_t) n * (n + 2) * 8;
    st = gbd_scan_stage(ctx, c, T, GBD_PRODUCTION, side, ev[0], nullptr);
    if (st != GX_OK) return st;
    HIP_CHK(ctx, hipEventRecord(ev[1], s));

    /* stage 2: partition.  The per-destination histogram goes straight into
     * the all-gather, so ONE host sync yields this rank's send layout, every
     * peer's counts, the partial group count and the error word. */
    gbd_partition P;
    devbuf all_b;
    HIP_CHK(ctx, all_b.alloc((size_t) n * n * 8));
    if ((st = gbd_part_hist(ctx, c, T, n, P)) != GX_OK) return st;
    HIP_CHK(ctx, hipEventRecord(ev[2], s));
    RCCL_CHK(ctx, ncclAllGather(P.dhist(), all_b.p, n, ncclUint64, ctx->comm, s));
    std::vector<unsigned long long> cnts_all((size_t) n * n);
    HIP_CHK(ctx, hipMemcpyAsync(cnts_all.data(), all_b.p, (size_t) n * n * 8,
                                hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, T.read_stats(s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    const gx_mlayout L = m_exchange_layout(cnts_all.data(), n, ctx->seg);
    const unsigned long long send_n = L.send_n, recv_n = L.recv_n;
    const size_t stride = (size_t) gbd_wire_words(c.a) * 8;
    st = hbm_budget_check(ctx, (send_n + recv_n) * stride + 64,
                          "groupby_desc exchange buffers");
    if (st != GX_OK) return st;
    devbuf recv_b;
    HIP_CHK(ctx, recv_b.alloc(recv_n * stride));
    st = gbd_part_emit(ctx, c, T, P, L.soff.data(), send_n, ev[3]);
    if (st != GX_OK) return st;
    HIP_CHK(ctx, hipEventRecord(ev[4], s));

    /* stage 3: exchange */
    st = m_exchange_payload(ctx, s, P.send.p, recv_b.p, L, stride);
    if (st != GX_OK) return st;
    HIP_CHK(ctx, hipEventRecord(ev[5], s));
    /* a failed partial stage sent no rows and is reported only now, after
     * this rank's sends and receives are enqueued, so the peers' matching
     * calls still complete */
    if ((st = gbd_verdict(ctx, T)) != GX_OK)
    {
        HIP_CHK(ctx, hipStreamSynchronize(s));
        return st;
    }

    /* stage 4: combine agg over the received partial states */
    st = gbd_combine(ctx, c, recv_b.p, (int64_t) recv_n, false, ev[6], out);
    if (st != GX_OK) return st;

    S.ms_partial = ms_between(ev[0], ev[1]);
    S.ms_partition = ms_between(ev[1], ev[2]) + ms_between(ev[3], ev[4]);
    S.ms_exchange = ms_between(ev[2], ev[3]) + ms_between(ev[4], ev[5]);
    S.ms_combine = ms_between(ev[5], ev[6]);
    S.partial_groups = S.sent_rows = (int64_t) send_n;
    S.recv_rows = (int64_t) recv_n;
    S.final_groups = out->ngroups;
    if (stats) *stats = S;
    return GX_OK;
}

extern "C" gx_status gx_groupby_desc_dist(gx_ctx *ctx, const gx_gb_desc *d,
                                          gx_gb_result *out, gx_gb_stats *stats)
{
    return gbd_run_dist(ctx, d, nullptr, nullptr, out, stats);
}

extern "C" gx_status gx_groupby_expr_dist(gx_ctx *ctx, const gx_gb_desc *d,
                                          const gx_gb_ext *ext, gx_gb_result *out,
                                          gx_gb_stats *stats)
{
    return gbd_run_dist(ctx, d, ext, nullptr, out, stats);
}

extern "C" gx_status gx_groupby_join_dist(gx_ctx *ctx, const gx_gb_desc *d,
                                          const gx_gbj_ext *jext,
                                          const gx_gb_ext *ext, gx_gb_result *out,
                                          gx_gb_stats *stats)
{
    gx_status st = gbj_check_call(ctx, jext, out);
    if (st != GX_OK) return st;
    return gbd_run_dist(ctx, d, ext, jext, out, stats);
}

/* Test ABI: partial agg + partition on one GPU for a given nsegs, through
 * the scan and partition stages of gbd_run_dist; jext: the join form */
static gx_status gbd_test_partial(gx_ctx *ctx, const gx_gb_desc *d,
                                  const gx_gbj_ext *jext, int nsegs,
                                  int64_t *out_counts, void *out_rows,
                                  int64_t cap_rows, int64_t *out_total)
{
    if (!ctx || !d || !out_counts || !out_total || cap_rows < 0 ||
        (cap_rows > 0 && !out_rows))
        return GX_ERR_INVALID;
    if (!d->t) { set_err(ctx, "groupby_desc: no table%s", ""); return GX_ERR_INVALID; }
    if (nsegs < 1 || nsegs > GB_MAX_SEGS)
        return gbd_invalid(ctx, "nsegs %ld outside 1..%ld", nsegs, GB_MAX_SEGS);
    gbd_call c(d, d->t, nullptr, jext);
    gx_status st = gbd_plan(ctx, c);
    if (st != GX_OK) return st;
    hipStream_t s = ctx->stream;
    gbd_table T;
    const uint64_t side = (uint64_t) std::max<int64_t>(d->t->nrows, 1) * 2 +
                          (uint64_t) nsegs * 16;
    st = gbd_scan_stage(ctx, c, T, GBD_PRODUCTION, side, nullptr, nullptr);
    if (st != GX_OK) return st;
    gbd_partition P;
    if ((st = gbd_part_hist(ctx, c, T, nsegs, P)) != GX_OK) return st;
    std::vector<unsigned long long> h(nsegs), off(nsegs + 1, 0);
    HIP_CHK(ctx, hipMemcpyAsync(h.data(), P.hist.p, (size_t) nsegs * 8,
                                hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, T.read_stats(s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    if ((st = gbd_verdict(ctx, T)) != GX_OK) return st;
    for (int i = 0; i < nsegs; i++) off[i + 1] = off[i] + h[i];
    const int64_t total = (int64_t) off[nsegs];
    if (total > cap_rows)
    { set_err(ctx, "gbd_partial: output capacity too small%s", ""); return GX_ERR_INVALID; }
    const size_t stride = (size_t) gbd_wire_words(c.a) * 8;
    st = hbm_budget_check(ctx, (uint64_t) total * stride + 64,
                          "groupby_desc exchange buffers");
    if (st != GX_OK) return st;
    st = gbd_part_emit(ctx, c, T, P, off.data(), (uint64_t) total, nullptr);
    if (st != GX_OK) return st;
    if (total)
        HIP_CHK(ctx, hipMemcpyAsync(out_rows, P.send.p, (size_t) total * stride,
                                    hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    for (int i = 0; i < nsegs; i++) out_counts[i] = (int64_t) h[i];
    *out_total = total;
    return GX_OK;
}

extern "C" gx_status gx_test_gbd_partial(gx_ctx *ctx, const gx_gb_desc *d,
                                         int nsegs, int64_t *out_counts,
                                         void *out_rows, int64_t cap_rows,
                                         int64_t *out_total)
{
    return gbd_test_partial(ctx, d, nullptr, nsegs, out_counts, out_rows, cap_rows,
                            out_total);
}

extern "C" gx_status gx_test_gbj_partial(gx_ctx *ctx, const gx_gb_desc *d,
                                         const gx_gbj_ext *jext, int nsegs,
                                         int64_t *out_counts, void *out_rows,
                                         int64_t cap_rows, int64_t *out_total)
{
    gx_status st = gbj_check_call(ctx, jext, nullptr);
    if (st != GX_OK) return st;
    return gbd_test_partial(ctx, d, jext, nsegs, out_counts, out_rows, cap_rows,
                            out_total);
}

/* Test ABI: the combine stage over host-supplied wire rows (the combine-only
 * plan: no table) */
static gx_status gbd_test_combine(gx_ctx *ctx, const gx_gb_desc *d, const void *rows,
                                  int64_t n, bool force_wide, gx_gb_result *out)
{
    gbd_call c(d, nullptr, nullptr, nullptr);
    gx_status st = gbd_plan(ctx, c);
    if (st != GX_OK) return st;
    const size_t stride = (size_t) gbd_wire_words(c.a) * 8;
    st = hbm_budget_check(ctx, (uint64_t) n * stride + 64,
                          "groupby_desc exchange buffers");
    if (st != GX_OK) return st;
    devbuf rows_b;
    HIP_CHK(ctx, rows_b.alloc((size_t) n * stride));
    if (n)
        HIP_CHK(ctx, hipMemcpyAsync(rows_b.p, rows, (size_t) n * stride,
                                    hipMemcpyHostToDevice, ctx->stream));
    return gbd_combine(ctx, c, rows_b.p, n, force_wide, nullptr, out);
}

extern "C" gx_status gx_test_gbd_combine(gx_ctx *ctx, const gx_gb_desc *d,
                                         const void *rows, int64_t n,
                                         int wide_rowid, gx_gb_result *out)
{
    if (!ctx || !d || !out || n < 0 || (n > 0 && !rows)) return GX_ERR_INVALID;
    memset(out, 0, sizeof *out);
    return gbd_test_combine(ctx, d, rows, n, wide_rowid != 0, out);
}


extern "C" int gx_selftest_gbd_route(const int64_t *keys, const uint8_t *key_null,
                                     const int32_t *widths, int nkeys, int64_t n,
                                     int nsegs, int32_t *out)
{
    if (n < 0 || nkeys < 0 || nkeys > GX_GB_MAX_KEYS || nsegs < 1 ||
        (n > 0 && !out) || (nkeys > 0 && !widths) ||
        (n > 0 && nkeys > 0 && (!keys || !key_null)))
        return 1;
    unsigned wide = 0;
    for (int k = 0; k < nkeys; k++)
    {
        if (!gbd_int_width(widths[k])) return 1;
        if (widths[k] == 8) wide |= 1u << k;
    }
    for (int64_t i = 0; i < n; i++)
    {
        int64_t kv[GX_GB_MAX_KEYS] = {0, 0, 0, 0};
        unsigned kn = 0;
        for (int k = 0; k < nkeys; k++)
        {
            const bool isnull = key_null[i * nkeys + k] != 0;
            kv[k] = isnull ? 0 : keys[i * nkeys + k];
            kn |= (unsigned) isnull << k;
        }
        out[i] = gbd_owner(kv, kn, wide, nkeys, nsegs);
    }
    return 0;
}

/* host restatements of the expression value and the float8 qual through
 * gbd_factor / gbd_fmul / gbd_fqual_pass, which the scan kernel calls */
extern "C" int gx_selftest_expr_eval(const gx_expr *ex, const double *vals,
                                     const uint8_t *isnull, int64_t n, int ncols,
                                     double *out, uint8_t *out_null)
{
    if (!ex || n < 0 || ncols < 1 || (n > 0 && (!vals || !out || !out_null)) ||
        ex->nfactors < 1 || ex->nfactors > GX_GB_MAX_FACTORS)
        return 1;
    for (int f = 0; f < ex->nfactors; f++)
        if (ex->f[f].col < 0 || ex->f[f].col >= ncols ||
            ex->f[f].form < GX_FACTOR_COL || ex->f[f].form > GX_FACTOR_ONE_PLUS)
            return 1;
    for (int64_t i = 0; i < n; i++)
    {
        const double *row = vals + i * ncols;
        bool isn = false;
        double v = gbd_factor(row[ex->f[0].col], ex->f[0].form);
        for (int f = 1; f < ex->nfactors; f++)
            v = gbd_fmul(v, gbd_factor(row[ex->f[f].col], ex->f[f].form));
        for (int f = 0; f < ex->nfactors; f++)
            isn = isn || (isnull && isnull[i * ncols + ex->f[f].col]);
        out[i] = isn ? 0.0 : v;
        out_null[i] = (uint8_t) isn;
    }
    return 0;
}

/* host restatement of the join table through gbj_home / gbj_next /
 * gbj_key_eq / gbj_probe, which k_gbj_build and the scan kernel call */
struct gbj_host_key {
    const int64_t *k;
    int64_t operator()(int64_t r) const { return k[r]; }
};

extern "C" int64_t gx_selftest_gbj_join(const int64_t *dim_keys, const uint8_t *dim_null,
                                        int64_t ndim, const int64_t *fact_keys,
                                        const uint8_t *fact_null, int64_t nfact,
                                        int64_t *out_row, int64_t *dup_key)
{
    if (ndim < 0 || nfact < 0 || ndim >= (int64_t) UINT32_MAX || !dup_key ||
        (ndim > 0 && !dim_keys) || (nfact > 0 && (!fact_keys || !out_row)))
        return -1;
    const uint64_t mask = gbj_slots(ndim) - 1;
    std::vector<uint32_t> slots(mask + 1, 0u);
    for (int64_t i = 0; i < ndim; i++)
    {
        if (dim_null && dim_null[i]) continue;
        uint64_t s = gbj_home(dim_keys[i], mask);
        for (;;)
        {
            const uint32_t cur = slots[s];
            if (cur == 0u) { slots[s] = (uint32_t) (i + 1); break; }
            if (gbj_key_eq(dim_keys[cur - 1], dim_keys[i]))
            { *dup_key = dim_keys[i]; return 1; }
            s = gbj_next(s, mask);
        }
    }
    for (int64_t f = 0; f < nfact; f++)
        out_row[f] = (fact_null && fact_null[f])
                         ? -1
                         : gbj_probe(slots.data(), mask, fact_keys[f],
                                     gbj_host_key{dim_keys});
    return 0;
}

extern "C" int64_t gx_selftest_gbj_slots(const int64_t *keys, int64_t n, int64_t ndim,
                                         uint32_t *out)
{
    if (n < 0 || ndim < 0 || ndim >= (int64_t) UINT32_MAX || (n > 0 && (!keys || !out)))
        return -1;
    const uint64_t mask = gbj_slots(ndim) - 1;
    for (int64_t i = 0; i < n; i++) out[i] = (uint32_t) gbj_home(keys[i], mask);
    return (int64_t) (mask + 1);
}

extern "C" int gx_selftest_fqual(int op, double x, double literal)
{
    if (op < 0 || op > 5) return -1;
    uint64_t xb, lb;
    memcpy(&xb, &x, 8);
    memcpy(&lb, &literal, 8);
    return gbd_fqual_pass(op, xb, gbd_fq_image(lb)) ? 1 : 0;
}

/* ABI self-description: struct sizes for cross-checking foreign-language
 * mirrors (ctypes tests; the PG extension's abi-check compiles against the
 * real header instead).  kind: 0 stats, 1 group, 2 kv_group, 3 desc,
 * 4 coldesc, 5 filter, 6 gb_stats, 7 test_tbl_layout, 8 gb_desc,
 * 9 gb_result, 10 agg, 11 gbd_stats, 13 gb_ext, 14 expr, 15 fqual,
 * 16 gb_join, 17 gbj_ext, 18 gbj_stats; 12 is unassigned and stays -1. */
extern "C" int64_t gx_abi_sizeof(int kind)
{
    switch (kind)
    {
        case 0: return (int64_t) sizeof(gx_q3_stats);
        case 1: return (int64_t) sizeof(gx_q3_group);
        case 2: return (int64_t) sizeof(gx_kv_group);
        case 3: return (int64_t) sizeof(gx_q3_desc);
        case 4: return (int64_t) sizeof(gx_coldesc);
        case 5: return (int64_t) sizeof(gx_filter);
        case 6: return (int64_t) sizeof(gx_gb_stats);
        case 7: return (int64_t) sizeof(gx_test_tbl_layout);
        case 8: return (int64_t) sizeof(gx_gb_desc);
        case 9: return (int64_t) sizeof(gx_gb_result);
        case 10: return (int64_t) sizeof(gx_agg);
        case 11: return (int64_t) sizeof(gx_gbd_stats);
        case 13: return (int64_t) sizeof(gx_gb_ext);
        case 14: return (int64_t) sizeof(gx_expr);
        case 15: return (int64_t) sizeof(gx_fqual);
        case 16: return (int64_t) sizeof(gx_gb_join);
        case 17: return (int64_t) sizeof(gx_gbj_ext);
        case 18: return (int64_t) sizeof(gx_gbj_stats);
        default: return -1;
    }
}

/* ---- test-only entry points of the Motion stages ----
 * Each one drives a stage of the nsegs>1 branch of gx_q3_run through the
 * shared seams above (same launches, dispatch and layout rules) for ANY
 * nsegs on one GPU; the exchange between stages is done by the caller on
 * the host with the counts returned here.  The RCCL calls themselves, the
 * cross-rank agreement on the bloom size and on dim_state, and multi-GPU
 * timing stay outside their reach. */

static bool test_is_pow2(uint64_t v) { return v && !(v & (v - 1)); }

static bool test_cols_are(const gx_table *t, std::initializer_list<int> widths)
{
    if (!t || t->cols.size() != widths.size()) return false;
    size_t i = 0;
    for (int w : widths)
    {
        if (t->cols[i].format != 0 || t->cols[i].m.width != w) return false;
        i++;
    }
    return true;
}

/* Motion 1 for one rank: orders cols [okey i64, ocust i64, odate i32,
 * oprio i32]; host_bloom_all (optional) holds nsegs * bwords words. */
static gx_status test_m1_impl(gx_ctx *ctx, gx_table *orders, gx_filter f,
                              int nsegs, int dim_join,
                              const uint64_t *host_bloom_all, uint64_t bwords,
                              int64_t *out_counts, gx_ord_row *out_rows,
                              int64_t cap, int64_t *out_total)
{
    if (!ctx || !out_counts || !out_total || nsegs < 1 || cap < 0 ||
        (cap > 0 && !out_rows) || !test_cols_are(orders, {8, 8, 4, 4}))
        return GX_ERR_INVALID;
    if (f.col < 2 || f.col > 3)
    {
        set_err(ctx, "test_m1: the mid filter reads an i32 column (2 or 3)%s", "");
        return GX_ERR_INVALID;
    }
    if (!gx_fold_filter(4, &f.op, &f.literal))
    {
        set_err(ctx, "test_m1: filter op must be in 0..5%s", "");
        return GX_ERR_INVALID;
    }
    if (host_bloom_all && (!test_is_pow2(bwords) || bwords < 4096))
    {
        set_err(ctx, "test_m1: bwords must be a power of two >= 4096%s", "");
        return GX_ERR_INVALID;
    }
    hipStream_t s = ctx->stream;
    /* as in gx_q3_run, the filter column is also the carried first attribute */
    const gx_col &ok = orders->cols[0], &oc = orders->cols[1],
                 &od = orders->cols[f.col], &op = orders->cols[3];
    devbuf dhist_b, dcur_b, dsend_b, dbloom_b;
    const unsigned long long *bloom_all = nullptr;
    uint64_t bwmask = 0;
    if (host_bloom_all)
    {
        HIP_CHK(ctx, dbloom_b.alloc((uint64_t) nsegs * bwords * 8));
        HIP_CHK(ctx, hipMemcpyAsync(dbloom_b.p, host_bloom_all,
                                    (uint64_t) nsegs * bwords * 8,
                                    hipMemcpyHostToDevice, s));
        bloom_all = dbloom_b.as<unsigned long long>();
        bwmask = bwords - 1;
    }
    HIP_CHK(ctx, dhist_b.alloc(nsegs * 8));
    HIP_CHK(ctx, dcur_b.alloc(nsegs * 8));
    unsigned long long *dhist = dhist_b.as<unsigned long long>();
    unsigned long long *dcur = dcur_b.as<unsigned long long>();
    HIP_CHK(ctx, hipMemsetAsync(dhist, 0, nsegs * 8, s));
    m1_launch_hist(s, od, oc, orders->dvmap, f.op, (int32_t) f.literal, nsegs,
                   dim_join, bloom_all, bwmask, dhist);
    std::vector<unsigned long long> h(nsegs);
    HIP_CHK(ctx, hipMemcpyAsync(h.data(), dhist, nsegs * 8, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    std::vector<unsigned long long> off(nsegs + 1, 0);
    for (int i = 0; i < nsegs; i++) off[i + 1] = off[i] + h[i];
    int64_t total = (int64_t) off[nsegs];
    if (total > cap)
    {
        set_err(ctx, "test_m1: output capacity too small%s", "");
        return GX_ERR_INVALID;
    }
    HIP_CHK(ctx, dsend_b.alloc(std::max<int64_t>(total, 1) * sizeof(gx_ord_row)));
    gx_ord_row *dsend = dsend_b.as<gx_ord_row>();
    HIP_CHK(ctx, hipMemcpyAsync(dcur, off.data(), nsegs * 8, hipMemcpyHostToDevice, s));
    m1_launch_emit(s, ok, oc, od, op, orders->dvmap, f.op, (int32_t) f.literal,
                   nsegs, dim_join, bloom_all, bwmask, dcur, dsend);
    if (total)
        HIP_CHK(ctx, hipMemcpyAsync(out_rows, dsend, total * sizeof(gx_ord_row),
                                    hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    for (int i = 0; i < nsegs; i++) out_counts[i] = (int64_t) h[i];
    *out_total = total;
    return GX_OK;
}

/* one rank's dim membership as the Motion path holds it: the production
 * q3_dimset, counted, sized and built by q3_dim_size_build without the
 * bitmap.  bwords == 0 takes this rank's own bloom size; a caller-chosen one
 * stands in for the max-over-ranks agreement.  q3_dim_size_build agrees
 * across ranks on a multi-rank communicator, which one rank calling a test
 * entry point alone would wait on for ever: such a context is refused. */
static gx_status test_build_dim(gx_ctx *ctx, gx_table *customer, int32_t op,
                                int64_t literal, uint64_t bwords,
                                q3_dimset &ds, int64_t *nsel = nullptr)
{
    if (!ctx || !test_cols_are(customer, {8, 1})) return GX_ERR_INVALID;
    if (ctx->nsegs > 1 && ctx->comm)
    {
        set_err(ctx, "test_dim: not on a multi-rank communicator%s", "");
        return GX_ERR_STATE;
    }
    if (!gx_fold_filter(1, &op, &literal))
    {
        set_err(ctx, "test_dim: filter op must be in 0..5%s", "");
        return GX_ERR_INVALID;
    }
    if (bwords && (!test_is_pow2(bwords) || bwords < 4096))
    {
        set_err(ctx, "test_dim: bwords must be a power of two >= 4096%s", "");
        return GX_ERR_INVALID;
    }
    q3_scratch sc;
    HIP_CHK(ctx, sc.ensure());
    int state = 0;
    return q3_dim_size_build(ctx, ctx->stream, sc,
                             {customer->cols[0], customer->cols[1], nullptr, op,
                              literal, customer->dvmap},
                             false, false, bwords, ds, &state, nsel);
}

extern "C" gx_status gx_test_dim(gx_ctx *ctx, gx_table *customer, int32_t op,
                                 int64_t literal, uint64_t bwords,
                                 uint64_t *out_bloom, int64_t *out_nsel,
                                 int32_t *out_set_width)
{
    if (!ctx || !out_bloom || !bwords) return GX_ERR_INVALID;
    q3_dimset ds;
    gx_status st = test_build_dim(ctx, customer, op, literal, bwords, ds, out_nsel);
    if (st != GX_OK) return st;
    HIP_CHK(ctx, hipMemcpyAsync(out_bloom, ds.bloom.p, bwords * 8,
                                hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHK(ctx, hipStreamSynchronize(ctx->stream));
    HIP_CHK(ctx, hipGetLastError());
    if (out_set_width) *out_set_width = ds.width;
    return GX_OK;
}

/* Motion 2 for one rank: its dim set against the rows it received */
static_assert(sizeof(gx_qual_row_abi) == sizeof(gx_qual_row), "qual row abi");
static gx_status test_m2_impl(gx_ctx *ctx, gx_table *customer, int32_t op,
                              int64_t literal, uint64_t bwords,
                              const gx_ord_row *host_rows, int64_t n,
                              int dim_join, int nsegs, int64_t *out_counts,
                              gx_qual_row_abi *out_rows, int64_t cap,
                              int64_t *out_total, int32_t *out_set_width)
{
    if (!ctx || !out_counts || !out_total || nsegs < 1 || n < 0 || cap < 0 ||
        (n > 0 && !host_rows) || (cap > 0 && !out_rows))
        return GX_ERR_INVALID;
    hipStream_t s = ctx->stream;
    q3_dimset ds;
    gx_status st = test_build_dim(ctx, customer, op, literal, bwords, ds);
    if (st != GX_OK) return st;
    devbuf rows_b, hist_b, cur_b, send_b;
    HIP_CHK(ctx, rows_b.alloc(std::max<int64_t>(n, 1) * sizeof(gx_ord_row)));
    if (n)
        HIP_CHK(ctx, hipMemcpyAsync(rows_b.p, host_rows, n * sizeof(gx_ord_row),
                                    hipMemcpyHostToDevice, s));
    HIP_CHK(ctx, hist_b.alloc(nsegs * 8));
    HIP_CHK(ctx, cur_b.alloc(nsegs * 8));
    HIP_CHK(ctx, hipMemsetAsync(hist_b.p, 0, nsegs * 8, s));
    m2_launch_hist(s, rows_b.as<gx_ord_row>(), n, ds, dim_join, nsegs,
                   hist_b.as<unsigned long long>());
    std::vector<unsigned long long> h(nsegs);
    HIP_CHK(ctx, hipMemcpyAsync(h.data(), hist_b.p, nsegs * 8, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    std::vector<unsigned long long> off(nsegs + 1, 0);
    for (int i = 0; i < nsegs; i++) off[i + 1] = off[i] + h[i];
    int64_t total = (int64_t) off[nsegs];
    if (total > cap)
    {
        set_err(ctx, "test_m2: output capacity too small%s", "");
        return GX_ERR_INVALID;
    }
    HIP_CHK(ctx, send_b.alloc(std::max<int64_t>(total, 1) * sizeof(gx_qual_row)));
    HIP_CHK(ctx, hipMemcpyAsync(cur_b.p, off.data(), nsegs * 8, hipMemcpyHostToDevice, s));
    m2_launch_emit(s, rows_b.as<gx_ord_row>(), n, ds, dim_join, nsegs,
                   cur_b.as<unsigned long long>(), send_b.as<gx_qual_row>());
    if (total)
        HIP_CHK(ctx, hipMemcpyAsync(out_rows, send_b.p, total * sizeof(gx_qual_row),
                                    hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    for (int i = 0; i < nsegs; i++) out_counts[i] = (int64_t) h[i];
    *out_total = total;
    if (out_set_width) *out_set_width = ds.width;
    return GX_OK;
}

static void test_fill_layout(gx_test_tbl_layout *o, const gx_tbl_layout &L,
                             unsigned long long kmin, unsigned long long kmax)
{
    o->key_width = L.key_width;
    o->interpolated = L.smap.scale < 0.0 ? 0 : 1;
    o->slots = L.slots;
    o->kmin = L.smap.kmin;
    o->scale = L.smap.scale;
    o->slot_kmin = L.smap.slot0(kmin);
    o->slot_kmax = L.smap.slot0(kmax);
}

/* Motion 3 for one rank: table from the received qualifying rows (layout,
 * key width and build launch as gx_q3_run picks them, nsegs from ctx), then
 * probe + aggregate its lineitem shard [lkey i64, price f64, disc f64,
 * shipdate i32] through the production probe dispatch, visimap honoured. */
static gx_status test_m3_impl(gx_ctx *ctx, const gx_qual_row_abi *host_rows,
                              int64_t n, gx_table *lineitem, int32_t fop,
                              int64_t flit, gx_q3_group **out,
                              int64_t *ngroups, gx_test_tbl_layout *lay)
{
    if (!ctx || !out || !ngroups || n < 0 || (n > 0 && !host_rows) ||
        !test_cols_are(lineitem, {8, 8, 8, 4}))
        return GX_ERR_INVALID;
    if (!gx_fold_filter(4, &fop, &flit))
    {
        set_err(ctx, "test_m3: filter op must be in 0..5%s", "");
        return GX_ERR_INVALID;
    }
    hipStream_t s = ctx->stream;
    devbuf rows_b;
    q3_scratch sc;
    q3_hashtbl t;
    q3_results r;
    HIP_CHK(ctx, sc.ensure());
    HIP_CHK(ctx, rows_b.alloc(n * sizeof(gx_qual_row)));
    if (n)
        HIP_CHK(ctx, hipMemcpyAsync(rows_b.p, host_rows, n * sizeof(gx_qual_row),
                                    hipMemcpyHostToDevice, s));
    q3_keystats ks;
    gx_tbl_layout TL;
    {
        gx_status lst = m3_recv_layout(ctx, s, sc, rows_b.as<gx_qual_row>(), n,
                                       ks, TL);
        if (lst != GX_OK) return lst;
    }
    if (lay) test_fill_layout(lay, TL, ks.kmin, ks.kmax);
    t.width = TL.key_width;
    t.smap = TL.smap;
    {
        gx_status ast = q3_alloc_hash(ctx, t, TL.slots);
        if (ast != GX_OK) return ast;
    }
    HIP_CHK(ctx, hipMemsetAsync(t.keys.p, 0, t.slots() * t.width, s));
    m3_launch_build(s, rows_b.as<gx_qual_row>(), n, t);
    const gx_col &lk = lineitem->cols[0], &lp = lineitem->cols[1],
                 &ld = lineitem->cols[2], &ls = lineitem->cols[3];
    unsigned long long *dhits = sc.word(q3_scratch::HITS),
                       *dcount = sc.word(q3_scratch::GROUPS);
    HIP_CHK(ctx, hipMemsetAsync(dhits, 0, 8, s));
    q3_launch_probe(s, lk, lp, ld, ls, lineitem->dvmap, fop, (int32_t) flit,
                    t, dhits, false, q3_unmatched{});
    HIP_CHK(ctx, r.alloc(std::max<int64_t>(n, 1)));
    HIP_CHK(ctx, hipMemsetAsync(dcount, 0, 8, s));
    {
        gx_status est = q3_launch_extract(
            ctx, s, t.width, t.keys.p, t.attrs.as<gx_attrpair>(),
            t.aggs.as<gx_aggslot>(), t.slots(), 0, r, dcount);
        if (est != GX_OK) return est;
    }
    unsigned long long ng = 0;
    HIP_CHK(ctx, hipMemcpyAsync(&ng, dcount, 8, hipMemcpyDeviceToHost, s));
    HIP_CHK(ctx, hipStreamSynchronize(s));
    HIP_CHK(ctx, hipGetLastError());
    int64_t m = (int64_t) ng;
    std::vector<int64_t> okey(m), cnt(m);
    std::vector<int32_t> odate(m), oprio(m);
    std::vector<double> rev(m);
    if (m)
    {
        HIP_CHK(ctx, hipMemcpy(okey.data(), r.okey.p, m * 8, hipMemcpyDeviceToHost));
        HIP_CHK(ctx, hipMemcpy(odate.data(), r.odate.p, m * 4, hipMemcpyDeviceToHost));
        HIP_CHK(ctx, hipMemcpy(oprio.data(), r.oprio.p, m * 4, hipMemcpyDeviceToHost));
        HIP_CHK(ctx, hipMemcpy(rev.data(), r.rev.p, m * 8, hipMemcpyDeviceToHost));
        HIP_CHK(ctx, hipMemcpy(cnt.data(), r.cnt.p, m * 8, hipMemcpyDeviceToHost));
    }
    std::vector<int64_t> idx(m);
    for (int64_t i = 0; i < m; i++) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return okey[a] < okey[b]; });
    /* zeroed: key_is_null / attrs_null / _pad are read by the callers */
    gx_q3_group *g = (gx_q3_group *) calloc(std::max<int64_t>(m, 1), sizeof(gx_q3_group));
    if (!g) return GX_ERR_OOM;
    for (int64_t i = 0; i < m; i++)
    {
        g[i].l_orderkey = okey[idx[i]];
        g[i].o_orderdate = odate[idx[i]];
        g[i].o_shippriority = oprio[idx[i]];
        g[i].revenue = rev[idx[i]];
        g[i].revenue_num = 0;
        g[i].nitems = cnt[idx[i]];
    }
    *out = g;
    *ngroups = m;
    return GX_OK;
}

extern "C" gx_status gx_test_m1(gx_ctx *ctx, gx_table *orders,
                                const gx_filter *mid_filter, int nsegs,
                                int dim_join, const uint64_t *bloom_all,
                                uint64_t bwords, int64_t *out_counts,
                                gx_ord_row *out_rows, int64_t cap,
                                int64_t *out_total)
{
    if (!mid_filter) return GX_ERR_INVALID;
    return test_m1_impl(ctx, orders, *mid_filter, nsegs, dim_join, bloom_all,
                        bwords, out_counts, out_rows, cap, out_total);
}

extern "C" gx_status gx_test_m2(gx_ctx *ctx, gx_table *customer, int32_t op,
                                int64_t literal, uint64_t bwords,
                                const gx_ord_row *rows, int64_t n,
                                int dim_join, int nsegs, int64_t *out_counts,
                                gx_qual_row_abi *out_rows, int64_t cap,
                                int64_t *out_total, int32_t *out_set_width)
{
    return test_m2_impl(ctx, customer, op, literal, bwords, rows, n, dim_join,
                        nsegs, out_counts, out_rows, cap, out_total,
                        out_set_width);
}

extern "C" gx_status gx_test_m3(gx_ctx *ctx, const gx_qual_row_abi *rows,
                                int64_t n, gx_table *lineitem, int32_t op,
                                int64_t literal, gx_q3_group **out,
                                int64_t *ngroups, gx_test_tbl_layout *layout)
{
    return test_m3_impl(ctx, rows, n, lineitem, op, literal, out, ngroups, layout);
}

/* the three original entry points: the Q3 constants on the same stages.
 * orders filter o_orderdate < cutoff, no prefilter */
extern "C" gx_status gx_test_motion1(gx_ctx *ctx, gx_table *orders,
                                     int32_t cutoff, int nsegs,
                                     int64_t *out_counts /* nsegs */,
                                     gx_ord_row *out_rows /* cap */,
                                     int64_t cap, int64_t *out_total)
{
    gx_filter f = {2, 0, cutoff};
    return test_m1_impl(ctx, orders, f, nsegs, 0, nullptr, 0, out_counts,
                        out_rows, cap, out_total);
}

/* dim filter c_mktsegment == 0, semi join, this rank's own bloom size */
extern "C" gx_status gx_test_qual(gx_ctx *ctx, gx_table *customer,
                                  const gx_ord_row *host_rows, int64_t n,
                                  int nsegs, int64_t *out_counts,
                                  gx_qual_row_abi *out_rows, int64_t cap,
                                  int64_t *out_total)
{
    return test_m2_impl(ctx, customer, 2, 0, 0, host_rows, n, 0, nsegs,
                        out_counts, out_rows, cap, out_total, nullptr);
}

/* fact filter l_shipdate > cutoff.  Caller frees *out with gx_free. */
extern "C" gx_status gx_test_q3_from_qual(gx_ctx *ctx,
                                          const gx_qual_row_abi *host_rows,
                                          int64_t n, gx_table *lineitem,
                                          int32_t cutoff, gx_q3_group **out,
                                          int64_t *ngroups)
{
    return test_m3_impl(ctx, host_rows, n, lineitem, 1, cutoff, out, ngroups,
                        nullptr);
}

/* The two pure host helpers of the Motion path on caller-supplied inputs
 * (callable without a GPU).  cnts_all (n×n, optional): this rank's send /
 * receive counts (n each) and offsets (n + 1 each).  layout (optional): the
 * table layout for qual keys in [kmin,kmax].  Returns 0, or 1 for bad
 * arguments. */
extern "C" int gx_selftest_motion_layout(const uint64_t *cnts_all, int n, int seg,
                                         uint64_t *scnt, uint64_t *soff,
                                         uint64_t *rcnt, uint64_t *roff,
                                         int64_t qual, uint64_t kmin,
                                         uint64_t kmax, int nsegs, int tf_pct,
                                         gx_test_tbl_layout *layout)
{
    if (cnts_all)
    {
        if (n < 1 || seg < 0 || seg >= n || !scnt || !soff || !rcnt || !roff)
            return 1;
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "u64");
        gx_mlayout L = m_exchange_layout((const unsigned long long *) cnts_all,
                                         n, seg);
        for (int i = 0; i < n; i++) { scnt[i] = L.scnt[i]; rcnt[i] = L.rcnt[i]; }
        for (int i = 0; i <= n; i++) { soff[i] = L.soff[i]; roff[i] = L.roff[i]; }
    }
    if (layout)
    {
        if (qual < 0 || nsegs < 1 || tf_pct < 0) return 1;
        test_fill_layout(layout,
                         q3_table_layout(qual, kmin, kmax, nsegs, tf_pct),
                         kmin, kmax);
    }
    return 0;
}

/* sizing's bound on the LEFT-OUTER unmatched groups (q3_unmatched_bound) on
 * caller-supplied column stats; callable without a GPU */
extern "C" uint64_t gx_selftest_unmatched_bound(int64_t nrows, uint64_t lmin,
                                                uint64_t lmax)
{
    return q3_unmatched_bound(nrows, lmin, lmax);
}

/* sizing's rank-form rule (q3_rank_eligible) on caller-supplied key stats,
 * and the keys one block of the prefix-popcount scan covers; callable without
 * a GPU */
extern "C" int gx_selftest_rank_eligible(int64_t qual, uint64_t kmin,
                                         uint64_t kmax, int enabled)
{
    return q3_rank_eligible(qual, kmin, kmax, enabled) ? 1 : 0;
}

extern "C" int64_t gx_rank_scan_block_keys(void)
{
    return (int64_t) GX_RANK_SCAN_WORDS * 64;
}

/* the orders stage's form rule (q3_orders_staged), its threshold, the staged
 * form's mark grid and the records of one wave's LDS segment; callable
 * without a GPU */
extern "C" int gx_selftest_orders_staged(int64_t qual, int64_t nrows, int env)
{
    return q3_orders_staged(qual, nrows, env) ? 1 : 0;
}

extern "C" int64_t gx_orders_stage_rule_k(void)
{
    return GX_ORDERS_STAGE_K;
}

extern "C" int64_t gx_selftest_orders_stage_grid(int64_t qual, int64_t nrows)
{
    return q3_stage_grid(qual, nrows);
}

extern "C" int64_t gx_orders_stage_wave_records(void)
{
    return GX_STAGE_WAVE_RECS;
}

/* bind's per-block routing of the fused RLE probe (parse_block_dir +
 * rle_block_class) over a host stream of 8-byte datums; callable without a
 * GPU.  Writes the gx_rle_class of the first min(blocks, cap) blocks and
 * returns the number of blocks, or -1 for a stream bind would refuse. */
extern "C" int64_t gx_selftest_rle_block_class(const uint8_t *stream,
                                               int64_t nbytes, int32_t *cls,
                                               int64_t cap)
{
    if (!stream || nbytes < 0 || (cap > 0 && !cls)) return -1;
    std::vector<gx_blockref> dir;
    int64_t rows = 0;
    if (parse_block_dir(stream, nbytes, dir, &rows) != GX_OK) return -1;
    for (int64_t b = 0; b < (int64_t) dir.size() && b < cap; b++)
        cls[b] = dir[b].cls;
    return (int64_t) dir.size();
}

/* RCCL linkage self-check: init a 1-rank communicator and run one
 * allgather — proves the collective stack works on this box without
 * needing multiple GPUs (the multi-rank path differs only in peer count). */
extern "C" int gx_selftest_rccl(int device)
{
    if (hipSetDevice(device) != hipSuccess) return 1;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return 2;
    ncclComm_t comm;
    if (ncclCommInitRank(&comm, 1, id, 0) != ncclSuccess) return 3;
    devbuf a, b;
    if (a.alloc(8) != hipSuccess || b.alloc(8) != hipSuccess) return 4;
    unsigned long long v = 0xC0FFEE;
    (void) hipMemcpy(a.p, &v, 8, hipMemcpyHostToDevice);
    hipStream_t s;
    if (hipStreamCreate(&s) != hipSuccess) return 4;
    int rc = 0;
    if (ncclAllGather(a.p, b.p, 1, ncclUint64, comm, s) != ncclSuccess)
        rc = 5;
    (void) hipStreamSynchronize(s);
    unsigned long long w = 0;
    (void) hipMemcpy(&w, b.p, 8, hipMemcpyDeviceToHost);
    if (rc == 0 && w != v) rc = 6;
    (void) hipStreamDestroy(s);
    ncclCommDestroy(comm);
    return rc;
}

/* host-side self-test of the division-free row→block addressing (callable
 * without a GPU; exercised by tests/test_abi_cpu.py) */
extern "C" int gx_selftest_addressing(void)
{
    for (int width : {1, 4, 8})
    {
        gx_colmeta m{};
        m.width = width;
        m.rpb = gx_aocs_rows_per_block(width, 32768);
        m.full_block_len = gx_aocs_block_len(width, m.rpb);
        gx_colmeta_finish(&m);
        /* boundaries of the first 4M blocks plus large sampled rows */
        for (int64_t b = 0; b < 4 * 1000 * 1000; b += 997)
            for (int64_t r : {(int64_t) 0, (int64_t) (m.rpb - 1)})
            {
                int64_t row = b * (int64_t) m.rpb + r;
                int64_t bb = (int64_t) gx_mulhi64((uint64_t) row, m.magic);
                if (bb != b) return 1;
            }
        for (int64_t row = 1; row < (int64_t) 1e15; row = row * 3 + 7)
            if ((int64_t) gx_mulhi64((uint64_t) row, m.magic) != row / m.rpb)
                return 2;
    }
    return 0;
}
