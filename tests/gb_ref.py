"""The one helper module of the descriptor GROUP BY tests (groupby_desc, its
two-stage form, the float8 expressions and the join): binding, the numpy
group-by reference with expression columns and float8 quals, result
comparison, the forced-Motion call, and a numpy inner join that materialises
the joined columns for the reference.

cols everywhere: a list of (values, nulls or None), one pair per column."""
import os

import numpy as np

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1


def stream(orc, vals, nulls=None, rle=False):
    """one column as a bind() spec: format 0 when NOT NULL and bindable so
    (widths 1/4/8), Orig-with-NULLs (format 1) otherwise; rle: an RLE block
    stream (format 1, NOT NULL)"""
    vals = np.ascontiguousarray(vals)
    n, w = len(vals), vals.itemsize
    if n == 0:
        return (b"", w, 0, 1)
    if rle:
        assert nulls is None
        return (orc.aocs_encode_rle(vals), w, n, 1)
    if nulls is None and w != 2:
        return (orc.aocs_encode(vals), w, n, 0)
    if nulls is None:
        nulls = np.zeros(n, np.bool_)
    return (orc.aocs_encode_orig_nulls(vals, nulls), w, n, 1)


def bind(ctx, orc, cols, hidden=None, rle=(), empty_hidden=False):
    """rle: column indexes bound as RLE; hidden: the visimap's deleted rows,
    an empty one set only with empty_hidden"""
    t = ctx.bind([stream(orc, v, nl, rle=i in rle)
                  for i, (v, nl) in enumerate(cols)])
    if hidden is not None and (empty_hidden or len(hidden)):
        t.set_visimap(hidden)
    return t


def nulls(col):
    v, nl = col
    return np.zeros(len(v), np.bool_) if nl is None else np.asarray(nl, np.bool_)


def expr_col(cols, factors):
    """(values, nulls) of ((f0 * f1) * f2), one numpy double operation a step;
    NULL where any factor's column is"""
    v, nl = None, np.zeros(len(cols[0][0]), np.bool_)
    with np.errstate(all="ignore"):
        for f in factors:
            form, c = f if isinstance(f, tuple) else ("", f)
            x = cols[c][0].astype(np.float64)
            x = {"": x, "1-": 1.0 - x, "1+": 1.0 + x}[form]
            v = x if v is None else v * x
            nl = nl | nulls(cols[c])
    return v, nl


def f8cmp(x, lit):
    """float8_cmp_internal(x, lit) per element: NaNs equal, above everything"""
    xn = np.isnan(x)
    with np.errstate(invalid="ignore"):
        c = np.where(x > lit, 1, np.where(x < lit, -1, 0))
    return np.where(xn, 0, -1) if np.isnan(lit) else np.where(xn, 1, c)


_OPS = {"<": lambda c: c < 0, ">": lambda c: c > 0, "==": lambda c: c == 0,
        "!=": lambda c: c != 0, "<=": lambda c: c <= 0, ">=": lambda c: c >= 0}


def fq_mask(cols, fquals):
    """rows the AND-ed float8 quals pass; a NULL input fails the row"""
    m = np.ones(len(cols[0][0]), np.bool_)
    for c, op, lit in fquals:
        m &= ~nulls(cols[c]) & _OPS[op](f8cmp(cols[c][0].astype(np.float64), lit))
    return m


def ref(cols, keys, aggs, mask=None):
    """numpy GROUP BY over the rows of mask.  keys = column indexes; aggs =
    (fn, col[, is_f64]) as for Context.groupby_expr, col a list of factors
    for an expression aggregate (float8).  Returns the dict shape
    groupby_desc returns: groups in np.unique's order over the (null, value)
    fields, column by column = lexicographic, NULLS LAST."""
    n = len(cols[0][0]) if cols else 0
    rows = np.arange(n) if mask is None else np.nonzero(mask)[0]
    nk = len(keys)
    if nk:
        rec = np.zeros(len(rows), [(f"{'nv'[f]}{k}", (np.uint8, np.int64)[f])
                                   for k in range(nk) for f in (0, 1)])
        for k, c in enumerate(keys):
            nl = nulls(cols[c])[rows]
            rec[f"n{k}"] = nl
            rec[f"v{k}"] = np.where(nl, 0, cols[c][0][rows].astype(np.int64))
        uniq, inv = np.unique(rec, return_inverse=True)
        inv = inv.reshape(-1)
        ng = len(uniq)
        kout = np.stack([uniq[f"v{k}"] for k in range(nk)], axis=1).reshape(ng, nk)
        knull = np.stack([uniq[f"n{k}"] for k in range(nk)], axis=1).reshape(ng, nk)
    else:
        ng, inv = 1, np.zeros(len(rows), np.int64)
        kout, knull = np.zeros((1, 0), np.int64), np.zeros((1, 0), np.uint8)
    acols, anull = [], np.zeros((ng, len(aggs)), np.bool_)
    for j, spec in enumerate(aggs):
        fn, c = spec[0], spec[1]
        f64 = len(spec) > 2 and spec[2]
        if fn == "count*":
            acols.append(np.bincount(inv, minlength=ng).astype(np.int64))
            continue
        if isinstance(c, (list, tuple)):
            col, f64 = expr_col(cols, c), True
        else:
            col = cols[c]
        ok = ~nulls(col)[rows]
        g, v = inv[ok], col[0][rows][ok]
        cnt = np.bincount(g, minlength=ng).astype(np.int64)
        if fn == "count":
            acols.append(cnt)
            continue
        anull[:, j] = cnt == 0
        if fn == "sum":
            out = np.zeros(ng, np.float64 if f64 else np.int64)
            np.add.at(out, g, v.astype(out.dtype))
        elif not f64:
            v = v.astype(np.int64)
            out = np.full(ng, INT64_MIN if fn == "max" else INT64_MAX, np.int64)
            (np.maximum if fn == "max" else np.minimum).at(out, g, v)
        else:
            # float8_cmp_internal's order: every NaN equal, above +inf
            isnan = np.isnan(v)
            nnan = np.bincount(g[isnan], minlength=ng)
            out = np.full(ng, -np.inf if fn == "max" else np.inf)
            (np.maximum if fn == "max" else np.minimum).at(out, g[~isnan], v[~isnan])
            if fn == "max":
                out[nnan > 0] = np.nan
            else:
                out[(nnan > 0) & (nnan == cnt)] = np.nan
        out[cnt == 0] = 0
        acols.append(out)
    return {"ngroups": ng, "keys": kout, "key_null": knull.astype(np.bool_),
            "aggs": acols, "agg_null": anull}


def same(a, b, float_tol=None):
    """equality of two results: keys, NULL flags, dtypes and values (NaN equal
    to NaN, -0 to +0); float8 values that are neither are compared bit for
    bit.  float_tol compares the float64 aggregates with rtol = atol =
    float_tol instead."""
    assert a["ngroups"] == b["ngroups"]
    np.testing.assert_array_equal(a["keys"], b["keys"])
    np.testing.assert_array_equal(a["key_null"], b["key_null"])
    np.testing.assert_array_equal(a["agg_null"], b["agg_null"])
    assert len(a["aggs"]) == len(b["aggs"])
    for x, y in zip(a["aggs"], b["aggs"]):
        assert x.dtype == y.dtype
        if float_tol is not None and x.dtype == np.float64:
            np.testing.assert_allclose(x, y, rtol=float_tol, atol=float_tol)
            continue
        np.testing.assert_array_equal(x, y)
        if x.dtype == np.float64:
            m = ~np.isnan(y) & (y != 0)
            np.testing.assert_array_equal(x.view(np.uint64)[m], y.view(np.uint64)[m])


def take(res, m):
    """the groups of a result selected by a boolean mask, order kept"""
    return {"ngroups": int(m.sum()), "keys": res["keys"][m],
            "key_null": res["key_null"][m], "aggs": [a[m] for a in res["aggs"]],
            "agg_null": res["agg_null"][m]}


def sorted_nulls_last(res):
    k, nl = res["keys"], res["key_null"]
    cols = []
    for c in range(k.shape[1] - 1, -1, -1):
        cols += [k[:, c], nl[:, c]]
    return (np.lexsort(cols) == np.arange(len(k))).all() if cols else True


def forced(ctx, call):
    """call() through the FULL exchange branch of a _dist form by
    self-exchange"""
    ctx.comm_init(ctx.comm_unique_id())
    os.environ["GX_FORCE_MOTION"] = "1"
    try:
        return call()
    finally:
        del os.environ["GX_FORCE_MOTION"]


def match(fact_col, dim_col, dim_live):
    """inner equi-join of one fact column with one dimension key column by a
    dict over the participating dimension rows (dim_live, NULL keys never):
    the matched dimension row of every fact row, or -1.  Both sides compare as
    Python ints, i.e. after sign extension."""
    dv, dn = dim_col[0], nulls(dim_col)
    table = {}
    for r in np.nonzero(np.asarray(dim_live, np.bool_) & ~dn)[0]:
        k = int(dv[r])
        assert k not in table, f"duplicate participating dimension key {k}"
        table[k] = int(r)
    fv, fn = fact_col[0], nulls(fact_col)
    return np.array([-1 if fn[i] else table.get(int(fv[i]), -1)
                     for i in range(len(fv))], np.int64)


def joined(fact_cols, dims, matches):
    """(cols, mask): the fact columns followed by every dimension's columns
    gathered at the matched rows, and the mask of the rows every join matched.
    Column c of dims[j] is column offset(j) + c of the result."""
    n = len(fact_cols[0][0])
    ok = np.ones(n, np.bool_)
    cols = list(fact_cols)
    for dcols, m in zip(dims, matches):
        ok &= m >= 0
        at = np.where(m >= 0, m, 0)
        for v, nl in dcols:
            if len(v) == 0:
                cols.append((np.zeros(n, v.dtype), np.ones(n, np.bool_)))
            else:
                cols.append((v[at], nulls((v, nl))[at]))
    return cols, ok
