"""Yardstick of the image-box tests: the projection formula (projection.py's docstring) evaluated beyond float64, and the
error unit the comparisons are made in.

L is the formula in np.longdouble where that type carries more than 52 mantissa bits (x86: 63), otherwise in `decimal`
at 40 digits on a subset.  The unit of an element is 2^-52 * A, A its condition magnitude: the sum of the absolute values
of every product and addend that enters the numerator, over |w'|, plus |result| (projection.box3d_to_bbox(...,
return_parts=True) computes it per projected point).  A bbox element is a min / max over eight points, and min / max
move by no more than the largest move of an argument, so its A is the largest of the eight.

K_REF is the worst |reference - L| / unit over the fixture's regular and behind-camera cases (the reference's own arrays in
tests/golden/ref_bbox.npz: numpy float64, einsum, a BLAS `@`, glibc's sin / cos), measured by test_projection_host.py and
asserted there not to exceed the constant.  The restatement and both GPU entry points must stay within
K = 4 * max(K_REF, 1) units of L: the factor 4 covers a device sincos of up to 2 ulp where glibc's stays below 1, and one
differently rounded operation per product.
"""
import decimal

import numpy as np

K_REF = 0.61         # measured: 0.608 on the projected points, 0.428 on the boxes (the restatement: 0.608 / 0.509)
K = 4 * max(K_REF, 1)
UNIT = 2.0 ** -52

CORNER_UNITS = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]], np.float64)
HAVE_LONGDOUBLE = np.finfo(np.longdouble).nmant > 52


def _formula(b, P, T, sin, cos):
    """points [N,8,2] of boxes b [N,7] with per-box matrices P [N,4,4] in number type T."""
    n = len(b)
    pts = np.empty((n, 8, 2), dtype=object if T is not np.longdouble else np.longdouble)
    half, one = T(0.5), T(1)
    for i in range(n):
        v = [T(float(x)) for x in b[i]]                         # exact in either type
        M = [[T(float(x)) for x in row] for row in P[i]]
        s, c = sin(v[6]), cos(v[6])
        for k in range(8):
            ux, uy, uz = (T(int(u)) for u in CORNER_UNITS[k])
            x, y, z = v[3] * (ux - half), v[4] * (uy - one), v[5] * (uz - half)
            X, Y, Z = x * c + z * s + v[0], y + v[1], -x * s + z * c + v[2]
            w = X * M[2][0] + Y * M[2][1] + Z * M[2][2]
            pts[i, k, 0] = (X * M[0][0] + Y * M[0][1] + Z * M[0][2]) / w
            pts[i, k, 1] = (X * M[1][0] + Y * M[1][1] + Z * M[1][2]) / w
    return pts


def _dec_sincos():
    def series(x, first, start):
        term, total, n = first, first, start
        while abs(term) > decimal.Decimal(10) ** -45:
            term = -term * x * x / ((n + 1) * (n + 2))
            total += term
            n += 2
        return total
    return (lambda x: series(x, x, 1)), (lambda x: series(x, decimal.Decimal(1), 0))


def exact_points(boxes, p2_per_box):
    """-> (points [N,8,2] as float-convertible high-precision numbers, rows used).  longdouble: every row; decimal: the
    first 20 rows."""
    b, P = np.asarray(boxes, np.float64), np.asarray(p2_per_box, np.float64)
    if HAVE_LONGDOUBLE:
        return _formula(b, P, np.longdouble, np.sin, np.cos), np.arange(len(b))
    rows = np.arange(min(20, len(b)))
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        sin, cos = _dec_sincos()
        return _formula(b[rows], P[rows], decimal.Decimal, sin, cos), rows


def point_ratios(got_points, exact, cond):
    """|got - L| / (2^-52 A), elementwise [N,8,2]."""
    got = np.asarray(got_points, np.float64)
    if exact.dtype == object:
        diff = np.array([[[abs(float(decimal.Decimal(float(got[i, k, j])) - exact[i, k, j])) for j in range(2)]
                          for k in range(8)] for i in range(len(got))])
    else:
        diff = np.abs(got.astype(np.longdouble) - exact).astype(np.float64)
    return diff / (UNIT * cond)


def bbox_ratios(got_bbox, exact, cond):
    """|got - L's bbox| / (2^-52 max A over the eight corners), elementwise [N,4]."""
    got = np.asarray(got_bbox, np.float64)
    lo, hi = exact.min(axis=1), exact.max(axis=1)              # [N,2] each; exact numbers compare exactly
    Lb = np.concatenate([lo, hi], axis=1)
    A = np.concatenate([cond.max(axis=1), cond.max(axis=1)], axis=1)
    if exact.dtype == object:
        diff = np.array([[abs(float(decimal.Decimal(float(got[i, j])) - Lb[i, j])) for j in range(4)] for i in range(len(got))])
    else:
        diff = np.abs(got.astype(np.longdouble) - Lb).astype(np.float64)
    return diff / (UNIT * A)


def number_class(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    a = np.asarray(a, np.float64)
    return np.where(np.isnan(a), 1, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 3, 0)))


def fixture(g):
    """(boxes, counts, p2, kind, frame of every box, p2 per box) of tests/golden/ref_bbox.npz."""
    counts = g["counts"]
    frame = np.repeat(np.arange(len(counts)), counts)
    return g["boxes"], counts, g["p2"], g["kind"], frame, g["p2"][frame]
