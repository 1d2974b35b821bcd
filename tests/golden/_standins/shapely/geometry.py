"""``Point`` and two-point ``LineString`` with ``intersection``, ``is_empty`` and ``distance``, by definition and in exact
rational arithmetic: the intersection of two segments is the set of points that lie on both -- empty, one point, or for
collinear overlap a segment -- computed on ``fractions.Fraction`` images of the float64 coordinates (exact), so there is no
tolerance anywhere; a distance is the exact rational squared distance, square-rooted and rounded to float64 once.  A zero-length
line is the point it degenerates to.  Anything else (longer lines, other geometry types, other methods) raises."""
from fractions import Fraction
from math import isqrt


def _pt(c):
    c = list(c)
    if len(c) < 2:
        raise ValueError("a coordinate needs x and y")
    return (Fraction(float(c[0])), Fraction(float(c[1])))          # (z, if any, is ignored: planar predicates, as shapely's)


def _sqrt(q):
    """float64 nearest to sqrt(q) for a Fraction q >= 0 (the integer root carries 200 bits more than a double)."""
    if q == 0:
        return 0.0
    n, d = q.numerator * q.denominator, q.denominator              # sqrt(p / d) = sqrt(p d) / d
    k = max(0, 200 - n.bit_length() // 2)
    return float(Fraction(isqrt(n << (2 * k)), d << k))


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1])


def _cross(a, b):
    return a[0] * b[1] - a[1] * b[0]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1]


def _along(p, t, d):
    return (p[0] + t * d[0], p[1] + t * d[1])


class _Geometry:
    pts = ()

    @property
    def is_empty(self):
        return len(self.pts) == 0

    def _segment(self):
        if not self.pts:
            raise ValueError("empty geometry")
        return self.pts[0], self.pts[-1]

    def distance(self, other):
        if not isinstance(other, Point):
            raise NotImplementedError("distance to a Point only")
        a, b = self._segment()
        x = other.pts[0]
        ab = _sub(b, a)
        L = _dot(ab, ab)
        t = Fraction(0) if L == 0 else min(Fraction(1), max(Fraction(0), _dot(_sub(x, a), ab) / L))
        d = _sub(_along(a, t, ab), x)
        return _sqrt(_dot(d, d))

    def intersection(self, other):
        p0, p1 = self._segment()
        q0, q1 = other._segment()
        r, s, qp = _sub(p1, p0), _sub(q1, q0), _sub(q0, p0)
        den = _cross(r, s)
        if den != 0:                                               # the two lines cross in exactly one point
            t, u = _cross(qp, s) / den, _cross(qp, r) / den
            return _make([_along(p0, t, r)]) if 0 <= t <= 1 and 0 <= u <= 1 else _make([])
        rr, ss = _dot(r, r), _dot(s, s)
        if rr == 0 and ss == 0:
            return _make([p0]) if p0 == q0 else _make([])
        if rr == 0:                                                # a point against a segment
            w = _dot(_sub(p0, q0), s)
            return _make([p0]) if _cross(_sub(p0, q0), s) == 0 and 0 <= w <= ss else _make([])
        if _cross(qp, r) != 0:                                     # parallel, distinct lines
            return _make([])
        a, b = sorted((_dot(qp, r) / rr, _dot(_sub(q1, p0), r) / rr))       # q's extent in p's parameter
        lo, hi = max(a, Fraction(0)), min(b, Fraction(1))
        if lo > hi:
            return _make([])
        return _make([_along(p0, lo, r)] if lo == hi else [_along(p0, lo, r), _along(p0, hi, r)])


def _make(pts):
    g = _Geometry()
    g.pts = tuple(pts)
    return g


class Point(_Geometry):
    def __init__(self, *coords):
        self.pts = (_pt(coords[0] if len(coords) == 1 else coords),)

    @property
    def x(self):
        return float(self.pts[0][0])

    @property
    def y(self):
        return float(self.pts[0][1])


class LineString(_Geometry):
    def __init__(self, coords):
        coords = list(coords)
        if len(coords) != 2:
            raise NotImplementedError("two-point lines only")
        self.pts = (_pt(coords[0]), _pt(coords[1]))
