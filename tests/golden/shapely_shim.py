"""A stand-in for the part of ``shapely.geometry`` that kitti_utils.get_iou3d uses, for the fixture generators (which must not rest on
an installed shapely): ``Polygon(coords)`` with ``.is_valid``, ``.area`` and ``.intersection(other).area`` for CONVEX quadrilaterals, in
f64.  In the spirit of numba_shim.py; it holds no reference text.  ``install()`` registers it as ``shapely.geometry``.

The intersection is a Sutherland-Hodgman clip (the ring of ``self`` cut by the edges of ``other``); areas are shoelace sums.
"""
import sys
import types


def _area2(ring):
    s = 0.0
    for i in range(len(ring)):
        x0, y0 = ring[i]
        x1, y1 = ring[(i + 1) % len(ring)]
        s += x0 * y1 - x1 * y0
    return s


class Polygon:
    def __init__(self, coords):
        self.ring = [(float(p[0]), float(p[1])) for p in coords]

    @property
    def area(self):
        return 0.5 * abs(_area2(self.ring)) if len(self.ring) >= 3 else 0.0

    @property
    def is_valid(self):
        """convex, with area"""
        n = len(self.ring)
        if n < 3 or self.area == 0.0:
            return False
        sign = 0
        for i in range(n):
            (x0, y0), (x1, y1), (x2, y2) = self.ring[i], self.ring[(i + 1) % n], self.ring[(i + 2) % n]
            c = (x1 - x0) * (y2 - y1) - (y1 - y0) * (x2 - x1)
            if c != 0.0:
                if sign and (c > 0) != (sign > 0):
                    return False
                sign = 1 if c > 0 else -1
        return True

    def intersection(self, other):
        out = list(self.ring)
        orient = 1.0 if _area2(other.ring) >= 0 else -1.0
        m = len(other.ring)
        for e in range(m):
            if not out:
                break
            (ax, ay), (bx, by) = other.ring[e], other.ring[(e + 1) % m]
            src, out = out, []
            for i in range(len(src)):
                (cx, cy), (nx, ny) = src[i], src[(i + 1) % len(src)]
                dc = orient * ((bx - ax) * (cy - ay) - (by - ay) * (cx - ax))
                dn = orient * ((bx - ax) * (ny - ay) - (by - ay) * (nx - ax))
                if dc >= 0:
                    out.append((cx, cy))
                if (dc >= 0) != (dn >= 0):
                    t = dc / (dc - dn)
                    out.append((cx + t * (nx - cx), cy + t * (ny - cy)))
        return Polygon(out)


def install():
    if "shapely.geometry" in sys.modules:
        return
    pkg, geo = types.ModuleType("shapely"), types.ModuleType("shapely.geometry")
    geo.Polygon = Polygon
    pkg.geometry = geo
    sys.modules["shapely"], sys.modules["shapely.geometry"] = pkg, geo
