"""Float64 checker of the ScanNet box kernels (csrc/scanbox.hip): convex hull by monotone chain, the rectangle of every hull edge,
containment, the margin between the best and the second-best edge.  Plain numpy -- no GPU, no reference import.

The rectangle of an edge is the reference's bounding_area: unit vector u of the edge, o = (-u_y, u_x), extents of all hull vertices
along u and o, area = length_parallel * length_orthogonal, centre (min_p + len_p / 2, min_o + len_o / 2) taken back to xy with
angle = atan2(u_y, u_x).  Edges run counter-clockwise from the lexicographically smallest hull vertex; the minimum is the first one.
"""
import numpy as np


def hull_ccw(xy):
    """Counter-clockwise convex hull of float64 [n, 2] points from the lexicographically smallest vertex; duplicates and collinear
    points dropped (cross <= 0 pops).  [0, 2] when fewer than three vertices remain."""
    p = np.unique(np.asarray(xy, dtype=np.float64), axis=0)        # sorted by (x, y)
    if len(p) < 3:
        return np.zeros((0, 2))
    pts = p.tolist()

    def half(seq):
        h = []
        for c in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (c[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (c[0] - h[-2][0]) <= 0.0:
                h.pop()
            h.append(c)
        return h
    lower, upper = half(pts), half(pts[::-1])
    h = np.array(lower[:-1] + upper[:-1])
    return h if len(h) >= 3 else np.zeros((0, 2))


def edge_rectangles(h, chunk=256):
    """Per hull edge: dict of float64 [H] arrays area, length_parallel, length_orthogonal, cx, cy, angle.  Edges are processed `chunk` at
    a time, so only a chunk x H block of projections exists at once."""
    H = len(h)
    out = {k: np.empty(H) for k in ("area", "length_parallel", "length_orthogonal", "cx", "cy", "angle")}
    nxt = np.roll(h, -1, axis=0)
    for a in range(0, H, chunk):
        p0, p1 = h[a:a + chunk], nxt[a:a + chunk]
        dis = np.sqrt((p0[:, 0] - p1[:, 0]) ** 2 + (p0[:, 1] - p1[:, 1]) ** 2)
        ux, uy = (p1[:, 0] - p0[:, 0]) / dis, (p1[:, 1] - p0[:, 1]) / dis
        dp = ux[:, None] * h[None, :, 0] + uy[:, None] * h[None, :, 1]
        do = (-uy)[:, None] * h[None, :, 0] + ux[:, None] * h[None, :, 1]
        min_p, min_o = dp.min(axis=1), do.min(axis=1)
        len_p, len_o = dp.max(axis=1) - min_p, do.max(axis=1) - min_o
        ang = np.arctan2(uy, ux)
        c0, c1 = min_p + len_p / 2, min_o + len_o / 2
        s = slice(a, a + len(p0))
        out["area"][s], out["length_parallel"][s], out["length_orthogonal"][s], out["angle"][s] = len_p * len_o, len_p, len_o, ang
        out["cx"][s] = c0 * np.cos(ang) + c1 * np.cos(ang + np.pi / 2)
        out["cy"][s] = c0 * np.sin(ang) + c1 * np.sin(ang + np.pi / 2)
    return out


def margin(areas):
    """(second-smallest edge-rectangle area / smallest) - 1; exact ties give 0."""
    a = np.sort(np.asarray(areas))
    return float(a[1] / a[0] - 1.0)


def min_rectangle(xy):
    """The first edge of minimum area: dict with edge, area, length_parallel, length_orthogonal, cx, cy, angle, margin, hull, second
    (the index of the second-best edge)."""
    h = hull_ccw(xy)
    if len(h) < 3:
        raise ValueError("degenerate point set")
    r = edge_rectangles(h)
    e = int(np.argmin(r["area"]))        # first minimum
    order = np.argsort(r["area"], kind="stable")
    out = {k: float(v[e]) for k, v in r.items()}
    out.update(edge=e, margin=margin(r["area"]), hull=h, second=int(order[1]), rects=r)
    return out


def outside_distance(xy, cx, cy, len_p, len_o, angle):
    """How far the worst point of xy lies outside the rectangle (<= 0 when all are inside), along the rectangle's own axes."""
    xy = np.asarray(xy, dtype=np.float64)
    u = np.array([np.cos(angle), np.sin(angle)])
    o = np.array([-np.sin(angle), np.cos(angle)])
    d = xy - np.array([cx, cy])
    return float(max((np.abs(d @ u) - len_p / 2).max(), (np.abs(d @ o) - len_o / 2).max()))


def parallel_error(angle, h):
    """Smallest angle (radians) between a side of the rectangle at `angle` and any hull edge."""
    e = np.roll(h, -1, axis=0) - h
    d = np.mod(np.arctan2(e[:, 1], e[:, 0]) - angle, np.pi / 2)
    return float(np.minimum(d, np.pi / 2 - d).min())
