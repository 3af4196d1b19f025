"""numpy restatement of the hull x box penetration of the cube kernels (robot_geometry="hull"): Minkowski Portal Refinement after Snethen, "XenoCollide"
(Game Programming Gems 7), with MuJoCo 2.1's defaults (mjOption.mpr_tolerance 1e-6, mpr_iterations 50).  Written from the published description, not from the HIP
routine; the checker for tests/test_hull_box*.py (the C oracle does not know the pair).

The Minkowski difference is M = hull - box.  The portal is a triangle of support points of M (v1, v2, v3) seen from an interior point v0 (hull vertex centroid minus
box centre); the ray from v0 through the origin passes through the portal.  Refinement pushes the portal outward along its normal until a new support point is no
more than the tolerance beyond it.  The final portal's normal is the contact normal (from the hull into the box); the extent of M along it -- the overlap of the
two shapes' projections on it -- is the depth.
"""
import numpy as np

TOL = 1e-6          # mjOption.mpr_tolerance
MAX_ITER = 50       # mjOption.mpr_iterations
EPS = np.finfo(float).eps

SEPARATED, PENETRATING, NOT_CONVERGED = 0, 1, 2


def support_hull(Vw, d):
    """world hull vertex with the largest projection on d (the lowest index among equals)"""
    return Vw[int(np.argmax(Vw @ d))]


def support_box(c, R, h, d):
    """box corner farthest along d: the sign pattern of d in the box frame (a zero component takes +h)"""
    loc = R.T @ d
    return c + R @ np.where(loc >= 0, h, -h)


class _Pt:
    """a point of M with the two shape points it came from"""
    __slots__ = ("v", "a", "b")

    def __init__(self, a, b):
        self.a, self.b = np.asarray(a, float), np.asarray(b, float)
        self.v = self.a - self.b


def _unit(x):
    n = np.sqrt(x @ x)
    return x / n if n > 0 else x


def mpr_penetration(V_body, R, p, box_c, box_R, box_h):
    """hull (body-frame vertices V_body at pose R, p) against the box (centre, rotation, half extents).
    -> (status, depth, normal[3], pos[3]); status SEPARATED / PENETRATING / NOT_CONVERGED"""
    V_body = np.asarray(V_body, float)
    R, p, box_c, box_R, box_h = (np.asarray(x, float) for x in (R, p, box_c, box_R, box_h))
    Vw = V_body @ R.T + p
    centroid = R @ (V_body.sum(axis=0) / len(V_body)) + p
    zero3 = np.zeros(3)

    def sup(d):
        return _Pt(support_hull(Vw, d), support_box(box_c, box_R, box_h, -d))

    none = (SEPARATED, 0.0, zero3, zero3)
    # -- find a portal the origin ray passes through
    o = _Pt(centroid, box_c)
    if not o.v.any():
        o.v = o.v + np.array([10 * EPS, 0.0, 0.0])
    d = _unit(-o.v)
    s1 = sup(d)
    if s1.v @ d < EPS:
        return none
    d = np.cross(o.v, s1.v)
    if d @ d < EPS:
        if not s1.v.any():
            return none
        L = np.sqrt(s1.v @ s1.v)
        return PENETRATING, L, s1.v / L, 0.5 * (s1.a + s1.b)
    d = _unit(d)
    s2 = sup(d)
    if s2.v @ d < EPS:
        return none
    d = _unit(np.cross(s1.v - o.v, s2.v - o.v))
    if d @ o.v > 0:
        s1, s2 = s2, s1
        d = -d
    portal = None
    for _ in range(MAX_ITER):
        s3 = sup(d)
        if s3.v @ d < EPS:
            return none
        t = np.cross(s1.v, s3.v) @ o.v
        if t < 0 and abs(t) >= EPS:
            s2 = s3
        else:
            t = np.cross(s3.v, s2.v) @ o.v
            if t < 0 and abs(t) >= EPS:
                s1 = s3
            else:
                portal = [o, s1, s2, s3]
                break
        d = _unit(np.cross(s1.v - o.v, s2.v - o.v))
    if portal is None:
        return NOT_CONVERGED, 0.0, zero3, zero3

    def normal():
        return _unit(np.cross(portal[2].v - portal[1].v, portal[3].v - portal[1].v))

    def close_enough(s4, d):
        return min(s4.v @ d - portal[k].v @ d for k in (1, 2, 3)) <= TOL

    def expand(s4):
        c = np.cross(s4.v, portal[0].v)
        if portal[1].v @ c > 0:
            k = 1 if portal[2].v @ c > 0 else 3
        else:
            k = 2 if portal[3].v @ c > 0 else 1
        portal[k] = s4

    # -- refine until the origin is on the inner side of the portal
    for _ in range(MAX_ITER):
        d = normal()
        if d @ portal[1].v > -EPS:
            break
        s4 = sup(d)
        if s4.v @ d < EPS or close_enough(s4, d):
            return none
        expand(s4)
    else:
        return NOT_CONVERGED, 0.0, zero3, zero3
    # -- push the portal to the boundary of M
    for _ in range(MAX_ITER):
        d = normal()
        s4 = sup(d)
        if close_enough(s4, d):
            break
        expand(s4)
    else:
        return NOT_CONVERGED, 0.0, zero3, zero3
    # depth: the extent of M along the final portal's normal -- how far the hull must move back along it to clear the box (the overlap of the two shapes'
    # projections on d); within the tolerance of the portal plane's distance from the origin
    depth = float(s4.v @ d)
    if not depth > 0:
        return none
    # -- contact position: the origin's barycentric weights in the tetrahedron (v0 .. v3) -- signed volumes -- on each shape's points, then their midpoint
    P = [s.v for s in portal]
    w = np.array([np.linalg.det(np.array([P[1], P[2], P[3]])), -np.linalg.det(np.array([P[0], P[2], P[3]])),
                  np.linalg.det(np.array([P[0], P[1], P[3]])), -np.linalg.det(np.array([P[0], P[1], P[2]]))])
    if w.sum() < EPS:   # a flat tetrahedron: the origin's projection along the portal normal in the triangle (v1, v2, v3)
        w = np.array([0.0, np.cross(P[2], P[3]) @ d, np.cross(P[3], P[1]) @ d, np.cross(P[1], P[2]) @ d])
    w = w / w.sum()
    pos = 0.5 * sum(w[k] * (portal[k].a + portal[k].b) for k in range(4))
    return PENETRATING, depth, d, pos


def support_value_hull(V_body, R, p, n):
    """max over the hull of n . x (world)"""
    return float(np.max((np.asarray(V_body) @ R.T + p) @ n))


def support_value_box(c, Rb, h, n):
    """min over the box of n . x (world)"""
    return float(c @ n - np.abs(Rb.T @ n) @ h)
