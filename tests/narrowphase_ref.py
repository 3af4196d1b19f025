"""What the primitive narrowphase is held to: an exact geometric reference of segment - segment, segment - box, the capsule - box stretch
and box - box, and a checker that judges an output of seg_seg / seg_box / cap_box_two / box_box2 by what it must satisfy, not by equality with one chosen witness.

Written from the geometry, in numpy: float64, or np.longdouble with dt=LD.  It reads neither the oracle nor the kernels; what it knows of the code are the
thresholds the code documents (EPS, BB_TIE, the 1.05 edge / face factor, 1 mm, 1e-9, r), which is where its bounds widen and where a case counts as a knife edge.

Conventions: a rotation is a unit quaternion (w, x, y, z); its matrix has the body axes as columns.  A query is a row of NP_QDIM doubles, an output a row of
NP_ODIM doubles, laid out as hrg_debug_narrowphase lays them out (include/hrgym.h)."""
import numpy as np

F64, LD = np.float64, np.longdouble
SEGSEG, SEGBOX, CAPBOX, BOXBOX = 0, 1, 2, 3
KINDS = {"seg_seg": SEGSEG, "seg_box": SEGBOX, "cap_box_two": CAPBOX, "box_box2": BOXBOX}
NP_QDIM, NP_ODIM = 24, 32
TOL = 1e-12            # metres: every comparison that is not a derived band (module docstring of tests/test_narrowphase.py says where it comes from)
EPS = 1e-12            # seg_seg: squared lengths and sin^2 below it are "zero"
BB_TIE = 1e-9          # box_box2: a later axis / candidate has to win by this much
EDGE_FACTOR = 1.05     # box_box2: an edge axis is taken only when clearly less penetrating
STRETCH_MIN = 1e-3     # cap_box_two: the two ends are at least 1 mm apart
TOUCH_MIN = 1e-9       # cap_box_two: an end whose axis point lies on the box gives no normal
N_SAMPLE = 20001       # capsule - box stretch: samples of the axis


# ------------------------------------------------------------------------------------------------ small vector tools (np.linalg has no long double)
def _v(x, dt):
    return np.asarray(x, dtype=dt)


def dot(a, b):
    return (a * b).sum(-1)


def norm(a):
    return np.sqrt(dot(a, a))


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def quat_mat(q, dt=F64):
    w, x, y, z = _v(q, dt)
    one, two = dt(1), dt(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=dt)


def unpack(kind, q, dt=F64):
    """a query row -> the routine's arguments, named"""
    q = _v(q, dt)
    if kind == SEGSEG:
        return dict(p1=q[0:3], q1=q[3:6], p2=q[6:9], q2=q[9:12])
    if kind in (SEGBOX, CAPBOX):
        return dict(p1=q[0:3], p2=q[3:6], c=q[6:9], quat=q[9:13], hb=q[13:16], r=q[16])
    return dict(pa=q[0:3], qa=q[3:7], ha=q[7:10], pb=q[10:13], qb=q[13:17], hb=q[17:20])


# ------------------------------------------------------------------------------------------------ segment - segment
def seg_seg_ref(p1, q1, p2, q2, dt=F64):
    """exact minimum over the KKT candidates: the interior stationary point (independent directions), the four end-point projections"""
    p1, q1, p2, q2 = (_v(x, dt) for x in (p1, q1, p2, q2))
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, b, c, f = dot(d1, d1), dot(d2, d2), dot(d1, d2), dot(d1, r), dot(d2, r)
    den = a * e - b * b
    cand = []
    if a > 0 and e > 0 and den > 0:
        s, t = (b * f - c * e) / den, (a * f - b * c) / den
        if 0 <= s <= 1 and 0 <= t <= 1:
            cand.append((s, t))
    for s in (dt(0), dt(1)):   # an end of the first segment against the second
        x = p1 + s * d1
        cand.append((s, np.clip(dot(x - p2, d2) / e, 0, 1) if e > 0 else dt(0)))
    for t in (dt(0), dt(1)):
        x = p2 + t * d2
        cand.append((np.clip(dot(x - p1, d1) / a, 0, 1) if a > 0 else dt(0), t))
    dist = [norm((p1 + s * d1) - (p2 + t * d2)) for s, t in cand]
    k = int(np.argmin(dist))
    return dict(d=dist[k], s=cand[k][0], t=cand[k][1], len1=np.sqrt(a), len2=np.sqrt(e), sin2=(den / (a * e) if a > 0 and e > 0 else dt(0)))


# ------------------------------------------------------------------------------------------------ segment - box
def _box_frame(p1, p2, c, quat, dt):
    R = quat_mat(quat, dt)
    return R, R.T @ (_v(p1, dt) - _v(c, dt)), R.T @ (_v(p2, dt) - _v(p1, dt))


def seg_box_ref(p1, p2, c, quat, hb, dt=F64):
    """f(t) = |P(t) - clamp(P(t))|^2 is a convex piecewise quadratic: exact minimum over the breakpoints (a box coordinate crosses +-h), the end points and the
    stationary point inside each piece"""
    hb = _v(hb, dt)
    R, a, d = _box_frame(p1, p2, c, quat, dt)
    ts = {dt(0), dt(1)}
    for k in range(3):
        if d[k] != 0:
            for sg in (-1, 1):
                t = (sg * hb[k] - a[k]) / d[k]
                if 0 < t < 1:
                    ts.add(t)
    ts = sorted(ts)
    cand = list(ts)
    for lo, hi in zip(ts[:-1], ts[1:]):
        x = a + (lo + hi) / 2 * d
        off = np.where(x > hb, hb, np.where(x < -hb, -hb, dt(0)))
        act = np.abs(x) > hb
        den = dot(d[act], d[act])
        if den > 0:
            t = -dot(d[act], (a - off)[act]) / den
            if lo < t < hi:
                cand.append(t)
    f = [norm((a + t * d) - np.clip(a + t * d, -hb, hb)) for t in cand]
    k = int(np.argmin(f))
    x = a + cand[k] * d
    # a stretch of closest points (a segment parallel to a face, or inside the box): another candidate as close as the minimum, away from it
    flat = any(fj - f[k] <= TOL and abs(tj - cand[k]) * norm(d) > 1e-9 for fj, tj in zip(f, cand))
    return dict(d=f[k], t=cand[k], x=x, y=np.clip(x, -hb, hb), on_seg=_v(c, dt) + R @ x, on_box=_v(c, dt) + R @ np.clip(x, -hb, hb), flat=flat)


# ------------------------------------------------------------------------------------------------ capsule - box stretch
def cap_box_ref(p1, p2, c, quat, hb, r, n=N_SAMPLE, dt=F64):
    """The rule of cap_box_two's comment by dense sampling of the axis: the stretch is the longest run, over the face of the closest pair's separating box axis,
    whose other two box coordinates stay within the half extents.  Returns its end parameters (lo, hi), whether both ends are closer than r (and off the box) and
    at least 1 mm apart, whether that answer holds with a 2 % margin on every threshold once the sampling step is allowed for (sure), and `knife`."""
    hb = _v(hb, dt)
    sb = seg_box_ref(p1, p2, c, quat, hb, dt)
    R, a, d = _box_frame(p1, p2, c, quat, dt)
    v = np.abs(sb["x"] - sb["y"])
    kn = int(np.argmax(v))
    vs = np.sort(v)
    if sb["d"] < TOUCH_MIN - TOL:   # the axis meets the box: no normal, the callers do not ask
        return dict(kn=kn, lo=None, hi=None, two=False, sure=True, knife=False, step=1.0 / (n - 1), first_t=sb["t"], d=sb["d"], touching=True)
    knife = bool(vs[2] - vs[1] <= TOL) or bool(abs(sb["d"] - TOUCH_MIN) <= TOL)   # the separating axis itself is a tie / the closest pair touches
    t = np.linspace(0, 1, n).astype(dt)
    X = a[None, :] + t[:, None] * d[None, :]
    oth = [k for k in range(3) if k != kn]
    for k in oth:
        knife |= bool(np.abs(np.abs(a[k]) - hb[k]) <= TOL and abs(d[k]) < 2e-12) or bool(abs(abs(d[k]) - 1e-12) <= 1e-13)
    inside = np.all(np.abs(X[:, oth]) <= hb[oth][None, :], axis=1)
    length = norm(d)
    step = length / (n - 1)
    out = dict(kn=kn, lo=None, hi=None, two=False, sure=True, knife=knife, step=1.0 / (n - 1), first_t=sb["t"], d=sb["d"])
    if not inside.any():
        # the true stretch may still be shorter than two steps
        return out
    idx = np.nonzero(inside)[0]
    runs = np.split(idx, np.nonzero(np.diff(idx) > 1)[0] + 1)
    run = max(runs, key=len)
    lo, hi = t[run[0]], t[run[-1]]
    ln = (hi - lo) * length
    de = [norm(X[i] - np.clip(X[i], -hb, hb)) for i in (run[0], run[-1])]
    two = bool(ln >= STRETCH_MIN and max(de) < r and min(de) > TOUCH_MIN)
    m = 1.02
    if two:   # the sampled stretch lies inside the true one; an end's distance moves by at most one step of the axis
        sure = bool(ln >= m * STRETCH_MIN and max(de) + step <= r / m and min(de) - step >= m * TOUCH_MIN)
    else:
        sure = bool(ln + 2 * step <= STRETCH_MIN / m or max(de) - step >= m * r or min(de) + step <= TOUCH_MIN / m)
    out.update(lo=lo, hi=hi, two=two, sure=sure, length=ln, de=de)
    return out


# ------------------------------------------------------------------------------------------------ box - box
def box_corners(p, quat, h, dt=F64):
    R, h = quat_mat(quat, dt), _v(h, dt)
    sg = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=dt)
    return _v(p, dt)[None, :] + (sg * h[None, :]) @ R.T


def sat_axes(pa, qa, ha, pb, qb, hb, dt=F64):
    """the 15 separating-axis candidates in the order (a's faces, b's faces, edge pairs i-major): dicts of kind 'A' / 'B' / 'E', indices, the unit axis oriented from
    a to b, s = the separation along it (negative: the overlap) and, for an edge pair, l2 = |A_i x B_j|^2.  Edge pairs with l2 = 0 are left out."""
    pa, ha, pb, hb = (_v(x, dt) for x in (pa, ha, pb, hb))
    Ra, Rb = quat_mat(qa, dt), quat_mat(qb, dt)
    t = pb - pa
    out = []

    def add(kind, i, j, n, l2):
        n = n / norm(n)
        tn = dot(t, n)
        if tn < 0:
            n, tn = -n, -tn
        s = tn - (dot(ha, np.abs(Ra.T @ n)) + dot(hb, np.abs(Rb.T @ n)))
        out.append(dict(kind=kind, i=i, j=j, n=n, s=s, l2=l2, tn=tn))
    for i in range(3):
        add("A", i, -1, Ra[:, i], dt(1))
    for j in range(3):
        add("B", -1, j, Rb[:, j], dt(1))
    for i in range(3):
        for j in range(3):
            n = cross(Ra[:, i], Rb[:, j])
            l2 = dot(n, n)
            if l2 > 0:
                add("E", i, j, n, l2)
    return out


def expected_axis(axes):
    """The documented choice (DESIGN D13): the face axis of least overlap, an edge axis only when its overlap times 1.05 is still smaller; near-ties go to the
    earlier axis unless the later wins by BB_TIE.  Returns (index into axes, knife)."""
    knife = False
    best = {"F": None, "E": None}
    for k, ax in enumerate(axes):
        g = "E" if ax["kind"] == "E" else "F"
        if g == "E":
            if abs(ax["l2"] / EPS - 1) <= 1e-3:
                knife = True
            if ax["l2"] < EPS:
                continue
        if best[g] is None:
            best[g] = k
            continue
        lim = axes[best[g]]["s"] + BB_TIE
        knife |= bool(abs(ax["s"] - lim) <= TOL)
        if ax["s"] > lim:
            best[g] = k
    if best["E"] is None:
        return best["F"], knife
    se, sf = axes[best["E"]]["s"], axes[best["F"]]["s"]
    knife |= bool(abs(se * EDGE_FACTOR - sf) <= TOL)
    return (best["E"] if se * EDGE_FACTOR > sf else best["F"]), knife


def clip_polygon(subject, hu, hv):
    """Sutherland - Hodgman: the convex polygon `subject` [m, 2] clipped to the rectangle |u| <= hu, |v| <= hv"""
    poly = [np.asarray(p) for p in subject]
    for ax, sg, lim in ((0, 1, hu), (0, -1, hu), (1, 1, hv), (1, -1, hv)):
        nxt = []
        for k in range(len(poly)):
            p, q = poly[k], poly[(k + 1) % len(poly)]
            ip, iq = sg * p[ax] <= lim, sg * q[ax] <= lim
            if ip:
                nxt.append(p)
            if ip != iq:
                w = (sg * lim - p[ax]) / (q[ax] - p[ax])
                x = p + w * (q - p)
                x[ax] = sg * lim
                nxt.append(x)
        poly = nxt
        if not poly:
            break
    return np.array(poly) if poly else np.zeros((0, 2), subject.dtype)


def polygon_area(P):
    if len(P) < 3:
        return P.dtype.type(0) if len(P) else 0.0
    x, y = P[:, 0], P[:, 1]
    return abs(dot(x, np.roll(y, -1)) - dot(y, np.roll(x, -1))) / 2


def hull_area(P):
    """area of the convex hull of a few points in convex position (or fewer than three)"""
    P = np.asarray(P)
    if len(P) < 3:
        return 0.0
    c = P.mean(0)
    return polygon_area(P[np.argsort(np.arctan2((P[:, 1] - c[1]).astype(F64), (P[:, 0] - c[0]).astype(F64)))])


def significant_vertices(P, tol):
    """The corners of the convex polygon P that stay when every vertex within 2 tol of a neighbour, or of the line through its neighbours, is dropped (one by one, the
    least significant first).  Also returns whether some vertex sat between tol / 2 and 2 tol: a knife edge of the kept-point rule, whose own margin is tol."""
    P = [p for p in P]
    knife = False
    while len(P) >= 3:
        m = len(P)
        sig = []
        for k in range(m):
            a, b, c = P[k - 1], P[k], P[(k + 1) % m]
            e = c - a
            le = norm(e)
            h = abs(e[0] * (b[1] - a[1]) - e[1] * (b[0] - a[0])) / le if le > 0 else 0.0
            sig.append(min(h, norm(b - a), norm(c - b)))
        k = int(np.argmin(sig))
        if sig[k] > 2 * tol:
            break
        if sig[k] >= tol / 2:
            knife = True
        P.pop(k)
    return np.array(P), knife


def face_frame(pr, qr, hr, r, nr, dt=F64):
    """the face of box (pr, qr, hr) along its axis r whose outward normal is nr: centre, the two in-plane axes (r+1, r+2), their half extents"""
    R = quat_mat(qr, dt)
    r1, r2 = (r + 1) % 3, (r + 2) % 3
    return _v(pr, dt) + nr * _v(hr, dt)[r], R[:, r1], R[:, r2], _v(hr, dt)[r1], _v(hr, dt)[r2]


def incident_face(pi, qi, hi, nr, dt=F64):
    """the face of box (pi, qi, hi) whose outward normal is most anti-parallel to nr: (axis k, outward normal, centre, margin to the runner-up)"""
    R, hi = quat_mat(qi, dt), _v(hi, dt)
    cs = np.abs(R.T @ nr)
    k = int(np.argmax(cs))
    no = R[:, k] * (-1 if dot(R[:, k], nr) > 0 else 1)
    return k, no, _v(pi, dt) + no * hi[k], np.sort(cs)[2] - np.sort(cs)[1]


def overlap_polygon(ref, inc, r, nr, dt=F64):
    """parallel faces: the incident box's facing face projected onto the reference face (u, v about the face centre) and clipped to its rectangle: [m, 2], area"""
    cr, eu, ev, hu, hv = face_frame(*ref, r, nr, dt)
    k, no, ci, _ = incident_face(*inc, nr, dt)
    Ri, hi = quat_mat(inc[1], dt), _v(inc[2], dt)
    k1, k2 = (k + 1) % 3, (k + 2) % 3
    quad = np.array([[dot(x - cr, eu), dot(x - cr, ev)] for x in (ci + s1 * hi[k1] * Ri[:, k1] + s2 * hi[k2] * Ri[:, k2] for s1, s2 in ((1, 1), (-1, 1), (-1, -1), (1, -1)))], dtype=dt)
    P = clip_polygon(quad, hu, hv)
    return P, polygon_area(P)


# ================================================================================================ the checker
class Verdict:
    """bad: what the output violates (empty: it passes); knife: the case sits on one of the code's own thresholds, the exact comparisons were left out;
    stats: measured figures (errors in metres, area ratio)"""

    def __init__(self):
        self.bad, self.knife, self.stats = [], False, {}
        self.free = False     # the witness (seg_seg, seg_box: the closest pair; box_box2: the order of the contacts) is not unique: two correct outputs need not agree on it
        self.wit_tol = TOL    # how far the witnesses of two correct outputs may lie apart (seg_seg: conditioned as 1 / sin^2 of the angle)

    def need(self, ok, msg):
        if not ok:
            self.bad.append(msg)

    def __bool__(self):
        return not self.bad


def _on_segment(V, what, x, p, q, tol=TOL):
    """x lies on the segment p - q: parameter in [0, 1] to tol, distance from the line within tol.  Returns the parameter."""
    d = q - p
    a = dot(d, d)
    if a == 0:
        V.need(norm(x - p) <= tol, f"{what}: off its (point) segment by {float(norm(x - p)):.3g}")
        return 0.0
    s = dot(x - p, d) / a
    V.need(-tol <= s <= 1 + tol, f"{what}: parameter {float(s)!r} outside [0, 1]")
    off = norm(x - (p + s * d))
    V.need(off <= tol, f"{what}: {float(off):.3g} off its segment's line")
    return s


def check_seg_seg(q, out, dt=F64):
    a = unpack(SEGSEG, q, dt)
    out = _v(out, dt)
    d2, c1, c2 = out[0], out[1:4], out[4:7]
    V = Verdict()
    ref = seg_seg_ref(**a, dt=dt)
    _on_segment(V, "c1", c1, a["p1"], a["q1"])
    _on_segment(V, "c2", c2, a["p2"], a["q2"])
    V.need(d2 >= 0, "negative squared distance")
    dc = np.sqrt(max(d2, 0))
    V.need(abs(norm(c1 - c2) - dc) <= TOL, f"witness distance {float(norm(c1 - c2))!r} != returned {float(dc)!r}")
    V.need(dc >= ref["d"] - TOL, f"closer than the minimum: {float(dc)!r} < {float(ref['d'])!r}")
    bound = TOL
    L = max(ref["len1"], ref["len2"])
    for ln in (ref["len1"], ref["len2"]):   # a segment shorter than 1e-6 m is a point to the code
        if ln * ln <= EPS * (1 + 1e-6):
            bound = bound + ln
            V.knife |= bool(ln > 0 and abs(ln * ln / EPS - 1) <= 1e-6)
    if min(ref["len1"], ref["len2"]) > 0 and ref["sin2"] <= EPS * (1 + 1e-6):   # near-parallel: the code starts from an end of the first segment
        bound = bound + L * 1e-6
        V.knife |= bool(abs(ref["sin2"] / EPS - 1) <= 1e-6)
    V.need(dc <= ref["d"] + bound, f"not the minimum: {float(dc)!r} > {float(ref['d'])!r} + {float(bound):.3g}")
    V.stats["err"] = float(dc - ref["d"])
    V.stats["banded"] = bool(bound > TOL)
    # the interior stationary point is a quotient by a e sin^2: the rounding of its numerator (2e-16 of products of the lengths and the offset) moves a witness by
    # about 1e-15 (|p1 - p2| + L) / sin^2; parallel or point-like segments have a whole stretch of closest pairs
    if bound > TOL or min(ref["len1"], ref["len2"]) == 0 or ref["sin2"] <= 1e-9:
        V.free = True
    else:
        V.wit_tol = TOL + 1e-15 * float(norm(a["p1"] - a["p2"]) + ref["len1"] + ref["len2"]) / float(ref["sin2"])
    return V


def check_seg_box(q, out, dt=F64, V=None):
    a = unpack(SEGBOX, q, dt)
    out = _v(out, dt)
    e2, cs, cb = out[0], out[1:4], out[4:7]
    V = V or Verdict()
    ref = seg_box_ref(a["p1"], a["p2"], a["c"], a["quat"], a["hb"], dt)
    _on_segment(V, "on_seg", cs, a["p1"], a["p2"])
    R = quat_mat(a["quat"], dt)
    y = R.T @ (cb - a["c"])
    V.need(bool(np.all(np.abs(y) <= a["hb"] + TOL)), f"on_box outside the box: local {y.astype(F64).tolist()}")
    V.need(e2 >= 0, "negative squared distance")
    dc = np.sqrt(max(e2, 0))
    V.need(abs(norm(cs - cb) - dc) <= TOL, f"witness distance {float(norm(cs - cb))!r} != returned {float(dc)!r}")
    V.need(abs(dc - ref["d"]) <= TOL, f"distance {float(dc)!r} != reference {float(ref['d'])!r}")
    V.stats["err"] = float(dc - ref["d"])
    V.free = bool(ref["flat"])
    return V


def check_cap_box(q, out, dt=F64, n=N_SAMPLE):
    a = unpack(CAPBOX, q, dt)
    out = _v(out, dt)
    V = check_seg_box(q, out[:7], dt)
    two = out[7] != 0
    ref = cap_box_ref(a["p1"], a["p2"], a["c"], a["quat"], a["hb"], a["r"], n, dt)
    V.knife = ref["knife"]
    V.stats["two"] = bool(two)
    if ref["sure"] and not ref["knife"]:
        V.need(two == ref["two"], f"answers {bool(two)}, the sampled rule says {ref['two']} with a 2 % margin (stretch {ref.get('length')}, end distances {ref.get('de')}, r {float(a['r'])})")
    if not two:
        return V
    R = quat_mat(a["quat"], dt)
    ends = []
    for e in range(2):
        s, b = out[8 + 6 * e:11 + 6 * e], out[11 + 6 * e:14 + 6 * e]
        ends.append(_on_segment(V, f"end {e} axis point", s, a["p1"], a["p2"]))
        x = R.T @ (s - a["c"])
        clamp = a["c"] + R @ np.clip(x, -a["hb"], a["hb"])
        V.need(norm(b - clamp) <= TOL, f"end {e}: box point is {float(norm(b - clamp)):.3g} from the clamp of its axis point")
        dd = norm(s - b)
        V.need(TOUCH_MIN < dd < a["r"], f"end {e}: distance {float(dd)!r} outside (1e-9, r = {float(a['r'])!r})")
    s0, s1 = out[8:11], out[14:17]
    V.need(norm(s1 - s0) >= STRETCH_MIN - TOL, f"ends {float(norm(s1 - s0))!r} apart: less than 1 mm")
    if ref["lo"] is not None and not ref["knife"]:
        for e, (got, want) in enumerate(zip(ends, (ref["lo"], ref["hi"]))):
            V.need(abs(got - want) <= ref["step"] + TOL, f"end {e} at parameter {float(got)!r}, the sampled stretch ends at {float(want)!r} (step {ref['step']:.3g})")
    elif ref["lo"] is None and not ref["knife"]:
        V.need(False, "answers true where the axis meets the box or no sample of it lies over the face")
    return V


def check_box_box(q, out, dt=F64, fixed=True):
    """out = [count | 4 x (pos 3, normal 3, dist)].  `fixed`: hold the kept points to the rule with the fourth-contact fix (False: the parent's rule, only the quarter)."""
    a = unpack(BOXBOX, q, dt)
    out = _v(out, dt)
    n = int(out[0])
    con = out[1:29].reshape(4, 7)[:max(0, min(n, 4))]
    V = Verdict()
    V.stats["n"] = n
    axes = sat_axes(**a, dt=dt)
    usable = [ax for ax in axes if ax["kind"] != "E" or ax["l2"] >= EPS]
    smax = max(ax["s"] for ax in usable)
    # (an edge pair's axis is a normalised cross product: its direction and its overlap carry the rounding of the factors divided by |A_i x B_j|)
    tol_of = lambda ax: TOL + (1e-15 / np.sqrt(ax["l2"]) if ax["kind"] == "E" else 0)  # noqa: E731
    V.need(0 <= n <= 4, f"count {n}")
    if abs(smax) <= TOL or any(ax["kind"] == "E" and abs(ax["s"]) <= tol_of(ax) and ax["s"] >= smax - tol_of(ax) for ax in usable) or any(ax["kind"] == "E" and abs(ax["l2"] / EPS - 1) <= 1e-3 and ax["s"] > -TOL for ax in axes):
        V.knife = True   # touching to rounding: either answer
    elif smax > 0:
        V.need(n == 0, f"{n} contacts although an axis separates the boxes by {float(smax):.3g}")
        return V
    else:
        V.need(n >= 1, f"no contact although every axis overlaps (least overlap {float(-smax):.3g})")
    if n == 0 or n > 4:
        return V
    nrm, dist, pos = con[:, 3:6], con[:, 6], con[:, 0:3]
    V.need(bool(np.all(np.abs(nrm - nrm[0]) == 0)), "the contacts do not share one normal")
    V.need(abs(norm(nrm[0]) - 1) <= TOL, f"normal of length {float(norm(nrm[0]))!r}")
    V.need(bool(np.all(dist < 0)), f"a kept contact does not penetrate: {dist.astype(F64).tolist()}")
    # the normal is a SAT axis, oriented from a to b, of near-least overlap
    err = [norm(nrm[0] - ax["n"]) if ax["tn"] > TOL else min(norm(nrm[0] - ax["n"]), norm(nrm[0] + ax["n"])) for ax in axes]
    k = next((m for m, ax in enumerate(axes) if err[m] <= tol_of(ax) and (ax["kind"] != "E" or ax["l2"] >= EPS)), int(np.argmin(err)))   # (a face axis before an edge pair along it)
    ax = axes[k]
    tol_n = tol_of(ax)
    V.need(err[k] <= tol_n, f"the normal is no separating-axis candidate oriented from a to b (nearest: {ax['kind']}{ax['i']}{ax['j']}, {float(err[k]):.3g} away)")
    if err[k] > 1e-6:
        return V
    V.need(ax["s"] >= EDGE_FACTOR * smax - EDGE_FACTOR * BB_TIE - TOL, f"axis of overlap {float(-ax['s']):.6g}, the least is {float(-smax):.6g}")
    ke, knife_axis = expected_axis(axes)
    V.knife |= knife_axis
    if not V.knife:
        V.need(k == ke or err[ke] <= tol_n, f"axis {ax['kind']}{ax['i']}{ax['j']} chosen, the rule gives {axes[ke]['kind']}{axes[ke]['i']}{axes[ke]['j']}")
    V.need(bool(np.all(dist >= ax["s"] - TOL)), f"a contact deeper ({float(-dist.min())!r}) than the axis's overlap ({float(-ax['s'])!r})")
    for name, (p, qq, h) in (("a", (a["pa"], a["qa"], a["ha"])), ("b", (a["pb"], a["qb"], a["hb"]))):
        loc = (pos - p[None, :]) @ quat_mat(qq, dt)
        V.need(bool(np.all(np.abs(loc) <= h[None, :] + 0.5 * np.abs(dist)[:, None] + TOL)), f"a contact point outside box {name} inflated by half its depth")
    if ax["kind"] == "E":
        V.need(n == 1, f"{n} contacts on an edge - edge axis")
        V.need(abs(dist[0] - ax["s"]) <= tol_n, f"edge contact of depth {float(-dist[0])!r}, the axis overlaps by {float(-ax['s'])!r}")
        Ra, Rb = quat_mat(a["qa"], dt), quat_mat(a["qb"], dt)
        i, j = ax["i"], ax["j"]
        ca, cb = Ra.T @ ax["n"], Rb.T @ ax["n"]
        if min(min(abs(ca[m]) for m in range(3) if m != i), min(abs(cb[m]) for m in range(3) if m != j)) <= TOL:
            V.knife = True   # the supporting edge is a tie
            return V
        pA = a["pa"] + sum(Ra[:, m] * np.sign(ca[m]) * a["ha"][m] for m in range(3) if m != i)
        pB = a["pb"] - sum(Rb[:, m] * np.sign(cb[m]) * a["hb"][m] for m in range(3) if m != j)
        u, w, d = Ra[:, i], Rb[:, j], pB - pA   # common perpendicular of the two edge lines
        uw = dot(u, w)
        den = 1 - uw * uw
        al, be = (dot(u, d) - uw * dot(w, d)) / den, (uw * dot(u, d) - dot(w, d)) / den
        mid = 0.5 * ((pA + al * u) + (pB + be * w))
        tol_p = TOL + 4e-16 * (1 + norm(d)) / den
        V.need(norm(pos[0] - mid) <= tol_p, f"edge contact {float(norm(pos[0] - mid)):.3g} from the midpoint of the edges' common perpendicular")
        V.stats["err"] = float(norm(pos[0] - mid))
        return V
    # a face axis: reference box, incident box
    refA = ax["kind"] == "A"
    ref, inc = ((a["pa"], a["qa"], a["ha"]), (a["pb"], a["qb"], a["hb"])) if refA else ((a["pb"], a["qb"], a["hb"]), (a["pa"], a["qa"], a["ha"]))
    r = ax["i"] if refA else ax["j"]
    nr = ax["n"] if refA else -ax["n"]   # outward normal of the reference face, towards the incident box
    if ax["tn"] <= TOL:
        V.knife = True
        return V
    cr, eu, ev, hu, hv = face_frame(*ref, r, nr, dt)
    kI, no, ci, gap = incident_face(*inc, nr, dt)
    if gap <= TOL:
        V.knife = True
        return V
    Ri, hi = quat_mat(inc[1], dt), _v(inc[2], dt)
    F = pos - 0.5 * dist[:, None] * nr[None, :]    # on the reference face ...
    I = pos + 0.5 * dist[:, None] * nr[None, :]    # ... and the point of the incident face under it: pos is their midpoint
    uv = np.stack([(F - cr) @ eu, (F - cr) @ ev], 1)
    V.need(bool(np.all(np.abs((F - cr) @ nr) <= TOL)), "midpoint convention: pos - dist/2 n is off the reference face's plane")
    V.need(bool(np.all(np.abs(uv[:, 0]) <= hu + TOL) and np.all(np.abs(uv[:, 1]) <= hv + TOL)), "a contact outside the reference face's rectangle")
    li = (I - ci) @ Ri
    V.need(bool(np.all(np.abs(li[:, kI]) <= TOL)), f"midpoint convention: pos + dist/2 n is off the incident face's plane by {float(np.abs(li[:, kI]).max()):.3g}")
    for m in ((kI + 1) % 3, (kI + 2) % 3):
        V.need(bool(np.all(np.abs(li[:, m]) <= hi[m] + TOL)), "a contact outside the incident face's rectangle")
    V.stats["err"] = float(max(np.abs((F - cr) @ nr).max(), np.abs(li[:, kI]).max()))
    for z in range(n):
        for y in range(z):
            V.need(norm(uv[z] - uv[y]) > 1e-6 * np.sqrt(hu * hu + hv * hv) * 0.5, f"contacts {y} and {z} coincide")
    # A corner of one face on the outline of the other (to rounding) is inside it or not as the rounding falls: the candidate exists under another index or not
    # at all, and the lowest index breaks the ties between equally deep and equally far candidates.  The kept set obeys everything above; its order is free.
    k1, k2 = (kI + 1) % 3, (kI + 2) % 3
    quad = np.array([ci + s1 * hi[k1] * Ri[:, k1] + s2 * hi[k2] * Ri[:, k2] for s1, s2 in ((1, 1), (-1, 1), (-1, -1), (1, -1))])
    qu, qv = (quad - cr) @ eu, (quad - cr) @ ev
    on_u, on_v = np.abs(np.abs(qu) - hu) <= TOL, np.abs(np.abs(qv) - hv) <= TOL
    V.free = bool(np.any(on_u & (np.abs(qv) <= hv + TOL)) or np.any(on_v & (np.abs(qu) <= hu + TOL)))
    for su, sv in ((1, 1), (-1, 1), (-1, -1), (1, -1)):   # ... and a corner of the reference face on an edge of the incident one
        for m in range(4):
            e0, e1 = np.array([qu[m], qv[m]]), np.array([qu[(m + 1) % 4], qv[(m + 1) % 4]])
            w, le = np.array([su * hu, sv * hv]) - e0, norm(e1 - e0)
            V.free |= bool(abs((e1 - e0)[0] * w[1] - (e1 - e0)[1] * w[0]) <= TOL * le and -TOL <= dot(w, e1 - e0) <= le * le + TOL)
    if norm(cross(nr, no)) > 1e-9:
        return V
    # parallel faces: the exact overlap polygon
    P, area = overlap_polygon(ref, inc, r, nr, dt)
    tol_v = 1e-6 * np.sqrt(hu * hu + hv * hv)
    if len(P) < 3 or area <= tol_v * tol_v:
        V.knife = True
        return V
    for z in range(n):
        dv = min(norm(uv[z] - p) for p in P)
        V.need(dv <= TOL, f"contact {z} is {float(dv):.3g} from the nearest corner of the overlap polygon")
    ratio = float(hull_area(uv) / area)
    V.stats["ratio"] = ratio
    S, knife_p = significant_vertices(P, tol_v)
    V.stats["corners"] = len(S)
    if len(S) >= 3:
        V.need(ratio >= 0.25 - 1e-9, f"the kept hull covers {ratio:.4f} of the overlap polygon: less than a quarter")
    if fixed and not knife_p:
        if len(S) >= 4:
            V.need(n == 4, f"{n} contacts kept of an overlap polygon with {len(S)} corners")
        if len(S) == 4 and n == 4:
            V.need(all(min(norm(s - p) for p in uv) <= 2 * tol_v for s in S), "a corner of the four-cornered overlap is not kept")
    return V


CHECK = {SEGSEG: check_seg_seg, SEGBOX: check_seg_box, CAPBOX: check_cap_box, BOXBOX: check_box_box}
