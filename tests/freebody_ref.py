"""Independent reference of the soft-constraint step for FREE BOXES OVER THE TABLE AND FLOOR PLANES (numpy only).

Written from MuJoCo's documented computation ("Computation" chapter: constraint model, solver parameters, the convex primal problem) and the
[UPSTREAM] functions named per rule, not from the oracle or the kernels.  What is this project's own convention and not MuJoCo's is marked "ours" and
comes from DESIGN.md (D3, D8, D13) and include/hrgym_state.h.  With no arm-box contact the robot block of the Newton system splits off exactly, so a box
of any stepper (the cube, handover and lifting kernels, the four stacking cubes) must follow this file.

    R = Rules()                                        # the rules as the project means them; the teeth test mutates one field at a time
    M = Model.from_desc(desc, np.longdouble)           # constants of a hrg_model_desc in the scalar type
    pos, quat, vel = advance(M, pos, quat, vel, n)     # n substeps of mj_step; stop="kkt" (default) solves to the KKT residual KKT_TOL and asserts it
    ... advance(..., stop="code", start="a0" | "warm") # stops by the rule the model publishes (solver_tol, solver_iters): only to measure a floor

Scalar type: np.float64 or np.longdouble (every array is kept in it; the 6 x 6 solves are written out because numpy.linalg has no long double)."""
from dataclasses import dataclass, replace

import numpy as np

KKT_TOL = 1e-13          # rule 6: ||M (a - a0) + J' grad s|| <= KKT_TOL (1 + ||M a0||)
# Rule 5, last line -- a NAMED DEVIATION of this project.  mj_makeImpedance [UPSTREAM engine_core_constraint.c] sets, after
# R = (1 - imp) / imp * diagApprox, R <- 2 mu^2 R on every edge of a PYRAMIDAL contact (MuJoCo's value: 2 * mu * mu, 2.0 at mu = 1).  The oracle and every
# kernel leave that factor out, and putting it in breaks a behavioural test of the hammering task, so the reference carries the code's value under this name:
MUJOCO_PYRAMID_R_SCALE = "2 mu^2"
PYRAMID_R_SCALE = 1.0    # the factor on R of a pyramid edge: a number, or MUJOCO_PYRAMID_R_SCALE


@dataclass(frozen=True)
class Rules:
    """the knobs of the rules below; defaults = the rules as stated.  Every other value is a mutation (tests/test_freebody.py, teeth)"""
    solimp_mid: float = None          # None: the model's solimp[3]
    pyramid_r_scale: object = PYRAMID_R_SCALE  # a number, or MUJOCO_PYRAMID_R_SCALE
    contact_at_surface: bool = False  # False: contact point at mid-depth (rule 2)
    position_from_old_velocity: bool = False   # False: p <- p + h v_new (rule 7, semi-implicit Euler)
    mu: float = None                  # None: the model's friction_static
    tangent_angle: float = 0.0        # tangents of a plane contact turned about the normal by this angle; 0: world x and y (rule 2)
    gyroscopic: bool = True           # the bias torque w x (I_world w) of rule 1
    table: bool = True                # False: no table plane (a stepper whose table is not a corner-against-plane test: the lifting board)


@dataclass
class Model:
    T: type
    h: object
    gravity: object
    solref: object
    solimp: object
    mu: object
    solver_tol: float
    solver_iters: int
    half: object
    mass: object
    inertia: object
    table_top_z: object
    table_center: object
    table_half: object
    floor_z: object

    @classmethod
    def from_desc(cls, d, T=np.float64, half=None, mass=None, inertia=None):
        v = lambda x: np.array([float(y) for y in x], dtype=T)  # noqa: E731
        return cls(T=T, h=T(d.timestep), gravity=v(d.gravity), solref=v(d.solref), solimp=v(d.solimp), mu=T(d.friction_static), solver_tol=float(d.solver_tol),
                   solver_iters=int(d.solver_iters), half=v(half if half is not None else d.box_half), mass=T(mass if mass is not None else d.box_mass),
                   inertia=v(inertia if inertia is not None else d.box_inertia), table_top_z=T(d.table_top_z), table_center=v(d.table_center),
                   table_half=v(d.table_half), floor_z=T(d.floor_z))


# ------------------------------------------------------------------------------------------------ small algebra in the scalar type
def quat_to_mat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=q.dtype)


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]], dtype=a.dtype)


def norm(x):
    return np.sqrt((x * x).sum())


def solve_spd(A, b):
    """x with A x = b for a symmetric positive definite A, by Cholesky, in A's scalar type"""
    n = len(b)
    L = np.zeros_like(A)
    for i in range(n):
        for j in range(i + 1):
            s = A[i, j] - (L[i, :j] * L[j, :j]).sum()
            L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
    y = np.zeros_like(b)
    for i in range(n):
        y[i] = (b[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    x = np.zeros_like(b)
    for i in reversed(range(n)):
        x[i] = (y[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    return x


# ------------------------------------------------------------------------------------------------ the rules
def impedance(M, R, dist):
    """rule 4, [UPSTREAM mj_makeImpedance / getimpedance]: imp(|dist|) of solimp (d0, dmax, width, midpoint, power 2) and the spring / damper (K, B) of solref"""
    T = M.T
    d0, dmax, width, mid, power = M.solimp
    assert power == 2
    if R.solimp_mid is not None:
        mid = T(R.solimp_mid)
    x = abs(dist) / width
    if x >= 1:
        y = T(1)
    elif x < mid:
        y = x * x / mid                      # a x^p with a = 1 / mid^(p - 1)
    else:
        y = 1 - (1 - x) * (1 - x) / (1 - mid)  # 1 - b (1 - x)^p with b = 1 / (1 - mid)^(p - 1)
    imp = d0 + y * (dmax - d0)
    tau, zeta = M.solref
    assert tau >= 2 * M.h                    # (mj_makeImpedance's "refsafe" clamp does not bind)
    return imp, 1 / (dmax * dmax * tau * tau * zeta * zeta), 2 / (dmax * tau)


def contacts(M, R, pos, Rm):
    """rule 2 (ours, DESIGN D3 / D8 / D13): a box corner under a plane is a contact, normal +z; -> list of (dist, point)"""
    T = M.T
    out = []
    for cn in range(8):
        loc = np.array([M.half[k] if (cn >> k) & 1 else -M.half[k] for k in range(3)], dtype=T)
        p = pos + Rm @ loc
        planes = [M.floor_z]
        if R.table and abs(p[0] - M.table_center[0]) <= M.table_half[0] and abs(p[1] - M.table_center[1]) <= M.table_half[1] and p[2] > M.table_top_z - T(0.05):
            planes.insert(0, M.table_top_z)
        for z0 in planes:
            dist = p[2] - z0
            if dist < 0:
                out.append((dist, np.array([p[0], p[1], z0 if R.contact_at_surface else z0 + dist / 2], dtype=T)))
    return out


def pyramid_r_scale(R, mu):
    """the factor on R of a pyramid edge under rules R, in mu's scalar type"""
    return 2 * mu * mu if R.pyramid_r_scale == MUJOCO_PYRAMID_R_SCALE else type(mu)(R.pyramid_r_scale)


def rows(M, R, pos, vel, cons):
    """rules 3-5 [UPSTREAM mj_instantiateContact, mj_diagApprox, mj_makeImpedance]: J, aref, D of the four pyramid edges of every contact"""
    T = M.T
    mu = M.mu if R.mu is None else T(R.mu)
    c, s = np.cos(T(R.tangent_angle)), np.sin(T(R.tangent_angle))
    n, t1, t2 = np.array([0, 0, 1], dtype=T), np.array([c, s, 0], dtype=T), np.array([-s, c, 0], dtype=T)
    J, aref, D = [], [], []
    for dist, point in cons:
        imp, K, B = impedance(M, R, dist)
        diag_approx = (1 / M.mass) * (1 + mu * mu)          # mj_diagApprox, pyramidal: tran + mu^2 tran, tran = body_invweight0 = 1 / m of a free body
        Rr = (1 - imp) / imp * diag_approx
        Rr = Rr * pyramid_r_scale(R, mu)
        r = point - pos
        for t, sg in ((t1, 1), (t1, -1), (t2, 1), (t2, -1)):
            d = n + sg * mu * t
            j = np.concatenate([d, np.cross(r, d)])         # d . (v + w x r) = d . v + (r x d) . w
            J.append(j)
            aref.append(-B * (j @ vel) - K * imp * dist)
            D.append(1 / Rr)
    return np.array(J, dtype=T).reshape(-1, 6), np.array(aref, dtype=T), np.array(D, dtype=T)


def line_search(c0, c1, x, p, D):
    """exact minimiser over alpha > 0 of phi(alpha) = cost(a + alpha d): phi' is piecewise linear and increasing, c0 + c1 alpha over the rows active at 0+
    (c0 < 0 < c1 on entry); walk its breakpoints alpha_r = -x_r / p_r in order, toggling row r, until the root of the current piece lies inside it"""
    act = (x < 0) | ((x == 0) & (p < 0))
    c0 = c0 + (D * x * p)[act].sum()
    c1 = c1 + (D * p * p)[act].sum()
    br = sorted((-x[r] / p[r], r) for r in range(len(x)) if p[r] != 0 and -x[r] / p[r] > 0)
    for al, r in br:
        if -c0 / c1 <= al:
            break
        sgn = -1 if act[r] else 1
        c0, c1, act[r] = c0 + sgn * D[r] * x[r] * p[r], c1 + sgn * D[r] * p[r] * p[r], not act[r]
    return -c0 / c1


def solve(Mm, a0, J, aref, D, a, tol, max_iter):
    """rule 6 [UPSTREAM mj_solNewton's problem, not its code]: minimise 1/2 (a - a0)' M (a - a0) + sum_r s_r(J_r a - aref_r), s(x) = 1/2 D x^2 for x < 0, else 0.
    Newton on the active set with an exact line search: the cost is strictly convex and piecewise quadratic, every step lands on the minimiser of the
    current piece or on the exact minimiser along the Newton direction, so the method ends after finitely many pieces.  -> (a, residual / (1 + ||M a0||))"""
    scale = 1 + norm(Mm @ a0)
    for it in range(max_iter + 1):
        x = J @ a - aref
        act = x < 0
        g = Mm @ (a - a0) + J.T @ np.where(act, D * x, 0)
        if norm(g) <= tol * scale or it == max_iter:
            break
        H = Mm + (J[act].T * D[act]) @ J[act]
        d = -solve_spd(H, g)
        p = J @ d
        stays = np.array_equal((x + p) < 0, act)
        a = a + (1 if stays else line_search((Mm @ (a - a0)) @ d, d @ (Mm @ d), x, p, D)) * d
    return a, norm(g) / scale


def substep(M, R, pos, quat, vel, warm=None, stop="kkt", start="a0"):
    """one mj_step [UPSTREAM mj_forward + mj_Euler] of one free box; -> pos, quat, vel, acceleration"""
    T = M.T
    Rm = quat_to_mat(quat)
    w = vel[3:]
    # rule 1 [UPSTREAM mj_crb / mj_rne for a free joint; ours: world-frame angular velocity]: M = blockdiag(m 1, R diag(I) R'), bias torque w x (I_world w)
    Iw = (Rm * M.inertia) @ Rm.T
    Mm = np.zeros((6, 6), dtype=T)
    Mm[:3, :3] = np.eye(3, dtype=T) * M.mass
    Mm[3:, 3:] = Iw
    bias = np.cross(w, Iw @ w) if R.gyroscopic else np.zeros(3, dtype=T)
    a0 = np.concatenate([M.gravity, solve_spd(Iw, -bias)])
    cons = contacts(M, R, pos, Rm)
    if cons:
        J, aref, D = rows(M, R, pos, vel, cons)
        if stop == "kkt":
            a, res = solve(Mm, a0, J, aref, D, a0.copy(), KKT_TOL, 60)
            assert res <= KKT_TOL, f"KKT residual {res:.3e} after the solve ({len(cons)} contacts)"
        else:
            a, res = solve(Mm, a0, J, aref, D, (a0 if start == "a0" or warm is None else warm).copy(), M.solver_tol, M.solver_iters)
    else:
        a = a0
    # rule 7 [UPSTREAM mj_Euler, mju_quatIntegrate], free joint, no damping
    vnew = vel + M.h * a
    pos = pos + M.h * (vel if R.position_from_old_velocity else vnew)[:3]
    wn = norm(vnew[3:])
    if wn > 0:
        half_angle = M.h * wn / 2
        dq = np.concatenate([[np.cos(half_angle)], np.sin(half_angle) * vnew[3:] / wn]).astype(T)
        quat = quat_mul(dq, quat)    # the angular velocity is world-frame (ours): the increment multiplies from the left
        quat = quat / norm(quat)
    return pos, quat, vnew, a


def advance(M, pos, quat, vel, n, rules=Rules(), stop="kkt", start="a0", warm=None, return_warm=False):
    """n substeps of one box from (pos[3], quat[4] (w, x, y, z), vel[6] (linear, angular; world frame)), all converted to the model's scalar type"""
    T = M.T
    pos, quat, vel = (np.array([float(x) for x in v], dtype=T) for v in (pos, quat, vel))
    for _ in range(n):
        pos, quat, vel, warm = substep(M, rules, pos, quat, vel, warm, stop, start)
    return (pos, quat, vel, warm) if return_warm else (pos, quat, vel)


def mutated(**kw):
    return replace(Rules(), **kw)
