"""Scenarios, kernel families and the bound of the free-body tests (tests/test_freebody.py on the oracle, tests/test_freebody_gpu.py on the kernels).

A scenario is a start state of one free box; a family is one stepper (a task's model + how its box state is reached).  Every env of a family's batch holds one
scenario (stacking: four, one per cube), takes zero actions, and is read back after every policy step.

The bound holds nothing against the code under test.  Per quantity X (pos, quat up to sign, linear and angular velocity) and policy step:
    floor_solve = max over the two starts of |X_ref(stop="code") - X_ref|      the stop rule the model publishes, from a0 and from the previous substep's solution
    floor_round = |X_ref(float64) - X_ref(long double)|
    |X_code - X_ref| <= 8 (floor_solve + floor_round)                          (the factor tests/test_sac_gpu.py gives its noise floor)
with X_ref the long double reference solved to its KKT residual, and a scenario counts only while floor_solve + floor_round stays under CAP.
The floors of a scenario are taken over the policy steps it is compared at (the largest): two valid computations that are 7e-16 apart after one policy step
are not closer after the next because the two roundings happened to cross there (measured: the float64 and long double positions of `overhang` agree to
0.05 ulp after step 2 and to 3 ulp after steps 1 and 3), and a float64 state cannot be asked to sit nearer to a long double one than float64 is spaced."""
import numpy as np

import freebody_ref as fr
from human_robot_gym_amd._cstruct import CONST
from parity import GEOM_BOX

CAP = dict(pos=1e-6, quat=1e-6, vel=1e-5)    # metres, quaternion components, m/s and rad/s
FACTOR = 8.0
N_POLICY = 3                                              # policy steps compared (25 substeps each at the default control rate)


def _q(axis, ang):
    ax = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax])


def _corner_spin(seed):
    """the scenario of a box dropped onto a corner with spin: one draw of pp_scenarios.tumble's distribution (spin, orientation, lateral speed), in its
    order, lowest corner 2 cm over the table, two policy steps"""
    rng = np.random.RandomState(seed)
    w = rng.uniform(-8, 8, 3)
    ang = rng.uniform(0, np.pi)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    return "table", _q(ax, ang), 0.02, [rng.uniform(-.3, .3), rng.uniform(-.3, .3), 0, w[0], w[1], w[2]], 2


# name -> (anchor, quat, gap: height of the box's lowest corner over the plane [m] (negative: inside), vel, policy steps compared)
# anchors: "table" on the table away from its edges, "edge" centre past the table's edge (two corners off it), "floor" beside the table, "air" no contact
SCENARIOS = {
    "drop_flat_1cm": ("table", _q([1, 0, 0], 0), 0.01, [0] * 6, 3),
    "inside_0.2mm": ("table", _q([1, 0, 0], 0), -0.0002, [0] * 6, 3),     # first half of the impedance curve (x < midpoint)
    "inside_0.7mm": ("table", _q([1, 0, 0], 0), -0.0007, [0] * 6, 3),     # second half
    "inside_2mm": ("table", _q([1, 0, 0], 0), -0.002, [0] * 6, 3),        # beyond width = 1 mm: saturated
    "drop_on_edge": ("table", _q([1, 0, 0], np.pi / 4), 0.002, [0, 0, -0.3, 0, 0, 0], 3),
    "corner_spin_s3": _corner_spin(3),
    "corner_spin_s7": _corner_spin(7),
    "slide_x": ("table", _q([1, 0, 0], 0), -0.0004, [0.5, 0, 0, 0, 0, 0], 3),
    "slide_diagonal": ("table", _q([1, 0, 0], 0), -0.0004, [0.35, 0.35, 0, 0, 0, 0], 3),
    "overhang": ("edge", _q([1, 0, 0], 0), -0.0003, [0] * 6, 3),
    "floor_1cm": ("floor", _q([1, 0, 0], 0), 0.01, [0] * 6, 3),
    "air_spin": ("air", _q([1, 2, -1], 0.7), 0.6, [0.1, -0.2, 1.0, 3.0, -2.0, 4.0], 3),
    "air_spin_level": ("air", _q([1, 0.5, 0], 0.15), 0.6, [0.1, -0.2, 1.0, 0.4, -0.3, 4.0], 3),   # nearly level throughout: the lifting task ends an episode on a tilted board
}
# table spots, as signs: 0.25 m inside the table's x edge and 0.3 m inside its y edge (the tables are 1.0 to 1.5 m x 2 m: 0.74 to 0.86 m from the robot's base axis, out of
# the resting arm's reach; a slide of 0.15 m stays on the table)
SLOTS = [(1, 1), (1, -1), (-1, 1), (-1, -1)]


def start_state(M, name, slot):
    """(pos, quat, vel) of a scenario for the box of model M at table spot `slot` (signs of x and y from the table's centre)"""
    anchor, quat, gap, vel, _ = SCENARIOS[name]
    half = np.array(M.half, float)
    ext = np.abs(np.array(fr.quat_to_mat(np.array(quat, float)))[2]) @ half      # the box's half extent along z at this orientation
    cx, cy = float(M.table_center[0]), float(M.table_center[1])
    sy = float(slot[1])
    x, y, plane = cx + slot[0] * (float(M.table_half[0]) - 0.25), cy + sy * (float(M.table_half[1]) - 0.3), float(M.table_top_z)
    if anchor == "edge":
        y = cy + sy * (float(M.table_half[1]) + 0.25 * half[1])
    elif anchor == "floor":
        y, plane = cy + sy * (float(M.table_half[1]) + 0.4), float(M.floor_z)
    return [x, y, plane + ext + gap], list(map(float, quat)), list(map(float, vel))


def quat_diff(a, b):
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    return min(np.abs(a - b).max(), np.abs(a + b).max())


def diffs(a, b):
    """|a - b| per quantity of two (pos, quat, vel) states"""
    (pa, qa, va), (pb, qb, vb) = a, b
    d = lambda x, y: float(np.abs(np.asarray(x, np.longdouble) - np.asarray(y, np.longdouble)).max())  # noqa: E731
    return dict(pos=d(pa, pb), quat=float(quat_diff(qa, qb)), vel=d(va, vb))


_CACHE = {}


def reference(desc, name, slot, n_cycles, rules=fr.Rules(), n_policy=N_POLICY, **box):
    """The reference trajectory of a scenario and its floors, computed once per (model constants, scenario, slot):
    -> list over policy steps of (state in long double, {quantity: floor_solve + floor_round, the largest over the steps})"""
    M = fr.Model.from_desc(desc, np.longdouble, **box)
    key = (repr([M.h, M.gravity, M.solref, M.solimp, M.mu, M.solver_tol, M.solver_iters, M.half, M.mass, M.inertia, M.table_top_z, M.table_center, M.table_half,
                 M.floor_z]), name, slot, n_cycles, rules, n_policy)
    if key not in _CACHE:
        M64 = fr.Model.from_desc(desc, np.float64, **box)
        s0 = list(start_state(M, name, slot))
        runs = dict(ref=(M, dict(stop="kkt")), f64=(M64, dict(stop="kkt")), a0=(M, dict(stop="code", start="a0")), warm=(M, dict(stop="code", start="warm")))
        cur = {k: s0 + [None] for k in runs}
        out = []
        for _ in range(min(SCENARIOS[name][4], n_policy)):
            for k, (Mk, kw) in runs.items():
                cur[k] = list(fr.advance(Mk, *cur[k][:3], n_cycles, rules, warm=cur[k][3], return_warm=True, **kw))
            dr, da, dw = (diffs(cur[k][:3], cur["ref"][:3]) for k in ("f64", "a0", "warm"))
            out.append((tuple(cur["ref"][:3]), {q: max(da[q], dw[q]) + dr[q] for q in dr}))
        top = {q: max(f[q] for _, f in out) for q in out[0][1]}
        _CACHE[key] = [(ref, top) for ref, _ in out]
    return _CACHE[key]


def check(what, got, ref_steps, k, report=print):
    """the comparison of one env at policy step k: prints every error and floor, asserts the cap, then the bound"""
    ref, floor = ref_steps[k]
    err = diffs(got, ref)
    for q in err:
        report(f"[freebody] {what} step {k} {q}: err {err[q]:.3e} floor {floor[q]:.3e} ratio {err[q] / floor[q] if floor[q] > 0 else float('inf' if err[q] > 0 else 'nan'):.2f} cap {CAP[q]:.0e}")
    for q in err:
        assert floor[q] <= CAP[q], f"{what} step {k}: the floor of {q} ({floor[q]:.3e}) is above the cap {CAP[q]:.0e}: the scenario amplifies too much to count"
    for q in err:
        assert err[q] <= FACTOR * floor[q], f"{what} step {k}: {q} is {err[q]:.3e} from the reference, bound {FACTOR:g} x {floor[q]:.3e}"
    return err, floor


# ------------------------------------------------------------------------------------------------ kernel families
GEOM_TABLE = CONST["HRG_NRCAP"] + CONST["HRG_NHB"]   # hrg_batch_contacts: the robot's capsules, the human's bodies, then table, floor and the task's objects
GEOM_FLOOR, GEOM_OBJECT0 = GEOM_TABLE + 1, GEOM_TABLE + 2
assert GEOM_OBJECT0 == GEOM_BOX
INFO_GOAL, INFO_CRASH = CONST["HRG_INFO_N_GOAL_REACHED"], CONST["HRG_INFO_SIM_CRASH"]
AIR_AND_FLOOR = ("floor_1cm", "air_spin_level")
# family -> env id, model keywords, the box state block ("box" | "stack"), scenarios, and whether its table is the corner-against-plane test of rule 2
FAMILIES = {
    "cube": dict(env_id="PickPlaceHumanCart", kw=dict(shield_type="OFF", horizon=100, seed=5), kind="box"),
    "brick": dict(env_id="PickPlaceHumanCart", kw=dict(shield_type="OFF", horizon=100, seed=5, object_full_size=[0.04, 0.07, 0.03]), kind="box"),   # three different edges
    "cube_hull": dict(env_id="PickPlaceHumanCart", kw=dict(shield_type="OFF", horizon=100, seed=5), kind="box", desc_kw=dict(robot_geometry="hull")),
    "stacking": dict(env_id="CollaborativeStackingCart", kw=dict(shield_type="OFF", horizon=400, seed=5, done_at_success=False), kind="stack"),
    # (ours: a handover cycle runs sim.step() twice, DESIGN section 1b -- 50 substeps per policy step, so two policy steps make the 100)
    "handover": dict(env_id="HumanRobotHandoverCart", kw=dict(shield_type="OFF", horizon=400, seed=5), kind="box", substeps=2, n_policy=2),
    # the lifting board meets the table as box against slab (DESIGN D13), not corner against plane: only the floor and the air are this reference's
    "lifting": dict(env_id="CollaborativeLiftingCart", kw=dict(shield_type="OFF", horizon=400, seed=5), kind="box", scenarios=AIR_AND_FLOOR, table=False),
}


def family_batch(name, cls):
    """(batch, desc) of a family on the given batch class (oracle.OracleBatch or _lib.HipBatch); one env per scenario, stacking one per four"""
    import human_robot_gym_amd as hrg
    from human_robot_gym_amd.mixed import task_clips, task_env_kwargs
    F = FAMILIES[name]
    if F["env_id"] == "PickPlaceHumanCart":
        clips = hrg.synthetic_clips(3, seed=0, min_frames=300, max_frames=600)
    else:
        clips = task_clips(F["env_id"], 2, min_frames=3000, max_frames=3200)   # long clips: no keyframe of the task's phase machine within the compared steps
    mk = lambda: hrg.build_model_desc(dict(task_env_kwargs(F["env_id"]), **F["kw"]), n_clips=clips.n_clips, env_id=F["env_id"], **F.get("desc_kw", {}))  # noqa: E731
    names = list(F.get("scenarios", SCENARIOS))
    n = len(names) if F["kind"] == "box" else (len(names) + 3) // 4
    return cls(mk(), clips, n), mk(), names


def run_family(name, B, desc, names, report=print):
    """Set every scenario of the family into batch B, step N_POLICY policy steps on zero actions and check every env-step against the reference.
    -> {scenario: {quantity: (largest error, floor)}}"""
    F = FAMILIES[name]
    rules = fr.mutated(table=F.get("table", True))
    M = fr.Model.from_desc(desc)
    dev = getattr(B, "device", None)
    B.reset()
    where = {}   # scenario -> (env, body, slot)
    for i, nm in enumerate(names):
        if F["kind"] == "stack":
            e, c = divmod(i, 4)
            slot = SLOTS[c]
        else:
            e, c = i, 0
            tgt = np.array(B.get_box(e).target[:2])
            slot = max(SLOTS, key=lambda s: np.hypot(*(np.array(start_state(M, "drop_flat_1cm", s)[0][:2]) - tgt)))   # the spot farthest from the task's target: no delivery
        where[nm] = (e, c, slot)
    for e in range(B.n):
        ob = B.get_stack(e) if F["kind"] == "stack" else B.get_box(e)
        for nm, (e_, c, slot) in where.items():
            if e_ != e:
                continue
            pos, quat, vel = start_state(M, nm, slot)
            if F["kind"] == "stack":
                ob.pos[c][:], ob.quat[c][:], ob.vel[c][:], ob.acc_warmstart[c][:], ob.obs_pos[c][:] = pos, quat, vel, [0.0] * 6, pos
            else:
                ob.pos[:], ob.quat[:], ob.vel[:], ob.acc_warmstart[:] = pos, quat, vel, [0.0] * 6
        if F["kind"] == "stack":
            ob.weld_active[:] = [0, 0]    # the human's two cubes lie free as well
            B.set_stack(e, ob)
        else:
            ob.weld_active = 0            # handover / lifting: the object is not held (0 already for the cube tasks)
            B.set_box(e, ob)
    n_policy = F.get("n_policy", N_POLICY)
    refs = {nm: reference(desc, nm, where[nm][2], desc.n_cycles * F.get("substeps", 1), rules, n_policy) for nm in names}
    worst = {nm: {} for nm in names}
    zero = np.zeros((B.n, 7))
    for k in range(n_policy):
        B.step(B.torch.from_numpy(zero).to(dev) if dev is not None else zero)
        if dev is not None:
            B.torch.cuda.synchronize(dev)
        info, done = (x.cpu().numpy() if hasattr(x, "cpu") else np.array(x) for x in (B.info, B.done))
        pairs, ncon = B.contacts()
        for nm, (e, c, slot) in where.items():
            if k >= len(refs[nm]):
                continue
            what = f"{name}/{nm}"
            # the test's own side: the solve split (every listed contact is table | floor against an object), nothing reset or teleported the object
            listed = pairs[e, :ncon[e]]
            assert np.isin(listed[:, 0], (GEOM_TABLE, GEOM_FLOOR)).all() and (listed[:, 1] >= GEOM_OBJECT0).all(), f"{what} step {k}: contacts {listed.tolist()}"
            assert done[e] == 0 and info[e, INFO_GOAL] == 0 and info[e, INFO_CRASH] == 0, f"{what} step {k}: done {done[e]} info {info[e].tolist()}"
            ob = B.get_stack(e) if F["kind"] == "stack" else B.get_box(e)
            got = (list(ob.pos[c]), list(ob.quat[c]), list(ob.vel[c])) if F["kind"] == "stack" else (list(ob.pos), list(ob.quat), list(ob.vel))
            err, floor = check(what, got, refs[nm], k, report)
            for q in err:
                worst[nm][q] = (max(err[q], worst[nm].get(q, (0.0, 0.0))[0]), floor[q])
    return worst
