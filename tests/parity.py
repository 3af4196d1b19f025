"""The oracle <-> HIP side-by-side loop, written once (DESIGN.md section 2 states the rules).

Two batches of the same model are stepped on the same actions.  `info`, `done`, the contact pairs and every integer of the state blocks must agree bit for bit; `obs`,
`reward`, `term_obs` and every float of the state blocks to 1e-5 relative (helpers.assert_state_close, with its knife edges of representations).  The harness owns the
loop and the rules; a test supplies its scenario and its own counters:

    run = Run(O, G, name=..., free_running=False)      # resets both sides and compares the reset obs, state and object blocks
    for s in run.steps(n_steps, actions):              # actions(k) -> [n, 7]: may edit both batches first (the scenario); then both sides step
        s.chk &= ~my_exclusion(s)                      # optional
        s.drop_flicker()                               # optional: only where a contact list that differs at agreeing floats is tolerated
        s.compare()                                    # everything, over s.chk
        s.resync()                                     # optional, or every k-th step
    run.finish(min_live=0.9)                           # record_live + close

Nothing here knows which side runs on the GPU: a side gets its actions as a device tensor if it keeps its buffers on a device, and every output goes through to_numpy."""
import numpy as np

from human_robot_gym_amd._cstruct import CONST, BoxState, EnvState, HammerState, StackState
from helpers import ATOL, RTOL, assert_state_close, record_live, states_as_bytes

GEOM_BOX = CONST["HRG_NRCAP"] + CONST["HRG_NHB"] + 2    # first object geom: after the robot capsules, the human bodies, table and floor

# The object block that rides next to hrg_env_state, per kind: its struct, per-env getter / setter, the keyword of OracleBatch.set_states_all, the fields of its flat
# pose vector (flicker rule) and the linear speed above which a free body makes the env violent (None: the stacking rule, 3 m/s while the cube touches something).
KINDS = {"box": dict(struct=BoxState, get="get_box", set="set_box", bulk="bx", pose=("pos", "quat"), speed=5.0),
         "stack": dict(struct=StackState, get="get_stack", set="set_stack", bulk="sk", pose=("pos", "quat"), speed=None),
         "hammer": dict(struct=HammerState, get="get_hammer", set="set_hammer", bulk="hm", pose=("pos", "quat", "nail_q"), speed=3.0)}


def kind_of(desc):
    """which object block a model streams next to hrg_env_state: a fact about desc.task"""
    return {CONST["HRG_TASK_REACH"]: None, CONST["HRG_TASK_STACKING"]: "stack", CONST["HRG_TASK_HAMMERING"]: "hammer"}.get(desc.task, "box")


def to_numpy(x):
    return x.cpu().numpy().copy() if hasattr(x, "cpu") else np.array(x)


def read_blocks(B, kind):
    """(EnvState[n], object block [n] | None) of every env of a batch, through the bulk getters where the batch has them"""
    if hasattr(B, "get_states_all"):
        r = B.get_states_all(**({kind: True} if kind else {}))
        return r[0], next((x for x in r[1:] if x is not None), None)
    st, bx = B.get_states(np.arange(B.n, dtype=np.int32))
    if kind in (None, "box"):
        return st, (bx if kind else None)
    K = KINDS[kind]
    return st, (K["struct"] * B.n)(*[getattr(B, K["get"])(e) for e in range(B.n)])


def write_blocks(B, kind, st, ob):
    if hasattr(B, "set_states_all"):
        return B.set_states_all(st, **({KINDS[kind]["bulk"]: ob} if kind else {}))
    B.set_states(np.arange(B.n, dtype=np.int32), st, ob if kind == "box" else None)
    if kind not in (None, "box"):
        for e in range(B.n):
            getattr(B, KINDS[kind]["set"])(e, ob[e])


def field(arr, name):
    """one float field of every struct of a ctypes array: [n, doubles]"""
    f = getattr(arr._type_, name)
    return np.ascontiguousarray(states_as_bytes(arr)[:, f.offset:f.offset + f.size]).view(np.float64)


def state_doubles(st):
    """every double of every env state (they come first, up to `timestep`): [n, nd]"""
    return np.ascontiguousarray(states_as_bytes(st)[:, :EnvState.timestep.offset]).view(np.float64)


def pose_vectors(kind, ob):
    """the flat pose vector of every env's object block: [n, m] ([n, 0] without one)"""
    return np.concatenate([field(ob, f) for f in KINDS[kind]["pose"]], axis=1) if kind else np.zeros((len(ob or ()), 0))


def object_speeds(ob):
    """largest linear velocity component of every free body: [n, bodies]"""
    return np.abs(field(ob, "vel").reshape(len(ob), -1, 6)[:, :, :3]).max(axis=2)


def floats_agree(so, sg, po, pg, tol=1e-7):
    """The flicker predicate, per env: every double of the env state and the object's pose vector agree to `tol` absolute plus `tol` relative.  A contact list that
    differs may leave a comparison only where this holds: a resting contact that carries no load sits AT distance zero, so whether it is listed is decided by
    rounding-level differences -- and a wrong contact moves something."""
    ok = np.all(np.abs(so - sg) <= tol + tol * np.abs(so), axis=1)
    return ok & np.all(np.abs(po - pg) <= tol + tol * np.abs(po), axis=1) if po.shape[1] else ok


class Side:
    """what one batch reported for one step"""

    def __init__(self, B, kind, sent):
        self.obs, self.reward, self.done, self.info, self.term_obs = (to_numpy(x) for x in (B.obs, B.reward, B.done, B.info, B.term_obs))
        self.pairs, self.ncon = B.contacts()
        self.states, self.objects = read_blocks(B, kind)
        self.executed = to_numpy(getattr(B, "last_actions", sent))   # (a batch with wrappers rewrites the rows it was given with the executed joint actions)


class Step:
    """One policy step of both sides: `o` / `g` (Side), the oracle's state before it (`pre_states`, `pre_objects`), `violent`, and `chk`: the envs compare() looks at."""

    def __init__(self, run, k, a, pre, o, g):
        self.run, self.k, self.a, self.o, self.g = run, k, a, o, g
        self.pre_states, self.pre_objects = pre
        self.msg = f"{run.name} step {k}"
        self.violent = run._violent(self)
        if run.free_running:
            run.live &= ~self.violent
        self.chk = run.live & ~self.violent
        self.contacts_differ = (o.ncon != g.ncon) | (o.pairs != g.pairs).any((1, 2))

    def drop_flicker(self, measure="state"):
        """Take the envs whose contact lists differ out of this step's comparison (free-running: for good), counted in run.flicker -- only while their floats agree
        (floats_agree); otherwise an assertion failure.  measure="pose": the object's pose vector alone, to 1e-7 absolute."""
        run = self.run
        so, sg = state_doubles(self.o.states), state_doubles(self.g.states)
        po, pg = pose_vectors(run.kind, self.o.objects), pose_vectors(run.kind, self.g.objects)
        agree = floats_agree(so, sg, po, pg) if measure == "state" else np.abs(po - pg).max(axis=1) < 1e-7
        for e in np.nonzero(self.chk & self.contacts_differ)[0]:
            worst = max(np.abs(so[e] - sg[e]).max() if measure == "state" else 0.0, np.abs(po[e] - pg[e]).max() if po.shape[1] else 0.0)
            assert agree[e], f"{self.msg} env {e}: contact lists differ and so do the floats of the state ({worst:.2e})"
            self.chk[e] = False
            run.flicker += 1
            if run.free_running:
                run.live[e] = False
                run.dropped_flicker += 1

    def _rows(self, what, got, want, atol=None):
        """rows of self.chk: bit-exact (atol None) or within RTOL / atol; the message names the first env that differs"""
        got, want = got.reshape(len(got), -1), want.reshape(len(want), -1)
        bad = (got != want) if atol is None else ~(np.abs(got.astype(np.float64) - want) <= atol + RTOL * np.abs(want.astype(np.float64)))
        rows = np.nonzero(self.chk & bad.any(axis=1))[0]
        if rows.size:
            e = int(rows[0])
            c = int(np.nonzero(bad[e])[0][0])
            raise AssertionError(f"{self.msg} env {e}: {what}[{c}] differs: oracle {want[e, c]!r} hip {got[e, c]!r} ({rows.size} envs: {rows[:8].tolist()})")

    def compare(self, skip=()):
        """Everything, over self.chk.  `skip`: names out of info, done, contacts, obs, reward, term_obs, state (a check switched off states at the call what was observed)."""
        run, o, g = self.run, self.o, self.g
        assert set(skip) <= {"info", "done", "contacts", "obs", "reward", "term_obs", "state"}, skip
        for what, got, want, atol in (("info", g.info, o.info, None), ("done", g.done, o.done, None), ("ncon", g.ncon, o.ncon, None), ("contacts", g.pairs, o.pairs, None),
                                      ("obs", g.obs, o.obs, run.atol), ("reward", g.reward, o.reward, run.reward_atol), ("term_obs", g.term_obs, o.term_obs, run.atol)):
            if ("contacts" if what == "ncon" else what) not in skip:
                self._rows(what, got, want, atol)
        if run.actions == "exact":
            self._rows("executed action", g.executed, o.executed)
        elif run.actions is not None:
            rtol, atol = run.actions
            np.testing.assert_allclose(g.executed[self.chk], o.executed[self.chk], rtol=rtol, atol=atol, err_msg=f"{self.msg}: executed actions")
        if "state" not in skip:
            for e in np.nonzero(self.chk)[0]:
                assert_state_close(o.states[e], g.states[e], f"{self.msg} env {e}")
                if run.kind:
                    assert_state_close(o.objects[e], g.objects[e], f"{self.msg} env {e} {run.kind}")
        run.compared += int(self.chk.sum())

    def resync(self):
        """the second side continues from the oracle's state"""
        write_blocks(self.run.G, self.run.kind, self.o.states, self.o.objects)


class Run:
    """violent: which envs leave a step as chaotic (free-running: for good).  "base": a simulation crash (info[:, 11]) or |qvel| > 5 rad/s after the step;
    "base+pre": or before it; "base+object" (default): or a free body of the object block too fast (KINDS: a cube above 5 m/s, a hammer or board above 3 m/s, a stacking
    cube above 3 m/s while it touches something); None: no env ever leaves.
    atol / reward_atol: absolute tolerance of obs and term_obs / of reward, next to RTOL.  actions: compare the executed action rows, "exact" or (rtol, atol)."""

    def __init__(self, O, G, name, free_running=False, desc=None, violent="base+object", atol=1e-6, reward_atol=1e-6, actions=None):
        assert violent in (None, "base", "base+pre", "base+object")
        self.O, self.G, self.name, self.free_running, self.violent, self.atol, self.reward_atol, self.actions = O, G, name, free_running, violent, atol, reward_atol, actions
        self.kind = kind_of(desc or O.desc)
        self.n = O.n
        self.live = np.ones(self.n, bool)
        self.flicker = self.dropped_flicker = self.compared = 0
        oo, og = to_numpy(O.reset()), to_numpy(G.reset())
        np.testing.assert_allclose(og, oo, rtol=RTOL, atol=ATOL, err_msg=f"{name} reset obs")
        (so, bo), (sg, bg) = read_blocks(O, self.kind), read_blocks(G, self.kind)
        for e in range(self.n):
            assert_state_close(so[e], sg[e], f"{name} reset env {e}")
            if self.kind:
                assert_state_close(bo[e], bg[e], f"{name} reset env {e} {self.kind}")

    def _send(self, B, a):
        """this side's own copy of the action rows, on the device where the batch keeps its buffers there"""
        a = np.array(a, dtype=np.float64, order="C")
        return B.torch.from_numpy(a).to(B.device) if hasattr(B, "device") else a

    def _violent(self, s):
        n = self.n
        if self.violent is None:
            return np.zeros(n, bool)
        v = (s.o.info[:, 11] != 0) | (np.abs(field(s.o.states, "qvel")).max(axis=1) > 5.0)
        if self.violent == "base+pre":
            v |= np.abs(field(s.pre_states, "qvel")).max(axis=1) > 5.0
        if self.violent == "base+object" and self.kind:
            fast = object_speeds(s.o.objects) > (KINDS[self.kind]["speed"] or 3.0)
            if self.kind == "stack":
                listed = np.arange(s.o.pairs.shape[1])[None, :] < s.o.ncon[:, None]
                fast &= np.stack([(listed & (s.o.pairs == GEOM_BOX + c).any(axis=2)).any(axis=1) for c in range(fast.shape[1])], axis=1)
            v |= fast.any(axis=1)
        return v

    def steps(self, n_steps, actions):
        O, G = self.O, self.G
        for k in range(n_steps):
            a = np.ascontiguousarray(actions(k), np.float64)
            pre = read_blocks(O, self.kind)
            sent = [self._send(B, a) for B in (O, G)]
            for B, x in zip((O, G), sent):
                B.step(x)
            for B in (O, G):
                if hasattr(B, "device"):
                    B.torch.cuda.synchronize(B.device)
            self.last = Step(self, k, a, pre, Side(O, self.kind, sent[0]), Side(G, self.kind, sent[1]))
            yield self.last

    def drops(self):
        """the two kinds of free-running drops, apart"""
        return dict(dropped_contact_list_flicker=self.dropped_flicker, dropped_violent=int(self.n - self.live.sum()) - self.dropped_flicker)

    def finish(self, min_live=None, **extra):
        """with a floor: the live fraction is printed, logged and asserted (helpers.record_live); both batches are closed"""
        try:
            if min_live is not None:
                record_live(self.name, self.live, min_live, **extra)
        finally:
            self.O.close(); self.G.close()
