"""The parity harness (tests/parity.py) against itself: a second OracleBatch stands where the HIP batch stands in the GPU tests.  Identical sides pass; a thin wrapper
that alters what the second side reports at one step and env must be caught, with that step and env in the message; the flicker and violent rules do what
DESIGN.md section 2 says."""
import json

import numpy as np
import pytest

import helpers
from helpers import make_pair
from parity import KINDS, Run

TASKS = ["ReachHuman", "PickPlaceHumanCart", "CollaborativeStackingCart", "CollaborativeHammeringCart"]   # one per kind: None, box, stack, hammer
N, STEP, ENV = 8, 2, 5


class Altered:
    """the second oracle, reporting `what` wrongly for env ENV after its step number STEP"""

    def __init__(self, B, what):
        self.B, self.what, self.k = B, what, -1

    def __getattr__(self, name):
        return getattr(self.B, name)

    def step(self, a):
        self.k += 1
        out = self.B.step(a)
        if self.k == STEP and self.what == "info":
            self.B.info[ENV, 0] += 1
        if self.k == STEP and self.what == "done":
            self.B.done[ENV] ^= 1
        if self.k == STEP and self.what == "obs":
            self.B.obs[ENV, np.argmax(np.abs(self.B.obs[ENV]))] *= 1 + 1e-4
        return out

    def contacts(self):
        pairs, ncon = self.B.contacts()
        if self.k == STEP and self.what in ("contacts", "contacts+qpos"):
            ncon[ENV] += 1
        return pairs, ncon

    def get_states_all(self, **kw):
        r = self.B.get_states_all(**kw)
        if self.k == STEP and self.what in ("qpos", "contacts+qpos"):
            r[0][ENV].qpos[2] += 1e-4
        if self.k == STEP and self.what == "pose":
            ob = next(x for x in r[1:] if x is not None)
            pos = ob[ENV].pos
            (pos if isinstance(pos[0], float) else pos[1])[0] += 1e-4
        return r


def _pair(env_id, what=None, seed=3):
    from oracle.oracle import OracleBatch
    O, G = make_pair(N, dict(shield_type="SSM", horizon=15, seed=seed), task_frames=(300, 420), env_id=env_id, second=OracleBatch)
    if what:
        desc, G = G.desc, Altered(G, what)
        G.desc = desc
    return O, G


def _run(run, n_steps, flicker=False, body=None):
    rng = np.random.RandomState(1)
    for s in run.steps(n_steps, lambda k: rng.uniform(-0.3, 0.3, (N, 7))):
        if body:
            body(s)
        if flicker:
            s.drop_flicker()
        s.compare()
        if not run.free_running:
            s.resync()


@pytest.fixture
def lines(monkeypatch):
    """what record_live hands to the log's writer, kept here instead"""
    got = []
    monkeypatch.setattr(helpers, "append_live_line", got.append)
    return got


def test_a_live_line_reaches_the_log():
    line = dict(test="test_parity_harness::log", live=1.0, n=N, floor=0.5)
    path = helpers.append_live_line(line)
    if path is not None:     # (a tree that cannot be written to keeps no log)
        with open(path) as f:
            assert json.loads(f.readlines()[-1]) == line


@pytest.mark.parametrize("free_running", [False, True])
@pytest.mark.parametrize("env_id", TASKS)
def test_identical_sides_pass(env_id, free_running, lines):
    run = Run(*_pair(env_id), name=f"test_parity_harness::{env_id}{'_free' if free_running else ''}", free_running=free_running)
    violent = []
    _run(run, 12, flicker=True, body=lambda s: violent.append(s.violent.any()))
    assert run.flicker == 0 and run.compared > 0
    assert run.live.all() or any(violent)
    assert run.compared == N * 12 or any(violent)
    run.finish(min_live=0.5)
    line, = lines
    assert line["test"] == run.name and line["n"] == N and line["floor"] == 0.5 and line["live"] == float(run.live.mean())


@pytest.mark.parametrize("env_id,what", [(e, "qpos") for e in TASKS] + [(e, "pose") for e in TASKS[1:]] +     # (ReachHuman has no object block)
                         list(zip(TASKS, ("info", "done", "obs", "contacts+qpos"))))
def test_an_altered_report_is_caught_with_its_step_and_env(env_id, what):
    run = Run(*_pair(env_id, what), name="altered", violent=None)
    with pytest.raises(AssertionError, match=f"step {STEP} env {ENV}"):
        _run(run, STEP + 2, flicker=what.startswith("contacts"))
    assert run.last.k == STEP
    run.finish()


@pytest.mark.parametrize("env_id", ["CollaborativeStackingCart", "CollaborativeHammeringCart"])
def test_flicker_is_excluded_and_counted_only_where_a_test_tolerates_it(env_id):
    run = Run(*_pair(env_id, "contacts"), name="flicker", violent=None)
    _run(run, STEP + 2, flicker=True)
    assert run.flicker == 1 and run.compared == N * (STEP + 2) - 1 and run.live.all()     # resynchronised: out for that step only
    run.finish()
    run = Run(*_pair(env_id, "contacts"), name="no_flicker", violent=None)
    with pytest.raises(AssertionError, match=f"step {STEP} env {ENV}"):
        _run(run, STEP + 2, flicker=False)
    run.finish()


def test_flicker_drops_a_free_running_stacking_env_for_good(lines):
    run = Run(*_pair("CollaborativeStackingCart", "contacts"), name="test_parity_harness::stacking_flicker_free", free_running=True, violent=None)
    _run(run, STEP + 3, flicker=True)
    assert run.flicker == 1 and not run.live[ENV] and run.live.sum() == N - 1
    assert run.compared == N * (STEP + 3) - 3
    assert run.drops() == dict(dropped_contact_list_flicker=1, dropped_violent=0)
    run.finish(min_live=0.8, **run.drops())
    assert lines[-1]["dropped_contact_list_flicker"] == 1 and lines[-1]["live"] == (N - 1) / N


def _spin(Bs, k):
    """env ENV's first joint at 6 rad/s on both sides before step STEP"""
    if k == STEP:
        for B in Bs:
            st = B.get_state(ENV)
            st.qvel[0] = 6.0
            B.set_state(ENV, st)


@pytest.mark.parametrize("free_running", [False, True])
def test_a_violent_env_leaves_the_step_or_the_run(free_running, lines):
    O, G = _pair("ReachHuman")
    run = Run(O, G, name="test_parity_harness::violent" + ("_free" if free_running else ""), free_running=free_running, violent="base+pre")
    rng = np.random.RandomState(1)
    out = []

    def actions(k):
        _spin((O, G), k)
        return rng.uniform(-0.3, 0.3, (N, 7))
    for s in run.steps(STEP + 3, actions):
        out.append(~s.chk)
        s.compare()
        if not free_running:
            s.resync()
    out = np.array(out)
    assert out[STEP, ENV] and not out[:STEP].any() and not np.delete(out, ENV, axis=1).any()
    if free_running:
        assert out[STEP:, ENV].all() and run.live.sum() == N - 1
        with pytest.raises(AssertionError, match="live fraction"):
            run.finish(min_live=0.9)          # 7 of 8
    else:
        assert not out[-1, ENV] and run.live.all()
        run.finish(min_live=1.0)


def test_the_object_kind_is_a_fact_about_the_task():
    import human_robot_gym_amd as hrg
    from parity import kind_of
    kinds = {e: kind_of(hrg.build_model_desc(None, env_id=e)) for e in TASKS + ["CollaborativeLiftingCart", "HumanRobotHandoverCart", "HumanObjectInspectionCart"]}
    assert [kinds[e] for e in TASKS] == [None, "box", "stack", "hammer"] and set(list(kinds.values())[4:]) == {"box"}
    assert kind_of(hrg.build_model_desc(None, reach_box=True)) == "box" and set(KINDS) == {"box", "stack", "hammer"}
