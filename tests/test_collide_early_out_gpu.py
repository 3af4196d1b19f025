"""collide's early-out inside the steppers against the oracle, which enumerates every pair and has no early-out.  -m gpu.

collide skips its pair rounds in a substep in which no robot self pair passes the broadphase, no human capsule is listed and the capsules that move are clear of table
and floor (tests/test_collide_early_out.py states the plane verdict).  Here 64 envs are moved through the state I/O to postures of three kinds -- the arm on the table,
the arm in contact with itself, the arm free -- and stepped for 3 policy steps of zero actions side by side with the oracle, in the style of
tests/test_self_cull_gpu.py::stepper_run: `ncon` and `con_pairs` equal the oracle's in every step, next to everything else the harness compares.  For ReachHuman and for
PickPlaceHumanCart, whose cube passes sit behind the skipped rounds: there every free env still lists the cube on the table.

The postures are chosen with the oracle alone: the first 2048 of tests/self_cull_ref.py's sample on an oracle batch, one step of zero actions (ReachHuman: 192 envs
then list a robot - table pair, 168 of them no other, 31 a robot - robot pair, 1849 no pair of the robot's; none lists the floor or the human), and of the first ones of each kind those that the
oracle keeps calm for 3 steps (the harness leaves an env out of a step that was violent for it, |qvel| > 5 rad/s).  28 table envs, 10 in self-contact and 26 free
ones make the 64; the counts are asserted on the oracle's own lists of the first step (at least 24, 8 and 24), and in no step may more than a quarter of a kind be
left out."""
import numpy as np
import pytest

from human_robot_gym_amd._cstruct import CONST

from self_cull_ref import NRCAP, sample
from test_self_cull_gpu import KW, place, robot_robot

pytestmark = pytest.mark.gpu

N_ENVS, N_STEPS, N_FIRST = 64, 3, 2048
N_TABLE, N_SELF, N_FREE = 28, 10, 26
GEOM_TABLE = NRCAP + CONST["HRG_NHB"]
GEOM_BOX = GEOM_TABLE + 2


def kinds_of(pairs, ncon):
    """{kind: [n] bool} of contact lists: `table` a robot capsule against the table and no robot - robot pair, `self` a robot - robot pair, `free` no pair with a robot
    capsule in it; `cube`: an object geom is listed"""
    listed = np.arange(pairs.shape[1])[None, :] < ncon[:, None]
    robot = listed & ((pairs[:, :, 0] < NRCAP) | (pairs[:, :, 1] < NRCAP))
    rr = robot_robot(pairs, ncon)
    table = (listed & (pairs[:, :, 0] < NRCAP) & (pairs[:, :, 1] == GEOM_TABLE)).any(axis=1)
    return dict(table=table & ~rr, self=rr, free=~robot.any(axis=1), cube=(listed & (pairs[:, :, 1] >= GEOM_BOX)).any(axis=1))


def oracle_batch(env_id, n):
    import human_robot_gym_amd as hrg
    from human_robot_gym_amd.mixed import task_clips, task_env_kwargs
    from oracle.oracle import OracleBatch
    clips = task_clips(env_id, 3, min_frames=300, max_frames=600)
    O = OracleBatch(hrg.build_model_desc(dict(task_env_kwargs(env_id), **KW), n_clips=clips.n_clips, env_id=env_id), clips, n, 0)
    O.reset()
    return O


def calm(O):
    """[n] bool: the last step was not violent for the env by the harness's base rule"""
    from parity import field, read_blocks
    return (np.asarray(O.info)[:, 11] == 0) & (np.abs(field(read_blocks(O, None)[0], "qvel")).max(axis=1) <= 5.0)


def postures(env_id):
    """[N_ENVS][NARM] and the kind of every row, chosen with the oracle alone"""
    q = sample(env_id)[2][:N_FIRST]
    O = oracle_batch(env_id, N_FIRST)
    place(O, q)
    O.step(np.zeros((N_FIRST, 7)))
    first = kinds_of(*O.contacts())
    O.close()
    print(f"{env_id}: of the first {N_FIRST} postures " + ", ".join(f"{int(first[k].sum())} {k}" for k in ("table", "self", "free")))
    cand = np.concatenate([np.flatnonzero(first[k])[:2 * n] for k, n in (("table", N_TABLE), ("self", N_SELF + 6), ("free", N_FREE))])
    O = oracle_batch(env_id, len(cand))
    place(O, q[cand])
    ok = np.ones(len(cand), bool)
    for _ in range(N_STEPS):
        O.step(np.zeros((len(cand), 7)))
        ok &= calm(O)
    O.close()
    pick = np.concatenate([[c for c, good in zip(cand, ok) if good and first[k][c]][:n] for k, n in (("table", N_TABLE), ("self", N_SELF), ("free", N_FREE))]).astype(int)
    assert len(pick) == N_ENVS
    return q[pick]


def stepper_run(env_id, second=None):
    """hold the second side's contact lists to the oracle's in every step (`second`: its class; the stepper on the GPU by default)"""
    from helpers import make_pair
    from parity import Run, read_blocks, write_blocks
    q = postures(env_id)
    O, G = make_pair(N_ENVS, KW, task_frames=(300, 600), env_id=env_id, second=second)
    run = Run(O, G, f"test_collide_early_out_gpu::{env_id}")
    place(O, q)
    write_blocks(G, run.kind, *read_blocks(O, run.kind))
    kinds = None
    for s in run.steps(N_STEPS, lambda k: np.zeros((N_ENVS, 7))):
        if kinds is None:
            kinds = kinds_of(s.o.pairs, s.o.ncon)
            print(f"{s.msg}: " + ", ".join(f"{int(kinds[k].sum())} {k}" for k in ("table", "self", "free", "cube")))
            assert kinds["table"].sum() >= 24 and kinds["self"].sum() >= 8 and kinds["free"].sum() >= 24
            if env_id != "ReachHuman":
                assert (kinds["cube"] & kinds["free"]).sum() >= 24, "the cube passes run behind the skipped rounds"
        for k in ("table", "self", "free"):
            out = int((kinds[k] & ~s.chk).sum())
            print(f"{s.msg}: {k}: {out} of {int(kinds[k].sum())} left out")
            assert 4 * out <= kinds[k].sum(), f"{s.msg}: {out} of {int(kinds[k].sum())} {k} envs left out of the comparison"
        s.compare()
        for what, got, want in (("ncon", s.g.ncon, s.o.ncon), ("con_pairs", s.g.pairs, s.o.pairs)):
            bad = (got != want).reshape(N_ENVS, -1).any(axis=1) & s.chk
            assert not bad.any(), f"{s.msg}: {what} differs in envs {np.flatnonzero(bad).tolist()}"
        s.resync()
    run.finish()


@pytest.mark.parametrize("env_id", ["ReachHuman", "PickPlaceHumanCart"])
def test_contact_lists_are_the_oracles(env_id):
    stepper_run(env_id)
