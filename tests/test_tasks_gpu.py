"""The two task tables agree: what the C host side (csrc/hrgym_host_batch.h: HRG_TASKS) lets a batch of each task do is what the Python row
(human_robot_gym_amd/tasks.py) says.  No step is made."""
import pytest

from human_robot_gym_amd._cstruct import BoxState, HammerState, StackState
from human_robot_gym_amd._lib import HrgError
from human_robot_gym_amd.expert import EXPERT_IDS, build_expert_desc
from human_robot_gym_amd.mixed import task_clips, task_env_kwargs
from human_robot_gym_amd.tasks import TASKS, task_row
from human_robot_gym_amd.vec_env import HipVecEnv

pytestmark = pytest.mark.gpu

EXPERT_ARGS = {"CollaborativeLiftingCart": dict(signal_to_noise_ratio=1.0, board_size=[1.0, 0.4, 0.03])}   # its constructor's required arguments
CART = ([-0.1, -0.1, -0.1, -1.0], [0.1, 0.1, 0.1, 1.0])
JOINT = ([-1.0] * 7, [1.0] * 7)
BLOCK_TYPE = {None: type(None), "box": BoxState, "stack": StackState, "hammer": HammerState}


@pytest.mark.parametrize("env_id,reach_box", [(e, False) for e in sorted(TASKS)] + [("ReachHuman", True)])
def test_a_batch_of_each_task_does_what_its_row_says(env_id, reach_box):
    row = task_row(env_id, reach_box)
    # the C table has a row per HRG_TASK_*, this one a row per env_id: PickPlaceCloseHumanCart steps as HRG_TASK_PICK_PLACE, so the library would take the pick-place
    # expert where HipVecEnv, by the narrower Python row, does not (tests/test_tasks.py); for every other env_id the two sets are the same
    c_experts = {eid for t in TASKS.values() if t.task == row.task for eid in t.experts} if not reach_box else set()
    assert c_experts == set(row.experts) or env_id == "PickPlaceCloseHumanCart"
    clips = task_clips(env_id, 2, min_frames=200, max_frames=300)
    for ik in (None, dict(action_limit=0.1)):
        env = HipVecEnv(2, env_id=env_id, env_kwargs=dict(horizon=20, **task_env_kwargs(env_id)), clips=clips, ik_position_delta=ik, reach_box=reach_box)
        try:
            batch = env._backend.batch
            for eid in EXPERT_IDS:   # every HRG_EXPERT_*, in its own action form: joint for ReachHumanExpert, Cartesian for every other
                cartesian = eid != "ReachHuman"
                desc = build_expert_desc(dict(id=eid, **EXPERT_ARGS.get(eid, {})), *(CART if cartesian else JOINT))
                if eid not in c_experts:
                    with pytest.raises(HrgError, match="error -4: this expert does not read the observation of the batch's task"):
                        batch.attach_expert(desc)
                elif cartesian != (ik is not None):
                    with pytest.raises(HrgError, match=r"error -4: the expert's action form is not the batch's \(Cartesian experts need the IK front-end, ik_enabled\)"):
                        batch.attach_expert(desc)
                else:
                    batch.attach_expert(desc)
            for block, get, missing in (("stack", batch.get_stack, "not a CollaborativeStackingCart batch"), ("hammer", batch.get_hammer, "not a CollaborativeHammeringCart batch")):
                if row.block == block:
                    get(0)
                else:
                    with pytest.raises(HrgError, match="error -1: " + missing):
                        get(0)
            # the library keeps a box array for every batch (hrg_batch_get_box: zeros where the kernels stream none); which block belongs to an env's state is the row's
            batch.get_box(0)
            assert all(type(blk) is BLOCK_TYPE[row.block] for _, blk in env.get_environment_state())
        finally:
            env.close()
