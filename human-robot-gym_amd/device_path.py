"""The device training path of `HipVecEnv`: the buffers beside the stepper (her.HerBuffer, rollout.RolloutBuffer, replay.ReplayBuffer), the learners and
populations next to them, and the loops that step the envs without the host (`collect_rollout`, `collect_steps`, `collect_dagger`, `evaluate`).  `DevicePath` owns all of its
mutable state; `HipVecEnv` keeps the public methods and their docstrings and calls in here, and on the host path the HIP backend does at three points:
`after_reset`, `before_step`, `after_step`.  Nothing in here allocates pinned memory, calls torch.cuda or opens the library: with a recording batch and CPU
tensors behind the backend the whole lifecycle runs without a GPU (tests/test_device_path.py)."""
from collections import namedtuple
from importlib import import_module

import numpy as np

from ._cstruct import CONST


def _observe(path, buf):
    buf.observe(path.env._backend.batch.obs)


def _observe_timed(path, buf):
    """The rows on the device (a reset's or the last step's) become the replay buffer's current rows, with the state imitation reward's time column."""
    be, time = path.env._backend, None
    if buf.observe_time:
        time = be.batch.sir[:, CONST["HRG_SIR_TIME_OBS"]].contiguous() if path.stepped else be.reset_time_device()
    buf.observe(be.batch.obs, time=time)


def _sent_rows(path, buf, rows):
    """What the hindsight buffer stores: the rows the step left, or behind the IK front-end (which writes no info["action"]) the rows the agent sent."""
    return rows.clone() if path.env._ik is not None else rows


def _policy_scale(path, buf, rows):
    """What the replay buffer stores on the host path: the agent's own rows, brought back to the policy's scale [-1, 1] by the action bounds."""
    low, high = path.bounds
    return (2.0 * ((rows[:, :buf.act_dim] - low) / (high - low)) - 1.0).to(path.torch.float32).contiguous()


# A kind of buffer; its key in KINDS names the buffer's module and the env's descriptor builder too: _<key>_desc(n_envs, **arguments of attach).  kernels,
# goal_env, host_path: the refusals (what another backend lacks; why a goal env, and an env whose wrappers work on the host path, cannot carry it, or None);
# observe: how the buffer is handed the rows on the device; agent_rows: the action it keeps of a host-path step (None: reset() / step() do not fill it)
BufferKind = namedtuple("BufferKind", "cls kernels goal_env host_path observe agent_rows")
KINDS = {
    "her": BufferKind("HerBuffer", "add and sample", None, None, _observe, _sent_rows),
    "rollout": BufferKind("RolloutBuffer", "rollout", "goal_env: dict observations belong to the off-policy path (attach_her)",
                          "their rewards and time column live on the host path", _observe, None),
    "replay": BufferKind("ReplayBuffer", "replay", "goal_env: dict observations and relabelling belong to attach_her", None, _observe_timed, _policy_scale),
}
LEARNERS = ("sac", "sac_population", "ppo", "ppo_population")
# the table of demonstration rows (bc.DemoTable) is no buffer, but is refused as one is: it is built by an attached buffer's view kernel
DEMONSTRATIONS = BufferKind(None, "view", "goal_env: the hindsight feature row is another layout (behaviour cloning covers flat observations)", None, None, None)
TABLE_KINDS = {"sac": "replay", "ppo": "rollout"}   # the buffer whose view a learner's table is built through
# the DAgger step (dagger.Dagger) is refused as a buffer is too: it labels the rows of an attached buffer's view with the batch's scripted expert
DAGGER = BufferKind(None, "dagger", "goal_env: the scripted experts read flat observations, and the hindsight feature row is another layout (DAgger covers flat "
                    "observations)", None, None, None)
# the discriminator of adversarial imitation (adversarial.Discriminator) is refused as the table it reads is
DISCRIMINATOR = BufferKind(None, "discriminator", "goal_env: the hindsight feature row is another layout (adversarial imitation covers flat observations)", None, None, None)


def widen(rows, A, actions):
    """`actions` [n, A] into the float64 [n, HRG_ACT_DIM] rows the kernel reads."""
    rows[:, :A] = actions
    if A < CONST["HRG_ACT_DIM"]:
        rows[:, A:] = 0.0   # behind the IK front-end: [dx, dy, dz, gripper, 0, 0, 0], as step_async sends it (the step rewrites the row)


class DevicePath:
    """All mutable state of an env's device training path.  Created once per env; survives seed()."""

    def __init__(self, env):
        self.env = env
        self.buffers = {}    # kind -> the attached buffer
        self.args = {}       # kind -> the arguments it was attached with, for the new, empty buffer after seed()
        self.learners = dict.fromkeys(LEARNERS)   # env.sac, env.sac_population, env.ppo, env.ppo_population
        self.bc = None       # env.bc: the behaviour cloning of one of the lone learners (bc.BehaviourCloning)
        self.dagger = None   # env.dagger: the DAgger step and its table (dagger.Dagger)
        self.dagger_args = None   # the arguments it was attached with, for the new, empty one after seed()
        self.discriminator = None   # env.discriminator: the discriminator of adversarial imitation (adversarial.Discriminator); seed() leaves it alone, as it leaves the learners
        self.loop = False    # the name of the device loop (collect_rollout, collect_steps, collect_dagger, evaluate) that has stepped the envs past the host accounting: step_async waits for a reset()
        self.behind = False  # an evaluation stepped the envs past the attached buffers: the next device loop starts from a reset
        self.rebind()

    def on_hip(self):
        from .vec_env import _TorchBackend
        return isinstance(self.env._backend, _TorchBackend)

    def rebind(self):
        """After the env built its backend (construction, seed()): the backend calls back here, and every attached buffer is created anew, empty."""
        be, space = self.env._backend, self.env.action_space
        if self.on_hip():
            be.path, self.torch = self, be.torch
            self.bounds = tuple(be.torch.from_numpy(np.asarray(x, np.float64)).to(be.batch.device) for x in (space.low, space.high))   # (low, high), float64 on the device
        self.loop = False
        self.stepped = False   # the rows on the device are a step's (their time column: the state imitation row's), not a reset's
        for kind, args in self.args.items():
            self._create(kind, args)
        if self.dagger_args is not None:
            self._create_dagger(**self.dagger_args)

    def refusal(self, kind):
        """Why the env cannot carry a device buffer of `kind`, or None."""
        env, row = self.env, {"demonstrations": DEMONSTRATIONS, "dagger": DAGGER, "discriminator": DISCRIMINATOR}.get(kind) or KINDS[kind]
        if not self.on_hip():
            return f"the {row.kernels} kernels run in the HIP library; another backend has none"
        if env.goal_env and row.goal_env is not None:
            return row.goal_env
        if row.host_path is not None:
            if env._norm is not None:
                return "obs_norm: the normalisation runs on the host path"
            if env._dataset is not None or env._sir is not None or env._imit_alpha is not None:
                return f"a dataset or an imitation reward: {row.host_path}"
        return None

    def _create(self, kind, args):
        env, row = self.env, KINDS[kind]
        desc = getattr(env, f"_{kind}_desc")(env.num_envs, **args)
        if kind in self.buffers:
            self.buffers.pop(kind).close()
        cls = getattr(import_module("." + kind, __package__), row.cls)
        self.buffers[kind] = cls(desc, device=env._backend.batch.device.index, info_keys=env._info_keys)
        self.args[kind] = args
        return self.buffers[kind]

    def attach(self, kind, args):
        """A new, empty buffer in place of the attached one of its kind, which is closed.  Between two runs of a device loop the new buffer has no current rows,
        so the envs start again; in mid-run on the host path the next transitions start from the rows the last reset / step left on the device."""
        buf = self._create(kind, args)
        if self.loop:
            self.restart()
        elif KINDS[kind].agent_rows is not None and self.env._last_full is not None:
            KINDS[kind].observe(self, buf)
        return buf

    def restart(self):
        """The reset a device loop starts from: the envs -- to a dataset state where a dataset is attached --, and the rows handed to every attached buffer."""
        self.env._backend.reset_device()
        self.after_reset()

    def after_reset(self, host=False):
        """`host`: reset() on the host path, whose accounting is whole again; a buffer that reset() / step() do not fill waits for its loop's own reset."""
        if host:
            self.loop = False
        self.behind = self.stepped = False
        for kind, buf in self.buffers.items():
            if not host or KINDS[kind].agent_rows is not None:
                KINDS[kind].observe(self, buf)

    def before_step(self, rows):
        """`rows`: float64 [n, HRG_ACT_DIM] on the device, as the agent sent them: what each buffer keeps of them, before the kernel rewrites them."""
        self.stepped = True
        self._kept = {kind: KINDS[kind].agent_rows(self, buf, rows) for kind, buf in self.buffers.items() if KINDS[kind].agent_rows is not None}

    def after_step(self):
        """On the step's stream, ahead of the host copy: the transition never leaves the device."""
        for kind, actions in self._kept.items():
            self._add(kind, actions)

    def _add(self, kind, actions):
        """The last step's transition into the buffer.  The imitation rows go along where a reward of that kind is attached: the episode return is the env's
        own reward, the time columns are the state imitation reward's."""
        be = self.env._backend
        b = be.batch
        self.buffers[kind].add_step(actions, b.obs, b.term_obs, b.reward, b.done, b.info, **be.imitation_rows())

    def close_buffers(self):
        for buf in self.buffers.values():
            buf.close()
        self.buffers.clear()

    def attach_learner(self, slot, cls, obs_dim, rb, *args, **kwargs):
        """What every attach of a learner or population ends with: one of the buffer's action width and device, kept as `env.<slot>`; the previous one is closed."""
        learner = cls(obs_dim, rb.act_dim, *args, device=rb.device.index, **kwargs)
        if self.learners[slot] is not None:
            if self.bc is not None and self.bc.learner is self.learners[slot]:
                self.close_bc()
            self.learners[slot].close()
        self.learners[slot] = learner
        return learner

    def demonstrations(self, dataset, algorithm=None):
        """bc.DemoTable of `dataset` through the attached buffer's own view: the replay buffer's for SAC, the rollout buffer's for PPO."""
        from .bc import DemoTable, demonstration_actions, demonstration_rows
        from .dataset import ExpertDataset
        env = self.env
        why = env.device_refusal("demonstrations")
        if why is not None:
            raise NotImplementedError(f"demonstrations: {why}")
        if algorithm is not None and algorithm not in TABLE_KINDS:
            raise ValueError(f"demonstrations: algorithm = {algorithm!r}: one of {sorted(TABLE_KINDS)}")
        attached = [a for a, kind in TABLE_KINDS.items() if kind in self.buffers and algorithm in (None, a)]
        if not attached:
            need = "attach_replay(buffer_size) (SAC) or attach_rollout(n_steps) (PPO)" if algorithm is None else f"attach_{TABLE_KINDS[algorithm]}"
            raise NotImplementedError(f"demonstrations: call {need} first: the table holds the attached buffer's view of the rows, what the policy will be shown")
        if len(attached) > 1:
            raise ValueError("demonstrations: a replay and a rollout buffer are attached: pass algorithm='sac' or algorithm='ppo'")
        buf = self.buffers[TABLE_KINDS[attached[0]]]
        if not isinstance(dataset, ExpertDataset):
            dataset = ExpertDataset.load(dataset, env_id=env.env_id, has_box=env._task.block == "box")
        if dataset.env_id != env.env_id:
            raise ValueError(f"demonstrations: a dataset of {dataset.env_id}, the env steps {env.env_id}")
        if dataset.cartesian != (env._ik is not None):
            raise ValueError(f"demonstrations: the dataset's actions are {'Cartesian [dx, dy, dz, gripper]' if dataset.cartesian else 'joint space'} (cartesian = "
                             f"{dataset.cartesian}), the env's {'are' if env._ik is not None else 'are not'} (ik_position_delta)")
        if dataset.robot_geometry != env._robot_geometry:
            raise ValueError(f"demonstrations: the dataset was recorded with robot_geometry = {dataset.robot_geometry!r}, the env collides the arm as "
                             f"{env._robot_geometry!r}")
        torch = self.torch
        rows, time = demonstration_rows(dataset)
        obs = torch.from_numpy(dataset.obs[rows]).to(buf.device)
        if attached[0] == "sac":
            view = buf.view(obs, time=torch.from_numpy(time).to(buf.device) if buf.observe_time else None)
        else:
            view = buf.view(obs)
        space = env.action_space
        actions = torch.from_numpy(demonstration_actions(dataset, space.low, space.high, scale=attached[0] == "sac")).to(buf.device)
        if actions.shape[1] != buf.act_dim:
            raise ValueError(f"demonstrations: actions of {actions.shape[1]} values for a buffer of {buf.act_dim}")
        return DemoTable(view, actions, attached[0])

    def attach_bc(self, table, seed=None, **kwargs):
        """bc.BehaviourCloning of the lone learner of the table's kind, kept as `env.bc`; the previous one is closed.  `seed` None: the env's."""
        from .bc import BehaviourCloning
        slot = getattr(table, "kind", None)
        if slot not in TABLE_KINDS:
            raise ValueError(f"attach_bc: {type(table).__name__} is no table of demonstrations (env.demonstrations(dataset))")
        learner = self.learners[slot]
        if learner is None:
            if self.learners[slot + "_population"] is not None:
                raise NotImplementedError(f"attach_bc: env.{slot}_population: behaviour cloning covers lone learners, not a population (pre-train one learner and load "
                                          "its parameters into the members)")
            raise NotImplementedError(f"attach_bc: call attach_{slot} first: behaviour cloning trains the actor of the attached learner")
        bc = BehaviourCloning(learner, table, seed=int(self.env._desc.seed) if seed is None else seed, **kwargs)
        self.close_bc()
        self.bc = bc
        return bc

    def close_bc(self):
        if self.bc is not None:
            self.bc.close()
            self.bc = None

    def dagger_kind(self, name):
        """The kind ("sac" | "ppo") of the lone learner a DAgger step serves, with the buffer its view comes from attached; the refusals of `name`."""
        env = self.env
        why = env.device_refusal("dagger")
        if why is not None:
            raise NotImplementedError(f"{name}: {why}")
        if env._expert_desc is None:
            raise NotImplementedError(f"{name}: no expert: construct the env with expert=dict(id=..., ...); the labels are the scripted expert's actions")
        if env._imit_alpha is not None:
            raise NotImplementedError(f"{name}: imitation_reward: the step's own expert call would advance the expert's noise a second time, so the label and the "
                                      "reward would see different expert actions (construct the env with the expert alone)")
        populations = [slot for slot in LEARNERS if slot.endswith("_population") and self.learners[slot] is not None]
        if populations:
            raise NotImplementedError(f"{name}: env.{populations[0]}: DAgger covers lone learners, not a population (train one learner and load its parameters into "
                                      "the members)")
        lone = [slot for slot in TABLE_KINDS if self.learners[slot] is not None]
        if len(lone) != 1:
            raise NotImplementedError(f"{name}: {'no learner is' if not lone else 'a sac and a ppo learner are'} attached: DAgger serves one lone learner; call "
                                      "attach_sac (after attach_replay) or attach_ppo (after attach_rollout)")
        if TABLE_KINDS[lone[0]] not in self.buffers:
            raise NotImplementedError(f"{name}: call attach_{TABLE_KINDS[lone[0]]} first: the table holds the attached buffer's view of the rows, what the learner is shown")
        return lone[0]

    def _create_dagger(self, capacity, beta, table, seed):
        from .dagger import Dagger
        env, kind = self.env, self.dagger_kind("attach_dagger")
        buf, space = self.buffers[TABLE_KINDS[kind]], env.action_space
        new = Dagger(kind, env.num_envs, buf.obs_dim, buf.act_dim, max(int(capacity) // env.num_envs, 1), space.low, space.high, beta=beta, pinned=table,
                     seed=int(env._desc.seed) if seed is None else seed, env_id0=env._env_id0, device=buf.device.index)
        old = self.dagger
        self.close_dagger()
        if self.bc is not None and old is not None and self.bc.table is old.table:
            self.bc.table = new.table   # (the cloning goes on, on the new, empty table)
        self.dagger, self.dagger_args = new, dict(capacity=capacity, beta=beta, table=table, seed=seed)
        return new

    def attach_dagger(self, capacity, beta, table, seed):
        """dagger.Dagger for the attached lone learner, kept as `env.dagger`; the previous one is closed."""
        if table is not None and getattr(table, "kind", None) not in TABLE_KINDS:
            raise ValueError(f"attach_dagger: {type(table).__name__} is no table of demonstrations (env.demonstrations(dataset))")
        return self._create_dagger(capacity, beta, table, seed)

    def close_dagger(self):
        if self.dagger is not None:
            self.dagger.close()
            self.dagger = None

    def attach_discriminator(self, table, seed=None, **kwargs):
        """adversarial.Discriminator of `table` (a table of demonstrations, or a dataset for `demonstrations`), kept as `env.discriminator`; the previous one is closed.
        `seed` None: the env's."""
        from .adversarial import Discriminator
        why = self.env.device_refusal("discriminator")
        if why is not None:
            raise NotImplementedError(f"attach_discriminator: {why}")
        if not hasattr(table, "kind"):
            table = self.demonstrations(table, algorithm="sac" if "replay" in self.buffers else None)
        disc = Discriminator(table, seed=int(self.env._desc.seed) if seed is None else seed, **kwargs)
        self.close_discriminator()
        self.discriminator = disc
        return disc

    def close_discriminator(self):
        if self.discriminator is not None:
            self.discriminator.close()
            self.discriminator = None

    def members(self, name, n_members, seeds, kwargs):
        """What both population attaches begin with: the number of members."""
        from ._learner import check_seeds
        P = check_seeds(n_members, range(int(n_members)) if seeds is None else seeds)[0]
        if "seed" in kwargs:
            raise TypeError(f"{name}: the members' seeds are `seeds` (one per member), not `seed`")
        return P

    def member_seeds(self, P, seeds):
        return [int(self.env._desc.seed) + p for p in range(P)] if seeds is None else seeds

    def close(self):
        self.close_bc()
        self.close_dagger()
        self.close_discriminator()
        for learner in filter(None, self.learners.values()):
            learner.close()
        self.learners = dict.fromkeys(LEARNERS)
        self.close_buffers()

    def enter(self, name, account, fresh=False):
        """What collect_rollout, collect_steps, collect_dagger and evaluate share: no Monitor csv; the first call (and the first after reset() or seed()) resets the envs and
        hands the rows to the attached buffers; from then on step_async raises until reset().  `fresh`: reset whatever ran before (evaluate).  A loop that
        follows an evaluation resets too: the evaluation stepped the envs past the attached buffers, whose current rows, running returns and lengths are its
        reset's."""
        if self.env._monitor is not None:
            raise NotImplementedError(f"{name} with monitor_dir: the Monitor csv is written by the host path; {account} is the device path's account of episodes")
        if fresh or not self.loop or self.behind:
            self.restart()
            self.env._last_full = None   # (the host's copy of the rows is stale from here on)
        self.loop = name

    def _rows(self):
        return self.torch.zeros(self.env.num_envs, CONST["HRG_ACT_DIM"], dtype=self.torch.float64, device=self.env._backend.batch.device)

    def _step(self, rows):
        self.env._backend.launch_step(rows)
        self.stepped = True

    def collect_rollout(self, policy, value_fn):
        rb = self.buffers.get("rollout")
        if rb is None:
            raise NotImplementedError("collect_rollout: call attach_rollout(n_steps, gamma, gae_lambda) first")
        self.enter("collect_rollout", "env.rollout.episode_stats()")
        torch, space, b = self.torch, self.env.action_space, self.env._backend.batch
        rb.reset()
        low, high = torch.from_numpy(space.low).to(b.device), torch.from_numpy(space.high).to(b.device)
        rows = self._rows()
        for _ in range(rb.n_steps):
            actions, values, log_probs = policy(rb.observation())
            widen(rows, rb.act_dim, torch.clamp(actions, low, high))   # SB3 clips what the env gets, not what the buffer stores
            self._step(rows)
            terminal_values = value_fn(rb.view(b.term_obs))
            rb.add_step(actions, values, log_probs, terminal_values, b.obs, b.term_obs, b.reward, b.done, b.info)
        rb.compute_returns_and_advantage(value_fn(rb.observation()))
        return rb

    def collect_steps(self, policy, n_steps):
        kind = "her" if "her" in self.buffers else "replay"
        rb = self.buffers.get(kind)
        if rb is None:
            raise NotImplementedError("collect_steps: call attach_replay(buffer_size) first, or attach_her(buffer_size) on a goal env")
        self.enter("collect_steps", f"env.{kind}.episode_stats()")
        low, high = self.bounds
        rows = self._rows()
        for _ in range(int(n_steps)):
            actions = policy(rb.observation())
            widen(rows, rb.act_dim, low + 0.5 * (actions.to(self.torch.float64) + 1.0) * (high - low))   # SB3's unscale_action
            kept = actions if kind == "replay" else _sent_rows(self, rb, rows)   # the policy's own action | what reset() / step() hand the hindsight buffer
            self._step(rows)
            self._add(kind, kept)
        return rb

    def collect_dagger(self, n_steps, deterministic):
        dg = self.dagger
        if dg is None:
            raise NotImplementedError("collect_dagger: call attach_dagger(capacity) first")
        kind = self.dagger_kind("collect_dagger")
        if kind != dg.table.kind:
            raise NotImplementedError(f"collect_dagger: env.dagger was attached for a {dg.table.kind} learner, the attached learner is a {kind} one: call attach_dagger again")
        learner, buf, on_policy = self.learners[kind], self.buffers[TABLE_KINDS[kind]], kind == "ppo"
        if on_policy and self.loop == "collect_dagger":
            self.behind = False   # (the last collect_dagger kept the rollout buffer's current rows in step: this one continues)
        self.enter("collect_dagger", "env.dagger.stats()")
        b = self.env._backend.batch
        rows = self._rows()
        kept = None if on_policy else self.torch.empty(buf.n, buf.act_dim, dtype=self.torch.float32, device=b.device)
        for _ in range(int(n_steps)):
            view = buf.observation()
            actions = learner.policy(view, deterministic)[0] if on_policy else learner.act(view, deterministic)
            dg.step(view, actions, b.expert_actions(), rows, kept)
            self._step(rows)
            if on_policy:
                buf.observe(b.obs)   # a mixture policy is not on-policy: no slot is written; the current rows follow the envs
            else:
                self._add("replay", kept)
        if on_policy:
            self.behind = True   # the rollout buffer's episode flags and running returns did not see these steps: collect_rollout starts from a reset
        return dg

    def evaluate(self, learner, params, n_eval_episodes, sync_every):
        from .evaluation import Evaluator
        env = self.env
        desc = env._eval_desc(env.num_envs, 1 if params is None else int(params.shape[0]), n_eval_episodes)
        self.enter("evaluate", "the EvalResult it returns", fresh=True)   # evaluate_policy starts from env.reset()
        self.behind = True
        be = env._backend
        b = be.batch
        ev = Evaluator(desc, device=b.device.index, info_keys=env._info_keys)
        try:
            ev.begin(b.obs, be.reset_time_device() if env._observe_time else None)
            bound, missing = ev.max_quota * env.horizon + sync_every, -1
            for step in range(1, bound + 1):
                self._step(ev.policy(learner, params))
                ev.step(b.obs, b.reward, b.done, b.info, **be.imitation_rows())
                if step % sync_every == 0 or step == bound:
                    missing = ev.remaining()
                    if missing == 0:
                        break
            if missing:
                raise RuntimeError(f"evaluate: {missing} episodes missing after {bound} steps (horizon {env.horizon}): an episode outlived the time limit")
            return ev.result()
        finally:
            ev.close()
