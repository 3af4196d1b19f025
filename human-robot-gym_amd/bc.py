"""Behaviour cloning on the device: supervised pre-training of a learner's actor on the (observation, expert action) pairs of a demonstration dataset
(dataset.ExpertDataset; tools/create_expert_dataset.py), the use SB2's `pretrain` made of one.  The cheapest baseline next to the action and the state
imitation reward, and a start for a fine-tuning run.

The table of pairs lives on the device, built once through the attached buffer's own view, so that it holds exactly what `collect_steps` / `collect_rollout`
will show the policy (the selected columns, the time column of a state imitation reward, obs_norm); the actions are at the scale the learner's actor emits.
One step is two kernel launches with no vendor BLAS and no autograd (csrc/hrgym_bc.h: the launches, the draws, what moves): rows drawn from the table, the
actor's trunk and mean head forward, mean squared error on the deterministic action, backward, Adam on the entries the loss reaches -- with moments and a
step count of the bc handle's own.  Nothing else of the learner moves: its Adam moments, counters, critics, targets, entropy coefficient, log_std, value
function.  A fine-tuning run after pre-training starts with a clean optimiser.

    env = HipVecEnv(1024, env_id="ReachHuman", obs_norm=...)
    env.attach_replay(buffer_size=1_000_000)
    learner = env.attach_sac(batch_size=128)
    table = env.demonstrations("reach-demo")             # datasets/reach-demo/hrg_dataset.npz, or a path, or an ExpertDataset
    bc = env.attach_bc(table, batch_size=128, learning_rate=1e-3)
    bc.train(2000)                                       # 2000 x two launches, nothing synchronises
    bc.diagnostics()                                     # loss of the last step, n_updates, learning_rate (synchronous)
    env.evaluate(learner, 20)                            # the pre-trained actor; then collect_steps / learner.train as before

SAC's critics are not pre-trained (the dataset holds no per-step reward): the first SAC updates after pre-training follow random critics."""
import ctypes

import numpy as np

from ._cstruct import CONST, BcDesc
from ._device import DeviceHandle
from ._learner import check_widths
from ._lib import _ptr

TILE = CONST["HRG_SAC_TILE"]
MAX_BATCH = CONST["HRG_BC_MAX_BATCH"]
KINDS = {"hrg_sac": ("sac", CONST["HRG_BC_SAC"]), "hrg_ppo": ("ppo", CONST["HRG_BC_PPO"])}   # by the learner's entry points: the table's kind, hrg_bc_desc.kind


def demonstration_rows(dataset):
    """(rows int64 [total_T], time float32 [total_T]): for every transition of `dataset`, episode after episode, the index of its observation row in
    `dataset.obs` -- rows 0 .. T_k - 1 of episode k; the terminal row has no action -- and the time value t / T_k the state imitation reward's kernels write
    into the time column (computed in double, rounded once)."""
    rows, time = np.empty(dataset.total_T, np.int64), np.empty(dataset.total_T, np.float32)
    for k in range(dataset.n_episodes):
        a, T = int(dataset.ep_offset[k]), dataset.T(k)
        rows[a:a + T] = dataset.obs_row0(k) + np.arange(T)
        time[a:a + T] = (np.arange(T, dtype=np.float64) / float(T)).astype(np.float32)
    return rows, time


def demonstration_actions(dataset, low, high, scale):
    """float32 [total_T, A]: the first A = len(low) columns of the expert's commanded actions, clipped to the action bounds; `scale`: brought to [-1, 1] by the
    bounds (SB3's scale_action: what the replay buffer stores and SAC's actor emits), otherwise left at the env's scale (what PPO's policy emits)."""
    low, high = np.asarray(low, np.float64), np.asarray(high, np.float64)
    a = np.clip(np.asarray(dataset.actions, np.float64)[:, :len(low)], low, high)
    if scale:
        a = 2.0 * ((a - low) / (high - low)) - 1.0
    return a.astype(np.float32)


class DemoTable:
    """The pairs of a demonstration dataset as a learner of `kind` ("sac" | "ppo") reads them: `observations` float32 [total_T, K], the policy's view of the
    rows, and `actions` float32 [total_T, A], both on one device (HipVecEnv.demonstrations builds it)."""

    def __init__(self, observations, actions, kind):
        if kind not in ("sac", "ppo"):
            raise ValueError(f"DemoTable: kind = {kind!r}: 'sac' or 'ppo'")
        if observations.dim() != 2 or actions.dim() != 2 or observations.shape[0] != actions.shape[0] or observations.shape[0] < 1:
            raise ValueError(f"DemoTable: observations {tuple(observations.shape)} and actions {tuple(actions.shape)} are not the rows of one table")
        self.observations, self.actions, self.kind = observations.contiguous(), actions.contiguous(), kind
        self.n_rows, self.obs_dim, self.act_dim = (int(x) for x in (observations.shape[0], observations.shape[1], actions.shape[1]))
        self.device = observations.device


def check_pair(learner, table):
    """(the table's kind, hrg_bc_desc.kind) of `learner`; the refusals of a learner and a table that do not belong together, before anything is allocated."""
    kind = KINDS.get(getattr(learner, "_prefix", None))
    if kind is None:
        raise NotImplementedError(f"behaviour cloning: {type(learner).__name__}: the kernels cover the actors of sac.SacLearner and ppo.PpoLearner")
    if int(getattr(learner, "n_members", 1)) != 1:
        raise NotImplementedError(f"behaviour cloning: {type(learner).__name__}: a population of {learner.n_members} members; behaviour cloning covers lone learners "
                                  "(pre-train member(p), or one learner, and load its parameters)")
    if table.kind != kind[0]:
        raise ValueError(f"behaviour cloning: a table of kind {table.kind!r} for a {kind[0]} learner: SAC's actions are stored at the policy's scale [-1, 1], PPO's at "
                         "the env's (build the table with the learner's buffer attached)")
    if (table.obs_dim, table.act_dim) != (learner.obs_dim, learner.act_dim):
        raise ValueError(f"behaviour cloning: the table holds observations of {table.obs_dim} and actions of {table.act_dim} values, the learner takes "
                         f"{learner.obs_dim} and {learner.act_dim}")
    return kind


class BehaviourCloning(DeviceHandle):
    """Behaviour cloning of `learner`'s actor (a lone sac.SacLearner or ppo.PpoLearner) on `table` (a DemoTable of the learner's kind and widths): it writes into
    `learner.p.params` in place, the actor's hidden layers and mean head only.  `learning_rate` is a plain attribute, passed with every step: a caller may
    schedule it.  `m`, `v`: Adam's moments of the bc steps, float32 [n_params] in the parameters' layout, the handle's own.  `step` and `train` are
    asynchronous, ordered on torch's current stream; `diagnostics` and `export` synchronise."""
    _destroy = "hrg_bc_destroy"

    def __init__(self, learner, table, batch_size=128, learning_rate=1e-3, seed=0):
        name, kind = check_pair(learner, table)
        _, _, self.batch_size = check_widths(table.obs_dim, table.act_dim, batch_size, TILE, MAX_BATCH)
        if table.device != learner.device:
            raise ValueError(f"behaviour cloning: the table lives on {table.device}, the learner on {learner.device}")
        desc = BcDesc()
        desc.kind, desc.batch_size, desc.seed = kind, self.batch_size, int(seed) & 0xFFFFFFFFFFFFFFFF
        self._create = f"hrg_bc_create_{name}"
        self._open(desc, learner.device.index, learner.h)
        self.learner, self.table, self.learning_rate = learner, table, float(learning_rate)
        self.m, self.v = self.torch.zeros_like(learner.p.params), self.torch.zeros_like(learner.p.params)
        self._keep = None

    def _sizes(self):
        w = (ctypes.c_int64 * 4)()
        self._check(self.lib, self.lib.hrg_bc_sizes(self.h, w))
        return [int(x) for x in w]

    @property
    def n_updates(self):
        """bc steps so far: the count behind Adam's bias corrections and the draws' key."""
        return self._sizes()[1]

    @property
    def n_entries(self):
        """Entries of the parameter vector a step updates."""
        return self._sizes()[0]

    def step(self, indices=None):
        """One step on `batch_size` rows of the table: drawn by the handle, or `indices` int64 [batch_size] on the device (tests; IndexError for a row outside
        the table, which reads their extremes back)."""
        t, tb, p = self.torch, self.table, self.learner.p
        if tb.n_rows == 0:   # (a dagger.DaggerTable without pinned rows, before its first step)
            raise ValueError("behaviour cloning: the table is empty (n_rows = 0): a step draws its rows from the table (env.collect_dagger fills a DaggerTable)")
        pi = None
        if indices is not None:
            pi = self._tensor(indices, t.int64, (self.batch_size,), "indices")
            lo, hi = int(indices.min()), int(indices.max())
            if lo < 0 or hi >= tb.n_rows:
                raise IndexError(f"indices: rows {lo} .. {hi} outside the table's {tb.n_rows} rows")
        with t.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_bc_step(self.h, _ptr(tb.observations), _ptr(tb.actions), tb.n_rows, pi, _ptr(p.params), _ptr(self.m), _ptr(self.v),
                                                        float(self.learning_rate), self._stream()))
        self._keep = indices

    def train(self, n_steps):
        """`n_steps` x the two launches on the handle's own draws, with no copy to the host and no synchronisation."""
        for _ in range(int(n_steps)):
            self.step()

    def export(self):
        """The last step's intermediates on the host (synchronous; tests): indices int64 [B] (the table rows), predictions float32 [B, act_dim] (the actor's
        deterministic actions), grad float32 [n_params] in the parameters' layout (zero where the loss does not reach), loss."""
        B, A = self.batch_size, self.table.act_dim
        idx, pred, grad, loss = np.zeros(B, np.int64), np.zeros((B, A), np.float32), np.zeros(self.learner.p.n_params, np.float32), np.zeros(1, np.float32)
        self._check(self.lib, self.lib.hrg_bc_export(self.h, *(a.ctypes.data_as(ctypes.c_void_p) for a in (idx, pred, grad, loss))))
        return dict(indices=idx, predictions=pred, grad=grad, loss=float(loss[0]))

    def diagnostics(self):
        """dict(loss: the last step's mean squared error, n_updates, learning_rate).  Synchronous."""
        loss = np.zeros(1, np.float32)
        self._check(self.lib, self.lib.hrg_bc_export(self.h, None, None, None, loss.ctypes.data_as(ctypes.c_void_p)))
        return dict(loss=float(loss[0]), n_updates=self.n_updates, learning_rate=self.learning_rate)
