"""What the device-side training objects share (her.HerBuffer, rollout.RolloutBuffer, replay.ReplayBuffer, sac.SacLearner, ppo.PpoLearner): a handle of the
library on a torch device, the column check of the buffers' descriptors, and the part of the rollout and the replay buffer that is the same code in the library
(csrc/hrgym_buffer.h: the policy's view of a row, the episode tracker).  What the two learners share beyond the handle is in _learner.py."""
import ctypes

import numpy as np

from ._cstruct import CONST
from ._lib import _ptr


def check_columns(prefix, obs_cols, act_dim=None, observe_time=False, ranges=True):
    """The `obs_cols` of a buffer's descriptor as a list of ints; `prefix`: the buffer's name in the messages.  The kernels handle one value of the policy's
    observation per lane: at most HRG_OBS_DIM columns, the time column (`observe_time`) counted.  `ranges`: also refuse columns outside the superset and an
    `act_dim` outside 1 .. HRG_ACT_DIM here (otherwise that is left to the library's create call)."""
    od, ad = CONST["HRG_OBS_DIM"], CONST["HRG_ACT_DIM"]
    if ranges and act_dim is not None and not 1 <= int(act_dim) <= ad:
        raise ValueError(f"{prefix}: act_dim = {act_dim} outside 1 .. {ad}")
    cols = [int(c) for c in obs_cols]
    K = len(cols) + int(bool(observe_time))
    if not cols or K > od:
        raise NotImplementedError(f"{prefix}: an observation of {K} values{' (time column included)' if observe_time else ''} (the kernels handle one value per lane: "
                                  f"1 .. {od}, at least one of them a column)")
    if ranges and (min(cols) < 0 or max(cols) >= od):
        raise ValueError(f"{prefix}: observation columns {sorted(set(c for c in cols if not 0 <= c < od))} outside the superset")
    return cols


class DeviceHandle:
    """A handle of the library on a torch device: `h`, made by the entry point `_create` from a descriptor and released by `_destroy`.  Tensor arguments are
    checked, not converted; the calls are ordered on torch's current stream of the device."""
    _create = _destroy = None   # names of the entry points (hrg_*_create, hrg_*_destroy)

    def _open(self, desc, device, *create_args):
        """`create_args`: what the create entry takes between the descriptor and the device."""
        import torch
        from ._lib import _check, load_library
        if not torch.cuda.is_available():
            raise RuntimeError(f"{type(self).__name__} needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.torch, self.lib, self._check = torch, load_library(), _check
        self.desc = desc
        self.device = torch.device("cuda", device)
        self.h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _check(self.lib, getattr(self.lib, self._create)(ctypes.byref(desc), *create_args, device, ctypes.byref(self.h)))

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _tensor(self, x, dtype, shape, what):
        if x.dtype != dtype or x.device != self.device or not x.is_contiguous() or tuple(x.shape) != tuple(shape):
            raise ValueError(f"{what}: expected a contiguous {dtype} tensor {tuple(shape)} on {self.device}, got {x.dtype} {tuple(x.shape)} on {x.device}")
        return ctypes.c_void_p(x.data_ptr())

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            getattr(self.lib, self._destroy)(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EpisodeBuffer(DeviceHandle):
    """What RolloutBuffer and ReplayBuffer share: the policy's view of rows and of the envs' current rows, the rows an episode starts from, and the episode
    statistics.  A subclass names its entry points (`_prefix`: hrg_rollout / hrg_replay), says whether they take time values (`_has_time`: the argument is there;
    `observe_time`: the observation has the column) and how many statistics columns it keeps (`_stats_dim`), and sets `n` and `obs_dim`.  her.HerBuffer
    (`_prefix` hrg_her) takes the handle, `_call` and the episode statistics from here; its view of a row is the feature row of its own `observation`."""
    _prefix, _has_time, _stats_dim = None, False, 3 + CONST["HRG_INFO_DIM"]
    observe_time = False

    def _open(self, desc, device, info_keys=None):
        self._create, self._destroy = self._prefix + "_create", self._prefix + "_destroy"
        super()._open(desc, device)
        if info_keys is None:
            from .vec_env import INFO_KEYS
            info_keys = INFO_KEYS
        self.info_keys = list(info_keys)

    def _call(self, name, *args):
        """The entry point `name` both buffers have under their prefix, on the device and torch's current stream."""
        with self.torch.cuda.device(self.device):
            self._check(self.lib, getattr(self.lib, f"{self._prefix}_{name}")(self.h, *args, self._stream()))

    def _time(self, time, m, what):
        """The time values of `m` rows as the entry points take them: () without the argument, else (pointer or None,)."""
        if not self._has_time:
            return ()
        if not self.observe_time:
            return (None,)
        if time is None:
            raise ValueError(f"{what}: the observation has a time column; pass the rows' time values (float32 [{m}])")
        return (self._tensor(time, self.torch.float32, (m,), what),)

    def _view(self, rows, time, out):
        t = self.torch
        if rows.dim() != 2:
            raise ValueError(f"rows: expected [m, {CONST['HRG_OBS_DIM']}], got {tuple(rows.shape)}")
        m = int(rows.shape[0])
        r = self._tensor(rows, t.float32, (m, CONST["HRG_OBS_DIM"]), "rows")
        tm = self._time(time, m, "time")
        if out is None:
            out = t.empty(m, self.obs_dim, dtype=t.float32, device=self.device)
        self._call("view", r, *tm, m, self._tensor(out, t.float32, (m, self.obs_dim), "out"))
        return out

    def _observe(self, obs, time, mask):
        t = self.torch
        o = self._tensor(obs, t.float32, (self.n, CONST["HRG_OBS_DIM"]), "obs")
        tm = self._time(time, self.n, "time")
        self._call("observe", o, *tm, None if mask is None else self._tensor(mask, t.uint8, (self.n,), "mask"))

    def observation(self):
        """The policy's view of every env's current row (SB3's _last_obs): float32 [n, obs_dim]."""
        t = self.torch
        out = t.empty(self.n, self.obs_dim, dtype=t.float32, device=self.device)
        self._call("view", None, *((None,) if self._has_time else ()), self.n, _ptr(out))
        return out

    def episode_stats_per_env(self, clear=True):
        """float64 [n, _stats_dim]: finished episodes, sum of returns, sum of lengths, sums of the info columns of their last steps and, where the buffer keeps
        them, of their imitation reward sums (synchronous)."""
        acc = np.zeros((self.n, self._stats_dim), np.float64)
        self._check(self.lib, getattr(self.lib, self._prefix + "_stats")(self.h, acc.ctypes.data_as(ctypes.c_void_p), int(bool(clear))))
        return acc

    def episode_stats(self, clear=True, groups=None):
        """The episodes that finished since the last clear, summed over the envs on the host: dict(episodes, r, l, **sums of the info columns at the
        episodes' last steps, by key name) -- what safe_mean over SB3's ep_info_buffer and LoggingCallback._info_buffer divide by `episodes`; `r` is Monitor's
        return.  A buffer that keeps the imitation reward sums adds `ep_im_rew`, the sum of the infos' ep_im_rew_mean.  `groups`: a list of that many dicts
        instead, one per group of n / groups consecutive envs (a population's members).  Synchronous."""
        n_info = CONST["HRG_INFO_DIM"]
        if groups is not None and (int(groups) < 1 or self.n % int(groups)):
            raise ValueError(f"episode_stats: {self.n} envs are not {groups} groups of the same size")
        per_env = self.episode_stats_per_env(clear)
        out = []
        for tot in per_env.reshape(1 if groups is None else int(groups), -1, self._stats_dim).sum(axis=1):
            d = dict(episodes=int(tot[0]), r=float(tot[1]), l=int(tot[2]))
            d.update({k: float(v) for k, v in zip(self.info_keys, tot[3:3 + n_info])})
            if self._stats_dim > 3 + n_info:
                d["ep_im_rew"] = float(tot[3 + n_info])
            out.append(d)
        return out[0] if groups is None else out
