"""Thin ctypes binding of libhrgym_hip.so (include/hrgym.h) + `HipBatch`, a tensor-level handle.

There is NO CPU fallback: if the HIP library is missing or the GPU is unavailable this module raises.
PyTorch-ROCm is used only to own device buffers / streams (plumbing); all compute is in the HIP library.
"""
import ctypes
import glob
import os
import subprocess

from ._cstruct import CONST, PROTOTYPES, EnvState, BoxState, StackState, HammerState, ModelDesc, ClipTable, ExpertDesc, DatasetDesc, HerDesc, RolloutDesc, ReplayDesc, SacDesc, PpoDesc  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhrgym_hip.so")   # the one shipping library; no environment variable redirects it
_variant = None   # tuning experiments only: set through use_variant_library(), reported by bench.py as "variant_lib"
SRC = os.path.join(_HERE, "csrc", "hrgym_hip.hip")
# SRC is the base unit (the ReachHuman kernels); every other unit is the same sources compiled with a task's additions: the manipulation object (box), the
# object <-> hand weld (handover), the connect equalities of the lifting task, the four cubes (stack), board + nail + hammer; *_hulls: the same kernels with the
# arm links' convex hulls as collision geometry (hull - cube pairs by MPR)
SOURCES = [os.path.join(_HERE, "csrc", f"hrgym_{unit}.hip") for unit in (
    "hip", "box", "handover", "lift", "stack", "hammer", "hulls", "box_hulls", "handover_hulls", "lift_hulls", "stack_hulls", "hammer_hulls")]
SRC_BOX_HULLS = SOURCES[7]   # the one unit a test looks up by name (tests/test_hull_box.py)
EXPORTS = list(PROTOTYPES)   # every function include/hrgym.h declares


def library_dependencies():
    """Every file the library is compiled from: the translation units and every header under csrc/ and include/, as the directories hold them."""
    return SOURCES + sorted(glob.glob(os.path.join(_HERE, "csrc", "*.h")) + glob.glob(os.path.join(os.path.dirname(_HERE), "include", "*.h")))


def build_library(force=False, verbose=False):
    """Compile the HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(d) for d in library_dependencies()):
        return LIB_PATH
    # -fapprox-func, device code only: FP64 divisions become v_rcp_f64 + two Newton steps + one residual correction (8 instructions, within an ulp) instead of the
    # IEEE-exact sequence with scaling and fix-up (12+): 140 division sites in the ReachHuman kernel alone, 5 % of its vector instructions.  The host side and the
    # oracle keep IEEE arithmetic; the parity tolerance (1e-5 relative) is eleven orders of magnitude above the difference.
    # -mllvm -disable-machine-licm: the machine-level loop-invariant code motion pulled the materialisation of ~25 FP64 literals (polynomial coefficients of the
    # in-loop sincos / atan / exp code) out of the 25-cycle loop into VGPR pairs that then stayed live across EVERY phase -- a fifth of the 128-register budget, one
    # pair spilled.  Without it the ReachHuman kernel allocates 120 VGPRs with no VGPR spill (was 128 + 5 spilled; SGPR spills 93 -> 64) and every variant is
    # 3 - 6 % faster (profiles/r03_*).
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value", "-Xarch_device", "-fapprox-func", "-mllvm", "-disable-machine-licm", "-o", LIB_PATH,
           *SOURCES]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None


def use_variant_library(path):
    """Tuning experiments only (tools/): load another build of the library instead of the shipping one.  Must be called before the first
    batch is created; `variant_library()` tells callers (bench.py echoes it in its JSON line) that results are not the shipping build's."""
    global _variant
    if _lib is not None:
        raise RuntimeError("use_variant_library() must be called before the library is loaded")
    _variant = os.path.abspath(path)


def variant_library():
    return _variant


def load_library():
    """dlopen the HIP library and declare signatures. Raises if it is missing (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    for var in ("HRG_LIB_PATH", "HRG_PHASE_MASK"):   # round-1 tuning switches: a stale variable must not change what runs
        if os.environ.get(var):
            raise RuntimeError(f"{var} is set: the library no longer honours it (use _lib.use_variant_library() / a -DHRG_STAMPS diagnostic build); unset it")
    path = _variant or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
                           "There is no CPU fallback for the stepper.")
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in PROTOTYPES.items():   # the signatures are the header's own (_cstruct.parse_prototypes)
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.hrg_state_bytes() != ctypes.sizeof(EnvState):
        raise RuntimeError("hrg_env_state layout mismatch between header mirror and library: rebuild")
    _lib = lib
    return lib


class HrgError(RuntimeError):
    pass


def _check(lib, rc):
    if rc != 0:
        raise HrgError(f"hrgym error {rc}: {lib.hrg_last_error().decode()}")


def _coerce(x, dtype, device):
    """`x` itself when it already is a contiguous `dtype` tensor on `device`, otherwise a converted copy (which the caller keeps alive until the kernel
    has read it)."""
    if x.dtype != dtype or x.device != device or not x.is_contiguous():
        x = x.to(device=device, dtype=dtype).contiguous()
    return x


def as_actions(actions, n, device):
    """Actions as the kernels read them: float64 [n, HRG_ACT_DIM], contiguous, on `device`."""
    import torch
    actions = _coerce(actions, torch.float64, device)
    if tuple(actions.shape) != (n, CONST["HRG_ACT_DIM"]):
        raise ValueError(f"actions must be [{n}, {CONST['HRG_ACT_DIM']}]")
    return actions


def as_obs(obs, n, device):
    """Rows of the observation superset: float32 [n, HRG_OBS_DIM], contiguous, on `device`."""
    import torch
    obs = _coerce(obs, torch.float32, device)
    if tuple(obs.shape) != (n, CONST["HRG_OBS_DIM"]):
        raise ValueError(f"obs must be [{n}, {CONST['HRG_OBS_DIM']}]")
    return obs


def as_mask(mask, device):
    """A reset mask: uint8, contiguous, on `device` (None: every env)."""
    import torch
    return None if mask is None else _coerce(mask, torch.uint8, device)


def _ptr(x):
    return None if x is None else ctypes.c_void_p(x.data_ptr())


class HipBatch:
    """n_envs ReachHuman environments resident on one MI355X.

    All I/O buffers are torch tensors on the batch's device; `step` is asynchronous (ordered on torch's
    current stream of that device)."""

    def __init__(self, desc, clips, n_envs, env_id0=0, device=0, out=None):
        """`out`: optional (obs, term_obs, reward, info, done) device tensors to write into — row slices of a larger block that several
        batches share (mixed.MixedBatch); by default the batch allocates its own packed block."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("HipBatch needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.torch = torch
        self.lib = load_library()
        self.n = int(n_envs)
        self.device = torch.device("cuda", device)
        self._clips = clips  # keep host frame table alive during create
        table = clips.table()
        if desc.n_clips != clips.n_clips:
            desc.n_clips = clips.n_clips
        self.h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.hrg_batch_create(ctypes.byref(desc), ctypes.byref(table), self.n, int(env_id0), device, ctypes.byref(self.h)))
            C = CONST
            # one contiguous SoA output block so that multi-GPU runs need ONE all-gather per step (dist.packed_layout):
            # [obs f32 n*57 | reward f32 n | info i32 n*13 | done u8 n | term_obs f32 n*57]; `packed_head` (everything but the terminal
            # observations) is the part a step publishes to the other ranks
            from .dist import packed_layout, packed_views
            n, od, idim = self.n, C["HRG_OBS_DIM"], C["HRG_INFO_DIM"]
            if out is not None:
                self.obs, self.term_obs, self.reward, self.info, self.done = out
                want = [((n, od), torch.float32), ((n, od), torch.float32), ((n,), torch.float32), ((n, idim), torch.int32), ((n,), torch.uint8)]
                for t, (shape, dt) in zip(out, want):
                    if tuple(t.shape) != shape or t.dtype != dt or t.device != self.device or not t.is_contiguous():
                        raise ValueError(f"out tensor {tuple(t.shape)} {t.dtype} on {t.device}: expected contiguous {shape} {dt} on {self.device}")
                self.packed = self.packed_head = None
                return
            lay = packed_layout(n)
            self.packed = torch.zeros(lay["total"], dtype=torch.uint8, device=self.device)
            self.packed_head = self.packed[:lay["head"]]
            v = packed_views(self.packed, n)
            self.obs, self.term_obs, self.reward, self.info, self.done = v["obs"], v["term_obs"], v["reward"], v["info"], v["done"]

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _reset(self, fn, mask):
        mask = as_mask(mask, self.device)
        with self.torch.cuda.device(self.device):
            _check(self.lib, fn(self.h, _ptr(mask), _ptr(self.obs), self._stream()))
        self._keep_mask = mask
        return self.obs

    def reset(self, mask=None):
        """Reset all envs (mask None) or those with mask != 0 (uint8 tensor on device). Returns obs tensor."""
        return self._reset(self.lib.hrg_batch_reset, mask)

    def _step(self, fn, actions, *extra):
        """One of the three step entries of the ABI: `fn(batch, actions, obs, term_obs, reward, done, info, *extra, stream)`."""
        actions = as_actions(actions, self.n, self.device)
        with self.torch.cuda.device(self.device):
            _check(self.lib, fn(self.h, _ptr(actions), _ptr(self.obs), _ptr(self.term_obs), _ptr(self.reward), _ptr(self.done), _ptr(self.info),
                                *map(_ptr, extra), self._stream()))
        self._keep = actions

    def step(self, actions):
        """actions: float64 tensor [n, 7] on device. Returns (obs, reward, done, info) device tensors (views)."""
        self._step(self.lib.hrg_batch_step, actions)
        return self.obs, self.reward, self.done, self.info

    def check_actions(self, actions):
        """HumanEnv.check_collision_action for the whole batch: uint8 tensor [n], 1 where the joint-space action's goal configuration collides
        with the static scene or the robot itself (nothing is stepped)."""
        t = self.torch
        actions = as_actions(actions, self.n, self.device)
        out = t.empty(self.n, dtype=t.uint8, device=self.device)
        with t.cuda.device(self.device):
            _check(self.lib, self.lib.hrg_batch_check_actions(self.h, _ptr(actions), _ptr(out), self._stream()))
        self._keep_chk = actions
        return out

    def attach_expert(self, desc):
        """Attach a scripted expert (and, with desc.reward_enabled, the action-based imitation reward): `desc` is an ExpertDesc, e.g. from
        expert.build_expert_desc.  Allocates and zeroes the expert's per-env buffers (synchronous; not on the step path).  HrgError when the expert does
        not fit the batch's task or action form."""
        t = self.torch
        with t.cuda.device(self.device):
            _check(self.lib, self.lib.hrg_batch_expert_attach(self.h, ctypes.byref(desc)))
        self.expert_desc = desc
        self.imit = t.zeros(self.n, CONST["HRG_IMIT_DIM"], dtype=t.float32, device=self.device)
        self._expert_act = t.zeros(self.n, CONST["HRG_ACT_DIM"], dtype=t.float64, device=self.device)

    def expert_actions(self, obs=None):
        """The expert's action for every env: float64 tensor [n, 7] on device (Cartesian experts fill the first four columns).  `obs`: float32 [n, 64]
        rows of the observation superset (default: the batch's own, as the last reset / step left them).  Every call advances the expert's noise once.
        The returned tensor is reused by the next call."""
        if getattr(self, "expert_desc", None) is None:
            raise HrgError("no expert attached: call attach_expert() first")
        obs = self.obs if obs is None else as_obs(obs, self.n, self.device)
        with self.torch.cuda.device(self.device):
            _check(self.lib, self.lib.hrg_batch_expert_actions(self.h, _ptr(obs), _ptr(self._expert_act), self._stream()))
        self._keep_obs = obs
        return self._expert_act

    def step_imitation(self, actions):
        """`step` with the attached imitation reward: returns (obs, reward, done, info, imit); `reward` is r_im alpha + r_env (1 - alpha), `imit` the
        float32 [n, HRG_IMIT_DIM] row per env (r_im, r_env, r_motion, r_gripper, episode sums of r_im / r_env, episode length, combined reward)."""
        if getattr(self, "expert_desc", None) is None:
            raise HrgError("no expert attached: call attach_expert() first")
        self._step(self.lib.hrg_batch_step_imitation, actions, self.imit)
        return self.obs, self.reward, self.done, self.info, self.imit

    def snapshot(self, states_out, boxes_out=None):
        """One asynchronous device-to-device copy of every env's state block into `states_out` (uint8 [n, hrg_state_bytes()] on the batch's device) and,
        for a task with a box block, of the box blocks into `boxes_out` (uint8 [n, hrg_box_bytes()])."""
        t = self.torch
        for x, nb in ((states_out, ctypes.sizeof(EnvState)), (boxes_out, ctypes.sizeof(BoxState))):
            if x is not None and (x.dtype != t.uint8 or x.device != self.device or not x.is_contiguous() or tuple(x.shape) != (self.n, nb)):
                raise ValueError(f"snapshot: expected a contiguous uint8 tensor [{self.n}, {nb}] on {self.device}")
        vp = ctypes.c_void_p
        with t.cuda.device(self.device):
            _check(self.lib, self.lib.hrg_batch_snapshot(self.h, vp(states_out.data_ptr()), vp(boxes_out.data_ptr()) if boxes_out is not None else None, self._stream()))

    def attach_dataset(self, dataset, rsi_prob=0.0, state_imitation_reward=None, seed=0):
        """Upload a demonstration dataset (dataset.ExpertDataset) for reference state initialisation and, with `state_imitation_reward`
        (dict: dataset.sir_kwargs), the state-based imitation reward.  Synchronous; not on the step path.  HrgError when the task cannot be restored from
        a dataset (stacking, hammering) or the reward does not read its observation."""
        from .dataset import build_dataset_desc
        t = self.torch
        desc, keep = build_dataset_desc(dataset, rsi_prob=rsi_prob, state_imitation_reward=state_imitation_reward, seed=seed)
        with t.cuda.device(self.device):
            _check(self.lib, self.lib.hrg_batch_dataset_attach(self.h, ctypes.byref(desc)))
        del keep   # host arrays: read by the attach only
        self.dataset_desc = desc
        self.sir = t.zeros(self.n, CONST["HRG_SIR_DIM"], dtype=t.float32, device=self.device)

    def dataset_reset(self, mask=None):
        """`reset`, then every reset env starts from a dataset state (DatasetRSIWrapper.reset).  Returns the obs tensor (dataset observation rows)."""
        if getattr(self, "dataset_desc", None) is None:
            raise HrgError("no dataset attached: call attach_dataset() first")
        return self._reset(self.lib.hrg_batch_dataset_reset, mask)

    def step_dataset(self, actions):
        """`step` (or `step_imitation`, with an expert reward attached) followed by the dataset kernels: returns (obs, reward, done, info, sir); `sir` is the
        float32 [n, HRG_SIR_DIM] row per env (dataset.SIR_COLUMNS); finished envs (done, or early termination) restart from a dataset state."""
        if getattr(self, "dataset_desc", None) is None:
            raise HrgError("no dataset attached: call attach_dataset() first")
        self._step(self.lib.hrg_batch_step_dataset, actions, getattr(self, "imit", None), self.sir)
        return self.obs, self.reward, self.done, self.info, self.sir

    def dataset_cursor(self):
        """(episode, step, T) of every env: int32 [n, 3] (synchronous parity hook)."""
        import numpy as np
        cur = np.zeros((self.n, 3), np.int32)
        _check(self.lib, self.lib.hrg_batch_dataset_cursor(self.h, cur.ctypes.data_as(ctypes.c_void_p)))
        return cur

    def get_state(self, e):
        s = EnvState()
        _check(self.lib, self.lib.hrg_batch_get_state(self.h, int(e), ctypes.byref(s), ctypes.sizeof(s)))
        return s

    def set_state(self, e, s):
        _check(self.lib, self.lib.hrg_batch_set_state(self.h, int(e), ctypes.byref(s), ctypes.sizeof(s)))

    def get_states(self, envs):
        """Environment states (+ manipulation objects) of several envs in one call: (EnvState[n], BoxState[n])."""
        import numpy as np
        idx = np.ascontiguousarray(envs, np.int32)
        st, bx = (EnvState * len(idx))(), (BoxState * len(idx))()
        _check(self.lib, self.lib.hrg_batch_get_states(self.h, idx.ctypes.data_as(ctypes.c_void_p), len(idx), ctypes.byref(st), ctypes.byref(bx)))
        return st, bx

    def set_states(self, envs, states, boxes=None):
        """Reference-state initialisation: overwrite the listed envs' states (wrappers/dataset_wrapper.py:88-160)."""
        import numpy as np
        idx = np.ascontiguousarray(envs, np.int32)
        assert len(states) == len(idx) and (boxes is None or len(boxes) == len(idx))
        _check(self.lib, self.lib.hrg_batch_set_states(self.h, idx.ctypes.data_as(ctypes.c_void_p), len(idx), ctypes.byref(states),
                                                       ctypes.byref(boxes) if boxes is not None else None))

    def stagger_episode_phases(self, horizon):
        """Spread the TimeLimit phase over the batch: env e continues as if it were (e * horizon) // n policy steps into its episode.  A freshly reset batch
        has every env at step 0, so that all of them time out in the same step, every `horizon` steps; a batch that has been training for a while has its
        episode ends spread evenly (early successes and failures shift each env's phase).  Benchmarks call this once after reset."""
        import numpy as np
        idx = np.arange(self.n, dtype=np.int32)
        st, bx = self.get_states(idx)
        for e in range(self.n):
            st[e].timestep = (e * int(horizon)) // self.n
        self.set_states(idx, st, bx)

    def get_box(self, e):
        """The manipulation object of env e (PickPlaceHumanCart; zeros for ReachHuman)."""
        s = BoxState()
        _check(self.lib, self.lib.hrg_batch_get_box(self.h, int(e), ctypes.byref(s), ctypes.sizeof(s)))
        return s

    def set_box(self, e, s):
        _check(self.lib, self.lib.hrg_batch_set_box(self.h, int(e), ctypes.byref(s), ctypes.sizeof(s)))

    def get_hammer(self, e):
        """Board, hammer, nail + task bookkeeping of env e (CollaborativeHammeringCart)."""
        s = HammerState()
        _check(self.lib, self.lib.hrg_batch_get_hammer(self.h, int(e), ctypes.byref(s), ctypes.sizeof(s)))
        return s

    def set_hammer(self, e, s):
        _check(self.lib, self.lib.hrg_batch_set_hammer(self.h, int(e), ctypes.byref(s), ctypes.sizeof(s)))

    def get_stack(self, e):
        """The four cubes + task bookkeeping of env e (CollaborativeStackingCart)."""
        s = StackState()
        _check(self.lib, self.lib.hrg_batch_get_stack(self.h, int(e), ctypes.byref(s), ctypes.sizeof(s)))
        return s

    def set_stack(self, e, s):
        _check(self.lib, self.lib.hrg_batch_set_stack(self.h, int(e), ctypes.byref(s), ctypes.sizeof(s)))

    def contacts(self):
        import numpy as np
        pairs = np.zeros((self.n, CONST["HRG_NCON_MAX"], 2), np.int32)
        ncon = np.zeros(self.n, np.int32)
        _check(self.lib, self.lib.hrg_batch_contacts(self.h, pairs.ctypes.data_as(ctypes.c_void_p), ncon.ctypes.data_as(ctypes.c_void_p)))
        return pairs, ncon

    def launch_order(self):
        """(order, n_busy): the env each workgroup of the next step launch will step, and how many of them -- from the front -- were busy in the last step."""
        import numpy as np
        order = np.zeros(self.n, np.int32)
        nb = ctypes.c_int32(0)
        _check(self.lib, self.lib.hrg_batch_launch_order(self.h, order.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nb)))
        return order, int(nb.value)

    def mpr_fallbacks(self):
        """Arm link hull - box pairs (robot_geometry="hull", every task with an object) whose MPR did not converge and kept the capsule contact, summed over every substep since create."""
        c = ctypes.c_int64()
        _check(self.lib, self.lib.hrg_batch_mpr_fallbacks(self.h, ctypes.byref(c)))
        return c.value

    def pose_table_bytes(self):
        """Device memory of the batch's human pose table (built at create for ReachHuman and CollaborativeLiftingCart; 0 for the tasks whose kernels keep the live tree kinematics)."""
        c = ctypes.c_int64()
        _check(self.lib, self.lib.hrg_batch_pose_table_bytes(self.h, ctypes.byref(c)))
        return c.value

    def enable_taps(self, on=True):
        _check(self.lib, self.lib.hrg_batch_enable_taps(self.h, int(bool(on))))

    def capsules(self):
        import numpy as np
        r = np.zeros((self.n, CONST["HRG_NSHIELD_RCAP"], 7))
        h = np.zeros((self.n, CONST["HRG_NHCAP_MAX"], 7))
        nh = np.zeros(self.n, np.int32)
        vp = ctypes.c_void_p
        _check(self.lib, self.lib.hrg_batch_capsules(self.h, r.ctypes.data_as(vp), h.ctypes.data_as(vp), nh.ctypes.data_as(vp)))
        return r, h, nh

    def kernel_time(self):
        """(avg kernel ms, launches) of the step kernels since the previous call (HIP events on the launch stream).
        The first call arms the timer."""
        ms, n = ctypes.c_double(), ctypes.c_int64()
        _check(self.lib, self.lib.hrg_batch_kernel_time(self.h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.hrg_batch_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
