"""What the device learners share (sac.SacLearner, ppo.PpoLearner; csrc/hrgym_mlp.h): the refusal of widths the tile kernels do not cover, the flat parameter
layout, the tensors behind `state_dict()` with their seeded initialisation, the learner's calls that differ by the entry points' prefix only, and what the
two populations share (sac.SacPopulation, ppo.PpoPopulation): the seeds table, the stacked tensors, a member as a lone learner, the checkpoints per member."""
import ctypes
import os
from collections import OrderedDict

import numpy as np

from ._cstruct import CONST
from ._device import DeviceHandle


def check_widths(obs_dim, act_dim, batch_size, tile, max_batch):
    """(obs_dim, act_dim, batch_size) as ints; NotImplementedError for what the kernels do not cover: batches are multiples of `tile` up to `max_batch`."""
    obs_dim, act_dim, batch_size = int(obs_dim), int(act_dim), int(batch_size)
    if not 1 <= obs_dim <= CONST["HRG_OBS_DIM"]:
        raise NotImplementedError(f"obs_dim = {obs_dim}: the kernels cover observations of 1 .. {CONST['HRG_OBS_DIM']} values")
    if not 1 <= act_dim <= CONST["HRG_ACT_DIM"]:
        raise NotImplementedError(f"act_dim = {act_dim}: the kernels cover actions of 1 .. {CONST['HRG_ACT_DIM']} values")
    if batch_size % tile or not tile <= batch_size <= max_batch:
        raise NotImplementedError(f"batch_size = {batch_size}: the kernels cover multiples of {tile} from {tile} to {max_batch}")
    return obs_dim, act_dim, batch_size


def build_layout(entries):
    """(name, shape) in the flat vector's order -> (OrderedDict name -> (offset, shape), total)."""
    out, o = OrderedDict(), 0
    for name, shape in entries:
        out[name] = (o, shape)
        o += int(np.prod(shape))
    return out, o


def mlp_entries(prefix, depth, in0, hidden):
    """The hidden layers `prefix`.{0, 2, ..}.weight / .bias of a torch Sequential of Linear and activation."""
    for l in range(depth):
        yield f"{prefix}.{2 * l}.weight", (hidden, hidden if l else in0)
        yield f"{prefix}.{2 * l}.bias", (hidden,)


class LearnerParams:
    """A learner's tensors, on any torch device: `params`, `adam_m`, `adam_v` float32 [n_params] in `layout`'s order, with `state_dict()` views under SB3's names.
    Initial weights are drawn under a forked generator seeded with `seed` (the global one stays as it is), a torch.nn.Linear per weight entry in the layout's
    order; its bias is the entry of the same name.  `_init_linear` may redraw a layer, `_init_rest` sets what is no layer."""

    def __init__(self, layout, n_params, seed, device):
        import torch
        self.torch = torch
        self.layout, self.n_params = layout, n_params
        flat = torch.zeros(n_params, dtype=torch.float32)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(int(seed))
            for name, (off, shape) in layout.items():
                if not name.endswith(".weight"):
                    continue
                lin = torch.nn.Linear(shape[1], shape[0])
                self._init_linear(name, lin)
                flat[off:off + lin.weight.numel()] = lin.weight.detach().reshape(-1)
                boff, _ = layout[name[:-len("weight")] + "bias"]
                flat[boff:boff + shape[0]] = lin.bias.detach()
        self._init_rest(flat)
        self.params = flat.to(device)
        self.adam_m, self.adam_v = torch.zeros_like(self.params), torch.zeros_like(self.params)

    def _init_linear(self, name, lin):
        pass

    def _init_rest(self, flat):
        pass

    def state_dict(self):
        """OrderedDict of views into the learner's tensors under SB3's names (writing into one writes the learner's parameter)."""
        return OrderedDict((name, self.params[off:off + int(np.prod(shape))].view(shape)) for name, (off, shape) in self.layout.items())

    def load_state_dict(self, state):
        """Copies every entry of `state` (tensors or arrays of the entries' shapes, every name of `state_dict()` present) into the learner's tensors."""
        t = self.torch
        own = self.state_dict()
        missing, unknown = sorted(set(own) - set(state)), sorted(set(state) - set(own))
        if missing or unknown:
            raise KeyError(f"load_state_dict: missing {missing}, unknown {unknown}")
        with t.no_grad():
            for name, view in own.items():
                src = t.as_tensor(state[name])
                if tuple(src.shape) != tuple(view.shape):
                    raise ValueError(f"load_state_dict: {name} has shape {tuple(src.shape)}, expected {tuple(view.shape)}")
                view.copy_(src.to(device=view.device, dtype=view.dtype))


# ---- checkpoints: one .npz per learner -- the descriptor's fields, the tensors, the counters, the scheduled attributes; arrays only, read without pickle ----
CHECKPOINT_FORMAT = 1
TENSORS = ("params", "adam_m", "adam_v", "target")   # `target`: where the learner keeps one (SAC)


def desc_fields(desc):
    """The fields of a ctypes descriptor as numpy scalars and arrays, by name (reserved_ left out)."""
    out = {}
    for name, _ in desc._fields_:
        if not name.endswith("_"):
            v = getattr(desc, name)
            out[name] = np.array(list(v)) if isinstance(v, ctypes.Array) else np.array(v)
    return out


def save_checkpoint(path, kind, desc, p, counters, hyper):
    """Writes the checkpoint of a learner of `kind` (its entry points' prefix) to `path`: `desc` its descriptor, `p` its LearnerParams (on any device), `counters`
    (steps, forward calls that drew their noise), `hyper` name -> number: the attributes a caller may schedule (None is stored as NaN)."""
    arrays = {"format": np.array(CHECKPOINT_FORMAT, np.int64), "kind": np.array(str(kind)), "counters": np.array([int(c) for c in counters], np.uint64)}
    arrays.update({"desc." + k: v for k, v in desc_fields(desc).items()})
    arrays.update({"hyper." + k: np.array(np.nan if v is None else v, np.float64) for k, v in hyper.items()})
    for name in TENSORS:
        if hasattr(p, name):
            arrays[name] = getattr(p, name).detach().cpu().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        np.savez(f, **arrays)
    return path


def load_checkpoint(path, kind):
    """The arrays of a checkpoint of a learner of `kind` as a dict, with `desc` and `hyper` as dicts of their own; ValueError for a file of another kind or
    format.  No pickle is read."""
    with np.load(path, allow_pickle=False) as f:
        arrays = {k: f[k] for k in f.files}
    for name in ("format", "kind", "counters", "params", "adam_m", "adam_v"):
        if name not in arrays:
            raise ValueError(f"{path}: no checkpoint of a device learner: {name} is missing")
    if int(arrays["format"]) != CHECKPOINT_FORMAT:
        raise ValueError(f"{path}: format = {int(arrays['format'])}, this build reads {CHECKPOINT_FORMAT}")
    if str(arrays["kind"]) != kind:
        raise ValueError(f"{path}: kind = {str(arrays['kind'])!r}: a checkpoint of another learner than {kind!r}")
    out = {k: v for k, v in arrays.items() if "." not in k}
    for group in ("desc", "hyper"):
        out[group] = {k[len(group) + 1:]: v for k, v in arrays.items() if k.startswith(group + ".")}
    return out


def restore_tensors(p, ckpt):
    """Copies the checkpoint's tensors into the LearnerParams `p`; ValueError, naming the field, where a shape differs."""
    import torch
    for name in TENSORS:
        if not hasattr(p, name):
            continue
        own = getattr(p, name)
        if name not in ckpt:
            raise ValueError(f"checkpoint: {name} is missing")
        src = np.asarray(ckpt[name])
        if tuple(src.shape) != tuple(own.shape) or src.dtype != np.float32:
            raise ValueError(f"checkpoint: {name} is {src.dtype} {tuple(src.shape)}, the learner's is float32 {tuple(own.shape)} (a checkpoint of other shapes)")
        with torch.no_grad():
            own.copy_(torch.from_numpy(src).to(own.device))


# ---- populations: what sac.SacPopulation and ppo.PpoPopulation share ----
MAX_POPULATION = CONST["HRG_SAC_MAX_POPULATION"]
assert MAX_POPULATION == CONST["HRG_PPO_MAX_POPULATION"]


def check_seeds(n_members, seeds):
    """(P, the members' seeds as uint64 [P]); NotImplementedError for a population the kernels do not cover, ValueError for a seeds table of another length."""
    P = int(n_members)
    if not 1 <= P <= MAX_POPULATION:
        raise NotImplementedError(f"n_members = {P}: a population has 1 .. {MAX_POPULATION} members")
    seeds = [int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds]
    if len(seeds) != P:
        raise ValueError(f"seeds: {len(seeds)} seeds for {P} members")
    return P, np.array(seeds, np.uint64)


class PopulationParams:
    """The tensors of a population, on any torch device: every tensor of the lone learners' LearnerParams `rows` stacked, [P, ...].  Row p is member p's,
    initialised exactly as the lone learner of its seed; `member(p)` is the rows of member p as views."""

    def __init__(self, rows, device):
        import torch
        self.layout, self.n_params = rows[0].layout, rows[0].n_params
        for name in TENSORS:
            if hasattr(rows[0], name):
                setattr(self, name, torch.stack([getattr(r, name) for r in rows]).to(device))

    def member(self, p):
        from types import SimpleNamespace
        return SimpleNamespace(**{name: getattr(self, name)[p] for name in TENSORS if hasattr(self, name)})


class Population:
    """What the populations add to their lone learner's class, ahead of it in the bases: `_lone` is that class, `n_members`, `seeds` (ints) and `_kwargs` (the
    lone learner's constructor keywords apart from the seed, the device and the scheduled attributes of `_hyper`) are set by the subclass, `p` is a
    PopulationParams."""
    _lone = None

    def _export(self, *arrays, member=0):
        self._check(self.lib, getattr(self.lib, self._prefix + "_population_export")(self.h, int(member), *(None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in arrays)))

    def export(self, member=0):
        """The lone learner's export of one member."""
        return super().export(member=member)

    def diagnostics(self):
        """The lone learner's diagnostics of every member: a list of n_members dicts.  Synchronous."""
        return [super(Population, self).diagnostics(member=p) for p in range(self.n_members)]

    def _restore(self, steps, calls):
        self._check(self.lib, getattr(self.lib, self._prefix + "_restore")(self.h, int(steps), int(calls)))

    def member(self, p):
        """Member p as a lone learner of its own: copies of its tensors, the population's counters and scheduled attributes.  Fed the same batches, it
        continues bit for bit.  The caller closes it."""
        if not 0 <= int(p) < self.n_members:
            raise IndexError(f"member {p} of {self.n_members}")
        learner = self._lone(self.obs_dim, self.act_dim, seed=self.seeds[p], device=self.device.index, **self._kwargs, **self._hyper())
        sizes = self._sizes()
        with self.torch.no_grad():
            for name, rows in vars(self.p.member(int(p))).items():
                getattr(learner.p, name).copy_(rows)
        Population._restore(learner, sizes[3], sizes[4])
        return learner

    def save(self, path):
        """One checkpoint per member, `path`/member_<p>.npz, in the lone learner's format: its `load` and tools/evaluate.py read them.  Synchronous."""
        sizes = self._sizes()
        for p in range(self.n_members):
            desc = type(self.desc).from_buffer_copy(self.desc)
            desc.seed = self.seeds[p]
            save_checkpoint(os.path.join(path, f"member_{p}.npz"), self._prefix, desc, self.p.member(p), (sizes[3], sizes[4]), self._hyper())
        return path

    @classmethod
    def load(cls, path, device=0):
        """The population of the member_<p>.npz under `path` (p = 0, 1, .. without a gap).  ValueError for members of different shapes, hyper-parameters or
        counters: those are no population."""
        files = []
        while os.path.exists(os.path.join(path, f"member_{len(files)}.npz")):
            files.append(os.path.join(path, f"member_{len(files)}.npz"))
        if not files:
            raise ValueError(f"{path}: no member_0.npz")
        ckpts = [load_checkpoint(f, cls._prefix) for f in files]
        first = ckpts[0]
        for f, c in zip(files, ckpts):
            differs = [k for k in first["desc"] if k != "seed" and not np.array_equal(first["desc"][k], c["desc"][k])]
            differs += [k for k in first["hyper"] if not np.array_equal(first["hyper"][k], c["hyper"][k], equal_nan=True)]
            if differs or not np.array_equal(first["counters"], c["counters"]):
                raise ValueError(f"{f}: {', '.join(differs) or 'counters'} differ from member 0's: the members of a population share them")
        pop = cls(n_members=len(ckpts), seeds=[int(c["desc"]["seed"]) for c in ckpts], device=device, **cls._checkpoint_kwargs(first["desc"], first["hyper"]))
        try:
            for p, c in enumerate(ckpts):
                restore_tensors(pop.p.member(p), c)
            pop._restore(*(int(x) for x in first["counters"]))
        except Exception:
            pop.close()
            raise
        return pop

    def state_dict(self):
        raise NotImplementedError("state_dict of a population: member(p).state_dict()")

    def load_state_dict(self, state):
        raise NotImplementedError("load_state_dict of a population: load the member's checkpoint")


class Learner(DeviceHandle):
    """What SacLearner and PpoLearner share on the handle.  A subclass names its entry points (`_prefix`: hrg_sac / hrg_ppo), sets `obs_dim`, `act_dim` and
    keeps its LearnerParams as `p`."""
    _prefix = None

    def _open(self, desc, device, *create_args, create="_create"):
        self._create, self._destroy = self._prefix + create, self._prefix + "_destroy"
        super()._open(desc, device, *create_args)

    def _sizes(self):
        w = (ctypes.c_int64 * 6)()
        self._check(self.lib, getattr(self.lib, self._prefix + "_sizes")(self.h, w))
        return [int(x) for x in w]

    @property
    def n_updates(self):
        """Steps so far: the optimisers' step count (SAC: SB3's _n_updates)."""
        return self._sizes()[3]

    def _tensor(self, x, shape, what):
        return super()._tensor(x, self.torch.float32, shape, what)

    def _rows(self, obs, eps):
        """(n, obs, eps) as a forward entry point takes them, for `obs` float32 [n, obs_dim] and `eps` float32 [n, act_dim] or None."""
        if obs.dim() != 2:
            raise ValueError(f"obs: expected [n, {self.obs_dim}], got {tuple(obs.shape)}")
        n = int(obs.shape[0])
        return n, self._tensor(obs, (n, self.obs_dim), "obs"), None if eps is None else self._tensor(eps, (n, self.act_dim), "eps")

    def _check_buffer(self, obs_dim, act_dim):
        """ValueError unless the buffer `train` reads holds rows of the learner's widths."""
        if (int(obs_dim), int(act_dim)) != (self.obs_dim, self.act_dim):
            raise ValueError(f"train: the buffer holds observations of {obs_dim} and actions of {act_dim} values, the learner takes {self.obs_dim} and {self.act_dim}")

    def _export(self, *arrays):
        """hrg_*_export into the host arrays (None: not asked for).  Synchronous."""
        self._check(self.lib, getattr(self.lib, self._prefix + "_export")(self.h, *(None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in arrays)))

    def save(self, path):
        """The learner as one .npz (`save_checkpoint`): the descriptor's fields, params, adam_m, adam_v, target (SAC), the counters and the scheduled attributes.
        Synchronous.  `load` makes a learner that continues bit for bit: Adam's bias corrections, the draws' keys and the phase of the target update follow
        from the counters."""
        sizes = self._sizes()
        return save_checkpoint(path, self._prefix, self.desc, self.p, (sizes[3], sizes[4]), self._hyper())

    @classmethod
    def load(cls, path, device=0):
        """A fresh learner from a checkpoint `save` wrote.  ValueError, naming the field, for a file of another learner or of other shapes."""
        ckpt = load_checkpoint(path, cls._prefix)
        learner = cls._from_checkpoint(ckpt["desc"], ckpt["hyper"], device)
        try:
            restore_tensors(learner.p, ckpt)
            steps, calls = (int(c) for c in ckpt["counters"])
            learner._check(learner.lib, getattr(learner.lib, cls._prefix + "_restore")(learner.h, steps, calls))
        except Exception:
            learner.close()
            raise
        return learner

    def state_dict(self):
        """Views of the parameters under SB3's names, torch's [out, in] weight layout (the names: `p`'s class)."""
        return self.p.state_dict()

    def load_state_dict(self, state):
        self.p.load_state_dict(state)
