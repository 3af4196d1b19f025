"""What the device learners share (sac.SacLearner, ppo.PpoLearner; csrc/hrgym_mlp.h): the refusal of widths the tile kernels do not cover, the flat parameter
layout, the tensors behind `state_dict()` with their seeded initialisation, the learner's calls that differ by the entry points' prefix only, and what the
two populations share (sac.SacPopulation, ppo.PpoPopulation): the seeds table, a value per member of every hyper-parameter the device table holds, the stacked
tensors, a member as a lone learner, the checkpoints per member and their manifest."""
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


def restore_tensors(p, ckpt, names=TENSORS):
    """Copies the checkpoint's tensors (`names`: which of them) into the LearnerParams `p`; ValueError, naming the field, where a shape differs."""
    import torch
    for name in names:
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


def per_member(name, value, n_members):
    """`value` of the hyper-parameter `name` for every member, a list of n_members: a scalar (a number, a string such as "auto_0.2", None) means every member,
    a list, tuple or array is one value per member; ValueError, naming the field, for a sequence of another length."""
    if isinstance(value, (list, tuple, np.ndarray)):
        values = [v.item() if isinstance(v, np.generic) else v for v in value]
        if len(values) != int(n_members):
            raise ValueError(f"{name}: {len(values)} values for {int(n_members)} members (a scalar, or one value per member)")
        return values
    return [value] * int(n_members)


def refuse_shared_sequences(shared, kwargs):
    """NotImplementedError where `kwargs` holds one value per member for a keyword of `shared` (name -> why every member of a population shares it).  net_arch
    is a list by itself: one per member would be a list of lists."""
    for name, why in shared.items():
        value = kwargs.get(name)
        many = isinstance(value, (list, tuple, np.ndarray))
        if name == "net_arch":
            many = many and len(value) > 0 and all(isinstance(v, (list, tuple)) for v in value)
        if many:
            raise NotImplementedError(f"{name} = {value}: one value per member is not supported: {why}")


# ---- the manifest of a population's folder: which fields of the members' checkpoints differ (one .npz of arrays, read without pickle) ----
MANIFEST = "population.npz"


def write_manifest(folder, kind, varies):
    """`folder`/population.npz for a population of `kind` whose members differ in the checkpoint fields `varies` (names of the desc.* and hyper.* entries);
    with nothing that varies no manifest is written, and one that is there is removed."""
    path = os.path.join(folder, MANIFEST)
    if not varies:
        if os.path.exists(path):
            os.remove(path)
        return None
    with open(path, "wb") as f:
        np.savez(f, format=np.array(CHECKPOINT_FORMAT, np.int64), kind=np.array(str(kind)), varies=np.array(sorted(str(v) for v in varies)))
    return path


def read_manifest(folder, kind):
    """The field names `folder`/population.npz lists, () without the file; ValueError for a manifest of another learner or format."""
    path = os.path.join(folder, MANIFEST)
    if not os.path.exists(path):
        return ()
    with np.load(path, allow_pickle=False) as f:
        arrays = {k: f[k] for k in f.files}
    if "varies" not in arrays or int(arrays.get("format", -1)) != CHECKPOINT_FORMAT or str(arrays.get("kind")) != kind:
        raise ValueError(f"{path}: no manifest of a population of {kind!r} in format {CHECKPOINT_FORMAT}")
    return tuple(str(v) for v in np.atleast_1d(arrays["varies"]))


def check_members(files, ckpts, varies=(), may_vary=()):
    """ValueError unless the checkpoints `ckpts` (load_checkpoint's dicts, of `files`) are the members of one population: the same descriptor fields (the seed
    apart), scheduled attributes and counters, but for the fields the manifest names (`varies`), which have to be among the ones the table holds (`may_vary`)."""
    unknown = sorted(set(varies) - set(may_vary))
    if unknown:
        raise ValueError(f"{os.path.dirname(files[0])}: the manifest names {', '.join(unknown)}: the members of a population share them (per member: {', '.join(may_vary)})")
    first = ckpts[0]
    for f, c in zip(files, ckpts):
        differs = [k for k in first["desc"] if k != "seed" and k not in varies and not np.array_equal(first["desc"][k], c["desc"][k])]
        differs += [k for k in first["hyper"] if k not in varies and not np.array_equal(first["hyper"][k], c["hyper"][k], equal_nan=True)]
        if differs or not np.array_equal(first["counters"], c["counters"]):
            raise ValueError(f"{f}: {', '.join(differs) or 'counters'} differ from member 0's: the members of a population share them")


def scheduled_attribute(name):
    """A scheduled attribute of a population (Population._scheduled): every member's value where they agree, else the list of them; a scalar or one value per
    member may be assigned between any two steps, and the table is uploaded again where it is the caller's."""
    def get(self):
        values = self._values[name]
        return values[0] if all(v == values[0] for v in values) else list(values)

    def put(self, value):
        self._set_values(**{name: value})
        self._sync_table()
    return property(get, put, doc=scheduled_attribute.__doc__)


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
    PopulationParams.

    Hyper-parameters per member.  `_fields` names the constructor keywords the handle's device table holds a row of per member, `_scheduled`
    those of them that are plain attributes of the lone learner (a scalar or a sequence may be assigned between steps), `_shared` the keywords every member
    shares, with the reason; `_convert(name, value)` checks one member's value and `_row(p)` is member p's row of the table (hrg_*_hyper).  `_values[name]` is the
    list of the members' values.  While every member has the same values nothing is uploaded: the step's scalar arguments fill the table, as for the lone
    learner.  From the first upload on the table is the caller's (`_per_member`), and every assignment uploads it again."""
    _lone = None
    _fields = _scheduled = _manifest_fields = ()
    _shared = {}
    _per_member = False

    @classmethod
    def member_values(cls, n_members, **values):
        """{name: the n_members members' values} of the table fields named, a scalar or a sequence each (per_member), every value checked (`_convert`)."""
        return {name: [cls._convert(name, v) for v in per_member(name, value, n_members)] for name, value in values.items()}

    def _set_values(self, **values):
        if "_values" not in self.__dict__:
            self._values = {}
        self._values.update(self.member_values(self.n_members, **values))
        self._member0 = tuple(self._values[name][0] for name in self._scheduled if name in self._values)   # (what a step passes as its scalars)

    @staticmethod
    def _convert(name, value):
        return float(value)

    def varying(self):
        """The table's fields in which the members differ, in the table's order."""
        return [name for name in self._fields if any(v != self._values[name][0] for v in self._values[name])]

    def member_hyper(self, p):
        """Every field of member p's row of the table, under the constructor's keywords and in its forms ("auto_0.2", clip_range_vf None)."""
        if not 0 <= int(p) < self.n_members:
            raise IndexError(f"member {p} of {self.n_members}")
        return {name: self._values[name][int(p)] for name in self._fields}

    def _scalar(self, name, member=0):
        return self._values[name][int(member)]

    def _sync_table(self):
        """Uploads the table where the members differ, or have differed before; ordered on torch's current stream behind the steps queued there."""
        if not (self._per_member or self.varying()) or not getattr(self, "h", None):
            return
        rows = (type(self._row(0)) * self.n_members)(*(self._row(p) for p in range(self.n_members)))
        with self.torch.cuda.device(self.device):
            self._check(self.lib, getattr(self.lib, self._prefix + "_population_set_hyper")(self.h, ctypes.byref(rows), self.n_members, self._stream()))
        self._per_member = True

    def _hyper_of(self, p):
        """The lone learner's `_hyper()` of member p."""
        return {k: (self._values[k][p] if k in self._scheduled else v) for k, v in self._hyper().items()}

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
        """Member p as a lone learner of its own: copies of its tensors, the population's counters, member p's hyper-parameters and scheduled attributes.  Fed
        the same batches, it continues bit for bit.  The caller closes it."""
        if not 0 <= int(p) < self.n_members:
            raise IndexError(f"member {p} of {self.n_members}")
        learner = self._lone(self.obs_dim, self.act_dim, seed=self.seeds[p], device=self.device.index, **{**self._kwargs, **self._hyper_of(int(p)), **self.member_hyper(p)})
        sizes = self._sizes()
        with self.torch.no_grad():
            for name, rows in vars(self.p.member(int(p))).items():
                getattr(learner.p, name).copy_(rows)
        Population._restore(learner, sizes[3], sizes[4])
        return learner

    def save(self, path):
        """One checkpoint per member, `path`/member_<p>.npz, in the lone learner's format with the member's own descriptor fields and scheduled attributes: its
        `load` and tools/evaluate.py read them.  Where the members differ in more than their seed, `path`/population.npz names the fields (write_manifest).
        Synchronous."""
        sizes = self._sizes()
        descs, hypers = [self._member_desc(p) for p in range(self.n_members)], [self._hyper_of(p) for p in range(self.n_members)]
        for p in range(self.n_members):
            save_checkpoint(os.path.join(path, f"member_{p}.npz"), self._prefix, descs[p], self.p.member(p), (sizes[3], sizes[4]), hypers[p])
        fields = [desc_fields(d) for d in descs]
        varies = [k for k in fields[0] if k != "seed" and any(not np.array_equal(f[k], fields[0][k]) for f in fields)]
        varies += [k for k in hypers[0] if any(h[k] != hypers[0][k] for h in hypers)]
        write_manifest(path, self._prefix, varies)
        return path

    @classmethod
    def load(cls, path, device=0):
        """The population of the member_<p>.npz under `path` (p = 0, 1, .. without a gap).  ValueError for members of different shapes, counters or
        hyper-parameters, but for those the folder's manifest names (population.npz, written by `save`): those are no population."""
        files = []
        while os.path.exists(os.path.join(path, f"member_{len(files)}.npz")):
            files.append(os.path.join(path, f"member_{len(files)}.npz"))
        if not files:
            raise ValueError(f"{path}: no member_0.npz")
        ckpts = [load_checkpoint(f, cls._prefix) for f in files]
        first = ckpts[0]
        varies = read_manifest(path, cls._prefix)
        check_members(files, ckpts, varies, cls._manifest_fields)
        kwargs = cls._checkpoint_kwargs(first["desc"], first["hyper"])
        if varies:
            members = [cls._checkpoint_kwargs(c["desc"], c["hyper"]) for c in ckpts]
            kwargs.update({name: [m[name] for m in members] for name in cls._fields if any(m[name] != members[0][name] for m in members)})
        pop = cls(n_members=len(ckpts), seeds=[int(c["desc"]["seed"]) for c in ckpts], device=device, **kwargs)
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

    def _scalar(self, name, member=0):
        """The scheduled attribute `name` as a step or a diagnostic reads it (a population: the member's)."""
        return getattr(self, name)

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

    def load_parameters(self, path):
        """The parameters of a checkpoint `save` wrote -- the tensors behind `state_dict()`: `params` and, where the learner keeps one, `target` -- into this
        learner, whose Adam moments, counters and scheduled attributes stay as they are: a run that starts from pre-trained weights (bc.BehaviourCloning)
        with a fresh optimiser.  ValueError, naming the field, for a file of another learner or of other shapes."""
        restore_tensors(self.p, load_checkpoint(path, self._prefix), names=("params", "target"))

    def state_dict(self):
        """Views of the parameters under SB3's names, torch's [out, in] weight layout (the names: `p`'s class)."""
        return self.p.state_dict()

    def load_state_dict(self, state):
        self.p.load_state_dict(state)
