"""What the device learners share (sac.SacLearner, ppo.PpoLearner; csrc/hrgym_mlp.h): the refusal of widths the tile kernels do not cover, the flat parameter
layout, the tensors behind `state_dict()` with their seeded initialisation, and the learner's calls that differ by the entry points' prefix only."""
import ctypes
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


class Learner(DeviceHandle):
    """What SacLearner and PpoLearner share on the handle.  A subclass names its entry points (`_prefix`: hrg_sac / hrg_ppo), sets `obs_dim`, `act_dim` and
    keeps its LearnerParams as `p`."""
    _prefix = None

    def _open(self, desc, device):
        self._create, self._destroy = self._prefix + "_create", self._prefix + "_destroy"
        super()._open(desc, device)

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

    def state_dict(self):
        """Views of the parameters under SB3's names, torch's [out, in] weight layout (the names: `p`'s class)."""
        return self.p.state_dict()

    def load_state_dict(self, state):
        self.p.load_state_dict(state)
