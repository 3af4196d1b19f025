"""Multi-GPU sharding: one process per GPU, envs split by global id, ONE all-gather of the packed outputs per step.

Envs never interact (one OS process each in the reference, utils/training_utils_SB3.py:71), so there is no data-path
collective inside a step; the only exchange is publishing every rank's (obs, term_obs, reward, info, done) block to
all ranks — RCCL `all_gather` over xGMI on GPUs ("nccl" backend), gloo on CPU for tests.
"""
import numpy as np

from ._cstruct import CONST


def shard_range(n_global, rank, world):
    """Global env ids [lo, hi) owned by `rank`; remainders go to the lowest ranks."""
    base, rem = divmod(n_global, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def packed_layout(n):
    """Byte layout of one rank's output block (HipBatch.packed).  Items are indexed [obs, term_obs, reward, info, done]; physically the
    terminal observations come LAST, so that the prefix of `head` bytes (obs, reward, info, done) is what a step publishes to the other
    ranks — terminal observations matter for the few envs that finished and stay on their rank."""
    od, idim = CONST["HRG_OBS_DIM"], CONST["HRG_INFO_DIM"]
    sizes = [4 * n * od, 4 * n * od, 4 * n, 4 * n * idim, n]
    offs, tot = [0] * 5, 0
    for item in (0, 2, 3, 4, 1):
        offs[item] = tot
        tot += (sizes[item] + 255) // 256 * 256
    return dict(offsets=offs, sizes=sizes, total=tot, head=offs[1])


def packed_views(block, n):
    """The typed views of one rank's output block of `n` envs: dict obs, term_obs, reward, info, done (no copies).  `block` is a uint8 torch tensor (device
    or pinned host) or a uint8 numpy array: the whole block, or only its published head, which has no `term_obs`.  The one place that slices the block."""
    lay = packed_layout(n)
    o, s = lay["offsets"], lay["sizes"]
    od, idim = CONST["HRG_OBS_DIM"], CONST["HRG_INFO_DIM"]
    if isinstance(block, np.ndarray):
        f32, i32 = np.float32, np.int32
    else:
        import torch
        f32, i32 = torch.float32, torch.int32
    items = [("obs", 0, f32, (n, od)), ("term_obs", 1, f32, (n, od)), ("reward", 2, f32, (n,)), ("info", 3, i32, (n, idim)), ("done", 4, None, (n,))]
    if block.shape[0] < lay["total"]:
        del items[1]
    return {k: (block[o[i]:o[i] + s[i]] if dt is None else block[o[i]:o[i] + s[i]].view(dt)).reshape(shape) for k, i, dt, shape in items}


unpack = packed_views   # (the name the multi-GPU callers use)


def all_gather_packed(packed, group=None):
    """All-gather equal-sized packed blocks (torch uint8 tensors). Returns a [world, total] tensor on every rank."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    out = torch.empty((world, packed.numel()), dtype=torch.uint8, device=packed.device)
    if dist.get_backend(group) == "gloo":
        parts = list(out.unbind(0))
        dist.all_gather(parts, packed.contiguous(), group=group)
        out = torch.stack(parts, 0)
    else:
        dist.all_gather_into_tensor(out.view(-1), packed.contiguous(), group=group)
    return out


def gather_global(packed, n_local, group=None):
    """Global (obs, term_obs, reward, info, done) numpy arrays in global env-id order (equal shards)."""
    g = all_gather_packed(packed, group).cpu().numpy()
    parts = [unpack(g[r], n_local) for r in range(g.shape[0])]
    return {k: np.concatenate([p[k] for p in parts], 0) for k in parts[0]}


class OverlappedGather:
    """Publishes every rank's packed output block to all ranks WITHOUT stalling the step kernel: the block is copied to one of two
    staging buffers on the compute stream (2 MB device-to-device), and the RCCL all-gather of that copy runs on a side stream while
    the next step's kernel is already executing.  xGMI is point-to-point (ring all-gather, per-link bound), so the ~2 MB per rank
    cost about as much as 10 % of a step when serialised; overlapped they cost nothing but their HBM traffic.

        og = OverlappedGather(batch.packed, world)
        for k in ...:
            batch.step(actions)              # compute stream
            og.publish(batch.packed, k)      # staging copy + all-gather on the side stream
            blocks = og.result(k - 1)        # [world, total] block of the previous step, gathered while this step ran
    On CPU tensors (gloo tests) the same calls run synchronously."""

    def __init__(self, packed, world, group=None):
        import torch
        self.torch, self.group, self.world = torch, group, world
        self.cuda = packed.is_cuda
        self.stage = [torch.empty_like(packed) for _ in range(2)]
        self.out = [torch.empty((world, packed.numel()), dtype=torch.uint8, device=packed.device) for _ in range(2)]
        if self.cuda:
            self.side = torch.cuda.Stream(device=packed.device)
            self.copied = [torch.cuda.Event() for _ in range(2)]
            self.gathered = [torch.cuda.Event() for _ in range(2)]
            self.used = [False, False]

    def publish(self, packed, k):
        import torch.distributed as dist
        b = k & 1
        if not self.cuda:
            self.stage[b].copy_(packed)
            self.out[b] = all_gather_packed(self.stage[b], self.group)
            return
        torch = self.torch
        main = torch.cuda.current_stream(packed.device)
        if self.used[b]:
            main.wait_event(self.gathered[b])      # the gather of step k-2 has finished reading this staging buffer
        self.stage[b].copy_(packed, non_blocking=True)
        self.copied[b].record(main)
        with torch.cuda.stream(self.side):
            self.side.wait_event(self.copied[b])
            dist.all_gather_into_tensor(self.out[b].view(-1), self.stage[b], group=self.group)
            self.gathered[b].record(self.side)
        self.used[b] = True

    def result(self, k):
        """[world, total] uint8 block of step k (k or k-1 relative to the last publish); waits for that gather only."""
        b = k & 1
        if self.cuda:
            self.torch.cuda.current_stream(self.out[b].device).wait_event(self.gathered[b])
        return self.out[b]

    def finish(self):
        if self.cuda:
            self.side.synchronize()
