"""Multi-GPU sharding of the vectorised env: one process per GPU (torchrun), contiguous env ranges.

Envs never interact, so the data path needs no collective: rank r owns global envs
[offset_r, offset_r + count_r) and passes offset_r as `env_offset`, which keys the in-kernel Philox
noise by GLOBAL env id -- results are identical for any number of ranks.  The only optional
exchange is for a single-host policy: gather every rank's observations (and rewards / flags) to one
rank, or all-gather them, over RCCL ("nccl" backend = RCCL on ROCm, xGMI between GPUs).

Per-env goals shard the same way: a box goal (`HeliVecEnv.set_goals(box=...)` on `shard.env`) is drawn from
(seed, GLOBAL env id, episode), so every env meets the same sequence of goals for any number of ranks, and
`heligym_amd.goal_ref` recomputes it from the global id; a goal table is sliced like any [total, ...] array.
"""
import torch
import torch.distributed as dist


def shard_bounds(total, rank, world):
    """(offset, count) of rank's contiguous share of `total` envs; the first total % world ranks
    get one extra env."""
    if world < 1 or not (0 <= rank < world):
        raise ValueError("bad rank/world")
    base, extra = divmod(int(total), int(world))
    count = base + (1 if rank < extra else 0)
    offset = rank * base + min(rank, extra)
    return offset, count


def fleet_shard_tiles(total, offset, count):
    """[lo, hi) of the global 64-env tiles a shard (offset, count) of `total` envs covers; ValueError unless
    the shard starts on a tile and ends on one or at the end of the batch."""
    if offset % 64 != 0 or (count % 64 != 0 and offset + count != total):
        raise ValueError(f"set_fleet: the shard [{offset}, {offset + count}) of {total} envs is not aligned to the "
                         "64-env tiles a fleet's classes are given by")
    return offset // 64, (offset + count + 63) // 64


def _staged(t, group):
    """gloo collectives take host tensors: GPU rows go through the host there (the rehearsal of the
    RCCL path on one GPU; RCCL itself moves device memory over xGMI)."""
    return t.cpu() if t.is_cuda and dist.get_backend(group) == "gloo" else t


def _pad_to(t, rows):
    if t.shape[0] == rows:
        return t
    pad = torch.zeros((rows - t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    return torch.cat([t, pad], 0)


def all_gather_rows(local, total, group=None):
    """All-gather per-rank row blocks (uneven shards allowed) into one [total, ...] tensor on every
    rank, in global env order."""
    world = dist.get_world_size(group)
    counts = [shard_bounds(total, r, world)[1] for r in range(world)]
    m = max(counts)
    x = _staged(_pad_to(local.contiguous(), m), group)
    buf = torch.empty((world * m,) + tuple(local.shape[1:]), dtype=local.dtype, device=x.device)
    dist.all_gather_into_tensor(buf, x, group=group)
    parts = [buf[r * m: r * m + counts[r]] for r in range(world)]
    return torch.cat(parts, 0).to(local.device)


def gather_rows(local, total, dst=0, group=None):
    """Gather per-rank row blocks to rank `dst` only ([total, ...] there, None elsewhere)."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    counts = [shard_bounds(total, r, world)[1] for r in range(world)]
    m = max(counts)
    x = _staged(_pad_to(local.contiguous(), m), group)
    if rank == dst:
        bufs = [torch.empty_like(x) for _ in range(world)]
        dist.gather(x, gather_list=bufs, dst=dst, group=group)
        return torch.cat([bufs[r][:counts[r]] for r in range(world)], 0).to(local.device)
    dist.gather(x, dst=dst, group=group)
    return None


class ShardedHeliVecEnv:
    """This rank's shard of a `total_envs` batch (one GPU per process).  step()/reset() act on the
    local shard only; gather_obs()/all_gather_obs() assemble the global observation batch."""

    def __init__(self, total_envs, rank=None, world=None, group=None, **env_kwargs):
        from .vector import HeliVecEnv
        self.group = group
        self.rank = dist.get_rank(group) if rank is None else rank
        self.world = dist.get_world_size(group) if world is None else world
        self.total_envs = int(total_envs)
        self.offset, self.count = shard_bounds(total_envs, self.rank, self.world)
        self.env = HeliVecEnv(self.count, env_offset=self.offset, **env_kwargs)

    def reset(self, **kw):
        return self.env.reset(**kw)

    def step(self, actions, **kw):
        return self.env.step(actions, **kw)

    def step_async(self, actions, **kw):
        return self.env.step_async(actions, **kw)

    def set_fleet(self, airframes, tile_class=None, **kw):
        """HeliVecEnv.set_fleet on this rank's shard with its slice of a global `tile_class` (one class per
        64 consecutive global envs).  Only the classes this shard's tiles use are set on it (a handle holds at
        most one class per tile); the returned status has the global length, 0 for the others.  The shard's
        bounds must be tile-aligned: its offset a multiple of 64, and its count too unless it is the last shard."""
        import numpy as np
        if airframes is None or tile_class is None:
            return self.env.set_fleet(airframes, tile_class=tile_class, **kw)
        lo, hi = fleet_shard_tiles(self.total_envs, self.offset, self.count)
        tc = tile_class.detach().cpu().numpy() if hasattr(tile_class, "detach") else tile_class
        if len(tc) != (self.total_envs + 63) // 64:
            raise ValueError(f"set_fleet: the global tile_class must have {(self.total_envs + 63) // 64} entries, "
                             f"got {len(tc)}")
        tc = np.asarray(tc)
        if tc.dtype.kind not in "iu" or tc.min() < 0 or tc.max() >= len(airframes):
            raise ValueError(f"set_fleet: tile_class entries must be integers in [0, {len(airframes)})")
        if kw.get("conds") is not None and len(kw["conds"]) != len(airframes):
            raise ValueError(f"set_fleet: need {len(airframes)} trim conditions (one per class), got {len(kw['conds'])}")
        used, local = np.unique(tc[lo:hi], return_inverse=True)
        if kw.get("conds") is not None:
            kw["conds"] = [kw["conds"][c] for c in used]
        status = np.zeros(len(airframes), dtype=np.int32)
        status[used] = self.env.set_fleet([airframes[c] for c in used], tile_class=local.astype(np.int32), **kw)
        return status

    def gather_obs(self, dst=0):
        return gather_rows(self.env.obs, self.total_envs, dst=dst, group=self.group)

    def all_gather_obs(self):
        return all_gather_rows(self.env.obs, self.total_envs, group=self.group)

    def close(self):
        self.env.close()
