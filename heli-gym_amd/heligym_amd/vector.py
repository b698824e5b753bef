"""Batched heli-gym environment on one MI355X: N helicopters advanced by one HIP kernel per step.

`HeliVecEnv` is the vectorised counterpart of the reference's `Heli` gymnasium env
(heligym/envs/helicopter.py:28-243): same 17-observation / 4-action contract, same reward, flags and
setters, with same-step auto-reset.  All buffers are PyTorch-ROCm tensors on the env's device; the
step itself runs in `libheligym_amd.so` (no CPU path exists).
"""
import ctypes

import numpy as np

from . import _abi, config
from . import goals as _goals


class Box:
    """Minimal stand-in for gymnasium.spaces.Box (gymnasium is optional)."""

    def __init__(self, low, high, shape, dtype=np.float32):
        self.low = np.full(shape, low, dtype=dtype)
        self.high = np.full(shape, high, dtype=dtype)
        self.shape = tuple(shape)
        self.dtype = np.dtype(dtype)

    def sample(self, rng=np.random):
        lo = np.where(np.isfinite(self.low), self.low, -1.0)
        hi = np.where(np.isfinite(self.high), self.high, 1.0)
        return rng.uniform(lo, hi).astype(self.dtype)

    def contains(self, x):
        x = np.asarray(x)
        return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))


def _make_box(low, high, shape):
    try:  # use the real class when gymnasium is installed
        from gymnasium import spaces
        return spaces.Box(low, high, shape=shape, dtype=np.float32)
    except ImportError:
        return Box(low, high, shape)


class LazyInfo(dict):
    """The info dict of HeliVecEnv.step(): keys present at once, each value computed on first
    access (then cached).  `valid()` says whether the step's buffers still hold its values; reading
    a field after they were reused raises instead of returning another step's data."""

    def __init__(self, thunks, valid, gen=None):
        """thunks: key -> f(info) computing the value (shared between steps: per-step state goes
        on the info object).  valid: () -> bool; or, with `gen`, the env whose step `gen` this is:
        the values stay readable while env._gen - gen < 2 (the step's buffer set is not reused
        before the step after next)."""
        super().__init__(dict.fromkeys(thunks))
        self._thunks = thunks
        self._pending = set(thunks)
        self._src = valid
        self._gen = gen

    def _valid(self):
        return self._src() if self._gen is None else self._src._gen - self._gen < 2

    def _get(self, k):
        if k in self._pending:
            if not self._valid():
                raise _abi.HeliGymError(f"info[{k!r}] read after its buffers were reused (read info before "
                                        "the step after next)")
            dict.__setitem__(self, k, self._thunks[k](self))
            self._pending.discard(k)
        return dict.__getitem__(self, k)

    def __getitem__(self, k):
        return self._get(k)

    def get(self, k, default=None):
        return self._get(k) if k in self else default

    def __iter__(self):
        return iter(list(dict.keys(self)))

    def items(self):
        return [(k, self._get(k)) for k in list(dict.keys(self))]

    def values(self):
        return [self._get(k) for k in list(dict.keys(self))]

    def copy(self):
        return {k: self._get(k) for k in list(dict.keys(self))}

    # every other read path goes through _get as well, so no caller ever sees a None placeholder
    def __setitem__(self, k, v):
        self._pending.discard(k)
        dict.__setitem__(self, k, v)

    def update(self, *args, **kw):
        for k, v in dict(*args, **kw).items():
            self[k] = v

    _MISSING = object()

    def pop(self, k, default=_MISSING):
        if k not in self:
            if default is LazyInfo._MISSING:
                raise KeyError(k)
            return default
        v = self._get(k)
        dict.pop(self, k)
        return v

    def popitem(self):
        if not len(self):
            raise KeyError("popitem(): dictionary is empty")
        k = list(dict.keys(self))[-1]
        return k, self.pop(k)

    def setdefault(self, k, default=None):
        if k in self:
            return self._get(k)
        dict.__setitem__(self, k, default)
        return default

    def __reduce__(self):   # pickles / deep-copies as the plain dict of its values
        return (dict, (self.copy(),))

    def __deepcopy__(self, memo):
        import copy
        return copy.deepcopy(self.copy(), memo)

    def __repr__(self):
        return repr(self.copy())

    def __eq__(self, other):
        return self.copy() == (other.copy() if isinstance(other, LazyInfo) else other)

    __hash__ = None


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


OBS_NAMES = ("POWER", "LON_AIR_SPD", "LAT_AIR_SPD", "DWN_AIR_SPD", "N_VEL", "E_VEL", "DES_RATE",
             "ROLL", "PITCH", "YAW", "ROLL_RATE", "PITCH_RATE", "YAW_RATE",
             "N_POS", "E_POS", "ALTITUDE", "GROUND_ALTITUDE")   # helicopter_dynamics.py:23-25


try:   # gymnasium.vector.VectorEnv lineage when gymnasium is installed (optional)
    from gymnasium.vector import VectorEnv as _VectorEnv
    _VEC_BASES = (_VectorEnv,)
except ImportError:
    _VEC_BASES = (object,)


class HeliVecEnv(*_VEC_BASES):
    """N independent helicopters (one `hg_env` handle) on one GPU.

    task: "hover" (HeliHover), "forward_flight" (HeliForwardFlight) or "heli" (Heli, reward 0).
    autoreset: finished envs are reset inside the step kernel; the returned observation row is
      the reset observation and the terminal one is in info["final_obs"] (rows of
      info["reset_index"]).  With autoreset=False, finished envs keep integrating until reset().
    env_offset: global id of env 0 (multi-GPU sharding keeps the noise stream of each env fixed).
    """

    metadata = {"render.modes": [], "video.frames_per_second": config.FPS}   # helicopter.py:29-32

    def __init__(self, num_envs, task="hover", dt=config.DT, heli_name="aw109", seed=0, device=None,
                 autoreset=True, env_offset=0, max_time=None, target=None, trim_cond=None,
                 turbulence_level=None, reset_mode="template", autoreset_mode="same_step",
                 max_episode_steps=None, terrain=None, specialize=False):
        import torch
        self.torch = torch
        self.lib = _abi.load_library()
        if not torch.cuda.is_available():
            raise _abi.HeliGymError("HeliVecEnv needs a HIP device (no CPU fallback)")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.num_envs = int(num_envs)
        self.task = task
        self.dt = float(dt)
        self.autoreset = bool(autoreset)
        self.cfg, doc = config.make_config(task=task, dt=dt, heli_name=heli_name, max_time=max_time,
                                           target=target, trim_cond=trim_cond, autoreset=autoreset,
                                           seed=seed, env_offset=env_offset,
                                           turbulence_level=turbulence_level, reset_mode=reset_mode,
                                           autoreset_mode=autoreset_mode, max_episode_steps=max_episode_steps)
        self.reset_mode = reset_mode
        self.autoreset_mode = autoreset_mode
        self.max_episode_steps = max_episode_steps
        # terrain: the airframe document's map, or a path / uint16 samples / float heights in ft
        if terrain is None or isinstance(terrain, str):
            u16 = config.load_terrain(doc) if terrain is None else config.read_terrain(terrain)
            self.terrain_ft = config.terrain_ft(u16, self.cfg.af.env_MAX_GR_ALT)
        else:
            t = np.asarray(terrain)
            self.terrain_ft = (config.terrain_ft(t, self.cfg.af.env_MAX_GR_ALT) if t.dtype == np.uint16
                               else np.ascontiguousarray(t, dtype=np.float64))
        if self.terrain_ft.ndim != 2:
            raise ValueError("terrain must be a 2-D map")
        self._target = dict(config.DEFAULT_TARGETS[task])
        self._target.update(target or {})
        self._trim_cond = config.fill_trim(_abi.hg_trim_cond(), trim_cond)
        self.max_time = self.cfg.max_time
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _abi.check(self.lib.hg_create(ctypes.byref(self.cfg), self.terrain_ft.ctypes.data,
                                          self.terrain_ft.shape[0], self.terrain_ft.shape[1],
                                          self.num_envs, ctypes.byref(h)), self.lib)
        self._h = h
        self._specialized = bool(self.lib.hg_set_specialized(h, 1))
        if specialize and not self._specialized:
            self.specialize()
        N, dev = self.num_envs, self.device
        f32, u8, i32 = torch.float32, torch.uint8, torch.int32
        self.obs = torch.empty((N, _abi.HG_N_OBS), dtype=f32, device=dev)
        self.reward = torch.empty((N,), dtype=f32, device=dev)
        self.terminated_u8 = torch.empty((N,), dtype=u8, device=dev)
        self.truncated_u8 = torch.empty((N,), dtype=u8, device=dev)
        # info bits and reset info alternate between two buffer sets from step to step, so that the
        # lazily evaluated info of step() stays valid until the step after next (no copies, no sync)
        self._sets = [dict(info=torch.zeros((N,), dtype=u8, device=dev),
                           index=torch.empty((N,), dtype=i32, device=dev),
                           final=torch.empty((N, _abi.HG_N_OBS), dtype=f32, device=dev)) for _ in range(2)]
        # reset counts rotate over three buffers: step k counts into ring[k % 3], which step k-1
        # zeroed from inside its kernel (hg_step_chained: no separate zeroing launch), and zeroes
        # ring[(k + 1) % 3]; step k's count is so readable until the step after next
        self._count_ring = torch.zeros((3,), dtype=i32, device=dev)
        self._ring_views = [self._count_ring[j:j + 1] for j in range(3)]
        self._p_ring = [v.data_ptr() for v in self._ring_views]
        # the per-step host path passes plain addresses (no per-call tensor -> pointer conversions)
        # and reads the current stream through torch's raw-stream accessor
        self._dev_index = dev.index if dev.index is not None else torch.cuda.current_device()
        self._raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        self._p_obs, self._p_rew = self.obs.data_ptr(), self.reward.data_ptr()
        self._p_term, self._p_trunc = self.terminated_u8.data_ptr(), self.truncated_u8.data_ptr()
        self._term_b, self._trunc_b = self.terminated_u8.view(torch.bool), self.truncated_u8.view(torch.bool)
        self._act_shape = (N, _abi.HG_N_ACT)
        for b in self._sets:
            b["count"] = self._ring_views[0]
            b["p"] = tuple(b[k].data_ptr() for k in ("info", "index", "final"))
            b["thunks"] = self._info_thunks(b)
            b["thunks_rows"] = self._info_thunks(b, rows=True)
            # step()'s hg_step_rows arguments after the actions, before the stream
            b["rows_args"] = (self._p_obs, self._p_rew, self._p_term, self._p_trunc, b["p"][0], None, b["p"][2])
        self._f32 = torch.float32
        self._step_rows = self.lib.hg_step_rows
        # step()'s direct path: same-step auto-reset with reset info (what _launch(rows=True) does),
        # and a raw-stream accessor to read the current stream with
        self._rows_fast = self.autoreset and self.autoreset_mode == "same_step" and self._raw_stream is not None
        self._gen = 0
        self._use_set(0)
        # gymnasium.vector's convention: one env's spaces (helicopter.py:56-57) and the batched ones
        self.single_observation_space = _make_box(-np.inf, np.inf, (_abi.HG_N_OBS,))
        self.single_action_space = _make_box(-1.0, 1.0, (_abi.HG_N_ACT,))
        self.observation_space = _make_box(-np.inf, np.inf, (N, _abi.HG_N_OBS))
        self.action_space = _make_box(-1.0, 1.0, (N, _abi.HG_N_ACT))
        self.normalizers = {                                                     # helicopter.py:63-68
            "t": float(np.sqrt(2 * self.cfg.af.mr_R / self.cfg.af.env_GRAV)),
            "x": 2 * self.cfg.af.mr_R,
            "v": float(np.sqrt(2 * self.cfg.af.mr_R * self.cfg.af.env_GRAV)),
            "a": self.cfg.af.env_GRAV,
        }

    # ------------------------------------------------------------------ plumbing
    def _use_set(self, g):
        b = self._sets[g & 1]
        b["count"] = self._ring_views[g % 3]
        self.info_u8, self.reset_count, self.reset_index, self.final_obs = b["info"], b["count"], b["index"], b["final"]
        return b

    def _stream(self):
        if self._raw_stream is not None:
            return ctypes.c_void_p(self._raw_stream(self._dev_index))
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _info_thunks(self, b, rows=False):
        """The lazy info fields of a step that used buffer set b: key -> f(info).  rows: the step
        went through hg_step_rows (reset envs flagged by HG_INFO_RESET, terminal observations at
        their own rows of b["final"]), else its reset info is the compacted one."""
        bits, index, final = b["info"], b["index"], b["final"]
        th = {"failed": lambda i: (bits & _abi.HG_INFO_FAILED) != 0,
              "successed": lambda i: (bits & _abi.HG_INFO_SUCCESSED) != 0,
              "time_up": lambda i: (bits & _abi.HG_INFO_TIME_UP) != 0,
              "success_step": lambda i: (bits & _abi.HG_INFO_SUCCESS_STEP) != 0}
        if self.autoreset and self.autoreset_mode == "same_step" and rows:
            def resets(i):   # (sorted env ids, their terminal observations); one nonzero per step
                r = getattr(i, "_resets", None)
                if r is None:
                    idx = self.torch.nonzero(bits & _abi.HG_INFO_RESET).flatten()
                    r = i._resets = (idx, final.index_select(0, idx))
                return r
            th["reset_index"] = lambda i: resets(i)[0]
            th["final_obs"] = lambda i: resets(i)[1]
        elif self.autoreset and self.autoreset_mode == "same_step":
            def resets(i):   # (sorted env ids, their terminal observations); one host read per step
                r = getattr(i, "_resets", None)
                if r is None:
                    k = int(b["count"].item())   # this set's step's ring slot
                    idx = index[:k].long()
                    order = self.torch.argsort(idx)
                    r = i._resets = (idx[order], final[:k][order])
                return r
            th["reset_index"] = lambda i: resets(i)[0]
            th["final_obs"] = lambda i: resets(i)[1]
        return th

    def _check(self, rc):
        return _abi.check(rc, self.lib)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.hg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ gym surface
    def reset(self, seed=None, options=None, mask=None):
        """Heli.reset (helicopter.py:208-217) for all envs, or for the envs where `mask` != 0.
        Returns (obs [N,17], info) like the reference (obs rows of unmasked envs untouched)."""
        m = None
        if mask is not None:
            m = self.torch.as_tensor(mask, device=self.device).to(self.torch.uint8).contiguous()
        self._check(self.lib.hg_reset(self._h, _ptr(m), _ptr(self.obs), self._stream()))
        tr = self.template()
        N = self.num_envs
        info = {"failed": self.torch.full((N,), bool(tr["failed"]), device=self.device),
                "successed": self.torch.zeros((N,), dtype=self.torch.bool, device=self.device),
                "time_up": self.torch.zeros((N,), dtype=self.torch.bool, device=self.device)}
        return self.obs, info

    def step_async(self, actions, eta=None, with_reset_info=True, obs_out=None):
        """Launch one step on the current stream and return immediately (no host sync).
        actions: float32 [N,4] device tensor.  eta: optional float32 [N,3] injected turbulence noise
        (already scaled by 1/sqrt(dt)), else in-kernel Philox.  obs_out: optional float32 [N,17]
        device tensor (16-byte aligned) the observations go to instead of `self.obs` (double
        buffering, e.g. while a previous step's observations are being gathered)."""
        self._launch(actions, eta, with_reset_info, obs_out)

    def _launch(self, actions, eta, with_reset_info, obs_out, rows=False):
        """step_async's launch; returns the buffer set the step's info went to.  rows: the reset
        info uncompacted (hg_step_rows, step()'s path), else compacted (hg_step_chained)."""
        a = actions
        if a.dtype != self.torch.float32 or not a.is_contiguous() or a.device != self.device:
            a = a.to(device=self.device, dtype=self.torch.float32).contiguous()
        if a.shape != self._act_shape:
            raise ValueError(f"actions must be [{self.num_envs}, 4], got {tuple(a.shape)}")
        e = None
        if eta is not None:
            e = eta.to(device=self.device, dtype=self.torch.float32).contiguous()
            if tuple(e.shape) != (self.num_envs, 3):
                raise ValueError("eta must be [N, 3]")
        p_obs = self._p_obs
        if obs_out is not None:
            if (obs_out.dtype != self.torch.float32 or obs_out.device != self.device or not obs_out.is_contiguous()
                    or tuple(obs_out.shape) != (self.num_envs, _abi.HG_N_OBS)):
                raise ValueError(f"obs_out must be a contiguous float32 [{self.num_envs}, 17] tensor on {self.device}")
            p_obs = obs_out.data_ptr()
        self._keep = (a, e, obs_out)
        self._gen += 1
        b = self._use_set(self._gen)
        p = b["p"]
        rs = with_reset_info and self.autoreset and self.autoreset_mode == "same_step"
        g = self._gen
        if not rs or rows:
            # only a compacted step (step_async with reset info) fills these; after any other step
            # they would hold another step's data
            self.reset_count = self.reset_index = self.final_obs = None
        if rs and rows:
            rc = self.lib.hg_step_rows(self._h, a.data_ptr(), p_obs, self._p_rew, self._p_term, self._p_trunc, p[0],
                                       None if e is None else e.data_ptr(), p[2], self._stream())
        elif rs:
            rc = self.lib.hg_step_chained(self._h, a.data_ptr(), p_obs, self._p_rew, self._p_term, self._p_trunc,
                                          p[0], None if e is None else e.data_ptr(), self._p_ring[g % 3], p[1], p[2],
                                          self._p_ring[(g + 1) % 3], self._stream())
        else:
            rc = self.lib.hg_step(self._h, a.data_ptr(), p_obs, self._p_rew, self._p_term, self._p_trunc, p[0],
                                  None if e is None else e.data_ptr(), None, None, None, self._stream())
        if rc:
            self._check(rc)
        return b

    def step(self, actions, eta=None):
        """Heli.step (helicopter.py:192-206) for all envs: (obs, reward, terminated, truncated, info).
        Returned tensors are the env's buffers, overwritten by the next step.  `info` is evaluated
        lazily: a field costs its device ops (and, for the same-step reset info, a read of the reset
        count) only when it is read, which must happen before the step after next.  The reset info
        comes uncompacted (hg_step_rows: the reset envs' info bytes carry HG_INFO_RESET and their
        terminal observations sit at their own rows), so the step is the plain kernel launch."""
        a = actions
        # the common call (a float32 [N,4] contiguous tensor on the env's device, in-kernel noise) goes
        # straight to hg_step_rows with the buffer set's addresses packed at construction: the host
        # cost per call is then the launch's, not the argument handling's
        if (eta is None and self._rows_fast and a.dtype is self._f32 and a.is_contiguous()
                and a.shape == self._act_shape and a.get_device() == self._dev_index):
            g = self._gen = self._gen + 1
            b = self._sets[g & 1]
            self.info_u8 = b["info"]
            if self.reset_count is not None:   # (only a compacted step fills these)
                self.reset_count = self.reset_index = self.final_obs = None
            self._keep = (a, None, None)
            rc = self._step_rows(self._h, a.data_ptr(), *b["rows_args"], self._raw_stream(self._dev_index))
            if rc:
                self._check(rc)
            return self.obs, self.reward, self._term_b, self._trunc_b, LazyInfo(b["thunks_rows"], self, g)
        b = self._launch(actions, eta, True, None, rows=True)
        return self.obs, self.reward, self._term_b, self._trunc_b, LazyInfo(b["thunks_rows"], self, self._gen)

    # ------------------------------------------------------------------ setters (helicopter.py:89-111)
    def set_max_time(self, max_time=None):
        self.max_time = config.DEFAULT_MAX_TIME if max_time is None else float(max_time)
        self._check(self.lib.hg_set_max_time(self._h, self.max_time))

    def set_target(self, target=None):
        new = dict(self._target)
        new.update(target or {})
        tg = _abi.hg_target()
        config.fill_target(tg, new)
        self._check(self.lib.hg_set_target(self._h, ctypes.byref(tg)))   # (refused while per-env goals are set)
        self._target = new

    def get_target(self):
        return dict(self._target)

    def set_specialized(self, enable=True):
        """Allow / forbid the step kernel with the default airframe's constants compiled in
        (csrc/baked.h; bitwise-identical results).  Returns whether it is in use."""
        rc = self.lib.hg_set_specialized(self._h, 1 if enable else 0)
        if rc < 0:
            self._check(rc)
        self._specialized = bool(rc)
        return self._specialized

    def set_retrim_overlap(self, enable=True):
        """reset_mode="retrim": with next-step auto-reset, trim the episodes a step ends while the next
        step runs (True, the default; False: always serial).  enable=2 also trims, with same-step
        auto-reset, a step's resets in the step's own launch as soon as each env's step is done (opt-in:
        bitwise the serial results but slower on MI355X).  hg_set_retrim_overlap.  Returns whether the
        next-step overlap is in effect."""
        mode = 2 if (enable == 2 and enable is not True) else (1 if enable else 0)
        rc = self.lib.hg_set_retrim_overlap(self._h, mode)
        if rc < 0:
            self._check(rc)
        return bool(rc)

    @property
    def specialized(self):
        """True when steps run a constant-specialised kernel: the library's own for the default AW109
        airframe (its constants compiled in; every step and rollout, with or without the optional
        features), or a run-time specialised one for any other airframe (specialize())."""
        return self._specialized

    def specialize(self):
        """Step this env with a kernel specialised for its airframe's constants (heligym_amd._rtc:
        compiled with hipcc on the first request for these constants, ~4 s, then cached), the way the
        default airframe always is: per-step launches with in-kernel noise use it, results bitwise
        those of the generic kernel.  Returns whether a specialised kernel is in use."""
        if self._specialized:
            return True
        from . import _rtc
        rows, cols = self.terrain_ft.shape
        path, img = _rtc.build(self.lib, self.cfg, rows, cols, self.cfg.task)
        buf = ctypes.create_string_buffer(img, len(img))
        rc = self.lib.hg_load_specialized(self._h, path.encode(), self.cfg.task, buf, len(img))
        if rc < 0:
            self._check(rc)
        self._specialized = bool(rc)
        return self._specialized

    def set_trim_cond(self, trim_cond=None):
        cur = self.get_trim_cond()
        cur.update(trim_cond or {})
        tc = _abi.hg_trim_cond()
        self._trim_cond = config.fill_trim(tc, cur)
        self._check(self.lib.hg_set_trim_cond(self._h, ctypes.byref(tc)))

    def get_trim_cond(self):
        import copy
        return copy.deepcopy(self._trim_cond)

    def template(self):
        r = _abi.hg_trim_result()
        self._check(self.lib.hg_get_template(self._h, ctypes.byref(r)))
        return {"state": np.array(r.state), "action": np.array(r.action), "obs": np.array(r.obs),
                "state_dots": np.array(r.state_dots), "residual": r.residual,
                "iterations": r.iterations, "failed": bool(r.failed)}

    # ------------------------------------------------------------------ state access
    def get_state(self):
        """(state [N,27] float32, counters [N,3] int32): heli 18 | wind 5 | carry 4.

        The rotor azimuths (columns 2, 3) are reconstructed from a per-env record (each step adds
        dt * Omega and wraps, bitwise what the step would have carried); the cost is one add-and-wrap
        per step since the env's last reset, set_state or get_state, and each call re-anchors the
        records, so a run that reads its state now and then keeps every read short."""
        t = self.torch
        s = t.empty((self.num_envs, _abi.HG_STATE_COLS), dtype=t.float32, device=self.device)
        c = t.empty((self.num_envs, _abi.HG_COUNTER_COLS), dtype=t.int32, device=self.device)
        self._check(self.lib.hg_get_state(self._h, _ptr(s), _ptr(c), self._stream()))
        return s, c

    def set_state(self, state=None, counters=None):
        t = self.torch
        s = None if state is None else t.as_tensor(state, device=self.device, dtype=t.float32).contiguous()
        c = None if counters is None else t.as_tensor(counters, device=self.device, dtype=t.int32).contiguous()
        if s is not None and tuple(s.shape) != (self.num_envs, _abi.HG_STATE_COLS):
            raise ValueError("state must be [N, 27]")
        if c is not None and tuple(c.shape) != (self.num_envs, _abi.HG_COUNTER_COLS):
            raise ValueError("counters must be [N, 3]")
        self._check(self.lib.hg_set_state(self._h, _ptr(s), _ptr(c), self._stream()))
        self._keep_state = (s, c)

    def rollout(self, actions, eta=None, out=None):
        """Open-loop rollout (hg_rollout): actions [K,N,4] applied over K consecutive steps in one
        launch, identical to K step() calls.  Returns (obs [K,N,17], reward [K,N], terminated,
        truncated [K,N] bool, info bits [K,N] uint8) device tensors (`out` buffers are reused if
        given, as returned by a previous call)."""
        t = self.torch
        a = actions
        if a.dtype != t.float32 or not a.is_contiguous() or a.device != self.device:
            a = a.to(device=self.device, dtype=t.float32).contiguous()
        if a.ndim != 3 or tuple(a.shape[1:]) != (self.num_envs, _abi.HG_N_ACT):
            raise ValueError(f"actions must be [K, {self.num_envs}, 4], got {tuple(a.shape)}")
        K, N = a.shape[0], self.num_envs
        e = None
        if eta is not None:
            e = eta.to(device=self.device, dtype=t.float32).contiguous()
            if tuple(e.shape) != (K, N, 3):
                raise ValueError("eta must be [K, N, 3]")
        if out is None or out[0].shape[0] != K:
            out = (t.empty((K, N, _abi.HG_N_OBS), dtype=t.float32, device=self.device),
                   t.empty((K, N), dtype=t.float32, device=self.device),
                   t.empty((K, N), dtype=t.uint8, device=self.device),
                   t.empty((K, N), dtype=t.uint8, device=self.device),
                   t.empty((K, N), dtype=t.uint8, device=self.device))
        obs, rew, term, trunc, info = out
        self._keep = (a, e)
        self._check(self.lib.hg_rollout(self._h, _ptr(a), K, _ptr(obs), _ptr(rew), _ptr(term), _ptr(trunc),
                                        _ptr(info), _ptr(e), self._stream()))
        return out

    # ------------------------------------------------------------------ closed-loop policy rollouts
    def set_policy(self, model_or_pairs, log_std=None, obs_mean=None, obs_scale=None):
        """Give the env its MLP policy (hg_set_policy): three (W, b) pairs or an nn.Sequential of
        Linear(17, 64) / Tanh / Linear(64, 64) / Tanh / Linear(64, 4), fp32 (heligym_amd.policy).
        log_std [4]: the action noise's log standard deviation, None for a deterministic policy;
        obs_mean / obs_scale [17]: the input normalisation x = (obs - obs_mean) * obs_scale.
        The weights are copied into the handle's own buffer on the current stream (no allocation, no
        sync, capturable): call it again after every update of the model."""
        from . import policy
        t = self.torch
        packed = policy.pack_policy(model_or_pairs, log_std, obs_mean, obs_scale)
        dev = tuple(None if p is None else p.to(device=self.device, dtype=t.float32).contiguous() for p in packed)
        self._keep_policy = dev
        self._check(self.lib.hg_set_policy(self._h, *(_ptr(p) for p in dev), self._stream()))

    def _obs_arg(self, obs, name):
        if obs is None:
            return self.obs
        t = self.torch
        if (obs.dtype != t.float32 or obs.device != self.device or not obs.is_contiguous()
                or tuple(obs.shape) != (self.num_envs, _abi.HG_N_OBS)):
            raise ValueError(f"{name} must be a contiguous float32 [{self.num_envs}, 17] tensor on {self.device}, "
                             f"got {tuple(obs.shape)} {obs.dtype} on {obs.device}")
        return obs

    def policy_act(self, obs=None, out=None):
        """The policy's actions [N,4] for the observations `obs` [N,17] (default: `self.obs`) with the
        noise of each env's current counters (hg_policy_act); the env is not modified.  policy_act then
        step(), repeated, is bitwise rollout_policy()."""
        t = self.torch
        o = self._obs_arg(obs, "obs")
        if out is None:
            out = t.empty(self._act_shape, dtype=t.float32, device=self.device)
        elif (tuple(out.shape) != self._act_shape or out.dtype != t.float32 or out.device != self.device
              or not out.is_contiguous()):
            raise ValueError(f"policy_act: out must be a contiguous float32 {self._act_shape} tensor on {self.device}")
        self._check(self.lib.hg_policy_act(self._h, _ptr(o), _ptr(out), self._stream()))
        return out

    def rollout_policy(self, K, obs0=None, eta=None, out=None):
        """Closed-loop rollout (hg_rollout_policy): K steps in one launch, each step's action computed
        in the kernel by the env's policy (set_policy) from the observation the previous step wrote,
        the first from `obs0` [N,17] (default: `self.obs`).  Returns (actions [K,N,4], obs [K,N,17],
        reward [K,N], terminated, truncated, info bits [K,N] uint8) device tensors (`out` buffers are
        reused if given, as returned by a previous call); `self.obs` is not written, so pass
        `obs[-1]` as the next call's obs0.  The action noise is keyed by each env's global id and its
        own counters, so sharding the envs over several HeliVecEnv (env_offset) changes nothing
        (ShardedHeliVecEnv itself does not expose the policy calls)."""
        t = self.torch
        K, N = int(K), self.num_envs
        o0 = self._obs_arg(obs0, "obs0")
        e = None
        if eta is not None:
            e = eta.to(device=self.device, dtype=t.float32).contiguous()
            if tuple(e.shape) != (K, N, 3):
                raise ValueError("eta must be [K, N, 3]")
        if out is None or out[0].shape[0] != K:
            out = (t.empty((K, N, _abi.HG_N_ACT), dtype=t.float32, device=self.device),
                   t.empty((K, N, _abi.HG_N_OBS), dtype=t.float32, device=self.device),
                   t.empty((K, N), dtype=t.float32, device=self.device),
                   t.empty((K, N), dtype=t.uint8, device=self.device),
                   t.empty((K, N), dtype=t.uint8, device=self.device),
                   t.empty((K, N), dtype=t.uint8, device=self.device))
        act, obs, rew, term, trunc, info = out
        self._keep = (o0, e)
        self._check(self.lib.hg_rollout_policy(self._h, _ptr(o0), K, _ptr(act), _ptr(obs), _ptr(rew), _ptr(term),
                                               _ptr(trunc), _ptr(info), _ptr(e), self._stream()))
        return out

    # ------------------------------------------------------------------ actor-critic rollouts
    AC_KEYS = ("actions", "obs", "reward", "terminated", "truncated", "info", "logp", "value", "next_value",
               "advantages", "returns")

    def set_value_head(self, head):
        """Give the policy a value head v = w_v . tanh(h2) + b_v on its trunk (hg_set_value_head): an
        nn.Linear(64, 1) or a (w, b) pair (heligym_amd.policy.pack_value_head).  Independent of
        set_policy: either order, and a later set_policy keeps the head.  Copied on the current stream
        (no allocation, no sync, capturable): call it again after every update."""
        from . import policy
        t = self.torch
        dev = tuple(p.to(device=self.device, dtype=t.float32).contiguous() for p in policy.pack_value_head(head))
        self._keep_value_head = dev
        self._check(self.lib.hg_set_value_head(self._h, _ptr(dev[0]), _ptr(dev[1]), self._stream()))

    def policy_evaluate(self, obs=None):
        """(actions [N,4], logp [N], value [N]) of the policy and its value head for the observations
        `obs` [N,17] (default: `self.obs`), with the noise of each env's current counters
        (hg_policy_eval); the env is not modified.  policy_evaluate then step(), repeated, is bitwise
        rollout_actor_critic()'s actions, logp and value."""
        t = self.torch
        o = self._obs_arg(obs, "obs")
        act = t.empty(self._act_shape, dtype=t.float32, device=self.device)
        logp = t.empty((self.num_envs,), dtype=t.float32, device=self.device)
        val = t.empty((self.num_envs,), dtype=t.float32, device=self.device)
        self._check(self.lib.hg_policy_eval(self._h, _ptr(o), _ptr(act), _ptr(logp), _ptr(val), self._stream()))
        return act, logp, val

    def _gae_rows(self, x, dtype, name, K):
        t = self.torch
        if x.dtype == t.bool and dtype == t.uint8:
            x = x.view(t.uint8)
        if (x.dtype != dtype or x.device != self.device or not x.is_contiguous() or x.ndim != 2
                or x.shape[0] != K or x.shape[1] != self.num_envs):
            raise ValueError(f"gae: {name} must be a contiguous {dtype} [{K}, {self.num_envs}] tensor on {self.device}, "
                             f"got {tuple(x.shape)} {x.dtype} on {x.device}")
        return x

    def gae(self, reward, value, next_value, terminated, truncated, gamma=0.99, lam=0.95, out=None):
        """Generalised advantage estimation (hg_gae) over [K,N] device rows, for rollout_actor_critic's
        outputs or a caller's own critic's values:
            delta_k = reward[k] + gamma next_value[k] - value[k]
            A_k = delta_k + gamma lam (terminated[k] | truncated[k] ? 0 : A_{k+1}),  A_K = 0
        Returns (advantages, returns = advantages + value), [K,N] float32 (`out`: such a pair to reuse)."""
        t = self.torch
        K = int(reward.shape[0])
        r = self._gae_rows(reward, t.float32, "reward", K)
        v = self._gae_rows(value, t.float32, "value", K)
        nv = self._gae_rows(next_value, t.float32, "next_value", K)
        te = self._gae_rows(terminated, t.uint8, "terminated", K)
        tr = self._gae_rows(truncated, t.uint8, "truncated", K)
        if out is None:
            out = (t.empty_like(r), t.empty_like(r))
        adv = self._gae_rows(out[0], t.float32, "out[0]", K)
        ret = self._gae_rows(out[1], t.float32, "out[1]", K)
        self._keep_gae = (r, v, nv, te, tr)
        self._check(self.lib.hg_gae(self._h, _ptr(r), _ptr(v), _ptr(nv), _ptr(te), _ptr(tr), K, float(gamma), float(lam),
                                    _ptr(adv), _ptr(ret), self._stream()))
        return out

    def rollout_actor_critic(self, K, gamma=0.99, lam=0.95, obs0=None, eta=None, out=None):
        """rollout_policy with what a PPO / A2C learner needs beside it, from the same launch
        (hg_rollout_ac, then hg_gae on the same stream).  Returns a dict of device tensors:
        rollout_policy's six (actions, obs, reward, terminated, truncated, info), bitwise the same, and
            logp [K,N]        log pi(a_k | o_k), o_k the observation a_k was computed from
            value [K,N]       V(o_k) of the value head (set_value_head)
            next_value [K,N]  terminated[k] ? 0 : V(observation step k produced before any auto-reset)
            advantages, returns [K,N]  GAE(gamma, lam) of them
        `out`: a dict returned by a previous call with the same K, whose buffers are reused.  Not
        available with autoreset_mode="next_step"."""
        t = self.torch
        K, N = int(K), self.num_envs
        o0 = self._obs_arg(obs0, "obs0")
        e = None
        if eta is not None:
            e = eta.to(device=self.device, dtype=t.float32).contiguous()
            if tuple(e.shape) != (K, N, 3):
                raise ValueError("eta must be [K, N, 3]")
        if out is None or out["actions"].shape[0] != K:
            f32 = lambda *s: t.empty(s, dtype=t.float32, device=self.device)   # noqa: E731
            u8 = lambda: t.empty((K, N), dtype=t.uint8, device=self.device)   # noqa: E731
            out = dict(actions=f32(K, N, _abi.HG_N_ACT), obs=f32(K, N, _abi.HG_N_OBS), reward=f32(K, N), terminated=u8(),
                       truncated=u8(), info=u8(), logp=f32(K, N), value=f32(K, N), next_value=f32(K, N),
                       advantages=f32(K, N), returns=f32(K, N))
        self._keep = (o0, e)
        p = {k: _ptr(out[k]) for k in self.AC_KEYS}
        self._check(self.lib.hg_rollout_ac(self._h, _ptr(o0), K, p["actions"], p["obs"], p["reward"], p["terminated"],
                                           p["truncated"], p["info"], _ptr(e), p["logp"], p["value"], p["next_value"],
                                           self._stream()))
        self._check(self.lib.hg_gae(self._h, p["reward"], p["value"], p["next_value"], p["terminated"], p["truncated"],
                                    K, float(gamma), float(lam), p["advantages"], p["returns"], self._stream()))
        return out

    # ------------------------------------------------------------------ the PPO update's gradient
    def _ppo_tensor(self, x, shape, name, dtype=None):
        t = self.torch
        dtype = t.float32 if dtype is None else dtype
        if (not isinstance(x, t.Tensor) or x.dtype != dtype or x.device != self.device or not x.is_contiguous()
                or tuple(x.shape) != tuple(shape)):
            got = f"{tuple(x.shape)} {x.dtype} on {x.device}" if isinstance(x, t.Tensor) else type(x).__name__
            raise ValueError(f"ppo_grad: {name} must be a contiguous {dtype} {tuple(shape)} tensor on {self.device}, "
                             f"got {got}")
        return x

    def _workspace(self):
        """hg_ppo_grad's workspace for the per-block partial sums, allocated once per env."""
        ws = getattr(self, "_ppo_workspace", None)
        if ws is None:
            ws = self._ppo_workspace = self.torch.empty((int(self.lib.hg_ppo_grad_workspace_bytes()),),
                                                        dtype=self.torch.uint8, device=self.device)
        return ws

    def ppo_grad(self, params, obs, actions, logp_old, adv, ret, index=None, clip=0.2, vf_coef=1.0, ent_coef=0.0,
                 obs_mean=None, obs_scale=None, stats=None):
        """The clipped PPO loss's gradient over a minibatch in one kernel (hg_ppo_grad; the loss is
        heligym_amd.policy.ppo_loss).  params: an ActorCriticParams on this device (its `theta` is read,
        its `grad` overwritten).  obs [B,17], actions [B,4], logp_old / adv / ret [B]: the stored rows
        (rollout_actor_critic's outputs, flattened; leading dimensions are merged), contiguous float32 on
        the env's device.  index: int32 [M] rows of the minibatch (entries outside [0, B) are skipped and
        counted in stats[7]), or None for all B rows in order.  obs_mean / obs_scale [17]: the policy's
        input normalisation.  Returns (params.grad, stats [8]: policy term, value term, approximate KL,
        clip fraction, entropy, loss, mean ratio, skipped entries); `stats`: a float32 [8] tensor to reuse.
        Asynchronous on the current stream, allocates nothing after the first call, capturable; the env
        is not modified."""
        t = self.torch
        theta = self._ppo_tensor(getattr(params, "theta", None), (_abi.HG_PPO_N_PARAMS,), "params.theta")
        grad = self._ppo_tensor(getattr(params, "grad", None), (_abi.HG_PPO_N_PARAMS,), "params.grad")
        if not isinstance(obs, t.Tensor) or obs.ndim < 2 or obs.shape[-1] != _abi.HG_N_OBS:
            raise ValueError("ppo_grad: obs must be a [..., 17] tensor")
        B = int(obs.numel() // _abi.HG_N_OBS)
        if B < 1:
            raise ValueError("ppo_grad: obs has no rows")
        lead = tuple(obs.shape[:-1])
        o = self._ppo_tensor(obs, lead + (_abi.HG_N_OBS,), "obs")
        a = self._ppo_tensor(actions, lead + (_abi.HG_N_ACT,), "actions")
        lp = self._ppo_tensor(logp_old, lead, "logp_old")
        ad = self._ppo_tensor(adv, lead, "adv")
        rt = self._ppo_tensor(ret, lead, "ret")
        M, ix = B, None
        if index is not None:
            if not isinstance(index, t.Tensor) or index.ndim != 1 or index.shape[0] < 1:
                raise ValueError("ppo_grad: index must be a non-empty int32 [M] tensor")
            M = int(index.shape[0])
            ix = self._ppo_tensor(index, (M,), "index", t.int32)
        mean = None if obs_mean is None else self._ppo_tensor(obs_mean, (_abi.HG_N_OBS,), "obs_mean")
        scale = None if obs_scale is None else self._ppo_tensor(obs_scale, (_abi.HG_N_OBS,), "obs_scale")
        if stats is None:
            stats = t.empty((8,), dtype=t.float32, device=self.device)
        st = self._ppo_tensor(stats, (8,), "stats")
        ws = self._workspace()
        self._keep_ppo = (theta, o, a, lp, ad, rt, ix, mean, scale)
        self._check(self.lib.hg_ppo_grad(self._h, _ptr(theta), _ptr(mean), _ptr(scale), _ptr(o), _ptr(a), _ptr(lp),
                                         _ptr(ad), _ptr(rt), B, _ptr(ix), M, float(clip), float(vf_coef),
                                         float(ent_coef), _ptr(grad), _ptr(st), _ptr(ws), self._stream()))
        return grad, st

    # ------------------------------------------------------------------ the PPO update on the device
    def _opt_tensor(self, x, shape, name, dtype=None, who="ppo_update"):
        t = self.torch
        dtype = t.float32 if dtype is None else dtype
        if (not isinstance(x, t.Tensor) or x.dtype != dtype or x.device != self.device or not x.is_contiguous()
                or tuple(x.shape) != tuple(shape)):
            got = f"{tuple(x.shape)} {x.dtype} on {x.device}" if isinstance(x, t.Tensor) else type(x).__name__
            raise ValueError(f"{who}: {name} must be a contiguous {dtype} {tuple(shape)} tensor on {self.device}, got {got}")
        return x

    def _opt_cfg(self, who, lr, betas, eps, max_grad_norm, target_kl, lr_dev):
        """The hg_ppo_opt_cfg of the keyword arguments (ValueError for what hg_ppo_adam would refuse)."""
        import math
        try:
            lr, eps, (b1, b2) = float(lr), float(eps), (float(b) for b in betas)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: lr and eps must be numbers and betas a pair of numbers") from None
        if not math.isfinite(lr) or lr < 0:
            raise ValueError(f"{who}: lr must be finite and >= 0, got {lr}")
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"{who}: betas must be in [0, 1), got {(b1, b2)}")
        if not math.isfinite(eps) or eps < 0:
            raise ValueError(f"{who}: eps must be finite and >= 0, got {eps}")
        mg = 0.0 if max_grad_norm is None else float(max_grad_norm)
        kl = 0.0 if target_kl is None else float(target_kl)
        if math.isnan(mg) or math.isnan(kl):
            raise ValueError(f"{who}: max_grad_norm and target_kl must not be NaN")
        p = None
        if lr_dev is not None:
            t = self.torch
            if (not isinstance(lr_dev, t.Tensor) or lr_dev.dtype != t.float32 or lr_dev.device != self.device
                    or lr_dev.numel() != 1):
                raise ValueError(f"{who}: lr_dev must be a float32 tensor of one element on {self.device}")
            p = lr_dev.data_ptr()
        return _abi.hg_ppo_opt_cfg(lr, p, b1, b2, eps, mg, kl)

    def _opt_state(self, state, who):
        from . import policy
        s = getattr(state, "state", None)
        return self._opt_tensor(s, (policy.PPO_OPT_WORDS,), "state.state (a PPOOptState)", self.torch.int32, who)

    def ppo_shuffle(self, B, seed, epoch=0, epoch_dev=None, out=None):
        """A stateless random permutation of 0..B-1 as an int32 [B] device tensor (hg_ppo_shuffle: a keyed
        Feistel network with cycle walking, no sort).  The key is (seed, epoch + *epoch_dev): epoch_dev, an
        int32 device tensor of one element (a PPOOptState's `seen`), is read when the kernel runs."""
        t = self.torch
        B = int(B)
        if B < 1 or B > 2 ** 31 - 256:
            raise ValueError(f"ppo_shuffle: B must be in 1 .. 2^31 - 256, got {B}")
        if epoch_dev is not None and (not isinstance(epoch_dev, t.Tensor) or epoch_dev.dtype != t.int32
                                      or epoch_dev.device != self.device or epoch_dev.numel() != 1):
            raise ValueError(f"ppo_shuffle: epoch_dev must be an int32 tensor of one element on {self.device}")
        if out is None:
            out = t.empty((B,), dtype=t.int32, device=self.device)
        out = self._opt_tensor(out, (B,), "out", t.int32, "ppo_shuffle")
        self._keep_shuffle = epoch_dev
        self._check(self.lib.hg_ppo_shuffle(self._h, B, int(seed) & (2 ** 64 - 1), int(epoch), _ptr(epoch_dev), _ptr(out),
                                            self._stream()))
        return out

    def ppo_adam(self, params, state, stats=None, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None,
                 target_kl=None, lr_dev=None):
        """One optimiser step on the device (hg_ppo_adam): params.theta is updated in place from params.grad
        (not modified) and `state` (a PPOOptState): the approximate-KL early stop on `stats` [8] (ppo_grad's,
        of the same minibatch; with target_kl), the non-finite guard, global gradient-norm clipping
        (max_grad_norm, torch's clip_grad_norm_) and Adam with fp64 bias corrections.  lr_dev: a float32
        device tensor of one element read when the kernel runs, in place of lr.  Asynchronous, allocates
        nothing, capturable."""
        theta = self._opt_tensor(getattr(params, "theta", None), (_abi.HG_PPO_N_PARAMS,), "params.theta", who="ppo_adam")
        grad = self._opt_tensor(getattr(params, "grad", None), (_abi.HG_PPO_N_PARAMS,), "params.grad", who="ppo_adam")
        st = None if stats is None else self._opt_tensor(stats, (8,), "stats", who="ppo_adam")
        s = self._opt_state(state, "ppo_adam")
        cfg = self._opt_cfg("ppo_adam", lr, betas, eps, max_grad_norm, target_kl, lr_dev)
        self._keep_adam = (theta, grad, st, s, lr_dev)
        self._check(self.lib.hg_ppo_adam(self._h, _ptr(theta), _ptr(grad), _ptr(st), _ptr(s), ctypes.byref(cfg),
                                         self._stream()))
        return theta

    def set_policy_theta(self, params, obs_mean=None, obs_scale=None):
        """set_policy + set_value_head from the flat vector params.theta (hg_set_policy_theta), bitwise those
        two calls on the actor, log_std and the critic; on the current stream, capturable."""
        theta = self._opt_tensor(getattr(params, "theta", None), (_abi.HG_PPO_N_PARAMS,), "params.theta",
                                 who="set_policy_theta")
        mean = None if obs_mean is None else self._opt_tensor(obs_mean, (_abi.HG_N_OBS,), "obs_mean", who="set_policy_theta")
        scale = None if obs_scale is None else self._opt_tensor(obs_scale, (_abi.HG_N_OBS,), "obs_scale",
                                                                who="set_policy_theta")
        self._keep_policy_theta = (theta, mean, scale)
        self._check(self.lib.hg_set_policy_theta(self._h, _ptr(theta), _ptr(mean), _ptr(scale), self._stream()))

    def ppo_update(self, params, state, obs, actions, logp_old, adv, ret, epochs=4, minibatches=4, seed=0, clip=0.2,
                   vf_coef=1.0, ent_coef=0.0, obs_mean=None, obs_scale=None, lr=3e-4, betas=(0.9, 0.999), eps=1e-8,
                   max_grad_norm=None, target_kl=None, lr_dev=None, stats=None, index=None, publish=False):
        """The whole update phase in one call (hg_ppo_update): `epochs` times a fresh permutation of the B
        stored rows (keyed by `seed` and the state's `seen` counter), cut into `minibatches` slices, and for
        each slice ppo_grad then ppo_adam, all enqueued on the current stream with no host decision in
        between.  The rows are ppo_grad's (leading dimensions are merged), the optimiser's arguments
        ppo_adam's.  Returns the statistics rows [epochs * minibatches, 8] (`stats`: such a tensor to reuse);
        `index`: an int32 [B] scratch tensor to reuse (it holds the last epoch's permutation afterwards).
        publish=True ends with set_policy_theta(params, obs_mean, obs_scale).  Bitwise the same calls made
        one by one; allocates nothing after the first call with these shapes; capturable."""
        t = self.torch
        who = "ppo_update"
        theta = self._opt_tensor(getattr(params, "theta", None), (_abi.HG_PPO_N_PARAMS,), "params.theta")
        grad = self._opt_tensor(getattr(params, "grad", None), (_abi.HG_PPO_N_PARAMS,), "params.grad")
        s = self._opt_state(state, who)
        if not isinstance(obs, t.Tensor) or obs.ndim < 2 or obs.shape[-1] != _abi.HG_N_OBS:
            raise ValueError("ppo_update: obs must be a [..., 17] tensor")
        B = int(obs.numel() // _abi.HG_N_OBS)
        if B < 1 or B > 2 ** 31 - 256:
            raise ValueError(f"ppo_update: obs must have 1 .. 2^31 - 256 rows, got {B}")
        lead = tuple(obs.shape[:-1])
        o = self._opt_tensor(obs, lead + (_abi.HG_N_OBS,), "obs")
        a = self._opt_tensor(actions, lead + (_abi.HG_N_ACT,), "actions")
        lp = self._opt_tensor(logp_old, lead, "logp_old")
        ad = self._opt_tensor(adv, lead, "adv")
        rt = self._opt_tensor(ret, lead, "ret")
        epochs, minibatches = int(epochs), int(minibatches)
        if epochs < 1:
            raise ValueError(f"ppo_update: epochs must be >= 1, got {epochs}")
        if minibatches < 1 or minibatches > B:
            raise ValueError(f"ppo_update: minibatches must be in 1 .. {B} (the rows), got {minibatches}")
        mean = None if obs_mean is None else self._opt_tensor(obs_mean, (_abi.HG_N_OBS,), "obs_mean")
        scale = None if obs_scale is None else self._opt_tensor(obs_scale, (_abi.HG_N_OBS,), "obs_scale")
        cfg = self._opt_cfg(who, lr, betas, eps, max_grad_norm, target_kl, lr_dev)
        if stats is None:
            stats = getattr(self, "_ppo_update_stats", None)
            if stats is None or tuple(stats.shape) != (epochs * minibatches, 8):
                stats = self._ppo_update_stats = t.empty((epochs * minibatches, 8), dtype=t.float32, device=self.device)
        st = self._opt_tensor(stats, (epochs * minibatches, 8), "stats")
        if index is None:
            index = getattr(self, "_ppo_update_index", None)
            if index is None or tuple(index.shape) != (B,):
                index = self._ppo_update_index = t.empty((B,), dtype=t.int32, device=self.device)
        ix = self._opt_tensor(index, (B,), "index", t.int32)
        ws = self._workspace()
        self._keep_ppo_update = (theta, grad, s, o, a, lp, ad, rt, mean, scale, st, ix, lr_dev)
        self._check(self.lib.hg_ppo_update(self._h, _ptr(theta), _ptr(mean), _ptr(scale), _ptr(o), _ptr(a), _ptr(lp),
                                           _ptr(ad), _ptr(rt), B, float(clip), float(vf_coef), float(ent_coef), _ptr(grad),
                                           _ptr(ws), epochs, minibatches, int(seed) & (2 ** 64 - 1), _ptr(ix), _ptr(st),
                                           _ptr(s), ctypes.byref(cfg), self._stream()))
        if publish:
            self.set_policy_theta(params, mean, scale)
        return st

    # ------------------------------------------------------------------ the imitation loss: gradient and update
    def _bc_rows(self, who, obs, target, weight, value_target, mode, vf_coef, ent_coef, obs_mean, obs_scale):
        """The checked row tensors and scalars bc_grad and bc_update share (ValueError for what needs no device)."""
        import math
        t = self.torch
        if mode not in _abi.BC_MODES:
            raise ValueError(f"{who}: mode must be one of {sorted(_abi.BC_MODES)}, got {mode!r}")
        vf_coef, ent_coef = float(vf_coef), float(ent_coef)
        if not (math.isfinite(vf_coef) and vf_coef >= 0 and math.isfinite(ent_coef) and ent_coef >= 0):
            raise ValueError(f"{who}: vf_coef and ent_coef must be finite and >= 0, got {vf_coef}, {ent_coef}")
        if value_target is None and vf_coef != 0:
            raise ValueError(f"{who}: value_target is None, so vf_coef must be 0, got {vf_coef}")
        if not isinstance(obs, t.Tensor) or obs.ndim < 2 or obs.shape[-1] != _abi.HG_N_OBS:
            raise ValueError(f"{who}: obs must be a [..., 17] tensor")
        B = int(obs.numel() // _abi.HG_N_OBS)
        if B < 1 or B > 2 ** 31 - 256:
            raise ValueError(f"{who}: obs must have 1 .. 2^31 - 256 rows, got {B}")
        lead = tuple(obs.shape[:-1])
        o = self._opt_tensor(obs, lead + (_abi.HG_N_OBS,), "obs", who=who)
        a = self._opt_tensor(target, lead + (_abi.HG_N_ACT,), "target", who=who)
        w = None if weight is None else self._opt_tensor(weight, lead, "weight", who=who)
        y = None if value_target is None else self._opt_tensor(value_target, lead, "value_target", who=who)
        mean = None if obs_mean is None else self._opt_tensor(obs_mean, (_abi.HG_N_OBS,), "obs_mean", who=who)
        scale = None if obs_scale is None else self._opt_tensor(obs_scale, (_abi.HG_N_OBS,), "obs_scale", who=who)
        return B, o, a, w, y, mean, scale, _abi.BC_MODES[mode], vf_coef, ent_coef

    def bc_grad(self, params, obs, target, weight=None, value_target=None, index=None, mode="nll", vf_coef=0.0,
                ent_coef=0.0, obs_mean=None, obs_scale=None, stats=None):
        """The weighted imitation loss's gradient over a minibatch in one kernel (hg_bc_grad; the loss is
        heligym_amd.policy.bc_loss): a regression of the policy's Gaussian onto `target` [B,4] at `obs` [B,17]
        plus a value regression onto `value_target` [B].  mode "nll": -logp(target), log_std is trained;
        "mse": 1/2 |target - mean|^2.  weight [B] or None (1) multiplies each row's action term;
        value_target None needs vf_coef == 0.  params, index, obs_mean / obs_scale, stats: as ppo_grad's.
        Returns (params.grad, stats [8]: weighted action term, value term, mean squared action error, mean
        weight, entropy, loss, mean logp(target), skipped entries).  Asynchronous on the current stream,
        allocates nothing after the first call, capturable; the env is not modified."""
        t = self.torch
        who = "bc_grad"
        theta = self._opt_tensor(getattr(params, "theta", None), (_abi.HG_PPO_N_PARAMS,), "params.theta", who=who)
        grad = self._opt_tensor(getattr(params, "grad", None), (_abi.HG_PPO_N_PARAMS,), "params.grad", who=who)
        B, o, a, w, y, mean, scale, m, vf_coef, ent_coef = self._bc_rows(who, obs, target, weight, value_target, mode,
                                                                         vf_coef, ent_coef, obs_mean, obs_scale)
        M, ix = B, None
        if index is not None:
            if not isinstance(index, t.Tensor) or index.ndim != 1 or index.shape[0] < 1:
                raise ValueError("bc_grad: index must be a non-empty int32 [M] tensor")
            M = int(index.shape[0])
            ix = self._opt_tensor(index, (M,), "index", t.int32, who)
        if stats is None:
            stats = t.empty((8,), dtype=t.float32, device=self.device)
        st = self._opt_tensor(stats, (8,), "stats", who=who)
        ws = self._workspace()
        self._keep_bc = (theta, o, a, w, y, ix, mean, scale)
        self._check(self.lib.hg_bc_grad(self._h, _ptr(theta), _ptr(mean), _ptr(scale), _ptr(o), _ptr(a), _ptr(w), _ptr(y),
                                        B, _ptr(ix), M, m, vf_coef, ent_coef, _ptr(grad), _ptr(st), _ptr(ws),
                                        self._stream()))
        return grad, st

    def bc_update(self, params, state, obs, target, weight=None, value_target=None, epochs=4, minibatches=4, seed=0,
                  mode="nll", vf_coef=0.0, ent_coef=0.0, obs_mean=None, obs_scale=None, lr=3e-4, betas=(0.9, 0.999),
                  eps=1e-8, max_grad_norm=None, lr_dev=None, stats=None, index=None, publish=True):
        """ppo_update's loop with bc_grad as the gradient (hg_bc_update): `epochs` fresh permutations of the B
        rows, `minibatches` slices each, bc_grad then ppo_adam per slice, one call, no host decision in
        between.  The rows and the loss's arguments are bc_grad's, the optimiser's ppo_adam's (there is no
        KL early stop: this loss has no KL).  Returns the statistics rows [epochs * minibatches, 8].
        publish=True ends with set_policy_theta(params, obs_mean, obs_scale): the env acts with the
        distilled weights.  Bitwise the same calls made one by one; capturable."""
        t = self.torch
        who = "bc_update"
        theta = self._opt_tensor(getattr(params, "theta", None), (_abi.HG_PPO_N_PARAMS,), "params.theta", who=who)
        grad = self._opt_tensor(getattr(params, "grad", None), (_abi.HG_PPO_N_PARAMS,), "params.grad", who=who)
        s = self._opt_state(state, who)
        B, o, a, w, y, mean, scale, m, vf_coef, ent_coef = self._bc_rows(who, obs, target, weight, value_target, mode,
                                                                         vf_coef, ent_coef, obs_mean, obs_scale)
        epochs, minibatches = int(epochs), int(minibatches)
        if epochs < 1:
            raise ValueError(f"bc_update: epochs must be >= 1, got {epochs}")
        if minibatches < 1 or minibatches > B:
            raise ValueError(f"bc_update: minibatches must be in 1 .. {B} (the rows), got {minibatches}")
        cfg = self._opt_cfg(who, lr, betas, eps, max_grad_norm, None, lr_dev)
        if stats is None:
            stats = getattr(self, "_bc_update_stats", None)
            if stats is None or tuple(stats.shape) != (epochs * minibatches, 8):
                stats = self._bc_update_stats = t.empty((epochs * minibatches, 8), dtype=t.float32, device=self.device)
        st = self._opt_tensor(stats, (epochs * minibatches, 8), "stats", who=who)
        if index is None:
            index = getattr(self, "_ppo_update_index", None)
            if index is None or tuple(index.shape) != (B,):
                index = self._ppo_update_index = t.empty((B,), dtype=t.int32, device=self.device)
        ix = self._opt_tensor(index, (B,), "index", t.int32, who)
        ws = self._workspace()
        self._keep_bc_update = (theta, grad, s, o, a, w, y, mean, scale, st, ix, lr_dev)
        self._check(self.lib.hg_bc_update(self._h, _ptr(theta), _ptr(mean), _ptr(scale), _ptr(o), _ptr(a), _ptr(w), _ptr(y),
                                          B, m, vf_coef, ent_coef, _ptr(grad), _ptr(ws), epochs, minibatches,
                                          int(seed) & (2 ** 64 - 1), _ptr(ix), _ptr(st), _ptr(s), ctypes.byref(cfg),
                                          self._stream()))
        if publish:
            self.set_policy_theta(params, mean, scale)
        return st

    # ------------------------------------------------------------------ running normalisation, episode statistics
    def rollout_stats(self, stats, rollout, gamma=0.99, obs0=None, obs_in=None, reward_out=None, update_obs=True,
                      update_ret=True, obs_eps=1e-8, ret_eps=1e-8, max_obs_scale=None, clip_reward=None):
        """Running normalisation and episode statistics of one rollout (hg_rollout_stats; the function is
        heligym_amd.stats.rollout_stats_ref).  stats: a RolloutStats of this env; rollout: what
        rollout_actor_critic (a dict) or rollout_policy (a tuple) returned, read as it is.  Updates the running
        moments of the observations and of the discounted return (gamma) and the per-env episode return /
        length, which persist from call to call, and fills stats.obs_mean / obs_scale (float32 [17], from the
        moments AFTER this batch: the next collection's normalisation), stats.reward_scale [1] and
        stats.episode [16] (stats.EPISODE_FIELDS: episodes completed in this call, their return's mean / std /
        min / max, mean length, terminated / truncated / success counts, ...).
        reward_out: a float32 [K,N] tensor (not the rollout's reward) for clamp(reward * reward_scale,
        +-clip_reward).  obs_in: a float32 [K,N,17] tensor for the observations the actions were computed from
        (obs0, obs[0], .., obs[K-2]), with obs0 [N,17], the rollout's start.  update_obs / update_ret False
        freeze that part (evaluation); max_obs_scale / clip_reward None: unbounded.  Returns `stats`.
        Asynchronous on the current stream, allocates nothing, capturable; the env is not modified."""
        import math
        from . import stats as _stats
        t = self.torch
        who = "rollout_stats"
        if not isinstance(stats, _stats.RolloutStats):
            raise ValueError(f"{who}: stats must be a RolloutStats, got {type(stats).__name__}")
        if isinstance(rollout, dict):
            try:
                obs, rew, term, trunc = (rollout[k] for k in ("obs", "reward", "terminated", "truncated"))
            except KeyError as e:
                raise ValueError(f"{who}: rollout has no {e.args[0]!r}") from None
            info = rollout.get("info")
        elif isinstance(rollout, (tuple, list)) and len(rollout) == 6:
            _, obs, rew, term, trunc, info = rollout
        else:
            raise ValueError(f"{who}: rollout must be rollout_actor_critic's dict or rollout_policy's tuple of six")
        if not isinstance(rew, t.Tensor) or rew.ndim != 2 or rew.shape[0] < 1:
            raise ValueError(f"{who}: reward must be a [K, N] tensor")
        K, N = int(rew.shape[0]), self.num_envs
        state = self._opt_tensor(stats.state, (_stats.stats_state_bytes(N) // 4,), "stats.state", t.int32, who)
        o = self._opt_tensor(obs, (K, N, _abi.HG_N_OBS), "obs", who=who)
        r = self._opt_tensor(rew, (K, N), "reward", who=who)
        te = self._opt_tensor(term, (K, N), "terminated", t.uint8, who)
        tr = self._opt_tensor(trunc, (K, N), "truncated", t.uint8, who)
        inf = None if info is None else self._opt_tensor(info, (K, N), "info", t.uint8, who)
        if obs_in is not None and obs0 is None:
            raise ValueError(f"{who}: obs_in needs obs0, the observations the rollout started from")
        o0 = None if obs0 is None else self._opt_tensor(obs0, (N, _abi.HG_N_OBS), "obs0", who=who)
        oi = None if obs_in is None else self._opt_tensor(obs_in, (K, N, _abi.HG_N_OBS), "obs_in", who=who)
        ro = None if reward_out is None else self._opt_tensor(reward_out, (K, N), "reward_out", who=who)
        if ro is not None and (ro is r or ro.data_ptr() == r.data_ptr()):
            raise ValueError(f"{who}: reward_out must not be the rollout's reward")
        outs = [self._opt_tensor(getattr(stats, k), s, f"stats.{k}", who=who)
                for k, s in (("obs_mean", (_abi.HG_N_OBS,)), ("obs_scale", (_abi.HG_N_OBS,)), ("reward_scale", (1,)),
                             ("episode", (16,)))]
        try:
            gamma, obs_eps, ret_eps = float(gamma), float(obs_eps), float(ret_eps)
            mos = math.inf if max_obs_scale is None else float(max_obs_scale)
            clip = math.inf if clip_reward is None else float(clip_reward)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: gamma, the eps, max_obs_scale and clip_reward must be numbers") from None
        if not 0.0 <= gamma <= 1.0:
            raise ValueError(f"{who}: gamma must be in [0, 1], got {gamma}")
        if not (0.0 <= obs_eps < math.inf and 0.0 <= ret_eps < math.inf):
            raise ValueError(f"{who}: obs_eps and ret_eps must be finite and >= 0, got {(obs_eps, ret_eps)}")
        if not (mos > 0.0 and clip > 0.0):
            raise ValueError(f"{who}: max_obs_scale and clip_reward must be > 0, got {(mos, clip)}")
        update = (_abi.HG_STATS_UPDATE_OBS if update_obs else 0) | (_abi.HG_STATS_UPDATE_RET if update_ret else 0)
        cfg = _abi.hg_rollout_stats_cfg(gamma, obs_eps, ret_eps, mos, clip, update, 0)
        self._keep_stats = (state, o, r, te, tr, inf, o0, oi, ro, outs)
        self._check(self.lib.hg_rollout_stats(self._h, _ptr(state), _ptr(o), _ptr(r), _ptr(te), _ptr(tr), _ptr(inf),
                                              _ptr(o0), K, ctypes.byref(cfg), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
                                              _ptr(ro), _ptr(oi), _ptr(outs[3]), self._stream()))
        return stats

    # ------------------------------------------------------------------ populations and evolution strategies
    def _pop_count(self, P, who, even=False, cap=65536):
        P = int(P)
        if P < (2 if even else 1) or P > cap or (even and P % 2):
            raise ValueError(f"{who}: the population must be {'even, ' if even else ''}in {2 if even else 1} .. {cap}, got {P}")
        return P

    def _pop_members(self, P, envs_per_member, who):
        P, m = self._pop_count(P, who), int(envs_per_member)
        if m < 64 or m % 64:
            raise ValueError(f"{who}: envs_per_member must be a positive multiple of 64, got {m}")
        if not (P - 1) * m < self.num_envs <= P * m:
            raise ValueError(f"{who}: {P} members of {m} envs do not cover {self.num_envs} envs "
                             f"(need (P - 1) * envs_per_member < num_envs <= P * envs_per_member)")
        return P, m

    def _pop_norm(self, obs_mean, obs_scale, who):
        mean = None if obs_mean is None else self._opt_tensor(obs_mean, (_abi.HG_N_OBS,), "obs_mean", who=who)
        scale = None if obs_scale is None else self._opt_tensor(obs_scale, (_abi.HG_N_OBS,), "obs_scale", who=who)
        return mean, scale

    def _gen_dev(self, gen_dev, who):
        t = self.torch
        if gen_dev is not None and (not isinstance(gen_dev, t.Tensor) or gen_dev.dtype != t.int32
                                    or gen_dev.device != self.device or gen_dev.numel() != 1):
            raise ValueError(f"{who}: gen_dev must be an int32 tensor of one element on {self.device}")
        return gen_dev

    def _sigma(self, sigma, who):
        import math
        sigma = float(sigma)
        if not math.isfinite(sigma) or sigma <= 0:
            raise ValueError(f"{who}: sigma must be finite and > 0, got {sigma}")
        return sigma

    def pop_pack(self, thetas, stochastic=True, obs_mean=None, obs_scale=None, out=None):
        """P packed policy images [P, 7552] from P flat parameter vectors `thetas` [P, 5641] in one launch
        (hg_pop_pack): image p is bitwise what set_policy_theta of thetas[p] leaves in a handle, value head
        included; stochastic=False gives deterministic policies (set_policy without log_std).  obs_mean /
        obs_scale [17] are shared.  `out`: a float32 [P, 7552] tensor to reuse."""
        t = self.torch
        if not isinstance(thetas, t.Tensor) or thetas.ndim != 2:
            raise ValueError("pop_pack: thetas must be a [P, 5641] tensor")
        P = self._pop_count(thetas.shape[0], "pop_pack")
        th = self._opt_tensor(thetas, (P, _abi.HG_PPO_N_PARAMS), "thetas", who="pop_pack")
        mean, scale = self._pop_norm(obs_mean, obs_scale, "pop_pack")
        if out is None:
            out = t.empty((P, _abi.HG_POLICY_IMAGE_FLOATS), dtype=t.float32, device=self.device)
        out = self._opt_tensor(out, (P, _abi.HG_POLICY_IMAGE_FLOATS), "out", who="pop_pack")
        self._keep_pop_pack = (th, mean, scale)
        self._check(self.lib.hg_pop_pack(self._h, _ptr(th), P, 1 if stochastic else 0, _ptr(mean), _ptr(scale), _ptr(out),
                                         self._stream()))
        return out

    def rollout_population(self, K, images, envs_per_member, obs0=None, out=None):
        """rollout_policy with one policy per block of `envs_per_member` consecutive envs (hg_rollout_pop):
        member p, image images[p] of a [P, 7552] population (pop_pack, es_perturb), drives envs
        p * envs_per_member .. ; the last member may be short.  Same outputs as rollout_policy, member p's
        rows bitwise those of a separate handle with that policy.  The env's own policy is not used."""
        t = self.torch
        K, N = int(K), self.num_envs
        if not isinstance(images, t.Tensor) or images.ndim != 2:
            raise ValueError("rollout_population: images must be a [P, 7552] tensor")
        P, m = self._pop_members(images.shape[0], envs_per_member, "rollout_population")
        im = self._opt_tensor(images, (P, _abi.HG_POLICY_IMAGE_FLOATS), "images", who="rollout_population")
        o0 = self._obs_arg(obs0, "obs0")
        if out is None or out[0].shape[0] != K:
            out = (t.empty((K, N, _abi.HG_N_ACT), dtype=t.float32, device=self.device),
                   t.empty((K, N, _abi.HG_N_OBS), dtype=t.float32, device=self.device),
                   t.empty((K, N), dtype=t.float32, device=self.device),
                   t.empty((K, N), dtype=t.uint8, device=self.device),
                   t.empty((K, N), dtype=t.uint8, device=self.device),
                   t.empty((K, N), dtype=t.uint8, device=self.device))
        act, obs, rew, term, trunc, info = out
        self._keep_pop = (o0, im)
        self._check(self.lib.hg_rollout_pop(self._h, _ptr(im), P, m, _ptr(o0), K, _ptr(act), _ptr(obs), _ptr(rew),
                                            _ptr(term), _ptr(trunc), _ptr(info), self._stream()))
        return out

    def es_perturb(self, params, population, sigma, seed, gen=0, gen_dev=None, stochastic=True, obs_mean=None,
                   obs_scale=None, out=None, member_theta=None):
        """The images [P, 7552] of an antithetic ES population around params.theta (or a flat tensor; hg_es_perturb): members
        2j and 2j+1 are theta +- sigma eps_j on the 5572 actor-mean parameters, eps from counters keyed by
        (seed, pair, gen + *gen_dev) and never stored.  member_theta: a float32 [P, 5641] tensor that also
        receives the members' parameter vectors.  Returns the images."""
        t = self.torch
        theta = params if isinstance(params, t.Tensor) else getattr(params, "theta", None)
        theta = self._opt_tensor(theta, (_abi.HG_PPO_N_PARAMS,), "params.theta", who="es_perturb")
        P = self._pop_count(population, "es_perturb", even=True)
        sigma = self._sigma(sigma, "es_perturb")
        gd = self._gen_dev(gen_dev, "es_perturb")
        mean, scale = self._pop_norm(obs_mean, obs_scale, "es_perturb")
        if out is None:
            out = t.empty((P, _abi.HG_POLICY_IMAGE_FLOATS), dtype=t.float32, device=self.device)
        out = self._opt_tensor(out, (P, _abi.HG_POLICY_IMAGE_FLOATS), "out", who="es_perturb")
        mt = None if member_theta is None else self._opt_tensor(member_theta, (P, _abi.HG_PPO_N_PARAMS), "member_theta",
                                                                who="es_perturb")
        self._keep_es_perturb = (theta, gd, mean, scale, mt)
        self._check(self.lib.hg_es_perturb(self._h, _ptr(theta), P, sigma, int(seed) & (2 ** 64 - 1), int(gen), _ptr(gd),
                                           1 if stochastic else 0, _ptr(mean), _ptr(scale), _ptr(out), _ptr(mt),
                                           self._stream()))
        return out

    def es_noise(self, seed, pair, gen=0, gen_dev=None, out=None):
        """eps_pair [5572] as es_perturb and es_grad compute it (hg_es_noise; a diagnostic, like debug_eta)."""
        t = self.torch
        gd = self._gen_dev(gen_dev, "es_noise")
        if out is None:
            out = t.empty((_abi.HG_ES_N_PERTURBED,), dtype=t.float32, device=self.device)
        out = self._opt_tensor(out, (_abi.HG_ES_N_PERTURBED,), "out", who="es_noise")
        self._keep_es_noise = gd
        self._check(self.lib.hg_es_noise(self._h, int(seed) & (2 ** 64 - 1), int(gen), _ptr(gd), int(pair), _ptr(out),
                                         self._stream()))
        return out

    def pop_fitness(self, reward, terminated, truncated, population, envs_per_member, sums, mode="window", restart=False,
                    alive=None, out=None):
        """Per-member fitness of a population rollout's rewards [K, N] (hg_pop_fitness), accumulated across
        calls in `sums` (float64 [P]): mode "window" counts every reward, "first_episode" each env's rewards
        up to its first terminated | truncated since the last restart (`alive`: uint8 [N], required).
        restart=True clears sums and alive first.  Returns out (float32 [P]) = sums / member env count."""
        t = self.torch
        if mode not in _abi.POP_FIT_MODES:
            raise ValueError(f"pop_fitness: mode must be one of {sorted(_abi.POP_FIT_MODES)}, got {mode!r}")
        P, m = self._pop_members(population, envs_per_member, "pop_fitness")
        if not isinstance(reward, t.Tensor) or reward.ndim != 2:
            raise ValueError("pop_fitness: reward must be a [K, N] tensor")
        K, N = int(reward.shape[0]), self.num_envs
        r = self._opt_tensor(reward, (K, N), "reward", who="pop_fitness")
        first = mode == "first_episode"
        te = None if terminated is None and not first else self._opt_tensor(terminated, (K, N), "terminated", t.uint8,
                                                                            "pop_fitness")
        tr = None if truncated is None and not first else self._opt_tensor(truncated, (K, N), "truncated", t.uint8,
                                                                           "pop_fitness")
        if first and alive is None:
            raise ValueError("pop_fitness: mode 'first_episode' needs alive (uint8 [N])")
        al = None if alive is None else self._opt_tensor(alive, (N,), "alive", t.uint8, "pop_fitness")
        s = self._opt_tensor(sums, (P,), "sums", t.float64, "pop_fitness")
        if out is None:
            out = t.empty((P,), dtype=t.float32, device=self.device)
        out = self._opt_tensor(out, (P,), "out", who="pop_fitness")
        self._keep_pop_fit = (r, te, tr, al, s)
        self._check(self.lib.hg_pop_fitness(self._h, _ptr(r), _ptr(te), _ptr(tr), K, P, m, _abi.POP_FIT_MODES[mode],
                                            1 if restart else 0, _ptr(al), _ptr(s), _ptr(out), self._stream()))
        return out

    def _es_workspace(self, P):
        ws = getattr(self, "_es_ws", None)
        need = int(self.lib.hg_es_workspace_bytes(P))
        if ws is None or ws.numel() < need:
            ws = self._es_ws = self.torch.empty((need,), dtype=self.torch.uint8, device=self.device)
        return ws

    def es_grad(self, params, fitness, sigma, seed, gen=0, gen_dev=None, stats=None):
        """The ES gradient estimate into params.grad (or a flat tensor; hg_es_grad): centred ranks of `fitness` [P] (non-finite
        ones rank lowest), grad = -1/(P sigma) sum_j (u_2j - u_2j+1) eps_j with eps regenerated from
        es_perturb's counters, zero outside the 5572 perturbed parameters; ppo_adam on it ascends the fitness.
        Returns (params.grad, stats [8]: mean, min, max of the finite fitnesses, non-finite count, best index,
        gradient norm, 0, 0).  The workspace is allocated once per population size, before any capture."""
        t = self.torch
        grad = params if isinstance(params, t.Tensor) else getattr(params, "grad", None)
        grad = self._opt_tensor(grad, (_abi.HG_PPO_N_PARAMS,), "params.grad", who="es_grad")
        if not isinstance(fitness, t.Tensor) or fitness.ndim != 1:
            raise ValueError("es_grad: fitness must be a [P] tensor")
        P = self._pop_count(fitness.shape[0], "es_grad", even=True, cap=_abi.HG_ES_MAX_POP)
        f = self._opt_tensor(fitness, (P,), "fitness", who="es_grad")
        sigma = self._sigma(sigma, "es_grad")
        gd = self._gen_dev(gen_dev, "es_grad")
        if stats is None:
            stats = t.empty((8,), dtype=t.float32, device=self.device)
        st = self._opt_tensor(stats, (8,), "stats", who="es_grad")
        ws = self._es_workspace(P)
        self._keep_es_grad = (f, gd)
        self._check(self.lib.hg_es_grad(self._h, _ptr(f), P, sigma, int(seed) & (2 ** 64 - 1), int(gen), _ptr(gd),
                                        _ptr(grad), _ptr(st), _ptr(ws), self._stream()))
        return grad, st

    def debug_policy_image(self, set_to=None, out=None):
        """The env's own packed policy image [7552] (a diagnostic); set_to: install that image instead."""
        t = self.torch
        if set_to is not None:
            im = self._opt_tensor(set_to, (_abi.HG_POLICY_IMAGE_FLOATS,), "set_to", who="debug_policy_image")
            self._check(self.lib.hg_debug_set_policy_image(self._h, _ptr(im), self._stream()))
            return im
        if out is None:
            out = t.empty((_abi.HG_POLICY_IMAGE_FLOATS,), dtype=t.float32, device=self.device)
        out = self._opt_tensor(out, (_abi.HG_POLICY_IMAGE_FLOATS,), "out", who="debug_policy_image")
        self._check(self.lib.hg_debug_get_policy_image(self._h, _ptr(out), self._stream()))
        return out

    # ------------------------------------------------------------------ branched planning rollouts
    def _plan_tensor(self, x, shape, name, dtype=None):
        """`x` as the library reads it: a contiguous tensor of `shape` and `dtype` on the env's device
        (ValueError otherwise: nothing is converted, the kernels take the buffers as they are)."""
        t = self.torch
        dtype = t.float32 if dtype is None else dtype
        if (not isinstance(x, t.Tensor) or x.dtype != dtype or x.device != self.device or not x.is_contiguous()
                or tuple(x.shape) != tuple(shape)):
            got = f"{tuple(x.shape)} {x.dtype} on {x.device}" if isinstance(x, t.Tensor) else type(x).__name__
            raise ValueError(f"{name} must be a contiguous {dtype} {tuple(shape)} tensor on {self.device}, got {got}")
        return x

    @staticmethod
    def _plan_count(v, name):
        if isinstance(v, bool) or int(v) != v or int(v) < 1:
            raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
        return int(v)

    def rollout_branch(self, actions, branches, gamma=1.0, noise="env", out=None):
        """Score `branches` candidate action sequences per env without touching the env
        (hg_rollout_branch).  actions [H, N*branches, 4], row e * branches + b the branch b of env e.
        Every branch starts from its env's current state and evolves as rollout() would, up to and
        including its first terminated / truncated step, with no reset.  Returns a dict of device
        tensors: returns [N, branches] float32 (sum of gamma^t reward_t), alive_steps [N, branches]
        int32 (steps up to and including the ending one) and end_info [N, branches] uint8 (the ending
        step's info bits, 0 for a branch that survived).  noise="env": every branch meets the
        turbulence its env is about to draw (the planner sees the gusts ahead); "off": none.
        `out`: a dict returned by a previous call with the same shapes, reused."""
        t = self.torch
        B, N = self._plan_count(branches, "branches"), self.num_envs
        if not isinstance(actions, t.Tensor) or actions.ndim != 3 or actions.shape[0] < 1:
            raise ValueError(f"actions must be a [H, {N * B}, 4] tensor")
        H = int(actions.shape[0])
        a = self._plan_tensor(actions, (H, N * B, _abi.HG_N_ACT), "actions")
        if noise not in _abi.BRANCH_NOISE_MODES:
            raise ValueError(f"noise must be one of {sorted(_abi.BRANCH_NOISE_MODES)}, got {noise!r}")
        if out is None:
            out = dict(returns=t.empty((N, B), dtype=t.float32, device=self.device),
                       alive_steps=t.empty((N, B), dtype=t.int32, device=self.device),
                       end_info=t.empty((N, B), dtype=t.uint8, device=self.device))
        ret = self._plan_tensor(out["returns"], (N, B), "out['returns']")
        alive = self._plan_tensor(out["alive_steps"], (N, B), "out['alive_steps']", t.int32)
        end = self._plan_tensor(out["end_info"], (N, B), "out['end_info']", t.uint8)
        self._keep_plan = a
        self._check(self.lib.hg_rollout_branch(self._h, _ptr(a), H, B, float(gamma), _abi.BRANCH_NOISE_MODES[noise],
                                               _ptr(ret), _ptr(alive), _ptr(end), self._stream()))
        return out

    @staticmethod
    def _four(v, name):
        a = np.asarray(v, dtype=np.float32).reshape(-1)
        if a.size == 1:
            a = np.repeat(a, 4)
        if a.size != 4:
            raise ValueError(f"{name} must be a scalar or 4 values, got {np.shape(v)}")
        return (ctypes.c_float * 4)(*a.tolist())

    def mppi_sample(self, nominal, branches, sigma, lo, hi, seed, out=None):
        """Candidates around `nominal` [H, N, 4] (hg_mppi_sample): out [H, N*branches, 4] =
        clamp(nominal + sigma * z, lo, hi) with z standard normals keyed by (global env id, t, branch)
        and `seed` (vary it per control step); branch 0 is the clamped nominal itself.  sigma, lo, hi:
        a scalar or 4 values each."""
        t = self.torch
        B, N = self._plan_count(branches, "branches"), self.num_envs
        if not isinstance(nominal, t.Tensor) or nominal.ndim != 3 or nominal.shape[0] < 1:
            raise ValueError(f"nominal must be a [H, {N}, 4] tensor")
        H = int(nominal.shape[0])
        m = self._plan_tensor(nominal, (H, N, _abi.HG_N_ACT), "nominal")
        s, l, h = self._four(sigma, "sigma"), self._four(lo, "lo"), self._four(hi, "hi")
        if out is None:
            out = t.empty((H, N * B, _abi.HG_N_ACT), dtype=t.float32, device=self.device)
        o = self._plan_tensor(out, (H, N * B, _abi.HG_N_ACT), "out")
        self._keep_plan = m
        self._check(self.lib.hg_mppi_sample(self._h, _ptr(m), H, B, s, l, h, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(o),
                                            self._stream()))
        return o

    def mppi_update(self, actions, returns, lam, out=None):
        """The MPPI update (hg_mppi_update): out [H, N, 4] = the candidates `actions` [H, N*branches, 4]
        averaged per env with weights exp((G_b - G_max) / lam) of `returns` [N, branches]; a
        non-finite return weighs 0, an env without a finite one keeps branch 0."""
        t = self.torch
        N = self.num_envs
        if not isinstance(returns, t.Tensor) or returns.ndim != 2 or returns.shape[1] < 1:
            raise ValueError(f"returns must be a [{N}, branches] tensor")
        B = int(returns.shape[1])
        g = self._plan_tensor(returns, (N, B), "returns")
        if not isinstance(actions, t.Tensor) or actions.ndim != 3 or actions.shape[0] < 1:
            raise ValueError(f"actions must be a [H, {N * B}, 4] tensor")
        H = int(actions.shape[0])
        a = self._plan_tensor(actions, (H, N * B, _abi.HG_N_ACT), "actions")
        if out is None:
            out = t.empty((H, N, _abi.HG_N_ACT), dtype=t.float32, device=self.device)
        o = self._plan_tensor(out, (H, N, _abi.HG_N_ACT), "out")
        self._keep_plan = (a, g)
        self._check(self.lib.hg_mppi_update(self._h, _ptr(a), _ptr(g), H, B, float(lam), _ptr(o), self._stream()))
        return o

    def mppi_value(self, returns, branches, lam, out=None):
        """What mppi_update's weights make of the returns themselves (hg_mppi_value): for `returns`
        [N, branches] a dict of value [N], the softmax-weighted mean return; best [N], the largest finite
        return; ess [N], the weights' effective sample size (sum w)^2 / sum w^2.  A non-finite return weighs
        0; an env without a finite one gets (0, -inf, 0).  `out`: such a dict to reuse."""
        t = self.torch
        N = self.num_envs
        B = self._plan_count(branches, "branches")
        lam = float(lam)
        if not (np.isfinite(lam) and lam > 0):
            raise ValueError(f"lam must be finite and > 0, got {lam!r}")
        if not isinstance(returns, t.Tensor) or returns.ndim != 2:
            raise ValueError(f"returns must be a [{N}, {B}] tensor")
        g = self._plan_tensor(returns, (N, B), "returns")
        if out is None:
            out = {k: t.empty((N,), dtype=t.float32, device=self.device) for k in ("value", "best", "ess")}
        v = self._plan_tensor(out["value"], (N,), "out['value']")
        b = self._plan_tensor(out["best"], (N,), "out['best']")
        s = self._plan_tensor(out["ess"], (N,), "out['ess']")
        self._keep_plan = g
        self._check(self.lib.hg_mppi_value(self._h, _ptr(g), B, lam, _ptr(v), _ptr(b), _ptr(s), self._stream()))
        return out

    # ------------------------------------------------------------------ policy-guided planning
    def _act_bounds(self, lo, hi):
        if (lo is None) != (hi is None):
            raise ValueError("lo and hi go together: both given (a scalar or 4 values each) or both None")
        if lo is None:
            return None, None
        return self._four(lo, "lo"), self._four(hi, "hi")

    def policy_act_mean(self, obs=None, residual=None, lo=None, hi=None, out=None, value=False):
        """The policy's MEAN action plus a residual, clamped (hg_policy_act_mean): out [N,4] =
        clamp(mu(obs) + residual, lo, hi) for `obs` [N,17] (default: `self.obs`).  Nothing is drawn, even for
        a stochastic policy; the env is not modified.  residual [N,4] or None; lo / hi: a scalar or 4 values
        each, or both None for no clamp.  value=True returns (actions, V(obs) [N]) and needs a value head.
        policy_act_mean then step(), repeated, is bitwise a branch of rollout_branch_policy()."""
        t = self.torch
        o = self._obs_arg(obs, "obs")
        r = None if residual is None else self._plan_tensor(residual, (self.num_envs, _abi.HG_N_ACT), "residual")
        l, h = self._act_bounds(lo, hi)
        if out is None:
            out = t.empty((self.num_envs, _abi.HG_N_ACT), dtype=t.float32, device=self.device)
        a = self._plan_tensor(out, (self.num_envs, _abi.HG_N_ACT), "out")
        v = t.empty((self.num_envs,), dtype=t.float32, device=self.device) if value else None
        self._keep_plan = (o, r)
        self._check(self.lib.hg_policy_act_mean(self._h, _ptr(o), _ptr(r), l, h, _ptr(a), _ptr(v), self._stream()))
        return (a, v) if value else a

    def rollout_branch_policy(self, residuals, branches, obs0=None, gamma=1.0, noise="env", lo=None, hi=None,
                              bootstrap=False, value_scale=1.0, out=None, horizon=None):
        """rollout_branch() with the env's policy inside the branches (hg_rollout_branch_policy): branch b of
        env e starts from the env's state and `obs0[e]` (default: `self.obs`) and takes
        a_t = clamp(mu(o_t) + residuals[t, e * branches + b], lo, hi), o_t its own latest observation.
        residuals [H, N*branches, 4], or None with horizon=H (no residual: pure policy evaluation).  bootstrap=True:
        a branch that survives the horizon, or is truncated without terminating, adds
        gamma^T * value_scale * V(its last observation) (needs a value head); value_scale = 1 / reward_scale
        turns a critic trained on scaled rewards into raw reward units.  Returns rollout_branch's dict."""
        t = self.torch
        B, N = self._plan_count(branches, "branches"), self.num_envs
        if residuals is None:
            if horizon is None:
                raise ValueError("residuals=None needs horizon=H")
            H, r = self._plan_count(horizon, "horizon"), None
        else:
            if not isinstance(residuals, t.Tensor) or residuals.ndim != 3 or residuals.shape[0] < 1:
                raise ValueError(f"residuals must be a [H, {N * B}, 4] tensor (or None with horizon=H)")
            H = int(residuals.shape[0])
            if horizon is not None and int(horizon) != H:
                raise ValueError(f"horizon {horizon!r} does not match residuals' {H} steps")
            r = self._plan_tensor(residuals, (H, N * B, _abi.HG_N_ACT), "residuals")
        o0 = self._obs_arg(obs0, "obs0")
        if noise not in _abi.BRANCH_NOISE_MODES:
            raise ValueError(f"noise must be one of {sorted(_abi.BRANCH_NOISE_MODES)}, got {noise!r}")
        l, h = self._act_bounds(lo, hi)
        value_scale = float(value_scale)
        if not np.isfinite(value_scale):
            raise ValueError(f"value_scale must be finite, got {value_scale!r}")
        if out is None:
            out = dict(returns=t.empty((N, B), dtype=t.float32, device=self.device),
                       alive_steps=t.empty((N, B), dtype=t.int32, device=self.device),
                       end_info=t.empty((N, B), dtype=t.uint8, device=self.device))
        ret = self._plan_tensor(out["returns"], (N, B), "out['returns']")
        alive = self._plan_tensor(out["alive_steps"], (N, B), "out['alive_steps']", t.int32)
        end = self._plan_tensor(out["end_info"], (N, B), "out['end_info']", t.uint8)
        self._keep_plan = (o0, r)
        self._check(self.lib.hg_rollout_branch_policy(
            self._h, _ptr(o0), _ptr(r), H, B, float(gamma), _abi.BRANCH_NOISE_MODES[noise], l, h,
            _abi.HG_BOOTSTRAP_VALUE if bootstrap else _abi.HG_BOOTSTRAP_NONE, value_scale, _ptr(ret), _ptr(alive),
            _ptr(end), self._stream()))
        return out

    def trim_batch(self, wind_ned):
        """Device batched trim (hg_trim_batch) of this env's trim condition against each row of
        `wind_ned` [K,3] (ft/s NED): the reset the reference computes from its second episode on.
        Returns dict of float32 device tensors state [K,18], action [K,4], obs [K,17] and int32
        status [K] (0 or HG_E_TRIM)."""
        t = self.torch
        w = t.as_tensor(wind_ned, device=self.device, dtype=t.float32).contiguous()
        if w.ndim != 2 or w.shape[1] != 3:
            raise ValueError("wind_ned must be [K, 3]")
        K = w.shape[0]
        out = {"state": t.empty((K, _abi.HG_N_HELI), dtype=t.float32, device=self.device),
               "action": t.empty((K, _abi.HG_N_ACT), dtype=t.float32, device=self.device),
               "obs": t.empty((K, _abi.HG_N_OBS), dtype=t.float32, device=self.device),
               "status": t.full((K,), -99, dtype=t.int32, device=self.device)}
        self._check(self.lib.hg_trim_batch(self._h, _ptr(w), K, _ptr(out["state"]), _ptr(out["action"]),
                                           _ptr(out["obs"]), _ptr(out["status"]), self._stream()))
        self._keep_trim = w
        return out

    def trim_conds(self, conds, wind_ned=None):
        """Device trims (hg_trim_conds_batch) for a list of trim-condition dicts (the reference's
        set_trim_cond keys, missing keys from the defaults), against `wind_ned` [K,3] or the mean
        wind.  Returns dict of device tensors state [K,18], action [K,4], obs [K,17], status [K]."""
        t = self.torch
        K = len(conds)
        arr = (_abi.hg_trim_cond * K)()
        for j, c in enumerate(conds):
            config.fill_trim(arr[j], c)
        w = None
        if wind_ned is not None:
            w = t.as_tensor(wind_ned, device=self.device, dtype=t.float32).contiguous()
            if tuple(w.shape) != (K, 3):
                raise ValueError("wind_ned must be [K, 3]")
        out = {"state": t.empty((K, _abi.HG_N_HELI), dtype=t.float32, device=self.device),
               "action": t.empty((K, _abi.HG_N_ACT), dtype=t.float32, device=self.device),
               "obs": t.empty((K, _abi.HG_N_OBS), dtype=t.float32, device=self.device),
               "status": t.full((K,), -99, dtype=t.int32, device=self.device)}
        self._check(self.lib.hg_trim_conds_batch(self._h, arr, K, _ptr(w), _ptr(out["state"]), _ptr(out["action"]),
                                                 _ptr(out["obs"]), _ptr(out["status"]), self._stream()))
        return out

    def set_trim_conds(self, conds):
        """Batched set_trim_cond (helicopter.py:101-103): env i resets to the trim of conds[i] (a
        list of N dicts).  Trims all on the device; raises if any trim fails.  `None` reverts to
        the shared condition (set_trim_cond)."""
        if conds is None:
            self._check(self.lib.hg_set_reset_templates(self._h, None, self._stream()))
            return None
        if len(conds) != self.num_envs:
            raise ValueError(f"need {self.num_envs} trim conditions, got {len(conds)}")
        r = self.trim_conds(conds)
        bad = (r["status"] != 0).nonzero().flatten()
        if len(bad):
            raise _abi.HeliGymError(f"trim failed for envs {bad[:10].tolist()}")
        obs = r["obs"]
        tmpl = self.torch.cat([r["state"], obs[:, 4:7], obs[:, 16:17], obs], dim=1).contiguous()
        self._check(self.lib.hg_set_reset_templates(self._h, _ptr(tmpl), self._stream()))
        return r

    def set_weather(self, turb_level=None, wind_dir=None, wind_spd=None, conds=None):
        """Per-env weather (hg_set_weather): turbulence level (0 .. 7, may be fractional), mean wind direction
        (degrees) and speed (ft/s), each a scalar or an [N] array; a missing key takes the airframe document's
        ENV value.  Every env is trimmed on the device against its own mean wind -- for `conds`, a list of N
        trim-condition dicts, or the env's shared condition -- and resets to that trim from now on.  Returns
        the trims as set_trim_conds does (state, obs, status; device tensors), `templates` included.  With no
        argument: back to the handle-wide weather and the shared template (returns None).  Raises
        HeliGymError naming the first envs whose trim failed; the env is then as it was.
        reset_mode="template" only.  Synchronises; call it outside graph capture, step inside as before."""
        t, N = self.torch, self.num_envs
        if turb_level is None and wind_dir is None and wind_spd is None and conds is None:
            self._check(self.lib.hg_set_weather(self._h, None, None, None, self._stream()))
            return None
        af = self.cfg.af
        cols = []
        for v, own, name in ((turb_level, af.env_TURB_LVL, "turb_level"), (wind_dir, af.env_WIND_DIR_deg, "wind_dir"),
                             (wind_spd, af.env_WIND_SPD, "wind_spd")):
            a = np.asarray(own if v is None else (v.detach().cpu().numpy() if hasattr(v, "detach") else v), dtype=np.float32)
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != N):
                raise ValueError(f"set_weather: {name} must be a scalar or have {N} entries, got shape {a.shape}")
            cols.append(np.broadcast_to(a, (N,)))
        arr = (_abi.hg_weather * N)()
        np.frombuffer(arr, dtype=np.float32).reshape(N, 3)[:] = np.stack(cols, axis=1)
        carr = None
        if conds is not None:
            if len(conds) != N:
                raise ValueError(f"need {N} trim conditions, got {len(conds)}")
            carr = (_abi.hg_trim_cond * N)()
            for j, c in enumerate(conds):
                config.fill_trim(carr[j], c)
        status = t.full((N,), -99, dtype=t.int32, device=self.device)
        rc = self.lib.hg_set_weather(self._h, arr, carr, _ptr(status), self._stream())
        if rc == -3:   # HG_E_TRIM: name the envs
            bad = (status != 0).nonzero().flatten()
            raise _abi.HeliGymError(f"heligym_amd error {rc}: trim failed for envs {bad[:10].tolist()} "
                                    f"({len(bad)} of {N}); the weather was not set")
        self._check(rc)
        tm = self.get_weather()["templates"]
        return {"state": tm[:, :_abi.HG_N_HELI], "obs": tm[:, 22:], "status": status, "templates": tm}

    def get_weather(self):
        """dict of [N] float32 arrays turb_level, wind_dir, wind_spd (the airframe's values while no per-env
        weather is set) and `templates`, the [N,39] device tensor of reset templates in use (state 18 | carry 4
        | observation 17)."""
        t, N = self.torch, self.num_envs
        arr = (_abi.hg_weather * N)()
        tm = t.empty((N, 39), dtype=t.float32, device=self.device)
        self._check(self.lib.hg_get_weather(self._h, arr, _ptr(tm), self._stream()))
        w = np.frombuffer(arr, dtype=np.float32).reshape(N, 3).copy()
        return {"turb_level": w[:, 0], "wind_dir": w[:, 1], "wind_spd": w[:, 2], "templates": tm}

    def set_goals(self, goals=None, box=None, relative=False):
        """Per-env goals (hg_set_goals).  `goals`: a dict over the task's fields (hover: north_loc, east_loc,
        sea_alt; forward_flight: sea_alt, vel), each a scalar or an [N] array; a missing key takes the env's
        target.  `box`: {field: (lo, hi)} -- every env's goal is redrawn inside it at each reset, in the kernel
        that resets it, a function of (seed, global env id, episode) that goal_ref restates.  `relative`: the
        observation rows carry position (or altitude and speed) minus the goal.  With no argument: back to the
        env's one target.  reset_mode="template" only, not together with set_weather or set_fleet.
        Synchronises; call it outside graph capture, step inside as before."""
        N = self.num_envs
        if goals is None and box is None:
            if relative:
                raise ValueError("set_goals: relative observations need goals or a box")
            self._check(self.lib.hg_set_goals(self._h, None, None, 0, self._stream()))
            return
        if goals is not None and box is not None:
            raise ValueError("set_goals: give goals or a box, not both")
        fields = _goals.GOAL_FIELDS.get(self.task)
        if fields is None:
            raise ValueError(f"set_goals: task {self.task!r} has no target")
        mode = _abi.HG_GOAL_OBS_RELATIVE if relative else _abi.HG_GOAL_OBS_ABSOLUTE
        own = dict.fromkeys(config.TARGET_KEYS, 0.0)
        own.update(self._target)
        if box is not None:
            lo, hi = _goals.box_arrays(box, self.task, own)   # (validates keys and ranges)
            b = _abi.hg_goal_box()
            config.fill_target(b.lo, own)
            config.fill_target(b.hi, own)
            for name in fields:
                r = box.get(name, own[name])
                a, c = (r, r) if np.isscalar(r) else r
                setattr(b.lo, name, float(a))
                setattr(b.hi, name, float(c))
            self._check(self.lib.hg_set_goals(self._h, None, ctypes.byref(b), mode, self._stream()))
            return
        if not isinstance(goals, dict):
            raise ValueError(f"set_goals: goals must be a dict over {fields}")
        unknown = sorted(set(goals) - set(fields))
        if unknown:
            raise ValueError(f"set_goals: unknown field(s) {unknown} for task {self.task!r}; its fields are {fields}")
        arr = (_abi.hg_target * N)()
        rows = np.frombuffer(arr, dtype=np.float64).reshape(N, len(config.TARGET_KEYS))
        for j, name in enumerate(config.TARGET_KEYS):
            v = goals.get(name, own[name]) if name in fields else own[name]
            a = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64)
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != N):
                raise ValueError(f"set_goals: {name} must be a scalar or have {N} entries, got shape {a.shape}")
            if name in fields and not np.all(np.isfinite(a)):
                raise ValueError(f"set_goals: {name} has a non-finite value")
            rows[:, j] = a
        self._check(self.lib.hg_set_goals(self._h, arr, None, mode, self._stream()))

    def get_goals(self):
        """dict of [N] float64 arrays over the task's fields (the env's one target while no goals are set; in box
        mode the float32 values the device table holds now), plus `mode` ("off", "table" or "box"), `box`
        ({field: (lo, hi)} or None) and `relative`."""
        N = self.num_envs
        arr = (_abi.hg_target * N)()
        b = _abi.hg_goal_box()
        mode, om = ctypes.c_int32(), ctypes.c_int32()
        self._check(self.lib.hg_get_goals(self._h, arr, ctypes.byref(b), ctypes.byref(mode), ctypes.byref(om), self._stream()))
        rows = np.frombuffer(arr, dtype=np.float64).reshape(N, len(config.TARGET_KEYS))
        fields = _goals.GOAL_FIELDS.get(self.task, ())
        out = {name: rows[:, config.TARGET_KEYS.index(name)].copy() for name in fields}
        out["mode"] = ("off", "table", "box")[mode.value]
        out["box"] = ({name: (getattr(b.lo, name), getattr(b.hi, name)) for name in fields}
                      if mode.value == _abi.HG_GOALS_BOX else None)
        out["relative"] = om.value == _abi.HG_GOAL_OBS_RELATIVE
        return out

    def set_fleet(self, airframes, tile_class=None, envs_per_class=None, conds=None):
        """Mixed fleet (hg_set_fleet): one airframe class per 64-env state tile.  `airframes` is a list of
        airframe documents or names (anything config.load_airframe takes, sample_fleet's output included);
        give either `tile_class`, the class of each of the ceil(N/64) tiles, or `envs_per_class`, a multiple of
        64: consecutive blocks of that many envs take classes 0, 1, ... (every class must get a tile).  Each
        class is trimmed on the host against its own mean wind -- for conds[c], a trim-condition dict per
        class, or the env's shared condition -- and its envs reset to that trim from now on.  Returns the
        per-class trim status (int32 array).  `set_fleet(None)`: back to the env's own airframe and the shared
        template (returns None).  Raises HeliGymError naming the classes whose trim failed (its `status`
        attribute holds them all); the env is then as it was.  reset_mode="template" only, not together with
        set_weather.  Synchronises; call it outside graph capture, step inside as before."""
        if airframes is None:
            self._check(self.lib.hg_set_fleet(self._h, None, None, 0, None, None, self._stream()))
            return None
        classes, tiles = fleet_arrays(airframes, self.num_envs, tile_class, envs_per_class)
        C = len(classes)
        carr = None
        if conds is not None:
            if len(conds) != C:
                raise ValueError(f"set_fleet: need {C} trim conditions (one per class), got {len(conds)}")
            carr = (_abi.hg_trim_cond * C)()
            for j, c in enumerate(conds):
                config.fill_trim(carr[j], c)
        status = np.full(C, -99, dtype=np.int32)
        rc = self.lib.hg_set_fleet(self._h, classes, carr, C, tiles.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                   status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), self._stream())
        if rc == -3:   # HG_E_TRIM: name the classes
            bad = np.nonzero(status != 0)[0]
            msg = self.lib.hg_last_error()
            err = _abi.HeliGymError(f"heligym_amd error {rc}: trim failed for classes {bad[:10].tolist()} ({len(bad)} of "
                                    f"{C}); the fleet was not set ({msg.decode() if msg else ''})")
            err.status = status
            raise err
        self._check(rc)
        return status

    def get_fleet(self):
        """dict of `airframes` (a list of {field: value} dicts, one per class; the env's own airframe while no
        fleet is set), `tile_class` (int32 [ceil(N/64)]) and `templates`, the [N,39] device tensor of reset
        templates in use."""
        t, N = self.torch, self.num_envs
        tiles = (N + 63) // 64
        n = ctypes.c_int32()
        self._check(self.lib.hg_get_fleet(self._h, ctypes.byref(n), None, None, None))
        tc = np.zeros(tiles, dtype=np.int32)
        arr = (_abi.hg_airframe * n.value)()
        tm = t.empty((N, 39), dtype=t.float32, device=self.device)
        self._check(self.lib.hg_get_fleet(self._h, None, tc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), arr, _ptr(tm)))
        names = [f for f, _ in _abi.hg_airframe._fields_ if f != "_pad0"]
        return {"airframes": [{f: getattr(a, f) for f in names} for a in arr], "tile_class": tc, "templates": tm}

    def retrim_failures(self):
        """Auto-resets in reset_mode="retrim" whose trim did not converge (they got the template)."""
        c = ctypes.c_int64()
        self._check(self.lib.hg_retrim_failures(self._h, ctypes.byref(c)))
        return c.value

    LAUNCH_KINDS = ("steps", "overlapped_retrim", "specialized", "helper", "lone_wave", "bulk")

    def debug_launches(self):
        """Diagnostic: host-side launch counts of this env (hg_debug_launches): step calls, steps that
        held the previous step's re-trims, and the kernel kinds that ran."""
        out = (ctypes.c_int64 * 6)()
        self._check(self.lib.hg_debug_launches(self._h, out))
        return dict(zip(self.LAUNCH_KINDS, (int(v) for v in out)))

    def retrim_solve_stats(self):
        """Diagnostic: (solves tried with the host trim's pivot order, of them re-solved with the pivot
        search after failing the residual test) over the device trims of this env (hg_debug_retrim_solves)."""
        c = (ctypes.c_int64 * 2)()
        self._check(self.lib.hg_debug_retrim_solves(self._h, c))
        return int(c[0]), int(c[1])

    def retrim_invalid_jobs(self):
        """Diagnostic: re-trim job records that named no env (skipped); 0 in a correct run."""
        c = ctypes.c_int64()
        self._check(self.lib.hg_debug_retrim_invalid(self._h, ctypes.byref(c)))
        return c.value

    def debug_eta(self, out=None):
        """Diagnostic: the turbulence noise [N,3] (scaled by 1/sqrt(dt), wind_dynamics.py:49-52) each
        env's next step draws in-kernel, from its current counters (hg_debug_eta).  Injecting it as
        `eta` gives bitwise the in-kernel step."""
        t = self.torch
        if out is None:
            out = t.empty((self.num_envs, 3), dtype=t.float32, device=self.device)
        elif (tuple(out.shape) != (self.num_envs, 3) or out.dtype != t.float32 or out.device != t.device(self.device)
              or not out.is_contiguous()):
            # the kernel writes 3 * num_envs floats: never hand it a buffer that does not hold them
            raise ValueError(f"debug_eta: out must be a contiguous float32 ({self.num_envs}, 3) tensor on "
                             f"{self.device}, got {tuple(out.shape)} {out.dtype} on {out.device}")
        self._check(self.lib.hg_debug_eta(self._h, _ptr(out), self._stream()))
        return out

    def debug_task(self, heli, dots, out=None):
        """Diagnostic: the task layer alone (hg_debug_task) on rows of post-step heli state [n,18] and k4
        derivatives [n,18], float32 on the env's device: (reward [n] float32, success_step [n] uint8) under the
        env's target, or, while per-env goals are set, row i under the goal of env i % num_envs."""
        t = self.torch
        n = int(heli.shape[0])
        for name, x in (("heli", heli), ("dots", dots)):
            if (tuple(x.shape) != (n, 18) or x.dtype != t.float32 or x.device != t.device(self.device)
                    or not x.is_contiguous()):
                raise ValueError(f"debug_task: {name} must be a contiguous float32 ({n}, 18) tensor on {self.device}")
        if out is None:
            out = (t.empty((n,), dtype=t.float32, device=self.device), t.empty((n,), dtype=t.uint8, device=self.device))
        rew, succ = out
        if (tuple(rew.shape) != (n,) or rew.dtype != t.float32 or tuple(succ.shape) != (n,) or succ.dtype != t.uint8
                or rew.device != t.device(self.device) or succ.device != t.device(self.device)
                or not rew.is_contiguous() or not succ.is_contiguous()):
            raise ValueError(f"debug_task: out must be (float32 ({n},), uint8 ({n},)) contiguous tensors on {self.device}")
        self._check(self.lib.hg_debug_task(self._h, _ptr(heli), _ptr(dots), _ptr(rew), _ptr(succ), n, self._stream()))
        return out

    def debug_failed(self, heli, dots):
        """Diagnostic: the failure test alone (hg_debug_failed) on rows of post-step heli state [n,18] and k4
        derivatives [n,18], float32 on the env's device: (failed [n] uint8, clauses [n] uint8 of HG_FAIL_* bits)
        with the env's constants and terrain, or, under a fleet, row i with the class of env i % num_envs."""
        t = self.torch
        n = int(heli.shape[0])
        for name, x in (("heli", heli), ("dots", dots)):
            if (tuple(x.shape) != (n, 18) or x.dtype != t.float32 or x.device != t.device(self.device)
                    or not x.is_contiguous()):
                raise ValueError(f"debug_failed: {name} must be a contiguous float32 ({n}, 18) tensor on {self.device}")
        failed = t.empty((n,), dtype=t.uint8, device=self.device)
        clauses = t.empty((n,), dtype=t.uint8, device=self.device)
        self._check(self.lib.hg_debug_failed(self._h, _ptr(heli), _ptr(dots), _ptr(failed), _ptr(clauses), n, self._stream()))
        return failed, clauses

    def random_actions(self, out, seed, step, lo=-1.0, hi=1.0):
        self._check(self.lib.hg_random_actions(self._h, _ptr(out), int(seed), int(step), float(lo),
                                               float(hi), self._stream()))
        return out


def task_reward_host(cfg, heli, dots, goals=None):
    """Diagnostic, no device: the task layer in fp64 on the host (hg_debug_task_host) for rows of post-step heli
    state [n,18] and k4 derivatives [n,18] under `cfg` (config.make_config): (reward [n] float64, success_step [n]
    bool).  goals: None (cfg's own target), or a dict over target fields (scalars or [n] arrays, a missing field
    is cfg's) -- row i then goes through the per-env goal forms with the fp32 record of its goal."""
    lib = _abi.load_library()
    h = np.ascontiguousarray(heli, dtype=np.float64)
    d = np.ascontiguousarray(dots, dtype=np.float64)
    if h.ndim != 2 or h.shape[1] != 18 or d.shape != h.shape:
        raise ValueError("task_reward_host: heli and dots must be [n, 18]")
    n = h.shape[0]
    arr = None
    if goals is not None:
        arr = (_abi.hg_target * max(n, 1))()
        rows = np.frombuffer(arr, dtype=np.float64).reshape(max(n, 1), len(config.TARGET_KEYS))
        for j, name in enumerate(config.TARGET_KEYS):
            rows[:, j] = np.asarray(goals.get(name, getattr(cfg.target, name)), dtype=np.float64)
    rew = np.empty(n, dtype=np.float64)
    succ = np.empty(n, dtype=np.uint8)
    _abi.check(lib.hg_debug_task_host(ctypes.byref(cfg), h.ctypes.data, d.ctypes.data, arr, n, rew.ctypes.data,
                                      succ.ctypes.data), lib)
    return rew, succ.astype(bool)


def is_failed_host(cfg, terrain, heli, dots):
    """Diagnostic, no device: Heli._is_failed in fp64 on the host (hg_debug_failed_host) for rows of post-step heli
    state [n,18] and k4 derivatives [n,18] under `cfg` over `terrain` [rows, cols] ft: (failed [n] bool, clauses [n]
    uint8 of HG_FAIL_* bits)."""
    lib = _abi.load_library()
    h = np.ascontiguousarray(heli, dtype=np.float64)
    d = np.ascontiguousarray(dots, dtype=np.float64)
    if h.ndim != 2 or h.shape[1] != 18 or d.shape != h.shape:
        raise ValueError("is_failed_host: heli and dots must be [n, 18]")
    ter = np.ascontiguousarray(terrain, dtype=np.float64)
    n = h.shape[0]
    failed = np.empty(n, dtype=np.uint8)
    clauses = np.empty(n, dtype=np.uint8)
    _abi.check(lib.hg_debug_failed_host(ctypes.byref(cfg), ter.ctypes.data, ter.shape[0], ter.shape[1], h.ctypes.data,
                                        d.ctypes.data, n, failed.ctypes.data, clauses.ctypes.data), lib)
    return failed.astype(bool), clauses


def _airframe_fields(af):
    """The flat {field: value} airframe of a document, a name, or such a dict itself."""
    if isinstance(af, dict) and "airframe" not in af and "ENV" not in af:
        return af
    return config.load_airframe(af)["airframe"]


def fleet_arrays(airframes, num_envs, tile_class=None, envs_per_class=None):
    """set_fleet's inputs checked and packed, before any library call: the (hg_airframe * C) array of the
    classes and the int32 [ceil(num_envs / 64)] class of each tile."""
    N = int(num_envs)
    tiles = (N + 63) // 64
    if isinstance(airframes, (str, dict)) or not hasattr(airframes, "__len__"):
        raise ValueError("set_fleet: airframes must be a list of airframe documents or names")
    C = len(airframes)
    if C < 1 or C > tiles:
        raise ValueError(f"set_fleet: need between 1 and {tiles} classes (one per 64-env tile at most), got {C}")
    if (tile_class is None) == (envs_per_class is None):
        raise ValueError("set_fleet: give exactly one of tile_class and envs_per_class")
    if envs_per_class is not None:
        e = int(envs_per_class)
        if e != envs_per_class or e < 64 or e % 64 != 0:
            raise ValueError(f"set_fleet: envs_per_class must be a positive multiple of 64, got {envs_per_class!r}")
        tc = np.arange(tiles, dtype=np.int64) // (e // 64)
        if tc[-1] != C - 1:
            raise ValueError(f"set_fleet: {N} envs in blocks of {e} make {int(tc[-1]) + 1} classes, got {C} airframes")
    else:
        tc = np.asarray(tile_class.detach().cpu().numpy() if hasattr(tile_class, "detach") else tile_class)
        if tc.ndim != 1 or tc.shape[0] != tiles:
            raise ValueError(f"set_fleet: tile_class must have {tiles} entries (one per 64-env tile), got shape {tc.shape}")
        if tc.dtype.kind not in "iu":
            raise ValueError(f"set_fleet: tile_class must be an integer array, got {tc.dtype}")
        if tc.min() < 0 or tc.max() >= C:
            raise ValueError(f"set_fleet: tile_class entries must be in [0, {C}), got [{tc.min()}, {tc.max()}]")
    arr = (_abi.hg_airframe * C)()
    for j, doc in enumerate(airframes):
        af = _airframe_fields(doc)
        for name, _ in _abi.hg_airframe._fields_:
            if name == "_pad0":
                continue
            v = af[name]
            if name == "env_TURB_LVL":
                arr[j].env_TURB_LVL = int(v)
                continue
            v = float(v)
            if not np.isfinite(v):
                raise ValueError(f"set_fleet: class {j}: {name} is not finite ({v})")
            setattr(arr[j], name, v)
    return arr, np.ascontiguousarray(tc, dtype=np.int32)


FLEET_SPREAD = {"WT": 0.15, "IX": 0.15, "IY": 0.15, "IZ": 0.15, "FS_CG": 0.01, "mr_RPM": 0.03, "tr_RPM": 0.03}


def sample_fleet(n_classes, base="aw109", spread=None, seed=0):
    """n_classes airframe documents around `base` (a name or a document) for HeliVecEnv.set_fleet: each field
    in `spread` ({field: s}, default FLEET_SPREAD: weight, inertias, CG station, both rotor speeds) is scaled
    by a uniform factor in [1 - s, 1 + s], a function of `seed` alone (NumPy's default_rng).  Class 0 is `base`
    itself."""
    import copy
    n = int(n_classes)
    if n < 1:
        raise ValueError(f"sample_fleet: n_classes must be >= 1, got {n_classes!r}")
    spread = dict(FLEET_SPREAD if spread is None else spread)
    doc0 = config.load_airframe(base)
    for k, s in spread.items():
        if k not in doc0["airframe"] or k.startswith("env_"):
            raise ValueError(f"sample_fleet: {k!r} is not an airframe field that can be spread")
        if not (np.isfinite(s) and 0.0 <= s < 1.0):
            raise ValueError(f"sample_fleet: spread[{k!r}] must be in [0, 1), got {s!r}")
    rng = np.random.default_rng(seed)
    f = rng.random((n, len(spread)))   # drawn for every class, so class c does not depend on n_classes
    docs = []
    for c in range(n):
        doc = copy.deepcopy(doc0)
        if c > 0:
            for j, (k, s) in enumerate(spread.items()):
                doc["airframe"][k] = float(doc0["airframe"][k]) * (1.0 + float(s) * (2.0 * f[c, j] - 1.0))
        docs.append(doc)
    return docs


def sample_weather(n, turb_level=(0.0, 7.0), wind_spd=(0.0, 40.0), wind_dir=(0.0, 360.0), seed=0):
    """Uniform draws of n weathers for HeliVecEnv.set_weather(**sample_weather(n, ...)): a dict of [n] float32
    arrays turb_level, wind_spd, wind_dir, each inside its closed (lo, hi) range, a function of `seed` alone
    (NumPy's PCG64).  A range may also be one number (every env the same)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, r in (("turb_level", turb_level), ("wind_spd", wind_spd), ("wind_dir", wind_dir)):
        lo, hi = (r, r) if np.isscalar(r) else r
        lo, hi = float(lo), float(hi)
        if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
            raise ValueError(f"sample_weather: {name} range must be finite with lo <= hi, got {r}")
        v = (lo + (hi - lo) * rng.random(int(n))).astype(np.float32)
        # (the fp32 rounding may step over an end that is not an fp32 number)
        v = np.where(v > hi, np.nextafter(v, np.float32(-np.inf)), v)
        out[name] = np.where(v < lo, np.nextafter(v, np.float32(np.inf)), v).astype(np.float32)
    return out
