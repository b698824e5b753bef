"""Sampling-based planning on the device: an MPPI controller over HeliVecEnv's branched rollouts.

Every control step the planner perturbs a nominal action sequence per env (hg_mppi_sample), scores all
candidates from the env's current state in one launch that does not touch the env (hg_rollout_branch),
and averages them with softmax weights of their returns (hg_mppi_update).  All buffers are allocated
once; a plan() is three kernel launches per iteration and no host synchronisation.

PolicyMPPI is the same loop around the env's own policy: the sequence it optimises is a *residual* on the
policy's mean action, every candidate is rolled out closed-loop with the policy inside the branch
(hg_rollout_branch_policy), and the value head scores what lies past the horizon.
"""
import numpy as np


class MPPI:
    """Model-predictive path integral control of the N envs of `env` (a HeliVecEnv).

    horizon: steps each candidate is rolled out; branches: candidates per env (branch 0 is always the
    unperturbed nominal); sigma: the perturbation's standard deviation, lam: the softmax temperature
    (in return units), lo / hi: the action bounds the candidates are clamped to -- each a scalar or 4
    values.  gamma: the discount of the candidates' returns.  noise: "env" -- every candidate meets the
    turbulence its env is about to draw, so the planner sees the gusts ahead -- or "off", a
    certainty-equivalent planner.  seed: the perturbations' key; each sampling advances it by one.

    The nominal starts at the env's trim action.  A control loop is
        a = mppi.plan(); env.step(a); mppi.shift()
    with mppi.reset(mask) for the envs whose episode ended.
    """

    def __init__(self, env, horizon, branches, sigma, lam, lo=-1.0, hi=1.0, gamma=1.0, noise="env", seed=0):
        self.env = env
        t = self.torch = env.torch
        self.horizon, self.branches = int(horizon), int(branches)
        if self.horizon < 1 or self.branches < 1:
            raise ValueError("horizon and branches must be >= 1")
        self.sigma, self.lam, self.lo, self.hi = sigma, float(lam), lo, hi
        self.gamma, self.noise, self.seed = float(gamma), noise, int(seed)
        N, H, B = env.num_envs, self.horizon, self.branches
        self.trim_action = self._rest()
        self.nominal = self.trim_action.expand(H, N, 4).contiguous()
        self._next = t.empty_like(self.nominal)
        self.actions = t.empty((H, N * B, 4), dtype=t.float32, device=env.device)
        self.scores = None
        self.samplings = 0

    def _rest(self):
        """The [4] row the nominal starts from and reset() returns it to: the env's trim action."""
        t, env = self.torch, self.env
        return t.as_tensor(np.asarray(env.template()["action"], dtype=np.float32), device=env.device)

    def _score(self):
        """Score the candidates in self.actions into self.scores."""
        self.scores = self.env.rollout_branch(self.actions, self.branches, gamma=self.gamma, noise=self.noise,
                                              out=self.scores)

    def _iterate(self, iterations):
        env = self.env
        for _ in range(int(iterations)):
            env.mppi_sample(self.nominal, self.branches, self.sigma, self.lo, self.hi, self.seed + self.samplings,
                            out=self.actions)
            self.samplings += 1
            self._score()
            env.mppi_update(self.actions, self.scores["returns"], self.lam, out=self._next)
            self.nominal, self._next = self._next, self.nominal

    def plan(self, iterations=1):
        """`iterations` rounds of sample -> rollout_branch -> update on the current stream.  Returns the
        nominal's first action [N, 4] (a view: step the env with it before the next plan / shift)."""
        self._iterate(iterations)
        return self.nominal[0]

    def value(self, out=None):
        """What the planner thinks each env's state is worth (hg_mppi_value of the last scored candidate set,
        with the planner's own temperature): a dict of value [N] (the softmax-weighted mean return: with
        PolicyMPPI's bootstrap the n-step lookahead value, a critic's regression target), best [N] (the largest
        finite return) and ess [N] (the weights' effective sample size).  `out`: such a dict to reuse."""
        if self.scores is None:
            raise ValueError("value() needs a scored candidate set: call plan() first")
        return self.env.mppi_value(self.scores["returns"], self.branches, self.lam, out=out)

    def shift(self):
        """Advance the nominal by one step: row t takes row t + 1, the last row is repeated."""
        if self.horizon > 1:
            self._next[:-1].copy_(self.nominal[1:])
            self._next[-1].copy_(self.nominal[-1])
            self.nominal, self._next = self._next, self.nominal

    def reset(self, mask=None):
        """The nominal of the envs where `mask` != 0 (all envs if None) back to the trim action."""
        if mask is None:
            self.nominal.copy_(self.trim_action.expand_as(self.nominal))
            return
        t = self.torch
        m = t.as_tensor(mask, device=self.nominal.device).reshape(-1) != 0
        if m.shape[0] != self.nominal.shape[1]:
            raise ValueError(f"mask must have {self.nominal.shape[1]} entries, got {m.shape[0]}")
        self.nominal.copy_(t.where(m[None, :, None], self.trim_action.expand_as(self.nominal), self.nominal))


class PolicyMPPI(MPPI):
    """MPPI around the env's policy (set_policy; set_value_head for the bootstrap): the nominal is a residual
    sequence on the policy's mean action -- zeros at the start and after reset(mask) -- and a candidate is
    rolled out closed-loop, a_t = clamp(mu(o_t) + residual_t, lo, hi), by rollout_branch_policy.

    sigma, lam, gamma, noise, seed: as MPPI's.  res_lo / res_hi: the bounds the *residual* candidates are
    clamped to by the sampling; lo / hi: the bounds of the *applied* action (both None: none).
    bootstrap: candidates the horizon or a truncation cuts add gamma^T * value_scale * V(last observation);
    value_scale = 1 / reward_scale for a critic trained on scaled rewards.

    A control loop is
        a = planner.plan(obs); obs, *_ = env.step(a); planner.shift()
    """

    def __init__(self, env, horizon, branches, sigma, lam, res_lo=-1.0, res_hi=1.0, lo=None, hi=None, gamma=1.0,
                 noise="env", seed=0, bootstrap=True, value_scale=1.0):
        super().__init__(env, horizon, branches, sigma, lam, lo=res_lo, hi=res_hi, gamma=gamma, noise=noise, seed=seed)
        self.act_lo, self.act_hi = lo, hi
        self.bootstrap, self.value_scale = bool(bootstrap), float(value_scale)
        self.action = self.torch.empty((env.num_envs, 4), dtype=self.torch.float32, device=env.device)
        self._obs = None

    def _rest(self):
        return self.torch.zeros(4, dtype=self.torch.float32, device=self.env.device)

    def _score(self):
        self.scores = self.env.rollout_branch_policy(self.actions, self.branches, obs0=self._obs, gamma=self.gamma,
                                                     noise=self.noise, lo=self.act_lo, hi=self.act_hi,
                                                     bootstrap=self.bootstrap, value_scale=self.value_scale,
                                                     out=self.scores)

    def plan(self, obs=None, iterations=1):
        """`iterations` rounds of sample -> rollout_branch_policy -> update from the envs' current observations
        `obs` [N, 17] (default: env.obs), then the action to apply: policy_act_mean(obs, residual=nominal[0],
        lo, hi) [N, 4], written into self.action."""
        self._obs = obs
        self._iterate(iterations)
        return self.env.policy_act_mean(obs, residual=self.nominal[0], lo=self.act_lo, hi=self.act_hi, out=self.action)
