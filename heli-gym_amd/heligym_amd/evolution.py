"""Evolution strategies on the device: OpenAI-ES (antithetic pairs, centred ranks) around the population
rollout, composed only of HeliVecEnv's calls (es_perturb, rollout_population, pop_fitness, es_grad,
ppo_adam, set_policy_theta), so a generation makes no host decision and can be captured into a graph.

The NumPy functions at the end restate what the kernels compute (include/heligym_amd.h), for the tests.
"""
import numpy as np

from . import _abi

N_PERTURBED = _abi.HG_ES_N_PERTURBED


class ES:
    """An ES learner for `params` (an ActorCriticParams on the env's device) with Adam `state` (a
    PPOOptState): `population` members (even) of `envs_per_member` consecutive envs each.

    generation(K, chunks) enqueues one generation on the current stream:
      es_perturb (noise keyed by `seed` and the state's `applied` word, so every applied step -- and every
      replay of a captured generation -- draws fresh noise), then `chunks` times rollout_population(K) +
      pop_fitness (the first with restart), then es_grad, ppo_adam and, with publish=True,
      set_policy_theta.  All buffers are allocated here, none in generation(): it is capturable.
    stats: float32 [8], es_grad's row of the last generation.  fitness: float32 [P].  member_theta
    [P, 5641] is kept when keep_members=True (best_member())."""

    def __init__(self, env, params, state, population, envs_per_member, sigma=0.05, seed=0, lr=1e-2,
                 betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, lr_dev=None, mode="window", stochastic=False,
                 obs_mean=None, obs_scale=None, keep_members=True, publish=True):
        t = env.torch
        self.env, self.params, self.state = env, params, state
        self.P, self.envs_per_member = env._pop_members(population, envs_per_member, "ES")
        env._pop_count(self.P, "ES", even=True, cap=_abi.HG_ES_MAX_POP)
        self.sigma, self.seed = env._sigma(sigma, "ES"), int(seed)
        if mode not in _abi.POP_FIT_MODES:
            raise ValueError(f"ES: mode must be one of {sorted(_abi.POP_FIT_MODES)}, got {mode!r}")
        self.mode, self.stochastic, self.publish = mode, bool(stochastic), bool(publish)
        self.obs_mean, self.obs_scale = obs_mean, obs_scale
        self.opt = dict(lr=lr, betas=betas, eps=eps, max_grad_norm=max_grad_norm, lr_dev=lr_dev)
        dev = env.device
        self.images = t.empty((self.P, _abi.HG_POLICY_IMAGE_FLOATS), dtype=t.float32, device=dev)
        self.member_theta = (t.empty((self.P, _abi.HG_PPO_N_PARAMS), dtype=t.float32, device=dev)
                             if keep_members else None)
        self.sums = t.zeros((self.P,), dtype=t.float64, device=dev)
        self.fitness = t.zeros((self.P,), dtype=t.float32, device=dev)
        self.alive = t.ones((env.num_envs,), dtype=t.uint8, device=dev)
        self.stats = t.zeros((8,), dtype=t.float32, device=dev)
        self.gen_dev = state.tail[0:1]   # `applied`
        self.obs_last = None
        self._out = None
        env._es_workspace(self.P)

    def generation(self, K, chunks=1, obs0=None):
        """One generation (see the class); returns (fitness [P], stats [8]).  obs0: the observations the
        first chunk starts from (default: the env's `obs`); later chunks start from the previous one's last
        row."""
        env = self.env
        K, chunks = int(K), int(chunks)
        if K < 1 or chunks < 1:
            raise ValueError("ES.generation: K and chunks must be >= 1")
        env.es_perturb(self.params, self.P, self.sigma, self.seed, gen_dev=self.gen_dev, stochastic=self.stochastic,
                       obs_mean=self.obs_mean, obs_scale=self.obs_scale, out=self.images,
                       member_theta=self.member_theta)
        o0 = obs0
        for c in range(chunks):
            self._out = env.rollout_population(K, self.images, self.envs_per_member, obs0=o0, out=self._out)
            _, obs, rew, term, trunc, _ = self._out
            env.pop_fitness(rew, term, trunc, self.P, self.envs_per_member, self.sums, mode=self.mode,
                            restart=(c == 0), alive=self.alive, out=self.fitness)
            o0 = obs[K - 1]
        self.obs_last = o0
        env.es_grad(self.params, self.fitness, self.sigma, self.seed, gen_dev=self.gen_dev, stats=self.stats)
        env.ppo_adam(self.params, self.state, **self.opt)
        if self.publish:
            env.set_policy_theta(self.params, obs_mean=self.obs_mean, obs_scale=self.obs_scale)
        return self.fitness, self.stats

    def best_member(self):
        """(index, fitness, theta [5641] or None) of the last generation's best member (synchronises)."""
        st = self.stats.cpu().numpy()
        i = int(st[4])
        if i < 0:
            return -1, float("nan"), None
        th = None if self.member_theta is None else self.member_theta[i].clone()
        return i, float(self.fitness[i].item()), th


# ---- NumPy restatements
def es_utilities_ref(fitness):
    """hg_es_grad's centred ranks, float32 [P]: r_p = #{q: f_q < f_p} + #{q < p: f_q == f_p} with every
    non-finite fitness taken as -inf; u_p = float32(r_p) / float32(P - 1) - 0.5 in float32."""
    f = np.asarray(fitness, dtype=np.float32)
    P = f.shape[0]
    if P < 2:
        raise ValueError("es_utilities_ref: P must be >= 2")
    key = np.where(np.isfinite(f), f, np.float32(-np.inf)).astype(np.float32)
    order = np.argsort(key, kind="stable")   # stable: equal keys keep index order
    r = np.empty(P, dtype=np.int64)
    r[order] = np.arange(P)
    q = r.astype(np.float32) / np.float32(P - 1)
    return (q - np.float32(0.5)).astype(np.float32)


def es_grad_ref(fitness, eps, sigma):
    """hg_es_grad's gradient in float64, [5641]: -(1 / (P sigma)) sum_j (u_2j - u_2j+1) eps_j on the first
    5572 entries, 0 beyond.  eps: [P / 2, 5572] (hg_es_noise's rows)."""
    u = es_utilities_ref(fitness)
    P = u.shape[0]
    eps = np.asarray(eps, dtype=np.float64)
    if P % 2 or eps.shape != (P // 2, N_PERTURBED):
        raise ValueError(f"es_grad_ref: eps must be [{P // 2}, {N_PERTURBED}] for {P} members")
    w = (u[0::2] - u[1::2]).astype(np.float32).astype(np.float64)
    g = np.zeros(_abi.HG_PPO_N_PARAMS, dtype=np.float64)
    g[:N_PERTURBED] = -(w @ eps) / (P * float(np.float32(sigma)))
    return g


def pop_fitness_ref(reward, terminated, truncated, population, envs_per_member, mode="window", alive=None, sums=None):
    """hg_pop_fitness in float64: returns (sums [P], fitness [P] float32, alive [N] uint8).  reward [K, N];
    alive / sums: the state before the call (None: a restart)."""
    r = np.asarray(reward, dtype=np.float64)
    K, N = r.shape
    P, m = int(population), int(envs_per_member)
    if mode not in _abi.POP_FIT_MODES:
        raise ValueError(f"pop_fitness_ref: unknown mode {mode!r}")
    al = np.ones(N, dtype=bool) if alive is None else np.asarray(alive).astype(bool).copy()
    s = np.zeros(P, dtype=np.float64) if sums is None else np.asarray(sums, dtype=np.float64).copy()
    env_sum = np.zeros(N, dtype=np.float64)
    if mode == "window":
        for k in range(K):
            env_sum = env_sum + r[k]
    else:
        done = (np.asarray(terminated) != 0) | (np.asarray(truncated) != 0)
        for k in range(K):
            env_sum = np.where(al, env_sum + r[k], env_sum)
            al = al & ~done[k]
    fit = np.empty(P, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for p in range(P):
            lo, hi = p * m, min(N, (p + 1) * m)
            s[p] = s[p] + env_sum[lo:hi].sum()
            fit[p] = np.float32(s[p] / (hi - lo))
    return s, fit, al.astype(np.uint8)
