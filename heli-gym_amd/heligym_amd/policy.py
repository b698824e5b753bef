"""The MLP policy `HeliVecEnv.set_policy` hands to the rollout kernel (hg_set_policy).

Model (include/heligym_amd.h): two tanh hidden layers of width 64,
    a = W3 tanh(W2 tanh(W1 x + b1) + b2) + b3 + exp(log_std) * z,   x = (obs - obs_mean) * obs_scale,
with W1 [64,17], W2 [64,64], W3 [4,64] row-major [out,in] as torch.nn.Linear stores them, fp32.

`pack_policy` is a pure function that runs on the CPU: it takes the weights either as three (W, b)
pairs or as an nn.Sequential of Linear / Tanh / Linear / Tanh / Linear, checks shapes and dtypes and
returns contiguous fp32 tensors in the order hg_set_policy takes them.  `pack_value_head` does the same
for the value head v = w_v . tanh(h2) + b_v on the policy's second hidden layer (hg_set_value_head).
"""
N_OBS, N_HIDDEN, N_ACT = 17, 64, 4
LAYER_SHAPES = ((N_HIDDEN, N_OBS), (N_HIDDEN, N_HIDDEN), (N_ACT, N_HIDDEN))


def _pairs_of(model):
    """[(W, b)] * 3 from an nn.Sequential(Linear, Tanh, Linear, Tanh, Linear) or from three pairs."""
    import torch
    nn = torch.nn
    if isinstance(model, nn.Module):
        mods = list(model.children()) if isinstance(model, nn.Sequential) else None
        kinds = (nn.Linear, nn.Tanh, nn.Linear, nn.Tanh, nn.Linear)
        if mods is None or len(mods) != 5 or not all(isinstance(m, k) for m, k in zip(mods, kinds)):
            got = [type(m).__name__ for m in mods] if mods is not None else type(model).__name__
            shapes = [tuple(m.weight.shape) for m in (mods or []) if isinstance(m, nn.Linear)]
            raise ValueError("policy must be nn.Sequential(Linear(17, 64), Tanh, Linear(64, 64), Tanh, Linear(64, 4)); "
                             f"got {got} with Linear weight shapes {shapes}")
        pairs = []
        for m in mods[0::2]:
            if m.bias is None:
                raise ValueError(f"policy Linear with weight shape {tuple(m.weight.shape)} has no bias")
            pairs.append((m.weight.detach(), m.bias.detach()))
        return pairs
    pairs = list(model)
    if len(pairs) != 3 or any(len(p) != 2 for p in pairs):
        raise ValueError(f"policy must be three (W, b) pairs, got {len(pairs)} items")
    return [(torch.as_tensor(w), torch.as_tensor(b)) for w, b in pairs]


def _vector(v, n, name):
    import torch
    if v is None:
        return None
    v = torch.as_tensor(v)
    if v.dtype != torch.float32 or tuple(v.shape) != (n,):
        raise ValueError(f"{name} must be float32 of shape ({n},), got {v.dtype} of shape {tuple(v.shape)}")
    return v.detach().contiguous()


def pack_policy(model_or_pairs, log_std=None, obs_mean=None, obs_scale=None):
    """Validate a policy and return (W1, b1, W2, b2, W3, b3, log_std, obs_mean, obs_scale): contiguous
    float32 tensors on the device their sources live on (the last three None when absent).  Raises
    ValueError naming the offending shape (or dtype) for anything but the fixed 17-64-64-4 fp32 model."""
    import torch
    out = []
    for j, ((w, b), shape) in enumerate(zip(_pairs_of(model_or_pairs), LAYER_SHAPES), start=1):
        if tuple(w.shape) != shape or tuple(b.shape) != shape[:1]:
            raise ValueError(f"policy layer {j}: W{j} must be {shape} and b{j} {shape[:1]}, "
                             f"got {tuple(w.shape)} and {tuple(b.shape)}")
        if w.dtype != torch.float32 or b.dtype != torch.float32:
            raise ValueError(f"policy layer {j}: W{j} {tuple(w.shape)} / b{j} {tuple(b.shape)} must be float32, "
                             f"got {w.dtype} / {b.dtype}")
        out += [w.detach().contiguous(), b.detach().contiguous()]
    return (*out, _vector(log_std, N_ACT, "log_std"), _vector(obs_mean, N_OBS, "obs_mean"),
            _vector(obs_scale, N_OBS, "obs_scale"))


def pack_value_head(head):
    """Validate a value head v = w_v . tanh(h2) + b_v on the policy's trunk (hg_set_value_head) and return
    (w_v [64], b_v [1]): contiguous float32 tensors.  `head` is an nn.Linear(64, 1) or a (w, b) pair with w
    of shape [1, 64] or [64] and b of shape [1].  Raises ValueError naming the offending shape (or dtype)."""
    import torch
    nn = torch.nn
    if isinstance(head, nn.Module):
        if not isinstance(head, nn.Linear):
            raise ValueError(f"value head must be nn.Linear({N_HIDDEN}, 1) or a (w, b) pair, got {type(head).__name__}")
        if head.bias is None:
            raise ValueError(f"value head Linear with weight shape {tuple(head.weight.shape)} has no bias")
        w, b = head.weight.detach(), head.bias.detach()
    else:
        pair = list(head)
        if len(pair) != 2:
            raise ValueError(f"value head must be nn.Linear({N_HIDDEN}, 1) or a (w, b) pair, got {len(pair)} items")
        if pair[1] is None:
            raise ValueError("value head has no bias: b must be float32 of shape (1,)")
        w, b = torch.as_tensor(pair[0]), torch.as_tensor(pair[1])
    if tuple(w.shape) not in ((1, N_HIDDEN), (N_HIDDEN,)) or tuple(b.shape) != (1,):
        raise ValueError(f"value head: w must be (1, {N_HIDDEN}) or ({N_HIDDEN},) and b (1,), "
                         f"got {tuple(w.shape)} and {tuple(b.shape)}")
    if w.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError(f"value head: w {tuple(w.shape)} / b {tuple(b.shape)} must be float32, got {w.dtype} / {b.dtype}")
    return w.detach().reshape(N_HIDDEN).contiguous(), b.detach().contiguous()


# ---- the learner's side: one flat parameter vector and the clipped PPO loss (hg_ppo_grad)
# name -> (offset, shape) in the flat vector theta [5641], in include/heligym_amd.h's order
PPO_LAYOUT = {
    "W1": (0, (N_HIDDEN, N_OBS)), "b1": (1088, (N_HIDDEN,)),
    "W2": (1152, (N_HIDDEN, N_HIDDEN)), "b2": (5248, (N_HIDDEN,)),
    "W3": (5312, (N_ACT, N_HIDDEN)), "b3": (5568, (N_ACT,)),
    "log_std": (5572, (N_ACT,)),
    "w_v": (5576, (N_HIDDEN,)), "b_v": (5640, (1,)),
}
PPO_N_PARAMS = 5641
LOG_2PI = 1.8378770664093453   # ln(2 pi)


def _count(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def ppo_views(flat):
    """{name: view of `flat` [5641] with the tensor's shape} in PPO_LAYOUT's order (views, no copies)."""
    if tuple(flat.shape) != (PPO_N_PARAMS,):
        raise ValueError(f"the flat parameter vector must have shape ({PPO_N_PARAMS},), got {tuple(flat.shape)}")
    return {k: flat[off:off + _count(shape)].view(shape) for k, (off, shape) in PPO_LAYOUT.items()}


class ActorCriticParams:
    """The actor nn.Sequential(Linear(17, 64), Tanh, Linear(64, 64), Tanh, Linear(64, 4)), the critic head
    nn.Linear(64, 1) on its trunk and log_std (an nn.Parameter or tensor of shape [4]) as ONE flat float32
    vector `theta` [5641] in hg_ppo_grad's layout, with one flat `grad` [5641] beside it.

    Every parameter's .data is re-pointed at its view of `theta` and its .grad at its view of `grad`, so a
    torch optimiser built on `parameters()` updates `theta` in place from what `HeliVecEnv.ppo_grad` wrote
    into `grad`, and `env.set_policy(actor, log_std=...)` / `env.set_value_head(critic)` keep working on the
    same modules.  (Do not call optimizer.zero_grad(): its default drops the .grad views, and ppo_grad
    overwrites `grad` anyway.)  Pure torch, runs on the CPU; the modules are validated by pack_policy / pack_value_head
    (ValueError for anything but the fixed fp32 model)."""

    def __init__(self, actor, critic, log_std):
        import torch
        nn = torch.nn
        pack_policy(actor, log_std=log_std.detach() if isinstance(log_std, torch.Tensor) else log_std)
        pack_value_head(critic)
        if not isinstance(actor, nn.Module) or not isinstance(critic, nn.Module):
            raise ValueError("ActorCriticParams needs the actor and the critic as torch modules (their parameters are "
                             "re-pointed at the flat vector)")
        if log_std is None:
            raise ValueError("log_std must be float32 of shape (4,), got None")
        if not isinstance(log_std, nn.Parameter):
            log_std = nn.Parameter(torch.as_tensor(log_std).detach().clone())
        self.actor, self.critic, self.log_std = actor, critic, log_std
        named = {"W1": actor[0].weight, "b1": actor[0].bias, "W2": actor[2].weight, "b2": actor[2].bias,
                 "W3": actor[4].weight, "b3": actor[4].bias, "log_std": log_std, "w_v": critic.weight,
                 "b_v": critic.bias}
        device = actor[0].weight.device
        for k, p in named.items():
            if p.device != device:
                raise ValueError(f"{k} lives on {p.device}, the actor on {device}")
        self.theta = torch.empty((PPO_N_PARAMS,), dtype=torch.float32, device=device)
        self.grad = torch.zeros((PPO_N_PARAMS,), dtype=torch.float32, device=device)
        tv, gv = ppo_views(self.theta), ppo_views(self.grad)
        self._named = named
        with torch.no_grad():
            for k, p in named.items():
                tv[k].copy_(p.detach().reshape(tv[k].shape))
                p.data = tv[k].view(p.shape)
                p.grad = gv[k].view(p.shape)

    def parameters(self):
        """The nine parameters in the flat vector's order (what an optimiser takes)."""
        return [self._named[k] for k in PPO_LAYOUT]

    def views(self):
        """{name: view of theta} in PPO_LAYOUT's order."""
        return ppo_views(self.theta)


# ---- the optimiser's state on the device (hg_ppo_adam, hg_ppo_update)
# name -> offset in 4-byte words, include/heligym_amd.h's table: the two moments, then the tail's words
PPO_OPT_TAIL = 11296
PPO_OPT_LAYOUT = {
    "m": 0, "v": 5648,
    "applied": PPO_OPT_TAIL + 0, "seen": PPO_OPT_TAIL + 1, "stop": PPO_OPT_TAIL + 2,
    "skipped_nonfinite": PPO_OPT_TAIL + 3, "skipped_stopped": PPO_OPT_TAIL + 4,
    "last_norm": PPO_OPT_TAIL + 5, "last_clip_coef": PPO_OPT_TAIL + 6,
}
PPO_OPT_WORDS = PPO_OPT_TAIL + 16
PPO_OPT_FLOAT_WORDS = ("last_norm", "last_clip_coef")


class PPOOptState:
    """Adam's state for the flat parameter vector, on `device`, in hg_ppo_adam's layout: `state` is one int32
    [11312] tensor (45 248 bytes, zeroed: what hg_ppo_opt_init leaves), `m` and `v` float32 [5641] views of it.
    counters() reads the tail with one copy."""

    def __init__(self, device):
        import torch
        self.state = torch.zeros((PPO_OPT_WORDS,), dtype=torch.int32, device=device)
        self.m = self.state[PPO_OPT_LAYOUT["m"]:PPO_OPT_LAYOUT["m"] + PPO_N_PARAMS].view(torch.float32)
        self.v = self.state[PPO_OPT_LAYOUT["v"]:PPO_OPT_LAYOUT["v"] + PPO_N_PARAMS].view(torch.float32)
        self.tail = self.state[PPO_OPT_TAIL:]
        self.seen = self.tail[1:2]   # the word hg_ppo_update keys its permutations on

    def zero_(self):
        self.state.zero_()
        return self

    def counters(self):
        """{applied, seen, stop, skipped_nonfinite, skipped_stopped: int; last_norm, last_clip_coef: float}
        (one device-to-host copy, which synchronises)."""
        import numpy as np
        t = self.tail.cpu().numpy()
        out = {}
        for k, off in PPO_OPT_LAYOUT.items():
            if off >= PPO_OPT_TAIL:
                w = t[off - PPO_OPT_TAIL:off - PPO_OPT_TAIL + 1]
                out[k] = float(w.view(np.float32)[0]) if k in PPO_OPT_FLOAT_WORDS else int(w[0])
        return out


def ppo_loss(theta_or_params, obs, actions, logp_old, adv, ret, clip, vf_coef, ent_coef, obs_mean=None,
             obs_scale=None):
    """The clipped PPO loss hg_ppo_grad differentiates (include/heligym_amd.h), in plain torch and in the
    dtype of `theta` (an ActorCriticParams, or a flat [5641] tensor in PPO_LAYOUT's order, which may
    require grad).  obs [M,17], actions [M,4], logp_old / adv / ret [M]: the minibatch's rows.  Returns
    (L, stats) with stats the eight values of hg_ppo_grad's stats (index 7, the skipped entries, is 0)."""
    import torch
    theta = theta_or_params.theta if isinstance(theta_or_params, ActorCriticParams) else theta_or_params
    p = ppo_views(theta)
    x = obs
    if obs_mean is not None:
        x = x - obs_mean
    if obs_scale is not None:
        x = x * obs_scale
    h1 = torch.tanh(x @ p["W1"].T + p["b1"])
    h2 = torch.tanh(h1 @ p["W2"].T + p["b2"])
    mu = h2 @ p["W3"].T + p["b3"]
    v = h2 @ p["w_v"] + p["b_v"]
    ls = p["log_std"]
    z = (actions - mu) * torch.exp(-ls)
    logp = -0.5 * (z * z).sum(-1) - ls.sum() - 2.0 * LOG_2PI
    r = torch.exp(logp - logp_old)
    pol = -torch.minimum(r * adv, torch.clamp(r, 1.0 - clip, 1.0 + clip) * adv)
    val = 0.5 * (v - ret) ** 2
    H = ls.sum() + 2.0 * (1.0 + LOG_2PI)
    L = (pol + vf_coef * val).mean() - ent_coef * H
    with torch.no_grad():
        out = ((r < 1.0 - clip) | (r > 1.0 + clip)).to(theta.dtype).mean()
        stats = torch.stack([pol.mean(), val.mean(), (logp_old - logp).mean(), out, H.detach(), L.detach(), r.mean(),
                             torch.zeros((), dtype=theta.dtype, device=theta.device)])
    return L, stats


BC_MODES = ("nll", "mse")


def bc_loss(theta_or_params, obs, target, weight, value_target, mode, vf_coef, ent_coef, obs_mean=None, obs_scale=None):
    """The weighted imitation loss hg_bc_grad differentiates (include/heligym_amd.h), in plain torch and in the
    dtype of `theta` (an ActorCriticParams, or a flat [5641] tensor in PPO_LAYOUT's order, which may require
    grad): the counterpart of ppo_loss.  obs [M,17], target [M,4]: the minibatch's rows and the actions to
    regress onto; weight [M] or None (1); value_target [M] or None (no value term: vf_coef must be 0).
    mode "nll": l = -logp(target) under the policy's Gaussian; "mse": l = 1/2 sum_c (target - mu)^2.
        L = mean(w l + vf_coef * 1/2 (v - y)^2) - ent_coef * H
    Returns (L, stats) with stats the eight values of hg_bc_grad's stats: mean w l, mean 1/2 (v - y)^2, mean
    squared action error, mean w, H, L, mean logp(target), 0 (the skipped entries)."""
    import torch
    if mode not in BC_MODES:
        raise ValueError(f"bc_loss: mode must be one of {BC_MODES}, got {mode!r}")
    if value_target is None and vf_coef != 0:
        raise ValueError("bc_loss: value_target is None, so vf_coef must be 0")
    theta = theta_or_params.theta if isinstance(theta_or_params, ActorCriticParams) else theta_or_params
    p = ppo_views(theta)
    x = obs
    if obs_mean is not None:
        x = x - obs_mean
    if obs_scale is not None:
        x = x * obs_scale
    h1 = torch.tanh(x @ p["W1"].T + p["b1"])
    h2 = torch.tanh(h1 @ p["W2"].T + p["b2"])
    mu = h2 @ p["W3"].T + p["b3"]
    v = h2 @ p["w_v"] + p["b_v"]
    ls = p["log_std"]
    diff = target - mu
    z = diff * torch.exp(-ls)
    logp = -0.5 * (z * z).sum(-1) - ls.sum() - 2.0 * LOG_2PI
    sq = (diff * diff).sum(-1)
    l = -logp if mode == "nll" else 0.5 * sq
    wl = l if weight is None else weight * l
    val = torch.zeros_like(wl) if value_target is None else 0.5 * (v - value_target) ** 2
    H = ls.sum() + 2.0 * (1.0 + LOG_2PI)
    L = (wl + vf_coef * val).mean() - ent_coef * H
    with torch.no_grad():
        one = torch.ones((), dtype=theta.dtype, device=theta.device)
        stats = torch.stack([wl.mean(), val.mean(), sq.mean(), one if weight is None else weight.mean() * one,
                             H.detach(), L.detach(), logp.mean(), 0.0 * one])
    return L, stats
