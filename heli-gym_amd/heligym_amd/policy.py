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
