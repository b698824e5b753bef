"""CPU-side checks of the PPO loss-gradient surface: hg_ppo_grad and hg_ppo_grad_workspace_bytes are
exported and declared with the header's argument counts, the flat parameter layout of heligym_amd.policy
is the header's, ActorCriticParams aliases the modules' parameters into one vector, and ppo_loss is the
loss the header states.  No device calls."""
import math
import re

import pytest
import torch

from test_policy_host import HEADER, header_arg_counts

from heligym_amd import ActorCriticParams, _abi, policy, ppo_loss

NEW = {"hg_ppo_grad_workspace_bytes": 0, "hg_ppo_grad": 19}


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def test_ppo_symbols_exported_and_declared(lib):
    counts = header_arg_counts()
    assert counts["hg_gae"] == 12   # (the parser reads a known prototype right)
    for name, n in NEW.items():
        assert hasattr(lib, name), name
        assert name in _abi.EXPORTED_SYMBOLS
        assert counts[name] == n, (name, counts.get(name))
        assert len(_abi._SIGS[name][1]) == n, name
    assert lib.hg_abi_version() == 3   # purely additive


def test_ppo_grad_refuses_a_null_env_and_reports_its_workspace(lib):
    lib.hg_num_envs(None)
    assert lib.hg_ppo_grad(*(None,) * 9, 4, None, 4, 0.2, 1.0, 0.0, None, None, None, None) == -1
    assert b"env is NULL" in lib.hg_last_error()
    nbytes = lib.hg_ppo_grad_workspace_bytes()
    assert nbytes > 0 and nbytes % 16 == 0


def test_layout_is_the_headers():
    txt = open(HEADER).read()
    n = int(re.search(r"#define\s+HG_PPO_N_PARAMS\s+(\d+)", txt).group(1))
    assert n == 5641 == policy.PPO_N_PARAMS == _abi.HG_PPO_N_PARAMS
    assert list(policy.PPO_LAYOUT) == ["W1", "b1", "W2", "b2", "W3", "b3", "log_std", "w_v", "b_v"]
    end = 0
    for name, (off, shape) in policy.PPO_LAYOUT.items():
        assert off == end, name   # contiguous, in the header's order
        end = off + math.prod(shape)
        # the header's table lists every tensor at its offset
        assert re.search(rf"\b{off}: {name} ", txt), (name, off)
    assert end == n == sum(math.prod(s) for _, s in policy.PPO_LAYOUT.values())


def _modules(dtype=torch.float32, widths=(17, 64, 64, 4), bias=True):
    nn = torch.nn
    torch.manual_seed(11)
    a, b, c, d = widths
    actor = nn.Sequential(nn.Linear(a, b), nn.Tanh(), nn.Linear(b, c), nn.Tanh(), nn.Linear(c, d)).to(dtype)
    critic = nn.Linear(c, 1, bias=bias).to(dtype)
    return actor, critic, nn.Parameter(torch.tensor([-1.0, -0.7, -1.3, -0.9]))


def test_actor_critic_params_alias_one_vector():
    actor, critic, log_std = _modules()
    before = {k: p.detach().clone() for k, p in (("W2", actor[2].weight), ("w_v", critic.weight), ("ls", log_std))}
    P = ActorCriticParams(actor, critic, log_std)
    assert P.theta.shape == (5641,) and P.grad.shape == (5641,) and P.theta.dtype == torch.float32
    v = P.views()
    assert torch.equal(v["W2"], before["W2"]) and torch.equal(v["w_v"], before["w_v"].reshape(64))
    assert torch.equal(v["log_std"], before["ls"])
    lo, hi = P.theta.data_ptr(), P.theta.data_ptr() + 4 * 5641
    glo = P.grad.data_ptr()
    for name, p in zip(policy.PPO_LAYOUT, P.parameters()):
        off = policy.PPO_LAYOUT[name][0]
        assert p.data_ptr() == lo + 4 * off < hi, name
        assert p.grad.data_ptr() == glo + 4 * off and p.grad.shape == p.shape, name
    # writes through either side are seen by the other
    P.theta[1152] = 3.5
    assert float(actor[2].weight.detach()[0, 0]) == 3.5
    P.grad.fill_(0.25)
    assert all(float(p.grad.min()) == 0.25 for p in P.parameters())
    # an optimiser on the module parameters updates theta in place
    theta0 = P.theta.clone()
    opt = torch.optim.Adam(P.parameters(), lr=1e-2)
    opt.step()
    assert P.theta.data_ptr() == lo
    assert float((P.theta - theta0).abs().min()) > 1e-3
    assert torch.equal(P.views()["W1"], actor[0].weight.detach())
    # and the packers still read the same modules
    assert torch.equal(policy.pack_policy(actor)[2], P.views()["W2"])
    assert torch.equal(policy.pack_value_head(critic)[0], P.views()["w_v"])


def test_actor_critic_params_rejects_what_the_kernel_cannot_run():
    actor, critic, log_std = _modules()
    with pytest.raises(ValueError, match=r"\(32, 17\)"):
        ActorCriticParams(_modules(widths=(17, 32, 64, 4))[0], critic, log_std)
    with pytest.raises(ValueError, match=r"float64"):
        ActorCriticParams(_modules(dtype=torch.float64)[0], critic, log_std)
    with pytest.raises(ValueError, match=r"float64"):
        ActorCriticParams(actor, _modules(dtype=torch.float64)[1], log_std)
    with pytest.raises(ValueError, match=r"no bias"):
        ActorCriticParams(actor, _modules(bias=False)[1], log_std)
    with pytest.raises(ValueError, match=r"\(1, 32\)"):
        ActorCriticParams(actor, torch.nn.Linear(32, 1), log_std)
    with pytest.raises(ValueError, match=r"\(5,\)"):
        ActorCriticParams(actor, critic, torch.zeros(5))


def _batch(m, dtype, seed=5):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64).to(dtype)   # noqa: E731
    return dict(theta=0.3 * r(5641), obs=r(m, 17), actions=0.5 * r(m, 4), adv=r(m), ret=r(m), mean=0.1 * r(17),
                scale=1.0 + 0.1 * r(17).abs())


def test_ppo_loss_agrees_with_a_per_sample_loop():
    f64 = torch.float64
    b = _batch(5, f64)
    clip, vf, ent = 0.2, 0.7, 0.01
    th = b["theta"]
    p = {k: th[o:o + math.prod(s)].reshape(s) for k, (o, s) in policy.PPO_LAYOUT.items()}
    logp, val = [], []
    for i in range(5):
        x = [(float(b["obs"][i, c]) - float(b["mean"][c])) * float(b["scale"][c]) for c in range(17)]
        h1 = [math.tanh(sum(float(p["W1"][j, c]) * x[c] for c in range(17)) + float(p["b1"][j])) for j in range(64)]
        h2 = [math.tanh(sum(float(p["W2"][j, c]) * h1[c] for c in range(64)) + float(p["b2"][j])) for j in range(64)]
        mu = [sum(float(p["W3"][j, c]) * h2[c] for c in range(64)) + float(p["b3"][j]) for j in range(4)]
        val.append(sum(float(p["w_v"][c]) * h2[c] for c in range(64)) + float(p["b_v"][0]))
        z = [(float(b["actions"][i, j]) - mu[j]) * math.exp(-float(p["log_std"][j])) for j in range(4)]
        logp.append(-0.5 * sum(q * q for q in z) - sum(float(q) for q in p["log_std"]) - 2 * math.log(2 * math.pi))
    # old log-probs that put ratios inside, above and below the clip range
    lp_old = torch.tensor(logp, dtype=f64) - torch.tensor([0.0, 0.5, -0.5, 0.05, -0.05], dtype=f64)
    H = sum(float(q) for q in p["log_std"]) + 2 * (1 + math.log(2 * math.pi))
    pol = vals = kl = outside = rsum = 0.0
    for i in range(5):
        r, A = math.exp(logp[i] - float(lp_old[i])), float(b["adv"][i])
        pol += -min(r * A, min(max(r, 1 - clip), 1 + clip) * A)
        vals += 0.5 * (val[i] - float(b["ret"][i])) ** 2
        kl += float(lp_old[i]) - logp[i]
        outside += float(r < 1 - clip or r > 1 + clip)
        rsum += r
    want = [pol / 5, vals / 5, kl / 5, outside / 5, H, pol / 5 + vf * vals / 5 - ent * H, rsum / 5, 0.0]
    L, stats = ppo_loss(th, b["obs"], b["actions"], lp_old, b["adv"], b["ret"], clip, vf, ent, b["mean"], b["scale"])
    assert L.dtype == f64 and stats.dtype == f64 and stats.shape == (8,)
    assert 0.0 < want[3] < 1.0
    assert float(L) == pytest.approx(want[5], rel=1e-12, abs=1e-13)
    for j in range(8):
        assert float(stats[j]) == pytest.approx(want[j], rel=1e-12, abs=1e-13), j


def test_ppo_loss_gradient_vanishes_when_every_sample_is_clipped_out():
    f64 = torch.float64
    b = _batch(5, f64, seed=6)
    th = b["theta"].clone().requires_grad_(True)
    with torch.no_grad():   # logp of the current weights, then ratios of e^(+-1) on the clipped side of each advantage
        p = policy.ppo_views(th)
        h2 = torch.tanh(torch.tanh(b["obs"] @ p["W1"].T + p["b1"]) @ p["W2"].T + p["b2"])
        z = (b["actions"] - (h2 @ p["W3"].T + p["b3"])) * torch.exp(-p["log_std"])
        logp = -0.5 * (z * z).sum(-1) - p["log_std"].sum() - 2 * policy.LOG_2PI
    lp_old = logp - torch.sign(b["adv"])   # r = e for A > 0, 1 / e for A < 0
    L, stats = ppo_loss(th, b["obs"], b["actions"], lp_old, b["adv"], b["ret"], 0.2, 0.0, 0.0)
    L.backward()
    assert float(stats[3]) == 1.0
    g = policy.ppo_views(th.grad)
    for name in ("W1", "b1", "W2", "b2", "W3", "b3", "log_std"):
        assert torch.count_nonzero(g[name]) == 0, name
    assert torch.count_nonzero(th.grad) == 0   # (vf_coef = 0: the value head's too)
