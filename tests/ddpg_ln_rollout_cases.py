"""
SyntheticVecEnv.ddpg_rollout_into with a LayerNorm actor (use_layernorm=True) on the one-launch path, with and without a
device parameter noise; shared by the CPU tier (test_ddpg_ln_rollout_cpu.py) and the GPU tier
(test_gpu_ddpg_ln_rollout.py):

  * ``DdpgLnRolloutCpuKernels`` -- the torch-CPU double that runs a LayerNorm actor (the ln arguments of
    synth_ddpg_rollout and param_noise_*) on top of the parameter-noise double; its fills are the float64 Philox
    restatement rounded to fp32;
  * ``set_layernorm`` -- random gains and biases (the defaults 1 / 0 would let a wrong affine step pass);
  * ``actor_out`` / ``action_distance`` -- the LayerNorm actor in float64;
  * ``make`` / ``run`` / ``final`` / ``same_bytes`` -- an env with its agent and replay, calls of ddpg_rollout_into, every
    byte they leave per actor.
"""
import numpy as np
import torch

import ddpg_rollout_cases as DC
import episode_monitor_cases as EM
import helpers as H
import param_noise_ref as PR
import test_param_noise_cpu as TP

LN_KEYS = ('ln1.W', 'ln1.b', 'ln2.W', 'ln2.b')
ORDER = PR.ORDER + LN_KEYS                       # DDPGModel's order of the actor's flat parameters
SEED, PSEED = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
EP, N_STEP = 11, 3
CALLS = (9, 13, 6)                               # episodes of 11 end inside calls, later calls start mid-episode
# actor shapes D, H1, H2, A
TINY = (5, 12, 8, 3)          # both widths below one 16-feature tile and below 64 lanes; D no multiple of 4
ODD = (17, 76, 132, 6)        # 76 = 64 + 12: a second, partial column pass; 132: just past two full ones
DEFAULT = (17, 300, 200, 6)
WIDE = (17, 640, 640, 6)      # the width limit: ten column passes
SHAPES = (TINY, ODD, DEFAULT, WIDE)


def closing(steps, t0=0, episode_len=EP, n_step=N_STEP):
    return sum(1 for s in range(steps) if (t0 + s) % episode_len >= n_step - 1)


class DdpgLnRolloutCpuKernels(TP.ParamNoiseCpuKernels):
    name = 'torch-cpu-double+ddpg-ln-rollout'
    ddpg_ln_launch = True
    _step = DC.DdpgRolloutCpuKernels.synth_ddpg_step      # (the launches' own steps: not the env's per-step calls)

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.ln_launches, self.ln_refreshes = [], []

    def _mu_ln(self, net, W, ln, eps, state):
        F = torch.nn.functional
        H1, H2 = net.H1, net.H2
        g1, c1, g2, c2 = ln[:H1], ln[H1:2 * H1], ln[2 * H1:2 * H1 + H2], ln[2 * H1 + H2:]
        rows = []
        for a in range(state.shape[0]):         # batch-1 forwards through the double's own layers, as DDPGAgent.act
            h1 = torch.relu(F.linear(state[a:a + 1], W['W1'], W['b1']))
            self.layernorm_forward(h1, g1, c1, eps, h1)
            h2 = torch.relu(F.linear(h1, W['W2'], W['b2']))
            self.layernorm_forward(h2, g2, c2, eps, h2)
            rows.append(torch.tanh(F.linear(h2, W['W3'], W['b3'])))
        return torch.cat(rows)

    def synth_ddpg_rollout(self, net, packed, r, steps, actors_per_workgroup=0, ln=None, ln_eps=0.0, pn=None,
                           measure_step=-1):
        if ln is None:
            return super().synth_ddpg_rollout(net, packed, r, steps, actors_per_workgroup, pn=pn,
                                              measure_step=measure_step)
        if pn is not None:
            self.launches.append(dict(steps=steps, measure_step=measure_step, acts=pn.acts, t=int(r['t']),
                                      actors_per_workgroup=actors_per_workgroup, ln=True))
        assert actors_per_workgroup in (0, 4, 8, 16) and ln.numel() == 2 * (net.H1 + net.H2)
        self.ln_launches.append(dict(steps=steps, t=int(r['t'])))
        n, cap = r['state'].shape[0], r['tables']['obs'].shape[0]
        W = dict(self._packed_views(packed, net))
        W.update({k: net.views[k] for k in ('b1', 'b2', 'b3')})
        r = dict(r)
        eps = r['eps']
        for s in range(steps):
            mu = self._mu_ln(net, W, ln, ln_eps, r['state'])
            r['eps'] = None if eps is None else eps[s]
            self._step(r, mu)
            if r['t'] >= r['n_step'] - 1:
                r['cursor'] = (r['cursor'] + n) % cap
            r['t'] = 0 if r['t'] + 1 >= r['episode_len'] else r['t'] + 1

    # ---- parameter noise: the fills are real (the restatement rounded to fp32), refreshes and launches are recorded ----
    @staticmethod
    def _fill(flat, pn, p, out):
        sg = np.float32(float(pn.sigma[p]))
        z = PR.normal(pn.seed, pn.agent_base + p, pn.generation, np.arange(flat.numel())).astype(np.float32)
        out.copy_(flat + torch.as_tensor(sg * z))

    def param_noise_fill(self, net, pn, p, out, ln=None):
        self._fill(torch.cat([net.views[k].reshape(-1) for k in PR.ORDER] + ([] if ln is None else [ln])), pn, p, out)

    def param_noise_copy_numel(self, net, ln=False):
        return 64 + (2 * (net.H1 + net.H2) + 63) // 64 * 64 if ln else super().param_noise_copy_numel(net)

    def param_noise_refresh(self, net, pn, ln=None):
        if ln is None:
            return super().param_noise_refresh(net, pn)
        self.ln_refreshes.append(dict(generation=pn.generation, acts=pn.acts, ln=ln.numel()))


def set_layernorm(agent, seed=7):
    """gains uniform in [0.5, 1.5), biases normal(0, 0.1), from a seeded generator"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in agent.model.actor_ln.items():
            src = torch.rand(v.shape, generator=g) + 0.5 if k.endswith('.W') else 0.1 * torch.randn(v.shape, generator=g)
            v.copy_(src)


def actor_params(agent):
    """the clean actor's ten arrays by name (numpy)"""
    out = {k: v.detach().cpu().numpy() for k, v in agent.model.actor.views.items()}
    out.update({k: v.detach().cpu().numpy() for k, v in agent.model.actor_ln.items()})
    return out


def layernorm64(x, gain, bias, eps):
    m = x.mean()
    return (x - m) / np.sqrt(((x - m) ** 2).mean() + eps) * gain + bias


def actor_out(params, x, eps):
    """tanh(W3 LN2(relu(W2 LN1(relu(W1 x + b1)) + b2)) + b3) in float64"""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    h1 = layernorm64(np.maximum(p['W1'] @ np.asarray(x, dtype=np.float64) + p['b1'], 0.0), p['ln1.W'], p['ln1.b'], eps)
    h2 = layernorm64(np.maximum(p['W2'] @ h1 + p['b2'], 0.0), p['ln2.W'], p['ln2.b'], eps)
    return np.tanh(p['W3'] @ h2 + p['b3'])


def action_distance(clean, noisy, x, eps):
    d = actor_out(noisy, x, eps) - actor_out(clean, x, eps)
    return float(np.sqrt(np.sum(d * d)))


def make(n, shape, noise='ou_noise', layernorm=True, ptype=None, apa=4, agent_base=0, actor_base=0, attach=False,
         params=None, episode_len=EP, capacity=4096, device='cuda', kernels=None, streams=False, w3_scale=1.0):
    """-> (agent, venv, replay, DeviceParamNoise or None, (lc, ec, sc)).  noise: 'normal' | 'ou_noise' | 'deterministic'; params: the
    actor's arrays to load (LayerNorm keys too); streams: the episode monitor and the exploration stream attached, the
    actors' global ids actor_base .. (their env seeds those ids)"""
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    D, H1, H2, A = shape
    det = noise == 'deterministic'
    lc, ec, sc = DC.configs(D, A, n, hidden=(H1, H2), n_step=N_STEP, noise_type='normal' if det else noise,
                            layernorm=layernorm, param_noise_type=ptype, memory_size=capacity, theta=2.0, dt=0.02,
                            folder='surreal_amd_ddpg_ln_rollout')
    agent = DC.make_agent(lc, ec, sc, mode='eval_deterministic_local' if det else 'training', w3_scale=w3_scale)
    if layernorm:
        set_layernorm(agent)
    if params is not None:
        with torch.no_grad():
            for k, v in params.items():
                (agent.model.actor_ln if k.startswith('ln') else agent.model.actor.views)[k].copy_(v)
    kw = dict(kernels=kernels) if kernels is not None else {}
    venv = SyntheticVecEnv(n, D, A, episode_len=episode_len, device=device,
                           seeds=list(range(actor_base, actor_base + n)), **kw)
    if streams:
        venv.attach_monitor(capacity=4)
        venv.attach_noise(SEED, actor_base=actor_base)
    pn = venv.attach_param_noise(agent, PSEED, actors_per_agent=apa, agent_base=agent_base) if attach else None
    return agent, venv, replay_of(lc, ec, sc), pn, (lc, ec, sc)


def replay_of(lc, ec, sc):
    from surreal_amd.replay import UniformReplay
    return UniformReplay(lc, ec, sc)


def run(agent, venv, replay, calls, eps=None, **kw):
    rows, s0 = 0, 0
    for T in calls:
        rows += venv.ddpg_rollout_into(agent, replay, T, eps=None if eps is None else eps[s0:s0 + T], **kw)
        s0 += T
    return rows


def final(venv, replay, rows):
    """every byte a run leaves: the ring per actor [actor, closing step, .] and whole, the env state, the OU and carry
    tensors, the monitor's state where one is attached"""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    n = venv.n
    ring = H.device_ring(replay, DC.FIELDS)
    out = {'ring_' + k: torch.as_tensor(v[:rows].reshape(rows // n, n, -1)).transpose(0, 1).contiguous()
           for k, v in ring.items()}
    out['rest'] = torch.cat([torch.as_tensor(v[rows:].reshape(-1)) for v in ring.values()])    # never written: zero
    out['state'] = venv.state.cpu()
    out.update({k: venv._ddpg[k].cpu() for k in ('ou', 'carry_obs', 'carry_act', 'carry_rew')})
    if getattr(venv, 'monitor', None) is not None:
        out.update({'mon_' + k: torch.as_tensor(v).reshape(n, -1) for k, v in EM.monitor_state(venv.monitor).items()})
    return out


def same_bytes(got, want, lo=0, hi=None):
    """`want` (a run over the actors lo .. hi - 1 alone) against those actors of `got`"""
    assert set(got) == set(want)
    for k in want:
        if k == 'rest':
            assert not got[k].view(torch.int32).any() and not want[k].view(torch.int32).any()
            continue
        g = got[k][lo:hi].contiguous()
        assert g.shape == want[k].shape and g.dtype == want[k].dtype, k
        assert torch.equal(g.view(torch.uint8), want[k].contiguous().view(torch.uint8)), k


def max_float_difference(got, want):
    """-> the largest |difference| over the float fields two runs leave; dones, the shapes and the rows never written
    must agree exactly"""
    assert set(got) == set(want)
    worst = 0.0
    for k in want:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, k
        if k in ('ring_dones', 'rest') or k.startswith('mon_'):
            assert torch.equal(g, w), k
        else:
            assert torch.isfinite(g).all() and torch.isfinite(w).all(), k
            worst = max(worst, float((g.double() - w.double()).abs().max()))
    assert not want['rest'].view(torch.int32).any()
    return worst
