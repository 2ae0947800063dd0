"""
SyntheticVecEnv.ddpg_rollout_into against the host path it replaces, shared by the CPU tier (test_ddpg_rollout_cpu.py)
and the GPU tier (test_gpu_ddpg_rollout.py):

  * ``DdpgRolloutCpuKernels`` -- the torch-CPU double of the three new entry points (a subclass of the existing
    double).  It forms every actor's mu the way the batch-1 ``DDPGAgent.act`` does, one row at a time through the
    double's dense layers, so that the CPU tier can compare bit for bit;
  * ``host_ring`` -- n ``SyntheticEnv`` + ``DDPGAgent(agent_id=a, num_agents=n)`` + ``ExpSenderWrapperSSARNStepBootstrap``
    driven step by step (reset / pre_episode on done), the noise draws injected, and the transitions they emit placed
    where the device writes them: the k-th closing step at rows (k n + a) mod capacity.
"""
import numpy as np
import torch

import helpers as H
from cpu_kernels import TorchCpuKernels
from surreal_amd import _lib as L
from surreal_amd.env.synthetic_env import _drift

FIELDS = ('obs', 'obs_next', 'actions', 'rewards', 'dones')


class DdpgRolloutCpuKernels(TorchCpuKernels):
    name = 'torch-cpu-double+ddpg-rollout'
    ddpg_ln_launch = False        # (kernels.ddpg_ln_launch: no LayerNorm actor in the launch; the camera double inherits it)

    def synth_ddpg_rollout_supported(self, net, ln=False):
        return self.lib_supported('smx_synth_ddpg_rollout_supported', net.D, net.H1, net.H2, net.OUT, bool(ln))

    def _mu_rows(self, net, W, b, state):
        F = torch.nn.functional
        rows = []
        for a in range(state.shape[0]):         # batch-1 forwards, as DDPGAgent.act
            h1 = torch.relu(F.linear(state[a:a + 1], W['W1'], b['b1']))
            h2 = torch.relu(F.linear(h1, W['W2'], b['b2']))
            rows.append(torch.tanh(F.linear(h2, W['W3'], b['b3'])))
        return torch.cat(rows)

    def synth_ddpg_rollout(self, net, packed, r, steps, actors_per_workgroup=0):
        assert actors_per_workgroup in (0, 4, 8, 16)
        n = r['state'].shape[0]
        m = 0
        t = int(r['t'])
        for _ in range(steps):
            m += t >= r['n_step'] - 1
            t = 0 if t + 1 >= r['episode_len'] else t + 1
        assert n * m <= r['tables']['obs'].shape[0]
        W = self._packed_views(packed, net)
        r = dict(r)
        eps, cap = r['eps'], r['tables']['obs'].shape[0]
        for s in range(steps):
            mu = self._mu_rows(net, W, net.views, r['state'])
            r['eps'] = None if eps is None else eps[s]
            self.synth_ddpg_step(r, mu)
            if r['t'] >= r['n_step'] - 1:
                r['cursor'] = (r['cursor'] + n) % cap
            r['t'] = 0 if r['t'] + 1 >= r['episode_len'] else r['t'] + 1

    def synth_ddpg_step(self, r, mu):
        """the kernel's expressions in the same fp64 order"""
        state, init = r['state'], r['init_state']
        n, D = state.shape
        A = mu.shape[1]
        N, tau = int(r['n_step']), int(r['t'])
        a = mu.clamp(-1.0, 1.0)
        noise = r['noise_type']
        if noise == L.SMX_DDPG_NOISE_GAUSSIAN:
            a = (a.double() + (0.0 + r['sigmas'].view(-1, 1) * r['eps'].double())).float()
        elif noise == L.SMX_DDPG_NOISE_OU:
            x = r['ou']
            if tau == 0:
                x.zero_()
            x.copy_((x + (r['theta'] * (0.0 - x)) * r['dt']) + (r['sigmas'] * r['root_dt']).view(-1, 1) * r['eps'].double())
            a = (a.double() + x).float()
        a = a.clamp(-1.0, 1.0)
        k = torch.arange(D)
        sn = (torch.tensor(0.9, dtype=torch.float32) * state + torch.tensor(0.5, dtype=torch.float32) * a[:, k % A])
        sn = (sn + torch.as_tensor(_drift(D))).clamp(-10.0, 10.0)
        q = torch.zeros(n, dtype=torch.float64)
        for j in range(A):
            v = a[:, j].double()
            q = q + v * v
        rew = (-0.1 * q + 0.05 * sn[:, 0].double()).float()
        done = tau + 1 >= r['episode_len']
        slot, jslot = tau % N, (tau + 1) % N
        r['carry_obs'][:, slot] = state
        r['carry_act'][:, slot] = a
        r['carry_rew'][:, slot] = rew
        if tau >= N - 1:
            tabs = r['tables']
            cap = tabs['obs'].shape[0]
            rows = (int(r['cursor']) + torch.arange(n)) % cap
            j = tau - N + 1
            R = r['carry_rew'][:, j % N].double()
            for u in range(j + 1, tau + 1):
                e = (u - j) if u >= N - 1 else (N - 1 - j)
                R = R + r['gpow'][e] * r['carry_rew'][:, u % N].double()
            tabs['obs'][rows] = r['carry_obs'][:, jslot]
            tabs['actions'][rows] = r['carry_act'][:, jslot]
            tabs['obs_next'][rows] = sn
            tabs['rewards'][rows] = R.float().view(n, 1)
            tabs['dones'][rows] = 1.0 if done else 0.0
        state.copy_(init if done else sn)


def configs(D, A, n, hidden=(24, 16), n_step=3, gamma=0.99, noise_type='normal', layernorm=False, memory_size=4096,
            max_sigma=1.0, theta=0.15, dt=1e-3, param_noise_type=None, folder='surreal_amd_ddpg_rollout'):
    from surreal_amd.main.ddpg_configs import ddpg_learner_config, ddpg_env_config, ddpg_session_config
    lc = ddpg_learner_config()
    lc.model.actor_fc_hidden_sizes, lc.model.critic_fc_hidden_sizes = list(hidden), [32, 24]
    lc.model.use_layernorm = layernorm
    lc.algo.n_step, lc.algo.gamma = n_step, gamma
    ex = lc.algo.exploration
    ex.noise_type, ex.max_sigma, ex.theta, ex.dt, ex.param_noise_type = noise_type, max_sigma, theta, dt, param_noise_type
    lc.replay.memory_size = memory_size
    return lc, ddpg_env_config(D, A, num_agents=n), ddpg_session_config(H.session_folder(folder))


def make_agent(lc, ec, sc, agent_id=0, mode='training', seed=0, w3_scale=8.0):
    """w3_scale > 1: a last layer that is not near zero, so that actions reach the clip without noise too (it scales
    the rounding differences of two summation orders with it)"""
    from surreal_amd.agent import DDPGAgent
    torch.manual_seed(seed)
    ag = DDPGAgent(lc, ec, sc, agent_id=agent_id, agent_mode=mode)
    with torch.no_grad():
        ag.model.actor.views['W3'].mul_(w3_scale)
    return ag


def host_ring(agent, lc, ec, sc, n, episode_len, eps_all, capacity):
    """the host path over all steps of eps_all [steps, n, A] (numpy) -> (ring {field: [capacity, width]}, rows written)"""
    from surreal_amd.agent import DDPGAgent
    from surreal_amd.env import ExpSenderWrapperSSARNStepBootstrap
    from surreal_amd.env.synthetic_env import SyntheticEnv
    D, A = agent.model.input_dim, agent.action_dim
    steps = eps_all.shape[0]
    actors = []
    for a in range(n):
        ag = DDPGAgent(lc, ec, sc, agent_id=a, agent_mode=agent.agent_mode)
        ag.model.load_state_dict(agent.model.state_dict())
        sent = []
        w = ExpSenderWrapperSSARNStepBootstrap(SyntheticEnv(D, A, episode_len=episode_len, seed=a), lc, sc,
                                               sink=sent.append)
        if ag.noise is not None:
            clock = {'t': 0}
            ag.noise._eps = (lambda a_=a, c=clock: np.asarray(eps_all[c['t'], a_], dtype=np.float64))
            ag._clock = clock
        ag.pre_episode()
        obs, _ = w.reset()
        actors.append([ag, w, obs, sent])
    ring = {'obs': np.zeros((capacity, D), np.float32), 'obs_next': np.zeros((capacity, D), np.float32),
            'actions': np.zeros((capacity, A), np.float32), 'rewards': np.zeros((capacity, 1), np.float32),
            'dones': np.zeros((capacity, 1), np.float32)}
    cursor = total = 0
    for s in range(steps):
        emitted = []
        for a, st in enumerate(actors):
            ag, w, obs, sent = st
            if ag.noise is not None:
                ag._clock['t'] = s
            action = ag.act(obs)
            obs, _, done, _ = w.step(action)
            if done:
                ag.pre_episode()
                obs, _ = w.reset()
            st[2] = obs
            emitted.append(list(sent))
            del sent[:]
        counts = {len(e) for e in emitted}
        assert counts <= {0, 1} and len(counts) == 1, counts     # a shared clock: all actors or none
        if counts == {1}:
            for a, (e,) in enumerate(emitted):
                row = (cursor + a) % capacity
                ring['obs'][row] = e['obs'][0]['low_dim']['flat_inputs']
                ring['obs_next'][row] = e['obs'][1]['low_dim']['flat_inputs']
                ring['actions'][row] = e['action']
                ring['rewards'][row] = np.float32(e['reward'])
                ring['dones'][row] = float(e['done'])
            cursor = (cursor + n) % capacity
            total += n
    return ring, total
