"""
SyntheticVecEnv.ppo_rollout_into (moving windows straight into the FIFO) against the host path it replaces, shared by
the CPU tier (test_ppo_window_rollout_cpu.py) and the GPU tier (test_gpu_ppo_window_rollout.py):

  * ``PpoWindowCpuKernels`` -- the torch-CPU double of the new entry points (a subclass of the LSTM rollout's double).
    Per step it issues the ops PPOAgent.act_batch issues (z-filter, [LSTM at T = 1,] actor, sampling head) and the
    synthetic step with SyntheticEnv's fp32 expressions, then the window rule of the kernel (carry rings, closing
    windows at rows (cursor + k n + a) % capacity), so that the CPU tier compares bit for bit;
  * ``host_windows`` -- n ``SyntheticEnv`` behind ``ExpSenderWrapperMultiStepMovingWindowWithInfo``, driven step by step
    by ``act_batch`` with injected eps (reset on done, the LSTM state never reset), the windows they emit in the order
    the device writes them: closing step by closing step, actor by actor;
  * ``cut_windows`` -- the same windows cut on the host from a [n, S + 1] rollout table and its clock.
"""
import numpy as np
import torch

import helpers as H
import lstm_rollout_cases as LC
from surreal_amd import _lib as L
from surreal_amd.env.synthetic_env import _drift

FIELDS = ('obs', 'obs_next', 'actions', 'rewards', 'dones', 'pds')


class PpoWindowCpuKernels(LC.LstmRolloutCpuKernels):
    name = 'torch-cpu-double+ppo-window'

    def __init__(self):
        super().__init__()
        self.window_launches = 0

    def synth_ppo_window_rollout_supported(self, model):
        if model.if_pixel or (model.if_rnn and model.rnn_layers != 1):
            return False
        a, r = model.actor, model.rnn
        if not model.if_rnn:
            return self.lib_supported('smx_synth_ppo_window_rollout_supported', a.D, 0, a.H1, a.H2, a.OUT)
        return a.D == r.H and self.lib_supported('smx_synth_ppo_window_rollout_supported', r.D, r.H, a.H1, a.H2, a.OUT)

    def _act_step(self, model, state, h, c, noise_scale, eps_s, zfilter):
        """act_batch's ops for all actors -> (actions, pd, h', c')"""
        n, D = state.shape
        actor, A = model.actor, model.actor.OUT
        if model.if_rnn:
            Hp, Hl = model.rnn_hidden, model.rnn_hidden_logical
            if zfilter is not None:
                m, sd = torch.empty(D), torch.empty(D)
                self.zfilter_stats(zfilter.running_sum, zfilter.running_sumsq, zfilter.count, zfilter.eps, m, sd)
                x = torch.empty(n, D)
                self.zfilter_forward(state, m, sd, x)
            else:
                x = state.clone()
            out, gates, cs = torch.empty(n, Hp), torch.empty(n, 4 * Hp), torch.empty(n, Hp)
            hn, cn = torch.empty(n, Hp), torch.empty(n, Hp)
            self.lstm_forward(model.rnn, x, n, 1, h, c, gates, out, cs, None, hn, cn)
            h, c = torch.zeros(n, Hp), torch.zeros(n, Hp)
            h[:, :Hl], c[:, :Hl] = hn[:, :Hl], cn[:, :Hl]
        else:
            out = torch.empty(n, D)
            if zfilter is not None:
                self.zfilter_forward_sums(state, zfilter.running_sum, zfilter.running_sumsq, zfilter.count, zfilter.eps,
                                          out)
            else:
                out.copy_(state)
        h1, h2, mean = torch.empty(n, actor.H1), torch.empty(n, actor.H2), torch.empty(n, A)
        self.mlp3_forward(actor, out, h1, h2, mean, L.SMX_ACT_TANH)
        acts, pd = torch.empty(n, A), torch.empty(n, 2 * A)
        self.diaggauss_sample(mean, model.log_var.view(-1), noise_scale, eps_s, acts, pd)
        return acts, pd, h, c

    @staticmethod
    def env_step(state, acts):
        """SyntheticEnv._step's fp32 expressions -> (next state before any reset, reward)"""
        n, D = state.shape
        A = acts.shape[1]
        a = acts.clamp(-1.0, 1.0)
        k = torch.arange(D)
        sn = torch.tensor(0.9, dtype=torch.float32) * state + torch.tensor(0.5, dtype=torch.float32) * a[:, k % A]
        sn = (sn + torch.as_tensor(_drift(D))).clamp(-10.0, 10.0)
        q = torch.zeros(n, dtype=torch.float64)
        for j in range(A):
            v = a[:, j].double()
            q = q + v * v
        return sn, (-0.1 * q + 0.05 * sn[:, 0].double()).float()

    def synth_ppo_window_rollout(self, model, packed, lstm_packed, state, init_state, noise_scale, eps, t, episode_len,
                                 steps, n_step, advance, carry, tables, cursor, zfilter, hN=None, cN=None, h0=None,
                                 c0=None, h_before=None, c_before=None, actors_per_workgroup=0):
        assert actors_per_workgroup in (0, 4, 8, 16)
        self.window_launches += 1
        n, D = state.shape
        A = model.actor.OUT
        N, adv = int(n_step), int(advance)
        S = -(-N // adv)
        cap = tables['obs'].shape[0]
        closing, tt = 0, t
        for _ in range(steps):
            closing += (tt + 1 - N >= 0 and (tt + 1 - N) % adv == 0)
            tt = 0 if tt + 1 >= episode_len else tt + 1
        assert n * closing <= cap
        rnn = model.if_rnn
        Hp = model.rnn_hidden if rnn else 0
        Hl = model.rnn_hidden_logical if rnn else 0
        h, c = torch.zeros(n, Hp), torch.zeros(n, Hp)
        if rnn and h0 is not None:
            h[:, :Hl], c[:, :Hl] = h0.reshape(n, Hl), c0.reshape(n, Hl)
        hb = cb = None
        base = int(cursor)
        for s in range(steps):
            hb, cb = h[:, :Hl].clone(), c[:, :Hl].clone()
            acts, pd, h, c = self._act_step(model, state, h, c, noise_scale, None if eps is None else eps[s], zfilter)
            sn, rew = self.env_step(state, acts)
            done = t + 1 >= episode_len
            slot, j = t % N, t + 1 - N
            carry['obs'][:, slot] = state
            carry['actions'][:, slot] = acts
            carry['rewards'][:, slot] = rew
            carry['pds'][:, slot] = pd
            if rnn and t % adv == 0:
                carry['cells'][:, (t // adv) % S, 0] = hb
                carry['cells'][:, (t // adv) % S, 1] = cb
            if j >= 0 and j % adv == 0:
                rows = (base + torch.arange(n)) % cap
                order = [(j + u) % N for u in range(N)]
                tables['obs'][rows] = carry['obs'][:, order].reshape(n, -1)
                tables['obs_next'][rows] = sn
                tables['actions'][rows] = carry['actions'][:, order].reshape(n, -1)
                tables['rewards'][rows] = carry['rewards'][:, order]
                d = torch.zeros(n, N)
                d[:, N - 1] = 1.0 if done else 0.0
                tables['dones'][rows] = d
                tables['pds'][rows] = carry['pds'][:, order].reshape(n, -1)
                if rnn:
                    tables['cells'][rows] = carry['cells'][:, (j // adv) % S].reshape(n, -1)
                base = (base + n) % cap
            state.copy_(init_state if done else sn)
            t = 0 if done else t + 1
        if rnn:
            hN.view(n, Hl).copy_(h[:, :Hl])
            cN.view(n, Hl).copy_(c[:, :Hl])
            if h_before is not None:
                h_before.view(n, Hl).copy_(hb)
                c_before.view(n, Hl).copy_(cb)


def configs(D, A, n_step, stride, hidden=(24, 16), rnn_hidden=None, use_z=True, memory_size=4096, batch_size=None):
    """PPO configs; rnn_hidden None: a plain-MLP policy, else a one-layer LSTM stem of that many units"""
    from surreal_amd.main.ppo_configs import ppo_learner_config, ppo_env_config, ppo_session_config
    lc = ppo_learner_config()
    lc.algo.rnn.if_rnn_policy = rnn_hidden is not None
    if rnn_hidden is not None:
        lc.algo.rnn.rnn_hidden = rnn_hidden
        lc.algo.rnn.rnn_layer = 1
    lc.algo.use_z_filter = use_z
    lc.algo.n_step, lc.algo.stride = n_step, stride
    lc.replay.memory_size = memory_size
    lc.replay.batch_size = batch_size or min(64, memory_size)
    lc.replay.sampling_start_size = lc.replay.batch_size
    lc.model.actor_fc_hidden_sizes = lc.model.critic_fc_hidden_sizes = list(hidden)
    return lc, ppo_env_config(D, A), ppo_session_config(H.session_folder('surreal_amd_test_ppo_window'))


def make_agent(D, A, n_step, stride, hidden=(24, 16), rnn_hidden=None, use_z=True, deterministic=False, seed=3,
               memory_size=4096, batch_size=None):
    from surreal_amd.agent import PPOAgent
    from surreal_amd import synthetic
    lc, ec, sc = configs(D, A, n_step, stride, hidden, rnn_hidden, use_z, memory_size, batch_size)
    agent = PPOAgent(lc, ec, sc, agent_id=1, agent_mode='eval_deterministic_local' if deterministic else 'training')
    agent.model.load_params(synthetic.make_ppo_params(D, A, hidden=tuple(hidden), seed=seed, final_scale=2.0,
                                                      log_sig_spread=0.4, rnn_hidden=rnn_hidden or 0))
    if use_z:
        agent.model.z_filter.load_state_dict(synthetic.make_zfilter_state(D, seed=seed + 1))
    return agent, (lc, ec, sc)


def closing_steps(t, steps, episode_len, n_step, stride):
    """the episode clocks of the closing steps among `steps` steps from clock t, in order"""
    from surreal_amd.env.exp_sender_wrapper import window_advance
    adv, out = window_advance(n_step, stride), []
    for _ in range(steps):
        j = t + 1 - n_step
        if j >= 0 and j % adv == 0:
            out.append(t)
        t = 0 if t + 1 >= episode_len else t + 1
    return out


def closing_count(t, steps, episode_len, n_step, stride):
    """closing steps among `steps` steps from clock t (the host's count)"""
    return len(closing_steps(t, steps, episode_len, n_step, stride))


def host_windows(agent, cfg, n, D, episode_len, steps, eps_all, device='cpu'):
    """the host path over `steps` steps with the draws eps_all [steps, n, A] (None: deterministic) -> {field: np
    [windows, ...]} in the device's row order"""
    from surreal_amd.env import ExpSenderWrapperMultiStepMovingWindowWithInfo
    from surreal_amd.env.synthetic_env import SyntheticEnv
    lc, ec, sc = cfg
    A = agent.action_dim
    rnn = agent.rnn_config.if_rnn_policy
    envs = []
    for a in range(n):
        sent = []
        w = ExpSenderWrapperMultiStepMovingWindowWithInfo(SyntheticEnv(D, A, episode_len=episode_len, seed=a), lc, sc,
                                                          sink=sent.append)
        obs, _ = w.reset()
        envs.append([w, obs, sent])
    out = {k: [] for k in FIELDS + (('cells',) if rnn else ())}
    for s in range(steps):
        x = torch.as_tensor(np.stack([e[1]['low_dim']['flat_inputs'] for e in envs]), device=device)
        acts, pd = agent.act_batch(x, eps=None if eps_all is None else eps_all[s].to(device))
        acts, pd = acts.cpu().numpy(), pd.cpu().numpy()
        if rnn:
            hb, cb = (v.detach().cpu().numpy() for v in agent.batch_cells_before)
        emitted = []
        for a, e in enumerate(envs):
            w, obs, sent = e
            once = [hb[:, a].copy(), cb[:, a].copy()] if rnn else []
            obs, _, done, _ = w.step((acts[a].copy(), [once, [pd[a].copy()]]))
            if done:
                obs, _ = w.reset()
            e[1] = obs
            emitted.append(list(sent))
            del sent[:]
        counts = {len(x) for x in emitted}
        assert counts <= {0, 1} and len(counts) == 1, counts     # a shared clock: all actors or none
        for e in emitted:
            if not e:
                continue
            x = e[0]
            out['obs'].append(np.stack([o['low_dim']['flat_inputs'] for o in x['obs']]))
            out['obs_next'].append(np.asarray(x['obs_next']['low_dim']['flat_inputs']).reshape(1, D))
            out['actions'].append(np.stack(x['actions']))
            out['rewards'].append(np.asarray(x['rewards'], dtype=np.float32))
            out['dones'].append(np.asarray(x['dones'], dtype=np.float32))
            out['pds'].append(np.stack([p[0] for p in x['persistent_infos']]))
            if rnn:
                out['cells'].append(np.stack(x['onetime_infos']))         # [2, 1, Hl]
    return {k: np.stack(v) if v else np.zeros((0,)) for k, v in out.items()}


def device_windows(venv, agent, replay, chunks, eps_all, actors_per_workgroup=0, as_numpy=True):
    """ppo_rollout_into over the chunk lengths `chunks` (eps_all [sum, n, A] split along them) -> ({field: np}, rows)
    (as_numpy=False: the popped device tensors)"""
    total, s0 = 0, 0
    for T in chunks:
        eps = None if eps_all is None else eps_all[s0:s0 + T].to(venv.device)
        total += venv.ppo_rollout_into(agent, replay, T, eps=eps, actors_per_workgroup=actors_per_workgroup)
        s0 += T
    if total == 0:
        return {}, 0
    got = replay.sample_batch(total)
    if not as_numpy:
        return got, total
    return {k: v.detach().cpu().numpy() for k, v in got.items()}, total


def cut_windows(table, clock0, episode_len, n_step, stride):
    """the windows of a rollout table {field: [n, S + 1, ...]} (synth_rollout / synth_lstm_rollout from clock clock0,
    'cells' [n, S + 1, 2, 1, Hl]) -> {field: [windows, ...]} in the device's row order, and the closing steps that were
    terminal (their obs_next is the table's reset state, not the terminal observation)"""
    from surreal_amd.env.exp_sender_wrapper import window_advance
    adv = window_advance(n_step, stride)
    S = table['obs'].shape[1] - 1
    out = {k: [] for k in table}
    terminal = []
    t = clock0
    for s in range(S):
        j = t + 1 - n_step
        if j >= 0 and j % adv == 0:
            lo = s - n_step + 1
            for k in table:
                if k == 'cells':
                    out[k].append(table[k][:, lo])
                elif k == 'obs_next':
                    continue
                else:
                    out[k].append(table[k][:, lo:s + 1])
            out.setdefault('obs_next', []).append(table['obs'][:, s + 1:s + 2])
            terminal.append(t + 1 >= episode_len)
        t = 0 if t + 1 >= episode_len else t + 1
    res = {}
    for k, v in out.items():
        if v:
            x = torch.stack(v)                  # [windows per actor, n, ...]: closing step major, actor minor
            res[k] = x.reshape((-1,) + tuple(x.shape[2:]))
    return res, terminal
