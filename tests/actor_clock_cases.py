"""
Episode clocks per actor in the one-launch rollouts (SyntheticVecEnv(..., episode_len=<sequence>); env/actor_clocks.py),
shared by the CPU tier (test_actor_clocks_cpu.py) and the GPU tier (test_gpu_actor_clocks.py):

  * ``ClockPpoWindowCpuKernels`` / ``ClockDdpgRolloutCpuKernels`` -- the torch-CPU doubles of the windowed PPO and the
    DDPG rollout with the ``clocks`` keyword and ``actor_clock_rows``: the parents' per-step ops for all actors, then
    every actor's record rule on its own clock, its closing records at (cursor + row_off[s, a]) % capacity;
  * ``host_windows`` / ``host_transitions`` -- n ``SyntheticEnv(D, A, episode_len=L[a], seed=a)`` behind the reference's
    experience wrappers, stepped in actor order (``ppo_window_cases.host_windows`` / ``ddpg_rollout_cases.host_ring``
    without their shared-clock assertion): the records in the order they are sent, and which (step, actor) sent each;
  * ``records_of`` -- the (step, actor) pairs of ``row_table`` in row order, and ``per_actor``: an actor's records out of
    a run's rows, in order.
"""
import numpy as np
import torch

import ddpg_rollout_cases as DC
import ppo_window_cases as PW
from surreal_amd import _lib as L
from surreal_amd.env import actor_clocks as AC

# the base shape of both tiers: one full 4-actor block and a ragged one; calls of (7, 1, 12) steps
N_ACTORS, D, A, HIDDEN = 6, 7, 3, (24, 16)
LENS = (5, 9, 4, 13, 3, 6)
CHUNKS = (7, 1, 12)
PPO_WINDOW = (4, 3)                # n_step, stride: 22 windows, actor 4 none, actor 2 only on its terminal step
DDPG_N_STEP = 3                    # 70 transitions


def _fill_table(t, episode_len, steps, n_step, advance, row_off):
    table, _ = AC.row_table(t.cpu().numpy(), episode_len.cpu().numpy(), steps, n_step, advance)
    row_off.copy_(torch.from_numpy(table))


class ClockPpoWindowCpuKernels(PW.PpoWindowCpuKernels):
    name = 'torch-cpu-double+ppo-window+actor-clocks'

    def actor_clock_rows(self, t, episode_len, steps, n_step, advance, row_off, t_host=None, episode_len_host=None):
        _fill_table(t, episode_len, steps, n_step, advance, row_off)

    def synth_ppo_window_rollout(self, model, packed, lstm_packed, state, init_state, noise_scale, eps, t, episode_len,
                                 steps, n_step, advance, carry, tables, cursor, zfilter, hN=None, cN=None, h0=None,
                                 c0=None, h_before=None, c_before=None, actors_per_workgroup=0, clocks=None):
        if clocks is None:
            return super().synth_ppo_window_rollout(model, packed, lstm_packed, state, init_state, noise_scale, eps, t,
                                                    episode_len, steps, n_step, advance, carry, tables, cursor, zfilter,
                                                    hN, cN, h0, c0, h_before, c_before, actors_per_workgroup)
        assert actors_per_workgroup in (0, 4, 8, 16)
        self.window_launches += 1
        n = state.shape[0]
        N, adv = int(n_step), int(advance)
        S = -(-N // adv)
        cap = tables['obs'].shape[0]
        tau, lens = clocks['t'].numpy().astype(np.int64), clocks['episode_len'].numpy()
        table, rows = clocks['row_off'].numpy(), int(clocks['rows'])
        assert 0 <= rows <= cap and table.shape == (steps, n)
        rnn = model.if_rnn
        Hp = model.rnn_hidden if rnn else 0
        Hl = model.rnn_hidden_logical if rnn else 0
        h, c = torch.zeros(n, Hp), torch.zeros(n, Hp)
        if rnn and h0 is not None:
            h[:, :Hl], c[:, :Hl] = h0.reshape(n, Hl), c0.reshape(n, Hl)
        hb = cb = None
        for s in range(steps):
            hb, cb = h[:, :Hl].clone(), c[:, :Hl].clone()
            acts, pd, h, c = self._act_step(model, state, h, c, noise_scale, None if eps is None else eps[s], zfilter)
            sn, rew = self.env_step(state, acts)
            for a in range(n):
                ta = int(tau[a])
                done = ta + 1 >= lens[a]
                slot, j = ta % N, ta + 1 - N
                carry['obs'][a, slot] = state[a]
                carry['actions'][a, slot] = acts[a]
                carry['rewards'][a, slot] = rew[a]
                carry['pds'][a, slot] = pd[a]
                if rnn and ta % adv == 0:
                    carry['cells'][a, (ta // adv) % S, 0] = hb[a]
                    carry['cells'][a, (ta // adv) % S, 1] = cb[a]
                off = int(table[s, a])
                if j >= 0 and j % adv == 0 and 0 <= off < rows:
                    row = (int(cursor) + off) % cap
                    order = [(j + u) % N for u in range(N)]
                    tables['obs'][row] = carry['obs'][a, order].reshape(-1)
                    tables['obs_next'][row] = sn[a]
                    tables['actions'][row] = carry['actions'][a, order].reshape(-1)
                    tables['rewards'][row] = carry['rewards'][a, order]
                    d = torch.zeros(N)
                    d[N - 1] = 1.0 if done else 0.0
                    tables['dones'][row] = d
                    tables['pds'][row] = carry['pds'][a, order].reshape(-1)
                    if rnn:
                        tables['cells'][row] = carry['cells'][a, (j // adv) % S].reshape(-1)
                state[a] = init_state[a] if done else sn[a]
                tau[a] = 0 if done else ta + 1
        if rnn:
            hN.view(n, Hl).copy_(h[:, :Hl])
            cN.view(n, Hl).copy_(c[:, :Hl])
            if h_before is not None:
                h_before.view(n, Hl).copy_(hb)
                c_before.view(n, Hl).copy_(cb)


class ClockDdpgRolloutCpuKernels(DC.DdpgRolloutCpuKernels):
    name = 'torch-cpu-double+ddpg-rollout+actor-clocks'

    def actor_clock_rows(self, t, episode_len, steps, n_step, advance, row_off, t_host=None, episode_len_host=None):
        _fill_table(t, episode_len, steps, n_step, advance, row_off)

    def synth_ddpg_rollout(self, net, packed, r, steps, actors_per_workgroup=0, clocks=None):
        if clocks is None:
            return super().synth_ddpg_rollout(net, packed, r, steps, actors_per_workgroup)
        assert actors_per_workgroup in (0, 4, 8, 16)
        state, init = r['state'], r['init_state']
        n, Dd = state.shape
        N = int(r['n_step'])
        tabs = r['tables']
        cap = tabs['obs'].shape[0]
        tau, lens = clocks['t'].numpy().astype(np.int64), clocks['episode_len'].numpy()
        table, rows = clocks['row_off'].numpy(), int(clocks['rows'])
        assert 0 <= rows <= cap and table.shape == (steps, n)
        W = self._packed_views(packed, net)
        noise = r['noise_type']
        k = torch.arange(Dd)
        for s in range(steps):
            mu = self._mu_rows(net, W, net.views, state)
            a = mu.clamp(-1.0, 1.0)
            Aa = a.shape[1]
            if noise == L.SMX_DDPG_NOISE_GAUSSIAN:
                a = (a.double() + (0.0 + r['sigmas'].view(-1, 1) * r['eps'][s].double())).float()
            elif noise == L.SMX_DDPG_NOISE_OU:
                x = r['ou']
                x[torch.from_numpy(tau == 0)] = 0.0
                x.copy_((x + (r['theta'] * (0.0 - x)) * r['dt'])
                        + (r['sigmas'] * r['root_dt']).view(-1, 1) * r['eps'][s].double())
                a = (a.double() + x).float()
            a = a.clamp(-1.0, 1.0)
            sn = (torch.tensor(0.9, dtype=torch.float32) * state + torch.tensor(0.5, dtype=torch.float32) * a[:, k % Aa])
            sn = (sn + torch.as_tensor(DC._drift(Dd))).clamp(-10.0, 10.0)
            q = torch.zeros(n, dtype=torch.float64)
            for j in range(Aa):
                v = a[:, j].double()
                q = q + v * v
            rew = (-0.1 * q + 0.05 * sn[:, 0].double()).float()
            for i in range(n):
                ti = int(tau[i])
                done = ti + 1 >= lens[i]
                slot, jslot = ti % N, (ti + 1) % N
                r['carry_obs'][i, slot] = state[i]
                r['carry_act'][i, slot] = a[i]
                r['carry_rew'][i, slot] = rew[i]
                off = int(table[s, i])
                if ti >= N - 1 and 0 <= off < rows:
                    row = (int(r['cursor']) + off) % cap
                    j = ti - N + 1
                    R = r['carry_rew'][i, j % N].double()
                    for u in range(j + 1, ti + 1):
                        e = (u - j) if u >= N - 1 else (N - 1 - j)
                        R = R + r['gpow'][e] * r['carry_rew'][i, u % N].double()
                    tabs['obs'][row] = r['carry_obs'][i, jslot]
                    tabs['actions'][row] = r['carry_act'][i, jslot]
                    tabs['obs_next'][row] = sn[i]
                    tabs['rewards'][row] = R.float()
                    tabs['dones'][row] = 1.0 if done else 0.0
                state[i] = init[i] if done else sn[i]
                tau[i] = 0 if done else ti + 1


def records_of(lens, steps, n_step, advance, t0=None):
    """-> the (step, actor) pairs that close a record, in row order (row_table's numbering)"""
    table, rows = AC.row_table(np.zeros(len(lens), np.int64) if t0 is None else t0, lens, steps, n_step, advance)
    pairs = [None] * rows
    for s, a in zip(*np.nonzero(table >= 0)):
        pairs[table[s, a]] = (int(s), int(a))
    assert None not in pairs
    return pairs


def per_actor(fields, pairs, a):
    """actor a's records out of {field: [rows, ...]} whose row i belongs to pairs[i], in order"""
    idx = [i for i, (_, b) in enumerate(pairs) if b == a]
    return {k: v[idx] for k, v in fields.items()}


def shared_pairs(n, episode_len, steps, n_step, advance):
    """the same for a shared clock: closing step major, actor minor"""
    return records_of([episode_len] * n, steps, n_step, advance)


def host_windows(agent, cfg, n, obs_dim, lens, steps, eps_all, device='cpu'):
    """ppo_window_cases.host_windows with an episode length per actor -> ({field: np [windows, ...]} in the order the
    wrappers sent them, [(step, actor)] of each)"""
    from surreal_amd.env import ExpSenderWrapperMultiStepMovingWindowWithInfo
    from surreal_amd.env.synthetic_env import SyntheticEnv
    lc, ec, sc = cfg
    act_dim = agent.action_dim
    rnn = agent.rnn_config.if_rnn_policy
    envs = []
    for a in range(n):
        sent = []
        w = ExpSenderWrapperMultiStepMovingWindowWithInfo(
            SyntheticEnv(obs_dim, act_dim, episode_len=int(lens[a]), seed=a), lc, sc, sink=sent.append)
        obs, _ = w.reset()
        envs.append([w, obs, sent])
    out = {k: [] for k in PW.FIELDS + (('cells',) if rnn else ())}
    pairs = []
    for s in range(steps):
        x = torch.as_tensor(np.stack([e[1]['low_dim']['flat_inputs'] for e in envs]), device=device)
        acts, pd = agent.act_batch(x, eps=None if eps_all is None else eps_all[s].to(device))
        acts, pd = acts.cpu().numpy(), pd.cpu().numpy()
        if rnn:
            hb, cb = (v.detach().cpu().numpy() for v in agent.batch_cells_before)
        for a, e in enumerate(envs):
            w, obs, sent = e
            once = [hb[:, a].copy(), cb[:, a].copy()] if rnn else []
            obs, _, done, _ = w.step((acts[a].copy(), [once, [pd[a].copy()]]))
            if done:
                obs, _ = w.reset()
            e[1] = obs
            assert len(sent) <= 1
            for x_ in sent:
                pairs.append((s, a))
                out['obs'].append(np.stack([o['low_dim']['flat_inputs'] for o in x_['obs']]))
                out['obs_next'].append(np.asarray(x_['obs_next']['low_dim']['flat_inputs']).reshape(1, obs_dim))
                out['actions'].append(np.stack(x_['actions']))
                out['rewards'].append(np.asarray(x_['rewards'], dtype=np.float32))
                out['dones'].append(np.asarray(x_['dones'], dtype=np.float32))
                out['pds'].append(np.stack([p[0] for p in x_['persistent_infos']]))
                if rnn:
                    out['cells'].append(np.stack(x_['onetime_infos']))         # [2, 1, Hl]
            del sent[:]
    return {k: np.stack(v) if v else np.zeros((0,)) for k, v in out.items()}, pairs


def host_transitions(agent, lc, ec, sc, n, lens, eps_all):
    """ddpg_rollout_cases.host_ring with an episode length per actor, over all steps of eps_all [steps, n, A] (numpy)
    -> ({field: np [transitions, width]} in the order the wrappers sent them, [(step, actor)] of each)"""
    from surreal_amd.agent import DDPGAgent
    from surreal_amd.env import ExpSenderWrapperSSARNStepBootstrap
    from surreal_amd.env.synthetic_env import SyntheticEnv
    obs_dim, act_dim = agent.model.input_dim, agent.action_dim
    actors = []
    for a in range(n):
        ag = DDPGAgent(lc, ec, sc, agent_id=a, agent_mode=agent.agent_mode)
        ag.model.load_state_dict(agent.model.state_dict())
        sent = []
        w = ExpSenderWrapperSSARNStepBootstrap(SyntheticEnv(obs_dim, act_dim, episode_len=int(lens[a]), seed=a), lc, sc,
                                               sink=sent.append)
        if ag.noise is not None:
            clock = {'t': 0}
            ag.noise._eps = (lambda a_=a, c=clock: np.asarray(eps_all[c['t'], a_], dtype=np.float64))
            ag._clock = clock
        ag.pre_episode()
        obs, _ = w.reset()
        actors.append([ag, w, obs, sent])
    out = {k: [] for k in DC.FIELDS}
    pairs = []
    for s in range(eps_all.shape[0]):
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
            assert len(sent) <= 1
            for e in sent:
                pairs.append((s, a))
                out['obs'].append(np.asarray(e['obs'][0]['low_dim']['flat_inputs'], dtype=np.float32))
                out['obs_next'].append(np.asarray(e['obs'][1]['low_dim']['flat_inputs'], dtype=np.float32))
                out['actions'].append(np.asarray(e['action'], dtype=np.float32))
                out['rewards'].append(np.asarray([e['reward']], dtype=np.float32))
                out['dones'].append(np.asarray([float(e['done'])], dtype=np.float32))
            del sent[:]
    return {k: np.stack(v) for k, v in out.items()}, pairs


def device_transitions(venv, agent, replay, chunks, eps_all, **kw):
    """ddpg_rollout_into over the chunk lengths `chunks` (eps_all [sum, n, A] torch or None, split along them) -> rows"""
    total, s0 = 0, 0
    for T in chunks:
        eps = None if eps_all is None else eps_all[s0:s0 + T].to(venv.device)
        total += venv.ddpg_rollout_into(agent, replay, T, eps=eps, **kw)
        s0 += T
    return total
