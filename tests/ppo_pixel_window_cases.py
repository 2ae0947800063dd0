"""
SyntheticVecEnv.ppo_rollout_into with a camera (perception -> [LSTM step ->] actor -> smx_synth_ppo_pixel_window_step per
step) against the host path it replaces, shared by the CPU tier (test_ppo_pixel_window_rollout_cpu.py) and the GPU tier
(test_gpu_ppo_pixel_window_rollout.py):

  * ``PpoPixelWindowCpuKernels`` -- the torch-CPU double of the new entry point (a subclass of the windowed rollout's
    double): the head is the double's diaggauss_sample, the step SyntheticEnv's fp32 expressions, the rings, the rows
    and the frames follow the header's index arithmetic;
  * ``host_windows`` -- n ``SyntheticEnv(pixel)`` under ``FrameStackWrapper`` under
    ``ExpSenderWrapperMultiStepMovingWindowWithInfo``, driven step by step by ``act_batch`` on the stacked observation
    dict with injected eps (reset on done, the LSTM state never reset), the windows in the device's row order;
  * ``frames_from_record`` -- the pixel / pixel_next a ring should hold, rendered by SyntheticEnv._frame from the
    low-dimensional states the same ring recorded.
"""
import collections

import numpy as np
import torch

import ppo_window_cases as PW
from ddpg_pixel_rollout_cases import render
from surreal_amd.env import stack_sources

FIELDS = PW.FIELDS + ('pixel', 'pixel_next')


class PpoPixelWindowCpuKernels(PW.PpoWindowCpuKernels):
    name = 'torch-cpu-double+ppo-pixel-window'

    def __init__(self):
        super().__init__()
        self.pixel_steps = 0

    @staticmethod
    def synth_ppo_pixel_window_step_supported(A):
        return 0 < A <= 64

    def synth_ppo_pixel_window_step(self, r, mu, copy_workgroups=0):
        """smx_synth_ppo_pixel_window_step by the header's index arithmetic"""
        self.pixel_steps += 1
        hist, obs_pix, tabs, carry, state = r['hist'], r['obs_pixel'], r['tables'], r['carry'], r['state']
        n, Hd, C, H, W = hist.shape
        S = obs_pix.shape[1] // C
        A = mu.shape[1]
        tau, N, adv, L_, pos = int(r['t']), int(r['n_step']), int(r['advance']), int(r['episode_len']), int(r['hist_pos'])
        Sc = -(-N // adv)
        cap = tabs['obs'].shape[0]
        assert Hd >= N + S and 0 <= pos < Hd and 0 < adv <= N and 0 <= tau < L_ and n <= cap
        # head, step
        acts, pd = torch.empty(n, A), torch.empty(n, 2 * A)
        self.diaggauss_sample(mu, r['log_var'], r.get('noise_scale'), r.get('eps'), acts, pd)
        sn, rew = self.env_step(state, acts)
        done = tau + 1 >= L_
        # carry rings
        slot, j = tau % N, tau + 1 - N
        carry['obs'][:, slot] = state
        carry['actions'][:, slot] = acts
        carry['rewards'][:, slot] = rew
        carry['pds'][:, slot] = pd
        if 'cells' in carry and r.get('h_before') is not None and tau % adv == 0:
            carry['cells'][:, (tau // adv) % Sc, 0] = r['h_before'].reshape(n, -1)
            carry['cells'][:, (tau // adv) % Sc, 1] = r['c_before'].reshape(n, -1)
        # frames
        new = torch.empty(n, C, H, W, dtype=torch.uint8)
        self.synth_frames(sn[:, 0], tau + 1, new)

        def frame(u):
            return new if u == tau + 1 else hist[:, (pos - tau + u) % Hd]

        def stacked(top):
            return torch.cat([frame(max(top - S + 1 + i, 0)) for i in range(S)], dim=1)
        nxt = stacked(tau + 1)
        if j >= 0 and j % adv == 0:
            rows = (int(r['cursor']) + torch.arange(n)) % cap
            order = [(j + u) % N for u in range(N)]
            tabs['obs'][rows] = carry['obs'][:, order].reshape(n, -1)
            tabs['obs_next'][rows] = sn
            tabs['actions'][rows] = carry['actions'][:, order].reshape(n, -1)
            tabs['rewards'][rows] = carry['rewards'][:, order]
            d = torch.zeros(n, N)
            d[:, N - 1] = 1.0 if done else 0.0
            tabs['dones'][rows] = d
            tabs['pds'][rows] = carry['pds'][:, order].reshape(n, -1)
            if 'cells' in carry and tabs.get('cells') is not None:
                tabs['cells'][rows] = carry['cells'][:, (j // adv) % Sc].reshape(n, -1)
            tabs['pixel'][rows] = torch.stack([stacked(j + u) for u in range(N)], dim=1).reshape(n, -1)
            tabs['pixel_next'][rows] = nxt.reshape(n, -1)
        if done:
            f0 = torch.empty(n, C, H, W, dtype=torch.uint8)
            self.synth_frames(r['init_state'][:, 0], 0, f0)
            hist[:, (pos + 1) % Hd] = f0
            obs_pix.copy_(f0.repeat(1, S, 1, 1))
        else:
            hist[:, (pos + 1) % Hd] = new
            obs_pix.copy_(nxt)
        state.copy_(r['init_state'] if done else sn)


def configs(D, A, n_step, stride, pixel, stacks, hidden=(24, 16), rnn_hidden=None, use_z=True, feat=12, memory_size=4096,
            batch_size=None):
    """PW.configs with camera0 = the stacked frame (stacks * C, H, W) and a small CNN stem"""
    from surreal_amd.main.ppo_configs import ppo_env_config
    lc, _, sc = PW.configs(D, A, n_step, stride, hidden, rnn_hidden, use_z, memory_size, batch_size)
    C, H, W = pixel
    lc.model.cnn_feature_dim = feat
    ec = ppo_env_config(D, A, pixel=(stacks * C, H, W))
    ec.frame_stacks = stacks
    return lc, ec, sc


def make_agent(D, A, n_step, stride, pixel, stacks, hidden=(24, 16), rnn_hidden=None, use_z=True, deterministic=False,
               seed=3, feat=12, memory_size=4096, batch_size=None, final_scale=2.0):
    from surreal_amd.agent import PPOAgent
    from surreal_amd import synthetic
    cfg = configs(D, A, n_step, stride, pixel, stacks, hidden, rnn_hidden, use_z, feat, memory_size, batch_size)
    agent = PPOAgent(*cfg, agent_id=1, agent_mode='eval_deterministic_local' if deterministic else 'training')
    C, H, W = pixel
    agent.model.load_params(synthetic.make_ppo_params(D, A, hidden=tuple(hidden), seed=seed, final_scale=final_scale,
                                                      log_sig_spread=0.4, rnn_hidden=rnn_hidden or 0,
                                                      pixel=(stacks * C, H, W), cnn_feature_dim=feat))
    if use_z:
        agent.model.z_filter.load_state_dict(synthetic.make_zfilter_state(D, seed=seed + 1))
    return agent, cfg


def make_venv(n, D, A, episode_len, pixel, stacks, device=None, kernels=None):
    from surreal_amd.env import SyntheticVecEnv
    return SyntheticVecEnv(n, D, A, episode_len=episode_len, seeds=list(range(n)), device=device, kernels=kernels,
                           pixel=pixel, frame_stacks=stacks)


def host_windows(agent, cfg, n, D, episode_len, steps, eps_all, pixel, stacks, device='cpu'):
    """the host path over `steps` steps with the draws eps_all [steps, n, A] (None: deterministic) -> {field: np
    [windows, ...]} in the device's row order"""
    from surreal_amd.env import ExpSenderWrapperMultiStepMovingWindowWithInfo, FrameStackWrapper
    from surreal_amd.env.synthetic_env import SyntheticEnv
    from surreal_amd.session import Config
    lc, ec, sc = cfg
    A = agent.action_dim
    rnn = agent.rnn_config.if_rnn_policy
    envs = []
    for a in range(n):
        sent = []
        env = FrameStackWrapper(SyntheticEnv(D, A, episode_len=episode_len, seed=a, pixel=pixel),
                                Config(frame_stacks=stacks, frame_stack_concatenate_on_env=True))
        w = ExpSenderWrapperMultiStepMovingWindowWithInfo(env, lc, sc, sink=sent.append)
        obs, _ = w.reset()
        envs.append([w, obs, sent])
    out = {k: [] for k in FIELDS + (('cells',) if rnn else ())}
    for s in range(steps):
        low = torch.as_tensor(np.stack([e[1]['low_dim']['flat_inputs'] for e in envs]), device=device)
        pix = torch.as_tensor(np.stack([np.asarray(e[1]['pixel']['camera0']) for e in envs]), device=device)
        obs_b = collections.OrderedDict(pixel=collections.OrderedDict(camera0=pix),
                                        low_dim=collections.OrderedDict(flat_inputs=low))
        acts, pd = agent.act_batch(obs_b, eps=None if eps_all is None else eps_all[s].to(device))
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
            out['pixel'].append(np.stack([np.asarray(o['pixel']['camera0']) for o in x['obs']]))
            out['pixel_next'].append(np.asarray(x['obs_next']['pixel']['camera0'])[None])
            out['actions'].append(np.stack(x['actions']))
            out['rewards'].append(np.asarray(x['rewards'], dtype=np.float32))
            out['dones'].append(np.asarray(x['dones'], dtype=np.float32))
            out['pds'].append(np.stack([p[0] for p in x['persistent_infos']]))
            if rnn:
                out['cells'].append(np.stack(x['onetime_infos']))         # [2, 1, Hl]
    return {k: np.stack(v) if v else np.zeros((0,)) for k, v in out.items()}


def frames_from_record(ring, rows_by_step, n, n_step, stacks, pixel):
    """The pixel [n_step, S*C, H, W] / pixel_next [1, S*C, H, W] rows the device should hold, from the low-dimensional
    states it recorded next to them.  rows_by_step: [(episode clock tau of the closing step, first ring row of its n
    actors)], in order, for a rollout that began at an episode start and whose rows did not wrap.  The state of step u
    of an episode is obs[u - j] of a window j .. j + n_step - 1 that holds it, or obs_next of the window that closed at
    u - 1; every step up to the last closing one has one because advance <= n_step."""
    states = {}                                        # (episode index, step) -> [n, D]
    eps_of = []
    ep, prev = 0, None
    for tau, r0 in rows_by_step:
        if prev is not None and tau <= prev:
            ep += 1
        prev = tau
        eps_of.append(ep)
        rows = np.arange(r0, r0 + n)
        obs = ring['obs'][rows].reshape(n, n_step, -1)
        for u in range(n_step):
            states[(ep, tau + 1 - n_step + u)] = obs[:, u]
        states[(ep, tau + 1)] = ring['obs_next'][rows].reshape(n, -1)
    want_pix, want_next = {}, {}
    for (tau, r0), ep in zip(rows_by_step, eps_of):
        j = tau + 1 - n_step
        for a in range(n):
            def stacked(top):
                return np.concatenate([render(pixel, u, float(states[(ep, u)][a, 0]))
                                       for u in stack_sources(top, stacks)], axis=0)
            want_pix[r0 + a] = np.stack([stacked(j + u) for u in range(n_step)])
            want_next[r0 + a] = stacked(tau + 1)[None]
    return want_pix, want_next
