"""
SyntheticVecEnv.ddpg_rollout_into with a camera (smx_synth_ddpg_pixel_step) against the host path it replaces, shared
by the CPU tier (test_ddpg_pixel_rollout_cpu.py) and the GPU tier (test_gpu_ddpg_pixel_rollout.py):

  * ``DdpgPixelRolloutCpuKernels`` -- the torch-CPU double of the new entry point (a subclass of the DDPG rollout
    double): the low-dimensional step is the double's synth_ddpg_step (the kernel's fp64 order), the frames follow the
    header's index arithmetic.  Its dense products (CNN stem, actor) run row by row, so that a batch-n perception gives
    the bits of the batch-1 one DDPGAgent.act runs and the CPU tier can compare bit for bit;
  * ``host_ring`` -- n ``SyntheticEnv(pixel)`` + ``FrameStackWrapper`` + ``DDPGAgent.act`` +
    ``ExpSenderWrapperSSARNStepBootstrap`` driven step by step, the transitions placed where the device writes them;
  * ``frames_from_record`` -- the pixel fields the device should hold, rebuilt from the low-dimensional states the
    ring recorded (SyntheticEnv._frame's rule, stacked by stack_sources).
"""
import numpy as np
import torch

import ddpg_rollout_cases as DC
from surreal_amd.env import stack_sources
from surreal_amd.env.synthetic_env import _drift

FIELDS = DC.FIELDS + ('pixel', 'pixel_next')


def _rows_linear(x, W, b):
    """F.linear one row at a time: the bits of a row do not depend on how many rows share the call"""
    F = torch.nn.functional
    return torch.cat([F.linear(x[i:i + 1], W, b) for i in range(x.shape[0])]) if x.shape[0] else F.linear(x, W, b)


class DdpgPixelRolloutCpuKernels(DC.DdpgRolloutCpuKernels):
    name = 'torch-cpu-double+ddpg-pixel-rollout'

    # ---- row-independent dense products ------------------------------------------------------------------------
    def linear(self, A, a_kc, B, b_kc, bias, C, M, N, K, act=0, relu_mask=None, lda=None, ldb=None,
               ldc=None, stop=None):
        if stop is not None and int(stop[0]) != 0:
            return
        lda = lda if lda is not None else A.stride(0)
        ldb = ldb if ldb is not None else B.stride(0)
        ldc = ldc if ldc is not None else C.stride(0)
        a = torch.as_strided(A, (M, K), (lda, 1) if a_kc else (1, lda)).contiguous()
        b = torch.as_strided(B, (N, K), (ldb, 1) if b_kc else (1, ldb)).contiguous()
        out = _rows_linear(a, b, None if bias is None else bias[:N])
        out = self._act(out, act)
        if relu_mask is not None:
            out = out * (torch.as_strided(relu_mask, (M, N), (ldc, 1)) > 0)
        torch.as_strided(C, (M, N), (ldc, 1)).copy_(out)

    def mlp3_forward(self, net, x, h1, h2, out, act, stop=None, pack=None):
        if stop is not None and int(stop[0]) != 0:
            return
        v = net.views
        h1.copy_(torch.relu(_rows_linear(x, v['W1'], v['b1'])))
        h2.copy_(torch.relu(_rows_linear(h1, v['W2'], v['b2'])))
        out.copy_(self._act(_rows_linear(h2, v['W3'], v['b3']), act))

    def conv_u8_forward(self, frames, F, C, Hin, Win, k, stride, W, bias, cout, y, stop=None):
        if stop is not None and int(stop[0]) != 0:
            return
        Ho, Wo = (Hin - k) // stride + 1, (Win - k) // stride + 1
        cols = torch.empty(F * Ho * Wo, C * k * k)
        self.im2col(frames, F, C, Hin, Win, k, stride, cols, scale_div=255.0)
        y[:F * Ho * Wo].copy_(torch.relu(_rows_linear(cols, W.reshape(cout, -1), bias)))

    def conv_cl_forward(self, src, F, C, Hin, Win, k, stride, W, bias, cout, y, stop=None):
        if stop is not None and int(stop[0]) != 0:
            return
        Ho, Wo = (Hin - k) // stride + 1, (Win - k) // stride + 1
        cols = torch.empty(F * Ho * Wo, C * k * k)
        self.im2col(src, F, C, Hin, Win, k, stride, cols, channel_last=True)
        y[:F * Ho * Wo].copy_(torch.relu(_rows_linear(cols, W.reshape(cout, -1), bias)))

    # ---- the new entry point -----------------------------------------------------------------------------------
    def synth_ddpg_pixel_step(self, r, mu):
        """smx_synth_ddpg_pixel_step: synth_ddpg_step, then the frames by the header's index arithmetic"""
        hist, obs_pix, tabs = r['hist'], r['obs_pixel'], r['tables']
        n, Hd, C, H, W = hist.shape
        S = obs_pix.shape[1] // C
        tau, N, L_, pos = int(r['t']), int(r['n_step']), int(r['episode_len']), int(r['hist_pos'])
        assert Hd >= N + S and 0 <= pos < Hd
        s0 = r['state'][:, 0].clone()
        self.synth_ddpg_step(r, mu)
        # element 0 of the next state before the reset, by synth_ddpg_step's expression, from the action it recorded
        a0 = r['carry_act'][:, tau % N, 0]
        sn0 = (torch.tensor(0.9, dtype=torch.float32) * s0 + torch.tensor(0.5, dtype=torch.float32) * a0)
        sn0 = (sn0 + torch.as_tensor(_drift(1))).clamp(-10.0, 10.0)
        new = torch.empty(n, C, H, W, dtype=torch.uint8)
        self.synth_frames(sn0, tau + 1, new)

        def frame(u):
            return new if u == tau + 1 else hist[:, (pos - tau + u) % Hd]

        def stacked(top):
            return torch.cat([frame(max(top - S + 1 + i, 0)) for i in range(S)], dim=1)
        nxt = stacked(tau + 1)
        if tau >= N - 1:
            cap = tabs['obs'].shape[0]
            rows = (int(r['cursor']) + torch.arange(n)) % cap
            tabs['pixel'][rows] = stacked(tau - N + 1).reshape(n, -1)
            tabs['pixel_next'][rows] = nxt.reshape(n, -1)
        if tau + 1 >= L_:
            f0 = torch.empty(n, C, H, W, dtype=torch.uint8)
            self.synth_frames(r['init_state'][:, 0], 0, f0)
            hist[:, (pos + 1) % Hd] = f0
            obs_pix.copy_(f0.repeat(1, S, 1, 1))
        else:
            hist[:, (pos + 1) % Hd] = new
            obs_pix.copy_(nxt)


def configs(D, A, n, pixel, stacks, hidden=(24, 16), feat=12, **kw):
    """DC.configs with camera0 = the stacked frame (stacks * C, H, W) and a small CNN stem"""
    from surreal_amd.main.ddpg_configs import ddpg_env_config
    lc, _, sc = DC.configs(D, A, n, hidden=hidden, **kw)
    C, H, W = pixel
    lc.model.conv_spec.hidden_output_dim = feat
    ec = ddpg_env_config(D, A, num_agents=n, pixel=(stacks * C, H, W))
    ec.frame_stacks = stacks
    return lc, ec, sc


def host_ring(agent, lc, ec, sc, n, episode_len, eps_all, capacity, pixel, stacks):
    """the host path over all steps of eps_all [steps, n, A] (numpy) -> (ring {field: [capacity, width]}, rows written)"""
    from surreal_amd.agent import DDPGAgent
    from surreal_amd.env import ExpSenderWrapperSSARNStepBootstrap, FrameStackWrapper
    from surreal_amd.env.synthetic_env import SyntheticEnv
    from surreal_amd.session import Config
    D, A = agent.model.low_dim, agent.action_dim
    Fs = stacks * int(np.prod(pixel))
    steps = eps_all.shape[0]
    actors = []
    for a in range(n):
        ag = DDPGAgent(lc, ec, sc, agent_id=a, agent_mode=agent.agent_mode)
        ag.model.load_state_dict(agent.model.state_dict())
        sent = []
        env = FrameStackWrapper(SyntheticEnv(D, A, episode_len=episode_len, seed=a, pixel=pixel),
                                Config(frame_stacks=stacks, frame_stack_concatenate_on_env=True))
        w = ExpSenderWrapperSSARNStepBootstrap(env, lc, sc, sink=sent.append)
        if ag.noise is not None:
            clock = {'t': 0}
            ag.noise._eps = (lambda a_=a, c=clock: np.asarray(eps_all[c['t'], a_], dtype=np.float64))
            ag._clock = clock
        ag.pre_episode()
        obs, _ = w.reset()
        actors.append([ag, w, obs, sent])
    ring = {'obs': np.zeros((capacity, D), np.float32), 'obs_next': np.zeros((capacity, D), np.float32),
            'actions': np.zeros((capacity, A), np.float32), 'rewards': np.zeros((capacity, 1), np.float32),
            'dones': np.zeros((capacity, 1), np.float32), 'pixel': np.zeros((capacity, Fs), np.uint8),
            'pixel_next': np.zeros((capacity, Fs), np.uint8)}
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
                ring['pixel'][row] = np.asarray(e['obs'][0]['pixel']['camera0']).reshape(-1)
                ring['pixel_next'][row] = np.asarray(e['obs'][1]['pixel']['camera0']).reshape(-1)
                ring['actions'][row] = e['action']
                ring['rewards'][row] = np.float32(e['reward'])
                ring['dones'][row] = float(e['done'])
            cursor = (cursor + n) % capacity
            total += n
    return ring, total


def render(pixel, t, s0):
    """SyntheticEnv._frame for step count t and first state component s0"""
    from surreal_amd.env.synthetic_env import SyntheticEnv
    env = SyntheticEnv(1, 1, pixel=pixel)
    env.t, env.state = t, np.asarray([s0], np.float32)
    return env._frame()


def frames_from_record(ring, rows_by_step, n, n_step, stacks, pixel, episode_len, t0=0):
    """The pixel / pixel_next rows the device should hold, from the low-dimensional states it recorded.
    rows_by_step: [(episode step tau of the closing step, first ring row of its n actors)], in order, for a rollout
    that began at an episode start.  The state of step u of an episode is obs of the transition opened at u (closed at
    u + n_step - 1) or obs_next of the one closed at u - 1; with episode_len >= 2 n_step - 1 every step has one."""
    states = {}                                        # (episode index, step) -> [n, D]
    ep, prev = 0, None
    for tau, r0 in rows_by_step:
        if prev is not None and tau <= prev:
            ep += 1
        prev = tau
        rows = np.arange(r0, r0 + n)
        states[(ep, tau - n_step + 1)] = ring['obs'][rows]
        states[(ep, tau + 1)] = ring['obs_next'][rows]
    want_pix, want_next = {}, {}
    ep, prev = 0, None
    for tau, r0 in rows_by_step:
        if prev is not None and tau <= prev:
            ep += 1
        prev = tau
        for key, top, dst in (('pixel', tau - n_step + 1, want_pix), ('pixel_next', tau + 1, want_next)):
            for a in range(n):
                src = stack_sources(top, stacks)
                dst[r0 + a] = np.concatenate([render(pixel, u, float(states[(ep, u)][a, 0])) for u in src], axis=0)
    return want_pix, want_next
