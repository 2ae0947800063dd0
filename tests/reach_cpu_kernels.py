"""
The torch-CPU double of the task entry points: ``TorchCpuKernels`` (through the windowed PPO and the DDPG rollout doubles,
with the episode monitor's mixin) plus the ``task=`` keyword on the three doubles that step the environment --
``synth_env_step``, ``synth_ppo_window_rollout`` and ``synth_ddpg_rollout``.  With 'reach' a step is the host definition
itself (surreal_amd/env/tasks.py reach_step), so the CPU tier compares bit for bit; with 'drift' every call goes to the
double it inherits, untouched.
"""
import contextlib

import numpy as np
import torch

import ddpg_rollout_cases as DC
import episode_monitor_cases as EM
import ppo_window_cases as PW
from surreal_amd import _lib as L
from surreal_amd.env import tasks as TK


def reach(state, acts):
    """reach_step on torch fp32 tensors -> (next state before any reset, reward)"""
    sn, rew = TK.reach_step(state.detach().cpu().numpy(), acts.detach().cpu().numpy())
    return torch.as_tensor(sn), torch.as_tensor(rew)


class ReachCpuKernels(EM.MonitorMixin, PW.PpoWindowCpuKernels, DC.DdpgRolloutCpuKernels):
    name = 'torch-cpu-double+tasks'
    _task = 'drift'

    @contextlib.contextmanager
    def _on_task(self, task):
        assert task in TK.TASKS, task
        prev, self._task = self._task, task
        try:
            yield
        finally:
            self._task = prev

    def synth_task_supported(self, task, D, A):
        tid = TK.TASK_IDS[task] if isinstance(task, str) else int(task)
        return self.lib_supported('smx_synth_task_supported', tid, D, A)

    # ---- the three doubles ---------------------------------------------------------------------------------------------
    def synth_env_step(self, state, init_state, actions, t, episode_len, slot, obs_roll, act_roll, rew_roll, done_roll,
                       monitor=None, task='drift'):
        if task == 'drift':
            return super().synth_env_step(state, init_state, actions, t, episode_len, slot, obs_roll, act_roll, rew_roll,
                                          done_roll, monitor=monitor)
        assert self.synth_task_supported(task, state.shape[1], actions.shape[1])
        sn, rew = reach(state, actions)
        done = t + 1 >= episode_len
        if monitor is not None:
            EM.feed(monitor, rew, done)
        if obs_roll is not None:
            obs_roll[:, slot] = state
            if slot + 1 < obs_roll.shape[1]:
                obs_roll[:, slot + 1] = sn
            act_roll[:, slot] = actions.clamp(-1.0, 1.0)
            rew_roll[:, slot] = rew
            done_roll[:, slot] = 1.0 if done else 0.0
        state.copy_(init_state if done else sn)

    def synth_ppo_window_rollout(self, model, *a, task='drift', noise=None, **kw):
        assert noise is None, 'the doubles draw from no stream: pass eps'
        if task != 'drift':
            assert self.synth_task_supported(task, model.rnn.D if model.if_rnn else model.actor.D, model.actor.OUT)
        with self._on_task(task):
            super().synth_ppo_window_rollout(model, *a, **kw)

    def synth_ddpg_rollout(self, net, packed, r, steps, actors_per_workgroup=0, monitor=None, noise=None, task='drift'):
        assert noise is None, 'the doubles draw from no stream: pass eps'
        if task != 'drift':
            assert self.synth_task_supported(task, net.D, net.OUT)
        with self._on_task(task):
            super().synth_ddpg_rollout(net, packed, r, steps, actors_per_workgroup, monitor=monitor)

    # ---- what they step through ---------------------------------------------------------------------------------------
    def env_step(self, state, acts):
        """the windowed double's step (the monitor's mixin feeds from it)"""
        if self._task == 'drift':
            return super().env_step(state, acts)
        sn, rew = reach(state, acts)
        if self._mon is not None:
            c = self._clock
            done = c[0] + 1 >= c[1]
            EM.feed(self._mon, rew, done)
            c[0] = 0 if done else c[0] + 1
        return sn, rew

    def synth_ddpg_step(self, r, mu, monitor=None):
        """DdpgRolloutCpuKernels.synth_ddpg_step with the task's dynamics in place of the drift's"""
        if self._task == 'drift':
            return super().synth_ddpg_step(r, mu, monitor=monitor)
        mon = monitor if monitor is not None else self._mon
        state, init = r['state'], r['init_state']
        n = state.shape[0]
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
        sn, rew = reach(state, a)
        done = tau + 1 >= r['episode_len']
        slot, jslot = tau % N, (tau + 1) % N
        r['carry_obs'][:, slot] = state
        r['carry_act'][:, slot] = a
        r['carry_rew'][:, slot] = rew
        if tau >= N - 1:
            tabs = r['tables']
            cap = tabs['obs'].shape[0]
            rows = (int(r['cursor']) + torch.arange(n)) % cap
            tabs['obs'][rows] = r['carry_obs'][:, jslot]
            tabs['actions'][rows] = r['carry_act'][:, jslot]
            tabs['obs_next'][rows] = sn
            tabs['rewards'][rows] = nstep_sum(r['carry_rew'], r['gpow'], N, tau).view(n, 1)
            tabs['dones'][rows] = 1.0 if done else 0.0
        if mon is not None:
            EM.feed(mon, rew, done)
        state.copy_(init if done else sn)


def nstep_sum(carry_rew, gpow, N, tau):
    """the closing transition's reward as the kernels' nstep_reward forms it: carry_rew [n, N] fp32 (step u in slot u %
    N), gpow fp64 [N]; transition j = tau - N + 1; fp64, u ascending, rounded once"""
    j = tau - N + 1
    R = carry_rew[:, j % N].double()
    for u in range(j + 1, tau + 1):
        e = (u - j) if u >= N - 1 else (N - 1 - j)
        R = R + gpow[e] * carry_rew[:, u % N].double()
    return R.float()


def np_nstep_sum(rewards, gpow, N, tau):
    """the same from numpy: rewards [n, tau + 1] fp32 by episode step"""
    r = torch.as_tensor(np.ascontiguousarray(rewards))
    ring = torch.zeros(r.shape[0], N)
    for u in range(max(tau - N + 1, 0), tau + 1):
        ring[:, u % N] = r[:, u]
    return nstep_sum(ring, torch.as_tensor(gpow), N, tau).numpy()
