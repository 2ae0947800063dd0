"""
The torch-CPU double of the reset-stream entry points: ``ReachCpuKernels`` plus ``reset_fill`` and the ``resets=`` keyword
on the three doubles that step the environment.  A drawn row is the host definition itself (surreal_amd/env/tasks.py
reach_reset_state), so the CPU tier compares bit for bit.  The doubles it inherits restart an actor with
``state.copy_(init_state)``: with a stream they are handed a buffer in init_state's place, which the per-step hooks
(``env_step``, ``synth_ddpg_step``: both get called once per step) fill with the rows of episode ``episode + ends`` right
before a closing step reads it.  Without ``resets`` every call goes to the double it inherits, untouched.
"""
import contextlib

import torch

from reach_cpu_kernels import ReachCpuKernels
from surreal_amd.env import tasks as TK


def drawn(resets, n, J, ahead=0):
    """[n, 3 J] fp32: the rows of episode resets[2] + ahead for the actors resets[1] .. resets[1] + n - 1"""
    seed, base, episode = (int(v) for v in resets)
    return torch.as_tensor(TK.reach_reset_state(seed, base + torch.arange(n).numpy(), episode + ahead, J))


class ResetsCpuKernels(ReachCpuKernels):
    name = 'torch-cpu-double+tasks+resets'
    _rst = None              # while a launch with a stream walks its steps: [resets, buffer, ends so far, t, episode_len]

    @contextlib.contextmanager
    def _drawing(self, resets, like, t, episode_len):
        prev = self._rst
        self._rst = None if resets is None else [resets, torch.empty_like(like), 0, int(t), int(episode_len)]
        try:
            yield like if resets is None else self._rst[1]
        finally:
            self._rst = prev

    def _before_step(self):
        """the hook of a step: on a closing one the buffer gets the next episode's rows"""
        q = self._rst
        if q is None:
            return
        done = q[3] + 1 >= q[4]
        if done:
            n, D = q[1].shape
            q[1].copy_(drawn(q[0], n, D // 3, q[2]))
            q[2] += 1
        q[3] = 0 if done else q[3] + 1

    def reset_fill(self, resets, out, task='reach'):
        assert task == 'reach' and self.synth_task_supported(task, out.shape[1], out.shape[1] // 3)
        out.copy_(drawn(resets, out.shape[0], out.shape[1] // 3))

    def synth_env_step(self, state, init_state, actions, t, episode_len, *a, task='drift', resets=None, **kw):
        if resets is None:
            return super().synth_env_step(state, init_state, actions, t, episode_len, *a, task=task, **kw)
        assert task == 'reach'
        with self._drawing(resets, state, t, episode_len) as init:
            self._before_step()
            super().synth_env_step(state, init, actions, t, episode_len, *a, task=task, **kw)

    def synth_ppo_window_rollout(self, model, packed, lstm_packed, state, init_state, noise_scale, eps, t, episode_len,
                                 *a, task='drift', resets=None, **kw):
        if resets is None:
            return super().synth_ppo_window_rollout(model, packed, lstm_packed, state, init_state, noise_scale, eps, t,
                                                    episode_len, *a, task=task, **kw)
        assert task == 'reach'
        with self._drawing(resets, state, t, episode_len) as init:
            super().synth_ppo_window_rollout(model, packed, lstm_packed, state, init, noise_scale, eps, t, episode_len,
                                             *a, task=task, **kw)

    def synth_ddpg_rollout(self, net, packed, r, steps, *a, task='drift', resets=None, **kw):
        if resets is None:
            return super().synth_ddpg_rollout(net, packed, r, steps, *a, task=task, **kw)
        assert task == 'reach'
        with self._drawing(resets, r['state'], r['t'], r['episode_len']) as init:
            super().synth_ddpg_rollout(net, packed, dict(r, init_state=init), steps, *a, task=task, **kw)

    def env_step(self, state, acts):
        self._before_step()
        return super().env_step(state, acts)

    def synth_ddpg_step(self, r, mu, monitor=None):
        self._before_step()
        return super().synth_ddpg_step(r, mu, monitor=monitor)
