"""
The on-device episode monitor (SyntheticVecEnv.attach_monitor -> DeviceEpisodeMonitor) against the host's EpisodeMonitor,
shared by the CPU tier (test_episode_monitor_cpu.py) and the GPU tier (test_gpu_episode_monitor.py):

  * ``MonitorMixin`` -- adds ``monitor=`` to every ``synth_*`` entry point of the existing torch-CPU doubles and applies
    the kernels' rule (smx_synth_env.inc.h episode_step) to the step's fp32 reward: the open fp64 sum in step order,
    the (reward, steps) pair into ring slot (finished episodes) % capacity on done.  ``PpoMonitorCpuKernels`` /
    ``DdpgMonitorCpuKernels`` are the PPO (raw step, rollout tables, LSTM rollout, windows, camera windows) and DDPG
    (persistent, per step, camera) doubles with it;
  * ``host_monitors`` -- while it is open, every ``SyntheticEnv`` the existing host-path helpers (host_ring,
    host_windows, ...) build is wrapped in ``wrap(env, index)`` (default: ``EpisodeMonitor``) before they wrap it
    further, so that the host monitors see the very steps those helpers drive;
  * ``sequential_sums`` -- the monitor a recorded [n, T] reward table implies, summed in fp64 in step order.
"""
import contextlib

import numpy as np
import torch

import ddpg_pixel_rollout_cases as DPC
import ppo_pixel_window_cases as PPC
import ppo_window_cases as PW


def feed(mon, rew, done):
    """episode_step for all actors: rew fp32 [n], done the shared clock's"""
    mon.ep_reward.add_(rew.double().view(-1))                  # (fp64 + widened fp32: one rounding, as the kernel)
    mon.ep_steps.add_(1)
    if done:
        n, c = mon.n, mon.capacity
        rows = torch.arange(n)
        slot = mon.ep_count % c
        mon.done_reward[rows, slot] = mon.ep_reward
        mon.done_steps[rows, slot] = mon.ep_steps
        mon.ep_count.add_(1)
        mon.ep_reward.zero_()
        mon.ep_steps.zero_()


class MonitorMixin(object):
    """monitor= on the doubles' entry points.  The launches that loop over steps call the per-step ones through self,
    so an entry point parks its monitor in self._mon and the per-step ones pick it up there."""
    _mon = None
    _clock = None            # [t, episode_len] while a windowed launch walks its steps (env_step does not get them)

    @contextlib.contextmanager
    def _parked(self, monitor, clock=None):
        prev = self._mon, self._clock
        self._mon = monitor if monitor is not None else self._mon
        self._clock = clock if clock is not None else self._clock
        try:
            yield
        finally:
            self._mon, self._clock = prev

    # ---- the per-step ends ---------------------------------------------------------------------------------------
    def synth_env_step(self, state, init_state, actions, t, episode_len, slot, obs_roll, act_roll, rew_roll, done_roll,
                       monitor=None):
        mon = monitor if monitor is not None else self._mon
        if mon is not None:
            _, rew = PW.PpoWindowCpuKernels.env_step(state, actions)
            feed(mon, rew, t + 1 >= episode_len)
        super().synth_env_step(state, init_state, actions, t, episode_len, slot, obs_roll, act_roll, rew_roll, done_roll)

    def env_step(self, state, acts):
        sn, rew = PW.PpoWindowCpuKernels.env_step(state, acts)
        if self._mon is not None:
            c = self._clock
            done = c[0] + 1 >= c[1]
            feed(self._mon, rew, done)
            c[0] = 0 if done else c[0] + 1
        return sn, rew

    def synth_ddpg_step(self, r, mu, monitor=None):
        mon = monitor if monitor is not None else self._mon
        tau, N = int(r['t']), int(r['n_step'])
        super().synth_ddpg_step(r, mu)
        if mon is not None:
            feed(mon, r['carry_rew'][:, tau % N], tau + 1 >= r['episode_len'])

    # ---- the entry points that reach them through self -------------------------------------------------------------
    def synth_act_env_step(self, *a, monitor=None):
        with self._parked(monitor):
            super().synth_act_env_step(*a)

    def synth_act_env_step_head(self, *a, monitor=None):
        with self._parked(monitor):
            super().synth_act_env_step_head(*a)

    def synth_lstm_rollout(self, *a, monitor=None, **kw):
        with self._parked(monitor):
            super().synth_lstm_rollout(*a, **kw)

    def synth_ppo_window_rollout(self, model, packed, lstm_packed, state, init_state, noise_scale, eps, t, episode_len,
                                 *a, monitor=None, **kw):
        with self._parked(monitor, [int(t), int(episode_len)]):
            super().synth_ppo_window_rollout(model, packed, lstm_packed, state, init_state, noise_scale, eps, t,
                                             episode_len, *a, **kw)

    def synth_ppo_pixel_window_step(self, r, mu, copy_workgroups=0, monitor=None):
        with self._parked(monitor, [int(r['t']), int(r['episode_len'])]):
            super().synth_ppo_pixel_window_step(r, mu, copy_workgroups)

    def synth_ddpg_rollout(self, net, packed, r, steps, actors_per_workgroup=0, monitor=None):
        with self._parked(monitor):
            super().synth_ddpg_rollout(net, packed, r, steps, actors_per_workgroup)

    def synth_ddpg_pixel_step(self, r, mu, monitor=None):
        with self._parked(monitor):
            super().synth_ddpg_pixel_step(r, mu)


class PpoMonitorCpuKernels(MonitorMixin, PPC.PpoPixelWindowCpuKernels):
    name = 'torch-cpu-double+episode-monitor(ppo)'


class DdpgMonitorCpuKernels(MonitorMixin, DPC.DdpgPixelRolloutCpuKernels):
    name = 'torch-cpu-double+episode-monitor(ddpg)'


@contextlib.contextmanager
def host_monitors(wrap=None):
    """-> the list the wrapped host envs are appended to, in the order they are built (actor order)"""
    from surreal_amd.env import EpisodeMonitor
    from surreal_amd.env import synthetic_env as SE
    wrap = wrap or (lambda env, index: EpisodeMonitor(env))
    made = []
    plain = SE.SyntheticEnv

    def monitored(*a, **kw):
        made.append(wrap(plain(*a, **kw), len(made)))
        return made[-1]
    SE.SyntheticEnv = monitored
    try:
        yield made
    finally:
        SE.SyntheticEnv = plain


def assert_equals_host(mon, hosts, polled=None):
    """the polled device monitor holds exactly what the host monitors hold: rewards and steps equal, not close"""
    if polled is None:
        mon.poll()
    assert mon.dropped == 0 and len(hosts) == mon.n
    for a, h in enumerate(hosts):
        assert mon.episode_steps[a] == h.episode_steps, (a, mon.episode_steps[a], h.episode_steps)
        assert mon.episode_rewards[a] == h.episode_rewards, (a, mon.episode_rewards[a], h.episode_rewards)
    assert mon.num_episodes == sum(h.num_episodes for h in hosts)
    assert mon.total_steps == sum(h.total_steps for h in hosts)
    # the open episodes: the host's running list of this episode's rewards
    rew, steps = mon.open_episodes()
    for a, h in enumerate(hosts):
        assert int(steps[a]) == len(h._rewards), (a, int(steps[a]), len(h._rewards))
        assert float(rew[a]) == float(sum(h._rewards)), a


def monitor_state(mon):
    """every word of the device monitor, as host tensors"""
    return {k: getattr(mon, k).detach().cpu().clone() for k in ('ep_reward', 'ep_steps', 'ep_count', 'done_reward',
                                                                 'done_steps')}


def assert_states_equal(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), k


def sequential_sums(rewards, clock0, episode_len, capacity):
    """rewards [n, T] fp32 recorded from clock clock0 -> the monitor state they imply (fp64 sums in step order)"""
    r = np.asarray(rewards, dtype=np.float32)
    n, T = r.shape
    out = {'ep_reward': np.zeros(n), 'ep_steps': np.zeros(n, np.int32), 'ep_count': np.zeros(n, np.int64),
           'done_reward': np.zeros((n, capacity)), 'done_steps': np.zeros((n, capacity), np.int32)}
    t = clock0
    for s in range(T):
        out['ep_reward'] = out['ep_reward'] + r[:, s].astype(np.float64)
        out['ep_steps'] += 1
        if t + 1 >= episode_len:
            slot = out['ep_count'] % capacity
            out['done_reward'][np.arange(n), slot] = out['ep_reward']
            out['done_steps'][np.arange(n), slot] = out['ep_steps']
            out['ep_count'] += 1
            out['ep_reward'] = np.zeros(n)
            out['ep_steps'][:] = 0
            t = 0
        else:
            t += 1
    return {k: torch.as_tensor(v) for k, v in out.items()}
