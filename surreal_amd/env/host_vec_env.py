"""
n host-stepped environments behind one batch interface: the way to run real simulators (GymAdapter, DMControlAdapter,
RobosuiteWrapper -- any ``Env`` whose observation is one flat low-dimensional array) with the device data path.  The
actors act as one batch on the device (``act_batch``), the simulators step on the host in actor order, and a
DeviceWindowRecorder / DeviceNStepRecorder (device_recorder.py) turns the step stream into the replay's experiences:

    venv = HostVecEnv([make_env(cfg)[0] for _ in range(n)])
    rec = DeviceWindowRecorder(n, venv.obs_dim, A, n_step, stride)
    venv.run_ppo(agent, rec, replay, T)          # begins the recorder on first use
    if replay.start_sample_condition():
        learner.learn(venv.to_batch(replay.sample_batch(batch_size)))

Episodes end whenever an environment says so; a done environment is reset right away and its first observation is what
the actor acts on next (Agent.main_loop's order, one process per agent in the reference).
"""
import collections

import numpy as np
import torch

from surreal_amd import kernels as KN


def flat_observation(obs):
    """the one low-dimensional array of an observation: the array itself, or the single entry of
    {'low_dim': {key: array}}"""
    if isinstance(obs, dict):
        mods = [m for m in obs if len(obs[m])]
        if mods != ['low_dim'] or len(obs['low_dim']) != 1:
            raise ValueError('HostVecEnv: one flat low-dimensional observation expected, got modalities %s'
                             % {m: list(obs[m]) for m in obs})
        obs = next(iter(obs['low_dim'].values()))
    return np.asarray(obs, dtype=np.float32).reshape(-1)


class HostVecEnv(object):
    def __init__(self, envs, device=None):
        self.envs = list(envs)
        if not self.envs:
            raise ValueError('HostVecEnv: no environments')
        self.n = len(self.envs)
        self.device = torch.device(device if device is not None else KN.default_device())
        self.obs_dim = None
        self._began = None                      # the recorder the current episodes were begun on

    def _buffers(self, D):
        pin = self.device.type == 'cuda'
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, pin_memory=pin)  # noqa: E731
        self.obs_dim = D
        self._obs, self._obs_next, self._obs_reset, self._rewards = f(self.n, D), f(self.n, D), f(self.n, D), f(self.n)
        self._dones = np.zeros(self.n, dtype=bool)
        self._actions = None

    def reset(self):
        """resets every environment -> their first observations [n, D] (a reused pinned buffer, as numpy)"""
        first = [flat_observation(env.reset()[0]) for env in self.envs]
        if self.obs_dim != first[0].size:
            self._buffers(first[0].size)
        obs = self._obs.numpy()
        for a, o in enumerate(first):
            obs[a] = o
        self._began = None
        return obs

    def step(self, actions):
        """actions [n, A] on the device: ONE device -> host copy, then every environment steps in actor order and the
        done ones are reset -> (obs_next [n, D] -- the terminal observation where done --, rewards [n], dones bool [n],
        obs_reset [n, D] -- the next episode's first observation in the rows of done actors, the other rows stale): numpy
        views of reused pinned buffers, valid until the next step()"""
        if self.obs_dim is None:
            raise RuntimeError('HostVecEnv.step before reset()')
        if self._actions is None or self._actions.shape != actions.shape:
            self._actions = torch.zeros(tuple(actions.shape), dtype=torch.float32,
                                        pin_memory=self.device.type == 'cuda')
        self._actions.copy_(actions)            # (a blocking copy: the actions are there when it returns)
        acts = self._actions.numpy()
        obs_next, obs_reset, rewards, dones = self._obs_next.numpy(), self._obs_reset.numpy(), self._rewards.numpy(), \
            self._dones
        for a, env in enumerate(self.envs):
            obs, reward, done, _ = env.step(acts[a].copy())
            obs_next[a] = flat_observation(obs)
            rewards[a] = reward
            dones[a] = bool(done)
            if dones[a]:
                obs_reset[a] = flat_observation(env.reset()[0])
        return obs_next, rewards, dones, obs_reset

    @staticmethod
    def to_batch(f):
        """the FIFO's window fields (sample_batch) -> the PPO learner's batch contract, as SyntheticVecEnv.to_batch"""
        low = lambda x: collections.OrderedDict(low_dim=collections.OrderedDict(flat_inputs=x))  # noqa: E731
        once = [f['cells'][:, 0], f['cells'][:, 1]] if 'cells' in f else None
        return {'obs': low(f['obs']), 'obs_next': low(f['obs_next']), 'actions': f['actions'], 'rewards': f['rewards'],
                'dones': f['dones'], 'persistent_infos': [f['pds']], 'onetime_infos': once}

    # ---- the acting loops ---------------------------------------------------------------------------------------
    def _begin(self, recorder):
        if self._began is not recorder:
            recorder.begin(self.reset())
            self._began = recorder

    def _done_mask(self, dones):
        return torch.as_tensor(dones).to(self.device)

    def run_ppo(self, agent, recorder, replay, T, monitor=None):
        """T steps of all environments under PPOAgent `agent`: act_batch on the recorder's observation, step, record
        (DeviceWindowRecorder), reset_batch for the done actors -> the number of windows written.  The first call on a
        recorder resets the environments and begins it; later calls go on where the last one stopped."""
        self._begin(recorder)
        rnn = bool(agent.rnn_config.if_rnn_policy)
        rows = 0
        for _ in range(int(T)):
            actions, pds = agent.act_batch(recorder.observation)
            cells = tuple(c[0] for c in agent.batch_cells_before) if rnn else None
            obs_next, rewards, dones, obs_reset = self.step(actions)
            rows += recorder.record(replay, actions, pds, rewards, dones, obs_next, obs_reset, cells_before=cells,
                                    monitor=monitor)
            if dones.any():
                agent.reset_batch(self._done_mask(dones))
        return rows

    def run_ddpg(self, agent, recorder, replay, T, monitor=None, sigmas=None):
        """T steps of all environments under DDPGAgent `agent` (act_batch; sigmas [n]: per-actor exploration scales),
        recorded as n-step transitions (DeviceNStepRecorder) -> the number of transitions written.  An agent whose batch
        path keeps per-actor exploration state (an OU process) restarts it for the done actors through its
        reset_batch(mask), as pre_episode does for one actor."""
        self._begin(recorder)
        rows = 0
        for _ in range(int(T)):
            actions = agent.act_batch(recorder.observation, sigmas=sigmas)
            obs_next, rewards, dones, obs_reset = self.step(actions)
            rows += recorder.record(replay, actions, rewards, dones, obs_next, obs_reset, monitor=monitor)
            if dones.any() and hasattr(agent, 'reset_batch'):
                agent.reset_batch(self._done_mask(dones))
        return rows
