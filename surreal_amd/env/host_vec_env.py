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

With ``frame_stacks=S`` the environments have a camera: each emits ONE raw uint8 frame per step,
``obs['pixel']['camera0']`` [C, H, W], next to the one flat low-dimensional array -- no FrameStackWrapper: the stacking
is the device's (the recorders' ``pixel=(C, H, W), frame_stacks=S``):

    venv = HostVecEnv(envs, frame_stacks=3)
    venv.reset()                                 # -> venv.obs_dim, venv.pixel
    rec = DeviceWindowRecorder(n, venv.obs_dim, A, n_step, stride, pixel=venv.pixel, frame_stacks=3)
    venv.run_ppo(agent, rec, replay, T)          # an agent with a CNN stem on camera0 (S*C, H, W)

Observations without a low-dimensional part and frames stacked on the host are not taken.

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


def camera_observation(obs):
    """(the one low-dimensional array, the one raw camera frame uint8 [C, H, W]) of an observation
    {'pixel': {camera: frame}, 'low_dim': {key: array}}"""
    if not isinstance(obs, dict) or not len(obs.get('pixel', ())):
        raise ValueError('HostVecEnv: frame_stacks is set and an environment has no camera (a camera on only some '
                         'environments is not taken), got %s'
                         % ({m: list(obs[m]) for m in obs} if isinstance(obs, dict) else type(obs).__name__))
    if len(obs['pixel']) != 1:
        raise ValueError('HostVecEnv: one camera expected, got %s' % list(obs['pixel']))
    if not len(obs.get('low_dim', ())):
        raise ValueError('HostVecEnv: a pixel-only observation (no low-dimensional part, D = 0) is not taken')
    frame = next(iter(obs['pixel'].values()))
    if isinstance(frame, (list, tuple)):
        raise ValueError('HostVecEnv: one raw frame per step expected, got a list of %d (frames stacked on the host '
                         'are not taken)' % len(frame))
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3:
        raise ValueError('HostVecEnv: the frame must be uint8 [C, H, W], got %s %s' % (frame.dtype, frame.shape))
    flat = flat_observation({'low_dim': obs['low_dim']})
    if flat.size == 0:
        raise ValueError('HostVecEnv: a pixel-only observation (no low-dimensional part, D = 0) is not taken')
    return flat, frame


def _nested(f, low, pix):
    """the observation dict of a batch: field `low` as low_dim / flat_inputs and, where the batch has it, field `pix` as
    pixel / camera0"""
    obs = collections.OrderedDict(low_dim=collections.OrderedDict(flat_inputs=f[low]))
    if pix in f:
        obs['pixel'] = collections.OrderedDict(camera0=f[pix])
    return obs


class HostVecEnv(object):
    def __init__(self, envs, device=None, frame_stacks=None):
        """frame_stacks = S: the environments have a camera (one raw frame per step, stacked S deep on the device)"""
        self.envs = list(envs)
        if not self.envs:
            raise ValueError('HostVecEnv: no environments')
        if frame_stacks is not None and int(frame_stacks) < 1:
            raise ValueError('HostVecEnv: frame_stacks must be positive, got %r' % (frame_stacks,))
        self.n = len(self.envs)
        self.device = torch.device(device if device is not None else KN.default_device())
        self.frame_stacks = None if frame_stacks is None else int(frame_stacks)
        self.obs_dim = None
        self.pixel = None                       # (C, H, W) of the raw frame, known after reset()
        self._began = None                      # the recorder the current episodes were begun on

    def _buffers(self, D, pixel=None):
        pin = self.device.type == 'cuda'
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, pin_memory=pin)  # noqa: E731
        self.obs_dim = D
        self._obs, self._obs_next, self._obs_reset, self._rewards = f(self.n, D), f(self.n, D), f(self.n, D), f(self.n)
        self._dones = np.zeros(self.n, dtype=bool)
        self._actions = None
        self.pixel = pixel
        if pixel is not None:
            u8 = lambda: torch.zeros((self.n,) + pixel, dtype=torch.uint8, pin_memory=pin)  # noqa: E731
            self._frames, self._frames_next, self._frames_reset = u8(), u8(), u8()

    def _observe(self, obs, a, flat_out, frame_out):
        """one environment's observation into row a of the buffers"""
        if self.frame_stacks is None:
            flat_out[a] = flat_observation(obs)
            return
        flat, frame = camera_observation(obs)
        if frame.shape != self.pixel:
            raise ValueError('HostVecEnv: environment %d emits frames %s, the others %s' % (a, frame.shape, self.pixel))
        flat_out[a] = flat
        frame_out[a] = frame

    def reset(self):
        """resets every environment -> their first observations [n, D] (a reused pinned buffer, as numpy); with a camera
        -> (observations, first frames uint8 [n, C, H, W])"""
        first = [env.reset()[0] for env in self.envs]
        if self.frame_stacks is None:
            D, pixel = flat_observation(first[0]).size, None
        else:
            flat, frame = camera_observation(first[0])
            D, pixel = flat.size, tuple(frame.shape)
        if self.obs_dim != D or self.pixel != pixel:
            self._buffers(D, pixel)
        obs = self._obs.numpy()
        frames = self._frames.numpy() if pixel is not None else None
        for a, o in enumerate(first):
            self._observe(o, a, obs, frames)
        self._began = None
        return obs if pixel is None else (obs, frames)

    def step(self, actions):
        """actions [n, A] on the device: ONE device -> host copy, then every environment steps in actor order and the
        done ones are reset -> (obs_next [n, D] -- the terminal observation where done --, rewards [n], dones bool [n],
        obs_reset [n, D] -- the next episode's first observation in the rows of done actors, the other rows stale): numpy
        views of reused pinned buffers, valid until the next step().  With a camera the tuple goes on with frames_next
        uint8 [n, C, H, W] (the terminal frame where done) and frames_reset (the rows of done actors)"""
        if self.obs_dim is None:
            raise RuntimeError('HostVecEnv.step before reset()')
        if self._actions is None or self._actions.shape != actions.shape:
            self._actions = torch.zeros(tuple(actions.shape), dtype=torch.float32,
                                        pin_memory=self.device.type == 'cuda')
        self._actions.copy_(actions)            # (a blocking copy: the actions are there when it returns)
        acts = self._actions.numpy()
        obs_next, obs_reset, rewards, dones = self._obs_next.numpy(), self._obs_reset.numpy(), self._rewards.numpy(), \
            self._dones
        camera = self.pixel is not None
        frames_next, frames_reset = (self._frames_next.numpy(), self._frames_reset.numpy()) if camera else (None, None)
        for a, env in enumerate(self.envs):
            obs, reward, done, _ = env.step(acts[a].copy())
            self._observe(obs, a, obs_next, frames_next)
            rewards[a] = reward
            dones[a] = bool(done)
            if dones[a]:
                self._observe(env.reset()[0], a, obs_reset, frames_reset)
        if camera:
            return obs_next, rewards, dones, obs_reset, frames_next, frames_reset
        return obs_next, rewards, dones, obs_reset

    @staticmethod
    def to_batch(f):
        """the FIFO's window fields (sample_batch) -> the PPO learner's batch contract, as SyntheticVecEnv.to_batch
        (with 'pixel' / 'pixel_next' the nested pixel + low_dim observations)"""
        once = [f['cells'][:, 0], f['cells'][:, 1]] if 'cells' in f else None
        return {'obs': _nested(f, 'obs', 'pixel'), 'obs_next': _nested(f, 'obs_next', 'pixel_next'),
                'actions': f['actions'], 'rewards': f['rewards'], 'dones': f['dones'], 'persistent_infos': [f['pds']],
                'onetime_infos': once}

    @staticmethod
    def to_ddpg_batch(f):
        """the uniform replay's transition fields (sample_batch, also into DDPGLearner.staging_fields) -> the DDPG
        learner's batch contract: nested observations, rewards / dones [B, 1]"""
        B = f['actions'].shape[0]
        return {'obs': _nested(f, 'obs', 'pixel'), 'obs_next': _nested(f, 'obs_next', 'pixel_next'),
                'actions': f['actions'], 'rewards': f['rewards'].view(B, 1), 'dones': f['dones'].view(B, 1)}

    # ---- the acting loops ---------------------------------------------------------------------------------------
    def _begin(self, recorder, agent=None):
        if self._began is not recorder:
            first = self.reset()
            self._camera_refusal(recorder, agent)
            if self.pixel is None:
                recorder.begin(first)
            else:
                recorder.begin(*first)
            self._began = recorder

    def _camera_refusal(self, recorder, agent):
        """environments, recorder and agent must agree on the camera"""
        S = self.frame_stacks
        if getattr(recorder, 'pixel', None) != self.pixel or (self.pixel is not None and recorder.frame_stacks != S):
            raise ValueError('HostVecEnv: the recorder\'s camera %s x %s is not the environments\' %s x %s'
                             % (getattr(recorder, 'pixel', None), getattr(recorder, 'frame_stacks', None), self.pixel, S))
        if self.pixel is None or agent is None:
            return
        C, H, W = self.pixel
        spec = getattr(agent, 'obs_spec', None) or {}
        cams = spec.get('pixel') or {}
        cam = tuple(int(v) for v in cams['camera0']) if 'camera0' in cams else None
        if cam != (S * C, H, W):
            raise ValueError('HostVecEnv: the agent\'s camera0 %s is not the environments\' stacked frame %s'
                             % (cam, (S * C, H, W)))

    @staticmethod
    def _frames_of(step):
        """record()'s camera arguments out of step()'s tuple"""
        return dict(frames_next=step[4], frames_reset=step[5]) if len(step) == 6 else {}

    def _done_mask(self, dones):
        return torch.as_tensor(dones).to(self.device)

    def run_ppo(self, agent, recorder, replay, T, monitor=None):
        """T steps of all environments under PPOAgent `agent`: act_batch on the recorder's observation, step, record
        (DeviceWindowRecorder), reset_batch for the done actors -> the number of windows written.  The first call on a
        recorder resets the environments and begins it; later calls go on where the last one stopped."""
        self._begin(recorder, agent)
        rnn = bool(agent.rnn_config.if_rnn_policy)
        rows = 0
        for _ in range(int(T)):
            actions, pds = agent.act_batch(recorder.observation)
            cells = tuple(c[0] for c in agent.batch_cells_before) if rnn else None
            step = self.step(actions)
            obs_next, rewards, dones, obs_reset = step[:4]
            rows += recorder.record(replay, actions, pds, rewards, dones, obs_next, obs_reset, cells_before=cells,
                                    monitor=monitor, **self._frames_of(step))
            if dones.any():
                agent.reset_batch(self._done_mask(dones))
        return rows

    def run_ddpg(self, agent, recorder, replay, T, monitor=None, sigmas=None):
        """T steps of all environments under DDPGAgent `agent` (act_batch; sigmas [n]: per-actor exploration scales),
        recorded as n-step transitions (DeviceNStepRecorder) -> the number of transitions written.  An agent whose batch
        path keeps per-actor exploration state (an OU process) restarts it for the done actors through its
        reset_batch(mask), as pre_episode does for one actor."""
        self._begin(recorder, agent)
        rows = 0
        for _ in range(int(T)):
            actions = agent.act_batch(recorder.observation, sigmas=sigmas)
            step = self.step(actions)
            obs_next, rewards, dones, obs_reset = step[:4]
            rows += recorder.record(replay, actions, rewards, dones, obs_next, obs_reset, monitor=monitor,
                                    **self._frames_of(step))
            if dones.any() and hasattr(agent, 'reset_batch'):
                agent.reset_batch(self._done_mask(dones))
        return rows
