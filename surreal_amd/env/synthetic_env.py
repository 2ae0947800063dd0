"""
Synthetic environments.  The reference has no synthetic env (it steps MuJoCo / Robosuite
simulators, one OS process per agent: surreal/agent/base.py:244-271, surreal/env/make_env.py);
BASELINE.json's configs[4] is a synthetic 1024-actor workload, so the dynamics are defined here
once and implemented twice with bit-identical fp32 results:

  * ``SyntheticEnv``    -- one actor, numpy, the reference ``Env`` protocol (reset/step, nested
    obs dicts): drives the reference-style Agent + windowing wrappers in tests;
  * ``SyntheticVecEnv`` -- all actors of a GPU stepped by ONE HIP launch
    (smx_synth_env_step_f32, csrc/smx_replay.hip) that also records the step straight into the
    device-resident rollout [actors, T, .]; ``emit_windows`` then cuts the rollout into
    n_step / stride sub-trajectories (smx_window_emit_f32) exactly as
    ExpSenderWrapperMultiStepMovingWindowWithInfo would have, without the data ever leaving HBM.

Dynamics (all fp32, no fused multiply-add):
    a      = clip(action, -1, 1)
    s'[k]  = clamp(0.9*s[k] + 0.5*a[k % A] + 0.01*((37k) % 17 - 8), -10, 10)
    reward = -0.1 * sum_j a[j]^2 + 0.05 * s'[0]      (accumulated in fp64, rounded once)
    done   = (t + 1 >= episode_len)

These are the dynamics of task 'drift', the default: a workload, not a task.  task='reach' (tasks.py) is one a policy can
learn, defined the same way -- once, in fp32 without fused multiply-add -- and run by both classes; task='arm' (tasks.py) is
a second one, a planar multi-link arm with nonlinear kinematics and a reward that couples all joints.
"""
import collections
import types

import numpy as np
import torch

from surreal_amd import kernels as KN
from surreal_amd import _lib as L
from . import actor_clocks as AC
from . import tasks as TK
from .base import Env


def _drift(D):
    k = np.arange(D)
    return (np.float32(0.01) * ((37 * k) % 17 - 8).astype(np.float32)).astype(np.float32)


class SyntheticEnv(Env):
    def __init__(self, obs_dim, action_dim, episode_len=200, seed=0, pixel=None, task='drift', resets=None,
                 disturbance=0.0):
        """pixel = (C, H, W): also emit a uint8 camera frame obs['pixel']['camera0'] (a fixed
        pattern shifted by the step count and the first state component).
        task: 'drift' (the dynamics above), 'reach' (env/tasks.py: obs_dim == 3 * action_dim, no camera) or 'arm' (likewise:
        obs_dim == 2 * action_dim + 2, no camera).
        resets = (seed, actor_id), tasks 'reach' and 'arm' only: every _reset() begins a NEW episode, drawn from the reset
        stream (tasks.reach_reset_state / arm_reset_state(seed, actor_id, self.episode, J); self.episode: the index of the
        next one, from 0) --
        the host form of SyntheticVecEnv.attach_resets; init_state is not read.
        disturbance = s in [0, 1], with resets= only: step t of the episode under way (self.episode - 1) adds s *
        tasks.disturbance(seed, actor_id, self.episode - 1, t, J) (env/tasks.py); the env is stepped from a reset()."""
        TK.check_task('SyntheticEnv', task, obs_dim, action_dim, pixel)
        self.task = task
        self.resets, self.episode = None, 0
        self.disturbance = float(TK.check_disturbance('SyntheticEnv', disturbance))
        self._draws = None
        if self.disturbance != 0 and task == 'drift':
            raise ValueError("SyntheticEnv: task %r takes no disturbance (tasks 'reach' and 'arm' do)" % (task,))
        if self.disturbance != 0 and resets is None:
            raise ValueError('SyntheticEnv: a disturbance is drawn from the reset stream: resets=(seed, actor_id) is required')
        if resets is not None:
            if task == 'drift':
                raise ValueError("SyntheticEnv: task %r has no reset distribution (resets=: task 'reach')" % (task,))
            self.resets = (int(resets[0]), int(resets[1]))
        self.D, self.A, self.episode_len = obs_dim, action_dim, episode_len
        self.pixel = tuple(pixel) if pixel is not None else None
        self.rs = np.random.RandomState(seed)
        self.init_state = self.rs.randn(obs_dim).astype(np.float32)
        self.state = self.init_state.copy()
        self.t = 0

    def observation_spec(self):
        spec = collections.OrderedDict(low_dim=collections.OrderedDict(flat_inputs=(self.D,)))
        if self.pixel is not None:
            spec['pixel'] = collections.OrderedDict(camera0=self.pixel)
        return spec

    def _frame(self):
        C, H, W = self.pixel
        c, y, x = np.meshgrid(np.arange(C), np.arange(H), np.arange(W), indexing='ij')
        shift = 3 * self.t + int(100 * abs(float(self.state[0])))
        return ((37 * c + 5 * y + 11 * x + shift) % 256).astype(np.uint8)

    def action_spec(self):
        return {'dim': (self.A,), 'type': 'continuous'}

    def _obs(self):
        obs = collections.OrderedDict(
            low_dim=collections.OrderedDict(flat_inputs=self.state.copy()))
        if self.pixel is not None:
            obs['pixel'] = collections.OrderedDict(camera0=self._frame())
        return obs

    def _reset(self):
        if self.resets is not None:
            self.state = TK.RESET_STATE[self.task](self.resets[0], self.resets[1], self.episode, self.A)
            self.episode += 1
        else:
            self.state = self.init_state.copy()
        self.t = 0
        return self._obs(), {}

    def _step(self, action):
        if self.task != 'drift':
            kw = {}
            if self.disturbance != 0:
                if self.episode < 1:
                    raise ValueError('SyntheticEnv: a disturbed env is stepped from a reset(): the episode under way has '
                                     'no index yet')
                if self._draws is None or self._draws[0] != self.episode - 1:
                    # (the draws of the episode's steps at once: the same numbers, one Philox call an episode)
                    self._draws = (self.episode - 1, TK.disturbance(self.resets[0], self.resets[1], self.episode - 1,
                                                                    np.arange(self.episode_len), self.A))
                kw = dict(w=self._draws[1][self.t], scale=self.disturbance)
            sn, reward = TK.STEP[self.task](self.state, np.asarray(action, dtype=np.float32).reshape(-1), **kw)
            done = (self.t + 1 >= self.episode_len)
            self.t += 1
            self.state = sn
            return self._obs(), float(reward), done, {}
        a = np.clip(np.asarray(action, dtype=np.float32).reshape(-1), -1.0, 1.0).astype(np.float32)
        k = np.arange(self.D)
        sn = (np.float32(0.9) * self.state + np.float32(0.5) * a[k % self.A]).astype(np.float32)
        sn = np.clip((sn + _drift(self.D)).astype(np.float32), -10.0, 10.0).astype(np.float32)
        reward = float(np.float32(-0.1 * np.sum(a.astype(np.float64) ** 2) + 0.05 * float(sn[0])))
        done = (self.t + 1 >= self.episode_len)
        self.t += 1
        self.state = sn
        return self._obs(), reward, done, {}


class SyntheticVecEnv(object):
    """n actors on one GPU; rollouts of T steps recorded on the device"""

    def __init__(self, n_actors, obs_dim, action_dim, episode_len=200, seeds=None, device=None,
                 kernels=None, pixel=None, frame_stacks=1, task='drift'):
        """task: 'drift', 'reach' or 'arm' (env/tasks.py; SyntheticEnv's rules: obs_dim == 3 * action_dim resp. 2 *
        action_dim + 2, no camera): a task
        env is stepped by step(), ppo_rollout_into and ddpg_rollout_into's one-launch route; every other stepping call
        and route refuses it (_drift_only).
        pixel = (C, H, W): every actor also has a camera (SyntheticEnv's frame: a pattern shifted by the step
        count and the first state component), rendered on the device; frame_stacks = n: the policy observes the
        last n frames on the channel axis (FrameStackWrapper's rule, surreal/env/wrapper.py:407-472) -- the rollout
        stores ONE raw uint8 frame per step and the stacking is a gather (smx_frame_stack_u8).
        episode_len: an int -- all actors share one episode clock -- or a sequence of n ints (also when they are all
        equal): every actor has an episode length and a clock of its own (per_actor_clocks; env/actor_clocks.py), which
        the one-launch low-dimensional ppo_rollout_into / ddpg_rollout_into take and every other stepping call refuses."""
        TK.check_task('SyntheticVecEnv', task, obs_dim, action_dim, pixel)
        self.task = task
        self.K = kernels or KN.default_kernels()
        self.device = device or KN.default_device()
        self.n, self.D, self.A = n_actors, obs_dim, action_dim
        self.per_actor_clocks = not isinstance(episode_len, (int, np.integer))
        if self.per_actor_clocks:
            lens = np.asarray(list(episode_len))
            if lens.shape != (n_actors,) or lens.dtype.kind not in 'iu' or (lens < 1).any() or (lens >= 2 ** 31).any():
                raise ValueError('SyntheticVecEnv: episode_len must be an int or %d ints >= 1, got %r'
                                 % (n_actors, episode_len))
            episode_len = np.ascontiguousarray(lens, dtype=np.int32)
            self._clk = {}            # the device copies: 'L', 't' int32 [n], the [T, n] row tables by T
        self.episode_len = episode_len
        self.pixel = tuple(pixel) if pixel is not None else None
        self.frame_stacks = int(frame_stacks) if pixel is not None else 1
        seeds = list(range(n_actors)) if seeds is None else list(seeds)
        init = np.stack([np.random.RandomState(s).randn(obs_dim).astype(np.float32) for s in seeds])
        self.init_state = torch.as_tensor(init).to(self.device)
        self.state = self.init_state.clone()
        self.t = self._clock_zero()
        self.rolls = None
        self.persistent = True        # rollout(): the one-launch kernel where the policy's shapes allow it
        self._ddpg = {}               # ddpg_rollout_into(): the open n-step transitions and OU states of the actors
        self._ppo = {}                # ppo_rollout_into(): the open moving windows of the actors
        self.monitor = None           # attach_monitor(): the actors' episode returns, kept by the step launches
        self.noise = None             # attach_noise(): the exploration noise as a per-actor stream, drawn by the launches
        self.resets = None            # attach_resets(): the episodes' first states as a per-actor stream, likewise
        self.param_noise = None       # attach_param_noise(): per-agent parameter-space noise for ddpg_rollout_into

    def _clock_zero(self):
        """the clock(s) right after a reset: an int, or with per-actor clocks int32 [n]"""
        return np.zeros(self.n, dtype=np.int32) if self.per_actor_clocks else 0

    @property
    def clocks(self):
        """every actor's step within its episode, np.int32 [n] (a copy)"""
        return np.array(np.broadcast_to(self.t, (self.n,)), dtype=np.int32)

    @property
    def episode_lens(self):
        """every actor's episode length, np.int32 [n] (a copy)"""
        return np.array(np.broadcast_to(self.episode_len, (self.n,)), dtype=np.int32)

    def _shared_clock_only(self, who):
        """`who` steps all actors on one clock: refused on an env whose actors have their own"""
        if self.per_actor_clocks:
            raise NotImplementedError('%s: per-actor episode clocks: the one-launch low-dimensional ppo_rollout_into / '
                                      'ddpg_rollout_into only' % who)

    def _drift_only(self, who, what=None, throw=True):
        """`who` (its variant `what`) steps the 'drift' dynamics only: refused on a task env -- raised here, or
        (throw=False) returned as (exception class, message) for the callers that collect their refusals; None on a
        'drift' env"""
        if self.task == 'drift':
            return None
        refusal = (NotImplementedError,
                   "%s%s: task %r is stepped by step(), ppo_rollout_into (a plain-MLP or one-layer LSTM policy the "
                   "one-launch kernel takes) and ddpg_rollout_into's 'launch' route (a plain actor, no parameter noise), on "
                   "one shared clock, only" % (who, ' with ' + what if what else '', self.task))
        if throw:
            raise refusal[0](refusal[1])
        return refusal

    def _task_kw(self, who):
        """the keyword a launch that takes tasks gets on a task env (none on 'drift': kernels objects that know no tasks
        are called as before); the shapes the device's task entry points refuse are refused here"""
        if self.task == 'drift':
            return {}
        if not self.K.synth_task_supported(self.task, self.D, self.A):
            raise ValueError('%s: task %r with %d actions; the device runs action_dim <= %d (smx_synth_task_supported)'
                             % (who, self.task, self.A, TK.MAX_A[self.task]))
        return {'task': self.task}

    def _disturbed_ok(self, who):
        """a stepping call on a disturbed env: the episode under way is DeviceResets.episode - 1, so one must have begun --
        by reset() -- since the stream was attached (or the counter set)"""
        if self.resets is not None and self.resets.disturbance != 0 and self.resets.episode < 1:
            raise ValueError('%s: a disturbed env is stepped from a reset(): the episode under way has no index yet '
                             '(DeviceResets.episode is %d, the index of the NEXT one)' % (who, self.resets.episode))

    def _clock_args(self, T, n_step, advance, rows):
        """the `clocks` keyword of a per-actor launch over the next T steps: the clocks as they are now and the episode
        lengths on the device, and the call's row table (one launch, K.actor_clock_rows; the buffers are reused: L once,
        t and the [T, n] table per call).  The clocks go up without a synchronisation, as the recorders' steps do
        (device_recorder._StagingSet): through one of two pinned host buffers, copied asynchronously on the stream; an
        event says when a buffer's copy has read it, and is waited for only before that buffer is written again, two
        calls later"""
        c, dev = self._clk, self.device
        if 'L' not in c:
            cuda = torch.device(dev).type == 'cuda'
            c['L'] = torch.from_numpy(self.episode_len).to(dev)
            c['t'] = torch.zeros(self.n, dtype=torch.int32, device=dev)
            c['stage'] = [[torch.zeros(self.n, dtype=torch.int32, pin_memory=cuda),
                           torch.cuda.Event() if cuda else None, False] for _ in range(2)]
            c['turn'] = 0
        if T not in c:
            c[T] = torch.empty(T, self.n, dtype=torch.int32, device=dev)
        stage = c['stage'][c['turn']]
        c['turn'] = 1 - c['turn']
        host, event, in_flight = stage
        if in_flight and event is not None:
            event.synchronize()                  # (the copy of two calls ago: long done)
        t_host = host.numpy()
        t_host[:] = self.t
        c['t'].copy_(host, non_blocking=True)
        if event is not None:
            event.record()
        stage[2] = True
        self.K.actor_clock_rows(c['t'], c['L'], T, n_step, advance, c[T], t_host=t_host, episode_len_host=self.episode_len)
        return {'clocks': dict(t=c['t'], episode_len=c['L'], row_off=c[T], rows=rows)}

    def attach_monitor(self, capacity=16):
        """-> a DeviceEpisodeMonitor (env/monitor.py) that every stepping launch from now on feeds: per actor the open
        episode's reward sum and length, and a ring of its last `capacity` finished episodes -- on the device, carried
        from call to call like the open windows; poll() it for the episodes.  Starts empty: the steps an open episode
        took before this call are not in it."""
        from .monitor import DeviceEpisodeMonitor
        self.monitor = DeviceEpisodeMonitor(self.n, capacity, self.device)
        return self.monitor

    def detach_monitor(self):
        """the launches stop feeding the monitor (which keeps what it has) -> it"""
        m, self.monitor = self.monitor, None
        return m

    def _mon(self, k=0):
        """the keyword a stepping launch takes when a monitor is attached (none otherwise: kernels objects that know
        no monitors are called as before), k env steps of every actor counted on the way"""
        if self.monitor is None:
            return {}
        self.monitor.count_steps(k)
        return {'monitor': self.monitor}

    def attach_noise(self, seed, actor_base=0):
        """-> a DeviceNoise (env/monitor.py): from now on a stepping call that gets no `eps` draws its exploration noise
        inside its launches, the standard normal of (seed, actor_base + a, draw step, component) for actor a (struct
        smx_noise_stream, include/surreal_amd.h) -- no [T, n, A] tensor is made.  The draw step is one host counter all
        actors share (DeviceNoise.step, readable and settable): every stepping call advances it by its env steps,
        whether or not its draws came from the stream; reset() does not rewind it.  An actor's noise then depends on
        its global id and the step count alone: not on n, T, the cut of a run into calls or the split of the actors
        over envs (actor_base: the global id of this env's actor 0).  An explicit `eps` still wins; the deterministic
        agent modes still draw nothing."""
        from .monitor import DeviceNoise
        self.noise = DeviceNoise(seed, actor_base, self.n, self.A, self.K, self.device)
        return self.noise

    def detach_noise(self):
        """the calls draw with torch.randn again -> the stream (which keeps its counter)"""
        m, self.noise = self.noise, None
        return m

    def attach_resets(self, seed, actor_base=0, disturbance=0.0):
        """-> a DeviceResets (env/monitor.py), tasks 'reach' and 'arm' only: from now on every episode begins with a row drawn
        from the reset stream -- element k of actor a's row for episode e is tasks.reach_reset_state(seed, actor_base + a,
        e, J)[k], on 'arm' arm_reset_state's (struct smx_reset_stream, include/surreal_amd.h) -- inside the launch that steps over the episode's end:
        no host round trip, no [n, D] upload, and init_state is not read.  The episode index is one host counter all
        actors share (DeviceResets.episode, readable and settable: the index of the NEXT episode to begin): reset()
        draws it and adds one, step / ppo_rollout_into / ddpg_rollout_into add their calls' episode ends.  An actor's
        episodes then depend on its global id and the index alone: not on n, T, the cut of a run into calls or the
        split of the actors over envs (actor_base: the global id of this env's actor 0).  The state is left as it is:
        reset() to begin episode `episode`.
        disturbance = s in [0, 1] (DeviceResets.disturbance): the task becomes stochastic -- step t of episode e of actor a
        adds s * tasks.disturbance(seed, actor_base + a, e, t, J)[j] to the sum that becomes v'[j] / omega'[j], drawn in the
        lane that forms it; a pure function of (seed, actor, episode, step), so everything above still holds.  0: no term
        is added, the bytes of an undisturbed stream.  A disturbed env is stepped from a reset() (the episode under way
        is episode - 1)."""
        if self.task == 'drift':
            if disturbance != 0:
                raise ValueError("attach_resets: task %r takes no disturbance (tasks 'reach' and 'arm' do)" % (self.task,))
            raise ValueError("attach_resets: task %r has no reset distribution (task 'reach' has)" % (self.task,))
        self._shared_clock_only('attach_resets')
        self._task_kw('attach_resets')
        from .monitor import DeviceResets
        self.resets = DeviceResets(seed, actor_base, self.n, self.D, self.K, self.device, task=self.task,
                                   disturbance=disturbance)
        return self.resets

    def detach_resets(self):
        """every actor restarts from its init_state again -> the stream (which keeps its counter)"""
        m, self.resets = self.resets, None
        return m

    def _rst(self, k):
        """the keyword a stepping launch of k steps takes when a reset stream is attached (none otherwise: kernels
        objects that know no streams are called as before).  The stream's index moves on by the call's episode ends,
        (t + k) // episode_len on the shared clock t: call this before the clock advances"""
        if self.resets is None:
            return {}
        at = self.resets.at()
        self.resets.episode += (int(self.t) + int(k)) // int(self.episode_len)
        return {'resets': at}

    def attach_param_noise(self, agent, seed, actors_per_agent=4, agent_base=0):
        """-> a DeviceParamNoise (env/monitor.py) of DDPGAgent `agent`'s parameter-space noise ('normal' or
        'adaptive_normal': its type, sigma, alpha and target_stddev): from now on ddpg_rollout_into runs every group of
        actors_per_agent consecutive actors (a multiple of 4) -- an AGENT, global id agent_base + its index -- from its
        own perturbed copy of the actor, made on the device, and with 'adaptive_normal' measures the action distance
        inside the launch.  The agent's host noise is switched off (on_parameter_fetched no longer perturbs: its model
        stays clean, nothing is perturbed twice); call refresh() on the returned object after every parameter fetch."""
        from .monitor import DeviceParamNoise
        self.param_noise = DeviceParamNoise(agent, seed, actors_per_agent, agent_base, self.n, self.K, self.device)
        agent.device_param_noise = True
        return self.param_noise

    def detach_param_noise(self):
        """ddpg_rollout_into does what it did before; the agent's host noise is on again -> the DeviceParamNoise"""
        m, self.param_noise = self.param_noise, None
        if m is not None:
            m.agent.device_param_noise = False
        return m

    def _noi(self, k, on=False):
        """the keyword a stepping launch takes when its draws come from the attached stream (`on`: what _draws
        answered; none otherwise: kernels objects that know no streams are called as before); the stream's clock moves
        on by the k env steps of the launch either way"""
        if self.noise is None:
            return {}
        at = self.noise.at()
        self.noise.step += int(k)
        return {'noise': at} if on else {}

    def reset(self):
        if self.resets is not None:
            self.resets.fill(self.state)      # (episode `episode` of every actor: the launches' own function)
            self.resets.episode += 1
        else:
            self.state.copy_(self.init_state)
        self.t = self._clock_zero()
        if self.monitor is not None:
            self.monitor.clear_open()         # (EpisodeMonitor._reset: an unfinished episode is dropped)
        for k in ('carry_obs', 'carry_act', 'carry_rew', 'ou', 'hist'):
            if self._ddpg.get(k) is not None:
                self._ddpg[k].zero_()
        self._ddpg['hist_pos'] = None         # (a camera's frame history is primed again at the next call)
        self._ddpg['pool_replay'] = None      # (so is its place in a replay's frame pool)
        self._ppo = {}                        # (the open windows: a new episode has none)
        return self.state

    # ---- the env's state (utils/run_state.py) ----------------------------------------------------------------------
    _ATTACHMENTS = ('noise', 'resets', 'monitor', 'param_noise')

    def _state_refusal(self, who):
        if self.pixel is not None:
            raise NotImplementedError('%s: a camera env: its frame histories (and a replay\'s frame pool) are not carried'
                                      % who)

    def state_dict(self):
        """What the next ppo_rollout_into / ddpg_rollout_into / step reads, as LIVE tensors (run_state.to_host / save_run
        make the host copy): `state`; the clock `t` (an int, or int32 [n] with per-actor clocks); the open PPO windows
        (_ppo: key, every carry tensor, t) and the open DDPG transitions and fp64 OU states (_ddpg: n_step, carry_obs /
        carry_act / carry_rew, ou); under their own keys the states of what is attached -- 'noise', 'resets', 'monitor',
        'param_noise', None where nothing is --; and a fingerprint: n, D, A, task, episode_len and init_state.
        Derived, so rebuilt and not stored: the device copies of the clocks (_clk), gamma's powers and the packed
        parameter copies (they follow the agent at every call).
        NOT carried: the recording table of start_rollout() / rollout() / emit_windows() (rolls, slot): a recorded
        rollout is one episode segment that starts after a reset; finish it before saving.
        A camera env: NotImplementedError."""
        self._state_refusal('SyntheticVecEnv.state_dict')
        ppo = None
        if self._ppo.get('key') is not None:
            ppo = {'key': list(self._ppo['key']), 'carry': dict(self._ppo['carry']), 't': self._ppo.get('t')}
        ddpg = None
        if self._ddpg.get('n_step') is not None:
            ddpg = {k: self._ddpg[k] for k in ('n_step', 'carry_obs', 'carry_act', 'carry_rew', 'ou')}
        sd = {'fingerprint': {'n': self.n, 'D': self.D, 'A': self.A, 'task': self.task, 'episode_len': self.episode_len,
                              'init_state': self.init_state},
              'state': self.state, 't': self.t, 'ppo': ppo, 'ddpg': ddpg}
        for k in self._ATTACHMENTS:
            part = getattr(self, k)
            sd[k] = None if part is None else part.state_dict()
        return sd

    def load_state_dict(self, sd):
        """state_dict()'s, back: `state` in place, the clock, the open windows and transitions; the attachments load
        their own.  ValueError -- before anything is written -- when the fingerprint differs (n, D, A, task,
        episode_len, the bytes of init_state), when something is attached on one side only, or when an attachment
        refuses its state (another stream seed, another monitor capacity, ...).  A camera env: NotImplementedError."""
        who = 'SyntheticVecEnv.load_state_dict'
        self._state_refusal(who)
        fp = sd['fingerprint']
        for k in ('n', 'D', 'A', 'task'):
            if fp[k] != getattr(self, k):
                raise ValueError('%s: the state is of an env with %s = %r, this one has %r' % (who, k, fp[k], getattr(self, k)))
        is_array = lambda v: torch.is_tensor(v) or isinstance(v, np.ndarray)  # noqa: E731
        as_np = lambda v: v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)  # noqa: E731
        lens = fp['episode_len']
        if is_array(lens) != self.per_actor_clocks or not np.array_equal(as_np(lens), self.episode_len):
            raise ValueError('%s: the state is of episode_len %s, this env of %s'
                             % (who, as_np(lens).tolist(), np.asarray(self.episode_len).tolist()))
        init = fp['init_state']
        if tuple(init.shape) != tuple(self.init_state.shape) or not torch.equal(init.to(self.init_state.device), self.init_state):
            raise ValueError('%s: the state is of an env with another init_state (other seeds)' % who)
        for k in self._ATTACHMENTS:
            part = getattr(self, k)
            if (part is None) != (sd.get(k) is None):
                raise ValueError('%s: %s is attached %s' % (who, k, 'to the saved env only' if part is None else
                                                            'to this env only'))
            if part is not None:
                part.check_state_dict(sd[k])
        n = self.n
        if tuple(sd['state'].shape) != tuple(self.state.shape):
            raise ValueError('%s: the saved state is %s' % (who, tuple(sd['state'].shape)))
        t = sd['t']
        if is_array(t) != self.per_actor_clocks or (self.per_actor_clocks and tuple(t.shape) != (n,)):
            raise ValueError('%s: the saved clock does not fit %s' % (who, 'per-actor clocks' if self.per_actor_clocks
                                                                       else 'one shared clock'))
        for part, names in ((sd['ppo'], None), (sd['ddpg'], ('carry_obs', 'carry_act', 'carry_rew', 'ou'))):
            tensors = {} if part is None else part['carry'] if names is None else {k: part[k] for k in names}
            for k, v in tensors.items():
                if not torch.is_tensor(v) or v.shape[0] != n:
                    raise ValueError('%s: the saved %s does not hold %d actors' % (who, k, n))
        # ---- everything fits: write ----
        clock = lambda v: np.array(as_np(v), dtype=np.int32) if is_array(v) else (None if v is None else int(v))  # noqa: E731
        dev = self.device
        self.state.copy_(sd['state'])
        self.t = clock(t)
        if self.per_actor_clocks:
            self._clk = {}                       # (the device copies: made again by the next call)
        self._ppo = {}
        if sd['ppo'] is not None:
            p = sd['ppo']
            self._ppo = {'key': tuple(tuple(v) if isinstance(v, list) else v for v in p['key']),
                         'carry': {k: v.to(dev, copy=True) for k, v in p['carry'].items()}, 't': clock(p['t'])}
        self._ddpg = {}
        if sd['ddpg'] is not None:
            d = sd['ddpg']
            self._ddpg = {'n_step': int(d['n_step']), 'hist': None}
            self._ddpg.update({k: d[k].to(dev, copy=True) for k in ('carry_obs', 'carry_act', 'carry_rew', 'ou')})
        for k in self._ATTACHMENTS:
            if getattr(self, k) is not None:
                getattr(self, k).load_state_dict(sd[k])

    def _clock_walk(self, k):
        """the shared clock at each of the next k steps and after them (k + 1 values): an episode ends at episode_len"""
        ts = [self.t]
        for _ in range(k):
            ts.append(0 if ts[-1] + 1 >= self.episode_len else ts[-1] + 1)
        return ts

    def _advance(self, k=1):
        self.t = self._clock_walk(k)[-1]

    def _closing_steps(self, T, closes):
        """-> (how many of the next T steps close something: closes(clock), the clock after them)"""
        ts = self._clock_walk(T)
        return sum(bool(closes(t)) for t in ts[:-1]), ts[-1]

    def _draws(self, agent, eps, T):
        """-> (the standard-normal draws of T steps, [T, n, A] contiguous: `eps`, by default drawn here in one launch;
        whether the launches draw from the attached stream instead).  (None, False) in the deterministic agent modes;
        (None, True) with a stream attached and no `eps`: the launches get it through _noi"""
        if agent.agent_mode in ('eval_deterministic', 'eval_deterministic_local'):
            return None, False
        if eps is None:
            if self.noise is not None:
                return None, True
            eps = torch.randn(T, self.n, self.A, device=self.device)
        return eps.contiguous(), False

    def _packed(self, attr, numel, pack):
        """the cached buffer `attr` of numel floats, (re)allocated when the size changed and packed again: the agent's
        parameters change between calls"""
        buf = getattr(self, attr, None)
        if buf is None or buf.numel() != numel:
            buf = torch.zeros(numel, device=self.device)
            setattr(self, attr, buf)
        pack(buf)
        return buf

    def _pack_actor(self, actor):
        return self._packed('_pk', self.K.epoch_packed_numel(actor), lambda b: self.K.epoch_pack([(actor, b)]))

    def _pack_lstm(self, rnn):
        return self._packed('_lpk', self.K.lstm_rollout_packed_numel(rnn), lambda b: self.K.lstm_rollout_pack(rnn, b))

    def _cell_outputs(self, Hl):
        """the LSTM launches' hN / cN / h_before / c_before, (1, n, Hl) each, by argument name"""
        return {k: torch.empty(1, self.n, Hl, device=self.device) for k in ('hN', 'cN', 'h_before', 'c_before')}

    @staticmethod
    def _hand_cells(agent, c):
        """leaves _cell_outputs' tensors where act_batch would have: the final (h, c) and the state before the last step"""
        agent._batch_cells = (c['hN'], c['cN'])
        agent.batch_cells_before = (c['h_before'], c['c_before'])

    def _camera_refusal(self, who, agent, camera):
        """the method `who` needs env and agent to agree on the camera -> (exception class, message), or None"""
        if (self.pixel is not None) != camera:
            return NotImplementedError, ('%s: a camera on one side only (env %s, agent %s); both or neither'
                                         % (who, 'camera' if self.pixel else 'low-dimensional',
                                            'camera' if camera else 'low-dimensional'))
        if camera:
            C, H, W = self.pixel
            S = self.frame_stacks
            cam = tuple(int(v) for v in agent.obs_spec['pixel']['camera0'])
            if cam != (S * C, H, W):
                return ValueError, ('%s: the agent\'s camera0 %s is not the env\'s stacked frame %s'
                                    % (who, cam, (S * C, H, W)))
            if agent.model.low_dim != self.D:
                return ValueError, '%s: the agent\'s low_dim %d is not the env\'s %d' % (who, agent.model.low_dim, self.D)
        return None

    def _frame_history(self, c, Hd):
        """the camera paths' frame history in the store dict c: 'hist' [n, Hd, C, H, W] (the current step's frame in
        slot 'hist_pos') and 'obs_pixel', the stacked acting observation; primed on first use and after reset() with the
        current frame in every slot, the observation that frame S times (Hd + 1 launches, once)"""
        K, n, S = self.K, self.n, self.frame_stacks
        C, H, W = self.pixel
        if c.get('hist') is None or tuple(c['hist'].shape) != (n, Hd, C, H, W):
            c['hist'] = torch.zeros((n, Hd, C, H, W), device=self.device, dtype=torch.uint8)
            c['obs_pixel'] = torch.zeros((n, S * C, H, W), device=self.device, dtype=torch.uint8)
            c['hist_pos'] = None
        if c.get('hist_pos') is None:
            for h in range(Hd):
                K.synth_frames(self.state[:, 0], self.t, c['hist'][:, h])
            K.frame_stack(c['hist'], S, 0, 1, 1, 1, c['obs_pixel'])
            c['hist_pos'] = 0

    def start_rollout(self, T, info_width=0):
        """allocate a device rollout of T steps.  Every roll has T + 1 rows per actor (the
        observation roll needs the observation after the last step; the others leave their last
        row unused) so that one env-step launch records all fields.  A rollout is one episode
        segment: it starts right after a reset and T <= episode_len, so `done` can only be set
        on the last recorded step and windows never straddle an episode boundary."""
        self._shared_clock_only('start_rollout')
        self._drift_only('start_rollout')
        assert self.t == 0 and T <= self.episode_len, 'rollouts start at an episode boundary'
        f = lambda *s: torch.zeros(*s, device=self.device, dtype=torch.float32)  # noqa: E731
        self.T = T
        R = T + 1
        self.rolls = {'obs': f(self.n, R, self.D), 'actions': f(self.n, R, self.A),
                      'rewards': f(self.n, R), 'dones': f(self.n, R)}
        if info_width:
            self.rolls['pds'] = f(self.n, R, info_width)
        self.slot = 0
        if self.pixel is not None:
            # raw camera frames, one per step, uint8 [actors, T + 1, C, H, W]; row 0 = the frame after reset
            self.frames = torch.zeros((self.n, R) + self.pixel, device=self.device, dtype=torch.uint8)
            self.K.synth_frames(self.state[:, 0], self.t, self.frames[:, 0])

    def observation(self):
        """what the policies see now: the state [n, D], or with a camera the nested observation
        {'pixel': {'camera0': uint8 [n, frame_stacks * C, H, W]}, 'low_dim': {'flat_inputs': state}}"""
        if self.pixel is None:
            return self.state
        C, H, W = self.pixel
        stacked = torch.empty(self.n, self.frame_stacks * C, H, W, device=self.device, dtype=torch.uint8)
        self.K.frame_stack(self.frames, self.frame_stacks, self.slot, 1, 1, 1, stacked)
        return collections.OrderedDict(pixel=collections.OrderedDict(camera0=stacked),
                                       low_dim=collections.OrderedDict(flat_inputs=self.state))

    def step(self, actions, pds=None):
        """actions [n, A] on the device -> next observation [n, D] (the state tensor)"""
        self._shared_clock_only('step')
        task = self._task_kw('step')
        self._disturbed_ok('step')
        r = self.rolls
        if r is not None and self.slot < self.T:
            self.K.synth_env_step(self.state, self.init_state, actions, self.t, self.episode_len,
                                  self.slot, r['obs'], r['actions'], r['rewards'], r['dones'], **self._mon(1),
                                  **self._noi(1), **task, **self._rst(1))
            if pds is not None and pds.data_ptr() != r['pds'][:, self.slot].data_ptr():
                r['pds'][:, self.slot] = pds         # (an agent may have written the slot in place)
            self.slot += 1
            if self.pixel is not None:
                # the camera frame of the observation AFTER this step (the terminal one when the episode ends here):
                # rendered from the recorded next observation, at the step count it belongs to
                self.K.synth_frames(r['obs'][:, self.slot, 0], self.t + 1, self.frames[:, self.slot])
        else:
            self.K.synth_env_step(self.state, self.init_state, actions, self.t, self.episode_len, 0,
                                  None, None, None, None, **self._mon(1), **self._noi(1), **task, **self._rst(1))
        self._advance()
        return self.state

    def rollout(self, agent, eps=None, actors_per_workgroup=0):
        """A whole recorded rollout (start_rollout(T) first) under `agent`'s plain-MLP policy (an LSTM-stem one:
        _rollout_lstm where the kernel takes it, else _rollout_stem): ONE launch
        (smx_synth_rollout_f32: a workgroup owns 4, 8 or 16 actors through all T steps) where the shapes allow it, else
        THREE launches per environment step (the two hidden layers, then one launch that forms the policy mean,
        samples the action, steps every actor, records the transition and z-filters the next observation).
        Same numbers (1e-6: the layers' fp32 summation order differs between the two) as
        ``for t: agent.act_batch(state) -> step(actions, pds)``.
        eps: [T, n, A] standard-normal draws (default: drawn here in one launch; None-eps agents in
        a deterministic mode ignore it).  actors_per_workgroup: 4 | 8 | 16 forces the one-launch kernel's block (0:
        automatic; 4 and 8 give the same bits, 16 sums the layers in another order)."""
        self._shared_clock_only('rollout')
        self._drift_only('rollout')
        T, n, K = self.T, self.n, self.K
        assert self.slot == 0 and 'pds' in self.rolls, 'start_rollout(T, info_width=2 * A) first'
        eps, ns = self._draws(agent, eps, T)
        if agent.rnn_config.if_rnn_policy or agent.model.if_pixel:
            if self._lstm_persistent(agent):
                return self._rollout_lstm(agent, eps, actors_per_workgroup, ns)
            return self._rollout_stem(agent, eps, ns)
        noise = agent.batch_noise(n).view(-1)
        zf = agent.model.z_filter if agent.use_z_filter else None
        log_var = agent.model.log_var.view(-1)
        actor = agent.model.actor
        plain_mlp = not (agent.rnn_config.if_rnn_policy or agent.model.if_pixel)
        if plain_mlp and self.persistent and K.synth_rollout_supported(actor):
            # ONE launch for the whole rollout: a workgroup owns 4, 8 or 16 actors and walks them through all T steps
            # (csrc/smx_rollout.hip).  The packed weight copy is refreshed here: the agent's parameters only change
            # between rollouts (fetch_parameter)
            K.synth_rollout(actor, self._pack_actor(actor), L.SMX_ACT_TANH, self.state, self.init_state, log_var, noise,
                            eps, self.t, self.episode_len, T, self.slot, self.rolls, zf, actors_per_workgroup,
                            **self._mon(T), **self._noi(T, ns))
            self.slot += T
            self._advance(T)
            return
        if getattr(self, '_xn', None) is None:
            self._xn = torch.empty(n, self.D, device=self.device)
        if zf is not None:
            K.zfilter_forward_sums(self.state, zf.running_sum, zf.running_sumsq, zf.count, zf.eps, self._xn)
        else:
            self._xn.copy_(self.state)
        if plain_mlp and actor.OUT <= 32:
            # THREE launches per environment step: the two hidden layers, then one launch that forms the policy
            # mean (output layer + tanh) per actor, samples, steps, records and z-filters the next observation
            if getattr(self, '_h1', None) is None or self._h1.shape != (n, actor.H1):
                self._h1 = torch.empty(n, actor.H1, device=self.device)
                self._h2 = torch.empty(n, actor.H2, device=self.device)
            v = actor.views
            for t in range(T):
                K.linear(self._xn, 1, v['W1'], 1, v['b1'], self._h1, n, actor.H1, actor.D, act=L.SMX_ACT_RELU)
                K.linear(self._h1, 1, v['W2'], 1, v['b2'], self._h2, n, actor.H2, actor.H1, act=L.SMX_ACT_RELU)
                K.synth_act_env_step_head(v['W3'], v['b3'], self._h2, L.SMX_ACT_TANH, self.state, self.init_state,
                                          log_var, noise, None if eps is None else eps[t], self.t,
                                          self.episode_len, self.slot, self.rolls, zf, self._xn, **self._mon(1),
                                          **self._noi(1, ns))
                self.slot += 1
                self._advance()
            return
        for t in range(T):                     # four launches per step: three policy layers + the step launch
            mean = agent.policy_mean(self._xn)
            K.synth_act_env_step(self.state, self.init_state, mean, log_var, noise,
                                 None if eps is None else eps[t], self.t, self.episode_len, self.slot,
                                 self.rolls, zf, self._xn, **self._mon(1), **self._noi(1, ns))
            self.slot += 1
            self._advance()

    def _lstm_persistent(self, agent):
        """an LSTM-stem policy the one-launch kernel runs: one layer, low-dimensional observations, shapes it takes,
        a kernels object that has the entry point (else _rollout_stem)"""
        return (self.persistent and self.pixel is None and agent.rnn_config.if_rnn_policy and not agent.model.if_pixel
                and getattr(self.K, 'synth_lstm_rollout', None) is not None
                and self.K.synth_lstm_rollout_supported(agent.model))

    def _lstm_launch(self, agent, eps, steps, slot, rolls, actors_per_workgroup, ns=False):
        """the LSTM rollout launch from the zero state (a rollout starts at an episode boundary, as in _rollout_stem);
        leaves the agent's batch cells where act_batch would have: _batch_cells the final (h, c), batch_cells_before the
        state before the last step, each (1, n, Hl)"""
        m = agent.model
        pk, lpk = self._pack_actor(m.actor), self._pack_lstm(m.rnn)
        cells = self._cell_outputs(m.rnn_hidden_logical)
        self.K.synth_lstm_rollout(m, pk, lpk, self.state, self.init_state, agent.batch_noise(self.n).view(-1), eps,
                                  self.t, self.episode_len, steps, slot, rolls,
                                  m.z_filter if agent.use_z_filter else None,
                                  actors_per_workgroup=actors_per_workgroup, **cells, **self._mon(steps),
                                  **self._noi(steps, ns))
        self._hand_cells(agent, cells)
        self._advance(steps)

    def _rollout_lstm(self, agent, eps, actors_per_workgroup=0, ns=False):
        """rollout() for an LSTM-stem policy in ONE launch (smx_synth_lstm_rollout_f32): what _rollout_stem records,
        the cells every actor held before each step included"""
        T, n = self.T, self.n
        if 'cells' not in self.rolls:
            nl, F = agent.rnn_config.rnn_layer, agent.rnn_config.rnn_hidden
            self.rolls['cells'] = torch.zeros(n, T + 1, 2, nl, F, device=self.device)
        self._lstm_launch(agent, eps, T, self.slot, self.rolls, actors_per_workgroup, ns)
        self.slot += T

    def can_rollout_into(self, agent):
        """rollout_into() needs a one-launch kernel: a plain-MLP policy whose shapes it takes, or an LSTM-stem one"""
        if agent.rnn_config.if_rnn_policy:
            return self._lstm_persistent(agent)
        return (self.persistent and self.pixel is None and not agent.model.if_pixel
                and self.K.synth_rollout_supported(agent.model.actor))

    def rollout_into(self, agent, out, eps=None, actors_per_workgroup=0):
        """A whole rollout recorded STRAIGHT INTO a replay's slots (Replay.reserve_batch(n, window_shapes(T)) ->
        `out`: obs [n, T, D], obs_next [n, 1, D], actions [n, T, A], rewards / dones [n, T], pds [n, T, 2A]): with
        stride == n_step == T the moving-window rule (exp_sender_wrapper.py:209-228) makes the one window of an actor
        its rollout, so nothing is cut and nothing is copied -- the one-launch kernel writes the fields where the
        learner will read them.  Starts at an episode boundary (reset() first), like start_rollout().  An LSTM-stem
        policy (window_shapes(T, agent)) also gets `out['cells']` [n, 2, 1, Hl]: the state at the window's first step.
        actors_per_workgroup: as in rollout()."""
        self._shared_clock_only('rollout_into')
        self._drift_only('rollout_into')
        K, n = self.K, self.n
        T = out['obs'].shape[1]
        assert self.t == 0 and T <= self.episode_len and self.can_rollout_into(agent)
        assert tuple(out['obs'].shape) == (n, T, self.D) and all(out[k].is_contiguous() for k in out)
        eps, ns = self._draws(agent, eps, T)
        rolls = {'obs': out['obs'], 'actions': out['actions'], 'rewards': out['rewards'], 'dones': out['dones'],
                 'pds': out['pds'], 'obs_last': out['obs_next']}
        if agent.rnn_config.if_rnn_policy:
            # the window's onetime_infos: the state at its first step -- the zero state a rollout starts from
            out['cells'].zero_()
            self._lstm_launch(agent, eps, T, 0, rolls, actors_per_workgroup, ns)
            return
        actor = agent.model.actor
        K.synth_rollout(actor, self._pack_actor(actor), L.SMX_ACT_TANH, self.state, self.init_state,
                        agent.model.log_var.view(-1), agent.batch_noise(n).view(-1), eps, self.t, self.episode_len, T, 0,
                        rolls, agent.model.z_filter if agent.use_z_filter else None, actors_per_workgroup,
                        **self._mon(T), **self._noi(T, ns))
        self._advance(T)

    def _ppo_window_refusal(self, agent):
        """why ppo_rollout_into cannot take `agent` -> (exception class, message), or None"""
        m = agent.model
        if self.task != 'drift':
            what = ('a camera agent' if m.if_pixel else 'per-actor episode clocks' if self.per_actor_clocks else
                    'rnn_layer %d' % agent.rnn_config.rnn_layer
                    if agent.rnn_config.if_rnn_policy and agent.rnn_config.rnn_layer != 1 else None)
            if what is not None:
                return self._drift_only('ppo_rollout_into', what, throw=False)
        refusal = self._camera_refusal('ppo_rollout_into', agent, bool(m.if_pixel))
        if refusal is not None:
            return refusal
        if m.if_pixel and self.per_actor_clocks:
            return NotImplementedError, ('ppo_rollout_into with a camera: per-actor episode clocks: the one-launch '
                                         'low-dimensional ppo_rollout_into / ddpg_rollout_into only')
        if agent.rnn_config.if_rnn_policy and agent.rnn_config.rnn_layer != 1:
            return NotImplementedError, ('ppo_rollout_into: rnn_layer %d; the windowed rollout runs one LSTM layer'
                                         % agent.rnn_config.rnn_layer)
        if m.if_pixel:
            if getattr(self.K, 'synth_ppo_pixel_window_step', None) is None:
                return NotImplementedError, 'ppo_rollout_into: the kernels object has no synth_ppo_pixel_window_step'
            if not self.K.synth_ppo_pixel_window_step_supported(self.A):
                return ValueError, ('ppo_rollout_into: %d actions; the camera step launch takes A <= %d '
                                    '(SMX_PPO_PIXEL_STEP_MAX_A)' % (self.A, L.SMX_PPO_PIXEL_STEP_MAX_A))
            return None
        if getattr(self.K, 'synth_ppo_window_rollout', None) is None:
            return NotImplementedError, 'ppo_rollout_into: the kernels object has no synth_ppo_window_rollout'
        if not self.K.synth_ppo_window_rollout_supported(m):
            return ValueError, ('ppo_rollout_into: policy shapes the persistent kernel refuses (A <= 32, hidden sizes '
                                'multiples of 4 up to 640, D <= 512, LSTM units up to 128; smx_synth_ppo_window_rollout_'
                                'supported)')
        return None

    def can_ppo_rollout_into(self, agent):
        """ppo_rollout_into() takes `agent`: a plain-MLP or one-layer LSTM policy on low-dimensional observations whose
        shapes the windowed kernel takes, or a camera policy (CNN stem, with or without one LSTM layer) on an env with
        the same camera"""
        return self._ppo_window_refusal(agent) is None

    def ppo_rollout_into(self, agent, replay, T, eps=None, actors_per_workgroup=0):
        """T steps of all actors under PPOAgent `agent` (act: z-filter -> [LSTM ->] policy MLP -> DiagGauss sample ->
        clip, ppo_agent.py:106-154), their moving windows (ExpSenderWrapperMultiStepMovingWindowWithInfo,
        exp_sender_wrapper.py:153-264; n_step / stride of the agent's algo config) written STRAIGHT INTO the FIFO
        replay's device ring (FIFOReplay.reserve_ring / commit_ring) -> the number of windows written.  ONE launch
        (smx_synth_ppo_window_rollout_f32).  Resumes wherever the actors are: the open windows carry from call to call
        (reset() clears them), T may be any length, windows never cross an episode.  An LSTM policy's state comes from
        agent._batch_cells (zeros when None) and is left there after the last step (batch_cells_before: the state
        before it), as act_batch leaves it; it is never reset at episode ends, as in the reference.
        eps [T, n, A] standard normals (default: drawn here in one launch; deterministic agent modes use none);
        actors_per_workgroup: 4 | 8 | 16 forces the kernel's block (0: automatic; every block size gives the same bits).
        A camera agent on a camera env (frame_stacks S) runs step by step instead (_ppo_pixel_steps): the perception of
        the stacked frames (PPOModel.perception_into), one LSTM step, the actor, and ONE launch
        (smx_synth_ppo_pixel_window_step) that samples, steps, keeps the carry rings and a history of n_step + S raw
        frames per actor, and writes the closing windows with their uint8 'pixel' [n_step, S*C, H, W] / 'pixel_next'
        [1, S*C, H, W] into the ring.  The history carries from call to call like the open windows.
        With per-actor episode clocks (low-dimensional only): TWO launches -- the call's row table from the clocks
        (smx_actor_clock_rows_i32), then smx_synth_ppo_window_rollout_clocks_f32; every actor's windows follow its own
        clock and go to the ring in the order n host wrappers stepped in actor order insert them (step by step, actor by
        actor).  The count and the clocks after the call are formed here (env/actor_clocks.py): nothing is read back."""
        refusal = self._ppo_window_refusal(agent)
        if refusal is not None:
            raise refusal[0](refusal[1])
        task = self._task_kw('ppo_rollout_into')
        self._disturbed_ok('ppo_rollout_into')
        T = int(T)
        if T < 1:
            raise ValueError('ppo_rollout_into: T must be positive, got %d' % T)
        from surreal_amd.env.exp_sender_wrapper import window_advance
        K, n, D, A, m = self.K, self.n, self.D, self.A, agent.model
        algo = agent.learner_config.algo
        N, adv = int(algo.n_step), window_advance(algo.n_step, algo.stride)
        rnn = bool(agent.rnn_config.if_rnn_policy)
        Hl = m.rnn_hidden_logical if rnn else 0
        camera = bool(m.if_pixel)
        c = self._ppo
        key = (N, adv, D, A, Hl) + ((self.pixel, self.frame_stacks) if camera else ())
        if c.get('key') != key or c.get('t') is None or not np.array_equal(c['t'], self.t):
            if np.any(self.t != 0):
                raise ValueError('ppo_rollout_into: the open windows of clock %s are not held (the environments were '
                                 'stepped outside ppo_rollout_into, or n_step / stride changed); reset() first' % self.t)
            f = lambda *s: torch.zeros(*s, device=self.device)  # noqa: E731
            c.clear()
            c.update(key=key, carry={'obs': f(n, N, D), 'actions': f(n, N, A), 'rewards': f(n, N), 'pds': f(n, N, 2 * A)})
            if rnn:
                c['carry']['cells'] = f(n, -(-N // adv), 2, Hl)
        if self.per_actor_clocks:
            # every actor closes its own windows: their number and the clocks after the call in closed form
            rows, t = int(AC.closings(self.t, self.episode_len, T, N, adv).sum()), AC.after(self.t, self.episode_len, T)
            if rows > replay.memory_size + 3:
                raise ValueError('ppo_rollout_into: the %d windows %d actors close in %d steps exceed the FIFO capacity '
                                 '%d (two of them would share a row)' % (rows, n, T, replay.memory_size + 3))
        else:
            # the closing steps of this call (the clock is shared by all actors): n windows each
            closing, t = self._closing_steps(T, lambda t: t + 1 - N >= 0 and (t + 1 - N) % adv == 0)
            rows = n * closing
            if rows > replay.memory_size + 3:
                raise ValueError('ppo_rollout_into: %d actors x %d closing steps = %d windows exceed the FIFO capacity '
                                 '%d (two of them would share a row)' % (n, closing, rows, replay.memory_size + 3))
        shapes = {'obs': (N, D), 'obs_next': (1, D), 'actions': (N, A), 'rewards': (N,), 'dones': (N,),
                  'pds': (N, 2 * A)}
        if rnn:
            shapes['cells'] = (2, 1, Hl)
        dtypes = None
        if camera:
            if n > replay.memory_size + 3:      # (the step launch gives every actor a row of its own)
                raise ValueError('ppo_rollout_into: %d actors exceed the FIFO capacity %d' % (n, replay.memory_size + 3))
            C, H, W = self.pixel
            S = self.frame_stacks
            shapes.update(pixel=(N, S * C, H, W), pixel_next=(1, S * C, H, W))
            dtypes = {'pixel': torch.uint8, 'pixel_next': torch.uint8}
        tables, cursor, cap = replay.reserve_ring(rows, shapes, dtypes)
        eps, ns = self._draws(agent, eps, T)
        assert eps is None or tuple(eps.shape) == (T, n, A)
        if camera:
            self._ppo_pixel_steps(agent, T, N, adv, tables, cursor, cap, eps, ns)
            replay.commit_ring(rows)
            c['t'] = self.t
            return rows
        pk, lpk, cells = self._pack_actor(m.actor), None, {}
        zf = m.z_filter if agent.use_z_filter else None
        noise = agent.batch_noise(n).view(-1)
        if rnn:
            lpk = self._pack_lstm(m.rnn)
            held = agent._batch_cells
            cells = self._cell_outputs(Hl)
            if held is not None and held[0].shape[1] == n:
                cells.update(h0=held[0].contiguous(), c0=held[1].contiguous())
        clk, clock = {}, (self.t, self.episode_len)
        if self.per_actor_clocks:
            clk, clock = self._clock_args(T, N, adv, rows), (0, 1)       # (the shared clock's arguments are ignored)
        K.synth_ppo_window_rollout(m, pk, lpk, self.state, self.init_state, noise, eps, clock[0], clock[1], T, N,
                                   adv, c['carry'], tables, cursor, zf, actors_per_workgroup=actors_per_workgroup, **cells,
                                   **self._mon(T), **self._noi(T, ns), **clk, **task, **self._rst(T))
        if rnn:
            self._hand_cells(agent, cells)
        replay.commit_ring(rows)
        self.t = c['t'] = t
        return rows

    def _ppo_pixel_steps(self, agent, T, N, adv, tables, cursor, cap, eps, ns=False):
        """ppo_rollout_into's camera path: per step perception -> [one LSTM step ->] actor -> the record launch.  The
        history (hist [n, N + S, C, H, W], the current step's frame in slot hist_pos) lives with the carry rings in
        self._ppo and is primed with them (first use, after reset()) as _ddpg_pixel_steps primes it; the perception's
        and the LSTM's buffers are cached across steps and calls."""
        K, n, c, m = self.K, self.n, self._ppo, agent.model
        Hd = N + self.frame_stacks
        rnn = bool(m.if_rnn)
        Hp, Hl = (m.rnn_hidden, m.rnn_hidden_logical) if rnn else (0, 0)
        self._frame_history(c, Hd)
        actor, p = m.actor, m.cnn
        key = (n, m.stem_in, p.C, p.H, p.W, p.c1, p.c2, p.feat, Hp, Hl, actor.H1, actor.H2, actor.OUT)
        w = getattr(self, '_ppo_ws', None)
        if w is None or w.key != key:
            f = lambda *s: torch.empty(*s, device=self.device)  # noqa: E731
            w = self._ppo_ws = types.SimpleNamespace(
                key=key, perc=m.perception_workspace(n, self.device), x=f(n, m.stem_in), h1=f(n, actor.H1),
                h2=f(n, actor.H2), mean=f(n, actor.OUT))
            if rnn:
                w.gates, w.out, w.cs = f(n, 4 * Hp), f(n, Hp), f(n, Hp)
                w.hc = [(torch.zeros(n, Hp, device=self.device), torch.zeros(n, Hp, device=self.device))
                        for _ in range(2)]
                w.before = (f(n, Hl), f(n, Hl)) if Hl != Hp else None
        r = dict(state=self.state, init_state=self.init_state, episode_len=self.episode_len, n_step=N, advance=adv,
                 log_var=m.log_var.view(-1), noise_scale=agent.batch_noise(n).view(-1), carry=c['carry'], tables=tables,
                 cursor=cursor, hist=c['hist'], obs_pixel=c['obs_pixel'])
        cur = 0
        if rnn:
            # the state the agent holds (zeros when none) into the padded buffers; a padded unit stays exactly zero
            # (its weights are zeros, PPOModel.__init__)
            cells = agent._batch_cells
            for buf, src in zip(w.hc[0], cells if cells is not None and cells[0].shape[1] == n else (None, None)):
                buf.zero_()
                if src is not None:
                    buf[:, :Hl].copy_(src.reshape(n, Hl))
        for s in range(T):
            m.perception_into(c['obs_pixel'], self.state, w.perc, w.x)
            feat = w.x
            if rnn:
                (h, cc), (hn, cn) = w.hc[cur], w.hc[1 - cur]
                K.lstm_forward(m.rnn, w.x, n, 1, h, cc, w.gates, w.out, w.cs, None, hn, cn)
                if w.before is not None:                       # (the step launch reads [n, Hl] rows)
                    w.before[0].copy_(h[:, :Hl])
                    w.before[1].copy_(cc[:, :Hl])
                    r['h_before'], r['c_before'] = w.before
                else:
                    r['h_before'], r['c_before'] = h, cc
                cur = 1 - cur
                feat = w.out
            K.mlp3_forward(actor, feat, w.h1, w.h2, w.mean, L.SMX_ACT_TANH)
            r['t'], r['hist_pos'] = self.t, c['hist_pos']
            r['eps'] = None if eps is None else eps[s]
            K.synth_ppo_pixel_window_step(r, w.mean, **self._mon(1), **self._noi(1, ns))
            c['hist_pos'] = (c['hist_pos'] + 1) % Hd
            j = self.t + 1 - N
            if j >= 0 and j % adv == 0:
                r['cursor'] = (r['cursor'] + n) % cap
            self._advance()
        if rnn:
            # as act_batch leaves them: the final state and the state before the last step, (1, n, Hl) each, the
            # agent's own tensors (the buffers here are written again by the next call)
            own = lambda x: x[:, :Hl].clone().view(1, n, Hl)  # noqa: E731
            agent._batch_cells = tuple(own(x) for x in w.hc[cur])
            agent.batch_cells_before = tuple(own(x) for x in w.hc[1 - cur])

    def _ddpg_route(self, agent, reference):
        """how ddpg_rollout_into runs `agent` -> (route, refusal): 'camera' (the per-step camera path), 'launch' (ONE
        launch), 'two_launch' (the persistent kernel's two-launch reference) or 'steps' (forward_actor and a step launch
        per step); refusal (exception class, message) or None.  A LayerNorm actor takes the launch where the kernels run
        one (kernels.ddpg_ln_launch); else it stays on the per-step path, refused under a parameter noise.  On a task
        env only the 'launch' route runs: the plain actor, and a LayerNorm actor or an attached parameter noise where the
        kernels run them there (kernels.ddpg_variant_task_launch)."""
        K, model, pn = self.K, agent.model, self.param_noise
        camera = model.is_pixel_input
        if self.task != 'drift':
            ln = not camera and bool(model.use_layernorm)
            variants = not camera and KN.ddpg_variant_task_launch(K) and (not ln or KN.ddpg_ln_launch(K))
            what = ('a camera agent' if camera else 'a LayerNorm actor' if ln and not variants else
                    'an attached parameter noise' if pn is not None and not variants else
                    'per-actor episode clocks' if self.per_actor_clocks else
                    "reference=True (the 'two_launch' route)" if reference else
                    "an actor shape the one-launch rollout does not take (the 'steps' route)"
                    if not K.synth_ddpg_rollout_supported(model.actor, **(dict(ln=True) if ln and variants else {}))
                    else None)
            if what is not None:
                return None, self._drift_only('ddpg_rollout_into', what, throw=False)
        refusal = self._camera_refusal('ddpg_rollout_into', agent, camera)
        if refusal is not None:
            return None, refusal
        ln = bool(model.use_layernorm)
        ln_launch = ln and not camera and KN.ddpg_ln_launch(K)
        # the launch takes the actor: its kind, then its shapes (kernels that run no LayerNorm are not asked about one)
        supported = not camera and (ln_launch or not ln) and K.synth_ddpg_rollout_supported(
            model.actor, **(dict(ln=True) if ln_launch else {}))
        refuse = lambda cls, why: (None, (cls, 'ddpg_rollout_into: ' + why))  # noqa: E731
        if pn is not None:
            why = ('a camera agent (the perception would need perturbing too)' if camera else
                   'a LayerNorm actor' if ln and not (ln_launch and pn.ln) else
                   'an actor shape the one-launch rollout does not take' if not supported else
                   'reference=True (the two-launch reference has one actor)' if reference else None)
            if why is not None:
                return refuse(NotImplementedError, 'no device parameter noise for ' + why)
            if agent is not pn.agent:
                return refuse(ValueError, 'the attached parameter noise belongs to another agent')
        elif agent.param_noise_type == 'adaptive_normal':
            return refuse(NotImplementedError, "'adaptive_normal' parameter noise measures an action distance per act() "
                          "on the host; use 'normal' parameter noise, none, or attach_param_noise")
        if camera and reference:
            return refuse(ValueError, 'reference=True has no camera path (no two-launch reference there)')
        route = 'camera' if camera else 'launch' if supported and not reference else \
            'two_launch' if reference and not ln else 'steps'
        if self.per_actor_clocks and route != 'launch':
            return refuse(NotImplementedError, "the '%s' route: per-actor episode clocks: the one-launch "
                          'low-dimensional ppo_rollout_into / ddpg_rollout_into only' % route)
        return route, None

    def ddpg_rollout_into(self, agent, replay, T, eps=None, sigmas=None, actors_per_workgroup=0, reference=False):
        """T steps of all actors under DDPGAgent `agent` (act: actor -> clip -> exploration noise -> clip,
        ddpg_agent.py:155-184), their n-step transitions (ExpSenderWrapperSSARNStepBootstrap, exp_sender_wrapper.py:72-112)
        written STRAIGHT INTO the uniform replay's device ring (reserve_ring / commit_ring) -> the number of rows written.
        Rollouts need not start at an episode boundary: the open transitions and the OU states carry from call to call
        (reset() clears them).  eps [T, n, A] standard normals (default: drawn here in one launch); sigmas [n] fp64
        (default agent.batch_sigmas(n)); actors_per_workgroup: 4 | 8 | 16 forces the persistent kernel's block (0:
        automatic).  _ddpg_route decides among:
        ONE launch (smx_synth_ddpg_rollout_f32) where the actor's shapes allow it: a plain actor or, its gains and biases
        in the launch's actor variant, a LayerNorm one.  With a DeviceParamNoise attached (attach_param_noise) the variant
        also holds the population: every agent's actors act from their agent's perturbed copy; with 'adaptive_normal' the
        call's last step s with (acts + s) % compute_dist_interval == 0 also measures each agent's action distance;
        acts += T.  Other shapes: per step one actor forward (DDPGModel.forward_actor) and one step launch
        (smx_synth_ddpg_step_f32).  reference=True: the two-launch reference of the persistent kernel
        (smx_epoch_forward_f32 for the actor, then the step launch) -- for parity tests, not the product loop; with a
        LayerNorm actor: the per-step path.
        A camera agent on a camera env (frame_stacks S): per step the perception (DDPGModel.perception_into) of the
        stacked frames, the actor, and ONE launch (smx_synth_ddpg_pixel_step) that also renders the step's frame into
        a history of n_step + S raw frames per actor, writes the closing transitions' uint8 'pixel' / 'pixel_next'
        [S*C, H, W] into the ring and the stacked observation of the next step.  The history carries from call to call
        like the open transitions.  Into a frame-pool replay (replay.device_frame_pool; replay/frame_pool.py) the launch
        is smx_synth_ddpg_pixel_pool_step: the step's frame goes ONCE into the replay's pool, which is the history as
        well, and the closing rows carry two counters in place of the stacked frames; such a call may go round the ring.
        With per-actor episode clocks (the ONE-launch route only): the call's row table from the clocks
        (smx_actor_clock_rows_i32), then smx_synth_ddpg_rollout_clocks_f32 -- as in ppo_rollout_into.
        On a task env (the ONE-launch route on the shared clock only): the plain actor (smx_synth_ddpg_rollout_task_f32 /
        _resets_f32) and, where the kernels run them there (kernels.ddpg_variant_task_launch), a LayerNorm actor and an
        attached parameter noise (smx_synth_ddpg_rollout_variant_task_f32) -- variant, task and reset stream in one call."""
        route, refusal = self._ddpg_route(agent, reference)
        if refusal is not None:
            raise refusal[0](refusal[1])
        K, n, A, pn = self.K, self.n, self.A, self.param_noise
        task = self._task_kw('ddpg_rollout_into')
        self._disturbed_ok('ddpg_rollout_into')
        shapes, dtypes = {'obs': (self.D,), 'obs_next': (self.D,), 'actions': (A,), 'rewards': (), 'dones': ()}, None
        # (a frame-pool replay, replay.device_frame_pool: the camera rows are counters into its pool, which is this
        # route's frame history as well)
        pool = route == 'camera' and bool(getattr(replay, 'frame_pool_on', False))
        if route == 'camera' and not pool:
            (C, H, W), S = self.pixel, self.frame_stacks
            shapes.update(pixel=(S * C, H, W), pixel_next=(S * C, H, W))
            dtypes = {'pixel': torch.uint8, 'pixel_next': torch.uint8}
        algo = agent.learner_config.algo
        N, gamma = int(algo.n_step), algo.gamma
        T = int(T)
        if self.per_actor_clocks:
            # every actor closes its own transitions: their number and the clocks after the call in closed form
            rows, t = int(AC.closings(self.t, self.episode_len, T, N, 1).sum()), AC.after(self.t, self.episode_len, T)
            if rows > replay.memory_size:
                raise ValueError('ddpg_rollout_into: the %d transitions %d actors close in %d steps exceed the replay '
                                 'capacity %d (two of them would share a row)' % (rows, n, T, replay.memory_size))
        else:
            # the closing steps of this call (the clock is shared by all actors): n of them per closing step
            m, t = self._closing_steps(T, lambda t: t >= N - 1)
            rows = n * m
            # (the frame-pool route is a launch per step, n rows each: a call may go round the ring)
            if rows > replay.memory_size and not (pool and n <= replay.memory_size):
                raise ValueError('ddpg_rollout_into: %d actors x %d closing steps = %d transitions exceed the replay '
                                 'capacity %d (two of them would share a row)' % (n, m, rows, replay.memory_size))
        if pool:
            plan = self._frame_pool_plan(replay, T, N)
            handle = replay.reserve_frame_pool(plan['steps'], shapes, n, self.pixel, self.frame_stacks, N)
            tables, cursor, cap = handle['tables'], handle['cursor'], handle['capacity']
        else:
            tables, cursor, cap = replay.reserve_ring(rows, shapes, dtypes)
        d = self._ddpg
        if d.get('n_step') != N:
            f = lambda *s: torch.zeros(*s, device=self.device)  # noqa: E731
            d.update(n_step=N, carry_obs=f(n, N, self.D), carry_act=f(n, N, A), carry_rew=f(n, N),
                     ou=torch.zeros(n, A, device=self.device, dtype=torch.float64), hist=None)
        if d.get('gamma') != gamma:
            d['gamma'] = gamma
            d['gpow'] = torch.tensor([pow(gamma, e) for e in range(N)], dtype=torch.float64, device=self.device)
        eps, ns = self._draws(agent, eps, T)
        deterministic = eps is None and not ns
        noise = L.SMX_DDPG_NOISE_NONE if deterministic else \
            {'normal': L.SMX_DDPG_NOISE_GAUSSIAN, 'ou_noise': L.SMX_DDPG_NOISE_OU}[agent.noise_type]
        if not deterministic:
            if sigmas is None:
                sigmas = agent.batch_sigmas(n)
            assert eps is None or tuple(eps.shape) == (T, n, A)
            assert sigmas.dtype == torch.float64 and sigmas.numel() == n
            sigmas = sigmas.contiguous()
        shared = (0, 1) if self.per_actor_clocks else (self.t, self.episode_len)       # (ignored with per-actor clocks)
        r = dict(state=self.state, init_state=self.init_state, t=shared[0], episode_len=shared[1], n_step=N,
                 noise_type=noise, eps=eps, sigmas=None if deterministic else sigmas,
                 theta=agent.theta, dt=agent.dt, root_dt=float(np.sqrt(agent.dt)), gpow=d['gpow'], ou=d['ou'],
                 carry_obs=d['carry_obs'], carry_act=d['carry_act'], carry_rew=d['carry_rew'], tables=tables,
                 cursor=cursor)
        actor, model = agent.model.actor, agent.model
        if route in ('launch', 'two_launch'):
            if d.get('pk') is None or d['pk'].numel() != K.epoch_packed_numel(actor):
                d['pk'] = torch.zeros(K.epoch_packed_numel(actor), device=self.device)
            K.epoch_pack([(actor, d['pk'])])        # (the agent's parameters only change between rollouts)
        if pool:
            self._ddpg_pixel_steps(agent, r, T, N, cap, eps, ns, pool=(replay, handle, plan))
            replay.commit_frame_pool(rows, plan['frames'][-1][0])
            return rows
        if route == 'camera':
            self._ddpg_pixel_steps(agent, r, T, N, cap, eps, ns)
        elif route == 'launch':
            variant = dict(ln=model.actor_ln_flat, ln_eps=model.ln_eps) if model.use_layernorm else {}    # (plain: none)
            if pn is not None:
                variant.update(pn=pn, measure_step=pn.measure_step(T))
            if self.per_actor_clocks:
                variant.update(self._clock_args(T, N, 1, rows))
            K.synth_ddpg_rollout(actor, d['pk'], r, T, actors_per_workgroup, **variant, **self._mon(T),
                                 **self._noi(T, ns), **task, **self._rst(T))
            if pn is not None:
                pn.acts += T
            self.t = t
        else:
            if route == 'two_launch':
                mu = torch.empty(n, A, device=self.device)
                ctrl = torch.zeros(L.CTRL_WORDS, device=self.device)
            for s in range(T):
                if route == 'two_launch':
                    K.epoch_forward([dict(net=actor, packed=d['pk'], x=self.state, out=mu, act=L.SMX_ACT_TANH)],
                                    None, ctrl, n)
                else:
                    mu = model.forward_actor(self.state)
                r['t'] = self.t
                r['eps'] = None if eps is None else eps[s]
                K.synth_ddpg_step(r, mu, **self._mon(1), **self._noi(1, ns))
                if self.t >= N - 1:
                    r['cursor'] = (r['cursor'] + n) % cap
                self._advance()
        replay.commit_ring(rows)
        return rows

    def _eval_refusal(self, agent, population=False):
        """why the evaluation launch cannot take `agent`'s policy on this env -> (exception class, message), or None
        (population: the parameter sets are the attached noise's own perturbed actors, so the noise is no obstacle)"""
        m = agent.model
        ppo = hasattr(agent, 'rnn_config')
        camera = bool(m.if_pixel if ppo else m.is_pixel_input)
        only = ('the evaluation launch runs a plain-MLP or one-layer LSTM PPO policy or a plain DDPG actor on '
                'low-dimensional observations, on one shared clock, only')
        what = ('a camera env' if self.pixel is not None else 'a camera agent' if camera else
                'per-actor episode clocks' if self.per_actor_clocks else
                'rnn_layer %d' % agent.rnn_config.rnn_layer
                if ppo and agent.rnn_config.if_rnn_policy and agent.rnn_config.rnn_layer != 1 else
                'a LayerNorm actor' if not ppo and m.use_layernorm else
                'an attached parameter noise' if not ppo and self.param_noise is not None and not population else None)
        if what is not None:
            return NotImplementedError, 'evaluate with %s: %s' % (what, only)
        if getattr(self.K, 'synth_ppo_eval' if ppo else 'synth_ddpg_eval', None) is None:
            return NotImplementedError, 'evaluate: the kernels object has no %s' % ('synth_ppo_eval' if ppo else
                                                                                    'synth_ddpg_eval')
        if not (self.K.synth_eval_supported(self.task, model=m) if ppo else
                self.K.synth_eval_supported(self.task, actor=m.actor)):
            return NotImplementedError, ('evaluate: shapes the evaluation launch refuses (A <= 32, hidden sizes multiples '
                                         'of 4 up to 640, D <= 512, LSTM units up to 128; task %r: action_dim <= %d; '
                                         'smx_synth_eval_supported)' % (self.task, TK.MAX_A[self.task] or TK.REACH_MAX_A))
        return None

    def can_evaluate(self, agent):
        """evaluate() takes `agent`'s policy: a plain-MLP or one-layer LSTM PPO policy, or a plain DDPG actor (no
        LayerNorm, no attached parameter noise), on low-dimensional observations, whose shapes the launch takes, on an
        env with one shared clock and no camera"""
        return self._eval_refusal(agent) is None

    @staticmethod
    def _eval_stream(who, what, value, n):
        """(seed, counter[, actor_base]) of evaluate()'s resets= / noise= -> the launches' (seed, actor_base, counter)"""
        v = tuple(int(x) for x in value)
        if len(v) not in (2, 3):
            raise ValueError('%s: %s must be (seed, %s[, actor_base]), got %r' % (who, what[0], what[1], value))
        seed, first, base = v[0], v[1], (v[2] if len(v) == 3 else 0)
        if not 0 <= seed < 1 << 64:
            raise ValueError('%s: the seed of %s must fit 64 bits, got %r' % (who, what[0], seed))
        if first < 0:
            raise ValueError('%s: %s %d is negative' % (who, what[1], first))
        if base < 0 or base + n > 1 << 32:
            raise ValueError('%s: global actor ids %d .. %d leave [0, 2^32)' % (who, base, base + n - 1))
        return (seed, base, first)

    def evaluate(self, agent, episodes=1, resets=None, noise=None, out=None, actors_per_workgroup=0, disturbance=None):
        """`episodes` whole episodes of every actor under `agent`'s policy in ONE launch, nothing recorded -> their
        returns, torch.float64 [n, episodes] on the device (`out`, or a new tensor); no synchronisation.  The device form
        of the reference's evaluation workers (agent_mode eval_deterministic / eval_stochastic, surreal/agent/base.py:
        277-345) and of surreal/main/rollout.py (smx_synth_ppo_eval_f32 / smx_synth_ddpg_eval_f32).
        The (actor, episode) pairs are independent rows of the launch: n * episodes rows walk episode_len steps each.
        resets: None -- every episode begins at init_state[a] -- or (seed, first_episode[, actor_base]), tasks 'reach'
        and 'arm' only: episode i of actor a begins with tasks.reach_reset_state(seed, actor_base + a, first_episode + i,
        J), on 'arm' arm_reset_state's, drawn inside the launch.
        disturbance: None or 0 -- undisturbed steps -- or a scale s in (0, 1], which requires resets=: step t of that
        episode adds s * tasks.disturbance(seed, actor_base + a, first_episode + i, t, J) as a recording launch on the
        stream does (attach_resets), so the return is the one the monitor records for that (seed, actor, episode, scale).
        The mode is the agent's: 'eval_deterministic[_local]' acts on the policy's mean (noise must be None);
        'eval_stochastic[_local]', PPO only, samples -- noise = (seed, first_step[, actor_base]) is required, and step t
        of episode i of actor a draws normal(seed, actor_base + a, first_step + i * episode_len + t, j): what a serial
        run of the actor's episodes on that noise stream draws; 'training': ValueError.  An LSTM policy starts every
        episode from the zero state.
        Pure: neither state, the clock, the attached streams' counters, the monitor, the open windows and transitions,
        agent._batch_cells nor any replay is read or written -- it can be called on the training env between chunks.
        actors_per_workgroup: 4 | 8 | 16 forces the kernel's block of rows (0: automatic; every size gives the same bits)."""
        ppo, E, resets, noise = self._eval_check(agent, episodes, resets, noise, disturbance=disturbance)
        n, L_ = self.n, int(self.episode_len)
        if out is None:
            out = torch.empty(n, E, dtype=torch.float64, device=self.device)
        elif out.dtype != torch.float64 or tuple(out.shape) != (n, E) or not out.is_contiguous():
            raise ValueError('evaluate: out must be a contiguous torch.float64 [%d, %d] tensor' % (n, E))
        m = agent.model
        kw = dict(task=self.task, resets=resets, actors_per_workgroup=actors_per_workgroup)
        # (packed copies of its own: the rollouts' stay as they are)
        pk = self._packed('_epk', self.K.epoch_packed_numel(m.actor), lambda b: self.K.epoch_pack([(m.actor, b)]))
        if not ppo:
            self.K.synth_ddpg_eval(m.actor, pk, self.init_state, E, L_, out, **kw)
            return out
        lpk = None
        if agent.rnn_config.if_rnn_policy:
            lpk = self._packed('_elpk', self.K.lstm_rollout_packed_numel(m.rnn), lambda b: self.K.lstm_rollout_pack(m.rnn, b))
        self.K.synth_ppo_eval(m, pk, lpk, self.init_state, E, L_, out, zfilter=m.z_filter if agent.use_z_filter else None,
                              noise=noise, **kw)
        return out

    def _eval_check(self, agent, episodes, resets, noise, population=False, sets=1, disturbance=None):
        """evaluate()'s refusals, mode rule and checks of episodes / resets= / noise= / the sizes, before anything is
        allocated or launched -> (ppo, episodes, resets, noise), the streams as the launches take them (seed, actor_base,
        counter).  population: _eval_refusal's, and the agent's mode is not asked (the perturbed actors act on their
        means); sets: the parameter sets of the launch (DeviceEvalSnapshots); disturbance: evaluate()'s -- a scale != 0
        makes resets (seed, actor_base, first_episode, scale)"""
        refusal = self._eval_refusal(agent, population)
        if refusal is not None:
            raise refusal[0](refusal[1])
        ppo = hasattr(agent, 'rnn_config')
        mode = 'eval_deterministic' if population else agent.agent_mode
        if mode not in ('eval_deterministic', 'eval_deterministic_local', 'eval_stochastic', 'eval_stochastic_local'):
            raise ValueError('evaluate: agent_mode %r; an evaluation agent (eval_deterministic[_local] / '
                             'eval_stochastic[_local])' % (mode,))
        stochastic = mode in ('eval_stochastic', 'eval_stochastic_local')
        if stochastic and not ppo:
            raise NotImplementedError('evaluate with a DDPG agent in %r: the evaluation launch runs a DDPG actor without '
                                      'exploration noise (eval_deterministic[_local]), only' % (mode,))
        if stochastic and noise is None:
            raise ValueError('evaluate: agent_mode %r samples: noise=(seed, first_step[, actor_base]) is required' % (mode,))
        if not stochastic and noise is not None:
            raise ValueError('evaluate: agent_mode %r draws nothing: noise must be None' % (mode,))
        E, n = int(episodes), self.n
        if E < 1:
            raise ValueError('evaluate: episodes must be positive, got %r' % (episodes,))
        if resets is not None:
            if self.task == 'drift':
                raise ValueError("evaluate: task %r has no reset distribution (resets=: task 'reach')" % (self.task,))
            resets = self._eval_stream('evaluate', ('resets', 'first_episode'), resets, n)
        if disturbance is not None:
            scale = float(TK.check_disturbance('evaluate', disturbance))
            if scale != 0:
                if self.task == 'drift':
                    raise ValueError("evaluate: task %r takes no disturbance (tasks 'reach' and 'arm' do)" % (self.task,))
                if resets is None:
                    raise ValueError('evaluate: a disturbance is drawn from the reset stream: resets=(seed, first_episode'
                                     '[, actor_base]) is required')
                if resets[2] + E > 1 << 32:
                    raise ValueError('evaluate: disturbed episodes %d .. %d leave [0, 2^32)' % (resets[2], resets[2] + E - 1))
                resets = resets + (scale,)
        if noise is not None:
            noise = self._eval_stream('evaluate', ('noise', 'first_step'), noise, n)
        L_ = int(self.episode_len)
        if n * E >= 1 << 31 or E * L_ >= 1 << 31:
            raise ValueError('evaluate: %d actors x %d episodes x %d steps: n * episodes and episodes * episode_len must '
                             'stay below 2^31' % (n, E, L_))
        if int(sets) * n * E >= 1 << 31:
            raise ValueError('evaluate: %d sets x %d actors x %d episodes must stay below 2^31' % (sets, n, E))
        return ppo, E, resets, noise

    def eval_snapshots(self, agent, capacity):
        """-> DeviceEvalSnapshots(self, agent, capacity): `capacity` parameter snapshots of `agent`'s architecture, all
        evaluated on the same episodes in ONE launch"""
        from .monitor import DeviceEvalSnapshots
        return DeviceEvalSnapshots(self, agent, capacity)

    def _frame_pool_plan(self, replay, T, N):
        """the next T steps of the shared clock in a replay's frame pool -> {'frames': [(f, first)] before each step and
        after the last: the counter of the current frame and of the episode's reset frame; 'steps': what
        reserve_frame_pool takes; 'prime': whether the current frame must be written first (first use of this replay,
        after reset())}.  A step writes the frame f + 1, a terminal one also the new episode's first, f + 2"""
        from surreal_amd.replay.frame_pool import oldest_frame
        d, S, fp = self._ddpg, self.frame_stacks, replay.frame_pool
        f = int(fp['counter'][0]) if fp is not None else -1
        prime = d.get('pool_replay') is not replay
        steps, frames = [], []
        if prime:
            f += 1                               # (the current frame: the oldest one any stack of this episode reaches)
            steps.append((0, f, f))
        first = f if prime else d['pool_first']
        for tau in self._clock_walk(T)[:-1]:
            frames.append((f, first))
            done = tau + 1 >= self.episode_len
            oldest = int(oldest_frame(f + 1, first, N, S))
            f += 2 if done else 1
            steps.append((self.n if tau >= N - 1 else 0, f, oldest))
            first = f if done else first
        frames.append((f, first))
        return dict(frames=frames, steps=steps, prime=prime)

    def _ddpg_pixel_steps(self, agent, r, T, N, cap, eps, ns=False, pool=None):
        """ddpg_rollout_into's camera path: per step perception -> actor -> smx_synth_ddpg_pixel_step.  The history
        (hist [n, N + S, C, H, W], the current step's frame in slot hist_pos) is primed on first use and after reset():
        the current frame in every slot, the actors' first observation that frame S times (N + S + 1 launches, once).
        pool = (replay, reserve_frame_pool's handle, _frame_pool_plan's plan): the frame-pool layout
        (smx_synth_ddpg_pixel_pool_step) -- the history is the replay's pool, primed with the current frame alone"""
        from surreal_amd.model.cnn_stem import CnnStem
        K, n, d, model = self.K, self.n, self._ddpg, agent.model
        if pool is None:
            Hd = N + self.frame_stacks
            d['pool_replay'] = None
            self._frame_history(d, Hd)
        else:
            replay, handle, plan = pool
            (C, H, W), S = self.pixel, self.frame_stacks
            if d.get('obs_pixel') is None or tuple(d['obs_pixel'].shape) != (n, S * C, H, W):
                d['obs_pixel'] = torch.zeros((n, S * C, H, W), device=self.device, dtype=torch.uint8)
            if plan['prime']:
                f0 = plan['frames'][0][0]
                slot = handle['pool'].view(n, -1, C, H, W)[:, f0 % handle['pool'].shape[1]]
                K.synth_frames(self.state[:, 0], self.t, slot)
                d['obs_pixel'].copy_(slot.repeat(1, S, 1, 1))
                d['pool_replay'], d['pool_first'], d['hist_pos'] = replay, f0, None
            r.update({k: handle[k] for k in ('pool', 'frame_next', 'frame_first', 'frame_actor')},
                     frame_shape=self.pixel)
        p = model.cnn
        key = (n, model.input_dim, p.C, p.H, p.W, p.c1, p.c2, p.feat)
        if d.get('perc_key') != key:        # the perception's workspace, cached across steps and calls
            d['perc_key'] = key
            d['cnn_ws'] = CnnStem.workspace(model.cnn, n, self.device, backward=False)
            d['x'] = torch.empty(n, model.input_dim, device=self.device)
        r.update(obs_pixel=d['obs_pixel'], **({} if pool else dict(hist=d['hist'])))
        for s in range(T):
            model.perception_into(d['obs_pixel'], self.state, d['cnn_ws'], d['x'])
            mu = model.forward_actor(d['x'])
            r['t'] = self.t
            r['eps'] = None if eps is None else eps[s]
            if pool:
                r['frame'], r['episode_first'] = plan['frames'][s]
                K.synth_ddpg_pixel_pool_step(r, mu, **self._mon(1), **self._noi(1, ns))
                d['pool_first'] = plan['frames'][s + 1][1]
            else:
                r['hist_pos'] = d['hist_pos']
                K.synth_ddpg_pixel_step(r, mu, **self._mon(1), **self._noi(1, ns))
                d['hist_pos'] = (d['hist_pos'] + 1) % Hd
            if self.t >= N - 1:
                r['cursor'] = (r['cursor'] + n) % cap
            self._advance()

    def _rollout_stem(self, agent, eps, ns=False):
        """policies with an LSTM and / or CNN stem: one batched act per step (PPOAgent.act_batch: the stem and the
        MLP for all actors at once) on the stacked observation, then the step launch; the LSTM state every actor
        held BEFORE each step is recorded (what the window that starts there carries as onetime_infos,
        ppo_agent.py:133-135)"""
        T, n = self.T, self.n
        rnn = agent.rnn_config.if_rnn_policy
        agent.reset_batch()                      # a rollout starts at an episode boundary: zero state
        if rnn and 'cells' not in self.rolls:
            nl, F = agent.rnn_config.rnn_layer, agent.rnn_config.rnn_hidden
            self.rolls['cells'] = torch.zeros(n, T + 1, 2, nl, F, device=self.device)
        for t in range(T):
            # (act_batch forms the sample, not one of the step launches: with a stream, its draws for this step from the
            # fill kernel -- the numbers a launch would have formed; step() below moves the stream's clock)
            e = self.noise.draws(1)[0] if ns else (None if eps is None else eps[t])
            a, pd = agent.act_batch(self.observation(), eps=e, out_pd=self.rolls['pds'][:, self.slot])
            if rnn:
                h, c = agent.batch_cells_before                   # (layers, n, hidden) each
                self.rolls['cells'][:, self.slot, 0].copy_(h.permute(1, 0, 2))
                self.rolls['cells'][:, self.slot, 1].copy_(c.permute(1, 0, 2))
            self.step(a, pds=pd)

    def rollout_reference(self, agent, eps):
        """the same rollout with TWO launches per step out of the kernels the persistent one is built from: the
        row-block forward (smx_epoch_forward_f32: the means) and the head + step launch.  Bit-identical to
        ``rollout`` on the persistent kernel -- the parity test's reference; not used by the product loop."""
        self._shared_clock_only('rollout_reference')
        self._drift_only('rollout_reference')
        T, n, K = self.T, self.n, self.K
        actor = agent.model.actor
        noise = agent.batch_noise(n).view(-1)
        zf = agent.model.z_filter if agent.use_z_filter else None
        xn = torch.empty(n, self.D, device=self.device)
        mean = torch.empty(n, actor.OUT, device=self.device)
        pk = torch.zeros(K.epoch_packed_numel(actor), device=self.device)
        K.epoch_pack([(actor, pk)])
        if zf is not None:
            K.zfilter_forward_sums(self.state, zf.running_sum, zf.running_sumsq, zf.count, zf.eps, xn)
        else:
            xn.copy_(self.state)
        ctrl = torch.zeros(L.CTRL_WORDS, device=self.device)
        for t in range(T):
            K.epoch_forward([dict(net=actor, packed=pk, x=xn, out=mean, act=L.SMX_ACT_TANH)], None, ctrl, n)
            K.synth_act_env_step(self.state, self.init_state, mean, agent.model.log_var.view(-1), noise,
                                 None if eps is None else eps[t], self.t, self.episode_len, self.slot, self.rolls, zf, xn,
                                 **self._mon(1), **self._noi(1))
            self.slot += 1
            self._advance()

    def window_shapes(self, n_step, agent=None):
        """per-experience shape of every field emit_windows produces (for Replay.reserve_batch); with a recurrent
        `agent` also its onetime_infos, 'cells' (2, rnn_layer, rnn_hidden)"""
        shp = {'obs': (n_step, self.D), 'obs_next': (1, self.D), 'actions': (n_step, self.A),
               'rewards': (n_step,), 'dones': (n_step,)}
        if self.rolls is not None and 'pds' in self.rolls:
            shp['pds'] = (n_step, self.rolls['pds'].shape[2])
        if self.pixel is not None:
            C, H, Wd = self.pixel
            shp['pixel'] = (n_step, self.frame_stacks * C, H, Wd)
            shp['pixel_next'] = (1, self.frame_stacks * C, H, Wd)
        if agent is not None and agent.rnn_config.if_rnn_policy:
            shp['cells'] = (2, agent.rnn_config.rnn_layer, agent.rnn_config.rnn_hidden)
        return shp

    def emit_windows(self, n_step, stride, out=None):
        """-> dict of [n*W, n_step, .] sub-trajectories (+ obs_next [n*W, 1, D]) cut from the
        recorded rollout with the reference's moving-window rule (exp_sender_wrapper.py:209-228), the
        same index arithmetic as the host wrapper (env/exp_sender_wrapper.py): window w = steps
        [w * advance, w * advance + n_step), W = windows_per_episode(T, n_step, stride) per actor"""
        from surreal_amd.env.exp_sender_wrapper import window_advance, windows_per_episode
        self._shared_clock_only('emit_windows')
        self._drift_only('emit_windows')
        T = self.T
        assert self.slot == T, 'rollout not complete'
        W = windows_per_episode(T, n_step, stride)
        stride = window_advance(n_step, stride)
        r, K, n = self.rolls, self.K, self.n
        f = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)  # noqa: E731
        if out is not None:
            # the caller's buffers (e.g. the replay table's next n*W rows: no copy on insert)
            out = dict(out)
            assert out['obs'].shape == (n * W, n_step, self.D) and all(t.is_contiguous() for t in out.values())
            out['rewards'] = out['rewards'].view(n * W, n_step, 1)
            out['dones'] = out['dones'].view(n * W, n_step, 1)
        else:
            out = {'obs': f(n * W, n_step, self.D), 'obs_next': f(n * W, 1, self.D),
                   'actions': f(n * W, n_step, self.A), 'rewards': f(n * W, n_step, 1),
                   'dones': f(n * W, n_step, 1)}
        K.window_emit(r['obs'], 0, n_step, stride, W, out['obs'])
        K.window_emit(r['obs'], n_step, 1, stride, W, out['obs_next'])
        K.window_emit(r['actions'], 0, n_step, stride, W, out['actions'])
        K.window_emit(r['rewards'].view(n, T + 1, 1), 0, n_step, stride, W, out['rewards'])
        K.window_emit(r['dones'].view(n, T + 1, 1), 0, n_step, stride, W, out['dones'])
        out['rewards'] = out['rewards'].view(n * W, n_step)
        out['dones'] = out['dones'].view(n * W, n_step)
        if 'pds' in r:
            if 'pds' not in out:
                out['pds'] = f(n * W, n_step, r['pds'].shape[2])
            K.window_emit(r['pds'], 0, n_step, stride, W, out['pds'])
        if self.pixel is not None:
            # the windows' camera observations: window cut and frame stacking in one gather over the raw frames
            C, H, Wd = self.pixel
            ns = self.frame_stacks
            u8 = lambda *s: torch.empty(*s, device=self.device, dtype=torch.uint8)  # noqa: E731
            if 'pixel' not in out:
                out['pixel'], out['pixel_next'] = u8(n * W, n_step, ns * C, H, Wd), u8(n * W, 1, ns * C, H, Wd)
            K.frame_stack(self.frames, ns, 0, n_step, stride, W, out['pixel'])
            K.frame_stack(self.frames, ns, n_step, 1, stride, W, out['pixel_next'])
        if 'cells' in r:
            # onetime_infos: the LSTM state at the FIRST step of every window (exp_sender_wrapper.py:236-242)
            cw = r['cells'][0, 0].numel()
            cells = out['cells'].view(n * W, 1, cw) if 'cells' in out else f(n * W, 1, cw)
            K.window_emit(r['cells'].view(n, T + 1, cw), 0, 1, stride, W, cells)
            out['cells'] = cells.view((n * W,) + tuple(r['cells'].shape[2:]))
        return out

    def to_batch(self, f):
        """emit_windows' fields -> the learner's batch contract (MultistepAggregatorWithInfo, aggregator.py:106-262)"""
        obs = collections.OrderedDict(low_dim=collections.OrderedDict(flat_inputs=f['obs']))
        nxt = collections.OrderedDict(low_dim=collections.OrderedDict(flat_inputs=f['obs_next']))
        if 'pixel' in f:
            obs['pixel'] = collections.OrderedDict(camera0=f['pixel'])
            nxt['pixel'] = collections.OrderedDict(camera0=f['pixel_next'])
        once = [f['cells'][:, 0], f['cells'][:, 1]] if 'cells' in f else None
        return {'obs': obs, 'obs_next': nxt, 'actions': f['actions'], 'rewards': f['rewards'], 'dones': f['dones'],
                'persistent_infos': [f['pds']], 'onetime_infos': once}
