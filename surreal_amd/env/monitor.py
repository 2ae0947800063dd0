"""
Episode bookkeeping around an environment and the periodic reports built on it
(surreal/env/monitor.py:11-218).

``EpisodeMonitor`` records per-episode reward / length / wall time and attaches
``info['episode']`` to the step that ends an episode.  The three reporting monitors differ only in
where a report goes and what happens after it, so they share ``_PeriodicReport``:

  ConsoleMonitor              a small table on stdout every `update_interval` episodes
  TrainingTensorplexMonitor   scalars ':reward' / 'step_per_s' under 'agent/<id>' every
                              tensorplex.update_schedule.training_env episodes
  EvalTensorplexMonitor       the same under 'eval/<id>' (update_schedule.eval_env), then sleeps
                              eval_env_sleep seconds and fetches fresh parameters

``DeviceEpisodeMonitor`` / ``DeviceTrainingMonitor`` are the same bookkeeping and the training reports for the actors
of a ``SyntheticVecEnv``, whose steps run on the device and never pass through a host ``Env``; ``DeviceEvaluator`` is the
evaluation worker behind ``EvalTensorplexMonitor`` for them: whole episodes in one launch (``SyntheticVecEnv.evaluate``).

The tensorplex process of the reference is replaced by any object with
``add_scalars(dict, global_step=...)`` (default: the in-memory ScalarRecorder the learners use).
"""
import collections
import time

from .base import Wrapper


def _mean(xs):
    return float(sum(xs)) / max(len(xs), 1)


def _fmt(x, precision):
    return ('%.*f' % (precision, x)).rstrip('0').rstrip('.')


class _Every(object):
    """True once per `period` calls (session/tracker.py PeriodicTracker.track_increment)"""

    def __init__(self, period):
        assert isinstance(period, int) and period > 0
        self.period, self.count = period, 0

    def __call__(self):
        self.count += 1
        if self.count >= self.period:
            self.count -= self.period
            return True
        return False


class EpisodeMonitor(Wrapper):
    def __init__(self, env):
        super().__init__(env)
        self._t_first = time.time()
        self._t_episode = None
        self._rewards = None
        self.episode_rewards, self.episode_steps, self.episode_durations = [], [], []
        self.total_steps = 0

    def _reset(self, **kwargs):
        self._rewards = []
        self._t_episode = time.time()
        return self.env.reset(**kwargs)

    def _step(self, action):
        ob, rew, done, info = self.env.step(action)
        self._rewards.append(rew)
        if done:
            now = time.time()
            ep = {'reward': round(sum(self._rewards), 6), 'steps': len(self._rewards),
                  'duration': round(now - self._t_episode, 6),
                  'total_elapsed': round(now - self._t_first, 6)}
            self.episode_rewards.append(ep['reward'])
            self.episode_steps.append(ep['steps'])
            self.episode_durations.append(ep['duration'])
            info['episode'] = ep
        self.total_steps += 1
        if done:
            self._on_episode_end()                   # reports see the finished step counted
        return ob, rew, done, info

    def _on_episode_end(self):
        pass

    @property
    def num_episodes(self):
        return len(self.episode_rewards)

    def step_per_sec(self, average_episodes):
        assert average_episodes > 0
        n = average_episodes
        return sum(self.episode_steps[-n:]) / (sum(self.episode_durations[-n:]) + 1e-7)


class _PeriodicReport(EpisodeMonitor):
    """calls report() at the end of every `period`-th episode"""

    def __init__(self, env, period, window):
        super().__init__(env)
        self._due = _Every(period)
        self._avg = window

    def _on_episode_end(self):
        if self._due():
            self.report(_mean(self.episode_rewards[-self._avg:]), self.step_per_sec(self._avg))

    def report(self, avg_reward, avg_speed):
        raise NotImplementedError


class ConsoleMonitor(_PeriodicReport):
    def __init__(self, env, update_interval=10, average_over=10, extra_rows=None, out=print):
        super().__init__(env, update_interval, average_over)
        if extra_rows is not None and not isinstance(extra_rows, collections.OrderedDict):
            raise AssertionError('extra_rows spec {"row caption": function(total_steps, num_episodes)} '
                                 'must be an OrderedDict')
        self._extra_rows = extra_rows or collections.OrderedDict()
        self._out = out

    def rows(self, avg_reward, avg_speed):
        rows = [['Last {} rewards'.format(self._avg), _fmt(avg_reward, 3)],
                ['Speed iter/s', _fmt(avg_speed, 1)],
                ['Total steps', self.total_steps],
                ['Episodes', self.num_episodes]]
        for caption, fn in self._extra_rows.items():
            rows.append([caption, str(fn(self.total_steps, self.num_episodes))])
        return rows

    def report(self, avg_reward, avg_speed):
        from tabulate import tabulate
        self._out(tabulate(self.rows(avg_reward, avg_speed), tablefmt='simple', numalign='left'))


class _TensorplexReport(_PeriodicReport):
    group = None
    schedule_key = None

    def __init__(self, env, ident, session_config, separate_plots, tensorplex=None):
        period = session_config['tensorplex']['update_schedule'][self.schedule_key]
        super().__init__(env, period, period)
        if tensorplex is None:
            from surreal_amd.learner.base import ScalarRecorder
            tensorplex = ScalarRecorder()
        self.tensorplex = tensorplex
        self.tensorplex_name = '{}/{}'.format(self.group, ident)
        self._separate_plots = separate_plots

    def _tag(self, tag):
        return ':' + tag if self._separate_plots else tag     # tensorplex: ':' = own section

    def report(self, avg_reward, avg_speed):
        self.tensorplex.add_scalars({self._tag('reward'): avg_reward, 'step_per_s': avg_speed},
                                    global_step=self.num_episodes)


class TrainingTensorplexMonitor(_TensorplexReport):
    group, schedule_key = 'agent', 'training_env'

    def __init__(self, env, agent_id, session_config, separate_plots=True, tensorplex=None):
        if not isinstance(agent_id, int):
            raise AssertionError('agent_id must be an int')
        super().__init__(env, agent_id, session_config, separate_plots, tensorplex)


class EvalTensorplexMonitor(_TensorplexReport):
    group, schedule_key = 'eval', 'eval_env'

    def __init__(self, env, eval_id, fetch_parameter, session_config, separate_plots=False,
                 tensorplex=None, sleep=time.sleep):
        super().__init__(env, eval_id, session_config, separate_plots, tensorplex)
        self._throttle_sleep = session_config['tensorplex']['update_schedule']['eval_env_sleep']
        self._sleep = sleep
        self._fetch_parameter = fetch_parameter
        self._fetch_parameter()                      # an evaluator that starts late catches up

    def report(self, avg_reward, avg_speed):
        super().report(avg_reward, avg_speed)
        self._sleep(self._throttle_sleep)
        self._fetch_parameter()


class DeviceEpisodeMonitor(object):
    """EpisodeMonitor for the actors of a SyntheticVecEnv, kept on the device (struct smx_episode_monitor,
    include/surreal_amd.h): every launch that steps the environments adds each actor's step reward to its open
    episode -- fp64, in step order, by the one lane that formed the reward -- and on done moves the (reward, steps)
    pair into the actor's ring of the last `capacity` finished episodes.  Nothing crosses to the host until poll().

    Made by SyntheticVecEnv.attach_monitor(capacity=...).  All words live in ONE buffer so that poll() is one copy:
    ep_reward fp64 [n] | ep_count int64 [n] | done_reward fp64 [n, capacity] | ep_steps int32 [n] | done_steps int32
    [n, capacity].  The rings are actor-major: finished episode e of actor a sits at [a, e % capacity], an actor's ring
    is one contiguous run that only its owning lane writes.

    episode_rewards / episode_steps: per-actor lists, as EpisodeMonitor's (each reward round(x, 6)); num_episodes: the
    finished episodes of all actors, dropped ones included; total_steps: the environment steps of all actors since
    the monitor was attached (counted on the host: n per step); dropped: finished episodes that left a ring before a
    poll() saw them (more than `capacity` of one actor between two polls)."""

    def __init__(self, n, capacity, device):
        import torch
        if int(capacity) < 1:
            raise ValueError('DeviceEpisodeMonitor: capacity must be positive, got %r' % (capacity,))
        self.n, self.capacity = int(n), int(capacity)
        n, c = self.n, self.capacity
        words = 2 * n + n * c                                    # the 8-byte fields
        self._buf = torch.zeros(words + (n + n * c + 1) // 2, dtype=torch.int64, device=device)
        b = self._buf
        self.ep_reward = b[:n].view(torch.float64)
        self.ep_count = b[n:2 * n]
        self.done_reward = b[2 * n:words].view(torch.float64).view(n, c)
        i32 = b[words:].view(torch.int32)
        self.ep_steps = i32[:n]
        self.done_steps = i32[n:n + n * c].view(n, c)
        self.episode_rewards = [[] for _ in range(n)]
        self.episode_steps = [[] for _ in range(n)]
        self.counts = [0] * n                                    # finished episodes of each actor at the last poll
        self.dropped_by_actor = [0] * n
        self.total_steps = 0
        self.steps_per_actor = 0

    def count_steps(self, k):
        """the env stepped every actor k times (SyntheticVecEnv calls this; the device is not asked)"""
        self.steps_per_actor += int(k)
        self.total_steps += int(k) * self.n

    def clear_open(self):
        """drops the open episode of every actor (EpisodeMonitor._reset); the finished ones stay"""
        self.ep_reward.zero_()
        self.ep_steps.zero_()

    @property
    def num_episodes(self):
        return sum(self.counts)

    @property
    def dropped(self):
        return sum(self.dropped_by_actor)

    def poll(self):
        """ONE device -> host read of the counters and rings -> the episodes finished since the last poll, as
        (actor, reward, steps) in actor order, each actor's oldest first.  An actor that finished more than `capacity`
        episodes since then lost the oldest: they are counted in `dropped`, the `capacity` newest are reported."""
        n, c = self.n, self.capacity
        host = self._buf.cpu()
        words = 2 * n + n * c
        counts = host[n:2 * n].tolist()
        rewards = host[2 * n:words].view(self.done_reward.dtype).view(n, c).tolist()
        steps = host[words:].view(self.done_steps.dtype)[n:n + n * c].view(n, c).tolist()
        new = []
        for a in range(n):
            first, last = self.counts[a], counts[a]
            if last - first > c:
                self.dropped_by_actor[a] += last - first - c
                first = last - c
            for e in range(first, last):
                r, s = round(rewards[a][e % c], 6), steps[a][e % c]
                self.episode_rewards[a].append(r)
                self.episode_steps[a].append(s)
                new.append((a, r, s))
            self.counts[a] = last
        return new

    def open_episodes(self):
        """(reward fp64 [n], steps int32 [n]) of the open episodes now, as host tensors (a second read; for tests)"""
        return self.ep_reward.cpu(), self.ep_steps.cpu()

    def mean_reward(self, last=10):
        """the mean over the last `last` polled episode rewards of every actor together (None before the first)"""
        xs = [r for per_actor in self.episode_rewards for r in per_actor[-int(last):]]
        return _mean(xs) if xs else None

    def state_dict(self):
        """the device words (the one LIVE buffer: open episodes, counts and rings) and what poll() keeps on the host"""
        return {'n': self.n, 'capacity': self.capacity, 'buf': self._buf,
                'episode_rewards': [list(x) for x in self.episode_rewards],
                'episode_steps': [list(x) for x in self.episode_steps], 'counts': list(self.counts),
                'dropped_by_actor': list(self.dropped_by_actor), 'total_steps': self.total_steps,
                'steps_per_actor': self.steps_per_actor}

    def check_state_dict(self, sd):
        if (int(sd['n']), int(sd['capacity'])) != (self.n, self.capacity) or tuple(sd['buf'].shape) != tuple(self._buf.shape):
            raise ValueError('DeviceEpisodeMonitor: the state is of %d actors with rings of %d, this monitor of %d with %d'
                             % (int(sd['n']), int(sd['capacity']), self.n, self.capacity))

    def load_state_dict(self, sd):
        self.check_state_dict(sd)
        self._buf.copy_(sd['buf'])
        self.episode_rewards = [[float(r) for r in x] for x in sd['episode_rewards']]
        self.episode_steps = [[int(s) for s in x] for x in sd['episode_steps']]
        self.counts = [int(c) for c in sd['counts']]
        self.dropped_by_actor = [int(c) for c in sd['dropped_by_actor']]
        self.total_steps, self.steps_per_actor = int(sd['total_steps']), int(sd['steps_per_actor'])


class DeviceNoise(object):
    """The exploration noise of a SyntheticVecEnv's actors as a counter-based stream (struct smx_noise_stream,
    include/surreal_amd.h): the standard normal of (seed, actor_base + a, step + k, j) for actor a, the k-th step from
    now and action component j is a pure function of the four (Philox4x32-10 and Box-Muller), formed inside the launch
    that consumes it.  Made by SyntheticVecEnv.attach_noise(seed, actor_base).

    step: the draw step of the env's next step -- one host integer all actors share, advanced by the env with every
    stepping call, never rewound by reset() (a new episode gets new noise); read it for a checkpoint, set it to resume
    (or to see the same draws again)."""

    def __init__(self, seed, actor_base, n, A, kernels, device):
        self.seed, self.actor_base, self.step = int(seed), int(actor_base), 0
        if not 0 <= self.seed < 1 << 64:
            raise ValueError('DeviceNoise: seed must fit 64 bits, got %r' % (seed,))
        if self.actor_base < 0 or self.actor_base + int(n) > 1 << 32:
            raise ValueError('DeviceNoise: global actor ids %d .. %d leave [0, 2^32)'
                             % (self.actor_base, self.actor_base + int(n) - 1))
        self.n, self.A, self.K, self.device = int(n), int(A), kernels, device

    def at(self, ahead=0):
        """(seed, actor_base, draw step `ahead` steps from now): what a launch's `noise=` keyword takes"""
        return (self.seed, self.actor_base, self.step + int(ahead))

    def draws(self, T, n=None, A=None):
        """-> [T, n, A] fp32 on the device: the draws the env's next T steps use (smx_noise_fill_f32: the launches'
        own function, the same bits), without advancing the counter.  n, A: the env's by default"""
        import torch
        out = torch.empty(int(T), self.n if n is None else int(n), self.A if A is None else int(A), device=self.device)
        self.K.noise_fill(self.at(), out)
        return out

    def state_dict(self):
        return {'seed': self.seed, 'actor_base': self.actor_base, 'step': self.step}

    def check_state_dict(self, sd):
        if int(sd['seed']) != self.seed or int(sd['actor_base']) != self.actor_base:
            raise ValueError('DeviceNoise: the state is of stream (seed %d, actor_base %d), this one of (%d, %d)'
                             % (int(sd['seed']), int(sd['actor_base']), self.seed, self.actor_base))
        if int(sd['step']) < 0:
            raise ValueError('DeviceNoise: step %d is negative' % int(sd['step']))

    def load_state_dict(self, sd):
        self.check_state_dict(sd)
        self.step = int(sd['step'])


class DeviceResets(object):
    """The episodes of a 'reach' or 'arm' SyntheticVecEnv as a counter-based stream (struct smx_reset_stream,
    include/surreal_amd.h; env/tasks.py: reach_reset_state, arm_reset_state): the row [p | v | g] resp. [theta | omega | g]
    that actor a (global id actor_base + a) begins episode e with is a pure function of (seed, actor_base + a, e), drawn inside the launch that steps over the
    episode's end.  Made by SyntheticVecEnv.attach_resets(seed, actor_base).

    disturbance: the scale s in [0, 1] of the per-step disturbance every launch on the stream applies (env/tasks.py:
    disturbance; 0: none, and at() is the triple it was).

    episode: the index of the NEXT episode to begin -- one host integer all actors share (they are on one clock).  A
    reset() draws it and adds one; a stepping call adds its episode ends (its i-th end draws episode + i).  Read it for
    a checkpoint, set it to resume or to see the same episodes again."""

    def __init__(self, seed, actor_base, n, D, kernels, device, task='reach', disturbance=0.0):
        from .tasks import check_disturbance
        self.disturbance = float(check_disturbance('DeviceResets', disturbance))     # (the fp32 value the launches get)
        self.seed, self.actor_base, self.episode = int(seed), int(actor_base), 0
        if not 0 <= self.seed < 1 << 64:
            raise ValueError('DeviceResets: seed must fit 64 bits, got %r' % (seed,))
        if self.actor_base < 0 or self.actor_base + int(n) > 1 << 32:
            raise ValueError('DeviceResets: global actor ids %d .. %d leave [0, 2^32)'
                             % (self.actor_base, self.actor_base + int(n) - 1))
        self.n, self.D, self.K, self.device, self.task = int(n), int(D), kernels, device, task

    def at(self, ahead=0):
        """(seed, actor_base, the episode index `ahead` episodes from now) -- with a disturbance (seed, actor_base, index,
        scale) --: what a launch's `resets=` keyword takes"""
        e = self.episode + int(ahead)
        if e < 0:
            raise ValueError('DeviceResets: episode %d is negative' % e)
        if self.disturbance != 0:
            return (self.seed, self.actor_base, e, self.disturbance)
        return (self.seed, self.actor_base, e)

    def states(self, e=None):
        """-> [n, D] fp32 on the device: the rows the actors begin episode e (None: the next one) with
        (smx_reset_fill_f32: the launches' own function, the same bits), without advancing the counter"""
        import torch
        out = torch.empty(self.n, self.D, device=self.device)
        self.fill(out, e)
        return out

    def fill(self, out, e=None):
        """states(e) into out [n, D]"""
        at = self.at() if e is None else (self.seed, self.actor_base, int(e))
        if at[2] < 0:
            raise ValueError('DeviceResets: episode %d is negative' % at[2])
        self.K.reset_fill(at, out, task=self.task)

    def state_dict(self):
        sd = {'seed': self.seed, 'actor_base': self.actor_base, 'episode': self.episode}
        if self.disturbance != 0:
            sd['disturbance'] = self.disturbance       # (an undisturbed stream keeps the keys it had)
        return sd

    def _same_disturbance(self, sd):
        """a checkpoint of another scale is refused (no key: scale 0)"""
        if float(sd.get('disturbance', 0.0)) != self.disturbance:
            raise ValueError('DeviceResets: the checkpoint is of a stream with disturbance %r, this one has %r'
                             % (float(sd.get('disturbance', 0.0)), self.disturbance))

    def check_state_dict(self, sd):
        """load_state_dict's refusals alone: nothing is written"""
        self._same_disturbance(sd)
        if int(sd['seed']) != self.seed or int(sd['actor_base']) != self.actor_base:
            raise ValueError('DeviceResets: the checkpoint is of stream (seed %d, actor_base %d), this one of (%d, %d)'
                             % (int(sd['seed']), int(sd['actor_base']), self.seed, self.actor_base))
        if int(sd['episode']) < 0:
            raise ValueError('DeviceResets: episode %d is negative' % int(sd['episode']))

    def load_state_dict(self, sd):
        self.check_state_dict(sd)
        self.episode = int(sd['episode'])


class DeviceParamNoise(object):
    """Parameter-space noise (agent/param_noise.py: 'normal' / 'adaptive_normal') for the actors of a SyntheticVecEnv, on
    the device.  The env's n actors form n / actors_per_agent AGENTS of consecutive actors that share one perturbation,
    as the actors of one reference agent process do -- an agent here spans at least 4 actors (one MFMA row block) where
    the reference's spans one environment.  Agent p (global id agent_base + p) acts from its own perturbed copy of the
    agent's actor, element i of the flat parameters W1 | b1 | W2 | b2 | W3 | b3 being w_i + (float)sigma[p] *
    z(seed, agent_base + p, generation, i): a pure function (struct smx_param_noise, include/surreal_amd.h).  Made by
    SyntheticVecEnv.attach_param_noise(agent, seed, actors_per_agent, agent_base).
    A LayerNorm actor (`ln`; where the kernels run one: kernels.ddpg_ln_launch): the flat parameters go on with ln1.W |
    ln1.b | ln2.W | ln2.b, perturbed by the same rule -- the reference perturbs every fetched array
    (param_noise.py:14-24) -- and every copy in pop carries them behind its biases.

    On the device: sigma fp64 [P], dist fp64 [P] (the action distance of each agent's first actor, written by the
    rollout launch at its measuring step), pop fp32 [P, copy floats] (the packed copies the launch reads).  On the host,
    readable and settable: generation (the perturbation in pop), acts (act() calls per actor since the last refresh).

    refresh() is on_parameter_fetched: call it whenever the agent's parameters changed."""

    def __init__(self, agent, seed, actors_per_agent, agent_base, n, kernels, device):
        import torch
        self.type = agent.param_noise_type
        if self.type not in ('normal', 'adaptive_normal'):
            raise ValueError('DeviceParamNoise: the agent\'s param_noise_type is %r; \'normal\' or \'adaptive_normal\''
                             % (self.type,))
        self.seed, self.agent_base, self.actors_per_agent = int(seed), int(agent_base), int(actors_per_agent)
        if not 0 <= self.seed < 1 << 64:
            raise ValueError('DeviceParamNoise: seed must fit 64 bits, got %r' % (seed,))
        if self.actors_per_agent <= 0 or self.actors_per_agent % 4 or int(n) % self.actors_per_agent:
            raise ValueError('DeviceParamNoise: actors_per_agent must be a multiple of 4 that divides the %d actors, got %d'
                             % (n, self.actors_per_agent))
        self.agents = int(n) // self.actors_per_agent
        if self.agent_base < 0 or self.agent_base + self.agents > 1 << 32:
            raise ValueError('DeviceParamNoise: global agent ids %d .. %d leave [0, 2^32)'
                             % (self.agent_base, self.agent_base + self.agents - 1))
        self.agent, self.K, self.device = agent, kernels, device
        self.adaptive = self.type == 'adaptive_normal'
        self.alpha, self.target = float(agent.param_noise_alpha), float(agent.param_noise_target_stddev)
        self.compute_dist_interval = 10          # AdaptiveNormalParameterNoise's default, which DDPGAgent leaves
        self.sigma = torch.full((self.agents,), float(agent.param_noise_sigma), dtype=torch.float64, device=device)
        self.dist = torch.zeros(self.agents, dtype=torch.float64, device=device)
        # (kernels that run no LayerNorm actor: the plain copies, and ddpg_rollout_into refuses a LayerNorm actor)
        from surreal_amd.kernels import ddpg_ln_launch
        self.ln = bool(agent.model.use_layernorm) and ddpg_ln_launch(kernels)
        self.pop = torch.zeros(self.agents, kernels.param_noise_copy_numel(agent.model.actor, ln=self.ln), device=device)
        self.generation, self.acts = -1, 0
        self.refresh()                           # generation 0; no act yet: no adaptation

    def _ln(self):
        """the clean actor's LayerNorm gains and biases as the kernels take them, None for a plain actor"""
        return self.agent.model.actor_ln_flat if self.ln else None

    def refresh(self):
        """the device form of on_parameter_fetched, no host synchronisation: with 'adaptive_normal' and acts > 0 every
        agent's sigma is divided (dist / acts > target_stddev) or multiplied by alpha; then all agents are perturbed
        again from the agent's current clean actor under generation + 1; acts = 0"""
        if self.generation + 1 >= 1 << 32:
            raise ValueError('DeviceParamNoise: generation %d leaves [0, 2^32)' % (self.generation + 1))
        self.generation += 1
        self.K.param_noise_refresh(self.agent.model.actor, self, ln=self._ln())
        self.acts = 0

    def measure_step(self, T):
        """the step of a call of T steps that measures the action distance: the last s with (acts + s) %
        compute_dist_interval == 0 (the reference overwrites its distance at every such act, param_noise.py:59-63: only
        the last one before a refresh counts); -1: none, and always for 'normal'"""
        if not self.adaptive:
            return -1
        k = self.compute_dist_interval
        s = (int(T) - 1) - (self.acts + int(T) - 1) % k
        return s if s >= 0 else -1

    def perturbed(self, p):
        """-> {'W1', 'b1', 'W2', 'b2', 'W3', 'b3'}, with a LayerNorm actor also {'ln1.W', 'ln1.b', 'ln2.W', 'ln2.b'}:
        agent p's perturbed actor parameters under the current generation and sigma, as tensors
        (smx_param_noise_fill_f32: the function the copies in pop are made of)"""
        import collections
        import torch
        model, actor = self.agent.model, self.agent.model.actor
        views = list(actor.views.items()) + (list(model.actor_ln.items()) if self.ln else [])
        flat = torch.empty(sum(v.numel() for _, v in views), device=self.device)
        self.K.param_noise_fill(actor, self, p, flat, ln=self._ln())
        out, o = collections.OrderedDict(), 0
        for k, v in views:
            out[k] = flat[o:o + v.numel()].view(v.shape)
            o += v.numel()
        return out

    def state_dict(self):
        return {'sigma': self.sigma.cpu(), 'dist': self.dist.cpu(), 'pop': self.pop.cpu(),
                'generation': self.generation, 'acts': self.acts}

    def check_state_dict(self, sd):
        """ValueError unless the state fits this population (agents, copy size): nothing is written"""
        for k in ('sigma', 'dist', 'pop'):
            have = getattr(self, k)
            if tuple(sd[k].shape) != tuple(have.shape) or sd[k].dtype != have.dtype:
                raise ValueError('DeviceParamNoise: the saved %s is %s %s, this population\'s %s %s'
                                 % (k, tuple(sd[k].shape), sd[k].dtype, tuple(have.shape), have.dtype))
        if not -1 <= int(sd['generation']) < 1 << 32 or int(sd['acts']) < 0:
            raise ValueError('DeviceParamNoise: generation %d, acts %d' % (int(sd['generation']), int(sd['acts'])))

    def load_state_dict(self, sd):
        for k in ('sigma', 'dist', 'pop'):
            getattr(self, k).copy_(sd[k])
        self.generation, self.acts = int(sd['generation']), int(sd['acts'])


class _DeviceActorReport(TrainingTensorplexMonitor):
    """TrainingTensorplexMonitor for one actor of a DeviceEpisodeMonitor: the same period, mean, tags and global_step,
    fed with polled episodes instead of wrapping an env"""

    def __init__(self, owner, agent_id, session_config, separate_plots, tensorplex):
        super().__init__(None, agent_id, session_config, separate_plots, tensorplex)
        self._owner = owner
        self._finished = 0

    @property
    def num_episodes(self):
        return self._finished

    def step_per_sec(self, average_episodes):
        return self._owner.step_per_s

    def feed(self, reward, steps, skipped=0):
        for _ in range(skipped):                     # episodes that left the ring unseen still count towards a period
            self._finished += 1
            self._due()
        self.episode_rewards.append(reward)
        self.episode_steps.append(steps)
        self._finished += 1
        self._on_episode_end()


class _DeviceEvalReport(_TensorplexReport):
    """EvalTensorplexMonitor's report for one actor of a DeviceEvaluator: the same period (update_schedule.eval_env),
    mean, tags and global_step under 'eval/<id>', fed with the returns of an evaluation launch instead of wrapping an
    env; it neither sleeps nor fetches (the evaluator fetches once per run)"""
    group, schedule_key = 'eval', 'eval_env'

    def __init__(self, owner, eval_id, session_config, separate_plots, tensorplex):
        super().__init__(None, eval_id, session_config, separate_plots, tensorplex)
        self._owner = owner
        self._finished = 0

    @property
    def num_episodes(self):
        return self._finished

    def step_per_sec(self, average_episodes):
        return self._owner.step_per_s

    def feed(self, reward, steps):
        self.episode_rewards.append(reward)
        self.episode_steps.append(steps)
        self._finished += 1
        self._on_episode_end()


class DeviceEvaluator(object):
    """The reference's evaluation worker behind EvalTensorplexMonitor (surreal/agent/base.py:277-345,
    surreal/env/monitor.py:164-218) for the n actors of a SyntheticVecEnv: run() fetches the agent's parameters, runs
    `episodes` whole episodes of every actor in ONE launch (SyntheticVecEnv.evaluate: nothing recorded, the env's state
    untouched), copies the [n, episodes] returns to the host once and feeds actor i's -- each round(x, 6), as
    EpisodeMonitor reports an episode -- to a report under 'eval/<eval_id_base + i>': every eval_env-th episode of an
    actor, 'reward' (':reward' with separate_plots; the mean of its last eval_env returns) and 'step_per_s' with
    global_step = that actor's episode count.  No sleep between reports: a run is one launch.
    resets: evaluate()'s -- None, or (seed, first_episode[, actor_base]): the same held-out episodes every run;
    disturbance: evaluate()'s scale on them.
    noise (an 'eval_stochastic' PPO agent): evaluate()'s (seed, first_step[, actor_base]); every run moves first_step on
    by its episodes * episode_len steps.  tensorplex None: one ScalarRecorder per actor (reports[i].tensorplex), else
    the one object all share.
    step_per_s: the environment steps of one actor per second of the last run()'s wall time."""

    def __init__(self, env, agent, session_config, episodes, resets=None, eval_id_base=0, tensorplex=None,
                 separate_plots=False, noise=None, disturbance=None):
        if int(episodes) < 1:
            raise ValueError('DeviceEvaluator: episodes must be positive, got %r' % (episodes,))
        self.env, self.agent, self.episodes = env, agent, int(episodes)
        self.disturbance = disturbance                 # (evaluate()'s: the held-out episodes' scale, None: undisturbed)
        self.resets = None if resets is None else tuple(int(v) for v in resets)
        self.noise = None if noise is None else [int(v) for v in noise]
        self.reports = [_DeviceEvalReport(self, int(eval_id_base) + i, session_config, separate_plots, tensorplex)
                        for i in range(env.n)]
        self.step_per_s = 0.0
        self.runs = 0
        self._out = None

    def run(self):
        """-> the returns of this run, np.float64 [n, episodes]"""
        self.agent.fetch_parameter()
        E, steps = self.episodes, int(self.env.episode_len)
        t0 = time.time()
        kw = {} if self.noise is None else {'noise': tuple(self.noise)}
        if self.disturbance is not None:
            kw['disturbance'] = self.disturbance
        self._out = self.env.evaluate(self.agent, E, resets=self.resets, out=self._out, **kw)
        host = self._out.cpu().numpy()                 # (the one device -> host copy; it waits for the launch)
        if self.noise is not None:
            self.noise[1] += E * steps
        self.step_per_s = E * steps / (time.time() - t0 + 1e-7)
        self.runs += 1
        for i, report in enumerate(self.reports):
            for e in range(E):
                report.feed(round(float(host[i, e]), 6), steps)
        return host

    def mean_return(self):
        """the mean over the last run's returns of every actor (None before the first run)"""
        xs = [r for report in self.reports for r in report.episode_rewards[-self.episodes:]]
        return _mean(xs) if xs else None


class DeviceEvalSnapshots(object):
    """`capacity` parameter SNAPSHOTS of one policy architecture on the device, all evaluated on the same episodes in ONE
    launch (smx_synth_ppo_eval_sets_f32 / smx_synth_ddpg_eval_sets_f32): a learning curve's snapshots, an actor and its
    target, the last K checkpoints.  Every set sees the same reset stream and the same noise stream, so a comparison
    between snapshots is paired; set k's returns have the bits of env.evaluate() of an agent holding its parameters.
    Also SyntheticVecEnv.eval_snapshots(agent, capacity).

    agent: the TEMPLATE, an evaluation agent env.can_evaluate() accepts (anything else: can_evaluate's refusal, before
    anything is allocated) -- it gives the architecture, whether a z-filter is used, and evaluate()'s mode.
    buf: float32 [capacity, stride] on the device, slot k one snapshot (smx_eval_snapshot_floats: the packed actor, its
    biases, a PPO policy's log_var, z-filter sums and packed LSTM); stored: which slots hold one."""

    def __init__(self, env, agent, capacity, _population=None):
        import torch
        pn = _population
        refusal = env._eval_refusal(agent, population=pn is not None)
        if refusal is not None:
            raise refusal[0](refusal[1])
        self.ppo = hasattr(agent, 'rnn_config')
        K = env.K
        for name in ('eval_snapshot_floats', 'eval_snapshot_store', 'synth_ppo_eval_sets' if self.ppo else 'synth_ddpg_eval_sets'):
            if getattr(K, name, None) is None:
                raise NotImplementedError('DeviceEvalSnapshots: the kernels object has no %s' % name)
        capacity = int(capacity)
        if not 1 <= capacity <= 65535:
            raise ValueError('DeviceEvalSnapshots: capacity must lie in [1, 65535], got %d' % capacity)
        self.env, self.agent, self.K, self.capacity = env, agent, K, capacity
        self.zfilter = bool(self.ppo and agent.use_z_filter)
        self.floats = self._floats(agent)
        if self.floats <= 0:
            raise NotImplementedError('DeviceEvalSnapshots: smx_eval_snapshot_floats refuses the policy\'s shapes')
        self.population = pn
        if pn is None:
            self.buf = torch.zeros(capacity, self.floats, device=env.device)
            self.stored = [False] * capacity
        else:
            self.buf = pn.pop                        # (zero copy: refresh() rewrites the slots)
            self.stored = [True] * capacity
        self.stride = int(self.buf.shape[1])

    @classmethod
    def from_param_noise(cls, env, pn):
        """a zero-copy view of a plain-actor DeviceParamNoise's population: slot p is agent p's perturbed actor as
        pn.pop holds it (one agent's copy IS a DDPG snapshot), so evaluate() gives every perturbed actor's returns over
        all n actors' episodes, acting without exploration noise.  The view cannot store(); pn.refresh() moves it on.
        A LayerNorm population: NotImplementedError"""
        if pn.ln:
            raise NotImplementedError('DeviceEvalSnapshots.from_param_noise with a LayerNorm actor: the evaluation launch '
                                      'runs a plain DDPG actor, only')
        snaps = cls(env, pn.agent, pn.agents, _population=pn)
        if int(pn.pop.shape[1]) < snaps.floats or int(pn.pop.shape[1]) % 4:
            raise ValueError('DeviceEvalSnapshots.from_param_noise: a copy of the population has %d floats, a snapshot %d'
                             % (int(pn.pop.shape[1]), snaps.floats))
        return snaps

    def _floats(self, agent):
        m = agent.model
        return self.K.eval_snapshot_floats(model=m, zfilter=self.zfilter) if self.ppo else \
            self.K.eval_snapshot_floats(actor=m.actor)

    @staticmethod
    def _architecture(agent):
        """what two agents must share to share snapshots"""
        ppo = hasattr(agent, 'rnn_config')
        m = agent.model
        a = m.actor
        arch = (ppo, a.D, a.H1, a.H2, a.OUT)
        if ppo:
            rnn = bool(agent.rnn_config.if_rnn_policy)
            arch += (bool(agent.use_z_filter), rnn) + ((m.rnn.D, m.rnn.H, m.rnn_hidden_logical) if rnn else ())
        return arch

    def _slots(self, first, count):
        first = int(first)
        count = self.capacity - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > self.capacity:
            raise ValueError('DeviceEvalSnapshots: slots [%d, %d) leave [0, %d)' % (first, first + count, self.capacity))
        return first, count

    def store(self, slot, agent=None):
        """slot <- the agent's (None: the template's) CURRENT parameters, the z-filter's sums with them where the
        template uses one; asynchronous, no host synchronisation (smx_eval_snapshot_store_f32).  The slot then no longer
        depends on the agent.  An agent of another architecture or z-filter use: ValueError"""
        if self.population is not None:
            raise ValueError('DeviceEvalSnapshots.store: a view of a parameter-noise population holds its perturbed '
                             'actors (refresh the noise)')
        slot, _ = self._slots(slot, 1)
        agent = self.agent if agent is None else agent
        if hasattr(agent, 'rnn_config') != self.ppo or self._architecture(agent) != self._architecture(self.agent):
            raise ValueError('DeviceEvalSnapshots.store: the agent\'s architecture %r is not the template\'s %r'
                             % (self._architecture(agent), self._architecture(self.agent)))
        m = agent.model
        if self.ppo:
            self.K.eval_snapshot_store(self.buf[slot], model=m, zfilter=m.z_filter if self.zfilter else None)
        else:
            self.K.eval_snapshot_store(self.buf[slot], actor=m.actor)
        self.stored[slot] = True

    def evaluate(self, episodes=1, first=0, count=None, resets=None, noise=None, out=None, actors_per_workgroup=0,
                 disturbance=None):
        """`episodes` whole episodes of every actor under each of the snapshots in slots [first, first + count) (count
        None: up to the last slot; all must have been stored, else ValueError) in ONE launch -> their returns,
        torch.float64 [count, n, episodes] on the device (`out`, or a new tensor); no synchronisation.  The mode rule,
        resets=, noise=, disturbance= and the size checks are SyntheticVecEnv.evaluate's, with the template agent's mode;
        it is pure in the same sense"""
        import torch
        first, count = self._slots(first, count)
        env = self.env
        ppo, E, resets, noise = env._eval_check(self.agent, episodes, resets, noise, self.population is not None, count,
                                                disturbance=disturbance)
        missing = [k for k in range(first, first + count) if not self.stored[k]]
        if missing:
            raise ValueError('DeviceEvalSnapshots.evaluate: slots %r were never stored' % (missing,))
        n, L_ = env.n, int(env.episode_len)
        if out is None:
            out = torch.empty(count, n, E, dtype=torch.float64, device=env.device)
        elif out.dtype != torch.float64 or tuple(out.shape) != (count, n, E) or not out.is_contiguous():
            raise ValueError('evaluate: out must be a contiguous torch.float64 [%d, %d, %d] tensor' % (count, n, E))
        blobs = self.buf[first:first + count]
        kw = dict(task=env.task, resets=resets, actors_per_workgroup=actors_per_workgroup)
        m = self.agent.model
        if ppo:
            self.K.synth_ppo_eval_sets(m, blobs, env.init_state, E, L_, out, zfilter=m.z_filter if self.zfilter else None,
                                       noise=noise, **kw)
        else:
            self.K.synth_ddpg_eval_sets(m.actor, blobs, env.init_state, E, L_, out, **kw)
        return out

    def state_dict(self):
        return {'buf': self.buf.to('cpu', copy=True), 'stored': list(self.stored)}

    def load_state_dict(self, sd):
        if tuple(sd['buf'].shape) != tuple(self.buf.shape) or len(sd['stored']) != self.capacity:
            raise ValueError('DeviceEvalSnapshots: the checkpoint holds %r floats in %d slots, this one %r in %d'
                             % (tuple(sd['buf'].shape), len(sd['stored']), tuple(self.buf.shape), self.capacity))
        self.buf.copy_(sd['buf'])
        self.stored = [bool(v) for v in sd['stored']]


class DeviceTrainingMonitor(object):
    """What n TrainingTensorplexMonitor(agent_id=i) around n host envs would report, for the actors of a
    SyntheticVecEnv: on each poll(), for actor i and every training_env-th of its episodes, ':reward' (the mean of its
    last training_env episode rewards) and 'step_per_s' under 'agent/<i>' with global_step = that actor's episode
    count.  tensorplex None: one ScalarRecorder per actor (reports[i].tensorplex), else the one object all share.

    step_per_s: the device keeps no per-episode wall clock, so this is the environment steps of one actor per second
    of wall time between the last two polls -- not the host monitor's per-episode figure."""

    def __init__(self, env, session_config, tensorplex=None, separate_plots=True):
        self.env = env
        self.monitor = env.monitor if getattr(env, 'monitor', None) is not None else env.attach_monitor()
        self.reports = [_DeviceActorReport(self, i, session_config, separate_plots, tensorplex)
                        for i in range(self.monitor.n)]
        self.step_per_s = 0.0
        self._t_poll, self._steps_poll = time.time(), self.monitor.steps_per_actor
        self._dropped_seen = list(self.monitor.dropped_by_actor)

    def poll(self):
        m = self.monitor
        new = m.poll()
        now = time.time()
        self.step_per_s = (m.steps_per_actor - self._steps_poll) / (now - self._t_poll + 1e-7)
        self._t_poll, self._steps_poll = now, m.steps_per_actor
        for a, reward, steps in new:
            skipped = m.dropped_by_actor[a] - self._dropped_seen[a]
            self._dropped_seen[a] = m.dropped_by_actor[a]
            self.reports[a].feed(reward, steps, skipped)
        return new

    def mean_reward(self, last=10):
        return self.monitor.mean_reward(last)
