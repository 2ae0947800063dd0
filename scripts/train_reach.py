"""The on-device loop on a task a policy can learn: `reach`, or with --task arm `arm` (surreal_amd/env/tasks.py).

    python scripts/train_reach.py --algo ppo|ddpg [--task reach|arm] [--actors N --J J --episode-len L --iters K --seed S
                                  --out FILE]
                                  [--random-resets [--heldout-episodes E]] [--eval-heldout] [--device-eval]
                                  [--snapshot-curve] [--save PATH [--save-every K]] [--resume PATH]
                                  [--layernorm] [--param-noise normal|adaptive_normal [--actors-per-agent K]]
                                  [--disturbance [S]] [--double-critic] [--policy-delay D]

Per iteration: one rollout chunk of all actors inside one launch (ppo_rollout_into / ddpg_rollout_into on a
SyntheticVecEnv(task='reach') with a DeviceEpisodeMonitor and an exploration noise stream attached) -> the replay's device
ring -> learn -> the parameters back to the agent (publish + fetch).  Every --eval-every iterations the deterministic
policy (an agent in mode 'eval_deterministic') is run from the reset states of the same seeds with step(), one episode.

Prints first the zero-action return and the PD controller's return on the same seeds, from the host env; then one JSON
line per evaluation: env steps, learner iterations, the training return from the monitor, the evaluation return, the share
of the zero -> PD gap the evaluation return closes, wall time.

--random-resets: every training episode begins with a new start and goal, drawn on the device from a reset stream
(SyntheticVecEnv.attach_resets, seed S + 2).  The evaluation env is attached to a stream with a DIFFERENT seed (S + 3)
whose episode index is set back to 0 before each evaluation, so every evaluation sees the same E held-out episodes per
actor (default 4), none of which training ever drew; the zero-action and PD returns come from the host env
(SyntheticEnv(resets=...)) on those same episodes.
--eval-heldout (without --random-resets): train the old way, from the 64 fixed reset states, but evaluate on the held-out
episodes -- the measurement that shows what random resets buy.
--device-eval: the evaluation return comes from ONE launch on the training env (SyntheticVecEnv.evaluate: whole episodes,
nothing recorded, the env untouched; the held-out form with resets=(S + 3, 0); a sampling evaluation agent -- PPO's under
env_config.stochastic_eval -- draws from a noise stream of seed S + 4); every curve line then also carries the
per-step figure on the same parameters (eval_return_per_step) and the wall time of both.  Without the flag nothing
changes.
--snapshot-curve: at every evaluation point the evaluation agent's parameters go into a slot of a DeviceEvalSnapshots on
the training env (one asynchronous store); after training ALL of them are evaluated in ONE launch on the evaluation's
episodes -- the held-out ones (resets=(S + 3, 0), --heldout-episodes per actor) where the evaluation is held out, else one
episode from every actor's reset state; a sampling PPO agent draws from ONE fixed noise stream (S + 4, first_step 0) for
all snapshots, so the points are paired -- and one last line {"kind": "snapshot_curve", ...} carries the mean return per
point.  With --device-eval and a deterministic evaluation agent every point must have the bits of the per-point device
evaluation made during training (asserted; "bits_match": true).  Without the flag every line is unchanged.
--save PATH: the whole run -- env, both agents, replay, learner, the torch generators, the loop's counters and the
baselines -- goes into ONE file (surreal_amd/utils/run_state.py; written atomically) after every K-th chunk (--save-every K)
and after the last one.  --resume PATH: the run goes on from that file, with the same --algo / --actors / --J /
--episode-len / --seed / reset flags (anything else: ValueError): from there on it prints exactly the lines the
uninterrupted run prints, wall times apart -- the baseline line is not printed again.  Not with --snapshot-curve.
DDPG only: --layernorm: a LayerNorm behind each hidden ReLU of actor and critic (use_layernorm; the rollout is the
LayerNorm instantiation of the one-launch kernel on the task).  --param-noise T: parameter-space noise of type T on the
device (SyntheticVecEnv.attach_param_noise, seed S + 5): every --actors-per-agent K consecutive actors (default 4, a
multiple of 4 that divides --actors) act from their own perturbed copy of the actor; where the loop hands the learner's
parameters to the agent the noise is refreshed ('adaptive_normal': every agent's sigma adapted to its measured action
distance first).  With a plain-actor population every evaluation point also prints {"kind": "population", ...}: the
deterministic return of every agent's perturbed actor on the evaluation's episodes, one launch for all
(DeviceEvalSnapshots.from_param_noise), and the agents' sigmas.  Neither option goes with --device-eval or
--snapshot-curve (the evaluation launch runs a plain actor without an attached noise).  Without them every printed line is
what it was.
--double-critic (DDPG): TD3's second critic (use_double_critic; the learner is asked for the row schedule,
ddpg_row_schedule = True).  --policy-delay D (DDPG): the actor and the target networks move once per D learner iterations
(learner_config.algo.network.policy_delay).  Both are named by the run's identity; without them every printed line is what
it was.
--task arm: the same loop on the planar arm of J links (D = 2 J + 2): the controller's line ("pd_return") is the
Jacobian-transpose baseline's (tasks.arm_jt_action), every line that names the run also carries "task": "arm".  The default,
reach, prints what it printed.
--disturbance [S] (needs --random-resets; S alone: DEFAULT_DISTURBANCE): the task is stochastic -- every step of every
training episode adds S * w to the sum that becomes the next velocity, w drawn on the device from the reset stream's Philox
(SyntheticVecEnv.attach_resets(disturbance=S); tasks.disturbance) -- and the held-out evaluation runs under the same scale
on its own stream (seed S + 3): the zero action's and the controller's returns come from the host env
(SyntheticEnv(resets=, disturbance=)) on those same disturbed episodes.  Every line that names the run carries
"disturbance": S.  Without the flag every printed line is what it was."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from surreal_amd.env import tasks as TK  # noqa: E402
from surreal_amd.env.synthetic_env import SyntheticEnv, SyntheticVecEnv  # noqa: E402

HIDDEN = [32, 32]
# --disturbance without a value.  Chosen on the host env and the CPU double before any training run (J = 2, episodes of 50,
# 64 actors x 4 held-out episodes, seed 0; profiles/task_disturbance_learning.jsonl has the table): large enough that the
# zero action's held-out return moves visibly, small enough that the baseline controller still solves the task
DEFAULT_DISTURBANCE = 0.25
DEFAULT_ITERS = {'ppo': 60, 'ddpg': 60}


def obs_dim(task, J):
    return {'reach': 3 * J, 'arm': 2 * J + 2}[task]


def host_return(J, episode_len, seeds, controller, task='reach'):
    """the mean episode return of controller(state) -> action from each seed's reset state, on the host env"""
    total = []
    for seed in seeds:
        env = SyntheticEnv(obs_dim(task, J), J, episode_len=episode_len, seed=seed, task=task)
        env._reset()
        ret, done = 0.0, False
        while not done:
            _, r, done, _ = env._step(controller(env.state))
            ret += r
        total.append(ret)
    return float(np.mean(total))


def baselines(J, episode_len, seeds, task='reach'):
    return {'zero_action_return': host_return(J, episode_len, seeds, lambda s: np.zeros(J, np.float32), task),
            'pd_return': host_return(J, episode_len, seeds, TK.BASELINE_ACTION[task], task)}


def heldout_return(J, episode_len, actors, seed, episodes, controller, task='reach', disturbance=0.0):
    """the mean episode return of controller(state) -> action over episodes 0 .. episodes - 1 of every actor of the
    reset stream `seed` (under its disturbance), on the host env"""
    total = []
    for g in range(actors):
        env = SyntheticEnv(obs_dim(task, J), J, episode_len=episode_len, task=task, resets=(seed, g),
                           disturbance=disturbance)
        for _ in range(episodes):
            env._reset()
            ret, done = 0.0, False
            while not done:
                _, r, done, _ = env._step(controller(env.state))
                ret += r
            total.append(ret)
    return float(np.mean(total))


def heldout_baselines(J, episode_len, actors, seed, episodes, task='reach', disturbance=0.0):
    return {'zero_action_return': heldout_return(J, episode_len, actors, seed, episodes, lambda s: np.zeros(J, np.float32),
                                                 task, disturbance),
            'pd_return': heldout_return(J, episode_len, actors, seed, episodes, TK.BASELINE_ACTION[task], task, disturbance)}


def ppo_configs(D, A, n, folder):
    from surreal_amd.main.ppo_configs import ppo_learner_config, ppo_env_config, ppo_session_config
    lc = ppo_learner_config()
    lc.model.actor_fc_hidden_sizes = lc.model.critic_fc_hidden_sizes = list(HIDDEN)
    lc.algo.rnn.if_rnn_policy = False
    lc.algo.n_step, lc.algo.stride = 10, 10
    lc.algo.gamma = 0.95
    lc.algo.ppo_mode = 'clip'
    lc.algo.network.lr_actor, lc.algo.network.lr_critic = 3e-3, 3e-3
    lc.algo.network.anneal.min_lr = 3e-3
    lc.algo.consts.init_log_sig = -0.5
    lc.replay.batch_size = 64
    lc.replay.memory_size = 8 * n
    lc.replay.sampling_start_size = 64
    lc.parameter_publish.exp_interval = 64
    return lc, ppo_env_config(D, A), ppo_session_config(folder)


def ddpg_configs(D, A, n, folder, layernorm=False, param_noise=None, double_critic=False, policy_delay=1):
    from surreal_amd.main.ddpg_configs import ddpg_learner_config, ddpg_env_config, ddpg_session_config
    lc = ddpg_learner_config()
    lc.model.actor_fc_hidden_sizes = lc.model.critic_fc_hidden_sizes = list(HIDDEN)
    # (a step's reward reaches -10 and more: a critic that learns fast and a slow actor; with the critic at the default
    # 1e-3 the actor saturated at a clip before the critic meant anything)
    lc.algo.n_step, lc.algo.gamma = 3, 0.95
    lc.algo.network.lr_actor, lc.algo.network.lr_critic = 1e-4, 1e-2
    lc.algo.network.target_update = {'type': 'soft', 'tau': 0.01}
    lc.algo.exploration.noise_type, lc.algo.exploration.max_sigma = 'normal', 1.0
    lc.replay.batch_size = 256
    lc.replay.memory_size = 64 * 1024
    lc.model.use_layernorm = bool(layernorm)
    lc.algo.exploration.param_noise_type = param_noise
    sc = ddpg_session_config(folder)
    if double_critic:                # (two critics take the row schedule only when asked to)
        lc.algo.network.use_double_critic = True
        sc.learner.ddpg_row_schedule = True
    if policy_delay != 1:
        lc.algo.network.policy_delay = policy_delay
    return lc, ddpg_env_config(D, A, num_agents=n), sc


class Loop(object):
    """the loop of one algorithm: the training env, agent, learner and replay, and the evaluation pair"""

    def __init__(self, algo, actors, J, episode_len, seed, device=None, folder='/tmp/surreal_amd_reach',
                 random_resets=False, heldout=0, layernorm=False, param_noise=None, actors_per_agent=4, task='reach',
                 disturbance=0.0, double_critic=False, policy_delay=1):
        """random_resets: the training env draws its episodes (reset stream seed + 2); heldout = E > 0: the evaluation
        runs E episodes per actor of the stream seed + 3, the same ones every time; layernorm / param_noise /
        actors_per_agent / double_critic / policy_delay (DDPG): the module docstring's; disturbance: the scale on both
        streams (needs both)"""
        self.disturbance = float(TK.check_disturbance('--disturbance', disturbance))
        if self.disturbance != 0 and not (random_resets and heldout):
            raise ValueError('--disturbance: the draws come from the reset streams: with --random-resets only')
        if algo != 'ddpg' and (layernorm or param_noise):
            raise ValueError('--layernorm / --param-noise: DDPG only')
        if algo != 'ddpg' and (double_critic or policy_delay != 1):
            raise ValueError('--double-critic / --policy-delay: DDPG only')
        if param_noise not in (None, 'normal', 'adaptive_normal'):
            raise ValueError('--param-noise: normal or adaptive_normal, got %r' % (param_noise,))
        torch.manual_seed(seed)
        self.seed = seed
        self.algo, self.n, self.J, self.L = algo, actors, J, episode_len
        self.task = task
        D, A = obs_dim(task, J), J
        kw = dict(device=device) if device is not None else {}
        if algo == 'ppo':
            from surreal_amd.agent import PPOAgent as Agent
            from surreal_amd.learner import PPOLearner as Learner
            from surreal_amd.replay import FIFOReplay as Replay
            cfg = ppo_configs(D, A, actors, folder)
        else:
            from surreal_amd.agent import DDPGAgent as Agent
            from surreal_amd.learner.ddpg import DDPGLearner as Learner
            from surreal_amd.replay import UniformReplay as Replay
            cfg = ddpg_configs(D, A, actors, folder, layernorm, param_noise, double_critic, policy_delay)
        self.lc = cfg[0]
        self.learner = Learner(*cfg)
        self.replay = Replay(*cfg)
        self.agent = Agent(*cfg, agent_id=0, agent_mode='training')
        self.eval_agent = Agent(*cfg, agent_id=1, agent_mode='eval_deterministic')
        for ag in (self.agent, self.eval_agent):
            ag.attach_learner(self.learner)
            ag.fetch_parameter()
        seeds = list(range(actors))
        self.venv = SyntheticVecEnv(actors, D, A, episode_len=episode_len, seeds=seeds, task=task, **kw)
        self.monitor = self.venv.attach_monitor(capacity=8)
        self.venv.attach_noise(seed=seed + 1)
        self.eval_env = SyntheticVecEnv(actors, D, A, episode_len=episode_len, seeds=seeds, task=task, **kw)
        self.heldout = int(heldout)
        self.eval_monitor = self.eval_env.attach_monitor(capacity=max(2, self.heldout))
        if random_resets:
            self.venv.attach_resets(seed + 2, disturbance=self.disturbance)
            self.venv.reset()
        if self.heldout:
            self.eval_env.attach_resets(seed + 3, disturbance=self.disturbance)
        self.layernorm = bool(layernorm)
        self.double_critic, self.policy_delay = bool(double_critic), policy_delay
        # (the parameter noise of the training agent, on the device: populations of actors_per_agent actors)
        self.pn = self.venv.attach_param_noise(self.agent, seed + 5, actors_per_agent=actors_per_agent) \
            if param_noise else None
        self.env_steps = self.learns = self.device_eval_steps = 0
        self.T = episode_len                       # a chunk: one episode of every actor

    def iterate(self):
        """one chunk -> replay -> learn -> parameters to the agent"""
        lc, B = self.lc, self.lc.replay.batch_size
        if self.algo == 'ppo':
            self.venv.ppo_rollout_into(self.agent, self.replay, self.T)
            while len(self.replay) >= B:
                self.learner.learn(self.venv.to_batch(self.replay.sample_batch(B, copy=False)))
                self.learns += 1
        else:
            self.venv.ddpg_rollout_into(self.agent, self.replay, self.T)
            if len(self.replay) >= 4 * B:
                stage = self.learner.staging_fields(B)
                for _ in range(self.T):
                    f = self.replay.sample_batch(B, out=stage)
                    self.learner.learn({'obs': {'low_dim': {'flat_inputs': f['obs']}},
                                        'obs_next': {'low_dim': {'flat_inputs': f['obs_next']}}, 'actions': f['actions'],
                                        'rewards': f['rewards'].view(B, 1), 'dones': f['dones'].view(B, 1)})
                    self.learns += 1
        self.env_steps += self.n * self.T
        self.learner.publish_parameter(self.learns, message='chunk')
        self.agent.fetch_parameter()
        if self.pn is not None:
            self.pn.refresh()                      # (the device form of on_parameter_fetched: adapt, perturb again)

    def identity(self):
        """what a saved run and the loop that goes on from it must share"""
        ident = {'algo': self.algo, 'actors': self.n, 'J': self.J, 'episode_len': self.L, 'seed': self.seed,
                 'random_resets': self.venv.resets is not None, 'heldout': self.heldout}
        if self.task != 'reach':
            ident['task'] = self.task
        if self.disturbance != 0:
            ident['disturbance'] = self.disturbance
        if self.layernorm:
            ident['layernorm'] = True
        if self.pn is not None:
            ident.update(param_noise=self.pn.type, actors_per_agent=self.pn.actors_per_agent)
        if self.double_critic:
            ident['double_critic'] = True
        if self.policy_delay != 1:
            ident['policy_delay'] = self.policy_delay
        return ident

    def population_line(self, it):
        """a plain-actor population: the deterministic return of every agent's perturbed actor on the evaluation's
        episodes (one launch over all agents), and the agents' sigmas; None for a LayerNorm population, which the
        evaluation launch does not run"""
        if self.pn is None or self.pn.ln:
            return None
        from surreal_amd.env.monitor import DeviceEvalSnapshots
        E, kw = self.snapshot_curve_args()
        returns = DeviceEvalSnapshots.from_param_noise(self.venv, self.pn).evaluate(E, **kw)      # [agents, n, E]
        return {'kind': 'population', 'algo': self.algo, 'iteration': it, 'generation': self.pn.generation,
                'agent_returns': [float(v) for v in returns.mean(dim=(1, 2)).cpu().numpy()],
                'sigma': [float(v) for v in self.pn.sigma.cpu().numpy()]}

    def state_parts(self, **script):
        """the parts of run_state.save_run: every holder's state (live tensors: save_run copies) and, under 'script',
        the loop's own counters with whatever the caller adds"""
        from surreal_amd.utils import run_state as RS
        script = dict(script, identity=self.identity(), env_steps=self.env_steps, learns=self.learns,
                      device_eval_steps=self.device_eval_steps)
        return dict(env=self.venv.state_dict(), agent=self.agent.state_dict(), eval_agent=self.eval_agent.state_dict(),
                    replay=self.replay.state_dict(), learner=self.learner.train_state_dict(),
                    torch_rng=RS.torch_rng_state(), script=script)

    def load_parts(self, parts):
        """run_state.load_run's parts into this loop's objects (ValueError: a run of another shape) -> parts['script']"""
        from surreal_amd.utils import run_state as RS
        script = parts['script']
        if script['identity'] != self.identity():
            raise ValueError('the saved run is %r, this one %r' % (script['identity'], self.identity()))
        self.learner.load_train_state_dict(parts['learner'])
        self.replay.load_state_dict(parts['replay'])
        self.venv.load_state_dict(parts['env'])
        self.agent.load_state_dict(parts['agent'])
        self.eval_agent.load_state_dict(parts['eval_agent'])
        RS.set_torch_rng_state(parts['torch_rng'])
        self.env_steps, self.learns = int(script['env_steps']), int(script['learns'])
        self.device_eval_steps = int(script['device_eval_steps'])
        return script

    def training_return(self):
        self.monitor.poll()
        return self.monitor.mean_reward(last=1)

    def evaluate(self):
        """the deterministic policy's mean episode return over the reset states of all actors (one episode, step())"""
        ag, env = self.eval_agent, self.eval_env
        ag.fetch_parameter()
        if self.heldout:
            return self._evaluate_heldout()
        env.reset()
        for _ in range(self.L):
            if self.algo == 'ppo':
                actions, _ = ag.act_batch(env.state, eps=None)
            else:
                actions = ag.model.forward_actor(env.state)
            env.step(actions)
        polled = self.eval_monitor.poll()
        assert len(polled) == self.n and all(steps == self.L for _, _, steps in polled)
        return float(np.mean([r for _, r, _ in polled]))

    def evaluate_device(self):
        """the same figure from one launch on the TRAINING env (SyntheticVecEnv.evaluate): one episode from every actor's
        reset state, or the held-out episodes 0 .. E - 1 of the stream seed + 3.  An evaluation agent that samples (the PPO
        agent under env_config.stochastic_eval, as in evaluate(): act_batch draws there) draws from a noise stream of its
        own, seed + 4, which moves on with every evaluation"""
        self.eval_agent.fetch_parameter()
        E = self.heldout or 1
        kw = {}
        if self.heldout:
            kw['resets'] = (self.seed + 3, 0)
            if self.disturbance != 0:
                kw['disturbance'] = self.disturbance
        if self.eval_agent.agent_mode in ('eval_stochastic', 'eval_stochastic_local'):
            kw['noise'] = (self.seed + 4, self.device_eval_steps)
            self.device_eval_steps += E * self.L
        returns = self.venv.evaluate(self.eval_agent, E, **kw)
        self.last_device_returns = returns           # (kept on the device: --snapshot-curve compares bits with it)
        return float(np.mean(returns.cpu().numpy()))

    def snapshot_curve_args(self):
        """(episodes, evaluate()'s keywords) of the one launch over all snapshots: the evaluation's own episodes; a
        sampling agent's draws from one fixed stream position for every snapshot"""
        kw = {}
        if self.heldout:
            kw['resets'] = (self.seed + 3, 0)
            if self.disturbance != 0:
                kw['disturbance'] = self.disturbance
        if self.eval_agent.agent_mode in ('eval_stochastic', 'eval_stochastic_local'):
            kw['noise'] = (self.seed + 4, 0)
        return self.heldout or 1, kw

    def _evaluate_heldout(self):
        """the same over the held-out episodes 0 .. E - 1 of every actor: the stream's index goes back to 0, reset()
        begins episode 0 and the closing steps draw the next ones inside their launches"""
        ag, env, E = self.eval_agent, self.eval_env, self.heldout
        env.resets.episode = 0
        env.reset()
        for _ in range(E * self.L):
            if self.algo == 'ppo':
                actions, _ = ag.act_batch(env.state, eps=None)
            else:
                actions = ag.model.forward_actor(env.state)
            env.step(actions)
        polled = self.eval_monitor.poll()
        assert len(polled) == E * self.n and all(steps == self.L for _, _, steps in polled)
        assert env.resets.episode == E + 1
        return float(np.mean([r for _, r, _ in polled]))


def train(algo, actors=64, J=2, episode_len=50, iters=None, seed=0, eval_every=10, device=None, log=print,
          random_resets=False, heldout_episodes=4, eval_heldout=False, device_eval=False, snapshot_curve=False,
          save=None, save_every=None, resume=None, layernorm=False, param_noise=None, actors_per_agent=4, task='reach',
          disturbance=0.0, double_critic=False, policy_delay=1):
    """-> (the baselines, the curve: one dict per evaluation).  random_resets / eval_heldout / device_eval / save /
    save_every (in chunks) / resume / layernorm / param_noise / actors_per_agent / task / double_critic / policy_delay: the
    module docstring's"""
    from surreal_amd.utils import run_state as RS
    iters = DEFAULT_ITERS[algo] if iters is None else iters
    heldout = int(heldout_episodes) if (random_resets or eval_heldout) else 0
    disturbance = float(TK.check_disturbance('--disturbance', disturbance))
    if disturbance != 0 and not random_resets:
        raise ValueError('--disturbance: the draws come from the reset streams: with --random-resets only')
    if snapshot_curve and (save or resume):
        raise ValueError('--snapshot-curve keeps its snapshots outside the saved run: not with --save / --resume')
    if (layernorm or param_noise) and (device_eval or snapshot_curve):
        raise ValueError('--layernorm / --param-noise: not with --device-eval / --snapshot-curve (the evaluation launch '
                         'runs a plain actor without an attached parameter noise)')
    if save_every is not None and (not save or int(save_every) < 1):
        raise ValueError('--save-every K: a positive number of chunks, with --save PATH')
    parts = RS.load_run(resume) if resume else None
    if parts is not None:
        base = parts['script']['base']               # (the baselines of the saved run: not computed, not printed again)
    elif heldout:
        base = dict(heldout_baselines(J, episode_len, actors, seed + 3, heldout, task, disturbance), algo=algo,
                    actors=actors, J=J, episode_len=episode_len, iters=iters, seed=seed, random_resets=bool(random_resets),
                    heldout_episodes=heldout)
        if disturbance != 0:
            base['disturbance'] = disturbance
    else:
        base = dict(baselines(J, episode_len, range(actors), task), algo=algo, actors=actors, J=J, episode_len=episode_len,
                    iters=iters, seed=seed)
    if parts is None:
        if task != 'reach':
            base['task'] = task
        if double_critic:
            base['double_critic'] = True
        if policy_delay != 1:
            base['policy_delay'] = policy_delay
        log(json.dumps(base))
    variant = {}
    if layernorm or param_noise:
        variant = dict(layernorm=layernorm, param_noise=param_noise, actors_per_agent=actors_per_agent)
    if task != 'reach':
        variant['task'] = task
    if disturbance != 0:
        variant['disturbance'] = disturbance
    if double_critic or policy_delay != 1:
        variant.update(double_critic=double_critic, policy_delay=policy_delay)
    loop = Loop(algo, actors, J, episode_len, seed, device, random_resets=random_resets, heldout=heldout, **variant)
    first = int(loop.load_parts(parts)['iteration']) if parts is not None else 0
    if first > iters:
        raise ValueError('the saved run has done %d chunks, --iters is %d' % (first, iters))
    gap = base['pd_return'] - base['zero_action_return']
    curve, t0 = [], time.time()
    points = [it for it in range(iters + 1) if it % eval_every == 0 or it == iters]
    snaps = loop.venv.eval_snapshots(loop.eval_agent, len(points)) if snapshot_curve else None
    per_point = []                                   # (--device-eval: the per-point launches' returns, on the device)
    for it in range(first, iters + 1):
        if it % eval_every == 0 or it == iters:
            extra = {}
            if device_eval:
                t1 = time.time()
                ev = loop.evaluate_device()
                t2 = time.time()
                per_step = loop.evaluate()
                extra = {'eval_return_per_step': per_step, 'eval_device_s': round(t2 - t1, 4),
                         'eval_per_step_s': round(time.time() - t2, 4)}
            else:
                ev = loop.evaluate()
            curve.append({'algo': algo, 'iteration': it, 'env_steps': loop.env_steps, 'learner_iterations': loop.learns,
                          'training_return': loop.training_return(), 'eval_return': ev,
                          'gap_closed': (ev - base['zero_action_return']) / gap, 'wall_s': round(time.time() - t0, 3)})
            curve[-1].update(extra)
            log(json.dumps(curve[-1]))
            pop = loop.population_line(it)
            if pop is not None:
                log(json.dumps(pop))
                curve[-1]['population'] = pop
            if snaps is not None:
                snaps.store(len(curve) - 1)          # (both evaluations fetched: the parameters they ran)
                if device_eval:
                    per_point.append(loop.last_device_returns)
        if it < iters:
            loop.iterate()
            if save and (it + 1 == iters or (save_every is not None and (it + 1) % int(save_every) == 0)):
                RS.save_run(save, **loop.state_parts(iteration=it + 1, base=base))
    if snaps is not None:
        E, kw = loop.snapshot_curve_args()
        t1 = time.time()
        returns = snaps.evaluate(E, **kw)            # [points, n, E]: ONE launch
        means = returns.mean(dim=(1, 2)).cpu().numpy()
        line = {'kind': 'snapshot_curve', 'algo': algo, 'points': len(points), 'iterations': points, 'episodes': E,
                'mean_return': [float(v) for v in means], 'wall_s': round(time.time() - t1, 4), 'bits_match': None}
        if device_eval and 'noise' not in kw:
            for k, want in enumerate(per_point):
                assert torch.equal(returns[k].view(torch.int64), want.view(torch.int64)), \
                    'snapshot %d (iteration %d) does not have the bits of its per-point evaluation' % (k, points[k])
            line['bits_match'] = True
        log(json.dumps(line))
        curve.append(line)
    return base, curve


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--algo', choices=['ppo', 'ddpg'], required=True)
    ap.add_argument('--task', choices=['reach', 'arm'], default='reach', help='the task the loop trains on')
    ap.add_argument('--actors', type=int, default=64)
    ap.add_argument('--J', type=int, default=2)
    ap.add_argument('--episode-len', type=int, default=50)
    ap.add_argument('--iters', type=int, default=None)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--eval-every', type=int, default=10)
    ap.add_argument('--out', default=None, help='append the lines to this file too')
    ap.add_argument('--random-resets', action='store_true', help='draw every training episode from a reset stream; '
                    'evaluate on held-out episodes of another stream')
    ap.add_argument('--heldout-episodes', type=int, default=4, help='held-out episodes per actor of an evaluation')
    ap.add_argument('--eval-heldout', action='store_true', help='fixed resets in training, held-out episodes in evaluation')
    ap.add_argument('--device-eval', action='store_true', help='evaluate in one launch on the training env; the curve '
                    'lines also carry the per-step figure')
    ap.add_argument('--snapshot-curve', action='store_true', help='store a parameter snapshot at every evaluation point '
                    'and evaluate all of them in one launch after training')
    ap.add_argument('--save', default=None, metavar='PATH', help='write the whole run into this file after the last '
                    'chunk (and after every K-th: --save-every)')
    ap.add_argument('--save-every', type=int, default=None, metavar='K', help='also save after every K-th chunk')
    ap.add_argument('--resume', default=None, metavar='PATH', help='go on from a file written by --save')
    ap.add_argument('--layernorm', action='store_true', help='DDPG: LayerNorm actor and critic (use_layernorm)')
    ap.add_argument('--param-noise', choices=['normal', 'adaptive_normal'], default=None,
                    help='DDPG: parameter-space noise on the device, one perturbed actor per agent')
    ap.add_argument('--actors-per-agent', type=int, default=4, metavar='K', help='actors that share a perturbation')
    ap.add_argument('--disturbance', type=float, nargs='?', const=DEFAULT_DISTURBANCE, default=0.0, metavar='S',
                    help='per-step disturbances of scale S in [0, 1] on the training and the held-out episodes '
                    '(needs --random-resets; without a value: %g)' % DEFAULT_DISTURBANCE)
    ap.add_argument('--double-critic', action='store_true', help="DDPG: TD3's second critic, on the row schedule")
    ap.add_argument('--policy-delay', type=int, default=1, metavar='D',
                    help='DDPG: the actor and the targets move once per D learner iterations')
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    train(args.algo, args.actors, args.J, args.episode_len, args.iters, args.seed, args.eval_every, log=log,
          random_resets=args.random_resets, heldout_episodes=args.heldout_episodes, eval_heldout=args.eval_heldout,
          device_eval=args.device_eval, snapshot_curve=args.snapshot_curve, save=args.save, save_every=args.save_every,
          resume=args.resume, layernorm=args.layernorm, param_noise=args.param_noise,
          actors_per_agent=args.actors_per_agent, task=args.task, disturbance=args.disturbance,
          double_critic=args.double_critic, policy_delay=args.policy_delay)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
