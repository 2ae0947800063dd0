"""
Resuming a device-resident run from one file (surreal_amd/utils/run_state.py), shared by the CPU tier
(test_run_state_cpu.py) and the GPU tier (test_gpu_run_state.py): the six loops, built as scripts/train_reach.py's Loop
builds its own -- env, training and evaluation agent, learner, replay, monitor, device noise, random resets on `reach` --
and what is recorded after every chunk.  No test functions here.

Shapes: the (32, 32) policies of device_eval_cases.py; n = 6 actors -- one full 4-row workgroup and a ragged one --,
chunks of T = 7 steps, episodes of 10: the cut after M = 3 chunks (step 21) falls mid-episode and mid-window.  Case 6 has
8 actors: a DeviceParamNoise agent spans a multiple of 4 actors, which must divide n.

Every comparison is an equality of bytes (`diff`): no tolerance anywhere.

What a record holds: the learner's train_state_dict(), the replay's state_dict() (tables, cursors, counters), the env's
state_dict(), monitor.poll(), and -- where the evaluation launch takes the policy (not a LayerNorm actor, an attached
parameter noise or per-actor clocks: SyntheticVecEnv.can_evaluate) -- the fp64 [n, 2] result of venv.evaluate(eval_agent, 2,
resets=...); the other cases record None there.
"""
import collections
import math

import numpy as np
import torch

import ddpg_rollout_cases as DC
import ppo_window_cases as PW
from surreal_amd.utils import run_state as RS

M, T, EPISODE = 3, 7, 10
N_ACTORS = 6
HIDDEN = (32, 32)
RNN = 10                                   # logical LSTM units (padded to 12), as device_eval_cases.RNN
NSEED = 0x9E3779B97F4A7C15                 # the noise stream's seed
RSEED = 0xC2B2AE3D27D4EB4F                 # the training reset stream's
ESEED = 0x165667B19E3779F9                 # the held-out evaluation episodes'
PSEED = 0x27D4EB2F165667C5                 # the parameter noise's
SEED_A, SEED_B = 11, 12                    # torch.manual_seed before a build: fresh parameters differ between the two

Case = collections.namedtuple('Case', 'id algo task D A n episode_len opts')
CASES = [
    Case('ppo-mlp-clip-reach', 'ppo', 'reach', 6, 2, N_ACTORS, EPISODE, dict(mode='clip')),
    Case('ppo-lstm-adapt-reach', 'ppo', 'reach', 6, 2, N_ACTORS, EPISODE, dict(mode='adapt', rnn=RNN)),
    Case('ppo-mlp-drift-clocks', 'ppo', 'drift', 17, 6, N_ACTORS, [5, 7, 11, 6, 9, 8], dict(mode='clip')),
    Case('ddpg-ou-reach', 'ddpg', 'reach', 6, 2, N_ACTORS, EPISODE, dict(noise_type='ou_noise')),
    Case('ddpg-td3-ln-rows-drift', 'ddpg', 'drift', 17, 6, N_ACTORS, EPISODE,
         dict(layernorm=True, double_critic=True, rows=True, hard=5)),
    Case('ddpg-param-noise-drift', 'ddpg', 'drift', 17, 6, 8, EPISODE, dict(param_noise='adaptive_normal')),
]
BY_ID = {c.id: c for c in CASES}


def ppo_configs(c, folder='surreal_amd_run_state'):
    """(n_step, stride) = (4, 3), FIFO of 64, batch 6; a publish every second learn (exp_interval 12), so some chunks
    end between two publishes; a learning rate that anneals, so the schedulers cross the cut"""
    lc, ec, sc = PW.configs(c.D, c.A, 4, 3, HIDDEN, c.opts.get('rnn'), True, memory_size=64, batch_size=6)
    lc.algo.ppo_mode = c.opts['mode']
    lc.algo.gamma = 0.95
    lc.algo.rnn.horizon = 2
    lc.algo.consts.epoch_policy = lc.algo.consts.epoch_baseline = 4
    lc.algo.network.lr_actor = lc.algo.network.lr_critic = 3e-3
    lc.algo.network.anneal.min_lr = 1e-4
    lc.algo.network.anneal.frames_to_anneal = 12 * 20
    lc.parameter_publish.exp_interval = 12
    ec.stochastic_eval = False                 # (the evaluation agent acts on the policy's mean)
    return lc, ec, sc


def ddpg_configs(c, folder='surreal_amd_run_state'):
    """n_step 3, a ring of 64 rows (it has wrapped before the cut: 30 rows a chunk), batch 16"""
    o = c.opts
    lc, ec, sc = DC.configs(c.D, c.A, c.n, hidden=HIDDEN, n_step=3, gamma=0.95, noise_type=o.get('noise_type', 'normal'),
                            layernorm=bool(o.get('layernorm')), memory_size=64, param_noise_type=o.get('param_noise'),
                            folder=folder)
    lc.model.critic_fc_hidden_sizes = list(HIDDEN)
    lc.algo.network.lr_actor, lc.algo.network.lr_critic = 1e-4, 1e-2
    lc.algo.network.use_double_critic = bool(o.get('double_critic'))
    if o.get('hard'):
        lc.algo.network.target_update = {'type': 'hard', 'interval': int(o['hard'])}
    else:
        lc.algo.network.target_update = {'type': 'soft', 'tau': 0.01}
    lc.replay.batch_size = 16
    if o.get('rows'):
        sc.learner.ddpg_row_schedule = True
    return lc, ec, sc


class Loop(object):
    """one case's loop, as scripts/train_reach.py's Loop: chunk() is its iterate()"""

    def __init__(self, c, init_seed, device=None, kernels=None, stream_noise=True):
        """stream_noise False: no DeviceNoise is attached -- the rollouts draw with torch.randn (kernel doubles that
        draw from no stream) and the file carries the part 'torch_rng'"""
        from surreal_amd.env.synthetic_env import SyntheticVecEnv
        torch.manual_seed(init_seed)
        np.random.seed(init_seed)
        self.c, self.stream_noise = c, stream_noise
        if c.algo == 'ppo':
            from surreal_amd.agent import PPOAgent as Agent
            from surreal_amd.learner import PPOLearner as Learner
            from surreal_amd.replay import FIFOReplay as Replay
            cfg = ppo_configs(c)
        else:
            from surreal_amd.agent import DDPGAgent as Agent
            from surreal_amd.learner.ddpg import DDPGLearner as Learner
            from surreal_amd.replay import UniformReplay as Replay
            cfg = ddpg_configs(c)
        self.cfg, self.B = cfg, cfg[0].replay.batch_size
        self.learner = Learner(*cfg)
        self.replay = Replay(*cfg)
        self.agent = Agent(*cfg, agent_id=0, agent_mode='training')
        self.eval_agent = Agent(*cfg, agent_id=1, agent_mode='eval_deterministic')
        kw = {}
        if device is not None:
            kw['device'] = device
        if kernels is not None:
            kw['kernels'] = kernels
        self.venv = SyntheticVecEnv(c.n, c.D, c.A, episode_len=c.episode_len, seeds=list(range(c.n)), task=c.task, **kw)
        self.monitor = self.venv.attach_monitor(capacity=8)
        if stream_noise:
            self.venv.attach_noise(seed=NSEED)
        if c.task == 'reach':
            self.venv.attach_resets(RSEED)
            self.venv.reset()
        # (the parameter noise before the first fetch: from then on the agent's host noise, which draws from numpy's
        # global stream at every fetch, is off)
        self.pn = None
        if c.opts.get('param_noise'):
            self.pn = self.venv.attach_param_noise(self.agent, PSEED, actors_per_agent=4)
        for ag in (self.agent, self.eval_agent):
            ag.attach_learner(self.learner)
            ag.fetch_parameter()
        if self.pn is not None:
            self.pn.refresh()
        self.learns = 0

    def chunk(self):
        """T steps of every actor -> replay -> learn -> the parameters to the agent"""
        B = self.B
        if self.c.algo == 'ppo':
            self.venv.ppo_rollout_into(self.agent, self.replay, T)
            while len(self.replay) >= B:
                self.learner.learn(self.venv.to_batch(self.replay.sample_batch(B, copy=False)))
                self.learns += 1
        else:
            self.venv.ddpg_rollout_into(self.agent, self.replay, T)
            if len(self.replay) >= B:
                stage = self.learner.staging_fields(B)
                for _ in range(T):
                    f = self.replay.sample_batch(B, out=stage)
                    self.learner.learn({'obs': {'low_dim': {'flat_inputs': f['obs']}},
                                        'obs_next': {'low_dim': {'flat_inputs': f['obs_next']}}, 'actions': f['actions'],
                                        'rewards': f['rewards'].view(B, 1), 'dones': f['dones'].view(B, 1)})
                    self.learns += 1
        self.learner.publish_parameter(self.learns, message='chunk')
        self.agent.fetch_parameter()
        if self.pn is not None:
            self.pn.refresh()                    # (on_parameter_fetched: one on each side of the cut)

    def record(self):
        """what is compared after a chunk, on the host (module docstring)"""
        polled = self.monitor.poll()
        returns = None
        self.eval_agent.fetch_parameter()
        if self.venv.can_evaluate(self.eval_agent):
            kw = {'resets': (ESEED, 0)} if self.c.task == 'reach' else {}
            returns = self.venv.evaluate(self.eval_agent, 2, **kw)
            assert returns.dtype == torch.float64 and tuple(returns.shape) == (self.c.n, 2)
        return RS.to_host({'learner': self.learner.train_state_dict(), 'replay': self.replay.state_dict(),
                           'env': self.venv.state_dict(), 'poll': polled, 'eval': returns, 'learns': self.learns})

    def run(self, chunks, save_each=None):
        """-> the records of `chunks` chunks; save_each: a path every chunk's state is saved to (a save is pure)"""
        out = []
        for _ in range(chunks):
            self.chunk()
            if save_each is not None:
                self.save(save_each)
            out.append(self.record())
        return out

    def parts(self):
        extra = {} if self.stream_noise else {'torch_rng': RS.torch_rng_state()}
        return dict(env=self.venv.state_dict(), agent=self.agent.state_dict(), eval_agent=self.eval_agent.state_dict(),
                    replay=self.replay.state_dict(), learner=self.learner.train_state_dict(),
                    loop={'learns': self.learns}, **extra)

    def save(self, path):
        RS.save_run(path, **self.parts())

    def load(self, path):
        parts = RS.load_run(path)
        self.learner.load_train_state_dict(parts['learner'])
        self.replay.load_state_dict(parts['replay'])
        self.venv.load_state_dict(parts['env'])
        self.agent.load_state_dict(parts['agent'])
        self.eval_agent.load_state_dict(parts['eval_agent'])
        self.learns = int(parts['loop']['learns'])
        if not self.stream_noise:
            RS.set_torch_rng_state(parts['torch_rng'])


# ---- equality of bytes ---------------------------------------------------------------------------------------------------

def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def diff(a, b, path='record'):
    """the paths at which two parts differ in type, shape, dtype or BYTES (floats by their bits) -> a list, empty when
    they are the same"""
    if torch.is_tensor(a) or torch.is_tensor(b):
        if not (torch.is_tensor(a) and torch.is_tensor(b)) or a.dtype != b.dtype or a.shape != b.shape:
            return ['%s: %s vs %s' % (path, _what(a), _what(b))]
        if not torch.equal(_bits(a), _bits(b)):
            return ['%s: %d of %d elements differ' % (path, int((a != b).sum()), a.numel())]
        return []
    if isinstance(a, dict) and isinstance(b, dict):
        out = [] if list(a) == list(b) else ['%s: keys %r vs %r' % (path, list(a), list(b))]
        for k in a:
            if k in b:
                out += diff(a[k], b[k], '%s[%r]' % (path, k))
        return out
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        out = [] if len(a) == len(b) else ['%s: %d vs %d entries' % (path, len(a), len(b))]
        for i, (x, y) in enumerate(zip(a, b)):
            out += diff(x, y, '%s[%d]' % (path, i))
        return out
    if isinstance(a, float) and isinstance(b, float):
        same = (math.isnan(a) and math.isnan(b)) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))
        return [] if same else ['%s: %r vs %r' % (path, a, b)]
    return [] if type(a) is type(b) and a == b else ['%s: %r vs %r' % (path, a, b)]


def _what(x):
    return '%s %s' % (tuple(x.shape), x.dtype) if torch.is_tensor(x) else type(x).__name__


def assert_same(got, want, what):
    d = diff(got, want, what)
    assert not d, '\n'.join(d[:20])


def parameters(tensors):
    """the learner's own model out of train_state_dict()['tensors']"""
    return {k: v for k, v in tensors.items() if k in ('model.flat', 'model.ac_flat')}


def learned(records):
    """the run did learn on both sides of the cut (else a resume has nothing to carry)"""
    return records[M - 1]['learns'] > 0 and records[-1]['learns'] > records[M - 1]['learns']
