"""
The device recorders (surreal_amd/env/device_recorder.py: per-actor episode clocks, smx_record_ppo_window_step_f32 /
smx_record_ddpg_nstep_step_f32) against the host wrappers they replace, shared by the CPU tier (test_recorder_cpu.py)
and the GPU tier (test_gpu_recorder.py):

  * ``ScriptedEnv`` -- an ``Env`` whose observations, rewards and reset observations are fp32 draws of a seeded
    RandomState and whose episode lengths cycle through a list, every actor from another rotation: the clocks of n of
    them diverge from the first episode on;
  * ``RecorderCpuKernels`` -- the torch-CPU double of the two entry points (a subclass of the stock double): the
    kernels' index rules, actor by actor;
  * ``host_ppo`` / ``host_ddpg`` -- n ScriptedEnv behind ExpSenderWrapperMultiStepMovingWindowWithInfo /
    ExpSenderWrapperSSARNStepBootstrap (and an EpisodeMonitor), stepped in actor order with a recorded action / pds /
    cells stream into ONE list sink -> the experiences in insertion order and the step stream the recorder is fed;
  * ``device_ppo`` / ``device_ddpg`` -- that stream through a recorder into a replay's ring.
"""
import collections
import types

import numpy as np
import torch

import helpers as H
import ppo_window_cases as PW
from cpu_kernels import TorchCpuKernels
from surreal_amd.env.base import Env


class ScriptedEnv(Env):
    """observations [D], rewards and reset observations drawn as fp32 from RandomState(seed); episode e lasts
    lengths[(rotation + e) % len(lengths)] steps (rotation: default the seed).  log: a shared list that receives
    (tag, 'reset' | 'step') in call order; the actions it was stepped with are kept in `actions`."""

    def __init__(self, seed, lengths, D=7, rotation=None, log=None, tag=None):
        self.rs = np.random.RandomState(seed)
        self.lengths = [int(x) for x in lengths]
        self.rotation = int(seed if rotation is None else rotation)
        self.D = int(D)
        self.log, self.tag = log, seed if tag is None else tag
        self.episode = self.t = 0
        self.length = None
        self.actions = []

    def _observe(self):
        return collections.OrderedDict(low_dim=collections.OrderedDict(
            flat_inputs=self.rs.standard_normal(self.D).astype(np.float32)))

    def _reset(self):
        self.length = self.lengths[(self.rotation + self.episode) % len(self.lengths)]
        self.episode += 1
        self.t = 0
        if self.log is not None:
            self.log.append((self.tag, 'reset'))
        return self._observe(), {}

    def _step(self, action):
        assert self.length is not None and self.t < self.length, 'stepped past the end of an episode'
        self.actions.append(np.array(action, copy=True))
        self.t += 1
        if self.log is not None:
            self.log.append((self.tag, 'step'))
        reward = float(np.float32(self.rs.standard_normal()))         # an fp32 value as a Python float
        return self._observe(), reward, self.t >= self.length, {}


def flat(obs):
    return np.asarray(obs['low_dim']['flat_inputs'], dtype=np.float32)


# ---- the torch-CPU double ----------------------------------------------------------------------------------------------
class RecorderCpuKernels(TorchCpuKernels):
    name = 'torch-cpu-double+recorder'

    def __init__(self):
        super().__init__()
        self.record_launches = 0

    @staticmethod
    def _account(mon, a, rew, done):
        """episode_account for actor a"""
        if mon is None:
            return
        mon.ep_reward[a] += float(rew)                 # (fp64 + widened fp32: one rounding, as the kernel)
        mon.ep_steps[a] += 1
        if done:
            slot = int(mon.ep_count[a]) % mon.capacity
            mon.done_reward[a, slot] = mon.ep_reward[a]
            mon.done_steps[a, slot] = mon.ep_steps[a]
            mon.ep_count[a] += 1
            mon.ep_reward[a] = 0.0
            mon.ep_steps[a] = 0

    @staticmethod
    def _clock(r, a):
        """(tau, rank or -1) of actor a under the kernels' guards; None: the actor is skipped"""
        tau, rank = int(r['t'][a]), int(r['rank'][a])
        if tau < 0:
            return None
        return tau, rank if 0 <= rank < int(r['rows']) else -1

    def record_ppo_window_step(self, r, copy_workgroups=0, monitor=None):
        self.record_launches += 1
        assert 0 <= copy_workgroups <= 1024
        n, D = r['cur_obs'].shape
        N, adv = int(r['n_step']), int(r['advance'])
        S = -(-N // adv)
        carry, tabs = r['carry'], r['tables']
        cap = tabs['obs'].shape[0]
        assert n <= cap and 0 <= int(r['cursor']) < cap
        hb, cb = r.get('h_before'), r.get('c_before')
        for a in range(n):
            clock = self._clock(r, a)
            if clock is None:
                continue
            tau, rank = clock
            done = bool(r['dones'][a] != 0)
            slot, j = tau % N, tau + 1 - N
            carry['obs'][a, slot] = r['cur_obs'][a]
            carry['actions'][a, slot] = r['actions'][a]
            carry['rewards'][a, slot] = r['rewards'][a]
            carry['pds'][a, slot] = r['pds'][a]
            if hb is not None and tau % adv == 0:
                carry['cells'][a, (tau // adv) % S, 0] = hb.reshape(n, -1)[a]
                carry['cells'][a, (tau // adv) % S, 1] = cb.reshape(n, -1)[a]
            if rank >= 0 and j >= 0 and j % adv == 0:
                row = (int(r['cursor']) + rank) % cap
                order = [(j + u) % N for u in range(N)]
                for k in ('obs', 'actions', 'rewards', 'pds'):
                    tabs[k][row] = carry[k][a, order].reshape(-1)
                tabs['obs_next'][row] = r['obs_next'][a]
                d = torch.zeros(N)
                d[N - 1] = 1.0 if done else 0.0
                tabs['dones'][row] = d
                if 'cells' in tabs:
                    tabs['cells'][row] = carry['cells'][a, (j // adv) % S].reshape(-1)
            r['cur_obs'][a] = r['obs_reset'][a] if done and r.get('obs_reset') is not None else r['obs_next'][a]
            self._account(monitor, a, r['rewards'][a], done)

    def record_ddpg_nstep_step(self, r, monitor=None):
        self.record_launches += 1
        n, D = r['cur_obs'].shape
        N = int(r['n_step'])
        carry, tabs, gpow = r['carry'], r['tables'], r['gpow']
        cap = tabs['obs'].shape[0]
        assert n <= cap and 0 <= int(r['cursor']) < cap
        for a in range(n):
            clock = self._clock(r, a)
            if clock is None:
                continue
            tau, rank = clock
            done = bool(r['dones'][a] != 0)
            slot = tau % N
            carry['obs'][a, slot] = r['cur_obs'][a]
            carry['actions'][a, slot] = r['actions'][a]
            carry['rewards'][a, slot] = r['rewards'][a]
            if rank >= 0 and tau >= N - 1:
                row = (int(r['cursor']) + rank) % cap
                j = tau - N + 1
                R = carry['rewards'][a, j % N].double()
                for u in range(j + 1, tau + 1):                       # nstep_reward: fp64, in step order
                    e = (u - j) if u >= N - 1 else (N - 1 - j)
                    R = R + gpow[e] * carry['rewards'][a, u % N].double()
                tabs['obs'][row] = carry['obs'][a, j % N]
                tabs['actions'][row] = carry['actions'][a, j % N]
                tabs['obs_next'][row] = r['obs_next'][a]
                tabs['rewards'][row] = R.float()
                tabs['dones'][row] = 1.0 if done else 0.0
            r['cur_obs'][a] = r['obs_reset'][a] if done and r.get('obs_reset') is not None else r['obs_next'][a]
            self._account(monitor, a, r['rewards'][a], done)


# ---- the host side: n wrappers, one sink -------------------------------------------------------------------------------
def _drive(n, D, lengths, steps, seed, wrap, act):
    """n ScriptedEnv (seeds seed + a, rotations a) behind EpisodeMonitor and `wrap`, stepped in actor order for `steps`
    steps with act(s, a) -> the wrapper's action argument; one list sink in insertion order"""
    from surreal_amd.env import EpisodeMonitor
    exps, monitors, ws = [], [], []
    for a in range(n):
        mon = EpisodeMonitor(ScriptedEnv(seed + a, lengths, D, rotation=a))
        monitors.append(mon)
        ws.append(wrap(mon, exps.append))
    s = types.SimpleNamespace(n=n, D=D, steps=steps, exps=exps, monitors=monitors,
                              first=np.stack([flat(w.reset()[0]) for w in ws]),
                              obs_next=np.zeros((steps, n, D), np.float32), obs_reset=np.zeros((steps, n, D), np.float32),
                              rewards=np.zeros((steps, n), np.float32), dones=np.zeros((steps, n), bool), count=[])
    for step in range(steps):
        for a, w in enumerate(ws):
            obs, reward, done, _ = w.step(act(step, a))
            s.obs_next[step, a], s.rewards[step, a], s.dones[step, a] = flat(obs), reward, done
            assert float(s.rewards[step, a]) == reward                # (the reward stream is fp32-exact)
            if done:
                s.obs_reset[step, a] = flat(w.reset()[0])
        s.count.append(len(exps))                                     # experiences inserted up to and including `step`
    return s


def host_ppo(n, D, A, lengths, steps, n_step, stride, rnn_hidden=0, seed=0):
    """-> the stream (first, actions, pds, h / c, obs_next, rewards, dones, obs_reset, count, monitors) and
    `fields`: {field: np [windows, ...]} of the emitted windows in insertion order, in the replay's shapes"""
    from surreal_amd.env import ExpSenderWrapperMultiStepMovingWindowWithInfo
    lc, ec, sc = PW.configs(D, A, n_step, stride, rnn_hidden=rnn_hidden or None)
    rs = np.random.RandomState(1000 + seed)
    actions = rs.uniform(-1, 1, (steps, n, A)).astype(np.float32)
    pds = rs.standard_normal((steps, n, 2 * A)).astype(np.float32)
    h = rs.standard_normal((steps, n, rnn_hidden)).astype(np.float32)
    c = rs.standard_normal((steps, n, rnn_hidden)).astype(np.float32)

    def act(s, a):
        once = [h[s, a][None].copy(), c[s, a][None].copy()] if rnn_hidden else []
        return actions[s, a].copy(), [once, [pds[s, a].copy()]]
    st = _drive(n, D, lengths, steps, seed,
                lambda env, sink: ExpSenderWrapperMultiStepMovingWindowWithInfo(env, lc, sc, sink=sink), act)
    st.A, st.actions, st.pds, st.h, st.c, st.rnn_hidden = A, actions, pds, h, c, rnn_hidden
    x = st.exps
    f = {'obs': [[flat(o) for o in e['obs']] for e in x], 'obs_next': [[flat(e['obs_next'])] for e in x],
         'actions': [e['actions'] for e in x], 'rewards': [e['rewards'] for e in x], 'dones': [e['dones'] for e in x],
         'pds': [[p[0] for p in e['persistent_infos']] for e in x]}
    if rnn_hidden:
        f['cells'] = [e['onetime_infos'] for e in x]                  # [2, 1, Hl]
    shapes = {'obs': (n_step, D), 'obs_next': (1, D), 'actions': (n_step, A), 'rewards': (n_step,), 'dones': (n_step,),
              'pds': (n_step, 2 * A), 'cells': (2, 1, rnn_hidden)}
    st.fields = {k: np.asarray(v, dtype=np.float32).reshape((len(x),) + shapes[k]) for k, v in f.items()}
    return st


def host_ddpg(n, D, A, lengths, steps, n_step, gamma, seed=0):
    """as host_ppo for ExpSenderWrapperSSARNStepBootstrap: fields obs / obs_next [rows, D], actions [rows, A], rewards /
    dones [rows] -- a reward is np.float32 of the wrapper's Python float"""
    import ddpg_rollout_cases as DC
    from surreal_amd.env import ExpSenderWrapperSSARNStepBootstrap
    lc, ec, sc = DC.configs(D, A, n, n_step=n_step, gamma=gamma, folder='surreal_amd_recorder')
    actions = np.random.RandomState(2000 + seed).uniform(-1, 1, (steps, n, A)).astype(np.float32)
    st = _drive(n, D, lengths, steps, seed, lambda env, sink: ExpSenderWrapperSSARNStepBootstrap(env, lc, sc, sink=sink),
                lambda s, a: actions[s, a].copy())
    st.A, st.actions = A, actions
    x = st.exps
    st.fields = {'obs': np.asarray([flat(e['obs'][0]) for e in x], np.float32).reshape(len(x), D),
                 'obs_next': np.asarray([flat(e['obs'][1]) for e in x], np.float32).reshape(len(x), D),
                 'actions': np.asarray([e['action'] for e in x], np.float32).reshape(len(x), A),
                 'rewards': np.asarray([np.float32(e['reward']) for e in x], np.float32),
                 'dones': np.asarray([float(e['done']) for e in x], np.float32)}
    return st


# ---- the device side ---------------------------------------------------------------------------------------------------
def _dev(x):
    from surreal_amd import kernels as KN
    return torch.as_tensor(np.ascontiguousarray(x)).to(KN.default_device())


def device_ppo(st, replay, n_step, stride, monitor=None, resume_at=(), copy_workgroups=0, as_tensors=False, on_step=None):
    """the stream of host_ppo through a DeviceWindowRecorder into `replay` -> (recorder, rows).  resume_at: steps before
    which the recorder is replaced by a new one loaded from its state_dict; as_tensors: rewards / obs_next / obs_reset
    go in as device tensors instead of host arrays; on_step(step, rows of the step) after every record()"""
    from surreal_amd.env import DeviceWindowRecorder
    make = lambda: DeviceWindowRecorder(st.n, st.D, st.A, n_step, stride, rnn_hidden=st.rnn_hidden)  # noqa: E731
    rec = make()
    rec.begin(st.first)
    total = 0
    put = _dev if as_tensors else (lambda x: x)
    for s in range(st.steps):
        if s in resume_at:
            sd = rec.state_dict()
            rec = make()
            rec.load_state_dict(sd)
        cells = (_dev(st.h[s]), _dev(st.c[s])) if st.rnn_hidden else None
        rows = rec.record(replay, _dev(st.actions[s]), _dev(st.pds[s]), put(st.rewards[s]), st.dones[s],
                          put(st.obs_next[s]), put(st.obs_reset[s]) if st.dones[s].any() or as_tensors else None,
                          cells_before=cells, monitor=monitor, copy_workgroups=copy_workgroups)
        total += rows
        if on_step is not None:
            on_step(s, rows)
    return rec, total


def device_ddpg(st, replay, n_step, gamma, monitor=None, resume_at=()):
    from surreal_amd.env import DeviceNStepRecorder
    make = lambda: DeviceNStepRecorder(st.n, st.D, st.A, n_step, gamma)  # noqa: E731
    rec = make()
    rec.begin(st.first)
    total = 0
    for s in range(st.steps):
        if s in resume_at:
            sd = rec.state_dict()
            rec = make()
            rec.load_state_dict(sd)
        total += rec.record(replay, _dev(st.actions[s]), st.rewards[s], st.dones[s], st.obs_next[s],
                            st.obs_reset[s] if st.dones[s].any() else None, monitor=monitor)
    return rec, total


def fifo(D, A, n_step, stride, memory_size, rnn_hidden=0):
    from surreal_amd.replay import FIFOReplay
    lc, ec, sc = PW.configs(D, A, n_step, stride, rnn_hidden=rnn_hidden or None, memory_size=memory_size,
                            batch_size=min(64, memory_size))
    return FIFOReplay(lc, ec, sc)


def uniform(D, A, n, n_step, gamma, memory_size):
    import ddpg_rollout_cases as DC
    from surreal_amd.replay import UniformReplay
    lc, ec, sc = DC.configs(D, A, n, n_step=n_step, gamma=gamma, memory_size=memory_size, folder='surreal_amd_recorder')
    return UniformReplay(lc, ec, sc)


def expected_ring(fields, capacity, cursor0=0):
    """experience i of `fields` at row (cursor0 + i) % capacity of a zeroed ring, in insertion order (later ones
    overwrite) -> {field: np [capacity, width]}"""
    ring = {}
    for k, v in fields.items():
        rows = v.reshape(v.shape[0], int(np.prod(v.shape[1:])))
        ring[k] = np.zeros((capacity, rows.shape[1]), np.float32)
        for i in range(rows.shape[0]):
            ring[k][(cursor0 + i) % capacity] = rows[i]
    return ring


def assert_ring_equals(replay, fields, capacity, cursor0=0):
    """bit for bit: torch.equal per field"""
    got = H.device_ring(replay)
    want = expected_ring(fields, capacity, cursor0)
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in want:
        g, w = torch.as_tensor(got[k]), torch.as_tensor(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert torch.equal(g, w), (k, np.argwhere(got[k] != want[k])[:5].tolist())


def check_ring_wrap(n=5, D=7, A=3, n_step=4, stride=3, steps=60, lengths=(2, 4, 9, 5, 14), memory_size=13):
    """a FIFO of memory_size 13 (capacity 16): the first step on which several actors close finds the cursor on the
    ring's last row, so its rows straddle the end; the oldest rows are dropped as the ring fills.  The popped
    sample_batch must equal that of a second FIFO fed the same experiences through insert_batch, step by step"""
    cap = memory_size + 3
    st = host_ppo(n, D, A, lengths, steps, n_step, stride)
    per_step = np.diff([0] + st.count)
    several = int(np.flatnonzero(per_step > 1)[0])                    # (there is such a step: the clocks coincide)
    pre = (cap - 1 - int(st.count[several] - per_step[several])) % cap
    replay, host = fifo(D, A, n_step, stride, memory_size), fifo(D, A, n_step, stride, memory_size)
    for r in (replay, host):                                          # move both cursors to row `pre`, nothing stored
        for _ in range(pre):
            r.insert_batch({k: torch.zeros((1,) + v.shape[1:], device=_dev(np.zeros(1)).device)
                            for k, v in st.fields.items()})
            r.sample_batch(1)
        assert (r._head, r._count) == (pre, 0)
    seen = []

    def feed_host(step, rows):
        lo, hi = (st.count[step - 1] if step else 0), st.count[step]
        assert hi - lo == rows
        cursor = (host._head + host._count) % cap
        seen.append(rows > 1 and cursor + rows > cap)
        if rows:
            host.insert_batch({k: _dev(v[lo:hi]) for k, v in st.fields.items()})
    device_ppo(st, replay, n_step, stride, on_step=feed_host)
    assert seen[several] and len(st.exps) > cap
    assert (replay._head, replay._count) == (host._head, host._count) and host._count == cap
    got, want = replay.sample_batch(memory_size), host.sample_batch(memory_size)
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def assert_monitor_equals_host(mon, st):
    """the polled (fp64 reward sum, steps) of every finished episode, per actor, against the host EpisodeMonitors"""
    mon.poll()
    assert mon.dropped == 0
    for a, host in enumerate(st.monitors):
        assert mon.episode_rewards[a] == host.episode_rewards, a
        assert mon.episode_steps[a] == host.episode_steps, a
    assert mon.num_episodes == sum(m.num_episodes for m in st.monitors) > 0


def brute_force_ranks(closes):
    """rank by counting, actor by actor"""
    rank, k = [], 0
    for c in closes:
        rank.append(k if c else -1)
        k += bool(c)
    return rank, k
