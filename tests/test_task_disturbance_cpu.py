"""CPU tier: the per-step disturbance of `reach` and `arm` (surreal_amd/env/tasks.py: disturbance; struct smx_reset_stream's
scale).  The host draw against the tests' own Philox (philox_ref, which reproduces the Random123 vectors); the steps with
scale 0 against today's bytes and with a scale against the written formula; SyntheticEnv(disturbance=) against the torch-CPU
double through every route -- the per-step call, PPO windows (MLP, LSTM), the four DDPG actors --, cuts into calls, split
envs; what evaluate() hands its launch; state_dict; every refusal, with the target unchanged after the raise; the entry
points' argument checks, which run before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import device_eval_cases as EV
import philox_ref as PR
import reach_resets_cases as RR
import rollout_envelope_cases as EC
import task_disturbance_cases as TD
from surreal_amd import _lib as L
from surreal_amd import kernels as KN
from surreal_amd.env import tasks as TK
from surreal_amd.env.synthetic_env import SyntheticEnv, SyntheticVecEnv

bits = TD.bits
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -5              # include/surreal_amd.h: SMX_E_NULL, SMX_E_SHAPE, SMX_E_ALIGN


@pytest.fixture
def double():
    prev = KN.set_default_kernels(TD.DisturbedCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


# ---- the host definition -------------------------------------------------------------------------------------------------

def test_header_codes_are_the_ones_used_here():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'surreal_amd.h')).read()
    for name, v in (('SMX_E_NULL', E_NULL), ('SMX_E_SHAPE', E_SHAPE), ('SMX_E_ALIGN', E_ALIGN)):
        assert int(re.search(r'%s = (-?\d+)' % name, hdr).group(1)) == v


def test_draw_is_the_written_rule_word_for_word():
    """counter (g, low32(e), t, 0x44530000 | j >> 2), word j & 3, 24 bits, scaled, minus one -- from the tests' own Philox,
    whose known answers are Random123's (test_reach_resets_cpu.py)"""
    assert len(PR.KAT) >= 3
    for counter, key, want in PR.KAT:
        assert [int(v) for v in PR.philox4x32_10(list(counter), list(key))] == [int(v) for v in want]
    seed = 0x0123456789ABCDEF
    for g, e, t, J in ((0, 0, 0, 1), (2 ** 32 - 1, 2 ** 32 - 1, 4, 30), (7, 3, 2 ** 31, 21), (5, 1, 1, 5)):
        got = TK.disturbance(seed, g, e, t, J)
        assert got.dtype == np.float32 and got.shape == (J,)
        for j in range(J):
            x = PR.philox4x32_10([g, e, t, 0x44530000 | (j >> 2)], [seed & 0xFFFFFFFF, seed >> 32])
            want = np.float32(int(x[j & 3]) >> 8) * np.float32(2.0 ** -23) - np.float32(1.0)
            assert bits(got[j], want), (g, e, t, j)
    assert TK.DISTURB_TAG == 0x44530000 != TK.RESET_TAG


def test_draws_are_multiples_of_2_to_the_minus_23_in_the_half_open_interval_and_pure():
    g, e, t = np.arange(40)[:, None, None], np.arange(3)[None, :, None], np.arange(5)[None, None, :]
    w = TK.disturbance(11, g, e, t, 21)
    assert w.shape == (40, 3, 5, 21) and w.dtype == np.float32
    assert (w >= -1.0).all() and (w < 1.0).all()
    k = (w.astype(np.float64) + 1.0) * 2.0 ** 23
    assert (k == np.round(k)).all() and len(np.unique(w)) > 0.99 * w.size
    assert abs(float(w.mean())) < 0.02 and abs(float(w.var()) - 1.0 / 3.0) < 0.02
    # a pure function of (seed, actor, episode, step, j): broadcasting, J and the neighbours change nothing
    assert bits(w[7, 2, 3], TK.disturbance(11, 7, 2, 3, 21)) and bits(w[7, 2, 3, :5], TK.disturbance(11, 7, 2, 3, 5))
    assert not bits(w[7, 2, 3], TK.disturbance(12, 7, 2, 3, 21)) and not bits(w[7, 2, 3], w[7, 2, 4])
    # other blocks than the reset stream's rows of the same (seed, actor, episode)
    assert not bits(TK.disturbance(11, 7, 2, 0, 3), TK.reach_reset_state(11, 7, 2, 1))
    for bad in (dict(actor=-1), dict(actor=2 ** 32), dict(episode=-1), dict(episode=2 ** 32), dict(t=-1), dict(t=2 ** 32)):
        kw = dict(dict(actor=0, episode=0, t=0), **bad)
        with pytest.raises(ValueError, match=r'in \[0, 2\^32\)'):
            TK.disturbance(11, kw['actor'], kw['episode'], kw['t'], 3)
    with pytest.raises(ValueError, match='64 bits'):
        TK.disturbance(1 << 64, 0, 0, 0, 3)


@pytest.mark.parametrize('task,J', [('reach', 1), ('reach', 5), ('reach', 21), ('arm', 1), ('arm', 5), ('arm', 30)])
def test_steps_with_scale_zero_are_todays_bytes_and_with_a_scale_the_formula(task, J):
    rs = np.random.RandomState(J)
    n, D = 9, TD.obs_dim(task, J)
    s = rs.uniform(-1, 1, size=(n, D)).astype(np.float32)
    a = rs.uniform(-1.5, 1.5, size=(n, J)).astype(np.float32)
    s[0, J:2 * J], a[0] = -0.0, 0.0                  # v = -0.0, a = 0
    s[2, J:2 * J], a[2] = -0.0, -0.0                 # v = a = -0.0: 0.9f * -0 + 0.2f * -0 = -0, which `+ 0` would lose
    s[1, J:2 * J], a[1] = 0.999, 1.5                 # the clamp binds
    step = TK.STEP[task]
    w = TK.disturbance(3, np.arange(n), 1, 2, J)
    plain = step(s, a)
    for zero in (step(s, a, w=None, scale=0.0), step(s, a, w=w, scale=0.0), step(s, a, w=w, scale=np.float32(-0.0))):
        assert bits(zero[0], plain[0]) and bits(zero[1], plain[1])
    assert np.signbit(plain[0][2, J:2 * J]).all() and (plain[0][2, J:2 * J] == 0).all()
    assert not np.signbit(plain[0][0, J:2 * J]).any() and (plain[0][0, J:2 * J] == 0).all()
    # the written formula, by hand
    sc = np.float32(0.3)
    decay, gain = (np.float32(0.9), np.float32(0.2)) if task == 'reach' else (np.float32(0.9), np.float32(0.4))
    ac = np.clip(a, -1, 1).astype(np.float32)
    vn = ((decay * s[:, J:2 * J]).astype(np.float32) + (gain * ac).astype(np.float32)).astype(np.float32)
    vn = np.clip((vn + (sc * w).astype(np.float32)).astype(np.float32), -1, 1).astype(np.float32)
    got, rew = step(s, a, w=w, scale=0.3)
    assert got.dtype == rew.dtype == np.float32 and bits(got[:, J:2 * J], vn) and not bits(got, plain[0])
    assert (np.abs(got[1, J:2 * J]) <= 1.0).all()
    # everything downstream of v' / omega' is the undisturbed step's: a step FROM the state with v' in place and a == 0 ...
    dt = np.float32(0.1) if task == 'reach' else np.float32(0.2)
    lim = np.float32(10.0) if task == 'reach' else TK.ARM_PI
    assert bits(got[:, :J], np.clip((s[:, :J] + (dt * vn).astype(np.float32)).astype(np.float32), -lim, lim))
    assert bits(got[:, 2 * J:], s[:, 2 * J:])
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
        step(s, a, w=w, scale=1.5)
    with pytest.raises(ValueError, match='takes its draws'):
        step(s, a, scale=0.5)


# ---- the host env ---------------------------------------------------------------------------------------------------------------

def test_host_env_draws_per_episode_and_step_and_refuses():
    for task, J in (('reach', 2), ('arm', 5)):
        D = TD.obs_dim(task, J)
        h = SyntheticEnv(D, J, episode_len=3, task=task, resets=(9, 4), disturbance=0.25)
        plain = SyntheticEnv(D, J, episode_len=3, task=task, resets=(9, 4))
        with pytest.raises(ValueError, match='stepped from a reset'):
            h._step(np.zeros(J, np.float32))
        assert h.t == 0 and h.episode == 0
        o, _ = h._reset()
        plain._reset()
        s = o['low_dim']['flat_inputs']
        act = np.full(J, 0.5, np.float32)
        for e in range(2):
            for t in range(3):
                want, r = TK.STEP[task](s, act, w=TK.disturbance(9, 4, e, t, J), scale=0.25)
                o, got_r, done, _ = h._step(act)
                assert bits(o['low_dim']['flat_inputs'], want) and got_r == float(r) and done == (t == 2)
                s = want
            o, _ = h._reset()
            s = o['low_dim']['flat_inputs']
            assert bits(s, TK.RESET_STATE[task](9, 4, e + 1, J))
        o2, _, _, _ = plain._step(act)
        assert not bits(o2['low_dim']['flat_inputs'], TK.STEP[task](TK.RESET_STATE[task](9, 4, 0, J), act,
                                                                  w=TK.disturbance(9, 4, 0, 0, J), scale=0.25)[0])
    with pytest.raises(ValueError, match='resets='):
        SyntheticEnv(6, 2, task='reach', disturbance=0.1)
    with pytest.raises(ValueError, match='takes no disturbance'):
        SyntheticEnv(17, 6, disturbance=0.1)
    for bad in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match=r'\[0, 1\]'):
            SyntheticEnv(6, 2, task='reach', resets=(1, 0), disturbance=bad)
    zero = SyntheticEnv(6, 2, episode_len=3, task='reach', resets=(9, 4), disturbance=0.0)
    zero._step(np.zeros(2, np.float32))               # (an undisturbed env steps without a reset, as before)


# ---- the double against the host step through every route ----------------------------------------------------------------------

@pytest.mark.parametrize('c', TD.CASES, ids=lambda c: c.id)
def test_recorded_rows_are_the_host_step_with_the_host_draws(c, double):
    x = TD.setup(c, 'cpu', double)
    got, rows = TD.run(x)
    assert x.resets.episode == 1 + sum(TD.CALLS) // TD.EP and x.resets.disturbance == TD.SCALE
    returns = TD.check_rows(got, x, rows)
    assert TD.draws_move_the_rows(got, x, rows)
    if returns is not None:
        assert returns == [r[:2] for r in TD.AC.monitor_returns(x.venv.monitor, x.c.n)] and all(len(r) == 2 for r in returns)


@pytest.mark.parametrize('task,J', [('reach', 2), ('arm', 5)])
@pytest.mark.parametrize('variant', [dict(), dict(layernorm=True), dict(param_noise='normal', n=8),
                                     dict(layernorm=True, param_noise='normal', n=8)], ids=['plain', 'ln', 'pop', 'popln'])
def test_ddpg_actors_against_host_chains(task, J, variant, double):
    got, want = TD.whole_steps('cpu', double, task=task, J=J, **variant)
    assert got == want and all(len(r) == 2 for r in got)
    assert double.routes[-1]['resets'][3] == TD.SCALE


@pytest.mark.parametrize('task,J', [('reach', 1), ('reach', 21), ('arm', 2), ('arm', 30)])
def test_per_step_call_against_host_envs(task, J, double):
    TD.per_step_chains('cpu', double, task, J, n=6)


@pytest.mark.parametrize('cid', ['reach-window-J5', 'reach-ddpg-J2', 'arm-lstm_window-J5', 'arm-ddpg-J30'])
def test_cuts_into_calls_and_split_envs_leave_the_same_bytes(cid, double):
    c = TD.BY_ID[cid]
    a = TD.run(TD.setup(c, 'cpu', double))[0]
    for calls in ((12,), (5, 5, 2)):
        EC.same_bits(TD.run(TD.setup(c, 'cpu', double), calls=calls)[0], a)
    (big, gb, rows), small = TD.split_envs(c, 'cpu', double)
    RR.same_actors(gb, small, rows)


@pytest.mark.parametrize('cid', ['reach-window-J1', 'arm-ddpg-J5'])
def test_scale_zero_is_a_stream_built_without_the_field(cid, double):
    c = TD.BY_ID[cid]
    xs = [TD.setup(c, 'cpu', double, scale=s) for s in (None, 0.0)]
    assert all(x.resets.disturbance == 0 and len(x.resets.at()) == 3 for x in xs)
    (a, rows), (b, _) = (TD.run(x) for x in xs)
    EC.same_bits(a, b)
    assert all(torch.equal(p, q) for p, q in zip(TD.monitor_bytes(xs[0]), TD.monitor_bytes(xs[1])))
    TD.check_rows(a, xs[0], rows, scale=0.0)


# ---- Python: the stream object, evaluate, the refusals ------------------------------------------------------------------------------

def test_device_resets_carries_the_scale_and_its_state(double):
    venv = SyntheticVecEnv(4, 6, 2, episode_len=5, device='cpu', task='reach', kernels=double)
    plain = venv.attach_resets(7, 3)
    assert plain.disturbance == 0 and plain.at() == (7, 3, 0) and set(plain.state_dict()) == {'seed', 'actor_base', 'episode'}
    rs = venv.attach_resets(7, 3, disturbance=0.3)
    assert rs.disturbance == float(np.float32(0.3)) and rs.at() == (7, 3, 0, rs.disturbance) and rs.at(2)[2] == 2
    sd = rs.state_dict()
    assert set(sd) == {'seed', 'actor_base', 'episode', 'disturbance'} and sd['disturbance'] == rs.disturbance
    rs.load_state_dict(dict(sd, episode=5))
    assert rs.episode == 5
    for other in (plain.state_dict(), dict(sd, disturbance=0.5)):
        for f in (rs.load_state_dict, rs.check_state_dict):
            with pytest.raises(ValueError, match='disturbance'):
                f(other)
    with pytest.raises(ValueError, match='disturbance'):
        plain.load_state_dict(sd)
    assert rs.episode == 5 and plain.episode == 0
    # the struct a launch gets
    q = KN.HipKernels._reset_args(rs.at())
    assert (q.seed, q.actor_base, q.episode, q.enabled) == (7, 3, 5, 1) and q.disturbance == rs.disturbance
    assert q.reserved == int(np.float32(0.3).view(np.int32))
    q = KN.HipKernels._reset_args(plain.at())
    assert q.reserved == 0 and q.disturbance == 0.0 and ctypes.sizeof(q) == 32


def test_attach_and_stepping_refusals_leave_the_env_as_it_was(double):
    drift = SyntheticVecEnv(4, 17, 6, episode_len=5, device='cpu', kernels=double)
    with pytest.raises(ValueError, match='takes no disturbance'):
        drift.attach_resets(1, disturbance=0.1)
    assert drift.resets is None
    venv = SyntheticVecEnv(4, 6, 2, episode_len=5, device='cpu', task='reach', kernels=double)
    keep = venv.attach_resets(5)
    for bad in (-0.5, 1.0001, float('nan'), 'x'):
        with pytest.raises(ValueError, match=r'\[0, 1\]'):
            venv.attach_resets(1, disturbance=bad)
    assert venv.resets is keep
    rs = venv.attach_resets(1, disturbance=1.0)
    # never reset() since the stream was attached: the episode under way has no index
    state, t = venv.state.clone(), venv.t
    agent, cfg = EV.make_agent(EV.BY_ID['ddpg-reach-J2'], 4, mode='training')
    ppo, pcfg = EV.make_agent(EV.BY_ID['mlp-reach-J2'], 4, mode='training')
    for call in (lambda: venv.step(torch.zeros(4, 2)),
                 lambda: venv.ddpg_rollout_into(agent, EV._replay_of(EV.BY_ID['ddpg-reach-J2'], cfg), 3),
                 lambda: venv.ppo_rollout_into(ppo, EV._replay_of(EV.BY_ID['mlp-reach-J2'], pcfg), 3)):
        with pytest.raises(ValueError, match='stepped from a reset'):
            call()
    assert torch.equal(venv.state, state) and venv.t == t and rs.episode == 0 and venv._ppo == {}
    assert double.routes == []
    venv.reset()
    venv.step(torch.zeros(4, 2))
    assert venv.t == 1 and rs.episode == 1


class EvalStub(TD.DisturbedCpuKernels):
    """the double with the evaluation launches stubbed (test_device_eval_cpu.py's): a launch is recorded"""
    synth_eval_supported = KN.HipKernels.synth_eval_supported
    _task_id = staticmethod(KN.HipKernels._task_id)

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.lib = L.load()
        self.launches = []

    def synth_ppo_eval(self, model, packed, lstm_packed, init_state, episodes, episode_len, returns, **kw):
        self.launches.append(dict(kw, kind='ppo'))
        returns.zero_()

    def synth_ddpg_eval(self, net, packed, init_state, episodes, episode_len, returns, **kw):
        self.launches.append(dict(kw, kind='ddpg'))
        returns.zero_()

    synth_ppo_eval_sets = synth_ppo_eval

    def synth_ddpg_eval_sets(self, net, blobs, init_state, episodes, episode_len, returns, **kw):
        self.launches.append(dict(kw, kind='ddpg_sets'))
        returns.zero_()


def test_evaluate_hands_the_launch_the_scale_and_refuses_before_it():
    stub = EvalStub()
    prev = KN.set_default_kernels(stub, 'cpu')
    try:
        for pid in ('mlp-reach-J2', 'ddpg-reach-J2'):
            p = EV.BY_ID[pid]
            n = 5
            venv = EV.make_env(p, n, 4, 'cpu', stub)
            agent, _ = EV.make_agent(p, n)
            venv.evaluate(agent, 3, resets=(7, 9, 2), disturbance=0.3)
            assert stub.launches[-1]['resets'] == (7, 2, 9, float(np.float32(0.3)))
            for none in (None, 0, 0.0):
                venv.evaluate(agent, 3, resets=(7, 9, 2), disturbance=none)
                assert stub.launches[-1]['resets'] == (7, 2, 9)
            venv.evaluate(agent, 3, disturbance=0.0)
            assert stub.launches[-1]['resets'] is None
            count = len(stub.launches)
            with pytest.raises(ValueError, match='resets='):
                venv.evaluate(agent, 3, disturbance=0.3)
            for bad in (-0.1, 1.5, float('nan')):
                with pytest.raises(ValueError, match=r'\[0, 1\]'):
                    venv.evaluate(agent, 3, resets=(7, 9), disturbance=bad)
            with pytest.raises(ValueError, match=r'leave \[0, 2\^32\)'):
                venv.evaluate(agent, 3, resets=(7, 2 ** 32 - 2), disturbance=0.3)
            venv.evaluate(agent, 2, resets=(7, 2 ** 32 - 2), disturbance=0.3)             # (the last index: taken)
            venv.evaluate(agent, 3, resets=(7, 2 ** 32 - 2))                              # (undisturbed: as before)
            assert len(stub.launches) == count + 2
        drift = EV.make_env(EV.BY_ID['mlp-drift-17-6'], 4, 4, 'cpu', stub)
        agent, _ = EV.make_agent(EV.BY_ID['mlp-drift-17-6'], 4)
        count = len(stub.launches)
        with pytest.raises(ValueError, match='takes no disturbance'):
            drift.evaluate(agent, 1, disturbance=0.2)
        assert len(stub.launches) == count
        # the snapshot sets and the evaluator pass it on
        p = EV.BY_ID['ddpg-reach-J2']
        venv = EV.make_env(p, 4, 4, 'cpu', stub)
        agent, (lc, ec, sc) = EV.make_agent(p, 4)
        from surreal_amd.env import DeviceEvaluator
        agent.fetch_parameter = lambda: None
        DeviceEvaluator(venv, agent, sc, 2, resets=(EV.RSEED, 5), disturbance=0.3).run()
        assert stub.launches[-1]['resets'] == (EV.RSEED, 0, 5, float(np.float32(0.3)))
    finally:
        KN.set_default_kernels(*prev)


# ---- the entry points' argument checks (before any launch: no GPU here) -----------------------------------------------------

def stream(scale, base=0, episode=1, enabled=1):
    q = L.ResetStream()
    q.seed, q.actor_base, q.episode, q.enabled = 1, base, episode, enabled
    q.disturbance = scale
    return q


def ddpg_block(D=6, A=2, n=8, steps=4, t=0, capacity=64):
    """an argument block that passes smx_synth_ddpg_rollout_f32's checks, every pointer a fake (aligned) address"""
    fake = 4096
    net = L.Mlp3()
    for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'):
        setattr(net, k, fake)
    net.D, net.H1, net.H2, net.OUT = D, 8, 4, A
    d = L.DdpgRollout()
    d.net, d.packed = ctypes.pointer(net), fake
    d.n, d.D, d.A, d.steps, d.t, d.episode_len, d.n_step = n, D, A, steps, t, 5, 3
    d.noise_type = L.SMX_DDPG_NOISE_NONE
    for k in ('gpow', 'state', 'init_state', 'carry_obs', 'carry_act', 'carry_rew', 'obs', 'obs_next', 'actions', 'rewards',
              'dones'):
        setattr(d, k, fake)
    d.cursor, d.capacity = 0, capacity
    d._net = net
    return d


def misaligned_population():
    """an actor variant the launch refuses with SMX_E_ALIGN -- behind every check of the stream: a stream that gets this
    code passed them, and nothing is launched"""
    v = L.DdpgActorVariant()
    v.packed_pop, v.packed_stride, v.actors_per_agent, v.agents, v.measure_step, v.dist = 4096 + 4, 1 << 14, 4, 2, -1, 4096
    return v


BAD_SCALES = (-0.25, 1.0000001, 2.0, float('nan'), float('inf'), -float('inf'))


def test_recording_entry_points_refuse_a_bad_scale_or_episode_before_any_launch():
    lib = L.load()
    fake = L.c_void_p(4096)
    step = lambda q, task=1, t=0: lib.smx_synth_task_env_step_resets_f32(fake, fake, fake, 4, 6, 2, t, 5, 0, 1, None, None,  # noqa: E731
                                                                         None, None, None, task, q, None)
    roll = lambda q, task=1, **kw: lib.smx_synth_ddpg_rollout_variant_task_f32(ddpg_block(**kw), misaligned_population(),  # noqa: E731
                                                                               task, q, None)
    for bad in BAD_SCALES:
        assert step(stream(bad)) == E_SHAPE and roll(stream(bad)) == E_SHAPE, bad
        assert step(stream(bad), task=0) == roll(stream(bad), task=0) == L.SMX_E_UNSUPPORTED        # drift: before the scale
    assert step(stream(0.3), task=0) == roll(stream(0.3), task=0) == L.SMX_E_UNSUPPORTED
    # the episode under way: episode - 1 + (episode ends before the call's last step), in [0, 2^32)
    assert step(stream(0.3, episode=0)) == E_SHAPE and roll(stream(0.3, episode=0)) == E_SHAPE
    assert step(stream(0.3, episode=2 ** 32 + 1)) == E_SHAPE and roll(stream(0.3, episode=2 ** 32 + 1)) == E_SHAPE
    assert step(stream(0.3), t=-1) == E_SHAPE and step(stream(0.3), t=5) == E_SHAPE
    assert roll(stream(0.3, episode=2 ** 32), t=1, steps=4) == E_ALIGN         # steps 1 .. 4 of episode 2^32 - 1: taken
    assert roll(stream(0.3, episode=2 ** 32), t=1, steps=5) == E_SHAPE         # its fifth step begins episode 2^32
    assert roll(stream(0.3, episode=2 ** 32), t=0, steps=5) == E_ALIGN         # (the end behind the last step draws only)
    assert roll(stream(0.3, episode=2 ** 63 - 1), t=4, steps=2) == E_SHAPE     # (no overflow on the way)
    for ok in (0.3, 1.0, 2.0 ** -149, 0.0, -0.0):
        assert roll(stream(ok)) == E_ALIGN, ok
    # scale 0 asks nothing new: episode 0 and an index past 2^32 pass as they did; a disabled stream is not read
    assert roll(stream(0.0, episode=0)) == roll(stream(0.0, episode=2 ** 40)) == E_ALIGN
    assert roll(stream(float('nan'), base=-1, episode=-1, enabled=0)) == E_ALIGN
    # the resets entry points of the plain actor run the same checks
    assert lib.smx_synth_ddpg_rollout_resets_f32(ddpg_block(capacity=8), 1, stream(0.3), None) == E_SHAPE
    for bad in BAD_SCALES:
        assert lib.smx_synth_ddpg_rollout_resets_f32(ddpg_block(), 1, stream(bad), None) == E_SHAPE
    assert lib.smx_synth_ddpg_rollout_resets_f32(ddpg_block(), 1, stream(0.3, episode=0), None) == E_SHAPE
    assert lib.smx_abi_version() == 2


def test_evaluation_entry_points_refuse_a_bad_scale_or_episode_before_any_launch():
    lib = L.load()

    def net(D=6, A=2):
        m = L.Mlp3()
        m.W1 = m.b1 = m.W2 = m.b2 = m.W3 = m.b3 = 4096
        m.D, m.H1, m.H2, m.OUT = D, 32, 32, A
        return m

    def ppo(resets, task=1, episodes=2, m=None):
        m = m or net()
        p = L.SynthPpoEval()
        # (packed off its 16 bytes: SMX_E_ALIGN behind every check of the stream, nothing launched)
        p.net, p.packed, p.log_var, p.init_state, p.returns = ctypes.pointer(m), 4096 + 4, 4096, 4096, 4096
        p.n, p.episodes, p.episode_len, p.task, p.resets = 4, episodes, 3, task, resets
        return lib.smx_synth_ppo_eval_f32(p, None)

    def ddpg(resets, task=1, episodes=2, m=None):
        m = m or net()
        p = L.SynthDdpgEval()
        p.net, p.packed, p.init_state, p.returns = ctypes.pointer(m), 4096 + 4, 4096, 4096
        p.n, p.episodes, p.episode_len, p.task, p.resets = 4, episodes, 3, task, resets
        return lib.smx_synth_ddpg_eval_f32(p, None)

    def sets(f_name, struct, resets, episodes=2, ddpg_=False):
        m = net()
        p = struct()
        p.net, p.init_state, p.returns = ctypes.pointer(m), 4096, 4096
        p.n, p.episodes, p.episode_len, p.task, p.resets = 4, episodes, 3, 1, resets
        s = L.EvalSets()
        s.blobs, s.stride, s.sets, s.zfilter = 4096 + 4, 1 << 14, 2, 0
        return getattr(lib, f_name)(p, s, None)
    psets = lambda q, **kw: sets('smx_synth_ppo_eval_sets_f32', L.SynthPpoEval, q, **kw)  # noqa: E731
    dsets = lambda q, **kw: sets('smx_synth_ddpg_eval_sets_f32', L.SynthDdpgEval, q, **kw)  # noqa: E731
    for f in (ppo, ddpg, psets, dsets):
        assert f(stream(0.3, episode=0)) == E_ALIGN                  # (an evaluation's first_episode IS under way)
        for bad in BAD_SCALES:
            assert f(stream(bad)) == E_SHAPE, (f, bad)
        assert f(stream(0.3, episode=2 ** 32 - 2), episodes=2) == E_ALIGN
        assert f(stream(0.3, episode=2 ** 32 - 2), episodes=3) == E_SHAPE
        assert f(stream(0.3, episode=2 ** 32)) == E_SHAPE and f(stream(0.0, episode=2 ** 32)) == E_ALIGN
        assert f(stream(float('nan'), enabled=0)) == E_ALIGN
    for f in (ppo, ddpg):
        assert f(stream(0.3), task=0, m=net(D=17, A=6)) == L.SMX_E_UNSUPPORTED


# ---- the double against the float64 restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize('cid', TD.RESTATED)
def test_double_meets_the_float64_restatement(cid, double):
    """rtol = atol = 1e-5 (rollout_envelope_cases.TOL) at the seeds under which the restatement alone keeps MARGIN from every
    kink: the check test_gpu_task_disturbance_restatement.py runs on the kernels"""
    import reach_cases as RC
    x = TD.setup(TD.BY_ID[cid], 'cpu', double, seed=TD.TUNED[cid])
    want, wrows, written, pol = TD.restatement(x)
    RC.input_conditions(pol, RC.MARGIN)
    got, rows = TD.run(x)
    assert rows == wrows
    errs = EC.worst_errors(got, want, written)
    assert max(errs.values()) <= 1.0, errs
