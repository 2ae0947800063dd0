"""CPU tier: the `arm` task (surreal_amd/env/tasks.py; arm_cases.py).  The host definition against a float64 restatement
and its own edges; the reset row for known words; check_task's refusals; the header's define; the library's host-side
queries and refusal codes for SMX_TASK_ARM (argument blocks whose pointers are never read: no GPU here); every route and
refusal of the environments on the torch-CPU double, with the shared checks of the GPU tier (arm_cases.check_rows: every
recorded row against the host step, first rows against the reset stream, monitor returns); the float64 restatement's input
conditions at the tuned seeds; scripts/train_reach.py --task arm on the double, both algorithms.

The learning run on the double that set test_gpu_arm_learning.py's chunk count is the last test's (figures there)."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import arm_cases as AC
import device_eval_cases as EV
import rollout_envelope_cases as EC
from surreal_amd import _lib as L
from surreal_amd.env import tasks as TK
from surreal_amd.env.synthetic_env import SyntheticEnv, SyntheticVecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [AC.tuned(c) for c in AC.CASES]
IDS = [c.id for c in CASES]
BIT_CASES = CASES + AC.BITS_ONLY                      # (the equalities of bits: also the case no seed tunes)
BIT_IDS = [c.id for c in BIT_CASES]
PI_F = np.float32(3.1415927)


@pytest.fixture
def double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(AC.ArmCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


# ---- the host definition -------------------------------------------------------------------------------------------------------

def random_states(rs, n, J):
    s = np.zeros((n, 2 * J + 2), np.float32)
    s[:, :J] = rs.uniform(-3.0, 3.0, (n, J))
    s[:, J:2 * J] = rs.uniform(-0.9, 0.9, (n, J))
    s[:, 2 * J:] = rs.uniform(-0.25, 0.25, (n, 2))
    return s


@pytest.mark.parametrize('J', [1, 2, 3, 4, 5, 30])
def test_arm_step_meets_the_float64_restatement(J):
    rs = np.random.RandomState(J)
    s = random_states(rs, 200, J)
    a = rs.uniform(-1.5, 1.5, (200, J)).astype(np.float32)
    sn, r = TK.arm_step(s, a)
    assert sn.dtype == np.float32 and r.dtype == np.float32 and sn.shape == s.shape and r.shape == (200,)
    env = AC.ArmEnv(torch.as_tensor(s).double(), J, 10, state=torch.as_tensor(s).double())
    _, wn, wr, _ = env.step(torch.as_tensor(a).double())
    assert np.abs(sn - wn.numpy()).max() <= 1e-6
    assert np.abs(r - wr.numpy()).max() <= 1e-6 * max(1.0, float(wr.abs().max()))
    assert np.array_equal(sn[:, 2 * J:], s[:, 2 * J:])
    # a batch is its rows: the sums go one term at a time
    one, r1 = TK.arm_step(s[7], a[7])
    assert np.array_equal(one.view(np.uint32), sn[7].view(np.uint32)) and np.float32(r1).tobytes() == r[7].tobytes()


def test_link_length_is_the_power_of_two():
    for J in range(1, 31):
        w = TK.arm_link(J)
        assert w == 2.0 ** -math.ceil(math.log2(J)) == AC.link(J) and 0.5 < J * w <= 1.0 or J == 1 and w == 1.0


def test_the_polynomials_are_sine_and_cosine_to_1e_6():
    x = np.linspace(-math.pi, math.pi, 200001).astype(np.float32)
    x = np.clip(x, -PI_F, PI_F)
    s, c = TK.arm_sincos(x)
    assert s.dtype == c.dtype == np.float32
    assert np.abs(s - np.sin(x.astype(np.float64))).max() <= 1e-6
    assert np.abs(c - np.cos(x.astype(np.float64))).max() <= 1e-6
    assert [float(v) for v in TK.ARM_SIN_C] == [float(np.float32(v)) for v in AC.SIN_C]
    assert [float(v) for v in TK.ARM_COS_C] == [float(np.float32(v)) for v in AC.COS_C]
    assert TK.arm_sincos(np.float32(0.0))[0] == 0.0 and TK.arm_sincos(np.float32(0.0))[1] == 1.0


def test_clamp_edges():
    J = 2
    s = np.zeros((4, 2 * J + 2), np.float32)
    s[0, :J], s[0, J:2 * J] = PI_F, 1.0                  # at both upper limits, pushed further
    s[1, :J], s[1, J:2 * J] = -PI_F, -1.0
    s[2, :J], s[2, J:2 * J] = np.float32(3.0), 1.0       # theta + 0.2 crosses the limit
    s[3, :J], s[3, J:2 * J] = np.float32(2.5), np.float32(0.95)
    a = np.array([[5.0, 5.0], [-5.0, -5.0], [1.0, 1.0], [1.0, 1.0]], np.float32)
    sn, r = TK.arm_step(s, a)
    assert (sn[0, :J] == PI_F).all() and (sn[0, J:2 * J] == 1.0).all()
    assert (sn[1, :J] == -PI_F).all() and (sn[1, J:2 * J] == -1.0).all()
    assert (sn[2, :J] == PI_F).all() and (sn[2, J:2 * J] == 1.0).all()
    assert (sn[3, J:2 * J] == 1.0).all() and (sn[3, :J] == np.float32(2.5) + np.float32(0.2) * np.float32(1.0)).all()
    assert np.isfinite(r).all()
    # the reward at the limit: both links point along -x, the tip at (-1, ~0) for J = 2 (w = 1/2)
    assert abs(float(r[0]) + (1.0 + 0.02)) < 1e-5


def test_reset_rows_for_known_words():
    seed, J = 0x0123456789ABCDEF, 5
    g, e = 7, 2 ** 33 + 1
    row = TK.arm_reset_state(seed, g, e, J)
    assert row.dtype == np.float32 and row.shape == (2 * J + 2,)
    for k in range(2 * J + 2):
        x = TK.philox4x32_10(np.array([g, e & 0xFFFFFFFF, e >> 32, TK.RESET_TAG | (k >> 2)], dtype=np.uint64),
                             np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
        u = np.float32(int(x[k & 3]) >> 8) * np.float32(2.0 ** -23) - np.float32(1.0)
        want = u if k < J else np.float32(0.0) if k < 2 * J else np.float32(0.25) * u
        assert row[k].tobytes() == np.float32(want).tobytes(), k
    # the same words serve reach's row: the stream is one
    u5 = TK.reach_reset_state(seed, g, e, 4)
    assert row[0] == u5[0] and row[2 * J] == np.float32(0.25) * u5[2 * J]


def test_reset_rows_stay_inside_the_limits_over_1e5_draws():
    J = 4
    rows = TK.arm_reset_state(11, np.arange(1000)[:, None], np.arange(25)[None, :], J)       # 25 000 rows, 10^5 orientations
    th, om, g = rows[..., :J], rows[..., J:2 * J], rows[..., 2 * J:]
    assert th.size == 100000
    assert (np.abs(th) < PI_F).all() and np.abs(th).max() <= 1.0
    assert (om == 0).all() and not np.signbit(om).any()
    assert (np.abs(g) <= 0.25).all() and np.hypot(g[..., 0], g[..., 1]).max() < 0.36
    assert np.abs(th).max() > 0.999 and np.abs(g).max() > 0.249
    with pytest.raises(ValueError, match='seed must fit 64 bits'):
        TK.arm_reset_state(1 << 64, 0, 0, 2)
    with pytest.raises(ValueError, match='actor ids'):
        TK.arm_reset_state(1, -1, 0, 2)


def test_jt_action_beats_the_zero_action():
    J, n, L_ = 2, 64, 50
    out = {}
    for name, ctrl in (('zero', lambda s: np.zeros((n, J), np.float32)), ('jt', TK.arm_jt_action)):
        s, total = TK.arm_reset_state(5, np.arange(n), 0, J), np.zeros(n)
        for _ in range(L_):
            s, r = TK.arm_step(s, ctrl(s))
            total += r
        out[name] = total.mean()
    assert out['jt'] > 0.5 * out['zero'] > out['zero']
    assert TK.arm_jt_action(np.zeros(6, np.float32)).shape == (2,)


def test_check_task_refusals():
    assert TK.TASKS == ('drift', 'reach', 'arm') and TK.TASK_IDS['arm'] == L.SMX_TASK_ARM == 2
    TK.check_task('x', 'arm', 6, 2)
    TK.check_task('x', 'arm', 62, 30)
    with pytest.raises(ValueError, match=r"task 'arm' has obs_dim == 2 \* action_dim \+ 2"):
        TK.check_task('x', 'arm', 7, 2)
    with pytest.raises(ValueError, match="task 'arm' has no camera"):
        TK.check_task('x', 'arm', 6, 2, pixel=(3, 8, 8))
    with pytest.raises(ValueError, match='task must be one of'):
        TK.check_task('x', 'leg', 6, 2)
    with pytest.raises(ValueError, match='obs_dim == 2'):
        SyntheticEnv(9, 3, task='arm')
    assert TK.MAX_A == {'drift': None, 'reach': 21, 'arm': 30}


def test_header_define_is_the_binding():
    text = open(os.path.join(ROOT, 'include', 'surreal_amd.h')).read()
    assert int(re.search(r'^#define SMX_TASK_ARM (\d+)$', text, re.M).group(1)) == L.SMX_TASK_ARM
    assert int(re.search(r'^#define SMX_TASK_REACH (\d+)$', text, re.M).group(1)) == L.SMX_TASK_REACH


# ---- the library's host side ---------------------------------------------------------------------------------------------------

def test_library_queries_take_the_arm_shapes():
    lib = L.load()
    ok = lib.smx_synth_task_supported
    ARM = L.SMX_TASK_ARM
    for J in (1, 2, 17, 30):
        assert ok(ARM, 2 * J + 2, J) == 1
    assert ok(ARM, 64, 31) == 0 and ok(ARM, 6, 3) == 0 and ok(ARM, 2, 0) == 0 and ok(ARM, 7, 2) == 0
    assert ok(ARM, 9, 3) == 0 and ok(L.SMX_TASK_REACH, 9, 3) == 1 and ok(L.SMX_TASK_REACH, 8, 3) == 0
    assert ok(3, 6, 2) == 0 and ok(7, 6, 2) == 0
    sup = lib.smx_synth_eval_supported                  # (ddpg, task, D, H, H1, H2, A)
    assert sup(0, ARM, 6, 0, 32, 32, 2) == 1 and sup(1, ARM, 6, 0, 28, 20, 2) == 1 and sup(0, ARM, 6, 12, 32, 32, 2) == 1
    assert sup(0, ARM, 62, 0, 32, 32, 30) == 1 and sup(1, ARM, 62, 0, 32, 32, 30) == 1
    assert sup(0, ARM, 64, 0, 32, 32, 31) == 0 and sup(1, ARM, 7, 0, 32, 32, 2) == 0 and sup(1, ARM, 6, 12, 32, 32, 2) == 0
    assert sup(0, ARM, 6, 0, 30, 32, 2) == 0
    assert lib.smx_abi_version() == 2


def test_entry_points_refuse_before_any_launch():
    lib = L.load()
    fake = L.c_void_p(4096)
    ARM = L.SMX_TASK_ARM
    E_NULL, E_SHAPE = -1, -2

    def stream(base=0, episode=0, enabled=1):
        q = L.ResetStream()
        q.seed, q.actor_base, q.episode, q.enabled = 1, base, episode, enabled
        return q
    fill = lambda q, task=ARM, n=4, D=6: lib.smx_reset_fill_f32(q, task, n, D, fake, None)  # noqa: E731
    assert fill(stream(), D=7) == L.SMX_E_UNSUPPORTED and fill(stream(), D=64) == L.SMX_E_UNSUPPORTED
    assert fill(stream(), D=2) == L.SMX_E_UNSUPPORTED and fill(stream(), D=0) == L.SMX_E_UNSUPPORTED
    assert fill(stream(), task=3) == L.SMX_E_UNSUPPORTED
    assert fill(None) == E_NULL and fill(None, D=4) == E_NULL and fill(None, D=62) == E_NULL
    assert fill(stream(base=-1)) == E_SHAPE and fill(stream(base=2 ** 32 - 3)) == E_SHAPE
    assert fill(stream(episode=-1)) == E_SHAPE and fill(stream(), n=0) == E_SHAPE
    step = lambda D, A, q=None: lib.smx_synth_task_env_step_resets_f32(fake, fake, fake, 4, D, A, 0, 5, 0, 1, None, None,  # noqa: E731
                                                                       None, None, None, ARM, q, None)
    assert step(7, 2) == L.SMX_E_UNSUPPORTED and step(64, 31) == L.SMX_E_UNSUPPORTED and step(6, 3) == L.SMX_E_UNSUPPORTED
    assert step(6, 2, stream(base=-1)) == E_SHAPE and step(6, 2, stream(episode=-1)) == E_SHAPE
    p, d = L.SynthPpoWindowRollout(), L.DdpgRollout()
    assert lib.smx_synth_ppo_window_rollout_task_f32(None, ARM, None) == E_NULL
    assert lib.smx_synth_ddpg_rollout_task_f32(None, ARM, None) == E_NULL
    assert lib.smx_synth_ppo_window_rollout_task_f32(p, 3, None) == L.SMX_E_UNSUPPORTED
    assert lib.smx_synth_ddpg_rollout_task_f32(d, 3, None) == L.SMX_E_UNSUPPORTED
    assert lib.smx_synth_ddpg_rollout_variant_task_f32(d, None, 3, None, None) == L.SMX_E_UNSUPPORTED
    assert lib.smx_synth_ddpg_rollout_variant_task_f32(None, None, ARM, None, None) == E_NULL


# ---- the environments on the double ------------------------------------------------------------------------------------------

def test_host_env_steps_and_resets(double):
    J, L_ = 3, 4
    env = SyntheticEnv(2 * J + 2, J, episode_len=L_, task='arm', resets=(9, 5))
    obs, _ = env._reset()
    assert AC.bits(obs['low_dim']['flat_inputs'], TK.arm_reset_state(9, 5, 0, J)) and env.episode == 1
    s = env.state.copy()
    for t in range(L_):
        a = np.full(J, 0.3, np.float32)
        obs, r, done, _ = env._step(a)
        s, wr = TK.arm_step(s, a)
        assert AC.bits(obs['low_dim']['flat_inputs'], s) and r == float(wr) and done == (t == L_ - 1)
    obs, _ = env._reset()
    assert AC.bits(obs['low_dim']['flat_inputs'], TK.arm_reset_state(9, 5, 1, J))
    with pytest.raises(ValueError, match="task 'drift' has no reset distribution"):
        SyntheticEnv(6, 2, task='drift', resets=(1, 2))


def test_vec_env_step_reset_stream_and_monitor(double):
    n, J, L_ = 6, 2, 3
    venv = SyntheticVecEnv(n, 2 * J + 2, J, episode_len=L_, device='cpu', task='arm')
    mon = venv.attach_monitor(capacity=4)
    rs = venv.attach_resets(AC.RSEED, actor_base=10)
    assert torch.equal(venv.reset(), rs.states(0)) and rs.episode == 1
    assert AC.bits(venv.state.numpy(), TK.arm_reset_state(AC.RSEED, 10 + np.arange(n), 0, J))
    hosts = [SyntheticEnv(2 * J + 2, J, episode_len=L_, task='arm', resets=(AC.RSEED, 10 + a)) for a in range(n)]
    for h in hosts:
        h._reset()
    acts = torch.randn(2 * L_ + 1, n, J, generator=torch.Generator().manual_seed(4)) * 1.5
    returns = [[0.0] for _ in range(n)]
    for s in range(acts.shape[0]):
        state = venv.step(acts[s]).clone()
        assert rs.episode == 1 + (s + 1) // L_
        for a, h in enumerate(hosts):
            obs, r, done, _ = h._step(acts[s, a].numpy())
            returns[a][-1] += r
            if done:
                obs, _ = h._reset()
                returns[a].append(0.0)
            assert AC.bits(state[a].numpy(), obs['low_dim']['flat_inputs']), (s, a)
    assert AC.monitor_returns(mon, n) == [r[:2] for r in returns]
    sd = venv.state_dict()
    assert sd['fingerprint']['task'] == 'arm' and sd['resets']['episode'] == rs.episode
    other = SyntheticVecEnv(n, 6, 2, episode_len=L_, device='cpu', task='reach')
    with pytest.raises(ValueError, match="task = 'arm'"):
        other.load_state_dict(sd)
    venv.load_state_dict(sd)


def test_refusals(double):
    with pytest.raises(ValueError, match='obs_dim == 2'):
        SyntheticVecEnv(4, 6, 3, device='cpu', task='arm')
    with pytest.raises(ValueError, match='no camera'):
        SyntheticVecEnv(4, 6, 2, device='cpu', task='arm', pixel=(3, 8, 8))
    wide = SyntheticVecEnv(4, 64, 31, episode_len=5, device='cpu', task='arm')
    with pytest.raises(ValueError, match=r"task 'arm' with 31 actions; the device runs action_dim <= 30"):
        wide.step(torch.zeros(4, 31))
    with pytest.raises(ValueError, match='action_dim <= 30'):
        wide.attach_resets(1)
    venv = SyntheticVecEnv(4, 6, 2, episode_len=5, device='cpu', task='arm')
    for call in (lambda: venv.start_rollout(4), ):
        with pytest.raises(NotImplementedError, match="task 'arm' is stepped by"):
            call()
    clocks = SyntheticVecEnv(4, 6, 2, episode_len=[5, 5, 5, 5], device='cpu', task='arm')
    with pytest.raises(NotImplementedError, match='per-actor episode clocks'):
        clocks.attach_resets(1)
    drift = SyntheticVecEnv(4, 6, 2, episode_len=5, device='cpu')
    with pytest.raises(ValueError, match=r"attach_resets: task 'drift' has no reset distribution \(task 'reach' has\)"):
        drift.attach_resets(1)
    p = EV.Policy('mlp-arm-J2', 'mlp', 'arm', 6, 2, (32, 32))
    agent, _ = EV.make_agent(p, 4)
    with pytest.raises(NotImplementedError, match='no synth_ppo_eval'):
        venv.evaluate(agent, 1)                       # (this double has no evaluation launch: refused before any)


@pytest.mark.parametrize('c', BIT_CASES, ids=BIT_IDS)
def test_rollouts_on_the_double_hold_the_host_step_and_the_reset_stream(c, double):
    x = AC.setup_resets(c, 'cpu', double)
    got, rows = AC.run(x)
    assert rows == x.rows and x.resets.episode == 1 + sum(AC.CALLS) // AC.EP
    returns = AC.check_rows(got, x, rows, resets=(AC.RSEED, 0))
    if returns is not None:
        assert AC.monitor_returns(x.venv.monitor, c.n) == returns
    # one call of 13 steps, and calls of 3 + 4 + 6, leave the bytes of 7 + 6
    for calls in ((13,), (3, 4, 6)):
        y = AC.setup_resets(c, 'cpu', double)
        EC.same_bits(AC.run(y, calls=calls)[0], got)
    if c.family == 'ddpg':
        assert [r['task'] for r in double.routes] == ['arm'] * 6


@pytest.mark.parametrize('cid', ['window-J1-n5', 'lstm_window-J30-n20', 'ddpg-J1-n20'])
def test_two_envs_of_four_record_what_one_of_eight_records(cid, double):
    import reach_resets_cases as RR
    c = [q for q in BIT_CASES if q.id == cid][0]
    (big, gb), small = AC.split_envs(c, 'cpu', double)
    RR.same_actors(gb, small, big.rows)


@pytest.mark.parametrize('variant', [dict(), dict(layernorm=True), dict(param_noise='normal', n=8),
                                     dict(layernorm=True, param_noise='normal', n=8)], ids=['plain', 'ln', 'pop', 'popln'])
def test_ddpg_whole_steps_and_monitor_returns(variant, double):
    got, want = AC.whole_steps('cpu', double, **variant)
    assert got == want and all(len(r) == 2 for r in got)
    assert all(r['task'] == 'arm' and r['ln'] == bool(variant.get('layernorm')) and r['pn'] == ('param_noise' in variant)
               for r in double.routes)


def test_ddpg_variants_route_to_the_variant_launch(double):
    """a LayerNorm actor on 'arm': the one launch with ln and the task (kernels.ddpg_variant_task_launch), as on 'reach'"""
    import ddpg_rollout_cases as DC
    import ddpg_ln_rollout_cases as LN
    n, J = 8, 2
    lc, ec, sc = DC.configs(6, J, n, hidden=(8, 4), n_step=3, noise_type='normal', memory_size=256, layernorm=True)
    agent = DC.make_agent(lc, ec, sc)
    venv = SyntheticVecEnv(n, 6, J, episode_len=5, device='cpu', task='arm')
    venv.attach_resets(3)
    venv.reset()
    venv.ddpg_rollout_into(agent, LN.replay_of(lc, ec, sc), 7, eps=torch.randn(7, n, J))
    assert [(r['task'], r['ln'], r['steps']) for r in double.routes] == [('arm', True, 7)]
    assert AC.bits(venv.state[:, 4:].numpy(), TK.arm_reset_state(3, np.arange(n), 1, J)[:, 4:])


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_restatement_meets_its_input_conditions_at_the_tuned_seed(c, double):
    x = AC.setup(c, 'cpu', double, wrap=False)
    AC.input_conditions(AC.restatement(x)[3], (2 if c.streams else 1) * AC.MARGIN)


# ---- scripts/train_reach.py --task arm --------------------------------------------------------------------------------------------

def train_reach():
    scripts = os.path.join(ROOT, 'scripts')
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import train_reach as TR
    return TR


@pytest.mark.parametrize('algo', ['ppo', 'ddpg'])
def test_train_reach_on_the_arm(algo, double, monkeypatch):
    """two chunks of the loop on the double (which draws from no noise stream: none is attached), random resets and
    held-out evaluation: the baseline line names the task and carries the Jacobian-transpose controller's return"""
    TR = train_reach()
    monkeypatch.setattr(SyntheticVecEnv, 'attach_noise', lambda self, seed, actor_base=0: None)
    lines = []
    base, curve = TR.train(algo, actors=8, J=2, episode_len=10, iters=2, eval_every=1, device='cpu', log=lines.append,
                           random_resets=True, heldout_episodes=2, task='arm')
    assert base['task'] == 'arm' and base['pd_return'] > base['zero_action_return']
    want = TR.heldout_return(2, 10, 8, 3, 2, TK.arm_jt_action, 'arm')
    assert base['pd_return'] == want
    assert [c['iteration'] for c in curve] == [0, 1, 2] and all(np.isfinite(c['eval_return']) for c in curve)
    if algo == 'ddpg':
        assert all(r['task'] == 'arm' for r in double.routes) and len(double.routes) == 2
    # the default is reach's loop, line for line
    assert 'task' not in TR.baselines(1, 3, range(2)) and TR.obs_dim('reach', 2) == 6 and TR.obs_dim('arm', 2) == 6
