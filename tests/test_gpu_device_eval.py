"""GPU tier (-m gpu): evaluation on the device -- whole episodes of a policy in ONE launch, nothing recorded
(SyntheticVecEnv.evaluate, DeviceEvaluator; smx_synth_ppo_eval_f32 / smx_synth_ddpg_eval_f32: the eighteen ppo_eval_kernel /
ddpg_eval_kernel instantiations).  Shapes (device_eval_cases): (n, E, L) = (5, 3, 7), (1, 1, 1), (9, 2, 4) -- 15 rows (a tail
at every block size), 1 row, 18 rows (two blocks at 16 rows per workgroup) -- each at 4, 8 and 16 rows per workgroup; reach
with 1, 2 and 21 masses, drift with (D, A) = (17, 6); hidden (32, 32), the ragged (28, 20) and the wide (24, 260: the generic
output-layer loop, H2 > 256); an LSTM stem of 10 units
(padded to 12); z-filters with non-trivial running sums; first_episode 0 and 2^32 - 2, actor_base 0 and 2^32 - n.

Every check is an equality of bits (fp64 returns compared as uint64); no tolerance anywhere:

  1. against the recording launches: per row a fresh env with a monitor, one episode through ppo_rollout_into /
     ddpg_rollout_into, the monitor's ring raw; MLP and DDPG also one serial call of T = E L;
  2. against the host definition under a constant action (zero weights; 0, and 0.3 / 1.7 on an identity head);
  3. 4, 8 and 16 rows per workgroup leave the same bytes;
  4. partition invariance: 8 actors = 4 + 4, E = 3 = 1 + 1 + 1, equal columns without a stream;
  5. purity: chunk, evaluate, chunk on the training env;
  6. DeviceEvaluator.run();
  7. the refusals, raised before any launch.

63 tests.
"""
import numpy as np
import pytest
import torch

import device_eval_cases as EV
from surreal_amd import _lib as L
from surreal_amd import kernels as KN

pytestmark = pytest.mark.gpu

DEV = 'cuda'
IDS = [p.id for p in EV.POLICIES]


def variants(p, n):
    """the start states of a case: (resets (seed, first_episode, actor_base) or None)"""
    if p.task != 'reach':
        return [None]
    return [None, (EV.RSEED, EV.FIRST_EPISODES[0], 0), (EV.RSEED, EV.FIRST_EPISODES[1], 2 ** 32 - n)]


def all_blocks(venv, agent, E, resets=None, noise=None):
    """evaluate at 4, 8 and 16 rows per workgroup and at the automatic size: the same bytes (3.) -> them"""
    got = [EV.evaluate(venv, agent, E, resets, noise, apw) for apw in EV.BLOCKS + (0,)]
    assert got[0].dtype == np.float64 and got[0].shape == (venv.n, E)
    for g in got[1:]:
        assert EV.same_f64(g, got[0])
    return got[0]


# ---- 1. against the recording launches ----------------------------------------------------------------------------------

@pytest.mark.parametrize('p', EV.POLICIES, ids=IDS)
def test_returns_are_the_recording_launches_bit_for_bit(p):
    for n, E, L_ in EV.SHAPES:
        agent, cfg = EV.make_agent(p, n)
        for resets in variants(p, n):
            venv = EV.make_env(p, n, L_, DEV)
            got = all_blocks(venv, agent, E, resets)
            want = EV.recorded_returns(p, n, E, L_, agent, cfg, DEV, resets)
            assert EV.same_f64(got, want), (n, E, L_, resets, got, want)
            assert np.isfinite(got).all() and (got != 0).any()
            if p.family != 'lstm':          # (an LSTM's state carries over episode ends in a serial run: not the same)
                assert EV.same_f64(got, EV.serial_returns(p, n, E, L_, agent, cfg, DEV, resets)), (n, E, L_, resets)


@pytest.mark.parametrize('p', [q for q in EV.POLICIES if q.family != 'ddpg'], ids=lambda q: q.id)
def test_stochastic_returns_are_the_recording_launches_bit_for_bit(p):
    """eval_stochastic: row (a, i) draws normal(seed, actor_base + a, first_step + i L + t, j)"""
    for n, E, L_ in EV.SHAPES:
        agent, cfg = EV.make_agent(p, n, mode='eval_stochastic_local')
        det, _ = EV.make_agent(p, n)
        for resets in variants(p, n)[-1:]:
            noise = (EV.NSEED, EV.FIRST_STEP, 2 ** 32 - n)
            venv = EV.make_env(p, n, L_, DEV)
            got = all_blocks(venv, agent, E, resets, noise)
            want = EV.recorded_returns(p, n, E, L_, agent, cfg, DEV, resets, noise)
            assert EV.same_f64(got, want), (n, E, L_, got, want)
            assert not EV.same_f64(got, EV.evaluate(venv, det, E, resets))          # (the draws matter)
            if p.family != 'lstm':
                assert EV.same_f64(got, EV.serial_returns(p, n, E, L_, agent, cfg, DEV, resets, noise))


# ---- 2. against the host definition ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('p', [q for q in EV.POLICIES if q.hidden == (32, 32)], ids=lambda q: q.id)
def test_zero_policy_returns_are_the_host_definition(p):
    for n, E, L_ in EV.SHAPES:
        agent, _ = EV.make_agent(p, n)
        EV.constant_policy(agent, 0.0)
        for resets in variants(p, n):
            venv = EV.make_env(p, n, L_, DEV)
            got = all_blocks(venv, agent, E, resets)
            want = EV.host_returns(p, n, E, L_, 0.0, resets, venv.init_state.cpu().numpy())
            assert EV.same_f64(got, want), (n, E, L_, resets, got, want)


@pytest.mark.parametrize('pid', ['mlp-reach-J2', 'mlp-reach-J21', 'mlp-drift-17-6', 'lstm-reach-J2'])
@pytest.mark.parametrize('value', [0.3, 1.7])
def test_constant_actions_on_an_identity_head_are_the_host_definition(pid, value):
    """PPO with out_act = identity and b3 = value: the action is value (1.7: clipped to 1) at every step"""
    p = EV.BY_ID[pid]
    K = KN.default_kernels()
    for n, E, L_ in EV.SHAPES:
        agent, _ = EV.make_agent(p, n)
        EV.constant_policy(agent, value)
        m = agent.model
        for resets in variants(p, n):
            venv = EV.make_env(p, n, L_, DEV)
            pk = torch.zeros(K.epoch_packed_numel(m.actor), device=DEV)
            K.epoch_pack([(m.actor, pk)])
            lpk = None
            if m.if_rnn:
                lpk = torch.zeros(K.lstm_rollout_packed_numel(m.rnn), device=DEV)
                K.lstm_rollout_pack(m.rnn, lpk)
            want = EV.host_returns(p, n, E, L_, value, resets, venv.init_state.cpu().numpy())
            for apw in EV.BLOCKS:
                out = torch.empty(n, E, dtype=torch.float64, device=DEV)
                K.synth_ppo_eval(m, pk, lpk, venv.init_state, E, L_, out, zfilter=m.z_filter, task=p.task,
                                 resets=None if resets is None else (resets[0], resets[2], resets[1]),
                                 actors_per_workgroup=apw, out_act=L.SMX_ACT_NONE)
                assert EV.same_f64(out.cpu().numpy(), want), (n, E, L_, resets, apw)


# ---- 4. partition invariance -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pid', ['mlp-reach-J2', 'lstm-reach-J2', 'ddpg-reach-J2'])
def test_eight_actors_are_two_envs_of_four(pid):
    p = EV.BY_ID[pid]
    E, L_ = 3, 7
    modes = ['eval_deterministic_local'] + (['eval_stochastic_local'] if p.family != 'ddpg' else [])
    for mode in modes:
        agent, _ = EV.make_agent(p, 8, mode=mode)
        stoch = mode.startswith('eval_stochastic')
        base = 2 ** 32 - 8
        resets = (EV.RSEED, EV.FIRST_EPISODES[1], base)
        noise = (EV.NSEED, EV.FIRST_STEP, base) if stoch else None
        whole = EV.evaluate(EV.make_env(p, 8, L_, DEV), agent, E, resets, noise)
        parts = [EV.evaluate(EV.make_env(p, 4, L_, DEV), agent, E, resets[:2] + (base + b,),
                             None if noise is None else noise[:2] + (base + b,), apw) for b, apw in ((0, 4), (4, 16))]
        assert EV.same_f64(whole, np.concatenate(parts)), mode


@pytest.mark.parametrize('pid', ['mlp-reach-J2', 'lstm-reach-J21', 'ddpg-reach-J1'])
def test_three_episodes_are_three_calls_of_one(pid):
    p = EV.BY_ID[pid]
    n, E, L_ = 5, 3, 7
    modes = ['eval_deterministic_local'] + (['eval_stochastic_local'] if p.family != 'ddpg' else [])
    for mode in modes:
        agent, _ = EV.make_agent(p, n, mode=mode)
        stoch = mode.startswith('eval_stochastic')
        venv = EV.make_env(p, n, L_, DEV)
        fe = EV.FIRST_EPISODES[1]
        noise = (EV.NSEED, EV.FIRST_STEP, 0) if stoch else None
        whole = EV.evaluate(venv, agent, E, (EV.RSEED, fe, 0), noise)
        cols = [EV.evaluate(venv, agent, 1, (EV.RSEED, fe + i, 0),
                            None if noise is None else (EV.NSEED, EV.FIRST_STEP + i * L_, 0)) for i in range(E)]
        assert EV.same_f64(whole, np.concatenate(cols, axis=1)), mode
        assert len({whole[:, i].tobytes() for i in range(E)}) == E          # (the episodes differ)


@pytest.mark.parametrize('p', [q for q in EV.POLICIES if q.hidden == (32, 32) and q.A in (2, 6)], ids=lambda q: q.id)
def test_without_a_stream_every_column_is_the_same_episode(p):
    n, E, L_ = 9, 4, 5
    agent, _ = EV.make_agent(p, n)
    got = EV.evaluate(EV.make_env(p, n, L_, DEV), agent, E)
    for i in range(1, E):
        assert EV.same_f64(got[:, i], got[:, 0])
    assert len({got[a, 0].tobytes() for a in range(n)}) == n                # (the actors differ)


# ---- 5. purity -------------------------------------------------------------------------------------------------------------------

def _snapshot(venv, replay, agent):
    s = {'state': venv.state.clone(), 't': int(venv.t), 'noise.step': venv.noise.step, 'resets.episode': venv.resets.episode,
         'monitor': venv.monitor._buf.clone(), 'monitor.steps': venv.monitor.total_steps}
    for k, v in (venv._ppo.get('carry') or {}).items():
        s['ppo.' + k] = v.clone()
    for k in ('carry_obs', 'carry_act', 'carry_rew', 'ou'):
        if venv._ddpg.get(k) is not None:
            s['ddpg.' + k] = venv._ddpg[k].clone()
    for k, tab in replay._tables.items():
        s['replay.' + k] = tab.data.clone()
    s['replay.cursor'] = tuple(getattr(replay, a) for a in ('_head', '_count', '_dev_next', '_dev_len') if hasattr(replay, a))
    s['replay.collected'] = replay.cumulative_collected_count
    cells = getattr(agent, '_batch_cells', None)
    if cells is not None:
        s['cells.h'], s['cells.c'] = cells[0].clone(), cells[1].clone()
    return s


def _same_snapshot(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize('pid', ['mlp-reach-J2', 'lstm-reach-J2', 'ddpg-reach-J2'])
def test_evaluate_between_two_training_chunks_changes_nothing(pid):
    p = EV.BY_ID[pid]
    n, L_, T = 9, 5, 7                                       # (chunks of 7 over episodes of 5: the second starts mid-episode)

    def sequence(with_eval):
        from surreal_amd.replay import FIFOReplay, UniformReplay
        train, cfg = EV.make_agent(p, n, mode='training', n_step=3, **({'stride': 2} if p.family != 'ddpg' else {}))
        ev, _ = EV.make_agent(p, n)
        venv = EV.make_env(p, n, L_, DEV)
        venv.attach_monitor(capacity=4)
        venv.attach_noise(EV.NSEED)
        venv.attach_resets(EV.RSEED)
        venv.reset()
        replay = (UniformReplay if p.family == 'ddpg' else FIFOReplay)(*cfg)
        roll = venv.ddpg_rollout_into if p.family == 'ddpg' else venv.ppo_rollout_into
        roll(train, replay, T)
        if with_eval:
            before = _snapshot(venv, replay, train)
            for kw in (dict(resets=(EV.RSEED + 1, 0)), dict()):
                got = venv.evaluate(ev, 2, **kw)
                assert got.shape == (n, 2) and bool(torch.isfinite(got).all())
            _same_snapshot(before, _snapshot(venv, replay, train))
        roll(train, replay, T)
        torch.cuda.synchronize()
        return _snapshot(venv, replay, train)
    _same_snapshot(sequence(False), sequence(True))


# ---- 6. DeviceEvaluator ---------------------------------------------------------------------------------------------------------

def test_device_evaluator_reports_what_host_eval_monitors_would():
    from surreal_amd.env import DeviceEvaluator
    p = EV.BY_ID['mlp-reach-J2']
    n, E, L_ = 5, 3, 7
    agent, (lc, ec, sc) = EV.make_agent(p, n)
    fetched = []
    agent.fetch_parameter = lambda: fetched.append(len(launches))
    launches = []
    orig = L.call

    def call(name, *args):
        if name.endswith('_eval_f32'):
            launches.append(name)
        return orig(name, *args)
    venv = EV.make_env(p, n, L_, DEV)
    sc.tensorplex.update_schedule.eval_env = 2
    de = DeviceEvaluator(venv, agent, sc, E, resets=(EV.RSEED, 0), eval_id_base=7)
    L.call = call
    try:
        runs = [de.run() for _ in range(2)]
    finally:
        L.call = orig
    assert fetched == [0, 1] and launches == ['smx_synth_ppo_eval_f32'] * 2          # one fetch before each launch
    want = EV.evaluate(venv, agent, E, (EV.RSEED, 0, 0))
    assert all(EV.same_f64(r, want) for r in runs)
    EV.check_reports(de, [np.concatenate([want[i], want[i]]).tolist() for i in range(n)], 7, sc)
    assert all(len(r.tensorplex.history) == 3 for r in de.reports)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_come_before_any_launch(monkeypatch):
    calls = []
    orig = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), orig(name, *a))[1])
    EV.check_python_refusals(DEV, None)
    assert not [c for c in calls if c.endswith('_eval_f32')], calls
    EV.check_entry_point_codes()
