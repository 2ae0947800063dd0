"""CPU tier: TD3's delayed policy updates (learner_config.algo.network.policy_delay) through the torch-CPU doubles -- every
schedule against the restatement (ddpg_delay_cases.py), the launch sequence of both kinds of iteration, the refusals, the
training state."""
import numpy as np
import pytest
import torch

import ddpg_delay_cases as DC
import ddpg_helpers as DH
import ddpg_ln_td3_rows_cases as LT

ROWS = {'ddpg_row_schedule': True}


@pytest.fixture
def double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(DC.DelayRowsCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


def flats(L):
    """every buffer that decides the next iteration, by name"""
    return {k: v.clone() for k, v in L._train_tensors().items()}


def same_bytes(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('name,schedule,d', DC.matrix())
def test_every_schedule_matches_the_restatement(double, name, schedule, d):
    """every statistic of every iteration at 1e-5, every element of model, target, second critic and its target at the
    case's parameter bound"""
    L = DC.run_against_reference(name, DC.schedules(name)[schedule], d)
    assert L._schedule(*L._ws.key) == schedule
    rows_calls = [c for c in double.calls if c.startswith('ddpg_rows')]
    assert bool(rows_calls) == (schedule == 'rows')


@pytest.mark.parametrize('name', ['tiny_soft_clipcritic', 'tiny_ln_td3_soft'])
def test_launch_sequence_at_delay_two(double, name):
    """critic-only iterations: the chain without the actor, the critic groups' steps without a target, the last of them
    reporting -- 2 launches, 3 with two critics; no actor chain, no actor step, no soft_update.  Update iterations: today's
    launches and the tail in front of the actor's step, whose step word reads 1, 2, 3"""
    case = DH.load(name)[1]
    two = bool(case['hyper'].get('double_critic'))
    L = DC.make_learner(case, ROWS, policy_delay=2)
    L.learn(DC.batch(case, 0))                        # (the packs ride in front of the first iteration)
    td3 = '_td3' if two else ''
    groups = ['critic', 'critic2'] if two else ['critic']
    ups = ['ddpg_rows_update:%s:wgrad' % g for g in groups]
    critic_only = ['ddpg_rows_critic_only' + td3] + ups
    full = ['ddpg_rows_critic' + td3] + ups + ['ddpg_rows_actor', 'ddpg_rows_delay_tail', 'ddpg_rows_update:actor:wgrad']
    assert [c for c in double.calls if not c.startswith('ddpg_rows_pack')] == critic_only, double.calls
    for it in range(1, DC.ITERS):
        del double.calls[:], double.update_log[:]
        L.learn(DC.batch(case, it))
        k = it + 1
        assert double.calls == (full if k % 2 == 0 else critic_only), (k, double.calls)
        want = [(g, k % 2 == 0, k, k % 2 == 1 and g == groups[-1]) for g in groups]
        if k % 2 == 0:
            want.append(('actor', True, k // 2, False))
            assert int(L._ws.astep[0]) == k // 2
        assert double.update_log == want, (k, double.update_log)
        assert int(L._ws.step[0]) == k == L.critic_step and L.actor_step == k // 2


def test_layers_and_levels_skip_the_actor_and_the_targets(double):
    case = DH.load('tiny_soft_clipcritic')[1]
    for sched in ('layers', 'levels'):
        L = DC.make_learner(case, DC.schedules('tiny_soft_clipcritic')[sched], policy_delay=2)
        for it in range(4):
            del double.calls[:]
            before = (L.model.actor_flat.clone(), L.model_target.actor_flat.clone(), L.model_target.critic_flat.clone(),
                      L.actor_exp_avg.clone())
            L.learn(DC.batch(case, it))
            after = (L.model.actor_flat, L.model_target.actor_flat, L.model_target.critic_flat, L.actor_exp_avg)
            update = (it + 1) % 2 == 0
            assert ('soft_update' in double.calls) == update, (sched, it, double.calls)
            assert double.calls.count('adam_step_dev') == (2 if update else 1)
            assert double.calls.count('ddpg_stats') == 1
            for a, b in zip(before, after):
                assert torch.equal(a, b) != update, (sched, it)


@pytest.mark.parametrize('name', ['tiny_soft_clipcritic', 'tiny_ln_td3_soft'])
@pytest.mark.parametrize('sched', ['rows', 'layers'])
def test_delay_one_is_the_learner_without_the_key(double, name, sched):
    case = DH.load(name)[1]
    runs = []
    for kw in ({}, {'policy_delay': 1}):
        del double.calls[:]
        L = DC.make_learner(case, DC.schedules(name)[sched], **kw)
        stats = [dict(L.learn(DC.batch(case, it))) for it in range(3)]
        assert L._ws.astep is None and 'policy_delay' not in L.train_state_dict()['words']
        runs.append((list(double.calls), flats(L), stats))
    assert runs[0][0] == runs[1][0]
    assert 'ddpg_rows_delay_tail' not in runs[0][0] and 'ddpg_rows_critic_only' not in runs[0][0]
    same_bytes(runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2]


@pytest.mark.parametrize('bad', [0, -1, 2.0, '2', True, None])
def test_a_delay_that_is_no_positive_integer_is_refused(double, bad):
    from surreal_amd.session import ConfigError
    case = DH.load('tiny_soft_clipcritic')[1]
    del double.calls[:]
    with pytest.raises(ConfigError, match='policy_delay'):
        DC.make_learner(case, ROWS, policy_delay=bad)
    assert double.calls == []


def test_a_delay_with_hard_target_updates_is_refused(double, monkeypatch):
    from surreal_amd.session import ConfigError
    import surreal_amd.learner.ddpg as LD
    case = DH.load('tiny_soft_clipcritic')[1]
    built = []
    monkeypatch.setattr(LD, 'DDPGModel', lambda *a, **kw: built.append(1))
    with pytest.raises(ConfigError, match='policy_delay'):
        DC.make_learner(case, ROWS, policy_delay=2, hard=True)
    assert built == []                               # nothing allocated
    monkeypatch.undo()
    L = DC.make_learner(case, ROWS, policy_delay=1, hard=True)       # (d = 1 keeps hard updates)
    assert L.policy_delay == 1 and L.target_update_type == 'hard'


@pytest.mark.parametrize('sched', ['rows', 'layers'])
def test_training_state_carries_the_delay_and_resumes(double, sched):
    name = 'tiny_ln_td3_soft'
    case = DH.load(name)[1]
    opts = DC.schedules(name)[sched]
    A = DC.make_learner(case, opts, policy_delay=2)
    for it in range(3):
        A.learn(DC.batch(case, it))
    sd = A.train_state_dict()
    assert sd['words']['policy_delay'] == 2 and sd['words']['actor_step'] == 1 and sd['words']['critic_step'] == 3
    sd = {'kind': sd['kind'], 'workspace': sd['workspace'], 'words': dict(sd['words']),
          'tensors': {k: v.clone() for k, v in sd['tensors'].items()}}
    for it in range(3, DC.ITERS):
        A.learn(DC.batch(case, it))
    B = DC.make_learner(case, opts, policy_delay=2)
    B.learn(DC.batch(case, 5))                        # (a workspace and a history of its own, then the state over it)
    B.load_train_state_dict(sd)
    assert int(B._ws.astep[0]) == 1 and int(B._ws.step[0]) == 3 and B._ws.rows_versions is None
    for it in range(3, DC.ITERS):
        B.learn(DC.batch(case, it))
    same_bytes(flats(A), flats(B))
    # another delay: refused before anything is written
    for other in (DC.make_learner(case, opts, policy_delay=3), DC.make_learner(case, opts)):
        before = flats(other)
        with pytest.raises(ValueError, match='policy_delay'):
            other.load_train_state_dict(sd)
        same_bytes(before, flats(other))
    plain = DC.make_learner(case, opts).train_state_dict()
    with pytest.raises(ValueError, match='policy_delay'):
        DC.make_learner(case, opts, policy_delay=2).load_train_state_dict(plain)


def test_a_double_without_the_capability_stays_on_layers():
    """the existing LayerNorm TD3 double knows nothing of ddpg_rows_delay: asked for the rows at d = 2 the learner runs
    layer by layer -- and matches the restatement; at d = 1 it takes the rows as before"""
    from surreal_amd import kernels as KN
    K = LT.LnTd3RowsCpuKernels()
    prev = KN.set_default_kernels(K, 'cpu')
    try:
        L = DC.run_against_reference('tiny_ln_td3_soft', ROWS, 2)
        assert L._schedule(*L._ws.key) == 'layers'
        assert not any(c.startswith('ddpg_rows') for c in K.calls)
        L1 = DC.make_learner(DH.load('tiny_ln_td3_soft')[1], ROWS)
        assert L1._schedule(L1.batch_size, DH.load('tiny_ln_td3_soft')[1]['D']) == 'rows'
    finally:
        KN.set_default_kernels(*prev)


def test_the_key_changes_the_result():
    """the restatements at d = 2 and d = 3 end far from d = 1's: a learner that ignored the key could not pass"""
    for name in DC.LOW_CASES:
        base = DC.reference(name, 1)[1]
        for d in DC.DELAYS:
            other = DC.reference(name, d)[1]
            gap = max(float(np.abs(base['model'][k] - other['model'][k]).max()) for k in base['model'])
            assert gap > 100 * DH.PARAM_ATOL_DEFAULT, (name, d, gap)


# ---- scripts/train_reach.py's options ----------------------------------------------------------------------------------

def train_reach():
    import os
    import sys
    scripts = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts')
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import train_reach as TR
    return TR


def test_train_reach_refuses_the_options_for_ppo():
    TR = train_reach()
    small = dict(actors=8, J=1, episode_len=5, iters=1, log=lambda s: None)
    with pytest.raises(ValueError, match='DDPG only'):
        TR.train('ppo', double_critic=True, **small)
    with pytest.raises(ValueError, match='DDPG only'):
        TR.train('ppo', policy_delay=2, **small)


def test_train_reach_runs_td3_with_a_delay_on_the_double(monkeypatch):
    """a short run of the loop with --double-critic --policy-delay 2 on the double: the row schedule, critic-only iterations
    at the odd ones, and the options in the lines that name the run"""
    from surreal_amd import kernels as KN
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    TR = train_reach()
    K = DC.ReachDelayCpuKernels()
    prev = KN.set_default_kernels(K, 'cpu')
    try:
        monkeypatch.setattr(SyntheticVecEnv, 'attach_noise', lambda self, seed, actor_base=0: None)
        lines = []
        base, curve = TR.train('ddpg', actors=64, J=1, episode_len=20, iters=2, eval_every=1, device='cpu',
                               log=lines.append, double_critic=True, policy_delay=2)
        assert base['double_critic'] is True and base['policy_delay'] == 2
        assert curve[-1]['learner_iterations'] == 40           # (both chunks fill the replay past 4 batches)
        n_only, n_full = K.calls.count('ddpg_rows_critic_only_td3'), K.calls.count('ddpg_rows_critic_td3')
        assert n_only == n_full == 20 and K.calls.count('ddpg_rows_delay_tail') == 20
        loop = TR.Loop('ddpg', 8, 1, 5, 0, 'cpu', double_critic=True, policy_delay=2)
        ident = loop.identity()
        assert ident['double_critic'] is True and ident['policy_delay'] == 2
        assert loop.learner.policy_delay == 2 and loop.learner.use_double_critic and loop.learner.row_schedule is True
        plain = TR.Loop('ddpg', 8, 1, 5, 0, 'cpu')
        assert set(plain.identity()) == {'algo', 'actors', 'J', 'episode_len', 'seed', 'random_resets', 'heldout'}
    finally:
        KN.set_default_kernels(*prev)
