"""GPU tier (-m gpu): several parameter snapshots of a policy evaluated in ONE launch (DeviceEvalSnapshots;
smx_eval_snapshot_store_f32, smx_synth_ppo_eval_sets_f32 / smx_synth_ddpg_eval_sets_f32: the SETS instantiations of
ppo_eval_kernel / ddpg_eval_kernel).  Shapes (device_eval_cases): (n, E, L) = (5, 3, 7), (1, 1, 1), (9, 2, 4) -- 15, 1 and
18 rows PER SET: a tail block per set at every block size, two blocks per set at 16 rows per workgroup -- each at 4, 8, 16
rows per workgroup and at the automatic size; K = 3 snapshots from three parameter seeds (PPO: three z-filter states).

Every check is an equality of bits (fp64 returns compared as uint64); the oracle is the single-set launch
(SyntheticVecEnv.evaluate) or the host definition (device_eval_cases.host_returns):

  1. against the single-set launch, every policy of device_eval_cases, deterministic and (PPO) sampling;
  2. indexing: K = 1, a window of slots, a permutation of the slots;
  3. snapshot semantics: a stored slot does not follow the agent; storing again does;
  4. against the host definition under constant actions;
  5. a parameter-noise population as snapshots (zero copy);
  6. fences around and between the snapshots and the returns, the padding inside a snapshot;
  7. purity: chunk, store + evaluate, chunk on the training env;
  8. the refusals, raised before any launch;
  9. scripts/train_reach.py --snapshot-curve.

47 tests, 4.2 s together on an MI355X.
"""
import numpy as np
import pytest
import torch

import device_eval_cases as EV
import eval_sets_cases as ES
from surreal_amd import _lib as L
from surreal_amd import kernels as KN

pytestmark = pytest.mark.gpu

DEV = 'cuda'
IDS = [p.id for p in EV.POLICIES]


def variants(p, n):
    """the start states of a case: resets (seed, first_episode, actor_base) or None (test_gpu_device_eval's)"""
    if p.task != 'reach':
        return [None]
    return [None, (EV.RSEED, EV.FIRST_EPISODES[0], 0), (EV.RSEED, EV.FIRST_EPISODES[1], 2 ** 32 - n)]


def all_blocks(snaps, E, resets=None, noise=None, **kw):
    """evaluate at 4, 8 and 16 rows per workgroup and at the automatic size: the same bytes -> them"""
    got = [ES.evaluate_sets(snaps, E, resets, noise, apw, **kw) for apw in EV.BLOCKS + (0,)]
    assert got[0].dtype == np.float64 and got[0].shape[1:] == (snaps.env.n, E)
    for g in got[1:]:
        assert EV.same_f64(g, got[0])
    return got[0]


# ---- 1. against the single-set launch ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('p', EV.POLICIES, ids=IDS)
def test_every_set_has_the_bits_of_the_single_set_launch(p):
    for n, E, L_ in EV.SHAPES:
        ags = ES.agents(p, n)
        venv = EV.make_env(p, n, L_, DEV)
        snaps = ES.stored(venv, ags)
        for resets in variants(p, n):
            got = all_blocks(snaps, E, resets)
            assert got.shape == (ES.K_SETS, n, E) and np.isfinite(got).all()
            for k, agent in enumerate(ags):
                want = EV.evaluate(venv, agent, E, resets)
                assert EV.same_f64(got[k], want), (n, E, L_, resets, k, got[k], want)
            assert not EV.same_f64(got[0], got[1]) and not EV.same_f64(got[1], got[2])     # (the sets differ)


@pytest.mark.parametrize('p', [q for q in EV.POLICIES if q.family != 'ddpg'], ids=lambda q: q.id)
def test_sampling_sets_have_the_bits_of_the_single_set_launch(p):
    """eval_stochastic: row (a, i) of EVERY set draws normal(seed, actor_base + a, first_step + i L + t, j)"""
    for n, E, L_ in EV.SHAPES:
        ags = ES.agents(p, n, mode='eval_stochastic_local')
        venv = EV.make_env(p, n, L_, DEV)
        snaps = ES.stored(venv, ags)
        noise = (EV.NSEED, EV.FIRST_STEP, 0)
        for resets in variants(p, n):
            got = all_blocks(snaps, E, resets, noise)
            for k, agent in enumerate(ags):
                assert EV.same_f64(got[k], EV.evaluate(venv, agent, E, resets, noise)), (n, E, L_, resets, k)
        det = ES.agents(p, n)
        assert not EV.same_f64(got[0], EV.evaluate(venv, det[0], E, variants(p, n)[-1]))   # (the draws matter)


# ---- 2. indexing ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pid', ['mlp-reach-J2', 'lstm-reach-J2', 'ddpg-reach-J2', 'mlp-drift-17-6'])
def test_one_set_a_window_of_slots_and_a_permutation(pid):
    p = EV.BY_ID[pid]
    for n, E, L_ in EV.SHAPES:
        ags = ES.agents(p, n)
        venv = EV.make_env(p, n, L_, DEV)
        resets = variants(p, n)[-1]
        one = venv.eval_snapshots(ags[1], 1)
        one.store(0)
        assert EV.same_f64(all_blocks(one, E, resets)[0], EV.evaluate(venv, ags[1], E, resets))
        full = all_blocks(ES.stored(venv, ags), E, resets)
        snaps = ES.stored(venv, ags)
        assert EV.same_f64(all_blocks(snaps, E, resets, first=1, count=2), full[1:3])
        assert EV.same_f64(all_blocks(snaps, E, resets, first=2), full[2:3])
        order = (2, 0, 1)
        perm = all_blocks(ES.stored(venv, ags, order), E, resets)
        for k, slot in enumerate(order):
            assert EV.same_f64(perm[slot], full[k])


# ---- 3. snapshot semantics ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pid', ['mlp-reach-J2', 'lstm-reach-J2', 'ddpg-reach-J2'])
def test_a_slot_keeps_its_bits_when_the_agent_changes_until_it_is_stored_again(pid):
    p = EV.BY_ID[pid]
    n, E, L_ = EV.SHAPES[0]
    a, b, _ = ES.agents(p, n)
    venv = EV.make_env(p, n, L_, DEV)
    resets = variants(p, n)[-1]
    want_a, want_b = EV.evaluate(venv, a, E, resets), EV.evaluate(venv, b, E, resets)
    assert not EV.same_f64(want_a, want_b)
    snaps = venv.eval_snapshots(a, 2)
    snaps.store(0)
    snaps.store(1)
    ES.overwrite(a, b)                                   # in place: parameters, log_var, z-filter, LSTM
    assert EV.same_f64(EV.evaluate(venv, a, E, resets), want_b)
    got = ES.evaluate_sets(snaps, E, resets)
    assert EV.same_f64(got[0], want_a) and EV.same_f64(got[1], want_a)
    snaps.store(1)
    got = ES.evaluate_sets(snaps, E, resets)
    assert EV.same_f64(got[0], want_a) and EV.same_f64(got[1], want_b)


# ---- 4. against the host definition --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pid', ['mlp-reach-J2', 'lstm-reach-J2', 'mlp-drift-17-6'])
def test_constant_policies_are_the_host_definition(pid):
    """zero weights and output bias 0 / 0.3 / 1.7 in the three slots, on an identity head (out_act = none, as
    test_gpu_device_eval's constant-action test: the action is the bias, 1.7 clipped to 1, at every step): row k is
    host_returns of its constant, bit for bit.  reach with a reset stream, drift from init_state"""
    p = EV.BY_ID[pid]
    K = KN.default_kernels()
    values = (0.0, 0.3, 1.7)
    for n, E, L_ in EV.SHAPES:
        ags = ES.agents(p, n)
        for agent, v in zip(ags, values):
            EV.constant_policy(agent, v)
        venv = EV.make_env(p, n, L_, DEV)
        snaps = ES.stored(venv, ags)
        m = ags[0].model
        resets = variants(p, n)[-1]
        want = [EV.host_returns(p, n, E, L_, v, resets, venv.init_state.cpu().numpy()) for v in values]
        for apw in EV.BLOCKS + (0,):
            out = torch.empty(3, n, E, dtype=torch.float64, device=DEV)
            K.synth_ppo_eval_sets(m, snaps.buf, venv.init_state, E, L_, out, zfilter=m.z_filter, task=p.task,
                                  resets=None if resets is None else (resets[0], resets[2], resets[1]),
                                  actors_per_workgroup=apw, out_act=L.SMX_ACT_NONE)
            got = out.cpu().numpy()
            for k in range(3):
                assert EV.same_f64(got[k], want[k]), (n, E, L_, apw, k, got[k], want[k])
        assert not EV.same_f64(want[0], want[1]) and not EV.same_f64(want[1], want[2])


@pytest.mark.parametrize('pid', ['ddpg-reach-J2', 'ddpg-drift-17-6'])
def test_the_zero_ddpg_actor_is_the_host_definition(pid):
    """a DDPG actor's head is tanh: its one constant the host states exactly is 0 (slot 1 of 3; the others are live actors)"""
    p = EV.BY_ID[pid]
    for n, E, L_ in EV.SHAPES:
        ags = ES.agents(p, n)
        EV.constant_policy(ags[1], 0.0)
        venv = EV.make_env(p, n, L_, DEV)
        resets = variants(p, n)[-1]
        got = all_blocks(ES.stored(venv, ags), E, resets)
        assert EV.same_f64(got[1], EV.host_returns(p, n, E, L_, 0.0, resets, venv.init_state.cpu().numpy()))
        assert EV.same_f64(got[0], EV.evaluate(venv, ags[0], E, resets)) and not EV.same_f64(got[0], got[1])


# ---- 5. a parameter-noise population -------------------------------------------------------------------------------------------------

def test_a_parameter_noise_population_is_an_array_of_snapshots():
    from surreal_amd.env import DeviceEvalSnapshots
    p = EV.BY_ID['ddpg-reach-J2']
    n, E, L_ = 12, 2, 5
    train, _ = EV.ddpg_agent(p, n, mode='training', param_noise_type='normal')
    venv = EV.make_env(p, n, L_, DEV)
    pn = venv.attach_param_noise(train, seed=77, actors_per_agent=4)
    assert pn.agents == 3 and not pn.ln
    before = pn.state_dict()
    snaps = DeviceEvalSnapshots.from_param_noise(venv, pn)
    assert snaps.buf.data_ptr() == pn.pop.data_ptr() and snaps.capacity == 3
    resets = (EV.RSEED, 5, 0)
    got = all_blocks(snaps, E, resets)
    clean = EV.make_env(p, n, L_, DEV)
    for k in range(3):
        fresh, _ = EV.ddpg_agent(p, n)
        with torch.no_grad():
            for name, v in pn.perturbed(k).items():
                fresh.model.actor.views[name].copy_(v)
        assert EV.same_f64(got[k], EV.evaluate(clean, fresh, E, resets)), k
    assert not EV.same_f64(got[0], got[1])
    after = pn.state_dict()
    assert before.keys() == after.keys()
    for k in before:
        if torch.is_tensor(before[k]):
            assert torch.equal(before[k].view(torch.uint8), after[k].view(torch.uint8)), k
        else:
            assert before[k] == after[k], k


def test_a_layernorm_population_is_refused():
    from surreal_amd.env import DeviceEvalSnapshots
    p = EV.BY_ID['ddpg-reach-J2']._replace(task='drift')
    n = 8
    train, _ = EV.ddpg_agent(p, n, mode='training', layernorm=True, param_noise_type='normal')
    venv = EV.make_env(p, n, 4, DEV)
    pn = venv.attach_param_noise(train, seed=5, actors_per_agent=4)
    assert pn.ln
    with pytest.raises(NotImplementedError, match='LayerNorm'):
        DeviceEvalSnapshots.from_param_noise(venv, pn)


# ---- 6. fences ------------------------------------------------------------------------------------------------------------------------

SENT32, SENT64 = -7.25e9, -3.0e200


@pytest.mark.parametrize('pid', ['mlp-reach-J2', 'lstm-reach-J21', 'ddpg-reach-J1', 'lstm-drift-17-6'])
def test_store_and_evaluate_write_nothing_outside_their_floats(pid):
    p = EV.BY_ID[pid]
    K = KN.default_kernels()
    n, E, L_ = EV.SHAPES[0]
    ags = ES.agents(p, n)
    ppo = p.family != 'ddpg'
    venv = EV.make_env(p, n, L_, DEV)
    m0 = ags[0].model
    floats = K.eval_snapshot_floats(model=m0, zfilter=True) if ppo else K.eval_snapshot_floats(actor=m0.actor)
    lay = ES.snapshot_layout(*ES.policy_dims(p), int(ppo))
    assert floats == lay['total']
    pad, stride, S = 64, floats + 64, ES.K_SETS
    big = torch.full((pad + S * stride + pad,), SENT32, device=DEV)
    blobs = big[pad:pad + S * stride].view(S, stride)
    for k, a in enumerate(ags):
        if ppo:
            K.eval_snapshot_store(blobs[k, :floats], model=a.model, zfilter=a.model.z_filter)
        else:
            K.eval_snapshot_store(blobs[k, :floats], actor=a.model.actor)
    rbig = torch.full((8 + S * n * E + 8,), SENT64, dtype=torch.float64, device=DEV)
    rets = rbig[8:8 + S * n * E].view(S, n, E)
    resets = None if p.task != 'reach' else (EV.RSEED, 2 ** 32 - n, EV.FIRST_EPISODES[1])
    for apw in EV.BLOCKS:
        rets.fill_(SENT64)
        if ppo:
            K.synth_ppo_eval_sets(m0, blobs, venv.init_state, E, L_, rets, zfilter=m0.z_filter, task=p.task, resets=resets,
                                  actors_per_workgroup=apw)
        else:
            K.synth_ddpg_eval_sets(m0.actor, blobs, venv.init_state, E, L_, rets, task=p.task, resets=resets,
                                   actors_per_workgroup=apw)
        got = rets.cpu().numpy()
        assert (rbig[:8] == SENT64).all() and (rbig[-8:] == SENT64).all() and (got != SENT64).all()
        for k, a in enumerate(ags):
            want = EV.evaluate(venv, a, E, None if resets is None else (resets[0], resets[2], resets[1]), apw=apw)
            assert EV.same_f64(got[k], want), (apw, k)
    host = big.cpu().numpy()
    assert (host[:pad] == np.float32(SENT32)).all() and (host[-pad:] == np.float32(SENT32)).all()
    order = sorted((v, k) for k, v in lay.items() if k not in ('end', 'total'))
    sizes = {'b1': p.hidden[0], 'b2': p.hidden[1], 'b3': p.A, 'log_var': p.A, 'zsum': p.D, 'zsumsq': p.D, 'zcount': 1}
    for k in range(S):
        row = host[pad + k * stride:pad + (k + 1) * stride]
        assert (row[floats:] == np.float32(SENT32)).all(), k                  # between this snapshot and the next
        assert not (row[:floats] == np.float32(SENT32)).any(), k              # all of the snapshot was written
        # the padding between the small arrays and behind the last block is exactly zero
        for (o, name), nxt in zip(order, [v for v, _ in order[1:]] + [None]):
            if name in sizes:
                gap = row[o + sizes[name]:nxt if nxt is not None else lay['total']]
                assert gap.size < 64 and not gap.any(), (k, name)
        assert not row[lay['end']:floats].any(), k
        assert np.array_equal(row[lay['b3']:lay['b3'] + p.A], ags[k].model.actor.views['b3'].cpu().numpy().reshape(-1))


# ---- 7. purity ---------------------------------------------------------------------------------------------------------------------------

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
def test_store_and_evaluate_between_two_training_chunks_change_nothing(pid):
    p = EV.BY_ID[pid]
    n, L_, T = 9, 5, 7                                       # (chunks of 7 over episodes of 5: the second starts mid-episode)

    def sequence(with_sets):
        from surreal_amd.replay import FIFOReplay, UniformReplay
        train, cfg = EV.make_agent(p, n, mode='training', n_step=3, **({'stride': 2} if p.family != 'ddpg' else {}))
        ev, other = ES.agents(p, n)[:2]
        venv = EV.make_env(p, n, L_, DEV)
        venv.attach_monitor(capacity=4)
        venv.attach_noise(EV.NSEED)
        venv.attach_resets(EV.RSEED)
        venv.reset()
        replay = (UniformReplay if p.family == 'ddpg' else FIFOReplay)(*cfg)
        roll = venv.ddpg_rollout_into if p.family == 'ddpg' else venv.ppo_rollout_into
        roll(train, replay, T)
        if with_sets:
            before = _snapshot(venv, replay, train)
            snaps = venv.eval_snapshots(ev, 2)
            snaps.store(0)
            snaps.store(1, other)
            for kw in (dict(resets=(EV.RSEED + 1, 0)), dict()):
                got = snaps.evaluate(2, **kw)
                assert got.shape == (2, n, 2) and bool(torch.isfinite(got).all())
            _same_snapshot(before, _snapshot(venv, replay, train))
        roll(train, replay, T)
        torch.cuda.synchronize()
        return _snapshot(venv, replay, train)
    _same_snapshot(sequence(False), sequence(True))


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_come_before_any_launch(monkeypatch):
    calls = []
    orig = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), orig(name, *a))[1])
    launched = lambda: [c for c in calls if 'eval' in c]  # noqa: E731
    snaps, refused, ctx = ES.check_python_refusals(DEV, None)
    assert launched() == [], calls
    snaps.store(0)
    snaps.store(1)
    assert launched() == ['smx_eval_snapshot_store_f32'] * 2
    ES.check_evaluate_refusals(snaps, refused, ctx, DEV)
    assert launched() == ['smx_eval_snapshot_store_f32'] * 2, calls
    ES.check_entry_point_codes()


# ---- 9. train_reach.py --snapshot-curve ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('heldout', [False, True])
def test_train_reach_snapshot_curve_has_the_bits_of_the_per_point_evaluations(heldout):
    """`train_reach.py --algo ddpg --device-eval --snapshot-curve [--eval-heldout]` (its train(), in this process): 64
    actors x 8 steps a chunk, so that the learner starts at the third chunk and the three points (iterations 0, 3, 6) differ.  The script
    itself asserts that every point has the bits of the per-point device evaluation; here: one value per point, those
    values the per-point lines' own"""
    import json
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))
    import train_reach as TR
    lines = []
    base, curve = TR.train('ddpg', actors=64, J=2, episode_len=8, iters=6, seed=0, eval_every=3, log=lines.append,
                           eval_heldout=heldout, heldout_episodes=2, device_eval=True, snapshot_curve=True)
    rows = [json.loads(ln) for ln in lines]
    points = [r for r in rows if 'iteration' in r]
    (last,) = [r for r in rows if r.get('kind') == 'snapshot_curve']
    assert rows[-1] is last and curve[-1] == last and last['bits_match'] is True
    assert last['points'] == len(points) == 3 and last['iterations'] == [0, 3, 6] and last['episodes'] == (2 if heldout else 1)
    assert len(last['mean_return']) == 3 and len(set(last['mean_return'])) == 3          # (the learner moved the actor)
    assert points[-1]['learner_iterations'] > 0
    for r, v in zip(points, last['mean_return']):
        assert abs(r['eval_return'] - v) <= 1e-9 * abs(v)          # (two means of the same bits, numpy's and torch's)
    # without the flag the lines are what they were
    plain = []
    TR.train('ddpg', actors=64, J=2, episode_len=8, iters=6, seed=0, eval_every=3, log=plain.append, eval_heldout=heldout,
             heldout_episodes=2, device_eval=True)
    # (the same lines with the same fields; their values are the purity test's business)
    shape = lambda ln: (sorted(json.loads(ln)), json.loads(ln).get('iteration'))  # noqa: E731
    assert [shape(ln) for ln in plain] == [shape(ln) for ln in lines[:-1]]
