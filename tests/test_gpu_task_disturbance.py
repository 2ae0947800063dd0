"""GPU tier (-m gpu): the per-step disturbance of `reach` and `arm` on the device (struct smx_reset_stream's scale;
disturbance_uniform of csrc/smx_philox.inc.h) -- the per-step launch (reach_env_step_kernel / arm_env_step_kernel) and
EnvLanes::step_reach / step_arm inside ppo_window_task_kernel, lstm_window_task_kernel, the four ddpg_rollout_kernel actors
and the evaluation kernels (single-set and SETS), at 4, 8 and 16 actors per workgroup.  Shapes (task_disturbance_cases.py):
reach J = 1, 2, 5, 21 and arm J = 1, 2, 5, 30 (J = 5: a second Philox block; 21 / 30: the widest rows); n = 5 (a tail block),
8 for populations and split envs; episodes of 5 over calls of 3 + 4 + 5 steps, two episode ends inside calls.

  1. every recorded (obs, action, obs_next, reward) row, fed to the host step with the draws the host definition gives for
     its (seed, actor, episode, step), reproduces obs_next and reward; the four DDPG actors and the per-step launch against
     host chains over SyntheticEnv(disturbance=);
  2. 4, 8 and 16 actors per workgroup, other cuts into calls, and two envs of 4 (actor_base 0 and 4) against one of 8 leave
     the same bytes;
  3. scale 0 leaves the bytes of a stream built without the field, in the replay, the state and the monitor;
  4. evaluate and the snapshot sets equal the recording launches' monitor for the same (seed, actor, episode, scale) as
     uint64, the host definition under a constant action, differ from the scale-0 returns, and touch nothing;
  5. one save / resume of a training loop with a disturbance on, byte for byte;
  6. the entry points refuse a bad scale or episode before any launch.

All equalities of bits."""
import numpy as np
import pytest
import torch

import arm_cases as AC
import device_eval_cases as EV
import reach_resets_cases as RR
import rollout_envelope_cases as EC
import task_disturbance_cases as TD
from surreal_amd import _lib as L
from surreal_amd.env import tasks as TK

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BLOCKS = (4, 8, 16)
_RUNS = {}


def spare_run(c, apw):
    """the case on the disturbed stream at a forced block size (once per module)"""
    if (c.id, apw) not in _RUNS:
        x = TD.setup(c, DEV)
        got, rows = TD.run(x, apw)
        assert x.resets.episode == 1 + sum(TD.CALLS) // TD.EP
        _RUNS[(c.id, apw)] = (got, x, rows, AC.monitor_returns(x.venv.monitor, x.c.n))
    return _RUNS[(c.id, apw)]


@pytest.mark.parametrize('c', TD.CASES, ids=lambda c: c.id)
def test_rows_hold_the_host_step_with_the_host_draws_at_every_block_size(c):
    first = None
    for apw in BLOCKS:
        got, x, rows, mon = spare_run(c, apw)
        if first is None:
            first = got
            returns = TD.check_rows(got, x, rows)                                   # (1)
            assert TD.draws_move_the_rows(got, x, rows)
            if returns is not None:
                assert [r[:2] for r in mon] == returns and all(len(r) == 2 for r in returns)
        EC.same_bits(got, first)                                                    # (2)
        assert mon == spare_run(c, BLOCKS[0])[3]


@pytest.mark.parametrize('task,J', [('reach', 2), ('reach', 21), ('arm', 5), ('arm', 30)])
@pytest.mark.parametrize('variant', [dict(), dict(layernorm=True), dict(param_noise='normal', n=8),
                                     dict(layernorm=True, param_noise='normal', n=8)], ids=['plain', 'ln', 'pop', 'popln'])
def test_ddpg_actors_whole_steps_and_monitor_returns(task, J, variant):
    # (a population's block holds the actors of ONE agent: agents of 4 actors run at 4 actors per workgroup)
    for apw in ((4, 0) if 'param_noise' in variant else BLOCKS):
        got, want = TD.whole_steps(DEV, task=task, J=J, apw=apw, **variant)
        assert got == want and all(len(r) == 2 for r in got)


@pytest.mark.parametrize('task,J', [('reach', 1), ('reach', 5), ('reach', 21), ('arm', 1), ('arm', 5), ('arm', 30)])
def test_per_step_launch_matches_the_host_env(task, J):
    TD.per_step_chains(DEV, task=task, J=J)


@pytest.mark.parametrize('c', TD.CASES, ids=lambda c: c.id)
def test_other_cuts_into_calls_leave_the_same_bytes(c):
    got = spare_run(c, 8)[0]
    for calls in ((12,), (5, 5, 2)):
        x = TD.setup(c, DEV)
        EC.same_bits(TD.run(x, 8, calls=calls)[0], got)


@pytest.mark.parametrize('cid', ['reach-window-J5', 'reach-lstm_window-J2', 'reach-ddpg-J21', 'arm-window-J30',
                                 'arm-lstm_window-J5', 'arm-ddpg-J5'])
def test_two_envs_of_four_record_what_one_of_eight_records(cid):
    c = TD.BY_ID[cid]
    for apw in (4, 8):
        (big, gb, rows), small = TD.split_envs(c, DEV, apw=apw)
        RR.same_actors(gb, small, rows)
        assert AC.monitor_returns(big.venv.monitor, 8) == sum((AC.monitor_returns(x.venv.monitor, 4) for x, _ in small), [])


@pytest.mark.parametrize('c', TD.CASES, ids=lambda c: c.id)
def test_scale_zero_leaves_the_bytes_of_a_stream_without_the_field(c):
    xs = [TD.setup(c, DEV, scale=s) for s in (None, 0.0)]
    (a, rows), (b, _) = (TD.run(x, 8) for x in xs)
    EC.same_bits(a, b)                                                              # (3)
    assert all(torch.equal(p, q) for p, q in zip(TD.monitor_bytes(xs[0]), TD.monitor_bytes(xs[1])))
    TD.check_rows(a, xs[0], rows, scale=0.0)
    assert not torch.equal(a['state'], spare_run(c, 8)[0]['state'])


# ---- (4) evaluation ------------------------------------------------------------------------------------------------------------

POLICIES = [EV.Policy('mlp-reach-J5', 'mlp', 'reach', 15, 5, (32, 32)),
            EV.Policy('lstm-reach-J21', 'lstm', 'reach', 63, 21, EV.RAGGED),
            EV.Policy('ddpg-reach-J1', 'ddpg', 'reach', 3, 1, EV.RAGGED),
            EV.Policy('mlp-arm-J30', 'mlp', 'arm', 62, 30, EV.RAGGED),
            EV.Policy('lstm-arm-J2', 'lstm', 'arm', 6, 2, (32, 32)),
            EV.Policy('ddpg-arm-J5', 'ddpg', 'arm', 12, 5, (32, 32))]
SHAPES = [(5, 3, 5), (9, 2, 4)]                            # (n, E, L): 15 rows, 18 rows


def evaluate(venv, agent, E, resets, scale, apw=0):
    out = venv.evaluate(agent, E, resets=resets, actors_per_workgroup=apw, disturbance=scale)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('p', POLICIES, ids=lambda q: q.id)
def test_evaluate_and_snapshot_sets_are_the_monitor_of_the_recording_launches(p):
    for n, E, L_ in SHAPES:
        agent, cfg = EV.make_agent(p, n)
        other, _ = EV.make_agent(p, n, seed=11)
        resets = (EV.RSEED, 2 ** 32 - 1 - E, 2 ** 32 - n)                  # (seed, first_episode, actor_base)
        venv = EV.make_env(p, n, L_, DEV)
        got = [evaluate(venv, agent, E, resets, TD.SCALE, apw) for apw in BLOCKS + (0,)]
        assert all(EV.same_f64(g, got[0]) for g in got[1:]) and got[0].shape == (n, E)
        want = TD.recorded_returns(p, n, E, L_, agent, cfg, DEV, (resets[0], resets[1], resets[2]), TD.SCALE)
        assert EV.same_f64(got[0], want), (n, E, L_, got[0], want)
        plain = evaluate(venv, agent, E, resets, None)
        assert EV.same_f64(plain, evaluate(venv, agent, E, resets, 0.0))
        assert np.isfinite(got[0]).all() and (got[0] != plain).all()
        snaps = venv.eval_snapshots(agent, 2)
        snaps.store(0)
        snaps.store(1, other)
        for apw in BLOCKS:
            sets = snaps.evaluate(E, resets=resets, actors_per_workgroup=apw, disturbance=TD.SCALE).cpu().numpy()
            assert EV.same_f64(sets[0], got[0]) and EV.same_f64(sets[1], evaluate(venv, other, E, resets, TD.SCALE))
        assert not EV.same_f64(sets[0], sets[1])


@pytest.mark.parametrize('p', [POLICIES[0], POLICIES[4], POLICIES[5]], ids=lambda q: q.id)
def test_zero_policy_returns_are_the_host_definition(p):
    for n, E, L_ in SHAPES:
        agent, _ = EV.make_agent(p, n)
        EV.constant_policy(agent, 0.0)
        resets = (EV.RSEED, 3, 2 ** 32 - n)
        venv = EV.make_env(p, n, L_, DEV)
        got = evaluate(venv, agent, E, resets, TD.SCALE)
        assert EV.same_f64(got, TD.host_eval_returns(p.task, p.A, n, E, L_, 0.0, resets, TD.SCALE)), (n, E, L_)


def test_evaluate_is_pure_on_a_disturbed_training_env():
    c = TD.BY_ID['arm-ddpg-J5']
    x = TD.setup(c, DEV)
    TD.run(x, 0, calls=(3,))
    venv = x.venv
    before = ([venv.state.clone(), venv.t, x.resets.episode] + [t.clone() for t in TD.monitor_bytes(x)]
              + [v.clone() for v in venv._ddpg.values() if torch.is_tensor(v)])
    p = EV.Policy('ddpg-arm-J5', 'ddpg', 'arm', 12, 5, (32, 32))
    agent, _ = EV.make_agent(p, x.c.n)
    a = evaluate(venv, agent, 2, (AC.RSEED, 0), TD.SCALE)
    b = evaluate(venv, agent, 2, (AC.RSEED, 0), TD.SCALE)
    assert EV.same_f64(a, b)
    after = ([venv.state, venv.t, x.resets.episode] + TD.monitor_bytes(x)
             + [v for v in venv._ddpg.values() if torch.is_tensor(v)])
    assert len(before) == len(after)
    for p_, q_ in zip(before, after):
        assert torch.equal(p_.cpu(), q_.cpu()) if torch.is_tensor(p_) else p_ == q_
    # the training run goes on as if nothing had happened
    if x.eps is not None:
        x.eps = x.eps[3:]
    rest = TD.run(x, 0, calls=(4, 5))[0]
    EC.same_bits(rest, spare_run(c, 0)[0])


# ---- (5) save / resume ---------------------------------------------------------------------------------------------------------

def test_a_disturbed_training_loop_resumes_byte_for_byte(tmp_path):
    """scripts/train_reach.py's loop (random resets, a disturbance, DDPG learning on both sides of the cut): saved after
    three chunks, two more; a fresh loop from the file, two more: the learner, the replay and the env hold the same bytes"""
    import os
    import sys
    scripts = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts')
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import train_reach as TR
    import run_state_cases as RSC
    from surreal_amd.utils import run_state as RS

    def loop(scale=0.25):
        return TR.Loop('ddpg', 64, 2, 8, 0, DEV, folder=str(tmp_path / 'session'), random_resets=True, heldout=2,
                       disturbance=scale)

    def record(lp):
        return RS.to_host({'learner': lp.learner.train_state_dict(), 'replay': lp.replay.state_dict(),
                           'env': lp.venv.state_dict(), 'eval': lp.evaluate_device(), 'learns': lp.learns})
    whole = loop()
    assert whole.identity()['disturbance'] == 0.25 and whole.venv.resets.disturbance == 0.25
    for _ in range(3):
        whole.iterate()
    path = str(tmp_path / 'run.pt')
    RS.save_run(path, **whole.state_parts(iteration=3, base={}))
    learns = whole.learns
    for _ in range(2):
        whole.iterate()
    assert 0 < learns < whole.learns and whole.venv.state_dict()['resets']['disturbance'] == 0.25
    resumed = loop()
    resumed.load_parts(RS.load_run(path))
    for _ in range(2):
        resumed.iterate()
    RSC.assert_same(record(resumed), record(whole), 'a disturbed run resumed from its file')
    with pytest.raises(ValueError):
        loop(0.5).load_parts(RS.load_run(path))


# ---- (6) the entry points refuse before any launch ------------------------------------------------------------------------------

@pytest.mark.parametrize('cid', ['reach-window-J1', 'reach-lstm_window-J2', 'arm-ddpg-J5'])
def test_entry_points_refuse_a_bad_stream_and_leave_everything_as_it_was(cid):
    """past the Python checks (switched off here) the C entry points refuse, before any launch: nothing moves"""
    c = TD.BY_ID[cid]
    for breakage in ('scale', 'nan', 'episode'):
        x = TD.setup(c, DEV)
        x.venv._disturbed_ok = lambda who: None
        if breakage == 'episode':
            x.resets.episode = 0
        else:
            x.resets.disturbance = 1.5 if breakage == 'scale' else float('nan')
        state = x.venv.state.clone()
        with pytest.raises(L.SmxError):
            TD.run(x, 0, calls=(3,))
        torch.cuda.synchronize()
        assert torch.equal(x.venv.state, state)
    venv = TD.per_step_chains(DEV, task='reach', J=2, n=6)
    venv._disturbed_ok = lambda who: None
    venv.resets.episode = 0
    state = venv.state.clone()
    with pytest.raises(L.SmxError):
        venv.step(torch.zeros(6, 2, device=DEV))
    assert torch.equal(venv.state, state)
    assert TK.DISTURB_TAG == 0x44530000
