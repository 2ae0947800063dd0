"""GPU tier (-m gpu): the five one-launch rollout kernels of csrc/smx_rollout.hip at the edges of their shape envelope,
against the float64 restatement of rollout_fp64_ref.py -- a reference outside the library's arithmetic.  The cases
(rollout_envelope_cases.py) reach the generic output layer of the PPO-family kernels (H2 > 256) and a second column pass
of the 4-row layers, every lane slot and wave part of the environment lanes (D up to 512), both output tiles and all 512
head lanes (A up to 32), 1 to 128 LSTM units, DDPG n_step 1 and n_step > episode_len, and each family's largest LDS
layout as the library's queries report it, bare and with the episode monitor and the noise stream attached; each at 4, 8
and 16 actors per workgroup and the automatic choice, 37 actors (3 at the corners too).

Bound: rtol = atol = 1e-5, the project's parity cap, for every float field; rows written, dones and the rows never
written exact.  Block sizes: the 4-row-loop families (LSTM, windows, DDPG) leave the same bits at every size, the plain
PPO rollout at 4 and 8 (rollout16_kernel sums in another order: held to the reference only).

Largest error over the case list in units of the bound (|got - want| / (1e-5 + 1e-5 |want|)), measured on an MI355X
(`pytest -s` prints the table again, per family and field; every case passed, so no weight was rescaled for the kernels'
sake and no kernel defect was found):
    ppo           0.05  actions, 512 -> 640 -> 640 -> 32 at 16 actors per workgroup (pds 0.05, obs 0.05, rewards 0.01)
    lstm          0.62  cells, D = 511 (cN 0.47, hN 0.20, pds 0.06, obs 0.05, actions 0.04)
    window        0.04  obs / obs_next at the corner (actions, pds 0.02)
    lstm_window   0.50  cells, D = 511 (cN 0.47, hN 0.20, obs_next 0.06)
    ddpg          0.15  obs_next at the corner (actions 0.14, obs 0.09, rewards 0.02)
    ddpg_ln       0.74  obs_next, the corner at 3 actors with sigmas up to 2 (obs 0.59, actions 0.39, rewards 0.08)
    ddpg_pop      0.23  obs_next (actions 0.18, obs 0.11; the action distance 0.003 of its bound)
    episode returns of the attached monitor: 0.02 at most; the per-step paths just outside the envelope: 0.23 at most
"""
import numpy as np
import pytest
import torch

import rollout_envelope_cases as EC
from surreal_amd import _lib as L

pytestmark = pytest.mark.gpu

MAXIMA = {}                       # (family, field) -> (the largest error / bound, the case and block it came from)
BIT_EQUAL = {'ppo': (4, 8)}       # every other family: all of 4, 8, 16


def blocks_of(c, x):
    if c.family != 'ddpg_pop':
        return EC.BLOCKS
    K = x.venv.K                  # a population: the block sizes the launch takes for 4-actor agents
    return tuple(b for b in EC.BLOCKS if b == 0 or K.synth_ddpg_population_block(c.n, 4, b) == b)


def note(c, apw, errs):
    for k, v in errs.items():
        if v > MAXIMA.get((c.family, k), (-1.0,))[0]:
            MAXIMA[(c.family, k)] = (v, '%s block %d' % (c.id, apw))


def monitor_against(x, env):
    """the attached monitor's finished episodes against the reference's: counts and lengths exact, an episode's reward
    sum (fp64 of the launch's fp32 rewards) within the bound of its terms: 1e-5 (steps + sum |reward|)"""
    c = x.c
    polled = x.venv.monitor.poll()
    assert len(polled) == c.n * len(env.finished)
    per_actor = {}
    for a, reward, steps in polled:
        per_actor.setdefault(a, []).append((reward, steps))
    worst = 0.0
    for a in range(c.n):
        for (reward, steps), (want, mag, length) in zip(per_actor[a], env.finished):
            assert steps == length
            worst = max(worst, abs(reward - float(want[a])) / (EC.TOL * (length + float(mag[a]))))
    return worst


@pytest.mark.parametrize('c', EC.CASES, ids=[c.id for c in EC.CASES])
def test_kernel_meets_the_float64_restatement(c):
    want = first = None
    same = BIT_EQUAL.get(c.family, (4, 8, 16))
    bits = {}
    for apw in blocks_of(c, EC.setup(c, 'cuda')):
        x = EC.setup(c, 'cuda')
        if want is None:
            want, wrows, written, pol = EC.reference_fields(x)
        got, rows = EC.device_fields(x, apw)
        assert rows == wrows, apw
        errs = EC.worst_errors(got, want, written)
        if c.streams:
            errs['episode returns'] = monitor_against(x, pol.env)
        if x.pn is not None:
            # the action distance of each agent's first actor at the last measuring step: two outputs of A components
            # within the bound each, so 2 sqrt(A) of it (test_gpu_param_noise.py's rule)
            dist, wd = x.pn.dist.cpu(), pol.dist
            assert float(wd.min()) > 1e-4
            errs['distance'] = float(((dist - wd).abs() / (2 * np.sqrt(c.A) * EC.TOL * (1 + wd.abs()))).max())
        print('%s block %d: error / bound %s' % (c.id, apw, {k: round(v, 3) for k, v in errs.items()}))
        note(c, apw, errs)
        assert max(errs.values()) <= 1.0, (apw, errs)
        bits[apw] = got
    for apw in same[1:]:
        if apw in bits and same[0] in bits:
            EC.same_bits(bits[apw], bits[same[0]])
    if c.family == 'ppo':          # the automatic choice is one of the forced ones
        assert any(all(torch.equal(bits[0][k], bits[b][k]) for k in bits[0]) for b in (4, 8, 16))
    elif 4 in bits:
        EC.same_bits(bits[0], bits[4])


OUTSIDE = EC.outside_cases()


def refused_launch(x):
    """the entry point itself, the facade's own shape check bypassed"""
    c, K = x.c, x.venv.K
    if c.family in ('ppo', 'lstm'):
        return EC.run_table(c, x.agent, x.venv, x.eps, 0)
    name = 'synth_ppo_window_rollout_supported' if c.family in ('window', 'lstm_window') else 'synth_ddpg_rollout_supported'
    setattr(K, name, lambda *a, **k: True)
    try:
        return EC.device_fields(x)
    finally:
        delattr(K, name)


@pytest.mark.parametrize('c', OUTSIDE, ids=[c.id for c in OUTSIDE])
def test_outside_the_envelope_the_entry_refuses_and_the_callers_fall_back(c):
    with pytest.raises(L.SmxError, match='rc=%d' % L.SMX_E_UNSUPPORTED):
        refused_launch(EC.setup(c, 'cuda'))
    x = EC.setup(c, 'cuda')
    if c.family in ('window', 'lstm_window'):
        assert not x.venv.can_ppo_rollout_into(x.agent)
        with pytest.raises(ValueError, match='policy shapes the persistent kernel refuses'):
            x.venv.ppo_rollout_into(x.agent, x.replay, c.calls[0], eps=x.eps[:c.calls[0]])
        return
    want, wrows, written, pol = EC.reference_fields(x)
    got, rows = EC.public_table(x) if c.family in ('ppo', 'lstm') else EC.device_fields(x)
    assert rows == wrows
    errs = EC.worst_errors(got, want, written)
    print('%s, the per-step path: error / bound %s' % (c.id, {k: round(v, 3) for k, v in errs.items()}))
    note(c._replace(family=c.family + ' (per-step path)'), 0, errs)
    assert max(errs.values()) <= 1.0, errs


def test_zz_largest_errors_per_family_and_field():
    """prints what the module's header and DESIGN.md section 3.6 record (-s); the assertions are the tests' above"""
    for (family, field), (v, where) in sorted(MAXIMA.items()):
        print('%-28s %-16s %.3f of the bound  (%s)' % (family, field, v, where))
        assert v <= 1.0
