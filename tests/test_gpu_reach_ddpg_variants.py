"""GPU tier (-m gpu): the actor variants of the one-launch DDPG rollout on the `reach` task --
ddpg_rollout_kernel<RG, NT, POP, LN, false, SMX_TASK_REACH> for (POP, LN) = (1, 0), (0, 1), (1, 1) at 4, 8 and 16 actors per
workgroup, through smx_synth_ddpg_rollout_variant_task_f32.  Shapes (reach_ddpg_variants_cases.py): (D, A) = (3, 1), (6, 2),
(63, 21) at hidden 8 / 4, one LayerNorm actor at hidden 76 / 132 (the partial second column pass of ln_rows); 5 actors (a
partial 4-actor block), 20, and populations of 32 at 4, 8 and 16 actors per agent; episodes of 5 steps over calls of 4, 5
and 3 steps with n_step 3, so two episode ends fall inside; rings that wrap; LayerNorm gains and biases from set_layernorm;
some cases with the reset stream, the noise stream and the episode monitor attached.

  1. env bits: the host reach_step applied to a recorded observation and action gives the recorded next observation bit
     for bit, the n-step rewards as test_gpu_reach.py forms them -- whatever the actor in front;
  2. 4, 8 and 16 actors per workgroup (where the block divides the agent) and the automatic choice leave the same bytes;
  3. a population without LayerNorm: every agent's actors hold the bytes the plain `reach` launch leaves on those actors
     alone from an agent whose model holds that agent's perturbed copy -- same streams, same actor_base;
  4. every variant against the float64 restatement (ReachEnv / DrawnReachEnv + DdpgPolicy) at the project's 1e-5, under
     input conditions the restatement alone meets; rows written, dones and never-written rows exact;
  5. the measuring step on an episode's last step and mid-episode: dist the same bits at every block size, within
     test_gpu_param_noise.py's bound of the restatement's, nothing written around it;
  6. with the streams attached two envs of 16 actors leave per actor the bytes of one env of 32;
  7. the entry point with SMX_TASK_DRIFT leaves the bytes of smx_synth_ddpg_rollout_f32 for each variant, with a NULL or
     all-zero variant on `reach` those of smx_synth_ddpg_rollout_task_f32 / _resets_f32.

With SMX_REACH_VARIANTS_ERRORS_OUT set to a path the run writes every case's worst observed error / bound there
(profiles/reach_ddpg_variants_errors.txt is such a run on an MI355X; `pytest -s` prints the figures per block size).

Measured on an MI355X: the largest error against the restatement is 0.30 of the bound (actions, popln8-63-21-n32; every
other field of every case at most 0.074), episode returns 0.012 of theirs, a measured distance 0.061 of its bound;
everything else in this file is an equality of bits.  52 tests, 3.3 s."""
import os

import numpy as np
import pytest
import torch

import ddpg_ln_rollout_cases as LN
import ddpg_rollout_cases as DC
import reach_cases as RC
import reach_ddpg_variants_cases as V
import reach_resets_cases as RRC
import rollout_envelope_cases as EC
from reach_cpu_kernels import np_nstep_sum
from surreal_amd import _lib as L
from surreal_amd.env import tasks as TK

pytestmark = pytest.mark.gpu

CASES = [V.tuned(c) for c in V.CASES]
IDS = [c.id for c in CASES]
POPS = [c for c in CASES if c.apa]
_RUNS = {}


def blocks(c):
    """the forced block sizes a case takes (a block never spans two agents), then the automatic choice"""
    return tuple(b for b in (4, 8, 16) if not c.apa or c.apa % b == 0) + (0,)


def wrapped_run(c, apw):
    """the case on a ring that wraps, at a forced block size (run once per module) -> every byte it left"""
    if (c.id, apw) not in _RUNS:
        x = V.make(c, 'cuda', wrap=True)
        assert V.run(x, apw) == x.rows > x.capacity
        _RUNS[(c.id, apw)] = V.everything(x)
    return _RUNS[(c.id, apw)]


def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope='module')
def errors():
    rec = {}
    yield rec
    path = os.environ.get('SMX_REACH_VARIANTS_ERRORS_OUT')
    if not path or not rec:
        return
    with open(path, 'w') as f:
        f.write('# worst observed error / bound per case over its block sizes (<= 1 passes): the fields of the float64\n'
                '# restatement at rtol = atol = 1e-5, episode returns at the bound of their terms, dist at 2e-6 * 2 sqrt(A)\n')
        for cid in sorted(rec):
            f.write('%s %s\n' % (cid, ' '.join('%s=%.4f' % kv for kv in sorted(rec[cid].items()))))


# ---- 1. env bits -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_rows_hold_the_host_step_bit_for_bit(c):
    """test_gpu_reach.py's chain: rows of one episode follow from each other by reach_step; where the rows j, j + 1, j + 2
    are all recorded, obs_next and the n-step sum follow from recorded values alone"""
    n, N = c.n, V.N_STEP
    x = V.make(c, 'cuda')
    assert V.run(x, 4) == x.rows
    got = V.ring(x)
    f = {k: got[k].numpy() for k in DC.FIELDS}
    t, closings = 0, []
    for _ in range(sum(V.CALLS)):
        if t >= N - 1:
            closings.append((t - N + 1, t))
        t = 0 if t + 1 >= V.EP else t + 1
    gpow = np.array([pow(V.GAMMA, e) for e in range(N)])
    row = lambda k: slice(k * n, (k + 1) * n)  # noqa: E731
    chained = summed = 0
    for k, (j, tau) in enumerate(closings):
        sn, r = TK.reach_step(f['obs'][row(k)], f['actions'][row(k)])
        assert np.abs(f['actions'][row(k)]).max() <= 1.0
        if k + 1 < len(closings) and closings[k + 1][0] == j + 1:
            assert bits(sn, f['obs'][row(k + 1)]), k
            chained += 1
        if k + N - 1 < len(closings) and closings[k + N - 1][0] == j + N - 1:
            rews, s_last = [], None
            for u in range(N):
                s_last, ru = TK.reach_step(f['obs'][row(k + u)], f['actions'][row(k + u)])
                rews.append(ru)
            assert bits(s_last, f['obs_next'][row(k)]), k
            full = np.zeros((n, tau + 1), np.float32)
            full[:, j:] = np.stack(rews, 1)
            assert bits(np_nstep_sum(full, gpow, N, tau), f['rewards'][row(k)].reshape(-1)), k
            summed += 1
        assert float(f['dones'][row(k)].min()) == float(f['dones'][row(k)].max()) == float(tau + 1 >= V.EP)
    assert chained >= 4 and summed >= 2
    # an episode's first row is where the episode begins: the drawn row, or the reset state
    first = RRC.rows_of(n, c.A)[:2] if c.streams else np.stack([x.venv.init_state.cpu().numpy()] * 2)
    assert bits(f['obs'][row(0)], first[0]) and bits(f['obs'][row(3)], first[1])


# ---- 2. block sizes ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_block_sizes_leave_the_same_bytes(c):
    first = None
    for apw in blocks(c):
        got = wrapped_run(c, apw)
        first = first or got
        assert set(got) == set(first)
        EC.same_bits(got, first)
    assert len(blocks(c)) >= 2


# ---- 3. a population without LayerNorm against the plain launch ------------------------------------------------------------

@pytest.mark.parametrize('c', [c for c in POPS if not c.ln], ids=[c.id for c in POPS if not c.ln])
def test_population_leaves_the_bytes_of_plain_launches_on_each_agents_copy(c):
    x = V.make(c, 'cuda')
    got = LN.final(x.venv, x.replay, V.run(x))
    pop = V.population(x)
    assert x.pn.agents == c.n // c.apa == len(pop)
    for p in range(x.pn.agents):
        lo = p * c.apa
        y = V.make(c, 'cuda', n=c.apa, actor_base=lo, attach=False, params=pop[p])
        assert y.pn is None and y.venv.param_noise is None
        want = LN.final(y.venv, y.replay, V.run(y))
        LN.same_bytes(got, want, lo, lo + c.apa)
    # and the perturbed copies differ from each other and from the clean actor
    assert not torch.equal(pop[0]['W1'], pop[1]['W1']) and not torch.equal(pop[0]['W1'], V.clean_params(x)['W1'])


# ---- 4. the float64 restatement ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_one_launch_meets_the_float64_restatement(c, errors):
    """rtol = atol = 1e-5 on every float field, rows written, dones and the rows never written exact; a population's
    last measured distances within 2e-6 * 2 sqrt(A) of the restatement's"""
    want, worst = None, {}
    for apw in blocks(c):
        x = V.make(c, 'cuda')
        if want is None:
            want, wrows, written, pol = V.restatement(x)
            print(c.id, 'input conditions', RC.input_conditions(pol, V.margin_of(c)))
        assert V.run(x, apw) == wrows
        errs = EC.worst_errors(V.ring(x), want, written)
        if c.streams:
            # the monitor's finished episodes against the restatement's: an episode's sum within the bound of its terms
            per_actor = {}
            for a, reward, steps in x.venv.monitor.poll():
                per_actor.setdefault(a, []).append((reward, steps))
            w = 0.0
            for a in range(c.n):
                assert len(per_actor[a]) == len(pol.env.finished) == 2
                for (reward, steps), (ret, mag, length) in zip(per_actor[a], pol.env.finished):
                    assert steps == length
                    w = max(w, abs(reward - float(ret[a])) / (EC.TOL * (length + float(mag[a])) + 1e-6))
            errs['episode returns'] = w
            assert x.venv.resets.episode == RRC.EPISODES == pol.env.begun
        if c.apa:
            dist = x.pn.dist.cpu()
            assert (pol.dist > 1e-4).all() and x.pn.acts == sum(V.CALLS)
            errs['dist'] = float((dist - pol.dist).abs().max()) / V.DIST_ATOL(c.A)
        print('%s block %d: error / bound %s' % (c.id, apw, {k: round(v, 3) for k, v in errs.items()}))
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert max(errs.values()) <= 1.0, (apw, errs)
    errors[c.id] = worst


# ---- 5. the measuring step ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('interval, step', [(4, 4), (3, 3)], ids=['last-step-of-the-episode', 'mid-episode'])
@pytest.mark.parametrize('c', POPS, ids=[c.id for c in POPS])
def test_measuring_step(c, interval, step):
    """one call of 5 steps from clock 0, the measuring step placed by compute_dist_interval: at clock 4 the step also ends
    the episode (the reset draw follows it), at clock 3 it does not.  dist lies inside a fenced buffer; a following call
    that measures nothing leaves it alone"""
    FENCE = -7.0
    first = want = None
    for apw in blocks(c):
        x = V.make(c, 'cuda', calls=(5,))
        pn = x.pn
        pn.compute_dist_interval = interval
        assert pn.measure_step(5) == step
        big = torch.full((pn.agents + 4,), FENCE, dtype=torch.float64, device='cuda')
        pn.dist = big[2:2 + pn.agents]
        pn.dist.fill_(-1.0)
        if want is None:
            pol = V.restatement(x, measure_at=(step,))[3]
            RC.input_conditions(pol, V.margin_of(c))
            want = pol.dist
        V.run(x, apw)
        torch.cuda.synchronize()
        dist = pn.dist.cpu()
        assert (big[:2] == FENCE).all() and (big[-2:] == FENCE).all()
        worst = float((dist - want).abs().max())
        print('%s block %d step %d: dist %s, |difference| %.3g (atol %.3g)' % (c.id, apw, step, dist.tolist()[:2], worst,
                                                                               V.DIST_ATOL(c.A)))
        assert (want > 1e-4).all() and worst <= V.DIST_ATOL(c.A)
        first = dist if first is None else first
        assert torch.equal(dist.view(torch.int64), first.view(torch.int64)), apw
        # act 5 of the population: no multiple of the interval, nothing measured
        assert pn.acts == 5 and pn.measure_step(1) == -1
        eps = None if x.eps is None else x.eps[5:6]
        x.venv.ddpg_rollout_into(x.agent, x.replay, 1, eps=eps, sigmas=x.sig, actors_per_workgroup=apw)
        torch.cuda.synchronize()
        assert torch.equal(pn.dist.cpu().view(torch.int64), dist.view(torch.int64)) and (big[:2] == FENCE).all() \
            and (big[-2:] == FENCE).all()


# ---- 6. the streams: two envs of 16 against one of 32 ----------------------------------------------------------------------

@pytest.mark.parametrize('c', [c for c in POPS if c.streams], ids=[c.id for c in POPS if c.streams])
def test_two_envs_of_16_leave_the_bytes_of_one_env_of_32(c):
    x = V.make(c, 'cuda')
    assert x.venv.noise is not None and x.venv.resets is not None and x.venv.monitor is not None
    got = LN.final(x.venv, x.replay, V.run(x))
    dist = x.pn.dist.cpu()
    for lo in (0, 16):
        y = V.make(c, 'cuda', n=16, actor_base=lo)
        assert y.pn.agent_base == lo // c.apa and y.venv.resets.actor_base == lo == y.venv.noise.actor_base
        want = LN.final(y.venv, y.replay, V.run(y))
        LN.same_bytes(got, want, lo, lo + 16)
        mine = dist[lo // c.apa:(lo + 16) // c.apa]
        assert torch.equal(y.pn.dist.cpu().view(torch.int64), mine.view(torch.int64))


# ---- 7. the entry point forwards ---------------------------------------------------------------------------------------------

def test_drift_through_the_variant_task_entry_point_leaves_the_same_bytes(monkeypatch):
    """SMX_TASK_DRIFT forwards: a drift env of each variant (and the plain actor) run through the new entry point against
    the same run through smx_synth_ddpg_rollout_f32, which the facade calls for 'drift'"""
    seen = []

    def through(redirect):
        orig = L.call

        def call(name, *args):
            if redirect and name == 'smx_synth_ddpg_rollout_f32':
                seen.append(name)
                return orig('smx_synth_ddpg_rollout_variant_task_f32', args[0], args[1], L.SMX_TASK_DRIFT, None, args[2])
            return orig(name, *args)
        out = {}
        with monkeypatch.context() as m:
            m.setattr(L, 'call', call)
            for c in (CASES[1], CASES[5], CASES[8]):
                x = V.make(c, 'cuda', task='drift')
                V.run(x, 4)
                out[c.id] = V.everything(x)
            x = V.make(CASES[5], 'cuda', task='drift', attach=False)
            V.run(x, 8)
            out['plain'] = V.everything(x)
        return out
    a, b = through(False), through(True)
    assert len(seen) == 4 * len(V.CALLS)
    for k in a:
        assert set(a[k]) == set(b[k])
        EC.same_bits(a[k], b[k])


@pytest.mark.parametrize('zeroed', [False, True], ids=['null-variant', 'all-zero-variant'])
def test_plain_actor_through_the_variant_task_entry_point_leaves_the_same_bytes(monkeypatch, zeroed):
    """a NULL (or all-zero) variant on `reach` is the plain actor: the bytes of smx_synth_ddpg_rollout_task_f32 and, with a
    stream, of smx_synth_ddpg_rollout_resets_f32"""
    seen = []

    def through(redirect):
        orig = L.call

        def call(name, *args):
            v = L.DdpgActorVariant() if zeroed else None
            if redirect and name == 'smx_synth_ddpg_rollout_task_f32':
                seen.append(name)
                return orig('smx_synth_ddpg_rollout_variant_task_f32', args[0], v, args[1], None, args[2])
            if redirect and name == 'smx_synth_ddpg_rollout_resets_f32':
                seen.append(name)
                return orig('smx_synth_ddpg_rollout_variant_task_f32', args[0], v, args[1], args[2], args[3])
            return orig(name, *args)
        out = {}
        with monkeypatch.context() as m:
            m.setattr(L, 'call', call)
            for c in (RC.CASES[5], RC.CASES[7]):
                c = RRC.tuned(c)
                out[c.id] = RC.run(RC.setup(c, 'cuda'), 4)[0]
                out[c.id + '+resets'] = RRC.run(RRC.setup(c, 'cuda'), 4)[0]
        return out
    a, b = through(False), through(True)
    assert sorted(set(seen)) == ['smx_synth_ddpg_rollout_resets_f32', 'smx_synth_ddpg_rollout_task_f32']
    for k in a:
        EC.same_bits(a[k], b[k])
