"""GPU tier (-m gpu): a LayerNorm actor on the one-launch DDPG rollout (smx_synth_ddpg_rollout_f32 with the `ln` of a
struct smx_ddpg_actor_variant) and under a device parameter noise (smx_param_noise_*_f32 with `ln`, the variant's packed_pop).

Actor shapes (ddpg_ln_rollout_cases): 5 -> 12 -> 8 -> 3, 17 -> 76 -> 132 -> 6, 17 -> 300 -> 200 -> 6, 17 -> 640 -> 640 -> 6;
37 actors (a partial last block at 4, 8 and 16), episodes of 11 against calls of 9 + 13 + 6, n_step 3; the default shape
also at 260 actors.  Every actor has random LayerNorm gains and biases."""
import copy

import numpy as np
import pytest
import torch

import ddpg_ln_rollout_cases as LC
import ddpg_rollout_cases as DC
import helpers as H
import param_noise_ref as PR

pytestmark = pytest.mark.gpu

N, STEPS = 37, sum(LC.CALLS)
# The one-launch rollout against the per-step path (DDPGModel.forward_actor + smx_synth_ddpg_step_f32), which this change
# leaves as it was: the two form the layer sums in different orders (the 4-row MFMA loop against smx_linear_f32), the
# LayerNorm in the same one.  Largest |difference| of a float field over the four shapes at 37 actors, the default shape
# at 260 and the noise modes normal / ou_noise / deterministic, measured on an MI355X: 9.3e-6 (5 -> 12 -> 8 -> 3,
# ou_noise; 17 -> 640 -> 640 -> 6 deterministic 8.6e-6; the default shape 4.2e-6 at most).  Times 4 for other seeds that is
# 4e-5, above the project's parity bar of 1e-5, which is the hard cap: the constant is the cap, not the derived figure,
# and DESIGN.md section 3.6 says what was found behind the 9.3e-6 (a LayerNorm over 8 or 12 features multiplies the
# rounding of its input by rstd, up to 1 / sqrt(eps) = 316).
STEP_ATOL = 1e-5
DIST_ATOL = STEP_ATOL * 2 * np.sqrt(3)        # a distance of two such outputs of A = 3 components (test_gpu_param_noise.py)
SIG = torch.linspace(0.05, 0.8, 16, dtype=torch.float64)        # the population tests' exploration scales, by actor id


def eps_for(n, A, steps=STEPS):
    return torch.randn(steps, n, A, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))


def rollout(n, shape, noise, calls=LC.CALLS, capacity=None, streams=False, b1=None, **kw):
    made = LC.make(n, shape, noise, capacity=capacity or n * LC.closing(sum(calls)) + 64, streams=streams)
    agent, venv, replay = made[:3]
    if b1 is not None:
        agent.model.actor.views['b1'].fill_(b1)
    eps = None if streams or noise == 'deterministic' else eps_for(n, shape[3], sum(calls))
    rows = LC.run(agent, venv, replay, calls, eps=eps, **kw)
    assert rows == n * LC.closing(sum(calls)) == len(replay)
    return LC.final(venv, replay, rows)


# ---- 1. block sizes, 2. call splits ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', LC.SHAPES)
def test_block_sizes_and_call_splits_leave_the_same_bytes(shape):
    first = rollout(N, shape, 'ou_noise', actors_per_workgroup=0)
    assert first['ring_obs'].shape == (N, LC.closing(STEPS), shape[0]) and float(first['ou'].abs().sum()) > 0
    for apw in (4, 8, 16):
        LC.same_bytes(rollout(N, shape, 'ou_noise', actors_per_workgroup=apw), first)
    LC.same_bytes(rollout(N, shape, 'ou_noise', calls=(STEPS,)), first)


def test_many_workgroups_leave_the_same_bytes_at_every_block_size():
    first = rollout(260, LC.DEFAULT, 'normal', actors_per_workgroup=4)
    for apw in (0, 8, 16):
        LC.same_bytes(rollout(260, LC.DEFAULT, 'normal', actors_per_workgroup=apw), first)


# ---- 3. against the per-step path ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('noise', ['normal', 'ou_noise', 'deterministic'])
@pytest.mark.parametrize('n,shape', [(N, s) for s in LC.SHAPES] + [(260, LC.DEFAULT)])
def test_one_launch_matches_the_per_step_path(n, shape, noise):
    want = rollout(n, shape, noise, reference=True)
    got = rollout(n, shape, noise)
    d = LC.max_float_difference(got, want)
    print('one launch against per step, %d actors, %s, %s: max |difference| %.3g (atol %.1g)'
          % (n, 'x'.join(map(str, shape)), noise, d, STEP_ATOL))
    assert d <= STEP_ATOL
    assert np.abs(got['ring_actions'].numpy()).max() > 0.05          # the actors do act


# ---- 4. against the host path ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [LC.TINY, LC.DEFAULT])
def test_one_launch_matches_the_host_path(shape):
    n, ep, calls, capacity = 3, 8, (5, 6), 40
    agent, venv, replay, _, cfg = LC.make(n, shape, 'ou_noise', capacity=capacity, episode_len=ep)
    eps_all = np.random.RandomState(3).randn(sum(calls), n, shape[3]).astype(np.float32)
    rows = LC.run(agent, venv, replay, calls, eps=torch.as_tensor(eps_all).cuda())
    torch.cuda.synchronize()
    want, total = DC.host_ring(agent, *cfg, n, ep, eps_all, capacity)
    assert rows == total > 0
    ring = H.device_ring(replay, DC.FIELDS)
    for k in DC.FIELDS:
        np.testing.assert_allclose(ring[k].reshape(want[k].shape), want[k], atol=1e-5, rtol=0, err_msg=k)
    assert np.array_equal(ring['dones'].reshape(want['dones'].shape), want['dones'])


# ---- 5. a dead first layer -------------------------------------------------------------------------------------------------

def test_dead_first_layer_normalises_zero_rows_to_the_bias():
    """b1 = -100: every first-layer ReLU row is zero, rs = 1 / sqrt(eps) and LN1's output its bias"""
    want = rollout(N, LC.ODD, 'ou_noise', b1=-100.0, reference=True)
    for apw in (4, 16):
        got = rollout(N, LC.ODD, 'ou_noise', b1=-100.0, actors_per_workgroup=apw)
        d = LC.max_float_difference(got, want)
        print('dead first layer, block %d: max |difference| %.3g (atol %.1g)' % (apw, d, STEP_ATOL))
        assert d <= STEP_ATOL


# ---- 6. with the stream and the monitor attached ---------------------------------------------------------------------------

def test_block_sizes_with_the_stream_and_the_monitor_attached():
    first = rollout(N, LC.ODD, 'ou_noise', streams=True, actors_per_workgroup=0)
    assert any(k.startswith('mon_') for k in first)
    for apw in (4, 8, 16):
        LC.same_bytes(rollout(N, LC.ODD, 'ou_noise', streams=True, actors_per_workgroup=apw), first)
    LC.same_bytes(rollout(N, LC.ODD, 'ou_noise', streams=True, calls=(STEPS,)), first)


# ---- 7. the population ------------------------------------------------------------------------------------------------------

T, EP, CLOSING = 7, 5, 3                      # clocks 0 1 2 3 4 0 1 of a call of 7: three of them >= n_step - 1


def population(n, ptype, noise='normal', apa=4, agent_base=0, actor_base=0, attach=True, params=None):
    return LC.make(n, LC.TINY, noise, ptype=ptype if attach else None, apa=apa, agent_base=agent_base,
                   actor_base=actor_base, attach=attach, params=params, episode_len=EP, streams=True)[:4]


def pop_run(agent, venv, replay, calls, actor_base=0, **kw):
    sig = SIG[actor_base:actor_base + venv.n].cuda()
    return LC.final(venv, replay, LC.run(agent, venv, replay, calls, sigmas=sig, **kw))


def per_agent_reference(pn, p, apa, calls, noise, agent_base=0):
    """the LayerNorm launch without a population on agent p's actors alone, from an agent whose model holds perturbed(p)"""
    lo = (agent_base + p) * apa
    agent, venv, replay, _ = population(apa, None, noise, actor_base=lo, attach=False, params=pn.perturbed(p))
    return pop_run(agent, venv, replay, calls, actor_base=lo)


@pytest.mark.parametrize('ptype', ['normal', 'adaptive_normal'])
def test_population_launch_leaves_the_bytes_of_per_agent_launches(ptype):
    agent, venv, replay, pn = population(16, ptype)
    assert pn.ln and set(pn.perturbed(0)) == set(LC.ORDER)
    one = pop_run(agent, venv, replay, (T,))
    assert one['ring_obs'].shape == (16, CLOSING, 5) and pn.acts == T
    for p in range(4):
        LC.same_bytes(one, per_agent_reference(pn, p, 4, (T,), 'normal'), 4 * p, 4 * p + 4)
    agent, venv, replay, _ = population(16, ptype)
    LC.same_bytes(one, pop_run(agent, venv, replay, (3, 4)))
    assert not torch.equal(one['ring_actions'][0:4], one['ring_actions'][4:8])


def test_agents_of_eight_actors_and_two_envs_of_two_agents():
    outs = []
    for apw in (4, 8):
        agent, venv, replay, pn = population(16, 'normal', 'ou_noise', apa=8)
        assert pn.agents == 2
        outs.append(pop_run(agent, venv, replay, (T,), actors_per_workgroup=apw))
    LC.same_bytes(outs[0], outs[1])
    for p in range(2):
        LC.same_bytes(outs[0], per_agent_reference(pn, p, 8, (T,), 'ou_noise'), 8 * p, 8 * p + 8)
    agent, venv, replay, _ = population(16, 'adaptive_normal')
    whole = pop_run(agent, venv, replay, (T,))
    for half in range(2):
        agent, venv, replay, _ = population(8, 'adaptive_normal', agent_base=2 * half, actor_base=8 * half)
        LC.same_bytes(whole, pop_run(agent, venv, replay, (T,), actor_base=8 * half), 8 * half, 8 * half + 8)


# ---- 8. the packed copies ---------------------------------------------------------------------------------------------------

def test_packed_copies_carry_the_perturbed_layernorm_parameters_with_zero_pads():
    agent, venv, _, pn = population(16, 'adaptive_normal')
    K, actor = venv.K, agent.model.actor
    numel = K.epoch_packed_numel(actor)
    assert pn.pop.shape[1] == K.param_noise_copy_numel(actor, ln=True) and pn.pop.shape[1] % 64 == 0
    twin = copy.deepcopy(agent.model)
    for p in range(pn.agents):
        pert = pn.perturbed(p)
        for k in PR.ORDER:
            twin.actor.views[k].copy_(pert[k])
        want = torch.zeros(numel, device='cuda')
        K.epoch_pack([(twin.actor, want)])
        got = pn.pop[p]
        assert torch.equal(got[:numel].view(torch.int32), want.view(torch.int32)), p
        tail = torch.cat([pert[k] for k in ('b1', 'b2', 'b3') + LC.LN_KEYS])
        assert tail.numel() == 12 + 8 + 3 + 2 * (12 + 8)
        assert torch.equal(got[numel:numel + tail.numel()].view(torch.int32), tail.view(torch.int32))
        assert not got[numel + tail.numel():].view(torch.int32).any()
        for k in LC.LN_KEYS:                               # perturbed, not the clean ones
            assert not torch.equal(pert[k], agent.model.actor_ln[k])
    # the fill against the restatement over the ten blocks
    clean = np.concatenate([v.reshape(-1) for v in LC.actor_params(agent).values()])
    for p in range(pn.agents):
        got = torch.cat([v.reshape(-1) for v in pn.perturbed(p).values()]).cpu().numpy()
        want = PR.perturbed_flat(clean, agent.param_noise_sigma, LC.PSEED, p, 0)
        assert np.abs(got.astype(np.float64) - want).max() <= 4e-7


# ---- 9. the distance and the adaptation ---------------------------------------------------------------------------------------

def test_distance_of_the_layernorm_actors_and_the_adaptation():
    agent, venv, replay, pn = population(16, 'adaptive_normal')
    pn.compute_dist_interval = 3
    pn.dist.fill_(-1.0)
    assert pn.measure_step(T) == 6
    pop_run(agent, venv, replay, (T,))
    dist = pn.dist.cpu().numpy()
    twin = population(16, 'adaptive_normal')                   # the observations before step 6
    pop_run(twin[0], twin[1], twin[2], (6,))
    obs = twin[1].state.cpu().numpy()
    clean = LC.actor_params(agent)
    for p in range(4):
        noisy = {k: v.cpu().numpy() for k, v in pn.perturbed(p).items()}
        want = LC.action_distance(clean, noisy, obs[4 * p], agent.model.ln_eps)
        print('agent %d: dist %.9g, float64 restatement %.9g, |difference| %.3g (atol %.3g)'
              % (p, dist[p], want, abs(dist[p] - want), DIST_ATOL))
        assert want > 1e-4 and abs(dist[p] - want) <= DIST_ATOL
    # clocks 7 and 8: no multiple of 3, nothing measured, dist untouched
    assert pn.acts == 7 and pn.measure_step(2) == -1
    venv.ddpg_rollout_into(agent, replay, 2, sigmas=SIG.cuda())
    torch.cuda.synchronize()
    assert np.array_equal(pn.dist.cpu().numpy(), dist) and pn.acts == 9
    # refresh() moves sigma by the Python rule
    per_act = sorted(float(d) / 9 for d in dist)
    pn.target = 0.5 * (per_act[1] + per_act[2])
    sigma0, gen = [float(v) for v in pn.sigma.cpu()], pn.generation
    pn.refresh()
    want = [PR.adapt(s, d, 9, pn.target, pn.alpha) for s, d in zip(sigma0, dist)]
    assert [float(v) for v in pn.sigma.cpu()] == want and len({w > s for w, s in zip(want, sigma0)}) == 2
    assert pn.acts == 0 and pn.generation == gen + 1


# ---- the one entry point: no variant and an empty one -------------------------------------------------------------------

def test_no_variant_and_an_empty_variant_leave_the_same_bytes():
    """smx_synth_ddpg_rollout_f32 with variant = NULL against a variant whose pointers are both NULL (what the facade
    passes for a plain actor): the plain launch either way.  5 -> 12 -> 8 -> 3, 8 actors, one call of 9 steps"""
    import ctypes
    from surreal_amd import _lib as L

    def null_variant(K):
        def launch(net, packed, r, steps, actors_per_workgroup=0, monitor=None, noise=None):
            p = K._ddpg_args(r, steps, net, packed, actors_per_workgroup, monitor, noise)
            L.call('smx_synth_ddpg_rollout_f32', ctypes.byref(p), None, K._st())
            calls.append(steps)
        return launch
    outs, calls = [], []
    for null in (True, False):
        agent, venv, replay, _, _ = LC.make(8, LC.TINY, 'ou_noise', layernorm=False, capacity=256)
        if null:
            venv.K.synth_ddpg_rollout = null_variant(venv.K)
        try:
            rows = LC.run(agent, venv, replay, (9,), eps=eps_for(8, 3, 9))
        finally:
            if null:
                del venv.K.synth_ddpg_rollout
        assert rows == 8 * LC.closing(9)
        outs.append(LC.final(venv, replay, rows))
    assert calls == [9] and float(outs[0]['ring_actions'].abs().sum()) > 0
    LC.same_bytes(outs[0], outs[1])
