"""GPU tier (-m gpu): SyntheticVecEnv.ddpg_rollout_into on the HIP path.

  * the one-launch kernel (smx_synth_ddpg_rollout_f32) against its two-launch reference (smx_epoch_forward_f32 + the
    step launch smx_synth_ddpg_step_f32): float fields to 2e-6, dones, row placement and counts exact, rows never
    written still zero; every forced block size bit for bit the same;
  * the device path against the host path (SyntheticEnv + DDPGAgent.act + ExpSenderWrapperSSARNStepBootstrap) to 1e-5,
    a LayerNorm actor (the per-step path) included;
  * rollout -> sample_batch(out=staging_fields) -> learn() == learn() on the same rows gathered by indices.
"""
import numpy as np
import pytest
import torch

import ddpg_rollout_cases as DC
import helpers as H
from surreal_amd.env.synthetic_env import SyntheticVecEnv
from surreal_amd.replay import UniformReplay

pytestmark = pytest.mark.gpu


def device_run(agent, lc, ec, sc, n, episode_len, eps, calls, **kw):
    D, A = agent.model.input_dim, agent.action_dim
    venv = SyntheticVecEnv(n, D, A, episode_len=episode_len, device='cuda')
    replay = UniformReplay(lc, ec, sc)
    written, s0 = 0, 0
    for T in calls:
        written += venv.ddpg_rollout_into(agent, replay, T, eps=eps[s0:s0 + T], **kw)
        s0 += T
    torch.cuda.synchronize()
    extra = {k: venv._ddpg[k].cpu().numpy() for k in ('ou', 'carry_obs', 'carry_act', 'carry_rew')}
    extra['state'] = venv.state.cpu().numpy()
    return written, replay, H.device_ring(replay, DC.FIELDS), extra


def compare(got, want, written, capacity, atol):
    rows = min(written, capacity)
    for k in DC.FIELDS:
        g, w = got[k], want[k]
        if k == 'dones':
            assert np.array_equal(g, w)
        elif atol == 0:
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), k
        else:
            np.testing.assert_allclose(g, w, atol=atol, rtol=0, err_msg=k)
        assert not np.any(g[rows:]), k                       # never written: still zero
    # every written row holds a transition (an observation is never all zero here)
    assert np.all(np.any(got['obs'][:rows] != 0, axis=1))


@pytest.mark.parametrize('noise', ['normal', 'ou_noise', 'deterministic'])
@pytest.mark.parametrize('n,hidden', [(37, (64, 32)), (1024, (300, 200))])
def test_persistent_kernel_matches_two_launch_reference(noise, n, hidden):
    D, A, L_ = 17, 6, 11
    calls = (9, 13, 6)                       # episodes end inside calls, later calls start mid-episode
    mode = 'eval_deterministic_local' if noise == 'deterministic' else 'training'
    capacity = 200000
    lc, ec, sc = DC.configs(D, A, n, hidden=hidden, n_step=3, gamma=0.99, memory_size=capacity,
                            noise_type='normal' if noise == 'deterministic' else noise, theta=2.0, dt=0.02)
    agent = DC.make_agent(lc, ec, sc, mode=mode, w3_scale=1.0)
    eps = torch.randn(sum(calls), n, A, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))
    w_ref, _, ring_ref, ex_ref = device_run(agent, lc, ec, sc, n, L_, eps, calls, reference=True)
    m = sum(1 for s in range(sum(calls)) if s % L_ >= 2)
    assert w_ref == n * m
    blocks = (0, 4, 8, 16) if n == 37 else (0, 16)
    first = None
    for apw in blocks:
        w, replay, ring, ex = device_run(agent, lc, ec, sc, n, L_, eps, calls, actors_per_workgroup=apw)
        assert w == w_ref and len(replay) == w and replay._dev_next == w and replay.cumulative_collected_count == w
        compare(ring, ring_ref, w, capacity, atol=2e-6)
        for k in ex:
            np.testing.assert_allclose(ex[k], ex_ref[k], atol=2e-6, rtol=0, err_msg=k)
        if first is None:
            first = (ring, ex)
        else:                                   # block sizes: the same bits
            compare(ring, first[0], w, capacity, atol=0)
            for k in ex:
                assert np.array_equal(ex[k], first[1][k]), k


def test_persistent_kernel_wraps_the_ring():
    n, D, A = 37, 17, 6
    lc, ec, sc = DC.configs(D, A, n, hidden=(64, 32), n_step=2, memory_size=100, noise_type='ou_noise')
    agent = DC.make_agent(lc, ec, sc, w3_scale=1.0)
    eps = torch.randn(7, n, A, device='cuda')
    outs = []
    for ref in (False, True):
        venv = SyntheticVecEnv(n, D, A, episode_len=5, device='cuda')
        replay = UniformReplay(lc, ec, sc)
        w = sum(venv.ddpg_rollout_into(agent, replay, 2, eps=eps[2 * i:2 * i + 2], reference=ref) for i in range(3))
        w += venv.ddpg_rollout_into(agent, replay, 1, eps=eps[6:], reference=ref)
        outs.append((w, replay._dev_next, len(replay), H.device_ring(replay, DC.FIELDS)))
    assert outs[0][:3] == outs[1][:3] == (5 * n, 5 * n % 100, 100)
    for k in DC.FIELDS:
        np.testing.assert_allclose(outs[0][3][k], outs[1][3][k], atol=2e-6, rtol=0, err_msg=k)


def host_parity(n, D, A, hidden, episode_len, calls, capacity, **cfg):
    lc, ec, sc = DC.configs(D, A, n, hidden=hidden, memory_size=capacity, **cfg)
    agent = DC.make_agent(lc, ec, sc, w3_scale=1.0)
    eps_all = np.random.RandomState(3).randn(sum(calls), n, A).astype(np.float32)
    w, replay, ring, _ = device_run(agent, lc, ec, sc, n, episode_len, torch.as_tensor(eps_all).cuda(), calls)
    want, total = DC.host_ring(agent, lc, ec, sc, n, episode_len, eps_all, capacity)
    assert w == total and len(replay) == min(total, capacity)
    for k in DC.FIELDS:
        np.testing.assert_allclose(ring[k].reshape(want[k].shape), want[k], atol=1e-5, rtol=0, err_msg=k)
    assert np.array_equal(ring['dones'], want['dones'])
    return total


def test_device_path_matches_host_path_default_shape():
    assert host_parity(4, 17, 6, (300, 200), 10, (7, 8), 64, n_step=3, gamma=0.99, noise_type='normal') > 0


def test_device_path_matches_host_path_ou():
    assert host_parity(3, 17, 6, (300, 200), 8, (5, 6), 40, n_step=2, gamma=0.5, noise_type='ou_noise',
                       theta=2.0, dt=0.05) > 0


def test_layernorm_actor_takes_per_step_path_and_matches_host():
    assert host_parity(3, 17, 6, (64, 32), 8, (5, 6), 40, n_step=3, gamma=0.99, noise_type='ou_noise',
                       layernorm=True) > 0


def test_rollout_then_sample_into_staging_then_learn():
    from surreal_amd.learner.ddpg import DDPGLearner
    n, D, A, B = 256, 17, 6, 128
    lc, ec, sc = DC.configs(D, A, n, hidden=(300, 200), n_step=3, memory_size=20000, noise_type='ou_noise')
    lc.replay.batch_size = B
    agent = DC.make_agent(lc, ec, sc, w3_scale=1.0)
    venv = SyntheticVecEnv(n, D, A, episode_len=20, device='cuda')
    replay = UniformReplay(lc, ec, sc)
    assert venv.ddpg_rollout_into(agent, replay, 30) == n * (18 + 8)
    learners = [DDPGLearner(lc, ec, sc), DDPGLearner(lc, ec, sc)]
    learners[1].model.load_state_dict(learners[0].model.state_dict())
    learners[1].model_target.load_state_dict(learners[0].model_target.state_dict())

    def batch(f):
        return {'obs': {'low_dim': {'flat_inputs': f['obs']}}, 'obs_next': {'low_dim': {'flat_inputs': f['obs_next']}},
                'actions': f['actions'], 'rewards': f['rewards'].view(B, 1), 'dones': f['dones'].view(B, 1)}
    for it in range(4):
        idx = replay.sample_indices(B)
        replay._draws -= B                      # the staged sample below draws the same Philox counters again
        stage = learners[0].staging_fields(B)
        f0 = replay.sample_batch(B, out=stage)
        f1 = replay.sample_batch(B, indices=idx)
        for k in f0:
            assert torch.equal(f0[k].reshape(-1), f1[k].reshape(-1)), k
        st0 = dict(learners[0].learn(batch(f0)))
        st1 = dict(learners[1].learn(batch(f1)))
        assert st0 == st1, (it, st0, st1)
        assert all(np.isfinite(v) for v in st0.values())
    assert torch.equal(learners[0].model.actor_flat, learners[1].model.actor_flat)
    assert torch.equal(learners[0].model.critic_flat, learners[1].model.critic_flat)
