"""CPU tier: SyntheticVecEnv.ddpg_rollout_into (DDPG acting + n-step transitions written into the uniform replay's
ring) on the torch-CPU double of its kernels against the host path -- n SyntheticEnv + DDPGAgent +
ExpSenderWrapperSSARNStepBootstrap stepped one by one -- bit for bit; its refusals."""

import numpy as np
import pytest
import torch

import ddpg_rollout_cases as DC
import helpers as H



@pytest.fixture
def ddpg_double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(DC.DdpgRolloutCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


def run_device(K, agent, lc, ec, sc, n, episode_len, eps_all, calls, **kw):
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    D, A = agent.model.input_dim, agent.action_dim
    venv = SyntheticVecEnv(n, D, A, episode_len=episode_len, device='cpu', kernels=K)
    replay = UniformReplay(lc, ec, sc)
    written, s0 = 0, 0
    for T in calls:
        eps = torch.as_tensor(eps_all[s0:s0 + T])
        written += venv.ddpg_rollout_into(agent, replay, T, eps=eps, **kw)
        s0 += T
        assert venv.t == H_clock(s0, episode_len)
    return venv, replay, written


def H_clock(steps, episode_len):
    return steps % episode_len


def assert_rings_equal(got, want, atol=0.0):
    for k in DC.FIELDS:
        g, w = got[k].reshape(want[k].shape), want[k]
        if atol == 0.0:
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (k, np.argwhere(g != w)[:5])
        else:
            np.testing.assert_allclose(g, w, atol=atol, rtol=0, err_msg=k)


def check_against_host(K, n=3, D=7, A=3, episode_len=9, calls=(5, 7, 4), capacity=23, mode='training',
                       atol=0.0, **cfg):
    lc, ec, sc = DC.configs(D, A, n, memory_size=capacity, **cfg)
    agent = DC.make_agent(lc, ec, sc, mode=mode)
    rs = np.random.RandomState(11)
    eps_all = rs.randn(sum(calls), n, A).astype(np.float32)
    venv, replay, written = run_device(K, agent, lc, ec, sc, n, episode_len, eps_all, calls)
    want, total = DC.host_ring(agent, lc, ec, sc, n, episode_len, eps_all, capacity)
    assert written == total
    assert len(replay) == min(capacity, total) and replay._dev_next == total % capacity
    assert replay.cumulative_collected_count == total
    if total:
        assert_rings_equal(H.device_ring(replay, DC.FIELDS), want, atol)
    return total


@pytest.mark.parametrize('gamma', [0.99, 0.5])
@pytest.mark.parametrize('n_step', [1, 3, 5])
@pytest.mark.parametrize('noise', ['normal', 'ou_noise', 'deterministic'])
def test_ddpg_rollout_matches_host_path_bit_for_bit(ddpg_double, noise, n_step, gamma):
    """three calls of 5, 7 and 4 steps over episodes of 9: episodes end inside calls, calls start mid-episode (the open
    transitions and the OU state carry over), and the 23-row ring wraps"""
    mode = 'eval_deterministic_local' if noise == 'deterministic' else 'training'
    total = check_against_host(ddpg_double, mode=mode, n_step=n_step, gamma=gamma,
                               noise_type='normal' if noise == 'deterministic' else noise, max_sigma=0.8)
    assert total > 23                          # the ring wrapped


def test_ddpg_rollout_default_shape_and_one_actor(ddpg_double):
    """one actor (sigma = max_sigma / 3) and an OU process with a visible drift"""
    check_against_host(ddpg_double, n=1, D=17, A=6, episode_len=6, calls=(4, 9), capacity=10, n_step=2,
                       noise_type='ou_noise', theta=3.0, dt=0.05, hidden=(32, 20))


def test_ddpg_rollout_n_step_longer_than_an_episode_writes_nothing(ddpg_double):
    total = check_against_host(ddpg_double, episode_len=4, calls=(6, 5), n_step=5)
    assert total == 0


def test_ddpg_rollout_layernorm_actor_takes_the_per_step_path(ddpg_double):
    """a LayerNorm actor is refused by the persistent kernel's path: one forward_actor over all actors per step, then
    the step launch (batched rows: the double's summation may round differently from batch-1 act)"""
    calls = []
    orig = ddpg_double.synth_ddpg_step
    ddpg_double.synth_ddpg_step = lambda r, mu: (calls.append(1), orig(r, mu))
    try:
        check_against_host(ddpg_double, layernorm=True, n_step=3, noise_type='ou_noise', atol=1e-5)
    finally:
        del ddpg_double.synth_ddpg_step
    assert len(calls) == 16


def test_ddpg_rollout_reference_path_agrees(ddpg_double):
    """the two-launch reference (epoch_forward + step launch) writes the same rows as the one-launch path"""
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    n, D, A, L_ = 5, 7, 3, 8
    lc, ec, sc = DC.configs(D, A, n, memory_size=200, n_step=3, noise_type='ou_noise')
    agent = DC.make_agent(lc, ec, sc)
    eps = torch.randn(12, n, A, generator=torch.Generator().manual_seed(2))
    out = []
    for ref in (False, True):
        venv = SyntheticVecEnv(n, D, A, episode_len=L_, device='cpu', kernels=ddpg_double)
        replay = UniformReplay(lc, ec, sc)
        w = venv.ddpg_rollout_into(agent, replay, 7, eps=eps[:7], reference=ref)
        w += venv.ddpg_rollout_into(agent, replay, 5, eps=eps[7:], reference=ref)
        out.append((w, H.device_ring(replay, DC.FIELDS), venv.state.clone()))
    assert out[0][0] == out[1][0] == n * (5 + 3)
    assert_rings_equal(out[1][1], out[0][1], atol=1e-6)
    assert torch.allclose(out[0][2], out[1][2], atol=1e-6, rtol=0)


def test_ddpg_rollout_reset_clears_the_carry(ddpg_double):
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    n, D, A = 2, 5, 2
    lc, ec, sc = DC.configs(D, A, n, memory_size=64, n_step=3, noise_type='ou_noise')
    agent = DC.make_agent(lc, ec, sc)
    venv = SyntheticVecEnv(n, D, A, episode_len=10, device='cpu', kernels=ddpg_double)
    replay = UniformReplay(lc, ec, sc)
    assert venv.ddpg_rollout_into(agent, replay, 4) == n * 2
    assert venv.t == 4 and float(venv._ddpg['ou'].abs().sum()) > 0 and float(venv._ddpg['carry_obs'].abs().sum()) > 0
    venv.reset()
    assert venv.t == 0 and torch.equal(venv.state, venv.init_state)
    for k in ('ou', 'carry_obs', 'carry_act', 'carry_rew'):
        assert float(venv._ddpg[k].abs().sum()) == 0, k


def test_ddpg_rollout_refusals(ddpg_double):
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    n, D, A = 4, 6, 2
    lc, ec, sc = DC.configs(D, A, n, memory_size=10, n_step=2)
    agent = DC.make_agent(lc, ec, sc)
    venv = SyntheticVecEnv(n, D, A, episode_len=20, device='cpu', kernels=ddpg_double)
    replay = UniformReplay(lc, ec, sc)
    with pytest.raises(ValueError, match='capacity'):
        venv.ddpg_rollout_into(agent, replay, 4)           # 3 closing steps x 4 actors > 10 rows
    assert venv.t == 0 and len(replay) == 0 and replay.cumulative_collected_count == 0
    assert venv.ddpg_rollout_into(agent, replay, 3) == 8   # 2 closing steps x 4 actors fit
    cam = SyntheticVecEnv(n, D, A, episode_len=20, device='cpu', kernels=ddpg_double, pixel=(3, 8, 8))
    with pytest.raises(NotImplementedError, match='camera'):
        cam.ddpg_rollout_into(agent, replay, 2)
    lc2, ec2, sc2 = DC.configs(D, A, n, memory_size=10, n_step=2, param_noise_type='adaptive_normal')
    adaptive = DC.make_agent(lc2, ec2, sc2)
    with pytest.raises(NotImplementedError, match='adaptive_normal'):
        venv.ddpg_rollout_into(adaptive, replay, 2)
    lc3, ec3, sc3 = DC.configs(D, A, n, memory_size=10, n_step=2, param_noise_type='normal')
    assert venv.ddpg_rollout_into(DC.make_agent(lc3, ec3, sc3), replay, 1) == n   # weight noise at fetch time: fine


def test_batch_sigmas_follow_the_per_agent_rule(ddpg_double):
    lc, ec, sc = DC.configs(5, 2, 7, max_sigma=0.7)
    agent = DC.make_agent(lc, ec, sc)
    s = agent.batch_sigmas(7)
    assert s.dtype == torch.float64
    for i in range(7):
        lci, eci, sci = DC.configs(5, 2, 7, max_sigma=0.7)
        assert float(s[i]) == DC.make_agent(lci, eci, sci, agent_id=i).sigma
    assert float(agent.batch_sigmas(1)[0]) == 0.7 / 3.0
