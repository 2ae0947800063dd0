"""GPU tier (-m gpu): SyntheticVecEnv.ddpg_rollout_into with a camera on the HIP path.

  * one launch of smx_synth_ddpg_pixel_step against the torch-CPU double on the same mu, state, carries and frame
    history: uint8 outputs, dones and row placement exact, float fields to 2e-6 -- 16-byte and byte paths, closing and
    non-closing steps, the last step of an episode, a ring that wraps;
  * the device path against the host path (SyntheticEnv(pixel) + FrameStackWrapper + DDPGAgent.act +
    ExpSenderWrapperSSARNStepBootstrap): float fields to 1e-5, dones exact; the pixel fields exactly as SyntheticEnv's
    camera renders the states the ring recorded, stacked by stack_sources;
  * rollout -> sample_batch(out=staging_fields) -> learn() == learn() on the same rows gathered by indices, with
    pixel / pixel_next staged in place (no reallocation, no recapture).
"""
import collections

import numpy as np
import pytest
import torch

import ddpg_pixel_rollout_cases as PC
import helpers as H
from surreal_amd import _lib as L
from surreal_amd.env.synthetic_env import SyntheticVecEnv
from surreal_amd.replay import UniformReplay

pytestmark = pytest.mark.gpu


def _step_inputs(n, D, A, pixel, S, N, tau, episode_len, cap, cursor, noise, seed):
    g = torch.Generator().manual_seed(seed)
    C, H, W = pixel
    Hd = N + S + 1
    F = C * H * W
    r = dict(state=torch.randn(n, D, generator=g) * 3, init_state=torch.randn(n, D, generator=g), t=tau,
             episode_len=episode_len, n_step=N, noise_type=noise, eps=torch.randn(n, A, generator=g),
             sigmas=torch.rand(n, generator=g, dtype=torch.float64), theta=2.0, dt=0.05, root_dt=float(np.sqrt(0.05)),
             gpow=torch.tensor([0.9 ** e for e in range(N)], dtype=torch.float64),
             ou=torch.randn(n, A, generator=g, dtype=torch.float64) * 0.1,
             carry_obs=torch.randn(n, N, D, generator=g), carry_act=torch.rand(n, N, A, generator=g) * 2 - 1,
             carry_rew=torch.randn(n, N, generator=g), cursor=cursor,
             hist=torch.randint(0, 256, (n, Hd, C, H, W), generator=g, dtype=torch.uint8),
             hist_pos=int(torch.randint(0, Hd, (1,), generator=g)),
             obs_pixel=torch.zeros(n, S * C, H, W, dtype=torch.uint8))
    if noise == L.SMX_DDPG_NOISE_NONE:
        r['eps'] = r['sigmas'] = None
    r['tables'] = {'obs': torch.zeros(cap, D), 'obs_next': torch.zeros(cap, D), 'actions': torch.zeros(cap, A),
                   'rewards': torch.zeros(cap, 1), 'dones': torch.zeros(cap, 1),
                   'pixel': torch.zeros(cap, S * F, dtype=torch.uint8),
                   'pixel_next': torch.zeros(cap, S * F, dtype=torch.uint8)}
    mu = torch.tanh(torch.randn(n, A, generator=g) * 2)
    return r, mu


@pytest.mark.parametrize('pixel', [(3, 36, 36), (1, 21, 22)])
@pytest.mark.parametrize('tau,noise', [(0, L.SMX_DDPG_NOISE_OU), (1, L.SMX_DDPG_NOISE_GAUSSIAN),
                                       (4, L.SMX_DDPG_NOISE_OU), (7, L.SMX_DDPG_NOISE_NONE),
                                       (8, L.SMX_DDPG_NOISE_GAUSSIAN)])
@pytest.mark.parametrize('n,S,N', [(37, 3, 3), (256, 4, 1), (5, 1, 5)])
def test_pixel_step_matches_the_double(pixel, tau, noise, n, S, N):
    """episodes of 9: tau = 8 ends one (terminal frame, new episode's first frame); tau < N - 1 closes nothing"""
    from surreal_amd import kernels as KN
    D, A, cap = 17, 6, 300
    r, mu = _step_inputs(n, D, A, pixel, S, N, tau, 9, cap, cap - n // 2, noise, seed=tau + 7 * n)
    want = H.tensors_to(r, 'cpu')
    got = H.tensors_to(r, 'cuda')
    PC.DdpgPixelRolloutCpuKernels().synth_ddpg_pixel_step(want, mu.clone())
    KN.HipKernels().synth_ddpg_pixel_step(got, mu.cuda())
    torch.cuda.synchronize()
    for k in ('hist', 'obs_pixel'):
        assert torch.equal(got[k].cpu(), want[k]), k
    for k, w in want['tables'].items():
        g = got['tables'][k].cpu()
        if w.dtype == torch.uint8 or k == 'dones':
            assert torch.equal(g, w), k
        else:
            assert torch.allclose(g, w, atol=2e-6, rtol=0), k
    for k in ('state', 'carry_obs', 'carry_act', 'carry_rew', 'ou'):
        assert torch.allclose(got[k].cpu(), want[k], atol=2e-6, rtol=0), k
    rows = (cap - n // 2 + torch.arange(n)) % cap
    written = torch.zeros(cap, dtype=torch.bool)
    written[rows] = tau >= N - 1
    tab = got['tables']['pixel'].cpu()
    assert bool((tab[~written] == 0).all())                       # rows outside the step's are never touched
    if tau >= N - 1 and n > 1:
        assert bool((tab[written].float().sum(1) > 0).all())


CASES = [(37, 1, 1, 'normal'), (37, 3, 3, 'ou_noise'), (37, 5, 4, 'deterministic'), (37, 3, 4, 'normal'),
         (37, 1, 3, 'ou_noise'), (37, 5, 1, 'ou_noise'), (256, 3, 3, 'ou_noise'), (256, 5, 4, 'normal')]


@pytest.mark.parametrize('n,n_step,stacks,noise', CASES)
def test_device_path_matches_host_path(n, n_step, stacks, noise):
    D, A, pixel, L_, calls = 17, 6, (3, 36, 36), 9, (5, 7, 6)      # two whole episodes: every state recorded
    steps = sum(calls)
    closing = [(s % L_) for s in range(steps) if s % L_ >= n_step - 1]
    capacity = n * len(closing) + 7                   # no row is overwritten
    mode = 'eval_deterministic_local' if noise == 'deterministic' else 'training'
    lc, ec, sc = PC.configs(D, A, n, pixel, stacks, hidden=(64, 32), feat=32, memory_size=capacity, n_step=n_step,
                            gamma=0.99, noise_type='normal' if noise == 'deterministic' else noise, theta=2.0, dt=0.05)
    agent = PC.DC.make_agent(lc, ec, sc, mode=mode, w3_scale=1.0)
    eps_all = np.random.RandomState(3).randn(steps, n, A).astype(np.float32)
    venv = SyntheticVecEnv(n, D, A, episode_len=L_, device='cuda', pixel=pixel, frame_stacks=stacks)
    replay = UniformReplay(lc, ec, sc)
    written, s0 = 0, 0
    for T in calls:
        written += venv.ddpg_rollout_into(agent, replay, T, eps=torch.as_tensor(eps_all[s0:s0 + T]).cuda())
        s0 += T
    torch.cuda.synchronize()
    ring = H.device_ring(replay, PC.FIELDS)
    want, total = PC.host_ring(agent, lc, ec, sc, n, L_, eps_all, capacity, pixel, stacks)
    assert written == total == n * len(closing) and len(replay) == total
    for k in PC.DC.FIELDS:
        np.testing.assert_allclose(ring[k].reshape(want[k].shape), want[k], atol=1e-5, rtol=0, err_msg=k)
    assert np.array_equal(ring['dones'].reshape(-1), want['dones'].reshape(-1))
    # the frames exactly as the camera renders the states the device recorded
    pix, nxt = PC.frames_from_record(ring, [(tau, k * n) for k, tau in enumerate(closing)], n, n_step, stacks, pixel,
                                     L_)
    for row in range(total):
        assert np.array_equal(ring['pixel'][row], pix[row].reshape(-1)), ('pixel', row)
        assert np.array_equal(ring['pixel_next'][row], nxt[row].reshape(-1)), ('pixel_next', row)
    assert not ring['pixel'][total:].any() and not ring['pixel_next'][total:].any()


def test_rollout_then_sample_into_staging_then_learn():
    from surreal_amd.learner.ddpg import DDPGLearner
    n, D, A, B, pixel, S = 64, 17, 6, 64, (3, 36, 36), 3
    lc, ec, sc = PC.configs(D, A, n, pixel, S, hidden=(64, 32), feat=32, memory_size=4000, n_step=3,
                            noise_type='ou_noise')
    lc.replay.batch_size = B
    agent = PC.DC.make_agent(lc, ec, sc, w3_scale=1.0)
    venv = SyntheticVecEnv(n, D, A, episode_len=20, device='cuda', pixel=pixel, frame_stacks=S)
    replay = UniformReplay(lc, ec, sc)
    assert venv.ddpg_rollout_into(agent, replay, 30) == n * (18 + 8)
    learners = [DDPGLearner(lc, ec, sc), DDPGLearner(lc, ec, sc)]
    learners[1].model.load_state_dict(learners[0].model.state_dict())
    learners[1].model_target.load_state_dict(learners[0].model_target.state_dict())

    def batch(f):
        obs = collections.OrderedDict(pixel={'camera0': f['pixel']}, low_dim={'flat_inputs': f['obs']})
        nxt = collections.OrderedDict(pixel={'camera0': f['pixel_next']}, low_dim={'flat_inputs': f['obs_next']})
        return {'obs': obs, 'obs_next': nxt, 'actions': f['actions'], 'rewards': f['rewards'].view(B, 1),
                'dones': f['dones'].view(B, 1)}
    addrs = graph = None
    for it in range(4):
        idx = replay.sample_indices(B)
        replay._draws -= B                      # the staged sample below draws the same Philox counters again
        stage = learners[0].staging_fields(B)
        assert stage['pixel'].dtype == torch.uint8 and tuple(stage['pixel'].shape) == (B, S * 3, 36, 36)
        f0 = replay.sample_batch(B, out=stage)
        f1 = replay.sample_batch(B, indices=idx)
        for k in f0:
            assert torch.equal(f0[k].reshape(-1), f1[k].reshape(-1)), k
        assert f0['pixel'].data_ptr() == stage['pixel'].data_ptr()
        st0 = dict(learners[0].learn(batch(f0)))
        st1 = dict(learners[1].learn(batch(f1)))
        assert st0 == st1, (it, st0, st1)
        assert all(np.isfinite(v) for v in st0.values())
        ws = learners[0]._ws
        now = {k: v.data_ptr() for k, v in learners[0].staging_fields(B).items()}
        assert ws.s_pix.data_ptr() == now['pixel'] and ws.s_pix_next.data_ptr() == now['pixel_next']
        if addrs is None:
            addrs, graph = now, ws.graph
        assert now == addrs and ws.graph is graph, it          # no reallocation, no recapture
    m0, m1 = learners[0].model, learners[1].model
    for a, b in ((m0.actor_flat, m1.actor_flat), (m0.critic_flat, m1.critic_flat),
                 (m0.perception_flat, m1.perception_flat)):
        assert torch.equal(a, b)
