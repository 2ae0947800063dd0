"""GPU tier (-m gpu): SyntheticVecEnv.ppo_rollout_into with a camera on the HIP path.

  * one launch of smx_synth_ppo_pixel_window_step against the torch-CPU double on the same mu, state, carry rings,
    cells and frame history: uint8 outputs, dones and row placement exact, float fields to 2e-6 -- 16-byte and byte
    paths, closing and non-closing steps, the last step of an episode with and without a closing window, window
    starts with and without cells, a cursor that wraps;
  * the device path against the host path (SyntheticEnv(pixel) under FrameStackWrapper under
    ExpSenderWrapperMultiStepMovingWindowWithInfo, driven by act_batch): float fields to 1e-5, dones exact; the pixel
    fields exactly as SyntheticEnv's camera renders the states the ring recorded next to them;
  * calls -> FIFO -> sample_batch(copy=False) -> PPOLearner.learn with the CNN + LSTM policy.
"""
import numpy as np
import pytest
import torch

import helpers as H
import ppo_pixel_window_cases as PP
import ppo_window_cases as PW

pytestmark = pytest.mark.gpu

TOL = 1e-5                      # (the window tests' tolerance, test_gpu_ppo_window_rollout.py)


def _step_inputs(n, D, A, pixel, S, N, adv, tau, episode_len, cap, cursor, Hl, cells, eps, seed):
    g = torch.Generator().manual_seed(seed)
    C, H, W = pixel
    Hd = N + S + 1
    F = C * H * W
    Sc = -(-N // adv)
    r = dict(state=torch.randn(n, D, generator=g) * 3, init_state=torch.randn(n, D, generator=g), t=tau,
             episode_len=episode_len, n_step=N, advance=adv, log_var=torch.randn(A, generator=g) * 0.3 - 1.0,
             noise_scale=torch.exp(torch.rand(n, generator=g) - 0.5), eps=torch.randn(n, A, generator=g) if eps else None,
             cursor=cursor, hist=torch.randint(0, 256, (n, Hd, C, H, W), generator=g, dtype=torch.uint8),
             hist_pos=int(torch.randint(0, Hd, (1,), generator=g)),
             obs_pixel=torch.zeros(n, S * C, H, W, dtype=torch.uint8))
    r['carry'] = {'obs': torch.randn(n, N, D, generator=g), 'actions': torch.rand(n, N, A, generator=g) * 2 - 1,
                  'rewards': torch.randn(n, N, generator=g), 'pds': torch.randn(n, N, 2 * A, generator=g)}
    r['tables'] = {'obs': torch.zeros(cap, N * D), 'obs_next': torch.zeros(cap, D), 'actions': torch.zeros(cap, N * A),
                   'rewards': torch.zeros(cap, N), 'dones': torch.full((cap, N), -1.0), 'pds': torch.zeros(cap, N * 2 * A),
                   'pixel': torch.zeros(cap, N * S * F, dtype=torch.uint8),
                   'pixel_next': torch.zeros(cap, S * F, dtype=torch.uint8)}
    if Hl:
        r['carry']['cells'] = torch.randn(n, Sc, 2, Hl, generator=g)
        r['tables']['cells'] = torch.zeros(cap, 2 * Hl)
        if cells:
            r['h_before'], r['c_before'] = torch.randn(n, Hl, generator=g), torch.randn(n, Hl, generator=g)
    mu = torch.tanh(torch.randn(n, A, generator=g) * 2)
    return r, mu


# episodes of 12, (n_step, advance) = (4, 2): windows close at tau = 3, 5, 7, 9, 11 (the terminal step); (5, 5): at 4 and 9,
# so tau = 11 ends an episode without a closing window.  (tau, N, adv, Hl, cells given, eps given)
STEPS = [(2, 4, 2, 12, True, True),          # a window start, nothing closes
         (2, 4, 2, 12, False, True),         # ... without cells: the cells' ring is left alone
         (4, 4, 2, 0, False, True),          # a policy without an LSTM, a non-closing step
         (5, 4, 2, 12, True, True),          # a closing step that is no window start
         (8, 4, 2, 12, True, False),         # a window start; deterministic
         (11, 4, 2, 12, True, True),         # the last step of an episode with a closing window
         (11, 5, 5, 12, False, True),        # ... and without one
         (9, 5, 5, 0, False, True),          # advance == n_step
         (0, 1, 1, 12, True, True)]          # n_step 1: every step starts and closes a window


@pytest.mark.parametrize('pixel', [(3, 36, 36), (1, 21, 22)])
@pytest.mark.parametrize('tau,N,adv,Hl,cells,eps', STEPS)
@pytest.mark.parametrize('n,S', [(37, 3), (256, 4), (5, 1)])
def test_step_matches_the_double(pixel, tau, N, adv, Hl, cells, eps, n, S):
    from surreal_amd import kernels as KN
    D, A, cap = 17, 6, 300
    cursor = cap - n // 2                                        # the rows wrap
    r, mu = _step_inputs(n, D, A, pixel, S, N, adv, tau, 12, cap, cursor, Hl, cells, eps, seed=tau + 7 * n + N)
    want, got = H.tensors_to(r, 'cpu'), H.tensors_to(r, 'cuda')
    PP.PpoPixelWindowCpuKernels().synth_ppo_pixel_window_step(want, mu.clone())
    KN.HipKernels().synth_ppo_pixel_window_step(got, mu.cuda())
    torch.cuda.synchronize()
    for k in ('hist', 'obs_pixel'):
        assert torch.equal(got[k].cpu(), want[k]), k
    for k, w in want['tables'].items():
        g = got['tables'][k].cpu()
        if w.dtype == torch.uint8 or k == 'dones':
            assert torch.equal(g, w), k
        else:
            err = float((g - w).abs().max())
            print('%s max abs error %.3g' % (k, err))
            assert err <= 2e-6, (k, err)
    for k, w in list(want['carry'].items()) + [('state', want['state'])]:
        g = got['carry'][k].cpu() if k != 'state' else got['state'].cpu()
        err = float((g - w).abs().max())
        assert err <= 2e-6, (k, err)
    j = tau + 1 - N
    closing = j >= 0 and j % adv == 0
    written = torch.zeros(cap, dtype=torch.bool)
    written[(cursor + torch.arange(n)) % cap] = closing
    for k in ('pixel', 'dones', 'obs'):
        tab = got['tables'][k].cpu()
        untouched = -1.0 if k == 'dones' else 0
        assert bool((tab[~written] == untouched).all()), k        # rows outside the step's are never touched
    if closing:
        assert bool((got['tables']['dones'].cpu()[written] >= 0).all())
        assert bool((got['tables']['pixel'].cpu()[written].float().sum(1) > 0).all())


CASES = [(37, 7, 3, 12, 3, True), (37, 5, 8, None, 1, True), (37, 4, 4, 12, 3, False), (256, 7, 3, None, 3, True),
         (5, 25, 20, 100, 3, True)]


@pytest.mark.parametrize('n,n_step,stride,rnn_hidden,stacks,use_z', CASES)
def test_device_path_matches_host_path(n, n_step, stride, rnn_hidden, stacks, use_z):
    """several calls over more than two whole episodes, windows closing at terminal steps where the lengths allow it"""
    from surreal_amd.replay import FIFOReplay
    D, A, pixel = 17, 6, (3, 36, 36)
    L_ = {7: 19, 5: 20, 4: 12, 25: 45}[n_step]
    calls = [L_ - 3, 5, L_ + 2, L_ // 2]
    steps = sum(calls)
    closing = PW.closing_steps(0, steps, L_, n_step, stride)
    total = n * len(closing)
    assert steps > 2 * L_ and L_ - 1 in closing
    kw = dict(hidden=(64, 32), rnn_hidden=rnn_hidden, use_z=use_z, feat=32, memory_size=total + 7, final_scale=1.0)
    eps = torch.randn(steps, n, A, generator=torch.Generator().manual_seed(3))
    host_agent, cfg = PP.make_agent(D, A, n_step, stride, pixel, stacks, **kw)
    want = PP.host_windows(host_agent, cfg, n, D, L_, steps, eps, pixel, stacks, device='cuda')
    agent, (lc, ec, sc) = PP.make_agent(D, A, n_step, stride, pixel, stacks, **kw)
    venv = PP.make_venv(n, D, A, L_, pixel, stacks)
    replay = FIFOReplay(lc, ec, sc)
    written, s0 = 0, 0
    for T in calls:
        written += venv.ppo_rollout_into(agent, replay, T, eps=eps[s0:s0 + T].cuda())
        s0 += T
    torch.cuda.synchronize()
    assert written == total == want['obs'].shape[0] == len(replay)
    ring = H.device_ring(replay)
    floats = [k for k in want if k not in ('pixel', 'pixel_next', 'dones')]
    for k in floats:
        g, w = ring[k][:total].reshape(want[k].shape), want[k]
        print('%s max abs error %.3g' % (k, float(np.abs(g - w).max())))
        np.testing.assert_allclose(g, w, rtol=TOL, atol=TOL, err_msg=k)
    assert np.array_equal(ring['dones'][:total].reshape(want['dones'].shape), want['dones'])
    # the frames exactly as the camera renders the states the device recorded next to them
    pix, nxt = PP.frames_from_record(ring, [(tau, k * n) for k, tau in enumerate(closing)], n, n_step, stacks, pixel)
    for row in range(total):
        assert np.array_equal(ring['pixel'][row], pix[row].reshape(-1)), ('pixel', row)
        assert np.array_equal(ring['pixel_next'][row], nxt[row].reshape(-1)), ('pixel_next', row)
    for k in ring:
        assert not ring[k][total:].any(), k                    # nothing written past the rows counted
    if rnn_hidden:
        for x, y in zip(agent._batch_cells + agent.batch_cells_before,
                        host_agent._batch_cells + host_agent.batch_cells_before):
            np.testing.assert_allclose(x.reshape(y.shape).cpu().numpy(), y.cpu().numpy(), rtol=TOL, atol=TOL)


def test_calls_to_fifo_to_learn():
    """the CNN + LSTM policy at the reference's window rule (n_step 25, stride 20, horizon 5): 64 actors, calls of 64
    steps of 1000-step episodes -> ppo_rollout_into -> FIFOReplay.sample_batch(copy=False) -> learn.  Every window
    written is learned or still queued, every statistic is finite, and the popped views still hold the rows they were
    popped with after learn"""
    from surreal_amd import synthetic
    from surreal_amd.learner import PPOLearner
    from surreal_amd.replay import FIFOReplay
    n, D, A, L_, T, calls, pixel, S, feat = 64, 17, 6, 1000, 64, 4, (3, 36, 36), 3, 64
    agent, (lc, ec, sc) = PP.make_agent(D, A, 25, 20, pixel, S, hidden=(300, 200), rnn_hidden=100, feat=feat,
                                        memory_size=512, batch_size=64)
    assert (lc.algo.n_step, lc.algo.stride, lc.algo.rnn.rnn_hidden, lc.algo.rnn.horizon) == (25, 20, 100, 5)
    learner = PPOLearner(lc, ec, sc)
    learner.model.load_params(synthetic.make_ppo_params(D, A, hidden=(300, 200), seed=9, rnn_hidden=100,
                                                        pixel=(S * pixel[0],) + pixel[1:], cnn_feature_dim=feat))
    replay = FIFOReplay(lc, ec, sc)
    venv = PP.make_venv(n, D, A, L_, pixel, S)
    learned = written = 0
    for _ in range(calls):
        written += venv.ppo_rollout_into(agent, replay, T)
        while len(replay) >= 64:
            views = replay.sample_batch(64, copy=False)
            assert views['pixel'].dtype == torch.uint8 and tuple(views['pixel'].shape) == (64, 25, 9, 36, 36)
            copies = {k: v.clone() for k, v in views.items()}
            stats = learner.learn(venv.to_batch(views))
            learned += 64
            for k, v in stats.items():
                assert np.isfinite(np.asarray(v, dtype=np.float64)).all(), k
            for k in views:
                assert torch.equal(views[k], copies[k]), k
    torch.cuda.synchronize()
    assert written == n * PW.closing_count(0, calls * T, L_, 25, 20)
    assert learned + len(replay) == written and learned >= 3 * 64
