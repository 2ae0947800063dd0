"""GPU tier (-m gpu): SyntheticVecEnv.rollout / rollout_into for an LSTM-stem PPO policy on the one-launch kernel
(smx_synth_lstm_rollout_f32) against the per-step stem path (_rollout_stem: act_batch + step launch per step)."""
import numpy as np
import pytest
import torch

import lstm_rollout_cases as LC

pytestmark = pytest.mark.gpu


def _pair(n, D, A, hidden, H, T, use_z=True, det=False, seed=3, episode_len=None, **kw):
    agent, cfg = LC.make_agent(D, A, hidden=hidden, rnn_hidden=H, use_z=use_z, deterministic=det, seed=seed, T=T, n=n)
    eps = torch.randn(T, n, A, generator=torch.Generator().manual_seed(seed)).cuda()
    ep = episode_len or T
    got = LC.run(agent, n, D, A, T, ep, eps, persistent=True, device='cuda', **kw)
    want = LC.run(agent, n, D, A, T, ep, eps, persistent=False, device='cuda')
    torch.cuda.synchronize()
    return got, want, agent, cfg, eps


def _max_diff(got, want):
    (g, gt, gc, gb, _), (w, wt, wc, wb, _) = got, want
    assert set(g) == set(w) and set(LC.RECORDED) <= set(g) and gt == wt
    assert torch.equal(g['dones'], w['dones'])
    worst = {}
    for k in w:
        worst[k] = float((g[k] - w[k]).abs().max())
    for what, x, y in (('h', gc[0], wc[0]), ('c', gc[1], wc[1]), ('h_before', gb[0], wb[0]), ('c_before', gb[1], wb[1])):
        assert x.shape == y.shape, what
        worst[what] = float((x - y).abs().max())
    return worst


def _assert_close(got, want, tol):
    (g, _, gc, gb, _), (w, _, wc, wb, _) = got, want
    for k in w:
        np.testing.assert_allclose(g[k].numpy(), w[k].numpy(), rtol=tol, atol=tol, err_msg=k)
    for x, y in zip(gc + gb, wc + wb):
        np.testing.assert_allclose(x.numpy(), y.numpy(), rtol=tol, atol=tol)


@pytest.mark.parametrize('n,D,A,hidden,H,T,use_z,det', [
    (37, 11, 3, (24, 16), 12, 9, True, False),          # partial last workgroups
    (32, 376, 17, (300, 200), 100, 6, True, False),     # the benchmark shape
    (64, 17, 6, (300, 200), 100, 16, True, False),      # HalfCheetah
    (37, 7, 3, (24, 16), 10, 8, True, False),           # padded units
    (37, 17, 6, (64, 32), 100, 8, True, True),          # deterministic
    (37, 17, 6, (64, 32), 100, 8, False, False),        # no z-filter
])
def test_one_launch_lstm_rollout_matches_the_stem_path(n, D, A, hidden, H, T, use_z, det):
    got, want, _, _, _ = _pair(n, D, A, hidden, H, T, use_z, det)
    _max_diff(got, want)
    _assert_close(got, want, 1e-5)
    g = got[0]
    assert float(g['cells'][:, 0].abs().sum()) == 0.0 and float(g['cells'][:, 1:T].abs().sum()) > 0.0


def test_every_block_size_gives_the_same_bits():
    n, D, A, T, H = 37, 17, 6, 9, 100
    agent, _ = LC.make_agent(D, A, hidden=(64, 32), rnn_hidden=H, T=T, n=n)
    eps = torch.randn(T, n, A, generator=torch.Generator().manual_seed(11)).cuda()
    outs = [LC.run(agent, n, D, A, T, T, eps, device='cuda', actors_per_workgroup=b) for b in (4, 8, 16)]
    torch.cuda.synchronize()
    ref = outs[0]
    for o in outs[1:]:
        assert o[1] == ref[1]
        for k in ref[0]:
            assert torch.equal(o[0][k], ref[0][k]), k
        for x, y in zip(o[2] + o[3], ref[2] + ref[3]):
            assert torch.equal(x, y)
    assert float(ref[0]['dones'].sum()) == n and ref[1] == 0


def test_continuing_from_the_final_state_equals_one_long_launch():
    """h0 / c0 in, hN / cN out: two launches of 5 + 4 steps give the bits of one launch of 9"""
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd import kernels as KN
    K = KN.default_kernels()
    n, D, A, T, H = 37, 17, 6, 9, 100
    agent, _ = LC.make_agent(D, A, hidden=(64, 32), rnn_hidden=H, T=T, n=n)
    m = agent.model
    eps = torch.randn(T, n, A, generator=torch.Generator().manual_seed(5)).cuda()
    pk = torch.zeros(K.epoch_packed_numel(m.actor), device='cuda')
    lpk = torch.zeros(K.lstm_rollout_packed_numel(m.rnn), device='cuda')
    K.epoch_pack([(m.actor, pk)])
    K.lstm_rollout_pack(m.rnn, lpk)
    noise = agent.batch_noise(n).view(-1)
    res = []
    for split in ((0, T), (0, 5, T)):
        venv = SyntheticVecEnv(n, D, A, episode_len=T, seeds=list(range(n)))
        f = lambda *s: torch.zeros(*s, device='cuda')  # noqa: E731
        rolls = {'obs': f(n, T + 1, D), 'actions': f(n, T + 1, A), 'rewards': f(n, T + 1), 'dones': f(n, T + 1),
                 'pds': f(n, T + 1, 2 * A), 'cells': f(n, T + 1, 2, 1, H)}
        h, c = None, None
        for s0, s1 in zip(split[:-1], split[1:]):
            hN, cN = f(n, H), f(n, H)
            K.synth_lstm_rollout(m, pk, lpk, venv.state, venv.init_state, noise, eps[s0:s1].contiguous(), s0, T,
                                 s1 - s0, s0, rolls, m.z_filter, hN, cN, h0=h, c0=c)
            h, c = hN, cN
        torch.cuda.synchronize()
        res.append((rolls, h, c, venv.state.clone()))
    (ra, ha, ca, sa), (rb, hb, cb, sb) = res
    assert torch.equal(ha, hb) and torch.equal(ca, cb) and torch.equal(sa, sb)
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k


def test_rollout_into_equals_rollout_emit_insert_and_learns_the_same():
    """stride == n_step == T: the kernel records straight into the FIFO's slots, bit for bit what rollout ->
    emit_windows -> insert_batch leaves there; learn() on either replay's batch gives the same finite statistics"""
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd.replay import FIFOReplay
    from surreal_amd.learner import PPOLearner
    n, D, A, T, H = 32, 17, 6, 8, 100
    agent, (lc, ec, sc) = LC.make_agent(D, A, hidden=(64, 32), rnn_hidden=H, T=T, n=n)
    eps = torch.randn(T, n, A, generator=torch.Generator().manual_seed(9)).cuda()
    venv = SyntheticVecEnv(n, D, A, episode_len=T, seeds=list(range(n)))
    venv.start_rollout(T, info_width=2 * A)
    venv.rollout(agent, eps=eps)
    a = FIFOReplay(lc, ec, sc)
    a.insert_batch(venv.emit_windows(T, T))
    zc = SyntheticVecEnv(n, D, A, episode_len=T, seeds=list(range(n)))
    assert zc.can_rollout_into(agent)
    zc.start_rollout(T, info_width=2 * A)
    b = FIFOReplay(lc, ec, sc)
    slots = b.reserve_batch(n, zc.window_shapes(T, agent))
    zc.rollout_into(agent, slots, eps=eps)
    b.commit_batch(n)
    torch.cuda.synchronize()
    assert torch.equal(zc.state, venv.state) and zc.t == venv.t
    pa, pb = a.sample_batch(n), b.sample_batch(n, copy=False)
    assert set(pa) == set(pb) and 'cells' in pa
    for k in pa:
        assert torch.equal(pb[k].reshape(pa[k].shape), pa[k]), k
    stats = []
    for env, batch in ((venv, pa), (zc, pb)):
        torch.manual_seed(0)
        learner = PPOLearner(lc, ec, sc)
        learner.model.load_params(agent.model.numpy_params())
        st = learner.learn(env.to_batch(batch))
        torch.cuda.synchronize()
        stats.append(st)
    for k in ('_surr_loss', '_val_loss', '_pol_kl'):
        assert k in stats[0] and np.isfinite(float(stats[0][k])), k
    for k in ('_surr_loss', '_val_loss', '_pol_kl', 'grad_norm_actor', 'grad_norm_critic'):
        if k in stats[0]:
            assert float(stats[0][k]) == float(stats[1][k]), k


def test_1024_actors_128_steps_against_the_stem_path():
    """the bench shape at full length: the recurrence over 128 steps stays within 1e-4 of the stem path"""
    got, want, _, _, _ = _pair(1024, 376, 17, (300, 200), 100, 128, seed=13)
    worst = _max_diff(got, want)
    print('\nlargest |one launch - stem| at 1024 x 128, D = 376, H = 100: %s' %
          ', '.join('%s %.3g' % kv for kv in sorted(worst.items())))
    _assert_close(got, want, 1e-4)
