"""GPU tier (-m gpu): SyntheticVecEnv.ppo_rollout_into on the windowed kernel (smx_synth_ppo_window_rollout_f32) against
the one-launch rollout kernels it shares its layer code with (bit for bit), against the host wrapper driven by act_batch
and a per-step reference (to the rollout tests' tolerance), and in the loop chunk -> FIFO -> PPOLearner.learn."""
import numpy as np
import pytest
import torch

import ppo_window_cases as PW
from surreal_amd import _lib as L

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _venv(n, D, A, L_):
    from surreal_amd.env import SyntheticVecEnv
    return SyntheticVecEnv(n, D, A, episode_len=L_, seeds=list(range(n)))


def _fifo(cfg, rows):
    from surreal_amd.replay import FIFOReplay
    lc, ec, sc = cfg
    lc.replay.memory_size = max(rows, 4)
    lc.replay.batch_size = lc.replay.sampling_start_size = min(64, lc.replay.memory_size)
    return FIFOReplay(lc, ec, sc)


def _table(agent, n, D, A, L_, S, eps):
    """the same S steps from clock 0 and the zero state through synth_rollout / synth_lstm_rollout at 4 actors per
    workgroup (the 4-row loop) into a [n, S + 1] table -> (table, (hN, cN) or None, the final state)"""
    from surreal_amd import kernels as KN
    K, m = KN.default_kernels(), agent.model
    venv = _venv(n, D, A, L_)
    f = lambda *s: torch.zeros(*s, device=venv.device)  # noqa: E731
    rolls = {'obs': f(n, S + 1, D), 'actions': f(n, S + 1, A), 'rewards': f(n, S + 1), 'dones': f(n, S + 1),
             'pds': f(n, S + 1, 2 * A)}
    pk = f(K.epoch_packed_numel(m.actor))
    K.epoch_pack([(m.actor, pk)])
    zf = m.z_filter if agent.use_z_filter else None
    noise = agent.batch_noise(n).view(-1)
    if not m.if_rnn:
        K.synth_rollout(m.actor, pk, L.SMX_ACT_TANH, venv.state, venv.init_state, m.log_var.view(-1), noise, eps, 0,
                        L_, S, 0, rolls, zf, 4)
        return rolls, None, venv.state
    Hl = m.rnn_hidden_logical
    rolls['cells'] = f(n, S + 1, 2, 1, Hl)
    lpk = f(K.lstm_rollout_packed_numel(m.rnn))
    K.lstm_rollout_pack(m.rnn, lpk)
    hN, cN = f(n, Hl), f(n, Hl)
    K.synth_lstm_rollout(m, pk, lpk, venv.state, venv.init_state, noise, eps, 0, L_, S, 0, rolls, zf, hN, cN,
                         actors_per_workgroup=4)
    return rolls, (hN, cN), venv.state


@pytest.mark.parametrize('D,A,hidden,H,n_step,stride,L_,chunks', [
    (11, 3, (24, 16), None, 25, 20, 53, [17, 40, 33, 29]),
    (11, 3, (24, 16), None, 7, 3, 19, [5, 9, 8, 14]),            # windows closing at terminal steps
    (17, 6, (64, 32), 100, 25, 20, 53, [17, 40, 33, 29]),
    (17, 6, (64, 32), 100, 5, 8, 21, [6, 11, 9]),
    (7, 3, (24, 16), 10, 7, 3, 19, [5, 9, 8, 14]),               # padded LSTM units
    (376, 17, (300, 200), None, 10, 10, 23, [7, 12, 15, 9]),
])
def test_windows_equal_the_one_launch_table_bit_for_bit(D, A, hidden, H, n_step, stride, L_, chunks):
    n = 37                                                        # partial last workgroups at every block size
    S = sum(chunks)
    agent, cfg = PW.make_agent(D, A, n_step, stride, hidden=hidden, rnn_hidden=H)
    eps = torch.randn(S, n, A, generator=torch.Generator().manual_seed(4)).cuda()
    table, cells, state = _table(agent, n, D, A, L_, S, eps)
    want, terminal = PW.cut_windows(table, 0, L_, n_step, stride)
    keep = torch.as_tensor(np.repeat(~np.asarray(terminal), n))  # (obs_next at a terminal step: the table's reset state)
    rows = n * PW.closing_count(0, S, L_, n_step, stride)
    assert any(terminal) == ((L_ - n_step) % min(n_step, stride) == 0)
    for apw in (4, 8, 16):
        agent._batch_cells = None
        venv = _venv(n, D, A, L_)
        got, total = PW.device_windows(venv, agent, _fifo(cfg, rows), chunks, eps, actors_per_workgroup=apw)
        torch.cuda.synchronize()
        assert total == rows == want['obs'].shape[0]
        for k, w in want.items():
            g = torch.as_tensor(got[k]).reshape(w.shape)
            w = w.cpu()
            if k == 'obs_next':
                g, w = g[keep], w[keep]
            assert torch.equal(g, w), (apw, k, float((g - w).abs().max()))
        assert torch.equal(venv.state, state), apw
        if cells is not None:
            for x, y in zip(agent._batch_cells, cells):
                assert torch.equal(x.reshape(y.shape).cpu(), y.cpu()), apw


@pytest.mark.parametrize('H,n_step,stride,L_,chunks', [
    (None, 7, 3, 19, [5, 9, 8, 14]),          # terminal observations of windows closing at the episode's last step
    (12, 7, 3, 19, [5, 9, 8, 14]),
    (12, 25, 20, 53, [17, 40, 33, 29]),
    (None, 5, 8, 21, [6, 11, 9]),
])
def test_windows_match_the_host_wrapper(H, n_step, stride, L_, chunks):
    n, D, A = 6, 7, 3
    S = sum(chunks)
    eps = torch.randn(S, n, A, generator=torch.Generator().manual_seed(6))
    host_agent, cfg = PW.make_agent(D, A, n_step, stride, rnn_hidden=H)
    want = PW.host_windows(host_agent, cfg, n, D, L_, S, eps, device='cuda')
    agent, cfg = PW.make_agent(D, A, n_step, stride, rnn_hidden=H)
    got, rows = PW.device_windows(_venv(n, D, A, L_), agent, _fifo(cfg, want['obs'].shape[0]), chunks, eps.cuda())
    assert rows == want['obs'].shape[0] > 0
    for k in want:
        np.testing.assert_allclose(got[k].reshape(want[k].shape), want[k], rtol=TOL, atol=TOL, err_msg=k)


def _per_step(agent, n, D, A, L_, S, eps):
    """act_batch + the step launch per step into a [n, S + 1] table (the LSTM state carried by act_batch)"""
    from surreal_amd import kernels as KN
    K = KN.default_kernels()
    venv = _venv(n, D, A, L_)
    f = lambda *s: torch.zeros(*s, device=venv.device)  # noqa: E731
    r = {'obs': f(n, S + 1, D), 'actions': f(n, S + 1, A), 'rewards': f(n, S + 1), 'dones': f(n, S + 1),
         'pds': f(n, S + 1, 2 * A)}
    rnn = agent.model.if_rnn
    if rnn:
        r['cells'] = f(n, S + 1, 2, 1, agent.model.rnn_hidden_logical)
    t = 0
    for s in range(S):
        acts, _ = agent.act_batch(venv.state, eps=eps[s], out_pd=r['pds'][:, s])
        if rnn:
            h, c = agent.batch_cells_before
            r['cells'][:, s, 0, 0] = h[0]
            r['cells'][:, s, 1, 0] = c[0]
        K.synth_env_step(venv.state, venv.init_state, acts, t, L_, s, r['obs'], r['actions'], r['rewards'], r['dones'])
        t = 0 if t + 1 >= L_ else t + 1
    return r


@pytest.mark.parametrize('D,A,hidden,H', [(376, 17, (300, 200), None), (17, 6, (300, 200), 100)])
def test_benchmark_shapes_match_a_per_step_reference(D, A, hidden, H):
    """1024 actors x 3 calls of 128 steps at (25, 20); (170 - 25) % 20 != 0: no window closes at a terminal step"""
    n, n_step, stride, L_, chunks = 1024, 25, 20, 170, [128, 128, 128]
    S = sum(chunks)
    eps = torch.randn(S, n, A, generator=torch.Generator().manual_seed(8)).cuda()
    ref_agent, cfg = PW.make_agent(D, A, n_step, stride, hidden=hidden, rnn_hidden=H, seed=5)
    want, terminal = PW.cut_windows(_per_step(ref_agent, n, D, A, L_, S, eps), 0, L_, n_step, stride)
    assert not any(terminal)
    agent, cfg = PW.make_agent(D, A, n_step, stride, hidden=hidden, rnn_hidden=H, seed=5)
    rows = want['obs'].shape[0]
    got, total = PW.device_windows(_venv(n, D, A, L_), agent, _fifo(cfg, rows), chunks, eps, as_numpy=False)
    assert total == rows == n * PW.closing_count(0, S, L_, n_step, stride)
    for k, w in want.items():
        g = got[k].reshape(w.shape)
        worst = float(((g - w).abs() - TOL * w.abs()).max())
        assert worst <= TOL, (k, worst)


def test_chunks_to_fifo_to_learn():
    """the reference-default algo config (n_step 25, stride 20, LSTM 100, horizon 5) at configs[1]'s shape: 64 actors,
    128-step chunks of 1000-step episodes -> ppo_rollout_into -> FIFOReplay.sample_batch(copy=False) -> learn.  Every
    window written is learned or still queued, every statistic is finite, and the popped views still hold the rows
    they were popped with after learn (learn reads them in place; the next chunk writes behind them)"""
    from surreal_amd import synthetic
    from surreal_amd.learner import PPOLearner
    n, D, A, L_, T, chunks = 64, 17, 6, 1000, 128, 3
    agent, cfg = PW.make_agent(D, A, 25, 20, hidden=(300, 200), rnn_hidden=100, memory_size=512, batch_size=64)
    lc, ec, sc = cfg
    assert (lc.algo.n_step, lc.algo.stride, lc.algo.rnn.rnn_hidden, lc.algo.rnn.horizon) == (25, 20, 100, 5)
    learner = PPOLearner(lc, ec, sc)
    learner.model.load_params(synthetic.make_ppo_params(D, A, hidden=(300, 200), seed=9, rnn_hidden=100))
    from surreal_amd.replay import FIFOReplay
    replay = FIFOReplay(lc, ec, sc)
    venv = _venv(n, D, A, L_)
    learned = written = 0
    for _ in range(chunks):
        written += venv.ppo_rollout_into(agent, replay, T)
        while len(replay) >= 64:
            views = replay.sample_batch(64, copy=False)
            copies = {k: v.clone() for k, v in views.items()}
            stats = learner.learn(venv.to_batch(views))
            learned += 64
            for k, v in stats.items():
                assert np.isfinite(np.asarray(v, dtype=np.float64)).all(), k
            for k in views:
                assert torch.equal(views[k], copies[k]), k
    torch.cuda.synchronize()
    assert written == n * PW.closing_count(0, chunks * T, L_, 25, 20)
    assert learned + len(replay) == written and learned >= 5 * 64
