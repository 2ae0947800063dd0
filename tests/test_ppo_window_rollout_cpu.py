"""CPU tier: SyntheticVecEnv.ppo_rollout_into (moving windows straight into the FIFO) through the windowed entry point's
torch-CPU double against n SyntheticEnv behind ExpSenderWrapperMultiStepMovingWindowWithInfo driven by act_batch, bit
for bit; the row arithmetic, FIFOReplay.reserve_ring / commit_ring against insert_batch, reset() and the refusals."""
import numpy as np
import pytest
import torch

import ppo_window_cases as PW


@pytest.fixture
def window_double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(PW.PpoWindowCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


def _run_pair(n, D, A, n_step, stride, rnn_hidden, episode_len, chunks, det=False, use_z=True, seed=3):
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd.replay import FIFOReplay
    steps = sum(chunks)
    eps = None if det else torch.randn(steps, n, A, generator=torch.Generator().manual_seed(seed))
    host_agent, cfg = PW.make_agent(D, A, n_step, stride, rnn_hidden=rnn_hidden, use_z=use_z, deterministic=det,
                                    seed=seed)
    want = PW.host_windows(host_agent, cfg, n, D, episode_len, steps, eps)
    agent, (lc, ec, sc) = PW.make_agent(D, A, n_step, stride, rnn_hidden=rnn_hidden, use_z=use_z, deterministic=det,
                                        seed=seed)
    venv = SyntheticVecEnv(n, D, A, episode_len=episode_len, seeds=list(range(n)), device='cpu')
    assert venv.can_ppo_rollout_into(agent)
    replay = FIFOReplay(lc, ec, sc)
    got, rows = PW.device_windows(venv, agent, replay, chunks, eps)
    return got, rows, want, venv, agent, host_agent


@pytest.mark.parametrize('n_step,stride,rnn_hidden,episode_len,chunks', [
    (25, 20, None, 53, [17, 40, 33, 29]),        # the reference default windows, an episode end inside calls
    (10, 10, None, 23, [7, 12, 15, 9]),          # stride == n_step; 23 - 10 = 13: no window closes at the last step
    (5, 8, None, 21, [6, 11, 9]),                # stride > n_step: advance = n_step
    (7, 3, None, 19, [5, 9, 8, 14]),             # three open windows; a window closes at the terminal step (19 - 7 = 12)
    (25, 20, 12, 53, [17, 40, 33, 29]),          # LSTM stem
    (7, 3, 10, 19, [5, 9, 8, 14]),               # padded LSTM units
    (5, 8, 12, 21, [6, 11, 9]),
    (10, 10, 12, 23, [7, 12, 15, 9]),
])
def test_windows_equal_the_host_wrapper(window_double, n_step, stride, rnn_hidden, episode_len, chunks):
    n, D, A = 5, 7, 3
    got, rows, want, venv, agent, host_agent = _run_pair(n, D, A, n_step, stride, rnn_hidden, episode_len, chunks)
    assert window_double.window_launches == len(chunks)
    closing = PW.closing_count(0, sum(chunks), episode_len, n_step, stride)
    assert rows == n * closing == want['obs'].shape[0] > 0
    keys = set(PW.FIELDS) | ({'cells'} if rnn_hidden else set())
    assert set(got) == keys
    for k in keys:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert venv.t == sum(chunks) % episode_len
    if rnn_hidden:
        for x, y in zip(agent._batch_cells + agent.batch_cells_before,
                        host_agent._batch_cells + host_agent.batch_cells_before):
            assert torch.equal(x.cpu().reshape(y.shape), y.cpu())
    # (the windows that close at a terminal step carry the terminal observation, not the reset state)
    assert float(want['dones'][:, :-1].sum()) == 0.0


@pytest.mark.parametrize('det,use_z', [(True, True), (False, False)])
def test_deterministic_and_unfiltered_agents(window_double, det, use_z):
    got, rows, want, _, _, _ = _run_pair(4, 6, 2, 7, 3, 12, 19, [10, 20], det=det, use_z=use_z)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_reset_equals_a_fresh_environment(window_double):
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd.replay import FIFOReplay
    n, D, A, L = 4, 6, 2, 19
    eps = torch.randn(30, n, A, generator=torch.Generator().manual_seed(5))
    outs = []
    for warm in (False, True):
        agent, (lc, ec, sc) = PW.make_agent(D, A, 7, 3, rnn_hidden=12)
        venv = SyntheticVecEnv(n, D, A, episode_len=L, device='cpu')
        if warm:
            venv.ppo_rollout_into(agent, FIFOReplay(lc, ec, sc), 11, eps=torch.randn(11, n, A))
            venv.reset()
            agent._batch_cells = None
            assert venv.t == 0 and venv._ppo == {}
        outs.append(PW.device_windows(venv, agent, FIFOReplay(lc, ec, sc), [13, 17], eps))
    (a, ra), (b, rb) = outs
    assert ra == rb > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize('t,steps,L,N,stride,want', [
    (0, 128, 1000, 25, 20, 6),                 # windows 0, 20, ..., 100 close at 24, 44, ..., 124
    (0, 10, 8, 10, 10, 0),                     # n_step > episode_len: no window ever
    (0, 100, 8, 10, 10, 0),
    (0, 60, 19, 7, 3, 3 * 5),                  # T longer than several episodes: 5 windows an episode (19 - 7) // 3 + 1
    (5, 14, 19, 7, 3, 5),                      # clocks 5 .. 18: windows 0, 3, .., 12 close at 6, 9, .., 18
    (0, 5, 19, 5, 8, 1),                       # stride > n_step: advance = n_step
])
def test_closing_steps(t, steps, L, N, stride, want):
    assert PW.closing_count(t, steps, L, N, stride) == want


def test_row_counts_of_the_env(window_double):
    """the host's count decides the rows reserved and committed: n_step > episode_len writes nothing, a T of several
    episodes writes every episode's windows"""
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd.replay import FIFOReplay
    n, D, A = 3, 5, 2
    agent, (lc, ec, sc) = PW.make_agent(D, A, 10, 10)
    venv = SyntheticVecEnv(n, D, A, episode_len=8, device='cpu')
    replay = FIFOReplay(lc, ec, sc)
    assert venv.ppo_rollout_into(agent, replay, 37) == 0 and len(replay) == 0 and venv.t == 37 % 8
    agent, (lc, ec, sc) = PW.make_agent(D, A, 7, 3)
    venv = SyntheticVecEnv(n, D, A, episode_len=19, device='cpu')
    replay = FIFOReplay(lc, ec, sc)
    assert venv.ppo_rollout_into(agent, replay, 60) == n * 15 == len(replay)


def _fifo(memory_size):
    lc, ec, sc = PW.configs(3, 2, 4, 4, memory_size=memory_size, batch_size=2)
    from surreal_amd.replay import FIFOReplay
    return FIFOReplay(lc, ec, sc)


@pytest.mark.parametrize('memory_size,batches', [
    (10, [(4, 0), (5, 3), (6, 2), (4, 0)]),    # (rows appended, rows popped): wraps inside a reservation
    (5, [(8, 0), (3, 2), (8, 5)]),             # overflow: the oldest rows are dropped, rows == capacity
    (6, [(0, 0), (9, 4), (2, 0)]),
])
def test_fifo_reserve_ring_equals_insert_batch(window_double, memory_size, batches):
    a, b = _fifo(memory_size), _fifo(memory_size)
    g = torch.Generator().manual_seed(1)
    shapes = {'obs': (2, 3), 'rewards': (2,)}
    for rows, pops in batches:
        f = {k: torch.randn((rows,) + s, generator=g) for k, s in shapes.items()}
        if rows:
            a.insert_batch(f)
        tables, cursor, cap = b.reserve_ring(rows, shapes)
        assert cap == memory_size + 3 and set(tables) == set(shapes)
        for k in shapes:
            for i in range(rows):
                tables[k][(cursor + i) % cap] = f[k][i].reshape(-1)
        b.commit_ring(rows)
        assert (len(a), a._head, a._count, a.cumulative_collected_count) == \
            (len(b), b._head, b._count, b.cumulative_collected_count)
        if pops:
            x, y = a.sample_batch(pops), b.sample_batch(pops)
            for k in shapes:
                assert torch.equal(x[k], y[k]), k


def test_fifo_reserve_ring_refusals(window_double):
    r = _fifo(5)
    with pytest.raises(ValueError, match='do not fit'):
        r.reserve_ring(9, {'obs': (2, 3)})
    r.reserve_ring(8, {'obs': (2, 3)})
    with pytest.raises(ValueError, match='does not match'):
        r.reserve_ring(1, {'obs': (3, 3)})
    with pytest.raises(ValueError, match='does not match'):
        r.reserve_ring(1, {'obs': (2, 3)}, {'obs': torch.uint8})
    with pytest.raises(ValueError, match='does not match'):
        r.reserve_ring(1, {'obs': (2, 3), 'actions': (2,)})


def test_refusals(window_double):
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd.replay import FIFOReplay
    from cpu_kernels import TorchCpuKernels
    n, D, A = 3, 5, 2
    agent, (lc, ec, sc) = PW.make_agent(D, A, 4, 4, rnn_hidden=12)
    replay = FIFOReplay(lc, ec, sc)
    cam = SyntheticVecEnv(n, D, A, episode_len=9, device='cpu', pixel=(1, 4, 4))
    assert not cam.can_ppo_rollout_into(agent)
    with pytest.raises(NotImplementedError, match='camera'):
        cam.ppo_rollout_into(agent, replay, 4)
    two, _ = PW.make_agent(D, A, 4, 4, rnn_hidden=12)
    two.rnn_config.rnn_layer = 2
    venv = SyntheticVecEnv(n, D, A, episode_len=9, device='cpu')
    with pytest.raises(NotImplementedError, match='rnn_layer'):
        venv.ppo_rollout_into(two, replay, 4)
    wide, _ = PW.make_agent(D, 33, 4, 4)
    with pytest.raises(ValueError, match='shapes'):
        SyntheticVecEnv(n, D, 33, episode_len=9, device='cpu').ppo_rollout_into(wide, replay, 4)
    with pytest.raises(NotImplementedError, match='synth_ppo_window_rollout'):
        SyntheticVecEnv(n, D, A, episode_len=9, device='cpu', kernels=TorchCpuKernels()).ppo_rollout_into(
            agent, replay, 4)
    with pytest.raises(ValueError, match='positive'):
        venv.ppo_rollout_into(agent, replay, 0)
    small, (lc2, ec2, sc2) = PW.make_agent(D, A, 4, 4, memory_size=4)
    with pytest.raises(ValueError, match='exceed the FIFO capacity'):
        venv.ppo_rollout_into(small, FIFOReplay(lc2, ec2, sc2), 13)      # 3 actors x 3 windows > 7 rows
    # a clock the carry does not hold: stepped outside ppo_rollout_into
    venv.step(torch.zeros(n, A))
    with pytest.raises(ValueError, match='reset'):
        venv.ppo_rollout_into(agent, replay, 4)
    venv.reset()
    assert venv.ppo_rollout_into(agent, replay, 4) == n
