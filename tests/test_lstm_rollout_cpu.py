"""CPU tier: SyntheticVecEnv.rollout / rollout_into for an LSTM-stem PPO policy through the one-launch entry points (on
their torch-CPU double) against _rollout_stem, bit for bit; which policies and environments take which path; the
replay-slot path and the learner's onetime_infos."""

import pytest
import torch

import lstm_rollout_cases as LC


@pytest.fixture
def lstm_double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(LC.LstmRolloutCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


def assert_same(a, b, what=''):
    assert a.shape == b.shape and torch.equal(a, b), (what, (a - b).abs().max() if a.shape == b.shape else a.shape)


@pytest.mark.parametrize('use_z,det,rnn_hidden', [(True, False, 12), (False, False, 12), (True, True, 12),
                                                  (True, False, 10)])
def test_one_launch_rollout_equals_the_stem_path(lstm_double, use_z, det, rnn_hidden):
    n, D, A, T = 5, 7, 3, 6
    agent, _ = LC.make_agent(D, A, rnn_hidden=rnn_hidden, use_z=use_z, deterministic=det)
    eps = torch.randn(T, n, A, generator=torch.Generator().manual_seed(2))
    got = LC.run(agent, n, D, A, T, T, eps, persistent=True)
    assert lstm_double.lstm_launches == 1
    want = LC.run(agent, n, D, A, T, T, eps, persistent=False)
    assert lstm_double.lstm_launches == 1
    (g, gt, gc, gb, _), (w, wt, wc, wb, _) = got, want
    assert set(g) == set(w) and set(LC.RECORDED) <= set(g)
    for k in w:
        assert_same(g[k], w[k], k)
    assert gt == wt
    for x, y, what in ((gc[0], wc[0], 'h'), (gc[1], wc[1], 'c'), (gb[0], wb[0], 'h before'), (gb[1], wb[1], 'c before')):
        assert_same(x, y, what)
    assert tuple(gc[0].shape) == (1, n, rnn_hidden)
    assert float(g['cells'][:, 0].abs().sum()) == 0.0 and float(g['cells'][:, 1:T].abs().sum()) > 0.0


def test_batch_noise_does_not_act(lstm_double):
    """a recurrent agent's exploration scales come without an act_batch: its cells stay untouched"""
    agent, _ = LC.make_agent(7, 3)
    s = agent.batch_noise(4)
    assert agent._batch_cells is None and tuple(s.shape) == (4, 1)
    agent.act_batch(torch.zeros(4, 7), eps=torch.zeros(4, 3))
    assert torch.equal(agent.batch_noise(4), s)


@pytest.mark.parametrize('case', ['two_layers', 'camera', 'not_persistent', 'no_entry'])
def test_what_takes_the_stem_path(lstm_double, case):
    from surreal_amd.env import SyntheticVecEnv
    from cpu_kernels import TorchCpuKernels
    n, D, A, T = 3, 5, 2, 4
    agent, _ = LC.make_agent(D, A, rnn_layer=2 if case == 'two_layers' else 1)
    venv = SyntheticVecEnv(n, D, A, episode_len=T, seeds=list(range(n)), device='cpu',
                           pixel=(1, 4, 4) if case == 'camera' else None,
                           kernels=TorchCpuKernels() if case == 'no_entry' else None)
    venv.persistent = case != 'not_persistent'
    assert not venv.can_rollout_into(agent)
    venv.start_rollout(T, info_width=2 * A)
    venv.rollout(agent, eps=torch.randn(T, n, A))
    assert lstm_double.lstm_launches == 0 and venv.slot == T
    assert float(venv.rolls['cells'][:, 1:T].abs().sum()) > 0.0


def test_rollout_into_the_replay_slots_gives_the_learners_onetime_infos(lstm_double):
    """stride == n_step == T: the one-launch kernel records straight into the FIFO's slots, the window's cells are the
    rollout's first state, and to_batch hands the learner what rollout -> emit_windows -> to_batch hands it"""
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd.replay import FIFOReplay
    n, D, A, T, HID = 4, 6, 2, 5, 10
    agent, (lc, ec, sc) = LC.make_agent(D, A, rnn_hidden=HID, T=T, n=n)
    eps = torch.randn(T, n, A, generator=torch.Generator().manual_seed(7))

    venv = SyntheticVecEnv(n, D, A, episode_len=T, seeds=list(range(n)), device='cpu')
    venv.start_rollout(T, info_width=2 * A)
    venv.rollout(agent, eps=eps)
    ref = venv.emit_windows(T, T)
    a = FIFOReplay(lc, ec, sc)
    a.insert_batch(ref)

    zc = SyntheticVecEnv(n, D, A, episode_len=T, seeds=list(range(n)), device='cpu')
    assert zc.can_rollout_into(agent)
    zc.start_rollout(T, info_width=2 * A)
    shp = zc.window_shapes(T, agent)
    assert shp['cells'] == (2, 1, HID) and 'cells' not in zc.window_shapes(T)
    b = FIFOReplay(lc, ec, sc)
    slots = b.reserve_batch(n, shp)
    slots['cells'].fill_(float('nan'))
    zc.rollout_into(agent, slots, eps=eps)
    b.commit_batch(n)
    assert lstm_double.lstm_launches == 2
    assert torch.equal(zc.state, venv.state) and zc.t == venv.t
    pa, pb = a.sample_batch(n), b.sample_batch(n, copy=False)
    assert set(pa) == set(pb) and 'cells' in pa
    for k in pa:
        assert_same(pb[k].reshape(pa[k].shape), pa[k], k)
    ba, bb = venv.to_batch(pa), zc.to_batch(pb)
    for x, y in zip(ba['onetime_infos'], bb['onetime_infos']):
        assert tuple(x.shape) == (n, 1, HID)
        assert_same(y.reshape(x.shape), x, 'onetime_infos')


def test_emit_windows_writes_the_reserved_cells():
    """emit_windows(out=...) fills a reserved 'cells' slot instead of allocating its own"""
    from surreal_amd.env import SyntheticVecEnv
    from cpu_kernels import TorchCpuKernels
    n, D, A, T = 2, 3, 1, 4
    venv = SyntheticVecEnv(n, D, A, episode_len=T, device='cpu', kernels=TorchCpuKernels())
    venv.start_rollout(T, info_width=2 * A)
    venv.rolls['cells'] = torch.randn(n, T + 1, 2, 1, 5)
    for t in range(T):
        venv.step(torch.zeros(n, A), pds=torch.zeros(n, 2 * A))
    f = lambda *s: torch.zeros(*s)  # noqa: E731
    out = {'obs': f(n, T, D), 'obs_next': f(n, 1, D), 'actions': f(n, T, A), 'rewards': f(n, T), 'dones': f(n, T),
           'pds': f(n, T, 2 * A), 'cells': torch.full((n, 2, 1, 5), float('nan'))}
    got = venv.emit_windows(T, T, out=out)
    assert got['cells'].data_ptr() == out['cells'].data_ptr()
    assert torch.equal(out['cells'], venv.rolls['cells'][:, 0])
