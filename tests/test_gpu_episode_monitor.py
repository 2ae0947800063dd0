"""GPU tier (-m gpu): the on-device episode monitor through the C ABI.

  * rollout(): the monitor equals the sequential fp64 sum of the same rollout's recorded rewards bit for bit, on the
    persistent kernel at 4, 8 and 16 actors per workgroup and on the three-launch path;
  * paths the existing tests hold bit-identical (4 against 8 actors per workgroup, the DDPG kernel's block sizes, split
    calls against one call, windowed PPO calls) leave bit-identical monitors;
  * paths the existing tests compare at a per-step atol leave episode sums within L x that atol for episodes of L
    steps, with equal step and episode counts.  (rollout against rollout_reference and the DDPG kernel against
    reference=True are such pairs: test_persistent_rollout_kernel and test_persistent_kernel_matches_two_launch_reference
    compare them at 2e-6 -- the 4-row and the 16-row MFMA loops sum a layer in different orders.)
  * a null monitor changes no byte of state, rolls or replay tables.
"""
import numpy as np
import pytest
import torch

import ddpg_pixel_rollout_cases as DPC
import ddpg_rollout_cases as DC
import episode_monitor_cases as EM
import helpers as H
import ppo_pixel_window_cases as PPC
import ppo_window_cases as PW
from test_gpu_kernels import _rollout_setup

pytestmark = pytest.mark.gpu

CAP = 4


@pytest.fixture
def K():
    from surreal_amd import kernels as KN
    return KN.default_kernels()


def assert_close_states(a, b, atol):
    """counts equal, sums within atol (an episode of L steps: L x the per-step atol of the paths' own test)"""
    for k in ('ep_steps', 'ep_count', 'done_steps'):
        assert torch.equal(a[k], b[k]), k
    for k in ('ep_reward', 'done_reward'):
        d = float((a[k] - b[k]).abs().max())
        print('episode monitor %s: max |difference| %.3g (bound %.3g)' % (k, d, atol))
        assert d <= atol, (k, d, atol)


# ---- rollout() -------------------------------------------------------------------------------------------------------

def _rollout(n, D, A, hidden, T, ep, how, apw=0, monitor=True, seed=11):
    """test_gpu_kernels._rollout_setup's run() with a monitor attached -> (recorded tables, monitor state or None)"""
    from surreal_amd.env import SyntheticVecEnv
    agent, _ = _rollout_setup(n, D, A, hidden, T, ep, True, False, seed=seed)
    eps = torch.randn(T, n, A, generator=torch.Generator().manual_seed(seed)).cuda()
    venv = SyntheticVecEnv(n, D, A, episode_len=ep, seeds=list(range(n)))
    mon = venv.attach_monitor(capacity=CAP) if monitor else None
    venv.T, venv.slot = T, 0
    f = lambda *s: torch.zeros(*s, device='cuda')  # noqa: E731
    venv.rolls = {'obs': f(n, T + 1, D), 'actions': f(n, T + 1, A), 'rewards': f(n, T + 1), 'dones': f(n, T + 1),
                  'pds': f(n, T + 1, 2 * A)}
    if how == 'reference':
        venv.rollout_reference(agent, eps)
    else:
        venv.persistent = how == 'persistent'
        venv.rollout(agent, eps=eps, actors_per_workgroup=apw)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in venv.rolls.items()}
    out['state'] = venv.state.cpu()
    return out, (EM.monitor_state(mon) if monitor else None)


SHAPES = [(48, 17, 6, (300, 200), 11, 4), (37, 29, 5, (40, 24), 9, 9)]     # (n, D, A, hidden, T, episode_len)


@pytest.mark.parametrize('how,apw', [('persistent', 4), ('persistent', 8), ('persistent', 16), ('layered', 0),
                                     ('reference', 0)])
@pytest.mark.parametrize('shape', SHAPES)
def test_rollout_monitor_is_the_sequential_sum_of_its_recorded_rewards(K, shape, how, apw):
    n, D, A, hidden, T, ep = shape
    rolls, got = _rollout(n, D, A, hidden, T, ep, how, apw)
    want = EM.sequential_sums(rolls['rewards'][:, :T].numpy(), 0, ep, CAP)
    EM.assert_states_equal(got, want)
    assert int(got['ep_count'][0]) == T // ep and int(got['ep_steps'][n - 1]) == T % ep


def test_rollout_paths_leave_agreeing_monitors(K):
    n, D, A, hidden, T, ep = SHAPES[0]
    _, four = _rollout(n, D, A, hidden, T, ep, 'persistent', 4)
    _, eight = _rollout(n, D, A, hidden, T, ep, 'persistent', 8)
    EM.assert_states_equal(four, eight)        # (test_persistent_rollout_kernel_row_group_counts_agree: the same bits)
    # test_persistent_rollout_kernel: persistent against rollout_reference and 16-actor blocks atol 2e-6 a step, against
    # the layered path 1e-5 a step
    assert_close_states(four, _rollout(n, D, A, hidden, T, ep, 'reference')[1], ep * 2e-6)
    assert_close_states(four, _rollout(n, D, A, hidden, T, ep, 'persistent', 16)[1], ep * 2e-6)
    assert_close_states(four, _rollout(n, D, A, hidden, T, ep, 'layered')[1], ep * 1e-5)


# ---- DDPG ------------------------------------------------------------------------------------------------------------

def _ddpg(n, hidden, L_, calls, monitor=True, camera=None, w3_scale=8.0, **kw):
    """ddpg_rollout_into over `calls` -> (ring, carried state, monitor state or None, what host_ring needs)"""
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    D, A = 17, 6
    run_kw = {k: kw.pop(k) for k in ('reference', 'actors_per_workgroup') if k in kw}
    steps = sum(calls)
    capacity = n * steps + 7
    if camera:
        lc, ec, sc = DPC.configs(D, A, n, camera[0], camera[1], hidden=hidden, feat=32, memory_size=capacity, **kw)
    else:
        lc, ec, sc = DC.configs(D, A, n, hidden=hidden, memory_size=capacity, **kw)
    agent = DC.make_agent(lc, ec, sc, w3_scale=w3_scale)
    eps_all = np.random.RandomState(3).randn(steps, n, A).astype(np.float32)
    venv = SyntheticVecEnv(n, D, A, episode_len=L_, device='cuda',
                           **(dict(pixel=camera[0], frame_stacks=camera[1]) if camera else {}))
    mon = venv.attach_monitor(capacity=CAP) if monitor else None
    replay = UniformReplay(lc, ec, sc)
    s0 = 0
    for T in calls:
        venv.ddpg_rollout_into(agent, replay, T, eps=torch.as_tensor(eps_all[s0:s0 + T]).cuda(), **run_kw)
        s0 += T
    torch.cuda.synchronize()
    carried = {k: venv._ddpg[k].cpu() for k in ('ou', 'carry_obs', 'carry_act', 'carry_rew')}
    carried['state'] = venv.state.cpu()
    ring = {k: torch.as_tensor(v) for k, v in H.device_ring(replay).items()}
    return ring, carried, (EM.monitor_state(mon) if monitor else None), (mon, agent, lc, ec, sc, eps_all, capacity)


def test_ddpg_bit_identical_paths_leave_bit_identical_monitors():
    kw = dict(n_step=3, noise_type='ou_noise')
    base = _ddpg(37, (64, 32), 9, (5, 7, 9), **kw)[2]
    for apw in (4, 8, 16):         # (test_persistent_kernel_matches_two_launch_reference: every block size, atol 0)
        EM.assert_states_equal(base, _ddpg(37, (64, 32), 9, (5, 7, 9), actors_per_workgroup=apw, **kw)[2])
    EM.assert_states_equal(base, _ddpg(37, (64, 32), 9, (21,), **kw)[2])                   # split calls == one call
    assert int(base['ep_count'][0]) == 2 and int(base['ep_steps'][36]) == 3
    # the two-launch reference: test_persistent_kernel_matches_two_launch_reference's 2e-6 a step
    assert_close_states(base, _ddpg(37, (64, 32), 9, (5, 7, 9), reference=True, **kw)[2], 9 * 2e-6)


def _assert_matches_host(mon, hosts, L_, atol):
    """polled device episodes against the host monitors': counts equal, an episode of L steps within L x atol (+ the
    half unit of the 6th digit both sides round to)"""
    mon.poll()
    for a, h in enumerate(hosts):
        assert mon.episode_steps[a] == h.episode_steps, a
        np.testing.assert_allclose(mon.episode_rewards[a], h.episode_rewards, atol=L_ * atol + 1e-6, rtol=0)
    rew, steps = mon.open_episodes()
    assert steps.tolist() == [len(h._rewards) for h in hosts]
    np.testing.assert_allclose(rew.numpy(), [float(sum(h._rewards)) for h in hosts], atol=L_ * atol, rtol=0)
    assert mon.num_episodes == sum(h.num_episodes for h in hosts) > 0


@pytest.mark.parametrize('layernorm,noise', [(False, 'normal'), (False, 'ou_noise'), (True, 'ou_noise')])
def test_ddpg_monitor_matches_the_host_monitors(layernorm, noise):
    """the persistent kernel and (a LayerNorm actor) the per-step path against the host path: test_gpu_ddpg_rollout's
    host_parity holds them at atol 1e-5 a step"""
    n, L_ = 4, 8
    *_, (mon, agent, lc, ec, sc, eps_all, capacity) = _ddpg(n, (64, 32), L_, (5, 6, 8), w3_scale=1.0, n_step=3,
                                                            noise_type=noise, layernorm=layernorm, theta=2.0, dt=0.05)
    with EM.host_monitors() as hosts:
        DC.host_ring(agent, lc, ec, sc, n, L_, eps_all, capacity)
    _assert_matches_host(mon, hosts, L_, 1e-5)


def test_ddpg_camera_monitor_matches_the_host_monitors():
    """test_gpu_ddpg_pixel_rollout.test_device_path_matches_host_path: atol 1e-5 a step"""
    n, L_, camera = 5, 9, ((3, 36, 36), 3)
    *_, (mon, agent, lc, ec, sc, eps_all, capacity) = _ddpg(n, (64, 32), L_, (5, 7, 9), camera=camera, w3_scale=1.0,
                                                            n_step=3, noise_type='ou_noise', theta=2.0, dt=0.05)
    with EM.host_monitors() as hosts:
        DPC.host_ring(agent, lc, ec, sc, n, L_, eps_all, capacity, *camera)
    _assert_matches_host(mon, hosts, L_, 1e-5)


# ---- windowed PPO ----------------------------------------------------------------------------------------------------

def _ppo(n, rnn_hidden, L_, chunks, monitor=True, camera=None, hosts=False, n_step=7, stride=3):
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd.replay import FIFOReplay
    D, A = 17, 6
    steps = sum(chunks)
    eps = torch.randn(steps, n, A, generator=torch.Generator().manual_seed(3))
    kw = dict(hidden=(64, 32), rnn_hidden=rnn_hidden, memory_size=n * steps + 7)
    make = (lambda: PPC.make_agent(D, A, n_step, stride, camera[0], camera[1], feat=32, final_scale=1.0, **kw)) \
        if camera else (lambda: PW.make_agent(D, A, n_step, stride, **kw))
    host = None
    if hosts:
        host_agent, cfg = make()
        with EM.host_monitors() as host:
            if camera:
                PPC.host_windows(host_agent, cfg, n, D, L_, steps, eps, camera[0], camera[1], device='cuda')
            else:
                PW.host_windows(host_agent, cfg, n, D, L_, steps, eps, device='cuda')
    agent, (lc, ec, sc) = make()
    venv = SyntheticVecEnv(n, D, A, episode_len=L_, seeds=list(range(n)),
                           **(dict(pixel=camera[0], frame_stacks=camera[1]) if camera else {}))
    mon = venv.attach_monitor(capacity=CAP) if monitor else None
    replay = FIFOReplay(lc, ec, sc)
    s0 = 0
    for T in chunks:
        venv.ppo_rollout_into(agent, replay, T, eps=eps[s0:s0 + T].cuda())
        s0 += T
    torch.cuda.synchronize()
    ring = {k: torch.as_tensor(v) for k, v in H.device_ring(replay).items()}
    carried = {k: v.cpu() for k, v in venv._ppo['carry'].items()}
    carried['state'] = venv.state.cpu()
    return ring, carried, (EM.monitor_state(mon) if monitor else None), mon, host


@pytest.mark.parametrize('rnn_hidden', [None, 12])
def test_ppo_window_split_calls_and_host_monitors(rnn_hidden):
    n, L_ = 37, 19
    _, _, split, mon, hosts = _ppo(n, rnn_hidden, L_, [5, 9, 8, 21], hosts=True)
    EM.assert_states_equal(split, _ppo(n, rnn_hidden, L_, [43])[2])                        # split calls == one call
    assert int(split['ep_count'][0]) == 2 and int(split['ep_steps'][n - 1]) == 5
    _assert_matches_host(mon, hosts, L_, 1e-5)        # (test_gpu_ppo_window_rollout.test_windows_match_the_host_wrapper)


@pytest.mark.parametrize('rnn_hidden', [None, 12])
def test_ppo_camera_monitor_matches_the_host_monitors(rnn_hidden):
    """test_gpu_ppo_pixel_window_rollout.test_device_path_matches_host_path: TOL 1e-5 a step"""
    n, L_, camera = 5, 19, ((3, 36, 36), 3)
    _, _, _, mon, hosts = _ppo(n, rnn_hidden, L_, [16, 5, 21], camera=camera, hosts=True)
    _assert_matches_host(mon, hosts, L_, 1e-5)


# ---- a null monitor changes nothing ----------------------------------------------------------------------------------

def _same_bytes(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = a[k].contiguous(), b[k].contiguous()
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k


@pytest.mark.parametrize('how,apw', [('persistent', 4), ('persistent', 16), ('layered', 0), ('reference', 0)])
def test_attached_monitor_changes_no_byte_of_a_rollout(K, how, apw):
    n, D, A, hidden, T, ep = SHAPES[0]
    with_mon, state = _rollout(n, D, A, hidden, T, ep, how, apw)
    without, none = _rollout(n, D, A, hidden, T, ep, how, apw, monitor=False)
    assert none is None and int(state['ep_count'].sum()) > 0
    _same_bytes(with_mon, without)


@pytest.mark.parametrize('family', ['ddpg', 'ddpg_step', 'ddpg_camera', 'ppo_window', 'ppo_lstm_window', 'ppo_camera'])
def test_attached_monitor_changes_no_byte_of_a_replay(family):
    def run(monitor):
        if family.startswith('ddpg'):
            return _ddpg(37, (64, 32), 9, (5, 7, 9), monitor=monitor, n_step=3, noise_type='ou_noise',
                         layernorm=family == 'ddpg_step',
                         camera=((3, 36, 36), 2) if family == 'ddpg_camera' else None)[:3]
        return _ppo(37, 12 if family == 'ppo_lstm_window' else None, 19, [5, 9, 8, 21], monitor=monitor,
                    camera=((3, 36, 36), 2) if family == 'ppo_camera' else None)[:3]
    (ring_a, carried_a, state), (ring_b, carried_b, none) = run(True), run(False)
    assert none is None and int(state['ep_count'].sum()) > 0
    _same_bytes(ring_a, ring_b)
    _same_bytes(carried_a, carried_b)
