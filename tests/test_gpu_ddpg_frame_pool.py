"""GPU tier (-m gpu): the frame-pool layout of the device DDPG replay (replay.device_frame_pool) on the HIP path, against
the stacked layout that exists today -- the same rollout with the same eps into a stacked replay and into a pool replay:

  * every live ring row through sample_batch(indices=rows): uint8 frames byte for byte, low-dimensional fields bit for
    bit; the live set from a plain Python simulation of the counters (ddpg_frame_pool_cases.simulate), len(replay)
    equal to it; the final acting observation, state and the episode monitor's poll();
  * one call of T steps leaves the bytes of several;
  * drawn sampling: sample_batch(B) == sample_batch(B, indices=sample_indices(B)) from the same draw offset, all rows
    live, and -- after rows have retired -- equal to the stacked twin's rows (no overwritten frame is read);
  * the learner: staging_fields + sample_batch(out=) + learn() from the pool replay == from the stacked replay;
  * the refusals and the derived memory.

The stacked twin takes the same steps in calls of memory_size // n steps: a call into the stacked layout may not go round
the ring (ddpg_rollout_into refuses it), the frame-pool route -- a launch per step -- may.
"""
import collections

import numpy as np
import pytest
import torch

import ddpg_frame_pool_cases as FC
import ddpg_pixel_rollout_cases as PC

pytestmark = pytest.mark.gpu
N_, D_, A_ = FC.N_, FC.D_, FC.A_


@pytest.mark.parametrize('pixel,N,S,episode_len', FC.TWIN_CASES)
def test_twin_rollout(pixel, N, S, episode_len):
    """n = 5, D = 7, A = 3, T = 23 in calls of 10 + 13, memory_size = 4 n with the default P: ring and pool wrap"""
    _, live = FC.check_twin(None, 'cuda', pixel, N, S, episode_len, monitor=True)
    assert live or N > episode_len - 1


@pytest.mark.parametrize('pixel', [(3, 8, 8), (3, 6, 7)])
def test_twin_rollout_smallest_pool(pixel):
    """device_frame_pool_steps = N + S + 1"""
    _, live = FC.check_twin(None, 'cuda', pixel, 3, 3, 9, pool_steps=7, monitor=True)
    assert 0 < len(live) < 4 * N_


@pytest.mark.parametrize('pixel', [(3, 8, 8), (3, 6, 7)])
def test_one_call_or_several(pixel):
    one = FC.twin(None, 'cuda', N_, D_, A_, pixel, 3, 3, 9, (23,), 4 * N_)['pool'][1]
    many = FC.twin(None, 'cuda', N_, D_, A_, pixel, 3, 3, 9, (3, 4, 1, 9, 6), 4 * N_)['pool'][1]
    assert len(one) == len(many) and one._dev_next == many._dev_next
    for k in ('pool', 'frame_next', 'frame_first', 'frame_actor'):
        assert torch.equal(one.frame_pool[k], many.frame_pool[k]), k
    for k in one._tables:
        assert torch.equal(one._tables[k].data, many._tables[k].data), k


@pytest.mark.parametrize('pixel,pool_steps', [((3, 8, 8), None), ((3, 6, 7), 8)])
def test_drawn_sampling(pixel, pool_steps):
    t = FC.twin(None, 'cuda', N_, D_, A_, pixel, 3, 3, 9, (10, 13), 4 * N_, pool_steps=pool_steps)
    replay, stacked = t['pool'][1], t['stacked'][1]
    live, _, _ = FC.simulate(N_, 3, 3, [9], 23, 4 * N_, replay.frame_pool['pool'].shape[1])
    assert len(replay) == len(live) and (pool_steps is None or len(live) < 4 * N_)     # (P = 8: rows have retired)
    B = 96
    draws = replay._draws
    idx = replay.sample_indices(B)
    assert set(idx.tolist()) <= set(live) and len(set(idx.tolist())) > len(live) // 2
    replay._draws = draws                        # the sample below draws the same Philox counters again
    idx_out = torch.empty(B, dtype=torch.int64, device='cuda')
    got = replay.sample_batch(B)
    assert replay._draws == draws + B
    again = replay.sample_batch(B, indices=idx)
    want = stacked.sample_batch(B, indices=idx)
    for k in want:
        assert torch.equal(got[k], again[k]), k
        assert torch.equal(got[k], want[k]), k
    # idx_out of the launch itself: the rows it drew
    from surreal_amd import kernels as KN
    names = list(replay._tables)
    outs = [torch.empty(B, replay._tables[k].width, device='cuda') for k in names]
    pix = [torch.empty(B, 3 * int(np.prod(pixel)), device='cuda', dtype=torch.uint8) for _ in range(2)]
    KN.default_kernels().uniform_gather_pool([replay._tables[k].data for k in names], outs, replay.frame_pool, pix[0],
                                             pix[1], len(replay), replay.seed, draws, replay._live_base(),
                                             idx_out=idx_out)
    assert torch.equal(idx_out, idx) and torch.equal(pix[0].view(want['pixel'].shape), want['pixel'])


def test_learner_from_the_pool_replay():
    """one iteration at batch 8 on the same injected indices: bit-equal statistics and parameters"""
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.learner.ddpg import DDPGLearner
    from surreal_amd.replay import UniformReplay
    n, D, A, B, pixel, S, N = 8, 17, 6, 8, (3, 36, 36), 3, 3
    kw = dict(hidden=(64, 32), feat=32, memory_size=128, n_step=N, noise_type='ou_noise')
    cfgs = {'stacked': PC.configs(D, A, n, pixel, S, **kw), 'pool': PC.configs(D, A, n, pixel, S, **kw)}
    cfgs['pool'][0].replay.device_frame_pool = True
    for c in cfgs.values():
        c[0].replay.batch_size = B
    agent = PC.DC.make_agent(*cfgs['stacked'], w3_scale=1.0)
    eps = torch.randn(12, n, A, generator=torch.Generator().manual_seed(1)).cuda()
    replays, learners = {}, {}
    for name, c in cfgs.items():
        venv = SyntheticVecEnv(n, D, A, episode_len=20, device='cuda', pixel=pixel, frame_stacks=S)
        replays[name] = UniformReplay(*c)
        for s0 in (0, 6):
            venv.ddpg_rollout_into(agent, replays[name], 6, eps=eps[s0:s0 + 6].contiguous())
        learners[name] = DDPGLearner(*c)
    assert len(replays['pool']) == len(replays['stacked']) == n * 10
    learners['pool'].model.load_state_dict(learners['stacked'].model.state_dict())
    learners['pool'].model_target.load_state_dict(learners['stacked'].model_target.state_dict())
    idx = torch.as_tensor([3, 79, 0, 41, 41, 17, 60, 8])
    stats = {}
    for name in ('stacked', 'pool'):
        stage = learners[name].staging_fields(B)
        f = replays[name].sample_batch(B, indices=idx, out=stage)
        assert f['pixel'].data_ptr() == stage['pixel'].data_ptr() and f['pixel'].dtype == torch.uint8
        obs = collections.OrderedDict(pixel={'camera0': f['pixel']}, low_dim={'flat_inputs': f['obs']})
        nxt = collections.OrderedDict(pixel={'camera0': f['pixel_next']}, low_dim={'flat_inputs': f['obs_next']})
        stats[name] = dict(learners[name].learn({'obs': obs, 'obs_next': nxt, 'actions': f['actions'],
                                                 'rewards': f['rewards'].view(B, 1), 'dones': f['dones'].view(B, 1)}))
    assert stats['pool'] == stats['stacked'] and all(np.isfinite(v) for v in stats['pool'].values())
    m0, m1 = learners['stacked'].model, learners['pool'].model
    for a, b in ((m0.actor_flat, m1.actor_flat), (m0.critic_flat, m1.critic_flat),
                 (m0.perception_flat, m1.perception_flat)):
        assert torch.equal(a, b)


def test_refusals_and_derived_memory():
    from surreal_amd import _lib as L
    from surreal_amd import kernels as KN
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    pixel, N, S, cap = (3, 8, 8), 3, 3, 4 * N_
    t = FC.twin(None, 'cuda', N_, D_, A_, pixel, N, S, 9, (23,), cap, pool_steps=8)
    replay, stacked = t['pool'][1], t['stacked'][1]
    F = 3 * 8 * 8
    assert replay.camera_bytes() == 8 * N_ * F + cap * (2 * 8 + 4)      # P n F, two int64 and the int32 actor per row
    assert stacked.camera_bytes() == cap * 2 * S * F
    live = len(replay)
    assert 0 < live < cap
    dead = (replay._dev_next - 1 - live) % cap
    with pytest.raises(ValueError, match='live'):
        replay.sample_batch(2, indices=torch.as_tensor([(replay._dev_next - 1) % cap, dead]).cuda())
    with pytest.raises(ValueError, match='frame-pool'):
        replay.insert_batch(stacked.sample_batch(4, indices=[0, 1, 2, 3]))
    lc, ec, sc = FC.pool_configs(D_, A_, N_, pixel, S, pool_steps=N + S, memory_size=cap, n_step=N)
    venv = SyntheticVecEnv(N_, D_, A_, episode_len=9, device='cuda', pixel=pixel, frame_stacks=S)
    with pytest.raises(ValueError, match='device_frame_pool_steps'):
        venv.ddpg_rollout_into(PC.DC.make_agent(lc, ec, sc), UniformReplay(lc, ec, sc), 2)
    # the ABI: P < N + S + 1 is SMX_E_SHAPE (-2) before any launch
    fp = dict(replay.frame_pool, pool=replay.frame_pool['pool'][:, :N + S].contiguous())
    names = list(replay._tables)
    outs = [torch.empty(4, replay._tables[k].width, device='cuda') for k in names]
    pix = [torch.empty(4, S * F, device='cuda', dtype=torch.uint8) for _ in range(2)]
    with pytest.raises(L.SmxError, match='rc=-2'):
        KN.default_kernels().uniform_gather_pool([replay._tables[k].data for k in names], outs, fp, pix[0], pix[1], live,
                                                 1, 0, 0)


# ---- the recorder of host-stepped environments ----------------------------------------------------------------------------
REC_LENGTHS = [4, 6, 9, 5, 7]                    # every actor cycles through them from its own offset: diverging clocks


@pytest.mark.parametrize('pixel,N,S,pool_steps', [((1, 4, 4), 3, 3, None), ((3, 5, 3), 1, 3, None),
                                                  ((2, 4, 6), 4, 2, None), ((1, 4, 4), 3, 3, 7), ((3, 5, 3), 3, 1, 5)])
def test_recorder_into_a_pool_replay(pixel, N, S, pool_steps):
    """F = 16: the 16-byte path, 45: the byte path, 48; the default pool and the smallest one"""
    from surreal_amd.env import DeviceEpisodeMonitor
    mon = DeviceEpisodeMonitor(N_, 32, 'cuda')
    FC.check_recorder_twin(pixel, N, S, REC_LENGTHS, pool_steps)
    FC.check_recorder_twin(pixel, N, S, REC_LENGTHS, pool_steps, monitor=mon, stacked_too=False)
    assert mon.total_steps == N_ * 40


def test_host_vec_env_into_a_pool_replay():
    """HostVecEnv.run_ddpg over scripted camera environments on diverging clocks, twice with the same seeds: into a
    stacked replay and into a pool replay; rec.observation, run_ddpg and to_ddpg_batch as the caller knows them"""
    import pixel_recorder_cases as PR
    from surreal_amd.env import HostVecEnv, DeviceNStepRecorder
    from surreal_amd.replay import UniformReplay
    n, Dv, Av, N, S, T, pixel, cap = 5, 17, 6, 3, 2, 40, (1, 36, 36), 20
    replays, dones, acting = {}, {}, {}
    for name in ('stacked', 'pool'):
        lc, ec, sc = PC.configs(Dv, Av, n, pixel, S, hidden=(64, 32), feat=32, memory_size=cap, n_step=N)
        lc.replay.device_frame_pool = name == 'pool'
        agent = PC.DC.make_agent(lc, ec, sc, w3_scale=1.0)
        replays[name] = UniformReplay(lc, ec, sc)
        venv = HostVecEnv([PR.ScriptedCameraEnv(40 + a, REC_LENGTHS, Dv, pixel, rotation=a) for a in range(n)],
                          frame_stacks=S)
        rec = DeviceNStepRecorder(n, Dv, Av, N, lc.algo.gamma, pixel=pixel, frame_stacks=S)
        log, inner = [], rec.record
        rec.record = lambda replay, actions, rewards, d, *a, _l=log, _r=inner, **kw: (
            _l.append(np.asarray(d).astype(bool).copy()), _r(replay, actions, rewards, d, *a, **kw))[1]
        torch.manual_seed(7)
        written = venv.run_ddpg(agent, rec, replays[name], T, sigmas=agent.batch_sigmas(n).float())
        dones[name], acting[name] = np.stack(log), rec.observation['pixel']['camera0'].clone()
        assert written == replays[name].cumulative_collected_count > cap
    assert np.array_equal(dones['pool'], dones['stacked']) and torch.equal(acting['pool'], acting['stacked'])
    pool = replays['pool']
    live, total = FC.simulate_recorder(dones['pool'], N, S, cap, pool.frame_pool['pool'].shape[1])
    assert len(pool) == len(live) > 0 and total == pool.cumulative_collected_count
    FC.assert_live_rows_equal({'pool': (None, pool), 'stacked': (None, replays['stacked'])}, live)
    f = pool.sample_batch(8)
    batch = venv.to_ddpg_batch(f)
    assert batch['obs']['pixel']['camera0'].dtype == torch.uint8
    assert tuple(batch['obs']['pixel']['camera0'].shape) == (8, S, 36, 36)


def test_equal_clocks_give_the_synthetic_routes_samples():
    """every actor on the same clock: the n_step-1 step stream of a camera SyntheticVecEnv recorded at n_step 3 into a
    pool replay gives the samples ddpg_rollout_into leaves in a pool replay at n_step 3"""
    import test_gpu_pixel_recorder as TR
    from surreal_amd.env import DeviceNStepRecorder, SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    n, Dv, Av, N, L_, pixel, S = 6, 11, 3, 3, 9, (3, 36, 36), 2
    T = 2 * L_ + 5
    eps = torch.randn(T, n, Av, generator=torch.Generator().manual_seed(4)).cuda()
    out = {}
    for ns, on in ((1, False), (N, True)):
        lc, ec, sc = PC.configs(Dv, Av, n, pixel, S, hidden=(64, 32), feat=32, memory_size=4096, n_step=ns, gamma=0.99,
                                noise_type='normal')
        lc.replay.device_frame_pool = on
        agent = PC.DC.make_agent(lc, ec, sc, w3_scale=1.0)
        venv = SyntheticVecEnv(n, Dv, Av, episode_len=L_, device='cuda', pixel=pixel, frame_stacks=S)
        replay = UniformReplay(lc, ec, sc)
        written = venv.ddpg_rollout_into(agent, replay, T, eps=eps)
        out[ns] = (replay, written, venv.init_state.clone(), (lc, ec, sc))
    stream, written, init_state, _ = out[1]
    steps = {k: t.data[:written].clone() for k, t in stream._tables.items()}
    want, rows_want, _, cfg = out[N]
    replay = UniformReplay(*cfg)
    rec = DeviceNStepRecorder(n, Dv, Av, N, 0.99, pixel=pixel, frame_stacks=S)
    rec.begin(init_state, TR._frames(rec.K, init_state[:, 0], 0, pixel))
    total = []
    TR._replay_stream(steps, n, L_, T, pixel, init_state, lambda s, f, done, fn, fr: total.append(
        rec.record(replay, f['actions'], f['rewards'].reshape(n), done, f['obs_next'], init_state, frames_next=fn,
                   frames_reset=fr)))
    assert sum(total) == rows_want == len(replay) == len(want) > 0
    FC.assert_live_rows_equal({'pool': (None, replay), 'stacked': (None, want)}, range(rows_want))
