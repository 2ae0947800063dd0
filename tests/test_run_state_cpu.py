"""CPU tier: the run-state container (surreal_amd/utils/run_state.py), every refusal of the holders' state_dict /
load_state_dict -- each raised before any tensor of the target is written --, and case 1 of run_state_cases.py (PPO,
plain MLP, `clip`, `reach`) uninterrupted against saved-and-resumed on the torch-CPU kernel doubles
(reach_resets_cpu_kernels.ResetsCpuKernels: ppo_rollout_into on `reach` with resets, noise and monitor, and the learner's
launches).  The doubles have no evaluation launch -- the records hold None there -- and draw from no noise stream: that loop
draws with torch.randn and its file carries the part 'torch_rng'."""
import pytest
import torch

import run_state_cases as RC
from run_state_cases import M
from surreal_amd.utils import run_state as RS


@pytest.fixture
def doubles():
    from surreal_amd import kernels as KN
    from reach_resets_cpu_kernels import ResetsCpuKernels
    K = ResetsCpuKernels()
    prev = KN.set_default_kernels(K, 'cpu')
    yield K
    KN.set_default_kernels(*prev)


# ---- the container -------------------------------------------------------------------------------------------------------

def _nested():
    import numpy as np
    return dict(a={'i64': torch.arange(5, dtype=torch.int64).view(1, 5), 'f64': torch.tensor([1.0, float('nan'), -0.0],
                                                                                           dtype=torch.float64),
                   'u8': torch.arange(6, dtype=torch.uint8).view(2, 3), 'i32': torch.tensor([-7], dtype=torch.int32),
                   'empty': torch.zeros(0, 4)},
                b=[1, 2.5, True, 'text', None, [3, {'deep': torch.ones(2, 2)}]],
                c={'array': np.arange(4, dtype=np.int32), 'scalar': np.float64(0.25), 'tuple': (1, 2), 7: 'an int key'})


def test_round_trip_keeps_dtypes_and_shapes(tmp_path):
    import numpy as np
    path = tmp_path / 'run.pt'
    parts = _nested()
    RS.save_run(path, **parts)
    got = RS.load_run(path)
    assert sorted(got) == ['a', 'b', 'c']
    for k, v in parts['a'].items():
        assert got['a'][k].dtype == v.dtype and got['a'][k].shape == v.shape
    want = dict(parts, c={'array': torch.from_numpy(np.arange(4, dtype=np.int32)), 'scalar': 0.25, 'tuple': [1, 2],
                          7: 'an int key'})
    assert not RC.diff(got, want)
    assert got['c']['array'].dtype == torch.int32 and isinstance(got['c']['scalar'], float)
    # a plain weights_only load: the file holds no code
    blob = torch.load(str(path), weights_only=True)
    assert blob['header'] == {'format': RS.FORMAT, 'version': RS.VERSION, 'parts': ['a', 'b', 'c']}


def test_a_saved_part_is_a_copy(tmp_path):
    t = torch.zeros(3)
    RS.save_run(tmp_path / 'run.pt', part={'t': t})
    host = RS.to_host({'t': t})
    t.fill_(1.0)
    assert RS.load_run(tmp_path / 'run.pt')['part']['t'].tolist() == [0.0] * 3 and host['t'].tolist() == [0.0] * 3


def test_what_a_part_may_not_hold(tmp_path):
    for bad in (object(), {1.5: 0}, {'f': lambda: 0}, torch.float32):
        with pytest.raises(TypeError):
            RS.save_run(tmp_path / 'run.pt', part={'x': bad})
    assert not (tmp_path / 'run.pt').exists()


def test_unknown_version_and_foreign_file(tmp_path):
    path = str(tmp_path / 'run.pt')
    RS.save_run(path, a={'x': 1})
    blob = torch.load(path, weights_only=True)
    blob['header']['version'] = RS.VERSION + 1
    torch.save(blob, path)
    with pytest.raises(ValueError, match='version'):
        RS.load_run(path)
    torch.save({'something': 'else'}, path)
    with pytest.raises(ValueError, match='not a run-state file'):
        RS.load_run(path)


def test_a_failed_save_leaves_the_previous_file(tmp_path, monkeypatch):
    path = tmp_path / 'run.pt'
    RS.save_run(path, a={'x': torch.arange(3)})
    real = torch.save

    def dies_midway(obj, f, *a, **kw):
        with open(f, 'wb') as fh:
            fh.write(b'half a file')
        raise OSError('disk full')
    monkeypatch.setattr(torch, 'save', dies_midway)
    with pytest.raises(OSError, match='disk full'):
        RS.save_run(path, a={'x': torch.arange(4)})
    monkeypatch.setattr(torch, 'save', real)
    assert [p.name for p in tmp_path.iterdir()] == ['run.pt']            # (no temporary file left behind)
    assert RS.load_run(path)['a']['x'].tolist() == [0, 1, 2]


def test_torch_rng_part(tmp_path):
    torch.manual_seed(5)
    torch.randn(3)
    RS.save_run(tmp_path / 'run.pt', torch_rng=RS.torch_rng_state())
    want = torch.randn(4)
    torch.manual_seed(99)
    RS.set_torch_rng_state(RS.load_run(tmp_path / 'run.pt')['torch_rng'])
    assert torch.equal(torch.randn(4), want)


# ---- the refusals: raised before anything of the target is written ---------------------------------------------------

def _env(K, n=RC.N_ACTORS, J=2, episode_len=RC.EPISODE, task='reach', seeds=None, D=None, A=None, **kw):
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    D, A = (3 * J, J) if D is None else (D, A)
    return SyntheticVecEnv(n, D, A, episode_len=episode_len, seeds=seeds or list(range(n)), device='cpu', kernels=K,
                           task=task, **kw)


def _stepped_env(K, agent, replay, steps=5, **kw):
    """an env with noise, resets and a monitor attached, some steps into an episode: open windows, counters moved (the
    doubles draw from no stream: the noise stream is attached after the steps, its counter set to them)"""
    venv = _env(K, **kw)
    venv.attach_monitor(capacity=4)
    venv.attach_resets(RC.RSEED)
    venv.reset()
    venv.ppo_rollout_into(agent, replay, steps)
    venv.attach_noise(RC.NSEED).step = steps
    return venv


def _ppo_parts():
    c = RC.BY_ID['ppo-mlp-clip-reach']
    from surreal_amd.agent import PPOAgent
    from surreal_amd.replay import FIFOReplay
    cfg = RC.ppo_configs(c)
    return cfg, PPOAgent(*cfg, agent_id=0, agent_mode='training'), FIFOReplay(*cfg)


def _raises_untouched(cls, call, holder_state, match=None):
    before = RS.to_host(holder_state())
    with pytest.raises(cls, match=match):
        call()
    assert not RC.diff(RS.to_host(holder_state()), before)


def test_env_refusals(doubles):
    K = doubles
    cfg, agent, replay = _ppo_parts()
    saved = RS.to_host(_stepped_env(K, agent, replay).state_dict())
    assert saved['ppo'] is not None and saved['t'] == 5 and saved['noise']['step'] == 5

    def target(**kw):
        torch.manual_seed(1)
        if 'J' in kw:                                               # (another D and A: the agent's policy does not fit it)
            venv = _env(K, **kw)
            venv.attach_monitor(capacity=4)
            venv.attach_resets(RC.RSEED)
            venv.reset()
            venv.attach_noise(RC.NSEED)
            return venv
        return _stepped_env(K, agent, type(replay)(*cfg), steps=7, **kw)        # (another state than the saved one)
    # the fingerprint: n, D / A, task, episode_len, init_state
    for kw, word in ((dict(n=5), 'n = '), (dict(J=1), 'D = '), (dict(episode_len=9), 'episode_len'),
                     (dict(seeds=[9, 8, 7, 6, 5, 4]), 'init_state')):
        venv = target(**kw)
        _raises_untouched(ValueError, lambda: venv.load_state_dict(saved), venv.state_dict, match=word)
    drift = _env(K, task='drift', D=6, A=2)
    drift.attach_monitor(capacity=4)
    drift.attach_noise(RC.NSEED)
    _raises_untouched(ValueError, lambda: drift.load_state_dict(saved), drift.state_dict, match='task')
    clocks = _env(K, episode_len=[RC.EPISODE] * RC.N_ACTORS)        # (per-actor clocks, though all of the saved length)
    _raises_untouched(ValueError, lambda: clocks.load_state_dict(saved), clocks.state_dict, match='episode_len')
    # something attached on one side only
    venv = target()
    venv.detach_noise()
    _raises_untouched(ValueError, lambda: venv.load_state_dict(saved), venv.state_dict, match='noise is attached')
    venv = target()
    venv.detach_resets()
    _raises_untouched(ValueError, lambda: venv.load_state_dict(saved), venv.state_dict, match='resets is attached')
    venv = target()
    venv.detach_monitor()
    _raises_untouched(ValueError, lambda: venv.load_state_dict(saved), venv.state_dict, match='monitor is attached')
    bare = dict(saved, monitor=None)
    venv = target()
    _raises_untouched(ValueError, lambda: venv.load_state_dict(bare), venv.state_dict, match='this env only')
    # an attachment's own check: another stream seed, another ring capacity
    venv = target()
    venv.noise.seed += 1
    _raises_untouched(ValueError, lambda: venv.load_state_dict(saved), venv.state_dict, match='DeviceNoise')
    venv = target()
    venv.resets.seed += 1
    _raises_untouched(ValueError, lambda: venv.load_state_dict(saved), venv.state_dict, match='DeviceResets')
    venv = target()
    venv.detach_monitor()
    venv.attach_monitor(capacity=5)
    _raises_untouched(ValueError, lambda: venv.load_state_dict(saved), venv.state_dict, match='DeviceEpisodeMonitor')
    # and the state that fits loads
    venv = target()
    venv.load_state_dict(saved)
    assert not RC.diff(RS.to_host(venv.state_dict()), saved)


def test_camera_env_is_refused(doubles):
    cam = _env(doubles, task='drift', D=6, A=2, pixel=(3, 8, 8))
    with pytest.raises(NotImplementedError, match='camera'):
        cam.state_dict()
    with pytest.raises(NotImplementedError, match='camera'):
        cam.load_state_dict({})


def test_replay_refusals(doubles):
    from surreal_amd.replay import FIFOReplay, UniformReplay
    cfg, agent, replay = _ppo_parts()
    _stepped_env(doubles, agent, replay)
    saved = RS.to_host(replay.state_dict())
    assert saved['tables'] is not None and saved['cursors']['_count'] > 0

    def filled(memory_size=None, n_step=None):
        c = RC.ppo_configs(RC.BY_ID['ppo-mlp-clip-reach'])
        if memory_size:
            c[0].replay.memory_size = memory_size
        if n_step:
            c[0].algo.n_step = n_step
        ag = type(agent)(*c, agent_id=0, agent_mode='training')
        r = FIFOReplay(*c)
        _stepped_env(doubles, ag, r, steps=8)
        return r
    r = filled(memory_size=65)
    _raises_untouched(ValueError, lambda: r.load_state_dict(saved), r.state_dict, match='memory_size')
    r = filled(n_step=3)                                     # (another field shape: windows of 3 steps)
    _raises_untouched(ValueError, lambda: r.load_state_dict(saved), r.state_dict, match='do not match')
    r = filled()
    r.insert(('an experience of the host tier',))
    with pytest.raises(ValueError, match='host tier'):
        r.load_state_dict(saved)
    with pytest.raises(ValueError, match='host tier'):
        r.state_dict()
    r._memory.clear()
    tables = {k: t.data.data_ptr() for k, t in r._tables.items()}
    r.load_state_dict(saved)                                 # tables that exist: in place
    assert {k: t.data.data_ptr() for k, t in r._tables.items()} == tables
    assert not RC.diff(RS.to_host(r.state_dict()), saved)
    empty = FIFOReplay(*cfg)                                 # none yet: reserved with the saved shapes and dtypes
    empty.load_state_dict(saved)
    assert not RC.diff(RS.to_host(empty.state_dict()), saved) and len(empty) == len(replay)
    other = UniformReplay(*RC.ddpg_configs(RC.BY_ID['ddpg-ou-reach']))
    _raises_untouched(ValueError, lambda: other.load_state_dict(saved), other.state_dict, match='FIFOReplay')
    lc, ec, sc = RC.ddpg_configs(RC.BY_ID['ddpg-ou-reach'])
    lc.replay.device_frame_pool = True
    pool = UniformReplay(lc, ec, sc)
    for call in (pool.state_dict, lambda: pool.load_state_dict(saved)):
        with pytest.raises(NotImplementedError, match='frame-pool'):
            call()


def test_uniform_replay_round_trip(doubles):
    from surreal_amd.replay import UniformReplay
    cfg = RC.ddpg_configs(RC.BY_ID['ddpg-ou-reach'])
    r = UniformReplay(*cfg)
    g = torch.Generator().manual_seed(3)
    for rows in (40, 30):                                    # (the ring wraps: 70 rows into 64)
        r.insert_batch({'obs': torch.randn(rows, 6, generator=g), 'rewards': torch.randn(rows, generator=g)})
    r.sample_batch(16)
    saved = RS.to_host(r.state_dict())
    assert saved['cursors'] == {'_dev_len': 64, '_dev_next': 6, '_draws': 16, 'seed': r.seed}
    want = r.sample_batch(16)
    fresh = UniformReplay(*cfg)
    fresh.load_state_dict(saved)
    got = fresh.sample_batch(16)
    assert not RC.diff(got, want) and fresh.cumulative_sampled_count == r.cumulative_sampled_count == 32


def test_learner_and_agent_refusals(doubles):
    from surreal_amd.learner import PPOLearner
    from surreal_amd.learner.ddpg import DDPGLearner
    cfg, agent, _ = _ppo_parts()
    for L in (PPOLearner(*cfg), DDPGLearner(*RC.ddpg_configs(RC.BY_ID['ddpg-ou-reach']))):
        saved = RS.to_host(L.train_state_dict())
        L.world_size = 2
        with pytest.raises(NotImplementedError, match='2 ranks'):
            L.train_state_dict()
        before = RS.to_host(L._train_tensors())
        with pytest.raises(NotImplementedError, match='2 ranks'):
            L.load_train_state_dict(saved)
        L.world_size = 1
        wrong = dict(saved, tensors={k: (v[:-1] if k.endswith('exp_avg') and v.dim() == 1 else v)
                                     for k, v in saved['tensors'].items()})
        with pytest.raises(ValueError, match='exp_avg'):
            L.load_train_state_dict(wrong)
        assert not RC.diff(RS.to_host(L._train_tensors()), before)
        L.load_train_state_dict(saved)
    adapt = RC.ppo_configs(RC.BY_ID['ppo-mlp-clip-reach'])
    adapt[0].algo.ppo_mode = 'adapt'
    with pytest.raises(ValueError, match='mode'):
        PPOLearner(*adapt).load_train_state_dict(RS.to_host(PPOLearner(*cfg).train_state_dict()))
    # an agent of another architecture; a camera agent
    saved = RS.to_host(agent.state_dict())
    wide = RC.ppo_configs(RC.BY_ID['ppo-mlp-clip-reach'])
    wide[0].model.actor_fc_hidden_sizes = wide[0].model.critic_fc_hidden_sizes = [32, 36]
    other = type(agent)(*wide, agent_id=0, agent_mode='training')
    _raises_untouched(ValueError, lambda: other.load_state_dict(saved), other.state_dict, match='flat')
    agent.model.if_pixel = True
    try:
        for call in (agent.state_dict, lambda: agent.load_state_dict(saved)):
            with pytest.raises(NotImplementedError, match='camera agent'):
                call()
    finally:
        agent.model.if_pixel = False
    agent.load_state_dict(saved)


def test_ddpg_restore_path_invalidates_the_packed_rows(doubles):
    """invalidate_packed() and the existing restore path (critic_step set from outside -> ws.dev_step != critic_step)"""
    from surreal_amd.learner.ddpg import DDPGLearner
    L = DDPGLearner(*RC.ddpg_configs(RC.BY_ID['ddpg-ou-reach']))
    L.invalidate_packed()                                    # (no workspace yet: nothing to do)
    B, D, A = 16, 6, 2
    g = torch.Generator().manual_seed(0)
    batch = lambda: {'obs': {'low_dim': {'flat_inputs': torch.randn(B, D, generator=g)}},  # noqa: E731
                     'obs_next': {'low_dim': {'flat_inputs': torch.randn(B, D, generator=g)}},
                     'actions': torch.rand(B, A, generator=g) * 2 - 1, 'rewards': torch.randn(B, 1, generator=g),
                     'dones': torch.zeros(B, 1)}
    L.learn(batch())
    ws = L._ws
    if getattr(ws, 'rows_args', None) is not None:
        assert ws.rows_versions == L._rows_versions()
    L.invalidate_packed()
    assert ws.rows_versions is None
    L.learn(batch())
    saved = RS.to_host(L.train_state_dict())
    L.learn(batch())
    L.load_train_state_dict(saved)
    assert int(ws.step) == L.critic_step == ws.dev_step == 2 and ws.rows_versions is None and L._ws is ws


# ---- case 1, uninterrupted against saved and resumed, on the doubles -----------------------------------------------------

def test_case_1_resumes_on_the_doubles(doubles, tmp_path):
    c = RC.CASES[0]
    want = RC.Loop(c, RC.SEED_A, device='cpu', kernels=doubles, stream_noise=False).run(2 * M)
    assert RC.learned(want) and all(r['eval'] is None for r in want)
    again = RC.Loop(c, RC.SEED_A, device='cpu', kernels=doubles, stream_noise=False).run(2 * M)
    for k in range(2 * M):
        RC.assert_same(again[k], want[k], 'chunk %d of a second uninterrupted run' % (k + 1))
    first = RC.Loop(c, RC.SEED_A, device='cpu', kernels=doubles, stream_noise=False)
    head = first.run(M)
    first.save(tmp_path / 'run.pt')
    fresh = RC.Loop(c, RC.SEED_B, device='cpu', kernels=doubles, stream_noise=False)
    built_a = RC.Loop(c, RC.SEED_A, device='cpu', kernels=doubles, stream_noise=False).learner.train_state_dict()['tensors']
    assert RC.diff(RC.parameters(RS.to_host(fresh.learner.train_state_dict()['tensors'])), RC.parameters(RS.to_host(built_a)))
    fresh.load(tmp_path / 'run.pt')
    got = fresh.run(M)
    for k in range(M):
        RC.assert_same(got[k], want[M + k], 'chunk %d after the resume' % (M + k + 1))
    # and in place, on the objects that ran on
    first.run(M)
    first.load(tmp_path / 'run.pt')
    got = first.run(M)
    for k in range(M):
        RC.assert_same(got[k], want[M + k], 'chunk %d after the in-place restore' % (M + k + 1))
