"""CPU tier: episode clocks per actor in the one-launch rollouts -- the closed forms of env/actor_clocks.py against the
brute-force row table, the two new structs against the header, the refusals of the three new entry points (before any
launch) and of SyntheticVecEnv, and the per-actor calls through the torch-CPU doubles against n host chains, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import actor_clock_cases as CC
import ddpg_rollout_cases as DC
import ppo_window_cases as PW
import test_ppo_window_abi as WABI
from helpers import _offsets
from surreal_amd.env import actor_clocks as AC

SMX_OK, SMX_E_NULL, SMX_E_SHAPE = 0, -1, -2


# ---- the closed forms ---------------------------------------------------------------------------------------------

def _random_cases(count, seed=0):
    rs = np.random.RandomState(seed)
    for i in range(count):
        n = int(rs.randint(1, 9))
        N = int(rs.randint(1, 9))
        adv = (1, N, int(rs.randint(1, N + 1)))[i % 3]
        L = rs.randint(1, 21, size=n)
        L[rs.rand(n) < 0.15] = 1
        L[rs.rand(n) < 0.15] = N
        if N > 1:
            L[rs.rand(n) < 0.15] = rs.randint(1, N)
        t = (rs.rand(n) * L).astype(np.int64)
        t[rs.rand(n) < 0.2] = 0
        last = rs.rand(n) < 0.2
        t[last] = L[last] - 1
        steps = 1 if i % 7 == 0 else int(rs.randint(1, 60))
        yield t, L, steps, N, adv


def test_closed_forms_equal_the_walk():
    seen = set()
    for t, L, steps, N, adv in _random_cases(3000):
        table, rows = AC.row_table(t, L, steps, N, adv)
        per = AC.closings(t, L, steps, N, adv)
        assert np.array_equal(per, (table >= 0).sum(axis=0)) and int(per.sum()) == rows
        assert np.array_equal(np.sort(table[table >= 0]), np.arange(rows))
        assert np.array_equal(table[table >= 0], np.arange(rows))          # (step, actor) order: row-major ascending
        tau = t.copy()
        for _ in range(steps):
            tau = np.where(tau + 1 >= L, 0, tau + 1)
        assert np.array_equal(AC.after(t, L, steps), tau) and AC.after(t, L, steps).dtype == np.int32
        seen |= {('L1', bool((L == 1).any())), ('L<N', bool((L < N).any())), ('L==N', bool((L == N).any())),
                 ('t=L-1', bool((t == L - 1).any())), ('steps1', steps == 1), ('adv1', adv == 1), ('advN', adv == N)}
    assert all((k, True) in seen for k in ('L1', 'L<N', 'L==N', 't=L-1', 'steps1', 'adv1', 'advN'))


def test_base_shape_counts():
    steps = sum(CC.CHUNKS)
    table, rows = AC.row_table(np.zeros(6, int), CC.LENS, steps, 4, 3)
    per = (table >= 0).sum(axis=0)
    assert rows == 22 and per[4] == 0
    mixed = sum(0 < (table[s] >= 0).sum() < 6 for s in range(steps))
    assert mixed == 12
    # actor 2 (episodes of 4 steps) closes only on its terminal steps
    assert all((s + 1) % 4 == 0 for s in np.nonzero(table[:, 2] >= 0)[0])
    table, rows = AC.row_table(np.zeros(6, int), CC.LENS, steps, CC.DDPG_N_STEP, 1)
    assert rows == 70 and sum(0 < (table[s] >= 0).sum() < 6 for s in range(steps)) == 17
    # the reference-sized case of the GPU tier
    big = (26, 40, 25, 31, 24, 33, 50, 27, 29)
    per = AC.closings(np.zeros(9, int), big, 60, 25, 20)
    assert int(per.sum()) == 15 and per[4] == 0


def test_equal_clocks_give_the_shared_rows():
    n, Lr, steps, N, adv = 5, 9, 31, 4, 3
    table, rows = AC.row_table(np.full(n, 2), [Lr] * n, steps, N, adv)
    k, t = 0, 2
    for s in range(steps):
        j = t + 1 - N
        if j >= 0 and j % adv == 0:
            assert np.array_equal(table[s], k * n + np.arange(n))
            k += 1
        else:
            assert (table[s] == -1).all()
        t = 0 if t + 1 >= Lr else t + 1
    assert rows == k * n


def test_bad_clocks_are_refused():
    for t, L in (([0, 3], [2, 3]), ([0, -1], [2, 3]), ([0, 0], [2, 0]), ([0], [2, 3])):
        with pytest.raises(ValueError):
            AC.closings(t, L, 5, 2, 1)


# ---- the C ABI ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cname,mirror', [('struct smx_actor_clock_rows', 'ActorClockRows'),
                                          ('struct smx_actor_clocks', 'ActorClocks')])
def test_structs_match_the_ctypes_mirrors(tmp_path, cname, mirror):
    from surreal_amd import _lib as L
    cls = getattr(L, mirror)
    got = _offsets(tmp_path, cname, cls)
    assert got['sizeof'] == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert got[fname] == getattr(cls, fname).offset, fname
    for sym in ('smx_actor_clock_rows_i32', 'smx_synth_ppo_window_rollout_clocks_f32', 'smx_synth_ddpg_rollout_clocks_f32'):
        assert sym in L.EXPORTED_SYMBOLS


FAKE = ctypes.c_void_p(4096)


def _rows_args(n=5, steps=7, n_step=4, advance=3, t=None, lens=None):
    from surreal_amd import _lib as L
    p = L.ActorClockRows()
    p.n, p.steps, p.n_step, p.advance = n, steps, n_step, advance
    p.t = p.episode_len = p.row_off = FAKE
    keep = [np.ascontiguousarray(x, dtype=np.int32) for x in (t, lens) if x is not None]
    if t is not None:
        p.t_host = keep[0].ctypes.data
    if lens is not None:
        p.episode_len_host = keep[-1].ctypes.data
    return p, keep


@pytest.mark.parametrize('change,want', [
    (dict(n=0), SMX_E_SHAPE),
    (dict(steps=0), SMX_E_SHAPE),
    (dict(n_step=0), SMX_E_SHAPE),
    (dict(advance=0), SMX_E_SHAPE),
    (dict(advance=5), SMX_E_SHAPE),
    (dict(n=1 << 16, steps=1 << 15), SMX_E_SHAPE),                                     # n * steps = 2^31
    (dict(t=[0, 1, 2, 3, 4], lens=[1, 2, 3, 4, 4]), SMX_E_SHAPE),                      # t == L
    (dict(t=[0, 1, -1, 3, 3], lens=[1, 2, 3, 4, 4]), SMX_E_SHAPE),
    (dict(t=[0, 0, 0, 0, 0], lens=[1, 2, 0, 4, 4]), SMX_E_SHAPE),
    (dict(t=[0, 0, -2, 0, 0]), SMX_E_SHAPE),                                           # (one host array alone)
    (dict(lens=[1, 2, 3, -4, 4]), SMX_E_SHAPE),
])
def test_table_entry_refuses_bad_shapes(change, want):
    from surreal_amd import _lib as L
    p, keep = _rows_args(**change)
    assert L.load().smx_actor_clock_rows_i32(ctypes.byref(p), None) == want


def test_table_entry_refuses_null_pointers():
    from surreal_amd import _lib as L
    lib = L.load()
    assert lib.smx_actor_clock_rows_i32(None, None) == SMX_E_NULL
    for f in ('t', 'episode_len', 'row_off'):
        p, keep = _rows_args()
        setattr(p, f, None)
        assert lib.smx_actor_clock_rows_i32(ctypes.byref(p), None) == SMX_E_NULL, f


def _clocks(rows=10, **null):
    from surreal_amd import _lib as L
    c = L.ActorClocks()
    c.t = c.episode_len = c.row_off = FAKE
    c.rows = rows
    for f in null:
        setattr(c, f, None)
    return c


def _ddpg_args(capacity=64, **change):
    from surreal_amd import _lib as L
    net = L.Mlp3()
    net.D, net.H1, net.H2, net.OUT = 7, 24, 16, 3
    net.W1 = net.b1 = net.W2 = net.b2 = net.W3 = net.b3 = FAKE
    p = L.DdpgRollout()
    p.net, p.packed = ctypes.pointer(net), FAKE
    p.n, p.D, p.A, p.steps, p.n_step = 8, 7, 3, 10, 3
    p.t, p.episode_len = -5, 0                                  # (ignored with clocks)
    for f in ('state', 'init_state', 'gpow', 'carry_obs', 'carry_act', 'carry_rew', 'obs', 'obs_next', 'actions',
              'rewards', 'dones'):
        setattr(p, f, FAKE)
    p.cursor, p.capacity = 0, capacity
    for k, v in change.items():
        setattr(p, k, v)
    return p, [net]


def test_clocked_rollouts_refuse_before_any_launch():
    from surreal_amd import _lib as L
    lib = L.load()
    ppo, ddpg = lib.smx_synth_ppo_window_rollout_clocks_f32, lib.smx_synth_ddpg_rollout_clocks_f32
    # the clocks: every pointer (the shared clock's own fields are ignored: t = 19, episode_len = 0 would be refused)
    for field in ('t', 'episode_len', 'row_off'):
        c = _clocks(**{field: 1})
        p, keep = WABI._args(t=19, episode_len=0)
        assert ppo(ctypes.byref(p), ctypes.byref(c), None) == SMX_E_NULL, field
        q, keep2 = _ddpg_args()
        assert ddpg(ctypes.byref(q), None, ctypes.byref(c), None) == SMX_E_NULL, field
    p, keep = WABI._args()
    assert ppo(ctypes.byref(p), None, None) == SMX_E_NULL
    assert ppo(None, ctypes.byref(_clocks()), None) == SMX_E_NULL
    q, keep2 = _ddpg_args()
    assert ddpg(ctypes.byref(q), None, None, None) == SMX_E_NULL
    assert ddpg(None, None, ctypes.byref(_clocks()), None) == SMX_E_NULL
    # rows within the ring
    for rows in (65, -1):
        p, keep = WABI._args(capacity=64)
        assert ppo(ctypes.byref(p), ctypes.byref(_clocks(rows=rows)), None) == SMX_E_SHAPE
        q, keep2 = _ddpg_args(capacity=64)
        assert ddpg(ctypes.byref(q), None, ctypes.byref(_clocks(rows=rows)), None) == SMX_E_SHAPE
    # the twins' own checks still hold
    for change in (dict(n_step=0), dict(advance=8), dict(cursor=64), dict(steps=0)):
        p, keep = WABI._args(**change)
        assert ppo(ctypes.byref(p), ctypes.byref(_clocks()), None) == SMX_E_SHAPE, change
    p, keep = WABI._args()
    p.pds = None
    assert ppo(ctypes.byref(p), ctypes.byref(_clocks()), None) == SMX_E_NULL
    for change in (dict(n_step=0), dict(cursor=64), dict(steps=0), dict(actors_per_workgroup=5)):
        q, keep2 = _ddpg_args(**change)
        assert ddpg(ctypes.byref(q), None, ctypes.byref(_clocks()), None) == SMX_E_SHAPE, change
    q, keep2 = _ddpg_args(obs_next=None)
    assert ddpg(ctypes.byref(q), None, ctypes.byref(_clocks()), None) == SMX_E_NULL


# ---- SyntheticVecEnv ------------------------------------------------------------------------------------------------

@pytest.fixture
def ppo_double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(CC.ClockPpoWindowCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


@pytest.fixture
def ddpg_double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(CC.ClockDdpgRolloutCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


def test_constructor_and_clock_views(ppo_double):
    from surreal_amd.env import SyntheticVecEnv
    shared = SyntheticVecEnv(3, 5, 2, episode_len=9, device='cpu')
    assert not shared.per_actor_clocks and shared.episode_len == 9
    assert shared.episode_lens.dtype == np.int32 and shared.episode_lens.tolist() == [9, 9, 9]
    assert shared.clocks.dtype == np.int32 and shared.clocks.tolist() == [0, 0, 0]
    own = SyntheticVecEnv(3, 5, 2, episode_len=[9, 9, 9], device='cpu')
    assert own.per_actor_clocks and own.episode_lens.tolist() == [9, 9, 9] and own.clocks.tolist() == [0, 0, 0]
    own.clocks[0] = 5                                             # (copies)
    own.episode_lens[0] = 5
    assert own.clocks.tolist() == [0, 0, 0] and own.episode_lens.tolist() == [9, 9, 9]
    for bad in ([9, 9], [9, 0, 9], [9.5, 9, 9], [[9, 9, 9]]):
        with pytest.raises(ValueError):
            SyntheticVecEnv(3, 5, 2, episode_len=bad, device='cpu')


def test_everything_else_is_refused(ppo_double):
    from surreal_amd.env import SyntheticVecEnv
    n, Dd, Aa = 3, 5, 2
    venv = SyntheticVecEnv(n, Dd, Aa, episode_len=[4, 5, 6], device='cpu')
    agent, _ = PW.make_agent(Dd, Aa, 4, 3)
    said = 'per-actor episode clocks: the one-launch low-dimensional ppo_rollout_into / ddpg_rollout_into only'
    calls = {
        'step': lambda: venv.step(torch.zeros(n, Aa)),
        'start_rollout': lambda: venv.start_rollout(4),
        'rollout': lambda: venv.rollout(agent),
        'rollout_into': lambda: venv.rollout_into(agent, {}),
        'rollout_reference': lambda: venv.rollout_reference(agent, None),
        'emit_windows': lambda: venv.emit_windows(4, 3),
    }
    for name, call in calls.items():
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value).startswith(name + ':') and said in str(e.value), name
    assert venv.can_ppo_rollout_into(agent)


def test_ddpg_routes_other_than_the_launch_are_refused(ddpg_double):
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    n, Dd, Aa = 3, 5, 2
    said = 'per-actor episode clocks: the one-launch low-dimensional ppo_rollout_into / ddpg_rollout_into only'
    lc, ec, sc = DC.configs(Dd, Aa, n)
    agent = DC.make_agent(lc, ec, sc)
    venv = SyntheticVecEnv(n, Dd, Aa, episode_len=[4, 5, 6], device='cpu')
    with pytest.raises(NotImplementedError) as e:
        venv.ddpg_rollout_into(agent, UniformReplay(lc, ec, sc), 3, reference=True)
    assert "'two_launch'" in str(e.value) and said in str(e.value)
    lc, ec, sc = DC.configs(Dd, Aa, n, hidden=(22, 16))            # a shape the launch refuses: the per-step path
    agent = DC.make_agent(lc, ec, sc)
    with pytest.raises(NotImplementedError) as e:
        venv.ddpg_rollout_into(agent, UniformReplay(lc, ec, sc), 3)
    assert "'steps'" in str(e.value) and said in str(e.value)


def test_camera_routes_are_refused(ppo_double):
    import ddpg_pixel_rollout_cases as DPC
    import ppo_pixel_window_cases as PPC
    from surreal_amd import kernels as KN
    from surreal_amd.env import SyntheticVecEnv
    said = 'per-actor episode clocks: the one-launch low-dimensional ppo_rollout_into / ddpg_rollout_into only'
    n, pixel = 2, (1, 24, 24)
    prev = KN.set_default_kernels(PPC.PpoPixelWindowCpuKernels(), 'cpu')
    try:
        agent, (lc, ec, sc) = PPC.make_agent(5, 2, 4, 3, pixel=pixel, stacks=2)
        venv = SyntheticVecEnv(n, 5, 2, episode_len=[4, 5], device='cpu', pixel=pixel, frame_stacks=2)
        assert not venv.can_ppo_rollout_into(agent)
        from surreal_amd.replay import FIFOReplay
        with pytest.raises(NotImplementedError) as e:
            venv.ppo_rollout_into(agent, FIFOReplay(lc, ec, sc), 3)
        assert said in str(e.value)
    finally:
        KN.set_default_kernels(*prev)
    prev = KN.set_default_kernels(DPC.DdpgPixelRolloutCpuKernels(), 'cpu')
    try:
        lc, ec, sc = DPC.configs(5, 2, n, pixel, 2)
        agent = DC.make_agent(lc, ec, sc)
        venv = SyntheticVecEnv(n, 5, 2, episode_len=[4, 5], device='cpu', pixel=pixel, frame_stacks=2)
        from surreal_amd.replay import UniformReplay
        with pytest.raises(NotImplementedError) as e:
            venv.ddpg_rollout_into(agent, UniformReplay(lc, ec, sc), 3)
        assert "'camera'" in str(e.value) and said in str(e.value)
    finally:
        KN.set_default_kernels(*prev)


# ---- through the doubles: n host chains, bit for bit ------------------------------------------------------------------

def _ppo_pair(rnn_hidden, det=False, lens=CC.LENS, chunks=CC.CHUNKS, window=CC.PPO_WINDOW, seed=3):
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd.replay import FIFOReplay
    n, Dd, Aa = len(lens), CC.D, CC.A
    steps = sum(chunks)
    eps = None if det else torch.randn(steps, n, Aa, generator=torch.Generator().manual_seed(seed))
    host_agent, cfg = PW.make_agent(Dd, Aa, *window, rnn_hidden=rnn_hidden, deterministic=det, seed=seed)
    want, pairs = CC.host_windows(host_agent, cfg, n, Dd, lens, steps, eps)
    agent, (lc, ec, sc) = PW.make_agent(Dd, Aa, *window, rnn_hidden=rnn_hidden, deterministic=det, seed=seed)
    venv = SyntheticVecEnv(n, Dd, Aa, episode_len=list(lens), device='cpu')
    got, rows = PW.device_windows(venv, agent, FIFOReplay(lc, ec, sc), chunks, eps)
    return got, rows, want, pairs, venv, agent, host_agent


@pytest.mark.parametrize('rnn_hidden,det', [(None, False), (10, False), (None, True)])
def test_ppo_windows_equal_the_host_chains(ppo_double, rnn_hidden, det):
    got, rows, want, pairs, venv, agent, host_agent = _ppo_pair(rnn_hidden, det)
    assert ppo_double.window_launches == len(CC.CHUNKS)
    assert rows == 22 == len(pairs) and pairs == CC.records_of(CC.LENS, sum(CC.CHUNKS), 4, 3)
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert np.array_equal(venv.clocks, np.array([sum(CC.CHUNKS) % x for x in CC.LENS]))
    if rnn_hidden:
        for x, y in zip(agent._batch_cells + agent.batch_cells_before,
                        host_agent._batch_cells + host_agent.batch_cells_before):
            assert torch.equal(x.cpu().reshape(y.shape), y.cpu())


def test_ppo_equal_clocks_leave_the_shared_bytes(ppo_double):
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd.replay import FIFOReplay
    n, Dd, Aa = 6, CC.D, CC.A
    eps = torch.randn(sum(CC.CHUNKS), n, Aa, generator=torch.Generator().manual_seed(1))
    outs = []
    for episode_len in (9, [9] * n):
        agent, (lc, ec, sc) = PW.make_agent(Dd, Aa, *CC.PPO_WINDOW, rnn_hidden=10)
        venv = SyntheticVecEnv(n, Dd, Aa, episode_len=episode_len, device='cpu')
        outs.append(PW.device_windows(venv, agent, FIFOReplay(lc, ec, sc), CC.CHUNKS, eps))
    assert outs[0][1] == outs[1][1] > 0
    for k in outs[0][0]:
        assert np.array_equal(outs[0][0][k], outs[1][0][k]), k


def test_ppo_held_windows_and_reset(ppo_double):
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd.replay import FIFOReplay
    n, Dd, Aa = 6, CC.D, CC.A
    agent, (lc, ec, sc) = PW.make_agent(Dd, Aa, *CC.PPO_WINDOW)
    venv = SyntheticVecEnv(n, Dd, Aa, episode_len=list(CC.LENS), device='cpu')
    replay = FIFOReplay(lc, ec, sc)
    venv.ppo_rollout_into(agent, replay, 7)
    assert venv.clocks.tolist() == [7 % x for x in CC.LENS]
    venv._ppo['t'] = venv._ppo['t'] + 1                        # (as if stepped elsewhere)
    with pytest.raises(ValueError, match='are not held'):
        venv.ppo_rollout_into(agent, replay, 1)
    venv.reset()
    assert venv.clocks.tolist() == [0] * n and venv._ppo == {}
    assert venv.ppo_rollout_into(agent, replay, 3) == 0         # n_step 4: nothing closes in three steps
    small = FIFOReplay(*PW.configs(Dd, Aa, *CC.PPO_WINDOW, memory_size=5, batch_size=4))
    with pytest.raises(ValueError, match='exceed the FIFO capacity'):
        venv.ppo_rollout_into(agent, small, 20)


@pytest.mark.parametrize('noise,mode', [('normal', 'training'), ('ou_noise', 'training'),
                                        ('normal', 'eval_deterministic_local')])
def test_ddpg_transitions_equal_the_host_chains(ddpg_double, noise, mode):
    import recorder_cases as RC
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    n, Dd, Aa, cap = CC.N_ACTORS, CC.D, CC.A, 96
    steps = sum(CC.CHUNKS)
    lc, ec, sc = DC.configs(Dd, Aa, n, hidden=CC.HIDDEN, n_step=CC.DDPG_N_STEP, noise_type=noise, memory_size=cap,
                            theta=2.0, dt=0.05)
    agent = DC.make_agent(lc, ec, sc, mode=mode)
    eps_all = np.random.RandomState(3).randn(steps, n, Aa).astype(np.float32)
    want, pairs = CC.host_transitions(agent, lc, ec, sc, n, CC.LENS, eps_all)
    assert len(pairs) == 70 and pairs == CC.records_of(CC.LENS, steps, CC.DDPG_N_STEP, 1)
    venv = SyntheticVecEnv(n, Dd, Aa, episode_len=list(CC.LENS), device='cpu')
    replay = UniformReplay(lc, ec, sc)
    eps = None if mode != 'training' else torch.as_tensor(eps_all)
    assert CC.device_transitions(venv, agent, replay, CC.CHUNKS, eps) == 70 == len(replay)
    RC.assert_ring_equals(replay, want, cap)
    assert np.array_equal(venv.clocks, np.array([steps % x for x in CC.LENS]))


def test_ddpg_capacity_is_checked(ddpg_double):
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    lc, ec, sc = DC.configs(CC.D, CC.A, 6, hidden=CC.HIDDEN, n_step=3, memory_size=64)
    agent = DC.make_agent(lc, ec, sc)
    venv = SyntheticVecEnv(6, CC.D, CC.A, episode_len=list(CC.LENS), device='cpu')
    with pytest.raises(ValueError, match='exceed the replay capacity'):
        venv.ddpg_rollout_into(agent, UniformReplay(lc, ec, sc), 20)
