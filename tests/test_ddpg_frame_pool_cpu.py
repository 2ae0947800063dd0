"""CPU tier: the frame-pool layout of the device DDPG replay (replay.device_frame_pool) on the torch-CPU doubles of its
launches: against the stacked layout, against n host chains SyntheticEnv(pixel) -> FrameStackWrapper -> DDPGAgent.act ->
ExpSenderWrapperSSARNStepBootstrap, the live-row ledger against brute force, the structs against the header, the
refusals, the derived memory, and the option off: the calls the replay makes today."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ddpg_frame_pool_cases as FC
import ddpg_pixel_rollout_cases as PC
from helpers import _offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_, D_, A_ = FC.N_, FC.D_, FC.A_
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -5              # (include/surreal_amd.h's smx_status)


@pytest.fixture
def pool_double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(FC.FramePoolCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


@pytest.mark.parametrize('pixel,N,S,episode_len', FC.TWIN_CASES)
def test_pool_rollout_matches_stacked_rollout(pool_double, pixel, N, S, episode_len):
    _, live = FC.check_twin(pool_double, 'cpu', pixel, N, S, episode_len)
    assert live or N > episode_len - 1


@pytest.mark.parametrize('N,S', [(3, 3), (1, 3), (4, 2)])
def test_smallest_pool(pool_double, N, S):
    """P = N + S + 1, the smallest legal pool: a row that reaches N + S frames back lives for one more step (one that
    clamps at its episode's reset frame for longer), so rows retire long before the ring overwrites them"""
    _, live = FC.check_twin(pool_double, 'cpu', (3, 8, 8), N, S, 9, pool_steps=N + S + 1)
    assert 0 < len(live) < 4 * N_


def test_one_call_or_several(pool_double):
    one = FC.twin(pool_double, 'cpu', N_, D_, A_, (3, 8, 8), 3, 3, 9, (23,), 4 * N_)['pool'][1]
    many = FC.twin(pool_double, 'cpu', N_, D_, A_, (3, 8, 8), 3, 3, 9, (3, 4, 1, 9, 6), 4 * N_)['pool'][1]
    assert len(one) == len(many) and one._dev_next == many._dev_next
    for k in ('pool', 'frame_next', 'frame_first', 'frame_actor'):
        assert torch.equal(one.frame_pool[k], many.frame_pool[k]), k
    for k in one._tables:
        assert torch.equal(one._tables[k].data, many._tables[k].data), k


@pytest.mark.parametrize('N,S,episode_len', [(3, 3, 9), (2, 2, 4)])
def test_pool_rollout_matches_host_chains(pool_double, N, S, episode_len):
    """the rows the pool replay returns against the host path's, bit for bit (the stacked layout's own CPU check)"""
    pixel, calls, cap = (2, 6, 7), (10, 13), 4 * N_
    kw = dict(memory_size=cap, n_step=N, gamma=0.9, noise_type='ou_noise', theta=2.0, dt=0.05)
    t = FC.twin(pool_double, 'cpu', N_, D_, A_, pixel, N, S, episode_len, calls, cap)
    lc, ec, sc = FC.configs(D_, A_, N_, pixel, S, **kw)
    eps_all = np.random.RandomState(5).randn(sum(calls), N_, A_).astype(np.float32)
    want, total = PC.host_ring(t['agent'], lc, ec, sc, N_, episode_len, eps_all, cap, pixel, S)
    replay = t['pool'][1]
    live, written, _ = FC.simulate(N_, N, S, [episode_len], sum(calls), cap, replay.frame_pool['pool'].shape[1])
    assert written == total and live
    rows = sorted(live)
    got = replay.sample_batch(len(rows), indices=rows)
    for k in PC.FIELDS:
        g, w = got[k].numpy().reshape(len(rows), -1), want[k][rows]
        if g.dtype == np.uint8:
            assert np.array_equal(g, w), k
        else:
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), k


def test_ledger_against_brute_force():
    """random episode-length patterns, ring sizes and pool lengths: the ledger's closed form == the row-by-row rule"""
    from surreal_amd.replay.frame_pool import FramePoolLedger
    rs = np.random.RandomState(0)
    for trial in range(200):
        n, N, S = int(rs.randint(1, 6)), int(rs.randint(1, 5)), int(rs.randint(1, 5))
        lengths = [int(v) for v in rs.randint(1, 12, size=rs.randint(1, 5))]
        cap = int(rs.randint(n, 8 * n + 1))
        P = N + S + 1 + int(rs.randint(0, 12))
        T = int(rs.randint(1, 60))
        ledger = FramePoolLedger(cap, P)
        f = first = tau = ep = 0
        for s in range(T):
            done = tau + 1 >= lengths[ep % len(lengths)]
            oldest = max(first, f + 2 - N - S)
            after = f + (2 if done else 1)
            if s % 3 == 0:                       # (either way of driving it: step by step, or a planned call)
                ledger.retire(after)
                ledger.add(n if tau >= N - 1 else 0, oldest)
            else:
                ledger.plan([(n if tau >= N - 1 else 0, after, oldest)])
            f = after
            first, tau, ep = (f, 0, ep + 1) if done else (first, tau + 1, ep)
            live, written, f_sim = FC.simulate(n, N, S, lengths, s + 1, cap, P)
            assert f_sim == f and ledger.live == len(live), (trial, s, ledger.live, len(live))
            assert set(live) == {(written - 1 - k) % cap for k in range(len(live))}


def test_ledger_per_actor_counters_are_conservative():
    """per-actor counters: a step's rows retire together, as soon as one of them names an overwritten frame"""
    from surreal_amd.replay.frame_pool import FramePoolLedger
    big = np.iinfo(np.int64).max
    ledger = FramePoolLedger(100, 6)
    ledger.add(2, np.array([0, 3, big]))
    ledger.add(1, np.array([big, big, 4]))
    assert ledger.retire(np.array([5, 8, 9])) == 3           # oldest live counters: 0, 3, 4
    assert ledger.retire(np.array([6, 8, 9])) == 1           # actor 0's frame 0 is overwritten: the whole step leaves
    assert ledger.plan([(4, np.array([6, 8, 10]), np.array([6, 8, 10]))]) == (0, 4)


@pytest.mark.parametrize('cname,pyname', [('struct smx_ddpg_pixel_pool_step', 'DdpgPixelPoolStep'),
                                          ('struct smx_gather_pool', 'GatherPool')])
def test_pool_structs_match_the_ctypes_mirrors(tmp_path, cname, pyname):
    from surreal_amd import _lib as L
    cls = getattr(L, pyname)
    got = _offsets(tmp_path, cname, cls)
    assert got['sizeof'] == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert got[fname] == getattr(cls, fname).offset, fname


def test_pool_entry_points_are_declared_as_bound():
    from surreal_amd import _lib as L
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'surreal_amd.h')).read(), flags=re.S)
    for name, nargs, first in (('smx_synth_ddpg_pixel_pool_step', 4, L.DdpgPixelPoolStep),
                               ('smx_uniform_gather_pool', 11, L.GatherJob)):
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, hdr)
        assert m, name
        restype, argtypes = L._SIGS[name]
        assert len(m.group(1).split(',')) == nargs == len(argtypes) and argtypes[0]._type_ is first
    assert L._SIGS['smx_uniform_gather_pool'][1][2]._type_ is L.GatherPool


def test_c_entry_points_refuse_a_short_pool():
    """P < N + S + 1 is SMX_E_SHAPE before any launch (the pointers are never dereferenced)"""
    from surreal_amd import _lib as L
    lib = L.load()
    fake = ctypes.c_void_p(4096)
    p = L.DdpgPixelPoolStep()
    for name, ctype in L.DdpgRollout._fields_:
        if ctype is ctypes.c_void_p and name not in ('packed', 'eps', 'sigmas'):
            setattr(p.base, name, fake)
    b = p.base
    b.n, b.D, b.A, b.steps, b.t, b.episode_len, b.n_step, b.noise_type = 5, 7, 3, 1, 0, 9, 3, L.SMX_DDPG_NOISE_NONE
    b.cursor, b.capacity = 0, 20
    p.C, p.H, p.W, p.frame_stacks, p.frame, p.episode_first = 3, 8, 8, 3, 4, 2
    for k in ('pool', 'obs_pixel', 'frame_next', 'frame_first', 'frame_actor'):
        setattr(p, k, fake)
    p.pool_len = 6
    assert lib.smx_synth_ddpg_pixel_pool_step(ctypes.byref(p), fake, 3, None) == E_SHAPE
    p.pool_len, p.episode_first = 7, 5                       # (a reset frame newer than the current one)
    assert lib.smx_synth_ddpg_pixel_pool_step(ctypes.byref(p), fake, 3, None) == E_SHAPE
    p.episode_first, p.frame_next = 2, ctypes.c_void_p(4100)
    assert lib.smx_synth_ddpg_pixel_pool_step(ctypes.byref(p), fake, 3, None) == E_ALIGN
    p.frame_next = None
    assert lib.smx_synth_ddpg_pixel_pool_step(ctypes.byref(p), fake, 3, None) == E_NULL
    job = (L.GatherJob * 1)()
    job[0].table, job[0].dst, job[0].row_bytes = fake, fake, 28
    q = L.GatherPool()
    for k in ('pool', 'frame_next', 'frame_first', 'frame_actor', 'pixel', 'pixel_next'):
        setattr(q, k, fake)
    q.pool_len, q.frame_bytes, q.actors, q.frame_stacks, q.n_step, q.base = 6, 192, 5, 3, 3, 0
    call = lambda: lib.smx_uniform_gather_pool(job, 1, ctypes.byref(q), 20, 8, None, 10, 1, 0, None, None)  # noqa: E731
    assert call() == E_SHAPE
    q.pool_len, q.base = 7, 20
    assert call() == E_SHAPE
    q.base, q.pixel = 0, None
    assert call() == E_NULL


def test_refusals_and_derived_memory(pool_double):
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    pixel, N, S, cap = (3, 8, 8), 3, 3, 4 * N_
    t = FC.twin(pool_double, 'cpu', N_, D_, A_, pixel, N, S, 9, (23,), cap)
    replay, stacked = t['pool'][1], t['stacked'][1]
    F, P = 3 * 8 * 8, 4 + N + S
    # the camera bytes, derived: the pool, two int64 counters and the int32 actor per row; stacked: 2 S F per row
    assert replay.camera_bytes() == P * N_ * F + cap * (2 * 8 + 4)
    assert stacked.camera_bytes() == cap * 2 * S * F
    live = len(replay)
    assert 0 < live < cap
    dead = (replay._dev_next - 1 - live) % cap
    with pytest.raises(ValueError, match='live'):
        replay.sample_batch(2, indices=[(replay._dev_next - 1) % cap, dead])
    with pytest.raises(ValueError, match='live'):
        replay.sample_batch(1, indices=[cap])
    fields = stacked.sample_batch(4, indices=[0, 1, 2, 3])
    with pytest.raises(ValueError, match='frame-pool'):
        replay.insert_batch(fields)
    with pytest.raises(ValueError, match='reserve_frame_pool'):
        replay.reserve_ring(2, {'pixel': (S * 3, 8, 8)}, {'pixel': torch.uint8})
    with pytest.raises(ValueError, match='device_frame_pool is off'):
        stacked.reserve_frame_pool([], {}, N_, pixel, S, N)
    lc, ec, sc = FC.pool_configs(D_, A_, N_, pixel, S, pool_steps=N + S, memory_size=cap, n_step=N)
    venv = SyntheticVecEnv(N_, D_, A_, episode_len=9, device='cpu', kernels=pool_double, pixel=pixel, frame_stacks=S)
    with pytest.raises(ValueError, match='device_frame_pool_steps'):
        venv.ddpg_rollout_into(PC.DC.make_agent(lc, ec, sc), UniformReplay(lc, ec, sc), 2)
    assert venv.t == 0


def test_drawn_sampling_sees_live_rows_only(pool_double):
    t = FC.twin(pool_double, 'cpu', N_, D_, A_, (3, 8, 8), 3, 3, 9, (10, 13), 4 * N_, pool_steps=8)
    replay, stacked = t['pool'][1], t['stacked'][1]
    live, _, _ = FC.simulate(N_, 3, 3, [9], 23, 4 * N_, 8)
    assert 0 < len(live) < 4 * N_ and len(replay) == len(live)
    B = 64
    draws = replay._draws
    idx = replay.sample_indices(B)
    assert set(idx.tolist()) <= set(live) and len(set(idx.tolist())) > 1
    replay._draws = draws
    got = replay.sample_batch(B)
    want = stacked.sample_batch(B, indices=idx)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert replay._draws == draws + B


def test_reset_primes_the_pool_again(pool_double):
    """after reset() the next call writes the current frame at the next counter and starts a new episode there"""
    t = FC.twin(pool_double, 'cpu', N_, D_, A_, (3, 8, 8), 3, 3, 9, (6,), 12 * N_)
    for name in ('stacked', 'pool'):
        venv, replay = t[name]
        venv.reset()
        eps = torch.randn(7, N_, A_, generator=torch.Generator().manual_seed(2))
        assert venv.ddpg_rollout_into(t['agent'], replay, 7, eps=eps) == 5 * N_
    replay = t['pool'][1]
    assert int(replay.frame_pool['counter'][0]) == 6 + 1 + 7       # 6 steps, the primed frame, 7 steps
    assert len(replay) == len(t['stacked'][1]) == 9 * N_           # (P = 18: every row's frames are still there)
    FC.assert_live_rows_equal(t, range(9 * N_))


def test_option_off_makes_todays_calls():
    """replay.device_frame_pool absent: reserve_ring / sample_batch call what they call today, recorded on the double"""
    from surreal_amd import kernels as KN
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    log = []

    class Recording(FC.FramePoolCpuKernels):
        def synth_ddpg_pixel_step(self, r, mu):
            log.append(('synth_ddpg_pixel_step', sorted(r['tables']), int(r['cursor']), int(r['hist_pos'])))
            super().synth_ddpg_pixel_step(r, mu)

        def synth_ddpg_pixel_pool_step(self, r, mu):
            log.append(('synth_ddpg_pixel_pool_step',))
            super().synth_ddpg_pixel_pool_step(r, mu)

        def uniform_gather_multi(self, tables, outs, length, seed, offset, idx=None, idx_out=None):
            log.append(('uniform_gather_multi', len(tables), int(length), int(offset), idx is not None))
            super().uniform_gather_multi(tables, outs, length, seed, offset, idx=idx, idx_out=idx_out)

        def uniform_gather_pool(self, *a, **kw):
            log.append(('uniform_gather_pool',))
            super().uniform_gather_pool(*a, **kw)
    K = Recording()
    prev = KN.set_default_kernels(K, 'cpu')
    try:
        pixel, N, S = (3, 8, 8), 2, 2
        lc, ec, sc = FC.configs(D_, A_, N_, pixel, S, memory_size=4 * N_, n_step=N)
        assert 'device_frame_pool' not in lc.replay
        agent = PC.DC.make_agent(lc, ec, sc)
        venv = SyntheticVecEnv(N_, D_, A_, episode_len=9, device='cpu', kernels=K, pixel=pixel, frame_stacks=S)
        replay = UniformReplay(lc, ec, sc)
        assert not replay.frame_pool_on and venv.ddpg_rollout_into(agent, replay, 3) == 2 * N_
        replay.sample_batch(4)
        replay.sample_batch(2, indices=[0, 1])
    finally:
        KN.set_default_kernels(*prev)
    names = sorted(PC.FIELDS)
    assert log == [('synth_ddpg_pixel_step', names, 0, 0), ('synth_ddpg_pixel_step', names, 0, 1),
                   ('synth_ddpg_pixel_step', names, N_, 2), ('uniform_gather_multi', 7, 2 * N_, 0, False),
                   ('uniform_gather_multi', 7, 2 * N_, 4, True)]
    assert replay.frame_pool is None and set(replay._tables) == set(PC.FIELDS)


# ---- the recorder of host-stepped environments ----------------------------------------------------------------------------
REC_LENGTHS = [4, 6, 9, 5, 7]                    # every actor cycles through them from its own offset: diverging clocks


@pytest.fixture
def recorder_double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(FC.FramePoolRecorderCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


@pytest.mark.parametrize('pixel,N,S,pool_steps', [((1, 4, 4), 3, 3, None), ((3, 5, 3), 1, 3, None),
                                                  ((2, 4, 6), 4, 2, None), ((1, 4, 4), 3, 3, 7), ((3, 5, 3), 3, 1, 5)])
def test_recorder_into_a_pool_replay(recorder_double, pixel, N, S, pool_steps):
    FC.check_recorder_twin(pixel, N, S, REC_LENGTHS, pool_steps)


def test_recorder_struct_matches_the_ctypes_mirror(tmp_path):
    from surreal_amd import _lib as L
    cls = L.RecordDdpgPixelPoolNstepStep
    got = _offsets(tmp_path, 'struct smx_record_ddpg_pixel_pool_nstep_step', cls)
    assert got['sizeof'] == ctypes.sizeof(cls) and cls._fields_[-1][0] == 'mon'
    for fname, _ in cls._fields_:
        assert got[fname] == getattr(cls, fname).offset, fname


def test_recorder_entry_point_refuses_a_short_pool():
    from surreal_amd import _lib as L
    lib = L.load()
    fake = ctypes.c_void_p(4096)
    p = L.RecordDdpgPixelPoolNstepStep()
    for name, ctype in p._fields_:
        if ctype is ctypes.c_void_p and name not in ('t_host', 'rank_host'):
            setattr(p, name, fake)
    p.counters_out = ctypes.c_void_p(8192)
    p.n, p.D, p.A, p.n_step, p.rows, p.cursor, p.capacity = 5, 7, 3, 3, 2, 0, 64
    p.C, p.H, p.W, p.frame_stacks, p.pool_len = 1, 4, 4, 3, 6
    assert lib.smx_record_ddpg_pixel_pool_nstep_step(ctypes.byref(p), None) == E_SHAPE
    p.pool_len, p.counters_out = 7, fake
    assert lib.smx_record_ddpg_pixel_pool_nstep_step(ctypes.byref(p), None) == E_SHAPE      # in == out
    p.counters_out, p.frame_actor = ctypes.c_void_p(8192), ctypes.c_void_p(4098)
    assert lib.smx_record_ddpg_pixel_pool_nstep_step(ctypes.byref(p), None) == E_ALIGN
    p.pool = None
    assert lib.smx_record_ddpg_pixel_pool_nstep_step(ctypes.byref(p), None) == E_NULL


def test_memory_at_the_reference_shape():
    """derived, not measured: n = 256, memory_size 333 333, 84 x 84 x 3, S = N = 3 -- the pool P n F plus two int64 and
    the int32 actor per row against 2 S F per stacked row"""
    from surreal_amd.replay.frame_pool import default_pool_steps
    n, rows, F, S, N = 256, 333333, 84 * 84 * 3, 3, 3
    P = default_pool_steps(rows, n, N, S)
    assert P == 1303 + 6
    pool, stacked = P * n * F + rows * 20, rows * 2 * S * F
    print('frame pool %.3f GB, stacked %.3f GB' % (pool / 1e9, stacked / 1e9))
    assert round(pool / 1e9, 2) == 7.10 and round(stacked / 1e9, 1) == 42.3


def test_a_call_of_no_steps_only_primes_the_pool(pool_double):
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    pixel, N, S = (3, 8, 8), 3, 3
    lc, ec, sc = FC.pool_configs(D_, A_, N_, pixel, S, memory_size=12 * N_, n_step=N)
    agent = PC.DC.make_agent(lc, ec, sc)
    venv = SyntheticVecEnv(N_, D_, A_, episode_len=9, device='cpu', kernels=pool_double, pixel=pixel, frame_stacks=S)
    replay = UniformReplay(lc, ec, sc)
    assert venv.ddpg_rollout_into(agent, replay, 0) == 0 and len(replay) == 0
    assert int(replay.frame_pool['counter'][0]) == 0 and int(replay.frame_pool['pool'][:, 0].sum()) > 0
    assert venv.ddpg_rollout_into(agent, replay, 5) == 3 * N_ == len(replay)
    assert int(replay.frame_pool['counter'][0]) == 5
