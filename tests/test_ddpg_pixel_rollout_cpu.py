"""CPU tier: SyntheticVecEnv.ddpg_rollout_into with a camera (perception -> actor -> smx_synth_ddpg_pixel_step per step)
on the torch-CPU double of its kernels against the host path -- n SyntheticEnv(pixel) + FrameStackWrapper + DDPGAgent.act
+ ExpSenderWrapperSSARNStepBootstrap stepped one by one -- bit for bit, uint8 frames included; its refusals, reset(),
reserve_ring's dtypes, a camera learner's staging buffers and the C ABI of the new entry point."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ddpg_pixel_rollout_cases as PC
import helpers as H
from helpers import _offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def pixel_double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(PC.DdpgPixelRolloutCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


def run_device(K, agent, lc, ec, sc, n, episode_len, eps_all, calls, pixel, stacks):
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    D, A = agent.model.low_dim, agent.action_dim
    venv = SyntheticVecEnv(n, D, A, episode_len=episode_len, device='cpu', kernels=K, pixel=pixel, frame_stacks=stacks)
    replay = UniformReplay(lc, ec, sc)
    written, s0 = 0, 0
    for T in calls:
        written += venv.ddpg_rollout_into(agent, replay, T, eps=torch.as_tensor(eps_all[s0:s0 + T]))
        s0 += T
        assert venv.t == s0 % episode_len
    return venv, replay, written


def assert_rings_equal(got, want):
    for k in PC.FIELDS:
        g, w = got[k].reshape(want[k].shape), want[k]
        if g.dtype == np.uint8:
            assert np.array_equal(g, w), (k, np.argwhere(g != w)[:5])
        else:
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (k, np.argwhere(g != w)[:5])


def check_against_host(K, n=3, D=5, A=2, pixel=(2, 20, 24), stacks=3, episode_len=9, calls=(5, 7, 4), capacity=23,
                       mode='training', **cfg):
    lc, ec, sc = PC.configs(D, A, n, pixel, stacks, memory_size=capacity, **cfg)
    agent = PC.DC.make_agent(lc, ec, sc, mode=mode)
    eps_all = np.random.RandomState(11).randn(sum(calls), n, A).astype(np.float32)
    venv, replay, written = run_device(K, agent, lc, ec, sc, n, episode_len, eps_all, calls, pixel, stacks)
    want, total = PC.host_ring(agent, lc, ec, sc, n, episode_len, eps_all, capacity, pixel, stacks)
    assert written == total
    assert len(replay) == min(capacity, total) and replay._dev_next == total % capacity
    assert replay.cumulative_collected_count == total
    got = H.device_ring(replay, PC.FIELDS)
    assert got['pixel'].dtype == np.uint8 and got['pixel_next'].dtype == np.uint8
    if total:
        assert_rings_equal(got, want)
    return total, venv


@pytest.mark.parametrize('stacks', [1, 3, 4])
@pytest.mark.parametrize('n_step', [1, 3, 5])
@pytest.mark.parametrize('noise', ['normal', 'ou_noise', 'deterministic'])
def test_pixel_rollout_matches_host_path_bit_for_bit(pixel_double, noise, n_step, stacks):
    """three calls of 5, 7 and 4 steps over episodes of 9: episodes end inside calls, calls start mid-episode (the open
    transitions, the OU state and the frame history carry over), and the 23-row ring wraps"""
    mode = 'eval_deterministic_local' if noise == 'deterministic' else 'training'
    total, _ = check_against_host(pixel_double, mode=mode, n_step=n_step, stacks=stacks, gamma=0.9,
                                  noise_type='normal' if noise == 'deterministic' else noise, max_sigma=0.8,
                                  theta=2.0, dt=0.05)
    assert total > 23                          # the ring wrapped


def test_pixel_rollout_frame_size_off_sixteen_and_one_actor(pixel_double):
    """C*H*W = 462 (not a multiple of 16: the launch's byte path) and a single actor"""
    check_against_host(pixel_double, n=1, pixel=(1, 21, 22), stacks=2, episode_len=6, calls=(4, 9), capacity=10,
                       n_step=2, noise_type='ou_noise')


def test_pixel_rollout_n_step_longer_than_an_episode_writes_nothing(pixel_double):
    total, venv = check_against_host(pixel_double, episode_len=4, calls=(6, 5), n_step=5, stacks=2)
    assert total == 0


def test_pixel_rollout_step_launches(pixel_double):
    """one perception, one actor forward and one step launch per step; the history primed once"""
    calls = {'step': 0, 'frames': 0, 'in_step': False}
    orig_step, orig_frames = pixel_double.synth_ddpg_pixel_step, pixel_double.synth_frames

    def step(r, mu):
        calls['step'] += 1
        calls['in_step'] = True
        orig_step(r, mu)
        calls['in_step'] = False

    def frames(*a):
        calls['frames'] += not calls['in_step']          # (the double's step renders through it too)
        orig_frames(*a)
    pixel_double.synth_ddpg_pixel_step, pixel_double.synth_frames = step, frames
    try:
        check_against_host(pixel_double, n_step=3, stacks=3, noise_type='ou_noise')
    finally:
        del pixel_double.synth_ddpg_pixel_step, pixel_double.synth_frames
    assert calls['step'] == 16 and calls['frames'] == 3 + 3     # 16 steps; the N + S history slots once


def _camera_setup(K, n=2, D=5, A=2, pixel=(2, 20, 24), stacks=2, memory_size=64, **cfg):
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    lc, ec, sc = PC.configs(D, A, n, pixel, stacks, memory_size=memory_size, n_step=2, **cfg)
    agent = PC.DC.make_agent(lc, ec, sc)
    venv = SyntheticVecEnv(n, D, A, episode_len=10, device='cpu', kernels=K, pixel=pixel, frame_stacks=stacks)
    return agent, venv, UniformReplay(lc, ec, sc), (lc, ec, sc)


def test_pixel_rollout_refusals(pixel_double):
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    K = pixel_double
    agent, venv, replay, (lc, ec, sc) = _camera_setup(K, memory_size=5)
    with pytest.raises(ValueError, match='capacity'):
        venv.ddpg_rollout_into(agent, replay, 4)             # 3 closing steps x 2 actors > 5 rows
    with pytest.raises(ValueError, match='reference'):
        venv.ddpg_rollout_into(agent, replay, 2, reference=True)
    for kw in (dict(pixel=(2, 20, 24), frame_stacks=3),      # camera0 is (4, 20, 24), the env stacks 3 frames
               dict(pixel=(1, 20, 24), frame_stacks=2),
               dict(pixel=(2, 24, 24), frame_stacks=2)):
        other = SyntheticVecEnv(2, 5, 2, episode_len=10, device='cpu', kernels=K, **kw)
        with pytest.raises(ValueError, match='camera0'):
            other.ddpg_rollout_into(agent, replay, 2)
        assert other.t == 0 and other._ddpg.get('hist') is None
    wide = SyntheticVecEnv(2, 6, 2, episode_len=10, device='cpu', kernels=K, pixel=(2, 20, 24), frame_stacks=2)
    with pytest.raises(ValueError, match='low_dim'):
        wide.ddpg_rollout_into(agent, replay, 2)
    flat = SyntheticVecEnv(2, 5, 2, episode_len=10, device='cpu', kernels=K)
    with pytest.raises(NotImplementedError, match='camera'):   # a camera agent on an env without one
        flat.ddpg_rollout_into(agent, replay, 2)
    lc2, ec2, sc2 = PC.configs(5, 2, 2, (2, 20, 24), 2, memory_size=5, n_step=2, param_noise_type='adaptive_normal')
    with pytest.raises(NotImplementedError, match='adaptive_normal'):
        venv.ddpg_rollout_into(PC.DC.make_agent(lc2, ec2, sc2), replay, 2)
    assert venv.t == 0 and len(replay) == 0 and replay.cumulative_collected_count == 0 and replay._tables is None
    assert venv.ddpg_rollout_into(agent, replay, 3) == 4      # 2 closing steps x 2 actors fit


def test_pixel_rollout_reset_clears_the_frame_history(pixel_double):
    K = pixel_double
    agent, venv, replay, _ = _camera_setup(K)
    assert venv.ddpg_rollout_into(agent, replay, 4) == 2 * 3
    d = venv._ddpg
    assert d['hist_pos'] == 4 % (2 + 2) and int(d['hist'].sum()) > 0
    venv.reset()
    assert venv.t == 0 and d['hist_pos'] is None and int(d['hist'].sum()) == 0
    for k in ('ou', 'carry_obs', 'carry_act', 'carry_rew'):
        assert float(d[k].abs().sum()) == 0, k
    # after reset() a rollout writes what a fresh env's does
    eps = torch.randn(5, 2, 2, generator=torch.Generator().manual_seed(4))
    agent2, fresh, replay2, _ = _camera_setup(K)
    first = replay._dev_next
    assert venv.ddpg_rollout_into(agent, replay, 5, eps=eps) == fresh.ddpg_rollout_into(agent, replay2, 5, eps=eps)
    for k in PC.FIELDS:
        a, b = replay._tables[k].data, replay2._tables[k].data
        assert torch.equal(a[first:first + 8], b[:8]), k
    assert torch.equal(venv._ddpg['hist'], fresh._ddpg['hist'])


def test_reserve_ring_dtypes(pixel_double):
    from surreal_amd.replay import UniformReplay
    lc, ec, sc = PC.configs(5, 2, 2, (2, 20, 24), 2, memory_size=16)
    replay = UniformReplay(lc, ec, sc)
    shapes = {'obs': (5,), 'pixel': (4, 20, 24)}
    tabs, cursor, cap = replay.reserve_ring(3, shapes, {'pixel': torch.uint8})
    assert (cursor, cap) == (0, 16)
    assert tabs['pixel'].dtype == torch.uint8 and tuple(tabs['pixel'].shape) == (16, 4 * 20 * 24)
    assert tabs['obs'].dtype == torch.float32 and tuple(tabs['obs'].shape) == (16, 5)
    again, _, _ = replay.reserve_ring(3, shapes, {'pixel': torch.uint8})
    assert again['pixel'].data_ptr() == tabs['pixel'].data_ptr()
    with pytest.raises(ValueError, match='pixel'):
        replay.reserve_ring(3, shapes)                      # the table is uint8, fp32 asked
    with pytest.raises(ValueError, match='obs'):
        replay.reserve_ring(3, {'obs': (5,)}, {'obs': torch.uint8})
    with pytest.raises(ValueError, match='pixel'):
        replay.reserve_ring(3, {'pixel': (2, 20, 24)}, {'pixel': torch.uint8})
    with pytest.raises(ValueError, match='fit'):
        replay.reserve_ring(17, shapes, {'pixel': torch.uint8})


def test_staging_fields_of_a_camera_learner(pixel_double):
    from surreal_amd.learner.ddpg import DDPGLearner
    lc, ec, sc = PC.configs(5, 2, 2, (2, 20, 24), 3)
    learner = DDPGLearner(lc, ec, sc)
    f = learner.staging_fields(8)
    assert set(f) == {'obs', 'obs_next', 'actions', 'rewards', 'dones', 'pixel', 'pixel_next'}
    for k in ('pixel', 'pixel_next'):
        assert f[k].dtype == torch.uint8 and tuple(f[k].shape) == (8, 6, 20, 24) and f[k].is_contiguous(), k
    assert tuple(f['obs'].shape) == (8, 5) and tuple(f['obs_next'].shape) == (8, 5)
    assert tuple(f['actions'].shape) == (8, 2) and tuple(f['rewards'].shape) == (8,)
    g = learner.staging_fields(8)
    assert all(g[k].data_ptr() == f[k].data_ptr() for k in f)


def test_act_batch_takes_the_nested_camera_observation(pixel_double):
    """act_batch(nested obs) = perception + actor over all rows; per row the bits of the batch-1 act (deterministic)"""
    import collections
    lc, ec, sc = PC.configs(5, 2, 3, (2, 20, 24), 2)
    agent = PC.DC.make_agent(lc, ec, sc, mode='eval_deterministic_local')
    rs = np.random.RandomState(2)
    pix = rs.randint(0, 256, size=(3, 4, 20, 24)).astype(np.uint8)
    low = rs.randn(3, 5).astype(np.float32)
    obs = collections.OrderedDict(pixel={'camera0': torch.as_tensor(pix)}, low_dim={'flat_inputs': torch.as_tensor(low)})
    got = agent.act_batch(obs).numpy()
    for i in range(3):
        want = agent.act(collections.OrderedDict(pixel={'camera0': pix[i]}, low_dim={'flat_inputs': low[i]}))
        assert np.array_equal(got[i], want), i
    x = agent.model.forward_perception(obs)                  # the tensor form is unchanged
    assert np.array_equal(agent.act_batch(x).numpy(), got)


def test_pixel_step_struct_matches_the_ctypes_mirror(tmp_path):
    from surreal_amd import _lib as L
    got = _offsets(tmp_path, 'struct smx_ddpg_pixel_step', L.DdpgPixelStep)
    assert got['sizeof'] == ctypes.sizeof(L.DdpgPixelStep)
    for fname, _ in L.DdpgPixelStep._fields_:
        assert got[fname] == getattr(L.DdpgPixelStep, fname).offset, fname
    assert got['base'] == 0 and ctypes.sizeof(L.DdpgRollout) <= got['C']


def test_pixel_step_signature_matches_the_header():
    from surreal_amd import _lib as L
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'surreal_amd.h')).read(), flags=re.S)
    m = re.search(r'\bint\s+smx_synth_ddpg_pixel_step\s*\(([^;]*)\)\s*;', hdr)
    assert m, 'smx_synth_ddpg_pixel_step is not declared'
    params = [p.strip() for p in m.group(1).split(',')]
    assert params[0].startswith('const struct smx_ddpg_pixel_step*') and params[1].startswith('const float*')
    assert params[2].startswith('int64_t') and params[3].startswith('smx_stream_t') and len(params) == 4
    restype, argtypes = L._SIGS['smx_synth_ddpg_pixel_step']
    assert restype is ctypes.c_int32
    assert argtypes[0]._type_ is L.DdpgPixelStep and argtypes[2] is ctypes.c_int64 and len(argtypes) == 4
