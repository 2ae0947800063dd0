"""CPU tier: SyntheticVecEnv.ppo_rollout_into with a camera (perception -> [LSTM step ->] actor ->
smx_synth_ppo_pixel_window_step per step) on the torch-CPU double of its kernels against the host path -- n
SyntheticEnv(pixel) under FrameStackWrapper under ExpSenderWrapperMultiStepMovingWindowWithInfo driven by act_batch --
bit for bit, uint8 frames included; chunking, a ring that wraps, reset(), the refusals and the C ABI of the new entry
point."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import helpers as H
import ppo_pixel_window_cases as PP
import ppo_window_cases as PW
from helpers import _offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIXEL = (2, 20, 24)


@pytest.fixture
def pixel_double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(PP.PpoPixelWindowCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


def _eps(steps, n, A, seed=3):
    return torch.randn(steps, n, A, generator=torch.Generator().manual_seed(seed))


def _assert_bits(got, want, key):
    got = got.reshape(want.shape)
    assert got.dtype == want.dtype, (key, got.dtype, want.dtype)
    if want.dtype == np.uint8:
        assert np.array_equal(got, want), (key, np.argwhere(got != want)[:5])
    else:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (key, np.argwhere(got != want)[:5])


def _run_pair(n_step, stride, rnn_hidden, episode_len, chunks, stacks, n=3, D=5, A=2, det=False, use_z=True,
              pixel=PIXEL, seed=3):
    from surreal_amd.replay import FIFOReplay
    steps = sum(chunks)
    eps = None if det else _eps(steps, n, A, seed)
    kw = dict(rnn_hidden=rnn_hidden, use_z=use_z, deterministic=det, seed=seed)
    host_agent, cfg = PP.make_agent(D, A, n_step, stride, pixel, stacks, **kw)
    want = PP.host_windows(host_agent, cfg, n, D, episode_len, steps, eps, pixel, stacks)
    agent, (lc, ec, sc) = PP.make_agent(D, A, n_step, stride, pixel, stacks, **kw)
    venv = PP.make_venv(n, D, A, episode_len, pixel, stacks, device='cpu')
    assert venv.can_ppo_rollout_into(agent)
    got, rows = PW.device_windows(venv, agent, FIFOReplay(lc, ec, sc), chunks, eps)
    return got, rows, want, venv, agent, host_agent


# (n_step, stride, episode_len, chunks): a window closes at every episode's terminal step ((L - n_step) % advance == 0)
# and the calls straddle the resets
WINDOWS = [(7, 3, 19, [5, 9, 8, 14]), (5, 8, 20, [6, 11, 9, 17]), (4, 4, 12, [5, 9, 8, 7])]


@pytest.mark.parametrize('stacks', [1, 3])
@pytest.mark.parametrize('n_step,stride,episode_len,chunks', WINDOWS)
@pytest.mark.parametrize('use_z', [True, False])
@pytest.mark.parametrize('rnn_hidden', [12, None])
def test_windows_equal_the_host_wrapper(pixel_double, rnn_hidden, use_z, n_step, stride, episode_len, chunks, stacks):
    n = 3
    got, rows, want, venv, agent, host_agent = _run_pair(n_step, stride, rnn_hidden, episode_len, chunks, stacks, n=n,
                                                         use_z=use_z)
    steps = sum(chunks)
    assert pixel_double.pixel_steps == steps and pixel_double.window_launches == 0
    closing = PW.closing_steps(0, steps, episode_len, n_step, stride)
    assert episode_len - 1 in closing                                  # windows that close at a terminal step
    assert rows == n * len(closing) == want['obs'].shape[0] > 0
    keys = set(PP.FIELDS) | ({'cells'} if rnn_hidden else set())
    assert set(got) == keys
    for k in keys:
        _assert_bits(got[k], want[k], k)
    assert tuple(got['pixel'].shape[1:]) == (n_step, stacks * PIXEL[0]) + PIXEL[1:]
    assert tuple(got['pixel_next'].shape[1:]) == (1, stacks * PIXEL[0]) + PIXEL[1:]
    assert venv.t == steps % episode_len
    if rnn_hidden:
        for x, y in zip(agent._batch_cells + agent.batch_cells_before,
                        host_agent._batch_cells + host_agent.batch_cells_before):
            assert torch.equal(x.reshape(y.shape), y)
    else:
        assert agent._batch_cells is None
    assert float(want['dones'][:, :-1].sum()) == 0.0 and float(want['dones'][:, -1].sum()) > 0


def test_padded_lstm_units_and_a_deterministic_mode(pixel_double):
    got, rows, want, _, agent, host_agent = _run_pair(7, 3, 10, 19, [5, 9, 8, 14], 3)     # 10 units padded to 12
    assert rows > 0 and tuple(got['cells'].shape[1:]) == (2, 1, 10)
    for k in want:
        _assert_bits(got[k], want[k], k)
    for x, y in zip(agent._batch_cells + agent.batch_cells_before,
                    host_agent._batch_cells + host_agent.batch_cells_before):
        assert torch.equal(x.reshape(y.shape), y)
    for rnn_hidden in (12, None):
        got, rows, want, _, _, _ = _run_pair(5, 8, rnn_hidden, 20, [6, 11, 9, 17], 3, det=True)
        assert rows > 0
        for k in want:
            _assert_bits(got[k], want[k], k)


def test_frame_size_off_sixteen_and_one_actor(pixel_double):
    """C*H*W = 462 (not a multiple of 16: the launch's byte path) and a single actor"""
    got, rows, want, _, _, _ = _run_pair(4, 4, 12, 12, [5, 9, 8, 7], 2, n=1, pixel=(1, 21, 22))
    assert rows == want['obs'].shape[0] > 0
    for k in want:
        _assert_bits(got[k], want[k], k)


def _state_of(venv, agent, replay):
    out = {'ring.' + k: t.data.clone() for k, t in replay._tables.items()}
    out.update(state=venv.state.clone(), hist=venv._ppo['hist'].clone(), obs_pixel=venv._ppo['obs_pixel'].clone(),
               hist_pos=torch.tensor(venv._ppo['hist_pos']), t=torch.tensor(venv.t))
    out.update({'carry.' + k: v.clone() for k, v in venv._ppo['carry'].items()})
    if agent._batch_cells is not None:
        for name, cells in (('cells', agent._batch_cells), ('before', agent.batch_cells_before)):
            out.update({'%s.%d' % (name, i): x.clone() for i, x in enumerate(cells)})
    return out


@pytest.mark.parametrize('rnn_hidden', [12, None])
def test_one_call_equals_uneven_chunks(pixel_double, rnn_hidden):
    from surreal_amd.replay import FIFOReplay
    n, D, A, L_, stacks, steps = 3, 5, 2, 19, 3, 45
    eps = _eps(steps, n, A, 9)
    outs = []
    for chunks in ([steps], [1, 17, 2, 20, 5]):
        agent, (lc, ec, sc) = PP.make_agent(D, A, 7, 3, PIXEL, stacks, rnn_hidden=rnn_hidden)
        venv = PP.make_venv(n, D, A, L_, PIXEL, stacks, device='cpu')
        replay = FIFOReplay(lc, ec, sc)
        s0 = rows = 0
        for T in chunks:
            rows += venv.ppo_rollout_into(agent, replay, T, eps=eps[s0:s0 + T])
            s0 += T
        outs.append((rows, _state_of(venv, agent, replay)))
    (ra, a), (rb, b) = outs
    assert ra == rb == n * len(PW.closing_steps(0, steps, L_, 7, 3)) and set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_ring_wraps_and_untouched_rows_stay_zero(pixel_double):
    from surreal_amd.replay import FIFOReplay
    n, D, A, L_, stacks, N, stride = 3, 5, 2, 19, 3, 7, 3
    chunks = [5, 9, 8, 14, 11]
    steps = sum(chunks)
    eps = _eps(steps, n, A, 4)
    host_agent, cfg = PP.make_agent(D, A, N, stride, PIXEL, stacks, rnn_hidden=12)
    want = PP.host_windows(host_agent, cfg, n, D, L_, steps, eps, PIXEL, stacks)
    total = want['obs'].shape[0]
    for memory_size in (20, 4096):                         # a ring of 23 rows wraps; one of 4099 does not
        agent, (lc, ec, sc) = PP.make_agent(D, A, N, stride, PIXEL, stacks, rnn_hidden=12, memory_size=memory_size)
        venv = PP.make_venv(n, D, A, L_, PIXEL, stacks, device='cpu')
        replay = FIFOReplay(lc, ec, sc)
        s0 = rows = 0
        for T in chunks:
            rows += venv.ppo_rollout_into(agent, replay, T, eps=eps[s0:s0 + T])
            s0 += T
        cap = memory_size + 3
        assert rows == total and (total > cap) == (memory_size == 20) and len(replay) == min(total, cap)
        ring = H.device_ring(replay)
        for i in range(max(0, total - cap), total):        # the last `cap` windows are where the device put them
            for k in want:
                _assert_bits(ring[k][i % cap], want[k][i].reshape(-1), (k, i))
        if total < cap:
            for k in ring:
                assert not ring[k][total:].any(), k


def test_reset_equals_a_fresh_environment(pixel_double):
    from surreal_amd.replay import FIFOReplay
    n, D, A, L_, stacks = 3, 5, 2, 19, 3
    eps = _eps(30, n, A, 5)
    outs = []
    for warm in (False, True):
        agent, (lc, ec, sc) = PP.make_agent(D, A, 7, 3, PIXEL, stacks, rnn_hidden=12)
        venv = PP.make_venv(n, D, A, L_, PIXEL, stacks, device='cpu')
        if warm:
            venv.ppo_rollout_into(agent, FIFOReplay(lc, ec, sc), 11, eps=torch.randn(11, n, A))
            assert venv._ppo['hist_pos'] == 11 % (7 + stacks)
            venv.reset()
            agent._batch_cells = None
            assert venv.t == 0 and venv._ppo == {}
        got, rows = PW.device_windows(venv, agent, FIFOReplay(lc, ec, sc), [13, 17], eps)
        outs.append((got, rows, venv._ppo['hist'].clone(), venv._ppo['obs_pixel'].clone()))
    (a, ra, ha, oa), (b, rb, hb, ob) = outs
    assert ra == rb > 0 and torch.equal(ha, hb) and torch.equal(oa, ob)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_history_is_primed_once(pixel_double):
    """N + S synth_frames launches prime the history on first use, none afterwards (the double's step renders through
    synth_frames too: those are not counted)"""
    from surreal_amd.replay import FIFOReplay
    calls = {'frames': 0, 'in_step': False}
    orig_step, orig_frames = pixel_double.synth_ppo_pixel_window_step, pixel_double.synth_frames

    def step(r, mu, copy_workgroups=0):
        calls['in_step'] = True
        orig_step(r, mu, copy_workgroups)
        calls['in_step'] = False

    def frames(*a):
        calls['frames'] += not calls['in_step']
        orig_frames(*a)
    pixel_double.synth_ppo_pixel_window_step, pixel_double.synth_frames = step, frames
    try:
        agent, (lc, ec, sc) = PP.make_agent(5, 2, 7, 3, PIXEL, 3, rnn_hidden=12)
        venv = PP.make_venv(3, 5, 2, 19, PIXEL, 3, device='cpu')
        replay = FIFOReplay(lc, ec, sc)
        venv.ppo_rollout_into(agent, replay, 9)
        ws = venv._ppo_ws
        venv.ppo_rollout_into(agent, replay, 12)
        assert venv._ppo_ws is ws                      # the perception's and the LSTM's buffers: kept across calls
    finally:
        del pixel_double.synth_ppo_pixel_window_step, pixel_double.synth_frames
    assert calls['frames'] == 7 + 3 and pixel_double.pixel_steps == 21


def test_refusals(pixel_double):
    from surreal_amd.replay import FIFOReplay
    from cpu_kernels import TorchCpuKernels
    n, D, A, stacks = 3, 5, 2, 2
    agent, (lc, ec, sc) = PP.make_agent(D, A, 4, 4, PIXEL, stacks, rnn_hidden=12)
    replay = FIFOReplay(lc, ec, sc)
    # a camera on one side only
    flat = PP.make_venv(n, D, A, 9, None, 1, device='cpu')
    assert not flat.can_ppo_rollout_into(agent)
    with pytest.raises(NotImplementedError, match='camera'):
        flat.ppo_rollout_into(agent, replay, 4)
    low, _ = PW.make_agent(D, A, 4, 4, rnn_hidden=12)
    cam = PP.make_venv(n, D, A, 9, PIXEL, stacks, device='cpu')
    assert not cam.can_ppo_rollout_into(low)
    with pytest.raises(NotImplementedError, match='camera'):
        cam.ppo_rollout_into(low, replay, 4)
    # another camera, another low-dimensional width
    for pixel, s in ((PIXEL, 3), ((1, 20, 24), 2), ((2, 24, 24), 2)):
        other = PP.make_venv(n, D, A, 9, pixel, s, device='cpu')
        assert not other.can_ppo_rollout_into(agent)
        with pytest.raises(ValueError, match='camera0'):
            other.ppo_rollout_into(agent, replay, 4)
        assert other.t == 0 and other._ppo == {}
    wide = PP.make_venv(n, D + 1, A, 9, PIXEL, stacks, device='cpu')
    with pytest.raises(ValueError, match='low_dim'):
        wide.ppo_rollout_into(agent, replay, 4)
    # two LSTM layers
    two, _ = PP.make_agent(D, A, 4, 4, PIXEL, stacks, rnn_hidden=12)
    two.rnn_config.rnn_layer = 2
    with pytest.raises(NotImplementedError, match='rnn_layer'):
        cam.ppo_rollout_into(two, replay, 4)
    # the step launch's limit on the actions
    many, _ = PP.make_agent(D, 65, 4, 4, PIXEL, stacks)
    big = PP.make_venv(n, D, 65, 9, PIXEL, stacks, device='cpu')
    assert not big.can_ppo_rollout_into(many)
    with pytest.raises(ValueError, match='A <= 64'):
        big.ppo_rollout_into(many, replay, 4)
    # a kernels object without the entry point
    with pytest.raises(NotImplementedError, match='synth_ppo_pixel_window_step'):
        PP.make_venv(n, D, A, 9, PIXEL, stacks, device='cpu', kernels=TorchCpuKernels()).ppo_rollout_into(
            agent, replay, 4)
    with pytest.raises(ValueError, match='positive'):
        cam.ppo_rollout_into(agent, replay, 0)
    small, (lc2, ec2, sc2) = PP.make_agent(D, A, 4, 4, PIXEL, stacks, memory_size=4)
    with pytest.raises(ValueError, match='exceed the FIFO capacity'):
        cam.ppo_rollout_into(small, FIFOReplay(lc2, ec2, sc2), 13)       # 3 actors x 3 windows > 7 rows
    assert cam.t == 0 and len(replay) == 0 and replay._tables is None
    # a clock the carry does not hold: stepped outside ppo_rollout_into
    assert cam.ppo_rollout_into(agent, replay, 4) == n
    cam.step(torch.zeros(n, A))
    with pytest.raises(ValueError, match='reset'):
        cam.ppo_rollout_into(agent, replay, 4)
    cam.reset()
    assert cam.ppo_rollout_into(agent, replay, 4) == n


def test_perception_into_equals_the_stem(pixel_double):
    """PPOModel.perception_into = the stem input _stem forms, into the caller's buffers"""
    for use_z in (True, False):
        agent, _ = PP.make_agent(5, 2, 4, 4, PIXEL, 2, use_z=use_z)
        m = agent.model
        rs = np.random.RandomState(2)
        pix = torch.as_tensor(rs.randint(0, 256, size=(3, 4, 20, 24)).astype(np.uint8))
        low = torch.as_tensor(rs.randn(3, 5).astype(np.float32) * 3)
        want, _ = m._stem({'low_dim': {'flat_inputs': low}, 'pixel': {'camera0': pix}}, None)
        ws = m.perception_workspace(3, 'cpu')
        x = torch.full((3, m.stem_in), float('nan'))
        m.perception_into(pix, low, ws, x)
        assert torch.equal(x, want)
        again = x.clone()
        m.perception_into(pix, low, ws, x)                   # the same workspace, the same bits
        assert torch.equal(x, again)


def test_step_struct_matches_the_ctypes_mirror(tmp_path):
    from surreal_amd import _lib as L
    cls = L.SynthPpoPixelWindowStep
    got = _offsets(tmp_path, 'struct smx_synth_ppo_pixel_window_step', cls)
    assert got['sizeof'] == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert got[fname] == getattr(cls, fname).offset, fname
    assert 'smx_synth_ppo_pixel_window_step' in L.EXPORTED_SYMBOLS
    hdr = open(os.path.join(ROOT, 'include', 'surreal_amd.h')).read()
    assert int(re.search(r'#define SMX_PPO_PIXEL_STEP_MAX_A (\d+)', hdr).group(1)) == L.SMX_PPO_PIXEL_STEP_MAX_A


def test_step_signature_matches_the_header():
    from surreal_amd import _lib as L
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'surreal_amd.h')).read(), flags=re.S)
    m = re.search(r'\bint\s+smx_synth_ppo_pixel_window_step\s*\(([^;]*)\)\s*;', hdr)
    assert m, 'smx_synth_ppo_pixel_window_step is not declared'
    params = [p.strip() for p in m.group(1).split(',')]
    assert params[0].startswith('const struct smx_synth_ppo_pixel_window_step*') and params[1].startswith('const float*')
    assert params[2].startswith('int64_t') and params[3].startswith('smx_stream_t') and len(params) == 4
    restype, argtypes = L._SIGS['smx_synth_ppo_pixel_window_step']
    assert restype is ctypes.c_int32
    assert argtypes[0]._type_ is L.SynthPpoPixelWindowStep and argtypes[2] is ctypes.c_int64 and len(argtypes) == 4


def _args(**change):
    """an argument block whose device pointers are never dereferenced: every call below is refused on the host"""
    from surreal_amd import _lib as L
    p = L.SynthPpoPixelWindowStep()
    fake = ctypes.c_void_p(4096)
    p.n, p.D, p.A, p.hidden, p.t, p.episode_len, p.n_step, p.advance = 8, 7, 3, 0, 0, 19, 7, 3
    for f in ('log_var', 'state', 'init_state', 'carry_obs', 'carry_act', 'carry_rew', 'carry_pd', 'obs', 'obs_next',
              'actions', 'rewards', 'dones', 'pds', 'hist', 'pixel', 'pixel_next', 'obs_pixel'):
        setattr(p, f, fake)
    p.cursor, p.capacity = 0, 64
    p.C, p.H, p.W, p.frame_stacks, p.hist_len, p.hist_pos = 2, 20, 24, 3, 10, 0
    for k, v in change.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize('change,want', [
    (dict(n_step=0), -2), (dict(advance=0), -2), (dict(advance=8), -2), (dict(capacity=0), -2), (dict(cursor=64), -2),
    (dict(t=19), -2), (dict(n=65), -2), (dict(hist_len=9), -2), (dict(hist_pos=10), -2), (dict(frame_stacks=0), -2),
    (dict(copy_workgroups=-1), -2), (dict(A=65), -3),
    (dict(log_var=None), -1), (dict(carry_pd=None), -1), (dict(pixel_next=None), -1), (dict(hist=None), -1),
    (dict(h_before=ctypes.c_void_p(4096)), -1),                                  # h without c
    (dict(h_before=ctypes.c_void_p(4096), c_before=ctypes.c_void_p(4096), hidden=4), -1),      # cells without their ring
])
def test_invalid_calls_are_refused(change, want):
    from surreal_amd import _lib as L
    lib = L.load()
    fake = ctypes.c_void_p(4096)
    assert lib.smx_synth_ppo_pixel_window_step(ctypes.byref(_args(**change)), fake, 3, None) == want
    assert lib.smx_synth_ppo_pixel_window_step(ctypes.byref(_args()), None, 3, None) == -1       # no mu
    assert lib.smx_synth_ppo_pixel_window_step(ctypes.byref(_args()), fake, 2, None) == -2       # ld_mu < A
