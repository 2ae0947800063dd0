"""CPU tier: struct smx_synth_ppo_window_rollout as gcc lays it out (include/surreal_amd.h) against its ctypes mirror, the
shapes its entry point takes, and the argument checks that refuse a call before anything is launched (no GPU needed)."""
import ctypes

import pytest

from helpers import _offsets

SMX_E_NULL, SMX_E_SHAPE, SMX_E_UNSUPPORTED = -1, -2, -3


def test_window_rollout_struct_matches_the_ctypes_mirror(tmp_path):
    from surreal_amd import _lib as L
    got = _offsets(tmp_path, 'struct smx_synth_ppo_window_rollout', L.SynthPpoWindowRollout)
    assert got['sizeof'] == ctypes.sizeof(L.SynthPpoWindowRollout)
    for fname, _ in L.SynthPpoWindowRollout._fields_:
        assert got[fname] == getattr(L.SynthPpoWindowRollout, fname).offset, fname
    assert got['base'] == 0 and ctypes.sizeof(L.SynthLstmRollout) <= got['n_step']
    assert 'smx_synth_ppo_window_rollout_f32' in L.EXPORTED_SYMBOLS
    assert 'smx_synth_ppo_window_rollout_supported' in L.EXPORTED_SYMBOLS


def test_window_rollout_shape_rules():
    from surreal_amd import _lib as L
    ok = L.load().smx_synth_ppo_window_rollout_supported
    assert ok(376, 0, 300, 200, 17) and ok(17, 0, 300, 200, 6) and ok(7, 0, 24, 16, 3)      # plain MLP
    assert ok(376, 100, 300, 200, 17) and ok(17, 100, 300, 200, 6) and ok(7, 12, 24, 16, 3)  # LSTM stem
    assert not ok(17, 0, 300, 200, 33) and not ok(17, 100, 300, 200, 33)   # A <= 32
    assert not ok(17, 0, 302, 200, 6)                                       # hidden sizes multiples of 4
    assert not ok(513, 0, 300, 200, 6)                                      # D <= 512
    assert not ok(17, 10, 300, 200, 6) and not ok(17, 132, 300, 200, 6)     # units padded to 4, <= 128
    # 16-actor blocks run the 4-row loop here: what rollout16_kernel's tighter tiles take need not fit
    assert not ok(512, 0, 640, 640, 17)


def _args(n=8, D=7, A=3, H1=24, H2=16, t=0, steps=10, episode_len=19, n_step=7, advance=3, cursor=0, capacity=64):
    """an argument block whose device pointers are never dereferenced: every call below is refused on the host"""
    from surreal_amd import _lib as L
    keep = []
    net = L.Mlp3()
    net.D, net.H1, net.H2, net.OUT = D, H1, H2, A
    fake = ctypes.c_void_p(4096)
    net.W1 = net.b1 = net.W2 = net.b2 = net.W3 = net.b3 = fake
    keep.append(net)
    p = L.SynthPpoWindowRollout()
    q = p.base.roll
    q.net, q.packed, q.log_var, q.state, q.init_state = ctypes.pointer(net), fake, fake, fake, fake
    q.n, q.t, q.steps, q.episode_len = n, t, steps, episode_len
    p.n_step, p.advance = n_step, advance
    for f in ('carry_obs', 'carry_act', 'carry_rew', 'carry_pd', 'obs', 'obs_next', 'actions', 'rewards', 'dones',
              'pds'):
        setattr(p, f, fake)
    p.cursor, p.capacity = cursor, capacity
    return p, keep


@pytest.mark.parametrize('change,want', [
    (dict(n_step=0), SMX_E_SHAPE),
    (dict(advance=0), SMX_E_SHAPE),
    (dict(advance=8), SMX_E_SHAPE),                 # advance = min(stride, n_step) <= n_step
    (dict(capacity=0), SMX_E_SHAPE),
    (dict(cursor=64), SMX_E_SHAPE),
    (dict(t=19), SMX_E_SHAPE),                      # the clock lies inside an episode
    (dict(steps=0), SMX_E_SHAPE),
    (dict(steps=40, capacity=63), SMX_E_SHAPE),     # 8 actors x 10 closing steps: two windows would share a row
    (dict(A=33), SMX_E_UNSUPPORTED),
])
def test_invalid_calls_are_refused(change, want):
    from surreal_amd import _lib as L
    p, keep = _args(**change)
    assert L.load().smx_synth_ppo_window_rollout_f32(ctypes.byref(p), None) == want


def test_missing_tables_are_refused():
    from surreal_amd import _lib as L
    lib = L.load()
    for f in ('carry_obs', 'carry_pd', 'obs_next', 'pds'):
        p, keep = _args()
        setattr(p, f, None)
        assert lib.smx_synth_ppo_window_rollout_f32(ctypes.byref(p), None) == SMX_E_NULL, f
    # an LSTM policy needs its state out and the cells' ring and table
    p, keep = _args()
    lstm = L.Lstm()
    p.base.lstm = ctypes.pointer(lstm)
    assert lib.smx_synth_ppo_window_rollout_f32(ctypes.byref(p), None) == SMX_E_NULL
