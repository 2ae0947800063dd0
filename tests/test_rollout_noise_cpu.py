"""CPU tier: the restatement of the rollouts' noise stream (noise_ref.py) against itself and against the scalar Philox the
known-answer vectors hold; the struct's layout against its ctypes mirror; the keyword the kernels objects take."""
import ctypes
import inspect
import os
import subprocess

import numpy as np

import noise_ref as NR
import philox_ref as PR

SEED = 0x9E3779B97F4A7C15          # fixed: the moments below are those of this seed, the test is deterministic
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_vector_philox_is_the_scalar_restatement():
    for ctr, key, want in PR.KAT:
        got = NR.philox_blocks(*[np.array([c]) for c in ctr], key[0], key[1])
        assert tuple(int(x[0]) for x in got) == want
    rs = np.random.RandomState(1)
    ctr = rs.randint(0, 2 ** 32, size=(4, 16), dtype=np.uint64)
    got = NR.philox_blocks(ctr[0], ctr[1], ctr[2], ctr[3], SEED & PR.MASK, SEED >> 32)
    for i in range(16):
        want = PR.philox4x32_10([int(ctr[k, i]) for k in range(4)], (SEED & PR.MASK, SEED >> 32))
        assert tuple(int(got[k][i]) for k in range(4)) == want


def test_a_draw_depends_on_seed_actor_step_component_alone():
    base, step = 2 ** 32 - 9, 2 ** 32 - 2                     # (the top actor ids, a carry into the high step word)
    big = NR.draws(SEED, base, step, 5, 9, 7)
    for T, n, A, da, ds in ((1, 1, 1, 0, 0), (2, 3, 6, 4, 1), (5, 2, 4, 7, 0), (3, 9, 2, 0, 2)):
        small = NR.draws(SEED, base + da, step + ds, T, n, A)
        assert np.array_equal(small, big[ds:ds + T, da:da + n, :A]), (T, n, A)
    # the counter and key words as the header states them, and the two Box-Muller pairs of a block
    g, s = base + 3, step + 4
    x = PR.philox4x32_10((g, s & PR.MASK, s >> 32, 1), (SEED & PR.MASK, SEED >> 32))
    u = [((w >> 8) + 0.5) * 2.0 ** -24 for w in x]
    want = [np.sqrt(-2 * np.log(u[0])) * np.cos(2 * np.pi * u[1]), np.sqrt(-2 * np.log(u[0])) * np.sin(2 * np.pi * u[1]),
            np.sqrt(-2 * np.log(u[2])) * np.cos(2 * np.pi * u[3]), np.sqrt(-2 * np.log(u[2])) * np.sin(2 * np.pi * u[3])]
    got = NR.normal(SEED, g, s, np.arange(4, 8))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
    assert not np.array_equal(NR.draws(SEED + 1, 0, 0, 2, 3, 4), NR.draws(SEED, 0, 0, 2, 3, 4))


def test_moments_and_bound_of_the_restatement():
    z = NR.draws(SEED, 0, 0, 64, 1024, 16)                    # 2^20 draws
    assert z.size == 2 ** 20
    NR.moments_ok(z)
    assert abs(NR.BOUND - 5.887) < 1e-3
    # the extreme words give the bound and stay finite: u0 = 2^-25 at x = 0
    assert np.isclose(np.sqrt(-2 * np.log((0 + 0.5) * 2.0 ** -24)), NR.BOUND)


def test_noise_struct_layout_matches_the_ctypes_mirror(tmp_path):
    """struct smx_noise_stream (by tag: the ABI test's typedef list does not see it) and the blocks that embed it, right
    in front of `mon`"""
    from surreal_amd import _lib as L
    pairs = [('struct smx_noise_stream', L.NoiseStream), ('struct smx_synth_lstm_rollout', L.SynthLstmRollout),
             ('struct smx_synth_ppo_window_rollout', L.SynthPpoWindowRollout),
             ('struct smx_ddpg_pixel_step', L.DdpgPixelStep),
             ('struct smx_synth_ppo_pixel_window_step', L.SynthPpoPixelWindowStep),
             ('smx_synth_rollout_t', L.SynthRollout), ('smx_ddpg_rollout_t', L.DdpgRollout),
             ('smx_synth_act_step_t', L.SynthActStep)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "surreal_amd.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append('  printf("%s|sizeof|%%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('  printf("%s|%s|%%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        c, f, v = ln.split('|')
        got[(c, f)] = int(v)
    for cname, cls in pairs:
        assert got[(cname, 'sizeof')] == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
    assert ctypes.sizeof(L.NoiseStream) == 32
    for cls in (L.SynthRollout, L.DdpgRollout, L.SynthActStep, L.SynthPpoPixelWindowStep):
        assert cls._fields_[-2][0] == 'noise' and cls._fields_[-1][0] == 'mon'


def test_every_sampling_launch_takes_the_noise_keyword_and_no_stream_passes_none():
    from surreal_amd import kernels as KN
    from surreal_amd.env import SyntheticVecEnv
    for name in ('synth_act_env_step', 'synth_act_env_step_head', 'synth_rollout', 'synth_lstm_rollout',
                 'synth_ppo_window_rollout', 'synth_ppo_pixel_window_step', 'synth_ddpg_rollout', 'synth_ddpg_step',
                 'synth_ddpg_pixel_step'):
        p = inspect.signature(getattr(KN.HipKernels, name)).parameters
        assert p['noise'].default is None and p['monitor'].default is None, name
    q = KN.HipKernels._noise_args(None)
    assert (q.seed, q.actor_base, q.step, q.enabled) == (0, 0, 0, 0)
    q = KN.HipKernels._noise_args((SEED, 7, 2 ** 40))
    assert (q.seed, q.actor_base, q.step, q.enabled) == (SEED, 7, 2 ** 40, 1)
    # an env without a stream hands the launches no keyword: kernels objects that know none are called as before

    class NoKernels(object):
        pass
    venv = SyntheticVecEnv(3, 4, 2, episode_len=5, device='cpu', kernels=NoKernels())
    assert venv._noi(4, True) == {} and venv.noise is None
    noise = venv.attach_noise(SEED, actor_base=9)
    assert venv._noi(4, True) == {'noise': (SEED, 9, 0)} and noise.step == 4
    assert venv._noi(3, False) == {} and noise.step == 7          # (an explicit eps: the clock still moves)
    venv.reset()
    assert noise.step == 7
    noise.step = 2
    assert noise.at() == (SEED, 9, 2) and noise.at(5) == (SEED, 9, 7)
    assert venv.detach_noise() is noise and venv._noi(1, True) == {}
