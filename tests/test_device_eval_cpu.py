"""CPU tier: evaluation on the device (SyntheticVecEnv.evaluate, DeviceEvaluator) where no kernel is needed -- the Python
refusals (raised before anything is launched), what evaluate() hands the launch, DeviceEvaluator's reporting with the launch
stubbed, the host restatement test_gpu_device_eval.py compares the kernels with against SyntheticEnv stepped with zero
actions, the C entry points' argument checks (host code), and the bindings against the header."""
import numpy as np
import pytest
import torch

import device_eval_cases as EV
from reach_resets_cpu_kernels import ResetsCpuKernels
from surreal_amd import _lib as L
from surreal_amd import kernels as KN
from surreal_amd.env.synthetic_env import SyntheticEnv


class EvalStubKernels(ResetsCpuKernels):
    """the torch-CPU double with the evaluation launches stubbed: a launch is recorded and fills the returns with
    100 a + i; the shape query is the library's own (host code)"""
    synth_eval_supported = KN.HipKernels.synth_eval_supported
    _task_id = staticmethod(KN.HipKernels._task_id)

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.lib = L.load()
        self.launches = []

    def _launch(self, kind, init_state, episodes, episode_len, returns, kw):
        n = init_state.shape[0]
        self.launches.append(dict(kw, kind=kind, n=n, episodes=episodes, episode_len=episode_len))
        returns.copy_(100.0 * torch.arange(n, dtype=torch.float64)[:, None] + torch.arange(episodes, dtype=torch.float64))

    def synth_ppo_eval(self, model, packed, lstm_packed, init_state, episodes, episode_len, returns, **kw):
        assert packed.numel() == self.epoch_packed_numel(model.actor) and (lstm_packed is not None) == bool(model.if_rnn)
        self._launch('ppo', init_state, episodes, episode_len, returns, kw)

    def synth_ddpg_eval(self, net, packed, init_state, episodes, episode_len, returns, **kw):
        assert packed.numel() == self.epoch_packed_numel(net)
        self._launch('ddpg', init_state, episodes, episode_len, returns, kw)


@pytest.fixture
def stub():
    prev = KN.set_default_kernels(EvalStubKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


def test_refusals_come_before_any_launch(stub):
    EV.check_python_refusals('cpu', stub)
    assert stub.launches == []


def test_a_kernels_object_without_the_launch_is_refused():
    prev = KN.set_default_kernels(ResetsCpuKernels(), 'cpu')
    try:
        p = EV.BY_ID['mlp-reach-J2']
        agent, _ = EV.make_agent(p, 4)
        venv = EV.make_env(p, 4, 3, 'cpu', KN.default_kernels())
        assert not venv.can_evaluate(agent)
        with pytest.raises(NotImplementedError, match='synth_ppo_eval'):
            venv.evaluate(agent)
    finally:
        KN.set_default_kernels(*prev)


def test_evaluate_hands_the_launch_the_streams_and_touches_nothing(stub):
    p = EV.BY_ID['lstm-reach-J2']
    n, L_ = 5, 4
    venv = EV.make_env(p, n, L_, 'cpu', stub)
    venv.attach_monitor(capacity=2)
    noise, resets = venv.attach_noise(EV.NSEED), venv.attach_resets(EV.RSEED)
    venv.reset()
    state, mon, open_ddpg = venv.state.clone(), venv.monitor._buf.clone(), dict(venv._ddpg)
    agent, _ = EV.make_agent(p, n, mode='eval_stochastic_local')
    out = venv.evaluate(agent, 3, resets=(7, 2 ** 32 - 2, 2 ** 32 - n), noise=(9, 11), actors_per_workgroup=8)
    assert out.dtype == torch.float64 and tuple(out.shape) == (n, 3) and out[2, 1] == 201.0
    (call,) = stub.launches
    assert call == dict(kind='ppo', n=n, episodes=3, episode_len=L_, task='reach', zfilter=agent.model.z_filter,
                        resets=(7, 2 ** 32 - n, 2 ** 32 - 2), noise=(9, 0, 11), actors_per_workgroup=8)
    assert torch.equal(venv.state, state) and torch.equal(venv.monitor._buf, mon) and venv.t == 0
    assert (noise.step, resets.episode) == (0, 1) and agent._batch_cells is None and venv._ppo == {} and venv._ddpg == open_ddpg
    again = torch.empty(n, 2, dtype=torch.float64)
    det, _ = EV.make_agent(EV.BY_ID['ddpg-reach-J2'], n)
    assert venv.evaluate(det, 2, out=again) is again
    assert stub.launches[1] == dict(kind='ddpg', n=n, episodes=2, episode_len=L_, task='reach', resets=None,
                                    actors_per_workgroup=0)


def test_device_evaluator_reports_what_host_eval_monitors_would(stub):
    from surreal_amd.env import DeviceEvaluator
    from surreal_amd.learner.base import ScalarRecorder
    p = EV.BY_ID['mlp-reach-J2']
    n, E, L_ = 3, 3, 4
    for separate in (False, True):
        agent, (lc, ec, sc) = EV.make_agent(p, n)
        sc.tensorplex.update_schedule.eval_env = 2
        order = []
        agent.fetch_parameter = lambda: order.append('fetch')
        venv = EV.make_env(p, n, L_, 'cpu', stub)
        real = venv.evaluate
        venv.evaluate = lambda *a, **kw: (order.append('evaluate'), real(*a, **kw))[1]
        de = DeviceEvaluator(venv, agent, sc, E, resets=(EV.RSEED, 5), eval_id_base=40, separate_plots=separate)
        got = [de.run() for _ in range(3)]
        assert order == ['fetch', 'evaluate'] * 3
        assert all(g.dtype == np.float64 and g.shape == (n, E) and g[1, 2] == 102.0 for g in got)
        assert stub.launches[-1]['resets'] == (EV.RSEED, 0, 5)
        EV.check_reports(de, [[100.0 * i + e for e in range(E)] * 3 for i in range(n)], 40, sc, separate)
        assert de.mean_return() == np.mean([100.0 * i + e for i in range(n) for e in range(E)]) and de.step_per_s > 0
    # one shared tensorplex object: every report goes to it
    rec = ScalarRecorder()
    de = DeviceEvaluator(venv, agent, sc, E, tensorplex=rec)
    de.run()
    assert len(rec.history) == n and [s for s, _ in rec.history] == [2] * n
    # a sampling agent: the noise stream moves on by the run's steps
    agent, (lc, ec, sc) = EV.make_agent(p, n, mode='eval_stochastic_local')
    agent.fetch_parameter = lambda: None
    de = DeviceEvaluator(venv, agent, sc, E, noise=(EV.NSEED, 10))
    de.run(), de.run()
    assert [c['noise'] for c in stub.launches[-2:]] == [(EV.NSEED, 0, 10), (EV.NSEED, 0, 10 + E * L_)]
    with pytest.raises(ValueError):
        DeviceEvaluator(venv, agent, sc, 0)


@pytest.mark.parametrize('J', [1, 2, 21])
def test_host_restatement_is_the_host_env_stepped_with_zero_actions(J):
    """host_returns (tasks.reach_step from tasks.reach_reset_state) against SyntheticEnv(task='reach', resets=(seed,
    actor_id)) stepped with zero actions: the same fp32 rewards, summed in fp64 in step order"""
    p = EV.Policy('host', 'mlp', 'reach', 3 * J, J, (32, 32))
    n, E, L_ = 3, 3, 7
    for first, base in ((0, 0), (2 ** 32 - 2, 2 ** 32 - n)):
        want = EV.host_returns(p, n, E, L_, 0.0, (EV.RSEED, first, base))
        for a in range(n):
            env = SyntheticEnv(3 * J, J, episode_len=L_, task='reach', resets=(EV.RSEED, base + a))
            env.episode = first
            for i in range(E):
                env._reset()
                total, done = 0.0, False
                while not done:
                    _, r, done, _ = env._step(np.zeros(J, np.float32))
                    total = total + r
                assert EV.same_f64(total, want[a, i]), (J, first, a, i)
    assert (want < 0).all() and len({w.tobytes() for w in want.reshape(-1)}) == n * E
    # from init_state, and on drift from the host env's own episode
    init = np.stack([np.random.RandomState(s).randn(3 * J).astype(np.float32) for s in range(n)])
    fixed = EV.host_returns(p, n, 2, L_, 0.0, None, init)
    assert EV.same_f64(fixed[:, 0], fixed[:, 1])
    drift = EV.host_returns(EV.BY_ID['mlp-drift-17-6'], n, 2, L_, 0.3, None, None)
    assert EV.same_f64(drift[:, 0], drift[:, 1]) and np.isfinite(drift).all()


def test_entry_points_refuse_before_any_launch():
    EV.check_entry_point_codes()
    assert L.load().smx_abi_version() == 2


def test_the_ragged_pair_is_at_the_edge_of_what_the_query_accepts():
    """hidden sizes are multiples of 4: (28, 20) -- no multiple of 8 -- is accepted, its odd neighbours are not"""
    sup = L.load().smx_synth_eval_supported
    h1, h2 = EV.RAGGED
    for ddpg in (0, 1):
        assert sup(ddpg, 1, 6, 0, h1, h2, 2) == 1
        for d1, d2 in ((1, 0), (0, 1), (2, 0), (0, 2), (-1, 0), (0, -2)):
            assert sup(ddpg, 1, 6, 0, h1 + d1, h2 + d2, 2) == 0
    assert h1 % 8 and h2 % 8 and sup(0, 1, 6, 12, h1, h2, 2) == 1


def test_bindings_match_the_header_structs(tmp_path):
    """struct smx_synth_ppo_eval / smx_synth_ddpg_eval as the C compiler lays them out against their ctypes mirrors"""
    import ctypes
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pairs = (('struct smx_synth_ppo_eval', L.SynthPpoEval), ('struct smx_synth_ddpg_eval', L.SynthDdpgEval))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "surreal_amd.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append('  printf("%%zu\\n", sizeof(%s));' % cname)
        for f, _ in cls._fields_:
            lines.append('  printf("%%zu\\n", offsetof(%s, %s));' % (cname, f))
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(root, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, cls in pairs:
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    assert got == want
