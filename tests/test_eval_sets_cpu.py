"""CPU tier: several parameter snapshots in one evaluation launch (DeviceEvalSnapshots) where no kernel is needed -- the
snapshot's size against a closed form written out here (eval_sets_cases.snapshot_layout), the new structs against the C
compiler's layout, the C entry points' argument checks (host code), and, with the launches stubbed by a CPU double, the
Python refusals (raised before anything is launched), the slot bookkeeping, what evaluate() hands the launch, and the
state_dict round trip."""
import ctypes
import itertools
import os
import subprocess

import pytest
import torch

import device_eval_cases as EV
import eval_sets_cases as ES
from reach_resets_cpu_kernels import ResetsCpuKernels
from surreal_amd import _lib as L
from surreal_amd import kernels as KN


class SetsStubKernels(ResetsCpuKernels):
    """the torch-CPU double with the snapshot store and the multi-set launches stubbed: a store writes a serial number
    into the blob's first float (and zeros behind it), a launch fills returns[s, a, i] = 1000 serial(s) + 100 a + i; the
    shape and size queries are the library's own (host code)"""
    synth_eval_supported = KN.HipKernels.synth_eval_supported
    eval_snapshot_floats = KN.HipKernels.eval_snapshot_floats
    _task_id = staticmethod(KN.HipKernels._task_id)

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.lib = L.load()
        self.stores, self.launches = [], []

    def synth_ppo_eval(self, *a, **kw):                 # (can_evaluate asks for them; nothing here launches one)
        raise AssertionError('a single-set launch')
    synth_ddpg_eval = synth_ppo_eval

    def eval_snapshot_store(self, blob, model=None, actor=None, zfilter=None):
        need = self.eval_snapshot_floats(model=model, zfilter=zfilter is not None) if actor is None else \
            self.eval_snapshot_floats(actor=actor)
        assert blob.numel() == need and blob.is_contiguous()
        self.stores.append(dict(ddpg=actor is not None, zfilter=zfilter))
        blob.zero_()
        blob[0] = float(len(self.stores))

    def _launch(self, kind, blobs, init_state, episodes, episode_len, returns, kw):
        n, sets = init_state.shape[0], blobs.shape[0]
        assert tuple(returns.shape) == (sets, n, episodes) and returns.dtype == torch.float64
        self.launches.append(dict(kw, kind=kind, n=n, sets=sets, episodes=episodes, episode_len=episode_len))
        returns.copy_(1000.0 * blobs[:, 0].double()[:, None, None] +
                      100.0 * torch.arange(n, dtype=torch.float64)[None, :, None] +
                      torch.arange(episodes, dtype=torch.float64)[None, None, :])

    def synth_ppo_eval_sets(self, model, blobs, init_state, episodes, episode_len, returns, **kw):
        self._launch('ppo', blobs, init_state, episodes, episode_len, returns, kw)

    def synth_ddpg_eval_sets(self, net, blobs, init_state, episodes, episode_len, returns, **kw):
        self._launch('ddpg', blobs, init_state, episodes, episode_len, returns, kw)


@pytest.fixture
def stub():
    prev = KN.set_default_kernels(SetsStubKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


# ---- the snapshot's size -------------------------------------------------------------------------------------------------------

def test_snapshot_floats_match_the_closed_form():
    lib = L.load()
    floats, sup = lib.smx_eval_snapshot_floats, lib.smx_synth_eval_supported
    seen = 0
    hidden = [(32, 32), EV.RAGGED, (300, 200), (64, 28), (29, 20), (28, 22), (30, 32), (32, 644)]
    for (D, A), (H1, H2), H, zf in itertools.product([(6, 2), (3, 1), (63, 21), (17, 6), (7, 2), (66, 22), (17, 33)],
                                                      hidden, (0, 12, 10, 128, 132), (0, 1)):
        for ddpg in (0, 1):
            accepted = any(sup(ddpg, task, D, H, H1, H2, A) for task in (0, 1)) and not (ddpg and zf)
            got = floats(ddpg, D, H, H1, H2, A, zf)
            if not accepted:
                assert got == 0, (ddpg, D, H, H1, H2, A, zf)
                continue
            seen += 1
            lay = ES.snapshot_layout(ddpg, D, H, H1, H2, A, zf)
            assert got == lay['total'] and got % 64 == 0 and got - lay['end'] < 64, (ddpg, D, H, H1, H2, A, zf)
            assert all(v % 4 == 0 for k, v in lay.items() if k != 'end')        # every block on 16 bytes
            if ddpg:
                assert got == lib.smx_param_noise_copy_floats(D, H1, H2, A, 0)
    assert seen > 60
    # the policies of the GPU tier, the ragged pair among them, and its refused neighbours
    for p in EV.POLICIES:
        dims = ES.policy_dims(p)
        for zf in ((0,) if dims[0] else (0, 1)):
            assert floats(*dims, zf) == ES.snapshot_floats(*dims, zf) > 0, p.id
    h1, h2 = EV.RAGGED
    for ddpg in (0, 1):
        for d1, d2 in ((1, 0), (0, 1), (2, 0), (0, 2), (-1, 0), (0, -2)):
            assert floats(ddpg, 6, 0, h1 + d1, h2 + d2, 2, 0) == 0
    assert floats(1, 6, 12, 32, 32, 2, 0) == 0 and floats(0, 6, 10, 32, 32, 2, 0) == 0 and floats(0, 6, 0, 32, 32, 2, 2) == 0
    assert floats(1, 6, 0, 32, 32, 2, 1) == 0 and floats(0, 6, -4, 32, 32, 2, 0) == 0
    # the blocks a z-filter and an LSTM add
    assert floats(0, 6, 0, 32, 32, 2, 1) >= floats(0, 6, 0, 32, 32, 2, 0) == floats(1, 6, 0, 32, 32, 2, 0)
    lay = ES.snapshot_layout(0, 6, 12, 32, 32, 2, 0)
    assert lay['end'] - lay['lstm'] == lib.smx_lstm_rollout_packed_floats(6, 12) == 4 * ES._pack_words(48, 8 + 12) + 48
    assert floats(0, 6, 12, 32, 32, 2, 0) > floats(0, 12, 0, 32, 32, 2, 0)


def test_bindings_match_the_header_structs(tmp_path):
    """struct smx_eval_sets / smx_eval_snapshot_src as the C compiler lays them out against their ctypes mirrors"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pairs = (('struct smx_eval_sets', L.EvalSets), ('struct smx_eval_snapshot_src', L.EvalSnapshotSrc))
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
    assert [f for f, _ in L.EvalSets._fields_] == ['blobs', 'stride', 'sets', 'zfilter']


def test_entry_points_refuse_before_any_launch():
    ES.check_entry_point_codes()


# ---- DeviceEvalSnapshots with the launches stubbed ------------------------------------------------------------------------------

def test_refusals_come_before_any_store_or_launch(stub):
    snaps, refused, ctx = ES.check_python_refusals('cpu', stub)
    assert stub.stores == [] and stub.launches == []
    snaps.store(0)
    snaps.store(1)
    ES.check_evaluate_refusals(snaps, refused, ctx, 'cpu')
    assert len(stub.stores) == 2 and stub.launches == []


def test_a_kernels_object_without_the_launches_is_refused():
    class Old(ResetsCpuKernels):
        synth_eval_supported = KN.HipKernels.synth_eval_supported
        _task_id = staticmethod(KN.HipKernels._task_id)
        lib = L.load()
        synth_ppo_eval = synth_ddpg_eval = lambda self, *a, **kw: None
    prev = KN.set_default_kernels(Old(), 'cpu')
    try:
        p = EV.BY_ID['mlp-reach-J2']
        venv = EV.make_env(p, 4, 3, 'cpu', KN.default_kernels())
        with pytest.raises(NotImplementedError, match='eval_snapshot_floats'):
            venv.eval_snapshots(EV.make_agent(p, 4)[0], 2)
    finally:
        KN.set_default_kernels(*prev)


def test_slots_streams_and_what_the_launch_is_handed(stub):
    p = EV.BY_ID['lstm-reach-J2']
    n, L_ = 5, 4
    venv = EV.make_env(p, n, L_, 'cpu', stub)
    venv.attach_monitor(capacity=2)
    noise, resets = venv.attach_noise(EV.NSEED), venv.attach_resets(EV.RSEED)
    venv.reset()
    state, mon = venv.state.clone(), venv.monitor._buf.clone()
    ags = ES.agents(p, n, mode='eval_stochastic_local')
    snaps = venv.eval_snapshots(ags[0], 4)
    assert tuple(snaps.buf.shape) == (4, ES.snapshot_floats(*ES.policy_dims(p), 1)) == (4, snaps.stride)
    assert snaps.buf.dtype == torch.float32 and not snaps.buf.any()
    for slot, a in ((2, ags[0]), (0, ags[1]), (1, None)):               # serials 1, 2, 3 in slots 2, 0, 1
        snaps.store(slot, a)
    assert snaps.stored == [True, True, True, False]
    assert [s['zfilter'] for s in stub.stores] == [ags[0].model.z_filter, ags[1].model.z_filter, ags[0].model.z_filter]
    out = snaps.evaluate(3, count=3, resets=(7, 2 ** 32 - 2, 2 ** 32 - n), noise=(9, 11), actors_per_workgroup=8)
    assert out.dtype == torch.float64 and tuple(out.shape) == (3, n, 3)
    assert out[:, 2, 1].tolist() == [2201.0, 3201.0, 1201.0]
    (call,) = stub.launches
    assert call == dict(kind='ppo', n=n, sets=3, episodes=3, episode_len=L_, task='reach', zfilter=ags[0].model.z_filter,
                        resets=(7, 2 ** 32 - n, 2 ** 32 - 2), noise=(9, 0, 11), actors_per_workgroup=8)
    # a window of slots, into a caller's tensor
    again = torch.empty(2, n, 1, dtype=torch.float64)
    assert snaps.evaluate(first=1, count=2, noise=(9, 0), out=again) is again
    assert again[:, 0, 0].tolist() == [3000.0, 1000.0] and stub.launches[1]['sets'] == 2
    with pytest.raises(ValueError, match='never stored'):
        snaps.evaluate(first=2, noise=(9, 0))                            # (count None: up to the last slot, 3)
    # pure: nothing of the env moved
    assert torch.equal(venv.state, state) and torch.equal(venv.monitor._buf, mon) and venv.t == 0
    assert (noise.step, resets.episode) == (0, 1) and venv._ppo == {} and all(a._batch_cells is None for a in ags)
    # DDPG: no z-filter in the snapshot, none handed on
    d = EV.BY_ID['ddpg-reach-J2']
    dsnaps = venv.eval_snapshots(EV.make_agent(d, n)[0], 1)
    dsnaps.store(0)
    assert tuple(dsnaps.buf.shape) == (1, ES.snapshot_floats(*ES.policy_dims(d), 0)) and stub.stores[-1]['ddpg']
    dsnaps.evaluate(2)
    assert stub.launches[-1] == dict(kind='ddpg', n=n, sets=1, episodes=2, episode_len=L_, task='reach', resets=None,
                                     actors_per_workgroup=0)


def test_state_dict_round_trip(stub):
    p = EV.BY_ID['mlp-reach-J2']
    n = 4
    venv = EV.make_env(p, n, 3, 'cpu', stub)
    agent = EV.make_agent(p, n)[0]
    a = venv.eval_snapshots(agent, 3)
    a.store(2)
    a.store(0)
    sd = a.state_dict()
    assert set(sd) == {'buf', 'stored'} and sd['stored'] == [True, False, True]
    b = venv.eval_snapshots(agent, 3)
    b.load_state_dict(sd)
    a.store(1)                                                      # (the copy no longer follows the source)
    assert b.stored == [True, False, True] and torch.equal(b.buf, sd['buf']) and not torch.equal(a.buf, b.buf)
    assert torch.equal(a.evaluate(2, first=2, count=1), b.evaluate(2, first=2, count=1))
    with pytest.raises(ValueError, match='never stored'):
        b.evaluate()
    with pytest.raises(ValueError, match='checkpoint'):
        venv.eval_snapshots(agent, 2).load_state_dict(sd)


def test_a_parameter_noise_view_is_zero_copy_and_read_only(stub):
    import types
    p = EV.BY_ID['ddpg-reach-J2']
    n = 8
    venv = EV.make_env(p, n, 3, 'cpu', stub)
    agent = EV.make_agent(p, n, mode='training')[0]
    floats = stub.eval_snapshot_floats(actor=agent.model.actor)
    pn = types.SimpleNamespace(agent=agent, agents=2, ln=False, pop=torch.zeros(2, floats))
    from surreal_amd.env import DeviceEvalSnapshots
    venv.param_noise = pn                                           # (attached: the population itself is what is evaluated)
    snaps = DeviceEvalSnapshots.from_param_noise(venv, pn)
    assert snaps.buf is pn.pop and snaps.stored == [True, True] and snaps.capacity == 2
    pn.pop[:, 0] = torch.tensor([5.0, 6.0])
    assert snaps.evaluate(1)[:, 1, 0].tolist() == [5100.0, 6100.0] and stub.launches[-1]['kind'] == 'ddpg'
    with pytest.raises(ValueError, match='parameter-noise population'):
        snaps.store(0)
    with pytest.raises(NotImplementedError, match='LayerNorm'):
        DeviceEvalSnapshots.from_param_noise(venv, types.SimpleNamespace(agent=agent, agents=2, ln=True, pop=pn.pop))
    with pytest.raises(ValueError, match='floats'):
        DeviceEvalSnapshots.from_param_noise(venv, types.SimpleNamespace(agent=agent, agents=2, ln=False,
                                                                         pop=torch.zeros(2, floats - 64)))
    assert stub.stores == []
