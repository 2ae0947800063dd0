"""GPU tier (-m gpu): the 13 kernels of csrc/smx_scan.hip by themselves over the case table of scan_cases.py -- every
slice-trip count of the GAE staging loop, both branches, one to ten lane passes, ragged grids, both sides of the LDS
opt-in and the last N each entry point takes, gae_norm's last-workgroup epilogue on one and on 301 workgroups, the
z-update's chunk regimes, the reward filter's grid cap -- each held against a float64 reference under a derived bound
in buffers whose surroundings are NaN (inputs) or a sentinel (outputs); scan_cases.py says how.  Then what only bits
can show (rows computed alone against the whole batch, the same call twice), every refusal as a return code with nothing
launched, and one learner whose n_step = 1400 takes the LDS opt-in under stream capture.

With SMX_SCAN_MARGINS_OUT set to a path, the run writes the largest share of its bound every case used there
(profiles/scan_case_margins.txt is such a run on an MI355X); writing it is no condition of passing."""
import copy
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import helpers as H
import learn_fold_cases as FC
import scan_cases as SC
from surreal_amd import _lib as L
from surreal_amd import synthetic
from test_gpu_kernels import K  # noqa: F401  (the module-scoped kernels fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def ids(cases):
    return [c.id for c in cases]


@pytest.fixture(scope='module')
def margins():
    rec = {}
    yield rec
    path = os.environ.get('SMX_SCAN_MARGINS_OUT')
    if not path or not rec:
        return
    try:
        worst = {}
        for cid, r in rec.items():
            for q, s in r.items():
                if s > worst.get(q, (-1.0, ''))[0]:
                    worst[q] = (s, cid)
        with open(path, 'w') as f:
            f.write('# tests/test_gpu_scan.py::test_case: the largest share of its bound each quantity of a case used\n')
            f.write('# bounds (scan_cases.py): adv ret zsum zsumsq (d + c) 2^-24 S; mom rf_sums rf_state 2 float32 ulps; norm norm3 '
                    'zmean zstd zfwd zsums rf_out concat 1e-5 + 1e-5 |ref|\n')
            for q in sorted(worst):
                f.write('# worst %-8s %.4f  %s\n' % (q, worst[q][0], worst[q][1]))
            for c in SC.CASES:
                if c.id in rec:
                    f.write(c.id + ' ' + ' '.join('%s=%.4f' % (q, rec[c.id][q]) for q in sorted(rec[c.id])) + '\n')
    except Exception as e:                                     # the report is no condition of passing
        print('scan margins not written: %r' % (e,))


def _kw(K, c):
    return dict(ws_lib=K.zfilter_update_ws_floats) if c.kind == 'zupd' else {}


@pytest.mark.parametrize('c', SC.CASES, ids=ids(SC.CASES))
def test_case(K, c, margins):
    record = SC.run_entry(K, c, DEV, **_kw(K, c))
    print(c.id, ' '.join('%s=%.4f' % kv for kv in sorted(record.items())))
    margins[c.id] = record


# ---------------------------------------------------------------------------------------------------------------------
# bit-level properties
# ---------------------------------------------------------------------------------------------------------------------
ROW_CASES = [c for c in SC.GAE_CASES if c.kind == 'gae' and c.B >= 5 and (c.N >= 600 or c.N in (64, 65, 127, 257))]


@pytest.mark.parametrize('c', ROW_CASES, ids=ids(ROW_CASES))
def test_rows_computed_alone_have_the_bits_they_have_in_the_batch(K, c):
    """rows [b0, b0 + k) in a launch of their own sit in other waves of other workgroups: the same bits"""
    p = SC.problem(c).inputs
    E = c.N - c.H + 1
    whole = SC.gae_bufs(c, p, DEV, False)
    SC.gae_call(K, c, whole, p)
    assert bool(torch.isfinite(whole.v['adv']).all())
    for b0, k in ((0, 1), (1, 3), (3, c.B - 3), (c.B - 1, 1)):
        part = SC.gae_bufs(c, p, DEV, True, rows=(b0, b0 + k))
        SC.gae_call(K, c, part, p)
        for q in ('adv', 'ret'):
            assert torch.equal(SC.bits(whole.v[q]).view(c.B, E)[b0:b0 + k], SC.bits(part.v[q]).view(k, E)), (q, b0, k)
        SC.check_fences(part, c.id)


def test_the_same_calls_twice_give_the_same_bits(K):
    for cid in ('norm-B1201-N19-H19-w-t0', 'zupd-r16385-D65-s1', 'rf-n200001', 'mom-n127000'):
        c = SC.BY_ID[cid]
        if c.kind == 'norm':
            p = SC.problem(c).inputs
            got = []
            for _ in range(2):
                x = SC.gae_bufs(c, p, DEV, True)
                x.out('mom', (3,), 5)
                SC.gae_call(K, c, x, p, norm=True, ticket=torch.zeros(1, dtype=torch.int32, device=DEV))
                got.append(SC.snapshot(x))
            for k in got[0]:
                assert torch.equal(got[0][k], got[1][k]), (cid, k)
        else:
            assert SC.run_entry(K, c, DEV, **_kw(K, c)) == SC.run_entry(K, c, DEV, **_kw(K, c)), cid


def test_learn_epilogue_moments_and_z_update_on_poisoned_buffers(K):
    """learn_epilogue_kernel runs the z-update and the moments roles of smx_learn_epilogue.inc.h in one launch: the bits of
    zupdate_kernel and moments_kernel on the same inputs, and the float64 reference"""
    g = SC._rng('epilogue')
    rows, D, A = 33, 65, 5
    data, ret = SC.f32(2.0 * g.randn(rows, D) + 0.5), SC.f32(1e4 + 1e-2 * g.randn(rows))
    rs0, rsq0 = SC.f32(100.0 * g.randn(D)), SC.f32(5000.0 * g.rand(D) + 300.0)
    sides = []
    for fused in (True, False):
        x = SC.Bufs(DEV)
        xv = SC._strided(x, 'x', data, 1)
        x.inp('ret', ret)
        x.inp('log_var', SC.f32(g.randn(A)) if fused else np.zeros(A, np.float32))
        z = types.SimpleNamespace(running_sum=x.state('rs', rs0, 5), running_sumsq=x.state('rsq', rsq0, 3),
                                  count=x.state('cnt', [1000.0], 5))
        x.out('mom', (3,), 5)
        x.out('out4', (4,), 3)
        ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
        if fused:
            K.learn_epilogue(x.v['ret'], x.v['mom'], x.v['log_var'], x.v['out4'], ticket, zfilter=z, x=xv, count_rows=rows)
            assert int(ticket[0]) == 0 and bool(torch.isfinite(x.v['out4']).all())
        else:
            K.moments(x.v['ret'], x.v['mom'])
            K.zfilter_update(xv, z.running_sum, z.running_sumsq, z.count, rows)
            x.v['out4'].zero_()
        SC.check_fences(x, 'epilogue')
        sides.append(x)
    for k in ('mom', 'rs', 'rsq', 'cnt'):
        assert torch.equal(SC.bits(sides[0].v[k]), SC.bits(sides[1].v[k])), k
    assert SC.ulps32(sides[0].get('mom'), SC.moments64(ret)) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# refusals: a return code, nothing launched
# ---------------------------------------------------------------------------------------------------------------------
def _hip():
    """the HIP runtime this process already has loaded (hipGetLastError is per thread)"""
    for line in open('/proc/self/maps'):
        if 'libamdhip64.so' in line:
            return ctypes.CDLL(line.split()[-1])
    raise AssertionError('no HIP runtime is loaded')


def _refusal_call(K, entry, what):
    """-> (the library call as a closure returning its code, the Bufs whose outputs must keep every byte, the ticket)"""
    lib, st, P = K.lib, K._st(), L.ptr
    x = SC.Bufs(DEV)
    g = np.random.RandomState(7)
    B, N, Hh, rows, D = 3, 8, 8, 6, 5
    if what.startswith('N='):
        N = Hh = int(what[2:])
        B = 1
    ticket = torch.full((1,), 5, dtype=torch.int32, device=DEV)          # (never read: nothing is launched)
    null = what[5:] if what.startswith('null:') else None
    a = {}
    if entry in ('gae', 'norm'):
        for k, shape in (('values', (B, N + 1)), ('rewards', (B, N)), ('dones', (B, N)), ('gpow', (N,)), ('lpow', (N,))):
            a[k] = x.inp(k, SC.f32(g.rand(*shape)))
        for k in ('adv', 'ret'):
            a[k] = x.out(k, (B,))
        a['mom'] = x.out('mom', (3,))
        a['ticket'] = ticket
        Bq, Nq, Hq = (0 if what == 'B=0' else B), N, (0 if what == 'H=0' else N + 1 if what == 'H>N' else Hh)
        q = {k: (None if k == null else P(v)) for k, v in a.items()}
        head = (q['values'], None, q['rewards'], q['dones'], q['gpow'], q['lpow'], 0.99, 0.9, Bq, Nq, Hq, q['adv'], q['ret'])
        if entry == 'gae':
            return (lambda: lib.smx_windowed_gae_returns_f32(*(head + (st,)))), x, ticket
        return (lambda: lib.smx_windowed_gae_norm_f32(*(head + (q['mom'], 1e-4, q['ticket'], st)))), x, ticket
    if entry == 'rf':
        a = dict(rewards=x.inp('rewards', SC.f32(g.rand(9))), out=x.out('out', (9,)), state=x.state('state', SC.RF_STATE0),
                 partials=x.out('partials', (130,), 2, dtype=torch.float64, fill=SC.SENTINEL), ticket=ticket)
        q = {k: (None if k == null else P(v)) for k, v in a.items()}
        if what == 'partials+4':
            q['partials'] = ctypes.c_void_p(a['partials'].data_ptr() + 4)
        return (lambda: lib.smx_reward_filter_f32(q['rewards'], 9, 0.5, 1, q['state'], 1e-5, 1, q['out'], None, q['partials'],
                                                  q['ticket'], st)), x, ticket
    if entry == 'mom':
        a = dict(x=x.inp('x', SC.f32(g.rand(9))), out=x.out('out', (3,)))
        q = {k: (None if k == null else P(v)) for k, v in a.items()}
        return (lambda: lib.smx_moments_f32(q['x'], 9, q['out'], st)), x, ticket
    if entry == 'merge':
        a = dict(parts=x.inp('parts', SC.f32(g.rand(6))), out=x.out('out', (3,)))
        q = {k: (None if k == null else P(v)) for k, v in a.items()}
        return (lambda: lib.smx_moments_merge_f32(q['parts'], 2, q['out'], st)), x, ticket
    if entry == 'advn':
        a = dict(x=x.state('x', SC.f32(g.rand(9))), mom=x.inp('mom', SC.f32([9, 0.5, 1.0])))
        q = {k: (None if k == null else P(v)) for k, v in a.items()}
        return (lambda: lib.smx_adv_normalize_f32(q['x'], 9, q['mom'], 1e-4, st)), x, ticket
    # the z-filter
    # (the workspace entry is told of 16384 rows: it gets them, although ldx < D is refused before any is read)
    a = dict(x=x.inp('x', SC.f32(g.rand(16384 if entry == 'zupd_ws' else rows, D))), rs=x.state('rs', SC.f32(g.rand(D))), rsq=x.state('rsq', SC.f32(g.rand(D) + 1)),
             cnt=x.state('cnt', [10.0]), mean=x.state('mean', SC.f32(g.rand(D))), std=x.state('std', SC.f32(g.rand(D) + 1)),
             out=x.out('out', (rows, D)), ws=x.out('ws', (2 * 32 * D,)))
    q = {k: (None if k == null else P(v)) for k, v in a.items()}
    rq, ldx = (0 if what == 'rows=0' else rows), (D - 1 if what == 'ldx<D' else D)
    if entry == 'zstats':
        return (lambda: lib.smx_zfilter_stats_f32(q['rs'], q['rsq'], q['cnt'], D, 1e-5, q['mean'], q['std'], st)), x, ticket
    if entry == 'zfwd':
        return (lambda: lib.smx_zfilter_forward_f32(q['x'], ldx, rq, D, q['mean'], q['std'], q['out'], st)), x, ticket
    if entry == 'zsums':
        return (lambda: lib.smx_zfilter_forward_sums_f32(q['x'], ldx, rq, D, q['rs'], q['rsq'], q['cnt'], 1e-5, q['out'],
                                                         st)), x, ticket
    if entry == 'zupd':
        return (lambda: lib.smx_zfilter_update_f32(q['x'], ldx, rq, D, q['rs'], q['rsq'], q['cnt'], 6.0, st)), x, ticket
    assert entry == 'zupd_ws'
    return (lambda: lib.smx_zfilter_update_ws_f32(q['x'], ldx, 16384, D, q['rs'], q['rsq'], q['cnt'], 6.0, q['ws'],
                                                  2 * 32 * D, st)), x, ticket


@pytest.mark.parametrize('entry,what,code', SC.REFUSALS, ids=['%s-%s' % (e, w) for e, w, _ in SC.REFUSALS])
def test_a_refusal_is_a_return_code_with_nothing_launched(K, entry, what, code):
    call, x, ticket = _refusal_call(K, entry, what)
    hip = _hip()
    torch.cuda.synchronize()
    hip.hipGetLastError()
    snap = SC.snapshot(x)
    assert call() == code
    torch.cuda.synchronize()
    assert hip.hipGetLastError() == 0
    SC.assert_untouched(x, snap)
    assert int(ticket[0]) == 5
    SC.check_fences(x, what)
    msg = K.lib.smx_error_string(code)
    assert msg and b'unknown' not in msg


# ---------------------------------------------------------------------------------------------------------------------
# learner level: n_step = 1400, eagerly and from the captured graph
# ---------------------------------------------------------------------------------------------------------------------
class Tap(FC.Recording):
    """passes every call on; keeps a copy of what the GAE launch was given"""
    seen = None

    def _keep(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, Hh, values_tail):
        v = values.reshape(-1).clone()
        if values_tail is not None:
            v = torch.cat([v.view(B, N), values_tail.reshape(B, 1)], 1)
        f = lambda t: t.detach().cpu().numpy().copy()  # noqa: E731
        self.seen = dict(values=f(v.view(B, N + 1)), rewards=f(rewards.reshape(B, N)), dones=f(dones.reshape(B, N)),
                         gpow=f(gpow), lpow=f(lpow), gamma=np.float32(gamma), gamma_H=np.float32(gamma_H), H=Hh)

    def gae_norm(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, Hh, adv, ret, mom, min_std, ticket,
                 values_tail=None):
        self._keep(values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, Hh, values_tail)
        self.calls.append('gae_norm')
        return self._inner.gae_norm(values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, Hh, adv, ret, mom, min_std,
                                    ticket, values_tail=values_tail)

    def gae(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, Hh, adv, ret, values_tail=None):
        self._keep(values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, Hh, values_tail)
        self.calls.append('gae')
        return self._inner.gae(values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, Hh, adv, ret,
                               values_tail=values_tail)


def _long_learner(graph):
    case = FC.learner_case('clip', 1e9, B=4, N=1400)
    case['hidden'] = [16, 8]
    shp = case['shape']
    params = synthetic.make_ppo_params(shp['D'], shp['A'], hidden=tuple(case['hidden']), **case['param_args'])
    zstate = synthetic.make_zfilter_state(shp['D'], **case['z_args'])
    return H.make_learner(case, params, zstate, session_overrides={'use_hip_graph': graph}), case


def test_a_learner_with_n_step_1400_learns_the_same_bits_eagerly_and_from_its_graph(K):
    """the one place the LDS opt-in (N = 1400: 67 216 B a workgroup) runs while a stream is being captured"""
    eager, case = _long_learner(False)
    graph, _ = _long_learner(True)
    shp = case['shape']
    assert SC.gae_lds(shp['N']) > SC.GAE_LDS_OPT_IN
    eager.K = tap = Tap(eager.K)
    batch = synthetic.make_ppo_batch(shp['B'], shp['N'], shp['D'], shp['A'], seed=77)
    eager.learn(copy.deepcopy(batch))
    graph.learn(copy.deepcopy(batch))
    torch.cuda.synchronize()
    assert graph._graphs, 'the second learner did not capture a graph'
    assert tap.seen is not None and tap.seen['H'] == shp['N']
    for k in ('adv', 'ret', 'adv_mom'):
        a, b = getattr(eager._ws, k), getattr(graph._ws, k)
        assert bool(torch.isfinite(a).all())
        assert torch.equal(SC.bits(a), SC.bits(b)), k
    for k in ('actor_flat', 'critic_flat'):
        assert torch.equal(SC.bits(getattr(eager.model, k)), SC.bits(getattr(graph.model, k))), k
    assert bool((eager._ws.ticket == 0).all()) and bool((graph._ws.ticket == 0).all())
    # ... and what both hold meets the table's bound against the float64 reference
    want = SC.gae_reference(tap.seen)
    d = SC.gae_depth(shp['N'], shp['N'])
    ret = graph._ws.ret.detach().cpu().numpy().astype(np.float64).reshape(shp['B'], 1)
    s_ret = SC.share(np.abs(ret - want['ret']), SC.sum_bound(d, SC.C_RET, want['S_ret']))
    assert s_ret <= 1.0, s_ret
    adv = graph._ws.adv.detach().cpu().numpy().astype(np.float64).reshape(shp['B'], 1)
    if 'gae_norm' in tap.calls or eager.norm_adv:
        # normalised in float32 from the moments the launch left: undone here, the normalisation's own roundings
        # (two, relative to |adv - mean|) on top of the sum's bound
        n, mean, m2 = graph._ws.adv_mom.detach().cpu().numpy().astype(np.float64)
        den = max(np.sqrt(m2 / (n - 1.0)), SC.MIN_STD)
        raw = adv * den + mean
        bound = SC.sum_bound(d, SC.C_ADV, want['S_adv']) + 4 * SC.U * (np.abs(raw - mean) + np.abs(mean))
    else:
        raw, bound = adv, SC.sum_bound(d, SC.C_ADV, want['S_adv'])
    s_adv = SC.share(np.abs(raw - want['adv']), bound)
    print('n_step 1400 learner: ret %.4f adv %.4f of the bound (%s)' % (s_ret, s_adv, tap.calls.count('gae_norm')))
    assert s_adv <= 1.0, s_adv
