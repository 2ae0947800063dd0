"""CPU tier: the case table of scan_cases.py (csrc/smx_scan.hip: GAE, moments, z-filter, reward filter) on the torch-CPU
double against the float64 reference with the GPU tier's bounds and poisoned buffers, the float32 order emulation inside
every bound, the coverage conditions the table must meet, and proof that its checks can fail: thirteen deliberately
wrong doubles, each of which must break a named case.  test_gpu_scan.py runs the same table objects on the HIP kernels."""
import os

import numpy as np
import pytest
import torch

import scan_cases as SC
from cpu_kernels import TorchCpuKernels
from surreal_amd import _lib as L

C = TorchCpuKernels()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ids(cases):
    return [c.id for c in cases]


def _kw(c):
    # smx_zfilter_update_ws_floats is host arithmetic: the library answers without a GPU
    return dict(ws_lib=lambda rows, D: int(L.load().smx_zfilter_update_ws_floats(rows, D))) if c.kind == 'zupd' else {}


@pytest.mark.parametrize('c', SC.CASES, ids=ids(SC.CASES))
def test_case_on_the_double(c):
    SC.run_entry(C, c, **_kw(c))


@pytest.mark.parametrize('c', SC.GAE_CASES, ids=ids(SC.GAE_CASES))
def test_the_float32_order_emulation_stays_inside_the_bound(c):
    P = SC.problem(c)                                          # (asserts it)
    assert 0.0 <= max(P.emu_share.values()) <= 1.0


def test_ids_are_unique_and_the_table_stays_small():
    assert len(set(ids(SC.CASES))) == len(SC.CASES)
    assert 90 <= len(SC.CASES) <= 130
    for c in SC.GAE_CASES:
        assert c.B * (c.N + 1) <= 40000 and SC.path(c)['accepted'], c.id
    assert max(c.B * c.N for c in SC.CASES if c.kind == 'zupd') == 131584 * 65       # the largest tensor: 34 MB


def test_the_gpu_file_runs_the_same_table_and_marks_nothing_to_skip():
    src = open(os.path.join(ROOT, 'tests', 'test_gpu_scan.py')).read()
    assert "parametrize('c', SC.CASES" in src
    assert 'skip' not in src and 'xfail' not in src


def test_the_reference_on_a_case_small_enough_to_do_by_hand():
    # B = 1, N = 2, H = 1: two windows; done after step 0 masks values[1]
    p = dict(values=SC.f32([[2.0, 4.0, 8.0]]), rewards=SC.f32([[1.0, 3.0]]), dones=SC.f32([[1.0, 0.0]]),
             gpow=SC.f32([1.0, 0.5]), lpow=SC.f32([1.0, 0.25]), gamma=np.float32(0.5), gamma_H=np.float32(0.5), H=1)
    w = SC.gae_reference(p)
    assert w['adv'].tolist() == [[1.0 + 0.0 - 2.0, 3.0 + 4.0 - 0.0]] and w['ret'].tolist() == [[1.0 + 0.0, 3.0 + 4.0]]
    assert w['S_adv'].tolist() == [[3.0, 7.0]] and w['S_ret'].tolist() == [[1.0, 7.0]]
    p['H'] = 2                                                 # one window of two terms, bootstrap v[2] gamma_H
    w = SC.gae_reference(p)
    assert w['adv'].tolist() == [[-1.0 + 0.5 * 0.25 * 7.0]] and w['ret'].tolist() == [[1.0 + 0.5 * 3.0 + 8.0 * 0.5]]
    a, r = SC.gae_emulation(p)
    assert a.tolist() == w['adv'].tolist() and r.tolist() == w['ret'].tolist()


# ---- the restated host side and the coverage conditions ---------------------------------------------------------------------
def test_path_restates_the_host_side():
    g = lambda N, H=None, B=1, kind='gae': SC.path(SC.Case('x', kind, B, N, H or N, 'w', 'none', ''))  # noqa: E731
    assert [g(N)['trips'] for N in (1, 255, 256, 511, 512, 1365, 3413)] == [1, 1, 2, 2, 3, 6, 14]
    assert g(64, 1)['passes'] == 1 and g(65, 1)['passes'] == 2 and g(600, 7)['passes'] == 10 and g(5)['branch'] == 'one'
    assert not g(1023)['optin'] and g(1024)['optin'] and not g(1023, kind='norm')['optin'] and g(1024, kind='norm')['optin']
    assert g(3413)['accepted'] and not g(3414)['accepted'] and g(3413)['lds'] == 160 * 1024
    assert g(2730, kind='norm')['accepted'] and not g(2731, kind='norm')['accepted']
    assert [g(5, B=B)['grid'] for B in (1, 4, 5, 1201)] == [1, 1, 2, 301]
    lib = L.load()
    for rows in (1, 16383, 16384, 16385, 16895, 33000, 131071, 131072, 131584, 10 ** 6):
        for D in (1, 5, 65, 376):
            assert int(lib.smx_zfilter_update_ws_floats(rows, D)) == SC.zupdate_ws_floats(rows, D), (rows, D)
    assert SC.zupdate_chunks(16385) == 32 and -(-16385 // 32) == 513 and SC.zupdate_regime(16385) == 'ragged'
    assert SC.zupdate_chunks(131584) == 256 and SC.zupdate_regime(131584) == 'capped' and SC.zupdate_regime(131072) == 'even'
    assert int(lib.smx_reward_filter_partials()) == 128 and SC.reward_grid(65536) == 64 == SC.reward_grid(65537)
    assert SC.reward_grid(65535) == 64 and SC.reward_grid(1025) == 2 and SC.reward_grid(1024) == 1


def test_the_table_covers_every_path():
    gae = [c for c in SC.CASES if c.kind == 'gae']
    norm = [c for c in SC.CASES if c.kind == 'norm']
    P = SC.path
    assert {P(c)['trips'] for c in gae} >= {1, 2, 3, 6, 14}
    assert {P(c)['branch'] for c in gae} == {'one', 'sliding'} == {P(c)['branch'] for c in norm}
    passes = {P(c)['passes'] for c in gae}
    assert {1, 2} <= passes and max(passes) > 4
    for cases in (gae, norm):                                  # opt-in on and off, at the boundary, and the last N accepted
        assert {P(c)['optin'] for c in cases} == {True, False}
        assert {c.N for c in cases} >= {1023, 1024}
        assert any(not P(c._replace(N=c.N + 1, H=c.N + 1))['accepted'] for c in cases)
    assert {c.N for c in gae if c.H == c.N} >= {1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1365, 1366, 3413}
    assert {(c.N, c.H) for c in gae} >= {(64, 1), (65, 1), (127, 64), (128, 64), (129, 65), (300, 1), (600, 530), (600, 7),
                                          (1400, 1336), (1400, 1335)}
    assert {c.N - c.H + 1 for c in gae} >= {64, 65, 71, 300, 594}
    for side in (lambda c: c.N < 256, lambda c: c.N >= 256):   # every B mod 4 on both sides of the first slice edge
        assert {c.B % 4 for c in gae if side(c)} == {0, 1, 2, 3}
        assert {c.B % 4 for c in gae if side(c) and c.H == c.N} >= {0, 1, 3}
    assert any(c.B % 4 and c.N - c.H + 1 > 1 and c.N > 256 for c in gae)            # ragged grid, windows, a long row
    assert {c.dones for c in gae} >= {'rand', 'none', 'all', 't0', 'last', 'edge'}
    assert {c.gam for c in gae if c.N > 256} == {'w', 'l'}
    assert {c.N for c in norm if c.H == c.N} >= {3, 257, 1023, 1024, 2730} and (1201, 19) in {(c.B, c.N) for c in norm}
    assert {c.B for c in norm if P(c)['grid'] == 1} >= {1, 2, 3, 4}
    assert any(c.dones == 'const' for c in norm) and any(c.B * (c.N - c.H + 1) == 1 for c in norm)
    by = lambda k: [c for c in SC.CASES if c.kind == k]  # noqa: E731
    assert {c.N for c in by('mom')} == {1, 2, 63, 64, 65, 1023, 1024, 1025, 127000}
    assert {(c.B, c.dones) for c in by('merge')} >= {(1, None), (2, None), (8, None), (8, 0), (8, 4), (8, 7)}
    assert {c.N for c in by('advn')} >= {1, 2048 * 256 + 3}
    assert {(c.N, c.H) for c in by('zfwd')} == {(D, s) for D in (1, 63, 64, 65, 129, 257, 376) for s in (0, 1)}
    one = {c.B for c in by('zupd') if SC.zupdate_regime(c.B) == 'one'}
    assert one >= {1, 15, 16, 17, 31, 32, 33, 16383}
    assert {(c.B, c.N) for c in by('zupd') if c.B >= 16384} == {(r, D) for r in (16384, 16385, 16895, 33000, 131072, 131584)
                                                                for D in (5, 65)}
    assert {SC.zupdate_regime(c.B) for c in by('zupd')} == {'one', 'even', 'ragged', 'capped'}
    assert {c.H for c in by('zupd')} == {0, 1}
    assert {c.N for c in by('rf')} == {1, 1023, 1024, 1025, 65535, 65536, 65537, 200001}


def test_the_refusals_cover_every_code_and_every_required_pointer():
    R = SC.REFUSALS
    assert len(set(R)) == len(R)
    assert ('gae', 'N=3414', SC.E_UNSUPPORTED) in R and ('norm', 'N=2731', SC.E_UNSUPPORTED) in R
    for e in ('gae', 'norm'):
        assert {w for ee, w, code in R if ee == e and code == SC.E_SHAPE} == {'H=0', 'H>N', 'B=0'}
    assert {(e, w) for e, w, code in R if code == SC.E_SHAPE and e.startswith('z')} >= {
        ('zfwd', 'rows=0'), ('zfwd', 'ldx<D'), ('zsums', 'ldx<D'), ('zupd', 'rows=0'), ('zupd', 'ldx<D')}
    assert ('rf', 'partials+4', SC.E_ALIGN) in R
    nulls = {}
    for e, w, code in R:
        if code == SC.E_NULL:
            nulls.setdefault(e, set()).add(w[5:])
    assert nulls == dict(gae={'values', 'rewards', 'dones', 'gpow', 'lpow', 'adv', 'ret'},
                         norm={'values', 'rewards', 'dones', 'gpow', 'lpow', 'adv', 'ret', 'mom', 'ticket'},
                         rf={'rewards', 'out', 'partials', 'ticket', 'state'}, mom={'x', 'out'}, merge={'parts', 'out'},
                         advn={'x', 'mom'}, zstats={'rs', 'rsq', 'cnt', 'mean', 'std'}, zfwd={'x', 'mean', 'std', 'out'},
                         zsums={'x', 'rs', 'rsq', 'cnt', 'out'}, zupd={'x', 'rs', 'rsq', 'cnt'})


def _profile(name):
    return os.path.join(ROOT, 'profiles', name)


def test_the_recorded_margins_cover_the_table():
    """profiles/scan_case_margins.txt (written by test_gpu_scan.py on an MI355X): one line per case, every share <= 1"""
    seen = {}
    for line in open(_profile('scan_case_margins.txt')):
        if line.startswith('#') or not line.strip():
            continue
        f = line.split()
        seen[f[0]] = {kv.split('=')[0]: float(kv.split('=')[1]) for kv in f[1:]}
    assert set(seen) == set(ids(SC.CASES))
    for cid, r in seen.items():
        assert r and max(r.values()) <= 1.0, cid


SCAN_KERNELS = ('gae_kernel', 'gae_norm_kernel', 'reward_filter_kernel', 'moments_kernel', 'moments_merge_kernel',
                'adv_normalize_kernel', 'zstats_kernel', 'zforward_kernel', 'zforward_sums_kernel', 'zupdate_kernel',
                'zupdate_part_kernel', 'zupdate_merge_kernel', 'learn_epilogue_kernel')


def test_the_committed_kernel_trace_names_all_13_kernels():
    """profiles/scan_paths_kernel_stats.csv: a kernel trace of tests/test_gpu_scan.py alone on an MI355X"""
    import csv
    calls = dict.fromkeys(SCAN_KERNELS, 0)
    for row in csv.DictReader(open(_profile('scan_paths_kernel_stats.csv'))):
        for k in SCAN_KERNELS:
            if row['Name'].startswith(k + '('):
                calls[k] += int(row['Calls'])
    assert len(SCAN_KERNELS) == 13
    for k, n in calls.items():
        assert n > 0, k
    src = open(os.path.join(ROOT, 'surreal_amd', 'csrc', 'smx_scan.hip')).read()
    assert src.count('__global__') == 13 and all(' void %s(' % k in src for k in SCAN_KERNELS)


# ---- the harness can fail: each wrong double breaks a named case -----------------------------------------------------------
class NoStagingPast256(TorchCpuKernels):               # 1. steps t >= 256 never reach the LDS row
    def gae(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, H, adv, ret, values_tail=None):
        rewards = rewards.clone()
        rewards[:, 256:] = 0.0
        if values_tail is None:
            values = values.clone().view(B, N + 1)
            values[:, 256:] = 0.0
            values = values.reshape(-1)
        else:
            values = values.clone().view(B, N)
            values[:, 256:] = 0.0
            values_tail = values_tail * 0.0 if N >= 256 else values_tail
        TorchCpuKernels.gae(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, H, adv, ret, values_tail)


class DonesShifted(TorchCpuKernels):                   # 2. Vm[t] masked by dones[t] instead of dones[t - 1]
    def gae(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, H, adv, ret, values_tail=None):
        d = torch.zeros_like(dones)
        d[:, :-1] = dones[:, 1:]
        TorchCpuKernels.gae(self, values, rewards, d, gpow, lpow, gamma, gamma_H, B, N, H, adv, ret, values_tail)


class TailNotMasked(TorchCpuKernels):                  # 3. the bootstrap value ignores the last done
    def gae(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, H, adv, ret, values_tail=None):
        d = dones.clone()
        d[:, N - 1] = 0.0
        TorchCpuKernels.gae(self, values, rewards, d, gpow, lpow, gamma, gamma_H, B, N, H, adv, ret, values_tail)


class DropsLastTerm(TorchCpuKernels):                  # 4. a window's last term
    def gae(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, H, adv, ret, values_tail=None):
        g = gpow.clone()
        g[H - 1] = 0.0
        TorchCpuKernels.gae(self, values, rewards, dones, g, lpow, gamma, gamma_H, B, N, H, adv, ret, values_tail)


class BootstrapOneEarly(TorchCpuKernels):              # 5. window s bootstraps from Vm[s + H - 1]
    def gae(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, H, adv, ret, values_tail=None):
        TorchCpuKernels.gae(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, H, adv, ret, values_tail)
        v = values.view(B, -1) if values_tail is None else torch.cat([values.view(B, N), values_tail.view(B, 1)], 1)
        v = v.clone()
        v[:, 1:] *= 1 - dones
        E = N - H + 1
        ret.view(B, E).add_((v[:, H - 1:H - 1 + E] - v[:, H:H + E]) * gamma_H)


class WindowsRoundedDown(TorchCpuKernels):             # 6. E rounded down to a multiple of 64
    def gae(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, H, adv, ret, values_tail=None):
        E = N - H + 1
        keep_a, keep_r = adv.clone(), ret.clone()
        TorchCpuKernels.gae(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, H, adv, ret, values_tail)
        if E > 1:
            adv.view(B, E)[:, E // 64 * 64:] = keep_a.view(B, E)[:, E // 64 * 64:]
            ret.view(B, E)[:, E // 64 * 64:] = keep_r.view(B, E)[:, E // 64 * 64:]


class SkipsLastRaggedRow(TorchCpuKernels):             # 7. row B - 1 where B mod 4 != 0
    def gae(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, H, adv, ret, values_tail=None):
        E = N - H + 1
        keep_a, keep_r = adv.clone(), ret.clone()
        TorchCpuKernels.gae(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, H, adv, ret, values_tail)
        if B % 4:
            adv.view(B, E)[B - 1] = keep_a.view(B, E)[B - 1]
            ret.view(B, E)[B - 1] = keep_r.view(B, E)[B - 1]


class BiasedStd(TorchCpuKernels):                      # 8. / n
    def adv_normalize(self, x, mom, min_std):
        std = torch.sqrt(mom[2] / mom[0])
        x.copy_((x - mom[1]) / (torch.tensor(min_std) if min_std > float(std) else std))


class MinStdAlways(TorchCpuKernels):                   # 9. the floor as the denominator whatever the deviation is
    def adv_normalize(self, x, mom, min_std):
        x.copy_((x - mom[1]) / min_std)


def _chunk_rows(rows):
    ch = SC.zupdate_chunks(rows)
    per = -(-rows // ch)
    return [(k * per, min((k + 1) * per, rows)) for k in range(ch)]


class DropsChunkTailRow(TorchCpuKernels):              # 10. zupdate_part_kernel without its one-row tail
    def zfilter_update(self, x_view, rs, rsq, cnt, count_rows, ws=None):
        rows, D = x_view.shape
        if ws is None or ws.numel() < SC.zupdate_ws_floats(rows, D) or SC.zupdate_chunks(rows) == 0:
            return TorchCpuKernels.zfilter_update(self, x_view, rs, rsq, cnt, count_rows)
        keep = torch.ones(rows, dtype=torch.bool)
        for r0, r1 in _chunk_rows(rows):
            full = r0 + (r1 - r0) // 32 * 32
            keep[full:min(full + 16, r1)] = False              # the rows whose partner 16 further on is past the chunk
        TorchCpuKernels.zfilter_update(self, x_view[keep], rs, rsq, cnt, count_rows)


class CountsPerChunk(TorchCpuKernels):                 # 11. count += count_rows in every chunk
    def zfilter_update(self, x_view, rs, rsq, cnt, count_rows, ws=None):
        rows, D = x_view.shape
        ch = SC.zupdate_chunks(rows) if ws is not None and ws.numel() >= SC.zupdate_ws_floats(rows, D) else 0
        TorchCpuKernels.zfilter_update(self, x_view, rs, rsq, cnt, count_rows * max(ch, 1))


class AccumulatesSumsq(TorchCpuKernels):               # 12. running_sumsq += where reward_filter.py:42 assigns
    def reward_filter(self, rewards, scale, state, eps, out, partials, ticket, use_filter=True, update=True, sums=None):
        before = state[2].clone()
        TorchCpuKernels.reward_filter(self, rewards, scale, state, eps, out, partials, ticket, use_filter, update, sums)
        if update:
            state[2] += before


class ClampEatsNaN(TorchCpuKernels):                   # 13. fminf(fmaxf(NaN, -5), 5) = 5
    def zfilter_forward(self, x_view, mean, std, out):
        out.copy_(torch.nan_to_num(torch.clamp((x_view - mean) / std, -5.0, 5.0), nan=5.0))


def _named(*prefixes):
    return [c.id for p in prefixes for c in SC.CASES if c.id.startswith(p)]


WRONG = [(NoStagingPast256, _named('gae-B5-N257-H257-l')), (DonesShifted, _named('gae-B4-N513-H513-l-edge', 'gae-B3-N300')),
         (TailNotMasked, _named('gae-B3-N300-H300-l-last')), (DropsLastTerm, _named('gae-B1-N1-', 'gae-B5-N3413')),
         (BootstrapOneEarly, _named('gae-B5-N64-', 'gae-B5-N600-H7')), (WindowsRoundedDown, _named('gae-B2-N65-H1-')),
         (SkipsLastRaggedRow, _named('gae-B9-N1400-H1335')), (BiasedStd, _named('norm-B3-N3-')),
         (MinStdAlways, _named('norm-B1201-N19')), (DropsChunkTailRow, _named('zupd-r16385-D5')),
         (CountsPerChunk, _named('zupd-r16384-D5')), (AccumulatesSumsq, _named('rf-n1024')),
         (ClampEatsNaN, _named('zfwd-D63-s1'))]


@pytest.mark.parametrize('double,named', WRONG, ids=[d.__name__ for d, _ in WRONG])
def test_a_wrong_double_fails_its_named_case(double, named):
    assert named, 'the case this double is there for left the table'
    kern = double()
    failed = []
    for cid in named:
        try:
            SC.run_entry(kern, SC.BY_ID[cid], **_kw(SC.BY_ID[cid]))
        except AssertionError:
            failed.append(cid)
    assert failed, '%s passed %s: the table cannot see that defect' % (double.__name__, named)
    SC.run_entry(C, SC.BY_ID[named[0]], **_kw(SC.BY_ID[named[0]]))      # ... which the right double passes
