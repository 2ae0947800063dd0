"""CPU tier: the dense-layer case table (dense_cases.py) on the torch-CPU double, the coverage conditions the table must
meet, and proof that its checks can fail: seven deliberately wrong doubles, each of which must break at least one case.
test_gpu_dense.py runs the same table objects on the HIP kernels."""
import collections
import os

import pytest
import torch

import dense_cases as DC
from cpu_kernels import TorchCpuKernels

C = TorchCpuKernels()
SMALL = [c for c in DC.LINEAR_CASES + DC.BATCHES + DC.WGRAD_CASES if not (isinstance(c, DC.Wg) and c.rows > 5000)]


def ids(cases):
    return [c.id for c in cases]


# ---- the table passes on the double: the references, the poisoning and the sentinel logic hold --------------------
@pytest.mark.parametrize('c', DC.LINEAR_CASES, ids=ids(DC.LINEAR_CASES))
def test_linear_case_on_the_double(c):
    DC.run_entry(C, c)


@pytest.mark.parametrize('c', DC.BATCHES, ids=ids(DC.BATCHES))
def test_batch_on_the_double(c):
    DC.run_entry(C, c)


@pytest.mark.parametrize('c', DC.WGRAD_CASES, ids=ids(DC.WGRAD_CASES))
def test_wgrad_case_on_the_double(c):
    DC.run_entry(C, c, ws_for=lambda w: torch.full((16,), float('nan')))


def test_ids_are_unique_and_the_table_is_a_few_hundred_launches():
    every = DC.LINEAR_CASES + DC.BATCHES + DC.WGRAD_CASES
    names = [c.id for c in every] + [j.id for b in DC.BATCHES for j in b.jobs]
    assert len(set(names)) == len(names)
    assert 200 <= len(every) <= 400


def test_the_gpu_file_runs_the_same_table_objects_and_marks_nothing_to_skip():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_gpu_dense.py')).read()
    for table in ('DC.LINEAR_CASES', 'DC.BATCHES', 'DC.WGRAD_CASES', 'DC.REFUSALS'):
        assert "parametrize('c', %s" % table in src or "parametrize('what', %s" % table in src
    assert 'skip' not in src and 'xfail' not in src


# ---- the restated dispatch gives every case the path it was built for ------------------------------------------------
def test_every_case_takes_the_path_it_declares():
    for c in DC.LINEAR_CASES:
        assert DC.expected_path(c) == (c.kernel, c.am, c.bm), c.id
    for b in DC.BATCHES:
        kernel, modes = DC.expected_path(b)
        assert kernel == b.kernel, b.id
        for j, (am, bm) in zip(b.jobs, modes):
            if isinstance(j, DC.Wg):
                assert (am, bm) == (2, 2), j.id
            else:
                assert (am, bm) == (j.am, j.bm), j.id
        assert 1 <= len(b.jobs) <= 9
    assert sorted(set(len(b.jobs) for b in DC.BATCHES)) == [1, 2, 3, 4, 9]
    assert any(isinstance(j, DC.Wg) for b in DC.BATCHES for j in b.jobs if len(b.jobs) == 9)


def test_all_23_cells_appear_each_with_a_case_ragged_in_m_n_and_k():
    seen = collections.defaultdict(list)
    for c in DC.LINEAR_CASES + DC.BATCHES:
        for k, a, b, ragged in DC.cells_of(c):
            seen[(k, a, b)].append(ragged)
    assert len(DC.ALL_CELLS) == 23
    for cell in DC.ALL_CELLS:
        assert cell in seen, 'no case reaches %r' % (cell,)
        assert any(seen[cell]), 'no case of %r is ragged in M, N and K at once' % (cell,)
    assert set(seen) == set(DC.ALL_CELLS)


def test_mode_1_is_reached_in_each_of_its_three_ways_alone_on_both_kernels_that_have_it():
    alone = collections.defaultdict(set)
    for c in DC.LINEAR_CASES:
        p = DC.prob_of(c)
        for r in (DC.mode1_reasons(p.a_kc, p.lda, p.K, p.a_off), DC.mode1_reasons(p.b_kc, p.ldb, p.K, p.b_off)):
            if len(r) == 1:
                alone[DC.expected_path(c)[0]] |= r
    for k in ('gemm32', 'rows'):
        assert alone[k] == {'K', 'ld', 'off'}, (k, alone[k])


def test_k_sweeps_m_n_edges_strides_epilogues_and_stop_flags():
    by = collections.defaultdict(list)
    for c in DC.LINEAR_CASES:
        by[c.kernel[:4] if c.kernel.startswith('tile') else c.kernel].append(c)
    ks = lambda k, f: {c.K for c in by[k] if f(c)}
    has0 = lambda c: c.am == 0 or c.bm == 0
    assert ks('gemm32', lambda c: not has0(c)) >= {1, 3, 31, 32, 33, 127, 128, 129, 383, 384, 385, 417, 769}
    assert ks('gemm32', has0) >= {4, 32, 36, 128, 132, 384, 388, 772}
    assert ks('gemm32_co', lambda c: True) >= {4, 28, 32, 36, 124, 128, 132, 252, 256, 260, 508, 512, 516, 1028}
    assert ks('rows', lambda c: not has0(c)) >= {1, 31, 32, 33, 95, 96, 97, 191, 193}
    assert ks('rows', has0) >= {4, 28, 32, 36, 92, 96, 100, 196}
    assert ks('tile', lambda c: (c.am, c.bm) == (0, 0)) >= {32, 36, 60, 64, 68, 100}
    assert ks('tile', lambda c: (c.am, c.bm) == (2, 2)) >= {32, 36, 60, 64, 68, 100, 33, 63, 65}
    cells = collections.defaultdict(set)
    for c in DC.LINEAR_CASES:
        cells[(c.kernel, c.am, c.bm)].add(c.K)
    assert all(len(v) >= 3 for v in cells.values()), {k: v for k, v in cells.items() if len(v) < 3}
    for k, Ms, Ns in (('gemm32', {1, 31, 32, 33, 65}, {1, 5, 32, 33, 70}), ('gemm32_co', {1, 31, 32, 33, 65}, {1, 5, 32, 33, 70}),
                      ('rows', {2048, 2049, 2081, 2177}, {1, 9, 33, 63}), ('tile', {2048, 2049, 2050, 2113}, {64, 65, 127, 130})):
        assert {c.M for c in by[k]} >= Ms and {c.N for c in by[k]} >= Ns, k
    assert any(c.N == 65 and c.K < 32 for c in by['rows'])
    assert any(c.M == 2050 and not c.a_kc for c in by['tile'])
    for k in ('gemm32', 'gemm32_co'):                                  # the XCD permutation's tile counts
        assert {DC.grid_of(c) for c in by[k]} >= {1, 2, 7, 8, 9, 15, 17, 63, 65}, k
    grids = {DC.grid_of(c) & 7 for c in by['tile']}
    assert 0 in grids and len(grids) > 2
    for k in by:
        assert {(c.bias, c.act, c.mask) for c in by[k] if c.values == 'int'} >= set(DC._EPI), k
        assert {c.stop for c in by[k]} == {None, 0, 1}, k
        assert any(c.act == DC.TANH and c.values == 'float' for c in by[k]), k
        assert {c.c_pad for c in by[k]} >= {0, 5}
        for side in ('a', 'b'):
            pads = {getattr(c, side + '_pad') for c in by[k]}
            assert pads >= {0, 4}, (k, side, pads)
    assert any(c.a_kc and c.K == 1 and c.a_pad == 0 for c in by['gemm32'])          # lda = 1 with K = 1
    assert any(c.c_off > 8 and c.c_pad > 8 for c in by['gemm32'])                   # a column block of a wider matrix
    # batches: a stop flag on one job only, a many-row job next to a small one, many-row jobs of differing storage
    stops = [b for b in DC.BATCHES if any(getattr(j, 'stop', None) == 1 for j in b.jobs)]
    assert stops and all(any(getattr(j, 'stop', None) != 1 for j in b.jobs) for b in stops)
    assert any(b.kernel == 'gemm32' and max(j.M for j in b.jobs) >= 2048 and min(j.M for j in b.jobs) < 2048 for b in DC.BATCHES)
    assert any(b.kernel == 'rows' and len({(j.a_kc, j.b_kc) for j in b.jobs}) > 1 for b in DC.BATCHES)


def test_weight_gradient_cases_cover_rows_shapes_strides_and_the_split_k_branches():
    W = DC.WGRAD_CASES
    assert {c.rows for c in W} >= {1, 33, 385, 2047, 2048, 2049, 4100, 34817, 34000}
    assert {c.M for c in W} >= {1, 33, 48} and {c.N for c in W} >= {1, 17, 70}
    assert any(c.z_pad and c.x_pad and c.w_pad for c in W) and any(not c.db for c in W)
    assert any(c.ws for c in W) and any(not c.ws for c in W)
    assert any(isinstance(j, DC.Wg) for b in DC.BATCHES for j in b.jobs)
    # (6, 10, 34817) on the 32 x 32 branch: 34 chunks of 1056 rows asked for, the last one empty, 33 left
    assert DC.split32_closed_form(6, 10, 34817) == (34, 1056, 33)
    assert 33 * 1056 >= 34817 > 32 * 1056
    by_id = {c.id: c for c in W}
    assert DC.wgrad_plan(by_id['wgrad-6x10x34817-ws-ldwN']) == (['gemm32', 'segmented_reduce'], 33)
    assert DC.wgrad_plan(by_id['wgrad-6x10x34817-ws-ldwN3']) == (['gemm32', 'splitk_reduce'], 33)
    # (8, 8, 34000): multiples of 4, but no cut of an 8 x 8 dW fits smx_wgrad.hip's wave tiles -> the 32 x 32 kernel too
    assert DC.wgrad_rows_groups(8, 8) == 0
    assert DC.wgrad_plan(by_id['wgrad-8x8x34000-ws-mult4']) == (['gemm32', 'segmented_reduce'], 33)
    # the register-resident kernel
    assert DC.wgrad_plan(by_id['wgrad-116x180x32768-ws-regs']) == (['wgrad_rows', 'segmented_reduce'], 256)
    assert DC.wgrad_plan(by_id['wgrad-116x180x32768-ws-regs-nodb']) == (['wgrad_rows', 'splitk_reduce'], 256)
    n = DC.predicted_launches()
    assert n['wgrad_rows'] == 2 and n['segmented_reduce'] >= 2 and n['splitk_reduce'] >= 2
    for k in ('gemm32', 'gemm32_co', 'rows', 'tile00', 'tile02', 'tile20', 'tile22'):
        assert n[k] > 0


def test_the_committed_kernel_trace_shows_the_predicted_launch_counts():
    """profiles/dense_paths_kernel_stats.csv (a kernel trace of tests/test_gpu_dense.py alone on an MI355X) against the
    restated dispatch: the kernel CHOICE is the library's.  (A table change needs a new trace.)"""
    import csv
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'dense_paths_kernel_stats.csv')
    calls = {}
    for row in csv.DictReader(open(path)):
        calls[row['Name']] = int(row['Calls'])
    names = {'gemm32': 'gemm32_kernel<false>', 'gemm32_co': 'gemm32_kernel<true>', 'rows': 'gemm_rows_kernel',
             'tile00': 'gemm_tile_kernel<0, 0, 1, 1>', 'tile02': 'gemm_tile_kernel<0, 2, 1, 1>',
             'tile20': 'gemm_tile_kernel<2, 0, 1, 1>', 'tile22': 'gemm_tile_kernel<2, 2, 1, 1>',
             'splitk_reduce': 'splitk_reduce_kernel', 'segmented_reduce': 'segmented_reduce_kernel',
             'wgrad_rows': 'wgrad_rows_kernel'}
    want = DC.predicted_launches()
    assert set(want) == set(names)
    for k, frag in names.items():
        got = [n for name, n in calls.items() if frag in name]
        assert got == [want[k]], (k, got, want[k])


# ---- the harness can fail: each wrong double breaks at least one case -------------------------------------------------
class DropsLastK(TorchCpuKernels):
    def linear(self, A, a_kc, B, b_kc, bias, C, M, N, K, **kw):
        TorchCpuKernels.linear(self, A, a_kc, B, b_kc, bias, C, M, N, K - 1, **kw)


class ReadsPastK(TorchCpuKernels):
    def linear(self, A, a_kc, B, b_kc, bias, C, M, N, K, **kw):
        TorchCpuKernels.linear(self, A, a_kc, B, b_kc, bias, C, M, N, K + (1 if a_kc and b_kc else 0), **kw)


class WritesPastN(TorchCpuKernels):
    def linear(self, A, a_kc, B, b_kc, bias, C, M, N, K, **kw):
        TorchCpuKernels.linear(self, A, a_kc, B, b_kc, bias, C, M, N, K, **kw)
        if not (kw.get('stop') is not None and int(kw['stop'][0])):
            torch.as_strided(C, (M, N + 1), (kw['ldc'], 1))[:, N] = 0.0


class SkipsLastRow(TorchCpuKernels):
    def linear(self, A, a_kc, B, b_kc, bias, C, M, N, K, **kw):
        if M > 1:
            TorchCpuKernels.linear(self, A, a_kc, B, b_kc, bias, C, M - 1, N, K, **kw)


class IgnoresStop(TorchCpuKernels):
    def linear(self, A, a_kc, B, b_kc, bias, C, M, N, K, **kw):
        TorchCpuKernels.linear(self, A, a_kc, B, b_kc, bias, C, M, N, K, **dict(kw, stop=None))


class MaskStrideN(TorchCpuKernels):
    def linear(self, A, a_kc, B, b_kc, bias, C, M, N, K, **kw):
        mask = kw.get('relu_mask')
        TorchCpuKernels.linear(self, A, a_kc, B, b_kc, bias, C, M, N, K, **dict(kw, relu_mask=None))
        if mask is not None and not (kw.get('stop') is not None and int(kw['stop'][0])):
            torch.as_strided(C, (M, N), (kw['ldc'], 1)).mul_(torch.as_strided(mask, (M, N), (N, 1)) > 0)


class BiasGradOverLdz(TorchCpuKernels):
    def linear_wgrad(self, dZ, X, dW, db, M, N, rows, ldz=None, **kw):
        TorchCpuKernels.linear_wgrad(self, dZ, X, dW, None, M, N, rows, ldz=ldz, **kw)
        if db is not None:
            db.view(-1)[:ldz].copy_(torch.as_strided(dZ, (rows, ldz), (ldz, 1)).sum(0))


WRONG = [DropsLastK, ReadsPastK, WritesPastN, SkipsLastRow, IgnoresStop, MaskStrideN, BiasGradOverLdz]


@pytest.mark.parametrize('double', WRONG, ids=[d.__name__ for d in WRONG])
def test_a_wrong_double_fails_at_least_one_case(double):
    kern = double()
    failed = []
    for c in SMALL:
        try:
            DC.run_entry(kern, c)
        except AssertionError:
            failed.append(c.id)
            if len(failed) >= 3:
                break
    assert failed, '%s passed every case: the table cannot see that defect' % double.__name__
