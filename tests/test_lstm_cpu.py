"""CPU tier: the LSTM case table (lstm_cases.py) on the torch-CPU double against the float64 reference at the GPU tier's
tolerances, the reference against torch.nn.LSTM().double() and autograd, the coverage conditions the table must meet, and
proof that its checks can fail: nine deliberately wrong doubles, each of which must break at least one case.
test_gpu_lstm.py runs the same table objects on the HIP kernels."""
import collections
import os

import pytest
import torch

import lstm_cases as LC
from cpu_kernels import TorchCpuKernels

C = TorchCpuKernels()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize('c', LC.CASES, ids=ids(LC.CASES))
def test_case_on_the_double(c):
    LC.run_entry(C, c)


def test_ids_are_unique_and_the_table_stays_small():
    assert len(set(ids(LC.CASES))) == len(LC.CASES)
    assert 100 <= len(LC.CASES) <= 160
    for c in LC.CASES:
        assert c.B <= 1040 and c.B * c.T * 4 * c.H * 4 <= 40 << 20, c.id
        assert c.off % 4 == 0


def test_the_gpu_file_runs_the_same_table_and_marks_nothing_to_skip():
    src = open(os.path.join(ROOT, 'tests', 'test_gpu_lstm.py')).read()
    assert "parametrize('c', LC.CASES" in src
    assert 'skip' not in src and 'xfail' not in src


@pytest.mark.parametrize('cells', [(True, True), (False, False), (True, False), (False, True)])
def test_the_reference_is_aten_lstm_in_double(cells):
    c = LC.Case('ref-check', 5, 9, 7, 12, cells[0], cells[1], True, False, 'none', False, 0)
    p = LC.make_inputs(c)
    want, aten = LC.reference(p), LC.aten_lstm(p, dtype=torch.float64)
    for k in ('out', 'hN', 'cN') + LC.GRAD_Q:
        assert torch.allclose(want[k], aten[k], rtol=1e-12, atol=1e-13), k
    # the saved tensors and dgates, which nn.LSTM does not show: autograd through the same equations
    pre = torch.zeros(c.B, c.T, 4 * c.H, dtype=torch.float64, requires_grad=True)      # added to the pre-activations
    W_ih, W_hh, b = p['W_ih'].double(), p['W_hh'].double(), (p['b_ih'] + 0).double() + p['b_hh'].double()
    h = p['h0'].double() if cells[0] else torch.zeros(c.B, c.H, dtype=torch.float64)
    cc = p['c0'].double() if cells[1] else torch.zeros(c.B, c.H, dtype=torch.float64)
    outs = []
    for t in range(c.T):
        assert torch.allclose(want['hprev'][:, t], h.detach(), rtol=1e-12, atol=1e-13)
        g = p['x'][:, t].double() @ W_ih.t() + h @ W_hh.t() + b + pre[:, t]
        i, f, gg, o = g.chunk(4, 1)
        cc = torch.sigmoid(f) * cc + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(cc)
        assert torch.allclose(want['cs'][:, t], cc.detach(), rtol=1e-12, atol=1e-13)
        outs.append(h)
    (torch.stack(outs, 1) * p['dout'].double()).sum().backward()
    assert torch.allclose(want['dgates'], pre.grad, rtol=1e-11, atol=1e-13)


# ---- the restated dispatch and the coverage conditions -------------------------------------------------------------------
def test_plan_restates_the_selection_rule():
    assert LC.plan(512, 17, 100) == ('m', 25, 25, 4, True) and LC.plan(512, 21, 104) == ('m', 28, 28, 4, False)
    assert LC.plan(511, 20, 104) == ('k', 7, 13, 1, True) and LC.plan(511, 20, 108) == ('k', 7, 16, 1, True)
    assert LC.plan(3, 5, 116) == ('k', 8, 16, 1, False) and LC.plan(512, 5, 128) == ('k', 8, 16, 2, False)
    assert LC.plan(512, 5, 132) == ('rows16', 24, 24, 16, False) and LC.plan(1, 5, 384).family == 'rows16'
    assert {LC.fwd_of(c) for c in LC.CASES} == set(LC.FWD_KERNELS) and len(LC.FWD_KERNELS) == 9
    assert {LC.bwd_of(c) for c in LC.CASES if c.save} == set(LC.BWD_KERNELS) and len(LC.BWD_KERNELS) == 6


def _range_of(kernel):
    """-> (smallest B of the kernel's range, batch rows per workgroup)"""
    many = 'fwdm' in kernel or 'bwdm' in kernel or ', 2' in kernel
    rows = 4 if ('fwdm' in kernel or 'bwdm' in kernel) else 2 if ', 2' in kernel else 16 if '<24>' in kernel else 1
    return (512 if many else 1), rows


def _rows_and_steps(kernel, cases):
    bmin, rows = _range_of(kernel)
    assert bmin in {c.B for c in cases}, '%s: no case at the smallest B of its range' % kernel
    if rows > 1:
        assert any(c.B % rows == 0 for c in cases) and any(c.B % rows for c in cases), '%s: full / ragged' % kernel
    ts = {c.T for c in cases}
    assert ts >= {1, 2, 3, 4, 5} and {t % 4 for t in ts} == {0, 1, 2, 3}, (kernel, ts)
    long_t = LC.LONG_T_MANY if bmin == 512 else LC.LONG_T
    assert any(c.T == long_t and c.B <= bmin + 1 for c in cases), '%s: no long sequence at its smallest B' % kernel


def test_every_forward_kernel_has_its_rows_steps_operands_and_saturated_case():
    for k in LC.FWD_KERNELS:
        cases = [c for c in LC.CASES if LC.fwd_of(c) == k]
        _rows_and_steps(k, cases)
        assert {(c.h0, c.c0) for c in cases} == {(True, True), (False, False), (True, False), (False, True)}, k
        assert any(not c.save for c in cases), '%s: no case without hprev, hN, cN' % k
        assert any(c.sat for c in cases), '%s: no bias-saturated case' % k


def test_every_backward_kernel_has_its_rows_steps_and_options():
    for k in LC.BWD_KERNELS:
        cases = [c for c in LC.CASES if c.save and LC.bwd_of(c) == k]
        _rows_and_steps(k, cases)
        assert {c.alias for c in cases} == {True, False}, k
        assert any(c.ws == 'none' for c in cases), k
        assert any(c.ws == 'exact' and LC.ws_floats(c.D, c.H, c.B, c.T) > 0 for c in cases), '%s: no workspace case' % k
        assert all(c.B * c.T < LC.DC.WGRAD_ROWS_MIN for c in cases)       # (the split-K rule restated is the 32 x 32 one)


def test_both_sides_of_every_selection_boundary_and_the_size_extremes():
    shapes = {(c.B >= 512, c.D <= 20, c.H) for c in LC.CASES if c.save}
    hs = lambda many: {h for m, _, h in shapes if m == many}  # noqa: E731
    assert hs(True) >= {100, 104, 112, 116, 128, 132}          # m 25 | 28, m | k two rows, k | 16-row at B >= 512
    assert hs(False) >= {104, 108, 112, 116, 128, 132}         # bwdk 13 | 16, fwdk 7 | 8, k | 16-row at B < 512
    for H in (100, 128):                                       # B 511 | 512 in both H ranges
        assert {c.B for c in LC.CASES if c.H == H and c.save} >= {511, 512}, H
    for many in (False, True):                                 # D 20 | 21 on the vector and on the m kernels
        assert {c.D for c in LC.CASES if (c.B >= 512) == many and c.H == 100 and c.save} >= {20, 21}
    every_h = {c.H for c in LC.CASES}
    assert every_h >= {4, 8, 16, 132, 140, 384}
    assert {c.H for c in LC.CASES if c.B >= 512} >= {4, 8}      # ... H = 4, 8 on the m kernels too
    assert {c.B for c in LC.CASES if c.H > 128} >= {1, 16, 17} and {c.B for c in LC.CASES if c.H == 384} >= {16, 17}
    assert any(c.H % 16 for c in LC.CASES if c.H > 128)
    fold_d = lambda k: {c.D for c in LC.CASES if LC.fwd_of(c) == k}  # noqa: E731
    assert fold_d('lstm_fwdk_kernel<7, 1, true>') >= {1, 5, 6, 10, 11, 15, 16, 20}
    assert fold_d('lstm_fwdm_kernel<25, true>') >= {1, 6, 20} and fold_d('lstm_fwdm_kernel<28, true>') >= {1, 6, 20}


def test_the_committed_kernel_trace_names_all_15_instantiations():
    """profiles/lstm_paths_kernel_stats.csv: a kernel trace of tests/test_gpu_lstm.py alone on an MI355X.  Every
    instantiation the restated dispatch names was launched, at least once per table case that plan() sends to it."""
    import csv
    calls = collections.Counter()
    for row in csv.DictReader(open(os.path.join(ROOT, 'profiles', 'lstm_paths_kernel_stats.csv'))):
        for k in LC.FWD_KERNELS + LC.BWD_KERNELS:
            if k + '(' in row['Name']:
                calls[k] += int(row['Calls'])
    assert len(LC.FWD_KERNELS + LC.BWD_KERNELS) == 15
    for k in LC.FWD_KERNELS:
        assert calls[k] >= sum(1 for c in LC.CASES if LC.fwd_of(c) == k) > 0, (k, calls[k])
    for k in LC.BWD_KERNELS:
        assert calls[k] >= sum(1 for c in LC.CASES if c.save and LC.bwd_of(c) == k) > 0, (k, calls[k])


def test_the_recorded_errors_cover_the_table():
    """profiles/lstm_cases_errors.txt (written by test_gpu_lstm.py on an MI355X): one line per case, every ratio <= 1"""
    seen = {}
    for line in open(os.path.join(ROOT, 'profiles', 'lstm_cases_errors.txt')):
        if line.startswith('#') or not line.strip():
            continue
        f = line.split()
        seen[f[0]] = {kv.split('=')[0]: float(kv.split('=')[1]) for kv in f[1:]}
    assert set(seen) == set(ids(LC.CASES))
    for c in LC.CASES:
        assert set(seen[c.id]) == (set(LC.FWD_Q + LC.BWD_Q) if c.save else {'out', 'gates', 'cs'}), c.id
        assert max(seen[c.id].values()) <= 1.0, c.id


# ---- the stop flag: the double states the contract the header gives -------------------------------------------------------
@pytest.mark.parametrize('tag', ['k7t-B3-T3-', 'r16-B17-T3-'])
def test_a_set_stop_flag_leaves_every_output_untouched_on_the_double(tag):
    c = next(c for c in LC.CASES if c.id.startswith(tag))._replace(alias=False)
    stop = torch.ones(1, dtype=torch.int32)
    x = LC.build(c)
    snap = LC.snapshot(x)
    LC.run_forward(C, x, stop)
    LC.assert_untouched(x, snap)
    LC.run_forward(C, x)
    snap = LC.snapshot(x)
    LC.run_backward(C, x, stop)
    LC.assert_untouched(x, snap)                       # dgates and grads still NaN, gates what the forward pass left


# ---- the harness can fail: each wrong double breaks at least one case -----------------------------------------------------
def _stopped(stop):
    return stop is not None and int(stop[0]) != 0


class DropsLastK(TorchCpuKernels):                     # 1. the last k-term of the recurrent sum
    def lstm_forward(self, net, x, B, T, h0, c0, gates, out, cs, hprev=None, hN=None, cN=None, stop=None):
        class Net(object):
            pass
        n2 = Net()
        n2.H, n2.views = net.H, dict(net.views)
        w = net.views['weight_hh'].clone()
        w[:, net.H - 1] = 0.0
        n2.views['weight_hh'] = w
        TorchCpuKernels.lstm_forward(self, n2, x, B, T, h0, c0, gates, out, cs, hprev, hN, cN, stop)


class IgnoresH0(TorchCpuKernels):                      # 2.
    def lstm_forward(self, net, x, B, T, h0, c0, gates, out, cs, hprev=None, hN=None, cN=None, stop=None):
        TorchCpuKernels.lstm_forward(self, net, x, B, T, None, c0, gates, out, cs, hprev, hN, cN, stop)


class BackwardForgetsC0(TorchCpuKernels):              # 3. c0 in the forward pass, zero as c_{-1} in the backward pass
    def lstm_backward(self, net, x, B, T, c0, gates, cs, hprev, dout, dgates, grads, stop=None, ws=None):
        TorchCpuKernels.lstm_backward(self, net, x, B, T, None, gates, cs, hprev, dout, dgates, grads, stop, ws)


class SwapsFandG(TorchCpuKernels):                     # 4. the f and g gate blocks change places in the saved gates
    def lstm_forward(self, net, x, B, T, h0, c0, gates, out, cs, hprev=None, hN=None, cN=None, stop=None):
        TorchCpuKernels.lstm_forward(self, net, x, B, T, h0, c0, gates, out, cs, hprev, hN, cN, stop)
        H = net.H
        g = gates.view(B * T, 4 * H)
        f = g[:, H:2 * H].clone()
        g[:, H:2 * H] = g[:, 2 * H:3 * H]
        g[:, 2 * H:3 * H] = f


class LeavesHprev0(TorchCpuKernels):                   # 5. hprev[:, 0] is never written
    def lstm_forward(self, net, x, B, T, h0, c0, gates, out, cs, hprev=None, hN=None, cN=None, stop=None):
        keep = None if hprev is None else hprev.view(B, T, net.H)[:, 0].clone()
        TorchCpuKernels.lstm_forward(self, net, x, B, T, h0, c0, gates, out, cs, hprev, hN, cN, stop)
        if keep is not None:
            hprev.view(B, T, net.H)[:, 0] = keep


class LeavesDbHh(TorchCpuKernels):                     # 6. db_hh is not written
    def lstm_backward(self, net, x, B, T, c0, gates, cs, hprev, dout, dgates, grads, stop=None, ws=None):
        keep = grads[-4 * net.H:].clone()
        TorchCpuKernels.lstm_backward(self, net, x, B, T, c0, gates, cs, hprev, dout, dgates, grads, stop, ws)
        grads[-4 * net.H:] = keep


class LeavesDgates0(TorchCpuKernels):                  # 7. dgates at t = 0 is not written (the gradients are right)
    def lstm_backward(self, net, x, B, T, c0, gates, cs, hprev, dout, dgates, grads, stop=None, ws=None):
        keep = dgates.view(B, T, 4 * net.H)[:, 0].clone()
        TorchCpuKernels.lstm_backward(self, net, x, B, T, c0, gates, cs, hprev, dout, dgates, grads, stop, ws)
        dgates.view(B, T, 4 * net.H)[:, 0] = keep


class StoresMissingRow(TorchCpuKernels):               # 8. a ragged workgroup's missing row goes one row past B
    def lstm_forward(self, net, x, B, T, h0, c0, gates, out, cs, hprev=None, hN=None, cN=None, stop=None):
        TorchCpuKernels.lstm_forward(self, net, x, B, T, h0, c0, gates, out, cs, hprev, hN, cN, stop)
        rows = LC.plan(B, x.shape[-1], net.H).rows
        if B % rows and not _stopped(stop):
            n = min(net.H, LC.TAIL)
            torch.as_strided(out, (n,), (1,), out.storage_offset() + B * T * net.H).copy_(out.reshape(-1)[:n])


class AccumulatesGrads(TorchCpuKernels):               # 9. grads += instead of grads =
    def lstm_backward(self, net, x, B, T, c0, gates, cs, hprev, dout, dgates, grads, stop=None, ws=None):
        before = grads.clone()
        TorchCpuKernels.lstm_backward(self, net, x, B, T, c0, gates, cs, hprev, dout, dgates, grads, stop, ws)
        if not _stopped(stop):
            grads.add_(before)


WRONG = [DropsLastK, IgnoresH0, BackwardForgetsC0, SwapsFandG, LeavesHprev0, LeavesDbHh, LeavesDgates0, StoresMissingRow,
         AccumulatesGrads]


@pytest.mark.parametrize('double', WRONG, ids=[d.__name__ for d in WRONG])
def test_a_wrong_double_fails_at_least_one_case(double):
    kern = double()
    failed = []
    for c in LC.SMALL:
        try:
            LC.run_entry(kern, c)
        except AssertionError:
            failed.append(c.id)
            if len(failed) >= 3:
                break
    assert failed, '%s passed every case: the table cannot see that defect' % double.__name__
