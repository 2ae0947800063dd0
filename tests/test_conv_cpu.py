"""CPU tier: the convolution case table (conv_cases.py) on the torch-CPU double, the coverage conditions the table must
meet (asserted from the restated dispatch), and proof that its checks can fail: eight deliberately wrong doubles, each of
which must break at least one case.  test_gpu_conv.py runs the same table objects on the HIP kernels."""
import collections
import os

import pytest
import torch

import conv_cases as CC
from cpu_kernels import TorchCpuKernels

C = TorchCpuKernels()
HERE = os.path.dirname(os.path.abspath(__file__))


def ids(cases):
    return [c.id for c in cases]


def by_inst():
    out = collections.defaultdict(list)
    for c in CC.CASES:
        out[CC.name_of(c)].append(c)
    return out


def ragged(c):
    return any(u % 16 for u in CC.units(c))


def family(c):
    if c.op != 'cl_dgrad':
        return c.op
    return 'cells' if CC.is_cells(c) else 'class'


FAMILIES = ('u8_fwd', 'u8_wgrad', 'cl_fwd', 'cl_wgrad', 'cells', 'class')


# ---- the table passes on the double: the references, the poisoning and the sentinel logic hold --------------------
@pytest.mark.parametrize('c', CC.CASES, ids=ids(CC.CASES))
def test_case_on_the_double(c):
    CC.run_entry(C, c)


@pytest.mark.parametrize('c', CC.ENVELOPE, ids=ids(CC.ENVELOPE))
def test_envelope_case_on_the_double(c):
    """the double takes every geometry: what the sweep's accepted cases are compared with holds for all of them, and
    the double's predicates are the shape conditions"""
    x = CC.build(c)
    assert CC.predicate(C, x) == CC.shape_ok(c)
    buf, n = CC.workspace(C, c)
    CC.run(C, x, ws=None if buf is None else buf[:n])
    CC.check(x)


def test_ids_are_unique_and_the_gpu_file_runs_the_same_objects_and_skips_nothing():
    names = ids(CC.CASES + CC.ENVELOPE + CC.WORKSPACE_REFUSALS)
    assert len(set(names)) == len(names)
    src = open(os.path.join(HERE, 'test_gpu_conv.py')).read()
    for table in ('CC.CASES', 'CC.ENVELOPE', 'CC.WORKSPACE_REFUSALS', 'CC.STEM_FALLBACK'):
        assert table in src
    assert 'skip' not in src and 'xfail' not in src


def test_float32_rounding_of_the_float64_quotient_is_the_correctly_rounded_byte_over_255():
    b = torch.arange(256)
    assert torch.equal((b.double() / 255).float(), b.float() / 255.0)


# ---- coverage, from the restated dispatch --------------------------------------------------------------------------
def test_every_instantiation_is_reached_ragged_below_a_channel_tile_and_at_its_largest_cout():
    seen = by_inst()
    assert len(CC.ALL_INSTANTIATIONS) == 8 + 6 + 6 + 4 + 4
    assert set(seen) == set(CC.ALL_INSTANTIATIONS)
    assert set(CC.NEWLY_REACHED) <= set(seen)
    for name in CC.ALL_INSTANTIATIONS:
        cases = seen[name]
        assert any(ragged(c) for c in cases), name
        assert any(c.cout % 16 and c.values == 'int' for c in cases), name
        assert any(c.cout == CC.max_cout(c) and c.values == 'int' and ragged(c) for c in cases), name
    for name in CC.NEWLY_REACHED:
        assert any(ragged(c) and c.values == 'int' and not c.stop for c in seen[name]), name


def test_multi_trip_cases_at_the_widest_and_a_narrow_instantiation_of_each_persistent_loop():
    multi = [c for c in CC.CASES if CC.plan(c).trips >= 3 and c.op in ('u8_fwd', 'cl_fwd', 'cl_dgrad')]
    fam = collections.defaultdict(list)
    for c in multi:
        assert CC.plan(c).grid == 2048 and max(CC.units(c)) > 262144 and max(CC.units(c)) % 16, c.id
        assert c.values == 'int' and c.stop is None and (c.opt or c.op != 'cl_dgrad'), c.id
        fam[family(c)].append(CC.plan(c).inst)
        # operands of tens of MB: the largest tensor of a case (the source, dy, or the output) below 100 MB
        Ho, Wo, rows = CC.geom(c)
        biggest = max(c.F * c.H * c.W * (c.C if c.op != 'u8_fwd' else 0) * 4, c.F * c.C * c.H * c.W, rows * c.cout * 4)
        assert biggest < 100e6, (c.id, biggest)
    assert sorted(fam['u8_fwd']) == [(4,), (16,)]
    assert sorted(fam['cl_fwd']) == [(4, 1), (16, 2)]
    assert sorted(fam['cells']) == [(1, False), (2, True)]
    assert sorted(fam['class']) == [(1, True), (2, False)]
    cls = [c for c in multi if family(c) == 'class']
    assert sorted(len(CC.units(c)) for c in cls) == [1, 4]
    four = [c for c in cls if len(CC.units(c)) == 4][0]
    assert four.s == 2 and four.H % 2 and four.W % 2 and len(set(CC.units(four))) == 3       # 9 / 6 / 6 / 4 pixels a frame
    # the classes of that case leave their loops after three, two and one trips
    nw = 4 * CC.plan(four).grid
    assert sorted(-(-(-(-u // 16)) // nw) for u in CC.units(four)) == [1, 2, 2, 3]


def test_weight_gradient_grids_and_partial_counts():
    for op, cap in (('u8_wgrad', 512), ('cl_wgrad', 256)):
        plans = [(c, CC.plan(c)) for c in CC.CASES if c.op == op]
        # one block whose wavefronts 1..3 have no group: their zero partials are summed all the same
        assert any(p.grid == 1 and -(-CC.geom(c)[2] // 16) < 4 and c.values == 'int' for c, p in plans), op
        assert any(2 <= p.grid <= 8 for c, p in plans), op
        assert any(p.grid == cap and p.trips >= 2 and ragged(c) for c, p in plans), op
        assert all(p.partials == (p.grid if op == 'u8_wgrad' else 4 * p.grid) for c, p in plans)
    counts = {CC.plan(c).partials for c in CC.CASES if c.op in ('u8_wgrad', 'cl_wgrad')}
    assert any(n < 16 for n in counts) and any(16 < n < 256 for n in counts)
    assert any(n % 4 and n < 16 for n in counts) and any(n % 4 and n > 16 for n in counts)
    assert {1, 3, 4, 8, 17, 512, 1024} <= counts


def test_geometry_edges_options_and_float_cases():
    fam = collections.defaultdict(list)
    for c in CC.CASES:
        fam[family(c)].append(c)
    for f in FAMILIES:
        cs = fam[f]
        assert any(CC.geom(c)[:2] == (1, 1) and c.F > 1 for c in cs), f
        assert any(c.F == 1 and max(CC.units(c)) < 16 for c in cs), f
        assert {c.stop for c in cs} == {None, 0, 1}, f
        assert sum(c.values == 'float' for c in cs) == 1, f
        if f != 'cells':                # (an even map under k = 4, s = 2 has no remainder)
            assert any((c.H - c.k) % c.s for c in cs if c.values == 'int'), f
        assert any(CC.plan(c).grid > 1 for c in cs), f
    for f in ('u8_wgrad', 'cl_wgrad', 'cells', 'class'):
        assert {c.opt for c in fam[f] if c.values == 'int' and not c.stop} == {True, False}, f
    assert any(CC.unseen_pixels(c) and c.values == 'int' for c in fam['class'])
    assert not any(CC.unseen_pixels(c) for c in fam['cells'])
    assert any(c.k == 6 and c.s == 3 for c in fam['class'])
    for f in ('u8_fwd', 'u8_wgrad'):
        assert any(c.fill == 0 for c in fam[f]) and any(c.fill == 255 for c in fam[f])
        sel = {CC.plan(c).inst for c in fam[f] if c.values == 'select'}
        assert sel == {(4,), (8,), (12,), (16,)}, f
    assert all(CC.shape_ok(c) and c.mis is None for c in CC.CASES + CC.WORKSPACE_REFUSALS)


def test_the_envelope_sweep_has_both_sides_of_every_boundary():
    E = collections.defaultdict(list)
    for c in CC.ENVELOPE:
        E[c.op].append(c)
    for op in ('u8_fwd', 'u8_wgrad'):
        assert {c.cout for c in E[op]} >= {16, 17}
        assert {c.k for c in E[op]} >= {2, 3, 4, 5, 8}
        assert {c.C * c.k * c.k for c in E[op]} >= {64, 80, 128, 192, 256, 320}
        assert {c.W % 4 for c in E[op]} == {0, 1, 2, 3} and {c.s for c in E[op]} >= {2, 4}
        assert {c.mis for c in E[op]} == {None, 'frames', 'W'}
    for op in ('cl_fwd', 'cl_wgrad'):
        assert {c.cout for c in E[op]} >= {16, 17, 32, 33} and {c.k for c in E[op]} >= {2, 3, 4, 5}
        assert {c.C for c in E[op]} == {15, 16, 17} and {c.mis for c in E[op]} == {None, 'src'}
    d = E['cl_dgrad']
    assert {c.cout for c in d} >= {16, 17, 32, 33} and {c.C for c in d} == {15, 16, 17}
    assert any(c.k == 2 * c.s for c in d) and any(c.k != 2 * c.s for c in d)
    assert {(c.cout % 4 == 0) for c in d if c.mis == 'dy'} == {True, False}
    for op, cs in E.items():
        assert any(CC.c_accepts(c) for c in cs) and any(not CC.shape_ok(c) for c in cs), op


def test_the_committed_kernel_trace_shows_the_predicted_launch_counts():
    """profiles/conv_paths_kernel_stats.csv (a kernel trace of tests/test_gpu_conv.py alone on an MI355X) against the
    restated dispatch, per instantiation: the kernel CHOICE is the library's.  (A table change needs a new trace.)"""
    import csv
    path = os.path.join(os.path.dirname(HERE), 'profiles', 'conv_paths_kernel_stats.csv')
    calls = {}
    for row in csv.DictReader(open(path)):
        calls[row['Name']] = int(row['Calls'])
    want = CC.predicted_launches()
    assert set(want) == set(CC.ALL_INSTANTIATIONS) | set(CC.REDUCES)
    for name, n in want.items():
        got = [k for nm, k in calls.items() if name + '(' in nm]
        assert got == [n], (name, got, n)
    # and nothing of smx_conv.hip's implicit-GEMM kernels besides
    assert sum(k for nm, k in calls.items() if 'conv_' in nm) == sum(want.values())


# ---- the harness can fail: each wrong double breaks at least one case -------------------------------------------------
def _stopped(stop):
    return stop is not None and int(stop[0]) != 0


class SwapsWeightOrder(TorchCpuKernels):          # (p, c) where torch keeps (c, p)
    def conv_cl_forward(self, src, F, C_, Hin, Win, k, stride, W, bias, cout, y, stop=None):
        W2 = W.reshape(cout, C_, k * k).transpose(1, 2).reshape(cout, -1)
        TorchCpuKernels.conv_cl_forward(self, src, F, C_, Hin, Win, k, stride, W2, bias, cout, y, stop=stop)


class DropsRaggedTile(TorchCpuKernels):
    def conv_u8_forward(self, frames, F, C_, Hin, Win, k, stride, W, bias, cout, y, stop=None):
        t = y.clone()
        TorchCpuKernels.conv_u8_forward(self, frames, F, C_, Hin, Win, k, stride, W, bias, cout, t, stop=stop)
        full = y.shape[0] // 16 * 16
        y[:full].copy_(t[:full])


class DropsChannelsFrom16(TorchCpuKernels):
    def conv_cl_forward(self, src, F, C_, Hin, Win, k, stride, W, bias, cout, y, stop=None):
        t = y.clone()
        TorchCpuKernels.conv_cl_forward(self, src, F, C_, Hin, Win, k, stride, W, bias, cout, t, stop=stop)
        y[:, :16].copy_(t[:, :16])


class MaskGreaterEqual(TorchCpuKernels):
    def conv_cl_dgrad(self, dy, F, C_, Hin, Win, k, stride, W, cout, relu_of, dx, stop=None):
        TorchCpuKernels.conv_cl_dgrad(self, dy, F, C_, Hin, Win, k, stride, W, cout, None, dx, stop=stop)
        if relu_of is not None and not _stopped(stop):
            dx.mul_((relu_of >= 0).float())


class LeavesUnseenPixels(TorchCpuKernels):
    def conv_cl_dgrad(self, dy, F, C_, Hin, Win, k, stride, W, cout, relu_of, dx, stop=None):
        t = dx.clone()
        TorchCpuKernels.conv_cl_dgrad(self, dy, F, C_, Hin, Win, k, stride, W, cout, relu_of, t, stop=stop)
        hs, ws_ = (Hin - k) // stride * stride + k, (Win - k) // stride * stride + k
        dx.view(F, Hin, Win, C_)[:, :hs, :ws_].copy_(t.view(F, Hin, Win, C_)[:, :hs, :ws_])


class DividesBy256(TorchCpuKernels):
    def conv_u8_forward(self, frames, F, C_, Hin, Win, k, stride, W, bias, cout, y, stop=None):
        if _stopped(stop):
            return
        rows = F * ((Hin - k) // stride + 1) * ((Win - k) // stride + 1)
        cols = torch.empty(rows, C_ * k * k)
        self.im2col(frames, F, C_, Hin, Win, k, stride, cols, scale_div=256.0)
        y[:rows].copy_(torch.relu(torch.nn.functional.linear(cols, W.reshape(cout, -1), bias)))


class StoresOnePast(TorchCpuKernels):
    def conv_cl_forward(self, src, F, C_, Hin, Win, k, stride, W, bias, cout, y, stop=None):
        TorchCpuKernels.conv_cl_forward(self, src, F, C_, Hin, Win, k, stride, W, bias, cout, y, stop=stop)
        if not _stopped(stop):
            torch.as_strided(y, (y.numel() + 1,), (1,))[y.numel()] = 0.0


class BiasGradMissesLastPartial(TorchCpuKernels):
    def conv_u8_wgrad(self, frames, F, C_, Hin, Win, k, stride, dy, cout, dW, db, ws, stop=None):
        TorchCpuKernels.conv_u8_wgrad(self, frames, F, C_, Hin, Win, k, stride, dy, cout, dW, db, ws, stop=stop)
        rows = dy.shape[0]
        if db is not None and not _stopped(stop):
            db.view(-1)[:cout].copy_(dy[:(rows - 1) // 16 * 16].sum(0))


WRONG = [SwapsWeightOrder, DropsRaggedTile, DropsChannelsFrom16, MaskGreaterEqual, LeavesUnseenPixels, DividesBy256,
         StoresOnePast, BiasGradMissesLastPartial]


@pytest.mark.parametrize('double', WRONG, ids=[d.__name__ for d in WRONG])
def test_a_wrong_double_fails_at_least_one_case(double):
    kern = double()
    failed = []
    for c in CC.SMALL:
        try:
            CC.run_entry(kern, c)
        except AssertionError:
            failed.append(c.id)
            if len(failed) >= 3:
                break
    assert failed, '%s passed every case: the table cannot see that defect' % double.__name__
