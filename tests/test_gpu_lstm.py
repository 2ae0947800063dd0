"""GPU tier (-m gpu): the LSTM recurrence of csrc/smx_lstm.hip by itself -- smx_lstm_forward_f32 / smx_lstm_backward_f32
over the case table of lstm_cases.py: all 9 forward and 6 backward instantiations, T at every residue of the four-step
rings, ragged workgroups, H and D at every selection boundary and at the edges of the quartered layouts, every
combination of the optional operands, aliased and separate dgates, with and without the split-K workspace.

Every case is held against a float64 reference -- forward outputs and saved tensors at 1e-5 absolute, dgates and each
gradient block against its own maximum -- in buffers whose surroundings are NaN (inputs) or a sentinel (outputs);
lstm_cases.py says how.  Then what only bits can show: the same call twice, batch rows permuted, two rows per workgroup
against one, T steps against the first T of T + 3; and the stop flag at the byte level, forward and backward.

With SMX_LSTM_ERRORS_OUT set to a path, the run writes every case's observed error / bar ratios there
(profiles/lstm_cases_errors.txt is such a run on an MI355X)."""
import os

import pytest
import torch

import lstm_cases as LC
from surreal_amd import _lib as L
from test_gpu_kernels import K  # noqa: F401  (the module-scoped kernels fixture)

pytestmark = pytest.mark.gpu


def ids(cases):
    return [c.id for c in cases]


@pytest.fixture(scope='module')
def errors():
    rec = {}
    yield rec
    path = os.environ.get('SMX_LSTM_ERRORS_OUT')
    if not path or not rec:
        return
    worst = {}
    for cid, r in rec.items():
        for q, (ratio, _) in r.items():
            if ratio > worst.get(q, (0.0, ''))[0]:
                worst[q] = (ratio, cid)
    with open(path, 'w') as f:
        f.write('# tests/test_gpu_lstm.py::test_case: observed max |got - float64 reference| / bar per case and quantity\n')
        f.write('# bars: out hN cN gates cs hprev 1e-5 absolute; dgates and each gradient block 2e-6 max|ref| + 1e-5 |ref|\n')
        for q in LC.FWD_Q + LC.BWD_Q:
            if q in worst:
                f.write('# worst %-6s %.4f  %s\n' % (q, worst[q][0], worst[q][1]))
        for c in LC.CASES:
            if c.id in rec:
                f.write(c.id + ' ' + ' '.join('%s=%.4f' % (q, rec[c.id][q][0]) for q in LC.FWD_Q + LC.BWD_Q if q in rec[c.id]))
                notes = [q + ':' + rec[c.id][q][1] for q in rec[c.id] if rec[c.id][q][1]]
                f.write('\n' + ''.join('#   %s\n' % n for n in notes))


@pytest.mark.parametrize('c', LC.CASES, ids=ids(LC.CASES))
def test_case(K, c, errors):
    _, record = LC.run_entry(K, c, 'cuda')
    for q, (ratio, note) in record.items():
        print('%s %s %.4f%s' % (c.id, q, ratio, note))
    errors[c.id] = record


def test_replaced_bars_name_table_cases():
    for cid, q in LC.REPLACED_BARS:
        assert cid in LC.BY_ID and q in LC.FWD_Q + LC.BWD_Q


# ---------------------------------------------------------------------------------------------------------------------
# bit-level properties
# ---------------------------------------------------------------------------------------------------------------------
def _shape(tag, B, T, D, H, alias=False):
    return LC.Case(tag, B, T, D, H, True, True, True, alias, 'none', False, 4)


def _both(K, c, inputs):
    """forward, then backward -> (built, bits of every output buffer after the forward call, ... after the backward)"""
    x = LC.build(c, 'cuda', inputs=inputs)
    LC.run_forward(K, x)
    after_f = LC.snapshot(x)
    LC.run_backward(K, x)
    after_b = LC.snapshot(x)
    LC.check_fences(x)
    return x, after_f, after_b


def _first(kernel, T):
    return next(c for c in LC.CASES if LC.fwd_of(c) == kernel and c.T == T and c.save)


@pytest.mark.parametrize('kernel', LC.FWD_KERNELS)
def test_the_same_call_twice_gives_the_same_bits(K, kernel):
    c = _first(kernel, 5)
    p = LC.make_inputs(c)
    _, f1, b1 = _both(K, c, p)
    _, f2, b2 = _both(K, c, p)
    for k in f1:
        assert torch.equal(f1[k], f2[k]), (k, 'after the forward call')
        assert torch.equal(b1[k], b2[k]), (k, 'after the backward call')
    assert not bool(torch.isnan(b1['grads'].view(torch.float32)[4:-LC.TAIL]).any())


def _rows(x, q, B):
    return x.v[q].detach().cpu().reshape(B, -1)


# B across several workgroups with a ragged last one, in each family (and both row counts of the vector kernels)
@pytest.mark.parametrize('B,D,H', [(515, 17, 100), (7, 17, 100), (513, 9, 116), (37, 11, 132)],
                         ids=['m', 'k', 'k-two-rows', 'rows16'])
def test_permuting_the_batch_rows_permutes_the_outputs_bit_for_bit(K, B, D, H):
    c = _shape('perm-%d-%d' % (B, H), B, 6, D, H)
    p = LC.make_inputs(c)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B))
    assert not torch.equal(perm, torch.arange(B))
    p2 = dict(p)
    for k in ('x', 'dout', 'h0', 'c0'):
        p2[k] = p[k][perm].contiguous()
    x1, _, _ = _both(K, c, p)
    x2, _, _ = _both(K, c, p2)
    for q in ('out', 'cs', 'gates', 'dgates', 'hprev', 'hN', 'cN'):
        a, b = _rows(x1, q, B), _rows(x2, q, B)
        assert bool(torch.isfinite(a).all())
        assert torch.equal(a[perm], b), '%s of a row depends on where the row sits in the batch' % q


@pytest.mark.parametrize('H', [116, 128])
def test_two_rows_per_workgroup_give_the_bits_of_one_row_per_workgroup(K, H):
    """the claim at lstm_fwdk_kernel / lstm_bwdk_kernel: RW rows per workgroup share the weights in registers and every
    row's arithmetic is what RW = 1 does.  (T = 3: both batches' input projections, 1539 and 27 rows, are on the same
    GEMM kernel, so the gates the recurrence starts from have the same bits.)"""
    B, T, D = 513, 3, 9
    big = _shape('two-rows-%d' % H, B, T, D, H)
    assert LC.plan(B, D, H).rows == 2 and LC.DC.launch_batch([LC.DC.Prob(B * T, 4 * H, D, 1, D, 0, 1, D, 0, False, 1, D)])[0] == \
        LC.DC.launch_batch([LC.DC.Prob(9 * T, 4 * H, D, 1, D, 0, 1, D, 0, False, 1, D)])[0]
    p = LC.make_inputs(big)
    idx = torch.tensor([0, 1, 2, 3, 256, 257, 510, 511, 512])       # both rows of workgroups, and the ragged last one's
    small = big._replace(B=len(idx))
    assert LC.plan(small.B, D, H).rows == 1
    p2 = dict(p)
    for k in ('x', 'dout', 'h0', 'c0'):
        p2[k] = p[k][idx].contiguous()
    x1, _, _ = _both(K, big, p)
    x2, _, _ = _both(K, small, p2)
    for q in ('out', 'cs', 'gates', 'dgates', 'hprev', 'hN', 'cN'):
        assert torch.equal(_rows(x1, q, B)[idx], _rows(x2, q, small.B)), q


@pytest.mark.parametrize('kernel', LC.FWD_KERNELS)
def test_t_steps_are_a_bit_exact_prefix_of_t_plus_3_steps(K, kernel):
    c8 = _first(kernel, 8)
    c5 = c8._replace(T=5)
    assert LC.fwd_of(c5) == kernel
    p = LC.make_inputs(c8)
    p5 = dict(p, x=p['x'][:, :5].contiguous(), dout=p['dout'][:, :5].contiguous())
    x8, x5 = LC.build(c8, 'cuda', inputs=p), LC.build(c5, 'cuda', inputs=p5)
    LC.run_forward(K, x8)
    LC.run_forward(K, x5)
    for q in ('out', 'cs', 'gates', 'hprev'):
        a = x8.v[q].detach().cpu().reshape(c8.B, 8, -1)[:, :5]
        b = x5.v[q].detach().cpu().reshape(c8.B, 5, -1)
        assert bool(torch.isfinite(b).all())
        assert torch.equal(a, b), '%s: the first 5 of 8 steps differ from 5 steps' % q
    LC.check_fences(x5)


# ---------------------------------------------------------------------------------------------------------------------
# the stop flag, at the byte level
# ---------------------------------------------------------------------------------------------------------------------
def _flag(v):
    return torch.tensor([v], dtype=torch.int32, device='cuda')


def _stop_case(family, ws):
    """a table case of the family whose backward call has a split-K workspace to take"""
    c = next(c for c in LC.CASES if c.save and LC.plan(c.B, c.D, c.H).family == family and c.T <= 8 and
             LC.ws_floats(c.D, c.H, c.B, c.T) > 0) if family != 'rows16' else LC.BY_ID[next(i for i in LC.BY_ID if i.startswith('r16-ws'))]
    return c._replace(alias=False, ws='exact' if ws else 'none')


@pytest.mark.parametrize('family', ['m', 'k', 'rows16'])
def test_a_set_stop_flag_leaves_every_byte_of_the_forward_outputs(K, family):
    c = _stop_case(family, False)
    x = LC.build(c, 'cuda')
    snap = LC.snapshot(x)
    LC.run_forward(K, x, _flag(1))
    torch.cuda.synchronize()
    LC.assert_untouched(x, snap)
    LC.run_forward(K, x, _flag(0))                     # a clear flag is no flag
    LC.check_forward(x, {})
    LC.check_fences(x)


@pytest.mark.parametrize('ws', [False, True], ids=['unsplit', 'workspace'])
@pytest.mark.parametrize('family', ['m', 'k', 'rows16'])
def test_a_set_stop_flag_leaves_dgates_grads_and_the_workspace(K, family, ws):
    """smx_lstm_backward_f32 under a set flag: neither the recurrence nor the weight-gradient launches run -- dgates, grads
    and ws keep every byte (here their NaN pre-fill), gates stay what the forward pass wrote; aliased, dgates = gates
    keeps the activated gates.  The same buffers then take the call with a clear flag and hold the reference."""
    c = _stop_case(family, ws)
    n = LC.ws_floats(c.D, c.H, c.B, c.T) if ws else 0
    assert not ws or n == K.lstm_backward_ws_floats(LC.problem_net_shape(c), c.B, c.T) > 0
    for alias in (False, True):
        c2 = c._replace(alias=alias)
        x = LC.build(c2, 'cuda', ws_n=n)
        assert ('ws' in x.v) == ws
        LC.run_forward(K, x)
        snap = LC.snapshot(x)
        LC.run_backward(K, x, _flag(1))
        torch.cuda.synchronize()
        LC.assert_untouched(x, snap)
        LC.run_backward(K, x, _flag(0))
        LC.check_backward(x, {}, snap['gates'])
        LC.check_fences(x)


def test_a_misaligned_w_hh_is_refused_before_anything_is_launched(K):
    """the alignment contract of the header: W_hh 16-byte aligned.  A parameter offset of 4 k + 1 floats breaks it; the call
    raises and writes nothing (nothing misaligned is launched)"""
    from surreal_amd.model.ppo_net import LstmParams
    c = LC.BY_ID[next(i for i in LC.BY_ID if i.startswith('k7t-B3-T3'))]
    x = LC.build(c, 'cuda')
    n = LC.param_count(c.D, c.H)
    flat = torch.zeros(n + 8, device='cuda')
    for off in (1, 2, 3):
        flat[off:off + n] = x.v['flat']
        x.net = LstmParams(flat, off, c.D, c.H)
        assert x.net.views['weight_hh'].data_ptr() % 16 != 0
        snap = LC.snapshot(x)
        with pytest.raises(L.SmxError):
            LC.run_forward(K, x)
        torch.cuda.synchronize()
        LC.assert_untouched(x, snap)
    x.net = LstmParams(x.buf['flat'], c.off, c.D, c.H)        # the same buffers, aligned, are accepted
    LC.run_forward(K, x)
    LC.check_forward(x, {})
