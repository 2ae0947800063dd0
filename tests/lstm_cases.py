"""The LSTM recurrence (csrc/smx_lstm.hip: smx_lstm_forward_f32 / smx_lstm_backward_f32, 9 forward and 6 backward kernel
instantiations) pinned down by itself: the case table, the poisoned buffers the cases run in, a float64 reference, and a
pure-Python restatement of the host dispatch.  Shared by test_lstm_cpu.py (the table on the torch-CPU double, the coverage
conditions, nine deliberately wrong doubles) and test_gpu_lstm.py (the same table on the HIP kernels, the bit-level
properties, the stop flag).

Reference.  reference() restates forward and backward in float64 with the equations of aten::lstm_cell (gates =
x W_ih^T + b_ih + h W_hh^T + b_hh, order i, f, g, o; c' = f c + i g; h' = o tanh c') and returns out, hN, cN, the saved
tensors (activated gates, c_t, h_{t-1}), dgates and the four gradient blocks.  test_lstm_cpu.py checks it against
torch.nn.LSTM(...).double() and autograd.

Inputs.  Weights and biases are +-u s with u uniform in [0.5, 1] and a random sign (no near-zero weight: every term
matters), s = 0.3 at H <= 16, 0.1 below H = 256, 0.05 from there on; x and dout standard normal, h0 and c0 0.3 normal.
At s = 1 the recurrence is chaotic and float32 against float64 says nothing, so problem() ASSERTS on the CPU, for every
case, that ATen in float32 (torch.nn.LSTM + autograd) agrees with the float64 reference to 1e-6 on `out` and to 2e-6 of
each gradient block's own maximum: a case that fails is a bad case, not a loose tolerance.  One case per forward kernel
has b_hh = +-6 on the i, f and g blocks (random sign per unit): both sigmoid tails, the tanh tails of the cell candidate and,
with f = 1 and i g = +-1 for steps on end, of tanh(c_t) at |c_t| up to 7 -- where fast_sigm / fast_tanh (smx_lstm_act.inc.h)
differ most from libm.  The o block stays unsaturated: with all four in the tails every gradient carries the 2.4e-5
relative error of 1 - 0.9975 formed from a float32 gate, and ATen float32 itself is 4e-6 of the block maxima from float64.
With many rows the bias gradients are sums of B T terms of either sign (max|db| grows as sqrt(B T), the rounding of the
sum faster): at B = 513 ATen float32 sits between 1e-6 and 5e-6 of max|db| whatever T is, so the B >= 512 cases are the
draws (SALTS) that it holds to the bound.

Tolerances.  out, hN, cN, gates, c_t, h_{t-1}: 1e-5 absolute against float64 (the project's bar).  dgates and each of dW_ih,
dW_hh, db_ih, db_hh separately: |diff| <= 2e-6 max|ref of that block| + 1e-5 |ref| (the bar of
test_lstm_forward_backward_match_aten, per block instead of over the whole gradient).  If a quantity of a case exceeds its
bar, check() computes ATen-float32's error on that case against the same reference and the bar becomes max(bar, 4 x that
error) -- 4 for another summation order plus the 1.5e-7 of the hardware exp / rcp; such a (case, quantity) must be listed
in REPLACED_BARS below with both numbers, anything beyond is a kernel bug.

Poisoned surroundings.  x, h0, c0, dout and the flat parameter vector (reached through LstmParams(flat, off, D, H)) each
sit in a larger flat buffer that is NaN in front of and behind the logical extent.  Every output -- gates, out, cs, hprev,
hN, cN, dgates, grads, ws -- is a flat buffer of the sentinel -7777 whose logical region is pre-filled with NaN: after the
call the logical region must be finite and equal the reference (for grads: overwritten, not accumulated) and every other
element must still hold the sentinel's bytes.

Alignment contract.  lstm_fwdm_kernel and lstm_fwd_kernel read W_hh rows as float4 (W_hh + col * H + 4 q), every other
global access of the 15 kernels is a scalar float: W_hh must be 16-byte aligned and H a multiple of 4, nothing else needs
more than 4 bytes.  Inside [W_ih | W_hh | b_ih | b_hh] W_hh is 4 H D floats behind W_ih, a multiple of 4, so the contract is
a parameter offset that is a multiple of 4 floats in a 16-byte aligned vector.  PPOModel keeps it (the actor block and the
CNN block are padded to multiples of 4 floats, an LSTM layer's count 4 H (D + H + 2) is one); smx_lstm_forward_f32
refuses a W_hh that is not (test_gpu_lstm.py tests the refusal, nothing misaligned is ever launched).  All front offsets
here are multiples of 4 floats, which also keeps the projection and weight-gradient GEMMs on the operand modes they have
in the learner.

Dispatch.  plan() restates lstm_plan(); fwd_kernel() / bwd_kernel() give the instantiation names it implies.  A kernel
trace of test_gpu_lstm.py alone (profiles/lstm_paths_kernel_stats.csv) shows all 15 names.

Long sequences.  T = 131 (past the workload's 124 - 129) runs on every kernel that takes B = 1; the kernels that need
B >= 512 (lstm_fwdm / bwdm, the two-row lstm_fwdk / bwdk) run T = 37 at B = 513 instead: 513 x 131 x 4 H floats are 108 MB a
tensor and several seconds of float64 reference, 513 x 37 are 30 MB.
"""
import collections
import functools
import zlib

import torch

import dense_cases as DC

SENTINEL = -7777.0
TAIL = 8
ABS_FWD = 1e-5                 # out, hN, cN and the saved tensors against float64
REL_BLOCK, REL_ELEM = 2e-6, 1e-5     # dgates and each gradient block: REL_BLOCK * max|ref| + REL_ELEM * |ref|
COND_OUT, COND_GRAD = 1e-6, 2e-6     # what ATen float32 must meet for a case to be in the table
LONG_T, LONG_T_MANY = 131, 37
MROWS_MIN_B = 512

FWD_Q = ('out', 'hN', 'cN', 'gates', 'cs', 'hprev')
GRAD_Q = ('dW_ih', 'dW_hh', 'db_ih', 'db_hh')
BWD_Q = ('dgates',) + GRAD_Q

# (case id, quantity) -> (the bar's ratio observed on the MI355X, ATen-float32's error it was replaced by 4 x of).
# Empty: the per-block bars and the T = 131 cases held on the first GPU run (profiles/lstm_cases_errors.txt: the worst
# is dW_ih at 0.67 of its bar).
REPLACED_BARS = {}

# A case's id seeds its inputs.  Where the first draw missed the conditioning assertion, or met it by less than a
# quarter (ATen's own float32 sums depend on the CPU and its thread count), the id carries a salt: the first one whose draw
# ATen float32 holds to 1.5e-6 of every gradient block's maximum.  Chosen on the CPU by ATen against float64 alone.  At
# B = 513 x T = 37 (18 981 rows) such draws are rare, about one in 300 -- hence salts of 69 to 354 on the five long
# B >= 512 cases; at T <= 8 the first or second draw does.
SALTS = {'m25t-long-B513-T37-D17-H100-6': 195, 'm25f-B516-T5-D24-H100-4': 1, 'm25f-long-B513-T37-D24-H100-6': 344,
         'm28t-B519-T8-D9-H108-5': 2, 'm28t-long-B513-T37-D9-H108-6': 163, 'm28f-long-B513-T37-D24-H112-6': 69,
         'm28f-sat-B513-T7-D24-H112-8': 2, 'k8x2-long-B513-T37-D9-H116-6': 354, 'k8x2-sat-B513-T7-D9-H116-8': 2,
         'small-m-B513-T6-D5-H8-10': 1, 'r16-ws-B17-T131-D11-H132-13': 1, 'edge-H112-B513-T6-D9-H112-10': 2,
         'edge-B512-B512-T5-D9-H128-10': 1, 'edge-D-B513-T6-D20-H100-11': 1, 'edge-D-B513-T6-D21-H100-10': 1,
         'fold-m-B514-T6-D1-H100-12': 4, 'fold-m-B514-T6-D1-H108-11': 2}

Case = collections.namedtuple('Case', 'id B T D H h0 c0 save alias ws sat off')
Plan = collections.namedtuple('Plan', 'family fwd_w bwd_w rows fold')


# ---------------------------------------------------------------------------------------------------------------------
# the host dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------
def plan(B, D, H):
    """lstm_plan(): (family, forward width, backward width, batch rows per workgroup, fold)"""
    many = B >= MROWS_MIN_B
    fold = H <= 112 and D <= 20
    if H <= 112 and many:
        w = 25 if H <= 100 else 28
        return Plan('m', w, w, 4, fold)
    if H <= 128:
        return Plan('k', 7 if H <= 112 else 8, 13 if H <= 104 else 16, 2 if many else 1, fold)
    return Plan('rows16', 24, 24, 16, fold)


def fwd_kernel(B, D, H):
    p = plan(B, D, H)
    fold = 'true' if p.fold else 'false'
    if p.family == 'm':
        return 'lstm_fwdm_kernel<%d, %s>' % (p.fwd_w, fold)
    if p.family == 'k':
        return 'lstm_fwdk_kernel<%d, %d, %s>' % (p.fwd_w, p.rows, fold)
    return 'lstm_fwd_kernel<24>'


def bwd_kernel(B, D, H):
    p = plan(B, D, H)
    if p.family == 'm':
        return 'lstm_bwdm_kernel<%d>' % p.bwd_w
    if p.family == 'k':
        return 'lstm_bwdk_kernel<%d, %d>' % (p.bwd_w, p.rows)
    return 'lstm_bwd_kernel<24>'


FWD_KERNELS = ('lstm_fwdm_kernel<25, true>', 'lstm_fwdm_kernel<25, false>', 'lstm_fwdm_kernel<28, true>',
               'lstm_fwdm_kernel<28, false>', 'lstm_fwdk_kernel<7, 1, true>', 'lstm_fwdk_kernel<7, 1, false>',
               'lstm_fwdk_kernel<8, 1, false>', 'lstm_fwdk_kernel<8, 2, false>', 'lstm_fwd_kernel<24>')
BWD_KERNELS = ('lstm_bwdm_kernel<25>', 'lstm_bwdm_kernel<28>', 'lstm_bwdk_kernel<13, 1>', 'lstm_bwdk_kernel<16, 1>',
               'lstm_bwdk_kernel<16, 2>', 'lstm_bwd_kernel<24>')


def fwd_of(c):
    return fwd_kernel(c.B, c.D, c.H)


def bwd_of(c):
    return bwd_kernel(c.B, c.D, c.H)


def ws_floats(D, H, B, T):
    """smx_lstm_backward_ws_floats: both weight gradients' split-K partials (smx_linear_wgrad_ws_floats twice)"""
    n = 0
    for N in (D, H):
        S = DC.pick_splits(4 * H, N, B * T)
        n += S * (4 * H * N + 4 * H) if S > 1 else 0
    return n


def param_count(D, H):
    return 4 * H * D + 4 * H * H + 8 * H


def scale_of(H):
    return 0.3 if H <= 16 else (0.1 if H < 256 else 0.05)


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
_CELLS = ((True, True), (False, False), (True, False), (False, True))        # (h0, c0)
_count = collections.Counter()
_ws_turn = collections.Counter()


def case(tag, B, T, D, H, save=True, sat=False, ws=None, cells=None, alias=None):
    f, b = fwd_kernel(B, D, H), bwd_kernel(B, D, H)
    i = _count[f]
    _count[f] += 1
    h0, c0 = _CELLS[i % 4] if cells is None else cells
    if alias is None:
        alias = i % 2 == 0
    if ws is None:                 # every second case of a backward kernel that has a workspace to give takes it
        ws = 'none'
        if save and ws_floats(D, H, B, T) > 0:
            _ws_turn[b] += 1
            ws = 'exact' if _ws_turn[b] % 2 else 'none'
    cid = '%s-B%d-T%d-D%d-H%d-%d' % (tag, B, T, D, H, i)
    if cid in SALTS:
        cid += '-s%d' % SALTS[cid]
    return Case(cid, B, T, D, H, h0, c0, save, alias, ws, sat, (0, 4, 8, 12)[i % 4])


# one sweep per forward kernel: (tag, D, H, the B of each step count, the B of the long sequence)
_MANY_B = (512, 513, 514, 515, 516, 519)
_SWEEPS = (('m25t', 17, 100, _MANY_B, 513), ('m25f', 24, 100, _MANY_B, 513), ('m28t', 9, 108, _MANY_B, 513),
           ('m28f', 24, 112, _MANY_B, 513), ('k7t', 17, 100, (1, 2, 3, 5, 37, 7), 1), ('k7f', 24, 104, (1, 2, 3, 5, 37, 7), 1),
           ('k8', 9, 128, (1, 2, 3, 5, 37, 7), 1), ('k8x2', 9, 116, _MANY_B, 513), ('r16', 11, 132, (1, 16, 17, 33, 40, 15), 1))
_SWEEP_T = (1, 2, 3, 4, 5, 8)


def _table():
    T = []
    for tag, D, H, Bs, long_b in _SWEEPS:
        for B, steps in zip(Bs, _SWEEP_T):
            T.append(case(tag, B, steps, D, H))
        T.append(case(tag + '-long', long_b, LONG_T_MANY if long_b >= MROWS_MIN_B else LONG_T, D, H))
        # hprev = None and hN / cN = None (forward only), and the bias-saturated case
        T.append(case(tag + '-nosave', Bs[2], 6, D, H, save=False))
        T.append(case(tag + '-sat', Bs[1] if Bs[1] > 1 else 3, 7, D, H, sat=True))
    # ---- size extremes.  H = 4: QS = 1, a k-quarter is one float, lstm_bwdk's odd eighths hold no word at all
    for H in (4, 8, 16):
        T.append(case('small', 3, 6, 5, H))
    for H in (4, 8):
        T.append(case('small-m', 513, 6, 5, H))
    T.append(case('small-nofold', 5, 6, 24, 12))
    T.append(case('partial-wave', 514, 6, 24, 52))        # lstm_fwdm / bwdm: the fourth wave holds 4 of its 16 units
    for B, H in ((17, 140), (20, 256), (16, 384), (17, 384)):     # 16-row: H mod 16 != 0; the largest LDS request
        T.append(case('r16-H', B, 6, 11, H))
    T.append(case('r16-ws', 17, LONG_T, 11, 132))         # 2227 rows: the 16-row kernels with a split-K workspace
    # ---- both sides of every selection boundary (the other side of each is in a sweep above)
    T.append(case('edge-H104', 513, 6, 17, 104))          # H 100 | 104 at B >= 512: the m width
    T.append(case('edge-H108', 3, 6, 17, 108))            # H 104 | 108 at B < 512: lstm_bwdk 13 -> 16
    T.append(case('edge-H112', 3, 6, 9, 112))             # H 112 | 116 at B < 512: lstm_fwdk 7 -> 8, the fold ends
    T.append(case('edge-H116', 3, 6, 9, 116))
    T.append(case('edge-H112', 513, 6, 9, 112))           # H 112 | 116 at B >= 512: m -> two rows on the vector kernels
    T.append(case('edge-H128', 513, 6, 9, 128))           # H 128 | 132 at B >= 512 and below
    T.append(case('edge-H132', 513, 3, 9, 132))
    T.append(case('edge-H132', 3, 6, 9, 132))
    T.append(case('edge-B511', 511, 5, 17, 100))          # B 511 | 512 at H <= 112 and at 112 < H <= 128 (2555 rows:
    T.append(case('edge-B511', 511, 5, 9, 128))           # lstm_bwdk<13, 1> / <16, 1> with a workspace)
    T.append(case('edge-B512', 512, 5, 9, 128))
    for D in (20, 21):                                    # D 20 | 21
        T.append(case('edge-D', 3, 6, D, 100))
        T.append(case('edge-D', 513, 6, D, 100))
    # ---- folded D: the staging lanes split the inputs xj / 5, the quad's lanes take 5 / 5 / 5 / 5 of them
    for D in (1, 5, 6, 10, 11, 15, 16, 20):
        T.append(case('fold', 3, 7, D, 100 if D % 2 else 112))
    for H in (100, 108):
        for D in (1, 6, 20):
            T.append(case('fold-m', 514, 6, D, H))
    return T


CASES = _table()
BY_ID = {c.id: c for c in CASES}
SMALL = [c for c in CASES if c.B * c.T * c.H <= 40000]


# ---------------------------------------------------------------------------------------------------------------------
# inputs, the float64 reference, ATen float32 next to it
# ---------------------------------------------------------------------------------------------------------------------
def _gen(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


def _weights(g, shape, s):
    u = 0.5 + 0.5 * torch.rand(shape, generator=g)
    sign = (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()
    return u * sign * s


def make_inputs(c):
    """float32 inputs of a case: x, dout, h0, c0 (None where the case passes none) and the four parameter tensors"""
    g = _gen(c.id)
    s = scale_of(c.H)
    p = dict(W_ih=_weights(g, (4 * c.H, c.D), s), W_hh=_weights(g, (4 * c.H, c.H), s), b_ih=_weights(g, (4 * c.H,), s),
             b_hh=_weights(g, (4 * c.H,), s))
    if c.sat:                      # +-6 on the i, f and g blocks (see the docstring)
        p['b_hh'][:3 * c.H] = 6.0 * (torch.randint(0, 2, (3 * c.H,), generator=g) * 2 - 1).float()
    p['x'] = torch.randn(c.B, c.T, c.D, generator=g)
    p['dout'] = torch.randn(c.B, c.T, c.H, generator=g)
    h0, c0 = 0.3 * torch.randn(c.B, c.H, generator=g), 0.3 * torch.randn(c.B, c.H, generator=g)
    p['h0'], p['c0'] = (h0 if c.h0 else None), (c0 if c.c0 else None)
    return p


def reference(p, backward=True):
    """forward and backward in float64 -> dict of float64 tensors"""
    d = lambda t: t.double()  # noqa: E731
    W_ih, W_hh, b_ih, b_hh, x = d(p['W_ih']), d(p['W_hh']), d(p['b_ih']), d(p['b_hh']), d(p['x'])
    B, T, _ = x.shape
    H = W_hh.shape[1]
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    h = d(p['h0']).clone() if p['h0'] is not None else z(B, H)
    c = d(p['c0']).clone() if p['c0'] is not None else z(B, H)
    c_init = c.clone()
    gates, out, cs, hprev = z(B, T, 4 * H), z(B, T, H), z(B, T, H), z(B, T, H)
    for t in range(T):
        pre = (x[:, t] @ W_ih.t() + b_ih) + (h @ W_hh.t() + b_hh)
        i, f, g, o = pre.chunk(4, 1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        hprev[:, t] = h
        c = f * c + i * g
        h = o * torch.tanh(c)
        gates[:, t] = torch.cat([i, f, g, o], 1)
        out[:, t], cs[:, t] = h, c
    w = dict(out=out, hN=h, cN=c, gates=gates, cs=cs, hprev=hprev)
    if not backward:
        return w
    dout = d(p['dout'])
    dgates = z(B, T, 4 * H)
    dh_rec, dc_rec = z(B, H), z(B, H)
    for t in range(T - 1, -1, -1):
        i, f, g, o = gates[:, t].chunk(4, 1)
        cp = cs[:, t - 1] if t > 0 else c_init
        dh = dout[:, t] + dh_rec
        tc = torch.tanh(cs[:, t])
        dc = dc_rec + dh * o * (1 - tc * tc)
        dg = torch.cat([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
        dgates[:, t] = dg
        dc_rec = dc * f
        dh_rec = dg @ W_hh
    d2 = dgates.reshape(B * T, 4 * H)
    w.update(dgates=dgates, dW_ih=d2.t() @ x.reshape(B * T, -1), dW_hh=d2.t() @ hprev.reshape(B * T, H), db_ih=d2.sum(0),
             db_hh=d2.sum(0))
    return w


def aten_lstm(p, dtype=torch.float32, backward=True):
    """torch.nn.LSTM (+ autograd) on the same inputs -> out, hN, cN and the four parameter gradients in `dtype`.  On one
    thread: how ATen cuts its float32 sums must not depend on the machine's core count"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _aten_lstm(p, dtype, backward)
    finally:
        torch.set_num_threads(threads)


def _aten_lstm(p, dtype, backward):
    H, D = p['W_hh'].shape[1], p['W_ih'].shape[1]
    B = p['x'].shape[0]
    m = torch.nn.LSTM(D, H, 1, batch_first=True).to(dtype)
    names = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')
    with torch.no_grad():
        for n, k in zip(names, ('W_ih', 'W_hh', 'b_ih', 'b_hh')):
            getattr(m, n).copy_(p[k].to(dtype))
    zero = torch.zeros(B, H, dtype=dtype)
    h0 = p['h0'].to(dtype) if p['h0'] is not None else zero
    c0 = p['c0'].to(dtype) if p['c0'] is not None else zero
    out, (hN, cN) = m(p['x'].to(dtype), (h0[None], c0[None]))
    r = dict(out=out.detach(), hN=hN[0].detach(), cN=cN[0].detach())
    if backward:
        (out * p['dout'].to(dtype)).sum().backward()
        for n, k in zip(names, GRAD_Q):
            r[k] = getattr(m, n).grad
    return r


class Problem(object):
    """a case's inputs, its float64 reference and ATen-float32's distance from it (all on the CPU, never modified)"""
    pass


@functools.lru_cache(maxsize=3)
def problem(c):
    P = Problem()
    P.case, P.inputs = c, make_inputs(c)
    P.want = reference(P.inputs, backward=c.save)
    a = aten_lstm(P.inputs, backward=c.save)
    P.aten_err = {k: float((v.double() - P.want[k]).abs().max()) for k, v in a.items()}
    # the conditioning assertion: float32 against float64 must mean something on this case
    assert P.aten_err['out'] <= COND_OUT, '%s: ATen float32 is %g from float64 on out: a bad case' % (c.id, P.aten_err['out'])
    for k in GRAD_Q if c.save else ():
        top = float(P.want[k].abs().max())
        assert P.aten_err[k] <= COND_GRAD * top, '%s: ATen float32 is %g of max|%s| from float64: a bad case' % (
            c.id, P.aten_err[k] / top, k)
    return P


def aten_error(P, q):
    """ATen-float32's largest error on quantity q of this case: torch.nn.LSTM where it gives q, else (the saved tensors,
    dgates) the torch-CPU double, which is the same equations on ATen float32 operators"""
    if q not in P.aten_err:
        from cpu_kernels import TorchCpuKernels
        x = build(P.case, 'cpu')
        run_forward(TorchCpuKernels(), x)
        got = {k: x.v[k].clone() for k in ('gates', 'cs', 'hprev') if k in x.v}
        if P.case.save:
            run_backward(TorchCpuKernels(), x)
            got['dgates'] = (x.v['gates'] if P.case.alias else x.v['dgates']).clone()
        for k, v in got.items():
            P.aten_err[k] = float((v.double().reshape(-1) - P.want[k].reshape(-1)).abs().max())
    return P.aten_err[q]


# ---------------------------------------------------------------------------------------------------------------------
# buffers, the two calls, checks
# ---------------------------------------------------------------------------------------------------------------------
class Built(object):
    """one case's buffers on a device: .buf[name] the flat buffer, .span[name] = (off, n) its logical extent, .v[name] the
    logical view handed to the kernels, .net the LstmParams over the poisoned parameter vector"""
    pass


def _in(x, name, t, off, device):
    n = t.numel()
    buf = torch.full((off + n + TAIL,), float('nan'))
    buf[off:off + n] = t.reshape(-1)
    buf = buf.to(device)
    x.buf[name], x.span[name], x.v[name] = buf, (off, n), buf[off:off + n].view(t.shape)


def _out(x, name, shape, off, device):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((off + n + TAIL,), SENTINEL)
    buf[off:off + n] = float('nan')
    buf = buf.to(device)
    x.buf[name], x.span[name], x.v[name] = buf, (off, n), buf[off:off + n].view(shape)
    x.outputs.append(name)


def build(c, device='cpu', ws_n=0, inputs=None):
    """the buffers of a case; `inputs`: other inputs of the case's shape (no reference then: the bit-level tests)"""
    from surreal_amd.model.ppo_net import LstmParams
    P = problem(c) if inputs is None else None
    p = P.inputs if inputs is None else inputs
    x = Built()
    x.case, x.P, x.buf, x.span, x.v, x.outputs = c, P, {}, {}, {}, []
    B, T, D, H = c.B, c.T, c.D, c.H
    _in(x, 'flat', torch.cat([p[k].reshape(-1) for k in ('W_ih', 'W_hh', 'b_ih', 'b_hh')]), c.off, device)
    x.net = LstmParams(x.buf['flat'], c.off, D, H)
    assert x.net.views['weight_hh'].data_ptr() % 16 == 0
    _in(x, 'x', p['x'].reshape(B * T, D), 4, device)
    _in(x, 'dout', p['dout'], 8, device)
    for k in ('h0', 'c0'):
        if p[k] is not None:
            _in(x, k, p[k], 4, device)
    _out(x, 'gates', (B * T, 4 * H), 4, device)
    _out(x, 'out', (B, T, H), 8, device)
    _out(x, 'cs', (B * T, H), 4, device)
    if c.save:
        _out(x, 'hprev', (B * T, H), 8, device)
        _out(x, 'hN', (B, H), 4, device)
        _out(x, 'cN', (B, H), 8, device)
        if not c.alias:
            _out(x, 'dgates', (B * T, 4 * H), 8, device)
        _out(x, 'grads', (param_count(D, H),), 4, device)
        if c.ws == 'exact' and ws_n > 0:
            _out(x, 'ws', (ws_n,), 4, device)
    return x


def run_forward(kern, x, stop=None):
    c, v = x.case, x.v
    kern.lstm_forward(x.net, v['x'], c.B, c.T, v.get('h0'), v.get('c0'), v['gates'], v['out'], v['cs'], v.get('hprev'),
                      v.get('hN'), v.get('cN'), stop=stop)


def run_backward(kern, x, stop=None):
    c, v = x.case, x.v
    kern.lstm_backward(x.net, v['x'], c.B, c.T, v.get('c0'), v['gates'], v['cs'], v['hprev'], v['dout'],
                       v['gates'] if c.alias else v['dgates'], v['grads'], stop, ws=v.get('ws'))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def snapshot(x, names=None):
    return {k: bits(x.buf[k]).clone() for k in (names or x.outputs)}


def assert_untouched(x, snap, names=None):
    for k in names or sorted(snap):
        assert torch.equal(bits(x.buf[k]), snap[k]), '%s: %s was written' % (x.case.id, k)


def check_fences(x):
    sent = bits(torch.tensor([SENTINEL]))[0]
    for k in x.outputs:
        off, n = x.span[k]
        b = bits(x.buf[k])
        bad = int((b[:off] != sent).sum()) + int((b[off + n:] != sent).sum())
        assert bad == 0, '%s: %d elements outside the logical extent of %s were written' % (x.case.id, bad, k)
    for k in ('flat', 'x', 'dout', 'h0', 'c0'):            # the inputs are inputs
        if k in x.buf:
            off, n = x.span[k]
            b = x.buf[k].detach().cpu()
            assert bool(torch.isnan(b[:off]).all()) and bool(torch.isnan(b[off + n:]).all()) and \
                bool(torch.isfinite(b[off:off + n]).all()), '%s: input %s was written' % (x.case.id, k)


def _judge(x, q, got, bar, record):
    """got against the reference of q under the element-wise bar; the 4 x ATen rule where the bar is missed"""
    cid, want = x.case.id, x.P.want[q].reshape(-1)
    got = got.detach().cpu().double().reshape(-1)
    assert got.numel() == want.numel()
    assert bool(torch.isfinite(got).all()), '%s: %d elements of %s are not finite (never written?)' % (
        cid, int((~torch.isfinite(got)).sum()), q)
    diff = (got - want).abs()
    ratio = float((diff / bar).max())
    note = ''
    if ratio > 1.0:
        e = aten_error(x.P, q)
        ratio2 = float((diff / torch.clamp(bar, min=4.0 * e)).max())
        note = ' bar missed at %.3f; ATen float32 error %.3g, 4 x that gives %.3f' % (ratio, e, ratio2)
        assert ratio2 <= 1.0, '%s: %s: max |diff| %.3g;%s: a kernel bug' % (cid, q, float(diff.max()), note)
        assert (cid, q) in REPLACED_BARS, '%s: %s:%s -- list it in lstm_cases.REPLACED_BARS' % (cid, q, note)
        ratio = ratio2
    record[q] = (ratio, note)


def _abs_bar(want):
    return torch.full((want.numel(),), ABS_FWD, dtype=torch.float64)


def _block_bar(want):
    w = want.reshape(-1).abs()
    return REL_BLOCK * w.max() + REL_ELEM * w


def check_forward(x, record):
    for q in FWD_Q:
        if q in x.v:
            _judge(x, q, x.v[q], _abs_bar(x.P.want[q]), record)


def check_backward(x, record, gates_before=None):
    c, want = x.case, x.P.want
    _judge(x, 'dgates', x.v['gates'] if c.alias else x.v['dgates'], _block_bar(want['dgates']), record)
    if not c.alias:
        assert torch.equal(bits(x.buf['gates']), gates_before), '%s: the backward pass changed gates' % c.id
    g = x.v['grads'].detach().cpu()
    o = 0
    for q in GRAD_Q:
        n = want[q].numel()
        _judge(x, q, g[o:o + n], _block_bar(want[q]), record)
        o += n
    assert o == g.numel()


def run_entry(kern, c, device='cpu'):
    """one table entry: the forward call, its checks, the backward call, its checks, every fence -> (built, record);
    record[quantity] = (observed error / bar, note)"""
    n = 0
    if c.save and c.ws == 'exact':
        n = ws_floats(c.D, c.H, c.B, c.T)
        if device != 'cpu':
            assert kern.lstm_backward_ws_floats(problem_net_shape(c), c.B, c.T) == n, c.id
    x = build(c, device, ws_n=n)
    record = {}
    run_forward(kern, x)
    check_forward(x, record)
    if c.save:
        before = bits(x.buf['gates']).clone()
        run_backward(kern, x)
        check_backward(x, record, before)
        for k in ('out', 'cs', 'hprev', 'hN', 'cN'):        # the backward pass writes dgates, grads and ws only
            _judge(x, k, x.v[k], _abs_bar(x.P.want[k]), {})
    check_fences(x)
    return x, record


class _Shape(object):
    def __init__(self, D, H):
        self.D, self.H = D, H


def problem_net_shape(c):
    """what K.lstm_backward_ws_floats reads of a net"""
    return _Shape(c.D, c.H)
