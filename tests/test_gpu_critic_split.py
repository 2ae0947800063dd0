"""Layer 1 of the fused critic pass on 3-way split-bf16 MFMA (smx_mlp3_rows16.hip, SPLIT1; K.mlp3_forward_fused's
split_bf16, session_config.learner.critic_split_bf16): against the fp32-MFMA launch (switch off) and against
tests/cpu_kernels.py's double evaluated in float64.

The error requirement: on the same inputs, max and mean absolute error against float64 of the split path are at most
1.5 x those of the fp32 path (a CPU emulation of the six-product sum gives 0.5 x; the factor is the allowance for the
rounding inside one bf16 MFMA).  An error RATIO is a statistic, so every case pools at least 1024 data rows: a case of
r rows per launch is launched ceil(1024 / r) times on fresh x with the same weights (one output of one row has an error
of either sign and any size down to zero, and its ratio says nothing)."""
import math
import types

import numpy as np
import pytest
import torch

from surreal_amd import _lib as L
from cpu_kernels import TorchCpuKernels

ATOL, RTOL = 1e-5, 1e-5
BOUND = 1.5
POOL = 1024
C = TorchCpuKernels()


def split3(w):
    """the pure statement of the planes: hi = RNE(w), mid = RNE(w - hi), lo = RNE(w - hi - mid), in bf16"""
    hi = w.to(torch.bfloat16)
    r1 = w - hi.float()
    mid = r1.to(torch.bfloat16)
    r2 = r1 - mid.float()
    return hi, mid, r2.to(torch.bfloat16)


def test_three_bf16_planes_sum_back_to_fp32_exactly():
    """CPU tier: every finite fp32 value whose low planes stay inside bf16's range is hi + mid + lo exactly; below
    about 2^-110 the low planes flush and the sum degrades towards fewer planes (such values contribute nothing at fp32
    either); Inf gives hi = Inf and NaN below it"""
    g = torch.Generator().manual_seed(0)
    bits = torch.randint(-2 ** 31, 2 ** 31, (200000,), generator=g, dtype=torch.int64).to(torch.int32)
    w = bits.view(torch.float32)
    w = torch.cat([w, torch.tensor([0.0, -0.0, 1.0, -1.0, 1e-30, 1e30, 5.0, -5.0, 2.0 ** -100, 3.0e38, 1.0 + 2.0 ** -23])])
    ok = torch.isfinite(w) & ((w.abs() >= 2.0 ** -100) | (w == 0)) & (w.abs() < 3.3e38)
    w = w[ok]
    hi, mid, lo = split3(w)
    s = hi.double() + mid.double() + lo.double()
    assert torch.equal(s, w.double())
    hi, mid, lo = split3(torch.tensor([float('inf'), float('-inf'), float('nan')]))
    assert torch.isinf(hi[:2]).all() and torch.isnan(mid).all() and torch.isnan(lo).all() and torch.isnan(hi[2])
    tiny = torch.tensor([2.0 ** -125, 1.2345e-38])
    hi, mid, lo = split3(tiny)
    assert float(((hi.double() + mid.double() + lo.double()) - tiny.double()).abs().max()) <= 2.0 ** -133


@pytest.fixture(scope='module')
def K():
    from surreal_amd.kernels import HipKernels
    return HipKernels()


def make_net64(D, H1, H2, OUT, seed, w1_rows=None):
    from surreal_amd.model.ppo_net import Mlp3Params
    g = torch.Generator().manual_seed(seed)
    flat = torch.rand(Mlp3Params.count(D, H1, H2, OUT), generator=g) * 2 - 1
    nc = Mlp3Params(flat.clone(), 0, D, H1, H2, OUT)
    for nm, v in nc.views.items():
        v.mul_(1.0 / np.sqrt(nc.views['W' + nm[1]].shape[1]))
    for r, val in (w1_rows or {}).items():
        nc.views['W1'][r].fill_(val)
    flat32 = torch.cat([v.reshape(-1) for v in nc.views.values()])
    n64 = Mlp3Params(flat32.double(), 0, D, H1, H2, OUT)
    nd = Mlp3Params(flat32.cuda(), 0, D, H1, H2, OUT)
    return n64, nd


def reference64(n64, xm, xt, zm, zs, act):
    rows = xm.shape[0] * (xm.shape[1] + (xt.shape[1] if xt is not None else 0))
    pc = torch.empty(C.mlp3_packed_numel(n64), dtype=torch.float64)
    C.mlp3_pack(n64, pc)
    out = torch.empty(rows * n64.OUT, dtype=torch.float64)
    d = lambda t: None if t is None else t.double()       # noqa: E731
    C.mlp3_forward_fused(pc, n64, d(xm), d(xt), d(zm), d(zs), out, act)
    return out


def launch(K, pd, nd, xm, xt, zm, zs, act, split):
    rows = xm.shape[0] * (xm.shape[1] + (xt.shape[1] if xt is not None else 0))
    od = torch.full((rows * nd.OUT,), float('nan'), device='cuda')
    K.mlp3_forward_fused(pd, nd, xm, xt, zm, zs, od, act, split_bf16=split)
    return od


def zstats_holder(D, g):
    rs = torch.randn(D, generator=g) * 100
    rsq = torch.rand(D, generator=g) * 5000 + 300
    return types.SimpleNamespace(running_sum=rs.cuda(), running_sumsq=rsq.cuda(), count=torch.tensor([1000.0 + 1e-5]).cuda(),
                                 eps=1e-5, _mean=torch.empty(D).cuda(), _std=torch.empty(D).cuda())


# rows per launch G x (T0 + T1): 1 (one lane group live), 16, 129 (a full workgroup plus one row), 300 with T1 = 1
# (ragged last workgroup, obs || obs_next addressing); D 4 (one partial chunk), 36 (a chunk plus 4), 376 (24-wide
# last chunk), 400; hidden sizes on <19,13> and <20,14> and the smallest legal ones; OUT 1 and 17; z: no filter, a
# plain one, one with zstd over 1e-3 .. 1e3 (the clip binds on many elements), and mlp3_pack_zstats as the producer of
# both the planes and the statistics
CASES = [
    (1, 1, 0, 4, 65, 65, 1, 'none'),
    (2, 8, 0, 36, 300, 200, 17, 'plain'),
    (43, 3, 0, 376, 300, 200, 1, 'plain'),
    (100, 2, 1, 376, 304, 208, 1, 'plain'),
    (60, 4, 1, 400, 305, 209, 17, 'none'),
    (43, 3, 0, 376, 300, 200, 1, 'wide'),
    (16, 1, 0, 36, 305, 209, 1, 'stats'),
    (43, 3, 0, 400, 65, 65, 17, 'plain'),
    (1, 16, 0, 4, 300, 200, 1, 'plain'),
]


@pytest.mark.gpu
@pytest.mark.parametrize('G,T0,T1,D,H1,H2,OUT,z', CASES)
def test_split_layer1_error_against_float64_is_within_the_fp32_paths(K, G, T0, T1, D, H1, H2, OUT, z):
    rows = G * (T0 + T1)
    reps = math.ceil(POOL / rows)
    n64, nd = make_net64(D, H1, H2, OUT, 31 * D + H1 + OUT)
    g = torch.Generator().manual_seed(1000 + rows + D)
    xm = torch.randn(reps * G, T0, D, generator=g) * 2 + 0.3
    xt = torch.randn(reps * G, T1, D, generator=g) if T1 else None
    pd = torch.empty(K.mlp3_packed_numel(nd), device='cuda')
    zm = zs = None
    if z == 'stats':
        zf = zstats_holder(D, g)
        K.mlp3_pack_zstats(nd, pd, zf)
        zm, zs = zf._mean.cpu(), zf._std.cpu()
    else:
        K.mlp3_pack(nd, pd)
        if z != 'none':
            zm = torch.randn(D, generator=g) * 0.3
            zs = 10.0 ** (torch.rand(D, generator=g) * 6 - 3) if z == 'wide' else torch.rand(D, generator=g) + 0.5
    act = L.SMX_ACT_NONE if OUT == 1 else L.SMX_ACT_TANH
    ref = reference64(n64, xm, xt, zm, zs, act).view(reps, rows * OUT)
    xmd, xtd = xm.cuda(), (xt.cuda() if T1 else None)
    zmd, zsd = (None, None) if zm is None else (zm.cuda(), zs.cuda())
    on, off = [], []
    for r in range(reps):       # one launch per repetition: G x (T0 + T1) rows each
        a, b = xmd[r * G:(r + 1) * G], (xtd[r * G:(r + 1) * G] if T1 else None)
        on.append(launch(K, pd, nd, a, b, zmd, zsd, act, True))
        off.append(launch(K, pd, nd, a, b, zmd, zsd, act, False))
    on, off = torch.stack(on).cpu().double(), torch.stack(off).cpu().double()
    e_on, e_off = (on - ref).abs(), (off - ref).abs()
    rmax, rmean = float(e_on.max() / e_off.max()), float(e_on.mean() / e_off.mean())
    print('\ncritic-split accuracy rows=%d D=%d H=(%d,%d) OUT=%d z=%s launches=%d: split max %.3e mean %.3e | fp32 max %.3e '
          'mean %.3e | ratio max %.3f mean %.3f' % (rows, D, H1, H2, OUT, z, reps, e_on.max(), e_on.mean(), e_off.max(),
                                                    e_off.mean(), rmax, rmean))
    assert not torch.equal(on, off), 'the split path did not run'
    np.testing.assert_allclose(on.numpy(), ref.numpy(), atol=ATOL, rtol=RTOL, err_msg='split against float64')
    np.testing.assert_allclose(on.numpy(), off.numpy(), atol=ATOL, rtol=RTOL, err_msg='split against the fp32 launch')
    assert rmax <= BOUND and rmean <= BOUND


@pytest.mark.gpu
@pytest.mark.parametrize('producer', ['pack', 'pack_zstats'])
def test_packed_planes_are_the_split_of_w1_in_fragment_order(K, producer):
    """both pack entry points write W1 = hi + mid + lo behind the fp32 image: [chunk][16-feature tile][plane][lane =
    16 (k / 8) + feature][8 k], zero beyond D and H1; the fp32 image in front is what a buffer without planes gets"""
    D, H1, H2, OUT = 36, 300, 200, 1
    n64, nd = make_net64(D, H1, H2, OUT, 5, w1_rows={1: 1e-30, 2: 1e30})
    pd = torch.full((K.mlp3_packed_numel(nd),), float('nan'), device='cuda')
    if producer == 'pack':
        K.mlp3_pack(nd, pd)
    else:
        K.mlp3_pack_zstats(nd, pd, zstats_holder(D, torch.Generator().manual_seed(1)))
    KC, NT = (D + 31) // 32, 20
    nplane = KC * NT * 3 * 64 * 4
    tot = pd.numel() - nplane
    old = torch.full((tot,), float('nan'), device='cuda')       # a buffer of the fp32 image's size: no planes, same image
    K.mlp3_pack(nd, old)
    assert torch.equal(old.view(torch.int32), pd[:tot].view(torch.int32))
    planes = pd[tot:].cpu().view(torch.bfloat16).view(KC, NT, 3, 4, 16, 8)      # [c][t][p][g][fm][j]
    W = torch.zeros(NT * 16, KC * 32)
    W[:H1, :D] = nd.views['W1'].cpu()
    want = torch.stack(split3(W), 0).view(3, NT, 16, KC, 4, 8).permute(3, 1, 0, 4, 2, 5)   # [p][t][fm][c][g][j] -> [c][t][p][g][fm][j]
    assert torch.equal(planes.view(torch.int16), want.contiguous().view(torch.int16))
    s = planes.double().sum(2).permute(1, 3, 0, 2, 4).reshape(NT * 16, KC * 32)           # [c][t][g][fm][j] -> [t][fm][c][g][j]
    assert torch.equal(s, W.double())


@pytest.mark.gpu
@pytest.mark.parametrize('z', [False, True])
def test_special_values_stay_in_their_rows(K, z):
    """a row of zeros, a row with a NaN, rows with +-Inf, one weight row of 1e-30 and one of 1e30: the affected rows
    come out finite or not exactly as on the fp32 path (an Inf may be a NaN here), every other row as always"""
    G, T0, D, H1, H2 = 129, 1, 376, 300, 200
    n64, nd = make_net64(D, H1, H2, 1, 77, w1_rows={2: 1e-30, 4: 1e30})
    g = torch.Generator().manual_seed(9)
    xm = torch.randn(G, T0, D, generator=g) * 2 + 0.3
    xm[3] = 0.0
    xm[5, 0, 100] = float('nan')
    xm[7, 0, 10] = float('inf')
    xm[9, 0, 375] = float('-inf')
    xm[128, 0, 0] = float('inf')
    zm = torch.randn(D, generator=g) * 0.3 if z else None
    zs = torch.rand(D, generator=g) + 0.5 if z else None
    pd = torch.empty(K.mlp3_packed_numel(nd), device='cuda')
    K.mlp3_pack(nd, pd)
    dv = lambda t: None if t is None else t.cuda()       # noqa: E731
    on = launch(K, pd, nd, xm.cuda(), None, dv(zm), dv(zs), L.SMX_ACT_NONE, True).cpu()
    off = launch(K, pd, nd, xm.cuda(), None, dv(zm), dv(zs), L.SMX_ACT_NONE, False).cpu()
    ref = reference64(n64, xm, None, zm, zs, L.SMX_ACT_NONE)
    assert torch.equal(torch.isfinite(on), torch.isfinite(off))
    bad = [5] if z else [5, 7, 9, 128]          # the filter's clip turns +-Inf into +-5
    fin = torch.ones(G, dtype=torch.bool)
    fin[bad] = False
    assert torch.equal(torch.isfinite(on), fin)
    np.testing.assert_allclose(on[fin].numpy(), off[fin].numpy(), atol=ATOL, rtol=RTOL)
    np.testing.assert_allclose(on[fin].double().numpy(), ref[fin].numpy(), atol=ATOL, rtol=RTOL)


@pytest.mark.gpu
@pytest.mark.parametrize('seed', range(6))
def test_split_random_shapes_agree_with_the_cpu_double(K, seed):
    """the sweep of test_mlp3_forward_fused_random_shapes_agree_with_the_32_row_kernel (same ranges) with the switch
    on, at the default tolerance, against the CPU double and the switch-off launch"""
    g = torch.Generator().manual_seed(200 + seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))       # noqa: E731
    D, H1, H2 = 4 * ri(1, 100), ri(65, 320), ri(65, 224)
    OUT = 1 if seed % 2 == 0 else ri(2, 16)
    G, T0, T1 = ri(1, 40), ri(1, 23), ri(0, 1)
    z = bool(seed % 3)
    n64, nd = make_net64(D, H1, H2, OUT, 17 + seed)
    xm = torch.randn(G, T0, D, generator=g) * 2 + 0.3
    xt = torch.randn(G, T1, D, generator=g) if T1 else None
    zm = (torch.randn(D, generator=g) * 0.3) if z else None
    zs = (torch.rand(D, generator=g) + 0.5) if z else None
    act = L.SMX_ACT_NONE if OUT == 1 else L.SMX_ACT_TANH
    ref = reference64(n64, xm, xt, zm, zs, act)
    pd = torch.empty(K.mlp3_packed_numel(nd), device='cuda')
    K.mlp3_pack(nd, pd)
    dv = lambda t: None if t is None else t.cuda()       # noqa: E731
    on = launch(K, pd, nd, xm.cuda(), dv(xt), dv(zm), dv(zs), act, True)
    off = launch(K, pd, nd, xm.cuda(), dv(xt), dv(zm), dv(zs), act, False)
    msg = 'D=%d H1=%d H2=%d OUT=%d rows=%d z=%s' % (D, H1, H2, OUT, G * (T0 + T1), z)
    np.testing.assert_allclose(on.cpu().double().numpy(), ref.numpy(), atol=ATOL, rtol=RTOL, err_msg=msg)
    np.testing.assert_allclose(on.cpu().numpy(), off.cpu().numpy(), atol=ATOL, rtol=RTOL, err_msg=msg)


@pytest.mark.gpu
def test_split_is_deterministic_and_the_fallbacks_are_the_fp32_kernel(K):
    """two launches with the switch on give identical bits; exact-z-filter mode, a packed buffer without planes and the
    launches that keep h1 / h2 (the stem forward) run the fp32 kernels: the bits of the switch-off launch"""
    bits = lambda t: t.view(torch.int32)        # noqa: E731
    G, T0, D, H1, H2 = 300, 1, 376, 300, 200
    n64, nd = make_net64(D, H1, H2, 1, 3)
    g = torch.Generator().manual_seed(4)
    xm = (torch.randn(G, T0, D, generator=g) * 2 + 0.3).cuda()
    zm, zs = (torch.randn(D, generator=g) * 0.3).cuda(), (torch.rand(D, generator=g) + 0.5).cuda()
    pd = torch.empty(K.mlp3_packed_numel(nd), device='cuda')
    K.mlp3_pack(nd, pd)
    a = launch(K, pd, nd, xm, None, zm, zs, L.SMX_ACT_NONE, True)
    b = launch(K, pd, nd, xm, None, zm, zs, L.SMX_ACT_NONE, True)
    off = launch(K, pd, nd, xm, None, zm, zs, L.SMX_ACT_NONE, False)
    assert torch.equal(bits(a), bits(b)) and not torch.equal(bits(a), bits(off))
    try:
        K.fused_exact_zfilter(True)
        ex_on = launch(K, pd, nd, xm, None, zm, zs, L.SMX_ACT_NONE, True)
        ex_off = launch(K, pd, nd, xm, None, zm, zs, L.SMX_ACT_NONE, False)
        ex_on_nz = launch(K, pd, nd, xm, None, None, None, L.SMX_ACT_NONE, True)
    finally:
        K.fused_exact_zfilter(False)
    off_nz = launch(K, pd, nd, xm, None, None, None, L.SMX_ACT_NONE, False)
    assert torch.equal(bits(ex_on), bits(ex_off)) and torch.equal(bits(ex_on_nz), bits(off_nz))
    short = pd[:pd.numel() - ((D + 31) // 32) * 20 * 3 * 64 * 4].clone()       # the fp32 image alone
    assert torch.equal(bits(launch(K, short, nd, xm, None, zm, zs, L.SMX_ACT_NONE, True)), bits(off))
    # the launch that keeps h1 / h2 (K.mlp3_forward with a pack buffer, from FUSED_ROWS_MIN rows on)
    rows, D2 = K.FUSED_ROWS_MIN + 77, 36
    n64, nd = make_net64(D2, H1, H2, 1, 8)
    x = torch.randn(rows, D2, generator=g).cuda()
    h1, h2, o = torch.empty(rows, H1).cuda(), torch.empty(rows, H2).cuda(), torch.empty(rows, 1).cuda()
    pk = torch.empty(K.mlp3_packed_numel(nd), device='cuda')
    K.mlp3_forward(nd, x, h1, h2, o, L.SMX_ACT_NONE, pack=pk)
    off = launch(K, pk, nd, x.view(rows, 1, D2), None, None, None, L.SMX_ACT_NONE, False)
    assert torch.equal(bits(o.view(-1)), bits(off))
