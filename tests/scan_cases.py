"""The kernels of csrc/smx_scan.hip (windowed GAE with and without the in-launch normalisation, batch moments and their
merge, the advantage normalisation, the z-filter's statistics / forward / update in both forms, the reward filter) pinned
down by themselves: the case table, the poisoned buffers the cases run in, a float64 numpy reference, derived bounds and a
Python restatement of the host side (path(), zupdate_chunks()).  Shared by test_scan_cpu.py (the table on the torch-CPU
double, the coverage conditions, thirteen deliberately wrong doubles) and test_gpu_scan.py (the same table on the HIP
kernels, the bit-level properties, the refusals, the margins report).

Reference.  gae_reference() is the formulas the kernel comments cite (ppo.py:387-418) in float64 numpy: values[:, 1:]
masked by 1 - dones, delta = r + gamma v' - v, window sums with the gpow / lpow tables, ret = sum gpow r + v[s + H]
gamma^H.  It takes the float32 gpow, lpow, gamma and gamma_H the kernel gets, widened: how the powers were formed is not
the kernel's error.  With every output it returns S, the sum of the absolute values of what was added up:
advantages sum_k gpow lpow (|r| + gamma |v'| + |v|), returns sum gpow |r| + gamma^H |v|.  It shares no code with
cpu_kernels.py or oracle/ppo_oracle.py.

Bound.  sum_bound(d, c, S) = (d + c) 2^-24 S.  A float32 sum whose longest chain of additions has depth d, over terms
t_k with sum |t_k| = S, is within d u S (1 + O(d u)) of the exact sum (u = 2^-24; Higham, Accuracy and Stability,
eq. 4.4: each partial sum is rounded once and no term passes through more than d additions); a term that was itself
formed with c roundings, each relative to no more than the term's absolute value, adds c u |t_k|.  d is the kernel's
own chain length:
    GAE, E = 1         ceil(N / 64) + 6   a lane's stride-64 chain, then the 6 butterfly steps (the bootstrap term of the
                                          return is one more addition: the chain's first trip adds to zero, exactly)
    GAE, E > 1         H                  one lane per window, H terms in order
    z-update           ceil(rows / 16) + 16 on the one-launch form (16 row-lanes, then the 16 of them in order),
                       ceil(per / 32) + 16 + chunks on the workspace form; S = sum |x| and sum x^2, plus one rounding of
                       the running sum it is added to
c is 4 for an advantage term and 2 for a return term.  (Uncontracted, an advantage term takes five roundings --
gamma v', + r, - v, * gpow, * lpow -- the first two relative to a part of the term only; hipcc contracts gamma v' + r and
the accumulation into FMAs, which leaves three.)  The bound is derived, not fitted: problem() ASSERTS on the CPU, before
a case is accepted, that a float32 numpy emulation of the kernel's order without any FMA -- lane-strided chains, then a
tree -- stays inside it; a case that fails that is a bad case.  What the device accumulates in float64 (moments, their
merge, the reward filter's sums, gae_norm's moments) is compared with the float64 reference to 2 float32 ulps of each
number; what is normalised in float32 (adv_normalize, the z-filter and reward-filter outputs) to the project's
1e-5 absolute + 1e-5 relative.  gae_norm's moments and normalised advantages are judged against float64 moments and a
float64 normalisation of the float32 advantages the launch itself formed (the `gae` launch: the same bits): the error
of those sums has its own bound one line earlier and is not counted twice.

Inputs.  Values 3 x normal, rewards normal.  Rows of N >= 255 run at gamma = 0.9999, lambda = 1 (the tables stay above
0.71 at N = 3413: a dropped, duplicated or shifted step anywhere in the row moves the output by far more than the
bound), the others, and two long rows next to them, at the workload's 0.995 / 0.97.  Done patterns: random 10 %, none,
all, only t = 0, only t = N - 1, only t = 255 and 256 (the mask of Vm[t] comes from dones[t - 1], across the slice edge).

Poisoned surroundings.  Every input sits in a larger flat buffer that is NaN in front of and behind its logical extent;
every output is a flat buffer of the sentinel -7777 whose logical region is pre-filled with NaN.  After the call the
logical region is finite (or NaN exactly where the reference is) and every other element still holds the sentinel's
bytes, compared through an integer view.  The clamped over-reads at a slice end and the waves of b >= B are thereby
checked behaviour: a read of r[N] or d[-1] pulls in a NaN.
"""
import collections
import functools
import zlib

import numpy as np
import torch

SENTINEL = -7777.0
FRONT, TAIL = 3, 5                    # floats in front of / behind a logical extent (odd: nothing here needs alignment)
U = 2.0 ** -24
ATOL = RTOL = 1e-5                    # the project's bar for what is normalised in float32
C_ADV, C_RET = 4, 2
GAMMA_W, LAM_W = 0.995, 0.97          # the workload's
GAMMA_L, LAM_L = 0.9999, 1.0          # long rows: every term counts
MIN_STD = 1e-4

# error codes of include/surreal_amd.h
E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = -1, -2, -3, -5

# the host side of the two GAE entry points (smx_scan.hip), restated
GAE_LDS_OPT_IN = 48 * 1024            # above it the launch raises the kernel's dynamic-LDS limit first (both entry points)
GAE_LDS_CAP = {'gae': 160 * 1024, 'norm': 128 * 1024}

Case = collections.namedtuple('Case', 'id kind B N H gam dones why')


def gae_lds(N):
    return 16 * (3 * N + 1)


def path(c):
    """what a GAE case runs through: slice trips of the staging loop, the branch, the lane passes of the sliding-window
    loop, whether the LDS opt-in runs, the grid"""
    E = c.N - c.H + 1
    return dict(trips=c.N // 256 + 1, branch='one' if E == 1 else 'sliding', passes=-(-E // 64),
                optin=gae_lds(c.N) > GAE_LDS_OPT_IN, grid=-(-c.B // 4), lds=gae_lds(c.N),
                accepted=gae_lds(c.N) <= GAE_LDS_CAP[c.kind])


def gae_depth(N, H):
    return -(-N // 64) + 6 if H == N else H


def zupdate_chunks(rows):
    """smx_zfilter_update_ws_floats / zupdate_part_kernel: 0 chunks is the one-launch form"""
    return 0 if rows < 16384 else min(rows // 512, 256)


def zupdate_ws_floats(rows, D):
    return 2 * zupdate_chunks(rows) * D if D > 0 else 0


def zupdate_regime(rows):
    """'one' (one launch), 'even' (every chunk full), 'ragged' (the last chunk short), 'capped' (256 chunks)"""
    ch = zupdate_chunks(rows)
    if ch == 0:
        return 'one'
    if ch == 256 and rows // 512 > 256:
        return 'capped'
    per = -(-rows // ch)
    return 'even' if per * ch == rows else 'ragged'


def zupdate_depth(rows):
    ch = zupdate_chunks(rows)
    if ch == 0:
        return -(-rows // 16) + 16
    return -(-(-(-rows // ch)) // 32) + 16 + ch


def reward_grid(n):
    return min(-(-n // 1024), 64)


def sum_bound(d, c, S):
    """(d + c) 2^-24 S: see the module docstring"""
    return (d + c) * U * S


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
_PATTERNS = ('rand', 'none', 'all', 't0', 'last', 'edge')
_turn = [0]


def _dones_for(N):
    while True:
        p = _PATTERNS[_turn[0] % len(_PATTERNS)]
        _turn[0] += 1
        if p != 'edge' or N >= 257:
            return p


def _gae(kind, B, N, H, why, gam=None, dones=None):
    gam = gam or ('l' if N >= 255 else 'w')
    dones = dones or _dones_for(N)
    return Case('%s-B%d-N%d-H%d-%s-%s' % (kind, B, N, H, gam, dones), kind, B, N, H, gam, dones, why)


def _table():
    T = []
    # ---- smx_windowed_gae_returns_f32, one window per row: every slice-trip count, both sides of the opt-in and the last
    # N the entry point takes; every B mod 4 the set {1, 3, 4, 5, 9} has on both sides of N = 256
    for N, B, dn, why in ((1, 1, 'rand', 'one step'), (2, 3, 'none', 'two steps'), (63, 4, 'all', 'a lane short of a wave'),
                          (64, 5, 't0', 'one wave'), (65, 9, 'last', 'a second chain trip'),
                          (255, 3, 'rand', 'one slice trip, t = N in its last lane'),
                          (256, 4, 'none', 'a second slice trip for t = N alone'), (257, 5, 'all', 'two slice trips'),
                          (511, 3, 't0', 'two full slice trips'), (512, 9, 'last', 'a third trip for t = N alone'),
                          (513, 4, 'edge', 'three trips; the done at t = 255, 256 across the first slice edge'),
                          (1023, 1, 'rand', 'last N below the LDS opt-in'), (1024, 3, 'none', 'first N that opts in'),
                          (1365, 1, 'all', 'six trips, 64 KiB of LDS less 4 B'), (1366, 3, 't0', 'six trips, past 64 KiB'),
                          (3413, 5, 'last', 'fourteen trips, the last N accepted: 160 KiB')):
        T.append(_gae('gae', B, N, N, why, dones=dn))
    T.append(_gae('gae', 5, 257, 257, 'two slice trips at the workload discount', gam='w', dones='edge'))
    T.append(_gae('gae', 3, 1366, 1366, 'six trips at the workload discount', gam='w', dones='rand'))
    T.append(_gae('gae', 3, 300, 300, 'the tail value masked by the last done, long row', dones='last'))
    # ---- sliding windows: E in {64, 65, 66, 71, 300, 594}, both sides of a lane pass, B mod 4 = 2 on both sides of 256
    for N, H, B, why in ((64, 1, 3, 'E = 64: one full lane pass'), (65, 1, 2, 'E = 65: a second pass for one window'),
                         (127, 64, 5, 'E = 64, H = 64'), (128, 64, 4, 'E = 65, H = 64'), (129, 65, 1, 'E = 65, H = 65'),
                         (300, 1, 6, 'E = 300: five passes, two slice trips'), (600, 530, 3, 'E = 71, three slice trips'),
                         (600, 7, 5, 'E = 594: ten passes, ragged grid'), (1400, 1336, 2, 'E = 65 with the opt-in'),
                         (1400, 1335, 9, 'E = 66 with the opt-in, ragged grid')):
        T.append(_gae('gae', B, N, H, why))
    # ---- smx_windowed_gae_norm_f32
    for N, B, why in ((3, 3, 'three steps'), (257, 2, 'two slice trips'), (1023, 5, 'last N below the opt-in'),
                      (1024, 4, 'first N that opts in'), (2730, 3, 'the last N accepted: 128 KiB')):
        T.append(_gae('norm', B, N, N, why))
    T.append(_gae('norm', 1201, 19, 19, '301 workgroups, moments over 1201 values'))
    for B in (1, 2, 3, 4):
        T.append(_gae('norm', B, 5, 3 if B == 1 else 5, 'a one-workgroup grid: the last block is the only block'))
    T.append(_gae('norm', 6, 40, 8, 'sliding windows under the epilogue: n = B E = 198'))
    T.append(_gae('norm', 7, 12, 12, 'constant advantages: the min_std floor', dones='const'))
    T.append(_gae('norm', 1, 4, 4, 'B E = 1: 0 / 0 as in torch', dones='none'))
    # ---- moments, merge, normalise
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 127000):
        T.append(Case('mom-n%d' % n, 'mom', 1, n, 0, '', '', 'mean 1e4, spread 1e-2: a one-pass float32 variance loses it'))
    for k, zero in ((1, None), (2, None), (8, None), (8, 0), (8, 4), (8, 7), (2, 0)):
        T.append(Case('merge-k%d-z%s' % (k, zero), 'merge', k, 0, 0, '', zero, 'Chan merge, a zero-count part at %s' % zero))
    for n in (1, 2, 300, 2048 * 256 + 3):
        T.append(Case('advn-n%d' % n, 'advn', 1, n, 0, '', '', 'n = 1: NaN; past 2048 x 256 the grid cap binds'))
    # ---- z-filter: statistics + forward (B = rows, N = D, H = 1: ldx > D)
    for D in (1, 63, 64, 65, 129, 257, 376):
        for strided in (0, 1):
            T.append(Case('zfwd-D%d-s%d' % (D, strided), 'zfwd', 37, D, strided, '', '', 'stats, forward, forward_sums'))
    for rows in (1, 15, 16, 17, 31, 32, 33, 16383):
        T.append(Case('zupd-r%d-D65-s1' % rows, 'zupd', rows, 65, 1, '', 'ws', 'one-launch form'))
    T.append(Case('zupd-r33-D376-s0', 'zupd', 33, 376, 0, '', 'ws', 'one-launch form, six column blocks'))
    for rows in (16384, 16385, 16384 + 511, 33000, 131072, 131584):
        for D in (5, 65):
            T.append(Case('zupd-r%d-D%d-s%d' % (rows, D, int(rows < 33000)), 'zupd', rows, D, int(rows < 33000), '',
                          'ws', 'workspace form: %s' % zupdate_regime(rows)))
    # ---- reward filter
    for n in (1, 1023, 1024, 1025, 65535, 65536, 65537, 200001):
        T.append(Case('rf-n%d' % n, 'rf', 1, n, 0, '', '', 'grid %d' % reward_grid(n)))
    return T


CASES = _table()
BY_ID = {c.id: c for c in CASES}
GAE_CASES = [c for c in CASES if c.kind in ('gae', 'norm')]

# (entry point, what is wrong, the code it returns); test_gpu_scan.py builds the call from `what`
REFUSALS = (
    [('gae', 'N=3414', E_UNSUPPORTED), ('norm', 'N=2731', E_UNSUPPORTED)] +
    [(e, w, E_SHAPE) for e in ('gae', 'norm') for w in ('H=0', 'H>N', 'B=0')] +
    [('zfwd', 'rows=0', E_SHAPE), ('zfwd', 'ldx<D', E_SHAPE), ('zsums', 'rows=0', E_SHAPE), ('zsums', 'ldx<D', E_SHAPE),
     ('zupd', 'rows=0', E_SHAPE), ('zupd', 'ldx<D', E_SHAPE), ('zupd_ws', 'ldx<D', E_SHAPE)] +
    [('gae', 'null:' + p, E_NULL) for p in ('values', 'rewards', 'dones', 'gpow', 'lpow', 'adv', 'ret')] +
    [('norm', 'null:' + p, E_NULL) for p in ('values', 'rewards', 'dones', 'gpow', 'lpow', 'adv', 'ret', 'mom', 'ticket')] +
    [('rf', 'null:' + p, E_NULL) for p in ('rewards', 'out', 'partials', 'ticket', 'state')] +
    [('mom', 'null:' + p, E_NULL) for p in ('x', 'out')] + [('merge', 'null:' + p, E_NULL) for p in ('parts', 'out')] +
    [('advn', 'null:' + p, E_NULL) for p in ('x', 'mom')] +
    [('zstats', 'null:' + p, E_NULL) for p in ('rs', 'rsq', 'cnt', 'mean', 'std')] +
    [('zfwd', 'null:' + p, E_NULL) for p in ('x', 'mean', 'std', 'out')] +
    [('zsums', 'null:' + p, E_NULL) for p in ('x', 'rs', 'rsq', 'cnt', 'out')] +
    [('zupd', 'null:' + p, E_NULL) for p in ('x', 'rs', 'rsq', 'cnt')] +
    [('rf', 'partials+4', E_ALIGN)])


# ---------------------------------------------------------------------------------------------------------------------
# inputs and the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def _rng(cid):
    return np.random.RandomState(zlib.crc32(cid.encode()) & 0x7fffffff)


def f32(x):
    return np.asarray(x, dtype=np.float32)


def gae_inputs(c, salt=''):
    """float32 inputs of a GAE case: values [B, N + 1], rewards, dones [B, N], gpow, lpow [N], gamma, gamma_H (float32)"""
    g = _rng(c.id + salt)
    B, N, H = c.B, c.N, c.H
    gamma, lam = (GAMMA_L, LAM_L) if c.gam == 'l' else (GAMMA_W, LAM_W)
    values, rewards = f32(3.0 * g.randn(B, N + 1)), f32(g.randn(B, N))
    dones = np.zeros((B, N), np.float32)
    if c.dones == 'rand':
        dones = f32(g.rand(B, N) < 0.1)
    elif c.dones == 'all':
        dones[:] = 1.0
    elif c.dones == 't0':
        dones[:, 0] = 1.0
    elif c.dones == 'last':
        dones[:, N - 1] = 1.0
    elif c.dones == 'edge':
        dones[:, 255:257] = 1.0
    elif c.dones == 'const':               # every advantage the same number
        values[:] = 0.0
        rewards[:] = 0.75
    idx = np.arange(N, dtype=np.float32)
    gpow, lpow = np.power(np.float32(gamma), idx).astype(np.float32), np.power(np.float32(lam), idx).astype(np.float32)
    return dict(values=values, rewards=rewards, dones=dones, gpow=gpow, lpow=lpow, gamma=np.float32(gamma),
                gamma_H=np.float32(gamma ** H), H=H)


def _windows(x, H):
    return np.lib.stride_tricks.sliding_window_view(x, H, axis=1)          # [B, E, H]


def gae_reference(p):
    """-> dict adv, ret, S_adv, S_ret: float64 [B, E]"""
    d = np.float64
    v, r, dn = p['values'].astype(d), p['rewards'].astype(d), p['dones'].astype(d)
    g, l, gamma, gamma_H, H = p['gpow'].astype(d)[:p['H']], p['lpow'].astype(d)[:p['H']], d(p['gamma']), d(p['gamma_H']), p['H']
    vm = v.copy()
    vm[:, 1:] *= 1.0 - dn                                                  # ppo.py:387
    delta = r + gamma * vm[:, 1:] - vm[:, :-1]                             # ppo.py:390
    mag = np.abs(r) + gamma * np.abs(vm[:, 1:]) + np.abs(vm[:, :-1])
    boot = vm[:, H:]                                                       # v[s + H], s = 0 .. E - 1
    return dict(adv=_windows(delta, H) @ (g * l), S_adv=_windows(mag, H) @ (g * l),
                ret=_windows(r, H) @ g + boot * gamma_H, S_ret=_windows(np.abs(r), H) @ g + gamma_H * np.abs(boot))


def _chain32(terms, lanes):
    """float32, no FMA: `lanes` chains of stride `lanes` over the last axis, then (lanes == 64) the xor butterfly of
    smx_wave_sum or (otherwise) the lanes in order"""
    n = terms.shape[-1]
    trips = -(-n // lanes)
    pad = np.zeros(terms.shape[:-1] + (trips * lanes,), np.float32)
    pad[..., :n] = terms
    pad = pad.reshape(terms.shape[:-1] + (trips, lanes))
    acc = np.zeros(terms.shape[:-1] + (lanes,), np.float32)
    for t in range(trips):
        acc = acc + pad[..., t, :]
    if lanes == 64:
        ix = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[..., ix ^ off]
        return acc[..., 0]
    out = np.zeros(terms.shape[:-1], np.float32)
    for k in range(lanes):
        out = out + acc[..., k]
    return out


def gae_emulation(p):
    """the kernel's order in float32 numpy: -> adv, ret float32 [B, E]"""
    v, r, dn, H = p['values'], p['rewards'], p['dones'], p['H']
    g, l = p['gpow'][:H], p['lpow'][:H]
    vm = v.copy()
    vm[:, 1:] = vm[:, 1:] * (np.float32(1.0) - dn)
    delta = (r + p['gamma'] * vm[:, 1:]) - vm[:, :-1]
    N = r.shape[1]
    if H == N:
        adv = _chain32((delta * g) * l, 64)[:, None]
        ret = (_chain32(g * r, 64) + vm[:, N] * p['gamma_H'])[:, None]
        return adv, ret
    E = N - H + 1
    a, s = np.zeros((r.shape[0], E), np.float32), np.zeros((r.shape[0], E), np.float32)
    for k in range(H):
        s = s + g[k] * r[:, k:k + E]
        a = a + (delta[:, k:k + E] * g[k]) * l[k]
    return a, s + vm[:, H:] * p['gamma_H']


def moments64(x):
    x = np.asarray(x, np.float64).reshape(-1)
    m = x.sum() / x.size
    return np.array([x.size, m, ((x - m) ** 2).sum()])


def normalise64(x, mom, min_std):
    with np.errstate(all='ignore'):
        std = np.sqrt(np.float64(mom[2]) / (mom[0] - 1.0))
        den = min_std if min_std > std else std                            # Python max(std, 1e-4): NaN std stays
        return (np.asarray(x, np.float64) - mom[1]) / den


def merge64(parts):
    n = mean = m2 = 0.0
    for nb, mb, qb in np.asarray(parts, np.float64).reshape(-1, 3):
        if nb <= 0:
            continue
        nt, d = n + nb, mb - mean
        m2, mean, n = m2 + qb + d * d * n * nb / nt, mean + d * nb / nt, nt
    return np.array([n, mean, m2])


def zstats64(rs, rsq, cnt, eps):
    with np.errstate(all='ignore'):
        m = rs.astype(np.float64) / np.float64(cnt)
        s = np.sqrt(rsq.astype(np.float64) / np.float64(cnt) - m * m)      # NaN for a negative variance
        return m, np.where(np.isnan(s), s, np.maximum(s, eps))             # a NaN is not floored


def clamp64(z):
    with np.errstate(all='ignore'):
        return np.where(np.isnan(z), z, np.minimum(np.maximum(z, -5.0), 5.0))      # a NaN is not clamped


# with mean 1 and standard deviation 0.5: exactly +5, the float32 below it, past it (clamped); the same at -5.  Every
# one of x - 1 and (x - 1) / 0.5 is exact in float32 (the inner ones are two ulps of x from the edge: one would be a tie)
EDGE_X = (3.5, 3.5 - 2.0 ** -22, 3.5 + 2.0 ** -22, -1.5, -1.5 + 2.0 ** -22, -1.5 - 2.0 ** -22)
EDGE_Z = (5.0, 5.0 - 2.0 ** -21, 5.0, -5.0, -5.0 + 2.0 ** -21, -5.0)


class Problem(object):
    pass


@functools.lru_cache(maxsize=4)
def problem(c):
    """a GAE case's inputs, reference and bounds, accepted only if the float32 emulation is inside the bounds"""
    assert c.kind in ('gae', 'norm')
    P = Problem()
    P.case, P.inputs = c, gae_inputs(c)
    P.want = gae_reference(P.inputs)
    d = gae_depth(c.N, c.H)
    P.bound = dict(adv=sum_bound(d, C_ADV, P.want['S_adv']), ret=sum_bound(d, C_RET, P.want['S_ret']))
    a, r = gae_emulation(P.inputs)
    P.emu_share = {}
    for q, got in (('adv', a), ('ret', r)):
        diff = np.abs(got.astype(np.float64) - P.want[q])
        assert bool((diff <= P.bound[q]).all()), '%s: the float32 emulation leaves the bound on %s: a bad case' % (c.id, q)
        P.emu_share[q] = share(diff, P.bound[q])
    return P


def share(diff, bound):
    """largest |diff| / bound (0 / 0 = 0)"""
    diff, bound = np.broadcast_arrays(np.asarray(diff, np.float64), np.asarray(bound, np.float64))
    out = np.zeros(diff.shape)
    np.divide(diff, bound, out=out, where=bound > 0)
    out[(bound <= 0) & (diff > 0)] = np.inf
    return float(out.max()) if out.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# poisoned buffers
# ---------------------------------------------------------------------------------------------------------------------
class Bufs(object):
    """flat buffers on `device`: .buf[name], .span[name] = (off, n), .v[name] the logical view; .outputs the names that
    must keep their sentinel"""
    def __init__(self, device):
        self.device, self.buf, self.span, self.v, self.outputs, self.inputs = device, {}, {}, {}, [], []

    def inp(self, name, a, off=FRONT, dtype=torch.float32):
        t = torch.as_tensor(np.ascontiguousarray(a)).to(dtype)
        n = t.numel()
        b = torch.full((off + n + TAIL,), float('nan'), dtype=dtype)
        b[off:off + n] = t.reshape(-1)
        b = b.to(self.device)
        self.buf[name], self.span[name], self.v[name] = b, (off, n), b[off:off + n].view(t.shape)
        self.inputs.append(name)
        return self.v[name]

    def out(self, name, shape, off=FRONT, dtype=torch.float32, fill=float('nan')):
        n = int(np.prod(shape))
        b = torch.full((off + n + TAIL,), SENTINEL, dtype=dtype)
        b[off:off + n] = fill
        b = b.to(self.device)
        self.buf[name], self.span[name], self.v[name] = b, (off, n), b[off:off + n].view(shape)
        self.outputs.append(name)
        return self.v[name]

    def state(self, name, a, off=FRONT):
        """an in/out tensor (running sums, a filter state): its values inside, the sentinel around"""
        a = torch.as_tensor(np.ascontiguousarray(a)).float()
        v = self.out(name, tuple(a.shape), off)
        v.copy_(a.to(self.device))
        return v

    def get(self, name):
        return self.v[name].detach().cpu().numpy()


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def snapshot(x, names=None):
    return {k: bits(x.buf[k]).clone() for k in (names or x.outputs)}


def assert_untouched(x, snap):
    for k in sorted(snap):
        assert torch.equal(bits(x.buf[k]), snap[k]), '%s was written' % k


def check_fences(x, tag=''):
    for k in x.outputs:
        off, n = x.span[k]
        b = bits(x.buf[k])
        sent = bits(torch.tensor([SENTINEL], dtype=x.buf[k].dtype))[0]
        bad = int((b[:off] != sent).sum()) + int((b[off + n:] != sent).sum())
        assert bad == 0, '%s: %d elements outside the logical extent of %s were written' % (tag, bad, k)
    for k in x.inputs:
        off, n = x.span[k]
        b = x.buf[k].detach().cpu()
        assert bool(torch.isnan(b[:off]).all()) and bool(torch.isnan(b[off + n:]).all()), '%s: input %s' % (tag, k)


def ulps32(got, want, k=2):
    """|got - want| against k float32 ulps of want -> share"""
    want = np.asarray(want, np.float64)
    tol = k * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return share(np.abs(np.asarray(got, np.float64) - want), tol)


def bar_share(got, want):
    """the 1e-5 + 1e-5 |want| bar; NaN exactly where the reference is NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), 'NaN at %d places, the reference at %d' % (
        int(np.isnan(got).sum()), int(np.isnan(want).sum()))
    ok = ~np.isnan(want)
    assert bool(np.isfinite(got[ok]).all())
    return share(np.abs(got[ok] - want[ok]), ATOL + RTOL * np.abs(want[ok]))


def _judge(record, q, s, cid):
    record[q] = max(record.get(q, 0.0), s)
    assert s <= 1.0, '%s: %s uses %.3f of its bound' % (cid, q, s)


def _finite(a, cid, q):
    assert bool(np.isfinite(a).all()), '%s: %d elements of %s are not finite (never written?)' % (
        cid, int((~np.isfinite(a)).sum()), q)


# ---------------------------------------------------------------------------------------------------------------------
# one table entry
# ---------------------------------------------------------------------------------------------------------------------
def gae_bufs(c, p, device, split, rows=None):
    """the buffers of a GAE call on rows [b0, b1) of the case's inputs"""
    b0, b1 = rows or (0, c.B)
    x = Bufs(device)
    v = p['values'][b0:b1]
    if split:
        x.inp('values', v[:, :c.N], 5)
        x.inp('tail', v[:, c.N], 3)
    else:
        x.inp('values', v, 5)
    x.inp('rewards', p['rewards'][b0:b1], 3)
    x.inp('dones', p['dones'][b0:b1], 7)
    x.inp('gpow', p['gpow'], 3)
    x.inp('lpow', p['lpow'], 5)
    E = c.N - c.H + 1
    x.out('adv', ((b1 - b0) * E,), 3)
    x.out('ret', ((b1 - b0) * E,), 5)
    x.B = b1 - b0
    return x


def gae_call(kern, c, x, p, norm=False, ticket=None):
    v = x.v
    args = (v['values'].reshape(-1), v['rewards'], v['dones'], v['gpow'], v['lpow'], float(p['gamma']), float(p['gamma_H']),
            x.B, c.N, c.H, v['adv'], v['ret'])
    if norm:
        kern.gae_norm(*(args + (v['mom'], MIN_STD, ticket)), values_tail=v.get('tail'))
    else:
        kern.gae(*args, values_tail=v.get('tail'))


def _run_gae(kern, c, device, record):
    P = problem(c)
    p, E = P.inputs, c.N - c.H + 1
    keep = {}
    for split in (False, True):
        x = gae_bufs(c, p, device, split)
        gae_call(kern, c, x, p)
        for q in ('adv', 'ret'):
            got = x.get(q).reshape(c.B, E)
            _finite(got, c.id, q)
            _judge(record, q, share(np.abs(got.astype(np.float64) - P.want[q]), P.bound[q]), c.id)
        check_fences(x, c.id)
        keep[split] = {q: bits(x.v[q]).clone() for q in ('adv', 'ret')}
    for q in ('adv', 'ret'):
        assert torch.equal(keep[False][q], keep[True][q]), '%s: %s differs between the two value layouts' % (c.id, q)
    return keep[False]


def _run_norm(kern, c, device, record):
    plain = _run_gae(kern, c, device, record)                   # adv before normalisation, and ret: the `gae` launch
    P = problem(c)
    p, E = P.inputs, c.N - c.H + 1
    adv32 = plain['adv'].view(torch.float32).numpy()
    mom = moments64(adv32)
    want_norm = normalise64(adv32, mom, MIN_STD)
    if c.dones == 'const':
        assert mom[2] == 0.0 and bool((adv32 == adv32[0]).all()), c.id
    # the three separate launches: gae (above), moments, adv_normalize
    three = Bufs(device)
    three.state('adv', adv32, 5)
    three.out('mom', (3,), 3)
    kern.moments(three.v['adv'], three.v['mom'])
    kern.adv_normalize(three.v['adv'], three.v['mom'], MIN_STD)
    check_fences(three, c.id)
    ticket = torch.zeros(1, dtype=torch.int32, device=device)
    for split in (False, True):
        x = gae_bufs(c, p, device, split)
        x.out('mom', (3,), 5)
        gae_call(kern, c, x, p, norm=True, ticket=ticket)
        assert torch.equal(bits(x.v['mom']), bits(three.v['mom'])), '%s: moments differ from the moments launch' % c.id
        _judge(record, 'norm3', bar_share(x.get('adv'), three.get('adv')), c.id)
        assert int(ticket[0]) == 0, '%s: the ticket is %d after the launch' % (c.id, int(ticket[0]))
        assert torch.equal(bits(x.v['ret']), plain['ret']), '%s: ret differs from the gae launch' % c.id
        got_mom = x.get('mom')
        if c.B * E > 1:
            _finite(got_mom, c.id, 'mom')
        _judge(record, 'mom', ulps32(got_mom, mom), c.id)
        if c.dones == 'const':                                  # the floor: exactly (adv - mean) / min_std
            exact = (adv32 - np.float32(mom[1])) / np.float32(MIN_STD)
            assert np.array_equal(x.get('adv'), exact), '%s: not (adv - mean) / min_std' % c.id
        _judge(record, 'norm', bar_share(x.get('adv'), want_norm), c.id)
        check_fences(x, c.id)
    # the same ticket, other inputs
    c2 = c
    p2 = gae_inputs(c, salt='-second')
    w2 = gae_reference(p2)
    x = gae_bufs(c2, p2, device, True)
    x.out('mom', (3,), 5)
    gae_call(kern, c2, x, p2, norm=True, ticket=ticket)
    assert int(ticket[0]) == 0
    d = gae_depth(c.N, c.H)
    _judge(record, 'ret', share(np.abs(x.get('ret').reshape(c.B, E) - w2['ret']), sum_bound(d, C_RET, w2['S_ret'])), c.id)
    y = gae_bufs(c2, p2, device, True)
    gae_call(kern, c2, y, p2)
    a2 = y.get('adv')
    m2 = moments64(a2)
    _judge(record, 'mom', ulps32(x.get('mom'), m2), c.id)
    _judge(record, 'norm', bar_share(x.get('adv'), normalise64(a2, m2, MIN_STD)), c.id)
    check_fences(x, c.id)


def _run_mom(kern, c, device, record):
    g = _rng(c.id)
    data = f32(1e4 + 1e-2 * g.randn(c.N))
    x = Bufs(device)
    x.inp('x', data)
    x.out('mom', (3,), 5)
    kern.moments(x.v['x'], x.v['mom'])
    _finite(x.get('mom'), c.id, 'mom')
    _judge(record, 'mom', ulps32(x.get('mom'), moments64(data)), c.id)
    check_fences(x, c.id)


def _run_merge(kern, c, device, record):
    g = _rng(c.id)
    k, zero = c.B, c.dones
    sets = [f32(0.5 + g.randn(int(g.randint(40, 200)))) for _ in range(k)]
    parts = np.stack([f32(moments64(s)) for s in sets])
    if zero is not None:
        parts[zero] = (0.0, 123.0, 456.0)                       # a zero-count part's mean and M2 are not read
        sets[zero] = f32([])
    x = Bufs(device)
    x.inp('parts', parts.reshape(-1))
    x.out('mom', (3,), 5)
    kern.moments_merge(x.v['parts'], x.v['mom'])
    _finite(x.get('mom'), c.id, 'mom')
    _judge(record, 'mom', ulps32(x.get('mom'), merge64(parts)), c.id)
    # ... and that is the moments of the concatenation, to what the float32 parts can carry
    _judge(record, 'concat', bar_share(x.get('mom'), moments64(np.concatenate(sets))), c.id)
    check_fences(x, c.id)


def _run_advn(kern, c, device, record):
    g = _rng(c.id)
    data = f32(0.3 + 2.0 * g.randn(c.N))
    mom = f32(moments64(data))
    x = Bufs(device)
    x.inp('mom', mom)
    x.state('x', data, 5)
    kern.adv_normalize(x.v['x'], x.v['mom'], MIN_STD)
    want = normalise64(data, mom.astype(np.float64), MIN_STD)
    assert bool(np.isnan(want).all()) == (c.N == 1)
    _judge(record, 'norm', bar_share(x.get('x'), want), c.id)
    check_fences(x, c.id)


def _strided(x, name, a, strided):
    """a [rows, D] input, or (strided) the [:, 0, :] view of [rows, 2, D] whose other half is NaN"""
    if not strided:
        return x.inp(name, a)
    rows, D = a.shape
    full = np.full((rows, 2, D), np.nan, np.float32)
    full[:, 0, :] = a
    return x.inp(name, full)[:, 0, :]


def _run_zfwd(kern, c, device, record):
    g = _rng(c.id)
    rows, D, eps = c.B, c.N, 1e-5
    cnt = np.float32(1000.0)
    rs, rsq = f32(100.0 * g.randn(D)), f32(5000.0 * g.rand(D) + 300.0)
    floored, negative = (D // 2, D - 1) if D >= 3 else (None, None)
    if D >= 3:
        rs[floored], rsq[floored] = 0.0, 1e-9                   # variance 1e-12 < eps^2: floored to eps
        rs[negative], rsq[negative] = 1000.0, 0.0               # variance -1: NaN std, NaN output
    data = f32(3.0 * g.randn(rows, D) + 0.5)
    data[0, 0], data[1, 0], data[2, 0] = np.nan, np.inf, -np.inf
    m64, s64 = zstats64(rs, rsq, cnt, eps)
    x = Bufs(device)
    for k, a in (('rs', rs), ('rsq', rsq), ('cnt', [cnt])):
        x.inp(k, a)
    x.out('mean', (D,), 5)
    x.out('std', (D,), 3)
    kern.zfilter_stats(x.v['rs'], x.v['rsq'], x.v['cnt'], eps, x.v['mean'], x.v['std'])
    _judge(record, 'zmean', bar_share(x.get('mean'), m64), c.id)
    _judge(record, 'zstd', bar_share(x.get('std'), s64), c.id)
    if D >= 3:
        assert x.get('std')[floored] == np.float32(eps) and np.isnan(x.get('std')[negative]), c.id
    # forward with a mean / std of its own: column 1 (or 0) lands exactly on +-5, just inside and just outside
    mean, std = x.get('mean').copy(), x.get('std').copy()
    col = min(1, D - 1)
    mean[col], std[col] = 1.0, 0.5
    edge = f32(EDGE_X)
    data[3:9, col] = edge
    xv = _strided(x, 'x', data, c.H)
    x.inp('fmean', mean)
    x.inp('fstd', std)
    x.out('y', (rows, D), 5)
    kern.zfilter_forward(xv, x.v['fmean'], x.v['fstd'], x.v['y'])
    with np.errstate(all='ignore'):
        want = clamp64((data.astype(np.float64) - mean.astype(np.float64)) / std.astype(np.float64))
    y = x.get('y')
    _judge(record, 'zfwd', bar_share(y, want), c.id)
    assert np.array_equal(y[3:9, col], f32(EDGE_Z)), (c.id, y[3:9, col])
    assert np.isnan(y[0, 0]) and y[1, 0] == 5.0 and y[2, 0] == -5.0, c.id       # NaN stays NaN, +-inf clamps
    if D >= 3:
        assert bool(np.isnan(y[:, negative]).all()), c.id
    # forward_sums = stats, then forward: the same bits
    x.inp('smean', x.get('mean'))
    x.inp('sstd', x.get('std'))
    x.out('y2', (rows, D), 3)
    x.out('y3', (rows, D), 5)
    kern.zfilter_forward(xv, x.v['smean'], x.v['sstd'], x.v['y2'])
    kern.zfilter_forward_sums(xv, x.v['rs'], x.v['rsq'], x.v['cnt'], eps, x.v['y3'])
    assert torch.equal(bits(x.v['y2']), bits(x.v['y3'])), '%s: forward_sums differs from stats + forward' % c.id
    with np.errstate(all='ignore'):
        _judge(record, 'zsums', bar_share(x.get('y3'), clamp64((data.astype(np.float64) - m64) / s64)), c.id)
    check_fences(x, c.id)


def zupdate_emulation(data, rows):
    """the kernels' order in float32 numpy -> (column sums, column sums of squares) of this batch"""
    ch = zupdate_chunks(rows)
    out = []
    for t in (data, data * data):
        t = np.ascontiguousarray(t.T)                           # [D, rows]
        if ch == 0:
            out.append(_chain32(t, 16))
            continue
        per = -(-rows // ch)
        acc = np.zeros(t.shape[0], np.float32)
        for k in range(ch):
            acc = acc + _chain32(t[:, k * per:min((k + 1) * per, rows)], 32)
        out.append(acc)
    return out


def _run_zupd(kern, c, device, record, ws_lib=None):
    g = _rng(c.id)
    rows, D = c.B, c.N
    data = f32(2.0 * g.randn(rows, D) + 0.5)
    rs0, rsq0, cnt0 = f32(100.0 * g.randn(D)), f32(5000.0 * g.rand(D) + 300.0), np.float32(1000.0)
    d = zupdate_depth(rows)
    d64 = data.astype(np.float64)
    S1, S2 = np.abs(d64).sum(0), (d64 * d64).sum(0)
    want1, want2 = rs0 + d64.sum(0), rsq0 + S2
    b1, b2 = sum_bound(d, 0, S1) + U * np.abs(want1), sum_bound(d, 1, S2) + U * np.abs(want2)
    e1, e2 = zupdate_emulation(data, rows)
    assert bool((np.abs((rs0 + e1).astype(np.float64) - want1) <= b1).all()) and \
        bool((np.abs((rsq0 + e2).astype(np.float64) - want2) <= b2).all()), '%s: the emulation leaves the bound' % c.id
    need = zupdate_ws_floats(rows, D)
    if ws_lib is not None:
        assert ws_lib(rows, D) == need, (c.id, ws_lib(rows, D), need)
    kept = {}
    for mode in (('exact', 'short', 'none') if need else ('none', 'spare')):
        x = Bufs(device)
        xv = _strided(x, 'x', data, c.H)
        x.state('rs', rs0, 5)
        x.state('rsq', rsq0, 3)
        x.state('cnt', [cnt0], 5)
        ws = None
        if mode in ('exact', 'short', 'spare'):
            ws = x.out('ws', (need if mode == 'exact' else need - 1 if mode == 'short' else 64,), 5)
        kern.zfilter_update(xv, x.v['rs'], x.v['rsq'], x.v['cnt'], float(rows), ws=ws)
        if mode == 'exact':
            got1, got2 = x.get('rs'), x.get('rsq')
            _finite(got1, c.id, 'rs'), _finite(got2, c.id, 'rsq')
            _judge(record, 'zsum', share(np.abs(got1.astype(np.float64) - want1), b1), c.id)
            _judge(record, 'zsumsq', share(np.abs(got2.astype(np.float64) - want2), b2), c.id)
        elif mode == 'none':
            d1 = -(-rows // 16) + 16
            _judge(record, 'zsum', share(np.abs(x.get('rs').astype(np.float64) - want1),
                                         sum_bound(d1, 0, S1) + U * np.abs(want1)), c.id)
            _judge(record, 'zsumsq', share(np.abs(x.get('rsq').astype(np.float64) - want2),
                                           sum_bound(d1, 1, S2) + U * np.abs(want2)), c.id)
        assert x.get('cnt')[0] == np.float32(cnt0 + np.float32(rows)), '%s: count is %r' % (c.id, x.get('cnt')[0])
        if mode in ('short', 'spare'):                          # a workspace that is not used is not written
            assert bool((bits(ws) == bits(torch.tensor([float('nan')]))[0]).all()), c.id
        kept[mode] = (bits(x.v['rs']).clone(), bits(x.v['rsq']).clone())
        check_fences(x, c.id)
    for mode in kept:                                           # too small a workspace, or none: the one-launch bits
        if mode not in ('exact', 'none'):
            assert torch.equal(kept[mode][0], kept['none'][0]) and torch.equal(kept[mode][1], kept['none'][1]), (c.id, mode)


# count, sum, sumsq: mean 1, standard deviation 0.5, exactly.  The batches are 2 x normal, x = r / 2 has mean 0: the
# variance of the following states, sum x^2 of one batch over the count of all, stays well away from zero
RF_STATE0 = (4.0, 4.0, 5.0)
RF_SCALE, RF_EPS = 0.5, 1e-5


def reward_reference(r, scale, state, eps, use_filter=True):
    """-> (out, sums, state after) in float64 from the float32 x = r * scale the kernel forms"""
    xs = (r * np.float32(scale)).astype(np.float64)
    with np.errstate(all='ignore'):
        mean = np.float64(state[1]) / np.float64(state[0])
        q = np.float64(state[2]) / np.float64(state[0])
        # (running_sumsq holds the LAST batch alone: q - mean^2 may well be negative.  Near zero the float32 result is
        # anything: such a state makes a bad case, not a loose tolerance)
        assert abs(q - mean * mean) > 1e-2 * (q + mean * mean), 'an ill-conditioned filter state: a bad case'
        sd = np.sqrt(q - mean * mean)
        sd = sd if np.isnan(sd) else max(sd, eps)
        out = clamp64((xs - mean) / sd) if use_filter else xs
    sums = np.array([xs.size, xs.sum(), (xs * xs).sum()])
    return out, sums, np.array([state[0] + sums[0], state[1] + sums[1], sums[2]])


def _rf_bufs(device, r, state, nparts, in_place=False):
    x = Bufs(device)
    if in_place:
        x.state('r', r)
        x.v['out'] = x.v['r']
    else:
        x.inp('r', r)
        x.out('out', (r.size,), 5)
    x.state('state', state, 5)
    x.out('sums', (3,), 3)
    x.out('partials', (nparts,), 2, dtype=torch.float64, fill=SENTINEL)
    x.ticket = torch.zeros(1, dtype=torch.int32, device=device)
    return x


def _rf_state_tol(old, add, new):
    """state += (float) t: two roundings, each within half an ulp of a number no larger than the largest of the three"""
    return 2 * np.spacing(np.maximum(np.maximum(np.abs(old), np.abs(add)), np.abs(new)).astype(np.float32)).astype(np.float64)


def _run_rf(kern, c, device, record):
    g = _rng(c.id)
    n = c.N
    nparts = kern.reward_filter_partials()
    state = f32(RF_STATE0)
    for batch in range(3):
        r = f32(2.0 * g.randn(n))
        if batch == 0 and n >= 1023:                            # x = 3.5 / -1.5 are exactly +-5; a ulp inside and outside
            r[:6] = f32(EDGE_X) / np.float32(RF_SCALE)
        want, sums, after = reward_reference(r, RF_SCALE, state, RF_EPS)
        x = _rf_bufs(device, r, state, nparts, in_place=(batch == 1))
        kern.reward_filter(x.v['r'], RF_SCALE, x.v['state'], RF_EPS, x.v['out'], x.v['partials'], x.ticket, sums=x.v['sums'])
        assert int(x.ticket[0]) == 0, c.id
        _judge(record, 'rf_out', bar_share(x.get('out'), want), c.id)
        if batch == 0 and n >= 1023:
            assert np.array_equal(x.get('out')[:6], f32(EDGE_Z)), c.id
        _judge(record, 'rf_sums', ulps32(x.get('sums'), sums), c.id)
        got_state = x.get('state').copy()
        _judge(record, 'rf_state', share(np.abs(got_state.astype(np.float64) - after),
                                         _rf_state_tol(state.astype(np.float64), sums, after)), c.id)
        grid = reward_grid(n)
        pb = bits(x.v['partials'])
        sent = bits(torch.tensor([SENTINEL], dtype=torch.float64))[0]
        assert bool((pb[2 * grid:] == sent).all()), '%s: partials past 2 x %d were written' % (c.id, grid)
        check_fences(x, c.id)
        state = got_state
    # a state with a negative variance: NaN std kept, every output NaN, the state still takes the batch in
    bad = f32((4.0, 8.0, 4.0))
    r = f32(2.0 * g.randn(n))
    want, sums, after = reward_reference(r, RF_SCALE, bad, RF_EPS)
    assert bool(np.isnan(want).all())
    x = _rf_bufs(device, r, bad, nparts)
    kern.reward_filter(x.v['r'], RF_SCALE, x.v['state'], RF_EPS, x.v['out'], x.v['partials'], x.ticket, sums=x.v['sums'])
    _judge(record, 'rf_out', bar_share(x.get('out'), want), c.id)
    _judge(record, 'rf_state', share(np.abs(x.get('state').astype(np.float64) - after),
                                     _rf_state_tol(bad.astype(np.float64), sums, after)), c.id)
    check_fences(x, c.id)
    # sums only: the state's bytes stay
    x = _rf_bufs(device, r, f32(RF_STATE0), nparts)
    snap = snapshot(x, ['state'])
    kern.reward_filter(x.v['r'], RF_SCALE, x.v['state'], RF_EPS, x.v['out'], x.v['partials'], x.ticket, update=False,
                       sums=x.v['sums'])
    assert_untouched(x, snap)
    assert int(x.ticket[0]) == 0
    want, sums, _ = reward_reference(r, RF_SCALE, f32(RF_STATE0), RF_EPS)
    _judge(record, 'rf_out', bar_share(x.get('out'), want), c.id)
    _judge(record, 'rf_sums', ulps32(x.get('sums'), sums), c.id)
    check_fences(x, c.id)


_RUN = dict(gae=_run_gae, norm=_run_norm, mom=_run_mom, merge=_run_merge, advn=_run_advn, zfwd=_run_zfwd, zupd=_run_zupd,
            rf=_run_rf)


def run_entry(kern, c, device='cpu', **kw):
    """one table entry on `kern` -> record[quantity] = the largest share of its bound that was used"""
    record = {}
    _RUN[c.kind](kern, c, device, record, **kw)
    return record
