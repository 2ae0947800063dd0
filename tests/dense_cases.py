"""The generic dense layer (csrc/smx_gemm.hip: smx_linear_f32, smx_linear_multi_f32, smx_linear_wgrad_f32 and the split-K
wrapper) pinned down by itself: the case table, the poisoned buffers the cases run in, their exact references, and a
pure-Python restatement of the host dispatch.  Shared by test_dense_cpu.py (the table on the torch-CPU double, the
coverage conditions, seven deliberately wrong doubles) and test_gpu_dense.py (the same table on the HIP kernels).

Exact inputs.  Operand values come from {+-1, +-2, +-3} (no zeros: every k-term matters), biases from the integers in
[-3, 3], so every product and every partial sum is an integer below 2**24 and the float32 result is exact in ANY summation
order, on any kernel: the reference is an int64 matmul and the comparison is torch.equal.  build() asserts
|want|.max() < 2**24 for every case.  Tanh and one realistic case per kernel use randn inputs (B scaled by 1 / sqrt(K))
against a float64 reference at rtol = atol = 2e-5, the tolerance of the existing direct test of this operator.

Poisoned surroundings.  Every logical matrix sits inside a larger flat buffer: `off` floats in front, a leading stride of
extent + pad, a few floats behind, everything outside the logical extent NaN (operands, bias, mask).  C is a flat buffer
of the sentinel -7777 whose logical [M, N] region is pre-filled with NaN: after the call the logical region must equal the
reference (an unwritten tile shows as NaN) and every other element must still be the sentinel.

Dispatch.  expected_path() / launch_batch() / wgrad_plan() restate gemm_prob, tile_mode_of, tiles_take, choose_kernel /
plan_batch, split_k and pick_splits.  The kernel choice is confirmed by a kernel trace
(profiles/dense_paths_kernel_stats.csv); the operand-mode pair inside gemm32_kernel<false> and gemm_rows_kernel rests on
the restated gemm_prob rule.
"""
import collections
import zlib

import torch

SENTINEL = -7777.0
TAIL = 8                      # floats behind every matrix
RTOL = ATOL = 2e-5            # float cases: tests/test_gpu_kernels.py::test_linear_tile_kernel_* uses the same
NONE, RELU, TANH = 0, 1, 2

Lin = collections.namedtuple('Lin', 'id kernel am bm M N K a_kc a_off a_pad b_kc b_off b_pad c_off c_pad bias act mask '
                                    'stop values')
Wg = collections.namedtuple('Wg', 'id M N rows z_off z_pad x_off x_pad w_off w_pad db ws')
Batch = collections.namedtuple('Batch', 'id kernel jobs')       # jobs: Lin / Wg (a Wg job is kind 1, 'wgrad')


# ---------------------------------------------------------------------------------------------------------------------
# the host dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------
def ld_of(kc, rows, K, pad):
    return (K if kc else rows) + pad


def mode_of(kc, ld, K, off):
    """gemm_prob: 0 K-contiguous and fully aligned, 1 K-contiguous otherwise, 2 K-strided (buffers are 16-byte aligned,
    so the base is aligned when `off` is a multiple of 4 floats)"""
    if not kc:
        return 2
    return 0 if (ld % 4 == 0 and K % 4 == 0 and off % 4 == 0) else 1


def mode1_reasons(kc, ld, K, off):
    return frozenset(r for r, hit in (('K', K % 4), ('ld', ld % 4), ('off', off % 4)) if hit) if kc else frozenset()


Prob = collections.namedtuple('Prob', 'M N K a_kc lda a_off b_kc ldb b_off dbias splits k_chunk')


def prob_of(c):
    if isinstance(c, Wg):
        return Prob(c.M, c.N, c.rows, 0, c.M + c.z_pad, c.z_off, 0, c.N + c.x_pad, c.x_off, c.db, 1, c.rows)
    return Prob(c.M, c.N, c.K, c.a_kc, ld_of(c.a_kc, c.M, c.K, c.a_pad), c.a_off, c.b_kc,
                ld_of(c.b_kc, c.N, c.K, c.b_pad), c.b_off, False, 1, c.K)


def prob_modes(p):
    return mode_of(p.a_kc, p.lda, p.K, p.a_off), mode_of(p.b_kc, p.ldb, p.K, p.b_off)


def tile_mode_of(kc, ld, off, mode):
    if kc:
        return 0 if mode == 0 else None
    return 2 if (ld % 4 == 0 and off % 4 == 0) else None


def tiles_take(probs):
    """tiles_take: every problem tile-eligible with the same storage -> the instantiation's (AM, BM), else None"""
    first = None
    for p in probs:
        am, bm = prob_modes(p)
        a, b = tile_mode_of(p.a_kc, p.lda, p.a_off, am), tile_mode_of(p.b_kc, p.ldb, p.b_off, bm)
        if a is None or b is None:
            return None
        if p.N < 64 or (p.k_chunk if p.splits > 1 else p.K) < 32:
            return None
        if first is not None and (a, b) != first:
            return None
        first = (a, b)
    return first


def launch_batch(probs):
    """-> (kernel, grid); kernel in 'gemm32_co', 'gemm32', 'rows', ('tile', AM, BM)"""
    rows_variant = all(p.M >= 2048 and not p.dbias and p.splits == 1 for p in probs)
    t = tiles_take(probs)
    wide = all(p.K >= 2048 and p.M >= 48 for p in probs)
    wgs = sum(-(-p.M // 64) * -(-p.N // 64) * p.splits for p in probs)
    if t is not None and (rows_variant or (wide and wgs >= 512)):
        return ('tile',) + t, wgs
    if rows_variant:
        return 'rows', sum(-(-p.M // 128) * -(-p.N // 32) for p in probs)
    grid = sum(-(-p.M // 32) * -(-p.N // 32) * p.splits for p in probs)
    return ('gemm32_co' if all(prob_modes(p) == (0, 0) for p in probs) else 'gemm32'), grid


def kernel_name(k):
    return 'tile%d%d' % k[1:] if isinstance(k, tuple) else k


def expected_path(c):
    """a Lin case -> (kernel, a_mode, b_mode); a Batch -> (kernel, [(a_mode, b_mode) per problem]).  Inside the tile
    kernel a K-contiguous operand is its mode 0, a K-strided one its mode 2."""
    if isinstance(c, Batch):
        probs = [prob_of(j) for j in c.jobs]
        return kernel_name(launch_batch(probs)[0]), [prob_modes(p) for p in probs]
    p = prob_of(c)
    return (kernel_name(launch_batch([p])[0]),) + prob_modes(p)


def grid_of(c):
    return launch_batch([prob_of(j) for j in c.jobs] if isinstance(c, Batch) else [prob_of(c)])[1]


# smx_wgrad.hip: which dW shapes one workgroup's registers hold (smx_wgrad_rows_plan / _groups)
def _size_ok(T, parts, lo, hi):
    q, rem = divmod(T, parts)
    return q >= lo and q + (1 if rem else 0) <= hi


def wgrad_rows_plan(M, N):
    Tm, Tn = -(-M // 16), -(-N // 16)
    return any(_size_ok(Tm, a, 4, 7) and _size_ok(Tn, b, 3, 5) for a, b in ((2, 4), (4, 2), (8, 1), (1, 8)))


def wgrad_rows_groups(M, N):
    if wgrad_rows_plan(M, N):
        return 1
    for g in (2, 3, 4):
        w = (-(-N // g) + 15) & ~15
        last = N - (g - 1) * w
        if last > 0 and wgrad_rows_plan(M, w) and wgrad_rows_plan(M, last):
            return g
    return 0


WGRAD_ROWS_MIN = 32768


def pick_splits(M, N, rows):
    if rows >= WGRAD_ROWS_MIN and M % 4 == 0 and N % 4 == 0 and wgrad_rows_groups(M, N) > 0:
        return min(rows // 128, 256)
    tiles = -(-M // 32) * -(-N // 32)
    s = min(rows // 1024, -(-2048 // tiles), 256)
    return 1 if s < 2 else s


def split32_closed_form(M, N, rows):
    """the 32 x 32 branch of the split-K wrapper -> (chunks asked for, k_chunk, chunks left by the shrink loop)"""
    S = pick_splits(M, N, rows)
    k_chunk = (-(-rows // S) + 31) & ~31
    left = S
    while (left - 1) * k_chunk >= rows:
        left -= 1
    return S, k_chunk, left


def wgrad_plan(c):
    """a Wg case through K.linear_wgrad -> (kernels launched in order, chunks left)"""
    p = prob_of(c)
    S = pick_splits(c.M, c.N, c.rows) if c.ws else 1
    if S <= 1:
        return [kernel_name(launch_batch([p])[0])], 1
    _, k_chunk, left = split32_closed_form(c.M, c.N, c.rows)
    reduce = 'segmented_reduce' if (c.w_pad == 0 and left > 32) else 'splitk_reduce'
    eligible = (c.rows >= WGRAD_ROWS_MIN and c.M % 4 == 0 and c.N % 4 == 0 and p.lda % 4 == 0 and p.ldb % 4 == 0 and
                c.z_off % 4 == 0 and c.x_off % 4 == 0 and wgrad_rows_groups(c.M, c.N) > 0)
    if eligible:
        return ['wgrad_rows', reduce], left
    p = p._replace(dbias=True, splits=left, k_chunk=k_chunk)         # (the partial bias sums are always asked for)
    return [kernel_name(launch_batch([p])[0]), reduce], left


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
def _operand(mode, rows, K, how, i, tile=False):
    """-> (kc, off, pad) that gives an operand of `rows` x K the wanted mode; `how` picks the way into mode 1"""
    if mode == 0:
        assert K % 4 == 0
        return 1, (0, 4)[i % 2], (0, 4)[(i // 2) % 2]
    if mode == 1:
        if how == 'K' and K % 4 == 0:
            how = 'ld'
        if how == 'K':
            return 1, 0, (-K) % 4 + (0, 4)[i % 2]                       # ld % 4 == 0, aligned base: K % 4 alone
        if how == 'ld':
            return 1, 0, 1 if (K + 1) % 4 else 3                        # an odd pad
        return 1, 1, (-K) % 4                                           # a base offset of one float
    if tile:
        return 0, (0, 4)[i % 2], (-rows) % 4 + (0, 4)[(i // 2) % 2]     # ld % 4 == 0 and an aligned base
    return 0, (0, 1, 4)[i % 3], (0, 4, 1)[(i // 2) % 3]


_HOW = ('K', 'ld', 'off')
_EPI = [(b, a, m) for b in (False, True) for a in (NONE, RELU) for m in (False, True)]
_counter = collections.Counter()


def lin(kernel, am, bm, M, N, K, how_a=None, how_b=None, epi=None, stop=None, values='int', act=None, c_geom=None,
        a_geom=None, tag=''):
    tile = kernel.startswith('tile')
    fam = 'tile' if tile else kernel
    i = _counter[fam]
    _counter[fam] += 1
    a_kc, a_off, a_pad = a_geom or _operand(am, M, K, how_a or _HOW[i % 3], i, tile)
    b_kc, b_off, b_pad = _operand(bm, N, K, how_b or _HOW[(i + 1) % 3], i + 1, tile)
    bias, act_, mask = _EPI[i % 8] if epi is None else epi
    c_off, c_pad = c_geom or ((0, 3)[i % 2], (0, 5)[(i // 2) % 2])
    cid = '%s-%d%d-%dx%dx%d-%d%s' % (kernel, am, bm, M, N, K, i, tag)
    return Lin(cid, kernel, am, bm, M, N, K, a_kc, a_off, a_pad, b_kc, b_off, b_pad, c_off, c_pad, bias,
               act_ if act is None else act, mask, stop, values)


def _linear_table():
    T = []
    pairs = [(a, b) for a in range(3) for b in range(3)]
    # ---- gemm32_kernel<false>: the nine mainloop<AM, BM> (NW = 4: the ring turns every 12 super-blocks = 384 in K)
    Ms, Ns = (1, 31, 32, 33, 65), (1, 5, 32, 33, 70)
    sweep, sweep0 = (1, 3, 31, 32, 33, 127, 128, 129, 383, 384, 385, 417, 769), (4, 32, 36, 128, 132, 384, 388, 772)
    n = 0
    for (am, bm) in pairs:
        if (am, bm) == (0, 0):
            continue                                   # reached by batching only (BATCHES below)
        has0 = am == 0 or bm == 0
        full = (am, bm) in ((1, 2), (0, 2))
        ks = (sweep0 if has0 else sweep) if full else ((36, 132, 388) if has0 else (33, 129, 385))
        for K in ks:
            T.append(lin('gemm32', am, bm, Ms[n % 5], Ns[(n // 5 + n) % 5], K))
            n += 1
        T.append(lin('gemm32', am, bm, 33, 70, 36 if has0 else 33, tag='-ragged'))
    # ---- gemm32_kernel<true>: the coalesced LDS-staged loop (two super-blocks per trip, the ring turns every 8)
    for n, K in enumerate((4, 28, 32, 36, 124, 128, 132, 252, 256, 260, 508, 512, 516, 1028)):
        T.append(lin('gemm32_co', 0, 0, Ms[n % 5], Ns[(n // 5 + n) % 5], K))
    T.append(lin('gemm32_co', 0, 0, 33, 70, 36, tag='-ragged'))
    # ---- the permutation over the eight XCDs at tile counts 1, 2, 7, 8, 9, 15, 17, 63, 65
    for t, (M, N) in ((1, (32, 32)), (2, (64, 32)), (7, (224, 32)), (8, (256, 32)), (9, (96, 96)), (15, (160, 96)),
                      (17, (544, 32)), (63, (288, 224)), (65, (416, 160))):
        T.append(lin('gemm32_co', 0, 0, M, N, 36, tag='-xcd%d' % t))
        T.append(lin('gemm32', 1, 1, M - 1, N - 3, 33, tag='-xcd%d' % t))
    # ---- the callers' forms: lda = 1 with K = 1; C a column block in the middle of a wider matrix, the weight's base
    # offset by c1 floats (K.linear(s.dz2, 1, c['W2'][:, c1:], 0, None, s.dxcat[:, c1:], rows, A, c2, ldb=ld, ldc=ld))
    T.append(lin('gemm32', 1, 1, 33, 5, 1, a_geom=(1, 0, 0), tag='-lda1'))
    T.append(lin('gemm32', 1, 2, 65, 6, 48, how_a='ld', c_geom=(17, 17), tag='-colblock'))
    # ---- gemm_rows_kernel: the nine mainloop<AM, BM, 1> (NW = 1: the ring turns every 3 super-blocks = 96 in K)
    Ms, Ns = (2048, 2049, 2081, 2177), (1, 9, 33, 63)
    sweep, sweep0 = (1, 31, 32, 33, 95, 96, 97, 191, 193), (4, 28, 32, 36, 92, 96, 100, 196)
    n = 0
    for (am, bm) in pairs:
        has0 = am == 0 or bm == 0
        full = (am, bm) in ((1, 2), (0, 2))
        ks = (sweep0 if has0 else sweep) if full else ((36, 100, 196) if has0 else (33, 97, 193))
        for K in ks:
            T.append(lin('rows', am, bm, Ms[n % 4], Ns[(n // 4 + n) % 4], K))
            n += 1
        T.append(lin('rows', am, bm, 2081, 33, 36 if has0 else 33, tag='-ragged'))
    T.append(lin('rows', 0, 0, 2049, 65, 28, tag='-n65'))           # N >= 64 but K < 32: not the tile kernel's
    T.append(lin('rows', 1, 1, 2049, 65, 36, how_a='off', how_b='ld', tag='-n65'))
    T.append(lin('rows', 2, 2, 2049, 64, 36, a_geom=(0, 0, 1), tag='-oddld'))   # K-strided, ld % 4 != 0: not eligible
    # ---- gemm_tile_kernel<AM, BM, 1, 1>: one K block of look-ahead, a permutation of its own
    Ms, Ns = (2048, 2049, 2050, 2113), (64, 65, 127, 130)
    n = 0
    for (am, bm), ks in (((0, 0), (32, 36, 60, 64, 68, 100)), ((2, 2), (32, 36, 60, 64, 68, 100, 33, 63, 65)),
                         ((0, 2), (36, 68, 100)), ((2, 0), (36, 68, 100))):
        for K in ks:
            T.append(lin('tile%d%d' % (am, bm), am, bm, Ms[n % 4], Ns[(n // 4 + n) % 4], K))
            n += 1
        # M = 2050 is no multiple of 4: a K-strided A is fetched four rows at a time, the poison behind row M - 1 may
        # reach output rows >= M (never stored) and nothing else
        T.append(lin('tile%d%d' % (am, bm), am, bm, 2050, 65, 36, tag='-ragged'))
    # ---- (the epilogues, bias x ReLU x mask, cycle with the case index inside each kernel family: lin())
    # the stop flag once per kernel: 1 leaves the whole C buffer untouched, the NaN pre-fill included, 0 gives the reference
    for k, am, bm, M, N, K in (('gemm32', 1, 2, 33, 33, 33), ('gemm32_co', 0, 0, 33, 33, 36), ('rows', 2, 1, 2049, 33, 33),
                               ('tile02', 0, 2, 2049, 65, 36)):
        for flag in (0, 1):
            T.append(lin(k, am, bm, M, N, K, epi=(True, RELU, False), stop=flag, tag='-stop%d' % flag))
    # ---- float cases: tanh, and one plain case per kernel
    for k, am, bm, M, N, K in (('gemm32', 2, 1, 65, 70, 129), ('gemm32_co', 0, 0, 65, 70, 260), ('rows', 1, 0, 2081, 33, 100),
                               ('tile00', 0, 0, 2049, 65, 100), ('tile22', 2, 2, 2050, 130, 65)):
        T.append(lin(k, am, bm, M, N, K, epi=(True, TANH, False), values='float', tag='-tanh'))
        T.append(lin(k, am, bm, M, N, K, epi=(True, RELU, True), values='float', tag='-float'))
    return T


LINEAR_CASES = _linear_table()


def wg(M, N, rows, ws, pads=(3, 4, 5), offs=(0, 0, 0), db=True, tag=''):
    cid = 'wgrad-%dx%dx%d-%s%s' % (M, N, rows, 'ws' if ws else 'nows', tag)
    return Wg(cid, M, N, rows, offs[0], pads[0], offs[1], pads[1], offs[2], pads[2], db, ws)


def _wgrad_table():
    T = []
    Ms, Ns = (1, 33, 48), (1, 17, 70)
    for n, rows in enumerate((1, 33, 385, 2047, 2048, 2049, 4100)):
        for ws in (False, True):
            j = 2 * n + ws
            T.append(wg(Ms[j % 3], Ns[(j // 3 + j) % 3], rows, ws, pads=((3, 4, 5), (1, 2, 3), (4, 4, 0))[j % 3],
                        offs=((0, 0, 0), (1, 2, 3))[j % 2], db=(j % 4 != 3)))
    T.append(wg(48, 70, 4100, True, tag='-b'))
    # 34 chunks of 1056 rows asked for, the last one empty: the shrink loop leaves 33 > 32, so ldw == N takes
    # segmented_reduce_kernel and ldw == N + 3 splitk_reduce_kernel (M, N no multiples of 4: the 32 x 32 kernel)
    T.append(wg(6, 10, 34817, True, pads=(3, 4, 0), tag='-ldwN'))
    T.append(wg(6, 10, 34817, True, pads=(3, 4, 3), tag='-ldwN3'))
    T.append(wg(6, 10, 34817, True, pads=(3, 4, 0), db=False, tag='-nodb'))
    T.append(wg(8, 8, 34000, True, pads=(4, 4, 0), tag='-mult4'))
    # the register-resident kernel of smx_wgrad.hip: rows >= 32768, M, N, the strides and the bases multiples of 4, and a
    # dW that cuts into 4..7 x 3..5 tiles of 16 per wavefront (116 x 180: 2 x 4 wavefronts of 4 x 3 tiles)
    T.append(wg(116, 180, 32768, True, pads=(4, 4, 0), tag='-regs'))
    T.append(wg(116, 180, 32768, True, pads=(4, 8, 4), db=False, tag='-regs-nodb'))
    return T


WGRAD_CASES = _wgrad_table()


def _batches():
    B = []
    co = lambda M, N, K, **kw: lin('gemm32_co', 0, 0, M, N, K, **kw)
    # the (0, 0) cell of the general kernel: a (vec, vec) job batched with one that is not
    B.append(Batch('multi-2-vec+wgrad', 'gemm32', [co(33, 70, 36, tag='-b'), wg(33, 17, 385, False, tag='-b0')]))
    B.append(Batch('multi-2-vec+strided', 'gemm32', [co(65, 33, 132, tag='-b'), lin('gemm32', 1, 2, 31, 5, 132, tag='-b')]))
    B.append(Batch('multi-2-vec+odd', 'gemm32', [lin('gemm32', 2, 1, 1, 70, 388, tag='-b'), co(32, 32, 388, tag='-b')]))
    B.append(Batch('multi-1', 'gemm32', [lin('gemm32', 1, 1, 33, 33, 129, tag='-b')]))
    B.append(Batch('multi-1-wgrad', 'gemm32', [wg(48, 70, 2049, False, tag='-b1')]))
    B.append(Batch('multi-2-allvec', 'gemm32_co', [co(65, 33, 260, tag='-b'), co(31, 70, 36, tag='-b')]))
    # weight gradients only (kind 1), across the row counts; one of them without a bias gradient
    B.append(Batch('multi-4-wgrads', 'gemm32', [wg(1, 70, 1, False, tag='-b4'), wg(33, 17, 2047, False, offs=(1, 2, 3), tag='-b4'),
                                                 wg(48, 1, 2048, False, db=False, tag='-b4'),
                                                 wg(48, 70, 4100, False, pads=(0, 0, 0), tag='-b4')]))
    nine = []
    pairs = [(a, b) for a in range(3) for b in range(3)]
    for j, (am, bm) in enumerate(pairs[:6] + pairs[7:]):
        K = 36 + 32 * j
        if (am, bm) == (0, 0):
            nine.append(co(33, 70, K, tag='-b9'))
        else:
            nine.append(lin('gemm32', am, bm, (33, 65, 1)[j % 3], (70, 5, 33)[j % 3], K if (am == 0 or bm == 0) else K + 1,
                            tag='-b9'))
    nine.insert(2, wg(33, 17, 33, False, tag='-b9'))
    B.append(Batch('multi-9', 'gemm32', nine))
    # a stop flag on one job of a batch skips that job only
    B.append(Batch('multi-3-stop', 'gemm32', [lin('gemm32', 1, 2, 33, 33, 33, tag='-b'),
                                               lin('gemm32', 2, 2, 65, 5, 33, stop=1, tag='-bstop1'),
                                               lin('gemm32', 1, 0, 31, 70, 36, stop=0, tag='-bstop0')]))
    # a many-row job with a small one: everything goes to gemm32
    B.append(Batch('multi-2-big+small', 'gemm32', [lin('tile00', 0, 0, 2049, 65, 36, tag='-b'),
                                                    lin('gemm32', 1, 1, 33, 5, 33, tag='-b')]))
    # many-row jobs with differing storage: the rows kernel (its (0, 0) cell, ragged, at N >= 64 and K >= 32)
    B.append(Batch('multi-2-rows', 'rows', [lin('tile00', 0, 0, 2049, 65, 36, tag='-b2'),
                                             lin('tile02', 0, 2, 2081, 65, 36, tag='-b2')]))
    B.append(Batch('multi-3-rows-stop', 'rows', [lin('rows', 1, 2, 2049, 9, 33, tag='-b'),
                                                  lin('rows', 0, 0, 2177, 33, 36, stop=1, tag='-bstop1'),
                                                  lin('rows', 2, 1, 2048, 63, 97, tag='-b')]))
    # many-row jobs of one eligible storage: the tile kernel takes the batch
    B.append(Batch('multi-2-tile', 'tile20', [lin('tile20', 2, 0, 2050, 65, 36, tag='-b'),
                                               lin('tile20', 2, 0, 2113, 130, 68, stop=1, tag='-bstop1')]))
    return B


BATCHES = _batches()

# refused by smx_linear_multi_f32 before anything is launched (test_gpu_dense.py builds them)
REFUSALS = ('ten-jobs', 'kind-2', 'ldc-below-N', 'M-zero', 'wgrad-lda-below-M')


def cells_of(c):
    """the (kernel family, a_mode, b_mode, ragged) cells a table entry exercises"""
    out = []
    if isinstance(c, Batch):
        k, modes = expected_path(c)
        jobs = c.jobs
    else:
        k, a, b = expected_path(c)
        modes, jobs = [(a, b)], [c]
    T = 64 if k.startswith('tile') else 32
    for j, (a, b) in zip(jobs, modes):
        p = prob_of(j)
        if k.startswith('tile'):
            a, b = (0 if p.a_kc else 2), (0 if p.b_kc else 2)
        out.append((k[:4] if k.startswith('tile') else k, a, b, bool(p.M % T and p.N % T and p.K % 32)))
    return out


ALL_CELLS = ([('gemm32_co', 0, 0)] + [('gemm32', a, b) for a in range(3) for b in range(3)] +
             [('rows', a, b) for a in range(3) for b in range(3)] + [('tile', a, b) for a in (0, 2) for b in (0, 2)])


def predicted_launches():
    """kernel launches of one pass of test_gpu_dense.py over the table: one library call per entry; a refusal launches
    nothing, and each refusal test but 'ten-jobs' then runs its three jobs undamaged (one gemm32 launch)"""
    n = collections.Counter()
    n['gemm32'] += len(REFUSALS) - 1
    for c in LINEAR_CASES:
        n[expected_path(c)[0]] += 1
    for c in BATCHES:
        n[expected_path(c)[0]] += 1
    for c in WGRAD_CASES:
        for k in wgrad_plan(c)[0]:
            n[k] += 1
    return dict(n)


# ---------------------------------------------------------------------------------------------------------------------
# buffers, references, checks
# ---------------------------------------------------------------------------------------------------------------------
def _gen(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


def _ints(g, shape, lo=1, hi=3):
    """nonzero integers of magnitude lo..hi"""
    mag = torch.randint(lo, hi + 1, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).float()


def place(logical, kc, off, pad, fill=float('nan')):
    """logical [rows, K] -> (flat buffer, ld): K-contiguous rows (kc) or K-strided, NaN (or `fill`) everywhere else"""
    rows, K = logical.shape
    ld = ld_of(kc, rows, K, pad)
    outer = rows if kc else K
    buf = torch.full((off + outer * ld + TAIL,), fill)
    view = torch.as_strided(buf, (rows, K), (ld, 1) if kc else (1, ld), off)
    view.copy_(logical)
    return buf, ld


def out_buffer(rows, cols, off, pad):
    ld = cols + pad
    buf = torch.full((off + rows * ld + TAIL,), SENTINEL)
    torch.as_strided(buf, (rows, cols), (ld, 1), off).fill_(float('nan'))
    return buf, ld


class Built(object):
    """one problem's buffers (on `device`), its reference and how to call a kernel object with it"""
    pass


def build(c, device='cpu'):
    g = _gen(c.id)
    x = Built()
    x.case = c
    if isinstance(c, Wg):
        dz, xx = _ints(g, (c.rows, c.M)), _ints(g, (c.rows, c.N))
        x.A, x.lda = place(dz, 1, c.z_off, c.z_pad)
        x.B, x.ldb = place(xx, 1, c.x_off, c.x_pad)
        x.C, x.ldc = out_buffer(c.M, c.N, c.w_off, c.w_pad)
        x.c_off, x.rows_c, x.cols_c = c.w_off, c.M, c.N
        x.db = None
        if c.db:
            x.db = torch.full((2 + c.M + TAIL,), SENTINEL)
            x.db[2:2 + c.M] = float('nan')
        x.want = (dz.long().t() @ xx.long())
        x.want_db = dz.long().sum(0)
        assert int(x.want.abs().max()) < 2 ** 24 and int(x.want_db.abs().max()) < 2 ** 24
        x.want, x.want_db = x.want.float(), x.want_db.float()
        x.exact, x.stopped = True, False
    else:
        if c.values == 'int':
            a, b = _ints(g, (c.M, c.K)), _ints(g, (c.N, c.K))
            bias = torch.randint(-3, 4, (c.N,), generator=g).float() if c.bias else None
        else:
            a, b = torch.randn(c.M, c.K, generator=g), torch.randn(c.N, c.K, generator=g) / c.K ** 0.5
            bias = torch.randn(c.N, generator=g) if c.bias else None
        mask = torch.randint(-1, 2, (c.M, c.N), generator=g).float() * 2 if c.mask else None       # {-2, 0, 2}
        x.A, x.lda = place(a, c.a_kc, c.a_off, c.a_pad)
        x.B, x.ldb = place(b, c.b_kc, c.b_off, c.b_pad)
        x.C, x.ldc = out_buffer(c.M, c.N, c.c_off, c.c_pad)
        x.c_off, x.rows_c, x.cols_c = c.c_off, c.M, c.N
        x.bias = None
        if bias is not None:
            x.bias = torch.full((c.N + TAIL,), float('nan'))
            x.bias[:c.N] = bias
        x.mask, x.m_off = None, 0
        if mask is not None:                       # its own buffer and base, C's leading stride
            x.m_off = 1 + c.c_off
            x.mask = torch.full((x.m_off + c.M * x.ldc + TAIL,), float('nan'))
            torch.as_strided(x.mask, (c.M, c.N), (x.ldc, 1), x.m_off).copy_(mask)
        x.stop = None if c.stop is None else torch.tensor([c.stop], dtype=torch.int32)
        x.stopped = bool(c.stop)
        x.exact = c.values == 'int'
        if x.exact:
            w = a.long() @ b.long().t()
            if bias is not None:
                w = w + bias.long()
            if c.act == RELU:
                w = w.clamp(min=0)
            assert c.act != TANH
            if mask is not None:
                w = w * (mask > 0).long()
            assert int(w.abs().max()) < 2 ** 24
            x.want = w.float()
        else:
            w = a.double() @ b.double().t()
            if bias is not None:
                w = w + bias.double()
            w = torch.relu(w) if c.act == RELU else torch.tanh(w) if c.act == TANH else w
            if mask is not None:
                w = w * (mask > 0).double()
            x.want = w
    for name in ('A', 'B', 'C', 'db', 'bias', 'mask', 'stop'):
        t = getattr(x, name, None)
        if t is not None and device != 'cpu':
            setattr(x, name, t.to(device))
    for name in ('A', 'B', 'C'):
        assert getattr(x, name).data_ptr() % 16 == 0        # what mode_of() assumes of a buffer's base
    return x


def linear_args(x):
    """-> (args, kwargs) of K.linear for a built Lin problem"""
    c = x.case
    kw = dict(act=c.act, relu_mask=None if x.mask is None else x.mask[x.m_off:], lda=x.lda, ldb=x.ldb, ldc=x.ldc,
              stop=x.stop)
    return (x.A[c.a_off:], c.a_kc, x.B[c.b_off:], c.b_kc, x.bias, x.C[c.c_off:], c.M, c.N, c.K), kw


def wgrad_args(x):
    c = x.case
    db = None if x.db is None else x.db[2:]
    return (x.A[c.z_off:], x.B[c.x_off:], x.C[c.w_off:], db, c.M, c.N, c.rows), dict(ldz=x.lda, ldx=x.ldb, ldw=x.ldc)


def job_of(x):
    if isinstance(x.case, Wg):
        a, kw = wgrad_args(x)
        return ('wgrad',) + a + (kw,)
    a, kw = linear_args(x)
    return ('linear',) + a + (kw,)


def run(kern, x, ws=None):
    if isinstance(x.case, Wg):
        a, kw = wgrad_args(x)
        kern.linear_wgrad(*a, ws=ws, **kw)
    else:
        a, kw = linear_args(x)
        kern.linear(*a, **kw)


def check(x):
    """the logical region equals the reference (or, stopped, is still NaN); everything else is still the sentinel"""
    C = x.C.detach().cpu()
    got = torch.as_strided(C, (x.rows_c, x.cols_c), (x.ldc, 1), x.c_off)
    cid = x.case.id
    if x.stopped:
        assert bool(torch.isnan(got).all()), '%s: a stopped problem wrote its output' % cid
    elif x.exact:
        bad = (got != x.want)                                # NaN != anything: an unwritten element counts
        assert not bool(bad.any()), '%s: %d of %d elements differ from the exact reference, first at %s: got %s want %s' % (
            cid, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()), got[bad][0].item(), x.want[bad][0].item())
    else:
        assert torch.allclose(got.double(), x.want, rtol=RTOL, atol=ATOL), '%s: max |got - want| = %g' % (
            cid, (got.double() - x.want).abs().max().item())
    outside = torch.ones(C.numel(), dtype=torch.bool)
    torch.as_strided(outside, (x.rows_c, x.cols_c), (x.ldc, 1), x.c_off).fill_(False)
    assert bool((C[outside] == SENTINEL).all()), '%s: %d elements outside [M, N] of C were written' % (
        cid, int((C[outside] != SENTINEL).sum()))
    if isinstance(x.case, Wg) and x.db is not None:
        db = x.db.detach().cpu()
        if x.stopped:
            assert bool(torch.isnan(db[2:2 + x.case.M]).all()), '%s: a refused problem wrote its db' % cid
        else:
            assert torch.equal(db[2:2 + x.case.M], x.want_db), '%s: db differs from the exact column sums' % cid
        rest = torch.cat([db[:2], db[2 + x.case.M:]])
        assert bool((rest == SENTINEL).all()), '%s: db written outside its M entries' % cid


def run_entry(kern, c, device='cpu', ws_for=None):
    """one table entry = one library call, then every check.  ws_for(Wg case) -> workspace tensor or None"""
    if isinstance(c, Batch):
        xs = [build(j, device) for j in c.jobs]
        kern.linear_multi([job_of(x) for x in xs])
        for x in xs:
            check(x)
        return xs
    x = build(c, device)
    ws = ws_for(c) if (isinstance(c, Wg) and c.ws and ws_for is not None) else None
    run(kern, x, ws=ws)
    check(x)
    return [x]
