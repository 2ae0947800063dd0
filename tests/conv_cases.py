"""The implicit-GEMM convolution kernels of csrc/smx_conv.hip (smx_conv_u8_forward_f32, smx_conv_u8_wgrad_f32,
smx_conv_cl_forward_f32, smx_conv_cl_wgrad_f32, smx_conv_cl_dgrad_f32 and the two partial reduces) pinned down by
themselves: the case table, the poisoned buffers the cases run in, their float64 references and a pure-Python restatement
of the host dispatch.  Shared by test_conv_cpu.py (the table on the torch-CPU double, the coverage conditions, eight
deliberately wrong doubles) and test_gpu_conv.py (the same table on the HIP kernels).

Exact inputs.  Channel-last sources hold integers in {1, 2, 3}, weights and dy integers from {+-1, +-2, +-3} (dy with a
share of exact zeros, a ReLU mask's), biases integers in [-3, 3], relu_of values from {-2, -0.0, 0.0, 2}; the uint8 frames
hold bytes from {0, 255}, so a patch is exactly {0, 1}.  Every product and partial sum is an integer below 2**24: the
float32 result is exact in ANY summation order, the comparison is torch.equal.  build() asserts |want|.max() < 2**24 for
every case, weight-gradient sums over all rows included.

References are float64 conv2d / conv_transpose2d / torch.nn.grad.conv2d_weight on the logical tensors: exact for these
integers, and no code shared with the unfold-based CPU double.

x / 255 bit for bit ('select' cases).  Forward: one one-hot weight row per output channel and bias 0 over frames of random
bytes, so an output IS one byte / 255 after its trip through the MFMA; the patches are disjoint there (stride 8) and the
selected taps are handed every byte value 0..255 (build() asserts that all 256 occur).  Weight gradient: dy holds a single
1.0 in a row of the ragged last group, that row's patch holds distinct bytes (at K = 256 a permutation of 0..255) among
overlapping patches, so dW[o, :] is that patch / 255.  The float64 reference holds one nonzero term per element there,
fl64(byte / 255), and its rounding to float32 is the correctly rounded quotient for every byte (test_conv_cpu.py checks
that against float32 division).

Poisoned surroundings.  Every fp32 operand sits inside a larger NaN-filled flat buffer (at an offset that keeps the
alignment the entry point asks for), uint8 frames inside a buffer of 255s (or, in the guard cases, of 0s under all-positive
weights / dy, so a stray byte of either kind changes a sum).  Every output is the NaN-pre-filled logical region of a
sentinel buffer: after the call the region equals the reference and everything else is still the sentinel.  The partial
workspace is NaN-filled to exactly *_ws_floats() with sentinels behind it.

Dispatch.  plan() restates the host side of the five entry points: the template instantiation, the grid, the number of
partials the reduce reads and the largest number of trips any wavefront makes through its persistent loop.  The kernel
choice is confirmed by a kernel trace (profiles/conv_paths_kernel_stats.csv), the weight gradients' grids by the number of
workspace floats that are no longer NaN after a call (test_gpu_conv.py); the forward and data-gradient grids, hence their
trip counts, rest on the restated rule blocks = min(ceil(tiles / 4), 2048).
"""
import collections
import zlib

import torch

SENTINEL = -7777.0
TAIL = 8                      # elements behind every buffer's logical region
NAN = float('nan')
# the float cases' tolerances (rtol = atol), those of the direct tests of the same kernels in tests/test_gpu_kernels.py
TOL = {'u8_fwd': 1e-5, 'cl_fwd': 1e-5, 'u8_wgrad': 2e-5, 'cl_wgrad': 2e-5, 'cl_dgrad': 2e-5}

# op: u8_fwd | u8_wgrad | cl_fwd | cl_wgrad | cl_dgrad;  values: int | float | select;  opt: db (weight gradients) /
# relu_of (data gradient) is passed;  fill: what surrounds the uint8 frames;  mis: an operand put one element off its
# required alignment (the envelope sweep only)
Case = collections.namedtuple('Case', 'id op F C H W k s cout values opt stop fill mis')
Plan = collections.namedtuple('Plan', 'kernel inst grid partials trips reduce')


def case(op, F, C, H, W, k, s, cout, values='int', opt=True, stop=None, fill=255, mis=None, tag=''):
    cid = '%s-F%dC%d-%dx%d-k%ds%d-o%d%s%s' % (op, F, C, H, W, k, s, cout, '' if values == 'int' else '-' + values, tag)
    return Case(cid, op, F, C, H, W, k, s, cout, values, opt, stop, fill, mis)


# ---------------------------------------------------------------------------------------------------------------------
# the host dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------
def geom(c):
    Ho, Wo = (c.H - c.k) // c.s + 1, (c.W - c.k) // c.s + 1
    return Ho, Wo, c.F * Ho * Wo


def _cdiv(a, b):
    return -(-a // b)


def is_cells(c):
    return c.op == 'cl_dgrad' and c.s == 2 and c.H % 2 == 0 and c.W % 2 == 0


def units(c):
    """what the persistent loop(s) of the case's kernel tile by 16: patch rows; cells; the pixels of each parity class"""
    if c.op != 'cl_dgrad':
        return [geom(c)[2]]
    if is_cells(c):
        return [c.F * (c.H // 2) * (c.W // 2)]
    out = []
    for cls in range(c.s * c.s):
        py, px = divmod(cls, c.s)
        ca, cb = (c.H - py + c.s - 1) // c.s, (c.W - px + c.s - 1) // c.s
        if ca > 0 and cb > 0:
            out.append(c.F * ca * cb)
    return out


def plan(c):
    rows = geom(c)[2]
    tiles = [_cdiv(u, 16) for u in units(c)]
    if c.op in ('u8_fwd', 'cl_fwd'):
        grid = min(_cdiv(tiles[0], 4), 2048)
        if c.op == 'u8_fwd':
            return Plan('conv_u8_fwd_kernel', (c.C * c.k * c.k // 16,), grid, None, _cdiv(tiles[0], 4 * grid), None)
        return Plan('conv_cl_fwd_kernel', (c.k * c.k, _cdiv(c.cout, 16)), grid, None, _cdiv(tiles[0], 4 * grid), None)
    if c.op in ('u8_wgrad', 'cl_wgrad'):
        cap = 512 if c.op == 'u8_wgrad' else 256
        grid = max(1, min(_cdiv(tiles[0], 32), cap))
        trips = _cdiv(tiles[0], 4 * grid)
        if c.op == 'u8_wgrad':          # one partial per workgroup
            return Plan('conv_u8_wgrad_kernel', (c.C * c.k * c.k // 16,), grid, grid, trips, 'conv_partial_reduce_kernel')
        return Plan('conv_cl_wgrad_kernel', (c.k * c.k, _cdiv(c.cout, 16)), grid, 4 * grid, trips,      # one per wavefront
                    'conv_cl_wgrad_reduce_kernel')
    host_tiles = (c.F * c.H * c.W // (c.s * c.s) + 15) >> 4
    grid = max(1, min(_cdiv(host_tiles, 4), 2048))
    inst = (_cdiv(c.cout, 16), c.cout % 4 == 0)
    kernel = 'conv_cl_dgrad_cells_kernel' if is_cells(c) else 'conv_cl_dgrad_kernel'
    return Plan(kernel, inst, grid, None, max(_cdiv(t, 4 * grid) for t in tiles), None)


def inst_name(kernel, inst):
    return '%s<%s>' % (kernel, ', '.join(str(v).lower() if isinstance(v, bool) else str(v) for v in inst))


def name_of(c):
    p = plan(c)
    return inst_name(p.kernel, p.inst)


ALL_INSTANTIATIONS = (
    [inst_name('conv_u8_fwd_kernel', (ng,)) for ng in (4, 8, 12, 16)] +
    [inst_name('conv_u8_wgrad_kernel', (ng,)) for ng in (4, 8, 12, 16)] +
    [inst_name('conv_cl_fwd_kernel', (np_, nt)) for np_ in (16, 9, 4) for nt in (1, 2)] +
    [inst_name('conv_cl_wgrad_kernel', (np_, nt)) for np_ in (16, 9, 4) for nt in (1, 2)] +
    [inst_name('conv_cl_dgrad_kernel', (nh, v)) for nh in (1, 2) for v in (True, False)] +
    [inst_name('conv_cl_dgrad_cells_kernel', (nh, v)) for nh in (1, 2) for v in (True, False)])
REDUCES = ('conv_partial_reduce_kernel', 'conv_cl_wgrad_reduce_kernel')
# what no direct test of tests/test_gpu_kernels.py launches
NEWLY_REACHED = ('conv_u8_wgrad_kernel<16>', 'conv_cl_fwd_kernel<9, 1>', 'conv_cl_fwd_kernel<4, 2>',
                 'conv_cl_wgrad_kernel<9, 1>', 'conv_cl_wgrad_kernel<4, 2>', 'conv_cl_dgrad_cells_kernel<1, true>',
                 'conv_cl_dgrad_cells_kernel<1, false>', 'conv_cl_dgrad_cells_kernel<2, false>',
                 'conv_cl_dgrad_kernel<2, false>')


def max_cout(c):
    """the largest cout the case's instantiation takes"""
    if c.op in ('u8_fwd', 'u8_wgrad'):
        return 16
    top = 16 * _cdiv(c.cout, 16)
    if c.op == 'cl_dgrad' and c.cout % 4:
        return top - 1
    return top


def shape_ok(c):
    """the shape-only conditions of K.conv_u8_supported / conv_cl_supported / conv_cl_dgrad_supported"""
    K = c.C * c.k * c.k
    if c.op in ('u8_fwd', 'u8_wgrad'):
        return c.cout <= 16 and c.k % 4 == 0 and c.W % 4 == 0 and c.s % 4 == 0 and K % 64 == 0 and K <= 256
    if c.op in ('cl_fwd', 'cl_wgrad'):
        return c.C == 16 and c.cout <= 32 and c.k in (2, 3, 4)
    return c.C == 16 and c.cout <= 32 and c.k == 2 * c.s


def c_accepts(c):
    """what the C entry point takes: the shape conditions and the alignments IT needs"""
    if not shape_ok(c):
        return False
    if c.op == 'u8_fwd':
        return c.mis not in ('frames', 'W')
    if c.op == 'u8_wgrad':
        return c.mis != 'frames'              # (no weight operand: the Python predicate's weight alignment is stricter)
    if c.op in ('cl_fwd', 'cl_wgrad'):
        return c.mis != 'src'
    return not (c.mis == 'dy' and c.cout % 4 == 0)      # (the scalar-load kernels take any dy: the predicate is stricter)


def unseen_pixels(c):
    return c.op == 'cl_dgrad' and ((c.H - c.k) % c.s != 0 or (c.W - c.k) % c.s != 0)


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
def _frames_past(per_frame, more_than):
    """the fewest frames that give more than `more_than` units with a ragged last tile"""
    F = more_than // per_frame + 1
    while (F * per_frame) % 16 == 0:
        F += 1
    return F


_U8_K8 = {4: 1, 8: 2, 12: 3, 16: 4}            # NG -> C at k = 8
_U8_K4 = {4: 4, 8: 8, 12: 12, 16: 16}          # NG -> C at k = 4
MULTI_TRIP = 2 * 8192 * 16                     # more units than this: some wavefront of a 2048-block grid makes three trips


def _table():
    T = []
    # ---- the uint8 first convolution: forward and weight gradient, NG = K / 16 in {4, 8, 12, 16}
    for n, ng in enumerate((4, 8, 12, 16)):
        for op in ('u8_fwd', 'u8_wgrad'):
            T.append(case(op, 3, _U8_K8[ng], 20, 24, 8, 4, 16, opt=(n % 2 == 0)))                   # 60 rows, cout = 16
            T.append(case(op, 7, _U8_K4[ng], 14, 16, 4, 4, 9, opt=(n % 2 == 1)))                    # 84 rows, (H - k) % s = 2
        T.append(case('u8_fwd', 3, _U8_K8[ng], 16, 24, 8, 8, 16, values='select'))                 # 18 disjoint patches
        T.append(case('u8_wgrad', 2, _U8_K8[ng], 16, 24, 8, 4, 16, values='select'))
        T.append(case('u8_wgrad', 3, _U8_K8[ng], 20, 24, 8, 4, 13, values='select', tag='-b'))
    for op in ('u8_fwd', 'u8_wgrad'):
        T.append(case(op, 5, 2, 8, 8, 8, 4, 16, tag='-1x1'))                                        # Ho = Wo = 1
        T.append(case(op, 1, 4, 12, 12, 4, 4, 5, tag='-f1'))                                        # F = 1, 9 rows: 3 idle waves
        T.append(case(op, 3, 3, 20, 24, 8, 4, 11, fill=0, tag='-guard0'))
        T.append(case(op, 5, 3, 84, 84, 8, 4, 16, tag='-blocks'))                                   # 2000 rows
        T.append(case(op, 3, 2, 20, 24, 8, 4, 16, values='float'))
        for flag in (0, 1):
            T.append(case(op, 3, 2, 20, 24, 8, 4, 12, stop=flag, tag='-stop%d' % flag))
    # weight-gradient grids: 3 partials (no multiple of 4), 17 (past 16, no multiple of 4), the capped 512
    T.append(case('u8_wgrad', 3, 1, 84, 84, 8, 4, 16, tag='-p3'))
    T.append(case('u8_wgrad', 21, 1, 84, 84, 8, 4, 7, opt=False, tag='-p17'))
    Fm = _frames_past(20 * 19, MULTI_TRIP)
    T.append(case('u8_wgrad', Fm, 1, 84, 80, 8, 4, 16, tag='-capped'))
    # the persistent loop's steady state: > 262144 rows, ragged, at the narrowest and the widest instantiation
    T.append(case('u8_fwd', Fm, 1, 84, 80, 8, 4, 9, tag='-trips'))
    T.append(case('u8_fwd', Fm, 4, 84, 80, 8, 4, 16, tag='-trips'))
    # ---- the channel-last second convolution: forward and weight gradient, (NP, NT) = (k * k, ceil(cout / 16))
    for n, (k, nt) in enumerate((k, nt) for k in (4, 3, 2) for nt in (1, 2)):
        for op in ('cl_fwd', 'cl_wgrad'):
            T.append(case(op, 3, 16, 9, 10, k, 1, 16 * nt, opt=(n % 2 == 0)))                       # the largest cout
            T.append(case(op, 5, 16, 11, 8, k, 2, (7, 20)[nt - 1], opt=(n % 2 == 1)))               # (H - k) % s != 0 at k = 4, 2
    for op in ('cl_fwd', 'cl_wgrad'):
        T.append(case(op, 5, 16, 4, 4, 4, 2, 32, tag='-1x1'))
        T.append(case(op, 1, 16, 5, 6, 3, 1, 9, tag='-f1'))                                         # F = 1, 12 rows
        T.append(case(op, 40, 16, 20, 20, 4, 2, 32, tag='-blocks'))                                 # 3240 rows
        T.append(case(op, 3, 16, 9, 11, 3, 1, 20, values='float'))
        for flag in (0, 1):
            T.append(case(op, 3, 16, 9, 10, 3, 1, 20, stop=flag, tag='-stop%d' % flag))
    T.append(case('cl_wgrad', 8, 16, 20, 20, 4, 2, 24, opt=False, tag='-p8'))                       # 648 rows: 2 blocks
    T.append(case('cl_wgrad', _frames_past(33 * 31, 255 * 32 * 16), 16, 34, 32, 2, 1, 20, tag='-capped'))
    T.append(case('cl_fwd', _frames_past(33 * 31, MULTI_TRIP), 16, 34, 32, 2, 1, 7, tag='-trips'))
    T.append(case('cl_fwd', _frames_past(33 * 31, MULTI_TRIP), 16, 36, 34, 4, 1, 32, tag='-trips'))
    # ---- the data gradient: the cells kernel (stride 2, even maps) and the parity-class kernel, (NH, cout % 4 == 0)
    for n, (big, small) in enumerate(((16, 12), (15, 7), (32, 20), (31, 18))):
        T.append(case('cl_dgrad', 3, 16, 10, 6, 4, 2, big, opt=(n % 2 == 0)))                       # 45 cells
        T.append(case('cl_dgrad', 5, 16, 6, 14, 4, 2, small, opt=(n % 2 == 1)))                     # 105 cells
        T.append(case('cl_dgrad', 3, 16, 7, 9, 4, 2, big, opt=(n % 2 == 1)))                        # classes of 60, 48, 45, 36
        T.append(case('cl_dgrad', 3, 16, 5, 7, 2, 1, small, opt=(n % 2 == 0)))                      # one class of 105
    T.append(case('cl_dgrad', 3, 16, 13, 9, 6, 3, 12, tag='-k6s3'))                                 # nine classes
    T.append(case('cl_dgrad', 3, 16, 14, 11, 6, 3, 30, opt=False, tag='-k6s3'))
    T.append(case('cl_dgrad', 5, 16, 4, 4, 4, 2, 32, tag='-1x1'))                                   # cells, Ho = Wo = 1
    T.append(case('cl_dgrad', 1, 16, 4, 6, 4, 2, 6, tag='-f1'))                                     # F = 1, 6 cells
    T.append(case('cl_dgrad', 1, 16, 5, 4, 4, 2, 16, tag='-f1'))                                    # F = 1, classes of 6, 6, 4, 4
    T.append(case('cl_dgrad', 40, 16, 20, 20, 4, 2, 32, tag='-blocks'))
    T.append(case('cl_dgrad', 5, 16, 20, 20, 4, 2, 32, values='float'))
    T.append(case('cl_dgrad', 3, 16, 13, 9, 6, 3, 12, values='float'))
    for flag in (0, 1):
        T.append(case('cl_dgrad', 3, 16, 10, 6, 4, 2, 20, stop=flag, tag='-stop%d' % flag))
        T.append(case('cl_dgrad', 3, 16, 7, 9, 4, 2, 20, stop=flag, tag='-stop%d' % flag))
    T.append(case('cl_dgrad', _frames_past(9, MULTI_TRIP), 16, 6, 6, 4, 2, 32, tag='-trips'))       # cells <2, true>
    T.append(case('cl_dgrad', _frames_past(9, MULTI_TRIP), 16, 6, 6, 4, 2, 7, tag='-trips'))        # cells <1, false>
    T.append(case('cl_dgrad', _frames_past(25, MULTI_TRIP), 16, 5, 5, 2, 1, 12, tag='-trips'))      # one class, <1, true>
    T.append(case('cl_dgrad', _frames_past(9, MULTI_TRIP), 16, 5, 5, 4, 2, 30, tag='-trips'))       # 9 / 6 / 6 / 4, <2, false>
    return T


CASES = _table()
BIG = frozenset(c.id for c in CASES if max(units(c)) > 100000)
SMALL = [c for c in CASES if c.id not in BIG]


def _envelope():
    """small shapes on both sides of every boundary of the three predicates"""
    E = []
    for op in ('u8_fwd', 'u8_wgrad'):
        for cout in (16, 17):
            E.append(case(op, 2, 1, 12, 12, 8, 4, cout, tag='-env'))
        for k in (2, 3, 4, 5, 8):                                   # K = 4 k^2 = 16, 36, 64, 100, 256
            E.append(case(op, 2, 4, 12, 12, k, 4, 8, tag='-env-k'))
        for C in (1, 2, 3, 4, 5):                                   # K = 64 .. 320 at k = 8
            E.append(case(op, 2, C, 12, 12, 8, 4, 8, tag='-env-K'))
        for C in (5, 12, 16, 20):                                   # K = 80, 192, 256, 320 at k = 4
            E.append(case(op, 2, C, 12, 12, 4, 4, 8, tag='-env-K'))
        for W in (12, 13, 14, 15):
            E.append(case(op, 2, 1, 12, W, 8, 4, 8, tag='-env-W'))
        for s in (2, 4, 8):
            E.append(case(op, 2, 1, 16, 16, 8, s, 8, tag='-env-s'))
        E.append(case(op, 2, 1, 12, 12, 8, 4, 8, mis='frames', tag='-env-misframes'))
        E.append(case(op, 2, 1, 12, 12, 8, 4, 8, mis='W', tag='-env-misW'))
    for op in ('cl_fwd', 'cl_wgrad'):
        for cout in (16, 17, 32, 33):
            E.append(case(op, 2, 16, 6, 7, 3, 1, cout, tag='-env'))
        for k in (1, 2, 3, 4, 5):
            E.append(case(op, 2, 16, 6, 7, k, 1, 8, tag='-env-k'))
        for C in (15, 16, 17):
            E.append(case(op, 2, C, 6, 7, 2, 1, 8, tag='-env-C'))
        E.append(case(op, 2, 16, 6, 7, 2, 1, 8, mis='src', tag='-env-missrc'))
    for cout in (16, 17, 32, 33):
        E.append(case('cl_dgrad', 2, 16, 6, 8, 4, 2, cout, tag='-env'))
    for k, s in ((2, 1), (3, 1), (4, 2), (4, 1), (5, 2), (6, 3), (8, 4), (2, 2), (3, 2)):
        E.append(case('cl_dgrad', 2, 16, 9, 8, k, s, 8, tag='-env-ks'))
    for C in (15, 16, 17):
        E.append(case('cl_dgrad', 2, C, 6, 8, 4, 2, 8, tag='-env-C'))
    E.append(case('cl_dgrad', 2, 16, 6, 8, 4, 2, 8, mis='dy', tag='-env-misdy'))        # cout % 4 == 0: refused
    E.append(case('cl_dgrad', 2, 16, 6, 8, 4, 2, 7, mis='dy', tag='-env-misdy'))        # scalar loads: taken
    E.append(case('cl_dgrad', 2, 16, 7, 8, 4, 2, 7, mis='dy', tag='-env-misdy'))
    return E


ENVELOPE = _envelope()
# weight gradients refused for a workspace one float short (test_gpu_conv.py): nothing is launched
WORKSPACE_REFUSALS = [case('u8_wgrad', 3, 2, 20, 24, 8, 4, 12, tag='-ws-short'),
                      case('cl_wgrad', 3, 16, 9, 10, 3, 1, 20, tag='-ws-short')]
# stems whose first convolution takes the materialised route (F, C, H, W, feat), each run with and without the implicit
# weight gradients: the second layer still goes through conv_cl_fwd<16, 2>, the cells data gradient and, with the
# workspace, conv_cl_wgrad<16, 2>
STEM_FALLBACK = [(3, 5, 20, 20, 8), (3, 3, 20, 22, 8)]


def predicted_launches():
    """kernel launches, per instantiation, of one pass of test_gpu_conv.py: one library call per table entry (a stopped
    one still launches), the accepted envelope cases, nothing for a refusal, and the stem cases' second layer"""
    n = collections.Counter()
    for c in CASES + [e for e in ENVELOPE if c_accepts(e)]:
        p = plan(c)
        n[inst_name(p.kernel, p.inst)] += 1
        if p.reduce:
            n[p.reduce] += 1
    for (F, C, H, W, feat) in STEM_FALLBACK:
        H1, W1 = (H - 8) // 4 + 1, (W - 8) // 4 + 1
        assert H1 % 2 == 0 and W1 % 2 == 0
        for implicit_wgrad in (True, False):
            n['conv_cl_fwd_kernel<16, 2>'] += 1
            n['conv_cl_dgrad_cells_kernel<2, true>'] += 1
            if implicit_wgrad:
                n['conv_cl_wgrad_kernel<16, 2>'] += 1
                n['conv_cl_wgrad_reduce_kernel'] += 1
    return dict(n)


# ---------------------------------------------------------------------------------------------------------------------
# buffers, references, checks
# ---------------------------------------------------------------------------------------------------------------------
def _gen(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


def _ints(g, shape, zeros=0.0, positive=False):
    """integers from {+-1, +-2, +-3} (all positive on request), a share of them replaced by exact zeros"""
    v = torch.randint(1, 4, shape, generator=g)
    if not positive:
        v = v * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    v = v.float()
    if zeros:
        v[torch.rand(shape, generator=g) < zeros] = 0.0
    return v


def place(t, off, fill=NAN):
    """logical tensor -> a flat buffer of `fill` with the tensor's elements at [off, off + numel)"""
    n = t.numel()
    buf = torch.full((off + n + TAIL,), fill, dtype=t.dtype)
    buf[off:off + n] = t.reshape(-1)
    return buf


def out_buffer(n, off):
    buf = torch.full((off + n + TAIL,), SENTINEL)
    buf[off:off + n] = NAN
    return buf


class Built(object):
    """one case's buffers (on `device`), its references and how to call a kernel object with it"""
    pass


def _nchw(t, F, H, W, C):
    return t.reshape(F, H, W, C).permute(0, 3, 1, 2).double()


def build(c, device='cpu'):
    g = _gen(c.id)
    Ho, Wo, rows = geom(c)
    K = c.C * c.k * c.k
    u8 = c.op.startswith('u8')
    exact = c.values != 'float'
    x = Built()
    x.case, x.exact, x.stopped = c, exact, bool(c.stop)
    x.ops, x.outs, x.want = {}, {}, {}

    def operand(name, t, off, fill=NAN):
        off += 1 if c.mis == name else 0
        x.ops[name] = (place(t, off, fill), off, tuple(t.shape))

    def output(name, shape, off, want):
        n = 1
        for d in shape:
            n *= d
        x.outs[name] = (out_buffer(n, off), off, tuple(shape))
        x.want[name] = want.reshape(shape)

    # ---- the source
    if u8:
        if c.values == 'int':
            frames = (torch.randint(0, 2, (c.F, c.C, c.H, c.W), generator=g) * 255).to(torch.uint8)
        else:
            frames = torch.randint(0, 256, (c.F, c.C, c.H, c.W), generator=g).to(torch.uint8)
        xs = None
    elif c.op != 'cl_dgrad':
        if exact:
            src = torch.randint(1, 4, (c.F, c.H * c.W, c.C), generator=g).float()
        else:
            src = torch.relu(torch.randn(c.F, c.H * c.W, c.C, generator=g))
        xs = _nchw(src, c.F, c.H, c.W, c.C)
    # ---- weights, bias, dy
    fwd = c.op in ('u8_fwd', 'cl_fwd')
    if fwd or c.op == 'cl_dgrad':
        if c.values == 'int':
            Wt = _ints(g, (c.cout, c.C, c.k, c.k), positive=(c.fill == 0))
            b = torch.randint(-3, 4, (c.cout,), generator=g).float()
        elif c.values == 'select':
            # channel o selects tap taps[o]; the patches are disjoint (s >= k), and output n = row * cout + o is handed
            # the byte 97 n mod 256: every byte value occurs once rows * cout >= 256
            assert c.op == 'u8_fwd' and c.s >= c.k and rows * c.cout >= 256
            taps = torch.randperm(K, generator=g)[:c.cout]
            Wt = torch.zeros(c.cout, K)
            Wt[torch.arange(c.cout), taps] = 1.0
            for r in range(rows):
                f, p = divmod(r, Ho * Wo)
                oy, ox = divmod(p, Wo)
                for o in range(c.cout):
                    ch, ij = divmod(int(taps[o]), c.k * c.k)
                    frames[f, ch, oy * c.s + ij // c.k, ox * c.s + ij % c.k] = ((r * c.cout + o) * 97) % 256
            Wt = Wt.reshape(c.cout, c.C, c.k, c.k)
            b = torch.zeros(c.cout)
        else:
            Wt = torch.randn(c.cout, c.C, c.k, c.k, generator=g) / K ** 0.5
            b = torch.randn(c.cout, generator=g) * 0.1
    if not fwd:
        if c.values == 'int':
            dy = _ints(g, (rows, c.cout), zeros=0.3, positive=(c.fill == 0))
        elif c.values == 'select':
            assert c.op == 'u8_wgrad' and K <= 256
            r, o = rows - 2, int(torch.randint(0, c.cout, (1,), generator=g))      # (a row of the last, ragged group)
            dy = torch.zeros(rows, c.cout)
            dy[r, o] = 1.0
            f, p = divmod(r, Ho * Wo)
            oy, ox = divmod(p, Wo)
            patch = torch.randperm(256, generator=g)[:K].to(torch.uint8).reshape(c.C, c.k, c.k)
            frames[f, :, oy * c.s:oy * c.s + c.k, ox * c.s:ox * c.s + c.k] = patch
            x.patch, x.sel = patch.reshape(-1), (r, o)
        elif c.op == 'cl_dgrad':
            dy = torch.randn(rows, c.cout, generator=g)
        else:
            dy = torch.randn(rows, c.cout, generator=g) / rows ** 0.5
            dy[torch.rand(rows, c.cout, generator=g) < 0.4] = 0.0
        dyl = dy.reshape(c.F, Ho, Wo, c.cout).permute(0, 3, 1, 2).double()
    if u8:
        xs = frames.double() / 255
        operand('frames', frames, 12, fill=c.fill)          # 4-byte aligned, not 16
    # ---- per entry point: the remaining operands, the outputs and their float64 references
    if fwd:
        if u8:
            operand('W', Wt, 4)
        else:
            operand('src', src, 8)
            operand('W', Wt, 3)
        operand('bias', b, 1)
        want = torch.relu(torch.nn.functional.conv2d(xs, Wt.double(), b.double(), stride=c.s))
        output('y', (rows, c.cout), 3, want.permute(0, 2, 3, 1))
        if c.values == 'select':
            bytes_seen = torch.unique((x.want['y'] * 255).round())
            assert bytes_seen.numel() == 256, '%s: only %d byte values at the selected taps' % (c.id, bytes_seen.numel())
    elif c.op in ('u8_wgrad', 'cl_wgrad'):
        if not u8:
            operand('src', src, 4)
        operand('dy', dy, 5)
        dW = torch.nn.grad.conv2d_weight(xs, (c.cout, c.C, c.k, c.k), dyl, stride=c.s)
        output('dW', (c.cout, K), 1, dW)
        if c.opt:
            output('db', (c.cout,), 2, dy.double().sum(0))
        if c.values == 'select':
            r, o = x.sel
            assert torch.equal(x.want['dW'][o], x.patch.double() / 255)
            assert int((x.want['dW'] != 0).sum()) == K - int((x.patch == 0).sum())
    else:
        operand('dy', dy, 4)
        operand('W', Wt, 5)
        relu_of = None
        if c.opt:
            if exact:
                relu_of = torch.tensor([-2.0, -0.0, 0.0, 2.0])[torch.randint(0, 4, (c.F * c.H * c.W, c.C), generator=g)]
            else:
                relu_of = torch.randn(c.F * c.H * c.W, c.C, generator=g)
            operand('relu_of', relu_of, 7)
        dx = torch.nn.functional.conv_transpose2d(dyl, Wt.double(), stride=c.s,
                                                  output_padding=((c.H - c.k) % c.s, (c.W - c.k) % c.s))
        assert dx.shape == (c.F, c.C, c.H, c.W)
        dx = dx.permute(0, 2, 3, 1).reshape(c.F * c.H * c.W, c.C)
        if relu_of is not None:
            dx = dx * (relu_of > 0).double()
        output('dx', (c.F * c.H * c.W, c.C), 5, dx)
    if exact:
        for name, w in x.want.items():
            assert float(w.abs().max()) < 2 ** 24, (c.id, name)
            if c.values == 'int':
                assert torch.equal(w, w.round()), (c.id, name)
            x.want[name] = w.float()
    x.stop = None if c.stop is None else torch.tensor([c.stop], dtype=torch.int32)
    if device != 'cpu':
        x.ops = {k: (v[0].to(device),) + v[1:] for k, v in x.ops.items()}
        x.outs = {k: (v[0].to(device),) + v[1:] for k, v in x.outs.items()}
        x.stop = None if x.stop is None else x.stop.to(device)
    for name, (buf, off, shape) in x.ops.items():
        assert buf.data_ptr() % 16 == 0             # what the offsets above assume of a buffer's base
    return x


def view(entry):
    """the logical tensor inside its buffer"""
    if entry is None:
        return None
    buf, off, shape = entry
    n = 1
    for d in shape:
        n *= d
    return buf[off:off + n].view(shape)


def workspace(kern, c, device='cpu', short=0):
    """NaN to exactly *_ws_floats() (less `short`), sentinels behind: -> (buffer, the floats handed over)"""
    if c.op == 'u8_wgrad':
        n = kern.conv_u8_wgrad_ws_floats(c.cout, c.C * c.k * c.k)
    elif c.op == 'cl_wgrad':
        n = kern.conv_cl_wgrad_ws_floats(c.cout, c.k)
    else:
        return None, 0
    n -= short
    buf = torch.full((n + TAIL,), SENTINEL, device=device)
    buf[:n] = NAN
    return buf, n


def predicate(kern, x):
    """the kernel object's conv_*_supported on the case's own operands"""
    c = x.case
    if c.op in ('u8_fwd', 'u8_wgrad'):
        W = view(x.ops.get('W'))
        if W is None and c.mis == 'W':              # (the weight gradient has no weight operand: a misaligned stand-in)
            W = torch.zeros(9, device=x.ops['frames'][0].device)[1:]
        return kern.conv_u8_supported(view(x.ops['frames']), c.C, c.H, c.W, c.k, c.s, c.cout, W)
    if c.op in ('cl_fwd', 'cl_wgrad'):
        return kern.conv_cl_supported(view(x.ops['src']), c.C, c.k, c.cout)
    return kern.conv_cl_dgrad_supported(view(x.ops['dy']), c.C, c.k, c.s, c.cout)


def run(kern, x, ws=None):
    c = x.case
    o, out = (lambda n: view(x.ops.get(n))), (lambda n: view(x.outs.get(n)))
    a = (c.F, c.C, c.H, c.W, c.k, c.s)
    if c.op == 'u8_fwd':
        kern.conv_u8_forward(o('frames'), *a, o('W'), o('bias'), c.cout, out('y'), stop=x.stop)
    elif c.op == 'u8_wgrad':
        kern.conv_u8_wgrad(o('frames'), *a, o('dy'), c.cout, out('dW'), out('db'), ws, stop=x.stop)
    elif c.op == 'cl_fwd':
        kern.conv_cl_forward(o('src'), *a, o('W'), o('bias'), c.cout, out('y'), stop=x.stop)
    elif c.op == 'cl_wgrad':
        kern.conv_cl_wgrad(o('src'), *a, o('dy'), c.cout, out('dW'), out('db'), ws, stop=x.stop)
    else:
        kern.conv_cl_dgrad(o('dy'), *a, o('W'), c.cout, o('relu_of'), out('dx'), stop=x.stop)


def check(x, untouched=False):
    """every output's logical region equals the reference (or, stopped / refused, is still NaN); everything else is
    still the sentinel"""
    cid = x.case.id
    for name, (buf, off, shape) in x.outs.items():
        flat = buf.detach().cpu()
        want = x.want[name]
        n = want.numel()
        got = flat[off:off + n].view(shape)
        if untouched or x.stopped:
            assert bool(torch.isnan(got).all()), '%s: %s was written by a call that must write nothing' % (cid, name)
        elif x.exact:
            bad = (got != want)                              # NaN != anything: an unwritten element counts
            assert not bool(bad.any()), '%s: %d of %d elements of %s differ from the exact reference, first at %s: got %s want %s' % (
                cid, int(bad.sum()), bad.numel(), name, tuple(bad.nonzero()[0].tolist()), got[bad][0].item(),
                want[bad][0].item())
        else:
            tol = TOL[x.case.op]
            assert torch.allclose(got.double(), want, rtol=tol, atol=tol), '%s: %s max |got - want| = %g' % (
                cid, name, (got.double() - want).abs().max().item())
        rest = torch.cat([flat[:off], flat[off + n:]])
        assert bool((rest == SENTINEL).all()), '%s: %d elements outside %s were written' % (
            cid, int((rest != SENTINEL).sum()), name)


def check_workspace(cid, buf, n):
    if buf is not None:
        assert bool((buf[n:].cpu() == SENTINEL).all()), '%s: written behind the workspace' % cid


def run_entry(kern, c, device='cpu'):
    """one table entry = one library call, then every check"""
    x = build(c, device)
    buf, n = workspace(kern, c, device)
    run(kern, x, ws=None if buf is None else buf[:n])
    check(x)
    check_workspace(c.id, buf, n)
    x.ws, x.ws_floats = buf, n
    return x


def partial_floats(c):
    """how many floats of the NaN-filled workspace a weight gradient writes: its grid's partials, each a padded dW plus a
    padded db -- idle wavefronts' zero partials included, nothing of the capped layout beyond the grid"""
    p = plan(c)
    K = c.C * c.k * c.k
    o = c.cout if c.op == 'u8_wgrad' else 16 * p.inst[1]
    return p.partials * (o * K + o)
