"""GPU tier (-m gpu): the implicit-GEMM convolution kernels of csrc/smx_conv.hip by themselves -- the uint8 first
convolution (forward, weight gradient), the 16-channel channel-last second convolution (forward, weight gradient, the
cells and the parity-class data gradient) and the two partial reduces -- over the case table of conv_cases.py: all 28
template instantiations, ragged last tiles, every persistent loop past its first trip, one-block to capped
weight-gradient grids, the optional arguments and the stop flags.

Integer-valued inputs make every float32 partial sum exact, so the comparison with the float64 reference is torch.equal at
any summation order; x / 255 is pinned bit for bit by one-hot selections; everything next to an operand is NaN (255 or 0
around the uint8 frames), everything around an output a sentinel, the workspace NaN (conv_cases.py says how).  One
library call per table entry: profiles/conv_paths_kernel_stats.csv, a kernel trace of this file alone, shows the launch
counts conv_cases.predicted_launches() gives."""
import pytest
import torch

import conv_cases as CC
import test_gpu_kernels as TK
from surreal_amd import _lib as L
from test_gpu_kernels import K  # noqa: F401  (the module-scoped kernels fixture)

pytestmark = pytest.mark.gpu


def ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize('c', CC.CASES, ids=ids(CC.CASES))
def test_conv_case(K, c):
    x = CC.run_entry(K, c, 'cuda')
    if x.ws is not None:                # the partials the restated grid says, and no others, were written
        written = int((~torch.isnan(x.ws[:x.ws_floats])).sum())
        assert written == (0 if x.stopped else CC.partial_floats(c)), c.id


@pytest.mark.parametrize('c', CC.ENVELOPE, ids=ids(CC.ENVELOPE))
def test_predicates_agree_with_the_entry_points(K, c):
    """K.conv_*_supported true -> the entry point takes the case and matches the reference; a shape outside the
    predicate -> SmxError with every output still as it was.  The Python predicates are knowingly stricter than C in
    two places, where only `true -> accepted` is asserted: conv_cl_dgrad_supported wants dy 16-byte aligned for every
    cout (C only for cout % 4 == 0, the float4 loads), and conv_u8_supported's weight alignment also guards the weight
    gradient, which has no weight operand."""
    x = CC.build(c, 'cuda')
    pred = CC.predicate(K, x)
    if c.mis is None:
        assert pred == CC.shape_ok(c)
    assert not pred or CC.c_accepts(c)
    buf, n = CC.workspace(K, c, 'cuda')
    ws = None if buf is None else buf[:n]
    if CC.c_accepts(c):
        CC.run(K, x, ws=ws)
        CC.check(x)
    else:
        with pytest.raises(L.SmxError):
            CC.run(K, x, ws=ws)
        torch.cuda.synchronize()
        CC.check(x, untouched=True)
        if buf is not None:
            assert bool(torch.isnan(buf[:n]).all())
    CC.check_workspace(c.id, buf, n)


@pytest.mark.parametrize('c', CC.WORKSPACE_REFUSALS, ids=ids(CC.WORKSPACE_REFUSALS))
def test_a_workspace_one_float_short_is_refused_and_nothing_is_written(K, c):
    x = CC.build(c, 'cuda')
    buf, n = CC.workspace(K, c, 'cuda', short=1)
    with pytest.raises(L.SmxError):
        CC.run(K, x, ws=buf[:n])
    torch.cuda.synchronize()
    CC.check(x, untouched=True)
    assert bool(torch.isnan(buf[:n]).all())
    CC.check_workspace(c.id, buf, n)


def test_the_workspace_sizes_are_the_partials_of_the_capped_grids(K):
    for c in CC.CASES:
        if c.op == 'u8_wgrad':
            Kc = c.C * c.k * c.k
            assert K.conv_u8_wgrad_ws_floats(c.cout, Kc) == 512 * (c.cout * Kc + c.cout), c.id
        elif c.op == 'cl_wgrad':
            OP = 16 * CC.plan(c).inst[1]
            assert K.conv_cl_wgrad_ws_floats(c.cout, c.k) == 1024 * (OP * 16 * c.k * c.k + OP), c.id
        if c.op in ('u8_wgrad', 'cl_wgrad'):
            assert CC.plan(c).partials <= (512 if c.op == 'u8_wgrad' else 1024)


@pytest.mark.parametrize('implicit_wgrad', [True, False])
@pytest.mark.parametrize('F,C,H,W,feat', CC.STEM_FALLBACK)
def test_cnn_stem_with_a_materialised_first_convolution_matches_aten(K, F, C, H, W, feat, implicit_wgrad):
    """the stem whose first convolution is outside conv_u8_supported (K = 320 > 256; W % 4 != 0) goes im2col / 255 +
    linear: the same comparison with ATen, at the same tolerances, as test_cnn_stem_forward_backward_match_aten"""
    frames = torch.zeros(F, C, H, W, dtype=torch.uint8, device='cuda')
    assert not K.conv_u8_supported(frames, C, H, W, 8, 4, 16)
    TK.test_cnn_stem_forward_backward_match_aten(K, F, C, H, W, feat, implicit_wgrad)
