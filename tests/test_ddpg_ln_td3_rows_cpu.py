"""CPU tier: use_layernorm together with TD3's double critic on the DDPG row schedule -- the learner's routing, the launch
sequence and what a torch write to the second critic's gain does, through the torch-CPU double of the LayerNorm TD3 row
launches (ddpg_ln_td3_rows_cases.py) against the reference goldens; and the host-side predicate of the library."""
import numpy as np
import pytest

import ddpg_helpers as DH
import ddpg_ln_rows_cases as LC
import ddpg_ln_td3_rows_cases as LT
from surreal_amd import synthetic

LN_TD3_CASES = ['tiny_ln_td3_soft', 'tiny_ln_td3_reg_clip']
ROWS = {'ddpg_row_schedule': True}


@pytest.fixture
def ln_td3_double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(LT.LnTd3RowsCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


def batch(case, seed):
    np.random.seed(1000 + seed)            # TD3's action-regularisation noise (numpy's global stream)
    return synthetic.make_ddpg_batch(case['B'], case['D'], case['A'], seed=seed,
                                     pixel=tuple(case['pixel']) if case.get('pixel') else None)


@pytest.mark.parametrize('name', LN_TD3_CASES)
def test_ln_td3_goldens_through_the_rows(ln_td3_double, name):
    """the helper's own bars: statistics and every element of model, target, model2 and target2, ln* included, at 1e-5"""
    L = DH.run_and_check(name, opts=dict(ROWS))
    assert L.use_layernorm and L.use_double_critic
    assert getattr(L._ws, 'rows_args', None) is not None
    assert L._schedule(L._ws.key[0], L._ws.key[1]) == 'rows'
    calls = ln_td3_double.calls
    assert 'ddpg_rows_critic_td3' in calls and 'ddpg_rows_update:critic2:wgrad' in calls
    assert 'ddpg_rows_critic' not in calls and not any(c.startswith('layernorm') for c in calls)
    assert any(k.startswith('critic.ln') for k in L.model2.numpy_params())


def test_ln_td3_rows_launch_sequence(ln_td3_double):
    """one pack and one pack of the second critic's buffer in front of the first iteration, then TD3's 5 launches per
    iteration"""
    g, case = DH.load('tiny_ln_td3_soft')
    L = DH.make_learner(case, ROWS)
    K = ln_td3_double
    del K.calls[:]
    it = ['ddpg_rows_critic_td3', 'ddpg_rows_update:critic:wgrad', 'ddpg_rows_update:critic2:wgrad', 'ddpg_rows_actor',
          'ddpg_rows_update:actor:wgrad']
    for i in range(3):
        L.learn(batch(case, 10 + i))
    assert K.calls == ['ddpg_rows_pack', 'ddpg_rows_pack_second'] + it * 3, K.calls


def stays_on_layers(double, name, opts):
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(double, 'cpu')
    try:
        g, case = DH.load(name)
        L = DH.make_learner(case, opts)
        assert L._schedule(case['B'], case['D']) == 'layers', (type(double).__name__, name, opts)
        L.learn(batch(case, 10))
        assert getattr(L._ws, 'rows_args', None) is None
        assert not any(c.startswith('ddpg_rows') for c in double.calls), double.calls
    finally:
        KN.set_default_kernels(*prev)


def test_ln_td3_stays_on_layers_unless_asked_and_able():
    """the stock double and the one-critic LayerNorm double cannot run it; with the capable double: the flag unset or
    False, ddpg_rows_fused_update = False, camera observations, a batch the predicate refuses"""
    from surreal_amd import kernels as KN
    stays_on_layers(LT.RecordingStockKernels(), 'tiny_ln_td3_soft', ROWS)
    stays_on_layers(LC.LnRowsCpuKernels(), 'tiny_ln_td3_soft', ROWS)
    for opts in ({}, {'ddpg_row_schedule': False}, dict(ROWS, ddpg_rows_fused_update=False)):
        stays_on_layers(LT.LnTd3RowsCpuKernels(), 'tiny_ln_td3_soft', opts)
    stays_on_layers(LT.LnTd3RowsCpuKernels(), 'tiny_ln_pixel_td3_soft', ROWS)
    prev = KN.set_default_kernels(LT.LnTd3RowsCpuKernels(), 'cpu')
    try:
        g, case = DH.load('tiny_ln_td3_soft')
        L = DH.make_learner(case, ROWS)
        assert L._schedule(case['B'], case['D']) == 'rows'
        # a batch the predicate refuses: the routing decision alone -- 2^24 rows cannot be allocated and run here, so there
        # is no iteration whose recorded calls could be inspected; _enqueue_iteration takes exactly this answer
        del KN.default_kernels().calls[:]
        assert L._schedule(2 ** 24, case['D']) == 'layers'
        assert not any(c.startswith('ddpg_rows') for c in KN.default_kernels().calls)
    finally:
        KN.set_default_kernels(*prev)


def test_the_other_routes_are_what_they_were(ln_td3_double):
    """a guard on UNCHANGED behaviour (it passes before the LayerNorm TD3 cell existed and does not cover that cell): the
    capable double routes the three other cells as their own doubles do -- plain DDPG on the rows by default, TD3 and
    one-critic LayerNorm on the rows when asked to and on the layers otherwise"""
    for name, opts, want in (('tiny_hard', None, 'rows'), ('tiny_td3_hard', None, 'layers'), ('tiny_td3_hard', ROWS, 'rows'),
                             ('tiny_ln_hard', None, 'layers'), ('tiny_ln_hard', ROWS, 'rows')):
        g, case = DH.load(name)
        L = DH.make_learner(case, opts)
        assert L._schedule(case['B'], case['D']) == want, (name, opts)


def test_a_torch_write_to_the_second_critics_gain_reaches_the_next_iteration(ln_td3_double):
    """the second critic's gains and biases are read from the parameter buffers: a write to ln2.W of model2 and of its
    target between iterations is what the next iteration runs with -- it equals the layer schedule's from the same state"""
    import torch
    g, case = DH.load('tiny_ln_td3_soft')
    rows, layers = DH.make_learner(case, ROWS), DH.make_learner(case)
    for i in range(2):
        rows.learn(batch(case, 10 + i))
        layers.learn(batch(case, 10 + i))
    gen = torch.Generator().manual_seed(5)
    new = 1.0 + 0.3 * torch.randn(rows.model2.critic['ln2.W'].shape, generator=gen)
    for L in (rows, layers):
        L.model2.critic['ln2.W'].copy_(new)
        L.model_target2.critic['ln2.W'].copy_(0.5 * new)
    before = rows.model2.critic['ln2.W'].clone()
    assert torch.equal(before, new)
    sa, sb = dict(rows.learn(batch(case, 12))), dict(layers.learn(batch(case, 12)))
    for k in sb:
        np.testing.assert_allclose(sa[k], sb[k], rtol=2e-5, atol=2e-6, err_msg=k)
    assert not torch.equal(before, rows.model2.critic['ln2.W'])                      # (and the gain took its step)
    for a, b in ((rows.model, layers.model), (rows.model_target, layers.model_target), (rows.model2, layers.model2),
                 (rows.model_target2, layers.model_target2)):
        pa, pb = a.numpy_params(), b.numpy_params()
        for k in pb:
            np.testing.assert_allclose(pa[k], pb[k], rtol=0, atol=1e-5, err_msg=k)
    assert getattr(rows._ws, 'rows_args', None) is not None and getattr(layers._ws, 'rows_args', None) is None
    # ... and it is the written gain the iteration ran with: without the write the statistics differ
    ref = DH.make_learner(case, ROWS)
    for i in range(2):
        ref.learn(batch(case, 10 + i))
    sc = dict(ref.learn(batch(case, 12)))
    assert abs(sc['critic_loss'] - sa['critic_loss']) > 1e-4 * abs(sc['critic_loss'])


def test_ln_td3_predicate_of_the_library():
    """host-side arithmetic of the library (no GPU): the predicate accepts the GPU sweep's shapes, refuses F > 1024, H not a
    multiple of 4, A > 32 and a row count whose byte offsets pass 2^31; it never accepts what the one-critic LayerNorm
    predicate or the TD3 predicate refuses"""
    from surreal_amd import _lib as L
    lib = L.load()
    f = lib.smx_ddpg_rows_ln_second_supported
    for D, A, ah, ch, B in LC.SWEEP:
        assert f(D, A, ah[0], ah[1], ch[0], ch[1], 512) == 1, (D, A, ah, ch)
        assert f(D, A, ah[0], ah[1], ch[0], ch[1], B) == 1, (D, A, ah, ch, B)
    for d in [(17, 6, 1028, 200, 400, 300), (17, 6, 300, 1028, 400, 300), (17, 6, 300, 200, 1028, 300),
              (17, 6, 300, 200, 400, 1028),                                                    # F > 1024
              (17, 6, 302, 200, 400, 300), (17, 6, 300, 202, 400, 300), (17, 6, 300, 200, 402, 300),
              (17, 6, 300, 200, 400, 298),                                                     # H not a multiple of 4
              (17, 33, 300, 200, 400, 300), (0, 6, 300, 200, 400, 300)]:
        assert f(*d, 512) == 0, d
    edge = [(D, 32, 1024, 1024, 1024, 1024) for D in range(64, 2049, 64)] + [(D, 6, 300, 200, 400, 300) for D in range(64, 2049, 64)]
    for d in edge:
        both = f(*d, 512)
        assert both <= lib.smx_ddpg_rows_ln_supported(*d, 512) and both <= lib.smx_ddpg_rows_second_supported(*d, 512), d
    assert f(2048, 32, 1024, 1024, 1024, 1024, 512) == 0
    # row counts
    d = (17, 6, 300, 200, 400, 300)
    assert f(*d, 0) == 0 and f(*d, 2 ** 24) == 0
    wide = (17, 32, 1024, 1024, 1024, 1024)                          # widest buffer: xcat / dxcat, 1056 floats a row
    limit = 2 ** 31 // (1056 * 4)
    assert f(*wide, limit) == 1
    assert f(*wide, limit + 1) == 0
