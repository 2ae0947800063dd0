"""CPU tier: use_layernorm (one critic) on the DDPG row schedule -- the learner's routing, the launch sequence and what a
torch write to a LayerNorm gain does, through the torch-CPU double of the LayerNorm row launches (ddpg_ln_rows_cases.py)
against the reference goldens; and the host-side predicate of the library."""
import numpy as np
import pytest

import ddpg_helpers as DH
import ddpg_ln_rows_cases as LC
from surreal_amd import synthetic

LN_CASES = ['tiny_ln_hard', 'ln_soft_clipcritic']
ROWS = {'ddpg_row_schedule': True}


@pytest.fixture
def ln_double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(LC.LnRowsCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


def batch(case, seed):
    return synthetic.make_ddpg_batch(case['B'], case['D'], case['A'], seed=seed)


@pytest.mark.parametrize('name', LN_CASES)
def test_ln_goldens_through_the_rows(ln_double, name):
    """the helper's own bars: statistics and every parameter, ln* included, at 1e-5"""
    L = DH.run_and_check(name, opts=dict(ROWS))
    assert getattr(L._ws, 'rows_args', None) is not None
    assert L._schedule(L._ws.key[0], L._ws.key[1]) == 'rows'
    assert 'ddpg_rows_critic' in ln_double.calls and not any(c.startswith('layernorm') for c in ln_double.calls)
    assert any(k.startswith('actor.ln') for k in L.model.numpy_params())


def test_ln_rows_launch_sequence(ln_double):
    """one pack in front of the first iteration, then 4 launches per iteration as for plain DDPG: critic chain, the critic's
    gradient-and-step launch, actor chain, the actor's"""
    g, case = DH.load('tiny_ln_hard')
    L = DH.make_learner(case, ROWS)
    K = ln_double
    del K.calls[:]
    it = ['ddpg_rows_critic', 'ddpg_rows_update:critic:wgrad', 'ddpg_rows_actor', 'ddpg_rows_update:actor:wgrad']
    for i in range(3):
        L.learn(batch(case, 10 + i))
    assert K.calls == ['ddpg_rows_pack'] + it * 3, K.calls


def test_a_torch_write_to_a_gain_reaches_the_next_iteration(ln_double):
    """the gains and biases are read from the parameter buffers: a write between iterations (to the model's and to the
    target's) is what the next iteration runs with -- it equals the layer schedule's from the same state"""
    import torch
    g, case = DH.load('ln_soft_clipcritic')
    rows, layers = DH.make_learner(case, ROWS), DH.make_learner(case)
    for i in range(2):
        rows.learn(batch(case, 10 + i))
        layers.learn(batch(case, 10 + i))
    gen = torch.Generator().manual_seed(5)
    new = {k: 1.0 + 0.3 * torch.randn(v.shape, generator=gen) for k, v in rows.model.named_parameters().items()
           if k.endswith('ln1.W') or k.endswith('ln2.W')}
    assert len(new) == 4
    for L in (rows, layers):
        for M in (L.model, L.model_target):
            named = M.named_parameters()
            for k, v in new.items():
                named[k].copy_(v if M is L.model else 0.5 * v)
    before = rows.model.critic['ln2.W'].clone()
    sa, sb = dict(rows.learn(batch(case, 12))), dict(layers.learn(batch(case, 12)))
    for k in sb:
        np.testing.assert_allclose(sa[k], sb[k], rtol=2e-5, atol=2e-6, err_msg=k)
    assert not torch.equal(before, rows.model.critic['ln2.W'])                       # (and the gain took its step)
    for a, b in ((rows.model, layers.model), (rows.model_target, layers.model_target)):
        pa, pb = a.numpy_params(), b.numpy_params()
        for k in pb:
            np.testing.assert_allclose(pa[k], pb[k], rtol=0, atol=1e-5, err_msg=k)
    assert getattr(rows._ws, 'rows_args', None) is not None and getattr(layers._ws, 'rows_args', None) is None


def test_ln_stays_on_layers_unless_asked_and_able(cpu_double):
    """the stock double has no LayerNorm row launches; with the capable double: the flag unset or False, a double critic,
    camera observations, ddpg_rows_fused_update = False, a batch the predicate refuses"""
    from surreal_amd import kernels as KN
    g, case = DH.load('tiny_ln_hard')
    L = DH.make_learner(case, ROWS)                                        # stock double
    assert L._schedule(case['B'], case['D']) == 'layers'
    L.learn(batch(case, 10))
    assert getattr(L._ws, 'rows_args', None) is None
    prev = KN.set_default_kernels(LC.LnRowsCpuKernels(), 'cpu')
    try:
        for opts in ({}, {'ddpg_row_schedule': False}, dict(ROWS, ddpg_rows_fused_update=False)):
            L = DH.make_learner(case, opts)
            assert L._schedule(case['B'], case['D']) == 'layers', opts
            L.learn(batch(case, 10))
            assert getattr(L._ws, 'rows_args', None) is None
            assert not any(c.startswith('ddpg_rows') for c in KN.default_kernels().calls)
        for name in ('tiny_ln_td3_soft', 'tiny_ln_pixel_hard'):
            g2, case2 = DH.load(name)
            L = DH.make_learner(case2, ROWS)
            assert L._schedule(case2['B'], case2['D']) == 'layers', name
            np.random.seed(1000)
            L.learn(synthetic.make_ddpg_batch(case2['B'], case2['D'], case2['A'], seed=10,
                                              pixel=tuple(case2['pixel']) if case2.get('pixel') else None))
            assert getattr(L._ws, 'rows_args', None) is None
            assert not any(c.startswith('ddpg_rows') for c in KN.default_kernels().calls)
        L = DH.make_learner(case, ROWS)
        assert L._schedule(case['B'], case['D']) == 'rows'
        assert L._schedule(2 ** 24, case['D']) == 'layers'                 # a batch the predicate refuses
    finally:
        KN.set_default_kernels(*prev)


def test_plain_and_td3_routes_are_what_they_were(ln_double):
    """the capable double changes nothing for learners without LayerNorm: plain DDPG takes the rows by default, TD3 stays
    on the layers (this double has no TD3 row launches)"""
    for name, want in (('tiny_hard', 'rows'), ('tiny_td3_hard', 'layers')):
        g, case = DH.load(name)
        L = DH.make_learner(case)
        assert L._schedule(case['B'], case['D']) == want, name


def test_ln_predicate_of_the_library():
    """host-side arithmetic of the library (no GPU): the predicate accepts the GPU sweep's shapes at 512 rows, refuses what
    the plain predicate refuses and what no longer fits in LDS with the pre-LayerNorm and dn tiles kept, and a batch whose
    widest row-major buffer passes 2^31 bytes (which the plain predicate lets through)"""
    from surreal_amd import _lib as L
    lib = L.load()
    for D, A, ah, ch, B in LC.SWEEP:
        assert lib.smx_ddpg_rows_ln_supported(D, A, ah[0], ah[1], ch[0], ch[1], 512) == 1, (D, A, ah, ch)
        assert lib.smx_ddpg_rows_ln_supported(D, A, ah[0], ah[1], ch[0], ch[1], B) == 1, (D, A, ah, ch, B)
    for d in [(17, 6, 302, 200, 400, 300), (17, 6, 300, 200, 400, 298), (17, 33, 300, 200, 400, 300), (0, 6, 300, 200, 400, 300),
              (17, 6, 300, 200, 1028, 300), (4096, 6, 300, 200, 400, 300)]:
        assert lib.smx_ddpg_rows_supported(*d) == 0, d
        assert lib.smx_ddpg_rows_ln_supported(*d, 512) == 0, d
    # never more than the plain predicate accepts, and strictly less somewhere: the observation widths around the LDS limit
    edge = [(D, 32, 1024, 1024, 1024, 1024) for D in range(64, 2049, 64)] + [(D, 6, 300, 200, 400, 300) for D in range(64, 2049, 64)]
    narrower = 0
    for d in edge:
        ln, plain = lib.smx_ddpg_rows_ln_supported(*d, 512), lib.smx_ddpg_rows_supported_at(*d, 512)
        assert ln <= plain, d
        narrower += plain - ln
    assert narrower > 0
    assert lib.smx_ddpg_rows_ln_supported(2048, 32, 1024, 1024, 1024, 1024, 512) == 0       # 177 KB of tiles
    # row counts
    d = (17, 6, 300, 200, 400, 300)
    assert lib.smx_ddpg_rows_ln_supported(*d, 0) == 0 and lib.smx_ddpg_rows_ln_supported(*d, 2 ** 24) == 0
    wide = (17, 32, 1024, 1024, 1024, 1024)                          # widest buffer: xcat / dxcat, 1056 floats a row
    limit = 2 ** 31 // (1056 * 4)
    assert lib.smx_ddpg_rows_ln_supported(*wide, limit) == 1
    assert lib.smx_ddpg_rows_ln_supported(*wide, limit + 1) == 0
    assert lib.smx_ddpg_rows_supported_at(*wide, limit + 1) == 1      # (the plain predicate has no such check)
