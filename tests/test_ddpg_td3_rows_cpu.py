"""CPU tier: TD3 (double critic, action regularisation) on the DDPG row schedule -- the learner's routing, the launch
sequence and WHEN each packed copy is refreshed, through the torch-CPU double of the TD3 row launches
(ddpg_td3_rows_cases.py) against the reference goldens; and the host-side predicate / size query of the library."""
import numpy as np
import pytest

import ddpg_helpers as DH
import ddpg_td3_rows_cases as TC
from surreal_amd import synthetic

TD3_CASES = ['tiny_td3_hard', 'tiny_double_soft']


@pytest.fixture
def td3_double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(TC.Td3RowsCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('name', TD3_CASES)
def test_td3_goldens_through_the_rows(td3_double, name, fused):
    L = DH.run_and_check(name, opts={'ddpg_row_schedule': True, 'ddpg_rows_fused_update': fused})
    assert getattr(L._ws, 'rows_args', None) is not None
    assert 'ddpg_rows_critic_td3' in td3_double.calls


@pytest.mark.parametrize('fused', [True, False])
def test_td3_rows_launch_sequence(td3_double, fused):
    """one rank: 2 chain launches + 3 gradient-and-step launches per iteration, in the order critic chain, critic-1 step,
    critic-2 step, actor chain, actor step; both packs once, in front of the first iteration only.  Unfused: each step has
    its linear_multi of weight gradients in front, and the two statistics launches close the iteration"""
    g, case = DH.load('tiny_td3_hard')
    L = DH.make_learner(case, {'ddpg_row_schedule': True, 'ddpg_rows_fused_update': fused})
    K = td3_double
    del K.calls[:]
    w = ':wgrad' if fused else ''
    it = ['ddpg_rows_critic_td3', 'ddpg_rows_update:critic' + w, 'ddpg_rows_update:critic2' + w, 'ddpg_rows_actor',
          'ddpg_rows_update:actor' + w]
    if not fused:
        it = [it[0], 'linear_multi', it[1], 'linear_multi', it[2], it[3], 'linear_multi', it[4], 'ddpg_stats', 'ddpg_stats']
    for i in range(3):
        np.random.seed(1000 + i)
        L.learn(synthetic.make_ddpg_batch(case['B'], case['D'], case['A'], seed=10 + i))
    assert K.calls == ['ddpg_rows_pack', 'ddpg_rows_pack_second'] + it * 3, K.calls
    # a parameter written from outside: both packs again, once
    del K.calls[:]
    L.model_target2.critic_flat.mul_(1.0)
    np.random.seed(1003)
    L.learn(synthetic.make_ddpg_batch(case['B'], case['D'], case['A'], seed=13))
    assert K.calls == ['ddpg_rows_pack', 'ddpg_rows_pack_second'] + it, K.calls


@pytest.mark.parametrize('name', TD3_CASES)
def test_td3_stays_on_layers_unless_asked_and_able(name, cpu_double, request):
    """the stock double has no TD3 row launches: a double-critic learner that asks for the rows falls back to the layer
    schedule; with the capable double it does so when the flag is unset or False, or the shapes are refused"""
    from surreal_amd import kernels as KN
    g, case = DH.load(name)
    b = synthetic.make_ddpg_batch(case['B'], case['D'], case['A'], seed=10)
    L = DH.make_learner(case, {'ddpg_row_schedule': True})                 # stock double
    assert L._schedule(case['B'], case['D']) == 'layers'
    L.learn(b)
    assert getattr(L._ws, 'rows_args', None) is None
    prev = KN.set_default_kernels(TC.Td3RowsCpuKernels(), 'cpu')
    try:
        for opts in ({}, {'ddpg_row_schedule': False}):
            L = DH.make_learner(case, opts)
            assert L._schedule(case['B'], case['D']) == 'layers', opts
            L.learn(synthetic.make_ddpg_batch(case['B'], case['D'], case['A'], seed=10))
            assert getattr(L._ws, 'rows_args', None) is None
            assert not any(c.startswith('ddpg_rows') for c in KN.default_kernels().calls)
        L = DH.make_learner(case, {'ddpg_row_schedule': True})
        assert L._schedule(case['B'], case['D']) == 'rows'
        assert L._schedule(2 ** 24, case['D']) == 'layers'                 # a batch the predicate refuses
    finally:
        KN.set_default_kernels(*prev)


def test_second_critic_predicate_and_size_query():
    """host-side arithmetic of the library (no GPU): the second packed buffer is the seven blocks' pack_words; the
    predicate refuses what the one-critic predicate refuses, what no longer fits in LDS with y kept, and a batch whose
    widest row-major buffer passes 2^31 bytes (which the old predicate lets through)"""
    from surreal_amd import _lib as L
    lib = L.load()
    shapes = [(17, 6, 300, 200, 400, 300), (1, 1, 4, 4, 4, 4), (50, 32, 1024, 64, 64, 1024), (17, 6, 304, 204, 404, 300),
              (2048, 3, 128, 36, 36, 128), (376, 17, 300, 200, 400, 300)]
    for d in shapes:
        assert lib.smx_ddpg_rows_second_supported(*d, 512) == 1, d
        want = 4 * sum(TC.pack_words(M, K) for M, K in TC.second_blocks(*d))
        assert lib.smx_ddpg_rows_second_packed_floats(*d) == want, d
        assert lib.smx_ddpg_rows_packed_floats(*d) > want           # (the first buffer is where it was: 16 blocks)
    # what dims_ok refuses
    for d in [(17, 6, 302, 200, 400, 300), (17, 6, 300, 200, 400, 298), (17, 33, 300, 200, 400, 300), (0, 6, 300, 200, 400, 300),
              (17, 6, 300, 200, 1028, 300), (4096, 6, 300, 200, 400, 300)]:
        assert lib.smx_ddpg_rows_supported(*d) == 0, d
        assert lib.smx_ddpg_rows_second_supported(*d, 512) == 0, d
        assert lib.smx_ddpg_rows_second_packed_floats(*d) == 0, d
    # never more than the one-critic predicate accepts: the observation widths around its LDS limit
    edge = [(D, 32, 1024, 1024, 1024, 1024) for D in range(64, 2049, 64)] + [(D, 6, 300, 200, 400, 300) for D in range(64, 2049, 64)]
    for d in edge:
        assert lib.smx_ddpg_rows_second_supported(*d, 512) <= lib.smx_ddpg_rows_supported(*d), d
    # row counts
    d = (17, 6, 300, 200, 400, 300)
    assert lib.smx_ddpg_rows_second_supported(*d, 0) == 0 and lib.smx_ddpg_rows_second_supported(*d, 2 ** 24) == 0
    wide = (17, 32, 1024, 1024, 1024, 1024)                          # widest buffer: xcat, 1056 floats a row
    limit = 2 ** 31 // (1056 * 4)
    assert lib.smx_ddpg_rows_second_supported(*wide, limit) == 1
    assert lib.smx_ddpg_rows_second_supported(*wide, limit + 1) == 0
    assert lib.smx_ddpg_rows_supported_at(*wide, limit + 1) == 1      # (the old predicate has no such check)
    obs = (2048, 3, 128, 36, 36, 128)                                # ... or the observations themselves
    assert lib.smx_ddpg_rows_second_supported(*obs, 2 ** 18 - 1) == 1 and lib.smx_ddpg_rows_second_supported(*obs, 2 ** 18) == 0
