"""GPU tier: TD3 (use_double_critic, use_action_regularization) on the DDPG row schedule -- smx_ddpg_rows_critic_td3_f32,
SMX_DDPG_GROUP_CRITIC2, SMX_DDPG_PACK_SECOND -- against the reference goldens, the float32 restatement at the real shape
and, buffer by buffer, the layer-by-layer schedule that carried TD3 alone before."""
import copy

import numpy as np
import pytest

import ddpg_helpers as DH
import ddpg_oracle
from surreal_amd import synthetic

pytestmark = pytest.mark.gpu

ROWS = {'ddpg_row_schedule': True}


def td3_case(D, A, ah, ch, B, action_reg=True, **hyper):
    """a TD3 case at the given shape with configs[2]'s learning rates (at the tiny goldens' 1e-2 one Adam step of a critic
    on a noise-floor gradient moves the actor phase of the same iteration by per cents: test_gpu_ddpg.py's sweep)"""
    g, case = DH.load('tiny_td3_hard' if action_reg else 'tiny_double_soft')
    h = dict(case['hyper'], lr_actor=1e-4, lr_critic=1e-3)
    h.update(hyper)
    return dict(case, D=D, A=A, ah=list(ah), ch=list(ch), B=B, hyper=h)


def learn(L, case, seed, np_seed):
    np.random.seed(np_seed)            # the action-regularisation noise comes from numpy's global stream
    return dict(L.learn(copy.deepcopy(synthetic.make_ddpg_batch(case['B'], case['D'], case['A'], seed=seed))))


def close(k, x, y):
    scale = float(y.abs().max()) + 1e-30
    d = float((x - y).abs().max())
    assert d <= 2e-6 * max(scale, 1.0) + 2e-5 * scale, '%s: max |diff| %g at scale %g' % (k, d, scale)


def packed_copies_are_current(L):
    import torch
    ws = L._ws
    torch.cuda.synchronize()
    kept, kept2 = ws.rows_packed.clone(), ws.rows_packed2.clone()
    L.K.ddpg_rows_pack(ws.rows_args)
    L.K.ddpg_rows_pack_second(ws.rows_args)
    torch.cuda.synchronize()
    assert torch.equal(kept, ws.rows_packed) and torch.equal(kept2, ws.rows_packed2)
    assert float(kept.abs().sum()) > 0 and float(kept2.abs().sum()) > 0


# ---- 1. the reference goldens through the rows ---------------------------------------------------------------------
@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('name', ['tiny_td3_hard', 'tiny_double_soft'])
def test_td3_goldens_through_the_row_schedule(name, fused):
    """the helper's own bars: statistics and every element of model, target, model2 and target2 at 1e-5"""
    opts = dict(ROWS) if fused else dict(ROWS, ddpg_rows_fused_update=False)
    L = DH.run_and_check(name, opts=opts)
    assert L._ws.rows_args is not None and L._ws.graph is not None
    assert L._schedule(L._ws.key[0], L._ws.key[1]) == 'rows'


# ---- 2. the restatement at the real shape --------------------------------------------------------------------------
def test_td3_rows_match_the_restatement_at_configs2_shape():
    """17 -> 300/200, 400/300, 6 actions, batch 512, both TD3 switches, three iterations across a hard update: statistics
    and every parameter of the four models and targets at 1e-5 (the bars cfg3_cheetah512 is held to)"""
    case = td3_case(17, 6, (300, 200), (400, 300), 512, target_update_interval=2)
    h = case['hyper']
    mk = lambda seed: ddpg_oracle.make_ddpg_params(17, 6, (300, 200), (400, 300), seed=seed)  # noqa: E731
    O = ddpg_oracle.OracleDDPGLearner(
        mk(3), gamma=h['gamma'], n_step=h['n_step'], lr_actor=h['lr_actor'], lr_critic=h['lr_critic'],
        clip_critic_gradient=h.get('clip_critic', False), target_update_type='hard', target_update_interval=2,
        use_double_critic=True, use_action_regularization=True, params2=mk(4), batch_size=512,
        **ddpg_oracle.clip_reg_kwargs(h))
    L = DH.make_learner(case, ROWS)
    for it in range(3):
        b = synthetic.make_ddpg_batch(512, 17, 6, seed=10 + it)
        np.random.seed(1000 + it)
        so = O.learn(copy.deepcopy(b))
        np.random.seed(1000 + it)
        sl = dict(L.learn(copy.deepcopy(b)))
        assert set(sl) == set(so)
        for k, v in so.items():
            print('iteration %d %s: %g' % (it, k, abs(sl[k] - v)))
            np.testing.assert_allclose(sl[k], v, atol=1e-5, rtol=1e-5, err_msg='iteration %d %s' % (it, k))
    assert L._ws.rows_args is not None
    for which, got, want in (('model', L.model, O.model), ('target', L.model_target, O.model_target),
                             ('model2', L.model2, O.model2), ('target2', L.model_target2, O.model_target2)):
        got, want = got.numpy_params(), want.numpy_params()
        assert got
        for k in got:
            d = float(np.abs(got[k] - want[k]).max())
            print('%s %s: %g' % (which, k, d))
            assert d <= 1e-5, (which, k, d)


# ---- 3. one iteration, buffer by buffer, against the layer schedule ------------------------------------------------
def check_buffers(case, prepare=None, np_seed=5):
    """-> (rows learner, layers learner, the layers side's mu'(s') before the iteration)"""
    import torch
    rows, layers = DH.make_learner(case, ROWS), DH.make_learner(case)
    for L in (rows, layers):
        if prepare is not None:
            prepare(L)
    B, D, A = case['B'], case['D'], case['A']
    b = synthetic.make_ddpg_batch(B, D, A, seed=91)
    # what the layer schedule overwrites within the iteration, formed by the same launches in front of it: the first
    # critic's forward pass at (s, a) -- its workspace serves Q(s, mu(s)) afterwards -- and the target policy's action
    t = lambda v: torch.as_tensor(v, dtype=torch.float32).cuda()  # noqa: E731
    x, xn, acts = t(b['obs']['low_dim']['flat_inputs']), t(b['obs_next']['low_dim']['flat_inputs']), t(b['actions'])
    w1, q1 = layers.model.workspace(B, 'cuda'), torch.empty(B, device='cuda')
    layers.model.critic_forward(x, acts, w1, q1)
    mu_next = torch.empty(B, A, device='cuda')
    layers.model_target.actor_forward(xn, layers.model.workspace(B, 'cuda'), mu_next)
    learn(rows, case, 91, np_seed)
    learn(layers, case, 91, np_seed)
    torch.cuda.synchronize()
    wr, wl = rows._ws, layers._ws
    assert getattr(wr, 'rows_args', None) is not None and getattr(wl, 'rows_args', None) is None
    r1, r2, l1, l2 = wr.critics[0], wr.critics[1], wl.critics[0], wl.critics[1]
    c1 = rows.model.c1
    pairs = [('q1', r1.q, l1.q), ('q1 (in front)', r1.q, q1), ('q2', r2.q, l2.q), ('y', wr.y, l1.y), ('y (critic 2)', wr.y, l2.y),
             ('dz3_1', wr.dz3, (2.0 * (l1.q - l1.y)) / B), ('dz3_2', r2.dz3, l2.dz3),
             ('xcat1', wr.xcat, w1.xcat), ('h2c1', wr.h2c, w1.h2c), ('xcat2', r2.w.xcat, l2.w.xcat), ('h2c2', r2.w.h2c, l2.w.h2c),
             ('q_next (Q1\')', wr.q_next, wl.q_next), ('q_next (min)', wr.q_next2, wl.q_next2),
             ('act', wr.act, wl.act), ('q_actor', wr.q_actor, wl.q_actor), ('dz3a', wr.dz3a, wl.dz3a),
             ('grads critic 1', r1.grads, l1.grads), ('grads critic 2', r2.grads, l2.grads), ('grads actor', wr.grads_a, wl.grads_a)]
    for k, a, bb in pairs:
        close(k, a, bb)
    assert int(wr.step[0]) == int(wl.step[0]) == 1
    return rows, layers, mu_next


@pytest.mark.parametrize('D,A,ah,ch,B', [
    (1, 1, (4, 4), (4, 4), 5),                    # the smallest shapes the row kernels take
    (50, 32, (1024, 64), (64, 1024), 130),        # two head tiles; K = 1024 split over the waves in two trips
    (17, 6, (304, 204), (404, 300), 515),         # tile counts off the multiples of eight, a ragged last block
    (17, 6, (300, 200), (400, 300), 37),
    (17, 6, (300, 200), (400, 300), 1030),        # several rounds of workgroups
])
def test_td3_row_launches_fill_the_layer_schedules_buffers(D, A, ah, ch, B):
    case = td3_case(D, A, ah, ch, B, target_update_type='soft', tau=0.1)
    rows, layers, _ = check_buffers(case)
    learn(rows, case, 92, 6)                       # (the update launches' copies, twice)
    packed_copies_are_current(rows)


# ---- 4. the switches bind ------------------------------------------------------------------------------------------
def test_td3_min_and_clamp_bind():
    """preconditions on the layer schedule's side: the min picks each critic on some rows, and the noised target action
    is clamped at +-1 on some elements and not on others (the target actor's last layer scaled so that tanh saturates on
    part of the batch) -- then y and the min'd Q' agree as in the sweep"""
    import torch
    case = td3_case(17, 6, (300, 200), (400, 300), 37, target_update_type='soft', tau=0.1)

    def saturate(L):
        with torch.no_grad():
            L.model_target.actor.views['W3'].mul_(6.0)
    rows, layers, mu_next = check_buffers(case, prepare=saturate)
    wl = layers._ws
    np.random.seed(5)
    noise = torch.as_tensor(np.clip(np.random.normal(0, 0.2, size=(37, 6)), -0.5, 0.5), dtype=torch.float32).cuda()
    pre = mu_next + noise
    assert bool((pre.abs() > 1.0).any()) and bool((pre.abs() < 1.0).any())
    assert torch.equal(wl.act_n, pre.clamp(-1.0, 1.0)) and torch.equal(wl.s_noise, noise)
    first = wl.q_next2 == wl.q_next                 # rows on which the first target critic is the smaller one
    assert bool(first.any()) and bool((~first).any())


def test_td3_rows_double_critic_without_action_regularization():
    case = td3_case(17, 6, (300, 200), (400, 300), 37, action_reg=False)
    rows, layers, _ = check_buffers(case)
    assert not rows.use_action_regularization and rows._ws.rows_args.second.contents.noise is None


# ---- 5. four iterations against the layer schedule -----------------------------------------------------------------
@pytest.mark.parametrize('name', ['tiny_td3_hard', 'tiny_double_soft'])
def test_td3_row_schedule_agrees_with_the_layer_schedule(name):
    """the bounds of test_row_schedule_agrees_with_the_level_schedule, for the second critic and its target too; once
    across a hard update at interval 2, once with soft updates"""
    g, case = DH.load(name)
    rows, layers = DH.make_learner(case, ROWS), DH.make_learner(case)
    for it in range(4):
        sa, sb = learn(rows, case, 10 + it, 1000 + it), learn(layers, case, 10 + it, 1000 + it)
        for k in sb:
            np.testing.assert_allclose(sa[k], sb[k], rtol=2e-5, atol=2e-6, err_msg='%s iteration %d' % (k, it))
    assert getattr(rows._ws, 'rows_args', None) is not None and getattr(layers._ws, 'rows_args', None) is None
    lr = max(case['hyper']['lr_actor'], case['hyper']['lr_critic'])
    flats = [(a.actor_flat, b.actor_flat) for a, b in ((rows.model, layers.model), (rows.model_target, layers.model_target))]
    flats += [(a.critic_flat, b.critic_flat) for a, b in ((rows.model, layers.model), (rows.model_target, layers.model_target),
                                                          (rows.model2, layers.model2),
                                                          (rows.model_target2, layers.model_target2))]
    for x, y in flats:
        d = (x - y).abs()
        assert float(d.max()) <= 2 * lr * 4 + 1e-6, float(d.max())
        assert float((d > 2e-6).float().mean()) < 0.02, float((d > 2e-6).float().mean())
    packed_copies_are_current(rows)


# ---- 6. writes from outside are repacked ---------------------------------------------------------------------------
def test_second_critic_written_from_outside_is_repacked():
    """parameters written into model2.critic_flat and model_target2.critic_flat between iterations (torch writes: the
    version counters move) reach the row kernels: the next iteration equals the layer schedule's from the same state"""
    import torch
    case = td3_case(17, 6, (300, 200), (400, 300), 37)
    rows, layers = DH.make_learner(case, ROWS), DH.make_learner(case)
    for it in range(3):
        learn(rows, case, 10 + it, 1000 + it)
        learn(layers, case, 10 + it, 1000 + it)
    gen = torch.Generator(device='cuda').manual_seed(5)
    new2 = torch.randn(rows.model2.critic_flat.shape, generator=gen, device='cuda') * 0.05
    newt2 = torch.randn(rows.model2.critic_flat.shape, generator=gen, device='cuda') * 0.05
    for L in (rows, layers):
        L.model2.critic_flat.copy_(new2)
        L.model_target2.critic_flat.copy_(newt2)
    sa, sb = learn(rows, case, 13, 1003), learn(layers, case, 13, 1003)
    for k in sb:
        np.testing.assert_allclose(sa[k], sb[k], rtol=2e-5, atol=2e-6, err_msg=k)
    torch.cuda.synchronize()
    close('q2', rows._ws.critics[1].q, layers._ws.critics[1].q)
    close('q_next (min)', rows._ws.q_next2, layers._ws.q_next2)
