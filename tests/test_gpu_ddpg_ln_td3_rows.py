"""GPU tier: use_layernorm together with TD3's double critic on the DDPG row schedule -- smx_ddpg_rows_critic_td3_f32 and
SMX_DDPG_GROUP_CRITIC2 with args->ln and its second part -- against the reference goldens, the float32 restatement at the
real shape, buffer by buffer the layer-by-layer schedule that carried this configuration alone before, and bit for bit
smx_layernorm_forward_f32 / _backward_f32 on the second critic's own buffers.  The bars are test_gpu_ddpg_ln_rows.py's."""
import copy
import types

import numpy as np
import pytest

import ddpg_helpers as DH
import ddpg_ln_rows_cases as LC
import ddpg_oracle
from surreal_amd import synthetic

pytestmark = pytest.mark.gpu

ROWS = {'ddpg_row_schedule': True}
LN_TD3_CASES = ['tiny_ln_td3_soft', 'tiny_ln_td3_reg_clip']


def ln_td3_case(D, A, ah, ch, B, **hyper):
    """a LayerNorm TD3 case (both TD3 switches) at the given shape with configs[2]'s learning rates (at the tiny goldens'
    1e-2 one Adam step of a critic on a noise-floor gradient moves the actor phase of the same iteration by per cents:
    test_gpu_ddpg.py's sweep)"""
    g, case = DH.load('tiny_ln_td3_soft')
    h = dict(case['hyper'], lr_actor=1e-4, lr_critic=1e-3)
    h.update(hyper)
    return dict(case, D=D, A=A, ah=list(ah), ch=list(ch), B=B, hyper=h)


def learn(L, case, seed, np_seed):
    np.random.seed(np_seed)            # the action-regularisation noise comes from numpy's global stream
    return dict(L.learn(copy.deepcopy(synthetic.make_ddpg_batch(case['B'], case['D'], case['A'], seed=seed))))


def close(k, x, y):
    scale = float(y.abs().max()) + 1e-30
    d = float((x - y).abs().max())
    print('%s: max |diff| %g at scale %g (bar %g)' % (k, d, scale, 2e-6 * max(scale, 1.0) + 2e-5 * scale))
    assert d <= 2e-6 * max(scale, 1.0) + 2e-5 * scale, '%s: max |diff| %g at scale %g' % (k, d, scale)


def on_the_ln_td3_rows(L):
    a = getattr(L._ws, 'rows_args', None)
    return a is not None and bool(a.ln) and bool(a.second) and bool(a.ln.contents.second)


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
@pytest.mark.parametrize('name', LN_TD3_CASES)
def test_ln_td3_goldens_through_the_row_schedule(name):
    """the helper's own bars: statistics and every element of model, target, model2 and target2, ln* included, at 1e-5;
    the iteration captured in a graph and replayed"""
    L = DH.run_and_check(name, opts=dict(ROWS))
    assert on_the_ln_td3_rows(L) and L._ws.graph is not None
    assert L._schedule(L._ws.key[0], L._ws.key[1]) == 'rows'
    assert L.K.ddpg_rows_ln_second_supported(*L._rows_dims(L._ws.key[1], L._ws.key[0]), L._ws.key[0])
    assert any(k.startswith('critic.ln') for k in L.model2.numpy_params())


# ---- 2. the restatement at the real shape --------------------------------------------------------------------------
def test_ln_td3_rows_match_the_restatement_at_configs2_shape():
    """17 -> 300/200, 400/300, 6 actions, batch 512, action regularisation on, three iterations across a hard update at
    interval 2: statistics and every parameter of the four models at 1e-5 (the bars cfg3_cheetah512 is held to).  The
    restatement is DH.make_oracle's class with DH.make_oracle's arguments and the two TD3 switches, which that helper does
    not pass"""
    case = ln_td3_case(17, 6, (300, 200), (400, 300), 512, target_update_type='hard', target_update_interval=2)
    h = case['hyper']
    mk = lambda seed: ddpg_oracle.make_ddpg_params(17, 6, (300, 200), (400, 300), seed=seed, layernorm=True)  # noqa: E731
    O = ddpg_oracle.OracleDDPGLearner(
        mk(3), gamma=h['gamma'], n_step=h['n_step'], lr_actor=h['lr_actor'], lr_critic=h['lr_critic'],
        clip_critic_gradient=h.get('clip_critic', False), target_update_type='hard', target_update_interval=2,
        tau=h.get('tau', 1e-3), use_double_critic=True, use_action_regularization=True, params2=mk(4), batch_size=512,
        **ddpg_oracle.clip_reg_kwargs(h))
    L = DH.make_learner(case, ROWS)
    assert L.use_action_regularization
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
    assert on_the_ln_td3_rows(L)
    for which, got, want in (('model', L.model, O.model), ('target', L.model_target, O.model_target),
                             ('model2', L.model2, O.model2), ('target2', L.model_target2, O.model_target2)):
        got, want = got.numpy_params(), want.numpy_params()
        assert any('ln' in k for k in got)
        for k in got:
            d = float(np.abs(got[k] - want[k]).max())
            print('%s %s: %g' % (which, k, d))
            assert d <= 1e-5, (which, k, d)


# ---- 3. one iteration, buffer by buffer, against the layer schedule ------------------------------------------------
def one_iteration(case, seed, np_seed=5):
    """a rows learner and a layers learner take one iteration on the same batch and noise.  -> (rows, layers, models as they
    were before the iteration, front): front[k] the layer schedule's CRITIC-phase buffers of critic k -- the first critic's
    workspace serves Q(s, mu(s)) afterwards and the backward scratch is one for both critics and the actor, so they are
    formed again by the same launches from the models before the iteration, against the layer schedule's own y"""
    import torch
    from surreal_amd.learner.ddpg import _grad_views
    rows, layers = DH.make_learner(case, ROWS), DH.make_learner(case)
    before = [copy.deepcopy(layers.model), copy.deepcopy(layers.model2)]
    B, D, A = case['B'], case['D'], case['A']
    b = synthetic.make_ddpg_batch(B, D, A, seed=seed)
    t = lambda v: torch.as_tensor(v, dtype=torch.float32).cuda()  # noqa: E731
    x, acts = t(b['obs']['low_dim']['flat_inputs']), t(b['actions'])
    learn(rows, case, seed, np_seed)
    learn(layers, case, seed, np_seed)
    torch.cuda.synchronize()
    wr, wl = rows._ws, layers._ws
    assert on_the_ln_td3_rows(rows) and getattr(wl, 'rows_args', None) is None
    front = []
    for m, cl in zip(before, wl.critics):
        w, s, q = m.workspace(B, 'cuda'), before[0].backward_workspace(B, 'cuda'), torch.empty(B, device='cuda')
        m.critic_forward(x, acts, w, q)
        g = torch.zeros_like(m.critic_flat)
        dz3 = (2.0 * (cl.q - cl.y)) / B
        m.critic_backward(x, w, s, dz3, _grad_views(g, m.critic.items()))
        front.append(types.SimpleNamespace(w=w, s=s, q=q, dz3=dz3, grads=g))
    torch.cuda.synchronize()
    return rows, layers, before, front


def check_buffers(case, seed, np_seed=5):
    rows, layers, before, front = one_iteration(case, seed, np_seed)
    wr, wl = rows._ws, layers._ws
    c1 = rows.model.c1
    r2, l1, l2 = wr.critics[1], wl.critics[0], wl.critics[1]
    f1, f2 = front
    # the precondition, on the layer side: no LayerNorm row of the case is nearly constant (rstd <= 32) -- such a row
    # amplifies fp32 product rounding by up to 1 / sqrt(eps) = 316, in the layer schedule as in the rows
    for k, r in (('critic ln1', f1.w.cr1), ('critic ln2', f1.w.cr2), ('critic 2 ln1', f2.w.cr1), ('critic 2 ln2', f2.w.cr2),
                 ('critic 2 ln1 (kept)', l2.w.cr1), ('critic 2 ln2 (kept)', l2.w.cr2),
                 ('actor ln1', wl.ar1), ('actor ln2', wl.ar2), ('critic ln1 at mu(s)', wl.cr1), ('critic ln2 at mu(s)', wl.cr2),
                 ('target actor ln1', l1.w_t.ar1), ('target actor ln2', l1.w_t.ar2), ('target critic ln1', l1.w_t.cr1),
                 ('target critic ln2', l1.w_t.cr2), ('target critic 2 ln1', l2.w_t.cr1), ('target critic 2 ln2', l2.w_t.cr2)):
        assert float(r.max()) <= 32.0, (k, float(r.max()))
    pairs = [('q1', wr.q, l1.q), ('q1 (in front)', wr.q, f1.q), ('q2', r2.q, l2.q), ('q2 (in front)', r2.q, f2.q),
             ('q_next (Q1\')', wr.q_next, wl.q_next), ('q_next2 (min)', wr.q_next2, wl.q_next2),
             ('y', wr.y, l1.y), ('y (critic 2)', wr.y, l2.y), ('dz3_1', wr.dz3, f1.dz3), ('dz3_2', r2.dz3, l2.dz3),
             # the first critic's forward pass at (s, a): activations in front of the LayerNorms, outputs, statistics
             ('c_a1', wr.c_a1, f1.w.c_a1), ('xcat', wr.xcat, f1.w.xcat), ('cm1', wr.cm1, f1.w.cm1), ('cr1', wr.cr1, f1.w.cr1),
             ('c_a2', wr.c_a2, f1.w.c_a2), ('c_n2', wr.c_n2, f1.w.c_n2), ('cm2', wr.cm2, f1.w.cm2), ('cr2', wr.cr2, f1.w.cr2),
             # its backward pass
             ('dn2', wr.bw.dn2, f1.s.dn2), ('dz2', wr.dz2, f1.s.dz2), ('dn1 (dxcat[:, :c1])', wr.dxcat[:, :c1], f1.s.dxcat[:, :c1]),
             ('dz1c', wr.bw.dz1c, f1.s.dz1c)]
    # the second critic's forward pass (the layer schedule keeps it: nothing else runs in its workspace) and backward pass
    for k in ('c_a1', 'xcat', 'cm1', 'cr1', 'c_a2', 'c_n2', 'cm2', 'cr2'):
        pairs += [('critic 2 ' + k, getattr(r2.w, k), getattr(l2.w, k)),
                  ('critic 2 %s (in front)' % k, getattr(r2.w, k), getattr(f2.w, k))]
    pairs += [('critic 2 dn2', wr.dn2_2, f2.s.dn2), ('critic 2 dz2', wr.dz2_2, f2.s.dz2),
              ('critic 2 dn1 (dxcat2[:, :c1])', wr.dxcat2[:, :c1], f2.s.dxcat[:, :c1]), ('critic 2 dz1c', wr.dz1c2, f2.s.dz1c),
              # the actor's forward pass, then the actor phase
              ('a1', wr.a1, wl.a1), ('n1', wr.n1, wl.n1), ('am1', wr.am1, wl.am1), ('ar1', wr.ar1, wl.ar1),
              ('a2', wr.a2, wl.a2), ('n2', wr.n2, wl.n2), ('am2', wr.am2, wl.am2), ('ar2', wr.ar2, wl.ar2),
              ('act', wr.act, wl.act), ('q_actor', wr.q_actor, wl.q_actor), ('dz3a', wr.dz3a, wl.dz3a),
              ('dn2a', wr.bw.dn2a, wl.bw.dn2a), ('dz2a', wr.dz2a, wl.dz2a), ('dn1a', wr.bw.dn1a, wl.bw.dn1a),
              ('dz1a', wr.dz1a, wl.dz1a),
              # the three groups' gradients, dgamma and dbeta included (the layer schedule's, and those formed in front)
              ('grads critic', wr.grads_c, l1.grads), ('grads critic (in front)', wr.grads_c, f1.grads),
              ('grads critic 2', r2.grads, l2.grads), ('grads critic 2 (in front)', r2.grads, f2.grads),
              ('grads actor', wr.grads_a, wl.grads_a)]
    for k in ('ln1.W', 'ln1.b', 'ln2.W', 'ln2.b'):
        pairs += [('critic d' + k, wr.gc[k], wl.gc[k]), ('critic 2 d' + k, r2.gv[k], l2.gv[k]), ('actor d' + k, wr.ga[k], wl.ga[k])]
        assert float(wl.gc[k].abs().max()) > 0 and float(l2.gv[k].abs().max()) > 0 and float(wl.ga[k].abs().max()) > 0
    failed = []
    for k, a, bb in pairs:
        try:
            close(k, a, bb)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, failed
    assert int(wr.step[0]) == int(wl.step[0]) == 1
    return rows, layers, before, front


# the batch seed: 91 as in the one-critic sweep; the smallest shape swaps it -- with four features a row whose ReLUs are all
# off is constant (rstd = 316) for most batches, SMALL_SEED is one for which the layer schedule has none in any of the six
# networks (searched with the CPU double, the noise seed fixed at 5)
SMALL_SEED = 263
SWEEP_SEEDS = [SMALL_SEED, 91, 91, 91, 91]


@pytest.mark.parametrize('shape,seed', list(zip(LC.SWEEP, SWEEP_SEEDS)))
def test_ln_td3_row_launches_fill_the_layer_schedules_buffers(shape, seed):
    D, A, ah, ch, B = shape
    case = ln_td3_case(D, A, ah, ch, B, target_update_type='soft', tau=0.1)
    dims = (D, A, ah[0], ah[1], ch[0], ch[1])
    rows, layers, _, _ = check_buffers(case, seed)
    assert rows.K.ddpg_rows_ln_second_supported(*dims, B)
    learn(rows, case, seed + 1, 6)                 # (the update launches' copies, twice)
    packed_copies_are_current(rows)


# ---- 4. the second critic's LayerNorms, bit for bit ----------------------------------------------------------------
@pytest.mark.parametrize('shape', [LC.SWEEP[1], LC.SWEEP[2]])
def test_second_critics_ln_rules_have_the_bits_of_the_layernorm_kernels(shape):
    """forward: smx_layernorm_forward_f32 on the rows' own pre-LayerNorm buffers of the second critic gives its LayerNorm
    outputs, means and rstds, torch.equal; backward: smx_layernorm_backward_f32 (relu_mask) on the rows' own dn,
    pre-LayerNorm buffer, mean and rstd gives the rows' dz bit for bit.  The parameter sums take another row order: `close`.
    (The first critic's and the actor's are held this way by test_gpu_ddpg_ln_rows.py, in the one-critic chain; here the
    first critic's once more, in TD3's.)"""
    import torch
    D, A, ah, ch, B = shape
    case = ln_td3_case(D, A, ah, ch, B, target_update_type='soft', tau=0.1)
    rows, layers, before, front = one_iteration(case, 91)
    K, wr, eps = rows.K, rows._ws, rows.model.ln_eps
    c1 = rows.model.c1
    r2 = wr.critics[1]
    cp, cp2 = before[0].critic, before[1].critic          # the parameters the iteration ran with
    e = lambda *s: torch.empty(*s, device='cuda')  # noqa: E731
    for k, pre, g, b, out, mean, rstd in (
            ('critic 2 ln1', r2.w.c_a1, cp2['ln1.W'], cp2['ln1.b'], r2.w.xcat[:, :c1], r2.w.cm1, r2.w.cr1),
            ('critic 2 ln2', r2.w.c_a2, cp2['ln2.W'], cp2['ln2.b'], r2.w.c_n2, r2.w.cm2, r2.w.cr2),
            ('critic ln1', wr.c_a1, cp['ln1.W'], cp['ln1.b'], wr.xcat[:, :c1], wr.cm1, wr.cr1),
            ('critic ln2', wr.c_a2, cp['ln2.W'], cp['ln2.b'], wr.c_n2, wr.cm2, wr.cr2)):
        y, m, rs = e(*pre.shape), e(B), e(B)
        K.layernorm_forward(pre, g, b, eps, y, m, rs)
        torch.cuda.synchronize()
        assert float(pre.abs().max()) > 0
        assert torch.equal(y, out) and torch.equal(m, mean) and torch.equal(rs, rstd), k
    ws = e(max(K.layernorm_backward_ws_floats(B, F) for F in (ch[0], ch[1])))
    for k, dn, pre, mean, rstd, g, dz, grads, name in (
            ('critic 2 ln2', wr.dn2_2, r2.w.c_a2, r2.w.cm2, r2.w.cr2, cp2['ln2.W'], wr.dz2_2, r2.gv, 'ln2'),
            ('critic 2 ln1', wr.dxcat2[:, :c1], r2.w.c_a1, r2.w.cm1, r2.w.cr1, cp2['ln1.W'], wr.dz1c2, r2.gv, 'ln1'),
            ('critic ln2', wr.bw.dn2, wr.c_a2, wr.cm2, wr.cr2, cp['ln2.W'], wr.dz2, wr.gc, 'ln2'),
            ('critic ln1', wr.dxcat[:, :c1], wr.c_a1, wr.cm1, wr.cr1, cp['ln1.W'], wr.bw.dz1c, wr.gc, 'ln1')):
        F = pre.shape[1]
        dx, dg, db = e(B, F), e(F), e(F)
        K.layernorm_backward(dn, pre, mean, rstd, g, dx, dg, db, ws, relu_mask=True)
        torch.cuda.synchronize()
        assert float(dn.abs().max()) > 0
        assert torch.equal(dx, dz), k
        close(k + ' dgamma', grads[name + '.W'], dg)
        close(k + ' dbeta', grads[name + '.b'], db)


# ---- 5. y and the noise --------------------------------------------------------------------------------------------
def test_y_is_the_bellman_target_of_the_smaller_target_critic_and_the_noise_reaches_the_second_alone():
    """on a batch where each target critic is the smaller one on some row, y is bitwise r + (gamma^n min(Q1', Q2')) (1 - done)
    with the min as the kernel leaves it (q_next2 = min(q_next, Q2'); r + t is monotone in Q', so the min of the two
    targets the kernel forms is the target of the min); another noise moves q_next2 and leaves q_next = Q1' bit-identical"""
    import torch
    case = ln_td3_case(17, 6, (300, 200), (400, 300), 37, target_update_type='soft', tau=0.1)
    a, b = DH.make_learner(case, ROWS), DH.make_learner(case, ROWS)
    learn(a, case, 91, 5)
    learn(b, case, 91, 6)
    torch.cuda.synchronize()
    wa, wb = a._ws, b._ws
    assert on_the_ln_td3_rows(a) and on_the_ln_td3_rows(b)
    assert a.use_action_regularization and not torch.equal(wa.s_noise, wb.s_noise)
    for ws in (wa, wb):
        first = ws.q_next2 == ws.q_next                 # rows on which the first target critic is the smaller one
        assert bool(first.any()) and bool((~first).any())
        assert bool((ws.q_next2 <= ws.q_next).all())
        gamma_n = torch.tensor(pow(a.discount_factor, a.n_step), dtype=torch.float32, device='cuda')
        t = (gamma_n * ws.q_next2) * (1.0 - ws.s_done)
        assert float(ws.y.abs().max()) > 0 and torch.equal(ws.y, ws.s_rew + t)
    assert torch.equal(wa.q_next, wb.q_next) and float(wa.q_next.abs().max()) > 0
    assert not torch.equal(wa.q_next2, wb.q_next2)


# ---- 6. the packed copies ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('update', ['soft', 'hard'])
def test_packed_copies_equal_a_fresh_pack_after_three_iterations(update):
    """rows_packed and rows_packed2 are kept current by the gradient-and-step launches alone (models, targets, the
    transposed blocks): after three iterations -- across a hard update at interval 2, or with soft updates -- a fresh pack
    of all six networks changes no bit"""
    case = ln_td3_case(17, 6, (304, 204), (404, 300), 37, target_update_type=update, target_update_interval=2, tau=0.1)
    L = DH.make_learner(case, ROWS)
    for it in range(3):
        learn(L, case, 10 + it, 1000 + it)
    assert on_the_ln_td3_rows(L)
    packed_copies_are_current(L)


# ---- 7. the other three cells are untouched ------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['tiny_hard', 'tiny_td3_hard', 'tiny_ln_hard'])
def test_the_other_row_routes_leave_the_same_bytes(name):
    """plain, TD3 and one-critic LayerNorm learners under the flag run with the second LayerNorm part NULL: the chains'
    five earlier instantiations, whose bytes a second learner of the same configuration reproduces in every workspace
    buffer and parameter"""
    import torch
    g, case = DH.load(name)
    a, b = DH.make_learner(case, ROWS), DH.make_learner(case, ROWS)
    for L in (a, b):
        for it in range(2):
            learn(L, case, 10 + it, 1000 + it)
    torch.cuda.synchronize()
    assert a._schedule(case['B'], case['D']) == b._schedule(case['B'], case['D']) == 'rows'
    for L in (a, b):
        args = L._ws.rows_args
        assert args is not None and bool(args.ln) == L.use_layernorm and bool(args.second) == L.use_double_critic
        assert not (bool(args.ln) and bool(args.ln.contents.second))
    wa, wb = a._ws, b._ws
    c1 = a.model.c1
    names = ['xcat', 'q', 'q_next', 'y', 'dz3', 'dz2', 'act', 'q_actor', 'dz3a', 'dz2a', 'dz1a', 'grads_c', 'grads_a', 'stats',
             'rows_packed']
    names += ['c_a1', 'cm1', 'cr1', 'c_a2', 'c_n2', 'cm2', 'cr2', 'a1', 'n1', 'am1', 'ar1', 'a2', 'n2', 'am2',
              'ar2'] if a.use_layernorm else ['h2c', 'h1a', 'h2a']
    names += ['dz2_2', 'dxcat2', 'q_next2', 'rows_packed2'] if a.use_double_critic else []
    pairs = [(k, getattr(wa, k), getattr(wb, k)) for k in names] + [('dxcat[:, :c1]', wa.dxcat[:, :c1], wb.dxcat[:, :c1])]
    if a.use_layernorm:
        pairs += [('bw.' + k, getattr(wa.bw, k), getattr(wb.bw, k)) for k in ('dn2', 'dz1c', 'dn2a', 'dn1a')]
    if a.use_double_critic:
        ca, cb = wa.critics[1], wb.critics[1]
        pairs += [('critic 2 ' + k, x, y) for k, x, y in (('q', ca.q, cb.q), ('dz3', ca.dz3, cb.dz3), ('grads', ca.grads, cb.grads),
                                                         ('stats', ca.stats, cb.stats), ('xcat', ca.w.xcat, cb.w.xcat),
                                                         ('h2c', ca.w.h2c, cb.w.h2c))]
    for k, x, y in pairs:
        assert float(x.abs().max()) > 0 and torch.equal(x, y), k
    models = [(a.model, b.model), (a.model_target, b.model_target)]
    if a.use_double_critic:
        models += [(a.model2, b.model2), (a.model_target2, b.model_target2)]
    for ma, mb in models:
        assert torch.equal(ma.critic_flat, mb.critic_flat)
        assert ma.actor_flat is None or torch.equal(ma.actor_flat, mb.actor_flat)


def test_ln_without_its_second_part_is_refused_beside_a_second_critic():
    """a LayerNorm TD3 block whose `ln` has lost its second part is refused by every entry, smx_ddpg_rows_critic_td3_f32
    first, before anything is launched: no buffer of the iteration changes.  With the part back the same block runs"""
    import ctypes
    import torch
    from surreal_amd import _lib
    case = ln_td3_case(17, 6, (300, 200), (400, 300), 37, target_update_type='soft', tau=0.1)
    L = DH.make_learner(case, ROWS)
    learn(L, case, 91, 5)
    torch.cuda.synchronize()
    ws = L._ws
    args = ws.rows_args
    assert on_the_ln_td3_rows(L)
    part = args._refs_ln2[0]                              # (the structure itself: a pointer read from the field aliases the field)
    watched = [ws.q, ws.q_next, ws.q_next2, ws.y, ws.critics[1].q, ws.dz2_2, ws.dn2_2, ws.dz1c2, ws.step, ws.act, ws.q_actor,
               ws.rows_packed2, L.model2.critic_flat, L.model.critic_flat]
    before = [t.clone() for t in watched]
    args.ln.contents.second = None
    try:
        with pytest.raises(_lib.SmxError):
            L.K.ddpg_rows_critic_td3(args)
        with pytest.raises(_lib.SmxError):
            L.K.ddpg_rows_critic(args)                    # (`second` together with `ln`: refused with or without the part)
        with pytest.raises(_lib.SmxError):
            L.K.ddpg_rows_actor(args)
        with pytest.raises(_lib.SmxError):
            L.K.ddpg_rows_pack_second(args)
    finally:
        args.ln.contents.second = ctypes.pointer(part)
    with pytest.raises(_lib.SmxError):
        L.K.ddpg_rows_critic(args)
    torch.cuda.synchronize()
    for t, t0 in zip(watched, before):
        assert torch.equal(t, t0)
    L.K.ddpg_rows_critic_td3(args)                        # the whole block: the chain runs (and counts the step)
    torch.cuda.synchronize()
    assert int(ws.step[0]) == int(before[8][0]) + 1
