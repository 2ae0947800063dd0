"""GPU tier (-m gpu): every Adam entry point against torch.optim.Adam(weight_decay=wd) on the CPU, with the clip the
reference puts in front of it -- clip_grad_value_ for the DDPG paths, clip_grad_norm_ for the PPO paths -- over several
consecutive steps from the same state: theta, exp_avg and exp_avg_sq after every step at 1e-6 (as
test_clip_adam_matches_torch_optim).  Weight decay up to a value that dominates the gradient, value clips that bind on
none / about half / all of the elements, a norm clip that binds or not, sizes around the 256-thread blocks, a late step
count, the learning rate and step count changed between steps where the kernel reads them from device memory, and
gradients with a NaN or an inf element (the expected result is what torch makes of the same inputs).  The PPO steps that
keep the fused epoch kernels' packed copy current, and the DDPG row-schedule updates, must leave their fragment-order copies
equal, bit for bit, to a fresh pack."""
import copy

import numpy as np
import pytest
import torch

import ddpg_helpers as DH
from surreal_amd import _lib as L
from surreal_amd import synthetic

pytestmark = pytest.mark.gpu

ATOL, RTOL = 1e-6, 1e-6
SIZES = [1, 255, 256, 257, 100003]
WDS = [0.0, 1e-2, 0.5]
# (step, lr): the first three steps, then a late one (the bias corrections near 1), lr changed every step
SCHEDULE = [(1, 1e-3), (2, 3e-3), (3, 5e-4), (5000, 2e-3)]
SCALE = 1e-2


@pytest.fixture(scope='module')
def K():
    from surreal_amd.kernels import HipKernels
    return HipKernels()


def close(a, b, msg):
    np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), atol=ATOL, rtol=RTOL, err_msg=msg)


class TorchAdam(object):
    """torch.optim.Adam on one CPU fp32 parameter, started from a given state, preceded by the reference's clip"""

    def __init__(self, theta, wd, m=None, v=None, step=0):
        self.p = torch.nn.Parameter(theta.detach().cpu().clone())
        self.opt = torch.optim.Adam([self.p], lr=1e-3, weight_decay=wd)
        if m is not None:
            self.opt.state[self.p] = {'step': torch.tensor(float(step)), 'exp_avg': m.detach().cpu().clone(),
                                      'exp_avg_sq': v.detach().cpu().clone()}

    def step(self, grad, step, lr, value_clip=0.0, max_norm=0.0):
        """returns the total norm clip_grad_norm_ saw (None without a norm clip)"""
        self.p.grad = grad.detach().cpu().clone()
        norm = None
        if value_clip > 0:
            torch.nn.utils.clip_grad_value_([self.p], value_clip)
        if max_norm > 0:
            norm = float(torch.nn.utils.clip_grad_norm_([self.p], max_norm))
        st = self.opt.state.get(self.p)
        if st:                                   # the step count the kernel is given (a jump to a late step included)
            st['step'] = torch.tensor(float(step - 1))
        else:
            assert step == 1
        self.opt.param_groups[0]['lr'] = lr
        self.opt.step()
        return norm

    def check(self, theta, m, v, msg):
        st = self.opt.state[self.p]
        close(theta, self.p.detach(), msg + ' theta')
        close(m, st['exp_avg'], msg + ' exp_avg')
        close(v, st['exp_avg_sq'], msg + ' exp_avg_sq')


def make_grad(g, n, nonfinite=None):
    """|g| uniform in [0.5, 1.5] * SCALE with a random sign: a value clip at SCALE binds on about half the elements, one
    at SCALE / 4 on all of them"""
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    grad = sign * (0.5 + torch.rand(n, generator=g)) * SCALE
    if nonfinite == 'nan':
        grad[n // 2] = float('nan')
    elif nonfinite == 'inf':
        grad[n // 3] = float('inf')
        grad[-1] = -float('inf')
    return grad


VALUE_CLIPS = {'off': 0.0, 'half': SCALE, 'all': SCALE / 4}


# ---------------------------------------------------------------------------------------------------------------
# DDPG: smx_adam_step_f32 (host-fed step and lr) and smx_adam_step_dev_f32 (both read on the device)
# ---------------------------------------------------------------------------------------------------------------
def _run_ddpg_adam(K, which, n, wd, clip, nonfinite=None, schedule=SCHEDULE, seed=0):
    g = torch.Generator().manual_seed(seed + n)
    theta0 = torch.randn(n, generator=g)
    th, m, v = theta0.cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()
    ref = TorchAdam(theta0, wd)
    lr_d, step_d = torch.zeros(1).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
    for step, lr in schedule:
        grad = make_grad(g, n, nonfinite)
        ref.step(grad, step, lr, value_clip=clip)
        if which == 'adam_step':
            K.adam_step(th, grad.cuda(), m, v, lr, step, weight_decay=wd, clip_value=clip)
        else:
            lr_d.fill_(lr)
            step_d.fill_(step)
            K.adam_step_dev(th, grad.cuda(), m, v, lr_d, step_d, weight_decay=wd, clip_value=clip)
        ref.check(th, m, v, '%s n=%d wd=%g clip=%g step %d' % (which, n, wd, clip, step))
    return th


@pytest.mark.parametrize('which', ['adam_step', 'adam_step_dev'])
@pytest.mark.parametrize('clip', list(VALUE_CLIPS))
@pytest.mark.parametrize('wd', WDS)
@pytest.mark.parametrize('n', SIZES)
def test_ddpg_adam_matches_torch(K, which, n, wd, clip):
    _run_ddpg_adam(K, which, n, wd, VALUE_CLIPS[clip])


@pytest.mark.parametrize('which', ['adam_step', 'adam_step_dev'])
@pytest.mark.parametrize('clip', list(VALUE_CLIPS))
@pytest.mark.parametrize('nonfinite', ['nan', 'inf'])
def test_ddpg_adam_nonfinite_gradient_as_torch(K, which, nonfinite, clip):
    """torch.clamp passes a NaN through (the element's parameter goes NaN) and clamps an inf to the clip"""
    th = _run_ddpg_adam(K, which, 257, 1e-2, VALUE_CLIPS[clip], nonfinite, schedule=SCHEDULE[:2])
    if nonfinite == 'nan':
        assert torch.isnan(th[257 // 2]).item()


# ---------------------------------------------------------------------------------------------------------------
# PPO: smx_clip_adam_step_f32 / _group_f32 / _pair_f32 (clip_grad_norm_ + Adam, step, lr, max norm, decay in the
# device-resident control block)
# ---------------------------------------------------------------------------------------------------------------
def _ctrl(lr, step, max_norm, wd, which=0, ctrl=None):
    """the group's words of the control block (smx_ppo_ctrl_t): lr, max norm, decay, Adam step"""
    ctrl = torch.zeros(L.CTRL_WORDS) if ctrl is None else ctrl
    ctrl[L.C_LR_CRITIC if which else L.C_LR_ACTOR] = lr
    ctrl[L.C_CRITIC_MAX_NORM if which else L.C_ACTOR_MAX_NORM] = max_norm
    ctrl[L.C_CRITIC_WD if which else L.C_ACTOR_WD] = wd
    ctrl.view(torch.int32)[L.C_STEP_CRITIC if which else L.C_STEP_ACTOR] = step
    return ctrl


def _norm_clip(mode, n):
    """off: max_norm 0 (clip_*_gradient False); loose: above the gradient's norm; tight: well below it"""
    rms = SCALE * np.sqrt(13.0 / 12.0)            # E|g|^2 of make_grad
    return {'off': 0.0, 'loose': 10.0 * rms * np.sqrt(n), 'tight': 0.3 * rms * np.sqrt(n)}[mode]


def _run_clip_adam(K, n, wd, mode, which=0, nonfinite=None, schedule=SCHEDULE):
    g = torch.Generator().manual_seed(100 + n)
    theta0 = torch.randn(n, generator=g)
    th, m, v = theta0.cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()
    ref = TorchAdam(theta0, wd)
    max_norm = _norm_clip(mode, n)
    nb = K.sumsq_blocks(n)
    part, gn = torch.zeros(nb).cuda(), torch.full((1,), -1.0).cuda()
    ctrl = torch.zeros(L.CTRL_WORDS).cuda()
    for step, lr in schedule:
        grad = make_grad(g, n, nonfinite)
        tn = ref.step(grad, step, lr, max_norm=max_norm)
        ctrl.copy_(_ctrl(lr, step, max_norm, wd, which))
        gd = grad.cuda()
        K.sumsq_partials(gd, part)
        K.clip_adam(th, gd, m, v, part, nb, ctrl, which, True, gn)
        msg = 'clip_adam n=%d wd=%g norm clip %s step %d' % (n, wd, mode, step)
        if tn is not None:
            np.testing.assert_allclose(float(gn), tn, rtol=1e-5, err_msg=msg + ' grad norm')
        ref.check(th, m, v, msg)
    return th


@pytest.mark.parametrize('mode', ['off', 'loose', 'tight'])
@pytest.mark.parametrize('wd', WDS)
@pytest.mark.parametrize('n', SIZES)
def test_clip_adam_with_decay_matches_torch(K, n, wd, mode):
    _run_clip_adam(K, n, wd, mode, which=n % 2)      # both groups' words of the control block


@pytest.mark.parametrize('mode', ['off', 'tight'])
@pytest.mark.parametrize('nonfinite', ['nan', 'inf'])
def test_clip_adam_nonfinite_gradient_as_torch(K, nonfinite, mode):
    """clip_grad_norm_ of a gradient with a NaN: the norm is NaN and so is every parameter after the step (torch clamps
    the coefficient with torch.clamp, which keeps NaN); with an inf the coefficient is 0 and the inf element goes NaN"""
    th = _run_clip_adam(K, 257, 1e-2, mode, nonfinite=nonfinite, schedule=SCHEDULE[:2])
    if nonfinite == 'nan' and mode == 'tight':
        assert bool(torch.isnan(th).all())


def _packed_groups(K, seed):
    """an actor and a critic MLP (cfg-2 shapes) at an offset inside their optimiser buffers, as in the PPO learner"""
    from surreal_amd.model.ppo_net import Mlp3Params
    g = torch.Generator().manual_seed(seed)
    out = []
    for OUT in (6, 1):
        cnt = Mlp3Params.count(17, 300, 200, OUT)
        flat = (torch.randn(cnt + 9, generator=g) * 0.05).cuda()
        net = Mlp3Params(flat, 3, 17, 300, 200, OUT)
        packed = torch.zeros(max(K.epoch_packed_numel(net), net.numel)).cuda()
        K.epoch_pack([(net, packed)])
        out.append((flat, net, packed))
    return g, out


@pytest.mark.parametrize('pair', [False, True])
def test_clip_adam_decay_keeps_the_packed_copies_current(K, pair):
    """decayed, norm-clipped steps through the group / pair entry points with the fused epoch kernels' packed copy: every
    step against torch, and the packed copies afterwards bit for bit what a fresh epoch_pack gives"""
    g, groups = _packed_groups(K, 7)
    wds, lrs = (0.5, 1e-2), (1e-3, 2e-3)
    refs = [TorchAdam(flat, wd) for (flat, _, _), wd in zip(groups, wds)]
    state = [(torch.zeros_like(flat), torch.zeros_like(flat)) for flat, _, _ in groups]
    parts = [torch.zeros(K.sumsq_blocks(flat.numel())).cuda() for flat, _, _ in groups]
    gns = [torch.zeros(1).cuda(), torch.zeros(1).cuda()]
    for step, lr in SCHEDULE:
        ctrl = None
        for k in range(2):
            ctrl = _ctrl(lrs[k] * lr / 1e-3, step, _norm_clip('tight', groups[k][0].numel()), wds[k], k, ctrl)
        ctrl = ctrl.cuda()
        grads = [make_grad(g, flat.numel()) for flat, _, _ in groups]
        for k in range(2):
            refs[k].step(grads[k], step, lrs[k] * lr / 1e-3, max_norm=_norm_clip('tight', groups[k][0].numel()))
            K.sumsq_partials(grads[k].cuda(), parts[k])
        gd = [gr.cuda() for gr in grads]
        if pair:
            K.clip_adam_pair(*[(groups[k][0], gd[k], state[k][0], state[k][1], parts[k], parts[k].numel(), True, gns[k])
                               for k in range(2)], ctrl, pack=tuple((groups[k][1], groups[k][2]) for k in range(2)))
        else:
            for k in range(2):
                K.clip_adam(groups[k][0], gd[k], state[k][0], state[k][1], parts[k], parts[k].numel(), ctrl, k, True,
                            gns[k], pack=(groups[k][1], groups[k][2]))
        for k in range(2):
            refs[k].check(groups[k][0], *state[k], 'group %d step %d' % (k, step))
    torch.cuda.synchronize()
    for flat, net, packed in groups:
        fresh = torch.zeros_like(packed)
        K.epoch_pack([(net, fresh)])
        torch.cuda.synchronize()
        assert torch.equal(packed, fresh)


# ---------------------------------------------------------------------------------------------------------------
# target updates
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tau', [0.05, 1.0])
@pytest.mark.parametrize('n', SIZES)
def test_soft_update_matches_torch(K, n, tau):
    g = torch.Generator().manual_seed(n)
    tgt, src = torch.randn(n, generator=g), torch.randn(n, generator=g)
    want = src.clone() if tau >= 1.0 else tgt * (1.0 - tau) + src * tau        # torchx Module.soft_update
    td = tgt.cuda()
    K.soft_update(td, src.cuda(), tau)
    close(td, want, 'soft_update n=%d tau=%g' % (n, tau))


@pytest.mark.parametrize('n', SIZES)
def test_hard_update_every_copies_on_the_interval(K, n):
    g = torch.Generator().manual_seed(n)
    src = torch.randn(n, generator=g).cuda()
    for step, interval in ((1, 2), (2, 2), (3, 2), (499, 500), (500, 500), (1000, 500), (7, 1)):
        tgt0 = torch.randn(n, generator=g).cuda()
        tgt = tgt0.clone()
        K.hard_update_every(tgt, src, torch.tensor([step], dtype=torch.int32).cuda(), interval)
        assert torch.equal(tgt, src if step % interval == 0 else tgt0), (n, step, interval)


# ---------------------------------------------------------------------------------------------------------------
# DDPG row schedule: smx_ddpg_rows_update_f32 (given gradients) and smx_ddpg_rows_wgrad_update_f32 (forms them)
# ---------------------------------------------------------------------------------------------------------------
def _rows_learner(name):
    g, case = DH.load(name)
    Lr = DH.make_learner(case, {'ddpg_row_schedule': True})
    Lr.learn(copy.deepcopy(synthetic.make_ddpg_batch(case['B'], case['D'], case['A'], seed=10)))
    assert getattr(Lr._ws, 'rows_args', None) is not None
    torch.cuda.synchronize()
    return Lr


def _group(Lr, group):
    m, mt = Lr.model, Lr.model_target
    if group == 'critic':
        return m.critic_flat, mt.critic_flat, Lr.critic_exp_avg, Lr.critic_exp_avg_sq, Lr._ws.grads_c
    return m.actor_flat, mt.actor_flat, Lr.actor_exp_avg, Lr.actor_exp_avg_sq, Lr._ws.grads_a


def _set_state(Lr, group, gen):
    """a known state -- parameters, target, moments -- written into the learner's buffers, the packed copy refreshed"""
    theta, tgt, m, v, _ = _group(Lr, group)
    n = theta.numel()
    theta.copy_(theta + 0.01 * torch.randn(n, generator=gen).cuda())
    tgt.copy_(theta + 0.01 * torch.randn(n, generator=gen).cuda())
    m.copy_(1e-3 * torch.randn(n, generator=gen).cuda())
    v.copy_(1e-5 * torch.rand(n, generator=gen).cuda())
    Lr.K.ddpg_rows_pack(Lr._ws.rows_args)
    torch.cuda.synchronize()


@pytest.mark.parametrize('wgrad', [False, True])
@pytest.mark.parametrize('clip', list(VALUE_CLIPS))
@pytest.mark.parametrize('wd', WDS)
@pytest.mark.parametrize('name,group', [('tiny_hard', 'critic'), ('tiny_hard', 'actor'), ('mid_reg_clip', 'critic')])
def test_ddpg_rows_update_matches_torch(name, group, wd, clip, wgrad):
    """the row schedule's update launches on a learner's own buffers, from a known state: theta, moments, target (hard
    every 2 steps, or soft) against torch after every step, the step count and lr read from device memory and changed
    between steps, and the fragment-order copies afterwards bit for bit a fresh ddpg_rows_pack.  wgrad: the launch
    forms the gradient from the last iteration's activations and writes it out -- the reference is stepped with it"""
    Lr = _rows_learner(name)
    K = Lr.K
    gen = torch.Generator().manual_seed(3)
    _set_state(Lr, group, gen)
    theta, tgt, m, v, grads = _group(Lr, group)
    n = theta.numel()
    hard = name == 'tiny_hard'
    tau, interval = (0.0, 2) if hard else (0.05, 0)
    lr_d, step_d = torch.zeros(1).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
    ref = TorchAdam(theta, wd, m, v, step=0)
    want_tgt = tgt.cpu().clone()
    if wgrad:                 # the gradient the launch forms: to place the clip, and the same every launch
        g_fixed = None
    for step, lr in [(1, 1e-3), (2, 3e-3), (3, 5e-4), (4, 2e-3), (5000, 1e-3)]:
        if wgrad:
            if g_fixed is None:
                save = [t.clone() for t in (theta, tgt, m, v)]
                lr_d.fill_(lr); step_d.fill_(step)
                K.ddpg_rows_update(Lr._ws.rows_args, group, theta, grads, m, v, lr_d, step_d, 0.0, 0.0, target=tgt,
                                   tau=tau, interval=interval, wgrad=True)
                torch.cuda.synchronize()
                g_fixed = grads.cpu().clone()
                for t, s in zip((theta, tgt, m, v), save):
                    t.copy_(s)
                K.ddpg_rows_pack(Lr._ws.rows_args)
                scale = float(g_fixed.abs().median())
            grad = g_fixed
        else:
            grad = make_grad(gen, n)
            scale = SCALE
        c = {'off': 0.0, 'half': scale, 'all': 0.0}[clip] if wgrad else VALUE_CLIPS[clip]
        if wgrad and clip == 'all':
            c = 0.25 * float(g_fixed.abs()[g_fixed != 0].min())
        ref.step(grad, step, lr, value_clip=c)
        lr_d.fill_(lr)
        step_d.fill_(step)
        if not wgrad:
            grads.copy_(grad)
        K.ddpg_rows_update(Lr._ws.rows_args, group, theta, grads, m, v, lr_d, step_d, wd, c, target=tgt, tau=tau,
                           interval=interval, wgrad=wgrad)
        msg = '%s %s wd=%g clip=%s wgrad=%s step %d' % (name, group, wd, clip, wgrad, step)
        if wgrad:
            assert torch.equal(grads.cpu(), g_fixed), msg
        ref.check(theta, m, v, msg)
        pn = ref.p.detach()
        if hard:
            if step % interval == 0:
                want_tgt = pn.clone()
        else:
            want_tgt = want_tgt * (1.0 - tau) + pn * tau
        close(tgt, want_tgt, msg + ' target')
        want_tgt = tgt.cpu().clone()                       # (each step's target update from the kernel's own state)
    torch.cuda.synchronize()
    kept = Lr._ws.rows_packed.clone()
    K.ddpg_rows_pack(Lr._ws.rows_args)
    torch.cuda.synchronize()
    assert torch.equal(kept, Lr._ws.rows_packed)


@pytest.mark.parametrize('nonfinite', ['nan', 'inf'])
def test_ddpg_rows_update_nonfinite_gradient_as_torch(nonfinite):
    Lr = _rows_learner('tiny_hard')
    gen = torch.Generator().manual_seed(4)
    _set_state(Lr, 'critic', gen)
    theta, tgt, m, v, grads = _group(Lr, 'critic')
    ref = TorchAdam(theta, 1e-2, m, v, step=0)
    lr_d, step_d = torch.full((1,), 1e-3).cuda(), torch.ones(1, dtype=torch.int32).cuda()
    grad = make_grad(gen, theta.numel(), nonfinite)
    ref.step(grad, 1, 1e-3, value_clip=SCALE)
    grads.copy_(grad)
    Lr.K.ddpg_rows_update(Lr._ws.rows_args, 'critic', theta, grads, m, v, lr_d, step_d, 1e-2, SCALE, target=tgt,
                          interval=2)
    ref.check(theta, m, v, 'rows update, %s gradient' % nonfinite)
    assert bool(torch.isnan(theta).any()) == (nonfinite == 'nan')
