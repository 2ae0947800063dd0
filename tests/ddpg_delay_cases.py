"""What the tests of TD3's delayed policy updates (learner_config.algo.network.policy_delay = d) share: the CPU restatement
of an iteration under a delay on top of oracle/ddpg_oracle.py's, a learner builder that sets the key, the torch-CPU double of
the row schedule's new launches (the critic-only chains, the tail in front of a delayed learner's actor step), and the run
that holds a learner against the restatement.

Iteration k = 1, 2, ... updates the critic(s) always; the actor -- Adam counting ITS updates, k / d -- and every target only
when k % d == 0.  A critic-only iteration reports actor_loss = -mean of Q(s, mu(s)) as the last actor update left it (zeros
before the first one)."""
import numpy as np
import torch
import torch.nn as nn

import ddpg_helpers as DH
import ddpg_oracle
from ddpg_ln_td3_rows_cases import LnTd3RowsCpuKernels
from surreal_amd import synthetic

# the four soft-update goldens' shapes and hyper-parameters (read from their case_json), and the camera one
LOW_CASES = ['tiny_soft_clipcritic', 'tiny_double_soft', 'ln_soft_clipcritic', 'tiny_ln_td3_soft']
PIXEL_CASE = 'tiny_pixel_td3_soft'
ITERS = 7                     # d = 2: updates at 2, 4, 6; d = 3: at 3, 6 -- both end on a critic-only iteration
DELAYS = (2, 3)
STAT_TOL = 1e-5               # absolute and relative


# Parameter bounds of the GPU tier: ddpg_helpers' (1e-5; the camera case's own entry) unless the SAME case at d = 1 -- the
# arithmetic of the learner without the key -- leaves 1e-5 over these 7 iterations on an MI355X; then twice that figure, at
# most 1e-4 (profiles/ddpg_policy_delay_errors.txt has both figures of every case)
GPU_PARAM_ATOL = {}


def gpu_param_atol(name):
    return GPU_PARAM_ATOL.get(name, DH.PARAM_ATOL.get(name, DH.PARAM_ATOL_DEFAULT))


def schedules(name):
    """the session options of every schedule the case can take: rows, layers -- and levels for the plain case"""
    h = DH.load(name)[1]['hyper']
    if DH.load(name)[1].get('pixel'):
        return {'layers': {}}
    out = {'rows': {'ddpg_row_schedule': True}, 'layers': {'ddpg_row_schedule': False, 'ddpg_level_schedule': False}}
    if not h.get('double_critic') and not h.get('layernorm'):
        out['levels'] = {'ddpg_row_schedule': False}
    return out


def matrix():
    """(case, schedule, d) of the whole matrix"""
    return [(n, s, d) for n in LOW_CASES + [PIXEL_CASE] for s in schedules(n) for d in DELAYS]


class DelayedOracle(ddpg_oracle.OracleDDPGLearner):
    """OracleDDPGLearner.optimize with the policy update delayed: its own iteration count; the actor optimiser steps and
    _target_update runs on update iterations only"""

    def __init__(self, *a, policy_delay=1, **kw):
        super().__init__(*a, **kw)
        self.policy_delay, self.k, self.kept_q = int(policy_delay), 0, None

    def optimize(self, obs, actions, rewards, obs_next, done):
        m, mt = self.model, self.model_target
        self.k += 1
        obs_next_raw, obs_raw = obs_next, obs
        obs_next = mt.forward_perception(obs_next)
        mu_next = mt.forward_actor(obs_next)
        y = rewards + pow(self.gamma, self.n_step) * mt.forward_critic(obs_next, mu_next) * (1.0 - done)
        if self.use_action_regularization:           # drawn on every iteration: y2 needs it
            noise = np.clip(np.random.normal(0, 0.2, size=(self.batch_size, mu_next.shape[1])), -0.5, 0.5)
            mu_next = (mu_next + torch.tensor(noise, dtype=torch.float32)).clamp(-1, 1)
        if self.use_double_critic:
            t2 = self.model_target2
            q2n = t2.forward_critic(t2.forward_perception(obs_next_raw), mu_next)
            y = torch.min(y, rewards + pow(self.gamma, self.n_step) * q2n * (1.0 - done))
        y = y.detach()
        obs = m.forward_perception(obs_raw)
        q = m.forward_critic(obs, actions.detach())
        q2 = self.model2.forward_critic(self.model2.forward_perception(obs_raw), actions.detach()) \
            if self.use_double_critic else None
        steps = [(m, q, self.critic_optim)] + ([(self.model2, q2, self.critic_optim2)] if self.use_double_critic else [])
        for model, qk, optim in steps:
            for p in model.critic_params():
                p.grad = None
            critic_loss = self.critic_criterion(qk, y)
            critic_loss.backward()
            if self.clip_critic_gradient:
                nn.utils.clip_grad_value_(model.critic_net_params(), self.critic_clip)
            optim.step()
        update = self.k % self.policy_delay == 0
        if update:
            for p in m.actor_params():
                p.grad = None
            q_mu = m.forward_critic(obs.detach(), m.forward_actor(obs.detach()))
            actor_loss = -q_mu.mean()
            actor_loss.backward()
            if self.clip_actor_gradient:
                nn.utils.clip_grad_value_(m.actor_params(), self.actor_clip)
            self.actor_optim.step()
            self.kept_q = q_mu.detach().clone()
        stats = {'actor_loss': 0.0 if self.kept_q is None else float(-self.kept_q.mean()),
                 'critic_loss': critic_loss.item(), 'action_norm': actions.norm(2, 1).mean().item(),
                 'rewards': rewards.mean().item(), 'Q_target': y.mean().item(), 'Q_policy': q.mean().item()}
        if self.use_double_critic:
            stats['Q_policy2'] = q2.mean().item()
        if update:
            self._target_update()
        return stats


def _params(case, seed):
    h = case['hyper']
    ln = bool(h.get('layernorm', False))
    if case.get('pixel'):
        return ddpg_oracle.make_ddpg_pixel_params(case['D'], case['A'], tuple(case['pixel']), case['conv_hidden'],
                                                  tuple(case['ah']), tuple(case['ch']), seed=seed, layernorm=ln)
    return ddpg_oracle.make_ddpg_params(case['D'], case['A'], tuple(case['ah']), tuple(case['ch']), seed=seed, layernorm=ln)


def make_oracle(case, d):
    h = case['hyper']
    double = bool(h.get('double_critic', False))
    return DelayedOracle(
        _params(case, 3), gamma=h['gamma'], n_step=h['n_step'], lr_actor=h['lr_actor'], lr_critic=h['lr_critic'],
        clip_critic_gradient=h.get('clip_critic', False), target_update_type=h['target_update_type'],
        target_update_interval=h['target_update_interval'], tau=h.get('tau', 1e-3), batch_size=case['B'],
        use_double_critic=double, use_action_regularization=bool(h.get('action_reg', False)),
        params2=_params(case, 4) if double else None, policy_delay=d, **ddpg_oracle.clip_reg_kwargs(h))


_MISSING = object()


def make_learner(case, opts=None, policy_delay=_MISSING, hard=False):
    """ddpg_helpers.make_learner with learner_config.algo.network.policy_delay set (left out: the key is absent)"""
    import surreal_amd.learner.ddpg as LD
    real = LD.DDPGLearner

    class WithDelay(real):
        def __init__(self, lc, ec, sc):
            if policy_delay is not _MISSING:
                lc.algo.network.policy_delay = policy_delay
            if hard:
                lc.algo.network.target_update.type = 'hard'
            super().__init__(lc, ec, sc)
    LD.DDPGLearner = WithDelay
    try:
        return DH.make_learner(case, opts)
    finally:
        LD.DDPGLearner = real


def batch(case, it):
    """iteration `it`'s batch, and numpy's global stream where TD3's action regularisation draws from it"""
    b = synthetic.make_ddpg_batch(case['B'], case['D'], case['A'], seed=10 + it,
                                  pixel=tuple(case['pixel']) if case.get('pixel') else None)
    np.random.seed(1000 + it)
    return b


_REFERENCE = {}


def reference(name, d):
    """the restatement's ITERS iterations of a case at delay d, run once: (statistics per iteration, final tensors)"""
    if (name, d) not in _REFERENCE:
        case = DH.load(name)[1]
        O = make_oracle(case, d)
        stats = []
        for it in range(ITERS):
            b = batch(case, it)
            stats.append(O.learn(b))
        finals = {'model': O.model.numpy_params(), 'target': O.model_target.numpy_params()}
        if O.use_double_critic:
            finals['model2'] = {k: v for k, v in O.model2.numpy_params().items() if not k.startswith('actor.')}
            finals['target2'] = {k: v for k, v in O.model_target2.numpy_params().items() if not k.startswith('actor.')}
        _REFERENCE[(name, d)] = (stats, finals)
    return _REFERENCE[(name, d)]


def learner_tensors(L):
    out = {'model': L.model.numpy_params(), 'target': L.model_target.numpy_params()}
    if L.use_double_critic:
        out['model2'], out['target2'] = L.model2.numpy_params(), L.model_target2.numpy_params()
    return out


def run_against_reference(name, opts, d, param_atol=None, report=None):
    """ITERS iterations of a learner at delay d against the restatement: every statistic of every iteration at STAT_TOL,
    every element of every final tensor at the case's parameter bound.  -> the learner"""
    case = DH.load(name)[1]
    want_stats, want = reference(name, d)
    atol = DH.PARAM_ATOL.get(name, DH.PARAM_ATOL_DEFAULT) if param_atol is None else param_atol
    L = make_learner(case, opts, policy_delay=d)
    worst = {'statistics': 0.0}
    for it in range(ITERS):
        st = dict(L.learn(batch(case, it)))
        assert set(st) == set(want_stats[it]), (sorted(st), sorted(want_stats[it]))
        for k, v in want_stats[it].items():
            worst['statistics'] = max(worst['statistics'], abs(st[k] - v))
            if report is None:
                np.testing.assert_allclose(st[k], v, atol=STAT_TOL, rtol=STAT_TOL,
                                           err_msg='%s d=%d iteration %d %s' % (name, d, it + 1, k))
    got = learner_tensors(L)
    for which in want:
        n = 0
        for k, v in want[which].items():
            if k not in got[which]:
                continue
            n += 1
            diff = float(np.abs(got[which][k] - v).max())
            worst[which] = max(worst.get(which, 0.0), diff)
            if report is None:
                assert diff <= atol, '%s d=%d %s %s: max diff %g (bound %g)' % (name, d, which, k, diff, atol)
        assert n >= 6, (which, n)
    print('%s d=%d %s: worst abs diff %s' % (name, d, sorted((opts or {}).items()), worst))
    if report is not None:
        report.update(worst)
    assert L.critic_step == ITERS and L.actor_step == ITERS // d
    return L


class DelayRowsCpuKernels(LnTd3RowsCpuKernels):
    """the LayerNorm TD3 double with the launches of a delayed policy update: the critic-only chains (the chain of the full
    iteration with the actor's buffers left as they were), the statistics in a critic group's launch, the tail.  update_log
    keeps, per ddpg_rows_update, (group, whether a target came along, the step word's value, whether it reported)"""
    ddpg_rows_delay = True
    RECORDED = tuple(LnTd3RowsCpuKernels.RECORDED) + ('ddpg_rows_critic_only', 'ddpg_rows_critic_only_td3',
                                                      'ddpg_rows_delay_tail')

    def __init__(self, *a, **kw):
        self.update_log = []
        super().__init__(*a, **kw)

    def _without_actor(self, chain, args):
        keep = [args.io[k] for k in ('h1a', 'h2a', 'act')]
        if getattr(args, 'io_ln', None) is not None:
            keep += [args.io_ln[k] for k in ('a1', 'am1', 'ar1', 'a2', 'am2', 'ar2')]
        saved = [t.clone() for t in keep]
        chain(self, args)
        for t, s in zip(keep, saved):
            t.copy_(s)

    def ddpg_rows_critic_only(self, args):
        self._without_actor(LnTd3RowsCpuKernels.ddpg_rows_critic, args)

    def ddpg_rows_critic_only_td3(self, args):
        self._without_actor(LnTd3RowsCpuKernels.ddpg_rows_critic_td3, args)

    def _report(self, args, stats, stats_host):
        io, io2 = args.io, getattr(args, 'io2', None)
        self.ddpg_stats(io['q'], io['y'], io['rewards'], io['actions'], io['q_actor'], stats)
        two = io2 is not None and io2.get('stats2') is not None
        if two:
            self.ddpg_stats(io2['q2'], io['y'], io['rewards'], io['actions'], io2['q2'], io2['stats2'])
        if stats_host is not None:
            slot = stats_host.view(2, 16 if two else 8)[int(io['step'][0]) & 1]
            slot[:7].copy_(stats[:7])
            if two:
                slot[8:15].copy_(io2['stats2'][:7])

    def ddpg_rows_delay_tail(self, args, actor_step, stats=None, stats_host=None):
        if stats is not None:
            self._report(args, stats, stats_host)
        actor_step += 1

    def ddpg_rows_update(self, args, group, theta, grads, exp_avg, exp_avg_sq, lr, step, weight_decay, clip_value,
                         target=None, tau=0.0, interval=0, wgrad=False, stats=None, stats_host=None):
        self.update_log.append((group, target is not None, int(step[0]), stats is not None))
        if stats is not None and group != 'actor':
            # (the statistics workgroup reads the chain launches' buffers, which the step leaves alone)
            assert wgrad
            self._report(args, stats, stats_host)
            stats = stats_host = None
        return LnTd3RowsCpuKernels.ddpg_rows_update(self, args, group, theta, grads, exp_avg, exp_avg_sq, lr, step,
                                                    weight_decay, clip_value, target=target, tau=tau, interval=interval,
                                                    wgrad=wgrad, stats=stats, stats_host=stats_host)


def _reach_double():
    import reach_ddpg_variants_cases as V

    class ReachDelayCpuKernels(DelayRowsCpuKernels, V.ReachVariantsCpuKernels):
        """the double of scripts/train_reach.py's loop (rollouts on the task) with the launches of a delayed policy update"""
    return ReachDelayCpuKernels


def ReachDelayCpuKernels(*a, **kw):
    return _reach_double()(*a, **kw)
