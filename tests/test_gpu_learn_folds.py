"""GPU tier (-m gpu): the learn's final forward-only policy pass with the launches behind it folded in
(smx_epoch_forward_final_f32, csrc/smx_epoch.hip) against those launches on the same inputs: smx_epoch_forward_f32 +
smx_epoch_backward_f32 (will_update = 0: statistics and the early exit only) + smx_ppo_learn_epilogue_f32.

The bar is bit identity, compared as integers after poisoning the outputs: the last policy workgroup adds the partial rows
in smx_epoch_backward_f32's order, and the end-of-learn roles run the 1024-thread arithmetic of learn_epilogue_kernel on 512
threads in two passes.  Cases, shapes and why: tests/learn_fold_cases.py.  Each case runs unpaired and in pair mode, each
fold alone and both together, three launches in a row and then captured once in a graph and replayed three times; the
z-filter sums accumulate over the rounds, so a round that ran a role twice or not at all cannot pass.  Every ticket word
reads zero at the end.

Learner level: two learners that differ in the two session keys alone get the same three batches; parameters, both Adam
moments, the z-filter state and the whole statistics block must have the same bits, with two launches fewer per learn."""
import copy

import pytest
import torch

import helpers as H
import learn_fold_cases as FC
from surreal_amd import _lib as L
from surreal_amd import synthetic
from test_gpu_epoch import build

pytestmark = pytest.mark.gpu

ROUNDS = 3


@pytest.fixture(scope='module')
def K():
    from surreal_amd.kernels import HipKernels
    return HipKernels()


def _bits(v):
    return v.contiguous().view(torch.int32)


class Side(object):
    """one copy of a case's problem: the policy pass's tensors (t), the end-of-learn launch's (e), two tickets"""

    def __init__(self, K, c):
        rows, A = c['rows'], c['A']
        self.c = c
        self.t = build(rows, FC.D, FC.H1, FC.H2, A, seed=rows + 31 * A, mode=c['mode'], device='cuda')['d']
        self.e = FC.epilogue_problem(c)
        t = self.t
        ci = t['ctrl'].view(torch.int32)
        t['ctrl'][L.C_KL_TARGET] = 1e-9 if c['ctrl'] == 'raises' else 1e9
        ci[L.C_STOP] = 1 if c['ctrl'] == 'stopped' else 0
        self.stop = ci[L.C_STOP:L.C_STOP + 1]
        K.epoch_pack([(t['act'], t['pk_a'])])

    def args(self):
        t, rows = self.t, self.c['rows']
        loss = dict(mode=self.c['mode'], rows=rows, log_var=t['log_var'], actions=t['actions'], behave=t['behave'],
                    ref=t['ref'], adv=t['adv'], g_surr=t['g_surr'], g_kl=t['g_kl'], partials=t['partials'],
                    check_stop=True, will_update=False, dlogvar=t['dlogvar'], dlogvar_sumsq=t['dlq'], stats=t['stats'])
        aj = dict(net=t['act'], packed=t['pk_a'], x=t['x'], h1T=t['h1aT'], h2T=t['h2aT'], out=t['mean'],
                  act=L.SMX_ACT_TANH, loss='policy', stop=self.stop, dz3T=t['dz3aT'], dz2T=t['dz2aT'], dz1T=t['dz1aT'])
        return [aj], loss

    def poison(self):
        for k in FC.POLICY_OUT:
            self.t[k].fill_(7.0)           # (a result nobody wrote, or one left by an earlier launch, must not pass)
        for k in FC.EPILOGUE_OUT:
            self.e[k].fill_(7.0)

    def parent(self, K, xchg):
        """the launches of the parent schedule"""
        jobs, loss = self.args()
        K.epoch_forward(jobs, loss, self.t['ctrl'], self.c['rows'], xchg=xchg)
        K.epoch_backward(jobs, loss, self.t['ctrl'], self.c['rows'])
        K.learn_epilogue(**FC.epilogue_args(self.c, self.t, self.e))

    def folded(self, K, xchg, stats, epi):
        jobs, loss = self.args()
        K.epoch_forward_final(jobs, loss, self.t['ctrl'], self.c['rows'], xchg=xchg,
                              stats_ticket=self.e['ticket'][1:2] if stats else None,
                              epilogue=FC.epilogue_args(self.c, self.t, self.e) if epi else None)
        if not stats:
            K.epoch_backward(jobs, loss, self.t['ctrl'], self.c['rows'])
        if not epi:
            K.learn_epilogue(**FC.epilogue_args(self.c, self.t, self.e))

    def words(self):
        """every word the launches write"""
        w = {k: self.t[k].clone() for k in FC.POLICY_OUT}
        w.update({k: self.e[k].clone() for k in FC.EPILOGUE_OUT})
        w['ctrl'] = self.t['ctrl'].clone()
        if self.e['z'] is not None:
            z = self.e['z']
            w.update(zsum=z.running_sum.clone(), zsumsq=z.running_sumsq.clone(), zcount=z.count.clone())
        return w


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


@pytest.mark.parametrize('c', FC.kernel_cases(), ids=FC.case_id)
def test_folded_final_launch_has_the_bits_of_the_launches_it_replaces(K, c):
    ref = Side(K, c)
    want = []
    for r in range(2 * ROUNDS):                     # three eager rounds, three more for the replays
        ref.poison()
        ref.parent(K, None)
        want.append(ref.words())
    torch.cuda.synchronize()
    if c['ctrl'] == 'stopped':                      # nothing of the policy pass was written
        assert bool((want[0]['stats'] == 7.0).all()) and bool((want[0]['mean'] == 7.0).all())
    else:
        assert not bool((want[0]['stats'][:4] == 7.0).any())
    if c['ctrl'] == 'raises':
        assert int(want[0]['ctrl'].view(torch.int32)[L.C_STOP]) == 1
    assert not bool((want[0]['fin'] == 7.0).any())
    if c['zfilter']:                                # the rounds do differ: the running sums take every batch in
        assert not torch.equal(want[0]['fin'], want[1]['fin'])
    nb = (c['rows'] + 15) // 16
    xchg = K.epoch_pair_xchg(ref.t['act'])
    for paired in (False, True):
        for stats, epi in ((True, True), (True, False), (False, True)):
            what = '%s, statistics %d, epilogue %d' % ('pair' if paired else 'unpaired', stats, epi)
            s = Side(K, c)
            px = xchg if paired else None
            flags0 = xchg[:16 * nb].view(torch.int32).clone()
            for r in range(ROUNDS):
                s.poison()
                s.folded(K, px, stats, epi)
                torch.cuda.synchronize()
                _same(s.words(), want[r], '%s, launch %d' % (what, r))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                s.folded(K, px, stats, epi)
            for r in range(ROUNDS, 2 * ROUNDS):
                s.poison()
                g.replay()
                torch.cuda.synchronize()
                _same(s.words(), want[r], '%s, replay %d' % (what, r - ROUNDS))
            assert bool((s.e['ticket'] == 0).all()), what
            assert int(s.t['ctrl'].view(torch.int32)[L.C_SYNC_ERR]) == 0
            if paired and c['ctrl'] == 'run':          # the launches did run on pairs: every workgroup published each of
                f = xchg[:16 * nb].view(torch.int32) - flags0     # its hand-overs once per launch, eager or replayed
                assert bool((f == 2 * ROUNDS).all()), what


# ---- learner level ----------------------------------------------------------------------------------------------------
def _learner(mode, kl_target, on, graph):
    case = FC.learner_case(mode, kl_target)
    shp = case['shape']
    params = synthetic.make_ppo_params(shp['D'], shp['A'], hidden=tuple(case['hidden']), **case['param_args'])
    zstate = synthetic.make_zfilter_state(shp['D'], **case['z_args'])
    over = {k: on for k in FC.FOLD_KEYS}
    over['use_hip_graph'] = graph
    return H.make_learner(case, params, zstate, session_overrides=over), case


def _state(learner):
    m = learner.model
    z = m.z_filter
    return dict(actor=m.actor_flat, critic=m.critic_flat, a_m=learner.actor_exp_avg, a_v=learner.actor_exp_avg_sq,
                c_m=learner.critic_exp_avg, c_v=learner.critic_exp_avg_sq, zsum=z.running_sum, zsumsq=z.running_sumsq,
                zcount=z.count, scal=learner._ws.scal, adv=learner._ws.adv, ret=learner._ws.ret)


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('kl_target', [1e9, FC.EARLY_EXIT_KL_TARGET], ids=['all_epochs', 'early_exit'])
@pytest.mark.parametrize('mode', ['adapt', 'clip'])
def test_learners_with_and_without_the_folds_stay_bit_identical(mode, kl_target, graph):
    off, case = _learner(mode, kl_target, False, graph)
    on, _ = _learner(mode, kl_target, True, graph)
    shp = case['shape']
    rec = {}
    if not graph:
        for name, lr in (('off', off), ('on', on)):
            lr.K = rec[name] = FC.Recording(lr.K)
    epochs = []
    for step in range(3):
        batch = synthetic.make_ppo_batch(shp['B'], shp['N'], shp['D'], shp['A'], seed=50 + step)
        for r in rec.values():
            del r.calls[:]
        off.learn(copy.deepcopy(batch))
        on.learn(copy.deepcopy(batch))
        torch.cuda.synchronize()
        a, b = _state(off), _state(on)
        for k in a:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (step, k)
        assert off.epochs_executed == on.epochs_executed
        epochs.append(on.epochs_executed)
        assert bool((on._ws.ticket == 0).all()) and bool((off._ws.ticket == 0).all())
    assert on._ws.fold_final_stats and on._ws.fold_epilogue and on._ws.merged_tail
    assert not off._ws.fold_final_stats and not off._ws.fold_epilogue
    if kl_target < 1.0:
        assert min(epochs) < case['hyper']['epoch_policy'], epochs        # the early exit was taken
    else:
        assert epochs == [case['hyper']['epoch_policy']] * 3
    if not graph:
        # two launches fewer per learn: the final pass's statistics launch and the end-of-learn launch
        c0, c1 = rec['off'].calls, rec['on'].calls
        assert len(c1) == len(c0) - 2
        assert c0.count('epoch_backward') == c1.count('epoch_backward') + 1
        assert c0.count('learn_epilogue') == 1 and c1.count('learn_epilogue') == 0
        assert c0.count('epoch_forward') == c1.count('epoch_forward') + 1 and c1.count('epoch_forward_final') == 1
        rest = lambda cs: [n for n in cs if n not in ('epoch_forward', 'epoch_forward_final', 'epoch_backward',  # noqa: E731
                                                      'learn_epilogue')]
        assert rest(c0) == rest(c1)
