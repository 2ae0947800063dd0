"""CPU tier: which launches the learner enqueues around the final policy pass (learner/ppo.py _ws_epochs,
_enqueue_fused_epochs).  The kernel double (tests/cpu_kernels.py) has no epoch_forward_final: with it the learner takes
no fold and enqueues the call sequence it always did.  A double that offers the launch gets it exactly where the final
pass carries the policy alone and no value epoch follows, under the two session keys, with the same results."""
import copy

import pytest
import torch

import helpers as H
import learn_fold_cases as FC
from surreal_amd import kernels as KN
from surreal_amd import synthetic

# one learn of FC.learner_case (three policy and three value epochs) on the fused row-block schedule, as the kernel
# double runs it (no pair mode there): the launches between the critic pass and the statistics read-back
TODAY = (['epoch_prepare', 'epoch_forward', 'gae_norm'] + ['epoch_fwdbwd', 'mlp3_wgrad_multi', 'clip_adam_pair'] * 3 +
         ['epoch_forward', 'epoch_backward', 'learn_epilogue'])
LAUNCHES = set(TODAY) | {'epoch_forward_final'}


def _run(kernels, mode='adapt', kl_target=1e9, overrides=None, hyper=None, steps=2):
    prev = KN.set_default_kernels(kernels, 'cpu')
    try:
        case = FC.learner_case(mode, kl_target)
        case['hyper'].update(hyper or {})
        shp = case['shape']
        params = synthetic.make_ppo_params(shp['D'], shp['A'], hidden=tuple(case['hidden']), **case['param_args'])
        zstate = synthetic.make_zfilter_state(shp['D'], **case['z_args'])
        learner = H.make_learner(case, params, zstate, session_overrides=overrides)
        rec = learner.K = FC.Recording(learner.K)
        seqs = []
        for step in range(steps):
            del rec.calls[:]
            learner.learn(copy.deepcopy(synthetic.make_ppo_batch(shp['B'], shp['N'], shp['D'], shp['A'], seed=50 + step)))
            seqs.append([n for n in rec.calls if n in LAUNCHES])
        m = learner.model
        state = dict(actor=m.actor_flat.clone(), critic=m.critic_flat.clone(), zsum=m.z_filter.running_sum.clone(),
                     zcount=m.z_filter.count.clone(), scal=learner._ws.scal.clone())
        return learner, seqs, state
    finally:
        KN.set_default_kernels(*prev)


def _double():
    from cpu_kernels import TorchCpuKernels
    return TorchCpuKernels()


def _offering():
    """the double with the folded launch: by contract the launches it replaces, back to back"""
    from cpu_kernels import TorchCpuKernels

    class Offering(TorchCpuKernels):
        def epoch_forward_final(self, jobs, loss, ctrl, n_total, xchg=None, stats_ticket=None, epilogue=None):
            assert len(jobs) == 1 and jobs[0]['loss'] == 'policy' and not loss['will_update']
            self.epoch_forward(jobs, loss, ctrl, n_total)
            if stats_ticket is not None:
                assert stats_ticket.numel() == 1 and int(stats_ticket[0]) == 0
                self.epoch_backward(jobs, loss, ctrl, n_total)
            if epilogue is not None:
                self.learn_epilogue(**epilogue)
    return Offering()


@pytest.mark.parametrize('mode', ['adapt', 'clip'])
def test_the_kernel_double_keeps_todays_call_sequence(mode):
    K = _double()
    assert not hasattr(K, 'epoch_forward_final')
    learner, seqs, _ = _run(K, mode)
    ws = learner._ws
    assert ws.fused and ws.merged_tail and not ws.fold_final_stats and not ws.fold_epilogue
    assert seqs == [TODAY, TODAY]
    # ... whatever the session asks for
    learner, seqs, _ = _run(K, mode, overrides={k: True for k in FC.FOLD_KEYS})
    assert not learner._ws.fold_final_stats and not learner._ws.fold_epilogue and seqs == [TODAY, TODAY]


FOLDED = TODAY[:-3] + ['epoch_forward_final']


@pytest.mark.parametrize('stats,epi', [(True, True), (True, False), (False, True), (False, False)])
def test_a_kernel_set_with_the_launch_gets_it_under_the_session_keys(stats, epi):
    _, _, want = _run(_double())
    over = dict(fold_final_stats=stats, fold_epilogue=epi)
    learner, seqs, got = _run(_offering(), overrides=over)
    ws = learner._ws
    assert (ws.fold_final_stats, ws.fold_epilogue) == (stats, epi)
    if not stats and not epi:
        expect = TODAY
    else:
        expect = FOLDED + ([] if stats else ['epoch_backward']) + ([] if epi else ['learn_epilogue'])
    # (the offering double's launch calls the ones it replaces: they are recorded on the learner's facade only when the
    # learner itself makes them)
    assert seqs == [expect, expect]
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_the_defaults_take_both_folds():
    learner, seqs, _ = _run(_offering(), steps=1)
    assert learner._ws.fold_final_stats and learner._ws.fold_epilogue and seqs == [FOLDED]


def test_a_value_epoch_in_or_behind_the_final_pass_keeps_the_separate_launches():
    """epoch_baseline > epoch_policy: the final pass's launch carries the critic too (or value epochs follow it), and the
    value finalize reads what they write"""
    for Ev in (4, 5):
        learner, seqs, _ = _run(_offering(), hyper=dict(epoch_policy=3, epoch_baseline=Ev), steps=1)
        assert not learner._ws.fold_final_stats and not learner._ws.fold_epilogue
        assert 'epoch_forward_final' not in seqs[0] and seqs[0][-1] == 'learn_epilogue'


def test_an_early_exit_leaves_the_same_state_with_the_folds():
    _, _, want = _run(_double(), kl_target=FC.EARLY_EXIT_KL_TARGET)
    learner, _, got = _run(_offering(), kl_target=FC.EARLY_EXIT_KL_TARGET)
    assert learner.epochs_executed < 3
    for k in want:
        assert torch.equal(got[k], want[k]), k
