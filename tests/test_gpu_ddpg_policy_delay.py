"""GPU tier (-m gpu): TD3's delayed policy updates (learner_config.algo.network.policy_delay) on the HIP kernels -- every case
on every schedule it can take against the restatement run live on the CPU (ddpg_delay_cases.py), and the bit-level
properties of the critic-only iterations: under the two captured graphs, across invalidate_packed(), across a resume."""
import pytest
import torch

import ddpg_delay_cases as DC
import ddpg_helpers as DH

pytestmark = pytest.mark.gpu

BIT_CASES = [('tiny_ln_td3_soft', 'rows'), ('tiny_ln_td3_soft', 'layers'), ('tiny_soft_clipcritic', 'rows'),
             ('tiny_soft_clipcritic', 'layers')]


def flats(L):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in L._train_tensors().items()}


def same_bytes(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def run(name, sched, iters=DC.ITERS, first=0, L=None, **kw):
    """iterations first .. iters - 1 of a learner (built here with **kw unless given) -> (learner, their statistics)"""
    case = DH.load(name)[1]
    opts = dict(DC.schedules(name)[sched], **kw.pop('opts', {}))
    if L is None:
        L = DC.make_learner(case, opts, **kw)
    stats = [dict(L.learn(DC.batch(case, it))) for it in range(first, iters)]
    assert L._schedule(*L._ws.key) == sched
    return L, stats


@pytest.mark.parametrize('name,schedule,d', DC.matrix())
def test_every_schedule_matches_the_restatement(name, schedule, d):
    L = DC.run_against_reference(name, DC.schedules(name)[schedule], d, param_atol=DC.gpu_param_atol(name))
    assert L._schedule(*L._ws.key) == schedule
    assert (L._ws.graph is not None) and (L._ws.graph_critic is not None)          # both kinds were captured and replayed


@pytest.mark.parametrize('name,sched', BIT_CASES)
def test_graphs_leave_the_eager_run_s_bytes(name, sched):
    eager, st_e = run(name, sched, policy_delay=2, opts={'use_hip_graph': False})
    graph, st_g = run(name, sched, policy_delay=2)
    assert eager._ws.graph is None and eager._ws.graph_critic is None
    assert graph._ws.graph is not None and graph._ws.graph_critic is not None
    same_bytes(flats(eager), flats(graph))
    assert st_e == st_g


@pytest.mark.parametrize('name,sched', BIT_CASES)
def test_critic_only_iterations_keep_the_actor_and_the_targets(name, sched):
    case = DH.load(name)[1]
    L = DC.make_learner(case, DC.schedules(name)[sched], policy_delay=2)

    def kept():
        torch.cuda.synchronize()
        out = [L.model.actor_flat, L.actor_exp_avg, L.actor_exp_avg_sq, L.model_target.actor_flat,
               L.model_target.critic_flat]
        if L.use_double_critic:
            out.append(L.model_target2.critic_flat)
        return [t.clone() for t in out]
    for it in range(DC.ITERS):
        before, critic = kept(), L.model.critic_flat.clone()
        L.learn(DC.batch(case, it))
        after = kept()
        assert not torch.equal(critic, L.model.critic_flat)
        for a, b in zip(before, after):
            assert torch.equal(a, b) == ((it + 1) % 2 != 0), it + 1


@pytest.mark.parametrize('name,sched', BIT_CASES)
def test_the_packed_copies_are_current_after_critic_only_iterations(name, sched):
    """invalidate_packed() after iteration 5 (critic-only, behind two updates) packs every network again from the
    parameters: the run goes on to the bytes of the one that never did"""
    straight, st_s = run(name, sched, policy_delay=2)
    L, st = run(name, sched, iters=5, policy_delay=2)
    L.invalidate_packed()
    _, st2 = run(name, sched, first=5, L=L)
    same_bytes(flats(straight), flats(L))
    assert st_s == st + st2


@pytest.mark.parametrize('name,sched', BIT_CASES)
def test_delay_one_is_the_learner_without_the_key(name, sched):
    a, st_a = run(name, sched, iters=4)
    b, st_b = run(name, sched, iters=4, policy_delay=1)
    assert b._ws.astep is None and b._ws.graph_critic is None
    same_bytes(flats(a), flats(b))
    assert st_a == st_b


@pytest.mark.parametrize('name,sched', BIT_CASES)
def test_a_resume_lands_on_the_uninterrupted_run(name, sched):
    A, _ = run(name, sched, iters=3, policy_delay=2)
    sd = A.train_state_dict()
    sd = dict(sd, words=dict(sd['words']), tensors={k: v.clone() for k, v in flats(A).items()})
    run(name, sched, first=3, L=A)
    B, _ = run(name, sched, iters=6, policy_delay=2)          # (both graphs captured, a history of its own)
    B.load_train_state_dict(sd)
    run(name, sched, first=3, L=B)
    assert B._ws.graph is not None and B._ws.graph_critic is not None
    same_bytes(flats(A), flats(B))
