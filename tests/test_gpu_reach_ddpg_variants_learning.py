"""GPU tier (-m gpu): the on-device DDPG loop learns `reach` with the actor variants.  scripts/train_reach.py's loop at 64
actors, J = 2, episodes of 50 steps, hidden 32 / 32, seed 0, three ways: --layernorm; --param-noise adaptive_normal
--actors-per-agent 4; both.  The rollout chunk is the variant's instantiation of the one-launch kernel on the task, the
noise is refreshed where the loop hands the learner's parameters to the agent.  Condition, test_gpu_reach_learning.py's:
the trained deterministic policy's mean return over the 64 reset states is above the zero action's, which the test takes
from the host env.

ITERS: the same loop on the torch-CPU double (reach_ddpg_variants_cases.ReachVariantsCpuKernels; the doubles draw from no
noise stream, so the exploration came from torch.randn) crossed the zero action's return (-216.8) before iteration 10 with
--layernorm (-103.7 at 10, -83.0 at 20, -61.5 at 30) and with both options (-100.0 at 10, -69.7 at 20, -60.2 at 30).  What
that says about the parameter noise is nothing: the double's population launch steps every actor from the clean actor, so
its run with both options is the LayerNorm learner with the refresh calls, and it has no evaluation launch for the
population line of the run without LayerNorm, which stops there.  The double cannot run the population's learner: the
count is plain DDPG's 30 (test_gpu_reach_learning.py), which the two runs above confirm for the LayerNorm learner.

The share of the zero -> PD gap closed is a measurement, not a bar: with SMX_REACH_VARIANTS_LEARNING_OUT set to a path the
run appends one line per variant there, plain DDPG's from the same run first (profiles/reach_ddpg_variants_learning.jsonl
is such a run on an MI355X)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

pytestmark = pytest.mark.gpu

ITERS = 30
VARIANTS = {
    'layernorm': dict(layernorm=True),
    'param-noise': dict(param_noise='adaptive_normal', actors_per_agent=4),
    'layernorm+param-noise': dict(layernorm=True, param_noise='adaptive_normal', actors_per_agent=4),
}


def run(**variant):
    import train_reach as TR
    lines = []
    base, curve = TR.train('ddpg', actors=64, J=2, episode_len=50, iters=ITERS, seed=0, eval_every=10, log=lines.append,
                           **variant)
    return base, curve, lines


@pytest.fixture(scope='module')
def record():
    path = os.environ.get('SMX_REACH_VARIANTS_LEARNING_OUT')
    rec = []
    if path:
        base, curve, _ = run()
        rec.append(dict(variant='plain', iterations=ITERS, eval_return=curve[-1]['eval_return'],
                        gap_closed=curve[-1]['gap_closed'], wall_s=curve[-1]['wall_s'],
                        zero_action_return=base['zero_action_return'], pd_return=base['pd_return']))
    yield rec
    if path and rec:
        with open(path, 'a') as f:
            for r in rec:
                f.write(json.dumps(r) + '\n')


@pytest.mark.parametrize('name', list(VARIANTS))
def test_the_loop_learns_reach_with_the_variant(name, record):
    variant = VARIANTS[name]
    base, curve, lines = run(**variant)
    print('\n'.join(lines))
    zero, pd = base['zero_action_return'], base['pd_return']
    assert pd > zero                                        # (both ends of the gap come from the host env)
    last = curve[-1]
    assert last['iteration'] == ITERS and last['learner_iterations'] > 0
    pop = [json.loads(s) for s in lines if '"kind": "population"' in s]
    if variant.get('param_noise') and not variant.get('layernorm'):
        # a plain-actor population: a line per evaluation point, a return per agent, the noise refreshed every chunk
        assert [p['iteration'] for p in pop] == [0, 10, 20, 30] and all(len(p['agent_returns']) == 16 for p in pop)
        assert [p['generation'] for p in pop] == [0, 10, 20, 30]
        assert pop[-1]['sigma'] != pop[0]['sigma']          # (adaptive: the refreshes moved the sigmas)
    else:
        assert not pop
    r = dict(variant=name, iterations=ITERS, eval_return=last['eval_return'], gap_closed=last['gap_closed'],
             wall_s=last['wall_s'])
    if pop:
        r.update(agent_returns=pop[-1]['agent_returns'], sigma=pop[-1]['sigma'])
    record.append(r)
    assert last['eval_return'] > zero, (last, zero)
