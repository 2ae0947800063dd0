"""GPU tier (-m gpu): the on-device loop learns.  scripts/train_reach.py's loop -- rollout chunk inside one launch on
SyntheticVecEnv(task='reach') -> the replay's device ring -> learn -> parameters back to the agent -- at 64 actors, J = 2,
episodes of 50 steps, hidden 32 / 32, fixed seeds, once per algorithm.  Condition: the trained deterministic policy's
mean return over the 64 reset states is above the zero action's, which the test takes from the host env.  A wrong sign, a
stale packed weight or an off-by-one in the n-step bootstrap leaves the policy at or below it.

ITERS: on the torch-CPU doubles of the same loop the evaluation return crossed the zero action's (-216.8) before
iteration 10 (PPO: -186 at 10, -74 at 20; DDPG: -279 at 10, -74 at 15, -50 at 20) -- 30 leaves room to spare and keeps a
run to seconds.  The share of the zero -> PD gap each algorithm closes is a measurement (profiles/reach_learning.jsonl),
not a bar.  Measured on an MI355X at 30 iterations: PPO -58.2 (0.89 of the gap), DDPG -57.3 (0.89); 0.5 s and 0.3 s."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

pytestmark = pytest.mark.gpu

ITERS = {'ppo': 30, 'ddpg': 30}


@pytest.mark.parametrize('algo', ['ddpg', 'ppo'])
def test_the_loop_learns_reach(algo):
    import train_reach as TR
    lines = []
    base, curve = TR.train(algo, actors=64, J=2, episode_len=50, iters=ITERS[algo], seed=0, eval_every=10, log=lines.append)
    print('\n'.join(lines))
    zero, pd = base['zero_action_return'], base['pd_return']
    assert pd > zero                                        # (both ends of the gap come from the host env)
    assert curve[-1]['iteration'] == ITERS[algo] and curve[-1]['learner_iterations'] > 0
    assert curve[-1]['eval_return'] > zero, (curve[-1], zero)
