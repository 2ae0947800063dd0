"""GPU tier (-m gpu): the on-device loop learns to reach goals it has not seen.  scripts/train_reach.py's loop with
random_resets=True -- every training episode begins with a start and goal drawn inside the rollout launch from a reset
stream (SyntheticVecEnv.attach_resets) -- at 64 actors, J = 2, episodes of 50 steps, hidden 32 / 32, fixed seeds, once per
algorithm.  The evaluation env draws from a stream with ANOTHER seed, set back to episode 0 before each evaluation: 4
held-out episodes per actor (256 start / goal pairs) that training never drew.  Condition: the trained deterministic
policy's mean return over them is above the zero action's on the same episodes; both ends of the gap (zero action, PD
controller) come from the host env, SyntheticEnv(resets=...).

ITERS: on the torch-CPU doubles of the same loop (zero action -57.74, PD -6.64 on the held-out episodes) the held-out
return crossed the zero action's between iterations 5 and 10 for PPO (-77.4 at 5, -47.2 at 10, -28.9 at 15, -13.5 at 30)
and between 10 and 15 for DDPG (-58.9 at 5, -74.5 at 10, -33.8 at 15, -13.4 at 30): crossing points 10 and 15, times 1.5
is 15 and 22.5 -- 30 for both, as test_gpu_reach_learning.py runs.  The share of the zero -> PD gap each algorithm closes
is a measurement (profiles/reach_resets_learning.jsonl), not a bar.  Measured on an MI355X at 30 iterations: PPO -11.1
(0.91 of the gap), DDPG -19.4 (0.75); 1.1 s and 0.7 s."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

pytestmark = pytest.mark.gpu

ITERS = {'ppo': 30, 'ddpg': 30}


@pytest.mark.parametrize('algo', ['ddpg', 'ppo'])
def test_the_loop_learns_to_reach_held_out_goals(algo):
    import train_reach as TR
    lines = []
    base, curve = TR.train(algo, actors=64, J=2, episode_len=50, iters=ITERS[algo], seed=0, eval_every=10, log=lines.append,
                           random_resets=True)
    print('\n'.join(lines))
    zero, pd = base['zero_action_return'], base['pd_return']
    assert base['random_resets'] and base['heldout_episodes'] == 4
    assert pd > zero                                        # (both ends of the gap come from the host env)
    assert curve[-1]['iteration'] == ITERS[algo] and curve[-1]['learner_iterations'] > 0
    assert curve[-1]['eval_return'] > zero, (curve[-1], zero)
