"""GPU tier (-m gpu): the on-device loop learns `arm`.  scripts/train_reach.py --task arm -- rollout chunk inside one
launch on SyntheticVecEnv(task='arm') -> the replay's device ring -> learn -> parameters back to the agent -- at 64 actors,
J = 2, episodes of 50 steps, hidden 32 / 32, seed 0, random resets (every training episode drawn on the device; the
evaluation on 4 held-out episodes per actor of another stream), once per algorithm.  Condition, test_gpu_reach_learning.py's:
the trained deterministic policy's mean return over the held-out episodes is above the zero action's on the same episodes,
which the test takes from the host env.  On this task an untrained policy may already be above the zero action (an arm
that moves at all sweeps past some goals), so the run must also end above its own iteration-0 return.

ITERS: the same loop on the torch-CPU double (arm_cases.ArmCpuKernels; the doubles draw from no noise stream, so the
exploration came from torch.randn), zero action -44.1, Jacobian-transpose controller -4.1: PPO -30.2 untrained, -12.7 at 20
chunks, -6.8 at 40, -6.0 at 100; DDPG -32.4 untrained, -6.7 at 20, -6.0 at 40.  40 leaves room and keeps a run to seconds.
(With the constants first proposed for the task -- gain 0.2, dt 0.1, orientations drawn from +-3 -- PPO stayed at the zero
action's -25.7 through 160 chunks on the double; the definition's constants were retuned before any GPU run.)

The share of the zero -> controller gap each algorithm closes is a measurement, not a bar: with SMX_ARM_LEARNING_OUT set to
a path the run appends one line per algorithm there (profiles/arm_learning.jsonl is such a run on an MI355X: one run each,
seed 0; other seeds are unmeasured).  Measured there at 40 chunks: DDPG -5.8 (0.96 of the gap, untrained -21.0), PPO -8.7
(0.89, untrained -28.2); 0.27 s and 0.47 s."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

pytestmark = pytest.mark.gpu

ITERS = {'ppo': 40, 'ddpg': 40}


@pytest.mark.parametrize('algo', ['ddpg', 'ppo'])
def test_the_loop_learns_arm(algo):
    import train_reach as TR
    lines = []
    base, curve = TR.train(algo, actors=64, J=2, episode_len=50, iters=ITERS[algo], seed=0, eval_every=10, log=lines.append,
                           random_resets=True, task='arm')
    print('\n'.join(lines))
    zero, jt = base['zero_action_return'], base['pd_return']
    assert base['task'] == 'arm' and base['heldout_episodes'] == 4
    assert jt > zero                                        # (both ends of the gap come from the host env)
    last = curve[-1]
    assert last['iteration'] == ITERS[algo] and last['learner_iterations'] > 0
    path = os.environ.get('SMX_ARM_LEARNING_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(task='arm', algo=algo, iterations=ITERS[algo], seed=0, zero_action_return=zero,
                                    jt_return=jt, untrained_return=curve[0]['eval_return'],
                                    eval_return=last['eval_return'], gap_closed=last['gap_closed'],
                                    wall_s=last['wall_s'])) + '\n')
    assert last['eval_return'] > zero, (last, zero)
    assert last['eval_return'] > curve[0]['eval_return'], (last, curve[0])
