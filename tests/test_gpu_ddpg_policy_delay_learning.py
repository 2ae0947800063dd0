"""GPU tier (-m gpu): the on-device DDPG loop learns `reach` as TD3 with delayed policy updates.  scripts/train_reach.py's
loop at test_gpu_reach_learning.py's protocol -- 64 actors, J = 2, episodes of 50 steps, hidden 32 / 32, seed 0, fixed resets
-- with --double-critic --policy-delay 2: two critics on the row schedule, the actor and the targets moving at every second
learner iteration.  Condition, test_gpu_reach_learning.py's: the trained deterministic policy's mean return over the 64 reset
states is above the zero action's, which the test takes from the host env.

ITERS: chosen on the torch-CPU double before any GPU run (ddpg_delay_cases.ReachDelayCpuKernels; the double draws from no
noise stream, so the exploration came from torch.randn).  With half the actor updates the evaluation return still crossed the
zero action's (-216.8) before chunk 10: -199.6 at 10, -113.1 at 20, -57.0 at 30, -52.2 at 40, -44.6 at 60, -43.7 at 80.  So
plain DDPG's 30 chunks stay (profiles/ddpg_policy_delay_learning.jsonl has that run and the MI355X's: -235.7 at 10, -248.0
at 20, -78.6 at 30 with the device's noise stream -- above the zero action's at the last point only, 0.77 of the gap closed).

The share of the zero -> PD gap closed is a measurement, not a bar: with SMX_POLICY_DELAY_LEARNING_OUT set to a path the run
appends its line there.  One run; other seeds unmeasured."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

pytestmark = pytest.mark.gpu

ITERS = 30


def test_the_loop_learns_reach_as_td3_with_a_delay():
    import train_reach as TR
    lines = []
    base, curve = TR.train('ddpg', actors=64, J=2, episode_len=50, iters=ITERS, seed=0, eval_every=10, log=lines.append,
                           double_critic=True, policy_delay=2)
    print('\n'.join(lines))
    zero, pd = base['zero_action_return'], base['pd_return']
    assert pd > zero                                        # (both ends of the gap come from the host env)
    assert base['double_critic'] is True and base['policy_delay'] == 2
    last = curve[-1]
    assert last['iteration'] == ITERS and last['learner_iterations'] > 0
    path = os.environ.get('SMX_POLICY_DELAY_LEARNING_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(variant='double-critic policy-delay 2', iterations=ITERS,
                                    learner_iterations=last['learner_iterations'], eval_return=last['eval_return'],
                                    gap_closed=last['gap_closed'], wall_s=last['wall_s'], zero_action_return=zero,
                                    pd_return=pd, curve=[(c['iteration'], c['eval_return']) for c in curve])) + '\n')
    assert last['eval_return'] > zero, (last, zero)
