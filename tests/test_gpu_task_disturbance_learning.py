"""GPU tier (-m gpu): the on-device loop learns the tasks under per-step disturbances.  scripts/train_reach.py
--random-resets --disturbance (its default scale, train_reach.DEFAULT_DISTURBANCE) -- every step of every training episode
disturbed on the device, the evaluation on 4 held-out episodes per actor of another stream under the same scale -- at 64
actors, J = 2, episodes of 50 steps, hidden 32 / 32, seed 0: PPO and DDPG on `reach`, DDPG on `arm`.  Condition, the
existing learning tests': the trained deterministic policy's mean return over the held-out disturbed episodes is above the
zero action's on the same episodes, which the test takes from the host env (SyntheticEnv(resets=, disturbance=)); on `arm`,
as in test_gpu_arm_learning.py, the run must also end above its own iteration-0 return.

The scale was chosen on the host env before any training run (profiles/task_disturbance_learning.jsonl, "what": "scale"):
at 0.25 the zero action's held-out return moves from -57.7 to -90.9 on `reach` and from -44.1 to -34.5 on `arm`, while the
PD / Jacobian-transpose controller still solves the task (-6.6 -> -7.6, -4.1 -> -4.3); at 0.5 the controller's return on
`reach` has nearly doubled (-11.1), at 0.1 the zero action's has moved by a tenth only.

The share of the zero -> controller gap each run closes is a measurement, not a bar: with SMX_DISTURBANCE_LEARNING_OUT set
to a path the run appends one line per run there (profiles/task_disturbance_learning.jsonl holds such a run on an MI355X:
one run each, seed 0; other seeds are unmeasured).  Measured there at 40 chunks: DDPG on `reach` -14.4 (0.92 of the gap,
untrained -136.6), PPO on `reach` -16.3 (0.89, untrained -120.9), DDPG on `arm` -5.9 (0.95, untrained -27.6); 0.28 s, 0.53 s and
0.28 s.  The same loops on the torch-CPU double (exploration from torch.randn), run before any GPU run: -13.2, -16.5, -5.9."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

pytestmark = pytest.mark.gpu

ITERS = 40                                      # (the undisturbed learning tests': 40 chunks leave room, a run takes seconds)


@pytest.mark.parametrize('algo,task', [('ddpg', 'reach'), ('ppo', 'reach'), ('ddpg', 'arm')])
def test_the_loop_learns_under_disturbance(algo, task):
    import train_reach as TR
    lines = []
    scale = TR.DEFAULT_DISTURBANCE
    base, curve = TR.train(algo, actors=64, J=2, episode_len=50, iters=ITERS, seed=0, eval_every=10, log=lines.append,
                           random_resets=True, task=task, disturbance=scale)
    print('\n'.join(lines))
    zero, ctl = base['zero_action_return'], base['pd_return']
    assert base['disturbance'] == scale and base['heldout_episodes'] == 4
    # both ends of the gap come from the host env, on the disturbed held-out episodes: not the undisturbed figures
    plain = TR.heldout_baselines(2, 50, 64, 3, 4, task)
    assert ctl > zero and zero != plain['zero_action_return'] and ctl != plain['pd_return']
    last = curve[-1]
    assert last['iteration'] == ITERS and last['learner_iterations'] > 0
    path = os.environ.get('SMX_DISTURBANCE_LEARNING_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(what='run', task=task, algo=algo, disturbance=scale, iterations=ITERS, seed=0,
                                    zero_action_return=zero, controller_return=ctl,
                                    undisturbed_zero_action_return=plain['zero_action_return'],
                                    undisturbed_controller_return=plain['pd_return'],
                                    untrained_return=curve[0]['eval_return'], eval_return=last['eval_return'],
                                    gap_closed=last['gap_closed'], wall_s=last['wall_s'])) + '\n')
    assert last['eval_return'] > zero, (last, zero)
    if task == 'arm':
        assert last['eval_return'] > curve[0]['eval_return'], (last, curve[0])
