"""GPU tier (-m gpu): one disturbed launch against the float64 restatement (tests/rollout_fp64_ref.py's policies, rings
and windows on task_disturbance_cases.DisturbedReachEnv / DisturbedArmEnv, which add scale * w in float64; the draws are
inputs, like the exploration draws) at the project's rtol = atol = 1e-5 (rollout_envelope_cases.TOL), rows written, dones
and the rows never written exact -- at parameter seeds under which the restatement ALONE keeps MARGIN from every clip, clamp
and ReLU kink (task_disturbance_cases.TUNED, found on the CPU).  Six cases: both tasks, the three kernel families, a second
Philox block (J = 5) and the widest rows (J = 21 / 30).

With SMX_DISTURBANCE_ERRORS_OUT set to a path the observed error / bound per case, block size and field is appended there
(profiles/task_disturbance_errors.txt is such a run on an MI355X)."""
import os

import pytest

import reach_cases as RC
import rollout_envelope_cases as EC
import task_disturbance_cases as TD

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.mark.parametrize('cid', TD.RESTATED)
def test_one_disturbed_launch_meets_the_float64_restatement(cid):
    c = TD.BY_ID[cid]
    want = None
    for apw in (4, 16, 0):
        x = TD.setup(c, DEV, seed=TD.TUNED[cid])
        if want is None:
            want, wrows, written, pol = TD.restatement(x)
            print(cid, 'input conditions', RC.input_conditions(pol))
        got, rows = TD.run(x, apw)
        assert rows == wrows
        errs = EC.worst_errors(got, want, written)
        line = '%s scale %g block %d: error / bound %s' % (cid, TD.SCALE, apw, {k: round(v, 3) for k, v in errs.items()})
        print(line)
        path = os.environ.get('SMX_DISTURBANCE_ERRORS_OUT')
        if path:
            with open(path, 'a') as f:
                f.write(line + '\n')
        assert max(errs.values()) <= 1.0, (apw, errs)
