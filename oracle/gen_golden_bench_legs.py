#!/usr/bin/env python
"""
TEST INFRASTRUCTURE ONLY (build container: needs the reference tree, oracle/ref_shims.py).  tests/golden/bench_cpu_legs.json:
the statistics of ONE learn of the REFERENCE'S OWN learner (surreal/learner/ppo.py `_preprocess_batch_ppo` + `_optimize`
under the shims, as bench.py's `kind: reference` CPU leg runs it) on the small shapes of
tests/test_bench_line.py::test_reference_and_port_cpu_legs_agree, MLP and LSTM policy.  With them the test holds the
restatement (oracle/ppo_oracle.py, bench.py's `kind: port` leg) to the reference where the reference tree is absent.

    python oracle/gen_golden_bench_legs.py          (seconds)
"""
import copy
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_shims  # noqa: E402
import ppo_oracle  # noqa: E402
from surreal_amd import synthetic  # noqa: E402

PATH = os.path.join(ROOT, 'tests', 'golden', 'bench_cpu_legs.json')
SPEC = {'B': 6, 'N': 12, 'D': 9, 'A': 3, 'hidden': [24, 16], 'batch_seed': 3, 'param_seed': 1,
        'hyper': {'kl_target': 1e9, 'ppo_mode': 'adapt'}, 'rnn': {'rnn_hidden': 12, 'horizon': 4}}


def case_inputs(spec, rnn):
    """the seeded batch, parameters and learner hyper-parameters of one case (the test rebuilds them from the spec)"""
    Bs, Ns, Ds, As = spec['B'], spec['N'], spec['D'], spec['A']
    F = spec['rnn']['rnn_hidden'] if rnn else 0
    batch = synthetic.make_ppo_batch(Bs, Ns, Ds, As, seed=spec['batch_seed'], rnn_hidden=F)
    params = synthetic.make_ppo_params(Ds, As, hidden=tuple(spec['hidden']), seed=spec['param_seed'], rnn_hidden=F)
    hyper = dict(spec['hyper'], n_step=Ns)
    if rnn:
        hyper.update(if_rnn_policy=True, horizon=spec['rnn']['horizon'])
    return batch, params, hyper


def main():
    import gen_golden as G
    ref = ref_shims.import_reference()
    Bs, Ns, Ds, As = SPEC['B'], SPEC['N'], SPEC['D'], SPEC['A']
    doc = {'spec': SPEC, 'stats': {}}
    for rnn in (False, True):
        batch, params, hyper = case_inputs(SPEC, rnn)
        Lr = G.build_reference_learner(ref, params, None, Bs, Ns, Ds, As, hyper)
        bd = Lr._preprocess_batch_ppo(ref_shims.BeneDict(copy.deepcopy(batch)))
        rs = Lr._optimize(bd.obs, bd.actions, bd.rewards, bd.obs_next, bd.persistent_infos, bd.onetime_infos, bd.dones)
        stats = {k: float(v) for k, v in rs.items() if k != '_lr'}
        # recorded only when the restatement agrees bit for bit on this host (what the live test asserts)
        port = ppo_oracle.OraclePPOLearner(params, As, Bs, **hyper).learn(copy.deepcopy(batch))
        for k, v in stats.items():
            assert v == float(port[k]) or (v != v and float(port[k]) != float(port[k])), (rnn, k, v, port[k])
        doc['stats']['lstm' if rnn else 'mlp'] = stats
    with open(PATH, 'w') as fp:
        json.dump(doc, fp, indent=1, sort_keys=True)
    print('wrote', PATH)


if __name__ == '__main__':
    main()
