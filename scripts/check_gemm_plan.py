"""The dense layer's planner (csrc/smx_gemm.hip: plan_batch) against its restatement in tests/dense_cases.py, on the host.

    hipcc ... scripts/micro/gemm_plan_hostcheck.hip ... -o scripts/micro/gemm_plan_hostcheck    (the recipe is in that file)
    python scripts/check_gemm_plan.py [program] > profiles/gemm_plan_hostcheck.txt

Feeds the program the problem list of every LINEAR_CASES and BATCHES entry, of every WGRAD_CASES entry that reaches the
GEMM kernels (split: the problem wgrad_plan forms), and the weight-gradient batches of the many-row split-K MLP backward
(tests/test_gpu_kernels.py::test_mlp3_backward_splitk_over_many_rows: hidden layers, output layer, and the two merged),
and compares kernel and grid with dense_cases.launch_batch.  Exits non-zero on any difference, or if a case went
uncompared.  Nothing is launched; no GPU is needed.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dense_cases as D  # noqa: E402


def wgrad_prob(c):
    """a Wg case -> the problem K.linear_wgrad hands the GEMM kernels, or None (smx_wgrad.hip takes it)"""
    p = D.prob_of(c)
    kernels, left = D.wgrad_plan(c)
    if kernels[0] == 'wgrad_rows':
        return None
    if len(kernels) == 1:
        return p
    return p._replace(dbias=True, splits=left, k_chunk=D.split32_closed_form(c.M, c.N, c.rows)[1])


def mlp3_batches(rows, Dm, H1, H2, OUT):
    """mlp3_splits / mlp3_wgrads_splitk below SMX_WGRAD_ROWS_MIN rows -> {name: problems}: the layers wide enough for the
    tile kernel, the rest, and the merged batch the library launches when the wide one stays off the tile kernel"""
    assert 2048 <= rows < D.WGRAD_ROWS_MIN
    t = sum(-(-m // 32) * -(-n // 32) for m, n in ((H1, Dm), (H2, H1), (OUT, H2)))
    S = min(rows // 1024, max(4096 // t, 1), 64)
    assert S >= 2
    k_chunk = (-(-rows // S) + 31) & ~31
    while (S - 1) * k_chunk >= rows:
        S -= 1
    wide, rest = [], []
    for M, N in ((H1, Dm), (H2, H1), (OUT, H2)):
        p = D.Prob(M, N, rows, 0, M, 0, 0, N, 0, True, S, k_chunk)
        (wide if (M >= 48 and N >= 64 and M % 4 == 0 and N % 4 == 0) else rest).append(p)
    out = {'wide': wide, 'rest': rest, 'merged': wide + rest}
    return {k: v for k, v in out.items() if v}


def main():
    prog = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'scripts', 'micro', 'gemm_plan_hostcheck')
    lists = []
    for c in D.LINEAR_CASES:
        lists.append((c.id, [D.prob_of(c)]))
    for c in D.BATCHES:
        lists.append((c.id, [D.prob_of(j) for j in c.jobs]))
    n_wgrad = 0
    for c in D.WGRAD_CASES:
        p = wgrad_prob(c)
        if p is not None:
            lists.append((c.id, [p]))
            n_wgrad += p.splits > 1
    # (the third, of test_mlp3_backward_fused_data_gradients_over_many_rows: its hidden layers DO take the tile kernel)
    for shape in ((7936, 100, 300, 200, 6), (2100, 17, 64, 40, 1), (30000, 100, 300, 200, 17)):
        for name, probs in mlp3_batches(*shape).items():
            lists.append(('mlp3-%dx%d-%d-%d-%d-%s' % (shape + (name,)), probs))
    assert len(set(i for i, _ in lists)) == len(lists)
    text = ''.join('list %s %d\n%s' % (i, len(ps), ''.join(' '.join(str(int(v)) for v in p) + '\n' for p in ps))
                   for i, ps in lists)
    env = {k: v for k, v in os.environ.items() if k != 'SMX_GEMM_ROWS_ONLY'}
    run = subprocess.run([prog], input=text, capture_output=True, text=True, env=env)
    sys.stderr.write(run.stderr)
    got = dict((f[0], f[1:]) for f in (line.split() for line in run.stdout.splitlines()))
    bad = compared = 0
    for i, ps in lists:
        kernel, grid = D.launch_batch(ps)
        want = [D.kernel_name(kernel), str(grid), str(int(isinstance(kernel, tuple)))]
        ok = got.get(i) == want
        compared += i in got
        bad += not ok
        print('%-44s %-10s grid %-6s %s' % (i, want[0], want[1], 'ok' if ok else 'DIFFERS: the library plans %s' % got.get(i)))
    print('%d lists: %d linear, %d batches, %d weight gradients (%d split), %d of the MLP backward; %d compared, %d differ' % (
        len(lists), len(D.LINEAR_CASES), len(D.BATCHES), len(lists) - len(D.LINEAR_CASES) - len(D.BATCHES) -
        sum(i.startswith('mlp3-') for i, _ in lists), n_wgrad, sum(i.startswith('mlp3-') for i, _ in lists), compared, bad))
    return 1 if (run.returncode or bad or compared != len(lists)) else 0


if __name__ == '__main__':
    sys.exit(main())
