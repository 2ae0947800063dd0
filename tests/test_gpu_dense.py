"""GPU tier (-m gpu): the generic dense layer of csrc/smx_gemm.hip by itself -- smx_linear_f32, smx_linear_multi_f32 and
the weight gradients (plain, split-K, the register-resident kernel of csrc/smx_wgrad.hip) over the case table of
dense_cases.py: all 23 (kernel, operand-mode pair) cells, K at every prefetch-ring boundary, ragged M / N / K, tile counts
on both sides of the XCD permutation's remainder, every epilogue, stop flags, padded / offset operands and outputs.

Integer-valued inputs make every float32 partial sum exact, so the comparison with the int64 reference is torch.equal at
any summation order; everything next to an operand is NaN and everything around the output a sentinel (dense_cases.py
says how).  One library call per table entry: profiles/dense_paths_kernel_stats.csv, a kernel trace of this file alone,
shows the launch counts dense_cases.predicted_launches() gives."""
import pytest
import torch

import dense_cases as DC
from surreal_amd import _lib as L
from test_gpu_kernels import K  # noqa: F401  (the module-scoped kernels fixture)

pytestmark = pytest.mark.gpu


def ids(cases):
    return [c.id for c in cases]


def ws_for(K):
    def make(c):
        n = K.linear_wgrad_ws_floats(c.M, c.N, c.rows)
        return torch.full((max(n, 1),), float('nan'), device='cuda')       # a partial that is never written shows
    return make


@pytest.mark.parametrize('c', DC.LINEAR_CASES, ids=ids(DC.LINEAR_CASES))
def test_linear_case(K, c):
    DC.run_entry(K, c, 'cuda')


@pytest.mark.parametrize('c', DC.BATCHES, ids=ids(DC.BATCHES))
def test_linear_multi_batch(K, c):
    DC.run_entry(K, c, 'cuda')


@pytest.mark.parametrize('c', DC.WGRAD_CASES, ids=ids(DC.WGRAD_CASES))
def test_weight_gradient_case(K, c):
    DC.run_entry(K, c, 'cuda', ws_for=ws_for(K))


def test_the_restated_split_arithmetic_is_the_librarys(K):
    """the workspace query gives the library's chunk count S: the restatement agrees for every workspace case, and the
    (6, 10, 34817) gradient really meets both conditions -- S = 34 chunks of 1056 rows with the last one empty (the shrink
    loop runs), 33 > 32 left (ldw == N takes segmented_reduce_kernel, ldw == N + 3 splitk_reduce_kernel)"""
    for c in DC.WGRAD_CASES:
        if c.ws:
            n, S = K.linear_wgrad_ws_floats(c.M, c.N, c.rows), DC.pick_splits(c.M, c.N, c.rows)
            assert n == (S * (c.M * c.N + c.M) if S > 1 else 0), c.id
    M, N, rows = 6, 10, 34817
    n = K.linear_wgrad_ws_floats(M, N, rows)
    assert n % (M * N + M) == 0
    S = n // (M * N + M)
    k_chunk = (-(-rows // S) + 31) & ~31
    assert (S, k_chunk) == (34, 1056)
    assert (S - 1) * k_chunk >= rows > (S - 2) * k_chunk          # exactly the last chunk is empty
    assert S - 1 > 32
    assert (S, k_chunk, S - 1) == DC.split32_closed_form(M, N, rows)


def _raw_multi(K, jobs, patch=None):
    """K.linear_multi with the job structs open to damage: patch(k, struct) edits job k before the call"""
    arr = (L.LinearJob * len(jobs))()
    for k, j in enumerate(jobs):
        a, kw = arr[k], j[-1]
        if j[0] == 'wgrad':
            _, dZ, X, dW, db, M, N, rows = j[:8]
            a.kind, a.A, a.B, a.C, a.dbias = 1, L.ptr(dZ), L.ptr(X), L.ptr(dW), L.ptr(db)
            a.lda, a.ldb, a.ldc, a.M, a.N, a.K = kw['ldz'], kw['ldx'], kw['ldw'], M, N, rows
        else:
            _, A, a_kc, B, b_kc, bias, C, M, N, Kd = j[:10]
            a.kind, a.act = 0, int(kw['act'])
            a.A, a.B, a.bias, a.C, a.relu_mask = L.ptr(A), L.ptr(B), L.ptr(bias), L.ptr(C), L.ptr(kw['relu_mask'])
            a.lda, a.ldb, a.ldc = kw['lda'], kw['ldb'], kw['ldc']
            a.a_kcontig, a.b_kcontig, a.M, a.N, a.K = int(a_kc), int(b_kc), M, N, Kd
            a.stop_flag = L.ptr(kw['stop'])
        if patch is not None:
            patch(k, a)
    L.call('smx_linear_multi_f32', arr, len(jobs), K._st())


@pytest.mark.parametrize('what', DC.REFUSALS)
def test_linear_multi_refuses_and_writes_nothing(K, what):
    lin = [c for c in DC.LINEAR_CASES if c.kernel == 'gemm32' and c.stop is None and c.values == 'int'][:10]
    wgr = [c for c in DC.WGRAD_CASES if c.rows < 500 and c.M > 1][:1]      # (M - 1 must stay a legal stride but for < M)
    cases = lin if what == 'ten-jobs' else lin[:2] + wgr
    xs = [DC.build(c, 'cuda') for c in cases]
    jobs = [DC.job_of(x) for x in xs]

    def patch(k, a):
        if what == 'kind-2' and k == 1:
            a.kind = 2
        if what == 'ldc-below-N' and k == 1:
            a.ldc = a.N - 1
        if what == 'M-zero' and k == 0:
            a.M = 0
        if what == 'wgrad-lda-below-M' and k == 2:
            a.lda = a.M - 1
    with pytest.raises(L.SmxError):
        _raw_multi(K, jobs, patch=patch)
    torch.cuda.synchronize()
    for x in xs:
        x.stopped = True                    # check(): the output region still NaN, the sentinel everywhere else
        DC.check(x)
    if what != 'ten-jobs':                  # the same structs undamaged are accepted: the refusal was the damage
        _raw_multi(K, jobs)
        for x in xs:
            x.stopped = False
            DC.check(x)
