"""Cases and helpers shared by the tests of the learn's folded launches (tests/test_gpu_learn_folds.py on the device,
tests/test_learn_folds_cpu.py on the kernel double).

smx_epoch_forward_final_f32 runs the final, forward-only policy pass with the launches that used to follow it inside:
the pass's statistics (smx_epoch_backward_f32 with will_update = 0) and the end-of-learn launch
(smx_ppo_learn_epilogue_f32).  The bar is bit identity with those launches, word for word.

Shapes: D = 24, hidden 32 / 16 (two feature tiles / one, so pair mode has a half without a tile of layer 2).  Rows: one (a partial
only block), 15 / 16 / 17 (around one block), 40 (three blocks, the last partial), 130 (nine blocks: more partial rows
than the reduction has chains per column) and 600 (38 blocks; the z-update's sixteen-loads-in-flight loop, which starts
above 240 rows, and its two shorter tails).  A = 1, 3, 17: a partial row of 10, 14 and 42 words (25, 18 and 6 chains per
column in the reduction).  N = 2, 5, 128 is the stride of the step-0 observations the z-update walks (N * D floats).
Value epochs 1, 10 and 17: the last needs a second value-finalize workgroup, whose epochs are "virtual" waves 0 - 15
of 512 threads playing 1024.  Observation widths 24 and 130: one column block, and three with a partial last one."""
import itertools

import torch

from surreal_amd import _lib as L

D, H1, H2 = 24, 32, 16
ROWS = (1, 15, 16, 17, 40, 130, 600)
ACTIONS = (1, 3, 17)
STEPS = (2, 5, 128)
MODES = (L.SMX_PPO_ADAPT, L.SMX_PPO_CLIP)
# what the control block does to the pass: 'run' -- no early exit; 'stopped' -- the flag is up before the launch (a KL
# exit in an earlier epoch); 'raises' -- the pass itself exceeds 4 kl_target: the first launch raises the flag and the
# launches behind it find it up
CTRL = ('run', 'stopped', 'raises')
EPOCHS = (10, 1, 17)
ZWIDTH = (24, 24, 130)


def kernel_cases():
    """every (rows, A, mode); N, the control case, the value epochs, the observation width and the NaN column go
    round so that each value meets every row count and every A"""
    out = []
    for i, (rows, A, mode) in enumerate(itertools.product(ROWS, ACTIONS, MODES)):
        k = i + i // 6
        out.append(dict(rows=rows, A=A, mode=mode, N=STEPS[k % 3], ctrl=CTRL[(k // 2) % 3], n_epochs=EPOCHS[(k + 1) % 3],
                        Dz=ZWIDTH[(k + 2) % 3], nan=(i % 4 == 1), zfilter=(i % 7 != 3)))
    return out


def case_id(c):
    return 'r%d-A%d-%s-N%d-%s-e%d-z%d%s%s' % (c['rows'], c['A'], 'adapt' if c['mode'] == L.SMX_PPO_ADAPT else 'clip', c['N'],
                                             c['ctrl'], c['n_epochs'], c['Dz'], '-nan' if c['nan'] else '',
                                             '' if c['zfilter'] else '-noz')


class ZState(object):
    """what the kernel facade reads of a ZFilter"""

    def __init__(self, Dz, gen, device):
        self.running_sum = (3.0 * torch.randn(Dz, generator=gen)).to(device)
        self.running_sumsq = (50.0 + 10.0 * torch.rand(Dz, generator=gen)).to(device)
        self.count = torch.tensor([37.0], device=device)


def epilogue_problem(c, device='cuda'):
    """the end-of-learn launch's inputs and outputs for case c"""
    g = torch.Generator().manual_seed(1000 + c['rows'] * 7 + c['A'])
    rows, N, Dz, Ev = c['rows'], c['N'], c['Dz'], c['n_epochs']
    nblk = (rows + 15) // 16
    obs = torch.randn(rows, N, Dz, generator=g)
    if c['nan']:
        obs[rows // 2, 0, Dz // 3] = float('nan')        # one observation column: its sums and the means go NaN
    vp = torch.zeros(Ev, nblk, 8)
    vp[:, :, 0] = 16.0
    vp[:, -1, 0] = float(rows - 16 * (nblk - 1))
    vp[:, :, 1] = 0.3 * torch.randn(Ev, nblk, generator=g)
    vp[:, :, 2] = 4.0 * torch.rand(Ev, nblk, generator=g)
    vp[:, :, 3] = torch.randn(Ev, nblk, generator=g)
    vp[:, :, 4] = 9.0 * torch.rand(Ev, nblk, generator=g)
    vp[:, :, 5] = 6.0 * torch.rand(Ev, nblk, generator=g)
    e = dict(obs=obs.to(device), ret=(2.0 * torch.randn(rows, generator=g)).to(device), v_partials=vp.to(device),
             ret_mom=torch.zeros(3, device=device), v_stats=torch.zeros(Ev, L.VS_STRIDE, device=device),
             fin=torch.zeros(4, device=device), ticket=torch.zeros(2, dtype=torch.int32, device=device),
             z=ZState(Dz, g, device) if c['zfilter'] else None)
    return e


def epilogue_args(c, t, e):
    return dict(ret=e['ret'], ret_mom=e['ret_mom'], log_var=t['log_var'], out4=e['fin'], ticket=e['ticket'][0:1],
                zfilter=e['z'], x=e['obs'][:, 0, :], count_rows=c['rows'], v_partials=e['v_partials'],
                n_epochs=c['n_epochs'], nblk=e['v_partials'].shape[1], v_stats=e['v_stats'], stats_stride=L.VS_STRIDE)


POLICY_OUT = ('h1aT', 'h2aT', 'mean', 'g_surr', 'g_kl', 'partials', 'stats', 'dlogvar', 'dlq')
EPILOGUE_OUT = ('ret_mom', 'v_stats', 'fin')


def learner_case(mode, kl_target, B=40, N=5, A=3):
    return dict(name='folds', shape=dict(B=B, N=N, D=D, A=A), hidden=[H1, H2],
                hyper=dict(ppo_mode=mode, kl_target=kl_target, epoch_policy=3, epoch_baseline=3),
                batch_args={}, param_args=dict(seed=1), z_args=dict(seed=2))


FOLD_KEYS = ('fold_final_stats', 'fold_epilogue')
# learner_case's mean KL after the first policy step is about 1e-5 in both modes: 4 x this is below it, the exit is taken
# at epoch 1
EARLY_EXIT_KL_TARGET = 1e-6


class Recording(object):
    """a kernel facade that passes every call on and notes its name (what it does not have, this does not have)"""

    def __init__(self, inner):
        self._inner = inner
        self.calls = []

    def __getattr__(self, name):
        v = getattr(self._inner, name)           # AttributeError where the inner facade has no such method
        if not callable(v) or name.startswith('_'):
            return v

        def call(*a, **kw):
            self.calls.append(name)
            return v(*a, **kw)
        return call
