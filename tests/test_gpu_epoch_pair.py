"""GPU tier (-m gpu): pair mode of the fused row-block epoch launches (csrc/smx_epoch.hip: every 16-row block on two
workgroups, smx_epoch_forward_pair_f32 / smx_epoch_fwdbwd_pair_f32) against the unpaired launches on the same inputs.

The bar is bit identity, compared as integers: a feature tile's arithmetic (K order, bias / activation epilogue) does not
depend on which workgroup carries it, the hand-overs move bits, and the reductions across blocks keep their order.

Shapes are the smallest at which the split can go wrong: one pair (16 rows), ragged last blocks (17, 33 rows), a layer
of ONE tile (H1 = 12: half 1 owns none of it), two tiles (20), three (H2 = 36: split 2 / 1), the benchmark's 19 / 13,
the scalar x path (D = 17), one action and seventeen, both PPO modes, both jobs together and each alone, the forward-only
launch (64 and 1024 rows: its two-job form that sorts the jobs over the XCDs) and the forward + backward launch; launches
of two DIFFERENT problems that follow each other on one exchange buffer, eagerly and replayed from a captured graph (a
word an earlier launch left in the buffer must not pass for the partner's)."""
import pytest
import torch

from surreal_amd import _lib as L
from test_gpu_epoch import build

pytestmark = pytest.mark.gpu

FWD_KEYS = ('h1aT', 'h2aT', 'h1cT', 'h2cT', 'mean', 'vpred', 'g_surr', 'g_kl', 'partials', 'v_dz3', 'v_partials')
FB_KEYS = ('h1aT', 'h2aT', 'h1cT', 'h2cT', 'mean', 'vpred', 'dz3aT', 'dz2aT', 'dz1aT', 'dz2cT', 'dz1cT', 'partials',
           'v_dz3', 'v_partials', 'stats', 'dlogvar', 'dlq')
NSYNC = 8


@pytest.fixture(scope='module')
def K():
    from surreal_amd.kernels import HipKernels
    return HipKernels()


def _problem(rows, D, H1, H2, A, mode, seed):
    t = build(rows, D, H1, H2, A, seed=seed, mode=mode, device='cuda')['d']
    t['ctrl'][L.C_KL_TARGET] = 1e9                     # (no early exit: every launch does all of its work)
    t['sync'] = torch.zeros(NSYNC, dtype=torch.int32, device='cuda')
    t['slots'] = torch.zeros(NSYNC, 2 * ((rows + 15) // 16), dtype=torch.int32, device='cuda')
    return t


def _launch(K, t, mode, jobs, kind, xchg, k=0):
    rows = t['x'].shape[0]
    loss = dict(mode=mode, rows=rows, log_var=t['log_var'], actions=t['actions'], behave=t['behave'], ref=t['ref'],
                adv=t['adv'], g_surr=t['g_surr'], g_kl=t['g_kl'], partials=t['partials'], check_stop=True,
                will_update=True, dlogvar=t['dlogvar'], dlogvar_sumsq=t['dlq'], stats=t['stats'],
                returns=t['returns'], v_dz3=t['v_dz3'], v_partials=t['v_partials'], v_will_update=True)
    aj = dict(net=t['act'], packed=t['pk_a'], x=t['x'], h1T=t['h1aT'], h2T=t['h2aT'], out=t['mean'], act=L.SMX_ACT_TANH,
              loss='policy', dz3T=t['dz3aT'], dz2T=t['dz2aT'], dz1T=t['dz1aT'])
    cj = dict(net=t['cri'], packed=t['pk_c'], x=t['x'], h1T=t['h1cT'], h2T=t['h2cT'], out=t['vpred'].view(-1, 1),
              act=L.SMX_ACT_NONE, loss='value', dz3=t['v_dz3'], dz3T=t['v_dz3'], dz2T=t['dz2cT'], dz1T=t['dz1cT'])
    js = {'both': [aj, cj], 'policy': [aj], 'value': [cj]}[jobs]
    if kind == 'fb':
        K.epoch_fwdbwd(js, loss, t['ctrl'], rows, t['sync'][k:k + 1], t['slots'][k], xchg=xchg)
    else:
        K.epoch_forward(js, loss, t['ctrl'], rows, xchg=xchg)
    return len(js)


def _poison(t, keys):
    for k in keys:
        t[k].fill_(7.0)            # (a result nobody wrote, or one left by an earlier launch, must not pass)


def _bits(v):
    return v.contiguous().view(torch.int32)


def _same(a, b, keys, what):
    for k in keys:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


def _flags(xchg, blocks):
    """[row block][half][hand-over]: hand-overs published so far"""
    return xchg[:16 * blocks].view(torch.int32).view(blocks, 2, 2)


SHAPES = [(16, 17, 12, 36, 1), (17, 376, 20, 200, 17), (33, 17, 300, 36, 17), (33, 376, 12, 200, 1),
          (64, 376, 300, 200, 17), (1024, 376, 300, 200, 17)]
CASES = [(s, m, j, kd) for s in SHAPES for kd in ('fwd', 'fb')
         for m, j in ((L.SMX_PPO_ADAPT, 'both'), (L.SMX_PPO_CLIP, 'both'), (L.SMX_PPO_ADAPT, 'policy'),
                      (L.SMX_PPO_CLIP, 'policy'), (L.SMX_PPO_CLIP, 'value'))]


@pytest.mark.parametrize('shape,mode,jobs,kind', CASES)
def test_pair_mode_has_the_bits_of_the_unpaired_launch(K, shape, mode, jobs, kind):
    rows, D, H1, H2, A = shape
    keys = FB_KEYS if kind == 'fb' else FWD_KEYS
    one = _problem(rows, D, H1, H2, A, mode, seed=rows + D + H1)
    two = _problem(rows, D, H1, H2, A, mode, seed=rows + D + H1)
    nb = (rows + 15) // 16
    blocks = nb * (2 if jobs == 'both' else 1)
    assert K.epoch_pair_fits(blocks)
    xchg = K.epoch_pair_xchg(one['act'], one['cri'])
    for t in (one, two):
        K.epoch_pack([(t['act'], t['pk_a']), (t['cri'], t['pk_c'])])
        _poison(t, keys)
    _launch(K, one, mode, jobs, kind, None)
    _launch(K, two, mode, jobs, kind, xchg)
    torch.cuda.synchronize()
    _same(two, one, keys, 'pair against unpaired')
    ci, cj = one['ctrl'].view(torch.int32), two['ctrl'].view(torch.int32)
    assert torch.equal(ci[L.C_STEP_ACTOR:], cj[L.C_STEP_ACTOR:])          # step counters, epochs done, no timeout
    assert int(cj[L.C_SYNC_ERR]) == 0
    if kind == 'fb':
        assert torch.equal(one['sync'], two['sync'])                       # every policy block counted once
        assert int(two['sync'][0]) == (nb if jobs != 'value' else 0)
    # the launch did run on pairs: every workgroup of every block published both of its hand-overs once
    assert bool((_flags(xchg, blocks) == 1).all())


POL_KEYS_SKIP = ('h1cT', 'h2cT', 'vpred', 'dz2cT', 'dz1cT', 'v_dz3', 'v_partials')


@pytest.mark.parametrize('kind', ['fwd', 'fb'])
@pytest.mark.parametrize('mode', [L.SMX_PPO_ADAPT, L.SMX_PPO_CLIP])
def test_pair_mode_launches_in_a_row_and_replayed_from_a_graph(K, mode, kind):
    """Four launches in a row on ONE exchange buffer, eagerly and then captured once and replayed twice: problem A with
    both jobs, problem B with both jobs, A's policy alone, B's policy alone.  A and B have the same shape and DIFFERENT
    inputs and weights (another seed), so what a launch finds in its partner's share of the buffer -- at every block, the
    tiles of the OTHER problem, left by the launch before it or by the previous replay -- is never what the partner is
    about to write: a reader that took a word of an earlier launch for this launch's (a tag that does not advance across
    launches or replays) would put the other problem's h1 / h2 into its tile and miss the bits of its own unpaired
    reference."""
    rows, D, H1, H2, A = 33, 376, 300, 36, 17
    keys = FB_KEYS if kind == 'fb' else FWD_KEYS
    pol_keys = [k for k in keys if k not in POL_KEYS_SKIP]
    nb = (rows + 15) // 16
    seeds = {'A': 5, 'B': 6}
    ref_both = {n: _problem(rows, D, H1, H2, A, mode, seed=sd) for n, sd in seeds.items()}
    ref_pol = {n: _problem(rows, D, H1, H2, A, mode, seed=sd) for n, sd in seeds.items()}
    t = {n: _problem(rows, D, H1, H2, A, mode, seed=sd) for n, sd in seeds.items()}
    for u in list(ref_both.values()) + list(ref_pol.values()) + list(t.values()):
        K.epoch_pack([(u['act'], u['pk_a']), (u['cri'], u['pk_c'])])
        _poison(u, keys)
    for n in seeds:
        _launch(K, ref_both[n], mode, 'both', kind, None)
        _launch(K, ref_pol[n], mode, 'policy', kind, None)
    torch.cuda.synchronize()
    assert not torch.equal(_bits(ref_both['A']['h1aT']), _bits(ref_both['B']['h1aT']))      # the problems do differ
    assert not torch.equal(_bits(ref_both['A']['h2cT']), _bits(ref_both['B']['h2cT']))
    xchg = K.epoch_pair_xchg(t['A']['act'], t['A']['cri'])
    snap = {n: {k: torch.empty_like(t[n][k]) for k in keys} for n in seeds}      # the outputs of the both-jobs launches

    def four_launches():
        for n in seeds:
            t[n]['sync'].zero_(); t[n]['slots'].zero_()
        for n in seeds:
            _launch(K, t[n], mode, 'both', kind, xchg, k=0)
            for k in keys:
                snap[n][k].copy_(t[n][k])
        for n in seeds:
            _launch(K, t[n], mode, 'policy', kind, xchg, k=1)

    def check(n_rounds, what):
        torch.cuda.synchronize()
        for n in seeds:
            _same(snap[n], ref_both[n], keys, '%s, %s: both jobs' % (what, n))
            _same(t[n], ref_pol[n], pol_keys, '%s, %s: the policy alone' % (what, n))
            assert int(t[n]['ctrl'].view(torch.int32)[L.C_SYNC_ERR]) == 0
        f = _flags(xchg, 2 * nb)         # policy blocks: four launches per round, the critic's: two
        assert bool((f[:nb] == 4 * n_rounds).all()) and bool((f[nb:] == 2 * n_rounds).all())

    four_launches()
    check(1, 'eager')
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        four_launches()
    for rep in range(2):         # (the capture itself ran nothing: the counts stand where the eager round left them)
        for n in seeds:
            _poison(t[n], keys); _poison(snap[n], keys)
        g.replay()
        check(2 + rep, 'replay %d' % rep)
