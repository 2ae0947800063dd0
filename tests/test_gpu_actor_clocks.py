"""GPU tier (-m gpu): episode clocks per actor in the one-launch rollouts (SyntheticVecEnv(..., episode_len=<sequence>)).

  * the table kernel (smx_actor_clock_rows_i32) against the brute-force row table;
  * actor by actor against the shared clock, bit for bit: actor a's k-th record, final state, OU state and LSTM state of
    the per-actor run equal those of today's shared-clock run with episode_len = L[a] -- same seeds, agent, draws (explicit
    eps and the attached stream) and chunks -- at 4, 8 and 16 actors per workgroup, the rows in row_table order;
  * equal clocks leave the bytes of the shared clock;
  * the n host chains (SyntheticEnv(episode_len=L[a]) behind the reference's wrappers): count, order and dones exact,
    values to the project's 1e-5;
  * ring wrap and resume; the episode monitor against the host EpisodeMonitors; one reference-sized window case.

Base shape (actor_clock_cases): n = 6, D = 7, A = 3, hidden (24, 16), L = (5, 9, 4, 13, 3, 6), calls of (7, 1, 12) steps:
22 PPO windows (n_step 4, stride 3; actor 4 none), 70 DDPG transitions (n_step 3)."""
import numpy as np
import pytest
import torch

import actor_clock_cases as CC
import ddpg_ln_rollout_cases as LC
import ddpg_rollout_cases as DC
import episode_monitor_cases as EM
import helpers as H
import ppo_window_cases as PW
import recorder_cases as RC
from surreal_amd.env import actor_clocks as AC

pytestmark = pytest.mark.gpu

TOL = 1e-5
STEPS = sum(CC.CHUNKS)
LENS8 = (5, 9, 4, 13, 3, 6, 9, 5)
LENS16 = LENS8 + (13, 4, 6, 3, 9, 5, 4, 13)
BIG = dict(n=9, D=376, A=17, hidden=(300, 200), window=(25, 20), lens=(26, 40, 25, 31, 24, 33, 50, 27, 29), chunks=(60,))


# ---- 1. the table kernel ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', ['base', 'wide'])
def test_table_kernel_equals_the_walk(case):
    from surreal_amd import kernels as KN
    if case == 'base':
        t, lens, steps, windows = np.array([2, 0, 3, 7, 1, 5]), np.array(CC.LENS), STEPS, ((4, 3), (3, 1), (4, 4))
    else:
        rs = np.random.RandomState(11)
        lens = rs.randint(1, 41, size=1030)
        t, steps, windows = (rs.rand(1030) * lens).astype(np.int64), 33, ((4, 3), (3, 1), (25, 20))
    K = KN.default_kernels()
    th, lh = t.astype(np.int32), lens.astype(np.int32)
    td, ld = torch.from_numpy(th).cuda(), torch.from_numpy(lh).cuda()
    for n_step, advance in windows:
        want, rows = AC.row_table(t, lens, steps, n_step, advance)
        got = torch.full((steps, t.size), -7, dtype=torch.int32, device='cuda')
        K.actor_clock_rows(td, ld, steps, n_step, advance, got, t_host=th, episode_len_host=lh)
        assert np.array_equal(got.cpu().numpy(), want), (case, n_step, advance)
        assert rows == int(AC.closings(t, lens, steps, n_step, advance).sum())


# ---- runs -----------------------------------------------------------------------------------------------------------

def ppo_run(episode_len, rnn_hidden=None, noise='eps', apw=0, chunks=CC.CHUNKS, n=CC.N_ACTORS, D=CC.D, A=CC.A,
            hidden=CC.HIDDEN, window=CC.PPO_WINDOW, det=False, memory_size=None, monitor=False, drain=False):
    """ppo_rollout_into over `chunks` on a fresh env and agent -> dict: 'fields' (the FIFO's windows in row order), 'rows',
    'state', 'cells' (hN, cN), 'venv'.  noise: 'eps' (explicit draws, seeded) | 'stream' (attach_noise)"""
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd.replay import FIFOReplay
    steps = sum(chunks)
    agent, (lc, ec, sc) = PW.make_agent(D, A, *window, hidden=hidden, rnn_hidden=rnn_hidden, deterministic=det,
                                        memory_size=memory_size or n * steps + 7)
    venv = SyntheticVecEnv(n, D, A, episode_len=episode_len, seeds=list(range(n)))
    eps = None
    if noise == 'stream':
        venv.attach_noise(LC.SEED)
    elif not det:
        eps = torch.randn(steps, n, A, generator=torch.Generator().manual_seed(4))
    if monitor:
        venv.attach_monitor(capacity=8)
    replay = FIFOReplay(lc, ec, sc)
    if drain:                                   # call by call: what each call wrote is popped before the next
        parts, rows, s0 = [], 0, 0
        for T in chunks:
            got, r = PW.device_windows(venv, agent, replay, [T], None if eps is None else eps[s0:s0 + T], apw)
            s0 += T
            rows += r
            if r:
                parts.append(got)
        fields = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    else:
        fields, rows = PW.device_windows(venv, agent, replay, chunks, eps, actors_per_workgroup=apw)
    torch.cuda.synchronize()
    cells = tuple(x.cpu().numpy().reshape(n, -1) for x in agent._batch_cells) if rnn_hidden else ()
    return dict(fields=fields, rows=rows, state=venv.state.cpu().numpy(), cells=cells, venv=venv, eps=eps, replay=replay)


def ddpg_run(episode_len, noise='normal', layernorm=False, attach=False, draws='eps', apw=0, chunks=CC.CHUNKS,
             n=CC.N_ACTORS, capacity=256, monitor=False, apa=4):
    """ddpg_rollout_into over `chunks` on a fresh env and agent (ddpg_ln_rollout_cases.make: n_step 3) -> dict: 'ring',
    'rows', 'state', 'ou', 'venv', 'eps' (numpy)"""
    shape = (CC.D,) + CC.HIDDEN + (CC.A,)
    agent, venv, replay, pn, cfg = LC.make(n, shape, noise=noise, layernorm=layernorm, ptype='normal' if attach else None,
                                           apa=apa, attach=attach, episode_len=episode_len, capacity=capacity)
    steps = sum(chunks)
    eps = eps_np = None
    if draws == 'stream':
        venv.attach_noise(LC.SEED)
    elif noise != 'deterministic':
        eps_np = np.random.RandomState(3).randn(steps, n, CC.A).astype(np.float32)
        eps = torch.as_tensor(eps_np).cuda()
    if monitor:
        venv.attach_monitor(capacity=8)
    rows = LC.run(agent, venv, replay, chunks, eps, actors_per_workgroup=apw)
    torch.cuda.synchronize()
    return dict(ring=H.device_ring(replay, DC.FIELDS), rows=rows, state=venv.state.cpu().numpy(),
                ou=venv._ddpg['ou'].cpu().numpy(), venv=venv, eps=eps_np, agent=agent, cfg=cfg, replay=replay)


def same_run(a, b, fields_of):
    assert a['rows'] == b['rows']
    fa, fb = fields_of(a), fields_of(b)
    assert set(fa) == set(fb)
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), k
    for k in ('state', 'ou'):
        if k in a:
            assert np.array_equal(a[k], b[k]), k
    for x, y in zip(a.get('cells', ()), b.get('cells', ())):
        assert np.array_equal(x, y)


# ---- 2. actor by actor against the shared clock ----------------------------------------------------------------------

def check_actor_by_actor(run, lens, n_step, advance, fields_of, steps=STEPS, blocks=(4, 8, 16), modes=('eps', 'stream')):
    """run(episode_len, draws, apw) -> a run dict; fields_of(run) -> {field: [rows, ...]} in row order"""
    n = len(lens)
    pairs = CC.records_of(lens, steps, n_step, advance)
    for draws in modes:
        first = None
        for apw in blocks:
            got = run(list(lens), draws, apw)
            assert got['rows'] == len(pairs)
            assert np.array_equal(got['venv'].clocks, AC.after(np.zeros(n, int), lens, steps))
            if first is None:
                first = got
            else:                               # every block size: the same bytes
                same_run(got, first, fields_of)
        mine = fields_of(first)
        for ell in sorted(set(lens)):
            ref = run(int(ell), draws, blocks[0])
            theirs, ref_pairs = fields_of(ref), CC.shared_pairs(n, int(ell), steps, n_step, advance)
            assert ref['rows'] == len(ref_pairs)
            for a in (a for a in range(n) if lens[a] == ell):
                g, w = CC.per_actor(mine, pairs, a), CC.per_actor(theirs, ref_pairs, a)
                for k in w:
                    assert g[k].shape == w[k].shape and np.array_equal(g[k], w[k]), (draws, ell, a, k)
                for k in ('state', 'ou'):
                    if k in first:
                        assert np.array_equal(first[k][a], ref[k][a]), (draws, ell, a, k)
                for x, y in zip(first.get('cells', ()), ref.get('cells', ())):
                    assert np.array_equal(x[a], y[a]), (draws, ell, a)


@pytest.mark.parametrize('rnn_hidden', [None, 10])
def test_ppo_actor_by_actor(rnn_hidden):
    check_actor_by_actor(lambda ep, draws, apw: ppo_run(ep, rnn_hidden, draws, apw), CC.LENS, 4, 3,
                         lambda r: r['fields'])
    assert ppo_run(list(CC.LENS), rnn_hidden)['rows'] == 22


def ring_rows(r):
    return {k: v[:r['rows']] for k, v in r['ring'].items()}


@pytest.mark.parametrize('noise,layernorm', [('normal', False), ('ou_noise', False), ('ou_noise', True)])
def test_ddpg_actor_by_actor(noise, layernorm):
    check_actor_by_actor(lambda ep, draws, apw: ddpg_run(ep, noise, layernorm, draws=draws, apw=apw), CC.LENS,
                         CC.DDPG_N_STEP, 1, ring_rows)
    assert ddpg_run(list(CC.LENS), noise, layernorm)['rows'] == 70


def test_ddpg_param_noise_actor_by_actor():
    # two agents of four actors, the issue's case: a block never spans two agents, so 4 per workgroup is the only size
    # the launch takes (8 and 16 do not divide 4: SMX_E_SHAPE)
    check_actor_by_actor(lambda ep, draws, apw: ddpg_run(ep, 'normal', attach=True, draws=draws, apw=apw, n=8), LENS8,
                         CC.DDPG_N_STEP, 1, ring_rows, blocks=(4,))


def test_ddpg_param_noise_agents_of_eight_actors_at_both_block_sizes():
    # two agents of eight actors: 4 and 8 per workgroup both divide them and must leave the same bytes
    check_actor_by_actor(lambda ep, draws, apw: ddpg_run(ep, 'normal', attach=True, draws=draws, apw=apw, n=16, apa=8,
                                                         capacity=512),
                         LENS16, CC.DDPG_N_STEP, 1, ring_rows, blocks=(4, 8))


def test_reference_sized_windows_actor_by_actor():
    b = BIG
    assert int(AC.closings(np.zeros(9, int), b['lens'], 60, 25, 20).sum()) == 15
    check_actor_by_actor(lambda ep, draws, apw: ppo_run(ep, None, draws, apw, chunks=b['chunks'], n=b['n'], D=b['D'],
                                                        A=b['A'], hidden=b['hidden'], window=b['window']),
                         b['lens'], 25, 20, lambda r: r['fields'], steps=60)


# ---- 3. equal clocks ----------------------------------------------------------------------------------------------

def test_equal_clocks_leave_the_shared_bytes():
    for rnn_hidden in (None, 10):
        same_run(ppo_run([9] * 6, rnn_hidden), ppo_run(9, rnn_hidden), lambda r: r['fields'])
    for noise in ('normal', 'ou_noise'):
        a, b = ddpg_run([9] * 6, noise), ddpg_run(9, noise)
        same_run(a, b, lambda r: r['ring'])
        assert a['rows'] > 0


# ---- 4. the host wrappers --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rnn_hidden,det', [(None, True), (None, False), (10, False)])
def test_ppo_windows_match_the_host_chains(rnn_hidden, det):
    got = ppo_run(list(CC.LENS), rnn_hidden, det=det)
    host_agent, cfg = PW.make_agent(CC.D, CC.A, *CC.PPO_WINDOW, hidden=CC.HIDDEN, rnn_hidden=rnn_hidden, deterministic=det)
    want, pairs = CC.host_windows(host_agent, cfg, CC.N_ACTORS, CC.D, CC.LENS, STEPS, got['eps'], device='cuda')
    assert got['rows'] == 22 == len(pairs) and pairs == CC.records_of(CC.LENS, STEPS, 4, 3)
    assert set(got['fields']) == set(want)
    for k, w in want.items():
        g = got['fields'][k].reshape(w.shape)
        if k == 'dones':
            assert np.array_equal(g, w)
        else:
            np.testing.assert_allclose(g, w, atol=TOL, rtol=0, err_msg=k)


@pytest.mark.parametrize('noise', ['deterministic', 'ou_noise'])
def test_ddpg_transitions_match_the_host_chains(noise):
    got = ddpg_run(list(CC.LENS), noise)
    lc, ec, sc = got['cfg']
    eps = got['eps'] if got['eps'] is not None else np.zeros((STEPS, CC.N_ACTORS, CC.A), np.float32)
    want, pairs = CC.host_transitions(got['agent'], lc, ec, sc, CC.N_ACTORS, CC.LENS, eps)
    assert got['rows'] == 70 == len(pairs) and pairs == CC.records_of(CC.LENS, STEPS, CC.DDPG_N_STEP, 1)
    mine = ring_rows(got)
    for k, w in want.items():
        if k == 'dones':
            assert np.array_equal(mine[k], w)
        else:
            np.testing.assert_allclose(mine[k], w, atol=TOL, rtol=0, err_msg=k)
    for k, v in got['ring'].items():
        assert not np.any(v[70:]), k                                  # never written: still zero


# ---- 5. ring wrap and resume -------------------------------------------------------------------------------------------

def test_uniform_replay_wraps_last_write_wins():
    flat = ddpg_run(list(CC.LENS), 'ou_noise')
    wrapped = ddpg_run(list(CC.LENS), 'ou_noise', capacity=64)
    assert wrapped['rows'] == 70 and len(wrapped['replay']) == 64
    want = RC.expected_ring(ring_rows(flat), 64)
    for k, w in want.items():
        assert np.array_equal(wrapped['ring'][k], w), k


def test_fifo_cursor_wraps_between_drained_calls():
    per_call, t = [], np.zeros(6, np.int64)
    for T in CC.CHUNKS:
        per_call.append(int(AC.closings(t, CC.LENS, T, 4, 3).sum()))
        t = AC.after(t, CC.LENS, T)
    memory_size = max(per_call)                                       # (the ring has memory_size + 3 rows)
    assert per_call == [7, 1, 14] and sum(per_call) == 22 > memory_size + 3     # every call fits, the cursor wraps
    for rnn_hidden in (None, 10):
        flat = ppo_run(list(CC.LENS), rnn_hidden)
        wrapped = ppo_run(list(CC.LENS), rnn_hidden, memory_size=memory_size, drain=True)
        same_run(wrapped, flat, lambda r: r['fields'])


def test_one_call_equals_the_same_steps_in_three():
    for rnn_hidden in (None, 10):
        same_run(ppo_run(list(CC.LENS), rnn_hidden, chunks=(STEPS,)), ppo_run(list(CC.LENS), rnn_hidden),
                 lambda r: r['fields'])
    for noise, ln in (('ou_noise', False), ('normal', True)):
        same_run(ddpg_run(list(CC.LENS), noise, ln, chunks=(STEPS,)), ddpg_run(list(CC.LENS), noise, ln),
                 lambda r: r['ring'])


# ---- 6. the episode monitor -------------------------------------------------------------------------------------------

def assert_polled_equals_hosts(mon, hosts, lens, what):
    """poll() against the host EpisodeMonitors of the n chains: every finished episode's length (= L[a]) and reward sum
    equal, nothing dropped; the open episodes' steps equal, their running sums within the host-parity tolerance a step"""
    mon.poll()
    for a, h in enumerate(hosts):
        print('%s actor %d: steps %s / host %s; reward sums %s / host %s' % (
            what, a, mon.episode_steps[a], h.episode_steps, mon.episode_rewards[a], h.episode_rewards))
    assert mon.dropped == 0 and len(hosts) == mon.n
    for a, h in enumerate(hosts):
        assert mon.episode_steps[a] == h.episode_steps == [lens[a]] * (STEPS // lens[a]), a
        assert mon.episode_rewards[a] == h.episode_rewards, (a, mon.episode_rewards[a], h.episode_rewards)
    assert mon.num_episodes == sum(h.num_episodes for h in hosts) == sum(STEPS // x for x in lens)
    assert mon.total_steps == sum(h.total_steps for h in hosts)
    rew, steps = mon.open_episodes()
    assert steps.tolist() == [len(h._rewards) for h in hosts] == [STEPS % x for x in lens]
    np.testing.assert_allclose(rew.numpy(), [float(sum(h._rewards)) for h in hosts], atol=max(lens) * TOL, rtol=0)


def test_ppo_monitor_equals_the_host_monitors():
    got = ppo_run(list(CC.LENS), None, monitor=True)
    host_agent, cfg = PW.make_agent(CC.D, CC.A, *CC.PPO_WINDOW, hidden=CC.HIDDEN)
    with EM.host_monitors() as hosts:
        CC.host_windows(host_agent, cfg, CC.N_ACTORS, CC.D, CC.LENS, STEPS, got['eps'], device='cuda')
    assert_polled_equals_hosts(got['venv'].monitor, hosts, CC.LENS, 'ppo')


def test_ddpg_monitor_equals_the_host_monitors():
    got = ddpg_run(list(CC.LENS), 'ou_noise', monitor=True)
    lc, ec, sc = got['cfg']
    with EM.host_monitors() as hosts:
        CC.host_transitions(got['agent'], lc, ec, sc, CC.N_ACTORS, CC.LENS, got['eps'])
    assert_polled_equals_hosts(got['venv'].monitor, hosts, CC.LENS, 'ddpg')
