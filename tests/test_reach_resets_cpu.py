"""CPU tier: the reset distribution of `reach` (surreal_amd/env/tasks.py reach_reset_state; struct smx_reset_stream).  The
host Philox against the Random123 vectors; the definition's properties; SyntheticEnv(resets=...); the host logic of
SyntheticVecEnv.attach_resets on the torch-CPU double -- the episode counter's closed form, reset(), state_dict, the
refusals, and that nothing changes while nothing is attached; the doubles against host chains bit for bit and against the
float64 restatement within the project's 1e-5; the entry points' argument checks, which run before any launch."""
import numpy as np
import pytest
import torch

import ddpg_rollout_cases as DC
import philox_ref as PR
import ppo_window_cases as PW
import reach_cases as RC
import reach_resets_cases as RR
import rollout_envelope_cases as EC
from reach_cpu_kernels import ReachCpuKernels
from reach_resets_cpu_kernels import ResetsCpuKernels
from surreal_amd import _lib as L
from surreal_amd.env import tasks as TK
from surreal_amd.env.synthetic_env import SyntheticEnv, SyntheticVecEnv


@pytest.fixture
def double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(ResetsCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the host definition -------------------------------------------------------------------------------------------------

def test_host_philox_reproduces_the_random123_vectors():
    assert len(PR.KAT) >= 3
    for counter, key, want in PR.KAT:
        got = TK.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert [int(v) for v in got] == [int(v) for v in want], (counter, key)
    # batched, against the tests' own implementation on other counters
    rs = np.random.RandomState(0)
    c = rs.randint(0, 2 ** 32, size=(7, 4), dtype=np.uint64)
    k = rs.randint(0, 2 ** 32, size=(7, 2), dtype=np.uint64)
    got = TK.philox4x32_10(c, k)
    for i in range(7):
        assert [int(v) for v in got[i]] == [int(v) for v in PR.philox4x32_10([int(v) for v in c[i]], [int(v) for v in k[i]])]


def test_reset_state_is_the_written_rule_word_for_word():
    """one row by hand from the tests' Philox: counter (g, lo e, hi e, tag | k >> 2), word k & 3, 24 bits, scaled"""
    seed, g, e, J = 0x0123456789ABCDEF, 2 ** 32 - 1, 2 ** 40 + 3, 21
    got = TK.reach_reset_state(seed, g, e, J)
    assert got.dtype == np.float32 and got.shape == (63,)
    for k in range(63):
        x = PR.philox4x32_10([g, e & 0xFFFFFFFF, e >> 32, 0x52530000 | (k >> 2)], [seed & 0xFFFFFFFF, seed >> 32])
        want = np.float32(int(x[k & 3]) >> 8) * np.float32(2.0 ** -23) - np.float32(1.0)
        if J <= k < 2 * J:
            want = np.float32(0.0)
        assert bits(got[k], want), k


def test_reset_state_properties():
    seed = RR.RSEED
    a = TK.reach_reset_state(seed, np.arange(64)[:, None], np.arange(64)[None, :], 2)          # [64, 64, 6]: 4096 rows
    assert a.shape == (64, 64, 6) and a.dtype == np.float32
    assert (a >= -1.0).all() and (a < 1.0).all()
    v = a[..., 2:4]
    assert (v == 0).all() and not np.signbit(v).any()                                            # exactly +0.0
    # element k does not depend on J's neighbours: the same (block, word) for any J -- where k is not a velocity in either
    for J in (1, 3, 21):
        b = TK.reach_reset_state(seed, 5, 9, J)
        for k in range(min(6, 3 * J)):
            if not (2 <= k < 4) and not (J <= k < 2 * J):
                assert bits(b[k], a[5, 9, k]), (J, k)
    # other actors and other episodes: other blocks
    flat = a[..., [0, 1, 4, 5]].reshape(4096, 4)
    assert len({r.tobytes() for r in flat}) == 4096
    assert not bits(TK.reach_reset_state(seed + 1, 5, 9, 2), a[5, 9])
    # 4096 draws of one element: mean 0 and variance 1/3 within 5 standard errors (uniform on [-1, 1): the variance of u
    # is 1/3, that of u^2 is 1/5 - 1/9 = 4/45)
    for k in (0, 1, 4, 5):
        u = a[..., k].reshape(-1).astype(np.float64)
        assert abs(u.mean()) <= 5 * np.sqrt(1 / 3 / 4096), (k, u.mean())
        assert abs((u ** 2).mean() - 1 / 3) <= 5 * np.sqrt(4 / 45 / 4096), (k, (u ** 2).mean())
    # scalars and arrays agree
    assert bits(TK.reach_reset_state(seed, 7, 3, 2), a[7, 3])
    for bad in (lambda: TK.reach_reset_state(seed, -1, 0, 2), lambda: TK.reach_reset_state(seed, 2 ** 32, 0, 2),
                lambda: TK.reach_reset_state(seed, 0, -1, 2), lambda: TK.reach_reset_state(1 << 64, 0, 0, 2)):
        with pytest.raises(ValueError):
            bad()


def test_host_env_draws_its_episodes():
    J, g = 2, 11
    env = SyntheticEnv(3 * J, J, episode_len=3, task='reach', resets=(RR.RSEED, g))
    assert env.episode == 0
    for e in range(4):
        obs, _ = env._reset()
        assert env.episode == e + 1 and env.t == 0
        assert bits(obs['low_dim']['flat_inputs'], TK.reach_reset_state(RR.RSEED, g, e, J))
        for _ in range(3):
            _, _, done, _ = env._step(np.ones(J, np.float32))
        assert done
    plain = SyntheticEnv(3 * J, J, episode_len=3, task='reach', seed=g)
    assert plain.resets is None and bits(plain._reset()[0]['low_dim']['flat_inputs'], plain.init_state)
    with pytest.raises(ValueError, match='no reset distribution'):
        SyntheticEnv(6, 2, resets=(1, 0))


# ---- the host logic of attach_resets on the double --------------------------------------------------------------------------

def make(c):
    return RR.setup(RR.tuned(c), 'cpu', ResetsCpuKernels(), wrap=False)


def test_reset_fills_from_the_stream_and_consumes_one_index(double):
    venv = SyntheticVecEnv(5, 6, 2, episode_len=3, device='cpu', task='reach')
    rs = venv.attach_resets(RR.RSEED, actor_base=7)
    assert venv.resets is rs and rs.episode == 0
    before = venv.state.clone()
    assert bits(rs.states().numpy(), RR.rows_of(5, 2, 7, 1)[0]) and rs.episode == 0        # (states() advances nothing)
    assert torch.equal(venv.state, before)                                                # (attaching leaves the state)
    venv.reset()
    assert rs.episode == 1 and bits(venv.state.numpy(), RR.rows_of(5, 2, 7, 1)[0])
    assert bits(rs.states(4).numpy(), RR.rows_of(5, 2, 7, 1, first=4)[0])
    rs.episode = 2 ** 40 + 3
    venv.reset()
    assert rs.episode == 2 ** 40 + 4 and bits(venv.state.numpy(), RR.rows_of(5, 2, 7, 1, first=2 ** 40 + 3)[0])
    sd = rs.state_dict()
    rs.episode = 0
    rs.load_state_dict(sd)
    assert rs.episode == 2 ** 40 + 4 and rs.state_dict() == sd
    with pytest.raises(ValueError):
        rs.load_state_dict(dict(sd, seed=1))
    with pytest.raises(ValueError):
        rs.load_state_dict(dict(sd, episode=-1))
    assert venv.detach_resets() is rs and venv.resets is None
    venv.reset()
    assert torch.equal(venv.state, venv.init_state) and rs.episode == 2 ** 40 + 4


@pytest.mark.parametrize('L_', [3, 7])
def test_step_counts_episode_ends_and_restarts_from_the_drawn_rows(double, L_):
    n, J = 5, 2
    venv = SyntheticVecEnv(n, 3 * J, J, episode_len=L_, device='cpu', task='reach')
    rs = venv.attach_resets(RR.RSEED)
    venv.reset()
    hosts = [SyntheticEnv(3 * J, J, episode_len=L_, task='reach', resets=(RR.RSEED, a)) for a in range(n)]
    for h in hosts:
        h._reset()
    acts = torch.randn(2 * L_ + 2, n, J, generator=torch.Generator().manual_seed(1))
    for s in range(acts.shape[0]):
        state = venv.step(acts[s])
        assert rs.episode == 1 + (s + 1) // L_
        for a, h in enumerate(hosts):
            obs, _, done, _ = h._step(acts[s, a].numpy())
            if done:
                obs, _ = h._reset()
            assert bits(state[a].numpy(), obs['low_dim']['flat_inputs']), (s, a)
        if (s + 1) % L_ == 0:
            assert bits(state.numpy(), rs.states(rs.episode - 1).numpy())


@pytest.mark.parametrize('c', [RC.CASES[1], RC.CASES[3], RC.CASES[6]], ids=lambda c: c.id)
def test_rollout_calls_advance_the_counter_by_the_closed_form(double, c):
    """episodes of 5 from clock 0: a call of 4 ends before an episode end, the next of 5 crosses one (and stops one
    short of the next), the last of 3 crosses one; then calls that end exactly ON an episode end"""
    x = make(c)
    venv, rs = x.venv, x.resets
    assert rs.episode == 1
    call = (lambda T, e: venv.ddpg_rollout_into(x.agent, x.replay, T, eps=e, sigmas=x.sig)) if c.family == 'ddpg' else \
        (lambda T, e: venv.ppo_rollout_into(x.agent, x.replay, T, eps=e))
    s0, want = 0, []
    for T in RC.CALLS:
        call(T, x.eps[s0:s0 + T])
        s0 += T
        want.append(1 + s0 // RC.EP)
        assert rs.episode == want[-1] and venv.t == s0 % RC.EP
    assert want == [1, 2, 3]


def test_a_call_that_ends_on_an_episode_end_counts_it(double):
    n, J = 4, 2
    agent, (lc, ec, sc) = PW.make_agent(3 * J, J, RC.N_STEP, RC.STRIDE, hidden=(8, 4))
    from surreal_amd.replay import FIFOReplay
    venv = SyntheticVecEnv(n, 3 * J, J, episode_len=5, device='cpu', task='reach')
    rs = venv.attach_resets(3)
    venv.reset()
    replay = FIFOReplay(lc, ec, sc)
    venv.ppo_rollout_into(agent, replay, 5)
    assert rs.episode == 2 and venv.t == 0 and bits(venv.state.numpy(), rs.states(1).numpy())
    venv.ppo_rollout_into(agent, replay, 10)
    assert rs.episode == 4 and bits(venv.state.numpy(), rs.states(3).numpy())


def test_refusals(double):
    drift = SyntheticVecEnv(4, 6, 2, episode_len=5, device='cpu')
    with pytest.raises(ValueError, match='no reset distribution'):
        drift.attach_resets(1)
    venv = SyntheticVecEnv(4, 6, 2, episode_len=5, device='cpu', task='reach')
    with pytest.raises(ValueError, match='2\\^32'):
        venv.attach_resets(1, actor_base=2 ** 32 - 3)
    with pytest.raises(ValueError, match='2\\^32'):
        venv.attach_resets(1, actor_base=-1)
    with pytest.raises(ValueError, match='64 bits'):
        venv.attach_resets(1 << 64)
    with pytest.raises(NotImplementedError, match='per-actor episode clocks'):
        SyntheticVecEnv(4, 6, 2, episode_len=[5, 5, 4, 3], device='cpu', task='reach').attach_resets(1)
    with pytest.raises(ValueError, match='action_dim <= 21'):
        SyntheticVecEnv(4, 66, 22, episode_len=5, device='cpu', task='reach').attach_resets(1)
    rs = venv.attach_resets(1)
    rs.episode = -1
    with pytest.raises(ValueError, match='negative'):
        venv.reset()
    rs.episode = 0
    # the calls that refuse a task env go on refusing it
    agent, _ = PW.make_agent(6, 2, 3, 2, hidden=(8, 4))
    for call in (lambda: venv.start_rollout(4), lambda: venv.rollout(agent), lambda: venv.rollout_into(agent, {}),
                 lambda: venv.emit_windows(3, 2)):
        with pytest.raises(NotImplementedError, match="task 'reach' is stepped by step"):
            call()
    with pytest.raises(NotImplementedError, match="task 'reach' is stepped by step"):
        venv.ddpg_rollout_into(DC.make_agent(*DC.configs(6, 2, 4, hidden=(8, 4))), None, 4, reference=True)
    assert rs.episode == 0


class Recording(ResetsCpuKernels):
    """every call of the three stepping doubles with its keywords"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def synth_env_step(self, *a, **kw):
        self.calls.append(('step', len(a), dict(kw)))
        return super().synth_env_step(*a, **kw)

    def synth_ppo_window_rollout(self, *a, **kw):
        self.calls.append(('ppo', len(a), dict(kw)))
        return super().synth_ppo_window_rollout(*a, **kw)

    def synth_ddpg_rollout(self, *a, **kw):
        self.calls.append(('ddpg', len(a), dict(kw)))
        return super().synth_ddpg_rollout(*a, **kw)


def test_nothing_attached_calls_the_doubles_with_the_arguments_of_before(double):
    """no `resets` keyword at all reaches a kernels object while no stream is attached -- one that knows no streams (the
    parent's ReachCpuKernels) is called as before and leaves the same bytes -- and exactly one does with one attached"""
    for c in (RC.CASES[1], RC.CASES[6]):
        c = RC.tuned(c)
        K = Recording()
        x = RC.setup(c, 'cpu', K, wrap=False)
        got = {k: v.clone() for k, v in RC.run(x)[0].items()}
        x.venv.step(torch.zeros(c.n, c.A))
        assert K.calls and all('resets' not in kw for _, _, kw in K.calls)
        old = RC.setup(c, 'cpu', ReachCpuKernels(), wrap=False)
        EC.same_bits(got, RC.run(old)[0])
        K2 = Recording()
        y = RR.setup(c, 'cpu', K2, wrap=False)
        RR.run(y)
        y.venv.step(torch.zeros(c.n, c.A))
        assert [kw.get('resets') for _, _, kw in K2.calls] == [(RR.RSEED, 0, e) for e in (1, 1, 2, 3)]
        assert [(k, na) for k, na, _ in K2.calls] == [(k, na) for k, na, _ in K.calls]
        for (_, _, kw), (_, _, kw2) in zip(K.calls, K2.calls):
            assert set(kw2) - set(kw) == {'resets'}


# ---- the doubles against the host chains and the restatement ----------------------------------------------------------------

@pytest.mark.parametrize('c', RC.CASES, ids=lambda c: c.id)
def test_restatement_meets_its_input_conditions_and_the_double_meets_it(double, c):
    c = RR.tuned(c)
    x = RR.setup(c, 'cpu', ResetsCpuKernels(), wrap=False)
    want, wrows, written, pol = RR.restatement(x)
    print(c.id, RC.input_conditions(pol, (2 if c.streams else 1) * RC.MARGIN))
    got, rows = RR.run(x)
    assert rows == wrows == x.rows
    errs = EC.worst_errors(got, want, written)
    print(c.id, {k: round(v, 3) for k, v in errs.items()})
    assert max(errs.values()) <= 1.0, errs
    assert pol.env.begun == RR.EPISODES and x.resets.episode == RR.EPISODES


def test_one_call_leaves_the_bytes_of_three_on_the_double(double):
    for c in (RC.CASES[1], RC.CASES[6]):
        a = RR.run(make(c))[0]
        b = RR.run(make(c), calls=(sum(RC.CALLS),))[0]
        EC.same_bits(a, b)


# ---- the entry points' argument checks (before any launch: no GPU here) -----------------------------------------------------

E_NULL, E_SHAPE = -1, -2              # include/surreal_amd.h: SMX_E_NULL, SMX_E_SHAPE


def test_reset_entry_points_refuse_before_any_launch():
    lib = L.load()
    fake = L.c_void_p(4096)

    def stream(base=0, episode=0, enabled=1):
        q = L.ResetStream()
        q.seed, q.actor_base, q.episode, q.enabled = 1, base, episode, enabled
        return q
    fill = lambda q, task=1, n=4, D=6: lib.smx_reset_fill_f32(q, task, n, D, fake, None)  # noqa: E731
    assert fill(stream(), task=0) == L.SMX_E_UNSUPPORTED and fill(stream(), D=7) == L.SMX_E_UNSUPPORTED
    assert fill(stream(), D=66) == L.SMX_E_UNSUPPORTED and fill(stream(), task=7) == L.SMX_E_UNSUPPORTED
    assert fill(None) == E_NULL
    assert fill(stream(base=-1)) == E_SHAPE and fill(stream(base=2 ** 32 - 3)) == E_SHAPE
    assert fill(stream(episode=-1)) == E_SHAPE and fill(stream(), n=0) == E_SHAPE
    step = lambda q, task=1: lib.smx_synth_task_env_step_resets_f32(fake, fake, fake, 4, 6, 2, 0, 5, 0, 1, None, None,  # noqa: E731
                                                                    None, None, None, task, q, None)
    assert step(stream(), task=0) == L.SMX_E_UNSUPPORTED
    assert step(stream(base=-1)) == E_SHAPE and step(stream(base=2 ** 32 - 3)) == E_SHAPE
    assert step(stream(episode=-1)) == E_SHAPE
    p, d = L.SynthPpoWindowRollout(), L.DdpgRollout()
    assert lib.smx_synth_ppo_window_rollout_resets_f32(p, 0, stream(), None) == L.SMX_E_UNSUPPORTED
    assert lib.smx_synth_ddpg_rollout_resets_f32(d, 0, stream(), None) == L.SMX_E_UNSUPPORTED
    assert lib.smx_synth_ppo_window_rollout_resets_f32(p, 7, stream(), None) == L.SMX_E_UNSUPPORTED
    assert lib.smx_synth_ddpg_rollout_resets_f32(d, 7, stream(), None) == L.SMX_E_UNSUPPORTED
    # a NULL or disabled stream is the task entry point: its codes
    for q in (None, stream(base=-1, enabled=0)):
        assert lib.smx_synth_ppo_window_rollout_resets_f32(None, 1, q, None) == \
            lib.smx_synth_ppo_window_rollout_task_f32(None, 1, None) == E_NULL
        assert lib.smx_synth_ddpg_rollout_resets_f32(None, 1, q, None) == \
            lib.smx_synth_ddpg_rollout_task_f32(None, 1, None) == E_NULL
        assert lib.smx_synth_task_env_step_resets_f32(None, fake, fake, 4, 6, 2, 0, 5, 0, 1, None, None, None, None, None,
                                                      1, q, None) == E_NULL
        assert lib.smx_synth_task_env_step_resets_f32(None, fake, fake, 4, 7, 2, 0, 5, 0, 1, None, None, None, None, None,
                                                      0, q, None) == E_NULL          # (drift forwards)
    assert lib.smx_abi_version() == 2


def test_binding_matches_the_header_struct():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'surreal_amd.h')).read()
    body = re.search(r'struct smx_reset_stream \{(.*?)\};', hdr, re.S).group(1)
    names = re.findall(r'(\w+)\s*[,;]', re.sub(r'/\*.*?\*/', '', body))
    assert names == [f[0] for f in L.ResetStream._fields_] == ['seed', 'actor_base', 'episode', 'enabled', 'reserved']
    import ctypes
    assert ctypes.sizeof(L.ResetStream) == 32


# ---- the checks the GPU tier runs on the kernels, here on the double --------------------------------------------------------

@pytest.mark.parametrize('c', [RC.CASES[0], RC.CASES[1], RC.CASES[3]], ids=lambda c: c.id)
def test_windowed_double_matches_the_host_chains_bit_for_bit(double, c):
    x = make(c)
    got, rows = RR.run(x)
    assert rows == 4 * c.n
    RR.window_chains(got, x)


@pytest.mark.parametrize('c', [RC.CASES[5], RC.CASES[6]], ids=lambda c: c.id)
def test_ddpg_double_matches_the_host_chains_bit_for_bit(double, c):
    x = make(c)
    got, rows = RR.run(x)
    assert rows == 6 * c.n
    RR.ddpg_chains(got, x)


def test_ddpg_double_whole_steps_and_monitor_returns(double):
    polled, want = RR.ddpg_whole_steps('cpu', ResetsCpuKernels())
    assert RR.polled_returns(polled, 5) == RR.rounded(want)


def test_two_envs_of_four_record_what_one_of_eight_records_on_the_double(double):
    """(the DDPG double forwards actor by actor; the windowed doubles' batched GEMMs round by batch size, so their split
    is the GPU tier's alone)"""
    (big, gb), small = RR.split_envs(RR.tuned(RC.CASES[6]), 'cpu', ResetsCpuKernels())
    RR.same_actors(gb, small, big.rows)
