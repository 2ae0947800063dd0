"""CPU tier of the rollout envelope (rollout_envelope_cases.py): the float64 restatement (rollout_fp64_ref.py) tested
without a GPU.

  * every case of the list through the existing fp32 torch doubles (TorchCpuKernels' layered path, LstmRolloutCpuKernels,
    PpoWindowCpuKernels, DdpgRolloutCpuKernels, DdpgLnRolloutCpuKernels) against the restatement, under the GPU tier's
    bound rtol = atol = 1e-5; rows, dones and the rows never written exact.  (The population has no double that perturbs
    per agent: its case checks the input conditions here, and the reference's per-agent path is anchored on its
    single-agent path and on ddpg_ln_rollout_cases.action_distance in a test of its own; the kernel on the GPU.)
  * the input conditions of every case, from the float64 reference alone;
  * the corners of the envelope as the library's queries report them;
  * every double's shape predicate equal to the library's query over a grid that straddles every limit;
  * just outside the envelope the public entry points fall back to their per-step paths (and still meet the reference),
    ppo_rollout_into raises its ValueError.
"""
import types

import numpy as np
import pytest
import torch

import rollout_envelope_cases as EC
from surreal_amd import _lib as L

IDS = [c.id for c in EC.CASES]


@pytest.mark.parametrize('c', EC.CASES, ids=IDS)
def test_double_meets_the_float64_restatement_under_the_input_conditions(c):
    with EC.on_double(c.family) as K:
        x = EC.setup(c, 'cpu', K)
        want, wrows, written, pol = EC.reference_fields(x)
        figures = EC.input_conditions(c, want, pol, written)
        if c.family == 'ddpg_pop':
            # the agents differ (their perturbed parameters do), and every call measures a distance
            acts = want['actions'][written].reshape(-1, c.n, c.A)
            assert not torch.equal(acts[:, 0:4], acts[:, 4:8])
            assert len(EC.measuring_steps(c)) == len(c.calls) and float(pol.dist.min()) > 1e-4
            return
        got, rows = EC.device_fields(x)
    assert rows == wrows
    errs = EC.worst_errors(got, want, written)
    print('%s: %s; worst error / bound %s' % (c.id, figures, {k: round(v, 4) for k, v in errs.items()}))
    assert max(errs.values()) <= 1.0, errs


def test_corners_are_what_the_queries_report():
    cor = EC.corners()
    for fam in ('ppo', 'ddpg', 'ddpg_ln'):
        assert cor[fam] == [(512, None, 640, 640, 32)], fam
    assert cor['window'] == [(512, None, 640, EC.FOUND['window_h2'], 32)]
    assert not EC.supported('window', 512, None, 640, EC.FOUND['window_h2'] + 4, 32)
    assert not EC.supported('window', 512, None, 640, 640, 32)
    for fam in ('lstm', 'lstm_window'):
        assert cor[fam] == [(EC.FOUND['lstm_d_at_128'], 128, 300, 200, 32), (512, 64, 640, EC.FOUND['lstm_h2_at_64'], 32)]
        assert EC.supported(fam, 376, 128, 300, 200, 32) and not EC.supported(fam, 512, 128, 300, 200, 32)
        assert EC.supported(fam, 512, 64, 300, 200, 32)
        assert not EC.supported(fam, EC.FOUND['lstm_d_at_128'] + 1, 128, 300, 200, 32)
        assert not any(EC.supported(fam, 512, 128, 640, h2, 32) for h2 in range(4, 644, 4))
    # every corner has a bare and a streams case at 3 and 37 actors
    for fam, shapes in cor.items():
        for ci, (D, Hl, H1, H2, A) in enumerate(shapes):
            hit = [c for c in EC.CASES if c.family == fam and (c.D, c.H, c.H1, c.H2, c.A) == (D, Hl, H1, H2, A)]
            assert sorted((c.n, c.streams) for c in hit) == [(3, False), (3, True), (37, False), (37, True)], (fam, ci)


def _ppo_model(D, Hl, H1, H2, A):
    Hp = (Hl + 3) & ~3
    actor = types.SimpleNamespace(D=Hp if Hl else D, H1=H1, H2=H2, OUT=A)
    return types.SimpleNamespace(actor=actor, if_pixel=False, if_rnn=bool(Hl), rnn_layers=1, rnn_hidden=Hp,
                                 rnn_hidden_logical=Hl, rnn=types.SimpleNamespace(D=D, H=Hp) if Hl else None)


def test_doubles_predicates_equal_the_library_queries():
    """D x H1 x H2 x A (x LSTM units, x ln) on both sides of every limit: A 32 | 33, widths multiples of 4 up to 640,
    D 512 | 513, units 128 | 132, and the LDS budget (the corners and their first refused neighbours).
    The doubles answer with the library's own query (TorchCpuKernels.lib_supported), so on the shape part this compares
    the library with itself: what it guards is that each double asks the RIGHT query with its arguments in the right
    order (the LSTM's D and padded H, not the actor's), and the conditions that are no shape: a camera, the LSTM layer
    count, an actor that sits on the LSTM's output.
    One query of the four is not mirrored: TorchCpuKernels.synth_rollout_supported answers False for every shape, because
    the double has no synth_rollout to route to -- on the CPU tier SyntheticVecEnv.rollout always walks the layered
    per-step path for a plain MLP, inside the envelope and outside it (asserted below)."""
    lib, dbl = L.load(), EC.doubles()
    Ds = (1, 17, 376, 472, 473, 512, 513)
    H1s = (4, 22, 300, 640, 644)
    H2s = (4, 30, 152, 156, 200, 600, 604, 640, 644)
    As = (1, 17, 32, 33)
    n = 0
    for D in Ds:
        for H1 in H1s:
            for H2 in H2s:
                for A in As:
                    net = types.SimpleNamespace(D=D, H1=H1, H2=H2, OUT=A)
                    for ln in (False, True):
                        want = bool(lib.smx_synth_ddpg_rollout_supported(D, H1, H2, A, int(ln)))
                        assert dbl['ddpg_ln']().synth_ddpg_rollout_supported(net, ln=ln) == want, (D, H1, H2, A, ln)
                    assert dbl['ddpg']().synth_ddpg_rollout_supported(net) == \
                        bool(lib.smx_synth_ddpg_rollout_supported(D, H1, H2, A, 0))
                    for Hl in (0, 1, 64, 125, 128, 132):
                        m = _ppo_model(D, Hl, H1, H2, A)
                        Hp = m.rnn_hidden
                        want = bool(lib.smx_synth_ppo_window_rollout_supported(D, Hp, H1, H2, A))
                        assert dbl['window']().synth_ppo_window_rollout_supported(m) == want, (D, Hl, H1, H2, A)
                        if Hl:
                            want = bool(lib.smx_synth_lstm_rollout_supported(D, Hp, H1, H2, A))
                            assert dbl['lstm']().synth_lstm_rollout_supported(m) == want, (D, Hl, H1, H2, A)
                        n += 1
    assert n == len(Ds) * len(H1s) * len(H2s) * len(As) * 6
    # what is no shape: a camera, a second LSTM layer, an actor that does not sit on the LSTM's output
    m = _ppo_model(17, 12, 64, 32, 6)
    for k, v in (('if_pixel', True), ('rnn_layers', 2)):
        bad = types.SimpleNamespace(**dict(vars(m), **{k: v}))
        assert not dbl['lstm']().synth_lstm_rollout_supported(bad) and not dbl['window']().synth_ppo_window_rollout_supported(bad)
    m.actor.D = 16
    assert not dbl['lstm']().synth_lstm_rollout_supported(m) and not dbl['window']().synth_ppo_window_rollout_supported(m)
    assert not dbl['lstm']().synth_lstm_rollout_supported(_ppo_model(17, 0, 64, 32, 6))
    for D, H1 in ((17, 64), (513, 64), (17, 644)):
        net = types.SimpleNamespace(D=D, H1=H1, H2=32, OUT=6)
        assert not any(dbl[f]().synth_rollout_supported(net) for f in ('ppo', 'lstm', 'window'))
        assert getattr(dbl['ppo'](), 'synth_rollout', None) is None


def test_population_reference_is_the_single_agent_reference_per_agent():
    """the restatement's per-agent path anchored without a GPU (no double perturbs per agent): agents given the SAME
    parameters act as the single-agent policy does on all actors; agents given different ones act as a single-agent
    policy of each on its own actors; the measured distance is ddpg_ln_rollout_cases.action_distance"""
    import ddpg_ln_rollout_cases as LN
    import rollout_fp64_ref as R
    g = torch.Generator().manual_seed(11)
    D, H1, H2, A, n, apa, eps_ln = 9, 20, 12, 3, 12, 4, 1e-5

    def params(scale):
        shapes = {'W1': (H1, D), 'b1': (H1,), 'W2': (H2, H1), 'b2': (H2,), 'W3': (A, H2), 'b3': (A,), 'ln1.W': (H1,),
                  'ln1.b': (H1,), 'ln2.W': (H2,), 'ln2.b': (H2,)}
        return {k: (scale * torch.randn(s, generator=g) + (1.0 if k.endswith('.W') and k.startswith('ln') else 0.0)).float()
                for k, s in shapes.items()}
    clean, others = params(0.4), [params(0.4) for _ in range(n // apa)]
    sig = torch.linspace(0.0, 0.5, n, dtype=torch.float64)
    state = torch.randn(n, D, generator=g, dtype=torch.float64)
    eps = torch.randn(n, A, generator=g, dtype=torch.float64)
    kw = dict(noise='ou_noise', sigmas=sig, theta=2.0, dt=0.02, ln=True, ln_eps=eps_ln)
    one = R.DdpgPolicy(clean, n, A, **kw).act(state, eps, 0)
    same = R.DdpgPolicy([clean] * (n // apa), n, A, actors_per_agent=apa, **kw).act(state, eps, 0)
    assert torch.equal(one, same)
    pop = R.DdpgPolicy(others, n, A, actors_per_agent=apa, **kw)
    pop.clean, pop.measure_at = {k: R.f64(v) for k, v in clean.items()}, (1,)
    first = pop.act(state, eps, 0)
    assert float(pop.dist.max()) == -1.0                        # act 0 measures nothing
    for p, q in enumerate(others):
        lo = p * apa
        alone = R.DdpgPolicy(q, apa, A, **dict(kw, sigmas=sig[lo:lo + apa])).act(state[lo:lo + apa], eps[lo:lo + apa], 0)
        assert torch.equal(first[lo:lo + apa], alone), p
    assert not torch.equal(first[0:apa], one[0:apa])
    pop.act(state, eps, 1)                                      # act 1 measures, at each agent's first actor
    for p, q in enumerate(others):
        want = LN.action_distance({k: v.numpy() for k, v in clean.items()}, {k: v.numpy() for k, v in q.items()},
                                  state[p * apa].numpy(), eps_ln)
        assert want > 1e-3 and abs(float(pop.dist[p]) - want) <= 1e-12 * (1 + want), (p, float(pop.dist[p]), want)


OUTSIDE = EC.outside_cases()


@pytest.mark.parametrize('c', OUTSIDE, ids=[c.id for c in OUTSIDE])
def test_outside_the_envelope_the_entries_fall_back_or_refuse(c):
    with EC.on_double(c.family) as K:
        x = EC.setup(c, 'cpu', K)
        if c.family in ('window', 'lstm_window'):
            assert not x.venv.can_ppo_rollout_into(x.agent)
            with pytest.raises(ValueError, match='policy shapes the persistent kernel refuses'):
                x.venv.ppo_rollout_into(x.agent, x.replay, c.calls[0], eps=x.eps[:c.calls[0]])
            return
        launches = []
        for name in ('synth_lstm_rollout', 'synth_ddpg_rollout'):
            if getattr(K, name, None) is not None:
                setattr(K, name, lambda *a, **k: launches.append(1))
        want, wrows, written, pol = EC.reference_fields(x)
        got, rows = EC.public_table(x) if c.family in ('ppo', 'lstm') else EC.device_fields(x)
    assert rows == wrows and not launches
    errs = EC.worst_errors(got, want, written)
    assert max(errs.values()) <= 1.0, errs
