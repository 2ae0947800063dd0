"""CPU tier: the actor variants of the one-launch DDPG rollout on the `reach` task (reach_ddpg_variants_cases.py).  The
routes ddpg_rollout_into takes on a double that advertises kernels.ddpg_variant_task_launch and what it hands the launch;
the refusals that remain there; the unchanged refusal on the doubles without the capability; the float64 restatement's
input conditions at the tuned seeds, and the LayerNorm double (which runs the real actor) against it; the codes of
smx_synth_ddpg_rollout_variant_task_f32 from argument blocks whose pointers are never read; scripts/train_reach.py's new
options: where they are refused, and two chunks of the loop with both on the double."""
import ctypes
import types

import pytest
import torch

import ddpg_ln_rollout_cases as LN
import ddpg_rollout_cases as DC
import reach_cases as RC
import reach_ddpg_variants_cases as V
import rollout_envelope_cases as EC
from reach_resets_cpu_kernels import ResetsCpuKernels
from surreal_amd import _lib as L
from surreal_amd import kernels as KN
from surreal_amd.env.synthetic_env import SyntheticVecEnv

CASES = [V.tuned(c) for c in V.CASES]
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -5              # include/surreal_amd.h: SMX_E_NULL, SMX_E_SHAPE, SMX_E_ALIGN
# SyntheticVecEnv._drift_only's words for ddpg_rollout_into on task 'reach', as they were before the variants ran there
REFUSAL = ("ddpg_rollout_into with %s: task 'reach' is stepped by step(), ppo_rollout_into (a plain-MLP or one-layer LSTM "
           "policy the one-launch kernel takes) and ddpg_rollout_into's 'launch' route (a plain actor, no parameter noise), "
           "on one shared clock, only")


def refused(what):
    import re
    return dict(match='^' + re.escape(REFUSAL % what) + '$')


@pytest.fixture
def double():
    prev = KN.set_default_kernels(V.ReachVariantsCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


def test_capability_is_a_property_of_the_kernels_object():
    assert KN.ddpg_variant_task_launch(V.ReachVariantsCpuKernels()) and KN.HipKernels.ddpg_variant_task_launch is True
    for K in (ResetsCpuKernels(), LN.DdpgLnRolloutCpuKernels(), object()):
        assert not KN.ddpg_variant_task_launch(K)


# ---- the routes --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', CASES, ids=lambda c: c.id)
def test_variants_take_the_launch_route_with_variant_task_and_resets_together(double, c):
    K = double
    x = V.make(c, 'cpu', K)
    assert x.venv._ddpg_route(x.agent, False) == ('launch', None)
    rows = V.run(x)
    assert rows == x.rows == c.n * 6 and x.venv.t == sum(V.CALLS) % V.EP
    assert len(K.routes) == 3
    acts, t, episode = 0, 0, 1
    for call, T in zip(K.routes, V.CALLS):
        assert call['task'] == 'reach' and call['ln'] == c.ln and call['pn'] == bool(c.apa) and call['steps'] == T
        assert call['t'] == t
        assert call['resets'] == ((V.RSEED, 0, episode) if c.streams else None)
        if c.apa:
            # the measuring step: DeviceParamNoise.measure_step's, from the acts before the call
            want = [s for s in range(T) if (acts + s) % V.INTERVAL == 0]
            assert call['acts'] == acts and call['measure_step'] == (want[-1] if want else -1)
        else:
            assert call['measure_step'] == -1
        episode += (t + T) // V.EP
        acts, t = acts + T, (t + T) % V.EP
    if c.apa:
        assert x.pn.acts == sum(V.CALLS) and x.pn.ln == c.ln and x.pn.agents * c.apa == c.n
        assert V.measuring_acts() == (3, 6, 9)
        # refresh() and state_dict() as on 'drift'
        x.pn.refresh()
        assert K.refreshes[-1] == dict(generation=1, acts=sum(V.CALLS), adaptive=True, ln=c.ln) and x.pn.acts == 0
        sd = x.pn.state_dict()
        assert set(sd) == {'sigma', 'dist', 'pop', 'generation', 'acts'}
        x.pn.load_state_dict(sd)
    if c.streams:
        assert x.venv.resets.episode == 3


def test_plain_actor_on_the_capable_double_is_called_as_before(double):
    """no variant keyword reaches the launch for a plain actor without a noise: the bytes of the resets double"""
    c = RC.tuned(RC.CASES[6])
    got = RC.run(RC.setup(c, 'cpu', double, wrap=False))[0]
    want = RC.run(RC.setup(c, 'cpu', ResetsCpuKernels(), wrap=False))[0]
    EC.same_bits(got, want)


@pytest.mark.parametrize('c', [c for c in CASES if not c.apa], ids=lambda c: c.id)
def test_restatement_meets_its_input_conditions_and_the_layernorm_double_meets_it(double, c):
    """the double of a LayerNorm actor without a population runs the real actor in fp32: held to the project's 1e-5"""
    x = V.make(c, 'cpu', double)
    want, wrows, written, pol = V.restatement(x)
    print(c.id, RC.input_conditions(pol, V.margin_of(c)))
    assert V.run(x) == wrows == x.rows
    errs = EC.worst_errors(V.ring(x), want, written)
    print(c.id, {k: round(v, 3) for k, v in errs.items()})
    assert max(errs.values()) <= 1.0, errs


@pytest.mark.parametrize('c', [c for c in CASES if c.apa], ids=lambda c: c.id)
def test_population_restatements_meet_their_input_conditions(c):
    """(the population double steps every actor from the clean actor: only the restatement is checked here)"""
    x = V.make(c, 'cpu', V.ReachVariantsCpuKernels())
    want, wrows, written, pol = V.restatement(x)
    print(c.id, RC.input_conditions(pol, V.margin_of(c)))
    assert wrows == x.rows and int(written.sum()) == x.rows
    assert (pol.dist > 1e-4).all(), pol.dist                    # every agent measured, at a distance worth measuring


# ---- the refusals ------------------------------------------------------------------------------------------------------------

def fake_agent(**model):
    return types.SimpleNamespace(model=types.SimpleNamespace(**model))


def agents(n=8, **kw):
    return DC.make_agent(*DC.configs(6, 2, n, hidden=kw.pop('hidden', (8, 4)), **kw))


def test_refusals_that_remain_on_a_task_env(double):
    venv = SyntheticVecEnv(8, 6, 2, episode_len=5, device='cpu', task='reach')
    ln, plain = agents(layernorm=True), agents()
    pna = agents(param_noise_type='adaptive_normal')
    with pytest.raises(NotImplementedError, **refused('a camera agent')):
        venv.ddpg_rollout_into(fake_agent(is_pixel_input=True), None, 4)
    clocked = SyntheticVecEnv(8, 6, 2, episode_len=[5, 5, 4, 3, 5, 5, 4, 3], device='cpu', task='reach')
    for ag in (ln, plain):
        with pytest.raises(NotImplementedError, **refused('per-actor episode clocks')):
            clocked.ddpg_rollout_into(ag, None, 4)
        with pytest.raises(NotImplementedError, **refused("reference=True (the 'two_launch' route)")):
            venv.ddpg_rollout_into(ag, None, 4, reference=True)
    steps = "an actor shape the one-launch rollout does not take (the 'steps' route)"
    for ag in (agents(hidden=(6, 4)), agents(hidden=(6, 4), layernorm=True), agents(hidden=(644, 4), layernorm=True)):
        with pytest.raises(NotImplementedError, **refused(steps)):
            venv.ddpg_rollout_into(ag, None, 4)
    # an 'adaptive_normal' agent without an attached noise, a noise of another agent: the messages of a 'drift' env
    with pytest.raises(NotImplementedError, match="'adaptive_normal' parameter noise measures an action distance"):
        venv.ddpg_rollout_into(pna, None, 4)
    pn = venv.attach_param_noise(pna, V.PSEED)
    with pytest.raises(ValueError, match='the attached parameter noise belongs to another agent'):
        venv.ddpg_rollout_into(plain, None, 4)
    with pytest.raises(NotImplementedError, **refused("reference=True (the 'two_launch' route)")):
        venv.ddpg_rollout_into(pna, None, 4, reference=True)
    clocked.param_noise = pn
    with pytest.raises(NotImplementedError, **refused('per-actor episode clocks')):
        clocked.ddpg_rollout_into(pna, None, 4)
    # more actions than the task's kernels take
    wide = SyntheticVecEnv(8, 66, 22, episode_len=5, device='cpu', task='reach')
    with pytest.raises(ValueError, match='action_dim <= 21'):
        wide.ddpg_rollout_into(DC.make_agent(*DC.configs(66, 22, 8, hidden=(8, 4), layernorm=True)), None, 4)
    # nothing above stepped anything
    assert venv.t == 0 and pn.acts == 0 and not double.routes and torch.equal(venv.state, venv.init_state)


@pytest.mark.parametrize('K', [ResetsCpuKernels, LN.DdpgLnRolloutCpuKernels], ids=['task-double', 'layernorm-double'])
def test_kernels_without_the_capability_refuse_word_for_word(K):
    """the reach double knows no variants, the LayerNorm double no tasks: neither advertises the capability"""
    K = K()
    prev = KN.set_default_kernels(K, 'cpu')
    try:
        venv = SyntheticVecEnv(8, 6, 2, episode_len=5, device='cpu', task='reach', kernels=K)
        with pytest.raises(NotImplementedError, **refused('a LayerNorm actor')):
            venv.ddpg_rollout_into(agents(layernorm=True), None, 4)
        venv.param_noise = object()
        with pytest.raises(NotImplementedError, **refused('an attached parameter noise')):
            venv.ddpg_rollout_into(agents(), None, 4)
        assert venv.t == 0
    finally:
        KN.set_default_kernels(*prev)


# ---- the entry point's argument checks (before any launch: no GPU here) -----------------------------------------------------

def block(D=6, A=2, H1=8, H2=4, n=8, steps=4, capacity=64):
    """an argument block that passes smx_synth_ddpg_rollout_f32's checks, every pointer a fake (aligned) address"""
    fake = 4096
    net = L.Mlp3()
    for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'):
        setattr(net, k, fake)
    net.D, net.H1, net.H2, net.OUT = D, H1, H2, A
    d = L.DdpgRollout()
    d.net, d.packed = ctypes.pointer(net), fake
    d.n, d.D, d.A, d.steps, d.t, d.episode_len, d.n_step = n, D, A, steps, 0, 5, 3
    d.noise_type = L.SMX_DDPG_NOISE_NONE
    for k in ('gpow', 'state', 'init_state', 'carry_obs', 'carry_act', 'carry_rew', 'obs', 'obs_next', 'actions', 'rewards',
              'dones'):
        setattr(d, k, fake)
    d.cursor, d.capacity = 0, capacity
    d._net = net                                    # (kept alive with the block)
    return d


def stream(base=0, episode=0, enabled=1):
    q = L.ResetStream()
    q.seed, q.actor_base, q.episode, q.enabled = 1, base, episode, enabled
    return q


def variant(layernorm=False, pop=False, **kw):
    v = L.DdpgActorVariant()
    if layernorm:
        v.ln, v.ln_eps = 4096, 1e-5
    if pop:
        v.packed_pop, v.packed_stride, v.actors_per_agent, v.agents, v.measure_step, v.dist = 4096, 1 << 14, 4, 2, -1, 4096
    for k, val in kw.items():
        setattr(v, k, val)
    return v


def test_variant_task_entry_point_refuses_before_any_launch():
    lib = L.load()
    f = lib.smx_synth_ddpg_rollout_variant_task_f32
    REACH, DRIFT = L.SMX_TASK_REACH, L.SMX_TASK_DRIFT
    # an enabled stream on drift, an unknown task: before the block is looked at
    for v in (None, variant(layernorm=True), variant(pop=True)):
        assert f(block(), v, DRIFT, stream(), None) == L.SMX_E_UNSUPPORTED
        assert f(block(), v, 7, None, None) == f(None, v, 7, stream(), None) == L.SMX_E_UNSUPPORTED
    # drift without an enabled stream forwards: smx_synth_ddpg_rollout_f32's codes
    for q in (None, stream(base=-1, enabled=0)):
        assert f(None, None, DRIFT, q, None) == lib.smx_synth_ddpg_rollout_f32(None, None, None) == E_NULL
        assert f(None, variant(pop=True), REACH, q, None) == E_NULL
    for v in (None, variant(), variant(layernorm=True), variant(pop=True), variant(layernorm=True, pop=True)):
        # the block's own checks, then synth_task_ok, then reset_shape_ok
        assert f(None, v, REACH, None, None) == E_NULL
        assert f(block(D=7), v, REACH, None, None) == L.SMX_E_UNSUPPORTED            # D != 3 A
        assert f(block(D=66, A=22), v, REACH, None, None) == L.SMX_E_UNSUPPORTED     # A > 21
        assert f(block(capacity=8), v, REACH, None, None) == E_SHAPE                 # 8 actors x 2 closing steps > 8 rows
        for q in (stream(base=-1), stream(base=2 ** 32 - 3), stream(episode=-1)):
            assert f(block(), v, REACH, q, None) == E_SHAPE
    # population_args' refusals, with their codes
    pop = lambda **kw: f(block(), variant(pop=True, **kw), REACH, stream(), None)  # noqa: E731
    assert pop(actors_per_agent=6) == E_SHAPE and pop(agents=3) == E_SHAPE and pop(actors_per_agent=0) == E_SHAPE
    assert pop(measure_step=4) == E_SHAPE and pop(measure_step=-2) == E_SHAPE
    assert pop(measure_step=0, dist=None) == E_NULL
    assert pop(packed_stride=8) == E_SHAPE and pop(packed_stride=(1 << 14) + 2) == E_SHAPE
    assert pop(packed_pop=4096 + 4) == E_ALIGN
    d = block()
    d.actors_per_workgroup = 8                       # a forced block that does not divide 4 actors per agent
    assert f(d, variant(pop=True), REACH, None, None) == E_SHAPE
    # ln_args' refusals, with their codes
    for popv in (False, True):
        lnv = lambda **kw: f(block(), variant(layernorm=True, pop=popv, **kw), REACH, stream(), None)  # noqa: E731
        assert lnv(ln_eps=0.0) == E_SHAPE and lnv(ln=4096 + 2) == E_ALIGN
    assert f(block(H1=644), variant(layernorm=True), REACH, None, None) == L.SMX_E_UNSUPPORTED
    # the same refusals as the drift launch's own, where both have them
    g = lib.smx_synth_ddpg_rollout_f32
    for kw in (dict(actors_per_agent=6), dict(measure_step=4), dict(packed_pop=4096 + 4)):
        assert g(block(), variant(pop=True, **kw), None) == f(block(), variant(pop=True, **kw), REACH, None, None)
    assert lib.smx_abi_version() == 2


# ---- scripts/train_reach.py's options ------------------------------------------------------------------------------------------

def train_reach():
    import os
    import sys
    scripts = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts')
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import train_reach as TR
    return TR


def test_train_reach_refuses_the_options_where_they_do_not_apply():
    TR = train_reach()
    small = dict(actors=8, J=1, episode_len=5, iters=1, log=lambda s: None)
    with pytest.raises(ValueError, match='DDPG only'):
        TR.train('ppo', layernorm=True, **small)
    with pytest.raises(ValueError, match='DDPG only'):
        TR.train('ppo', param_noise='normal', **small)
    for kw in (dict(device_eval=True), dict(snapshot_curve=True)):
        with pytest.raises(ValueError, match='not with --device-eval / --snapshot-curve'):
            TR.train('ddpg', layernorm=True, **small, **kw)
        with pytest.raises(ValueError, match='not with --device-eval / --snapshot-curve'):
            TR.train('ddpg', param_noise='adaptive_normal', **small, **kw)


def test_train_reach_loop_refreshes_the_noise_at_every_parameter_hand_over(double, monkeypatch):
    """two chunks of the loop with both options on the double (which draws from no noise stream: none is attached): the
    LayerNorm population launch on the task per chunk, a refresh per hand-over behind the one of attach_param_noise, no
    population line for a LayerNorm population, and the run's identity names the options"""
    TR = train_reach()
    monkeypatch.setattr(SyntheticVecEnv, 'attach_noise', lambda self, seed, actor_base=0: None)
    lines = []
    base, curve = TR.train('ddpg', actors=8, J=1, episode_len=5, iters=2, eval_every=1, device='cpu', log=lines.append,
                           layernorm=True, param_noise='adaptive_normal', actors_per_agent=4)
    assert [c['iteration'] for c in curve] == [0, 1, 2] and not any('"kind"' in s for s in lines)
    launches = [r for r in double.routes if r['pn']]
    assert len(launches) == 2 and all(r['task'] == 'reach' and r['ln'] and r['steps'] == 5 for r in launches)
    assert [r['generation'] for r in double.refreshes] == [0, 1, 2] and [r['acts'] for r in double.refreshes] == [0, 5, 5]
    # without the options the identity of a saved run is what it was
    plain = TR.Loop('ddpg', 8, 1, 5, 0, 'cpu')
    assert set(plain.identity()) == {'algo', 'actors', 'J', 'episode_len', 'seed', 'random_resets', 'heldout'}
    both = TR.Loop('ddpg', 8, 1, 5, 0, 'cpu', layernorm=True, param_noise='normal', actors_per_agent=8)
    ident = both.identity()
    assert ident['param_noise'] == 'normal' and ident['actors_per_agent'] == 8 and ident['layernorm']
