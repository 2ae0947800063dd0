"""CPU tier: the host side of the device parameter-space noise (SyntheticVecEnv.attach_param_noise -> DeviceParamNoise)
on a torch-CPU double that records what the launches are handed: the measure_step arithmetic across calls and refreshes,
the block-size choice of the population launch and its refusals (the library's own host-side rule), the refusals of
ddpg_rollout_into, the flag that switches the agent's host noise off, the layout of the new argument blocks."""
import ctypes
import time

import numpy as np
import pytest
import torch

import ddpg_pixel_rollout_cases as PC
import ddpg_rollout_cases as DC
import helpers as H
import param_noise_ref as PR

D, HID, A, EP, SEED = 5, (12, 8), 3, 5, 0xD1B54A32D192ED03


class ParamNoiseCpuKernels(PC.DdpgPixelRolloutCpuKernels):
    """the double's new methods: refreshes and population launches are recorded; a population launch then steps the env
    through the double's plain rollout (one actor for all: these tests read clocks and counters, not actions)"""
    name = 'torch-cpu-double+param-noise'

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.refreshes, self.launches = [], []

    def param_noise_copy_numel(self, net, ln=False):
        return 64

    def param_noise_refresh(self, net, pn, ln=None):
        self.refreshes.append(dict(generation=pn.generation, acts=pn.acts, adaptive=pn.adaptive))

    def synth_ddpg_rollout(self, net, packed, r, steps, actors_per_workgroup=0, pn=None, measure_step=-1):
        if pn is not None:
            self.launches.append(dict(steps=steps, measure_step=measure_step, acts=pn.acts, t=int(r['t']),
                                      actors_per_workgroup=actors_per_workgroup))
        super().synth_ddpg_rollout(net, packed, r, steps, actors_per_workgroup)


@pytest.fixture
def K():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(ParamNoiseCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


def make(K, n=8, ptype='adaptive_normal', hidden=HID, layernorm=False, camera=None, **kw):
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    cfg = dict(hidden=hidden, n_step=3, param_noise_type=ptype, layernorm=layernorm, memory_size=512,
               folder='surreal_amd_param_noise_cpu')
    if camera:
        lc, ec, sc = PC.configs(D, A, n, camera[0], camera[1], **cfg)
    else:
        lc, ec, sc = DC.configs(D, A, n, **cfg)
    agent = DC.make_agent(lc, ec, sc)
    venv = SyntheticVecEnv(n, D, A, episode_len=EP, device='cpu', kernels=K,
                           **(dict(pixel=camera[0], frame_stacks=camera[1]) if camera else {}))
    return agent, venv, UniformReplay(lc, ec, sc)


def roll(agent, venv, replay, T, **kw):
    return venv.ddpg_rollout_into(agent, replay, T, eps=torch.zeros(T, venv.n, A), **kw)


def test_measure_step_across_calls_and_refreshes(K):
    agent, venv, replay = make(K)
    pn = venv.attach_param_noise(agent, SEED)
    assert (pn.agents, pn.actors_per_agent, pn.generation, pn.acts) == (2, 4, 0, 0)
    assert pn.compute_dist_interval == 10 and (pn.alpha, pn.target) == (1.15, 0.005)
    assert K.refreshes == [dict(generation=0, acts=0, adaptive=True)]
    assert pn.sigma.dtype == torch.float64 and pn.sigma.tolist() == [0.05, 0.05]
    for T in (7, 2, 3, 12):                    # clocks 0-6, 7-8, 9-11 (measures at 10), 12-23 (at 20)
        roll(agent, venv, replay, T)
    assert [(c['acts'], c['measure_step']) for c in K.launches] == [(0, 0), (7, -1), (9, 1), (12, 8)]
    assert pn.acts == 24 and [c['t'] for c in K.launches] == [0, 7 % EP, 9 % EP, 12 % EP]
    pn.refresh()
    assert K.refreshes[-1] == dict(generation=1, acts=24, adaptive=True) and (pn.generation, pn.acts) == (1, 0)
    roll(agent, venv, replay, 4)
    assert (K.launches[-1]['acts'], K.launches[-1]['measure_step']) == (0, 0)
    # an interval of 3, as the GPU tests use it; every T and every count of acts against the definition
    pn.compute_dist_interval = 3
    for acts in range(8):
        for T in range(1, 9):
            pn.acts = acts
            want = [s for s in range(T) if (acts + s) % 3 == 0]
            assert pn.measure_step(T) == (want[-1] if want else -1), (acts, T)
    # settable counters, the checkpoint's host half
    sd = pn.state_dict()
    assert set(sd) == {'sigma', 'dist', 'pop', 'generation', 'acts'}
    pn.generation, pn.acts = 9, 5
    pn.load_state_dict(sd)
    assert (pn.generation, pn.acts) == (sd['generation'], sd['acts'])
    # 'normal' never measures
    agent, venv, replay = make(K, ptype='normal')
    pn = venv.attach_param_noise(agent, SEED, actors_per_agent=8)
    roll(agent, venv, replay, 11)
    assert K.launches[-1]['measure_step'] == -1 and pn.acts == 11 and not pn.adaptive and pn.agents == 1


def test_attach_refuses_what_no_population_can_be_made_of(K):
    agent, venv, _ = make(K)
    for apa in (0, 2, 6, 16):                  # no multiple of 4, or no divisor of the 8 actors
        with pytest.raises(ValueError):
            venv.attach_param_noise(agent, SEED, actors_per_agent=apa)
    with pytest.raises(ValueError):
        venv.attach_param_noise(agent, SEED, agent_base=2 ** 32 - 1)
    with pytest.raises(ValueError):
        venv.attach_param_noise(make(K, ptype=None)[0], SEED)
    assert venv.param_noise is None and not agent.device_param_noise


def test_block_size_choice_of_the_population_launch():
    """the library's own rule (host-side arithmetic, no GPU needed): the usual block if it divides actors_per_agent, else
    the next smaller of 16 / 8 / 4; a forced block must divide"""
    from surreal_amd import _lib as L
    f = L.load().smx_synth_ddpg_population_block
    n = 1 << 17                                # more actors than 8 per CU on any chip: the usual block is 16
    assert [f(n, apa, 0) for apa in (4, 8, 12, 16, 24, 32, 64)] == [4, 8, 4, 16, 8, 16, 16]
    assert [f(8, apa, 0) for apa in (4, 8)] == [4, 4]           # a grid that fits the chip once: 4
    assert [f(n, 8, b) for b in (4, 8, 16)] == [4, 8, 0]
    assert [f(n, 16, b) for b in (4, 8, 16)] == [4, 8, 16]
    assert [f(n, 12, b) for b in (4, 8, 16)] == [4, 0, 0]
    assert f(n, 6, 0) == 0 and f(n, 0, 0) == 0 and f(n, 8, 5) == 0 and f(0, 8, 0) == 0


def test_rollout_refusals_with_a_device_parameter_noise_attached(K):
    def attached(**kw):
        agent, venv, replay = make(K, **kw)
        # (attach first reads the actor's shapes only: every case attaches)
        venv.attach_param_noise(agent, SEED)
        return agent, venv, replay
    for kw, word in ((dict(camera=((2, 20, 24), 2)), 'camera'), (dict(layernorm=True), 'LayerNorm'),
                     (dict(hidden=(12, 10)), 'shape')):
        agent, venv, replay = attached(**kw)
        with pytest.raises(NotImplementedError, match=word):
            roll(agent, venv, replay, 3)
    agent, venv, replay = attached()
    with pytest.raises(NotImplementedError, match='reference=True'):
        roll(agent, venv, replay, 3, reference=True)
    assert K.launches == []
    other = make(K)[0]
    with pytest.raises(ValueError):
        roll(other, venv, replay, 3)
    assert roll(agent, venv, replay, 3) == venv.n and len(K.launches) == 1


def test_adaptive_normal_is_still_refused_with_nothing_attached(K):
    agent, venv, replay = make(K)
    with pytest.raises(NotImplementedError, match='adaptive_normal'):
        roll(agent, venv, replay, 3)
    pn = venv.attach_param_noise(agent, SEED)
    assert roll(agent, venv, replay, 3) == venv.n
    assert venv.detach_param_noise() is pn and venv.param_noise is None
    with pytest.raises(NotImplementedError, match='adaptive_normal'):
        roll(agent, venv, replay, 3)
    # 'normal' with nothing attached: the plain launch, as before
    agent, venv, replay = make(K, ptype='normal')
    assert roll(agent, venv, replay, 3) == venv.n and len(K.launches) == 1


def test_attach_switches_the_agents_host_noise_off(K):
    agent, venv, _ = make(K, ptype='normal')
    calls = []
    agent.param_noise.apply = lambda params: calls.append(1) or params
    params = {'ddpg': {k: v.detach().cpu().numpy() for k, v in agent.model.named_parameters().items()}}
    agent.on_parameter_fetched(params, {'time': time.time()})
    assert calls == [1] and not agent.device_param_noise
    venv.attach_param_noise(agent, SEED)
    assert agent.device_param_noise
    agent.on_parameter_fetched(params, {'time': time.time()})
    assert calls == [1]
    venv.detach_param_noise()
    agent.on_parameter_fetched(params, {'time': time.time()})
    assert calls == [1, 1]


def test_new_argument_blocks_match_their_ctypes_mirrors(tmp_path):
    from surreal_amd import _lib as L
    for cname, cls in (('struct smx_param_noise', L.ParamNoise), ('struct smx_ddpg_actor_variant', L.DdpgActorVariant),
                       ('smx_ddpg_rollout_t', L.DdpgRollout)):
        sub = tmp_path / cname.split()[-1]
        sub.mkdir()
        got = H._offsets(sub, cname, cls)
        assert got['sizeof'] == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert got[f] == getattr(cls, f).offset, (cname, f)
    # smx_ddpg_rollout_t is what it was, `mon` its last member: the variant travels beside it, not behind it
    assert L.DdpgRollout._fields_[-1][0] == 'mon'
    assert L.DdpgRollout.mon.offset + ctypes.sizeof(L.EpisodeMonitor) == ctypes.sizeof(L.DdpgRollout)


SMX_E_NULL, SMX_E_SHAPE, SMX_E_ALIGN = -1, -2, -5


def test_actor_variant_is_refused_before_any_launch():
    """the one rollout entry point's checks of struct smx_ddpg_actor_variant (host side: no GPU needed, and nothing a
    launch could succeed on -- every pointer is a fake)"""
    from surreal_amd import _lib as L
    lib = L.load()
    fake = ctypes.c_void_p(4096)
    net = L.Mlp3()
    for f in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'):
        setattr(net, f, fake)
    net.D, net.H1, net.H2, net.OUT = 17, 300, 200, 6      # (1000 LayerNorm floats: the two copies differ in size)
    p = L.DdpgRollout()
    for f in ('packed', 'state', 'init_state', 'gpow', 'carry_obs', 'carry_act', 'carry_rew', 'obs', 'obs_next',
              'actions', 'rewards', 'dones'):
        setattr(p, f, fake)
    p.net = ctypes.pointer(net)
    p.n, p.D, p.A, p.steps, p.n_step, p.episode_len, p.capacity = 8, 17, 6, 9, 3, 11, 4096

    def rc(**fields):
        v = L.DdpgActorVariant()
        for k, x in fields.items():
            setattr(v, k, x)
        return lib.smx_synth_ddpg_rollout_f32(ctypes.byref(p), ctypes.byref(v), None)
    copy = {ln: lib.smx_param_noise_copy_floats(17, 300, 200, 6, ln) for ln in (0, 1)}
    assert copy[1] > copy[0] > 0
    pop = dict(packed_pop=fake, actors_per_agent=4, agents=2, measure_step=-1, packed_stride=copy[1])
    assert rc(ln=fake, ln_eps=0.0) == SMX_E_SHAPE and rc(ln=fake, ln_eps=-1e-5) == SMX_E_SHAPE
    assert rc(ln=ctypes.c_void_p(4098), ln_eps=1e-5) == SMX_E_ALIGN
    # the stride bound is that of the ln actually passed
    assert rc(**dict(pop, packed_stride=copy[0] - 4)) == SMX_E_SHAPE
    assert rc(**dict(pop, packed_stride=copy[1] - 4, ln=fake, ln_eps=1e-5)) == SMX_E_SHAPE
    # (a plain population takes the plain copy's stride: it gets as far as the next check, the copies' alignment)
    assert copy[1] - 4 >= copy[0] and rc(**dict(pop, packed_stride=copy[0], packed_pop=ctypes.c_void_p(4104))) == SMX_E_ALIGN
    assert rc(**dict(pop, measure_step=0)) == SMX_E_NULL and rc(**dict(pop, measure_step=0, ln=fake, ln_eps=1e-5)) == SMX_E_NULL
    assert rc(**dict(pop, agents=3)) == SMX_E_SHAPE and rc(**dict(pop, actors_per_agent=8)) == SMX_E_SHAPE


def test_restatement_uses_the_fixed_fourth_counter_word():
    import philox_ref as P
    g, q, i = 7, 3, 9
    x = P.philox4x32_10((g, q, i >> 2, 0x504E0001), (SEED & P.MASK, SEED >> 32))
    u0, u1 = ((x[0] >> 8) + 0.5) * 2.0 ** -24, ((x[1] >> 8) + 0.5) * 2.0 ** -24
    want = np.sqrt(-2 * np.log(u0)) * np.sin(2 * np.pi * u1)             # i & 3 == 1: the first pair's sine
    assert abs(float(PR.normal(SEED, g, q, [i])[0]) - want) < 1e-15
    flat = np.linspace(-1, 1, 11).astype(np.float32)
    p = PR.perturbed_flat(flat, 0.05, SEED, g, q)
    assert np.allclose((p - flat) / float(np.float32(0.05)), PR.normal(SEED, g, q, np.arange(11)))
