"""CPU tier: a LayerNorm actor in SyntheticVecEnv.ddpg_rollout_into on a torch-CPU double that runs one in the launch
(ddpg_ln_rollout_cases.DdpgLnRolloutCpuKernels): which path a call takes, the one-launch double against the host
path, the perturbed parameters of a LayerNorm actor against the float64 restatement, the checkpoint, the layout of the new
argument blocks."""
import ctypes

import numpy as np
import pytest
import torch

import ddpg_ln_rollout_cases as LC
import ddpg_rollout_cases as DC
import helpers as H
import param_noise_ref as PR

SHAPE = (7, 24, 16, 3)


def use(kernels):
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(kernels, 'cpu')
    return KN, prev


@pytest.fixture
def K():
    KN, prev = use(LC.DdpgLnRolloutCpuKernels())
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


@pytest.fixture
def K_without():
    """the existing double: no LayerNorm actor in the launch (ddpg_ln_launch False)"""
    KN, prev = use(DC.DdpgRolloutCpuKernels())
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


def counted(K):
    """-> the list the env's own per-step calls of synth_ddpg_step are counted in"""
    calls = []
    orig = K.synth_ddpg_step
    K.synth_ddpg_step = lambda r, mu: (calls.append(1), orig(r, mu))
    return calls


def test_layernorm_actor_takes_one_launch_per_call(K):
    agent, venv, replay, _, _ = LC.make(3, SHAPE, device='cpu', kernels=K, capacity=64)
    steps = counted(K)
    eps = torch.randn(12, 3, 3, generator=torch.Generator().manual_seed(1))
    assert LC.run(agent, venv, replay, (5, 7), eps=eps) == 3 * LC.closing(12)
    assert [c['steps'] for c in K.ln_launches] == [5, 7] and [c['t'] for c in K.ln_launches] == [0, 5]
    assert steps == [] and venv.t == 12 % LC.EP
    # reference=True: the per-step path, one forward_actor and one step launch per step
    agent, venv, replay, _, _ = LC.make(3, SHAPE, device='cpu', kernels=K, capacity=64)
    assert LC.run(agent, venv, replay, (5, 7), eps=eps, reference=True) == 3 * LC.closing(12)
    assert len(K.ln_launches) == 2 and len(steps) == 12
    # a plain actor: the plain launch, as before
    agent, venv, replay, _, _ = LC.make(3, SHAPE, device='cpu', kernels=K, capacity=64, layernorm=False)
    LC.run(agent, venv, replay, (5,), eps=eps[:5])
    assert len(K.ln_launches) == 2


def test_kernels_without_the_entry_keep_the_per_step_path(K_without):
    agent, venv, replay, _, _ = LC.make(3, SHAPE, device='cpu', kernels=K_without, capacity=64)
    steps = counted(K_without)
    eps = torch.randn(5, 3, 3, generator=torch.Generator().manual_seed(1))
    assert LC.run(agent, venv, replay, (5,), eps=eps) == 3 * LC.closing(5)
    assert len(steps) == 5


def test_unsupported_shape_takes_the_per_step_path(K):
    agent, venv, replay, _, _ = LC.make(3, (7, 22, 16, 3), device='cpu', kernels=K, capacity=64)     # 22 % 4 != 0
    steps = counted(K)
    LC.run(agent, venv, replay, (4,), eps=torch.zeros(4, 3, 3))
    assert K.ln_launches == [] and len(steps) == 4


@pytest.mark.parametrize('shape', [SHAPE, (17, 300, 200, 6)])
def test_one_launch_double_matches_the_host_path(K, shape):
    """calls split mid-episode, OU noise: SyntheticEnv + DDPGAgent.act + the n-step wrapper, to 1e-5"""
    n, ep, calls, capacity = 3, 8, (5, 6), 40
    agent, venv, replay, _, cfg = LC.make(n, shape, device='cpu', kernels=K, capacity=capacity, episode_len=ep)
    eps_all = np.random.RandomState(3).randn(sum(calls), n, shape[3]).astype(np.float32)
    rows = LC.run(agent, venv, replay, calls, eps=torch.as_tensor(eps_all))
    want, total = DC.host_ring(agent, *cfg, n, ep, eps_all, capacity)
    assert rows == total > 0 and len(K.ln_launches) == 2
    got = H.device_ring(replay, DC.FIELDS)
    for k in DC.FIELDS:
        np.testing.assert_allclose(got[k].reshape(want[k].shape), want[k], atol=1e-5, rtol=0, err_msg=k)
    assert np.array_equal(got['dones'].reshape(want['dones'].shape), want['dones'])
    # the gains and biases matter: the plain actor of the same weights acts differently
    plain = LC.make(n, shape, device='cpu', kernels=K, capacity=capacity, episode_len=ep, layernorm=False)
    LC.run(*plain[:3], calls, eps=torch.as_tensor(eps_all))
    assert np.abs(H.device_ring(plain[2], DC.FIELDS)['actions'] - got['actions']).max() > 1e-3


def test_perturbed_parameters_of_a_layernorm_actor(K):
    agent, venv, _, pn, _ = LC.make(12, SHAPE, ptype='normal', device='cpu', kernels=K, attach=True, agent_base=2)
    assert pn.ln and pn.agents == 3 and K.ln_refreshes == [dict(generation=0, acts=0, ln=2 * (24 + 16))]
    assert K.refreshes == []
    assert pn.pop.shape == (3, K.param_noise_copy_numel(agent.model.actor, ln=True))
    plain_agent, plain_env, _, plain, _ = LC.make(12, SHAPE, ptype='normal', device='cpu', kernels=K, attach=True,
                                                  agent_base=2, layernorm=False)
    assert not plain.ln and len(K.refreshes) == 1
    clean = np.concatenate([v.reshape(-1) for v in LC.actor_params(agent).values()])
    assert clean.size == agent.model.actor_flat.numel() == agent.model.actor.numel + 80
    for q in (0, 1):
        if q:
            pn.refresh()
            plain.refresh()
        for p in range(3):
            got = pn.perturbed(p)
            assert tuple(got) == LC.ORDER
            for k in LC.LN_KEYS:
                assert got[k].shape == agent.model.actor_ln[k].shape
            flat = torch.cat([v.reshape(-1) for v in got.values()]).numpy()
            want = PR.perturbed_flat(clean, agent.param_noise_sigma, LC.PSEED, 2 + p, q)
            assert np.abs(flat.astype(np.float64) - want).max() <= 4e-7
            # the LayerNorm block is perturbed, under indices of its own
            assert np.abs(flat[-80:] - clean[-80:]).min() > 0
            # the first six blocks: what the same seed gives the plain actor of the same shape, bit for bit
            base = plain.perturbed(p)
            assert tuple(base) == PR.ORDER
            for k in PR.ORDER:
                assert torch.equal(got[k].view(torch.int32), base[k].view(torch.int32)), k


def test_state_dict_round_trip(K):
    agent, venv, _, pn, _ = LC.make(8, SHAPE, ptype='adaptive_normal', device='cpu', kernels=K, attach=True)
    pn.pop.copy_(torch.arange(pn.pop.numel(), dtype=torch.float32).view(pn.pop.shape))
    pn.sigma.mul_(2.0)
    pn.acts = 5
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in pn.state_dict().items()}
    assert set(sd) == {'sigma', 'dist', 'pop', 'generation', 'acts'}
    assert sd['pop'].shape[1] == K.param_noise_copy_numel(agent.model.actor, ln=True)
    other = LC.make(8, SHAPE, ptype='adaptive_normal', device='cpu', kernels=K, attach=True)[3]
    other.refresh()
    other.load_state_dict(sd)
    assert torch.equal(other.pop, sd['pop']) and torch.equal(other.sigma, sd['sigma'])
    assert (other.generation, other.acts) == (0, 5)
    # a plain actor's state dict loads as before
    plain = LC.make(8, SHAPE, ptype='adaptive_normal', device='cpu', kernels=K, attach=True, layernorm=False)[3]
    psd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in plain.state_dict().items()}
    assert psd['pop'].shape[1] == K.param_noise_copy_numel(None)
    plain.refresh()
    plain.acts = 3
    plain.load_state_dict(psd)
    assert (plain.generation, plain.acts) == (0, 0) and torch.equal(plain.pop, psd['pop'])


def test_population_launch_of_a_layernorm_actor_and_its_refusals(K):
    agent, venv, replay, pn, _ = LC.make(8, SHAPE, ptype='adaptive_normal', device='cpu', kernels=K, attach=True,
                                         capacity=512)
    eps = torch.zeros(7, 8, 3)
    assert LC.run(agent, venv, replay, (7,), eps=eps) == 8 * LC.closing(7)
    assert K.launches == [dict(steps=7, measure_step=0, acts=0, t=0, actors_per_workgroup=0, ln=True)] and pn.acts == 7
    with pytest.raises(NotImplementedError, match='reference=True'):
        LC.run(agent, venv, replay, (3,), eps=eps[:3], reference=True)
    agent, venv, replay, pn, _ = LC.make(8, (7, 22, 16, 3), ptype='normal', device='cpu', kernels=K, attach=True)
    with pytest.raises(NotImplementedError, match='shape'):
        LC.run(agent, venv, replay, (3,), eps=eps[:3])


def test_new_argument_blocks_match_their_ctypes_mirrors(tmp_path):
    from surreal_amd import _lib as L
    got = {}
    for cname, cls in (('struct smx_ddpg_actor_variant', L.DdpgActorVariant), ('struct smx_param_noise', L.ParamNoise)):
        sub = tmp_path / cname.split()[-1]
        sub.mkdir()
        got[cls] = H._offsets(sub, cname, cls)
        assert got[cls]['sizeof'] == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert got[cls][f] == getattr(cls, f).offset, (cname, f)
    # the LayerNorm block leads the variant; in the parameter noise it trails the existing fields, which are where they were
    assert L.DdpgActorVariant.ln.offset == 0 and L.DdpgActorVariant.ln_eps.offset == 8
    assert L.ParamNoise._fields_[-1][0] == 'ln'
    assert L.ParamNoise.ln.offset == L.ParamNoise.packed_stride.offset + 8 == ctypes.sizeof(L.ParamNoise) - 8


def test_supported_shapes_include_the_layernorm_floats():
    """host-side arithmetic, no GPU needed: the plain rule, and the LDS budget with 2 (H1 + H2) floats more"""
    from surreal_amd import _lib as L
    lib = L.load()
    for shape in LC.SHAPES:
        D, H1, H2, A = shape
        assert lib.smx_synth_ddpg_rollout_supported(D, H1, H2, A, 1) == 1
    assert lib.smx_synth_ddpg_rollout_supported(512, 640, 640, 32, 1) == 1       # the largest plain shape still fits
    assert lib.smx_synth_ddpg_rollout_supported(17, 302, 200, 6, 1) == 0
    assert lib.smx_synth_ddpg_rollout_supported(17, 644, 200, 6, 1) == 0
    assert lib.smx_synth_ddpg_rollout_supported(17, 300, 200, 33, 1) == 0
    assert lib.smx_param_noise_copy_floats(5, 12, 8, 3, 1) % 64 == 0
    assert lib.smx_param_noise_copy_floats(5, 12, 8, 3, 1) >= lib.smx_param_noise_copy_floats(5, 12, 8, 3, 0) + 40 - 63
    assert lib.smx_param_noise_copy_floats(0, 12, 8, 3, 1) == 0
