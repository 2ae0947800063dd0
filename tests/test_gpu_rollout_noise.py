"""GPU tier (-m gpu): the rollouts' exploration noise drawn on the device from per-actor Philox streams
(struct smx_noise_stream, SyntheticVecEnv.attach_noise -> DeviceNoise).

  * smx_noise_fill_f32 against the numpy float64 restatement (noise_ref.py) at atol 1e-5 -- the project's parity bar;
    the fp32 chain (logf, sqrtf, sincospif, one product) is a few ulp of a value no larger than 5.89: below ~5e-6 --
    at the top actor ids and across a carry into the counter's high step word; the moments and the bound of 2^20 device
    draws; SMX_E_SHAPE for global actor ids past 2^32;
  * per launch path: a run with the stream attached and eps=None leaves exactly the bytes of a run without a stream
    that is handed eps = draws(T, n, A) -- tables or ring, state, LSTM cells, OU state, carry rings, monitor;
  * continuity (calls of 3 + 4 steps == one call of 7), sharding (two envs of 4 actors == one env of 8, actor by
    actor), precedence of an explicit eps, the deterministic agent modes, reset() and the settable counter.

Shapes: the smallest that reach the kernels' edges -- n = 6 actors (a partial 4-actor block), A = 6 (the second Philox
block half used), episode_len 5 against T = 7 (a call crosses an episode end), windows (3, 2), DDPG n_step 3; the
camera 3 x 20 x 20 (the smallest frame the CNN stem takes), frame_stacks 2."""
import numpy as np
import pytest
import torch

import ddpg_pixel_rollout_cases as DPC
import ddpg_rollout_cases as DC
import episode_monitor_cases as EM
import helpers as H
import lstm_rollout_cases as LC
import noise_ref as NR
import ppo_pixel_window_cases as PPC
import ppo_window_cases as PW

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15          # (both key words in use)
N, D, A, HID, RNN = 6, 12, 6, (16, 8), 8
EP, T = 5, 7
N_STEP, STRIDE = 3, 2
CAMERA = ((3, 20, 20), 2)
BASE, STEP0 = 5, 3                 # a stream that starts neither at actor 0 nor at step 0


@pytest.fixture
def K():
    from surreal_amd import kernels as KN
    return KN.default_kernels()


def same_bytes(a, b):
    assert set(a) == set(b), (sorted(a), sorted(b))
    for k in a:
        x, y = a[k].contiguous(), b[k].contiguous()
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k


def _env(n=N, d=D, a=A, camera=None, seeds=None, monitor=True):
    from surreal_amd.env import SyntheticVecEnv
    venv = SyntheticVecEnv(n, d, a, episode_len=EP, seeds=list(range(n)) if seeds is None else list(seeds),
                           **(dict(pixel=camera[0], frame_stacks=camera[1]) if camera else {}))
    if monitor:
        venv.attach_monitor(capacity=4)
    return venv


def _arm(venv, how, seed=SEED, base=BASE, step=STEP0):
    """how 'stream': the stream attached at (base, step) -> None (the calls get no eps); how 'explicit': no stream ->
    a function T -> the [T, n, A] draws the streamed run's next T steps use (its own counter, advanced here)"""
    if how == 'stream':
        venv.attach_noise(seed, actor_base=base).step = step
        return lambda steps: None
    from surreal_amd.env import DeviceNoise
    src = DeviceNoise(seed, base, venv.n, venv.A, venv.K, venv.device)
    src.step = step

    def take(steps):
        e = src.draws(steps)
        src.step += steps
        return e
    return take


def _final(venv, extra):
    torch.cuda.synchronize()
    out = {k: v.detach().cpu() for k, v in extra.items() if v is not None}
    out['state'] = venv.state.cpu()
    if venv.monitor is not None:
        out.update({'mon_' + k: v for k, v in EM.monitor_state(venv.monitor).items()})
    return out


# ---- the fill kernel against the restatement ---------------------------------------------------------------------------

def test_fill_matches_the_restatement_at_the_top_ids_and_across_the_step_carry(K):
    steps, n, a = 3, 5, 6
    base, step = 2 ** 32 - 5, 2 ** 32 - 1
    out = torch.empty(steps, n, a, device='cuda')
    K.noise_fill((SEED, base, step), out)
    want = NR.draws(SEED, base, step, steps, n, a)
    d = float(np.abs(out.cpu().numpy().astype(np.float64) - want).max())
    print('smx_noise_fill_f32 against the float64 restatement: max |difference| %.3g (atol 1e-5)' % d)
    assert d <= 1e-5
    # a draw is a function of (g, s, j) alone: the same numbers through another tensor shape
    one = torch.empty(1, 1, 2, device='cuda')
    K.noise_fill((SEED, base + 4, step + 2), one)
    assert torch.equal(one[0, 0], out[2, 4, :2])


def test_fill_moments_and_bound_on_the_device(K):
    out = torch.empty(64, 1024, 16, device='cuda')          # 2^20 draws
    K.noise_fill((SEED, 0, 0), out)
    z = out.cpu().numpy()
    NR.moments_ok(z)
    d = float(np.abs(z[:4].astype(np.float64) - NR.draws(SEED, 0, 0, 4, 1024, 16)).max())
    assert d <= 1e-5, d


def test_fill_and_launches_refuse_actor_ids_past_32_bits(K):
    from surreal_amd._lib import SmxError
    out = torch.empty(1, 5, A, device='cuda')
    K.noise_fill((SEED, 2 ** 32 - 5, 0), out)
    for base in (2 ** 32 - 4, -1):
        with pytest.raises(SmxError, match='rc=-2 '):           # SMX_E_SHAPE
            K.noise_fill((SEED, base, 0), out)
    # a launch with the stream enabled checks the same
    agent = _mlp_agent()[0]
    venv = _env(n=5)
    _tables(venv, T, A)
    with pytest.raises(SmxError, match='rc=-2 '):
        K.synth_rollout(agent.model.actor, venv._pack_actor(agent.model.actor), 2, venv.state, venv.init_state,
                        agent.model.log_var.view(-1), None, None, 0, EP, T, 0, venv.rolls, None,
                        noise=(SEED, 2 ** 32 - 4, 0))
    venv = _env(n=5)
    with pytest.raises(ValueError):
        venv.attach_noise(SEED, actor_base=2 ** 32 - 4)


# ---- rollout() / rollout_into(): the rollout tables ------------------------------------------------------------------

def _mlp_agent(d=D, a=A, mode='training'):
    from surreal_amd.agent import PPOAgent
    from surreal_amd import synthetic
    lc, ec, sc = PW.configs(d, a, N_STEP, STRIDE, HID, None, True, 4096, None)
    agent = PPOAgent(lc, ec, sc, agent_id=1, agent_mode=mode)
    agent.model.load_params(synthetic.make_ppo_params(d, a, hidden=HID, seed=3, final_scale=2.0, log_sig_spread=0.4))
    agent.model.z_filter.load_state_dict(synthetic.make_zfilter_state(d, seed=4))
    return agent, (lc, ec, sc)


def _tables(venv, steps, a):
    f = lambda *s: torch.zeros(*s, device='cuda')  # noqa: E731
    venv.T, venv.slot = steps, 0
    venv.rolls = {'obs': f(venv.n, steps + 1, venv.D), 'actions': f(venv.n, steps + 1, a),
                  'rewards': f(venv.n, steps + 1), 'dones': f(venv.n, steps + 1), 'pds': f(venv.n, steps + 1, 2 * a)}


def _rollout(how, path, apw=0):
    """rollout() over T steps (tables of T + 1 rows laid out by hand: the call crosses an episode end) -> every output"""
    d, a = (36, 33) if path == 'four_launch' else (D, A)        # (A > 32: the step launch that is handed the mean)
    lstm = path in ('lstm', 'stem')
    agent = LC.make_agent(d, a, HID, RNN, T=T, n=N)[0] if lstm else _mlp_agent(d, a)[0]
    venv = _env(d=d, a=a)
    venv.persistent = path in ('persistent', 'lstm')
    take = _arm(venv, how)
    _tables(venv, T, a)
    venv.rollout(agent, eps=take(T), actors_per_workgroup=apw)
    extra = dict(venv.rolls)
    if lstm:
        extra.update(hN=agent._batch_cells[0], cN=agent._batch_cells[1])
    return _final(venv, extra), venv


@pytest.mark.parametrize('path,apw', [('persistent', 0), ('persistent', 16), ('head_launch', 0), ('four_launch', 0),
                                      ('lstm', 0), ('stem', 0)])
def test_rollout_draws_in_the_launch_what_the_fill_kernel_hands_out(K, path, apw):
    streamed, venv = _rollout('stream', path, apw)
    explicit, _ = _rollout('explicit', path, apw)
    same_bytes(streamed, explicit)
    assert venv.noise.step == STEP0 + T and float(streamed['actions'][:, :T].abs().sum()) > 0
    assert int(streamed['mon_ep_count'][0]) == 1


def _rollout_into(how, lstm):
    agent = LC.make_agent(D, A, HID, RNN, T=EP, n=N)[0] if lstm else _mlp_agent()[0]
    venv = _env()
    take = _arm(venv, how)
    f = lambda *s: torch.zeros(*s, device='cuda')  # noqa: E731
    out = {'obs': f(N, EP, D), 'obs_next': f(N, 1, D), 'actions': f(N, EP, A), 'rewards': f(N, EP), 'dones': f(N, EP),
           'pds': f(N, EP, 2 * A)}
    if lstm:
        out['cells'] = f(N, 2, 1, RNN)
    assert venv.can_rollout_into(agent)
    venv.rollout_into(agent, out, eps=take(EP))
    return _final(venv, out), venv


@pytest.mark.parametrize('lstm', [False, True])
def test_rollout_into_draws_in_the_launch(K, lstm):
    streamed, venv = _rollout_into('stream', lstm)
    same_bytes(streamed, _rollout_into('explicit', lstm)[0])
    assert venv.noise.step == STEP0 + EP and float(streamed['dones'][:, -1].sum()) == N


# ---- ppo_rollout_into -------------------------------------------------------------------------------------------------

def _ppo(how, kind, chunks=(T,), n=N, seeds=None, base=BASE, mode=None, apw=0, eps_over=None):
    """ppo_rollout_into over `chunks` -> (ring, carried state and monitor, venv).  kind: 'mlp' | 'lstm' | 'camera'"""
    from surreal_amd.replay import FIFOReplay
    camera = CAMERA if kind == 'camera' else None
    kw = dict(hidden=HID, rnn_hidden=RNN if kind == 'lstm' else None, memory_size=n * sum(chunks) + 7)
    if camera:
        agent, (lc, ec, sc) = PPC.make_agent(D, A, N_STEP, STRIDE, camera[0], camera[1], feat=12, final_scale=1.0, **kw)
    else:
        agent, (lc, ec, sc) = PW.make_agent(D, A, N_STEP, STRIDE, **kw)
    if mode is not None:
        agent.set_agent_mode(mode)              # (before the first batch_noise(): the per-actor scales follow the mode)
    venv = _env(n=n, camera=camera, seeds=seeds)
    take = _arm(venv, how, base=base) if how != 'none' else (lambda steps: None)
    replay = FIFOReplay(lc, ec, sc)
    for steps in chunks:
        venv.ppo_rollout_into(agent, replay, steps, eps=take(steps) if eps_over is None else eps_over(steps),
                              actors_per_workgroup=apw)
    extra = dict(venv._ppo['carry'])
    if kind == 'lstm':
        extra.update(hN=agent._batch_cells[0], cN=agent._batch_cells[1])
    final = _final(venv, extra)
    ring = {k: torch.as_tensor(v) for k, v in H.device_ring(replay).items()}
    return ring, final, venv


@pytest.mark.parametrize('kind', ['mlp', 'lstm', 'camera'])
def test_ppo_windows_draw_in_the_launch(kind):
    ring, final, venv = _ppo('stream', kind)
    ring_e, final_e, _ = _ppo('explicit', kind)
    same_bytes(ring, ring_e)
    same_bytes(final, final_e)
    assert venv.noise.step == STEP0 + T and float(ring['actions'].abs().sum()) > 0


@pytest.mark.parametrize('kind', ['mlp', 'lstm', 'camera'])
def test_ppo_split_calls_continue_the_stream(kind):
    """3 then 4 steps == 7 steps: nothing is passed, the counter carries like the open windows"""
    ring, final, _ = _ppo('stream', kind, chunks=(3, 4))
    ring_1, final_1, _ = _ppo('stream', kind, chunks=(7,))
    same_bytes(ring, ring_1)
    same_bytes(final, final_1)


# ---- ddpg_rollout_into ------------------------------------------------------------------------------------------------

def _ddpg(how, noise_type='normal', layernorm=False, camera=None, chunks=(T,), n=N, seeds=None, base=BASE, sigmas=None,
          mode='training', eps_over=None):
    from surreal_amd.replay import UniformReplay
    capacity = n * sum(chunks) + 7
    kw = dict(hidden=HID, n_step=3, noise_type=noise_type, layernorm=layernorm, memory_size=capacity, theta=2.0, dt=0.05)
    if camera:
        lc, ec, sc = DPC.configs(D, A, n, camera[0], camera[1], feat=12, **kw)
    else:
        lc, ec, sc = DC.configs(D, A, n, **kw)
    agent = DC.make_agent(lc, ec, sc, mode=mode, w3_scale=1.0)
    venv = _env(n=n, camera=camera, seeds=seeds)
    take = _arm(venv, how, base=base) if how != 'none' else (lambda steps: None)
    replay = UniformReplay(lc, ec, sc)
    for steps in chunks:
        venv.ddpg_rollout_into(agent, replay, steps, eps=take(steps) if eps_over is None else eps_over(steps),
                               sigmas=sigmas)
    final = _final(venv, {k: venv._ddpg[k] for k in ('ou', 'carry_obs', 'carry_act', 'carry_rew')})
    ring = {k: torch.as_tensor(v) for k, v in H.device_ring(replay).items()}
    return ring, final, venv


DDPG_PATHS = {'persistent_gaussian': dict(noise_type='normal'), 'persistent_ou': dict(noise_type='ou_noise'),
              'per_step_layernorm': dict(noise_type='ou_noise', layernorm=True),
              'camera': dict(noise_type='ou_noise', camera=CAMERA)}


@pytest.mark.parametrize('path', sorted(DDPG_PATHS))
def test_ddpg_draws_in_the_launch(path):
    ring, final, venv = _ddpg('stream', **DDPG_PATHS[path])
    ring_e, final_e, _ = _ddpg('explicit', **DDPG_PATHS[path])
    same_bytes(ring, ring_e)
    same_bytes(final, final_e)
    assert venv.noise.step == STEP0 + T
    # the noise is there: the same run without exploration leaves other actions
    quiet = _ddpg('none', mode='eval_deterministic_local', **DDPG_PATHS[path])[0]
    assert not torch.equal(ring['actions'], quiet['actions'])


@pytest.mark.parametrize('path', ['persistent_ou', 'per_step_layernorm'])
def test_ddpg_split_calls_continue_the_stream(path):
    ring, final, _ = _ddpg('stream', chunks=(3, 4), **DDPG_PATHS[path])
    ring_1, final_1, _ = _ddpg('stream', chunks=(7,), **DDPG_PATHS[path])
    same_bytes(ring, ring_1)
    same_bytes(final, final_1)


# ---- sharding ---------------------------------------------------------------------------------------------------------

def _rows_by_actor(ring, n, rows):
    """ring rows 0 .. rows - 1 are (closing step k, actor a) at k n + a -> {field: [closing steps, n, width]}"""
    return {k: v[:rows].reshape(rows // n, n, -1) for k, v in ring.items()}


def test_ppo_shards_see_the_whole_envs_noise():
    """8 actors in one env against 4 + 4 in two (actor_base 0 and 4), an eval_stochastic_local agent (every actor's
    scale 1, and it samples): actor g's windows are the same bytes"""
    kw = dict(mode='eval_stochastic_local', apw=4)
    whole, fw, _ = _ppo('stream', 'mlp', n=8, seeds=range(8), base=0, **kw)
    closing = sum(1 for t in _clock(T) if t + 1 >= N_STEP and (t + 1 - N_STEP) % STRIDE == 0)
    w = _rows_by_actor(whole, 8, 8 * closing)
    assert float(w['actions'].abs().sum()) > 0
    for base in (0, 4):
        shard, fs, _ = _ppo('stream', 'mlp', n=4, seeds=range(base, base + 4), base=base, **kw)
        s = _rows_by_actor(shard, 4, 4 * closing)
        for k in w:
            assert torch.equal(w[k][:, base:base + 4], s[k]), (k, base)
        assert torch.equal(fw['state'][base:base + 4], fs['state'])


def test_ddpg_shards_see_the_whole_envs_noise():
    sig = torch.linspace(0.1, 0.8, 8, dtype=torch.float64, device='cuda')
    closing = sum(1 for t in _clock(T) if t >= 2)
    whole, fw, _ = _ddpg('stream', 'ou_noise', n=8, seeds=range(8), base=0, sigmas=sig)
    w = _rows_by_actor(whole, 8, 8 * closing)
    for base in (0, 4):
        shard, fs, _ = _ddpg('stream', 'ou_noise', n=4, seeds=range(base, base + 4), base=base,
                             sigmas=sig[base:base + 4].clone())
        s = _rows_by_actor(shard, 4, 4 * closing)
        for k in w:
            assert torch.equal(w[k][:, base:base + 4], s[k]), (k, base)
        for k in ('state', 'ou', 'carry_act'):
            assert torch.equal(fw[k][base:base + 4], fs[k]), (k, base)


def _clock(steps, t=0):
    out = []
    for _ in range(steps):
        out.append(t)
        t = 0 if t + 1 >= EP else t + 1
    return out


# ---- precedence, modes, reset, the counter ------------------------------------------------------------------------------

def test_explicit_eps_wins_and_still_moves_the_counter():
    eps = torch.randn(T, N, A, generator=torch.Generator().manual_seed(5)).cuda()
    for run in (lambda how: _ppo(how, 'mlp', eps_over=lambda s: eps), lambda how: _ddpg(how, 'ou_noise', eps_over=lambda s: eps)):
        ring, final, venv = run('stream')
        ring_n, final_n, _ = run('none')
        same_bytes(ring, ring_n)
        same_bytes(final, final_n)
        assert venv.noise.step == STEP0 + T


def test_deterministic_modes_draw_nothing_from_the_stream():
    ring, final, venv = _ppo('stream', 'mlp', mode='eval_deterministic_local')
    ring_n, final_n, _ = _ppo('none', 'mlp', mode='eval_deterministic_local')
    same_bytes(ring, ring_n)
    same_bytes(final, final_n)
    ring, final, _ = _ddpg('stream', mode='eval_deterministic_local')
    ring_n, final_n, _ = _ddpg('none', mode='eval_deterministic_local')
    same_bytes(ring, ring_n)
    same_bytes(final, final_n)


def test_reset_keeps_the_counter_and_a_set_counter_repeats_the_draws():
    from surreal_amd.replay import FIFOReplay
    agent, (lc, ec, sc) = PW.make_agent(D, A, N_STEP, STRIDE, hidden=HID, memory_size=4096)
    venv = _env()
    noise = venv.attach_noise(SEED, actor_base=BASE)

    def run():
        replay = FIFOReplay(lc, ec, sc)
        venv.ppo_rollout_into(agent, replay, T)
        torch.cuda.synchronize()
        return {k: torch.as_tensor(v) for k, v in H.device_ring(replay).items()}
    first = noise.draws(T)
    a = run()
    assert noise.step == T
    venv.reset()
    assert noise.step == T                         # a new episode gets new noise
    assert not torch.equal(noise.draws(T), first)
    b = run()
    assert noise.step == 2 * T and not torch.equal(a['actions'], b['actions'])
    venv.reset()
    noise.step = 0                                 # resume from a checkpointed counter: the same draws come again
    assert torch.equal(noise.draws(T), first)
    same_bytes(a, run())
    assert venv.detach_noise() is noise and venv.noise is None
