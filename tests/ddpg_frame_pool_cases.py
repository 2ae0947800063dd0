"""
The frame-pool layout of the device DDPG replay (replay.device_frame_pool) against the stacked layout it replaces, shared
by the CPU tier (test_ddpg_frame_pool_cpu.py) and the GPU tier (test_gpu_ddpg_frame_pool.py):

  * ``FramePoolCpuKernels`` -- the torch-CPU doubles of smx_synth_ddpg_pixel_pool_step and smx_uniform_gather_pool (a
    subclass of the camera rollout's double), by the header's counter arithmetic;
  * ``simulate`` -- a plain Python run of the counters of a shared episode clock: which ring rows a rollout leaves
    live, computed row by row from rule "the oldest frame a row names has not been overwritten" -- nothing of the
    replay's own bookkeeping;
  * ``twin`` -- the same rollout (same agent, same eps) into a stacked replay and into a pool replay.
"""
import numpy as np
import torch

import ddpg_pixel_rollout_cases as PC
import pixel_recorder_cases as PR
from surreal_amd.env.synthetic_env import _drift

FIELDS = PC.FIELDS
N_, D_, A_ = 5, 7, 3                                # the twin rollouts' actors, observation and action sizes
# 16-byte and byte-path frames; (n_step, frame_stacks); episodes shorter than N + S (every stack clamps) and of 9
TWIN_CASES = [(pixel, N, S, L_) for pixel in ((3, 8, 8), (3, 6, 7)) for N, S in ((3, 3), (1, 3), (3, 1), (4, 2))
              for L_ in (4, 9)]


class PoolGatherDouble(object):
    """smx_uniform_gather_pool on the double's uniform_gather_multi / uniform_indices"""

    def uniform_gather_pool(self, tables, outs, pool, pixel, pixel_next, length, seed, offset, base, idx=None,
                            idx_out=None):
        cap = tables[0].shape[0]
        if idx is None:
            idx = torch.empty(outs[0].shape[0], dtype=torch.int64)
            self.uniform_indices(idx, length, seed, offset)
            idx = (idx + int(base)) % cap
        self.uniform_gather_multi(tables, outs, length, seed, offset, idx=idx, idx_out=idx_out)
        fp, S, N = pool['pool'], int(pool['frame_stacks']), int(pool['n_step'])
        P = fp.shape[1]
        for dst, back in ((pixel, N), (pixel_next, 0)):
            d = dst.view(idx.numel(), S, -1)
            for i, row in enumerate(idx.tolist()):
                a, lo = int(pool['frame_actor'][row]), int(pool['frame_first'][row])
                top = int(pool['frame_next'][row]) - back
                for k in range(S):
                    d[i, k] = fp[a, max(top - S + 1 + k, lo) % P]


class FramePoolRecorderCpuKernels(PoolGatherDouble, PR.PixelRecorderCpuKernels):
    name = 'torch-cpu-double+frame-pool-recorder'

    def record_ddpg_pixel_pool_nstep_step(self, r, copy_workgroups=0, monitor=None):
        """smx_record_ddpg_pixel_pool_nstep_step: the frames by the header's per-actor counters, then the double's
        low-dimensional record step"""
        pool, obs, tabs = r['pool'], r['obs_pixel'], r['tables']
        n, P, F = pool.shape
        S, N = obs.shape[1] // r['frame_shape'][0], int(r['n_step'])
        cin, cout = r['counters_in'], r['counters_out']
        assert P >= N + S + 1 and cin.data_ptr() != cout.data_ptr() and 0 <= copy_workgroups <= 1024
        fnext = r['frames_next'].reshape(n, F)
        freset = None if r.get('frames_reset') is None else r['frames_reset'].reshape(n, F)
        cap = tabs['obs'].shape[0]
        for a in range(n):
            tau, rank = int(r['t'][a]), int(r['rank'][a])
            if tau < 0:
                continue
            f, first = int(cin[0, a]), int(cin[1, a])
            restart = bool(r['dones'][a] != 0) and freset is not None
            if 0 <= rank < int(r['rows']) and tau >= N - 1:
                row = (int(r['cursor']) + rank) % cap
                r['frame_next'][row], r['frame_first'][row], r['frame_actor'][row] = f + 1, first, a
            pool[a, (f + 1) % P] = fnext[a]
            if restart:
                pool[a, (f + 2) % P] = freset[a]
                obs[a] = freset[a].repeat(S).view(obs[a].shape)
                cout[0, a] = cout[1, a] = f + 2
            else:
                obs[a] = torch.cat([pool[a, max(f + 2 - S + i, first) % P] for i in range(S)]).view(obs[a].shape)
                cout[0, a], cout[1, a] = f + 1, first
        self.record_ddpg_nstep_step(r, monitor=monitor)


class FramePoolCpuKernels(PoolGatherDouble, PC.DdpgPixelRolloutCpuKernels):
    name = 'torch-cpu-double+ddpg-frame-pool'

    def synth_ddpg_pixel_pool_step(self, r, mu):
        """smx_synth_ddpg_pixel_pool_step: synth_ddpg_step, then the frames by the header's counters"""
        pool, obs_pix, tabs = r['pool'], r['obs_pixel'], r['tables']
        n, P, F = pool.shape
        C, H, W = r['frame_shape']
        S = obs_pix.shape[1] // C
        tau, N, L_ = int(r['t']), int(r['n_step']), int(r['episode_len'])
        f, first = int(r['frame']), int(r['episode_first'])
        assert P >= N + S + 1 and 0 <= first <= f
        s0 = r['state'][:, 0].clone()
        self.synth_ddpg_step(r, mu)
        a0 = r['carry_act'][:, tau % N, 0]
        sn0 = (torch.tensor(0.9, dtype=torch.float32) * s0 + torch.tensor(0.5, dtype=torch.float32) * a0)
        sn0 = (sn0 + torch.as_tensor(_drift(1))).clamp(-10.0, 10.0)
        new = torch.empty(n, C, H, W, dtype=torch.uint8)
        self.synth_frames(sn0, tau + 1, new)
        pool[:, (f + 1) % P] = new.reshape(n, F)
        if tau >= N - 1:
            rows = (int(r['cursor']) + torch.arange(n)) % tabs['obs'].shape[0]
            r['frame_next'][rows] = f + 1
            r['frame_first'][rows] = first
            r['frame_actor'][rows] = torch.arange(n, dtype=torch.int32)
        if tau + 1 >= L_:
            f0 = torch.empty(n, C, H, W, dtype=torch.uint8)
            self.synth_frames(r['init_state'][:, 0], 0, f0)
            pool[:, (f + 2) % P] = f0.reshape(n, F)
            obs_pix.copy_(f0.repeat(1, S, 1, 1))
        else:
            obs_pix.copy_(torch.cat([pool[:, max(f + 2 - S + i, first) % P] for i in range(S)], 1).view(obs_pix.shape))


def configs(D, A, n, pixel, stacks, **kw):
    """PC.configs with a stem for frames of 6 x 7 and up: 3 x 3 and 2 x 2 kernels at stride 1"""
    lc, ec, sc = PC.configs(D, A, n, pixel, stacks, **kw)
    lc.model.conv_spec.out_channels, lc.model.conv_spec.kernel_sizes, lc.model.conv_spec.strides = [4, 8], [3, 2], [1, 1]
    return lc, ec, sc


def pool_configs(D, A, n, pixel, stacks, pool_steps=None, **kw):
    """configs with replay.device_frame_pool on"""
    lc, ec, sc = configs(D, A, n, pixel, stacks, **kw)
    lc.replay.device_frame_pool = True
    if pool_steps is not None:
        lc.replay.device_frame_pool_steps = pool_steps
    return lc, ec, sc


def simulate(n, N, S, lengths, T, capacity, P):
    """T steps of n actors on a shared clock whose successive episodes have the lengths `lengths` (cycled), from a
    primed pool (counter 0 = the first reset frame) -> (live {ring row: (actor, frame_next, frame_first)}, rows written,
    the counter).  A row is live while max(frame_first, frame_next - N - S + 1) >= counter - P + 1"""
    ring, written = {}, 0
    f = first = 0
    tau, ep = 0, 0
    for _ in range(T):
        done = tau + 1 >= lengths[ep % len(lengths)]
        if tau >= N - 1:
            for a in range(n):
                ring[written % capacity] = (a, f + 1, first)
                written += 1
        f += 2 if done else 1
        if done:
            first, tau, ep = f, 0, ep + 1
        else:
            tau += 1
    live = {row: v for row, v in ring.items() if max(v[2], v[1] - N - S + 1) >= f - P + 1}
    return live, written, f


def _chunks(calls, most):
    return [min(most, T - k) for T in calls for k in range(0, T, most)]


def simulate_recorder(dones, n_step, S, capacity, P):
    """dones bool [steps, n] of a recorder that began with every actor's first frame at counter 0 -> (live: the ring rows
    that may be sampled, rows written).  Per row the rule of simulate(); the rows of a step retire together, and with them
    every older step's, so the live rows are the newest ones of the ring"""
    steps, n = dones.shape
    f, first, t = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    recorded, written = [], 0
    for s in range(steps):
        rows = []
        for a in range(n):
            if t[a] >= n_step - 1:
                rows.append((written, max(first[a], f[a] + 2 - n_step - S), a))
                written += 1
        recorded.append(rows)
        for a in range(n):
            f[a] += 2 if dones[s, a] else 1
            first[a], t[a] = (f[a], 0) if dones[s, a] else (first[a], t[a] + 1)
    live = set()
    for rows in reversed(recorded):
        if any(oldest < f[a] - P + 1 for _, oldest, a in rows):
            break                                # a row names an overwritten frame: its step and every older one left
        keep = [g for g, _, _ in rows if written - g <= capacity]
        live |= {g % capacity for g in keep}
        if len(keep) < len(rows):
            break                                # the ring has overwritten the rest
    return live, written


def twin(K, device, n, D, A, pixel, N, S, episode_len, calls, memory_size, pool_steps=None, monitor=False, seed=5,
         **cfg):
    """the same rollout into a stacked replay and a pool replay -> dict(stacked=(venv, replay), pool=(venv, replay),
    agent, configs of the pool side, and per side '<side>_rows' = the sum of what the calls returned)"""
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    kw = dict(memory_size=memory_size, n_step=N, gamma=0.9, noise_type='ou_noise', theta=2.0, dt=0.05)
    kw.update(cfg)
    lc, ec, sc = configs(D, A, n, pixel, S, **kw)
    lcp, ecp, scp = pool_configs(D, A, n, pixel, S, pool_steps=pool_steps, **kw)
    agent = PC.DC.make_agent(lc, ec, sc, w3_scale=1.0)
    eps = torch.as_tensor(np.random.RandomState(seed).randn(sum(calls), n, A).astype(np.float32)).to(device)
    out = dict(agent=agent, configs=(lcp, ecp, scp))
    for name, cfgs in (('stacked', (lc, ec, sc)), ('pool', (lcp, ecp, scp))):
        venv = SyntheticVecEnv(n, D, A, episode_len=episode_len, device=device, kernels=K, pixel=pixel, frame_stacks=S)
        mon = venv.attach_monitor(8) if monitor else None
        replay = UniformReplay(*cfgs)
        s0 = 0
        rows = []
        # (a call into the stacked layout may not go round the ring: the same steps in calls of memory_size // n)
        for T in (calls if name == 'pool' else _chunks(calls, max(1, memory_size // n))):
            rows.append(venv.ddpg_rollout_into(agent, replay, T, eps=eps[s0:s0 + T].contiguous()))
            s0 += T
        out[name] = (venv, replay)
        out[name + '_rows'] = sum(rows)
        out[name + '_episodes'] = mon.poll() if monitor else None
    return out


def assert_live_rows_equal(t, live_rows):
    """sample_batch(indices=live rows) of the pool replay == the stacked replay's: uint8 bytes and fp32 bits"""
    idx = torch.as_tensor(sorted(live_rows), dtype=torch.int64)
    B = idx.numel()
    got = t['pool'][1].sample_batch(B, indices=idx)
    want = t['stacked'][1].sample_batch(B, indices=idx)
    assert list(got) == list(want)
    for k in want:
        g, w = got[k].cpu(), want[k].cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, k
        if w.dtype == torch.uint8:
            assert torch.equal(g, w), (k, torch.nonzero(g != w)[:5])
        else:
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), k


def check_twin(K, device, pixel, N, S, episode_len, calls=(10, 13), pool_steps=None, monitor=False):
    t = twin(K, device, N_, D_, A_, pixel, N, S, episode_len, calls, 4 * N_, pool_steps=pool_steps, monitor=monitor)
    (venv_s, rep_s), (venv_p, rep_p) = t['stacked'], t['pool']
    P = rep_p.frame_pool['pool'].shape[1]
    assert P == (pool_steps or 4 + N + S)
    live, written, f = simulate(N_, N, S, [episode_len], sum(calls), 4 * N_, P)
    assert t['pool_rows'] == t['stacked_rows'] == written
    assert len(rep_p) == len(live) and int(rep_p.frame_pool['counter'][0]) == f
    assert rep_p._dev_next == rep_s._dev_next and set(rep_p._tables) == set(PC.DC.FIELDS)
    if live:
        # (the live rows are the newest of the ring)
        assert set(live) == {(rep_p._dev_next - 1 - k) % (4 * N_) for k in range(len(live))}
        assert_live_rows_equal(t, live)
    assert torch.equal(venv_p._ddpg['obs_pixel'].cpu(), venv_s._ddpg['obs_pixel'].cpu())
    assert torch.equal(venv_p.state.cpu(), venv_s.state.cpu()) and venv_p.t == venv_s.t
    assert t['pool_episodes'] == t['stacked_episodes']
    return t, live


def check_recorder_twin(pixel, N, S, lengths, pool_steps=None, n=5, D=7, A=3, steps=40, capacity=4 * 5, monitor=None,
                        stacked_too=True):
    """the step stream of n host chains on diverging clocks through a DeviceNStepRecorder into a stacked replay and into
    a pool replay (the acting observation checked after every step on both): live rows byte for byte, the live set from
    simulate_recorder -> (stacked replay, pool replay, live rows).  stacked_too False: the pool side alone (a monitor
    counts one run)"""
    import ddpg_rollout_cases as DC
    import recorder_cases as RC
    from surreal_amd.replay import UniformReplay
    st = PR.host_ddpg_pixel(n, D, A, pixel, S, lengths, steps, N, 0.99)
    lc, ec, sc = DC.configs(D, A, n, n_step=N, gamma=0.99, memory_size=capacity, folder='surreal_amd_recorder')
    lc.replay.device_frame_pool = True
    if pool_steps is not None:
        lc.replay.device_frame_pool_steps = pool_steps
    stacked, pool = RC.uniform(D, A, n, N, 0.99, capacity), UniformReplay(lc, ec, sc)
    written = [PR.device_ddpg_pixel(st, r, N, 0.99, monitor=monitor)[1] if r is pool or stacked_too else len(st.exps)
               for r in (stacked, pool)]
    P = pool.frame_pool['pool'].shape[1]
    assert P == (pool_steps or -(-capacity // n) + N + S)
    live, total = simulate_recorder(st.dones, N, S, capacity, P)
    assert written == [total, total] == [len(st.exps)] * 2 and total > capacity
    assert len(pool) == len(live) > 0 and (not stacked_too or pool._dev_next == stacked._dev_next)
    assert set(pool._tables) == set(DC.FIELDS)
    if stacked_too:
        assert_live_rows_equal({'pool': (None, pool), 'stacked': (None, stacked)}, live)
    elif monitor is not None:
        RC.assert_monitor_equals_host(monitor, st)
    return stacked, pool, live
