"""
Several parameter snapshots of a policy evaluated in one launch (DeviceEvalSnapshots; smx_eval_snapshot_floats,
smx_eval_snapshot_store_f32, smx_synth_ppo_eval_sets_f32 / smx_synth_ddpg_eval_sets_f32), shared by the CPU tier
(test_eval_sets_cpu.py) and the GPU tier (test_gpu_eval_sets.py).  The policies, shapes, streams and the host definition
are device_eval_cases'; every numeric check is an equality of fp64 bits against the single-set launch or the host
definition.

  * ``snapshot_floats`` -- the closed form of a snapshot's size and of its blocks' offsets, written out from the layout
    include/surreal_amd.h states;
  * ``agents`` -- K agents of one policy from K parameter seeds (a PPO agent's z-filter state differs with the seed too);
  * ``check_python_refusals`` / ``check_entry_point_codes`` -- every refusal of the new surface (the caller checks that
    nothing was launched).
"""
import ctypes

import pytest
import torch

import device_eval_cases as EV

K_SETS = 3
SEEDS = (3, 11, 29)                                        # the parameter seeds of the K snapshots
E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = -1, -2, -3, -5   # include/surreal_amd.h


# ---- the layout, in closed form ------------------------------------------------------------------------------------------------

def _pack_words(M, K):
    """16-byte words of one packed [M, K] block: whole tiles of 16 rows, an even number of 32-wide K chunks"""
    chunks = (((K + 31) >> 5) + 1) & ~1
    return ((M + 15) >> 4) * chunks * 128


def _up(x, m):
    return (x + m - 1) // m * m


def snapshot_layout(ddpg, D, H, H1, H2, A, zfilter):
    """{block: float offset} and 'total' of a snapshot: [W1 | W2 | W3 | W2^T | W3^T packed | b1 | b2 | b3], a PPO policy's
    log_var [A], zsum [D] | zsumsq [D] | zcount [1] (zfilter), the LSTM's packed gate pass [4H, Dp + H] and its 4H summed
    biases (H > 0) -- each on 4 floats, the whole rounded up to 64.  D: the observation's width; the actor reads the H
    units where there is an LSTM"""
    Din = H if H > 0 else D
    o = 4 * (_pack_words(H1, Din) + _pack_words(H2, H1) + _pack_words(A, H2) + _pack_words(H1, H2) + _pack_words(H2, A))
    lay = {'b1': o, 'b2': o + H1, 'b3': o + H1 + H2}
    o += H1 + H2 + A
    if not ddpg:
        lay['log_var'] = o = _up(o, 4)
        o += A
        if zfilter:
            for k, w in (('zsum', D), ('zsumsq', D), ('zcount', 1)):
                lay[k] = o = _up(o, 4)
                o += w
        if H > 0:
            lay['lstm'] = o = _up(o, 4)
            o += 4 * _pack_words(4 * H, _up(D, 4) + H) + 4 * H
    lay['end'] = o
    lay['total'] = _up(o, 64)
    return lay


def snapshot_floats(ddpg, D, H, H1, H2, A, zfilter):
    return snapshot_layout(ddpg, D, H, H1, H2, A, zfilter)['total']


def policy_dims(p):
    """(ddpg, D, H, H1, H2, A) of a device_eval_cases policy as smx_eval_snapshot_floats takes them (10 LSTM units: 12)"""
    H = _up(EV.RNN, 4) if p.family == 'lstm' else 0
    return (int(p.family == 'ddpg'), p.D, H, p.hidden[0], p.hidden[1], p.A)


# ---- agents ----------------------------------------------------------------------------------------------------------------------

def agents(p, n, mode='eval_deterministic_local', seeds=SEEDS):
    """one agent per parameter seed (PPO: three different z-filter states with them)"""
    return [EV.make_agent(p, n, mode, seed=s)[0] for s in seeds]


def overwrite(dst, src):
    """dst's parameters (and z-filter state) <- src's, IN PLACE: the tensors dst's snapshots were packed from change"""
    with torch.no_grad():
        for k, v in dst.model.actor.views.items():
            v.copy_(src.model.actor.views[k])
        if hasattr(dst, 'rnn_config'):
            dst.model.log_var.copy_(src.model.log_var)
            zd, zs = dst.model.z_filter, src.model.z_filter
            for k in ('running_sum', 'running_sumsq', 'count'):
                getattr(zd, k).copy_(getattr(zs, k))
            if dst.rnn_config.if_rnn_policy:
                for k, v in dst.model.rnn.views.items():
                    v.copy_(src.model.rnn.views[k])


def stored(venv, ags, order=None):
    """a DeviceEvalSnapshots of len(ags) slots on venv, agent k in slot order[k]"""
    snaps = venv.eval_snapshots(ags[0], len(ags))
    for k, a in enumerate(ags):
        snaps.store(k if order is None else order[k], a)
    return snaps


def evaluate_sets(snaps, E, resets=None, noise=None, apw=0, **kw):
    """snaps.evaluate -> np.float64 [count, n, E]; resets / noise as device_eval_cases.evaluate takes them"""
    if resets is not None:
        kw['resets'] = (resets[0], resets[1], resets[2])
    if noise is not None:
        kw['noise'] = (noise[0], noise[1], noise[2])
    return snaps.evaluate(E, actors_per_workgroup=apw, **kw).cpu().numpy()


# ---- the refusals ----------------------------------------------------------------------------------------------------------------

def check_python_refusals(device, kernels):
    """every refusal of DeviceEvalSnapshots (the caller checks that nothing was launched)"""
    from surreal_amd.env import DeviceEvalSnapshots
    mlp, ddpg, drift = EV.BY_ID['mlp-reach-J2'], EV.BY_ID['ddpg-reach-J2'], EV.BY_ID['mlp-drift-17-6']
    n, L = 5, 4
    env = lambda p, **kw: EV.make_env(p, n, L, device, kernels, **kw)  # noqa: E731
    agent, dagent = EV.make_agent(mlp, n)[0], EV.make_agent(ddpg, n)[0]
    venv = env(mlp)

    def refused(cls, words, f, *a, **kw):
        with pytest.raises(cls) as e:
            f(*a, **kw)
        assert type(e.value) is cls and all(w in str(e.value) for w in words), str(e.value)

    # construction: can_evaluate's refusals, before anything is allocated
    refused(NotImplementedError, ('a camera env',), env(drift, pixel=(3, 8, 8)).eval_snapshots, EV.make_agent(drift, n)[0], 2)
    refused(NotImplementedError, ('a LayerNorm actor',), venv.eval_snapshots, EV.ddpg_agent(ddpg, n, layernorm=True)[0], 2)
    noisy = env(ddpg)
    noisy.param_noise = object()
    refused(NotImplementedError, ('an attached parameter noise',), noisy.eval_snapshots, dagent, 2)
    refused(NotImplementedError, ('per-actor episode clocks',),
            EV.make_env(drift, n, [L] * n, device, kernels).eval_snapshots, EV.make_agent(drift, n)[0], 2)
    refused(NotImplementedError, ('smx_synth_eval_supported',), venv.eval_snapshots,
            EV.make_agent(mlp._replace(hidden=(30, 32)), n)[0], 2)
    lstm = EV.make_agent(EV.BY_ID['lstm-reach-J2'], n)[0]
    lstm.rnn_config.rnn_layer = 2
    try:
        refused(NotImplementedError, ('rnn_layer 2',), venv.eval_snapshots, lstm, 2)
    finally:
        lstm.rnn_config.rnn_layer = 1
    refused(ValueError, ('capacity',), venv.eval_snapshots, agent, 0)
    refused(ValueError, ('capacity',), venv.eval_snapshots, agent, 65536)
    # store: the slot, the architecture, the z-filter use
    snaps = venv.eval_snapshots(agent, 3)
    assert isinstance(snaps, DeviceEvalSnapshots) and snaps.stored == [False] * 3
    refused(ValueError, ('slots',), snaps.store, 3)
    refused(ValueError, ('slots',), snaps.store, -1)
    refused(ValueError, ('architecture',), snaps.store, 0, dagent)
    refused(ValueError, ('architecture',), snaps.store, 0, EV.make_agent(mlp._replace(hidden=(28, 20)), n)[0])
    refused(ValueError, ('architecture',), snaps.store, 0, lstm)
    nozf = EV.make_agent(mlp, n)[0]
    nozf.use_z_filter = False
    refused(ValueError, ('architecture',), snaps.store, 0, nozf)
    # evaluate: slots never stored, the slot range, then evaluate()'s own rules
    refused(ValueError, ('never stored',), snaps.evaluate)
    return snaps, refused, (mlp, ddpg, drift, n, L, env)


def check_evaluate_refusals(snaps, refused, ctx, device):
    """with slots 0 and 1 of `snaps` stored (the caller's business: a launch on the GPU tier, a double on the CPU tier)"""
    mlp, ddpg, drift, n, L, env = ctx
    refused(ValueError, ('never stored', '[2]'), snaps.evaluate)
    refused(ValueError, ('slots',), snaps.evaluate, first=2, count=2)
    refused(ValueError, ('slots',), snaps.evaluate, first=0, count=0)
    ok = dict(first=0, count=2)
    refused(ValueError, ('noise must be None',), snaps.evaluate, noise=(EV.NSEED, 0), **ok)
    refused(ValueError, ('episodes',), snaps.evaluate, 0, **ok)
    refused(ValueError, ('first_episode', 'negative'), snaps.evaluate, resets=(EV.RSEED, -1), **ok)
    refused(ValueError, ('2^32',), snaps.evaluate, resets=(EV.RSEED, 0, 2 ** 32 - n + 1), **ok)
    refused(ValueError, ('out',), snaps.evaluate, out=torch.empty(2, n, 2, dtype=torch.float64, device=device), **ok)
    refused(ValueError, ('out',), snaps.evaluate, out=torch.empty(n, 1, dtype=torch.float64, device=device), **ok)
    refused(ValueError, ('2^31',), snaps.evaluate, 2 ** 31 // n + 1, **ok)
    refused(ValueError, ('sets', '2^31'), snaps.evaluate, 2 ** 31 // (2 * n) + 1, **ok)
    snaps.agent.agent_mode = 'training'
    try:
        refused(ValueError, ('training',), snaps.evaluate, **ok)
    finally:
        snaps.agent.agent_mode = 'eval_deterministic_local'
    snaps.agent.agent_mode = 'eval_stochastic_local'
    try:
        refused(ValueError, ('noise=', 'required'), snaps.evaluate, **ok)
    finally:
        snaps.agent.agent_mode = 'eval_deterministic_local'
    d = env(drift).eval_snapshots(EV.make_agent(drift, n)[0], 1)
    d.stored[0] = True                                          # (bookkeeping alone: the refusal comes first)
    refused(ValueError, ('no reset distribution',), d.evaluate, resets=(EV.RSEED, 0))
    dd = env(ddpg).eval_snapshots(EV.make_agent(ddpg, n, mode='eval_stochastic_local')[0], 1)
    dd.stored[0] = True
    refused(NotImplementedError, ('DDPG', 'eval_stochastic'), dd.evaluate, noise=(EV.NSEED, 0))


def check_entry_point_codes():
    """the C entry points' argument checks, which run before any launch (host code: no GPU needed)"""
    from surreal_amd import _lib as L
    lib = L.load()
    floats = lib.smx_eval_snapshot_floats

    def net(D=6, H1=32, H2=32, A=2):
        m = L.Mlp3()
        m.W1 = m.b1 = m.W2 = m.b2 = m.W3 = m.b3 = 4096
        m.D, m.H1, m.H2, m.OUT = D, H1, H2, A
        return m

    def lstm_net(D=6, H=12):
        q = L.Lstm()
        q.W_ih = q.W_hh = q.b_ih = q.b_hh = 4096
        q.D, q.H = D, H
        return q

    def stream(cls, base=0, counter=0):
        q = cls()
        q.seed, q.actor_base, q.enabled = 1, base, 1
        setattr(q, 'episode' if cls is L.ResetStream else 'step', counter)
        return q

    def sets_of(need, blobs=4096, stride=None, sets=2, zfilter=0):
        s = L.EvalSets()
        s.blobs, s.stride, s.sets, s.zfilter = blobs, need if stride is None else stride, sets, zfilter
        return s

    def ppo(task=1, n=4, episodes=2, episode_len=3, m=None, lstm=None, give=True, fields=(), **skw):
        m = m or net()
        p = L.SynthPpoEval()
        p.net, p.init_state, p.returns = ctypes.pointer(m), 4096, 4096
        p.n, p.episodes, p.episode_len, p.task = n, episodes, episode_len, task
        D, H = m.D, 0
        if lstm is not None:
            p.lstm, p.hidden = ctypes.pointer(lstm), lstm.H
            D, H = lstm.D, lstm.H
        for k, v in dict(fields).items():
            setattr(p, k, v)
        need = floats(0, D, H, m.H1, m.H2, m.OUT, 1 if skw.get('zfilter') else 0) or 64
        return lib.smx_synth_ppo_eval_sets_f32(p, sets_of(need, **skw) if give else None, None)

    def ddpg(task=1, n=4, episodes=2, episode_len=3, m=None, give=True, fields=(), **skw):
        m = m or net()
        p = L.SynthDdpgEval()
        p.net, p.init_state, p.returns = ctypes.pointer(m), 4096, 4096
        p.n, p.episodes, p.episode_len, p.task = n, episodes, episode_len, task
        for k, v in dict(fields).items():
            setattr(p, k, v)
        need = floats(1, m.D, 0, m.H1, m.H2, m.OUT, 0) or 64
        return lib.smx_synth_ddpg_eval_sets_f32(p, sets_of(need, **skw) if give else None, None)
    R, N = L.ResetStream, L.NoiseStream
    need = floats(0, 6, 0, 32, 32, 2, 0)
    for f in (ppo, ddpg):
        # the sets
        assert f(give=False) == E_NULL and f(blobs=None) == E_NULL
        assert f(sets=0) == E_SHAPE and f(sets=-1) == E_SHAPE and f(sets=65536) == E_SHAPE
        assert f(n=2 ** 15, episodes=2 ** 10, sets=64) == E_SHAPE          # (sets * n * episodes = 2^31)
        assert f(stride=need - 64) == E_SHAPE and f(stride=need + 2) == E_SHAPE and f(stride=0) == E_SHAPE
        assert f(blobs=4096 + 4) == E_ALIGN and f(blobs=4096 + 8) == E_ALIGN
        assert f(zfilter=2) == E_SHAPE and f(zfilter=-1) == E_SHAPE
        # what the single-set entry points refuse, with their codes
        assert f(task=0, m=net(D=17, A=6), fields={'resets': stream(R)}) == E_UNSUPPORTED
        assert f(task=1, m=net(D=7, A=2)) == E_UNSUPPORTED and f(task=7) == E_UNSUPPORTED
        assert f(m=net(H1=30)) == E_UNSUPPORTED
        assert f(fields={'resets': stream(R, base=-1)}) == E_SHAPE and f(fields={'resets': stream(R, counter=-1)}) == E_SHAPE
        assert f(episodes=0) == E_SHAPE and f(episode_len=0) == E_SHAPE and f(n=0) == E_SHAPE
        assert f(n=2 ** 20, episodes=2 ** 11) == E_SHAPE
        assert f(fields={'actors_per_workgroup': 5}) == E_SHAPE
        for k in ('net', 'init_state', 'returns'):
            assert f(fields={k: None}) == E_NULL, k
    assert lib.smx_synth_ppo_eval_sets_f32(None, sets_of(need), None) == E_NULL
    assert lib.smx_synth_ddpg_eval_sets_f32(None, sets_of(need), None) == E_NULL
    # a layout sized without the z-filter's sums, read with them: the stride is short of it
    # (63 observation elements: the three sums do not fit the padding of the layout without them)
    wide = floats(0, 63, 0, 32, 32, 21, 0)
    assert floats(0, 63, 0, 32, 32, 21, 1) > wide > 0
    assert ppo(m=net(D=63, A=21), zfilter=1, stride=wide) == E_SHAPE and ppo(m=net(D=63, A=21), stride=wide - 4) == E_SHAPE
    assert ddpg(zfilter=1) == E_SHAPE                                       # (a DDPG actor has no z-filter)
    assert ppo(fields={'noise': stream(N, base=-1)}) == E_SHAPE
    assert ppo(lstm=lstm_net(H=12), m=net(D=8)) == E_SHAPE                  # (the actor reads the LSTM's units)
    assert ppo(lstm=lstm_net(H=12), m=net(D=12), stride=need) == E_SHAPE    # (an MLP policy's stride under an LSTM's)
    # the store
    store = lib.smx_eval_snapshot_store_f32

    def src(m=None, ddpg=0, lstm=None, **fields):
        s = L.EvalSnapshotSrc()
        m = m or net()
        s.net, s.log_var, s.ddpg = ctypes.pointer(m), 4096, ddpg
        if lstm is not None:
            s.lstm = ctypes.pointer(lstm)
        for k, v in fields.items():
            setattr(s, k, v)
        return s
    assert store(None, 4096, None) == E_NULL and store(src(), None, None) == E_NULL
    assert store(src(net=None), 4096, None) == E_NULL and store(src(log_var=None), 4096, None) == E_NULL
    broken = net()
    broken.b2 = None
    assert store(src(m=broken), 4096, None) == E_NULL and store(src(m=broken, ddpg=1), 4096, None) == E_NULL
    assert store(src(zsum=4096), 4096, None) == E_NULL and store(src(zsum=4096, zsumsq=4096), 4096, None) == E_NULL
    half = lstm_net()
    half.W_hh = None
    assert store(src(m=net(D=12), lstm=half), 4096, None) == E_NULL
    assert store(src(m=net(D=8), lstm=lstm_net(H=12)), 4096, None) == E_SHAPE
    assert store(src(m=net(H1=30)), 4096, None) == E_UNSUPPORTED
    assert store(src(m=net(H1=30), ddpg=1, log_var=None), 4096, None) == E_UNSUPPORTED
    assert store(src(ddpg=1, zsum=4096, zsumsq=4096, zcount=4096), 4096, None) == E_UNSUPPORTED
    assert store(src(m=net(D=12), lstm=lstm_net(H=12), ddpg=1), 4096, None) == E_UNSUPPORTED
    assert store(src(), 4096 + 4, None) == E_ALIGN and store(src(ddpg=1, log_var=None), 4096 + 8, None) == E_ALIGN
