"""
The actor variants of the one-launch DDPG rollout -- a LayerNorm actor, a parameter-noise population, both -- on the
`reach` task (ddpg_rollout_kernel<RG, NT, POP, LN, false, SMX_TASK_REACH>; smx_synth_ddpg_rollout_variant_task_f32), shared by
the CPU tier (test_reach_ddpg_variants_cpu.py) and the GPU tier (test_gpu_reach_ddpg_variants.py).  Built on reach_cases
(the task's float64 restatement, calls, episodes, bounds), reach_resets_cases (drawn episodes), ddpg_ln_rollout_cases (the
LayerNorm parameters, every byte a run leaves) and rollout_fp64_ref (DdpgPolicy: LayerNorm and populations):

  * ``ReachVariantsCpuKernels`` -- the reset-stream double of the task composed with the LayerNorm / population double;
    it advertises ``ddpg_variant_task_launch`` and records the launches it is handed.  As in the double it inherits, a
    population launch steps every actor from the clean actor: the CPU tier reads routes, clocks and counters, not actions;
  * ``Case`` / ``make`` / ``run`` / ``ring`` / ``restatement`` -- a case on a kernels object and its float64 reference, the
    input conditions (reach_cases.MARGIN) stated on the reference alone;
  * ``tuned`` -- the seed per case, found on the CPU on the restatement alone (``python tests/reach_ddpg_variants_cases.py``
    prints the entries that differ from the case's own).
"""
import collections
import types

import numpy as np
import torch

import ddpg_ln_rollout_cases as LN
import ddpg_rollout_cases as DC
import episode_monitor_cases as EM
import noise_ref as NR
import reach_cases as RC
import reach_resets_cases as RRC
import rollout_envelope_cases as EC
import rollout_fp64_ref as R
from reach_resets_cpu_kernels import ResetsCpuKernels

EP, CALLS, N_STEP, GAMMA, MARGIN = RC.EP, RC.CALLS, RC.N_STEP, RC.GAMMA, RC.MARGIN
SEED, RSEED, PSEED = RC.SEED, RRC.RSEED, LN.PSEED
INTERVAL = 3                      # compute_dist_interval: calls of 4, 5, 3 steps measure at acts 3, 6 and 9 (clocks 3, 1, 4)
MAX_N = 32
# the exploration scales by GLOBAL actor id (an env of actors lo .. hi takes its slice), as test_gpu_param_noise.py's
SIG = torch.linspace(0.05, 0.8, MAX_N, dtype=torch.float64)
# test_gpu_param_noise.py's bound on a measured distance: two actor outputs of A components, each held to 2e-6
DIST_ATOL = lambda A: 2e-6 * 2 * np.sqrt(A)  # noqa: E731


class ReachVariantsCpuKernels(ResetsCpuKernels, LN.DdpgLnRolloutCpuKernels):
    name = 'torch-cpu-double+tasks+resets+ddpg-variants'
    ddpg_ln_launch = True
    ddpg_variant_task_launch = True

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.routes, self.refreshes, self.launches, self.ln_launches = [], [], [], []

    def synth_ddpg_rollout(self, net, packed, r, steps, actors_per_workgroup=0, monitor=None, noise=None, ln=None,
                           ln_eps=0.0, pn=None, measure_step=-1, clocks=None, task='drift', resets=None):
        assert noise is None, 'the doubles draw from no stream: pass eps'
        assert clocks is None and actors_per_workgroup in (0, 4, 8, 16)
        self.routes.append(dict(task=task, ln=ln is not None, pn=pn is not None, resets=resets, steps=steps,
                                measure_step=measure_step, t=int(r['t']), acts=None if pn is None else pn.acts))
        if ln is None and pn is None:
            kw = dict(resets=resets) if resets is not None else {}
            return ResetsCpuKernels.synth_ddpg_rollout(self, net, packed, r, steps, actors_per_workgroup, monitor=monitor,
                                                       task=task, **kw)
        if task != 'drift':
            assert self.synth_task_supported(task, net.D, net.OUT)
        assert self.synth_ddpg_rollout_supported(net, ln=ln is not None)
        if pn is not None:
            assert pn.actors_per_agent % 4 == 0 and pn.agents * pn.actors_per_agent == r['state'].shape[0]
            assert -1 <= measure_step < steps
        n, cap = r['state'].shape[0], r['tables']['obs'].shape[0]
        W = dict(self._packed_views(packed, net))
        W.update({k: net.views[k] for k in ('b1', 'b2', 'b3')})
        # the LayerNorm double's loop over the steps, the step the task's (synth_ddpg_step: the resets double's hook, then
        # the task double's dynamics), the monitor parked for it
        with self._on_task(task), self._parked(monitor), \
                self._drawing(resets, r['state'], r['t'], r['episode_len']) as init:
            r = dict(r, init_state=init) if resets is not None else dict(r)
            eps = r['eps']
            for s in range(steps):
                mu = self._mu_rows(net, W, W, r['state']) if ln is None else self._mu_ln(net, W, ln, ln_eps, r['state'])
                r['eps'] = None if eps is None else eps[s]
                self.synth_ddpg_step(r, mu)
                if r['t'] >= r['n_step'] - 1:
                    r['cursor'] = (r['cursor'] + n) % cap
                r['t'] = 0 if r['t'] + 1 >= r['episode_len'] else r['t'] + 1

    def param_noise_refresh(self, net, pn, ln=None):
        self.refreshes.append(dict(generation=pn.generation, acts=pn.acts, adaptive=pn.adaptive, ln=ln is not None))


# ---- the cases -------------------------------------------------------------------------------------------------------------

Case = collections.namedtuple('Case', 'id D A n H1 H2 ln apa seed scale streams')
# ln: a LayerNorm actor; apa: actors per agent of an 'adaptive_normal' population (0: none).  n = 5: a partial 4-actor
# block; n = 20: more than one block at every size, a partial one at 8 and 16; populations: 32 actors, so that 4, 8 and 16
# actors per agent make 8, 4 and 2 agents.  Hidden 76 / 132: ln_rows' second, partial column pass.  streams: the reset
# stream, and on the GPU the noise stream and the episode monitor.  scale: the gain of the output layer's weights -- 1 behind a
# LayerNorm, whose rows are of unit size (at reach_cases' 6 the tanh saturates to within MARGIN of the clip), 2 without one.
CASES = [
    Case('ln-3-1-n5', 3, 1, 5, 8, 4, True, 0, 0, 1.0, False),
    Case('ln-6-2-n20-streams', 6, 2, 20, 8, 4, True, 0, 0, 1.0, True),
    Case('ln-63-21-n20', 63, 21, 20, 8, 4, True, 0, 0, 1.0, False),
    Case('ln-6-2-h76-132-n5', 6, 2, 5, 76, 132, True, 0, 0, 1.0, False),
    Case('pop4-6-2-n32-streams', 6, 2, 32, 8, 4, False, 4, 0, 2.0, True),
    Case('pop8-3-1-n32', 3, 1, 32, 8, 4, False, 8, 0, 2.0, False),
    Case('pop16-63-21-n32-streams', 63, 21, 32, 8, 4, False, 16, 0, 2.0, True),
    Case('popln4-3-1-n32-streams', 3, 1, 32, 8, 4, True, 4, 0, 1.0, True),
    Case('popln8-63-21-n32', 63, 21, 32, 8, 4, True, 8, 0, 1.0, False),
    Case('popln16-6-2-n32-streams', 6, 2, 32, 8, 4, True, 16, 0, 1.0, True),
]
# the first seed under which the float64 restatement ALONE keeps every ReLU pre-activation, action clip and environment
# clamp MARGIN (twice MARGIN: a streams case) from its kink -- tune(), below, on the CPU
TUNED = {
    'ln-6-2-n20-streams': 2,
    'ln-63-21-n20': 2,
    'ln-6-2-h76-132-n5': 4,
    'pop4-6-2-n32-streams': 1,
    'pop16-63-21-n32-streams': 6,
    'popln4-3-1-n32-streams': 1,
    'popln8-63-21-n32': 7,
    'popln16-6-2-n32-streams': 7,
}


def tuned(c):
    return c._replace(seed=TUNED.get(c.id, c.seed))


def closing_steps(calls=CALLS, t0=0):
    t, k = t0, 0
    for _ in range(sum(calls)):
        k += t >= N_STEP - 1
        t = 0 if t + 1 >= EP else t + 1
    return k


def measuring_acts(calls=CALLS, interval=INTERVAL, acts=0):
    """the act() calls (counted from 0) at which DeviceParamNoise.measure_step places a call's measuring step"""
    out = []
    for T in calls:
        s = (T - 1) - (acts + T - 1) % interval
        if s >= 0:
            out.append(acts + s)
        acts += T
    return tuple(out)


def explicit_draws(c, device, lo, n, streams):
    """[S, n, A] fp32 for the actors lo .. lo + n - 1: a streams case's are the noise stream's own (its float64
    restatement rounded to fp32 -- what a double gets as eps; the GPU tier reads DeviceNoise.draws instead), else seeded
    normals by global actor id"""
    S = sum(CALLS)
    if streams:
        e = torch.as_tensor(NR.draws(SEED, lo, 0, S, n, c.A).astype(np.float32))
    else:
        e = torch.randn(S, MAX_N, c.A, generator=torch.Generator().manual_seed(100 + c.seed))[:, lo:lo + n].contiguous()
    return e.to(device)


def make(c, device, kernels=None, **kw):
    """a case's agent, task env, replay, parameter noise and draws, made afresh -> a namespace.  n / actor_base: an env of
    n actors with the global ids actor_base .. (default: the case's, from 0); wrap: a ring smaller than the rows the run
    writes; attach=False: no population (the agent then has no parameter noise); layernorm: the case's by default;
    params: the actor's arrays to load in place of the case's own; calls: CALLS"""
    from surreal_amd import kernels as KN
    if kernels is not None:                         # (the agents take the default kernels object)
        prev = KN.set_default_kernels(kernels, device)
        try:
            return _make(c, device, kernels, **kw)
        finally:
            KN.set_default_kernels(*prev)
    return _make(c, device, None, **kw)


def _make(c, device, kernels, n=None, actor_base=0, wrap=False, attach=True, layernorm=None, params=None, task='reach',
          calls=CALLS):
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    n = c.n if n is None else n
    ln = c.ln if layernorm is None else layernorm
    pop = bool(c.apa) and attach
    rows = n * closing_steps(calls)
    x = types.SimpleNamespace(c=c, n=n, lo=actor_base, rows=rows, capacity=(rows - n - 1) if wrap else rows + 7, pn=None,
                              calls=calls, ln=ln)
    lc, ec, sc = DC.configs(c.D, c.A, n, hidden=(c.H1, c.H2), n_step=N_STEP, gamma=GAMMA, noise_type='ou_noise',
                            layernorm=ln, param_noise_type='adaptive_normal' if pop else None, memory_size=x.capacity,
                            theta=2.0, dt=0.02, folder='surreal_amd_reach_ddpg_variants')
    x.agent = DC.make_agent(lc, ec, sc, seed=c.seed, w3_scale=1.0)
    # the actor's parameters from numpy, as reach_cases._setup makes them (the seeds are found on the CPU and must mean
    # the same weights on the GPU); the gains and biases from set_layernorm's seeded CPU generator
    rs = np.random.RandomState(1000 + c.seed)
    with torch.no_grad():
        for i, fan_in in ((1, c.D), (2, c.H1), (3, c.H2)):
            for k in ('W%d' % i, 'b%d' % i):
                v = x.agent.model.actor.views[k]
                w = rs.uniform(-1.0, 1.0, size=tuple(v.shape)).astype(np.float32) / np.float32(np.sqrt(fan_in))
                v.copy_(torch.as_tensor(w * np.float32(c.scale if k == 'W3' else 1.0)))
        if ln:
            LN.set_layernorm(x.agent, seed=7 + c.seed)
        if params is not None:
            for k, v in params.items():
                (x.agent.model.actor_ln if k.startswith('ln') else x.agent.model.actor.views)[k].copy_(v)
    kk = dict(kernels=kernels) if kernels is not None else {}
    if task is not None:
        kk['task'] = task
    x.venv = SyntheticVecEnv(n, c.D, c.A, episode_len=EP, seeds=list(range(actor_base, actor_base + n)), device=device, **kk)
    x.replay = LN.replay_of(lc, ec, sc)
    x.sig = SIG[actor_base:actor_base + n].to(device).contiguous()
    stream = c.streams and device != 'cpu' and task == 'reach'
    if stream:
        x.venv.attach_monitor(capacity=4)
        x.venv.attach_noise(SEED, actor_base)
        x.eps_ref, x.eps = x.venv.noise.draws(sum(calls)), None
    else:
        x.eps_ref = x.eps = explicit_draws(c, device, actor_base, n, c.streams)
    if c.streams and task == 'reach':
        x.venv.attach_resets(RSEED, actor_base)
        x.venv.reset()
    if pop:
        assert actor_base % c.apa == 0
        x.pn = x.venv.attach_param_noise(x.agent, PSEED, actors_per_agent=c.apa, agent_base=actor_base // c.apa)
        x.pn.compute_dist_interval = INTERVAL
        x.pn.dist.fill_(-1.0)
    return x


def run(x, apw=0):
    """the case's calls of ddpg_rollout_into -> the rows written"""
    rows, s0 = 0, 0
    for T in x.calls:
        eps = None if x.eps is None else x.eps[s0:s0 + T]
        rows += x.venv.ddpg_rollout_into(x.agent, x.replay, T, eps=eps, sigmas=x.sig, actors_per_workgroup=apw)
        s0 += T
    return rows


def ring(x):
    """what a run left, on the CPU: the ring in row order, the state and the OU states (what the restatement returns)"""
    got = EC.ring_fields(x.replay, DC.FIELDS)
    got['state'], got['ou'] = x.venv.state, x.venv._ddpg['ou']
    if x.venv.device != 'cpu':
        torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in got.items()}


def everything(x):
    """ring(x) and the rest of the bytes a run leaves: the open transitions, the distances, the monitor's words"""
    got = ring(x)
    got.update({k: x.venv._ddpg[k].detach().cpu() for k in ('carry_obs', 'carry_act', 'carry_rew')})
    if x.pn is not None:
        got['dist'] = x.pn.dist.detach().cpu()
    if x.venv.monitor is not None:
        got.update({'mon_' + k: torch.as_tensor(v) for k, v in EM.monitor_state(x.venv.monitor).items()})
    return got


def population(x):
    """the agents' perturbed parameters as the launch reads them (DeviceParamNoise.perturbed), on the CPU"""
    return [{k: v.detach().cpu() for k, v in x.pn.perturbed(p).items()} for p in range(x.pn.agents)]


def clean_params(x):
    m = x.agent.model
    p = {k: v.detach().cpu() for k, v in m.actor.views.items()}
    if x.ln:
        p.update({k: v.detach().cpu() for k, v in m.actor_ln.items()})
    return p


# ---- the float64 restatement and its input conditions ------------------------------------------------------------------

class ProbedPolicy(R.DdpgPolicy):
    """DdpgPolicy that also keeps how close its kinks came (reach_cases.Margins): every hidden pre-activation of every
    agent's actor on its own actors' rows -- and of the clean actor on the measured rows -- and both action clips"""

    def _layers(self, p, x):
        h = x
        for i in (1, 2):
            z = h @ p['W%d' % i].t() + p['b%d' % i]
            self.margins.relu = min(self.margins.relu, float(z.abs().min()))
            h = torch.relu(z)
            if self.ln:
                h = R.layernorm(h, p['ln%d.W' % i], p['ln%d.b' % i], self.ln_eps)

    def mu(self, state):
        if self.acts in self.measure_at:
            self._layers(self.clean, state[::self.apa])
        out = super().mu(state)
        for p, lo in enumerate(range(0, state.shape[0], self.apa)):
            self._layers(self.pop[p], state[lo:lo + self.apa])
        self.margins.clipped(out)
        self._mu = out
        return out

    def act(self, state, eps, tau):
        a = super().act(state, eps, tau)
        self.margins.clipped(torch.clamp(self._mu, -1.0, 1.0) + self.ou)
        return a


def restatement(x, measure_at=None):
    """-> (want {field: float64}, rows, written mask, the policy: .margins, .env, .dist) on x's ring (rows to spare: the
    caller compares a wrapped ring by its bytes across block sizes instead); measure_at: the acts that measure
    (default: where the case's calls place them)"""
    c = x.c
    if x.venv.resets is not None:
        env = RRC.DrawnReachEnv(RRC.rows_of(x.n, c.A, x.lo), c.A, EP)
    else:
        env = RC.ReachEnv(x.venv.init_state, c.A, EP)
    m = x.agent.model
    clean = clean_params(x)
    kw = dict(noise='ou_noise', sigmas=x.sig, theta=x.agent.theta, dt=x.agent.dt, ln=x.ln, ln_eps=m.ln_eps if x.ln else 0.0)
    if x.pn is not None:
        pol = ProbedPolicy(population(x), x.n, c.A, actors_per_agent=c.apa, **kw)
        pol.clean = {k: R.f64(v) for k, v in clean.items()}
        pol.measure_at = measuring_acts(x.calls) if measure_at is None else tuple(measure_at)
    else:
        pol = ProbedPolicy(clean, x.n, c.A, **kw)
    pol.margins = RC.Margins()
    want, rows, written = R.ddpg_ring(pol, env, R.f64(x.eps_ref), sum(x.calls), N_STEP, GAMMA, x.capacity)
    pol.env = env
    return want, rows, written, pol


def margin_of(c):
    """twice MARGIN for a streams case: its draws on the GPU are the stream's own fp32, an ulp from the restatement's
    rounded here (and a population's copies the device's fills, an ulp from the double's)"""
    return (2 if c.streams else 1) * MARGIN


def tune(c, seeds=range(1000)):
    """-> the first seed under which the restatement meets the input conditions, the case's own first"""
    for seed in [c.seed] + list(seeds):
        t = c._replace(seed=seed)
        x = make(t, 'cpu', ReachVariantsCpuKernels())
        try:
            RC.input_conditions(restatement(x)[3], margin_of(c))
            return seed
        except AssertionError:
            continue
    return None


if __name__ == '__main__':          # prints TUNED's entries
    for c_ in CASES:
        got_ = tune(c_)
        if got_ != c_.seed:
            print('    %r: %r,' % (c_.id, got_), flush=True)
