"""
SyntheticVecEnv.rollout for an LSTM-stem PPO policy in one launch against the per-step stem path it replaces
(_rollout_stem: PPOAgent.act_batch + the step launch per step), shared by the CPU tier (test_lstm_rollout_cpu.py) and
the GPU tier (test_gpu_lstm_rollout.py):

  * ``LstmRolloutCpuKernels`` -- the torch-CPU double of the new entry points (a subclass of the existing double).  It
    composes the double's own ops step by step in the order the stem path issues them (z-filter, LSTM at T = 1, actor,
    sampling head, environment step), so the CPU tier compares bit for bit;
  * ``make_agent`` / ``run`` -- a recurrent PPOAgent with spread-out weights and one rollout on either path.
"""
import torch

import helpers as H
from cpu_kernels import TorchCpuKernels
from surreal_amd import _lib as L

RECORDED = ('obs', 'actions', 'rewards', 'dones', 'pds', 'cells')


class LstmRolloutCpuKernels(TorchCpuKernels):
    name = 'torch-cpu-double+lstm-rollout'

    def __init__(self):
        self.lstm_launches = 0

    def synth_lstm_rollout_supported(self, model):
        if not model.if_rnn or model.rnn_layers != 1 or model.if_pixel:
            return False
        a, r = model.actor, model.rnn
        return a.D == r.H and self.lib_supported('smx_synth_lstm_rollout_supported', r.D, r.H, a.H1, a.H2, a.OUT)

    def lstm_rollout_packed_numel(self, lstm):
        return 4

    def lstm_rollout_pack(self, lstm, packed):
        packed.zero_()                           # (the double reads the parameters themselves)

    def synth_lstm_rollout(self, model, packed, lstm_packed, state, init_state, noise_scale, eps, t, episode_len, steps,
                           slot, rolls, zfilter, hN, cN, h0=None, c0=None, h_before=None, c_before=None,
                           actors_per_workgroup=0):
        assert actors_per_workgroup in (0, 4, 8, 16)
        self.lstm_launches += 1
        n, D = state.shape
        Hp, Hl, A = model.rnn_hidden, model.rnn_hidden_logical, model.actor.OUT
        actor = model.actor
        r = rolls or {}
        h, c = torch.zeros(n, Hp), torch.zeros(n, Hp)
        if h0 is not None:
            h[:, :Hl], c[:, :Hl] = h0.reshape(n, Hl), c0.reshape(n, Hl)
        hb = cb = None
        for s in range(steps):
            row = slot + s
            if zfilter is not None:              # ZFilter.forward's two ops
                m, sd = torch.empty(D), torch.empty(D)
                self.zfilter_stats(zfilter.running_sum, zfilter.running_sumsq, zfilter.count, zfilter.eps, m, sd)
                x = torch.empty(n, D)
                self.zfilter_forward(state, m, sd, x)
            else:
                x = state.clone()
            hb, cb = h[:, :Hl].clone(), c[:, :Hl].clone()
            if 'cells' in r:
                r['cells'][:, row, 0, 0] = hb
                r['cells'][:, row, 1, 0] = cb
            out, gates, cs = torch.empty(n, Hp), torch.empty(n, 4 * Hp), torch.empty(n, Hp)
            hn, cn = torch.empty(n, Hp), torch.empty(n, Hp)
            self.lstm_forward(model.rnn, x, n, 1, h, c, gates, out, cs, None, hn, cn)
            h, c = torch.zeros(n, Hp), torch.zeros(n, Hp)
            h[:, :Hl], c[:, :Hl] = hn[:, :Hl], cn[:, :Hl]
            h1, h2, mean = torch.empty(n, actor.H1), torch.empty(n, actor.H2), torch.empty(n, A)
            self.mlp3_forward(actor, out, h1, h2, mean, L.SMX_ACT_TANH)
            acts, pd = torch.empty(n, A), torch.empty(n, 2 * A)
            self.diaggauss_sample(mean, model.log_var.view(-1), noise_scale, None if eps is None else eps[s], acts, pd)
            if 'pds' in r:
                r['pds'][:, row] = pd
            if r.get('obs_last') is not None and row + 1 == r['obs'].shape[1]:
                ac = acts.clamp(-1.0, 1.0)
                k = torch.arange(D)
                drift = 0.01 * (((37 * k) % 17) - 8).float()
                r['obs_last'].view(n, D).copy_(((0.9 * state + 0.5 * ac[:, k % A]) + drift).clamp(-10.0, 10.0))
            self.synth_env_step(state, init_state, acts, t, episode_len, row, r.get('obs'), r.get('actions'),
                                r.get('rewards'), r.get('dones'))
            t = 0 if t + 1 >= episode_len else t + 1
        hN.view(n, Hl).copy_(h[:, :Hl])
        cN.view(n, Hl).copy_(c[:, :Hl])
        if h_before is not None:
            h_before.view(n, Hl).copy_(hb)
            c_before.view(n, Hl).copy_(cb)


def configs(D, A, hidden=(24, 16), rnn_hidden=12, rnn_layer=1, use_z=True, pixel=None, T=6, n=4):
    from surreal_amd.main.ppo_configs import ppo_learner_config, ppo_env_config, ppo_session_config
    lc = ppo_learner_config()
    lc.algo.rnn.if_rnn_policy = True
    lc.algo.rnn.rnn_hidden = rnn_hidden
    lc.algo.rnn.rnn_layer = rnn_layer
    lc.algo.rnn.horizon = min(3, T)
    lc.algo.use_z_filter = use_z
    lc.algo.n_step = lc.algo.stride = T
    lc.replay.batch_size, lc.replay.memory_size, lc.replay.sampling_start_size = n, 2 * n, n
    lc.model.actor_fc_hidden_sizes = lc.model.critic_fc_hidden_sizes = list(hidden)
    ec = ppo_env_config(D, A, pixel=pixel)
    if pixel is not None:
        lc.model.cnn_feature_dim = 8
    return lc, ec, ppo_session_config(H.session_folder('surreal_amd_test_lstm_rollout'))


def make_agent(D, A, hidden=(24, 16), rnn_hidden=12, rnn_layer=1, use_z=True, deterministic=False, seed=3, pixel=None,
               T=6, n=4):
    from surreal_amd.agent import PPOAgent
    from surreal_amd import synthetic
    lc, ec, sc = configs(D, A, hidden, rnn_hidden, rnn_layer, use_z, pixel, T, n)
    agent = PPOAgent(lc, ec, sc, agent_id=1, agent_mode='eval_deterministic_local' if deterministic else 'training')
    if pixel is None:
        agent.model.load_params(synthetic.make_ppo_params(D, A, hidden=tuple(hidden), seed=seed, final_scale=2.0,
                                                          log_sig_spread=0.4, rnn_hidden=rnn_hidden,
                                                          rnn_layers=rnn_layer))
    if use_z:
        agent.model.z_filter.load_state_dict(synthetic.make_zfilter_state(D, seed=seed + 1))
    return agent, (lc, ec, sc)


def run(agent, n, D, A, T, episode_len, eps, persistent=True, actors_per_workgroup=0, device='cpu', pixel=None):
    """one rollout from a fresh environment -> (recorded tables, final state, clock, agent (h, c), agent cells before)"""
    from surreal_amd.env import SyntheticVecEnv
    venv = SyntheticVecEnv(n, D, A, episode_len=episode_len, seeds=list(range(n)), device=device, pixel=pixel)
    venv.persistent = persistent
    venv.start_rollout(T, info_width=2 * A)
    venv.rollout(agent, eps=eps, actors_per_workgroup=actors_per_workgroup)
    assert venv.slot == T
    out = {k: v.detach().cpu().clone() for k, v in venv.rolls.items()}
    out['state'] = venv.state.cpu().clone()
    cells = tuple(x.detach().cpu().clone().contiguous() for x in agent._batch_cells)
    before = tuple(x.detach().cpu().clone().contiguous() for x in agent.batch_cells_before)
    return out, venv.t, cells, before, venv
