"""
DDPGLearner for MI355X -- drop-in for ``surreal.learner.ddpg.DDPGLearner``
(surreal/learner/ddpg.py:12-440): same constructor, config keys, SSAR batch contract,
statistics keys; one iteration = target estimate, critic MSE step (Adam 1e-3), actor step
through the UPDATED critic (-mean Q, gradient value-clip 1, Adam 1e-4), hard / soft target
update (ddpg.py:244-352, 403-428), as a chain of HIP launches with no host synchronisation
until the statistics are read.

Dense layers run on the FP32-MFMA layer kernel (csrc/smx_gemm.hip); the critic's
"concatenate the action into layer 2" (builders.py:58-84) is done with row strides instead of a
copy: layer 1 writes into the first c1 columns of a [B, c1+A] buffer whose last A columns hold
the action.

The TD3 switches are built too (ddpg.py:119-147, 266-283, 312-319): ``use_double_critic`` (a
second critic with its own optimiser and target, y = min of the two targets, ``Q_policy2`` and
the second critic's loss reported as the reference does) and ``use_action_regularization``
(clipped noise on the target policy's action, drawn from numpy's global stream like the
reference's).  The iteration is captured once in a hipGraph and replayed: the Adam step count,
the learning rates and the hard-update decision live on the device.

Pixel observations (ddpg_net.py:37-88): the perception CNN (model/cnn_stem.py, the PPO stem's
kernels) runs on camera0 / 255, its features go in front of the low-dim vector, it is trained by
the critic loss (Adam with the critic's hyper-parameters) and follows the target updates; the actor
update reuses the features formed before the critic step, as the reference does.

Three launch schedules (_schedule): row blocks and dependency levels for low-dimensional observations with one critic, and
the layer-by-layer one (_enqueue_iteration_layers) that carries every switch.  TD3 without LayerNorm on low-dimensional
observations also runs on the row blocks when session_config.learner.ddpg_row_schedule is True (5 launches; opt-in).  What belongs to one critic -- model, target,
buffers, gradients, Adam group -- is one record (_critic_workspace): the second critic's update is the first one's code.

use_layernorm (default off) runs layer by layer too, with every other switch: the variant lives in DDPGModel's passes
(actor_forward ... actor_backward), the learner's iteration is the same.  With low-dimensional observations, one
rank and the fused update it also runs on the row blocks when session_config.learner.ddpg_row_schedule is True (4 launches,
5 with TD3's double critic; a LayerNorm rule behind each hidden layer's step; opt-in).  LayerNorm with camera observations, on
several ranks or with ddpg_rows_fused_update = False stays layer by layer.  torchx's LayerNorm semantics are unpinned (its source is absent): taken as
torch.nn.LayerNorm over the features.

TD3's third ingredient, delayed policy updates: learner_config.algo.network.policy_delay = d (optional, default 1 = the
reference's iteration).  Iteration k = critic_step after its increment updates the critic(s) as always; the actor -- Adam on the
count of ACTOR updates, k / d, a device word of its own -- and every target move when k % d == 0 only.  The host picks the
iteration's kind from k (every rank agrees), each kind has its own captured graph, and every schedule has a critic-only form:
the layer schedule ends after the last critic's step and the statistics, the levels lose the actor's problems and levels 11-19,
the rows run the chain programs without the actor's forward pass and 2 launches instead of 4 (3 instead of 5 with two
critics).  The statistics of a critic-only iteration read Q(s, mu(s)) as the last actor update left it (zeros before the first;
the buffer is workspace scratch: not part of train_state_dict).  d > 1 needs soft target updates.
"""
import gc
import types

import numpy as np
import torch

from surreal_amd import _lib as L
from surreal_amd import kernels as KN
from surreal_amd.learner.aggregator import SSARAggregator, FrameStackPreprocessor
from surreal_amd.learner.base import Learner, DeferredStats
from surreal_amd.learner.dist import _dist_info, setup_peer_exchange
from surreal_amd.model.ddpg_net import DDPGModel
from surreal_amd.session import ConfigError


def _grad_views(flat, named_params):
    """views by parameter name into a flat gradient buffer laid out like the parameters' own"""
    views, o = {}, 0
    for name, v in named_params:
        views[name] = flat[o:o + v.numel()].view(v.shape)
        o += v.numel()
    return views


def _stage(dst, src):
    """copy src into the staging buffer dst unless it IS dst -- the SAME buffer, not merely the same address: a strided /
    reshaped view that starts at the staging buffer's address is copied like any other source"""
    if not (src.data_ptr() == dst.data_ptr() and src.shape == dst.shape and src.stride() == dst.stride()
            and src.dtype == dst.dtype):
        dst.copy_(src)


class DDPGLearner(Learner):
    def __init__(self, learner_config, env_config, session_config):
        super().__init__(learner_config, env_config, session_config)
        self.K = KN.default_kernels()
        self.device = KN.default_device()
        self.current_iteration = 0
        self.batch_size = self.learner_config.replay.batch_size
        self.discount_factor = self.learner_config.algo.gamma
        self.n_step = self.learner_config.algo.n_step
        self.is_pixel_input = self.env_config.get('pixel_input', False)
        self.use_layernorm = self.learner_config.model.use_layernorm
        net = self.learner_config.algo.network
        self.use_double_critic = net.use_double_critic
        self.use_action_regularization = net.use_action_regularization
        # TD3's delayed policy updates: the actor and every target network move once per policy_delay critic updates
        # (1, the default: every iteration, the reference's ddpg.py:244-352)
        self.policy_delay = self._policy_delay(net)
        self._target_update_init()
        # data-parallel: every rank owns batch_size samples of the global batch (uniform replay shards
        # per GPU, ddpg_configs.py:89-93 / SURVEY.md 8(e)); gradients are averaged before each Adam step
        self._dist, self.world_size, self.rank = _dist_info()
        # several ranks: the iteration is ONE hipGraph too when its exchanges run as kernels over IPC-mapped peer buffers
        # (PeerExchange, set up and self-checked with the workspace); on the process group (RCCL) the launches stay eager
        self.use_graph = bool(self.session_config.learner.get('use_hip_graph', True)) and self.device != 'cpu'
        self.exchange_kind = None
        self._pending_stats = None
        self.lazy_stats = self.device != 'cpu' and bool(self.session_config.learner.get('lazy_stats', True))
        self.clip_actor_gradient = net.clip_actor_gradient
        self.actor_gradient_clip_value = net.actor_gradient_value_clip if self.clip_actor_gradient else 0.0
        self.clip_critic_gradient = net.clip_critic_gradient
        self.critic_gradient_clip_value = net.critic_gradient_value_clip if self.clip_critic_gradient else 0.0
        self.lr_actor, self.lr_critic = net.lr_actor, net.lr_critic
        self.actor_regularization = net.actor_regularization
        self.critic_regularization = net.critic_regularization
        self.action_dim = self.env_config.action_spec.dim[0]
        conv = self.learner_config.model.get('conv_spec', None) or {}
        mk = dict(obs_spec=self.env_config.obs_spec, action_dim=self.action_dim,
                  use_layernorm=self.use_layernorm,
                  actor_fc_hidden_sizes=self.learner_config.model.actor_fc_hidden_sizes,
                  critic_fc_hidden_sizes=self.learner_config.model.critic_fc_hidden_sizes,
                  conv_out_channels=conv.get('out_channels'), conv_kernel_sizes=conv.get('kernel_sizes'),
                  conv_strides=conv.get('strides'), conv_hidden_dim=conv.get('hidden_output_dim'),
                  device=self.device, kernels=self.K)
        self.model = DDPGModel(**mk)
        self.model_target = DDPGModel(**mk)
        self.model_target.load_state_dict(self.model.state_dict())       # hard_update (ddpg.py:175-176)
        self.is_pixel_input = self.model.is_pixel_input
        # Adam's (exp_avg, exp_avg_sq) per optimiser group; the perception CNN is in the critic's optimiser (ddpg_net.py:57-61)
        moments = lambda flat: None if flat is None else (torch.zeros_like(flat), torch.zeros_like(flat))  # noqa: E731
        self.actor_exp_avg, self.actor_exp_avg_sq = moments(self.model.actor_flat)
        self.critic_exp_avg, self.critic_exp_avg_sq = moments(self.model.critic_flat)
        self.perception_moments = moments(self.model.perception_flat)
        if self.use_double_critic:
            # TD3's second critic (ddpg.py:119-147, 162-166, 177-178): own parameters, optimiser, target
            self.model2 = DDPGModel(critic_only=True, **mk)
            self.model_target2 = DDPGModel(critic_only=True, **mk)
            self.model_target2.load_state_dict(self.model2.state_dict())
            self.critic2_moments = moments(self.model2.critic_flat)
            self.perception2_moments = moments(self.model2.perception_flat)
        self.actor_step = 0
        self.critic_step = 0
        self.frame_stack_concatenate_on_env = self.env_config.get('frame_stack_concatenate_on_env', True)
        self.frame_stack_preprocess = FrameStackPreprocessor(self.env_config.get('frame_stacks', 1))
        self.aggregator = SSARAggregator(self.env_config.obs_spec, self.env_config.action_spec)
        self._ws = None
        # independent layers of an iteration share launches (_enqueue_iteration_levels); off: one launch per layer
        self.level_schedule = bool(self.session_config.learner.get('ddpg_level_schedule', True))
        # the iteration on row blocks (smx_ddpg_rows.hip): two chain launches instead of fifteen dense ones.  Unset: used
        # for batches of up to 1024 rows per rank -- 4-row workgroups, measured 0.134 against 0.190 ms per iteration at
        # batch 512; past that more rounds of 4-row workgroups stream the weights again and the level schedule is used.  True / False
        # force it on (where the shapes allow) / off.
        rs = self.session_config.learner.get('ddpg_row_schedule', None)
        self.row_schedule = None if rs is None else bool(rs)
        # ... with a group's weight gradients formed in its update launch (one rank)
        self.rows_fused_update = bool(self.session_config.learner.get('ddpg_rows_fused_update', True))

    @staticmethod
    def _policy_delay(net):
        d = net.get('policy_delay', 1)
        if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or d < 1:
            raise ConfigError('learner_config.algo.network.policy_delay must be an integer >= 1, got %r' % (d,))
        if d > 1 and net.target_update.type == 'hard':
            raise ConfigError('learner_config.algo.network.policy_delay = %d needs target_update.type = "soft": what the '
                              'hard update\'s interval counts under a delay is not defined' % d)
        return int(d)

    def _updates_actor(self, k):
        """whether iteration k = 1, 2, ... (critic_step after its increment) also updates the actor and the targets"""
        return k % self.policy_delay == 0

    # ---- target update (ddpg.py:389-428) ----------------------------------------------------
    def _target_update_init(self):
        cfg = self.learner_config.algo.network.target_update
        self.target_update_type = cfg.type
        if self.target_update_type == 'soft':
            self.target_update_tau = cfg.tau
        elif self.target_update_type == 'hard':
            self.target_update_counter = 0
            self.target_update_interval = cfg.interval
        else:
            raise ConfigError('Unsupported ddpg update type: {}'.format(cfg.type))

    # ---- batch (ddpg.py:186-242) ---------------------------------------------------------------
    def _to_dev(self, x):
        if torch.is_tensor(x):
            return x.to(self.device, torch.float32)
        return torch.as_tensor(np.asarray(x), dtype=torch.float32).to(self.device)

    def preprocess(self, batch):
        for key in ('obs', 'obs_next'):
            for modality in batch[key]:
                for k in batch[key][modality]:
                    v = batch[key][modality][k]
                    if modality == 'pixel':      # stay uint8: the patch kernel applies / 255 while reading
                        v = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))
                        batch[key][modality][k] = v.to(self.device)
                    else:
                        batch[key][modality][k] = self._to_dev(v)
        for key in ('actions', 'rewards', 'dones'):
            batch[key] = self._to_dev(batch[key])
        return batch
    preprocess.device_move_only = True       # (start_prefetching: the pinned stager does exactly this move)

    def _workspace(self, B, D):
        if self._ws is not None and self._ws.key == (B, D):
            return self._ws
        m, mt, A = self.model, self.model_target, self.action_dim
        f = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)  # noqa: E731
        ws = types.SimpleNamespace(key=(B, D))
        a, c1, c2 = m.actor, m.c1, m.c2
        # the Adam step count and the learning rates live on the device: one captured hipGraph of
        # the iteration is replayed while they change (smx_adam_step_dev_f32)
        ws.step = torch.full((1,), self.critic_step, dtype=torch.int32, device=self.device)
        ws.dev_step = self.critic_step
        ws.lr = torch.tensor([self.lr_actor, self.lr_critic], dtype=torch.float32, device=self.device)
        ws.lr_host = (self.lr_actor, self.lr_critic)
        ws.act, ws.q_next, ws.q_actor, ws.q_policy = f(B, A), f(B), f(B), f(B)
        # a delayed policy update: the actor's Adam counts ITS updates in a word of its own, and the statistics of the
        # iterations before the first actor update read Q(s, mu(s)) = 0
        ws.astep, ws.dev_astep = None, self.actor_step
        if self.policy_delay > 1:
            ws.astep = torch.full((1,), self.actor_step, dtype=torch.int32, device=self.device)
            ws.q_actor.zero_()
        if self.is_pixel_input:
            ws.dxin = f(B, m.input_dim)
            ws.cnn_sk = m._cnn_stem.splitk_workspace(m.cnn, B, self.device)
            ws.s_pix = ws.s_pix_next = None              # staged frames (allocated in their dtype)
        c = self._critic_workspace(ws, m, mt, (self.critic_exp_avg, self.critic_exp_avg_sq), self.perception_moments)
        ws.critics = [c]
        if self.use_double_critic:
            ws.critics.append(self._critic_workspace(ws, self.model2, self.model_target2, self.critic2_moments,
                                                     self.perception2_moments))
            ws.q_next2, ws.stats2 = f(B), ws.critics[1].stats
        ws.bw = m.backward_workspace(B, self.device)          # (one critic or the actor at a time)
        ws.dz2, ws.dxcat, ws.dz3a, ws.dz2a, ws.dz1a = ws.bw.dz2, ws.bw.dxcat, ws.bw.dz3a, ws.bw.dz2a, ws.bw.dz1a
        # the first critic's buffers under the names the row and level schedules know them by: its (and the actor's)
        # forward workspace -- h1a, h2a, xcat, h2c without LayerNorm --, gradients, Q, y, dLoss/dQ, statistics
        for k, v in vars(c.w).items():
            setattr(ws, k, v)
        ws.grads_c, ws.gc, ws.q, ws.y, ws.dz3, ws.stats = c.grads, c.gv, c.q, c.y, c.dz3, c.stats
        ws.grads_a = torch.zeros_like(m.actor_flat)
        ws.ga = _grad_views(ws.grads_a, list(a.views.items()) + list(m.actor_ln.items()))
        ws.adam_actor = (m.actor_flat, ws.grads_a, self.actor_exp_avg, self.actor_exp_avg_sq, ws.lr[0:1],
                         self.actor_regularization, self.actor_gradient_clip_value)
        # (target, source) buffers of the target-network update (ddpg.py:344-352): actor + critic as the one buffer they
        # share when both models have it, then the perception CNN, the second critic and its perception CNN
        if getattr(mt, 'ac_flat', None) is not None and getattr(m, 'ac_flat', None) is not None:
            ws.target_pairs = [(mt.ac_flat, m.ac_flat)]
        else:
            ws.target_pairs = [(mt.actor_flat, m.actor_flat), (mt.critic_flat, m.critic_flat)]
        if self.is_pixel_input:
            ws.target_pairs.append((mt.perception_flat, m.perception_flat))
        for second in ws.critics[1:]:
            ws.target_pairs.append((second.target.critic_flat, second.model.critic_flat))
            if self.is_pixel_input:
                ws.target_pairs.append((second.target.perception_flat, second.model.perception_flat))
        # the levelled schedule (_enqueue_iteration_levels) keeps the four forward chains of an iteration apart: target
        # actor, target critic, critic, actor each have their own activations, so independent layers share a launch
        ws.h1a_t, ws.h2a_t = f(B, a.H1), f(B, a.H2)
        ws.xcat_t, ws.h2c_t = f(B, c1 + A), f(B, c2)
        ws.xcat_a, ws.h2c_a = f(B, c1 + A), f(B, c2)
        ws.dz3_actor = torch.full((B,), -1.0 / B, device=self.device)       # d(-mean Q) / dQ  (ddpg.py:331)
        # the batch is staged into fixed buffers (5 small copies) so that the graph's pointers hold
        ws.s_obs, ws.s_next, ws.s_act, ws.s_rew, ws.s_done = f(B, D), f(B, D), f(B, A), f(B), f(B)
        if self.use_action_regularization:
            ws.s_noise, ws.act_n = f(B, A), f(B, A)
        ws.graph = ws.graph_critic = None         # the captured iteration; the critic-only one of a delayed policy update
        self._rank_weight = 1.0
        ws.xerr = torch.zeros(1, dtype=torch.int32, device=self.device) if self.device != 'cpu' else None
        if self.world_size > 1:            # a rank's share of the global batch: the means are weighted sums
            mine = torch.tensor([B], dtype=torch.int64, device=self.device)
            every = torch.empty(self.world_size, dtype=torch.int64, device=self.device)
            self._dist.all_gather_into_tensor(every, mine)
            self._rank_weight = float(B) / float(sum(every.tolist()))
            self._setup_peer_exchange(ws)
        self._ws = ws
        return ws

    def _critic_workspace(self, ws, model, target, moments, perception_moments):
        """what belongs to ONE critic: model and target, their forward workspaces, Q / y / dLoss/dQ, the gradient buffer
        with its views by parameter name, the statistics block and the Adam group (parameters, gradients, exp_avg,
        exp_avg_sq, lr slot, decay, value clip: _enqueue_adam) -- with camera observations its perception CNN's features
        of s / s', workspaces, gradients and Adam group as well"""
        B = ws.key[0]
        f = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)  # noqa: E731
        c = types.SimpleNamespace(model=model, target=target, q=f(B), y=f(B), dz3=f(B),
                                  stats=torch.zeros(8, device=self.device), grads=torch.zeros_like(model.critic_flat))
        c.w = model.workspace(B, self.device)
        c.w_t = target.target_workspace(c.w, B, self.device)
        c.gv = _grad_views(c.grads, model.critic.items())
        c.adam = (model.critic_flat, c.grads) + moments + (ws.lr[1:2], self.critic_regularization,
                                                           self.critic_gradient_clip_value)
        c.adam_p = None
        if self.is_pixel_input:
            from surreal_amd.model.cnn_stem import CnnStem
            c.xf, c.xnf = f(B, model.input_dim), f(B, model.input_dim)
            c.cnn = CnnStem.workspace(model.cnn, B, self.device, backward=True)
            c.cnn.sk = ws.cnn_sk
            c.cnn_t = CnnStem.workspace(model.cnn, B, self.device, backward=False)
            c.grads_p = torch.zeros_like(model.perception_flat)
            # the critic's optimiser and decay, but no clip: ddpg.py:308-309 clips self.model.critic alone
            c.adam_p = (model.perception_flat, c.grads_p) + perception_moments + (ws.lr[1:2], self.critic_regularization, 0.0)
        return c

    def _setup_peer_exchange(self, ws):
        """several ranks on one node: the gradient / statistics all-reduces of an iteration (ddpg.py:244-400 run on
        shards: SURVEY.md 8(e) "same pattern, 2 grad all-reduces per iteration") as kernels over IPC-mapped peer buffers
        -- set up and SELF-CHECKED once, collectively; any failure leaves the process group in place and the launches
        eager.  session_config.learner.peer_exchange = False keeps the process group."""
        groups = [ws.adam_actor] + [g for c in ws.critics for g in (c.adam, c.adam_p) if g is not None]
        setup_peer_exchange(self, ws.xerr, max([64] + [grads.numel() for _, grads, *_ in groups]))
        self.exchange_kind = self._dist.kind()
        if self._dist.exchange is None:
            self.use_graph = False            # process-group collectives are not captured

    def _enqueue_adam(self, ws, group, step=None):
        """one optimiser group's Adam step (the actor's, a critic's, a critic's perception CNN's); step count and lr are
        read on the device"""
        flat, grads, exp_avg, exp_avg_sq, lr, decay, clip = group
        self.K.adam_step_dev(flat, grads, exp_avg, exp_avg_sq, lr, ws.step if step is None else step, decay, clip)

    def _enqueue_actor_adam(self, ws):
        """the actor's Adam step.  With a delayed policy update its step count is the number of ACTOR updates: the word of
        its own moves first"""
        if ws.astep is not None:
            ws.astep.add_(1)
        self._enqueue_adam(ws, ws.adam_actor, ws.astep)

    def _enqueue_target_update(self, ws):
        """ddpg.py:389-428"""
        for tgt, src in ws.target_pairs:
            if self.target_update_type == 'soft':
                self.K.soft_update(tgt, src, self.target_update_tau)
            else:
                self.K.hard_update_every(tgt, src, ws.step, self.target_update_interval)

    def _average_over_ranks(self, t):
        """a per-rank mean -> the mean over the global batch: weighted by the rank's share of it, then
        one all-reduce; a no-op for one rank"""
        if self.world_size > 1:
            t.mul_(self._rank_weight)
            self._dist.all_reduce(t)

    def _enqueue_iteration_levels(self, ws, x, xn, actions, rewards, done, update=True):
        """One DDPG iteration (ddpg.py:244-352; low-dimensional observations, one critic, one rank) scheduled by
        DEPENDENCY LEVEL: the layers of the target actor, the target critic, the critic and the actor that do not
        depend on each other share a launch (smx_linear_multi_f32), and so do a level's weight gradients --
        22 dependent launches where the layer-by-layer schedule takes ~40 (each ~6 us at batch 512: the
        iteration is launch-latency bound).  The arithmetic of every layer is the same kernel with the same
        operands as in _enqueue_iteration_layers: identical results.
        The actor's forward pass for ITS update (ddpg.py:326-329) only reads the actor's parameters, which the
        critic update does not touch, so it rides in levels 1-3."""
        K, m, mt, A = self.K, self.model, self.model_target, self.action_dim
        B, D = x.shape
        a, ta, c, tc = m.actor.views, mt.actor.views, m.critic, mt.critic
        c1, c2, ld = m.c1, m.c2, m.c1 + A
        H1, H2 = m.actor.H1, m.actor.H2
        R, T = L.SMX_ACT_RELU, L.SMX_ACT_TANH
        # (update False -- a critic-only iteration of a delayed policy update: the actor's problems leave levels 1-3,
        # levels 11-19 and the target update are skipped)
        only = (lambda *problems: list(problems)) if update else (lambda *problems: [])
        # 1: first layers of all four chains (none depends on another) -- and the batch's actions into the last A columns
        # of the critic's concat buffer as a fifth problem of the launch, actions . I^T (exact for FINITE actions: one product
        # with 1, the rest with 0 -- the contract |a| <= 1 of ddpg.py:262-263, which the statistics launch checks on `actions`
        # itself; an Inf would turn its row's other columns into NaN here, -0.0 becomes +0.0); as a strided torch copy in
        # front it was a 9 us launch of its own
        if getattr(ws, 'eyeA', None) is None:
            ws.eyeA = torch.eye(A, device=self.device)
        K.linear_multi([('linear', xn, 1, ta['W1'], 1, ta['b1'], ws.h1a_t, B, H1, D, dict(act=R)),
                        ('linear', xn, 1, tc['W1'], 1, tc['b1'], ws.xcat_t, B, c1, D, dict(act=R, ldc=ld)),
                        ('linear', x, 1, c['W1'], 1, c['b1'], ws.xcat, B, c1, D, dict(act=R, ldc=ld))]
                       + only(('linear', x, 1, a['W1'], 1, a['b1'], ws.h1a, B, H1, D, dict(act=R)))
                       + [('linear', actions, 1, ws.eyeA, 1, None, ws.xcat[:, c1:], B, A, A, dict(ldc=ld))])
        # 2
        K.linear_multi([('linear', ws.h1a_t, 1, ta['W2'], 1, ta['b2'], ws.h2a_t, B, H2, H1, dict(act=R)),
                        ('linear', ws.xcat, 1, c['W2'], 1, c['b2'], ws.h2c, B, c2, ld, dict(act=R))]
                       + only(('linear', ws.h1a, 1, a['W2'], 1, a['b2'], ws.h2a, B, H2, H1, dict(act=R))))
        # 3: the target policy's action lands in the target critic's concat buffer, the policy's own action in the
        # concat buffer of the actor update's critic pass
        K.linear_multi([('linear', ws.h2a_t, 1, ta['W3'], 1, ta['b3'], ws.xcat_t[:, c1:], B, A, H2, dict(act=T, ldc=ld)),
                        ('linear', ws.h2c, 1, c['W3'], 1, c['b3'], ws.q.view(B, 1), B, 1, c2, dict(act=0))]
                       + only(('linear', ws.h2a, 1, a['W3'], 1, a['b3'], ws.xcat_a[:, c1:], B, A, H2, dict(act=T, ldc=ld)),
                              ('linear', ws.h2a, 1, a['W3'], 1, a['b3'], ws.act, B, A, H2, dict(act=T))))   # (dense copy: tanh')
        # 4, 5: Q'(s', mu'(s'))
        K.linear(ws.xcat_t, 1, tc['W2'], 1, tc['b2'], ws.h2c_t, B, c2, ld, act=R)
        K.linear(ws.h2c_t, 1, tc['W3'], 1, tc['b3'], ws.q_next.view(B, 1), B, 1, c2, act=0)
        # 6: y, critic loss gradient, the iteration's Adam step count
        K.ddpg_critic_loss_step(ws.q, ws.q_next, rewards, done, pow(self.discount_factor, self.n_step), ws.y, ws.dz3,
                                ws.step)
        # 7-9: critic backward; a layer's weight gradient shares the launch of the next data gradient
        dz3 = ws.dz3.view(B, 1)
        K.linear_multi([('linear', dz3, 1, c['W3'], 0, None, ws.dz2, B, c2, 1, dict(relu_mask=ws.h2c, lda=1, ldb=c2)),
                        ('wgrad', dz3, ws.h2c, ws.gc['W3'], ws.gc['b3'], 1, c2, B, dict(ldz=1))])
        K.linear_multi([('linear', ws.dz2, 1, c['W2'], 0, None, ws.dxcat, B, c1, c2,
                         dict(relu_mask=ws.xcat, ldb=ld, ldc=ld)),
                        ('wgrad', ws.dz2, ws.xcat, ws.gc['W2'], ws.gc['b2'], c2, ld, B, {})])
        K.linear_wgrad(ws.dxcat, x, ws.gc['W1'], ws.gc['b1'], c1, D, B, ldz=ld)
        # 10
        self._enqueue_adam(ws, ws.critics[0].adam)
        if not update:               # (the statistics on Q(s, mu(s)) as the last actor update left it)
            K.ddpg_stats(ws.q, ws.y, rewards, actions, ws.q_actor, ws.stats)
            return
        # 11-13: Q(s, mu(s)) through the UPDATED critic; d(-mean Q)/d(layer 2) needs only that pass's ReLU mask
        K.linear(x, 1, c['W1'], 1, c['b1'], ws.xcat_a, B, c1, D, act=R, ldc=ld)
        K.linear(ws.xcat_a, 1, c['W2'], 1, c['b2'], ws.h2c_a, B, c2, ld, act=R)
        K.linear_multi([('linear', ws.h2c_a, 1, c['W3'], 1, c['b3'], ws.q_actor.view(B, 1), B, 1, c2, dict(act=0)),
                        ('linear', ws.dz3_actor.view(B, 1), 1, c['W3'], 0, None, ws.dz2, B, c2, 1,
                         dict(relu_mask=ws.h2c_a, lda=1, ldb=c2))])
        # 14, 15: d/d(action), through tanh
        K.linear(ws.dz2, 1, c['W2'][:, c1:], 0, None, ws.dz3a, B, A, c2, ldb=ld)
        K.tanh_backward(ws.dz3a, ws.act, ws.dz3a)
        # 16-18: actor backward (data gradients, weight gradients), 19: its Adam step
        K.mlp3_backward(m.actor, x, ws.h1a, ws.h2a, ws.dz3a, ws.dz2a, ws.dz1a, ws.grads_a, None)
        self._enqueue_actor_adam(ws)
        K.ddpg_stats(ws.q, ws.y, rewards, actions, ws.q_actor, ws.stats)
        self._enqueue_target_update(ws)

    def _rows_dims(self, D, rows=None):
        """(D, A, H1, H2, c1, c2) when the row-block kernels take these shapes (for a batch of `rows`), else None"""
        m = self.model
        dims = (D, self.action_dim, m.actor.H1, m.actor.H2, m.c1, m.c2)
        if self.use_layernorm:
            # LayerNorm: low-dimensional observations, one rank, the fused update (the gains' and biases' gradients are
            # formed by the gradient-and-step launch alone) -- everything else stays layer by layer
            ok = (rows is not None and not self.is_pixel_input and self.world_size == 1
                  and self.rows_fused_update and KN.ddpg_rows_ln(self.K) and self.K.ddpg_rows_ln_supported(*dims, rows))
            if ok and self.use_double_critic:
                # ... with TD3's second critic where the kernels run that cell too: y kept between the two losses.  (The
                # library's last predicate implies the TD3 one; both are asked because a kernels object -- a test
                # double -- may answer each more loosely)
                ok = (KN.ddpg_rows_ln_td3(self.K) and KN.ddpg_rows_td3(self.K)
                      and self.K.ddpg_rows_second_supported(*dims, rows) and self.K.ddpg_rows_ln_second_supported(*dims, rows))
            return dims if ok and self.K.ddpg_rows_supported(*dims, rows=rows) else None
        if self.use_double_critic and not (rows is not None and KN.ddpg_rows_td3(self.K)
                                           and self.K.ddpg_rows_second_supported(*dims, rows)):
            return None              # (TD3's chain keeps y between the two losses and addresses more buffers)
        return dims if self.K.ddpg_rows_supported(*dims, rows=rows) else None

    def _rows_args(self, ws, x, xn, actions, rewards, done):
        if getattr(ws, 'rows_args', None) is not None and ws.rows_key == (x.data_ptr(), xn.data_ptr(), actions.data_ptr(),
                                                                         rewards.data_ptr(), done.data_ptr()):
            return ws.rows_args
        K, m, mt = self.K, self.model, self.model_target
        dims = self._rows_dims(x.shape[1], x.shape[0])
        ws.rows_packed = torch.zeros(K.ddpg_rows_packed_floats(*dims), device=self.device)
        ws.rows_versions = None          # nothing packed yet
        if getattr(ws, 'stats_slots', None) is None:      # (two blocks of 8 per slot with a second critic)
            ws.stats_slots = torch.zeros(2, 16 if self.use_double_critic else 8, pin_memory=torch.cuda.is_available())
        nets = {'actor': m.actor.views, 'critic': m.critic, 'target_actor': mt.actor.views, 'target_critic': mt.critic}
        ln = self.use_layernorm
        # (LayerNorm: what the weight gradients multiply are the LayerNorm outputs -- the layer schedule's c_n2, n1, n2)
        io = dict(x=x, x_next=xn, actions=actions, rewards=rewards, dones=done, xcat=ws.xcat, h2c=ws.c_n2 if ln else ws.h2c,
                  q=ws.q, q_next=ws.q_next, y=ws.y, dz3=ws.dz3, dz2=ws.dz2, dxcat=ws.dxcat, h1a=ws.n1 if ln else ws.h1a,
                  h2a=ws.n2 if ln else ws.h2a, act=ws.act, q_actor=ws.q_actor, dz3a=ws.dz3a, dz2a=ws.dz2a, dz1a=ws.dz1a,
                  step=ws.step)
        ws.rows_args = K.ddpg_rows_args(dims, nets, ws.rows_packed, io, pow(self.discount_factor, self.n_step))
        if ln:
            # the gains and biases (read row-major from the parameter buffers: no packed copy) and exactly the layer
            # schedule's buffers: the workspace of DDPGModel's passes and their backward scratch, allocated once
            ln_nets = {'actor': m.actor_ln, 'critic': m.critic, 'target_actor': mt.actor_ln, 'target_critic': mt.critic}
            io_ln = dict(c_a1=ws.c_a1, cm1=ws.cm1, cr1=ws.cr1, c_a2=ws.c_a2, cm2=ws.cm2, cr2=ws.cr2, dn2=ws.bw.dn2,
                         dz1c=ws.bw.dz1c, a1=ws.a1, am1=ws.am1, ar1=ws.ar1, a2=ws.a2, am2=ws.am2, ar2=ws.ar2,
                         dn2a=ws.bw.dn2a, dn1a=ws.bw.dn1a)
            ws.rows_args = K.ddpg_rows_ln_attach(ws.rows_args, ln_nets, m.ln_eps, io_ln)
        if self.use_double_critic:
            # TD3: the second critic's networks, its own packed buffer and its own buffers -- dz2 / dxcat too (ws.bw is
            # one critic's at a time; here both critics' data gradients exist before either weight-gradient launch)
            s = ws.critics[1]
            B, c1, c2, A = x.shape[0], m.c1, m.c2, self.action_dim
            ws.rows_packed2 = torch.zeros(K.ddpg_rows_second_packed_floats(*dims), device=self.device)
            ws.dz2_2 = torch.zeros(B, c2, device=self.device)
            ws.dxcat2 = torch.zeros(B, c1 + A, device=self.device)
            nets2 = {'critic2': s.model.critic, 'target_critic2': s.target.critic}
            io2 = dict(noise=ws.s_noise if self.use_action_regularization else None, xcat2=s.w.xcat,
                       h2c2=s.w.c_n2 if ln else s.w.h2c, q2=s.q, q_next2=ws.q_next2, dz3_2=s.dz3, dz2_2=ws.dz2_2,
                       dxcat2=ws.dxcat2, stats2=s.stats)
            ws.rows_args = K.ddpg_rows_second(ws.rows_args, nets2, ws.rows_packed2, io2)
            if ln:
                # ... and its LayerNorms: the second critic's gains and biases in place, its forward workspace, and dn2 /
                # dz1 of its own (as dz2_2 / dxcat2 above: both critics' backward passes precede either step)
                ws.dn2_2 = torch.zeros(B, c2, device=self.device)
                ws.dz1c2 = torch.zeros(B, c1, device=self.device)
                io_ln2 = dict(c2_a1=s.w.c_a1, c2m1=s.w.cm1, c2r1=s.w.cr1, c2_a2=s.w.c_a2, c2m2=s.w.cm2, c2r2=s.w.cr2,
                              dn2_2=ws.dn2_2, dz1c2=ws.dz1c2)
                ws.rows_args = K.ddpg_rows_ln_second_attach(ws.rows_args, nets2, io_ln2)
        ws.rows_key = (x.data_ptr(), xn.data_ptr(), actions.data_ptr(), rewards.data_ptr(), done.data_ptr())
        return ws.rows_args

    def _enqueue_iteration_rows(self, ws, x, xn, actions, rewards, done, update=True):
        """One DDPG iteration (ddpg.py:244-352; low-dimensional observations, one critic -- TD3's two below) on ROW BLOCKS: a
        workgroup carries 4 batch rows through whole chains -- target actor -> target critic -> y, critic -> loss ->
        its data gradients, and the actor's forward pass in one launch; Q(s, mu(s)) through the updated critic -> the
        actor's data gradients in a second (smx_ddpg_rows.hip).  Weight gradients (sums over all rows), Adam, the
        target update and the statistics are the launches of the other schedules, on the same buffers: 10 launches where
        the level schedule takes 22.  The MFMA loop sums a layer's products in another order than smx_linear_f32:
        equal to the level schedule within fp32 rounding (tests/test_gpu_ddpg.py), not bit for bit.
        TD3 (use_double_critic, with or without action regularisation): the critic chain carries both target critics --
        the second at the noised, clamped action --, y = min of the two targets and both critics' losses and data
        gradients (smx_ddpg_rows_critic_td3_f32); the second critic's step is a third update launch between the first
        critic's and the actor chain, which goes through the first critic only.  5 launches, no ATen arithmetic.
        use_layernorm (one rank, the fused update: _rows_dims): the same 4 launches with a LayerNorm rule behind
        every hidden layer's step and its backward rule behind the backward products, on the buffers of DDPGModel's
        passes; the gains' and biases' gradients and steps are further workgroups of the group's gradient-and-step launch.
        With a double critic it is TD3's 5 launches, the LayerNorm rules behind TD3's chain and the second critic's gains
        and biases stepped by its own gradient-and-step launch.  LayerNorm with camera observations, on several ranks or
        with ddpg_rows_fused_update = False stays layer by layer (_schedule).
        policy_delay > 1, a critic-only iteration (update False): the critic chain without the actor's forward pass
        (smx_ddpg_rows_critic_only_f32 / _td3_f32: the same kernels, a shorter step table) and the critic groups'
        gradient-and-step launches WITHOUT their target, the last of them carrying the statistics (Q(s, mu(s)) as the last
        actor update left it) -- 2 launches, 3 with TD3; no actor chain, no actor step.  Its update iterations are the 4 / 5
        launches with the actor's step reading the actor's own step word, and one workgroup more between the actor chain
        and that step (smx_ddpg_rows_delay_tail_f32): the statistics -- their host slot goes by the iteration's word, which
        the actor's launch no longer reads -- and the word's increment.  5 / 6 launches."""
        K, m, mt, A = self.K, self.model, self.model_target, self.action_dim
        B, D = x.shape
        c1, c2, ld = m.c1, m.c2, m.c1 + A
        H1, H2 = m.actor.H1, m.actor.H2
        args = self._rows_args(ws, x, xn, actions, rewards, done)
        gc, ga = ws.gc, ws.ga
        # every network's weights in fragment order: the update launches below keep the copies current element by
        # element; a full pack only when something ELSE wrote parameters since (construction, a checkpoint, a fetched
        # state dict -- _rows_refresh, outside a captured graph)
        if not torch.cuda.is_available() or not torch.cuda.is_current_stream_capturing():
            self._rows_refresh(ws)
        soft = self.target_update_type == 'soft'
        tgt = dict(tau=self.target_update_tau if soft else 0.0, interval=0 if soft else self.target_update_interval)
        # one rank: a group's weight gradients and its step are ONE launch (value clipping needs no norm over the group);
        # several: the gradients are averaged over the ranks between them
        fuse = self.world_size == 1 and self.rows_fused_update
        assert fuse or not self.use_layernorm
        second = ws.critics[1] if self.use_double_critic else None
        delayed = ws.astep is not None
        if not update:               # (a critic-only iteration: the targets stay, the last critic group reports)
            tgt = dict(tau=0.0, interval=0)
            last = dict(stats=ws.stats if fuse else None, stats_host=ws.stats_slots if fuse and self.lazy_stats else None)
        if second is not None:
            (K.ddpg_rows_critic_td3 if update else K.ddpg_rows_critic_only_td3)(args)
        else:
            (K.ddpg_rows_critic if update else K.ddpg_rows_critic_only)(args)
        if not fuse:
            K.linear_multi([('wgrad', ws.dxcat, x, gc['W1'], gc['b1'], c1, D, B, dict(ldz=ld)),
                            ('wgrad', ws.dz2, ws.xcat, gc['W2'], gc['b2'], c2, ld, B, {}),
                            ('wgrad', ws.dz3.view(B, 1), ws.h2c, gc['W3'], gc['b3'], 1, c2, B, dict(ldz=1))])
            self._average_over_ranks(ws.grads_c)
        K.ddpg_rows_update(args, 'critic', m.critic_flat, ws.grads_c, self.critic_exp_avg, self.critic_exp_avg_sq,
                           ws.lr[1:2], ws.step, self.critic_regularization, self.critic_gradient_clip_value,
                           target=mt.critic_flat if update else None, wgrad=fuse,
                           **(tgt if update or second is not None else dict(tgt, **last)))
        if second is not None:
            g2, w2 = second.gv, second.w
            if not fuse:
                K.linear_multi([('wgrad', ws.dxcat2, x, g2['W1'], g2['b1'], c1, D, B, dict(ldz=ld)),
                                ('wgrad', ws.dz2_2, w2.xcat, g2['W2'], g2['b2'], c2, ld, B, {}),
                                ('wgrad', second.dz3.view(B, 1), w2.h2c, g2['W3'], g2['b3'], 1, c2, B, dict(ldz=1))])
                self._average_over_ranks(second.grads)
            K.ddpg_rows_update(args, 'critic2', second.model.critic_flat, second.grads, self.critic2_moments[0],
                               self.critic2_moments[1], ws.lr[1:2], ws.step, self.critic_regularization,
                               self.critic_gradient_clip_value, target=second.target.critic_flat if update else None,
                               wgrad=fuse, **(tgt if update else dict(tgt, **last)))
        if update:
            K.ddpg_rows_actor(args)
            if not fuse:
                K.linear_multi([('wgrad', ws.dz1a, x, ga['W1'], ga['b1'], H1, D, B, {}),
                                ('wgrad', ws.dz2a, ws.h1a, ga['W2'], ga['b2'], H2, H1, B, {}),
                                ('wgrad', ws.dz3a, ws.h2a, ga['W3'], ga['b3'], A, H2, B, {})])
                self._average_over_ranks(ws.grads_a)
            # the statistics ride in the actor's launch -- unless the learner delays its policy updates: the actor's
            # launch then reads the ACTOR's step word, and the workgroup in front of it reports and moves that word
            ride = fuse and not delayed
            if delayed and fuse:
                K.ddpg_rows_delay_tail(args, ws.astep, stats=ws.stats,
                                       stats_host=ws.stats_slots if self.lazy_stats else None)
            elif delayed:
                ws.astep.add_(1)
            K.ddpg_rows_update(args, 'actor', m.actor_flat, ws.grads_a, self.actor_exp_avg, self.actor_exp_avg_sq,
                               ws.lr[0:1], ws.astep if delayed else ws.step, self.actor_regularization,
                               self.actor_gradient_clip_value, target=mt.actor_flat, wgrad=fuse,
                               stats=ws.stats if ride else None,
                               stats_host=ws.stats_slots if ride and self.lazy_stats else None, **tgt)
        ws.stats_zero_copy = bool(fuse and self.lazy_stats)
        if not fuse:                 # (fused: the statistics are one more workgroup of the actor's launch)
            K.ddpg_stats(ws.q, ws.y, rewards, actions, ws.q_actor, ws.stats)
            self._average_over_ranks(ws.stats[:6])
            if second is not None:       # the second critic's loss and Q_policy2, as the layer schedule reports them
                K.ddpg_stats(second.q, ws.y, rewards, actions, second.q, second.stats)
                self._average_over_ranks(second.stats[:6])
        ws.rows_versions = self._rows_versions()

    def _rows_versions(self):
        """torch's write counters of the four parameter buffers (six with a second critic): the HIP launches do not move
        them (raw pointers), anything that writes parameters through torch does"""
        m, mt = self.model, self.model_target
        flats = [m.actor_flat, m.critic_flat, mt.actor_flat, mt.critic_flat]
        if self.use_double_critic:
            flats += [self.model2.critic_flat, self.model_target2.critic_flat]
        return tuple(int(t._version) for t in flats)

    def _rows_refresh(self, ws):
        """the row schedule's fragment-order copies follow the parameters through ddpg_rows_update only: repack all of
        them when the parameters were written from outside since the last iteration (or never packed)"""
        args = getattr(ws, 'rows_args', None)
        if args is not None and getattr(ws, 'rows_versions', None) != self._rows_versions():
            self.K.ddpg_rows_pack(args)
            if self.use_double_critic:
                self.K.ddpg_rows_pack_second(args)
            ws.rows_versions = self._rows_versions()

    def _enqueue_critic_update(self, ws, c, x):
        """critic c's step from c.dz3 = dLoss/dQ: backward -> perception backward -> rank averaging -> Adam on the critic
        -> Adam on its perception CNN"""
        dz1, ld = c.model.critic_backward(x, c.w, ws.bw, c.dz3, c.gv)
        if self.is_pixel_input:
            # the critic loss's gradient through the perception CNN (ddpg.py:304-308: critic_loss.backward() reaches
            # model.perception): d(critic layer 1 input) = dz1 . W1, masked by the feature ReLU, then the stem's own backward
            model, B = c.model, x.shape[0]
            self.K.linear(dz1, 1, model.critic['W1'], 0, None, ws.dxin, B, model.input_dim, model.c1, relu_mask=x, lda=ld,
                          ldb=model.input_dim)
            model._cnn_stem.backward(model.cnn, B, c.cnn, ws.dxin[:, :model.feat_dim], c.grads_p)
            self._average_over_ranks(c.grads_p)
        self._average_over_ranks(c.grads)
        self._enqueue_adam(ws, c.adam)
        if self.is_pixel_input:
            self._enqueue_adam(ws, c.adam_p)

    def _enqueue_iteration_layers(self, ws, x, xn, actions, rewards, done, pix=None, pix_next=None, update=True):
        """one DDPG iteration (ddpg.py:244-352) layer by layer, with every switch: camera observations (the perception CNN
        in front of both networks, trained by the critic loss, ddpg_net.py:37-88), the TD3 double critic and action
        regularisation (ddpg.py:119-147, 266-283, 312-319), several ranks -- and use_layernorm, which the model's passes
        (DDPGModel.actor_forward ... actor_backward) keep to themselves"""
        K, m, mt = self.K, self.model, self.model_target
        B = x.shape[0]
        c, c2 = ws.critics[0], ws.critics[1] if self.use_double_critic else None
        low, low_next = x, xn
        if self.is_pixel_input:
            # forward_perception (ddpg_net.py:67-78): [CNN(camera0 / 255) | low_dim]; the model's own
            # features are formed ONCE, before the critic update, and reused by the actor update
            # (ddpg.py:287, 326-327: perception.detach())
            mt.perception_into(pix_next, low_next, c.cnn_t, c.xnf)
            m.perception_into(pix, low, c.cnn, c.xf)
            x, xn = c.xf, c.xnf
        # ---- target: y = r + gamma^n * Q'(s', mu'(s')) * (1 - done) ----
        mt.actor_forward(xn, c.w_t, ws.act)
        mt.critic_forward(xn, ws.act, c.w_t, ws.q_next)
        q_next, gamma_n = ws.q_next, pow(self.discount_factor, self.n_step)
        if c2 is not None:
            # TD3 (ddpg.py:266-283): y = min(y1, y2), the second target critic evaluated at the target
            # policy's action -- with clipped noise added when action regularisation is on (the
            # reference adds it AFTER the first critic's target was formed, so only y2 sees it).
            # r + t is monotone in t: min(r + t1, r + t2) = r + gamma^n (1 - d) min(Q1', Q2')
            a2 = ws.act
            if self.use_action_regularization:
                torch.add(ws.act, ws.s_noise, out=ws.act_n)
                ws.act_n.clamp_(-1.0, 1.0)
                a2 = ws.act_n
            xn2 = xn
            if self.is_pixel_input:                  # the second target has its own perception
                c2.target.perception_into(pix_next, low_next, c2.cnn_t, c2.xnf)
                xn2 = c2.xnf
            c2.target.critic_forward(xn2, a2, c2.w_t, ws.q_next2)
            torch.minimum(ws.q_next, ws.q_next2, out=ws.q_next2)
            q_next = ws.q_next2
        # ---- critic update(s) ----
        m.critic_forward(x, actions, c.w, c.q)
        x2 = x
        if c2 is not None:
            if self.is_pixel_input:
                c2.model.perception_into(pix, low, c2.cnn, c2.xf)
                x2 = c2.xf
            c2.model.critic_forward(x2, actions, c2.w, c2.q)
        K.ddpg_critic_loss_step(c.q, q_next, rewards, done, gamma_n, c.y, c.dz3, ws.step)
        self._enqueue_critic_update(ws, c, x)
        ws.q_policy.copy_(c.q)
        if c2 is not None:                               # ddpg.py:312-319
            K.ddpg_critic_loss(c2.q, q_next, rewards, done, gamma_n, c2.y, c2.dz3)
            self._enqueue_critic_update(ws, c2, x2)
            # the reference reports the SECOND critic's loss as 'critic_loss' (it overwrites the
            # variable, ddpg.py:313) and adds Q_policy2
            K.ddpg_stats(c2.q, c2.y, rewards, actions, c2.q, c2.stats)
            self._average_over_ranks(c2.stats[:6])
        # ---- actor update through the UPDATED critic: loss = -mean Q(s, mu(s)) ----
        # (update False -- a critic-only iteration of a delayed policy update: the iteration ends with the statistics, on
        # Q(s, mu(s)) as the last actor update left it)
        if update:
            m.actor_forward(x, c.w, ws.act)
            m.critic_forward(x, ws.act, c.w, ws.q_actor)
            K.fill(c.dz3, -1.0 / B)
            m.actor_backward(x, c.w, ws.bw, c.dz3, ws.act, ws.ga, ws.grads_a)
            self._average_over_ranks(ws.grads_a)
            self._enqueue_actor_adam(ws)
        K.ddpg_stats(ws.q_policy, c.y, rewards, actions, ws.q_actor, c.stats)
        self._average_over_ranks(c.stats[:6])       # means over the global batch (max |a| stays local)
        if update:
            self._enqueue_target_update(ws)

    def _schedule(self, B, D):
        """which launch schedule an iteration on B rows of D inputs takes -- 'rows' (row blocks), 'levels' (dependency
        levels) or 'layers' (layer by layer: every switch).  Asked at each enqueue: level_schedule / row_schedule may be
        set after construction"""
        # (a delayed policy update takes the rows only where the kernels run its critic-only iterations)
        can_rows = self.policy_delay == 1 or KN.ddpg_rows_delay(self.K)
        if self.use_layernorm:
            # LayerNorm takes the rows only when asked to (ddpg_row_schedule = True) and where _rows_dims lets it:
            # low-dimensional observations, one rank, the fused update (one critic or two); otherwise layer by layer
            return 'rows' if self.row_schedule is True and can_rows and self._rows_dims(D, B) is not None else 'layers'
        if not self.is_pixel_input:
            if self.use_double_critic:
                # TD3 takes the rows only when asked to (ddpg_row_schedule = True), where the kernels run it and the
                # shapes fit; unset, it stays layer by layer as before -- and there are no levels for two critics
                return 'rows' if self.row_schedule is True and can_rows and self._rows_dims(D, B) is not None else 'layers'
            rows = self.row_schedule if self.row_schedule is not None else B <= 1024
            if rows and can_rows and self._rows_dims(D, B) is not None:
                return 'rows'
            if self.level_schedule and self.world_size == 1:
                return 'levels'
        return 'layers'

    def _enqueue_iteration(self, ws, x, xn, actions, rewards, done, pix=None, pix_next=None, update=True):
        """one DDPG iteration (ddpg.py:244-352) as a launch sequence without host round trips; update False: a critic-only
        iteration of a delayed policy update -- everything up to the critics' steps and the statistics"""
        schedule = self._schedule(*x.shape)
        if schedule == 'rows':
            return self._enqueue_iteration_rows(ws, x, xn, actions, rewards, done, update)
        if schedule == 'levels':
            return self._enqueue_iteration_levels(ws, x, xn, actions, rewards, done, update)
        return self._enqueue_iteration_layers(ws, x, xn, actions, rewards, done, pix, pix_next, update)

    def _optimize(self, obs, actions, rewards, obs_next, done):       # ddpg.py:244-352
        x = obs['low_dim']['flat_inputs']
        xn = obs_next['low_dim']['flat_inputs']
        B, D = x.shape
        ws = self._workspace(B, D)
        if ws.dev_step != self.critic_step:          # restored from a checkpoint
            ws.step.fill_(self.critic_step)
            self.invalidate_packed()
        if ws.astep is not None and ws.dev_astep != self.actor_step:
            ws.astep.fill_(self.actor_step)
        if ws.lr_host != (self.lr_actor, self.lr_critic):
            ws.lr_host = (self.lr_actor, self.lr_critic)
            ws.lr.copy_(torch.tensor(ws.lr_host, dtype=torch.float32))
        # (a batch sampled straight into staging_fields() is already where the captured iteration reads it)
        _stage(ws.s_obs, x)
        _stage(ws.s_next, xn)
        _stage(ws.s_act, actions.reshape(B, -1))
        _stage(ws.s_rew, rewards.reshape(-1))
        _stage(ws.s_done, done.reshape(-1))
        frames = ()
        if self.is_pixel_input:
            pix, pix_next = obs['pixel']['camera0'], obs_next['pixel']['camera0']
            if ws.s_pix is None or ws.s_pix.dtype != pix.dtype:
                self._alloc_frame_staging(ws, pix.shape, pix.dtype)
            _stage(ws.s_pix, pix)
            _stage(ws.s_pix_next, pix_next)
            frames = (ws.s_pix, ws.s_pix_next)
        if self.use_action_regularization:
            # ddpg.py:268-274: policy_noise 0.2 clipped at 0.5, from numpy's global stream
            noise = np.clip(np.random.normal(0, 0.2, size=(self.batch_size, self.action_dim)), -0.5, 0.5)
            ws.s_noise.copy_(torch.as_tensor(noise, dtype=torch.float32))
        # the iteration's kind, from its number alone (every rank agrees): with a delayed policy update a workspace holds
        # two captured graphs, the full iteration and the critic-only one, each captured after one eager iteration of its kind
        update = self._updates_actor(self.critic_step + 1)
        which = 'graph' if update else 'graph_critic'
        batch = (ws.s_obs, ws.s_next, ws.s_act, ws.s_rew, ws.s_done) + tuple(frames)
        if self.use_graph and getattr(ws, which) is None:
            # capture after one eager iteration (lazy allocations, module load); its effects are
            # real: the capture itself executes nothing
            self._enqueue_iteration(ws, *batch, update=update)
            gc.collect()
            gc.disable()               # a collection inside capture may free device memory: illegal
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._enqueue_iteration(ws, *batch, update=update)
                setattr(ws, which, g)
            finally:
                gc.enable()
        elif getattr(ws, which) is not None:
            self._rows_refresh(ws)
            getattr(ws, which).replay()
            if getattr(ws, 'rows_args', None) is not None:
                ws.rows_versions = self._rows_versions()
        else:
            self._enqueue_iteration(ws, *batch, update=update)
        self.critic_step += 1
        if update:
            self.actor_step += 1
        ws.dev_step, ws.dev_astep = self.critic_step, self.actor_step
        if self.target_update_type == 'hard':
            self.target_update_counter += 1
        return self._collect_stats(ws)

    def _alloc_frame_staging(self, ws, shape, dtype):
        """the staged camera frames of s and s' (again): the captured iteration read the old ones, so the graph goes"""
        ws.s_pix = torch.empty(tuple(shape), device=self.device, dtype=dtype)
        ws.s_pix_next = torch.empty(tuple(shape), device=self.device, dtype=dtype)
        ws.graph = ws.graph_critic = None

    def staging_fields(self, batch_size):
        """the buffers the captured iteration reads its batch from, by replay field name:
        ``replay.sample_batch(B, out=learner.staging_fields(B))`` gathers the sample where learn() would otherwise copy
        it (five small copies per iteration, 6 % of one at batch 512).  A camera learner also stages 'pixel' and
        'pixel_next', uint8 [B] + obs_spec camera0 (allocated here on first use, kept while their dtype holds)"""
        B = int(batch_size)
        ws = self._workspace(B, self.model.low_dim)      # (_optimize keys it by the low-dimensional width)
        fields = {'obs': ws.s_obs, 'obs_next': ws.s_next, 'actions': ws.s_act, 'rewards': ws.s_rew, 'dones': ws.s_done}
        if self.is_pixel_input:
            cam = (B,) + tuple(int(v) for v in self.env_config.obs_spec['pixel']['camera0'])
            if ws.s_pix is None or ws.s_pix.dtype != torch.uint8 or tuple(ws.s_pix.shape) != cam:
                self._alloc_frame_staging(ws, cam, torch.uint8)
            fields['pixel'], fields['pixel_next'] = ws.s_pix, ws.s_pix_next
        return fields

    def _collect_stats(self, ws):
        """the iteration's one read-back; asynchronous on a GPU (resolved when looked at, at the latest
        after the next iteration has been enqueued -- see learner/base.py DeferredStats)"""
        if not self.lazy_stats:
            return self._decode_stats(ws.stats.cpu(), ws.stats2.cpu() if self.use_double_critic else None)
        self._flush_stats()
        if getattr(ws, 'stats_host', None) is None:
            ws.stats_host = torch.empty(3, 8, pin_memory=True)
        if getattr(ws, 'stats_zero_copy', False):
            # the row schedule's last launch wrote the statistics into host-mapped memory itself (slot = the iteration's
            # Adam step & 1: the slot of the iteration before is still being read): no copy launch
            host0 = ws.stats_slots[self.critic_step & 1]
            host1 = host0[8:] if self.use_double_critic else None      # (the second block of the slot)
        else:
            ws.stats_host[0].copy_(ws.stats, non_blocking=True)
            host0 = ws.stats_host[0]
            host1 = ws.stats_host[1] if self.use_double_critic else None
        if ws.xerr is not None and self.world_size > 1:      # a peer exchange that timed out in this iteration
            ws.stats_host[2, :1].view(torch.int32).copy_(ws.xerr, non_blocking=True)
        else:
            ws.stats_host[2].zero_()
        if self.use_double_critic and not getattr(ws, 'stats_zero_copy', False):
            ws.stats_host[1].copy_(ws.stats2, non_blocking=True)
        # (two events in turn, recorded on a Stream object cached per raw handle: Event() + record() through
        # torch.cuda.current_stream() were 15 us of host time per iteration)
        raw = L.current_stream().value
        if getattr(ws, 'ev_raw', -1) != raw:
            ws.ev_raw, ws.ev_stream = raw, torch.cuda.current_stream()
            ws.ev_pair, ws.ev_turn = (torch.cuda.Event(), torch.cuda.Event()), 0
        ev = ws.ev_pair[ws.ev_turn]
        ws.ev_turn ^= 1
        ev.record(ws.ev_stream)
        handle = DeferredStats(self._flush_stats)
        self._pending_stats = (ev, ws.stats_host, handle, host0, host1)
        return handle

    def _flush_stats(self):
        pend, self._pending_stats = self._pending_stats, None
        if pend is not None:
            ev, host, handle, host0, host1 = pend
            ev.synchronize()
            if int(host[2, :1].view(torch.int32)[0]) != 0:
                raise RuntimeError('a peer exchange timed out in the last DDPG iteration: error word 0x%x (0x100 | phase << 4 '
                                   '| peer) -- a rank died or fell behind by more than the timeout'
                                   % (int(host[2, :1].view(torch.int32)[0]) & 0xffff))
            handle._value = self._decode_stats(host0, host1)

    def _decode_stats(self, st, st2):
        st = st.numpy()
        amax = float(st[6])
        assert amax <= 1.0, 'actions must lie in [-1, 1] (ddpg.py:262-263), got |a| = %g' % amax
        out = {'actor_loss': float(st[0]), 'critic_loss': float(st[1]), 'action_norm': float(st[2]),
               'rewards': float(st[3]), 'Q_target': float(st[4]), 'Q_policy': float(st[5])}
        if st2 is not None:
            st2 = st2.numpy()
            out['critic_loss'], out['Q_policy2'] = float(st2[1]), float(st2[5])
        return out

    def learn(self, batch):
        self.current_iteration += 1
        batch = self.preprocess(batch)
        stats = self._optimize(batch['obs'], batch['actions'], batch['rewards'], batch['obs_next'],
                               batch['dones'])
        self.tensorplex.add_scalars(stats, global_step=self.current_iteration)
        self.periodic_checkpoint(global_steps=self.current_iteration, score=None)
        return stats

    def module_dict(self):
        return {'ddpg': self.model}

    def checkpoint_attributes(self):
        return ['current_iteration', 'model', 'model_target']

    # ---- the whole training state (utils/run_state.py); the reference-format checkpoint above stays what it is ---------
    def invalidate_packed(self):
        """The row schedule's fragment-order weight copies (ws.rows_packed) follow the parameters through the update
        launches alone; a write from outside is noticed only through torch's write counters (_rows_versions).  A writer
        that does not move them -- raw pointers: a ctypes / hipMemcpy loader, a DLPack or numpy alias, a peer or IPC
        broadcast -- MUST call this after writing model, model_target (model2, model_target2): the next iteration then
        packs every network again.  load_train_state_dict and the checkpoint-restore path call it."""
        if self._ws is not None:
            self._ws.rows_versions = None

    def _train_tensors(self):
        """every device tensor that decides the next learn(), LIVE, by name: the models and targets (TD3: the second
        critic and its target) and every Adam moment group"""
        from surreal_amd.utils.run_state import model_tensors
        out = {}
        models = [('model', self.model), ('model_target', self.model_target)]
        moments = [('actor', (self.actor_exp_avg, self.actor_exp_avg_sq)),
                   ('critic', (self.critic_exp_avg, self.critic_exp_avg_sq)), ('perception', self.perception_moments)]
        if self.use_double_critic:
            models += [('model2', self.model2), ('model_target2', self.model_target2)]
            moments += [('critic2', self.critic2_moments), ('perception2', self.perception2_moments)]
        for name, m in models:
            for k, v in model_tensors(m).items():
                out['%s.%s' % (name, k)] = v
        for name, pair in moments:
            if pair is not None and pair[0] is not None:
                out['%s.exp_avg' % name], out['%s.exp_avg_sq' % name] = pair
        return out

    _TRAIN_WORDS = ('current_iteration', 'current_iter', 'actor_step', 'critic_step', 'lr_actor', 'lr_critic')

    def _train_state_refusal(self, who):
        if self.world_size > 1:
            raise NotImplementedError('%s: %d ranks; one rank only' % (who, self.world_size))

    def train_state_dict(self):
        """Everything that decides the bytes of the next learn(), as LIVE tensors (run_state.to_host / save_run make
        the host copy): the models and their targets, TD3's second critic and its target, every Adam moment group (the
        second critic's and the perception CNNs' included), actor_step / critic_step (the device step word ws.step is
        derived from critic_step), the learning rates, current_iteration, the hard update's counter, the publish
        counter, and the key of the workspace.  Not carried: the numpy global stream TD3's action regularisation draws
        from, the scalar history.  Several ranks: NotImplementedError."""
        self._train_state_refusal('DDPGLearner.train_state_dict')
        words = {k: getattr(self, k) for k in self._TRAIN_WORDS}
        words['publish_seq'] = int(getattr(self, '_publish_seq', 0))
        if self.target_update_type == 'hard':
            words['target_update_counter'] = int(self.target_update_counter)
        if self.policy_delay > 1:        # (a state without the key is of a learner that updates its policy every iteration)
            words['policy_delay'] = int(self.policy_delay)
        return {'kind': 'DDPGLearner', 'tensors': self._train_tensors(), 'words': words,
                'workspace': None if self._ws is None else list(self._ws.key)}

    def load_train_state_dict(self, sd):
        """train_state_dict()'s, back, IN PLACE (copy_ into the existing tensors: a captured hipGraph stays valid; a
        workspace that does not exist yet is built first).  Afterwards the device step word equals critic_step -- the
        statistics slot parity (critic_step & 1) agrees with it, both come from the one value --, the learning-rate
        words are the saved ones and the packed row weights are invalidated.  ValueError before anything is written when
        a tensor's name, shape or dtype differs; several ranks: NotImplementedError."""
        from surreal_amd.utils.run_state import check_tensors, load_tensors
        who = 'DDPGLearner.load_train_state_dict'
        self._train_state_refusal(who)
        if sd.get('kind') != 'DDPGLearner':
            raise ValueError('%s: the state is of a %s' % (who, sd.get('kind')))
        live = self._train_tensors()
        check_tensors(who, sd['tensors'], live)
        words = sd['words']
        if ('target_update_counter' in words) != (self.target_update_type == 'hard'):
            raise ValueError('%s: the state is of a %s target update, this learner\'s is %s'
                             % (who, 'hard' if 'target_update_counter' in words else 'soft', self.target_update_type))
        if int(words.get('policy_delay', 1)) != self.policy_delay:
            raise ValueError('%s: the state is of policy_delay = %d, this learner\'s is %d'
                             % (who, int(words.get('policy_delay', 1)), self.policy_delay))
        self._flush_stats()                         # (a read-back in flight belongs to the state that goes)
        load_tensors(sd['tensors'], live)
        for k in self._TRAIN_WORDS:
            setattr(self, k, type(getattr(self, k))(words[k]))
        self._publish_seq = int(words['publish_seq'])
        if self.target_update_type == 'hard':
            self.target_update_counter = int(words['target_update_counter'])
        if self._ws is None and sd.get('workspace') is not None:
            self._workspace(*(int(v) for v in sd['workspace']))
        ws = self._ws
        if ws is not None:
            ws.step.fill_(self.critic_step)
            ws.dev_step = self.critic_step
            if ws.astep is not None:         # the actor's own Adam step word of a delayed policy update
                ws.astep.fill_(self.actor_step)
            ws.dev_astep = self.actor_step
            ws.lr_host = (self.lr_actor, self.lr_critic)
            ws.lr.copy_(torch.tensor(ws.lr_host, dtype=torch.float32))
        self.invalidate_packed()

    def _prefetcher_preprocess(self, batch):
        if not self.frame_stack_concatenate_on_env:        # ddpg.py:430-440
            batch = self.frame_stack_preprocess.preprocess_list(batch)
        return self.aggregator.aggregate(batch)
