"""
DDPGModel on MI355X (surreal/model/ddpg_net.py:13-95; ActorNetworkX / CriticNetworkX,
model_builders/builders.py:35-84).  use_layernorm=True (reference default: off, ddpg_configs.py:21) puts a LayerNorm over
the features behind every hidden ReLU (builders.py:42-48, 65-75; torchx's L.LayerNorm(1) taken as torch.nn.LayerNorm(F) -- its
source is not in the reference tree) -- low-dimensional observations only.  With camera frames in the observation the "perception" CNN
(CNNStemNetwork, builders.py:8-33; ddpg_net.py:37-44, 67-78) runs on ``camera0 / 255`` and its
features are concatenated IN FRONT of the low-dim vector; it trains with the critic
(ddpg_net.py:57-61).

  actor : Linear(D,h1)-ReLU[-LN]-Linear(h1,h2)-ReLU[-LN]-Linear(h2,A)-Tanh
  critic: Linear(D,c1)-ReLU[-LN] ; concat action ; Linear(c1+A,c2)-ReLU[-LN] ; Linear(c2,1)

One flat fp32 parameter buffer per network (actor / critic / perception).
"""
import collections
import types

import numpy as np
import torch

from surreal_amd import kernels as KN
from surreal_amd.model.cnn_stem import CnnParams, CnnStem
from surreal_amd.model.ppo_net import Mlp3Params


class DDPGModel(object):
    def __init__(self, obs_spec, action_dim, use_layernorm, actor_fc_hidden_sizes,
                 critic_fc_hidden_sizes, conv_out_channels=None, conv_kernel_sizes=None,
                 conv_strides=None, conv_hidden_dim=None, critic_only=False, device=None,
                 kernels=None):
        self.K = kernels or KN.default_kernels()
        device = device or KN.default_device()
        self._ctor = dict(obs_spec=obs_spec, action_dim=action_dim, use_layernorm=use_layernorm,
                          actor_fc_hidden_sizes=list(actor_fc_hidden_sizes),
                          critic_fc_hidden_sizes=list(critic_fc_hidden_sizes),
                          conv_out_channels=conv_out_channels, conv_kernel_sizes=conv_kernel_sizes,
                          conv_strides=conv_strides, conv_hidden_dim=conv_hidden_dim,
                          critic_only=critic_only, device=device, kernels=self.K)
        self.is_pixel_input = 'pixel' in obs_spec
        self.action_dim = A = action_dim
        self.use_layernorm = use_layernorm
        self.low_dim = int(obs_spec['low_dim']['flat_inputs'][0]) if 'low_dim' in obs_spec else 0
        self.cnn = self.perception_flat = self._cnn_stem = None
        self.feat_dim = 0
        if self.is_pixel_input:
            if len(obs_spec['pixel']) != 1 or 'camera0' not in obs_spec['pixel']:
                raise NotImplementedError('one camera (camera0), as ddpg_net.py:34-35')
            cam = tuple(int(v) for v in obs_spec['pixel']['camera0'])
            self.feat_dim = int(conv_hidden_dim)
            geo = dict(conv_channels=tuple(conv_out_channels or (16, 32)),
                       kernel_sizes=tuple(conv_kernel_sizes or (8, 4)), strides=tuple(conv_strides or (4, 2)))
            self.perception_flat = torch.empty(CnnParams.count(cam, self.feat_dim, **geo), device=device)
            self.cnn = CnnParams(self.perception_flat, 0, cam, self.feat_dim, **geo)
            self._cnn_stem = CnnStem(self.K)
        self.input_dim = D = self.feat_dim + self.low_dim          # ddpg_net.py:36-46
        self.device = device
        ah, ch = list(actor_fc_hidden_sizes), list(critic_fc_hidden_sizes)
        self.c1, self.c2 = ch
        c1, c2 = ch
        sizes = [('W1', (c1, D)), ('b1', (c1,)), ('W2', (c2, c1 + A)), ('b2', (c2,)),
                 ('W3', (1, c2)), ('b3', (1,))]
        if use_layernorm:            # the affine parameters of the two LayerNorms, behind the dense ones
            sizes += [('ln1.W', (c1,)), ('ln1.b', (c1,)), ('ln2.W', (c2,)), ('ln2.b', (c2,))]
        n = sum(int(np.prod(s)) for _, s in sizes)
        self.ln_eps = 1e-5           # torch.nn.LayerNorm's default
        if use_layernorm and max(list(actor_fc_hidden_sizes) + list(critic_fc_hidden_sizes)) > 1024:
            raise NotImplementedError('use_layernorm: hidden sizes up to 1024 (smx_layernorm_*_f32 keep a row in one workgroup)')
        self.actor_flat = self.ac_flat = None
        if not critic_only:
            # actor and critic parameters live in ONE buffer (each on a 256-byte boundary, the gap zero): the target
            # network's soft / hard update is then one launch over `ac_flat` instead of one per network
            n_mlp = Mlp3Params.count(D, ah[0], ah[1], A)
            na = n_mlp + (2 * (ah[0] + ah[1]) if use_layernorm else 0)
            na_pad = (na + 63) // 64 * 64
            self.ac_flat = torch.zeros(na_pad + n, device=device)
            self.actor_flat = self.ac_flat[:na]
            self.actor = Mlp3Params(self.actor_flat, 0, D, ah[0], ah[1], A)
            self.actor_ln = collections.OrderedDict()
            self.actor_ln_flat = self.actor_flat[n_mlp:]      # ln1.W | ln1.b | ln2.W | ln2.b (empty without LayerNorm)
            if use_layernorm:
                o = n_mlp
                for name, k in (('ln1.W', ah[0]), ('ln1.b', ah[0]), ('ln2.W', ah[1]), ('ln2.b', ah[1])):
                    self.actor_ln[name] = self.actor_flat[o:o + k]
                    o += k
            self.critic_flat = self.ac_flat[na_pad:na_pad + n]
        else:
            self.actor = None
            self.critic_flat = torch.empty(n, device=device)
        self.critic = collections.OrderedDict()
        o = 0
        for name, shp in sizes:
            k = int(np.prod(shp))
            self.critic[name] = self.critic_flat[o:o + k].view(*shp)
            o += k
        self._init()

    def _init(self):
        if self.cnn is not None:
            self.perception_flat.zero_()
            self.cnn.init_torch_default()
        nets = [self.critic] + ([self.actor.views] if self.actor is not None else [])
        for views in nets:
            for name, v in views.items():
                if name.startswith('ln'):
                    continue
                fan = views['W' + name[1]].shape[1]
                v.uniform_(-1.0 / np.sqrt(fan), 1.0 / np.sqrt(fan))
        if self.use_layernorm:           # torch.nn.LayerNorm: weight 1, bias 0
            for views in [self.critic] + ([self.actor_ln] if self.actor is not None else []):
                for name, v in views.items():
                    if name.startswith('ln'):
                        v.fill_(1.0 if name.endswith('.W') else 0.0)

    def named_parameters(self):
        out = collections.OrderedDict()
        if self.actor is not None:
            for i in (1, 2, 3):
                out['actor.fc%d.W' % i] = self.actor.views['W%d' % i]
                out['actor.fc%d.b' % i] = self.actor.views['b%d' % i]
        for i in (1, 2, 3):
            out['critic.fc%d.W' % i] = self.critic['W%d' % i]
            out['critic.fc%d.b' % i] = self.critic['b%d' % i]
        if self.use_layernorm:
            if self.actor is not None:
                for k, v in self.actor_ln.items():
                    out['actor.' + k] = v
            for k in ('ln1.W', 'ln1.b', 'ln2.W', 'ln2.b'):
                out['critic.' + k] = self.critic[k]
        if self.cnn is not None:
            for k, v in self.cnn.views.items():
                out['cnn.' + k] = v
        return out

    def load_params(self, params):
        with torch.no_grad():
            for k, v in self.named_parameters().items():
                v.copy_(torch.as_tensor(np.asarray(params[k]), dtype=torch.float32).view(v.shape))

    def numpy_params(self):
        return collections.OrderedDict((k, v.detach().cpu().numpy().copy())
                                       for k, v in self.named_parameters().items())

    def state_dict(self):
        return collections.OrderedDict(self.named_parameters())

    def load_state_dict(self, sd):
        with torch.no_grad():
            for k, v in self.named_parameters().items():
                src = sd[k]
                if not torch.is_tensor(src):
                    src = torch.as_tensor(np.asarray(src), dtype=torch.float32)
                v.copy_(src.view(v.shape))

    def get_actor_parameters(self):
        return [self.actor_flat]

    def get_critic_parameters(self):
        return [self.critic_flat] + ([self.perception_flat] if self.cnn is not None else [])

    # ---- forward passes (eager helpers; the learner uses its own workspace) -----------------
    def perception_into(self, frames, low, cnn_ws, out):
        """out [rows, feat + low_dim] = [CNN(frames / 255) | low]; cnn_ws keeps the activations (a
        backward pass may follow)"""
        rows = out.shape[0]
        self._cnn_stem.forward(self.cnn, frames, rows, cnn_ws, out[:, :self.feat_dim])
        if self.low_dim:
            out[:, self.feat_dim:].copy_(low)

    def forward_perception(self, obs):
        if not self.is_pixel_input:
            return obs['low_dim']['flat_inputs']
        frames = obs['pixel']['camera0'].contiguous()
        rows = frames.shape[0]
        out = torch.empty(rows, self.input_dim, device=frames.device)
        cws = CnnStem.workspace(self.cnn, rows, frames.device, backward=False)
        self.perception_into(frames, obs['low_dim']['flat_inputs'] if self.low_dim else None, cws, out)
        return out

    # ---- actor / critic passes in a workspace: ONE calling shape, the plain and the LayerNorm variant behind it ----
    def _workspace_cached(self, rows, device):
        """the per-step act path (forward_actor / forward_critic): one workspace per (rows, device), not an allocation
        per buffer and call"""
        key = (int(rows), str(device))
        cache = self.__dict__.setdefault('_ws_cache', {})
        if key not in cache:
            if len(cache) > 8:
                cache.clear()
            cache[key] = self.workspace(rows, device)
        return cache[key]

    def workspace(self, rows, device=None):
        """what one actor and one critic pass keep for a backward pass: the hidden activations h1a / h2a and xcat =
        [layer 1 | action] / h2c -- with LayerNorm the activations in front of each LayerNorm, its outputs and the row
        means / reciprocal standard deviations instead"""
        f = lambda *s: torch.empty(*s, device=device or self.device)  # noqa: E731
        w = types.SimpleNamespace(xcat=f(rows, self.c1 + self.action_dim))
        a = self.actor
        if not self.use_layernorm:
            if a is not None:
                w.h1a, w.h2a = f(rows, a.H1), f(rows, a.H2)
            w.h2c = f(rows, self.c2)
            return w
        if a is not None:
            w.a1, w.n1, w.a2, w.n2 = f(rows, a.H1), f(rows, a.H1), f(rows, a.H2), f(rows, a.H2)
            w.am1, w.ar1, w.am2, w.ar2 = f(rows), f(rows), f(rows), f(rows)
        w.c_a1, w.c_a2, w.c_n2 = f(rows, self.c1), f(rows, self.c2), f(rows, self.c2)
        w.cm1, w.cr1, w.cm2, w.cr2 = f(rows), f(rows), f(rows), f(rows)
        return w

    def target_workspace(self, w, rows, device=None):
        """where a target copy of the network whose passes run in `w` runs: the plain variant's target passes go through
        `w` itself, ahead of the network's own; the LayerNorm variant keeps them apart"""
        return self.workspace(rows, device) if self.use_layernorm else w

    def backward_workspace(self, rows, device=None):
        """scratch of critic_backward / actor_backward (one at a time: every critic of a learner shares it)"""
        f = lambda *s: torch.empty(*s, device=device or self.device)  # noqa: E731
        a, A, c1, c2 = self.actor, self.action_dim, self.c1, self.c2
        s = types.SimpleNamespace(dz2=f(rows, c2), dxcat=f(rows, c1 + A), dz3a=f(rows, A), dz2a=f(rows, a.H2),
                                  dz1a=f(rows, a.H1))
        if self.use_layernorm:
            s.dn2, s.dz1c, s.dn2a, s.dn1a = f(rows, c2), f(rows, c1), f(rows, a.H2), f(rows, a.H1)
            s.ln_ws = f(max(self.K.layernorm_backward_ws_floats(rows, k) for k in (c1, c2, a.H1, a.H2)))
            s.ln_scr = f(2 * max(c1, c2))
        return s

    def actor_forward(self, x, w, out):
        """out = tanh(fc3(relu(fc2(relu(fc1 x))))), a LayerNorm behind each ReLU with use_layernorm (builders.py:35-56)"""
        K, a = self.K, self.actor
        if not self.use_layernorm:
            return K.mlp3_forward(a, x, w.h1a, w.h2a, out, 2)
        v, ln = a.views, self.actor_ln
        rows, D = x.shape
        K.linear(x, 1, v['W1'], 1, v['b1'], w.a1, rows, a.H1, D, act=1)
        K.layernorm_forward(w.a1, ln['ln1.W'], ln['ln1.b'], self.ln_eps, w.n1, w.am1, w.ar1)
        K.linear(w.n1, 1, v['W2'], 1, v['b2'], w.a2, rows, a.H2, a.H1, act=1)
        K.layernorm_forward(w.a2, ln['ln2.W'], ln['ln2.b'], self.ln_eps, w.n2, w.am2, w.ar2)
        K.linear(w.n2, 1, v['W3'], 1, v['b3'], out, rows, a.OUT, a.H2, act=2)

    def critic_forward(self, x, action, w, q):
        """q [rows] = Q(x, action); w.xcat [rows, c1 + A] receives (LN of) relu(fc1 x) | action   (builders.py:58-84)"""
        K, c = self.K, self.critic
        rows, D = x.shape
        A, c1, c2 = self.action_dim, self.c1, self.c2
        xcat = w.xcat
        if not self.use_layernorm:
            K.linear(x, 1, c['W1'], 1, c['b1'], xcat, rows, c1, D, act=1, ldc=c1 + A)
            xcat[:, c1:].copy_(action)
            K.linear(xcat, 1, c['W2'], 1, c['b2'], w.h2c, rows, c2, c1 + A, act=1)
            K.linear(w.h2c, 1, c['W3'], 1, c['b3'], q.view(rows, 1), rows, 1, c2, act=0)
            return
        K.linear(x, 1, c['W1'], 1, c['b1'], w.c_a1, rows, c1, D, act=1)
        K.layernorm_forward(w.c_a1, c['ln1.W'], c['ln1.b'], self.ln_eps, xcat[:, :c1], w.cm1, w.cr1)
        xcat[:, c1:].copy_(action)
        K.linear(xcat, 1, c['W2'], 1, c['b2'], w.c_a2, rows, c2, c1 + A, act=1)
        K.layernorm_forward(w.c_a2, c['ln2.W'], c['ln2.b'], self.ln_eps, w.c_n2, w.cm2, w.cr2)
        K.linear(w.c_n2, 1, c['W3'], 1, c['b3'], q.view(rows, 1), rows, 1, c2, act=0)

    def critic_backward(self, x, w, s, dq, g):
        """gradients g (views by parameter name) of the critic's parameters from dq = dLoss/dQ [rows], behind
        critic_forward(x, ., w, .); dLoss/d(action) is left in the last A columns of s.dxcat.
        -> (dLoss/d(layer 1's output in front of its ReLU), its leading dimension): the perception CNN's way in"""
        K, c = self.K, self.critic
        rows, D = x.shape
        A, c1, c2 = self.action_dim, self.c1, self.c2
        ld = c1 + A
        dq = dq.view(rows, 1)
        if not self.use_layernorm:
            K.linear(dq, 1, c['W3'], 0, None, s.dz2, rows, c2, 1, relu_mask=w.h2c, lda=1, ldb=c2)
            # d/d(relu(layer1)) masked by relu', into the first c1 columns of dxcat
            K.linear(s.dz2, 1, c['W2'], 0, None, s.dxcat, rows, c1, c2, relu_mask=w.xcat, ldb=ld, ldc=ld)
            # d/d(action) into the last A columns (no mask)
            K.linear(s.dz2, 1, c['W2'][:, c1:], 0, None, s.dxcat[:, c1:], rows, A, c2, ldb=ld, ldc=ld)
            K.linear_wgrad(s.dxcat, x, g['W1'], g['b1'], c1, D, rows, ldz=ld)
            K.linear_wgrad(s.dz2, w.xcat, g['W2'], g['b2'], c2, ld, rows)
            K.linear_wgrad(dq, w.h2c, g['W3'], g['b3'], 1, c2, rows, ldz=1)
            return s.dxcat, ld
        K.linear_wgrad(dq, w.c_n2, g['W3'], g['b3'], 1, c2, rows, ldz=1)
        K.linear(dq, 1, c['W3'], 0, None, s.dn2, rows, c2, 1, lda=1, ldb=c2)                 # d/d(LN2 output)
        K.layernorm_backward(s.dn2, w.c_a2, w.cm2, w.cr2, c['ln2.W'], s.dz2, g['ln2.W'], g['ln2.b'], s.ln_ws, relu_mask=True)
        K.linear_wgrad(s.dz2, w.xcat, g['W2'], g['b2'], c2, ld, rows)
        K.linear(s.dz2, 1, c['W2'], 0, None, s.dxcat, rows, ld, c2, ldb=ld, ldc=ld)        # d/d([LN1 output | action])
        K.layernorm_backward(s.dxcat[:, :c1], w.c_a1, w.cm1, w.cr1, c['ln1.W'], s.dz1c, g['ln1.W'], g['ln1.b'], s.ln_ws,
                             relu_mask=True)
        K.linear_wgrad(s.dz1c, x, g['W1'], g['b1'], c1, D, rows)
        return s.dz1c, c1

    def actor_backward(self, x, w, s, dq, act, g, g_flat):
        """gradients of the actor's parameters (g_flat, g its views by name) from dq = dLoss/dQ(x, act) [rows], behind
        actor_forward(x, w, act) and critic_forward(x, act, w, .); the critic's own gradients are not formed"""
        K, a, c = self.K, self.actor, self.critic
        rows, D = x.shape
        A, c1, c2 = self.action_dim, self.c1, self.c2
        ld = c1 + A
        dq = dq.view(rows, 1)
        if not self.use_layernorm:
            K.linear(dq, 1, c['W3'], 0, None, s.dz2, rows, c2, 1, relu_mask=w.h2c, lda=1, ldb=c2)
        else:
            K.linear(dq, 1, c['W3'], 0, None, s.dn2, rows, c2, 1, lda=1, ldb=c2)
            K.layernorm_backward(s.dn2, w.c_a2, w.cm2, w.cr2, c['ln2.W'], s.dz2, s.ln_scr[:c2], s.ln_scr[c2:2 * c2], s.ln_ws,
                                 relu_mask=True)
        K.linear(s.dz2, 1, c['W2'][:, c1:], 0, None, s.dxcat[:, c1:], rows, A, c2, ldb=ld, ldc=ld)   # d/d(action)
        s.dz3a.copy_(s.dxcat[:, c1:])        # dense [rows, A]
        K.tanh_backward(s.dz3a, act, s.dz3a)
        if not self.use_layernorm:
            return K.mlp3_backward(a, x, w.h1a, w.h2a, s.dz3a, s.dz2a, s.dz1a, g_flat, None)
        v, ln = a.views, self.actor_ln
        K.linear_wgrad(s.dz3a, w.n2, g['W3'], g['b3'], A, a.H2, rows)
        K.linear(s.dz3a, 1, v['W3'], 0, None, s.dn2a, rows, a.H2, A, ldb=a.H2)
        K.layernorm_backward(s.dn2a, w.a2, w.am2, w.ar2, ln['ln2.W'], s.dz2a, g['ln2.W'], g['ln2.b'], s.ln_ws, relu_mask=True)
        K.linear_wgrad(s.dz2a, w.n1, g['W2'], g['b2'], a.H2, a.H1, rows)
        K.linear(s.dz2a, 1, v['W2'], 0, None, s.dn1a, rows, a.H1, a.H2, ldb=a.H1)
        K.layernorm_backward(s.dn1a, w.a1, w.am1, w.ar1, ln['ln1.W'], s.dz1a, g['ln1.W'], g['ln1.b'], s.ln_ws, relu_mask=True)
        K.linear_wgrad(s.dz1a, x, g['W1'], g['b1'], a.H1, D, rows)

    def forward_actor(self, x):
        rows = x.shape[0]
        out = torch.empty(rows, self.actor.OUT, device=x.device)
        self.actor_forward(x.contiguous(), self._workspace_cached(rows, x.device), out)
        return out

    def forward_critic(self, x, action):
        rows = x.shape[0]
        q = torch.empty(rows, device=x.device)
        self.critic_forward(x.contiguous(), action, self._workspace_cached(rows, x.device), q)
        return q.view(rows, 1)

    def __deepcopy__(self, memo):
        """same architecture, own parameter buffers holding the same values (the kernel facade and
        the device are shared, not copied)"""
        twin = DDPGModel(**self._ctor)
        twin.load_state_dict(self.state_dict())
        return twin

    def __call__(self, obs_in, calculate_value=True, action=None):
        return self.forward(obs_in, calculate_value=calculate_value, action=action)

    def forward(self, obs_in, calculate_value=True, action=None):
        x = self.forward_perception(obs_in)
        if action is None:
            action = self.forward_actor(x)
        value = self.forward_critic(x, action) if calculate_value else None
        return action, value
