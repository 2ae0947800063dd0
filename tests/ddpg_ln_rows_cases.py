"""The torch-CPU double of the row schedule's LayerNorm launches (smx_ddpg_rows_critic_f32 / _actor_f32 /
_wgrad_update_f32 with args->ln), on top of the stock double: like it, every launch works from row-major SNAPSHOTS of the
dense parameters that only a pack or an update launch refreshes; the LayerNorms' gains and biases are read from the
parameter buffers themselves, as the kernels read them (they have no packed copy).  Top-level kernel calls are recorded in
`calls`.  Also the shapes that the GPU tier's sweep and the predicate's test share."""
import functools

import torch

from cpu_kernels import TorchCpuKernels

# (D, A, (H1, H2), (c1, c2), rows): F = 1024 is LayerNorm's upper bound, 4 its lower; 515 and 130 leave ragged last blocks,
# 1030 takes several rounds of workgroups
SWEEP = [(1, 1, (4, 4), (4, 4), 5),
         (50, 32, (1024, 64), (64, 1024), 130),
         (17, 6, (304, 204), (404, 300), 515),
         (17, 6, (300, 200), (400, 300), 37),
         (17, 6, (300, 200), (400, 300), 1030)]


def ln_fwd(x, g, b, eps):
    """-> (LayerNorm(x), mean [rows], rstd [rows]): torch.nn.LayerNorm's biased variance, eps inside the root"""
    m = x.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - m) ** 2).mean(1, keepdim=True) + eps)
    return (x - m) * rs * g + b, m.view(-1), rs.view(-1)


def ln_bwd(dn, pre, m, rs, g):
    """the gradient at the input of the ReLU in front of the LayerNorm (smx_layernorm_backward_f32 with relu_mask)"""
    xh = (pre - m.view(-1, 1)) * rs.view(-1, 1)
    gg = dn * g
    v = rs.view(-1, 1) * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    return v * (pre > 0)


class LnRowsCpuKernels(TorchCpuKernels):
    ddpg_rows_ln = True
    RECORDED = ('linear', 'linear_multi', 'linear_wgrad', 'mlp3_forward', 'mlp3_backward', 'adam_step_dev', 'soft_update',
                'hard_update_every', 'ddpg_critic_loss', 'ddpg_critic_loss_step', 'ddpg_stats', 'tanh_backward', 'fill',
                'layernorm_forward', 'layernorm_backward', 'ddpg_rows_pack', 'ddpg_rows_critic', 'ddpg_rows_actor',
                'ddpg_rows_update')

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls, self._depth = [], 0
        for name in self.RECORDED:
            if hasattr(self, name):
                setattr(self, name, self._recording(name, getattr(self, name)))

    def _recording(self, name, fn):
        @functools.wraps(fn)
        def wrapped(*a, **kw):
            if self._depth == 0:
                tag = name
                if name == 'ddpg_rows_update':
                    tag = '%s:%s%s' % (name, a[1], ':wgrad' if kw.get('wgrad') else '')
                self.calls.append(tag)
            self._depth += 1
            try:
                return fn(*a, **kw)
            finally:
                self._depth -= 1
        return wrapped

    # ---- the LayerNorm variant ----------------------------------------------------------------------------------
    def ddpg_rows_ln_supported(self, D, A, H1, H2, c1, c2, rows):
        widest = max(c1 + A, H1, H2, c2, D)
        return (self.ddpg_rows_supported(D, A, H1, H2, c1, c2, rows=rows) and 0 < rows < 2 ** 24
                and max(H1, H2, c1, c2) <= 1024 and rows * widest * 4 < 2 ** 31)

    def ddpg_rows_ln_attach(self, args, ln_nets, eps, io_ln):
        args.ln_nets, args.eps, args.io_ln = ln_nets, float(eps), io_ln
        return args

    @staticmethod
    def _ln_actor_fwd(n, ln, eps, x):
        a1 = torch.relu(x @ n['W1'].t() + n['b1'])
        n1, m1, r1 = ln_fwd(a1, ln['ln1.W'], ln['ln1.b'], eps)
        a2 = torch.relu(n1 @ n['W2'].t() + n['b2'])
        n2, m2, r2 = ln_fwd(a2, ln['ln2.W'], ln['ln2.b'], eps)
        return dict(a1=a1, n1=n1, am1=m1, ar1=r1, a2=a2, n2=n2, am2=m2, ar2=r2, act=torch.tanh(n2 @ n['W3'].t() + n['b3']))

    @staticmethod
    def _ln_critic_fwd(n, ln, eps, x, a):
        c_a1 = torch.relu(x @ n['W1'].t() + n['b1'])
        n1, m1, r1 = ln_fwd(c_a1, ln['ln1.W'], ln['ln1.b'], eps)
        xcat = torch.cat([n1, a], 1)
        c_a2 = torch.relu(xcat @ n['W2'].t() + n['b2'])
        n2, m2, r2 = ln_fwd(c_a2, ln['ln2.W'], ln['ln2.b'], eps)
        return dict(c_a1=c_a1, xcat=xcat, cm1=m1, cr1=r1, c_a2=c_a2, c_n2=n2, cm2=m2, cr2=r2,
                    q=(n2 @ n['W3'].t() + n['b3']).view(-1))

    def ddpg_rows_critic(self, args):
        if getattr(args, 'ln_nets', None) is None:
            return super().ddpg_rows_critic(args)
        io, il, S, LN, eps = args.io, args.io_ln, args.snap, args.ln_nets, args.eps
        D, A, H1, H2, c1, c2 = args.dims
        x, xn = io['x'], io['x_next']
        B = x.shape[0]
        a_next = self._ln_actor_fwd(S['target_actor'], LN['target_actor'], eps, xn)['act']
        q_next = self._ln_critic_fwd(S['target_critic'], LN['target_critic'], eps, xn, a_next)['q']
        c = self._ln_critic_fwd(S['critic'], LN['critic'], eps, x, io['actions'])
        y = io['rewards'].view(-1) + (args.gamma_n * q_next) * (1.0 - io['dones'].view(-1))
        dz3 = 2.0 * (c['q'] - y) / B
        io['xcat'].copy_(c['xcat']); io['h2c'].copy_(c['c_n2']); io['q'].copy_(c['q']); io['q_next'].copy_(q_next)
        io['y'].copy_(y); io['dz3'].copy_(dz3)
        for k in ('c_a1', 'cm1', 'cr1', 'c_a2', 'cm2', 'cr2'):
            il[k].copy_(c[k])
        if io.get('step') is not None:
            io['step'] += 1
        W2, W3 = S['critic']['W2'], S['critic']['W3']
        dn2 = dz3.view(B, 1) * W3.view(1, c2)
        dz2 = ln_bwd(dn2, c['c_a2'], c['cm2'], c['cr2'], LN['critic']['ln2.W'])
        dn1 = dz2 @ W2[:, :c1]
        il['dn2'].copy_(dn2); io['dz2'].copy_(dz2); io['dxcat'][:, :c1].copy_(dn1)
        il['dz1c'].copy_(ln_bwd(dn1, c['c_a1'], c['cm1'], c['cr1'], LN['critic']['ln1.W']))
        a = self._ln_actor_fwd(S['actor'], LN['actor'], eps, x)
        io['h1a'].copy_(a['n1']); io['h2a'].copy_(a['n2']); io['act'].copy_(a['act'])
        for k in ('a1', 'am1', 'ar1', 'a2', 'am2', 'ar2'):
            il[k].copy_(a[k])

    def ddpg_rows_actor(self, args):
        if getattr(args, 'ln_nets', None) is None:
            return super().ddpg_rows_actor(args)
        io, il, S, LN, eps = args.io, args.io_ln, args.snap, args.ln_nets, args.eps
        D, A, H1, H2, c1, c2 = args.dims
        x = io['x']
        B = x.shape[0]
        c = self._ln_critic_fwd(S['critic'], LN['critic'], eps, x, io['act'])
        io['q_actor'].copy_(c['q'])
        W2, W3 = S['critic']['W2'], S['critic']['W3']
        dn2 = torch.full((B, 1), -1.0 / B) * W3.view(1, c2)
        dz2 = ln_bwd(dn2, c['c_a2'], c['cm2'], c['cr2'], LN['critic']['ln2.W'])      # (back through LayerNorm 2 only)
        dz3a = (dz2 @ W2[:, c1:]) * (1.0 - io['act'] * io['act'])
        io['dz3a'].copy_(dz3a)
        dn2a = dz3a @ S['actor']['W3']
        dz2a = ln_bwd(dn2a, il['a2'], il['am2'], il['ar2'], LN['actor']['ln2.W'])
        dn1a = dz2a @ S['actor']['W2']
        il['dn2a'].copy_(dn2a); io['dz2a'].copy_(dz2a); il['dn1a'].copy_(dn1a)
        io['dz1a'].copy_(ln_bwd(dn1a, il['a1'], il['am1'], il['ar1'], LN['actor']['ln1.W']))

    def ddpg_rows_update(self, args, group, theta, grads, exp_avg, exp_avg_sq, lr, step, weight_decay, clip_value,
                         target=None, tau=0.0, interval=0, wgrad=False, stats=None, stats_host=None):
        if getattr(args, 'ln_nets', None) is None:
            return super().ddpg_rows_update(args, group, theta, grads, exp_avg, exp_avg_sq, lr, step, weight_decay,
                                            clip_value, target=target, tau=tau, interval=interval, wgrad=wgrad, stats=stats,
                                            stats_host=stats_host)
        assert wgrad and group in ('actor', 'critic'), 'the LayerNorm path steps with its gradients only'
        io, il = args.io, args.io_ln
        D, A, H1, H2, c1, c2 = args.dims
        x = io['x']
        if group == 'critic':
            pairs = [(il['dz1c'], x), (io['dz2'], io['xcat']), (io['dz3'].view(-1, 1), io['h2c'])]
            lns = [(io['dxcat'][:, :c1], il['c_a1'], il['cm1'], il['cr1']), (il['dn2'], il['c_a2'], il['cm2'], il['cr2'])]
        else:
            pairs = [(io['dz1a'], x), (io['dz2a'], io['h1a']), (io['dz3a'], io['h2a'])]
            lns = [(il['dn1a'], il['a1'], il['am1'], il['ar1']), (il['dn2a'], il['a2'], il['am2'], il['ar2'])]
        o = 0
        for dz, xin in pairs:
            M, N = dz.shape[1], xin.shape[1]
            grads[o:o + M * N].copy_((dz.t() @ xin).reshape(-1))
            o += M * N
            grads[o:o + M].copy_(dz.sum(0))
            o += M
        for dn, pre, m, rs in lns:             # the LayerNorm elements sit behind the dense ones: gain, bias, gain, bias
            F = dn.shape[1]
            xh = (pre - m.view(-1, 1)) * rs.view(-1, 1)
            grads[o:o + F].copy_((dn * xh).sum(0))
            grads[o + F:o + 2 * F].copy_(dn.sum(0))
            o += 2 * F
        assert o == grads.numel()
        if stats is not None:
            self.ddpg_stats(io['q'], io['y'], io['rewards'], io['actions'], io['q_actor'], stats)
            if stats_host is not None:
                stats_host.view(2, 8)[int(step[0]) & 1, :7].copy_(stats[:7])
        self.adam_step_dev(theta, grads, exp_avg, exp_avg_sq, lr, step, weight_decay, clip_value)
        if target is not None:
            if interval > 0:
                self.hard_update_every(target, theta, step, interval)
            else:
                self.soft_update(target, theta, tau)
        for name in ((group, 'target_' + group) if target is not None else (group,)):
            args.snap[name] = {k: v.clone() for k, v in args.nets[name].items()}

