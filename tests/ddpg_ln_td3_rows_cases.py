"""The torch-CPU double of the row schedule's LayerNorm TD3 launches (smx_ddpg_rows_critic_td3_f32 and
SMX_DDPG_GROUP_CRITIC2 with args->ln and its second part), on top of the one-critic LayerNorm double and the TD3 double:
like them, every launch works from row-major SNAPSHOTS of the dense parameters that only a pack or an update launch
refreshes; the LayerNorms' gains and biases -- the second critic's too -- are read from the parameter buffers themselves,
as the kernels read them.  Top-level kernel calls are recorded in `calls`."""
import functools

import torch

from cpu_kernels import TorchCpuKernels
from ddpg_ln_rows_cases import LnRowsCpuKernels, ln_bwd
from ddpg_td3_rows_cases import Td3RowsCpuKernels

RECORDED = tuple(sorted(set(LnRowsCpuKernels.RECORDED) | set(Td3RowsCpuKernels.RECORDED)))


class RecordingStockKernels(TorchCpuKernels):
    """the stock double (no TD3, no LayerNorm row launches) with the same record of top-level calls"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls, self._depth = [], 0
        for name in RECORDED:
            if hasattr(self, name):
                setattr(self, name, self._recording(name, getattr(self, name)))

    def _recording(self, name, fn):
        @functools.wraps(fn)
        def wrapped(*a, **kw):
            if self._depth == 0:
                self.calls.append(name)
            self._depth += 1
            try:
                return fn(*a, **kw)
            finally:
                self._depth -= 1
        return wrapped


class LnTd3RowsCpuKernels(LnRowsCpuKernels, Td3RowsCpuKernels):
    ddpg_rows_ln = True
    ddpg_rows_td3 = True
    ddpg_rows_ln_td3 = True
    RECORDED = RECORDED

    def ddpg_rows_ln_second_supported(self, D, A, H1, H2, c1, c2, rows):
        return (self.ddpg_rows_ln_supported(D, A, H1, H2, c1, c2, rows)
                and self.ddpg_rows_second_supported(D, A, H1, H2, c1, c2, rows))

    def ddpg_rows_ln_second_attach(self, args, ln_nets2, io_ln2):
        assert getattr(args, 'ln_nets', None) is not None and getattr(args, 'io2', None) is not None
        args.ln_nets2, args.io_ln2 = ln_nets2, io_ln2
        return args

    def ddpg_rows_critic(self, args):
        assert getattr(args, 'ln_nets', None) is None or getattr(args, 'io2', None) is None, 'ln with second is refused'
        return super().ddpg_rows_critic(args)

    def ddpg_rows_critic_td3(self, args):
        if getattr(args, 'ln_nets', None) is None:
            return super().ddpg_rows_critic_td3(args)
        assert getattr(args, 'ln_nets2', None) is not None, 'ln without its second part is refused'
        io, io2, il, il2, S, eps = args.io, args.io2, args.io_ln, args.io_ln2, args.snap, args.eps
        LN, LN2 = args.ln_nets, args.ln_nets2
        D, A, H1, H2, c1, c2 = args.dims
        x, xn = io['x'], io['x_next']
        B = x.shape[0]
        rew, dn = io['rewards'].view(-1), io['dones'].view(-1)
        a_next = self._ln_actor_fwd(S['target_actor'], LN['target_actor'], eps, xn)['act']
        q1n = self._ln_critic_fwd(S['target_critic'], LN['target_critic'], eps, xn, a_next)['q']
        a2 = a_next if io2.get('noise') is None else torch.add(a_next, io2['noise']).clamp_(-1.0, 1.0)
        q2n = self._ln_critic_fwd(S['target_critic2'], LN2['target_critic2'], eps, xn, a2)['q']
        y = torch.minimum(rew + (args.gamma_n * q1n) * (1.0 - dn), rew + (args.gamma_n * q2n) * (1.0 - dn))
        io['q_next'].copy_(q1n); io2['q_next2'].copy_(torch.minimum(q1n, q2n)); io['y'].copy_(y)
        if io.get('step') is not None:
            io['step'] += 1
        first = dict(xcat=io['xcat'], c_n2=io['h2c'], q=io['q'], dz3=io['dz3'], dz2=io['dz2'], dxcat=io['dxcat'],
                     dn2=il['dn2'], dz1c=il['dz1c'], c_a1=il['c_a1'], cm1=il['cm1'], cr1=il['cr1'], c_a2=il['c_a2'],
                     cm2=il['cm2'], cr2=il['cr2'])
        second = dict(xcat=io2['xcat2'], c_n2=io2['h2c2'], q=io2['q2'], dz3=io2['dz3_2'], dz2=io2['dz2_2'],
                      dxcat=io2['dxcat2'], dn2=il2['dn2_2'], dz1c=il2['dz1c2'], c_a1=il2['c2_a1'], cm1=il2['c2m1'],
                      cr1=il2['c2r1'], c_a2=il2['c2_a2'], cm2=il2['c2m2'], cr2=il2['c2r2'])
        for net, ln, out in ((S['critic'], LN['critic'], first), (S['critic2'], LN2['critic2'], second)):
            c = self._ln_critic_fwd(net, ln, eps, x, io['actions'])
            dz3 = 2.0 * (c['q'] - y) / B
            for k in ('xcat', 'c_n2', 'q', 'c_a1', 'cm1', 'cr1', 'c_a2', 'cm2', 'cr2'):
                out[k].copy_(c[k])
            dn2 = dz3.view(B, 1) * net['W3'].view(1, c2)
            dz2 = ln_bwd(dn2, c['c_a2'], c['cm2'], c['cr2'], ln['ln2.W'])
            dn1 = dz2 @ net['W2'][:, :c1]
            out['dz3'].copy_(dz3); out['dn2'].copy_(dn2); out['dz2'].copy_(dz2); out['dxcat'][:, :c1].copy_(dn1)
            out['dz1c'].copy_(ln_bwd(dn1, c['c_a1'], c['cm1'], c['cr1'], ln['ln1.W']))
        a = self._ln_actor_fwd(S['actor'], LN['actor'], eps, x)
        io['h1a'].copy_(a['n1']); io['h2a'].copy_(a['n2']); io['act'].copy_(a['act'])
        for k in ('a1', 'am1', 'ar1', 'a2', 'am2', 'ar2'):
            il[k].copy_(a[k])

    def ddpg_rows_update(self, args, group, theta, grads, exp_avg, exp_avg_sq, lr, step, weight_decay, clip_value,
                         target=None, tau=0.0, interval=0, wgrad=False, stats=None, stats_host=None):
        if getattr(args, 'ln_nets', None) is None or getattr(args, 'io2', None) is None:
            return super().ddpg_rows_update(args, group, theta, grads, exp_avg, exp_avg_sq, lr, step, weight_decay,
                                            clip_value, target=target, tau=tau, interval=interval, wgrad=wgrad, stats=stats,
                                            stats_host=stats_host)
        assert wgrad and group in ('actor', 'critic', 'critic2'), 'the LayerNorm path steps with its gradients only'
        assert getattr(args, 'ln_nets2', None) is not None
        io, il, io2, il2 = args.io, args.io_ln, args.io2, args.io_ln2
        D, A, H1, H2, c1, c2 = args.dims
        x = io['x']
        if group == 'critic':
            pairs = [(il['dz1c'], x), (io['dz2'], io['xcat']), (io['dz3'].view(-1, 1), io['h2c'])]
            lns = [(io['dxcat'][:, :c1], il['c_a1'], il['cm1'], il['cr1']), (il['dn2'], il['c_a2'], il['cm2'], il['cr2'])]
        elif group == 'critic2':
            pairs = [(il2['dz1c2'], x), (io2['dz2_2'], io2['xcat2']), (io2['dz3_2'].view(-1, 1), io2['h2c2'])]
            lns = [(io2['dxcat2'][:, :c1], il2['c2_a1'], il2['c2m1'], il2['c2r1']),
                   (il2['dn2_2'], il2['c2_a2'], il2['c2m2'], il2['c2r2'])]
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
            assert group == 'actor'
            self.ddpg_stats(io['q'], io['y'], io['rewards'], io['actions'], io['q_actor'], stats)
            if io2.get('stats2') is not None:      # the second block, (q2, y), by the same launch
                self.ddpg_stats(io2['q2'], io['y'], io['rewards'], io['actions'], io2['q2'], io2['stats2'])
            if stats_host is not None:
                slot = stats_host.view(2, 16)[int(step[0]) & 1]
                slot[:7].copy_(stats[:7])
                if io2.get('stats2') is not None:
                    slot[8:15].copy_(io2['stats2'][:7])
        self.adam_step_dev(theta, grads, exp_avg, exp_avg_sq, lr, step, weight_decay, clip_value)
        if target is not None:
            if interval > 0:
                self.hard_update_every(target, theta, step, interval)
            else:
                self.soft_update(target, theta, tau)
        nets = args.nets2 if group == 'critic2' else args.nets
        for name in ((group, 'target_' + group) if target is not None else (group,)):
            args.snap[name] = {k: v.clone() for k, v in nets[name].items()}
