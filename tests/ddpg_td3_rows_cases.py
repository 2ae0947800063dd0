"""The torch-CPU double of the row schedule's TD3 launches (smx_ddpg_rows_critic_td3_f32, SMX_DDPG_GROUP_CRITIC2,
SMX_DDPG_PACK_SECOND), on top of the stock double: like it, every launch works from row-major SNAPSHOTS of the parameters
that only a pack or an update launch refreshes, so a schedule that left a copy stale fails the goldens here as it would on
the device.  Top-level kernel calls are recorded in `calls`."""
import functools

import torch

from cpu_kernels import TorchCpuKernels


def pack_chunks(K):
    return (((K + 31) >> 5) + 1) & ~1


def pack_words(M, K):
    """16-byte words of one fragment-order block (csrc/smx_epoch_pack.inc.h)"""
    return ((M + 15) >> 4) * pack_chunks(K) * 128


def second_blocks(D, A, H1, H2, c1, c2):
    """(M, K) of the second critic's seven blocks: W1, W2, W3, W2^T lo; the target's W1, W2, W3"""
    return [(c1, D), (c2, c1 + A), (1, c2), (c1, c2), (c1, D), (c2, c1 + A), (1, c2)]


class Td3RowsCpuKernels(TorchCpuKernels):
    ddpg_rows_td3 = True
    RECORDED = ('linear', 'linear_multi', 'linear_wgrad', 'mlp3_forward', 'mlp3_backward', 'adam_step_dev', 'soft_update',
                'hard_update_every', 'ddpg_critic_loss', 'ddpg_critic_loss_step', 'ddpg_stats', 'tanh_backward', 'fill',
                'ddpg_rows_pack', 'ddpg_rows_pack_second', 'ddpg_rows_critic', 'ddpg_rows_critic_td3', 'ddpg_rows_actor',
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

    # ---- the second critic --------------------------------------------------------------------------------------
    def ddpg_rows_second_supported(self, D, A, H1, H2, c1, c2, rows):
        widest = max(c1 + A, H1, H2, c2, D)
        return self.ddpg_rows_supported(D, A, H1, H2, c1, c2, rows=rows) and 0 < rows and rows * widest * 4 < 2 ** 31

    def ddpg_rows_second_packed_floats(self, D, A, H1, H2, c1, c2):
        return 64

    def ddpg_rows_second(self, args, nets2, packed2, io2):
        args.nets2, args.packed2, args.io2 = nets2, packed2, io2
        return args

    def ddpg_rows_pack_second(self, args):
        for name in ('critic2', 'target_critic2'):
            args.snap[name] = {k: v.clone() for k, v in args.nets2[name].items()}

    def ddpg_rows_critic_td3(self, args):
        io, io2, S = args.io, args.io2, args.snap
        D, A, H1, H2, c1, c2 = args.dims
        x, xn = io['x'], io['x_next']
        B = x.shape[0]
        rew, dn = io['rewards'].view(-1), io['dones'].view(-1)
        _, _, a_next = self._rows_actor_fwd(S['target_actor'], xn)
        _, _, q1n = self._rows_critic_fwd(S['target_critic'], xn, a_next)
        a2 = a_next if io2.get('noise') is None else torch.add(a_next, io2['noise']).clamp_(-1.0, 1.0)
        _, _, q2n = self._rows_critic_fwd(S['target_critic2'], xn, a2)
        y = torch.minimum(rew + (args.gamma_n * q1n) * (1.0 - dn), rew + (args.gamma_n * q2n) * (1.0 - dn))
        io['q_next'].copy_(q1n); io2['q_next2'].copy_(torch.minimum(q1n, q2n)); io['y'].copy_(y)
        if io.get('step') is not None:
            io['step'] += 1
        for net, out in ((S['critic'], dict(xcat=io['xcat'], h2c=io['h2c'], q=io['q'], dz3=io['dz3'], dz2=io['dz2'],
                                            dxcat=io['dxcat'])),
                         (S['critic2'], dict(xcat=io2['xcat2'], h2c=io2['h2c2'], q=io2['q2'], dz3=io2['dz3_2'],
                                             dz2=io2['dz2_2'], dxcat=io2['dxcat2']))):
            xcat, h2c, q = self._rows_critic_fwd(net, x, io['actions'])
            dz3 = 2.0 * (q - y) / B
            dz2 = (dz3.view(B, 1) * net['W3'].view(1, c2)) * (h2c > 0)
            out['xcat'].copy_(xcat); out['h2c'].copy_(h2c); out['q'].copy_(q); out['dz3'].copy_(dz3); out['dz2'].copy_(dz2)
            out['dxcat'][:, :c1].copy_((dz2 @ net['W2'][:, :c1]) * (xcat[:, :c1] > 0))
        h1a, h2a, act = self._rows_actor_fwd(S['actor'], x)
        io['h1a'].copy_(h1a); io['h2a'].copy_(h2a); io['act'].copy_(act)

    def ddpg_rows_update(self, args, group, theta, grads, exp_avg, exp_avg_sq, lr, step, weight_decay, clip_value,
                         target=None, tau=0.0, interval=0, wgrad=False, stats=None, stats_host=None):
        io2 = getattr(args, 'io2', None)
        if stats is not None and io2 is not None and io2.get('stats2') is not None:
            # the second block, as ddpg_stats forms it for (q2, y), by the launch that forms the first
            self.ddpg_stats(io2['q2'], args.io['y'], args.io['rewards'], args.io['actions'], io2['q2'], io2['stats2'])
            if stats_host is not None:
                stats_host.view(2, 16)[int(step[0]) & 1, 8:15].copy_(io2['stats2'][:7])
        if group != 'critic2':
            if stats_host is not None and io2 is not None:
                super().ddpg_rows_update(args, group, theta, grads, exp_avg, exp_avg_sq, lr, step, weight_decay, clip_value,
                                         target=target, tau=tau, interval=interval, wgrad=wgrad, stats=stats)
                stats_host.view(2, 16)[int(step[0]) & 1, :7].copy_(stats[:7])
                return
            return super().ddpg_rows_update(args, group, theta, grads, exp_avg, exp_avg_sq, lr, step, weight_decay,
                                            clip_value, target=target, tau=tau, interval=interval, wgrad=wgrad, stats=stats,
                                            stats_host=stats_host)
        assert stats is None
        if wgrad:
            D, A, H1, H2, c1, c2 = args.dims
            o = 0
            for dz, xin in ((io2['dxcat2'][:, :c1], args.io['x']), (io2['dz2_2'], io2['xcat2']),
                            (io2['dz3_2'].view(-1, 1), io2['h2c2'])):
                M, N = dz.shape[1], xin.shape[1]
                grads[o:o + M * N].copy_((dz.t() @ xin).reshape(-1))
                o += M * N
                grads[o:o + M].copy_(dz.sum(0))
                o += M
            assert o == grads.numel()
        self.adam_step_dev(theta, grads, exp_avg, exp_avg_sq, lr, step, weight_decay, clip_value)
        if target is not None:
            if interval > 0:
                self.hard_update_every(target, theta, step, interval)
            else:
                self.soft_update(target, theta, tau)
        for name in (('critic2', 'target_critic2') if target is not None else ('critic2',)):
            args.snap[name] = {k: v.clone() for k, v in args.nets2[name].items()}
