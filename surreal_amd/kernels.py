"""
Tensor-level facade over the C ABI (include/surreal_amd.h): every method takes torch device
tensors (views allowed where a leading stride is part of the C signature), passes raw
pointers + sizes + the current HIP stream to libsurreal_amd.so, and returns nothing -- outputs
are written into caller-owned tensors, nothing allocates, nothing synchronises.

The learner / replay / agent classes talk to the GPU only through this object, which is what
lets the multi-process (gloo, CPU) tests exercise the sharding logic with a test double.
There is NO fallback in the product: `HipKernels()` raises when the library or a GPU is absent.
"""
import ctypes

import numpy as np
import torch

from surreal_amd import _lib as L


def _row_stride(view, width):
    """leading stride (floats) of a 2-D view whose rows are `width` contiguous floats"""
    assert view.dim() == 2 and view.shape[1] == width and (width == 1 or view.stride(1) == 1), \
        (tuple(view.shape), view.stride())
    return view.stride(0) if view.shape[0] > 1 else max(view.stride(0), width)


def ddpg_rows_ln(kernels):
    """whether `kernels` runs a use_layernorm DDPG iteration (one critic) on the row schedule -- the ddpg_rows_ln_supported /
    ddpg_rows_ln_attach methods below: its `ddpg_rows_ln` attribute; an object without it keeps LayerNorm learners on the
    layer schedule"""
    return bool(getattr(kernels, 'ddpg_rows_ln', False))


def ddpg_rows_ln_td3(kernels):
    """whether `kernels` runs a use_layernorm DDPG iteration with TD3's double critic on the row schedule -- the
    ddpg_rows_ln_second_supported / ddpg_rows_ln_second_attach methods below: its `ddpg_rows_ln_td3` attribute; an object
    without it (ddpg_rows_ln and ddpg_rows_td3 alone do not say so) keeps such learners on the layer-by-layer schedule"""
    return bool(getattr(kernels, 'ddpg_rows_ln_td3', False))


def ddpg_rows_delay(kernels):
    """whether `kernels` runs the row schedule's critic-only iterations of a delayed policy update (policy_delay > 1) -- the
    ddpg_rows_critic_only / ddpg_rows_critic_only_td3 / ddpg_rows_delay_tail methods below: its `ddpg_rows_delay`
    attribute; an object without it keeps a learner with policy_delay > 1 on the layer-by-layer schedule"""
    return bool(getattr(kernels, 'ddpg_rows_delay', False))


def ddpg_rows_td3(kernels):
    """whether this kernels object runs TD3 (a second critic, clipped noise on the target action) on the row schedule --
    the ddpg_rows_second_* / ddpg_rows_critic_td3 methods below: its `ddpg_rows_td3` attribute; an object without it
    (an older CPU double) keeps a double-critic learner on the layer-by-layer schedule"""
    return bool(getattr(kernels, 'ddpg_rows_td3', False))


def ddpg_ln_launch(kernels):
    """whether `kernels` runs a LayerNorm DDPG actor in the one-launch rollout and under the device parameter noise
    (the ln arguments of synth_ddpg_rollout and param_noise_*): its `ddpg_ln_launch` attribute; an object without
    one does not.  A property of the kernels object alone, never of an actor's shape."""
    return bool(getattr(kernels, 'ddpg_ln_launch', False))


def ddpg_variant_task_launch(kernels):
    """whether `kernels` runs a LayerNorm actor and a parameter-noise population in the one-launch DDPG rollout on a task
    env (the ln / pn arguments of synth_ddpg_rollout together with task and resets): its `ddpg_variant_task_launch`
    attribute; an object without one runs the plain actor there.  A property of the kernels object alone."""
    return bool(getattr(kernels, 'ddpg_variant_task_launch', False))


class HipKernels(object):
    name = 'hip'

    def __init__(self):
        L.require_gpu()
        self.lib = L.load()

    @staticmethod
    def _st():
        return L.current_stream()

    # ---- z-filter -----------------------------------------------------------------------
    def zfilter_stats(self, rs, rsq, cnt, eps, mean_out, std_out):
        L.call('smx_zfilter_stats_f32', L.ptr(rs), L.ptr(rsq), L.ptr(cnt), rs.numel(), float(eps),
               L.ptr(mean_out), L.ptr(std_out), self._st())

    def zfilter_forward(self, x_view, mean, std, out):
        rows, D = x_view.shape
        L.call('smx_zfilter_forward_f32', L.ptr(x_view), _row_stride(x_view, D), rows, D,
               L.ptr(mean), L.ptr(std), L.ptr(out), self._st())

    def zfilter_forward_sums(self, x_view, rs, rsq, cnt, eps, out):
        """stats + forward in one launch (an acting agent's one observation per step)"""
        rows, D = x_view.shape
        L.call('smx_zfilter_forward_sums_f32', L.ptr(x_view), _row_stride(x_view, D), rows, D,
               L.ptr(rs), L.ptr(rsq), L.ptr(cnt), float(eps), L.ptr(out), self._st())

    def diaggauss_sample(self, mean, log_var, noise_scale, eps, actions, pd):
        """acting head: pd = [mean, exp(log_var) * noise], actions = clip(eps * std + mean, -1, 1);
        eps None: clip(mean).  actions / pd may be row-strided views (rollout slots)."""
        rows, A = mean.shape
        L.call('smx_diaggauss_sample_f32', L.ptr(mean), _row_stride(mean, A), L.ptr(log_var),
               L.ptr(noise_scale), L.ptr(eps), 0 if eps is None else _row_stride(eps, A), rows, A,
               L.ptr(actions), _row_stride(actions, A), L.ptr(pd),
               0 if pd is None else _row_stride(pd, 2 * A), self._st())

    def zfilter_update(self, x_view, rs, rsq, cnt, count_rows, ws=None):
        """ws: optional scratch of zfilter_update_ws_floats(rows, D) floats -- many rows are then summed by many
        workgroups (smx_zfilter_update_ws_f32)"""
        rows, D = x_view.shape
        if ws is not None:
            L.call('smx_zfilter_update_ws_f32', L.ptr(x_view), _row_stride(x_view, D), rows, D, L.ptr(rs),
                   L.ptr(rsq), L.ptr(cnt), float(count_rows), L.ptr(ws), ws.numel(), self._st())
            return
        L.call('smx_zfilter_update_f32', L.ptr(x_view), _row_stride(x_view, D), rows, D, L.ptr(rs),
               L.ptr(rsq), L.ptr(cnt), float(count_rows), self._st())

    def zfilter_update_ws_floats(self, rows, D):
        return int(self.lib.smx_zfilter_update_ws_floats(int(rows), int(D)))

    # ---- MLP ----------------------------------------------------------------------------
    def mlp3_packed_numel(self, net):
        nbytes = self.lib.smx_mlp3_packed_bytes(net.D, net.H1, net.H2, net.OUT)
        if nbytes == 0:
            raise L.SmxError('fused MLP kernel does not support D=%d H1=%d H2=%d OUT=%d'
                             % (net.D, net.H1, net.H2, net.OUT))
        return nbytes // 4

    def mlp3_pack(self, net, packed):
        L.call('smx_mlp3_pack_f32', ctypes.byref(net.desc), L.ptr(packed), packed.numel() * 4,
               self._st())

    def mlp3_pack_zstats(self, net, packed, zf):
        """mlp3_pack + the statistics of ZFilter `zf` (its _mean / _std buffers) in one launch"""
        L.call('smx_mlp3_pack_zstats_f32', ctypes.byref(net.desc), L.ptr(packed), packed.numel() * 4,
               L.ptr(zf.running_sum), L.ptr(zf.running_sumsq), L.ptr(zf.count), zf.running_sum.numel(),
               float(zf.eps), L.ptr(zf._mean), L.ptr(zf._std), self._st())

    def fused_exact_zfilter(self, on):
        """process-wide: the fused critic pass z-filters with the reference's division (z_filter.py:77) instead of
        (x - m) * (1 / s); the goldens run with the default (off), DESIGN.md 1"""
        L.call('smx_mlp3_fused_exact_zfilter', 1 if on else 0)

    def mlp3_forward_fused(self, packed, net, x_main, x_tail, zmean, zstd, out, act, split_bf16=True):
        """split_bf16: layer 1 of the 16-row kernel on 3-way split-bf16 MFMA (session_config.learner.critic_split_bf16;
        DESIGN.md 3.1) where `packed` carries W1's planes; False: fp32 MFMA throughout"""
        G, T0, D = x_main.shape
        T1 = 0 if x_tail is None else x_tail.shape[1]
        assert x_main.is_contiguous() and (x_tail is None or x_tail.is_contiguous())
        L.call('smx_mlp3_forward_fused_split_f32', L.ptr(packed), packed.numel() * 4, 1 if split_bf16 else 0,
               net.D, net.H1, net.H2, net.OUT, L.ptr(x_main), L.ptr(x_tail), G, T0, T1, L.ptr(zmean),
               L.ptr(zstd), L.ptr(out), act, self._st())

    # rows from which the fused many-row forward pays: below, its 128-row workgroups leave most of the 256 CUs idle and
    # the layered GEMMs (32 x 32 / 64 x 64 tiles) win (7936 rows: 62 workgroups, measured equal)
    FUSED_ROWS_MIN = 24576

    def mlp3_forward(self, net, x, h1, h2, out, act, stop=None, pack=None):
        """forward keeping h1 / h2.  pack: scratch of mlp3_packed_numel(net) floats -- with it, a pass over >=
        FUSED_ROWS_MIN rows of a supported shape runs as ONE fused launch (smx_mlp3_forward_rows_f32)"""
        assert x.is_contiguous()
        if pack is not None and x.shape[0] >= self.FUSED_ROWS_MIN and h1.is_contiguous() and h2.is_contiguous() and \
                L.load().smx_mlp3_forward_rows_supported(net.D, net.H1, net.H2, net.OUT):
            ld = 0 if out.dim() < 2 or out.stride(0) == out.shape[1] else out.stride(0)
            rc = L.load().smx_mlp3_forward_rows_f32(ctypes.byref(net.desc), L.ptr(x), x.shape[0], L.ptr(h1), L.ptr(h2),
                                                    L.ptr(out), act, ld, L.ptr(pack), pack.numel() * 4, L.ptr(stop), self._st())
            if rc != L.SMX_E_UNSUPPORTED:
                L.check(rc, 'smx_mlp3_forward_rows_f32')
                return
        L.call('smx_mlp3_forward_f32', ctypes.byref(net.desc), L.ptr(x), x.shape[0], L.ptr(h1),
               L.ptr(h2), L.ptr(out), act, L.ptr(stop), self._st())

    def _jobs(self, jobs):
        arr = (L.Mlp3Job * len(jobs))()
        for k, j in enumerate(jobs):
            g = lambda name: L.ptr(j.get(name)) if j.get(name) is not None else None  # noqa: E731
            arr[k].net = ctypes.pointer(j['net'].desc)
            arr[k].x = g('x')
            arr[k].rows = j['x'].shape[0]
            arr[k].h1, arr[k].h2, arr[k].out = g('h1'), g('h2'), g('out')
            arr[k].out_act = int(j.get('act', 0))
            out = j.get('out')
            arr[k].out_ld = 0 if out is None or out.dim() < 2 or out.stride(0) == out.shape[1] \
                else out.stride(0)
            arr[k].dz3, arr[k].dz2, arr[k].dz1 = g('dz3'), g('dz2'), g('dz1')
            arr[k].grads, arr[k].sumsq_partials = g('grads'), g('sumsq')
            arr[k].stop_flag = g('stop')
            arr[k].h1T, arr[k].h2T, arr[k].xT = g('h1T'), g('h2T'), g('xT')
            arr[k].dz3T, arr[k].dz2T, arr[k].dz1T = g('dz3T'), g('dz2T'), g('dz1T')
            tv = j.get('h1T')      # all transposed views of a job share one row stride
            arr[k].ldT = 0 if tv is None else (tv.stride(0) if tv.shape[0] > 1 else tv.shape[1])
        return arr

    def mlp3_forward_multi(self, jobs):
        """jobs: list of dicts(net, x, h1, h2, out, act[, stop]) -- one launch per layer for all"""
        L.call('smx_mlp3_forward_multi_f32', self._jobs(jobs), len(jobs), self._st())

    def mlp3_backward_multi(self, jobs):
        """jobs: list of dicts(net, x, h1, h2, dz3, dz2, dz1, grads, sumsq[, stop])"""
        L.call('smx_mlp3_backward_multi_f32', self._jobs(jobs), len(jobs), self._st())

    def mlp3_backward_partials(self, net):
        return self.lib.smx_mlp3_backward_partials(net.D, net.H1, net.H2, net.OUT)

    def mlp3_backward(self, net, x, h1, h2, dz3, dz2, dz1, grads, sumsq, stop=None, ws=None, packT=None, dx=None):
        """ws: optional split-K workspace (>= mlp3_backward_ws_floats(net, rows) floats) for many-row calls that do
        not need the sum-of-squares partials: the weight gradients' rows are cut into chunks.
        packT (scratch of mlp3_dgrad_rows_ws_floats(net) floats) [+ dx (rows, D): wanted gradient w.r.t. x]: from
        FUSED_ROWS_MIN rows on the three data-gradient products run as ONE fused launch (smx_mlp3_backward_rows_f32).
        -> True when dx was written (the caller then skips its own dz1 . W1 product)"""
        if ws is not None and sumsq is None and packT is not None and x.shape[0] >= self.FUSED_ROWS_MIN and \
                dz2.is_contiguous() and dz1.is_contiguous() and (dx is None or dx.is_contiguous()):
            rc = L.load().smx_mlp3_backward_rows_f32(
                ctypes.byref(net.desc), L.ptr(x), L.ptr(h1), L.ptr(h2), L.ptr(dz3), x.shape[0], L.ptr(dz2), L.ptr(dz1),
                L.ptr(dx), L.ptr(grads), L.ptr(ws), ws.numel(), L.ptr(packT), packT.numel(), L.ptr(stop), self._st())
            if rc != L.SMX_E_UNSUPPORTED:
                L.check(rc, 'smx_mlp3_backward_rows_f32')
                return dx is not None
        if ws is not None and sumsq is None:
            L.call('smx_mlp3_backward_splitk_f32', ctypes.byref(net.desc), L.ptr(x), L.ptr(h1), L.ptr(h2),
                   L.ptr(dz3), x.shape[0], L.ptr(dz2), L.ptr(dz1), L.ptr(grads), L.ptr(ws), ws.numel(),
                   L.ptr(stop), self._st())
            return False
        L.call('smx_mlp3_backward_f32', ctypes.byref(net.desc), L.ptr(x), L.ptr(h1), L.ptr(h2),
               L.ptr(dz3), x.shape[0], L.ptr(dz2), L.ptr(dz1), L.ptr(grads), L.ptr(sumsq),
               L.ptr(stop), self._st())

    def mlp3_backward_ws_floats(self, net, rows):
        return int(self.lib.smx_mlp3_backward_ws_floats(net.D, net.H1, net.H2, net.OUT, int(rows)))

    def mlp3_dgrad_rows_ws_floats(self, net):
        """floats of the transposed-weights scratch of the fused many-row data gradients (0: shape not supported)"""
        return int(self.lib.smx_mlp3_dgrad_rows_ws_floats(net.D, net.H1, net.H2, net.OUT))

    # ---- fused row-block epoch kernels (csrc/smx_epoch.hip) ------------------------------
    def epoch_supported(self, *nets):
        """every network by itself, and the launch that carries all of them (its LDS tiles are sized for
        the widest layer of any job)"""
        ok = all(self.lib.smx_epoch_supported(n.D, n.H1, n.H2, n.OUT) for n in nets)
        return bool(ok and self.lib.smx_epoch_supported(max(n.D for n in nets), max(n.H1 for n in nets),
                                                        max(n.H2 for n in nets), max(n.OUT for n in nets)))

    def epoch_blocks(self, rows):
        return self.lib.smx_epoch_blocks(rows)

    def epoch_packed_numel(self, net):
        return self.lib.smx_epoch_packed_floats(net.D, net.H1, net.H2, net.OUT)

    def epoch_pack(self, items):
        """items: [(net, packed)], up to 4: the weights in the forward kernel's fragment order, one launch"""
        arr = (L.EpochPack * len(items))()
        for k, (net, packed) in enumerate(items):
            arr[k].net = ctypes.pointer(net.desc)
            arr[k].packed = L.ptr(packed)
        L.call('smx_epoch_pack_f32', arr, len(items), self._st())

    def epoch_prepare(self, obs0, xn, xnT, xr, zmean=None, zstd=None, ref_filter=None, obs_next=None, xnext=None,
                      ref_log_var=None, ref_std=None, pack=(), zero_words=None):
        """the per-learn preparation of the epoch loops in one launch (smx_epoch_prepare_f32): obs0 /
        obs_next are row-strided [rows, D] views, ref_filter the reference policy's ZFilter (or None),
        ref_std the [rows, A] std columns of ref_pol (a column-slice view), pack [(net, packed)]"""
        rows, D = obs0.shape
        a = L.EpochPrep()
        a.obs0, a.ld_obs0, a.rows, a.D = L.ptr(obs0), _row_stride(obs0, D), rows, D
        a.zmean, a.zstd = L.ptr(zmean), L.ptr(zstd)
        a.xn, a.xnT = L.ptr(xn), L.ptr(xnT)
        a.ldT = 0 if xnT is None else (xnT.stride(0) if xnT.shape[0] > 1 else xnT.shape[1])
        if ref_filter is not None:
            a.ref_sum, a.ref_sumsq, a.ref_count = L.ptr(ref_filter.running_sum), L.ptr(ref_filter.running_sumsq), \
                L.ptr(ref_filter.count)
            a.ref_eps, a.ref_filter = float(ref_filter.eps), 1
        a.xr = L.ptr(xr)
        if xnext is not None:
            a.obs_next, a.ld_next, a.xnext = L.ptr(obs_next), _row_stride(obs_next, D), L.ptr(xnext)
        if ref_std is not None:
            A = ref_std.shape[1]
            a.A, a.ref_log_var, a.ref_std, a.ld_ref = A, L.ptr(ref_log_var), L.ptr(ref_std), _row_stride(ref_std, A)
        if zero_words is not None:
            a.zero_words, a.n_zero = L.ptr(zero_words), zero_words.numel()
        a.n_pack = len(pack)
        for k, (net, packed) in enumerate(pack):
            a.pack[k].net = ctypes.pointer(net.desc)
            a.pack[k].packed = L.ptr(packed)
        L.call('smx_epoch_prepare_f32', ctypes.byref(a), self._st())

    _EPOCH_LOSS = {None: L.EPOCH_LOSS_NONE, 'policy': L.EPOCH_LOSS_POLICY, 'value': L.EPOCH_LOSS_VALUE,
                   'rhs_surr': L.EPOCH_RHS_SURR, 'rhs_kl': L.EPOCH_RHS_KL}

    def _epoch_jobs(self, jobs):
        arr = (L.EpochJob * len(jobs))()
        for k, j in enumerate(jobs):
            g = lambda name: L.ptr(j.get(name)) if j.get(name) is not None else None  # noqa: E731
            x = j['x']
            assert x.is_contiguous()
            arr[k].net = ctypes.pointer(j['net'].desc)
            arr[k].x, arr[k].rows = L.ptr(x), x.shape[0]
            arr[k].h1T, arr[k].h2T = g('h1T'), g('h2T')
            tv = j.get('h1T')
            arr[k].ldT = 0 if tv is None else (tv.stride(0) if tv.shape[0] > 1 else tv.shape[1])
            out = j.get('out')
            arr[k].out = g('out')
            arr[k].out_ld = 0 if out is None or out.dim() < 2 or out.stride(0) == out.shape[1] else out.stride(0)
            arr[k].out_act = int(j.get('act', 0))
            arr[k].loss = self._EPOCH_LOSS[j.get('loss')]
            arr[k].stop_flag = g('stop')
            arr[k].dz3, arr[k].dz3T, arr[k].dz2T, arr[k].dz1T = g('dz3'), g('dz3T'), g('dz2T'), g('dz1T')
            arr[k].packed = g('packed')
        return arr

    @staticmethod
    def _epoch_loss(loss):
        if loss is None:
            return None
        a = L.PpoLosses()
        g = lambda name: L.ptr(loss.get(name)) if loss.get(name) is not None else None  # noqa: E731
        a.mode = int(loss.get('mode', 0))
        if loss.get('log_var') is not None:
            A = loss['log_var'].numel()
            a.A, a.rows = A, int(loss['rows'])
            a.log_var, a.adv = g('log_var'), g('adv')
            if loss.get('actions') is not None:
                a.actions, a.ld_act = g('actions'), _row_stride(loss['actions'], A)
                a.behave, a.ld_beh = g('behave'), _row_stride(loss['behave'], 2 * A)
                a.ref, a.ld_ref = g('ref'), _row_stride(loss['ref'], 2 * A)
            a.g_surr, a.g_kl, a.row_partials = g('g_surr'), g('g_kl'), g('partials')
            a.check_stop, a.will_update = int(loss.get('check_stop', 0)), int(loss.get('will_update', 0))
            a.dlogvar, a.dlogvar_sumsq, a.stats = g('dlogvar'), g('dlogvar_sumsq'), g('stats')
        a.returns, a.v_dz3, a.v_partials = g('returns'), g('v_dz3'), g('v_partials')
        a.v_will_update = int(loss.get('v_will_update', 0))
        return ctypes.byref(a)

    def epoch_pair_fits(self, blocks):
        """can a launch of `blocks` row blocks run with two workgroups per block (all of them resident at once)?"""
        return bool(self.lib.smx_epoch_pair_fits(int(blocks)))

    def epoch_pair_xchg(self, *nets, device=None):
        """the exchange buffer of pair-mode launches over `nets` (zero: its tags count hand-overs from here on; one
        buffer serves every launch of a stream)"""
        n = self.lib.smx_epoch_pair_xchg_bytes(max(t.H1 for t in nets), max(t.H2 for t in nets))
        return torch.zeros(n, dtype=torch.uint8, device=device if device is not None else 'cuda')

    def epoch_forward(self, jobs, loss=None, ctrl=None, n_total=0, xchg=None):
        """jobs: dicts(net, x[, h1T, h2T, out, act, loss='policy'|'value', stop]); loss: dict of the
        loss tensors (see smx_epoch_forward_f32).  One launch: 16 rows per workgroup through the three
        layers and the job's loss.  xchg (epoch_pair_xchg): pair mode, two workgroups per row block where the
        doubled grid fits the device (smx_epoch_forward_pair_f32; the same bits)"""
        if xchg is not None:
            L.call('smx_epoch_forward_pair_f32', self._epoch_jobs(jobs), len(jobs), self._epoch_loss(loss),
                   L.ptr(ctrl), int(n_total), L.ptr(xchg), xchg.numel(), self._st())
            return
        L.call('smx_epoch_forward_f32', self._epoch_jobs(jobs), len(jobs), self._epoch_loss(loss),
               L.ptr(ctrl), int(n_total), self._st())

    def epoch_forward_final(self, jobs, loss, ctrl, n_total, xchg=None, stats_ticket=None, epilogue=None):
        """the learn's final forward-only policy pass with what used to follow it in the same launch
        (smx_epoch_forward_final_f32): stats_ticket (one int32, zero) -- the pass's statistics, epoch_backward's for
        will_update = 0; epilogue (dict of learn_epilogue's arguments) -- the end-of-learn launch.  The same bits."""
        epi = None if epilogue is None else ctypes.byref(self._learn_epilogue_args(**epilogue))
        L.call('smx_epoch_forward_final_f32', self._epoch_jobs(jobs), len(jobs), self._epoch_loss(loss), L.ptr(ctrl),
               int(n_total), L.ptr(xchg), 0 if xchg is None else xchg.numel(), L.ptr(stats_ticket), epi, self._st())

    def epoch_backward(self, jobs, loss, ctrl, n_total):
        """jobs: dicts(net, x, h1T, h2T, loss, dz2T, dz1T[, dz3T (policy), dz3 (value), stop])"""
        L.call('smx_epoch_backward_f32', self._epoch_jobs(jobs), len(jobs), self._epoch_loss(loss),
               L.ptr(ctrl), int(n_total), self._st())

    def epoch_fwdbwd_supported(self, *nets):
        return bool(all(self.lib.smx_epoch_fwdbwd_supported(n.D, n.H1, n.H2, n.OUT) for n in nets) and
                    self.lib.smx_epoch_fwdbwd_supported(max(n.D for n in nets), max(n.H1 for n in nets),
                                                        max(n.H2 for n in nets), max(n.OUT for n in nets)))

    def epoch_fwdbwd(self, jobs, loss, ctrl, n_total, sync_word, kl_slots, xchg=None):
        """epoch_forward + epoch_backward of an updating epoch in ONE launch (smx_epoch_fwdbwd_f32); sync_word: one
        int32, kl_slots: 2 * epoch_blocks(rows) 4-byte words (8-byte aligned) per launch, zero on entry; xchg: pair
        mode as in epoch_forward (smx_epoch_fwdbwd_pair_f32)"""
        if xchg is not None:
            L.call('smx_epoch_fwdbwd_pair_f32', self._epoch_jobs(jobs), len(jobs), self._epoch_loss(loss),
                   L.ptr(ctrl), int(n_total), L.ptr(sync_word), L.ptr(kl_slots), L.ptr(xchg), xchg.numel(), self._st())
            return
        L.call('smx_epoch_fwdbwd_f32', self._epoch_jobs(jobs), len(jobs), self._epoch_loss(loss),
               L.ptr(ctrl), int(n_total), L.ptr(sync_word), L.ptr(kl_slots), self._st())

    def layernorm_forward(self, x, gamma, beta, eps, y, mean=None, rstd=None):
        """y = LayerNorm(x) over the last dimension (rows of x / y may be strided); mean / rstd [rows] for the backward"""
        rows, F = x.shape
        L.call('smx_layernorm_forward_f32', L.ptr(x), x.stride(0), rows, F, L.ptr(gamma), L.ptr(beta), float(eps), L.ptr(y),
               y.stride(0), L.ptr(mean), L.ptr(rstd), self._st())

    def layernorm_backward_ws_floats(self, rows, F):
        return int(self.lib.smx_layernorm_backward_ws_floats(int(rows), int(F)))

    def layernorm_backward(self, dy, x, mean, rstd, gamma, dx, dgamma, dbeta, ws, relu_mask=False):
        """dx (optionally times x > 0: x is a ReLU's output) and the affine parameters' gradients (overwritten)"""
        rows, F = x.shape
        L.call('smx_layernorm_backward_f32', L.ptr(dy), dy.stride(0), L.ptr(x), x.stride(0), L.ptr(mean), L.ptr(rstd),
               L.ptr(gamma), rows, F, int(bool(relu_mask)), L.ptr(dx), dx.stride(0), L.ptr(dgamma), L.ptr(dbeta), L.ptr(ws),
               ws.numel(), self._st())

    def device_occupy(self, blocks, microseconds):
        """a co-tenant on the current stream: `blocks` workgroups that each hold one CU for `microseconds` (smx_device_occupy)"""
        L.call('smx_device_occupy', int(blocks), int(microseconds), self._st())

    def mlp3_wgrad_multi(self, jobs):
        """the weight-gradient launch alone: dicts(net, x (for rows), grads, sumsq, xT, h1T, h2T, dz3T,
        dz2T, dz1T[, stop])"""
        L.call('smx_mlp3_wgrad_multi_f32', self._jobs(jobs), len(jobs), self._st())

    # ---- GAE / normalisation ------------------------------------------------------------
    def gae(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, H, adv, ret,
            values_tail=None):
        L.call('smx_windowed_gae_returns_f32', L.ptr(values), L.ptr(values_tail), L.ptr(rewards),
               L.ptr(dones),
               L.ptr(gpow), L.ptr(lpow), float(gamma), float(gamma_H), B, N, H, L.ptr(adv),
               L.ptr(ret), self._st())

    def gae_norm(self, values, rewards, dones, gpow, lpow, gamma, gamma_H, B, N, H, adv, ret, adv_mom, min_std, ticket,
                 values_tail=None):
        """gae + moments + adv_normalize in one launch (single rank)"""
        L.call('smx_windowed_gae_norm_f32', L.ptr(values), L.ptr(values_tail), L.ptr(rewards), L.ptr(dones),
               L.ptr(gpow), L.ptr(lpow), float(gamma), float(gamma_H), B, N, H, L.ptr(adv), L.ptr(ret), L.ptr(adv_mom),
               float(min_std), L.ptr(ticket), self._st())

    def reward_filter_partials(self):
        return int(self.lib.smx_reward_filter_partials())

    def reward_filter(self, rewards, scale, state, eps, out, partials, ticket, use_filter=True, update=True, sums=None):
        """out = clamp((rewards * scale - mean) / std, -5, 5) from `state` = [count, sum, sumsq] as it was BEFORE
        the call, then state <- batch (reward_filter.py:33-57); use_filter=False: the scale alone"""
        L.call('smx_reward_filter_f32', L.ptr(rewards), rewards.numel(), float(scale), int(use_filter), L.ptr(state),
               float(eps), int(update), L.ptr(out), L.ptr(sums), L.ptr(partials), L.ptr(ticket), self._st())

    def learn_epilogue(self, ret, ret_mom, log_var, out4, ticket, zfilter=None, x=None, count_rows=0, v_partials=None,
                       n_epochs=0, nblk=0, v_stats=None, stats_stride=0):
        """value_finalize + moments(ret) + zfilter_update(x) + final_stats in one launch (single rank)"""
        a = self._learn_epilogue_args(ret, ret_mom, log_var, out4, ticket, zfilter, x, count_rows, v_partials, n_epochs,
                                      nblk, v_stats, stats_stride)
        L.call('smx_ppo_learn_epilogue_f32', ctypes.byref(a), self._st())

    @staticmethod
    def _learn_epilogue_args(ret, ret_mom, log_var, out4, ticket, zfilter=None, x=None, count_rows=0, v_partials=None,
                             n_epochs=0, nblk=0, v_stats=None, stats_stride=0):
        a = L.LearnEpilogue()
        if zfilter is not None:
            rows, D = x.shape
            a.x, a.ldx, a.rows, a.D = L.ptr(x), _row_stride(x, D), rows, D
            a.running_sum, a.running_sumsq, a.count = L.ptr(zfilter.running_sum), L.ptr(zfilter.running_sumsq), \
                L.ptr(zfilter.count)
            a.count_rows = float(count_rows)
        a.A = log_var.numel()
        a.ret, a.n_ret, a.ret_moments = L.ptr(ret), ret.numel(), L.ptr(ret_mom)
        a.v_partials, a.n_epochs, a.nblk, a.v_stats, a.stats_stride = L.ptr(v_partials), n_epochs, nblk, L.ptr(v_stats), \
            stats_stride
        a.log_var, a.out4, a.ticket = L.ptr(log_var), L.ptr(out4), L.ptr(ticket)
        return a

    def moments(self, x, out):
        L.call('smx_moments_f32', L.ptr(x), x.numel(), L.ptr(out), self._st())

    def moments_merge(self, parts, out):
        L.call('smx_moments_merge_f32', L.ptr(parts), parts.numel() // 3, L.ptr(out), self._st())

    def adv_normalize(self, x, mom, min_std):
        L.call('smx_adv_normalize_f32', L.ptr(x), x.numel(), L.ptr(mom), float(min_std), self._st())

    # ---- losses -------------------------------------------------------------------------
    def loss_blocks(self, rows):
        return self.lib.smx_ppo_loss_blocks(rows)

    def policy_loss(self, mode, mean, log_var, actions, behave, ref, adv, ctrl, g_surr, g_kl,
                    partials):
        rows, A = mean.shape
        L.call('smx_ppo_policy_loss_f32', mode, L.ptr(mean), L.ptr(log_var), L.ptr(actions),
               _row_stride(actions, A), L.ptr(behave), _row_stride(behave, 2 * A), L.ptr(ref),
               _row_stride(ref, 2 * A), L.ptr(adv), rows, A, L.ptr(ctrl), L.ptr(g_surr),
               L.ptr(g_kl), L.ptr(partials), self._st())

    def partials_fold(self, partials, nblk, out, ctrl=None):
        """out[j] = sum of the partial rows [j R, (j + 1) R), R = ceil(nblk / len(out)) (smx_ppo_partials_fold_f32)"""
        L.call('smx_ppo_partials_fold_f32', L.ptr(partials), int(nblk), partials.stride(0), L.ptr(out), out.shape[0],
               L.ptr(ctrl), self._st())

    def policy_finalize(self, mode, partials, nblk, g_surr, g_kl, log_var, n_total, ctrl,
                        check_stop, will_update, dz3, dlogvar, dlogvar_sumsq, stats, dz3_t=None):
        rows, A = g_surr.shape
        L.call('smx_ppo_loss_finalize_f32', mode, L.ptr(partials), nblk, L.ptr(g_surr),
               L.ptr(g_kl), L.ptr(log_var), rows, n_total, A, L.ptr(ctrl), int(check_stop),
               int(will_update), L.ptr(dz3), L.ptr(dz3_t),
               0 if dz3_t is None else dz3_t.stride(0), L.ptr(dlogvar), L.ptr(dlogvar_sumsq),
               L.ptr(stats), self._st())

    def _losses_args(self, mode, mean, log_var, actions, behave, ref, adv, g_surr, g_kl, partials,
                     check_stop, will_update, values, returns, v_dz3, v_partials, v_will_update):
        rows, A = mean.shape
        a = L.PpoLosses()
        a.mode, a.A, a.rows = mode, A, rows
        a.mean, a.log_var, a.adv = L.ptr(mean), L.ptr(log_var), L.ptr(adv)
        a.actions, a.ld_act = L.ptr(actions), _row_stride(actions, A)
        a.behave, a.ld_beh = L.ptr(behave), _row_stride(behave, 2 * A)
        a.ref, a.ld_ref = L.ptr(ref), _row_stride(ref, 2 * A)
        a.g_surr, a.g_kl, a.row_partials = L.ptr(g_surr), L.ptr(g_kl), L.ptr(partials)
        a.check_stop, a.will_update = int(check_stop), int(will_update)
        a.values, a.returns = L.ptr(values), L.ptr(returns)
        a.v_dz3, a.v_partials, a.v_will_update = L.ptr(v_dz3), L.ptr(v_partials), int(v_will_update)
        return a

    def epoch_losses(self, mode, mean, log_var, actions, behave, ref, adv, ctrl, g_surr, g_kl,
                     partials, check_stop, will_update, dz3, dlogvar, dlogvar_sumsq, stats, dz3_t=None,
                     values=None, returns=None, v_dz3=None, v_partials=None, v_will_update=True):
        """policy_loss + policy_finalize (+ value_loss) of a single-GPU lock-step epoch, one launch"""
        a = self._losses_args(mode, mean, log_var, actions, behave, ref, adv, g_surr, g_kl, partials,
                              check_stop, will_update, values, returns, v_dz3, v_partials, v_will_update)
        a.dz3, a.dz3_t = L.ptr(dz3), L.ptr(dz3_t)
        a.ld_t = 0 if dz3_t is None else (dz3_t.stride(0) if dz3_t.shape[0] > 1 else dz3_t.shape[1])
        a.dlogvar, a.dlogvar_sumsq, a.stats = L.ptr(dlogvar), L.ptr(dlogvar_sumsq), L.ptr(stats)
        L.call('smx_ppo_epoch_losses_f32', ctypes.byref(a), L.ptr(ctrl), self._st())

    def epoch_losses_dp(self, mode, mean, log_var, actions, behave, ref, adv, ctrl, g_surr, g_kl,
                        partials, n_total, g_surr_t=None, g_kl_t=None, values=None, returns=None,
                        v_dz3=None, v_partials=None, v_will_update=True):
        """the loss launch of a data-parallel lock-step epoch: gradient tiles come out divided by
        n_total (+ transposed copies), no finalize -- see smx_ppo_epoch_combine_f32"""
        a = self._losses_args(mode, mean, log_var, actions, behave, ref, adv, g_surr, g_kl, partials,
                              False, False, values, returns, v_dz3, v_partials, v_will_update)
        t = g_surr_t
        a.ld_t = 0 if t is None else (t.stride(0) if t.shape[0] > 1 else t.shape[1])
        L.call('smx_ppo_epoch_losses_dp_f32', ctypes.byref(a), int(n_total), L.ptr(g_surr_t),
               L.ptr(g_kl_t), L.ptr(ctrl), self._st())

    def epoch_combine(self, mode, partials, nblk, n_total, log_var, ctrl, check_stop, will_update,
                      stats, grads_a, grads_kl, n_mlp, sumsq_a, grads_c=None, sumsq_c=None):
        """after the all-reduce of a data-parallel epoch: grads_a += c_kl * grads_kl, log_var's
        gradient, statistics / early exit, sum-of-squares partials of both groups"""
        a = L.PpoCombine()
        a.mode, a.A, a.nblk, a.n_total = mode, log_var.numel(), nblk, int(n_total)
        a.row_partials, a.log_var, a.stats = L.ptr(partials), L.ptr(log_var), L.ptr(stats)
        a.check_stop, a.will_update = int(check_stop), int(will_update)
        a.grads_a, a.grads_kl = L.ptr(grads_a), L.ptr(grads_kl)
        a.n_mlp, a.n_a, a.sumsq_a = int(n_mlp), grads_a.numel(), L.ptr(sumsq_a)
        a.grads_c, a.sumsq_c = L.ptr(grads_c), L.ptr(sumsq_c)
        a.n_c = 0 if grads_c is None else grads_c.numel()
        L.call('smx_ppo_epoch_combine_f32', ctypes.byref(a), L.ptr(ctrl), self._st())

    def final_stats(self, log_var, zfilter, out4):
        """means the learner reports once per learn (ppo.py:572, 580-583), formed on the device so
        that the statistics need ONE read-back"""
        zf = zfilter
        L.call('smx_ppo_final_stats_f32', L.ptr(log_var), log_var.numel(),
               L.ptr(zf.running_sum) if zf is not None else None,
               L.ptr(zf.running_sumsq) if zf is not None else None,
               L.ptr(zf.count) if zf is not None else None,
               zf.running_sum.numel() if zf is not None else 0, L.ptr(out4), self._st())

    def value_loss_blocks(self, rows):
        return self.lib.smx_value_loss_blocks(rows)

    def value_loss(self, values, returns, n_total, dz3, partials, ctrl, will_update):
        L.call('smx_value_loss_f32', L.ptr(values), L.ptr(returns), values.numel(), n_total,
               L.ptr(dz3), L.ptr(partials), L.ptr(ctrl), int(will_update), self._st())

    def value_finalize(self, partials, count, nblk, stats, stride):
        L.call('smx_value_loss_finalize_f32', L.ptr(partials), count, nblk, L.ptr(stats), stride,
               self._st())

    # ---- optimiser ----------------------------------------------------------------------
    def clip_adam(self, theta, grads, m, v, sumsq, npart, ctrl, which, honour_stop, grad_norm_out, pack=None):
        if pack is not None:
            g = L.AdamGroup(L.ptr(theta), L.ptr(grads), L.ptr(m), L.ptr(v), theta.numel(), L.ptr(sumsq), npart,
                            int(honour_stop), L.ptr(grad_norm_out))
            g.pack_net, g.packed = ctypes.pointer(pack[0].desc), L.ptr(pack[1])
            L.call('smx_clip_adam_step_group_f32', ctypes.byref(g), which, L.ptr(ctrl), self._st())
            return
        L.call('smx_clip_adam_step_f32', L.ptr(theta), L.ptr(grads), L.ptr(m), L.ptr(v),
               theta.numel(), L.ptr(sumsq), npart, L.ptr(ctrl), which, int(honour_stop),
               L.ptr(grad_norm_out), self._st())

    def clip_adam_pair(self, actor, critic, ctrl, pack=None):
        """actor / critic: (theta, grads, m, v, sumsq, npart, honour_stop, grad_norm_out);
        pack: ((actor net, packed), (critic net, packed)) -- the step also refreshes the fused epoch
        kernels' packed weight copies"""
        gs = []
        for k, (theta, grads, m, v, sumsq, npart, honour_stop, gno) in enumerate((actor, critic)):
            g = L.AdamGroup(L.ptr(theta), L.ptr(grads), L.ptr(m), L.ptr(v), theta.numel(),
                            L.ptr(sumsq), npart, int(honour_stop), L.ptr(gno))
            if pack is not None:
                g.pack_net, g.packed = ctypes.pointer(pack[k][0].desc), L.ptr(pack[k][1])
            gs.append(g)
        L.call('smx_clip_adam_step_pair_f32', ctypes.byref(gs[0]), ctypes.byref(gs[1]), L.ptr(ctrl),
               self._st())

    def sumsq_blocks(self, n):
        return self.lib.smx_sumsq_blocks(n)

    def sumsq_partials(self, x, partials):
        L.call('smx_sumsq_partials_f32', L.ptr(x), x.numel(), L.ptr(partials), self._st())

    # ---- replay / windowing ---------------------------------------------------------------
    def ring_insert(self, table, cursor, src):
        """table [capacity, width] <- src [n, width] at ring position `cursor`; fp32 or any other element type
        (uint8 frames), as long as both agree"""
        cap, width = table.shape
        assert table.dtype == src.dtype and src.is_contiguous(), (table.dtype, src.dtype)
        if table.dtype == torch.float32:
            L.call('smx_ring_insert_f32', L.ptr(table), cap, width, int(cursor), L.ptr(src),
                   src.shape[0], self._st())
        else:
            L.call('smx_ring_insert_bytes', L.ptr(table), cap, width * table.element_size(), int(cursor),
                   L.ptr(src), src.shape[0], self._st())

    def gather_rows(self, table, idx, dst):
        cap, width = table.shape
        assert table.dtype == dst.dtype and dst.is_contiguous(), (table.dtype, dst.dtype)
        if table.dtype == torch.float32:
            L.call('smx_gather_rows_f32', L.ptr(table), cap, width, L.ptr(idx), idx.numel(),
                   L.ptr(dst), self._st())
        else:
            L.call('smx_gather_rows_bytes', L.ptr(table), cap, width * table.element_size(), L.ptr(idx),
                   idx.numel(), L.ptr(dst), self._st())

    def uniform_gather_multi(self, tables, outs, length, seed, offset, idx=None, idx_out=None):
        """a whole uniform sample in one launch: row idx[i] -- or, idx None, the row smx_uniform_indices(length, seed,
        offset) would draw -- of every table [capacity, width] -> outs[k] [rows, width] (<= 8 tables, fp32 or uint8)"""
        arr = (L.GatherJob * len(tables))()
        cap, rows = tables[0].shape[0], outs[0].shape[0]
        for k, (t, o) in enumerate(zip(tables, outs)):
            assert t.dtype == o.dtype and o.is_contiguous() and t.shape[0] == cap and o.shape[0] == rows
            arr[k].table, arr[k].dst, arr[k].row_bytes = L.ptr(t), L.ptr(o), t.shape[1] * t.element_size()
        L.call('smx_uniform_gather_multi', arr, len(tables), cap, rows, L.ptr(idx), int(length), int(seed), int(offset),
               L.ptr(idx_out), self._st())

    def uniform_gather_pool(self, tables, outs, pool, pixel, pixel_next, length, seed, offset, base, idx=None,
                            idx_out=None):
        """uniform_gather_multi for a frame-pool replay, ONE launch (smx_uniform_gather_pool): the field tables as there,
        and for the same rows pixel / pixel_next uint8 [rows, S*F] built from the pool.  pool: the replay's frame pool
        (UniformReplay.frame_pool): 'pool' uint8 [n, P, F], 'frame_next' / 'frame_first' int64 [capacity],
        'frame_actor' int32 [capacity], 'frame_stacks', 'n_step'.  A drawn row is (base + u) % capacity, u the draw of
        uniform_indices(length, seed, offset)"""
        arr = (L.GatherJob * len(tables))()
        cap, rows = tables[0].shape[0], outs[0].shape[0]
        for k, (t, o) in enumerate(zip(tables, outs)):
            assert t.dtype == o.dtype and o.is_contiguous() and t.shape[0] == cap and o.shape[0] == rows
            arr[k].table, arr[k].dst, arr[k].row_bytes = L.ptr(t), L.ptr(o), t.shape[1] * t.element_size()
        fp, S = pool['pool'], int(pool['frame_stacks'])
        n, P, F = fp.shape
        assert fp.dtype == torch.uint8 and fp.is_contiguous()
        for k, dt in (('frame_next', torch.int64), ('frame_first', torch.int64), ('frame_actor', torch.int32)):
            assert pool[k].dtype == dt and pool[k].is_contiguous() and pool[k].numel() == cap, k
        for o in (pixel, pixel_next):
            assert o.dtype == torch.uint8 and o.is_contiguous() and o.numel() == rows * S * F
        q = L.GatherPool()
        q.pool, q.pool_len, q.frame_bytes = L.ptr(fp), P, F
        q.actors, q.frame_stacks, q.n_step = n, S, int(pool['n_step'])
        q.frame_next, q.frame_first, q.frame_actor = (L.ptr(pool[k]) for k in ('frame_next', 'frame_first',
                                                                               'frame_actor'))
        q.pixel, q.pixel_next, q.base = L.ptr(pixel), L.ptr(pixel_next), int(base)
        L.call('smx_uniform_gather_pool', arr, len(tables), ctypes.byref(q), cap, rows, L.ptr(idx), int(length),
               int(seed), int(offset), L.ptr(idx_out), self._st())

    def philox4x32_10(self, ctr_key, out):
        """ctr_key [n, 6] int32 (bit patterns of uint32) -> out [n, 4] int32: the sampler's generator by itself"""
        L.call('smx_philox4x32_10', L.ptr(ctr_key), ctr_key.shape[0], L.ptr(out), self._st())

    def uniform_indices(self, idx, length, seed, offset):
        L.call('smx_uniform_indices', L.ptr(idx), idx.numel(), int(length), int(seed), int(offset),
               self._st())

    def window_emit(self, src, start, n_step, stride, W, dst):
        """src [actors, T, width] -> dst [actors*W, n_step, width]"""
        actors, T, width = src.shape
        assert src.is_contiguous() and dst.is_contiguous() and src.dtype == dst.dtype
        if src.dtype == torch.float32:
            L.call('smx_window_emit_f32', L.ptr(src), actors, T, width, start, n_step, stride, W,
                   L.ptr(dst), self._st())
        else:
            L.call('smx_window_emit_bytes', L.ptr(src), actors, T, width * src.element_size(), start, n_step,
                   stride, W, L.ptr(dst), self._st())

    def frame_stack(self, frames, n_stack, start, n_step, stride, W, dst, episode_first=None):
        """frames [actors, R, C, H, W] uint8 (one raw frame per step) -> dst [actors*W, n_step, n_stack*C, H, W]: the
        last n_stack frames on the channel axis, oldest first, history filled with the first frame after a reset"""
        actors, R = frames.shape[:2]
        fb = frames[0, 0].numel() * frames.element_size()
        assert frames.is_contiguous() and dst.is_contiguous() and frames.dtype == dst.dtype
        assert dst.numel() == actors * W * n_step * n_stack * frames[0, 0].numel()
        L.call('smx_frame_stack_u8', L.ptr(frames), actors, R, fb, int(n_stack), L.ptr(episode_first), int(start),
               int(n_step), int(stride), int(W), L.ptr(dst), self._st())

    def synth_frames(self, s0, t, dst):
        """the synthetic camera for all actors: s0 [n] (strided view allowed), dst [n, C, H, W] uint8 (row-strided
        view allowed: a rollout slot)"""
        n, C, H, W = dst.shape
        assert dst.dtype == torch.uint8 and dst[0].is_contiguous() and s0.dim() == 1
        L.call('smx_synth_frame_u8', L.ptr(s0), s0.stride(0), n, C, H, W, int(t), L.ptr(dst), dst.stride(0), self._st())

    @staticmethod
    def _monitor_args(monitor, n):
        """struct smx_episode_monitor of a DeviceEpisodeMonitor (surreal_amd/env/monitor.py) over n actors; None: the
        null monitor, with which every launch does what it does without one"""
        q = L.EpisodeMonitor()
        if monitor is not None:
            m = monitor
            assert m.n == n and m.ep_reward.dtype == torch.float64 and m.done_reward.dtype == torch.float64
            assert m.ep_steps.dtype == torch.int32 and m.done_steps.dtype == torch.int32 and m.ep_count.dtype == torch.int64
            assert m.ep_reward.numel() == m.ep_steps.numel() == m.ep_count.numel() == n
            assert m.done_reward.numel() == m.done_steps.numel() == n * m.capacity
            for x in (m.ep_reward, m.ep_steps, m.ep_count, m.done_reward, m.done_steps):
                assert x.is_contiguous()
            q.ep_reward, q.ep_steps, q.ep_count = L.ptr(m.ep_reward), L.ptr(m.ep_steps), L.ptr(m.ep_count)
            q.done_reward, q.done_steps, q.capacity = L.ptr(m.done_reward), L.ptr(m.done_steps), int(m.capacity)
        return q

    @staticmethod
    def _noise_args(noise):
        """struct smx_noise_stream of a (seed, actor_base, step) triple (DeviceNoise.at, surreal_amd/env/monitor.py):
        the stream a launch forms its draws from when it gets no eps; None: the zero struct, no stream"""
        q = L.NoiseStream()
        if noise is not None:
            q.seed, q.actor_base, q.step = (int(v) for v in noise)
            q.enabled = 1
        return q

    @staticmethod
    def _reset_args(resets):
        """struct smx_reset_stream of a (seed, actor_base, episode[, disturbance]) tuple (DeviceResets.at,
        surreal_amd/env/monitor.py): the stream a task launch draws its episodes' first rows from, and -- with a fourth
        element != 0, the scale -- its per-step disturbances (env/tasks.py: disturbance)"""
        q = L.ResetStream()
        q.seed, q.actor_base, q.episode = (int(v) for v in resets[:3])
        if len(resets) > 3:
            q.disturbance = float(resets[3])
        q.enabled = 1
        return q

    def reset_fill(self, resets, out, task='reach'):
        """out [n, D] fp32 contiguous <- the rows the n actors of a `task` env on the stream `resets` = (seed,
        actor_base, episode) begin that episode with (smx_reset_fill_f32)"""
        n, D = out.shape
        assert out.is_contiguous() and out.dtype == torch.float32
        L.call('smx_reset_fill_f32', ctypes.byref(self._reset_args(resets)), self._task_id(task), n, D, L.ptr(out),
               self._st())

    def noise_fill(self, noise, out):
        """out [steps, n, A] fp32 contiguous <- the draws a launch on the stream `noise` = (seed, actor_base, step)
        forms for n actors over `steps` steps (smx_noise_fill_f32)"""
        steps, n, A = out.shape
        assert out.is_contiguous() and out.dtype == torch.float32
        L.call('smx_noise_fill_f32', ctypes.byref(self._noise_args(noise)), steps, n, A, L.ptr(out), self._st())

    @classmethod
    def _synth_act_step(cls, state, init_state, mean, A, log_var, noise_scale, eps, t, episode_len, slot, rolls, zfilter,
                        xn_out, monitor=None, noise=None):
        n, D = state.shape
        p = L.SynthActStep()
        p.mon = cls._monitor_args(monitor, n)
        p.noise = cls._noise_args(noise)
        p.state, p.init_state = L.ptr(state), L.ptr(init_state)
        p.mean, p.ld_mean, p.log_var = L.ptr(mean), (0 if mean is None else _row_stride(mean, A)), L.ptr(log_var)
        p.noise_scale, p.eps = L.ptr(noise_scale), L.ptr(eps)
        p.ld_eps = 0 if eps is None else _row_stride(eps, A)
        p.n, p.D, p.A, p.t, p.episode_len, p.slot = n, D, A, int(t), int(episode_len), int(slot)
        r = rolls or {}
        p.T = r['obs'].shape[1] if 'obs' in r else 1
        p.obs_roll, p.act_roll = L.ptr(r.get('obs')), L.ptr(r.get('actions'))
        p.rew_roll, p.done_roll, p.pd_roll = L.ptr(r.get('rewards')), L.ptr(r.get('dones')), L.ptr(r.get('pds'))
        if zfilter is not None:
            p.zsum, p.zsumsq, p.zcount = L.ptr(zfilter.running_sum), L.ptr(zfilter.running_sumsq), L.ptr(zfilter.count)
            p.zeps = float(zfilter.eps)
        p.xn_out = L.ptr(xn_out)
        return p

    def synth_act_env_step(self, state, init_state, mean, log_var, noise_scale, eps, t, episode_len,
                           slot, rolls, zfilter, xn_out, monitor=None, noise=None):
        """acting head + env step + next observation's z-filter, one launch (see the header);
        rolls: dict obs / actions / rewards / dones [/ pds] or None; zfilter: ZFilter or None; monitor: a
        DeviceEpisodeMonitor or None; noise: (seed, actor_base, step) of the stream the launch draws from when eps is
        None, or None (every synth_* launch below that samples takes both the same way)"""
        p = self._synth_act_step(state, init_state, mean, mean.shape[1], log_var, noise_scale, eps, t, episode_len,
                                 slot, rolls, zfilter, xn_out, monitor, noise)
        L.call('smx_synth_act_env_step_f32', ctypes.byref(p), self._st())

    def synth_act_env_step_head(self, W3, b3, h2, out_act, state, init_state, log_var, noise_scale, eps, t,
                                episode_len, slot, rolls, zfilter, xn_out, monitor=None, noise=None):
        """the same launch with the policy's output layer folded in: mean = act(h2 . W3^T + b3) formed per actor"""
        A, H2 = W3.shape
        p = self._synth_act_step(state, init_state, None, A, log_var, noise_scale, eps, t, episode_len, slot, rolls,
                                 zfilter, xn_out, monitor, noise)
        L.call('smx_synth_act_env_step_head_f32', ctypes.byref(p), L.ptr(W3), L.ptr(b3), L.ptr(h2),
               _row_stride(h2, H2), H2, int(out_act), self._st())

    def synth_rollout_supported(self, net):
        return bool(self.lib.smx_synth_rollout_supported(net.D, net.H1, net.H2, net.OUT))

    @classmethod
    def _roll_args(cls, q, net, packed, out_act, state, init_state, log_var, noise_scale, eps, t, episode_len, steps,
                   zfilter, actors_per_workgroup, rolls=None, slot=0, monitor=None, noise=None):
        """fills the SynthRollout `q`: the network, the head, the z-filter, state and clock, and (rolls: dict as in
        synth_act_env_step, also 'obs_last' / 'cells') the rollout tables"""
        n = state.shape[0]
        q.net, q.packed, q.out_act, q.n = ctypes.pointer(net.desc), L.ptr(packed), int(out_act), n
        q.log_var, q.noise_scale, q.eps = L.ptr(log_var), L.ptr(noise_scale), L.ptr(eps)
        if eps is not None:
            assert eps.is_contiguous() and tuple(eps.shape) == (steps, n, net.OUT)
        if zfilter is not None:
            q.zsum, q.zsumsq, q.zcount = L.ptr(zfilter.running_sum), L.ptr(zfilter.running_sumsq), L.ptr(zfilter.count)
            q.zeps = float(zfilter.eps)
        q.t, q.episode_len, q.steps, q.slot = int(t), int(episode_len), int(steps), int(slot)
        q.state, q.init_state = L.ptr(state), L.ptr(init_state)
        q.actors_per_workgroup = int(actors_per_workgroup)
        q.mon = cls._monitor_args(monitor, n)
        q.noise = cls._noise_args(noise)
        if rolls is not None:
            r = rolls
            q.rows_per_actor = r['obs'].shape[1] if 'obs' in r else (r['cells'].shape[1] if 'cells' in r else 1)
            q.obs_roll, q.act_roll = L.ptr(r.get('obs')), L.ptr(r.get('actions'))
            q.rew_roll, q.done_roll, q.pd_roll = L.ptr(r.get('rewards')), L.ptr(r.get('dones')), L.ptr(r.get('pds'))
            q.obs_last = L.ptr(r.get('obs_last'))      # rows_per_actor == steps: the replay's layout (obs_next apart)

    @staticmethod
    def _lstm_args(p, model, lstm_packed, n, hN, cN, h0, c0, h_before, c_before):
        """fills the LSTM block of the SynthLstmRollout `p`; the states [n, Hl] contiguous"""
        Hl = model.rnn_hidden_logical
        for x in (h0, c0, hN, cN, h_before, c_before):
            assert x is None or (x.is_contiguous() and x.numel() == n * Hl)
        p.lstm, p.lstm_packed, p.hidden = ctypes.pointer(model.rnn.desc), L.ptr(lstm_packed), Hl
        p.h0, p.c0, p.hN, p.cN = L.ptr(h0), L.ptr(c0), L.ptr(hN), L.ptr(cN)
        p.h_before, p.c_before = L.ptr(h_before), L.ptr(c_before)

    @staticmethod
    def _window_args(p, n_step, advance, carry, tables, cursor):
        """fills the moving-window block of `p`: the carry rings, the FIFO's tables by replay field name, the cursor"""
        p.n_step, p.advance = int(n_step), int(advance)
        p.carry_obs, p.carry_act, p.carry_rew = L.ptr(carry['obs']), L.ptr(carry['actions']), L.ptr(carry['rewards'])
        p.carry_pd, p.carry_cells = L.ptr(carry['pds']), L.ptr(carry.get('cells'))
        p.obs, p.obs_next, p.actions = L.ptr(tables['obs']), L.ptr(tables['obs_next']), L.ptr(tables['actions'])
        p.rewards, p.dones, p.pds = L.ptr(tables['rewards']), L.ptr(tables['dones']), L.ptr(tables['pds'])
        p.cells = L.ptr(tables.get('cells'))
        p.cursor, p.capacity = int(cursor), int(tables['obs'].shape[0])

    @staticmethod
    def _camera_args(p, r, frames_per_row):
        """checks and fills the camera block of `p` from r['hist'] [n, Hd, C, H, W], r['obs_pixel'] [n, S*C, H, W],
        r['hist_pos'] and the ring's 'pixel' (frames_per_row stacked frames a row) / 'pixel_next' (one) uint8 tables"""
        n, Hd, C, H, W = r['hist'].shape
        tabs = r['tables']
        S = r['obs_pixel'].shape[1] // C
        for k in ('hist', 'obs_pixel'):
            assert r[k].dtype == torch.uint8 and r[k].is_contiguous(), k
        assert tuple(r['obs_pixel'].shape) == (n, S * C, H, W) and r['state'].shape[0] == n
        for k, w in (('pixel', frames_per_row * S * C * H * W), ('pixel_next', S * C * H * W)):
            assert tabs[k].dtype == torch.uint8 and tabs[k].is_contiguous(), k
            assert tuple(tabs[k].shape) == (tabs['obs'].shape[0], w), k
        p.C, p.H, p.W, p.frame_stacks = C, H, W, S
        p.hist_len, p.hist_pos = Hd, int(r['hist_pos'])
        p.hist, p.obs_pixel = L.ptr(r['hist']), L.ptr(r['obs_pixel'])
        p.pixel, p.pixel_next = L.ptr(tabs['pixel']), L.ptr(tabs['pixel_next'])

    def synth_rollout(self, net, packed, out_act, state, init_state, log_var, noise_scale, eps, t, episode_len,
                      steps, slot, rolls, zfilter, actors_per_workgroup=0, monitor=None, noise=None):
        """`steps` acting + environment steps of all actors in ONE launch (csrc/smx_rollout.hip): a workgroup owns
        4, 8 or 16 actors for the whole rollout (actors_per_workgroup; 0: the smallest whose grid fits the CUs once).
        packed: epoch_pack of `net`; eps [steps, n, A] or None; rolls as in synth_act_env_step ([n, T + 1, .]
        tables)."""
        p = L.SynthRollout()
        self._roll_args(p, net, packed, out_act, state, init_state, log_var, noise_scale, eps, t, episode_len, steps,
                        zfilter, actors_per_workgroup, rolls or {}, slot, monitor, noise)
        L.call('smx_synth_rollout_f32', ctypes.byref(p), self._st())

    def synth_lstm_rollout_supported(self, model):
        """a PPOModel whose policy smx_synth_lstm_rollout_f32 runs: one LSTM layer on low-dimensional observations,
        shapes it takes"""
        if not model.if_rnn or model.rnn_layers != 1 or model.if_pixel:
            return False
        a, r = model.actor, model.rnn
        return a.D == r.H and bool(self.lib.smx_synth_lstm_rollout_supported(r.D, r.H, a.H1, a.H2, a.OUT))

    def lstm_rollout_packed_numel(self, lstm):
        return int(self.lib.smx_lstm_rollout_packed_floats(lstm.D, lstm.H))

    def lstm_rollout_pack(self, lstm, packed):
        """the gate pass's packed copy of an LstmParams (smx_lstm_rollout_pack_f32)"""
        L.call('smx_lstm_rollout_pack_f32', ctypes.byref(lstm.desc), L.ptr(packed), self._st())

    def synth_lstm_rollout(self, model, packed, lstm_packed, state, init_state, noise_scale, eps, t, episode_len, steps,
                           slot, rolls, zfilter, hN, cN, h0=None, c0=None, h_before=None, c_before=None,
                           actors_per_workgroup=0, monitor=None, noise=None):
        """synth_rollout for a PPOModel with a one-layer LSTM stem, ONE launch (smx_synth_lstm_rollout_f32): packed =
        epoch_pack of model.actor, lstm_packed = lstm_rollout_pack of model.rnn; rolls may also hold 'cells'
        [n, R, 2, 1, Hl] (the state before every step); h0 / c0 (None: zeros), hN / cN, h_before / c_before: [n, Hl]
        contiguous, Hl = model.rnn_hidden_logical"""
        r = rolls or {}
        p = L.SynthLstmRollout()
        self._roll_args(p.roll, model.actor, packed, L.SMX_ACT_TANH, state, init_state, model.log_var, noise_scale, eps,
                        t, episode_len, steps, zfilter, actors_per_workgroup, r, slot, monitor, noise)
        self._lstm_args(p, model, lstm_packed, state.shape[0], hN, cN, h0, c0, h_before, c_before)
        if 'cells' in r:
            assert r['cells'].is_contiguous() and tuple(r['cells'].shape[2:]) == (2, 1, model.rnn_hidden_logical)
        p.cell_roll = L.ptr(r.get('cells'))
        L.call('smx_synth_lstm_rollout_f32', ctypes.byref(p), self._st())

    def synth_ppo_window_rollout_supported(self, model):
        """a PPOModel whose policy smx_synth_ppo_window_rollout_f32 runs: a plain MLP, or one LSTM layer, on
        low-dimensional observations, shapes it takes"""
        if model.if_pixel or (model.if_rnn and model.rnn_layers != 1):
            return False
        a = model.actor
        if not model.if_rnn:
            return bool(self.lib.smx_synth_ppo_window_rollout_supported(a.D, 0, a.H1, a.H2, a.OUT))
        r = model.rnn
        return a.D == r.H and bool(self.lib.smx_synth_ppo_window_rollout_supported(r.D, r.H, a.H1, a.H2, a.OUT))

    def synth_ppo_window_rollout(self, model, packed, lstm_packed, state, init_state, noise_scale, eps, t, episode_len,
                                 steps, n_step, advance, carry, tables, cursor, zfilter, hN=None, cN=None, h0=None,
                                 c0=None, h_before=None, c_before=None, actors_per_workgroup=0, monitor=None,
                                 noise=None, clocks=None, task='drift', resets=None):
        """`steps` steps of synth_rollout (model.rnn None) / synth_lstm_rollout recorded as moving windows of n_step
        steps, `advance` apart, straight into a FIFO ring, ONE launch (smx_synth_ppo_window_rollout_f32).
        carry: the open windows {'obs' [n, n_step, D], 'actions' [n, n_step, A], 'rewards' [n, n_step], 'pds'
        [n, n_step, 2A], 'cells' [n, ceil(n_step / advance), 2, Hl] (LSTM)}; tables: the ring by replay field name
        ('obs' [capacity, n_step * D], 'obs_next', 'actions', 'rewards', 'dones', 'pds', 'cells' (LSTM)); the k-th
        closing step writes actor a to row (cursor + k n + a) % capacity.  h0 / c0 (None: zeros), hN / cN (LSTM),
        h_before / c_before: [n, Hl] contiguous, Hl = model.rnn_hidden_logical.
        clocks: an episode clock per actor (_clock_args; smx_synth_ppo_window_rollout_clocks_f32) -- t / episode_len
        are then ignored and the closing windows go to the rows of clocks['row_off'] (actor_clock_rows).
        task: the environment's dynamics (env/tasks.py; smx_synth_ppo_window_rollout_task_f32; the shared clock only).
        resets: a task env's reset stream (_reset_args; smx_synth_ppo_window_rollout_resets_f32) -- init_state is then not
        read"""
        p = L.SynthPpoWindowRollout()
        self._roll_args(p.base.roll, model.actor, packed, L.SMX_ACT_TANH, state, init_state, model.log_var, noise_scale,
                        eps, t, episode_len, steps, zfilter, actors_per_workgroup, monitor=monitor, noise=noise)
        if model.if_rnn:
            self._lstm_args(p.base, model, lstm_packed, state.shape[0], hN, cN, h0, c0, h_before, c_before)
        for k, x in list(carry.items()) + list(tables.items()):
            assert x.is_contiguous() and x.dtype == torch.float32, k
        self._window_args(p, n_step, advance, carry, tables, cursor)
        assert resets is None or task != 'drift', "task 'drift' has no reset distribution"
        if task != 'drift':
            assert clocks is None, 'a task env has one shared clock'
            if resets is not None:
                L.call('smx_synth_ppo_window_rollout_resets_f32', ctypes.byref(p), self._task_id(task),
                       ctypes.byref(self._reset_args(resets)), self._st())
                return
            L.call('smx_synth_ppo_window_rollout_task_f32', ctypes.byref(p), self._task_id(task), self._st())
            return
        if clocks is not None:
            c = self._clock_args(clocks, state.shape[0], steps)
            L.call('smx_synth_ppo_window_rollout_clocks_f32', ctypes.byref(p), ctypes.byref(c), self._st())
            return
        L.call('smx_synth_ppo_window_rollout_f32', ctypes.byref(p), self._st())

    @staticmethod
    def _task_id(task):
        """SMX_TASK_* of a task's name (env/tasks.py)"""
        from surreal_amd.env.tasks import TASK_IDS
        return int(TASK_IDS[task])

    def synth_task_supported(self, task, D, A):
        """the (task, observation width, action width) the task entry points take (smx_synth_task_supported); task: a
        name of env/tasks.py or a raw SMX_TASK_* id"""
        tid = self._task_id(task) if isinstance(task, str) else int(task)
        return bool(self.lib.smx_synth_task_supported(tid, int(D), int(A)))

    def synth_eval_supported(self, task, model=None, actor=None):
        """the policies the evaluation launches take on `task` (smx_synth_eval_supported): model, a PPOModel with a
        plain-MLP or one-layer LSTM policy on low-dimensional observations; or actor, a plain DDPG actor's Mlp3Params"""
        tid = self._task_id(task)
        if actor is not None:
            return bool(self.lib.smx_synth_eval_supported(1, tid, actor.D, 0, actor.H1, actor.H2, actor.OUT))
        if model.if_pixel or (model.if_rnn and model.rnn_layers != 1):
            return False
        a = model.actor
        if not model.if_rnn:
            return bool(self.lib.smx_synth_eval_supported(0, tid, a.D, 0, a.H1, a.H2, a.OUT))
        r = model.rnn
        return a.D == r.H and bool(self.lib.smx_synth_eval_supported(0, tid, r.D, r.H, a.H1, a.H2, a.OUT))

    @staticmethod
    def _eval_returns(returns, n, episodes):
        assert returns.dtype == torch.float64 and returns.is_contiguous() and tuple(returns.shape) == (n, episodes)
        return L.ptr(returns)

    def _eval_block(self, p, net, init_state, episodes, episode_len, task, resets, actors_per_workgroup):
        """what both evaluation blocks (p: a fresh SynthPpoEval / SynthDdpgEval) hold whether the parameters come from
        the caller's tensors or from snapshots: the actor's shapes, the rows, the task and the reset stream -> (p, n)"""
        n = init_state.shape[0]
        assert init_state.is_contiguous() and init_state.dtype == torch.float32
        p.net, p.n = ctypes.pointer(net.desc), n
        p.episodes, p.episode_len, p.task = int(episodes), int(episode_len), self._task_id(task)
        p.actors_per_workgroup = int(actors_per_workgroup)
        p.init_state = L.ptr(init_state)
        if resets is not None:
            p.resets = self._reset_args(resets)
        return p, n

    def _ppo_eval_block(self, model, init_state, episodes, episode_len, zfilter, task, resets, noise,
                        actors_per_workgroup, out_act):
        """_eval_block for PPOModel `model`, with the LSTM stem's shapes, the z-filter's eps and the noise stream"""
        p, n = self._eval_block(L.SynthPpoEval(), model.actor, init_state, episodes, episode_len, task, resets,
                                actors_per_workgroup)
        p.out_act = int(out_act)
        if zfilter is not None:
            p.zeps = float(zfilter.eps)
        if model.if_rnn:
            p.lstm, p.hidden = ctypes.pointer(model.rnn.desc), model.rnn_hidden_logical
        p.noise = self._noise_args(noise)
        return p, n

    def synth_ppo_eval(self, model, packed, lstm_packed, init_state, episodes, episode_len, returns, zfilter=None,
                       task='drift', resets=None, noise=None, actors_per_workgroup=0, out_act=L.SMX_ACT_TANH):
        """`episodes` whole episodes of every actor under PPOModel `model`'s policy, ONE launch, nothing recorded
        (smx_synth_ppo_eval_f32): returns [n, episodes] fp64 <- the episodes' returns.  packed: epoch_pack of model.actor,
        lstm_packed: lstm_rollout_pack of model.rnn (None: a plain MLP); init_state [n, D]; resets: (seed, actor_base,
        first_episode) of the reset stream the episodes begin from, or None: every episode begins at init_state[a];
        noise: (seed, actor_base, first_step) -- the policy samples (eval_stochastic) -- or None: it acts on its mean;
        out_act: the output layer's activation (PPOModel's is tanh)"""
        p, n = self._ppo_eval_block(model, init_state, episodes, episode_len, zfilter, task, resets, noise,
                                    actors_per_workgroup, out_act)
        p.packed, p.log_var = L.ptr(packed), L.ptr(model.log_var)
        if zfilter is not None:
            p.zsum, p.zsumsq, p.zcount = L.ptr(zfilter.running_sum), L.ptr(zfilter.running_sumsq), L.ptr(zfilter.count)
        if model.if_rnn:
            p.lstm_packed = L.ptr(lstm_packed)
        p.returns = self._eval_returns(returns, n, int(episodes))
        L.call('smx_synth_ppo_eval_f32', ctypes.byref(p), self._st())

    def synth_ddpg_eval(self, net, packed, init_state, episodes, episode_len, returns, task='drift', resets=None,
                        actors_per_workgroup=0):
        """the same for a plain DDPG actor `net` in a deterministic agent mode (smx_synth_ddpg_eval_f32)"""
        p, n = self._eval_block(L.SynthDdpgEval(), net, init_state, episodes, episode_len, task, resets,
                                actors_per_workgroup)
        p.packed = L.ptr(packed)
        p.returns = self._eval_returns(returns, n, int(episodes))
        L.call('smx_synth_ddpg_eval_f32', ctypes.byref(p), self._st())

    # ---- several parameter sets in one evaluation launch (snapshots) ----
    def eval_snapshot_floats(self, model=None, actor=None, zfilter=False):
        """floats of one snapshot (smx_eval_snapshot_floats): model, a PPOModel (zfilter: its z-filter's sums are part of
        the snapshot), or actor, a plain DDPG actor's Mlp3Params; 0: a policy no evaluation launch takes"""
        if actor is not None:
            return int(self.lib.smx_eval_snapshot_floats(1, actor.D, 0, actor.H1, actor.H2, actor.OUT, 0))
        a = model.actor
        if model.if_pixel or (model.if_rnn and (model.rnn_layers != 1 or a.D != model.rnn.H)):
            return 0
        D, H = (model.rnn.D, model.rnn.H) if model.if_rnn else (a.D, 0)
        return int(self.lib.smx_eval_snapshot_floats(0, D, H, a.H1, a.H2, a.OUT, int(bool(zfilter))))

    def eval_snapshot_store(self, blob, model=None, actor=None, zfilter=None):
        """blob (float32, 16-byte aligned, eval_snapshot_floats long) <- the snapshot of the live parameters, no
        synchronisation (smx_eval_snapshot_store_f32): model, a PPOModel, with zfilter its ZFilter or None; or actor, a
        plain DDPG actor's Mlp3Params"""
        s = L.EvalSnapshotSrc()
        if actor is not None:
            need = self.eval_snapshot_floats(actor=actor)
            s.net, s.ddpg = ctypes.pointer(actor.desc), 1
        else:
            need = self.eval_snapshot_floats(model=model, zfilter=zfilter is not None)
            s.net, s.log_var = ctypes.pointer(model.actor.desc), L.ptr(model.log_var)
            if zfilter is not None:
                s.zsum, s.zsumsq, s.zcount = L.ptr(zfilter.running_sum), L.ptr(zfilter.running_sumsq), L.ptr(zfilter.count)
            if model.if_rnn:
                s.lstm = ctypes.pointer(model.rnn.desc)
        assert blob.dtype == torch.float32 and blob.is_contiguous() and blob.numel() >= need > 0
        L.call('smx_eval_snapshot_store_f32', ctypes.byref(s), L.ptr(blob), self._st())

    @staticmethod
    def _eval_sets(blobs, sets, zfilter, returns, n, episodes):
        """struct smx_eval_sets of the first `sets` rows of blobs [K, stride] (a row-strided float32 view), and the
        check of returns [sets, n, episodes]"""
        assert blobs.dtype == torch.float32 and blobs.dim() == 2 and blobs.stride(1) == 1 and blobs.shape[0] >= sets
        assert returns.dtype == torch.float64 and returns.is_contiguous() and tuple(returns.shape) == (sets, n, episodes)
        s = L.EvalSets()
        s.blobs, s.stride = L.ptr(blobs), int(blobs.stride(0)) if blobs.shape[0] > 1 else int(blobs.shape[1])
        s.sets, s.zfilter = int(sets), int(bool(zfilter))
        return s

    def synth_ppo_eval_sets(self, model, blobs, init_state, episodes, episode_len, returns, zfilter=None, task='drift',
                            resets=None, noise=None, actors_per_workgroup=0, out_act=L.SMX_ACT_TANH):
        """synth_ppo_eval for the blobs.shape[0] snapshots in the rows of blobs [sets, stride] in ONE launch
        (smx_synth_ppo_eval_sets_f32): returns [sets, n, episodes] fp64.  model gives the shapes alone -- its parameters
        are not read; zfilter: the ZFilter whose eps applies (the snapshots hold the sums), or None"""
        p, n = self._ppo_eval_block(model, init_state, episodes, episode_len, zfilter, task, resets, noise,
                                    actors_per_workgroup, out_act)
        s = self._eval_sets(blobs, blobs.shape[0], zfilter is not None, returns, n, int(episodes))
        p.returns = L.ptr(returns)
        L.call('smx_synth_ppo_eval_sets_f32', ctypes.byref(p), ctypes.byref(s), self._st())

    def synth_ddpg_eval_sets(self, net, blobs, init_state, episodes, episode_len, returns, task='drift', resets=None,
                             actors_per_workgroup=0):
        """the same for plain DDPG actors of net's shapes (smx_synth_ddpg_eval_sets_f32)"""
        p, n = self._eval_block(L.SynthDdpgEval(), net, init_state, episodes, episode_len, task, resets,
                                actors_per_workgroup)
        s = self._eval_sets(blobs, blobs.shape[0], False, returns, n, int(episodes))
        p.returns = L.ptr(returns)
        L.call('smx_synth_ddpg_eval_sets_f32', ctypes.byref(p), ctypes.byref(s), self._st())

    def actor_clock_rows(self, t, episode_len, steps, n_step, advance, row_off, t_host=None, episode_len_host=None):
        """row_off [steps, n] int32 <- where every closing (step, actor) pair of a call of `steps` steps goes, counted
        from the ring's cursor in (step, actor) order, -1 where the pair closes nothing (smx_actor_clock_rows_i32): actor
        a starts at clock t[a] of episodes of episode_len[a] steps (int32 [n] on the device) and closes a record at
        clock tau iff j = tau + 1 - n_step >= 0 and j % advance == 0 (DDPG: advance 1).  t_host / episode_len_host: the
        numpy int32 arrays they were copied from, checked before the launch"""
        n = t.numel()
        for x in (t, episode_len, row_off):
            assert x.dtype == torch.int32 and x.is_contiguous()
        assert episode_len.numel() == n and tuple(row_off.shape) == (steps, n)
        p = L.ActorClockRows()
        p.n, p.steps, p.n_step, p.advance = n, int(steps), int(n_step), int(advance)
        p.t, p.episode_len, p.row_off = L.ptr(t), L.ptr(episode_len), L.ptr(row_off)
        for name, h in (('t_host', t_host), ('episode_len_host', episode_len_host)):
            if h is not None:
                assert h.dtype == np.int32 and h.flags['C_CONTIGUOUS'] and h.size == n
                setattr(p, name, h.ctypes.data)
        L.call('smx_actor_clock_rows_i32', ctypes.byref(p), self._st())

    @staticmethod
    def _clock_args(clocks, n, steps):
        """struct smx_actor_clocks from {'t', 'episode_len' int32 [n], 'row_off' int32 [steps, n], 'rows'}"""
        c = L.ActorClocks()
        for k in ('t', 'episode_len', 'row_off'):
            assert clocks[k].dtype == torch.int32 and clocks[k].is_contiguous(), k
        assert clocks['t'].numel() == n == clocks['episode_len'].numel()
        assert tuple(clocks['row_off'].shape) == (steps, n)
        c.t, c.episode_len, c.row_off = L.ptr(clocks['t']), L.ptr(clocks['episode_len']), L.ptr(clocks['row_off'])
        c.rows = int(clocks['rows'])
        return c

    # a LayerNorm actor runs in the one-launch DDPG rollout and under the parameter noise (ddpg_ln_launch(), above)
    ddpg_ln_launch = True
    # both of them on a task env too (ddpg_variant_task_launch(), above)
    ddpg_variant_task_launch = True
    # TD3 on the row schedule (ddpg_rows_td3(), above)
    ddpg_rows_td3 = True
    # use_layernorm on the row schedule (ddpg_rows_ln(), above)
    ddpg_rows_ln = True
    # use_layernorm together with TD3 on the row schedule (ddpg_rows_ln_td3(), above)
    ddpg_rows_ln_td3 = True
    # critic-only iterations of a delayed policy update on the row schedule (ddpg_rows_delay(), above)
    ddpg_rows_delay = True

    def synth_ddpg_rollout_supported(self, net, ln=False):
        """the actor shapes synth_ddpg_rollout takes; ln: with a LayerNorm behind each hidden ReLU"""
        return bool(self.lib.smx_synth_ddpg_rollout_supported(net.D, net.H1, net.H2, net.OUT, int(bool(ln))))

    @classmethod
    def _ddpg_args(cls, r, steps, net=None, packed=None, actors_per_workgroup=0, monitor=None, noise=None):
        """smx_ddpg_rollout_t from the dict SyntheticVecEnv.ddpg_rollout_into builds: state / init_state [n, D],
        t, episode_len, n_step, noise_type, eps, sigmas (fp64), theta / dt / root_dt, gpow (fp64 [n_step]), ou (fp64
        [n, A]), carry_obs / carry_act / carry_rew, the ring tables by replay field name, cursor, capacity"""
        n, D = r['state'].shape
        tabs = r['tables']
        p = L.DdpgRollout()
        p.net = ctypes.pointer(net.desc) if net is not None else None
        p.packed = L.ptr(packed)
        p.n, p.D, p.A, p.steps = n, D, tabs['actions'].shape[1], int(steps)
        p.t, p.episode_len, p.n_step, p.noise_type = int(r['t']), int(r['episode_len']), int(r['n_step']), \
            int(r['noise_type'])
        p.actors_per_workgroup = int(actors_per_workgroup)
        p.eps, p.sigmas = L.ptr(r['eps']), L.ptr(r['sigmas'])
        p.theta, p.dt, p.root_dt = float(r['theta']), float(r['dt']), float(r['root_dt'])
        p.gpow, p.ou = L.ptr(r['gpow']), L.ptr(r['ou'])
        p.state, p.init_state = L.ptr(r['state']), L.ptr(r['init_state'])
        p.carry_obs, p.carry_act, p.carry_rew = L.ptr(r['carry_obs']), L.ptr(r['carry_act']), L.ptr(r['carry_rew'])
        p.obs, p.obs_next, p.actions = L.ptr(tabs['obs']), L.ptr(tabs['obs_next']), L.ptr(tabs['actions'])
        p.rewards, p.dones = L.ptr(tabs['rewards']), L.ptr(tabs['dones'])
        p.cursor, p.capacity = int(r['cursor']), int(tabs['obs'].shape[0])
        p.mon = cls._monitor_args(monitor, n)
        p.noise = cls._noise_args(noise)
        return p

    @staticmethod
    def _ln_ptr(net, ln):
        """ln: None, or ln1.W | ln1.b | ln2.W | ln2.b contiguous (DDPGModel.actor_ln_flat)"""
        if ln is None:
            return None
        assert ln.dtype == torch.float32 and ln.is_contiguous() and ln.numel() == 2 * (net.H1 + net.H2)
        return L.ptr(ln)

    @staticmethod
    def _population_ptrs(pn):
        """-> (pop, its row stride, dist) of a DeviceParamNoise-like `pn`: pop fp32 [P, stride], dist fp64 [P]"""
        assert pn.pop.dtype == torch.float32 and pn.pop.is_contiguous() and pn.dist.dtype == torch.float64
        assert pn.pop.shape[0] == int(pn.agents) == pn.dist.numel() and pn.dist.is_contiguous()
        return L.ptr(pn.pop), pn.pop.shape[1], L.ptr(pn.dist)

    @classmethod
    def _variant_args(cls, net, ln, ln_eps, pn, measure_step):
        """struct smx_ddpg_actor_variant of synth_ddpg_rollout's ln / ln_eps / pn / measure_step"""
        v = L.DdpgActorVariant()
        v.ln, v.ln_eps = cls._ln_ptr(net, ln), float(ln_eps)
        if pn is not None:
            v.packed_pop, v.packed_stride, v.dist = cls._population_ptrs(pn)
            v.actors_per_agent, v.agents, v.measure_step = int(pn.actors_per_agent), int(pn.agents), int(measure_step)
        return v

    def synth_ddpg_rollout(self, net, packed, r, steps, actors_per_workgroup=0, monitor=None, noise=None, ln=None,
                           ln_eps=0.0, pn=None, measure_step=-1, clocks=None, task='drift', resets=None):
        """`steps` DDPG acting + environment steps of all actors with their n-step transitions written into the ring
        tables, ONE launch (smx_synth_ddpg_rollout_f32, csrc/smx_rollout.hip).  packed: epoch_pack of the actor `net`;
        r: see _ddpg_args (eps [steps, n, A]).
        ln, ln_eps: a LayerNorm (gains and biases, eps) behind each hidden ReLU of `net`.
        pn: every agent of `pn` (pn.actors_per_agent consecutive actors) acts from its own copy in pn.pop
        (param_noise_refresh's, for the same ln); net / packed / ln are the clean actor, evaluated at step measure_step
        (-1: never) for pn.dist.
        clocks: an episode clock per actor (_clock_args; smx_synth_ddpg_rollout_clocks_f32) -- r['t'] / r['episode_len']
        are then ignored and the closing transitions go to the rows of clocks['row_off'] (actor_clock_rows, advance 1).
        task: the environment's dynamics (env/tasks.py; smx_synth_ddpg_rollout_task_f32, with ln or pn
        smx_synth_ddpg_rollout_variant_task_f32: the shared clock only).  resets: a task env's reset stream (_reset_args;
        smx_synth_ddpg_rollout_resets_f32) -- r['init_state'] is then not read"""
        if r['eps'] is not None:
            assert r['eps'].is_contiguous() and tuple(r['eps'].shape) == (steps, r['state'].shape[0], net.OUT)
        p = self._ddpg_args(r, steps, net, packed, actors_per_workgroup, monitor, noise)
        assert resets is None or task != 'drift', "task 'drift' has no reset distribution"
        if task != 'drift':
            assert clocks is None, 'a task env runs on one shared clock'
            if ln is not None or pn is not None:
                # the actor variants on a task (smx_synth_ddpg_rollout_variant_task_f32)
                v = self._variant_args(net, ln, ln_eps, pn, measure_step)
                L.call('smx_synth_ddpg_rollout_variant_task_f32', ctypes.byref(p), ctypes.byref(v), self._task_id(task),
                       ctypes.byref(self._reset_args(resets)) if resets is not None else None, self._st())
                return
            if resets is not None:
                L.call('smx_synth_ddpg_rollout_resets_f32', ctypes.byref(p), self._task_id(task),
                       ctypes.byref(self._reset_args(resets)), self._st())
                return
            L.call('smx_synth_ddpg_rollout_task_f32', ctypes.byref(p), self._task_id(task), self._st())
            return
        v = self._variant_args(net, ln, ln_eps, pn, measure_step)
        if clocks is not None:
            c = self._clock_args(clocks, r['state'].shape[0], steps)
            L.call('smx_synth_ddpg_rollout_clocks_f32', ctypes.byref(p), ctypes.byref(v), ctypes.byref(c), self._st())
            return
        L.call('smx_synth_ddpg_rollout_f32', ctypes.byref(p), ctypes.byref(v), self._st())

    def synth_ddpg_population_block(self, n, actors_per_agent, forced=0):
        """the block size the launch takes for a population (0: it refuses)"""
        return int(self.lib.smx_synth_ddpg_population_block(int(n), int(actors_per_agent), int(forced)))

    # ---- parameter-space noise on the device (csrc/smx_param_noise.hip; DeviceParamNoise, env/monitor.py); ln: as above,
    # the flat parameters then go on with it and every copy carries the perturbed four behind its biases ----
    def param_noise_copy_numel(self, net, ln=False):
        """floats of one agent's copy in the population buffer: epoch_pack's layout, then the biases, then (ln) the
        LayerNorm parameters"""
        return int(self.lib.smx_param_noise_copy_floats(net.D, net.H1, net.H2, net.OUT, int(bool(ln))))

    @classmethod
    def _param_noise_args(cls, net, pn, ln):
        """struct smx_param_noise of the clean actor `net` (, `ln`) and a DeviceParamNoise-like `pn`: seed, agent_base,
        generation, acts, adaptive, alpha, target, sigma / dist (fp64 [P]), pop ([P, stride] fp32)"""
        q = L.ParamNoise()
        q.net = ctypes.pointer(net.desc)
        q.seed, q.agent_base, q.generation = int(pn.seed), int(pn.agent_base), int(pn.generation)
        q.agents, q.adaptive, q.acts = int(pn.agents), int(bool(pn.adaptive)), int(pn.acts)
        q.alpha, q.target = float(pn.alpha), float(pn.target)
        assert pn.sigma.dtype == torch.float64 and pn.sigma.numel() == q.agents and pn.sigma.is_contiguous()
        q.sigma, q.ln = L.ptr(pn.sigma), cls._ln_ptr(net, ln)
        q.packed_pop, q.packed_stride, q.dist = cls._population_ptrs(pn)
        return q

    def param_noise_fill(self, net, pn, p, out, ln=None):
        """out [numel of the actor's flat parameters, ln's included] <- agent p's perturbed parameters
        (smx_param_noise_fill_f32)"""
        assert out.is_contiguous() and out.dtype == torch.float32
        assert out.numel() == net.numel + (0 if ln is None else ln.numel())
        L.call('smx_param_noise_fill_f32', ctypes.byref(self._param_noise_args(net, pn, ln)), int(p), L.ptr(out),
               self._st())

    def param_noise_refresh(self, net, pn, ln=None):
        """the device form of on_parameter_fetched for all agents of `pn` (smx_param_noise_refresh_f32): the adaptive
        rule on sigma when pn.adaptive and pn.acts > 0, then every agent's copy of the perturbed `net` (, `ln`) into
        pn.pop"""
        L.call('smx_param_noise_refresh_f32', ctypes.byref(self._param_noise_args(net, pn, ln)), self._st())

    def synth_ddpg_step(self, r, mu, monitor=None, noise=None):
        """one step of synth_ddpg_rollout given the actor's output mu [n, A] (r['eps']: this step's [n, A] draws;
        r['cursor']: where this step's closing transitions go)"""
        A = mu.shape[1]
        p = self._ddpg_args(r, 1, monitor=monitor, noise=noise)
        L.call('smx_synth_ddpg_step_f32', ctypes.byref(p), L.ptr(mu), _row_stride(mu, A), self._st())

    def synth_ddpg_pixel_step(self, r, mu, monitor=None, noise=None):
        """synth_ddpg_step for actors with a camera, in the same launch: r also holds hist uint8 [n, Hd, C, H, W] (the
        raw frames, the current step's in slot hist_pos), obs_pixel uint8 [n, S*C, H, W] (receives the stacked
        observation of the next step) and the ring tables 'pixel' / 'pixel_next' uint8 [capacity, S*C*H*W]
        (include/surreal_amd.h smx_synth_ddpg_pixel_step)"""
        p = L.DdpgPixelStep()
        self._camera_args(p, r, 1)
        p.base = self._ddpg_args(r, 1, monitor=monitor, noise=noise)
        L.call('smx_synth_ddpg_pixel_step', ctypes.byref(p), L.ptr(mu), _row_stride(mu, mu.shape[1]), self._st())

    def synth_ddpg_pixel_pool_step(self, r, mu, monitor=None, noise=None):
        """synth_ddpg_pixel_step in the frame-pool layout (include/surreal_amd.h smx_synth_ddpg_pixel_pool_step): r holds,
        in place of hist / hist_pos, pool uint8 [n, P, F] with frame (the counter of the current step's frame) and
        episode_first (that of the episode's reset frame), and the ring's counter columns frame_next / frame_first int64
        [capacity], frame_actor int32 [capacity]; obs_pixel uint8 [n, S*C, H, W] as there.  The ring tables hold no
        'pixel' / 'pixel_next'"""
        pool, obs = r['pool'], r['obs_pixel']
        n, P, F = pool.shape
        C, H, W = r['frame_shape']
        S = obs.shape[1] // C
        cap = r['tables']['obs'].shape[0]
        assert C * H * W == F and tuple(obs.shape) == (n, S * C, H, W) and r['state'].shape[0] == n
        for k in (pool, obs):
            assert k.dtype == torch.uint8 and k.is_contiguous()
        for k, dt in (('frame_next', torch.int64), ('frame_first', torch.int64), ('frame_actor', torch.int32)):
            assert r[k].dtype == dt and r[k].is_contiguous() and r[k].numel() == cap, k
        p = L.DdpgPixelPoolStep()
        p.base = self._ddpg_args(r, 1, monitor=monitor, noise=noise)
        p.C, p.H, p.W, p.frame_stacks = C, H, W, S
        p.pool_len, p.frame, p.episode_first = P, int(r['frame']), int(r['episode_first'])
        p.pool, p.obs_pixel = L.ptr(pool), L.ptr(obs)
        p.frame_next, p.frame_first, p.frame_actor = L.ptr(r['frame_next']), L.ptr(r['frame_first']), \
            L.ptr(r['frame_actor'])
        L.call('smx_synth_ddpg_pixel_pool_step', ctypes.byref(p), L.ptr(mu), _row_stride(mu, mu.shape[1]), self._st())

    @staticmethod
    def synth_ppo_pixel_window_step_supported(A):
        """the actions smx_synth_ppo_pixel_window_step takes (one thread each, A <= SMX_PPO_PIXEL_STEP_MAX_A)"""
        return 0 < A <= L.SMX_PPO_PIXEL_STEP_MAX_A

    def synth_ppo_pixel_window_step(self, r, mu, copy_workgroups=0, monitor=None, noise=None):
        """ONE step of the windowed PPO rollout for actors with a camera given the policy mean mu [n, A] (row-strided
        view allowed): head, environment step, carry rings, frame history and -- at a closing step -- the windows into
        the FIFO's ring from row r['cursor'] (include/surreal_amd.h smx_synth_ppo_pixel_window_step).  r: state /
        init_state [n, D], t, episode_len, n_step, advance, log_var [A], noise_scale [n] or None, eps [n, A] or None,
        h_before / c_before [n, Hl] or None, carry {'obs', 'actions', 'rewards', 'pds' (, 'cells')}, tables (the ring by
        replay field name, 'pixel' [capacity, n_step * S*C*H*W] and 'pixel_next' [capacity, S*C*H*W] uint8 among
        them), cursor, hist uint8 [n, Hd, C, H, W] (the current step's frame in slot hist_pos), obs_pixel uint8
        [n, S*C, H, W] (receives the stacked observation of the next step)"""
        n, D, A = r['state'].shape[0], r['state'].shape[1], mu.shape[1]
        tabs, carry = r['tables'], r['carry']
        N = int(r['n_step'])
        cap = tabs['obs'].shape[0]
        p = L.SynthPpoPixelWindowStep()
        self._camera_args(p, r, N)
        for k, x in list(carry.items()) + [(k, x) for k, x in tabs.items() if k not in ('pixel', 'pixel_next')]:
            assert x.is_contiguous() and x.dtype == torch.float32, k
        assert tuple(tabs['obs'].shape) == (cap, N * D) and tuple(carry['obs'].shape) == (n, N, D)
        hb, cb = r.get('h_before'), r.get('c_before')
        Hl = 0
        if 'cells' in carry:
            Hl = carry['cells'].shape[-1]
            assert tuple(carry['cells'].shape) == (n, -(-N // int(r['advance'])), 2, Hl)
            for x in (hb, cb):
                assert x is None or (x.is_contiguous() and x.numel() == n * Hl)
            assert 'cells' not in tabs or tabs['cells'].shape[1] == 2 * Hl
        if r.get('eps') is not None:
            assert r['eps'].is_contiguous() and tuple(r['eps'].shape) == (n, A)
        p.n, p.D, p.A, p.hidden = n, D, A, Hl
        p.t, p.episode_len = int(r['t']), int(r['episode_len'])
        p.log_var, p.noise_scale, p.eps = L.ptr(r['log_var']), L.ptr(r.get('noise_scale')), L.ptr(r.get('eps'))
        p.state, p.init_state = L.ptr(r['state']), L.ptr(r['init_state'])
        p.h_before, p.c_before = L.ptr(hb), L.ptr(cb)
        self._window_args(p, N, r['advance'], carry, tabs, r['cursor'])
        p.copy_workgroups = int(copy_workgroups)
        p.mon = self._monitor_args(monitor, n)
        p.noise = self._noise_args(noise)
        L.call('smx_synth_ppo_pixel_window_step', ctypes.byref(p), L.ptr(mu), _row_stride(mu, A), self._st())

    @staticmethod
    def _record_step_args(p, r, N):
        """checks and fills what the two record launches share: the clocks and ranks (device int32 [n], and the host
        arrays they were copied from), cur_obs [n, D], the step's results, the cursor -> (n, D, A, tables, capacity)"""
        n, D = r['cur_obs'].shape
        A = r['actions'].shape[1]
        tabs = r['tables']
        cap = tabs['obs'].shape[0]
        for k in ('t', 'rank'):
            assert r[k].dtype == torch.int32 and r[k].is_contiguous() and r[k].numel() == n, k
            h = r.get(k + '_host')
            assert h is None or (h.dtype == np.int32 and h.flags['C_CONTIGUOUS'] and h.size == n), k
            setattr(p, k, L.ptr(r[k]))
            setattr(p, k + '_host', None if h is None else ctypes.c_void_p(h.ctypes.data))
        for k, w in (('cur_obs', D), ('actions', A), ('obs_next', D), ('rewards', 1), ('dones', 1), ('obs_reset', D)):
            x = r.get(k)
            assert k == 'obs_reset' or x is not None, k
            assert x is None or (x.dtype == torch.float32 and x.is_contiguous() and x.numel() == n * w), k
        for k, x in tabs.items():
            assert x.is_contiguous() and x.shape[0] == cap, k
            assert x.dtype == (torch.uint8 if k in ('pixel', 'pixel_next') else torch.float32), k
        assert tabs['obs'].shape[1] == N * D and tabs['obs_next'].shape[1] == D and tabs['actions'].shape[1] == N * A
        assert tabs['rewards'].shape[1] == N and tabs['dones'].shape[1] == N
        p.n, p.D, p.A, p.n_step, p.rows = n, D, A, N, int(r['rows'])
        p.cur_obs, p.step_actions, p.step_obs_next = L.ptr(r['cur_obs']), L.ptr(r['actions']), L.ptr(r['obs_next'])
        p.step_rewards, p.step_dones, p.step_obs_reset = L.ptr(r['rewards']), L.ptr(r['dones']), L.ptr(r.get('obs_reset'))
        p.cursor, p.capacity = int(r['cursor']), cap
        return n, D, A, tabs, cap

    def _record_ppo_args(self, p, r, copy_workgroups, monitor):
        """checks and fills a PPO record launch's argument struct `p` (either entry point) from r"""
        N = int(r['n_step'])
        n, D, A, tabs, cap = self._record_step_args(p, r, N)
        carry = r['carry']
        for k, x in carry.items():
            assert x.is_contiguous() and x.dtype == torch.float32, k
        assert tuple(carry['obs'].shape) == (n, N, D) and tuple(carry['actions'].shape) == (n, N, A)
        assert tuple(carry['rewards'].shape) == (n, N) and tuple(carry['pds'].shape) == (n, N, 2 * A)
        assert r['pds'].is_contiguous() and r['pds'].dtype == torch.float32 and r['pds'].numel() == n * 2 * A
        assert tabs['pds'].shape[1] == N * 2 * A
        hb, cb = r.get('h_before'), r.get('c_before')
        Hl = 0
        if 'cells' in carry:
            Hl = carry['cells'].shape[-1]
            assert tuple(carry['cells'].shape) == (n, -(-N // int(r['advance'])), 2, Hl)
            for x in (hb, cb):
                assert x is None or (x.is_contiguous() and x.dtype == torch.float32 and x.numel() == n * Hl)
            assert 'cells' not in tabs or tabs['cells'].shape[1] == 2 * Hl
        else:
            assert hb is None and cb is None and 'cells' not in tabs
        p.hidden, p.step_pds, p.h_before, p.c_before = Hl, L.ptr(r['pds']), L.ptr(hb), L.ptr(cb)
        cursor = p.cursor
        self._window_args(p, N, r['advance'], carry, tabs, cursor)
        p.copy_workgroups = int(copy_workgroups)
        p.mon = self._monitor_args(monitor, n)

    def record_ppo_window_step(self, r, copy_workgroups=0, monitor=None):
        """ONE step of n host-stepped actors' moving windows, every actor on its own episode clock
        (include/surreal_amd.h smx_record_ppo_window_step_f32).  r: t / rank int32 [n] on the device (t_host / rank_host:
        the numpy arrays they were copied from, checked before the launch), rows (the closing actors), cur_obs [n, D]
        (in: acted on, out: the next acting observation), actions [n, A], pds [n, 2A], obs_next [n, D], rewards [n],
        dones [n] (0 / 1), obs_reset [n, D] or None, h_before / c_before [n, Hl] or None, n_step, advance, carry {'obs',
        'actions', 'rewards', 'pds' (, 'cells')}, tables (the FIFO's ring by replay field name), cursor"""
        p = L.RecordPpoWindowStep()
        self._record_ppo_args(p, r, copy_workgroups, monitor)
        L.call('smx_record_ppo_window_step_f32', ctypes.byref(p), self._st())

    def _record_ddpg_args(self, p, r, monitor):
        """checks and fills a DDPG record launch's argument struct `p` (either entry point) from r"""
        N = int(r['n_step'])
        n, D, A, tabs, cap = self._record_step_args(p, r, 1)
        carry = r['carry']
        for k, x in carry.items():
            assert x.is_contiguous() and x.dtype == torch.float32, k
        assert tuple(carry['obs'].shape) == (n, N, D) and tuple(carry['actions'].shape) == (n, N, A)
        assert tuple(carry['rewards'].shape) == (n, N)
        assert r['gpow'].dtype == torch.float64 and r['gpow'].is_contiguous() and r['gpow'].numel() == N
        p.n_step, p.gpow = N, L.ptr(r['gpow'])
        p.carry_obs, p.carry_act, p.carry_rew = L.ptr(carry['obs']), L.ptr(carry['actions']), L.ptr(carry['rewards'])
        p.obs, p.obs_next, p.actions = L.ptr(tabs['obs']), L.ptr(tabs['obs_next']), L.ptr(tabs['actions'])
        p.rewards, p.dones = L.ptr(tabs['rewards']), L.ptr(tabs['dones'])
        p.mon = self._monitor_args(monitor, n)

    def record_ddpg_nstep_step(self, r, monitor=None):
        """ONE step of n host-stepped actors' n-step transitions, every actor on its own episode clock
        (include/surreal_amd.h smx_record_ddpg_nstep_step_f32).  r: as record_ppo_window_step without pds, cells and
        advance; gpow [n_step] fp64 (gamma ** e), carry {'obs', 'actions', 'rewards'}, tables: the uniform replay's ring
        (obs / obs_next [capacity, D], actions [capacity, A], rewards / dones [capacity, 1])"""
        p = L.RecordDdpgNstepStep()
        self._record_ddpg_args(p, r, monitor)
        L.call('smx_record_ddpg_nstep_step_f32', ctypes.byref(p), self._st())

    def _record_camera_args(self, p, r, frames_per_row):
        """the camera block of a record launch: _camera_args' buffers (hist, hist_pos, obs_pixel, the 'pixel' /
        'pixel_next' tables) and the step's frames: frames_next uint8 [n, C, H, W], frames_reset the same or None"""
        self._camera_args(p, dict(r, state=r['cur_obs']), frames_per_row)
        n, C, H, W = r['hist'].shape[0], p.C, p.H, p.W
        for k in ('frames_next', 'frames_reset'):
            x = r.get(k)
            assert k == 'frames_reset' or x is not None, k
            assert x is None or (x.dtype == torch.uint8 and x.is_contiguous() and x.numel() == n * C * H * W), k
        p.step_frame_next, p.step_frame_reset = L.ptr(r['frames_next']), L.ptr(r.get('frames_reset'))

    def record_ppo_pixel_window_step(self, r, copy_workgroups=0, monitor=None):
        """record_ppo_window_step for actors with a camera, the frames in the same launch (include/surreal_amd.h
        smx_record_ppo_pixel_window_step).  r also holds hist uint8 [n, Hd, C, H, W] (actor a's current frame in slot
        hist_pos), hist_pos, obs_pixel uint8 [n, S*C, H, W] (receives the stacked observation of the next step),
        frames_next / frames_reset uint8 [n, C, H, W] (frames_reset None: no actor is done) and the ring tables 'pixel'
        [capacity, n_step * S*C*H*W] / 'pixel_next' [capacity, S*C*H*W] uint8.  copy_workgroups: the workgroups per
        actor that move frames"""
        p = L.RecordPpoPixelWindowStep()
        self._record_ppo_args(p, r, copy_workgroups, monitor)
        self._record_camera_args(p, r, int(r['n_step']))
        L.call('smx_record_ppo_pixel_window_step', ctypes.byref(p), self._st())

    def record_ddpg_pixel_nstep_step(self, r, copy_workgroups=0, monitor=None):
        """record_ddpg_nstep_step for actors with a camera (include/surreal_amd.h smx_record_ddpg_pixel_nstep_step): r
        as record_ppo_pixel_window_step's camera entries, tables 'pixel' / 'pixel_next' [capacity, S*C*H*W] uint8"""
        p = L.RecordDdpgPixelNstepStep()
        self._record_ddpg_args(p, r, monitor)
        self._record_camera_args(p, r, 1)
        p.copy_workgroups = int(copy_workgroups)
        L.call('smx_record_ddpg_pixel_nstep_step', ctypes.byref(p), self._st())

    def record_ddpg_pixel_pool_nstep_step(self, r, copy_workgroups=0, monitor=None):
        """record_ddpg_pixel_nstep_step in the frame-pool layout (include/surreal_amd.h
        smx_record_ddpg_pixel_pool_nstep_step): r holds, in place of hist / hist_pos and the 'pixel' / 'pixel_next'
        tables, pool uint8 [n, P, F], counters_in / counters_out int64 [2, n] (f | first before and after the step: two
        buffers) and the ring's frame_next / frame_first int64 [capacity], frame_actor int32 [capacity]"""
        p = L.RecordDdpgPixelPoolNstepStep()
        self._record_ddpg_args(p, r, monitor)
        pool, obs = r['pool'], r['obs_pixel']
        n, P, F = pool.shape
        C, H, W = r['frame_shape']
        S = obs.shape[1] // C
        cap = r['tables']['obs'].shape[0]
        assert C * H * W == F and tuple(obs.shape) == (n, S * C, H, W) and r['cur_obs'].shape[0] == n
        for x in (pool, obs):
            assert x.dtype == torch.uint8 and x.is_contiguous()
        for k, dt in (('frame_next', torch.int64), ('frame_first', torch.int64), ('frame_actor', torch.int32)):
            assert r[k].dtype == dt and r[k].is_contiguous() and r[k].numel() == cap, k
        for k in ('counters_in', 'counters_out'):
            assert r[k].dtype == torch.int64 and r[k].is_contiguous() and r[k].numel() == 2 * n, k
        for k in ('frames_next', 'frames_reset'):
            x = r.get(k)
            assert k == 'frames_reset' or x is not None, k
            assert x is None or (x.dtype == torch.uint8 and x.is_contiguous() and x.numel() == n * F), k
        p.C, p.H, p.W, p.frame_stacks, p.pool_len, p.copy_workgroups = C, H, W, S, P, int(copy_workgroups)
        p.step_frame_next, p.step_frame_reset = L.ptr(r['frames_next']), L.ptr(r.get('frames_reset'))
        p.pool, p.obs_pixel = L.ptr(pool), L.ptr(obs)
        p.counters_in, p.counters_out = L.ptr(r['counters_in']), L.ptr(r['counters_out'])
        p.frame_next, p.frame_first, p.frame_actor = L.ptr(r['frame_next']), L.ptr(r['frame_first']), \
            L.ptr(r['frame_actor'])
        L.call('smx_record_ddpg_pixel_pool_nstep_step', ctypes.byref(p), self._st())

    def synth_env_step(self, state, init_state, actions, t, episode_len, slot, obs_roll, act_roll,
                       rew_roll, done_roll, monitor=None, task='drift', resets=None):
        """one environment step of all actors on given actions [n, A]; task: the dynamics (env/tasks.py;
        smx_synth_task_env_step_f32); resets: a task env's reset stream (_reset_args;
        smx_synth_task_env_step_resets_f32) -- init_state is then not read"""
        n, D = state.shape
        A = actions.shape[1]
        T = obs_roll.shape[1] if obs_roll is not None else 1
        args = (L.ptr(state), L.ptr(init_state), L.ptr(actions), n, D, A,
                int(t), int(episode_len), int(slot), T, L.ptr(obs_roll), L.ptr(act_roll),
                L.ptr(rew_roll), L.ptr(done_roll),
                None if monitor is None else ctypes.byref(self._monitor_args(monitor, n)))
        assert resets is None or task != 'drift', "task 'drift' has no reset distribution"
        if task != 'drift':
            if resets is not None:
                L.call('smx_synth_task_env_step_resets_f32', *args, self._task_id(task),
                       ctypes.byref(self._reset_args(resets)), self._st())
                return
            L.call('smx_synth_task_env_step_f32', *args, self._task_id(task), self._st())
            return
        L.call('smx_synth_env_step_f32', *args, self._st())


    # ---- generic dense layer + DDPG pieces ---------------------------------------------------
    def linear(self, A, a_kc, B, b_kc, bias, C, M, N, K, act=0, relu_mask=None, lda=None, ldb=None,
               ldc=None, stop=None):
        """C[M,N] = act(A . B^T + bias) with explicit leading strides (views into wider buffers)"""
        lda = lda if lda is not None else A.stride(0)
        ldb = ldb if ldb is not None else B.stride(0)
        ldc = ldc if ldc is not None else C.stride(0)
        L.call('smx_linear_f32', L.ptr(A), lda, int(a_kc), L.ptr(B), ldb, int(b_kc), L.ptr(bias),
               L.ptr(C), ldc, M, N, K, act, L.ptr(relu_mask), L.ptr(stop), self._st())

    def linear_multi(self, jobs):
        """independent dense problems in ONE launch (<= 9).  Each job is the argument tuple of ``linear``
        (``('linear', A, a_kc, B, b_kc, bias, C, M, N, K, {act, relu_mask, lda, ldb, ldc, stop})``) or of
        ``linear_wgrad`` (``('wgrad', dZ, X, dW, db, M, N, rows, {ldz, ldx, ldw})``)."""
        arr = (L.LinearJob * len(jobs))()
        for k, j in enumerate(jobs):
            kw = j[-1] if isinstance(j[-1], dict) else {}
            a = arr[k]
            if j[0] == 'wgrad':
                _, dZ, X, dW, db, M, N, rows = j[:8]
                a.kind, a.A, a.B, a.C, a.dbias = 1, L.ptr(dZ), L.ptr(X), L.ptr(dW), L.ptr(db)
                a.lda, a.ldb, a.ldc = kw.get('ldz') or dZ.stride(0), kw.get('ldx') or X.stride(0), kw.get('ldw') or dW.stride(0)
                a.M, a.N, a.K = M, N, rows
            else:
                _, A, a_kc, B, b_kc, bias, C, M, N, K = j[:10]
                a.kind, a.act = 0, int(kw.get('act', 0))
                a.A, a.B, a.bias, a.C, a.relu_mask = L.ptr(A), L.ptr(B), L.ptr(bias), L.ptr(C), L.ptr(kw.get('relu_mask'))
                a.lda, a.ldb, a.ldc = kw.get('lda') or A.stride(0), kw.get('ldb') or B.stride(0), kw.get('ldc') or C.stride(0)
                a.a_kcontig, a.b_kcontig, a.M, a.N, a.K = int(a_kc), int(b_kc), M, N, K
                a.stop_flag = L.ptr(kw.get('stop'))
        L.call('smx_linear_multi_f32', arr, len(jobs), self._st())

    def linear_wgrad(self, dZ, X, dW, db, M, N, rows, ldz=None, ldx=None, ldw=None, ws=None):
        """ws: optional split-K workspace (>= linear_wgrad_ws_floats(M, N, rows) floats)"""
        ldz = ldz if ldz is not None else dZ.stride(0)
        ldx = ldx if ldx is not None else X.stride(0)
        ldw = ldw if ldw is not None else dW.stride(0)
        L.call('smx_linear_wgrad_splitk_f32', L.ptr(dZ), ldz, L.ptr(X), ldx, L.ptr(dW), ldw, L.ptr(db),
               M, N, rows, L.ptr(ws), 0 if ws is None else ws.numel(), self._st())

    def linear_wgrad_pair(self, dZ, X1, dW1, db1, X2, dW2, db2, rows, ws):
        """dW1 = dZ^T . X1, dW2 = dZ^T . X2 (+ column sums of dZ) -- one split-K launch where both run on the 32 x 32 kernel;
        ws >= linear_wgrad_ws_floats(M, N1, rows) + linear_wgrad_ws_floats(M, N2, rows) floats"""
        M, N1, N2 = dW1.shape[0], dW1.shape[1], dW2.shape[1]
        L.call('smx_linear_wgrad_splitk_pair_f32', L.ptr(dZ), dZ.stride(0), M, rows, L.ptr(X1), X1.stride(0), L.ptr(dW1),
               L.ptr(db1), N1, L.ptr(X2), X2.stride(0), L.ptr(dW2), L.ptr(db2), N2, L.ptr(ws),
               0 if ws is None else ws.numel(), self._st())

    def linear_wgrad_ws_floats(self, M, N, rows):
        return int(self.lib.smx_linear_wgrad_ws_floats(M, N, rows))

    def lstm_backward_ws_floats(self, net, B, T):
        return int(self.lib.smx_lstm_backward_ws_floats(net.D, net.H, B, T))

    def ddpg_critic_loss(self, q, q_next, rewards, dones, gamma_n, y, dz3):
        L.call('smx_ddpg_critic_loss_f32', L.ptr(q), L.ptr(q_next), L.ptr(rewards), L.ptr(dones),
               float(gamma_n), q.numel(), L.ptr(y), L.ptr(dz3), self._st())

    def tanh_backward(self, da, a, out):
        L.call('smx_tanh_backward_f32', L.ptr(da), L.ptr(a), a.numel(), L.ptr(out), self._st())

    def fill(self, x, value):
        L.call('smx_fill_f32', L.ptr(x), x.numel(), float(value), self._st())

    def adam_step(self, theta, grads, m, v, lr, step, weight_decay=0.0, clip_value=0.0):
        L.call('smx_adam_step_f32', L.ptr(theta), L.ptr(grads), L.ptr(m), L.ptr(v), theta.numel(),
               float(lr), int(step), float(weight_decay), float(clip_value), self._st())

    def soft_update(self, target, source, tau):
        L.call('smx_soft_update_f32', L.ptr(target), L.ptr(source), float(tau), target.numel(),
               self._st())

    def ddpg_critic_loss_step(self, q, q_next, rewards, dones, gamma_n, y, dz3, step):
        """ddpg_critic_loss + (step[0] += 1): the iteration's Adam step count, on the device"""
        L.call('smx_ddpg_critic_loss_step_f32', L.ptr(q), L.ptr(q_next), L.ptr(rewards), L.ptr(dones),
               float(gamma_n), q.numel(), L.ptr(y), L.ptr(dz3), L.ptr(step), self._st())

    def adam_step_dev(self, theta, grads, m, v, lr, step, weight_decay=0.0, clip_value=0.0):
        """adam_step with lr ([1] float tensor) and step ([1] int32 tensor) read on the device"""
        L.call('smx_adam_step_dev_f32', L.ptr(theta), L.ptr(grads), L.ptr(m), L.ptr(v), theta.numel(),
               L.ptr(lr), L.ptr(step), float(weight_decay), float(clip_value), self._st())

    def hard_update_every(self, target, source, step, interval):
        L.call('smx_hard_update_every_f32', L.ptr(target), L.ptr(source), target.numel(), L.ptr(step),
               int(interval), self._st())

    def ddpg_stats(self, q, y, rewards, actions, q_actor, stats):
        rows, A = actions.shape
        L.call('smx_ddpg_stats_f32', L.ptr(q), L.ptr(y), L.ptr(rewards), L.ptr(actions),
               _row_stride(actions, A), A, L.ptr(q_actor), rows, L.ptr(stats), self._st())


    # ---- one DDPG iteration on row blocks (smx_ddpg_rows.hip) -------------------------------------------
    def ddpg_rows_supported(self, D, A, H1, H2, c1, c2, rows=None):
        if rows is not None:
            return bool(self.lib.smx_ddpg_rows_supported_at(D, A, H1, H2, c1, c2, int(rows)))
        return bool(self.lib.smx_ddpg_rows_supported(D, A, H1, H2, c1, c2))

    def ddpg_rows_packed_floats(self, D, A, H1, H2, c1, c2):
        return int(self.lib.smx_ddpg_rows_packed_floats(D, A, H1, H2, c1, c2))

    def ddpg_rows_args(self, dims, nets, packed, io, gamma_n):
        """the argument block of the three launches below.  dims = (D, A, H1, H2, c1, c2); nets: {'actor' | 'critic' |
        'target_actor' | 'target_critic': {'W1', 'b1', ... 'b3'}} (views into the parameter buffers); packed: the
        fragment-order weight copy (ddpg_rows_packed_floats floats); io: the tensors smx_ddpg_rows_t names
        (include/surreal_amd.h).  Holds references to every tensor."""
        a = L.DdpgRows()
        a.D, a.A, a.H1, a.H2, a.c1, a.c2 = [int(v) for v in dims]
        a.rows = int(io['x'].shape[0])
        for name in ('actor', 'critic', 'target_actor', 'target_critic'):
            n = getattr(a, name)
            for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'):
                setattr(n, k, nets[name][k].data_ptr())
        a.packed = packed.data_ptr()
        a.gamma_n = float(gamma_n)
        for k in ('x', 'x_next', 'actions', 'rewards', 'dones', 'xcat', 'h2c', 'q', 'q_next', 'y', 'dz3', 'dz2', 'dxcat',
                  'h1a', 'h2a', 'act', 'q_actor', 'dz3a', 'dz2a', 'dz1a', 'step'):
            t = io.get(k)
            assert t is None or t.is_contiguous(), k
            setattr(a, k, None if t is None else t.data_ptr())
        a._refs = (nets, packed, io)
        return a

    def ddpg_rows_pack(self, args, critic_only=False):
        L.call('smx_ddpg_rows_pack_f32', ctypes.byref(args), 1 if critic_only else 0, self._st())

    def ddpg_rows_critic(self, args):
        L.call('smx_ddpg_rows_critic_f32', ctypes.byref(args), self._st())

    def ddpg_rows_actor(self, args):
        L.call('smx_ddpg_rows_actor_f32', ctypes.byref(args), self._st())

    # TD3: the second critic rides in args.second (smx_ddpg_rows_second); the single-critic calls around it are unchanged
    def ddpg_rows_second_supported(self, D, A, H1, H2, c1, c2, rows):
        return bool(self.lib.smx_ddpg_rows_second_supported(D, A, H1, H2, c1, c2, int(rows)))

    def ddpg_rows_second_packed_floats(self, D, A, H1, H2, c1, c2):
        return int(self.lib.smx_ddpg_rows_second_packed_floats(D, A, H1, H2, c1, c2))

    def ddpg_rows_second(self, args, nets2, packed2, io2):
        """attach the second critic to a ddpg_rows_args block.  nets2: {'critic2' | 'target_critic2': {'W1' ... 'b3'}};
        packed2: ddpg_rows_second_packed_floats floats; io2: noise (or None), xcat2, h2c2, q2, q_next2, dz3_2, dz2_2, dxcat2,
        stats2 (or None).  Returns args."""
        s = L.DdpgRowsSecond()
        for name in ('critic2', 'target_critic2'):
            n = getattr(s, name)
            for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'):
                setattr(n, k, nets2[name][k].data_ptr())
        s.packed2 = packed2.data_ptr()
        for k in ('noise', 'xcat2', 'h2c2', 'q2', 'q_next2', 'dz3_2', 'dz2_2', 'dxcat2', 'stats2'):
            t = io2.get(k)
            assert t is None or t.is_contiguous(), k
            setattr(s, k, None if t is None else t.data_ptr())
        args.second = ctypes.pointer(s)
        args._refs2 = (s, nets2, packed2, io2)
        return args

    def ddpg_rows_pack_second(self, args):
        L.call('smx_ddpg_rows_pack_f32', ctypes.byref(args), 2, self._st())

    def ddpg_rows_critic_td3(self, args):
        L.call('smx_ddpg_rows_critic_td3_f32', ctypes.byref(args), self._st())

    # policy_delay > 1: the critic chains without the actor's forward pass (an iteration that leaves the actor and the
    # targets alone), and the one-workgroup launch in front of a delayed learner's actor step
    def ddpg_rows_critic_only(self, args):
        L.call('smx_ddpg_rows_critic_only_f32', ctypes.byref(args), self._st())

    def ddpg_rows_critic_only_td3(self, args):
        L.call('smx_ddpg_rows_critic_only_td3_f32', ctypes.byref(args), self._st())

    def ddpg_rows_delay_tail(self, args, actor_step, stats=None, stats_host=None):
        """smx_ddpg_rows_delay_tail_f32: the iteration's statistics (stats: args' q, y, rewards, actions, q_actor -> [7],
        second block to args.second.stats2; stats_host: the pinned mirror, slot *args.step & 1), then *actor_step += 1"""
        assert actor_step.dtype == torch.int32 and actor_step.numel() == 1
        assert stats_host is None or (stats is not None and stats_host.is_pinned() and stats_host.numel() >= 16)
        assert stats_host is None or not (bool(args.second) and args.second.contents.stats2) or stats_host.numel() >= 32
        L.call('smx_ddpg_rows_delay_tail_f32', ctypes.byref(args), actor_step.data_ptr(),
               None if stats is None else stats.data_ptr(), None if stats_host is None else stats_host.data_ptr(), self._st())

    # use_layernorm: the four networks' gains and biases and the extra buffers ride in args.ln (smx_ddpg_rows_ln); the
    # chain launches and the gradient-and-step launch around it honour it, the other entries refuse it
    def ddpg_rows_ln_supported(self, D, A, H1, H2, c1, c2, rows):
        return bool(self.lib.smx_ddpg_rows_ln_supported(D, A, H1, H2, c1, c2, int(rows)))

    def ddpg_rows_ln_attach(self, args, ln_nets, eps, io_ln):
        """attach the LayerNorms to a ddpg_rows_args block.  ln_nets: {'actor' | 'critic' | 'target_actor' | 'target_critic':
        {'ln1.W', 'ln1.b', 'ln2.W', 'ln2.b'}} (views into the parameter buffers); io_ln: c_a1, cm1, cr1, c_a2, cm2, cr2, dn2,
        dz1c, a1, am1, ar1, a2, am2, ar2, dn2a, dn1a.  The block's xcat[:, :c1], h2c, h1a, h2a are then the LayerNorm
        OUTPUTS (include/surreal_amd.h).  Returns args."""
        s = L.DdpgRowsLn()
        for name in ('actor', 'critic', 'target_actor', 'target_critic'):
            n = getattr(s, name)
            for k, f in (('ln1.W', 'g1'), ('ln1.b', 'b1'), ('ln2.W', 'g2'), ('ln2.b', 'b2')):
                setattr(n, f, ln_nets[name][k].data_ptr())
        s.eps = float(eps)
        for k in ('c_a1', 'cm1', 'cr1', 'c_a2', 'cm2', 'cr2', 'dn2', 'dz1c', 'a1', 'am1', 'ar1', 'a2', 'am2', 'ar2', 'dn2a',
                  'dn1a'):
            t = io_ln[k]
            assert t.is_contiguous(), k
            setattr(s, k, t.data_ptr())
        args.ln = ctypes.pointer(s)
        args._refs_ln = (s, ln_nets, io_ln)
        return args

    # use_layernorm with TD3: the second critic's LayerNorms and buffers ride in args.ln.second
    # (smx_ddpg_rows_ln_second), beside args.second; ddpg_rows_critic_td3 then runs the LayerNorm TD3 chain
    def ddpg_rows_ln_second_supported(self, D, A, H1, H2, c1, c2, rows):
        return bool(self.lib.smx_ddpg_rows_ln_second_supported(D, A, H1, H2, c1, c2, int(rows)))

    def ddpg_rows_ln_second_attach(self, args, ln_nets2, io_ln2):
        """attach the second critic's LayerNorm part to a block that ddpg_rows_ln_attach and ddpg_rows_second have been
        through.  ln_nets2: {'critic2' | 'target_critic2': {'ln1.W', 'ln1.b', 'ln2.W', 'ln2.b'}}; io_ln2: c2_a1, c2m1, c2r1,
        c2_a2, c2m2, c2r2, dn2_2, dz1c2.  The block's xcat2[:, :c1] and h2c2 are then the LayerNorm OUTPUTS.  Returns args."""
        assert bool(args.ln) and bool(args.second)
        s = L.DdpgRowsLnSecond()
        for name in ('critic2', 'target_critic2'):
            n = getattr(s, name)
            for k, f in (('ln1.W', 'g1'), ('ln1.b', 'b1'), ('ln2.W', 'g2'), ('ln2.b', 'b2')):
                setattr(n, f, ln_nets2[name][k].data_ptr())
        for k in ('c2_a1', 'c2m1', 'c2r1', 'c2_a2', 'c2m2', 'c2r2', 'dn2_2', 'dz1c2'):
            t = io_ln2[k]
            assert t.is_contiguous(), k
            setattr(s, k, t.data_ptr())
        args.ln.contents.second = ctypes.pointer(s)
        args._refs_ln2 = (s, ln_nets2, io_ln2)
        return args

    def ddpg_rows_update(self, args, group, theta, grads, exp_avg, exp_avg_sq, lr, step, weight_decay, clip_value,
                         target=None, tau=0.0, interval=0, wgrad=False, stats=None, stats_host=None):
        """smx_ddpg_rows_update_f32 (wgrad: smx_ddpg_rows_wgrad_update_f32, which forms the gradients first): Adam on the group ('actor' | 'critic' | 'critic2', TD3's second), its target network's update (soft with tau,
        or hard every `interval` iterations of *step; target None: none) and the fragment-order copies of both"""
        u = L.DdpgUpdate()
        u.theta, u.grads, u.exp_avg, u.exp_avg_sq = (t.data_ptr() for t in (theta, grads, exp_avg, exp_avg_sq))
        u.target = None if target is None else target.data_ptr()
        u.n = theta.numel()
        assert grads.numel() == u.n and exp_avg.numel() == u.n and exp_avg_sq.numel() == u.n
        assert target is None or target.numel() == u.n
        u.lr, u.step = lr.data_ptr(), step.data_ptr()
        assert stats is None or wgrad
        u.stats = None if stats is None else stats.data_ptr()
        assert stats_host is None or (stats is not None and stats_host.is_pinned() and stats_host.numel() >= 16)
        # (a second statistics block doubles the slots: include/surreal_amd.h)
        assert stats_host is None or not (bool(args.second) and args.second.contents.stats2) or stats_host.numel() >= 32
        u.stats_host = None if stats_host is None else stats_host.data_ptr()
        u.weight_decay, u.clip_value, u.tau, u.interval = float(weight_decay or 0.0), float(clip_value or 0.0), float(tau), int(interval)
        L.call('smx_ddpg_rows_wgrad_update_f32' if wgrad else 'smx_ddpg_rows_update_f32', ctypes.byref(args),
               {'actor': 0, 'critic': 1, 'critic2': 2}[group], ctypes.byref(u), self._st())


    # ---- LSTM stem ----------------------------------------------------------------------------
    def lstm_forward(self, net, x, B, T, h0, c0, gates, out, cs, hprev=None, hN=None, cN=None,
                     stop=None):
        """net: model.ppo_net.LstmParams; x [B*T, D] contiguous; see smx_lstm_forward_f32"""
        L.call('smx_lstm_forward_f32', ctypes.byref(net.desc), L.ptr(x), B, T, L.ptr(h0), L.ptr(c0),
               L.ptr(gates), L.ptr(out), L.ptr(cs), L.ptr(hprev), L.ptr(hN), L.ptr(cN), L.ptr(stop),
               self._st())

    def lstm_backward(self, net, x, B, T, c0, gates, cs, hprev, dout, dgates, grads, stop=None,
                      ws=None):
        L.call('smx_lstm_backward_f32', ctypes.byref(net.desc), L.ptr(x), B, T, L.ptr(c0),
               L.ptr(gates), L.ptr(cs), L.ptr(hprev), L.ptr(dout), L.ptr(dgates), L.ptr(grads),
               L.ptr(stop), L.ptr(ws), 0 if ws is None else ws.numel(), self._st())


    # ---- CNN stem data movement ----------------------------------------------------------------
    def im2col(self, src, F, C, Hin, Win, k, stride, cols, channel_last=False, scale_div=0.0):
        """src: uint8 / fp32 frames [F, C, Hin, Win] or (channel_last) fp32 [F, Hin*Win, C]"""
        L.call('smx_im2col_f32', L.ptr(src), int(src.dtype == torch.uint8), int(channel_last), F, C,
               Hin, Win, k, k, stride, float(scale_div), L.ptr(cols), self._st())

    @staticmethod
    def conv_u8_supported(frames, C, Hin, Win, k, stride, cout, W=None):
        """shapes smx_conv_u8_forward_f32 takes (the implicit-GEMM first convolution over uint8 frames); `W`:
        the layer's weight, a view into the flat parameter buffer whose 16-byte alignment depends on its offset"""
        K = C * k * k
        return frames.dtype == torch.uint8 and cout <= 16 and k % 4 == 0 and Win % 4 == 0 and stride % 4 == 0 \
            and K % 64 == 0 and K <= 256 and frames.data_ptr() % 4 == 0 and (W is None or W.data_ptr() % 16 == 0)

    def conv_u8_forward(self, frames, F, C, Hin, Win, k, stride, W, bias, cout, y, stop=None):
        """y [F*Ho*Wo, cout] = relu(conv(frames / 255, W) + bias), no patch matrix (see the header)"""
        L.call('smx_conv_u8_forward_f32', L.ptr(frames), F, C, Hin, Win, k, stride, L.ptr(W), L.ptr(bias), cout,
               L.ptr(y), L.ptr(stop), self._st())

    def conv_u8_wgrad_ws_floats(self, cout, K):
        return int(self.lib.smx_conv_u8_wgrad_ws_floats(cout, K))

    def conv_u8_wgrad(self, frames, F, C, Hin, Win, k, stride, dy, cout, dW, db, ws, stop=None):
        """dW [cout, C*k*k] (torch's Conv2d.weight order), db [cout] from dy [F*Ho*Wo, cout] and the uint8 frames"""
        L.call('smx_conv_u8_wgrad_f32', L.ptr(frames), F, C, Hin, Win, k, stride, L.ptr(dy), cout, L.ptr(dW), L.ptr(db),
               L.ptr(ws), ws.numel(), L.ptr(stop), self._st())

    @staticmethod
    def conv_cl_supported(src, C, k, cout):
        """shapes smx_conv_cl_forward_f32 / _wgrad_f32 take (implicit GEMMs over a 16-channel channel-last source)"""
        return src.dtype == torch.float32 and C == 16 and cout <= 32 and k in (2, 3, 4) and src.data_ptr() % 16 == 0

    def conv_cl_forward(self, src, F, C, Hin, Win, k, stride, W, bias, cout, y, stop=None):
        L.call('smx_conv_cl_forward_f32', L.ptr(src), F, C, Hin, Win, k, stride, L.ptr(W), L.ptr(bias), cout, L.ptr(y),
               L.ptr(stop), self._st())

    def conv_cl_wgrad_ws_floats(self, cout, k):
        return int(self.lib.smx_conv_cl_wgrad_ws_floats(cout, k))

    def conv_cl_wgrad(self, src, F, C, Hin, Win, k, stride, dy, cout, dW, db, ws, stop=None):
        L.call('smx_conv_cl_wgrad_f32', L.ptr(src), F, C, Hin, Win, k, stride, L.ptr(dy), cout, L.ptr(dW), L.ptr(db),
               L.ptr(ws), ws.numel(), L.ptr(stop), self._st())

    @staticmethod
    def conv_cl_dgrad_supported(dy, C, k, stride, cout):
        return C == 16 and cout <= 32 and k == 2 * stride and dy.data_ptr() % 16 == 0

    def conv_cl_dgrad(self, dy, F, C, Hin, Win, k, stride, W, cout, relu_of, dx, stop=None):
        """dx [F*Hin*Win, 16] = relu'(relu_of) * conv_transpose(dy [F*Ho*Wo, cout], W [cout, 16, k, k])"""
        L.call('smx_conv_cl_dgrad_f32', L.ptr(dy), F, C, Hin, Win, k, stride, L.ptr(W), cout, L.ptr(relu_of), L.ptr(dx),
               L.ptr(stop), self._st())

    def col2im(self, dcols, F, C, Hin, Win, k, stride, relu_of, dx):
        L.call('smx_col2im_f32', L.ptr(dcols), F, C, Hin, Win, k, k, stride, L.ptr(relu_of),
               L.ptr(dx), self._st())

    def flatten_order(self, src, O, C, P, to_channel_last, out):
        L.call('smx_flatten_order_f32', L.ptr(src), O, C, P, int(to_channel_last), L.ptr(out),
               self._st())


# ------------------------------------------------------------------------------------------
# process-wide default.  The product default is HipKernels on 'cuda' and nothing in
# surreal_amd/ ever installs anything else; tests/ install a CPU test double to exercise
# the host logic (sharding, epoch control, stats) without a GPU.
# ------------------------------------------------------------------------------------------
_default = {'kernels': None, 'device': 'cuda'}


def default_kernels():
    if _default['kernels'] is None:
        _default['kernels'] = HipKernels()   # raises without the .so or without a GPU
    return _default['kernels']


def default_device():
    return _default['device']


def set_default_kernels(kernels, device):
    """test hook: returns the previous (kernels, device) so it can be restored"""
    prev = (_default['kernels'], _default['device'])
    _default['kernels'], _default['device'] = kernels, device
    return prev
