"""
What the learners share of the distributed plumbing: the counting wrapper around ``torch.distributed`` with its
hook for graph segments, the segmented graph itself, and the collective set-up of the peer-buffer exchange.
"""
import torch


class _SegmentedGraph(object):
    """A learn() on several ranks as hipGraph SEGMENTS with the collectives issued between them: the
    kernels (and the few torch ops) between two collectives are captured once and replayed, RCCL is
    called eagerly on the same stream.  One learn of the benchmark is ~70 launches; issued one by
    one from Python they cost more host time than the GPU needs to run them, which a single-rank
    learner never pays (its whole step is one graph)."""

    def __init__(self):
        self.items = []
        self.pool = torch.cuda.graph_pool_handle()      # one pool: a segment's temporaries outlive it
        self._cur = None

    def _open(self):
        g = torch.cuda.CUDAGraph()
        # thread_local: the process group's watchdog thread queries events while we capture; under the
        # default (global) mode a HIP call from ANY thread invalidates the capture
        ctx = torch.cuda.graph(g, pool=self.pool, capture_error_mode='thread_local')
        ctx.__enter__()
        self._cur = (g, ctx)

    def _close(self):
        g, ctx = self._cur
        ctx.__exit__(None, None, None)
        self.items.append(g)
        self._cur = None

    def capture(self, fn, dist_proxy):
        dist_proxy.recorder = self
        self._open()
        try:
            fn()
        finally:
            self._close()
            dist_proxy.recorder = None

    def collective(self, thunk):
        """called by the distributed proxy while capturing: cut the graph here (the collective is NOT
        executed during the capture pass -- the kernels around it are not either)"""
        self._close()
        self.items.append(thunk)
        self._open()

    def replay(self):
        for it in self.items:
            if isinstance(it, torch.cuda.CUDAGraph):
                it.replay()
            else:
                it()


class _CountingDist(object):
    """torch.distributed with a counter on the collectives a learn() issues (reported by bench.py), a hook
    for _SegmentedGraph, and -- when the ranks share a node -- the fp32 exchanges routed through
    surreal_amd.distributed.PeerExchange (one kernel on the learner's stream, part of its graph) instead of
    the process group (an eager RCCL call that cuts the graph)."""

    def __init__(self, dist):
        self._d = dist
        self.count = 0
        self.recorder = None
        self.exchange = None         # PeerExchange, once a workspace has set it up and checked it
        self.err_word = None         # device int32 a timed-out exchange raises (the learner's control block)

    def _run(self, name, a, k):
        def thunk():
            self.count += 1
            return getattr(self._d, name)(*a, **k)
        if self.recorder is not None:
            self.recorder.collective(thunk)
            return None
        return thunk()

    def _peer_ok(self, *tensors):
        ex = self.exchange
        return ex is not None and all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and
                                      t.numel() <= ex.capacity and t.data_ptr() % 16 == 0 for t in tensors)

    def all_reduce(self, t, *a, **k):
        if not a and not k and self._peer_ok(t):
            self.count += 1
            return self.exchange.all_reduce(t, err=self.err_word)
        return self._run('all_reduce', (t,) + a, k)

    def all_gather_into_tensor(self, out, t, *a, **k):
        if not a and not k and self._peer_ok(out, t):
            self.count += 1
            return self.exchange.all_gather_into_tensor(out, t, err=self.err_word)
        return self._run('all_gather_into_tensor', (out, t) + a, k)

    def kind(self):
        """what the fp32 exchanges run on (the learners report it as exchange_kind)"""
        return 'peer buffers (%s)' % self.exchange.check_message if self.exchange is not None else 'process group'

    def __getattr__(self, name):
        return getattr(self._d, name)


def _dist_info():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return _CountingDist(dist), dist.get_world_size(), dist.get_rank()
    return None, 1, 0


def setup_peer_exchange(learner, err_word, need):
    """several ranks on one node: the fp32 exchanges of a learn() as kernels over IPC-mapped peer buffers
    (surreal_amd.distributed.PeerExchange) -- set up and SELF-CHECKED once, collectively; any failure leaves
    the process group (RCCL) in place.  session_config.learner.peer_exchange = False keeps RCCL.  An exchange too
    small for `need` floats is closed (behind a barrier) and created again.  True when an exchange was created or
    attempted here."""
    d = learner._dist
    d.err_word = err_word
    lcfg = learner.session_config.learner
    want = bool(lcfg.get('peer_exchange', True)) and learner.device != 'cpu'
    if not want or (d.exchange is not None and d.exchange.capacity >= need):
        return False
    if d.exchange is not None:
        d._d.barrier()
        d.exchange.close()
        d.exchange = None
    from surreal_amd.distributed.peer_exchange import PeerExchange
    d.exchange = PeerExchange.create(d._d, need, timeout_s=float(lcfg.get('peer_exchange_timeout_s', 5.0)))
    return True
