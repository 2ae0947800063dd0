"""
Replay plugin base class: the constructor signature, abstract methods and counters of the
reference's ``surreal.replay.base.Replay`` (surreal/replay/base.py:9-256) without its ZeroMQ
servers.  The reference runs a collector thread (agents PUSH pyarrow blobs) and a sampler
thread (learner REQ -> ``sample`` -> pyarrow blob); here agents and the learner live in the same
process (one per GPU) and call ``insert`` / ``sample`` directly, so ``start_threads`` / ``join``
are no-ops kept for call-site compatibility.

Two storage tiers behind the same object:
  * host tier  -- ``insert(exp_dict)`` / ``sample(batch_size) -> list[exp]``: exactly the
    reference's Python semantics (what external, CPU-simulator agents use);
  * device tier -- ``insert_batch(fields)`` / ``sample_batch(batch_size)``: experience fields as
    struct-of-arrays tables in HBM moved by the ring-insert / row-gather HIP kernels
    (csrc/smx_replay.hip); what GPU-resident rollouts use, and what the benchmark path feeds
    the learner from without ever touching the host.
"""
import time

import torch

from surreal_amd import kernels as KN


def table_dtype(dtype):
    """element type a field is stored with: uint8 (camera frames, `pixel_input`) stays uint8 -- a quarter of the
    HBM and copy bytes of an fp32 widening, and what the CNN stem's im2col reads anyway; every other field
    (observations, actions, rewards, dones, policy infos) is fp32 like the learner's batch contract"""
    return torch.uint8 if dtype == torch.uint8 else torch.float32


class DeviceTable(object):
    """one experience field: [capacity, width] rows in HBM, fp32 or uint8 (``table_dtype``)"""

    def __init__(self, capacity, shape, device, kernels, dtype=torch.float32):
        self.shape = tuple(shape)
        width = 1
        for s in self.shape:
            width *= int(s)
        self.width = width
        self.dtype = table_dtype(dtype)
        self.data = torch.zeros(capacity, width, device=device, dtype=self.dtype)
        self.K = kernels

    def insert(self, cursor, rows):
        self.K.ring_insert(self.data, cursor, rows.reshape(rows.shape[0], -1).to(self.dtype).contiguous())

    def gather(self, idx):
        out = torch.empty(idx.numel(), self.width, device=self.data.device, dtype=self.dtype)
        self.K.gather_rows(self.data, idx, out)
        return out.view((idx.numel(),) + self.shape)

    def rows(self, first, n):
        """the n consecutive rows from `first` as a VIEW of the table, in the field's shape"""
        return self.data[first:first + n].view((n,) + self.shape)


class Replay(object):
    def __init__(self, learner_config, env_config, session_config, index=0):
        self.learner_config = learner_config
        self.env_config = env_config
        self.session_config = session_config
        self.index = index
        self._evict_interval = session_config.replay.get('evict_interval', 0.0)
        self._setup_logging()
        # device tier (created lazily by insert_batch)
        self._tables = None
        self._dev_capacity = 0

    # ---- lifecycle: in-process, nothing to start -----------------------------------------
    def start_threads(self):
        pass

    def join(self):
        pass

    # ---- abstract (base.py:69-113) --------------------------------------------------------
    def insert(self, exp_dict):
        raise NotImplementedError

    def sample(self, batch_size):
        raise NotImplementedError

    def evict(self):
        pass

    def start_sample_condition(self):
        raise NotImplementedError

    def __len__(self):
        raise NotImplementedError

    # ---- counters / wrappers (base.py:115-171) ---------------------------------------------
    def _setup_logging(self):
        self.init_time = time.time()
        self.cumulative_collected_count = 0
        self.cumulative_sampled_count = 0
        self.cumulative_request_count = 0
        self.last_report_time = self.init_time

    def _insert_wrapper(self, exp):
        self.cumulative_collected_count += 1
        self.insert(exp)

    def _sample_request_handler(self, batch_size):
        """what the reference's sampler thread does per learner request (base.py:156-171),
        minus the 10 ms spin and the serialisation"""
        if not self.start_sample_condition():
            return None
        self.cumulative_sampled_count += batch_size
        self.cumulative_request_count += 1
        return self.sample(batch_size)

    def generate_tensorplex_report(self):
        now = time.time()
        dt = max(now - self.last_report_time, 1e-9)
        self.last_report_time = now
        return {
            'num_exps': len(self),
            'cumulative_exps': self.cumulative_collected_count,
            'cumulative_sampled': self.cumulative_sampled_count,
            'cumulative_requests': self.cumulative_request_count,
            'lifetime_experience_utilization_percent':
                self.cumulative_sampled_count / max(self.cumulative_collected_count, 1) * 100,
            'report_interval_s': dt,
        }

    # ---- the device tier's state (utils/run_state.py) ----------------------------------------------
    _state_cursors = ()          # the subclass's cursor / count attributes, all ints

    def _state_capacity(self):
        """the rows of a device table of this replay"""
        raise NotImplementedError

    def _state_refusals(self, who):
        if getattr(self, 'frame_pool_on', False):
            raise NotImplementedError('%s: a frame-pool replay (replay.device_frame_pool): its pool and ledger are not '
                                      'carried' % who)
        if len(getattr(self, '_memory', ())):
            raise ValueError('%s: the host tier holds %d experiences; it is not carried (the device tier only)'
                             % (who, len(self._memory)))

    def state_dict(self):
        """the device tier: every table in full (the LIVE tensors: run_state.to_host / save_run make the host copy), the
        cursors and counts, the cumulative counters.  NotImplementedError for a frame-pool replay, ValueError while the
        host tier holds experiences (it is not carried)."""
        self._state_refusals('state_dict')
        tables = None
        if self._tables is not None:
            tables = {k: {'shape': list(t.shape), 'data': t.data} for k, t in self._tables.items()}
        return {'kind': type(self).__name__, 'memory_size': int(self.memory_size), 'tables': tables,
                'cursors': {k: int(getattr(self, k)) for k in self._state_cursors},
                'counters': {k: int(getattr(self, k)) for k in ('cumulative_collected_count', 'cumulative_sampled_count',
                                                                'cumulative_request_count')}}

    def load_state_dict(self, sd):
        """state_dict()'s, back.  Tables that exist are written in place (they keep their addresses: views and captured
        graphs stay valid); a replay that has none yet reserves them through reserve_ring with the saved shapes and
        dtypes.  ValueError -- before anything is written -- when the kind, memory_size, the fields, their shapes or
        dtypes differ or the host tier holds experiences; NotImplementedError for a frame-pool replay."""
        who = '%s.load_state_dict' % type(self).__name__
        self._state_refusals(who)
        if sd.get('kind') != type(self).__name__ or int(sd['memory_size']) != int(self.memory_size):
            raise ValueError('%s: the state is of a %s of memory_size %s, this is a %s of %d'
                             % (who, sd.get('kind'), sd.get('memory_size'), type(self).__name__, self.memory_size))
        if sorted(sd['cursors']) != sorted(self._state_cursors):
            raise ValueError('%s: the state holds the cursors %r, this replay %r'
                             % (who, sorted(sd['cursors']), sorted(self._state_cursors)))
        saved, cap = sd['tables'], self._state_capacity()
        for k, t in (saved or {}).items():
            width = int(torch.Size(t['shape']).numel())
            if tuple(t['data'].shape) != (cap, width) or t['data'].dtype != table_dtype(t['data'].dtype):
                raise ValueError('%s: the saved table %r is %s %s, a table of this replay has %d rows of %d'
                                 % (who, k, tuple(t['data'].shape), t['data'].dtype, cap, width))
        if self._tables is not None:
            mine = {k: (t.shape, t.dtype) for k, t in self._tables.items()}
            theirs = {k: (tuple(t['shape']), t['data'].dtype) for k, t in (saved or {}).items()}
            if mine != theirs:
                raise ValueError('%s: the saved fields %r do not match the replay tables %r' % (who, theirs, mine))
        elif saved:
            self.reserve_ring(0, {k: tuple(t['shape']) for k, t in saved.items()},
                              {k: t['data'].dtype for k, t in saved.items()})
        for k, t in (saved or {}).items():
            self._tables[k].data.copy_(t['data'])
        for k, v in sd['cursors'].items():
            setattr(self, k, int(v))
        for k, v in sd['counters'].items():
            setattr(self, k, int(v))

    # ---- device tier helpers ---------------------------------------------------------------
    def _ensure_tables(self, capacity, fields):
        if self._tables is None:
            K, dev = KN.default_kernels(), KN.default_device()
            self._tables = {name: DeviceTable(capacity, t.shape[1:], dev, K, t.dtype)
                            for name, t in fields.items()}
            self._dev_capacity = capacity
            self._K, self._dev = K, dev
        return self._tables
