"""
The state of a device-resident training run in ONE file: ``save_run(path, **parts)`` / ``load_run(path) -> dict``.

A part is what a holder of state hands out -- SyntheticVecEnv.state_dict(), PPOAgent / DDPGAgent.state_dict(),
FIFOReplay / UniformReplay.state_dict(), PPOLearner / DDPGLearner.train_state_dict() -- or anything else of the same
kind: a nested dict / list of tensors, ints, floats, bools, strings and None, and nothing else.  The holders hand out
their LIVE tensors (as torch's Module.state_dict does: no copy, no launch); ``to_host`` makes the host copy -- every
device tensor into a pinned buffer with an asynchronous copy, then ONE synchronisation -- and ``save_run`` is ``to_host``
of all parts, ``torch.save`` into a temporary file of the same directory, ``os.replace``: a save that fails leaves the
previous file as it was.  The file is read with ``torch.load(..., weights_only=True)``: it holds no code.

    save_run(path, env=venv.state_dict(), agent=agent.state_dict(), replay=replay.state_dict(),
             learner=learner.train_state_dict(), torch_rng=torch_rng_state())
    parts = load_run(path)
    learner.load_train_state_dict(parts['learner']); replay.load_state_dict(parts['replay']); ...

The optional part ``torch_rng`` (torch_rng_state / set_torch_rng_state) is for loops that draw their exploration noise
with torch.randn because no DeviceNoise is attached: the CPU generator's state and every device generator's.
"""
import os

import numpy as np
import torch

FORMAT = 'surreal_amd.run_state'
VERSION = 1


def _plain(x, path, device_copies):
    """x with every container a dict / list, every array a CPU tensor; device tensors are copied asynchronously into
    pinned buffers (listed in device_copies: the caller synchronises once)"""
    if isinstance(x, np.generic) and x.dtype.kind in 'biuf':          # (np.float64 is a float: before the plain types)
        return x.item()
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, np.ndarray):
        if x.dtype.kind not in 'biuf':
            raise TypeError('run_state: %s is a numpy array of dtype %s' % (path, x.dtype))
        return torch.from_numpy(np.array(x, copy=True, order='C'))
    if torch.is_tensor(x):
        x = x.detach()
        if x.device.type == 'cpu':
            return x.clone()
        host = torch.empty(x.shape, dtype=x.dtype, pin_memory=True)
        host.copy_(x, non_blocking=True)
        device_copies.append(host)
        return host
    if isinstance(x, dict):
        out = {}
        for k, v in x.items():
            if not isinstance(k, (str, int)) or isinstance(k, bool):
                raise TypeError('run_state: %s has the key %r; keys are strings or ints' % (path, k))
            out[k] = _plain(v, '%s[%r]' % (path, k), device_copies)
        return out
    if isinstance(x, (list, tuple)):
        return [_plain(v, '%s[%d]' % (path, i), device_copies) for i, v in enumerate(x)]
    raise TypeError('run_state: %s is a %s; a part holds dicts, lists, tensors, ints, floats, bools, strings and None'
                    % (path, type(x).__name__))


def to_host(part, name='part'):
    """a deep host copy of a part: containers as dict / list, numpy arrays as tensors, every device tensor copied to
    the host -- asynchronously, then one synchronisation; no launch"""
    copies = []
    out = _plain(part, name, copies)
    if copies:
        torch.cuda.synchronize()
    return out


def save_run(path, **parts):
    """writes the parts into `path`, atomically (a temporary file beside it, then os.replace); one synchronisation, at
    the device -> host copies, and no launch"""
    copies = []
    body = {name: _plain(part, name, copies) for name, part in parts.items()}
    if copies:
        torch.cuda.synchronize()
    blob = {'header': {'format': FORMAT, 'version': VERSION, 'parts': sorted(body)}, 'parts': body}
    path = os.fspath(path)
    tmp = '%s.tmp.%d' % (path, os.getpid())
    try:
        torch.save(blob, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def load_run(path):
    """-> {part name: part}, every tensor on the host.  ValueError for a file of another format or version"""
    blob = torch.load(os.fspath(path), map_location='cpu', weights_only=True)
    header = blob.get('header') if isinstance(blob, dict) else None
    if not isinstance(header, dict) or header.get('format') != FORMAT:
        raise ValueError('load_run: %s is not a run-state file' % (path,))
    if header.get('version') != VERSION:
        raise ValueError('load_run: %s has format version %r; this code reads version %d'
                         % (path, header.get('version'), VERSION))
    parts = blob.get('parts')
    if not isinstance(parts, dict) or sorted(parts) != list(header.get('parts', ())):
        raise ValueError('load_run: %s: the parts do not match the header %r' % (path, header.get('parts')))
    return parts


def torch_rng_state():
    """the part 'torch_rng': the CPU generator's state and, where a device is there, every device generator's"""
    return {'cpu': torch.get_rng_state(),
            'cuda': list(torch.cuda.get_rng_state_all()) if torch.cuda.is_available() else []}


def set_torch_rng_state(sd):
    torch.set_rng_state(sd['cpu'])
    if sd['cuda']:
        if not torch.cuda.is_available() or len(sd['cuda']) != torch.cuda.device_count():
            raise ValueError('torch_rng: the file holds %d device generators, this process has %d'
                             % (len(sd['cuda']), torch.cuda.device_count() if torch.cuda.is_available() else 0))
        torch.cuda.set_rng_state_all(list(sd['cuda']))


# ---- helpers of the holders' load_state_dict: check everything, then write ------------------------------------------------

def check_tensor(who, name, src, dst):
    """ValueError unless the saved tensor `src` fits the live tensor `dst` (shape and dtype)"""
    if not torch.is_tensor(src) or tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
        got = '%s %s' % (tuple(src.shape), src.dtype) if torch.is_tensor(src) else type(src).__name__
        raise ValueError('%s: the saved %s is %s, this one %s %s' % (who, name, got, tuple(dst.shape), dst.dtype))


def check_tensors(who, saved, live):
    """ValueError unless the dict `saved` holds exactly the tensors of the dict `live`, each of its shape and dtype"""
    if not isinstance(saved, dict) or sorted(saved) != sorted(live):
        raise ValueError('%s: the state holds %r, this object %r'
                         % (who, sorted(saved) if isinstance(saved, dict) else type(saved).__name__, sorted(live)))
    for k, dst in live.items():
        check_tensor(who, k, saved[k], dst)


def load_tensors(saved, live):
    for k, dst in live.items():
        dst.copy_(saved[k])


def model_tensors(model):
    """the LIVE tensors that are a model's whole state, by name: a PPOModel's one flat parameter buffer and its
    z-filter's sums; a DDPGModel's actor + critic buffer (a critic-only model's critic buffer) and its perception
    CNN's.  Whole buffers, the padding included: a copy of them is a copy of the model, bit for bit."""
    out = {}
    if getattr(model, 'flat', None) is not None:                       # PPOModel
        out['flat'] = model.flat
        if getattr(model, 'use_z_filter', False):
            zf = model.z_filter
            out.update({'z_filter.running_sum': zf.running_sum, 'z_filter.running_sumsq': zf.running_sumsq,
                        'z_filter.count': zf.count})
        return out
    if getattr(model, 'ac_flat', None) is not None:                    # DDPGModel
        out['ac_flat'] = model.ac_flat
    else:
        out['critic_flat'] = model.critic_flat
    if getattr(model, 'perception_flat', None) is not None:
        out['perception_flat'] = model.perception_flat
    return out
