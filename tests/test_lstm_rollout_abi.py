"""CPU tier: struct smx_synth_lstm_rollout as gcc lays it out (include/surreal_amd.h) against its ctypes mirror, and
the host-side shape rules of its entry points (no GPU needed)."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _offsets(tmp_path, cname, cls):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "surreal_amd.h"', 'int main(void) {',
             '  printf("sizeof %%zu\\n", sizeof(%s));' % cname]
    for fname, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(%s, %s));' % (fname, cname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}


def test_lstm_rollout_struct_matches_the_ctypes_mirror(tmp_path):
    from surreal_amd import _lib as L
    got = _offsets(tmp_path, 'struct smx_synth_lstm_rollout', L.SynthLstmRollout)
    assert got['sizeof'] == ctypes.sizeof(L.SynthLstmRollout)
    for fname, _ in L.SynthLstmRollout._fields_:
        assert got[fname] == getattr(L.SynthLstmRollout, fname).offset, fname
    assert got['roll'] == 0 and ctypes.sizeof(L.SynthRollout) <= got['lstm']


def test_lstm_rollout_shape_rules():
    from surreal_amd import _lib as L
    lib = L.load()
    ok = lib.smx_synth_lstm_rollout_supported
    assert ok(376, 100, 300, 200, 17) and ok(17, 100, 300, 200, 6) and ok(7, 12, 24, 16, 3)
    assert not ok(17, 10, 300, 200, 6)          # units padded to 4 by the model
    assert not ok(17, 132, 300, 200, 6)         # H <= 128
    assert not ok(17, 100, 300, 200, 33)        # A <= 32
    assert not ok(1024, 128, 640, 640, 17)      # past the LDS of a 16-actor block
    # [4H, Dp + H] in fragment order (tiles of 16 rows, K chunks of 32 rounded up to an even count) + the biases
    assert lib.smx_lstm_rollout_packed_floats(376, 100) == 25 * 16 * 512 + 400
    assert lib.smx_lstm_rollout_packed_floats(17, 12) == 3 * 2 * 512 + 48
    assert lib.smx_lstm_rollout_packed_floats(17, 10) == 0
