"""CPU tier: struct smx_synth_lstm_rollout as gcc lays it out (include/surreal_amd.h) against its ctypes mirror, and
the host-side shape rules of its entry points (no GPU needed)."""
import ctypes

from helpers import _offsets


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
