"""Host-side pieces of streaming generation (no GPU): the push planner, the sample-release rule of both tail modes, the
prototypes of the stream entry points against the binding, and argument errors caught before any device work."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ready_mirror(frames_in, hop, pad, last):
    if last:
        return frames_in * hop
    r = (frames_in - pad) * hop
    return r // 32 * 32 if r > 0 else 0


@pytest.mark.parametrize('hop,pad', [(275, 2), (275, 0), (200, 3), (16, 2)])
def test_ready_steps_matches_the_planning_rule(hop, pad):
    from tacotronv2_wavernn_chinese_amd import _cabi
    prev = 0
    for frames_in in range(0, 60):
        got = _cabi.stream_ready_steps(frames_in, hop, pad, False)
        assert got == _ready_mirror(frames_in, hop, pad, False), frames_in
        assert got % 32 == 0 and got >= prev                        # resume points on Philox block boundaries, monotone
        assert got <= max(frames_in - pad, 0) * hop                 # never a step whose frame lacks its `pad` lookahead
        assert got > max(frames_in - pad, 0) * hop - 32             # ... and nothing ready is held back beyond the rounding
        assert _cabi.stream_ready_steps(frames_in, hop, pad, True) == frames_in * hop   # `last` releases everything
        prev = got


def test_ready_steps_rejects_bad_arguments():
    from tacotronv2_wavernn_chinese_amd import _cabi
    assert _cabi.stream_ready_steps(-1, 275, 2, False) == -1
    assert _cabi.stream_ready_steps(5, 0, 2, False) == -1
    assert _cabi.stream_ready_steps(5, 275, -1, True) == -1


def test_release_rule_of_both_tail_modes():
    from tacotronv2_wavernn_chinese_amd.vocoder import stream_release
    hop = 275
    for frames_in in range(0, 50):
        steps = _ready_mirror(frames_in, hop, 2, False)
        ref = stream_release(frames_in, steps, False, hop, 'reference')
        assert ref == min(max((frames_in - 21) * hop, 0), steps)
        assert ref <= steps and ref <= max(frames_in - 21, 0) * hop   # nothing the trim / fade-out may still touch
        assert stream_release(frames_in, steps, False, hop, 'none') == steps
        if frames_in >= 21:
            assert stream_release(frames_in, frames_in * hop, True, hop, 'reference') == (frames_in - 1) * hop
        assert stream_release(frames_in, frames_in * hop, True, hop, 'none') == frames_in * hop


def test_stream_prototypes_match_the_binding():
    """wrnn_stream is opaque (no struct to mirror): every stream entry point of the header has as many parameters as its
    ctypes prototype declares."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    hdr = open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read()
    assert re.search(r'typedef struct wrnn_stream wrnn_stream;', hdr)
    lib = _cabi.load_library()
    names = [s for s in _cabi.EXPORTED_SYMBOLS if s.startswith('wrnn_stream_')]
    assert sorted(names) == sorted(set(re.findall(r'\b(wrnn_stream_[a-z_]+)\s*\(', hdr)))
    for name in names:
        params = re.search(name + r'\s*\(([^)]*)\)', hdr).group(1)
        assert len([p for p in params.split(',') if p.strip()]) == len(getattr(lib, name).argtypes), name


def test_stream_entry_points_refuse_null_arguments():
    from tacotronv2_wavernn_chinese_amd import _cabi
    lib = _cabi.load_library()
    out = ctypes.c_void_p()
    n = ctypes.c_int64()
    assert lib.wrnn_stream_open(None, 1, None, ctypes.byref(out)) == _cabi.ERR_INVALID and not out.value
    assert lib.wrnn_stream_push(None, None, 0, 0, None, None, 0, ctypes.byref(n), None) == _cabi.ERR_INVALID
    assert lib.wrnn_stream_sync(None, None) == _cabi.ERR_INVALID
    assert lib.wrnn_stream_info(None, None, None, None) == _cabi.ERR_INVALID
    lib.wrnn_stream_close(None)   # a no-op


def test_stream_option_errors_need_no_device():
    """What a stream cannot do is refused before the model touches a device."""
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    m = WaveRNN(**DEFAULT_DIMS, mode='RAW')
    mol = WaveRNN(**DEFAULT_DIMS, mode='MOL')
    with pytest.raises(ValueError, match='whole clip'):
        m.stream(noise_mode='reference')
    with pytest.raises(ValueError, match='whole clip'):
        m.stream(noise_mode='injected')
    with pytest.raises(ValueError, match='fold'):
        m.stream(batched=True)
    with pytest.raises(ValueError, match='tail'):
        m.stream(tail='fade')
    with pytest.raises(ValueError, match='kernel'):
        m.stream(kernel='batch_cs')
    with pytest.raises(ValueError, match='RAW-only'):
        mol.stream(noise_mode='argmax')
    with pytest.raises(ValueError, match='batch'):
        m.stream(batch=0)
