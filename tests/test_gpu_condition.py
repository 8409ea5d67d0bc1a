"""The wav conditioning on the GPU (``csrc/condition.hip``) against the float64 restatement ``tests/condition_ref.py``.

What is asked.  Bounds and lengths EQUAL to the restatement's: every fixture keeps every frame 0.1 dB or more from the threshold
(``tests/test_condition_host.py`` asserts it), and the kernel's float64 energies differ from the restatement's by a summation order only.
Energies within 1e-12 relative: another float64 order over at most 2048 squares costs about 2048 x 1.1e-16 = 2.3e-13.  The conditioned
samples BIT-EQUAL to NumPy's float32 ``x[start:end] / peak * target`` (a correctly rounded divide, then one multiply), the padding
exactly zero, and every row of a ragged call bit-equal to the call on that clip alone.  Each parity test prints its largest energy error
before it asserts (``pytest -s``)."""
import numpy as np
import pytest
import torch

from tests import condition_ref as cr

pytestmark = pytest.mark.gpu
CASES = cr.cases()
_refs = {}


def ref(i):
    """(energies, (start, end), peak, y) of case i in the restatement, computed once and shared."""
    if i not in _refs:
        _, x, top_db, L, h = CASES[i]
        y, bounds, peak = cr.condition(x, top_db, 0.999, L, h)
        _refs[i] = (cr.frame_energies(x, L, h), bounds, peak, y)
    return _refs[i]


def _cond(top_db=25.0, peak=True, L=2048, h=512):
    from tacotronv2_wavernn_chinese_amd.frontend import WavConditioner
    return WavConditioner(top_db, peak, frame_length=L, hop_length=h)


def _run(c, buf, lens):
    """condition_padded with every optional output -> host arrays (out, n_out, bounds, peaks, energies or None)."""
    B, n_max = buf.shape
    bounds = torch.full((B, 2), -7, dtype=torch.int32, device='cuda')
    peaks = torch.full((B,), -7.0, dtype=torch.float32, device='cuda')
    en = torch.full((B, 1 + n_max // c.hop_length), -7.0, dtype=torch.float64, device='cuda') if c.trim_top_db is not None else None
    out, n_out = c.condition_padded(buf, lens, bounds=bounds, peaks=peaks, energies=en)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, n_max) and n_out.dtype == torch.int32 and tuple(n_out.shape) == (B,)
    return out.cpu().numpy(), n_out.cpu().numpy(), bounds.cpu().numpy(), peaks.cpu().numpy(), None if en is None else en.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_row(name, i, out, n_out, bounds, peak, en):
    e_ref, (start, end), peak_ref, y = ref(i)
    F = e_ref.shape[0]
    rel = float(np.max(np.abs(en[:F] - e_ref) / e_ref))
    print(f'condition {name}: {F} frames, largest relative energy error {rel:.3e} (bound 1e-12), bounds {tuple(bounds)} (restatement {(start, end)})')
    assert tuple(int(v) for v in bounds) == (start, end) and int(n_out) == end - start, name
    assert rel <= 1e-12 and not en[F:].any(), name
    assert _bits(peak) == _bits(peak_ref), name
    np.testing.assert_array_equal(_bits(out[:end - start]), _bits(y), err_msg=name)
    assert not _bits(out[end - start:]).any(), name          # exactly +0 up to n_out_max


@pytest.mark.parametrize('i', range(len(CASES)), ids=[c[0] for c in CASES])
def test_each_clip_alone(i):
    name, x, top_db, L, h = CASES[i]
    out, n_out, bounds, peaks, en = _run(_cond(top_db, True, L, h), torch.from_numpy(x).cuda().view(1, -1), [x.shape[0]])
    _check_row(name, i, out[0], n_out[0], bounds[0], peaks[0], en[0])


SETTINGS = sorted({c[2:] for c in CASES})


@pytest.mark.parametrize('top_db, L, h', SETTINGS, ids=[f'db{int(s[0])}_w{s[1]}' for s in SETTINGS])
def test_ragged_batch_rows_are_bit_equal_to_the_solo_calls_and_padding_is_never_read(top_db, L, h):
    """All the clips of one setting as the rows of one call, what lies past each clip filled with NaN."""
    ids = [i for i, c in enumerate(CASES) if c[2:] == (top_db, L, h)]
    lens = [CASES[i][1].shape[0] for i in ids]
    assert len(ids) > 8 and len(set(lens)) > 2
    buf = torch.full((len(ids), max(lens) + 5), float('nan'), dtype=torch.float32, device='cuda')
    for r, i in enumerate(ids):
        buf[r, :lens[r]] = torch.from_numpy(CASES[i][1]).cuda()
    c = _cond(top_db, True, L, h)
    out, n_out, bounds, peaks, en = _run(c, buf, lens)
    for r, i in enumerate(ids):
        _check_row('ragged/' + CASES[i][0], i, out[r], n_out[r], bounds[r], peaks[r], en[r])
        so, sn, sb, sp, se = _run(c, torch.from_numpy(CASES[i][1]).cuda().view(1, -1), [lens[r]])
        np.testing.assert_array_equal(_bits(out[r, :lens[r]]), _bits(so[0]))
        F = se.shape[1]
        np.testing.assert_array_equal(en[r, :F].view(np.uint64), se[0].view(np.uint64))    # the energies too, bit for bit
        assert sn[0] == n_out[r] and tuple(sb[0]) == tuple(bounds[r]) and _bits(sp[0]) == _bits(peaks[r])
    listed = c.condition([CASES[i][1] for i in ids])                                       # the same batch from host clips
    assert c.last_lens == [int(n) for n in n_out] and c.last_bounds.tolist() == bounds.tolist()
    np.testing.assert_array_equal(_bits(c.last_peaks), _bits(peaks))
    np.testing.assert_array_equal(_bits(listed.cpu().numpy()), _bits(out[:, :max(lens)]))


def test_all_zero_clip_comes_back_whole_and_unscaled():
    out, n_out, bounds, peaks, en = _run(_cond(), torch.zeros((1, 5000), dtype=torch.float32, device='cuda'), [5000])
    assert n_out[0] == 5000 and tuple(bounds[0]) == (0, 5000) and peaks[0] == 0 and not _bits(out).any() and not en.any()
    buf = torch.zeros((2, 6000), dtype=torch.float32, device='cuda')
    buf[1] = torch.from_numpy(CASES[0][1][:1].repeat(6000)).cuda()      # a constant row next to it: every frame equally loud, kept whole
    out, n_out, bounds, peaks, en = _run(_cond(), buf, [5000, 6000])
    assert n_out.tolist() == [5000, 6000] and bounds.tolist() == [[0, 5000], [0, 6000]] and not _bits(out[0]).any()


def test_trim_only_is_a_bit_exact_slice():
    i = next(k for k, c in enumerate(CASES) if c[0].startswith('n12345_mid_db25_w2048'))
    x = CASES[i][1]
    start, end = ref(i)[1]
    out, n_out, bounds, peaks, en = _run(_cond(25.0, None), torch.from_numpy(x).cuda().view(1, -1), [x.shape[0]])
    assert 0 < start < end < x.shape[0] and tuple(bounds[0]) == (start, end) and n_out[0] == end - start
    np.testing.assert_array_equal(_bits(out[0, :end - start]), _bits(x[start:end]))
    assert not _bits(out[0, end - start:]).any() and _bits(peaks[0]) == _bits(ref(i)[2])


def test_peak_only_keeps_the_whole_clip():
    i = next(k for k, c in enumerate(CASES) if c[0].startswith('n12345_mid_db25_w2048'))
    x = CASES[i][1]
    short = x[:700]                                    # no trimming: a clip shorter than the trim window is welcome
    for clip in (x, short):
        out, n_out, bounds, peaks, en = _run(_cond(None, 0.5), torch.from_numpy(clip).cuda().view(1, -1), [clip.shape[0]])
        assert en is None and tuple(bounds[0]) == (0, clip.shape[0]) and n_out[0] == clip.shape[0]
        y, _, peak = cr.condition(clip, None, 0.5)
        assert _bits(peaks[0]) == _bits(peak)
        np.testing.assert_array_equal(_bits(out[0]), _bits(y))


def test_lengths_may_stay_on_the_device():
    """The lengths one call returns are the next call's ``lens``: conditioning twice changes nothing but the last bit of the scale."""
    ids = [i for i, c in enumerate(CASES) if c[2:] == (25.0, 2048, 512) and c[1].shape[0] >= 5119][:6]
    lens = [CASES[i][1].shape[0] for i in ids]
    buf = torch.zeros((len(ids), max(lens)), dtype=torch.float32, device='cuda')
    for r, i in enumerate(ids):
        buf[r, :lens[r]] = torch.from_numpy(CASES[i][1]).cuda()
    c = _cond(None, True)
    out, n_out = c.condition_padded(buf, lens)
    again, n_again = c.condition_padded(out, n_out)
    assert n_again.tolist() == n_out.tolist() == lens
    assert float((again - out).abs().max()) <= 2.0 ** -23


def test_non_finite_samples_stay_inside_the_clip():
    x = CASES[0][1].copy()
    big = np.tile(x, 8)[:6000]
    for bad in (np.nan, np.inf, -np.inf):
        y = big.copy()
        y[[0, 3000, 5999]] = bad
        out, n_out, bounds, peaks, en = _run(_cond(), torch.from_numpy(y).cuda().view(1, -1), [6000])
        assert 0 <= bounds[0, 0] <= bounds[0, 1] <= 6000 and n_out[0] == bounds[0, 1] - bounds[0, 0]
    out, n_out, bounds, peaks, en = _run(_cond(), torch.full((1, 6000), float('nan'), dtype=torch.float32, device='cuda'), [6000])
    assert 0 <= bounds[0, 0] <= bounds[0, 1] <= 6000 and n_out[0] == bounds[0, 1] - bounds[0, 0]


def test_error_paths_start_no_launch(monkeypatch):
    from tacotronv2_wavernn_chinese_amd import _cabi
    launches = []
    real = _cabi.condition
    monkeypatch.setattr(_cabi, 'condition', lambda *a: (launches.append(a), real(*a))[1])
    c = _cond()
    good = torch.zeros((2, 3000), dtype=torch.float32, device='cuda')
    for wav, lens in [(good.cpu(), [3000, 2000]), (good[:0], []), (good, [3000, 3001]), (good, [3000]), (good, [3000, 0]),
                      (good, [3000, 1024]),                        # too short for the trim window
                      (good.double(), [3000, 2000]), (good[:, ::2], [1500, 1500]),
                      (good, torch.tensor([3000, 2000], dtype=torch.int64, device='cuda')), (good, torch.tensor([3000], dtype=torch.int32, device='cuda'))]:
        with pytest.raises(ValueError):
            c.condition_padded(wav, lens)
    for kw in (dict(bounds=torch.zeros((2, 2), dtype=torch.int64, device='cuda')), dict(peaks=torch.zeros(3, dtype=torch.float32, device='cuda')),
               dict(energies=torch.zeros((2, 5), dtype=torch.float64, device='cuda'))):
        with pytest.raises(ValueError):
            c.condition_padded(good, [3000, 2000], **kw)
    with pytest.raises(ValueError):
        _cond(None, True).condition_padded(good, [3000, 2000], energies=torch.zeros((2, 6), dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError):
        c.condition([])
    assert not launches
    c.condition_padded(good, [3000, 2000])
    assert len(launches) == 1
