"""The contract every handle family of ``libwavernn_amd.so`` keeps, pinned for the families that can be created without a device:
``*_last_error(NULL)``, a refused create that still hands out a handle with its text, the compute entry that answers such a handle
before it reads an argument, ``*_destroy`` of it and of NULL, and the ``struct_size`` refusal.  The host side of these entries is one
shared runtime (``csrc/handle_common.h``); the texts below are the ones each family has always given."""
import ctypes as C

import pytest

from tacotronv2_wavernn_chinese_amd import _cabi
from tacotronv2_wavernn_chinese_amd.tacotron import make_dims

MEL = dict(sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, n_mels=80, fmin=95.0, min_level_db=-100.0, device=0)
REFUSED_BY = "the handle's configuration was refused by wrnn_%s_create"


def _mel_config(**kw):
    return _cabi.MelConfig(**dict(MEL, **kw))


def _short(struct):
    struct.struct_size -= 4
    return struct


def _mel_create(lib, h, cfg=None, feat=None):
    return lib.wrnn_mel_create_features(C.byref(cfg or _mel_config()), C.byref(feat or _cabi.MelFeatures()), C.byref(h))


def _griffin_create(lib, h, cfg=None, griffin=None):
    return lib.wrnn_griffin_create(C.byref(cfg or _mel_config()), C.byref(_cabi.MelFeatures()), C.byref(griffin or _cabi.GriffinConfig()), C.byref(h))


def _score_create(lib, h, score=None):
    return lib.wrnn_score_create(C.byref(_mel_config()), None, C.byref(score or _cabi.ScoreConfig()), C.byref(h))


def _pitch_create(lib, h, pitch=None):
    return lib.wrnn_pitch_create(C.byref(pitch or _cabi.PitchConfig()), C.byref(h))


def _align_create(lib, h, align=None):
    return lib.wrnn_align_create(C.byref(_mel_config()), None, C.byref(align or _cabi.AlignConfig()), C.byref(h))


def _taco_create(lib, h, dims=None):
    return lib.wrnn_taco_create(C.byref(dims or make_dims()), C.byref(h))


# family -> (create with one bad field, its status, a piece of its text,
#            the compute entry on the refused handle with every pointer NULL, its status, its text,
#            create with struct_size off by four (None: the family has no struct), its text)
FAMILIES = {
    'mel': (lambda lib, h: _mel_create(lib, h, cfg=_mel_config(n_fft=1024)), _cabi.ERR_UNSUPPORTED,
            b'n_fft = 1024: the front end is built for n_fft = 2048 only',
            lambda lib, h: lib.wrnn_melspectrogram(h, None, 0, None, 0, 0, None, None), _cabi.ERR_STATE, REFUSED_BY % 'mel',
            lambda lib, h: _mel_create(lib, h, feat=_short(_cabi.MelFeatures())),
            b"features.struct_size = 28, this library's wrnn_mel_features has 32 bytes"),
    'griffin': (lambda lib, h: _griffin_create(lib, h, cfg=_mel_config(n_fft=1024)), _cabi.ERR_UNSUPPORTED,
                b'n_fft = 1024: Griffin-Lim is built for n_fft = 2048 only',
                lambda lib, h: lib.wrnn_griffin_lim(h, None, None, 0, 0, 0, 0, 0, None, None, 0, None, None), _cabi.ERR_STATE,
                REFUSED_BY % 'griffin',
                lambda lib, h: _griffin_create(lib, h, griffin=_short(_cabi.GriffinConfig())),
                b"griffin.struct_size = 8, this library's wrnn_griffin_config has 12 bytes"),
    'score': (lambda lib, h: _score_create(lib, h, score=_cabi.ScoreConfig(mcd_order=0)), _cabi.ERR_INVALID,
              b'mcd_order = 0: 1 <= mcd_order <= n_mels - 1 = 79',
              lambda lib, h: lib.wrnn_score(h, None, None, 0, None, 0, None, None, 0, None), _cabi.ERR_STATE, REFUSED_BY % 'score',
              lambda lib, h: _score_create(lib, h, score=_short(_cabi.ScoreConfig())),
              b"score.struct_size = 60, this library's wrnn_score_config has 64 bytes"),
    'pitch': (lambda lib, h: _pitch_create(lib, h, pitch=_cabi.PitchConfig(hop=0)), _cabi.ERR_INVALID,
              b'sample_rate = 22050, hop = 0: both are at least 1',
              lambda lib, h: lib.wrnn_pitch_score(h, None, None, 0, None, 0, None, None, 0, None), _cabi.ERR_STATE, REFUSED_BY % 'pitch',
              lambda lib, h: _pitch_create(lib, h, pitch=_short(_cabi.PitchConfig())),
              b"struct_size = 60, this library's wrnn_pitch_config has 64 bytes"),
    'align': (lambda lib, h: _align_create(lib, h, align=_cabi.AlignConfig(mcd_order=99)), _cabi.ERR_INVALID,
              b'mcd_order = 99: 1 <= mcd_order <= n_mels - 1 = 79',
              lambda lib, h: lib.wrnn_align_score(h, None, 0, None, None, 0, None, 0, None, None, 0, None, None, None, None, None),
              _cabi.ERR_STATE, REFUSED_BY % 'align',
              lambda lib, h: _align_create(lib, h, align=_short(_cabi.AlignConfig())),
              b"align.struct_size = 12, this library's wrnn_align_config has 16 bytes"),
    'resample': (lambda lib, h: lib.wrnn_resample_create(44100, 22050, -1, C.byref(h)), _cabi.ERR_INVALID, b'bad configuration: device >= 0',
                 lambda lib, h: lib.wrnn_resample(h, None, 0, None, 0, 0, None, None), _cabi.ERR_STATE,
                 "the handle's rates were refused by wrnn_resample_create", None, None),
    # the Tacotron section answers a refused handle with WRNN_ERR_INVALID and a text of its own
    'taco': (lambda lib, h: _taco_create(lib, h, dims=make_dims(decoder_layers=9)), _cabi.ERR_INVALID,
             b'unsupported dims: decoder_layers 9 outside 1 .. 4',
             lambda lib, h: lib.wrnn_taco_synthesize(h, None, None), _cabi.ERR_INVALID, 'the handle was refused at creation',
             lambda lib, h: _taco_create(lib, h, dims=_short(make_dims())),
             b"wrnn_taco_dims.struct_size %d, this library's is %d" % (C.sizeof(_cabi.TacoDims) - 4, C.sizeof(_cabi.TacoDims))),
}


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_handle_contract(family):
    lib = _cabi.load_library()
    bad_create, bad_status, bad_text, compute, refused_status, refused_text, short_create, short_text = FAMILIES[family]
    last_error, destroy = getattr(lib, f'wrnn_{family}_last_error'), getattr(lib, f'wrnn_{family}_destroy')
    assert last_error(None) == b'null handle'
    destroy(None)
    h = C.c_void_p()
    assert bad_create(lib, h) == bad_status
    assert h.value, 'a refused create still hands out its handle'
    assert last_error(h) == bad_text
    assert compute(lib, h) == refused_status
    assert last_error(h) == refused_text.encode()
    destroy(h)
    if short_create is not None:
        h = C.c_void_p()
        assert short_create(lib, h) == _cabi.ERR_INVALID
        assert h.value and last_error(h) == short_text
        destroy(h)
