"""INTEGRATION.md option B (the ctypes stub a maintainer pastes into the reference class) is the (b) row's evidence: it is pinned here.

CPU: the stub's three ctypes.Structure definitions are extracted from the markdown, executed, and compared field by field with the
gcc-compiled header (the same check tests/test_cabi_symbols.py applies to the package's own binding), and the ABI number the stub asserts is
the header's.  GPU: the stub's `_generate_device` is bound onto a reference-shaped module (same attribute names and state_dict as
fatchord_version.WaveRNN, :93-129) and its output for a T = 21 clip is checked against the oracle.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stub_namespace():
    md = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    sec = md[md.index('## Option B'):]
    code = re.search(r'```python\n(.*?)```', sec, re.S).group(1)
    ns = {}
    exec(compile(code, 'INTEGRATION.md:option-B', 'exec'), ns)
    return ns, code


def test_option_b_structs_match_the_header(tmp_path):
    ns, code = _stub_namespace()
    hdr = open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read()
    hdr_abi = int(re.search(r'#define WRNN_ABI_VERSION (\d+)', hdr).group(1))
    assert int(re.search(r'wrnn_abi_version\(\) == (\d+)', code).group(1)) == hdr_abi
    structs = {'wrnn_config': ns['_Cfg'], 'wrnn_tensor_desc': ns['_Desc'], 'wrnn_sample_opts': ns['_Opts']}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/wavernn_amd.h"', 'int main(void) {']
    for cname, st in structs.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in st._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c11', '-o', str(exe), str(src)])
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in subprocess.check_output([str(exe)], text=True).split('\n') if l.strip()}
    for cname, st in structs.items():
        assert got[(cname, 'size')] == C.sizeof(st), cname
        for fname, _ in st._fields_:
            assert got[(cname, fname)] == getattr(st, fname).offset, (cname, fname)
    # the entry points the stub calls exist in the header
    for sym in set(re.findall(r'lib\.(wrnn_[a-z_]+)', code)):
        assert re.search(r'\b' + sym + r'\s*\(', hdr), sym


@pytest.mark.parametrize('mode,bits', [('RAW', 10), ('MOL', 9)])
def test_option_b_config_and_descriptors_from_the_real_reference_class(mode, bits):
    """The stub reads attributes of the class it is pasted into (self.rnn_dims, self.fc1.out_features, self.pad, self.upsample..., :93-129).
    What its ``_cfg_of`` / ``_descs_of`` gave on the REAL ``wavernn.models.fatchord_version.WaveRNN`` (loaded with the same seeded weights)
    is recorded in tests/golden/option_b_reference_class.json (`python -m oracle.make_golden module`): it must be the wrnn_config and the
    tensor table the package's binding builds for the same weights, and the stub must give the same on this package's WaveRNN (what the
    GPU test binds it onto)."""
    import json
    import torch
    from oracle import make_golden as mg
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    ns, _ = _stub_namespace()
    with open(os.path.join(ROOT, 'tests', 'golden', 'option_b_reference_class.json')) as f:
        rec = json.load(f)[mode]
    assert rec['module'] == 'wavernn.models.fatchord_version.WaveRNN'
    sd = make_state_dict(0, mode=mode, variant='default', bits=bits)
    dims = dict(DEFAULT_DIMS, bits=bits)
    want = dict(rnn_dims=dims['rnn_dims'], fc_dims=dims['fc_dims'], bits=bits, pad=dims['pad'], n_upsample=len(dims['upsample_factors']),
                feat_dims=dims['feat_dims'], compute_dims=dims['compute_dims'], res_out_dims=dims['res_out_dims'], res_blocks=dims['res_blocks'],
                hop_length=dims['hop_length'], sample_rate=dims['sample_rate'], mode=_cabi.MODE_RAW if mode == 'RAW' else _cabi.MODE_MOL, device=3)
    for k, v in want.items():
        assert rec['cfg'][k] == v, k
    assert rec['cfg']['upsample_factors'][:rec['cfg']['n_upsample']] == list(dims['upsample_factors'])
    ours = WaveRNN(**dims, mode=mode)
    ours.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    cfg = ns['_cfg_of'](ours, 3)
    assert {f: (list(getattr(cfg, f)) if f == 'upsample_factors' else getattr(cfg, f)) for f, _ in cfg._fields_} == rec['cfg']
    ours_sd = {k: v.numpy() for k, v in ours.state_dict().items() if v.dtype == torch.float32}
    assert {name: (dt, tuple(shape)) for name, dt, shape, _ in rec['descs']} == {k: (_cabi.DTYPE_F32, a.shape) for k, a in ours_sd.items()}
    for name, _, _, sha in rec['descs']:   # the reference module's data pointers carried these weights
        assert sha == mg.tensor_sha256(ours_sd[name].reshape(-1)), name
    keep, descs = ns['_descs_of'](ours)
    assert [[d.name.decode(), d.dtype, list(d.shape[:d.ndim])] for d in descs] == [r[:3] for r in rec['descs']]
    for d, r in zip(descs, rec['descs']):
        a = np.ctypeslib.as_array(C.cast(d.data, C.POINTER(C.c_float)), shape=(int(np.prod(d.shape[:d.ndim])),))
        assert mg.tensor_sha256(a) == r[3], r[0]


@pytest.mark.gpu
def test_option_b_stub_generates_what_the_oracle_generates(monkeypatch):
    import torch
    from oracle import oracle as orc
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS, make_mels, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    from tests.parity_util import NEAR_TIE
    from tests.philox_ref import philox_uniform_raw_torch
    monkeypatch.setenv('WAVERNN_AMD_LIB', _cabi.LIB_PATH)
    ns, _ = _stub_namespace()
    sd = make_state_dict(0, variant='peaky')
    # the parameter container with the reference's attribute names and state_dict keys (fatchord_version.py:93-129); only the stub touches the library
    m = WaveRNN(**DEFAULT_DIMS, mode='RAW')
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    T = 21
    mels = make_mels(5, 1, T)
    seeds = []
    real_randint = torch.randint
    monkeypatch.setattr(torch, 'randint', lambda *a, **k: (lambda r: (seeds.append(int(r)), r)[1])(real_randint(*a, **k)))
    out = ns['_generate_device'](m, mels, False, 11000, 550)
    assert out.shape == (1, T * 275) and out.dtype == np.float64
    lab = np.rint((out[0] + 1.0) * 1023.0 / 2.0).astype(np.int64)
    np.testing.assert_allclose(2.0 * lab / 1023.0 - 1.0, out[0], atol=1e-6)
    # the oracle on the device's Philox draws (replayed on the host), driven along the stub's own trajectory
    L = T * 275
    u = philox_uniform_raw_torch(seeds[-1], 0, L, [0], device='cuda')
    q = (-torch.log(u.to(torch.float64))).to(torch.float32).cpu().numpy()
    om = orc.OracleModel(sd, fast=True)
    cm, ca = om.conditioning(mels)
    ref = om.loop(cm, ca, orc.NOISE_EXPO, q, x_forced=np.ascontiguousarray(out.T.astype(np.float32)))
    bad = np.flatnonzero(lab != ref['labels'][:, 0])
    for t in bad:
        assert ref['margin'][t, 0] < NEAR_TIE and lab[t] == ref['runner'][t, 0], f'step {t}'
    assert bad.size <= 1
