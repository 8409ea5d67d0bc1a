"""MI355X: `wrnn_train_last_recurrence` says which kernels ran the two GRU recurrences of the last training call on a handle: the
per-step kernels on the generic dims (rnn 256), the persistent team kernels with `min(8, ceil(B / n))` rows per team on the default
dims (rnn 512), the per-step kernels again once `train_force_step_kernels` is on; WRNN_ERR_STATE before any training call.  The calls
themselves are those of tests/test_gpu_train_steer.py (steered inputs, `sync_status` after each); what they compute is held to float64
there, here the gradients only have to come out finite."""
import pytest
import torch

from tests import train_steer as ts


def _step(nat, st, mode, dev, grads=True):
    from tacotronv2_wavernn_chinese_amd import _cabi
    B, L = st['x'].shape
    ps = [torch.from_numpy(st['sd'][k]).to(dev).contiguous() for k in _cabi.LOOP_PARAM_KEYS]
    gs = [torch.full_like(p, float('nan')) for p in ps]
    x, mu, au = (torch.from_numpy(st[k]).to(dev).contiguous() for k in ('x', 'mels_up', 'aux'))
    y = torch.from_numpy(st['y']).to(dev).to(torch.int32 if mode == 'RAW' else torch.float32).contiguous()
    dm, da = torch.full_like(mu, float('nan')), torch.full_like(au, float('nan'))
    loss = torch.full((), float('nan'), device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    nat.train_step([p.data_ptr() for p in ps], [g.data_ptr() for g in gs] if grads else None, x.data_ptr(), mu.data_ptr(), au.data_ptr(), y.data_ptr(),
                   B, L, loss.data_ptr(), 0, dm.data_ptr() if grads else 0, da.data_ptr() if grads else 0, stream)
    nat.sync_status(stream)
    assert bool(torch.isfinite(loss))
    if grads:
        assert all(bool(torch.isfinite(g).all()) for g in gs + [dm, da])


@pytest.mark.gpu
@pytest.mark.parametrize('dims_name', ['generic', 'default'])
def test_last_recurrence_reports_what_auto_ran(dims_name):
    from tacotronv2_wavernn_chinese_amd import _cabi
    dev = torch.device('cuda:0')
    nat = _cabi.NativeVocoder(**ts.dims_of(dims_name), mode='RAW', device=0)
    try:
        assert nat.lib.wrnn_train_last_recurrence(nat._h, None, None) == -3          # WRNN_ERR_STATE: no training call yet
        with pytest.raises(_cabi.WrnnError):
            nat.train_last_recurrence()
        ok, n, why = nat.team_info()
        assert n >= 1, why
        if dims_name == 'default':
            assert ok, why
        team = dims_name == 'default'
        for B, L in ((3, 2), (4 * n + 1, 3), (8 * n + 6, 2)):
            st = ts.steered('RAW', B, L, 100 + B, ts.dims_of(dims_name), device=dev)
            _step(nat, st, 'RAW', dev)
            assert nat.train_last_recurrence() == (('team512', min(8, -(-B // n))) if team else ('steps', 0)), (B, L)
            _step(nat, st, 'RAW', dev, grads=False)                                  # a forward-only call reports alike
            assert nat.train_last_recurrence() == (('team512', min(8, -(-B // n))) if team else ('steps', 0)), (B, L)
        nat.train_force_step_kernels(True)
        _step(nat, st, 'RAW', dev)
        assert nat.train_last_recurrence() == ('steps', 0)
        nat.train_force_step_kernels(False)
        _step(nat, st, 'RAW', dev)
        assert nat.train_last_recurrence() == (('team512', 8) if team else ('steps', 0))
        import ctypes as C
        kk = C.c_int32(-9)                                                           # either out pointer may be NULL
        assert nat.lib.wrnn_train_last_recurrence(nat._h, C.byref(kk), None) == 0 and kk.value == (1 if team else 0)
    finally:
        nat.close()
