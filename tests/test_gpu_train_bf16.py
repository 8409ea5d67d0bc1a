"""MI355X: the training calls with `train_precision = 'bf16'` -- the wiring of csrc/train_gemm_bf16.hip into `train_impl`, not the proof of
the kernel (tests/test_gpu_train_gemm_bf16.py holds every product to float64 within accumulation rounding).

Steered inputs (tests/train_steer.py), the float64 emulation of the bf16 mode and e_bf per tensor from tests/train_bf16_ref.py; the
conditions this comparison rests on are asserted on the CPU by tests/test_train_bf16_host.py.  n = number of 32-CU teams:

    default dims (team recurrences where they can run)   RAW (4n + 1, 7), RAW (5, 3), MOL (5, 7)
    GENERIC_DIMS (step kernels)                          MOL (33, 3), RAW (5, 7)
    split pass, train_forward then train_backward        RAW default (4n + 1, 3), fed the float64 reference's d_logits

Per tensor (loss, logits, the 16 gradients, d_mels_up, d_aux), in max norm over the float64 reference's largest entry:

    |kernel - emulation64|        <= EMU_FACTOR x e_bf   (1.0: twice what torch's float32 run of the emulation needs on the CPU; the
                                                         tail is discrete bf16-neighbour events, not noise, hence the margin of 2)
    |kernel - float64 reference|  <= REF_FACTOR x e_bf   (2.0: the emulation is 1.0 from the reference by definition)

fc3.bias in the split pass has no rounded product in it and is held to the fp32 kernels' 2e-5 instead (train_bf16_ref.UNROUNDED).
MEASURED_ON_MI355X below is the table these factors are judged by.

Also here: `train_last_gemms` (2 fp32 GEMMs -- the x column, forward and backward -- and the rest bf16), two bf16 calls bit-identical,
a handle switched bf16 -> f32 bit-identical to a fresh fp32 handle, and five Adam steps through `training_loss` in bf16 (finite,
decreasing; the fp32 trajectory printed next to it -- no bound between the two is asserted, none can be derived).
"""
import numpy as np
import pytest
import torch

from tests import train_bf16_ref as br
from tests import train_steer as ts

EMU_FACTOR = 1.0
REF_FACTOR = 2.0
MEASURED_ON_MI355X = """n = 8, worst tensor per case, error / e_bf (every tensor: profiles/train_bf16.txt, section 5)
    RAW default (33, 7) team512     emulation 0.432 (d_mels_up)            reference 1.050 (d_mels_up)
    RAW default (5, 3)  team512     emulation 0.006 (rnn1.weight_hh_l0)    reference 1.000 (loss)
    MOL default (5, 7)  team512     emulation 0.134 (I.weight)             reference 1.003 (rnn1.bias_ih_l0)
    MOL generic (33, 3) steps       emulation 0.005 (rnn2.weight_hh_l0)    reference 1.001 (loss)
    RAW generic (5, 7)  steps       emulation 0.032 (rnn1.weight_ih_l0)    reference 1.000 (I.bias)
    split RAW default (33, 3)       emulation 0.350 (d_mels_up)            reference 1.015 (rnn1.bias_ih_l0)
No case exceeds its starting factor, so both stand as set.  Adam, loss per step: f32 5.55166 5.48348 5.39870 5.27119 5.10430,
bf16 5.55164 5.48359 5.39904 5.27185 5.10478."""


@pytest.fixture(scope='module')
def handle_of():
    """(mode, dims name) -> (native handle in bf16 mode, number of teams); one model per pair, kept for the module."""
    from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    models = {}

    def get(mode, dims_name):
        if (mode, dims_name) not in models:
            dims = ts.dims_of(dims_name)
            m = WaveRNN(**dims, mode=mode)
            m.verbose = False
            m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in make_state_dict(0, mode=mode, variant='default', **dims).items()})
            m.to('cuda:0')
            m.train()
            m.train_precision = 'bf16'
            models[(mode, dims_name)] = m
        nat = models[(mode, dims_name)]._native_handle()
        assert nat.train_precision == 'bf16'
        ok, n, _ = nat.team_info()
        return nat, (n if n >= 1 else 8)

    yield get
    models.clear()


class _Call:
    """The device tensors of one case: steered parameters in LOOP_PARAM_KEYS order, inputs, NaN-filled outputs."""

    def __init__(self, st, mode, dev):
        from tacotronv2_wavernn_chinese_amd import _cabi
        nan = float('nan')
        self.keys = _cabi.LOOP_PARAM_KEYS
        self.B, self.L = st['x'].shape
        self.ps = [torch.from_numpy(st['sd'][k]).to(dev).contiguous() for k in self.keys]
        self.x = torch.from_numpy(st['x']).to(dev).contiguous()
        self.mu = torch.from_numpy(st['mels_up']).to(dev).contiguous()
        self.au = torch.from_numpy(st['aux']).to(dev).contiguous()
        self.y = torch.from_numpy(st['y']).to(dev).to(torch.int32 if mode == 'RAW' else torch.float32).contiguous()
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self.gs = [torch.full_like(p, nan) for p in self.ps]
        self.dm, self.da = torch.full_like(self.mu, nan), torch.full_like(self.au, nan)
        self.logits = torch.full((self.B, self.L, self.ps[-1].shape[0]), nan, device=dev)
        self.loss = torch.full((), nan, device=dev)

    @staticmethod
    def ptrs(ts_):
        return [t.data_ptr() for t in ts_]

    def step(self, nat):
        nat.train_step(self.ptrs(self.ps), self.ptrs(self.gs), self.x.data_ptr(), self.mu.data_ptr(), self.au.data_ptr(), self.y.data_ptr(),
                       self.B, self.L, self.loss.data_ptr(), self.logits.data_ptr(), self.dm.data_ptr(), self.da.data_ptr(), self.stream)
        nat.sync_status(self.stream)

    def got(self, loss=True):
        g = {k: t.cpu().numpy().astype(np.float64) for k, t in zip(self.keys, self.gs)}
        g['d_mels_up'], g['d_aux'] = self.dm.cpu().numpy().astype(np.float64), self.da.cpu().numpy().astype(np.float64)
        g['logits'] = self.logits.cpu().numpy().astype(np.float64)
        if loss:
            g['loss'] = np.array([float(self.loss)], np.float64)
        return g

    def bits(self):
        return [t.cpu().numpy().copy() for t in self.gs + [self.dm, self.da, self.logits, self.loss]]


def _hold(tag, case, got, c):
    """Print error / e_bf of every tensor against the emulation and the reference, then assert the two factors."""
    e_bf, unrounded = c['e_bf'], br.UNROUNDED.get(case, ())
    d_emu, d_ref = br.errors(got, {k: c['emu'][k] for k in got}, c['ref']), br.errors(got, {k: c['ref'][k] for k in got}, c['ref'])
    rows = [(k, e_bf[k], d_emu[k] / e_bf[k], d_ref[k] / e_bf[k]) for k in got if k not in unrounded]
    print(f'\n{tag}  tensor: e_bf, |kernel - emulation| / e_bf, |kernel - reference| / e_bf')
    for k, e, a, b in rows:
        print(f'    {k:22s} {e:.2e}  {a:.3f}  {b:.3f}')
    wa, wb = max(rows, key=lambda r: r[2]), max(rows, key=lambda r: r[3])
    print(f'{tag}  worst: emulation {wa[2]:.3f} ({wa[0]}), reference {wb[3]:.3f} ({wb[0]})')
    for k in unrounded:
        print(f'    {k:22s} no rounded product: |kernel - reference| {d_ref[k]:.2e} of the largest entry')
        assert d_ref[k] <= br.F32_TOL, (tag, k, d_ref[k])
    for k, e, a, b in rows:
        assert np.isfinite(a) and a <= EMU_FACTOR, (tag, k, a, e)
        assert b <= REF_FACTOR, (tag, k, b, e)


@pytest.mark.gpu
@pytest.mark.parametrize('case', br.CASES, ids=br.case_id)
def test_bf16_train_step_is_the_emulation_within_e_bf(case, handle_of):
    mode, dims_name, spec, L, _ = case
    dev = torch.device('cuda:0')
    nat, n = handle_of(mode, dims_name)
    c = br.case_reference(case, n, device=dev)
    call = _Call(c['st'], mode, dev)
    call.step(nat)
    first = call.bits()
    n_f32, n_bf16 = nat.train_last_gemms()
    assert n_f32 == 2 and n_bf16 > 0, (n_f32, n_bf16)       # the x column of I, forward and backward; everything else
    call.step(nat)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, call.bits())), 'two bf16 calls differ'
    _hold(f'[train bf16 {br.case_id(case)} B={call.B} {nat.train_last_recurrence()[0]}]', case, call.got(), c)


@pytest.mark.gpu
def test_bf16_split_pass_from_the_float64_loss_gradient(handle_of):
    case = br.SPLIT_CASE
    mode, dims_name, spec, L, _ = case
    dev = torch.device('cuda:0')
    nat, n = handle_of(mode, dims_name)
    c = br.case_reference(case, n, device=dev)
    call = _Call(c['st'], mode, dev)
    dl = torch.from_numpy(c['d_logits'].astype(np.float32)).to(dev).contiguous()
    nat.train_forward(call.ptrs(call.ps), call.x.data_ptr(), call.mu.data_ptr(), call.au.data_ptr(), call.B, L, call.logits.data_ptr(), call.stream)
    nat.sync_status(call.stream)
    assert nat.train_last_gemms()[0] == 1
    nat.train_backward(call.ptrs(call.ps), call.ptrs(call.gs), dl.data_ptr(), call.x.data_ptr(), call.mu.data_ptr(), call.au.data_ptr(), call.B, L,
                       call.dm.data_ptr(), call.da.data_ptr(), call.stream)
    nat.sync_status(call.stream)
    n_f32, n_bf16 = nat.train_last_gemms()
    assert n_f32 == 1 and n_bf16 > 0, (n_f32, n_bf16)
    _hold(f'[train bf16 split {br.case_id(case)} B={call.B}]', case, call.got(loss=False), c)


@pytest.mark.gpu
def test_switching_back_to_f32_is_bit_identical_to_a_fresh_f32_handle(handle_of):
    from tacotronv2_wavernn_chinese_amd import _cabi
    case = br.CASES[1]
    mode, dims_name, spec, L, _ = case
    dev = torch.device('cuda:0')
    nat, n = handle_of(mode, dims_name)
    c = br.case_reference(case, n, device=dev)
    fresh = _cabi.NativeVocoder(device=0, mode=mode, **ts.dims_of(dims_name))
    try:
        assert fresh.train_precision == 'f32'
        with pytest.raises(_cabi.WrnnError) as e:
            fresh.train_last_gemms()
        assert e.value.code == _cabi.ERR_STATE
        a, b, d = _Call(c['st'], mode, dev), _Call(c['st'], mode, dev), _Call(c['st'], mode, dev)
        a.step(nat)                                   # bf16
        nat.set_train_precision('f32')
        b.step(nat)
        assert nat.train_last_gemms()[1] == 0 and nat.train_last_gemms()[0] > 2
        d.step(fresh)
        assert fresh.train_last_gemms() == nat.train_last_gemms()
    finally:
        nat.set_train_precision('bf16')
        fresh.close()
    assert all(np.array_equal(p, q) for p, q in zip(b.bits(), d.bits())), 'bf16 -> f32 differs from a fresh f32 handle'
    assert not all(np.array_equal(p, q) for p, q in zip(a.bits(), b.bits())), 'the bf16 call returned the f32 bits'
    with pytest.raises(ValueError):
        nat.set_train_precision('fp16')


@pytest.mark.gpu
def test_five_adam_steps_in_bf16_decrease_the_loss():
    from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    dims = dict(ts.GENERIC_DIMS, upsample_factors=(4, 4, 4), hop_length=64)     # L = one frame of 64 samples
    B, L = 8, 64
    rng = np.random.Generator(np.random.PCG64(11))
    lab = rng.integers(0, 2 ** dims['bits'], size=(B, L + 1))
    x = torch.from_numpy((2.0 * lab[:, :-1] / (2 ** dims['bits'] - 1.0) - 1.0).astype(np.float32)).cuda()
    y = torch.from_numpy(lab[:, 1:]).cuda()
    mels = torch.from_numpy(rng.random((B, dims['feat_dims'], 1 + 2 * dims['pad']), dtype=np.float32)).cuda()
    curves = {}
    for prec in ('f32', 'bf16'):
        m = WaveRNN(**dims, mode='RAW')
        m.verbose = False
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in make_state_dict(0, mode='RAW', variant='default', **dims).items()})
        m.to('cuda:0')
        m.train()
        m.train_precision = prec
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        out = []
        for _ in range(5):
            loss = m.training_loss(x, mels, y)
            opt.zero_grad()
            loss.backward()
            opt.step()
            out.append(loss.item())
        status = m.training_status()
        assert status['train_precision'] == prec and (status['gemms'][1] > 0) == (prec == 'bf16'), status
        curves[prec] = out
    print('\n[train bf16 adam] B=8 L=64 loss per step  f32: ' + ' '.join(f'{v:.5f}' for v in curves['f32']) +
          '  bf16: ' + ' '.join(f'{v:.5f}' for v in curves['bf16']))
    assert all(np.isfinite(v) for v in curves['bf16'])
    assert curves['bf16'][-1] < curves['bf16'][0], curves['bf16']
