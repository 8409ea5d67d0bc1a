"""MI355X: `wrnn_train_step` (csrc/train.hip, csrc/train_team.hip) against float64 autograd on STEERED inputs (tests/train_steer.py:
both ReLU masks known and every pre-activation at least 0.25 from zero, asserted on the CPU by tests/test_train_steer_host.py), so
that every entry of every gradient is held to one tight bound -- no quantile, no excused (row, step) pairs -- at the shapes where
the kernels branch.  n = the number of 32-CU teams (`team_info`, 8 on the MI355X); default dims (H = 512) unless stated:

    rows per team   RAW, L = 7 (three unrolled pairs + a tail step), B = n (r - 1) + 1 for r = 1 ... 8: rpb = r with a ragged last
                    batch (B = 1: n - 1 teams idle; B = 6 n + 1: seven full batches); B = 8 n (full), 8 n + 6 (team 0 runs a second
                    batch), 16 n + 2 (17 batches: team 0 runs three)
    length          RAW, B in {5, 4 n + 1, 16 n + 2} x L in {1, 2, 3, 64, 65}: the `a.L > 1`, `t + 1 < a.L`, `t + 2 < a.L` guards and
                    the liveness check at t = 62, with a tail step after it at 65; K = B L from 5 up: split-K slices past the end of K,
                    `col_sum_part_kernel` chunks past M
    MOL             (4 n + 1, 7), (5, 1), (16 n + 2, 3): the 30-wide fc3 tile, `gemm_tn` with Mo = 30, `mol_grad_kernel`
    generic `<0>`   rnn 256 / fc 384 / 40 mels / aux 24, RAW and MOL at (33, 3), (35, 7), (1, 1)
    split pass      train_forward, then train_backward from the float64 reference's d_logits (rounded to float32), at (4 n + 1, 3)
    branches of `<0>`  six models (tests/train_steer.py BRANCH_DIMS, tiny upsampler), RAW at (1, 1) -- only the `have == false` step --,
                    (2, 2) -- one carry step -- and (33, 3) -- a second row block holding one real row, two carries --; MOL at (33, 3)
                    for h48 and h272; the split pass at h272 (33, 3); each asserts train_last_recurrence() == ('steps', 0).
                    G = 3 rnn columns of dGH staged in chunks of 768, nblk = rnn / 4 workgroups remapped by `xcd_tile` iff nblk % 8 == 0:
                      h16   rnn 16 / fc 8 / 32 classes / 3 mels / aux 4: kq = 4 (one MFMA step per wave), one 48-column chunk, nblk = 4
                            (identity map), fewer classes than lanes in `ce_grad_kernel`, A = 1
                      h48   rnn 48 / fc 200 / 128 / 13 / 20: one partial chunk of 144, nblk = 12 (identity), A = 5 (aux slices only 4-byte
                            aligned, R = 20), fc > max(3 rnn, classes): the widest `colsum` is fc's (the `cs_part` sizing)
                      h272  rnn 272 / fc 72 / 256 / 40 / 96: G = 768 + 48, the shortest tail chunk; nblk = 68 (identity)
                      h320  rnn 320 / fc 96 / 256 / 40 / 96: G = 768 + 192; nblk = 80, the remapped arm with a tail chunk
                      h528  rnn 528 / fc 64 / 64 / 20 / 32: G = 2 x 768 + 48, three chunks, the first size above the 512 kernels
                      h880  rnn 880 / fc 64 / 64 / 20 / 32: the largest `train_impl` admits (forward LDS 163 776 of 163 840 B),
                            G = 3 x 768 + 336
    refusals        rnn_dims 24 ("multiple of 16") and 896 ("too large for the step kernels' LDS tiles"): WrnnError, every NaN-prefilled
                    output untouched, no recurrence on record, `sync_status` clean

Every default-dims case runs on the team kernels and, after train_force_step_kernels(True), on `gru_*_step_kernel<512>`; twice each,
so the second call replays (the captured step graphs on the step path).  One handle per (mode, dims) for the whole module: the shapes
change from case to case on it, which is the workspace regrow and the graph rebuild of `train_impl`.  `sync_status` after every call:
a timed-out exchange of the team kernels fails the test.

Bounds.  TOL = 2e-5 of the tensor's largest float64 entry on every entry of the 16 gradients, d_mels_up, d_aux and the logits, and
relative on the loss: the bound of test_loop_gradients_from_float64_conditioning for this same comparison, ~25x the float32 noise of
the reference itself on these inputs (torch float32 vs float64: 9.4e-7 at most, test_train_steer_host.py; 1.31e-6 on the sets of the
`<0>` branches, h880 (1, 1): 15x) and >= 50x below what one
omitted (row, step) pair of at most 8 450 moves.  ROW_TOL = 1.3e-4 on every batch row of d_mels_up / d_aux against that row's OWN
largest entry, so that a wrong row with small gradients cannot hide behind a large one: torch's float32 restatement on the same RAW
inputs is off by up to 3.26e-5 per row (B = 130, L = 1; 3.6e-6 at most in the other cases), times 4 for the different summation
order.  Neither figure comes from the kernels.

Measured on the MI355X (n = 8; every case and path in profiles/train_steer.txt), worst over the 57 RAW / 9 MOL runs: loss 5.0e-8 /
3.7e-8, logits 1.1e-6 / 8.5e-7, gradients 1.36e-6 (d_mels_up, B = 130, L = 64, team) / 6.4e-6 (d_aux, generic (35, 7)), per row
1.1e-5 (B = 130, L = 1, both paths: the row torch's float32 is 3.3e-5 off on) / 2.2e-5 (MOL (33, 7), steps).  Team and step kernels
agree with float64 alike.  Sensitivity, tried once against deliberately wrong builds: a backward team kernel that skips the refill of
step 0's inputs fails every team case with L >= 3 (I.weight 0.08 ... 0.39 off), a forward team kernel that hands the second row quad
the first quad's products fails every team case with rpb >= 5 and L >= 2 (1.2e-2 ... 1.7e-2).

The branches of `<0>`, measured alike over their 18 RAW / 2 MOL runs and the h272 split pass: loss 9.0e-8 / 3.4e-8, logits 3.6e-7 /
5.3e-7, gradients 1.36e-6 (d_mels_up, h880 (1, 1): torch's float32 is 1.31e-6 off there) / 2.4e-6 (d_mels_up, MOL h272), per row
1.6e-6 (h48 (33, 3)) / 3.6e-6 (MOL h48); the figures of the cases above did not move by a digit.  Sensitivity, tried once: a
`gru_bwd_step_kernel<0>` that skips its partial last chunk (`if (cw < GB_KC) continue;`) fails all 14 of these runs with L >= 2 and the
h272 split pass (I.weight 1.3e-2 ... 5.2e-2 off) while every earlier case, generic `<0>` at rnn 256 included, still passes.
"""
import numpy as np
import pytest
import torch

from tests import train_steer as ts

TOL = 2e-5
ROW_TOL = 1.3e-4          # 4 x 3.26e-5, see the docstring
PATHS = ('team', 'steps')
RUNS = [(c, p) for c in ts.ALL_CASES for p in (PATHS if c[1] == 'default' else ('steps',))]
_REF = {}                 # the last case's inputs and float64 reference: shared by its paths, never written to


def _run_id(r):
    return f'{ts.case_id(r[0])}-{r[1]}'


@pytest.fixture(scope='module')
def handle_of():
    """(mode, dims name) -> (native handle, number of teams, why the team kernels cannot run or ''); one model per pair, kept for the module."""
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
            models[(mode, dims_name)] = m
        nat = models[(mode, dims_name)]._native_handle()
        ok, n, why = nat.team_info()
        return nat, (n if n >= 1 else 8), ('' if ok else (why or 'team_info: the team kernels cannot run'))

    yield get
    models.clear()


def _inputs(case, n, dev):
    if _REF.get('key') != (case, n):
        mode, dims_name, spec, L = case
        st = ts.steered(mode, ts.batch_of(spec, n), L, ts.case_seed(case), ts.dims_of(dims_name), device=dev)
        _REF.update(key=(case, n), st=st, ref=ts.reference(st, mode, device=dev, d_logits=True))
    return _REF['st'], _REF['ref']


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
        self.nc = self.ps[-1].shape[0]
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self.gs = [torch.full_like(p, nan) for p in self.ps]
        self.dm, self.da = torch.full_like(self.mu, nan), torch.full_like(self.au, nan)
        self.logits = torch.full((self.B, self.L, self.nc), nan, device=dev)
        self.loss, self.loss2 = torch.full((), nan, device=dev), torch.full((), nan, device=dev)

    def ptrs(self, ts_):
        return [t.data_ptr() for t in ts_]

    def got(self):
        g = {k: t.cpu().numpy() for k, t in zip(self.keys, self.gs)}
        g['d_mels_up'], g['d_aux'] = self.dm.cpu().numpy(), self.da.cpu().numpy()
        return g


def _check_grads(tag, got, ref, L):
    worst, where, row_worst = ts.worst_errors(got, ref['grads'])
    print(f'\n{tag} gradients {worst:.2e} ({where}), per row of d_mels_up / d_aux {row_worst:.2e}')
    for k, w in ref['grads'].items():
        assert got[k].shape == w.shape
        err = float(np.abs(got[k] - w).max() / max(np.abs(w).max(), 1e-300))
        assert err <= TOL, (tag, k, err)
    assert row_worst <= ROW_TOL, (tag, row_worst)
    if L == 1:   # h_{-1} = 0: nothing reaches the recurrent weights
        assert not got['rnn1.weight_hh_l0'].any() and not got['rnn2.weight_hh_l0'].any(), tag


@pytest.mark.gpu
@pytest.mark.parametrize('run', RUNS, ids=_run_id)
def test_train_step_equals_float64_on_steered_inputs(run, handle_of):
    case, path = run
    mode, dims_name, spec, L = case
    dev = torch.device('cuda:0')
    nat, n, why_not = handle_of(mode, dims_name)
    if path == 'team' and why_not:
        pytest.skip(why_not)
    st, ref = _inputs(case, n, dev)
    c = _Call(st, mode, dev)
    B = c.B
    try:
        nat.train_force_step_kernels(path == 'steps')
        for _ in range(2):   # the second call replays
            nat.train_step(c.ptrs(c.ps), c.ptrs(c.gs), c.x.data_ptr(), c.mu.data_ptr(), c.au.data_ptr(), c.y.data_ptr(), B, L, c.loss.data_ptr(),
                           c.logits.data_ptr(), c.dm.data_ptr(), c.da.data_ptr(), c.stream)
            nat.sync_status(c.stream)
        nat.train_step(c.ptrs(c.ps), None, c.x.data_ptr(), c.mu.data_ptr(), c.au.data_ptr(), c.y.data_ptr(), B, L, c.loss2.data_ptr(), 0, 0, 0, c.stream)
        nat.sync_status(c.stream)
        if dims_name in ts.BRANCH_DIMS:
            assert nat.train_last_recurrence() == ('steps', 0)
    finally:
        nat.train_force_step_kernels(False)
    loss, loss2 = float(c.loss), float(c.loss2)
    logits = c.logits.cpu().numpy()
    e_loss = abs(loss - ref['loss']) / abs(ref['loss'])
    e_log = float(np.abs(logits - ref['logits']).max() / np.abs(ref['logits']).max())
    tag = f'[steer {ts.case_id(case)} {path}] B={B}: loss {e_loss:.2e}, logits {e_log:.2e},'
    _check_grads(tag, c.got(), ref, L)
    assert e_loss <= TOL, (tag, loss, ref['loss'])
    assert loss2 == loss, (tag, loss, loss2)          # forward + loss only (g = NULL): the same bits
    assert e_log <= TOL, tag


def _split_pass(case, path, handle_of):
    mode, dims_name, spec, L = case
    dev = torch.device('cuda:0')
    nat, n, why_not = handle_of(mode, dims_name)
    if path == 'team' and why_not:
        pytest.skip(why_not)
    st, ref = _inputs(case, n, dev)
    c = _Call(st, mode, dev)
    B = c.B
    dl = torch.from_numpy(ref['d_logits'].astype(np.float32)).to(dev).contiguous()
    try:
        nat.train_force_step_kernels(path == 'steps')
        for _ in range(2):
            nat.train_forward(c.ptrs(c.ps), c.x.data_ptr(), c.mu.data_ptr(), c.au.data_ptr(), B, L, c.logits.data_ptr(), c.stream)
            nat.sync_status(c.stream)
            nat.train_backward(c.ptrs(c.ps), c.ptrs(c.gs), dl.data_ptr(), c.x.data_ptr(), c.mu.data_ptr(), c.au.data_ptr(), B, L, c.dm.data_ptr(),
                               c.da.data_ptr(), c.stream)
            nat.sync_status(c.stream)
    finally:
        nat.train_force_step_kernels(False)
    e_log = float(np.abs(c.logits.cpu().numpy() - ref['logits']).max() / np.abs(ref['logits']).max())
    tag = f'[steer split {ts.case_id(case)} {path}] B={B}: logits {e_log:.2e},'
    _check_grads(tag, c.got(), ref, L)
    assert e_log <= TOL, tag
    return nat


@pytest.mark.gpu
@pytest.mark.parametrize('path', PATHS)
def test_split_pass_from_the_float64_loss_gradient(path, handle_of):
    """train_forward, then train_backward fed d_logits of the float64 reference (rounded to float32): the device loss gradient
    (`ce_grad_kernel`) takes no part, the gradients are held to the same bounds."""
    _split_pass(ts.SPLIT_CASE, path, handle_of)


@pytest.mark.gpu
def test_split_pass_on_a_tail_chunk_of_the_generic_step_kernels(handle_of):
    """The same split pass at rnn 272 (G = 768 + 48), where `gru_bwd_step_kernel<0>` stages a second, 48-column chunk."""
    nat = _split_pass(ts.BRANCH_SPLIT_CASE, 'steps', handle_of)
    assert nat.train_last_recurrence() == ('steps', 0)


@pytest.mark.gpu
@pytest.mark.parametrize('rnn_dims,why', [(24, 'multiple of 16'), (896, "too large for the step kernels' LDS tiles")])
def test_train_step_refuses_the_rnn_dims_the_step_kernels_cannot_run(rnn_dims, why):
    """rnn_dims that is no multiple of 16, and the first multiple of 16 whose forward tile is over the 160 KiB of LDS (880 is the largest
    admitted: RAW-h880-* above): WrnnError that says which, nothing launched -- every output still as prefilled, no recurrence on record."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
    dev = torch.device('cuda:0')
    dims = dict(ts.dims_of('h16'), rnn_dims=rnn_dims)
    sd = make_state_dict(0, mode='RAW', variant='default', **dims)
    rng = np.random.Generator(np.random.PCG64(rnn_dims))
    A, nc = dims['res_out_dims'] // 4, 2 ** dims['bits']
    st = dict(sd={k: np.array(sd[k], np.float32) for k in ts.GRAD_KEYS}, x=rng.uniform(-1, 1, (1, 1)).astype(np.float32),
              mels_up=rng.random((1, 1, dims['feat_dims']), dtype=np.float32), aux=rng.standard_normal((1, 1, 4 * A)).astype(np.float32),
              y=rng.integers(0, nc, size=(1, 1)).astype(np.int64))
    assert st['sd']['rnn1.weight_hh_l0'].shape == (3 * rnn_dims, rnn_dims) and st['sd']['fc3.weight'].shape[0] == nc
    c = _Call(st, 'RAW', dev)
    nat = _cabi.NativeVocoder(**dims, mode='RAW', device=0)
    try:
        with pytest.raises(_cabi.WrnnError) as ei:
            nat.train_step(c.ptrs(c.ps), c.ptrs(c.gs), c.x.data_ptr(), c.mu.data_ptr(), c.au.data_ptr(), c.y.data_ptr(), 1, 1, c.loss.data_ptr(),
                           c.logits.data_ptr(), c.dm.data_ptr(), c.da.data_ptr(), c.stream)
        assert why in str(ei.value), str(ei.value)
        assert nat.lib.wrnn_train_last_recurrence(nat._h, None, None) == -3          # WRNN_ERR_STATE: no training call ran
        nat.sync_status(c.stream)
        for t in c.gs + [c.dm, c.da, c.loss, c.logits]:
            assert bool(torch.isnan(t).all())
    finally:
        nat.close()
