"""MI355X: `gemm_bf16_kernel` (csrc/train_gemm_bf16.hip) and `sgemm_kernel` through `debug_train_gemm` -- the GEMM dispatcher and split-K
wrapper of the training calls -- against float64.  This is the proof of the bf16 kernel: the end-to-end comparison of
tests/test_gpu_train_bf16.py cannot be tight, this one is.

Expected value.  bf16: the float64 product of torch's float32 -> bfloat16 -> float64 conversions of the operands (round to nearest
even), plus bias, plus the C input where beta = 1, then ReLU.  f32: the same on the unrounded operands.

Bound, derived, not measured; per element, evaluated in float64:

    (K + 4) * 2^-24 * (|A| . |B| + |bias| + |C_in|)        (A, B as the kernel uses them: rounded for bf16)

A product of two bf16 values (8 significand bits each) is exact in float32, and a float32 product rounds once (2^-24 relative), so
what remains is the K - 1 roundings of the accumulation, in any order, the fp32 split-K sum, the bias add, the beta add and the store: at
most K + 4 roundings of partial sums that never exceed |A| . |B| + |bias| + |C_in|.  A bf16 ulp is 2^-8 relative: with K <= 4096 the
bound is four orders below it, so a truncating conversion, a swapped operand lane map, a missed rounding or an accumulator rounded
to bf16 all fail.  Exact ties (1 + 2^-8, 1 + 3 * 2^-8 and their negatives: nearest even sends them to 1 and 1 + 2^-6, truncation and
round-half-up do not) are planted in both operands.  Operands are normal numbers of order 1: no claim about bf16 subnormals.

Shapes: the smallest at which something can still go wrong -- one element; fewer rows / columns / k than a tile, an MFMA tile or a k pair
(7, 30, 33); one past a block tile (129, 130); several blocks (200 x 1536); K = 30 (MOL's fc3) and K = 455 (no multiple of the k tile)
-- with the operand placements of `train_impl`: B = W + 1 with ldb = 113 (a column block of I.weight: 4-byte alignment only, odd
leading dimension), lda > K, B = W + 512 with ldb = 544, ldc > N, and split K with 1, 3, 64 (slices past the end of K) and 0 (the
wrapper's choice) slices.
"""
import numpy as np
import pytest
import torch

# (form, M, N, K, extras): NT = A (M, K) . B (N, K)^T, NN = A (M, K) . B (K, N), TN = A (K, M)^T . B (K, N)
NT = [(1, 1, 1), (7, 30, 33), (129, 130, 32), (200, 96, 80), (63, 1536, 512)]
NN = [(7, 32, 30), (129, 80, 512), (200, 512, 1536)]
TN = [(30, 512, 7), (512, 1, 63), (1536, 32, 455), (1536, 512, 455)]
NT_VARIANTS = [dict(), dict(bias=True), dict(beta=True), dict(bias=True, relu=True), dict(bias=True, beta=True, relu=True)]
CALLS = [('NT', s, v) for s in NT for v in NT_VARIANTS[:(5 if s[2] <= 80 else 2)]] + [('NN', s, v) for s in NN for v in (dict(), dict(beta=True))] + \
        [('TN', s, dict(slices=sl)) for s in TN for sl in (1, 3, 64, 0)]
TIES = (1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8))


def _call_id(c):
    return f'{c[0]}-{"x".join(map(str, c[1]))}' + ''.join(f'-{k}{"" if v is True else v}' for k, v in c[2].items())


@pytest.fixture(scope='module')
def nat():
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS
    h = _cabi.NativeVocoder(device=0, mode='RAW', **DEFAULT_DIMS)
    yield h
    h.close()


def _operand(rng, rows, cols, ld, off):
    """(storage, view): a (rows, cols) float32 matrix of order-1 normal values at float offset `off` of a buffer with row pitch ld,
    exact bf16 ties planted; the rest of the buffer is NaN (a read outside the operand poisons the result)."""
    buf = np.full(off + rows * ld, np.nan, np.float32)
    v = rng.uniform(0.5, 2.0, size=(rows, cols)).astype(np.float32) * rng.choice(np.float32([-1, 1]), size=(rows, cols))
    flat = v.reshape(-1)
    where = rng.permutation(flat.size)[:max(1, flat.size // 7)]
    flat[where] = np.float32(TIES)[np.arange(where.size) % 4]
    view = np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, cols), strides=(4 * ld, 4))
    view[:] = v
    return buf, v


def _bf64(a):
    return torch.from_numpy(a).to(torch.bfloat16).to(torch.float64)


def _run(nat, precision, call, seed):
    form, (M, N, K), ex = call
    rng = np.random.Generator(np.random.PCG64(seed))
    dev = torch.device('cuda:0')
    ta, tb = form == 'TN', form == 'NT'
    if form == 'NT':
        lda, (ldb, boff) = K + 3, (113, 1) if K <= 112 else (K + 1, 1)   # B = W + 1, ldb = 113: a column block of I.weight
        a_shape, b_shape = (M, K), (N, K)
    elif form == 'NN':
        lda, (ldb, boff) = K + 5, (544, 512) if N <= 32 else (N + 32, 512)   # B = W + 512 (fc1.weight's aux block: ldb = 544)
        a_shape, b_shape = (M, K), (K, N)
    else:
        lda, (ldb, boff) = M + 1, (N + 3, 0)
        a_shape, b_shape = (K, M), (K, N)
    ldc = N + 3
    abuf, a = _operand(rng, a_shape[0], a_shape[1], lda, 3)
    bbuf, b = _operand(rng, b_shape[0], b_shape[1], ldb, boff)
    bias = rng.standard_normal(N).astype(np.float32) if ex.get('bias') else None
    cin = rng.standard_normal((M, ldc)).astype(np.float32)
    A_d, B_d, C_d = torch.from_numpy(abuf).to(dev), torch.from_numpy(bbuf).to(dev), torch.from_numpy(cin).to(dev)
    bias_d = torch.from_numpy(bias).to(dev) if bias is not None else None
    st = torch.cuda.current_stream(dev).cuda_stream
    nat.debug_train_gemm(precision, ta, tb, A_d.data_ptr() + 4 * 3, lda, B_d.data_ptr() + 4 * boff, ldb, C_d.data_ptr(), ldc, M, N, K,
                         beta=bool(ex.get('beta')), bias_ptr=bias_d.data_ptr() if bias is not None else 0, relu=bool(ex.get('relu')),
                         slices=ex.get('slices', 1), stream=st)
    torch.cuda.synchronize(dev)
    got = C_d.cpu().numpy().astype(np.float64)
    conv = _bf64 if precision == 'bf16' else (lambda t: torch.from_numpy(t).to(torch.float64))
    a64, b64 = conv(a), conv(b)
    a64 = a64.t() if ta else a64
    b64 = b64.t() if tb else b64
    want = (a64 @ b64).numpy()
    mag = (a64.abs() @ b64.abs()).numpy()
    if bias is not None:
        want, mag = want + bias.astype(np.float64), mag + np.abs(bias.astype(np.float64))
    if ex.get('beta'):
        want, mag = want + cin[:, :N].astype(np.float64), mag + np.abs(cin[:, :N].astype(np.float64))
    if ex.get('relu'):
        want = np.maximum(want, 0.0)
    bound = (K + 4) * 2.0 ** -24 * mag
    err = np.abs(got[:, :N] - want)
    worst = float((err / bound).max())
    print(f'\n[train gemm {precision} {_call_id(call)}] worst error / bound {worst:.3f}, largest error {err.max():.2e}')
    assert np.array_equal(got[:, N:], cin[:, N:].astype(np.float64)), 'wrote past column N of C'
    assert np.isfinite(got[:, :N]).all()
    assert worst <= 1.0, (precision, _call_id(call), worst)
    if ex.get('relu'):
        assert (got[:, :N] >= 0).all()
        if M * N >= 64:   # both arms taken
            assert (got[:, :N] == 0).any() and (got[:, :N] > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize('call', CALLS, ids=_call_id)
def test_bf16_gemm_is_the_float64_product_of_bf16_rounded_operands(call, nat):
    _run(nat, 'bf16', call, 1000 + CALLS.index(call))


@pytest.mark.gpu
@pytest.mark.parametrize('call', CALLS, ids=_call_id)
def test_f32_gemm_is_the_float64_product_of_the_operands(call, nat):
    _run(nat, 'f32', call, 1000 + CALLS.index(call))


@pytest.mark.gpu
def test_bf16_rounding_is_visible_at_this_bound(nat):
    """The bound tells bf16 operands from unrounded ones: on the same operands the f32 kernel's product is hundreds of bounds away from
    the bf16 expectation, so a kernel that skipped the rounding could not pass the test above."""
    M, N, K = 7, 30, 33
    rng = np.random.Generator(np.random.PCG64(5))
    dev = torch.device('cuda:0')
    _, a = _operand(rng, M, K, K, 0)
    _, b = _operand(rng, N, K, K, 0)
    A_d, B_d, C_d = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), torch.zeros(M, N, device=dev)
    nat.debug_train_gemm('f32', False, True, A_d.data_ptr(), K, B_d.data_ptr(), K, C_d.data_ptr(), N, M, N, K,
                         stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    want = (_bf64(a) @ _bf64(b).t()).numpy()
    mag = (_bf64(a).abs() @ _bf64(b).abs().t()).numpy()
    ratio = np.abs(C_d.cpu().numpy() - want) / ((K + 4) * 2.0 ** -24 * mag)
    assert ratio.max() > 100.0, float(ratio.max())


@pytest.mark.gpu
def test_tt_in_bf16_is_unsupported(nat):
    from tacotronv2_wavernn_chinese_amd import _cabi
    dev = torch.device('cuda:0')
    t = torch.zeros(64, device=dev)
    with pytest.raises(_cabi.WrnnError) as e:
        nat.debug_train_gemm('bf16', True, True, t.data_ptr(), 8, t.data_ptr(), 8, t.data_ptr(), 8, 8, 8, 8)
    assert e.value.code == _cabi.ERR_UNSUPPORTED
