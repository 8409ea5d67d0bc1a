"""numpy restatement of the device counter RNG (csrc/device_util.h: philox4x32_10 + wrnn_uniform)."""
import numpy as np


def _philox(c, k):
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
    c0, c1, c2, c3 = [x.astype(np.uint32) for x in c]
    k0, k1 = np.uint32(k[0]), np.uint32(k[1])
    with np.errstate(over='ignore'):
        for _ in range(10):
            p0 = M0 * c0.astype(np.uint64)
            p1 = M1 * c2.astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), p0.astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), p1.astype(np.uint32)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
            k0 = np.uint32((int(k0) + int(W0)) & 0xFFFFFFFF)
            k1 = np.uint32((int(k1) + int(W1)) & 0xFFFFFFFF)
    return c0, c1, c2, c3


def _u01(bits):
    """u01_from_bits of device_util.h: (m + 0.5) * 2^-23, m = the top 23 bits (exact in fp32, never 0 or 1)."""
    return ((bits >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 8388608.0)


def philox_uniform_at(seed: int, t, rows, n: int) -> np.ndarray:
    """(len(t), len(rows), n) float32 uniforms identical to wrnn_uniform(seed, t[i], rows[j], k), k < n, for arbitrary
    64-bit steps ``t`` and GLOBAL row indices ``rows``: block counter (t lo, t hi, row, k >> 2), word k & 3 of the block."""
    return _u01(_philox_words_at(seed, t, rows, (n + 3) // 4)[:, :, :n])


def _philox_words_at(seed, t, rows, nblk):
    """uint32 (len(t), len(rows), 4 * nblk): the words x, y, z, w of the blocks (t, row, 0 .. nblk - 1), block-major."""
    t = np.asarray(t, dtype=np.uint64).reshape(-1)[:, None, None]
    r = np.asarray(rows, dtype=np.uint32).reshape(-1)[None, :, None]
    k4 = np.arange(nblk, dtype=np.uint32)[None, None, :]
    shape = (t.shape[0], r.shape[1], nblk)
    c0 = np.broadcast_to((t & np.uint64(0xFFFFFFFF)).astype(np.uint32), shape)
    c1 = np.broadcast_to((t >> np.uint64(32)).astype(np.uint32), shape)
    c2 = np.broadcast_to(r, shape)
    c3 = np.broadcast_to(k4, shape)
    out = _philox((c0, c1, c2, c3), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return np.stack(out, axis=-1).reshape(shape[0], shape[1], -1)


def philox_uniform(seed: int, steps: int, rows: int, n: int) -> np.ndarray:
    """(steps, rows, n) float32 uniforms identical to wrnn_uniform(seed, t, row, k)."""
    return philox_uniform_at(seed, np.arange(steps, dtype=np.uint64), np.arange(rows), n)


# ---- MOL: wrnn_uniform_mol = wrnn_mol_from_u01(wrnn_uniform(...)) = fmaf(w, 1.0f - 2e-5f, 1e-5f) ----------------------------------------
# ONE rounding (the four MOL kernels compile the expression to v_fmamk_f32; csrc/device_util.h spells the fused form out).  numpy has no
# fp32 fma, and float64 arithmetic would round twice, so the replay is exact integer arithmetic: w = (2m + 1) * 2^-24 (m = the top 23
# bits), c = MOL_C * 2^-24, a = MOL_A * 2^-40, so a + w * c = ((2m + 1) * MOL_C + MOL_A * 2^8) * 2^-48 with an integer < 2^49, and the
# int64 -> float32 conversion rounds it once, to nearest even, like the fma.
_MOL_A32 = np.float32(1e-5)                               # 0x3727c5ac
_MOL_C32 = np.float32(1.0) - np.float32(2e-5)             # 0x3f7ffeb0: `1.0f - 2e-5f` is an fp32 subtraction
MOL_A = int(float(_MOL_A32) * 2.0 ** 40)
MOL_C = int(float(_MOL_C32) * 2.0 ** 24)
assert MOL_A * 2.0 ** -40 == float(_MOL_A32) and MOL_C * 2.0 ** -24 == float(_MOL_C32)
assert _MOL_A32.view(np.uint32) == 0x3727C5AC and _MOL_C32.view(np.uint32) == 0x3F7FFEB0


def mol_from_bits(bits) -> np.ndarray:
    """wrnn_mol_from_u01(u01_from_bits(bits)) of device_util.h, bit for bit (bits: uint32 array)."""
    m = (np.asarray(bits, dtype=np.uint32) >> np.uint32(9)).astype(np.int64)
    n = (2 * m + 1) * MOL_C + (MOL_A << 8)
    return n.astype(np.float32) * np.float32(2.0 ** -48)


def philox_mol_uniforms(seed: int, t0: int, n: int, rows):
    """What the MOL kernels feed their logf's in WRNN_NOISE_PHILOX mode for steps [t0, t0 + n) and the given GLOBAL row indices:
    u_mix (n, len(rows), 10) = wrnn_uniform_mol(seed, t, row, 0 .. 9) (the Gumbel draws of the mixture pick) and u_log (n, len(rows)) =
    wrnn_uniform_mol(seed, t, row, 10) (the logistic draw), float32, laid out like the injected-noise arrays the oracle consumes."""
    w = _philox_words_at(seed, np.arange(t0, t0 + n, dtype=np.uint64), rows, 3)
    u = mol_from_bits(w[:, :, :11])
    return np.ascontiguousarray(u[:, :, :10]), np.ascontiguousarray(u[:, :, 10])


def philox_dm_exponentials(seed: int, t0: int, n: int, quant: int = 256) -> np.ndarray:
    """The dual-softmax kernels' draws as DeepmindOracle.generate consumes them: q (n, 2, quant) float32 Exp(1) draws, q = -log u with
    u = wrnn_uniform(seed, t, which, k), which = 0 coarse / 1 fine (the device races logit - logf(-logf(u)); the log here is float64,
    rounded once to fp32, as for RAW)."""
    u = philox_uniform_at(seed, np.arange(t0, t0 + n, dtype=np.uint64), [0, 1], quant)
    return (-np.log(u.astype(np.float64))).astype(np.float32)


def philox_uniform_raw(seed: int, steps: int, rows: int, n: int) -> np.ndarray:
    """(steps, rows, n) uniforms identical to wrnn_uniform_raw(seed, t, row, k):
    block counter (t>>1, row, k>>1), element ((t&1)<<1)|(k&1)."""
    th = (np.arange(steps, dtype=np.uint64) >> np.uint64(1))[:, None, None]
    r = np.arange(rows, dtype=np.uint32)[None, :, None]
    k2 = np.arange((n + 1) // 2, dtype=np.uint32)[None, None, :]
    shape = (steps, rows, k2.shape[-1])
    c0 = np.broadcast_to((th & np.uint64(0xFFFFFFFF)).astype(np.uint32), shape)
    c1 = np.broadcast_to((th >> np.uint64(32)).astype(np.uint32), shape)
    c2 = np.broadcast_to(r, shape)
    c3 = np.broadcast_to(k2, shape)
    x, y, z, w = _philox((c0, c1, c2, c3), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    odd = (np.arange(steps) & 1).astype(bool)[:, None, None]
    e0 = np.where(odd, z, x)   # class 2j
    e1 = np.where(odd, w, y)   # class 2j + 1
    bits = np.stack([e0, e1], axis=-1).reshape(steps, rows, -1)[:, :, :n]
    return _u01(bits)


def _philox_torch(c0, c1, c2, c3, seed):
    """Philox4x32-10 on int64 tensors holding 32-bit words: 32x32 -> 64-bit products in wrapped int64, hi/lo by shift and mask."""
    M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    k0, k1 = seed & MASK, (seed >> 32) & MASK

    def mulhilo(a, m):
        # a < 2^32, m < 2^32: the int64 product wraps modulo 2^64, which keeps all 64 bits of the unsigned product
        lo_part = a * (m & 0xFFFF)                 # < 2^48
        hi_part = a * (m >> 16)                    # < 2^48
        full_lo = (lo_part + ((hi_part & 0xFFFF) << 16))            # bits 0..48 of the product (no wrap: < 2^49)
        lo = full_lo & MASK
        hi = ((hi_part >> 16) + (full_lo >> 32)) & MASK
        return hi, lo
    for _ in range(10):
        hi0, lo0 = mulhilo(c0, M0)
        hi1, lo1 = mulhilo(c2, M1)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_uniform_raw_torch(seed: int, t0: int, n: int, rows, device='cpu'):
    """The same draws as ``philox_uniform_raw`` for steps [t0, t0 + n) and the given GLOBAL row indices, evaluated with
    torch int64 arithmetic (on the GPU when ``device`` says so: the numpy replay of a 110 275-step clip costs minutes of
    host time on some boxes).  Returns a float32 tensor (n, len(rows), 1024) on ``device``.  An independent second
    implementation of the generator's specification: 32x32 -> 64-bit products in wrapped int64, hi/lo by shift and mask."""
    import torch
    MASK = 0xFFFFFFFF
    t = torch.arange(t0, t0 + n, dtype=torch.int64, device=device)
    th = (t >> 1)[:, None, None]
    r = torch.as_tensor(list(rows), dtype=torch.int64, device=device)[None, :, None]
    k2 = torch.arange(512, dtype=torch.int64, device=device)[None, None, :]
    shape = (n, r.shape[1], 512)
    c0 = (th & MASK).expand(shape).clone()
    c1 = ((th >> 32) & MASK).expand(shape).clone()
    c2 = r.expand(shape).clone()
    c3 = k2.expand(shape).clone()
    c0, c1, c2, c3 = _philox_torch(c0, c1, c2, c3, seed)
    odd = (t & 1).bool()[:, None, None]
    e0 = torch.where(odd, c2, c0)   # x | z : class 2j
    e1 = torch.where(odd, c3, c1)   # y | w : class 2j + 1
    bits = torch.stack([e0, e1], dim=-1).reshape(n, r.shape[1], 1024)
    return ((bits >> 9).to(torch.float32) + 0.5) * (1.0 / 8388608.0)


def mol_from_bits_torch(bits):
    """``mol_from_bits`` on an int64 tensor of 32-bit words (same integer arithmetic, one int64 -> float32 rounding)."""
    import torch
    m = bits >> 9
    return ((2 * m + 1) * MOL_C + (MOL_A << 8)).to(torch.float32) * (2.0 ** -48)


def philox_mol_uniforms_torch(seed: int, t0: int, n: int, rows, device='cpu'):
    """``philox_mol_uniforms`` with torch int64 arithmetic (on the GPU when ``device`` says so), an independent second implementation:
    float32 tensors u_mix (n, len(rows), 10), u_log (n, len(rows)) on ``device``."""
    import torch
    MASK = 0xFFFFFFFF
    t = torch.arange(t0, t0 + n, dtype=torch.int64, device=device)[:, None, None]
    r = torch.as_tensor(list(rows), dtype=torch.int64, device=device)[None, :, None]
    k4 = torch.arange(3, dtype=torch.int64, device=device)[None, None, :]
    shape = (n, r.shape[1], 3)
    words = _philox_torch((t & MASK).expand(shape).clone(), ((t >> 32) & MASK).expand(shape).clone(), r.expand(shape).clone(),
                          k4.expand(shape).clone(), seed)
    u = mol_from_bits_torch(torch.stack(words, dim=-1).reshape(n, r.shape[1], 12)[:, :, :11])
    return u[:, :, :10].contiguous(), u[:, :, 10].contiguous()
