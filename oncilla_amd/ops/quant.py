"""The MXFP8 record format of ``ocm_copy_onesided_quant`` in plain torch on the CPU.

These two functions are the oracle of the format and its documentation: the gfx950
kernel (``csrc/src/kernels/xfer_quant.hip``) and the host codec
(``csrc/include/ocm/mx8.h``) must agree with them byte for byte.

Per group of 32 consecutive elements, widened exactly to fp32:

1. ``amax = max |x|``.
2. ``amax == 0``: the scale byte is 127 (``e = 0``).
3. Otherwise ``amax = m * 2**ex`` with ``m`` in [0.5, 1) (frexp), and ``e = ex - 9`` if
   ``m <= 0.875`` else ``ex - 8``: the smallest ``e`` with ``amax * 2**-e <= 448``.
4. ``e`` is clamped to [-127, 127]; the scale byte is ``e + 127`` (E8M0, 255 never written).
5. ``y = clamp(x * 2**-e, -448, 448)`` (exact: a power of two).
6. ``code = RNE(y)`` to OCP e4m3fn, fp8 subnormals kept.

Decoding gives ``float(code) * 2**e`` in fp32, rounded to nearest even into the
element type. A record is the codes followed by the scale bytes.
"""
from __future__ import annotations

GROUP = 32


def mx8_encode_reference(x):
    """x: a bf16 / fp16 tensor whose element count is a multiple of 32.
    Returns (codes_u8 [n], scales_u8 [n / 32]) as CPU uint8 tensors."""
    import torch

    if x.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("mx8_encode_reference takes bfloat16 or float16")
    f = x.detach().cpu().reshape(-1).to(torch.float32)
    if f.numel() % GROUP:
        raise ValueError("element count must be a multiple of 32")
    g = f.view(-1, GROUP)
    amax = g.abs().amax(dim=1)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.875, ex - 9, ex - 8)
    e = torch.where(amax == 0, torch.zeros_like(e), e).clamp(-127, 127).to(torch.int32)
    # x * 2**-e through float64, where every such product is exact; back in fp32 it is the
    # fp32 product (exact too, save for quotients far below the smallest fp8 subnormal)
    y = torch.ldexp(g.double(), -e[:, None]).to(torch.float32).clamp(-448.0, 448.0)
    codes = y.to(torch.float8_e4m3fn).view(torch.uint8).reshape(-1)
    scales = (e + 127).to(torch.uint8)
    return codes.contiguous(), scales.contiguous()


def mx8_decode_reference(codes, scales, dtype):
    """codes [n] and scales [n / 32] (uint8) -> a CPU tensor of n elements of `dtype`."""
    import torch

    if dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("mx8_decode_reference gives bfloat16 or float16")
    c = codes.detach().cpu().reshape(-1).contiguous()
    s = scales.detach().cpu().reshape(-1)
    if c.numel() != s.numel() * GROUP:
        raise ValueError("one scale byte per 32 codes")
    f = c.view(torch.float8_e4m3fn).to(torch.float32).view(-1, GROUP)
    e = s.to(torch.int32) - 127
    # float(code) * 2**e is exact in float64; rounding it to fp32 is the fp32 product
    # (inexact only among fp32 subnormals, where it rounds to nearest even once)
    return torch.ldexp(f.double(), e[:, None]).to(torch.float32).reshape(-1).to(dtype)


def mx8_record_reference(x):
    """The record bytes of x as one uint8 tensor: codes, then scales."""
    import torch

    codes, scales = mx8_encode_reference(x)
    return torch.cat([codes, scales])


def mx8_rows_reference(x2d):
    """The records of a [rows, row_elems] tensor as ``ocm_copy_onesided_quant_strided`` writes
    them, one per row (each row's codes, then its scale bytes): a uint8 tensor
    [rows, row_elems + row_elems / 32]."""
    import torch

    if x2d.dim() != 2:
        raise ValueError("mx8_rows_reference takes a [rows, row_elems] tensor")
    if x2d.shape[0] == 0:
        return torch.zeros((0, x2d.shape[1] + x2d.shape[1] // GROUP), dtype=torch.uint8)
    return torch.stack([mx8_record_reference(row) for row in x2d])
