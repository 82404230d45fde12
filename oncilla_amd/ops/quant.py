"""The record formats of ``ocm_copy_onesided_quant`` in plain torch on the CPU: MXFP8
first, MXFP4 below.

These functions are the oracle of the format and its documentation: the gfx950
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

A get decodes whatever record it finds, one of another producer too: every code under
every scale byte 0..255 decodes by the line above (scale byte 255 is ``e = 128``:
infinities, and zero for the zero codes; scale byte 0 gives fp32 subnormal products,
rounded once). A NaN code (``0x7f``, ``0xff``) decodes to some NaN of the element type;
the payload is not specified.

The MXFP4 format (``OCM_QUANT_MXFP4``, the ``mx4_*`` functions; host codec
``csrc/include/ocm/mx4.h``) differs in the code alone. Per group of 32 elements:

1. ``amax`` and ``e`` as above, but ``e = ex - 3`` if ``m <= 0.75`` else ``ex - 2``: the
   smallest ``e`` with ``amax * 2**-e <= 6``; clamped to [-127, 127], scale byte ``e + 127``.
2. ``y = clamp(x * 2**-e, -6, 6)``; ``code = RNE(y)`` to OCP E2M1: bit 3 is the sign, the
   magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 are codes 0 to 7, a tie goes to the even code, and
   ``-0`` (as everything that rounds to zero from below) keeps its sign.
3. Decoding gives ``value(code) * 2**e`` in fp32 (exact), rounded to nearest even into the
   element type: fp16 overflows to infinity and underflows through its subnormals.
   This holds for every code byte under every scale byte 0..254. Scale byte 255 is E8M0's
   NaN: it is never written, and what it decodes to is not specified for MXFP4 (the gfx950
   fp4 converts take the scale as the exponent field of an operand; this function gives
   ``value(code) * 2**128``). Observed once on an MI355X, as a record and no promise: the
   kernel returned a NaN for every code, zero codes included (bf16 ``0xffc0``, fp16 ``0xfe00``).

An MXFP4 record of n elements is n / 2 code bytes (element 2i in the low nibble of byte i,
element 2i + 1 in the high nibble), then n / 32 scale bytes.
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


# ---- MXFP4 ----

def _e2m1_values():
    import torch

    return torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float32)


def mx4_encode_reference(x):
    """x: a bf16 / fp16 tensor whose element count is a multiple of 32.
    Returns (codes_u8 [n / 2], scales_u8 [n / 32]) as CPU uint8 tensors; integer and float
    ops only (no torch fp4 dtype)."""
    import torch

    if x.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("mx4_encode_reference takes bfloat16 or float16")
    f = x.detach().cpu().reshape(-1).to(torch.float32)
    if f.numel() % GROUP:
        raise ValueError("element count must be a multiple of 32")
    g = f.view(-1, GROUP)
    amax = g.abs().amax(dim=1)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.75, ex - 3, ex - 2)
    e = torch.where(amax == 0, torch.zeros_like(e), e).clamp(-127, 127).to(torch.int32)
    # x * 2**-e through float64, where every such product is exact
    y = torch.ldexp(g.double(), -e[:, None]).clamp(-6.0, 6.0)
    a = y.abs()
    # the magnitude code: how many of the midpoints between neighbouring values |y| has passed.
    # A tie stays below a midpoint whose lower neighbour is the even code (0.25, 1.25, 2.5, 5.0)
    # and passes one whose upper neighbour is (0.75, 1.75, 3.5).
    mag = torch.zeros_like(a, dtype=torch.int32)
    for mid, up_on_tie in ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False)):
        mag += ((a >= mid) if up_on_tie else (a > mid)).to(torch.int32)
    sign = torch.signbit(y).to(torch.int32) << 3
    nib = (sign | mag).to(torch.uint8).reshape(-1, 2)
    codes = nib[:, 0] | (nib[:, 1] << 4)
    scales = (e + 127).to(torch.uint8)
    return codes.contiguous(), scales.contiguous()


def mx4_decode_reference(codes, scales, dtype):
    """codes [n / 2] and scales [n / 32] (uint8) -> a CPU tensor of n elements of `dtype`."""
    import torch

    if dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("mx4_decode_reference gives bfloat16 or float16")
    c = codes.detach().cpu().reshape(-1).contiguous()
    s = scales.detach().cpu().reshape(-1)
    if 2 * c.numel() != s.numel() * GROUP:
        raise ValueError("one scale byte per 16 code bytes")
    nib = torch.stack([c & 15, c >> 4], dim=1).reshape(-1).to(torch.int64)
    v = _e2m1_values()[nib & 7]
    v = torch.where((nib & 8) != 0, -v, v).view(-1, GROUP)
    e = s.to(torch.int32) - 127
    # value(code) * 2**e is exact in float64 and in fp32 (one or two significant bits)
    return torch.ldexp(v.double(), e[:, None]).to(torch.float32).reshape(-1).to(dtype)


def mx4_record_reference(x):
    """The MXFP4 record bytes of x as one uint8 tensor: codes, then scales."""
    import torch

    codes, scales = mx4_encode_reference(x)
    return torch.cat([codes, scales])


def mx4_rows_reference(x2d):
    """The MXFP4 records of a [rows, row_elems] tensor as ``ocm_copy_onesided_quant_strided``
    writes them, one per row: a uint8 tensor [rows, row_elems / 2 + row_elems / 32]."""
    import torch

    if x2d.dim() != 2:
        raise ValueError("mx4_rows_reference takes a [rows, row_elems] tensor")
    if x2d.shape[0] == 0:
        return torch.zeros((0, x2d.shape[1] // 2 + x2d.shape[1] // GROUP), dtype=torch.uint8)
    return torch.stack([mx4_record_reference(row) for row in x2d])
