"""The element rule of ``ocm_copy_onesided_accumulate`` in plain torch on the CPU.

This function is the oracle of the rule and its documentation: the gfx950 kernel
(``csrc/src/kernels/xfer_acc.hip``) and the host path (``csrc/include/ocm/acc.h``) must
agree with it bit for bit.

For every element, with ``x`` widened exactly to fp32::

    p = scale * x      (fp32, rounded to nearest even)
    r = acc + p        (fp32, rounded to nearest even)

Two roundings, never one fused multiply-add; subnormals are kept. A NaN result is some
NaN: its payload is not specified.
"""
from __future__ import annotations


def accumulate_reference(acc_f32, x, scale=1.0):
    """acc_f32: fp32 accumulators; x: as many fp32 / bf16 / fp16 elements; scale: a finite
    number (taken as fp32). Returns the new accumulators as a CPU fp32 tensor of acc's shape."""
    import torch

    if acc_f32.dtype != torch.float32:
        raise ValueError("accumulators are float32")
    if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError("accumulate_reference takes float32, bfloat16 or float16 elements")
    acc = acc_f32.detach().cpu()
    xf = x.detach().cpu().reshape(acc.shape).to(torch.float32)
    p = xf * torch.tensor(scale, dtype=torch.float32)  # one rounding
    return acc + p                                      # and another
