"""Raw access to the gfx950 transfer kernels (tests, micro-benchmarks), and the torch
oracles of the MXFP8 and MXFP4 record formats and of the accumulate rule."""
from .acc import accumulate_reference
from .quant import (mx4_decode_reference, mx4_encode_reference, mx4_record_reference, mx4_rows_reference, mx8_decode_reference, mx8_encode_reference, mx8_record_reference, mx8_rows_reference)
from .xfer import XFER_AUTO, XFER_LDS, XFER_PCIE, XFER_PUSH, XFER_REG, batch, device_copy_seconds, striped_reference, xfer

__all__ = ["accumulate_reference", "XFER_AUTO", "XFER_LDS", "XFER_PCIE", "XFER_PUSH", "XFER_REG", "batch", "device_copy_seconds", "striped_reference", "xfer",
           "mx8_decode_reference", "mx8_encode_reference", "mx8_record_reference", "mx8_rows_reference",
           "mx4_decode_reference", "mx4_encode_reference", "mx4_record_reference", "mx4_rows_reference"]
