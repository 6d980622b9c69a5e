"""
The guarded device buffer of the dispatch-path modules (test_conv2d_paths_gpu.py, test_nnops_paths_gpu.py,
test_bn_attention_paths_gpu.py, test_rnn_paths_gpu.py, test_gemm_paths_gpu.py, test_gemm16_paths_gpu.py,
test_augment_paths_gpu.py): a payload inside a larger NaN-filled allocation whose words before and after the payload must
still hold the fill afterwards.
"""
import ctypes

import numpy as np
import torch

GUARD = 64                      # words before and after every output / workspace (256 bytes: keeps 16-byte alignment)
NAN_BITS = 0x7FC00000           # torch.full(..., nan)


class Guarded:
    """`shape` elements inside a larger buffer; everything starts as NaN (0xA5 bytes for uint8).  `shift` moves a float32
    payload that many words past its 16-byte aligned place (a misaligned output); bfloat16 payloads are 8-byte aligned."""

    def __init__(self, shape, dtype=torch.float32, init=None, shift=0):
        n = int(np.prod(shape))
        assert shift == 0 or dtype == torch.float32, "only float32 payloads can be shifted"
        if dtype == torch.uint8:
            self.lo = 4 * GUARD
            self.buf = torch.full((n + 8 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        elif dtype == torch.bfloat16:
            self.lo = 2 * GUARD
            self.buf = torch.full((n + 4 * GUARD,), float("nan"), dtype=torch.bfloat16, device="cuda")
        else:
            self.lo = GUARD + shift
            self.buf = torch.full((n + 2 * GUARD + shift,), float("nan"), dtype=torch.float32, device="cuda")
        self.shift = shift
        self.view = self.buf[self.lo:self.lo + n].view(shape)
        if init is not None:
            self.view.copy_(init)
        self.n = n

    @property
    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def check(self):
        """the words around the payload are untouched"""
        if self.buf.dtype == torch.uint8:
            raw, want = self.buf, 0xA5
        elif self.buf.dtype == torch.bfloat16:
            raw, want = self.buf.view(torch.int16), NAN_BITS >> 16
        else:
            raw, want = self.buf.view(torch.int32), NAN_BITS
        lo, hi = raw[:self.lo], raw[self.lo + self.n:]
        assert hi.numel() == lo.numel() - self.shift and bool((lo == want).all()) and bool((hi == want).all()), "guard words overwritten"

    def numpy(self):
        """the payload, after checking that the words around it are untouched (bfloat16: as float32)"""
        self.check()
        v = self.view.float() if self.buf.dtype == torch.bfloat16 else self.view
        return v.cpu().numpy()
