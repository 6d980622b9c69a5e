"""
Sparse device operands for tests/test_gemm_far_gpu.py: a rows descriptor whose strides put its last row gigabytes behind its base,
inside ONE allocation

    [front margin: 2^31 + 256 bytes][extent][256 bytes]

filled with the NaN pattern of guarded.py (0x7FC0 in every element while the arena holds bfloat16 rows); the base a kernel gets is
the start of the extent.  A 32-bit byte offset that a kernel
sign-extends lands in the front margin, one it truncates lands inside the extent: both read NaN or a foreign row and neither leaves
the allocation (tests/test_oracle_gemm_paths.py proves that on the CPU for every row and every planted mistake).

Payload rows are written with one copy_ into a torch.as_strided view (64-bit strides, storage offset = the margin) and read back the
same way; an extent is never copied to the host.  After a call, changed_words() counts on the device, in chunks, the words of the
whole allocation that no longer hold the fill: for an input that must be the payload's size with the payload bit-identical, for C
exactly the M x N payload positions.
"""
import ctypes

import torch

from guarded import NAN_BITS

MARGIN = (1 << 31) + 256            # bytes in front of the base
TAIL = 256                          # bytes behind the extent
CHUNK = 1 << 27                     # words per counting step (512 MiB read, a 128 MiB temporary)


NAN16X2 = 0x7FC07FC0                # two bfloat16 NaN: the fill of an arena that holds a bf16 operand


class Arena:
    """one allocation that holds a far operand of up to `extent_bytes`; reused by every case of a module.  It holds float32 rows
    (fill NAN_BITS) until refill(bf16=True) makes it hold bfloat16 rows (fill 0x7FC0 in every element)."""

    def __init__(self, extent_bytes):
        assert extent_bytes % 16 == 0
        self.extent = extent_bytes
        self.words = torch.empty((MARGIN + extent_bytes + TAIL) // 4, dtype=torch.int32, device="cuda")
        self.refill()
        assert (self.words.data_ptr() + MARGIN) % 16 == 0

    def refill(self, bf16=False):
        self.dtype = torch.bfloat16 if bf16 else torch.float32
        self.fill = NAN16X2 if bf16 else NAN_BITS
        self.words.fill_(self.fill)

    @property
    def base(self):
        return self.words.data_ptr() + MARGIN

    @property
    def ptr(self):
        return ctypes.c_void_p(self.base)

    def _view(self, t, d, cols):
        """[batch, rpb, cols] through the descriptor's own strides (in elements of t)"""
        size = t.element_size()
        last = (d["batch"] - 1) * d["bs"] + (d["rpb"] - 1) * d["rs"] + cols
        assert d["bs"] >= 0 and d["rs"] >= 0 and last * size <= self.extent, "the descriptor does not fit the arena"
        return torch.as_strided(t, (d["batch"], d["rpb"], cols), (d["bs"], d["rs"], 1), MARGIN // size)

    def put(self, d, cols, payload):
        """payload: a device or host tensor / array of [M, cols] float32 values (bf16 values for a bf16 arena); rows must not overlap"""
        p = torch.as_tensor(payload, dtype=torch.float32).to("cuda").to(self.dtype).reshape(d["batch"], d["rpb"], cols)
        self._view(self.words.view(self.dtype), d, cols).copy_(p)
        return p.reshape(-1, cols)

    def get(self, d, cols):
        return self._view(self.words.view(self.dtype), d, cols).reshape(-1, cols).clone()

    def same_bits(self, d, cols, payload):
        bits = torch.int32 if self.dtype == torch.float32 else torch.int16
        return bool(torch.equal(self.get(d, cols).view(bits), payload.reshape(-1, cols).view(bits)))

    def clear(self, d, cols):
        if self.dtype == torch.float32:
            self._view(self.words, d, cols).fill_(NAN_BITS)
        else:
            self._view(self.words.view(torch.int16), d, cols).fill_(NAN16X2 & 0xFFFF)

    def changed_words(self):
        """32-bit words of the whole allocation, margins included, that differ from the fill"""
        n = torch.zeros((), dtype=torch.int64, device="cuda")
        for lo in range(0, self.words.numel(), CHUNK):
            n += torch.count_nonzero(self.words[lo:lo + CHUNK] != self.fill)
        return int(n.item())
