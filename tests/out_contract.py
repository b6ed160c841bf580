"""Guard bands for result buffers: a result view inside a larger buffer pre-filled with one
sentinel bit pattern, and the report of every element beside the view -- before it, after it, or
in a gap between its strides -- that no longer holds the sentinel.  Shared by
tests/test_out_contract_host.py and tests/test_gpu_out_contract.py; a test helper, not part of the
product.

The sentinel is a quiet NaN with a payload no kernel of the project produces (their NaNs are the
canonical 0x7FF8000000000000 / 0x7FC00000, a copied operand's, or the hardware's default); it is
written and compared on an integer view, so that neither NaN != NaN nor a payload-dropping copy
can hide a store.
"""

import numpy as np
import torch

GUARD = 4096  # elements before and after the view: far more than one block stores at test sizes
SENTINEL = {torch.float64: 0x7FF80C0FFEE0BAD5, torch.float32: 0x7FC5BAD5}
_INT = {torch.float64: torch.int64, torch.float32: torch.int32}


def strides_of(shape):
    """C-contiguous strides, in elements"""
    out, step = [], 1
    for n in reversed(shape):
        out.append(step)
        step *= max(int(n), 1)
    return tuple(reversed(out))


class Guarded:
    """``view``: a tensor of ``shape`` / ``strides`` (default C-contiguous; in elements) that starts
    ``GUARD + offset`` elements into ``buf``, a 1-D sentinel-filled tensor ending ``GUARD`` elements
    past the view's last element.  ``buf`` starts on the allocator's boundary (16-byte aligned at
    the least), and GUARD elements are a multiple of 16 bytes: ``offset`` 0 gives an aligned view,
    ``offset`` 1 one that starts one element past an aligned address."""

    def __init__(self, shape, dtype, device="cpu", offset=0, strides=None, guard=GUARD):
        shape = tuple(int(n) for n in shape)
        strides = strides_of(shape) if strides is None else tuple(int(s) for s in strides)
        assert len(strides) == len(shape) and all(n > 0 for n in shape)
        self.start = guard + int(offset)
        self.span = 1 + sum((n - 1) * s for n, s in zip(shape, strides))
        self.sentinel = SENTINEL[dtype]
        self.buf = torch.empty(self.start + self.span + guard, dtype=dtype, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.buf.view(_INT[dtype]).fill_(self.sentinel)
        self.view = self.buf.as_strided(shape, strides, self.start)
        inside = np.zeros(1, dtype=np.int64)
        for n, s in zip(shape, strides):
            inside = (inside[:, None] + np.arange(n, dtype=np.int64) * s).reshape(-1)
        self._inside = inside  # offsets of the view's elements from its first

    def _bits(self):
        return self.buf.cpu().numpy().view(np.int64 if self.buf.dtype == torch.float64 else np.int32)

    def changed(self):
        """Offsets, in elements from the view's first element (negative: before it), of every
        element outside the view that no longer holds the sentinel bits; ascending."""
        differs = self._bits() != self.sentinel
        differs[self.start + self._inside] = False
        return [int(i) - self.start for i in np.flatnonzero(differs)]

    def unwritten(self):
        """How many elements of the view still hold the sentinel bits (a skipped store)."""
        return int((self._bits()[self.start + self._inside] == self.sentinel).sum())

    def assert_intact(self, what=""):
        bad = self.changed()
        assert not bad, (f"{what}: {len(bad)} element(s) beside the result were written, at offsets "
                         f"{bad[:16]} from its first element (the view spans {self.span})")
