"""Guard bands and poisoned interiors for the buffers the library sizes (workspace, topology, driver states, capacity buffers).

`Arena.take(nbytes, fill)` hands out a uint8 view of EXACTLY `nbytes` with 1 MiB of the byte 0xA5 before it and 1 MiB after it, all
inside one allocation of the test's own, the interior filled with `fill` (0x00, or 0xFF: a NaN as fp32 and fp64, -1 as any integer,
an index far out of range).  A kernel that stores past either end of the buffer then damages a band instead of a neighbour the
caching allocator happened to place there, and `Arena.check()` finds it by comparing bytes; a kernel that reads what nobody wrote
reads the fill, so its outputs differ between the two fills.

The view starts on a 256-byte boundary, the alignment `Carve::take` (csrc/m3g_internal.h: align_up to 256) gives every region of
a carve, so offsets inside the buffer are those the library's carves assume.  Its END is wherever `nbytes` puts it: the band after
begins at the very next byte.

What this cannot see: a stray write farther than 1 MiB from the buffer (the band covers the largest single-tile store of the code,
64 rows x 160 columns x 4 B, many times over; it is a condition, not a measurement), and stray READS outside the buffer, which
return band bytes without a trace unless they reach an output.  tests/test_guarded_cpu.py is the evidence that damage inside the
bands is reported with the right label, side and offsets."""
from __future__ import annotations

import math

import torch

BAND = 1 << 20
PATTERN = 0xA5
ALIGN = 256   # Carve::take: align_up(bytes, 256)


class Arena:
    def __init__(self, device):
        self.device = torch.device(device)
        self._takes = []   # (label, whole allocation, interior offset, nbytes)
        self._pattern = torch.full((BAND,), PATTERN, dtype=torch.uint8, device=self.device)

    def take(self, nbytes: int, fill: int, label: str | None = None) -> torch.Tensor:
        """uint8 view of exactly `nbytes` filled with `fill`, 256-byte aligned, a band of BAND bytes of PATTERN on either side."""
        nbytes = int(nbytes)
        if nbytes < 0 or not 0 <= fill <= 0xFF:
            raise ValueError("take: nbytes >= 0 and a byte value for fill")
        whole = torch.full((BAND + ALIGN + nbytes + BAND,), PATTERN, dtype=torch.uint8, device=self.device)
        off = BAND + (-(whole.data_ptr() + BAND)) % ALIGN
        view = whole[off:off + nbytes]
        view.fill_(fill)
        assert nbytes == 0 or view.data_ptr() % ALIGN == 0
        self._takes.append((label if label is not None else f"buffer {len(self._takes)}", whole, off, nbytes))
        return view

    def take_like(self, shape, dtype: torch.dtype, fill: int, label: str | None = None) -> torch.Tensor:
        """A contiguous tensor of `shape` and `dtype` over a `take` of exactly its bytes."""
        shape = tuple(int(n) for n in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        item = torch.empty((), dtype=dtype).element_size()
        return self.take(math.prod(shape) * item, fill, label).view(dtype).view(shape)

    def take_copy(self, src: torch.Tensor, label: str | None = None) -> torch.Tensor:
        """A guarded contiguous copy of `src` (read-only inputs)."""
        out = self.take_like(src.shape, src.dtype, 0, label)
        out.copy_(src)
        return out

    def spans(self):
        """(label, first byte address, one past the last) of every take's interior."""
        return [(label, whole.data_ptr() + off, whole.data_ptr() + off + n) for label, whole, off, n in self._takes]

    def check(self) -> None:
        """Every band still holds PATTERN; else AssertionError: label, side, first and last damaged byte relative to the buffer's edge
        (before: -1 is the byte just below the buffer; after: +0 is the byte just past its end)."""
        for label, whole, off, nbytes in self._takes:
            for side, lo, edge in (("before", off - BAND, off), ("after", off + nbytes, off + nbytes)):
                band = whole[lo:lo + BAND]
                if torch.equal(band, self._pattern):
                    continue
                bad = torch.nonzero(band != PATTERN).flatten()
                first, last = int(bad[0]) + lo - edge, int(bad[-1]) + lo - edge
                raise AssertionError(f"guard band damaged: {label}, {side}, {first:+d} .. {last:+d} ({int(bad.numel())} bytes differ; "
                                     f"buffer of {nbytes} bytes)")
