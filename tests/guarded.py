"""Guarded memory for the workspace-contract tests: one allocation (the arena), regions carved out of it with at least ``GUARD`` bytes of
untouched pattern on each side, and a check that the pattern is still there.  Works on CPU and device tensors alike.

Why an arena of the test's own: a kernel that writes one slab, one padded fragment tile or one counter past the end of a
``torch.empty(exactly the declared size)`` lands in the caching allocator's slack or in a neighbour's tensor and nothing notices.  Here
every buffer of a call -- inputs, outputs and the workspace -- is a region of ONE arena, so an overrun of the sizes in question (far below
``GUARD``) lands in bytes this test owns and ``Arena.check()`` names the region, the side and the first and last offset touched.

The patterns are 0xFF and 0x00 ONLY.  As f32 and bf16 they read NaN and 0, as an int32 / int64 index -1 and 0: a kernel that uses a stale
word of a poisoned workspace as an index therefore stays within one element of the pointer it offsets, inside the arena.  Never add a
pattern whose integer reading is large: these tests must not be able to send a kernel to an unmapped address.

``guarded_empty`` routes the device allocations of product modules (``torch.empty`` / ``torch.empty_like`` as those modules look them up)
through an arena for the duration of a call."""
from __future__ import annotations

import contextlib

import torch

GUARD = 1 << 20
PATTERNS = (0xFF, 0x00)


def _pattern(value: int) -> int:
    if value not in PATTERNS:
        raise ValueError(f"fill patterns are 0xFF and 0x00 only (got {value!r}): an index read from one must stay inside the arena")
    return value


class Arena:
    """``Arena(device, nbytes, pattern=0xFF)``: one ``uint8`` allocation filled with ``pattern``; ``region()`` hands out views."""

    def __init__(self, device, nbytes: int, pattern: int = 0xFF):
        self.pattern = _pattern(pattern)
        self.buf = torch.full((int(nbytes),), self.pattern, dtype=torch.uint8, device=device)
        if self.buf.is_cuda:
            torch.cuda.synchronize(self.buf.device)          # regions are handed to side streams too: the pattern is there before any of them runs
        self.regions = []                      # (name, start, end) in ascending order; the gaps between them are the guards
        self._cursor = 0

    def region(self, nbytes: int, align: int = 256, shift: int = 0, fill: int | None = None, name: str | None = None) -> torch.Tensor:
        """A ``uint8`` view of ``nbytes`` bytes whose address is ``shift`` modulo ``align``, at least ``GUARD`` bytes behind the previous
        region and in front of the arena's end.  ``fill`` (0xFF / 0x00) overwrites the region; ``None`` leaves the arena's pattern."""
        if align < 1 or not 0 <= shift < align:
            raise ValueError(f"need 0 <= shift < align (got shift {shift}, align {align})")
        base = self.buf.data_ptr()
        addr = base + self._cursor + GUARD
        addr += (shift - addr) % align
        start, end = addr - base, addr - base + int(nbytes)
        if end + GUARD > self.buf.numel():
            raise MemoryError(f"arena of {self.buf.numel()} bytes is full: region {name!r} of {nbytes} bytes needs {end + GUARD}")
        self.regions.append((name if name is not None else f"#{len(self.regions)}", start, end))
        self._cursor = end
        view = self.buf[start:end]
        if fill is not None:
            view.fill_(_pattern(fill))
        return view

    def typed(self, shape, dtype, align: int = 256, shift: int = 0, fill: int | None = 0xFF, name: str | None = None) -> torch.Tensor:
        """A region viewed as ``dtype`` in ``shape`` (filled 0xFF by default: NaN as a float, -1 as an index)"""
        n = 1
        for s in shape:
            n *= int(s)
        return self.region(n * torch.empty((), dtype=dtype).element_size(), align, shift, fill, name).view(dtype).view(*shape)

    def put(self, tensor: torch.Tensor, align: int = 256, shift: int = 0, name: str | None = None) -> torch.Tensor:
        """A region holding a copy of ``tensor`` (an input of the call under test)"""
        t = tensor.contiguous()
        out = self.typed(t.shape, t.dtype, align, shift, None, name)
        out.copy_(t)
        return out

    def violations(self) -> list:
        """[(region name, 'before' | 'behind', first offset, last offset)]: offsets count bytes from the region's edge, from 1"""
        touched = self.buf != self.pattern
        for _, start, end in self.regions:
            touched[start:end] = False
        if not bool(touched.any()):
            return []
        found, n = [], self.buf.numel()
        edges = [(None, 0, 0)] + self.regions + [(None, n, n)]
        for (prev, _, lo), (nxt, hi, _) in zip(edges[:-1], edges[1:]):
            at = touched[lo:hi].nonzero().flatten()
            if at.numel() == 0:
                continue
            at = at.cpu() + lo
            mid = hi if prev is not None and nxt is None else (lo if prev is None else (lo + hi) // 2)
            behind, before = at[at < mid], at[at >= mid]
            if behind.numel():
                found.append((prev, "behind", int(behind[0]) - lo + 1, int(behind[-1]) - lo + 1))
            if before.numel():
                found.append((nxt, "before", hi - int(before[-1]), hi - int(before[0])))
        return found

    def check(self) -> None:
        """Every guard byte still holds the pattern"""
        found = self.violations()
        assert not found, "guard bytes were written: " + "; ".join(
            f"region {name!r}: {side} it, bytes {first} .. {last} from its edge" for name, side, first, last in found)


def arena_for(device, *nbytes: int) -> Arena:
    """An arena with room for one region of each of ``nbytes`` bytes, guards and alignment included"""
    return Arena(device, sum(int(n) for n in nbytes) + (len(nbytes) + 1) * (GUARD + 256))


def is_fill(t: torch.Tensor, pattern: int = 0xFF) -> bool:
    """every byte of ``t`` (a view of a region) still holds ``pattern``: as 0xFF, NaN in every float"""
    return bool((t.contiguous().view(torch.uint8) == _pattern(pattern)).all())


class _TorchView:
    """The ``torch`` a patched module sees: ``empty`` / ``empty_like`` replaced, everything else the real module's"""

    def __init__(self, empty, empty_like):
        self.empty, self.empty_like = empty, empty_like

    def __getattr__(self, name):
        return getattr(torch, name)


@contextlib.contextmanager
def guarded_empty(arena: Arena, fill: int, modules, align: int = 256, shift: int = 0, log: list | None = None, reuse: list | None = None):
    """While active, ``torch.empty`` / ``torch.empty_like`` as looked up by ``modules`` (they say ``torch.empty``: their global ``torch`` is
    replaced) take every allocation on the arena's device from a region of ``arena`` filled with ``fill``; CPU and pinned allocations pass
    through untouched; every region's address is ``shift`` modulo ``align``.  Only the modules' name is patched, nothing process-wide.

    ``log``: every tensor handed out is appended to it.  ``reuse``: a list of such tensors whose work has ended; the allocations of this
    context get THEM, in order and as they are (same shapes and dtypes, no fill) -- what the caching allocator does to a pipeline's
    blocks: the bytes a call finds are another call's results."""
    _pattern(fill)
    dev = arena.buf.device
    recycled = iter(reuse) if reuse is not None else None

    def on_arena(shape, dtype):
        if recycled is not None:
            t = next(recycled)
            assert tuple(t.shape) == tuple(shape) and t.dtype == dtype, f"allocation {tuple(shape)} {dtype} where {tuple(t.shape)} {t.dtype} was logged"
        else:
            t = arena.typed(tuple(shape), dtype, align, shift, fill, f"empty{tuple(shape)}")
        if log is not None:
            log.append(t)
        return t

    def empty(*size, **kw):
        device = kw.get("device")
        if device is None or torch.device(device).type != dev.type or kw.get("pin_memory"):
            return torch.empty(*size, **kw)
        meta = torch.empty(*size, **{**kw, "device": "meta"})
        return on_arena(meta.shape, meta.dtype)

    def empty_like(t, **kw):
        device = torch.device(kw.get("device", t.device))
        if device.type != dev.type or kw.get("pin_memory"):
            return torch.empty_like(t, **kw)
        return on_arena(t.shape, kw.get("dtype", t.dtype))

    view = _TorchView(empty, empty_like)
    saved = [(m, m.torch) for m in modules]
    try:
        for m, _ in saved:
            m.torch = view
        yield arena
    finally:
        for m, real in saved:
            m.torch = real
