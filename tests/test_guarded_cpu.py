"""tests/guarded.py on the CPU: the arena's teeth (a write one byte outside a region is reported with the right region, side and
offsets), the address residue of a region, what two fills change, and the ``torch.empty`` patch of a module."""
import types

import pytest
import torch

from tests import guarded
from tests.guarded import GUARD, Arena


def _arena(pattern=0xFF, regions=3):
    return Arena("cpu", regions * (GUARD + 4096) + GUARD + 4096, pattern)


@pytest.mark.parametrize("pattern", [0xFF, 0x00])
def test_clean_arena_passes_and_writes_inside_regions_are_free(pattern):
    a = _arena(pattern)
    r = [a.region(n, name=f"r{n}") for n in (1, 1000, 4096)]
    for t in r:
        t.fill_(0x5A)
    a.check()
    assert a.violations() == []


@pytest.mark.parametrize("pattern", [0xFF, 0x00])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_one_byte_before_or_behind_a_region_is_named(pattern, which):
    for side in ("before", "behind"):
        a = _arena(pattern)
        regions = [a.region(n, name=f"r{k}") for k, n in enumerate((100, 1000, 333))]
        _, start, end = a.regions[which]
        assert regions[which].data_ptr() == a.buf.data_ptr() + start
        a.buf[start - 1 if side == "before" else end] = 0x5A          # what an off-by-one store of the code under test would do
        with pytest.raises(AssertionError) as err:
            a.check()
        assert a.violations() == [(f"r{which}", side, 1, 1)]
        assert f"'r{which}'" in str(err.value) and side in str(err.value) and "bytes 1 .. 1" in str(err.value)


def test_a_run_of_bytes_reports_first_and_last_offset():
    a = _arena()
    a.region(64, name="in")
    ws = a.region(512, name="ws")
    _, start, end = a.regions[1]
    a.buf[end + 3:end + 20] = 0          # bytes 4 .. 20 behind the workspace
    a.buf[start - 9:start - 2] = 0       # bytes 3 .. 9 in front of it
    assert a.violations() == [("ws", "before", 3, 9), ("ws", "behind", 4, 20)]
    assert ws.numel() == 512


def test_a_write_of_the_pattern_itself_is_invisible_which_is_why_rows_run_at_both_patterns():
    for pattern, other in ((0xFF, 0x00), (0x00, 0xFF)):
        a = _arena(pattern)
        a.region(16, name="r")
        _, _, end = a.regions[0]
        a.buf[end] = pattern
        a.check()
        a.buf[end] = other
        with pytest.raises(AssertionError):
            a.check()


@pytest.mark.parametrize("align,shift", [(256, 0), (256, 16), (512, 256), (64, 4), (16, 0), (1, 0)])
def test_region_has_the_requested_address_residue_and_guards(align, shift):
    a = _arena()
    got = [a.region(n, align=align, shift=shift) for n in (7, 1025, 64)]
    for t in got:
        assert t.dtype == torch.uint8 and t.data_ptr() % align == shift
    edges = [0] + [e for _, s, e in a.regions for e in (s, e)] + [a.buf.numel()]
    assert all(hi - lo >= GUARD for lo, hi in zip(edges[0::2], edges[1::2]))          # every gap, the two ends of the arena included
    if align % 4 == 0 and shift % 4 == 0:
        assert got[2].view(torch.float32).shape == (16,)          # .view(dtype) of a region gives typed buffers
    with pytest.raises(ValueError):
        a.region(8, align=16, shift=16)
    with pytest.raises(MemoryError):
        a.region(a.buf.numel())


def test_typed_regions_read_nan_and_minus_one_or_zero():
    a = _arena(regions=6)
    f = a.typed((3, 5), torch.float32)
    i = a.typed((7,), torch.int64)
    h = a.typed((4,), torch.bfloat16)
    assert bool(torch.isnan(f).all()) and bool((i == -1).all()) and bool(torch.isnan(h).all())
    z = a.typed((3,), torch.float32, fill=0x00)
    assert bool((z == 0).all()) and bool((a.typed((2,), torch.int32, fill=0x00) == 0).all())
    src = torch.arange(12.0).view(3, 4)
    assert torch.equal(a.put(src.t()), src.t())
    a.check()


def test_two_fills_differ_only_inside_the_filled_region():
    a, b = _arena(), _arena()
    for arena, fill in ((a, 0xFF), (b, 0x00)):
        arena.region(100, name="in", fill=0xFF)
        arena.region(300, name="ws", fill=fill)
        arena.region(50, name="out", fill=0xFF)
    assert [(n, e - s) for n, s, e in a.regions] == [(n, e - s) for n, s, e in b.regions]
    for (_, sa, ea), (name, sb, eb) in zip(a.regions, b.regions):          # (the two bases need not have the same residue)
        same = torch.equal(a.buf[sa:ea], b.buf[sb:eb])
        assert same == (name != "ws")
    assert bool((a.buf[a.regions[1][1]:a.regions[1][2]] == 0xFF).all()) and bool((b.buf[b.regions[1][1]:b.regions[1][2]] == 0).all())
    for arena in (a, b):          # and outside the regions both arenas are all pattern
        outside = torch.ones_like(arena.buf, dtype=torch.bool)
        for _, s, e in arena.regions:
            outside[s:e] = False
        assert bool((arena.buf[outside] == 0xFF).all())
    a.check()
    b.check()


def test_only_the_two_patterns_exist():
    for bad in (0x7F, 0xAA, 1, -1, 256):
        with pytest.raises(ValueError):
            Arena("cpu", 16, bad)
        with pytest.raises(ValueError):
            _arena().region(4, fill=bad)
    assert guarded.PATTERNS == (0xFF, 0x00)


def test_guarded_empty_patches_the_modules_name_only():
    mod = types.ModuleType("fake_product_module")
    mod.torch = torch
    exec("def alloc(n, **kw):\n    return torch.empty(n, **kw), torch.empty_like(torch.zeros(2, 3), **kw)", mod.__dict__)
    real_empty = torch.empty
    a = _arena(regions=10)
    with guarded.guarded_empty(a, 0x00, [mod]):
        t, u = mod.alloc(10, device="cpu", dtype=torch.float32)
        p, _ = mod.alloc(10, device="cpu", pin_memory=False)
        n, _ = mod.alloc(10)                                           # no device named: not the arena's business
        assert torch.empty is real_empty and mod.torch is not torch
        assert mod.torch.float32 is torch.float32
    assert mod.torch is torch
    lo, hi = a.buf.data_ptr(), a.buf.data_ptr() + a.buf.numel()
    assert lo <= t.data_ptr() < hi and lo <= u.data_ptr() < hi and lo <= p.data_ptr() < hi
    assert not lo <= n.data_ptr() < hi
    assert t.shape == (10,) and u.shape == (2, 3) and bool((t == 0).all()) and bool((u == 0).all())
    t.fill_(1.0)
    a.check()
    log = []
    with guarded.guarded_empty(a, 0xFF, [mod], align=512, shift=256, log=log):
        first = mod.alloc(6, device="cpu", dtype=torch.int64)
    assert [id(t) for t in log] == [id(t) for t in first] and all(t.data_ptr() % 512 == 256 for t in log) and bool((first[0] == -1).all())
    first[0].fill_(7)
    n_regions = len(a.regions)
    with guarded.guarded_empty(a, 0x00, [mod], reuse=list(log)):          # the same blocks again, as they are: no new region, no fill
        again = mod.alloc(6, device="cpu", dtype=torch.int64)
    assert again[0].data_ptr() == first[0].data_ptr() and bool((again[0] == 7).all()) and len(a.regions) == n_regions
    with pytest.raises(AssertionError):        # a reused block must be the allocation that was logged
        with guarded.guarded_empty(a, 0x00, [mod], reuse=log):
            mod.alloc(7, device="cpu", dtype=torch.int64)
    a.check()
    with pytest.raises(RuntimeError):          # the patch is undone on an exception too
        with guarded.guarded_empty(a, 0xFF, [mod]):
            raise RuntimeError("x")
    assert mod.torch is torch
