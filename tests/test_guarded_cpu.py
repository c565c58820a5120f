"""tests/guarded.py on a CPU arena: the tool reports what it claims to report.  A one-byte write at each of the four extremes of the
bands (the byte next to the buffer and the byte farthest from it, on either side) is named with the buffer's label, its side and its
offset from the buffer's edge; an untouched arena passes; takes never overlap; interiors are aligned, exact in size and filled."""
import pytest
import torch

from guarded import ALIGN, BAND, PATTERN, Arena


def _arena():
    arena = Arena("cpu")
    views = {"first": arena.take(1000, 0x00, "first"), "odd": arena.take(777, 0xFF, "odd"), "empty": arena.take(0, 0xFF, "empty"),
             "typed": arena.take_like((5, 3), torch.float64, 0xFF, "typed")}
    return arena, views


def _whole(arena, label):
    return next((whole, off, n) for lab, whole, off, n in arena._takes if lab == label)


def test_untouched_arena_passes_and_interiors_are_exact():
    arena, views = _arena()
    arena.check()
    assert views["first"].dtype == torch.uint8 and views["first"].numel() == 1000 and not views["first"].any()
    assert views["odd"].numel() == 777 and bool((views["odd"] == 0xFF).all())
    assert views["empty"].numel() == 0
    assert views["typed"].shape == (5, 3) and views["typed"].dtype == torch.float64 and views["typed"].is_contiguous()
    assert bool(torch.isnan(views["typed"]).all())   # all-ones bytes: a NaN as fp64
    assert bool(torch.isnan(arena.take_like(7, torch.float32, 0xFF)).all()) and bool((arena.take_like(3, torch.int64, 0xFF) == -1).all())
    for name in ("first", "odd", "typed"):
        assert views[name].data_ptr() % ALIGN == 0, name
    # writing every interior byte leaves the bands alone
    for v in views.values():
        v.view(torch.uint8).fill_(0x3C)
    arena.check()
    src = torch.arange(12, dtype=torch.int32).view(3, 4)
    assert torch.equal(arena.take_copy(src, "copy"), src)
    arena.check()


def test_bands_hold_the_pattern_for_a_full_mebibyte_on_both_sides():
    arena, _ = _arena()
    for label, n in (("first", 1000), ("odd", 777), ("empty", 0), ("typed", 120)):
        whole, off, nbytes = _whole(arena, label)
        assert nbytes == n and off >= BAND and whole.numel() - (off + nbytes) >= BAND
        assert bool((whole[off - BAND:off] == PATTERN).all()) and bool((whole[off + nbytes:off + nbytes + BAND] == PATTERN).all())


@pytest.mark.parametrize("label", ["first", "odd", "empty", "typed"])
@pytest.mark.parametrize("side,rel", [("before", -1), ("before", -BAND), ("after", 0), ("after", BAND - 1)])
def test_one_damaged_byte_is_reported_with_label_side_and_offset(label, side, rel):
    arena, _ = _arena()
    whole, off, nbytes = _whole(arena, label)
    edge = off if side == "before" else off + nbytes
    whole[edge + rel] = 0x00   # one plain torch write
    with pytest.raises(AssertionError) as err:
        arena.check()
    msg = str(err.value)
    assert msg.startswith(f"guard band damaged: {label}, {side}, {rel:+d} .. {rel:+d} (1 bytes differ"), msg
    whole[edge + rel] = PATTERN
    arena.check()


def test_a_damaged_range_reports_its_first_and_last_byte():
    arena, _ = _arena()
    whole, off, nbytes = _whole(arena, "odd")
    whole[off + nbytes:off + nbytes + 1024] = 0x11   # a tile row stored past the end
    with pytest.raises(AssertionError, match=r"odd, after, \+0 \.\. \+1023 \(1024 bytes differ; buffer of 777 bytes\)"):
        arena.check()
    whole[off + nbytes:off + nbytes + 1024] = PATTERN
    whole[off - 64:off - 3] = 0x11
    with pytest.raises(AssertionError, match=r"odd, before, -64 \.\. -4 "):
        arena.check()


def test_take_refuses_a_negative_size_and_a_fill_that_is_no_byte():
    arena = Arena("cpu")
    with pytest.raises(ValueError):
        arena.take(-1, 0)
    with pytest.raises(ValueError):
        arena.take(8, 256)


def test_takes_never_overlap_bands_included():
    arena = Arena("cpu")
    for i, n in enumerate((0, 1, 255, 256, 257, 4096, 100_000, 0, 3)):
        arena.take(n, 0xFF if i % 2 else 0x00, f"t{i}")
    spans = sorted((lo - BAND, hi + BAND, label) for label, lo, hi in arena.spans())   # each interior with its two bands
    for (lo0, hi0, a), (lo1, hi1, b) in zip(spans, spans[1:]):
        assert hi0 <= lo1, (a, b)
    # and each span lies inside its own allocation
    for (label, whole, off, n), (_, lo, hi) in zip(arena._takes, arena.spans()):
        assert whole.data_ptr() <= lo - BAND and hi + BAND <= whole.data_ptr() + whole.numel(), label
