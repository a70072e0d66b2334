"""tests/guarded.py itself, on the CPU: plain torch functions stand in for a kernel and commit, one at a time, the faults
the containment tests exist to see.  No tolerance anywhere: guards are compared bytewise, results with torch.equal."""
import pytest
import torch

from guarded import (ALIGN, GUARD_MIN_BYTES, IN_GUARD, OUT_GUARD, assert_guards_intact, assert_written, guard_bytes, guarded_inout,
                     guarded_input, guarded_output, guarded_workspace)

BF16 = torch.bfloat16
DTYPES = [BF16, torch.float32, torch.uint8, torch.int32]


def _source(shape, dtype):
    g = torch.Generator().manual_seed(3)
    return torch.randint(0, 5, shape, generator=g).to(dtype)


def _elems(buf):
    """The whole allocation in the buffer's own element type, and the index of the view's first element in it."""
    return buf.flat.view(buf.dtype), buf.guard // buf.t.element_size()


@pytest.mark.parametrize("shape,dtype,want", [((7,), BF16, 4096), ((1000, 3), torch.float32, 4096), ((300, 264), BF16, 256 * 528),
                                              ((2, 70, 384), BF16, 256 * 768), ((5, 7), BF16, 4096), ((5, 1001), torch.uint8, 256 * 1001 + 15 & ~15)])
def test_guard_size_is_256_rows_of_the_pitch_at_least_4_kib_and_a_multiple_of_16(shape, dtype, want):
    g = guard_bytes(shape, dtype)
    assert g == want and g % ALIGN == 0 and g >= GUARD_MIN_BYTES
    buf = guarded_output("c", shape, dtype, device="cpu")
    assert buf.guard == g and buf.t.data_ptr() % ALIGN == 0 and tuple(buf.t.shape) == tuple(shape) and buf.t.dtype == dtype
    assert buf.t.data_ptr() - buf.flat.data_ptr() == g                           # the view sits right behind the near guard
    assert buf.flat.numel() - g - buf.nbytes >= g                                # and a whole guard follows its last byte
    assert buf.t.is_contiguous()


def test_patterns_of_the_roles():
    src = _source((5, 8), BF16)
    i, o = guarded_input("x", src, device="cpu"), guarded_output("y", (5, 8), torch.float32, device="cpu")
    w0, w1 = guarded_workspace("ws", 100, 0x00, device="cpu"), guarded_workspace("ws", 100, 0xFF, device="cpu")
    io = guarded_inout("m", src.float(), device="cpu")
    assert torch.equal(i.t, src) and torch.equal(io.t, src.float())
    assert bool((i.flat[:i.guard] == IN_GUARD).all()) and bool((i.flat[i.guard + i.nbytes:] == IN_GUARD).all())
    for b in (o, w0, w1, io):
        assert bool((b.flat[:b.guard] == OUT_GUARD).all()) and bool((b.flat[b.guard + b.nbytes:] == OUT_GUARD).all())
    assert bool(torch.isnan(o.t).all())                                          # nothing written yet
    assert w0.nbytes == 100 and bool((w0.t == 0).all()) and bool((w1.t == 0xFF).all())     # the size asked for, not a byte more
    assert_guards_intact([i, o, w0, w1, io])
    # the input guard is NaN as bf16 and fp32, -1 as int32
    assert bool(torch.isnan(i.flat[:16].view(BF16)).all()) and bool(torch.isnan(i.flat[:16].view(torch.float32)).all())
    assert bool((i.flat[:16].view(torch.int32) == -1).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_function_that_stays_inside_passes(dtype):
    src = _source((6, 24), dtype)
    x, y = guarded_input("x", src, device="cpu"), guarded_output("y", (6, 24), dtype, device="cpu")
    y.t.copy_(x.t + x.t)
    assert_guards_intact([x, y])
    assert_written(y)
    assert torch.equal(y.t, src + src)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["past the end", "before the start"])
def test_one_element_outside_the_view_is_flagged(dtype, where):
    y = guarded_output("y", (6, 24), dtype, device="cpu")
    y.t.zero_()
    whole, first = _elems(y)
    at = first + y.t.numel() if where == "past the end" else first - 1
    whole[at] = 1                                                                # through the flat tensor, as a stray store would
    assert not y.intact()
    assert y.violations()[0] == (y.nbytes if where == "past the end" else -y.t.element_size())
    with pytest.raises(AssertionError, match="guard of 'y' overwritten"):
        assert_guards_intact([y], "stray")
    assert bool((y.t == 0).all())                                                # the payload itself is untouched


def test_a_nan_written_into_an_output_guard_is_flagged():
    y = guarded_output("y", (4, 8), torch.float32, device="cpu")
    whole, first = _elems(y)
    whole[first + 32] = float("nan")                                             # row M of a [4, 8] output
    assert not y.intact()


def test_a_write_to_row_m_plus_k_lands_in_the_guard():
    M, N = 7, 264
    y = guarded_output("y", (M, N), BF16, device="cpu")
    whole, first = _elems(y)
    for k in (0, 100, 255):                                                      # up to one full tile of rows below the last
        y.flat[y.guard + y.nbytes:] = OUT_GUARD
        whole[first + (M + k) * N + N - 1] = 0
        assert y.violations() == [((M + k) * N + N - 1) * 2, ((M + k) * N + N - 1) * 2 + 1]


@pytest.mark.parametrize("dtype", [BF16, torch.float32])
def test_an_unwritten_element_is_flagged(dtype):
    y = guarded_output("y", (6, 24), dtype, device="cpu")
    y.t.zero_()
    assert_written(y)
    y2 = guarded_output("y", (6, 24), dtype, device="cpu")
    y2.t[:5].zero_()
    y2.t[5, :23].zero_()                                                         # the last element is never written
    assert_guards_intact([y2])
    with pytest.raises(AssertionError, match="unwritten or non-finite"):
        assert_written(y2, "short")
    assert not torch.equal(y2.t, y.t)


@pytest.mark.parametrize("dtype", [BF16, torch.float32])
@pytest.mark.parametrize("where", ["past the end", "before the start"])
def test_a_read_of_the_input_guard_gives_a_non_finite_result(dtype, where):
    src = _source((6, 24), dtype)
    x = guarded_input("x", src, device="cpu")
    whole, first = _elems(x)
    n = src.numel()
    inside = whole[first:first + n].float()
    stray = whole[first:first + n + 1] if where == "past the end" else whole[first - 1:first + n]
    assert bool(torch.isfinite(inside.sum())) and torch.equal(inside.view(6, 24), src.float())
    assert not bool(torch.isfinite(stray.float().sum()))
    assert not bool(torch.isfinite((stray.float() * 0.0).sum()))                 # even multiplied by zero
    assert_guards_intact([x])                                                    # reading changes nothing


def test_integer_inputs_read_past_the_view_give_a_different_result():
    src = _source((5, 7), torch.uint8)
    x = guarded_input("map", src, device="cpu")
    whole, first = _elems(x)
    assert int(whole[first:first + 36].sum()) == int(src.sum()) + 255
    ids = guarded_input("ids", _source((9,), torch.int32), device="cpu")
    whole, first = _elems(ids)
    assert int(whole[first + 9]) == -1 and int(whole[first - 1]) == -1
