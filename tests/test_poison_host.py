"""The poisoning allocator of tests/guard_alloc.py, on the CPU: what its fill byte reads as in every type the engine allocates, that the
defined-content calls stay defined, and that the band check notices a stray byte for any fill."""
import pytest
import torch

import guard_alloc
from guard_alloc import PAD, POISON, Guarded

FLOATS = [torch.float16, torch.bfloat16, torch.float32, torch.float64]
INTS = [torch.int8, torch.int16, torch.int32, torch.int64]


@pytest.mark.parametrize('dtype', FLOATS, ids=str)
def test_poisoned_empty_reads_nan_in_every_float_type(dtype):
    g = Guarded(POISON)
    for t in (g.empty((3, 5, 7), dtype=dtype), g.empty(3, 5, 7, dtype=dtype), g.empty_like(torch.zeros((4, 9), dtype=dtype)),
              g.empty_like(torch.zeros((4, 9)), dtype=dtype)):
        assert t.dtype == dtype and t.device.type == 'cpu'
        assert bool(torch.isnan(t).all())
        assert bool((t.view(torch.uint8) == 0xFF).all())
    # NaN survives what a kernel might cancel an unowned lane with
    t = g.empty((8,), dtype=dtype)
    assert bool(torch.isnan(t * 0).all()) and bool(torch.isnan(t + 1).all()) and bool(torch.isnan(t.sum()))


@pytest.mark.parametrize('dtype', INTS, ids=str)
def test_poisoned_empty_reads_minus_one_in_every_signed_integer_type(dtype):
    g = Guarded(POISON)
    t = g.empty((6, 11), dtype=dtype)
    assert t.dtype == dtype and bool((t == -1).all())
    assert bool((g.empty((5,), dtype=torch.uint8) == 255).all())


def test_the_default_fill_is_the_out_of_bounds_pattern():
    """0xA5: negative and tiny in every float type, negative in every signed integer type -- the same sign of garbage as the poison, so
    the poison changes values and not which addresses a correct kernel forms"""
    g = Guarded()
    assert g.fill == guard_alloc.FILL == 0xA5
    assert -3e-16 < float(g.empty((1,), dtype=torch.float32)[0]) < -2.8e-16
    assert -3e-16 < float(g.empty((1,), dtype=torch.bfloat16)[0]) < -2.8e-16
    assert -0.023 < float(g.empty((1,), dtype=torch.float16)[0]) < -0.021
    assert -2.6e-127 < float(g.empty((1,), dtype=torch.float64)[0]) < -2.4e-127
    for dtype in INTS:
        assert int(g.empty((1,), dtype=dtype)[0]) < 0
    with pytest.raises(ValueError):
        Guarded(256)


@pytest.mark.parametrize('fill', [0x00, 0xA5, 0xFF])
def test_defined_allocations_keep_their_contents(fill):
    g = Guarded(fill)
    for dtype in FLOATS + INTS:
        assert bool((g.zeros((4, 6), dtype=dtype) == 0).all())
        assert bool((g.zeros(4, 6, dtype=dtype) == 0).all())
        assert bool((g.zeros_like(torch.ones((7,), dtype=dtype)) == 0).all())
        assert bool((g.full((5, 3), 3, dtype=dtype) == 3).all())
    assert g.zeros((2, 2)).dtype == torch.float32 and g.empty((2, 2)).dtype == torch.float32
    assert bool((g.full((9,), 0.5) == 0.5).all())
    # everything else is torch's own
    assert g.float16 is torch.float16 and g.randn is torch.randn


@pytest.mark.parametrize('fill', [0x00, 0xA5, 0xFF])
def test_band_check_passes_untouched_and_fails_after_a_stray_byte(fill):
    g = Guarded(fill, track_host=True)
    t = g.empty((4, 8), dtype=torch.float32)
    z = g.zeros((3,), dtype=torch.float16)
    t.fill_(1.5)                   # writing the whole tensor is inside its bounds
    z.fill_(2.0)
    assert g.check() == 2
    assert g.live == []
    for where in (PAD - 1, PAD + 4 * 8 * 4):          # the last byte in front, the first byte behind
        t = g.empty((4, 8), dtype=torch.float32)
        base = g.live[-1][0]
        base[where] = fill ^ 0x01
        with pytest.raises(AssertionError, match='written outside'):
            g.check()
    assert Guarded(fill).empty((2,)) is not None and Guarded(fill).live == []       # host buffers are not kept unless asked for


@pytest.mark.parametrize('fill', [0x00, 0xFF])
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float32], ids=str)
def test_slab_views_and_refilling_outside_a_channel_view(fill, dtype):
    g = Guarded(fill, track_host=True)
    vals = torch.arange(2 * 3 * 4 * 5 * 6, dtype=torch.float32).reshape(2, 3, 4, 5, 6)
    buf, v = g.slab((2, 3, 4, 5, 6), dtype, None, lead=8, tail=4, values=vals)
    assert tuple(buf.shape) == (2, 3, 4, 5, 18) and tuple(v.shape) == (2, 3, 4, 5, 6) and v.stride(3) == 18 and v.stride(4) == 1
    assert torch.equal(v, vals.to(dtype)) and g.untouched(buf, 8, 6)
    assert bool((buf[..., :8].contiguous().view(torch.uint8) == fill).all()) and bool((buf[..., 14:].contiguous().view(torch.uint8) == fill).all())
    buf[1, 2, 3, 4, 14] = 1.0          # a neighbour channel written
    assert not g.untouched(buf, 8, 6)
    buf[..., :8] = 2.0
    g.refill_outside(buf, 8, 6)
    assert g.untouched(buf, 8, 6) and torch.equal(v, vals.to(dtype))
    g.refill(v)                        # an output view that is not accumulated into
    assert bool((buf.view(torch.uint8) == fill).all())
    _, e = g.slab((1, 2, 2, 2, 4), dtype, None, lead=4, tail=4)
    assert bool((e.contiguous().view(torch.uint8) == fill).all())
    if fill == 0xFF:
        assert bool(torch.isnan(buf).all())
    c = g.refill(g.zeros((5, 5), dtype=dtype))
    assert bool((c.view(torch.uint8) == fill).all())
    assert g.check() == 3
