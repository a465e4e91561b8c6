"""-m gpu: the class-location kernel (bts_class_locations, ops.class_locations) against tests/sampling_ref.py: exact integer equality of
the counts and of the whole table.

A wave of the kernel takes 1024 consecutive voxels and a workgroup 4096, so the volumes are: one voxel; one partial step; exactly one
workgroup (16^3 = 4096); one row over it (17*16*16); several workgroups with a ragged tail (40*33*29 = 38280 = 9 * 4096 + 1416, the
last wave holding 392 voxels, no multiple of 4).  K in {1, 7, 64, 10000} against classes of K - 1, K, K + 1 and 2K + 1 voxels (the
stride turns 2 at K + 1 and 3 at 2K + 1) and a class that is the whole volume."""
import ctypes

import numpy as np
import pytest
import torch

import sampling_ref as S

pytestmark = pytest.mark.gpu

VOLUMES = [(1, 1, 1), (3, 5, 7), (16, 16, 16), (17, 16, 16), (40, 33, 29)]
KS = (1, 7, 64, 10000)
OUT_CHS = (1, 3, 4)


def dev():
    return torch.device('cuda', 0)


def ops():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    return ops


def patterns(vol, out_ch, k, rs):
    """name -> float32 label volume"""
    v = int(np.prod(vol))
    out = {'background': np.zeros(vol, np.float32)}
    for c in sorted({0, out_ch - 1}):
        out['all_class%d' % c] = np.full(vol, c + 1, np.float32)
    last = np.zeros(v, np.float32)
    last[-1] = out_ch
    out['last_voxel'] = last.reshape(vol)
    for density in (0.5, 0.01):
        lab = rs.randint(1, out_ch + 1, v) * (rs.random_sample(v) < density)
        out['random%g' % density] = lab.astype(np.float32).reshape(vol)
    # labels above out_ch are in no class: the value out_ch + 1, and (for out_ch = 3: BraTS' 4 before it is remapped) the value 4
    out['above'] = rs.randint(0, out_ch + 2, v).astype(np.float32).reshape(vol)
    if out_ch == 3:
        out['label4'] = rs.choice([0, 1, 2, 4], v).astype(np.float32).reshape(vol)
    out['non_integer'] = (rs.randint(0, 2 * out_ch + 1, v) * 0.5).astype(np.float32).reshape(vol)
    # classes of exactly n voxels, around the capacity: class out_ch-1 holds n voxels at random places, the rest is class 0 or background
    for n in (k - 1, k, k + 1, 2 * k + 1):
        if 1 <= n <= v:
            lab = (rs.random_sample(v) < 0.3).astype(np.float32) if out_ch > 1 else np.zeros(v, np.float32)
            lab[rs.permutation(v)[:n]] = out_ch
            if out_ch == 1:
                assert int((lab == 1).sum()) == n
            out['exact%d' % n] = lab.reshape(vol)
    return out


def check(o, y, out_ch, k, what):
    want_counts, want_loc = S.class_locations_ref(y, out_ch, k)
    counts, loc = o.class_locations(torch.from_numpy(y).to(dev()), out_ch, k)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (out_ch,) and counts.is_cuda
    assert loc.dtype == torch.int32 and tuple(loc.shape) == (out_ch, k) and loc.is_cuda
    assert np.array_equal(counts.cpu().numpy(), want_counts), (what, counts.cpu().tolist(), want_counts.tolist())
    got = loc.cpu().numpy()
    assert np.array_equal(got, want_loc), (what, 'first difference at', np.argwhere(got != want_loc)[:1].tolist())


@pytest.mark.parametrize('out_ch', OUT_CHS, ids=lambda v: 'out_ch%d' % v)
@pytest.mark.parametrize('vol', VOLUMES, ids=lambda v: 'x'.join(map(str, v)))
def test_counts_and_table_equal_the_reference(vol, out_ch):
    o = ops()
    rs = np.random.RandomState(sum(vol) * 10 + out_ch)
    for k in KS:
        for name, y in patterns(vol, out_ch, k, rs).items():
            check(o, y, out_ch, k, (vol, out_ch, k, name))


def test_rank_4_labels_and_a_view_that_is_not_16_byte_aligned():
    """the dataset's (S0,S1,S2,1) labels; and a dense volume that starts 4 bytes into a buffer, where the kernel reads voxel by voxel"""
    o = ops()
    rs = np.random.RandomState(3)
    vol = (17, 16, 16)
    y = rs.randint(0, 4, vol).astype(np.float32)
    want_counts, want_loc = S.class_locations_ref(y, 3, 64)
    counts, loc = o.class_locations(torch.from_numpy(y[..., None]).to(dev()), 3, 64)
    assert np.array_equal(counts.cpu().numpy(), want_counts) and np.array_equal(loc.cpu().numpy(), want_loc)
    buf = torch.zeros(y.size + 1, device=dev())
    view = buf[1:].view(vol)
    view.copy_(torch.from_numpy(y))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    counts, loc = o.class_locations(view, 3, 64)
    assert np.array_equal(counts.cpu().numpy(), want_counts) and np.array_equal(loc.cpu().numpy(), want_loc)


def _raw(o, y, counts, loc, out_ch, k):
    """bts_class_locations into the caller's tensors"""
    ws, nb = o._core.scratch('bts_class_locations_workspace', y.device, y.numel(), out_ch)
    o.lib().call('bts_class_locations', o._p(y), o._p(counts), o._p(loc), o._p(ws), nb, y.numel(), out_ch, k, o._stream())


def test_two_calls_are_bit_identical_and_every_entry_is_overwritten():
    o = ops()
    rs = np.random.RandomState(11)
    vol, out_ch = (40, 33, 29), 4
    y = (rs.randint(1, out_ch + 1, vol) * (rs.random_sample(vol) < 0.3)).astype(np.float32)
    y[y == 2] = 0                                            # an absent class: its whole row is the -1 fill
    yd = torch.from_numpy(y).to(dev())
    for k in (7, 10000):
        want_counts, want_loc = S.class_locations_ref(y, out_ch, k)
        runs = []
        for fill in (12345, -7):
            counts = torch.full((out_ch,), fill, dtype=torch.int64, device=dev())
            loc = torch.full((out_ch, k), fill, dtype=torch.int32, device=dev())
            _raw(o, yd, counts, loc, out_ch, k)
            runs.append((counts.cpu().numpy(), loc.cpu().numpy()))
            assert np.array_equal(runs[-1][0], want_counts) and np.array_equal(runs[-1][1], want_loc), (k, fill)
        assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
        a, b = o.class_locations(yd, out_ch, k), o.class_locations(yd, out_ch, k)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_the_library_refuses_before_any_launch():
    """section 1's refusals, by their codes: BTS_ERR_SHAPE -1, BTS_ERR_WORKSPACE -4"""
    o = ops()
    L = o.lib()
    y = torch.zeros(64, device=dev())
    counts = torch.full((3,), 5, dtype=torch.int64, device=dev())
    loc = torch.full((3, 4), 5, dtype=torch.int32, device=dev())
    ws = torch.zeros(1 << 12, dtype=torch.uint8, device=dev())
    P, stream = o._p, o._stream()
    call = L._bts_class_locations
    assert L._bts_class_locations_workspace(64, 3) > 0
    assert L._bts_class_locations_workspace(2 ** 31, 3) == -1 and L._bts_class_locations_workspace(64, 9) == -1
    assert call(P(y), P(counts), P(loc), P(ws), ws.numel(), 2 ** 31, 3, 4, stream) == -1
    assert call(P(y), P(counts), P(loc), P(ws), ws.numel(), 0, 3, 4, stream) == -1
    for out_ch in (0, 9):
        assert call(P(y), P(counts), P(loc), P(ws), ws.numel(), 64, out_ch, 4, stream) == -1
    assert call(P(y), P(counts), P(loc), P(ws), ws.numel(), 64, 3, 0, stream) == -1
    assert call(None, P(counts), P(loc), P(ws), ws.numel(), 64, 3, 4, stream) == -1
    assert call(P(y), None, P(loc), P(ws), ws.numel(), 64, 3, 4, stream) == -1
    assert call(P(y), P(counts), None, P(ws), ws.numel(), 64, 3, 4, stream) == -1
    assert call(P(y), P(counts), P(loc), None, ws.numel(), 64, 3, 4, stream) == -4
    assert call(P(y), P(counts), P(loc), P(ws), 4, 64, 3, 4, stream) == -4
    torch.cuda.synchronize()
    assert bool((counts == 5).all()) and bool((loc == 5).all())          # nothing ran
    assert call(P(y), P(counts), P(loc), P(ws), ws.numel(), 64, 3, 4, stream) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0, 0] and bool((loc == -1).all())


def test_the_wrapper_refuses_with_value_error_before_the_library(monkeypatch):
    o = ops()
    good = torch.zeros((4, 5, 6), device=dev())

    def reached():
        raise AssertionError('the library was reached')
    with monkeypatch.context() as mp:
        mp.setattr(o._core, 'lib', reached)
        for y in (torch.zeros((4, 5, 6)),                                            # on the host
                  torch.zeros((4, 5, 6), dtype=torch.float64, device=dev()),
                  torch.zeros((4, 5, 6), dtype=torch.int32, device=dev()),
                  torch.zeros((4, 5, 12), device=dev())[..., ::2],                   # not dense
                  torch.zeros((4, 5, 6, 2), device=dev()),                           # rank 4 needs a last dimension of 1
                  torch.zeros((5, 6), device=dev()), torch.zeros((1, 4, 5, 6, 1), device=dev()),
                  torch.zeros((0, 5, 6), device=dev()), np.zeros((4, 5, 6), np.float32)):
            with pytest.raises(ValueError):
                o.class_locations(y, 3, 8)
        for out_ch, k in ((0, 8), (9, 8), (3, 0), (3, -1), (3.0, 8), (3, 8.5), (True, 8)):
            with pytest.raises(ValueError):
                o.class_locations(good, out_ch, k)
    counts, loc = o.class_locations(good, 8, 1)                                      # the largest out_ch, the smallest table
    assert counts.tolist() == [0] * 8 and loc.tolist() == [[-1]] * 8
    assert ctypes.sizeof(ctypes.c_long) == 8                                         # counts travel as `long*`
