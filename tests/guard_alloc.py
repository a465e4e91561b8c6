"""Guard-banded, pattern-filled allocator for the bts_amd modules (shared by tests/test_guard_gpu.py, tests/test_poison_host.py and
tests/test_poison_gpu.py; imported the way lowp_ref and norm_ref are).

Every buffer the host side hands to the C ABI -- outputs, saved activations, gradient buffers, partial-sum scratch and each `*_workspace`
buffer, sized EXACTLY by its query -- is carved out of a larger allocation pre-filled with one byte value, PAD bytes of it on either side.
`Guarded` stands in for the `torch` module inside the package: `empty` and `empty_like` return the fill, `zeros`, `zeros_like` and `full`
their defined contents; `check()` asserts that every band still holds the fill.  `install()` swaps it in for every bts_amd module -- the
subject modules of the `ops` package included, which `ops/__init__.py` imports eagerly -- and replaces `ops._core.workspace`, the one
binding every wrapper looks up and `ops.workspace` reads (it normally hands out a grow-only buffer of at least 1 MB, i.e. would hide an over-run of the queried
size and keep an earlier call's contents).

The fill byte decides what an unwritten element reads as:
  0xA5  the out-of-bounds pattern: -2.9e-16 as fp32 / bf16, -0.022 as fp16, -2.5e-127 as fp64 -- close to zero, so a kernel that adds in
        unwritten scratch stays inside every tolerance; good for finding stray WRITES;
  0xFF  NaN in every float type (fp16 0xFFFF, bf16 0xFFFF, fp32 0xFFFFFFFF, fp64 all ones), -1 in every signed integer type;
  0x00  zero.
Running a case with 0x00 and again with 0xFF and comparing the results bit for bit finds READS of bytes nobody wrote: NaN survives a
multiplication by a zero weight, an addition and a maximum, so any dependence shows.  Both 0xA5 and 0xFF are negative in every signed
integer type: the poison changes values, not the addresses a correct kernel forms."""
import importlib
import sys

import torch

PAD = 4096
FILL = 0xA5
POISON = 0xFF

OPS = ('_core', 'streams', 'profile', 'conv', 'norm', 'pointwise', 'loss', 'volume', 'window', 'score', 'augment', 'regions', 'prepro', 'coreg',
       'n4')
MODULES = ('model', 'util', 'tape', 'ops') + tuple('ops.' + m for m in OPS) + (
    'lowp', 'lowp_train', 'parallel', 'data', 'infer', 'train', 'layers._base', 'layers.resnet', 'layers.group_norm', 'layers.downsample',
    'layers.upsample', 'layers.vae', 'layers.encoder', 'layers.decoder')


class Guarded(object):
    """stand-in for the `torch` module inside bts_amd: allocation calls return views into guard-banded buffers.  Buffers on the GPU are
    kept for check(); host buffers too with track_host=True (the CPU tests of the allocator itself)"""

    def __init__(self, fill=FILL, track_host=False):
        if not 0 <= int(fill) <= 255:
            raise ValueError('fill is one byte, got %r' % (fill,))
        self.fill = int(fill)
        self.track_host = track_host
        self.live = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _alloc(self, shape, dtype, device, zero=False, value=None):
        if isinstance(shape, int):
            shape = (shape,)
        shape = tuple(int(s) for s in shape)
        dtype = dtype or torch.float32
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        big = torch.full((nbytes + 2 * PAD,), self.fill, dtype=torch.uint8, device=device if device is not None else 'cpu')
        view = big[PAD:PAD + nbytes].view(dtype).view(shape)
        if zero:
            view.zero_()
        if value is not None:
            view.fill_(value)
        if big.is_cuda or self.track_host:
            self.live.append((big, nbytes))
        return view

    def empty(self, *shape, dtype=None, device=None, **kw):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = shape[0]
        return self._alloc(shape, dtype, device)

    def zeros(self, *shape, dtype=None, device=None, **kw):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = shape[0]
        return self._alloc(shape, dtype, device, zero=True)

    def full(self, shape, value, dtype=None, device=None, **kw):
        return self._alloc(shape, dtype, device, value=value)

    def empty_like(self, t, dtype=None, **kw):
        return self._alloc(tuple(t.shape), dtype or t.dtype, t.device)

    def zeros_like(self, t, dtype=None, **kw):
        return self._alloc(tuple(t.shape), dtype or t.dtype, t.device, zero=True)

    def check(self):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        bad = 0
        for big, nbytes in self.live:
            if not bool((big[:PAD] == self.fill).all()) or not bool((big[PAD + nbytes:] == self.fill).all()):
                bad += 1
        n = len(self.live)
        self.live = []
        assert bad == 0, '%d of %d guarded buffers were written outside their bounds' % (bad, n)
        return n

    # ---- channel-slice views of wider slabs (ld > C) ----
    def slab(self, shape, dtype, device, lead, tail, values=None):
        """a guarded (..., lead + C + tail) buffer, every byte the fill, and its channel view [..., lead:lead + C] (holding `values`,
        cast to dtype, when given; left as the fill otherwise) -> (buffer, view)"""
        shape = tuple(int(s) for s in shape)
        c = shape[-1]
        buf = self._alloc(shape[:-1] + (lead + c + tail,), dtype, device)
        view = buf[..., lead:lead + c]
        if values is not None:
            view.copy_(values.to(dtype).to(buf.device))
        return buf, view

    def refill_outside(self, buf, lead, c):
        """set every byte of a slab outside its channel view [..., lead:lead + c] back to the fill"""
        b8 = buf.view(torch.uint8).reshape(-1, buf.shape[-1], buf.element_size())
        b8[:, :lead].fill_(self.fill)
        b8[:, lead + c:].fill_(self.fill)

    def refill(self, t):
        """set every element of a tensor (a channel view included) to the fill byte: an output that is not accumulated into"""
        if t.is_contiguous():
            t.view(torch.uint8).fill_(self.fill)
        else:
            t.copy_(torch.full((t.element_size(),), self.fill, dtype=torch.uint8, device=t.device).view(t.dtype))
        return t

    def untouched(self, buf, lead, c):
        """do the channels of a slab outside [..., lead:lead + c] still hold the fill, byte for byte?"""
        b8 = buf.view(torch.uint8).reshape(-1, buf.shape[-1], buf.element_size())
        return bool((b8[:, :lead] == self.fill).all()) and bool((b8[:, lead + c:] == self.fill).all())


def install(monkeypatch, fill=FILL):
    """swap a Guarded(fill) in for `torch` in every bts_amd module and an exact-size, filled buffer for ops._core.workspace; undone with
    the monkeypatch.  -> the Guarded"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    g = Guarded(fill)
    for name in MODULES:
        importlib.import_module('bts_amd.' + name)
    mods = [m for n, m in list(sys.modules.items()) if n == 'bts_amd' or n.startswith('bts_amd.')]
    for m in mods:
        if getattr(m, 'torch', None) is torch:
            monkeypatch.setattr(m, 'torch', g)
    for name in OPS:                           # every subject module that allocates does so from the Guarded
        m = sys.modules['bts_amd.ops.' + name]
        assert getattr(m, 'torch', g) is g, 'bts_amd.ops.%s still allocates from torch' % name

    def exact_workspace(nbytes, device):       # exactly what the *_workspace query asked for -- no 1 MB floor, no reuse
        return g._alloc((max(int(nbytes), 1),), torch.uint8, device)
    monkeypatch.setattr(ops._core, 'workspace', exact_workspace)
    # one binding: the callers of ops.workspace outside the package (lowp.py, the tests' own raw calls) get the guarded one too
    assert ops.workspace is ops._core.workspace is exact_workspace and 'workspace' not in vars(ops)
    return g
