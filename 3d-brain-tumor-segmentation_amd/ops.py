"""Thin, checked Python wrappers over the C ABI (include/bts_hip.h): torch tensors in, raw pointers out.

torch is used for device memory and the current HIP stream only.  Every function enqueues on
torch.cuda.current_stream() and raises RuntimeError on a non-zero status -- there is no CPU path.
Activations are [N,D,H,W,C] fp32 tensors whose last-dim stride is 1 and whose voxel stride (`ld`) may exceed C
(channel slices of a slab).
"""
import ctypes
import weakref

import numpy as np
import torch

from ._lib import ERRORS, lib

K1, K3S1, K3S2, K3S2T = 0, 1, 2, 3
ROLE_FWD, ROLE_BWD = 0, 1
FLAG_SIGMOID, FLAG_ACCUM = 1, 2
GN_SLAB, GN_CHANNEL = 0, 1

_workspaces = {}

# ---- optional live kernel timing (bench.py roofline): the library records HIP events on the launch stream around its
# igemm_kernel / wgrad_kernel launches (bts_profile_*), i.e. the same per-launch durations rocprofv3 reports ----
_CFG = {0: '2,1,4,1', 1: '2,2,4,1', 2: '1,2,2,2', 3: '1,1,2,2', 4: '1,1,4,1'}


# profile symbol -> kernel name (fp32 conv engine and its weight gradient: SYM_* of csrc/conv_plan.h; the 16-bit kernels name theirs at the launch)
_SYMBOLS = {20: 'upm_kernel', 21: 'k1s_kernel', 22: 'dsc_kernel', 23: 'wino_kernel', 24: 'wgw_kernel', 25: 'c2_kernel', 26: 'k1w_kernel',
            27: 'w3_kernel', 30: 'lp_conv_s1_kernel', 31: 'lp_conv_gather_kernel', 32: 'lp_wgrad_kernel', 33: 'lp_s1d_kernel',
            34: 'lp_k1_kernel', 35: 'lp_up_kernel', 36: 'lp_wgs_kernel', 37: 'lp_wgd_kernel', 38: 'lp_s1z_kernel', 39: 'lp_s2t_kernel',
            40: 'lp_c2_kernel'}
_SYMBOLS.update({cfg + 8 * k1: 'igemm_kernel<%s,%d>' % (_CFG[cfg], 4 if k1 else 1) for cfg in _CFG for k1 in (0, 1)})      # the tiled kernel
_SYMBOLS.update({100 + v: 'wgrad_kernel<%d,%d>' % (v >> 2, v & 3) for v in range(12)})      # 100 + (MODE << 2 | FIXG)


_VARIANTS = {33: {1: '<0,5>', 2: '<0,4>', 3: '<1,5>', 4: '<1,4>'},          # lp_s1d_kernel<MODE, TXL>
             32: {1: '<3x3x3>', 2: '<1x1x1>'}}                                 # lp_wgrad_kernel by kernel size


def kernel_symbol(sym, detail=False):
    """name of a profiled launch; bits 16+ of `sym` carry a kernel-specific variant, shown only with detail=True (tests count launches
    by the plain name, bench.py's kernel_breakdown tells the variants apart)"""
    var, sym = sym >> 16, sym & 0xffff
    if var and detail and sym in _VARIANTS:
        return kernel_symbol(sym) + _VARIANTS[sym].get(var, '<%d>' % var)
    return _SYMBOLS[sym]


def profile_enable(on):
    lib().call('bts_profile_enable', 1 if on else 0)


def profile_records(detail=False):
    """-> [(symbol, algorithmic_flops, ms)] ; synchronise the device first.  detail: kernel variants in the symbol names"""
    L = lib()
    out = []
    sym, fl, ms = ctypes.c_int(), ctypes.c_double(), ctypes.c_float()
    for i in range(L._bts_profile_count()):
        L.call('bts_profile_get', i, ctypes.byref(sym), ctypes.byref(fl), ctypes.byref(ms))
        out.append((kernel_symbol(sym.value, detail), fl.value, ms.value))
    return out


def conv_bwd_data_pair(dy, wp_bwd, dy2, wp2_bwd, dx, accumulate):
    """dx (+)= bwd_data(3x3x3)(dy) + bwd_data(1x1x1)(dy2): both gradient paths into a ResNet block's input in one pass"""
    n, d, h, w, cin = dx.shape
    cout = dy.shape[4]
    nb = lib().query('bts_conv3d_bwd_data_pair_workspace', n, d, h, w, cin, cout)
    ws = workspace(nb, dy.device) if nb > 0 else None
    lib().call('bts_conv3d_bwd_data_pair', _p(dy), _p(wp_bwd), _p(dy2), _p(wp2_bwd), _p(dx), _p(ws), nb, n, d, h, w, cin,
               ld_of(dx), cout, ld_of(dy), ld_of(dy2), FLAG_ACCUM if accumulate else 0, _stream())
    return dx


def conv_flops(kind, n, d, h, w, cin, cout):
    """algorithmic FLOPs of one conv call, SURVEY 8(d) convention (MAC = 2; (d,h,w) = forward INPUT dims)"""
    v = n * d * h * w
    if kind == K1:
        return 2.0 * cin * cout * v
    if kind == K3S2:
        return 2.0 * 27 * cin * cout * (v // 8)
    return 2.0 * 27 * cin * cout * v   # K3S1; K3S2T counts 27*Cin*Cout*V_in MACs


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_side = {}
_side_enabled = True


_fence = {}


def step_fence(kind='train', depth=2):
    """Bound how far the host runs ahead of the GPU: call at the START of a step -- waits (host side) until the step issued `depth`
    calls earlier has finished, then notes this one.  A step enqueues in 2-12 ms what the GPU runs in 7-80 ms; left unbounded, the
    host gets many steps ahead, every one of them holding its activations (blocks freed on a side stream cannot be handed out again
    before that stream's work has run), the caching allocator answers with new hipMalloc segments inside the timed region -- the
    reserved pool was seen to grow from 100 to 140 GB for 42 GB of live tensors, and steps to take 120-400 ms instead of 79.  With
    at most `depth` steps in flight the allocation pattern is the same every step.  BTS_STEP_FENCE=0 disables it (A/B)."""
    import os
    if not torch.cuda.is_available() or os.environ.get('BTS_STEP_FENCE') == '0':
        return
    key = (torch.cuda.current_device(), kind)
    q = _fence.setdefault(key, [])
    while len(q) >= depth:
        q.pop(0).synchronize()
    ev = torch.cuda.Event()
    q.append(ev)
    return ev


def step_fence_done(ev):
    """call at the END of the step with what step_fence returned: the event is recorded behind everything the step enqueued on the
    current stream (side streams are joined before a step returns)"""
    if ev is not None:
        ev.record(torch.cuda.current_stream())


def enable_side_streams(on):
    """switch the extra streams off / on at run time (bench.py measures per-kernel launch durations with one stream: a kernel
    that shares the chip with another stream's kernels has no launch duration of its own)"""
    global _side_enabled
    join_side_stream()
    _side_enabled = bool(on)


def side_stream(which='wgrad'):
    """Extra HIP streams of a training step (one process still drives one GPU):
      'wgrad'  the weight gradients (a third of the step, needed only by the optimiser) run there while the data-gradient
               chain -- with its many short normalisation / gate kernels that leave most CUs idle -- keeps the main stream;
      'gate'   a ResNet block's shortcut / squeeze-excitation branch (HBM-bound 1x1x1 conv, pooling, tiny MLP and their
               gradients: resnet.py:118-130) next to its conv branch (matrix-pipe-bound), joined where the two meet.
    BTS_WGRAD_STREAM=0 / BTS_GATE_STREAM=0 put the respective work back on the main stream (A/B aids)."""
    import os
    if not _side_enabled or not torch.cuda.is_available() or os.environ.get('BTS_%s_STREAM' % which.upper()) == '0':
        return None
    key = (torch.cuda.current_device(), which)
    s = _side.get(key)
    if s is None:
        s = torch.cuda.Stream(device=key[0])
        _side[key] = s
    return s


def join_side_stream():
    """the current stream waits for everything enqueued on the side streams so far (before the regulariser / the gradient
    exchange / the optimiser touch the parameter gradients)"""
    if not torch.cuda.is_available():
        return
    dev = torch.cuda.current_device()
    for (d, _), s in _side.items():
        if d == dev:
            torch.cuda.current_stream().wait_stream(s)


def wait_side_stream_event(which='wgrad'):
    """the current stream waits for what side stream `which` holds at this moment (an event recorded there now); later launches on
    the side stream are not waited for.  A gloo group drains the producing stream on the host instead (parallel._sum_over_ranks)."""
    if not torch.cuda.is_available():
        return
    s = _side.get((torch.cuda.current_device(), which))
    if s is None:
        return
    ev = torch.cuda.Event()
    ev.record(s)
    torch.cuda.current_stream().wait_event(ev)


def workspace(nbytes, device):
    """one grow-only scratch buffer per device AND stream; all users of a buffer are ordered on that stream"""
    key = (device.type, device.index, torch.cuda.current_stream().cuda_stream if device.type == 'cuda' else 0)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


def _check(t, name='tensor'):
    if not t.is_cuda:
        raise RuntimeError('%s must live on the GPU (no CPU fallback exists for the product path)' % name)
    if t.dtype != torch.float32:
        raise RuntimeError('%s must be float32' % name)


def ld_of(t):
    """voxel stride of an NDHWC view (validates that the view is a channel slice of a dense NDHWC buffer)"""
    _check(t)
    if t.dim() != 5 or t.stride(4) != 1 and t.shape[4] != 1:
        raise RuntimeError('expected an [N,D,H,W,C] tensor with unit channel stride, got strides %s' % (t.stride(),))
    n, d, h, w, c = t.shape
    ld = t.stride(3)
    if w == 1:
        ld = t.stride(2) if h > 1 else (t.stride(1) if d > 1 else (t.stride(0) if n > 1 else c))
    exp = (d * h * w * ld, h * w * ld, w * ld, ld)
    for i in range(4):
        if t.shape[i] > 1 and t.stride(i) != exp[i]:
            raise RuntimeError('tensor is not a channel slice of a dense NDHWC buffer: strides %s' % (t.stride(),))
    if ld < c:
        raise RuntimeError('bad voxel stride')
    return ld


def conv_kind_taps(kind):
    return 1 if kind == K1 else 27


def conv_pack(kind, role, w, cin_ref, cout, cin_slab=None, dup_start=0, dup_shift=0):
    """reference-layout kernel -> packed image for the implicit-GEMM kernel"""
    _check(w, 'kernel')
    cin_slab = cin_ref if cin_slab is None else cin_slab
    n = lib().query('bts_conv_packed_floats', kind, role, cin_slab, cout)
    wp = torch.empty(n, dtype=torch.float32, device=w.device)
    wc = w.contiguous()
    lib().call('bts_conv_pack', kind, role, _p(wc), _p(wp), cin_ref, cout, cin_slab, dup_start, dup_shift,
               _stream())
    if wc is not w:      # packed from a temporary copy: the library must not re-pack a form on demand from that address later
        lib()._bts_conv_pack_forget(_p(wp))
    else:                # the library keys its record of the image by address: drop it with the tensor
        fin = weakref.finalize(wp, _forget_image, wp.data_ptr())
        fin.atexit = False
    return wp


def _forget_image(ptr):
    try:
        lib()._bts_conv_pack_forget(ctypes.c_void_p(ptr))
    except Exception:      # (interpreter shutdown)
        pass


class PackTable(object):
    """Device-resident descriptor table for bts_conv_pack_batch: entries = [(kind, role, w, wp, cin_ref, cout, cin_slab,
    dup_start, dup_shift)] with torch tensors w (reference layout) / wp (packed image).  Rebuilt only when a pointer or
    the entry list changes."""

    def __init__(self):
        self.key = None
        self.dev = None
        self.host = None
        self.n = 0
        self.blocks = 0

    def run(self, entries):
        if not entries:
            return
        # (+ the library's form-usage generation: images are re-packed in the forms their layers read; a table built before a new form
        # was first read is rebuilt here, once)
        key = (lib().query('bts_conv_pack_generation'),) + tuple((e[0], e[1], e[2].data_ptr(), e[3].data_ptr()) + tuple(e[4:]) for e in entries)
        if key != self.key:
            L = lib()
            nb = L._bts_conv_pack_desc_bytes()
            host = (ctypes.c_char * (nb * len(entries)))()
            first = 0
            for i, (kind, role, w, wp, cin_ref, cout, cin_slab, dup_start, dup_shift) in enumerate(entries):
                _check(w, 'kernel')
                _check(wp, 'packed image')
                if not w.is_contiguous():
                    raise ValueError('conv_pack_batch: kernels must be contiguous')
                r = L._bts_conv_pack_desc(ctypes.cast(host, ctypes.c_void_p), i, first, kind, role, _p(w), _p(wp), cin_ref,
                                          cout, cin_slab, dup_start, dup_shift)
                if r <= 0:
                    raise RuntimeError('bts_conv_pack_desc failed: %s' % ERRORS.get(r, r))
                first += r
            dev = entries[0][3].device
            self.dev = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(dev)
            self.host = host      # (kept: the library reads each entry's forms from the host copy of the table it is asked to run)
            self.key, self.n, self.blocks = key, len(entries), first
        lib().call('bts_conv_pack_batch', _p(self.dev), ctypes.cast(self.host, ctypes.c_void_p), self.n, self.blocks, _stream())


def conv_packed_empty(kind, role, cin_slab, cout, device):
    return torch.empty(lib().query('bts_conv_packed_floats', kind, role, cin_slab, cout), dtype=torch.float32, device=device)


def conv_out_shape(kind, x_shape, cout):
    n, d, h, w, _ = x_shape
    if kind == K3S2:
        return (n, d // 2, h // 2, w // 2, cout)
    if kind == K3S2T:
        return (n, 2 * d, 2 * h, 2 * w, cout)
    return (n, d, h, w, cout)


def conv_fwd(kind, x, wp, bias, cout, out=None, sigmoid=False):
    n, d, h, w, cin = x.shape
    if out is None:
        out = torch.empty(conv_out_shape(kind, x.shape, cout), dtype=torch.float32, device=x.device)
    nb = lib().query('bts_conv3d_fwd_workspace', kind, n, d, h, w, cin, cout)
    ws = workspace(nb, x.device) if nb > 0 else None
    lib().call('bts_conv3d_fwd', kind, _p(x), _p(wp), _p(bias), _p(out), _p(ws), nb, n, d, h, w, cin, ld_of(x), cout,
               ld_of(out), FLAG_SIGMOID if sigmoid else 0, _stream())
    return out


def conv_fwd_fused2(x, wp3, bias3, wp1, bias1, cout):
    """(c1, res) = (conv3x3x3(x)+bias3, conv1x1x1(x)+bias1) from one pass over x, or None when the selected tiling cannot
    hold the second accumulator set (the caller then launches the two convolutions separately)"""
    n, d, h, w, cin = x.shape
    if not lib()._bts_conv3d_fwd_can_fuse(n, d, h, w, cin, cout):
        return None
    c1 = torch.empty((n, d, h, w, cout), dtype=torch.float32, device=x.device)
    res = torch.empty_like(c1)
    lib().call('bts_conv3d_fwd_fused2', _p(x), _p(wp3), _p(bias3), _p(c1), _p(wp1), _p(bias1), _p(res), n, d, h, w, cin,
               ld_of(x), cout, cout, cout, _stream())
    return c1, res


def conv_fwd_gn(kind, x, wp, bias, cout, groups, eps):
    """(y, mean, rstd): y = conv(x) + bias (dense) and the slab-mode GroupNorm statistics of y, in one pass where the
    tiled kernel can emit them from its epilogue (the library falls back to bts_gn_stats otherwise)"""
    n, d, h, w, cin = x.shape
    y = torch.empty(conv_out_shape(kind, x.shape, cout), dtype=torch.float32, device=x.device)
    mean = torch.empty(n * groups, dtype=torch.float32, device=x.device)
    rstd = torch.empty(n * groups, dtype=torch.float32, device=x.device)
    nb = lib().query('bts_conv3d_fwd_gn_workspace', kind, n, d, h, w, cin, cout, groups)
    ws = workspace(nb, x.device)
    lib().call('bts_conv3d_fwd_gn', kind, _p(x), _p(wp), _p(bias), _p(y), _p(ws), nb, n, d, h, w, cin, ld_of(x), cout, groups,
               float(eps), _p(mean), _p(rstd), _stream())
    return y, mean, rstd


def conv_fwd_fused2_gn(x, wp3, bias3, wp1, bias1, cout, groups, eps):
    """conv_fwd_fused2 with the GroupNorm statistics of its 3x3x3 output: (c1, res, mean, rstd) or None"""
    n, d, h, w, cin = x.shape
    if not lib()._bts_conv3d_fwd_can_fuse(n, d, h, w, cin, cout):
        return None
    c1 = torch.empty((n, d, h, w, cout), dtype=torch.float32, device=x.device)
    res = torch.empty_like(c1)
    mean = torch.empty(n * groups, dtype=torch.float32, device=x.device)
    rstd = torch.empty(n * groups, dtype=torch.float32, device=x.device)
    nb = lib().query('bts_conv3d_fwd_gn_workspace', K3S1, n, d, h, w, cin, cout, groups)
    ws = workspace(nb, x.device)
    lib().call('bts_conv3d_fwd_fused2_gn', _p(x), _p(wp3), _p(bias3), _p(c1), _p(wp1), _p(bias1), _p(res), _p(ws), nb, n, d, h, w,
               cin, ld_of(x), cout, cout, groups, float(eps), _p(mean), _p(rstd), _stream())
    return c1, res, mean, rstd


def conv_bwd_data(kind, dy, wp_bwd, dx, accumulate):
    """dx: [N,D,H,W,Cin] view of the forward input's gradient"""
    n, d, h, w, cin = dx.shape
    cout = dy.shape[4]
    nb = lib().query('bts_conv3d_bwd_data_workspace', kind, n, d, h, w, cin, cout)
    ws = workspace(nb, dy.device) if nb > 0 else None
    lib().call('bts_conv3d_bwd_data', kind, _p(dy), _p(wp_bwd), _p(dx), _p(ws), nb, n, d, h, w, cin, ld_of(dx), cout,
               ld_of(dy), FLAG_ACCUM if accumulate else 0, _stream())
    return dx


def conv_bwd_weight(kind, x, dy, dw, db, dup_start=0, dup_shift=0, accumulate=False):
    n, d, h, w, cin = x.shape
    cout = dy.shape[4]
    nb = lib().query('bts_conv3d_bwd_weight_workspace', kind, n, d, h, w, cin, cout)
    ws = workspace(nb, x.device)
    lib().call('bts_conv3d_bwd_weight', kind, _p(x), _p(dy), _p(dw), _p(db), _p(ws), nb, n, d, h, w, cin, ld_of(x),
               cout, ld_of(dy), dup_start, dup_shift, 1 if accumulate else 0, _stream())


def _conv_bwd_weight_query(name, kind, x, dy):
    n, d, h, w, cin = x.shape
    aligned = (1 if x.data_ptr() % 16 == 0 else 0) | (2 if dy.data_ptr() % 16 == 0 else 0)
    return lib().probe(name, kind, n, d, h, w, cin, ld_of(x), dy.shape[4], ld_of(dy), aligned)


def conv_bwd_weight_form(kind, x, dy):
    """the form conv_bwd_weight takes for these operands (host-only query): 3 Winograd over all axes | 0 every other kernel"""
    return _conv_bwd_weight_query('bts_conv3d_bwd_weight_form', kind, x, dy)


def conv_bwd_weight_kernel(kind, x, dy):
    """the profile symbol of the kernel conv_bwd_weight runs for these operands (host-only query): 100 | 104 | 109 | 110 the direct kernel's
    variants, 24 wgw_kernel, 26 k1w_kernel"""
    return _conv_bwd_weight_query('bts_conv3d_bwd_weight_kernel', kind, x, dy)


def gn_stats(x, groups, mode, eps=1e-5):
    """x dense [N,D,H,W,C] -> (mean, rstd) each (N*G,)"""
    if not x.is_contiguous():
        raise RuntimeError('GroupNormalization statistics need a dense tensor')
    n, c = x.shape[0], x.shape[4]
    v = x.shape[1] * x.shape[2] * x.shape[3]
    nb = lib().query('bts_gn_workspace', n, v, c, groups, mode)
    ws = workspace(nb, x.device)
    mean = torch.empty(n * groups, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    lib().call('bts_gn_stats', _p(x), _p(mean), _p(rstd), _p(ws), nb, n, v, c, groups, mode, eps, _stream())
    return mean, rstd


def gn_apply(x, gamma, beta, mean, rstd, groups, mode, relu, out=None):
    n, c = x.shape[0], x.shape[4]
    v = x.shape[1] * x.shape[2] * x.shape[3]
    if out is None:
        out = torch.empty_like(x)
    lib().call('bts_gn_apply', _p(x), _p(out), _p(gamma), _p(beta), _p(mean), _p(rstd), n, v, c, ld_of(out), groups, mode,
               1 if relu else 0, _stream())
    return out


def gn_bwd(x, dy, gamma, beta, mean, rstd, dgamma, dbeta, groups, mode, relu, accumulate_params=False):
    n, c = x.shape[0], x.shape[4]
    v = x.shape[1] * x.shape[2] * x.shape[3]
    nb = lib().query('bts_gn_bwd_workspace', n, v, c, groups, mode)
    ws = workspace(nb, x.device)
    dx = torch.empty_like(x)
    lib().call('bts_gn_bwd', _p(x), _p(dy), _p(dx), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(dgamma), _p(dbeta), _p(ws),
               nb, n, v, c, ld_of(dy), groups, mode, 1 if relu else 0, 1 if accumulate_params else 0, _stream())
    return dx


def colsum(x, scale=1.0, sum_over_n=False, out=None, accumulate=False):
    """x [N,...,C] (channel slice allowed) -> [N,C] (or [C]) column sums * scale"""
    n, c = x.shape[0], x.shape[-1]
    rows = x.numel() // (n * c)
    ld = ld_of(x) if x.dim() == 5 else x.stride(-2)
    nb = lib().query('bts_colsum_workspace', n, rows, c)
    ws = workspace(nb, x.device)
    if out is None:
        out = torch.empty((c,) if sum_over_n else (n, c), dtype=torch.float32, device=x.device)
    lib().call('bts_colsum', _p(x), _p(out), _p(ws), nb, n, rows, c, ld, float(scale), 1 if sum_over_n else 0,
               1 if accumulate else 0, _stream())
    return out


def se_mlp_fwd(gap, w1, w2):
    n, f = gap.shape
    r = w1.shape[1]
    h = torch.empty((n, r), dtype=torch.float32, device=gap.device)
    ch = torch.empty((n, f), dtype=torch.float32, device=gap.device)
    lib().call('bts_se_mlp_fwd', _p(gap), _p(w1), _p(w2), _p(h), _p(ch), n, f, r, _stream())
    return h, ch


def block_epilogue_fwd(res, c2, out, wsp, ch, gamma, beta, mean, rstd, groups, mode):
    n, f = res.shape[0], res.shape[4]
    v = res.shape[1] * res.shape[2] * res.shape[3]
    sp = torch.empty(n * v, dtype=torch.float32, device=res.device)
    lib().call('bts_block_epilogue_fwd', _p(res), _p(c2), _p(out), _p(sp), _p(wsp), _p(ch), _p(gamma), _p(beta), _p(mean),
               _p(rstd), n, v, f, ld_of(out), groups, mode, _stream())
    return sp


def se_bwd(dout, res, sp, gap, h, ch, w1, w2, wsp, dw1, dw2, dwsp, accumulate_params=False):
    n, f = res.shape[0], res.shape[4]
    v = res.shape[1] * res.shape[2] * res.shape[3]
    r = w1.shape[1]
    nb = lib().query('bts_se_bwd_workspace', n, v, f, r)
    ws = workspace(nb, res.device)
    dres = torch.empty_like(res)
    ds = torch.empty(n * v, dtype=torch.float32, device=res.device)
    dgap = torch.empty((n, f), dtype=torch.float32, device=res.device)
    lib().call('bts_se_bwd', _p(dout), _p(res), _p(sp), _p(gap), _p(h), _p(ch), _p(w1), _p(w2), _p(wsp), _p(dres), _p(ds),
               _p(dgap), _p(dw1), _p(dw2), _p(dwsp), _p(ws), nb, n, v, f, r, ld_of(dout), 1 if accumulate_params else 0,
               _stream())
    return dres


def block_bwd_takes(res, r, groups, dout, c2):
    """does the fused gate + GroupNorm-2 backward take this block?  Asked BEFORE the grad slots are claimed, so it checks everything
    block_bwd and bts_block_bwd check (tiling, row stride, contiguity, 16-byte alignment of the three streamed tensors): once this
    says yes, block_bwd does not decline."""
    n, f = res.shape[0], res.shape[4]
    v = res.shape[1] * res.shape[2] * res.shape[3]
    return (lib().probe('bts_block_bwd_workspace', n, v, f, r, groups) >= 0 and ld_of(dout) % 4 == 0 and res.is_contiguous()
            and c2.is_contiguous() and all(t.data_ptr() % 16 == 0 for t in (dout, res, c2)))


def block_bwd(dout, res, c2, sp, gap, h, ch, w1, w2, wsp, gamma, beta, mean, rstd, groups, dw1, dw2, dwsp, dgamma, dbeta,
              accumulate_gate_params=False, accumulate_norm_params=False):
    """gate backward + GroupNorm-2 backward (slab mode, ReLU) of a ResnetBlock in one pair of passes -> (dres, dc2), or None where
    the fused kernels do not take the shape (the caller runs se_bwd and gn_bwd)"""
    n, f = res.shape[0], res.shape[4]
    v = res.shape[1] * res.shape[2] * res.shape[3]
    r = w1.shape[1]
    nb = lib().probe('bts_block_bwd_workspace', n, v, f, r, groups)      # (-1: outside the fused kernels' tiling, not an error)
    if not block_bwd_takes(res, r, groups, dout, c2):
        return None
    ws = workspace(nb, res.device)
    dres = torch.empty_like(res)
    dc2 = torch.empty_like(c2)
    ds = torch.empty(n * v, dtype=torch.float32, device=res.device)
    dgap = torch.empty((n, f), dtype=torch.float32, device=res.device)
    lib().call('bts_block_bwd', _p(dout), ld_of(dout), _p(res), _p(c2), _p(sp), _p(gap), _p(h), _p(ch), _p(w1), _p(w2), _p(wsp), _p(gamma), _p(beta),
               _p(mean), _p(rstd), _p(dres), _p(dc2), _p(ds), _p(dgap), _p(dw1), _p(dw2), _p(dwsp), _p(dgamma), _p(dbeta), _p(ws), nb, n, v, f, r,
               groups, 1 if accumulate_gate_params else 0, 1 if accumulate_norm_params else 0, _stream())
    return dres, dc2


def dropout_mask(shape, rate, seed, device):
    m = torch.empty(shape, dtype=torch.uint8, device=device)
    lib().call('bts_dropout_mask', _p(m), m.numel(), float(rate), int(seed) & (2 ** 64 - 1), _stream())
    return m


def dropout_apply(x, mask, rate):
    y = torch.empty_like(x)
    lib().call('bts_dropout_apply', _p(x), _p(mask), _p(y), x.numel(), float(rate), _stream())
    return y


def normal(shape, seed, device):
    out = torch.empty(shape, dtype=torch.float32, device=device)
    lib().call('bts_normal', _p(out), out.numel(), int(seed) & (2 ** 64 - 1), _stream())
    return out


def vae_sample_fwd(proj, eps):
    n, l2 = proj.shape
    z = torch.empty((n, l2 // 2), dtype=torch.float32, device=proj.device)
    lib().call('bts_vae_sample_fwd', _p(proj), _p(eps), _p(z), n, l2 // 2, _stream())
    return z


def vae_sample_bwd(proj, eps, dz, dproj):
    n, l2 = proj.shape
    lib().call('bts_vae_sample_bwd', _p(proj), _p(eps), _p(dz), _p(dproj), n, l2 // 2, _stream())


def fill(t, v):
    lib().call('bts_fill', _p(t), t.numel(), float(v), _stream())
    return t


def axpy(y, x, a=1.0):
    lib().call('bts_axpy', _p(y), _p(x), y.numel(), float(a), _stream())


def add_strided(dst, src, accumulate):
    """dst[..., :C] (+)= src[..., :C] for NDHWC channel-slice views"""
    c = src.shape[-1]
    rows = src.numel() // c
    ldd = ld_of(dst) if dst.dim() == 5 else dst.stride(-2)
    lds = ld_of(src) if src.dim() == 5 else src.stride(-2)
    lib().call('bts_add_strided', _p(dst), _p(src), rows, c, ldd, lds, 1 if accumulate else 0, _stream())


def scalar_lincomb(a, b, ca=1.0, cb=1.0):
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    lib().call('bts_scalar_lincomb', _p(out), _p(a), _p(b), float(ca), float(cb), _stream())
    return out


def relu_bwd(y, dy):
    dx = torch.empty_like(y)
    lib().call('bts_relu_bwd', _p(y), _p(dy), _p(dx), y.numel(), _stream())
    return dx


def sigmoid_bwd(y, dy):
    c = y.shape[-1]
    rows = y.numel() // c
    dx = torch.empty(y.shape, dtype=torch.float32, device=y.device)
    lib().call('bts_sigmoid_bwd', _p(y), _p(dy), _p(dx), rows, c, ld_of(y), ld_of(dy), _stream())
    return dx


def dense_fwd(x, w, b, relu):
    n, fin = x.shape
    fout = w.shape[1]
    nb = lib().query('bts_dense_workspace', n, fin, fout)
    ws = workspace(nb, x.device)
    y = torch.empty((n, fout), dtype=torch.float32, device=x.device)
    lib().call('bts_dense_fwd', _p(x), _p(w), _p(b), _p(y), _p(ws), nb, n, fin, fout, 1 if relu else 0, _stream())
    return y


def dense_bwd(x, w, g, dx, dw, db, accumulate_dx=False, accumulate_params=False):
    n, fin = x.shape
    fout = w.shape[1]
    lib().call('bts_dense_bwd', _p(x), _p(w), _p(g), _p(dx), _p(dw), _p(db), n, fin, fout, 1 if accumulate_dx else 0,
               1 if accumulate_params else 0, _stream())


def loss_sums(y_pred, y, x, y_vae, proj):
    """-> sums (3C+4,) float64 device tensor (see include/bts_hip.h)"""
    n, c = y_pred.shape[0], y_pred.shape[4]
    v = y_pred.shape[1] * y_pred.shape[2] * y_pred.shape[3]
    sums = torch.empty(3 * c + 4, dtype=torch.float64, device=y_pred.device)
    nb = lib().query('bts_loss_workspace')
    ws = workspace(nb, y_pred.device)
    has_vae = x is not None
    cx = x.shape[4] if has_vae else 0
    lz = proj.shape[1] // 2 if proj is not None else 0
    lib().call('bts_loss_sums', _p(y_pred), _p(y), _p(x), _p(y_vae), _p(proj), _p(sums), _p(ws), nb, n, v, c, ld_of(y_pred),
               ld_of(y), cx, ld_of(x) if has_vae else 0, ld_of(y_vae) if has_vae else 0, lz, _stream())
    return sums


def loss_value(sums, c, has_vae=True):
    loss = torch.empty(1, dtype=torch.float32, device=sums.device)
    parts = torch.empty(3, dtype=torch.float32, device=sums.device)
    lib().call('bts_loss_value', _p(sums), _p(loss), _p(parts), c, 1 if has_vae else 0, _stream())
    return loss, parts


def loss_bwd(y_pred, y, x, y_vae, proj, sums, gscale, dypred, dyvae, dproj, through_sigmoid=False):
    n, c = y_pred.shape[0], y_pred.shape[4]
    v = y_pred.shape[1] * y_pred.shape[2] * y_pred.shape[3]
    has_vae = x is not None
    cx = x.shape[4] if has_vae else 0
    lz = proj.shape[1] // 2 if proj is not None else 0
    lib().call('bts_loss_bwd', _p(y_pred), _p(y), _p(x), _p(y_vae), _p(proj), _p(sums), _p(gscale), _p(dypred), _p(dyvae),
               _p(dproj), n, v, c, ld_of(y_pred), ld_of(y), cx, ld_of(x) if has_vae else 0, ld_of(y_vae) if has_vae else 0,
               lz, 1 if through_sigmoid else 0, _stream())


def _seg_loss_dims(y_pred, x, y_vae, proj):
    n, c = y_pred.shape[0], y_pred.shape[4]
    v = y_pred.shape[1] * y_pred.shape[2] * y_pred.shape[3]
    has_vae = x is not None
    cx = x.shape[4] if has_vae else 0
    lz = proj.shape[1] // 2 if proj is not None else 0
    return n, v, c, cx, ld_of(x) if has_vae else 0, ld_of(y_vae) if has_vae else 0, lz


def seg_loss_sums(y_pred, y, x, y_vae, proj, gamma=0.0, w_pos=1.0, w_neg=1.0):
    """the compound loss's raw sums in one pass -> (4C+5,) float64 device tensor: loss_sums' 3C+4, the cross-entropy / focal sums per
    channel, this shard's N*V (see include/bts_hip.h)"""
    n, v, c, cx, ldx, ldv, lz = _seg_loss_dims(y_pred, x, y_vae, proj)
    sums = torch.empty(4 * c + 5, dtype=torch.float64, device=y_pred.device)
    nb = lib().query('bts_seg_loss_workspace')
    ws = workspace(nb, y_pred.device)
    lib().call('bts_seg_loss_sums', _p(y_pred), _p(y), _p(x), _p(y_vae), _p(proj), _p(sums), _p(ws), nb, n, v, c, ld_of(y_pred),
               ld_of(y), cx, ldx, ldv, lz, gamma, w_pos, w_neg, _stream())
    return sums


def seg_loss_value(sums, c, has_vae=True, w_dice=1.0, w_ce=1.0):
    """-> loss (1,), parts (4,) = dice, l2, kl, cross-entropy"""
    loss = torch.empty(1, dtype=torch.float32, device=sums.device)
    parts = torch.empty(4, dtype=torch.float32, device=sums.device)
    lib().call('bts_seg_loss_value', _p(sums), _p(loss), _p(parts), c, 1 if has_vae else 0, w_dice, w_ce, _stream())
    return loss, parts


def seg_loss_bwd(y_pred, y, x, y_vae, proj, sums, gscale, dypred, dyvae, dproj, through_sigmoid=False, w_dice=1.0, w_ce=1.0,
                 gamma=0.0, w_pos=1.0, w_neg=1.0):
    n, v, c, cx, ldx, ldv, lz = _seg_loss_dims(y_pred, x, y_vae, proj)
    lib().call('bts_seg_loss_bwd', _p(y_pred), _p(y), _p(x), _p(y_vae), _p(proj), _p(sums), _p(gscale), _p(dypred), _p(dyvae),
               _p(dproj), n, v, c, ld_of(y_pred), ld_of(y), cx, ldx, ldv, lz, 1 if through_sigmoid else 0, w_dice, w_ce, gamma,
               w_pos, w_neg, _stream())


def dice_metric_sums(y_true, y_pred, channels_last_axes=True, want_labels=True):
    n, d, h, w, c = y_pred.shape
    cells = w if channels_last_axes else 1
    table = torch.empty(cells * c * 3, dtype=torch.float64, device=y_pred.device)
    labels = torch.empty((n, d, h, w), dtype=torch.uint8, device=y_pred.device) if want_labels else None
    lib().call('bts_dice_metric_sums', _p(y_true), _p(y_pred), _p(labels), _p(table), n, d * h * w, w, c, ld_of(y_true),
               ld_of(y_pred), 1 if channels_last_axes else 0, _stream())
    return table, labels


def dice_metric_value(table, w, c, channels_last_axes=True):
    out = torch.empty(2, dtype=torch.float32, device=table.device)
    lib().call('bts_dice_metric_value', _p(table), _p(out), w, c, 1 if channels_last_axes else 0, _stream())
    return out


def _ranges(ranges):
    nr = len(ranges)
    off = (ctypes.c_long * max(nr, 1))(*[r[0] for r in ranges])
    ln = (ctypes.c_long * max(nr, 1))(*[r[1] for r in ranges])
    cf = (ctypes.c_float * max(nr, 1))(*[r[2] for r in ranges])
    return off, ln, cf, nr


def l2_reg_fwd(params_flat, ranges):
    """ranges: [(offset, length, coefficient)] (<= 128) into the flat parameter buffer"""
    off, ln, cf, nr = _ranges(ranges)
    out = torch.empty(1, dtype=torch.float32, device=params_flat.device)
    nb = lib().query('bts_l2_workspace')
    ws = workspace(nb, params_flat.device)
    lib().call('bts_l2_reg_fwd', _p(params_flat), ctypes.cast(off, ctypes.c_void_p), ctypes.cast(ln, ctypes.c_void_p),
               ctypes.cast(cf, ctypes.c_void_p), nr, _p(out), _p(ws), nb, _stream())
    return out


def l2_reg_bwd(params_flat, grads_flat, ranges, gscale=None):
    off, ln, cf, nr = _ranges(ranges)
    lib().call('bts_l2_reg_bwd', _p(params_flat), _p(grads_flat), ctypes.cast(off, ctypes.c_void_p),
               ctypes.cast(ln, ctypes.c_void_p), ctypes.cast(cf, ctypes.c_void_p), nr, _p(gscale), _stream())


def adam_tf_step(p, g, m, v, lr_t, beta1, beta2, eps, gmul=1.0, skip=None):
    """skip: device int32[1]; the whole update is dropped on the device when it is non-zero (grad_nonfinite below)"""
    if skip is not None:
        lib().call('bts_adam_tf_step_guarded', _p(p), _p(g), _p(m), _p(v), p.numel(), float(lr_t), float(beta1), float(beta2),
                   float(eps), float(gmul), _p(skip), _stream())
        return
    lib().call('bts_adam_tf_step', _p(p), _p(g), _p(m), _p(v), p.numel(), float(lr_t), float(beta1), float(beta2),
               float(eps), float(gmul), _stream())


def grad_nonfinite(g, flag):
    """flag[0] (device int32) = 1 iff any element of the flat fp32 gradient is Inf / NaN"""
    lib().call('bts_grad_nonfinite', _p(g), g.numel(), _p(flag), _stream())


# ---- full-volume inference helpers ----
def flip_affine(src, flip_mask=0, mean=None, std=None, scale=1.0, out=None, accumulate=False):
    """out (+)= scale * t(flip(src)); flip_mask bits 4|2|1 = reverse D|H|W; t = (v - mean[c]) / std[c] when given"""
    _check(src, 'src')
    if not src.is_contiguous():
        raise ValueError('flip_affine: src must be a dense NDHWC tensor')
    n, d, h, w, c = src.shape
    if out is None:
        if accumulate:
            raise ValueError('flip_affine: accumulate needs an output tensor')
        out = torch.empty_like(src)
    lib().call('bts_flip_affine', _p(src), _p(out), _p(mean), _p(std), n, d, h, w, c, int(flip_mask), float(scale),
               1 if accumulate else 0, _stream())
    return out


def tta_finish(prob, bmask, threshold=0.5, want_probabilities=True, want_labels=True):
    """-> (prob * bmask, uint8 label map): argmax + 1, >= 3 -> 4, 0 where masked out / below threshold"""
    n, d, h, w, c = prob.shape
    y = torch.empty_like(prob) if want_probabilities else None
    labels = torch.empty((n, d, h, w), dtype=torch.uint8, device=prob.device) if want_labels else None
    lib().call('bts_tta_finish', _p(prob.contiguous()), _p(bmask.contiguous()), _p(y), _p(labels), n * d * h * w, c,
               float(threshold), _stream())
    return y, labels


# ---- resampling of a scan to the 1 mm^3 grid and back (test.py:15-72) ----
def _check_volume(t, name):
    _check(t, name)
    if t.dim() != 4 or not t.is_contiguous():
        raise ValueError('%s must be a dense (D,H,W,C) tensor, got shape %s strides %s' % (name, tuple(t.shape), t.stride()))


def spline_prefilter3d(x, out=None):
    """cubic B-spline coefficients of a dense (D,H,W,C) volume along D, H and W (the spline_filter half of
    scipy.ndimage.zoom(order=3, mode='reflect')); C <= 8, spatial extents >= 4"""
    _check_volume(x, 'spline_prefilter3d: x')
    d, h, w, c = x.shape
    if out is None:
        out = torch.empty_like(x)
    elif tuple(out.shape) != tuple(x.shape) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError('spline_prefilter3d: out must be a dense float32 tensor of the shape of x')
    lib().call('bts_spline_prefilter3d', _p(x), _p(out), d, h, w, c, _stream())
    return out


def zoom3d(coef, out_shape, order=3, pad_to=None, want_mask=False, mean=None, std=None):
    """coef (D,H,W,C) evaluated on zoom()'s grid of spatial extent out_shape: order 3 takes spline_prefilter3d coefficients, orders 0
    and 1 the samples themselves.  pad_to >= out_shape: extent of the result, zero outside out_shape (pad_to_spatial_res in the same
    pass).  want_mask: also (max_c value > 0) as float32 (..., 1).  mean/std (C,): the result is normalised after the mask test.
    -> volume, or (volume, mask) with want_mask"""
    _check_volume(coef, 'zoom3d: coef')
    if order not in (0, 1, 3):
        raise ValueError('zoom3d: order must be 0, 1 or 3, got %r' % (order,))
    do, ho, wo = (int(v) for v in out_shape)
    dp, hp, wp = (do, ho, wo) if pad_to is None else (int(v) for v in pad_to)
    if min(do, ho, wo) < 1 or dp < do or hp < ho or wp < wo:
        raise ValueError('zoom3d: out_shape %s must be positive and within pad_to %s' % ((do, ho, wo), (dp, hp, wp)))
    if (mean is None) != (std is None):
        raise ValueError('zoom3d: mean and std go together')
    d, h, w, c = coef.shape
    out = torch.empty((dp, hp, wp, c), dtype=torch.float32, device=coef.device)
    mask = torch.empty((dp, hp, wp, 1), dtype=torch.float32, device=coef.device) if want_mask else None
    lib().call('bts_zoom3d', _p(coef), _p(out), _p(mask), _p(mean), _p(std), d, h, w, do, ho, wo, c, dp, hp, wp, int(order),
               _stream())
    return (out, mask) if want_mask else out


# ---- conforming a scan to an oriented grid by its affine (infer.Conformer) ----
def reorient3d(x, perm, flip, out=None):
    """x (D,H,W,C) -> the exact copy np.flip(np.transpose(x, perm + (3,)), [a for a in range(3) if flip[a]]): output axis a runs along
    axis perm[a] of x, reversed where flip[a]; C <= 8"""
    _check_volume(x, 'reorient3d: x')
    try:
        perm = tuple(int(v) for v in perm)
        flip = tuple(bool(v) for v in flip)
    except TypeError:
        perm, flip = (), ()
    if sorted(perm) != [0, 1, 2] or len(flip) != 3:
        raise ValueError('reorient3d: perm must be a permutation of (0, 1, 2) and flip three booleans, got %r and %r' % (perm, flip))
    d, h, w, c = x.shape
    shape = tuple(x.shape[p] for p in perm) + (c,)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != shape or not out.is_contiguous() or out.dtype != torch.float32 or out.data_ptr() == x.data_ptr():
        raise ValueError('reorient3d: out must be a dense float32 tensor of shape %s that is not x' % (shape,))
    lib().call('bts_reorient3d', _p(x), _p(out), d, h, w, c, perm[0], perm[1], perm[2], 4 * flip[0] + 2 * flip[1] + 1 * flip[2],
               _stream())
    return out


def affine_resample3d(coef, matrix, out_shape, order=3, pad_to=None, out=None, channel=0, want_mask=False):
    """coef (D,H,W,C) evaluated where the 3x4 (or 4x4) float64 `matrix` sends the voxels of a grid of spatial extent out_shape: source
    voxel coordinate = matrix @ (o0, o1, o2, 1).  order 3 takes spline_prefilter3d coefficients, orders 0 and 1 the samples themselves;
    taps and the reflect rule are zoom3d's (order 1 is weighted and summed in float64 and rounded once).  Voxels whose coordinate lies outside [-0.5, n - 0.5] on any axis are 0, as are
    those of pad_to >= out_shape outside out_shape.  out: a dense float32 (pad_to, K) volume, K >= channel + C, whose channels
    channel .. channel+C-1 are written and whose others are left as they are (modalities on different grids: one call each).
    want_mask: also (max_c value > 0) as float32 (..., 1); only a call that writes every channel of the result can give it.
    -> volume, or (volume, mask) with want_mask"""
    _check_volume(coef, 'affine_resample3d: coef')
    if order not in (0, 1, 3):
        raise ValueError('affine_resample3d: order must be 0, 1 or 3, got %r' % (order,))
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape == (4, 4):
        m = m[:3]
    if m.shape != (3, 4) or not np.all(np.isfinite(m)):
        raise ValueError('affine_resample3d: matrix must be a finite 3x4 or 4x4 array, got %r' % (matrix,))
    do, ho, wo = (int(v) for v in out_shape)
    dp, hp, wp = (do, ho, wo) if pad_to is None else (int(v) for v in pad_to)
    if min(do, ho, wo) < 1 or dp < do or hp < ho or wp < wo:
        raise ValueError('affine_resample3d: out_shape %s must be positive and within pad_to %s' % ((do, ho, wo), (dp, hp, wp)))
    d, h, w, c = coef.shape
    c0 = int(channel)
    if out is None:
        if c0 != 0:
            raise ValueError('affine_resample3d: channel %d needs an output volume to write into' % c0)
        out = torch.empty((dp, hp, wp, c), dtype=torch.float32, device=coef.device)
    else:
        _check_volume(out, 'affine_resample3d: out')
        if tuple(out.shape[:3]) != (dp, hp, wp) or c0 < 0 or c0 + c > out.shape[3]:
            raise ValueError('affine_resample3d: out has shape %s; channels %d .. %d of a %s volume are asked for'
                             % (tuple(out.shape), c0, c0 + c - 1, (dp, hp, wp)))
    ld = int(out.shape[3])
    if want_mask and (c0 != 0 or ld != c):
        raise ValueError('affine_resample3d: the mask is the maximum over all channels; this call writes %d of %d' % (c, ld))
    mask = torch.empty((dp, hp, wp, 1), dtype=torch.float32, device=coef.device) if want_mask else None
    m12 = (ctypes.c_double * 12)(*[float(v) for v in m.reshape(-1)])
    lib().call('bts_affine_resample3d', _p(coef), d, h, w, c, _p(out), ld, c0, _p(mask), do, ho, wo, dp, hp, wp, m12, int(order),
               _stream())
    return (out, mask) if want_mask else out


# ---- the two-stage hand-over and the per-case score (test.py:181-270) ----
def skull_strip(x, p, m, orig, pad_to, out=None):
    """x (Da,Ha,Wa,C), p and m (Da,Ha,Wa,1) dense float32; orig = the unpadded extent (D,H,W); pad_to = (Db,Hb,Wb) >= orig
    -> (xo (Db,Hb,Wb,C) = x * (1 - p) inside orig, 0 outside; mo (Db,Hb,Wb,1) = m inside, 0 outside)   [test.py:244-254]
    out: (xo, mo) dense float32 tensors of those shapes to write into"""
    _check_volume(x, 'skull_strip: x')
    da, ha, wa, c = x.shape
    for t, name in ((p, 'p'), (m, 'm')):
        _check_volume(t, 'skull_strip: ' + name)
        if tuple(t.shape) != (da, ha, wa, 1):
            raise ValueError('skull_strip: %s must have shape %s, got %s' % (name, (da, ha, wa, 1), tuple(t.shape)))
    d, h, w = (int(v) for v in orig)
    db, hb, wb = (int(v) for v in pad_to)
    if out is None:
        xo = torch.empty((db, hb, wb, c), dtype=torch.float32, device=x.device)
        mo = torch.empty((db, hb, wb, 1), dtype=torch.float32, device=x.device)
    else:
        xo, mo = out
        _check_volume(xo, 'skull_strip: xo')
        _check_volume(mo, 'skull_strip: mo')
        if tuple(xo.shape) != (db, hb, wb, c) or tuple(mo.shape) != (db, hb, wb, 1):
            raise ValueError('skull_strip: out must have shapes %s and %s, got %s and %s'
                             % ((db, hb, wb, c), (db, hb, wb, 1), tuple(xo.shape), tuple(mo.shape)))
    lib().call('bts_skull_strip', _p(x), _p(p), _p(m), _p(xo), _p(mo), da, ha, wa, d, h, w, db, hb, wb, c, _stream())
    return xo, mo


def label_confusion(truth, pred, n_classes=4, counts=None):
    """truth, pred: dense uint8 label maps of equal size on the GPU -> counts (K,K) int64 on the GPU with
    counts[min(t,K-1), min(p,K-1)] += 1 per voxel.  counts: a zeroed (or partly filled) buffer to add into; a new one otherwise"""
    k = int(n_classes)
    for t, name in ((truth, 'truth'), (pred, 'pred')):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError('label_confusion: %s must be a dense uint8 tensor on the GPU' % name)
    if truth.numel() != pred.numel():
        raise ValueError('label_confusion: %d truth and %d predicted voxels' % (truth.numel(), pred.numel()))
    if counts is None:
        counts = torch.zeros((max(k, 0), max(k, 0)), dtype=torch.int64, device=truth.device)
    elif not isinstance(counts, torch.Tensor) or not counts.is_cuda or counts.dtype != torch.int64 or counts.numel() != k * k \
            or not counts.is_contiguous():
        raise ValueError('label_confusion: counts must be %d dense int64 values on the GPU' % (k * k))
    lib().call('bts_label_confusion', _p(truth), _p(pred), truth.numel(), k, _p(counts), _stream())
    return counts


# ---- sliding-window inference (csrc/window.hip) ----
def window_batch_max():
    """jobs one launch of bts_window_gather / bts_window_accumulate carries"""
    return int(lib().query('bts_window_batch_max'))


def _window_jobs(who, starts, flips):
    """the host side of a job list -> (B, 3B ints, B ints) as ctypes arrays"""
    n = len(flips)
    if n == 0 or len(starts) != n or any(len(s) != 3 for s in starts):
        raise ValueError('%s: %d flips need as many (z0,y0,x0) starts, got %d' % (who, n, len(starts)))
    st = (ctypes.c_int * (3 * n))(*[int(v) for tri in starts for v in tri])
    fl = (ctypes.c_int * n)(*[int(f) for f in flips])
    return n, st, fl


def window_gather(x, roi, starts, flips, means, stds, out=None):
    """x (D,H,W,C) dense float32; roi (R0,R1,R2); per job b: starts[b] = (z0,y0,x0) inside the volume, flips[b] (bits 4|2|1 = D|H|W),
    means[b] / stds[b] = C host floats -> out (B,R0,R1,R2,C): the window normalised and flipped, (0 - mean) / std beyond the volume's end.
    out: a dense float32 tensor of that shape to write into"""
    _check_volume(x, 'window_gather: x')
    d, h, w, c = x.shape
    r0, r1, r2 = (int(v) for v in roi)
    n, st, fl = _window_jobs('window_gather', starts, flips)
    if len(means) != n or len(stds) != n or any(len(m) != c for m in means) or any(len(s) != c for s in stds):
        raise ValueError('window_gather: every one of the %d jobs needs %d means and %d stds' % (n, c, c))
    shape = (n, r0, r1, r2, c)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        _check(out, 'window_gather: out')
        if tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError('window_gather: out must be a dense %s tensor, got shape %s strides %s' % (shape, tuple(out.shape), out.stride()))
    mean = (ctypes.c_float * (n * c))(*[float(v) for row in means for v in row])
    std = (ctypes.c_float * (n * c))(*[float(v) for row in stds for v in row])
    as_p = lambda a: ctypes.cast(a, ctypes.c_void_p)      # noqa: E731
    lib().call('bts_window_gather', _p(x), _p(out), d, h, w, c, r0, r1, r2, n, as_p(st), as_p(fl), as_p(mean), as_p(std), _stream())
    return out


def window_accumulate(pred, acc, tables, starts, flips, rows, scale=1.0):
    """pred (B,R0,R1,R2,K): the forward's output for the jobs, still flipped; acc (D,H,W,K), updated IN PLACE; tables = (nz (n0,R0),
    ny (n1,R1), nx (n2,R2)) dense float32 on the GPU (infer.window_plan's, as float32); per job b: starts[b], flips[b] as in
    window_gather and rows[b] = (iz,iy,ix), its window's rows in the tables.
    acc[z0+d, y0+h, x0+w, k] += scale * nz[iz][d] * ny[iy][h] * nx[ix][w] * pred[b, fd(d), fh(h), fw(w), k] inside the volume -> acc"""
    _check_volume(acc, 'window_accumulate: acc')
    _check(pred, 'window_accumulate: pred')
    d, h, w, k = acc.shape
    if pred.dim() != 5 or not pred.is_contiguous() or pred.shape[4] != k:
        raise ValueError('window_accumulate: pred must be a dense (B,R0,R1,R2,%d) tensor, got shape %s strides %s'
                         % (k, tuple(pred.shape), pred.stride()))
    n, st, fl = _window_jobs('window_accumulate', starts, flips)
    r0, r1, r2 = (int(v) for v in pred.shape[1:4])
    if pred.shape[0] != n or len(rows) != n or any(len(r) != 3 for r in rows):
        raise ValueError('window_accumulate: pred holds %d jobs, the lists %d starts and %d rows' % (pred.shape[0], n, len(rows)))
    if len(tables) != 3:
        raise ValueError('window_accumulate: tables must be (nz, ny, nx)')
    for t, r, name in zip(tables, (r0, r1, r2), ('nz', 'ny', 'nx')):
        _check(t, 'window_accumulate: ' + name)
        if t.dim() != 2 or t.shape[1] != r or t.shape[0] < 1 or not t.is_contiguous():
            raise ValueError('window_accumulate: %s must be a dense (windows, %d) tensor, got shape %s' % (name, r, tuple(t.shape)))
    rw = (ctypes.c_int * (3 * n))(*[int(v) for tri in rows for v in tri])
    as_p = lambda a: ctypes.cast(a, ctypes.c_void_p)      # noqa: E731
    lib().call('bts_window_accumulate', _p(pred), _p(acc), _p(tables[0]), _p(tables[1]), _p(tables[2]), tables[0].shape[0],
               tables[1].shape[0], tables[2].shape[0], d, h, w, k, r0, r1, r2, n, as_p(st), as_p(fl), as_p(rw), float(scale), _stream())
    return acc


def window_occupancy(mask, roi, starts, out=None):
    """mask (D,H,W,1) dense float32; starts = (z starts, y starts, x starts) of a window plan -> int32 (n0,n1,n2) on the GPU: the voxels
    with mask > 0 inside each window, clipped to the volume.  out: a dense int32 tensor of that shape to write into"""
    _check_volume(mask, 'window_occupancy: mask')
    d, h, w, c = mask.shape
    if c != 1:
        raise ValueError('window_occupancy: mask must have shape (D,H,W,1), got %s' % (tuple(mask.shape),))
    if len(starts) != 3 or any(len(s) == 0 for s in starts):
        raise ValueError('window_occupancy: starts must be three non-empty lists, got %r' % (starts,))
    r0, r1, r2 = (int(v) for v in roi)
    n0, n1, n2 = (len(s) for s in starts)
    if out is None:
        out = torch.empty((n0, n1, n2), dtype=torch.int32, device=mask.device)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.int32 or tuple(out.shape) != (n0, n1, n2) \
            or not out.is_contiguous():
        raise ValueError('window_occupancy: out must be a dense int32 %s tensor on the GPU' % ((n0, n1, n2),))
    st = torch.tensor([int(v) for s in starts for v in s], dtype=torch.int32).to(mask.device)
    lib().call('bts_window_occupancy', _p(mask), _p(st), _p(out), n0, n1, n2, d, h, w, r0, r1, r2, _stream())
    return out


# ---- the distance side of the per-case score (test.py:266-270; csrc/surface.hip) ----
def _dense(t, dtype, name, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError('%s must be a dense %s tensor on the GPU' % (name, what))
    return t


def region_surface(lab, n_classes=4, class_mask=0b1110, out=None, count=None):
    """lab: dense uint8 label map (D,H,W) on the GPU; the region is the set of classes min(label, K-1) whose bit is set in class_mask
    -> (surf uint8 (D,H,W): 1 on the region's surface voxels (a face neighbour outside the region or the volume), 0 elsewhere;
    count: one int64 on the GPU, += their number).  out: a dense uint8 tensor of lab's size to write into; count: a zeroed (or partly
    filled) int64 element to add into; new ones otherwise"""
    _dense(lab, torch.uint8, 'region_surface: lab', 'uint8')
    if lab.dim() != 3:
        raise ValueError('region_surface: lab must have shape (D,H,W), got %s' % (tuple(lab.shape),))
    if out is None:
        out = torch.empty_like(lab)
    elif _dense(out, torch.uint8, 'region_surface: out', 'uint8').numel() != lab.numel():
        raise ValueError('region_surface: out holds %d voxels, lab %d' % (out.numel(), lab.numel()))
    if count is None:
        count = torch.zeros(1, dtype=torch.int64, device=lab.device)
    elif _dense(count, torch.int64, 'region_surface: count', 'int64').numel() != 1:
        raise ValueError('region_surface: count must be one int64 value on the GPU')
    d, h, w = lab.shape
    lib().call('bts_region_surface', _p(lab), _p(out), _p(count), d, h, w, int(n_classes), int(class_mask), _stream())
    return out, count


def edt3d_sq(feat, spacing=(1.0, 1.0, 1.0), out=None):
    """feat: dense uint8 (D,H,W) on the GPU, spacing (sd,sh,sw) in mm -> float64 (D,H,W): the squared distance in mm^2 to the nearest
    voxel with feat != 0 (+inf when there is none), exact.  out: a dense float64 tensor of feat's size to write into"""
    _dense(feat, torch.uint8, 'edt3d_sq: feat', 'uint8')
    if feat.dim() != 3:
        raise ValueError('edt3d_sq: feat must have shape (D,H,W), got %s' % (tuple(feat.shape),))
    sd, sh, sw = (float(s) for s in spacing)
    if out is None:
        out = torch.empty(tuple(feat.shape), dtype=torch.float64, device=feat.device)
    elif _dense(out, torch.float64, 'edt3d_sq: out', 'float64').numel() != feat.numel():
        raise ValueError('edt3d_sq: out holds %d voxels, feat %d' % (out.numel(), feat.numel()))
    d, h, w = feat.shape
    lib().call('bts_edt3d_sq', _p(feat), _p(out), d, h, w, sd, sh, sw, _stream())
    return out


def masked_select(v, mask, ranks, out=None):
    """v: dense NON-NEGATIVE float64, mask: dense uint8 of the same size, both on the GPU; ranks: up to 8 host integers
    -> float64 (len(ranks),) on the GPU: the ranks[i]-th smallest (0-based) of v[mask != 0], the bits np.sort gives; nan where
    ranks[i] is not below the number of selected values.  out: a dense float64 tensor of len(ranks) values to write into"""
    _dense(v, torch.float64, 'masked_select: v', 'float64')
    _dense(mask, torch.uint8, 'masked_select: mask', 'uint8')
    if v.numel() != mask.numel():
        raise ValueError('masked_select: %d values and %d mask bytes' % (v.numel(), mask.numel()))
    ranks = [int(r) for r in ranks]
    nr = len(ranks)
    if out is None:
        out = torch.empty(nr, dtype=torch.float64, device=v.device)
    elif _dense(out, torch.float64, 'masked_select: out', 'float64').numel() != nr:
        raise ValueError('masked_select: out must hold %d float64 values' % nr)
    if nr == 0:
        return out
    nb = lib().query('bts_masked_select_workspace', nr)
    ws = workspace(nb, v.device)
    rk = (ctypes.c_long * nr)(*ranks)
    lib().call('bts_masked_select', _p(v), _p(mask), v.numel(), ctypes.cast(rk, ctypes.c_void_p), nr, _p(out), _p(ws), _stream())
    if v.numel() == 0:
        out.fill_(float('nan'))                                  # nothing is selected, and the call launches nothing for no values
    return out


# ---- connected components of a region of a label map (csrc/components.hip) ----
def components3d(lab, class_mask, K=4, connectivity=26, out=None):
    """lab: dense uint8 label map (D,H,W) on the GPU; the region is the set of classes min(label, K-1) whose bit is set in class_mask;
    connectivity 6 | 18 | 26 (scipy's generate_binary_structure(3, 1 | 2 | 3))
    -> comp int32 (D,H,W): 0 outside the region, 1 + the smallest linear index of the voxel's component inside (the same bytes in
    every run; comp[v] == v + 1 marks a root).  out: a dense int32 tensor of lab's size to write into"""
    _dense(lab, torch.uint8, 'components3d: lab', 'uint8')
    if lab.dim() != 3:
        raise ValueError('components3d: lab must have shape (D,H,W), got %s' % (tuple(lab.shape),))
    if out is None:
        out = torch.empty(tuple(lab.shape), dtype=torch.int32, device=lab.device)
    elif _dense(out, torch.int32, 'components3d: out', 'int32').numel() != lab.numel():
        raise ValueError('components3d: out holds %d voxels, lab %d' % (out.numel(), lab.numel()))
    d, h, w = lab.shape
    lib().call('bts_components3d', _p(lab), _p(out), d, h, w, int(K), int(class_mask), int(connectivity), _stream())
    return out


def component_sizes(comp, out=None, count=None):
    """comp: the int32 map of components3d -> (size int32 (comp.numel(),): size[r] = voxels of the component whose root is r, 0
    elsewhere; count: one int64 on the GPU, += the number of components).  out: a dense int32 tensor of that size to write into (the
    call zeroes it); count: a zeroed (or partly filled) int64 element to add into; new ones otherwise"""
    _dense(comp, torch.int32, 'component_sizes: comp', 'int32')
    n = comp.numel()
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=comp.device)
    elif _dense(out, torch.int32, 'component_sizes: out', 'int32').numel() != n:
        raise ValueError('component_sizes: out holds %d values, comp %d' % (out.numel(), n))
    if count is None:
        count = torch.zeros(1, dtype=torch.int64, device=comp.device)
    elif _dense(count, torch.int64, 'component_sizes: count', 'int64').numel() != 1:
        raise ValueError('component_sizes: count must be one int64 value on the GPU')
    lib().call('bts_component_sizes', _p(comp), n, _p(out), _p(count), _stream())
    return out, count


def component_largest(size, out=None):
    """size: the int32 sizes of component_sizes -> key: one int64 on the GPU holding (size << 32) | (0xFFFFFFFF - root) of the largest
    component, the smallest root among equal sizes; 0 when there is none.  out: an int64 element to write into"""
    _dense(size, torch.int32, 'component_largest: size', 'int32')
    if out is None:
        out = torch.zeros(1, dtype=torch.int64, device=size.device)
    elif _dense(out, torch.int64, 'component_largest: out', 'int64').numel() != 1:
        raise ValueError('component_largest: out must be one int64 value on the GPU')
    lib().call('bts_component_largest', _p(size), size.numel(), _p(out), _stream())
    return out


def components_apply(lab, comp, size, key=None, min_voxels=0, largest_only=False, fill=0, removed=None):
    """in place on the dense uint8 map `lab`: every voxel of a component (comp, size as above) that fails `size >= min_voxels and (not
    largest_only or it is the component of key)` becomes `fill`; no other voxel is written
    -> removed: two int64 on the GPU, += (voxels, components) removed.  removed: a zeroed (or partly filled) pair to add into"""
    _dense(lab, torch.uint8, 'components_apply: lab', 'uint8')
    _dense(comp, torch.int32, 'components_apply: comp', 'int32')
    _dense(size, torch.int32, 'components_apply: size', 'int32')
    n = lab.numel()
    if comp.numel() != n or size.numel() != n:
        raise ValueError('components_apply: lab holds %d voxels, comp %d, size %d' % (n, comp.numel(), size.numel()))
    if largest_only and key is None:
        raise ValueError('components_apply: largest_only needs the key of component_largest')
    if key is not None and _dense(key, torch.int64, 'components_apply: key', 'int64').numel() != 1:
        raise ValueError('components_apply: key must be one int64 value on the GPU')
    if removed is None:
        removed = torch.zeros(2, dtype=torch.int64, device=lab.device)
    elif _dense(removed, torch.int64, 'components_apply: removed', 'int64').numel() != 2:
        raise ValueError('components_apply: removed must be two int64 values on the GPU')
    lib().call('bts_components_apply', _p(lab), _p(comp), _p(size), _p(key), n, int(min_voxels), 1 if largest_only else 0, int(fill),
               _p(removed[0:1]), _p(removed[1:2]), _stream())
    return removed


def region_relabel(lab, class_mask, fill, limit, K=4, changed=None):
    """in place on the dense uint8 map `lab`: when the region (K, class_mask as in components3d) holds between 1 and limit - 1 voxels,
    each becomes `fill` -> changed: one int64 on the GPU, += their number.  The count is taken on the device (label_confusion of the map
    with itself) and the decision is made there.  changed: a zeroed (or partly filled) int64 element to add into"""
    _dense(lab, torch.uint8, 'region_relabel: lab', 'uint8')
    if changed is None:
        changed = torch.zeros(1, dtype=torch.int64, device=lab.device)
    elif _dense(changed, torch.int64, 'region_relabel: changed', 'int64').numel() != 1:
        raise ValueError('region_relabel: changed must be one int64 value on the GPU')
    flat = lab.view(-1)
    conf = label_confusion(flat, flat, K)
    lib().call('bts_region_relabel', _p(lab), lab.numel(), int(K), int(class_mask), int(fill), _p(conf), int(limit), _p(changed),
               _stream())
    return changed


# ---- between the labelling and the distances of a lesion-wise score (csrc/lesion.hip) ----
def _volume3(t, dtype, name, what):
    _dense(t, dtype, name, what)
    if t.dim() != 3:
        raise ValueError('%s must have shape (D,H,W), got %s' % (name, tuple(t.shape)))
    return t


def dilate3d(lab, class_mask, K=4, connectivity=18, iterations=1, out=None, fuse=0):
    """lab: dense uint8 label map (D,H,W) on the GPU; the region is the set of classes min(label, K-1) whose bit is set in class_mask;
    connectivity 6 | 18 | 26 (scipy's generate_binary_structure(3, 1 | 2 | 3)); iterations >= 0
    -> uint8 (D,H,W): 1 where scipy.ndimage.binary_dilation(region, structure, iterations, border_value=0) is set, 0 elsewhere (the
    region itself for 0 iterations).  out: a dense uint8 tensor of lab's size to write into, not lab itself; fuse: iterations run per
    pass over the volume, 1..6 (0: the library's default)"""
    _volume3(lab, torch.uint8, 'dilate3d: lab', 'uint8')
    if out is None:
        out = torch.empty_like(lab)
    elif _dense(out, torch.uint8, 'dilate3d: out', 'uint8').numel() != lab.numel():
        raise ValueError('dilate3d: out holds %d voxels, lab %d' % (out.numel(), lab.numel()))
    elif out.data_ptr() == lab.data_ptr():
        raise ValueError('dilate3d: out must not be lab (a tile reads its neighbours\' voxels)')
    d, h, w = lab.shape
    nb = lib().query('bts_dilate3d_workspace', d, h, w, int(iterations), int(fuse))
    ws = workspace(nb, lab.device) if nb else None
    lib().call('bts_dilate3d', _p(lab), _p(out), d, h, w, int(K), int(class_mask), int(connectivity), int(iterations), int(fuse),
               _p(ws), _stream())
    return out


def lesion_pairs_capacity(n_td, n_pred):
    """slots of the pairing table for n_td dilated lesions and n_pred predicted components: a power of two, at least four times their
    sum (a component usually meets one lesion and a lesion a few components; a table that is too small is grown, not an error)"""
    need = 4 * (max(int(n_td), 0) + max(int(n_pred), 0))
    cap = 256
    while cap < need:
        cap *= 2
    return cap


def lesion_pairs(td_comp, truth, pred_comp, class_mask, K=4, counts=None, capacity=None, lesion_vox=None):
    """td_comp, pred_comp: the int32 maps components3d gives for the dilated truth and for the prediction; truth: the dense uint8 truth
    map of the same size, its region K / class_mask
    -> (rows: int64 numpy (pairs, 4), one row (lesion_root, pred_root, reach, overlap) per pair of a dilated component and a predicted
    component that share a voxel -- reach: the voxels they share, overlap: those of them that are truth -- in lexicographic order;
    lesion_vox: int32 (n,) on the GPU, lesion_vox[r] = the truth voxels inside the dilated component of root r, 0 elsewhere).
    counts: (dilated components, predicted components) as host integers, from which the table's capacity is derived; counted here (one
    more host read) when neither they nor `capacity` are given.  A table that proves too small is grown and the pass run again: the rows
    do not depend on the capacity.  One host read per pass.  lesion_vox: a dense int32 tensor of n values to write into"""
    _dense(td_comp, torch.int32, 'lesion_pairs: td_comp', 'int32')
    _dense(pred_comp, torch.int32, 'lesion_pairs: pred_comp', 'int32')
    _dense(truth, torch.uint8, 'lesion_pairs: truth', 'uint8')
    n = td_comp.numel()
    if pred_comp.numel() != n or truth.numel() != n:
        raise ValueError('lesion_pairs: td_comp holds %d voxels, truth %d, pred_comp %d' % (n, truth.numel(), pred_comp.numel()))
    if lesion_vox is None:
        lesion_vox = torch.empty(n, dtype=torch.int32, device=td_comp.device)
    elif _dense(lesion_vox, torch.int32, 'lesion_pairs: lesion_vox', 'int32').numel() != n:
        raise ValueError('lesion_pairs: lesion_vox holds %d values, td_comp %d' % (lesion_vox.numel(), n))
    if capacity is None:
        if counts is None:
            both = torch.zeros(2, dtype=torch.int64, device=td_comp.device)
            scratch = torch.empty(n, dtype=torch.int32, device=td_comp.device)
            component_sizes(td_comp, out=scratch, count=both[0:1])
            component_sizes(pred_comp, out=scratch, count=both[1:2])
            counts = both.cpu().tolist()
        capacity = lesion_pairs_capacity(*counts)
    capacity = int(capacity)
    if capacity < 1:
        raise ValueError('lesion_pairs: the capacity must be positive, got %r' % (capacity,))
    while True:
        lib().query('bts_lesion_pairs_table_bytes', capacity)
        buf = torch.empty(2 + 2 * capacity, dtype=torch.int64, device=td_comp.device)       # status, keys, (reach, overlap) pairs
        lib().call('bts_lesion_pairs', _p(td_comp), _p(truth), _p(pred_comp), n, int(K), int(class_mask), _p(lesion_vox), _p(buf[2:]),
                   capacity, _p(buf[0:2]), _stream())
        host = buf.cpu().numpy()                                                            # the one read of this pass
        stored, refused = int(host[0]), int(host[1])
        if refused == 0:
            break
        capacity = lesion_pairs_capacity(stored + refused, 0)                               # enough by construction: one rerun
    keys = host[2:2 + capacity]
    cnt = host[2 + capacity:].view(np.int32).reshape(capacity, 2)
    used = np.nonzero(keys)[0]
    rows = np.empty((len(used), 4), dtype=np.int64)
    rows[:, 0] = (keys[used] >> 32) - 1
    rows[:, 1] = (keys[used] & 0xFFFFFFFF) - 1
    rows[:, 2:] = cnt[used]
    if len(used) != stored:
        raise RuntimeError('lesion_pairs: the table holds %d pairs, its status word says %d' % (len(used), stored))
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))], lesion_vox


def _roots(roots, name, device):
    """-> (dense int32 tensor on the GPU or None, length); a host sequence is checked to ascend and uploaded"""
    if isinstance(roots, torch.Tensor):
        _dense(roots, torch.int32, name, 'int32')
        return (roots if roots.numel() else None), roots.numel()
    r = np.asarray(roots, dtype=np.int64).reshape(-1)
    if len(r) and (r[0] < 0 or r[-1] >= 2 ** 31 - 1 or (np.diff(r) <= 0).any()):
        raise ValueError('%s must ascend strictly inside [0, 2^31 - 1)' % name)
    return (torch.from_numpy(r.astype(np.int32)).to(device) if len(r) else None), len(r)


def component_boxes(comp, roots, out=None):
    """comp: the int32 map (D,H,W) of components3d; roots: ASCENDING roots, a dense int32 tensor on the GPU or a host sequence
    -> int32 (len(roots), 6) on the GPU: the half-open bounding box (d0,h0,w0,d1,h1,w1) of each root's component.  out: a dense int32
    tensor of that size to write into"""
    _volume3(comp, torch.int32, 'component_boxes: comp', 'int32')
    rt, m = _roots(roots, 'component_boxes: roots', comp.device)
    if out is None:
        out = torch.empty((m, 6), dtype=torch.int32, device=comp.device)
    elif _dense(out, torch.int32, 'component_boxes: out', 'int32').numel() != 6 * m:
        raise ValueError('component_boxes: out must hold %d int32 values' % (6 * m))
    d, h, w = comp.shape
    lib().call('bts_component_boxes', _p(comp), d, h, w, _p(rt), m, _p(out), _stream())
    return out


def lesion_crop(td_comp, truth, pred_comp, class_mask, box, td_root, roots, K=4, out=None):
    """td_comp, truth, pred_comp as in lesion_pairs, shape (D,H,W); box: host (d0,h0,w0,d1,h1,w1), half-open and inside the volume;
    td_root: the root of one dilated component; roots: ASCENDING roots of predicted components (tensor or host sequence)
    -> (g, m): dense uint8 maps of the box's extent; g = 1 where the voxel is truth inside that dilated component, m = 1 where the
    voxel's predicted component is one of `roots`.  out: a pair of dense uint8 tensors of the box's size to write into"""
    _volume3(td_comp, torch.int32, 'lesion_crop: td_comp', 'int32')
    _volume3(pred_comp, torch.int32, 'lesion_crop: pred_comp', 'int32')
    _volume3(truth, torch.uint8, 'lesion_crop: truth', 'uint8')
    if tuple(td_comp.shape) != tuple(truth.shape) or tuple(pred_comp.shape) != tuple(truth.shape):
        raise ValueError('lesion_crop: the three maps differ in shape: %s, %s, %s' %
                         (tuple(td_comp.shape), tuple(truth.shape), tuple(pred_comp.shape)))
    d, h, w = truth.shape
    box = tuple(int(v) for v in box)
    if len(box) != 6 or min(box[:3]) < 0 or any(b1 <= b0 for b0, b1 in zip(box[:3], box[3:])) or any(b1 > s for b1, s in zip(box[3:], (d, h, w))):
        raise ValueError('lesion_crop: box must be a non-empty half-open (d0,h0,w0,d1,h1,w1) inside %s, got %r' % ((d, h, w), box))
    ext = tuple(b1 - b0 for b0, b1 in zip(box[:3], box[3:]))
    nbox = ext[0] * ext[1] * ext[2]
    rt, m = _roots(roots, 'lesion_crop: roots', truth.device)
    if out is None:
        out = (torch.empty(ext, dtype=torch.uint8, device=truth.device), torch.empty(ext, dtype=torch.uint8, device=truth.device))
    else:
        for t, name in zip(out, ('g', 'm')):
            if _dense(t, torch.uint8, 'lesion_crop: out ' + name, 'uint8').numel() != nbox:
                raise ValueError('lesion_crop: out %s holds %d voxels, the box %d' % (name, t.numel(), nbox))
    lib().call('bts_lesion_crop', _p(td_comp), _p(truth), _p(pred_comp), d, h, w, int(K), int(class_mask), *box, int(td_root), _p(rt), m,
               _p(out[0]), _p(out[1]), _stream())
    return out


# ---- training-time augmentation on the device ----
def channel_moments(x):
    """per-channel (mean, population variance) over all voxels of a dense (..., C) tensor, C <= 16 -> two (C,) tensors"""
    _check(x, 'x')
    c = x.shape[-1]
    nvox = x.numel() // c
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    var = torch.empty(c, dtype=torch.float32, device=x.device)
    nb = lib().query('bts_channel_moments_workspace', c)
    ws = workspace(nb, x.device)
    lib().call('bts_channel_moments', _p(x.contiguous()), _p(mean), _p(var), _p(ws), nb, nvox, c, c, _stream())
    return mean, var


def augment_crop(x, y, var, crop, offsets, flip_mask, shift, scale, out_ch):
    """x: (S0,S1,S2,C), y: (S0,S1,S2) or (S0,S1,S2,1) float labels, var: (C,) device tensor; shift/scale: C python floats
    -> (x_out (T0,T1,T2,C), y_out (T0,T1,T2,out_ch))"""
    s0, s1, s2, c = x.shape
    t0, t1, t2 = crop
    xo = torch.empty((t0, t1, t2, c), dtype=torch.float32, device=x.device)
    yo = torch.empty((t0, t1, t2, out_ch), dtype=torch.float32, device=x.device)
    sh = (ctypes.c_float * c)(*[float(v) for v in shift])
    sc = (ctypes.c_float * c)(*[float(v) for v in scale])
    lib().call('bts_augment_crop', _p(x.contiguous()), _p(y.contiguous()), _p(var), _p(xo), _p(yo), s0, s1, s2, c, t0, t1, t2,
               int(offsets[0]), int(offsets[1]), int(offsets[2]), int(flip_mask), ctypes.cast(sh, ctypes.c_void_p),
               ctypes.cast(sc, ctypes.c_void_p), int(out_ch), _stream())
    return xo, yo


def augment_batch_max():
    """examples one launch of bts_augment_batch carries (ops.augment_batch takes any number: the call splits)"""
    return int(lib().query('bts_augment_batch_max'))


def augment_batch(xs, ys, variances, crop, offsets, flip_masks, shifts, scales, out_ch, channels_first=False, out=None):
    """augment_crop for N examples in one launch, written straight into the batch tensors.  xs: N dense (S0,S1,S2,C) tensors of one
    shape, ys: their labels, variances: N (C,) device tensors; offsets: N triples, flip_masks: N ints, shifts / scales: N lists of
    C floats -> (x (N,T0,T1,T2,C), y (N,T0,T1,T2,out_ch)), or with channels_first (N,C,T0,T1,T2), (N,out_ch,T0,T1,T2).
    out: (x, y) dense tensors of those shapes to write into (views of larger buffers are fine)"""
    n = len(xs)
    if n == 0 or not (len(ys) == len(variances) == len(offsets) == len(flip_masks) == len(shifts) == len(scales) == n):
        raise ValueError('augment_batch: %d examples need as many labels, variances and draws' % n)
    s0, s1, s2, c = xs[0].shape
    for x, y, v in zip(xs, ys, variances):
        _check(x, 'x'), _check(y, 'y'), _check(v, 'var')
        if tuple(x.shape) != (s0, s1, s2, c) or y.numel() != s0 * s1 * s2 or v.numel() != c:
            raise ValueError('augment_batch: every example must be a (%d,%d,%d,%d) volume with its labels and %d variances' % (s0, s1, s2, c, c))
        if not (x.is_contiguous() and y.is_contiguous() and v.is_contiguous()):
            raise ValueError('augment_batch: dense tensors only')
    t0, t1, t2 = (int(t) for t in crop)
    dev = xs[0].device
    xshape = (n, c, t0, t1, t2) if channels_first else (n, t0, t1, t2, c)
    yshape = (n, out_ch, t0, t1, t2) if channels_first else (n, t0, t1, t2, out_ch)
    if out is None:
        xo = torch.empty(xshape, dtype=torch.float32, device=dev)
        yo = torch.empty(yshape, dtype=torch.float32, device=dev)
    else:
        xo, yo = out
        _check(xo, 'out x'), _check(yo, 'out y')
        if tuple(xo.shape) != xshape or tuple(yo.shape) != yshape or not (xo.is_contiguous() and yo.is_contiguous()):
            raise ValueError('augment_batch: out must be dense %s and %s tensors' % (xshape, yshape))
    ptrs = ctypes.c_void_p * n
    off = (ctypes.c_int * (3 * n))(*[int(o) for tri in offsets for o in tri])
    fl = (ctypes.c_int * n)(*[int(f) for f in flip_masks])
    sh = (ctypes.c_float * (n * c))(*[float(v) for row in shifts for v in row])
    sc = (ctypes.c_float * (n * c))(*[float(v) for row in scales for v in row])
    as_p = lambda a: ctypes.cast(a, ctypes.c_void_p)      # noqa: E731
    lib().call('bts_augment_batch', as_p(ptrs(*[x.data_ptr() for x in xs])), as_p(ptrs(*[y.data_ptr() for y in ys])),
               as_p(ptrs(*[v.data_ptr() for v in variances])), _p(xo), _p(yo), n, s0, s1, s2, c, t0, t1, t2, as_p(off), as_p(fl), as_p(sh),
               as_p(sc), int(out_ch), 1 if channels_first else 0, _stream())
    return xo, yo


def augment_spatial_batch_max():
    """examples one launch of bts_augment_spatial_batch carries (ops.augment_spatial_batch takes any number: the call splits)"""
    return int(lib().query('bts_augment_spatial_batch_max'))


def augment_spatial_batch(xs, ys, variances, crop, offsets, flip_masks, shifts, scales, out_ch, spatial, matrices, phis, spacings,
                          fills=None, channels_first=False, out=None):
    """augment_batch with a spatial transform per example (bts_augment_spatial_batch: s = o + (T-1)/2 + M (t~ - (T-1)/2) + u(t~),
    trilinear image with `fill` outside the volume, nearest labels).  The arguments of augment_batch plus, per example: spatial (a
    false flag: the plain copy, bit-equal to augment_batch), matrices (9 floats, row-major, or a 3x3 nesting), phis (a dense fp32
    (G0,G1,G2,3) device tensor with G_k = (T_k-1)//spacing + 4, or None for no elastic part), spacings (ints >= 1) and fills (C floats
    each; None: zeros) -> the tensors of augment_batch"""
    n = len(xs)
    if n == 0 or not (len(ys) == len(variances) == len(offsets) == len(flip_masks) == len(shifts) == len(scales) == n):
        raise ValueError('augment_spatial_batch: %d examples need as many labels, variances and draws' % n)
    if not (len(spatial) == len(matrices) == len(phis) == len(spacings) == n) or (fills is not None and len(fills) != n):
        raise ValueError('augment_spatial_batch: %d examples need as many flags, matrices, fields, spacings and fills' % n)
    s0, s1, s2, c = xs[0].shape
    for x, y, v in zip(xs, ys, variances):
        _check(x, 'x'), _check(y, 'y'), _check(v, 'var')
        if tuple(x.shape) != (s0, s1, s2, c) or y.numel() != s0 * s1 * s2 or v.numel() != c:
            raise ValueError('augment_spatial_batch: every example must be a (%d,%d,%d,%d) volume with its labels and %d variances'
                             % (s0, s1, s2, c, c))
        if not (x.is_contiguous() and y.is_contiguous() and v.is_contiguous()):
            raise ValueError('augment_spatial_batch: dense tensors only')
    t0, t1, t2 = (int(t) for t in crop)
    mats = []
    for m in matrices:
        flat = [float(v) for row in m for v in row] if len(m) == 3 else [float(v) for v in m]
        if len(flat) != 9:
            raise ValueError('augment_spatial_batch: a matrix is 9 floats')
        mats += flat
    for ph, sp in zip(phis, spacings):
        if int(sp) < 1:
            raise ValueError('augment_spatial_batch: spacing must be >= 1, got %r' % (sp,))
        if ph is None:
            continue
        _check(ph, 'phi')
        g = tuple((t - 1) // int(sp) + 4 for t in (t0, t1, t2)) + (3,)
        if tuple(ph.shape) != g or not ph.is_contiguous():
            raise ValueError('augment_spatial_batch: phi must be a dense %s tensor for spacing %d, got %s' % (g, int(sp), tuple(ph.shape)))
    if fills is None:
        fills = [[0.0] * c] * n
    if any(len(f) != c for f in fills):
        raise ValueError('augment_spatial_batch: a fill is %d floats' % c)
    dev = xs[0].device
    xshape = (n, c, t0, t1, t2) if channels_first else (n, t0, t1, t2, c)
    yshape = (n, out_ch, t0, t1, t2) if channels_first else (n, t0, t1, t2, out_ch)
    if out is None:
        xo = torch.empty(xshape, dtype=torch.float32, device=dev)
        yo = torch.empty(yshape, dtype=torch.float32, device=dev)
    else:
        xo, yo = out
        _check(xo, 'out x'), _check(yo, 'out y')
        if tuple(xo.shape) != xshape or tuple(yo.shape) != yshape or not (xo.is_contiguous() and yo.is_contiguous()):
            raise ValueError('augment_spatial_batch: out must be dense %s and %s tensors' % (xshape, yshape))
    ptrs = ctypes.c_void_p * n
    off = (ctypes.c_int * (3 * n))(*[int(o) for tri in offsets for o in tri])
    fl = (ctypes.c_int * n)(*[int(f) for f in flip_masks])
    sh = (ctypes.c_float * (n * c))(*[float(v) for row in shifts for v in row])
    sc = (ctypes.c_float * (n * c))(*[float(v) for row in scales for v in row])
    on = (ctypes.c_int * n)(*[1 if f else 0 for f in spatial])
    mm = (ctypes.c_float * (9 * n))(*mats)
    spc = (ctypes.c_int * n)(*[int(v) for v in spacings])
    fi = (ctypes.c_float * (n * c))(*[float(v) for row in fills for v in row])
    as_p = lambda a: ctypes.cast(a, ctypes.c_void_p)      # noqa: E731
    lib().call('bts_augment_spatial_batch', as_p(ptrs(*[x.data_ptr() for x in xs])), as_p(ptrs(*[y.data_ptr() for y in ys])),
               as_p(ptrs(*[v.data_ptr() for v in variances])), _p(xo), _p(yo), n, s0, s1, s2, c, t0, t1, t2, as_p(off), as_p(fl), as_p(sh),
               as_p(sc), as_p(on), as_p(mm), as_p(ptrs(*[None if ph is None else ph.data_ptr() for ph in phis])), as_p(spc), as_p(fi),
               int(out_ch), 1 if channels_first else 0, _stream())
    return xo, yo


# ---- intensity augmentation of an augmented batch (bts_intensity_batch) ----
INTENSITY_NOISE, INTENSITY_BLUR, INTENSITY_BRIGHT, INTENSITY_CONTRAST, INTENSITY_GAMMA, INTENSITY_INVERT = 1, 2, 4, 8, 16, 32


def intensity_blur_weights(sigma):
    """(radius, the radius + 1 float weights w[|j|]) of the Gaussian blur of `sigma` as bts_intensity_batch applies it (host only)"""
    buf = (ctypes.c_float * 17)()
    r = lib().probe('bts_intensity_blur_weights', float(sigma), ctypes.cast(buf, ctypes.c_void_p))
    if r < 0:
        raise ValueError('intensity_blur_weights: sigma must be positive with a radius int(4 sigma + 0.5) <= 16, got %r' % (sigma,))
    return int(r), [float(buf[k]) for k in range(r + 1)]


def intensity_batch(x, params, keys, channels_first=False):
    """Gaussian noise, Gaussian blur, brightness, contrast and gamma on the batch an augment launch wrote, IN PLACE (-> x).
    x: dense fp32 (N,T0,T1,T2,C), or (N,C,T0,T1,T2) with channels_first.  params: N rows of C entries
    (flags, s, sigma, m, f, gamma), flags a sum of INTENSITY_*; a stage whose flag is off ignores its number.  keys: N pairs
    (k0, k1) of uint32, the Philox key of each example's noise.  The semantics are written above bts_intensity_batch in
    include/bts_hip.h; an (n, c) without a flag is not written."""
    _check(x, 'x')
    if x.dtype != torch.float32 or x.dim() != 5 or not x.is_contiguous():
        raise ValueError('intensity_batch: x must be a dense float32 batch of five dimensions, got %s %s' % (x.dtype, tuple(x.shape)))
    if channels_first:
        n, c, t0, t1, t2 = x.shape
    else:
        n, t0, t1, t2, c = x.shape
    if n == 0 or len(params) != n or len(keys) != n:
        raise ValueError('intensity_batch: %d examples need as many parameter rows and keys' % n)
    fl, pr, ky = [], [], []
    for row, key in zip(params, keys):
        if len(row) != c or len(key) != 2:
            raise ValueError('intensity_batch: a parameter row has %d entries of (flags, s, sigma, m, f, gamma), a key two words' % c)
        for e in row:
            if len(e) != 6:
                raise ValueError('intensity_batch: an entry is (flags, s, sigma, m, f, gamma)')
            fl.append(int(e[0]))
            pr.extend(float(v) for v in e[1:])
        ky.extend(int(k) & 0xffffffff for k in key)
    nb = lib().query('bts_intensity_batch_workspace', n, t0, t1, t2, c)
    ws = workspace(nb, x.device)
    as_p = lambda a: ctypes.cast(a, ctypes.c_void_p)      # noqa: E731
    lib().call('bts_intensity_batch', _p(x), n, t0, t1, t2, c, 1 if channels_first else 0, as_p((ctypes.c_int * len(fl))(*fl)),
               as_p((ctypes.c_float * len(pr))(*pr)), as_p((ctypes.c_uint32 * len(ky))(*ky)), _p(ws), ws.numel(), _stream())
    return x


# ---- the nested BraTS regions WT, TC, ET as targets and as the decoded prediction (csrc/regions.hip) ----
REGION_CHANNELS = 3


def _region_channels(c, who):
    if int(c) != REGION_CHANNELS:
        raise ValueError('%s: the BraTS regions (WT, TC, ET) are three channels, got %d' % (who, int(c)))


def region_targets(y, channels_first=False):
    """the label batch an augment launch wrote (one-hot minus the background), IN PLACE (-> y): (l1, l2, l3) -> the nested regions
    (l1 + l2 + l3, l1 + l3, l3) = (WT, TC, ET).  y: dense fp32 (N, ..., 3), or (N, 3, ...) with channels_first; a view into a larger
    buffer is fine"""
    if not isinstance(y, torch.Tensor) or not y.is_cuda or y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError('region_targets: y must be a dense float32 tensor on the GPU')
    if y.dim() < (3 if channels_first else 2):
        raise ValueError('region_targets: y must be (N, ..., 3), or (N, 3, ...) with channels_first, got shape %s' % (tuple(y.shape),))
    c = y.shape[1] if channels_first else y.shape[-1]
    _region_channels(c, 'region_targets')
    n = y.shape[0]
    if y.numel() == 0:
        raise ValueError('region_targets: y is empty, shape %s' % (tuple(y.shape),))
    lib().call('bts_region_targets', _p(y), n, y.numel() // (n * c), c, 1 if channels_first else 0, _stream())
    return y


def region_dice_sums(y_true, y_pred, want_labels=True):
    """y_true, y_pred: (N,D,H,W,3) channel slices of dense NDHWC buffers, channels (WT, TC, ET) -> (table (9,) float64: (I, P, T) per
    region, counted exactly with p > 0.5 and t > 0.5 -- what dice_metric_value(table, w, 3, False) reduces; labels (N,D,H,W) uint8:
    the decode of region_finish with p > 0.5, coded 0, 1, 2, 3 (ET) like dice_metric_sums' map, or None)"""
    if y_true.dim() != 5 or tuple(y_true.shape) != tuple(y_pred.shape):
        raise ValueError('region_dice_sums: y_true and y_pred must be (N,D,H,W,3) tensors of one shape, got %s and %s' %
                         (tuple(y_true.shape), tuple(y_pred.shape)))
    n, d, h, w, c = y_pred.shape
    _region_channels(c, 'region_dice_sums')
    ldt, ldp = ld_of(y_true), ld_of(y_pred)
    table = torch.empty(3 * c, dtype=torch.float64, device=y_pred.device)
    labels = torch.empty((n, d, h, w), dtype=torch.uint8, device=y_pred.device) if want_labels else None
    lib().call('bts_region_dice_sums', _p(y_true), _p(y_pred), _p(labels), _p(table), n * d * h * w, c, ldt, ldp, _stream())
    return table, labels


def region_finish(prob, bmask, threshold=0.5, want_probabilities=True, want_labels=True):
    """tta_finish for a network trained on the regions: prob (N,D,H,W,3) = (WT, TC, ET), bmask one float per voxel
    -> (prob * bmask, uint8 label map (N,D,H,W)): 4 where et >= threshold, else 1 where tc >= threshold, else 2 where wt >= threshold,
    else 0 (the masked probabilities; the overwrite rule, not the nested one), 0 where masked out"""
    _check(prob, 'prob'), _check(bmask, 'bmask')
    if prob.dim() != 5:
        raise ValueError('region_finish: prob must be (N,D,H,W,3), got shape %s' % (tuple(prob.shape),))
    n, d, h, w, c = prob.shape
    _region_channels(c, 'region_finish')
    if bmask.numel() != n * d * h * w:
        raise ValueError('region_finish: bmask holds %d values, prob %d voxels' % (bmask.numel(), n * d * h * w))
    y = torch.empty(tuple(prob.shape), dtype=torch.float32, device=prob.device) if want_probabilities else None
    labels = torch.empty((n, d, h, w), dtype=torch.uint8, device=prob.device) if want_labels else None
    lib().call('bts_region_finish', _p(prob.contiguous()), _p(bmask.contiguous()), _p(y), _p(labels), n * d * h * w, c,
               float(threshold), _stream())
    return y, labels


# ---- dataset preprocessing on the device (preprocess.py:17-131) ----
def _window(v, c, name):
    """(st0, st1) of a view made by slicing a dense (S0,S1,S2,c) parent on its three spatial axes; no copy is ever made here"""
    if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.float32:
        raise ValueError('%s must be a float32 tensor on the GPU' % name)
    if v.dim() != 4 or v.shape[3] != c or min(v.shape) < 1:
        raise ValueError('%s must have shape (T0,T1,T2,%d), got %s' % (name, c, tuple(v.shape)))
    if v.stride(3) != 1 or v.stride(2) != c:
        raise ValueError('%s must be a spatial slice of a dense channels-last volume (strides (*,*,%d,1)), got strides %s'
                         % (name, c, v.stride()))
    if v.stride(1) < v.shape[2] * c or v.stride(0) < v.shape[1] * v.stride(1):
        raise ValueError('%s: strides %s overlap for shape %s' % (name, v.stride(), tuple(v.shape)))
    return v.stride(0), v.stride(1)


def _f64(t, n, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or t.numel() != n or not t.is_contiguous():
        raise ValueError('%s must be %d dense float64 values on the GPU' % (name, n))
    return t


def prepro_occupancy(x, occ):
    """sets occ[a] = 1 (int32, S0+S1+S2 entries, axis 0 first) for every plane of every axis of the dense (S0,S1,S2,C) volume x that
    holds an x != 0; never clears a flag, so one zeroed buffer collects a whole dataset"""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError('prepro_occupancy: x must be a dense (S0,S1,S2,C) volume')
    _window(x, x.shape[3], 'prepro_occupancy: x')
    if not x.is_contiguous():
        raise ValueError('prepro_occupancy: x must be dense, got strides %s' % (x.stride(),))
    s0, s1, s2, c = x.shape
    if not isinstance(occ, torch.Tensor) or not occ.is_cuda or occ.dtype != torch.int32 or occ.numel() != s0 + s1 + s2 or not occ.is_contiguous():
        raise ValueError('prepro_occupancy: occ must be %d dense int32 values on the GPU' % (s0 + s1 + s2))
    lib().call('bts_prepro_occupancy', _p(x), _p(occ), s0, s1, s2, c, _stream())
    return occ


def prepro_sums(v, acc, mean=None):
    """window v (T0,T1,T2,C) of a dense volume.  mean None: acc[0:C] += sum x, acc[C:2C] += #(x > 0); mean (C float64 on the GPU):
    acc[0:C] += sum (x - mean)^2.  acc: float64 on the GPU (2C / C values); fp64 throughout, fixed summation order"""
    if not isinstance(v, torch.Tensor) or v.dim() != 4:
        raise ValueError('prepro_sums: v must be a (T0,T1,T2,C) window')
    c = v.shape[3]
    st0, st1 = _window(v, c, 'prepro_sums: v')
    _f64(acc, c if mean is not None else 2 * c, 'prepro_sums: acc')
    if mean is not None:
        _f64(mean, c, 'prepro_sums: mean')
    nb = lib().query('bts_prepro_workspace', c)
    ws = workspace(nb, v.device)
    lib().call('bts_prepro_sums', _p(v), st0, st1, v.shape[0], v.shape[1], v.shape[2], c, _p(mean), _p(acc), _p(ws), nb, _stream())
    return acc


def prepro_crop_norm(v, yv, mean, std):
    """windows v (T0,T1,T2,C) and yv (T0,T1,T2,1) (or None) -> dense (float((double(x) - mean) / std), y with labels >= 4 -> 3);
    mean, std: C float64 values on the GPU"""
    if not isinstance(v, torch.Tensor) or v.dim() != 4:
        raise ValueError('prepro_crop_norm: v must be a (T0,T1,T2,C) window')
    c = v.shape[3]
    st0, st1 = _window(v, c, 'prepro_crop_norm: x')
    _f64(mean, c, 'prepro_crop_norm: mean')
    _f64(std, c, 'prepro_crop_norm: std')
    t0, t1, t2 = v.shape[:3]
    xo = torch.empty((t0, t1, t2, c), dtype=torch.float32, device=v.device)
    yo, yst0, yst1 = None, 0, 0
    if yv is not None:
        if not isinstance(yv, torch.Tensor) or yv.dim() != 4 or tuple(yv.shape) != (t0, t1, t2, 1):
            raise ValueError('prepro_crop_norm: y must have shape %s' % ((t0, t1, t2, 1),))
        yst0, yst1 = _window(yv, 1, 'prepro_crop_norm: y')
        yo = torch.empty((t0, t1, t2, 1), dtype=torch.float32, device=v.device)
    lib().call('bts_prepro_crop_norm', _p(v), _p(yv), st0, st1, yst0, yst1, t0, t1, t2, c, _p(mean), _p(std), _p(xo), _p(yo), _stream())
    return xo, yo


# ---- per-case normalisation over the brain voxels ----
def check_clip(clip, who='clip'):
    """None | (lo, hi) with 0 <= lo <= hi <= 100 -> None | (float, float)"""
    if clip is None:
        return None
    try:
        lo, hi = (float(v) for v in clip)
    except (TypeError, ValueError):
        raise ValueError('%s must be None or two percentiles (lo, hi), got %r' % (who, clip))
    if not 0.0 <= lo <= hi <= 100.0:
        raise ValueError('%s: percentiles must satisfy 0 <= lo <= hi <= 100, got %r' % (who, clip))
    return lo, hi


def case_norm(x, mask=None, clip=None, y=None, out=None):
    """normalise one case on its own voxels: window x (T0,T1,T2,C) of a dense channels-last volume -> (xn, stats), or (xn, yn, stats)
    with a label window y (T0,T1,T2,1) (labels >= 4 -> 3, as prepro_crop_norm).  mask: float32 window (T0,T1,T2) or (T0,T1,T2,1),
    non-zero = inside; None: a voxel is inside when any of its channels is > 0.  clip: None or the percentiles (lo, hi) the inside values of
    each channel are clamped to first.  xn (dense, `out` when given) = float32((clamp(x) - mean_c) / std_c) inside, evaluated in
    float64, +0.0 outside, +0.0 throughout a channel whose deviation is 0; mean_c and std_c (population) over the inside voxels.
    stats: 1 + 4C float64 on the device: n, then (mean, std, lo, hi) per channel.  Everything stays on the stream (bts_case_norm)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError('case_norm: x must be a (T0,T1,T2,C) window')
    c = x.shape[3]
    st0, st1 = _window(x, c, 'case_norm: x')
    t0, t1, t2 = x.shape[:3]
    clip = check_clip(clip, 'case_norm: clip')
    mst0 = mst1 = 0
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) not in ((t0, t1, t2), (t0, t1, t2, 1)):
            raise ValueError('case_norm: mask must have shape %s or %s' % ((t0, t1, t2), (t0, t1, t2, 1)))
        mask = mask if mask.dim() == 4 else mask.unsqueeze(-1)
        mst0, mst1 = _window(mask, 1, 'case_norm: mask')
    yo, yst0, yst1 = None, 0, 0
    if y is not None:
        if not isinstance(y, torch.Tensor) or y.dim() != 4 or tuple(y.shape) != (t0, t1, t2, 1):
            raise ValueError('case_norm: y must have shape %s' % ((t0, t1, t2, 1),))
        yst0, yst1 = _window(y, 1, 'case_norm: y')
        yo = torch.empty((t0, t1, t2, 1), dtype=torch.float32, device=x.device)
    if out is None:
        out = torch.empty((t0, t1, t2, c), dtype=torch.float32, device=x.device)
    elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (t0, t1, t2, c)
          or not out.is_contiguous()):
        raise ValueError('case_norm: out must be a dense float32 tensor of shape %s on the GPU' % ((t0, t1, t2, c),))
    stats = torch.empty(1 + 4 * c, dtype=torch.float64, device=x.device)
    nb = lib().query('bts_case_norm_workspace', c)
    ws = workspace(nb, x.device)
    lo, hi = clip if clip is not None else (0.0, 100.0)
    lib().call('bts_case_norm', _p(x), st0, st1, _p(mask), mst0, mst1, _p(y), yst0, yst1, t0, t1, t2, c, 1 if clip is not None else 0,
               lo, hi, _p(out), _p(yo), _p(stats), _p(ws), nb, _stream())
    return (out, stats) if y is None else (out, yo, stats)


# ---- rigid co-registration by mutual information ----
def _check_bins(bins, who):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 2 <= int(bins) <= 64:
        raise ValueError('%s: bins must be an integer in 2..64, got %r' % (who, bins))
    return int(bins)


def quantize_bins(x, lo, hi, bins=32):
    """dense float32 device tensor -> uint8 tensor of its shape: clamp(floor((double(x) - lo) * bins / (hi - lo)), 0, bins - 1), evaluated
    in float64 (bts_quantize_bins); lo < hi finite, bins in 2..64"""
    bins = _check_bins(bins, 'quantize_bins')
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() < 1:
        raise ValueError('quantize_bins: x must be a dense, non-empty float32 tensor on the GPU')
    try:
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError('quantize_bins: lo and hi must be numbers, got %r and %r' % (lo, hi))
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo and np.isfinite(hi - lo)):
        raise ValueError('quantize_bins: lo < hi must be finite, got %r and %r' % (lo, hi))
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    lib().call('bts_quantize_bins', _p(x), _p(q), x.numel(), lo, hi, bins, _stream())
    return q


def _int3(v, name, who):
    try:
        out = tuple(int(t) for t in v)
        ok = len(out) == 3 and all(float(t) == int(t) for t in v)
    except (TypeError, ValueError):
        out, ok = (), False
    if not ok:
        raise ValueError('%s: %s must be three integers, got %r' % (who, name, v))
    return out


def joint_hist_pv(qf, qm, origin, stride, counts, matrices, bins=32):
    """K joint histograms by partial-volume interpolation (bts_joint_hist_pv): qf (Df,Hf,Wf) and qm (Dm,Hm,Wm) dense uint8 device volumes of
    bin numbers below `bins`; the lattice origin + l * stride, 0 <= l < counts, of the fixed grid; matrices (K,3,4) or (K,4,4) float64, fixed
    voxel -> moving voxel, 1 <= K <= 32 -> (K,bins,bins) int64 on the device, [k][fixed bin][moving bin]; every counted lattice point adds
    32768 to its candidate's histogram"""
    who = 'joint_hist_pv'
    bins = _check_bins(bins, who)
    for t, name in ((qf, 'qf'), (qm, 'qm')):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 3 or not t.is_contiguous() \
                or t.numel() < 1 or t.numel() >= 2 ** 31:
            raise ValueError('%s: %s must be a dense, non-empty (D,H,W) uint8 volume on the GPU' % (who, name))
    if qf.device != qm.device:
        raise ValueError('%s: qf and qm live on different devices' % who)
    o, s, n = _int3(origin, 'origin', who), _int3(stride, 'stride', who), _int3(counts, 'counts', who)
    for a in range(3):
        if o[a] < 0 or s[a] < 1 or n[a] < 1 or o[a] + (n[a] - 1) * s[a] > qf.shape[a] - 1:
            raise ValueError('%s: the lattice origin %s stride %s counts %s does not lie inside the fixed extent %s'
                             % (who, o, s, n, tuple(qf.shape)))
    try:
        m = np.asarray(matrices, dtype=np.float64)
    except (TypeError, ValueError):
        m = np.zeros(0)
    if m.ndim == 3 and m.shape[1:] == (4, 4):
        m = m[:, :3]
    if m.ndim != 3 or m.shape[1:] != (3, 4) or not 1 <= m.shape[0] <= 32 or not np.all(np.isfinite(m)):
        raise ValueError('%s: matrices must be 1..32 finite 3x4 or 4x4 arrays, got shape %s' % (who, np.shape(matrices)))
    k = m.shape[0]
    hist = torch.empty((k, bins, bins), dtype=torch.int64, device=qf.device)
    m12 = (ctypes.c_double * (12 * k))(*[float(v) for v in m.reshape(-1)])
    lib().call('bts_joint_hist_pv', _p(qf), qf.shape[0], qf.shape[1], qf.shape[2], _p(qm), qm.shape[0], qm.shape[1], qm.shape[2],
               o[0], o[1], o[2], s[0], s[1], s[2], n[0], n[1], n[2], m12, k, bins, _p(hist), _stream())
    return hist


# ---- N4 bias-field correction ----
N4_MAX_BINS, N4_MAX_MESH, N4_MAX_AXIS = 1024, 64, 512


def n4_lattice(shape, stride, who='n4'):
    """-> the lattice counts per axis of the strided sub-grid origin stride // 2 (bts_n4_*); 1 <= stride <= extent per axis"""
    shape, stride = _int3(shape, 'shape', who), _int3(stride, 'stride', who)
    if min(shape) < 1 or shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError('%s: the volume must have 1 .. 2^31 - 1 voxels, got shape %s' % (who, shape))
    if any(not 1 <= s <= n for s, n in zip(stride, shape)):
        raise ValueError('%s: stride %s must lie in 1..extent per axis of %s' % (who, stride, shape))
    return tuple((n - 1 - s // 2) // s + 1 for n, s in zip(shape, stride))


def _n4_mesh(mesh, who):
    mesh = _int3(mesh, 'mesh', who)
    if any(not 1 <= m <= N4_MAX_MESH for m in mesh):
        raise ValueError('%s: mesh must lie in 1..%d per axis, got %s' % (who, N4_MAX_MESH, mesh))
    return mesh


def _n4_bins(bins, who):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 2 <= int(bins) <= N4_MAX_BINS:
        raise ValueError('%s: bins must be an integer in 2..%d, got %r' % (who, N4_MAX_BINS, bins))
    return int(bins)


def _n4_dense(t, dtype, shape, name, who):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError('%s: %s must be a dense %s tensor of shape %s on the GPU' % (who, name, str(dtype).replace('torch.', ''), tuple(shape)))
    return t


def _n4_points(t, name, who):
    """a lattice array: dense, three-dimensional, non-empty"""
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.numel() < 1:
        raise ValueError('%s: %s must be a non-empty (n0,n1,n2) lattice array' % (who, name))
    return tuple(t.shape)


def n4_log_lattice(x, mask=None, stride=(1, 1, 1)):
    """dense float32 (D,H,W) device volume -> (v float64, lmask uint8) on the lattice of `stride`: v = log(x) and lmask = 1 where x > 0 and
    finite and mask (uint8 or bool (D,H,W), non-zero = inside; None: everywhere) allows it, 0 and 0 elsewhere (bts_n4_log_lattice)"""
    who = 'n4_log_lattice'
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError('%s: x must be a (D,H,W) volume' % who)
    _n4_dense(x, torch.float32, x.shape, 'x', who)
    n = n4_lattice(x.shape, stride, who)
    s = _int3(stride, 'stride', who)
    if mask is not None:
        if isinstance(mask, torch.Tensor) and mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        _n4_dense(mask, torch.uint8, x.shape, 'mask', who)
    v = torch.empty(n, dtype=torch.float64, device=x.device)
    lm = torch.empty(n, dtype=torch.uint8, device=x.device)
    lib().call('bts_n4_log_lattice', _p(x), _p(mask), x.shape[0], x.shape[1], x.shape[2], s[0], s[1], s[2], _p(v), _p(lm), _stream())
    return v, lm


def n4_hist(v, f, lmask, bins=200):
    """-> (r, lohi, hist): r = v - f on the lattice mask (0 elsewhere), lohi = its exact (min, max) over the mask as 2 float64 on the device
    ((+inf, -inf) for an empty mask), hist = `bins` int64 counts with linear two-bin weights, 2^24 per masked point (bts_n4_range_hist)"""
    who = 'n4_hist'
    bins = _n4_bins(bins, who)
    n = _n4_points(v, 'v', who)
    _n4_dense(v, torch.float64, n, 'v', who)
    _n4_dense(f, torch.float64, n, 'f', who)
    _n4_dense(lmask, torch.uint8, n, 'lmask', who)
    r = torch.empty(n, dtype=torch.float64, device=v.device)
    range4 = torch.empty(4, dtype=torch.float64, device=v.device)
    hist = torch.empty(bins, dtype=torch.int64, device=v.device)
    lib().call('bts_n4_range_hist', _p(v), _p(f), _p(lmask), v.numel(), bins, _p(r), _p(range4), _p(hist), _stream())
    return r, range4[:2], hist


def n4_residual(r, lmask, table, lo, sl):
    """-> res = r - (E[i] (1 - o) + E[i+1] o) on the mask, 0 elsewhere: the table E (`bins` float64 on the device) looked up at
    c = (r - lo) / sl, i = min(floor(c), bins - 2), o = c - i (bts_n4_residual); lo finite, sl >= 0 finite"""
    who = 'n4_residual'
    n = _n4_points(r, 'r', who)
    _n4_dense(r, torch.float64, n, 'r', who)
    _n4_dense(lmask, torch.uint8, n, 'lmask', who)
    if not isinstance(table, torch.Tensor) or table.dim() != 1:
        raise ValueError('%s: the table must be a vector of float64 on the GPU' % who)
    bins = _n4_bins(int(table.numel()), who)
    _n4_dense(table, torch.float64, (bins,), 'table', who)
    lo, sl = float(lo), float(sl)
    if not (np.isfinite(lo) and np.isfinite(sl) and sl >= 0.0):
        raise ValueError('%s: lo must be finite and sl finite and not negative, got %r and %r' % (who, lo, sl))
    res = torch.empty(n, dtype=torch.float64, device=r.device)
    lib().call('bts_n4_residual', _p(r), _p(lmask), _p(table), r.numel(), bins, lo, sl, _p(res), _stream())
    return res


def _n4_geometry(shape, stride, mesh, lmask, who):
    n = n4_lattice(shape, stride, who)
    mesh = _n4_mesh(mesh, who)
    _n4_dense(lmask, torch.uint8, n, 'lmask', who)
    shape, stride = _int3(shape, 'shape', who), _int3(stride, 'stride', who)
    return n, mesh, shape + stride + mesh


def n4_fit(res, lmask, shape, stride, mesh, phi=None):
    """one level of multilevel B-spline approximation of the residuals on the lattice of `stride` in a volume of `shape` -> (num, den,
    dphi), float64 of shape mesh + 3: num = sum w^3 z / S, den = sum w^2 over the masked lattice points in each control point's support,
    dphi = num / den, 0 where den == 0; phi (the same shape), when given, grows by dphi in place (bts_n4_fit)"""
    who = 'n4_fit'
    n, mesh, geo = _n4_geometry(shape, stride, mesh, lmask, who)
    if max(n) > N4_MAX_AXIS:
        raise ValueError('%s: at most %d lattice points per axis, got %s' % (who, N4_MAX_AXIS, n))
    _n4_dense(res, torch.float64, n, 'res', who)
    cp = tuple(m + 3 for m in mesh)
    if phi is not None:
        _n4_dense(phi, torch.float64, cp, 'phi', who)
    num, den, dphi = (torch.empty(cp, dtype=torch.float64, device=res.device) for _ in range(3))
    lib().call('bts_n4_fit', _p(res), _p(lmask), *(geo + (_p(num), _p(den), _p(dphi), _p(phi), _stream())))
    return num, den, dphi


def n4_eval(phi, lmask, f_old, shape, stride, mesh):
    """-> (f_new, parts): the spline of phi (float64, mesh + 3) at every lattice point, and parts (B,2) float64, the sums of
    e = exp(f_new - f_old) and e^2 over the masked points of each run of 1024 lattice points (bts_n4_eval)"""
    who = 'n4_eval'
    n, mesh, geo = _n4_geometry(shape, stride, mesh, lmask, who)
    _n4_dense(phi, torch.float64, tuple(m + 3 for m in mesh), 'phi', who)
    _n4_dense(f_old, torch.float64, n, 'f_old', who)
    f_new = torch.empty(n, dtype=torch.float64, device=phi.device)
    parts = torch.empty((lib().query('bts_n4_eval_parts', n[0] * n[1] * n[2]), 2), dtype=torch.float64, device=phi.device)
    lib().call('bts_n4_eval', _p(phi), *(geo + (_p(f_old), _p(lmask), _p(f_new), _p(parts), _stream())))
    return f_new, parts


def n4_apply(x, phi, mesh, field=False):
    """dense float32 (D,H,W) device volume -> float32(x / exp(spline of phi)) at every voxel; with field=True also float32(exp(spline))
    (bts_n4_apply)"""
    who = 'n4_apply'
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError('%s: x must be a (D,H,W) volume' % who)
    _n4_dense(x, torch.float32, x.shape, 'x', who)
    n4_lattice(x.shape, (1, 1, 1), who)
    mesh = _n4_mesh(mesh, who)
    _n4_dense(phi, torch.float64, tuple(m + 3 for m in mesh), 'phi', who)
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    fld = torch.empty(x.shape, dtype=torch.float32, device=x.device) if field else None
    lib().call('bts_n4_apply', _p(x), x.shape[0], x.shape[1], x.shape[2], _p(phi), mesh[0], mesh[1], mesh[2], _p(out), _p(fld), _stream())
    return (out, fld) if field else out


# ---- non-default samplers ----
def maxpool2_fwd(x):
    n, d, h, w, c = x.shape
    y = torch.empty((n, d // 2, h // 2, w // 2, c), dtype=torch.float32, device=x.device)
    idx = torch.empty((n, d // 2, h // 2, w // 2, c), dtype=torch.uint8, device=x.device)
    lib().call('bts_maxpool2_fwd', _p(x), _p(y), _p(idx), n, d, h, w, c, ld_of(x), c, _stream())
    return y, idx


def maxpool2_bwd(dy, idx, dx, accumulate):
    """dx: [N,D,H,W,C] view of the input's gradient (may be a slab slice)"""
    n, d, h, w, c = dx.shape
    lib().call('bts_maxpool2_bwd', _p(dy), _p(idx), _p(dx), n, d, h, w, c, ld_of(dy), ld_of(dx), 1 if accumulate else 0, _stream())
    return dx


def upsample2_fwd(x, out=None):
    n, d, h, w, c = x.shape
    if out is None:
        out = torch.empty((n, 2 * d, 2 * h, 2 * w, c), dtype=torch.float32, device=x.device)
    lib().call('bts_upsample2_fwd', _p(x), _p(out), n, d, h, w, c, ld_of(x), ld_of(out), _stream())
    return out


def upsample2_bwd(dy, dx=None, accumulate=False):
    n, d2, h2, w2, c = dy.shape
    if dx is None:
        dx = torch.empty((n, d2 // 2, h2 // 2, w2 // 2, c), dtype=torch.float32, device=dy.device)
    lib().call('bts_upsample2_bwd', _p(dy), _p(dx), n, d2 // 2, h2 // 2, w2 // 2, c, ld_of(dy), ld_of(dx),
               1 if accumulate else 0, _stream())
    return dx
