"""Optional live kernel timing (bench.py roofline): the library records HIP events on the launch stream around its launches (bts_profile_*),
i.e. the same per-launch durations rocprofv3 reports; and the names of what it records."""
import ctypes

from . import _core


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
    _core.lib().call('bts_profile_enable', 1 if on else 0)


def profile_records(detail=False):
    """-> [(symbol, algorithmic_flops, ms)] ; synchronise the device first.  detail: kernel variants in the symbol names"""
    L = _core.lib()
    out = []
    sym, fl, ms = ctypes.c_int(), ctypes.c_double(), ctypes.c_float()
    for i in range(L._bts_profile_count()):
        L.call('bts_profile_get', i, ctypes.byref(sym), ctypes.byref(fl), ctypes.byref(ms))
        out.append((kernel_symbol(sym.value, detail), fl.value, ms.value))
    return out


def conv_flops(kind, n, d, h, w, cin, cout):
    """algorithmic FLOPs of one conv call, SURVEY 8(d) convention (MAC = 2; (d,h,w) = forward INPUT dims)"""
    v = n * d * h * w
    if kind == _core.K1:
        return 2.0 * cin * cout * v
    if kind == _core.K3S2:
        return 2.0 * 27 * cin * cout * (v // 8)
    return 2.0 * 27 * cin * cout * v   # K3S1; K3S2T counts 27*Cin*Cout*V_in MACs
