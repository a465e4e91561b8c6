"""Minimal single-file NIfTI-1 reader and writer in numpy + gzip (the reference reads its scans with nibabel, test.py:29-37, and
writes mask.nii with it, test.py:69-70).

Supported: `.nii` and `.nii.gz`, either byte order (detected from sizeof_hdr == 348), datatypes uint8, int16, int32, float32,
float64 and uint16, scl_slope / scl_inter (applied when the slope is non-zero).  Everything else -- NIfTI-2, `.hdr/.img` pairs,
complex or RGB types -- raises ValueError naming the offending field.  Offsets are those of the NIfTI-1 specification (nifti1.h).
"""
import gzip
import struct

import numpy as np

_DTYPES = {2: 'u1', 4: 'i2', 8: 'i4', 16: 'f4', 64: 'f8', 512: 'u2'}
_CODES = {np.dtype(v).str[1:]: k for k, v in _DTYPES.items()}
HEADER_BYTES = 348


def _read(path):
    with open(path, 'rb') as f:
        raw = f.read()
    if raw[:2] == b'\x1f\x8b':
        raw = gzip.decompress(raw)
    return raw


def load(path):
    """-> (array in file (Fortran) order, as nibabel's dataobj gives it; header dict with dim, datatype, pixdim (8 floats; [0:4]
    is what the reference averages), scl_slope, scl_inter, qform_code, sform_code, srow_x/y/z and the 4x4 `affine` of the srows)"""
    raw = _read(path)
    if len(raw) < HEADER_BYTES:
        raise ValueError('%s: %d bytes is shorter than a NIfTI-1 header' % (path, len(raw)))
    for end in ('<', '>'):
        if struct.unpack(end + 'i', raw[:4])[0] == HEADER_BYTES:
            break
    else:
        size = struct.unpack('<i', raw[:4])[0]
        if size == 540 or struct.unpack('>i', raw[:4])[0] == 540:
            raise ValueError('%s: sizeof_hdr = 540 is NIfTI-2; only NIfTI-1 (348) is supported' % path)
        raise ValueError('%s: sizeof_hdr = %d is not a NIfTI-1 header (348) in either byte order' % (path, size))
    magic = raw[344:348]
    if magic != b'n+1\x00':
        raise ValueError('%s: magic = %r; only single-file NIfTI-1 (b"n+1\\x00") is supported, not .hdr/.img pairs' % (path, magic))
    dim = struct.unpack(end + '8h', raw[40:56])
    datatype, bitpix = struct.unpack(end + '2h', raw[70:74])
    if datatype not in _DTYPES:
        raise ValueError('%s: datatype = %d is not supported (uint8 2, int16 4, int32 8, float32 16, float64 64, uint16 512)'
                         % (path, datatype))
    if not 1 <= dim[0] <= 7:
        raise ValueError('%s: dim[0] = %d is not a rank between 1 and 7' % (path, dim[0]))
    shape = tuple(int(v) for v in dim[1:1 + dim[0]])
    if min(shape) < 1:
        raise ValueError('%s: dim = %s has a non-positive extent' % (path, list(dim)))
    pixdim = np.array(struct.unpack(end + '8f', raw[76:108]), dtype=np.float32)
    vox_offset, slope, inter = struct.unpack(end + '3f', raw[108:120])
    qform_code, sform_code = struct.unpack(end + '2h', raw[252:256])
    srow = np.array(struct.unpack(end + '12f', raw[280:328]), dtype=np.float32).reshape(3, 4)
    dt = np.dtype(end + _DTYPES[datatype])
    if bitpix != dt.itemsize * 8:
        raise ValueError('%s: bitpix = %d does not match datatype %d' % (path, bitpix, datatype))
    off = int(vox_offset)
    if off < 352:
        raise ValueError('%s: vox_offset = %r lies inside the header' % (path, vox_offset))
    count = int(np.prod(shape))
    if len(raw) < off + count * dt.itemsize:
        raise ValueError('%s: dim = %s needs %d data bytes, the file has %d' % (path, list(dim), count * dt.itemsize, len(raw) - off))
    data = np.frombuffer(raw, dtype=dt, count=count, offset=off).reshape(shape, order='F')
    data = data.astype(dt.newbyteorder('='))
    if slope != 0.0 and not np.isnan(slope) and not (slope == 1.0 and inter == 0.0):
        data = data.astype(np.float64) * np.float64(slope) + np.float64(inter)
    header = {'dim': np.array(dim, dtype=np.int16), 'datatype': int(datatype), 'bitpix': int(bitpix), 'pixdim': pixdim,
              'vox_offset': float(vox_offset), 'scl_slope': float(slope), 'scl_inter': float(inter),
              'qform_code': int(qform_code), 'sform_code': int(sform_code),
              'srow_x': srow[0].copy(), 'srow_y': srow[1].copy(), 'srow_z': srow[2].copy(),
              'affine': np.concatenate([srow, np.array([[0., 0., 0., 1.]], dtype=np.float32)], axis=0)}
    return data, header


def save(path, array, affine):
    """single-file NIfTI-1, little endian, unscaled; gzip-compressed when the name ends in .gz.  The affine goes into srow_x/y/z
    (sform_code 2, aligned), its column norms into pixdim[1:4]."""
    array = np.asarray(array)
    key = array.dtype.newbyteorder('=').str[1:]
    if key not in _CODES:
        raise ValueError('dtype = %s cannot be stored (uint8, int16, int32, float32, float64, uint16)' % array.dtype)
    if not 1 <= array.ndim <= 7:
        raise ValueError('array rank = %d is not between 1 and 7' % array.ndim)
    if max(array.shape) > 32767:
        raise ValueError('shape = %s does not fit the int16 dim field' % (array.shape,))
    affine = np.asarray(affine, dtype=np.float64)
    if affine.shape != (4, 4):
        raise ValueError('affine shape = %s, expected (4, 4)' % (affine.shape,))
    dt = np.dtype('<' + key)
    hdr = bytearray(352)
    struct.pack_into('<i', hdr, 0, HEADER_BYTES)
    dim = [array.ndim] + list(array.shape) + [1] * (7 - array.ndim)
    struct.pack_into('<8h', hdr, 40, *dim)
    struct.pack_into('<2h', hdr, 70, _CODES[key], dt.itemsize * 8)
    pixdim = [1.0] + [float(np.linalg.norm(affine[:3, i])) for i in range(3)] + [1.0] * 4
    struct.pack_into('<8f', hdr, 76, *pixdim)
    struct.pack_into('<3f', hdr, 108, 352.0, 1.0, 0.0)
    hdr[123] = 2                                     # xyzt_units: millimetres
    struct.pack_into('<2h', hdr, 252, 0, 2)
    struct.pack_into('<12f', hdr, 280, *[float(v) for v in affine[:3].reshape(-1)])
    hdr[344:348] = b'n+1\x00'
    blob = bytes(hdr) + np.asarray(array, dtype=dt).tobytes(order='F')
    if str(path).endswith('.gz'):
        with gzip.open(path, 'wb') as f:
            f.write(blob)
    else:
        with open(path, 'wb') as f:
            f.write(blob)
