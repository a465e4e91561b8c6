"""Minimal single-file NIfTI-1 reader and writer in numpy + gzip (the reference reads its scans with nibabel, test.py:29-37, and
writes mask.nii with it, test.py:69-70).

Supported: `.nii` and `.nii.gz`, either byte order (detected from sizeof_hdr == 348), datatypes uint8, int16, int32, float32,
float64 and uint16, scl_slope / scl_inter (applied when the slope is non-zero).  Everything else -- NIfTI-2, `.hdr/.img` pairs,
complex or RGB types -- raises ValueError naming the offending field.  Offsets are those of the NIfTI-1 specification (nifti1.h).

Geometry (host, float64; world is NIfTI's RAS+): `qform_affine` is nifti1.h's quaternion formula, `best_affine` the sform where
sform_code > 0, else the qform where qform_code > 0, else an error: an unknown orientation is not guessed.  `orientation` names the
closest axis code of an affine ('LPS': the array axes increase toward Left, Posterior, Superior, as BraTS stores its arrays),
`reorientation` the axis permutation and flips between two codes.
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
    is what the reference averages), scl_slope, scl_inter, qform_code, sform_code, srow_x/y/z, the 4x4 `affine` of the srows, and the
    qform's fields: quatern (b, c, d), qoffset (x, y, z), qfac (-1 where pixdim[0] == -1, else 1))"""
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
    quatern = np.array(struct.unpack(end + '3f', raw[256:268]), dtype=np.float32)
    qoffset = np.array(struct.unpack(end + '3f', raw[268:280]), dtype=np.float32)
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
              'affine': np.concatenate([srow, np.array([[0., 0., 0., 1.]], dtype=np.float32)], axis=0),
              'quatern': quatern, 'qoffset': qoffset, 'qfac': -1.0 if pixdim[0] == -1.0 else 1.0}
    return data, header


def qform_affine(header):
    """the 4x4 float64 affine of the qform fields (nifti1.h, "METHOD 2"): a = sqrt(max(0, 1 - b^2 - c^2 - d^2)), the rotation of the unit
    quaternion (a, b, c, d) with its columns scaled by pixdim[1], pixdim[2], qfac * pixdim[3], the translation qoffset"""
    b, c, d = (float(v) for v in header['quatern'])
    a = float(np.sqrt(max(0.0, 1.0 - b * b - c * c - d * d)))
    rot = np.array([[a * a + b * b - c * c - d * d, 2.0 * (b * c - a * d), 2.0 * (b * d + a * c)],
                    [2.0 * (b * c + a * d), a * a + c * c - b * b - d * d, 2.0 * (c * d - a * b)],
                    [2.0 * (b * d - a * c), 2.0 * (c * d + a * b), a * a + d * d - b * b - c * c]], dtype=np.float64)
    pix = np.asarray(header['pixdim'], dtype=np.float64)
    out = np.eye(4, dtype=np.float64)
    out[:3, :3] = rot * np.array([pix[1], pix[2], float(header['qfac']) * pix[3]])
    out[:3, 3] = np.asarray(header['qoffset'], dtype=np.float64)
    return out


def best_affine(header):
    """the affine a reader should use, float64: the srows where sform_code > 0, else the qform affine where qform_code > 0; a header
    with neither says nothing about the orientation, which is not guessed: ValueError naming the codes"""
    if int(header['sform_code']) > 0:
        return np.asarray(header['affine'], dtype=np.float64).copy()
    if int(header['qform_code']) > 0:
        return qform_affine(header)
    raise ValueError('sform_code = %d and qform_code = %d: the header gives no orientation, and none is assumed'
                     % (int(header['sform_code']), int(header['qform_code'])))


_LETTERS = (('L', 'R'), ('P', 'A'), ('I', 'S'))          # world row 0, 1, 2 of RAS+: the letter toward - and toward +


def orientation(affine):
    """three-letter axis code of a 4x4 (or 3x3) affine: letter j says toward which side array axis j increases.  The columns of the
    3x3 part are normalised; three times the largest |entry| among the world rows and array columns not yet assigned is taken (ties:
    lowest column, then lowest row) and its sign picks the letter.  A zero or non-finite column or a (near-)singular matrix: ValueError"""
    r = np.asarray(affine, dtype=np.float64)[:3, :3].copy()
    norms = np.sqrt((r * r).sum(axis=0))
    if not np.all(np.isfinite(r)) or not np.all(norms > 0):
        raise ValueError('orientation: the affine has a zero or non-finite column: %s' % (r.tolist(),))
    r /= norms
    if not abs(np.linalg.det(r)) >= 1e-6:
        raise ValueError('orientation: the affine is singular (|det| of the normalised columns %.3g)' % abs(np.linalg.det(r)))
    code, rows, cols = [None] * 3, [0, 1, 2], [0, 1, 2]
    for _ in range(3):
        best = None
        for j in cols:
            for w in rows:
                if best is None or abs(r[w, j]) > abs(r[best[0], best[1]]):
                    best = (w, j)
        w, j = best
        code[j] = _LETTERS[w][1 if r[w, j] > 0 else 0]
        rows.remove(w)
        cols.remove(j)
    return ''.join(code)


def _code_axes(code):
    """'LPS' -> [(world axis, +1 | -1) per letter]; anything but one letter from each of R/L, A/P, S/I: ValueError"""
    out = []
    for ch in str(code):
        hit = [(w, 1 if pair[1] == ch else -1) for w, pair in enumerate(_LETTERS) if ch in pair]
        if not hit:
            break
        out.append(hit[0])
    if len(str(code)) != 3 or len(out) != 3 or sorted(w for w, _ in out) != [0, 1, 2]:
        raise ValueError('%r is not an orientation code: one letter from each of R/L, A/P, S/I in any order' % (code,))
    return out


def reorientation(src_code, dst_code):
    """-> (perm, flip): output axis a of an array in `dst_code` runs along axis perm[a] of the array in `src_code`, reversed where
    flip[a]: dst = np.flip(np.transpose(src, perm), [a for a in range(3) if flip[a]])"""
    src, dst = _code_axes(src_code), _code_axes(dst_code)
    perm, flip = [], []
    for w, sign in dst:
        j = [k for k, (ws, _) in enumerate(src) if ws == w][0]
        perm.append(j)
        flip.append(src[j][1] != sign)
    return tuple(perm), tuple(flip)


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
