"""FreeSurfer MGH / MGZ volumes: `load_mgh` (mri.jl:1217-1372, without the slice / frame subset) and `save_mgh` (mri.jl:1939-2036).
Pure host code (NumPy).  Files are big-endian: a 284-byte header (seven int32, the int16 ras_good_flag, 15 float32 of geometry, 194
unused bytes), the voxels with x fastest and frames planar, then four float32 MR parameters (tr, flip angle, te, ti).  `.mgz` and
`.mgh.gz` are inflated and deflated in-process (the reference shells out to zcat / gzip), as nifti.py does for `.nii.gz`.

The vox2ras matrix M is built as xform._vox2ras builds its matrices: float64 from the float32 header fields, Pcrs_c = dims / 2,
rounded to float32 once (the reference multiplies in Float32)."""
import gzip
import struct

import numpy as np

MGH_HEADER_BYTES = 284
_UNUSED = 256 - 2 - (3 * 4 + 4 * 3 * 4)                        # UNUSED_SPACE_SIZE - 2 - USED_SPACE_SIZE (mri.jl:1261-1281)
_MGH_DTYPES = {0: np.uint8, 1: np.int32, 3: np.float32, 4: np.int16, 10: np.uint16}     # MRI_UCHAR, MRI_INT, MRI_FLOAT, MRI_SHORT, MRI_USHRT
_MGH_CODES = {np.dtype(v): k for k, v in _MGH_DTYPES.items()}


def _is_gz(fname):
    low = fname.lower()
    return low.endswith(".mgz") or low.endswith(".gz")


def _open(fname, mode):
    return gzip.open(fname, mode) if _is_gz(fname) else open(fname, mode)


def load_mgh(fname, headeronly=False):
    """load_mgh(fname; headeronly) -> (vol, M, mr_parms, volsz): vol [n1, n2, n3, nframes] Fortran-ordered in the file's element type
    (empty with headeronly), M float32 [4, 4] vox2ras, mr_parms float32 [4] (empty when the file ends behind the voxels), volsz the
    four sizes.  ras_good_flag <= 0 is an error ("Loading ... as MGH", mri.jl:634-635); so is an element type other than UCHAR, INT,
    FLOAT, SHORT, USHRT."""
    with _open(fname, "rb") as fh:
        head = fh.read(MGH_HEADER_BYTES)
        if len(head) != MGH_HEADER_BYTES:
            raise ValueError("%s is shorter than an MGH header" % fname)
        _, n1, n2, n3, nframes, typ, _ = struct.unpack(">7i", head[:28])
        (ras_good_flag,) = struct.unpack(">h", head[28:30])
        if ras_good_flag <= 0:
            raise ValueError("Loading " + fname + " as MGH")
        geo = np.frombuffer(head, ">f4", 15, 30).astype(np.float32)
        delta, Mdc, c_ras = geo[:3], geo[3:12].reshape(3, 3).T, geo[12:15]      # (Mdc is stored column by column: x_ras, y_ras, z_ras)
        if typ not in _MGH_DTYPES:
            raise ValueError("MGH data type %d in %s is not supported" % (typ, fname))
        if min(n1, n2, n3, nframes) < 1:
            raise ValueError("%s has non-positive dimensions %s" % (fname, (n1, n2, n3, nframes)))
        dt = np.dtype(_MGH_DTYPES[typ])
        volsz = (n1, n2, n3, nframes)
        MdcD = Mdc.astype(np.float64) * delta.astype(np.float64)                 # Mdc * Diagonal(delta)
        M = np.eye(4)
        M[:3, :3] = MdcD
        M[:3, 3] = c_ras.astype(np.float64) - (MdcD @ np.array([n1, n2, n3], np.float64)) / 2
        M = M.astype(np.float32)
        nv = n1 * n2 * n3 * nframes
        if headeronly:
            vol = np.zeros((0, 0, 0, 0), dt)
            left = nv * dt.itemsize
            while left:                                                          # (a gzip stream cannot seek cheaply: read and drop)
                k = len(fh.read(min(left, 1 << 24)))
                if not k:
                    break
                left -= k
        else:
            raw = fh.read(nv * dt.itemsize)
            if len(raw) != nv * dt.itemsize:
                raise ValueError("%s, read a %s volume but did not reach its end" % (fname, volsz))
            vol = np.frombuffer(raw, dt.newbyteorder(">")).astype(dt).reshape(volsz, order="F")
        tail = fh.read(16)
        mr_parms = np.frombuffer(tail, ">f4").astype(np.float32) if len(tail) == 16 else np.zeros(0, np.float32)
    return vol, M, mr_parms, volsz


def save_mgh(vol, fname, M=None, mr_parms=None):
    """save_mgh(vol, fname, M, mr_parms): vol 3-D or 4-D in one of the five element types, M [4, 4] vox2ras (default: identity),
    mr_parms [4] (default: zeros).  Returns True on error (a byte count that is not the expected one), like the reference."""
    M = np.eye(4) if M is None else np.asarray(M, np.float64)
    mr_parms = np.zeros(4) if mr_parms is None else np.asarray(mr_parms, np.float64).reshape(-1)
    if M.shape != (4, 4):
        raise ValueError("M size=%s, must be (4, 4)" % (M.shape,))
    if mr_parms.size != 4:
        raise ValueError("mr_parms length=%d, must be 4" % mr_parms.size)
    vol = np.asanyarray(vol)
    if vol.ndim == 3:
        vol = vol[..., None]
    if vol.ndim != 4:
        raise ValueError("vol must be 3-D or 4-D")
    if vol.dtype not in _MGH_CODES:
        raise ValueError("Data type %s not supported by MGH files" % vol.dtype)
    n1, n2, n3, nframes = vol.shape
    MdcD = M[:3, :3]
    delta = np.sqrt((MdcD ** 2).sum(axis=0))
    Mdc = MdcD / delta
    c_ras = (M @ np.array([n1 / 2, n2 / 2, n3 / 2, 1.0]))[:3]
    head = (struct.pack(">7i", 1, n1, n2, n3, nframes, _MGH_CODES[vol.dtype], 1) + struct.pack(">h", 1)
            + delta.astype(">f4").tobytes() + Mdc.T.astype(">f4").tobytes() + c_ras.astype(">f4").tobytes() + b"\0" * _UNUSED)
    data = vol.astype(vol.dtype.newbyteorder(">")).tobytes(order="F")
    with _open(fname, "wb") as fh:
        nb = fh.write(head) + fh.write(data) + fh.write(mr_parms.astype(">f4").tobytes())
    return nb != MGH_HEADER_BYTES + vol.size * vol.dtype.itemsize + 16
