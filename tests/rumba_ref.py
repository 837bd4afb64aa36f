"""NumPy restatement of rumba_rec (rusd.jl:419-636) in a chosen float type.  Test infrastructure only: the product computes this on
the GPU (fibers.jl_amd/csrc/rumba.hip).

float64 is the reference the HIP path is measured against; the same code run in float32 is the yardstick of how far a legitimate
float32 implementation of a case may drift from it (tests/test_gpu_rumba.py: |gpu - ref64| <= C max|ref32 - ref64| + floor).

Unlike oracle.rumba_rec, the kernel matrix K [ndir, ncomp] is an input (RumbaPlan.kernel(), checked against the oracle to 2e-7), so
a comparison isolates the iteration, and the TV term runs over all compartments at once on [nz, ny, nx, ncomp] arrays.

The algorithm's constants are its own whatever the float type: eps(Float32) (rusd.jl:269, 553), sigma0 = 1/15 (:536), the clamp
(1/80)^2 .. (1/8)^2 (:324), lambda >= (1/30)^2 (:336) and the peak threshold 0.1 (:594), each rounded once to the float type."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
NPEAK = 5                                                                  # rusd.jl:593
FTHRESH = 0.1                                                              # rusd.jl:594
ANG_NEIG = {362: 12.5, 321: 12.5, 181: 16.0}                               # rusd.jl:476-480 (sphere_724 / 642 / 362)


def coil_order(ncoils, coil_combine):
    """n_order (rusd.jl:429-435)"""
    if coil_combine == "SoS-GRAPPA":
        return int(ncoils)
    if coil_combine != "SMF-SENSE":
        raise ValueError("Unknown coil combine mode " + coil_combine)
    return 1


def besseli_ratio(nu, z):
    """besseli_ratio (rusd.jl:170-177) in z's float type.  This is the reference's Perron continued fraction TRUNCATED after its
    fourth level, not the true I_nu(z) / I_{nu-1}(z): the kernel and every restatement keep the truncation."""
    T = z.dtype.type
    a, two = T(2 * nu), T(2)
    with np.errstate(all="ignore"):
        return z / ((a + z) - ((a + T(1)) * z / (two * z + (a + T(1)) - ((a + T(3)) * z / ((a + T(2)) + two * z -
                    ((a + T(5)) * z / ((a + T(3)) + two * z)))))))


def signal_matrix(dwi, mask, bval, dtype):
    """signal_mat [ndir, nmask] and ind_mask (0-based, Fortran voxel order) (rusd.jl:444-464); dwi float32 [nx, ny, nz, nvol]"""
    dwi = np.asarray(dwi, np.float32)
    nvol = dwi.shape[3]
    bval = np.asarray(bval, np.float32)
    ib0 = bval == bval.min()                                               # :449
    ind = np.flatnonzero(np.asarray(mask).reshape(-1, order="F") > 0)      # :446
    vol = np.maximum(dwi.reshape(-1, nvol, order="F")[ind].astype(dtype), dtype(0))   # max.(dwi, 0)
    sig = np.empty((int((~ib0).sum()) + 1, ind.size), dtype)
    sig[0] = vol[:, ib0].mean(axis=1, dtype=dtype)                         # :456-457
    with np.errstate(all="ignore"):
        sig[1:] = vol[:, ~ib0].T / sig[0][None, :]                         # :458-461
    sig[np.isnan(sig)] = 0                                                 # :462
    sig[0] = sig[0] > 0                                                    # :463
    sig[sig > 1] = 1                                                       # :464
    return sig, ind


def _along(a, ax, idx):
    s = [slice(None)] * a.ndim
    s[ax] = idx
    return tuple(s)


def sd_grad(vol, ax):
    """one component of sd_grad! (rusd.jl:183-188): f[[2:end; end]] - f along axis ax (the far face replicated)"""
    n = vol.shape[ax]
    return np.take(vol, np.r_[1:n, n - 1], axis=ax) - vol


def sd_div(G, ax):
    """one axis of sd_div! (rusd.jl:194-207): interior G[i] - G[i-1], first G[1], last -G[end-1].  An axis of length 1 has no
    G[end-1] (the reference throws BoundsError there); the product's rule is the first-row term G[1], which sd_grad makes 0, so a
    singleton axis adds nothing."""
    n = G.shape[ax]
    D = np.empty_like(G)
    if n == 1:
        D[...] = G
        return D
    D[_along(D, ax, slice(1, n - 1))] = G[_along(G, ax, slice(1, n - 1))] - G[_along(G, ax, slice(0, n - 2))]
    D[_along(D, ax, 0)] = G[_along(G, ax, 0)]
    D[_along(D, ax, n - 1)] = -G[_along(G, ax, n - 2)]
    return D


def tv_term(vol, lam):
    """rumba_tv! (rusd.jl:216-235) on vol [nz, ny, nx, ...] (x = axis 2, y = 1, z = 0) with lam broadcastable to it"""
    T = vol.dtype.type
    gx, gy, gz = sd_grad(vol, 2), sd_grad(vol, 1), sd_grad(vol, 0)
    nrm = np.sqrt(((gx * gx + gy * gy) + gz * gz) + T(EPS32))
    gx, gy, gz = gx / nrm, gy / nrm, gz / nrm
    div = (sd_div(gx, 2) + sd_div(gy, 1)) + sd_div(gz, 0)
    return T(1) / (np.abs(T(1) - lam * div) + T(EPS32))


def neighbour_table(vertices):
    """idx_neig (rusd.jl:475-493) as a padded table [nvert, L]; the pad index is nvert"""
    V = np.asarray(vertices, np.float32)
    nvert = V.shape[0] // 2
    H = V[:nvert]
    c = np.clip(H @ H.T, -1, 1)                                            # half_vertices * half_vertices' in Float32
    ang = np.degrees(np.arccos(c.astype(np.float64)))
    ang = np.minimum(ang, 180 - ang)
    isn = ang < ANG_NEIG[nvert]
    np.fill_diagonal(isn, False)
    L = int(isn.sum(1).max())
    tab = np.full((nvert, L), nvert, np.int64)
    for i in range(nvert):
        nb = np.flatnonzero(isn[i])
        tab[i, :nb.size] = nb
    return tab


def rumba_ref(dwi, mask, bval, K, vertices, niter, ncoils=1, coil_combine="SMF-SENSE", ipat_factor=1, use_tv=True,
              dtype=np.float64):
    """rumba_rec (rusd.jl:419-636) with the kernel matrix K given.  Returns the RUMBASD fields as arrays (fodf [nx,ny,nz,nvert], fgm,
    fcsf, gfa, var [nx,ny,nz], peak: five [nx,ny,nz,3], snr_mean, snr_std) and, for tie-aware peak checks, over the masked voxels
    (ind, Fortran voxel order): fodf_mat [ncomp, nmask] (the iterate before the energy preservation), odf [nmask, nvert] (the fODF
    the peaks are taken from), peak_vertex [nmask, 5] (-1: no peak at that rank) and peak_margin [nmask, nvert], the margin by which
    a vertex passes (> 0) or fails (<= 0) the peak test min(f - thr_abs, f - max(neighbours), f)."""
    T = np.dtype(dtype).type
    n_order = coil_order(ncoils, coil_combine)
    if ipat_factor < 1:
        raise ValueError("iPAT factor must be a positive integer")         # :437
    dwi = np.asarray(dwi, np.float32)
    nx, ny, nz = dwi.shape[:3]
    nxyz = nx * ny * nz
    K = np.asarray(K, np.float32).astype(T)
    ndir, ncomp = K.shape
    nvert = ncomp - 2
    sig, ind = signal_matrix(dwi, mask, bval, T)
    assert sig.shape[0] == ndir, "K does not belong to this acquisition"
    nmask = ind.size
    eps = T(EPS32)

    # initial estimates (rusd.jl:529-538, rumba_sd_initialize! :241-259)
    fodf0 = np.full(ncomp, T(1) / T(2 * nvert + 2), T)
    fodf0 = fodf0 / fodf0.sum(dtype=T)
    fodf = np.repeat(fodf0[:, None], nmask, 1)
    dodf = np.repeat((K @ fodf0)[:, None], nmask, 1)
    lam0 = T(1 / 15) * T(1 / 15)
    lam = np.full((nz, ny, nx, 1), lam0, T)                                # the volume W.lambda, [z, y, x] + a compartment axis
    lamf = lam.reshape(-1)                                                 # (a view: flat index = Fortran voxel index)
    s2 = np.full(nmask, lam0, T)
    with np.errstate(all="ignore"):
        dsig = (sig * dodf) / s2[None, :]
    tv = np.ones((ncomp, nmask), T)
    snr = np.zeros(nmask, T)
    vol = np.zeros((nxyz, ncomp), T) if use_tv else None
    with np.errstate(all="ignore"):
        for _ in range(niter):                                             # rumba_sd_iterate! (:266-345)
            ir = besseli_ratio(n_order, dsig)                              # :275
            rl = K.T @ (sig * ir)                                          # :277
            rl2 = K.T @ dodf + eps                                         # :278-279
            rl = rl / rl2
            if use_tv:                                                     # :282-296, every compartment at once
                vol[ind] = fodf.T
                tv = tv_term(vol.reshape(nz, ny, nx, ncomp), lam).reshape(nxyz, ncomp)[ind].T
            fodf = np.maximum(fodf * rl * tv, T(0))                        # :301 (NaN stays NaN)
            dodf = K @ fodf                                                # :313
            dsig = (sig * dodf) / s2[None, :]                              # :314
            ir = (sig * sig + dodf * dodf) / T(2) - (s2[None, :] * dsig) * ir   # :317-318
            s2 = ir.sum(axis=0, dtype=T) / T(n_order * ndir)               # :319
            s2 = np.clip(s2, T((1 / 80) ** 2), T((1 / 8) ** 2))            # :324
            snr = T(1) / np.sqrt(s2)                                       # :326
            if use_tv:
                if ipat_factor == 1:                                       # :333-336
                    lam[...] = np.maximum(s2.mean(dtype=T), T((1 / 30) ** 2))
                else:                                                      # :337-343
                    lam[...] = 0
                    lamf[ind] = s2
    # mean / corrected std of the SNR (rusd.jl:540-547; 0 without iterations).  One masked voxel: Julia's corrected std is 0/0 = NaN;
    # the product (and the oracle) return 0
    snr64 = snr.astype(np.float64)
    snr_mean = float(snr64.mean()) if niter > 0 and nmask else 0.0
    snr_std = float(np.sqrt(((snr64 - snr_mean) ** 2).sum() / (nmask - 1))) if niter > 0 and nmask > 1 else 0.0
    fodf_mat = fodf

    # post-processing (rusd.jl:549-590)
    with np.errstate(all="ignore"):
        f = fodf / (fodf.sum(axis=0, dtype=T) + eps)                       # :553
    out = np.zeros((nxyz, nvert), T)
    out[ind] = f[:nvert].T                                                 # :566-568
    fcsf = np.zeros(nxyz, T); fcsf[ind] = f[nvert]                         # :571
    fgm = np.zeros(nxyz, T); fgm[ind] = f[nvert + 1]                       # :574
    fiso = fgm + fcsf                                                      # :576
    out = out + fiso[:, None]                                              # :579
    with np.errstate(all="ignore"):
        out = out / out.sum(axis=1, dtype=T, keepdims=True)                # :581
    out[np.isnan(out)] = 0                                                 # :582
    var = np.zeros(nxyz, T); var[ind] = s2                                 # :585
    with np.errstate(all="ignore"):
        gfa = out.std(axis=1, ddof=1, dtype=T) / np.sqrt((out * out).mean(axis=1, dtype=T))   # :589
    gfa[np.isnan(gfa)] = 0                                                 # :590

    # peak extraction (rumba_peaks! :348-373, rusd.jl:595-631), over the masked voxels in blocks
    H = np.asarray(vertices, np.float32)[:nvert].astype(T)
    tab = neighbour_table(vertices)
    peaks = np.zeros((NPEAK, nxyz, 3), T)
    odf = out[ind]
    pvert = np.full((nmask, NPEAK), -1, np.int64)
    margin = np.empty((nmask, nvert), T)
    for b0 in range(0, nmask, 2048):
        o = odf[b0:b0 + 2048]
        fi = fiso[ind[b0:b0 + 2048]]
        with np.errstate(all="ignore"):
            thr_abs = (T(FTHRESH) / (T(1) - fi)) * o.max(axis=1)           # :358, 364
            opad = np.concatenate([o, np.full((o.shape[0], 1), -np.inf, T)], 1)
            nmax = opad[:, tab].max(axis=2)                                # maximum(fodf[idx_neig[ivert]])
            keep = ~((o < thr_abs[:, None]) | (o <= nmax))                 # :367-371
            pk = np.where(keep, o, T(0))
            margin[b0:b0 + 2048] = np.minimum(np.minimum(o - thr_abs[:, None], o - nmax), o)
        isort = np.argsort(-pk, axis=1, kind="stable")[:, :NPEAK]          # sortperm!(..., rev=true): stable, ties -> lower index
        n = np.minimum((pk > 0).sum(axis=1), NPEAK)                        # :373, 609
        live = np.arange(NPEAK)[None, :] < n[:, None]
        amp = np.take_along_axis(o, isort, 1)
        with np.errstate(all="ignore"):
            ssum = np.zeros(o.shape[0], T)
            for k in range(NPEAK):                                         # sum(fodf[isort[1:n]]) in rank order
                ssum = ssum + np.where(live[:, k], amp[:, k], T(0))
            fnorm = (T(1) - fi) / ssum                                     # :611-612
        for k in range(NPEAK):                                             # :614-618
            sel = live[:, k]
            v = ind[b0:b0 + 2048][sel]
            peaks[k, v] = H[isort[sel, k]] * (amp[sel, k] * fnorm[sel])[:, None]
        pvert[b0:b0 + 2048] = np.where(live, isort, -1)

    shp = (nx, ny, nz)
    return dict(fodf=out.reshape(shp + (nvert,), order="F"), fgm=fgm.reshape(shp, order="F"), fcsf=fcsf.reshape(shp, order="F"),
                gfa=gfa.reshape(shp, order="F"), var=var.reshape(shp, order="F"),
                peak=[peaks[k].reshape(shp + (3,), order="F") for k in range(NPEAK)], snr_mean=snr_mean, snr_std=snr_std,
                ind=ind, fodf_mat=fodf_mat, odf=odf, peak_vertex=pvert, peak_margin=margin)
