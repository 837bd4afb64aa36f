/*
 * fibers_hip.h — C ABI of libfibers_hip.so, the MI355X (gfx950) back end for the
 * Fibers.jl per-voxel reconstruction + streamline hot path.
 *
 * The reference (lincbrain/Fibers.jl) has no FFI: its boundary is the exported Julia
 * function surface plus the MRI / Tract field layouts.  Each entry point below names the
 * reference function (file:line under the reference's src/) whose body it replaces; the
 * Julia `ccall` stubs a maintainer would add are in INTEGRATION.md.
 *
 * Conventions
 *   - All volumes are float32, Julia column-major [nx,ny,nz,nframes] exactly as
 *     `MRI.vol` (mri.jl:81): x fastest, frame slowest ("planar").  nvox = nx*ny*nz.
 *   - bvec is [nvol x 3] column-major like `MRI.bvec` (mri.jl:129).
 *   - Streamline coordinates are float32, 1-based voxel coordinates exactly as
 *     `pos_now` in stream.jl:660.
 *   - Every function returns FIB_OK (0) or a negative fib_status; the message is
 *     available from fib_last_error() (thread-local).  No C++ exception and no abort()
 *     crosses this boundary.  There is NO CPU fallback: without a usable HIP device
 *     every compute entry point fails with FIB_ERR_NO_DEVICE.
 *   - fib_*  : host-buffer ("drop-in") entry points; blocking; buffers are caller-owned
 *              host memory (Julia arrays under GC.@preserve); nothing is retained.
 *   - fibd_* : device-resident entry points (pointers are HIP device pointers, `stream`
 *              is a hipStream_t passed as void*, may be NULL); asynchronous on `stream`
 *              unless stated.  Used by the multi-GPU host layer and by bench.py.
 */
#ifndef FIBERS_HIP_H
#define FIBERS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    FIB_OK = 0,
    FIB_ERR_INVALID = -1,       /* bad argument (NULL pointer, non-positive size, ...) */
    FIB_ERR_NO_DEVICE = -2,     /* no HIP device / device index out of range */
    FIB_ERR_HIP = -3,           /* a HIP runtime call failed; see fib_last_error() */
    FIB_ERR_MISSING_BVAL = -4,  /* "Missing b-value table from input DWI structure"  (dti.jl:167,224 gqi.jl:112 dsi.jl:174) */
    FIB_ERR_MISSING_BVEC = -5,  /* "Missing gradient table from input DWI structure" (dti.jl:228 gqi.jl:116 dsi.jl:178) */
    FIB_ERR_DIM_MISMATCH = -6,  /* "Dimension mismatch between seed mask ... and brain mask ..." (stream.jl:746-749) */
    FIB_ERR_UNSUPPORTED = -7,   /* e.g. q-space grid other than 16^3, ODF vertex degree too large */
    FIB_ERR_NOMEM = -8,
    FIB_ERR_CAPACITY = -9       /* caller-provided output buffers too small (fibd_stream_run): the counts say what is needed */
} fib_status;

/* element type of a mask / seed volume handed over by the host (any numeric array in Julia) */
typedef enum {
    FIB_U8 = 0, FIB_I8 = 1, FIB_I16 = 2, FIB_U16 = 3, FIB_I32 = 4, FIB_U32 = 5,
    FIB_F32 = 6, FIB_F64 = 7, FIB_I64 = 8, FIB_BOOL = 9
} fib_dtype;

const char *fib_last_error(void);
const char *fib_version(void);
int fib_device_count(void);                 /* number of visible HIP devices (0 if none) */

/* ------------------------------------------------------------------------------------ */
/* Measurement hooks (bench.py): per-kernel HIP-event timing on the launch stream         */
/* ------------------------------------------------------------------------------------ */
/* When enabled, every hot-path kernel launch is bracketed by a hipEvent pair recorded on the
 * stream it is launched on.  fib_profile_get synchronises the pending events of `kernel`
 * ("dti_fit", "odf_gemm", "odf_peaks", "qa_normalize", "stream_trace", "stream_pack", ...) and
 * returns the accumulated device time and launch count since the last fib_profile_reset.
 * fib_profile_filter("odf_gemm,dti_fit"): only the named kernels are bracketed (NULL or "": all of them) -- an event pair is two packets in
 * the queue, and a measurement of one kernel inside a timed region should not pay for the others' brackets. */
int fib_profile_enable(int on);
int fib_profile_filter(const char *names);
int fib_profile_reset(void);
int fib_profile_get(const char *kernel, double *total_ms, int64_t *count);

/* ------------------------------------------------------------------------------------ */
/* Plans = the reference's pre-computed work structs, resident on one device             */
/* ------------------------------------------------------------------------------------ */
/* A plan also owns the scratch of the calls made on it (voxel lists, counters, work arrays: the reference's per-thread
 * work structs): use one plan per concurrent call / stream; plans themselves are independent of each other. */
typedef struct fib_dti_plan fib_dti_plan;   /* DTIwork / ADCwork  (dti.jl:39-84, 101-155) */
typedef struct fib_odf_plan fib_odf_plan;   /* GQIwork (gqi.jl:32-82) or DSIwork (dsi.jl:41-143) */

/* DTIwork(bval, bvec) (dti.jl:110): design matrix A[nvol x 7] and pA = pinv(A); with
 * bvec == NULL builds ADCwork(bval) (dti.jl:48): A = [-b, 1].  Host tables in, device plan out. */
int fib_dti_plan_create(int device, const float *bval, const float *bvec, int nvol, fib_dti_plan **plan);
void fib_dti_plan_destroy(fib_dti_plan *plan);
/* copies of the host-side tables for inspection/tests: A [nvol x np] and pA [np x nvol], column-major */
int fib_dti_plan_tables(const fib_dti_plan *plan, float *A, float *pA, int *np);

/* GQIwork(bval, bvec, odf_dirs, sigma) (gqi.jl:42): A = sinc.(V[nvert+1:end,:] * bq') and the
 * folded face table.  verts [nverts x 3] column-major, faces [nfaces x 3] column-major, 1-based. */
int fib_gqi_plan_create(int device, const float *bval, const float *bvec, int nvol,
                        const float *verts, int nverts, const int32_t *faces, int nfaces,
                        float sigma, fib_odf_plan **plan);
/* DSIwork(bval, bvec, odf_dirs, hann_width) (dsi.jl:59).  The per-voxel chain
 * scatter -> Hanning -> centred 16^3 FFT -> Re -> radial trilinear integration (dsi.jl:204-242)
 * is linear in the clamped signal up to the 1/sum(p) scalar, so the plan holds it as two dense
 * maps: pdf = C[nvol x nvol] s / sum(p), odf = M[nvert x nvol] s / sum(p). */
int fib_dsi_plan_create(int device, const float *bval, const float *bvec, int nvol,
                        const float *verts, int nverts, const int32_t *faces, int nfaces,
                        int hann_width, fib_odf_plan **plan);
/* The same with the operand format of the contraction A*s chosen per plan.  The reference runs an f32 sgemv (gqi.jl:144);
 * the kernels run it on the matrix cores in one of three forms, all f32 in / f32 accumulate / f32 out:
 *   FIB_ODF_FORMAT_FP16X2  two fp16 pieces per f32 operand (23 of 24 significant bits, three piece products; the default)
 *   FIB_ODF_FORMAT_BF16X3  three bf16 pieces per operand, six piece products: every f32 product exact
 *   FIB_ODF_FORMAT_F32     v_mfma_f32_32x32x2_f32: a k-ordered f32 fma chain
 *   FIB_ODF_FORMAT_DEFAULT what the environment selects (FIBERS_ODF_FORMAT = fp16x2 | bf16x3 | f32), else FP16X2.
 * A plan may fall back to a wider form when its matrix does not fit a narrower one (non-finite entries, < 2 stages):
 * fib_odf_plan_format reports what the plan's kernels actually run; fib_odf_default_format what DEFAULT resolves to now. */
#define FIB_ODF_FORMAT_DEFAULT 0
#define FIB_ODF_FORMAT_FP16X2 1
#define FIB_ODF_FORMAT_BF16X3 2
#define FIB_ODF_FORMAT_F32 3
int fib_gqi_plan_create_fmt(int device, const float *bval, const float *bvec, int nvol,
                            const float *verts, int nverts, const int32_t *faces, int nfaces,
                            float sigma, int format, fib_odf_plan **plan);
int fib_dsi_plan_create_fmt(int device, const float *bval, const float *bvec, int nvol,
                            const float *verts, int nverts, const int32_t *faces, int nfaces,
                            int hann_width, int format, fib_odf_plan **plan);
int fib_odf_plan_format(const fib_odf_plan *plan);   /* FIB_ODF_FORMAT_* (> 0) or a negative error code */
/* Diagnostic: the unit of the voxel list the plan's next fibd_odf_rec call will use -- 1: aligned groups of 32 voxels (a wave's
 * 128-byte row segments are whole cache lines whatever the mask's runs look like; the default), 0: aligned groups of 4 (chosen by
 * the previous call when groups of 32 would list more than 1.5 x the voxels: sparse masks).  Results do not depend on it.
 * Waits for `stream`. */
int fib_odf_plan_list_unit(const fib_odf_plan *plan, void *stream);
int fib_odf_default_format(void);
void fib_odf_plan_destroy(fib_odf_plan *plan);
/* host copy of the reconstruction matrix [nrows x nvol] column-major (GQI: nrows = nvert;
 * DSI: nrows = nvol + nvert, pdf rows first); pass NULL to query sizes only. */
int fib_odf_plan_matrix(const fib_odf_plan *plan, float *A, int *nrows, int *nvol, int *nvert);

/* ------------------------------------------------------------------------------------ */
/* Device-resident hot path                                                              */
/* ------------------------------------------------------------------------------------ */

/* 10 output volumes of dti_fit_ls (dti.jl:247-256): scalars [nvox], eigvecs [nvox*3] planar */
typedef struct {
    float *s0, *eigval1, *eigval2, *eigval3;
    float *eigvec1, *eigvec2, *eigvec3;
    float *rd, *md, *fa;
} fib_dti_out;

/* dti_fit_ls(dwi::MRI, mask::MRI) volume loop (dti.jl:258-275) + per-voxel fit (dti.jl:286-316)
 * + dti_maps (dti.jl:325-335).  mask: uint8 [nvox], non-zero = fit (dti.jl:261).  All outputs are
 * fully written (zeros where the reference leaves its zero-initialised volumes untouched). */
int fibd_dti_fit(const fib_dti_plan *plan, const float *dwi, const uint8_t *mask, int64_t nvox,
                 const fib_dti_out *out, void *stream);
/* adc_fit (dti.jl:164-213) */
int fibd_adc_fit(const fib_dti_plan *plan, const float *dwi, const uint8_t *mask, int64_t nvox,
                 float *adc, float *s0, void *stream);
/* st_eigen (structens.jl:13-37): eigen(Symmetric(S, :L)) per voxel with the diffusion tensor's 3x3 solver.
 * S = {Sxx, Sxy, Sxz, Syy, Syz, Szz}, each [nvox]; eigval [nvox*3] ascending (eigval[ix,iy,iz,k]);
 * eigvec [nvox*9], component i of eigenvector j at (i + 3*j)*nvox + vox (eigvec[ix,iy,iz,i,j]). */
int fibd_st_eigen(const float *const S[6], int64_t nvox, float *eigvec, float *eigval, void *stream);
/* st_recon (structens.jl:40-88): G_sigma smoothing (skipped when sigma <= 0), Scharr gradients, the six products, G_rho smoothing
 * (skipped when rho <= 0), eigen(Symmetric(S, :L)); every filter is imfilter(..., "reflect").  Radii 2*ceil(sigma) and
 * 2*ceil(rho) up to 16 (sigma, rho <= 8); larger ones are FIB_ERR_UNSUPPORTED.
 * vol: planes [zin0, zin0 + nzin) of an nx*ny*nz float volume, x fastest.  Writes output planes [z0, z1); vol must hold
 * [max(0, z0-H), min(nz, z1+H)) with H = fib_st_recon_halo(sigma, rho) (reflection is taken against the whole volume).
 * eigvec [9][nvox_out], eigval [3][nvox_out] in fibd_st_eigen's layout, nvox_out = nx*ny*(z1-z0).  S_out: NULL, or six [nvox_out]
 * volumes that receive the smoothed tensor (Sxx Sxy Sxz Syy Syz Szz) that was decomposed.  work: device scratch of at least
 * fibd_st_recon_work_size(nx, ny, z1 - z0, ...) bytes (the gradients). */
int fib_st_recon_halo(float sigma, float rho, int *halo);
int fibd_st_recon_work_size(int nx, int ny, int nz_out, float sigma, float rho, size_t *bytes);
int fibd_st_recon(const float *vol, int nx, int ny, int nz, int zin0, int nzin, int z0, int z1, float sigma, float rho,
                  float *eigvec, float *eigval, float *const *S_out, void *work, size_t work_bytes, void *stream);
/* number of voxels the last fibd_dti_fit/fibd_adc_fit call on this plan sent through the
 * per-voxel pinv branch (dti.jl:297-298, 206-207); synchronises `stream`. */
int fibd_dti_last_partial_count(const fib_dti_plan *plan, void *stream, int64_t *count);

/* ---- diffusion kurtosis imaging (not in the reference; definition in DESIGN.md §5) ----
 * ln S = ln S0 - b g'Dg + (b^2 / 6) sum g_i g_j g_k g_l V_ijkl with V = MD^2 W.  22 unknowns per voxel: d[0..5] = Dxx Dxy Dxz Dyy Dyz Dzz,
 * d[6..20] = V in the monomial order xxxx yyyy zzzz xxxy xxxz xyyy yyyz xzzz yzzz xxyy xxzz yyzz xxyz xyyz xyzz, d[21] = ln S0. */
typedef struct fib_dki_plan fib_dki_plan;
typedef struct {
    float min_signal;        /* samples are clamped to this from below before the logarithm (1e-4) */
    float min_diffusivity;   /* floor of D(n) in K(n) = V(n) / D(n)^2 (1e-6) */
    float min_kurtosis;      /* K(n) is clipped to [min_kurtosis, max_kurtosis] (-3/7, 10); no clip when min >= max */
    float max_kurtosis;
} fib_dki_params;
/* the ten volumes of fib_dti_out, then mean / axial / radial kurtosis [nvox] and the kurtosis tensor W [15][nvox] (NULL: not written) */
typedef struct {
    float *s0, *eigval1, *eigval2, *eigval3;
    float *eigvec1, *eigvec2, *eigvec3;
    float *rd, *md, *fa;
    float *mk, *ak, *rk, *kt;
} fib_dki_out;
/* Host only (no device needed): the design A [nvol x 22] with b in ms/um^2 and pA [22 x nvol] = pinv(A) with rows 0-5 scaled by 1e-3 and
 * rows 6-20 by 1e-6, so that d = pA log(s) is in mm^2/s and mm^4/s^2; both built in float64 and rounded once, column-major; A, pA may be
 * NULL.  *rank: the rank of A under pinv's cut-off sigma > eps(Float32) * min(m, n) * sigma_max.  A rank below 22 is FIB_ERR_INVALID
 * (DKI needs a b ~ 0 frame and two non-zero shells); the tables and *rank are filled all the same. */
int fib_dki_design(const float *bval, const float *bvec, int nvol, float *A, float *pA, int *rank);
/* verts [nverts x 3] column-major: mk is the mean of K(n) over rows 0 .. nverts/2 - 1.  params NULL: the defaults. */
int fib_dki_plan_create(int device, const float *bval, const float *bvec, int nvol, const float *verts, int nverts,
                        const fib_dki_params *params, fib_dki_plan **plan);
void fib_dki_plan_destroy(fib_dki_plan *plan);
/* host copies: A, pA as fib_dki_design's; dirs [nverts/2][21] row-major, the 6 quadratic (off-diagonals doubled) and 15
 * multiplicity-weighted quartic monomials of every direction of mk.  Any of them may be NULL. */
int fib_dki_plan_tables(const fib_dki_plan *plan, float *A, float *pA, float *dirs);
/* dwi [nvol][nvox] planar, mask uint8 [nvox].  Every output is written in every voxel: zeros outside the mask and where max(s) <= 0 or a
 * sample is NaN; elsewhere d = pA log(max(s, min_signal)) (no row-subset fit: the clamp is the rule for non-positive samples). */
int fibd_dki_fit(const fib_dki_plan *plan, const float *dwi, const uint8_t *mask, int64_t nvox,
                 const fib_dki_out *out, void *stream);

/* ---- Constrained spherical deconvolution (not in the reference; this section and DESIGN.md §5 are the definition) ----
 * Basis: real, even-order spherical harmonics up to lmax in {2, 4, 6, 8}: n = (lmax + 1)(lmax + 2) / 2 = 6, 15, 28, 45 columns, column
 *   l (l + 1) / 2 + m.  Y_lm = N_l^|m| P_l^|m|(cos theta) {sqrt 2 cos(m phi), m > 0; 1, m = 0; sqrt 2 sin(|m| phi), m < 0},
 *   N = sqrt((2l + 1) / (4 pi) (l - |m|)! / (l + |m|)!), P with the Condon-Shortley phase, theta from +z, phi = atan2(y, x).
 * Shell: frames with b <= b0_thresh are b0 frames and are not read.  shell <= 0 means the largest b; the shell frames are those with
 *   b > b0_thresh and |b - shell| <= b_tol shell, nshell of them in frame order.  nshell < n is FIB_ERR_INVALID, and so is a kernel matrix
 *   X whose rank (fib_dki_design's rule: singular values > eps(Float32) min(m, n) sigma_max, on the float64 matrix) is below n.
 * Response: a prolate tensor (lambda_para, lambda_perp) and s0.  R_l = sqrt(4 pi / (2l + 1)) 2 pi int_-1^1 s0 exp(-bbar (lambda_perp +
 *   (lambda_para - lambda_perp) t^2)) Y_l0(t) dt by 64-point Gauss-Legendre quadrature in float64; bbar = the mean b of the shell frames.
 * Tables, built in float64 and rounded once to float32:
 *   X [nshell x n] = Y(shell bvecs) diag(R_l);  Y [nreg x n] = the basis at the first-half vertices (nreg = nverts / 2);
 *   B [nreg x n] = Y lambda R_0 nshell / nreg (at 362 directions the scaling of Tournier 2007).
 * Per voxel (skipped, all outputs 0, when the mask is 0 or no shell sample is > 0), with s the shell samples:
 *   f = the least-squares solution on the first min(n, 15) columns of X, the other coefficients 0;  thr = tau B[0,0] f[0];
 *   repeat up to niter times:  a = B f;  set = {i : a_i < thr};  from the second pass on, stop if the set equals the previous one;
 *     solve (X'X + sum_{i in set} b_i b_i') f = X's by Cholesky  (b_i = row i of B; the first pass always solves).
 *   sh = f;  odf = max(Y f, 0);  niter = the number of solves;  peak[k], f[k] = vertex and odf amplitude of the k-th peak of find_peaks!
 *   on odf (fibd_find_peaks on the tessellation's faces), zeros beyond the number of peaks.
 * Arithmetic: float64 from the float32 samples and tables on (X's, a, the matrix, its factor, the solves, Y f); outputs are rounded to
 *   float32 once.  This is a matter of correctness: membership in the set is discontinuous, one direction changing sides changes the
 *   matrix by a whole b b', and amplitudes come within 1e-5 of thr (relative) in a few hundred voxels -- float32 sums deviate by 3e-6. */
typedef struct fib_csd_plan fib_csd_plan;
typedef struct {
    int lmax;                /* 2, 4, 6 or 8 */
    float lambda_para;       /* the response: eigenvalues of the prolate tensor (mm^2/s) and its b = 0 signal */
    float lambda_perp;
    float s0;
    float b0_thresh;         /* 50 */
    float shell;             /* <= 0: the largest b */
    float b_tol;             /* 0.05 */
    float lambda;            /* weight of the constraint rows (1) */
    float tau;               /* threshold as a fraction of the initial mean amplitude (0.1) */
    int niter;               /* most solves per voxel (50) */
} fib_csd_params;
/* sh [n][nvox], odf [nreg][nvox], niter [nvox] (a count, stored as float32 like every volume), peak[k] [3][nvox], f[k] [nvox] */
typedef struct {
    float *sh, *odf, *niter;
    float *peak[3];
    float *f[3];
} fib_csd_out;
/* Host only (no device needed).  frames [nvol] receives the nshell shell frames (0-based), R [lmax / 2 + 1], X [nshell x n], B and Y
 * [nreg x n] column-major; any of them may be NULL (size X for nvol rows when nshell is not known).  The frame list and *nshell are filled
 * even when the scheme is refused, *rank and the tables whenever nshell >= n.  verts [nverts x 3] column-major. */
int fib_csd_design(const float *bval, const float *bvec, int nvol, const float *verts, int nverts, const fib_csd_params *params,
                   int32_t *frames, int *nshell, float *R, float *X, float *B, float *Y, int *rank);
/* faces [nfaces x 3] column-major, 1-based: the peak finder's neighbour table.  Shells of more than 256 frames and tessellations of more
 * than 384 directions are FIB_ERR_UNSUPPORTED. */
int fib_csd_plan_create(int device, const float *bval, const float *bvec, int nvol, const float *verts, int nverts,
                        const int32_t *faces, int nfaces, const fib_csd_params *params, fib_csd_plan **plan);
void fib_csd_plan_destroy(fib_csd_plan *plan);
/* host copies of the plan's tables, as fib_csd_design returns them; any pointer may be NULL */
int fib_csd_plan_tables(const fib_csd_plan *plan, int32_t *frames, int *nshell, float *R, float *X, float *B, float *Y);
/* dwi [nvol][nvox] planar (every frame of the scheme; the kernel reads the shell's), mask uint8 [nvox].  Every output is written in every
 * voxel.  The plan holds the peak finder's scratch of the call: one call at a time per plan. */
int fibd_csd_rec(const fib_csd_plan *plan, const float *dwi, const uint8_t *mask, int64_t nvox, const fib_csd_out *out, void *stream);

/* ---- Multi-shell multi-tissue deconvolution (not in the reference; this section and DESIGN.md §5 are the definition) ----
 * After Jeurissen et al. 2014: the signal of ALL shells is decomposed into a white-matter fODF and isotropic tissue fractions.  Where this
 * section is silent, "Constrained spherical deconvolution" above applies unchanged: basis, column order, float64 arithmetic from the
 * float32 loads on, outputs rounded once.
 * Shells: b is taken as float32.  Frames with b <= b0_thresh form shell 0 (it may be empty).  The other frames are walked in ascending b,
 *   ties in frame order: a frame joins the current shell while b <= (1 + 2 b_tol) b_first (float64 arithmetic on the float32 values),
 *   b_first the smallest b of that shell; otherwise it opens a new shell.  nshells counts shell 0.  bbar_s = the float64 mean of the shell's
 *   float32 b values (0 for an empty shell 0).  More than 8 shells above b0_thresh, or more than 512 frames in all, is FIB_ERR_UNSUPPORTED;
 *   a frame of a shell >= 1 with a zero bvec row is FIB_ERR_INVALID.  Every frame of the series is read: there is no unused frame.
 * Tissues: tissue 0 is white matter, anisotropic, n_wm = (lmax + 1)(lmax + 2) / 2 coefficients, lmax in {2, 4, 6, 8}; then niso in
 *   {0, 1, 2} isotropic tissues (by convention GM, then CSF), one coefficient each.  n = n_wm + niso <= 47; column order: the WM harmonics,
 *   then the isotropic tissues.
 * Responses are tables, not a model: wm_R [nshells][lmax / 2 + 1] row-major holds R_l per shell (the R_l of the section above),
 *   iso_r [niso][nshells] row-major the tissue's mean signal in each shell; both float32.  A table for another number of shells than the
 *   walk finds is FIB_ERR_INVALID.
 * Tables, built in float64 from those and rounded once to float32:
 *   X [nvol x n]: a shell-0 row is [Y_00 R_0(0), 0, ..], whatever its bvec says; a row of shell s >= 1 is Y(bvec) diag(R_l(s)); column
 *     n_wm + t is iso_r[t][shell(frame)].
 *   Y [nreg x n]: the basis at the first-half vertices, zero isotropic columns.
 *   B [(nreg + niso) x n]: row i < nreg is Y_i lambda (sum over frames of R_0(shell(frame))) / nreg (with one shell and no b0 frame the
 *     scaling of the section above); row nreg + t is lambda_iso (sum over frames of iso_r[t][shell(frame)]) e_{n_wm + t}.
 *   nvol < n, or an X whose rank (fib_dki_design's rule) is below n, is FIB_ERR_INVALID: this refuses two isotropic tissues on a series
 *   of fewer than three distinct shells (shell 0 counted).
 * Per voxel (skipped, all outputs 0, when the mask is 0 or no sample is > 0), with s all nvol samples:
 *   f = the least-squares solution on the WM columns of l <= 4 together with the isotropic columns, every other coefficient 0;
 *   thr_i = tau B[0,0] f[0] for i < nreg, 0 for the isotropic rows;
 *   repeat up to niter times:  a = B f;  set = {i : a_i < thr_i};  from the second pass on, stop if the set equals the previous one;
 *     solve (X'X + sum_{i in set} b_i b_i') f = X's by Cholesky.
 *   sh = f[0 : n_wm];  iso[t] = f[n_wm + t], NOT clamped (a negative fraction is diagnostic);  odf = max(Y f, 0);  niter = the number
 *   of solves;  peak[k], f[k] as in the section above. */
typedef struct fib_msmt_plan fib_msmt_plan;
typedef struct {
    int lmax;                /* 2, 4, 6 or 8 */
    int niso;                /* 0, 1 or 2 isotropic tissues */
    float b0_thresh;         /* 50 */
    float b_tol;             /* 0.05 */
    float lambda;            /* weight of the WM constraint rows (1) */
    float lambda_iso;        /* weight of the isotropic constraint rows (1) */
    float tau;               /* WM threshold as a fraction of the initial mean amplitude (0) */
    int niter;               /* most solves per voxel (50) */
} fib_msmt_params;
/* sh [n_wm][nvox], iso[t] [nvox] for t < niso (the others are not read), odf [nreg][nvox], niter [nvox], peak[k] [3][nvox], f[k] [nvox] */
typedef struct {
    float *sh;
    float *iso[2];
    float *odf, *niter;
    float *peak[3];
    float *f[3];
} fib_msmt_out;
/* Host only: R [nshells][lmax / 2 + 1] of a prolate tensor (lambda_para, lambda_perp) with b = 0 signal s0 at each bbar[s], by the 64-point
 * quadrature of the section above in float64, rounded once. */
int fib_msmt_wm_response(float lambda_para, float lambda_perp, float s0, const double *bbar, int nshells, int lmax, float *R);
/* Host only (no device needed).  shell [nvol] receives the shell of every frame, *nshells their number, bbar [9] their mean b; they are
 * filled even when the series is refused.  With wm_R NULL only this shell walk is made (verts and iso_r are not read).  Otherwise
 * X [nvol x n], B [(nreg + niso) x n], Y [nreg x n] column-major and *rank are filled whenever nshells_in matches and nvol >= n.  Any
 * output pointer may be NULL.  verts [nverts x 3] column-major. */
int fib_msmt_design(const float *bval, const float *bvec, int nvol, const float *verts, int nverts, const fib_msmt_params *params,
                    const float *wm_R, const float *iso_r, int nshells_in, int32_t *shell, int *nshells, double *bbar,
                    float *X, float *B, float *Y, int *rank);
/* faces [nfaces x 3] column-major, 1-based: the peak finder's neighbour table.  Tessellations of more than 384 directions are
 * FIB_ERR_UNSUPPORTED. */
int fib_msmt_plan_create(int device, const float *bval, const float *bvec, int nvol, const float *verts, int nverts,
                         const int32_t *faces, int nfaces, const fib_msmt_params *params, const float *wm_R, const float *iso_r,
                         int nshells_in, fib_msmt_plan **plan);
void fib_msmt_plan_destroy(fib_msmt_plan *plan);
/* host copies of the plan's tables, as fib_msmt_design returns them; any pointer may be NULL */
int fib_msmt_plan_tables(const fib_msmt_plan *plan, int32_t *shell, int *nshells, double *bbar, float *X, float *B, float *Y);
/* dwi [nvol][nvox] planar, mask uint8 [nvox].  Every output is written in every voxel.  The plan holds the peak finder's scratch of the
 * call: one call at a time per plan. */
int fibd_msmt_rec(const fib_msmt_plan *plan, const float *dwi, const uint8_t *mask, int64_t nvox, const fib_msmt_out *out, void *stream);

/* ---- Marchenko-Pastur PCA denoising (not in the reference; this section and DESIGN.md §5 are the definition) ----
 * Inputs: dwi float32 [N][nvox] planar, x fastest, N >= 2 frames; a uint8 mask; a patch edge P in {3, 5, 7}; an estimator.  Every
 *   dimension of the volume must be >= P (FIB_ERR_INVALID otherwise).
 * Patch of voxel (x, y, z): the P^3 block that starts at x0 = min(max(x - P / 2, 0), nx - P) (integer division), likewise y0, z0: the
 *   block nearest to the voxel that lies wholly inside the volume (no mirroring: mirrored patches of small volumes repeat rows and make
 *   the Gram matrix exactly singular).  The patch reads every voxel, whatever the mask says.
 * X is M x N, M = P^3; row (dz P + dy) P + dx holds the N samples of that voxel, c is the row of the voxel itself.  r = min(M, N),
 *   q = max(M, N).  G = X X' when M <= N, else X' X: r x r, float64 sums of float64 products of the float32 samples, with eigenvalues
 *   l_0 <= ... <= l_{r-1}.
 * The rule (Veraart et al. 2016 as EXP1, Cordero-Grande's variant as EXP2):
 *   lam_p = max(l_p, 0) / q;  clam = 0;  cutoff = 0;  sigma2 = 0
 *   for p = 0 .. r-1:  clam += lam_p;  gam = (p + 1) / q (EXP1) or (p + 1) / (q - (r - p - 1)) (EXP2);
 *                      s1 = clam / (p + 1);  s2 = (lam_p - lam_0) / (4 sqrt(gam));  if s2 < s1: sigma2 = s1, cutoff = p + 1
 * Per voxel inside the mask: rank = r - cutoff; sigma = sqrt(sigma2); the denoised row from E, the eigenvectors of the `rank` largest
 *   eigenvalues (equal eigenvalues: the lower index counts as the smaller): X' (E E' e_c) when M <= N, else E E' x_c.  Everything is
 *   float64 and is rounded to float32 once.  cutoff = 0 leaves the row as it is (the projector is the identity) with sigma = 0;
 *   cutoff = r gives a zero row.  Outside the mask all three outputs are 0.  rank is a count stored as float32, like every volume.
 * The eigen-decomposition is cyclic Jacobi in float64, a rotation being skipped when |g_pq| <= 2^-52 sqrt|g_pp g_qq|; a voxel that
 *   has not converged after 24 sweeps gets its input row back with sigma = NaN and rank = -1.
 * r > 128 is FIB_ERR_UNSUPPORTED: P = 5 serves any N, P = 7 up to 128 frames. */
#define FIB_DENOISE_EXP1 1
#define FIB_DENOISE_EXP2 2
/* Host only (no device needed): the refusals above for a whole volume, FIB_OK when fib_dwi_denoise would accept it. */
int fib_dwi_denoise_check(int nx, int ny, int nz, int nvol, int patch, int estimator);
/* bytes of workspace fibd_dwi_denoise needs for nz output planes: a ticket counter and the rotation records of its persistent
 * workgroups (at most 512 of them, each sized by the cap on sweeps), so it does not grow with the volume. */
int fibd_dwi_denoise_work_size(int nx, int ny, int nz, int nvol, int patch, size_t *bytes);
/* dwi holds planes [zin0, zin0 + nzin) of every frame, [nvol][nx * ny * nzin]; outputs cover planes [z0, z1): out [nvol][n], sigma [n],
 * rank [n], mask uint8 [n] with n = nx * ny * (z1 - z0).  The patch clamp is taken against the whole volume's nz, so dwi must hold the
 * planes from the patch of plane z0 to the patch of plane z1 - 1: at most P - 1 planes beyond [z0, z1), all to one side at a face.
 * work: 8-byte aligned, work_bytes >= fibd_dwi_denoise_work_size(nx, ny, z1 - z0, ...); one call at a time per workspace. */
int fibd_dwi_denoise(const float *dwi, int nx, int ny, int nz, int zin0, int nzin, int z0, int z1, int nvol, int patch, int estimator,
                     const uint8_t *mask, float *out, float *sigma, float *rank, void *work, size_t work_bytes, void *stream);

/* ---- Brain mask: median-Otsu, the volume median and the components of a mask (not in the reference; this section is the definition,
 *      DESIGN.md §5 points here, tests/mask_ref.py restates it in NumPy and the kernels are held to that bit for bit) ----
 * Linear voxel index i = x + nx (y + ny z).
 * Order of float32 values: by the ordered-uint key of the bit pattern b: key = ~b when the sign bit is set, else b | 0x80000000.  So
 *   -0 < +0, NaNs sort to the two ends by their sign bit, and every comparison below, being one of keys, has a result for any pattern.
 * Mean b0: frames is a list of frame indices (they may repeat).  b0[i] = the float64 sequential sum of the float32 samples in the
 *   list's order, divided by the count in float64, rounded to float32 once.  The sum starts from +0, so a mean of -0 samples is +0.
 * Median, radius r in {1, 2, 3}: the window of (x, y, z) is the (2r+1)^3 cube with every coordinate clamped into the volume (edge
 *   replication; any dimension >= 1); the result is the element of rank floor(n / 2) (0-based) of the n = (2r+1)^3 keys.  numpass >= 0
 *   passes, each on the output of the one before.
 * Histogram of the filtered volume: lo, hi = its smallest and largest finite value (by key; non-finite = exponent all ones).  No finite
 *   value, or hi == lo (as floats): the mask is all zero and info.status = 1 -- a result, not an error.  A finite v falls in bin
 *   min(255, (int64) floor(((double) v - lo) / ((double) hi - lo) * 256.0)); non-finite voxels enter no bin and are outside the mask.
 * Otsu on the 256 int64 counts h: for k = 0 .. 254, c0 = sum_{j<=k} h_j, s0 = sum_{j<=k} j h_j, c1 and s1 the rest; candidates with
 *   c0 == 0 or c1 == 0 are skipped; d = s0 c1 - s1 c0 (int64, exact for nvox <= 2^27; more voxels: FIB_ERR_UNSUPPORTED);
 *   crit = ((double) d * (double) d) / ((double) c0 * (double) c1); k* = the first maximum of crit.  A voxel is above threshold iff its
 *   bin > k*.  info.threshold = lo + (k* + 1) (hi - lo) / 256 in float64 is for reporting; the mask never compares against it.
 * Components: 6-connectivity over the voxels above threshold.  A component's label is 1 + the smallest linear index in it.
 *   FIB_MASK_KEEP_LARGEST keeps the component of most voxels, ties to the smaller label.
 * Holes: FIB_MASK_FILL_HOLES adds every 6-connected component of the complement that has no voxel on a face of the volume.
 * Dilation: dilate >= 0 passes of the 6-neighbourhood, last.
 * info: status (0; 1 = no threshold exists, see above; -1 = an iteration cap of the labelling was reached, which a correct run never
 *   does), kstar (-1 with status 1), lo, hi (0 without a finite value), threshold (0 with status 1), n_above (voxels above threshold),
 *   n_components (of those), n_kept (after the selection), n_filled (added by the holes), n_mask (the result's voxels). */
#define FIB_MASK_KEEP_LARGEST 1
#define FIB_MASK_FILL_HOLES 2
typedef struct {
    int radius, numpass;      /* the median */
    int flags;                /* FIB_MASK_KEEP_LARGEST | FIB_MASK_FILL_HOLES */
    int dilate;
} fib_mask_params;
typedef struct {
    int32_t status, kstar;
    float lo, hi;
    double threshold;
    int64_t n_above, n_components, n_kept, n_filled, n_mask;
} fib_mask_info;
/* Host only (no device needed): the refusals of dwi_mask -- radius outside 1..3, negative numpass or dilate, unknown flags, an empty
 * frame list or an index outside [0, nvol): FIB_ERR_INVALID; more than 2^27 voxels: FIB_ERR_UNSUPPORTED. */
int fib_dwi_mask_check(int nx, int ny, int nz, int nvol, const int32_t *frames, int nframes, const fib_mask_params *params);
/* The median of a device volume: in, out float32 [nx * ny * nz], distinct buffers; numpass = 0 copies.  work: 8-byte aligned,
 * fibd_vol_median_work_size bytes (one volume when numpass >= 2). */
int fibd_vol_median_work_size(int nx, int ny, int nz, int numpass, size_t *bytes);
int fibd_vol_median(const float *in, int nx, int ny, int nz, int radius, int numpass, float *out, void *work, size_t work_bytes, void *stream);
/* Components of a device mask (uint8, nonzero = inside), then the selection and the holes as `flags` say.  out_mask (or NULL): the
 * result as 0 / 1; labels (or NULL): int32, the labels of the result's components (0 outside).  info: 64 bytes of DEVICE memory
 * (status, n_above = the input's voxels, n_components, n_kept, n_filled, n_mask; the rest 0), complete when the stream has run.
 * At most 2^27 voxels. */
int fibd_mask_components_work_size(int nx, int ny, int nz, size_t *bytes);
int fibd_mask_components(const uint8_t *mask, int nx, int ny, int nz, int flags, int32_t *labels, uint8_t *out_mask, fib_mask_info *info,
                         void *work, size_t work_bytes, void *stream);
/* dwi_mask on a planar device series: frame f begins at dwi + f * frame_stride (frame_stride >= nx * ny * nz); frames is a HOST list of
 * nframes indices into the nvol frames.  mask uint8 [nvox], b0 float32 [nvox] or NULL, info in DEVICE memory; nothing returns to the
 * host between the steps.  Up to 64 frames are summed and finalised in one launch, longer lists frame by frame into a float64 buffer
 * of the workspace: the same sums. */
int fibd_dwi_mask_work_size(int nx, int ny, int nz, size_t *bytes);
int fibd_dwi_mask(const float *dwi, int64_t frame_stride, int nvol, const int32_t *frames, int nframes, int nx, int ny, int nz,
                  const fib_mask_params *params, uint8_t *mask, float *b0, fib_mask_info *info, void *work, size_t work_bytes, void *stream);

/* ---- Gibbs-ringing removal: local subvoxel shifts (not in the reference; after Kellner et al. 2016, the method of MRtrix's mrdegibbs
 *      and dipy's gibbs_removal; this section is the definition, DESIGN.md §5 points here and tests/degibbs_ref.py restates it in
 *      float64 by two routes.  Conformity to either tool bit for bit is not claimed) ----
 * dwi: float32 [N][nvox], planar, x fastest.  slice_axis in {0, 1, 2} names the axis across the slices; the two other axes, in
 *   ascending order, are the in-plane axes u and v of sizes nu and nv.  nshifts K, 1 <= K <= 32; windows 1 <= minW <= maxW <= 6.
 *   Each in-plane size must be >= 2 maxW + 3 (FIB_ERR_INVALID) and <= FIB_DEGIBBS_MAX_SIZE (FIB_ERR_UNSUPPORTED, the limit in the
 *   message).  There is no mask: the method works on whole slices, and slices and frames are independent of each other.
 * Everything below is float64 on the float32 samples; the result is rounded to float32 once.  No fused contraction is prescribed.
 * Per slice a[u][v]:
 *   1. A = DFT2(a), A[p][q] = sum a[u][v] e^{-2 pi i (p u / nu + q v / nv)}.
 *   2. cu[p] = 1 + cos(2 pi p / nu), and exactly 0 when 2 p == nu; cv[q] likewise.
 *   3. Gu = cv / (cu + cv), Gv = cu / (cu + cv); both are 0 in the bin where 2 p == nu and 2 q == nv (decided by the integer test).
 *   4. au = Re IDFT2(A Gu), av = Re IDFT2(A Gv): au still rings along u only, av along v only.
 *   5. result = unring(au along u) + unring(av along v).
 * unring of one row r[0 .. n-1], indices circular.  Candidates, J = 2 K + 1: s_0 = 0, s_j = j / J for j = 1 .. K, s_{K+j} = -j / J for
 *   j = 1 .. K.  r_0 = r; for j >= 1, r_j[l] = sum_m r[m] D(l - m + s_j) with D(t) = (1 / n) (1 + 2 sum_{k=1..h} cos(2 pi k t / n)),
 *   h = floor((n - 1) / 2): the band-limited row sampled at l + s_j, the Nyquist term of an even n dropped.
 *   d_j[l] = |r_j[l+1] - r_j[l]|; L_j[l] = sum_{w=minW..maxW} d_j[l-w-1]; R_j[l] = sum_{w=minW..maxW} d_j[l+w], both sequential in
 *   ascending w; t_j[l] = min(L_j[l], R_j[l]); j*(l) = the first j, in the order above, that attains min_j t_j[l].
 *   Output, s = s_{j*}: s > 0: r_{j*}[l] (1 - s) + r_{j*}[l-1] s; otherwise r_{j*}[l] (1 + s) - r_{j*}[l+1] s.  j* = 0 returns r[l].
 * Consequences: an all-zero slice returns exact zeros (every candidate ties at 0 and j* = 0).  A slice that holds a non-finite sample
 *   has an unspecified result; the call still returns FIB_OK and every other slice is unaffected.
 * shift_u, shift_v (int8 [N][nvox], or NULL): j* of the search along u and along v, the diagnostic that lets the choice be checked. */
#define FIB_DEGIBBS_MAX_SIZE 256
typedef struct {
    int slice_axis;           /* 0, 1 or 2: the axis across the slices */
    int nshifts;              /* K */
    int minW, maxW;
} fib_degibbs_params;
#define FIB_DEGIBBS_PARAMS_DEFAULT { 2, 20, 1, 3 }
/* Host only (no device needed): the refusals above, non-positive dimensions and nvol < 1 (FIB_ERR_INVALID).  params NULL: the default. */
int fib_dwi_degibbs_check(int nx, int ny, int nz, int nvol, const fib_degibbs_params *params);
/* Host only: the circulant table of a row length n (1 .. FIB_DEGIBBS_MAX_SIZE), float64 [2 nshifts][n]: table[(j - 1) n + t] =
 * D(t + s_j), t = 0 .. n - 1, summed in extended precision and rounded once.  The kernels read this table. */
int fib_degibbs_table(int n, int nshifts, double *table);
/* The device entry: dwi, out float32 [nvol][nvox] on the device, distinct buffers (out == dwi, or any overlap: FIB_ERR_INVALID);
 * shift_u, shift_v int8 [nvol][nvox] or NULL.  work: 8-byte aligned, fibd_dwi_degibbs_work_size bytes (the tables and the float64
 * planes of a batch of slices; the batch does not change the result).  Asynchronous on `stream`. */
int fibd_dwi_degibbs_work_size(int nx, int ny, int nz, int nvol, const fib_degibbs_params *params, size_t *bytes);
int fibd_dwi_degibbs(const float *dwi, int nx, int ny, int nz, int nvol, const fib_degibbs_params *params, float *out, int8_t *shift_u,
                     int8_t *shift_v, void *work, size_t work_bytes, void *stream);

/* gqi_rec / dsi_rec volume loop + find_peaks! + peak/qa extraction (gqi.jl:132-162,
 * dsi.jl:197-261).  odf [nvox*nvert] planar; pdf [nvox*nvol] (DSI plans only, else NULL);
 * peak[k] [nvox*3] planar, qa[k] [nvox].  `flags` is a bit set:
 *   FIB_ODF_NORMALIZE  the global step qa ./= maximum(mean(odf, dims=4)) (gqi.jl:164-168,
 *                      dsi.jl:263-267) is applied in-stream; without it qa is left un-normalised and
 *                      *odfmax_dev (device float[2]: {max, nan-flag}) holds this call's local maximum so
 *                      that ranks can all-reduce it and call fibd_qa_normalize;
 *   FIB_ODF_PREZEROED  the caller guarantees that every output is already 0 at the voxels outside
 *                      `mask` (e.g. buffers from a previous call with the same mask); otherwise they
 *                      are zero-filled here, like the reference's freshly allocated volumes;
 *   FIB_ODF_SEPARATE_PEAKS  run find_peaks! as its own kernel on the stored ODF instead of on the contraction
 *                      kernel's accumulators (the fused form needs 16-byte aligned rows, nvox % 4 == 0, and
 *                      computes two of the 321 rows of sphere_642 with a different rounding): a caller that
 *                      cuts one volume into pieces sets it for ALL pieces when any piece is unaligned, so
 *                      that the result does not depend on the cut (the host-buffer tier does).
 *   FIB_ODF_RAW_ODFMAX the form of *odfmax_dev a MAX all-reduce can take as it is: {maximum of the voxel means that
 *                      are not NaN (-Inf if there is none), nan-flag}.  Without it the first element is NaN when the
 *                      flag is set (what maximum() returns, gqi.jl:164).  fibd_qa_normalize_pair consumes the raw form.
 * Only voxels inside the mask are computed: the mask is compacted on the device into a voxel list
 * (reconstruction) and a list of 64-voxel tiles (peak finder), so cost scales with the mask. */
#define FIB_ODF_NORMALIZE 1
#define FIB_ODF_PREZEROED 2
#define FIB_ODF_SEPARATE_PEAKS 4
#define FIB_ODF_RAW_ODFMAX 8
int fibd_odf_rec(const fib_odf_plan *plan, const float *dwi, const uint8_t *mask, int64_t nvox,
                 float *pdf, float *odf, float *const peak[3], float *const qa[3],
                 float *odfmax_dev, int flags, void *stream);
/* qa[k] ./= odfmax for all voxels (gqi.jl:166-168) */
int fibd_qa_normalize(float *const qa[3], int64_t nvox, float odfmax, void *stream);
/* same with the divisor read from device memory (the all-reduced odfmax stays on the device: no host round trip) */
int fibd_qa_normalize_dev(float *const qa[3], int64_t nvox, const float *odfmax_dev, void *stream);
/* .. from the raw pair {maximum of the non-NaN means, nan-flag} (FIB_ODF_RAW_ODFMAX, MAX-all-reduced over the ranks): the
 * divisor is NaN when the flag is set, and odfmax_pair_dev[0] is rewritten to that divisor (what maximum() returns) */
int fibd_qa_normalize_pair(float *const qa[3], int64_t nvox, float *odfmax_pair_dev, void *stream);

/* find_peaks!(W) (gqi.jl:180-201) on a planar ODF volume [nvox*nvert]: for every voxel the
 * indices (0-based, first-half vertex rows) of the first 3 entries of `isort` and `nvalid`.
 * isort_top [3*nvox] planar int32 (-1 where fewer than k+1 vertices exist). */
int fibd_find_peaks(const fib_odf_plan *plan, const float *odf, int64_t nvox,
                    int32_t *isort_top, int32_t *nvalid, void *stream);
/* .. with all of the work struct's outputs: odf_peak [nvert*nvox] planar (gqi.jl:184-196), isort [nvert*nvox] planar int32
 * (the complete permutation, 0-based, gqi.jl:198), nvalid [nvox] (gqi.jl:200) */
int fibd_find_peaks_work(const fib_odf_plan *plan, const float *odf, int64_t nvox,
                         float *odf_peak, int32_t *isort, int32_t *nvalid, void *stream);

/* ------------------------------------------------------------------------------------ */
/* RUMBA-SD (rusd.jl), SURVEY.md row N4                                                   */
/* ------------------------------------------------------------------------------------ */
typedef struct fib_rumba_plan fib_rumba_plan;   /* kernel of the multi-tensor model + the two contraction plans */

/* rumba_rec's set-up (rusd.jl:449, 466-521, 529-531): ib0 = (bval .== minimum(bval)); the kernel K [ndir x (nvert+2)]
 * (ndir = 1 + number of non-low-b frames; one prolate tensor per half-sphere vertex, isotropic CSF and GM columns),
 * the angular peak neighbourhoods (12.5 deg for sphere_642/724, 16 deg for sphere_362) and the uniform initial fODF.
 * verts [nverts x 3] column-major as for the GQI plan.  Reference defaults: lam_para 1.7e-3, lam_perp 0.2e-3,
 * lam_csf 3.0e-3, lam_gm 0.8e-4. */
int fib_rumba_plan_create(int device, const float *bval, const float *bvec, int nvol, const float *verts, int nverts,
                          float lam_para, float lam_perp, float lam_csf, float lam_gm, fib_rumba_plan **plan);
void fib_rumba_plan_destroy(fib_rumba_plan *plan);
/* host copy of the kernel, column-major [ndir x ncomp]; K == NULL queries the sizes only */
int fib_rumba_plan_kernel(const fib_rumba_plan *plan, float *K, int *ndir, int *ncomp);

/* outputs of rumba_rec (the RUMBASD struct, rusd.jl:11-20): fodf planar [nvert][nvox]; fgm, fcsf, gfa, var [nvox];
 * peak[k] planar [3][nvox], k = 0..4 */
typedef struct {
    float *fodf, *fgm, *fcsf, *gfa, *var;
    float *peak[5];
} fib_rumba_out;

/* rumba_rec(dwi, mask, odf_dirs, niter, ...) (rusd.jl:419-636) on device-resident volumes: dwi planar [nvol][nvox],
 * mask uint8 [nvox] (already `> 0`-tested).  niter: Richardson-Lucy iterations (reference default 600); ncoils /
 * sos_grappa: coil_combine == "SoS-GRAPPA" uses n_order = ncoils, "SMF-SENSE" n_order = 1; ipat_factor >= 1; use_tv:
 * total-variation prior.  snr_mean / snr_std: host scalars (may be NULL).  Blocking.  The plan keeps the call's work arrays
 * (8 x [ndir or ncomp][masked voxels] floats) for the next call: one call at a time per plan; destroy the plan to release them. */
int fibd_rumba_rec(const fib_rumba_plan *plan, const float *dwi, const uint8_t *mask, int nx, int ny, int nz,
                   int niter, int ncoils, int sos_grappa, int ipat_factor, int use_tv,
                   const fib_rumba_out *out, float *snr_mean, float *snr_std, void *stream);

/* ------------------------------------------------------------------------------------ */
/* Streamlines                                                                            */
/* ------------------------------------------------------------------------------------ */
typedef struct {
    int32_t nx, ny, nz, nvec;
    int32_t len_min;        /* default 3 */
    int32_t len_max;        /* default max(nx,ny,nz)      (stream.jl:74) */
    float cosang_thresh;    /* cosd(ang_thresh), default cosd(45) (stream.jl:193) */
    float step_size;        /* default .5 */
    float smooth_coeff;     /* default .2 */
    /* microscopy regime (stream.jl:83: minimum(volres) <= 0.05 mm; 252-287, 547-619): search_dist > 0 selects it.
     * Each step then moves to the voxel, within search_dist voxels of the tentative position and a cone of
     * search_ang around the current direction, whose first orientation vector is best aligned with it.
     * Reference defaults in that regime: search_dist 15, search_ang 10, nsub 0, ang_thresh 20, step 1, smooth 0. */
    int32_t search_dist;    /* 0: macro-scale tracking */
    float search_cosang;    /* cosd(search_ang) */
    struct fib_stream_ws *ws;   /* optional scratch arena (fibd_stream_ws_create); NULL: the job allocates and frees its own */
    /* 0: the reference's nearest-voxel lookup (stream.jl:514).  1: NOT in the reference — the direction followed is the trilinear
     * blend of the 8 voxels around the tentative position: w = normalise(sum_c t_c s_c u_c), t_c the trilinear weight of corner c
     * (corners outside the volume dropped), u_c the corner's vector picked by the angle rule of stream.jl:340-374 against the
     * current direction (corners without a vector dropped), s_c the sign of its cosine; a zero blend ends the line.  Bounds,
     * mask and the nearest voxel's pick still decide termination exactly as in the reference; macro scale, angle picking only.
     *
     * 2, 3: the same trilinear field with a midpoint (RK2) / classical Runge-Kutta (RK4) integrator instead of forward Euler (NOT in
     * the reference either; the FIB_STREAM_* constants below).  Let D(p, r) be the blend above: the direction at position p, corners
     * picked and sign-aligned against the reference direction r, normalised; NONE when the blend is zero or not finite or p is not
     * finite.  A step of the trilinear tracker at state (pos, vec) is
     *     nxt = pos + vec * step ; bounds / mask / nearest-voxel pick at nxt (ends the pass, sets the carried vector index) ;
     *     vnext = D(nxt, vec) (NONE ends the pass) ; emit pos ; bend test dot(vec, vnext) ; len_max ; smoothing ; advance
     * and the integrator changes ONLY how nxt is obtained from (pos, vec) -- vnext and the bend test stay taken against vec.
     * With h = step, half = step * 0.5f, sixth = step / 6.0f (one IEEE division), all Float32, every multiply and add rounded on
     * its own (no fused multiply-add), component-wise:
     *     1 Euler:    nxt = pos + vec * h
     *     2 midpoint: k2 = D(pos + vec * half, vec) ;  nxt = pos + k2 * h
     *     3 RK4:      k2 = D(pos + vec * half, vec) ;  k3 = D(pos + k2 * half, k2) ;  k4 = D(pos + k3 * h, k3) ;
     *                 s = ((vec + 2 * k2) + 2 * k3) + k4 ;  nxt = pos + s * sixth          (the sum is not renormalised)
     * A stage whose D is NONE ends the pass exactly like an invalid nxt does (stream.jl:657): pos is not emitted.  Stage positions
     * are not tested against bounds or mask by themselves: corners outside the volume and masked voxels contribute nothing to D,
     * and an empty blend is NONE.  k1 is the CARRIED direction vec -- with smooth_coeff > 0 that is the smoothed direction, not a
     * fresh sample of the field at pos, which costs RK4 some of its accuracy (CPU restatement, circles of radius 9-16 voxels,
     * step 0.5: drift <= 0.002 voxel without smoothing, 0.06-0.12 with smooth_coeff 0.2; midpoint <= 0.002 either way; Euler
     * 0.8-1.3 and 1.1-1.9).  Values 1, 2, 3 with the microscopy regime or LCMs: FIB_ERR_UNSUPPORTED. */
    int32_t interp;
    /* microscopy regime with 2-D orientation-angle inputs (one frame per volume, stream.jl:147-172): StreamWork sets the search
     * distance of the through-plane axis -- the one with the largest voxel size -- to 0 (stream.jl:153-155).  0: none (a cubic
     * search area); 1, 2, 3: the x, y, z axis is searched over one voxel only.  (The angles themselves are expanded to 3-D
     * vectors by the host-language wrapper, cos / sin or cosd / sind like the constructor does: ovec stays [nvox*3].) */
    int32_t search_flat_axis;
} fib_stream_params;

/* values of fib_stream_params.interp */
#define FIB_STREAM_NEAREST 0        /* nearest voxel, forward Euler: the reference (stream.jl:512-520) */
#define FIB_STREAM_TRILINEAR 1      /* trilinear blend, forward Euler */
#define FIB_STREAM_TRILINEAR_RK2 2  /* trilinear blend, midpoint rule */
#define FIB_STREAM_TRILINEAR_RK4 3  /* trilinear blend, classical Runge-Kutta */

typedef struct fib_stream_job fib_stream_job;
/* Grow-only scratch arena of the tracer, owned by the caller (the reference's per-thread StreamWork scratch, stream.jl:43-60):
 * worst-case point rows for every line (3.4 GB per million lines at len_max 140) are expensive to allocate per call.  One job
 * at a time takes the arena; a job that finds it busy (or on another device) allocates its own scratch.  Releasing is
 * stream-ordered: the next job waits on its own stream for the previous job's last launch. */
typedef struct fib_stream_ws fib_stream_ws;
int fibd_stream_ws_create(int device, fib_stream_ws **ws);
void fibd_stream_ws_destroy(fib_stream_ws *ws);

/* StreamWork mask + vector repack (stream.jl:95-145): mask_out = (mask > 0 | any nonzero vector)
 * & (fa >= fa_thresh); field[vox][k] = ovec[k][vox,:] * (mask_out & f[k] >= f_thresh), stored as
 * float4 (xyz0) [nvox*nvec].  ovec[k] planar [nvox*3]; f[k] [nvox] or f == NULL; fa, mask may be NULL. */
int fibd_stream_field(int32_t nvec, int64_t nvox, const float *const *ovec, const float *const *f,
                      float f_thresh, const float *fa, float fa_thresh, const uint8_t *mask,
                      float *field4, uint8_t *mask_out, void *stream);

/* stream_new_line for every (seed, sub-voxel offset) pair (stream.jl:761-781 + 625-690, angle
 * picking, non-LCM, macro scale).  seeds: int64 [nseed] 0-based column-major linear voxel indices
 * in the reference's findall order; sublist [nsub*3] (xyz per offset; caller-generated, stream.jl:176-181).
 * Traces into library-owned scratch, applies len_min (stream.jl:769) and computes output offsets.
 * Synchronises `stream`; returns the number of kept lines and their total point count.
 * field4, seeds and sublist must stay valid and unchanged until the job has been packed.  Orientation fields of 2^28 vectors
 * (4 GiB) or more take a form of the tracer with 64-bit gather offsets, chosen at launch. */
int fibd_stream_trace(const fib_stream_params *prm, const float *field4, const int64_t *seeds, int64_t nseed,
                      const float *sublist, int32_t nsub, void *stream,
                      fib_stream_job **job, int64_t *nlines, int64_t *npoints);
/* packs the kept lines, in (seed, sub) order == reference order, into caller device buffers:
 * npts [nlines] int32, seed_index [nlines] int64 (= seed*nsub+sub), xyz [3*npoints] (x,y,z per point,
 * line after line, each line ordered [fwd_N..fwd_1, bwd_1..bwd_M] as stream.jl:652 builds it). */
int fibd_stream_pack(fib_stream_job *job, int32_t *npts, int64_t *seed_index, float *xyz, void *stream);

/* trace + pack in ONE call into caller-provided device buffers (npts [lines_cap] int32, seed_index [lines_cap] int64, xyz
 * [3*points_cap] float): the same lines, order and layout as fibd_stream_trace + fibd_stream_pack without the second call and
 * without any allocation on the caller's side of the boundary between them.  From 2^21 lines on (nearest-voxel tracking, 1, 2 or 3
 * vectors per voxel, lines that fit a 16-line LDS tile) it is ONE kernel: the workgroup that traced 512 lines packs them behind a
 * decoupled look-back over the workgroups' totals.  *nlines / *npoints receive the totals; when they exceed the capacities the call
 * returns FIB_ERR_CAPACITY (lines that did not fit are missing from the buffers; call again with larger ones).  Macro-scale angle
 * picking only (prm->search_dist == 0, no LCMs); synchronises `stream`. */
int fibd_stream_run(const fib_stream_params *prm, const float *field4, const int64_t *seeds, int64_t nseed,
                    const float *sublist, int32_t nsub, int32_t *npts, int64_t *seed_index, int64_t lines_cap,
                    float *xyz, int64_t points_cap, int64_t *nlines, int64_t *npoints, void *stream);

/* fibd_stream_run without the host round trip at its end: returns once the work is enqueued on `stream`, which also writes
 * counts_dev[0] = lines, counts_dev[1] = points (DEVICE memory, 2 x int64; the totals the run NEEDED: larger than the capacities when
 * lines were dropped for lack of room -- compare after synchronising, there is no FIB_ERR_CAPACITY here).  The buffers and the
 * workspace of prm->ws stay in use until `stream` has passed the call.  For callers that keep a stream of volumes in flight: the
 * synchronising form idles the GPU for the download of its two counts between consecutive calls. */
int fibd_stream_run_enqueue(const fib_stream_params *prm, const float *field4, const int64_t *seeds, int64_t nseed,
                            const float *sublist, int32_t nsub, int32_t *npts, int64_t *seed_index, int64_t lines_cap,
                            float *xyz, int64_t points_cap, int64_t *counts_dev, void *stream);

/* LCM-guided tracking (stream(...; lcms, lcm_thresh), stream.jl:200-236, 380-495, 526-538): when a line enters a new
 * voxel the exit edge is drawn from the voxel's local connection matrix restricted to the entry edge, and the
 * orientation vector best aligned with a jump towards that edge is followed; the angle threshold is not applied
 * (stream.jl:668).  lcms: planar [10][nvox] = MRI.vol[nx,ny,nz,10]; elements below lcm_thresh are dropped
 * (stream.jl:217).  strdim0/1: the two in-plane dimensions (0-based; the reference takes the dimension in which the
 * first orientation volume is zero everywhere as through-plane, stream.jl:221-223).
 * RANDOM-NUMBER CONTRACT.  The reference draws `rand(Categorical(lcm))` from Julia's global RNG, which no other
 * implementation can reproduce.  Here the k-th uniform consumed by streamline `line` (= seed*nsub + sub) is
 *     u = float(splitmix64(rng_seed ^ splitmix64(line * 0xD1342543DE82EF95 + k)) >> 40) * 2^-24   in [0,1),
 * and the category is the first index whose running sum of the normalised weights exceeds u (what
 * Distributions.jl's sampler does with its uniform).  Results depend on rng_seed only, not on scheduling.
 * fibd_stream_pack_flags additionally returns one byte per point: the LCM pick and the angle pick chose different
 * vectors (the `flags` the reference stores as a per-point scalar of the Tract, stream.jl:538, 666, 787). */
int fibd_stream_trace_lcm(const fib_stream_params *prm, const float *field4, const float *lcms, float lcm_thresh,
                          int32_t strdim0, int32_t strdim1, uint64_t rng_seed,
                          const int64_t *seeds, int64_t nseed, const float *sublist, int32_t nsub, void *stream,
                          fib_stream_job **job, int64_t *nlines, int64_t *npoints);
int fibd_stream_pack_flags(fib_stream_job *job, int32_t *npts, int64_t *seed_index, float *xyz, uint8_t *flags, void *stream);
/* same lines serialised as the body of a TrackVis .trk file (everything after the 1000-byte header, as
 * trk_write emits it, trk.jl:469-485): per line Int32 npts then npts x 3 Float32 = (xyz + .5) * voxel_size.
 * body: device buffer of 4*nlines + 12*npoints bytes. */
int fibd_stream_pack_trk(fib_stream_job *job, const float voxel_size[3], void *body, void *stream);
/* the .trk body of str_xform(xfm, tr) (trk.jl:316-347) for the lines of `job`, straight from the tracer's scratch: every point goes
 * through xfm_apply (util.jl:401-420, vox2vox as in fibd_xfm_apply, applied to stream's 1-based coordinates as they are) and then
 * the same epilogue, (p + .5) * voxel_size with voxel_size = xfm.outres.  LCM jobs: FIB_ERR_UNSUPPORTED, as fibd_stream_pack_trk. */
int fibd_stream_pack_trk_xfm(fib_stream_job *job, const float vox2vox[16], const float voxel_size[3], void *body, void *stream);
/* fib_xfm_apply's device form: in / out are device buffers, asynchronous on `stream`.  One streaming kernel (24 B per point). */
int fibd_xfm_apply(const float vox2vox[16], const float *in, float *out, int64_t npoints, void *stream);
/* per-(seed,sub) point counts of every traced line, incl. those dropped by len_min: int32 [nseed*nsub] */
int fibd_stream_all_npts(fib_stream_job *job, int32_t *all_npts, void *stream);
void fib_stream_job_destroy(fib_stream_job *job);

/* ------------------------------------------------------------------------------------ */
/* Tract maps: density, along-tract sampling, line statistics (NOT in the reference)     */
/* ------------------------------------------------------------------------------------ */
/* Inputs are PACKED LINES as fibd_stream_run / fibd_stream_pack emit them and `Tract` holds them: xyz float32 [npoints][3] (x, y, z
 * of a point adjacent, 1-based voxel coordinates), npts int32 [nlines], lines one after the other.  Points need only be 4-byte
 * aligned (views into a larger buffer), as for fibd_xfm_apply.  These definitions are this project's own; they are the contract.
 *
 * VOXEL OF A POINT.  v = rint(p) per component, ties to even (the tracer's rule, stream.jl:514).  The point is INSIDE iff all three
 * components are finite and 1 <= v_x <= nx, 1 <= v_y <= ny, 1 <= v_z <= nz, tested on the float value before any conversion to an
 * integer (+-1e30, +-Inf and NaN are simply outside).  Linear index lin(v) = (v_x-1) + nx*((v_y-1) + ny*(v_z-1)), 64-bit.
 *
 * DENSITY D, uint32 [nx*ny*nz]; `mode` is one of
 *   FIB_DENSITY_POINTS     D[v] = number of inside points with voxel v;
 *   FIB_DENSITY_LINES      D[v] = number of lines that have AT LEAST ONE inside point with voxel v: a line counts once per voxel
 *                          however often it samples it or comes back to it (track density).  Exact for lines of any length (lines of
 *                          up to 256 points are de-duplicated in LDS, longer ones through a bitmap over the voxels they span);
 *                          volumes of 2^31 voxels or more: FIB_ERR_UNSUPPORTED in this mode;
 *   FIB_DENSITY_ENDPOINTS  for every line with npts >= 1, +1 at the voxel of its first point and +1 at the voxel of its last point
 *                          (a one-point line adds 2 to one voxel), each only if inside;
 * optionally OR-ed with
 *   FIB_DENSITY_ACCUMULATE add to what D holds; without it the call zero-fills D first.  Tractograms that arrive in batches sum into
 *                          one map, and integer sums make the result independent of batch and arrival order (two runs: same bytes).
 * n_outside (int64): the number of points (POINTS, LINES) or line ends (ENDPOINTS) that were not inside, so that
 * sum(D) + n_outside = npoints in mode POINTS and = 2 * #{npts >= 1} in mode ENDPOINTS (on a zero-filled D).  Counts wrap at 2^32.
 * Lines with npts = 0 are legal and contribute nothing.  npts < 0 or sum(npts) != npoints is FIB_ERR_INVALID: the host form checks
 * before anything is written; the device form cannot without a host round trip -- its offset scan sees both, the kernels behind it
 * then add nothing and *n_outside_dev is set to -1 (D is zero-filled, or with ACCUMULATE left as it was; never partly counted).
 *
 * SAMPLE S, float32 [npoints][nframes] (point-major, the order of .trk records and Tract.scalars): S[i][f] = vol[f][lin(v_i)] if
 * point i is inside, else `outside` (NaN allowed).  vol planar float32 [nframes][nvox] = MRI.vol.  Nearest voxel only.
 *
 * LINE STATISTICS P, float32 [nlines][1 + nscalars] (line-major, Tract.properties):
 *   column 0       length in mm: the sum over the line's consecutive point pairs of
 *                  sqrt(((x1-x0)*r_x)*((x1-x0)*r_x) + ((y1-y0)*r_y)*((y1-y0)*r_y) + ((z1-z0)*r_z)*((z1-z0)*r_z)), every operation in
 *                  float64 on the float32 inputs (r = volres as float32), the three squares added left to right, no fused
 *                  multiply-add, the sum rounded to float32 once.  0 for npts <= 1.
 *   column 1 + c   the mean of column c of the per-point scalars [npoints][nscalars] over the line's points: float64 sum, divided by
 *                  npts in float64, rounded once.  NaN samples propagate; npts = 0 gives NaN (0/0).
 * The ORDER of either sum is free (lanes reduce a line in parallel): an n-term float64 sum in any order differs from the sequential
 * one by at most n * 2^-53 * sum|t_i|, and rounding to float32 moves either by at most one float32 ulp.  The device form writes no
 * row at all for an input its offset scan refuses (npts < 0, sum(npts) != npoints). */
#define FIB_DENSITY_POINTS 0
#define FIB_DENSITY_LINES 1
#define FIB_DENSITY_ENDPOINTS 2
#define FIB_DENSITY_ACCUMULATE 0x100
/* bytes of device scratch fibd_str_density / fibd_str_stats need for nlines lines (the int64 offset of every line's first point and the
 * scan's block totals); 8-byte aligned */
int fibd_str_work_size(int64_t nlines, size_t *bytes);
/* density: xyz, npts, density, n_outside_dev (one int64) and work are device pointers.  Asynchronous on `stream`, no allocation and no
 * synchronisation inside.  Adds are vector atomics on uint32, one per run of consecutive points in the same voxel. */
int fibd_str_density(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz, int mode,
                     uint32_t *density, int64_t *n_outside_dev, void *work, size_t work_bytes, void *stream);
/* sample: one pass over the points.  nlines is not needed (a sample belongs to a point).  npoints = 0 does nothing. */
int fibd_str_sample(const float *xyz, int64_t npoints, const float *vol, int nx, int ny, int nz, int nframes, float outside,
                    float *scalars, void *stream);
/* statistics: scalars may be NULL when nscalars = 0 (props is then [nlines][1]: the lengths) */
int fibd_str_stats(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, const float volres[3], const float *scalars,
                   int nscalars, float *props, void *work, size_t work_bytes, void *stream);

/* ------------------------------------------------------------------------------------ */
/* Tract selection and connectomes: ROI filters, label matrix (NOT in the reference)     */
/* ------------------------------------------------------------------------------------ */
/* Inputs are PACKED LINES exactly as for the tract maps above (xyz float32 [npoints][3], 4-byte alignment suffices; npts int32
 * [nlines]); the VOXEL OF A POINT, the INSIDE test and lin(v) are the ones defined there and nothing else.  These definitions are
 * this project's own; they are the contract.  npts is INVALID if any entry is negative or sum(npts) != npoints; the device forms see
 * that in their offset scan (no host round trip) and refuse as said under each function.
 *
 * ROI BIT VOLUME roibits, uint32 [nvox]: bit r is set iff ROI r (r < 32) is non-zero at that voxel, so that one 4-byte gather per
 * point serves up to 32 ROIs.  fibd_str_roi_pack makes it from rois, planar uint8 [nroi][nvox] (any non-zero byte sets the bit;
 * bits nroi..31 are 0).
 *
 * SELECTION.  Per-line predicates, all three 0 for an empty line:
 *   visit  the OR of roibits[lin(v)] over the line's inside points;
 *   end0   roibits at the voxel of the first point if that point is inside, else 0;
 *   end1   the same for the last point (a one-point line has end0 == end1).
 * The RULE is four masks and a point-count window.  A line is KEPT iff all of
 *   (visit & visit_all) == visit_all          it passes through every ROI of visit_all
 *   (visit & visit_none) == 0                 and through none of visit_none
 *   ((end0 | end1) & end_any) == end_any      every ROI of end_any holds at least one of its ends
 *   (end0 & end1 & end_both) == end_both      every ROI of end_both holds both
 *   min_npts <= npts and (max_npts == 0 or npts <= max_npts)
 * hold.  With every mask 0 and the window (0, 0) every line is kept, lines with npts = 0 included.  The masks are 32-bit; they
 * travel as uint64_t, as every unsigned scalar of this ABI does, and a bit above bit 31 is FIB_ERR_INVALID.  roibits may be NULL
 * when all four masks are 0 (the predicates are then 0).
 * Outputs: keep uint8 [nlines], 0 or 1; hits uint32 [nlines][3] = {visit, end0, end1}, may be NULL; counts int64 [2] in device
 * memory = {kept lines, kept points}.  INVALID npts: keep is zero-filled, hits is left untouched, counts = {-1, -1}.
 *
 * COMPACTION (gather) takes ANY keep flags, not only those of the selection: a line is kept iff keep[line] != 0.  The kept lines are
 * copied in input order (stable): xyz_out [kept points][3], npts_out [nkept], optionally index_out int64 [nkept] = the line's index
 * in the input (what carries seed_index, properties or anything else per line) and scalars_out [kept points][nscalars] from scalars
 * [npoints][nscalars].  The copies are byte-identical (32-bit words: NaN payloads and -0.0 survive).  counts int64 [3] in device
 * memory = {kept lines, kept points, status}: the true totals and status 0; if a total exceeds cap_lines / cap_points the totals are
 * still true, status is -1 and NOTHING is written to the four outputs; INVALID npts: {-1, -1, 0} and nothing is written.  There is
 * never a partial result.
 *
 * CONNECTOME.  labels int32 [nvox]; remap int32 [nremap] or NULL for the identity; L = nnodes, the number of nodes.  NODE OF A LINE
 * END: 0 if the end point is outside; else x = labels[lin(v)], y = remap[x] (remap NULL: y = x; x outside 0 <= x < nremap: y = 0),
 * and the node is y if 1 <= y <= L, else 0.  Node 0 means "unassigned".  For every line with npts >= 1 let a, b be the nodes of its
 * first and last point, i = min(a, b), j = max(a, b):
 *   C[i][j] += 1, and if i != j also C[j][i] += 1.  C is uint32 [L+1][L+1], row-major, symmetric; row and column 0 hold the
 *              unassigned ends; a self-connection counts once, on the diagonal.  The sum of the upper triangle with the diagonal
 *              is #{npts >= 1} (on a zero-filled C).  Counts wrap at 2^32.
 *   W[i][j] (and W[j][i] if i != j) += the line's length in mm.  W is float64 [L+1][L+1], may be NULL.  The length is the column-0
 *              sum of the LINE STATISTICS above (the same float64 terms, r = volres), kept in float64 and NOT rounded to float32.
 *              The order of both sums is free (lanes sum a line, atomic adds sum a cell): against sequential float64 sums
 *              |W - W_seq| <= (n_max + m) * 2^-52 * W_seq per cell, n_max the points of the longest of the cell's m lines.  A
 *              cell with C = 0 is exactly 0.  When W is NULL no length is computed and volres may be NULL.
 *   assign     int32 [nlines][2] = (a, b) in line order (first end, last end), (0, 0) for empty lines; may be NULL.
 * *n_lines_dev (int64, device) = the number of lines counted (#{npts >= 1}), or -1 for INVALID npts, and then nothing is added and
 * assign is not written.  flags: 0, or FIB_CONNECTOME_ACCUMULATE to add to what C and W hold (without it the call zero-fills them
 * first, for an INVALID npts too).  Integer counts make C independent of batch and arrival order (same bytes). */
#define FIB_CONNECTOME_ACCUMULATE 0x100
/* rois, roibits: device pointers.  nroi 0..32.  Asynchronous on `stream`. */
int fibd_str_roi_pack(const uint8_t *rois, int nroi, int64_t nvox, uint32_t *roibits, void *stream);
/* bytes of device scratch fibd_str_select / fibd_str_gather / fibd_str_connectome need for nlines lines (three int64 per line and
 * per block of the scan: each line's first point, its place among the kept lines and among their points); 8-byte aligned */
int fibd_str_select_work_size(int64_t nlines, size_t *bytes);
/* All three: every array is a device pointer; asynchronous on `stream`, no allocation and no synchronisation inside. */
int fibd_str_select(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz, const uint32_t *roibits,
                    uint64_t visit_all, uint64_t visit_none, uint64_t end_any, uint64_t end_both, int32_t min_npts, int32_t max_npts,
                    uint8_t *keep, uint32_t *hits, int64_t *counts, void *work, size_t work_bytes, void *stream);
int fibd_str_gather(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, const uint8_t *keep, const float *scalars,
                    int nscalars, int64_t cap_lines, int64_t cap_points, float *xyz_out, int32_t *npts_out, int64_t *index_out,
                    float *scalars_out, int64_t *counts, void *work, size_t work_bytes, void *stream);
int fibd_str_connectome(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz, const float volres[3],
                        const int32_t *labels, const int32_t *remap, int64_t nremap, int nnodes, int flags, uint32_t *cmat, double *wmat,
                        int32_t *assign, int64_t *n_lines_dev, void *work, size_t work_bytes, void *stream);

/* ------------------------------------------------------------------------------------ */
/* Bundle tools: resampling, MDF assignment, centroids (NOT in the reference)            */
/* ------------------------------------------------------------------------------------ */
/* What a tractography user does right after "I have a million lines": bring every line to the same number of points, compare it with
 * a set of model bundles, and work per bundle.  Inputs of RESAMPLE are PACKED LINES exactly as for the tract maps above; npts is
 * INVALID as defined there.  These definitions are this project's own; they are the contract.  r = volres as float32; every
 * operation below is IEEE float64 on the float32 inputs, rounded one by one, NO fused multiply-add.
 *
 * RESAMPLE gives every line K points (2 <= K <= 256, else FIB_ERR_UNSUPPORTED), equidistant in arc length in mm: out float32
 * [nlines][K][3].  For a line with points p_0 .. p_{n-1}:
 *   l_i (i = 0 .. n-2)  the length of segment i: exactly the term of the LINE STATISTICS length above,
 *                       sqrt(((x1-x0)*r_x)*((x1-x0)*r_x) + ((y1-y0)*r_y)*((y1-y0)*r_y) + ((z1-z0)*r_z)*((z1-z0)*r_z)), squares added left to right;
 *   c_0 = 0, c_{i+1} = c_i + l_i, T = c_{n-1}.  The order of these additions is free on the device (any-order float64 prefix sums
 *                       are each within (n-1) * 2^-53 * T of the exact ones), but ONE set of c serves both the search and the
 *                       interpolation below.  (The shipped kernel adds them in sequence, which is what makes c non-decreasing and
 *                       gives every output row exactly one owner.)
 *   row 0 is a bit copy of p_0 and row K-1 a bit copy of p_{n-1}.  For 0 < k < K-1:
 *                       t_k = (T * (double)k) / (double)(K-1);  j = the largest i <= n-2 with c_i <= t_k;
 *                       a = (t_k - c_j) / (c_{j+1} - c_j) clamped to [0, 1], or 0 if that denominator is not > 0;
 *                       each component is (double)p_j + a * ((double)p_{j+1} - (double)p_j), rounded to float32 once.
 *   n = 1: all K rows are bit copies of p_0.  n = 0, or n >= 2 and T not finite (a NaN or +-Inf coordinate): every component of all
 *   K rows is the quiet NaN 0x7FC00000, rows 0 and K-1 included.  Coordinates of +-1e30 make T huge but finite: legal.  Duplicated
 *   consecutive points (the tracer emits the seed twice) are segments of length 0 that own no row; a line of equal points gives copies.
 *   flip, uint8 [nlines] or NULL: for a line whose flag is non-zero, output row k holds what row K-1-k would have held, bit for bit.
 *   A line's result depends on the line alone -- not on its index, its neighbours or the batch it arrives in: two runs, or the same
 *   lines in another order, give the same bytes per line; the host form equals the device form byte for byte.
 *   *status_dev (int64, device) = the number of lines written (nlines), or -1 for an INVALID npts, and then nothing is written to out.
 *
 * ASSIGN: the MDF (mean direct-flip) distance of every line to every model bundle, the nearest model and the orientation.  lines
 * float32 [nlines][K][3] and models float32 [nmodels][K][3], both in voxel coordinates (K >= 1; 1 <= nmodels < 2^24).  For a pair
 * (a, m):  d_dir = (sum_{k=0}^{K-1} |(a_k - m_k) o r|) / K,  d_flip = the same sum with m_{K-1-k};  each norm is the term l above on
 * the pair of points (a_k first: (m - a) is NOT used; the three components are ((double)a_c - (double)m_c) * (double)r_c); the sum
 * runs over k SEQUENTIALLY from 0 in float64, then one float64 division by (double)K.  f = (d_flip < d_dir), d = f ? d_flip : d_dir.
 * A NaN d compares as larger than everything.  Per line:
 *   label int32   the first m that attains the minimum d (float64, strict <) if that d <= (double)thresh_mm, else -1; -1 when every
 *                 d is NaN (and for a NaN thresh_mm);
 *   dist float32  the minimum d rounded to float32 once, written whatever the threshold says; NaN if every d is NaN;
 *   flip uint8    f of the pair that gives dist (whatever the threshold says), 0 if every d is NaN;
 *   dist_all      float32 [nlines][nmodels], every d rounded once; may be NULL.
 * Every NaN that dist and dist_all hold is the quiet NaN 0x7FC00000.
 * The k-sum is sequential and every term an IEEE float64 value: everything this call writes is BIT-IDENTICAL to a NumPy restatement.
 *
 * CENTROIDS: per-bundle sums of oriented lines, so that assign -> centroids -> assign is a refinement loop that stays on the device.
 * For every line with 0 <= label < nmodels:  counts[label] += 1 (uint32, wraps at 2^32) and sums[label][k][c] += (double) of the line's
 * row (flip ? K-1-k : k), component c; sums float64 [nmodels][K][3].  Other labels contribute nothing; flip may be NULL (all 0).  flags:
 * 0, or FIB_CENTROIDS_ACCUMULATE to add to what the outputs hold (without it the call zero-fills them first).  The order of the
 * float64 additions is free: against the sequential sum |sums - sums_seq| <= (N_b - 1) * 2^-52 * sum|t| per cell, N_b the lines of
 * the bundle; a bundle without lines is exactly 0 (on zero-filled outputs).  counts are exact and independent of batch and order. */
#define FIB_CENTROIDS_ACCUMULATE 0x100
/* All three: every array is a device pointer; asynchronous on `stream`, no allocation and no synchronisation inside.  work is sized by
 * fibd_str_work_size(nlines). */
int fibd_str_resample(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, const float volres[3], int K,
                      const uint8_t *flip, float *out, int64_t *status_dev, void *work, size_t work_bytes, void *stream);
int fibd_str_assign(const float *lines, int64_t nlines, int K, const float *models, int nmodels, const float volres[3],
                    float thresh_mm, int32_t *label, float *dist, uint8_t *flip, float *dist_all, void *stream);
int fibd_str_centroids(const float *lines, int64_t nlines, int K, const int32_t *label, const uint8_t *flip, int nmodels,
                       int flags, double *sums, uint32_t *counts, void *stream);

/* ------------------------------------------------------------------------------------ */
/* Tractogram weights: fit line weights to fixel amplitudes (NOT in the reference)       */
/* ------------------------------------------------------------------------------------ */
/* A line count depends on seeding density, bundle length and curvature; a WEIGHT per line, chosen so that the weighted track density
 * of every fibre population matches that population's amplitude, does not (what SIFT2, COMMIT and LiFE are for).  These definitions
 * are this project's own; they are the contract.  The fit is a fixed number of ISRA steps (the multiplicative iteration for
 * non-negative least squares), NOT SIFT2's line search: no decision depends on the data.
 *
 * INPUTS.  PACKED LINES exactly as for the tract maps above (xyz float32 [npoints][3], 1-based voxel coordinates, 4-byte alignment
 * suffices; npts int32 [nlines]); the VOXEL OF A POINT, the INSIDE test and lin(v) are the ones defined there; npts is INVALID as
 * defined there.  The PEAK FIELD is the arrays fibd_stream_field takes: ovec[k] planar float32 [3][nvox], f[k] float32 [nvox],
 * k < nvec <= 3 (host arrays of nvec device pointers); mask uint8 [nvox] or NULL.  nvec * nvox < 2^31 and npoints < 2^31, else
 * FIB_ERR_UNSUPPORTED (fixel ids are int32).  f_thresh >= 0 (amplitudes are positive), else FIB_ERR_INVALID.
 *
 * FIXEL.  phi = k * nvox + lin(v).  It EXISTS iff the mask is NULL or non-zero at v, f[k][v] is finite and > f_thresh, and the three
 * components of ovec[k][v] are finite and not all zero.  The directions are taken as unit vectors; they are not renormalised.
 *
 * FIXEL OF A POINT.  A line with npts >= 2 has a tangent at every point: t_i = p_{i+1} - p_{i-1}, one-sided at the two ends
 * (t_0 = p_1 - p_0, t_{n-1} = p_{n-1} - p_{n-2}), float32, component by component.  For every existing fixel k of the point's voxel
 *   d_k = (t_x*u_x + t_y*u_y) + t_z*u_z       float32, every operation rounded on its own, no fused multiply-add.
 * The point takes the k with the largest |d_k|: the candidates are compared in the order k = 0, 1, 2 with a strict >, so a tie goes
 * to the smallest k and a NaN d_k is never taken.  The point KEEPS that fixel iff
 *   d_k*d_k >= cos2 * ((t_x*t_x + t_y*t_y) + t_z*t_z)      by the same float32 rules; cos2 is a float32 the caller computes
 * (cos^2 of the angle threshold).  A point is UNASSIGNED (fixel id -1) if it is outside, has a non-finite or all-zero tangent,
 * belongs to a line with npts < 2, or has no kept fixel.  n_{s,phi} = the number of points of line s assigned to phi.  Counts stand
 * for lengths: the input must have a UNIFORM STEP (fibd_stream_run, fibd_prob_run and fibd_str_resample write uniform steps).
 *
 * FIXED POINT, so that every sum is an integer sum.  A weight is a uint32 q in units of 2^-20: w = q * 2^-20, 0 <= w < 4096.  Every
 * line starts at q = 2^20, or at the caller's q0.
 *   a_scale = 2^30 / max f       float64; the max over the EXISTING fixels (a maximum has no order); 0 when no fixel exists
 *   Aq_phi  = rint(f_phi * a_scale) as uint64 (f widened to float64, one product, rint ties to even); 0 where no fixel exists
 *   TDq_phi = sum_s q_s * n_{s,phi}    uint64, by vector atomic adds on uint64 in any order; one add covers a run of consecutive
 *             points of a line in the same fixel (runs are cut every 16 points of a line)
 *   N_s = sum_i Aq_{phi(i)} over the assigned points of line s, once;  D_s = sum_i TDq_{phi(i)}, every iteration; both uint64
 *   mu  = (double(sum Aq) / a_scale) / (double(sum TDq0) * 2^-20)   from the initial weights, float64, fixed for the whole call;
 *         0 when no fixel exists or sum TDq0 = 0
 * UPDATE (ISRA), float64, every operation rounded on its own, integer-to-double conversions round to nearest:
 *   w' = ((q * 2^-20) * (double(N_s) / a_scale)) / (mu * (double(D_s) * 2^-20))
 *   q' = rint(min(w', 4096 - 2^-20) * 2^20)
 * A line with no assigned point, or with D_s = 0, gets q' = 0.  niter is fixed.  The sums are exact while every TDq < 2^44 and every
 * line has at most 2^20 points; an update adds to `overflow` the number of ASSIGNED POINTS whose gathered TDq is >= 2^44 (summed over
 * the iterations), and beyond that the uint64 sums wrap as uint64 sums do -- never silently: the Python tier raises on overflow != 0.
 *
 * OUTPUTS.  q uint32 [nlines]; weights float32 [nlines] = float32(q) * 2^-20 (one rounding); td float32 [nvec][nvox] =
 * float32((double(TDq) * 2^-20) * mu), the fitted density on the scale of f, 0 where no fixel exists; cost float64 [niter + 1],
 * cost[j] = sum_phi (mu * (double(TDq) * 2^-20) - double(Aq) / a_scale)^2 after j updates (a term with Aq = 0 takes 0 for the
 * quotient).  Everything but cost is bit-exact.  The ORDER of the cost sum is free: it is within n * 2^-53 * sum|t| of the exact sum
 * of its n terms t; the kernels add it in a fixed order, so two runs, and the device and host forms, give the same bytes.
 * STATE: FIB_FIXEL_STATE_SLOTS slots of 8 bytes in device memory:
 *   [0] a_scale (float64)  [1] mu (float64)  [2] sum Aq  [3] sum TDq0  [4] the bits of max f  [5] points unassigned, -1 for an
 *   INVALID npts  [6] lines without an assigned point (empty lines included)  [7] lines at the clamp (q = 2^32 - 1)
 *   [8] lines at q = 0  [9] overflow  [10..15] reserved.   [7], [8] describe the final q.
 * INVALID npts (device forms): slot [5] is -1, no id is written, nothing is added and no weight is updated (q = q0). */
#define FIB_FIXEL_STATE_SLOTS 16
#define FIB_FIXEL_COST_WORK_BYTES 2048
/* All: every array is a device pointer (ovec / f: host arrays of nvec device pointers), asynchronous on `stream`, no allocation and
 * no synchronisation inside, no workgroup waits for another.  `work` of the line entries: fibd_str_work_size(nlines) bytes.
 * quantise: zero-fills state, then writes slots [0], [2], [4] and aq uint64 [nvec * nvox]. */
int fibd_fixel_quantise(int32_t nvec, int64_t nvox, const float *const *ovec, const float *const *f, const uint8_t *mask, float f_thresh,
                        uint64_t *aq, void *state, void *stream);
/* assign: ids int32 [npoints]; counts int64 [2] = {points unassigned or -1, lines without an assigned point} (state slots [5], [6]) */
int fibd_fixel_assign(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz, int32_t nvec,
                      const float *const *ovec, const float *const *f, const uint8_t *mask, float f_thresh, float cos2, int32_t *ids,
                      int64_t *counts, void *work, size_t work_bytes, void *stream);
/* td: zero-fills tdq uint64 [nfixels] and scatters q (uint32 [nlines]) along the ids; an id outside [0, nfixels) adds nothing */
int fibd_fixel_td(const int32_t *ids, const int32_t *npts, int64_t nlines, int64_t npoints, const uint32_t *q, int64_t nfixels,
                  uint64_t *tdq, void *work, size_t work_bytes, void *stream);
/* mu: slots [3] and [1] from the TDq of the initial weights */
int fibd_fixel_mu(const uint64_t *tdq, int64_t nfixels, void *state, void *stream);
/* update: one ISRA step of q in place; first != 0: N_s is made and kept in nline (uint64 [nlines]), else read from it */
int fibd_fixel_update(const int32_t *ids, const int32_t *npts, int64_t nlines, int64_t npoints, const uint64_t *aq, const uint64_t *tdq,
                      int64_t nfixels, int first, void *state, uint64_t *nline, uint32_t *q, void *work, size_t work_bytes, void *stream);
/* cost: one float64 in device memory; work: FIB_FIXEL_COST_WORK_BYTES */
int fibd_fixel_cost(const uint64_t *aq, const uint64_t *tdq, int64_t nfixels, const void *state, double *cost, void *work, size_t work_bytes,
                    void *stream);
/* output: weights, td and slots [7], [8] from the final q and TDq */
int fibd_fixel_output(const uint32_t *q, int64_t nlines, const uint64_t *tdq, int64_t nfixels, void *state, float *weights, float *td,
                      void *stream);
/* fit: everything behind quantise and assign on ids that stay resident -- the first scatter, mu, cost[0], then niter times update,
 * scatter, cost -- and output.  q holds the start weights and receives the final ones.  work: fibd_fixel_fit_work_size(nlines). */
int fibd_fixel_fit_work_size(int64_t nlines, size_t *bytes);
int fibd_fixel_fit(const int32_t *ids, const int32_t *npts, int64_t nlines, int64_t npoints, const uint64_t *aq, int64_t nfixels, int niter,
                   uint32_t *q, float *weights, float *td, double *cost, void *state, uint64_t *tdq, uint64_t *nline, void *work,
                   size_t work_bytes, void *stream);
/* the whole fit on device arrays: quantise, assign, fit, with ids, Aq, TDq and N_s in the caller's work area
 * (fibd_str_weights_work_size bytes: 4 B a point, 16 B a fixel, 16 B a line and the scan).  q0 uint32 [nlines] or NULL. */
int fibd_str_weights_work_size(int64_t nlines, int64_t npoints, int32_t nvec, int64_t nvox, size_t *bytes);
int fibd_str_weights(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz, int32_t nvec,
                     const float *const *ovec, const float *const *f, const uint8_t *mask, float f_thresh, float cos2, int niter,
                     const uint32_t *q0, uint32_t *q, float *weights, float *td, double *cost, void *state, void *work, size_t work_bytes,
                     void *stream);

/* ------------------------------------------------------------------------------------ */
/* Probabilistic tracking: ODF-sampled streamlines (NOT in the reference)                */
/* ------------------------------------------------------------------------------------ */
/* Streamlines whose direction at every step is DRAWN from the ODF of the voxel ahead, restricted to a cone around the direction of
 * travel.  These definitions are this project's own; they are the contract.  Wherever a sum is formed it is an integer sum, and every
 * float32 operation is rounded on its own (no fused multiply-add): the output is BIT-IDENTICAL to a NumPy restatement.
 *
 * DIRECTIONS.  U[i], i < nvert: the first half of an ODF sphere's vertices (the vertices gqi_rec reports peaks on), float32 [nvert][3].
 * 1 <= nvert <= 512, else FIB_ERR_UNSUPPORTED.
 *
 * WEIGHT TABLE, uint16 [nvox][pitch], pitch = fib_prob_row_pitch(nvert) = 64 * ceil(nvert / 64), padding zero, 16-byte aligned.  Built
 * from an ODF float32 [nvert][nvox] planar (what fibd_odf_rec writes and MRI.vol[nx,ny,nz,nvert] is).  Per voxel, o_i its amplitudes:
 *   m = the minimum of the o_i that are not NaN if subtract_min, else 0;   w_i = o_i - m if that is > 0, else 0 (a NaN fails the test);
 *   wmax = max_i w_i.  If wmax is 0 or not finite, or the voxel's mask byte is 0 (mask uint8 [nvox] or NULL), the row is all zero.
 *   Otherwise t_i = w_i / wmax (one IEEE float32 division), q_i = 0 where t_i < pmf_thresh, else (uint16) floorf(t_i * 65535.0f).
 * The table carries the mask: a zero row ends a line.
 *
 * CONE.  c(j,i) = (U[j].x*U[i].x + U[j].y*U[i].y) + U[j].z*U[i].z, every product and sum rounded to float32 on its own.
 *   allow(j,i) = |c(j,i)| >= cosang_thresh,   same(j,i) = c(j,i) > 0.   cosang_thresh must be > 0 (an angle below 90 degrees), else
 *   FIB_ERR_INVALID: the cone is the only bend limit.
 *
 * RANDOM NUMBERS.  The generator of fibd_stream_trace_lcm, h(line, k) = splitmix64(rng_seed ^ splitmix64(line * 0xD1342543DE82EF95 + k)),
 * here its top 32 bits: u = h >> 32.  A draw from weights q with Q = sum q_i > 0 is r = (u * Q) >> 32 in 64-bit integers, and the pick
 * is the first i whose running integer sum exceeds r.  Q < 2^25: nothing overflows, and a unit of weight owns at least 128 values of u.
 * Known answers for h >> 32: (rng_seed 0, line 0, k 0) 2802244911; (1234, 5, 2) 1460108722; (2^63 + 1, 10^6, 141) 2790284181.
 *
 * A LINE.  line = i * nsub + sub for the i-th seed of the list (seeds: 0-based column-major voxel indices; one outside the volume has no
 * points); k counts the line's draws from 0.  pos0 = the seed voxel (1-based, as float32) + sublist[sub].  If the seed voxel's row has
 * Q = 0 the line has no points.  Otherwise j0 is drawn from the whole row (no cone), and then for s0 in (+1, -1), each pass starting from
 * pos = pos0, j = j0, s = s0:
 *   1. vec = s * U[j] (exact); nxt = pos + vec * step_size: multiply, then add, each rounded.
 *   2. vox = rint(nxt), ties to even.  nxt not finite or vox outside 1..n: the pass ends.
 *   3. q'_i = allow(j,i) ? table[vox][i] : 0.  Q' = sum q'_i = 0: the pass ends and NO DRAW IS CONSUMED.
 *   4. i* is drawn from q'; s = same(j,i*) ? s : -s; j = i*.
 *   5. pos is emitted and npts incremented; npts > len_max: the pass ends; otherwise pos = nxt.
 * (the shape of stream.jl:625-690: a point is saved only if its successor step is valid, the seed is emitted once per direction, npts is
 * shared by both directions.)  Output order [fwd_N .. fwd_1, bwd_1 .. bwd_M], at most len_max + 2 points; a line is kept iff
 * npts >= len_min.  No smoothing and no separate bend test: a direction is always a vertex and the cone is the bend limit.
 * Results depend on the arguments and rng_seed only -- not on scheduling, the launch shape or how often the call is made. */
typedef struct fib_prob_plan fib_prob_plan;
/* the row pitch of the weight table in elements; 0 for an unsupported nvert */
int fib_prob_row_pitch(int nvert);
/* odf, mask (or NULL) and table are device pointers; asynchronous on `stream`, no allocation and no synchronisation inside.  A transpose
 * through LDS: 4 * nvert bytes read and 2 * pitch written per voxel. */
int fibd_prob_table(const float *odf, const uint8_t *mask, int64_t nvox, int nvert, int subtract_min, float pmf_thresh, uint16_t *table,
                    void *stream);
/* the plan holds U and the bit rows of allow and same (nvert x pitch bits each) on `device`; vertices is host memory [nvert][3] */
int fib_prob_plan_create(int device, const float *vertices, int nvert, float cosang_thresh, fib_prob_plan **plan);
void fib_prob_plan_destroy(fib_prob_plan *plan);
/* bytes of device scratch fibd_prob_run needs for nlines = nseed * nsub lines (24 per line and the scan's block totals); 8-byte aligned.
 * After a call, also one that returned FIB_ERR_CAPACITY, work begins with int32 [nlines][2] = {nfwd, nbwd} of EVERY line in (seed, sub)
 * order, those dropped by len_min included (their sum is the line's npts). */
int fibd_prob_work_size(int64_t nlines, size_t *bytes);
/* Trace and pack into caller-provided device buffers, the layout of fibd_stream_run: npts int32 [lines_cap], seed_index int64
 * [lines_cap] (= seed * nsub + sub), xyz float32 [3 * points_cap], kept lines in (seed, sub) order, one after the other.  No row of
 * len_max + 2 points is reserved per line: a first pass traces and counts, a scan applies len_min and places every kept line, a second
 * pass replays the kept lines (the generator is counter-based) and stores every point at its final place.  *nlines / *npoints receive the
 * totals (host); when they exceed the capacities the call returns FIB_ERR_CAPACITY after the first pass and has written NOTHING to the
 * three buffers.  plan's device must be current; table, seeds, sublist and work are device pointers; synchronises `stream`. */
int fibd_prob_run(const fib_prob_plan *plan, int nx, int ny, int nz, int32_t len_min, int32_t len_max, float step_size, const uint16_t *table,
                  const int64_t *seeds, int64_t nseed, const float *sublist, int32_t nsub, uint64_t rng_seed, int32_t *npts,
                  int64_t *seed_index, int64_t lines_cap, float *xyz, int64_t points_cap, int64_t *nlines, int64_t *npoints, void *work,
                  size_t work_bytes, void *stream);

/* ------------------------------------------------------------------------------------ */
/* Volume resampling: a volume moved through an Xform (NOT in the reference)             */
/* ------------------------------------------------------------------------------------ */
/* Volumes are planar [nframes][nz][ny][nx], x fastest (MRI.vol in Fortran order), 32-bit elements.  Voxel coordinates are 0-BASED
 * ARRAY INDICES, the convention of .lta and FSL vox2vox matrices; the tract code's 1-based point coordinates are not involved.  These
 * definitions are this project's own; they are the contract.
 *
 * PULL-BACK.  For the output voxel o = (i, j, k), taken as float32 values, p = xfm_point(M, i, j, k): the arithmetic of fib_xfm_apply
 * (float32, every multiply and add rounded on its own, IEEE division, the projective last row honoured).  M = out2in is the
 * OUTPUT -> INPUT matrix, row-major float[16]; the Python layer makes it as float32(inv(float64(xfm.vox2vox))), rounded once.
 *
 * INSIDE.  A sample is inside iff for every component 0 <= rint(p_c) <= n_c - 1 (ties to even), tested on the float value before any
 * conversion to an integer: NaN fails, -0.0 passes.  The same rule for both interpolations (the tract maps' "voxel of a point" moved
 * to 0-based; what FreeSurfer's sampler does).  Otherwise the output word is `outside_bits`, in every frame.
 *
 * FIB_VOL_NEAREST.  The 32-bit word at voxel rint(p) is copied untouched: float32 (NaN payloads included), int32 and uint32 volumes
 * go through the same kernel.  The fill is a 32-bit pattern (declared int32_t: the bit pattern of a float32 or uint32 fill).
 *
 * FIB_VOL_TRILINEAR, float32 only.  Per component i0 = floor(p_c), f = p_c - floor(p_c) (one rounded float32 subtraction: it may
 * round to 1.0 for a tiny negative p_c), g = 1 - f, and the neighbour indices i0 and i0 + 1 are each CLAMPED into [0, n_c - 1].  Then,
 * without fused multiply-add and in exactly this order,
 *   c00 = gx*v000 + fx*v100,  c10 = gx*v010 + fx*v110,  c01 = gx*v001 + fx*v101,  c11 = gx*v011 + fx*v111   (v_xyz, x the first digit)
 *   c0 = gy*c00 + fy*c10,  c1 = gy*c01 + fy*c11,  out = gz*c0 + fz*c1.
 * f == 0 and the clamped shell are not special-cased (g*v + f*v is not v in float32).  Consequences, documented and not fixed: an Inf
 * neighbour with weight 0 gives NaN; NaN voxels propagate.
 * Every frame uses the same p, indices and weights.
 *
 * fibd_vol_xform: vol and out are device pointers (4-byte alignment suffices: views into a larger buffer); asynchronous on `stream`,
 * no allocation and no synchronisation inside.  One thread per output voxel, 64-bit element offsets in and out.  FIB_ERR_INVALID:
 * non-positive sizes, an unknown interp, NULL pointers, ANY overlap of vol and out (a gather has no in-place form); a dimension above
 * 2^24 is FIB_ERR_UNSUPPORTED. */
#define FIB_VOL_NEAREST 0
#define FIB_VOL_TRILINEAR 1
int fibd_vol_xform(const float out2in[16], const void *vol, int nxi, int nyi, int nzi, int nframes, int interp, int32_t outside_bits,
                   void *out, int nxo, int nyo, int nzo, void *stream);

/* ------------------------------------------------------------------------------------ */
/* Non-linear warps: a displacement field applied to points and volumes, and inverted    */
/* (NOT in the reference)                                                                 */
/* ------------------------------------------------------------------------------------ */
/* The non-linear sibling of fib_xfm_apply and of the volume resampling above, with their conventions: float32, every multiply and add
 * rounded on its own (no fused multiply-add), planar volumes [nframes][nz][ny][nx], 0-based voxel indices for volumes.  These
 * definitions are this project's own; they are the contract.
 *
 * FIELD.  A displacement field is a float32 volume of 3 frames on a grid of its own (nx, ny, nz and the vox2ras of that grid, RAS mm):
 * frame c at voxel (i, j, k) is component c of the displacement IN MM, RAS.  It defines phi(x) = x + d(x) for a RAS point x of the
 * field's space A; phi(x) is a RAS point of the other space B.  Points travel A -> B; a volume is pulled back, so a volume of B lands on
 * a grid of A.  Device form: float4 [nvox] = (dx, dy, dz, 0), 16-byte aligned, made once by fibd_warp_pack from the planar field (one
 * aligned 16-byte gather per neighbour).  The host forms take the planar field and pack it themselves.
 *
 * SAMPLE S(q), q in float32 field-voxel coordinates (0-based).  If any q_c is NaN all three results are NaN.  Otherwise per component,
 * with n_c the field's size: qc = q_c < 0 ? 0 : (q_c > n_c - 1 ? n_c - 1 : q_c) -- beyond the grid the EDGE displacement continues
 * (+-Inf clamp, -0.0 passes; no zero outside and no inside test: a jump to zero at the border makes the inversion below oscillate in
 * the border voxels, the clamped rule converges) -- then i0 = (int)floor(qc), f = qc - floor(qc) (one rounding), g = 1 - f,
 * i1 = min(i0 + 1, n_c - 1).  Each displacement component is then interpolated between the 8 neighbours in the order and with the
 * roundings of FIB_VOL_TRILINEAR above (x pairs, then y, then z); f == 0 is not special-cased.
 *
 * WARP OF A POINT p (any 3-vector of caller coordinates) with three row-major float[16] matrices, each applied with fib_xfm_apply's
 * arithmetic (xfm_point: the projective row and the IEEE division included):
 *   x = xfm_point(to_ras, p),  q = xfm_point(to_field, p),  d = S(q),  y_c = x_c + d_c (one rounding each),  p' = xfm_point(from_ras, y).
 * to_ras takes caller coordinates to RAS of space A, to_field to the field's voxels, from_ras takes RAS of space B to the caller's
 * output coordinates.
 *
 * WARP OF A VOLUME.  For the output voxel (i, j, k), taken as floats, p' is the warp of that point; `vol` is then sampled at p' exactly
 * as fibd_vol_xform samples at its p: the INSIDE rule, FIB_VOL_NEAREST / FIB_VOL_TRILINEAR, outside_bits, every frame with the same p'.
 *
 * INVERSE.  For the output voxel (i, j, k) of a grid in space B: y = xfm_point(out_to_ras, i, j, k), x = y; niter times
 * q = xfm_point(ras_to_field, x), d = S(q), x_c = y_c - d_c; then inv_c = x_c - y_c (three planar frames on the output grid: the field
 * of phi^-1, mm RAS) and, once more, d = S(xfm_point(ras_to_field, x)), r_c = (x_c + d_c) - y_c, err = max_c |r_c| (a NaN in any r_c
 * gives NaN).  niter = 0 gives inv = 0 and err = the displacement at y.  The kernel leaves the loop when an iterate repeats bit for bit
 * (every later one is the same) and uses no other stopping rule.  The iteration converges where the field's Jacobian norm is below 1;
 * err is the caller's check where the field folds.
 *
 * The four device entries are asynchronous on `stream`, allocate nothing and do not synchronise; element offsets are 64-bit.
 * FIB_ERR_INVALID: NULL pointers (err of fibd_warp_invert may be NULL), non-positive sizes (npoints == 0 does nothing), niter < 0, an
 * unknown interp, a packed field that is not 16-byte aligned, ANY overlap of vol and out; a dimension above 2^24 is
 * FIB_ERR_UNSUPPORTED.  fibd_warp_points: out == xyz is allowed (other overlaps are not) and points need only be 4-byte aligned, as
 * for fibd_xfm_apply; volumes, inv and err need only be 4-byte aligned. */
int fibd_warp_pack(const float *disp, int nx, int ny, int nz, void *packed, void *stream);
int fibd_warp_points(const void *packed, int nx, int ny, int nz, const float to_ras[16], const float to_field[16], const float from_ras[16],
                     const float *xyz, float *out, int64_t npoints, void *stream);
int fibd_warp_volume(const void *packed, int nx, int ny, int nz, const float to_ras[16], const float to_field[16], const float from_ras[16],
                     const void *vol, int nxi, int nyi, int nzi, int nframes, int interp, int32_t outside_bits, void *out, int nxo, int nyo,
                     int nzo, void *stream);
int fibd_warp_invert(const void *packed, int nx, int ny, int nz, const float out_to_ras[16], const float ras_to_field[16], int niter,
                     float *inv, float *err, int nxo, int nyo, int nzo, void *stream);

/* ------------------------------------------------------------------------------------ */
/* Registration: rigid / affine alignment by normalised mutual information               */
/* (NOT in the reference)                                                                 */
/* ------------------------------------------------------------------------------------ */
/* The conventions of "Volume resampling": planar volumes with x fastest, 0-based voxel indices, float32 with every multiply and add
 * rounded on its own, matrices derived in float64 from float32 fields and rounded to float32 once.  These definitions are this
 * project's own; they are the contract, tests/register_ref.py restates them in NumPy, and everything up to the histogram is held to
 * that bit for bit (a joint histogram is an integer count).
 *
 * PYRAMID (fibd_vol_halve).  The output size is ceil(n_c / 2) per axis.  Output voxel (i, j, k) is the float32 sum of the EXISTING
 * input voxels (2i + dx, 2j + dy, 2k + dz), dx, dy, dz in {0, 1}, started from +0 and added with dz outermost and dx innermost,
 * divided by their count as a float32 (a block cut by an odd size has fewer than 8).  Level-l voxel x sits at level-0 voxel
 * 2^l x + (2^l - 1) / 2: the matrix D_l.
 *
 * RANGE (fibd_vol_range), per frame, 16 bytes { float lo, hi, scale; uint32_t nfinite }: lo and hi are the smallest and largest FINITE
 * value by the ordered-uint key of "Brain mask" (so -0 < +0 and the result does not depend on the order of the reduction),
 * scale = float32(nbins) / (hi - lo), one float32 division, nfinite the number of finite values.  Without a finite value lo = hi = 0 and
 * scale = NaN; hi == lo gives scale = +Inf.  The device form writes that and returns; the drivers refuse it ("constant volume",
 * FIB_ERR_INVALID).
 *
 * BIN.  t = (v - lo) * scale, two float32 roundings.  A NaN t (a NaN v, or Inf * 0) has no bin; otherwise
 * bin(v) = clamp(floor(t), 0, nbins - 1), clamped as a float before the conversion (so v = hi, and +-Inf, land in an end bin).
 *
 * JOINT HISTOGRAMS (fibd_reg_hist).  One fixed volume, the frames of a moving series and njobs jobs; job j is (moving frame
 * job_frame[j], out2in matrix job_out2in + 16 j: FIXED voxel -> MOVING voxel, row-major float[16]).  For every fixed voxel (i, j, k)
 * whose value a is finite: p = xfm_point(M_j, i, j, k) with fib_xfm_apply's arithmetic; the INSIDE rule of "Volume resampling" on p
 * against the moving size -- outside samples are SKIPPED, not filled; v = the FIB_VOL_TRILINEAR value of the frame at p, in that
 * section's operation order; a sample without a bin on either side is skipped; else hist[j][bin_fixed(a)][bin_moving(v)] += 1, with the
 * fixed volume's range and the range of frame job_frame[j].  hist is uint32 [njobs][nbins][nbins], zeroed by the call; every sum is an
 * integer sum, so the result does not depend on the launch shape.  nbins in FIB_REG_MIN_BINS .. FIB_REG_MAX_BINS.  job_frame and
 * job_out2in are HOST arrays (copied to the head of `work` on the stream before the launch: they may be reused on return); the ranges
 * are DEVICE memory as fibd_vol_range leaves them.  The kernel is asynchronous on `stream` and nothing is allocated; the copy of the job
 * table (80 bytes a job) comes from pageable host memory, which the runtime stages before the call returns and for which it may wait for
 * earlier work of `stream`: no other wait is inside.  `work` is
 * 8-byte aligned, fibd_reg_hist_work_size bytes.  The launch's third dimension is the job: one launch carries the 2 dof candidates of
 * every live frame of a series.  FIB_ERR_INVALID: NULL pointers, non-positive sizes, nbins or njobs out of range, a frame index outside
 * [0, nframes), a short workspace, misaligned pointers, ANY overlap of hist or work with a volume, a range or each other; a dimension
 * above 2^24 is FIB_ERR_UNSUPPORTED.
 *
 * MATRICES (fib_reg_matrix; host, float64).  theta: dof 6 = (tx, ty, tz mm; rx, ry, rz degrees); dof 12 adds (ln sx, ln sy, ln sz;
 * hxy, hxz, hyz).  A = [Rz Ry Rx Sh S | t] with the right-handed rotations about x, y, z, Sh unit upper-triangular with the three
 * shears and S = diag(exp(.)); G(theta) = C A C^-1 with C the translation to c = fixed.vox2ras (n - 1) / 2; G maps FIXED RAS -> MOVING
 * RAS.  out2in_l = float32(inv(V_mov D_l) G (V_fix D_l)).  G (or NULL) receives G itself, row-major double[16]; out2in may be NULL.
 *
 * COST (fib_reg_nmi; host, float64).  N = sum hist; cost = -Inf when N == 0 or N < min_overlap * nfinite_fixed (the finite fixed voxels
 * of that level); H(c) = ln N - (sum c ln c) / N over the non-zero cells in row-major order; cost = (H(rows) + H(cols)) / H(joint), -Inf
 * when H(joint) == 0.
 *
 * PATTERN SEARCH (fib_reg_search_*; host, float64, HIP-free: the caller evaluates the histograms).  Levels run from the coarsest,
 * levels - 1, to 0; levels = 0 means fib_reg_levels: 1 + the largest l <= 3 at which both volumes keep every dimension >= 8.  Steps at
 * level l: h = 2^l min(fixed.volres), R = 0.5 sqrt(sum (n_c res_c)^2) / sqrt(3); h mm, degrees(h / R) and h / R for translations,
 * rotations and scale / shear.  A stage (a level, the first 6 or all 12 parameters) starts with ONE job, the cost of the current theta
 * at that level; then every iteration hands out the 2 n candidates theta +- step_i e_i (index 2 i: +, 2 i + 1: -), takes the first
 * maximum of their costs, moves there iff it is strictly greater than the current cost, else halves all steps.  A stage ends after
 * halvings + 1 failures or maxit iterations.  dof 12 runs the 6-parameter stages over all levels, then one 12-parameter stage at level 0
 * from that result.  fib_reg_search_jobs: the level and the matrices to evaluate (njobs <= 24; 0 when the search has finished);
 * fib_reg_search_feed: their histograms [njobs][nbins][nbins] with that level's nfinite.  fib_reg_search_result: theta (12 values, zero
 * beyond dof), the cost of theta at level 0, the number of iterations and min(niter, trace_rows) rows of FIB_REG_TRACE_ROW doubles:
 * level, parameters searched, chosen index, 1 = moved / 0 = halved, the cost before, the candidates' costs (NaN beyond 2 n).
 *
 * RUN (fibd_reg_run).  nsearch searches (all created for the same volumes and `levels`), search s against moving frame frames[s], run
 * to their end on device-resident volumes: the pyramids and the ranges of all levels are made in `work` (16-byte aligned,
 * fibd_reg_run_work_size bytes) and the ranges read back once -- a volume without two distinct finite values at any level is
 * FIB_ERR_INVALID ("constant volume"); then, every round, the searches that wait at the coarsest pending level put their jobs into ONE
 * fibd_reg_hist launch, the histograms come back once and every search decides.  Finished searches leave the job list.  Searches are
 * independent: a search's result does not depend on what shares its launches.  The call waits on `stream` once per round; the results
 * are read from the handles.
 *
 * HOST FORM (fib_mri_register).  Every frame of `moving` [nframes][nvox_m] registered to `fixed`, each from theta = 0, on one device
 * (FIB_DEVICE_ALL: FIB_ERR_UNSUPPORTED): theta [nframes][12], cost [nframes], niter [nframes] (each may be NULL but theta), trace
 * [nframes][trace_rows][FIB_REG_TRACE_ROW] or NULL.  levels = 0: fib_reg_levels.  resampled (or NULL): [nframes][nvox_f], frame f pulled
 * through its own final level-0 out2in with fibd_vol_xform, FIB_VOL_TRILINEAR, 0 outside -- the series of dwi_moco. */
#define FIB_REG_MIN_BINS 8
#define FIB_REG_MAX_BINS 64
#define FIB_REG_MAX_JOBS 65535
#define FIB_REG_TRACE_ROW 29
typedef struct fib_reg_search fib_reg_search;
int fibd_vol_halve(const float *in, int nx, int ny, int nz, int nframes, float *out, void *stream);
int fibd_vol_range(const float *vol, int64_t nvox, int nframes, int nbins, void *range, void *stream);
int fibd_reg_hist_work_size(int njobs, size_t *bytes);
int fibd_reg_hist(const float *fixed, int nxf, int nyf, int nzf, const void *fixed_range, const float *moving, int nxm, int nym, int nzm,
                  int nframes, const void *moving_range, const int32_t *job_frame, const float *job_out2in, int njobs, int nbins,
                  uint32_t *hist, void *work, size_t work_bytes, void *stream);
int fib_reg_levels(const int32_t fixed_size[3], const int32_t moving_size[3], int *levels);
int fib_reg_matrix(const double *theta, int dof, const float fixed_vox2ras[16], const int32_t fixed_size[3], const float moving_vox2ras[16],
                   int level, float out2in[16], double *G);
int fib_reg_nmi(const uint32_t *hist, int nbins, int64_t nfinite_fixed, double min_overlap, double *cost);
int fib_reg_search_create(int dof, const int32_t fixed_size[3], const float fixed_res[3], const float fixed_vox2ras[16],
                          const int32_t moving_size[3], const float moving_vox2ras[16], int levels, int halvings, int maxit,
                          double min_overlap, const double *theta0, fib_reg_search **out);
void fib_reg_search_destroy(fib_reg_search *search);
int fib_reg_search_jobs(fib_reg_search *search, int *level, int *njobs, float *out2in);
int fib_reg_search_feed(fib_reg_search *search, const uint32_t *hist, int nbins, int64_t nfinite_fixed);
int fib_reg_search_result(const fib_reg_search *search, double *theta, double *cost, int *niter, double *trace, int trace_rows);
int fibd_reg_run_work_size(const int32_t fixed_size[3], const int32_t moving_size[3], int nframes, int nsearch, int levels, int nbins,
                           size_t *bytes);
int fibd_reg_run(fib_reg_search *const *searches, const int32_t *frames, int nsearch, const float *fixed, const int32_t fixed_size[3],
                 const float *moving, const int32_t moving_size[3], int nframes, int levels, int nbins, void *work, size_t work_bytes,
                 void *stream);
int fib_mri_register(int device, const float *moving, const int32_t moving_size[3], const float moving_vox2ras[16], int nframes,
                     const float *fixed, const int32_t fixed_size[3], const float fixed_res[3], const float fixed_vox2ras[16], int dof,
                     int nbins, int levels, int halvings, int maxit, double min_overlap, double *theta, double *cost, int *niter,
                     double *trace, int trace_rows, float *resampled);

/* ------------------------------------------------------------------------------------ */
/* Non-linear registration: a displacement field estimated by demons, its Jacobian map   */
/* (NOT in the reference)                                                                 */
/* ------------------------------------------------------------------------------------ */
/* The estimator of the field that "Non-linear warps" applies: single-contrast, multi-resolution, additive demons (Thirion 1998; the
 * forces come from the FIXED image's gradient) with a fixed number of iterations per level, so nothing in it depends on the data.  The
 * conventions are those of "Non-linear warps": float32, every multiply, add and divide rounded on its own, no fused multiply-add, planar
 * volumes [nframes][nz][ny][nx], 0-based voxels, the packed float4 field on the device.  These definitions are this project's own; they
 * are the contract, and tests/nlreg_ref.py restates them in NumPy.
 *
 * GEOMETRY.  The field lives on the FIXED volume's grid (space A) and phi(x) = x + d(x) takes fixed RAS to moving RAS (space B), so that
 * fib_warp_volume of the moving volume onto the fixed grid pulls it into place (the ANTs convention).  `post` is the initial affine,
 * fixed RAS -> moving RAS, row-major float[16] (NULL: the identity).  Level l of a pyramid of `levels` levels (1 .. 4) holds the volumes
 * halved l times by fibd_vol_halve; the level-l field sits on the level-l fixed grid, whose vox2ras is V_fix D_l (D_l of "Registration").
 * fib_nlreg_level makes what a level needs, in float64 from the float32 inputs and rounded once:
 *   to_ras = float32(V_fix D_l),  from_ras = float32(inv(V_mov D_l) post),  T = float32(inv(L)^T) with L the 3 x 3 linear part of
 *   V_fix D_l (row-major float[9]),  kappa = float32(1 / ell^2) with ell = 2^l step, `step` in mm (the bindings default it to the
 *   smallest fixed voxel size).
 *
 * ONE ITERATION at level l, for every fixed level-l voxel (i, j, k):
 *   1. NORMALISED VALUES.  n(v) = (v - lo) * s, two roundings, with lo, hi the level volume's finite range by fibd_vol_range's rule and
 *      s = float32(1) / (hi - lo), one float32 subtraction and one division.  norm[4] = { lo_fixed, s_fixed, lo_moving, s_moving }.  A
 *      level volume without two distinct finite values is refused by the drivers ("constant volume", FIB_ERR_INVALID).
 *   2. MOVING SAMPLE.  m = the value fibd_warp_volume gives at this voxel with FIB_VOL_TRILINEAR, the current level field, to_field the
 *      identity (q = (i, j, k); S(q) is still the 8-neighbour sample with f = 0, not special-cased), to_ras and from_ras as above.  A
 *      sample that the INSIDE rule puts outside the moving level volume is ABSENT, not filled.  Then m <- n_moving(m).
 *   3. FIXED GRADIENT.  f = n_fixed(F) at the voxel.  THE DIFFERENCE RULE along a voxel axis of size n at index i:
 *      (f[i + 1] - f[i - 1]) * 0.5 for 0 < i < n - 1, f[1] - f[0] at i = 0, f[n - 1] - f[n - 2] at i = n - 1, and 0 when n == 1.
 *      g_c = (T[c][0] v_0 + T[c][1] v_1) + T[c][2] v_2 with v the three voxel-axis differences: the gradient in 1 / mm, RAS.
 *   4. FORCE.  diff = f - m;  den = ((g_0 g_0 + g_1 g_1) + g_2 g_2) + (diff diff) kappa.  u = 0 if m is absent, if any of f, m, g_c is not
 *      finite, or if den is zero or not finite; otherwise q = diff / den and u_c = q g_c.  d'_c = d_c + u_c with d the field's value AT
 *      the voxel; the fourth word of the packed field is written as 0.  |u| <= ell / 2: an iteration moves a sample by at most half a
 *      level voxel.
 *   5. COST.  count = the number of voxels whose u was computed (exact); ssd = the float64 sum of the float32 squares diff diff over
 *      them (the order of the sum is the kernel's: workgroup partials, then one workgroup over the partials; a run repeats its bits);
 *      cost = ssd / count, NaN when count == 0.
 *   6. REGULARISATION.  d' is smoothed by a separable Gaussian of sigma level voxels (0: none; at most 4): radius r = ceil(3 sigma),
 *      taps w_t = float32(exp(-t^2 / (2 sigma^2)) / sum over t = -r .. r, added in that order) made in float64 on the host; per
 *      component and pass acc = +0, then acc = acc + w_t v[clamp(i + t, 0, n - 1)] for t = -r .. r in that order (the edge value
 *      continues beyond the grid, as in SAMPLE); the x pass over the whole field, then y, then z, each rounded to float32 before the next.
 *
 * BETWEEN LEVELS (fibd_warp_upsample).  The coarsest level starts from zero.  The level-l field becomes the start of level l - 1: fine
 * voxel y takes S(q) of the coarse field at q_c = 0.5 y_c - 0.25 (exact in float32; S is SAMPLE with its clamp).  Displacements are mm
 * and are not scaled.  niter[r] is the count of row r, the rows running from the COARSEST level (r = 0) to level 0; there is no other
 * stopping rule.
 *
 * JACOBIAN MAP (fibd_warp_jacobian).  Per field voxel, D[c][k] = the difference rule of step 3 on component c of the field along voxel
 * axis k; G[c][r] = (D[c][0] Linv[0][r] + D[c][1] Linv[1][r]) + D[c][2] Linv[2][r] with linv = float32(inv(L)), L the linear part of
 * the field's vox2ras (row-major float[9]); J = G with 1 + G[c][c] on the diagonal;
 *   m0 = J11 J22 - J12 J21,  m1 = J10 J22 - J12 J20,  m2 = J10 J21 - J11 J20,  det = (J00 m0 - J01 m1) + J02 m2,
 * every product and difference rounded on its own.  A value <= 0 marks a fold: the estimate-side companion of fibd_warp_invert's err.
 *
 * DEVICE ENTRIES.  Asynchronous on `stream`, nothing is allocated, 64-bit offsets, one thread per field voxel, and no kernel waits for
 * another workgroup.  fibd_nlreg_step: steps 1-5; reads `packed`, writes `out` (another packed field) and *cost = { double ssd;
 * uint64_t count } in DEVICE memory (8-byte aligned); `work` (8-byte aligned, fibd_nlreg_step_work_size bytes) takes the workgroups'
 * partials.  fibd_warp_smooth: step 6 from `packed` into `out` through `work` (a third packed field: 16 nvox bytes, 16-byte aligned);
 * sigma == 0 copies.  fibd_warp_unpack: packed -> planar, the inverse of fibd_warp_pack.  FIB_ERR_INVALID: NULL pointers, non-positive
 * sizes, a packed field that is not 16-byte aligned (volumes, disp and out of the Jacobian: 4 bytes), a short workspace, sigma outside
 * [0, 4], niter < 0, levels outside 1 .. 4, a step that is not positive and finite, a singular vox2ras, ANY overlap between an output
 * or the workspace and anything else the call touches; a dimension above 2^24 is FIB_ERR_UNSUPPORTED.
 *
 * RUN (fibd_nlreg_run).  The whole pyramid on device-resident volumes: the pyramids, the ranges (read back once: a constant level volume
 * is FIB_ERR_INVALID), three packed fields of the level-0 size, the partials and a level's costs live in `work` (16-byte aligned,
 * fibd_nlreg_work_size bytes).  `field` receives the packed level-0 field.  cost and count (HOST arrays, or NULL) are
 * [levels][max(1, max niter)], row r for niter[r]; entries no iteration fills are NaN and 0.  The call waits on `stream` once for the
 * ranges and once per level for that level's costs (not at all for a level when both are NULL).
 *
 * HOST FORMS.  fib_mri_nlreg: one volume `moving` against `fixed` on one device (FIB_DEVICE_ALL: FIB_ERR_UNSUPPORTED), on that device's
 * lease; disp receives the planar field [3][nvox_f].  warped (or NULL) receives fibd_warp_volume of `moving` through the final field
 * onto the fixed grid, FIB_VOL_TRILINEAR, 0 outside, with the three matrices warp_mats = { to_ras, to_field, from_ras } (48 floats:
 * what the caller would hand fib_warp_volume, so the two agree bit for bit).  fib_warp_jacobian: the planar field in, the map out. */
int fib_nlreg_level(const float fixed_vox2ras[16], const float moving_vox2ras[16], const float *post, int level, float step,
                    float to_ras[16], float from_ras[16], float T[9], float *kappa);
int fibd_nlreg_step_work_size(int nx, int ny, int nz, size_t *bytes);
int fibd_nlreg_step(const float *fixed, int nxf, int nyf, int nzf, const float *moving, int nxm, int nym, int nzm, const float norm[4],
                    const float to_ras[16], const float from_ras[16], const float T[9], float kappa, const void *packed, void *out,
                    void *cost, void *work, size_t work_bytes, void *stream);
int fibd_warp_smooth(const void *packed, int nx, int ny, int nz, float sigma, void *out, void *work, size_t work_bytes, void *stream);
int fibd_warp_upsample(const void *coarse, int cx, int cy, int cz, void *out, int nx, int ny, int nz, void *stream);
int fibd_warp_unpack(const void *packed, int nx, int ny, int nz, float *disp, void *stream);
int fibd_warp_jacobian(const void *packed, int nx, int ny, int nz, const float linv[9], float *out, void *stream);
int fibd_nlreg_work_size(const int32_t fixed_size[3], const int32_t moving_size[3], int levels, const int32_t *niter, size_t *bytes);
int fibd_nlreg_run(const float *fixed, const int32_t fixed_size[3], const float fixed_vox2ras[16], const float *moving,
                   const int32_t moving_size[3], const float moving_vox2ras[16], const float *post, int levels, const int32_t *niter,
                   float sigma, float step, void *field, double *cost, int64_t *count, void *work, size_t work_bytes, void *stream);
int fib_mri_nlreg(int device, const float *moving, const int32_t moving_size[3], const float moving_vox2ras[16], const float *fixed,
                  const int32_t fixed_size[3], const float fixed_vox2ras[16], const float *post, int levels, const int32_t *niter,
                  float sigma, float step, float *disp, double *cost, int64_t *count, const float *warp_mats, float *warped);
int fib_warp_jacobian(int device, const float *disp, int nx, int ny, int nz, const float linv[9], float *out);

/* ------------------------------------------------------------------------------------ */
/* Host-buffer drop-in entry points (what the Julia wrapper ccalls)                       */
/* ------------------------------------------------------------------------------------ */

/* The host tier mirrors the reference's own parallel decomposition — `Threads.@threads for iz` over z-slices in the fits
 * (dti.jl:258, gqi.jl:132, dsi.jl:197), contiguous seed chunks in `stream` (stream.jl:757-761) — with GPUs in place of
 * threads.  `device` is a HIP device index, or FIB_DEVICE_ALL for the device set declared with fib_init: the volume is
 * then cut into contiguous voxel slabs (one per entry, one host thread each), seeds are dealt round-robin, the global
 * odfmax (gqi.jl:164) is reduced over the slabs before qa is normalised, and streamlines are merged back into the
 * reference's (seed, sub) order.  Results do not depend on the device set.  Each entry of the set runs a three-stage
 * pipeline over voxel chunks (pinned staging ring: upload || kernels || download), and caches its plans and buffers
 * between calls; calls that share an entry are serialised, calls on different entries run concurrently.  A call that names one device
 * runs on that device's own entry.  Every host-buffer form holds its entry's lock from its first device buffer to its last copy, the
 * single-device forms (fib_st_eigen, fib_st_recon, fib_vol_xform, fib_warp_*, fib_rumba_rec, fib_find_peaks*, fib_str_*,
 * fib_prob_stream) included; fib_trim / fib_shutdown wait for all of them.
 * (fib_rumba_rec and fib_find_peaks* build their plan, a few small tables on the device, before they take the lock.)
 * fib_init(ndev, devs): devs[i] may repeat (two pipelines on one GPU); ndev == 0 selects every visible device (also
 * the default of FIB_DEVICE_ALL without fib_init).  fib_shutdown releases every cached plan, stream and buffer.
 * What a worker KEEPS between calls (grow-only, so that the next call of the same size allocates nothing): its pinned staging ring and the
 * ring's device mirror (3 x (rows in + rows out) x chunk x 4 bytes each: ~1.9 GB of host and of device memory after fib_gqi_rec on 270
 * frames), the device buffers of fib_stream (orientation field, seeds, and the packed result: 1.5 GB after 129 M points), the tracer's
 * workspace (scratch for every line in flight) and the device buffers of fib_str_density / fib_str_sample / fib_str_stats (one chunk of
 * points with its counts, samples and statistics, the density or sampled volume, the offset scratch) and of fib_str_select /
 * fib_str_connectome (the ROI bit volume and the ROIs it was packed from, keep and hits of a chunk, labels, remap, C, W, assign) and of
 * fib_str_resample / fib_str_assign / fib_str_centroids (the equal-length lines of a chunk, the models, label / dist / flip, sums, counts).  A process that shares the GPU with other users of its memory calls fib_trim() when it
 * is done with a batch: everything listed above goes back to the driver (plans are kept: small, and costly to rebuild), the next call
 * re-allocates what it needs.  fib_trim waits for calls in flight; it returns FIB_OK. */
#define FIB_DEVICE_ALL (-1)
/* May be OR-ed into the mask_dtype of fib_dti_fit / fib_adc_fit / fib_gqi_rec / fib_dsi_rec: the caller's output arrays are zero already
 * (freshly allocated -- what the reference does itself: MRI(mask, n, Float32) -> zeros, mri.jl:251-255).  Voxels outside the mask
 * need then not be written, and where only the voxels inside the mask travel (a mask that keeps < 90 % of the volume in runs of 16
 * voxels or more) they are not: with a mask that keeps a third of the volume the scatter stage of the transfer pipeline writes a
 * third of the bytes.  Without the flag every output voxel is written (outside the mask: 0). */
#define FIB_MASK_OUTPUTS_ZEROED 0x100
int fib_init(int ndev, const int *devs);
int fib_trim(void);
void fib_shutdown(void);

/* dti_fit(dwi::MRI, mask::MRI)::DTI (dti.jl:221).  bval/bvec NULL or nvol<=0 reproduce the
 * reference's error() as FIB_ERR_MISSING_BVAL / FIB_ERR_MISSING_BVEC. */
int fib_dti_fit(int device, const float *dwi, int nx, int ny, int nz, int nvol,
                const void *mask, int mask_dtype, const float *bval, const float *bvec,
                const fib_dti_out *out);
/* dki_fit: fibd_dki_fit on host arrays, sharded and chunked like fib_dti_fit; the same missing-table errors.  kt [nvox*15] or NULL. */
int fib_dki_fit(int device, const float *dwi, int nx, int ny, int nz, int nvol,
                const void *mask, int mask_dtype, const float *bval, const float *bvec,
                const float *verts, int nverts, const fib_dki_params *params, const fib_dki_out *out);
/* csd_rec: fibd_csd_rec on host arrays, sharded and chunked like fib_dki_fit (FIB_DEVICE_ALL: the device set); the same missing-table
 * errors, the refusals of fib_csd_design. */
int fib_csd_rec(int device, const float *dwi, int nx, int ny, int nz, int nvol,
                const void *mask, int mask_dtype, const float *bval, const float *bvec,
                const float *verts, int nverts, const int32_t *faces, int nfaces, const fib_csd_params *params, const fib_csd_out *out);
/* msmt_rec: fibd_msmt_rec on host arrays, sharded and chunked like fib_csd_rec (FIB_DEVICE_ALL: the device set); the same missing-table
 * errors, the refusals of fib_msmt_design. */
int fib_msmt_rec(int device, const float *dwi, int nx, int ny, int nz, int nvol,
                 const void *mask, int mask_dtype, const float *bval, const float *bvec,
                 const float *verts, int nverts, const int32_t *faces, int nfaces, const fib_msmt_params *params,
                 const float *wm_R, const float *iso_r, int nshells, const fib_msmt_out *out);
/* adc_fit(dwi::MRI, mask::MRI) (dti.jl:164) */
/* host-buffer form of fibd_st_eigen (structens.jl:13-37) */
int fib_st_eigen(int device, const float *const S[6], int64_t nvox, float *eigvec, float *eigval);
/* host-buffer form of fibd_st_recon: eigvec [nx,ny,nz,3,3], eigval [nx,ny,nz,3] as st_recon returns them (column-major).  The volume
 * goes through in z-slabs sized to half the free device memory (FIBERS_ST_RECON_SLAB=<planes> overrides), each with its halo, so a
 * volume larger than the device's memory still goes through; results do not depend on the slab thickness.  FIB_DEVICE_ALL:
 * FIB_ERR_UNSUPPORTED. */
int fib_st_recon(int device, const float *vol, int nx, int ny, int nz, float sigma, float rho, float *eigvec, float *eigval);
/* host-buffer form of fibd_dwi_denoise: dwi and out [nx,ny,nz,nvol], mask uint8 [nx,ny,nz], sigma and rank [nx,ny,nz] (column-major).
 * The volume goes through the device in z-slabs with a halo of P - 1 planes (FIBERS_DENOISE_SLAB forces the output planes per slab);
 * results do not depend on the slab thickness.  FIB_DEVICE_ALL: FIB_ERR_UNSUPPORTED. */
int fib_dwi_denoise(int device, const float *dwi, int nx, int ny, int nz, int nvol, const uint8_t *mask, int patch, int estimator,
                    float *out, float *sigma, float *rank);
/* host-buffer forms of the brain mask section.  fib_dwi_mask: dwi float32 [nx,ny,nz,nvol] (column-major), mask uint8 [nx,ny,nz], b0
 * float32 [nx,ny,nz] or NULL, info in host memory.  Only the listed frames are uploaded, in chunks of what fits in half the free device
 * memory (FIBERS_MASK_FRAMES forces the frames per chunk), and summed into a float64 buffer on the device: a series larger than the
 * device goes through, and the result does not depend on the chunk.  fib_vol_median: in, out float32 [nx,ny,nz,nframes], every frame
 * on its own, chunked likewise (FIBERS_MEDIAN_FRAMES).  fib_mask_components: mask uint8 (nonzero = inside); labels int32 or NULL,
 * out_mask uint8 or NULL.  FIB_DEVICE_ALL: FIB_ERR_UNSUPPORTED. */
int fib_dwi_mask(int device, const float *dwi, int nx, int ny, int nz, int nvol, const int32_t *frames, int nframes,
                 const fib_mask_params *params, uint8_t *mask, float *b0, fib_mask_info *info);
int fib_vol_median(int device, const float *in, int nx, int ny, int nz, int nframes, int radius, int numpass, float *out);
int fib_mask_components(int device, const uint8_t *mask, int nx, int ny, int nz, int flags, int32_t *labels, uint8_t *out_mask,
                        fib_mask_info *info);
/* host-buffer form of the Gibbs-ringing removal: dwi, out float32 [nx,ny,nz,nvol] (column-major; overlapping buffers: FIB_ERR_INVALID),
 * shift_u, shift_v int8 of that shape or NULL.  Slices are independent, so the series travels in chunks of whole slices: whole frames
 * where more than one fits in half the free device memory, else slabs of slices of one frame (FIBERS_DEGIBBS_SLICES forces the slices
 * per chunk); the result does not depend on the chunk.  FIB_DEVICE_ALL: FIB_ERR_UNSUPPORTED. */
int fib_dwi_degibbs(int device, const float *dwi, int nx, int ny, int nz, int nvol, const fib_degibbs_params *params, float *out,
                    int8_t *shift_u, int8_t *shift_v);
/* xfm_apply(xfm, point) (util.jl:385-420) on npoints float32 points [npoints][3] (x, y, z of a point adjacent, as the 3N vector the
 * reference takes).  vox2vox is ROW-major: vox2vox[4 * i + j] = xfm.vox2vox[i + 1, j + 1] (Julia passes permutedims(vox2vox)).
 * Per point, in float32 with every multiply and add rounded on its own, in the reference's order: w = 0 + m41 x + m42 y + m43 z + m44,
 * then for each row i (0 + mi1 x + mi2 y + mi3 z + mi4) / w with an IEEE division, also for affine matrices (a non-finite input
 * gives a NaN triplet, as in the reference).  in == out is allowed; other overlaps are FIB_ERR_INVALID.  Points need only be 4-byte
 * aligned.  Host-buffer form: the points go through the host tier's chunk pipeline; FIB_DEVICE_ALL splits them over the device set.
 * npoints == 0 does nothing. */
int fib_xfm_apply(int device, const float vox2vox[16], const float *in, float *out, int64_t npoints);
/* host-buffer form of fibd_vol_xform (the "Volume resampling" section above): vol [nframes][nzi][nyi][nxi] and out
 * [nframes][nzo][nyo][nxo] are host memory.  Frames are independent: the call walks chunks of whole frames (upload, one launch,
 * download), sized so that the input and output frames of a chunk fit in half the free device memory (FIBERS_VOL_XFORM_FRAMES=<n>
 * overrides); results do not depend on the chunking.  The chunk's device buffers are local to the call: nothing is kept between
 * calls.  One device: FIB_DEVICE_ALL is FIB_ERR_UNSUPPORTED. */
int fib_vol_xform(int device, const float out2in[16], const void *vol, int nxi, int nyi, int nzi, int nframes, int interp,
                  int32_t outside_bits, void *out, int nxo, int nyo, int nzo);
/* host-buffer forms of the non-linear warps (the "Non-linear warps" section above): every array is host memory and `disp` is the PLANAR
 * field [3][nz][ny][nx]; the call uploads it, packs it on the device and keeps it resident until it returns.  One device
 * (FIB_DEVICE_ALL is FIB_ERR_UNSUPPORTED); the device buffers are local to the call.  Results do not depend on the chunking.
 * fib_warp_points: the points go in chunks of 2^22 (FIBERS_WARP_POINTS=<n> overrides); out == xyz is allowed, other overlaps are
 * FIB_ERR_INVALID; npoints == 0 does nothing.  fib_warp_volume: chunks of whole frames sized to half the free device memory, as
 * fib_vol_xform walks them (FIBERS_WARP_FRAMES=<n> overrides).  fib_warp_invert: inv [3][nzo][nyo][nxo], err [nzo][nyo][nxo] or NULL. */
int fib_warp_points(int device, const float *disp, int nx, int ny, int nz, const float to_ras[16], const float to_field[16],
                    const float from_ras[16], const float *xyz, float *out, int64_t npoints);
int fib_warp_volume(int device, const float *disp, int nx, int ny, int nz, const float to_ras[16], const float to_field[16],
                    const float from_ras[16], const void *vol, int nxi, int nyi, int nzi, int nframes, int interp, int32_t outside_bits,
                    void *out, int nxo, int nyo, int nzo);
int fib_warp_invert(int device, const float *disp, int nx, int ny, int nz, const float out_to_ras[16], const float ras_to_field[16], int niter,
                    float *inv, float *err, int nxo, int nyo, int nzo);
int fib_adc_fit(int device, const float *dwi, int nx, int ny, int nz, int nvol,
                const void *mask, int mask_dtype, const float *bval, float *adc, float *s0);
/* host-buffer forms of the tract maps (fibd_str_density / fibd_str_sample / fibd_str_stats above): every array is host memory.  The
 * points are the large operand: they go to the device in chunks cut at line boundaries (str_sample: at points), while the density
 * volume and the sampled volume stay resident for the call.  density is read only with FIB_DENSITY_ACCUMULATE and always written;
 * *n_outside receives this call's count.  npts < 0 or sum(npts) != npoints: FIB_ERR_INVALID before anything is written.
 * device = FIB_DEVICE_ALL: FIB_ERR_UNSUPPORTED (FIB_DENSITY_ACCUMULATE is the building block for splitting a tractogram). */
int fib_str_density(int device, const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz, int mode,
                    uint32_t *density, int64_t *n_outside);
int fib_str_sample(int device, const float *xyz, int64_t npoints, const float *vol, int nx, int ny, int nz, int nframes, float outside,
                   float *scalars);
int fib_str_stats(int device, const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, const float volres[3],
                  const float *scalars, int nscalars, float *props);
/* host-buffer forms of the selection and the connectome (fibd_str_select / fibd_str_connectome above): every array is host memory.
 * The points go to the device in chunks cut at line boundaries; the ROI bit volume (packed on the device from rois, nroi pointers to
 * uint8 [nvox] volumes, nroi <= 32 or FIB_ERR_INVALID) or the label volume, and C / W, stay resident for the call.  fib_str_select
 * returns keep [nlines], hits [nlines][3] (may be NULL) and counts[2] (host).  Compacting HOST arrays by keep is a host copy and
 * belongs to the caller's language: there is no host form of the gather.  fib_str_connectome accumulates chunk after chunk into one
 * C / W (read only with FIB_CONNECTOME_ACCUMULATE, always written; wmat and assign may be NULL); *n_lines = the lines counted.
 * npts < 0 or sum(npts) != npoints: FIB_ERR_INVALID before anything is written.  device = FIB_DEVICE_ALL: FIB_ERR_UNSUPPORTED. */
int fib_str_select(int device, const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz,
                   const uint8_t *const *rois, int nroi, uint64_t visit_all, uint64_t visit_none, uint64_t end_any, uint64_t end_both,
                   int32_t min_npts, int32_t max_npts, uint8_t *keep, uint32_t *hits, int64_t *counts);
int fib_str_connectome(int device, const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz,
                       const float volres[3], const int32_t *labels, const int32_t *remap, int64_t nremap, int nnodes, int flags,
                       uint32_t *cmat, double *wmat, int32_t *assign, int64_t *n_lines);
/* host-buffer form of the tractogram weights (fibd_str_weights above): every array is host memory (ovec / f: nvec pointers to host
 * arrays).  The points go to the device once, in chunks cut at line boundaries (2^22 points; FIBERS_FIXEL_POINTS=<n> overrides, in the
 * product build too, as FIBERS_WARP_POINTS does), only to make the fixel ids; the ids, q, TDq and the field stay resident for the
 * iterations.  q0 may be NULL.  *mu = state slot [1]; counts int64 [5] = state slots [5..9] (points unassigned, lines without an
 * assigned point, lines at the clamp, lines at q = 0, overflow).  Everything it writes equals the device form's output byte for byte.
 * npts < 0 or sum(npts) != npoints: FIB_ERR_INVALID before anything is written.  device = FIB_DEVICE_ALL: FIB_ERR_UNSUPPORTED. */
int fib_str_weights(int device, const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz,
                    int32_t nvec, const float *const *ovec, const float *const *f, const uint8_t *mask, float f_thresh, float cos2,
                    int niter, const uint32_t *q0, uint32_t *q, float *weights, float *td, double *mu, double *cost, int64_t *counts);
/* host-buffer forms of the bundle tools (fibd_str_resample / fibd_str_assign / fibd_str_centroids above): every array is host memory.
 * The lines go to the device in chunks cut at line boundaries; the models, and sums / counts, stay resident for the call.  Everything
 * fib_str_resample and fib_str_assign write equals the device form's output byte for byte (a line's result depends on the line
 * alone); fib_str_centroids adds chunk after chunk into one sums / counts (read only with FIB_CENTROIDS_ACCUMULATE, always written):
 * counts equal the device form's, sums are within the bound stated above.  npts < 0 or sum(npts) != npoints: FIB_ERR_INVALID before
 * anything is written.  device = FIB_DEVICE_ALL: FIB_ERR_UNSUPPORTED. */
int fib_str_resample(int device, const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, const float volres[3], int K,
                     const uint8_t *flip, float *out);
int fib_str_assign(int device, const float *lines, int64_t nlines, int K, const float *models, int nmodels, const float volres[3],
                   float thresh_mm, int32_t *label, float *dist, uint8_t *flip, float *dist_all);
int fib_str_centroids(int device, const float *lines, int64_t nlines, int K, const int32_t *label, const uint8_t *flip, int nmodels,
                      int flags, double *sums, uint32_t *counts);
/* gqi_rec(dwi, mask, odf_dirs, sigma)::GQI (gqi.jl:109) */
int fib_gqi_rec(int device, const float *dwi, int nx, int ny, int nz, int nvol,
                const void *mask, int mask_dtype, const float *bval, const float *bvec,
                const float *verts, int nverts, const int32_t *faces, int nfaces, float sigma,
                float *odf, float *const peak[3], float *const qa[3]);
/* dsi_rec(dwi, mask, odf_dirs, hann_width)::DSI (dsi.jl:171) */
int fib_dsi_rec(int device, const float *dwi, int nx, int ny, int nz, int nvol,
                const void *mask, int mask_dtype, const float *bval, const float *bvec,
                const float *verts, int nverts, const int32_t *faces, int nfaces, int hann_width,
                float *pdf, float *odf, float *const peak[3], float *const qa[3]);

/* rumba_rec(dwi, mask, odf_dirs, niter, lam_para, lam_perp, lam_csf, lam_gm, ncoils, coil_combine, ipat_factor, use_tv)
 * ::RUMBASD (rusd.jl:419); host buffers, outputs caller-allocated like the other fits. */
int fib_rumba_rec(int device, const float *dwi, int nx, int ny, int nz, int nvol, const void *mask, int mask_dtype,
                  const float *bval, const float *bvec, const float *verts, int nverts, int niter,
                  float lam_para, float lam_perp, float lam_csf, float lam_gm, int ncoils, int sos_grappa, int ipat_factor,
                  int use_tv, const fib_rumba_out *out, float *snr_mean, float *snr_std);

/* find_peaks!(W) (gqi.jl:180-201) for nvox ODFs in host memory.  odf [nvox x nvert] planar (row v = the nvox
 * amplitudes of half-sphere vertex v, like MRI.vol[:,:,:,v]); isort_top [3 x nvox] planar: the first three entries
 * of `isort` (0-based first-half vertex rows, -1 where the sphere has fewer vertices); nvalid [nvox] (gqi.jl:200). */
int fib_find_peaks(int device, const float *odf, int64_t nvox, const float *verts, int nverts,
                   const int32_t *faces, int nfaces, int32_t *isort_top, int32_t *nvalid);
/* find_peaks!(W) with every output the reference's work struct receives (gqi.jl:180-201): odf_peak [nvox x nvert] planar
 * (W.odf_peak: the amplitudes of the local peaks, 0 elsewhere, :184-196), isort [nvox x nvert] planar (W.isort: the complete
 * sortperm(odf_peak, rev=true), 0-based, :198) and nvalid [nvox] (the return value, :200). */
int fib_find_peaks_work(int device, const float *odf, int64_t nvox, const float *verts, int nverts,
                        const int32_t *faces, int nfaces, float *odf_peak, int32_t *isort, int32_t *nvalid);

/* stream(ovec; f, f_thresh, fa, fa_thresh, mask, seed, ...)::Tract (stream.jl:730), non-LCM macro path.
 * ovec[k] [nx,ny,nz,3]; f[k] [nx,ny,nz] or f == NULL; fa / mask / seed may be NULL (mask == NULL:
 * any-nonzero-vector mask, stream.jl:96-100; seed == NULL: brain mask seeds, stream.jl:744).
 * Output is library-allocated (release with fib_tract_free): */
typedef struct {
    int64_t nlines;       /* streamlines kept (npts >= len_min) */
    int64_t npoints;      /* sum of npts */
    int32_t *npts;        /* [nlines] */
    int64_t *seed_index;  /* [nlines] seed*nsub + sub, seeds counted in findall order */
    float *xyz;           /* [3*npoints] */
    uint8_t *flags;       /* [npoints] (fib_stream_lcm only, else NULL): LCM and angle pick disagreed at this point */
} fib_tract_out;

int fib_stream(int device, const fib_stream_params *prm, const float *const *ovec, const float *const *f,
               float f_thresh, const float *fa, float fa_thresh, const void *mask, int mask_dtype,
               const void *seed, int seed_dtype, const float *sublist, int32_t nsub, fib_tract_out *out);
/* stream(ovec; ..., lcms, lcm_thresh) (stream.jl:730): fib_stream with local connection matrices lcms [nx,ny,nz,10]
 * (see fibd_stream_trace_lcm for the semantics and the random-number contract); out->flags is filled. */
int fib_stream_lcm(int device, const fib_stream_params *prm, const float *const *ovec, const float *const *f,
                   float f_thresh, const float *fa, float fa_thresh, const void *mask, int mask_dtype,
                   const void *seed, int seed_dtype, const float *sublist, int32_t nsub,
                   const float *lcms, float lcm_thresh, uint64_t rng_seed, fib_tract_out *out);
/* prob_stream: the host-buffer form of the "Probabilistic tracking" section.  odf [nx,ny,nz,nvert] column-major (planar [nvert][nvox]),
 * vertices [nvert][3]; mask and seed uint8 [nvox] (non-zero = inside) or NULL (mask NULL: no mask; seed NULL: the mask's voxels, or all).
 * The weight table is built from voxel chunks of the host ODF, so the float ODF is never whole on the device (the table, 2 * pitch bytes
 * per voxel, is).  Fills a library-allocated fib_tract_out like fib_stream (release with fib_tract_free); flags stays NULL.  The same
 * bytes as fibd_prob_table + fibd_prob_run.  One device: FIB_DEVICE_ALL is FIB_ERR_UNSUPPORTED. */
int fib_prob_stream(int device, int nx, int ny, int nz, const float *odf, int nvert, const float *vertices, const uint8_t *mask,
                    const uint8_t *seed, const float *sublist, int32_t nsub, int32_t len_min, int32_t len_max, float cosang_thresh,
                    float step_size, float pmf_thresh, int32_t subtract_min, uint64_t rng_seed, fib_tract_out *out);
void fib_tract_free(fib_tract_out *out);

#ifdef __cplusplus
}
#endif
#endif /* FIBERS_HIP_H */
