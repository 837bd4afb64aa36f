#=
  FibersHIP.jl — the binding a Fibers.jl maintainer would add to route the hot path through
  libfibers_hip.so (MI355X / gfx950).  Mechanically derived from include/fibers_hip.h.

  NOT EXECUTED IN THIS REPOSITORY'S CI: the build image has no Julia.  It keeps the reference's
  signatures (dti_fit, adc_fit, gqi_rec, dsi_rec, stream) and result structs; only the bodies change.
  Include after src/Fibers.jl's own definitions of MRI, ODF, DTI, GQI, DSI, Tract, str_add!.
=#

const libfibers = get(ENV, "FIBERS_HIP_LIB", "libfibers_hip.so")

const FIB_DTYPE = Dict(UInt8=>0, Int8=>1, Int16=>2, UInt16=>3, Int32=>4, UInt32=>5,
                       Float32=>6, Float64=>7, Int64=>8, Bool=>9)
# OR-ed into mask_dtype by the fits below: their outputs are MRI(mask, n, Float32) = zeros (mri.jl:251-255), so the library need not
# write the voxels outside the mask (include/fibers_hip.h)
const FIB_MASK_OUTPUTS_ZEROED = Cint(0x100)

# Multi-GPU: `device = FIB_DEVICE_ALL` shards a call over the device set declared here (contiguous voxel slabs for the fits,
# as Threads.@threads shards the z loop in dti.jl:258 / gqi.jl:132 / dsi.jl:197; round-robin seeds for stream).  Without
# fib_init the set is every visible GPU.  Results do not depend on the set.
const FIB_DEVICE_ALL = Cint(-1)
# values of fib_stream_params.interp: the reference's nearest-voxel Euler tracker; the trilinear field stepped by Euler, midpoint, RK4
const FIB_STREAM_NEAREST = Int32(0)
const FIB_STREAM_TRILINEAR = Int32(1)
const FIB_STREAM_TRILINEAR_RK2 = Int32(2)
const FIB_STREAM_TRILINEAR_RK4 = Int32(3)
fib_init(devs::Vector{<:Integer}=Int[]) = fib_check(ccall((:fib_init, libfibers), Cint, (Cint, Ptr{Cint}), length(devs), Cint.(devs)))
fib_trim() = ccall((:fib_trim, libfibers), Cint, ())          # buffers kept between calls go back to the driver (plans stay)
fib_shutdown() = ccall((:fib_shutdown, libfibers), Cvoid, ())

function fib_check(rc::Cint)
  rc == 0 && return
  msg = unsafe_string(ccall((:fib_last_error, libfibers), Cstring, ()))
  error(msg)                       # same strings as the reference's error() calls
end

# layout: fib_dti_out sizeof 80: s0@0 eigval1@8 eigval2@16 eigval3@24 eigvec1@32 eigvec2@40 eigvec3@48 rd@56 md@64 fa@72
struct FibDtiOut
  s0::Ptr{Float32}; eigval1::Ptr{Float32}; eigval2::Ptr{Float32}; eigval3::Ptr{Float32}
  eigvec1::Ptr{Float32}; eigvec2::Ptr{Float32}; eigvec3::Ptr{Float32}
  rd::Ptr{Float32}; md::Ptr{Float32}; fa::Ptr{Float32}
end

"dti_fit(dwi::MRI, mask::MRI) — replaces dti.jl:221-316"
function dti_fit(dwi::MRI, mask::MRI; device::Integer=0)
  isempty(dwi.bval) && error("Missing b-value table from input DWI structure")
  isempty(dwi.bvec) && error("Missing gradient table from input DWI structure")
  nx, ny, nz, nvol = size(dwi.vol)
  S0 = MRI(mask, 1, Float32); E1 = MRI(mask, 1, Float32); E2 = MRI(mask, 1, Float32); E3 = MRI(mask, 1, Float32)
  V1 = MRI(mask, 3, Float32); V2 = MRI(mask, 3, Float32); V3 = MRI(mask, 3, Float32)
  RD = MRI(mask, 1, Float32); MD = MRI(mask, 1, Float32); FA = MRI(mask, 1, Float32)
  vol = dwi.vol::Array{Float32,4}; m = mask.vol
  GC.@preserve vol m S0 E1 E2 E3 V1 V2 V3 RD MD FA begin
    out = Ref(FibDtiOut(pointer(S0.vol), pointer(E1.vol), pointer(E2.vol), pointer(E3.vol),
                        pointer(V1.vol), pointer(V2.vol), pointer(V3.vol),
                        pointer(RD.vol), pointer(MD.vol), pointer(FA.vol)))
    fib_check(ccall((:fib_dti_fit, libfibers), Cint,
                    (Cint, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32}, Ref{FibDtiOut}),
                    device, vol, nx, ny, nz, nvol, m, FIB_DTYPE[eltype(m)] | FIB_MASK_OUTPUTS_ZEROED, dwi.bval, dwi.bvec, out))
  end
  return DTI(S0, E1, E2, E3, V1, V2, V3, RD, MD, FA)
end

"adc_fit(dwi::MRI, mask::MRI) — replaces dti.jl:164-213"
function adc_fit(dwi::MRI, mask::MRI; device::Integer=0)
  isempty(dwi.bval) && error("Missing b-value table from input DWI structure")
  nx, ny, nz, nvol = size(dwi.vol)
  adc = MRI(mask, 1, Float32); s0 = MRI(mask, 1, Float32)
  vol = dwi.vol::Array{Float32,4}; m = mask.vol
  GC.@preserve vol m adc s0 fib_check(ccall((:fib_adc_fit, libfibers), Cint,
      (Cint, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
      device, vol, nx, ny, nz, nvol, m, FIB_DTYPE[eltype(m)] | FIB_MASK_OUTPUTS_ZEROED, dwi.bval, adc.vol, s0.vol))
  return adc, s0
end

# layout: fib_dki_params sizeof 16: min_signal@0 min_diffusivity@4 min_kurtosis@8 max_kurtosis@12
struct FibDkiParams
  min_signal::Cfloat; min_diffusivity::Cfloat; min_kurtosis::Cfloat; max_kurtosis::Cfloat
end

# layout: fib_dki_out sizeof 112: s0@0 eigval1@8 eigval2@16 eigval3@24 eigvec1@32 eigvec2@40 eigvec3@48 rd@56 md@64 fa@72 mk@80 ak@88 rk@96 kt@104
struct FibDkiOut
  s0::Ptr{Float32}; eigval1::Ptr{Float32}; eigval2::Ptr{Float32}; eigval3::Ptr{Float32}
  eigvec1::Ptr{Float32}; eigvec2::Ptr{Float32}; eigvec3::Ptr{Float32}
  rd::Ptr{Float32}; md::Ptr{Float32}; fa::Ptr{Float32}
  mk::Ptr{Float32}; ak::Ptr{Float32}; rk::Ptr{Float32}; kt::Ptr{Float32}
end

"Container for outputs of a DKI fit: the fields of `DTI`, mean / axial / radial kurtosis and the kurtosis tensor W (15 frames)"
struct DKI
  s0::MRI; eigval1::MRI; eigval2::MRI; eigval3::MRI; eigvec1::MRI; eigvec2::MRI; eigvec3::MRI; rd::MRI; md::MRI; fa::MRI
  mk::MRI; ak::MRI; rk::MRI; kt::MRI
end

"dki_design(bval, bvec) — the DKI design (b in ms/um^2), its scaled pseudo-inverse and its rank, on the host (include/fibers_hip.h)"
function dki_design(bval::Vector{Float32}, bvec::Matrix{Float32})
  nvol = length(bval)
  A = zeros(Float32, nvol, 22); pA = zeros(Float32, 22, nvol); rank = Ref{Cint}(0)
  fib_check(ccall((:fib_dki_design, libfibers), Cint, (Ptr{Float32}, Ptr{Float32}, Cint, Ptr{Float32}, Ptr{Float32}, Ref{Cint}),
                  bval, bvec, nvol, A, pA, rank))
  return A, pA, Int(rank[])
end

"dki_fit(dwi, mask, odf_dirs) — diffusion kurtosis fit with MK / AK / RK maps (not in the reference; DESIGN.md §5)"
function dki_fit(dwi::MRI, mask::MRI, odf_dirs::ODF=sphere_642; min_signal::Real=1f-4, min_diffusivity::Real=1f-6,
                 min_kurtosis::Real=-3f0/7f0, max_kurtosis::Real=10f0, device::Integer=0)
  isempty(dwi.bval) && error("Missing b-value table from input DWI structure")
  isempty(dwi.bvec) && error("Missing gradient table from input DWI structure")
  nx, ny, nz, nvol = size(dwi.vol)
  S0 = MRI(mask, 1, Float32); E1 = MRI(mask, 1, Float32); E2 = MRI(mask, 1, Float32); E3 = MRI(mask, 1, Float32)
  V1 = MRI(mask, 3, Float32); V2 = MRI(mask, 3, Float32); V3 = MRI(mask, 3, Float32)
  RD = MRI(mask, 1, Float32); MD = MRI(mask, 1, Float32); FA = MRI(mask, 1, Float32)
  MK = MRI(mask, 1, Float32); AK = MRI(mask, 1, Float32); RK = MRI(mask, 1, Float32); KT = MRI(mask, 15, Float32)
  vol = dwi.vol::Array{Float32,4}; m = mask.vol; verts = odf_dirs.vertices
  par = Ref(FibDkiParams(min_signal, min_diffusivity, min_kurtosis, max_kurtosis))
  GC.@preserve vol m verts S0 E1 E2 E3 V1 V2 V3 RD MD FA MK AK RK KT begin
    out = Ref(FibDkiOut(pointer(S0.vol), pointer(E1.vol), pointer(E2.vol), pointer(E3.vol),
                        pointer(V1.vol), pointer(V2.vol), pointer(V3.vol),
                        pointer(RD.vol), pointer(MD.vol), pointer(FA.vol),
                        pointer(MK.vol), pointer(AK.vol), pointer(RK.vol), pointer(KT.vol)))
    fib_check(ccall((:fib_dki_fit, libfibers), Cint,
                    (Cint, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32},
                     Ptr{Float32}, Cint, Ref{FibDkiParams}, Ref{FibDkiOut}),
                    device, vol, nx, ny, nz, nvol, m, FIB_DTYPE[eltype(m)] | FIB_MASK_OUTPUTS_ZEROED, dwi.bval, dwi.bvec,
                    verts, size(verts, 1), par, out))
  end
  return DKI(S0, E1, E2, E3, V1, V2, V3, RD, MD, FA, MK, AK, RK, KT)
end

# layout: fib_csd_params sizeof 40: lmax@0 lambda_para@4 lambda_perp@8 s0@12 b0_thresh@16 shell@20 b_tol@24 lambda@28 tau@32 niter@36
struct FibCsdParams
  lmax::Cint; lambda_para::Cfloat; lambda_perp::Cfloat; s0::Cfloat; b0_thresh::Cfloat; shell::Cfloat; b_tol::Cfloat
  lambda::Cfloat; tau::Cfloat; niter::Cint
end

# layout: fib_csd_out sizeof 72: sh@0 odf@8 niter@16 peak@24 f@48
struct FibCsdOut
  sh::Ptr{Float32}; odf::Ptr{Float32}; niter::Ptr{Float32}
  peak::NTuple{3,Ptr{Float32}}; f::NTuple{3,Ptr{Float32}}
end

"Container for outputs of a CSD reconstruction: harmonic coefficients, fibre ODF, its three peaks with their amplitudes, solves per voxel"
struct CSD
  sh::MRI; odf::MRI; peak::Vector{MRI}; f::Vector{MRI}; niter::MRI
end

"csd_rec(dwi, mask, response, odf_dirs) — constrained spherical deconvolution of one shell (not in the reference; include/fibers_hip.h).
 response = (lambda_para, lambda_perp, s0); shell <= 0: the largest b"
function csd_rec(dwi::MRI, mask::MRI, response::NTuple{3,<:Real}, odf_dirs::ODF=sphere_724; lmax::Integer=8, b0_thresh::Real=50f0,
                 shell::Real=0f0, b_tol::Real=0.05f0, lambda::Real=1f0, tau::Real=0.1f0, niter::Integer=50, device::Integer=0)
  isempty(dwi.bval) && error("Missing b-value table from input DWI structure")
  isempty(dwi.bvec) && error("Missing gradient table from input DWI structure")
  nx, ny, nz, nvol = size(dwi.vol)
  n = div((lmax + 1) * (lmax + 2), 2)
  nreg = div(size(odf_dirs.vertices, 1), 2)
  SH = MRI(mask, n, Float32); O = MRI(mask, nreg, Float32); NI = MRI(mask, 1, Float32)
  peak = [MRI(mask, 3, Float32) for _ in 1:3]; f = [MRI(mask, 1, Float32) for _ in 1:3]
  faces = Int32.(odf_dirs.faces); verts = odf_dirs.vertices; vol = dwi.vol::Array{Float32,4}; m = mask.vol
  par = Ref(FibCsdParams(lmax, response[1], response[2], response[3], b0_thresh, shell, b_tol, lambda, tau, niter))
  GC.@preserve vol m SH O NI peak f faces verts begin
    out = Ref(FibCsdOut(pointer(SH.vol), pointer(O.vol), pointer(NI.vol),
                        (pointer(peak[1].vol), pointer(peak[2].vol), pointer(peak[3].vol)),
                        (pointer(f[1].vol), pointer(f[2].vol), pointer(f[3].vol))))
    fib_check(ccall((:fib_csd_rec, libfibers), Cint,
                    (Cint, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32},
                     Ptr{Float32}, Cint, Ptr{Int32}, Cint, Ref{FibCsdParams}, Ref{FibCsdOut}),
                    device, vol, nx, ny, nz, nvol, m, FIB_DTYPE[eltype(m)] | FIB_MASK_OUTPUTS_ZEROED, dwi.bval, dwi.bvec,
                    verts, size(verts, 1), faces, size(faces, 1), par, out))
  end
  return CSD(SH, O, peak, f, NI)
end

# layout: fib_msmt_params sizeof 32: lmax@0 niso@4 b0_thresh@8 b_tol@12 lambda@16 lambda_iso@20 tau@24 niter@28
struct FibMsmtParams
  lmax::Cint; niso::Cint; b0_thresh::Cfloat; b_tol::Cfloat; lambda::Cfloat; lambda_iso::Cfloat; tau::Cfloat; niter::Cint
end

# layout: fib_msmt_out sizeof 88: sh@0 iso@8 odf@24 niter@32 peak@40 f@64
struct FibMsmtOut
  sh::Ptr{Float32}; iso::NTuple{2,Ptr{Float32}}; odf::Ptr{Float32}; niter::Ptr{Float32}
  peak::NTuple{3,Ptr{Float32}}; f::NTuple{3,Ptr{Float32}}
end

"Container for outputs of a multi-tissue deconvolution: WM harmonic coefficients, isotropic fractions (GM, CSF; not clamped), WM fibre ODF,
 its three peaks with their amplitudes, solves per voxel"
struct MSMT
  sh::MRI; iso::Vector{MRI}; odf::MRI; peak::Vector{MRI}; f::Vector{MRI}; niter::MRI
end

"msmt_shells(bval) — the shell of every frame (0-based; shell 0 = b <= b0_thresh) and the mean b of every shell"
function msmt_shells(bval::Vector{Float32}; b0_thresh::Real=50f0, b_tol::Real=0.05f0)
  nvol = length(bval)
  bvec = ones(Float32, nvol, 3); shell = zeros(Int32, nvol); bbar = zeros(Float64, 9); ns = Ref{Cint}(0)
  par = Ref(FibMsmtParams(8, 0, b0_thresh, b_tol, 1f0, 1f0, 0f0, 1))
  fib_check(ccall((:fib_msmt_design, libfibers), Cint,
                  (Ptr{Float32}, Ptr{Float32}, Cint, Ptr{Float32}, Cint, Ref{FibMsmtParams}, Ptr{Float32}, Ptr{Float32}, Cint,
                   Ptr{Int32}, Ref{Cint}, Ptr{Float64}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cint}),
                  bval, bvec, nvol, C_NULL, 0, par, C_NULL, C_NULL, 0, shell, ns, bbar, C_NULL, C_NULL, C_NULL, C_NULL))
  return shell, bbar[1:ns[]]
end

"msmt_wm_response(lambda_para, lambda_perp, s0, bbar; lmax) — R_l of a prolate tensor at every shell: [lmax / 2 + 1, nshells]
 (one column per shell: the row-major table of the C ABI)"
function msmt_wm_response(lambda_para::Real, lambda_perp::Real, s0::Real, bbar::Vector{Float64}; lmax::Integer=8)
  R = zeros(Float32, div(lmax, 2) + 1, length(bbar))
  fib_check(ccall((:fib_msmt_wm_response, libfibers), Cint, (Cfloat, Cfloat, Cfloat, Ptr{Float64}, Cint, Cint, Ptr{Float32}),
                  lambda_para, lambda_perp, s0, bbar, length(bbar), lmax, R))
  return R
end

"msmt_rec(dwi, mask, wm_R, iso_r, odf_dirs) — multi-shell multi-tissue deconvolution of every frame (not in the reference;
 include/fibers_hip.h).  wm_R [lmax / 2 + 1, nshells] as msmt_wm_response returns it; iso_r [nshells, niso]: the mean signal of every
 isotropic tissue (GM, then CSF) per shell, niso = 0, 1 or 2"
function msmt_rec(dwi::MRI, mask::MRI, wm_R::Matrix{Float32}, iso_r::Matrix{Float32}, odf_dirs::ODF=sphere_724; lmax::Integer=8,
                  b0_thresh::Real=50f0, b_tol::Real=0.05f0, lambda::Real=1f0, lambda_iso::Real=1f0, tau::Real=0f0, niter::Integer=50,
                  device::Integer=0)
  isempty(dwi.bval) && error("Missing b-value table from input DWI structure")
  isempty(dwi.bvec) && error("Missing gradient table from input DWI structure")
  nx, ny, nz, nvol = size(dwi.vol)
  nshells = size(wm_R, 2); niso = size(iso_r, 2)
  size(wm_R, 1) == div(lmax, 2) + 1 || error("wm_R must be [lmax / 2 + 1, nshells]")
  (niso <= 2 && (niso == 0 || size(iso_r, 1) == nshells)) || error("iso_r must be [nshells, niso] with niso <= 2")
  nwm = div((lmax + 1) * (lmax + 2), 2)
  nreg = div(size(odf_dirs.vertices, 1), 2)
  SH = MRI(mask, nwm, Float32); O = MRI(mask, nreg, Float32); NI = MRI(mask, 1, Float32)
  iso = [MRI(mask, 1, Float32) for _ in 1:niso]
  peak = [MRI(mask, 3, Float32) for _ in 1:3]; f = [MRI(mask, 1, Float32) for _ in 1:3]
  faces = Int32.(odf_dirs.faces); verts = odf_dirs.vertices; vol = dwi.vol::Array{Float32,4}; m = mask.vol
  par = Ref(FibMsmtParams(lmax, niso, b0_thresh, b_tol, lambda, lambda_iso, tau, niter))
  GC.@preserve vol m SH O NI iso peak f faces verts wm_R iso_r begin
    isop = ntuple(t -> t <= niso ? pointer(iso[t].vol) : Ptr{Float32}(C_NULL), 2)
    out = Ref(FibMsmtOut(pointer(SH.vol), isop, pointer(O.vol), pointer(NI.vol),
                         (pointer(peak[1].vol), pointer(peak[2].vol), pointer(peak[3].vol)),
                         (pointer(f[1].vol), pointer(f[2].vol), pointer(f[3].vol))))
    fib_check(ccall((:fib_msmt_rec, libfibers), Cint,
                    (Cint, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32},
                     Ptr{Float32}, Cint, Ptr{Int32}, Cint, Ref{FibMsmtParams}, Ptr{Float32}, Ptr{Float32}, Cint, Ref{FibMsmtOut}),
                    device, vol, nx, ny, nz, nvol, m, FIB_DTYPE[eltype(m)] | FIB_MASK_OUTPUTS_ZEROED, dwi.bval, dwi.bvec,
                    verts, size(verts, 1), faces, size(faces, 1), par, wm_R, iso_r, nshells, out))
  end
  return MSMT(SH, iso, O, peak, f, NI)
end

"find_peaks(odf, odf_dirs) — find_peaks!(W) (gqi.jl:180-201) for a whole ODF volume [nx,ny,nz,nvert]:
 returns (isort_top [nx,ny,nz,3] 1-based first-half vertex rows, 0 where absent; nvalid [nx,ny,nz])"
function find_peaks(odf::MRI, odf_dirs::ODF=sphere_642; device::Integer=0)
  nx, ny, nz, nvert = size(odf.vol)
  nvox = nx * ny * nz
  top = Array{Int32}(undef, nx, ny, nz, 3); nvalid = Array{Int32}(undef, nx, ny, nz)
  faces = Int32.(odf_dirs.faces); verts = odf_dirs.vertices; vol = odf.vol::Array{Float32,4}
  GC.@preserve vol top nvalid faces verts fib_check(ccall((:fib_find_peaks, libfibers), Cint,
      (Cint, Ptr{Float32}, Int64, Ptr{Float32}, Cint, Ptr{Int32}, Cint, Ptr{Int32}, Ptr{Int32}),
      device, vol, nvox, verts, size(verts, 1), faces, size(faces, 1), top, nvalid))
  return top .+ Int32(1), nvalid
end

"""
    find_peaks!(W::Union{GQIwork, DSIwork})

The reference's own surface (gqi.jl:180-201): reads `W.o[tid]` of the calling thread, fills `W.odf_peak[tid]` (amplitudes of the
local peaks, 0 elsewhere) and `W.isort[tid]` (`sortperm(odf_peak, rev=true)`, 1-based), returns `count(odf_peak .> 0)`.
`W.faces` is the FOLDED face table of the work struct (vertex indices 1..nvert); the library folds faces itself, so the
unfolded tessellation is rebuilt by pairing every half-sphere vertex with a placeholder antipode that no face uses.
One voxel per call, as in the reference; `gqi_rec` / `dsi_rec` do not come through here (they find the peaks on the GPU while
the ODF is on chip) — this is for code that calls `find_peaks!` directly.
"""
function find_peaks!(W; device::Integer=0)
  tid = Threads.threadid()
  o = W.o[tid]::Vector{Float32}
  nvert = W.nvert
  faces = Int32.(W.faces)                                 # folded, 1-based, [nf x 3]
  verts = zeros(Float32, 2 * nvert, 3)                    # coordinates are not used by find_peaks!
  pk = Vector{Float32}(undef, nvert); isort = Vector{Int32}(undef, nvert); nvalid = Ref{Int32}(0)
  GC.@preserve o pk isort faces verts fib_check(ccall((:fib_find_peaks_work, libfibers), Cint,
      (Cint, Ptr{Float32}, Int64, Ptr{Float32}, Cint, Ptr{Int32}, Cint, Ptr{Float32}, Ptr{Int32}, Ref{Int32}),
      device, o, 1, verts, 2 * nvert, faces, size(faces, 1), pk, isort, nvalid))
  W.odf_peak[tid] .= pk
  W.isort[tid] .= Int.(isort) .+ 1
  return Int(nvalid[])
end

"gqi_rec(dwi, mask, odf_dirs, σ) — replaces gqi.jl:109-171 (and find_peaks! gqi.jl:180-201)"
function gqi_rec(dwi::MRI, mask::MRI, odf_dirs::ODF=sphere_642, σ::Float32=Float32(1.25); device::Integer=0)
  isempty(dwi.bval) && error("Missing b-value table from input DWI structure")
  isempty(dwi.bvec) && error("Missing gradient table from input DWI structure")
  nx, ny, nz, nvol = size(dwi.vol)
  nvert = div(size(odf_dirs.vertices, 1), 2)
  odf = MRI(mask, nvert, Float32)
  peak = [MRI(mask, 3, Float32) for _ in 1:3]; qa = [MRI(mask, 1, Float32) for _ in 1:3]
  faces = Int32.(odf_dirs.faces); verts = odf_dirs.vertices; vol = dwi.vol::Array{Float32,4}; m = mask.vol
  pk = [pointer(p.vol) for p in peak]; pq = [pointer(q.vol) for q in qa]
  GC.@preserve vol m odf peak qa faces verts fib_check(ccall((:fib_gqi_rec, libfibers), Cint,
      (Cint, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32},
       Ptr{Float32}, Cint, Ptr{Int32}, Cint, Cfloat, Ptr{Float32}, Ptr{Ptr{Float32}}, Ptr{Ptr{Float32}}),
      device, vol, nx, ny, nz, nvol, m, FIB_DTYPE[eltype(m)] | FIB_MASK_OUTPUTS_ZEROED, dwi.bval, dwi.bvec,
      verts, size(verts, 1), faces, size(faces, 1), σ, odf.vol, pk, pq))
  return GQI(odf, peak, qa)
end

"dsi_rec(dwi, mask, odf_dirs, hann_width) — replaces dsi.jl:171-270"
function dsi_rec(dwi::MRI, mask::MRI, odf_dirs::ODF=sphere_642, hann_width::Int=32; device::Integer=0)
  isempty(dwi.bval) && error("Missing b-value table from input DWI structure")
  isempty(dwi.bvec) && error("Missing gradient table from input DWI structure")
  nx, ny, nz, nvol = size(dwi.vol)
  nvert = div(size(odf_dirs.vertices, 1), 2)
  pdf = MRI(mask, nvol, Float32); odf = MRI(mask, nvert, Float32)
  peak = [MRI(mask, 3, Float32) for _ in 1:3]; qa = [MRI(mask, 1, Float32) for _ in 1:3]
  faces = Int32.(odf_dirs.faces); verts = odf_dirs.vertices; vol = dwi.vol::Array{Float32,4}; m = mask.vol
  pk = [pointer(p.vol) for p in peak]; pq = [pointer(q.vol) for q in qa]
  GC.@preserve vol m pdf odf peak qa faces verts fib_check(ccall((:fib_dsi_rec, libfibers), Cint,
      (Cint, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32},
       Ptr{Float32}, Cint, Ptr{Int32}, Cint, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Ptr{Float32}}, Ptr{Ptr{Float32}}),
      device, vol, nx, ny, nz, nvol, m, FIB_DTYPE[eltype(m)] | FIB_MASK_OUTPUTS_ZEROED, dwi.bval, dwi.bvec,
      verts, size(verts, 1), faces, size(faces, 1), hann_width, pdf.vol, odf.vol, pk, pq))
  return DSI(pdf, odf, peak, qa)
end

# layout: fib_rumba_out sizeof 80: fodf@0 fgm@8 fcsf@16 gfa@24 var@32 peak@40
struct FibRumbaOut
  fodf::Ptr{Float32}; fgm::Ptr{Float32}; fcsf::Ptr{Float32}; gfa::Ptr{Float32}; var::Ptr{Float32}
  peak::NTuple{5, Ptr{Float32}}
end

"st_eigen(Sxx, Sxy, Sxz, Syy, Syz, Szz) — replaces structens.jl:13-37"
function st_eigen(Sxx::Array{Float32,3}, Sxy::Array{Float32,3}, Sxz::Array{Float32,3},
                  Syy::Array{Float32,3}, Syz::Array{Float32,3}, Szz::Array{Float32,3}; device::Integer=0)
  eigvec = Array{Float32,5}(undef, size(Sxx)..., 3, 3)
  eigval = Array{Float32,4}(undef, size(Sxx)..., 3)
  S = [pointer(Sxx), pointer(Sxy), pointer(Sxz), pointer(Syy), pointer(Syz), pointer(Szz)]
  GC.@preserve Sxx Sxy Sxz Syy Syz Szz S eigvec eigval fib_check(ccall((:fib_st_eigen, libfibers), Cint,
      (Cint, Ptr{Ptr{Cfloat}}, Int64, Ptr{Cfloat}, Ptr{Cfloat}), device, S, length(Sxx), eigvec, eigval))
  return eigvec, eigval
end

"st_recon(vol, sigma, rho) — replaces structens.jl:40-88 (sigma, rho <= 8; each stage skipped when <= 0)"
function st_recon(vol::Array{Float32,3}, sigma::Number, rho::Number; device::Integer=0)
  nx, ny, nz = size(vol)
  eigvec = Array{Float32,5}(undef, nx, ny, nz, 3, 3)
  eigval = Array{Float32,4}(undef, nx, ny, nz, 3)
  GC.@preserve vol eigvec eigval fib_check(ccall((:fib_st_recon, libfibers), Cint,
      (Cint, Ptr{Cfloat}, Cint, Cint, Cint, Cfloat, Cfloat, Ptr{Cfloat}, Ptr{Cfloat}), device, vol, nx, ny, nz, sigma, rho, eigvec, eigval))
  return eigvec, eigval
end

"Container for outputs of dwi_denoise: the denoised series, the noise level and the number of components kept per voxel"
struct Denoised
  dwi::MRI; sigma::MRI; rank::MRI
end

"dwi_denoise(dwi, mask; patch, estimator) — Marchenko-Pastur PCA denoising (not in the reference; include/fibers_hip.h).
 patch in (3, 5, 7); estimator :exp1 or :exp2.  The mask is read as nonzero = inside."
function dwi_denoise(dwi::MRI, mask::MRI; patch::Integer=5, estimator::Symbol=:exp2, device::Integer=0)
  nx, ny, nz, nvol = size(dwi.vol)
  est = estimator == :exp1 ? 1 : estimator == :exp2 ? 2 : error("estimator must be :exp1 or :exp2")
  fib_check(ccall((:fib_dwi_denoise_check, libfibers), Cint, (Cint, Cint, Cint, Cint, Cint, Cint), nx, ny, nz, nvol, patch, est))
  vol = dwi.vol::Array{Float32,4}
  m = UInt8.(view(mask.vol, :, :, :, 1) .!= 0)
  out = Array{Float32,4}(undef, nx, ny, nz, nvol)
  S = MRI(mask, 1, Float32); R = MRI(mask, 1, Float32)
  GC.@preserve vol m out S R fib_check(ccall((:fib_dwi_denoise, libfibers), Cint,
      (Cint, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{UInt8}, Cint, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
      device, vol, nx, ny, nz, nvol, m, patch, est, out, pointer(S.vol), pointer(R.vol)))
  D = deepcopy(dwi)
  D.vol = out
  return Denoised(D, S, R)
end

# layout: fib_mask_params sizeof 16: radius@0 numpass@4 flags@8 dilate@12
struct FibMaskParams
  radius::Cint; numpass::Cint; flags::Cint; dilate::Cint
end
# layout: fib_mask_info sizeof 64: status@0 kstar@4 lo@8 hi@12 threshold@16 n_above@24 n_components@32 n_kept@40 n_filled@48 n_mask@56
mutable struct FibMaskInfo
  status::Int32; kstar::Int32; lo::Float32; hi::Float32; threshold::Float64
  n_above::Int64; n_components::Int64; n_kept::Int64; n_filled::Int64; n_mask::Int64
  FibMaskInfo() = new(0, 0, 0f0, 0f0, 0.0, 0, 0, 0, 0, 0)
end
mask_flags(keep_largest::Bool, fill_holes::Bool) = Cint((keep_largest ? 1 : 0) | (fill_holes ? 2 : 0))

"Container for outputs of dwi_mask: the mask (UInt8), the mean of the chosen frames and the info record"
struct BrainMask
  mask::MRI; b0::MRI; info::FibMaskInfo
end

"dwi_mask(dwi; frames, radius, numpass, keep_largest, fill_holes, dilate) — median-Otsu brain mask (not in the reference;
 include/fibers_hip.h).  frames are 1-based; the default is the frames of the smallest b-value (dti.jl:117), frame 1 without a b-table."
function dwi_mask(dwi::MRI; frames::Union{Nothing,Vector{<:Integer}}=nothing, radius::Integer=2, numpass::Integer=4,
                  keep_largest::Bool=true, fill_holes::Bool=true, dilate::Integer=0, device::Integer=0)
  nx, ny, nz, nvol = size(dwi.vol)
  fr = frames !== nothing ? Int32.(frames .- 1) : isempty(dwi.bval) ? Int32[0] : Int32.(findall(dwi.bval .== minimum(dwi.bval)) .- 1)
  p = FibMaskParams(radius, numpass, mask_flags(keep_largest, fill_holes), dilate)
  vol = dwi.vol::Array{Float32,4}
  M = MRI(dwi, 1, UInt8); B = MRI(dwi, 1, Float32)
  info = FibMaskInfo()
  GC.@preserve vol fr M B fib_check(ccall((:fib_dwi_mask, libfibers), Cint,
      (Cint, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Int32}, Cint, Ref{FibMaskParams}, Ptr{UInt8}, Ptr{Float32}, Ref{FibMaskInfo}),
      device, vol, nx, ny, nz, nvol, fr, length(fr), p, pointer(M.vol), pointer(B.vol), info))
  return BrainMask(M, B, info)
end

"vol_median(mri; radius, numpass) — the 3-D median of every frame, window (2 radius + 1)^3 with edge replication"
function vol_median(mri::MRI; radius::Integer=1, numpass::Integer=1, device::Integer=0)
  nx, ny, nz, nf = size(mri.vol)
  vol = mri.vol::Array{Float32,4}
  out = Array{Float32,4}(undef, nx, ny, nz, nf)
  GC.@preserve vol out fib_check(ccall((:fib_vol_median, libfibers), Cint,
      (Cint, Ptr{Float32}, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float32}),
      device, vol, nx, ny, nz, nf, radius, numpass, out))
  D = deepcopy(mri)
  D.vol = out
  return D
end

# layout: fib_degibbs_params sizeof 16: slice_axis@0 nshifts@4 minW@8 maxW@12
struct FibDegibbsParams
  slice_axis::Cint; nshifts::Cint; minW::Cint; maxW::Cint
end

"Container for outputs of dwi_degibbs: the unrung series and, with shifts=true, the chosen candidates along the two in-plane axes"
struct Degibbsed
  dwi::MRI; shift_u::Union{Nothing,Array{Int8,4}}; shift_v::Union{Nothing,Array{Int8,4}}
end

"dwi_degibbs(dwi; slice_axis, nshifts, min_w, max_w, shifts) — Gibbs-ringing removal by local subvoxel shifts (not in the reference;
 include/fibers_hip.h).  slice_axis is 1-based (3: slices across z); 1 <= nshifts <= 32, 1 <= min_w <= max_w <= 6."
function dwi_degibbs(dwi::MRI; slice_axis::Integer=3, nshifts::Integer=20, min_w::Integer=1, max_w::Integer=3, shifts::Bool=false,
                     device::Integer=0)
  nx, ny, nz, nvol = size(dwi.vol)
  p = FibDegibbsParams(slice_axis - 1, nshifts, min_w, max_w)
  fib_check(ccall((:fib_dwi_degibbs_check, libfibers), Cint, (Cint, Cint, Cint, Cint, Ref{FibDegibbsParams}), nx, ny, nz, nvol, p))
  vol = dwi.vol::Array{Float32,4}
  out = Array{Float32,4}(undef, nx, ny, nz, nvol)
  su = shifts ? Array{Int8,4}(undef, nx, ny, nz, nvol) : nothing
  sv = shifts ? Array{Int8,4}(undef, nx, ny, nz, nvol) : nothing
  GC.@preserve vol out su sv fib_check(ccall((:fib_dwi_degibbs, libfibers), Cint,
      (Cint, Ptr{Float32}, Cint, Cint, Cint, Cint, Ref{FibDegibbsParams}, Ptr{Float32}, Ptr{Int8}, Ptr{Int8}),
      device, vol, nx, ny, nz, nvol, p, out, shifts ? pointer(su) : C_NULL, shifts ? pointer(sv) : C_NULL))
  D = deepcopy(dwi)
  D.vol = out
  return Degibbsed(D, su, sv)
end

"mask_components(mask; keep_largest, fill_holes, compact) — Int32 labels of the 6-connected components of mask .!= 0 (after the selection
 and the holes); a label is 1 + the smallest 0-based linear index of its component, compact=true renumbers them 1..n in that order"
function mask_components(mask::MRI; keep_largest::Bool=false, fill_holes::Bool=false, compact::Bool=true, device::Integer=0)
  nx, ny, nz = size(mask.vol)[1:3]
  m = UInt8.(view(mask.vol, :, :, :, 1) .!= 0)
  L = MRI(mask, 1, Int32)
  info = FibMaskInfo()
  GC.@preserve m L fib_check(ccall((:fib_mask_components, libfibers), Cint,
      (Cint, Ptr{UInt8}, Cint, Cint, Cint, Cint, Ptr{Int32}, Ptr{UInt8}, Ref{FibMaskInfo}),
      device, m, nx, ny, nz, mask_flags(keep_largest, fill_holes), pointer(L.vol), C_NULL, info))
  if compact
    u = sort(unique(filter(!=(0), L.vol)))
    rank = Dict(v => Int32(i) for (i, v) in enumerate(u))
    L.vol = map(v -> v == 0 ? Int32(0) : rank[v], L.vol)
  end
  return L
end

"rumba_rec(dwi, mask, odf_dirs, niter, ...) — replaces rusd.jl:419-636"
function rumba_rec(dwi::MRI, mask::MRI, odf_dirs::ODF=sphere_724, niter::Integer=600, λ_para::Float32=Float32(1.7e-3),
                   λ_perp::Float32=Float32(0.2e-3), λ_csf::Float32=Float32(3.0e-3), λ_gm::Float32=Float32(0.8e-4),
                   ncoils::Integer=1, coil_combine::String="SMF-SENSE", ipat_factor::Integer=1, use_tv::Bool=true;
                   device::Integer=0)
  isempty(dwi.bval) && error("Missing b-value table from input DWI structure")
  isempty(dwi.bvec) && error("Missing gradient table from input DWI structure")
  sos = coil_combine == "SoS-GRAPPA" ? 1 : (coil_combine == "SMF-SENSE" ? 0 : error("Unknown coil combine mode " * coil_combine))
  ipat_factor < 1 && error("iPAT factor must be a positive integer")
  nx, ny, nz, nvol = size(dwi.vol)
  nvert = div(size(odf_dirs.vertices, 1), 2)
  fodf = MRI(mask, nvert, Float32); fgm = MRI(mask, 1, Float32); fcsf = MRI(mask, 1, Float32)
  gfa = MRI(mask, 1, Float32); var = MRI(mask, 1, Float32); peak = [MRI(mask, 3, Float32) for _ in 1:5]
  verts = odf_dirs.vertices; vol = dwi.vol::Array{Float32,4}; m = mask.vol
  snr = Ref{Float32}(0); snrsd = Ref{Float32}(0)
  out = Ref(FibRumbaOut(pointer(fodf.vol), pointer(fgm.vol), pointer(fcsf.vol), pointer(gfa.vol), pointer(var.vol),
                        ntuple(i -> pointer(peak[i].vol), 5)))
  GC.@preserve vol m fodf fgm fcsf gfa var peak verts fib_check(ccall((:fib_rumba_rec, libfibers), Cint,
      (Cint, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cint, Cint,
       Cfloat, Cfloat, Cfloat, Cfloat, Cint, Cint, Cint, Cint, Ref{FibRumbaOut}, Ref{Float32}, Ref{Float32}),
      device, vol, nx, ny, nz, nvol, m, FIB_DTYPE[eltype(m)], dwi.bval, dwi.bvec, verts, size(verts, 1), niter,
      λ_para, λ_perp, λ_csf, λ_gm, ncoils, sos, ipat_factor, use_tv ? 1 : 0, out, snr, snrsd))
  return RUMBASD(fodf, fgm, fcsf, peak, gfa, var, snr[], snrsd[])
end

# layout: fib_stream_params sizeof 64: nx@0 ny@4 nz@8 nvec@12 len_min@16 len_max@20 cosang_thresh@24 step_size@28 smooth_coeff@32 search_dist@36 search_cosang@40 ws@48 interp@56 search_flat_axis@60
struct FibStreamParams
  nx::Int32; ny::Int32; nz::Int32; nvec::Int32; len_min::Int32; len_max::Int32
  cosang_thresh::Float32; step_size::Float32; smooth_coeff::Float32
  search_dist::Int32; search_cosang::Float32          # microscopy regime (stream.jl:83, 547-619) when search_dist > 0
  ws::Ptr{Cvoid}                                      # optional tracer workspace (fibd_stream_ws_create); C_NULL for the host-buffer calls
  interp::Int32                                       # FIB_STREAM_*: 0 nearest voxel (stream.jl:514); 1 trilinear blend, 2 / 3 the same stepped by RK2 / RK4 (not in the reference)
  search_flat_axis::Int32                             # microscopy regime + 2-D angle inputs: 1..3 = the through-plane axis (search distance 0, stream.jl:153-155); 0: none
end

# layout: fib_tract_out sizeof 48: nlines@0 npoints@8 npts@16 seed_index@24 xyz@32 flags@40
mutable struct FibTractOut
  nlines::Int64; npoints::Int64
  npts::Ptr{Int32}; seed_index::Ptr{Int64}; xyz::Ptr{Float32}; flags::Ptr{UInt8}
  FibTractOut() = new(0, 0, C_NULL, C_NULL, C_NULL, C_NULL)
end

"stream(ovec; ...) — replaces stream.jl:730-790 for the angle-picking path and the microscopy regime (no lcms)"
function stream(ovec::Union{MRI,Vector{MRI}}; f::Union{MRI,Vector{MRI},Nothing}=nothing, f_thresh::Real=.03,
                fa::Union{MRI,Nothing}=nothing, fa_thresh::Real=.1, mask::Union{MRI,Nothing}=nothing,
                seed::Union{MRI,Nothing}=nothing, nsub::Union{Integer,Nothing}=3, len_min::Integer=3,
                len_max::Integer=(isa(ovec,MRI) ? maximum(ovec.volsize) : maximum(ovec[1].volsize)),
                ang_thresh::Union{Real,Nothing}=45, step_size::Union{Real,Nothing}=.5,
                smooth_coeff::Union{Real,Nothing}=.2, search_dist::Integer=15, search_ang::Real=10,
                lcms::Union{MRI,Nothing}=nothing, lcm_thresh::Real=.099, rng_seed::Integer=rand(UInt64),
                device::Integer=0, interp::Symbol=:nearest, integrator::Symbol=:euler)
  ovecs = isa(ovec, MRI) ? MRI[ovec] : ovec
  fs    = isa(f, MRI) ? MRI[f] : f
  # interp = :trilinear and integrator = :rk2 | :rk4 are NOT in the reference (fib_stream_params.interp in include/fibers_hip.h)
  interp in (:nearest, :trilinear) || error("interp must be :nearest or :trilinear")
  integrator in (:euler, :rk2, :rk4) || error("integrator must be :euler, :rk2 or :rk4")
  interp == :nearest && integrator != :euler && error("integrator $(integrator) needs interp = :trilinear")
  interp_code = interp == :nearest ? FIB_STREAM_NEAREST :
                integrator == :euler ? FIB_STREAM_TRILINEAR : integrator == :rk2 ? FIB_STREAM_TRILINEAR_RK2 : FIB_STREAM_TRILINEAR_RK4
  nx, ny, nz = size(ovecs[1].vol)[1:3]
  # 2-D orientation angles (one frame) become 3-D vectors here, with the reference's own arithmetic (stream.jl:147-172):
  # through-plane = the dimension with the largest voxel size, cos / sin (radians) or cosd / sind (degrees) in the other two
  flat_axis = Int32(0)
  lcm_frames = size(ovecs[1].vol, 4)                                        # what stream.jl:221 looks at (BEFORE the expansion)
  lcm_zero = [all(x -> x == 0, view(ovecs[1].vol, :, :, :, c)) for c in 1:lcm_frames]
  ovecs = map(ovecs) do o
    size(o.vol, 4) == 3 && return o
    size(o.vol, 4) == 1 || error("Input orientations should be 3D vectors or angles ∊ [-90, 90]")
    thrudim = argmax(o.volres); strdims = setdiff(1:3, thrudim)
    flat_axis = Int32(thrudim)
    a = view(o.vol, :, :, :, 1)
    v = zeros(Float32, nx, ny, nz, 3)
    if -π/2-eps(Float32) <= minimum(a) && maximum(a) <= π/2+eps(Float32)
      v[:, :, :, strdims[1]] .= cos.(a);  v[:, :, :, strdims[2]] .= sin.(a)
    elseif -90 <= minimum(a) && maximum(a) <= 90
      v[:, :, :, strdims[1]] .= cosd.(a); v[:, :, :, strdims[2]] .= sind.(a)
    else
      error("Input orientations should be 3D vectors or angles ∊ [-90, 90]")
    end
    e = MRI(o, 3, Float32); e.vol .= v
    e
  end
  if !isnothing(seed) && size(seed.vol) != size(mask.vol)
    error("Dimension mismatch between seed mask " * string(size(seed.vol)) * " and brain mask " * string(size(mask.vol)))
  end
  domicro = minimum(ovecs[1].volres) <= 0.05                                # stream.jl:83
  isnothing(nsub) && (nsub = domicro ? 0 : 3); isnothing(ang_thresh) && (ang_thresh = domicro ? 20 : 45)   # :89-92
  isnothing(step_size) && (step_size = domicro ? 1 : .5); isnothing(smooth_coeff) && (smooth_coeff = domicro ? 0 : .2)
  # sub-voxel offsets from the GLOBAL RNG, exactly as stream.jl:176-181
  sublist = nsub > 0 ? hcat([Float32.(rand(Uniform(-.5+eps(), .5-eps()), 3)) for _ in 1:nsub]...) : zeros(Float32, 3, 1)
  prm = Ref(FibStreamParams(nx, ny, nz, length(ovecs), len_min, len_max,
                            cosd(Float32(ang_thresh)), Float32(step_size), Float32(smooth_coeff),
                            domicro ? Int32(search_dist) : Int32(0), cosd(Float32(search_ang)), C_NULL, interp_code,
                            domicro ? flat_axis : Int32(0)))                   # micro_search_dist[thrudim] = 0, stream.jl:153-155
  pv = [pointer(o.vol) for o in ovecs]
  pf = isnothing(fs) ? C_NULL : [pointer(x.vol) for x in fs]
  out = FibTractOut()
  if !isnothing(lcms)     # LCM-guided tracking (stream.jl:380-495); the library's uniform stream replaces the global RNG
    lv = lcms.vol::Array{Float32,4}
    GC.@preserve ovecs fs fa mask seed sublist pv pf lv fib_check(ccall((:fib_stream_lcm, libfibers), Cint,
      (Cint, Ref{FibStreamParams}, Ptr{Ptr{Float32}}, Ptr{Ptr{Float32}}, Cfloat, Ptr{Float32}, Cfloat,
       Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Ptr{Float32}, Cint, Ptr{Float32}, Cfloat, UInt64, Ref{FibTractOut}),
      device, prm, pv, pf, Float32(f_thresh), isnothing(fa) ? C_NULL : pointer(fa.vol), Float32(fa_thresh),
      isnothing(mask) ? C_NULL : pointer(mask.vol), isnothing(mask) ? 0 : FIB_DTYPE[eltype(mask.vol)],
      isnothing(seed) ? C_NULL : pointer(seed.vol), isnothing(seed) ? 0 : FIB_DTYPE[eltype(seed.vol)],
      sublist, size(sublist, 2), lv, Float32(lcm_thresh), UInt64(rng_seed), out))
  else
  GC.@preserve ovecs fs fa mask seed sublist pv pf fib_check(ccall((:fib_stream, libfibers), Cint,
      (Cint, Ref{FibStreamParams}, Ptr{Ptr{Float32}}, Ptr{Ptr{Float32}}, Cfloat, Ptr{Float32}, Cfloat,
       Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Ptr{Float32}, Cint, Ref{FibTractOut}),
      device, prm, pv, pf, Float32(f_thresh), isnothing(fa) ? C_NULL : pointer(fa.vol), Float32(fa_thresh),
      isnothing(mask) ? C_NULL : pointer(mask.vol), isnothing(mask) ? 0 : FIB_DTYPE[eltype(mask.vol)],
      isnothing(seed) ? C_NULL : pointer(seed.vol), isnothing(seed) ? 0 : FIB_DTYPE[eltype(seed.vol)],
      sublist, size(sublist, 2), out))
  end
  npts = unsafe_wrap(Array, out.npts, out.nlines)
  xyz  = unsafe_wrap(Array, out.xyz, (3, Int(out.npoints)))
  off  = cumsum(vcat(0, Int.(npts)))
  str  = [xyz[:, off[i]+1:off[i+1]] for i in 1:length(npts)]          # Vector{Matrix{Float32}} [3 x npts]
  flag = isnothing(lcms) ? nothing :
         (fl = unsafe_wrap(Array, out.flags, Int(out.npoints)); [Float32.(fl[off[i]+1:off[i+1]]) for i in 1:length(npts)])
  ccall((:fib_tract_free, libfibers), Cvoid, (Ref{FibTractOut},), out)
  tr = Tract{Float32}(mask)
  str_add!(tr, str, flag)                                             # stream.jl:784-787
  return tr
end

"xfm_apply(xfm, point) — replaces util.jl:385-420 for Float32 points (a 3N vector or 3 x N matrix); vox2vox goes to the C ABI row-major"
function xfm_apply(xfm::Xform{Float32}, point::Array{Float32}; device::Integer=0)
  length(point) % 3 == 0 || error("xfm_apply takes 3N coordinates")
  newpoint = similar(point)
  m = Matrix{Float32}(permutedims(xfm.vox2vox))
  GC.@preserve m point newpoint fib_check(ccall((:fib_xfm_apply, libfibers), Cint,
      (Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int64), device, m, point, newpoint, length(point) ÷ 3))
  return newpoint
end

"str_xform(xfm, tr) — replaces trk.jl:316-347: the points of every line go through ONE fib_xfm_apply call, packed and unpacked"
function str_xform(xfm::Xform{Float32}, tr::Tract{Float32}; device::Integer=0)
  trnew = Tract{Float32}()
  for var in setdiff(fieldnames(Tract), (:dim, :voxel_size, :vox_to_ras, :image_orientation_patient, :xyz))
    setfield!(trnew, var, getfield(tr, var))
  end
  trnew.dim = Int16.(xfm.outsize)
  trnew.voxel_size = Float32.(xfm.outres)
  trnew.vox_to_ras = Float32.(xfm.outvox2ras)
  orient = vox2ras_to_orient(trnew.vox_to_ras)
  trnew.voxel_order          = vcat(UInt8.(collect(orient)), UInt8(0))
  trnew.voxel_order_original = trnew.voxel_order
  p2s = [-1 0 0; 0 -1 0; 0 0 1] * trnew.vox_to_ras[1:3, 1:2] * Diagonal([1, 1]./trnew.voxel_size[1:2])
  trnew.image_orientation_patient = Float32.(p2s[:])
  n   = [size(x, 2) for x in tr.xyz]
  off = cumsum(vcat(0, n))
  packed = isempty(n) ? Matrix{Float32}(undef, 3, 0) : reduce(hcat, tr.xyz)          # 3 x total: x, y, z of a point adjacent
  moved  = xfm_apply(xfm, packed; device=device)
  trnew.xyz = [moved[:, off[i]+1:off[i+1]] for i in 1:length(n)]
  return trnew
end

# ---- volume resampling (NOT in the reference; the definitions are the "Volume resampling" section of include/fibers_hip.h) ---------
const FIB_VOL_INTERP = Dict(:nearest => 0, :trilinear => 1)

"the output -> input matrix of vol_xform, row-major for the C ABI: Float32(inv(Float64(vox2vox))), rounded once"
vol_xform_matrix(xfm::Xform{Float32}) = Matrix{Float32}(permutedims(Float32.(inv(Float64.(xfm.vox2vox)))))

function vol_xform_call(xfm::Xform{Float32}, vol::Array{T,4}, interp::Symbol, bits::Int32, device::Integer) where T<:Union{Float32,Int32}
  haskey(FIB_VOL_INTERP, interp) || error("interp must be :nearest or :trilinear")
  collect(size(vol)[1:3]) == collect(xfm.insize) || error("the volume is " * string(size(vol)[1:3]) * " but the transform's input space is " * string(xfm.insize))
  nxi, nyi, nzi, nf = size(vol)
  nxo, nyo, nzo = Int.(xfm.outsize)
  out = Array{T,4}(undef, nxo, nyo, nzo, nf)
  m = vol_xform_matrix(xfm)
  GC.@preserve m vol out fib_check(ccall((:fib_vol_xform, libfibers), Cint,
      (Cint, Ptr{Float32}, Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Int32, Ptr{Cvoid}, Cint, Cint, Cint),
      device, m, vol, nxi, nyi, nzi, nf, FIB_VOL_INTERP[interp], bits, out, nxo, nyo, nzo))
  return out
end

"vol_xform(xfm, vol) — a volume [nx, ny, nz, nframes] resampled onto the output grid of xfm (nearest voxel or trilinear; voxels whose
nearest input voxel does not exist get `outside`).  Gradient tables are not reoriented: that is the caller's business."
vol_xform(xfm::Xform{Float32}, vol::Array{Float32,4}; interp::Symbol=:trilinear, outside::Real=0f0, device::Integer=0) =
  vol_xform_call(xfm, vol, interp, reinterpret(Int32, Float32(outside)), device)
"vol_xform(xfm, labels) — Int32 volumes (label maps) go through nearest-voxel resampling only"
function vol_xform(xfm::Xform{Float32}, vol::Array{Int32,4}; interp::Symbol=:nearest, outside::Integer=0, device::Integer=0)
  interp == :nearest || error("Int32 volumes take interp=:nearest only")
  return vol_xform_call(xfm, vol, interp, Int32(outside), device)
end

# ---- registration (NOT in the reference; the definitions are the "Registration" section of include/fibers_hip.h) ------------------
const FIB_REG_TRACE_ROW = 29
rowmajor(m) = Matrix{Float32}(permutedims(Float32.(m)))        # a 4 x 4 matrix as the row-major float[16] of the C ABI
# an MRI's Float32 voxels as [nx, ny, nz, nframes]: MRI(ref, 1, T) and a one-frame file hold a 3-D array (mri.jl:251-252); same memory
vol4(v::Array{Float32}) = reshape(v, size(v, 1), size(v, 2), size(v, 3), size(v, 4))
# the rotational part of a vox2vox, U * Vt of its SVD (util.jl:265-267), kept in Float64
rot64(v2v) = (F = svd(Float64.(v2v[1:3, 1:3])); F.U * F.Vt)

"G(theta), fixed RAS -> moving RAS, Float64 4 x 4 (fib_reg_matrix)"
function reg_G(theta::Vector{Float64}, fixed::MRI, moving::MRI)
  G = Matrix{Float64}(undef, 4, 4)
  fv = rowmajor(fixed.vox2ras0); mv = rowmajor(moving.vox2ras0); fs = Int32.(collect(fixed.volsize[1:3]))
  GC.@preserve theta fv mv fs G fib_check(ccall((:fib_reg_matrix, libfibers), Cint,
      (Ptr{Float64}, Cint, Ptr{Float32}, Ptr{Int32}, Ptr{Float32}, Cint, Ptr{Float32}, Ptr{Float64}),
      theta, length(theta), fv, fs, mv, 0, C_NULL, G))
  return permutedims(G)
end

"the Xform of a registration result, in = moving, out = fixed: ras2ras = Float32(inv(G)), vox2vox = Float32(inv(V_fix) inv(G) V_mov)"
function reg_xform(theta::Vector{Float64}, moving::MRI, fixed::MRI)
  Gi = inv(reg_G(theta, fixed, moving))
  v2v = Float32.(inv(Float64.(fixed.vox2ras0)) * Gi * Float64.(moving.vox2ras0))
  return Xform{Float32}(collect(moving.volsize[1:3]), collect(fixed.volsize[1:3]), Float32.(moving.volres), Float32.(fixed.volres),
                        Float32.(moving.vox2ras0), Float32.(fixed.vox2ras0), v2v, Float32.(Gi), Float32.(rot64(v2v)))
end

"every frame of `vol` registered to frame 1 of `fixed` (fib_mri_register): (theta [12, N], cost [N], niter [N], trace [29, rows, N], resampled)"
function reg_call(vol::Array{Float32,4}, moving::MRI, fixed::MRI, dof::Integer, nbins::Integer, levels::Integer, resample::Bool, device::Integer)
  nf = size(vol, 4); rows = 400
  fvol = vol4(fixed.vol)
  ms = Int32.(collect(size(vol)[1:3])); fs = Int32.(collect(size(fvol)[1:3])); fres = Float32.(collect(fixed.volres))
  mv = rowmajor(moving.vox2ras0); fv = rowmajor(fixed.vox2ras0)
  theta = zeros(Float64, 12, nf); cost = zeros(Float64, nf); niter = zeros(Int32, nf); trace = Array{Float64,3}(undef, FIB_REG_TRACE_ROW, rows, nf)
  out = resample ? Array{Float32,4}(undef, fs[1], fs[2], fs[3], nf) : Array{Float32,4}(undef, 0, 0, 0, 0)
  GC.@preserve vol fvol ms fs fres mv fv theta cost niter trace out fib_check(ccall((:fib_mri_register, libfibers), Cint,
      (Cint, Ptr{Float32}, Ptr{Int32}, Ptr{Float32}, Cint, Ptr{Float32}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Cint, Cint, Cint, Cint, Cint, Cdouble,
       Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Cint, Ptr{Float32}),
      device, vol, ms, mv, nf, fvol, fs, fres, fv, dof, nbins, levels, 4, 80, 0.5,
      theta, cost, niter, trace, rows, resample ? pointer(out) : Ptr{Float32}(C_NULL)))
  return theta, cost, niter, trace, out
end

"mri_register(moving, fixed; dof, nbins, levels, frame) — rigid (dof 6) or affine (dof 12) registration by normalised mutual information;
returns (xfm, theta, cost, trace): mri_xform / vol_xform through `xfm` puts the moving volume on the fixed grid.  levels = 0: the default."
function mri_register(moving::MRI, fixed::MRI; dof::Integer=6, nbins::Integer=32, levels::Integer=0, frame::Integer=1, device::Integer=0)
  vol = vol4(moving.vol)[:, :, :, frame:frame]
  theta, cost, niter, trace, _ = reg_call(vol, moving, fixed, dof, nbins, levels, false, device)
  th = theta[1:dof, 1]
  return (xfm = reg_xform(th, moving, fixed), theta = th, cost = cost[1], trace = trace[:, 1:niter[1], 1])
end

"dwi_moco(dwi; target, nbins, levels) — every frame registered (dof 6) to `target` (default: the Float64 mean of the frames of the
smallest b-value) and resampled onto its grid, trilinear, 0 outside; bvec rows rotated by the rotational part of their frame's transform
(U * Vt of the SVD of vox2vox in Float64, applied in Float64, rounded once: what fibers_jl_amd.register.rotate_bvec does).
Returns (dwi, theta, xfm, cost)."
function dwi_moco(dwi::MRI; target::Union{MRI,Nothing}=nothing, nbins::Integer=32, levels::Integer=0, device::Integer=0)
  vol = vol4(dwi.vol)
  if target === nothing
    fr = isempty(dwi.bval) ? [1] : findall(dwi.bval .== minimum(dwi.bval))
    acc = zeros(Float64, size(vol)[1:3])
    for f in fr; acc .+= Float64.(view(vol, :, :, :, f)); end
    target = MRI(dwi, 1, Float32)
    target.vol = Float32.(acc ./ length(fr))                        # (3-D, as MRI(dwi, 1, Float32) holds it)
  end
  theta, cost, _, _, out = reg_call(vol, dwi, target, 6, nbins, levels, true, device)
  nf = size(vol, 4)
  xfms = [reg_xform(theta[1:6, f], dwi, target) for f in 1:nf]
  moved = MRI(target, nf, Float32)
  moved.vol = nf == 1 ? out[:, :, :, 1] : out                     # (MRI(target, 1, Float32) holds a 3-D array)
  moved.bval = copy(dwi.bval)
  moved.bvec = isempty(dwi.bvec) ? copy(dwi.bvec) : Float32.(reduce(vcat, [(rot64(xfms[f].vox2vox) * Float64.(dwi.bvec[f, :]))' for f in 1:nf]))
  return (dwi = moved, theta = theta[1:6, :], xfm = xfms, cost = cost)
end

# ---- non-linear warps (NOT in the reference; the definitions are the "Non-linear warps" section of include/fibers_hip.h) -----------
# A field is a Float32 array [nx, ny, nz, 3] (the displacement in mm, RAS) with the vox2ras of its grid.  Matrices are made in Float64
# from the Float32 fields, rounded once, and go to the C ABI row-major.
warp_rowmajor(m) = Matrix{Float32}(permutedims(Float32.(m)))
warp_shift(v) = [1.0 0 0 v; 0 1 0 v; 0 0 1 v; 0 0 0 1]

"str_warp(field, field_vox2ras, tr, out_vox2ras) — the lines of tr through phi(x) = x + d(x): tract volume -> (pre_ras2ras) -> the
field's space -> phi -> (post_ras2ras) -> the volume of out_vox2ras.  `origin` is the index of the first voxel's centre in the tract's
coordinates (1 for what `stream` makes).  Returns the moved lines; the header of the new Tract is the caller's to fill from the output
volume, as str_xform does."
function str_warp(field::Array{Float32,4}, field_vox2ras::Matrix{Float32}, tr::Tract{Float32}, out_vox2ras::Matrix{Float32};
                  pre_ras2ras=Matrix{Float64}(I, 4, 4), post_ras2ras=Matrix{Float64}(I, 4, 4), origin::Real=1, device::Integer=0)
  size(field, 4) == 3 || error("a displacement field has 3 frames")
  to_ras   = Float64.(pre_ras2ras) * Float64.(tr.vox_to_ras) * warp_shift(-Float64(origin))
  to_field = inv(Float64.(field_vox2ras)) * to_ras
  from_ras = warp_shift(Float64(origin)) * inv(Float64.(out_vox2ras)) * Float64.(post_ras2ras)
  a, q, b = warp_rowmajor(to_ras), warp_rowmajor(to_field), warp_rowmajor(from_ras)
  n   = [size(x, 2) for x in tr.xyz]
  off = cumsum(vcat(0, n))
  packed = isempty(n) ? Matrix{Float32}(undef, 3, 0) : reduce(hcat, tr.xyz)
  moved  = similar(packed)
  nx, ny, nz = size(field)[1:3]
  GC.@preserve field a q b packed moved fib_check(ccall((:fib_warp_points, libfibers), Cint,
      (Cint, Ptr{Float32}, Cint, Cint, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int64),
      device, field, nx, ny, nz, a, q, b, packed, moved, size(packed, 2)))
  return [moved[:, off[i]+1:off[i+1]] for i in 1:length(n)]
end

"mri_warp(field, field_vox2ras, vol, vol_vox2ras, outsize, out_vox2ras) — vol [nx, ny, nz, nframes] pulled back through the field onto
the grid (outsize, out_vox2ras): the sampling positions travel output voxel -> (pre) -> the field's space -> phi -> (post) -> vol's voxels"
function mri_warp(field::Array{Float32,4}, field_vox2ras::Matrix{Float32}, vol::Array{T,4}, vol_vox2ras::Matrix{Float32}, outsize,
                  out_vox2ras::Matrix{Float32}; interp::Symbol=(T == Float32 ? :trilinear : :nearest), outside::Real=0,
                  pre_ras2ras=Matrix{Float64}(I, 4, 4), post_ras2ras=Matrix{Float64}(I, 4, 4), device::Integer=0) where T<:Union{Float32,Int32}
  size(field, 4) == 3 || error("a displacement field has 3 frames")
  haskey(FIB_VOL_INTERP, interp) || error("interp must be :nearest or :trilinear")
  (T == Float32 || interp == :nearest) || error("Int32 volumes take interp=:nearest only")
  to_ras   = Float64.(pre_ras2ras) * Float64.(out_vox2ras)
  to_field = inv(Float64.(field_vox2ras)) * to_ras
  from_ras = inv(Float64.(vol_vox2ras)) * Float64.(post_ras2ras)
  a, q, b = warp_rowmajor(to_ras), warp_rowmajor(to_field), warp_rowmajor(from_ras)
  nx, ny, nz = size(field)[1:3]
  nxi, nyi, nzi, nf = size(vol)
  nxo, nyo, nzo = Int.(outsize)
  out  = Array{T,4}(undef, nxo, nyo, nzo, nf)
  bits = T == Float32 ? reinterpret(Int32, Float32(outside)) : Int32(outside)
  GC.@preserve field a q b vol out fib_check(ccall((:fib_warp_volume, libfibers), Cint,
      (Cint, Ptr{Float32}, Cint, Cint, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Int32,
       Ptr{Cvoid}, Cint, Cint, Cint),
      device, field, nx, ny, nz, a, q, b, vol, nxi, nyi, nzi, nf, FIB_VOL_INTERP[interp], bits, out, nxo, nyo, nzo))
  return out
end

"warp_invert(field, field_vox2ras, outsize, out_vox2ras) — (inv [nxo, nyo, nzo, 3], err [nxo, nyo, nzo]): the field of phi^-1 on the
output grid by niter fixed-point steps, and the residual max_c |x_c + d_c(x) - y_c| in mm at every voxel"
function warp_invert(field::Array{Float32,4}, field_vox2ras::Matrix{Float32}, outsize, out_vox2ras::Matrix{Float32};
                     niter::Integer=20, device::Integer=0)
  size(field, 4) == 3 || error("a displacement field has 3 frames")
  y, q = warp_rowmajor(out_vox2ras), warp_rowmajor(inv(Float64.(field_vox2ras)))
  nx, ny, nz = size(field)[1:3]
  nxo, nyo, nzo = Int.(outsize)
  invf = Array{Float32,4}(undef, nxo, nyo, nzo, 3)
  err  = Array{Float32,3}(undef, nxo, nyo, nzo)
  GC.@preserve field y q invf err fib_check(ccall((:fib_warp_invert, libfibers), Cint,
      (Cint, Ptr{Float32}, Cint, Cint, Cint, Ptr{Float32}, Ptr{Float32}, Cint, Ptr{Float32}, Ptr{Float32}, Cint, Cint, Cint),
      device, field, nx, ny, nz, y, q, niter, invf, err, nxo, nyo, nzo))
  return invf, err
end

# ---- non-linear registration (NOT in the reference; "Non-linear registration" in include/fibers_hip.h) -----------------------------
"mri_nlreg(moving, fixed; init, levels, niter, sigma, step, frame) — the displacement field (additive demons, a fixed number of
iterations per level) that takes `moving` onto `fixed`.  `init`: the Xform of mri_register(moving, fixed) (in = moving, out = fixed);
levels = 0: mri_register's default; niter: one count, or one per level from the coarsest; sigma in level voxels; step in mm (default: the
smallest fixed voxel size).  Returns (field [nx, ny, nz, 3] on the fixed grid, post_ras2ras (fixed RAS -> moving RAS, what mri_warp and
str_warp take with the field), warped [nx, ny, nz], cost [maxit, levels], count): warped equals mri_warp(field, fixed.vox2ras0, moving
frame, moving.vox2ras0, size(fixed), fixed.vox2ras0; post_ras2ras) bit for bit."
function mri_nlreg(moving::MRI, fixed::MRI; init::Union{Xform{Float32},Nothing}=nothing, levels::Integer=0, niter=30, sigma::Real=1.0,
                   step::Real=minimum(Float32.(fixed.volres)), frame::Integer=1, device::Integer=0)
  mvol = vol4(moving.vol)[:, :, :, frame:frame]; fvol = vol4(fixed.vol)[:, :, :, 1:1]
  ms = Int32.(collect(size(mvol)[1:3])); fs = Int32.(collect(size(fvol)[1:3]))
  mv = rowmajor(moving.vox2ras0); fv = rowmajor(fixed.vox2ras0)
  if levels == 0
    nl = Ref{Cint}(0)
    GC.@preserve fs ms fib_check(ccall((:fib_reg_levels, libfibers), Cint, (Ptr{Int32}, Ptr{Int32}, Ref{Cint}), fs, ms, nl))
    levels = Int(nl[])
  end
  n = niter isa Integer ? fill(Int32(niter), levels) : Int32.(collect(niter))
  length(n) == levels || error("niter holds $(length(n)) counts for a pyramid of $levels levels (one per level, coarsest first)")
  post64 = init === nothing ? Matrix{Float64}(I, 4, 4) : Float64.(Float32.(inv(Float64.(init.ras2ras))))
  post = rowmajor(post64)
  to_ras = Float64.(fixed.vox2ras0)
  mats = hcat(vec(permutedims(Float32.(to_ras))), vec(permutedims(Float32.(inv(Float64.(fixed.vox2ras0)) * to_ras))),
              vec(permutedims(Float32.(inv(Float64.(moving.vox2ras0)) * post64))))      # to_ras, to_field, from_ras of mri_warp, row-major
  width = max(1, Int(maximum(n)))
  field = Array{Float32,4}(undef, fs[1], fs[2], fs[3], 3); warped = Array{Float32,3}(undef, fs[1], fs[2], fs[3])
  cost = Matrix{Float64}(undef, width, levels); count = Matrix{Int64}(undef, width, levels)
  GC.@preserve mvol fvol ms fs mv fv post n field cost count mats warped fib_check(ccall((:fib_mri_nlreg, libfibers), Cint,
      (Cint, Ptr{Float32}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Cint, Ptr{Int32}, Cfloat, Cfloat,
       Ptr{Float32}, Ptr{Float64}, Ptr{Int64}, Ptr{Float32}, Ptr{Float32}),
      device, mvol, ms, mv, fvol, fs, fv, init === nothing ? Ptr{Float32}(C_NULL) : pointer(post), levels, n, Float32(sigma), Float32(step),
      field, cost, count, mats, warped))
  return (field = field, post_ras2ras = Float32.(post64), warped = warped, cost = cost, count = count)
end

"warp_jacobian(field, field_vox2ras) — det(I + dd/dx) [nx, ny, nz] of a displacement field: a value <= 0 marks a fold"
function warp_jacobian(field::Array{Float32,4}, field_vox2ras::Matrix{Float32}; device::Integer=0)
  size(field, 4) == 3 || error("a displacement field has 3 frames")
  linv = Matrix{Float32}(permutedims(Float32.(inv(Float64.(field_vox2ras[1:3, 1:3])))))     # row-major float[9]
  nx, ny, nz = size(field)[1:3]
  out = Array{Float32,3}(undef, nx, ny, nz)
  GC.@preserve field linv out fib_check(ccall((:fib_warp_jacobian, libfibers), Cint,
      (Cint, Ptr{Float32}, Cint, Cint, Cint, Ptr{Float32}, Ptr{Float32}),
      device, field, nx, ny, nz, linv, out))
  return out
end

# ---- tract maps (NOT in the reference; the definitions are the "Tract maps" section of include/fibers_hip.h) ----------------------
const FIB_DENSITY_MODES = Dict(:points => 0, :lines => 1, :endpoints => 2)
const FIB_DENSITY_ACCUMULATE = 0x100

"packed lines of a Tract: (xyz [3 x npoints], npts Int32[nlines])"
function str_packed(tr::Tract{Float32})
  npts = Int32[size(x, 2) for x in tr.xyz]
  xyz  = isempty(npts) ? Matrix{Float32}(undef, 3, 0) : reduce(hcat, tr.xyz)
  return xyz, npts
end

"""str_density(tr; mode = :lines | :points | :endpoints, dims, out) -> (D::Array{UInt32,3}, n_outside) — path density of a tractogram:
points per voxel, lines per voxel (each line once per voxel it visits), or line ends per voxel.  `out`: an earlier map to add to."""
function str_density(tr::Tract{Float32}; mode::Symbol=:lines, dims=Int.(tr.dim), out::Union{Array{UInt32,3},Nothing}=nothing, device::Integer=0)
  haskey(FIB_DENSITY_MODES, mode) || error("mode must be :points, :lines or :endpoints")
  xyz, npts = str_packed(tr)
  code = FIB_DENSITY_MODES[mode] | (isnothing(out) ? 0 : FIB_DENSITY_ACCUMULATE)
  D = isnothing(out) ? zeros(UInt32, dims[1], dims[2], dims[3]) : out
  nout = Ref{Int64}(0)
  GC.@preserve xyz npts D fib_check(ccall((:fib_str_density, libfibers), Cint,
      (Cint, Ptr{Float32}, Ptr{Int32}, Int64, Int64, Cint, Cint, Cint, Cint, Ptr{UInt32}, Ref{Int64}),
      device, xyz, npts, length(npts), size(xyz, 2), size(D, 1), size(D, 2), size(D, 3), code, D, nout))
  return D, nout[]
end

"str_sample(tr, vol; outside) -> one [nframes x npts] matrix per line (the layout of Tract.scalars): vol[:, :, :, f] at every point's nearest voxel"
function str_sample(tr::Tract{Float32}, vol::Array{Float32,4}; outside::Real=0, device::Integer=0)
  xyz, npts = str_packed(tr)
  nf = size(vol, 4)
  S = Matrix{Float32}(undef, nf, size(xyz, 2))
  GC.@preserve xyz vol S fib_check(ccall((:fib_str_sample, libfibers), Cint,
      (Cint, Ptr{Float32}, Int64, Ptr{Float32}, Cint, Cint, Cint, Cint, Cfloat, Ptr{Float32}),
      device, xyz, size(xyz, 2), vol, size(vol, 1), size(vol, 2), size(vol, 3), nf, Float32(outside), S))
  off = cumsum(vcat(0, Int.(npts)))
  return [S[:, off[i]+1:off[i+1]] for i in 1:length(npts)]
end

"str_stats(tr) -> [1 + n_scalars x nlines] (the layout of Tract.properties): length in mm, then the mean of every scalar along the line"
function str_stats(tr::Tract{Float32}; device::Integer=0)
  xyz, npts = str_packed(tr)
  ns = isempty(tr.scalars) ? 0 : size(tr.scalars[1], 1)
  sc = ns == 0 ? Matrix{Float32}(undef, 0, 0) : reduce(hcat, tr.scalars)          # [ns x npoints]: a point's scalars adjacent
  P = Matrix{Float32}(undef, 1 + ns, length(npts))
  res = Float32.(tr.voxel_size)
  GC.@preserve xyz npts sc P res fib_check(ccall((:fib_str_stats, libfibers), Cint,
      (Cint, Ptr{Float32}, Ptr{Int32}, Int64, Int64, Ptr{Float32}, Ptr{Float32}, Cint, Ptr{Float32}),
      device, xyz, npts, length(npts), size(xyz, 2), res, sc, ns, P))
  return P
end

# ---- tract selection and connectomes (NOT in the reference; "Tract selection and connectomes" in include/fibers_hip.h) --------------
const FIB_CONNECTOME_ACCUMULATE = 0x100

"the kept lines of a Tract (a host copy): xyz, scalars, properties of the lines whose flag is set, in order"
function str_take(tr::Tract{Float32}, keep::AbstractVector{Bool})
  trnew = deepcopy(tr)
  trnew.xyz = tr.xyz[keep]
  isempty(tr.scalars) || (trnew.scalars = tr.scalars[keep])
  isempty(tr.properties) || (trnew.properties = tr.properties[:, keep])
  trnew.npts = Int32[size(x, 2) for x in trnew.xyz]
  trnew.n_count = length(trnew.xyz)
  return trnew
end

"""str_select(tr; include, exclude, end_in, both_ends_in, min_npts, max_npts) -> Tract — the lines that pass through every volume of
`include` and none of `exclude`, have an end in every volume of `end_in` and both ends in every volume of `both_ends_in` (volumes:
`Array{UInt8,3}` of `tr.dim`, non-zero inside; 32 in all), with min_npts <= npts (<= max_npts unless 0).  Also returns keep and hits."""
function str_select(tr::Tract{Float32}; include=Array{UInt8,3}[], exclude=Array{UInt8,3}[], end_in=Array{UInt8,3}[], both_ends_in=Array{UInt8,3}[],
                    min_npts::Integer=0, max_npts::Integer=0, device::Integer=0)
  groups = (include, exclude, end_in, both_ends_in)
  rois = Array{UInt8,3}[r for g in groups for r in g]
  length(rois) <= 32 || error("one call takes 32 regions")
  masks, bit = UInt64[], 0
  for g in groups
    push!(masks, reduce(|, (UInt64(1) << (bit + k - 1) for k in 1:length(g)); init=UInt64(0)))
    bit += length(g)
  end
  xyz, npts = str_packed(tr)
  dims = Int.(tr.dim)
  keep = Vector{UInt8}(undef, length(npts))
  hits = Matrix{UInt32}(undef, 3, length(npts))
  counts = zeros(Int64, 2)
  ptrs = Ptr{UInt8}[pointer(r) for r in rois]
  GC.@preserve xyz npts rois ptrs keep hits counts fib_check(ccall((:fib_str_select, libfibers), Cint,
      (Cint, Ptr{Float32}, Ptr{Int32}, Int64, Int64, Cint, Cint, Cint, Ptr{Ptr{UInt8}}, Cint, UInt64, UInt64, UInt64, UInt64, Int32, Int32,
       Ptr{UInt8}, Ptr{UInt32}, Ptr{Int64}),
      device, xyz, npts, length(npts), size(xyz, 2), dims[1], dims[2], dims[3], ptrs, length(rois), masks[1], masks[2], masks[3], masks[4],
      min_npts, max_npts, keep, hits, counts))
  return str_take(tr, keep .!= 0), keep, hits
end

"""str_connectome(tr, labels; ids, lengths) -> (C::Matrix{UInt32}, mean_length::Matrix{Float64}, ids, assign) — lines between every pair
of nodes of the label volume (`Array{Int32,3}` of `tr.dim`), and their mean length in mm; node k = ids[k], row / column 1 of the
matrices (node 0) holds the ends that are outside or in no node."""
function str_connectome(tr::Tract{Float32}, labels::Array{Int32,3}; ids=sort(unique(labels[labels .> 0])), lengths::Bool=true, device::Integer=0)
  L = length(ids)
  remap = zeros(Int32, maximum(ids) + 1)
  for (k, v) in enumerate(ids); remap[v + 1] = k; end
  xyz, npts = str_packed(tr)
  Cm = zeros(UInt32, L + 1, L + 1)
  W = zeros(Float64, L + 1, L + 1)
  assign = Matrix{Int32}(undef, 2, length(npts))
  nl = Ref{Int64}(0)
  res = Float32.(tr.voxel_size)
  GC.@preserve xyz npts labels remap Cm W assign res fib_check(ccall((:fib_str_connectome, libfibers), Cint,
      (Cint, Ptr{Float32}, Ptr{Int32}, Int64, Int64, Cint, Cint, Cint, Ptr{Float32}, Ptr{Int32}, Ptr{Int32}, Int64, Cint, Cint,
       Ptr{UInt32}, Ptr{Float64}, Ptr{Int32}, Ref{Int64}),
      device, xyz, npts, length(npts), size(xyz, 2), size(labels, 1), size(labels, 2), size(labels, 3), res, labels, remap, length(remap), L, 0,
      Cm, lengths ? pointer(W) : Ptr{Float64}(C_NULL), assign, nl))
  return Cm, (lengths ? map((w, c) -> c > 0 ? w / c : 0.0, W, Cm) : nothing), ids, assign
end

# ---- tractogram weights (NOT in the reference; "Tractogram weights" in include/fibers_hip.h) ----------------------------------------
"""str_weights(tr, peak, f; mask, f_thresh, ang_thresh, niter, q0) -> (weights, q, td, mu, cost, counts) — a weight per line such that the
weighted track density of every fixel (one peak in one voxel) matches the peak's amplitude.  `peak`: up to three `Array{Float32,4}`
[nx,ny,nz,3] (e.g. `gqi.peak[k].vol`), `f`: their amplitudes `Array{Float32,3}`.  The lines must have a uniform step (point counts
stand for lengths).  `niter` steps of ISRA from the weight 1 (or `q0`, UInt32 in units of 2^-20), not SIFT2's line search.  `counts` =
(points unassigned, lines without an assigned point, lines at the clamp, lines at q = 0, overflow); a non-zero overflow is an error."""
function str_weights(tr::Tract{Float32}, peak::Vector{Array{Float32,4}}, f::Vector{Array{Float32,3}};
                     mask::Union{Array{UInt8,3},Nothing}=nothing, f_thresh::Real=0.03, ang_thresh::Real=45, niter::Integer=50,
                     q0::Union{Vector{UInt32},Nothing}=nothing, device::Integer=0)
  nvec = length(peak)
  (1 <= nvec <= 3 && length(f) == nvec) || error("one to three orientation volumes and one amplitude volume for each")
  dims = size(f[1])
  xyz, npts = str_packed(tr)
  nl = length(npts)
  (isnothing(q0) || length(q0) == nl) || error("q0 must hold one weight per line")
  q = Vector{UInt32}(undef, nl)
  w = Vector{Float32}(undef, nl)
  td = Array{Float32,4}(undef, dims[1], dims[2], dims[3], nvec)
  cost = Vector{Float64}(undef, niter + 1)
  mu = Ref{Float64}(0)
  counts = zeros(Int64, 5)
  pv = Ptr{Float32}[pointer(p) for p in peak]
  pf = Ptr{Float32}[pointer(a) for a in f]
  cos2 = Float32(cosd(Float64(ang_thresh))^2)
  GC.@preserve xyz npts peak f pv pf mask q0 q w td cost counts fib_check(ccall((:fib_str_weights, libfibers), Cint,
      (Cint, Ptr{Float32}, Ptr{Int32}, Int64, Int64, Cint, Cint, Cint, Int32, Ptr{Ptr{Float32}}, Ptr{Ptr{Float32}}, Ptr{UInt8}, Cfloat, Cfloat,
       Cint, Ptr{UInt32}, Ptr{UInt32}, Ptr{Float32}, Ptr{Float32}, Ref{Float64}, Ptr{Float64}, Ptr{Int64}),
      device, xyz, npts, nl, size(xyz, 2), dims[1], dims[2], dims[3], nvec, pv, pf, isnothing(mask) ? Ptr{UInt8}(C_NULL) : pointer(mask),
      f_thresh, cos2, niter, isnothing(q0) ? Ptr{UInt32}(C_NULL) : pointer(q0), q, w, td, mu, cost, counts))
  counts[5] == 0 || error("str_weights: $(counts[5]) gathered track densities reached 2^44 units, the integer sums are no longer exact")
  return w, q, td, mu[], cost, counts
end

# ---- bundle tools (NOT in the reference; "Bundle tools" in include/fibers_hip.h) -----------------------------------------------------
const FIB_CENTROIDS_ACCUMULATE = 0x100

"""str_resample(tr, K; flip) -> [3 x K x nlines] — every line with K points (2 to 256) equidistant in arc length in mm (tr.voxel_size);
`flip`: per-line flags, a flagged line comes out reversed.  Lines without points or with a NaN / Inf coordinate are NaN."""
function str_resample(tr::Tract{Float32}, K::Integer=20; flip::Union{Vector{UInt8},Nothing}=nothing, device::Integer=0)
  xyz, npts = str_packed(tr)
  out = Array{Float32,3}(undef, 3, K, length(npts))
  res = Float32.(tr.voxel_size)
  fl = isnothing(flip) ? UInt8[] : flip
  GC.@preserve xyz npts res fl out fib_check(ccall((:fib_str_resample, libfibers), Cint,
      (Cint, Ptr{Float32}, Ptr{Int32}, Int64, Int64, Ptr{Float32}, Cint, Ptr{UInt8}, Ptr{Float32}),
      device, xyz, npts, length(npts), size(xyz, 2), res, K, isnothing(flip) ? Ptr{UInt8}(C_NULL) : pointer(fl), out))
  return out
end

"""str_assign(lines, models, voxel_size, thresh_mm) -> (label, dist, flip) — lines [3 x K x nlines], models [3 x K x nmodels]: the
nearest model of every line by MDF distance in mm (0-based index, -1 beyond `thresh_mm`), the distance, and 1 where the line runs
against its model."""
function str_assign(lines::Array{Float32,3}, models::Array{Float32,3}, voxel_size, thresh_mm::Real; device::Integer=0)
  K, nl, nm = size(lines, 2), size(lines, 3), size(models, 3)
  size(models, 2) == K || error("models and lines must have the same number of points")
  label, dist, flip = Vector{Int32}(undef, nl), Vector{Float32}(undef, nl), Vector{UInt8}(undef, nl)
  res = Float32.(voxel_size)
  GC.@preserve lines models res label dist flip fib_check(ccall((:fib_str_assign, libfibers), Cint,
      (Cint, Ptr{Float32}, Int64, Cint, Ptr{Float32}, Cint, Ptr{Float32}, Cfloat, Ptr{Int32}, Ptr{Float32}, Ptr{UInt8}, Ptr{Float32}),
      device, lines, nl, K, models, nm, res, Float32(thresh_mm), label, dist, flip, Ptr{Float32}(C_NULL)))
  return label, dist, flip
end

"str_centroids(lines, label, flip, nmodels) -> (sums [3 x K x nmodels] Float64, counts UInt32[nmodels]): per-bundle sums of the oriented lines"
function str_centroids(lines::Array{Float32,3}, label::Vector{Int32}, flip::Vector{UInt8}, nmodels::Integer; device::Integer=0)
  K, nl = size(lines, 2), size(lines, 3)
  sums, counts = zeros(Float64, 3, K, nmodels), zeros(UInt32, nmodels)
  GC.@preserve lines label flip sums counts fib_check(ccall((:fib_str_centroids, libfibers), Cint,
      (Cint, Ptr{Float32}, Int64, Cint, Ptr{Int32}, Ptr{UInt8}, Cint, Cint, Ptr{Float64}, Ptr{UInt32}),
      device, lines, nl, K, label, flip, nmodels, 0, sums, counts))
  return sums, counts
end

# device tier: the same kernels on device pointers (a caller that holds them, e.g. through AMDGPU.jl, passes them as Ptr{Cvoid})
fibd_str_roi_pack(rois::Ptr{Cvoid}, nroi::Integer, nvox::Integer, roibits::Ptr{Cvoid}, stream::Ptr{Cvoid}=C_NULL) =
  fib_check(ccall((:fibd_str_roi_pack, libfibers), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}), rois, nroi, nvox, roibits, stream))

function fibd_str_select_work_size(nlines::Integer)
  b = Ref{UInt64}(0)
  fib_check(ccall((:fibd_str_select_work_size, libfibers), Cint, (Int64, Ref{UInt64}), nlines, b))
  return Int(b[])
end

fibd_str_select(xyz::Ptr{Cvoid}, npts::Ptr{Cvoid}, nlines::Integer, npoints::Integer, dims, roibits::Ptr{Cvoid}, visit_all::UInt64, visit_none::UInt64,
                end_any::UInt64, end_both::UInt64, min_npts::Integer, max_npts::Integer, keep::Ptr{Cvoid}, hits::Ptr{Cvoid}, counts::Ptr{Cvoid},
                work::Ptr{Cvoid}, work_bytes::Integer, stream::Ptr{Cvoid}=C_NULL) =
  fib_check(ccall((:fibd_str_select, libfibers), Cint,
      (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Cint, Cint, Ptr{Cvoid}, UInt64, UInt64, UInt64, UInt64, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid},
       Ptr{Cvoid}, Ptr{Cvoid}, UInt64, Ptr{Cvoid}),
      xyz, npts, nlines, npoints, dims[1], dims[2], dims[3], roibits, visit_all, visit_none, end_any, end_both, min_npts, max_npts, keep, hits,
      counts, work, work_bytes, stream))

fibd_str_gather(xyz::Ptr{Cvoid}, npts::Ptr{Cvoid}, nlines::Integer, npoints::Integer, keep::Ptr{Cvoid}, scalars::Ptr{Cvoid}, nscalars::Integer,
                cap_lines::Integer, cap_points::Integer, xyz_out::Ptr{Cvoid}, npts_out::Ptr{Cvoid}, index_out::Ptr{Cvoid}, scalars_out::Ptr{Cvoid},
                counts::Ptr{Cvoid}, work::Ptr{Cvoid}, work_bytes::Integer, stream::Ptr{Cvoid}=C_NULL) =
  fib_check(ccall((:fibd_str_gather, libfibers), Cint,
      (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
       Ptr{Cvoid}, UInt64, Ptr{Cvoid}),
      xyz, npts, nlines, npoints, keep, scalars, nscalars, cap_lines, cap_points, xyz_out, npts_out, index_out, scalars_out, counts, work,
      work_bytes, stream))

fibd_str_connectome(xyz::Ptr{Cvoid}, npts::Ptr{Cvoid}, nlines::Integer, npoints::Integer, dims, volres::Vector{Float32}, labels::Ptr{Cvoid},
                    remap::Ptr{Cvoid}, nremap::Integer, nnodes::Integer, flags::Integer, cmat::Ptr{Cvoid}, wmat::Ptr{Cvoid}, assign::Ptr{Cvoid},
                    n_lines::Ptr{Cvoid}, work::Ptr{Cvoid}, work_bytes::Integer, stream::Ptr{Cvoid}=C_NULL) =
  fib_check(ccall((:fibd_str_connectome, libfibers), Cint,
      (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Cint, Cint, Ptr{Float32}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cvoid}, Ptr{Cvoid},
       Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, UInt64, Ptr{Cvoid}),
      xyz, npts, nlines, npoints, dims[1], dims[2], dims[3], volres, labels, remap, nremap, nnodes, flags, cmat, wmat, assign, n_lines, work,
      work_bytes, stream))

# ---- probabilistic tracking (NOT in the reference; "Probabilistic tracking" in include/fibers_hip.h) -----------------------------
"""prob_stream(odf, odf_dirs; mask, seed, nsub, len_min, len_max, ang_thresh, step_size, pmf_thresh, subtract_min, rng_seed) -> Tract —
probabilistic tractography from an ODF volume [nx,ny,nz,nvert] (e.g. `gqi_rec(...).odf`): at every step the direction is drawn from the
ODF of the voxel ahead inside a cone of `ang_thresh` degrees (below 90) around the direction of travel.  Seeds, `nsub` and the line
layout follow `stream`; the draws come from the library's counter-based generator (`rng_seed`), the sub-voxel offsets from Julia's RNG."""
function prob_stream(odf::MRI, odf_dirs::ODF=sphere_642; mask::Union{MRI,Nothing}=nothing, seed::Union{MRI,Nothing}=nothing,
                     nsub::Integer=3, len_min::Integer=3, len_max::Integer=maximum(odf.volsize), ang_thresh::Real=45,
                     step_size::Real=.5, pmf_thresh::Real=.1, subtract_min::Bool=true, rng_seed::Integer=rand(UInt64),
                     device::Integer=0)
  vol = odf.vol::Array{Float32,4}
  nx, ny, nz, nvert = size(vol)
  nvert == size(odf_dirs.vertices, 1) ÷ 2 || error("odf must have one frame per direction of the half sphere")
  U = Matrix{Float32}(permutedims(odf_dirs.vertices[1:nvert, :]))            # [3 x nvert] = [nvert][3] on the C side
  m8 = isnothing(mask) ? UInt8[] : UInt8.(view(mask.vol, :, :, :, 1) .> 0)
  s8 = isnothing(seed) ? UInt8[] : UInt8.(view(seed.vol, :, :, :, 1) .> 0)
  sublist = nsub > 0 ? hcat([Float32.(rand(Uniform(-.5+eps(), .5-eps()), 3)) for _ in 1:nsub]...) : zeros(Float32, 3, 1)
  out = FibTractOut()
  GC.@preserve vol U m8 s8 sublist fib_check(ccall((:fib_prob_stream, libfibers), Cint,
      (Cint, Cint, Cint, Cint, Ptr{Float32}, Cint, Ptr{Float32}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float32}, Int32, Int32, Int32, Cfloat, Cfloat,
       Cfloat, Int32, UInt64, Ref{FibTractOut}),
      device, nx, ny, nz, vol, nvert, U, isnothing(mask) ? Ptr{UInt8}(C_NULL) : pointer(m8), isnothing(seed) ? Ptr{UInt8}(C_NULL) : pointer(s8),
      sublist, size(sublist, 2), len_min, len_max, cosd(Float32(ang_thresh)), Float32(step_size), Float32(pmf_thresh), Int32(subtract_min),
      UInt64(rng_seed), out))
  npts = unsafe_wrap(Array, out.npts, out.nlines)
  xyz  = unsafe_wrap(Array, out.xyz, (3, Int(out.npoints)))
  off  = cumsum(vcat(0, Int.(npts)))
  str  = [xyz[:, off[i]+1:off[i+1]] for i in 1:length(npts)]
  ccall((:fib_tract_free, libfibers), Cvoid, (Ref{FibTractOut},), out)
  tr = Tract{Float32}(isnothing(mask) ? odf : mask)
  str_add!(tr, str)
  return tr
end

# device tier
fib_prob_row_pitch(nvert::Integer) = Int(ccall((:fib_prob_row_pitch, libfibers), Cint, (Cint,), nvert))

fibd_prob_table(odf::Ptr{Cvoid}, mask::Ptr{Cvoid}, nvox::Integer, nvert::Integer, subtract_min::Bool, pmf_thresh::Real, table::Ptr{Cvoid},
                stream::Ptr{Cvoid}=C_NULL) =
  fib_check(ccall((:fibd_prob_table, libfibers), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cint, Cint, Cfloat, Ptr{Cvoid}, Ptr{Cvoid}),
      odf, mask, nvox, nvert, Int32(subtract_min), Float32(pmf_thresh), table, stream))

function fib_prob_plan_create(device::Integer, U::Matrix{Float32}, cosang_thresh::Real)
  h = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve U fib_check(ccall((:fib_prob_plan_create, libfibers), Cint, (Cint, Ptr{Float32}, Cint, Cfloat, Ref{Ptr{Cvoid}}),
      device, U, size(U, 2), Float32(cosang_thresh), h))
  return h[]
end
fib_prob_plan_destroy(plan::Ptr{Cvoid}) = ccall((:fib_prob_plan_destroy, libfibers), Cvoid, (Ptr{Cvoid},), plan)

function fibd_prob_work_size(nlines::Integer)
  b = Ref{UInt64}(0)
  fib_check(ccall((:fibd_prob_work_size, libfibers), Cint, (Int64, Ref{UInt64}), nlines, b))
  return Int(b[])
end

"fibd_prob_run on device pointers -> (status, nlines, npoints); status FIB_ERR_CAPACITY (-9): the counts say what the buffers must hold"
function fibd_prob_run(plan::Ptr{Cvoid}, dims, len_min::Integer, len_max::Integer, step_size::Real, table::Ptr{Cvoid}, seeds::Ptr{Cvoid},
                       nseed::Integer, sublist::Ptr{Cvoid}, nsub::Integer, rng_seed::Integer, npts::Ptr{Cvoid}, seed_index::Ptr{Cvoid},
                       lines_cap::Integer, xyz::Ptr{Cvoid}, points_cap::Integer, work::Ptr{Cvoid}, work_bytes::Integer,
                       stream::Ptr{Cvoid}=C_NULL)
  nl, np = Ref{Int64}(0), Ref{Int64}(0)
  rc = ccall((:fibd_prob_run, libfibers), Cint,
      (Ptr{Cvoid}, Cint, Cint, Cint, Int32, Int32, Cfloat, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int32, UInt64, Ptr{Cvoid}, Ptr{Cvoid},
       Int64, Ptr{Cvoid}, Int64, Ref{Int64}, Ref{Int64}, Ptr{Cvoid}, UInt64, Ptr{Cvoid}),
      plan, dims[1], dims[2], dims[3], len_min, len_max, Float32(step_size), table, seeds, nseed, sublist, nsub, UInt64(rng_seed), npts,
      seed_index, lines_cap, xyz, points_cap, nl, np, work, work_bytes, stream)
  rc == 0 || rc == -9 || fib_check(rc)
  return rc, nl[], np[]
end
