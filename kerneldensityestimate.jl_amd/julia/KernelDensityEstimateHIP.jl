# KernelDensityEstimateHIP.jl -- thin `ccall` shim over libkdehip.so (include/kdehip.h).
#
# Host code stays in Julia: densities are built by the reference's own `kde!` / `BallTreeDensity`
# (KernelDensityEstimate.jl), and only the Gibbs engine `gibbs1` (reference src/MSGibbs01.jl:527-629)
# is replaced by the MI355X HIP kernels.  Two ways to use it:
#
#   using KernelDensityEstimate, KernelDensityEstimateHIP
#   pGM, idx = KernelDensityEstimateHIP.prodAppxMSGibbsS(dummy, [p1; p2; p3], nothing, nothing; Niter=5)
#
# or, to route every existing caller (`*`, IncrementalInference, ...) through the GPU:
#
#   KernelDensityEstimateHIP.enable!()      # overrides KernelDensityEstimate.prodAppxMSGibbsS and .gibbs1 (the hot path)
#   KernelDensityEstimateHIP.enable!(kde=true, trees=true, evaluate=true)
#                                           # opt-in: also kde!(points), kde!(points, ks[, weights]) and evaluateDualTree,
#                                           # i.e. the WHOLE `*` -- product, bandwidth search AND tree construction
#
# After enable!() a call of the reference's `prodAppxMSGibbsS` WITHOUT `randU=`/`randN=` (what `*` and every
# JuliaRobotics caller does) no longer draws `rand(Np*Ndens*(Niter+2)*Nlevels)` / `randn(...)` on the host
# (src/MSGibbs01.jl:661-662; 9.4 MB at 6-D x 4 x 1000, Np = 2048) nor uploads them: it goes to
# `kdehip_prod_philox`, whose random numbers are drawn on the device.  Calls WITH explicit streams keep the
# reference's consumption order through the `gibbs1` override.
#
# NOTE: Julia is not installed in the build container, so this file has been written against the
# C ABI but never executed; tests/ exercise the same entry points through the Python mirror, and
# tests/test_julia_shim_syntax.py checks block structure, every ccall against include/kdehip.h and the list of
# methods enable!() overrides.
module KernelDensityEstimateHIP

using KernelDensityEstimate
const KDE = KernelDensityEstimate

const libkdehip = get(ENV, "KDEHIP_LIB", joinpath(@__DIR__, "..", "libkdehip.so"))

# struct kdehip_density (include/kdehip.h)
struct CDensity
  npts::Int64
  ndim::Int64
  means::Ptr{Float64}
  bandwidth::Ptr{Float64}
  weights::Ptr{Float64}
  left_child::Ptr{Int64}
  right_child::Ptr{Int64}
  permutation::Ptr{Int64}
end

CDensity(bd::BallTreeDensity) = CDensity(bd.bt.num_points, bd.bt.dims, pointer(bd.means), pointer(bd.bandwidth),
                                         pointer(bd.bt.weights), pointer(bd.bt.left_child),
                                         pointer(bd.bt.right_child), pointer(bd.bt.permutation))

lasterror() = unsafe_string(ccall((:kdehip_last_error, libkdehip), Cstring, ()))
devicecount() = Int(ccall((:kdehip_device_count, libkdehip), Cint, ()))

const KDEHIP_ERR_UNSUPPORTED = -7        # ndims > 8, Ndens > 16, ... (include/kdehip.h)

function check(rc::Integer)
  rc == 0 && return nothing
  msg = lasterror()
  rc == -3 && throw(BoundsError(msg))   # randU / randN too short
  error("libkdehip ($rc): $msg")         # incl. "kdes must have same dimension"
end

# The reference's own gibbs1: `KDE.gibbs1` until enable!() has overwritten that method, the saved original
# afterwards (calling KDE.gibbs1 from the fallback paths would then recurse into this module).
const ORIGINAL_GIBBS1 = Ref{Any}(nothing)
reference_gibbs1(args...; kw...) =
  ORIGINAL_GIBBS1[] === nothing ? KDE.gibbs1(args...; kw...) : ORIGINAL_GIBBS1[](args...; kw...)

# the same for the front end (enable!() overwrites KDE.prodAppxMSGibbsS as well)
const ORIGINAL_PROD = Ref{Any}(nothing)
reference_prodAppxMSGibbsS(args...; kw...) =
  ORIGINAL_PROD[] === nothing ? KDE.prodAppxMSGibbsS(args...; kw...) : ORIGINAL_PROD[](args...; kw...)

# ... and for the callers either side of the product: `kde!(points)` (LOOCV bandwidth; the second half of `*`,
# src/MSGibbs01.jl:725), the explicit-bandwidth constructors `kde!(points, ks[, weights])` (src/KDE01.jl:34-76: every
# tree of every caller) and `evaluateDualTree` (src/DualTree01.jl:370-421)
const ORIGINAL_KDE_AUTO = Ref{Any}(nothing)
reference_kde_auto(args...) = ORIGINAL_KDE_AUTO[] === nothing ? KDE.kde!(args...) : ORIGINAL_KDE_AUTO[](args...)
const ORIGINAL_KDE_BW = Ref{Any}(nothing)     # kde!(points, ks, addop, diffop)
const ORIGINAL_KDE_BWW = Ref{Any}(nothing)    # kde!(points, ks, weights, addop, diffop)
reference_kde_bw(args...) = ORIGINAL_KDE_BW[] === nothing ? KDE.kde!(args...) : ORIGINAL_KDE_BW[](args...)
reference_kde_bww(args...) = ORIGINAL_KDE_BWW[] === nothing ? KDE.kde!(args...) : ORIGINAL_KDE_BWW[](args...)
const ORIGINAL_EVAL = Ref{Any}(nothing)
const ORIGINAL_EVAL_BD = Ref{Any}(nothing)
reference_evaluateDualTree(args...) =
  ORIGINAL_EVAL[] === nothing ? KDE.evaluateDualTree(args...) : ORIGINAL_EVAL[](args...)
reference_evaluateDualTree_bd(args...) =
  ORIGINAL_EVAL_BD[] === nothing ? KDE.evaluateDualTree(args...) : ORIGINAL_EVAL_BD[](args...)

isEuclidOps(addop, diffop) = all(f -> f === +, addop) && all(f -> f === -, diffop)
# the direct evaluation kernel stands for the reference's default only (FORCE_EVAL_DIRECT = true,
# src/KernelDensityEstimate.jl:54; setForceEvalDirect!(false) brings the dual-tree recursion back: reference path)
directEval() = KDE.FORCE_EVAL_DIRECT

isEuclid(addop, diffop, getMu, getLambda) =
  all(f -> f === +, addop) && all(f -> f === -, diffop) &&
  all(f -> f === KDE.getEuclidMu, getMu) && all(f -> f === KDE.getEuclidLambda, getLambda)

maskbytes(partialDimMask, Ndens, ndims) =
  UInt8[partialDimMask[j][d] ? 0x01 : 0x00 for d in 1:ndims, j in 1:Ndens]   # density-major in memory

"""
    gibbs1(Ndens, trees, Np, Niter, pts, ind, randU, randN; kw...)

Drop-in for `KernelDensityEstimate.gibbs1` (same arguments, fills `pts` and `ind` in place).
Non-Euclidean manifold operators cannot cross the C ABI: they fall back to the reference.
"""
function gibbs1(Ndens::Int, trees::Array{BallTreeDensity,1}, Np::Int, Niter::Int,
                pts::Array{Float64,1}, ind::Array{Int}, randU::Array{Float64,1}, randN::Array{Float64,1};
                addop=(+,), diffop=(-,), getMu=(KDE.getEuclidMu,), getLambda=(KDE.getEuclidLambda,),
                glbs=KDE.makeEmptyGbGlb(), addEntropy::Bool=true,
                ndims::Int=maximum(Ndim.(trees)),
                partialDimMask::AbstractVector{<:BitVector}=[ones(Int, ndims) .== 1 for i in 1:Ndens],
                device::Int=0, ngpus::Int=1)
  fallback() = reference_gibbs1(Ndens, trees, Np, Niter, pts, ind, randU, randN; addop=addop, diffop=diffop,
                                getMu=getMu, getLambda=getLambda, glbs=glbs, addEntropy=addEntropy, ndims=ndims,
                                partialDimMask=partialDimMask)
  isEuclid(addop, diffop, getMu, getLambda) || return fallback()
  cds = CDensity[CDensity(t) for t in trees]
  mask = maskbytes(partialDimMask, Ndens, ndims)
  # glbs.recordChoosen (src/MSGibbs01.jl:29-31): the label trace comes back as labels[level, density, sample]
  Nlevels = floor(Int, log(Float64(maximum(Npts.(trees)))) / log(2.0) + 1.0)   # :568
  labels = glbs.recordChoosen ? zeros(Int32, Nlevels, Ndens, Np) : Int32[]
  GC.@preserve trees cds mask labels begin
    # chains split over `ngpus` devices (device .. device+ngpus-1) in contiguous ranges; ngpus = 1: one GPU
    rc = ccall((:kdehip_gibbs1_multi, libkdehip), Cint,
               (Cint, Ptr{CDensity}, Int64, Cint, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Float64},
                Int64, Cint, Cint, Ptr{UInt8}, Cint, Cint, Ptr{Int32}),
               Ndens, cds, Np, Niter, pts, ind, randU, length(randU), randN, length(randN),
               addEntropy ? 1 : 0, ndims, mask, device, ngpus, glbs.recordChoosen ? pointer(labels) : C_NULL)
  end
  # shapes beyond the compiled limits (ndims > 8, Ndens > 16) stay on the reference path: the caller sees the
  # same behaviour as without this package, only slower (nothing has been written to pts / ind yet)
  rc == KDEHIP_ERR_UNSUPPORTED && return fallback()
  check(rc)
  if glbs.recordChoosen   # same nesting and 1-based keys as :471-472, :575-583, :109-112
    glbs.labelsChoosen = Dict{Int,Dict{Int,Dict{Int,Int}}}()
    for s in 1:Np
      glbs.labelsChoosen[s] = Dict{Int,Dict{Int,Int}}()
      for j in 1:Ndens
        glbs.labelsChoosen[s][j] = Niter > 0 ? Dict{Int,Int}(l => Int(labels[l, j, s]) for l in 1:Nlevels) :
                                               Dict{Int,Int}()
      end
    end
  end
  nothing
end

"""
    prodAppxMSGibbsS(npd0, trees, anFcns, anParams; Niter=3, ..., seed=nothing, device=0, ngpus=1)

Same keywords and return value as the reference (src/MSGibbs01.jl:645-703), `maxNp` and `Nlevels` included
(:659-660; they only size the random streams, the engine derives its level count from the trees, :568).
With `randU`/`randN` given they are consumed exactly like the reference consumes them; otherwise the
on-device Philox stream keyed by `seed` replaces `rand`/`randn`.
"""
function prodAppxMSGibbsS(npd0::BallTreeDensity, trees::Array{BallTreeDensity,1}, anFcns, anParams;
                          Niter::Int=3, addop=(+,), diffop=(-,), getMu=(KDE.getEuclidMu,),
                          getLambda=(KDE.getEuclidLambda,), glbs=KDE.makeEmptyGbGlb(), addEntropy::Bool=true,
                          ndims::Integer=maximum(Ndim.(trees)), Ndens=length(trees), Np=Npts(npd0),
                          maxNp=maximum([Np; Npts.(trees)]),
                          Nlevels=floor(Int, (log(Float64(maxNp)) / log(2.0)) + 1.0),
                          randU=nothing, randN=nothing,
                          partialDimMask::AbstractVector{<:BitVector}=[ones(Int, ndims) .== 1 for i in 1:length(trees)],
                          seed::Union{Nothing,UInt64}=nothing, device::Int=0, ngpus::Int=1)
  # the reference's own front end and engine, with the streams the reference would have drawn itself
  reference() = reference_prodAppxMSGibbsS(npd0, trees, anFcns, anParams; Niter=Niter, addop=addop, diffop=diffop,
                                           getMu=getMu, getLambda=getLambda, glbs=glbs, addEntropy=addEntropy,
                                           ndims=ndims, Ndens=Ndens, Np=Np, maxNp=maxNp, Nlevels=Nlevels,
                                           randU=(randU === nothing ? rand(Int(Np * Ndens * (Niter + 2) * Nlevels)) : randU),
                                           randN=(randN === nothing ? randn(Int(ndims * Np * (Nlevels + 1))) : randN),
                                           partialDimMask=partialDimMask)
  isEuclid(addop, diffop, getMu, getLambda) || return reference()
  points = zeros(ndims * Np)
  indices = ones(Int, Ndens, Np)
  if randU !== nothing || randN !== nothing || glbs.recordChoosen
    if randU === nothing || randN === nothing   # (label traces go through the drop-in: streams from the host twin of the device RNG)
      s = seed === nothing ? rand(UInt64) : seed
      Ltree = floor(Int, log(Float64(maximum(Npts.(trees)))) / log(2.0) + 1.0)
      K, R = Ndens * (1 + Ltree * (Niter + 1)), ndims * (Ltree + 1)
      if randU === nothing
        randU = zeros(Np * K)
        ccall((:kdehip_philox_fill_uniform, libkdehip), Cvoid, (UInt64, Int64, Int64, Int64, Ptr{Float64}), s, 0, Np, K, randU)
      end
      if randN === nothing
        randN = zeros(Np * R)
        ccall((:kdehip_philox_fill_normal, libkdehip), Cvoid, (UInt64, Int64, Int64, Int64, Ptr{Float64}), s, 0, Np, R, randN)
      end
    end
    gibbs1(Ndens, trees, Np, Niter, points, indices, randU, randN; glbs=glbs, addEntropy=addEntropy,
           ndims=Int(ndims), partialDimMask=partialDimMask, device=device, ngpus=ngpus)
    return reshape(points, ndims, Np), indices
  end
  cds = CDensity[CDensity(t) for t in trees]
  mask = maskbytes(partialDimMask, Ndens, ndims)
  s = seed === nothing ? rand(UInt64) : seed
  GC.@preserve trees cds mask begin
    # one-shot: pack, upload, run (device Philox stream keyed by `s`), copy back; chains split over `ngpus` devices
    rc = ccall((:kdehip_prod_philox, libkdehip), Cint,
               (Cint, Ptr{CDensity}, Int64, Cint, Ptr{Float64}, Ptr{Int64}, UInt64, Cint, Cint, Ptr{UInt8}, Cint, Cint,
                Cint, Ptr{Int32}),
               Ndens, cds, Np, Niter, points, indices, s, addEntropy ? 1 : 0, ndims, mask, 64, device, ngpus, C_NULL)
  end
  rc == KDEHIP_ERR_UNSUPPORTED && return reference()   # beyond the compiled limits (nothing has been written yet)
  check(rc)
  return reshape(points, ndims, Np), indices
end

# the reference's deprecated positional form (src/MSGibbs01.jl:632-643)
function prodAppxMSGibbsS(npd0::BallTreeDensity, trees::Array{BallTreeDensity,1}, anFcns, anParams, Niter::Int)
  @warn "prodApproxMSGibbs has new keyword interface, use (..; Niter::Int=5 ) instead"
  prodAppxMSGibbsS(npd0, trees, anFcns, anParams; Niter=Niter)
end

"""
    DeviceDensity(bd; device=0)

A `BallTreeDensity` uploaded ONCE and kept in HBM (`kdehip_density_upload`; include/kdehip.h section 2c).  Products of
such densities -- `prodAppxMSGibbsS(npd0, ::Vector{DeviceDensity}, ...)` -- are laid out into tiles by the GPU: no host
re-layout, no upload per product.  `free!(d)` releases it (also run by the finalizer).
"""
mutable struct DeviceDensity
  handle::Ptr{Cvoid}
  npts::Int
  ndim::Int
  function DeviceDensity(bd::BallTreeDensity; device::Int=0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    cd = Ref(CDensity(bd))
    GC.@preserve bd begin
      check(ccall((:kdehip_density_upload, libkdehip), Cint, (Ref{Ptr{Cvoid}}, Ref{CDensity}, Cint), h, cd, device))
    end
    d = new(h[], Npts(bd), Ndim(bd))
    finalizer(free!, d)
    return d
  end
  function DeviceDensity(handle::Ptr{Cvoid}, npts::Int, ndim::Int)   # a density the library built (resident chain)
    d = new(handle, npts, ndim)
    finalizer(free!, d)
    return d
  end
end
# handle -> DeviceDensity for densities the library built itself (the resident chain below)
function DeviceDensity(handle::Ptr{Cvoid})
  d = ccall((:kdehip_density_npts, libkdehip), Int64, (Ptr{Cvoid},), handle)
  k = ccall((:kdehip_density_ndim, libkdehip), Cint, (Ptr{Cvoid},), handle)
  return DeviceDensity(handle, Int(d), Int(k))
end
function free!(d::DeviceDensity)
  if d.handle != C_NULL
    ccall((:kdehip_density_free, libkdehip), Cvoid, (Ptr{Cvoid},), d.handle)
    d.handle = C_NULL
  end
  nothing
end

"""
    *(trees::Vector{DeviceDensity}; addEntropy=true, seed=nothing) -> DeviceDensity

The reference's `*` (src/MSGibbs01.jl:707-726: product with Niter = 5 and Np = round(mean Npts), then `kde!(pGM)`) on
densities that live in HBM, result in HBM (`kdehip_mul_device`): the sample matrix never leaves the device -- the
bandwidth search reads it there, the tree is built from one copy that comes down meanwhile, the new density's block
goes straight back up.  A belief-propagation sweep chains such products without PCIe traffic per message besides that.
`BallTreeDensity(d)` downloads the reference's arrays when the host wants them.
"""
function Base.:*(trees::Vector{DeviceDensity}; addEntropy::Bool=true, seed::Union{Nothing,UInt64}=nothing)
  h = Ref{Ptr{Cvoid}}(C_NULL)
  handles = Ptr{Cvoid}[t.handle for t in trees]
  s = seed === nothing ? rand(UInt64) : seed
  GC.@preserve trees handles begin
    check(ccall((:kdehip_mul_device, libkdehip), Cint,
                (Ref{Ptr{Cvoid}}, Cint, Ptr{Ptr{Cvoid}}, UInt64, Cint, Ptr{Float64}, Ptr{Int32}),
                h, length(trees), handles, s, addEntropy ? 1 : 0, C_NULL, C_NULL))
  end
  return DeviceDensity(h[])
end
Base.:*(p::DeviceDensity, q::DeviceDensity) = *([p; q])

struct CMulItem                       # struct kdehip_mul_item, include/kdehip.h
  Ndens::Int32
  addEntropy::Int32
  trees::Ptr{Ptr{Cvoid}}
  seed::UInt64
end

"""
    mul_batch(products::Vector{Vector{DeviceDensity}}; addEntropy=true, seeds=nothing) -> Vector{DeviceDensity}

MANY `*` (src/MSGibbs01.jl:707-726) in ONE library call (`kdehip_mul_device_batch`) -- what a belief-propagation sweep
issues, on the reference's own sizes (100-300 points, test/runtests.jl:189-201): batched sampler, the LOOCV bandwidth
searches of all results of one size in the same launches, the trees on the library's host pool under them.  Result `i` is
bit for bit `*(products[i]; addEntropy, seed=seeds[i])`.
"""
function mul_batch(products::Vector{Vector{DeviceDensity}}; addEntropy::Bool=true,
                   seeds::Union{Nothing,Vector{UInt64}}=nothing)
  n = length(products)
  n == 0 && return DeviceDensity[]
  sds = seeds === nothing ? rand(UInt64, n) : seeds
  handles = [Ptr{Cvoid}[t.handle for t in p] for p in products]
  out = fill(Ptr{Cvoid}(C_NULL), n)
  GC.@preserve products handles begin
    items = CMulItem[CMulItem(length(handles[i]), addEntropy ? 1 : 0, pointer(handles[i]), sds[i]) for i in 1:n]
    check(ccall((:kdehip_mul_device_batch, libkdehip), Cint,
                (Cint, Ptr{CMulItem}, Ptr{Ptr{Cvoid}}, Ptr{Float64}, Ptr{Int32}),
                n, items, out, C_NULL, C_NULL))
  end
  return DeviceDensity[DeviceDensity(h) for h in out]
end

"""
    hip_prod_manifold(trees::Vector{BallTreeDensity}, manifold; Np, Niter=3, addEntropy=true, partialDimMask=nothing,
                      seed=nothing, device=0, ngpus=1) -> (points, indices)

`prodAppxMSGibbsS` without caller streams on a manifold, on one or several GPUs (`kdehip_prod_philox_manifold`,
include/kdehip.h section 2): device Philox keyed by `seed`, the sampler's circular fast mode where the densities qualify,
the same numbers for every `ngpus`.  Labels are those of `gibbs1` with the enum manifold on the host twin of the Philox
streams; points agree with it to rounding (1e-12, on the circle in the circular dimensions).  `manifold`: as `hip_mul`.
The plan and batch entries of sections 2, 2b and 2e (`kdehip_product_create_manifold`, `kdehip_product_multi_create_manifold`,
`kdehip_prod_philox_batch_manifold`) have no wrapper here, as their Euclidean forms have none: this shim binds no plans.
"""
function hip_prod_manifold(trees::Vector{BallTreeDensity}, manifold; Np::Int, Niter::Int=3, addEntropy::Bool=true,
                           partialDimMask=nothing, seed::Union{Nothing,UInt64}=nothing, device::Int=0, ngpus::Int=1)
  Ndens = length(trees)
  ndims = trees[1].bt.dims
  cds = CDensity[CDensity(t) for t in trees]
  mask = maskbytes(partialDimMask, Ndens, ndims)
  man = manifold_bytes(manifold, ndims)
  points = zeros(ndims * Np)
  indices = ones(Int64, Ndens, Np)
  s = seed === nothing ? rand(UInt64) : seed
  GC.@preserve trees cds mask man begin
    check(ccall((:kdehip_prod_philox_manifold, libkdehip), Cint,
                (Cint, Ptr{CDensity}, Int64, Cint, Ptr{Float64}, Ptr{Int64}, UInt64, Cint, Cint, Ptr{UInt8}, Ptr{UInt8}, Cint,
                 Cint, Cint, Ptr{Int32}),
                Ndens, cds, Np, Niter, points, indices, s, addEntropy ? 1 : 0, ndims, mask, man, 64, device, ngpus, C_NULL))
  end
  return reshape(points, ndims, Np), indices
end

"""
    hip_mul(trees::Vector{DeviceDensity}, manifold; addEntropy=true, seed=nothing) -> DeviceDensity

`*` on resident densities on a manifold (`kdehip_mul_device_manifold`, include/kdehip.h section 2d): the circular product,
then `kde!(pGM)` with the same manifold; the result stays in HBM.  `manifold`: a vector of `:euclid` / `:circular` (or 0 / 1),
one per dimension.  Not installed by `enable!()`: `*` itself stays the Euclidean operator.
"""
function hip_mul(trees::Vector{DeviceDensity}, manifold::AbstractVector; addEntropy::Bool=true,
                 seed::Union{Nothing,UInt64}=nothing)
  h = Ref{Ptr{Cvoid}}(C_NULL)
  handles = Ptr{Cvoid}[t.handle for t in trees]
  man = manifold_bytes(manifold, trees[1].ndim)
  s = seed === nothing ? rand(UInt64) : seed
  GC.@preserve trees handles man begin
    check(ccall((:kdehip_mul_device_manifold, libkdehip), Cint,
                (Ref{Ptr{Cvoid}}, Cint, Ptr{Ptr{Cvoid}}, UInt64, Cint, Ptr{Float64}, Ptr{Int32}, Ptr{UInt8}),
                h, length(trees), handles, s, addEntropy ? 1 : 0, C_NULL, C_NULL, man))
  end
  return DeviceDensity(h[])
end

"""
    hip_mul_batch(products, manifolds; addEntropy=true, seeds=nothing) -> Vector{DeviceDensity}

`mul_batch` with a manifold per product (`kdehip_mul_device_batch_manifold`): `manifolds[i]` is `nothing` (Euclidean) or the
manifold of product `i`.  Result `i` is bit for bit `hip_mul(products[i], manifolds[i]; addEntropy, seed=seeds[i])`.
"""
function hip_mul_batch(products::Vector{Vector{DeviceDensity}}, manifolds::AbstractVector; addEntropy::Bool=true,
                       seeds::Union{Nothing,Vector{UInt64}}=nothing)
  n = length(products)
  n == 0 && return DeviceDensity[]
  length(manifolds) == n || error("one manifold (or nothing) per product")
  sds = seeds === nothing ? rand(UInt64, n) : seeds
  handles = [Ptr{Cvoid}[t.handle for t in p] for p in products]
  rows = zeros(UInt8, 8, n)          # column i = row i of the C array: KDEHIP_MAX_DIMS bytes per product
  for i in 1:n
    manifolds[i] === nothing && continue
    D = products[i][1].ndim
    rows[1:D, i] = manifold_bytes(manifolds[i], D)
  end
  out = fill(Ptr{Cvoid}(C_NULL), n)
  GC.@preserve products handles rows begin
    items = CMulItem[CMulItem(length(handles[i]), addEntropy ? 1 : 0, pointer(handles[i]), sds[i]) for i in 1:n]
    check(ccall((:kdehip_mul_device_batch_manifold, libkdehip), Cint,
                (Cint, Ptr{CMulItem}, Ptr{UInt8}, Ptr{Ptr{Cvoid}}, Ptr{Float64}, Ptr{Int32}),
                n, items, rows, out, C_NULL, C_NULL))
  end
  return DeviceDensity[DeviceDensity(h) for h in out]
end

"""
    BallTreeDensity(d::DeviceDensity)

The reference's struct for a density that was BUILT on the device (`*` above): `kdehip_density_download` returns the
twelve arrays of `BallTreeDensity` / `BallTree` (src/BallTreeDensity01.jl:11-24, src/BallTree01.jl:10-28).
"""
function KDE.BallTreeDensity(d::DeviceDensity)
  N, D = d.npts, d.ndim
  centers, ranges, means, bandwidth = zeros(2N * D), zeros(2N * D), zeros(2N * D), zeros(2N * D)
  bwmin, bwmax, weights = zeros(N * D), zeros(N * D), zeros(2N)
  left, right, lowest, highest, perm = zeros(Int, 2N), zeros(Int, 2N), zeros(Int, 2N), zeros(Int, 2N), zeros(Int, 2N)
  check(ccall((:kdehip_density_download, libkdehip), Cint,
              (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64},
               Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
              d.handle, centers, ranges, weights, left, right, lowest, highest, perm, means, bandwidth, bwmin, bwmax, C_NULL))
  return density_from_arrays(D, N, centers, ranges, weights, left, right, lowest, highest, perm, means, bandwidth, bwmin, bwmax)
end

# The reference's struct around twelve arrays the library filled: the field order of the reference's constructors
# (src/BallTree01.jl:453-457, src/BallTreeDensity01.jl:225-226), the function handles makeBallTreeDensity installs
# (src/BallTreeDensity01.jl:200-201), uniform bandwidth (multibandwidth = 0, :213), and `next` where buildTree! leaves it:
# it starts at 2 and grows by one per internal node below the root (src/BallTree01.jl:384-393,430) = max(N, 2).
function density_from_arrays(D::Int, N::Int, centers, ranges, weights, left, right, lowest, highest, perm, means, bandwidth,
                             bwmin, bwmax)
  bt = KDE.BallTree(D, N, centers, ranges, weights, left, right, lowest, highest, perm, max(N, 2), KDE.swapDensity!,
                    KDE.calcStatsDensity!, [])
  bd = KDE.BallTreeDensity(bt, KDE.GaussianKer, 0, means, bandwidth, bwmin, bwmax, bt.calcStatsHandle, bt.swapHandle)
  bd.bt.data = bd   # the circular reference the reference keeps "for emulating polymorphism"
  return bd
end

# whether `kde!(points, ks[, weights])` can be built by the library: Euclidean operators, uniform bandwidth given as 1 or D
# standard deviations, at most 8 dimensions, at least one point (everything else: the reference's own constructor, with
# the reference's own errors)
builds_here(points, ks, addop, diffop) =
  isEuclidOps(addop, diffop) && 1 <= size(points, 1) <= 8 && size(points, 2) >= 1 && (length(ks) == 1 || length(ks) == size(points, 1))

"""
    kde!(points, ks[, weights])

`kde!(points, ks, weights)` / `kde!(points, ks)` (src/KDE01.jl:34-76 -> makeBallTreeDensity, src/BallTreeDensity01.jl:192-231
-> buildTree!, src/BallTree01.jl:415-434) built by the library's pooled host builder (`kdehip_make_density`): the same
twelve arrays as the reference's single-threaded quick-select gives (same split rule, swap order, node numbering and
moment matching; pinned by the reference's own golden files) -- bit for bit with unit weights (`kde!(points, ks)`).  With
other weights the normalisation `weights ./ sum(weights)` (src/KDE01.jl:46) is a sequential sum in the library and a
pairwise `@simd` sum in Julia: the total, hence every weight and moment-matched node, may differ in the last bit (which
is why the override `enable!(trees=true)` installs hands only unit weights to the library).

`tree_manifold`: `nothing`, or a vector of `:euclid` / `:circular` (or 0 / 1), one per dimension -- the operators of tree
construction, `kde!(points, ks, weights, addop, diffop)`, as THIS library's enum (`kdehip_make_density_tree`, include/kdehip.h
section 4: wrap to [-pi, pi) in most_spread_coord, select! and calcStatsBall!).  Nothing maps a caller's addop / diffop
functions to it automatically: the overrides of `enable!()` keep sending non-Euclidean operators to the reference.
"""
function kde!(points::AbstractMatrix{<:Real}, ks::Vector{Float64}, weights::Union{Nothing,Vector{Float64}}=nothing;
              tree_manifold::Union{Nothing,AbstractVector}=nothing)
  D, N = size(points)
  pts = Matrix{Float64}(points)
  weights === nothing || length(weights) == N || error("weights must have one entry per point")
  centers, ranges, means, bandwidth = zeros(2N * D), zeros(2N * D), zeros(2N * D), zeros(2N * D)
  bwmin, bwmax, w = zeros(N * D), zeros(N * D), zeros(2N)
  left, right, lowest, highest, perm = zeros(Int, 2N), zeros(Int, 2N), zeros(Int, 2N), zeros(Int, 2N), zeros(Int, 2N)
  if tree_manifold === nothing
    GC.@preserve pts ks weights begin
      check(ccall((:kdehip_make_density, libkdehip), Cint,
                  (Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}),
                  D, N, pts, ks, length(ks), weights === nothing ? C_NULL : pointer(weights), centers, ranges, w, left, right,
                  lowest, highest, perm, means, bandwidth, bwmin, bwmax))
    end
  else
    tman = manifold_bytes(tree_manifold, D)
    GC.@preserve pts ks weights tman begin
      check(ccall((:kdehip_make_density_tree, libkdehip), Cint,
                  (Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}, Ptr{UInt8}),
                  D, N, pts, ks, length(ks), weights === nothing ? C_NULL : pointer(weights), centers, ranges, w, left, right,
                  lowest, highest, perm, means, bandwidth, bwmin, bwmax, tman))
    end
  end
  return density_from_arrays(D, N, centers, ranges, w, left, right, lowest, highest, perm, means, bandwidth, bwmin, bwmax)
end

function prodAppxMSGibbsS(npd0, trees::Vector{DeviceDensity}, anFcns, anParams;
                          Niter::Int=3, addEntropy::Bool=true, ndims::Integer=maximum(t.ndim for t in trees),
                          Ndens=length(trees), Np=(npd0 isa BallTreeDensity ? Npts(npd0) : Int(npd0)),
                          partialDimMask::AbstractVector{<:BitVector}=[ones(Int, ndims) .== 1 for i in 1:length(trees)],
                          seed::Union{Nothing,UInt64}=nothing, precision::Int=64)
  points = zeros(ndims * Np)
  indices = ones(Int, Ndens, Np)
  handles = Ptr{Cvoid}[t.handle for t in trees]
  mask = maskbytes(partialDimMask, Ndens, ndims)
  s = seed === nothing ? rand(UInt64) : seed
  GC.@preserve trees handles mask begin
    check(ccall((:kdehip_prod_philox_resident, libkdehip), Cint,
                (Cint, Ptr{Ptr{Cvoid}}, Int64, Cint, UInt64, Cint, Ptr{UInt8}, Cint, Ptr{Float64}, Ptr{Int64}),
                Ndens, handles, Np, Niter, s, addEntropy ? 1 : 0, mask, precision, points, indices))
  end
  return reshape(points, ndims, Np), indices
end

"""
    hip_prodAppxMSGibbsS(npd0, trees::Vector{DeviceDensity}, manifold; Niter=3, addEntropy=true, ...)

`prodAppxMSGibbsS` on resident densities on a manifold, host outputs (`kdehip_prod_philox_resident_manifold`, include/kdehip.h
section 2c): the sampler's circular operators, nothing but descriptors goes up.  fp64 only.  Not installed by `enable!()`.
(The device-output entry `kdehip_prod_philox_device_manifold` has no wrapper here, like `kdehip_prod_philox_device`: this
shim holds no device arrays of its own.)
"""
function hip_prodAppxMSGibbsS(npd0, trees::Vector{DeviceDensity}, manifold::AbstractVector;
                              Niter::Int=3, addEntropy::Bool=true, ndims::Integer=maximum(t.ndim for t in trees),
                              Ndens=length(trees), Np=(npd0 isa BallTreeDensity ? Npts(npd0) : Int(npd0)),
                              partialDimMask::AbstractVector{<:BitVector}=[ones(Int, ndims) .== 1 for i in 1:length(trees)],
                              seed::Union{Nothing,UInt64}=nothing)
  points = zeros(ndims * Np)
  indices = ones(Int, Ndens, Np)
  handles = Ptr{Cvoid}[t.handle for t in trees]
  mask = maskbytes(partialDimMask, Ndens, ndims)
  man = manifold_bytes(manifold, Int(ndims))
  s = seed === nothing ? rand(UInt64) : seed
  GC.@preserve trees handles mask man begin
    check(ccall((:kdehip_prod_philox_resident_manifold, libkdehip), Cint,
                (Cint, Ptr{Ptr{Cvoid}}, Int64, Cint, UInt64, Cint, Ptr{UInt8}, Ptr{UInt8}, Cint, Ptr{Float64}, Ptr{Int64}),
                Ndens, handles, Np, Niter, s, addEntropy ? 1 : 0, mask, man, 64, points, indices))
  end
  return reshape(points, ndims, Np), indices
end

"""
    evaluateDualTree(bd, pos, lvFlag=false)

`evaluateDualTree` / `bd(pos)` with the reference's default `FORCE_EVAL_DIRECT = true`
(src/DualTree01.jl:370-446) on the GPU.  `lvFlag=true`: leave-one-out at `bd`'s own points.
"""
function evaluateDualTree(bd::BallTreeDensity, pos::AbstractMatrix{Float64}, lvFlag::Bool=false; device::Int=0)
  Ndim(bd) == size(pos, 1) || error("bd and pos must have the same dimension")
  Nq = lvFlag ? Npts(bd) : size(pos, 2)
  out = zeros(Nq)
  cd = Ref(CDensity(bd))
  posd = Matrix{Float64}(pos)
  GC.@preserve bd posd begin
    check(ccall((:kdehip_evaluate, libkdehip), Cint, (Ref{CDensity}, Ptr{Float64}, Int64, Cint, Ptr{Float64}, Cint),
                cd, posd, size(pos, 2), lvFlag ? 1 : 0, out, device))
  end
  return out
end

# per-dimension manifold enum of include/kdehip.h: a vector of 0 / 1 or :euclid / :circular, one per dimension
function manifold_bytes(manifold, D::Int)
  length(manifold) == D || error("manifold needs one entry per dimension")
  return UInt8[(m === :circular || m == 1) ? 0x01 : ((m === :euclid || m == 0) ? 0x00 : error("manifold entries are :euclid or :circular")) for m in manifold]
end

"""
    hip_evaluateDualTree(bd, pos, manifold, lvFlag=false; device=0)

`evaluateDualTree` with circular differences in the dimensions `manifold` marks (`kdehip_evaluate_manifold`,
include/kdehip.h section 5d: `wrap(a - b)` before the square, nothing else changes).  The circular semantic is the
library's own; a caller's `diffop` need not be it, so this is not installed by `enable!()`.
"""
function hip_evaluateDualTree(bd::BallTreeDensity, pos::AbstractMatrix{Float64}, manifold::AbstractVector, lvFlag::Bool=false;
                              device::Int=0)
  Ndim(bd) == size(pos, 1) || error("bd and pos must have the same dimension")
  man = manifold_bytes(manifold, Ndim(bd))
  Nq = lvFlag ? Npts(bd) : size(pos, 2)
  out = zeros(Nq)
  cd = Ref(CDensity(bd))
  posd = Matrix{Float64}(pos)
  GC.@preserve bd posd man begin
    check(ccall((:kdehip_evaluate_manifold, libkdehip), Cint,
                (Ref{CDensity}, Ptr{Float64}, Int64, Cint, Ptr{Float64}, Cint, Ptr{UInt8}),
                cd, posd, size(pos, 2), lvFlag ? 1 : 0, out, device, man))
  end
  return out
end

"""
    hip_evalAvgLogL(bd1, bd2, manifold; device=0)

`evalAvgLogL` with circular differences in the marked dimensions (`kdehip_eval_avg_logl_manifold`); `hip_entropy`,
`hip_kld` and `hip_minkld` with a manifold are its compositions.  Not installed by `enable!()`.
"""
function hip_evalAvgLogL(bd1::BallTreeDensity, bd2::BallTreeDensity, manifold::AbstractVector; device::Int=0)
  Ndim(bd1) == Ndim(bd2) || error("evaluate -- dimensions of two BallTreeDensities must match")
  man = manifold_bytes(manifold, Ndim(bd1))
  loo = bd1 === bd2
  c1 = Ref(CDensity(bd1))
  c2 = loo ? c1 : Ref(CDensity(bd2))
  out = Ref{Float64}(0.0)
  GC.@preserve bd1 bd2 man begin
    check(ccall((:kdehip_eval_avg_logl_manifold, libkdehip), Cint,
                (Ref{CDensity}, Ref{CDensity}, Cint, Ptr{Float64}, Cint, Ptr{UInt8}),
                c1, c2, loo ? 1 : 0, out, device, man))
  end
  return out[]
end
hip_entropy(bd::BallTreeDensity, manifold::AbstractVector; device::Int=0) = -hip_evalAvgLogL(bd, bd, manifold; device=device)
hip_kld(p1::BallTreeDensity, p2::BallTreeDensity, manifold::AbstractVector; device::Int=0) =
  hip_evalAvgLogL(p1, p1, manifold; device=device) - hip_evalAvgLogL(p2, p1, manifold; device=device)
hip_minkld(p::BallTreeDensity, q::BallTreeDensity, manifold::AbstractVector; device::Int=0) =
  min(abs(hip_kld(p, q, manifold; device=device)), abs(hip_kld(q, p, manifold; device=device)))

"""
    hip_evaluate_log(bd, pos, lvFlag=false; manifold=nothing, device=0)

`log.(evaluateDualTree(bd, pos, lvFlag))` by log-sum-exp in the kernel (`kdehip_evaluate_log`, include/kdehip.h
section 5f): finite where the density itself underflows to 0.  `manifold` as in `hip_evaluateDualTree`, `nothing` =
Euclidean.  The semantic is the library's own (the reference has no counterpart): not installed by `enable!()`.
"""
function hip_evaluate_log(bd::BallTreeDensity, pos::AbstractMatrix{Float64}, lvFlag::Bool=false; manifold=nothing, device::Int=0)
  Ndim(bd) == size(pos, 1) || error("bd and pos must have the same dimension")
  man = manifold === nothing ? zeros(UInt8, Ndim(bd)) : manifold_bytes(manifold, Ndim(bd))
  Nq = lvFlag ? Npts(bd) : size(pos, 2)
  out = zeros(Nq)
  cd = Ref(CDensity(bd))
  posd = Matrix{Float64}(pos)
  GC.@preserve bd posd man begin
    check(ccall((:kdehip_evaluate_log, libkdehip), Cint,
                (Ref{CDensity}, Ptr{Float64}, Int64, Cint, Ptr{Float64}, Cint, Ptr{UInt8}),
                cd, posd, size(pos, 2), lvFlag ? 1 : 0, out, device, man))
  end
  return out
end

"""
    hip_evaluate_tol(bd, pos, lvFlag=false; rel_tol=1e-3, abs_tol=0.0, manifold=nothing, device=0)

`evaluateDualTree(bd, pos, lvFlag)` within a tolerance (`kdehip_evaluate_tol`, include/kdehip.h section 5m): the all-pairs
sum pruned on the 128-leaf chunks of `bd`, `p (1 - rel_tol) - abs_tol <= result <= p` -- the library's form of
`setForceEvalDirect!(false)`.  The columns of `pos` are processed in the given order, 256 to a block: pass them in the leaf
order of a tree over them for the most pruning.  Returns `(values, (tiles visited, tiles in all))`.  Not installed by
`enable!()`: the override keeps summing every pair.
"""
function hip_evaluate_tol(bd::BallTreeDensity, pos::AbstractMatrix{Float64}, lvFlag::Bool=false; rel_tol::Float64=1e-3,
                          abs_tol::Float64=0.0, manifold=nothing, device::Int=0)
  Ndim(bd) == size(pos, 1) || error("bd and pos must have the same dimension")
  man = manifold === nothing ? zeros(UInt8, Ndim(bd)) : manifold_bytes(manifold, Ndim(bd))
  Nq = lvFlag ? Npts(bd) : size(pos, 2)
  out = zeros(Nq)
  stats = zeros(Int64, 2)
  rt = [rel_tol]
  at = [abs_tol]
  cd = Ref(CDensity(bd))
  posd = Matrix{Float64}(pos)
  GC.@preserve bd posd man rt at stats begin
    check(ccall((:kdehip_evaluate_tol, libkdehip), Cint,
                (Ref{CDensity}, Ptr{Float64}, Int64, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Cint, Ptr{UInt8}),
                cd, posd, size(pos, 2), lvFlag ? 1 : 0, rt, at, out, stats, device, man))
  end
  return out, (stats[1], stats[2])
end

"""
    hip_knn(bd, pos, k=1, lvFlag=false; scale=nothing, manifold=nothing, device=0)

The `k` points of `bd` nearest to every column of `pos` (`kdehip_knn`, include/kdehip.h section 5n): exact, ties in distance
to the lower point index.  Returns `(d2, idx, (tiles visited, tiles in all))`, `d2` the `k x Nq` SQUARED distances and `idx`
the 1-based columns of `getPoints(bd)`.  `lvFlag=true`: the neighbours of `bd`'s own points, each left out by index (`pos`
unread).  `scale`: `nothing` (Euclidean) or one factor `> 0` per dimension, `d2 = sum_k scale[k] d_k^2`.  The columns of
`pos` are processed in the given order, 256 to a block: pass them in the leaf order of a tree over them for the most
pruning.  The reference has no counterpart, so `enable!()` installs nothing.
"""
function hip_knn(bd::BallTreeDensity, pos::AbstractMatrix{Float64}, k::Int=1, lvFlag::Bool=false; scale=nothing,
                 manifold=nothing, device::Int=0)
  Ndim(bd) == size(pos, 1) || error("bd and pos must have the same dimension")
  man = manifold === nothing ? zeros(UInt8, Ndim(bd)) : manifold_bytes(manifold, Ndim(bd))
  sc = scale === nothing ? ones(Ndim(bd)) : Vector{Float64}(scale)
  length(sc) == Ndim(bd) || error("scale needs one entry per dimension")
  Nq = lvFlag ? Npts(bd) : size(pos, 2)
  d2 = zeros(max(k, 1), Nq)
  idx = zeros(Int64, max(k, 1), Nq)
  stats = zeros(Int64, 2)
  cd = Ref(CDensity(bd))
  posd = Matrix{Float64}(pos)
  GC.@preserve bd posd man sc d2 idx stats begin
    check(ccall((:kdehip_knn, libkdehip), Cint,
                (Ref{CDensity}, Ptr{Float64}, Int64, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Cint,
                 Ptr{UInt8}),
                cd, posd, size(pos, 2), k, lvFlag ? 1 : 0, sc, d2, idx, stats, device, man))
  end
  return d2, idx, (stats[1], stats[2])
end

"""
    hip_evalAvgLogL_log(bd1, bd2; manifold=nothing, device=0)

Log-domain `evalAvgLogL` (`kdehip_eval_avg_logl_log`, section 5f): the sum over `W != 0` of `W log p` with `log p` by
log-sum-exp, `-Inf` only where `bd1` has no weighted point; `hip_entropy_log`, `hip_kld_log` and `hip_minkld_log` are its
compositions, leave-one-out where the arguments are the same object.  Not installed by `enable!()`.
"""
function hip_evalAvgLogL_log(bd1::BallTreeDensity, bd2::BallTreeDensity; manifold=nothing, device::Int=0)
  Ndim(bd1) == Ndim(bd2) || error("evaluate -- dimensions of two BallTreeDensities must match")
  man = manifold === nothing ? zeros(UInt8, Ndim(bd1)) : manifold_bytes(manifold, Ndim(bd1))
  loo = bd1 === bd2
  c1 = Ref(CDensity(bd1))
  c2 = loo ? c1 : Ref(CDensity(bd2))
  out = Ref{Float64}(0.0)
  GC.@preserve bd1 bd2 man begin
    check(ccall((:kdehip_eval_avg_logl_log, libkdehip), Cint,
                (Ref{CDensity}, Ref{CDensity}, Cint, Ptr{Float64}, Cint, Ptr{UInt8}),
                c1, c2, loo ? 1 : 0, out, device, man))
  end
  return out[]
end
hip_entropy_log(bd::BallTreeDensity; manifold=nothing, device::Int=0) = -hip_evalAvgLogL_log(bd, bd; manifold=manifold, device=device)
hip_kld_log(p1::BallTreeDensity, p2::BallTreeDensity; manifold=nothing, device::Int=0) =
  hip_evalAvgLogL_log(p1, p1; manifold=manifold, device=device) - hip_evalAvgLogL_log(p2, p1; manifold=manifold, device=device)
hip_minkld_log(p::BallTreeDensity, q::BallTreeDensity; manifold=nothing, device::Int=0) =
  min(abs(hip_kld_log(p, q; manifold=manifold, device=device)), abs(hip_kld_log(q, p; manifold=manifold, device=device)))

"""
    hip_auto_bandwidth(points, manifold; device=0)

The bandwidth of `kde!(points, addop, diffop)` with the library's circular `diffop` in the marked dimensions
(`kdehip_auto_bandwidth_manifold`): only the leave-one-out likelihoods of the search wrap, as in the reference.
"""
function hip_auto_bandwidth(points::AbstractMatrix{Float64}, manifold::AbstractVector; device::Int=0)
  D, N = size(points)
  man = manifold_bytes(manifold, D)
  bw = zeros(D)
  nev = Ref{Int32}(0)
  pts = Matrix{Float64}(points)
  GC.@preserve man begin
    check(ccall((:kdehip_auto_bandwidth_manifold, libkdehip), Cint,
                (Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ref{Int32}, Cint, Ptr{UInt8}),
                D, N, pts, bw, nev, device, man))
  end
  return bw
end

"""
    hip_sample(bd, Npts[, ind]; seed=nothing, sample_offset=0, device=0) -> (points, ind)

`sample(npd, Npts)` / `sample(npd, Npts, ind)` (src/KDE01.jl:164-189) on the GPU (`kdehip_sample`): labels by weight
(first i with cumsum(w)[i] / cumsum(w)[end] > u), points `getPoints(bd)[:, i] + getBW(bd)[:, i] .* n`, ind 1-based.  The
random numbers come from the library's Philox stream (include/kdehip.h section 2f), and the samples are in draw order
where the reference groups them by ascending label: same distribution, not the same matrix.  Not installed by `enable!()`.
"""
function hip_sample(bd::BallTreeDensity, Npts::Int, ind::Union{Nothing,Vector{Int}}=nothing;
                    seed::Union{Nothing,UInt64}=nothing, sample_offset::Int=0, device::Int=0)
  D = Ndim(bd)
  pts = zeros(D, Npts)
  out = zeros(Int, Npts)
  s = seed === nothing ? rand(UInt64) : seed
  cd = Ref(CDensity(bd))
  lab = ind === nothing ? C_NULL : Vector{Int64}(ind)
  GC.@preserve bd lab begin
    check(ccall((:kdehip_sample, libkdehip), Cint,
                (Ref{CDensity}, Int64, UInt64, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Cint),
                cd, Npts, s, sample_offset, lab, pts, out, device))
  end
  return pts, out
end

"`rand(p, N=1)` (src/KDE01.jl:196-198): the points of `hip_sample(p, N)`."
hip_rand(p::BallTreeDensity, N::Int=1; seed::Union{Nothing,UInt64}=nothing) = hip_sample(p, N; seed=seed)[1]

"""
    hip_resample(p, Np=-1, ksType=:lcv; seed=nothing)

`resample(p, Np, :lcv)` (src/BallTreeDensity01.jl:312-334): `kde!(hip_sample(p, Np)[1])`; Np <= 0 means Npts(p) (the
reference's default calls an undefined `getNpts`).
"""
function hip_resample(p::BallTreeDensity, Np::Int=-1, ksType::Symbol=:lcv; seed::Union{Nothing,UInt64}=nothing)
  ksType == :lcv || error("hip_resample: only ksType = :lcv")
  n = Np <= 0 ? Npts(p) : Np
  pts, = hip_sample(p, n; seed=seed)
  return kde!(pts)
end

"""
    hip_evalAvgLogL(bd1, bd2; device=0)

`evalAvgLogL(bd1, bd2)` (src/DualTree01.jl:450-470) on the GPU (`kdehip_eval_avg_logl`, include/kdehip.h section 5b):
sum over bd2's points of W log L, L = bd1 at those points by the direct sum, -Inf when an L == 0 carries weight.
Leave-one-out when `bd1 === bd2`, as the reference's `bd == locations` decides it.  Not installed by `enable!()`.
"""
function hip_evalAvgLogL(bd1::BallTreeDensity, bd2::BallTreeDensity; device::Int=0)
  Ndim(bd1) == Ndim(bd2) || error("evaluate -- dimensions of two BallTreeDensities must match")
  loo = bd1 === bd2
  c1 = Ref(CDensity(bd1))
  c2 = loo ? c1 : Ref(CDensity(bd2))
  out = Ref{Float64}(0.0)
  GC.@preserve bd1 bd2 begin
    check(ccall((:kdehip_eval_avg_logl, libkdehip), Cint, (Ref{CDensity}, Ref{CDensity}, Cint, Ptr{Float64}, Cint),
                c1, c2, loo ? 1 : 0, out, device))
  end
  return out[]
end

"`entropy(bd)` (src/DualTree01.jl:505-508) = -hip_evalAvgLogL(bd, bd)."
hip_entropy(bd::BallTreeDensity; device::Int=0) = -hip_evalAvgLogL(bd, bd; device=device)

"`kld(p1, p2; method=:direct)` (src/DualTree01.jl:477-503) = hip_evalAvgLogL(p1, p1) - hip_evalAvgLogL(p2, p1)."
function hip_kld(p1::BallTreeDensity, p2::BallTreeDensity; method::Symbol=:direct, device::Int=0)
  method == :direct || error("hip_kld: only method = :direct is supported")
  return hip_evalAvgLogL(p1, p1; device=device) - hip_evalAvgLogL(p2, p1; device=device)
end

"`minkld(p, q)` (src/DualTree01.jl:510) = min(|kld(p, q)|, |kld(q, p)|)."
hip_minkld(p::BallTreeDensity, q::BallTreeDensity; device::Int=0) =
  min(abs(hip_kld(p, q; device=device)), abs(hip_kld(q, p; device=device)))

"""
    hip_kernel_sum(a, b, var=nothing; normalize=false, manifold=nothing, device=0)

The weighted all-pairs Gaussian sum `S(a, b; var)` over the leaf points and weights of two densities (`kdehip_kernel_sum`,
include/kdehip.h section 5g): `var` = D variances, or `nothing` = the sum of the two densities' leaf variances;
`normalize` divides by `prod_k sqrt(2 pi var_k)`.  The full square is summed, whatever the identity of the arguments.
`hip_intersIntg`, `hip_ise` and `hip_mmd` are its compositions.  The library's own: not installed by `enable!()`.
"""
function hip_kernel_sum(a::BallTreeDensity, b::BallTreeDensity, var::Union{Nothing,AbstractVector{Float64}}=nothing;
                        normalize::Bool=false, manifold=nothing, device::Int=0)
  Ndim(a) == Ndim(b) || error("kernel sum -- dimensions of two BallTreeDensities must match")
  var === nothing || length(var) == Ndim(a) || error("var needs one variance per dimension")
  man = manifold === nothing ? zeros(UInt8, Ndim(a)) : manifold_bytes(manifold, Ndim(a))
  v = var === nothing ? Float64[] : Vector{Float64}(var)
  ca = Ref(CDensity(a))
  cb = a === b ? ca : Ref(CDensity(b))
  out = Ref{Float64}(0.0)
  GC.@preserve a b v man begin
    check(ccall((:kdehip_kernel_sum, libkdehip), Cint,
                (Ref{CDensity}, Ref{CDensity}, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Ptr{UInt8}),
                ca, cb, var === nothing ? Ptr{Float64}(C_NULL) : pointer(v), normalize ? 1 : 0, out, device, man))
  end
  return out[]
end

"The exact integral of p q (what `intersIntgAppxIS` approximates, in any dimension up to 8): the normalised sum at the summed leaf variances."
hip_intersIntg(p::BallTreeDensity, q::BallTreeDensity; manifold=nothing, device::Int=0) =
  hip_kernel_sum(p, q; normalize=true, manifold=manifold, device=device)

"The integrated squared error, integral of (p - q)^2: symmetric, exactly 0 for `hip_ise(p, p)`."
hip_ise(p::BallTreeDensity, q::BallTreeDensity; manifold=nothing, device::Int=0) =
  hip_intersIntg(p, p; manifold=manifold, device=device) - 2.0 * hip_intersIntg(p, q; manifold=manifold, device=device) +
  hip_intersIntg(q, q; manifold=manifold, device=device)

"The biased MMD^2 under the Gaussian kernel of standard deviation `bw` (one entry or one per dimension, squared as `kde!` squares it)."
function hip_mmd(p::BallTreeDensity, q::BallTreeDensity, bw::AbstractVector{Float64}; manifold=nothing, device::Int=0)
  length(bw) == 1 || length(bw) == Ndim(p) || error("bw needs 1 or D entries")
  v = Float64[(length(bw) == 1 ? bw[1] : bw[k])^2 for k in 1:Ndim(p)]
  s(a, b) = hip_kernel_sum(a, b, v; manifold=manifold, device=device)
  return s(p, p) - 2.0 * s(p, q) + s(q, q)
end

"""
    hip_prod_exact(p, q, Np=Npts(p); seed=rand(UInt64), sample_offset=0, device=0)

`(pts, ind, logz)`: `Np` EXACT draws of the product of two densities (`kdehip_prod_exact`, include/kdehip.h section 5p) --
`pts` is `D x Np`, `ind` is `2 x Np` (the 1-based original indices of the drawn kernels of `p` and `q`), `logz` is
`log(integral of p q)`.  One all-pairs pass and two inverse-CDF walks per draw: no sweeps, no `Niter`.  Both densities
need ONE bandwidth vector.  The library's own: not installed by `enable!()`.
"""
function hip_prod_exact(p::BallTreeDensity, q::BallTreeDensity, Np::Int=Npts(p); seed::UInt64=rand(UInt64),
                        sample_offset::Int=0, device::Int=0)
  Ndim(p) == Ndim(q) || error("prod_exact -- dimensions of two BallTreeDensities must match")
  pts = zeros(Ndim(p), max(Np, 0))
  ind = zeros(Int64, 2, max(Np, 0))
  logz = Ref{Float64}(0.0)
  cp = Ref(CDensity(p))
  cq = p === q ? cp : Ref(CDensity(q))
  GC.@preserve p q pts ind begin
    check(ccall((:kdehip_prod_exact, libkdehip), Cint,
                (Ref{CDensity}, Ref{CDensity}, Int64, UInt64, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Cint),
                cp, cq, Np, seed, sample_offset, pts, ind, logz, device))
  end
  return pts, ind, logz[]
end

"`log(hip_intersIntg(p, q))` by log-sum-exp (`kdehip_prod_exact` with no draws): finite where the integral underflows to 0."
function hip_log_intersIntg(p::BallTreeDensity, q::BallTreeDensity; device::Int=0)
  Ndim(p) == Ndim(q) || error("prod_exact -- dimensions of two BallTreeDensities must match")
  logz = Ref{Float64}(0.0)
  cp = Ref(CDensity(p))
  cq = p === q ? cp : Ref(CDensity(q))
  GC.@preserve p q begin
    check(ccall((:kdehip_prod_exact, libkdehip), Cint,
                (Ref{CDensity}, Ref{CDensity}, Int64, UInt64, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Cint),
                cp, cq, 0, UInt64(0), 0, Ptr{Float64}(C_NULL), Ptr{Int64}(C_NULL), logz, device))
  end
  return logz[]
end

"""
    hip_evaluate_grad(bd, pos; log=true, manifold=nothing, device=0)

`(val, grad)` at the columns of `pos` (`kdehip_evaluate_grad`, include/kdehip.h section 5h): `log p` and its gradient
`-S_k / (S_0 v_k)`, or with `log=false` `p` and its gradient; `val` has `Nq` entries, `grad` is `D x Nq`.  `log p` and its
gradient stay finite where `p` underflows to 0.  The library's own (the reference has no gradient): not installed by
`enable!()`.
"""
function hip_evaluate_grad(bd::BallTreeDensity, pos::AbstractMatrix{Float64}; log::Bool=true, manifold=nothing, device::Int=0)
  Ndim(bd) == size(pos, 1) || error("bd and pos must have the same dimension")
  man = manifold === nothing ? zeros(UInt8, Ndim(bd)) : manifold_bytes(manifold, Ndim(bd))
  Nq = size(pos, 2)
  val = zeros(Nq)
  grad = zeros(Ndim(bd), Nq)
  cd = Ref(CDensity(bd))
  posd = Matrix{Float64}(pos)
  GC.@preserve bd posd man begin
    check(ccall((:kdehip_evaluate_grad, libkdehip), Cint,
                (Ref{CDensity}, Ptr{Float64}, Int64, Cint, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{UInt8}),
                cd, posd, Nq, log ? 1 : 0, val, grad, device, man))
  end
  return val, grad
end

"""
    hip_meanshift(bd, starts=nothing; tol=1e-9, maxiter=500, manifold=nothing, device=0)

`(x, logp, iters)` (`kdehip_meanshift`, include/kdehip.h section 5h): every column of `starts` -- `nothing`: the density's
own points, in `getPoints` order -- moved by mean-shift steps `x_k <- x_k - S_k / S_0` (wrapped to `[-pi, pi)` in a circular
dimension) on the device until a step is at most `tol` bandwidths long in every dimension, or for `maxiter` steps; `iters` =
the steps taken, negative where the last was still above `tol`; `logp` = `log p` at `x`.  Not installed by `enable!()`.
"""
function hip_meanshift(bd::BallTreeDensity, starts::Union{Nothing,AbstractMatrix{Float64}}=nothing; tol::Float64=1e-9,
                       maxiter::Int=500, manifold=nothing, device::Int=0)
  D = Ndim(bd)
  starts === nothing || D == size(starts, 1) || error("bd and starts must have the same dimension")
  man = manifold === nothing ? zeros(UInt8, D) : manifold_bytes(manifold, D)
  K = starts === nothing ? Npts(bd) : size(starts, 2)
  x = zeros(D, K)
  logp = zeros(K)
  iters = zeros(Int32, K)
  cd = Ref(CDensity(bd))
  sd = starts === nothing ? zeros(0, 0) : Matrix{Float64}(starts)
  tolv = Float64[tol]
  GC.@preserve bd sd tolv man begin
    check(ccall((:kdehip_meanshift, libkdehip), Cint,
                (Ref{CDensity}, Ptr{Float64}, Int64, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Cint, Ptr{UInt8}),
                cd, starts === nothing ? Ptr{Float64}(C_NULL) : pointer(sd), K, tolv, maxiter, x, logp, iters, device, man))
  end
  return x, logp, iters
end

"""
    hip_modes(bd, starts=nothing; tol=1e-9, maxiter=500, merge=1e-3, manifold=nothing, device=0)

`(modes, logp, mass, labels)`: `hip_meanshift`, then the converged points merged greedily -- in descending `logp`, ties by
index, a point joins the first kept mode within `merge` bandwidths (`max_k |diff_k| / sd_k`, wrapped where circular), else it
founds a new one.  `mass` = the summed weights of the starts labelled to a mode when the starts are the density's own points
(shares of the starts otherwise); an unconverged start is labelled 0 and belongs to no mode; labels are 1-based.
"""
function hip_modes(bd::BallTreeDensity, starts::Union{Nothing,AbstractMatrix{Float64}}=nothing; tol::Float64=1e-9,
                   maxiter::Int=500, merge::Float64=1e-3, manifold=nothing, device::Int=0)
  D = Ndim(bd)
  own = starts === nothing
  x, logp, iters = hip_meanshift(bd, starts; tol=tol, maxiter=maxiter, manifold=manifold, device=device)
  circ = manifold === nothing ? falses(D) : (manifold_bytes(manifold, D) .== 0x01)
  sd = getBW(bd)[:, 1]
  K = size(x, 2)
  labels = zeros(Int, K)
  kept = Int[]
  order = sort([q for q in 1:K if iters[q] >= 0]; by = q -> (-logp[q], q))
  for q in order
    home = 0
    for (j, f) in enumerate(kept)
      d = x[:, q] .- x[:, f]
      for k in 1:D
        circ[k] && (d[k] = d[k] - 2pi * floor((d[k] + pi) / 2pi))
      end
      if maximum(abs.(d) ./ sd) <= merge
        home = j
        break
      end
    end
    if home == 0
      push!(kept, q)
      home = length(kept)
    end
    labels[q] = home
  end
  w = own ? getWeights(bd) : fill(1.0 / max(K, 1), K)
  mass = Float64[sum(w[labels .== j]) for j in 1:length(kept)]
  return x[:, kept], logp[kept], mass, labels
end

"""
    hip_getKDEMode(bd; kwargs...)

The joint mode of the density: the highest of `hip_modes(bd; kwargs...)`, a local maximum of the D-dimensional density
itself.  `getKDEMax` is the grid argmax of every 1-D marginal on its own: for a multimodal density its coordinates may come
from different modes.
"""
hip_getKDEMode(bd::BallTreeDensity; kwargs...) = hip_modes(bd; kwargs...)[1][:, 1]

"""
    hip_evaluate_hess(bd, pos; manifold=nothing, device=0)

`(logp, grad, hess, cov, definite)` at the columns of `pos` (`kdehip_evaluate_hess`, include/kdehip.h section 5k): `log p`,
its gradient (`D x Nq`), its Hessian `H_kl = S_kl / (S_0 v_k v_l) - delta_kl / v_k - g_k g_l` (`D x D x Nq`, symmetric bit
for bit), `cov = (-H)^-1` by Cholesky and `definite` (`Bool`, `Nq`): where a pivot fails -- a saddle, a minimum, a flat
direction -- `definite` is false and that `cov[:, :, q]` is NaN.  The library's own: not installed by `enable!()`.
"""
function hip_evaluate_hess(bd::BallTreeDensity, pos::AbstractMatrix{Float64}; manifold=nothing, device::Int=0)
  D = Ndim(bd)
  D == size(pos, 1) || error("bd and pos must have the same dimension")
  man = manifold === nothing ? zeros(UInt8, D) : manifold_bytes(manifold, D)
  Nq = size(pos, 2)
  logp = zeros(Nq)
  grad = zeros(D, Nq)
  hess = zeros(D, D, Nq)
  cov = zeros(D, D, Nq)
  definite = zeros(Int32, Nq)
  cd = Ref(CDensity(bd))
  posd = Matrix{Float64}(pos)
  GC.@preserve bd posd man begin
    check(ccall((:kdehip_evaluate_hess, libkdehip), Cint,
                (Ref{CDensity}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Cint,
                 Ptr{UInt8}),
                cd, posd, Nq, logp, grad, hess, cov, definite, device, man))
  end
  return logp, grad, hess, cov, definite .!= 0
end

"""
    hip_fit_modes(bd, starts=nothing; kwargs...)

`(means, covs, mass, logp, definite)`: `hip_modes(bd, starts; kwargs...)`, then `hip_evaluate_hess` at the modes -- a Gaussian
per mode, in descending `logp`.  `mass` is the basin mass of `hip_modes`, not a Laplace evidence.
"""
function hip_fit_modes(bd::BallTreeDensity, starts::Union{Nothing,AbstractMatrix{Float64}}=nothing; manifold=nothing,
                       device::Int=0, kwargs...)
  means, logp, mass, _ = hip_modes(bd, starts; manifold=manifold, device=device, kwargs...)
  _, _, _, covs, definite = hip_evaluate_hess(bd, means; manifold=manifold, device=device)
  return means, covs, mass, logp, definite
end

"""
    hip_joint_bandwidth(bd, start=nothing; tol=1e-3, maxiter=200, manifold=nothing, device=0)

`(bw, logl, iters, status, trace)` (`kdehip_bandwidth_joint`, include/kdehip.h section 5q): the `D` standard deviations the
joint leave-one-out iteration `v_k <- sum_i w_i T_ik / S0_i / sum_i w_i` reaches from `start` (`D` standard deviations;
`nothing`: the density's own bandwidth) once a step changes no log standard deviation by more than `tol`, or after `maxiter`
steps.  `logl` = the leave-one-out average log-likelihood at `bw`; `iters` = the steps taken, negative where the last was still
above `tol`; `status` = 1 when degenerate data froze the iteration; `trace` = the log-likelihood of every iterate, the start
included.  `kde!(points)` searches every 1-D marginal on its own; this is the library's own: not installed by `enable!()`.
"""
function hip_joint_bandwidth(bd::BallTreeDensity, start::Union{Nothing,AbstractVector{Float64}}=nothing; tol::Float64=1e-3,
                             maxiter::Int=200, manifold=nothing, device::Int=0)
  D = Ndim(bd)
  start === nothing || length(start) == D || error("start needs one standard deviation per dimension")
  man = manifold === nothing ? zeros(UInt8, D) : manifold_bytes(manifold, D)
  bw = zeros(D)
  logl = Float64[0.0]
  iters = Int32[0]
  status = Int32[0]
  trace = fill(NaN, maxiter + 1)
  cd = Ref(CDensity(bd))
  sd = start === nothing ? zeros(0) : Vector{Float64}(start)
  tolv = Float64[tol]
  GC.@preserve bd sd tolv man begin
    check(ccall((:kdehip_bandwidth_joint, libkdehip), Cint,
                (Ref{CDensity}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64},
                 Cint, Ptr{UInt8}),
                cd, start === nothing ? Ptr{Float64}(C_NULL) : pointer(sd), tolv, maxiter, bw, logl, iters, status, trace, device,
                man))
  end
  return bw, logl[1], Int(iters[1]), Int(status[1]), trace[1:abs(Int(iters[1])) + 1]
end

"""
    hip_kde_joint(points[, weights]; start=nothing, tol=1e-3, maxiter=200, manifold=nothing, tree_manifold=nothing, device=0)

`kde!(points, bw, weights)` with the joint bandwidth of `hip_joint_bandwidth`.  `start=nothing` starts the iteration from the
bandwidth `kde!(points)` selects, so the result is never worse than `kde!(points)` in leave-one-out likelihood.
"""
function hip_kde_joint(points::AbstractMatrix{Float64}, weights::Union{Nothing,Vector{Float64}}=nothing;
                       start::Union{Nothing,AbstractVector{Float64}}=nothing, tol::Float64=1e-3, maxiter::Int=200,
                       manifold=nothing, tree_manifold=nothing, device::Int=0)
  s = start !== nothing ? Vector{Float64}(start) :
      manifold === nothing ? auto_bandwidth(points; device=device) : hip_auto_bandwidth(points, manifold; device=device)
  p0 = kde!(points, s, weights; tree_manifold=tree_manifold)
  bw, _, _, _, _ = hip_joint_bandwidth(p0; tol=tol, maxiter=maxiter, manifold=manifold, device=device)
  return kde!(points, bw, weights; tree_manifold=tree_manifold)
end

# the first leaf's variances: the one bandwidth vector of a density that kde! built
leaf_variances(bd::BallTreeDensity) = bd.bandwidth[bd.bt.num_points * bd.bt.dims .+ (1:bd.bt.dims)]

"""
    hip_sinkhorn(p, q; reg=1.0, scale=nothing, tol=1e-6, maxiter=1000, manifold=nothing, device=0)

Entropic optimal transport between the points of `p` and of `q` (`kdehip_sinkhorn`, include/kdehip.h section 5s): the cost is
`1/2 sum_k diff_k^2 / scale_k^2` (`scale=nothing`: `sqrt(v_p + v_q)`, the bandwidths combined), `reg` its entropic weight;
`q === p` runs the symmetric iteration of `p` against itself.  Returns a named tuple: `value` (the dual objective),
`transport_cost`, `err` (the L1 row-marginal error at the stop), `mass`, `iters` (negative where the last step was still above
`tol`), the potentials `phi`, `gamma`, and `delta`, `map` (`D x N`): the barycentric displacement and image of every point
of `p`, all in the order of `getPoints`.  The library's own: not installed by `enable!()`.
"""
function hip_sinkhorn(p::BallTreeDensity, q::BallTreeDensity; reg::Float64=1.0, scale::Union{Nothing,AbstractVector{Float64}}=nothing,
                      tol::Float64=1e-6, maxiter::Int=1000, manifold=nothing, device::Int=0)
  D = Ndim(p)
  Ndim(q) == D || error("the two densities must have the same dimension")
  scale === nothing || length(scale) == D || error("scale needs one entry per dimension")
  man = manifold === nothing ? zeros(UInt8, D) : manifold_bytes(manifold, D)
  N, M = p.bt.num_points, q.bt.num_points
  vals = zeros(4)
  iters = Int32[0]
  phi, gamma, delta, tmap = zeros(N), zeros(M), zeros(D, N), zeros(D, N)
  cp = Ref(CDensity(p))
  cq = q === p ? cp : Ref(CDensity(q))
  sc = scale === nothing ? zeros(0) : Vector{Float64}(scale)
  regv, tolv = Float64[reg], Float64[tol]
  GC.@preserve p q sc regv tolv man vals begin
    check(ccall((:kdehip_sinkhorn, libkdehip), Cint,
                (Ref{CDensity}, Ref{CDensity}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{UInt8}),
                cp, cq, scale === nothing ? Ptr{Float64}(C_NULL) : pointer(sc), regv, tolv, maxiter, pointer(vals, 1),
                pointer(vals, 2), pointer(vals, 3), pointer(vals, 4), iters, phi, gamma, delta, tmap, device, man))
  end
  return (value=vals[1], transport_cost=vals[2], err=vals[3], mass=vals[4], iters=Int(iters[1]), phi=phi, gamma=gamma,
          delta=delta, map=tmap)
end

"""
    hip_sinkhorn_divergence(p, q; reg=1.0, scale=nothing, tol=1e-6, maxiter=1000, manifold=nothing, device=0)

`S(p, q) = value(p, q) - value(p, p) / 2 - value(q, q) / 2`, all three at ONE scale (`scale=nothing`: the pair's
`sqrt(v_p + v_q)`); `0.0` for `q === p`, by definition.
"""
function hip_sinkhorn_divergence(p::BallTreeDensity, q::BallTreeDensity; reg::Float64=1.0,
                                 scale::Union{Nothing,AbstractVector{Float64}}=nothing, tol::Float64=1e-6, maxiter::Int=1000,
                                 manifold=nothing, device::Int=0)
  q === p && return 0.0
  s = scale === nothing ? sqrt.(leaf_variances(p) .+ leaf_variances(q)) : Vector{Float64}(scale)
  value(a, b) = hip_sinkhorn(a, b; reg=reg, scale=s, tol=tol, maxiter=maxiter, manifold=manifold, device=device).value
  return value(p, q) - value(p, p) / 2 - value(q, q) / 2
end

"""
    hip_transport_map(p, q; reg=1.0, scale=nothing, tol=1e-6, maxiter=1000, manifold=nothing, device=0)

`T` (`D x N`): the barycentric image of every point of `p` under the entropic plan onto `q`, in the order of `getPoints`
(wrapped to `[-pi, pi)` in a circular dimension).  `movePoints!(p, T - getPoints(p))` moves `p` there.
"""
function hip_transport_map(p::BallTreeDensity, q::BallTreeDensity; reg::Float64=1.0,
                           scale::Union{Nothing,AbstractVector{Float64}}=nothing, tol::Float64=1e-6, maxiter::Int=1000,
                           manifold=nothing, device::Int=0)
  return hip_sinkhorn(p, q; reg=reg, scale=scale, tol=tol, maxiter=maxiter, manifold=manifold, device=device).map
end

"""
    hip_herding_order(p, M; bw=nothing, manifold=nothing, stepwise=false, device=0)

The first `M` kernel-herding picks of `p` (`kdehip_compress`, include/kdehip.h section 5t) under the Gaussian kernel of
standard deviation `bw` (one entry per dimension; `nothing`: `sqrt(2)` times the bandwidth of `p`).  Returns a named tuple:
`idx` (1-based, by original point, in pick order), `zpick`, `rpick`, `self_sum` and `mmd2`, the squared MMD (not
normalised) between `p` and the equal-weight density on the first `1 .. M` picks.  The first `m` picks of a run to `M` are
the run to `m`.  The library's own: not installed by `enable!()`.
"""
function hip_herding_order(p::BallTreeDensity, M::Int; bw::Union{Nothing,AbstractVector{Float64}}=nothing, manifold=nothing,
                           stepwise::Bool=false, device::Int=0)
  D = Ndim(p)
  1 <= M <= p.bt.num_points || error("M must lie in 1..Npts(p)")
  bw === nothing || length(bw) == D || error("bw needs one entry per dimension")
  man = manifold === nothing ? zeros(UInt8, D) : manifold_bytes(manifold, D)
  var = bw === nothing ? zeros(0) : Vector{Float64}(bw) .* Vector{Float64}(bw)
  idx, zpick, rpick, self = zeros(Int64, M), zeros(M), zeros(M), zeros(1)
  cp = Ref(CDensity(p))
  GC.@preserve p var man begin
    check(ccall((:kdehip_compress, libkdehip), Cint,
                (Ref{CDensity}, Int64, Ptr{Float64}, Cint, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{UInt8}),
                cp, M, bw === nothing ? Ptr{Float64}(C_NULL) : pointer(var), stepwise ? 1 : 0, idx, zpick, rpick, self, device, man))
  end
  m = collect(1.0:M)
  mmd2 = self[1] .- (2.0 ./ m) .* cumsum(zpick) .+ (m .+ 2.0 .* cumsum(rpick)) ./ (m .* m)
  return (idx=idx, zpick=zpick, rpick=rpick, self_sum=self[1], mmd2=mmd2)
end

"""
    hip_compress(p, M; bw=nothing, ks=nothing, manifold=nothing, device=0)

`p` cut to `M` of its own points by kernel herding: `kde!(getPoints(p)[:, idx], ks, fill(1/M, M))` with `idx` the picks of
`hip_herding_order` and `ks` the bandwidth of the result (`nothing`: unchanged).
"""
function hip_compress(p::BallTreeDensity, M::Int; bw::Union{Nothing,AbstractVector{Float64}}=nothing,
                      ks::Union{Nothing,AbstractVector{Float64}}=nothing, manifold=nothing, device::Int=0)
  order = hip_herding_order(p, M; bw=bw, manifold=manifold, device=device)
  sd = ks === nothing ? sqrt.(leaf_variances(p)) : Vector{Float64}(ks)
  return kde!(getPoints(p)[:, order.idx], sd, fill(1.0 / M, M))
end

"`compress` of a resident density as a new handle (`kdehip_density_compress_device`): the picks never leave the device but for the builder's one copy."
function hip_compress(d::DeviceDensity, M::Int; bw::Union{Nothing,AbstractVector{Float64}}=nothing,
                      ks::Union{Nothing,AbstractVector{Float64}}=nothing, manifold=nothing, tree_manifold=nothing)
  D = d.ndim
  man = manifold === nothing ? zeros(UInt8, D) : manifold_bytes(manifold, D)
  tman = tree_manifold === nothing ? zeros(UInt8, D) : manifold_bytes(tree_manifold, D)
  var = bw === nothing ? zeros(0) : Vector{Float64}(bw) .* Vector{Float64}(bw)
  sd = ks === nothing ? zeros(0) : Vector{Float64}(ks)
  h = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve var sd man tman begin
    check(ccall((:kdehip_density_compress_device, libkdehip), Cint,
                (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{UInt8}),
                h, d.handle, M, bw === nothing ? Ptr{Float64}(C_NULL) : pointer(var),
                ks === nothing ? Ptr{Float64}(C_NULL) : pointer(sd), man, tman))
  end
  return DeviceDensity(h[])
end

"""
    hip_box_mass(bd, lo, hi; dims=nothing, manifold=nothing, device=0)

The probability that `x[dims]` lies in the box `[lo[:, q], hi[:, q]]` under `bd`, one value per column
(`kdehip_box_mass`, include/kdehip.h section 5l): `lo` and `hi` are `nb x Nq`, their rows in the order of `dims` (1-based,
distinct; `nothing`: every dimension).  `-Inf` and `Inf` are bounds like any other, `lo >= hi` in a dimension gives exactly 0,
a NaN bound gives NaN for that box only.  A circular dimension cannot be bounded.  The library's own: not installed by
`enable!()`.
"""
function hip_box_mass(bd::BallTreeDensity, lo::AbstractMatrix{Float64}, hi::AbstractMatrix{Float64}; dims=nothing,
                      manifold=nothing, device::Int=0)
  D = Ndim(bd)
  dl = dims === nothing ? collect(1:D) : collect(Int, dims)
  (length(dl) >= 1 && allunique(dl) && all(d -> 1 <= d <= D, dl)) || error("dims must be distinct dimensions of bd, 1-based")
  (size(lo) == size(hi) && size(lo, 1) == length(dl)) || error("lo and hi hold one row per bounded dimension")
  man = manifold === nothing ? zeros(UInt8, D) : manifold_bytes(manifold, D)
  order = sortperm(dl)
  mask = UInt64(0)
  for d in dl
    mask |= UInt64(1) << (d - 1)
  end
  Nq = size(lo, 2)
  lod = Matrix{Float64}(lo[order, :])
  hid = Matrix{Float64}(hi[order, :])
  mass = zeros(Nq)
  cd = Ref(CDensity(bd))
  GC.@preserve bd lod hid man begin
    check(ccall((:kdehip_box_mass, libkdehip), Cint,
                (Ref{CDensity}, UInt64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Cint, Ptr{UInt8}),
                cd, mask, lod, hid, Nq, mass, device, man))
  end
  return mass
end

"""
    hip_quantile(bd, alpha, dim; tol=1e-12, max_iter=100, manifold=nothing, device=0)

`(x, resid, iters, converged)`: the `alpha` quantiles of the marginal of dimension `dim` (1-based) of `bd`
(`kdehip_quantile`, include/kdehip.h section 5l), by a bracketed Newton iteration on the device: `cdf(x) = alpha` to `tol`
(absolute in the cdf); `resid = cdf(x) - alpha` at the returned `x`, `iters` the number of cdf evaluations, `converged`
false where `max_iter` evaluations did not reach `tol`.  An `alpha` outside (0, 1) or NaN gives NaN for that level only.
"""
function hip_quantile(bd::BallTreeDensity, alpha::AbstractVector{Float64}, dim::Int; tol::Float64=1e-12, max_iter::Int=100,
                      manifold=nothing, device::Int=0)
  D = Ndim(bd)
  1 <= dim <= D || error("dim must be a dimension of bd, 1-based")
  man = manifold === nothing ? zeros(UInt8, D) : manifold_bytes(manifold, D)
  Nq = length(alpha)
  av = Vector{Float64}(alpha)
  tolv = [tol]
  x = zeros(Nq)
  resid = zeros(Nq)
  iters = zeros(Int32, Nq)
  converged = zeros(Int32, Nq)
  cd = Ref(CDensity(bd))
  GC.@preserve bd av tolv man begin
    check(ccall((:kdehip_quantile, libkdehip), Cint,
                (Ref{CDensity}, Cint, Ptr{Float64}, Int64, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32},
                 Cint, Ptr{UInt8}),
                cd, dim - 1, av, Nq, tolv, max_iter, x, resid, iters, converged, device, man))
  end
  return x, resid, iters, converged .!= 0
end

"""
    hip_getKDEMax(p; N=200, device=0)

`getKDEMax(p; N)` (src/DualTree01.jl:558-570) on the GPU (`kdehip_kde_max`, include/kdehip.h section 5c): per dimension the
1-D marginal on the N-point grid over its range with extend 0.1, by the direct sum, and the grid point of the FIRST maximum.
The grid is lo + k h, each operation rounded on its own, where `range` forms its points in double-double: they may differ
in the last bit.  Not installed by `enable!()`.
"""
function hip_getKDEMax(p::BallTreeDensity; N::Int=200, device::Int=0)
  m = zeros(Ndim(p))
  cd = Ref(CDensity(p))
  GC.@preserve p begin
    check(ccall((:kdehip_kde_max, libkdehip), Cint, (Ref{CDensity}, Int64, Ptr{Float64}, Ptr{Float64}, Cint),
                cd, N, m, C_NULL, device))
  end
  return m
end

"The same for a resident density (`kdehip_density_summary`, extend 0.1)."
function hip_getKDEMax(d::DeviceDensity; N::Int=200)
  m = zeros(d.ndim)
  check(ccall((:kdehip_density_summary, libkdehip), Cint,
              (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
              d.handle, C_NULL, N, C_NULL, C_NULL, C_NULL, m, C_NULL))
  return m
end

"""
    hip_getKDEfit(d::DeviceDensity)

`getKDEfit(p)` (src/DualTree01.jl:574-578) = `fit(MvNormal, getPoints(p))` of a resident density (`kdehip_density_summary`):
the sequential mean of getKDEMean and the MLE covariance (1/N) sum (x - mu)(x - mu)', summed in original point order.
A host density: `hip_getKDEfit(DeviceDensity(p))`.  Not installed by `enable!()`.
"""
function hip_getKDEfit(d::DeviceDensity)
  D = d.ndim
  mu = zeros(D)
  sig = zeros(D, D)
  check(ccall((:kdehip_density_summary, libkdehip), Cint,
              (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
              d.handle, C_NULL, 2, C_NULL, mu, sig, C_NULL, C_NULL))
  return KDE.MvNormal(mu, sig)
end
hip_getKDEfit(p::BallTreeDensity; device::Int=0) = hip_getKDEfit(DeviceDensity(p; device=device))

"""
    hip_intersIntgAppxIS(p, q; N=201, device=0)

`intersIntgAppxIS(p, q; N)` (src/DualTree01.jl:581-618) for 1-D and 2-D densities (`kdehip_inters_intg_appx_is`): p and q
evaluated by the direct sum on the grid over p's marginal ranges with extend 0.3, the products summed row by row in order
(the reference's `sum` is pairwise: equal to a tolerance).  Not installed by `enable!()`.
"""
function hip_intersIntgAppxIS(p::BallTreeDensity, q::BallTreeDensity; N::Int=201, device::Int=0)
  out = Ref{Float64}(0.0)
  cp = Ref(CDensity(p))
  cq = Ref(CDensity(q))
  GC.@preserve p q begin
    check(ccall((:kdehip_inters_intg_appx_is, libkdehip), Cint, (Ref{CDensity}, Ref{CDensity}, Int64, Ptr{Float64}, Cint),
                cp, cq, N, out, device))
  end
  return out[]
end

# ---- the same functions on a manifold (include/kdehip.h section 5e).  `manifold`: a vector of `:euclid` / `:circular` (or
# 0 / 1), one per dimension -- the library's circular semantic (wrap to [-pi, pi), tangent offsets at original point 1's
# angle), which a caller's own addop / diffop need not share: as with the other manifold functions, nothing maps the
# reference's operator arguments to it automatically.  Module functions, not installed by `enable!()`.

"`hip_sample` with the drawn coordinates of the circular dimensions wrapped to [-pi, pi) (`kdehip_sample_manifold`)."
function hip_sample(bd::BallTreeDensity, Npts::Int, manifold::AbstractVector, ind::Union{Nothing,Vector{Int}}=nothing;
                    seed::Union{Nothing,UInt64}=nothing, sample_offset::Int=0, device::Int=0)
  D = Ndim(bd)
  man = manifold_bytes(manifold, D)
  pts = zeros(D, Npts)
  out = zeros(Int, Npts)
  s = seed === nothing ? rand(UInt64) : seed
  cd = Ref(CDensity(bd))
  lab = ind === nothing ? C_NULL : Vector{Int64}(ind)
  GC.@preserve bd lab man begin
    check(ccall((:kdehip_sample_manifold, libkdehip), Cint,
                (Ref{CDensity}, Int64, UInt64, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Cint, Ptr{UInt8}),
                cd, Npts, s, sample_offset, lab, pts, out, device, man))
  end
  return pts, out
end

hip_rand(p::BallTreeDensity, manifold::AbstractVector, N::Int=1; seed::Union{Nothing,UInt64}=nothing) =
  hip_sample(p, N, manifold; seed=seed)[1]

"`resample(p, Np, :lcv)` on a manifold: the wrapped draw, then `kde!(pts; manifold, tree_manifold=manifold)`."
function hip_resample(p::BallTreeDensity, manifold::AbstractVector, Np::Int=-1, ksType::Symbol=:lcv;
                      seed::Union{Nothing,UInt64}=nothing)
  ksType == :lcv || error("hip_resample: only ksType = :lcv")
  n = Np <= 0 ? Npts(p) : Np
  pts, = hip_sample(p, n, manifold; seed=seed)
  return kde!(pts; manifold=manifold, tree_manifold=manifold)
end

"`resample` of a resident density without leaving the device (`kdehip_resample_device_manifold`)."
function hip_resample(d::DeviceDensity, manifold::AbstractVector, Np::Int=-1; seed::Union{Nothing,UInt64}=nothing,
                      tree_manifold::AbstractVector=manifold)
  man = manifold_bytes(manifold, d.ndim)
  tman = manifold_bytes(tree_manifold, d.ndim)
  s = seed === nothing ? rand(UInt64) : seed
  h = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve man tman begin
    check(ccall((:kdehip_resample_device_manifold, libkdehip), Cint,
                (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Int64, UInt64, Ptr{Float64}, Ptr{Int32}, Ptr{UInt8}, Ptr{UInt8}),
                h, d.handle, Np, s, C_NULL, C_NULL, man, tman))
  end
  return DeviceDensity(h[])
end

# changeWeights! / movePoints! and the Bayes update of a resident density as NEW handles (include/kdehip.h section 5r): the
# tree stays, the node statistics are recomputed on the device.  d_values / d_delta are DEVICE pointers (npts doubles by
# original point, or by leaf position with leaf_order=true; ndims x npts column-major); the calls block.
function hip_refit(d::DeviceDensity, d_values::Ptr{Float64}, kind::Int, d_delta::Ptr{Float64}, leaf_order::Bool, tree_manifold)
  tman = tree_manifold === nothing ? UInt8[] : manifold_bytes(tree_manifold, d.ndim)
  h = Ref{Ptr{Cvoid}}(C_NULL)
  res = zeros(Float64, 2)  # log evidence, effective sample size
  GC.@preserve tman res begin
    check(ccall((:kdehip_density_refit_device, libkdehip), Cint,
                (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Float64}, Cint, Cint, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}),
                h, d.handle, d_values, kind, leaf_order ? 1 : 0, d_delta, isempty(tman) ? C_NULL : pointer(tman),
                pointer(res), pointer(res) + 8))
  end
  return DeviceDensity(h[]), res[1], res[2]
end

"`changeWeights!(bd, newWeights)` (reference src/BallTreeDensity01.jl:298-309) of a resident density, as a new handle."
function hip_changeWeights(d::DeviceDensity, d_weights::Ptr{Float64}; leaf_order::Bool=false, tree_manifold=nothing)
  return hip_refit(d, d_weights, 1, Ptr{Float64}(C_NULL), leaf_order, tree_manifold)[1]
end

"`movePoints!(bd, delta)` (reference src/BallTreeDensity01.jl:281-296) of a resident density, as a new handle."
function hip_movePoints(d::DeviceDensity, d_delta::Ptr{Float64}; leaf_order::Bool=false, tree_manifold=nothing)
  return hip_refit(d, Ptr{Float64}(C_NULL), 0, d_delta, leaf_order, tree_manifold)[1]
end

"`w_i <- w_i exp(l_i)`, normalised, on a resident density: (new handle, log evidence, effective sample size)."
function hip_bayes_update(d::DeviceDensity, d_logl::Ptr{Float64}; leaf_order::Bool=false, tree_manifold=nothing)
  return hip_refit(d, d_logl, 2, Ptr{Float64}(C_NULL), leaf_order, tree_manifold)
end

"`marginal(p, dims)` of a resident density, its tree built with `tree_manifold[dims]` (`kdehip_density_marginal_device_tree`)."
function hip_marginal(d::DeviceDensity, dims::Vector{Int}, tree_manifold::AbstractVector)
  tman = manifold_bytes(tree_manifold, d.ndim)[dims]
  sel = Vector{Int32}(dims)
  h = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve sel tman begin
    check(ccall((:kdehip_density_marginal_device_tree, libkdehip), Cint,
                (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Cint, Ptr{Int32}, Ptr{UInt8}), h, d.handle, length(sel), sel, tman))
  end
  return DeviceDensity(h[])
end

"`getKDEMax(p, addop, diffop; N)` with the library's circular operators (`kdehip_kde_max_manifold`): the argmax wrapped."
function hip_getKDEMax(p::BallTreeDensity, manifold::AbstractVector; N::Int=200, device::Int=0)
  man = manifold_bytes(manifold, Ndim(p))
  m = zeros(Ndim(p))
  cd = Ref(CDensity(p))
  GC.@preserve p man begin
    check(ccall((:kdehip_kde_max_manifold, libkdehip), Cint,
                (Ref{CDensity}, Int64, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{UInt8}), cd, N, m, C_NULL, device, man))
  end
  return m
end

# (range: D x 2 column-major, mean: D, cov: D x D, argmax: D; any of them `nothing` to skip)
function summary_manifold(d::DeviceDensity, manifold::AbstractVector, extend::Float64, N::Int, range, mean, cov, argmax)
  man = manifold_bytes(manifold, d.ndim)
  ext = Ref{Float64}(extend)
  p(x) = x === nothing ? Ptr{Float64}(C_NULL) : pointer(x)
  GC.@preserve man range mean cov argmax begin
    check(ccall((:kdehip_density_summary_manifold, libkdehip), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{UInt8}), d.handle, ext, N, p(range), p(mean), p(cov), p(argmax), C_NULL, man))
  end
  return nothing
end

function hip_getKDEMax(d::DeviceDensity, manifold::AbstractVector; N::Int=200)
  m = zeros(d.ndim)
  summary_manifold(d, manifold, 0.1, N, nothing, nothing, nothing, m)
  return m
end

"`getKDERange(p, addop, diffop; extend)` on the circle: the unwrapped arc per circular dimension (section 5e)."
function hip_getKDERange(d::DeviceDensity, manifold::AbstractVector; extend::Float64=0.1)
  r = zeros(d.ndim, 2)
  summary_manifold(d, manifold, extend, 2, r, nothing, nothing, nothing)
  return r
end

"`getKDEMean` on the circle: wrap(a0 + mean of the tangent offsets) per circular dimension (section 5e)."
function hip_getKDEMean(d::DeviceDensity, manifold::AbstractVector)
  mu = zeros(d.ndim)
  summary_manifold(d, manifold, 0.1, 2, nothing, mu, nothing, nothing)
  return mu
end

"`getKDEfit` on the circle: the circular mean and the covariance of the wrapped residuals."
function hip_getKDEfit(d::DeviceDensity, manifold::AbstractVector)
  mu = zeros(d.ndim)
  sig = zeros(d.ndim, d.ndim)
  summary_manifold(d, manifold, 0.1, 2, nothing, mu, sig, nothing)
  return KDE.MvNormal(mu, sig)
end

"`intersIntgAppxIS(p, q, addop, diffop; N)` with the library's circular operators (`kdehip_inters_intg_appx_is_manifold`)."
function hip_intersIntgAppxIS(p::BallTreeDensity, q::BallTreeDensity, manifold::AbstractVector; N::Int=201, device::Int=0)
  man = manifold_bytes(manifold, Ndim(p))
  out = Ref{Float64}(0.0)
  cp = Ref(CDensity(p))
  cq = Ref(CDensity(q))
  GC.@preserve p q man begin
    check(ccall((:kdehip_inters_intg_appx_is_manifold, libkdehip), Cint,
                (Ref{CDensity}, Ref{CDensity}, Int64, Ptr{Float64}, Cint, Ptr{UInt8}), cp, cq, N, out, device, man))
  end
  return out[]
end

"""
    kde!(points)

`kde!(points)` (src/KDE01.jl:3-27) in ONE library call (`kdehip_make_density_auto`): the per-dimension LOOCV bandwidth is
searched on the GPU while the library's pooled host builder makes the ball tree (topology, bounding boxes, weights and
means do not depend on the bandwidth); the variances are filled in afterwards.  The arrays are those of
`kde!(points, bw)` with the bandwidth found, bit for bit.

`manifold` / `tree_manifold` (vectors of `:euclid` / `:circular`, or `nothing`): the bandwidth search's and the tree
builder's operators as the library's enum (`kdehip_make_density_auto_tree`); the reference's `kde!(points, addop, diffop)`
with circular operators of THIS semantic is both set to the same value.  Never chosen automatically.
"""
function kde!(points::AbstractMatrix{Float64}; device::Int=0, manifold::Union{Nothing,AbstractVector}=nothing,
              tree_manifold::Union{Nothing,AbstractVector}=nothing)
  D, N = size(points)
  on_manifold = manifold !== nothing || tree_manifold !== nothing
  (N < 2 || D > 8) && !on_manifold && return reference_kde_auto(points)   # (the library's limits: the reference path)
  bw = zeros(D)
  nev = Ref{Int32}(0)
  pts = Matrix{Float64}(points)
  centers, ranges, means, bandwidth = zeros(2N * D), zeros(2N * D), zeros(2N * D), zeros(2N * D)
  bwmin, bwmax, w = zeros(N * D), zeros(N * D), zeros(2N)
  left, right, lowest, highest, perm = zeros(Int, 2N), zeros(Int, 2N), zeros(Int, 2N), zeros(Int, 2N), zeros(Int, 2N)
  if !on_manifold
    check(ccall((:kdehip_make_density_auto, libkdehip), Cint,
                (Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ref{Int32}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}),
                D, N, pts, bw, nev, device, centers, ranges, w, left, right, lowest, highest, perm, means, bandwidth, bwmin,
                bwmax))
  else
    man = manifold === nothing ? zeros(UInt8, D) : manifold_bytes(manifold, D)
    tman = tree_manifold === nothing ? zeros(UInt8, D) : manifold_bytes(tree_manifold, D)
    GC.@preserve man tman begin
      check(ccall((:kdehip_make_density_auto_tree, libkdehip), Cint,
                  (Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ref{Int32}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}, Ptr{UInt8}, Ptr{UInt8}),
                  D, N, pts, bw, nev, device, centers, ranges, w, left, right, lowest, highest, perm, means, bandwidth, bwmin,
                  bwmax, man, tman))
    end
  end
  return density_from_arrays(D, N, centers, ranges, w, left, right, lowest, highest, perm, means, bandwidth, bwmin, bwmax)
end

"""
    auto_bandwidth(points)

The bandwidth `kde!(points)` selects (D standard deviations; `kdehip_auto_bandwidth`), without building the density.
"""
function auto_bandwidth(points::AbstractMatrix{Float64}; device::Int=0)
  D, N = size(points)
  bw = zeros(D)
  nev = Ref{Int32}(0)
  pts = Matrix{Float64}(points)
  check(ccall((:kdehip_auto_bandwidth, libkdehip), Cint, (Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ref{Int32}, Cint),
              D, N, pts, bw, nev, device))
  return bw
end

"""
    enable!(; kde=false, trees=false, evaluate=false)

Route `KernelDensityEstimate.prodAppxMSGibbsS` and `KernelDensityEstimate.gibbs1` -- and with them `*` and every
downstream caller -- through libkdehip.so (method overwrites).  A product called without `randU`/`randN`
takes the device-RNG one-shot entry (`kdehip_prod_philox`: no host `rand`/`randn`, no upload of the streams);
explicit streams are consumed in the reference's order by the `gibbs1` override.  The reference's own methods
stay reachable for non-Euclidean manifolds and for shapes beyond the compiled limits: they are invoked in the
world age in which they were defined.

The callers either side of the product are OPT-IN by keyword (all off by default: none of this file has been executed
yet -- no Julia in the build image -- so the default keeps the blast radius at the two hot-path methods; switch them on
once `oracle/julia_crosscheck.jl --shim` has passed on your installation): `kde` = `kde!(points)` (LOOCV
bandwidth + tree in one library call), `trees` = `kde!(points, ks)` and `kde!(points, ks, weights)` (every tree of every
caller built by the library's pooled builder instead of the reference's single-threaded quick-select), `evaluate` = both
forms of `evaluateDualTree`.  An override whose reference method cannot be found by its signature (another version of
KernelDensityEstimate.jl) is skipped with a warning: the reference method stays in place.
"""
function enable!(; kde::Bool=false, trees::Bool=false, evaluate::Bool=false)
  devicecount() > 0 || error("libkdehip: no MI355X visible; refusing to enable (no CPU fallback in the library)")
  ORIGINAL_GIBBS1[] === nothing || return nothing   # already enabled
  orig = KDE.gibbs1
  m = first(methods(orig))
  invoke_original(args...; kw...) = Base.invoke_in_world(m.primary_world, orig, args...; kw...)
  origprod = KDE.prodAppxMSGibbsS
  mp = first(mm for mm in methods(origprod) if mm.nargs == 5)   # the keyword method: 4 positional arguments
  invoke_original_prod(args...; kw...) = Base.invoke_in_world(mp.primary_world, origprod, args...; kw...)
  ORIGINAL_GIBBS1[] = invoke_original
  ORIGINAL_PROD[] = invoke_original_prod
  # kde!(points, addop, diffop) (src/KDE01.jl:3-27), kde!(points, ks, addop, diffop) (:64-76), kde!(points, ks, weights,
  # addop, diffop) (:34-57) and the matrix / density forms of evaluateDualTree (src/DualTree01.jl:370-421): found by
  # concrete argument types, invoked in the world they were defined in; a miss leaves the reference method in place
  origkde = KDE.kde!
  origeval = KDE.evaluateDualTree
  Pl, Mi = Tuple{typeof(+)}, Tuple{typeof(-)}
  function saved(f, sig, what)
    try
      mth = which(f, sig)
      return (args...) -> Base.invoke_in_world(mth.primary_world, f, args...)
    catch err
      @warn "KernelDensityEstimateHIP.enable!: reference method not found, override skipped" what err
      return nothing
    end
  end
  kde_auto = kde ? saved(origkde, Tuple{Matrix{Float64},Pl,Mi}, "kde!(points, addop, diffop)") : nothing
  kde_bw = trees ? saved(origkde, Tuple{Matrix{Float64},Vector{Float64},Pl,Mi}, "kde!(points, ks, addop, diffop)") : nothing
  kde_bww = trees ? saved(origkde, Tuple{Matrix{Float64},Vector{Float64},Vector{Float64},Pl,Mi}, "kde!(points, ks, weights, addop, diffop)") : nothing
  eval_m = evaluate ? saved(origeval, Tuple{BallTreeDensity,Matrix{Float64},Bool,Float64,Pl,Mi}, "evaluateDualTree(bd, pos::Matrix)") : nothing
  eval_b = evaluate ? saved(origeval, Tuple{BallTreeDensity,BallTreeDensity,Bool,Float64,Pl,Mi}, "evaluateDualTree(bd, pos::BallTreeDensity)") : nothing
  kde_auto === nothing || (ORIGINAL_KDE_AUTO[] = kde_auto)
  kde_bw === nothing || (ORIGINAL_KDE_BW[] = kde_bw)
  kde_bww === nothing || (ORIGINAL_KDE_BWW[] = kde_bww)
  eval_m === nothing || (ORIGINAL_EVAL[] = eval_m)
  eval_b === nothing || (ORIGINAL_EVAL_BD[] = eval_b)
  @eval KDE function gibbs1(Ndens::Int, trees::Array{BallTreeDensity,1}, Np::Int, Niter::Int,
                            pts::Array{Float64,1}, ind::Array{Int}, randU::Array{Float64,1},
                            randN::Array{Float64,1}; addop=(+,), diffop=(-,), getMu=(getEuclidMu,),
                            getLambda=(getEuclidLambda,), glbs=makeEmptyGbGlb(), addEntropy::Bool=true,
                            ndims::Int=maximum(Ndim.(trees)),
                            partialDimMask::AbstractVector{<:BitVector}=[ones(Int, ndims) .== 1 for i in 1:Ndens])
    if $(isEuclid)(addop, diffop, getMu, getLambda)
      return $(gibbs1)(Ndens, trees, Np, Niter, pts, ind, randU, randN; glbs=glbs, addEntropy=addEntropy,
                       ndims=ndims, partialDimMask=partialDimMask)
    end
    return $(invoke_original)(Ndens, trees, Np, Niter, pts, ind, randU, randN; addop=addop, diffop=diffop,
                              getMu=getMu, getLambda=getLambda, glbs=glbs, addEntropy=addEntropy, ndims=ndims,
                              partialDimMask=partialDimMask)
  end
  # the front end: the reference's keyword list (src/MSGibbs01.jl:645-664) with `nothing` in place of the eager
  # rand(...) / randn(...) defaults, so that "no streams given" can be told from "streams given"
  @eval KDE function prodAppxMSGibbsS(npd0::BallTreeDensity, trees::Array{BallTreeDensity,1}, anFcns, anParams;
                                      Niter::Int=3, addop=(+,), diffop=(-,), getMu=(getEuclidMu,),
                                      getLambda=(getEuclidLambda,), glbs=makeEmptyGbGlb(), addEntropy::Bool=true,
                                      ndims::Integer=maximum(Ndim.(trees)), Ndens=length(trees), Np=Npts(npd0),
                                      maxNp=maximum([Np; Npts.(trees)]),
                                      Nlevels=floor(Int, (log(Float64(maxNp)) / log(2.0)) + 1.0),
                                      randU=nothing, randN=nothing,
                                      partialDimMask::AbstractVector{<:BitVector}=[ones(Int, ndims) .== 1 for i in 1:length(trees)])
    return $(prodAppxMSGibbsS)(npd0, trees, anFcns, anParams; Niter=Niter, addop=addop, diffop=diffop, getMu=getMu,
                               getLambda=getLambda, glbs=glbs, addEntropy=addEntropy, ndims=ndims, Ndens=Ndens,
                               Np=Np, maxNp=maxNp, Nlevels=Nlevels, randU=randU, randN=randN,
                               partialDimMask=partialDimMask)
  end
  # kde!(points) -- the second half of `*` (src/MSGibbs01.jl:725) and of every README usage: LOOCV bandwidth search on the
  # GPU and the tree on the library's host pool, one call (kdehip_make_density_auto)
  kde_auto === nothing || @eval KDE function kde!(points::A, addop::Tuple=(+,), diffop::Tuple=(-,)) where {A <: AbstractArray{Float64,2}}
    if $(isEuclidOps)(addop, diffop) && size(points, 2) >= 2 && size(points, 1) <= 8
      return $(kde!)(points)
    end
    return $(reference_kde_auto)(points, addop, diffop)
  end
  # kde!(points, ks) / kde!(points, ks, weights) -- every tree any caller builds (src/KDE01.jl:34-76): the library's pooled
  # builder (kdehip_make_density); same signatures as the reference's methods, so these definitions replace them
  kde_bw === nothing || @eval KDE function kde!(points::A, ks::Array{Float64,1}, addop::Tuple=(+,), diffop::Tuple=(-,)) where {A <: AbstractArray{Float64,2}}
    if $(builds_here)(points, ks, addop, diffop)
      return $(kde!)(points, ks, nothing)
    end
    return $(reference_kde_bw)(points, ks, addop, diffop)
  end
  kde_bww === nothing || @eval KDE function kde!(points::AbstractArray{<:Real,2}, ks::Array{Float64,1}, weights::Array{Float64,1},
                                                 addop=(+,), diffop=(-,))
    # (unit weights only -- what kde!(points, ks) passes: there `weights ./ sum(weights)` is exact in any summation order)
    if $(builds_here)(points, ks, addop, diffop) && length(weights) == size(points, 2) && all(isone, weights)
      return $(kde!)(points, ks, nothing)
    end
    return $(reference_kde_bww)(points, ks, weights, addop, diffop)
  end
  # evaluateDualTree(bd, pos::Matrix) / bd(pos) / evaluateDualTree(bd, pos::BallTreeDensity): direct evaluation on the GPU
  # while the reference's own default FORCE_EVAL_DIRECT = true stands and the operators are Euclidean
  eval_m === nothing || @eval KDE function evaluateDualTree(bd::BallTreeDensity, pos::Array{Float64,2}, lvFlag::Bool=false, errTol::Float64=1e-3,
                                      addop=(+,), diffop=(-,))
    if $(isEuclidOps)(addop, diffop) && $(directEval)() && bd.bt.dims <= 8 && bd.multibandwidth == 0
      return $(evaluateDualTree)(bd, pos, lvFlag)
    end
    return $(reference_evaluateDualTree)(bd, pos, lvFlag, errTol, addop, diffop)
  end
  eval_b === nothing || @eval KDE function evaluateDualTree(bd::BallTreeDensity, pos::BallTreeDensity, lvFlag::Bool=false, errTol::Float64=1e-3,
                                      addop=(+,), diffop=(-,))
    if $(isEuclidOps)(addop, diffop) && $(directEval)() && bd.bt.dims <= 8 && bd.multibandwidth == 0
      bd.bt.dims == pos.bt.dims || error("bd and pos must have the same dimension")
      return $(evaluateDualTree)(bd, getPoints(pos), lvFlag)
    end
    return $(reference_evaluateDualTree_bd)(bd, pos, lvFlag, errTol, addop, diffop)
  end
  nothing
end

"""
    overridden_methods()

What `enable!(kde=true, trees=true, evaluate=true)` replaces in `KernelDensityEstimate` (pinned by
tests/test_julia_shim_syntax.py; plain `enable!()` replaces the first two): with all of them, an unchanged caller of `*`
runs product, bandwidth search, tree construction and evaluation in libkdehip.so.
"""
overridden_methods() = ["gibbs1", "prodAppxMSGibbsS", "kde!(points)", "kde!(points, ks)", "kde!(points, ks, weights)",
                        "evaluateDualTree(bd, pos::Array{Float64,2})", "evaluateDualTree(bd, pos::BallTreeDensity)"]

end # module
