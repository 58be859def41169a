# CompressedSensingAMD.jl -- Julia host for libcsmp.so (MI355X / gfx950).
#
# Keeps CompressedSensing.jl's matching-pursuit API surface -- mp / omp / gomp / sp with the same
# positional and keyword forms, the MP / OMP / GOMP update functors -- and forwards the work through
# `ccall` to the C ABI declared in include/csmp.h.  Results are `SparseVector{Float64,Int}` with
# sorted 1-based `nzind`, exactly what the reference returns (src/matchingpursuit.jl:76).
#
# NOTE: the build container has no `julia`, so this file has never been executed; it is the
# reference-side binding a maintainer adds (see INTEGRATION.md).  The same ABI is exercised by the
# Python/ctypes mirror (compressedsensing.jl_amd/_lib.py, api.py), which the test suite drives.
module CompressedSensingAMD

using LinearAlgebra
using SparseArrays
using Random

const libcsmp = get(ENV, "LIBCSMP", joinpath(@__DIR__, "..", "csrc", "libcsmp.so"))

const CSMP_F32, CSMP_F64 = Cint(0), Cint(1)
const CSMP_HOST, CSMP_DEVICE, CSMP_HOST_STREAMED = Cint(0), Cint(1), Cint(2)
const ALGO_MP, ALGO_OMP, ALGO_GOMP, ALGO_FR, ALGO_SP, ALGO_OMPR = Cint(0), Cint(1), Cint(2), Cint(3), Cint(4), Cint(5)

dtype_code(::Type{Float32}) = CSMP_F32
dtype_code(::Type{Float64}) = CSMP_F64

# ---------------------------------------------------------------------------------- context
"""
    Dictionary(A; device = 0, streamed = false)
    Dictionary(path::AbstractString; device = 0, streamed = false)

The measurement matrix resident in HBM (uploaded once).  Stands in for the `A` field of the
reference's MP / OMP / GOMP / SP structs.  `streamed = true` leaves it in host memory, mapped into the
device: every sweep reads it over the host link -- for a dictionary larger than HBM (the array is kept
alive by the object and must not be changed).  `path`: a dictionary file (`write_dictionary_file`).
"""
mutable struct Dictionary{T<:Union{Float32,Float64}}
    ctx::Ptr{Cvoid}
    n::Int   # rows  (reference: n, m = size(A), src/matchingpursuit.jl:20)
    m::Int   # atoms
    keep::Any  # a streamed array, held for the context's lifetime
    function Dictionary{T}(n::Integer, m::Integer, device::Integer) where {T<:Union{Float32,Float64}}
        ref = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:csmp_create, libcsmp), Cint, (Ref{Ptr{Cvoid}}, Cint), ref, device)
        rc == 0 || throw(unsafe_string(ccall((:csmp_last_error, libcsmp), Cstring, (Ptr{Cvoid},), C_NULL)))
        D = new{T}(ref[], n, m, nothing)
        finalizer(d -> ccall((:csmp_destroy, libcsmp), Cint, (Ptr{Cvoid},), d.ctx), D)
        return D
    end
end
function Dictionary(A::StridedMatrix{T}; device::Integer = 0, streamed::Bool = false) where {T<:Union{Float32,Float64}}
    D = Dictionary{T}(size(A, 1), size(A, 2), device)
    GC.@preserve A check(D, ccall((:csmp_set_dictionary, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Cint),
        D.ctx, pointer(A), size(A, 1), size(A, 2), stride(A, 2), dtype_code(T), streamed ? CSMP_HOST_STREAMED : CSMP_HOST))
    streamed && (D.keep = A)
    return D
end
function Dictionary(path::AbstractString; device::Integer = 0, streamed::Bool = false)
    n, m, dt = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0)
    rc = ccall((:csmp_dictionary_file_info, libcsmp), Cint, (Cstring, Ref{Int64}, Ref{Int64}, Ref{Cint}), path, n, m, dt)
    rc == 0 || throw("$path is not a dictionary file")
    D = Dictionary{dt[] == CSMP_F32 ? Float32 : Float64}(n[], m[], device)
    check(D, ccall((:csmp_set_dictionary_file, libcsmp), Cint, (Ptr{Cvoid}, Cstring, Cint), D.ctx, path, streamed ? CSMP_HOST_STREAMED : CSMP_DEVICE))
    return D
end

"""
    write_dictionary_file(path, A)

`A` as a dictionary file (include/csmp.h: a 64-byte header and the columns, padded to 16 bytes); host only.
"""
function write_dictionary_file(path::AbstractString, A::StridedMatrix{T}) where {T<:Union{Float32,Float64}}
    rc = GC.@preserve A ccall((:csmp_dictionary_file_write, libcsmp), Cint, (Cstring, Ptr{Cvoid}, Int64, Int64, Int64, Cint),
        path, pointer(A), size(A, 1), size(A, 2), stride(A, 2), dtype_code(T))
    rc == 0 || throw("cannot write $path")
    return path
end
Base.size(D::Dictionary) = (D.n, D.m)
Base.size(D::Dictionary, i::Int) = size(D)[i]
Base.eltype(::Dictionary{T}) where {T} = T

# the reference throws bare strings (src/matchingpursuit.jl:74; src/twostage.jl:76): so do we
function check(D::Dictionary, rc::Integer)
    rc == 0 && return
    throw(unsafe_string(ccall((:csmp_last_error, libcsmp), Cstring, (Ptr{Cvoid},), D.ctx)))
end

# ---------------------------------------------------------------------------------- options (include/csmp.h, CSMP_OPT_*)
# The reference passes its behavioural choices as arguments and so does this module; the choices that exist only on the GPU
# side are per-Dictionary options.  The library reads no environment variable.
const OPTIONS = Dict(:batch_cert => 1, :batch_gram => 2, :batch_window => 3, :pipeline => 4, :solves_in_flight => 9, :screened_sweep => 10,
                     :batch_screen => 11)
set_option!(D::Dictionary, key::Symbol, value::Integer) =
    check(D, ccall((:csmp_set_option, libcsmp), Cint, (Ptr{Cvoid}, Cint, Int64), D.ctx, OPTIONS[key], value))
function get_option(D::Dictionary, key::Symbol)
    v = Ref{Int64}(0)
    check(D, ccall((:csmp_get_option, libcsmp), Cint, (Ptr{Cvoid}, Cint, Ref{Int64}), D.ctx, OPTIONS[key], v))
    v[]
end

const MatOrDict{T} = Union{StridedMatrix{T}, Dictionary{T}}
dict(A::Dictionary) = A
dict(A::StridedMatrix) = Dictionary(A)

function to_sparse(m::Int, idx::Vector{Int64}, val::Vector{Float64}, nnz::Integer)
    # 0-based sorted indices from the ABI -> SparseVector{Float64,Int} (src/matchingpursuit.jl:76)
    SparseVector(m, idx[1:nnz] .+ 1, val[1:nnz])
end

bvec(b::AbstractVector{Float32}) = (convert(Vector{Float32}, b), CSMP_F32)
bvec(b::AbstractVector) = (convert(Vector{Float64}, b), CSMP_F64)

# ---------------------------------------------------------------------------------- omp
# src/matchingpursuit.jl:73-91
function omp(A::MatOrDict{T}, b::AbstractVector, ε::Real, k::Int = size(A, 1)) where {T}
    ε ≥ 0 || throw("ε = $ε has to be non-negative")
    D = dict(A)
    bb, bt = bvec(b)
    idx, val, nnz = zeros(Int64, max(k, 1)), zeros(Float64, max(k, 1)), Ref{Int64}(0)
    GC.@preserve bb idx val check(D, ccall((:csmp_omp, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Cdouble, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}, Ptr{Int64}),
        D.ctx, bb, bt, k, ε, idx, val, nnz, C_NULL))
    to_sparse(size(D, 2), idx, val, nnz[])
end
omp(A::MatOrDict{T}, b::AbstractVector, k::Int) where {T} = omp(A, b, eps(T), k)
omp(A::MatOrDict{T}, b::AbstractVector; max_residual = eps(T), sparsity = min(size(A)...)) where {T} =
    omp(A, b, max_residual, sparsity)

# ---------------------------------------------------------------------------------- gomp
# src/matchingpursuit.jl:126-148
function gomp(A::MatOrDict{T}, b::AbstractVector, l::Int, ε::Real, k::Int = size(A, 1)) where {T}
    ε ≥ 0 || throw("ε = $ε has to be non-negative")
    D = dict(A)
    bb, bt = bvec(b)
    cap = max(k + l, 1)
    idx, val, nnz = zeros(Int64, cap), zeros(Float64, cap), Ref{Int64}(0)
    GC.@preserve bb idx val check(D, ccall((:csmp_gomp, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Cdouble, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}, Ptr{Int64}),
        D.ctx, bb, bt, l, k, ε, idx, val, nnz, C_NULL))
    to_sparse(size(D, 2), idx, val, nnz[])
end
gomp(A::MatOrDict{T}, b::AbstractVector, l::Int, k::Int) where {T} = gomp(A, b, l, eps(T), k)
gomp(A::MatOrDict{T}, b::AbstractVector, l::Int; max_residual = eps(T), sparsity = size(A, 2)) where {T} =
    gomp(A, b, l, max_residual, sparsity)

# ---------------------------------------------------------------------------------- mp
# src/matchingpursuit.jl:34-40 (x is a warm start and is updated in place)
function mp(A::MatOrDict{T}, b::AbstractVector, k::Int, x::SparseVector = spzeros(size(A, 2))) where {T}
    D = dict(A)
    bb, bt = bvec(b)
    idx0, val0 = convert(Vector{Int64}, x.nzind .- 1), convert(Vector{Float64}, x.nzval)
    cap = max(k + length(idx0), 1)
    idx, val, nnz = zeros(Int64, cap), zeros(Float64, cap), Ref{Int64}(0)
    GC.@preserve bb idx0 val0 idx val check(D, ccall((:csmp_mp, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Ptr{Int64}, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}),
        D.ctx, bb, bt, k, idx0, val0, length(idx0), idx, val, nnz))
    y = to_sparse(size(D, 2), idx, val, nnz[])
    resize!(x.nzind, nnz[]); resize!(x.nzval, nnz[])
    copyto!(x.nzind, y.nzind); copyto!(x.nzval, y.nzval)
    return x
end

# ---------------------------------------------------------------------------------- ista / fista
# src/basispursuit.jl:144,164-204: x <- shrinkage(x + 2α A'(b - A x), wα) on ‖b - A x‖² + Σ w_j |x_j|, exactly maxiter times.
# fista is the Beck-Teboulle acceleration of the same iteration (the reference's own, :186-204, does not run).
shrinkage(x::Real, α::Real) = sign(x) * max(abs(x) - α, zero(x))
function ista_call(A::MatOrDict, b::AbstractVector, w::Vector{Float64}, x::AbstractVector, maxiter::Int, stepsize::Real, accel::Bool)
    D = dict(A)
    bb, bt = bvec(b)
    x0 = sparse(x)
    idx0, val0 = convert(Vector{Int64}, x0.nzind .- 1), convert(Vector{Float64}, x0.nzval)
    xd, rn = zeros(Float64, size(D, 2)), Ref{Cdouble}(0)
    GC.@preserve bb w idx0 val0 xd check(D, ccall((:csmp_ista, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{Cdouble}, Int64, Int64, Cdouble, Cint, Ptr{Cdouble}, Cint, Ref{Cdouble}),
        D.ctx, bb, bt, w, length(w), idx0, val0, length(idx0), maxiter, stepsize, Cint(accel), xd, CSMP_HOST, rn))
    return sparse(xd)  # (exact zeros are structural zeros: dropzeros!, :180)
end
ista(A::MatOrDict, b::AbstractVector, w::AbstractVector, x::AbstractVector = spzeros(size(A, 2)); maxiter::Int = 1024, stepsize::Real = 1e-2) =
    ista_call(A, b, convert(Vector{Float64}, w), x, maxiter, stepsize, false)
ista(A::MatOrDict, b::AbstractVector, λ::Real, x::AbstractVector = spzeros(size(A, 2)); maxiter::Int = 1024, stepsize::Real = 1e-2) =
    ista_call(A, b, Float64[λ], x, maxiter, stepsize, false)
fista(A::MatOrDict, b::AbstractVector, w::AbstractVector, x::AbstractVector = spzeros(size(A, 2)); maxiter::Int = 1024, stepsize::Real = 1e-2) =
    ista_call(A, b, convert(Vector{Float64}, w), x, maxiter, stepsize, true)
fista(A::MatOrDict, b::AbstractVector, λ::Real, x::AbstractVector = spzeros(size(A, 2)); maxiter::Int = 1024, stepsize::Real = 1e-2) =
    ista_call(A, b, Float64[λ], x, maxiter, stepsize, true)

# [ista(A, B[:, s], w_s, x0_s) for s in axes(B, 2)]: up to eight signals take their iterations together on shared launches, every result
# ista's bit for bit (csmp_ista_batch).  The weights: a λ or an N-vector shared by all signals, an nsig-vector of λs (one per signal; when
# nsig == N a vector is the shared N-vector) or an N x nsig matrix (a weight vector per signal).  X0: the dense warm starts, N x nsig.
function ista_batch_call(A::MatOrDict, B::AbstractMatrix, w::Array{Float64}, ldw::Int, X0::Union{Nothing,AbstractMatrix}, maxiter::Int,
                         stepsize::Real, accel::Bool)
    D = dict(A)
    BB = B isa StridedMatrix && eltype(B) <: Union{Float32,Float64} && stride(B, 1) == 1 ? B : convert(Matrix{Float64}, B)
    size(BB, 1) == size(D, 1) || throw(DimensionMismatch("size(B, 1) = $(size(BB, 1)) but size(A, 1) = $(size(D, 1))"))
    nsig, N = size(BB, 2), size(D, 2)
    X = zeros(Float64, N, nsig)
    if X0 !== nothing
        size(X0) == (N, nsig) || throw(DimensionMismatch("size(X0) = $(size(X0)) but the warm starts are $N x $nsig"))
        copyto!(X, X0)  # (continued in place: X0 == X)
    end
    rn = zeros(Float64, nsig)
    nw = ldw == 0 ? length(w) : size(w, 1)
    GC.@preserve BB w X rn check(D, ccall((:csmp_ista_batch, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Cint, Ptr{Cdouble}, Int64, Int64, Ptr{Cdouble}, Int64, Int64, Cdouble, Cint, Ptr{Cdouble}, Int64,
         Cint, Ptr{Cdouble}),
        D.ctx, BB, dtype_code(eltype(BB)), max(stride(BB, 2), size(BB, 1)), nsig, CSMP_HOST, w, nw, ldw, X0 === nothing ? C_NULL : pointer(X), max(N, 1),
        maxiter, stepsize, Cint(accel), X, max(N, 1), CSMP_HOST, rn))
    return [sparse(X[:, s]) for s in 1:nsig]
end
function ista_batch_weights(A::MatOrDict, B::AbstractMatrix, w::AbstractVector)
    N, nsig = size(A, 2), size(B, 2)
    length(w) == N && return convert(Vector{Float64}, w), 0
    length(w) == nsig && return reshape(convert(Vector{Float64}, w), 1, nsig), 1
    throw(DimensionMismatch("length(w) = $(length(w)) is neither size(A, 2) = $N nor size(B, 2) = $nsig"))
end
function ista_batch_weights(A::MatOrDict, B::AbstractMatrix, W::AbstractMatrix)
    size(W) == (size(A, 2), size(B, 2)) || throw(DimensionMismatch("size(W) = $(size(W)) but size(A, 2) x size(B, 2) = $((size(A, 2), size(B, 2)))"))
    return convert(Matrix{Float64}, W), max(size(W, 1), 1)
end
ista_batch_weights(A::MatOrDict, B::AbstractMatrix, λ::Real) = (Float64[λ], 0)
ista_batch(A::MatOrDict, B::AbstractMatrix, w::Union{Real,AbstractVecOrMat}, X0::Union{Nothing,AbstractMatrix} = nothing; maxiter::Int = 1024,
           stepsize::Real = 1e-2) = ista_batch_call(A, B, ista_batch_weights(A, B, w)..., X0, maxiter, stepsize, false)
fista_batch(A::MatOrDict, B::AbstractMatrix, w::Union{Real,AbstractVecOrMat}, X0::Union{Nothing,AbstractMatrix} = nothing; maxiter::Int = 1024,
            stepsize::Real = 1e-2) = ista_batch_call(A, B, ista_batch_weights(A, B, w)..., X0, maxiter, stepsize, true)

# ista / fista for columns of B that share ONE support: the row-sparse (l2,1) objective ‖B - A X‖_F² + Σ_j w_j ‖X[j, :]‖₂, the convex
# counterpart of somp (csmp_ista_joint).  The weights: a λ, or one weight per ROW of X.  X0: the dense warm start, N x nsig.  Returns
# SparseVectors that all carry the same nzind (the non-zero rows); return_info: (xs, (rows, resnorm)).
function ista_joint_call(A::MatOrDict, B::AbstractMatrix, w::Vector{Float64}, X0::Union{Nothing,AbstractMatrix}, maxiter::Int, stepsize::Real,
                         accel::Bool, return_info::Bool)
    D = dict(A)
    BB = B isa StridedMatrix && eltype(B) <: Union{Float32,Float64} && stride(B, 1) == 1 ? B : convert(Matrix{Float64}, B)
    size(BB, 1) == size(D, 1) || throw(DimensionMismatch("size(B, 1) = $(size(BB, 1)) but size(A, 1) = $(size(D, 1))"))
    nsig, N = size(BB, 2), size(D, 2)
    length(w) in (1, N) || throw(DimensionMismatch("length(w) = $(length(w)) but size(A, 2) = $N"))
    X = zeros(Float64, N, nsig)
    if X0 !== nothing
        size(X0) == (N, nsig) || throw(DimensionMismatch("size(X0) = $(size(X0)) but the warm start is $N x $nsig"))
        copyto!(X, X0)  # (continued in place: X0 == X)
    end
    rn, rows = zeros(Float64, max(nsig, 1)), Ref{Int64}(0)
    GC.@preserve BB w X rn check(D, ccall((:csmp_ista_joint, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Cint, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64, Int64, Cdouble, Cint, Ptr{Cdouble}, Int64,
         Cint, Ref{Int64}, Ptr{Cdouble}),
        D.ctx, BB, dtype_code(eltype(BB)), max(stride(BB, 2), size(BB, 1)), nsig, CSMP_HOST, w, length(w), X0 === nothing ? C_NULL : pointer(X),
        max(N, 1), maxiter, stepsize, Cint(accel), X, max(N, 1), CSMP_HOST, rows, rn))
    nz = findall(j -> any(!iszero, view(X, j, :)), 1:N)
    xs = [SparseVector(N, nz, X[nz, s]) for s in 1:nsig]
    return return_info ? (xs, (rows = Int(rows[]), resnorm = rn[1:nsig])) : xs
end
ista_joint(A::MatOrDict, B::AbstractMatrix, w::Union{Real,AbstractVector}, X0::Union{Nothing,AbstractMatrix} = nothing; maxiter::Int = 1024,
           stepsize::Real = 1e-2, return_info::Bool = false) =
    ista_joint_call(A, B, w isa Real ? Float64[w] : convert(Vector{Float64}, w), X0, maxiter, stepsize, false, return_info)
fista_joint(A::MatOrDict, B::AbstractMatrix, w::Union{Real,AbstractVector}, X0::Union{Nothing,AbstractMatrix} = nothing; maxiter::Int = 1024,
            stepsize::Real = 1e-2, return_info::Bool = false) =
    ista_joint_call(A, B, w isa Real ? Float64[w] : convert(Vector{Float64}, w), X0, maxiter, stepsize, true, return_info)

# ---------------------------------------------------------------------------------- reweighted l1
# src/basispursuit.jl:18-74: candes_weights!, ard_weights! and basispursuit_reweighting with ista / fista as the solver of
# ‖b - A x‖² + λ Σ w_j |x_j| (the loops around bp and bpd themselves: bp_candes / bp_ard and bpd_candes / bpd_ard below).
const CSMP_ARD_KMAX = 1024
const CSMP_REWEIGHT_CANDES = 0
const CSMP_REWEIGHT_ARD = 1
candes_weight(x, ε) = inv(abs(x) + ε)
function candes_weights!(w::AbstractVector, x::AbstractVector, ε::Real)
    ε > 0 || throw("ε = $ε has to be positive")
    @. w = candes_weight(x, ε)
    if any(isnan, w) || any(isinf, w)
        throw("weights contain NaN or Inf: $w")
    end
    return w
end
function ard_weights!(w::Vector{Float64}, A::MatOrDict, x::AbstractVector, ε::Real, iter::Int = 8)
    any(==(0), w) && error("weights cannot be zero")
    D = dict(A)
    xd = convert(Vector{Float64}, Vector(x))
    GC.@preserve xd w check(D, ccall((:csmp_ard_weights, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Int64, Ptr{Cdouble}, Cint),
        D.ctx, xd, w, ε, iter, w, CSMP_HOST))
    return w
end
function ista_reweighted(A::MatOrDict, b::AbstractVector, λ::Real, scheme::Integer, ε::Real, ard_iter::Int, maxiter::Int, min_decrease::Real,
                         inner_maxiter::Int, stepsize::Real, accel::Bool, return_weights::Bool)
    D = dict(A)
    bb, bt = bvec(b)
    xd, w = zeros(Float64, size(D, 2)), zeros(Float64, size(D, 2))
    done, rn = Ref{Int64}(0), Ref{Cdouble}(0)
    GC.@preserve bb xd w check(D, ccall((:csmp_ista_reweighted, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Cint, Cdouble, Int64, Int64, Cdouble, Int64, Cdouble, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble},
         Ref{Int64}, Ref{Cdouble}),
        D.ctx, bb, bt, λ, Cint(scheme), ε, ard_iter, maxiter, min_decrease, inner_maxiter, stepsize, Cint(accel), xd, CSMP_HOST, w, done, rn))
    return return_weights ? (sparse(xd), w) : sparse(xd)
end
ista_candes(A::MatOrDict, b::AbstractVector, λ::Real, ε::Real = 1e-2; maxiter::Int = 8, min_decrease::Real = 1e-8, inner_maxiter::Int = 1024,
            stepsize::Real = 1e-2, accel::Bool = false, return_weights::Bool = false) =
    ista_reweighted(A, b, λ, CSMP_REWEIGHT_CANDES, ε, 8, maxiter, min_decrease, inner_maxiter, stepsize, accel, return_weights)
ista_ard(A::MatOrDict, b::AbstractVector, λ::Real, ε::Real = 1e-2; maxiter::Int = 8, min_decrease::Real = 1e-8, inner_maxiter::Int = 1024,
         stepsize::Real = 1e-2, accel::Bool = false, return_weights::Bool = false, iter::Int = 8) =
    ista_reweighted(A, b, λ, CSMP_REWEIGHT_ARD, ε, iter, maxiter, min_decrease, inner_maxiter, stepsize, accel, return_weights)

# ---------------------------------------------------------------------------------- basis pursuit
# src/basispursuit.jl:1-74: bp(A, b[, w]) = basispursuit -- min Σ w_j |x_j| subject to A x = b, by ADMM with one Cholesky factorisation of
# A Aᵀ per Dictionary (csmp_bp, include/csmp.h) -- and bp_candes / bp_ard, basispursuit_reweighting around it (csmp_bp_reweighted).
const CSMP_BP_CONVERGED = 1
const CSMP_BP_FACTORED = 2
function bp_call(A::MatOrDict, b::AbstractVector, w::Vector{Float64}, rho::Real, maxiter::Int, tol::Real, check_every::Int, return_info::Bool)
    D = dict(A)
    bb, bt = bvec(b)
    xd = zeros(Float64, size(D, 2))
    it, rn, flags = Ref{Int64}(0), Ref{Cdouble}(0), Ref{Cint}(0)
    GC.@preserve bb w xd check(D, ccall((:csmp_bp, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cdouble}, Int64, Cdouble, Int64, Cdouble, Int64, Ptr{Cdouble}, Cint, Ref{Int64}, Ref{Cdouble}, Ref{Cint}),
        D.ctx, bb, bt, w, length(w), rho, maxiter, tol, check_every, xd, CSMP_HOST, it, rn, flags))
    info = (iterations = Int(it[]), converged = flags[] & CSMP_BP_CONVERGED != 0, factored = flags[] & CSMP_BP_FACTORED != 0, resnorm = rn[])
    return return_info ? (sparse(xd), info) : sparse(xd)
end
bp(A::MatOrDict, b::AbstractVector; rho::Real = 1.0, maxiter::Int = 16384, tol::Real = 1e-8, check_every::Int = 32, return_info::Bool = false) =
    bp_call(A, b, Float64[1.0], rho, maxiter, tol, check_every, return_info)
bp(A::MatOrDict, b::AbstractVector, w::AbstractVector; rho::Real = 1.0, maxiter::Int = 16384, tol::Real = 1e-8, check_every::Int = 32,
   return_info::Bool = false) = bp_call(A, b, convert(Vector{Float64}, w), rho, maxiter, tol, check_every, return_info)
const basispursuit = bp
# [bp(A, B[:, s], w) for s in axes(B, 2)]: up to eight signals take their iterations in lockstep on shared launches, every result bp's bit
# for bit (csmp_bp_batch).  The weights are shared by all signals.
function bp_batch_call(A::MatOrDict, B::AbstractMatrix, w::Vector{Float64}, rho::Real, maxiter::Int, tol::Real, check_every::Int, return_info::Bool)
    D = dict(A)
    BB = B isa StridedMatrix && eltype(B) <: Union{Float32,Float64} && stride(B, 1) == 1 ? B : convert(Matrix{Float64}, B)
    size(BB, 1) == size(D, 1) || throw(DimensionMismatch("size(B, 1) = $(size(BB, 1)) but size(A, 1) = $(size(D, 1))"))
    nsig, N = size(BB, 2), size(D, 2)
    X = zeros(Float64, N, nsig)
    it, rn, flags = zeros(Int64, nsig), zeros(Float64, nsig), zeros(Cint, nsig)
    GC.@preserve BB w X it rn flags check(D, ccall((:csmp_bp_batch, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Cint, Ptr{Cdouble}, Int64, Cdouble, Int64, Cdouble, Int64, Ptr{Cdouble}, Int64, Cint,
         Ptr{Int64}, Ptr{Cdouble}, Ptr{Cint}),
        D.ctx, BB, dtype_code(eltype(BB)), max(stride(BB, 2), size(BB, 1)), nsig, CSMP_HOST, w, length(w), rho, maxiter, tol, check_every, X, max(N, 1),
        CSMP_HOST, it, rn, flags))
    xs = [sparse(X[:, s]) for s in 1:nsig]
    info = (iterations = it, converged = flags .& CSMP_BP_CONVERGED .!= 0, resnorm = rn, factored = nsig > 0 && flags[1] & CSMP_BP_FACTORED != 0)
    return return_info ? (xs, info) : xs
end
bp_batch(A::MatOrDict, B::AbstractMatrix; rho::Real = 1.0, maxiter::Int = 16384, tol::Real = 1e-8, check_every::Int = 32, return_info::Bool = false) =
    bp_batch_call(A, B, Float64[1.0], rho, maxiter, tol, check_every, return_info)
bp_batch(A::MatOrDict, B::AbstractMatrix, w::AbstractVector; rho::Real = 1.0, maxiter::Int = 16384, tol::Real = 1e-8, check_every::Int = 32,
         return_info::Bool = false) = bp_batch_call(A, B, convert(Vector{Float64}, w), rho, maxiter, tol, check_every, return_info)
# bp for columns of B that share ONE support: min Σ_j w_j ‖X[j, :]‖₂ subject to A X = B, the row-sparse (l2,1) programme with ONE
# stopping rule for all columns (csmp_bp_joint); one column is bp.  The weights: one per ROW of X.  Returns SparseVectors that all carry
# the same nzind (the non-zero rows); return_info: (xs, (iterations, converged, factored, rows, resnorm)).
function bp_joint_call(A::MatOrDict, B::AbstractMatrix, w::Vector{Float64}, rho::Real, maxiter::Int, tol::Real, check_every::Int, return_info::Bool)
    D = dict(A)
    BB = B isa StridedMatrix && eltype(B) <: Union{Float32,Float64} && stride(B, 1) == 1 ? B : convert(Matrix{Float64}, B)
    size(BB, 1) == size(D, 1) || throw(DimensionMismatch("size(B, 1) = $(size(BB, 1)) but size(A, 1) = $(size(D, 1))"))
    nsig, N = size(BB, 2), size(D, 2)
    length(w) in (1, N) || throw(DimensionMismatch("length(w) = $(length(w)) but size(A, 2) = $N"))
    X = zeros(Float64, N, nsig)
    rn, it, rows, flags = zeros(Float64, max(nsig, 1)), Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0)
    GC.@preserve BB w X rn check(D, ccall((:csmp_bp_joint, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Cint, Ptr{Cdouble}, Int64, Cdouble, Int64, Cdouble, Int64, Ptr{Cdouble}, Int64, Cint,
         Ref{Int64}, Ref{Int64}, Ptr{Cdouble}, Ref{Cint}),
        D.ctx, BB, dtype_code(eltype(BB)), max(stride(BB, 2), size(BB, 1)), nsig, CSMP_HOST, w, length(w), rho, maxiter, tol, check_every, X, max(N, 1),
        CSMP_HOST, it, rows, rn, flags))
    nz = findall(j -> any(!iszero, view(X, j, :)), 1:N)
    xs = [SparseVector(N, nz, X[nz, s]) for s in 1:nsig]
    info = (iterations = Int(it[]), converged = flags[] & CSMP_BP_CONVERGED != 0, factored = flags[] & CSMP_BP_FACTORED != 0, rows = Int(rows[]),
            resnorm = rn[1:nsig])
    return return_info ? (xs, info) : xs
end
bp_joint(A::MatOrDict, B::AbstractMatrix; rho::Real = 1.0, maxiter::Int = 16384, tol::Real = 1e-8, check_every::Int = 32, return_info::Bool = false) =
    bp_joint_call(A, B, Float64[1.0], rho, maxiter, tol, check_every, return_info)
bp_joint(A::MatOrDict, B::AbstractMatrix, w::Union{Real,AbstractVector}; rho::Real = 1.0, maxiter::Int = 16384, tol::Real = 1e-8,
         check_every::Int = 32, return_info::Bool = false) =
    bp_joint_call(A, B, w isa Real ? Float64[w] : convert(Vector{Float64}, w), rho, maxiter, tol, check_every, return_info)
function bp_reweighted(A::MatOrDict, b::AbstractVector, scheme::Integer, ε::Real, ard_iter::Int, maxiter::Int, min_decrease::Real, rho::Real,
                       inner_maxiter::Int, tol::Real, check_every::Int, return_weights::Bool)
    D = dict(A)
    bb, bt = bvec(b)
    xd, w = zeros(Float64, size(D, 2)), zeros(Float64, size(D, 2))
    done, rn = Ref{Int64}(0), Ref{Cdouble}(0)
    GC.@preserve bb xd w check(D, ccall((:csmp_bp_reweighted, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cdouble, Int64, Int64, Cdouble, Cdouble, Int64, Cdouble, Int64, Ptr{Cdouble}, Cint, Ptr{Cdouble},
         Ref{Int64}, Ref{Cdouble}),
        D.ctx, bb, bt, Cint(scheme), ε, ard_iter, maxiter, min_decrease, rho, inner_maxiter, tol, check_every, xd, CSMP_HOST, w, done, rn))
    return return_weights ? (sparse(xd), w) : sparse(xd)
end
bp_candes(A::MatOrDict, b::AbstractVector, ε::Real = 1e-2; maxiter::Int = 8, min_decrease::Real = 1e-8, rho::Real = 1.0, inner_maxiter::Int = 16384,
          tol::Real = 1e-8, check_every::Int = 32, return_weights::Bool = false) =
    bp_reweighted(A, b, CSMP_REWEIGHT_CANDES, ε, 8, maxiter, min_decrease, rho, inner_maxiter, tol, check_every, return_weights)
bp_ard(A::MatOrDict, b::AbstractVector, ε::Real = 1e-2; maxiter::Int = 8, min_decrease::Real = 1e-8, iter::Int = 8, rho::Real = 1.0,
       inner_maxiter::Int = 16384, tol::Real = 1e-8, check_every::Int = 32, return_weights::Bool = false) =
    bp_reweighted(A, b, CSMP_REWEIGHT_ARD, ε, iter, maxiter, min_decrease, rho, inner_maxiter, tol, check_every, return_weights)

# ---------------------------------------------------------------------------------- basis pursuit denoising
# src/basispursuit.jl:76-124: bpd(A, b, δ[, w]) = basis_pursuit_denoising -- min Σ w_j |x_j| subject to ‖A x − b‖₂ ≤ δ, by graph-form ADMM
# with one Cholesky factorisation of I + A Aᵀ per Dictionary (csmp_bpd, include/csmp.h; no SOCP solver) -- and bpd_candes / bpd_ard,
# bpd_reweighting around it (csmp_bpd_reweighted).  rho = 100: DESIGN.md section 14.
const CSMP_BPD_CONVERGED = 1
const CSMP_BPD_FACTORED = 2
function bpd_call(A::MatOrDict, b::AbstractVector, δ::Real, w::Vector{Float64}, rho::Real, maxiter::Int, tol::Real, check_every::Int,
                  return_info::Bool)
    D = dict(A)
    bb, bt = bvec(b)
    xd = zeros(Float64, size(D, 2))
    it, rn, flags = Ref{Int64}(0), Ref{Cdouble}(0), Ref{Cint}(0)
    GC.@preserve bb w xd check(D, ccall((:csmp_bpd, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Ptr{Cdouble}, Int64, Cdouble, Int64, Cdouble, Int64, Ptr{Cdouble}, Cint, Ref{Int64}, Ref{Cdouble}, Ref{Cint}),
        D.ctx, bb, bt, δ, w, length(w), rho, maxiter, tol, check_every, xd, CSMP_HOST, it, rn, flags))
    info = (iterations = Int(it[]), converged = flags[] & CSMP_BPD_CONVERGED != 0, factored = flags[] & CSMP_BPD_FACTORED != 0, resnorm = rn[])
    return return_info ? (sparse(xd), info) : sparse(xd)
end
bpd(A::MatOrDict, b::AbstractVector, δ::Real; rho::Real = 100.0, maxiter::Int = 16384, tol::Real = 1e-8, check_every::Int = 32,
    return_info::Bool = false) = bpd_call(A, b, δ, Float64[1.0], rho, maxiter, tol, check_every, return_info)
bpd(A::MatOrDict, b::AbstractVector, δ::Real, w::AbstractVector; rho::Real = 100.0, maxiter::Int = 16384, tol::Real = 1e-8, check_every::Int = 32,
    return_info::Bool = false) = bpd_call(A, b, δ, convert(Vector{Float64}, w), rho, maxiter, tol, check_every, return_info)
const basis_pursuit_denoising = bpd
# [bpd(A, B[:, s], δ[s], w) for s in axes(B, 2)]: up to eight signals take their iterations in lockstep on shared launches, every result
# bpd's bit for bit (csmp_bpd_batch).  δ: one radius, or one per column of B.  The weights are shared by all signals.
function bpd_batch_call(A::MatOrDict, B::AbstractMatrix, δ::Union{Real,AbstractVector}, w::Vector{Float64}, rho::Real, maxiter::Int, tol::Real,
                        check_every::Int, return_info::Bool)
    D = dict(A)
    BB = B isa StridedMatrix && eltype(B) <: Union{Float32,Float64} && stride(B, 1) == 1 ? B : convert(Matrix{Float64}, B)
    size(BB, 1) == size(D, 1) || throw(DimensionMismatch("size(B, 1) = $(size(BB, 1)) but size(A, 1) = $(size(D, 1))"))
    nsig, N = size(BB, 2), size(D, 2)
    dd = δ isa Real ? Float64[δ] : convert(Vector{Float64}, δ)
    δ isa Real || length(dd) == nsig || throw(DimensionMismatch("length(δ) = $(length(dd)) but size(B, 2) = $nsig"))
    X = zeros(Float64, N, nsig)
    it, rn, flags = zeros(Int64, nsig), zeros(Float64, nsig), zeros(Cint, nsig)
    GC.@preserve BB dd w X it rn flags check(D, ccall((:csmp_bpd_batch, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Cint, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64, Cdouble, Int64, Cdouble, Int64, Ptr{Cdouble}, Int64,
         Cint, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cint}),
        D.ctx, BB, dtype_code(eltype(BB)), max(stride(BB, 2), size(BB, 1)), nsig, CSMP_HOST, dd, length(dd), w, length(w), rho, maxiter, tol, check_every,
        X, max(N, 1), CSMP_HOST, it, rn, flags))
    xs = [sparse(X[:, s]) for s in 1:nsig]
    info = (iterations = it, converged = flags .& CSMP_BPD_CONVERGED .!= 0, resnorm = rn, factored = nsig > 0 && flags[1] & CSMP_BPD_FACTORED != 0)
    return return_info ? (xs, info) : xs
end
bpd_batch(A::MatOrDict, B::AbstractMatrix, δ::Union{Real,AbstractVector}; rho::Real = 100.0, maxiter::Int = 16384, tol::Real = 1e-8,
          check_every::Int = 32, return_info::Bool = false) = bpd_batch_call(A, B, δ, Float64[1.0], rho, maxiter, tol, check_every, return_info)
bpd_batch(A::MatOrDict, B::AbstractMatrix, δ::Union{Real,AbstractVector}, w::AbstractVector; rho::Real = 100.0, maxiter::Int = 16384,
          tol::Real = 1e-8, check_every::Int = 32, return_info::Bool = false) =
    bpd_batch_call(A, B, δ, convert(Vector{Float64}, w), rho, maxiter, tol, check_every, return_info)
function bpd_reweighted(A::MatOrDict, b::AbstractVector, δ::Real, scheme::Integer, ε::Real, ard_iter::Int, maxiter::Int, min_decrease::Real,
                        rho::Real, inner_maxiter::Int, tol::Real, check_every::Int, return_weights::Bool)
    D = dict(A)
    bb, bt = bvec(b)
    xd, w = zeros(Float64, size(D, 2)), zeros(Float64, size(D, 2))
    done, rn = Ref{Int64}(0), Ref{Cdouble}(0)
    GC.@preserve bb xd w check(D, ccall((:csmp_bpd_reweighted, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Cint, Cdouble, Int64, Int64, Cdouble, Cdouble, Int64, Cdouble, Int64, Ptr{Cdouble}, Cint, Ptr{Cdouble},
         Ref{Int64}, Ref{Cdouble}),
        D.ctx, bb, bt, δ, Cint(scheme), ε, ard_iter, maxiter, min_decrease, rho, inner_maxiter, tol, check_every, xd, CSMP_HOST, w, done, rn))
    return return_weights ? (sparse(xd), w) : sparse(xd)
end
bpd_candes(A::MatOrDict, b::AbstractVector, δ::Real, ε::Real = δ; maxiter::Int = 8, min_decrease::Real = 1e-4, rho::Real = 100.0,
           inner_maxiter::Int = 16384, tol::Real = 1e-8, check_every::Int = 32, return_weights::Bool = false) =
    bpd_reweighted(A, b, δ, CSMP_REWEIGHT_CANDES, ε, 8, maxiter, min_decrease, rho, inner_maxiter, tol, check_every, return_weights)
bpd_ard(A::MatOrDict, b::AbstractVector, δ::Real, ε::Real = δ^2; maxiter::Int = 8, min_decrease::Real = 1e-4, iter::Int = 8, rho::Real = 100.0,
        inner_maxiter::Int = 16384, tol::Real = 1e-8, check_every::Int = 32, return_weights::Bool = false) =
    bpd_reweighted(A, b, δ, CSMP_REWEIGHT_ARD, ε, iter, maxiter, min_decrease, rho, inner_maxiter, tol, check_every, return_weights)

# ---------------------------------------------------------------------------------- sparse Bayesian learning
# src/sbl.jl:1-51: sbl(A, b, σ²) and SBL(A, b, σ²) with update! for a SCALAR noise variance, in the Woodbury form on the M × M matrix
# σ² I + A Γ Aᵀ (csmp_sbl, include/csmp.h).  A noise covariance matrix Σ is not served; fsbl and rmps follow below.
const CSMP_SBL_CONVERGED = 1
function sbl_call(D::Dictionary, b::AbstractVector, σ²::Real, γ::Vector{Float64}, maxiter::Int, min_change::Real)
    bb, bt = bvec(b)
    xd = zeros(Float64, size(D, 2))
    it, flags = Ref{Int64}(0), Ref{Cint}(0)
    GC.@preserve bb γ xd check(D, ccall((:csmp_sbl, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Int64, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ref{Int64}, Ref{Cint}),
        D.ctx, bb, bt, σ², maxiter, min_change, γ, xd, γ, CSMP_HOST, it, flags))
    return xd, (iterations = Int(it[]), converged = flags[] & CSMP_SBL_CONVERGED != 0, gamma = γ)
end
function sbl(A::MatOrDict, b::AbstractVector, σ²::Real; maxiter::Int = 128size(A, 2), min_change::Real = 1e-6, return_info::Bool = false)
    xd, info = sbl_call(dict(A), b, σ², ones(Float64, size(A, 2)), maxiter, min_change)
    return return_info ? (xd, info) : xd
end
sbl(A::MatOrDict, b::AbstractVector, Σ::AbstractMatrix; kwargs...) = error("sbl: a noise covariance matrix Σ is not served: scalar σ² only")
# SBL(A, b, σ²): the prior variances Γ.diag live in `gamma`, ones at the start; update!(S, x) is one csmp_sbl update (:26-35)
struct SparseBayesianLearning
    D::Dictionary
    b::Vector{Float64}
    σ²::Float64
    gamma::Vector{Float64}
end
const SBL = SparseBayesianLearning
SBL(A::MatOrDict, b::AbstractVector, σ²::Real) = SparseBayesianLearning(dict(A), convert(Vector{Float64}, b), Float64(σ²), ones(Float64, size(A, 2)))
SBL(A::MatOrDict, b::AbstractVector, Σ::AbstractMatrix) = error("SBL: a noise covariance matrix Σ is not served: scalar σ² only")
function update!(S::SparseBayesianLearning, x::AbstractVector = zeros(length(S.gamma)))
    xd, _ = sbl_call(S.D, S.b, S.σ², S.gamma, 1, 0.0)
    x .= xd
    return x
end
(S::SparseBayesianLearning)(x::AbstractVector = zeros(length(S.gamma))) = update!(S, x)

# ---------------------------------------------------------------------------------- greedy sparse Bayesian learning
# src/sbl.jl:57-437: fsbl(A, b, σ²) and rmps(A, b, σ²) for a SCALAR noise variance (csmp_fsbl, csmp_rmps, include/csmp.h): every step
# changes the prior precision α_i of one atom.  x is exactly zero off the active set.  alpha: prior precisions to start from (Inf =
# inactive).  return_info: (x, info) with the history of applied steps as (action, index) pairs, 1 add, 2 delete, 3 re-estimate, the
# index 1-based.  A covariance matrix and the σ²-optimising rmps(A, b, Val(true)) are refused.
const CSMP_FSBL_CONVERGED = 1
const CSMP_RMPS_CONVERGED = 1
greedy_info(it, flags, α, hist, n) = (iterations = Int(it[]), converged = flags[] & CSMP_FSBL_CONVERGED != 0, alpha = α,
                                      history = [(Int(hist[1, t]), Int(hist[2, t]) + 1) for t in 1:n])
function fsbl(A::MatOrDict, b::AbstractVector, σ²::Real; maxiter::Int = 2size(A, 2), min_increase::Real = 1e-6,
              alpha::Union{Nothing, AbstractVector} = nothing, return_info::Bool = false)
    D = dict(A)
    bb, bt = bvec(b)
    xd = zeros(Float64, size(D, 2))
    α = alpha === nothing ? fill(Inf, size(D, 2)) : convert(Vector{Float64}, alpha)
    cap = max(maxiter, 1)
    hist = zeros(Int64, 2, cap)
    it, flags = Ref{Int64}(0), Ref{Cint}(0)
    GC.@preserve bb α xd hist check(D, ccall((:csmp_fsbl, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Int64, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Int64}, Int64, Ref{Int64}, Ref{Cint}),
        D.ctx, bb, bt, σ², maxiter, min_increase, α, xd, α, CSMP_HOST, hist, cap, it, flags))
    x = sparse(xd)
    return return_info ? (x, greedy_info(it, flags, α, hist, count(!iszero, view(hist, 1, :)))) : x
end
function rmps(A::MatOrDict, b::AbstractVector, σ²::Real; maxiter::Int = size(A, 1), maxiter_acquisition::Int = size(A, 1),
              maxiter_deletion::Int = size(A, 1), min_increase::Real = 1e-6, alpha::Union{Nothing, AbstractVector} = nothing,
              return_info::Bool = false, history_cap::Int = 4size(A, 2))
    D = dict(A)
    bb, bt = bvec(b)
    xd = zeros(Float64, size(D, 2))
    α = alpha === nothing ? fill(Inf, size(D, 2)) : convert(Vector{Float64}, alpha)
    hist = zeros(Int64, 2, max(history_cap, 1))
    it, flags = Ref{Int64}(0), Ref{Cint}(0)
    GC.@preserve bb α xd hist check(D, ccall((:csmp_rmps, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Int64, Int64, Int64, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Int64}, Int64,
         Ref{Int64}, Ref{Cint}),
        D.ctx, bb, bt, σ², maxiter, maxiter_acquisition, maxiter_deletion, min_increase, α, xd, α, CSMP_HOST, hist, max(history_cap, 0), it, flags))
    x = sparse(xd)
    return return_info ? (x, greedy_info(it, flags, α, hist, min(Int(it[]), max(history_cap, 0)))) : x
end
fsbl(A::MatOrDict, b::AbstractVector, Σ::AbstractMatrix; kwargs...) = error("fsbl: only a scalar noise variance σ² is served, not a covariance matrix")
rmps(A::MatOrDict, b::AbstractVector, Σ::AbstractMatrix; kwargs...) = error("rmps: only a scalar noise variance σ² is served, not a covariance matrix")
rmps(A::MatOrDict, b::AbstractVector, ::Val{true}, args...; kwargs...) = error("rmps: the σ²-optimising form is not served: pass the noise variance σ²")

# [fsbl(A, B[:, s], σ²_s) for s in axes(B, 2)] and rmps likewise: up to eight signals take their greedy steps in lockstep, the product sweep
# of a step reads the dictionary once for all of them, every result the single call's bit for bit (csmp_fsbl_batch, csmp_rmps_batch).
# σ²: one noise variance, or one per signal.  alpha: the N x nsig prior precisions to start from.  return_info: (xs, infos), an info per signal.
function greedy_batch_setup(A::MatOrDict, B::AbstractMatrix, σ²::Union{Real,AbstractVector}, alpha::Union{Nothing,AbstractMatrix}, cap::Int)
    D = dict(A)
    BB = B isa StridedMatrix && eltype(B) <: Union{Float32,Float64} && stride(B, 1) == 1 ? B : convert(Matrix{Float64}, B)
    size(BB, 1) == size(D, 1) || throw(DimensionMismatch("size(B, 1) = $(size(BB, 1)) but size(A, 1) = $(size(D, 1))"))
    nsig, N = size(BB, 2), size(D, 2)
    s2 = σ² isa Real ? Float64[σ²] : convert(Vector{Float64}, σ²)
    length(s2) in (1, nsig) || throw(DimensionMismatch("length(σ²) = $(length(s2)) but B holds $nsig signals"))
    α = alpha === nothing ? fill(Inf, N, nsig) : convert(Matrix{Float64}, alpha)
    size(α) == (N, nsig) || throw(DimensionMismatch("size(alpha) = $(size(α)) but the warm starts are $N x $nsig"))
    return D, BB, s2, α, zeros(Float64, N, nsig), zeros(Int64, 2, max(cap, 1), max(nsig, 1)), zeros(Int64, nsig), zeros(Cint, nsig)
end
greedy_batch_info(it, flags, α, hist, s, n) = (iterations = Int(it[s]), converged = flags[s] & CSMP_FSBL_CONVERGED != 0, alpha = α[:, s],
                                               history = [(Int(hist[1, t, s]), Int(hist[2, t, s]) + 1) for t in 1:n])
function fsbl_batch(A::MatOrDict, B::AbstractMatrix, σ²::Union{Real,AbstractVector}; maxiter::Int = 2size(A, 2), min_increase::Real = 1e-6,
                    alpha::Union{Nothing,AbstractMatrix} = nothing, return_info::Bool = false)
    cap = max(maxiter, 1)
    D, BB, s2, α, X, hist, it, flags = greedy_batch_setup(A, B, σ², alpha, cap)
    nsig, N = size(BB, 2), size(D, 2)
    GC.@preserve BB s2 α X hist it flags check(D, ccall((:csmp_fsbl_batch, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Cint, Ptr{Cdouble}, Int64, Int64, Cdouble, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64,
         Ptr{Cdouble}, Int64, Cint, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Cint}),
        D.ctx, BB, dtype_code(eltype(BB)), max(stride(BB, 2), size(BB, 1)), nsig, CSMP_HOST, s2, length(s2), maxiter, min_increase, α, max(N, 1),
        X, max(N, 1), α, max(N, 1), CSMP_HOST, hist, cap, it, flags))
    xs = [sparse(X[:, s]) for s in 1:nsig]
    return return_info ? (xs, [greedy_batch_info(it, flags, α, hist, s, count(!iszero, view(hist, 1, :, s))) for s in 1:nsig]) : xs
end
function rmps_batch(A::MatOrDict, B::AbstractMatrix, σ²::Union{Real,AbstractVector}; maxiter::Int = size(A, 1),
                    maxiter_acquisition::Int = size(A, 1), maxiter_deletion::Int = size(A, 1), min_increase::Real = 1e-6,
                    alpha::Union{Nothing,AbstractMatrix} = nothing, return_info::Bool = false, history_cap::Int = 4size(A, 2))
    cap = max(history_cap, 0)
    D, BB, s2, α, X, hist, it, flags = greedy_batch_setup(A, B, σ², alpha, cap)
    nsig, N = size(BB, 2), size(D, 2)
    GC.@preserve BB s2 α X hist it flags check(D, ccall((:csmp_rmps_batch, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Cint, Ptr{Cdouble}, Int64, Int64, Int64, Int64, Cdouble, Ptr{Cdouble}, Int64, Ptr{Cdouble},
         Int64, Ptr{Cdouble}, Int64, Cint, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Cint}),
        D.ctx, BB, dtype_code(eltype(BB)), max(stride(BB, 2), size(BB, 1)), nsig, CSMP_HOST, s2, length(s2), maxiter, maxiter_acquisition,
        maxiter_deletion, min_increase, α, max(N, 1), X, max(N, 1), α, max(N, 1), CSMP_HOST, cap == 0 ? C_NULL : pointer(hist), cap, it, flags))
    xs = [sparse(X[:, s]) for s in 1:nsig]
    return return_info ? (xs, [greedy_batch_info(it, flags, α, hist, s, min(Int(it[s]), cap)) for s in 1:nsig]) : xs
end
fsbl_batch(A::MatOrDict, B::AbstractMatrix, Σ::AbstractMatrix; kwargs...) = error("fsbl_batch: only scalar noise variances σ² are served, not a covariance matrix")
rmps_batch(A::MatOrDict, B::AbstractMatrix, Σ::AbstractMatrix; kwargs...) = error("rmps_batch: only scalar noise variances σ² are served, not a covariance matrix")
rmps_batch(A::MatOrDict, B::AbstractMatrix, ::Val{true}, args...; kwargs...) = error("rmps_batch: the σ²-optimising form is not served: pass the noise variance σ²")

# ---------------------------------------------------------------------------------- dictionary analysis
# src/util.jl:2,96-115: colnorms, coherence, babel, cumbabel.  The inner products are raw, as in the reference (which assumes unit-norm
# columns); normalize = true divides each by ‖a_i‖ ‖a_j‖.  cumbabel_pair also returns the columns (i, j), i < j, 1-based, that attain
# μ₁(1) (the lowest i, then the lowest j among equals; (0, 0) for a single column).
const CSMP_BABEL_KMAX = 1024
function colnorms(A::MatOrDict)
    D = dict(A)
    out = zeros(Float64, size(D, 2))
    GC.@preserve out check(D, ccall((:csmp_colnorms, libcsmp), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint), D.ctx, out, CSMP_HOST))
    return out
end
function cumbabel_pair(A::MatOrDict, k::Integer; normalize::Bool = false)
    D = dict(A)
    1 ≤ k ≤ min(size(D, 2), CSMP_BABEL_KMAX) || throw("k = $k has to lie in 1 .. min(size(A, 2), $CSMP_BABEL_KMAX)")
    μ₁, pair = zeros(Float64, k), zeros(Int64, 2)
    GC.@preserve μ₁ pair check(D, ccall((:csmp_cumbabel, libcsmp), Cint, (Ptr{Cvoid}, Int64, Cint, Ptr{Cdouble}, Ptr{Int64}),
        D.ctx, k, Cint(normalize), μ₁, pair))
    return μ₁, (Int(pair[1]) + 1, Int(pair[2]) + 1)
end
cumbabel(A::MatOrDict, k::Integer; normalize::Bool = false) = cumbabel_pair(A, k; normalize = normalize)[1]
babel(A::MatOrDict, k::Integer; normalize::Bool = false) = cumbabel(A, k; normalize = normalize)[k]
function coherence(A::MatOrDict; normalize::Bool = false, return_pair::Bool = false)
    μ₁, pair = cumbabel_pair(A, 1; normalize = normalize)
    return return_pair ? (μ₁[1], pair) : μ₁[1]
end

# ---------------------------------------------------------------------------------- sp
# src/twostage.jl:87-101
function sp(A::MatOrDict{T}, b::AbstractVector, k::Int, δ::Real = 1e-12; maxiter = 16k) where {T}
    2k > length(b) && error("2k = $(2k) > $(length(b)) = length(b) is invalid for Subspace Pursuit")
    D = dict(A)
    bb, bt = bvec(b)
    idx, val, nnz, iters = zeros(Int64, 2k), zeros(Float64, 2k), Ref{Int64}(0), Ref{Int64}(0)
    GC.@preserve bb idx val check(D, ccall((:csmp_sp, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Cdouble, Int64, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}, Ref{Int64}),
        D.ctx, bb, bt, k, δ, maxiter, idx, val, nnz, iters))
    to_sparse(size(D, 2), idx, val, nnz[])
end

# ---------------------------------------------------------------------------------- ompr
# src/twostage.jl:184-202 (x starting empty: the support is filled by oblivious_acquisition!)
function ompr(A::MatOrDict{T}, b::AbstractVector, k::Int, δ::Real; maxiter = size(A, 1)) where {T}
    D = dict(A)
    bb, bt = bvec(b)
    idx, val, nnz, iters = zeros(Int64, k), zeros(Float64, k), Ref{Int64}(0), Ref{Int64}(0)
    GC.@preserve bb idx val check(D, ccall((:csmp_ompr, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Cdouble, Int64, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}, Ref{Int64}),
        D.ctx, bb, bt, k, δ, maxiter, idx, val, nnz, iters))
    to_sparse(size(D, 2), idx, val, nnz[])
end

# [ompr(A, B[:, s], k, δ_s; maxiter) for s in axes(B, 2)]: up to eight signals take their update! in lockstep, the product sweep of an
# iteration reads the dictionary once for all of them, every result the single call's bit for bit (csmp_ompr_batch).  δ: one threshold,
# or one per column.  return_info: (xs, infos), per signal the iterations and whether it was solved alone (it left its group).
const CSMP_OMPR_SOLVED_ALONE = 1
function ompr_batch(A::MatOrDict, B::AbstractMatrix, k::Int, δ::Union{Real,AbstractVector}; maxiter::Int = size(A, 1), return_info::Bool = false)
    D = dict(A)
    BB = B isa StridedMatrix && eltype(B) <: Union{Float32,Float64} && stride(B, 1) == 1 ? B : convert(Matrix{Float64}, B)
    size(BB, 1) == size(D, 1) || throw(DimensionMismatch("size(B, 1) = $(size(BB, 1)) but size(A, 1) = $(size(D, 1))"))
    nsig = size(BB, 2)
    1 <= k <= min(size(D, 1), size(D, 2)) || throw(ArgumentError("k = $k has to lie in 1:min(size(A)...)"))
    d = δ isa Real ? Float64[δ] : convert(Vector{Float64}, δ)
    length(d) in (1, nsig) || throw(DimensionMismatch("length(δ) = $(length(d)) but B holds $nsig signals"))
    any(isnan, d) && throw(ArgumentError("δ is NaN"))
    idx, val = zeros(Int64, k, max(nsig, 1)), zeros(Float64, k, max(nsig, 1))
    nnz, it, flags = zeros(Int64, max(nsig, 1)), zeros(Int64, max(nsig, 1)), zeros(Cint, max(nsig, 1))
    GC.@preserve BB d idx val nnz it flags check(D, ccall((:csmp_ompr_batch, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Cint, Int64, Ptr{Cdouble}, Int64, Int64, Ptr{Int64}, Ptr{Cdouble}, Ptr{Int64}, Ptr{Int64},
         Ptr{Cint}),
        D.ctx, BB, dtype_code(eltype(BB)), max(stride(BB, 2), size(BB, 1)), nsig, CSMP_HOST, k, d, length(d), maxiter, idx, val, nnz, it, flags))
    xs = [to_sparse(size(D, 2), idx[:, s], val[:, s], nnz[s]) for s in 1:nsig]
    return return_info ? (xs, [(iterations = Int(it[s]), solved_alone = flags[s] & CSMP_OMPR_SOLVED_ALONE != 0) for s in 1:nsig]) : xs
end

# ---------------------------------------------------------------------------------- fr = ols = oomp = ormp
# src/forward.jl:34-54 (x starting empty)
function fr(A::MatOrDict{T}, b::AbstractVector, max_ε::Real, min_δ::Real, k::Int = size(A, 1)) where {T}
    size(A, 1) == length(b) || throw(DimensionMismatch("size(A, 1) = $(size(A, 1)) ≠ $(length(b)) = length(b)"))
    D = dict(A)
    bb, bt = bvec(b)
    k = min(k, size(A, 1))
    idx, val, nnz = zeros(Int64, max(k, 1)), zeros(Float64, max(k, 1)), Ref{Int64}(0)
    GC.@preserve bb idx val check(D, ccall((:csmp_fr, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Cdouble, Cdouble, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}, Ptr{Int64}),
        D.ctx, bb, bt, k, max_ε, min_δ, idx, val, nnz, C_NULL))
    to_sparse(size(D, 2), idx, val, nnz[])
end
fr(A::MatOrDict, b::AbstractVector; max_residual::Real = 0., min_decrease::Real = 0., sparsity::Int = size(A, 2)) =
    fr(A, b, max_residual, min_decrease, sparsity)
const ols = fr
const oomp = fr
const ormp = fr

# ---------------------------------------------------------------------------------- srr
# src/twostage.jl:3-33 (x starting empty; initialization 1 = oblivious, 2 = forward regression, 3 = random: the k atoms are
# drawn here without replacement (randperm; the reference: sample(1:n, k, replace = false), src/matchingpursuit.jl:196) or taken
# from `init` (1-based), and handed to csmp_srr_from)
function srr(A::MatOrDict{T}, b::AbstractVector, k::Int, δ::Real = 1e-12; maxiter = 4k,
             initialization::Int = 1, l::Int = 1, init = nothing) where {T}
    D = dict(A)
    bb, bt = bvec(b)
    idx, val, nnz, iters = zeros(Int64, k + l + 1), zeros(Float64, k + l + 1), Ref{Int64}(0), Ref{Int64}(0)
    if initialization == 3
        ind = init === nothing ? randperm(size(D, 2))[1:k] : collect(init)
        ind0 = Int64.(ind) .- 1
        GC.@preserve bb idx val ind0 check(D, ccall((:csmp_srr_from, libcsmp), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Cdouble, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}, Ref{Int64}),
            D.ctx, bb, bt, k, δ, maxiter, ind0, l, idx, val, nnz, iters))
        return to_sparse(size(D, 2), idx, val, nnz[])
    end
    GC.@preserve bb idx val check(D, ccall((:csmp_srr, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Cdouble, Int64, Cint, Int64, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}, Ref{Int64}),
        D.ctx, bb, bt, k, δ, maxiter, initialization, l, idx, val, nnz, iters))
    to_sparse(size(D, 2), idx, val, nnz[])
end

# ---------------------------------------------------------------------------------- rmp, foba
# src/stepwise.jl:5-56 (x starting empty).  kmax bounds the support the forward stage may build (<= 4095).
# (one literal ccall per entry point: ccall needs its symbol and its argument types as constants)
function stepwise_out(A::MatOrDict, kmax::Int)
    cap = min(size(A, 1), size(A, 2), 4095, kmax > 0 ? kmax : typemax(Int))
    cap, zeros(Int64, cap + 1), zeros(Float64, cap + 1), Ref{Int64}(0)
end
function rmp(A::MatOrDict, b::AbstractVector, δ::Real, maxiter::Int = 1; kmax::Int = 0)
    D = dict(A)
    bb, bt = bvec(b)
    cap, idx, val, nnz = stepwise_out(A, kmax)
    GC.@preserve bb idx val check(D, ccall((:csmp_rmp_delta, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Int64, Int64, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}),
        D.ctx, bb, bt, Float64(δ), Int64(maxiter), cap, idx, val, nnz))
    to_sparse(size(D, 2), idx, val, nnz[])
end
function rmp(A::MatOrDict, b::AbstractVector, k::Int; kmax::Int = 0)
    D = dict(A)
    bb, bt = bvec(b)
    cap, idx, val, nnz = stepwise_out(A, kmax)
    GC.@preserve bb idx val check(D, ccall((:csmp_rmp_k, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}),
        D.ctx, bb, bt, Int64(k), cap, idx, val, nnz))
    to_sparse(size(D, 2), idx, val, nnz[])
end
# isfast is accepted for signature parity (src/stepwise.jl:47): Val(false) computes the same backward scores the slow way
function foba(A::MatOrDict, b::AbstractVector, δ::Real; kmax::Int = 0, isfast::Val = Val(true))
    D = dict(A)
    bb, bt = bvec(b)
    cap, idx, val, nnz = stepwise_out(A, kmax)
    GC.@preserve bb idx val check(D, ccall((:csmp_foba, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Int64, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}),
        D.ctx, bb, bt, Float64(δ), cap, idx, val, nnz))
    to_sparse(size(D, 2), idx, val, nnz[])
end

# ---------------------------------------------------------------------------------- br = fbr, lace
# src/backward.jl:27-41,148-162,226-242
function backward_call(A::MatOrDict, b::AbstractVector, max_ε::Real, max_δ::Real, k::Int, lace::Bool)
    n, m = size(A)
    n ≥ m || throw("A needs to be overdetermined but is of size ($n, $m)")
    D = dict(A)
    bb, bt = bvec(b)
    idx, val, nnz = zeros(Int64, m + 1), zeros(Float64, m + 1), Ref{Int64}(0)
    GC.@preserve bb idx val check(D, ccall((:csmp_br, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Cdouble, Int64, Cint, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}),
        D.ctx, bb, bt, max_ε, max_δ, k, lace, idx, val, nnz))
    to_sparse(m, idx, val, nnz[])
end
br(A::MatOrDict, b::AbstractVector, max_ε::Real, max_δ::Real, k::Int) = backward_call(A, b, max_ε, max_δ, k, false)
br(A::MatOrDict, b::AbstractVector; max_residual::Real = Inf, max_increase::Real = Inf, sparsity::Int = 0) =
    br(A, b, max_residual, max_increase, sparsity)
const fbr = br
lace(A::MatOrDict, b::AbstractVector, ε::Real, δ::Real, k::Int) = backward_call(A, b, ε, δ, k, true)
lace(A::MatOrDict, b::AbstractVector; max_residual::Real = Inf, max_increase::Real = Inf, sparsity::Int = 0) =
    lace(A, b, max_residual, max_increase, sparsity)

# ---------------------------------------------------------------------------------- functors
# abstract type Update; (U::Update)(x) = update!(U, x)   (src/CompressedSensing.jl:22-23)
abstract type Update{T} end
(U::Update)(x) = update!(U, x)

# Every functor works on a context of its OWN that borrows the Dictionary's device memory (csmp_clone): like the
# reference's P objects, two functors on one A -- or a functor and a driver call -- share A and nothing else.
mutable struct DevicePursuit{T} <: Update{T}
    D::Dictionary{T}     # keeps the borrowed dictionary alive
    ctx::Ptr{Cvoid}      # the clone
    algo::Cint
    l::Int
    kcap::Int
    b::Any               # the signal (the reference's P.b): a two-stage functor restarts from a foreign x with it
end
function begin_solver(A::MatOrDict{T}, b, algo, kcap, l = 1) where {T}
    D = dict(A)
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    check(D, ccall((:csmp_clone, libcsmp), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), D.ctx, ref))
    P = DevicePursuit{T}(D, ref[], algo, l, kcap, b)
    finalizer(p -> ccall((:csmp_destroy, libcsmp), Cint, (Ptr{Cvoid},), p.ctx), P)
    bb, bt = bvec(b)
    GC.@preserve bb pcheck(P, ccall((:csmp_solver_begin, libcsmp), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Int64, Ptr{Int64}, Ptr{Cdouble}, Int64),
        P.ctx, algo, bb, bt, kcap, C_NULL, C_NULL, 0))
    P
end
pcheck(P::DevicePursuit, rc::Integer) =
    rc == 0 || throw(unsafe_string(ccall((:csmp_last_error, libcsmp), Cstring, (Ptr{Cvoid},), P.ctx)))
MP(A, b; steps::Integer = 4096) = begin_solver(A, b, ALGO_MP, steps)                       # :19-24 (steps: length of the device's step log)
OMP(A, b, k::Integer = size(A, 1)) = begin_solver(A, b, ALGO_OMP, min(k, size(A, 1)))      # :54-60
GOMP(A, b, l::Int, k::Integer = size(A, 1)) = begin_solver(A, b, ALGO_GOMP, min(k, size(A, 1)), l)  # :108-114

# update!(P, x): one greedy step on the device, then x <- the device's current solution
function update!(P::DevicePursuit, x::SparseVector = spzeros(size(P.D, 2)), l::Int = P.l)
    (P.algo == ALGO_SP || P.algo == ALGO_OMPR) && return update_twostage!(P, x)
    pcheck(P, ccall((:csmp_solver_step, libcsmp), Cint, (Ptr{Cvoid}, Int64), P.ctx, l))
    idx, val, nnz = zeros(Int64, P.kcap), zeros(Float64, P.kcap), Ref{Int64}(0)
    GC.@preserve idx val pcheck(P, ccall((:csmp_solver_state, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}, Ptr{Cdouble}, Ptr{Int64}, Ptr{Cint}),
        P.ctx, idx, val, nnz, C_NULL, C_NULL, C_NULL))
    y = to_sparse(size(P.D, 2), idx, val, nnz[])
    resize!(x.nzind, nnz[]); resize!(x.nzval, nnz[])
    copyto!(x.nzind, y.nzind); copyto!(x.nzval, y.nzval)
    return x
end

# ---- the two-stage functors: SP (src/twostage.jl:42-83) and OMPR (:110-180).  The device solver owns the x it produced last; the x
# handed to update! is checked against it: SP restarts from a foreign x (the reference recomputes the residual from whatever x it
# is given, :68), OMPR refuses one (its factorisation belongs to the x it built).
function SP(A::MatOrDict, b::AbstractVector, k::Integer)
    2k > length(b) && error("2k = $(2k) > $(length(b)) = length(b) is invalid for Subspace Pursuit")  # :55
    begin_solver(A, b, ALGO_SP, Int(k))
end
const SubspacePursuit = SP
OMPR(A::MatOrDict, b::AbstractVector, k::Int) = begin_solver(A, b, ALGO_OMPR, k)  # :124-132
mutable struct TwoStageX  # the x a two-stage functor returned last (per functor; keyed by the clone's handle)
    nzind::Vector{Int}
    nzval::Vector{Float64}
end
const LAST_X = Dict{Ptr{Cvoid},TwoStageX}()
function fetch_x!(P::DevicePursuit, x::SparseVector)
    cap = 2 * P.kcap
    idx, val, nnz = zeros(Int64, cap), zeros(Float64, cap), Ref{Int64}(0)
    GC.@preserve idx val pcheck(P, ccall((:csmp_solver_state, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Int64}, Ptr{Cdouble}, Ref{Int64}, Ptr{Cdouble}, Ptr{Int64}, Ptr{Cint}),
        P.ctx, idx, val, nnz, C_NULL, C_NULL, C_NULL))
    y = to_sparse(size(P.D, 2), idx, val, nnz[])
    resize!(x.nzind, nnz[]); resize!(x.nzval, nnz[])
    copyto!(x.nzind, y.nzind); copyto!(x.nzval, y.nzval)
    LAST_X[P.ctx] = TwoStageX(copy(x.nzind), copy(x.nzval))
    return x
end
is_mine(P::DevicePursuit, x::SparseVector) = (l = get(LAST_X, P.ctx, TwoStageX(Int[], Float64[])); x.nzind == l.nzind && x.nzval == l.nzval)
# a foreign x restarts the SP solver from it (csmp_solver_begin with the x's entries, 0-based)
function load_x!(P::DevicePursuit, x::SparseVector)
    is_mine(P, x) && return
    bb, bt = bvec(P.b)
    i0, v0 = x.nzind .- 1, Vector{Float64}(x.nzval)
    GC.@preserve bb i0 v0 pcheck(P, ccall((:csmp_solver_begin, libcsmp), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Int64, Ptr{Int64}, Ptr{Cdouble}, Int64),
        P.ctx, P.algo, bb, bt, P.kcap, i0, v0, length(i0)))
    LAST_X[P.ctx] = TwoStageX(copy(x.nzind), copy(x.nzval))
end
# sp_acquisition!(P, x, k = P.k): :67-72
function sp_acquisition!(P::DevicePursuit, x::SparseVector, k::Int = P.kcap)
    P.algo == ALGO_SP || throw("sp_acquisition!: P is not an SP")
    load_x!(P, x)
    pcheck(P, ccall((:csmp_solver_acquire, libcsmp), Cint, (Ptr{Cvoid}, Int64), P.ctx, k))
    fetch_x!(P, x)
end
# oblivious_acquisition!(P, x, k): src/matchingpursuit.jl:207-216, for the functors that keep an updatable QR (OMPR, OMP, GOMP)
function oblivious_acquisition!(P::DevicePursuit, x::SparseVector, k::Int)
    P.algo in (ALGO_OMPR, ALGO_OMP, ALGO_GOMP) || throw("oblivious_acquisition!: P keeps no updatable QR")
    pcheck(P, ccall((:csmp_solver_acquire, libcsmp), Cint, (Ptr{Cvoid}, Int64), P.ctx, k))
    fetch_x!(P, x)
end
# update!(P::SP, x) (:75-83) and update!(P::OMPR, x) (:134-180, eta = 1): nnz(x) == k or the reference's String is thrown (:76, :135)
function update_twostage!(P::DevicePursuit, x::SparseVector)
    nnz(x) == P.kcap || throw("nnz(x) = $(nnz(x)) ≠ $(P.kcap) = k")
    if P.algo == ALGO_SP
        load_x!(P, x)
    else
        is_mine(P, x) || throw("update!(P::OMPR, x): x is not the vector this OMPR object's QR was built for")
    end
    pcheck(P, ccall((:csmp_solver_step, libcsmp), Cint, (Ptr{Cvoid}, Int64), P.ctx, 1))
    fetch_x!(P, x)
end

# ---------------------------------------------------------------------------------- many signals
# [omp(A, B[:, s], eps, k) for s in axes(B, 2)] on one GPU.  method = :exact: single-signal sweeps, three signals
# pipelined (csmp_omp_batch); :mfma: one bf16 screening GEMM per step + Float64 rescoring (csmp_omp_batch_mfma), with
# certificate = :rigorous (the library's default) | :statistical and gram = true | false (CSMP_OPT_BATCH_CERT /
# CSMP_OPT_BATCH_GRAM).  A keyword that is not given leaves the Dictionary's option (set_option!) alone; one that is given holds
# for this call only.
# Returns (idx k x nsig 0-based, -1 padded; val; nnz) as the C ABI does -- the layout csmp_pack_results packs.
function omp_batch_raw(A::MatOrDict{T}, B::StridedMatrix, ε::Real, k::Int; method::Symbol = :exact,
                       certificate::Union{Symbol,Nothing} = nothing, gram::Union{Bool,Nothing} = nothing) where {T}
    D = dict(A)
    saved = Pair{Symbol,Int64}[]
    if method === :mfma && certificate !== nothing
        push!(saved, :batch_cert => get_option(D, :batch_cert))
        set_option!(D, :batch_cert, certificate === :rigorous ? 1 : 0)
    end
    if method === :mfma && gram !== nothing
        push!(saved, :batch_gram => get_option(D, :batch_gram))
        set_option!(D, :batch_gram, gram ? 1 : 0)
    end
    try
        return omp_batch_call(D, B, ε, k, method)
    finally
        for (key, v) in saved
            set_option!(D, key, v)
        end
    end
end
function omp_batch_call(D::Dictionary, B::StridedMatrix, ε::Real, k::Int, method::Symbol)
    BB = eltype(B) <: Union{Float32,Float64} ? B : convert(Matrix{Float64}, B)
    nsig = size(BB, 2)
    idx, val, nnz = fill(Int64(-1), k, nsig), zeros(Float64, k, nsig), zeros(Int64, nsig)
    if method === :mfma
        GC.@preserve BB idx val nnz check(D, ccall((:csmp_omp_batch_mfma, libcsmp), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Cint, Int64, Cdouble, Ptr{Int64}, Ptr{Cdouble}, Ptr{Int64}, Cint),
            D.ctx, BB, dtype_code(eltype(BB)), stride(BB, 2), nsig, CSMP_HOST, k, ε, idx, val, nnz, CSMP_HOST))
    else
        GC.@preserve BB idx val nnz check(D, ccall((:csmp_omp_batch, libcsmp), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Cint, Int64, Cdouble, Ptr{Int64}, Ptr{Cdouble}, Ptr{Int64}, Cint),
            D.ctx, BB, dtype_code(eltype(BB)), stride(BB, 2), nsig, CSMP_HOST, k, ε, idx, val, nnz, CSMP_HOST))
    end
    idx, val, nnz
end
omp_batch(A::MatOrDict, B::StridedMatrix, ε::Real, k::Int; kw...) = begin
    idx, val, nnz = omp_batch_raw(A, B, ε, k; kw...)
    [to_sparse(size(A, 2), idx[:, s], val[:, s], nnz[s]) for s in 1:size(B, 2)]
end

# [mp(A, B[:, s], k) for s in axes(B, 2)], x starting from 0: up to eight signals share each pass over A (csmp_mp_batch)
function mp_batch(A::MatOrDict{T}, B::StridedMatrix, k::Int) where {T}
    D = dict(A)
    BB = eltype(B) <: Union{Float32,Float64} ? B : convert(Matrix{Float64}, B)
    nsig = size(BB, 2)
    idx, val, nnz = fill(Int64(-1), k, nsig), zeros(Float64, k, nsig), zeros(Int64, nsig)
    GC.@preserve BB idx val nnz check(D, ccall((:csmp_mp_batch, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Cint, Int64, Ptr{Int64}, Ptr{Cdouble}, Ptr{Int64}, Cint),
        D.ctx, BB, dtype_code(eltype(BB)), stride(BB, 2), nsig, CSMP_HOST, k, idx, val, nnz, CSMP_HOST))
    [to_sparse(size(A, 2), idx[:, s], val[:, s], nnz[s]) for s in 1:nsig]
end

# somp(A, B, ε, k; p): simultaneous OMP for columns of B that share ONE support (Tropp, Gilbert and Strauss 2006) -- omp's driver with the
# residual matrix in place of the residual: the atom that maximises sum_l |<a_j, r_l>|^p, one append, every residual projected
# (csmp_somp).  Returns SparseVectors that all carry the same nzind; return_info: (xs, (order, resnorm, steps, passes)).
function somp(A::MatOrDict{T}, B::AbstractMatrix, ε::Real, k::Int = min(size(A)...); p::Int = 1, return_info::Bool = false) where {T}
    ε ≥ 0 || throw(ArgumentError("ε = $ε has to be non-negative"))
    p in (1, 2) || throw(ArgumentError("p = $p has to be 1 or 2"))
    D = dict(A)
    BB = B isa StridedMatrix && eltype(B) <: Union{Float32,Float64} && stride(B, 1) == 1 ? B : convert(Matrix{Float64}, B)
    size(BB, 1) == size(D, 1) || throw(DimensionMismatch("size(B, 1) = $(size(BB, 1)) but size(A, 1) = $(size(D, 1))"))
    1 <= k <= min(size(D, 1), size(D, 2)) || throw(ArgumentError("k = $k has to lie in 1:min(size(A)...)"))
    nsig = size(BB, 2)
    idx, order, val = zeros(Int64, k), zeros(Int64, k), zeros(Float64, k, max(nsig, 1))
    resnorm, nnz, passes = zeros(Float64, max(nsig, 1)), Ref{Int64}(0), Ref{Int64}(0)
    GC.@preserve BB idx val order resnorm check(D, ccall((:csmp_somp, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Cint, Int64, Cdouble, Cint, Ptr{Int64}, Ptr{Cdouble}, Int64, Ref{Int64}, Ptr{Int64},
         Ptr{Cdouble}, Ref{Int64}, Cint),
        D.ctx, BB, dtype_code(eltype(BB)), max(stride(BB, 2), size(BB, 1)), nsig, CSMP_HOST, k, ε, p, idx, val, k, nnz, order, resnorm, passes,
        CSMP_HOST))
    n = Int(nnz[])
    xs = [SparseVector(size(D, 2), idx[1:n] .+ 1, val[1:n, s]) for s in 1:nsig]
    return return_info ? (xs, (order = order[1:n] .+ 1, resnorm = resnorm[1:nsig], steps = n, passes = Int(passes[]))) : xs
end
somp(A::MatOrDict{T}, B::AbstractMatrix, k::Int; kw...) where {T} = somp(A, B, eps(T), k; kw...)
somp(A::MatOrDict{T}, B::AbstractMatrix; max_residual = eps(T), sparsity = min(size(A)...), kw...) where {T} =
    somp(A, B, max_residual, sparsity; kw...)

# [gomp(A, B[:, s], l, eps, k) for s in axes(B, 2)]: two solves in flight on two streams (csmp_gomp_batch)
function gomp_batch(A::MatOrDict{T}, B::StridedMatrix, l::Int, ε::Real, k::Int) where {T}
    D = dict(A)
    BB = eltype(B) <: Union{Float32,Float64} ? B : convert(Matrix{Float64}, B)
    nsig = size(BB, 2)
    idx, val, nnz = fill(Int64(-1), k, nsig), zeros(Float64, k, nsig), zeros(Int64, nsig)
    GC.@preserve BB idx val nnz check(D, ccall((:csmp_gomp_batch, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Cint, Int64, Int64, Cdouble, Ptr{Int64}, Ptr{Cdouble}, Ptr{Int64}, Cint),
        D.ctx, BB, dtype_code(eltype(BB)), stride(BB, 2), nsig, CSMP_HOST, l, k, ε, idx, val, nnz, CSMP_HOST))
    [to_sparse(size(A, 2), idx[:, s], val[:, s], nnz[s]) for s in 1:nsig]
end

# [sp(A, B[:, s], k, δ; maxiter) for s in axes(B, 2)]: up to four solves in flight (csmp_sp_batch; CSMP_OPT_SOLVES_IN_FLIGHT)
function sp_batch(A::MatOrDict{T}, B::StridedMatrix, k::Int, δ::Real = 1e-12; maxiter = 16k) where {T}
    2k > size(B, 1) && error("2k = $(2k) > $(size(B, 1)) = length(b) is invalid for Subspace Pursuit")
    D = dict(A)
    BB = eltype(B) <: Union{Float32,Float64} ? B : convert(Matrix{Float64}, B)
    nsig = size(BB, 2)
    idx, val, nnz, its = fill(Int64(-1), k, nsig), zeros(Float64, k, nsig), zeros(Int64, nsig), zeros(Int64, nsig)
    GC.@preserve BB idx val nnz its check(D, ccall((:csmp_sp_batch, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Int64, Cdouble, Int64, Ptr{Int64}, Ptr{Cdouble}, Ptr{Int64}, Ptr{Int64}),
        D.ctx, BB, dtype_code(eltype(BB)), stride(BB, 2), nsig, k, δ, maxiter, idx, val, nnz, its))
    [to_sparse(size(A, 2), idx[:, s], val[:, s], nnz[s]) for s in 1:nsig]
end

# Signals sharded over ranks (SURVEY section 8e), ONE PROCESS PER GPU, the collective INSIDE the library (csmp_omp_sharded: one
# ncclAllGather over xGMI, device memory to device memory) -- no collective package on the Julia side:
#     id = rank == 0 ? comm_id() : nothing          # 128 bytes; hand them to every rank by whatever started the ranks
#     comm_init!(D, id, rank, world)                # (a file, a socket, Distributed.remotecall_fetch, ...): collective
#     xs = omp_sharded(D, B[:, lo+1:hi], nsig, ε, k; method = :mfma)   # every rank: its block in, ALL nsig results out
const CSMP_COMM_ID_BYTES = 128
function comm_id()
    id = zeros(UInt8, CSMP_COMM_ID_BYTES)
    rc = ccall((:csmp_comm_id, libcsmp), Cint, (Ptr{Cvoid},), id)
    rc == 0 || throw(unsafe_string(ccall((:csmp_last_error, libcsmp), Cstring, (Ptr{Cvoid},), C_NULL)))
    id
end
comm_init!(D::Dictionary, id::Vector{UInt8}, rank::Integer, world::Integer) =
    check(D, ccall((:csmp_comm_init, libcsmp), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint), D.ctx, id, rank, world))
comm_free!(D::Dictionary) = check(D, ccall((:csmp_comm_free, libcsmp), Cint, (Ptr{Cvoid},), D.ctx))
# this rank's contiguous block of nsig signals, 1-based inclusive (csmp_shard_range)
function shard_range(nsig::Integer, rank::Integer, world::Integer)
    lo, hi = Ref{Int64}(0), Ref{Int64}(0)
    ccall((:csmp_shard_range, libcsmp), Cint, (Int64, Cint, Cint, Ref{Int64}, Ref{Int64}), nsig, rank, world, lo, hi)
    (lo[] + 1):hi[]
end
function omp_sharded(D::Dictionary, Bblock::StridedMatrix, nsig::Integer, ε::Real, k::Int; method::Symbol = :exact)
    BB = eltype(Bblock) <: Union{Float32,Float64} ? Bblock : convert(Matrix{Float64}, Bblock)
    idx, val, nnz = fill(Int64(-1), k, nsig), zeros(Float64, k, nsig), zeros(Int64, nsig)
    GC.@preserve BB idx val nnz check(D, ccall((:csmp_omp_sharded, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Cint, Int64, Cdouble, Cint, Ptr{Int64}, Ptr{Cdouble}, Ptr{Int64}, Cint),
        D.ctx, BB, dtype_code(eltype(BB)), max(stride(BB, 2), size(D, 1)), nsig, CSMP_HOST, k, ε, method === :mfma ? 1 : 0, idx, val, nnz, CSMP_HOST))
    [to_sparse(size(D, 2), idx[:, s], val[:, s], nnz[s]) for s in 1:nsig]
end

# The same sharding under a collective the HOST brings (any single-signal driver, or a site that already runs MPI):
# `allgather(v::Vector{Float64}) -> Vector{Float64}`; every rank passes a block of the same length (blocks are padded to the
# longest one: ceil(nsig / world) signals).
function omp_sharded(A::MatOrDict, B::StridedMatrix, ε::Real, k::Int, rank::Int, world::Int, allgather;
                     method::Symbol = :exact, kw...)
    nsig = size(B, 2)
    lo, hi = Ref{Int64}(0), Ref{Int64}(0)
    ccall((:csmp_shard_range, libcsmp), Cint, (Int64, Cint, Cint, Ref{Int64}, Ref{Int64}), nsig, rank, world, lo, hi)
    n = hi[] - lo[]
    idx, val, nnz = omp_batch_raw(A, B[:, lo[]+1:hi[]], ε, k; method = method, kw...)
    maxn = cld(nsig, world)
    w = 2k + 1
    packed = zeros(Float64, w * maxn)                     # row-major rows of 2k+1: [idx | val | nnz] per signal
    ccall((:csmp_pack_results, libcsmp), Cint, (Ptr{Int64}, Ptr{Cdouble}, Ptr{Int64}, Int64, Int64, Ptr{Cdouble}),
          idx, val, nnz, k, n, packed)                    # (idx/val are k x n column-major = n rows of k, as the ABI wants)
    all = allgather(packed)
    out = Vector{SparseVector{Float64,Int}}(undef, nsig)
    for r in 0:world-1
        ccall((:csmp_shard_range, libcsmp), Cint, (Int64, Cint, Cint, Ref{Int64}, Ref{Int64}), nsig, r, world, lo, hi)
        m = hi[] - lo[]
        ri, rv, rn = zeros(Int64, k, m), zeros(Float64, k, m), zeros(Int64, m)
        block = all[r*w*maxn+1:r*w*maxn+w*m]
        ccall((:csmp_unpack_results, libcsmp), Cint, (Ptr{Cdouble}, Int64, Int64, Ptr{Int64}, Ptr{Cdouble}, Ptr{Int64}),
              block, k, m, ri, rv, rn)
        for s in 1:m
            out[lo[]+s] = to_sparse(size(A, 2), ri[:, s], rv[:, s], rn[s])
        end
    end
    out
end

# argmaxinner!(P) / argmaxinner!(P, k): src/matchingpursuit.jl:181-193
function argmaxinner(D::Dictionary, r::AbstractVector, k::Int = 1)
    rr = convert(Vector{Float64}, r)
    ti, tv = zeros(Int64, k), zeros(Float64, k)
    GC.@preserve rr ti tv check(D, ccall((:csmp_sweep, libcsmp), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{Cdouble}),
        D.ctx, rr, C_NULL, k, ti, tv))
    k == 1 ? ti[1] + 1 : ti .+ 1
end

end # module
