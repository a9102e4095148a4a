# julia/dfm_hip.jl -- the thin `ccall` shim between QuantEcon/dynamic_factor_models' Julia code and
# libdfmhip.so (include/dfm_hip.h).  It fills the dispatch slot the reference declares but leaves empty:
# `struct Parametric <: EstimationMethod end` (dfm_functions.ipynb:21-23); the reference implements only
# `estimate!(m, ::NonParametric)` (dfm_functions.ipynb:530-543).
#
# Usage (in the notebook's working directory, after the reference's own includes so that DFMModel,
# Parametric, standardize_data and drop_missing_col exist -- Stock_Watson.ipynb:39-41):
#     include("readin_functions.jl"); @nbinclude("dfm_functions.ipynb")
#     include("julia/dfm_hip.jl")                      # this file; needs ENV["DFMHIP_LIB"] or the default path
#     estimate!(dfmm, Parametric(); max_em_iter = 50)  # instead of estimate!(dfmm, NonParametric())
# Nothing else in the notebook changes: `Stock_Watson.ipynb` never passes `Parametric()` itself, so it keeps
# running unchanged on the pure-Julia path.
#
# NOT EXECUTED IN THE BUILD IMAGE (no Julia there): kept deliberately thin -- every numerical step is a
# single ccall; the same sequence of calls is exercised by dynamic_factor_models_amd/api.py (tests/
# test_gpu_api.py), which mirrors this file step by step, and tests/test_julia_shim_cpu.py parses every ccall below
# and checks symbol, return type, argument count and argument types against include/dfm_hip.h.

module DFMHip

const LIB = get(ENV, "DFMHIP_LIB", joinpath(@__DIR__, "..", "dynamic_factor_models_amd", "lib", "libdfmhip.so"))
const DFM_F_MAY_HAVE_MISSING = Cuint(1)
const DFM_F_SINGULAR_Q = Cuint(2)
const DFM_SV_UNIT_EFFECT = Cuint(4)
const DFM_E_NUMERIC = Cint(-5)

mutable struct Handle
    ptr::Ptr{Cvoid}
end

function check(h::Ptr{Cvoid}, rc::Cint)
    rc == 0 && return nothing
    msg = h == C_NULL ? "no handle" : unsafe_string(ccall((:dfm_last_error, LIB), Cstring, (Ptr{Cvoid},), h))
    error("libdfmhip: status $rc: $msg")            # same style as the reference's error("...") (dfm_functions.ipynb:124-126)
end

function create(device::Integer = 0)
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:dfm_create, LIB), Cint, (Ref{Ptr{Cvoid}}, Cint, Ptr{Cvoid}), ref, device, C_NULL)
    rc == 0 || error("libdfmhip: dfm_create failed with status $rc (no HIP device?)")
    h = Handle(ref[])
    finalizer(x -> (x.ptr != C_NULL && ccall((:dfm_destroy, LIB), Cint, (Ptr{Cvoid},), x.ptr); x.ptr = C_NULL), h)
    return h
end

# One handle (context + device workspace) per device for the whole session: the notebook calls the estimator ~200 times
# per table (Stock_Watson.ipynb:516, 591, 643, 893) and a handle per call would allocate and free the workspace each time.
const HANDLES = Dict{Int,Handle}()
function handle(device::Integer = 0)
    h = get(HANDLES, Int(device), nothing)
    (h === nothing || h.ptr == C_NULL) && (h = HANDLES[Int(device)] = create(device))
    return h
end

# The C side wants panel[b][t][i] with i fastest.  A Julia Array{Float64,3} of size (N, T, B) has exactly
# that memory order, so the shim permutes the reference's T x ns matrix once: permutedims(x, (2, 1)).
to_c_panel(z::AbstractMatrix{Float64}) = reshape(permutedims(z, (2, 1)), size(z, 2), size(z, 1), 1)
nan_for_missing(x) = Float64[ismissing(v) ? NaN : Float64(v) for v in x]       # Union{Missing,Float64} is not C layout

"PCA + OLS start of EM on a balanced standardised T x N panel (dfm_pca_init_batch)."
function pca_init(h::Handle, xbal::Matrix{Float64}, r::Integer)
    T, N = size(xbal)
    panel = to_c_panel(xbal)
    Lam = Array{Float64}(undef, r, N, 1); R = Array{Float64}(undef, N, 1)
    A = Array{Float64}(undef, r, r, 1); Q = similar(A); P0 = similar(A); mu0 = Array{Float64}(undef, r, 1)
    F = Array{Float64}(undef, r, T, 1)
    GC.@preserve panel Lam R A Q mu0 P0 F begin
        rc = ccall((:dfm_pca_init_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                   h.ptr, 1, T, N, r, panel, Lam, R, A, Q, mu0, P0, F)
        check(h.ptr, rc)
    end
    # C row-major [i][k] == Julia column-major (k, i): transpose back to the reference's ns x r / T x r
    return (Lam = permutedims(Lam[:, :, 1]), R = R[:, 1], A = permutedims(A[:, :, 1]), Q = permutedims(Q[:, :, 1]),
            mu0 = mu0[:, 1], P0 = permutedims(P0[:, :, 1]), F = permutedims(F[:, :, 1]))
end

"max_iter EM iterations from the given start (dfm_em_batch); z is T x N with NaN for missing."
function em(h::Handle, z::Matrix{Float64}, p; max_iter::Integer = 50, tol::Real = 1e-6)
    T, N = size(z); r = size(p.Lam, 2)
    panel = to_c_panel(z)
    Lam = reshape(permutedims(p.Lam), r, N, 1); R = reshape(copy(p.R), N, 1)
    A = reshape(permutedims(p.A), r, r, 1); Q = reshape(permutedims(p.Q), r, r, 1)
    mu0 = reshape(copy(p.mu0), r, 1); P0 = reshape(permutedims(p.P0), r, r, 1)
    path = Array{Float64}(undef, max_iter, 1); iters = Array{Cint}(undef, 1)
    f = Array{Float64}(undef, r, T, 1); np = div(r * (r + 1), 2); P = Array{Float64}(undef, np, T, 1)
    flags = any(isnan, z) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)
    start = (copy(Lam), copy(R), copy(A), copy(Q), copy(mu0), copy(P0))
    fallback = false
    GC.@preserve panel Lam R A Q mu0 P0 path iters f P begin
        rc = ccall((:dfm_em_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Cdouble, Ptr{Float64}, Ptr{Cint},
                    Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, T, N, r, panel, Lam, R, A, Q, mu0, P0, max_iter, tol, path, iters, f, P, flags)
        fallback = rc == DFM_E_NUMERIC
        if fallback
            # the information-form recursion inverts Q; a PCA start on fewer than 2r + 1 periods has a rank-deficient VAR
            # residual covariance: run the covariance-form recursion instead (as api.estimate does)
            Lam, R, A, Q, mu0, P0 = start
            rc = ccall((:dfm_em_batch, LIB), Cint,
                       (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                        Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Cdouble, Ptr{Float64}, Ptr{Cint},
                        Ptr{Float64}, Ptr{Float64}, Cuint),
                       h.ptr, 1, T, N, r, panel, Lam, R, A, Q, mu0, P0, max_iter, tol, path, iters, f, P,
                       flags | DFM_F_SINGULAR_Q)
        end
        check(h.ptr, rc)
    end
    k = Int(iters[1])
    return (Lam = permutedims(Lam[:, :, 1]), R = R[:, 1], A = permutedims(A[:, :, 1]), Q = permutedims(Q[:, :, 1]),
            mu0 = mu0[:, 1], P0 = permutedims(P0[:, :, 1]), loglik = path[1:k, 1], iters = k,
            factor = permutedims(f[:, :, 1]), singular_q = fallback)
end

"EM with OBSERVED factors as known regressors (dfm_em_obs_batch; include/dfm_hip.h): z is T x N (NaN = missing), G the
T x r_o observed factors (no gaps), p.Lam N x (r_o + r_u) with the observed-factor loadings FIRST (the reference's column
order, dfm_functions.ipynb:364), p.A / p.Q / p.P0 r_u x r_u, p.mu0 r_u."
function em_obs(h::Handle, z::Matrix{Float64}, G::Matrix{Float64}, p; max_iter::Integer = 50, tol::Real = 1e-6)
    T, N = size(z); ro = size(G, 2); re = size(p.Lam, 2); ru = re - ro
    panel = to_c_panel(z); Gc = reshape(permutedims(G, (2, 1)), ro, T, 1)
    Lam = reshape(permutedims(p.Lam), re, N, 1); R = reshape(copy(p.R), N, 1)
    A = reshape(permutedims(p.A), ru, ru, 1); Q = reshape(permutedims(p.Q), ru, ru, 1)
    mu0 = reshape(copy(p.mu0), ru, 1); P0 = reshape(permutedims(p.P0), ru, ru, 1)
    path = Array{Float64}(undef, max_iter, 1); iters = Array{Cint}(undef, 1)
    f = Array{Float64}(undef, ru, T, 1); np = div(ru * (ru + 1), 2); P = Array{Float64}(undef, np, T, 1)
    flags = any(isnan, z) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)
    GC.@preserve panel Gc Lam R A Q mu0 P0 path iters f P begin
        rc = ccall((:dfm_em_obs_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Cdouble, Ptr{Float64}, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, T, N, ru, ro, panel, Gc, Lam, R, A, Q, mu0, P0, max_iter, tol, path, iters, f, P, flags)
        check(h.ptr, rc)
    end
    k = Int(iters[1])
    return (Lam = permutedims(Lam[:, :, 1]), R = R[:, 1], A = permutedims(A[:, :, 1]), Q = permutedims(Q[:, :, 1]),
            mu0 = mu0[:, 1], P0 = permutedims(P0[:, :, 1]), loglik = path[1:k, 1], iters = k, factor = permutedims(f[:, :, 1]))
end

# C [b][i][k] <-> Julia: a vector of B matrices (rows x cols) -> Array (cols, rows, B), and back
pack3(ms::Vector{Matrix{Float64}}) = cat([permutedims(m) for m in ms]...; dims = 3)
unpack3(a::Array{Float64,3}) = [permutedims(a[:, :, b]) for b in 1:size(a, 3)]

"B smoother passes in ONE call (dfm_ks_pass_batch; with ngpu > 1: dfm_ks_pass_batch_multi, replicates split over the
GPUs): panels[b] is T x N (NaN = missing), params[b] = (Lam N x r, R, A, Q, mu0, P0).  Returns per-replicate smoothed
factors (T x r), packed covariances (T x r(r+1)/2) and log-likelihoods."
function ks_pass_batch(h::Handle, panels::Vector{Matrix{Float64}}, params::Vector; ngpu::Integer = 1)
    B = length(panels); T, N = size(panels[1]); r = size(params[1].Lam, 2)
    panel = cat([permutedims(z, (2, 1)) for z in panels]...; dims = 3)           # (N, T, B) == C [b][t][i]
    Lam = pack3([p.Lam for p in params]); R = hcat([p.R for p in params]...)
    A = pack3([p.A for p in params]); Q = pack3([p.Q for p in params]); P0 = pack3([p.P0 for p in params])
    mu0 = hcat([p.mu0 for p in params]...)
    np = div(r * (r + 1), 2)
    f = Array{Float64}(undef, r, T, B); P = Array{Float64}(undef, np, T, B); ll = Array{Float64}(undef, B)
    flags = any(isnan, panel) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)
    GC.@preserve panel Lam R A Q mu0 P0 f P ll begin
        if ngpu <= 1
            rc = ccall((:dfm_ks_pass_batch, LIB), Cint,
                       (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                        Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cuint),
                       h.ptr, B, T, N, r, panel, Lam, R, A, Q, mu0, P0, f, P, ll, flags)
            check(h.ptr, rc)
        else
            err = zeros(UInt8, 700)
            rc = ccall((:dfm_ks_pass_batch_multi, LIB), Cint,
                       (Cint, Ptr{Cint}, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                        Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cuint,
                        Ptr{UInt8}, Cint),
                       ngpu, C_NULL, B, T, N, r, panel, Lam, R, A, Q, mu0, P0, f, P, ll, flags, err, length(err))
            rc == 0 || error("libdfmhip: status $rc: $(unsafe_string(pointer(err)))")
        end
    end
    return (factor = unpack3(f), P = unpack3(P), loglik = ll)
end

# ---- the library's multi-GPU object (dfm_multi, csrc/multi.hip): per-GPU handles / streams / workspaces and ONE RCCL
# communicator, created once and cached per GPU count; a job's replicates stay resident on the GPUs between calls -------
mutable struct Multi
    ptr::Ptr{Cvoid}
    shape::NTuple{4,Int}      # (B, T, N, r) of the resident job
    max_iter::Int
end
const DFM_MULTI_F_FORCE_COMM = Cuint(1)
const MULTI_LAM, MULTI_R, MULTI_A, MULTI_Q, MULTI_MU0, MULTI_P0, MULTI_F_SMOOTH, MULTI_P_SMOOTH, MULTI_LOGLIK,
      MULTI_LOGLIK_PATH, MULTI_ITERS, MULTI_PANEL = Cint.(0:11)

function mcheck(m::Multi, rc::Cint)
    rc == 0 && return nothing
    error("libdfmhip: status $rc: " * unsafe_string(ccall((:dfm_multi_last_error, LIB), Cstring, (Ptr{Cvoid},), m.ptr)))
end

function multi_create(ngpu::Integer = 1; device_ids = nothing, force_comm::Bool = false)
    ref = Ref{Ptr{Cvoid}}(C_NULL); err = zeros(UInt8, 700)
    ids = device_ids === nothing ? Cint[] : Cint.(device_ids)
    GC.@preserve ids err begin
        rc = ccall((:dfm_multi_create, LIB), Cint, (Ref{Ptr{Cvoid}}, Cint, Ptr{Cint}, Cuint, Ptr{UInt8}, Cint),
                   ref, ngpu, device_ids === nothing ? Ptr{Cint}(C_NULL) : pointer(ids),
                   force_comm ? DFM_MULTI_F_FORCE_COMM : Cuint(0), err, length(err))
        rc == 0 || error("libdfmhip: dfm_multi_create: status $rc: $(unsafe_string(pointer(err)))")
    end
    m = Multi(ref[], (0, 0, 0, 0), 0)
    finalizer(x -> (x.ptr != C_NULL && ccall((:dfm_multi_destroy, LIB), Cint, (Ptr{Cvoid},), x.ptr); x.ptr = C_NULL), m)
    return m
end
const MULTIS = Dict{Int,Multi}()
function multi(ngpu::Integer = 1)
    m = get(MULTIS, Int(ngpu), nothing)
    (m === nothing || m.ptr == C_NULL) && (m = MULTIS[Int(ngpu)] = multi_create(ngpu))
    return m
end

"Upload a job: panel (N, T, B), Lam (r, N, B), R (N, B), A / Q / P0 (r, r, B), mu0 (r, B) -- the C layouts."
function multi_load(m::Multi, panel::Array{Float64,3}, Lam::Array{Float64,3}, R::Matrix{Float64}, A::Array{Float64,3},
                    Q::Array{Float64,3}, mu0::Matrix{Float64}, P0::Array{Float64,3})
    N, T, B = size(panel); r = size(Lam, 1)
    GC.@preserve panel Lam R A Q mu0 P0 begin
        mcheck(m, ccall((:dfm_multi_load, LIB), Cint,
                        (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), m.ptr, B, T, N, r, panel, Lam, R, A, Q, mu0, P0))
    end
    m.shape = (B, T, N, r)
    return m
end

"Generate a synthetic job where it lives (SURVEY 8(d) DGP): GPU g draws replicates first_replicate + [lo_g, hi_g); nothing
crosses PCIe (BASELINE configs[2]: 65 536 replicates).  pca_start: the PCA + OLS start instead of the DGP parameters."
function multi_synth(m::Multi, seed::Integer, first_replicate::Integer, B::Integer, T::Integer, N::Integer, r::Integer;
                     missing_prob::Real = 0.0, pca_start::Bool = false)
    mcheck(m, ccall((:dfm_multi_synth, LIB), Cint, (Ptr{Cvoid}, UInt64, Int64, Cint, Cint, Cint, Cint, Cdouble, Cint),
                    m.ptr, seed, first_replicate, B, T, N, r, missing_prob, pca_start ? 1 : 0))
    m.shape = (Int(B), Int(T), Int(N), Int(r))
    return m
end

function multi_ks_pass(m::Multi; want_P::Bool = true, flags::Cuint = Cuint(0))
    mcheck(m, ccall((:dfm_multi_ks_pass, LIB), Cint, (Ptr{Cvoid}, Cint, Cuint), m.ptr, want_P ? 1 : 0, flags))
end

"The EM loop on the resident job (one ncclAllGather of {loglik, active} per iteration); returns the iterations run."
function multi_em(m::Multi; max_iter::Integer = 50, tol::Real = 1e-6, want_smooth::Bool = false, want_P::Bool = false,
                  flags::Cuint = Cuint(0))
    ran = Ref{Cint}(0)
    m.max_iter = Int(max_iter)
    mcheck(m, ccall((:dfm_multi_em, LIB), Cint, (Ptr{Cvoid}, Cint, Cdouble, Cint, Cint, Cuint, Ptr{Cint}),
                    m.ptr, max_iter, tol, want_smooth ? 1 : 0, want_P ? 1 : 0, flags, ran))
    return Int(ran[])
end

"One resident array of the whole job in global replicate order, in its C layout (replicate index last in Julia)."
function multi_fetch(m::Multi, what::Cint)
    B, T, N, r = m.shape; np = div(r * (r + 1), 2)
    if what == MULTI_ITERS
        out = Array{Cint}(undef, B)
        GC.@preserve out mcheck(m, ccall((:dfm_multi_fetch, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), m.ptr, what, pointer(out)))
        return out
    end
    dims = what == MULTI_LAM ? (r, N, B) : what == MULTI_R ? (N, B) : what == MULTI_MU0 ? (r, B) :
           what == MULTI_F_SMOOTH ? (r, T, B) : what == MULTI_P_SMOOTH ? (np, T, B) : what == MULTI_LOGLIK ? (B,) :
           what == MULTI_LOGLIK_PATH ? (m.max_iter, B) : what == MULTI_PANEL ? (N, T, B) : (r, r, B)
    out = Array{Float64}(undef, dims...)
    GC.@preserve out mcheck(m, ccall((:dfm_multi_fetch, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), m.ptr, what, pointer(out)))
    return out
end

"EM for B replicates in ONE call on `ngpu` GPUs of this node: the cached multi-GPU object (one RCCL communicator per GPU
count for the whole session) -- replicates split over the GPUs, one host thread per GPU inside the library, ONE RCCL
all-gather of {loglik, active} after every EM iteration (SURVEY.md 8(e)).  panels[b]: T x N, starts[b] = (Lam, R, A, Q,
mu0, P0).  Returns the per-replicate estimates, log-likelihood paths and iteration counts."
function em_batch(panels::Vector{Matrix{Float64}}, starts::Vector; max_iter::Integer = 50, tol::Real = 1e-6,
                  ngpu::Integer = 1, want_smooth::Bool = false, singular_q::Bool = false)
    B = length(panels); T, N = size(panels[1]); r = size(starts[1].Lam, 2)
    panel = cat([permutedims(z, (2, 1)) for z in panels]...; dims = 3)
    Lam = pack3([p.Lam for p in starts]); R = hcat([p.R for p in starts]...)
    A = pack3([p.A for p in starts]); Q = pack3([p.Q for p in starts]); P0 = pack3([p.P0 for p in starts])
    mu0 = hcat([p.mu0 for p in starts]...)
    flags = (any(isnan, panel) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    m = multi_load(multi(ngpu), panel, Lam, R, A, Q, mu0, P0)
    ran = multi_em(m; max_iter = max_iter, tol = tol, want_smooth = want_smooth, want_P = want_smooth, flags = flags)
    path = multi_fetch(m, MULTI_LOGLIK_PATH); iters = multi_fetch(m, MULTI_ITERS)
    Rm = multi_fetch(m, MULTI_R); mu = multi_fetch(m, MULTI_MU0)
    return (Lam = unpack3(multi_fetch(m, MULTI_LAM)), R = [Rm[:, b] for b in 1:B], A = unpack3(multi_fetch(m, MULTI_A)),
            Q = unpack3(multi_fetch(m, MULTI_Q)), mu0 = [mu[:, b] for b in 1:B], P0 = unpack3(multi_fetch(m, MULTI_P0)),
            loglik = [path[1:iters[b], b] for b in 1:B], iters = Int.(iters), iterations = ran,
            factor = want_smooth ? unpack3(multi_fetch(m, MULTI_F_SMOOTH)) : nothing)
end

"EM for VAR(p) factor dynamics in companion form (dfm_em_varp_batch; include/dfm_hip.h): p.Avar is r x (r p) =
[A_1 .. A_p], p.mu0 / p.P0 the moments of z_0 = (f_0, .., f_{1-p})."
function em_varp(h::Handle, z::Matrix{Float64}, p, nlag::Integer; max_iter::Integer = 50, tol::Real = 1e-6,
                 singular_q::Bool = false)   # singular_q: the r x r block Q may be rank deficient (DFM_F_SINGULAR_Q)
    T, N = size(z); r = size(p.Lam, 2); k = r * nlag
    panel = to_c_panel(z)
    Lam = reshape(permutedims(p.Lam), r, N, 1); R = reshape(copy(p.R), N, 1)
    Avar = reshape(permutedims(p.Avar), k, r, 1); Q = reshape(permutedims(p.Q), r, r, 1)
    mu0 = reshape(copy(p.mu0), k, 1); P0 = reshape(permutedims(p.P0), k, k, 1)
    path = Array{Float64}(undef, max_iter, 1); iters = Array{Cint}(undef, 1)
    f = Array{Float64}(undef, r, T, 1); np = div(r * (r + 1), 2); P = Array{Float64}(undef, np, T, 1)
    flags = (any(isnan, z) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve panel Lam R Avar Q mu0 P0 path iters f P begin
        rc = ccall((:dfm_em_varp_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Cdouble, Ptr{Float64}, Ptr{Cint},
                    Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, T, N, r, nlag, panel, Lam, R, Avar, Q, mu0, P0, max_iter, tol, path, iters, f, P, flags)
        check(h.ptr, rc)
    end
    kk = Int(iters[1])
    return (Lam = permutedims(Lam[:, :, 1]), R = R[:, 1], A = permutedims(Avar[:, :, 1]), Q = permutedims(Q[:, :, 1]),
            mu0 = mu0[:, 1], P0 = permutedims(P0[:, :, 1]), loglik = path[1:kk, 1], iters = kk,
            factor = permutedims(f[:, :, 1]))
end

"Nowcasts and H-step forecasts of the panel (dfm_forecast_batch; include/dfm_hip.h): z is T x N (NaN = missing, standardised
as in the fit), params the fitted model (Lam N x r, R, A or Avar r x (r nlag), Q, mu0, P0 as `em` / `em_varp` return them);
mean / sd (length N, both or neither) put the outputs into data units.  Rows 1..T+H: x = observed cells as they are and
E[x_ti | X] elsewhere, xvar (0 on observed cells), common, factor (T+H x r), P (packed lower per row), loglik."
function forecast(h::Handle, z::Matrix{Float64}, params, H::Integer; nlag::Integer = 1, mean = nothing, sd = nothing,
                  singular_q::Bool = false)
    (mean === nothing) == (sd === nothing) || error("mean and sd go together")
    T, N = size(z); r = size(params.Lam, 2); k = r * nlag; TH = T + H
    Av = hasproperty(params, :Avar) ? params.Avar : params.A
    panel = to_c_panel(z)
    Lam = permutedims(params.Lam); R = copy(params.R); AC = permutedims(Av); QC = permutedims(params.Q)
    mu0 = copy(params.mu0); P0C = permutedims(params.P0)
    meanC = mean === nothing ? C_NULL : Vector{Float64}(mean); sdC = sd === nothing ? C_NULL : Vector{Float64}(sd)
    xhat = Array{Float64}(undef, N, TH); xvar = Array{Float64}(undef, N, TH); common = Array{Float64}(undef, N, TH)
    f = Array{Float64}(undef, r, TH); np = div(r * (r + 1), 2); P = Array{Float64}(undef, np, TH); ll = Array{Float64}(undef, 1)
    flags = (any(isnan, z) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve panel Lam R AC QC mu0 P0C meanC sdC xhat xvar common f P ll begin
        rc = ccall((:dfm_forecast_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, T, N, r, nlag, H, panel, Lam, R, AC, QC, mu0, P0C, meanC, sdC, xhat, xvar, common, f, P, ll, flags)
        check(h.ptr, rc)
    end
    return (x = permutedims(xhat), xvar = permutedims(xvar), common = permutedims(common), factor = permutedims(f),
            P = permutedims(P), loglik = ll[1])
end

# dfm_filter_batch for one replicate (include/dfm_hip.h); the parameters are held fixed over all origins.
function filter_call(h::Handle, z::Matrix{Float64}, params, H::Integer, t0::Integer; nlag::Integer = 1, mean = nothing, sd = nothing)
    (mean === nothing) == (sd === nothing) || error("mean and sd go together")
    T, N = size(z); r = size(params.Lam, 2); k = r * nlag; kk = div(k * (k + 1), 2)
    Av = hasproperty(params, :Avar) ? params.Avar : params.A
    panel = to_c_panel(z)
    Lam = permutedims(params.Lam); R = copy(params.R); AC = permutedims(Av); QC = permutedims(params.Q)
    mu0 = copy(params.mu0); P0C = permutedims(params.P0)
    meanC = mean === nothing ? C_NULL : Vector{Float64}(mean); sdC = sd === nothing ? C_NULL : Vector{Float64}(sd)
    zp = Array{Float64}(undef, k, T); Pp = Array{Float64}(undef, kk, T); zf = Array{Float64}(undef, k, T); Pf = Array{Float64}(undef, kk, T)
    ll = Array{Float64}(undef, T); xp = Array{Float64}(undef, N, T); ve = Array{Float64}(undef, N, T); vs = Array{Float64}(undef, N, T)
    ms = Array{Float64}(undef, N, H); m0 = Array{Float64}(undef, N, H); cnt = Array{Cint}(undef, N, H)
    flags = any(isnan, z) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)
    GC.@preserve panel Lam R AC QC mu0 P0C meanC sdC zp Pp zf Pf ll xp ve vs ms m0 cnt begin
        rc = ccall((:dfm_filter_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Cuint),
                   h.ptr, 1, T, N, r, nlag, H, t0, panel, Lam, R, AC, QC, mu0, P0C, meanC, sdC, zp, Pp, zf, Pf, ll, xp, ve, vs,
                   H > 0 ? ms : C_NULL, H > 0 ? m0 : C_NULL, H > 0 ? cnt : C_NULL, flags)
        check(h.ptr, rc)
    end
    return (zp = zp, Pp = Pp, zf = zf, Pf = Pf, ll = ll, xp = xp, ve = ve, vs = vs, ms = ms, m0 = m0, cnt = cnt)
end

"Predicted and filtered states, per-period log-likelihoods and one-step prediction errors (dfm_filter_batch; include/dfm_hip.h):
z, params, nlag, mean, sd as `forecast`.  Rows 1..T: state_pred / state_filt (T x r nlag), P_pred / P_filt (packed lower per row),
loglik_t, x_pred, error (data units) and error_std (NaN on missing cells)."
function filter_states(h::Handle, z::Matrix{Float64}, params; nlag::Integer = 1, mean = nothing, sd = nothing)
    o = filter_call(h, z, params, 0, 0; nlag = nlag, mean = mean, sd = sd)
    return (state_pred = permutedims(o.zp), P_pred = permutedims(o.Pp), state_filt = permutedims(o.zf), P_filt = permutedims(o.Pf),
            loglik_t = o.ll, x_pred = permutedims(o.xp), error = permutedims(o.ve), error_std = permutedims(o.vs))
end

"The pseudo-out-of-sample record with the fit held fixed (dfm_filter_batch; include/dfm_hip.h): origins first_origin..T-h (1-based
rows of z), horizons h = 1..H.  Returns msfe, rmsfe, relative (msfe over the unconditional-mean forecast's) and count, each H x N."
function evaluate_forecasts(h::Handle, z::Matrix{Float64}, params, H::Integer; first_origin::Integer = div(size(z, 1), 2) + 1,
                            nlag::Integer = 1, mean = nothing, sd = nothing)
    H >= 1 || error("H must be >= 1")
    o = filter_call(h, z, params, H, first_origin - 1; nlag = nlag, mean = mean, sd = sd)
    msfe = permutedims(o.ms)
    return (msfe = msfe, rmsfe = sqrt.(msfe), relative = msfe ./ permutedims(o.m0), count = permutedims(o.cnt))
end

"The rolling-window out-of-sample record, re-estimated at every origin (dfm_rolling_eval_batch; include/dfm_hip.h): x is the RAW
T x N panel (NaN = missing), origins increasing 1-based rows in W..T, lags the publication lags (length N) or nothing; start the
parameters every window's EM starts from (Lam N x r, R, A or Avar r x (r nlag), Q, mu0, P0 as `em` / `em_varp` return them), in the
units of sd_start (length N) or, with nothing, in each window's own.  max_iter = 0: no EM.  Returns forecast, variance, error,
error_std (O x (H+1) x N, horizons 0..H), msfe, rmsfe, relative, count ((H+1) x N), mean, sd (O x N), iters, loglik (O x max_iter) and
the windows' parameters Lam (O x N x r), R (O x N), A (O x r x r nlag), Q, mu0, P0."
function evaluate_forecasts_rolling(h::Handle, x::Matrix{Float64}, start, H::Integer, W::Integer, origins::AbstractVector{<:Integer};
                                    nlag::Integer = 1, lags = nothing, sd_start = nothing, min_obs::Integer = size(start.Lam, 2) + 1,
                                    max_iter::Integer = 50, tol::Real = 1e-6, singular_q::Bool = false)
    T, N = size(x); r = size(start.Lam, 2); k = r * nlag; O = length(origins); H1 = H + 1
    Av = hasproperty(start, :Avar) ? start.Avar : start.A
    panel = to_c_panel(x)
    org = Vector{Cint}(origins .- 1)
    lagC = lags === nothing ? C_NULL : Vector{Cint}(lags)
    Lam0 = permutedims(start.Lam); R0 = copy(start.R); A0 = permutedims(Av); Q0 = permutedims(start.Q)
    m0 = copy(start.mu0); P00 = permutedims(start.P0)
    sdC = sd_start === nothing ? C_NULL : Vector{Float64}(sd_start)
    Lam = Array{Float64}(undef, r, N, O); R = Array{Float64}(undef, N, O); A = Array{Float64}(undef, k, r, O)
    Q = Array{Float64}(undef, r, r, O); mu0 = Array{Float64}(undef, k, O); P0 = Array{Float64}(undef, k, k, O)
    path = Array{Float64}(undef, max(max_iter, 1), O); iters = Array{Cint}(undef, O)
    wm = Array{Float64}(undef, N, O); ws = Array{Float64}(undef, N, O); wn = Array{Cint}(undef, N, O)
    fc = Array{Float64}(undef, N, H1, O); fv = Array{Float64}(undef, N, H1, O); er = Array{Float64}(undef, N, H1, O)
    es = Array{Float64}(undef, N, H1, O); ms = Array{Float64}(undef, N, H1); ms0 = Array{Float64}(undef, N, H1); cnt = Array{Cint}(undef, N, H1)
    missing_cells = any(isnan, x) || (lags !== nothing && any(>(0), lags))
    flags = (missing_cells ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve panel org lagC Lam0 R0 A0 Q0 m0 P00 sdC Lam R A Q mu0 P0 path iters wm ws wn fc fv er es ms ms0 cnt begin
        rc = ccall((:dfm_rolling_eval_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Cint}, Ptr{Cint}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Cdouble, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Cint}, Cuint),
                   h.ptr, T, N, r, nlag, W, H, O, min_obs, 1, panel, org, lagC, Lam0, R0, A0, Q0, m0, P00, sdC, max_iter, tol, Lam, R, A, Q,
                   mu0, P0, max_iter > 0 ? path : C_NULL, iters, wm, ws, wn, C_NULL, fc, fv, er, es, ms, ms0, cnt, flags)
        check(h.ptr, rc)
    end
    msfe = permutedims(ms)
    return (forecast = permutedims(fc, (3, 2, 1)), variance = permutedims(fv, (3, 2, 1)), error = permutedims(er, (3, 2, 1)),
            error_std = permutedims(es, (3, 2, 1)), msfe = msfe, rmsfe = sqrt.(msfe), relative = msfe ./ permutedims(ms0),
            count = permutedims(cnt), mean = permutedims(wm), sd = permutedims(ws), iters = Vector{Int}(iters),
            loglik = permutedims(path)[:, 1:max_iter], Lam = permutedims(Lam, (3, 2, 1)), R = permutedims(R),
            A = permutedims(A, (3, 2, 1)), Q = permutedims(Q, (3, 2, 1)), mu0 = permutedims(mu0), P0 = permutedims(P0, (3, 2, 1)))
end

"Diffusion-index forecasts from the non-parametric fit, out of sample (dfm_diffusion_eval_batch; include/dfm_hip.h): x is the RAW
T x N panel (NaN = missing), origins increasing 1-based rows in W..T, lags the publication lags (length N) or nothing; F_start the
T x r factor path every window's ALS starts from (its rows of the window), q the number of own lags in the direct regressions.
max_iter = 0: the factors are the start.  Returns forecast, forecast_ar, variance, error, error_ar, error_std (O x (H+1) x N, horizons
0..H), msfe, msfe_ar, msfe_mean, count ((H+1) x N), factor (O x W x r), loadings (O x N x r), iters, ssr (O), mean, sd (O x N)."
function forecast_diffusion_index(h::Handle, x::Matrix{Float64}, F_start::Matrix{Float64}, H::Integer, W::Integer,
                                  origins::AbstractVector{<:Integer}; q::Integer = 4, lags = nothing,
                                  min_obs::Integer = size(F_start, 2) + 1, nt_min::Integer = 20, max_iter::Integer = 1000,
                                  tol::Real = 1e-8)
    T, N = size(x); r = size(F_start, 2); O = length(origins); H1 = H + 1
    size(F_start, 1) == T || error("F_start must have one row per row of x")
    panel = to_c_panel(x)
    org = Vector{Cint}(origins .- 1)
    lagC = lags === nothing ? C_NULL : Vector{Cint}(lags)
    F0 = permutedims(F_start)
    F = Array{Float64}(undef, r, W, O); Lam = Array{Float64}(undef, r, N, O); iters = Array{Cint}(undef, O); ssr = Array{Float64}(undef, O)
    wm = Array{Float64}(undef, N, O); ws = Array{Float64}(undef, N, O); wn = Array{Cint}(undef, N, O)
    fc = Array{Float64}(undef, N, H1, O); fa = Array{Float64}(undef, N, H1, O); fv = Array{Float64}(undef, N, H1, O)
    er = Array{Float64}(undef, N, H1, O); ea = Array{Float64}(undef, N, H1, O); es = Array{Float64}(undef, N, H1, O)
    ms = Array{Float64}(undef, N, H1); ma = Array{Float64}(undef, N, H1); ms0 = Array{Float64}(undef, N, H1); cnt = Array{Cint}(undef, N, H1)
    missing_cells = any(isnan, x) || (lags !== nothing && any(>(0), lags))
    flags = missing_cells ? DFM_F_MAY_HAVE_MISSING : Cuint(0)
    GC.@preserve panel org lagC F0 F Lam iters ssr wm ws wn fc fa fv er ea es ms ma ms0 cnt begin
        rc = ccall((:dfm_diffusion_eval_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Cint}, Ptr{Cint}, Ptr{Float64},
                    Cint, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Cuint),
                   h.ptr, T, N, r, q, W, H, O, min_obs, nt_min, 1, panel, org, lagC, F0, max_iter, tol, F, Lam, iters, ssr, wm, ws, wn, C_NULL,
                   fc, fa, fv, er, ea, es, C_NULL, C_NULL, ms, ma, ms0, cnt, flags)
        check(h.ptr, rc)
    end
    p3 = a -> permutedims(a, (3, 2, 1))
    return (forecast = p3(fc), forecast_ar = p3(fa), variance = p3(fv), error = p3(er), error_ar = p3(ea), error_std = p3(es),
            msfe = permutedims(ms), msfe_ar = permutedims(ma), msfe_mean = permutedims(ms0), count = permutedims(cnt),
            factor = p3(F), loadings = p3(Lam), iters = Vector{Int}(iters), ssr = ssr, mean = permutedims(wm), sd = permutedims(ws))
end

"Identified impulse responses and forecast-error variance shares of every series (dfm_irf_batch; include/dfm_hip.h): params as
`forecast`; named = r distinct series (1-based; factor k is the common component of series named[k], their order the recursive
ordering) or nothing (S = chol Q); cumulate = series (1-based) whose responses are cumulated; sd (length N) puts the responses
into data units.  Returns irf (N x H x r: series, horizon, shock) and fevd (N x H x (r+1), the last slot idiosyncratic)."
function structural_irf(h::Handle, params, H::Integer; nlag::Integer = 1, named = nothing, cumulate = nothing, sd = nothing,
                        unit_effect::Bool = false)
    N, r = size(params.Lam)
    Av = hasproperty(params, :Avar) ? params.Avar : params.A
    Lam = permutedims(params.Lam); R = copy(params.R); AC = permutedims(Av); QC = permutedims(params.Q)
    sdC = sd === nothing ? C_NULL : Vector{Float64}(sd)
    namedC = named === nothing ? C_NULL : Vector{Cint}(named .- 1)
    cumC = C_NULL
    if cumulate !== nothing
        cumC = zeros(Cint, N); cumC[cumulate] .= 1
    end
    irf = Array{Float64}(undef, N, H, r); fevd = Array{Float64}(undef, N, H, r + 1)
    flags = unit_effect ? DFM_SV_UNIT_EFFECT : Cuint(0)
    GC.@preserve Lam R AC QC sdC namedC cumC irf fevd begin
        rc = ccall((:dfm_irf_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Cint}, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, N, r, nlag, H, Lam, AC, QC, R, sdC, namedC, cumC, irf, fevd, flags)
        check(h.ptr, rc)
    end
    return (irf = irf, fevd = fevd)              # the C layout [k][h][i] is column-major N x H x r as it stands
end

"Impulse responses identified by sign restrictions (dfm_signirf_batch; include/dfm_hip.h): params, nlag, named, cumulate, sd as
`structural_irf`; restrictions = rows (series, shock, h0, h1, sign) with series and shock 1-based and horizons 0-based (0 = impact);
`candidates` Haar rotations of the base impact matrix are drawn on the GPU from `seed` (candidates first_cand, first_cand + 1, ..),
the first `keep` accepted ones are returned.  Returns n_accept, mask (candidates), cand (keep; 0-based candidate index, -1 = empty
slot), impact (r x r x keep), irf (N x H x r x keep) and fevd (N x H x (r+1) x keep); empty slots hold NaN."
function structural_irf_signs(h::Handle, params, H::Integer, restrictions; candidates::Integer = 1000, keep::Integer = 1,
                              nlag::Integer = 1, named = nothing, cumulate = nothing, sd = nothing, seed::Integer = 20160415,
                              first_cand::Integer = 0)
    N, r = size(params.Lam)
    Av = hasproperty(params, :Avar) ? params.Avar : params.A
    Lam = permutedims(params.Lam); R = copy(params.R); AC = permutedims(Av); QC = permutedims(params.Q)
    sdC = sd === nothing ? C_NULL : Vector{Float64}(sd)
    namedC = named === nothing ? C_NULL : Vector{Cint}(named .- 1)
    cumC = C_NULL
    if cumulate !== nothing
        cumC = zeros(Cint, N); cumC[cumulate] .= 1
    end
    G = length(restrictions)
    restrC = G == 0 ? C_NULL : Matrix{Cint}(undef, 5, G)         # column g = row g of the C array [G][5]
    for (g, q) in enumerate(restrictions)
        restrC[:, g] .= (q[1] - 1, q[2] - 1, q[3], q[4], q[5])
    end
    M = Int(candidates); K = Int(keep)
    nacc = Vector{Cint}(undef, 1); mask = Vector{Cint}(undef, M); cand = Vector{Cint}(undef, K)
    S = Array{Float64}(undef, r, r, K); irf = Array{Float64}(undef, N, H, r, K); fevd = Array{Float64}(undef, N, H, r + 1, K)
    GC.@preserve Lam R AC QC sdC namedC cumC restrC nacc mask cand S irf fevd begin
        rc = ccall((:dfm_signirf_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Cint}, Ptr{Cint}, Cint, Ptr{Cint}, Cint, Cint, UInt64, Int64, Ptr{Cint}, Ptr{Cint},
                    Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, N, r, nlag, H, Lam, AC, QC, R, sdC, namedC, cumC, G, restrC, M, K, UInt64(seed), Int64(first_cand),
                   nacc, mask, cand, S, irf, fevd, Cuint(0))
        check(h.ptr, rc)
    end
    # the C layouts [s][i][k] and [s][k][h][i] are column-major (k, i, s) and (i, h, k, s): the impact matrices are transposed back
    return (n_accept = Int(nacc[1]), mask = mask, cand = cand, impact = permutedims(S, (2, 1, 3)), irf = irf, fevd = fevd)
end

"Impulse responses to one shock identified by an external instrument (dfm_proxyirf_batch; include/dfm_hip.h): z, params, nlag,
sd, singular_q as `historical_decomposition`, cumulate as `structural_irf`; instrument = one entry per row of z, NaN where it does
not exist; norm = the series (1-based) whose impact response is made non-negative (exactly 1 with unit_effect); draws moving block
draws of the instrument moment with blocks of `block` usable periods (default ceil(n^(1/3))), a pure function of (seed,
first_draw + draw index).  Slot 1 is the sample, slots 2 .. draws + 1 the block draws.  Returns impact (r x (draws+1)), relevance
(draws+1), irf and fevd (N x H x (draws+1)), shock (T), factor (T x r) and loglik."
function structural_irf_proxy(h::Handle, z::Matrix{Float64}, params, H::Integer, instrument; norm::Integer, draws::Integer = 0,
                              block = nothing, nlag::Integer = 1, cumulate = nothing, sd = nothing, unit_effect::Bool = false,
                              seed::Integer = 20160415, first_draw::Integer = 0, singular_q::Bool = false)
    T, N = size(z); r = size(params.Lam, 2)
    length(instrument) == T || error("the instrument must have one entry per row of z")
    Av = hasproperty(params, :Avar) ? params.Avar : params.A
    panel = to_c_panel(z)
    Lam = permutedims(params.Lam); R = copy(params.R); AC = permutedims(Av); QC = permutedims(params.Q)
    mu0 = copy(params.mu0); P0C = permutedims(params.P0)
    sdC = sd === nothing ? C_NULL : Vector{Float64}(sd)
    cumC = C_NULL
    if cumulate !== nothing
        cumC = zeros(Cint, N); cumC[cumulate] .= 1
    end
    zC = Vector{Float64}(instrument)
    n = count(isfinite, zC[nlag + 1:end])
    L = block === nothing ? max(1, ceil(Int, n^(1 / 3) - 1e-12)) : Int(block)
    D1 = Int(draws) + 1
    impact = Array{Float64}(undef, r, D1); rel = Vector{Float64}(undef, D1)
    irf = Array{Float64}(undef, N, H, D1); fevd = Array{Float64}(undef, N, H, D1)
    u = Vector{Float64}(undef, T); f = Array{Float64}(undef, r, T); ll = Array{Float64}(undef, 1)
    flags = (any(isnan, z) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0)) |
            (unit_effect ? DFM_SV_UNIT_EFFECT : Cuint(0))
    GC.@preserve panel Lam R AC QC mu0 P0C sdC cumC zC impact rel irf fevd u f ll begin
        rc = ccall((:dfm_proxyirf_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ptr{Float64}, Cint, Cint, Cint, UInt64,
                    Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Cuint),
                   h.ptr, 1, T, N, r, nlag, H, panel, Lam, R, AC, QC, mu0, P0C, sdC, cumC, zC, norm - 1, Int(draws), L,
                   UInt64(seed), Int64(first_draw), impact, rel, irf, fevd, u, f, ll, flags)
        check(h.ptr, rc)
    end
    # the C layouts [s][c] and [s][h][i] are column-major (c, s) and (i, h, s) as they stand
    return (impact = impact, relevance = rel, irf = irf, fevd = fevd, shock = u, factor = permutedims(f), loglik = ll[1])
end

"Historical decomposition (dfm_histdecomp_batch; include/dfm_hip.h): z, params, nlag, sd, singular_q as `forecast`, named as
`structural_irf`.  Returns contributions (T x N x (r+1): the last slot is the initial condition), shocks (T x r), factor
(T x r) and loglik."
function historical_decomposition(h::Handle, z::Matrix{Float64}, params; nlag::Integer = 1, named = nothing, sd = nothing,
                                  singular_q::Bool = false)
    T, N = size(z); r = size(params.Lam, 2)
    Av = hasproperty(params, :Avar) ? params.Avar : params.A
    panel = to_c_panel(z)
    Lam = permutedims(params.Lam); R = copy(params.R); AC = permutedims(Av); QC = permutedims(params.Q)
    mu0 = copy(params.mu0); P0C = permutedims(params.P0)
    sdC = sd === nothing ? C_NULL : Vector{Float64}(sd)
    namedC = named === nothing ? C_NULL : Vector{Cint}(named .- 1)
    hd = Array{Float64}(undef, N, T, r + 1); u = Array{Float64}(undef, r, T); f = Array{Float64}(undef, r, T)
    ll = Array{Float64}(undef, 1)
    flags = (any(isnan, z) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve panel Lam R AC QC mu0 P0C sdC namedC hd u f ll begin
        rc = ccall((:dfm_histdecomp_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, T, N, r, nlag, panel, Lam, R, AC, QC, mu0, P0C, sdC, namedC, hd, u, f, ll, flags)
        check(h.ptr, rc)
    end
    return (contributions = permutedims(hd, (2, 1, 3)), shocks = permutedims(u), factor = permutedims(f), loglik = ll[1])
end

"Joint posterior draws of the factor path and of the missing / future cells (dfm_simsmooth_batch; include/dfm_hip.h): z, params,
nlag, mean / sd as `forecast`; ndraws exact, independent draws over rows 1..T+H by the simulation smoother, a pure function of
(seed, first_draw + draw index).  Returns factor (ndraws x (T+H) x r) and x (ndraws x (T+H) x N: observed cells as given)."
function draw_paths(h::Handle, z::Matrix{Float64}, params, ndraws::Integer, H::Integer = 0; nlag::Integer = 1,
                    seed::Integer = 20160415, first_draw::Integer = 0, mean = nothing, sd = nothing,
                    singular_q::Bool = false)
    (mean === nothing) == (sd === nothing) || error("mean and sd go together")
    T, N = size(z); r = size(params.Lam, 2); TH = T + H
    Av = hasproperty(params, :Avar) ? params.Avar : params.A
    panel = to_c_panel(z)
    Lam = permutedims(params.Lam); R = copy(params.R); AC = permutedims(Av); QC = permutedims(params.Q)
    mu0 = copy(params.mu0); P0C = permutedims(params.P0)
    meanC = mean === nothing ? C_NULL : Vector{Float64}(mean); sdC = sd === nothing ? C_NULL : Vector{Float64}(sd)
    f = Array{Float64}(undef, r, TH, ndraws); x = Array{Float64}(undef, N, TH, ndraws)
    flags = (any(isnan, z) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve panel Lam R AC QC mu0 P0C meanC sdC f x begin
        rc = ccall((:dfm_simsmooth_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, UInt64, Int64,
                    Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, ndraws, T, N, r, nlag, H, panel, Lam, R, AC, QC, mu0, P0C, meanC, sdC, UInt64(seed),
                   Int64(first_draw), f, x, flags)
        check(h.ptr, rc)
    end
    return (factor = permutedims(f, (3, 2, 1)), x = permutedims(x, (3, 2, 1)))
end

"Bayesian estimation by the Gibbs sampler (dfm_gibbs_batch; include/dfm_hip.h): z, params, nlag as `forecast`; `chains` chains
start at params, run `burn` sweeps and keep `ndraws` sweeps each, one in `thin`.  prior = (tau_lam, nu_R, s_R, tau_A, nu_Q, s_Q)
with A0 (r x r nlag, the prior mean of [A_1 .. A_p]) or nothing for zero.  mu0 and P0 stay fixed.  Returns the kept draws with
chains x ndraws on the first axis (chain-major): Lam (. x N x r), R (. x N), A (. x r x r nlag), Q (. x r x r), factor (. x T x r).
Lam, A and Q are not identified one by one (no rotation or scale normalisation): use them through the common component,
forecasts or named-factor IRFs."
function estimate_bayesian(h::Handle, z::Matrix{Float64}, params, ndraws::Integer; nlag::Integer = 1, chains::Integer = 4,
                           burn::Integer = 500, thin::Integer = 1, seed::Integer = 20160415, first_sweep::Integer = 0,
                           prior = (tau_lam = 1.0, nu_R = 4.0, s_R = 0.25, tau_A = 1.0, nu_Q = size(params.Lam, 2) + 2.0, s_Q = 0.5),
                           A0 = nothing, singular_q::Bool = false)
    T, N = size(z); r = size(params.Lam, 2); k = r * nlag; B = Int(chains); K = Int(ndraws)
    Av = hasproperty(params, :Avar) ? params.Avar : params.A
    rep(a) = repeat(a, outer = (ntuple(_ -> 1, ndims(a))..., B))
    panel = rep(to_c_panel(z)[:, :, 1])
    Lam = rep(permutedims(params.Lam)); R = rep(copy(params.R)); AC = rep(permutedims(Av)); QC = rep(permutedims(params.Q))
    mu0 = rep(copy(params.mu0)); P0C = rep(permutedims(params.P0))
    A0C = A0 === nothing ? C_NULL : rep(permutedims(Matrix{Float64}(A0)))
    n_sweeps = burn + (K - 1) * thin + 1
    Ld = Array{Float64}(undef, r, N, K, B); Rd = Array{Float64}(undef, N, K, B); Ad = Array{Float64}(undef, k, r, K, B)
    Qd = Array{Float64}(undef, r, r, K, B); fd = Array{Float64}(undef, r, T, K, B)
    flags = (any(isnan, z) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve panel Lam R AC QC mu0 P0C A0C Ld Rd Ad Qd fd begin
        rc = ccall((:dfm_gibbs_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cdouble, Cdouble, Cdouble, Cdouble, Ptr{Float64}, Cint, Cint,
                    Cint, UInt64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, B, T, N, r, nlag, panel, mu0, P0C, Lam, R, AC, QC, prior.tau_lam, prior.nu_R, prior.s_R, prior.tau_A,
                   prior.nu_Q, prior.s_Q, A0C, n_sweeps, burn, thin, UInt64(seed), Int64(first_sweep), Ld, Rd, Ad, Qd, fd, flags)
        check(h.ptr, rc)
    end
    flat(a, perm) = (p = permutedims(a, perm); reshape(permutedims(p, (2, 1, 3:ndims(p)...)), :, size(p)[3:end]...))
    return (Lam = flat(Ld, (4, 3, 2, 1)), R = flat(Rd, (3, 2, 1)), A = flat(Ad, (4, 3, 2, 1)), Q = flat(Qd, (4, 3, 2, 1)),
            factor = flat(fd, (4, 3, 2, 1)))
end

"Bayesian estimation of the model with AR(q) idiosyncratic terms by its Gibbs sampler (dfm_gibbs_ar_batch; include/dfm_hip.h):
z is T x N (NaN = missing, in deviations from the series means), params has Lam (N x r), sig2 (N), rho (N x q), Avar (r x r nlag),
Q, mu0 (r m) and P0 (r m x r m), m = max(nlag, q + 1), as the AR pass takes them.  `chains` chains start at params, run `burn`
sweeps and keep `ndraws` sweeps each, one in `thin`.  prior = (tau_lam, nu_R, s_R, tau_rho, tau_A, nu_Q, s_Q) with A0 or nothing.
Returns the kept draws with chains x ndraws on the first axis (chain-major): Lam, sig2, rho (. x N x q), A, Q and factor
(. x T - q x r).  rho, sig2, the common component and forecasts are identified; Lam, A and Q one by one are not."
function estimate_bayesian_ar(h::Handle, z::Matrix{Float64}, params, ndraws::Integer; nlag::Integer = 1, chains::Integer = 4,
                              burn::Integer = 500, thin::Integer = 1, seed::Integer = 20160415, first_sweep::Integer = 0,
                              prior = (tau_lam = 1.0, nu_R = 4.0, s_R = 0.25, tau_rho = 4.0, tau_A = 1.0,
                                       nu_Q = size(params.Lam, 2) + 2.0, s_Q = 0.5),
                              A0 = nothing, singular_q::Bool = false)
    T, N = size(z); r = size(params.Lam, 2); q = size(params.rho, 2); k = r * nlag; B = Int(chains); K = Int(ndraws); n = T - q
    rep(a) = repeat(a, outer = (ntuple(_ -> 1, ndims(a))..., B))
    panel = rep(to_c_panel(z)[:, :, 1])
    Lam = rep(permutedims(params.Lam)); S2 = rep(copy(params.sig2)); Rho = rep(permutedims(params.rho))
    AC = rep(permutedims(params.Avar)); QC = rep(permutedims(params.Q)); mu0 = rep(copy(params.mu0)); P0C = rep(permutedims(params.P0))
    A0C = A0 === nothing ? C_NULL : rep(permutedims(Matrix{Float64}(A0)))
    n_sweeps = burn + (K - 1) * thin + 1
    Ld = Array{Float64}(undef, r, N, K, B); Sd = Array{Float64}(undef, N, K, B); Rd = Array{Float64}(undef, q, N, K, B)
    Ad = Array{Float64}(undef, k, r, K, B); Qd = Array{Float64}(undef, r, r, K, B); fd = Array{Float64}(undef, r, n, K, B)
    flags = (any(isnan, z) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve panel Lam S2 Rho AC QC mu0 P0C A0C Ld Sd Rd Ad Qd fd begin
        rc = ccall((:dfm_gibbs_ar_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cdouble, Cdouble, Cdouble, Cdouble, Cdouble,
                    Ptr{Float64}, Cint, Cint, Cint, UInt64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, B, T, N, r, nlag, q, panel, mu0, P0C, Lam, S2, Rho, AC, QC, prior.tau_lam, prior.nu_R, prior.s_R,
                   prior.tau_rho, prior.tau_A, prior.nu_Q, prior.s_Q, A0C, n_sweeps, burn, thin, UInt64(seed), Int64(first_sweep),
                   Ld, Sd, Rd, Ad, Qd, fd, flags)
        check(h.ptr, rc)
    end
    flat(a, perm) = (p = permutedims(a, perm); reshape(permutedims(p, (2, 1, 3:ndims(p)...)), :, size(p)[3:end]...))
    return (Lam = flat(Ld, (4, 3, 2, 1)), sig2 = flat(Sd, (3, 2, 1)), rho = flat(Rd, (4, 3, 2, 1)), A = flat(Ad, (4, 3, 2, 1)),
            Q = flat(Qd, (4, 3, 2, 1)), factor = flat(fd, (4, 3, 2, 1)))
end

"News decomposition of the revision of G target cells between two vintages (dfm_news_batch; include/dfm_hip.h): zold / znew
are T x N (NaN = missing, standardised; every cell of zold observed in znew), params, nlag, mean / sd as `forecast`; targets =
G (row, column) pairs, 1-based, rows past T are forecasts.  Returns yhat (3 x G: old, revised old, new), impact (G x N), news
(T x N) and weight (G x T x N), in data units with mean / sd."
function news(h::Handle, zold::Matrix{Float64}, znew::Matrix{Float64}, params, targets; nlag::Integer = 1, mean = nothing,
              sd = nothing, singular_q::Bool = false)
    (mean === nothing) == (sd === nothing) || error("mean and sd go together")
    size(zold) == size(znew) || error("zold and znew must have the same size")
    T, N = size(znew); r = size(params.Lam, 2); G = length(targets)
    Av = hasproperty(params, :Avar) ? params.Avar : params.A
    po = to_c_panel(zold); pn = to_c_panel(znew)
    Lam = permutedims(params.Lam); R = copy(params.R); AC = permutedims(Av); QC = permutedims(params.Q)
    mu0 = copy(params.mu0); P0C = permutedims(params.P0)
    meanC = mean === nothing ? C_NULL : Vector{Float64}(mean); sdC = sd === nothing ? C_NULL : Vector{Float64}(sd)
    tt = Cint[t - 1 for (t, _) in targets]; ti = Cint[i - 1 for (_, i) in targets]
    yhat = Array{Float64}(undef, G, 3); impact = Array{Float64}(undef, N, G); nw = Array{Float64}(undef, N, T)
    w = Array{Float64}(undef, N, T, G)
    flags = (any(isnan, znew) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve po pn Lam R AC QC mu0 P0C meanC sdC tt ti yhat impact nw w begin
        rc = ccall((:dfm_news_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Cint},
                    Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, T, N, r, nlag, po, pn, Lam, R, AC, QC, mu0, P0C, meanC, sdC, G, tt, ti, yhat, impact, nw, w, flags)
        check(h.ptr, rc)
    end
    return (yhat = permutedims(yhat), impact = permutedims(impact), news = permutedims(nw), weight = permutedims(w, (3, 2, 1)))
end

"Smoother pass with AR(q) idiosyncratic terms (dfm_ks_pass_ar_batch; include/dfm_hip.h): x is T x N (NaN = missing, in
deviations from its intercept), Lam N x r, sig2 = uar_ser.^2, rho = uar_coef (N x q), Avar r x (r p), Q r x r, mu0 / P0
the moments of z_q, r max(p, q+1) wide.  Returns the smoothed factors of rows q+1..T and the conditional log-likelihood."
function ks_pass_ar(h::Handle, x::Matrix{Float64}, Lam::Matrix{Float64}, sig2::Vector{Float64}, rho::Matrix{Float64},
                    Avar::Matrix{Float64}, Q::Matrix{Float64}, mu0::Vector{Float64}, P0::Matrix{Float64};
                    singular_q::Bool = false)
    T, N = size(x); r = size(Lam, 2); q = size(rho, 2); p = div(size(Avar, 2), r)
    panel = to_c_panel(x)
    LamC = permutedims(Lam); rhoC = permutedims(rho); AC = permutedims(Avar); QC = permutedims(Q); P0C = permutedims(P0)
    f = Array{Float64}(undef, r, T - q); np = div(r * (r + 1), 2); P = Array{Float64}(undef, np, T - q)
    ll = Array{Float64}(undef, 1)
    flags = (any(isnan, x) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve panel LamC sig2 rhoC AC QC mu0 P0C f P ll begin
        rc = ccall((:dfm_ks_pass_ar_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, T, N, r, p, q, panel, LamC, sig2, rhoC, AC, QC, mu0, P0C, f, P, ll, flags)
        check(h.ptr, rc)
    end
    return (factor = permutedims(f), P = permutedims(P), loglik = ll[1])
end

"Nowcasts and H-step forecasts of the panel with AR(q) idiosyncratic terms (dfm_forecast_ar_batch; include/dfm_hip.h): arguments
as ks_pass_ar (1 <= q <= 4); v0 (length N, default sig2) is the variance of the q idiosyncratic terms before the first output row,
mean / sd (length N, both or neither) put the cells into data units.  Rows q+1..T+H: x = observed cells as they are and
E[x_ti | X] = common + idio elsewhere, xvar (0 on observed cells; the factor and idiosyncratic variances added, not exact), common,
idio, factor (T+H-q x r), P (packed lower per row), loglik (conditional on the first q rows)."
function forecast_ar(h::Handle, x::Matrix{Float64}, Lam::Matrix{Float64}, sig2::Vector{Float64}, rho::Matrix{Float64},
                     Avar::Matrix{Float64}, Q::Matrix{Float64}, mu0::Vector{Float64}, P0::Matrix{Float64}, H::Integer;
                     v0 = nothing, mean = nothing, sd = nothing, singular_q::Bool = false)
    (mean === nothing) == (sd === nothing) || error("mean and sd go together")
    T, N = size(x); r = size(Lam, 2); q = size(rho, 2); p = div(size(Avar, 2), r); n = T + H - q
    panel = to_c_panel(x)
    LamC = permutedims(Lam); rhoC = permutedims(rho); AC = permutedims(Avar); QC = permutedims(Q); P0C = permutedims(P0)
    v0C = v0 === nothing ? C_NULL : Vector{Float64}(v0)
    meanC = mean === nothing ? C_NULL : Vector{Float64}(mean); sdC = sd === nothing ? C_NULL : Vector{Float64}(sd)
    xhat = Array{Float64}(undef, N, n); xvar = Array{Float64}(undef, N, n); common = Array{Float64}(undef, N, n)
    idio = Array{Float64}(undef, N, n)
    f = Array{Float64}(undef, r, n); np = div(r * (r + 1), 2); P = Array{Float64}(undef, np, n); ll = Array{Float64}(undef, 1)
    flags = (any(isnan, x) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve panel LamC sig2 rhoC AC QC mu0 P0C v0C meanC sdC xhat xvar common idio f P ll begin
        rc = ccall((:dfm_forecast_ar_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, T, N, r, p, q, H, panel, LamC, sig2, rhoC, AC, QC, mu0, P0C, v0C, meanC, sdC, xhat, xvar, common, idio,
                   f, P, ll, flags)
        check(h.ptr, rc)
    end
    return (x = permutedims(xhat), xvar = permutedims(xvar), common = permutedims(common), idio = permutedims(idio),
            factor = permutedims(f), P = permutedims(P), loglik = ll[1])
end

"News decomposition of the revision of G target cells between two vintages under the model with AR(q) idiosyncratic terms
(dfm_news_ar_batch; include/dfm_hip.h): xold / xnew are T x N (NaN = missing) and EDGE-SHAPED -- each series observed on rows
1..L with no gap, L >= 2q in xold, every cell of xold observed in xnew; anything else is DFM_E_VINTAGE.  Parameters, v0, mean / sd
as forecast_ar; targets = G (row, column) pairs, 1-based, row > q, rows past T are forecasts.  Returns yhat (3 x G: old, revised
old, new), impact (G x N), news (T-q x N) and weight (G x T-q x N) over rows q+1..T, in data units with mean / sd."
function news_ar(h::Handle, xold::Matrix{Float64}, xnew::Matrix{Float64}, Lam::Matrix{Float64}, sig2::Vector{Float64},
                 rho::Matrix{Float64}, Avar::Matrix{Float64}, Q::Matrix{Float64}, mu0::Vector{Float64}, P0::Matrix{Float64},
                 targets; v0 = nothing, mean = nothing, sd = nothing, singular_q::Bool = false)
    (mean === nothing) == (sd === nothing) || error("mean and sd go together")
    size(xold) == size(xnew) || error("xold and xnew must have the same size")
    T, N = size(xnew); r = size(Lam, 2); q = size(rho, 2); p = div(size(Avar, 2), r); G = length(targets); ns = T - q
    po = to_c_panel(xold); pn = to_c_panel(xnew)
    LamC = permutedims(Lam); rhoC = permutedims(rho); AC = permutedims(Avar); QC = permutedims(Q); P0C = permutedims(P0)
    v0C = v0 === nothing ? C_NULL : Vector{Float64}(v0)
    meanC = mean === nothing ? C_NULL : Vector{Float64}(mean); sdC = sd === nothing ? C_NULL : Vector{Float64}(sd)
    tt = Cint[t - 1 for (t, _) in targets]; ti = Cint[i - 1 for (_, i) in targets]
    yhat = Array{Float64}(undef, G, 3); impact = Array{Float64}(undef, N, G); nw = Array{Float64}(undef, N, ns)
    w = Array{Float64}(undef, N, ns, G)
    flags = (any(isnan, xnew) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve po pn LamC sig2 rhoC AC QC mu0 P0C v0C meanC sdC tt ti yhat impact nw w begin
        rc = ccall((:dfm_news_ar_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, T, N, r, p, q, po, pn, LamC, sig2, rhoC, AC, QC, mu0, P0C, v0C, meanC, sdC, G, tt, ti, yhat, impact, nw,
                   w, flags)
        check(h.ptr, rc)
    end
    return (yhat = permutedims(yhat), impact = permutedims(impact), news = permutedims(nw), weight = permutedims(w, (3, 2, 1)))
end

# dfm_filter_ar_batch for one replicate (include/dfm_hip.h); the parameters are held fixed over all origins.  t0: a 0-based panel row.
function filter_ar_call(h::Handle, x::Matrix{Float64}, Lam::Matrix{Float64}, sig2::Vector{Float64}, rho::Matrix{Float64},
                        Avar::Matrix{Float64}, Q::Matrix{Float64}, mu0::Vector{Float64}, P0::Matrix{Float64}, H::Integer, t0::Integer;
                        mean = nothing, sd = nothing, singular_q::Bool = false)
    (mean === nothing) == (sd === nothing) || error("mean and sd go together")
    T, N = size(x); r = size(Lam, 2); q = size(rho, 2); p = div(size(Avar, 2), r); n = T - q
    k = r * max(p, q + 1); kk = div(k * (k + 1), 2)
    panel = to_c_panel(x)
    LamC = permutedims(Lam); rhoC = permutedims(rho); AC = permutedims(Avar); QC = permutedims(Q); P0C = permutedims(P0)
    meanC = mean === nothing ? C_NULL : Vector{Float64}(mean); sdC = sd === nothing ? C_NULL : Vector{Float64}(sd)
    zp = Array{Float64}(undef, k, n); Pp = Array{Float64}(undef, kk, n); zf = Array{Float64}(undef, k, n); Pf = Array{Float64}(undef, kk, n)
    ll = Array{Float64}(undef, n); xp = Array{Float64}(undef, N, n); ve = Array{Float64}(undef, N, n); vs = Array{Float64}(undef, N, n)
    ms = Array{Float64}(undef, N, H); mc = Array{Float64}(undef, N, H); m0 = Array{Float64}(undef, N, H); cnt = Array{Cint}(undef, N, H)
    flags = (any(isnan, x) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve panel LamC sig2 rhoC AC QC mu0 P0C meanC sdC zp Pp zf Pf ll xp ve vs ms mc m0 cnt begin
        rc = ccall((:dfm_filter_ar_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Cint}, Cuint),
                   h.ptr, 1, T, N, r, p, q, H, t0, panel, LamC, sig2, rhoC, AC, QC, mu0, P0C, meanC, sdC, zp, Pp, zf, Pf, ll, xp, ve, vs,
                   H > 0 ? ms : C_NULL, H > 0 ? mc : C_NULL, H > 0 ? m0 : C_NULL, H > 0 ? cnt : C_NULL, flags)
        check(h.ptr, rc)
    end
    return (zp = zp, Pp = Pp, zf = zf, Pf = Pf, ll = ll, xp = xp, ve = ve, vs = vs, ms = ms, mc = mc, m0 = m0, cnt = cnt)
end

"Predicted and filtered states, per-period log-likelihoods and one-step prediction errors of the model with AR(q) idiosyncratic
terms (dfm_filter_ar_batch; include/dfm_hip.h): arguments as forecast_ar.  Rows q+1..T: state_pred / state_filt (T-q x r max(p, q+1)),
P_pred / P_filt (packed lower per row), loglik_t (its sum is ks_pass_ar's loglik), x_pred (NaN where a lag is missing), error (data
units) and error_std (NaN where the cell or one of its q lags is missing)."
function filter_ar(h::Handle, x::Matrix{Float64}, Lam::Matrix{Float64}, sig2::Vector{Float64}, rho::Matrix{Float64},
                   Avar::Matrix{Float64}, Q::Matrix{Float64}, mu0::Vector{Float64}, P0::Matrix{Float64};
                   mean = nothing, sd = nothing, singular_q::Bool = false)
    o = filter_ar_call(h, x, Lam, sig2, rho, Avar, Q, mu0, P0, 0, size(rho, 2); mean = mean, sd = sd, singular_q = singular_q)
    return (state_pred = permutedims(o.zp), P_pred = permutedims(o.Pp), state_filt = permutedims(o.zf), P_filt = permutedims(o.Pf),
            loglik_t = o.ll, x_pred = permutedims(o.xp), error = permutedims(o.ve), error_std = permutedims(o.vs))
end

"The pseudo-out-of-sample record of the model with AR(q) idiosyncratic terms, the fit held fixed (dfm_filter_ar_batch;
include/dfm_hip.h): origins first_origin..T-h (1-based rows of x, first_origin > q) whose last q cells and target are observed,
horizons h = 1..H.  Returns msfe, rmsfe, msfe_common (the factor-only forecast from the same state), gain (msfe ./ msfe_common),
relative (msfe over the unconditional-mean forecast's) and count, each H x N."
function evaluate_forecasts_ar(h::Handle, x::Matrix{Float64}, Lam::Matrix{Float64}, sig2::Vector{Float64}, rho::Matrix{Float64},
                               Avar::Matrix{Float64}, Q::Matrix{Float64}, mu0::Vector{Float64}, P0::Matrix{Float64}, H::Integer;
                               first_origin::Integer = size(rho, 2) + div(size(x, 1) - size(rho, 2), 2) + 1,
                               mean = nothing, sd = nothing, singular_q::Bool = false)
    H >= 1 || error("H must be >= 1")
    o = filter_ar_call(h, x, Lam, sig2, rho, Avar, Q, mu0, P0, H, first_origin - 1; mean = mean, sd = sd, singular_q = singular_q)
    msfe = permutedims(o.ms); msfec = permutedims(o.mc)
    return (msfe = msfe, rmsfe = sqrt.(msfe), msfe_common = msfec, gain = msfe ./ msfec, relative = msfe ./ permutedims(o.m0),
            count = permutedims(o.cnt))
end

"Joint posterior draws of the factor path and of the missing / future cells with AR(q) idiosyncratic terms
(dfm_simsmooth_ar_batch; include/dfm_hip.h): arguments as forecast_ar; ndraws independent draws over rows q+1..T+H by the
simulation smoother, a pure function of (seed, first_draw + draw index), with mean `forecast_ar`'s x and the joint covariance of
its error (exact posterior draws when the only missing cells are ragged-edge and horizon cells).  Returns factor
(ndraws x (T+H-q) x r) and x (ndraws x (T+H-q) x N: observed cells as given)."
function draw_paths_ar(h::Handle, x::Matrix{Float64}, Lam::Matrix{Float64}, sig2::Vector{Float64}, rho::Matrix{Float64},
                       Avar::Matrix{Float64}, Q::Matrix{Float64}, mu0::Vector{Float64}, P0::Matrix{Float64}, ndraws::Integer,
                       H::Integer = 0; v0 = nothing, mean = nothing, sd = nothing, seed::Integer = 20160415,
                       first_draw::Integer = 0, singular_q::Bool = false)
    (mean === nothing) == (sd === nothing) || error("mean and sd go together")
    T, N = size(x); r = size(Lam, 2); q = size(rho, 2); p = div(size(Avar, 2), r); n = T + H - q
    panel = to_c_panel(x)
    LamC = permutedims(Lam); rhoC = permutedims(rho); AC = permutedims(Avar); QC = permutedims(Q); P0C = permutedims(P0)
    v0C = v0 === nothing ? C_NULL : Vector{Float64}(v0)
    meanC = mean === nothing ? C_NULL : Vector{Float64}(mean); sdC = sd === nothing ? C_NULL : Vector{Float64}(sd)
    f = Array{Float64}(undef, r, n, ndraws); xd = Array{Float64}(undef, N, n, ndraws)
    flags = (any(isnan, x) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve panel LamC sig2 rhoC AC QC mu0 P0C v0C meanC sdC f xd begin
        rc = ccall((:dfm_simsmooth_ar_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, UInt64, Int64, Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, ndraws, T, N, r, p, q, H, panel, LamC, sig2, rhoC, AC, QC, mu0, P0C, v0C, meanC, sdC, UInt64(seed),
                   Int64(first_draw), f, xd, flags)
        check(h.ptr, rc)
    end
    return (factor = permutedims(f, (3, 2, 1)), x = permutedims(xd, (3, 2, 1)))
end

"Panels simulated from a given model (dfm_simulate_batch; include/dfm_hip.h): params, nlag as `forecast`; ndraws panels of T rows,
draw d the x+ of `draw_paths`' unconditional step for the same (seed, first_draw + d).  `mask` (T x N, or nothing: balanced) is read
for its NaN pattern only: a cell is NaN where it is.  Returns x (ndraws x T x N) and factor (ndraws x T x r)."
function simulate(h::Handle, params, ndraws::Integer, T::Integer; nlag::Integer = 1, mask = nothing, seed::Integer = 20160415,
                  first_draw::Integer = 0)
    N, r = size(params.Lam)
    mask === nothing || size(mask) == (T, N) || error("mask must be T x N")
    Av = hasproperty(params, :Avar) ? params.Avar : params.A
    maskC = mask === nothing ? C_NULL : to_c_panel(Matrix{Float64}(mask))
    Lam = permutedims(params.Lam); R = copy(params.R); AC = permutedims(Av); QC = permutedims(params.Q)
    mu0 = copy(params.mu0); P0C = permutedims(params.P0)
    f = Array{Float64}(undef, r, T, ndraws); x = Array{Float64}(undef, N, T, ndraws)
    GC.@preserve maskC Lam R AC QC mu0 P0C f x begin
        rc = ccall((:dfm_simulate_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, UInt64, Int64, Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, ndraws, T, N, r, nlag, maskC, Lam, R, AC, QC, mu0, P0C, UInt64(seed), Int64(first_draw), x, f, Cuint(0))
        check(h.ptr, rc)
    end
    return (x = permutedims(x, (3, 2, 1)), factor = permutedims(f, (3, 2, 1)))
end

"The device-pointer twin (dfm_simulate_batch_dev) for arrays that already live on the GPU, row-major as the C interface has them:
B replicates, D draws each; mask_panel and f_sim may be C_NULL.  Enqueues on the handle's stream and returns; the caller synchronises."
function simulate_dev!(h::Handle, B::Integer, D::Integer, T::Integer, N::Integer, r::Integer, p::Integer, mask_panel::Ptr{Float64},
                       Lam::Ptr{Float64}, R::Ptr{Float64}, Avar::Ptr{Float64}, Q::Ptr{Float64}, mu0::Ptr{Float64}, P0::Ptr{Float64},
                       seed::Integer, first_draw::Integer, x_sim::Ptr{Float64}, f_sim::Ptr{Float64})
    rc = ccall((:dfm_simulate_batch_dev, LIB), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, UInt64, Int64, Ptr{Float64}, Ptr{Float64}, Cuint),
               h.ptr, B, D, T, N, r, p, mask_panel, Lam, R, Avar, Q, mu0, P0, UInt64(seed), Int64(first_draw), x_sim, f_sim, Cuint(0))
    check(h.ptr, rc)
    return nothing
end

"Panels simulated from the model with AR(q) idiosyncratic terms (dfm_simulate_ar_batch; include/dfm_hip.h): parameters as
forecast_ar.  With a panel `x` (T x N) the draws repeat its first q rows and carry its NaN pattern -- the parametric bootstrap of
`em_ar`, conditional on what its likelihood conditions on; with x = nothing every cell of the T rows is simulated.  Draw d is the
x+ of `draw_paths_ar` for the same (seed, first_draw + d).  Returns x (ndraws x T x N) and factor (ndraws x (T-q) x r)."
function simulate_ar(h::Handle, Lam::Matrix{Float64}, sig2::Vector{Float64}, rho::Matrix{Float64}, Avar::Matrix{Float64},
                     Q::Matrix{Float64}, mu0::Vector{Float64}, P0::Matrix{Float64}, ndraws::Integer, T::Integer; x = nothing,
                     v0 = nothing, seed::Integer = 20160415, first_draw::Integer = 0)
    N, r = size(Lam); q = size(rho, 2); p = div(size(Avar, 2), r); n = T - q
    x === nothing || size(x) == (T, N) || error("x must be T x N")
    panel = x === nothing ? C_NULL : to_c_panel(Matrix{Float64}(x))
    LamC = permutedims(Lam); rhoC = permutedims(rho); AC = permutedims(Avar); QC = permutedims(Q); P0C = permutedims(P0)
    v0C = v0 === nothing ? C_NULL : Vector{Float64}(v0)
    f = Array{Float64}(undef, r, n, ndraws); xs = Array{Float64}(undef, N, T, ndraws)
    GC.@preserve panel LamC sig2 rhoC AC QC mu0 P0C v0C f xs begin
        rc = ccall((:dfm_simulate_ar_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, UInt64, Int64, Ptr{Float64},
                    Ptr{Float64}, Cuint),
                   h.ptr, 1, ndraws, T, N, r, p, q, panel, LamC, sig2, rhoC, AC, QC, mu0, P0C, v0C, UInt64(seed), Int64(first_draw),
                   xs, f, Cuint(0))
        check(h.ptr, rc)
    end
    return (x = permutedims(xs, (3, 2, 1)), factor = permutedims(f, (3, 2, 1)))
end

"The device-pointer twin (dfm_simulate_ar_batch_dev): as simulate_dev!, with panel, v0 and f_sim allowed to be C_NULL."
function simulate_ar_dev!(h::Handle, B::Integer, D::Integer, T::Integer, N::Integer, r::Integer, p::Integer, q::Integer,
                          panel::Ptr{Float64}, Lam::Ptr{Float64}, sig2::Ptr{Float64}, rho::Ptr{Float64}, Avar::Ptr{Float64},
                          Q::Ptr{Float64}, mu0::Ptr{Float64}, P0::Ptr{Float64}, v0::Ptr{Float64}, seed::Integer,
                          first_draw::Integer, x_sim::Ptr{Float64}, f_sim::Ptr{Float64})
    rc = ccall((:dfm_simulate_ar_batch_dev, LIB), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, UInt64, Int64, Ptr{Float64}, Ptr{Float64},
                Cuint),
               h.ptr, B, D, T, N, r, p, q, panel, Lam, sig2, rho, Avar, Q, mu0, P0, v0, UInt64(seed), Int64(first_draw), x_sim,
               f_sim, Cuint(0))
    check(h.ptr, rc)
    return nothing
end

"Joint ECM estimation with AR(q) idiosyncratic terms (dfm_em_ar_batch; include/dfm_hip.h): the re-estimation of the
reference's `lambda`, `uar_coef`, `uar_ser` (dfm_functions.ipynb:391-415) and factor VAR inside the parametric model.
Arguments as ks_pass_ar (the start: what `estimate!(m)` left in the model).  Returns the updated parameters, the
log-likelihood path (conditional on the first q rows; non-decreasing) and the smoothed factors of rows q+1..T."
function em_ar(h::Handle, x::Matrix{Float64}, Lam::Matrix{Float64}, sig2::Vector{Float64}, rho::Matrix{Float64},
               Avar::Matrix{Float64}, Q::Matrix{Float64}, mu0::Vector{Float64}, P0::Matrix{Float64};
               max_iter::Integer = 20, tol::Real = 1e-6, singular_q::Bool = false)
    T, N = size(x); r = size(Lam, 2); q = size(rho, 2); p = div(size(Avar, 2), r)
    panel = to_c_panel(x)
    LamC = permutedims(Lam); sig = copy(sig2); rhoC = permutedims(rho); AC = permutedims(Avar); QC = permutedims(Q)
    mu = copy(mu0); P0C = permutedims(P0)
    path = Array{Float64}(undef, max_iter); iters = Array{Cint}(undef, 1)
    f = Array{Float64}(undef, r, T - q); np = div(r * (r + 1), 2); P = Array{Float64}(undef, np, T - q)
    flags = (any(isnan, x) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve panel LamC sig rhoC AC QC mu P0C path iters f P begin
        rc = ccall((:dfm_em_ar_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Cdouble, Ptr{Float64}, Ptr{Cint},
                    Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, T, N, r, p, q, panel, LamC, sig, rhoC, AC, QC, mu, P0C, max_iter, tol, path, iters, f, P, flags)
        check(h.ptr, rc)
    end
    kk = Int(iters[1])
    return (Lam = permutedims(LamC), sig2 = sig, rho = permutedims(rhoC), Avar = permutedims(AC), Q = permutedims(QC),
            mu0 = mu, P0 = permutedims(P0C), loglik = path[1:kk], iters = kk, factor = permutedims(f))
end

# ---- the reference's NON-parametric estimator on the GPU (als.hip) ------------------------------------------------

const MF_WEIGHTS = Dict("m" => [1.0], "q_flow" => [1, 2, 3, 2, 1] ./ 3, "q_avg" => [1, 1, 1] ./ 3)

"N x L aggregation weights from the matrix itself or from a vector of \"m\" / \"q_flow\" / \"q_avg\" (include/dfm_hip.h, mixed frequency)."
function mf_weights(weights, N::Integer)
    if weights isa AbstractMatrix
        W = Matrix{Float64}(weights)
    else
        L = maximum(length(MF_WEIGHTS[k]) for k in weights)
        W = zeros(length(weights), L)
        for (i, k) in enumerate(weights)
            w = MF_WEIGHTS[k]
            W[i, 1:length(w)] = w
        end
    end
    size(W, 1) == N || error("weights: $(size(W, 1)) rows for $N series")
    return W
end

"EM iterations of the mixed-frequency model from a given start (dfm_em_mf_batch; include/dfm_hip.h): z is the standardised MONTHLY
panel (T x N, NaN = missing; a quarterly series sits in the third month of its quarter), W N x L, Lam N x r, R, Avar r x (r p), Q,
mu0 / P0 the moments of z_0, r max(p, L) wide.  Returns the updated parameters, the log-likelihood path and the smoothed factors."
function em_mf(h::Handle, z::Matrix{Float64}, W::Matrix{Float64}, Lam::Matrix{Float64}, R::Vector{Float64}, Avar::Matrix{Float64},
               Q::Matrix{Float64}, mu0::Vector{Float64}, P0::Matrix{Float64}; max_iter::Integer = 50, tol::Real = 1e-6,
               singular_q::Bool = false)
    T, N = size(z); r = size(Lam, 2); L = size(W, 2); p = div(size(Avar, 2), r)
    panel = to_c_panel(z)
    LamC = permutedims(Lam); Rc = copy(R); WC = permutedims(W); AC = permutedims(Avar); QC = permutedims(Q)
    mu = copy(mu0); P0C = permutedims(P0)
    path = Array{Float64}(undef, max_iter); iters = Array{Cint}(undef, 1)
    f = Array{Float64}(undef, r, T); np = div(r * (r + 1), 2); P = Array{Float64}(undef, np, T)
    flags = (any(isnan, z) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve panel LamC Rc WC AC QC mu P0C path iters f P begin
        rc = ccall((:dfm_em_mf_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Cdouble, Ptr{Float64}, Ptr{Cint},
                    Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, T, N, r, p, L, panel, LamC, Rc, WC, AC, QC, mu, P0C, max_iter, tol, path, iters, f, P, flags)
        check(h.ptr, rc)
    end
    kk = Int(iters[1])
    return (Lam = permutedims(LamC), R = Rc, Avar = permutedims(AC), Q = permutedims(QC), mu0 = mu, P0 = permutedims(P0C),
            loglik = path[1:kk], iters = kk, factor = permutedims(f))
end

"em_mf with FIXED loadings (dfm_em_mf_blocks_batch; include/dfm_hip.h): `free` is N x r, true / nonzero = estimated; a fixed loading
keeps the value it has in Lam (0 for a block structure, 1 for a normalisation).  Arguments and result otherwise as em_mf."
function em_mf_blocks(h::Handle, z::Matrix{Float64}, W::Matrix{Float64}, free::AbstractMatrix, Lam::Matrix{Float64}, R::Vector{Float64},
                      Avar::Matrix{Float64}, Q::Matrix{Float64}, mu0::Vector{Float64}, P0::Matrix{Float64}; max_iter::Integer = 50,
                      tol::Real = 1e-6, singular_q::Bool = false)
    T, N = size(z); r = size(Lam, 2); L = size(W, 2); p = div(size(Avar, 2), r)
    size(free) == (N, r) || error("free: $(size(free)) for $N series and $r factors")
    panel = to_c_panel(z)
    LamC = permutedims(Lam); Rc = copy(R); WC = permutedims(W); AC = permutedims(Avar); QC = permutedims(Q)
    freeC = Matrix{UInt8}(permutedims(free .!= 0))
    mu = copy(mu0); P0C = permutedims(P0)
    path = Array{Float64}(undef, max_iter); iters = Array{Cint}(undef, 1)
    f = Array{Float64}(undef, r, T); np = div(r * (r + 1), 2); P = Array{Float64}(undef, np, T)
    flags = (any(isnan, z) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve panel LamC Rc WC freeC AC QC mu P0C path iters f P begin
        rc = ccall((:dfm_em_mf_blocks_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Cdouble, Ptr{Float64}, Ptr{Cint},
                    Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, T, N, r, p, L, panel, LamC, Rc, WC, freeC, AC, QC, mu, P0C, max_iter, tol, path, iters, f, P, flags)
        check(h.ptr, rc)
    end
    kk = Int(iters[1])
    return (Lam = permutedims(LamC), R = Rc, Avar = permutedims(AC), Q = permutedims(QC), mu0 = mu, P0 = permutedims(P0C),
            loglik = path[1:kk], iters = kk, factor = permutedims(f))
end

"The device-pointer twin (dfm_em_mf_blocks_batch_dev) for arrays that already live on the GPU, row-major as the C interface has them:
B replicates, parameters updated in place, `free` N x r bytes read only (C_NULL: every loading estimated); f / P may be C_NULL.
Enqueues on the handle's stream and returns; the caller synchronises."
function em_mf_blocks_dev!(h::Handle, B::Integer, T::Integer, N::Integer, r::Integer, p::Integer, L::Integer, panel::Ptr{Float64},
                           Lam::Ptr{Float64}, R::Ptr{Float64}, W::Ptr{Float64}, free::Ptr{Cvoid}, Avar::Ptr{Float64}, Q::Ptr{Float64},
                           mu0::Ptr{Float64}, P0::Ptr{Float64}, max_iter::Integer, tol::Real, path::Ptr{Float64}, iters::Ptr{Cint},
                           f::Ptr{Float64}, P::Ptr{Float64}, flags::Cuint)
    rc = ccall((:dfm_em_mf_blocks_batch_dev, LIB), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Cdouble, Ptr{Float64}, Ptr{Cint},
                Ptr{Float64}, Ptr{Float64}, Cuint),
               h.ptr, B, T, N, r, p, L, panel, Lam, R, W, free, Avar, Q, mu0, P0, max_iter, tol, path, iters, f, P, flags)
    check(h.ptr, rc)
    return nothing
end

"Smoother pass of the mixed-frequency model (dfm_ks_pass_mf_batch): arguments as em_mf; returns the smoothed monthly factors, their
packed covariances and the log-likelihood."
function ks_pass_mf(h::Handle, z::Matrix{Float64}, W::Matrix{Float64}, Lam::Matrix{Float64}, R::Vector{Float64}, Avar::Matrix{Float64},
                    Q::Matrix{Float64}, mu0::Vector{Float64}, P0::Matrix{Float64}; singular_q::Bool = false)
    T, N = size(z); r = size(Lam, 2); L = size(W, 2); p = div(size(Avar, 2), r)
    panel = to_c_panel(z)
    LamC = permutedims(Lam); WC = permutedims(W); AC = permutedims(Avar); QC = permutedims(Q); P0C = permutedims(P0)
    f = Array{Float64}(undef, r, T); np = div(r * (r + 1), 2); P = Array{Float64}(undef, np, T)
    ll = Array{Float64}(undef, 1)
    flags = (any(isnan, z) ? DFM_F_MAY_HAVE_MISSING : Cuint(0)) | (singular_q ? DFM_F_SINGULAR_Q : Cuint(0))
    GC.@preserve panel LamC R WC AC QC mu0 P0C f P ll begin
        rc = ccall((:dfm_ks_pass_mf_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cuint),
                   h.ptr, 1, T, N, r, p, L, panel, LamC, R, WC, AC, QC, mu0, P0C, f, P, ll, flags)
        check(h.ptr, rc)
    end
    return (factor = permutedims(f), P = permutedims(P), loglik = ll[1])
end

"Maximum likelihood of the mixed-frequency DFM (api.estimate_mixed_frequency's steps): x is the MONTHLY panel in data units (T x N,
NaN = missing), `weights` the N x L matrix or a vector of \"m\" / \"q_flow\" / \"q_avg\".  Every series is standardised with its own
mean and population s.d.; the start is the PCA of the fully observed monthly series (pca_init), every series' loadings by a
regression on the aggregated PCA factors, a VAR(p) by OLS; then dfm_em_mf_batch.  Returns the parameters (standardised units),
W, mean, sd, the log-likelihood path and the smoothed monthly factors.  (No bootstrap replicates here: nrep is Python's.)"
function estimate_mixed(x::Matrix{Float64}, weights, r::Integer, p::Integer; max_em_iter::Integer = 50, tol_em::Real = 1e-6,
                        h::Handle = handle())
    T, N = size(x)
    W = mf_weights(weights, N)
    L = size(W, 2); m = max(p, L)
    obs = .!isnan.(x)
    mu = [sum(x[obs[:, i], i]) / count(obs[:, i]) for i in 1:N]
    sd = [sqrt(sum((x[obs[:, i], i] .- mu[i]) .^ 2) / count(obs[:, i])) for i in 1:N]
    z = (x .- mu') ./ sd'
    monthly = [W[i, 1] == 1.0 && all(W[i, 2:end] .== 0.0) for i in 1:N]
    bal = [monthly[i] && all(obs[:, i]) for i in 1:N]
    count(bal) >= r || error("fewer fully observed monthly series than factors: cannot initialise by PCA")
    F = pca_init(h, z[:, bal], r).F
    Lam = zeros(N, r); R = ones(N)
    for i in 1:N
        g = zeros(T, r)
        for l in 0:L-1
            g[l+1:T, :] .+= W[i, l+1] .* F[1:T-l, :]
        end
        o = copy(obs[:, i]); o[1:L-1] .= false
        count(o) < r + 1 && continue
        Lam[i, :] = g[o, :] \ z[o, i]
        R[i] = max(sum((z[o, i] .- g[o, :] * Lam[i, :]) .^ 2) / count(o), 0.05)
    end
    lagged(k) = hcat([F[k-l:T-l, :] for l in 0:k-1]...)          # rows (f_t, .., f_{t-k+1}), t = k..T
    Z = lagged(p)
    Y = F[p+1:T, :]; Xl = Z[1:end-1, :]
    Avar = permutedims((Xl' * Xl) \ (Xl' * Y))
    e = Y .- Xl * Avar'
    Q = e' * e ./ (T - p); Q = (Q .+ Q') ./ 2
    Zm = lagged(m)
    P0 = Zm' * Zm ./ size(Zm, 1); P0 = (P0 .+ P0') ./ 2
    for j in 1:r*m
        P0[j, j] += 1e-3
    end
    est = try
        em_mf(h, z, W, Lam, R, Avar, Q, zeros(r * m), P0; max_iter = max_em_iter, tol = tol_em)
    catch err                                                    # the information form inverts Q: retry in covariance form
        (err isa ErrorException && occursin("status $(DFM_E_NUMERIC):", err.msg)) || rethrow()
        em_mf(h, z, W, Lam, R, Avar, Q, zeros(r * m), P0; max_iter = max_em_iter, tol = tol_em, singular_q = true)
    end
    return merge(est, (W = W, mean = mu, sd = sd))
end

"`estimate_factor!` sweeps (dfm_functions.ipynb:352-370) for ONE run: z is the standardised T x N window (NaN =
missing), F0 the T x r start (pca_score).  dfm_als_batch; returns factors, loadings (NaN rows: no loadings), ssr,
iterations, R2."
function als(h::Handle, z::Matrix{Float64}, F0::Matrix{Float64}; nt_min::Integer = 20,
             max_iter::Integer = 100000000, tol::Real = 1e-8, want_R2::Bool = true)
    T, N = size(z); r = size(F0, 2)
    zc = permutedims(z, (2, 1))                                   # (N, T) column-major == C [t][i]
    F = reshape(permutedims(F0, (2, 1)), r, T, 1)                 # C [b][t][k]
    Lam = Array{Float64}(undef, r, N, 1); iters = Array{Cint}(undef, 1); ssr = Array{Float64}(undef, 1)
    R2 = Array{Float64}(undef, N, 1)
    GC.@preserve zc F Lam iters ssr R2 begin
        rc = ccall((:dfm_als_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Float64}, Clonglong, Ptr{Cint}, Ptr{Float64}, Ptr{Float64},
                    Cint, Cint, Cdouble, Ptr{Float64}, Cint, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}),
                   h.ptr, 1, T, N, r, zc, 0, C_NULL, F, Lam, nt_min, min(max_iter, typemax(Cint)), tol, C_NULL, 0,
                   iters, ssr, want_R2 ? pointer(R2) : Ptr{Float64}(C_NULL))
        check(h.ptr, rc)
    end
    return (factor = permutedims(F[:, :, 1]), Lam = permutedims(Lam[:, :, 1]), ssr = ssr[1], iters = Int(iters[1]),
            R2 = R2[:, 1])
end

"`estimate_factor!` sweeps for B runs in ONE call (dfm_als_batch): the runs of `estimate_factor_numbers` /
`amengual_watson_test` (dfm_functions.ipynb:698-768).  zs: one T x N window shared by every run, or a vector of B windows;
F0s[b]: T x r_b start (the first r_b columns of a `pca_score`); every run may have its own number of factors."
function als_batch(h::Handle, zs, F0s::Vector{Matrix{Float64}}; nt_min::Integer = 20, max_iter::Integer = 100000000,
                   tol::Real = 1e-8)
    shared = zs isa AbstractMatrix
    B = length(F0s); T = size(F0s[1], 1); r = maximum(size(f, 2) for f in F0s)
    N = shared ? size(zs, 2) : size(zs[1], 2)
    zc = shared ? permutedims(zs, (2, 1)) : cat([permutedims(z, (2, 1)) for z in zs]...; dims = 3)   # C [b][t][i]
    F = zeros(r, T, B)
    for b in 1:B
        F[1:size(F0s[b], 2), :, b] = permutedims(F0s[b], (2, 1))
    end
    r_each = Cint[size(f, 2) for f in F0s]
    Lam = Array{Float64}(undef, r, N, B); iters = Array{Cint}(undef, B); ssr = Array{Float64}(undef, B)
    R2 = Array{Float64}(undef, N, B)
    GC.@preserve zc r_each F Lam iters ssr R2 begin
        rc = ccall((:dfm_als_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Float64}, Clonglong, Ptr{Cint}, Ptr{Float64}, Ptr{Float64},
                    Cint, Cint, Cdouble, Ptr{Float64}, Cint, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}),
                   h.ptr, B, T, N, r, zc, shared ? 0 : T * N, r_each, F, Lam, nt_min, min(max_iter, typemax(Cint)), tol,
                   C_NULL, 0, iters, ssr, R2)
        check(h.ptr, rc)
    end
    return (factor = [permutedims(F[1:r_each[b], :, b]) for b in 1:B], Lam = [permutedims(Lam[1:r_each[b], :, b]) for b in 1:B],
            ssr = ssr, iters = Int.(iters), R2 = [R2[:, b] for b in 1:B])
end

"P complete-case regressions (`ols_skipmissing(..., Balanced())`, dfm_functions.ipynb:242-252): column p of Y (T x P,
NaN = missing) on the shared regressors X (T x K).  dfm_ols_batch; returns beta (K x P), resid (T x P), ssr, tss, nobs."
function ols(h::Handle, X::Matrix{Float64}, Y::Matrix{Float64}; nt_min::Integer = 0)
    T, K = size(X); P = size(Y, 2)
    Xc = permutedims(X, (2, 1)); Yc = permutedims(Y, (2, 1))      # C [t][k], C [t][p]
    beta = Array{Float64}(undef, K, P); resid = Array{Float64}(undef, T, P)
    ssr = Array{Float64}(undef, P); tss = similar(ssr); nobs = Array{Cint}(undef, P)
    GC.@preserve Xc Yc beta resid ssr tss nobs begin
        rc = ccall((:dfm_ols_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, Clonglong, Ptr{Float64}, Clonglong, Clonglong, Cint,
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}),
                   h.ptr, P, T, K, Xc, 0, Yc, 1, P, nt_min, beta, resid, ssr, tss, nobs)
        check(h.ptr, rc)
    end
    return (beta = beta, resid = resid, ssr = ssr, tss = tss, nobs = Int.(nobs))   # beta[:, p]: C [p][k] == Julia (k, p)
end

"Chow statistics with HAC covariance (dfm_chow_batch): series s = complete cases ys[s] (vector), Xs[s] (T_s x k);
problem p = (prob_series[p] (1-based), prob_break[p] rows before the break, bandwidth prob_q[p]).  `compute_qlr` is the
maximum over the problems of one series (dfm_functions.ipynb:1019-1047)."
function chow_batch(h::Handle, ys::Vector{Vector{Float64}}, Xs::Vector{Matrix{Float64}}, prob_series::Vector{<:Integer},
                    prob_break::Vector{<:Integer}, prob_q::Vector{<:Integer})
    S = length(ys); k = size(Xs[1], 2); Tlen = Cint[length(v) for v in ys]; Tmax = maximum(Tlen)
    y = zeros(Tmax, S); X = zeros(k, Tmax, S)                     # C [s][t], C [s][t][k]
    for s in 1:S
        y[1:Tlen[s], s] = ys[s]; X[:, 1:Tlen[s], s] = permutedims(Xs[s], (2, 1))
    end
    ps = Cint.(prob_series .- 1); pb = Cint.(prob_break); pq = Cint.(prob_q); P = length(ps)
    out = Array{Float64}(undef, P)
    GC.@preserve y X Tlen ps pb pq out begin
        rc = ccall((:dfm_chow_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Cint},
                    Ptr{Float64}), h.ptr, S, Tmax, k, y, X, Tlen, P, ps, pb, pq, out)
        check(h.ptr, rc)
    end
    return out
end

"B wild-bootstrap draws of the VAR's impulse responses (dfm_var_bootstrap_irf) and their nearest-rank quantile bands
(dfm_quantile_bands).  y, resid: T x ns over the estimation window; betahat: (1 + ns p) x ns as in `estimate_var!`."
function bootstrap_irf(h::Handle, y::Matrix{Float64}, betahat::Matrix{Float64}, resid::Matrix{Float64}, p::Integer,
                       H::Integer, ndraws::Integer; seed::Integer = 20160415, first_draw::Integer = 0,
                       quantiles = [0.05, 0.16, 0.5, 0.84, 0.95])
    T, ns = size(y)
    yc = permutedims(y, (2, 1)); bc = permutedims(betahat, (2, 1)); ec = permutedims(resid, (2, 1))
    irf = Array{Float64}(undef, ns, H, ns, ndraws)                # C [d][i][h][k] == Julia (k, h, i, d)
    q = Float64.(quantiles); bands = Array{Float64}(undef, ns, H, ns, length(q))
    GC.@preserve yc bc ec irf q bands begin
        rc = ccall((:dfm_var_bootstrap_irf, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    UInt64, Int64, Ptr{Float64}, Ptr{Float64}),
                   h.ptr, ndraws, T, ns, p, H, yc, bc, ec, C_NULL, seed, first_draw, C_NULL, irf)
        check(h.ptr, rc)
        rc = ccall((:dfm_quantile_bands, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                   h.ptr, ndraws, ns * H * ns, length(q), irf, q, bands)
        check(h.ptr, rc)
    end
    # to the reference's irf[variable, horizon, shock] (dfm_functions.ipynb:793-816), draws / quantiles last
    return (draws = permutedims(irf, (3, 2, 1, 4)), bands = permutedims(bands, (3, 2, 1, 4)))
end

end # module

import Random
using LinearAlgebra

# ---------------------------------------------------------------------------------------------------------
# The new method (SURVEY.md 8(b)).  Same mutate-in-place convention as the reference's estimate!
# (dfm_functions.ipynb:530-543); additionally returns the per-iteration log-likelihood vector.
#   nrep > 0: after the point estimate, `nrep` parametric-bootstrap replicates of the standardised window are drawn
#   from the fitted model (same missing pattern; Julia's RNG seeded with `seed`) and re-estimated by EM IN ONE BATCHED
#   CALL on `ngpu` GPUs (DFMHip.em_batch -> dfm_em_batch_multi: replicates sharded over the GPUs, one RCCL all-gather
#   per EM iteration); the method then returns (loglik = ..., replicates = ...).
function estimate!(m::DFMModel, ::Parametric; max_em_iter::Integer = 50, tol_em::Real = 1e-6,
                   factor_lags::Integer = m.n_factorlag, nrep::Integer = 0, seed::Integer = 20160415, ngpu::Integer = 1,
                   device::Integer = 0, handle = nothing, lam_constr_f = nothing, lam_constr_fl = nothing)
    (lam_constr_f === nothing && lam_constr_fl === nothing) ||
        error("loading constraints are not supported on the parametric path")   # never drop them silently
    m.nfac_o == 0 || return estimate_observed!(m; max_em_iter = max_em_iter, tol_em = tol_em, device = device, handle = handle)
    r = m.nfac_u
    nlag = Int(factor_lags)
    (nlag >= 1 && r * nlag <= 32) || error("need 1 <= factor_lags and nfac_u * factor_lags <= 32")
    (nrep == 0 || nlag == 1) || error("bootstrap replicates (nrep > 0) need factor_lags = 1")
    incl = m.inclcode .== 1
    xdata = m.data[m.initperiod:m.lastperiod, incl]                       # dfm_functions.ipynb:335-336
    xstd, xsd = standardize_data(xdata)                                   # :339
    m.fes.tss = sum(skipmissing(xstd .^ 2))                               # :342
    m.fes.nobs = count(.!ismissing.(xstd))                                # :343
    # :357 -- a series with fewer than nt_min_factor_estimation observed periods gets no loadings in the reference's
    # estimator: it is left out here too (api.estimate: `enough`)
    enough = vec(sum(.!ismissing.(xstd), dims = 1)) .>= m.nt_min_factor_estimation
    xstd = xstd[:, enough]; xsd = vec(xsd)[enough]
    z = reshape(DFMHip.nan_for_missing(xstd), size(xstd))
    xbal, balmask = drop_missing_col(xstd)                                # :345
    balmask = vec(balmask)
    size(xbal, 2) >= r || error("fewer fully observed series than factors: cannot initialise by PCA")
    h = handle === nothing ? DFMHip.handle(device) : handle               # one cached handle per device
    p0 = DFMHip.pca_init(h, Float64.(xbal), r)                            # pca_score (:179-183) + OLS start, on the GPU
    N = size(z, 2)
    Lam = Matrix{Float64}(undef, N, r); R = Vector{Float64}(undef, N)
    Lam[balmask, :] = p0.Lam; R[balmask] = p0.R
    gap = findall(.!balmask)
    if !isempty(gap)                                                      # series with gaps: complete-case OLS on the PCA
        o = DFMHip.ols(h, p0.F, z[:, gap])                                # factors (:242-252), one dfm_ols_batch call
        Lam[gap, :] = permutedims(o.beta); R[gap] = o.ssr ./ max.(o.nobs, 1)
    end
    fit = if nlag == 1
        DFMHip.em(h, z, (Lam = Lam, R = R, A = p0.A, Q = p0.Q, mu0 = p0.mu0, P0 = p0.P0);
                  max_iter = max_em_iter, tol = tol_em)
    else   # VAR(p) start: OLS of the PCA factors on their lags, no constant (dfm_ols_batch); companion-form EM
        T = size(z, 1)
        Z = hcat([p0.F[nlag-l:T-l, :] for l in 0:nlag-1]...)                  # row j: (f_{p-1+j}, .., f_j)
        o = DFMHip.ols(h, Z[1:end-1, :], p0.F[nlag+1:end, :])
        Qv = o.resid' * o.resid / (T - nlag)
        P0v = Z' * Z / size(Z, 1)
        DFMHip.em_varp(h, z, (Lam = Lam, R = R, Avar = permutedims(o.beta), Q = (Qv + Qv') / 2, mu0 = zeros(r * nlag),
                              P0 = (P0v + P0v') / 2), nlag; max_iter = max_em_iter, tol = tol_em)
    end
    m.factor[m.initperiod:m.lastperiod, :] = fit.factor                   # in place: aliases factor_var_model.y (:80, :371)
    cols = findall(incl)[enough]
    m.lambda[cols, :] = fit.Lam .* xsd
    m.uar_ser[cols] = sqrt.(fit.R) .* xsd
    m.uar_coef[cols, :] .= 0.0
    common = fit.factor * fit.Lam'
    e = [isnan(z[t, i]) ? 0.0 : z[t, i] - common[t, i] for t in 1:size(z, 1), i in 1:N]
    m.fes.ssr = sum(abs2, e)                                              # :366
    var = m.factor_var_model                                              # fill_matrices! (:477-492), VAR(1) block
    fill!(var.M, 0.0); fill!(var.Q, 0.0); fill!(var.G, 0.0)
    ka = min(size(fit.A, 2), size(var.M, 2))
    var.M[1:r, 1:ka] = fit.A[:, 1:ka]                                     # [A_1 .. A_p] (:484-486)
    var.nlag > 1 && (var.M[r+1:end, 1:end-r] = Matrix(1.0I, r * (var.nlag - 1), r * (var.nlag - 1)))
    var.Q[1:r, 1:r] = Matrix(1.0I, r, r)
    var.seps[:, :] = fit.Q
    # fill_matrices! takes the lower Cholesky factor (:489); a rank-deficient Q (covariance-form fit) has none: its
    # symmetric square root then stands in (G G' = Q still holds)
    var.G[1:r, 1:r] = isposdef(Symmetric(fit.Q)) ? cholesky(Symmetric(fit.Q)).L :
                      (e = eigen(Symmetric(fit.Q)); e.vectors * Diagonal(sqrt.(max.(e.values, 0.0))) * e.vectors')
    nrep == 0 && return fit.loglik
    # ---- parametric-bootstrap replicates, re-estimated in one batched multi-GPU call (api.estimate: same steps) ----
    rng = Random.MersenneTwister(seed)
    T = size(z, 1)
    # square roots by eigendecomposition: a fit that needed the covariance-form recursion (DFM_F_SINGULAR_Q) has a
    # rank-deficient Q, and `cholesky` would throw AFTER the point estimate was written into the model
    psd_sqrt(S) = (e = eigen(Symmetric((S + S') / 2)); e.vectors * Diagonal(sqrt.(max.(e.values, 0.0))))
    LQ = psd_sqrt(fit.Q)
    LS = psd_sqrt(fit.P0)                                                 # start the factor path from the fitted f_0 moments
    panels = Vector{Matrix{Float64}}(undef, nrep)
    for b in 1:nrep
        f = fit.mu0 + LS * randn(rng, r)
        x = Matrix{Float64}(undef, T, N)
        for t in 1:T
            f = fit.A * f + LQ * randn(rng, r)
            x[t, :] = fit.Lam * f + sqrt.(fit.R) .* randn(rng, N)
        end
        x[isnan.(z)] .= NaN                                               # the window's own missing pattern
        panels[b] = x
    end
    start = (Lam = fit.Lam, R = fit.R, A = fit.A, Q = fit.Q, mu0 = fit.mu0, P0 = fit.P0)
    reps = DFMHip.em_batch(panels, [start for _ in 1:nrep]; max_iter = max_em_iter, tol = tol_em, ngpu = ngpu,
                           singular_q = fit.singular_q)
    return (loglik = fit.loglik, replicates = reps)
end


# ---------------------------------------------------------------------------------------------------------
# The reference's own estimator on the GPU: same arguments and effects as `estimate_factor!(m, max_iter, computeR2)`
# (dfm_functions.ipynb:328-382), PCA start and every sweep on the GPU.  Loading constraints (`lam_constr`, used at
# Stock_Watson.ipynb:1336-1344) are NOT implemented on the HIP path: with constraints this method hands the call to the
# reference's own pure-Julia method when the maintainer has kept it under the name `estimate_factor_cpu!` (see
# INTEGRATION.md for the two-line change), and raises otherwise -- it never drops them.
function estimate_factor_hip!(m::DFMModel, max_iter::Integer = 100000000, computeR2::Bool = true; lam_constr = nothing,
                              device::Integer = 0, handle = nothing)
    if lam_constr !== nothing
        isdefined(Main, :estimate_factor_cpu!) ||
            error("estimate_factor_hip!: loading constraints are not supported on the HIP path and the reference's " *
                  "method is not available as estimate_factor_cpu! (INTEGRATION.md)")
        return Main.estimate_factor_cpu!(m, max_iter, computeR2; lam_constr = lam_constr)
    end
    m.nfac_o == 0 || error("observed factors are not supported on the HIP path")
    xdata = m.data[m.initperiod:m.lastperiod, m.inclcode .== 1]           # :335-336
    xstd, _ = standardize_data(xdata)                                     # :339
    m.fes.tss = sum(skipmissing(xstd .^ 2))                               # :342
    m.fes.nobs = count(.!ismissing.(xstd))                                # :343
    xbal, _ = drop_missing_col(xstd)                                      # :345
    h = handle === nothing ? DFMHip.handle(device) : handle               # cached: the notebook calls this ~200 times a table
    F0 = DFMHip.pca_init(h, Float64.(xbal), m.nfac_u).F                  # pca_score (:348)
    z = reshape(DFMHip.nan_for_missing(xstd), size(xstd))
    fit = DFMHip.als(h, z, F0; nt_min = m.nt_min_factor_estimation, max_iter = max_iter, tol = m.tol,
                     want_R2 = computeR2)                                 # :352-370, :372-380
    m.factor[m.initperiod:m.lastperiod, :] = fit.factor                   # :371
    m.fes.ssr = fit.ssr                                                   # :366
    computeR2 && (m.fes.R2 = fit.R2)
    return nothing
end

# `impulse_response(varm, shock_id::Real, T)` (dfm_functions.ipynb:817-821) repaired.  The reference's method cannot run: it passes an
# undefined `x` and SIX arguments to the five-argument `compute_irf_single_shock!(irfs, varm, i, shock_id, T)` (:801-810).  What it
# means is evident from the vector method (:793-799): the same recursion -- irf[:, t] = Q M^(t-1) G[:, shock_id] -- written into a
# ny x T matrix (`irfs[:, t, 1]` addresses a Matrix: a trailing index 1 is legal).  Defining it here REPLACES the broken method once
# the notebook's functions are loaded (same signature); the vector and `:all` methods (:793-799, :822-825) are the reference's own.
# Mirror: dynamic_factor_models_amd/api.py impulse_response (scalar shock id).
function impulse_response(varm::VARModel, shock_id::Real, T::Integer)
    isinteger(shock_id) && 1 <= shock_id <= size(varm.G, 2) ||
        throw(ArgumentError("shock_id must be an integer in 1:$(size(varm.G, 2))"))
    irfs = Matrix{Float64}(undef, size(varm.Q, 1), T)
    compute_irf_single_shock!(irfs, varm, 1, Int(shock_id), T)
    return irfs
end

# Wild-bootstrap bands of `impulse_response(varm, shock_ids, T)` (dfm_functions.ipynb:793-816) for an estimated VARModel.
function bootstrap_irf_bands(varm::VARModel, H::Integer; ndraws::Integer = 10000, seed::Integer = 20160415,
                             device::Integer = 0, handle = nothing)
    rows = findall(t -> !any(ismissing, varm.resid[t, :]), 1:size(varm.resid, 1))
    first = rows[1] - varm.nlag
    y = Float64.(varm.y[first:rows[end], :])
    resid = zeros(size(y)); resid[varm.nlag+1:end, :] = Float64.(varm.resid[rows, :])
    h = handle === nothing ? DFMHip.handle(device) : handle
    return DFMHip.bootstrap_irf(h, y, Float64.(varm.betahat), resid, varm.nlag, H, ndraws; seed = seed)
end

# ---------------------------------------------------------------------------------------------------------
# `estimate_factor_numbers(m, nfacs)` (dfm_functions.ipynb:698-725) with its batch axis on the GPU.  The reference runs
# `estimate_factor!` once per static factor count and, inside each, `amengual_watson_test` (:734-768) runs it once more per
# dynamic factor count: 10 + 55 serial estimations for Table 2 (Stock_Watson.ipynb:516, 591, 643, 893).  Here:
#   1 dfm_pca_init_batch + ONE dfm_als_batch        for the max_nfac static runs (shared window, r_each = 1..max_nfac;
#                                                    `pca_score` columns are nested, so run r starts from the first r);
#   per static count i: 1 dfm_ols_batch             (every series on [1, lags of the i factors], :741-750) and
#                       1 dfm_pca_init_batch        (start of the residual panel's runs);
#   ONE dfm_als_batch                                for ALL max_nfac (max_nfac + 1) / 2 dynamic runs, each on its own
#                                                    residual window.
# Same return type and fields as the reference (FactorNumberEstimateStats); mirrors api.estimate_factor_numbers(with_aw).
function estimate_factor_numbers_hip(m::DFMModel, nfacs::Union{Real, AbstractVector}; device::Integer = 0, handle = nothing)
    m.nfac_o == 0 || error("observed factors are not supported on the HIP path")
    max_nfac = Int(maximum(nfacs))
    h = handle === nothing ? DFMHip.handle(device) : handle
    incl = m.inclcode .== 1
    ns = count(incl)
    xdata = m.data[m.initperiod:m.lastperiod, incl]                       # :335-336
    xstd, _ = standardize_data(xdata)                                     # :339
    tss = sum(skipmissing(xstd .^ 2)); nobs = count(.!ismissing.(xstd)); T = size(xstd, 1)
    xbal, _ = drop_missing_col(xstd)                                      # :345
    F0 = DFMHip.pca_init(h, Float64.(xbal), max_nfac).F                   # pca_score (:348), nested columns
    z = reshape(DFMHip.nan_for_missing(xstd), size(xstd))
    st = DFMHip.als_batch(h, z, [F0[:, 1:k] for k in 1:max_nfac]; nt_min = m.nt_min_factor_estimation, tol = m.tol)
    bn(ssr, no, Tn, k) = (nbar = no / Tn; log(ssr / no) + k * log(min(nbar, Tn)) * (nbar + Tn) / no)   # bai_ng_criterion (:684-690)
    bn_icp = Vector{Union{Missing, Float64}}(undef, max_nfac)
    ssr_static = Vector{Float64}(undef, max_nfac)
    R2_static = Matrix{Union{Missing, Float64}}(undef, ns, max_nfac)
    aw_icp = Matrix{Union{Missing, Float64}}(missing, max_nfac, max_nfac)
    ssr_dynamic = Matrix{Union{Missing, Float64}}(missing, max_nfac, max_nfac)
    R2_dynamic = Array{Union{Missing, Float64}}(missing, ns, max_nfac, max_nfac)
    nan2missing(v) = Union{Missing, Float64}[isnan(x) ? missing : x for x in v]
    for i in 1:max_nfac
        bn_icp[i] = bn(st.ssr[i], nobs, T, i); ssr_static[i] = st.ssr[i]; R2_static[:, i] = nan2missing(st.R2[i])
    end
    # ---- amengual_watson_test of every static run: residual panels, then ALL dynamic runs in one call ----
    est = m.data[:, incl]
    Tall = size(est, 1)
    nlag = m.factor_var_model.nlag
    estn = reshape(DFMHip.nan_for_missing(est), size(est))
    zs = Matrix{Float64}[]; F0s = Matrix{Float64}[]; owner = Tuple{Int,Int}[]; nobs_i = Int[]; T_i = Int[]
    for i in 1:max_nfac
        fac = Matrix{Union{Missing, Float64}}(missing, Tall, i)
        fac[m.initperiod:m.lastperiod, :] = st.factor[i]
        x = [ones(Tall) lagmat(fac, 1:nlag)]                              # :741
        xn = reshape(DFMHip.nan_for_missing(x), size(x))
        # a series keeps its residuals when it has at least nt_min rows MORE than regressors (:744)
        o = DFMHip.ols(h, xn, estn; nt_min = size(xn, 2) + m.nt_min_factor_estimation)
        res = Union{Missing, Float64}[isnan(v) ? missing : v for v in o.resid]
        rstd, _ = standardize_data(res[m.initperiod+4:m.lastperiod, :])  # :761 (the reference hard-codes the 4)
        rbal, _ = drop_missing_col(rstd)
        Fi = DFMHip.pca_init(h, Float64.(rbal), i).F
        zi = reshape(DFMHip.nan_for_missing(rstd), size(rstd))
        for k in 1:i
            push!(zs, zi); push!(F0s, Fi[:, 1:k]); push!(owner, (k, i))
        end
        push!(nobs_i, count(.!ismissing.(rstd))); push!(T_i, size(rstd, 1))
    end
    dy = DFMHip.als_batch(h, zs, F0s; nt_min = m.nt_min_factor_estimation, tol = m.tol)
    for (b, (k, i)) in enumerate(owner)
        aw_icp[k, i] = bn(dy.ssr[b], nobs_i[i], T_i[i], k)
        ssr_dynamic[k, i] = dy.ssr[b]
        R2_dynamic[:, k, i] = nan2missing(dy.R2[b])
    end
    return FactorNumberEstimateStats(bn_icp, ssr_static, R2_static, aw_icp, ssr_dynamic, R2_dynamic, tss, nobs, T)
end


# ---------------------------------------------------------------------------------------------------------
# `estimate!(m, Parametric())` with OBSERVED factors (nfac_o > 0).  The reference's estimator is non-functional there
# (dfm_functions.ipynb:358-359, :371), so the semantics are those its data layout implies (include/dfm_hip.h,
# oracle/obs_oracle.py; api._estimate_parametric_observed is the same sequence): the caller has filled
# m.factor[initperiod:lastperiod, 1:nfac_o] with the observed factors; they are known regressors of the measurement
# equation, only the nfac_u remaining factors are latent.  Afterwards m.factor[:, nfac_o+1:end] = E[f_t | X], m.lambda the
# nfac_t loadings, and the factor VAR of ALL factors is the reference's own `estimate_var!(m.factor_var_model)`.
function estimate_observed!(m::DFMModel; max_em_iter::Integer = 50, tol_em::Real = 1e-6, device::Integer = 0, handle = nothing)
    ro, ru = m.nfac_o, m.nfac_u
    incl = m.inclcode .== 1
    Gm = m.factor[m.initperiod:m.lastperiod, 1:ro]
    any(ismissing, Gm) && error("observed factors: fill m.factor[initperiod:lastperiod, 1:nfac_o] (no gaps) before estimate!")
    G = Float64.(Gm)
    xstd, xsd = standardize_data(m.data[m.initperiod:m.lastperiod, incl])      # :335-339
    m.fes.tss = sum(skipmissing(xstd .^ 2)); m.fes.nobs = count(.!ismissing.(xstd))
    enough = vec(sum(.!ismissing.(xstd), dims = 1)) .>= m.nt_min_factor_estimation
    xstd = xstd[:, enough]; xsd = vec(xsd)[enough]
    z = reshape(DFMHip.nan_for_missing(xstd), size(xstd))
    h = handle === nothing ? DFMHip.handle(device) : handle
    og = DFMHip.ols(h, G, z)                                                   # every series on the observed factors
    res = Union{Missing, Float64}[isnan(v) ? missing : v for v in og.resid]
    rbal, balmask = drop_missing_col(res)
    balmask = vec(balmask)
    size(rbal, 2) >= ru || error("fewer fully observed series than unobserved factors: cannot initialise by PCA")
    p0 = DFMHip.pca_init(h, Float64.(rbal), ru)
    N = size(z, 2)
    Lam_u = Matrix{Float64}(undef, N, ru); R = Vector{Float64}(undef, N)
    Lam_u[balmask, :] = p0.Lam; R[balmask] = p0.R
    gap = findall(.!balmask)
    if !isempty(gap)
        o = DFMHip.ols(h, p0.F, og.resid[:, gap])
        Lam_u[gap, :] = permutedims(o.beta); R[gap] = o.ssr ./ max.(o.nobs, 1)
    end
    fit = DFMHip.em_obs(h, z, G, (Lam = hcat(permutedims(og.beta), Lam_u), R = R, A = p0.A, Q = p0.Q, mu0 = p0.mu0, P0 = p0.P0);
                        max_iter = max_em_iter, tol = tol_em)
    m.factor[m.initperiod:m.lastperiod, ro+1:end] = fit.factor               # in place (aliases factor_var_model.y, :80)
    cols = findall(incl)[enough]
    m.lambda[cols, :] = fit.Lam .* xsd
    m.uar_ser[cols] = sqrt.(fit.R) .* xsd
    m.uar_coef[cols, :] .= 0.0
    common = hcat(G, fit.factor) * fit.Lam'
    m.fes.ssr = sum(abs2, [isnan(z[t, i]) ? 0.0 : z[t, i] - common[t, i] for t in 1:size(z, 1), i in 1:N])
    estimate_var!(m.factor_var_model)                                          # VAR of (g, f): the reference's second stage (:444-492)
    return fit.loglik
end
