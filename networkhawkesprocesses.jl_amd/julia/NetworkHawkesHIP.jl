# NetworkHawkesHIP.jl -- the reference-side binding of libnhp.so (include/nhp.h, ABI 2).
#
# Drop-in for the hot path only: `using NetworkHawkesProcesses; include("NetworkHawkesHIP.jl")` gives GPU methods with
# the package's own names, argument meaning, keyword arguments and result structs
#     loglikelihood / intensity / resample_parents / mle! / mcmc!                (src/continuous.jl, src/parents.jl)
#     convolve / intensity / loglikelihood / update! / vb! / mle! / mcmc!        (src/discrete.jl, src/inference.jl)
# that take the package's process structs and data and `ccall` the C ABI.  Nothing else of the package changes.
# Julia is not installed in the build image, so this file is NOT executed by the test-suite; every entry point it binds
# is exercised through the identical ctypes binding (networkhawkesprocesses.jl_amd/_lib.py), and the struct layouts it
# assumes are checked against the loaded library when the module initialises (ABI_LAYOUT below; the same numbers are
# asserted from ctypes in tests/test_abi_and_host.py).  Keep it declarative: all logic lives behind the C ABI.
module NetworkHawkesHIP

using NetworkHawkesProcesses
import Optim                      # already a dependency of NetworkHawkesProcesses (Project.toml)
const NHP = NetworkHawkesProcesses

const libnhp = get(ENV, "NHP_LIB", joinpath(@__DIR__, "..", "libnhp.so"))

# sizeof / offsetof of nhp_cont_model_desc (80 bytes), nhp_gibbs_priors (64), nhp_cont_stats (40), then NHP_MAX_SLOTS and
# NHP_COMM_ID_BYTES -- what nhp_abi_layout() of the library must return for the structs below to be passed by reference
const ABI_LAYOUT = Int32[80, 0, 4, 8, 16, 24, 28, 32, 40, 48, 56, 64, 72,
                         64, 0, 8, 16, 24, 32, 40, 48, 56,
                         40, 0, 8, 16, 24, 32,
                         4096, 128]

function __init__()
    v = ccall((:nhp_abi_version, libnhp), Int32, ())
    v == 2 || error("libnhp.so has ABI version $v, this binding expects 2")
    got = zeros(Int32, 64)
    n = ccall((:nhp_abi_layout, libnhp), Int32, (Ptr{Int32}, Int32), got, 64)
    got[1:n] == ABI_LAYOUT || error("struct layout mismatch between NetworkHawkesHIP.jl and libnhp.so: $(got[1:n])")
    sizeof(ModelDesc) == 80 && sizeof(Priors) == 64 && sizeof(Stats) == 40 || error("Julia struct sizes differ from the C ABI")
end

# --- status -> exception (include/nhp.h: nhp_status) ---------------------------------------
function check(rc::Int32, ctx::Ptr{Cvoid}=C_NULL)
    rc == 0 && return
    msg = unsafe_string(ccall((:nhp_last_error, libnhp), Cstring, (Ptr{Cvoid},), ctx))
    rc == 2 && throw(DomainError(msg))            # NHP_EDOMAIN  (src/baselines.jl:100,106,111,116)
    rc == 3 && error(msg)                         # NHP_ESHAPE   (src/impulses.jl:44-45, src/weights.jl:10-11)
    rc == 1 && throw(ArgumentError(msg))          # NHP_EINVAL
    error("libnhp status $rc: $msg")              # NHP_ENOMEM / NHP_EHIP / NHP_ENOTIMPL / NHP_ERCCL
end

mutable struct Context
    h::Ptr{Cvoid}
    function Context(device::Integer=parse(Int, get(ENV, "NHP_DEVICE", get(ENV, "LOCAL_RANK", "0"))))
        r = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:nhp_ctx_create, libnhp), Int32, (Int32, Ref{Ptr{Cvoid}}), device, r))
        ctx = new(r[])
        finalizer(c -> ccall((:nhp_ctx_destroy, libnhp), Cvoid, (Ptr{Cvoid},), c.h), ctx)
    end
end
const DEFAULT = Ref{Union{Nothing,Context}}(nothing)
context() = (DEFAULT[] === nothing && (DEFAULT[] = Context()); DEFAULT[])

# --- nhp_cont_model_desc: the lowered (Baseline, ImpulseResponse, Weights, A); offsets in ABI_LAYOUT[2:13] -----------
struct ModelDesc
    n_nodes::Int32; baseline_kind::Int32; lambda0::Ptr{Float64}; grid_x::Ptr{Float64}
    grid_n::Int32; impulse_kind::Int32; theta::Ptr{Float64}; mu::Ptr{Float64}; tau::Ptr{Float64}
    dt_max::Float64; W::Ptr{Float64}; A::Ptr{Float64}
end
struct Priors   # nhp_gibbs_priors; offsets in ABI_LAYOUT[15:22]
    α0::Float64; β0::Float64; κ::Float64; ν::Float64; a::Float64; b::Float64; μμ::Float64; κμ::Float64
end
struct Stats    # nhp_cont_stats; offsets in ABI_LAYOUT[24:28]
    cnt0::Ptr{Float64}; Mn::Ptr{Float64}; Mnm::Ptr{Float64}; Xnm::Ptr{Float64}; Vnm::Ptr{Float64}
end

# Julia arrays are already column-major [parent, child]: pointers are passed untouched.
function lower(p::NHP.ContinuousHawkesProcess)
    keep = Any[]
    f64(x) = (a = Array{Float64}(x); push!(keep, a); pointer(a))
    N = NHP.ndims(p)
    if p.baseline isa NHP.HomogeneousProcess
        bk, l0, gx, gn = Int32(0), f64(p.baseline.λ), Ptr{Float64}(C_NULL), Int32(0)
    else   # LogGaussianCoxProcess evaluator: grid x, λ[k] per node (src/baselines.jl:148-173)
        bk, l0, gx, gn = Int32(1), f64(vcat(p.baseline.λ...)), f64(p.baseline.x), Int32(length(p.baseline.x))
    end
    nul = Ptr{Float64}(C_NULL)
    if p.impulses isa NHP.ExponentialImpulseResponse
        ik, th, mu, tau = Int32(0), f64(p.impulses.θ), nul, nul
    else
        ik, th, mu, tau = Int32(1), nul, f64(p.impulses.μ), f64(p.impulses.τ)
    end
    A = p isa NHP.ContinuousNetworkHawkesProcess ? f64(p.adjacency_matrix) : nul
    ModelDesc(N, bk, l0, gx, gn, ik, th, mu, tau, Float64(p.impulses.Δtmax), f64(p.weights.W), A), keep
end

mutable struct Dataset          # (events, nodes, duration) uploaded once; pre-pass for Δtmax done
    h::Ptr{Cvoid}
end
# columns = 1-based node range this process evaluates (one loglikelihood / chain over several GPUs: `comm` keyword of the
# entry points below); the default is the whole dataset.  build = :host (the pre-pass on the host) or :device (on the
# GPU, nhp_cont_dataset_create_device: the same dataset, byte for byte)
function Dataset(ctx::Context, data, N::Integer, Δtmax::Real; columns::UnitRange{Int}=1:N, build::Symbol=:host)
    events, nodes, duration = data
    ev, nd = Vector{Float64}(events), Vector{Int64}(nodes)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    if build === :device
        GC.@preserve ev nd check(ccall((:nhp_cont_dataset_create_device, libnhp), Int32,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Int64, Int32, Float64, Float64, Int32, Int32, Int32, Ref{Ptr{Cvoid}}),
            ctx.h, ev, nd, length(ev), N, duration, Δtmax, first(columns) - 1, last(columns), Int32(0), r), ctx.h)
    elseif build === :host
        GC.@preserve ev nd check(ccall((:nhp_cont_dataset_create_columns, libnhp), Int32,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Int64, Int32, Float64, Float64, Int32, Int32, Ref{Ptr{Cvoid}}),
            ctx.h, ev, nd, length(ev), N, duration, Δtmax, first(columns) - 1, last(columns), r), ctx.h)
    else
        throw(ArgumentError("build must be :host or :device"))
    end
    ds = Dataset(r[])
    finalizer(d -> ccall((:nhp_cont_dataset_destroy, libnhp), Cvoid, (Ptr{Cvoid},), d.h), ds)
end

# Several independent trials [(events_r, nodes_r, T_r), ...] over the same nodes as ONE dataset (DESIGN §3.26): stacked along
# one clock, trial r on [o_r, o_r + T_r]; no look-back window crosses a trial's first event.  The shift rounds every time
# once: a delay inside a trial changes by at most one ulp of ΣT_r.
function stack_event_trials(trials)
    R = length(trials)
    f, o = zeros(Int64, R + 1), zeros(Float64, R + 1)
    ev, nd = Float64[], Int64[]
    for (r, (e, n, T)) in enumerate(trials)
        (isfinite(T) && T > 0) || throw(DomainError(T, "trial $r: duration must be positive and finite"))
        length(e) == length(n) || throw(ArgumentError("trial $r: events and nodes must have the same length"))
        issorted(e) || throw(ArgumentError("trial $r: events must be sorted"))
        all(t -> 0 <= t <= T, e) || throw(DomainError(T, "trial $r: events must lie in [0, $T]"))
        append!(ev, e .+ o[r]); append!(nd, n)
        f[r + 1], o[r + 1] = f[r] + length(e), o[r] + T
    end
    (events=ev, nodes=nd, duration=o[end], event_offsets=f, time_offsets=o)
end
function Dataset(ctx::Context, trials::AbstractVector{<:Tuple}, N::Integer, Δtmax::Real; build::Symbol=:host)
    build in (:host, :device) || throw(ArgumentError("build must be :host or :device"))
    s = stack_event_trials(trials)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    ev, nd, f, o = s.events, s.nodes, s.event_offsets, s.time_offsets
    GC.@preserve ev nd f o check(ccall((:nhp_cont_dataset_create_trials, libnhp), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Int64, Int32, Ptr{Int64}, Ptr{Float64}, Int32, Float64, Int32, Ref{Ptr{Cvoid}}),
        ctx.h, ev, nd, length(ev), N, f, o, length(trials), Δtmax, Int32(build === :device ? 1 : 0), r), ctx.h)
    ds = Dataset(r[])
    finalizer(d -> ccall((:nhp_cont_dataset_destroy, libnhp), Cvoid, (Ptr{Cvoid},), d.h), ds)
end
# (event_offsets, time_offsets, first_positive) of a dataset; one recording is one trial
function trial_offsets(ds::Dataset)
    n = Ref{Int32}(0)
    check(ccall((:nhp_cont_dataset_get_trials, libnhp), Int32, (Ptr{Cvoid}, Ref{Int32}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
                ds.h, n, Ptr{Int64}(C_NULL), Ptr{Float64}(C_NULL), Ptr{Int64}(C_NULL)))
    f, o, g = zeros(Int64, n[] + 1), zeros(Float64, n[] + 1), zeros(Int64, n[])
    check(ccall((:nhp_cont_dataset_get_trials, libnhp), Int32, (Ptr{Cvoid}, Ref{Int32}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
                ds.h, n, f, o, g))
    f, o, g
end

function with_model(f, ctx::Context, p)
    desc, keep = lower(p)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve keep begin
        check(ccall((:nhp_cont_model_create, libnhp), Int32, (Ptr{Cvoid}, Ref{ModelDesc}, Ref{Ptr{Cvoid}}),
                    ctx.h, Ref(desc), r), ctx.h)
    end
    try f(r[]) finally ccall((:nhp_cont_model_destroy, libnhp), Cvoid, (Ptr{Cvoid},), r[]) end
end

llflags(p, recursive) = Int32(recursive && p.impulses isa NHP.ExponentialImpulseResponse ? 1 : 0)

# ---- several GPUs: RCCL over xGMI through the library (include/nhp.h, multi-GPU section) ------------------------------
# Rank 0: id = unique_id(); ship the 128 bytes to the other ranks (Distributed.remotecall, a file, MPI.bcast ...); every
# rank: comm = Comm(ctx, id, rank, world).  `comm` is then a keyword of loglikelihood / loglikelihood_gradient / mle! /
# mcmc! (ONE evaluation or chain over all ranks, each its column range), and gather_moments collects the independent
# chains of BASELINE config 5.
mutable struct Comm
    h::Ptr{Cvoid}; rank::Int; world::Int
end
function unique_id()
    id = zeros(UInt8, 128)
    check(ccall((:nhp_comm_unique_id, libnhp), Int32, (Ptr{UInt8},), id))
    id
end
function Comm(ctx::Context, id::Vector{UInt8}, rank::Integer, world::Integer)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:nhp_comm_create, libnhp), Int32, (Ptr{Cvoid}, Ptr{UInt8}, Int32, Int32, Ref{Ptr{Cvoid}}), ctx.h, id, rank, world, r), ctx.h)
    c = Comm(r[], rank, world)
    finalizer(x -> ccall((:nhp_comm_destroy, libnhp), Cvoid, (Ptr{Cvoid},), x.h), c)
end
commptr(c) = c === nothing ? Ptr{Cvoid}(C_NULL) : c.h
function allreduce_sum!(x::Vector{Float64}, comm::Comm; ctx=context())
    check(ccall((:nhp_allreduce_sum, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64), ctx.h, comm.h, x, length(x)), ctx.h)
    x
end

# --- loglikelihood(process, data; recursive=true)  src/continuous.jl:210,360 ----------------
function loglikelihood(p::NHP.ContinuousHawkesProcess, data; recursive=true, ctx=context(), comm=nothing,
                       ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    ll = Ref{Float64}(0.0)
    with_model(ctx, p) do m
        if comm === nothing
            check(ccall((:nhp_cont_loglik, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{Float64}),
                        ctx.h, ds.h, m, llflags(p, recursive), ll), ctx.h)
        else    # ds is this rank's column shard: partial results summed on the device over RCCL
            check(ccall((:nhp_cont_loglik_allreduce, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{Float64}),
                        ctx.h, comm.h, ds.h, m, llflags(p, recursive), ll), ctx.h)
        end
    end
    ll[]
end

# --- intensity(process, data, times) -> length(times) x N; intensity(process, data, time) -> N  src/continuous.jl:76-96
function intensity(p::NHP.ContinuousHawkesProcess, data, times::Vector{Float64}; ctx=context(),
                   ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    out = Matrix{Float64}(undef, length(times), NHP.ndims(p))
    with_model(ctx, p) do m
        check(ccall((:nhp_cont_intensity, libnhp), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}),
                    ctx.h, ds.h, m, times, length(times), out), ctx.h)
    end
    out
end
intensity(p::NHP.ContinuousHawkesProcess, data, time::Float64; kw...) = vec(intensity(p, data, [time]; kw...))

# --- resample_parents(process, data) -> (parents, parentnodes)  src/parents.jl:1-23 ----------
# stats=true also returns the Gibbs sufficient statistics of the same sweep (src/parents.jl:61-79, src/baselines.jl:87-96,
# src/impulses.jl:84-96,216-252) as a NamedTuple of N / N x N Float64 arrays.
function resample_parents(p::NHP.ContinuousHawkesProcess, data; seed::UInt64=UInt64(0), step::UInt64=UInt64(0), stats=false,
                          ctx=context(), ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    M, N = length(data[1]), NHP.ndims(p)
    parents, parentnodes = Vector{Int64}(undef, M), Vector{Int64}(undef, M)
    cnt0, Mn, Mnm, Xnm, Vnm = zeros(N), zeros(N), zeros(N, N), zeros(N, N), zeros(N, N)
    st = Ref(Stats(pointer(cnt0), pointer(Mn), pointer(Mnm), pointer(Xnm), pointer(Vnm)))
    with_model(ctx, p) do m
        GC.@preserve st cnt0 Mn Mnm Xnm Vnm check(ccall((:nhp_cont_resample_parents, libnhp), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, UInt64, UInt64, Ptr{Int64}, Ptr{Int64}, Ptr{Cvoid}),
                    ctx.h, ds.h, m, C_NULL, seed, step, parents, parentnodes, stats ? Base.unsafe_convert(Ptr{Cvoid}, st) : C_NULL), ctx.h)
    end
    stats ? (parents, parentnodes, (cnt0=cnt0, Mn=Mn, Mnm=Mnm, Xnm=Xnm, Vnm=Vnm)) : (parents, parentnodes)
end

# --- rand(process, duration) -> (events, nodes, duration)  src/continuous.jl:16-48,131-142,335-348 ---------------------
# The GPU generator (Philox-keyed by `seed`: same law as the package's rand, not Julia's random stream).  device=false
# defers to the package's own rand.  More than max_events kept events: ErrorException "branching process exploded".
function rand(p::NHP.ContinuousHawkesProcess, duration::Float64; device::Bool=true, seed::Integer=0,
              max_events::Integer=5_000_000, ctx=context())
    device || return NHP.rand(p, duration)
    times, nodes, n = Vector{Float64}(undef, max(max_events, 1)), Vector{Int64}(undef, max(max_events, 1)), Ref{Int64}(0)
    with_model(ctx, p) do m
        check(ccall((:nhp_cont_simulate, libnhp), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Float64, UInt64, Int64, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ref{Int64}),
                    ctx.h, m, duration, seed % UInt64, max_events, Int32(0), times, nodes, C_NULL, n), ctx.h)
    end
    times[1:n[]], nodes[1:n[]], duration
end

# --- rand(process, steps) -> N x steps counts  src/discrete.jl:20-38 ---------------------------------------------------
# The discrete branching sampler on the GPU (nhp_disc_simulate; same law, Philox-keyed by `seed`).  background=true also
# returns the immigrants alone (parents[:, :, 1] of the augmented model, as N x steps).  A DiscreteLogGaussianCoxProcess
# baseline enters as its per-bin means intensity(baseline, 1:steps).
function rand(p::NHP.DiscreteHawkesProcess, steps::Int64; device::Bool=true, seed::Integer=0, max_events::Integer=50_000_000,
              background::Bool=false, ctx=context())
    device || return NHP.rand(p, steps)
    steps >= 1 || error("steps must be positive")
    N = NHP.ndims(p)
    lgcp = p.baseline isa NHP.DiscreteLogGaussianCoxProcess
    lgcp && (1 >= p.baseline.x[1] && steps <= p.baseline.x[end] || error("Sample duration does not match process duration."))
    l0 = lgcp ? nothing : Vector{Float64}(p.baseline.λ)
    base = lgcp ? Matrix{Float64}(NHP.intensity(p.baseline, Float64.(1:steps))) : nothing          # T x N, t fastest
    W, θ = Matrix{Float64}(p.weights.W), Array{Float64,3}(p.impulses.θ)
    A = p isa NHP.DiscreteNetworkHawkesProcess ? Matrix{Float64}(p.adjacency_matrix) : nothing
    phi = basis_matrix(p.impulses)
    L, B = size(phi)
    counts, n = Matrix{Int64}(undef, N, steps), Ref{Int64}(0)
    bg = background ? Matrix{Int64}(undef, N, steps) : nothing
    GC.@preserve l0 base A bg check(ccall((:nhp_disc_simulate, libnhp), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Float64, Int32,
         Int64, UInt64, Int64, Int32, Ptr{Int64}, Ptr{Int64}, Ref{Int64}, Ptr{Int32}),
        ctx.h, aptr(l0), aptr(base), W, θ, aptr(A), phi, L, B, p.dt, N, steps, seed % UInt64, max_events, Int32(0), counts,
        bg === nothing ? Ptr{Int64}(C_NULL) : pointer(bg), n, Ptr{Int32}(C_NULL)), ctx.h)
    background ? (counts, bg) : counts
end

# --- compensator(process, data) -> (at_events, residuals, total): no reference counterpart ------------------------------
# The exact integral Λ_c(t) of the intensity of src/continuous.jl:84-96 (the reference's own integral term is "approximate
# (exact requires cdf)", src/continuous.jl:247): at_events[k] = Λ_{n_k}(t_k), residuals[k] = its increment since the previous
# event of node n_k (Exp(1) under the true model: time rescaling), total[c] = Λ_c(duration), the expected count of node c.
function compensator(p::NHP.ContinuousHawkesProcess, data; ctx=context(), ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    M, N = length(data[1]), NHP.ndims(p)
    at_events, residuals, total = Vector{Float64}(undef, M), Vector{Float64}(undef, M), Vector{Float64}(undef, N)
    with_model(ctx, p) do m
        check(ccall((:nhp_cont_compensator, libnhp), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    ctx.h, ds.h, m, Int32(0), at_events, residuals, total), ctx.h)
    end
    (at_events=at_events, residuals=residuals, total=total)
end

# --- map_parents(process, data) -> (parents, parentnodes, prob): no reference counterpart --------------------------------
# The posterior-mode parent of every event over the categories resample_parents draws from (the events of the look-back
# window, most recent first, then the baseline) and its posterior probability w_max / Σw.  parents[i] = 0 (baseline) or the
# 1-based event index; the first maximum wins (of equal parent weights the most recent, a parent before the baseline).
function map_parents(p::NHP.ContinuousHawkesProcess, data; ctx=context(), ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    M = length(data[1])
    parents, parentnodes, prob = Vector{Int64}(undef, M), Vector{Int64}(undef, M), Vector{Float64}(undef, M)
    with_model(ctx, p) do m
        check(ccall((:nhp_cont_map_parents, libnhp), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}),
                    ctx.h, ds.h, m, Int32(0), parents, parentnodes, prob), ctx.h)
    end
    (parents=parents, parentnodes=parentnodes, prob=prob)
end

# --- cascades(process, data; parents=:map) -> NamedTuple: no reference counterpart ---------------------------------------
# The forest a parent assignment forms: parents = :map (map_parents), :sample (one draw of resample_parents with `seed`) or
# a Vector{Int64} of length M (0 = immigrant, else the 1-based index of an earlier event; anything else: DomainError).
# Per event root, generation, descendants; per cascade (ascending root) cascade_root, cascade_size, cascade_depth,
# cascade_end; per node immigrants, offspring and reach[p, c] = events on node c whose root is on node p.
function cascades(p::NHP.ContinuousHawkesProcess, data; parents=:map, seed::Integer=0, ctx=context(),
                  ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    M, N = length(data[1]), NHP.ndims(p)
    if parents isa Symbol
        parents in (:map, :sample) || throw(ArgumentError("parents must be :map, :sample or a Vector{Int64} of length $M"))
        par = parents == :map ? map_parents(p, data; ctx=ctx, ds=ds).parents : resample_parents(p, data; seed=seed % UInt64, ctx=ctx, ds=ds)[1]
    else
        eltype(parents) <: Integer || throw(ArgumentError("parents must hold integers"))
        length(parents) == M || throw(ArgumentError("parents must hold one entry per event: expected length $M, got $(length(parents))"))
        par = Vector{Int64}(parents)
    end
    root, generation, descendants = Vector{Int64}(undef, M), Vector{Int64}(undef, M), Vector{Int64}(undef, M)
    croot, csize, cdepth, cend = Vector{Int64}(undef, M), Vector{Int64}(undef, M), Vector{Int64}(undef, M), Vector{Float64}(undef, M)
    immigrants, offspring, reach = Vector{Int64}(undef, N), Vector{Int64}(undef, N), Matrix{Int64}(undef, N, N)
    n, rounds = Ref{Int64}(0), Ref{Int32}(0)
    check(ccall((:nhp_cont_cascades, libnhp), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Int32, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64},
                 Ptr{Float64}, Ref{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ref{Int32}),
                ctx.h, ds.h, par, Int32(0), Int32(0), root, generation, descendants, croot, csize, cdepth, cend, n, immigrants, offspring,
                reach, rounds), ctx.h)
    k = n[]
    (parents=par, root=root, generation=generation, descendants=descendants, cascade_root=croot[1:k], cascade_size=csize[1:k],
     cascade_depth=cdepth[1:k], cascade_end=cend[1:k], immigrants=immigrants, offspring=offspring, reach=reach, rounds=Int(rounds[]))
end

# --- forecast(process, data, horizon) -> (counts, carry, paths): no reference counterpart -------------------------------
# nsamples independent continuations of data = (events, nodes, T) on (T, T + horizon], conditional on the observed events,
# under the generative model of rand (exponential delays not cut at Δtmax, W·A expected children per link; not the
# likelihood's convention): counts is nsamples x N, carry[c] the expected number of carry-over events of node c, paths
# (with paths=true) = (times, nodes, offsets), replica r owning offsets[r]+1 : offsets[r+1] of the absolute, ascending times
# and the 1-based nodes.  Homogeneous baselines only.  More than max_events events in all: "branching process exploded".
function forecast(p::NHP.ContinuousHawkesProcess, data, horizon::Real; nsamples::Integer=1000, seed::Integer=0, paths::Bool=false,
                  max_events::Integer=5_000_000, ctx=context(), ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    N, S = NHP.ndims(p), Int(nsamples)
    counts, carry = Matrix{Int64}(undef, N, max(S, 0)), Vector{Float64}(undef, N)      # column r = replica r (replica-major in memory)
    cap = max(max_events, 1)
    times, nodes = paths ? (Vector{Float64}(undef, cap), Vector{Int64}(undef, cap)) : (Float64[], Int64[])
    offsets = paths ? Vector{Int64}(undef, S + 1) : Int64[]
    with_model(ctx, p) do m
        check(ccall((:nhp_cont_forecast, libnhp), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Int32, UInt64, Int64, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Float64},
                     Ptr{Int64}, Ptr{Int64}, Ptr{Float64}),
                    ctx.h, ds.h, m, Float64(horizon), Int32(S), seed % UInt64, max_events, Int32(0), carry, counts,
                    paths ? times : C_NULL, paths ? nodes : C_NULL, paths ? offsets : C_NULL, C_NULL), ctx.h)
    end
    n = paths ? offsets[end] : 0
    (counts=permutedims(counts), carry=carry, paths=paths ? (times[1:n], nodes[1:n], offsets) : nothing)
end

# --- forecast(process::DiscreteHawkesProcess, data, horizon): no reference counterpart -----------------------------------
# nsamples independent continuations of the N x T0 count matrix over the next `horizon` bins, conditional on the observed
# counts, under the law of rand (nhp_disc_forecast): totals is nsamples x N, mean / expected / carry are N x horizon (the
# ensemble mean per cell, the exact predictive mean, the expected carry-over children of the observed events), paths (with
# paths=true) is N x horizon x nsamples.  Only the last nlags bins of data are read.  A DiscreteLogGaussianCoxProcess grid
# must reach T0 + horizon.  More than max_events events in all replicas: "branching process exploded".
function forecast(p::NHP.DiscreteHawkesProcess, data::Matrix{Int64}, horizon::Integer; nsamples::Integer=1000, seed::Integer=0,
                  paths::Bool=false, max_events::Integer=50_000_000, ctx=context())
    N, T0 = size(data)
    N == NHP.ndims(p) && T0 >= 1 || error("data must be an N x T matrix with N = $(NHP.ndims(p)) rows and at least one bin")
    H, S = Int64(horizon), Int64(nsamples)
    H >= 1 && S >= 1 || error("horizon and nsamples must be positive")
    all(>=(0), data) || throw(DomainError(minimum(data), "counts must be non-negative"))
    lgcp = p.baseline isa NHP.DiscreteLogGaussianCoxProcess
    lgcp && (T0 + 1 >= p.baseline.x[1] && T0 + H <= p.baseline.x[end] || error("Sample duration does not match process duration."))
    l0 = lgcp ? nothing : Vector{Float64}(p.baseline.λ)
    base = lgcp ? Matrix{Float64}(NHP.intensity(p.baseline, Float64.(T0+1:T0+H))) : nothing        # H x N, k fastest
    W, θ = Matrix{Float64}(p.weights.W), Array{Float64,3}(p.impulses.θ)
    A = p isa NHP.DiscreteNetworkHawkesProcess ? Matrix{Float64}(p.adjacency_matrix) : nothing
    phi = basis_matrix(p.impulses)
    L, B = size(phi)
    tail = Matrix{Int64}(data[:, max(1, T0 - L + 1):T0])                 # N x Tu, node fastest
    totals, cell = Matrix{Int64}(undef, N, S), Matrix{Int64}(undef, N, H)  # column r = replica r, column k = bin k
    carry, expected = Matrix{Float64}(undef, N, H), Matrix{Float64}(undef, N, H)
    pth = paths ? Array{Int64,3}(undef, N, H, S) : nothing
    n, gens = Ref{Int64}(0), Ref{Int32}(0)
    GC.@preserve l0 base A pth check(ccall((:nhp_disc_forecast, libnhp), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Float64, Int32,
         Ptr{Int64}, Int64, Int32, Int64, Int64, UInt64, Int64, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64},
         Ref{Int64}, Ref{Int32}),
        ctx.h, aptr(l0), aptr(base), W, θ, aptr(A), phi, L, B, p.dt, N, tail, size(tail, 2), Int32(0), H, S, seed % UInt64, max_events,
        Int32(0), totals, cell, pth === nothing ? Ptr{Int64}(C_NULL) : pointer(pth), carry, expected, n, gens), ctx.h)
    (totals=permutedims(totals), mean=cell ./ S, expected=expected, carry=carry, paths=pth, events=n[], generations=Int(gens[]))
end

# --- objective + analytic gradient of mle!  src/continuous.jl:144-198 -------------------------------------------------
function loglikelihood_gradient(p::NHP.ContinuousStandardHawkesProcess, data; recursive=true, ctx=context(), comm=nothing,
                                ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    P = length(NHP.params(p))
    g, ll = Vector{Float64}(undef, P), Ref{Float64}(0.0)
    with_model(ctx, p) do m
        grad_call(ctx, comm, ds, m, llflags(p, recursive), ll, g)
    end
    ll[], g
end
function grad_call(ctx, comm, ds, m, flags, ll, g)
    if comm === nothing
        check(ccall((:nhp_cont_loglik_grad, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{Float64}, Ptr{Float64}, Int64),
                    ctx.h, ds.h, m, flags, ll, g, length(g)), ctx.h)
    else
        check(ccall((:nhp_cont_loglik_grad_allreduce, libnhp), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{Float64}, Ptr{Float64}, Int64),
                    ctx.h, comm.h, ds.h, m, flags, ll, g, length(g)), ctx.h)
    end
end

# loglikelihood(process::LogGaussianCoxProcess, data, node, y) for every node at once
# (src/baselines.jl:247-254): Y is G x N, column c the candidate latent curve of node c.
# `parentnodes === nothing` reuses the attribution the latest resample_parents left on the device.
function lgcp_loglikelihood(b::NHP.LogGaussianCoxProcess, ds::Dataset, Y::Matrix{Float64};
                            parentnodes::Union{Nothing,Vector{Int64}}=nothing, ctx=context())
    lam = exp.(b.m .+ Y)
    ll = Vector{Float64}(undef, size(Y, 2))
    pn = parentnodes === nothing ? Ptr{Int64}(C_NULL) : pointer(parentnodes)
    GC.@preserve parentnodes lam ll check(ccall((:nhp_cont_lgcp_loglik, libnhp), Int32,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
        ctx.h, ds.h, pn, b.x, Int32(length(b.x)), lam, ll), ctx.h)
    ll
end

# ---- the reference's mle! driver around an objective/gradient pair ---------------------------------------------------
# Same keyword arguments, box, callback logic, printed banners and result struct as src/continuous.jl:144-198 and
# src/discrete.jl:211-296 (`max_increase_steps` is the discrete method's extra stop rule; `nothing` = not used).
# `fg!(G, x)` returns -loglikelihood [- logprior] and fills G with its gradient; the reference hands Optim no gradient
# (2P objective calls per finite-difference gradient), here it is analytic and comes from the same GPU call.
function run_mle(fg!, guess; optimizer, verbose, f_abstol, max_increase_steps=nothing)
    minloss, outer_iter, converged, steps, increase_steps = Inf, 0, false, 0, 0
    function banner(o, what)
        println("\n* Status: $what criteria reached!")
        println("    elapsed: $(o.metadata["time"])")
        println("    final loss: $(o.value)")
        println("    min. loss: $(minloss)")
        println("    outer iterations: $outer_iter")
        println("    inner iterations: $(o.iteration)\n")
    end
    function status_update(o)
        if o.iteration == 0
            verbose && println("* iteration (n=$outer_iter)")
            outer_iter += 1
            minloss = Inf
        end
        verbose && println(" > step: $(o.iteration), loss: $(o.value), elapsed: $(o.metadata["time"])")
        if abs(o.value - minloss) < f_abstol
            converged = true; steps = o.iteration
            banner(o, "f_abstol convergence")
            return true
        elseif max_increase_steps !== nothing && o.value > minloss
            increase_steps += 1
            if increase_steps >= max_increase_steps
                converged = true; steps = o.iteration
                banner(o, "loss increase")
                return true
            end
        else
            minloss = o.value
            increase_steps = 0
        end
        return false
    end
    lower, upper = fill(1e-6, size(guess)), fill(1e1, size(guess))
    res = Optim.optimize(Optim.only_fg!((F, G, x) -> fg!(G, x)), lower, upper, guess, Optim.Fminbox(optimizer()),
                         Optim.Options(callback=status_update))
    NHP.MaximumLikelihood(res.minimizer, -res.minimum, steps, res.time_run, converged ? "success" : "failure")
end

# d/dx of logprior(process) (src/continuous.jl:278-284) in params! order [λ0; θ | μ; τ; W]: the Gamma / normal-gamma
# log-densities of src/baselines.jl:120-122, src/impulses.jl:110-112,254-259, src/weights.jl:66-68 differentiated
function logprior_gradient(p::NHP.ContinuousStandardHawkesProcess)
    b, w, imp = p.baseline, p.weights, p.impulses
    g = [(b.α0 - 1) ./ b.λ .- b.β0]
    if imp isa NHP.ExponentialImpulseResponse
        push!(g, vec((imp.α - 1) ./ imp.θ .- imp.β))
    else
        push!(g, vec(-imp.κμ .* imp.τ .* (imp.μ .- imp.μμ)))
        push!(g, vec((imp.α0 - 1) ./ imp.τ .- imp.β0 .+ 0.5 ./ imp.τ .- 0.5 .* imp.κμ .* (imp.μ .- imp.μμ) .^ 2))
    end
    push!(g, vec((w.κ - 1) ./ w.W .- w.ν))
    vcat(g...)
end

# --- mle!(process, data; optimizer=BFGS, verbose=false, f_abstol=1e-6, regularize=false, guess=nothing)
#     -> MaximumLikelihood   src/continuous.jl:144-198 ------------------------------------------------------------
# Extra keywords (not in the reference): recursive (the loglikelihood dispatch), ctx / ds / comm (device handles), max_steps
# and optimizer=:device (the whole iteration inside the library, nhp_cont_mle_run).
function mle!(p::NHP.ContinuousStandardHawkesProcess, data; optimizer=Optim.BFGS, verbose=false, f_abstol=1e-6, regularize=false,
              guess=nothing, recursive=true, ctx=context(), comm=nothing, max_steps=1000,
              ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    guess = guess === nothing ? NHP._rand_init_(p) : guess
    P = length(guess)
    flags = llflags(p, recursive)
    if optimizer === :device
        # the optimizer's state on the device (nhp_cont_mle_run: projected L-BFGS in HBM on the same box [1e-6, 10], the same
        # |f_k - f_{k-1}| < f_abstol rule; the host reads scalars).  At 2.1e6 parameters one step costs milliseconds instead
        # of the parameter upload + gradient download + host-side quasi-Newton update of the Optim route.
        regularize && error("optimizer=:device minimises -loglikelihood only; use an Optim optimizer with regularize=true")
        x = clamp.(Vector{Float64}(guess), 1e-6, 1e1)
        loss, steps, conv, evals = Ref{Float64}(0.0), Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0)
        t0 = time()
        with_model(ctx, p) do m
            check(ccall((:nhp_cont_mle_run, libnhp), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float64, Float64, Float64, Int32, Ptr{Float64}, Int64,
                 Ref{Float64}, Ref{Int32}, Ref{Int32}, Ref{Int32}),
                ctx.h, comm === nothing ? C_NULL : comm.h, ds.h, m, flags, 1e-6, 1e1, f_abstol, Int32(max_steps), x, P,
                loss, steps, conv, evals), ctx.h)
        end
        verbose && println(" > steps: $(steps[]), objective evaluations: $(evals[]), loss: $(loss[])")
        NHP.params!(p, x)
        return NHP.MaximumLikelihood(x, -loss[], Int(steps[]), time() - t0, conv[] == 1 ? "success" : "failure")
    end
    res = with_model(ctx, p) do m
        ll, g = Ref{Float64}(0.0), Vector{Float64}(undef, P)
        function fg!(G, x)
            # params!(process, x) straight into the device-resident model (x already is the column-major parameter vector)
            check(ccall((:nhp_cont_model_set_params, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64), ctx.h, m, x, P), ctx.h)
            grad_call(ctx, comm, ds, m, flags, ll, g)
            f = -ll[]
            if regularize
                NHP.params!(p, x)
                f -= NHP.logprior(p)
                g .+= logprior_gradient(p)
            end
            G === nothing || (G .= .-g)
            f
        end
        run_mle(fg!, guess; optimizer=optimizer, verbose=verbose, f_abstol=f_abstol)
    end
    NHP.params!(p, res.maximizer)                      # "all inference methods overwrite model parameters"
    res
end

# --- expected_statistics(process, data) and em!(process, data; ...) -> MaximumLikelihood: no reference counterpart --------
# The expected branching structure (one E-step, nhp_cont_em_stats) and the expectation-maximisation fit with the whole
# iteration on the device (nhp_cont_em_run): mle!'s objective, box [1e-6, 10], start and |f - f_prev| < f_abstol rule; the
# M-step is closed-form in every coordinate (with the package's priors too: regularize=true), no step lowers the objective.
# S2 (logit-normal only) is centred at the current μ: Σ r (z - μ)².
function expected_statistics(p::NHP.ContinuousStandardHawkesProcess, data; recursive=true, ctx=context(),
                             ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    N = NHP.ndims(p)
    ln = !(p.impulses isa NHP.ExponentialImpulseResponse)
    ll, bg = Ref{Float64}(0.0), Vector{Float64}(undef, N)
    EM, S1, S2 = Matrix{Float64}(undef, N, N), Matrix{Float64}(undef, N, N), Matrix{Float64}(undef, N, N)
    with_model(ctx, p) do m
        check(ccall((:nhp_cont_em_stats, libnhp), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ref{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    ctx.h, ds.h, m, llflags(p, recursive), Int32(0), ll, bg, EM, S1, ln ? pointer(S2) : Ptr{Float64}(C_NULL)), ctx.h)
    end
    (ll=ll[], bg=bg, EM=EM, S1=S1, S2=ln ? S2 : nothing)
end

function em!(p::NHP.ContinuousStandardHawkesProcess, data; max_steps=1000, f_abstol=1e-6, regularize=false, guess=nothing,
             recursive=true, verbose=false, ctx=context(), keep_trace=false,
             ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    p.baseline isa NHP.HomogeneousProcess || error("em!: the M-step of a LogGaussianCoxProcess baseline has no closed form")
    guess = guess === nothing ? NHP._rand_init_(p) : guess
    x = clamp.(Vector{Float64}(guess), 1e-6, 1e1)
    P = length(x)
    P == length(NHP.params(p)) || error("Parameter vector length does not match model parameter length.")
    loss, steps, conv = Ref{Float64}(0.0), Ref{Int32}(0), Ref{Int32}(0)
    trace = fill(NaN, max_steps + 1)
    pri = Ref(priors(p))
    t0 = time()
    with_model(ctx, p) do m
        GC.@preserve pri check(ccall((:nhp_cont_em_run, libnhp), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Priors}, Float64, Float64, Float64, Int32, Ptr{Float64}, Int64,
             Ref{Float64}, Ref{Int32}, Ref{Int32}, Ptr{Float64}),
            ctx.h, ds.h, m, llflags(p, recursive), regularize ? Base.unsafe_convert(Ptr{Priors}, pri) : Ptr{Priors}(C_NULL),
            1e-6, 1e1, f_abstol, Int32(max_steps), x, P, loss, steps, conv, trace), ctx.h)
    end
    verbose && println(" > steps: $(steps[]), loss: $(loss[])")
    NHP.params!(p, x)
    res = NHP.MaximumLikelihood(x, -loss[], Int(steps[]), time() - t0, conv[] == 1 ? "success" : "failure")
    keep_trace ? (res, trace[1:steps[]+1]) : res
end

# --- vb!(process, data; ...) and update!(process, data; state) for the continuous standard process: no reference counterpart ---
# Mean-field variational inference under the process's own priors (nhp_cont_vb_run / nhp_cont_vb_step; the definition is in
# include/nhp.h): one Gamma factor per entry of λ0, W and θ, one normal-gamma factor per (μ, τ), held in two planes S (shape-like)
# and R (rate-like) in params! order.  vb! returns (S, R, elbo, trace, steps, status, elapsed) and overwrites the process with
# the posterior means; state=(S, R) resumes.  update! is one step from a state, or from the process's current parameters
# (state=nothing), and returns (S, R, stats) with the nine numbers of nhp_cont_vb_step; the process is not changed.
const VB_RESUME, VB_FROM_MODEL = Int32(256), Int32(512)

function vb!(p::NHP.ContinuousStandardHawkesProcess, data; max_steps=1000, f_abstol=1e-6, guess=nothing, recursive=true,
             state=nothing, verbose=false, ctx=context(), ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    p.baseline isa NHP.HomogeneousProcess || error("vb!: the M-step of a LogGaussianCoxProcess baseline has no closed form")
    P = length(NHP.params(p))
    x = Vector{Float64}(guess === nothing ? NHP.params(p) : guess)
    length(x) == P || error("Parameter vector length does not match model parameter length.")
    S, R = state === nothing ? (Vector{Float64}(undef, P), Vector{Float64}(undef, P)) : (Vector{Float64}(state[1]), Vector{Float64}(state[2]))
    (length(S) == P && length(R) == P) || error("Parameter vector length does not match model parameter length.")
    flags = llflags(p, recursive) | (state === nothing ? Int32(0) : VB_RESUME)
    elbo, steps, conv = Ref{Float64}(0.0), Ref{Int32}(0), Ref{Int32}(0)
    trace = fill(NaN, max_steps + 1)
    pri = Ref(priors(p))
    t0 = time()
    state === nothing && NHP.params!(p, x)
    with_model(ctx, p) do m
        GC.@preserve pri check(ccall((:nhp_cont_vb_run, libnhp), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Priors}, Float64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64,
             Ref{Float64}, Ref{Int32}, Ref{Int32}, Ptr{Float64}),
            ctx.h, ds.h, m, flags, Base.unsafe_convert(Ptr{Priors}, pri), f_abstol, Int32(max_steps), x, S, R, P, elbo, steps, conv,
            trace), ctx.h)
    end
    verbose && println(" > steps: $(steps[]), elbo: $(elbo[])")
    NHP.params!(p, x)
    first = state === nothing ? 2 : 1
    (S=S, R=R, elbo=elbo[], trace=trace[first:steps[]+1], steps=Int(steps[]), status=conv[] == 1 ? "success" : "failure",
     elapsed=time() - t0)
end

function update!(p::NHP.ContinuousStandardHawkesProcess, data; state=nothing, recursive=true, ctx=context(),
                 ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    P = length(NHP.params(p))
    S, R = state === nothing ? (Vector{Float64}(undef, P), Vector{Float64}(undef, P)) : (Vector{Float64}(state[1]), Vector{Float64}(state[2]))
    (length(S) == P && length(R) == P) || error("Parameter vector length does not match model parameter length.")
    flags = llflags(p, recursive) | (state === nothing ? VB_FROM_MODEL : Int32(0))
    stats = Vector{Float64}(undef, 9)
    pri = Ref(priors(p))
    with_model(ctx, p) do m
        GC.@preserve pri check(ccall((:nhp_cont_vb_step, libnhp), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Priors}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Ptr{Float64}),
            ctx.h, ds.h, m, flags, Base.unsafe_convert(Ptr{Priors}, pri), S, R, P, Int32(0), stats), ctx.h)
    end
    (S=S, R=R, stats=stats)
end

# --- vb!(process, data; ...) and update!(process, data; state) for the continuous NETWORK process: no reference counterpart ---
# Spike-and-slab weights (SparseWeightModel) under a DenseNetworkModel or BernoulliNetworkModel (nhp_cont_netvb_run /
# nhp_cont_netvb_step; the definition is in include/nhp.h).  The state is (S, R, Q): the standard fit's planes in the device
# order [λ0; impulses; W] with the slab's (κv1, νv1) in the W block, and Q = [κv0; νv0; ρv; αv; βv] (3N² + 2).  vb! returns
# (S, R, Q, rho, elbo, trace, steps, status, elapsed) and overwrites the process: posterior means, weights.W = κv1/νv1,
# adjacency_matrix = (ρv > ½), network.ρ = αv/(αv + βv) with αv, βv, and the weights' variational tables.  update! is one step
# and returns (S, R, Q, stats) with the eleven numbers of nhp_cont_netvb_step; the process is not changed.
const VB_DENSE_NETWORK = Int32(1024)

function netvb_setup(p::NHP.ContinuousNetworkHawkesProcess, what)
    p.weights isa NHP.SparseWeightModel || throw(ArgumentError("$what on a ContinuousNetworkHawkesProcess needs a SparseWeightModel"))
    p.baseline isa NHP.HomogeneousProcess || error("$what: the update of a LogGaussianCoxProcess baseline has no closed form")
    dense = p.network isa NHP.DenseNetworkModel
    (dense || p.network isa NHP.BernoulliNetworkModel) || error("$what: only DenseNetworkModel and BernoulliNetworkModel are implemented")
    w, imp, b = p.weights, p.impulses, p.baseline
    pri = imp isa NHP.ExponentialImpulseResponse ? Priors(b.α0, b.β0, w.κ1, w.ν1, imp.α, imp.β, 0.0, 1.0) :
                                                   Priors(b.α0, b.β0, w.κ1, w.ν1, imp.α0, imp.β0, imp.μμ, imp.κμ)
    net = Float64[w.κ0, w.ν0, dense ? 1.0 : p.network.α, dense ? 1.0 : p.network.β]
    N = NHP.ndims(p)
    P = N + N * N * (imp isa NHP.ExponentialImpulseResponse ? 2 : 3)
    pri, net, dense, N, P
end

# Q of a start without a state.  A run or a step from a guess reads of it the pair (αv, βv) alone (include/nhp.h): the three
# planes are output only there, so the ρv plane written here (the network's link probability, where the Python front end
# takes weights.ρv when it is set) never enters a result.
function netvb_start_Q(p, dense, N)
    rho = dense ? ones(N, N) : fill(Float64(p.network.ρ), N, N)
    vcat(ones(2 * N * N), vec(rho), dense ? [1.0, 1.0] : Float64[p.network.αv, p.network.βv])
end

function vb!(p::NHP.ContinuousNetworkHawkesProcess, data; max_steps=1000, f_abstol=1e-6, guess=nothing, recursive=true,
             state=nothing, verbose=false, ctx=context(), ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    pri0, net, dense, N, P = netvb_setup(p, "vb!")
    x = Vector{Float64}(guess === nothing ? vcat(NHP.params(p.baseline), NHP.params(p.impulses), NHP.params(p.weights)) : guess)
    length(x) == P || error("Parameter vector length does not match model parameter length.")
    S, R, Q = state === nothing ? (Vector{Float64}(undef, P), Vector{Float64}(undef, P), netvb_start_Q(p, dense, N)) :
                                  (Vector{Float64}(state[1]), Vector{Float64}(state[2]), Vector{Float64}(state[3]))
    (length(S) == P && length(R) == P && length(Q) == 3 * N * N + 2) || error("Parameter vector length does not match model parameter length.")
    flags = llflags(p, recursive) | (state === nothing ? Int32(0) : VB_RESUME) | (dense ? VB_DENSE_NETWORK : Int32(0))
    elbo, steps, conv = Ref{Float64}(0.0), Ref{Int32}(0), Ref{Int32}(0)
    trace = fill(NaN, max_steps + 1)
    pri = Ref(pri0)
    t0 = time()
    with_model(ctx, p) do m
        GC.@preserve pri check(ccall((:nhp_cont_netvb_run, libnhp), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Priors}, Ptr{Float64}, Float64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Int64, Ptr{Float64}, Ref{Float64}, Ref{Int32}, Ref{Int32}, Ptr{Float64}),
            ctx.h, ds.h, m, flags, Base.unsafe_convert(Ptr{Priors}, pri), net, f_abstol, Int32(max_steps), x, S, R, P, Q, elbo, steps, conv,
            trace), ctx.h)
    end
    verbose && println(" > steps: $(steps[]), elbo: $(elbo[])")
    NN = N * N
    nimp = P - N - NN
    NHP.params!(p.baseline, x[1:N]); NHP.params!(p.impulses, x[N+1:N+nimp]); NHP.params!(p.weights, x[N+nimp+1:end])
    tab(v, j) = reshape(v[(j-1)*NN+1:j*NN], N, N)
    rho = tab(Q, 3)
    w = p.weights
    w.κv0, w.νv0, w.κv1, w.νv1 = tab(Q, 1), tab(Q, 2), reshape(S[P-NN+1:P], N, N), reshape(R[P-NN+1:P], N, N)
    p.adjacency_matrix .= rho .> 0.5
    if !dense
        p.network.αv, p.network.βv = Q[end-1], Q[end]
        p.network.ρ = Q[end-1] / (Q[end-1] + Q[end])
    end
    first = state === nothing ? 2 : 1
    (S=S, R=R, Q=Q, rho=rho, elbo=elbo[], trace=trace[first:steps[]+1], steps=Int(steps[]), status=conv[] == 1 ? "success" : "failure",
     elapsed=time() - t0)
end

function update!(p::NHP.ContinuousNetworkHawkesProcess, data; state=nothing, recursive=true, ctx=context(),
                 ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    pri0, net, dense, N, P = netvb_setup(p, "update!")
    S, R, Q = state === nothing ? (Vector{Float64}(undef, P), Vector{Float64}(undef, P), netvb_start_Q(p, dense, N)) :
                                  (Vector{Float64}(state[1]), Vector{Float64}(state[2]), Vector{Float64}(state[3]))
    (length(S) == P && length(R) == P && length(Q) == 3 * N * N + 2) || error("Parameter vector length does not match model parameter length.")
    flags = llflags(p, recursive) | (state === nothing ? VB_FROM_MODEL : Int32(0)) | (dense ? VB_DENSE_NETWORK : Int32(0))
    stats = Vector{Float64}(undef, 11)
    pri = Ref(pri0)
    with_model(ctx, p) do m
        GC.@preserve pri check(ccall((:nhp_cont_netvb_step, libnhp), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Priors}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Int32,
             Ptr{Float64}),
            ctx.h, ds.h, m, flags, Base.unsafe_convert(Ptr{Priors}, pri), net, S, R, P, Q, Int32(0), stats), ctx.h)
    end
    (S=S, R=R, Q=Q, stats=stats)
end

# ... under a STOCHASTIC BLOCK network (nhp_cont_sbmvb_run / nhp_cont_sbmvb_step; the definition is in include/nhp.h).  The
# reference package has no block model type, so the caller passes the priors sbm = (α, β, γ), the number of blocks and the
# block state B = [vec αv; vec βv; γv; vec m] (2K² + K + N·K, column-major; m[n, :] on the simplex and not uniform: the uniform
# state is a fixed point of the label update).  Q holds the three planes [κv0; νv0; ρv] (3N²).  The label sweep runs at the
# steps whose number step0 + 1, step0 + 2, ... is a multiple of labels_every.  block_vb! returns (S, R, Q, B, rho, m, elbo,
# trace, steps, status, elapsed) and overwrites the process as vb! does (p.network is not touched); block_update! is one step
# and returns (S, R, Q, B, stats) with the 21 numbers of nhp_cont_sbmvb_step; the process is not changed.
function sbmvb_setup(p::NHP.ContinuousNetworkHawkesProcess, what, sbm, n_blocks, B)
    p.weights isa NHP.SparseWeightModel || throw(ArgumentError("$what on a ContinuousNetworkHawkesProcess needs a SparseWeightModel"))
    p.baseline isa NHP.HomogeneousProcess || error("$what: the update of a LogGaussianCoxProcess baseline has no closed form")
    w, imp, b = p.weights, p.impulses, p.baseline
    pri = imp isa NHP.ExponentialImpulseResponse ? Priors(b.α0, b.β0, w.κ1, w.ν1, imp.α, imp.β, 0.0, 1.0) :
                                                   Priors(b.α0, b.β0, w.κ1, w.ν1, imp.α0, imp.β0, imp.μμ, imp.κμ)
    N = NHP.ndims(p)
    P = N + N * N * (imp isa NHP.ExponentialImpulseResponse ? 2 : 3)
    K = Int(n_blocks)
    1 <= K <= 64 || error("$what: n_blocks must lie in 1..64")
    length(B) == 2 * K * K + K + N * K || error("$what: B must hold 2K² + K + N·K numbers")
    length(sbm) == 3 || error("$what: sbm = (α, β, γ)")
    pri, Float64[w.κ0, w.ν0], Float64[sbm...], N, P, K
end

function block_vb!(p::NHP.ContinuousNetworkHawkesProcess, data, sbm, n_blocks, B; labels_every=1, step0=0, max_steps=1000, f_abstol=1e-6,
                   guess=nothing, recursive=true, state=nothing, verbose=false, ctx=context(),
                   ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    pri0, net, sb, N, P, K = sbmvb_setup(p, "vb!", sbm, n_blocks, B)
    x = Vector{Float64}(guess === nothing ? vcat(NHP.params(p.baseline), NHP.params(p.impulses), NHP.params(p.weights)) : guess)
    length(x) == P || error("Parameter vector length does not match model parameter length.")
    NN = N * N
    S, R, Q = state === nothing ? (Vector{Float64}(undef, P), Vector{Float64}(undef, P), vcat(ones(2 * NN), fill(0.5, NN))) :
                                  (Vector{Float64}(state[1]), Vector{Float64}(state[2]), Vector{Float64}(state[3]))
    (length(S) == P && length(R) == P && length(Q) == 3 * NN) || error("Parameter vector length does not match model parameter length.")
    Bv = Vector{Float64}(B)
    flags = llflags(p, recursive) | (state === nothing ? Int32(0) : VB_RESUME)
    elbo, steps, conv = Ref{Float64}(0.0), Ref{Int32}(0), Ref{Int32}(0)
    trace = fill(NaN, max_steps + 1)
    pri = Ref(pri0)
    t0 = time()
    with_model(ctx, p) do m
        GC.@preserve pri check(ccall((:nhp_cont_sbmvb_run, libnhp), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Priors}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Int64, Float64, Int32,
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ref{Int32}, Ref{Int32}, Ptr{Float64}),
            ctx.h, ds.h, m, flags, Base.unsafe_convert(Ptr{Priors}, pri), net, sb, Int32(K), Int32(labels_every), Int64(step0), f_abstol,
            Int32(max_steps), x, S, R, P, Q, Bv, elbo, steps, conv, trace), ctx.h)
    end
    verbose && println(" > steps: $(steps[]), elbo: $(elbo[])")
    nimp = P - N - NN
    NHP.params!(p.baseline, x[1:N]); NHP.params!(p.impulses, x[N+1:N+nimp]); NHP.params!(p.weights, x[N+nimp+1:end])
    tab(v, j) = reshape(v[(j-1)*NN+1:j*NN], N, N)
    rho = tab(Q, 3)
    w = p.weights
    w.κv0, w.νv0, w.κv1, w.νv1 = tab(Q, 1), tab(Q, 2), reshape(S[P-NN+1:P], N, N), reshape(R[P-NN+1:P], N, N)
    p.adjacency_matrix .= rho .> 0.5
    first = state === nothing ? 2 : 1
    (S=S, R=R, Q=Q, B=Bv, rho=rho, m=reshape(Bv[2*K*K+K+1:end], N, K), elbo=elbo[], trace=trace[first:steps[]+1], steps=Int(steps[]),
     status=conv[] == 1 ? "success" : "failure", elapsed=time() - t0)
end

function block_update!(p::NHP.ContinuousNetworkHawkesProcess, data, sbm, n_blocks, B; labels_every=1, step0=0, state=nothing, recursive=true,
                       ctx=context(), ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    pri0, net, sb, N, P, K = sbmvb_setup(p, "update!", sbm, n_blocks, B)
    NN = N * N
    S, R, Q = state === nothing ? (Vector{Float64}(undef, P), Vector{Float64}(undef, P), vcat(ones(2 * NN), fill(0.5, NN))) :
                                  (Vector{Float64}(state[1]), Vector{Float64}(state[2]), Vector{Float64}(state[3]))
    (length(S) == P && length(R) == P && length(Q) == 3 * NN) || error("Parameter vector length does not match model parameter length.")
    Bv = Vector{Float64}(B)
    flags = llflags(p, recursive) | (state === nothing ? VB_FROM_MODEL : Int32(0))
    stats = Vector{Float64}(undef, 21)
    pri = Ref(pri0)
    with_model(ctx, p) do m
        GC.@preserve pri check(ccall((:nhp_cont_sbmvb_step, libnhp), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Priors}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Int64, Ptr{Float64}, Ptr{Float64},
             Int64, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}),
            ctx.h, ds.h, m, flags, Base.unsafe_convert(Ptr{Priors}, pri), net, sb, Int32(K), Int32(labels_every), Int64(step0), S, R, P, Q, Bv,
            Int32(0), stats), ctx.h)
    end
    (S=S, R=R, Q=Q, B=Bv, stats=stats)
end

# ... under a LATENT DISTANCE network (nhp_cont_latvb_run / nhp_cont_latvb_step; the definition is in include/nhp.h).  The reference
# package has no latent distance model type either, so the caller passes the priors lat = (σ, μb, σb), the positions z (N x D, rows
# not all equal: equal positions are a saddle of the ascent) and the offset b; Z = [vec z; b].  Q holds the three planes
# [κv0; νv0; ρv] (3N²).  latent_vb! returns (S, R, Q, Z, rho, z, b, elbo, trace, steps, status, elapsed) and overwrites the process
# as vb! does (p.network is not touched); latent_update! is one step and returns (S, R, Q, Z, stats) with the 19 + ascent_steps
# numbers of nhp_cont_latvb_step; the process is not changed.  latent_expected_loglik is nhp_latent_expected_loglik: (F, ∇F).
function latvb_setup(p::NHP.ContinuousNetworkHawkesProcess, what, lat, z, b, ascent_steps)
    p.weights isa NHP.SparseWeightModel || throw(ArgumentError("$what on a ContinuousNetworkHawkesProcess needs a SparseWeightModel"))
    p.baseline isa NHP.HomogeneousProcess || error("$what: the update of a LogGaussianCoxProcess baseline has no closed form")
    w, imp, bl = p.weights, p.impulses, p.baseline
    pri = imp isa NHP.ExponentialImpulseResponse ? Priors(bl.α0, bl.β0, w.κ1, w.ν1, imp.α, imp.β, 0.0, 1.0) :
                                                   Priors(bl.α0, bl.β0, w.κ1, w.ν1, imp.α0, imp.β0, imp.μμ, imp.κμ)
    N = NHP.ndims(p)
    P = N + N * N * (imp isa NHP.ExponentialImpulseResponse ? 2 : 3)
    size(z, 1) == N || error("$what: z must have one row per node")
    D = size(z, 2)
    1 <= D <= 8 || error("$what: the latent dimension must lie in 1..8")
    0 <= ascent_steps <= 64 || error("$what: ascent_steps must lie in 0..64")
    length(lat) == 3 || error("$what: lat = (σ, μb, σb)")
    pri, Float64[w.κ0, w.ν0], Float64[lat...], N, P, D, vcat(vec(Matrix{Float64}(z)), Float64(b))
end

function latent_vb!(p::NHP.ContinuousNetworkHawkesProcess, data, lat, z, b; ascent_steps=4, max_steps=1000, f_abstol=1e-6, guess=nothing,
                    recursive=true, state=nothing, verbose=false, ctx=context(), ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    pri0, net, la, N, P, D, Z = latvb_setup(p, "vb!", lat, z, b, ascent_steps)
    x = Vector{Float64}(guess === nothing ? vcat(NHP.params(p.baseline), NHP.params(p.impulses), NHP.params(p.weights)) : guess)
    length(x) == P || error("Parameter vector length does not match model parameter length.")
    NN = N * N
    S, R, Q = state === nothing ? (Vector{Float64}(undef, P), Vector{Float64}(undef, P), vcat(ones(2 * NN), fill(0.5, NN))) :
                                  (Vector{Float64}(state[1]), Vector{Float64}(state[2]), Vector{Float64}(state[3]))
    (length(S) == P && length(R) == P && length(Q) == 3 * NN) || error("Parameter vector length does not match model parameter length.")
    flags = llflags(p, recursive) | (state === nothing ? Int32(0) : VB_RESUME)
    elbo, steps, conv = Ref{Float64}(0.0), Ref{Int32}(0), Ref{Int32}(0)
    trace = fill(NaN, max_steps + 1)
    pri = Ref(pri0)
    t0 = time()
    with_model(ctx, p) do m
        GC.@preserve pri check(ccall((:nhp_cont_latvb_run, libnhp), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Priors}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Float64, Int32,
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ref{Int32}, Ref{Int32}, Ptr{Float64}),
            ctx.h, ds.h, m, flags, Base.unsafe_convert(Ptr{Priors}, pri), net, la, Int32(D), Int32(ascent_steps), f_abstol,
            Int32(max_steps), x, S, R, P, Q, Z, elbo, steps, conv, trace), ctx.h)
    end
    verbose && println(" > steps: $(steps[]), elbo: $(elbo[])")
    nimp = P - N - NN
    NHP.params!(p.baseline, x[1:N]); NHP.params!(p.impulses, x[N+1:N+nimp]); NHP.params!(p.weights, x[N+nimp+1:end])
    tab(v, j) = reshape(v[(j-1)*NN+1:j*NN], N, N)
    rho = tab(Q, 3)
    w = p.weights
    w.κv0, w.νv0, w.κv1, w.νv1 = tab(Q, 1), tab(Q, 2), reshape(S[P-NN+1:P], N, N), reshape(R[P-NN+1:P], N, N)
    p.adjacency_matrix .= rho .> 0.5
    first = state === nothing ? 2 : 1
    (S=S, R=R, Q=Q, Z=Z, rho=rho, z=reshape(Z[1:N*D], N, D), b=Z[end], elbo=elbo[], trace=trace[first:steps[]+1], steps=Int(steps[]),
     status=conv[] == 1 ? "success" : "failure", elapsed=time() - t0)
end

function latent_update!(p::NHP.ContinuousNetworkHawkesProcess, data, lat, z, b; ascent_steps=4, state=nothing, recursive=true,
                        ctx=context(), ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    pri0, net, la, N, P, D, Z = latvb_setup(p, "update!", lat, z, b, ascent_steps)
    NN = N * N
    S, R, Q = state === nothing ? (Vector{Float64}(undef, P), Vector{Float64}(undef, P), vcat(ones(2 * NN), fill(0.5, NN))) :
                                  (Vector{Float64}(state[1]), Vector{Float64}(state[2]), Vector{Float64}(state[3]))
    (length(S) == P && length(R) == P && length(Q) == 3 * NN) || error("Parameter vector length does not match model parameter length.")
    flags = llflags(p, recursive) | (state === nothing ? VB_FROM_MODEL : Int32(0))
    stats = Vector{Float64}(undef, 19 + ascent_steps)
    pri = Ref(pri0)
    with_model(ctx, p) do m
        GC.@preserve pri check(ccall((:nhp_cont_latvb_step, libnhp), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Priors}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64},
             Int64, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}),
            ctx.h, ds.h, m, flags, Base.unsafe_convert(Ptr{Priors}, pri), net, la, Int32(D), Int32(ascent_steps), S, R, P, Q, Z,
            Int32(0), stats), ctx.h)
    end
    (S=S, R=R, Q=Q, Z=Z, stats=stats)
end

function latent_expected_loglik(rho::AbstractMatrix, z::AbstractMatrix, b, lat; ctx=context())
    N, D = size(z)
    size(rho) == (N, N) || error("rho must be N x N")
    out = Vector{Float64}(undef, N * D + 2)
    check(ccall((:nhp_latent_expected_loglik, libnhp), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}),
                ctx.h, Matrix{Float64}(rho), Int32(N), Int32(D), Matrix{Float64}(z), Float64(b), Float64[lat...], out), ctx.h)
    (F=out[1], grad=out[2:end])
end

# --- observed_information(process, data) and hessian_vector_product(process, data, v): no reference counterpart ---------------
# The objective separates by child node, so minus its Hessian is block diagonal: blocks[:, :, k] is the D x D block of column
# columns[k] (1-based here) over [λ0[c]; θ[:,c] | μ[:,c]; τ[:,c]; W[:,c]], D = 1 + kinds·N (nhp_cont_information; homogeneous
# baseline).  hessian_vector_product returns H·v (the Hessian itself) in params! order (nhp_cont_hessian_vec).  recursive=true
# sums every earlier event through the truncated windows of loglikelihood and errors where there is none.
function observed_information(p::NHP.ContinuousHawkesProcess, data; columns=nothing, recursive=true, tile_nodes=0, ctx=context(),
                              ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    N = NHP.ndims(p)
    kinds = p.impulses isa NHP.ExponentialImpulseResponse ? 2 : 3
    D = 1 + kinds * N
    cols = columns === nothing ? collect(1:N) : collect(Int, columns)
    c0 = Vector{Int32}(cols .- 1)
    ll, blocks = Ref{Float64}(0.0), Array{Float64}(undef, D, D, length(cols))
    with_model(ctx, p) do m
        check(ccall((:nhp_cont_information, libnhp), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Int32}, Int32, Int32, Int32, Ref{Float64}, Ptr{Float64}),
                    ctx.h, ds.h, m, llflags(p, recursive), c0, Int32(length(c0)), Int32(tile_nodes), Int32(0), ll, blocks), ctx.h)
    end
    (ll=ll[], columns=cols, blocks=blocks)
end

function hessian_vector_product(p::NHP.ContinuousHawkesProcess, data, v::AbstractVector; recursive=true, ctx=context(),
                                ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    x = Vector{Float64}(v)
    out = similar(x)
    with_model(ctx, p) do m
        check(ccall((:nhp_cont_hessian_vec, libnhp), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int64),
                    ctx.h, ds.h, m, llflags(p, recursive), Int32(0), x, out, length(x)), ctx.h)
    end
    out
end

# --- mcmc!(process, data; nsteps=1000, log_freq=100, verbose=false) -> MarkovChainMonteCarlo  src/inference.jl:49-70
# A sweep -- parents, sufficient statistics, conjugate draws, (network) adjacency sweep and ρ -- stays on the device
# (nhp_cont_gibbs_step / nhp_cont_network_step); `push!(res.samples, params(process))` downloads the parameters every
# step exactly as the reference keeps them.  Extra keywords: seed (keys every Philox stream: reproducible chains,
# independent across seeds), keep_samples=false runs the chain inside the library (nhp_cont_mcmc_run: one
# synchronisation per log_freq steps, posterior moments accumulated on the device and returned by `moments`),
# ctx / ds / comm.  Draws are distributionally, not bitwise, those of Julia's samplers.
priors(p) = p.impulses isa NHP.ExponentialImpulseResponse ?
    Priors(p.baseline.α0, p.baseline.β0, p.weights.κ, p.weights.ν, p.impulses.α, p.impulses.β, 0.0, 1.0) :
    Priors(p.baseline.α0, p.baseline.β0, p.weights.κ, p.weights.ν, p.impulses.α0, p.impulses.β0, p.impulses.μμ, p.impulses.κμ)

function pull!(p::NHP.ContinuousHawkesProcess, ctx, m)     # device-resident model -> the mutable component structs
    N = NHP.ndims(p)
    nimp = N * N * (p.impulses isa NHP.ExponentialImpulseResponse ? 1 : 2)
    x = Vector{Float64}(undef, N + nimp + N * N)
    check(ccall((:nhp_cont_model_get_params, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64), ctx.h, m, x, length(x)), ctx.h)
    NHP.params!(p.baseline, x[1:N]); NHP.params!(p.impulses, x[N+1:N+nimp]); NHP.params!(p.weights, x[N+nimp+1:end])
    if p isa NHP.ContinuousNetworkHawkesProcess
        A = Matrix{Float64}(undef, N, N)
        check(ccall((:nhp_cont_model_get_adjacency, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64), ctx.h, m, A, N * N), ctx.h)
        p.adjacency_matrix = A
        if p.network isa NHP.BernoulliNetworkModel
            r = zeros(3)
            check(ccall((:nhp_cont_model_get_rho, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}), ctx.h, m, r), ctx.h)
            p.network.ρ = r[1]
        end
    end
end

# moments=true: the chain's posterior sums over the steps >= burn are kept on the device (nhp_cont_model_moments_*, what
# `gather_moments` exchanges between chains) and come back as the second value: (res, (sum, sumsq, count, rho)) -- fetched
# before the device model is released.  Without it no sum is accumulated (burn = -1 to the library).
# diagnostics=true (with moments=true): batch-means ESS, MCSE and split R-hat are accumulated in the same pass
# (nhp_cont_model_diagnostics_configure before the chain, batch_len = max(1, isqrt(nsteps - burn)) unless given) and a third
# value follows: (summary, batch_len), summary the 9 x 6 matrix of nhp_cont_model_diagnostics_fetch -- fields x groups
# (λ0, θ | μ, τ, W, vec(A), ρ), include/nhp.h; group-relative indices are 0-based as the library returns them.
function mcmc!(p::NHP.ContinuousHawkesProcess, data; nsteps=1000, log_freq=100, verbose=false, seed::UInt64=UInt64(0),
               keep_samples=true, moments=false, burn::Integer=0, ctx=context(), comm=nothing,
               diagnostics=false, batch_len::Integer=max(1, isqrt(max(0, nsteps - burn))), ess_below=100.0, rhat_above=1.01,
               ds=Dataset(ctx, data, NHP.ndims(p), p.impulses.Δtmax))
    p.baseline isa NHP.HomogeneousProcess || error("mcmc! on the device draws the homogeneous baseline; use the package's mcmc! with an LGCP baseline")
    diagnostics && !moments && throw(ArgumentError("diagnostics need the device-side running sums (moments=true)"))
    diagnostics && comm !== nothing && error("convergence diagnostics are not available for a sharded chain")
    res = NHP.MarkovChainMonteCarlo(p)
    mom = nothing
    diag = nothing
    start_time = time()
    network = p isa NHP.ContinuousNetworkHawkesProcess
    bern = network && p.network isa NHP.BernoulliNetworkModel
    na, nb = bern ? (Float64(p.network.α), Float64(p.network.β)) : (0.0, 0.0)      # 0, 0: ρ held at 1 (DenseNetworkModel)
    pr = Ref(priors(p))
    with_model(ctx, p) do m
        network && check(ccall((:nhp_cont_model_set_rho, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Float64), ctx.h, m, bern ? p.network.ρ : 1.0), ctx.h)
        check(ccall((:nhp_cont_model_diagnostics_configure, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64), ctx.h, m,
                    diagnostics ? Int64(batch_len) : Int64(0), diagnostics ? Int64(max(0, nsteps - burn)) : Int64(0)), ctx.h)
        moments && check(ccall((:nhp_cont_model_moments_reset, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.h, m), ctx.h)
        while res.steps < nsteps
            n = keep_samples ? 1 : min(nsteps - res.steps, verbose ? log_freq : nsteps)
            check(ccall((:nhp_cont_mcmc_run, libnhp), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Priors}, Float64, Float64, UInt64, UInt64, Int64, Int64),
                        ctx.h, commptr(comm), ds.h, m, pr, na, nb, seed, UInt64(res.steps), n, moments ? Int64(burn) : Int64(-1)), ctx.h)
            res.steps += n
            if keep_samples || res.steps == nsteps
                pull!(p, ctx, m)
                keep_samples && push!(res.samples, NHP.params(p))
            end
            if res.steps % log_freq == 0 && verbose
                res.elapsed = time() - start_time
                println(" > step: $(res.steps), elapsed: $(res.elapsed)")
            end
        end
        if moments                                          # while the model is alive
            N = NHP.ndims(p)
            len = N + N * N * (p.impulses isa NHP.ExponentialImpulseResponse ? 1 : 2) + N * N + (network ? N * N : 0)
            s, q, cnt, rho = Vector{Float64}(undef, len), Vector{Float64}(undef, len), Ref{Int64}(0), zeros(3)
            check(ccall((:nhp_cont_model_moments_fetch, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ref{Int64}),
                        ctx.h, m, s, q, len, cnt), ctx.h)
            network && check(ccall((:nhp_cont_model_get_rho, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}), ctx.h, m, rho), ctx.h)
            mom = (s, q, cnt[], rho)
            if diagnostics && cnt[] >= 1
                summary = Matrix{Float64}(undef, 9, 6)
                check(ccall((:nhp_cont_model_diagnostics_fetch, libnhp), Int32,
                            (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64),
                            ctx.h, m, Float64(ess_below), Float64(rhat_above), summary, C_NULL, C_NULL, C_NULL, len), ctx.h)
                diag = (summary, Int(batch_len))
            end
        end
    end
    res.elapsed = time() - start_time
    return diagnostics ? (res, mom, diag) : moments ? (res, mom) : res
end

# --- streaming quantiles of a device-resident chain (include/nhp.h: nhp_cont_model_quantiles_*, nhp_disc_model_quantiles_*) ----
# Credible intervals with no sample kept: the extended P² markers of every parameter entry sit next to a device model `m`
# (with_model / a discrete model handle; discrete=true picks the nhp_disc_model_* entries).  Configure before the chain's first
# kept step (with moments: nhp_*_mcmc_run then feeds every `every`-th kept step itself; a step-by-step driver calls
# quantiles_accumulate! after its moments accumulate) and fetch while the model is alive.  `len` is the sums' length;
# values is len x m (column j: the estimate of probs[j]), NaN at vec(A) and, while count < 2m + 3, everywhere; min and max are
# exact; rho = (the m estimates, min, max) of a Bernoulli network's scalar ρ, NaN otherwise.
function quantiles_configure!(ctx, m, probs; every::Integer=1, effective_weights::Bool=false, discrete::Bool=false)
    p = collect(Float64, probs)
    if discrete
        check(ccall((:nhp_disc_model_quantiles_configure, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Int32),
                    ctx.h, m, p, Int32(length(p)), Int32(every), Int32(effective_weights)), ctx.h)
    else
        check(ccall((:nhp_cont_model_quantiles_configure, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Int32),
                    ctx.h, m, p, Int32(length(p)), Int32(every), Int32(effective_weights)), ctx.h)
    end
end

quantiles_off!(ctx, m; discrete::Bool=false) = quantiles_configure!(ctx, m, Float64[]; discrete=discrete)

function quantiles_accumulate!(ctx, m; discrete::Bool=false)
    if discrete
        check(ccall((:nhp_disc_model_quantiles_accumulate, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.h, m), ctx.h)
    else
        check(ccall((:nhp_cont_model_quantiles_accumulate, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.h, m), ctx.h)
    end
end

function quantiles_fetch(ctx, m, nprobs::Integer, len::Integer; discrete::Bool=false)
    values, lo, hi = Matrix{Float64}(undef, len, nprobs), Vector{Float64}(undef, len), Vector{Float64}(undef, len)
    rho, cnt = Vector{Float64}(undef, nprobs + 2), Ref{Int64}(0)
    if discrete
        check(ccall((:nhp_disc_model_quantiles_fetch, libnhp), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ref{Int64}),
                    ctx.h, m, values, lo, hi, rho, Int64(len), cnt), ctx.h)
    else
        check(ccall((:nhp_cont_model_quantiles_fetch, libnhp), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ref{Int64}),
                    ctx.h, m, values, lo, hi, rho, Int64(len), cnt), ctx.h)
    end
    return (values, lo, hi, rho, cnt[])
end

# --- StochasticBlockNetworkModel: the reference names it and leaves an empty stub (src/networks.jl, last lines) -------------
# z_n ~ Categorical(π), π ~ Dirichlet(γ), ρ[k,l] ~ Beta(α, β), A[p,c] ~ Bernoulli(ρ[z_p, z_c]); labels are 1-based here and
# 0-based in the library.  resample!(net, A) runs on the GPU through the stand-alone entries (csrc/sbm.hip); set_sbm! /
# get_sbm! / sbm_step! keep the state next to a device model `m` (with_model), where nhp_cont_mcmc_run takes the block-model
# network step by itself.  Block labels are identified only up to a permutation: a chain can switch them.
mutable struct StochasticBlockNetworkModel
    nnodes::Int; nblocks::Int
    ρ::Matrix{Float64}; π::Vector{Float64}; z::Vector{Int}
    α::Float64; β::Float64; γ::Float64
end
StochasticBlockNetworkModel(nnodes, nblocks; ρ=fill(0.5, nblocks, nblocks), π=fill(1 / nblocks, nblocks),
                            z=[mod(n - 1, nblocks) + 1 for n in 1:nnodes], α=1.0, β=1.0, γ=1.0) =
    StochasticBlockNetworkModel(nnodes, nblocks, ρ, π, z, α, β, γ)
NHP.params(net::StochasticBlockNetworkModel) = [vec(net.ρ); net.π]
link_probability(net::StochasticBlockNetworkModel) = net.ρ[net.z, net.z]

function block_counts(net::StochasticBlockNetworkModel, A::Matrix{Float64}; ctx=context())
    K = net.nblocks
    z0, L, n = Int32.(net.z .- 1), Matrix{Int64}(undef, K, K), Vector{Int64}(undef, K)
    check(ccall((:nhp_sbm_block_counts, libnhp), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}),
                ctx.h, A, net.nnodes, K, z0, L, n), ctx.h)
    L, n
end

function resample!(net::StochasticBlockNetworkModel, A::Matrix{Float64}; seed::UInt64=UInt64(0), step::Integer=0, ctx=context())
    K = net.nblocks
    L, n = block_counts(net, A; ctx=ctx)
    check(ccall((:nhp_sbm_draw, libnhp), Int32,
                (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Int64}, Float64, Float64, Float64, UInt64, UInt64, Ptr{Float64}, Ptr{Float64}),
                ctx.h, K, L, n, net.α, net.β, net.γ, seed, UInt64(step), net.ρ, net.π), ctx.h)
    z0 = Int32.(net.z .- 1)
    check(ccall((:nhp_sbm_resample_blocks, libnhp), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, UInt64, UInt64, Int32,
                 Ptr{Float64}, Ptr{Float64}),
                ctx.h, A, net.nnodes, K, z0, net.ρ, net.π, C_NULL, seed, UInt64(step), Int32(1), C_NULL, C_NULL), ctx.h)
    net.z = Int.(z0) .+ 1
    NHP.params(net)
end

function set_sbm!(ctx::Context, m::Ptr{Cvoid}, net::StochasticBlockNetworkModel; labels_every::Integer=1)
    check(ccall((:nhp_cont_model_set_sbm, libnhp), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Float64),
                ctx.h, m, net.nblocks, Int32.(net.z .- 1), net.ρ, net.π, net.α, net.β, net.γ), ctx.h)
    check(ccall((:nhp_cont_model_set_sbm_labels_every, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), ctx.h, m, labels_every), ctx.h)
end

# -> (sums = [Σρ; Σρ²; Σπ; Σπ²], block_counts N x K) over the kept steps; the state itself goes into `net`
function get_sbm!(ctx::Context, m::Ptr{Cvoid}, net::StochasticBlockNetworkModel)
    K, N = net.nblocks, net.nnodes
    z0, sums, bc = Vector{Int32}(undef, N), Vector{Float64}(undef, 2K * K + 2K), Matrix{Int64}(undef, N, K)
    check(ccall((:nhp_cont_model_get_sbm, libnhp), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                ctx.h, m, z0, net.ρ, net.π, sums, bc), ctx.h)
    net.z = Int.(z0) .+ 1
    sums, bc
end

# one network step of mcmc! under the block model (asynchronous): link probabilities, adjacency sweep, resample!(network, A)
sbm_step!(ctx::Context, ds, m::Ptr{Cvoid}; seed::UInt64=UInt64(0), step::Integer=0) =
    check(ccall((:nhp_cont_sbm_step, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, UInt64, UInt64), ctx.h, ds.h, m, seed, UInt64(step)), ctx.h)

# --- LatentDistanceNetworkModel: the other empty stub at the end of src/networks.jl -------------------------------------------
# z_n ~ N(0, σ² I_D), b ~ N(μb, σb²), A[p,c] ~ Bernoulli(1 / (1 + exp(-(b - ‖z_p - z_c‖²)))); z is N x D.  resample!(net, A) runs on
# the GPU through the stand-alone entry (csrc/latent.hip): one elliptical-slice sweep over the positions, then the offset;
# set_latent! / get_latent! / latent_step! keep the state next to a device model `m` (with_model), where nhp_cont_mcmc_run
# takes the latent network step by itself.  Positions are identified only up to rotation, reflection and sign.
mutable struct LatentDistanceNetworkModel
    nnodes::Int; ndims::Int
    z::Matrix{Float64}; b::Float64
    σ::Float64; μb::Float64; σb::Float64
end
LatentDistanceNetworkModel(nnodes, ndims=2; z=zeros(nnodes, ndims), b=0.0, σ=1.0, μb=0.0, σb=1.0) =
    LatentDistanceNetworkModel(nnodes, ndims, z, b, σ, μb, σb)
NHP.params(net::LatentDistanceNetworkModel) = [net.b]
link_probability(net::LatentDistanceNetworkModel) =
    [1 / (1 + exp(sum(abs2, net.z[p, :] .- net.z[c, :]) - net.b)) for p in 1:net.nnodes, c in 1:net.nnodes]

# -> (log p(A | z, b), the N conditional terms L_n the position sweep slices on)
function latent_loglikelihood(net::LatentDistanceNetworkModel, A::Matrix{Float64}; ctx=context())
    out = Vector{Float64}(undef, net.nnodes + 1)
    check(ccall((:nhp_latent_loglik, libnhp), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Float64, Ptr{Float64}),
                ctx.h, A, net.nnodes, net.ndims, net.z, net.b, out), ctx.h)
    out[1], out[2:end]
end

# -> the number of slice steps that used up their 100 attempts and kept their value
function resample!(net::LatentDistanceNetworkModel, A::Matrix{Float64}; seed::UInt64=UInt64(0), step::Integer=0, positions::Bool=true,
                   ctx=context())
    b, exhausted = Ref{Float64}(net.b), Ref{Int64}(0)
    check(ccall((:nhp_latent_resample, libnhp), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ref{Float64}, Float64, Float64, Float64, Ptr{Float64}, UInt64, UInt64,
                 Int32, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ref{Int64}),
                ctx.h, A, net.nnodes, net.ndims, net.z, b, net.σ, net.μb, net.σb, C_NULL, seed, UInt64(step), Int32(positions ? 1 : 0),
                Int32(1), C_NULL, C_NULL, C_NULL, exhausted), ctx.h)
    net.b = b[]
    exhausted[]
end

function set_latent!(ctx::Context, m::Ptr{Cvoid}, net::LatentDistanceNetworkModel; positions_every::Integer=1)
    check(ccall((:nhp_cont_model_set_latent, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Float64, Float64, Float64, Float64),
                ctx.h, m, net.ndims, net.z, net.b, net.σ, net.μb, net.σb), ctx.h)
    check(ccall((:nhp_cont_model_set_latent_positions_every, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), ctx.h, m, positions_every), ctx.h)
end

# -> (sums = [Σb; Σb²], Σ link probability N x N, exhausted slice steps) over the kept steps; the state itself goes into `net`
function get_latent!(ctx::Context, m::Ptr{Cvoid}, net::LatentDistanceNetworkModel)
    N = net.nnodes
    b, sums, ps, exhausted = Ref{Float64}(0.0), Vector{Float64}(undef, 2), Matrix{Float64}(undef, N, N), Ref{Int64}(0)
    check(ccall((:nhp_cont_model_get_latent, libnhp), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ref{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}),
                ctx.h, m, net.z, b, sums, ps, exhausted), ctx.h)
    net.b = b[]
    sums, ps, exhausted[]
end

# one network step of mcmc! under the latent distance model (asynchronous): link probabilities, adjacency sweep, resample!(network, A)
latent_step!(ctx::Context, ds, m::Ptr{Cvoid}; seed::UInt64=UInt64(0), step::Integer=0) =
    check(ccall((:nhp_cont_latent_step, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, UInt64, UInt64), ctx.h, ds.h, m, seed, UInt64(step)), ctx.h)

# BASELINE config 5: after every rank ran its own chain with keep_samples=false, the per-chain posterior sums (still on
# the devices) all-gathered over RCCL: returns (sum, sumsq) as len x world matrices, the sample counts, and ρ's sums.
function gather_moments(ctx::Context, comm::Comm, m::Ptr{Cvoid}, len::Integer)
    s, q = Matrix{Float64}(undef, len, comm.world), Matrix{Float64}(undef, len, comm.world)
    counts, rho = Vector{Int64}(undef, comm.world), Matrix{Float64}(undef, 3, comm.world)
    check(ccall((:nhp_gather_moments, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}),
                ctx.h, comm.h, m, s, q, len, counts, rho), ctx.h)
    s, q, counts, rho
end

# ======================================================================================================================
# Discrete half: src/discrete.jl:86-151,211-296,369-375; src/inference.jl:153-181; src/parents.jl:82-177
# ======================================================================================================================

# convolve(process, data) keeps Ŝ (T x N x B, 3.3 GB at BASELINE config 4) on the device: `Convolved` stands where the
# reference passes the `convolved` array, and `Array(c)` / `convolve(...; fetch=true)` gives the array itself.
mutable struct Convolved
    h::Ptr{Cvoid}; N::Int; T::Int; B::Int
    data::Matrix{Int64}
    host::Union{Nothing,Array{Float64,3}}
end

function basis_matrix(imp::NHP.DiscreteGaussianImpulseResponse)        # basis(impulse): L x B  src/impulses.jl:321-335
    L, B = imp.nlags, size(imp.θ, 3)
    phi = Matrix{Float64}(undef, L, B)
    check(ccall((:nhp_disc_basis, libnhp), Int32, (Int32, Int32, Float64, Ptr{Float64}), L, B, imp.dt, phi))
    phi
end

# --- convolve(process, data)  src/discrete.jl:146-151 ---------------------------------------------------------------
function convolve(p::NHP.DiscreteHawkesProcess, data::Matrix{Int64}; fetch=false, ctx=context())
    N, T = size(data)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:nhp_disc_dataset_create, libnhp), Int32, (Ptr{Cvoid}, Ptr{Int64}, Int32, Int64, Ref{Ptr{Cvoid}}), ctx.h, data, N, T, r), ctx.h)
    phi = basis_matrix(p.impulses)
    L, B = size(phi)
    host = fetch ? Array{Float64,3}(undef, T, N, B) : nothing
    GC.@preserve host check(ccall((:nhp_disc_convolve, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{Float64}),
                ctx.h, r[], phi, L, B, fetch ? pointer(host) : Ptr{Float64}(C_NULL)), ctx.h)
    c = Convolved(r[], N, T, B, data, host)
    finalizer(x -> ccall((:nhp_disc_dataset_destroy, libnhp), Cvoid, (Ptr{Cvoid},), x.h), c)
end

# --- independent trials: N x T_r matrices stacked along time, the convolution stops at every trial's first bin --------------
# stack_trials(trials) -> (counts N x ΣT_r, offsets [R + 1]); convolve(p, trials) -> `Convolved` over the stacked bins.  Every
# call that takes a `Convolved` works on rows of Ŝ and takes it as it is; the library refuses an LGCP baseline and the
# streamed svi window on several trials (NHP_ENOTIMPL).
function stack_trials(trials::AbstractVector{<:AbstractMatrix{<:Integer}})
    isempty(trials) && throw(ArgumentError("trials is empty: at least one N x T count matrix is needed"))
    N = size(trials[1], 1)
    for (r, x) in enumerate(trials)
        size(x, 1) == N || throw(ArgumentError("trial $r has $(size(x, 1)) nodes, trial 1 has $N"))
        size(x, 2) >= 1 || throw(ArgumentError("trial $r holds no bins"))
        any(<(0), x) && throw(DomainError(r, "counts must be non-negative"))
    end
    Matrix{Int64}(reduce(hcat, trials)), Int64[0; cumsum(size.(trials, 2))]
end

function set_trials!(c::Convolved, offsets::Vector{Int64}; ctx=context())
    check(ccall((:nhp_disc_dataset_set_trials, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Int32), ctx.h, c.h, offsets,
                length(offsets) - 1), ctx.h)
    c.B = 0; c.host = nothing                       # Ŝ is dropped: convolve again
    c
end

function trial_offsets(c::Convolved)
    n = Ref{Int32}(0)
    check(ccall((:nhp_disc_dataset_get_trials, libnhp), Int32, (Ptr{Cvoid}, Ref{Int32}, Ptr{Int64}), c.h, n, Ptr{Int64}(C_NULL)))
    off = Vector{Int64}(undef, n[] + 1)
    check(ccall((:nhp_disc_dataset_get_trials, libnhp), Int32, (Ptr{Cvoid}, Ref{Int32}, Ptr{Int64}), c.h, n, off))
    off
end

# Σ_t Ŝ[t, n, b] as the convolution left it on the device -> N x B
function convsum(c::Convolved; ctx=context())
    out = Matrix{Float64}(undef, c.N, c.B)
    check(ccall((:nhp_disc_dataset_get_convsum, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}), ctx.h, c.h, out), ctx.h)
    out
end

function convolve(p::NHP.DiscreteHawkesProcess, trials::AbstractVector{<:AbstractMatrix{<:Integer}}; fetch=false, ctx=context())
    data, offsets = stack_trials(trials)
    N, T = size(data)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:nhp_disc_dataset_create, libnhp), Int32, (Ptr{Cvoid}, Ptr{Int64}, Int32, Int64, Ref{Ptr{Cvoid}}), ctx.h, data, N, T, r), ctx.h)
    c = Convolved(r[], N, T, 0, data, nothing)
    finalizer(x -> ccall((:nhp_disc_dataset_destroy, libnhp), Cvoid, (Ptr{Cvoid},), x.h), c)
    set_trials!(c, offsets; ctx=ctx)
    phi = basis_matrix(p.impulses)
    L, B = size(phi)
    host = fetch ? Array{Float64,3}(undef, T, N, B) : nothing
    GC.@preserve host check(ccall((:nhp_disc_convolve, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{Float64}),
                ctx.h, c.h, phi, L, B, fetch ? pointer(host) : Ptr{Float64}(C_NULL)), ctx.h)
    c.B = B; c.host = host
    c
end

lowered(p::NHP.DiscreteHawkesProcess) = (Vector{Float64}(p.baseline.λ), Matrix{Float64}(p.weights.W), Array{Float64,3}(p.impulses.θ),
    p isa NHP.DiscreteNetworkHawkesProcess ? Matrix{Float64}(p.adjacency_matrix) : nothing)
aptr(A) = A === nothing ? Ptr{Float64}(C_NULL) : pointer(A)

# --- intensity(process, convolved) -> T x N  src/discrete.jl:115-131 --------------------------------------------------
function intensity(p::NHP.DiscreteHawkesProcess, c::Convolved; ctx=context())
    l0, W, θ, A = lowered(p)
    λ = Matrix{Float64}(undef, c.T, c.N)
    GC.@preserve A check(ccall((:nhp_disc_intensity, libnhp), Int32,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}),
        ctx.h, c.h, l0, W, θ, aptr(A), p.dt, λ), ctx.h)
    λ
end

# --- loglikelihood(process, data[, convolved])  src/discrete.jl:86-102 ------------------------------------------------
function loglikelihood(p::NHP.DiscreteHawkesProcess, data::Matrix{Int64}, c::Convolved=convolve(p, data); ctx=context())
    l0, W, θ, A = lowered(p)
    ll = Ref{Float64}(0.0)
    GC.@preserve A check(ccall((:nhp_disc_loglik, libnhp), Int32,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Ref{Float64}),
        ctx.h, c.h, l0, W, θ, aptr(A), p.dt, ll), ctx.h)
    ll[]
end

# --- residuals(process, data[, convolved]): no reference counterpart -------------------------------------------------------
# Goodness of fit of a discrete process on its counts (nhp_disc_residuals): cell (t, c) is Poisson(λ[t,c]) with λ =
# intensity(p, c); pit (T x N, with pit=true) is the randomized probability integral transform F(s-1) + v·p(s) of every cell,
# uniform on [0, 1) under the model; pearson = (s-λ)/√λ; cumulative = cumsum(λ, dims=1); per node expected = Σλ, observed = Σs,
# chi2 = Σ(s-λ)²/λ, deviance, and histogram (nbins x N) of the pit values; impossible = the cells with λ = 0 and s > 0.
# Homogeneous baselines (the LGCP baseline goes through the dataset, as for the other discrete calls of the Python binding).
function residuals(p::NHP.DiscreteHawkesProcess, data::Matrix{Int64}, c::Convolved=convolve(p, data); seed::Integer=0, nbins::Integer=20,
                   pit::Bool=true, pearson::Bool=false, cumulative::Bool=false, ctx=context())
    1 <= nbins <= 4096 || throw(ArgumentError("nbins = $nbins outside [1, 4096]"))
    l0, W, θ, A = lowered(p)
    plane(on) = on ? Matrix{Float64}(undef, c.T, c.N) : nothing
    u, r, cum = plane(pit), plane(pearson), plane(cumulative)
    expected, chi2, deviance = Vector{Float64}(undef, c.N), Vector{Float64}(undef, c.N), Vector{Float64}(undef, c.N)
    observed, histogram, impossible = Vector{Int64}(undef, c.N), Matrix{Int64}(undef, nbins, c.N), Ref{Int64}(0)
    GC.@preserve A u r cum check(ccall((:nhp_disc_residuals, libnhp), Int32,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, UInt64, Int32, Int32, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ref{Int64}, Ptr{Float64}),
        ctx.h, c.h, l0, W, θ, aptr(A), p.dt, seed % UInt64, Int32(nbins), Int32(0), aptr(u), aptr(r), aptr(cum), expected, observed,
        chi2, deviance, histogram, impossible, Ptr{Float64}(C_NULL)), ctx.h)
    (pit=u, pearson=r, cumulative=cum, expected=expected, observed=observed, chi2=chi2, deviance=deviance, histogram=histogram,
     impossible=impossible[])
end

# --- update!(process, data, convolved): one mean-field step  src/discrete.jl:369-375 ----------------------------------
# (src/parents.jl:136-177 + src/baselines.jl:444-452, src/weights.jl:70-91, src/impulses.jl:355-371, fused: the
# T x N x (1+NB) responsibilities are never formed).  Overwrites the variational parameters of the components in place
# and returns variational_params(process) like the reference.  n_steps > 1 keeps them on the device in between.
function update!(p::NHP.DiscreteStandardHawkesProcess, data, c::Convolved; n_steps::Integer=1, ctx=context())
    b, w, imp = p.baseline, p.weights, p.impulses
    αv, βv = Vector{Float64}(b.αv), Vector{Float64}(b.βv)
    κv, νv, γv = Matrix{Float64}(w.κv), Matrix{Float64}(w.νv), Array{Float64,3}(imp.γv)
    check(ccall((:nhp_disc_vb_run, libnhp), Int32,
        (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Float64, Float64, Float64, Int32,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        ctx.h, c.h, p.dt, b.α0, b.β0, w.κ, w.ν, imp.γ, n_steps, αv, βv, κv, νv, γv), ctx.h)
    b.αv, b.βv, w.κv, w.νv, imp.γv = αv, βv, κv, νv, γv
    NHP.variational_params(p)
end

# --- vb!(process, data; max_steps=1_000, Δx_thresh=1e-6, Δq_thresh=1e-2, verbose=false) -> VariationalInference
#     src/inference.jl:153-181 (its convergence test is commented out in the reference: max_steps updates always run)
function vb!(p::NHP.DiscreteStandardHawkesProcess, data::Matrix{Int64}; max_steps::Int64=1_000, Δx_thresh=1e-6, Δq_thresh=1e-2,
             verbose=false, ctx=context())
    convolved = convolve(p, data; ctx=ctx)
    res = NHP.VariationalInference(p)
    start_time = time()
    while res.step < max_steps
        push!(res.trace, update!(p, data, convolved; ctx=ctx))
        res.step += 1
    end
    res.elapsed = time() - start_time
    println(" ** maximum steps reached **")
    return res
end

# --- svi!(process, data; nsteps=1_000, batch_bins=4096, delay=1.0, forgetting=0.6, seed=0, blocks=nothing, streamed=false,
#          trace_every=0, step0=0) -> VariationalInference       a stub in the reference (src/inference.jl:190)
# Stochastic variational inference (nhp_disc_svi_run; the contract is in include/nhp.h): the T bins are cut into
# nb = cld(T, batch_bins) consecutive blocks, step i = step0 + k takes one block -- blocks[k] (0-based, as the library counts
# them), or a draw that depends on (seed, i) alone -- and blends the block's update!, scaled by nb, into the variational
# parameters with weight (i + delay)^(-forgetting).  streamed=true convolves each block on the fly and never holds the
# T x N x B convolution.  trace_every = k appends variational_params(process) every k steps; 0 keeps the final ones.
function svi!(p::NHP.DiscreteStandardHawkesProcess, data::Matrix{Int64}; nsteps::Integer=1_000, batch_bins::Integer=4096, delay=1.0,
              forgetting=0.6, seed::Integer=0, blocks=nothing, streamed::Bool=false, trace_every::Integer=0, step0::Integer=0,
              ctx=context())
    p.weights isa NHP.DenseWeightModel || error("svi! exists only for DenseWeightModel")
    p.baseline isa NHP.DiscreteHomogeneousProcess || error("svi! is defined for DiscreteHomogeneousProcess baselines only")
    N, T = size(data)
    (batch_bins >= T || (batch_bins >= 16 && batch_bins % 16 == 0)) || throw(ArgumentError("batch_bins must be a multiple of 16, or >= the number of bins"))
    delay >= 0 || throw(ArgumentError("delay must be >= 0"))
    0.5 < forgetting <= 1 || throw(ArgumentError("forgetting must lie in (0.5, 1]"))
    nb = cld(T, min(batch_bins, T))
    blk = blocks === nothing ? nothing : Vector{Int32}(blocks)
    blk === nothing || (length(blk) >= nsteps && all(0 .<= blk .< nb)) || throw(ArgumentError("blocks: nsteps indices in [0, $nb) are required"))
    phi = basis_matrix(p.impulses)
    L, B = size(phi)
    if streamed
        r = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:nhp_disc_dataset_create, libnhp), Int32, (Ptr{Cvoid}, Ptr{Int64}, Int32, Int64, Ref{Ptr{Cvoid}}), ctx.h, data, N, T, r), ctx.h)
        c = Convolved(r[], N, T, 0, data, nothing)
        finalizer(x -> ccall((:nhp_disc_dataset_destroy, libnhp), Cvoid, (Ptr{Cvoid},), x.h), c)
    else
        c = convolve(p, data; ctx=ctx)
    end
    b, w, imp = p.baseline, p.weights, p.impulses
    αv, βv = Vector{Float64}(b.αv), Vector{Float64}(b.βv)
    κv, νv, γv = Matrix{Float64}(w.κv), Matrix{Float64}(w.νv), Array{Float64,3}(imp.γv)
    res = NHP.VariationalInference(p)
    res.step = step0
    start_time = time()
    done = 0
    while done < nsteps
        n = trace_every > 0 ? min(trace_every, nsteps - done) : nsteps
        bp = blk === nothing ? Ptr{Int32}(C_NULL) : pointer(blk, done + 1)
        GC.@preserve blk phi c check(ccall((:nhp_disc_svi_run, libnhp), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Float64, Float64, Float64, Int64, Float64, Float64, UInt64, Int64, Int32,
             Ptr{Int32}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
            ctx.h, c.h, p.dt, b.α0, b.β0, w.κ, w.ν, imp.γ, batch_bins, delay, forgetting, seed % UInt64, step0 + done, n,
            bp, streamed ? pointer(phi) : Ptr{Float64}(C_NULL), L, B, αv, βv, κv, νv, γv), ctx.h)
        done += n
        res.step = step0 + done
        b.αv, b.βv, w.κv, w.νv, imp.γv = copy(αv), copy(βv), copy(κv), copy(νv), copy(γv)
        trace_every > 0 && push!(res.trace, NHP.variational_params(p))
    end
    trace_every > 0 || push!(res.trace, NHP.variational_params(p))
    res.elapsed = time() - start_time
    return res
end

# --- update! / vb! / svi! for DiscreteNetworkHawkesProcess + SparseWeightModel (nhp_disc_netvb_run, nhp_disc_netsvi_run) ---
# The reference's methods throw on their wiring (src/discrete.jl:494-501, src/weights.jl:141-173); the formulas are its own
# (include/nhp.h).  Its SparseWeightModel has no field for q(A = 1), so ρv travels as an N x N matrix the caller keeps: it
# is updated in place, `nothing` starts from link_probability(network).  DenseNetworkModel gives ρv ≡ 1; the Bernoulli
# network's αv, βv are updated in place; other networks and baselines are refused by the library.
net_kind(n::NHP.DenseNetworkModel) = Int32(0)
net_kind(n::NHP.BernoulliNetworkModel) = Int32(1)
net_kind(n) = error("network VB is built for DenseNetworkModel and BernoulliNetworkModel")
net_prior(n::NHP.BernoulliNetworkModel) = (Float64(n.α), Float64(n.β), Ref(Float64(n.αv)), Ref(Float64(n.βv)))
net_prior(n) = (1.0, 1.0, Ref(1.0), Ref(1.0))
function net_store!(p::NHP.DiscreteNetworkHawkesProcess, αv, βv, κ0, ν0, κ1, ν1, γv, na, nb)
    b, w, imp = p.baseline, p.weights, p.impulses
    b.αv, b.βv, w.κv0, w.νv0, w.κv1, w.νv1, imp.γv = copy(αv), copy(βv), copy(κ0), copy(ν0), copy(κ1), copy(ν1), copy(γv)
    p.network isa NHP.BernoulliNetworkModel && ((p.network.αv, p.network.βv) = (na[], nb[]))
end
net_params(p, ρv, na, nb) = p.network isa NHP.BernoulliNetworkModel ?
    [NHP.variational_params(p.baseline); NHP.variational_params(p.weights); NHP.variational_params(p.impulses); vec(ρv); na[]; nb[]] :
    [NHP.variational_params(p.baseline); NHP.variational_params(p.weights); NHP.variational_params(p.impulses); vec(ρv)]

function update!(p::NHP.DiscreteNetworkHawkesProcess, data, c::Convolved; ρv::Union{Nothing,Matrix{Float64}}=nothing,
                 n_steps::Integer=1, ctx=context())
    p.weights isa NHP.SparseWeightModel || error("network update! needs a SparseWeightModel")
    b, w, imp = p.baseline, p.weights, p.impulses
    ρ = ρv === nothing ? Matrix{Float64}(NHP.link_probability(p.network)) : ρv
    αv, βv, γv = Vector{Float64}(b.αv), Vector{Float64}(b.βv), Array{Float64,3}(imp.γv)
    κ0, ν0, κ1, ν1 = Matrix{Float64}(w.κv0), Matrix{Float64}(w.νv0), Matrix{Float64}(w.κv1), Matrix{Float64}(w.νv1)
    α, β, na, nb = net_prior(p.network)
    check(ccall((:nhp_disc_netvb_run, libnhp), Int32,
        (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Float64, Float64, Float64, Float64, Float64, Int32, Float64, Float64, Int32,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ref{Float64}, Ref{Float64}),
        ctx.h, c.h, p.dt, b.α0, b.β0, w.κ0, w.ν0, w.κ1, w.ν1, imp.γ, net_kind(p.network), α, β, n_steps,
        αv, βv, κ0, ν0, κ1, ν1, γv, ρ, na, nb), ctx.h)
    net_store!(p, αv, βv, κ0, ν0, κ1, ν1, γv, na, nb)
    (net_params(p, ρ, na, nb), ρ)
end

function vb!(p::NHP.DiscreteNetworkHawkesProcess, data::Matrix{Int64}; max_steps::Int64=1_000, Δx_thresh=1e-6, Δq_thresh=1e-2,
             verbose=false, ρv::Union{Nothing,Matrix{Float64}}=nothing, ctx=context())
    convolved = convolve(p, data; ctx=ctx)
    res = NHP.VariationalInference(p)
    ρ = ρv === nothing ? Matrix{Float64}(NHP.link_probability(p.network)) : ρv
    start_time = time()
    while res.step < max_steps
        push!(res.trace, update!(p, data, convolved; ρv=ρ, ctx=ctx)[1])
        res.step += 1
    end
    res.elapsed = time() - start_time
    return res, ρ
end

# resident mode; the keywords are svi!'s for the standard process
function svi!(p::NHP.DiscreteNetworkHawkesProcess, data::Matrix{Int64}; nsteps::Integer=1_000, batch_bins::Integer=4096, delay=1.0,
              forgetting=0.6, seed::Integer=0, blocks=nothing, step0::Integer=0, ρv::Union{Nothing,Matrix{Float64}}=nothing,
              ctx=context())
    p.weights isa NHP.SparseWeightModel || error("network svi! needs a SparseWeightModel")
    N, T = size(data)
    nb_ = cld(T, min(batch_bins, T))
    blk = blocks === nothing ? nothing : Vector{Int32}(blocks)
    blk === nothing || (length(blk) >= nsteps && all(0 .<= blk .< nb_)) || throw(ArgumentError("blocks: nsteps indices in [0, $nb_) are required"))
    c = convolve(p, data; ctx=ctx)
    b, w, imp = p.baseline, p.weights, p.impulses
    ρ = ρv === nothing ? Matrix{Float64}(NHP.link_probability(p.network)) : ρv
    αv, βv, γv = Vector{Float64}(b.αv), Vector{Float64}(b.βv), Array{Float64,3}(imp.γv)
    κ0, ν0, κ1, ν1 = Matrix{Float64}(w.κv0), Matrix{Float64}(w.νv0), Matrix{Float64}(w.κv1), Matrix{Float64}(w.νv1)
    α, β, na, nb = net_prior(p.network)
    res = NHP.VariationalInference(p)
    bp = blk === nothing ? Ptr{Int32}(C_NULL) : pointer(blk)
    start_time = time()
    GC.@preserve blk c check(ccall((:nhp_disc_netsvi_run, libnhp), Int32,
        (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Float64, Float64, Float64, Float64, Float64, Int32, Float64, Float64,
         Int64, Float64, Float64, UInt64, Int64, Int32, Ptr{Int32}, Ptr{Float64}, Int32, Int32,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ref{Float64}, Ref{Float64}),
        ctx.h, c.h, p.dt, b.α0, b.β0, w.κ0, w.ν0, w.κ1, w.ν1, imp.γ, net_kind(p.network), α, β,
        batch_bins, delay, forgetting, seed % UInt64, step0, nsteps, bp, Ptr{Float64}(C_NULL), 0, 0,
        αv, βv, κ0, ν0, κ1, ν1, γv, ρ, na, nb), ctx.h)
    net_store!(p, αv, βv, κ0, ν0, κ1, ν1, γv, na, nb)
    res.step = step0 + nsteps
    push!(res.trace, net_params(p, ρ, na, nb))
    res.elapsed = time() - start_time
    return res, ρ
end

# --- update! / svi! with a StochasticBlockNetworkModel (nhp_disc_sbmvb_run, nhp_disc_sbmsvi_run; DESIGN §3.21) ---
# q(z_n) = Categorical(m[n,:]), q(ρ[k,l]) = Beta(αv[k,l], βv[k,l]), q(π) = Dirichlet(γv) around the network step above.  The
# block model here is this module's own struct, so it travels next to the process (whose `network` field is not read), and
# its variational state is a BlockVariational the caller keeps, updated in place like ρv.  Mean-field over labels has the
# uniform state as a fixed point: variational_init refuses sharpness = 0, and nothing creates the state implicitly.
mutable struct BlockVariational
    m::Matrix{Float64}; αv::Matrix{Float64}; βv::Matrix{Float64}; γv::Vector{Float64}
    labels_every::Int
    step::Int          # VB steps taken so far: the sweep runs at the global steps that are multiples of labels_every
end
function variational_init(net::StochasticBlockNetworkModel; sharpness=0.5, labels_every::Integer=1)
    0 < sharpness <= 1 || throw(ArgumentError("sharpness must lie in (0, 1]; 0 is the symmetric fixed point of the label update"))
    labels_every >= 1 || throw(ArgumentError("labels_every must be positive"))
    N, K = net.nnodes, net.nblocks
    m = fill((1 - sharpness) / K, N, K)
    for n in 1:N
        m[n, net.z[n]] += sharpness
    end
    BlockVariational(m ./ sum(m, dims=2), fill(net.α, K, K), fill(net.β, K, K), fill(net.γ, K), labels_every, 0)
end
block_params(p, ρv, q::BlockVariational) =
    [NHP.variational_params(p.baseline); NHP.variational_params(p.weights); NHP.variational_params(p.impulses); vec(ρv);
     vec(q.αv); vec(q.βv); q.γv; vec(q.m)]

function sbm_update!(p::NHP.DiscreteNetworkHawkesProcess, data, c::Convolved, net::StochasticBlockNetworkModel, q::BlockVariational;
                     ρv::Union{Nothing,Matrix{Float64}}=nothing, n_steps::Integer=1, ctx=context())
    p.weights isa NHP.SparseWeightModel || error("network update! needs a SparseWeightModel")
    b, w, imp = p.baseline, p.weights, p.impulses
    ρ = ρv === nothing ? Matrix{Float64}(link_probability(net)) : ρv
    αv, βv, γv = Vector{Float64}(b.αv), Vector{Float64}(b.βv), Array{Float64,3}(imp.γv)
    κ0, ν0, κ1, ν1 = Matrix{Float64}(w.κv0), Matrix{Float64}(w.νv0), Matrix{Float64}(w.κv1), Matrix{Float64}(w.νv1)
    check(ccall((:nhp_disc_sbmvb_run, libnhp), Int32,
        (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Float64, Float64, Float64, Float64, Float64, Int32, Float64, Float64, Float64,
         Int32, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        ctx.h, c.h, p.dt, b.α0, b.β0, w.κ0, w.ν0, w.κ1, w.ν1, imp.γ, net.nblocks, net.α, net.β, net.γ, q.labels_every, q.step, n_steps,
        αv, βv, κ0, ν0, κ1, ν1, γv, ρ, q.m, q.αv, q.βv, q.γv), ctx.h)
    q.step += n_steps
    b.αv, b.βv, w.κv0, w.νv0, w.κv1, w.νv1, imp.γv = αv, βv, κ0, ν0, κ1, ν1, γv
    (block_params(p, ρ, q), ρ)
end

# resident mode; the keywords are svi!'s for the standard process
function sbm_svi!(p::NHP.DiscreteNetworkHawkesProcess, data::Matrix{Int64}, net::StochasticBlockNetworkModel, q::BlockVariational;
                  nsteps::Integer=1_000, batch_bins::Integer=4096, delay=1.0, forgetting=0.6, seed::Integer=0, blocks=nothing,
                  step0::Integer=0, ρv::Union{Nothing,Matrix{Float64}}=nothing, ctx=context())
    p.weights isa NHP.SparseWeightModel || error("network svi! needs a SparseWeightModel")
    N, T = size(data)
    nb_ = cld(T, min(batch_bins, T))
    blk = blocks === nothing ? nothing : Vector{Int32}(blocks)
    blk === nothing || (length(blk) >= nsteps && all(0 .<= blk .< nb_)) || throw(ArgumentError("blocks: nsteps indices in [0, $nb_) are required"))
    c = convolve(p, data; ctx=ctx)
    b, w, imp = p.baseline, p.weights, p.impulses
    ρ = ρv === nothing ? Matrix{Float64}(link_probability(net)) : ρv
    αv, βv, γv = Vector{Float64}(b.αv), Vector{Float64}(b.βv), Array{Float64,3}(imp.γv)
    κ0, ν0, κ1, ν1 = Matrix{Float64}(w.κv0), Matrix{Float64}(w.νv0), Matrix{Float64}(w.κv1), Matrix{Float64}(w.νv1)
    res = NHP.VariationalInference(p)
    bp = blk === nothing ? Ptr{Int32}(C_NULL) : pointer(blk)
    start_time = time()
    GC.@preserve blk c check(ccall((:nhp_disc_sbmsvi_run, libnhp), Int32,
        (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Float64, Float64, Float64, Float64, Float64, Int32, Float64, Float64, Float64,
         Int32, Int64, Float64, Float64, UInt64, Int64, Int32, Ptr{Int32}, Ptr{Float64}, Int32, Int32,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        ctx.h, c.h, p.dt, b.α0, b.β0, w.κ0, w.ν0, w.κ1, w.ν1, imp.γ, net.nblocks, net.α, net.β, net.γ, q.labels_every,
        batch_bins, delay, forgetting, seed % UInt64, step0, nsteps, bp, Ptr{Float64}(C_NULL), 0, 0,
        αv, βv, κ0, ν0, κ1, ν1, γv, ρ, q.m, q.αv, q.βv, q.γv), ctx.h)
    b.αv, b.βv, w.κv0, w.νv0, w.κv1, w.νv1, imp.γv = αv, βv, κ0, ν0, κ1, ν1, γv
    res.step = step0 + nsteps
    push!(res.trace, block_params(p, ρ, q))
    res.elapsed = time() - start_time
    return res, ρ
end

# the fit as a block model: ρ = αv/(αv + βv), π = γv/Σγv, z = argmax_k m (1-based)
function variational_mean!(net::StochasticBlockNetworkModel, q::BlockVariational)
    net.ρ = q.αv ./ (q.αv .+ q.βv)
    net.π = q.γv ./ sum(q.γv)
    net.z = [argmax(q.m[n, :]) for n in 1:net.nnodes]
    net
end

# --- mle!(process::DiscreteStandardHawkesProcess, data; optimizer=BFGS, verbose=false, f_abstol=1e-6, regularize=false,
#          guess=nothing, max_increase_steps=3) -> MaximumLikelihood   src/discrete.jl:211-296 ---------------------------
# Parameter vector [λ0; vec(W .* θ)] (params / params!, src/discrete.jl:174-201).  regularize=true calls the reference's
# logprior(process), which reads fields the process does not have (SURVEY D5): it throws here as it does there.
function mle!(p::NHP.DiscreteStandardHawkesProcess, data::Matrix{Int64}; optimizer=Optim.BFGS, verbose=false, f_abstol=1e-6,
              regularize=false, guess=nothing, max_increase_steps=3, max_steps=1000, ctx=context())
    convolved = convolve(p, data; ctx=ctx)
    guess = guess === nothing ? NHP._rand_init_(p) : guess
    P = length(guess)
    if optimizer === :device
        # the whole iteration inside the library (nhp_disc_mle_run): x = params(process) stays on the device, params!'s split
        # into W and θ is redone there per evaluation; homogeneous baseline
        regularize && error("optimizer=:device minimises -loglikelihood only")
        x = clamp.(Vector{Float64}(guess), 1e-6, 1e1)
        loss, steps, conv, evals = Ref{Float64}(0.0), Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0)
        t0 = time()
        check(ccall((:nhp_disc_mle_run, libnhp), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Float64, Int32, Ptr{Float64}, Int64, Ref{Float64}, Ref{Int32}, Ref{Int32}, Ref{Int32}),
            ctx.h, convolved.h, p.dt, 1e-6, 1e1, f_abstol, Int32(max_steps), x, P, loss, steps, conv, evals), ctx.h)
        verbose && println(" > steps: $(steps[]), objective evaluations: $(evals[]), loss: $(loss[])")
        NHP.params!(p, x)
        return NHP.MaximumLikelihood(x, -loss[], Int(steps[]), time() - t0, conv[] == 1 ? "success" : "failure")
    end
    ll, g = Ref{Float64}(0.0), Vector{Float64}(undef, P)
    function fg!(G, x)
        NHP.params!(p, x)
        l0, W, θ, _ = lowered(p)
        check(ccall((:nhp_disc_loglik_grad, libnhp), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Ref{Float64}, Ptr{Float64}, Int64),
            ctx.h, convolved.h, l0, W, θ, p.dt, ll, g, P), ctx.h)
        f = -ll[]
        regularize && (f -= NHP.logprior(p))
        G === nothing || (G .= .-g)
        f
    end
    run_mle(fg!, guess; optimizer=optimizer, verbose=verbose, f_abstol=f_abstol, max_increase_steps=max_increase_steps)
end

# --- observed_information(process, data) and hessian_vector_product(process, data, v) for the discrete process: no reference
# counterpart.  In mle!'s parameters [λ0; vec(W .* θ)] the intensity is linear, so the information is block diagonal by child
# node: blocks[:, :, k] is the D x D block, D = 1 + N·B, of column columns[k] (1-based here) over [λ0[c]; η[:,c,:]], row 1 the
# baseline, row 1 + (b-1)·N + p the entry η[p,c,b] (nhp_disc_information; homogeneous baseline).  kind = :observed is minus the
# Hessian, :fisher its expectation.  hessian_vector_product returns J·v, the INFORMATION times v (positive semi-definite sign).
function observed_information(p::NHP.DiscreteStandardHawkesProcess, data::Matrix{Int64}; columns=nothing, kind=:observed,
                              tile_rows=0, slab_bins=0, ctx=context(), convolved=convolve(p, data; ctx=ctx))
    N = NHP.ndims(p)
    D = 1 + N * size(p.impulses.θ, 3)
    cols = columns === nothing ? collect(1:N) : collect(Int, columns)
    c0 = Vector{Int32}(cols .- 1)
    l0, W, θ, _ = lowered(p)
    ll, blocks = Ref{Float64}(0.0), Array{Float64}(undef, D, D, length(cols))
    check(ccall((:nhp_disc_information, libnhp), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Int32, Ptr{Int32}, Int32, Int32, Int32,
                 Ref{Float64}, Ptr{Float64}),
                ctx.h, convolved.h, l0, W, θ, p.dt, Int32(kind === :fisher ? 1 : 0), c0, Int32(length(c0)), Int32(tile_rows),
                Int32(slab_bins), ll, blocks), ctx.h)
    (ll=ll[], columns=cols, blocks=blocks, kind=kind)
end

function hessian_vector_product(p::NHP.DiscreteStandardHawkesProcess, data::Matrix{Int64}, v::AbstractVector; kind=:observed,
                                ctx=context(), convolved=convolve(p, data; ctx=ctx))
    x = Vector{Float64}(v)
    length(x) == length(NHP.params(p)) || error("Parameter vector length does not match model parameter length.")
    out = similar(x)
    l0, W, θ, _ = lowered(p)
    check(ccall((:nhp_disc_hessian_vec, libnhp), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Int32, Ptr{Float64}, Ptr{Float64}),
                ctx.h, convolved.h, l0, W, θ, p.dt, Int32(kind === :fisher ? 1 : 0), x, out), ctx.h)
    out
end

# --- resample!(process, data, convolved): one discrete Gibbs sweep  src/discrete.jl:362-368,416-422 -------------------
# Parent counts (src/parents.jl:82-134, reduced straight to counts[N, 1+NB]) and the conjugate draws on the device; the
# network process then sweeps its adjacency matrix (src/discrete.jl:424-480) and redraws ρ (src/networks.jl:70-78).
function resample!(p::NHP.DiscreteHawkesProcess, data, c::Convolved; seed::UInt64=UInt64(0), step::UInt64=UInt64(0), ctx=context())
    b, w, imp = p.baseline, p.weights, p.impulses
    l0, W, θ, A = lowered(p)
    GC.@preserve A check(ccall((:nhp_disc_gibbs_step, libnhp), Int32,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Float64, Float64, Float64, Float64, UInt64, UInt64),
        ctx.h, c.h, l0, W, θ, aptr(A), p.dt, b.α0, b.β0, w.κ, w.ν, imp.γ, seed, step), ctx.h)
    b.λ, w.W, imp.θ = l0, W, θ
    if p isa NHP.DiscreteNetworkHawkesProcess
        links = Ref{Float64}(0.0)
        ρ = p.network isa NHP.BernoulliNetworkModel ? Float64(p.network.ρ) : 1.0
        check(ccall((:nhp_disc_resample_adjacency, libnhp), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Float64, Ptr{Float64}, UInt64, UInt64, Ref{Float64}),
            ctx.h, c.h, l0, W, θ, A, p.dt, C_NULL, ρ, C_NULL, seed, step, links), ctx.h)
        p.adjacency_matrix = A
        NHP.resample!(p.network, A)                                # ρ ~ Beta(α + ΣA, β + N² - ΣA): host, O(1)
    end
    NHP.params(p)
end

# --- the discrete chain on the device (nhp_disc_model, csrc/disc_chain.hip) ---------------------------------------------
# λ0 | W | θ | A in one device block, the Gibbs step and the adjacency sweep in place (the bits of resample! above), ρ drawn
# on the device; running sums and convergence diagnostics as for the continuous chain.  Returns res, or (res, (sum, sumsq,
# count, rho)) with moments, or (res, mom, (summary, batch_len)) with diagnostics: sums in params(p) order without ρ
# ([λ0; vec(W); vec(θ); vec(A)], or [λ0; vec(W .* θ)] for a standard process), summary the 9 x 6 matrix of
# nhp_disc_model_diagnostics_fetch -- fields x groups (λ0, θ | W∘θ, -, W, vec(A), ρ), include/nhp.h.
function resident_mcmc!(p::NHP.DiscreteHawkesProcess, convolved::Convolved, ctx; nsteps, log_freq, verbose, seed, keep_samples, moments,
                        burn, diagnostics, batch_len, ess_below, rhat_above)
    p.baseline isa NHP.DiscreteHomogeneousProcess || error("the device-resident discrete chain draws a homogeneous baseline; the default route (keep_samples=true, moments=false) takes an LGCP baseline")
    p.weights isa NHP.SparseWeightModel && error("the device-resident discrete chain is built for DenseWeightModel; the default route takes a SparseWeightModel")
    network = p isa NHP.DiscreteNetworkHawkesProcess
    bern = network && p.network isa NHP.BernoulliNetworkModel
    network && !bern && !(p.network isa NHP.DenseNetworkModel) &&
        error("the device-resident discrete chain holds a DenseNetworkModel or a BernoulliNetworkModel; the default route takes $(typeof(p.network))")
    N, B = NHP.ndims(p), size(p.impulses.θ, 3)
    b, w, imp = p.baseline, p.weights, p.impulses
    na, nb = bern ? (Float64(p.network.α), Float64(p.network.β)) : (0.0, 0.0)      # 0, 0: ρ held at 1 (DenseNetworkModel)
    res = NHP.MarkovChainMonteCarlo(p)
    mom = nothing
    diag = nothing
    start_time = time()
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:nhp_disc_model_create, libnhp), Int32, (Ptr{Cvoid}, Int32, Int32, Int32, Float64, Ref{Ptr{Cvoid}}),
                ctx.h, Int32(N), Int32(B), Int32(network), Float64(p.dt), h), ctx.h)
    m = h[]
    pull = function ()
        l0, W, θ, A = lowered(p)
        GC.@preserve A check(ccall((:nhp_disc_model_get, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                   ctx.h, m, l0, W, θ, aptr(A)), ctx.h)
        b.λ, w.W, imp.θ = l0, W, θ
        rho = zeros(3)
        if network
            p.adjacency_matrix = A
            if bern
                check(ccall((:nhp_disc_model_get_rho, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}), ctx.h, m, rho), ctx.h)
                p.network.ρ = rho[1]
            end
        end
        rho
    end
    try
        l0, W, θ, A = lowered(p)
        GC.@preserve A check(ccall((:nhp_disc_model_set, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                   ctx.h, m, l0, W, θ, aptr(A)), ctx.h)
        network && check(ccall((:nhp_disc_model_set_rho, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Float64), ctx.h, m, bern ? Float64(p.network.ρ) : 1.0), ctx.h)
        diagnostics && check(ccall((:nhp_disc_model_diagnostics_configure, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64), ctx.h, m,
                                   Int64(batch_len), Int64(max(0, nsteps - burn))), ctx.h)
        moments && check(ccall((:nhp_disc_model_moments_reset, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.h, m), ctx.h)
        while res.steps < nsteps
            n = keep_samples ? 1 : min(nsteps - res.steps, verbose ? log_freq : nsteps)
            check(ccall((:nhp_disc_mcmc_run, libnhp), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Float64, Float64, Float64, Float64, UInt64, UInt64, Int64, Int64),
                        ctx.h, convolved.h, m, b.α0, b.β0, w.κ, w.ν, imp.γ, na, nb, seed, UInt64(res.steps), n, moments ? Int64(burn) : Int64(-1)), ctx.h)
            res.steps += n
            if keep_samples
                pull()
                push!(res.samples, NHP.params(p))
            end
            if res.steps % log_freq == 0 && verbose
                res.elapsed = time() - start_time
                println(" > step: $(res.steps), elapsed: $(res.elapsed)")
            end
        end
        rho = pull()
        keep_samples || push!(res.samples, NHP.params(p))
        if moments
            len = N + N * N * B + (network ? 2 * N * N : 0)
            s, q, cnt = Vector{Float64}(undef, len), Vector{Float64}(undef, len), Ref{Int64}(0)
            check(ccall((:nhp_disc_model_moments_fetch, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ref{Int64}),
                        ctx.h, m, s, q, len, cnt), ctx.h)
            mom = (s, q, cnt[], rho)
            if diagnostics && cnt[] >= 1
                summary = Matrix{Float64}(undef, 9, 6)
                check(ccall((:nhp_disc_model_diagnostics_fetch, libnhp), Int32,
                            (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64),
                            ctx.h, m, Float64(ess_below), Float64(rhat_above), summary, C_NULL, C_NULL, C_NULL, len), ctx.h)
                diag = (summary, Int(batch_len))
            end
        end
    finally
        ccall((:nhp_disc_model_destroy, libnhp), Cvoid, (Ptr{Cvoid},), m)
    end
    res.elapsed = time() - start_time
    return diagnostics ? (res, mom, diag) : moments ? (res, mom) : res
end

# --- mcmc!(process::DiscreteHawkesProcess, data; nsteps=1000, log_freq=100, verbose=false)  src/inference.jl:49-70 ----
# keep_samples=false or moments=true: the chain's state stays on the device (resident_mcmc! above); otherwise every step goes
# through the host arrays, as before.
function mcmc!(p::NHP.DiscreteHawkesProcess, data::Matrix{Int64}; nsteps=1000, log_freq=100, verbose=false, seed::UInt64=UInt64(0),
               ctx=context(), keep_samples=true, moments=false, burn::Integer=0, diagnostics=false,
               batch_len::Integer=max(1, isqrt(max(0, nsteps - burn))), ess_below=100.0, rhat_above=1.01)
    diagnostics && !moments && throw(ArgumentError("diagnostics need the device-side running sums (moments=true)"))
    batch_len >= 1 || throw(ArgumentError("batch_len must be a positive integer"))
    if moments || !keep_samples
        return resident_mcmc!(p, convolve(p, data; ctx=ctx), ctx; nsteps=nsteps, log_freq=log_freq, verbose=verbose, seed=seed,
                              keep_samples=keep_samples, moments=moments, burn=burn, diagnostics=diagnostics, batch_len=batch_len,
                              ess_below=ess_below, rhat_above=rhat_above)
    end
    res = NHP.MarkovChainMonteCarlo(p)
    start_time = time()
    convolved = convolve(p, data; ctx=ctx)
    while res.steps < nsteps
        push!(res.samples, resample!(p, data, convolved; seed=seed, step=UInt64(res.steps), ctx=ctx))
        res.steps += 1
        if res.steps % log_freq == 0 && verbose
            res.elapsed = time() - start_time
            println(" > step: $(res.steps), elapsed: $(res.elapsed)")
        end
    end
    res.elapsed = time() - start_time
    return res
end

# --- scoring a discrete chain: held-out predictive log-likelihood and WAIC (include/nhp.h: nhp_disc_score_*) ---------------
# Thin wrappers: a scorer on bins [t0, t1) (0-based, half-open) of a convolved dataset, fed the state of an nhp_disc_model
# handle `m` draw by draw (score_accumulate!) or attached to it so that nhp_disc_mcmc_run scores the kept steps itself.
const SCORE_FIELDS = (:n, :cells, :lppd, :p_waic, :elpd_waic, :waic, :se_elpd, :joint_lpd, :joint_mean, :joint_sd)

function score_create(convolved, t0::Integer, t1::Integer; ctx=context())
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:nhp_disc_score_create, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ref{Ptr{Cvoid}}),
                ctx.h, convolved.h, Int64(t0), Int64(t1), h), ctx.h)
    return h[]
end
score_destroy(score::Ptr{Cvoid}) = ccall((:nhp_disc_score_destroy, libnhp), Cvoid, (Ptr{Cvoid},), score)
score_reset!(score::Ptr{Cvoid}; ctx=context()) =
    check(ccall((:nhp_disc_score_reset, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.h, score), ctx.h)
score_accumulate!(score::Ptr{Cvoid}, m::Ptr{Cvoid}; ctx=context()) =
    check(ccall((:nhp_disc_score_accumulate, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), ctx.h, score, m), ctx.h)
# every >= 1; score = C_NULL detaches every scorer of the model
score_attach!(m::Ptr{Cvoid}, score::Ptr{Cvoid}, every::Integer=1; ctx=context()) =
    check(ccall((:nhp_disc_model_attach_score, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64), ctx.h, m, score, Int64(every)), ctx.h)

# -> (summary::NamedTuple over SCORE_FIELDS, per_node 3 x N rows lppd / p_waic / elpd_waic, pointwise R x N or nothing)
function score_fetch(score::Ptr{Cvoid}, N::Integer, R::Integer; pointwise=false, ctx=context())
    summary, per_node = Vector{Float64}(undef, 10), Vector{Float64}(undef, 3 * N)
    pw = pointwise ? Matrix{Float64}(undef, R, N) : nothing
    check(ccall((:nhp_disc_score_fetch, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                ctx.h, score, summary, per_node, pointwise ? pointer(pw) : Ptr{Float64}(C_NULL)), ctx.h)
    return NamedTuple{SCORE_FIELDS}(Tuple(summary)), permutedims(reshape(per_node, Int(N), 3)), pw
end

# the running planes (lse, mean, M2 of ℓ without its loggamma), each R x N
function score_fetch_planes(score::Ptr{Cvoid}, N::Integer, R::Integer; ctx=context())
    lse, mean, m2 = (Matrix{Float64}(undef, R, N) for _ in 1:3)
    check(ccall((:nhp_disc_score_fetch_planes, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                ctx.h, score, lse, mean, m2), ctx.h)
    return lse, mean, m2
end

# --- scoring a continuous chain (include/nhp.h: nhp_cont_score_*) ---------------------------------------------------------------
# The same wrappers for a continuous dataset handle `ds` and an nhp_cont_model handle `m`: a scorer on the blocks
# [edges[k], edges[k+1]) of the recording (0 <= edges[1] < ... < edges[end] <= duration), K = length(edges) - 1.
function cont_score_create(ds::Ptr{Cvoid}, edges::AbstractVector{<:Real}; ctx=context())
    e = Vector{Float64}(edges)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:nhp_cont_score_create, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64, Ref{Ptr{Cvoid}}),
                ctx.h, ds, e, Int64(length(e)), h), ctx.h)
    return h[]
end
cont_score_destroy(score::Ptr{Cvoid}) = ccall((:nhp_cont_score_destroy, libnhp), Cvoid, (Ptr{Cvoid},), score)
cont_score_reset!(score::Ptr{Cvoid}; ctx=context()) =
    check(ccall((:nhp_cont_score_reset, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.h, score), ctx.h)
cont_score_accumulate!(score::Ptr{Cvoid}, m::Ptr{Cvoid}; ctx=context()) =
    check(ccall((:nhp_cont_score_accumulate, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), ctx.h, score, m), ctx.h)
# every >= 1; score = C_NULL detaches every scorer of the model (detach before a scorer is destroyed)
cont_score_attach!(m::Ptr{Cvoid}, score::Ptr{Cvoid}, every::Integer=1; ctx=context()) =
    check(ccall((:nhp_cont_model_attach_score, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64), ctx.h, m, score, Int64(every)), ctx.h)

# -> (summary::NamedTuple over SCORE_FIELDS, per_node 3 x N, pointwise K x N or nothing)
function cont_score_fetch(score::Ptr{Cvoid}, N::Integer, K::Integer; pointwise=false, ctx=context())
    summary, per_node = Vector{Float64}(undef, 10), Vector{Float64}(undef, 3 * N)
    pw = pointwise ? Matrix{Float64}(undef, K, N) : nothing
    check(ccall((:nhp_cont_score_fetch, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                ctx.h, score, summary, per_node, pointwise ? pointer(pw) : Ptr{Float64}(C_NULL)), ctx.h)
    return NamedTuple{SCORE_FIELDS}(Tuple(summary)), permutedims(reshape(per_node, Int(N), 3)), pw
end

function cont_score_fetch_planes(score::Ptr{Cvoid}, N::Integer, K::Integer; ctx=context())
    lse, mean, m2 = (Matrix{Float64}(undef, K, N) for _ in 1:3)
    check(ccall((:nhp_cont_score_fetch_planes, libnhp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                ctx.h, score, lse, mean, m2), ctx.h)
    return lse, mean, m2
end

end # module
