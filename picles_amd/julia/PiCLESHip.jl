# PiCLESHip.jl — Julia-side binding of libpicles_hip.so (include/picles_hip.h).
#
# Drop-in for the 2D time step of PiCLES: a `WaveGrowth2DHIP <: Abstract2DModel` whose
# `time_step!`, `movie_time_step!`, `time_step!_advance`, `time_step!_remesh` and
# `init_particles!` methods forward to the HIP kernels through `ccall`, so `run!(sim)`
# (src/Simulations/run.jl:36-122) works unchanged.
#
# The field `State` is a `LazyState <: AbstractArray{Float64,3}`: the data lives in HBM, the host
# mirror is pulled only when somebody READS it, and the write `run!` performs every iteration —
# `sim.model.State .= 0.0` (run.jl:75-79) — is RECORDED and passed to the library as
# PICLES_STEP_ZERO_FIRST, where the zero-fill rides on the scatter's store.  An unobserved
# `State .= 0; time_step!` loop therefore stays on the fused one-launch-per-step path and moves
# nothing over PCIe; `push_state_to_storage!` / `copy(model.State)` pull once per stored step.
#
# STATUS: UNEXECUTED.  Julia is not installed in the build container or on the GPU boxes, so this file is
# syntax-reviewed only.  The same protocol is carried by picles_amd/models.py (`LazyState`),
# picles_amd/timesteppers.py and picles_amd/simulations.py, which ARE executed against the same C
# symbols (tests/test_gpu_lazy_state.py: an unobserved 10-step run! loop makes 10 fused launches,
# <= 1 stand-alone scatter and no State transfer).  Struct layouts mirror include/picles_hip.h
# field by field (ABI version 4; tests/test_capi_symbols.py holds the struct blocks below against the header).
module PiCLESHip

using PiCLES
using DifferentialEquations: DP5, Tsit5
using PiCLES.Architectures: Abstract2DModel
using PiCLES.Grids.CartesianGrid: TwoDCartesianGridMesh
using PiCLES.custom_structures: N_Periodic
import PiCLES.Operators.TimeSteppers: time_step!, movie_time_step!, time_step!_advance, time_step!_remesh
import PiCLES.Simulations: init_particles!

const libpicles = get(ENV, "PICLES_HIP_LIB", "libpicles_hip.so")
const PICLES_ABI_VERSION = Int32(20)

# ---- C structs (include/picles_hip.h) ----------------------------------------------------
struct picles_grid
    Nx::Int32; Ny::Int32
    dx::Float64; dy::Float64
    periodic_x::Int32; periodic_y::Int32
    mask::Ptr{Int8}
    j_begin::Int32; j_end::Int32
end

struct picles_phys
    r_g::Float64; C_alpha::Float64; C_phi::Float64; C_e::Float64; g::Float64
    gamma::Float64; q::Float64
    c_beta::Float64; c_D::Float64; c_e::Float64; c_alpha::Float64
    propagation::Int32; input::Int32; dissipation::Int32; peak_shift::Int32; direction::Int32
    _pad0::Int32
    dir_deadband::Float64
end

struct picles_ode
    abstol::Float64; reltol::Float64; dt0::Float64; dtmin::Float64
    force_dtmin::Int32; solver::Int32
    maxiters::Int64
    log_energy_minimum::Float64; log_energy_maximum::Float64; wind_min_squared::Float64
    timestep::Float64
end

struct picles_model
    periodic_boundary::Int32; init_type::Int32
    default_particle::NTuple{3,Float64}
    minimal_state::NTuple{2,Float64}
end

struct picles_counters
    rhs_evals::UInt64; steps_accepted::UInt64; steps_rejected::UInt64; reseeds::UInt64
    clamps::UInt64; maxiters_hits::UInt64; particles_advanced::UInt64; halo_overflow::UInt64
    max_reach::Int32; max_reach_seen::Int32
    dropped_nonfinite::UInt64
    wave_attempt_slots::UInt64
end

const STEP_ZERO_FIRST = Int32(1)
const STEP_MOVIE      = Int32(2)
const STEP_ATOMIC     = Int32(4)
# per-particle status bits (picles_get_particles)
const ST_MAXITERS, ST_RESEED_NAN, ST_RESEED_INF, ST_DTMIN, ST_NONFINITE = Int32(2), Int32(4), Int32(8), Int32(64), Int32(128)

check(ctx, rc, what) = rc == 0 || error("$what failed (rc=$rc): " *
    unsafe_string(ccall((:picles_last_error, libpicles), Cstring, (Ptr{Cvoid},), ctx)))

# ---- State: a lazy host view of the device field --------------------------------------------
"""
    LazyState

`model.State` as the rest of PiCLES sees it (`Array{Float64,3}(Nx, Ny, 3)` semantics) while the field lives in HBM.
`host_valid`: the host mirror equals the device field.  `dirty`: the mirror was written element-wise and must be
uploaded before the next step.  `zeroed`: the last write was `State .= 0` — nothing is executed, the next
`time_step!` passes `PICLES_STEP_ZERO_FIRST`.  (Python twin: picles_amd.models.LazyState.)
"""
mutable struct LazyState <: AbstractArray{Float64,3}
    host::Array{Float64,3}
    ctx::Ptr{Cvoid}
    host_valid::Bool
    dirty::Bool
    zeroed::Bool
    pulls::Int
    uploads::Int
end
LazyState(Nx::Integer, Ny::Integer) = LazyState(zeros(Nx, Ny, 3), C_NULL, false, false, false, 0, 0)

Base.size(s::LazyState) = size(s.host)
Base.IndexStyle(::Type{LazyState}) = IndexLinear()

function pull!(s::LazyState)
    if s.zeroed && !s.dirty
        s.host_valid || fill!(s.host, 0.0)
        s.host_valid = true
    elseif !s.host_valid && !s.dirty
        check(s.ctx, ccall((:picles_get_state, libpicles), Int32, (Ptr{Cvoid}, Ptr{Float64}), s.ctx, s.host), "picles_get_state")
        s.host_valid = true
        s.pulls += 1
    end
    return s.host
end

Base.getindex(s::LazyState, i::Int) = @inbounds pull!(s)[i]
function Base.setindex!(s::LazyState, v, i::Int)
    @inbounds pull!(s)[i] = v
    s.dirty = true; s.zeroed = false
    return v
end
# `State .= 0.0` lowers to copyto!(State, Broadcasted(identity, (0.0,))) and Base routes that to fill!(State, 0.0)
function Base.fill!(s::LazyState, x)
    if iszero(x)
        s.zeroed = true; s.dirty = false; s.host_valid = false
    else
        fill!(pull!(s), x)
        s.dirty = true; s.zeroed = false
    end
    return s
end
Base.copy(s::LazyState) = copy(pull!(s))
Base.Array(s::LazyState) = copy(pull!(s))

"called by the steppers: upload a written mirror; returns true if the step starts from a zeroed State"
function before_step!(s::LazyState)
    if s.dirty
        check(s.ctx, ccall((:picles_set_state, libpicles), Int32, (Ptr{Cvoid}, Ptr{Float64}), s.ctx, s.host), "picles_set_state")
        s.uploads += 1
        s.dirty = false
        return false
    end
    return s.zeroed
end
after_step!(s::LazyState) = (s.host_valid = false; s.zeroed = false; s.dirty = false; nothing)

# ---- the model type -----------------------------------------------------------------------
mutable struct WaveGrowth2DHIP{G,W,C} <: Abstract2DModel
    grid::G
    winds::W                      # (u = (x,y,t)->..., v = ...): sampled on the host, never called on device
    clock::C
    ODEsettings
    ODEdefaults
    minimal_state::Vector{Float64}
    periodic_boundary::Bool
    ocean_points::Vector
    State::LazyState              # lazy host view of the device field (what run! zeroes and stores)
    MovieState::Union{Nothing,Array{Float64,3}}
    FailedCollection::Vector
    ctx::Ptr{Cvoid}
    mask::Matrix{Int8}
    winds_static::Bool
    winds_uploaded::Bool          # static winds: sampled and shipped once
    wind_level::Union{Nothing,Tuple{Float64,Matrix{Float64},Matrix{Float64}}}   # (t, u, v) sampled for the end of the last step
end

"""
    WaveGrowth2DHIP(; grid, winds, ODEsets, γ, q, IDConstants, ...)

Same keywords as `WaveGrowth2D` (src/Models/WaveGrowthModels2D.jl:194-208); `γ, q, IDConstants` and the five switches
are the keyword arguments that would go to `particle_equations`, because the RHS itself runs inside the HIP kernel.
`wind_lattice = (x, y, t, u, v)` hands gridded winds (`Utils/WindEmulator.jl:18-43`) to the device once
(`picles_set_wind_grid`): no wind data crosses PCIe inside the time loop.
"""
function WaveGrowth2DHIP(; grid::TwoDCartesianGridMesh, winds, ODEsets, γ, q, IDConstants,
        propagation=true, input=true, dissipation=true, peak_shift=true, direction=true,
        ODEinit_type="wind_sea", minimal_state=nothing, periodic_boundary=true,
        clock, device::Integer=0, winds_static::Bool=false, wind_lattice=nothing, wind_lattice_mode::Symbol=:linear)
    ccall((:picles_abi_version, libpicles), Int32, ()) == PICLES_ABI_VERSION ||
        error("libpicles_hip.so: ABI version mismatch (this binding expects $PICLES_ABI_VERSION)")
    st = grid.stats
    mask = Matrix{Int8}(grid.data.mask)
    ms = isnothing(minimal_state) ? PiCLES.FetchRelations.MinimalState(2, 2, ODEsets.timestep) : minimal_state
    P = ODEsets.Parameters
    per_y = st.Ny isa N_Periodic ? 1 : (nameof(typeof(st.Ny)) == :N_TripolarNorth ? 2 : 0)
    g = Ref(picles_grid(st.Nx.N, st.Ny.N, st.dx, st.dy, st.Nx isa N_Periodic, per_y,
                        pointer(mask), 0, st.Ny.N))
    p = Ref(picles_phys(P.r_g, P.C_α, P.C_φ, P.C_e, P.g, γ, q,
                        IDConstants.c_β, IDConstants.c_D, IDConstants.c_e, IDConstants.c_alpha,
                        propagation, input, dissipation, peak_shift, direction, 0, 0.0))
    solver_id = ODEsets.solver isa DP5 ? 0 : ODEsets.solver isa Tsit5 ? 1 : 2     # 2 = AutoTsit5(Rosenbrock23()), the default
    o = Ref(picles_ode(ODEsets.abstol, ODEsets.reltol, ODEsets.dt, ODEsets.dtmin, ODEsets.force_dtmin, solver_id,
                       ODEsets.maxiters, ODEsets.log_energy_minimum, ODEsets.log_energy_maximum,
                       ODEsets.wind_min_squared, ODEsets.timestep))
    fixed = !(ODEinit_type isa String)
    dp = fixed ? (ODEinit_type.lne, ODEinit_type.c̄_x, ODEinit_type.c̄_y) : (0.0, 0.0, 0.0)
    m = Ref(picles_model(periodic_boundary, fixed, dp, (ms[1], ms[2])))
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve mask ccall((:picles_create, libpicles), Int32,
        (Ref{picles_grid}, Ref{picles_phys}, Ref{picles_ode}, Ref{picles_model}, Int32, Int32, Ref{Ptr{Cvoid}}),
        g, p, o, m, device, 1, ctx)
    rc == 0 || error("picles_create failed (rc=$rc): " *
        unsafe_string(ccall((:picles_last_error, libpicles), Cstring, (Ptr{Cvoid},), C_NULL)))
    Nx, Ny = st.Nx.N, st.Ny.N
    ocean = findall(mask .== 1)
    periodic_boundary && append!(ocean, findall(mask .== 3))
    state = LazyState(Nx, Ny)
    state.ctx = ctx[]
    model = WaveGrowth2DHIP(grid, winds, clock, ODEsets, fixed ? ODEinit_type : nothing, collect(Float64, ms),
        periodic_boundary, ocean, state, nothing, [], ctx[], mask, winds_static, false, nothing)
    if wind_lattice !== nothing
        x, y, t, u, v = wind_lattice            # regular knots; u, v :: Array{Float64,3}(nx, ny, nt)
        check(ctx[], ccall((:picles_set_wind_grid, libpicles), Int32,
            (Ptr{Cvoid}, Int32, Int32, Int32, Float64, Float64, Float64, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Float64, Float64),
            ctx[], length(x), length(y), length(t), x[1], x[2] - x[1], y[1], y[2] - y[1], t[1], t[2] - t[1],
            u, v, grid.data.x[1, 1], grid.data.y[1, 1]), "picles_set_wind_grid")
        # time semantics inside a model step (include/picles_hip.h): :linear — the interpolant itself, a time knot inside the step is a
        # kink the RHS sees (what wind_interpolator's linear_interpolation gives the reference, Utils/WindEmulator.jl:18-43; a step
        # holding two or more knots is refused); :smooth3 — the lattice tabulates a smooth closure, three levels and the parabola
        wind_lattice_mode === :smooth3 && check(ctx[], ccall((:picles_set_wind_grid_mode, libpicles), Int32, (Ptr{Cvoid}, Int32),
            ctx[], Int32(1)), "picles_set_wind_grid_mode")
        model.winds_uploaded = true               # the device samples every step by itself
        model.winds_static = true
    end
    finalizer(mdl -> ccall((:picles_destroy, libpicles), Int32, (Ptr{Cvoid},), mdl.ctx), model)
    return model
end

# node-sample the wind closures for [t, t+Δt] by broadcast — the only place user closures run.  Static winds are
# shipped once; time-varying winds go as THREE levels (t, t+Δt/2, t+Δt: the kernels evaluate the parabola through them at
# every Runge-Kutta stage time, the stand-in for the reference calling u_wind(x,y,t) inside the RHS,
# particle_waves_v5.jl:494-495) and reuse the level sampled for the end of the previous step.
function upload_winds!(model::WaveGrowth2DHIP, t, Δt)
    model.winds_static && model.winds_uploaded && return
    x, y = model.grid.data.x, model.grid.data.y
    lvl = model.wind_level
    u0, v0 = (lvl !== nothing && lvl[1] == t) ? (lvl[2], lvl[3]) :
             (Matrix{Float64}(model.winds.u.(x, y, t)), Matrix{Float64}(model.winds.v.(x, y, t)))
    if model.winds_static
        rc = ccall((:picles_set_winds, libpicles), Int32,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Float64),
            model.ctx, u0, v0, t, C_NULL, C_NULL, t)
        model.winds_uploaded = true
    else
        um = Matrix{Float64}(model.winds.u.(x, y, t + Δt / 2))
        vm = Matrix{Float64}(model.winds.v.(x, y, t + Δt / 2))
        u1 = Matrix{Float64}(model.winds.u.(x, y, t + Δt))
        v1 = Matrix{Float64}(model.winds.v.(x, y, t + Δt))
        rc = ccall((:picles_set_winds3, libpicles), Int32,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64),
            model.ctx, u0, v0, t, um, vm, u1, v1, t + Δt)
        model.wind_level = (t + Δt, u1, v1)
    end
    check(model.ctx, rc, "picles_set_winds")
end

function counters(model::WaveGrowth2DHIP)
    c = Ref{picles_counters}()
    check(model.ctx, ccall((:picles_get_counters, libpicles), Int32, (Ptr{Cvoid}, Ref{picles_counters}), model.ctx, c), "picles_get_counters")
    return c[]
end

"""
diagnostic: `(busy, calm, order)` — the dispatch order the latest whole-grid fused step filed for its successor (the cost-ordered
dispatch of mixed calm / busy runs), or `nothing` when the run is not mixed
"""
function dispatch_order(model::WaveGrowth2DHIP)
    n = ccall((:picles_get_dispatch_order, libpicles), Int32, (Ptr{Cvoid}, Ptr{Int32}, Int32), model.ctx, C_NULL, 0)
    n < 0 && check(model.ctx, n, "picles_get_dispatch_order")
    n == 0 && return nothing
    out = Vector{Int32}(undef, 2 + n)
    ccall((:picles_get_dispatch_order, libpicles), Int32, (Ptr{Cvoid}, Ptr{Int32}, Int32), model.ctx, out, length(out)) == n || return nothing
    return (Int(out[1]), Int(out[2]), out[3:end])
end

"""
diagnostic: `(class_waves, empty_waves)` — waves of the wave-per-row fused step whose pull skipped the candidate codes because their
whole neighbourhood carried one record code, and those among them whose neighbourhood held no record
"""
function pull_class_counts(model::WaveGrowth2DHIP)
    out = zeros(Int64, 2)
    check(model.ctx, ccall((:picles_get_pull_class_counts, libpicles), Int32, (Ptr{Cvoid}, Ptr{Int64}), model.ctx, out), "picles_get_pull_class_counts")
    return (out[1], out[2])
end

"""
particles that could not be scattered: farther than the reach cap of the pull scatter (64 cells per model step for a
whole-grid context — a deliberate limit of this implementation, INTEGRATION.md; the reference wraps at any distance) or
with a non-finite position (the reference throws in `Int(floor(NaN))`).  They are counted, never silently lost.
"""
function check_dropped(model::WaveGrowth2DHIP)
    c = counters(model)
    (c.halo_overflow > 0 || c.dropped_nonfinite > 0) &&
        @warn "PiCLESHip: particles were NOT scattered" beyond_reach_cap=c.halo_overflow non_finite_position=c.dropped_nonfinite
    return c
end

"`debug=true` (TimeSteppers.jl:113-120, run.jl:84-92): particles whose last advance failed, from the per-particle status bits"
function collect_failed!(model::WaveGrowth2DHIP)
    N = length(model.mask)
    status = Vector{Int32}(undef, N)
    check(model.ctx, ccall((:picles_get_particles, libpicles), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Int32}), model.ctx, C_NULL, C_NULL, C_NULL, status), "picles_get_particles")
    bad = ST_MAXITERS | ST_DTMIN | ST_NONFINITE | ST_RESEED_NAN | ST_RESEED_INF
    model.FailedCollection = [(position_ij=Tuple(CartesianIndices(model.mask)[k]), status=status[k], time=model.clock.time)
                              for k in 1:N if (status[k] & bad) != 0]
    return model.FailedCollection
end

# ---- the drop-in methods --------------------------------------------------------------------
# init_particles!(model) — run.jl:199-247
function init_particles!(model::WaveGrowth2DHIP; defaults=nothing, verbose::Bool=false)
    model.winds_uploaded = model.winds_uploaded && model.winds_static && model.wind_level === nothing
    upload_winds!(model, 0.0, model.ODEsettings.timestep)
    check(model.ctx, ccall((:picles_seed, libpicles), Int32, (Ptr{Cvoid}, Float64), model.ctx, model.clock.time), "picles_seed")
    after_step!(model.State)
    nothing
end

# time_step!(model, Δt) — TimeSteppers.jl:109-166.  run! zeroes State before calling (run.jl:75-79); the lazy view
# has recorded that, and the zero-fill is requested with ZERO_FIRST (fused into the scatter's store).
function time_step!(model::WaveGrowth2DHIP, Δt::Float64; callbacks=nothing, debug=false)
    upload_winds!(model, model.clock.time, Δt)
    flags = before_step!(model.State) ? STEP_ZERO_FIRST : Int32(0)
    check(model.ctx, ccall((:picles_time_step, libpicles), Int32, (Ptr{Cvoid}, Float64, Int32), model.ctx, Δt, flags), "picles_time_step")
    after_step!(model.State)
    PiCLES.Operators.TimeSteppers.tick!(model.clock, Δt)
    if debug
        collect_failed!(model)
        check_dropped(model)
    end
    callbacks === nothing || callbacks(model)
    nothing
end

# movie_time_step!(model, Δt) — TimeSteppers.jl:212-247
function movie_time_step!(model::WaveGrowth2DHIP, Δt; callbacks=nothing, debug=false)
    upload_winds!(model, model.clock.time, Δt)
    before_step!(model.State) &&
        check(model.ctx, ccall((:picles_zero_state, libpicles), Int32, (Ptr{Cvoid},), model.ctx), "picles_zero_state")
    check(model.ctx, ccall((:picles_time_step, libpicles), Int32, (Ptr{Cvoid}, Float64, Int32), model.ctx, Δt, STEP_MOVIE), "picles_time_step")
    model.MovieState === nothing && (model.MovieState = Array{Float64,3}(undef, size(model.State)...))
    check(model.ctx, ccall((:picles_get_movie_state, libpicles), Int32, (Ptr{Cvoid}, Ptr{Float64}), model.ctx, model.MovieState), "picles_get_movie_state")
    after_step!(model.State)                    # State is zero on the device after the remesh (:245)
    PiCLES.Operators.TimeSteppers.tick!(model.clock, Δt)
    debug && collect_failed!(model)
    nothing
end

# time_step!_advance / time_step!_remesh — TimeSteppers.jl:168-193
function time_step!_advance(model::WaveGrowth2DHIP, Δt::Float64, FailedCollection)
    upload_winds!(model, model.clock.time, Δt)
    before_step!(model.State) &&
        check(model.ctx, ccall((:picles_zero_state, libpicles), Int32, (Ptr{Cvoid},), model.ctx), "picles_zero_state")
    check(model.ctx, ccall((:picles_advance, libpicles), Int32, (Ptr{Cvoid}, Float64, Int32), model.ctx, Δt, 0), "picles_advance")
    after_step!(model.State)
end

function time_step!_remesh(model::WaveGrowth2DHIP, Δt::Float64)
    before_step!(model.State)                   # uploads a written mirror
    check(model.ctx, ccall((:picles_remesh, libpicles), Int32, (Ptr{Cvoid}, Float64), model.ctx, Δt), "picles_remesh")
end

"""
    run_stored!(model, Δt, n_steps, sink!; every=1, slots=3)

The stepping loop of `run!(sim; store=true)` (run.jl:72-114, storing.jl:109-119) with the device-side snapshot ring:
`picles_run_steps` enqueues `every` fused steps from C, `picles_store_push` snapshots State on the device and copies
it to pinned host memory on a side stream while the next steps run; `sink!(i, state::Array{Float64,3}, t)` receives the
snapshots in order (e.g. `(i, s, t) -> store["data"][i, :, :, :] = s`).
"""
function run_stored!(model::WaveGrowth2DHIP, Δt::Float64, n_steps::Integer, sink!; every::Integer=1, slots::Integer=3)
    upload_winds!(model, model.clock.time, Δt)
    model.winds_static || error("run_stored! needs winds the device can produce by itself (static winds or wind_lattice)")
    check(model.ctx, ccall((:picles_store_init, libpicles), Int32, (Ptr{Cvoid}, Int32), model.ctx, slots), "picles_store_init")
    buf = Array{Float64,3}(undef, size(model.State)...)
    t = Ref(0.0)
    i = 1
    drain_one() = begin
        check(model.ctx, ccall((:picles_store_pop, libpicles), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ref{Float64}), model.ctx, buf, t), "picles_store_pop")
        sink!(i, buf, t[]); i += 1
    end
    done = 0
    while done < n_steps
        k = min(every, n_steps - done)
        check(model.ctx, ccall((:picles_run_steps, libpicles), Int32, (Ptr{Cvoid}, Float64, Int32), model.ctx, Δt, k), "picles_run_steps")
        for _ in 1:k
            PiCLES.Operators.TimeSteppers.tick!(model.clock, Δt)
        end
        done += k
        ccall((:picles_store_pending, libpicles), Int32, (Ptr{Cvoid},), model.ctx) == slots && drain_one()
        check(model.ctx, ccall((:picles_store_push, libpicles), Int32, (Ptr{Cvoid},), model.ctx), "picles_store_push")
    end
    while ccall((:picles_store_pending, libpicles), Int32, (Ptr{Cvoid},), model.ctx) > 0
        drain_one()
    end
    after_step!(model.State)
    check_dropped(model)
    nothing
end

const DIAG_FIELDS = (:hs, :tp, :cg_x, :cg_y, :e, :m_x, :m_y)      # PICLES_DIAG_* bits in plane order

"""
    run_fields!(model, Δt, n_steps, sink!; every=10, coarsen=(4, 4), fields=(:hs, :tp, :cg_x, :cg_y), slots=3)

The stepping loop of `run!` with coarse wave fields as its output instead of State snapshots: what `PartitionOutput`
(examples/example_00_minimal_state_vector.jl:21-57), `GetGroupVelocity` (Operators/core_2D.jl:138-147) and `mean_of_state` /
`max_energy` (Operators/TimeSteppers.jl:15-29) derive from State on the host is formed on the device (`picles_diag_*`, the
definition is in include/picles_hip.h).  `picles_run_steps` enqueues `every` fused steps from C, `picles_diag_push` reduces State
to float32 planes and tile partials and copies them to pinned host memory on a side stream while the next steps run;
`sink!(i, planes::Array{Float32,3}, partials::Matrix{Float64}, t)` receives the snapshots in order, the first being the state the
loop starts from: `planes[I, J, f]` with f in the order of `DIAG_FIELDS`, `partials[:, k]` the seven doubles
(sum_e, sum_mx, sum_my, n_wet, max_e, max_mx, max_my) of tile k, to be summed / maximised sequentially in k.
"""
function run_fields!(model::WaveGrowth2DHIP, Δt::Float64, n_steps::Integer, sink!; every::Integer=10, coarsen=(4, 4),
                     fields=(:hs, :tp, :cg_x, :cg_y), slots::Integer=3)
    upload_winds!(model, model.clock.time, Δt)
    model.winds_static || error("run_fields! needs winds the device can produce by itself (static winds or wind_lattice)")
    mask = Int32(0)
    for f in fields
        k = findfirst(==(Symbol(f)), DIAG_FIELDS)
        k === nothing && error("unknown diagnostic field $f")
        mask |= Int32(1) << (k - 1)
    end
    check(model.ctx, ccall((:picles_diag_init, libpicles), Int32, (Ptr{Cvoid}, Int32, Int32, Int32, Int32), model.ctx, coarsen[1], coarsen[2], mask, slots), "picles_diag_init")
    nxc, nyc, nf, np = Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0)
    nbytes = Ref{Csize_t}(0)
    ccall((:picles_diag_shape, libpicles), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Csize_t}), model.ctx, nxc, nyc, nf, np, nbytes) == 0 ||
        error("picles_diag_shape failed")
    planes = Array{Float32,3}(undef, nxc[], nyc[], nf[])
    partials = Matrix{Float64}(undef, 7, np[])
    t = Ref(0.0)
    i = 1
    drain_one() = begin
        check(model.ctx, ccall((:picles_diag_pop, libpicles), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ref{Float64}), model.ctx, planes, partials, t), "picles_diag_pop")
        sink!(i, planes, partials, t[]); i += 1
    end
    check(model.ctx, ccall((:picles_diag_push, libpicles), Int32, (Ptr{Cvoid},), model.ctx), "picles_diag_push")
    done = 0
    while done < n_steps
        k = min(every, n_steps - done)
        check(model.ctx, ccall((:picles_run_steps, libpicles), Int32, (Ptr{Cvoid}, Float64, Int32), model.ctx, Δt, k), "picles_run_steps")
        for _ in 1:k
            PiCLES.Operators.TimeSteppers.tick!(model.clock, Δt)
        end
        done += k
        k == every || break                       # a remainder shorter than `every` ends the run without an output
        ccall((:picles_diag_pending, libpicles), Int32, (Ptr{Cvoid},), model.ctx) == slots && drain_one()
        check(model.ctx, ccall((:picles_diag_push, libpicles), Int32, (Ptr{Cvoid},), model.ctx), "picles_diag_push")
    end
    while ccall((:picles_diag_pending, libpicles), Int32, (Ptr{Cvoid},), model.ctx) > 0
        drain_one()
    end
    after_step!(model.State)
    check_dropped(model)
    nothing
end

"""
    wind_stream_init!(model, x, y, t0, dt; slots=3)
    wind_stream_push!(model, k, u, v; stream=C_NULL)
    diag_export!(model, fields, partials=C_NULL; stream=C_NULL)

Coupling (`picles_wind_stream_*`, `picles_diag_export`; the contract is in include/picles_hip.h, "streamed winds"): the winds as a
lattice over the regular axes `x`, `y` whose time levels `t0 + k dt` arrive one at a time in a ring of `slots` levels on the device,
and the coarse diagnostics written into the caller's device buffers.  `wind_stream_push!` takes host `Matrix{Float64}` /
`Matrix{Float32}` levels `[nx, ny]`, or device pointers (`Ptr{Float64}` / `Ptr{Float32}`, e.g. of a ROCArray) with the HIP stream
that produces them: the library orders its copy behind that stream and the stream behind the copy.  A step whose levels are not
held is refused by `picles_run_steps` / `picles_time_step` with a text that names the missing level.  `diag_export!` needs
`picles_diag_init` first (`run_fields!` makes it); `fields` and `partials` are device pointers.
"""
function wind_stream_init!(model::WaveGrowth2DHIP, x::AbstractVector{<:Real}, y::AbstractVector{<:Real}, t0::Real, dt::Real; slots::Integer=3)
    grid = model.grid
    check(model.ctx, ccall((:picles_wind_stream_init, libpicles), Int32,
        (Ptr{Cvoid}, Int32, Int32, Float64, Float64, Float64, Float64, Float64, Float64, Float64, Float64, Int32),
        model.ctx, length(x), length(y), x[1], x[2] - x[1], y[1], y[2] - y[1], t0, dt, grid.data.x[1, 1], grid.data.y[1, 1], slots), "picles_wind_stream_init")
    model.winds_uploaded = true      # the device produces every window by itself: upload_winds! has nothing to do, the chunked paths apply
    model.winds_static = true
    nothing
end

function wind_stream_push!(model::WaveGrowth2DHIP, k::Integer, u::Matrix{T}, v::Matrix{T}) where {T<:Union{Float32,Float64}}
    size(u) == size(v) || error("wind_stream_push!: u and v differ in shape")
    check(model.ctx, ccall((:picles_wind_stream_push, libpicles), Int32, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}),
        model.ctx, k, u, v, T === Float32 ? 1 : 0, 0, C_NULL), "picles_wind_stream_push")
    nothing
end

function wind_stream_push!(model::WaveGrowth2DHIP, k::Integer, u::Ptr{T}, v::Ptr{T}; stream::Ptr{Cvoid}=C_NULL) where {T<:Union{Float32,Float64}}
    check(model.ctx, ccall((:picles_wind_stream_push, libpicles), Int32, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}),
        model.ctx, k, u, v, T === Float32 ? 1 : 0, 1, stream), "picles_wind_stream_push")
    nothing
end

function diag_export!(model::WaveGrowth2DHIP, fields::Ptr{Float32}, partials::Ptr{Float64}=Ptr{Float64}(C_NULL); stream::Ptr{Cvoid}=C_NULL)
    check(model.ctx, ccall((:picles_diag_export, libpicles), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}),
        model.ctx, fields, partials, stream), "picles_diag_export")
    after_step!(model.State)
    nothing
end

const FLUX_FIELDS = (:phi_in, :phi_dis, :phi_shift, :tq_in_x, :tq_in_y, :tq_dis_x, :tq_dis_y, :us_x, :us_y)      # PICLES_FLUX_* bits in plane order

"""
    flux_init!(model; coarsen=(4, 4), fields=FLUX_FIELDS, rho_water=1025.0, slots=3)
    flux_shape(model) -> (nxc, nyc, n_fields, n_partials, bytes)
    flux_push!(model); flux_pop!(model, planes, partials) -> t; flux_pending(model)
    flux_export!(model, fields, partials=C_NULL; stream=C_NULL)
    flux_free!(model)
    run_fluxes!(model, Δt, n_steps, sink!; every=10, coarsen=(4, 4), fields=FLUX_FIELDS, rho_water=1025.0, slots=3)

Coupling fluxes (`picles_flux_*`; the contract is in include/picles_hip.h, "coupling fluxes"): what the partner models consume —
the energy and momentum the waves take out of the wind (`phi_in`, `tq_in`: the wave-supported stress), what the breaking waves
hand down to the ocean (`phi_dis`, `tq_dis`) and the surface Stokes drift (`us`) — formed on the device from State and the wind at
the clock, as area means over coarse cells.  `rho_water` sets the scales: the `phi` planes come in W m⁻² (`rho_water * g`), the `tq`
planes in N m⁻².  `run_fluxes!` is `run_fields!` with these planes: `sink!(i, planes::Array{Float32,3}, partials::Matrix{Float64}, t)`,
`partials[:, k]` the eleven doubles (nine unscaled sums, n_active, n_bad) of tile k.  A push or export at a clock where the wind
window holds no level is refused: the end of every model step is a level.
"""
function flux_init!(model::WaveGrowth2DHIP; coarsen=(4, 4), fields=FLUX_FIELDS, rho_water::Real=1025.0, slots::Integer=3)
    mask = Int32(0)
    for f in fields
        k = findfirst(==(Symbol(f)), FLUX_FIELDS)
        k === nothing && error("unknown flux plane $f")
        mask |= Int32(1) << (k - 1)
    end
    check(model.ctx, ccall((:picles_flux_init, libpicles), Int32, (Ptr{Cvoid}, Int32, Int32, Int32, Float64, Float64, Int32),
        model.ctx, coarsen[1], coarsen[2], mask, Float64(rho_water) * 9.81, Float64(rho_water), slots), "picles_flux_init")
    nothing
end

function flux_shape(model::WaveGrowth2DHIP)
    nxc, nyc, nf, np = Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0)
    nbytes = Ref{Csize_t}(0)
    ccall((:picles_flux_shape, libpicles), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Csize_t}), model.ctx, nxc, nyc, nf, np, nbytes) == 0 ||
        error("picles_flux_shape failed: flux_init! first")
    (nxc[], nyc[], nf[], np[], nbytes[])
end

flux_push!(model::WaveGrowth2DHIP) = (check(model.ctx, ccall((:picles_flux_push, libpicles), Int32, (Ptr{Cvoid},), model.ctx), "picles_flux_push"); after_step!(model.State); nothing)

function flux_pop!(model::WaveGrowth2DHIP, planes::Array{Float32,3}, partials::Matrix{Float64})
    t = Ref(0.0)
    check(model.ctx, ccall((:picles_flux_pop, libpicles), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ref{Float64}), model.ctx, planes, partials, t), "picles_flux_pop")
    t[]
end

flux_pending(model::WaveGrowth2DHIP) = ccall((:picles_flux_pending, libpicles), Int32, (Ptr{Cvoid},), model.ctx)

function flux_export!(model::WaveGrowth2DHIP, fields::Ptr{Float32}, partials::Ptr{Float64}=Ptr{Float64}(C_NULL); stream::Ptr{Cvoid}=C_NULL)
    check(model.ctx, ccall((:picles_flux_export, libpicles), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}),
        model.ctx, fields, partials, stream), "picles_flux_export")
    after_step!(model.State)
    nothing
end

flux_free!(model::WaveGrowth2DHIP) = (check(model.ctx, ccall((:picles_flux_free, libpicles), Int32, (Ptr{Cvoid},), model.ctx), "picles_flux_free"); nothing)

"""
    flux_mean_init!(model; every=1, first=1)
    flux_mean_shape(model) -> (every, n_planes, bytes)
    flux_mean_update!(model; stream=C_NULL)
    flux_mean_push!(model; reset=true)                       # served by flux_pop! / flux_pending
    flux_mean_export!(model, fields, partials=C_NULL; stream=C_NULL, reset=true)
    flux_mean_get(model) -> (planes::Array{Float64,3}, n_samples, t_first, t_last)
    flux_mean_set!(model, planes, n_samples, t_first, t_last)
    flux_mean_reset!(model); flux_mean_free!(model)

Flux means (`picles_flux_mean_*`; the contract is in include/picles_hip.h, "flux means"): the coupling fluxes accumulated on the
device behind every model step — a pending fused step stays pending — and exported as the mean over the samples of a coupling
interval.  The set takes its cells, mask and scales from the flux set (`flux_init!` first).  `flux_mean_get` returns the eleven raw
fp64 accumulator planes `[Nxc, nyc, 11]`; a picked-up run puts them back with `flux_mean_set!`.
"""
flux_mean_init!(model::WaveGrowth2DHIP; every::Integer=1, first::Integer=1) =
    (check(model.ctx, ccall((:picles_flux_mean_init, libpicles), Int32, (Ptr{Cvoid}, Int32, Int32), model.ctx, every, first), "picles_flux_mean_init"); nothing)

function flux_mean_shape(model::WaveGrowth2DHIP)
    ev = Ref{Int32}(0); npl = Ref{Int32}(0); nbytes = Ref{Csize_t}(0)
    ccall((:picles_flux_mean_shape, libpicles), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Csize_t}), model.ctx, ev, npl, nbytes) == 0 ||
        error("picles_flux_mean_shape failed: flux_mean_init! first")
    (Int(ev[]), Int(npl[]), Int(nbytes[]))
end

flux_mean_update!(model::WaveGrowth2DHIP; stream::Ptr{Cvoid}=C_NULL) =
    (check(model.ctx, ccall((:picles_flux_mean_update, libpicles), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), model.ctx, stream), "picles_flux_mean_update"); nothing)

flux_mean_push!(model::WaveGrowth2DHIP; reset::Bool=true) =
    (check(model.ctx, ccall((:picles_flux_mean_push, libpicles), Int32, (Ptr{Cvoid}, Int32), model.ctx, reset ? 1 : 0), "picles_flux_mean_push"); nothing)

function flux_mean_export!(model::WaveGrowth2DHIP, fields::Ptr{Float32}, partials::Ptr{Float64}=Ptr{Float64}(C_NULL); stream::Ptr{Cvoid}=C_NULL,
                           reset::Bool=true)
    check(model.ctx, ccall((:picles_flux_mean_export, libpicles), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}, Int32),
        model.ctx, fields, partials, stream, reset ? 1 : 0), "picles_flux_mean_export")
    nothing
end

function flux_mean_get(model::WaveGrowth2DHIP)
    nxc, nyc, _, _, _ = flux_shape(model)
    planes = Array{Float64,3}(undef, nxc, nyc, 11)
    n = Ref{Int64}(0); t0 = Ref{Float64}(0.0); t1 = Ref{Float64}(0.0)
    check(model.ctx, ccall((:picles_flux_mean_get, libpicles), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ref{Int64}, Ref{Float64}, Ref{Float64}),
        model.ctx, planes, n, t0, t1), "picles_flux_mean_get")
    (planes, n[], t0[], t1[])
end

function flux_mean_set!(model::WaveGrowth2DHIP, planes::Array{Float64,3}, n_samples::Integer, t_first::Real, t_last::Real)
    nxc, nyc, _, _, _ = flux_shape(model)
    size(planes) == (nxc, nyc, 11) || error("flux_mean_set!: planes must be $nxc x $nyc x 11")
    check(model.ctx, ccall((:picles_flux_mean_set, libpicles), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Float64, Float64),
        model.ctx, planes, n_samples, Float64(t_first), Float64(t_last)), "picles_flux_mean_set")
    nothing
end

flux_mean_reset!(model::WaveGrowth2DHIP) = (check(model.ctx, ccall((:picles_flux_mean_reset, libpicles), Int32, (Ptr{Cvoid},), model.ctx), "picles_flux_mean_reset"); nothing)
flux_mean_free!(model::WaveGrowth2DHIP) = (check(model.ctx, ccall((:picles_flux_mean_free, libpicles), Int32, (Ptr{Cvoid},), model.ctx), "picles_flux_mean_free"); nothing)

function run_fluxes!(model::WaveGrowth2DHIP, Δt::Float64, n_steps::Integer, sink!; every::Integer=10, coarsen=(4, 4),
                     fields=FLUX_FIELDS, rho_water::Real=1025.0, slots::Integer=3)
    upload_winds!(model, model.clock.time, Δt)
    model.winds_static || error("run_fluxes! needs winds the device can produce by itself (static winds or wind_lattice)")
    flux_init!(model; coarsen=coarsen, fields=fields, rho_water=rho_water, slots=slots)
    nxc, nyc, nf, np, _ = flux_shape(model)
    planes = Array{Float32,3}(undef, nxc, nyc, nf)
    partials = Matrix{Float64}(undef, 11, np)
    i = 1
    drain_one() = begin
        t = flux_pop!(model, planes, partials)
        sink!(i, planes, partials, t); i += 1
    end
    flux_push!(model)
    done = 0
    while done < n_steps
        k = min(every, n_steps - done)
        check(model.ctx, ccall((:picles_run_steps, libpicles), Int32, (Ptr{Cvoid}, Float64, Int32), model.ctx, Δt, k), "picles_run_steps")
        for _ in 1:k
            PiCLES.Operators.TimeSteppers.tick!(model.clock, Δt)
        end
        done += k
        k == every || break                       # a remainder shorter than `every` ends the run without an output
        flux_pending(model) == slots && drain_one()
        flux_push!(model)
    end
    while flux_pending(model) > 0
        drain_one()
    end
    flux_free!(model)
    check_dropped(model)
    nothing
end

"""
    probe_init!(model, nodes; every=1, first=1, capacity=64)

Station probes (`picles_probe_*`, the contract is in include/picles_hip.h): `nodes` is a vector of 1-based `(i, j)` (Julia indices
of `State[i, j, :]`).  After every model step `s` with `s >= first` and `(s - first) % every == 0` the library samples
`State[i, j, :]` at these nodes on the device — from the scatter records of the pending fused step, which stays pending — and
copies the sample to pinned host memory beside the steps that follow.  What the reference's scripts cut out of `cash_store`
snapshots (tests/T04_2D_reg_test.jl) without a snapshot.  `probe_sample!` takes one sample now (the seeded state), `probe_pop!`
hands out the oldest samples, `probe_free!` drops the set.
"""
function probe_init!(model::WaveGrowth2DHIP, nodes; every::Integer=1, first::Integer=1, capacity::Integer=64)
    n = length(nodes)
    ij = Vector{Int32}(undef, 2n)
    for (k, (i, j)) in enumerate(nodes)
        ij[k] = Int32(i - 1); ij[n + k] = Int32(j - 1)
    end
    check(model.ctx, ccall((:picles_probe_init, libpicles), Int32, (Ptr{Cvoid}, Int32, Ptr{Int32}, Int32, Int32, Int32), model.ctx, n, ij, every, first, capacity), "picles_probe_init")
    nothing
end

probe_sample!(model::WaveGrowth2DHIP) =
    check(model.ctx, ccall((:picles_probe_sample, libpicles), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), model.ctx, C_NULL), "picles_probe_sample")

probe_pending(model::WaveGrowth2DHIP) = ccall((:picles_probe_pending, libpicles), Int32, (Ptr{Cvoid},), model.ctx)

"`(values[node, k, sample], times, steps)` of the oldest samples (all that are pending by default); k = e, m_x, m_y"
function probe_pop!(model::WaveGrowth2DHIP; max_samples::Integer=typemax(Int32))
    n, every, cap = Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0)
    ccall((:picles_probe_shape, libpicles), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}), model.ctx, n, every, cap) == 0 ||
        error("picles_probe_shape failed: probe_init! first")
    m = max(1, min(Int(max_samples), Int(probe_pending(model))))
    values = Array{Float64,3}(undef, n[], 3, m)
    times = Vector{Float64}(undef, m)
    steps = Vector{Int64}(undef, m)
    got = Ref{Int32}(0)
    check(model.ctx, ccall((:picles_probe_pop, libpicles), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ref{Int32}), model.ctx, m, values, times, steps, got), "picles_probe_pop")
    values[:, :, 1:got[]], times[1:got[]], steps[1:got[]]
end

probe_free!(model::WaveGrowth2DHIP) = check(model.ctx, ccall((:picles_probe_free, libpicles), Int32, (Ptr{Cvoid},), model.ctx), "picles_probe_free")

"""
    track_init!(model, times, corners, weights, horizon)
    track_sample!(model); track_fetch_begin!(model, k0, n); track_fetch_end!(model, n); track_info(model); track_free!(model)

Track samples (`picles_track_*`, the contract is in include/picles_hip.h): the sea state at events `(t_k, x_k, y_k)` along moving
platforms.  `times` is sorted; `corners` is an `m × 4` matrix of 1-based `(i, j)` tuples and `weights` an `m × 4` matrix, in the
visiting order of `locate_points` (picles_amd/station_output.py); `horizon` is the longest step to come.  Behind every step the
library samples the events whose time lies next to the clock and keeps, per event, the latest sample before and the earliest after
it in a table on the device.  `track_fetch_begin!` (0-based first event `k0`, `n` events) starts the copy of a range of the table,
`track_fetch_end!` hands it out as an `n × 8` matrix (columns e_b, mx_b, my_b, t_b, e_a, mx_a, my_a, t_a).
"""
function track_init!(model::WaveGrowth2DHIP, times::AbstractVector{<:Real}, corners::AbstractMatrix, weights::AbstractMatrix{<:Real}, horizon::Real)
    m = length(times)
    size(corners) == (m, 4) && size(weights) == (m, 4) || error("track_init!: corners and weights must be m × 4")
    t = Vector{Float64}(times)
    ij = Vector{Int32}(undef, 8m)
    w = Vector{Float64}(undef, 4m)
    for c in 1:4, k in 1:m
        ij[(c - 1) * m + k] = Int32(corners[k, c][1] - 1); ij[(3 + c) * m + k] = Int32(corners[k, c][2] - 1)
        w[(c - 1) * m + k] = Float64(weights[k, c])
    end
    check(model.ctx, ccall((:picles_track_init, libpicles), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Float64), model.ctx, m, t, ij, w, horizon), "picles_track_init")
    nothing
end

track_sample!(model::WaveGrowth2DHIP) =
    check(model.ctx, ccall((:picles_track_sample, libpicles), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), model.ctx, C_NULL), "picles_track_sample")

track_fetch_begin!(model::WaveGrowth2DHIP, k0::Integer, n::Integer) =
    check(model.ctx, ccall((:picles_track_fetch_begin, libpicles), Int32, (Ptr{Cvoid}, Int32, Int32), model.ctx, k0, n), "picles_track_fetch_begin")

function track_fetch_end!(model::WaveGrowth2DHIP, n::Integer)
    out = Matrix{Float64}(undef, n, 8)
    check(model.ctx, ccall((:picles_track_fetch_end, libpicles), Int32, (Ptr{Cvoid}, Ptr{Float64}), model.ctx, out), "picles_track_fetch_end")
    out
end

"`(m, horizon, samples_taken)` of the track set"
function track_info(model::WaveGrowth2DHIP)
    m, h, s = Ref{Int32}(0), Ref{Float64}(0.0), Ref{Int64}(0)
    ccall((:picles_track_info, libpicles), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Float64}, Ref{Int64}), model.ctx, m, h, s) == 0 ||
        error("picles_track_info failed: track_init! first")
    Int(m[]), h[], Int(s[])
end

track_free!(model::WaveGrowth2DHIP) = check(model.ctx, ccall((:picles_track_free, libpicles), Int32, (Ptr{Cvoid},), model.ctx), "picles_track_free")

"""
    bforce_init!(model, nodes; band=false, weights=nothing)
    bforce_set_levels!(model, t0, v0[, t1, v1])
    bforce_free!(model)

Open-boundary forcing (`picles_bforce_*`, the contract is in include/picles_hip.h): `nodes` is a vector of 1-based `(i, j)`, each a
grid-boundary node (mask class 3) of a model without `periodic_boundary`.  Behind every model step's launch a particle is born at
each of them from the prescribed `(e, m_x, m_y)` at the step's start time, advanced with the model's solver and scattered with the
others; fused steps stay fused.  `v0`, `v1` are `n x 3` matrices; one level is constant in time, two are followed linearly in `t`,
and every step must start inside `[t0, t1]`: set the next pair before the clock leaves the window.
"""
function bforce_init!(model::WaveGrowth2DHIP, nodes; band::Bool=false, weights::Union{Nothing,AbstractVector}=nothing)
    n = length(nodes)
    ij = Vector{Int32}(undef, 2n)
    for (k, (i, j)) in enumerate(nodes)
        ij[k] = Int32(i - 1); ij[n + k] = Int32(j - 1)
    end
    if band || weights !== nothing
        # a band set (`picles_bforce_init_band`): ocean nodes (mask class 1) are taken too and are not stepped while the set lives;
        # `weights` in (0, 1] blend the prescribed value into the model's own State, v = m + w (p - m)
        w = weights === nothing ? nothing : Vector{Float64}(weights)
        w === nothing || length(w) == n || error("bforce_init!: one weight per node")
        GC.@preserve w begin
            pw = w === nothing ? Ptr{Float64}(C_NULL) : pointer(w)
            check(model.ctx, ccall((:picles_bforce_init_band, libpicles), Int32, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Float64}), model.ctx, n, ij, pw), "picles_bforce_init_band")
        end
    else
        check(model.ctx, ccall((:picles_bforce_init, libpicles), Int32, (Ptr{Cvoid}, Int32, Ptr{Int32}), model.ctx, n, ij), "picles_bforce_init")
    end
    nothing
end

function bforce_set_levels!(model::WaveGrowth2DHIP, t0::Real, v0::AbstractMatrix, t1::Real=t0, v1::Union{Nothing,AbstractMatrix}=nothing)
    a = Matrix{Float64}(v0)
    b = v1 === nothing ? nothing : Matrix{Float64}(v1)
    size(a, 2) == 3 && (b === nothing || size(b) == size(a)) || error("bforce_set_levels!: levels are n x 3 matrices of (e, m_x, m_y)")
    GC.@preserve a b begin
        pb = b === nothing ? Ptr{Float64}(C_NULL) : pointer(b)
        check(model.ctx, ccall((:picles_bforce_set_levels, libpicles), Int32, (Ptr{Cvoid}, Float64, Ptr{Float64}, Float64, Ptr{Float64}), model.ctx, Float64(t0), pointer(a), Float64(t1), pb), "picles_bforce_set_levels")
    end
    nothing
end

bforce_free!(model::WaveGrowth2DHIP) = check(model.ctx, ccall((:picles_bforce_free, libpicles), Int32, (Ptr{Cvoid},), model.ctx), "picles_bforce_free")

"""
    bforce_get_levels(model) -> (v0, v1)

The levels as the device holds them, `n x 3` matrices of `(e, m_x, m_y)` (`nothing` for a level the set does not hold);
stream-ordered behind whatever wrote them, completes no pending step.
"""
function bforce_get_levels(model::WaveGrowth2DHIP)
    n, lv = Ref{Int32}(0), Ref{Int32}(0)
    ccall((:picles_bforce_info, libpicles), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ptr{Float64}, Ptr{Float64}), model.ctx, n, lv, C_NULL, C_NULL) == 0 ||
        error("bforce_get_levels: bforce_init! first")
    a = lv[] >= 1 ? Matrix{Float64}(undef, n[], 3) : nothing
    b = lv[] >= 2 ? Matrix{Float64}(undef, n[], 3) : nothing
    GC.@preserve a b begin
        pa = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
        pb = b === nothing ? Ptr{Float64}(C_NULL) : pointer(b)
        check(model.ctx, ccall((:picles_bforce_get_levels, libpicles), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), model.ctx, pa, pb), "picles_bforce_get_levels")
    end
    a, b
end

"""
    nest_init!(child, parent, corner_nodes, index, weights)
    nest_sample!(child)
    nest_free!(child)

One-way nesting (`picles_nest_*`, the contract is in include/picles_hip.h): the forcing set of `child` (`bforce_init!` first) takes
its levels from the State of `parent`, a whole-grid model on the same device.  `corner_nodes` is a vector of distinct 1-based
`(i, j)` in the parent; `index` (`n x 4`, 1-based into `corner_nodes`) and `weights` (`n x 4`) give, per forced child node in the
set's order, the four corners to mix — the station definition of the header.  `nest_sample!` takes a level from the parent as it
stands now (level 0 first, then level 1, then the pair rotates) and returns after enqueueing; the child then steps inside
`[t0, t1]` (`r` steps for a refinement of `r`), the parent takes a step, and the next sample follows.
"""
function nest_init!(child::WaveGrowth2DHIP, parent::WaveGrowth2DHIP, corner_nodes, index::AbstractMatrix, weights::AbstractMatrix)
    nc = length(corner_nodes)
    ij = Vector{Int32}(undef, 2nc)
    for (k, (i, j)) in enumerate(corner_nodes)
        ij[k] = Int32(i - 1); ij[nc + k] = Int32(j - 1)
    end
    size(index, 2) == 4 && size(index) == size(weights) || error("nest_init!: index and weights are n x 4 matrices")
    ix = Matrix{Int32}(index .- 1)          # column-major n x 4: four planes of n
    w = Matrix{Float64}(weights)
    check(child.ctx, ccall((:picles_nest_init, libpicles), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}), child.ctx, parent.ctx, nc, ij, ix, w), "picles_nest_init")
    nothing
end

nest_sample!(child::WaveGrowth2DHIP) = check(child.ctx, ccall((:picles_nest_sample, libpicles), Int32, (Ptr{Cvoid},), child.ctx), "picles_nest_sample")

nest_free!(child::WaveGrowth2DHIP) = check(child.ctx, ccall((:picles_nest_free, libpicles), Int32, (Ptr{Cvoid},), child.ctx), "picles_nest_free")

"""
    nest_set_levels!(child, t0, v0, t1, v1)

A nest resumed (`picles_nest_set_levels`, ABI 16; the contract is in include/picles_hip.h): the pair a checkpointed child held —
`n x 3` matrices of `(e, m_x, m_y)` as `bforce_get_levels(child)` returned them, NaN rows included, over `[t0, t1]` — put back into
a fresh nest as if two samples had been taken.  Load both models' blobs first (`pickup!`); the parent's clock must be `t1`.
"""
function nest_set_levels!(child::WaveGrowth2DHIP, t0::Real, v0::AbstractMatrix, t1::Real, v1::AbstractMatrix)
    a, b = Matrix{Float64}(v0), Matrix{Float64}(v1)
    size(a, 2) == 3 && size(b) == size(a) || error("nest_set_levels!: levels are n x 3 matrices of (e, m_x, m_y)")
    GC.@preserve a b begin
        check(child.ctx, ccall((:picles_nest_set_levels, libpicles), Int32, (Ptr{Cvoid}, Float64, Ptr{Float64}, Float64, Ptr{Float64}), child.ctx, Float64(t0), pointer(a), Float64(t1), pointer(b)), "picles_nest_set_levels")
    end
    nothing
end

"""
    nest_prolong!(child, parent, ix0, ix1, wx, iy0, iy1, wy, dt)

A child started from its parent (`picles_nest_prolong`, ABI 15; the contract is in include/picles_hip.h): the State of `parent` at its
clock `t`, prolonged onto every node of `child`, and the child's particles made from it with the library's remesh at clock `t` and step
`dt`; the child is reset as `picles_seed(child, t)` resets it.  Per child column `i` the 1-based parent columns `ix0[i]`, `ix1[i]` and
the weight `wx[i]`, per child row `j` the parent rows `iy0[j]`, `iy1[j]` and `wy[j]` (weights in `[0, 1]`; a periodic parent's wrap
cell is `ix0 = Nx`, `ix1 = 1`).  Returns after enqueueing.
"""
function nest_prolong!(child::WaveGrowth2DHIP, parent::WaveGrowth2DHIP, ix0, ix1, wx, iy0, iy1, wy, dt::Real)
    a0, a1, b0, b1 = (Vector{Int32}(v .- 1) for v in (ix0, ix1, iy0, iy1))
    fx, fy = Vector{Float64}(wx), Vector{Float64}(wy)
    check(child.ctx, ccall((:picles_nest_prolong, libpicles), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Float64), child.ctx, parent.ctx, a0, a1, fx, b0, b1, fy, Float64(dt)), "picles_nest_prolong")
    nothing
end

"""
    nest_relocate!(child, parent, si, sj, keep_margin, ix0, ix1, wx, iy0, iy1, wy, dt; mesh_x0 = 0.0, mesh_y0 = 0.0)

A child moved across its parent between two legs of a nested run (`picles_nest_relocate`, ABI 18; the contract is in
include/picles_hip.h): the box is translated by `(si, sj)` child nodes; new node `(i, j)` keeps the State of old node `(i + si, j + sj)`
where that lies at least `keep_margin` nodes inside the old box, and takes the parent's prolonged State elsewhere.  The tables are
`nest_prolong!`'s, for the NEW box (1-based).  `mesh_x0`, `mesh_y0`: the new coordinates of node (1, 1), for a wind lattice the child
holds (ignored without one).  The child is reset as `picles_seed(child, t)` resets it and remeshed with step `dt`; MovieState then holds
the relocated State.  Refused for a child that still holds a nest, a forcing set, a feedback or a statistics set, that has land, a
periodic axis, a metric or a wind stream, and for unequal clocks.  Returns after enqueueing.
"""
function nest_relocate!(child::WaveGrowth2DHIP, parent::WaveGrowth2DHIP, si::Integer, sj::Integer, keep_margin::Integer, ix0, ix1, wx, iy0, iy1, wy, dt::Real;
                        mesh_x0::Real = 0.0, mesh_y0::Real = 0.0)
    a0, a1, b0, b1 = (Vector{Int32}(v .- 1) for v in (ix0, ix1, iy0, iy1))
    fx, fy = Vector{Float64}(wx), Vector{Float64}(wy)
    check(child.ctx, ccall((:picles_nest_relocate, libpicles), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Float64, Float64, Float64), child.ctx, parent.ctx, Int32(si), Int32(sj), Int32(keep_margin), a0, a1, fx, b0, b1, fy, Float64(dt), Float64(mesh_x0), Float64(mesh_y0)), "picles_nest_relocate")
    nothing
end

"""
    nest_feedback_init!(child, fb_nodes, src_nodes, index, weights)
    nest_feedback!(child)
    nest_feedback_info(child)
    nest_feedback_free!(child)

Two-way nesting (`picles_nest_feedback_*`, the contract is in include/picles_hip.h): the nested `child` (`nest_init!` first) feeds its
State back into its parent.  `fb_nodes` is a vector of 1-based `(i, j)` of the parent's ocean nodes to feed, `src_nodes` one of
distinct 1-based `(i, j)` of the child; `index` (`n_fb x m`, 1-based into `src_nodes`) and `weights` (`n_fb x m`, `>= 0`, `0.0`
marking padding) give the restriction stencil per feedback node.  `nest_feedback!` takes one level at the child's clock, which must
be the parent's, and returns after enqueueing; the parent's next step bears its feedback particles from it.
`nest_feedback_info` returns `(n_fb, n_src, m, taken)`.
"""
function nest_feedback_init!(child::WaveGrowth2DHIP, fb_nodes, src_nodes, index::AbstractMatrix, weights::AbstractMatrix)
    planes(nodes) = begin
        n = length(nodes)
        ij = Vector{Int32}(undef, 2n)
        for (k, (i, j)) in enumerate(nodes)
            ij[k] = Int32(i - 1); ij[n + k] = Int32(j - 1)
        end
        ij
    end
    nf, ns = length(fb_nodes), length(src_nodes)
    size(index, 1) == nf && size(index) == size(weights) || error("nest_feedback_init!: index and weights are n_fb x m matrices")
    fb, sn = planes(fb_nodes), planes(src_nodes)
    ix = Matrix{Int32}(index .- 1)          # column-major n_fb x m: m planes of n_fb
    w = Matrix{Float64}(weights)
    check(child.ctx, ccall((:picles_nest_feedback_init, libpicles), Int32, (Ptr{Cvoid}, Int32, Ptr{Int32}, Int32, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Float64}), child.ctx, nf, fb, ns, sn, size(index, 2), ix, w), "picles_nest_feedback_init")
    nothing
end

nest_feedback!(child::WaveGrowth2DHIP) = check(child.ctx, ccall((:picles_nest_feedback, libpicles), Int32, (Ptr{Cvoid},), child.ctx), "picles_nest_feedback")

function nest_feedback_info(child::WaveGrowth2DHIP)
    a, b, m, t = Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0), Ref{Int64}(0)
    ccall((:picles_nest_feedback_info, libpicles), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Int64}), child.ctx, a, b, m, t) == 0 ||
        error("picles_nest_feedback_info failed: nest_feedback_init! first")
    (a[], b[], m[], t[])
end

nest_feedback_free!(child::WaveGrowth2DHIP) = check(child.ctx, ccall((:picles_nest_feedback_free, libpicles), Int32, (Ptr{Cvoid},), child.ctx), "picles_nest_feedback_free")

const PICLES_STAT_PEAK, PICLES_STAT_MEAN, PICLES_STAT_EXCEED = Int32(1), Int32(2), Int32(4)

"""
    stat_init!(model; peak=true, mean=true, thresholds=Float64[], every=1, first=1)

Run statistics (`picles_stat_*`, the contract is in include/picles_hip.h): per-node accumulators of every node, kept in device
memory and updated behind every model step `s` with `s >= first` and `(s - first) % every == 0` — from the scatter records of the
pending fused step, which stays pending.  `thresholds` (1 ... 4 ascending Hs values) selects the exceedance counts.  `stat_get`
returns the planes as a `Dict` of `Nx x Ny` arrays (`:n_exc` is `Nx x Ny x length(thresholds)`) with `:n_samples`, `:t_first`,
`:t_last`; `stat_set!` uploads such a `Dict` (a picked-up run continues its window); `stat_reset!` zeroes; `stat_free!` drops the set.
"""
function stat_init!(model::WaveGrowth2DHIP; peak::Bool=true, mean::Bool=true, thresholds=Float64[], every::Integer=1, first::Integer=1)
    thr = Vector{Float64}(thresholds)
    mask = (peak ? PICLES_STAT_PEAK : Int32(0)) | (mean ? PICLES_STAT_MEAN : Int32(0)) | (isempty(thr) ? Int32(0) : PICLES_STAT_EXCEED)
    check(model.ctx, ccall((:picles_stat_init, libpicles), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Int32, Int32), model.ctx, mask, length(thr), thr, every, first), "picles_stat_init")
    nothing
end

function stat_shape(model::WaveGrowth2DHIP)
    mask, nthr, every, npl = Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0)
    thr = zeros(Float64, 4)
    bytes = Ref{Csize_t}(0)
    ccall((:picles_stat_shape, libpicles), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ptr{Float64}, Ref{Int32}, Ref{Int32}, Ref{Csize_t}), model.ctx, mask, nthr, thr, every, npl, bytes) == 0 ||
        error("picles_stat_shape failed: stat_init! first")
    (mask = mask[], thresholds = thr[1:nthr[]], every = every[], n_planes = npl[], bytes = Int(bytes[]))
end

stat_update!(model::WaveGrowth2DHIP) =
    check(model.ctx, ccall((:picles_stat_update, libpicles), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), model.ctx, C_NULL), "picles_stat_update")

# the plane block of picles_stat_get / picles_stat_set: fp64 planes first, then the uint32 ones
function stat_layout(mask::Integer, nthr::Integer)
    lay = Tuple{Symbol,DataType,Int}[]
    mask & PICLES_STAT_PEAK != 0 && append!(lay, [(s, Float64, 1) for s in (:e_peak, :mx_peak, :my_peak, :t_peak)])
    mask & PICLES_STAT_MEAN != 0 && append!(lay, [(s, Float64, 1) for s in (:sum_e, :sum_mx, :sum_my, :sum_hs)])
    push!(lay, (:n_wet, UInt32, 1))
    mask & PICLES_STAT_EXCEED != 0 && push!(lay, (:n_exc, UInt32, Int(nthr)))
    lay
end

function stat_get(model::WaveGrowth2DHIP)
    sh = stat_shape(model)
    Nx, Ny = size(model.State, 1), size(model.State, 2)
    buf = Vector{UInt8}(undef, sh.bytes)
    n, t0, t1 = Ref{Int64}(0), Ref{Float64}(0.0), Ref{Float64}(0.0)
    check(model.ctx, ccall((:picles_stat_get, libpicles), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ref{Int64}, Ref{Float64}, Ref{Float64}), model.ctx, sh.mask, buf, n, t0, t1), "picles_stat_get")
    out = Dict{Symbol,Any}(:n_samples => n[], :t_first => t0[], :t_last => t1[], :thresholds => sh.thresholds, :mask => sh.mask)
    at = 0
    for (name, T, k) in stat_layout(sh.mask, length(sh.thresholds))
        nb = sizeof(T) * Nx * Ny * k
        a = collect(reinterpret(T, view(buf, at + 1:at + nb)))
        out[name] = name == :n_exc ? reshape(a, Nx, Ny, k) : reshape(a, Nx, Ny)
        at += nb
    end
    out
end

function stat_set!(model::WaveGrowth2DHIP, acc::Dict{Symbol,Any})
    sh = stat_shape(model)
    buf = UInt8[]
    for (name, T, k) in stat_layout(sh.mask, length(sh.thresholds))
        append!(buf, reinterpret(UInt8, vec(Array{T}(acc[name]))))
    end
    length(buf) == sh.bytes || error("stat_set!: the planes do not fill the set's plane block")
    check(model.ctx, ccall((:picles_stat_set, libpicles), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Float64, Float64), model.ctx, sh.mask, buf, Int64(acc[:n_samples]), Float64(acc[:t_first]), Float64(acc[:t_last])), "picles_stat_set")
    nothing
end

stat_reset!(model::WaveGrowth2DHIP) = check(model.ctx, ccall((:picles_stat_reset, libpicles), Int32, (Ptr{Cvoid},), model.ctx), "picles_stat_reset")
stat_free!(model::WaveGrowth2DHIP) = check(model.ctx, ccall((:picles_stat_free, libpicles), Int32, (Ptr{Cvoid},), model.ctx), "picles_stat_free")

"""
    checkpoint!(model, path; iteration = model.clock.iteration)

Exact-restart file of the model at its current step boundary (`picles_checkpoint_begin` + `picles_checkpoint_end`: the library's
blob, DESIGN.md §11) with the clock, in the layout of picles_amd/checkpointing.py: 8 bytes "PICLESCF" | UInt32 1 | Int32 -1 |
Int64 iteration | Float64 time | UInt64 blob bytes | blob.  Written to a temporary name, fsync'ed and renamed.
The reference accepts `run!(sim; pickup = true)` and ignores it (run.jl:36); `pickup!` is what that keyword means in Oceananigans.
"""
function checkpoint!(model::WaveGrowth2DHIP, path::AbstractString; iteration::Integer = model.clock.iteration)
    n = Ref{Csize_t}(0)
    check(model.ctx, ccall((:picles_checkpoint_size, libpicles), Int32, (Ptr{Cvoid}, Ref{Csize_t}), model.ctx, n), "picles_checkpoint_size")
    blob = Vector{UInt8}(undef, n[])
    check(model.ctx, ccall((:picles_checkpoint_begin, libpicles), Int32, (Ptr{Cvoid},), model.ctx), "picles_checkpoint_begin")
    check(model.ctx, ccall((:picles_checkpoint_end, libpicles), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), model.ctx, blob, n[]),
          "picles_checkpoint_end")
    tmp = joinpath(dirname(abspath(path)), "." * basename(path) * ".tmp-$(getpid())")
    open(tmp, "w") do io
        write(io, b"PICLESCF", htol(UInt32(1)), htol(Int32(-1)), htol(Int64(iteration)), htol(Float64(model.clock.time)),
              htol(UInt64(length(blob))), blob)
        flush(io)
        ccall(:fsync, Cint, (Cint,), Base.Libc.fd(io))
    end
    mv(tmp, path; force = true)
    path
end

"""
    pickup!(model, path)

Load a file of `checkpoint!` (or of picles_amd's Checkpointer) into a model built by the same script — grid, mask, physics,
ODE settings, winds — and restore its clock; the library refuses a file of another configuration, a truncated or damaged one.
"""
function pickup!(model::WaveGrowth2DHIP, path::AbstractString)
    raw = read(path)
    length(raw) >= 40 && raw[1:8] == b"PICLESCF" || error("$path: not a checkpoint file")
    iteration = ltoh(reinterpret(Int64, raw[17:24])[1])
    time = ltoh(reinterpret(Float64, raw[25:32])[1])
    nblob = ltoh(reinterpret(UInt64, raw[33:40])[1])
    length(raw) - 40 == nblob || error("$path: truncated checkpoint file")
    upload_winds!(model, time, model.ODEsettings.timestep)      # the wind source the blob's fingerprint covers
    blob = raw[41:end]
    check(model.ctx, ccall((:picles_checkpoint_load, libpicles), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), model.ctx, blob, length(blob)),
          "picles_checkpoint_load")
    model.clock.time = time
    model.clock.iteration = iteration
    after_step!(model.State)
    model
end

end # module
