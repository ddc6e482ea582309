/*
 * picles_hip.h — C ABI of the MI355X-native PiCLES 2D particle-in-cell time step.
 *
 * This header IS the drop-in boundary.  The reference (mochell/PiCLES, pure Julia)
 * has no FFI layer of its own; the functions a replacement must provide are the
 * Julia methods of Operators.TimeSteppers / Simulations listed next to each entry
 * point below (file:line are into the reference tree).  A Julia maintainer binds
 * them with `ccall`; the in-repo Python host layer
 * (picles_amd/) binds the very same symbols with ctypes.
 *
 * Conventions
 *   - every function returns int32: 0 = OK, <0 = error (text via picles_last_error)
 *   - all arrays handed across the ABI are caller-owned HOST memory unless the
 *     name says `_dev`; the library never frees caller memory and never calls back
 *   - fields are column-major [i + Nx*(j + Ny*k)] exactly like the reference's
 *     State[Nx,Ny,3] (k = e, m_x, m_y)   (WaveGrowthModels2D.jl:136-143)
 *   - a context belongs to ONE GPU (one process per GPU) and owns the rows
 *     [j_begin, j_end) of the global grid (y-slab); single-GPU use: 0, Ny
 *   - a context is not re-entrant (the reference calls time_step! from one task)
 *   - there is NO CPU fallback: creating a context without a HIP device fails
 */
#ifndef PICLES_HIP_H
#define PICLES_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PICLES_ABI_VERSION 20

/* ---- grid: TwoDCartesianGridStatistics + mesh mask (Grids/CartesianGrid.jl:26-101,
 *      Grids/mask_utils.jl:38-55) ------------------------------------------------ */
typedef struct picles_grid {
    int32_t Nx, Ny;          /* global node counts                                   */
    double  dx, dy;          /* node spacing [m]; ProjetionKernel M = diag(1/dx,1/dy) */
    int32_t periodic_x;      /* 1: Nx isa N_Periodic, 0: N_NonPeriodic (scatter wrap/drop) */
    int32_t periodic_y;      /* 0 / 1 likewise; 2: Ny isa N_TripolarNorth — open at the south edge, corners beyond the
                                north edge fold back mirrored in x (ParticleInCell.jl:353-361, 409-428); needs periodic_x */
    const int8_t *mask;      /* Nx*Ny total mask {0 land,1 ocean,2 land bnd,3 grid bnd};
                                NULL => all ocean + make_boundaries() ring on non-periodic axes */
    int32_t j_begin, j_end;  /* rows owned by this context (slab); 0, Ny for one device */
} picles_grid;

/* ---- physics: ODEParameters NamedTuple + particle_equations kwargs
 *      (particle_waves_v5.jl:107-128,154-162,184-196,382-395) -------------------- */
typedef struct picles_phys {
    double r_g, C_alpha, C_phi, C_e, g;   /* params NamedTuple (g is carried but, as in the
                                             reference :281-287,504, NOT used by the RHS)   */
    double gamma, q;                      /* particle_equations(u,v; γ, q)                  */
    double c_beta, c_D, c_e, c_alpha;     /* IDConstants fields entering e_T_func :271      */
    int32_t propagation, input, dissipation, peak_shift, direction;  /* RHS switches :383-387 */
    int32_t _pad0;
    double  dir_deadband;   /* OPT-IN, 0 = off (reference-exact).  |sin(θ_c - θ_w)| below this value is
                               treated as exact alignment in S_dir (particle_waves_v5.jl:345-346): round-off
                               misalignment (~1e-16) otherwise excites the stiff direction mode of the
                               explicit stepper.  1e-9 changes the RHS by < 1e-9 relative. */
} picles_phys;

/* ---- ODESettings (particle_waves_v5.jl:34-75) ---------------------------------- */
typedef struct picles_ode {
    double  abstol, reltol;
    double  dt0;             /* ODESettings.dt : initial dt of a freshly built integrator   */
    double  dtmin;
    int32_t force_dtmin;
    int32_t solver;          /* 0 = DP5 (Dormand-Prince 5(4), bench06:93); 1 = Tsit5 (the explicit
                                half of the ODESettings default); 2 = AutoTsit5(Rosenbrock23()),
                                the ODESettings default itself (particle_waves_v5.jl:47): Tsit5 with
                                the stiffness test of OrdinaryDiffEq's AutoSwitch and a Rosenbrock23
                                fallback on an exact hand-written Jacobian (restated, unpinned)   */
    int64_t maxiters;        /* per model step                        */
    double  log_energy_minimum, log_energy_maximum, wind_min_squared;
    double  timestep;        /* ODESettings.timestep: seed time-scale of init_particles!    */
} picles_ode;

/* ---- model flags (WaveGrowthModels2D.jl:194-345) ------------------------------- */
typedef struct picles_model {
    int32_t periodic_boundary;   /* model flag: selects ocean_points / boundary flag        */
    int32_t init_type;           /* 0 "wind_sea" (ODEdefaults = nothing); 1 fixed ParticleDefaults */
    double  default_particle[3]; /* lne, c̄_x, c̄_y when init_type == 1                      */
    double  minimal_state[2];    /* [E_min, m²_min]  (FetchRelations.MinimalState)          */
} picles_model;

/* flags of picles_time_step */
#define PICLES_STEP_ZERO_FIRST   1  /* run!: State .= 0 before time_step!  (run.jl:75-82)    */
#define PICLES_STEP_MOVIE        2  /* movie_time_step!: snapshot State->MovieState between
                                       advance and remesh, zero State after  (TimeSteppers.jl:212-247) */
#define PICLES_STEP_ATOMIC       4  /* scatter with the LDS-tiled fp64-atomic push instead of the
                                       deterministic (bitwise reproducible) pull                 */

/* per-particle status bits (returned by picles_get_particles) */
#define PICLES_ST_STEPPED        1  /* particle is in ocean_points                              */
#define PICLES_ST_MAXITERS       2  /* internal RK loop hit maxiters in the last advance        */
#define PICLES_ST_RESEED_NAN     4  /* NaN guard re-seeded (mapping_2D.jl:196-211)              */
#define PICLES_ST_RESEED_INF     8  /* Inf guard re-seeded (:213-222)                           */
#define PICLES_ST_CLAMPED       16  /* lne clamped to log_energy_maximum (:224-235)             */
#define PICLES_ST_SWITCHED_ON   32  /* off -> on by wind test in advance (:172-185)             */
#define PICLES_ST_DTMIN         64  /* stopped: dt <= dtmin without force_dtmin                 */
#define PICLES_ST_NONFINITE    128  /* a non-finite error estimate was rejected                 */

typedef struct picles_counters {
    uint64_t rhs_evals;       /* RHS evaluations                      */
    uint64_t steps_accepted;  /* accepted internal RK steps           */
    uint64_t steps_rejected;
    uint64_t reseeds;         /* NaN/Inf guards + off->on + remesh B/C */
    uint64_t clamps;
    uint64_t maxiters_hits;
    uint64_t particles_advanced;  /* particles that ran the ODE       */
    uint64_t halo_overflow;   /* particles that travelled beyond the scatter reach the context covers — halo_rows for a
                                 slab, 64 cells per model step for a whole-grid context — and were NOT scattered */
    int32_t  max_reach;       /* max |cell offset| any scatter corner had in the last advance */
    int32_t  max_reach_seen;  /* the largest max_reach since picles_seed / picles_reset_counters (slab halos are sized from it) */
    uint64_t dropped_nonfinite; /* switched-on particles whose advanced position was NaN / Inf: not scattered.  The reference
                                 would throw in Int(floor(NaN)) (ParticleInCell.jl:58-71); here they are dropped and counted */
    uint64_t wave_attempt_slots; /* sum over wavefronts of 64 x (the largest number of internal RK attempts any lane of the wave
                                 made): (steps_accepted + steps_rejected) / wave_attempt_slots is the lane efficiency of the
                                 adaptive advance — 1 when all particles of a wave take the same number of attempts */
} picles_counters;

typedef struct picles_timing {     /* accumulated device time, ms (HIP events on the compute stream) */
    double advance_ms, scatter_ms, remesh_ms, other_ms;
    uint64_t advance_launches, scatter_launches, remesh_launches;
} picles_timing;

typedef struct picles_ctx picles_ctx;

/* WaveGrowth2D(...) constructor: allocates State, particles (WaveGrowthModels2D.jl:194-345).
 * device_id: HIP device ordinal.  halo_rows: ghost rows kept on each side of the slab
 * (>= the scatter reach in y; ignored for a single slab covering [0,Ny) ). */
int32_t picles_create(const picles_grid *g, const picles_phys *p, const picles_ode *o,
                      const picles_model *m, int32_t device_id, int32_t halo_rows,
                      picles_ctx **out);
int32_t picles_destroy(picles_ctx *ctx);
const char *picles_last_error(const picles_ctx *ctx);   /* ctx may be NULL: last create() error */
int32_t picles_abi_version(void);

/* winds: node-sampled u,v (col-major, the context's own rows only: Nx*(j_end-j_begin))
 * at two time levels; the RHS lerps in t.  u1==NULL => time-constant.
 * Replaces the Julia closures winds.u(x,y,t) (particle_waves_v5.jl:494-495). */
int32_t picles_set_winds(picles_ctx *ctx, const double *u0, const double *v0, double t0,
                         const double *u1, const double *v1, double t1);
/* The same with a third level (um, vm) at the middle of the window, (t0 + t1)/2: the RHS evaluates the parabola through the
 * three levels.  For closures that are not linear in t inside a model step (tests/T04_2D_reg_test.jl:166-167 multiplies u by
 * cos(3t/(3600 2π))) the two-level form misses the reference's u_wind(x,y,t) at the stage times (particle_waves_v5.jl:494-495)
 * by (ω Δt)²/8 of the amplitude, this one by (ω Δt)³/125.  um == NULL is picles_set_winds. */
int32_t picles_set_winds3(picles_ctx *ctx, const double *u0, const double *v0, double t0,
                          const double *um, const double *vm,
                          const double *u1, const double *v1, double t1);
/* Three levels with the middle one at a KNOT of a gridded wind, t0 < tk < t1: the RHS evaluates the two straight segments
 * (t0,u0)-(tk,uk)-(t1,u1).  This is the exact form, inside one model step, of wind_interpolator's
 * linear_interpolation((x,y,t), u) (Utils/WindEmulator.jl:18-43) when one time knot of the lattice falls inside the step: the
 * reference's RHS evaluates that interpolant at every stage time (particle_waves_v5.jl:494-495), so the solver sees the kink.
 * A window without an interior knot is picles_set_winds; one with two or more is picles_set_winds_polyline. */
int32_t picles_set_winds_knot(picles_ctx *ctx, const double *u0, const double *v0, double t0,
                              const double *uk, const double *vk, double tk,
                              const double *u1, const double *v1, double t1);
/* The general form: nlev >= 2 node-sampled levels (u[k], v[k]) at strictly increasing times[k], times[0] and times[nlev-1] the
 * ends of the window — the piecewise-linear wind through them, i.e. the reference's interpolant inside a model step that holds
 * nlev - 2 time knots of the wind lattice.  2 levels = picles_set_winds, 3 = picles_set_winds_knot; more: a POLYLINE window,
 * u(s) = u0 + s du + Σ_k max(s - s_k, 0) b_k with one term per knot (at most PICLES_MAX_KNOTS = 8 knots).  A step under a polyline
 * window runs the plain phases (stand-alone advance, general flavour; scatter + remesh behind it) instead of the fused launch —
 * the same results to the bit, one launch more per step. */
#define PICLES_MAX_KNOTS 8
int32_t picles_set_winds_polyline(picles_ctx *ctx, int32_t nlev, const double *const *u, const double *const *v, const double *times);

/* Non-Cartesian meshes (SphericalGrid.jl:207-240, spherical_grid_corrections.jl:3-21): per-node
 * projection kernel M = diag(m11, m22) of the propagation terms (particle_waves_v5.jl:536) and the
 * great-circle coefficient of PropagationCorrection, S_sphere = c̄_x * pc (:521-530); own rows,
 * col-major.  NULL pointers restore the Cartesian constants M = diag(1/dx, 1/dy), pc = 0. */
int32_t picles_set_metric(picles_ctx *ctx, const double *m11, const double *m22, const double *pc);

/* Gridded wind forcing (Utils/WindEmulator.jl:18-43 wind_interpolator =
 * Interpolations.linear_interpolation((x,y,t), u; extrapolation_bc = Periodic())): u,v on a regular
 * (x,y,t) lattice [nx*ny*nt], x fastest.  The library keeps the lattice in HBM and samples the
 * time levels of every step at the mesh nodes itself (tri-linear, periodic continuation), so no
 * wind data crosses PCIe inside the time loop.  mesh_x0/mesh_y0: coordinates of node (0,0).
 * Replaces picles_set_winds until picles_set_winds is called again.
 * Time semantics inside a model step [t, t+Δt] (picles_set_wind_grid_mode; LINEAR after every picles_set_wind_grid):
 *   PICLES_LATTICE_LINEAR  the reference's: the interpolant itself, kinks included.  No lattice knot strictly inside the step:
 *                          two levels (t, t+Δt), a straight line.  One knot inside: a third level AT the knot, two straight
 *                          segments (= picles_set_winds_knot).  Two to PICLES_MAX_KNOTS knots inside one step: a level at every
 *                          knot, the polyline through them (= picles_set_winds_polyline; such a step takes the plain phases instead
 *                          of the fused launch).  More than PICLES_MAX_KNOTS: the step is REFUSED with an error text before it has
 *                          changed anything (take shorter steps, or the mode below).
 *   PICLES_LATTICE_SMOOTH3 for a lattice that tabulates a smooth closure u(x,y,t) (knots at Δt/2 or finer): three levels
 *                          (t, t+Δt/2, t+Δt), the parabola through them (= picles_set_winds3 with the lattice sampled on the
 *                          device) — what carries tests/T04_2D_reg_test.jl:166-167's cos(3t/(3600 2π)) forcing to 1e-3 with no
 *                          host work in the time loop.  An approximation of the closure by design, not of the interpolant. */
int32_t picles_set_wind_grid(picles_ctx *ctx, int32_t nx, int32_t ny, int32_t nt,
                             double x0, double dx, double y0, double dy, double t0, double dt,
                             const double *u, const double *v, double mesh_x0, double mesh_y0);
#define PICLES_LATTICE_LINEAR  0
#define PICLES_LATTICE_SMOOTH3 1
int32_t picles_set_wind_grid_mode(picles_ctx *ctx, int32_t mode);
/* The interior knot of the lattice in the window (t, t+dt), as the LINEAR mode classifies it: returns the number of lattice
 * time knots strictly inside (0, 1, or 2 = "two or more"); *tk = the time of the first one.  A knot closer to either end than
 * 1e-9 of the lattice spacing counts as that end.  Host arithmetic only; the host layers use it to build the same windows
 * from host-sampled levels (picles_set_winds_knot).  (The periodic continuation in t has a whole number of
 * lattice intervals as its period: knots stay at whole multiples of lat_dt from lat_t0.) */
int32_t picles_lattice_knots(double lat_t0, double lat_dt, double t, double dt, double *tk);
/* All of them: returns the number of lattice time knots strictly inside (t, t+dt) by the same rule and writes the times of the first
 * `cap` into tks (tks may be NULL with cap = 0). */
int32_t picles_lattice_knot_times(double lat_t0, double lat_dt, double t, double dt, double *tks, int32_t cap);
/* ---- streamed winds: a lattice whose time levels arrive one at a time, from device memory, in stream order (ABI 17) ---
 * The third source of the wind window, for a coupled run: an atmosphere hands over one level per coupling interval and does not know
 * the next.  A WIND STREAM is a lattice with regular (x, y) axes as in picles_set_wind_grid (the periodic continuation in x and y stays),
 * a time axis t_k = t0 + k dt, k = 0, 1, ... WITHOUT periodic continuation, and a ring of n_slots >= 2 level pairs (u, v) in HBM:
 * level k lives in slot k % n_slots.
 *
 * THE TIME RULE.  c = (t - t0) * (1 / dt), evaluated as the lattice sampler evaluates it; if |c - rint(c)| <= 1e-9, c := rint(c) (the
 * slack of picles_lattice_knots); k = floor(c), f = c - k.  A sample with f == 0 reads level k alone; otherwise it is, per corner,
 * L_k + (L_k+1 - L_k) f in exactly the operation order of the lattice sampler.  The host computes (k, f) once per sampled time and
 * hands slot indices and f to the kernel (k_wind_sample_ring).  A result never depends on WHEN a level was pushed.
 * picles_wind_stream_coord is that rule, host arithmetic only (returns -2 for dt <= 0 or a time before t0).
 *
 *   init   replaces whatever winds the context had, as picles_set_wind_grid does; the mode is PICLES_LATTICE_LINEAR and
 *          picles_set_wind_grid_mode works on it.  Refused: nx, ny < 2, non-positive spacing, n_slots < 2, slab mode, slabs, a nest
 *          (streamed nests are not carried).  picles_set_slab_mode(1) and picles_nest_init are refused while a stream exists.
 *   push   level k from planes of nx * ny values, x fastest; dtype PICLES_WIND_F64 | PICLES_WIND_F32, where PICLES_WIND_HOST |
 *          PICLES_WIND_DEVICE.  A DEVICE push records an event on caller_stream, lets the context's stream wait for it, fills the slot
 *          (a device-to-device copy for f64, k_wind_ingest for f32: widening is exact) and records an event that caller_stream waits
 *          for: the caller may overwrite its buffer in stream order.  caller_stream == NULL: the caller has synchronised already, and
 *          keeps the buffer until the context's stream has passed the copy.  A HOST push is complete on return.  Neither completes a
 *          pending fused step.  Refused before anything has changed: k is not newest + 1 (the first push of an empty ring may be any
 *          k >= 0; a level once held is not pushed again or corrected); the slot holds a level the clock's interval still needs,
 *          k - n_slots >= floor(c(clock)); NULL planes, unknown dtype / where.
 *   info   n_slots, the oldest and newest level held (-1, -1: none), pushes so far; any pointer may be NULL
 *   reset  completes a pending fused step (as picles_set_wind_grid_mode does), empties the ring and invalidates the window
 *
 * STEPS.  The window of a step is classified by the knots t_k strictly inside it with the rule of picles_lattice_knots: the TWO, KNOT,
 * POLYLINE and (PICLES_LATTICE_SMOOTH3) PARABOLA forms come out as for an uploaded lattice.  picles_time_step, picles_run_steps,
 * picles_advance, picles_begin_step and picles_begin_fused_step check BEFORE they enqueue anything that every level the windows of
 * the next n steps read is held, and refuse with -2 and a text that names the first missing k and its time.  A step with nk interior
 * knots reads nk + 2 levels: n_slots < nk + 2 is refused with its own text.  picles_seed reads the level(s) bracketing the seed time.
 * CHECKPOINT.  The fingerprint takes "stream", the geometry, t0, dt, the mode and n_slots, not the contents; the blob holds no levels.
 * picles_checkpoint_load invalidates the window; levels still in the ring stay valid; a fresh context needs the levels bracketing the
 * restored clock pushed again before it steps.  Irregular coupling intervals are not carried. */
#define PICLES_WIND_F64    0
#define PICLES_WIND_F32    1
#define PICLES_WIND_HOST   0
#define PICLES_WIND_DEVICE 1
int32_t picles_wind_stream_init(picles_ctx *ctx, int32_t nx, int32_t ny, double x0, double dx, double y0, double dy,
                                double t0, double dt, double mesh_x0, double mesh_y0, int32_t n_slots);
int32_t picles_wind_stream_push(picles_ctx *ctx, int64_t k, const void *u, const void *v, int32_t dtype, int32_t where, void *caller_stream);
int32_t picles_wind_stream_info(const picles_ctx *ctx, int32_t *n_slots, int64_t *oldest, int64_t *newest, int64_t *pushes);
int32_t picles_wind_stream_reset(picles_ctx *ctx);
int32_t picles_wind_stream_coord(double t0, double dt, double t, int64_t *k, double *f);
/* node winds currently on the device (own rows); any pointer may be NULL */
int32_t picles_get_winds(picles_ctx *ctx, double *u0, double *v0, double *u1, double *v1);
/* the mid-window level of three-level winds; returns 1 (and writes nothing) when the current winds have two levels */
int32_t picles_get_winds_mid(picles_ctx *ctx, double *um, double *vm);

/* init_particles!(model) + SeedParticle (run.jl:199-247, core_2D.jl:434-488); clock := t0 */
int32_t picles_seed(picles_ctx *ctx, double t0);

/* time_step!(model, Δt) / movie_time_step! (TimeSteppers.jl:109-166,212-247) */
int32_t picles_time_step(picles_ctx *ctx, double dt, int32_t flags);
/* n consecutive run!-style steps (State .= 0; time_step!) enqueued back to back from C: the loop of
 * run! (run.jl:72-114) when nothing observes State between the steps.  Asynchronous like picles_time_step. */
int32_t picles_run_steps(picles_ctx *ctx, double dt, int32_t n_steps);
/* time_step!_advance / time_step!_remesh (TimeSteppers.jl:168-193); remesh does NOT tick */
int32_t picles_advance(picles_ctx *ctx, double dt, int32_t flags);
int32_t picles_remesh(picles_ctx *ctx, double dt);
int32_t picles_tick(picles_ctx *ctx, double dt);          /* tick!(clock, Δt) :163 */
int32_t picles_zero_state(picles_ctx *ctx);               /* State .= 0  (run.jl:75-79) */
double  picles_clock(const picles_ctx *ctx);

/* State / MovieState access (own rows; 3 planes of Nx*(j_end-j_begin)) */
int32_t picles_get_state(picles_ctx *ctx, double *state);
int32_t picles_set_state(picles_ctx *ctx, const double *state);
int32_t picles_get_movie_state(picles_ctx *ctx, double *state);

/* ---- State snapshots for run!(…; store / cash_store) (run.jl:94-112, storing.jl:109-119) ----------
 * push: stream-ordered device copy of State into a ring slot, then an asynchronous D2H copy into
 * pinned host memory on a side stream — the next time steps overlap the PCIe transfer.
 * pop: wait for the OLDEST pushed snapshot and hand it out (Nx*ny_loc*3 doubles + its model time).
 * The host writes it wherever the store lives (HDF5 waves/data[time,x,y,state] in the reference). */
int32_t picles_store_init(picles_ctx *ctx, int32_t n_slots);
int32_t picles_store_push(picles_ctx *ctx);
int32_t picles_store_pop(picles_ctx *ctx, double *state, double *time);
int32_t picles_store_pending(const picles_ctx *ctx);

/* ---- coarse wave diagnostics: Hs / Tp / group velocity planes and global sums, reduced on the device ----------------------
 * What the reference's users derive from State on the host afterwards — Hs = 4 sqrt(e) (visualization/movie_2D.jl:49,162), the
 * group-velocity vector of GetGroupVelocity (Operators/core_2D.jl:138-147) and PartitionOutput
 * (examples/example_00_minimal_state_vector.jl:21-57), the peak frequency of c_g_conversions_vector (particle_waves_v5.jl:281-291),
 * mean_of_state / max_energy / max_cgx / max_cgy (Operators/TimeSteppers.jl:15-29) — formed where the data is: one kernel pass
 * over State writes coarsened float32 planes and one partial of seven doubles per tile, and a snapshot ring like the State ring
 * carries them to the host while the next steps run.
 *
 * THE DEFINITION (this text is the contract; tests restate it in NumPy).
 * Coarsening factors cx, cy, each 1 ... 16.  Coarse cell (I, J) covers the nodes i in [I cx, min((I+1) cx, Nx)),
 * j in [J cy, min((J+1) cy, Ny)) in GLOBAL indices: Nxc = ceil(Nx / cx), Nyc = ceil(Ny / cy); tail cells are partial.  A context
 * holds the coarse rows of its own node rows, nyc_loc = ceil((j_end - j_begin) / cy), and needs j_begin % cy == 0.
 * A node is WET when e, m_x, m_y are finite, e > 0 and m2 = m_x m_x + m_y m_y > 0 (land and switched-off nodes hold zeros);
 * this is read from State alone, not from the mask.
 * Per coarse cell, in fp64, over the wet nodes in the fixed order j outer, i inner, every sum starting from +0.0:
 *     n = count,  E = (Σ e) / n,  MX = (Σ m_x) / n,  MY = (Σ m_y) / n,  M2 = MX MX + MY MY
 * (the conserved quantities are averaged; the derived ones follow from the averages).  The cell is VALID when n > 0 and M2 > 0.
 * With g, r_g of the context's picles_phys, every operation one correctly rounded IEEE operation in the order written (no
 * contraction into fused multiply-adds):
 *     hs   = 4.0 * sqrt(E)
 *     cg_x = (MX * E) / (2.0 * M2)          cg_y = (MY * E) / (2.0 * M2)
 *     cbar = E / (2.0 * sqrt(M2))
 *     tp   = (FOUR_PI * fmax(cbar / r_g, 0.1)) / g          FOUR_PI = 12.566370614359172 (4 M_PI as a double)
 * (The reference forms m_amp = sqrt(m2) and squares it again; here M2 is used directly.  The planes are therefore NOT
 * bit-compatible with the Julia expressions, and do not need to be: they agree to rounding.)
 * Each field selected in the bit mask is one plane of Nxc x nyc_loc float32 — the fp64 value rounded to nearest even —
 * column-major [I + Nxc J], planes in ascending bit order; a cell that is not valid holds a quiet NaN in every plane.
 *
 * Scalars, per TILE: a tile is PICLES_DIAG_TILE = 256 consecutive coarse columns I in [256 T, 256 T + 256) of one coarse row J;
 * tiles_per_row = ceil(Nxc / 256), n_partials = nyc_loc * tiles_per_row, partial index = J_loc * tiles_per_row + T.  A partial is
 * seven doubles: [sum_e, sum_mx, sum_my, n_wet, max_e, max_mx, max_my].  Lane l = 0 ... 255 of a tile holds the cell
 * I = 256 T + l: its Σ e, Σ m_x, Σ m_y and n as above (before the division; +0.0 where I >= Nxc) and the maxima of the three planes
 * over ALL nodes of the cell, wet or not (fmax from -inf: a NaN is skipped; -inf where I >= Nxc).  The reduction tree, the same
 * for the four sums with + and the three maxima with fmax:
 *     inside each group of 64 lanes w = 0 ... 3 (lanes 64 w ... 64 w + 63), for s = 32, 16, 8, 4, 2, 1:  v[l] = v[l] + v[l + s]
 *     for l < s (l counted inside the group);  the tile's value is ((v0 + v1) + v2) + v3 of the four groups' v[0].
 * A maximum that is a zero is stored as +0.0 (x + 0.0 is applied to the three maxima of the partial).  The host combines the
 * partials sequentially in ascending (J, T) order from +0.0 / -inf; over several slabs in rank order, J ascending — a slab whose
 * j_begin is a multiple of cy produces exactly the tiles of the whole grid, so the totals are the same bit for bit whatever the
 * decomposition, and no floating-point atomic is involved.  mean_of_state = sum_e / (Nx Ny) (TimeSteppers.jl:15-19).
 *
 *   init:    refuses factors outside 1..16, an empty or unknown field mask, n_slots < 1, a second init, a slab with j_begin % cy != 0
 *   shape:   coarse shape, number of selected planes and partials, bytes of the field block (4 Nxc nyc_loc n_fields); no device work
 *   push:    completes a pending fused step as picles_store_push does, launches the kernel on the context stream into the slot's
 *            device buffer and starts the asynchronous copy into pinned host memory on the store stream: steps enqueued after it
 *            overlap the copy.  Refuses: not initialised, ring full
 *   pop:     waits for the OLDEST snapshot: fields (bytes of picles_diag_shape; float32 planes), partials (n_partials * 7 doubles,
 *            may be NULL), its model time (may be NULL).  Refuses: none pending
 *   pending: snapshots pushed and not yet popped
 * picles_destroy frees the ring; picles_checkpoint_load / begin treat a diagnostics snapshot in flight like a store snapshot. */
#define PICLES_DIAG_HS    1
#define PICLES_DIAG_TP    2
#define PICLES_DIAG_CG_X  4
#define PICLES_DIAG_CG_Y  8
#define PICLES_DIAG_E    16
#define PICLES_DIAG_MX   32
#define PICLES_DIAG_MY   64
#define PICLES_DIAG_ALL 127
#define PICLES_DIAG_TILE 256
int32_t picles_diag_init(picles_ctx *ctx, int32_t cx, int32_t cy, int32_t field_mask, int32_t n_slots);
int32_t picles_diag_shape(const picles_ctx *ctx, int32_t *nxc, int32_t *nyc_loc, int32_t *n_fields, int32_t *n_partials, size_t *bytes);
int32_t picles_diag_push(picles_ctx *ctx);
int32_t picles_diag_pop(picles_ctx *ctx, void *fields, double *partials, double *time);
int32_t picles_diag_pending(const picles_ctx *ctx);
/* export: what push does up to the kernel launch — a pending fused step is completed on the context stream — with the kernel writing
 * into the CALLER's device buffers: fields_dev (bytes of picles_diag_shape) and partials_dev (n_partials * 7 doubles; may be NULL), the
 * layout of pop.  No ring slot, no copy to the host; an event recorded behind the kernel is waited for by caller_stream (NULL: the
 * caller orders itself, e.g. picles_sync).  The same bits as push + pop.  Refuses: not initialised, fields_dev NULL */
int32_t picles_diag_export(picles_ctx *ctx, void *fields_dev, double *partials_dev, void *caller_stream);

/* ---- coupling fluxes: wind input, dissipation, wave-supported stress and Stokes drift planes (ABI 19) ------------------------
 * What the partner models of a coupled system consume.  The atmosphere: the momentum the waves take out of the wind (the
 * wave-supported stress, WAVEWATCH III's taw).  The ocean: the momentum and energy the breaking waves hand down (two, phioc) and the
 * surface Stokes drift (uss).  The model evaluates the terms behind them at every Runge-Kutta stage — Ĩ = C_e α² H_β, the wind
 * input, and D̃ = eⁿ (k_p/e_T)²ⁿ, the dissipation (particle_waves_v5.jl:317-335) — and fuses them into d ln e/dt; here they are
 * formed apart, once, from State and the wind at the clock, coarsened and reduced on the device like the diagnostics above.
 * The set is NOT part of the PICLES_DIAG_* mask, and no part of the checkpoint blob.  It only reads: a push or export leaves State,
 * particles, counters and the restart blob as a flush alone would.  Works on slabs, spheres and nests.
 *
 * THE NODE (picles_amd/csrc/k_flux.h states the arithmetic operation by operation; the tests build that header for the host).
 * A node is ACTIVE when e, m_x, m_y are finite, e >= minimal_state[0] and m_x m_x + m_y m_y >= minimal_state[1] (NodeToParticle!'s
 * branch A).  It becomes a particle (ln e, c̄ = m e / (2 |m|²)), and under the wind (u, v) the general form of the right-hand side
 * gives ω_p, k_p (with their speed floors), Ĩ (α <= 500; 0 for a vanishing wind), D̃ (n = 2 and general n) and ω_p r_g S_cg, with the
 * physics switches honoured: a switched-off term is an exact +0.0.  With d = c̄ / |c̄|, nine values per node:
 *     phi_in    = e ω_p Ĩ               energy (variance) input from the wind [m² s⁻¹]
 *     phi_dis   = e ω_p D̃               dissipation
 *     phi_shift = e ω_p r_g S_cg        the peak-downshift term of the energy equation
 *     tq_in     = ω_p phi_in d          momentum from air to waves (x, y)      (deep water: c_p = g/ω_p, τ = ρ_w g φ / c_p = ρ_w ω_p φ)
 *     tq_dis    = ω_p phi_dis d         momentum from waves to ocean (x, y)
 *     us        = 2 e ω_p k_p d         surface Stokes drift of the peak wave [m s⁻¹] (x, y)
 * phi_in - phi_dis + phi_shift = e d(ln e)/dt of the right-hand side, to rounding.  An active node one of whose nine values is not
 * finite is BAD.  A node that is not active, or bad, contributes zero to everything; bad nodes are counted apart.
 *
 * PLANES.  Coarse cells, tiles and layout are those of picles_diag_* (cx, cy in 1 ... 16, global cells, j_begin % cy == 0, planes of
 * Nxc x nyc_loc float32, column-major [I + Nxc J], selected planes in ascending bit order).  A cell's value is the AREA mean: the sum
 * over its active nodes in the order j outer, i inner from +0.0, divided by the number of nodes the cell covers (cx cy, fewer in a
 * ragged last cell) — land and calm nodes count as zero; the partner model applies its own sea fraction — then multiplied by the
 * set's scale as the last fp64 operation (scale_phi for the three phi planes, scale_tau for the four tq planes, 1 for us) and
 * rounded to float32, nearest even.  A cell without an active node holds +0.0, never a NaN (a node's non-finite values do not reach
 * a sum: the node is BAD; a finite mean beyond the float32 range rounds to ±inf).  scale_phi = ρ_w g gives W m⁻², scale_tau = ρ_w N m⁻².
 * PARTIALS.  Eleven doubles per tile: the nine UNSCALED sums of the tile's cells (before the division), n_active, n_bad, each reduced
 * by the tree of the diagnostics' sums; the host combines them in ascending (J, T) order from +0.0, over slabs in rank order.
 *
 * THE WIND AT THE CLOCK.  The kernel reads a level plane the wind window holds at the clock; nothing is interpolated.  A static
 * window: its level.  A clock equal to the window's start: level 0.  A clock equal to the window's end — the time the (u1, v1)
 * planes hold, which is where every model step leaves the clock; for a knot or polyline window its end level — those planes as they
 * stand.  Under host-set levels (picles_set_winds*) any other clock is refused (-2) with a text that names the remedy — step to a
 * level, or set the window — before anything is launched: a pending fused step stays pending.  A lattice or streamed context
 * (picles_set_wind_grid, picles_wind_stream_*) reads the planes its last step or seed sampled where they hold the clock's level, and
 * otherwise — a clock between levels; after picles_set_wind_grid*, picles_nest_relocate, picles_checkpoint_load — samples the level at
 * the clock with the sampler of its windows (a function of the time alone) into a spare pair of planes, made on first use; a wind
 * stream that does not hold the level(s) bracketing the clock refuses (-2, naming the level to push).
 *
 *   init:    refuses (-2, context unchanged) factors outside 1..16, an empty or unknown mask, scales that are not finite and positive,
 *            n_slots < 1, a second init, a slab with j_begin % cy != 0
 *   shape:   coarse shape, number of selected planes and partials, bytes of the field block (4 Nxc nyc_loc n_fields); no device work
 *   push:    completes a pending fused step as picles_diag_push does, launches the kernel on the context stream into the slot's device
 *            buffer and starts the asynchronous copy into pinned host memory on the store stream (the ring of §15 that snapshots,
 *            diagnostics and probes share).  Refuses: not initialised, ring full (-3), the wind rule
 *   pop:     waits for the OLDEST snapshot: fields (bytes of picles_flux_shape), partials (n_partials * 11 doubles, may be NULL), its
 *            model time (may be NULL).  Refuses: none pending (-3)
 *   pending: snapshots pushed and not yet popped
 *   export:  what push does up to the kernel launch, with the kernel writing into the CALLER's device buffers (fields_dev; partials_dev
 *            may be NULL), the layout of pop; an event recorded behind the kernel is waited for by caller_stream (NULL: the caller
 *            orders itself).  The same bits as push + pop.  Refuses: not initialised, fields_dev NULL, the wind rule
 *   free:    drops the set with whatever is pending; init may follow.  picles_destroy frees it too; picles_checkpoint_load treats a
 *            flux snapshot in flight like a store snapshot */
#define PICLES_FLUX_PHI_IN     1
#define PICLES_FLUX_PHI_DIS    2
#define PICLES_FLUX_PHI_SHIFT  4
#define PICLES_FLUX_TQ_IN_X    8
#define PICLES_FLUX_TQ_IN_Y   16
#define PICLES_FLUX_TQ_DIS_X  32
#define PICLES_FLUX_TQ_DIS_Y  64
#define PICLES_FLUX_US_X     128
#define PICLES_FLUX_US_Y     256
#define PICLES_FLUX_ALL      511
#define PICLES_FLUX_NPARTIAL  11
int32_t picles_flux_init(picles_ctx *ctx, int32_t cx, int32_t cy, int32_t field_mask, double scale_phi, double scale_tau, int32_t n_slots);
int32_t picles_flux_shape(const picles_ctx *ctx, int32_t *nxc, int32_t *nyc_loc, int32_t *n_fields, int32_t *n_partials, size_t *bytes);
int32_t picles_flux_push(picles_ctx *ctx);
int32_t picles_flux_pop(picles_ctx *ctx, void *fields, double *partials, double *time);
int32_t picles_flux_pending(const picles_ctx *ctx);
int32_t picles_flux_export(picles_ctx *ctx, void *fields_dev, double *partials_dev, void *caller_stream);
int32_t picles_flux_free(picles_ctx *ctx);

/* ---- flux means: the coupling fluxes accumulated behind every step and exported as interval means (ABI 20) ---------------------
 * A coupler does not exchange snapshots: the wave model takes several steps per coupling interval, and what the partners must
 * receive is the momentum and energy that crossed the surface over the interval — the time mean of the fluxes over the wave steps
 * in it (WAVEWATCH III and the couplers built on OASIS or ESMF exchange interval means for this reason).  A context that holds a flux
 * set (picles_flux_init) may also hold ONE mean set; it takes its coarse cells, its mask and its scales from the flux set.
 *
 * STORAGE.  Eleven fp64 accumulator planes of Nxc x nyc_loc, column-major [I + Nxc J] like the flux planes, all zero at init: the
 * nine sums in PICLES_FLUX_* bit order — always all nine: the mask selects only at export — then n_active and n_bad, which are
 * counts.  88 B per coarse cell.  The host side keeps n_samples, t_first and t_last, as the statistics set does.
 *
 * ONE UPDATE, at a moment when the clock is t:
 *   1. every node gets the State value picles_get_state would return for it at that moment, bit for bit: with a fused step pending
 *      from its scatter records, by the pull the scatter would run (as the statistics set and the station probes do); otherwise
 *      from State in memory;
 *   2. the wind is THE WIND AT THE CLOCK of the flux set (above), with its refusals, which come before anything is launched;
 *   3. per coarse cell the eleven cell sums S_q are those of the flux kernel: the node arithmetic of k_flux.h per node, the nodes
 *      visited j outer, i inner, from +0.0; active nodes add their nine values and count into n_active, bad nodes into n_bad;
 *   4. acc_q = acc_q + S_q, one fp64 addition per plane and cell; n_samples goes up by one, t_last = t (and t_first = t at the
 *      first sample).
 * An update does not complete a pending fused step and does not synchronise the host; it leaves State, particles, counters, reach
 * counters, dispatch order, clock and the restart blob untouched.  Samples carry EQUAL weight: a caller who changes Δt inside an
 * interval should export before the change.
 *
 * AUTOMATIC UPDATES.  picles_time_step, picles_run_steps and picles_slab_run_steps update behind every model step they complete for
 * which s >= first and (s - first) % every == 0, s counting the steps completed since picles_flux_mean_init: the schedule, the
 * places and the stream ordering of the statistics set (in the native ring: the probe stream).  The split-phase calls count steps
 * and do not update: their caller calls picles_flux_mean_update(ctx, stream) behind the scatter of the step.  Operations on the
 * accumulators are ordered behind each other whatever streams they use.  An automatic update runs BEHIND its step: where the wind rule
 * refuses it — only a host-set window that does not end where the step ends can: a static window, a window over [t, t + dt], a
 * lattice and a stream always hold or sample the level — the call returns -2 with the step taken, the clock advanced and no
 * sample counted (in picles_run_steps and picles_slab_run_steps: at that step, the steps before it taken and sampled); the text
 * names the remedy, and the caller may set the window and call picles_flux_mean_update for the sample that is missing.
 *
 * THE MEAN needs n = n_samples >= 1.  For a selected plane q a cell holds
 *     plane_q = (float)((acc_q / (n_cover * n)) * scale_q)
 * n_cover the nodes the cell covers; the product n_cover * n formed in fp64 (exact), then one division; the scale the last fp64
 * operation; rounded to float32, nearest even.  scale_q and the selection of planes are the flux set's.  The tile partials of a mean
 * are eleven doubles per tile of 256 coarse columns: each accumulator plane reduced by the tree of the flux partials, unscaled and
 * undivided; the host divides by n.
 *
 *   init:    refuses (-2, context unchanged): no flux set, every < 1, first < 1, a second init
 *   shape:   every, the number of accumulator planes (11), their bytes; -1 without a set; no device work
 *   update:  one update now, on `stream` (NULL: the context stream).  Refuses: no set; the wind rule
 *   push:    the finalising kernel writes fields and partials into the next slot of the FLUX SET's ring, in the slot layout of
 *            picles_flux_push; picles_flux_pop / picles_flux_pending serve it; the slot's time is the clock.  With reset != 0 the
 *            accumulators and the three scalars go to zero in stream order behind it.  A pending step stays pending.  Refuses: no
 *            set, ring full (-3), n_samples == 0 (-2)
 *   export:  the same into the CALLER's device buffers (partials_dev may be NULL), ordered like picles_flux_export
 *   get:     the raw accumulators (11 planes of Nxc nyc_loc doubles) and the three scalars; waits for the latest operation on the
 *            accumulators only, through an event: a pending step stays pending.  planes may be NULL: the scalars alone, which the
 *            host keeps — no device work
 *   set:     the raw accumulators in, behind the updates already issued: how a picked-up run continues an open interval
 *            (picles_checkpoint_load leaves the accumulators as they are: they are no part of the blob)
 *   reset:   accumulators and scalars to zero, in stream order; s goes on
 *   free:    drops the mean set.  picles_flux_free and picles_destroy drop it with the flux set.  picles_nest_relocate on a context
 *            whose mean set holds samples refuses (-2): push or reset first — the cells would mean another place after the move */
int32_t picles_flux_mean_init(picles_ctx *ctx, int32_t every, int32_t first);
int32_t picles_flux_mean_shape(const picles_ctx *ctx, int32_t *every, int32_t *n_planes, size_t *bytes);
int32_t picles_flux_mean_update(picles_ctx *ctx, void *stream);
int32_t picles_flux_mean_push(picles_ctx *ctx, int32_t reset);
int32_t picles_flux_mean_export(picles_ctx *ctx, void *fields_dev, double *partials_dev, void *caller_stream, int32_t reset);
int32_t picles_flux_mean_get(picles_ctx *ctx, double *planes, int64_t *n_samples, double *t_first, double *t_last);
int32_t picles_flux_mean_set(picles_ctx *ctx, const double *planes, int64_t n_samples, double t_first, double t_last);
int32_t picles_flux_mean_reset(picles_ctx *ctx);
int32_t picles_flux_mean_free(picles_ctx *ctx);

/* ---- station probes: the State value of chosen nodes after every step, with the fused path kept --------------------------------
 * Point output — the series of the sea state at buoys, platforms, validation points — is what the reference's scripts cut out of
 * full cash_store snapshots (State[i, j, :] against time: tests/T04_2D_reg_test.jl and the B0x regressions).  Here a few thousand
 * nodes are sampled on the device behind each step and carried to the host by a ring like the two above.
 *
 * THE CONTRACT (tests restate it).
 * A context holds at most one probe set: n >= 1 nodes given by GLOBAL 0-based indices (i, j), 0 <= i < Nx and j_begin <= j < j_end
 * (the context's own rows), as two planes ij[0 .. n) = i, ij[n .. 2n) = j like picles_scatter_particles.  Duplicates, land nodes
 * and nodes on the grid's boundary are allowed.
 * A SAMPLE is, for every node of the set in the order given, the three doubles (e, m_x, m_y) picles_get_state would return for
 * that node if it were called at that moment — bit for bit — laid out as 3 planes of n doubles, [k][node], k = e, m_x, m_y.
 * Taking a sample does NOT complete a pending fused step, does not synchronise the host, and leaves State, particles, counters,
 * reach counters, dispatch order and clock untouched.  With a fused step pending the values are formed from that step's scatter
 * records by the pull k_scatter would run for the node; otherwise (freshly seeded, after a step of the plain phases, after
 * PICLES_STEP_MOVIE — then zeros, as picles_get_state shows —, PICLES_STEP_ATOMIC, picles_set_state, a checkpoint load) they
 * are read from State.  A sample carries the model clock and s, the number of model steps the context has completed since
 * picles_probe_init (a step completes in picles_end_fused_step or picles_scatter_remesh, whoever calls them).
 *
 * AUTOMATIC SAMPLING: picles_time_step, picles_run_steps and picles_slab_run_steps take a sample after every model step they
 * complete (fused or plain, any flags) for which s >= first and (s - first) % every == 0; every >= 1, first >= 1 (a run picked up
 * from a checkpoint continues the cadence of the run that wrote it through `first`).  The split-phase calls (picles_begin_step /
 * advance_rows / scatter_remesh, picles_begin_fused_step / step_rows / end_fused_step) count steps and do not sample: their
 * caller calls picles_probe_sample once the step's halo exchange has been delivered.
 *
 * RING: capacity samples in device memory and as many in pinned host memory; each sample is copied out asynchronously on the store
 * stream behind an event, and the steps enqueued after it overlap the copy.  When a sample is due and capacity samples are
 * un-popped, the step entry point refuses with PICLES_PROBE_E_FULL before it has changed anything (clock, particles and records
 * as they were; the same call succeeds after a pop); picles_run_steps / picles_slab_run_steps (n) refuse up front when the n steps
 * would overrun the ring, not half-way.  Nothing is dropped silently.
 *
 *   init:    refuses (context unchanged, picles_last_error set) n < 1, a node outside [0, Nx) x [j_begin, j_end), every < 1,
 *            first < 1, capacity < 1, a second init without picles_probe_free
 *   sample:  one sample now, on `stream` (NULL: the context stream) — the stream behind which the caller has ordered everything
 *            the sample depends on: the seeded state, or the launches and the delivered halo of a split-phase step.
 *            Refuses: no set, ring full (PICLES_PROBE_E_FULL)
 *   pop:     waits for the OLDEST samples only and hands out min(max_samples, pending) of them, oldest first: values
 *            (3 n doubles each), times and steps (one each; may be NULL), *n_out = their number.  Refuses: no set,
 *            max_samples < 1, none pending (-3, as the other rings)
 *   pending: samples taken and not yet popped;  shape: n, every, capacity (-1 without a set; no device work)
 *   free:    drops the set — samples pending with it — so that a new one may be created; picles_destroy does it too
 * picles_checkpoint_load with samples pending is PICLES_CKPT_E_BUSY; the probe set is no part of the blob or its fingerprint. */
#define PICLES_PROBE_E_FULL -30
int32_t picles_probe_init(picles_ctx *ctx, int32_t n, const int32_t *ij, int32_t every, int32_t first, int32_t capacity);
int32_t picles_probe_sample(picles_ctx *ctx, void *stream);
int32_t picles_probe_pop(picles_ctx *ctx, int32_t max_samples, double *values, double *times, int64_t *steps, int32_t *n_out);
int32_t picles_probe_pending(const picles_ctx *ctx);
int32_t picles_probe_shape(const picles_ctx *ctx, int32_t *n, int32_t *every, int32_t *capacity);
int32_t picles_probe_free(picles_ctx *ctx);

/* ---- run statistics: storm-peak, mean and exceedance maps of every node, kept on the device, with the fused path kept -------------
 * What a hindcast reports per node over a run — the maximum significant wave height and when it occurred, period and direction at
 * that peak, mean Hs, mean direction, the share of time above a height threshold — needs State at EVERY step.  Here every node is
 * sampled on the device behind each step, as the station probes sample a few, and folded into per-node accumulators that stay in
 * device memory: State never crosses PCIe, and the host derives the reported variables from the accumulators at the end.
 *
 * THE CONTRACT (tests restate it).
 * A context holds at most one statistics set, created by picles_stat_init(ctx, group_mask, n_thresholds, thresholds, every, first).
 * A SAMPLE of a node is the three doubles (e, m_x, m_y) picles_get_state would return for it at that moment — bit for bit —, formed
 * from the scatter records of a pending fused step by the pull k_scatter would run for the node, otherwise read from State: the rule
 * of the probe contract above (freshly seeded, after a step of the plain phases, after PICLES_STEP_MOVIE — then zeros —,
 * PICLES_STEP_ATOMIC, picles_set_state, a checkpoint load: State).  A sample carries the model clock.
 * A sample is WET by the rule of picles_diag_*: e, m_x, m_y finite, e > 0 and m_x m_x + m_y m_y > 0.  A sample that is not wet
 * changes nothing at that node.
 * Per node and wet sample, in fp64, every operation one correctly rounded IEEE operation in the order written (no contraction into
 * fused multiply-adds); all accumulators start from zero:
 *   always               n_wet (uint32 plane) is incremented (it wraps at 2^32)
 *   PICLES_STAT_PEAK     planes e_peak, mx_peak, my_peak, t_peak (fp64): if this is the node's first wet sample (n_wet was 0) or
 *                        e > e_peak, all four are replaced by e, m_x, m_y and the sample's clock.  The comparison is strict: the
 *                        first of equal maxima is kept
 *   PICLES_STAT_MEAN     planes sum_e, sum_mx, sum_my, sum_hs (fp64): each  sum = sum + x,  with  hs = 4.0 * sqrt(e)
 *   PICLES_STAT_EXCEED   n_thresholds in 1 ... 4 Hs thresholds, finite, positive, strictly ascending: one uint32 plane n_exc[k] per
 *                        threshold, incremented when hs >= thr[k], hs as above
 * The context also keeps, on the host, n_samples (updates since init / reset, wet or not) and the clocks of the first and the last
 * of them (0.0 while there is none).
 * Planes are column-major [i + Nx * jl] over the context's own rows, like State: per-node accumulators do not depend on the slab
 * decomposition, and the planes of the whole grid are the slabs' planes row block after row block.
 * THE PLANE BLOCK of get / set: the planes of the groups selected by the call's mask — a subset of the set's mask; n_wet always —
 * back to back, the fp64 planes first: [e_peak mx_peak my_peak t_peak] [sum_e sum_mx sum_my sum_hs] as doubles, then n_wet
 * [n_exc[0] ... n_exc[n_thresholds - 1]] as uint32: N (8 (4 [PEAK] + 4 [MEAN]) + 4 (1 + n_thresholds [EXCEED])) bytes, N = Nx (j_end -
 * j_begin).  That is 4 + 32 + 32 + 4 n_thresholds bytes of device memory per node for the whole set.
 *
 * AUTOMATIC UPDATES: picles_time_step, picles_run_steps and picles_slab_run_steps update after every model step they complete
 * (fused or plain, any flags) for which s >= first and (s - first) % every == 0, every >= 1, first >= 1; s counts the model steps
 * the context has completed since picles_stat_init (a step completes in picles_end_fused_step or picles_scatter_remesh, whoever
 * calls them).  The split-phase calls count steps and do not update: their caller calls picles_stat_update(ctx, stream) behind the
 * stream that orders the step's launches and its delivered halo, and keeps the launches that overwrite the record buffer two steps
 * later behind that stream.  Operations on the planes (update, reset, set) are ordered behind each other whatever streams they use.
 * An update does NOT complete a pending fused step, does not synchronise the host, and leaves State, particles, counters, reach
 * counters, dispatch order and clock untouched.
 *
 *   init:    refuses (context unchanged, picles_last_error set) an empty or unknown mask, n_thresholds outside 1 ... 4 or thresholds
 *            that break the rule with EXCEED, n_thresholds != 0 without it, every < 1, first < 1, a second init without
 *            picles_stat_free
 *   shape:   mask, n_thresholds, thresholds (room for 4), every, number of planes and bytes of the whole set's plane block (any
 *            pointer may be NULL; -1 without a set; no device work)
 *   update:  one update now, on `stream` (NULL: the context stream).  Refuses: no set
 *   get:     waits for the latest operation on the planes only — through an event, not a device synchronisation; a pending step
 *            stays pending — and copies the plane block of `group_mask` and the three scalars out (the scalar pointers may be
 *            NULL).  Refuses: no set, planes NULL, a mask that is no subset of the set's
 *   set:     uploads a plane block and the three scalars, behind the updates already issued: how a picked-up run continues.
 *            Refuses: no set, planes NULL, n_samples < 0, a mask that is no subset of the set's
 *   reset:   planes and scalars to zero, in stream order behind the updates already issued; the step count s goes on
 *   free:    drops the set so that a new one may be created; picles_destroy does it too
 * The set is no part of the checkpoint blob or its fingerprint; picles_checkpoint_load leaves it as it is. */
#define PICLES_STAT_PEAK   1
#define PICLES_STAT_MEAN   2
#define PICLES_STAT_EXCEED 4
#define PICLES_STAT_ALL    7
int32_t picles_stat_init(picles_ctx *ctx, int32_t group_mask, int32_t n_thresholds, const double *thresholds, int32_t every, int32_t first);
int32_t picles_stat_shape(const picles_ctx *ctx, int32_t *group_mask, int32_t *n_thresholds, double *thresholds, int32_t *every, int32_t *n_planes, size_t *bytes);
int32_t picles_stat_update(picles_ctx *ctx, void *stream);
int32_t picles_stat_get(picles_ctx *ctx, int32_t group_mask, void *planes, int64_t *n_samples, double *t_first, double *t_last);
int32_t picles_stat_set(picles_ctx *ctx, int32_t group_mask, const void *planes, int64_t n_samples, double t_first, double t_last);
int32_t picles_stat_reset(picles_ctx *ctx);
int32_t picles_stat_free(picles_ctx *ctx);

/* ---- open-boundary forcing: prescribed sea state at the rim (swell from a parent model, a storm outside the box, a buoy
 * spectrum at the mouth of a basin).  No counterpart in the reference: its `boundary_defaults` is a constant and its rim nodes are
 * as dead as this library's are without a set. ----
 * THE NODES.  On a model without periodic_boundary the grid-boundary nodes (mask class 3) carry no particle: energy that reaches
 * them is dropped and nothing enters.  A forcing set names n of them, ij = the i plane then the j plane (global, 0-based), each
 * once.  At every such node and every model step a particle is BORN from the prescribed (e, m_x, m_y) at the step's start time t
 * (the model clock before the tick, the time the remesh uses), advanced over the step with the model's solver under the node's
 * wind, and scattered with all other particles; it is reborn the next step, so a forced node carries nothing from step to step.
 * THE VALUE.  Levels are 3 planes of n doubles (e, then m_x, then m_y, node k of the list at [k]).  One level (v1 == NULL): v = v0.
 * Two levels at t0 < t1: per component, each operation one IEEE operation,
 *     s = (t - t0) / (t1 - t0);    v = v0 + s * (v1 - v0)
 * THE BIRTH.  If e, m_x, m_y are finite, e >= minimal_state[0] and m_x² + m_y² >= minimal_state[1] (NodeToParticle!'s test of a
 * node value): lne = log e, c̄ = m e / (2 |m|²), x = y = 0, with the step-size memory of a freshly seeded particle — every step,
 * so the result does not depend on how the model got here.  Otherwise no particle is born at that node this step (on = 0, an
 * empty scatter record); nothing is re-seeded from the wind there.  The guards of the advance (NaN / Inf re-seed, energy cap,
 * maxiters, reach cap) treat and count a forced particle like any other; picles_get_particles shows it at its node.
 * WHERE IT RUNS.  One small kernel behind the launch that writes a step's records, on its stream, in picles_time_step,
 * picles_run_steps and picles_advance alike: fused steps stay fused, and probes, statistics, snapshots and checkpoints taken
 * behind a step see its forced particles.  The sum order of the scatter is the plain column-major one over all records (a forced
 * record is on the ocean list: there is no second list).
 * THE WINDOW.  With two levels every step must START inside [t0, t1] (an end is met within 1e-9 of t1 - t0, the rule of
 * picles_lattice_knots).  picles_run_steps checks all n start times before it enqueues anything; picles_time_step, picles_advance
 * and picles_begin_fused_step check theirs.  A refused call has changed nothing: set the next pair and call again.
 *
 *   init:       refuses (context unchanged, picles_last_error set) n < 1, a node outside the grid, a node that is not mask class 3,
 *               a node given twice, a model with periodic_boundary (its rim is stepped), a tripolar grid, a slab context, slab
 *               mode or a native ring, a second init without picles_bforce_free.  The set has no levels yet: steps are refused
 *               until picles_bforce_set_levels
 *   set_levels: uploads one or two levels in stream order behind the steps already enqueued (they keep the levels they were
 *               enqueued under; a pending fused step stays pending); the caller's arrays are free on return.  Refuses: no set,
 *               v0 NULL, two levels without finite t0 < t1
 *   info:       n, levels held (0, 1 or 2), t0, t1 (any pointer may be NULL; -1 without a set; no device work)
 *   free:       completes a pending step, empties the forced nodes' scatter records, switches their particles off (on = 0,
 *               status = 0: what a rim node shows without a set) and drops the set; picles_destroy drops it too
 * SLABS ARE OUT OF SCOPE: the edge rows' records are exchanged before a kernel behind the launch could run.  With a set,
 * picles_set_slab_mode, picles_slab_comm_init / _run_steps / _exchange and picles_begin_step fail (-5) and change nothing;
 * picles_bforce_init fails likewise on a slab.  A picles_advance_rows / picles_step_rows of less than all rows fails (-5) and
 * launches nothing; a step that picles_begin_fused_step had opened on a whole-grid context stays open, and picles_step_rows of
 * all rows followed by picles_end_fused_step completes it.
 * The set is no part of the checkpoint blob or its fingerprint (a forced particle carries nothing across a step boundary);
 * picles_checkpoint_load leaves it as it is, and the host sets the levels that bracket the restored clock. */
int32_t picles_bforce_init(picles_ctx *ctx, int32_t n, const int32_t *ij);
int32_t picles_bforce_set_levels(picles_ctx *ctx, double t0, const double *v0, double t1, const double *v1);
int32_t picles_bforce_info(const picles_ctx *ctx, int32_t *n, int32_t *levels, double *t0, double *t1);
int32_t picles_bforce_free(picles_ctx *ctx);
/* the level planes as the device holds them, 3 planes of n doubles each (NULL skips one; asking for a level the set does not hold
 * fails, -2).  Stream-ordered behind whatever wrote them — an upload, or a parent's nest sample —; completes no pending step. */
int32_t picles_bforce_get_levels(picles_ctx *ctx, double *v0, double *v1);
/* ---- forcing bands (ABI 12): a set that also holds OCEAN nodes, with an optional blend weight per node.  Sea that
 * travels more than one cell a step crosses a forced rim column between two levels and never enters; a band as deep as the swell
 * travels closes that hole, and a weight that falls off inward makes the band a relaxation zone.
 *   init_band:  ij as for picles_bforce_init; nodes of mask class 3 and of class 1 (ocean).  weight: NULL (every node 1.0) or n
 *               doubles.  Refuses everything picles_bforce_init refuses, a node of class 0 or 2, and a weight that is not finite or
 *               not in (0, 1].  picles_bforce_set_levels / _get_levels / _info / _free, the window rule and picles_nest_* work on
 *               either kind of set; picles_bforce_init itself still refuses a class-1 node.
 * A FORCED OCEAN NODE IS NOT STEPPED while the set lives: init clears its "stepped" flag in stream order behind whatever is enqueued
 * (a pending fused step stays pending; the records it left at these nodes are pulled by the next step).  From then on the node is
 * what a forced rim node is: no step kernel touches its particle slot or writes its record, k_bforce bears its particle and writes
 * its record every step (the empty one where the value is refused), it takes no wind re-seed, and the counters count it once.
 * picles_bforce_free restores the flags from the mask and the model; the next remesh seeds the nodes like any other.
 * CHECKPOINTS.  The flags plane is a segment of the blob, but picles_checkpoint_load leaves a context with ITS OWN flags — the home
 * flags with the set that lives in it applied, whatever the blob carried: a blob written under a band set and loaded into a context
 * without one steps the band nodes again.  The fingerprint does not depend on the set.
 * THE BLEND.  With p the prescribed value after the time interpolation above, m the model's State at the node at the step's start
 * (what picles_probe_sample gives for that node: from the records of a pending fused step, or from State in memory) and w the
 * node's weight, per component, each operation one IEEE operation,
 *     v = m + w * (p - m)
 * and THE BIRTH test is made on v.  A node with w == 1.0 reads no State: v is p to the bit, and a set without a weight below 1
 * runs the kernels of an unweighted set. */
int32_t picles_bforce_init_band(picles_ctx *ctx, int32_t n, const int32_t *ij, const double *weight);

/* ---- one-way nesting: a child box forced by its parent, all on the device.  The forcing set of `child` (picles_bforce_init) takes
 * its time levels from the State of `parent`, another whole-grid context on the same device, instead of from the host: the parent
 * is sampled behind its step, the sample is mixed onto the child's forced nodes and written into the child's level block in stream
 * order.  State never leaves the device, the host waits for nothing, and both contexts stay on the fused path. ----
 * THE GEOMETRY is the host's: n_corner distinct parent nodes, corner_ij = their i plane then their j plane (0-based, in the parent);
 * per forced child node k, in the order of the child's set, four corners index[c n + k] into that list with the weights
 * weight[c n + k], c = 0..3 (n = the set's node count).  The library uses them as given: no coordinate arithmetic on the device.
 * A SAMPLE (picles_nest_sample) takes one time level at the parent's clock as it stands now: the State of the corner nodes — from
 * the records of the parent's pending fused step where one is pending (it stays pending), from State in memory otherwise: the
 * choice of picles_probe_sample — and per child node, every operation one IEEE operation in the order written:
 *     a corner is WET when e, m_x, m_y are finite, e > 0 and m_x*m_x + m_y*m_y > 0
 *     W = SE = SX = SY = +0.0;  for c = 0..3, if corner c is wet:  W = W + w;  SE = SE + w*e;  SX = SX + w*m_x;  SY = SY + w*m_y
 *     E = SE / W;  MX = SX / W;  MY = SY / W;  M2 = MX*MX + MY*MY
 *     the node is VALID when W > 0 and M2 > 0: its level is (E, MX, MY); otherwise NaN in all three
 * (the station definition of picles_amd/station_output.py).  A NaN level is what THE BIRTH above refuses: that node bears no
 * particle while either level of the pair is NaN.
 * THE LEVELS.  The first sample after picles_nest_init is level 0 alone (levels = 1: constant, t0 = t1 = the parent's clock); the
 * second becomes level 1; every later one rotates: level 1 becomes level 0, t0 <- t1, and the new level 1 is the parent's State at
 * the parent's clock t1.  THE WINDOW rule above holds unchanged: the child steps inside [t0, t1], then the parent is stepped and
 * sampled.  Steps of the child already enqueued keep the pair they were enqueued under.
 * ORDERING.  picles_nest_sample returns after enqueueing: no synchronisation, no copy to the host.  Its two kernels run on the
 * parent's stream behind whatever wrote the parent's records; the child's next launch that reads the levels waits for an event
 * behind them, and they wait for an event behind the child's last launch that read the slot they overwrite (three slots rotate by
 * pointer, so that launch lies a whole window back: the parent's step kernels never wait for the child's current steps).
 *
 *   init:    refuses (-2 / -5, both contexts unchanged and usable, picles_last_error(child) names the remedy) child == parent,
 *            contexts on different devices, either context a slab, in slab mode or on a native ring, either context that has run
 *            on caller-provided streams, a child without a boundary forcing set, n_corner < 1, an index outside [0, n_corner), a
 *            corner outside the parent's grid, a weight that is not finite, a second init on the same child.  The arrays are free
 *            on return.  The set has no levels afterwards (levels uploaded before are dropped): steps of the child are refused
 *            until the first sample
 *   sample:  refuses (-2, nothing changed) a child without a nest, a nest whose parent was destroyed, and a call while the
 *            parent's clock has not moved past t1
 *   info:    n_corner and the samples taken so far (either pointer may be NULL; -1 without a nest; no device work)
 *   free:    drops the nest; the set keeps the level pair it holds and takes uploads again (picles_bforce_set_levels)
 * With a nest, picles_bforce_set_levels is refused (-2: the levels come from the parent; picles_nest_free first).
 * picles_bforce_free and picles_destroy on a nested child release the nest first.  picles_destroy(parent) detaches its children:
 * each keeps its set and its last levels and goes on stepping under them; a later picles_nest_sample on it fails with a text.
 * A parent may serve several children.  The nest is no part of a checkpoint.
 * A NEST RESUMED (ABI 16).  The blob holds nothing of a nest, so a checkpointed PAIR is restarted from three things the
 * host kept: the child's blob, the parent's blob at the parent's clock — which is t1 of the pair the child held — and that pair
 * itself, as picles_bforce_info / picles_bforce_get_levels(child) gave it when the blobs were taken.  Load both blobs, make the
 * child's set and the nest again (picles_bforce_init[_band], picles_nest_init), and put the pair back:
 *   set_levels: v0, v1 are 3 planes of n doubles each, the layout of picles_bforce_get_levels; copied verbatim (NaN payloads
 *            survive) into the slots the pair names, in stream order on the child's stream; blocking: the buffers are free on
 *            return.  Afterwards levels = 2 over [t0, t1] and picles_nest_info reports 2 samples: the next picles_nest_sample
 *            rotates as a third sample does, and is refused until the parent's clock has moved past t1.  No seed sample and, with
 *            feedback, no seed feedback is taken: the next feedback stands in front of the next parent step, on a common clock.
 *            Refuses (-2, both contexts unchanged and usable, picles_last_error(child) has the text) a child without a nest, a
 *            nest whose parent was destroyed, a nest that has taken a sample, v0 or v1 NULL, times that are not finite or not
 *            t1 > t0, a parent whose clock is not exactly t1, and contexts that have run on caller-provided streams. */
int32_t picles_nest_init(picles_ctx *child, picles_ctx *parent, int32_t n_corner, const int32_t *corner_ij, const int32_t *index, const double *weight);
int32_t picles_nest_sample(picles_ctx *child);
int32_t picles_nest_info(const picles_ctx *child, int32_t *n_corner, int64_t *samples);
int32_t picles_nest_free(picles_ctx *child);
int32_t picles_nest_set_levels(picles_ctx *child, double t0, const double *v0, double t1, const double *v1);

/* ---- a child started from its parent (ABI 15): the State of `parent` at its clock t, prolonged onto EVERY node of `child`,
 * and the child's particles made from it — a child switched on beside a parent that has been running, instead of seeded cold at t = 0. ----
 * THE GEOMETRY is the host's and separable: per child column i the parent columns ix0[i], ix1[i] and the weight wx[i] (ncx entries, the
 * child's Nx), per child row j the parent rows iy0[j], iy1[j] and wy[j] (ncy entries) — picles_amd.station_output._axis of the child's
 * node coordinates in the parent.  A periodic parent's wrap cell is ix0 = Nx - 1, ix1 = 0.  Per child node (i, j), every operation one
 * IEEE operation in the order written:
 *     gx = 1 - wx[i];  gy = 1 - wy[j];  the corners in visiting order (ix0, iy0), (ix1, iy0), (ix0, iy1), (ix1, iy1) with the weights
 *     gx*gy, wx*gy, gx*wy, wx*wy;  over them the station definition of "one-way nesting" above: the wet test, the serial sums, E, MX, MY
 *     a VALID node's State is (E, MX, MY); any other node's is (0, 0, 0) — a calm node, whose particle the remesh makes from the local
 *     wind.  Every child node is written, whatever its mask class.
 * THE CALL, in this order: completes the parent's pending step (on the parent's stream; the host waits as picles_get_state would not:
 * nothing is copied); resets the child as picles_seed(child, t) resets it — clock t, no step pending, record buffers, reach words,
 * class map and counters zeroed, every particle seeded under the wind at t with fresh controller memory; a child under a wind lattice
 * samples the two-level window [t, t + dt] first, as picles_seed does at 0.0, a child under host-set winds keeps the window it holds
 * —; orders the child's stream behind the parent's with an event; writes the child's State (k_nest_prolong, picles_amd/csrc/k_nest.h)
 * and remeshes it (picles_remesh(child, dt): branches A-D at clock t).  It returns after enqueueing.  What the child holds afterwards
 * is, bit for bit, what picles_seed(child, t), picles_set_state(child, <the prolonged State>), picles_remesh(child, dt) leave.
 *   refuses (-2 / -5, both contexts as they were, picles_last_error(child) has the text): child == parent, different devices, either
 *   context a slab, in slab mode or on a native ring, either context that has run on caller-provided streams, dt <= 0, a table that
 *   is missing, an index outside the parent's grid, a weight that is not finite or lies outside [0, 1].  The tables are free on
 *   return; the child keeps a device copy until the next call or picles_destroy.  A forcing set or a nest of the child is not touched. */
int32_t picles_nest_prolong(picles_ctx *child, picles_ctx *parent, const int32_t *ix0, const int32_t *ix1, const double *wx,
                            const int32_t *iy0, const int32_t *iy1, const double *wy, double dt);

/* ---- a child moved across its parent (ABI 18): between two legs of a nested run the child's box is translated by
 * (si, sj) of its own nodes — a vortex-following nest —, so that new node (i, j) lies where old node (i + si, j + sj) lay.  The child
 * keeps the sea it has resolved where the old and the new box overlap and takes the parent's where the new box is freshly exposed. ----
 * THE STATE, per new node (i, j), with Ncx x Ncy the child's grid and m = keep_margin (the nodes dropped along the old box's rim and
 * band, whose State is prescribed rather than resolved):
 *     KEPT when m <= i + si < Ncx - m and m <= j + sj < Ncy - m: the bits of the child's State at old node (i + si, j + sj), as they
 *     stand — calm (0, 0, 0) nodes and NaN payloads included;
 *     any other node: picles_nest_prolong's value at (i, j) for the tables given, which are those of the NEW box in the parent
 *     (the same corners, weights, wet test, serial sums and divisions; (0, 0, 0) where no corner is wet).
 * kx ky nodes are kept, kx = max(0, Ncx - max(m, si) - max(m, -si)) and ky likewise; |si| >= Ncx - 2m keeps none, and the call is
 * picles_nest_prolong at the new place.  k_nest_relocate (picles_amd/csrc/k_nest.h) writes the result into MovieState, which
 * afterwards HOLDS THE RELOCATED STATE (picles_get_movie_state reads it; the next step with PICLES_STEP_MOVIE overwrites it).
 * THE CALL, in this order: completes the parent's pending step and the child's own, each on its own stream; orders the child's
 * stream behind the parent's with an event; launches the kernel; orders the parent's stream behind it; moves the mesh origin of a wind
 * lattice the child holds to (mesh_x0, mesh_y0) — the lattice is not uploaded again; without a lattice the two arguments are ignored —;
 * resets the child as picles_seed(child, t) resets it at its clock t (a lattice child samples the two-level window [t, t + dt] at the
 * new nodes; a child under host-set winds keeps the window it holds: upload the winds at the new nodes just before); copies the
 * relocated State into State and remeshes it (picles_remesh(child, dt)).  It returns after enqueueing.  What the child holds afterwards
 * is, bit for bit, what picles_seed(child, t), picles_set_state(child, <the relocated State>), picles_remesh(child, dt) leave on a
 * child created at the new position.  Neither clock moves.
 *   refuses (-2 / -5, both contexts as they were, picles_last_error(child) has the text): everything picles_nest_prolong refuses; a
 *   child that was never seeded; clocks of child and parent that differ; keep_margin < 0; a child that still holds a nest, a forcing
 *   set, a feedback or a statistics set (their nodes are index space and would go stale silently: end the leg first); a child with a
 *   periodic axis, with a metric set (picles_set_metric), with land nodes in its mask (class 0 or 2: the mask would travel with the
 *   box) or under a wind stream.  Probe, track and diagnostics sets sample index space and are left alone: they move with the box.
 *   Not carried across a move: statistics accumulators, a track table's geometry, the checkpoint fingerprint of the old origin (a
 *   blob written after a move is loaded by a context created at that leg's origin). */
int32_t picles_nest_relocate(picles_ctx *child, picles_ctx *parent, int32_t si, int32_t sj, int32_t keep_margin,
                             const int32_t *ix0, const int32_t *ix1, const double *wx,
                             const int32_t *iy0, const int32_t *iy1, const double *wy,
                             double dt, double mesh_x0, double mesh_y0);

/* ---- two-way nesting: the child's sea state fed back into its parent.  A nested child (picles_nest_init) may feed back: the library
 * makes a forcing set on the PARENT — its ocean nodes under the child — whose one level is the child's State restricted onto them,
 * written on the device behind the child's steps.  The set is picles_bforce_init_band's kind (its nodes leave the parent's step
 * kernels' hands and bear their particle from the level behind every parent step: THE BIRTH above), unweighted, of mask class 1
 * only, and it is allowed on a periodic_boundary parent.  No step kernel differs; both contexts stay on the fused path. ----
 * THE GEOMETRY is the host's: n_fb parent nodes fb_ij (i plane, then j plane, 0-based, each once, mask class 1); n_src distinct child
 * nodes src_ij likewise; per feedback node p a stencil of m entries, entry c at [c n_fb + p]: index into the source list and weight
 * (finite, >= 0; 0.0 marks padding, which is skipped whatever its index names; at least one entry per node is not padding).
 * A FEEDBACK (picles_nest_feedback) takes one level at the child's clock: the State of the source nodes — from the records of the
 * child's pending fused step where one is pending (it stays pending), from State in memory otherwise — and per feedback node the
 * station definition above over its m entries in order, every operation one IEEE operation:
 *     W = SE = SX = SY = +0.0;  for c = 0..m-1, if w_c != 0 and source c is wet:  W = W + w;  SE = SE + w*e;  SX = SX + w*m_x;  SY = SY + w*m_y
 *     E = SE / W;  MX = SX / W;  MY = SY / W;  valid when W > 0 and MX*MX + MY*MY > 0, otherwise NaN in all three
 * A calm or dry source counts as missing, not as zero; a NaN level bears no particle: a parent node the child sees as land or wholly
 * calm is empty in the parent for that step.
 * THE LEVEL.  The parent's set always holds one level (levels = 1, constant; t0 = t1 = the child's clock at the feedback): the next
 * parent step bears its feedback particles from it as it is.  It lives in the set's own two slots, used alternately; steps of the
 * parent already enqueued keep the slot they were enqueued under.
 * ORDERING.  picles_nest_feedback returns after enqueueing: no synchronisation, no copy to the host.  Its two kernels run on the
 * child's stream behind whatever wrote the child's records; the parent's next k_bforce (behind its step kernel, which therefore
 * still overlaps the child's steps) and picles_bforce_get_levels(parent) wait for an event behind them, and they wait for an event
 * behind the parent's last launch that read the slot they overwrite — the parent step before last.
 *
 *   init:    refuses (-2 / -5, both contexts unchanged and usable, picles_last_error(child) has the text) a child without a nest or
 *            whose parent was destroyed, a parent that holds a forcing set of its own (a context carries one set: feedback and an own
 *            forcing of the parent are not supported together), either context that has run on caller-provided streams, n_fb < 1,
 *            n_src < 1, m < 1, a source node outside the child's grid, an index outside [0, n_src), a weight that is not finite or is
 *            negative, a node whose weights are all zero, a second init, and whatever picles_bforce_init_band refuses of a set on the
 *            parent (a node off the grid or given twice, a tripolar grid, slabs, the native ring) or a node not of mask class 1.
 *            The arrays are free on return.  The parent's set has no level afterwards: its steps are refused until the first feedback
 *   feedback: refuses (-2, nothing changed) a child without feedback, a destroyed parent, and clocks of child and parent that differ
 *            by more than 1e-9 of the child's step length (before any step of the child: that differ at all)
 *   info:    the set's shape and the levels taken so far (any pointer may be NULL; -1 without feedback; no device work)
 *   free:    drops the feedback and the parent's set; the parent's nodes go back to its step kernels (picles_bforce_free's way)
 * While feedback lives, picles_bforce_set_levels(parent) is refused; picles_bforce_free(parent) drops the feedback with the set (the
 * child keeps its one-way nest); picles_nest_free, picles_bforce_free and picles_destroy on the child release the feedback first;
 * picles_destroy(parent) detaches it: a later picles_nest_feedback fails with a text.  Slab mode and the native ring stay refused
 * on both contexts.  The feedback is no part of a checkpoint. */
int32_t picles_nest_feedback_init(picles_ctx *child, int32_t n_fb, const int32_t *fb_ij, int32_t n_src, const int32_t *src_ij, int32_t m,
                                  const int32_t *index, const double *weight);
int32_t picles_nest_feedback(picles_ctx *child);
int32_t picles_nest_feedback_info(const picles_ctx *child, int32_t *n_fb, int32_t *n_src, int32_t *m, int64_t *taken);
int32_t picles_nest_feedback_free(picles_ctx *child);

/* ---- track samples (ABI 14): sea state along moving platforms — altimeter passes, ships, drifting buoys — sampled on
 * the device.  Every observation is an EVENT with its own time and place (t_k, x_k, y_k); this output is addressed by event, not by node
 * and cadence: behind each step only the events whose time lies next to the clock are sampled, and their four corners are mixed on the
 * device into a table that stays in device memory. ----
 * THE SET.  A context holds at most one track set of m >= 1 events: t[m] the event times, finite and nondecreasing; ij[8 m] the corner
 * nodes as planes — ij[c m + k] the global 0-based i of corner c of event k, ij[(4 + c) m + k] its j, c = 0..3 in the visiting order of
 * picles_amd.station_output.locate_points —; w[4 m] the weights, w[c m + k], finite and >= 0; and the HORIZON H > 0, the longest step
 * that will be taken while the set lives.  The geometry is the host's: no coordinate arithmetic on the device.
 * THE TABLE.  Per event 8 doubles, as 8 planes of m: planes 0-3 e_b, mx_b, my_b, t_b (the BEFORE slot), planes 4-7 e_a, mx_a, my_a, t_a
 * (the AFTER slot).  Every entry is NaN after init.
 * A TRACK SAMPLE at the clock T visits exactly the events with  T - H < t_k < T + H  (T - H and T + H one IEEE operation each): the
 * library keeps a host copy of t and finds that contiguous range by binary search; when it is empty nothing is launched.  Per visited
 * event (E, MX, MY) is the station definition of the nesting section above over its four corners in order — a corner is WET when e, m_x,
 * m_y are finite, e > 0 and m_x*m_x + m_y*m_y > 0;  W = SE = SX = SY = +0.0;  for c = 0..3, if wet:  W = W + w;  SE = SE + w*e;
 * SX = SX + w*m_x;  SY = SY + w*m_y;  E = SE / W;  MX = SX / W;  MY = SY / W;  valid when W > 0 and MX*MX + MY*MY > 0, otherwise NaN in
 * all three; every operation one IEEE operation — where a corner's value is what picles_get_state would return for that node at that
 * moment.  Then
 *     if t_k >= T:                         the before slot becomes (E, MX, MY, T), overwriting what was there
 *     if t_k <= T and t_a is still NaN:    the after slot becomes (E, MX, MY, T)
 * With sample clocks no farther apart than H, an event inside the sampled span ends with before = the latest sample at a clock <= t_k
 * and after = the earliest sample at a clock >= t_k; an event on a clock gets both slots from that one sample.  The host interpolates.
 * Taking a sample has the rules of a probe sample: it does NOT complete a pending fused step, does not synchronise the host, and leaves
 * State, particles, counters, reach counters, class map, dispatch order and clock untouched; with a fused step pending the corner
 * values are formed from that step's scatter records by the pull k_scatter would run for the node, otherwise read from State.
 * AUTOMATIC SAMPLING: picles_time_step and picles_run_steps take a sample behind every model step they complete, at the clock after the
 * tick, on the context stream, where the automatic probe sample sits.  A step longer than H is refused (-2) before anything is enqueued;
 * picles_run_steps checks up front.  The split-phase calls do not sample.
 *
 *   init:        refuses (context unchanged, picles_last_error set) m < 1, 8 m beyond INT32_MAX, t unsorted or not finite, a node off
 *                the grid, a weight that is negative or not finite, a horizon that is not finite or <= 0, a second init without
 *                picles_track_free, and a context that is a slab, is in slab mode, is on the native ring, has j_begin > 0 or fewer rows
 *                than the grid.  Everything the set needs is allocated here (the fetch staging apart); the arrays are free on return
 *   sample:      one sample now at picles_clock(ctx), on `stream` (NULL: the context stream): picles_probe_sample's semantics.
 *                Refuses: no set
 *   fetch_begin: behind the work enqueued on the context stream so far, gathers the 8 planes of the events [k0, k0 + n) — as they are
 *                at that point of the stream — and starts their copy into pinned staging (grown lazily) on the store stream behind an
 *                event.  Refuses: no set, a fetch already open, a range outside [0, m)
 *   fetch_end:   waits for that copy only and hands out 8 n doubles, [plane][event]; steps enqueued after fetch_begin overlap the copy
 *                and are not waited for.  Refuses: no set, no fetch open
 *   info:        m, the horizon, the samples taken so far — those that visited no event included — (any pointer may be NULL; -1, and
 *                -1 in *m, without a set; no device work)
 *   free:        drops the set so that a new one may be created; picles_destroy does it too, an open fetch included
 * The set is no part of the checkpoint blob or its fingerprint; picles_checkpoint_load and picles_seed leave the set and its table as
 * they are.  picles_set_slab_mode(on) and picles_slab_comm_init refuse (-5) a context that holds a set. */
int32_t picles_track_init(picles_ctx *ctx, int32_t m, const double *t, const int32_t *ij, const double *w, double horizon);
int32_t picles_track_sample(picles_ctx *ctx, void *stream);
int32_t picles_track_fetch_begin(picles_ctx *ctx, int32_t k0, int32_t n);
int32_t picles_track_fetch_end(picles_ctx *ctx, double *out);
int32_t picles_track_info(const picles_ctx *ctx, int32_t *m, double *horizon, int64_t *samples_taken);
int32_t picles_track_free(picles_ctx *ctx);

/* particles (own rows; z is 5 planes: lne, c̄x, c̄y, x, y). Any pointer may be NULL.
 * The state vector of a switched-off particle (on == 0) is dead storage: its content is unspecified. */
int32_t picles_get_particles(picles_ctx *ctx, double *z, uint8_t *on, uint8_t *boundary,
                             int32_t *status);
int32_t picles_set_particles(picles_ctx *ctx, const double *z, const uint8_t *on);

int32_t picles_get_counters(picles_ctx *ctx, picles_counters *c);   /* syncs */
int32_t picles_reset_counters(picles_ctx *ctx);                    /* syncs the device; does NOT complete a pending fused step */
/* on = 1: HIP events around every kernel launch (per-launch samples); on = 2: one event pair around each picles_run_steps call —
 * its launches are back to back on one stream, so advance_ms / advance_launches is the mean launch duration with nothing
 * recorded between the launches (an event between two dependent launches costs about half a microsecond of idle GPU: 20 % of a
 * 256² step, 0.6 % of a 4096² one); picles_slab_run_steps likewise: one pair on the stream of its interior launches (the edge
 * launches and exchanges of its steps are ordered into that stream), no phase events; other launches are timed per launch as
 * with 1.  0: off. */
int32_t picles_enable_timing(picles_ctx *ctx, int32_t on);
int32_t picles_get_timing(picles_ctx *ctx, picles_timing *t);       /* syncs */
/* per-launch device durations [ms] since picles_enable_timing(1): kind 0 = step / advance launches, 1 = scatter, 2 = remesh.
 * Copies up to cap values; returns the number of samples held (>= 0) or an error (< 0). */
int32_t picles_get_timing_samples(picles_ctx *ctx, int32_t kind, double *out_ms, int32_t cap);
/* Diagnostic: the dispatch order the latest whole-grid fused step filed for its successor (cost-ordered dispatch):
 * out[0] = workgroups that did work, out[1] = workgroups with nothing to do, out[2 ...] = the logical 256-node blocks in the order
 * they will be dealt (busy ones from the front, calm ones from the back).  Copies min(cap, 2 + n) ints; returns n = the number of
 * workgroups of that launch when a complete order was filed (out[0] + out[1] == n), 0 when none was (the run is not mixed; a slab reports
 * the order of the launch over its interior rows), < 0 on error.  Syncs and completes a pending fused step, like every getter.  No counterpart in the reference. */
int32_t picles_get_dispatch_order(picles_ctx *ctx, int32_t *out, int32_t cap);
/* Diagnostic: the pull scatter of the wave-per-row fused step skips the candidate codes of a wave whose whole neighbourhood carries one
 * record code (the tile class map; PICLES_PULL_CLASS=0 turns it off).  out[0] = waves that took that path since
 * picles_seed / picles_reset_counters, out[1] = those among them whose neighbourhood held no record at all.  Speed only: results never
 * depend on the path.  Syncs the device; does NOT complete a pending fused step (it can be asked after every step of a fused run).
 * No counterpart in the reference. */
int32_t picles_get_pull_class_counts(picles_ctx *ctx, int64_t *out);
int32_t picles_sync(picles_ctx *ctx);

/* ---- split phases for the slab-partitioned (multi-GPU) step -------------------
 * One model step on rank r:
 *   picles_advance_rows(EDGE)  -> edge rows' scatter records are final
 *   [host: exchange picles_halo_send_dev -> neighbour's picles_halo_recv_dev (RCCL)]
 *   picles_advance_rows(INTERIOR)   (overlaps the exchange on another stream)
 *   picles_scatter_remesh()    -> pull-scatter own rows from own + ghost records, remesh
 * Streams are caller-provided HIP streams (void* = hipStream_t; NULL = context stream). */
#define PICLES_ROWS_ALL      0
#define PICLES_ROWS_EDGE     1
#define PICLES_ROWS_INTERIOR 2
int32_t picles_begin_step(picles_ctx *ctx, double dt, int32_t flags);
int32_t picles_advance_rows(picles_ctx *ctx, int32_t which, void *stream);
int32_t picles_scatter_remesh(picles_ctx *ctx, void *stream);  /* + tick */
/* Fused form of the same step (DESIGN.md k_step): the scatter + remesh of the PREVIOUS step ride on
 * the advance launches of the current one, so a model step is picles_step_rows(EDGE) -> exchange ||
 * picles_step_rows(INTERIOR), with no separate scatter launch.  picles_begin_fused_step returns 1
 * (and does nothing) when the step cannot be fused — time-varying or gridded winds, a per-node
 * metric — in which case the plain phases above are used.  The last step's scatter + remesh are
 * completed lazily by whichever call observes State / particles / counters. */
int32_t picles_begin_fused_step(picles_ctx *ctx, double dt);
int32_t picles_step_rows(picles_ctx *ctx, int32_t which, void *stream);
int32_t picles_end_fused_step(picles_ctx *ctx);
/* device pointers + byte count of the contiguous halo blocks (halo_rows record rows each):
 * side 0 = low-j neighbour, 1 = high-j neighbour */
int32_t picles_halo_send_dev(picles_ctx *ctx, int32_t side, void **ptr, size_t *bytes);
int32_t picles_halo_recv_dev(picles_ctx *ctx, int32_t side, void **ptr, size_t *bytes);
int32_t picles_halo_rows(const picles_ctx *ctx);
int32_t picles_set_halo_rows(picles_ctx *ctx, int32_t halo_rows);  /* re-allocates records */
/* Treat a context that owns ALL rows as a slab anyway (on = 1): the y wrap of a periodic mesh then goes through the ghost
 * rows — filled by the halo exchange with itself, the "ring of one" — instead of being resolved locally.  Results are
 * bit-identical; it exists so that ONE GPU can run, and check, the complete multi-GPU data path (received ghost rows are
 * consumed by the pull).  Call before picles_seed. */
int32_t picles_set_slab_mode(picles_ctx *ctx, int32_t on);

/* ---- native slab ring: the multi-GPU model step driven from C, RCCL send/recv over xGMI -------------------
 * One process per GPU; rank r owns slab r (rows [j_begin, j_end) of its picles_grid), neighbours r-1 / r+1, closed to a
 * ring when the mesh is periodic in y.  RCCL is bound at run time with dlopen (no link-time dependency):
 *   rank 0:  picles_slab_unique_id(id)  ->  the host distributes the 128 bytes (MPI_Bcast, a TCP store, a file ...)
 *   all:     picles_slab_comm_init(ctx, id, rank, world)       ncclCommInitRank + two HIP streams
 *   all:     picles_slab_run_steps(ctx, dt, n, flags)           n model steps, asynchronous, no host work in between:
 *              edge rows (stream E) -> ncclGroup{Send,Send,Recv,Recv} of the halo blocks in place (stream E)
 *              || interior rows (stream M) -> M waits for E
 *            flags as picles_time_step (PICLES_STEP_ZERO_FIRST = run!-style = fused k_step launches)
 *   picles_sync / picles_get_state / ... complete the last step as usual.
 * Replaces the @threads loops of time_step! (TimeSteppers.jl:144-178) across GPUs; the reference has no distributed
 * counterpart on this path. */
#define PICLES_SLAB_ID_BYTES 128
int32_t picles_slab_unique_id(void *id128);
int32_t picles_slab_comm_init(picles_ctx *ctx, const void *id128, int32_t rank, int32_t world);
int32_t picles_slab_run_steps(picles_ctx *ctx, double dt, int32_t n_steps, int32_t flags);
int32_t picles_slab_exchange(picles_ctx *ctx);        /* one synchronous halo exchange of the current records (warm-up of the RCCL channels) */
int32_t picles_slab_streams(picles_ctx *ctx, void **edge_stream, void **interior_stream);   /* hipStream_t of the ring (timing, profiling) */
int32_t picles_slab_comm_destroy(picles_ctx *ctx);
/* Where a ring step's time goes, from HIP events the ring records on its two streams while picles_enable_timing(ctx, 1) is on
 * (five per step): sums over the steps since the last call.  The diagnosis of a multi-GPU run in one look: the edge launch, the
 * exchange behind it (ncclGroup of the halo blocks, on the edge stream), the interior launch (other stream), and whether the
 * exchange had completed when the interior launch ended (it then cost nothing).  Syncs the device; clears the sums. */
typedef struct picles_slab_phases {
    uint64_t steps;            /* ring steps measured                                                          */
    uint64_t exchange_hidden;  /* ... of which the exchange had completed before the interior launch ended      */
    double   edge_ms;          /* edge-row launches (stream E)                                                  */
    double   exchange_ms;      /* end of the edge launch -> end of the send/recv group (stream E)               */
    double   interior_ms;      /* interior launches (stream M)                                                  */
    double   slack_ms;         /* interior end - exchange end, summed: > 0 = the exchange finished first        */
    double   span_ms;          /* edge begin -> the later of exchange end and interior end, summed              */
} picles_slab_phases;
int32_t picles_slab_get_phases(picles_ctx *ctx, picles_slab_phases *out);

/* ---- exact restart: the checkpoint blob (run!(sim; pickup = true) of an Oceananigans-style Checkpointer; the reference's
 * `pickup` keyword is accepted and ignored, run.jl:36) ----------------------------------------------------------------------
 * A blob holds the prognostic state of the context's rows at a step boundary: State, the particles (z, on, status, the step-size
 * memory dtn / qold, the AutoSwitch state), the statistics and scatter-reach counters and the clock (layout: DESIGN.md §11).  The
 * configuration is NOT saved: the restoring program builds the same model (grid, mask, physics, ODE settings, metric, wind source)
 * and loads the blob into it; a fingerprint of that configuration in the blob's header is checked.  A loaded context continues
 * bit for bit as the context that wrote the blob would have.
 *   size:  header + payload bytes of a blob of this context (no device work)
 *   begin: completes a pending step, packs the planes into a device snapshot (one kernel on the context stream) and starts an
 *          asynchronous copy into pinned host memory on the store stream — steps enqueued after it overlap the copy
 *   end:   waits for that copy and writes the blob into buf (>= size bytes).  A synchronous save is begin directly followed by end.
 *   load:  refuses (each with its code below and a picles_last_error text, the context unchanged) a short buffer, a foreign
 *          blob, another format / ABI version, a different configuration, a payload whose checksum (verified on the device,
 *          before anything is overwritten) does not match, and a context with a store snapshot or checkpoint in flight. */
#define PICLES_CKPT_E_SHORT    -20   /* buffer shorter than a header, or than the payload the header announces      */
#define PICLES_CKPT_E_MAGIC    -21   /* not a checkpoint blob                                                         */
#define PICLES_CKPT_E_VERSION  -22   /* another blob format or ABI version                                            */
#define PICLES_CKPT_E_CONFIG   -23   /* fingerprint mismatch: the context was not built from the same configuration   */
#define PICLES_CKPT_E_CHECKSUM -24   /* the payload's checksum does not match                                         */
#define PICLES_CKPT_E_BUSY     -25   /* a store / diagnostics snapshot or checkpoint of this context is in flight (load), or a checkpoint is (begin) */
int32_t picles_checkpoint_size(picles_ctx *ctx, size_t *bytes);
int32_t picles_checkpoint_begin(picles_ctx *ctx);
int32_t picles_checkpoint_end(picles_ctx *ctx, void *buf, size_t bytes);
int32_t picles_checkpoint_load(picles_ctx *ctx, const void *buf, size_t bytes);

/* ---- generic particle->mesh scatter of an arbitrary particle list --------------
 * (ParticleInCell.push_to_grid! over a list, ParticleInCell.jl:341-376,530-538):
 * counting-sort into a cell list, LDS-staged grid tiles (ds_add_f64 per corner), one global fp64 atomic per touched tile node.
 * ij: 2*n int32 (0-based birth node), xy: 2*n positions in cell units relative to ij,
 * charge: 3*n (e,mx,my), all SoA planes.  Adds into State. */
int32_t picles_scatter_particles(picles_ctx *ctx, int64_t n, const int32_t *ij,
                                 const double *xy, const double *charge);

#ifdef __cplusplus
}
#endif
#endif /* PICLES_HIP_H */
