# CCLQR.jl -- `ccall` shim between ConstrainedControl.jl and libcclqr.so (include/cclqr.h).
#
# STATUS: source only.  No Julia toolchain exists in the build/test pipeline of this repository, so this file has never been
# executed; the ABI it binds IS exercised (by constrainedcontrol.jl_amd/_capi.py through ctypes).  Struct layouts below mirror
# include/cclqr.h field by field.  `mech_tables` / `ctrl_joints`, which read ConstrainedDynamics internals, are the only
# parts that depend on that package's field names (0.9.x); everything else is plain arrays.
#
# Drop-in points in the reference (janbruedigam/ConstrainedControl.jl v0.3.0):
#   src/control/lqr.jl:63   A, Bu, Bλ, G = linearsystem(...)          ->  CCLQR.linearsystem(h, zd, ctrl, Fd)
#   src/control/lqr.jl:39   Ku = dlqr(A, Bu, Bλ, G, Q, R, Ntemp)      ->  CCLQR.dlqr(A, Bu, Bλ, G, Q, R, Ntemp)
#   src/control/lqr_tracking.jl:40  Ku = dlqr(mechanism, xd, ...)      ->  CCLQR.dlqr_tracking(h, zd, Fd, ctrl, Q, R, N)
#   simulate!(mech, tend, lqr; record) on a batch                     ->  CCLQR.simulate_batch!(h, c, z0, steps; record, noise)
module CCLQR

using LinearAlgebra

const lib = get(ENV, "CCLQR_LIB", joinpath(@__DIR__, "..", "constrainedcontrol.jl_amd", "libcclqr.so"))

struct MechDesc            # cclqr_mech_desc
    nb::Int32; ne::Int32
    dt::Float64; g::Float64
    mass::Ptr{Float64}; inertia::Ptr{Float64}
    parent::Ptr{Int32}; child::Ptr{Int32}; type::Ptr{Int32}
    p1::Ptr{Float64}; p2::Ptr{Float64}; axis::Ptr{Float64}; qoff::Ptr{Float64}
end

struct CtrlDesc            # cclqr_ctrl_desc
    mu::Int32; ctrl_joint::Ptr{Int32}
    nK::Int32; N::Int32; K::Ptr{Float64}
    nsp::Int32; zd::Ptr{Float64}; Fd::Ptr{Float64}
    fric::Ptr{Float64}; noise_scale::Float64
    npid::Int32; pid_joint::Ptr{Int32}
    pid_P::Ptr{Float64}; pid_I::Ptr{Float64}; pid_D::Ptr{Float64}; pid_goal::Ptr{Float64}     # PID{T,N}, src/control/pid.jl:3-11
    noise_philox::Int32; noise_seed::UInt64                                                    # reproducible stand-in for randn()
    n_ctrl::Int32                                                                              # > 1: one (K, zd, Fd) table per instance
end

struct RolloutOpts         # cclqr_rollout_opts
    first_instance::Int64
    pid_state_dev::Ptr{Float64}
    pid_state_len::Int64
    noise_ws_dev::Ptr{Float64}
    noise_ws_len::Int64
    newton_mode::Int32
    flags::Int32               # ROLLOUT_NO_ALLOC: the call may neither allocate nor synchronise (a hipGraph capture is open on the device)
    newton_eps_alone::Float64
end
const ROLLOUT_NO_ALLOC = Int32(1)
const ROLLOUT_CARRY_STATUS = Int32(4)      # `status` carries an instance's status across launches: a lost instance stays frozen (step-per-launch loops)
const ROLLOUT_RUNTIME_PLAN = Int32(16)     # a single 16- / 17-link chain runs on the general chain kernel instead of its fixed-plan kernel: same bits
const ROLLOUT_PACK_WAVEFRONTS = Int32(2)   # every wavefront of a chain launch full whatever the batch size (many launches sharing the device at once)

struct RiccatiOpts         # cclqr_riccati_opts
    path::Int32
    bf16_terms::Int32
    keep_last::Int32
    reserved::Int32
end

const ABI_VERSION = 202    # include/cclqr.h CCLQR_ABI_VERSION: the structs above mirror THAT header field by field
"sizeof / fieldoffset of the four mirrors above in the order cclqr_abi_layout reports the library's own (include/cclqr.h)"
mirrored_layout() = Int32[x for S in (MechDesc, CtrlDesc, RiccatiOpts, RolloutOpts) for x in (sizeof(S), (fieldoffset(S, i) for i in 1:fieldcount(S))...)]
"call once after loading: a library built from another header would read these structs past their end (ADVICE r2).  The version number says which
header the library was built from; cclqr_abi_layout says what the C compiler made of it, so the mirrors are verified field by field (VERDICT r4)."
function check_abi()
    v = ccall((:cclqr_version, lib), Cint, ())
    v == ABI_VERSION || error("libcclqr.so has ABI version $v, CCLQR.jl was written for $ABI_VERSION")
    want = mirrored_layout()
    got = zeros(Int32, length(want))
    n = ccall((:cclqr_abi_layout, lib), Cint, (Ptr{Int32}, Int32), got, Int32(length(got)))
    (n == length(want) && got == want) || error("struct layout mismatch: libcclqr.so reports $got, CCLQR.jl mirrors $want")
    nothing
end

const REVOLUTE = Int32(0)
const PRISMATIC = Int32(1)
const FIXED_ORIENTATION = Int32(2)     # FixedOrientation(a, b; qoffset): one Rotational3 constraint (examples/lqr_deltabot.jl:25)

# Closed-loop mechanisms (examples/lqr_deltabot.jl): `linearize_projected` returns A' = A - Bλ (G Bλ)^-1 G A and D = Bu - Bλ (G Bλ)^-1 G Bu
# (lqr.jl:151) from cclqr_linearize_projected; pass them to `riccati` with empty Bλ (mx x 0) and G (0 x mx).
function linearize_projected(mech::Ptr{Cvoid}, zd::Vector{Float64}, nb::Int, ctrl_joint::Vector{Int32}, Fd::Vector{Float64}; h = 0.0)
    mx, mu = 12nb, length(ctrl_joint)
    Ap, D = zeros(mx * mx), zeros(mx * mu)
    check(ccall((:cclqr_linearize_projected, lib), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}),
                mech, Int32(1), zd, Int32(mu), ctrl_joint, Fd, h, Ap, D))
    return permutedims(reshape(Ap, mx, mx)), permutedims(reshape(D, mu, mx))      # row-major on the C side
end

# One LQR per setpoint, built and kept on the device (cclqr_ctrl_create_lqr_batch): zd is nb*13*n doubles, Q / R the Δt-scaled weights
# (lqr.jl:18-19) row-major; returns the controller handle for rollout!(...) and the break indices.
function lqr_batch(mech::Ptr{Cvoid}, n::Int, zd::Vector{Float64}, ctrl_joint::Vector{Int32}, Q::Vector{Float64}, R::Vector{Float64}, N::Int;
                   tol = 1e-5, infinite_horizon = false)      # infinite_horizon: LQR{T,Inf} -- N = ceil(10/Δt) (lqr.jl:26), only Ku[1] is kept
    h = Ref{Ptr{Cvoid}}(C_NULL); kb = zeros(Int32, n)
    check(ccall((:cclqr_ctrl_create_lqr_batch, lib), Cint,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Float64, Ptr{Int32}, Ref{Ptr{Cvoid}}),
                mech, Int32(n), zd, Int32(length(ctrl_joint)), ctrl_joint, C_NULL, Q, R, Int32(N), Int32(infinite_horizon ? 1 : 0), tol, kb, h))
    return h[], kb
end

# Time-varying recursion (lqr_tracking.jl:73-122) on per-knot models the caller brings (row-major [N-1][..][..] flattened), e.g. the
# projected pairs of a closed-loop mechanism with ml = 0
function dlqr_tv(mx::Int, mu::Int, ml::Int, A::Vector{Float64}, Bu::Vector{Float64}, Bl::Vector{Float64}, G::Vector{Float64},
                 Q::Vector{Float64}, R::Vector{Float64}, N::Int; tol = 1e-5)
    K = zeros((N - 1) * mu * mx); kb = zeros(Int32, 1)
    check(ccall((:cclqr_riccati_tv, lib), Cint,
                (Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Ptr{Float64}, Ptr{Int32}),
                Int32(mx), Int32(mu), Int32(ml), A, Bu, ml > 0 ? pointer(Bl) : C_NULL, ml > 0 ? pointer(G) : C_NULL, Q, R, Int32(N), tol, K, kb))
    return K, Int(kb[1])
end

lasterror() = unsafe_string(ccall((:cclqr_last_error, lib), Cstring, ()))
function check(rc::Integer)
    rc == 0 && return nothing
    msg = lasterror()
    rc == -1 && throw(AssertionError(msg))          # CCLQR_EINVAL   <-> the reference's @assert (lqr.jl:59-60)
    rc == -2 && throw(SingularException(0))         # CCLQR_ESINGULAR <-> LAPACK exception from lqr.jl:151,160
    rc == -3 && (@info msg; return nothing)         # CCLQR_ENOCONV  <-> `@info "Riccati recursion did not converge."` (lqr.jl:41)
    error("cclqr ($rc): $msg")
end

# ---------------------------------------------------------------------------------------------------------------------
# Mechanism -> flat tables.  Assumes ConstrainedDynamics 0.9.x field names: mechanism.bodies / eqconstraints / origin / Δt / g,
# body.m, body.J, eqc.parentid, eqc.childids, eqc.constraints with .vertices, .V3 (axis row), .qoffset.
# Body ids 1..Nb, joint ids Nb+1.. (examples/trackingLQR_triple_cartpole.jl:109-111).
#
# An EqualityConstraint may bundle SEVERAL joints off one parent: examples/lqr_deltabot.jl:25 builds
#   EqualityConstraint(Revolute(origin, lowerlegl, ...), Revolute(origin, lowerlegr, ...), FixedOrientation(origin, platform))
# whose `constraints` is the flat tuple (Translational3, Rotational2, Translational3, Rotational2, Rotational3) with
# `childids` = (l, l, r, r, platform) -- one entry per component.  The C side knows 1-DoF joints and the FixedOrientation, one child
# each, so every EqualityConstraint is EXPANDED into one table joint per distinct child (components grouped by child id, in order):
#   Translational{3} + Rotational{2} -> REVOLUTE,  Translational{2} + Rotational{3} -> PRISMATIC,  a lone Rotational{3} -> FIXED_ORIENTATION;
# anything else is refused (a silent flattening would simulate a different mechanism).  `joint_of_eqc[id]` lists the 0-based table
# joints an EqualityConstraint id became: an LQR's `eqcids` (lqr.jl:49-57; one input per 1-DoF joint) map through it.
nrows(c) = length(c)                                  # Joint{T,N}: N constraint rows
istrans(c) = occursin("Translational", string(typeof(c)))
function mech_tables(mechanism)
    bodies = collect(mechanism.bodies); eqcs = collect(mechanism.eqconstraints)
    nb = length(bodies)
    bodyindex = Dict(b.id => Int32(i - 1) for (i, b) in enumerate(bodies))
    mass = Float64[b.m for b in bodies]
    inertia = reduce(vcat, [vec(permutedims(Matrix(b.J))) for b in bodies])          # row-major 3x3 per body
    parent = Int32[]; child = Int32[]; typ = Int32[]
    p1 = Float64[]; p2 = Float64[]; axis = Float64[]; qoff = Float64[]
    joint_of_eqc = Dict{Int,Vector{Int32}}()
    for e in eqcs
        cs = collect(e.constraints); cids = collect(e.childids)
        length(cs) == length(cids) || error("EqualityConstraint $(e.id): constraints and childids differ in length")
        joint_of_eqc[e.id] = Int32[]
        i = 1
        while i <= length(cs)
            j = i
            while j < length(cs) && cids[j+1] == cids[i]; j += 1; end
            comp = cs[i:j]
            tr = [c for c in comp if istrans(c)]; ro = [c for c in comp if !istrans(c)]
            kind = if length(tr) == 1 && length(ro) == 1 && nrows(tr[1]) == 3 && nrows(ro[1]) == 2
                REVOLUTE
            elseif length(tr) == 1 && length(ro) == 1 && nrows(tr[1]) == 2 && nrows(ro[1]) == 3
                PRISMATIC
            elseif isempty(tr) && length(ro) == 1 && nrows(ro[1]) == 3
                FIXED_ORIENTATION
            else
                error("EqualityConstraint $(e.id), child $(cids[i]): only Revolute, Prismatic and FixedOrientation components are supported")
            end
            push!(joint_of_eqc[e.id], Int32(length(typ)))
            push!(parent, get(bodyindex, e.parentid, Int32(-1)))                       # origin -> -1
            push!(child, bodyindex[cids[i]]); push!(typ, kind)
            if kind == FIXED_ORIENTATION
                append!(p1, zeros(3)); append!(p2, zeros(3)); append!(axis, [1.0, 0.0, 0.0])
            else
                append!(p1, Vector{Float64}(tr[1].vertices[1])); append!(p2, Vector{Float64}(tr[1].vertices[2]))
                append!(axis, Vector{Float64}(vec(kind == REVOLUTE ? ro[1].V3 : tr[1].V3)))
            end
            q = ro[1].qoffset
            append!(qoff, Float64[q.s, q.v1, q.v2, q.v3])
            i = j + 1
        end
    end
    ne = length(typ)
    return (; nb, ne, dt = Float64(mechanism.Δt), g = Float64(mechanism.g), mass, inertia, parent, child, typ, p1, p2, axis, qoff, joint_of_eqc)
end
"0-based table joints of the 1-DoF joints named by an LQR's eqcids (lqr.jl:49-57): every id must have become exactly one 1-DoF joint"
function ctrl_joints(t, eqcids)
    out = Int32[]
    for id in eqcids
        js = [j for j in t.joint_of_eqc[id] if t.typ[j+1] != FIXED_ORIENTATION]
        length(js) == 1 || throw(AssertionError("eqcid $id bundles $(length(js)) 1-DoF joints: name the joint (lqr.jl:1-2 'Only for 1dof joints')"))
        push!(out, js[1])
    end
    out
end

mutable struct MechHandle
    ptr::Ptr{Cvoid}
    nb::Int
    function MechHandle(t)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve t begin
            d = MechDesc(t.nb, t.ne, t.dt, t.g, pointer(t.mass), pointer(t.inertia), pointer(t.parent), pointer(t.child), pointer(t.typ),
                         pointer(t.p1), pointer(t.p2), pointer(t.axis), pointer(t.qoff))
            check_abi()
            check(ccall((:cclqr_mech_create, lib), Cint, (Ref{MechDesc}, Ref{Ptr{Cvoid}}), d, h))
        end
        obj = new(h[], t.nb)
        finalizer(o -> ccall((:cclqr_mech_destroy, lib), Cint, (Ptr{Cvoid},), o.ptr), obj)
        obj
    end
end
MechHandle(mechanism, ::Val{:mechanism}) = MechHandle(mech_tables(mechanism))

# body states as the 13 x Nb matrix the C side reads as [nb][13] = x(3) q(4) v(3) ω(3)
pack_state(xd, qd, vd, ωd) = reduce(hcat, [Float64[x...; q.s; q.v1; q.v2; q.v3; v...; ω...] for (x, q, v, ω) in zip(xd, qd, vd, ωd)])

# C is row-major, Julia column-major: a C matrix [r][c] is read here as a (c, r) array and transposed lazily.
cmat(buf, r, c) = permutedims(reshape(buf, c, r))

"linearsystem(mechanism, xd, vd, qd, ωd, Fτd, bodyids, eqcids) replacement (lqr.jl:63).  ctrl = 0-based joint indices."
function linearsystem(h::MechHandle, zd::Matrix{Float64}, ctrl::Vector{Int32}, Fd::Vector{Float64})
    nb = h.nb; mx, ml, mu = 12nb, 5nb, length(ctrl)
    A = zeros(mx * mx); Bu = zeros(mx * max(mu, 1)); Bl = zeros(mx * ml); G = zeros(ml * mx)
    check(ccall((:cclqr_linearize, lib), Cint,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                h.ptr, 1, zd, mu, ctrl, Fd, A, Bu, Bl, G))
    cmat(A, mx, mx), cmat(Bu[1:mx*mu], mx, mu), cmat(Bl, mx, ml), cmat(G, ml, mx)
end

"dlqr(A,Bu,Bλ,G,Q,R,N) replacement (lqr.jl:141-184).  Q, R are the Δt-scaled block diagonals of lqr.jl:18-19.  Returns Ku[k][i] and the break index."
function dlqr(A, Bu, Bλ, G, Q, R, N::Integer; tol = 1e-5)
    mx, mu, ml = size(A, 1), size(Bu, 2), size(Bλ, 2)
    rowmajor(M) = vec(permutedims(Matrix{Float64}(M)))
    K = zeros(mx * mu * max(N - 1, 0)); kb = Ref{Int32}(0)
    check(ccall((:cclqr_riccati, lib), Cint,
                (Int32, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Float64,
                 Ptr{Float64}, Ref{Int32}),
                1, mx, mu, ml, rowmajor(A), rowmajor(Bu), rowmajor(Bλ), rowmajor(G), rowmajor(Q), rowmajor(R), N, tol, K, kb))
    K3 = reshape(K, mx, mu, N - 1)                                   # C layout [N-1][mu][mx]
    Ku = [[reshape(K3[:, i, k], 1, mx) for i = 1:mu] for k = 1:N-1]   # the layout of lqr.jl:145
    Ku, Int(kb[])
end

"dlqr(A_p, Bu_p, Bλ_p, G_p, Q_p, R_p, N) (lqr.jl:141-184) for every p in one launch (cclqr_riccati_weights): vectors of matrices, one model per problem; Qs and Rs
 hold ONE pair of Δt-scaled weights (shared) or one pair per problem -- any other count is refused by the library.  Returns (Ku[p][k][i], kbreak[p])."
function dlqr_weights(As::Vector, Bus::Vector, Bλs::Vector, Gs::Vector, Qs::Vector, Rs::Vector, N::Integer; tol = 1e-5)
    np = length(As); mx, mu, ml = size(As[1], 1), size(Bus[1], 2), size(Bλs[1], 2)
    length(Qs) == length(Rs) || throw(AssertionError("Qs and Rs must hold the same number of weight pairs"))
    rowmajor(Ms) = reduce(vcat, [vec(permutedims(Matrix{Float64}(M))) for M in Ms]; init = Float64[])
    K = zeros(mx * mu * max(N - 1, 0) * np); kb = zeros(Int32, np)
    check(ccall((:cclqr_riccati_weights, lib), Cint,
                (Int32, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Float64,
                 Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}),
                np, mx, mu, ml, rowmajor(As), rowmajor(Bus), rowmajor(Bλs), rowmajor(Gs), Int32(length(Qs)), rowmajor(Qs), rowmajor(Rs), N, tol, K, kb, C_NULL))
    K4 = reshape(K, mx, mu, max(N - 1, 0), np)                       # C layout [np][N-1][mu][mx]
    [[[reshape(K4[:, i, k, p], 1, mx) for i = 1:mu] for k = 1:N-1] for p = 1:np], Int.(kb)
end

"dlqr(mechanism, xd, vd, qd, ωd, Fτd, eqcids, Q, R, N) replacement (lqr_tracking.jl:73-122): zd is 13 x Nb x N, Fd is mu x N."
function dlqr_tracking(h::MechHandle, zd::Array{Float64,3}, Fd::Matrix{Float64}, ctrl::Vector{Int32}, Q, R, N::Integer; tol = 1e-5)
    mx, mu = 12h.nb, length(ctrl)
    rowmajor(M) = vec(permutedims(Matrix{Float64}(M)))
    K = zeros(mx * mu * (N - 1)); kb = Ref{Int32}(0)
    check(ccall((:cclqr_riccati_tracking, lib), Cint,
                (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Ptr{Float64}, Ref{Int32}),
                h.ptr, mu, ctrl, zd, Fd, rowmajor(Q), rowmajor(R), N, tol, K, kb))
    K3 = reshape(K, mx, mu, N - 1)
    [[reshape(K3[:, i, k], 1, mx) for i = 1:mu] for k = 1:N-1], Int(kb[])
end

mutable struct CtrlHandle
    ptr::Ptr{Cvoid}
end
"Device controller tables from the fields of an LQR / TrackingLQR (lqr.jl:3-15, lqr_tracking.jl:3-15).
 K: mx x mu x nK, zd: 13 x Nb x nsp, Fd: mu x nsp, N = horizon steps (0 for LQR{T,Inf}), ctrl = 0-based joint indices."
function CtrlHandle(h::MechHandle, ctrl::Vector{Int32}, K::Array{Float64,3}, N::Integer, zd::Array{Float64,3}, Fd::Matrix{Float64};
                    fric::Union{Nothing,Vector{Float64}} = nothing, noise_scale = 0.0, n_ctrl::Integer = 0)
    c = Ref{Ptr{Cvoid}}(C_NULL)
    nc = max(n_ctrl, 1)          # n_ctrl > 1: K is mx x mu x (nK * n_ctrl), zd 13 x Nb x (nsp * n_ctrl), Fd mu x (nsp * n_ctrl): one table per instance
    GC.@preserve ctrl K zd Fd fric begin
        d = CtrlDesc(length(ctrl), pointer(ctrl), size(K, 3) ÷ nc, N, pointer(K), size(zd, 3) ÷ nc, pointer(zd), pointer(Fd),
                     fric === nothing ? Ptr{Float64}(C_NULL) : pointer(fric), noise_scale,
                     0, Ptr{Int32}(C_NULL), Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL), 0, UInt64(0),
                     n_ctrl)
        check(ccall((:cclqr_ctrl_create, lib), Cint, (Ptr{Cvoid}, Ref{CtrlDesc}, Ref{Ptr{Cvoid}}), h.ptr, d, c))
    end
    obj = CtrlHandle(c[])
    finalizer(o -> ccall((:cclqr_ctrl_destroy, lib), Cint, (Ptr{Cvoid},), o.ptr), obj)
    obj
end

"Batched simulate!: z0 is 13 x Nb x n_inst; returns (traj 13 x Nb x steps x n_inst or nothing, zT, status)."
function simulate_batch!(h::MechHandle, c::CtrlHandle, z0::Array{Float64,3}, steps::Integer; record = true, noise = nothing, k0 = 1,
                         first_instance = 0, newton_mode = 0, newton_eps_alone = 0.0)
    n = size(z0, 3)
    traj = record ? zeros(13, h.nb, steps, n) : nothing
    zT = similar(z0); status = zeros(Int32, n)
    o = RolloutOpts(first_instance, C_NULL, 0, C_NULL, 0, newton_mode, 0, newton_eps_alone)      # first_instance: global index of instance 1 of this shard
    check(ccall((:cclqr_rollout_host_ex, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ref{RolloutOpts}),
                h.ptr, c.ptr, n, steps, k0, z0, noise === nothing ? C_NULL : noise, record ? traj : C_NULL, zT, status, o))
    traj, zT, status
end

"Device-pointer rollout with explicit options (cclqr_rollout_ex): all pointers are device addresses (e.g. from AMDGPU.jl), the launch is
 asynchronous on `stream`.  first_instance = global index of instance 1 of this shard (noise stream and per-instance controller table),
 pid_state = device buffer n_inst x Nb x 2 carrying the PID integrators between launches (C_NULL: none), noise_ws = device workspace of
 n_inst x steps doubles for the Philox samples (C_NULL: the controller handle's own; see reserve_noise!), newton_mode 0 = exact rule,
 flags = ROLLOUT_NO_ALLOC | ROLLOUT_PACK_WAVEFRONTS | ROLLOUT_CARRY_STATUS | ROLLOUT_RUNTIME_PLAN (include/cclqr.h)."
function rollout_dev!(h::MechHandle, c::CtrlHandle, n::Integer, steps::Integer, k0::Integer, z0::Ptr{Float64}, lam::Ptr{Float64},
                      traj::Ptr{Float64}, zT::Ptr{Float64}, status::Ptr{Int32}; noise::Ptr{Float64} = Ptr{Float64}(C_NULL), noise_stride = 0,
                      first_instance = 0, pid_state::Ptr{Float64} = Ptr{Float64}(C_NULL), noise_ws::Ptr{Float64} = Ptr{Float64}(C_NULL),
                      newton_mode = 0, newton_eps_alone = 0.0, flags = Int32(0), stream::Ptr{Cvoid} = C_NULL)
    o = RolloutOpts(first_instance, pid_state, pid_state == C_NULL ? 0 : n * h.nb * 2, noise_ws, noise_ws == C_NULL ? 0 : n * steps, newton_mode, Int32(flags), newton_eps_alone)
    check(ccall((:cclqr_rollout_ex, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int32},
                 Ref{RolloutOpts}, Ptr{Cvoid}),
                h.ptr, c.ptr, n, steps, k0, z0, lam, noise, noise_stride, traj, zT, status, o, stream))
end

"Per-instance plants (cclqr_plants_create): what `Box(...)`, `Revolute(...; p1, p2)` and `Mechanism(...)` (examples/lqr_cartpole.jl:21-32) fix for one plant, one set
 per instance.  mass Nb x n, inertia 9 x Nb x n (each 3 x 3 block column-major = row-major, it is symmetric), p1 / p2 3 x Ne x n in the order of mech_tables; `nothing` =
 the mechanism's own value.  first_index = global index (0-based) of the first plant.  Host arrays."
mutable struct PlantsHandle
    ptr::Ptr{Cvoid}
    n::Int
    mech::MechHandle      # keeps the mechanism alive: the plants were packed in its link order
end
function PlantsHandle(h::MechHandle, n::Integer; mass = nothing, inertia = nothing, p1 = nothing, p2 = nothing, first_index = 0)
    arg(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve mass inertia p1 p2 check(ccall((:cclqr_plants_create, lib), Cint,
                (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
                h.ptr, n, first_index, arg(mass), arg(inertia), arg(p1), arg(p2), 0, C_NULL, out))
    obj = PlantsHandle(out[], n, h)
    finalizer(o -> ccall((:cclqr_plants_destroy, lib), Cint, (Ptr{Cvoid},), o.ptr), obj)
    obj
end

"rollout_dev! on per-instance plants (cclqr_rollout_plants): instance i of the launch runs plant first_instance + i - first_index of `p`; the states must lie on each
 instance's own plant's constraint manifold.  Everything else as rollout_dev!."
function rollout_plants_dev!(h::MechHandle, p::PlantsHandle, c::CtrlHandle, n::Integer, steps::Integer, k0::Integer, z0::Ptr{Float64}, lam::Ptr{Float64},
                             traj::Ptr{Float64}, zT::Ptr{Float64}, status::Ptr{Int32}; noise::Ptr{Float64} = Ptr{Float64}(C_NULL), noise_stride = 0,
                             first_instance = 0, pid_state::Ptr{Float64} = Ptr{Float64}(C_NULL), noise_ws::Ptr{Float64} = Ptr{Float64}(C_NULL),
                             newton_mode = 0, newton_eps_alone = 0.0, flags = Int32(0), stream::Ptr{Cvoid} = C_NULL)
    o = RolloutOpts(first_instance, pid_state, pid_state == C_NULL ? 0 : n * h.nb * 2, noise_ws, noise_ws == C_NULL ? 0 : n * steps, newton_mode, Int32(flags), newton_eps_alone)
    check(ccall((:cclqr_rollout_plants, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int32},
                 Ref{RolloutOpts}, Ptr{Cvoid}),
                h.ptr, p.ptr, c.ptr, n, steps, k0, z0, lam, noise, noise_stride, traj, zT, status, o, stream))
end

"linearsystem (lqr.jl:63) of knot k on plant first_plant + k of `p` (cclqr_linearize_plants): zd is 13 x Nb x nk on the plants' own constraint manifolds, Fd is
 mu x nk.  Returns the row-major buffers of the nk models (cmat reads one)."
function linearsystem_plants(h::MechHandle, p::PlantsHandle, nk::Integer, zd::Array{Float64}, ctrl::Vector{Int32}, Fd::Array{Float64}; first_plant = 0)
    nb = h.nb; mx, ml, mu = 12nb, 5nb, length(ctrl)
    A = zeros(nk * mx * mx); Bu = zeros(nk * mx * max(mu, 1)); Bl = zeros(nk * mx * ml); G = zeros(nk * ml * mx)
    check(ccall((:cclqr_linearize_plants, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                h.ptr, p.ptr, first_plant, nk, zd, mu, ctrl, Fd, A, Bu, Bl, G))
    A, Bu, Bl, G
end

"One LQR per plant, built and kept on the device (cclqr_ctrl_create_lqr_batch_plants): lqr_batch with table k designed on plant first_plant + k of `p` -- linearsystem
 (lqr.jl:63) and dlqr (lqr.jl:141-184) on the mechanism rebuilt with that plant's numbers.  Fd (mu x n, or nothing) holds the caller's holding inputs."
function lqr_batch_plants(h::MechHandle, p::PlantsHandle, n::Int, zd::Array{Float64}, ctrl_joint::Vector{Int32}, Q::Vector{Float64}, R::Vector{Float64}, N::Int;
                          Fd = nothing, first_plant = 0, tol = 1e-5, infinite_horizon = false)
    out = Ref{Ptr{Cvoid}}(C_NULL); kb = zeros(Int32, n)
    fd = Fd === nothing ? Ptr{Float64}(C_NULL) : pointer(Fd)
    GC.@preserve Fd check(ccall((:cclqr_ctrl_create_lqr_batch_plants, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Float64, Ptr{Int32},
                 Ref{Ptr{Cvoid}}),
                h.ptr, p.ptr, first_plant, Int32(n), zd, Int32(length(ctrl_joint)), ctrl_joint, fd, Q, R, Int32(N), Int32(infinite_horizon ? 1 : 0), tol, kb, out))
    return out[], kb
end

"One LQR per weight candidate, built and kept on the device (cclqr_ctrl_create_lqr_batch_weights): table k is LQR(mechanism, bodyids, eqcids, Q_k, R_k, horizon; ...)
 (lqr.jl:49-66) at setpoint k (zd 13 x Nb x n), on plant first_plant + k of `p` (`nothing`: the mechanism's own plant).  Q holds n_weights row-major 12Nb x 12Nb
 matrices one behind the other, R n_weights mu x mu ones, Δt-scaled (lqr.jl:18-19); n_weights is 1 or n, anything else is refused by the library."
function lqr_batch_weights(h::MechHandle, p::Union{PlantsHandle,Nothing}, n::Int, zd::Array{Float64}, ctrl_joint::Vector{Int32}, n_weights::Int, Q::Vector{Float64},
                           R::Vector{Float64}, N::Int; Fd = nothing, first_plant = 0, tol = 1e-5, infinite_horizon = false)
    out = Ref{Ptr{Cvoid}}(C_NULL); kb = zeros(Int32, n)
    fd = Fd === nothing ? Ptr{Float64}(C_NULL) : pointer(Fd)
    GC.@preserve Fd check(ccall((:cclqr_ctrl_create_lqr_batch_weights, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Float64, Ptr{Int32},
                 Ref{Ptr{Cvoid}}),
                h.ptr, p === nothing ? C_NULL : p.ptr, first_plant, Int32(n), zd, Int32(length(ctrl_joint)), ctrl_joint, fd, Int32(n_weights), Q, R, Int32(N),
                Int32(infinite_horizon ? 1 : 0), tol, kb, out))
    return out[], kb
end

"One TrackingLQR per plant and / or reference trajectory, built and kept on the device (cclqr_ctrl_create_tracking_batch_plants): table k is
 TrackingLQR(mechanism_k, storage_k, Fτ_k, eqcids, Q, R) (lqr_tracking.jl:17-43) on plant first_plant + k of `p` (`nothing`: the mechanism's own plant for every
 trajectory).  zd is 13 x Nb x N x n (storage_k's x, q, v, ω of every step, each trajectory on its own plant's constraint manifold), Fd mu x N x n or nothing; host arrays.
 fric (one entry per joint) / noise_scale / noise_seed fix the friction / noise law of examples/trackingLQR_triple_cartpole.jl:93-111 on the controller.
 workspace_bytes <= 0: the library's default budget; the problems run in chunks that stay within it.  Returns the controller handle and the break indices."
function tracking_batch_plants(h::MechHandle, p::Union{Nothing,PlantsHandle}, n::Int, N::Int, zd::Array{Float64}, ctrl_joint::Vector{Int32}, Q::Vector{Float64},
                               R::Vector{Float64}; Fd = nothing, first_plant = 0, tol = 1e-5, fric = nothing, noise_scale = 0.0, noise_seed = nothing,
                               workspace_bytes = 0, stream::Ptr{Cvoid} = C_NULL)
    out = Ref{Ptr{Cvoid}}(C_NULL); kb = zeros(Int32, n)
    fd = Fd === nothing ? Ptr{Float64}(C_NULL) : pointer(Fd)
    GC.@preserve Fd fric begin
        law = CtrlDesc(0, Ptr{Int32}(C_NULL), 0, 0, Ptr{Float64}(C_NULL), 0, Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL),
                       fric === nothing ? Ptr{Float64}(C_NULL) : pointer(fric), noise_scale,
                       0, Ptr{Int32}(C_NULL), Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL),
                       noise_seed === nothing ? 0 : 1, noise_seed === nothing ? UInt64(0) : UInt64(noise_seed), 0)
        check(ccall((:cclqr_ctrl_create_tracking_batch_plants, lib), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Float64, Ref{CtrlDesc},
                     Int64, Ptr{Int32}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
                    h.ptr, p === nothing ? C_NULL : p.ptr, first_plant, Int32(n), Int32(N), zd, fd, Int32(0), Int32(length(ctrl_joint)), ctrl_joint, Q, R, tol, law,
                    workspace_bytes, kb, stream, out))
    end
    return out[], kb
end

"lqr.K[k][i] (lqr.jl:4, lqr_tracking.jl:4) of one table (0-based) of a controller, read back from the device (cclqr_ctrl_get_gains): mx x mu x nK, the caller's body order.
 `c` is the pointer a constructor returned (CtrlHandle(...).ptr, lqr_batch, lqr_batch_plants, tracking_batch_plants)."
function ctrl_gains(h::MechHandle, c::Ptr{Cvoid}, table::Integer, nK::Integer, mu::Integer)
    K = zeros(12 * h.nb, mu, nK)
    check(ccall((:cclqr_ctrl_get_gains, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}), h.ptr, c, table, K))
    K
end

"The weights a run is ranked by, on the device (cclqr_score_create): Qb is 12 x 12 x Nb -- body b's block TRANSPOSED into Julia's column-major order, i.e.
 Qb[:, :, b] = Q[b]' -- in the order of mech_tables, R is mu x mu transposed likewise; both already scaled by Δt (lqr.jl:18-19).  settle_tol: the stage cost under
 which an instance counts as settled."
mutable struct ScoreHandle
    ptr::Ptr{Cvoid}
    mech::MechHandle
end
function ScoreHandle(h::MechHandle, Qb::Array{Float64}, R::Array{Float64}, mu::Integer; settle_tol = 0.0)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:cclqr_score_create, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Float64, Ref{Ptr{Cvoid}}), h.ptr, Qb, Int32(mu), R, settle_tol, out))
    obj = ScoreHandle(out[], h)
    finalizer(o -> ccall((:cclqr_score_destroy, lib), Cint, (Ptr{Cvoid},), o.ptr), obj)
    obj
end

"Score the slab a rollout_dev! launch has just written (cclqr_rollout_score; device pointers, asynchronous on `stream`): score is 4 x n = (Jx, Ju, peak, last_out) per
 instance, read when k0 > 1 and always written, so that a horizon rolled out chunk by chunk into one small slab (k0 continuation: carry z, lam, status with
 ROLLOUT_CARRY_STATUS, the PID state) is scored bitwise as one launch would be:
     for k0 in 1:chunk:steps
         s = min(chunk, steps - k0 + 1)
         rollout_dev!(h, c, n, s, k0, z, lam, slab, zn, status; flags = ROLLOUT_CARRY_STATUS, stream = stream)
         rollout_score!(h, c, sc, n, s, k0, slab, score; stream = stream)
         z, zn = zn, z
     end"
function rollout_score!(h::MechHandle, c::CtrlHandle, s::ScoreHandle, n::Integer, steps::Integer, k0::Integer, traj::Ptr{Float64}, score::Ptr{Float64};
                        first_instance = 0, stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:cclqr_rollout_score, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                h.ptr, c.ptr, s.ptr, n, steps, k0, first_instance, traj, score, stream))
end

"Bytes of device workspace one rollout_ensemble! call of these sizes needs (cclqr_rollout_ensemble_ws_bytes)."
function rollout_ensemble_ws_bytes(h::MechHandle, mu::Integer, n::Integer, steps::Integer, n_cov::Integer)
    out = Ref{Csize_t}(0)
    check(ccall((:cclqr_rollout_ensemble_ws_bytes, lib), Cint, (Ptr{Cvoid}, Int32, Int64, Int32, Int32, Ref{Csize_t}), h.ptr, mu, n, steps, n_cov, out))
    Int(out[])
end

"The statistics of the slab a rollout_dev! launch has just written ACROSS its instances (cclqr_rollout_ensemble; device pointers except cov_steps, asynchronous on
 `stream`): mean and m2 are (12 nb + mu) x steps -- per step the mean and the centred sum of squares of every coordinate of (Δz, Δu), Δz in the caller's body order --
 and cov is 12 nb x 12 nb x length(cov_steps), the centred co-moment matrices of Δz at the listed absolute steps (each within k0 : k0 + steps - 1).  One fixed
 summation order: behind every launch of the chunk loop of rollout_score!, with mean / m2 advanced by (k0 - 1) columns, the horizon's statistics are bitwise those
 of one call."
function rollout_ensemble!(h::MechHandle, c::CtrlHandle, n::Integer, steps::Integer, k0::Integer, traj::Ptr{Float64}, mean::Ptr{Float64}, m2::Ptr{Float64},
                           ws::Ptr{Cvoid}, ws_bytes::Integer; cov_steps::Vector{Int32} = Int32[], cov::Ptr{Float64} = Ptr{Float64}(C_NULL), first_instance = 0,
                           stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:cclqr_rollout_ensemble, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
                h.ptr, c.ptr, n, steps, k0, first_instance, traj, mean, m2, length(cov_steps), cov_steps, cov, ws, ws_bytes, stream))
end

"(min_bytes, full_bytes) of device workspace for rollout_quantiles! (cclqr_rollout_quantiles_ws_bytes): one slab row, all `steps` rows."
function rollout_quantiles_ws_bytes(h::MechHandle, mu::Integer, n::Integer, steps::Integer)
    lo = Ref{Csize_t}(0); full = Ref{Csize_t}(0)
    check(ccall((:cclqr_rollout_quantiles_ws_bytes, lib), Cint, (Ptr{Cvoid}, Int32, Int64, Int32, Ref{Csize_t}, Ref{Csize_t}), h.ptr, mu, n, steps, lo, full))
    Int(lo[]), Int(full[])
end

"The quantiles of the slab a rollout_dev! launch has just written ACROSS its instances (cclqr_rollout_quantiles; device pointers except prob, asynchronous on
 `stream`): quant is (12 nb + mu) x length(prob) x steps -- per step and probability the quantile of the finite values of every coordinate of (Δz, Δu), 0 the
 minimum, 1 the maximum --, finite (12 nb + mu) x steps their number (or C_NULL).  At most 16384 instances and 16 probabilities.  A function of the multiset of
 values alone: behind every launch of the chunk loop, with quant / finite advanced by (k0 - 1) steps, any chunking and any ws_bytes >= min_bytes give the same bits."
function rollout_quantiles!(h::MechHandle, c::CtrlHandle, n::Integer, steps::Integer, k0::Integer, traj::Ptr{Float64}, prob::Vector{Float64}, quant::Ptr{Float64},
                            ws::Ptr{Cvoid}, ws_bytes::Integer; finite::Ptr{Int32} = Ptr{Int32}(C_NULL), first_instance = 0, stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:cclqr_rollout_quantiles, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32, Int64, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
                h.ptr, c.ptr, n, steps, k0, first_instance, traj, length(prob), prob, quant, finite, ws, ws_bytes, stream))
end

const JOINTS_RAW = Int32(0)
const JOINTS_CONTINUOUS = Int32(1)

"The joint coordinates of the slab a rollout_dev! launch has just written (cclqr_rollout_joints; device pointers, asynchronous on `stream`): theta and rate are
 ne x out_steps x n -- per instance, absolute step and joint (the caller's joint order) the minimal coordinate of pid.jl:43-57 and the relative joint velocity of
 trackingLQR_triple_cartpole.jl:98-101; columns k0 : k0 + steps - 1 are written, so the chunks of a horizon fill one series.  mode JOINTS_CONTINUOUS makes a
 revolute's angle continuous in time; carry (2 x ne x n: w_prev, turns) then travels from launch to launch.  p: a PlantsHandle or nothing."
function rollout_joints!(h::MechHandle, p, n::Integer, steps::Integer, k0::Integer, traj::Ptr{Float64}, mode::Integer, out_steps::Integer, theta::Ptr{Float64};
                         rate::Ptr{Float64} = Ptr{Float64}(C_NULL), carry::Ptr{Float64} = Ptr{Float64}(C_NULL), first_instance = 0, stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:cclqr_rollout_joints, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32, Int64, Ptr{Float64}, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                h.ptr, p === nothing ? C_NULL : p.ptr, n, steps, k0, first_instance, traj, mode, out_steps, theta, rate, carry, stream))
end

const INVARIANTS_LEN = 6
const INVARIANTS_SUMMARY_LEN = 8

"The integrator's invariants of the slab a rollout_dev! launch has just written (cclqr_rollout_invariants; device pointers, asynchronous on `stream`): inv is
 6 x out_steps x n -- per instance and absolute step T, V, E = T + V, the largest translational and the largest rotational constraint residual over all joints and
 the largest |q.q - 1| over the bodies --, rows 5 x ne x out_steps x n the constraint rows themselves (the caller's joint order), summary 8 x n per instance
 (E at the first finite row, min E, max E, max gap, its step, max twist, max quat, rows that are not finite), which is read when k0 > 1 and so travels from launch
 to launch.  Columns k0 : k0 + steps - 1 are written; any of the three may be C_NULL, not all.  p: a PlantsHandle or nothing."
function rollout_invariants!(h::MechHandle, p, n::Integer, steps::Integer, k0::Integer, traj::Ptr{Float64}, out_steps::Integer;
                             inv::Ptr{Float64} = Ptr{Float64}(C_NULL), rows::Ptr{Float64} = Ptr{Float64}(C_NULL), summary::Ptr{Float64} = Ptr{Float64}(C_NULL),
                             first_instance = 0, stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:cclqr_rollout_invariants, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                h.ptr, p === nothing ? C_NULL : p.ptr, n, steps, k0, first_instance, traj, out_steps, inv, rows, summary, stream))
end

"Bytes of device workspace one series_ensemble! call of these sizes needs (cclqr_series_ensemble_ws_bytes)."
function series_ensemble_ws_bytes(n::Integer, steps::Integer, nc::Integer)
    out = Ref{Csize_t}(0)
    check(ccall((:cclqr_series_ensemble_ws_bytes, lib), Cint, (Int64, Int32, Int32, Ref{Csize_t}), n, steps, nc, out))
    Int(out[])
end

"The mean and the centred sum of squares of every coordinate of a series x (nc x steps x n, device) ACROSS its instances, per step (cclqr_series_ensemble): mean and
 m2 are nc x steps.  One fixed summation order, no atomics."
function series_ensemble!(n::Integer, steps::Integer, nc::Integer, x::Ptr{Float64}, mean::Ptr{Float64}, m2::Ptr{Float64}, ws::Ptr{Cvoid}, ws_bytes::Integer;
                          stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:cclqr_series_ensemble, lib), Cint, (Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
                n, steps, nc, x, mean, m2, ws, ws_bytes, stream))
end

"(min_bytes, full_bytes) of device workspace for series_quantiles! (cclqr_series_quantiles_ws_bytes): one row of the series, all `steps` rows."
function series_quantiles_ws_bytes(n::Integer, steps::Integer, nc::Integer)
    lo = Ref{Csize_t}(0); full = Ref{Csize_t}(0)
    check(ccall((:cclqr_series_quantiles_ws_bytes, lib), Cint, (Int64, Int32, Int32, Ref{Csize_t}, Ref{Csize_t}), n, steps, nc, lo, full))
    Int(lo[]), Int(full[])
end

"The quantiles of every coordinate of a series x (nc x steps x n, device) ACROSS its instances, per step (cclqr_series_quantiles): quant is nc x length(prob) x
 steps, finite nc x steps the number of finite values (or C_NULL).  At most 16384 instances and 16 probabilities."
function series_quantiles!(n::Integer, steps::Integer, nc::Integer, x::Ptr{Float64}, prob::Vector{Float64}, quant::Ptr{Float64}, ws::Ptr{Cvoid}, ws_bytes::Integer;
                           finite::Ptr{Int32} = Ptr{Int32}(C_NULL), stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:cclqr_series_quantiles, lib), Cint, (Int64, Int32, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
                n, steps, nc, x, length(prob), prob, quant, finite, ws, ws_bytes, stream))
end

"dlqr_weights that also returns the cost-to-go (cclqr_riccati_value): P[p] is the Pkp1 of lqr.jl:170 at the last backward step problem p executed (the step the
 break test of lqr.jl:172 fired on, else step 1; Q_p when N = 1), mx x mx as the recursion holds it.  Returns (Ku[p][k][i], P[p], kbreak[p])."
function dlqr_value(As::Vector, Bus::Vector, Bλs::Vector, Gs::Vector, Qs::Vector, Rs::Vector, N::Integer; tol = 1e-5)
    np = length(As); mx, mu, ml = size(As[1], 1), size(Bus[1], 2), size(Bλs[1], 2)
    length(Qs) == length(Rs) || throw(AssertionError("Qs and Rs must hold the same number of weight pairs"))
    rowmajor(Ms) = reduce(vcat, [vec(permutedims(Matrix{Float64}(M))) for M in Ms]; init = Float64[])
    K = zeros(mx * mu * max(N - 1, 0) * np); P = zeros(mx * mx * np); kb = zeros(Int32, np)
    check(ccall((:cclqr_riccati_value, lib), Cint,
                (Int32, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Int32,
                 Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}),
                np, mx, mu, ml, rowmajor(As), rowmajor(Bus), rowmajor(Bλs), rowmajor(Gs), Int32(length(Qs)), rowmajor(Qs), rowmajor(Rs), N, tol, Int32(0), K, P, kb, C_NULL))
    K4 = reshape(K, mx, mu, max(N - 1, 0), np)                       # C layout [np][N-1][mu][mx]
    P3 = reshape(P, mx, mx, np)                                      # C layout [np][mx][mx]: row-major, so transposed here
    [[[reshape(K4[:, i, k, p], 1, mx) for i = 1:mu] for k = 1:N-1] for p = 1:np], [permutedims(P3[:, :, p]) for p = 1:np], Int.(kb)
end

"The cost-to-go tables of a controller on the device (cclqr_value_create: P is 12Nb x 12Nb x n_tables, table t TRANSPOSED into Julia's column-major order, i.e.
 P[:, :, t] = P_t'; or the handle lqr_batch_value returns)."
mutable struct ValueHandle
    ptr::Ptr{Cvoid}
    mech::MechHandle
end
function value_create(h::MechHandle, P::Array{Float64,3})
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:cclqr_value_create, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{Ptr{Cvoid}}), h.ptr, size(P, 3), P, out))
    obj = ValueHandle(out[], h)
    finalizer(o -> ccall((:cclqr_value_destroy, lib), Cint, (Ptr{Cvoid},), o.ptr), obj)
    obj
end
"table `table` (0-based) of a ValueHandle read back (cclqr_value_get), as the matrix P of lqr.jl:170"
function value_get(v::ValueHandle, table::Integer, mx::Integer)
    P = zeros(mx, mx)
    check(ccall((:cclqr_value_get, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), v.ptr, table, P))
    permutedims(P)
end
"lqr_batch_weights that also keeps every table's cost-to-go on the device (cclqr_ctrl_create_lqr_batch_value).  Returns (controller pointer, kbreak, ValueHandle)."
function lqr_batch_value(h::MechHandle, p::Union{PlantsHandle,Nothing}, n::Int, zd::Array{Float64}, ctrl_joint::Vector{Int32}, n_weights::Int, Q::Vector{Float64},
                         R::Vector{Float64}, N::Int; Fd = nothing, first_plant = 0, tol = 1e-5, infinite_horizon = false)
    out = Ref{Ptr{Cvoid}}(C_NULL); val = Ref{Ptr{Cvoid}}(C_NULL); kb = zeros(Int32, n)
    fd = Fd === nothing ? Ptr{Float64}(C_NULL) : pointer(Fd)
    GC.@preserve Fd check(ccall((:cclqr_ctrl_create_lqr_batch_value, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Float64, Ptr{Int32},
                 Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}),
                h.ptr, p === nothing ? C_NULL : p.ptr, first_plant, Int32(n), zd, Int32(length(ctrl_joint)), ctrl_joint, fd, Int32(n_weights), Q, R, Int32(N),
                Int32(infinite_horizon ? 1 : 0), tol, kb, out, val))
    obj = ValueHandle(val[], h)
    finalizer(o -> ccall((:cclqr_value_destroy, lib), Cint, (Ptr{Cvoid},), o.ptr), obj)
    return out[], kb, obj
end
"V_i = Δz_i' P_t Δz_i for n states on the device (cclqr_value_eval; device pointers, asynchronous on `stream`): state i at z + 8 i z_stride bytes (z_stride >= 13 Nb
 doubles), the error of lqr.jl:92-103 about setpoint row 1 of controller table first_instance + i."
function value_eval!(h::MechHandle, c::CtrlHandle, v::ValueHandle, n::Integer, z::Ptr{Float64}, out::Ptr{Float64}; first_instance = 0, z_stride = 13 * h.nb,
                     stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:cclqr_value_eval, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Cvoid}),
                h.ptr, c.ptr, v.ptr, n, first_instance, z, z_stride, out, stream))
end

"Policy evaluation (cclqr_policy_value): dlqr's cost recursion (lqr.jl:147-177) with the gains GIVEN in place of lqr.jl:160 -- what the table Ks costs on the models
 (As, Bus, Bλs, Gs), which need not be the model it was designed on.  Ks: one table (a Vector of N-1 or 1 gains, each mu x mx) shared by all problems, or a Vector of
 such tables, one per problem; Qs, Rs: one pair or one per problem.  Returns (P[p], kbreak[p], dnorm[p] = (norm(Pk - Pkp1) of the last executed step, of the step before
 it; NaN where no such step ran)).  The evaluation converged iff dnorm[p][1] < tol; a recursion that does not is the answer, not an error."
function policy_value(As::Vector, Bus::Vector, Bλs::Vector, Gs::Vector, Ks::Vector, Qs::Vector, Rs::Vector, N::Integer; tol = 1e-5, path = 0)
    np = length(As); mx, mu, ml = size(As[1], 1), size(Bus[1], 2), size(Bλs[1], 2)
    length(Qs) == length(Rs) || throw(AssertionError("Qs and Rs must hold the same number of weight pairs"))
    tables = (isempty(Ks) || Ks[1] isa AbstractMatrix) ? [Ks] : Ks
    nK = length(tables[1])
    rowmajor(Ms) = reduce(vcat, [vec(permutedims(Matrix{Float64}(M))) for M in Ms]; init = Float64[])
    K = reduce(vcat, [rowmajor(t) for t in tables]; init = Float64[])
    P = zeros(mx * mx * np); kb = zeros(Int32, np); dn = zeros(2 * np)
    opts = Int32[path, 0, 0, 0]                                      # cclqr_riccati_opts: only `path` is read
    check(ccall((:cclqr_policy_value, lib), Cint,
                (Int32, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32,
                 Float64, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}),
                np, mx, mu, ml, rowmajor(As), rowmajor(Bus), rowmajor(Bλs), rowmajor(Gs), Int32(length(tables)), Int32(nK), K, Int32(length(Qs)), rowmajor(Qs), rowmajor(Rs),
                N, tol, P, kb, dn, opts))
    P3 = reshape(P, mx, mx, np)                                      # C layout [np][mx][mx]: row-major, so transposed here
    [permutedims(P3[:, :, p]) for p = 1:np], Int.(kb), [(dn[2p - 1], dn[2p]) for p = 1:np]
end
"The policy evaluation of controller `c` on a mechanism's plants (cclqr_value_create_policy): linearsystem (lqr.jl:63) at the n setpoints zd (13 x Nb x n), setpoint k on
 plant first_plant + k (p === nothing: the mechanism's own plant), the controller's gains gathered on the device (one table shared by all models, or table k for model
 k), the recursion of lqr.jl:147-177 with lqr.jl:160 given.  Q, R: n_weights (1 or n) row-major pairs, Δt-scaled.  Returns (ValueHandle of n tables for value_eval! /
 value_get, kbreak, dnorm 2 x n)."
function value_create_policy(h::MechHandle, p::Union{PlantsHandle,Nothing}, n::Int, zd::Array{Float64}, ctrl_joint::Vector{Int32}, c::CtrlHandle, n_weights::Int,
                             Q::Vector{Float64}, R::Vector{Float64}, N::Int; Fd = nothing, first_plant = 0, tol = 1e-5)
    val = Ref{Ptr{Cvoid}}(C_NULL); kb = zeros(Int32, n); dn = zeros(2, n)
    fd = Fd === nothing ? Ptr{Float64}(C_NULL) : pointer(Fd)
    GC.@preserve Fd check(ccall((:cclqr_value_create_policy, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Ptr{Int32},
                 Ptr{Float64}, Ref{Ptr{Cvoid}}),
                h.ptr, p === nothing ? C_NULL : p.ptr, first_plant, Int32(n), zd, Int32(length(ctrl_joint)), ctrl_joint, fd, c.ptr, Int32(n_weights), Q, R, Int32(N), tol, kb,
                dn, val))
    obj = ValueHandle(val[], h)
    finalizer(o -> ccall((:cclqr_value_destroy, lib), Cint, (Ptr{Cvoid},), o.ptr), obj)
    return obj, kb, dn
end

"A STATIONARY gain's cost-to-go by doubling (cclqr_policy_value_doubling): the one gain of LQR{T,Inf} (lqr.jl:40-43) makes Abar (lqr.jl:169) and Qbar = Q + K'RK
 (lqr.jl:170) constant, and S(a+b) = S(a) + M(a)' S(b) M(a) reaches N - 1 steps in at most 2 log2 N combinations.  Ks: one gain (mu x mx) per problem, or a Vector of
 one shared by all; N >= 1: that horizon exactly (what policy_value gives for a one-row table and tol = 0); N == 0: level by level to convergence.  Returns (P[p],
 levels[p], reason[p] (0 converged, 1 max_levels, 2 norm(M) > 1e50), dnorm[p], gnorm[p]: the increment norms and norm(M) of the last level and the one before)."
function policy_value_doubling(As::Vector, Bus::Vector, Bλs::Vector, Gs::Vector, Ks::Vector, Qs::Vector, Rs::Vector, N::Integer; tol = 1e-5, max_levels = 40, path = 0)
    np = length(As); mx, mu, ml = size(As[1], 1), size(Bus[1], 2), size(Bλs[1], 2)
    length(Qs) == length(Rs) || throw(AssertionError("Qs and Rs must hold the same number of weight pairs"))
    rowmajor(Ms) = reduce(vcat, [vec(permutedims(Matrix{Float64}(M))) for M in Ms]; init = Float64[])
    P = zeros(mx * mx * np); lv = zeros(Int32, np); rs = zeros(Int32, np); dn = zeros(2 * np); gn = zeros(2 * np)
    opts = Int32[path, 0, 0, 0]                                      # cclqr_riccati_opts: only `path` is read
    check(ccall((:cclqr_policy_value_doubling, lib), Cint,
                (Int32, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32,
                 Float64, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                np, mx, mu, ml, rowmajor(As), rowmajor(Bus), rowmajor(Bλs), rowmajor(Gs), Int32(length(Ks)), rowmajor(Ks), Int32(length(Qs)), rowmajor(Qs), rowmajor(Rs),
                N, tol, Int32(max_levels), P, lv, rs, dn, gn, opts))
    P3 = reshape(P, mx, mx, np)                                      # C layout [np][mx][mx]: row-major, so transposed here
    [permutedims(P3[:, :, p]) for p = 1:np], Int.(lv), Int.(rs), [(dn[2p - 1], dn[2p]) for p = 1:np], [(gn[2p - 1], gn[2p]) for p = 1:np]
end
"The doubling evaluation of controller `c`'s stationary gain on a mechanism's plants (cclqr_value_create_policy_doubling): linearisation and gain gather as
 value_create_policy, then lqr.jl:169-170 by doubling.  N >= 1 knots, or 0 = to convergence.  Returns (ValueHandle of n tables, levels, reason, dnorm 2 x n, gnorm 2 x n)."
function value_create_policy_doubling(h::MechHandle, p::Union{PlantsHandle,Nothing}, n::Int, zd::Array{Float64}, ctrl_joint::Vector{Int32}, c::CtrlHandle, n_weights::Int,
                                      Q::Vector{Float64}, R::Vector{Float64}, N::Int; Fd = nothing, first_plant = 0, tol = 1e-5, max_levels = 40)
    val = Ref{Ptr{Cvoid}}(C_NULL); lv = zeros(Int32, n); rs = zeros(Int32, n); dn = zeros(2, n); gn = zeros(2, n)
    fd = Fd === nothing ? Ptr{Float64}(C_NULL) : pointer(Fd)
    GC.@preserve Fd check(ccall((:cclqr_value_create_policy_doubling, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Int32,
                 Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ref{Ptr{Cvoid}}),
                h.ptr, p === nothing ? C_NULL : p.ptr, first_plant, Int32(n), zd, Int32(length(ctrl_joint)), ctrl_joint, fd, c.ptr, Int32(n_weights), Q, R, Int32(N), tol,
                Int32(max_levels), lv, rs, dn, gn, val))
    obj = ValueHandle(val[], h)
    finalizer(o -> ccall((:cclqr_value_destroy, lib), Cint, (Ptr{Cvoid},), o.ptr), obj)
    return obj, lv, rs, dn, gn
end

"The closed-loop state covariance of ONE stationary gain under input noise, by doubling (cclqr_covariance_doubling): with Abar = A' - D K (lqr.jl:169) and w ~ (0, Wu)
 on the inputs (the noise of trackingLQR_triple_cartpole.jl:98), Σ_n = C(n) + M(n) Σ0 M(n)' by the pair recursion of policy_value_doubling on (Abar', D Wu D').
 Wus (mu x mu) and Σ0s (mx x mx): one per problem or one shared; either may be empty (= 0), not both.  N >= 1: N - 1 steps exactly; N == 0: the steady state (Σ0s
 empty).  Returns (Σ[p], cost[p] = (tr(QΣ), tr(R KΣK')), zstd[p], ustd[p], levels[p], reason[p], dnorm[p], gnorm[p])."
function covariance_doubling(As::Vector, Bus::Vector, Bλs::Vector, Gs::Vector, Ks::Vector, Qs::Vector, Rs::Vector, Wus::Vector, Σ0s::Vector, N::Integer;
                             tol = 1e-8, max_levels = 40, path = 0)
    np = length(As); mx, mu, ml = size(As[1], 1), size(Bus[1], 2), size(Bλs[1], 2)
    length(Qs) == length(Rs) || throw(AssertionError("Qs and Rs must hold the same number of weight pairs"))
    (isempty(Wus) || isempty(Σ0s) || length(Wus) == length(Σ0s)) || throw(AssertionError("Wus and Σ0s must hold the same number of matrices"))
    rowmajor(Ms) = reduce(vcat, [vec(permutedims(Matrix{Float64}(M))) for M in Ms]; init = Float64[])
    Σ = zeros(mx * mx * np); cost = zeros(2 * np); zs = zeros(mx * np); us = zeros(max(mu * np, 1))
    lv = zeros(Int32, np); rs = zeros(Int32, np); dn = zeros(2 * np); gn = zeros(2 * np)
    opts = Int32[path, 0, 0, 0]                                      # cclqr_riccati_opts: only `path` is read
    wu = rowmajor(Wus); s0 = rowmajor(Σ0s)
    GC.@preserve wu s0 check(ccall((:cclqr_covariance_doubling, lib), Cint,
                (Int32, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32,
                 Ptr{Float64}, Ptr{Float64}, Int32, Float64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Int32}),
                np, mx, mu, ml, rowmajor(As), rowmajor(Bus), rowmajor(Bλs), rowmajor(Gs), Int32(length(Ks)), rowmajor(Ks), Int32(length(Qs)), rowmajor(Qs), rowmajor(Rs),
                Int32(max(length(Wus), length(Σ0s))), isempty(Wus) ? Ptr{Float64}(C_NULL) : pointer(wu), isempty(Σ0s) ? Ptr{Float64}(C_NULL) : pointer(s0),
                N, tol, Int32(max_levels), Σ, cost, zs, us, lv, rs, dn, gn, opts))
    Σ3 = reshape(Σ, mx, mx, np)                                      # C layout [np][mx][mx]: row-major, so transposed here
    [permutedims(Σ3[:, :, p]) for p = 1:np], [(cost[2p - 1], cost[2p]) for p = 1:np], [zs[(p - 1) * mx + 1:p * mx] for p = 1:np],
        [us[(p - 1) * mu + 1:p * mu] for p = 1:np], Int.(lv), Int.(rs), [(dn[2p - 1], dn[2p]) for p = 1:np], [(gn[2p - 1], gn[2p]) for p = 1:np]
end
"The covariance above for controller `c`'s stationary gain on a mechanism's plants (cclqr_value_create_covariance_doubling): linearisation and gain gather as
 value_create_policy_doubling.  Wu (n_noise mu x mu blocks, row-major) and Σ0 (n_noise mx x mx) flat, or nothing.  Returns (ValueHandle of n tables holding Σ, cost 2 x n,
 zstd mx x n, ustd mu x n, levels, reason, dnorm 2 x n, gnorm 2 x n)."
function value_create_covariance_doubling(h::MechHandle, p::Union{PlantsHandle,Nothing}, n::Int, zd::Array{Float64}, ctrl_joint::Vector{Int32}, c::CtrlHandle,
                                          n_weights::Int, Q::Vector{Float64}, R::Vector{Float64}, n_noise::Int, Wu, Σ0, N::Int, mx::Int;
                                          Fd = nothing, first_plant = 0, tol = 1e-8, max_levels = 40)
    mu = length(ctrl_joint)
    val = Ref{Ptr{Cvoid}}(C_NULL); lv = zeros(Int32, n); rs = zeros(Int32, n); dn = zeros(2, n); gn = zeros(2, n)
    cost = zeros(2, n); zs = zeros(mx, n); us = zeros(mu, n)
    fd = Fd === nothing ? Ptr{Float64}(C_NULL) : pointer(Fd)
    wu = Wu === nothing ? Ptr{Float64}(C_NULL) : pointer(Wu)
    s0 = Σ0 === nothing ? Ptr{Float64}(C_NULL) : pointer(Σ0)
    GC.@preserve Fd Wu Σ0 check(ccall((:cclqr_value_create_covariance_doubling, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64},
                 Ptr{Float64}, Int32, Float64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ref{Ptr{Cvoid}}),
                h.ptr, p === nothing ? C_NULL : p.ptr, first_plant, Int32(n), zd, Int32(mu), ctrl_joint, fd, c.ptr, Int32(n_weights), Q, R, Int32(n_noise), wu, s0,
                Int32(N), tol, Int32(max_levels), cost, zs, us, lv, rs, dn, gn, val))
    obj = ValueHandle(val[], h)
    finalizer(o -> ccall((:cclqr_value_destroy, lib), Cint, (Ptr{Cvoid},), o.ptr), obj)
    return obj, cost, zs, us, lv, rs, dn, gn
end

"The state covariance of a TRACKED run under input noise at every knot (cclqr_covariance_tracking): Σ_{j+1} = Abar_j Σ_j Abar_j' + D_j Wu D_j' with Abar_j = A'_j - D_j K_j
 (lqr_tracking.jl:107), the model and the gain row of knot j (lqr_tracking.jl:63, 88), w ~ (0, Wu) on the inputs (trackingLQR_triple_cartpole.jl:98).  As[p], Bus[p], Bλs[p],
 Gs[p]: vectors of nlin = 1 or N - 1 matrices per problem; Ks[p]: vectors of nK = 1 or N - 1 gain rows (one table shared: length(Ks) == 1).  Wus, Σ0s: one per problem or one
 shared; either may be empty (= 0), not both.  Returns (Σ[p] = Σ_{N-1}, cost 2 x N x np, zstd mx x N x np, ustd mu x N x np, total 2 x np)."
function covariance_tracking(As::Vector, Bus::Vector, Bλs::Vector, Gs::Vector, Ks::Vector, Qs::Vector, Rs::Vector, Wus::Vector, Σ0s::Vector, N::Integer; path = 0)
    np = length(As); nlin = length(As[1])
    mx, mu, ml = size(As[1][1], 1), size(Bus[1][1], 2), size(Bλs[1][1], 2)
    nK = (mu == 0 || isempty(Ks)) ? 1 : length(Ks[1])                # no inputs: no gains, Ks may be empty
    length(Qs) == length(Rs) || throw(AssertionError("Qs and Rs must hold the same number of weight pairs"))
    (isempty(Wus) || isempty(Σ0s) || length(Wus) == length(Σ0s)) || throw(AssertionError("Wus and Σ0s must hold the same number of matrices"))
    rowmajor(Ms) = reduce(vcat, [vec(permutedims(Matrix{Float64}(M))) for M in Ms]; init = Float64[])
    nested(Vs) = reduce(vcat, [rowmajor(V) for V in Vs]; init = Float64[])
    Σ = zeros(mx * mx * np); cost = zeros(2, N, np); zs = zeros(mx, N, np); us = zeros(max(mu, 1), N, np); tot = zeros(2, np)
    opts = Int32[path, 0, 0, 0]                                      # cclqr_riccati_opts: only `path` is read
    wu = rowmajor(Wus); s0 = rowmajor(Σ0s)
    GC.@preserve wu s0 check(ccall((:cclqr_covariance_tracking, lib), Cint,
                (Int32, Int32, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64},
                 Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                np, mx, mu, ml, nlin, nested(As), nested(Bus), nested(Bλs), nested(Gs), Int32(max(length(Ks), 1)), Int32(nK), nested(Ks), Int32(length(Qs)), rowmajor(Qs),
                rowmajor(Rs), Int32(max(length(Wus), length(Σ0s))), isempty(Wus) ? Ptr{Float64}(C_NULL) : pointer(wu), isempty(Σ0s) ? Ptr{Float64}(C_NULL) : pointer(s0),
                N, Σ, Ptr{Float64}(C_NULL), cost, zs, mu > 0 ? pointer(us) : Ptr{Float64}(C_NULL), tot, opts))
    Σ3 = reshape(Σ, mx, mx, np)                                      # C layout [np][mx][mx]: row-major, so transposed here
    [permutedims(Σ3[:, :, p]) for p = 1:np], cost, zs, us[1:mu, :, :], tot
end
"The covariance above for controller `c`'s gain rows along n trajectories on a mechanism's plants (cclqr_value_create_covariance_tracking): zd 13 x nb x N x n and Fd
 mu x N x n (or nothing) host arrays, linearised at the knots 0 .. N-2 of trajectory k on plant first_plant + k.  Wu (n_noise mu x mu blocks, row-major) and Σ0 (n_noise
 mx x mx) flat, or nothing.  Returns (ValueHandle of n tables holding Σ_{N-1}, cost 2 x N x n, zstd mx x N x n, ustd mu x N x n, total 2 x n)."
function value_create_covariance_tracking(h::MechHandle, p::Union{PlantsHandle,Nothing}, n::Int, N::Int, zd::Array{Float64}, ctrl_joint::Vector{Int32}, c::CtrlHandle,
                                          n_weights::Int, Q::Vector{Float64}, R::Vector{Float64}, n_noise::Int, Wu, Σ0, mx::Int;
                                          Fd = nothing, first_plant = 0, workspace_bytes = 0)
    mu = length(ctrl_joint)
    val = Ref{Ptr{Cvoid}}(C_NULL)
    cost = zeros(2, N, n); zs = zeros(mx, N, n); us = zeros(mu, N, n); tot = zeros(2, n)
    fd = Fd === nothing ? Ptr{Float64}(C_NULL) : pointer(Fd)
    wu = Wu === nothing ? Ptr{Float64}(C_NULL) : pointer(Wu)
    s0 = Σ0 === nothing ? Ptr{Float64}(C_NULL) : pointer(Σ0)
    GC.@preserve Fd Wu Σ0 check(ccall((:cclqr_value_create_covariance_tracking, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Int32}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Int32,
                 Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
                h.ptr, p === nothing ? C_NULL : p.ptr, first_plant, Int32(n), Int32(N), zd, fd, Int32(0), Int32(mu), ctrl_joint, c.ptr, Int32(n_weights), Q, R,
                Int32(n_noise), wu, s0, Int64(workspace_bytes), cost, zs, us, tot, C_NULL, val))
    obj = ValueHandle(val[], h)
    finalizer(o -> ccall((:cclqr_value_destroy, lib), Cint, (Ptr{Cvoid},), o.ptr), obj)
    return obj, cost, zs, us, tot
end

"The cost-to-go of a TRACKED run at every knot and the price of its noise (cclqr_policy_value_tracking): P_{N-1} = Q, P_j = Q + K_j' R K_j + Abar_j' P_{j+1} Abar_j
 (lqr_tracking.jl:107-108 with the gain row of knot j given, lqr_tracking.jl:63, 88), price_j = tr(Wu D_j' P_{j+1} D_j) for w ~ (0, Wu) on the inputs
 (trackingLQR_triple_cartpole.jl:98).  Models, gains and weights as covariance_tracking takes them; Wus: one per problem, one shared, or empty (no price).
 Returns (P[p] = P_0, price N x np, noise_total np)."
function policy_value_tracking(As::Vector, Bus::Vector, Bλs::Vector, Gs::Vector, Ks::Vector, Qs::Vector, Rs::Vector, Wus::Vector, N::Integer; path = 0)
    np = length(As); nlin = length(As[1])
    mx, mu, ml = size(As[1][1], 1), size(Bus[1][1], 2), size(Bλs[1][1], 2)
    nK = (mu == 0 || isempty(Ks)) ? 1 : length(Ks[1])                # no inputs: no gains, Ks may be empty
    length(Qs) == length(Rs) || throw(AssertionError("Qs and Rs must hold the same number of weight pairs"))
    rowmajor(Ms) = reduce(vcat, [vec(permutedims(Matrix{Float64}(M))) for M in Ms]; init = Float64[])
    nested(Vs) = reduce(vcat, [rowmajor(V) for V in Vs]; init = Float64[])
    P = zeros(mx * mx * np); price = zeros(N, np); tot = zeros(np)
    opts = Int32[path, 0, 0, 0]                                      # cclqr_riccati_opts: only `path` is read
    wu = rowmajor(Wus)
    priced = !isempty(Wus)
    GC.@preserve wu price tot check(ccall((:cclqr_policy_value_tracking, lib), Cint,
                (Int32, Int32, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64},
                 Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                np, mx, mu, ml, nlin, nested(As), nested(Bus), nested(Bλs), nested(Gs), Int32(max(length(Ks), 1)), Int32(nK), nested(Ks), Int32(length(Qs)), rowmajor(Qs),
                rowmajor(Rs), Int32(max(length(Wus), 1)), priced ? pointer(wu) : Ptr{Float64}(C_NULL), N, P, Ptr{Float64}(C_NULL),
                priced ? pointer(price) : Ptr{Float64}(C_NULL), priced ? pointer(tot) : Ptr{Float64}(C_NULL), opts))
    P3 = reshape(P, mx, mx, np)                                      # C layout [np][mx][mx]: row-major, so transposed here
    [permutedims(P3[:, :, p]) for p = 1:np], price, tot
end
"The cost-to-go above for controller `c`'s gain rows along n trajectories on a mechanism's plants, down to `knot` (0-based, cclqr_value_create_policy_tracking): zd, Fd,
 Q, R, Wu as value_create_covariance_tracking takes them (Wu nothing: no price).  Returns (ValueHandle of n tables holding P_knot, price N x n, noise_total n)."
function value_create_policy_tracking(h::MechHandle, p::Union{PlantsHandle,Nothing}, n::Int, N::Int, zd::Array{Float64}, ctrl_joint::Vector{Int32}, c::CtrlHandle,
                                      n_weights::Int, Q::Vector{Float64}, R::Vector{Float64}, n_noise::Int, Wu;
                                      Fd = nothing, first_plant = 0, knot = 0, workspace_bytes = 0)
    mu = length(ctrl_joint)
    val = Ref{Ptr{Cvoid}}(C_NULL)
    price = zeros(N, n); tot = zeros(n)
    fd = Fd === nothing ? Ptr{Float64}(C_NULL) : pointer(Fd)
    wu = Wu === nothing ? Ptr{Float64}(C_NULL) : pointer(Wu)
    GC.@preserve Fd Wu price tot check(ccall((:cclqr_value_create_policy_tracking, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Int32}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Int32,
                 Ptr{Float64}, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
                h.ptr, p === nothing ? C_NULL : p.ptr, first_plant, Int32(n), Int32(N), zd, fd, Int32(0), Int32(mu), ctrl_joint, c.ptr, Int32(n_weights), Q, R,
                Int32(n_noise), wu, Int32(knot), Int64(workspace_bytes), Wu === nothing ? Ptr{Float64}(C_NULL) : pointer(price),
                Wu === nothing ? Ptr{Float64}(C_NULL) : pointer(tot), C_NULL, val))
    obj = ValueHandle(val[], h)
    finalizer(o -> ccall((:cclqr_value_destroy, lib), Cint, (Ptr{Cvoid},), o.ptr), obj)
    return obj, price, tot
end

"The stationary LQR gain by doubling the Riccati map (cclqr_riccati_doubling): n backward steps of dlqr (lqr.jl:141-184) are a triple (A_n, G_n, H_n), two triples compose
 in one pivoted solve and five products, and the one gain LQR{T,Inf} keeps (lqr.jl:25-27, 39-43) is reached in log2 n compositions.  Qs, Rs: one exactly symmetric pair,
 or one per problem.  N >= 2: Ku[1] and the last Pkp1 of dlqr(.., N) with tol = 0; N == 0: level by level to convergence.  Returns (K[p], P[p], levels[p], reason[p]
 (0 converged, 1 max_levels, 2 norm(A) > 1e50 or not finite, 3 pivot), dnorm[p], anorm[p]: the increment norms and norm(A) of the last level and the one before)."
function riccati_doubling(As::Vector, Bus::Vector, Bλs::Vector, Gs::Vector, Qs::Vector, Rs::Vector, N::Integer; tol = 1e-5, max_levels = 40)
    np = length(As); mx, mu, ml = size(As[1], 1), size(Bus[1], 2), size(Bλs[1], 2)
    length(Qs) == length(Rs) || throw(AssertionError("Qs and Rs must hold the same number of weight pairs"))
    rowmajor(Ms) = reduce(vcat, [vec(permutedims(Matrix{Float64}(M))) for M in Ms]; init = Float64[])
    K = zeros(mu * mx * np); P = zeros(mx * mx * np); lv = zeros(Int32, np); rs = zeros(Int32, np); dn = zeros(2 * np); an = zeros(2 * np)
    opts = Int32[0, 0, 1, 0]                                         # cclqr_riccati_opts: only bf16_terms is looked at
    check(ccall((:cclqr_riccati_doubling, lib), Cint,
                (Int32, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Int32,
                 Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                np, mx, mu, ml, rowmajor(As), rowmajor(Bus), rowmajor(Bλs), rowmajor(Gs), Int32(length(Qs)), rowmajor(Qs), rowmajor(Rs), N, tol, Int32(max_levels),
                K, P, lv, rs, dn, an, opts))
    K3 = reshape(K, mx, mu, np); P3 = reshape(P, mx, mx, np)         # C layouts [np][mu][mx], [np][mx][mx]: row-major, so transposed here
    [permutedims(K3[:, :, p]) for p = 1:np], [permutedims(P3[:, :, p]) for p = 1:np], Int.(lv), Int.(rs), [(dn[2p - 1], dn[2p]) for p = 1:np],
        [(an[2p - 1], an[2p]) for p = 1:np]
end
"lqr_batch_value with infinite_horizon and the gain by the doubling above (cclqr_ctrl_create_lqr_batch_doubling): one gain row per table, gains and P device-resident.
 N >= 2 knots, or 0 = to convergence.  Returns (controller pointer, ValueHandle, levels, reason, dnorm 2 x n, anorm 2 x n)."
function lqr_batch_doubling(h::MechHandle, p::Union{PlantsHandle,Nothing}, n::Int, zd::Array{Float64}, ctrl_joint::Vector{Int32}, n_weights::Int, Q::Vector{Float64},
                            R::Vector{Float64}, N::Int; Fd = nothing, first_plant = 0, tol = 1e-5, max_levels = 40)
    out = Ref{Ptr{Cvoid}}(C_NULL); val = Ref{Ptr{Cvoid}}(C_NULL); lv = zeros(Int32, n); rs = zeros(Int32, n); dn = zeros(2, n); an = zeros(2, n)
    fd = Fd === nothing ? Ptr{Float64}(C_NULL) : pointer(Fd)
    GC.@preserve Fd check(ccall((:cclqr_ctrl_create_lqr_batch_doubling, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Int32,
                 Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}),
                h.ptr, p === nothing ? C_NULL : p.ptr, first_plant, Int32(n), zd, Int32(length(ctrl_joint)), ctrl_joint, fd, Int32(n_weights), Q, R, Int32(N), tol,
                Int32(max_levels), lv, rs, dn, an, out, val))
    obj = ValueHandle(val[], h)
    finalizer(o -> ccall((:cclqr_value_destroy, lib), Cint, (Ptr{Cvoid},), o.ptr), obj)
    return out[], obj, lv, rs, dn, an
end

"Size the controller handle's Philox workspace before step-per-launch rollouts are captured into a hipGraph (cclqr_ctrl_reserve_noise)."
reserve_noise!(c::CtrlHandle, n::Integer, steps::Integer) = check(ccall((:cclqr_ctrl_reserve_noise, lib), Cint, (Ptr{Cvoid}, Int64, Int32), c.ptr, n, steps))

"The `controlfunction` hook (lqr.jl:14, :56) with the closure on the host: U (mu x nsp x n_ctrl, as given to CtrlHandle) are the joint inputs the
closure computed for the next single-step launch (cclqr_ctrl_set_feedforward; host array, copied synchronously).  Step the batch with
`rollout_dev!(...; flags = ROLLOUT_CARRY_STATUS)` and a zeroed status array: an instance lost in an earlier launch then stays frozen, as in one launch over the horizon."
set_feedforward!(c::CtrlHandle, U::Array{Float64}) =
    check(ccall((:cclqr_ctrl_set_feedforward, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int32, Ptr{Cvoid}), c.ptr, U, length(U), 0, C_NULL))

"Storage{T}(steps, Nb) view of instance n of a batched trajectory: storage.x[i][k] etc. (lqr_tracking.jl:32-35)."
function storage_fields(traj::Array{Float64,4}, n::Integer)
    nb, steps = size(traj, 2), size(traj, 3)
    x = [[traj[1:3, i, k, n] for k = 1:steps] for i = 1:nb]
    q = [[traj[4:7, i, k, n] for k = 1:steps] for i = 1:nb]
    v = [[traj[8:10, i, k, n] for k = 1:steps] for i = 1:nb]
    ω = [[traj[11:13, i, k, n] for k = 1:steps] for i = 1:nb]
    (; x, q, v, ω)
end

end # module
